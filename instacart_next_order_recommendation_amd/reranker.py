"""Reranking with a BERT cross-encoder: the second half of a sentence-transformers retrieval stack.

The bi-encoder retrieves (recommender.py: embed the context, cosine top-k over the catalog); a cross-encoder then reads
each `[CLS] query [SEP] product [SEP]` as ONE sequence and returns one relevance score per pair - what
`sentence_transformers.CrossEncoder.predict` / `.rank` do for the cross-encoder/ms-marco-MiniLM-L-*-v2 family
(BertForSequenceClassification with one label).  `predict` / `rank` assemble the pairs on the host from the two sides'
token ids (model_io.assemble_pairs) and score them in one libicrec call (icrec_score_pairs: segment ids in the embedding
kernel, the last layer on the [CLS] rows only, the pooler + classifier head kernel).  RerankedRecommender keeps the
catalog's product sides on the GPU (DeviceReranker) and goes from icrec_search's candidate rows to the final top k without
leaving the device: icrec_assemble_pairs -> icrec_score_pairs -> icrec_rerank_select on one stream, captured together with
the retrieval for one request, chunked for a batch.  No CPU or PyTorch fallback.
"""
from __future__ import annotations

from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native
from ._native import ptr, stream_ptr
from .adapter import DEFAULT_SCALE, fit_plan
from .encoder import DeviceEncoder
from .model_io import assemble_pairs, load_cross_encoder_dir, strip_specials

RERANK_TOKENS_PER_CALL = 1 << 18  # a batch is reranked in calls of at most this many (bound) tokens


def pair_token_bound(q_lens: Sequence[int], k: int, cat_max_len: int, max_len: int) -> int:
    """The most tokens the pairs of `k` candidates per query can hold, whichever catalog rows the candidates are: the sum
    over the queries of k * min(max_len, 3 + len_q + cat_max_len), len_q the query side's ids without specials and
    cat_max_len the longest product side.  What icrec_assemble_pairs wants as ids_cap."""
    return int(sum(int(k) * min(int(max_len), 3 + int(n) + int(cat_max_len)) for n in q_lens))


class CrossEncoderReranker:
    """A cross-encoder directory (model_io.load_cross_encoder_dir) resident on one GPU."""

    def __init__(self, model_dir: Path | str, gemm_mode: str = "f16x3", device: str | torch.device = "cuda:0"):
        m = load_cross_encoder_dir(model_dir)
        self.shape, self.max_seq_length, self.activation, self.tokenizer = m.shape, m.max_seq_length, m.activation, m.tokenizer
        vocab = (Path(model_dir) / "vocab.txt").read_text().split("\n")
        self.cls_id, self.sep_id = (vocab.index(self.tokenizer.specials[k]) for k in ("cls_token", "sep_token"))
        self.encoder = DeviceEncoder(m.weights, m.shape, device, gemm_mode=gemm_mode, max_seq_length=m.max_seq_length)
        self.encoder.set_score_head(m.pooler_w, m.pooler_b, m.cls_w, m.cls_b)

    def side_ids(self, texts: Sequence[str]) -> list[np.ndarray]:
        """One side's token ids per text, without [CLS] / [SEP]: what assemble_pairs takes."""
        return strip_specials(*self.tokenizer.packed(list(texts)))

    def score_ids(self, a_ids: Sequence[np.ndarray], b_ids: Sequence[np.ndarray]) -> np.ndarray:
        """Scores float32 [n] of pairs given as the two sides' token ids: assembled and truncated on the host, ONE
        score_packed call, then the model's activation (sigmoid in float32, or the raw logit)."""
        if len(a_ids) == 0:
            return np.zeros(0, np.float32)
        return self.activate(self.logit_ids(a_ids, b_ids).cpu().numpy())

    def logit_ids(self, a_ids: Sequence[np.ndarray], b_ids: Sequence[np.ndarray]) -> torch.Tensor:
        """score_ids' raw logits, float32 [n >= 1] on the device."""
        ids, cu, seg_b = assemble_pairs(a_ids, b_ids, self.max_seq_length, self.cls_id, self.sep_id)
        dev = self.encoder.device
        return self.encoder.score_packed(torch.from_numpy(ids).to(dev), torch.from_numpy(cu).to(dev),
                                         torch.from_numpy(seg_b).to(dev), int(np.diff(cu).max()))

    def activate(self, logits: np.ndarray) -> np.ndarray:
        """The model's activation on raw float32 logits: sigmoid in float32, or the logit itself."""
        if self.activation == "identity":
            return logits
        return (np.float32(1) / (np.float32(1) + np.exp(-logits, dtype=np.float32))).astype(np.float32)

    def pair_token_bound(self, q_lens: Sequence[int], k: int, cat_max_len: int) -> int:
        """pair_token_bound at this model's max_seq_length."""
        return pair_token_bound(q_lens, k, cat_max_len, self.max_seq_length)

    def predict(self, pairs: Sequence[tuple[str, str]]) -> np.ndarray:
        """CrossEncoder.predict: one score per (query, document) pair, float32 [n]."""
        return self.score_ids(self.side_ids([a for a, _ in pairs]), self.side_ids([b for _, b in pairs]))

    def rank(self, query: str, documents: Sequence[str], top_k: Optional[int] = None) -> list[tuple[int, float]]:
        """CrossEncoder.rank: (index into documents, score), best first, ties by lower index; the best top_k if given."""
        scores = self.predict([(query, d) for d in documents])
        return best_first(scores, top_k)

    def close(self) -> None:
        self.encoder.close()


def best_first(scores: np.ndarray, top_k: Optional[int] = None) -> list[tuple[int, float]]:
    """(index, score) by score descending, ties by lower index (a stable sort of the negated scores)."""
    order = np.argsort(-np.asarray(scores, np.float32), kind="stable")
    return [(int(i), float(scores[i])) for i in (order if top_k is None else order[:max(int(top_k), 0)])]


class RerankBuffers:
    """The caller-owned buffers of one DeviceReranker.rerank_into call of a fixed shape (a captured graph bakes their
    addresses): the packed pairs (ids[ids_cap], cu[n_pairs + 1], seg_b[n_pairs]), their logits, the two workspaces, and
    the results out_idx int64 / out_logit float32 [n_queries, top_k] - in pinned host memory with `pinned_out`, which the
    select kernel then writes directly (fastpath.py's way of returning a request's results without a copy node)."""

    def __init__(self, dr: "DeviceReranker", n_queries: int, k: int, top_k: int, ids_cap: int, pinned_out: bool = False,
                 out: Optional[tuple[torch.Tensor, torch.Tensor]] = None):
        L, dev, n_pairs = _native.lib(), dr.device, n_queries * k
        self.n_queries, self.k, self.top_k, self.ids_cap = n_queries, k, top_k, int(ids_cap)
        self.ids = torch.empty(self.ids_cap, dtype=torch.int32, device=dev)
        self.cu = torch.empty(n_pairs + 1, dtype=torch.int32, device=dev)
        self.seg_b = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        self.logits = torch.empty(n_pairs, dtype=torch.float32, device=dev)
        self.asm_ws = torch.empty(int(L.icrec_assemble_pairs_workspace_bytes(n_queries, k)), dtype=torch.uint8, device=dev)
        self.score_ws = torch.empty(int(L.icrec_score_pairs_workspace_bytes(dr.reranker.encoder._h, self.ids_cap, n_pairs)),
                                    dtype=torch.uint8, device=dev)
        if out is not None:
            self.out_idx, self.out_logit = out
        elif pinned_out:
            self.out_idx = torch.full((n_queries, top_k), -1, dtype=torch.int64).pin_memory()
            self.out_logit = torch.zeros((n_queries, top_k), dtype=torch.float32).pin_memory()
        else:
            self.out_idx = torch.empty((n_queries, top_k), dtype=torch.int64, device=dev)
            self.out_logit = torch.empty((n_queries, top_k), dtype=torch.float32, device=dev)


class DeviceReranker:
    """A cross-encoder plus the token store of a catalog's product sides on its GPU: cat_ids int32[total] and cat_cu
    int32[n_rows + 1], without specials, row r = index row row_offset + r; cat_max_len, the longest side, stays on the
    host (it enters the token bound).  rerank_into runs candidates -> pairs -> logits -> top k on the current stream."""

    def __init__(self, reranker: CrossEncoderReranker, product_sides: Sequence[np.ndarray], row_offset: int = 0):
        self.reranker, self.device, self.row_offset = reranker, reranker.encoder.device, int(row_offset)
        self.n_rows = len(product_sides)
        cu = np.zeros(self.n_rows + 1, np.int32)
        np.cumsum([len(s) for s in product_sides], out=cu[1:])
        ids = np.zeros(max(int(cu[-1]), 1), np.int32)  # (never an empty allocation: the ABI refuses NULL)
        if cu[-1]:
            ids[:] = np.concatenate([np.asarray(s, np.int32) for s in product_sides])
        self.cat_max_len = int(np.diff(cu).max()) if self.n_rows else 0
        self.cat_ids, self.cat_cu = torch.from_numpy(ids).to(self.device), torch.from_numpy(cu).to(self.device)

    def token_bound(self, q_lens: Sequence[int], k: int) -> int:
        return self.reranker.pair_token_bound(q_lens, k, self.cat_max_len)

    def max_pair_len(self, q_len: int) -> int:
        """The longest pair a query side of q_len ids can make: the bound's term, icrec_score_pairs' max_seqlen."""
        return min(self.reranker.max_seq_length, 3 + int(q_len) + self.cat_max_len)

    def query_side_cap(self) -> int:
        """A query side longer than this assembles to the same pairs cut to it: it is then the longer side against every
        product and the pair is over budget, and neither of the two tests reads more of its length."""
        return max(self.cat_max_len, self.reranker.max_seq_length - 3) + 1

    def rerank_into(self, q_ids: torch.Tensor, q_cu: torch.Tensor, cand_idx: torch.Tensor, max_seqlen: int,
                    b: RerankBuffers, cand_score: Optional[torch.Tensor] = None) -> None:
        """icrec_assemble_pairs -> icrec_score_pairs -> icrec_rerank_select on the current stream, nothing allocated:
        device int32 q_ids / q_cu[n_queries + 1] (query sides without specials) and int64 cand_idx [n_queries, k]
        (icrec_search's out_idx) -> b.out_idx / b.out_logit.  b.ids_cap must be at least token_bound of the query sides
        and max_seqlen at least their largest max_pair_len."""
        L, r, dev = _native.lib(), self.reranker, self.device
        n_pairs = b.n_queries * b.k
        _native.check(L.icrec_assemble_pairs(ptr(q_ids), ptr(q_cu), b.n_queries, ptr(self.cat_ids), ptr(self.cat_cu), self.n_rows,
                                             self.row_offset, ptr(cand_idx), b.k, r.max_seq_length, r.cls_id, r.sep_id,
                                             ptr(b.ids), b.ids_cap, ptr(b.cu), ptr(b.seg_b), ptr(b.asm_ws), b.asm_ws.numel(),
                                             dev.index, stream_ptr(dev)), "icrec_assemble_pairs")
        r.encoder.score_into(b.ids, b.cu, b.seg_b, n_pairs, b.ids_cap, int(max_seqlen), b.logits, b.score_ws)
        _native.check(L.icrec_rerank_select(ptr(b.logits), ptr(cand_idx), ptr(cand_score), b.n_queries, b.k, b.top_k,
                                            ptr(b.out_idx), ptr(b.out_logit), dev.index, stream_ptr(dev)), "icrec_rerank_select")


class _CapturedRequest:
    """One request - bi-encoder encode, search, assemble, score, select - as ONE captured graph per (bi-encoder token
    bucket, cross-encoder query-side bucket, candidates, top_k), built like fastpath._Captured: the kernels read both
    tokenisations and the exclusions as views of one device buffer filled by a single H2D copy, the candidates stay on
    the device, and the select kernel writes the top_k results into pinned host memory."""

    def __init__(self, owner: "RerankedRecommender", bucket: int, ce_bucket: int, k: int, top_k: int):
        from .fastpath import MAX_EXCLUDED

        rec, dr = owner.recommender, owner._device
        enc, index, dev = rec.model.encoder, rec._index, dr.device
        self.bucket, self.ce_bucket = bucket, ce_bucket
        # [cu (2) | excl_off (2) | q_cu (2) | unused (2) | ids (bucket) | q_ids (ce_bucket) | excl_idx (MAX_EXCLUDED)]
        self.h_in = torch.zeros(8 + bucket + ce_bucket + MAX_EXCLUDED, dtype=torch.int32).pin_memory()
        self.d_in = torch.zeros_like(self.h_in, device=dev)
        cu, excl_off, q_cu = self.d_in[0:2], self.d_in[2:4], self.d_in[4:6]
        ids, q_ids = self.d_in[8:8 + bucket], self.d_in[8 + bucket:8 + bucket + ce_bucket]
        excl_idx = self.d_in[8 + bucket + ce_bucket:]
        emb = torch.empty((1, enc.shape.hidden), dtype=torch.float32, device=dev)
        cand_idx = torch.empty((1, k), dtype=torch.int64, device=dev)
        cand_sc = torch.empty((1, k), dtype=torch.float32, device=dev)
        self.bufs = RerankBuffers(dr, 1, k, top_k, dr.token_bound([ce_bucket], k), pinned_out=True)
        L = _native.lib()
        enc_ws = torch.empty(int(L.icrec_encode_workspace_bytes(enc._h, bucket, 1)), dtype=torch.uint8, device=dev)
        srch_ws = torch.empty(int(L.icrec_search_workspace_bytes(index._h, 1, k)), dtype=torch.uint8, device=dev)
        max_seqlen = dr.max_pair_len(ce_bucket)

        def body():
            enc.encode_into(ids, cu, 1, bucket, bucket, emb, enc_ws)
            index.search_into(emb, k, excl_idx, excl_off, cand_idx, cand_sc, srch_ws)
            dr.rerank_into(q_ids, q_cu, cand_idx, max_seqlen, self.bufs, cand_sc)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up: function attributes
            for _ in range(2):
                body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self._keep = (emb, cand_idx, cand_sc, enc_ws, srch_ws)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            body()

    def run(self, ids: np.ndarray, q_side: np.ndarray, excluded_rows: Sequence[int]):
        """-> (row indices int64 [top_k], logits float32 [top_k]) on the host, -1 / 0 padded."""
        h, n, nq, o = self.h_in, len(ids), len(q_side), 8 + self.bucket
        ex = sorted(set(int(r) for r in excluded_rows))
        h[0:8] = torch.tensor([0, n, 0, len(ex), 0, nq, 0, 0], dtype=torch.int32)
        h[8:8 + n] = torch.as_tensor(ids, dtype=torch.int32)
        h[8 + n:o] = 0
        h[o:o + nq] = torch.as_tensor(q_side, dtype=torch.int32)
        h[o + nq:o + self.ce_bucket] = 0
        if ex:
            h[o + self.ce_bucket:o + self.ce_bucket + len(ex)] = torch.as_tensor(ex, dtype=torch.int32)
        self.d_in.copy_(h, non_blocking=True)
        self.graph.replay()
        torch.cuda.current_stream(self.d_in.device).synchronize()  # the select kernel wrote into pinned host memory
        return self.bufs.out_idx[0].numpy().copy(), self.bufs.out_logit[0].numpy().copy()


class RerankedRecommender:
    """Retrieve with a Recommender, rerank with a CrossEncoderReranker: the reference's duck type
    `recommend(query, top_k, exclude_product_ids)`.  The wrapped recommender finds `candidates` products (exclusions are
    applied there); their product sides were tokenised once, here at construction, and live on the GPU; the query is
    tokenised once per call by each of the two models; the best top_k come back as (product_id, cross-encoder score),
    ordered by raw logit, ties by retrieval position, the model's activation applied to the returned logits on the host.
    One request replays one captured graph (_CapturedRequest) when the recommender's single-request path supports it;
    recommend_batch runs one retrieval call and reranks in calls of at most RERANK_TOKENS_PER_CALL tokens.
    device_assembly=False keeps the host path - candidates copied to the host, pairs assembled in numpy
    (model_io.assemble_pairs), one score_packed call, np.argsort on the activated scores - as the comparison."""

    def __init__(self, recommender, reranker: CrossEncoderReranker, candidates: int = 100, device_assembly: bool = True):
        self.recommender, self.reranker, self.candidates = recommender, reranker, int(candidates)
        sides = reranker.side_ids(recommender.product_texts)
        self._product_side = dict(zip(recommender.product_ids, sides))
        self._cat_max_len = max((len(s) for s in sides), default=0)
        self.device_assembly = bool(device_assembly)
        if self.device_assembly:
            if recommender.device != reranker.encoder.device:
                raise ValueError(f"recommender on {recommender.device}, reranker on {reranker.encoder.device}: device "
                                 "assembly needs both on one GPU")
            self._device = DeviceReranker(reranker, sides, recommender._index.row_offset)
            self._graphs: dict[tuple, _CapturedRequest] = {}
            self._graphs_of = None  # the single-request path the graphs were captured against

    # -- the host path ---------------------------------------------------------------------------
    def _recommend_host(self, query: str, top_k: int, exclude_product_ids) -> list[tuple[str, float]]:
        found = self.recommender.recommend(query, self.candidates, exclude_product_ids)
        if not found:
            return []
        q = self.reranker.side_ids([query])[0]
        scores = self.reranker.score_ids([q] * len(found), [self._product_side[pid] for pid, _ in found])
        return [(found[i][0], s) for i, s in best_first(scores, max(int(top_k), 1))]

    def _recommend_batch_host(self, queries, top_k: int, exclude_product_ids) -> list[list[tuple[str, float]]]:
        found = self.recommender.recommend_batch(queries, self.candidates, exclude_product_ids)
        q_sides = self.reranker.side_ids(list(queries))
        out: list[list[tuple[str, float]]] = []
        for lo, hi in self._chunks([len(q) for q in q_sides], max((len(f) for f in found), default=0)):
            a = [q_sides[i] for i in range(lo, hi) for _ in found[i]]
            b = [self._product_side[pid] for i in range(lo, hi) for pid, _ in found[i]]
            scores, at = self.reranker.score_ids(a, b), 0
            for i in range(lo, hi):
                s = scores[at:at + len(found[i])]
                at += len(found[i])
                out.append([(found[i][j][0], v) for j, v in best_first(s, max(int(top_k), 1))])
        return out

    # -- the device path -------------------------------------------------------------------------
    def _chunks(self, q_lens: Sequence[int], k: int):
        """Query ranges [lo, hi) whose pair-token bound stays within RERANK_TOKENS_PER_CALL (one query at the least)."""
        lo, tokens = 0, 0
        for i, n in enumerate(q_lens):
            t = self.reranker.pair_token_bound([n], k, self._cat_max_len)
            if i > lo and tokens + t > RERANK_TOKENS_PER_CALL:
                yield lo, i
                lo, tokens = i, 0
            tokens += t
        if len(q_lens) > lo:
            yield lo, len(q_lens)

    def _shape(self, top_k: int) -> tuple[int, int]:
        k = self.recommender._k(self.candidates)
        return k, min(max(int(top_k), 1), k)

    def _query_sides(self, queries: Sequence[str]) -> list[np.ndarray]:
        cap = self._device.query_side_cap()
        return [q[:cap] for q in self.reranker.side_ids(list(queries))]

    def _results(self, idx_row: np.ndarray, logit_row: np.ndarray) -> list[tuple[str, float]]:
        keep = idx_row >= 0
        scores = self.reranker.activate(np.ascontiguousarray(logit_row[keep], dtype=np.float32))
        return [(self.recommender.product_ids[int(i)], float(s)) for i, s in zip(idx_row[keep], scores)]

    def _rerank_batch(self, ids: np.ndarray, cu: np.ndarray, q_sides: list[np.ndarray], k: int, top: int, ex):
        """Un-captured: one encode + search, then rerank_into per chunk of queries -> host (idx, logits) [n, top]."""
        rec, dr, dev = self.recommender, self._device, self._device.device
        n = len(q_sides)
        cand_idx, cand_sc = rec._index.search(rec.model.encoder.encode_packed_host(ids, cu), k, ex)
        q_lens = [len(q) for q in q_sides]
        q_cu = np.zeros(n + 1, np.int64)
        np.cumsum(q_lens, out=q_cu[1:])
        flat = np.concatenate(list(q_sides) + [np.zeros(1, np.int32)]).astype(np.int32)  # (one spare id: no chunk's view is empty)
        q_ids = torch.from_numpy(flat).to(dev, non_blocking=True)
        out_idx = torch.empty((n, top), dtype=torch.int64, device=dev)
        out_logit = torch.empty((n, top), dtype=torch.float32, device=dev)
        for lo, hi in self._chunks(q_lens, k):
            b = RerankBuffers(dr, hi - lo, k, top, dr.token_bound(q_lens[lo:hi], k), out=(out_idx[lo:hi], out_logit[lo:hi]))
            cu_c = torch.from_numpy((q_cu[lo:hi + 1] - q_cu[lo]).astype(np.int32)).to(dev, non_blocking=True)
            dr.rerank_into(q_ids[int(q_cu[lo]):], cu_c, cand_idx[lo:hi], dr.max_pair_len(max(q_lens[lo:hi])), b,
                           cand_sc[lo:hi])
        return out_idx.cpu().numpy(), out_logit.cpu().numpy()

    def recommend(self, query: str, top_k: int = 10, exclude_product_ids: set[str] | None = None) -> list[tuple[str, float]]:
        if not self.device_assembly:
            return self._recommend_host(query, top_k, exclude_product_ids)
        rec = self.recommender
        k, top = self._shape(top_k)
        ids, cu = rec.model.tokenizer.packed([query])
        q_side = self._query_sides([query])[0]
        ex = rec._exclusion_rows([exclude_product_ids])
        rows = ex[0] if ex else []
        fast = rec._fast_path()
        if fast is not None and fast.supports(len(ids), k, len(rows)):
            bucket = next(b for b in fast.buckets if len(ids) <= b)
            ce_bucket = 32
            while ce_bucket < len(q_side):
                ce_bucket *= 2
            if self._graphs_of is not fast:  # a rebuilt fast path: a new index or encoder under the graphs
                self._graphs.clear()
                self._graphs_of = fast
            key = (bucket, ce_bucket, k, top)
            c = self._graphs.get(key)
            if c is None:
                c = self._graphs[key] = _CapturedRequest(self, bucket, ce_bucket, k, top)
            return self._results(*c.run(ids, q_side, rows))
        idx, logit = self._rerank_batch(ids, cu, [q_side], k, top, ex)
        return self._results(idx[0], logit[0])

    def distill_adapter(self, contexts: Sequence[str], candidates: Optional[int] = None, temperature: float = 1.0,
                        **fit) -> list[float]:
        """Teach the first stage's query adapter what the cross-encoder prefers, without labels: every context's
        `candidates` products (default: self.candidates) are retrieved with the CURRENT first stage, the cross-encoder
        gives each its raw logit, the targets are softmax(logits / temperature) over a context's candidates (torch, on
        the device), and the recommender's adapter is trained on these lists (QueryAdapter.fit_lists; `fit`: its epochs,
        batch_size, lr, weight_decay, scale, seed) - installed if there was none, in place otherwise -> the per-step
        losses.  The logits come from the host-assembled path, in chunks of RERANK_TOKENS_PER_CALL tokens: a set-up
        call, never while a request is being served.  ValueError before any GPU work: no context, one that is not a
        string, candidates outside [1, ICREC_ADAPTER_MAX_LIST], a temperature that is not finite and > 0, fit_plan's."""
        rec = self.recommender
        contexts = list(contexts) if not isinstance(contexts, (str, bytes)) else None
        if not contexts or not all(isinstance(c, str) for c in contexts):
            raise ValueError("contexts must be a non-empty sequence of strings")
        k = self.candidates if candidates is None else candidates
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _native.ICREC_ADAPTER_MAX_LIST:
            raise ValueError(f"candidates must be an integer in [1, {_native.ICREC_ADAPTER_MAX_LIST}], got {k!r}")
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.integer, np.floating)) or not 0 < temperature < float("inf"):
            raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
        unknown = set(fit) - {"epochs", "batch_size", "lr", "weight_decay", "scale", "seed"}
        if unknown:
            raise ValueError(f"distill_adapter takes fit_lists' arguments, not {sorted(unknown)}")
        fit_plan(len(contexts), fit.get("epochs", 5), fit.get("batch_size", 64), 0, fit.get("lr", 2e-3),
                 fit.get("weight_decay", 0.01), fit.get("scale", DEFAULT_SCALE))
        k = int(k)
        found = rec.recommend_batch(contexts, k)
        q_sides = self.reranker.side_ids(contexts)
        dev = rec.device
        rows = torch.full((len(contexts), k), -1, dtype=torch.int32)
        logits = torch.full((len(contexts), k), float("-inf"), dtype=torch.float32, device=dev)
        for lo, hi in self._chunks([len(q) for q in q_sides], k):
            a = [q_sides[i] for i in range(lo, hi) for _ in found[i]]
            if not a:
                continue
            scores = self.reranker.logit_ids(a, [self._product_side[pid] for i in range(lo, hi) for pid, _ in found[i]])
            at = 0
            for i in range(lo, hi):
                n = len(found[i])
                rows[i, :n] = torch.tensor([rec._pid_to_row[pid] for pid, _ in found[i]], dtype=torch.int32)
                logits[i, :n] = scores[at:at + n]
                at += n
        target = torch.nan_to_num(torch.softmax(logits / float(temperature), dim=1), nan=0.0)  # (nothing found: no target)
        lists = (torch.arange(len(contexts) + 1, dtype=torch.int32, device=dev) * k, rows.to(dev).reshape(-1),
                 target.reshape(-1), k)
        anchors = rec.model.encode_to_device(contexts)
        return rec._train_adapter(lambda adapter: adapter.fit_lists(rec._index, anchors, lists, **fit))

    def recommend_batch(self, queries: Sequence[str], top_k: int = 10,
                        exclude_product_ids: Optional[Sequence[Optional[set[str]]]] = None
                        ) -> list[list[tuple[str, float]]]:
        """Many contexts: one retrieval pass, the rerank in chunks; element i equals recommend(queries[i], ...)."""
        if not queries:
            return []
        if not self.device_assembly:
            return self._recommend_batch_host(queries, top_k, exclude_product_ids)
        rec = self.recommender
        k, top = self._shape(top_k)
        idx, logit = self._rerank_batch(*rec.model.tokenizer.packed(list(queries)), self._query_sides(queries), k, top,
                                        rec._exclusion_rows(exclude_product_ids))
        return [self._results(idx[i], logit[i]) for i in range(len(queries))]
