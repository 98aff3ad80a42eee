"""Batched ranking consumer: the reference's ContentBasedBaseline.rank_all
(src/baselines/content_based.py:16-64; the same shape is used by
scripts/compare_untrained_vs_trained.py:38-85).

The reference encodes all eval queries, builds the dense [13,120 x 49,688] fp32 score matrix on
the host (2.6 GB) and fully argsorts every row, although its metrics
(src/baselines/metrics.py:122-176: Accuracy@1/3/5/10, Recall@10, MRR@10, NDCG@10, MAP@100) never
look past rank 100.  Here queries stream through the GPU in passes of `queries_per_pass`.
`rank_all()` returns the reference's complete order (icrec_rank_all: exact score rows sorted on the
device per pass); `rank_all(depth=100)` is the fast form for the metrics: one encode + one fused
score/top-`depth` search per pass, no score matrix at all.
"""
from __future__ import annotations

import csv
import ctypes as C
import json
from pathlib import Path

import numpy as np
import torch

from . import _native, ir_metrics
from ._native import ptr, stream_ptr
from .adapter import QueryAdapter
from .model_io import load_model_dir
from .recommender import SbertModel
from .search import DeviceIndex, fuse_select, rrf_weights


def _evaluate(baseline, relevant_docs: dict[str, set[str]], depth: int, queries_per_pass: int | None,
              **pass_args) -> dict[str, float]:
    """The eight IR metrics of a baseline's top-`depth` rows, pass by pass on the device."""
    row_of = {pid: j for j, pid in enumerate(baseline.product_ids)}
    sums = []
    for rows, qids in baseline._row_passes(depth, queries_per_pass, **pass_args):
        off, rel = ir_metrics.relevant_csr(qids, relevant_docs, row_of, baseline.device)
        sums.append(ir_metrics.ir_metrics_rows_raw(rows, off, rel)[0])
    if not sums:
        return ir_metrics.metrics_from_sums(np.zeros(9))
    return ir_metrics.metrics_from_sums(torch.stack(sums).cpu().numpy())


class ContentBasedBaseline:
    """Same constructor and `rank_all` contract as the reference class, with `model_name` a LOCAL
    SentenceTransformer directory (no hub access).  adapter: a QueryAdapter, or the file one was saved to, that every
    query vector goes through before the search (q' = q + D q; adapter.py) - the corpus embeddings are what they are
    without it, so `evaluate` reports the eight metrics with and without the adapter over the same index."""

    def __init__(self, eval_queries: dict[str, str], eval_corpus: dict[str, str], model_name: str | Path,
                 batch_size: int = 64, device: str | torch.device = "cuda:0", adapter=None):
        self.eval_queries = eval_queries
        self.eval_corpus = eval_corpus
        self.product_ids = list(eval_corpus.keys())
        self.corpus_texts = [eval_corpus[pid] for pid in self.product_ids]
        self.device = torch.device(device)
        self.model = SbertModel(load_model_dir(model_name), self.device)
        self.corpus_embeddings = self.model.encode(self.corpus_texts, batch_size=batch_size,
                                                   show_progress_bar=True, normalize_embeddings=True)
        self._index = DeviceIndex(self.corpus_embeddings, self.device)
        if adapter is not None and not isinstance(adapter, QueryAdapter):
            adapter = QueryAdapter.load(adapter, self.device)
        if adapter is not None and adapter.dim != self._index.dim:
            raise ValueError(f"the adapter is {adapter.dim} wide, the model {self._index.dim}")
        self.adapter = adapter

    def _query_embeddings(self, qids) -> torch.Tensor:
        """The queries' vectors on the device, through the adapter when there is one."""
        emb = self.model.encode_to_device([self.eval_queries[q] for q in qids])
        return emb if self.adapter is None else self.adapter.apply(emb)

    def rank_all(self, depth: int | None = None, queries_per_pass: int | None = None) -> dict[str, list[str]]:
        """query_id -> product ids by cosine similarity, best first (score desc, then lower corpus row first
        on exact ties).  depth=None: every product, like the reference (content_based.py:58-63);
        1 <= depth <= 128: only the best `depth` (what the metrics read), through the fused search."""
        full = depth is None
        if not full and not 1 <= depth <= _native.ICREC_MAX_K:
            raise ValueError(f"depth must be None (full order) or in [1, {_native.ICREC_MAX_K}]")
        if queries_per_pass is None:
            queries_per_pass = 256 if full else 1024
        depth = len(self.product_ids) if full else min(depth, len(self.product_ids))
        query_ids = list(self.eval_queries.keys())
        out: dict[str, list[str]] = {}
        for s in range(0, len(query_ids), queries_per_pass):
            qids = query_ids[s:s + queries_per_pass]
            emb = self._query_embeddings(qids)
            idx = self._index.rank_all(emb) if full else self._index.search(emb, depth)[0]
            idx = idx.cpu().numpy()
            for i, qid in enumerate(qids):
                out[qid] = [self.product_ids[j] for j in idx[i] if j >= 0]
        return out

    def boost_lists(self, query_ids: list[str], boosts: dict, boost_weight) -> list[dict[int, float]]:
        """query id -> product ids to boost (e.g. ItemItemCFBaseline's histories) -> per query {corpus row: weight},
        what DeviceIndex.search_boosted takes.  Products outside the corpus are skipped; a list of more than
        ICREC_MAX_BOOSTS corpus products keeps the first ICREC_MAX_BOOSTS in corpus order."""
        if boost_weight is None or not float(boost_weight) >= 0.0:  # (a NaN fails the comparison)
            raise ValueError(f"boosts needs a boost_weight >= 0, got {boost_weight!r}")
        if not hasattr(self, "_row_of"):
            self._row_of = {pid: j for j, pid in enumerate(self.product_ids)}
        w = float(boost_weight)
        return [{r: w for r in sorted(self._row_of[p] for p in set(boosts.get(q, ())) if p in self._row_of)[:_native.ICREC_MAX_BOOSTS]}
                for q in query_ids]

    def _row_passes(self, depth: int, queries_per_pass: int | None, boosts: dict | None = None, boost_weight=None):
        if not 1 <= depth <= _native.ICREC_MAX_K:
            raise ValueError(f"depth must be in [1, {_native.ICREC_MAX_K}]")
        query_ids = list(self.eval_queries.keys())
        step = queries_per_pass or 1024
        for s in range(0, len(query_ids), step):
            qids = query_ids[s:s + step]
            lists = None if boosts is None else self.boost_lists(qids, boosts, boost_weight)
            emb = self._query_embeddings(qids)
            yield (self._index.search(emb, depth) if lists is None else self._index.search_boosted(emb, depth, lists))[0], qids

    def rank_rows(self, depth: int = 100, queries_per_pass: int | None = None, boosts: dict | None = None,
                  boost_weight=None) -> tuple[torch.Tensor, list[str]]:
        """(int64 [Q, depth] corpus rows on the device, best first with -1 pads; the query ids in row order): what
        `rank_all(depth)` turns into id strings.  boosts: query id -> the products to lift by boost_weight (a user's
        earlier purchases): the ranking is then by cosine + boost_weight for those, over the whole corpus."""
        passes = list(self._row_passes(depth, queries_per_pass, boosts, boost_weight))
        return torch.cat([r for r, _ in passes]), [q for _, qs in passes for q in qs]

    def evaluate(self, relevant_docs: dict[str, set[str]], depth: int = 100,
                 queries_per_pass: int | None = None, boosts: dict | None = None, boost_weight=None) -> dict[str, float]:
        """compute_ir_metrics(rank_all(depth), relevant_docs) without leaving the device: the eight-metric dict.
        boosts / boost_weight: as rank_rows takes them."""
        return _evaluate(self, relevant_docs, depth, queries_per_pass, boosts=boosts, boost_weight=boost_weight)


def _read_csv_columns(path: Path, names: tuple[str, ...]):
    """The named columns of a CSV file with a header row, as lists of strings."""
    with open(path, newline="") as f:
        rd = csv.reader(f)
        header = next(rd)
        at = [header.index(n) for n in names]
        cols = [[] for _ in names]
        for rec in rd:
            for c, a in zip(cols, at):
                c.append(rec[a])
    return cols


class ItemItemCFBaseline:
    """The reference's item-item co-occurrence baseline (src/baselines/collaborative_filtering.py:50-163) with the
    same constructor and `rank_all` contract: score(candidate) = sum over the products h of the user's prior orders
    of the number of orders that hold both.  No co-occurrence table is built: libicrec ranks from the order x product
    incidence matrix (icrec_cf_rank / icrec_cf_rank_all)."""

    def __init__(self, data_dir: str | Path, processed_dir: str | Path, order_products_chunk_size: int = 500_000,
                 device: str | torch.device = "cuda:0"):
        self.data_dir, self.processed_dir = Path(data_dir), Path(processed_dir)
        self.order_products_chunk_size = order_products_chunk_size  # the reference's pandas chunking; the csv reader streams
        arrays = self.load_arrays(self.data_dir, self.processed_dir)
        self._init_arrays(device=device, **arrays)

    @classmethod
    def from_arrays(cls, baskets, histories: dict[str, list[str]], corpus_ids: list[str],
                    device: str | torch.device = "cuda:0") -> "ItemItemCFBaseline":
        """From memory: `baskets` an iterable of product-id lists (one per prior order, repeats allowed), `histories`
        query id -> product ids of the user's earlier orders, `corpus_ids` the candidates in ranking-tie order."""
        self = cls.__new__(cls)
        self.data_dir = self.processed_dir = None
        self._init_arrays([list(b) for b in baskets], {q: set(h) for q, h in histories.items()}, list(corpus_ids), device)
        return self

    @staticmethod
    def load_arrays(data_dir: Path, processed_dir: Path) -> dict:
        """The reference's selection rules (collaborative_filtering.py:72-138) with the stdlib csv module:
        baskets = the prior orders of users who have an eval order (rows in file order, per order); history of an eval
        order = products of its user's prior orders with a smaller order_number; an eval query without a train order
        gets an empty history; candidates = eval_corpus keys in file order."""
        eval_q = json.loads((processed_dir / "eval_queries.json").read_text())
        corpus_ids = list(json.loads((processed_dir / "eval_corpus.json").read_text()).keys())
        eval_order_ids = {int(q) for q in eval_q}
        oid, uid, onum, eset = _read_csv_columns(data_dir / "orders.csv", ("order_id", "user_id", "order_number", "eval_set"))
        train = {int(o): (int(u), int(n)) for o, u, n, e in zip(oid, uid, onum, eset) if e == "train"}
        users_eval = {train[o][0] for o in eval_order_ids if o in train}
        prior = {int(o): (int(u), int(n)) for o, u, n, e in zip(oid, uid, onum, eset) if e == "prior" and int(u) in users_eval}
        order_to_products: dict[int, list[str]] = {}
        with open(data_dir / "order_products__prior.csv", newline="") as f:
            rd = csv.reader(f)
            header = next(rd)
            a_o, a_p = header.index("order_id"), header.index("product_id")
            for rec in rd:
                o = int(rec[a_o])
                if o in prior:
                    order_to_products.setdefault(o, []).append(str(int(float(rec[a_p]))))
        by_user: dict[int, list[tuple[int, int]]] = {}
        for o, (u, n) in prior.items():
            by_user.setdefault(u, []).append((n, o))
        histories: dict[str, set[str]] = {}
        for q in eval_q:
            hist: set[str] = set()
            if int(q) in train:
                u, n = train[int(q)]
                for pn, po in by_user.get(u, ()):
                    if pn < n:
                        hist.update(order_to_products.get(po, ()))
            histories[q] = hist
        return {"baskets": list(order_to_products.values()), "histories": histories, "corpus_ids": corpus_ids}

    def _init_arrays(self, baskets: list[list[str]], histories: dict[str, set[str]], corpus_ids: list[str], device) -> None:
        self.device = _native.hip_device(device, "ItemItemCFBaseline")
        self.baskets, self.eval_order_to_history, self.corpus_ids = baskets, histories, corpus_ids
        self.product_ids = corpus_ids  # candidate rows, as ContentBasedBaseline names them
        # items: the corpus rows first, then every other product of a basket (histories are subsets of those)
        self.item_of = {pid: j for j, pid in enumerate(corpus_ids)}
        if len(self.item_of) != len(corpus_ids):
            raise ValueError("corpus ids must be unique")
        for b in baskets:
            for pid in b:
                self.item_of.setdefault(pid, len(self.item_of))
        off = np.zeros(len(baskets) + 1, np.int64)
        np.cumsum([len(b) for b in baskets], out=off[1:])
        items = np.fromiter((self.item_of[p] for b in baskets for p in b), np.int32, count=int(off[-1]))
        if not baskets:  # a catalog nobody bought from: one empty order keeps the index well-formed
            off = np.zeros(2, np.int64)
        self._h = None
        if not corpus_ids:
            return
        h = C.c_void_p()
        _native.check(_native.lib().icrec_cf_create(off.ctypes.data_as(C.c_void_p), items.ctypes.data_as(C.c_void_p),
                                                    len(off) - 1, len(self.item_of), len(corpus_ids), self.device.index,
                                                    C.byref(h)), "icrec_cf_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.lib().icrec_cf_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def history_csr(self, query_ids: list[str]) -> tuple[torch.Tensor, torch.Tensor]:
        """(off int32[Q+1], items int32[nnz]) on the device, each history's item numbers ascending; a product no
        basket or corpus row knows cannot co-occur with anything and is dropped."""
        off = np.zeros(len(query_ids) + 1, np.int32)
        flat: list[int] = []
        for i, q in enumerate(query_ids):
            flat.extend(sorted(self.item_of[p] for p in self.eval_order_to_history.get(q, ()) if p in self.item_of))
            off[i + 1] = len(flat)
        return torch.from_numpy(off).to(self.device), torch.from_numpy(np.asarray(flat, np.int32)).to(self.device)

    def history_csr_from(self, histories) -> tuple[torch.Tensor, torch.Tensor]:
        """history_csr for ad-hoc histories: per query an iterable of product ids (None: an empty history) -> the same
        (off, items) device CSR, each history's item numbers ascending and unique, unknown products dropped."""
        off = np.zeros(len(histories) + 1, np.int32)
        flat: list[int] = []
        for i, h in enumerate(histories):
            flat.extend(sorted({self.item_of[p] for p in (h or ()) if p in self.item_of}))
            off[i + 1] = len(flat)
        return torch.from_numpy(off).to(self.device), torch.from_numpy(np.asarray(flat, np.int32)).to(self.device)

    def rank_workspace_bytes(self, n_queries: int, depth: int) -> int:
        """icrec_cf_rank_workspace_bytes: what one pass of rank_rows_scores(.., depth) over n_queries allocates."""
        return int(_native.lib().icrec_cf_rank_workspace_bytes(self._h, int(n_queries), int(depth))) if self._h else 0

    def rank_rows_scores(self, query_ids, depth: int | None) -> tuple[torch.Tensor, torch.Tensor | None]:
        """One pass on the device: (rows int64 [Q, depth or n_candidates], int32 scores [Q, depth] or None).
        query_ids: a list of eval query ids, or the (off, items) device CSR history_csr / history_csr_from return."""
        if self._h is None:
            raise _native.IcrecError("ItemItemCFBaseline has an empty corpus: nothing to rank")
        L = _native.lib()
        if isinstance(query_ids, tuple) and len(query_ids) == 2 and isinstance(query_ids[0], torch.Tensor):
            off, items = query_ids
            Q = int(off.numel()) - 1
        else:
            Q = len(query_ids)
            off, items = self.history_csr(query_ids)
        st = stream_ptr(self.device)
        if depth is None:
            ws = torch.empty(max(int(L.icrec_cf_rank_all_workspace_bytes(self._h, Q)), 1), dtype=torch.uint8, device=self.device)
            rows = torch.empty((Q, len(self.corpus_ids)), dtype=torch.int64, device=self.device)
            _native.check(L.icrec_cf_rank_all(self._h, ptr(off), ptr(items), Q, ptr(rows), ptr(ws), ws.numel(), st),
                          "icrec_cf_rank_all")
            return rows, None
        ws = torch.empty(max(int(L.icrec_cf_rank_workspace_bytes(self._h, Q, depth)), 1), dtype=torch.uint8, device=self.device)
        rows = torch.empty((Q, depth), dtype=torch.int64, device=self.device)
        scores = torch.empty((Q, depth), dtype=torch.int32, device=self.device)
        _native.check(L.icrec_cf_rank(self._h, ptr(off), ptr(items), Q, depth, ptr(rows), ptr(scores), ptr(ws), ws.numel(), st),
                      "icrec_cf_rank")
        return rows, scores

    def _row_passes(self, depth: int | None, queries_per_pass: int | None, eval_query_ids: list[str] | None = None):
        if depth is not None and not 1 <= depth <= _native.ICREC_MAX_K:
            raise ValueError(f"depth must be None (full order) or in [1, {_native.ICREC_MAX_K}]")
        query_ids = list(self.eval_order_to_history.keys()) if eval_query_ids is None else list(eval_query_ids)
        step = queries_per_pass or (256 if depth is None else 1024)
        for s in range(0, len(query_ids), step):
            qids = query_ids[s:s + step]
            yield self.rank_rows_scores(qids, depth)[0], qids

    def rank_all(self, eval_query_ids: list[str] | None = None, depth: int | None = None,
                 queries_per_pass: int | None = None) -> dict[str, list[str]]:
        """query_id -> candidate product ids by CF score, best first (score desc, then corpus order), without the
        products of the query's own history.  depth=None: every remaining candidate, like the reference
        (collaborative_filtering.py:140-163); 1 <= depth <= 128: only the best `depth`."""
        out: dict[str, list[str]] = {}
        for rows, qids in self._row_passes(depth, queries_per_pass, eval_query_ids):
            rows = rows.cpu().numpy()
            for i, qid in enumerate(qids):
                out[qid] = [self.corpus_ids[j] for j in rows[i] if j >= 0]
        return out

    def rank_rows(self, depth: int = 100, queries_per_pass: int | None = None,
                  eval_query_ids: list[str] | None = None) -> tuple[torch.Tensor, list[str]]:
        """(int64 [Q, depth] corpus rows on the device, best first with -1 pads; the query ids in row order)."""
        passes = list(self._row_passes(depth, queries_per_pass, eval_query_ids))
        return torch.cat([r for r, _ in passes]), [q for _, qs in passes for q in qs]

    def evaluate(self, relevant_docs: dict[str, set[str]], depth: int = 100,
                 queries_per_pass: int | None = None) -> dict[str, float]:
        """compute_ir_metrics(rank_all(depth=depth), relevant_docs) without leaving the device."""
        return _evaluate(self, relevant_docs, depth, queries_per_pass)


class HybridBaseline:
    """The content ranking and the item-item CF ranking of the same corpus rows fused by position on the device
    (reciprocal rank fusion, icrec_fuse_select): per pass the content search and icrec_cf_rank run `depth` wide on the
    same queries, and a product's fused score is 1 / (rrf_c + its content position + 1) + cf_weight / (rrf_c + its CF
    position + 1), a list that does not hold it adding 0.  The CF scores gate the CF list: a candidate that co-occurs
    with nothing in the history does not vote.  Same `rank_rows` / `rank_all(depth)` / `evaluate` contracts as the two
    baselines it is built from."""

    def __init__(self, content: ContentBasedBaseline, cf: ItemItemCFBaseline, depth: int = 100, cf_weight: float = 1.0,
                 rrf_c: float = 60.0):
        if list(content.product_ids) != list(cf.product_ids):
            raise ValueError("HybridBaseline: the content and the CF baseline must rank the same product ids in the same order")
        if not 1 <= depth <= _native.ICREC_MAX_K:
            raise ValueError(f"depth must be in [1, {_native.ICREC_MAX_K}]")
        if torch.device(content.device) != torch.device(cf.device):
            raise ValueError(f"HybridBaseline: the baselines live on {content.device} and {cf.device}")
        self.content, self.cf, self.depth = content, cf, int(depth)
        self.cf_weight, self.rrf_c = float(cf_weight), float(rrf_c)
        self.product_ids, self.device = cf.product_ids, cf.device
        self.eval_queries = content.eval_queries

    def _tables(self, depth: int):
        """(the content list's, the CF list's) position tables on the device."""
        return (torch.from_numpy(rrf_weights(depth, self.rrf_c, 1.0)).to(self.device),
                torch.from_numpy(rrf_weights(depth, self.rrf_c, self.cf_weight)).to(self.device))

    def _row_passes(self, depth: int | None, queries_per_pass: int | None):
        depth = self.depth if depth is None else depth
        if not 1 <= depth <= _native.ICREC_MAX_K:
            raise ValueError(f"depth must be in [1, {_native.ICREC_MAX_K}]")
        a_w, b_w = self._tables(depth)
        for a_idx, qids in self.content._row_passes(depth, queries_per_pass):
            b_idx, b_sc = self.cf.rank_rows_scores(qids, depth)
            yield fuse_select(a_idx, b_idx, a_w, b_w, depth, len(self.product_ids), b_gate=b_sc)[0], qids

    def rank_rows(self, depth: int | None = None, queries_per_pass: int | None = None) -> tuple[torch.Tensor, list[str]]:
        """(int64 [Q, depth] corpus rows on the device, best first with -1 pads; the query ids in row order).  depth
        None: the constructor's."""
        passes = list(self._row_passes(depth, queries_per_pass))
        return torch.cat([r for r, _ in passes]), [q for _, qs in passes for q in qs]

    def rank_all(self, depth: int | None = None, queries_per_pass: int | None = None) -> dict[str, list[str]]:
        """query_id -> product ids by fused score, best first (lower corpus row first on ties): the best `depth` of
        the union of the two `depth`-wide lists."""
        out: dict[str, list[str]] = {}
        for rows, qids in self._row_passes(depth, queries_per_pass):
            rows = rows.cpu().numpy()
            for i, qid in enumerate(qids):
                out[qid] = [self.product_ids[j] for j in rows[i] if j >= 0]
        return out

    def evaluate(self, relevant_docs: dict[str, set[str]], depth: int | None = None,
                 queries_per_pass: int | None = None) -> dict[str, float]:
        """compute_ir_metrics(rank_all(depth), relevant_docs) without leaving the device."""
        return _evaluate(self, relevant_docs, self.depth if depth is None else depth, queries_per_pass)
