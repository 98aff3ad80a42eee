"""Reranking with a BERT cross-encoder: the second half of a sentence-transformers retrieval stack.

The bi-encoder retrieves (recommender.py: embed the context, cosine top-k over the catalog); a cross-encoder then reads
each `[CLS] query [SEP] product [SEP]` as ONE sequence and returns one relevance score per pair - what
`sentence_transformers.CrossEncoder.predict` / `.rank` do for the cross-encoder/ms-marco-MiniLM-L-*-v2 family
(BertForSequenceClassification with one label).  Here the pairs are assembled on the host from the two sides' token ids
(model_io.assemble_pairs) and scored in one libicrec call (icrec_score_pairs: segment ids in the embedding kernel, the
last layer on the [CLS] rows only, the pooler + classifier head kernel).  No CPU or PyTorch fallback.
"""
from __future__ import annotations

from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from .encoder import DeviceEncoder
from .model_io import assemble_pairs, load_cross_encoder_dir, strip_specials


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
        ids, cu, seg_b = assemble_pairs(a_ids, b_ids, self.max_seq_length, self.cls_id, self.sep_id)
        dev = self.encoder.device
        logits = self.encoder.score_packed(torch.from_numpy(ids).to(dev), torch.from_numpy(cu).to(dev),
                                           torch.from_numpy(seg_b).to(dev), int(np.diff(cu).max())).cpu().numpy()
        if self.activation == "identity":
            return logits
        return (np.float32(1) / (np.float32(1) + np.exp(-logits, dtype=np.float32))).astype(np.float32)

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


class RerankedRecommender:
    """Retrieve with a Recommender, rerank with a CrossEncoderReranker: the reference's duck type
    `recommend(query, top_k, exclude_product_ids)`.  The wrapped recommender returns `candidates` products (exclusions are
    applied there); their product sides were tokenised once, here at construction, the query is tokenised once per call,
    and one score_packed call scores the candidates: the best top_k come back as (product_id, cross-encoder score)."""

    def __init__(self, recommender, reranker: CrossEncoderReranker, candidates: int = 100):
        self.recommender, self.reranker, self.candidates = recommender, reranker, int(candidates)
        self._product_side = dict(zip(recommender.product_ids, reranker.side_ids(recommender.product_texts)))

    def recommend(self, query: str, top_k: int = 10, exclude_product_ids: set[str] | None = None) -> list[tuple[str, float]]:
        found = self.recommender.recommend(query, self.candidates, exclude_product_ids)
        if not found:
            return []
        q = self.reranker.side_ids([query])[0]
        scores = self.reranker.score_ids([q] * len(found), [self._product_side[pid] for pid, _ in found])
        return [(found[i][0], s) for i, s in best_first(scores, max(int(top_k), 1))]
