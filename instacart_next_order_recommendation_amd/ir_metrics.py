"""IR metrics of ranked lists, on the device: the reference's compute_ir_metrics
(src/baselines/metrics.py:122-176) over ROWS instead of product-id strings.

`compute_ir_metrics` keeps the reference's signature (dicts of id lists and id sets) and maps ids to
rows; `compute_ir_metrics_rows` takes the device tensors a search or ranking call already returned, so
an evaluation never builds the dict of string lists (icrec_ir_metrics, csrc/metrics.hip).
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from . import _native
from ._native import ptr, stream_ptr

METRIC_KEYS = ("accuracy_at_1", "accuracy_at_3", "accuracy_at_5", "accuracy_at_10", "recall_at_10", "mrr_at_10",
               "ndcg_at_10", "map_at_100")


def load_eval_data(processed_dir: str | Path) -> tuple[dict[str, str], dict[str, str], dict[str, set[str]]]:
    """(eval_queries, eval_corpus, eval_relevant_docs) of a processed directory
    (collaborative_filtering.py:30-47)."""
    processed_dir = Path(processed_dir)
    queries = json.loads((processed_dir / "eval_queries.json").read_text())
    corpus = json.loads((processed_dir / "eval_corpus.json").read_text())
    relevant = {k: set(v) for k, v in json.loads((processed_dir / "eval_relevant_docs.json").read_text()).items()}
    return queries, corpus, relevant


def relevant_csr(query_ids, relevant_docs: dict[str, set[str]], row_of: dict[str, int], device=None):
    """Relevant sets of `query_ids` as (off int64[Q+1], rows int64[nnz]), rows ascending per query.  A query that is
    not in `relevant_docs` gets an empty set (it is then not counted)."""
    off = np.zeros(len(query_ids) + 1, np.int64)
    flat: list[int] = []
    for i, qid in enumerate(query_ids):
        flat.extend(sorted(row_of[p] for p in relevant_docs.get(qid, ())))
        off[i + 1] = len(flat)
    rows = np.asarray(flat, np.int64)
    if device is None:
        return off, rows
    return torch.from_numpy(off).to(device), torch.from_numpy(rows).to(device)


def ir_metrics_rows_raw(ranked_rows: torch.Tensor, rel_off: torch.Tensor, rel_rows: torch.Tensor, per_query: bool = False):
    """(sums double[9] on the device, per-query double[Q, 8] or None): icrec_ir_metrics as it is."""
    dev = _native.hip_device(ranked_rows.device, "compute_ir_metrics_rows")
    if ranked_rows.dim() != 2 or ranked_rows.dtype != torch.int64:
        raise ValueError("ranked_rows must be int64 [Q, depth]")
    ranked_rows = ranked_rows.contiguous()
    Q, depth = int(ranked_rows.shape[0]), int(ranked_rows.shape[1])
    if rel_off.numel() != Q + 1:
        raise ValueError(f"rel_off has {rel_off.numel()} entries for {Q} queries")
    rel_off = rel_off.to(device=dev, dtype=torch.int64).contiguous()
    rel_rows = rel_rows.to(device=dev, dtype=torch.int64).contiguous()
    L = _native.lib()
    sums = torch.empty(9, dtype=torch.float64, device=dev)
    pq = torch.empty((Q, 8), dtype=torch.float64, device=dev) if per_query else None
    ws = torch.empty(max(int(L.icrec_ir_metrics_workspace_bytes(Q)), 1), dtype=torch.uint8, device=dev)
    _native.check(L.icrec_ir_metrics(ptr(ranked_rows), depth, ptr(rel_off), ptr(rel_rows), Q, ptr(sums), ptr(pq), ptr(ws),
                                     ws.numel(), dev.index, stream_ptr(dev)), "icrec_ir_metrics")
    return sums, pq


def metrics_from_sums(sums) -> dict[str, float]:
    """The eight means from one or more double[9] sum vectors (passes add up); all 0.0 when no query counted."""
    total = np.sum(np.atleast_2d(np.asarray(sums, np.float64)), axis=0)
    n = total[8]
    return {key: (float(total[i] / n) if n > 0 else 0.0) for i, key in enumerate(METRIC_KEYS)}


def compute_ir_metrics_rows(ranked_rows: torch.Tensor, rel_off: torch.Tensor, rel_rows: torch.Tensor) -> dict[str, float]:
    """The eight-metric dict for ranked rows int64 [Q, depth] (-1 ends a list) against the relevant-row CSR."""
    sums, _ = ir_metrics_rows_raw(ranked_rows, rel_off, rel_rows)
    return metrics_from_sums(sums.cpu().numpy())


def compute_ir_metrics(query_rankings: dict[str, list[str]], relevant_docs: dict[str, set[str]],
                       device: str | torch.device = "cuda:0") -> dict[str, float]:
    """The reference's signature and keys.  Only the first 128 entries of a ranking are read: no metric looks past
    rank 100."""
    dev = _native.hip_device(device, "compute_ir_metrics")
    qids = [q for q in query_rankings if q in relevant_docs and relevant_docs[q]]
    if not qids:
        return {key: 0.0 for key in METRIC_KEYS}
    depth = max(1, min(_native.ICREC_MAX_K, max(len(query_rankings[q]) for q in qids)))
    row_of: dict[str, int] = {}
    ranked = np.full((len(qids), depth), -1, np.int64)
    for i, q in enumerate(qids):
        for p in relevant_docs[q]:
            row_of.setdefault(p, len(row_of))
        for j, p in enumerate(query_rankings[q][:depth]):
            ranked[i, j] = row_of.setdefault(p, len(row_of))
    off, rows = relevant_csr(qids, relevant_docs, row_of, dev)
    return compute_ir_metrics_rows(torch.from_numpy(ranked).to(dev), off, rows)
