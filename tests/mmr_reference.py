"""icrec_mmr_select's definition (include/icrec.h) in numpy float32, over the oracle's arithmetic: the stored rows are
oracle.normalize_rows (rounded through bfloat16 for the bf16 storages), a query's similarity matrix is oracle.scores -
the un-normalising j-ascending fmaf chain - of its valid candidates' rows with themselves, and the greedy loop uses
np.float32 products and difference (three roundings, no fused multiply-add) under rerank's ordering rule.  Importing
this needs no GPU."""
from __future__ import annotations

import numpy as np

from oracle import oracle


def stored_rows(P, storage: str = "f32") -> np.ndarray:
    """The rows an index of `storage` holds for the host matrix P, as float32."""
    p_hat = oracle.normalize_rows(np.ascontiguousarray(P, np.float32))
    return oracle.round_bf16(p_hat) if storage.startswith("bf16") else p_hat


def ordered_first(values: np.ndarray, among: np.ndarray) -> int:
    """The position among the marked ones whose value is ordered first: a number before a NaN, the greater value
    (compared as floats, -0 == +0), the lower position; -1 when nothing is marked."""
    numbers = among & ~np.isnan(values)
    if numbers.any():
        return int(np.flatnonzero(numbers & (values == values[numbers].max()))[0])
    return int(np.flatnonzero(among)[0]) if among.any() else -1


def valid_candidates(cand: np.ndarray, n_rows: int, row_offset: int = 0) -> np.ndarray:
    local = cand.astype(np.int64) - row_offset
    return (cand >= 0) & (local >= 0) & (local < n_rows)


def select_positions(p_hat: np.ndarray, cand: np.ndarray, rel: np.ndarray, top_k: int, lam, row_offset: int = 0) -> list[int]:
    """One query: cand int64 [k], rel float32 [k] -> the picked positions j, in selection order (at most top_k)."""
    cand = np.asarray(cand, np.int64)
    rel = np.asarray(rel, np.float32)
    k = cand.size
    left = valid_candidates(cand, p_hat.shape[0], row_offset)
    sim = np.zeros((k, k), np.float32)
    where = np.flatnonzero(left)
    if where.size:
        rows = np.ascontiguousarray(p_hat[cand[where] - row_offset])
        sim[np.ix_(where, where)] = oracle.scores(rows, rows)
    lam = np.float32(lam)
    oml = np.float32(1.0) - lam
    maxsim = np.full(k, -np.inf, np.float32)
    picks: list[int] = []
    with np.errstate(invalid="ignore", over="ignore"):
        while len(picks) < top_k:
            value = rel if not picks else (lam * rel) - (oml * maxsim)  # float32 arrays: every operation rounds once
            assert value.dtype == np.float32
            j = ordered_first(value, left)
            if j < 0:
                break
            picks.append(j)
            left[j] = False
            maxsim = np.where(sim[j] > maxsim, sim[j], maxsim)
    return picks


def mmr_select(p_hat: np.ndarray, cand: np.ndarray, rel: np.ndarray, top_k: int, lam, row_offset: int = 0):
    """cand int64 [Q, k], rel float32 [Q, k] -> (idx int64 [Q, top_k] with -1 pads, rel float32 [Q, top_k] with 0 pads),
    what icrec_mmr_select returns for an index whose stored rows are p_hat (stored_rows)."""
    cand = np.asarray(cand, np.int64)
    rel = np.asarray(rel, np.float32)
    out_idx = np.full((cand.shape[0], top_k), -1, np.int64)
    out_rel = np.zeros((cand.shape[0], top_k), np.float32)
    for q in range(cand.shape[0]):
        picks = select_positions(p_hat, cand[q], rel[q], top_k, lam, row_offset)
        out_idx[q, :len(picks)] = cand[q, picks]
        out_rel[q, :len(picks)] = rel[q, picks]
    return out_idx, out_rel
