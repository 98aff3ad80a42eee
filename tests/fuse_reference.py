"""icrec_fuse_select's definition (include/icrec.h) in plain numpy: one sequential loop per query, fp32 arithmetic
through np.float32.  Importing it needs no GPU."""
from __future__ import annotations

import numpy as np


def effective(w) -> np.ndarray:
    """The effective weights of a position table: w where w > 0 (+inf included), else +0.0 (NaN, negatives, -0)."""
    w = np.asarray(w, np.float32)
    out = np.zeros(w.shape, np.float32)
    keep = w > 0  # (a NaN fails the comparison)
    out[keep] = w[keep]
    return out


def live_entries(ids, gate, n_ids: int, excluded) -> dict[int, int]:
    """One query's list -> {id: position of its live entry}, in position order."""
    seen: dict[int, int] = {}
    for j, v in enumerate(ids):
        v = int(v)
        if not 0 <= v < n_ids:
            continue
        if gate is not None and not int(gate[j]) > 0:
            continue
        if v <= 2**31 - 1 and v in excluded:
            continue
        if v not in seen:  # the first passing occurrence wins
            seen[v] = j
    return seen


def fuse_select(a_idx, b_idx, a_w, b_w, top_k: int, n_ids: int, a_gate=None, b_gate=None, exclude=None):
    """-> (out_idx int64 [Q, top_k], out_score float32 [Q, top_k], out_pos int32 [Q, top_k, 2]).  exclude: None or per
    query an iterable of ids."""
    a_idx, b_idx = np.asarray(a_idx, np.int64), np.asarray(b_idx, np.int64)
    Q = a_idx.shape[0]
    ea, eb = effective(a_w), effective(b_w)
    out_idx = np.full((Q, top_k), -1, np.int64)
    out_score = np.zeros((Q, top_k), np.float32)
    out_pos = np.full((Q, top_k, 2), -1, np.int32)
    zero = np.float32(0.0)
    for q in range(Q):
        ex = set() if exclude is None else {int(v) for v in exclude[q]}
        la = live_entries(a_idx[q], None if a_gate is None else a_gate[q], n_ids, ex)
        lb = live_entries(b_idx[q], None if b_gate is None else b_gate[q], n_ids, ex)
        fused = []
        for v in set(la) | set(lb):
            pa, pb = la.get(v, -1), lb.get(v, -1)
            with np.errstate(over="ignore"):
                f = np.float32((ea[pa] if pa >= 0 else zero) + (eb[pb] if pb >= 0 else zero))
            fused.append((-float(f), v, f, pa, pb))  # float64 holds every fp32 value and orders -inf .. +inf alike
        fused.sort(key=lambda t: (t[0], t[1]))
        for i, (_, v, f, pa, pb) in enumerate(fused[:top_k]):
            out_idx[q, i], out_score[q, i], out_pos[q, i] = v, f, (pa, pb)
    return out_idx, out_score, out_pos
