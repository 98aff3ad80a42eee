"""icrec_compose_queries' definition (include/icrec.h) in numpy float32, over the oracle's arithmetic: the base is
oracle.normalize_rows (the 64 strided fmaf partials and the xor butterfly of the device's normalisation), the stored rows
are mmr_reference.stored_rows (rounded through bfloat16 for the bf16 storages), and a valid term adds (w * p) to the
accumulator with two float32 roundings - the product, then the sum - in list order.  Importing this needs no GPU."""
from __future__ import annotations

import numpy as np

from oracle import oracle
from tests.mmr_reference import stored_rows  # noqa: F401  (re-exported: the rows a test composes from)

F32 = np.float32


def term_valid(row, w, n_rows: int) -> bool:
    """0 <= row < n_rows and a finite weight."""
    return 0 <= int(row) < n_rows and bool(np.isfinite(F32(w)))


def base_part(base, base_w) -> np.ndarray:
    """acc before the first term for base float32 [Q, dim] and weights base_w float32 [Q] (None: every a = 1): a * q_hat,
    one float32 multiplication, where a weight that is not finite counts as 0."""
    q_hat = oracle.normalize_rows(np.ascontiguousarray(base, F32))
    a = np.ones(q_hat.shape[0], F32) if base_w is None else np.array(base_w, F32)
    a[~np.isfinite(a)] = 0.0
    return (a[:, None] * q_hat).astype(F32)


def add_terms(p_hat: np.ndarray, acc: np.ndarray, rows, weights, max_terms: int) -> np.ndarray:
    """One query: the valid ones of the first max_terms terms added to acc float32 [dim] in list order (weights None:
    all 1), each with two float32 roundings."""
    n_rows = p_hat.shape[0]
    acc = np.array(acc, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for t, row in enumerate(list(rows)[:max(int(max_terms), 0)]):
            w = F32(1.0) if weights is None else F32(weights[t])
            if not term_valid(row, w, n_rows):
                continue
            prod = (w * p_hat[int(row)]).astype(F32)
            acc = (acc + prod).astype(F32)
    assert acc.dtype == F32
    return acc


def compose_one(p_hat: np.ndarray, base, a, rows, weights, max_terms: int) -> np.ndarray:
    """One query: base float32 [dim] or None, a its weight (None: 1), the terms rows / weights (weights None: all 1) of
    which the first max_terms are read -> float32 [dim]."""
    dim = p_hat.shape[1]
    start = np.zeros(dim, F32) if base is None else base_part(np.reshape(base, (1, dim)), None if a is None else [a])[0]
    return add_terms(p_hat, start, rows, weights, max_terms)


def compose(p_hat: np.ndarray, base, base_w, off, rows, weights, max_terms: int) -> np.ndarray:
    """The CSR form icrec_compose_queries takes: base float32 [Q, dim] or None, base_w float32 [Q] or None, off int32
    [Q+1], rows int32, weights float32 or None -> float32 [Q, dim].  A segment whose end lies before its start is empty."""
    off = np.asarray(off, np.int64)
    Q = off.size - 1
    out = np.zeros((Q, p_hat.shape[1]), F32) if base is None else base_part(base, base_w)
    for i in range(Q):
        lo, hi = int(off[i]), int(off[i + 1])
        seg = slice(lo, max(hi, lo))
        out[i] = add_terms(p_hat, out[i], rows[seg], None if weights is None else weights[seg], max_terms)
    return out


def compose_lists(p_hat: np.ndarray, base, terms, base_w=None) -> np.ndarray:
    """The list form DeviceIndex.compose_queries takes: terms[i] None or a sequence of (row, weight) pairs, all read."""
    Q = len(terms)
    out = np.zeros((Q, p_hat.shape[1]), F32) if base is None else base_part(base, base_w)
    for i, t in enumerate(terms):
        pairs = list(t.items()) if hasattr(t, "items") else list(t or ())
        out[i] = add_terms(p_hat, out[i], [r for r, _ in pairs], [w for _, w in pairs], len(pairs))
    return out
