"""Shared by tests/test_cls_pooling.py (CPU) and tests/test_cls_pooling_gpu.py: the cases of the CLS-pooling comparison
against the references, and the references themselves.

Nothing in oracle/ knows about CLS pooling, and nothing there needs to: Pooling(cls) IS the last hidden state of each
sequence's first token, so the fp32 reference is rows cu[:-1] of `oracle.encode(..., return_hidden=True)` passed
n_normalize times through `oracle.normalize_rows`, and the float64 reference is the same rows of
oracle/float64_reference.py's token states, normalised in float64.  The bound a GPU result must meet is
`margin x E_ref` under tests/token_states.py's metric, E_ref being the fp32 reference's own error against the float64
one on the same inputs.
"""
from __future__ import annotations

import numpy as np

from tests import token_states as ts
from tests.encoder_harness import packed

#: (hidden, layers): 6 layers and 1 layer at hidden 384 (with one layer the pruned layer is also layer 0), 2 at 768
SHAPES = [(384, 6), (384, 1), (768, 2)]
#: name -> (sequence lengths of one batch, the encoder's max_seq_length, seed of the ids)
BATCHES = {"to256": ([1, 2, 31, 32, 33, 64, 128, 256], None, 2), "to512": ([257, 300, 512], 512, 3)}
N_NORMALIZE = (1, 2)

#: margin on E_ref per (gemm mode, hidden, weight set), (rms, max abs): token_states.MARGINS, which were measured on
#: per-token rows.  The ratios E_gpu / E_ref of the normalised CLS rows measured on the MI355X
#: (profiles/cls_pooling_errors.md) stay under every entry divided by 1.5, so none is replaced here.
MARGINS = dict(ts.MARGINS)

_refs: dict = {}


def normalize64(v: np.ndarray, n: int) -> np.ndarray:
    """n times v / max(|v|_2, 1e-12) per row, in float64."""
    v = np.asarray(v, np.float64)
    for _ in range(n):
        v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    return v


def reference(kind: str, hidden: int, layers: int, batch: str) -> dict:
    """Weights, inputs and both references' hidden states of one case, computed once and shared.  `cls64[n]` /
    `mean64[n]` are the float64 CLS / mean embeddings under n normalisations, `cls32[n]` the fp32 oracle's CLS
    embeddings."""
    key = (kind, hidden, layers, batch)
    if key not in _refs:
        from oracle import float64_reference as f64
        from oracle import oracle

        lens, max_len, seed = BATCHES[batch]
        s = ts.shape(hidden, layers)
        w = ts.weights(kind, s)
        ids, cu = packed(lens, seed, ts.VOCAB)
        want_h, _ = f64.encode(w, s, ids, cu)
        want_h = np.asarray(want_h, np.float64)
        _, ora_h = oracle.encode(w, oracle.cfg_for(s), ids, cu, return_hidden=True)
        first = cu[:-1].astype(np.int64)
        mean_h = np.stack([want_h[cu[i]:cu[i + 1]].mean(0) for i in range(cu.size - 1)])
        cls32 = {0: np.ascontiguousarray(ora_h[first])}
        for n in range(1, max(N_NORMALIZE) + 1):
            cls32[n] = oracle.normalize_rows(cls32[n - 1])
        _refs[key] = dict(s=s, w=w, ids=ids, cu=cu, kind=kind, max_len=max_len, want_h=want_h, ora_h=ora_h,
                          cls64={n: normalize64(want_h[first], n) for n in N_NORMALIZE},
                          mean64={n: normalize64(mean_h, n) for n in N_NORMALIZE},
                          cls32=cls32)
    return _refs[key]


def bound(r: dict, mode: str, n_norm: int):
    """(rms bound, max-abs bound, E_ref rms, E_ref abs) for the CLS embeddings of case r under n_norm normalisations."""
    e_rms, e_abs = ts.row_errors(r["cls32"][n_norm], r["cls64"][n_norm])
    m_rms, m_abs = MARGINS[(mode, r["s"].hidden, r["kind"])]
    return m_rms * e_rms, m_abs * e_abs, e_rms, e_abs
