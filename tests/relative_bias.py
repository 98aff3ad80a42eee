"""Shared by tests/test_attention_bias.py (CPU), tests/test_attention_bias_gpu.py and tools/attention_bias_bench.py: the
encoder with a relative-position attention bias restated in torch, the two bias tables, the cases and the margins.

oracle/ knows no bias.  `encode` below is the encoder written from the math of oracle/float64_reference.py plus the one
term an MPNet layer adds:

    ctx_h = softmax(Q_h K_h^T / sqrt(d) + B_h) V_h        B_h[i, j] = table[h, 511 + (j - i)]   in EVERY layer

parameterised by dtype.  In float64 it is the truth.  The SAME code in float32 on the CPU gives E_ref, the error an fp32
implementation makes on the same inputs under tests/token_states.row_errors; a GPU result must meet `margin x E_ref`,
the margin coming from TOKEN_MARGINS / EMB_MARGINS, chosen from the ratios measured on the MI355X
(profiles/attention_bias_errors.md) by the rule of tests/token_states.py.  Without a table the function is the plain
encoder, and the GPU tests run bias-free cases through it under token_states.MARGINS: that checks this helper, not the
kernels.  It is why the linear layers are not a BLAS matmul (TorchBert._linear): with one accumulator per output the
float32 run errs as the fp32 C oracle does (within 3 % on the token states at both widths), with a blocked matmul it errs
half as much at hidden 768 and the bias-free cases miss token_states.MARGINS.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from instacart_next_order_recommendation_amd import relative_bias as rb
from instacart_next_order_recommendation_amd import synthetic as syn
from tests import token_states as ts
from tests.encoder_harness import packed

N_OFFSETS = 2 * rb.MAX_OFFSET + 1  # 1023
SHAPES = [(384, 6), (384, 1), (768, 2)]
TABLES = ("bucketed", "dense")
#: name -> (sequence lengths, the encoder's max_seq_length, seed of the ids): every key-tile and bucket edge, offsets to +-511
BATCHES = {"to256": ([1, 2, 31, 32, 33, 64, 65, 128, 129, 192, 193, 256], None, 21),
           "to512": ([257, 300, 511, 512], 512, 22)}

#: margin on E_ref per (gemm mode, hidden, weight set): (per-token-row rms, max abs) - TOKEN_MARGINS for the token states
#: of the biased cases, EMB_MARGINS for their pooled rows (mean and CLS embeddings: the helper pools with torch's
#: pairwise mean, the kernels add the tokens in order, so a pooled row's ratios are larger than its tokens').  Each is
#: the smallest of {2, 3, 4, 6, 8} that leaves 1.5x headroom over the worst ratio E_gpu / E_ref measured on the MI355X
#: over every case of tests/test_attention_bias_gpu.py (profiles/attention_bias_errors.md holds the ratios; the worst of
#: all is 5.13, under 8 / 1.5).
TOKEN_MARGINS = {
    ("f32", 384, "standard"): (2, 2), ("f32", 384, "sharp"): (2, 2),
    ("f32", 768, "standard"): (2, 2), ("f32", 768, "sharp"): (2, 2),
    ("f16x3", 384, "standard"): (3, 3), ("f16x3", 384, "sharp"): (3, 4),
    ("f16x3", 768, "standard"): (2, 2), ("f16x3", 768, "sharp"): (2, 2),
}
EMB_MARGINS = {
    ("f32", 384, "standard"): (6, 6), ("f32", 384, "sharp"): (6, 8),
    ("f32", 768, "standard"): (6, 6), ("f32", 768, "sharp"): (4, 6),
    ("f16x3", 384, "standard"): (6, 8), ("f16x3", 384, "sharp"): (6, 8),
    ("f16x3", 768, "standard"): (6, 6), ("f16x3", 768, "sharp"): (6, 6),
}


def bucket_weight(heads: int, seed: int = 31, lo: float = -4.0, hi: float = 4.0) -> np.ndarray:
    """A [32, heads] relative-attention embedding, uniform in [lo, hi]: the shape of a real model's."""
    u = syn.uniform(seed, 1, rb.NUM_BUCKETS * heads).reshape(rb.NUM_BUCKETS, heads)
    return (lo + (hi - lo) * u).astype(np.float32)


def table(name: str, heads: int, seed: int = 31, lo: float = -4.0, hi: float = 4.0) -> Optional[np.ndarray]:
    """float32 [heads, 1023], or None for "none".
    "bucketed": bucket_weight through the MPNet buckets.  "dense": all 1,023 offsets of every head independent, uniform
    in [lo, hi] - buckets hide an off-by-one beyond distance 8 and any error beyond +-128, this table does not.  Both are
    asymmetric in the sign of the offset and differ per head."""
    if name == "none":
        return None
    if name == "bucketed":
        return rb.table_from_buckets(bucket_weight(heads, seed, lo, hi))
    assert name == "dense", name
    u = syn.uniform(seed, 2, heads * N_OFFSETS).reshape(heads, N_OFFSETS)
    return (lo + (hi - lo) * u).astype(np.float32)


class TorchBert:
    """The blob's model in `dtype` on the CPU; encode() -> (last hidden state [T, H], mean-pooled + normalised [n, H])."""

    def __init__(self, blob: np.ndarray, shape, dtype=torch.float64):
        self.shape, self.dtype = shape, dtype
        sd = syn.blob_to_state_dict(np.asarray(blob, np.float32), shape)
        self.p = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd.items()}

    def _ln(self, v, name):
        mean = v.mean(-1, keepdim=True)
        var = ((v - mean) ** 2).mean(-1, keepdim=True)
        return (v - mean) / torch.sqrt(var + float(self.shape.ln_eps)) * self.p[name + ".weight"] + self.p[name + ".bias"]

    @staticmethod
    def _linear(t, weight, bias):
        """t W^T + b with ONE accumulator per output, the K products added in ascending order in the working dtype: what a
        kernel's MFMA chain and a C loop do.  (A BLAS matmul splits K into blocks with an accumulator each and adds the
        blocks at the end: in float32 it errs 2 - 2.5x less at K = 3,072 than any single-accumulator fp32 implementation,
        and E_ref would not be the error such an implementation makes.)"""
        acc = torch.zeros((t.shape[0], weight.shape[0]), dtype=t.dtype)
        tT, wT = t.T.contiguous(), weight.T.contiguous()
        for k in range(tT.shape[0]):
            acc.addcmul_(tT[k][:, None], wT[k][None, :])
        return acc + bias

    @torch.no_grad()
    def encode(self, ids: np.ndarray, cu: np.ndarray, table: Optional[np.ndarray] = None):
        s, p = self.shape, self.p
        H, nh = s.hidden, s.heads
        d = H // nh
        ids_t = torch.from_numpy(np.asarray(ids, np.int64))
        cu = np.asarray(cu, np.int64)
        pos = torch.from_numpy(np.concatenate([np.arange(b - a) for a, b in zip(cu[:-1], cu[1:])]))
        tbl = None if table is None else torch.from_numpy(np.asarray(table, np.float32)).to(self.dtype)
        assert tbl is None or tuple(tbl.shape) == (nh, N_OFFSETS)
        x = (p["embeddings.word_embeddings.weight"][ids_t] + p["embeddings.token_type_embeddings.weight"][0]
             + p["embeddings.position_embeddings.weight"][pos])
        x = self._ln(x, "embeddings.LayerNorm")
        for l in range(s.layers):
            q = f"encoder.layer.{l}."

            def lin(t, name):
                return self._linear(t, p[q + name + ".weight"], p[q + name + ".bias"])

            Q, K, V = lin(x, "attention.self.query"), lin(x, "attention.self.key"), lin(x, "attention.self.value")
            ctx = torch.empty_like(x)
            for a, b in zip(cu[:-1], cu[1:]):
                n = int(b - a)
                qh = Q[a:b].view(n, nh, d).transpose(0, 1)  # [heads, n, d]
                kh = K[a:b].view(n, nh, d).transpose(0, 1)
                vh = V[a:b].view(n, nh, d).transpose(0, 1)
                logits = qh @ kh.transpose(1, 2) * (1.0 / math.sqrt(d))  # [heads, n queries, n keys]
                if tbl is not None:
                    at = torch.arange(n)
                    logits = logits + tbl[:, rb.MAX_OFFSET + at[None, :] - at[:, None]]  # key - query
                ctx[a:b] = (torch.softmax(logits, dim=-1) @ vh).transpose(0, 1).reshape(n, H)
            x = self._ln(lin(ctx, "attention.output.dense") + x, q + "attention.output.LayerNorm")
            u = lin(x, "intermediate.dense")
            g = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
            x = self._ln(lin(g, "output.dense") + x, q + "output.LayerNorm")
        emb = torch.stack([x[a:b].mean(0) for a, b in zip(cu[:-1], cu[1:])])
        for _ in range(s.n_normalize):
            emb = emb / emb.norm(dim=1, keepdim=True).clamp(min=1e-12)
        return x.numpy(), emb.numpy()


def encode(blob, shape, ids, cu, table=None, dtype=torch.float64):
    """One-shot form of TorchBert(blob, shape, dtype).encode(ids, cu, table)."""
    return TorchBert(blob, shape, dtype).encode(ids, cu, table)


def normalize(v: np.ndarray, n: int) -> np.ndarray:
    """n times v / max(|v|_2, 1e-12) per row, in v's own precision."""
    for _ in range(n):
        v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), v.dtype.type(1e-12))
    return v


_refs: dict = {}


def reference(kind: str, hidden: int, layers: int, batch: str, table_name: str) -> dict:
    """Weights, inputs, table and both precisions' results of one case, computed once, shared and never changed:
    h64 / e64 the float64 token states / mean embeddings, h32 / e32 the float32 ones; c64 / c32 the CLS embeddings (the
    first-token rows, normalised n_normalize times)."""
    key = (kind, hidden, layers, batch, table_name)
    if key not in _refs:
        lens, max_len, seed = BATCHES[batch]
        s = ts.shape(hidden, layers)
        w = ts.weights(kind, s)
        ids, cu = packed(lens, seed, ts.VOCAB)
        tbl = table(table_name, s.heads)
        h64, e64 = encode(w, s, ids, cu, tbl, torch.float64)
        h32, e32 = encode(w, s, ids, cu, tbl, torch.float32)
        first = cu[:-1].astype(np.int64)
        for a in (h64, e64, h32, e32):
            a.setflags(write=False)
        _refs[key] = dict(s=s, w=w, ids=ids, cu=cu, kind=kind, max_len=max_len, table=tbl, table_name=table_name,
                          h64=h64, e64=e64, h32=h32, e32=e32, c64=normalize(np.ascontiguousarray(h64[first]), s.n_normalize),
                          c32=normalize(np.ascontiguousarray(h32[first]), s.n_normalize))
    return _refs[key]


def margins(r: dict, mode: str, what: str = "tokens"):
    """(rms, max abs) margins of case r: TOKEN_MARGINS / EMB_MARGINS (what = "tokens" / "embeddings") with a table;
    without one token_states.MARGINS, which were measured on per-token rows against the C oracle's E_ref (the helper's own
    check: tokens only)."""
    if r["table"] is None:
        assert what == "tokens"
        return ts.MARGINS[(mode, r["s"].hidden, r["kind"])]
    return (TOKEN_MARGINS if what == "tokens" else EMB_MARGINS)[(mode, r["s"].hidden, r["kind"])]


def check(what: str, got: np.ndarray, want64: np.ndarray, ref32: np.ndarray, margin, cu=None):
    """Prints `RATIO ...` (E_gpu / E_ref, rms and max abs), then asserts E_gpu <= margin x E_ref for both."""
    e_rms, e_abs = ts.row_errors(ref32, want64)
    g_rms, g_abs = ts.row_errors(got, want64)
    assert e_rms > 0 and e_abs > 0
    print(f"RATIO {what}: E_gpu rms {g_rms:.3e} abs {g_abs:.3e}, E_ref rms {e_rms:.3e} abs {e_abs:.3e}, "
          f"ratio rms {g_rms / e_rms:.2f} abs {g_abs / e_abs:.2f} (margins {margin[0]} / {margin[1]})")
    where = "" if cu is None else ts.worst_element(got, want64, cu)
    assert g_rms <= margin[0] * e_rms and g_abs <= margin[1] * e_abs, (what, where)
