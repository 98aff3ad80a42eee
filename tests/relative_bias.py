"""Shared by tests/test_attention_bias.py (CPU), tests/test_attention_bias_gpu.py and tools/attention_bias_bench.py: the
two bias tables and the cases of the comparison against the reference.

The reference is oracle/float64_reference.py with the table as `attention_bias`: in float64 the truth, the SAME code in
float32 (one accumulator per linear-layer output, see there) E_ref, the error an fp32 implementation makes on the same
inputs under tests/token_states.row_errors.  A GPU result must meet `margin x E_ref` (token_states.check), the margin
coming from token_states.TOKEN_MARGINS / EMB_MARGINS.  Without a table the reference is the plain encoder, and the GPU
tests run bias-free cases through its float32 form under token_states.MARGINS - margins measured against the fp32 C
oracle's E_ref: that checks the float32 reference, not the kernels.  It is why the float32 linear layers are not a BLAS
matmul: with one accumulator per output the float32 run errs as the fp32 C oracle does (within 3 % on the token states
at both widths), with a blocked matmul it errs half as much at hidden 768 and the bias-free cases miss
token_states.MARGINS.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from instacart_next_order_recommendation_amd import relative_bias as rb
from instacart_next_order_recommendation_amd import synthetic as syn
from tests import token_states as ts

N_OFFSETS = 2 * rb.MAX_OFFSET + 1  # 1023
SHAPES = [(384, 6), (384, 1), (768, 2)]
TABLES = ("bucketed", "dense")
#: name -> (sequence lengths, the encoder's max_seq_length, seed of the ids): every key-tile and bucket edge, offsets to +-511
BATCHES = {"to256": ([1, 2, 31, 32, 33, 64, 65, 128, 129, 192, 193, 256], None, 21),
           "to512": ([257, 300, 511, 512], 512, 22)}


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


def reference(kind: str, hidden: int, layers: int, batch: str, table_name: str) -> dict:
    """token_states.reference of a named case; E_ref is the float32 reference's error, also for table "none"."""
    lens, max_len, seed = BATCHES[batch]
    return ts.reference(kind, hidden, layers, lens, seed, max_len, table(table_name, ts.WIDTHS[hidden]["heads"]), ref32="float32")


def margins(r: dict, mode: str, what: str = "tokens"):
    """(rms, max abs) margins of case r: TOKEN_MARGINS / EMB_MARGINS (what = "tokens" / "embeddings") with a table;
    without one token_states.MARGINS, which were measured on per-token rows against the C oracle's E_ref (the float32
    reference's own check: tokens only)."""
    if r["table"] is None:
        assert what == "tokens"
        return ts.MARGINS[(mode, r["s"].hidden, r["kind"])]
    return (ts.TOKEN_MARGINS if what == "tokens" else ts.EMB_MARGINS)[(mode, r["s"].hidden, r["kind"])]
