"""The MPNet family's relative-position attention bias on the host.

transformers' MPNetEncoder adds `relative_attention_bias(bucket(key - query))[head]` to every attention logit of every
layer: one embedding table [num_buckets, heads] shared by all layers, indexed by a T5-style bucket of the offset
(half the buckets per sign; in each half the first ones hold one offset each, the rest grow logarithmically up to
max_distance, beyond which every offset falls into the last).  The device takes the bias per offset
(icrec_encoder_set_attention_bias: [heads, 2 * 512 - 1]); this module turns the one into the other.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native

MAX_OFFSET = _native.ICREC_MAX_SEQLEN - 1  # offsets -511 .. +511
NUM_BUCKETS, MAX_DISTANCE = 32, 128        # MPNetEncoder's defaults (compute_position_bias passes no max_distance)


def relative_position_bucket(offset, num_buckets: int = NUM_BUCKETS, max_distance: int = MAX_DISTANCE) -> np.ndarray:
    """The bucket of `offset` = key position - query position (int array), as MPNetEncoder.relative_position_bucket
    computes it - the logarithm in float32, as torch does there, so that offsets on a bucket edge fall the same way."""
    rel = np.asarray(offset, np.int64)
    n = -rel
    half = num_buckets // 2
    ret = (n < 0).astype(np.int64) * half
    n = np.abs(n)
    max_exact = half // 2
    # torch: log(n.float() / max_exact) / math.log(max_distance / max_exact) * (half - max_exact), float32 throughout
    # (offsets below max_exact take their own bucket: the logarithm is not used for them)
    nf = np.maximum(n, max_exact).astype(np.float32)
    q = np.log(nf / np.float32(max_exact)) / np.float32(math.log(max_distance / max_exact))
    large = max_exact + (q * np.float32(half - max_exact)).astype(np.int64)
    large = np.minimum(large, half - 1)
    return ret + np.where(n < max_exact, n, large)


def table_from_buckets(weight: np.ndarray, max_distance: int = MAX_DISTANCE) -> np.ndarray:
    """weight float[num_buckets, heads] (encoder.relative_attention_bias.weight) -> float32 [heads, 2 * 512 - 1]: entry
    [h, 511 + o] is the bias of offset o = key - query."""
    w = np.asarray(weight, np.float32)
    if w.ndim != 2:
        raise ValueError(f"relative_attention_bias.weight must be [num_buckets, heads], got {w.shape}")
    b = relative_position_bucket(np.arange(-MAX_OFFSET, MAX_OFFSET + 1), w.shape[0], max_distance)
    return np.ascontiguousarray(w[b].T)
