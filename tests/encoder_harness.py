"""Shared by the encoder tests (tests/test_*_gpu.py, tests/token_states.py): how an encoder is created under ICREC_*
settings, how a packed batch is made, run and given to the oracle, and the embedding tolerance.  One definition each;
nothing here is specific to one test file."""
from __future__ import annotations

import numpy as np

from oracle import oracle

# Tolerance for embeddings (unit vectors): fp32 everywhere, GEMM / LayerNorm / pooling orders are
# identical to the oracle's; the only differences are expf / erff (device libm vs glibc) by a few ulp.
EMB_TOL = 5e-6


def make_encoder(monkeypatch, w, shape, mode="f16x3", max_seq_length=None, **env):
    """An encoder created under the given ICREC_* settings: they are read once, at creation, and unset again here
    (also when creation raises)."""
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return DeviceEncoder(w, shape, gemm_mode=mode, max_seq_length=max_seq_length)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def run(enc, ids, cu, **kw):
    """encode_packed on host arrays -> numpy; `kw` (cu_host=, return_tokens=) goes through.  With return_tokens the
    result is the tuple (embeddings, token states)."""
    import torch

    out = enc.encode_packed(torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), int(np.diff(cu).max()), **kw)
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


def packed(lens, seed, vocab_size):
    """Random ids in [0, vocab_size) for sequences of the given lengths -> (ids int32[T], cu int32[n+1])."""
    rng = np.random.default_rng(seed)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rng.integers(0, vocab_size, int(cu[-1])).astype(np.int32), cu


def oracle_rows(w, shape, ids, cu, rows=None):
    """Oracle embeddings of `rows` (default all) of the packed batch; the oracle is batch-invariant."""
    cfg = oracle.cfg_for(shape)
    if rows is None:
        return oracle.encode(w, cfg, ids, cu)
    sub_ids = np.concatenate([ids[cu[r]:cu[r + 1]] for r in rows])
    sub_cu = np.concatenate([[0], np.cumsum([cu[r + 1] - cu[r] for r in rows])]).astype(np.int32)
    return oracle.encode(w, cfg, sub_ids, sub_cu)


def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def round_plus_remainder(enc, cu, lo, hi, first=1):
    """(n, main_tokens, tail_tokens) of the first prefix of the batch, of at least `first` sequences, that
    enc.batch_split cuts into whole rounds (64 tokens per CU) + a remainder of lo .. hi tokens."""
    for n in range(first, cu.size):
        main_t, tail_t = enc.batch_split(cu[n])
        if lo <= tail_t <= hi:
            return n, main_t, tail_t
    raise AssertionError(f"no prefix with a remainder in [{lo}, {hi}]")
