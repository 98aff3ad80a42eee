"""Shared by the encoder tests (tests/test_*_gpu.py, tests/token_states.py): how an encoder is created under ICREC_*
settings, the named dispatch forms, how a packed batch is made, run and given to the oracle, the embedding tolerance,
and the bodies of the poisoned-workspace and graph-capture tests.  One definition each; nothing here is specific to one
test file."""
from __future__ import annotations

import numpy as np

from oracle import oracle

# Tolerance for embeddings (unit vectors): fp32 everywhere, GEMM / LayerNorm / pooling orders are
# identical to the oracle's; the only differences are expf / erff (device libm vs glibc) by a few ulp.
EMB_TOL = 5e-6

#: the named dispatch forms every "same bits" test runs; a test adds the ICREC_SMALL_M values its shapes need
FORMS = [("default", {}), ("unfused", {"ICREC_FUSE": 0}), ("one_stream", {"ICREC_SIDE_STREAM": 0})]


def make_encoder(monkeypatch, w, shape, mode="f16x3", max_seq_length=None, pooling=None, attention_bias=None, **env):
    """An encoder created under the given ICREC_* settings: they are read once, at creation, and unset again here
    (also when creation raises).  `pooling` and `attention_bias` reach DeviceEncoder only when given."""
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    kw = {k: v for k, v in (("pooling", pooling), ("attention_bias", attention_bias)) if v is not None}
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        enc = DeviceEncoder(w, shape, gemm_mode=mode, max_seq_length=max_seq_length, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    assert enc.has_attention_bias == (attention_bias is not None)
    return enc


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


def long_mixed_lens(n, seed):
    """n sequence lengths of 1-256 tokens with one of 257-512 at every twelfth place."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    _, cu = syn.synthetic_token_batch(n, seed=seed, mean_len=90, std_len=60, lo=1, hi=256)
    lens = np.diff(cu)
    long_at = np.arange(3, n, 12)
    lens[long_at] = np.linspace(257, 512, long_at.size).astype(np.int64)
    return lens.tolist()


def long_rounds_plus_remainder(monkeypatch, w, shape, vocab_size, **enc_kw):
    """(ids, cu, (main_tokens, tail_tokens)): the first prefix of long_mixed_lens(420, 11), of more than 64 sequences,
    that an f16x3 encoder with max_seq_length 512 cuts into whole rounds plus a remainder (the side stream's range);
    at least three of its sequences are longer than 256 tokens."""
    lens = long_mixed_lens(420, seed=11)
    probe = make_encoder(monkeypatch, w, shape, max_seq_length=512, **enc_kw)
    n, main_t, tail_t = round_plus_remainder(probe, np.concatenate([[0], np.cumsum(lens)]), 1, np.inf, first=64)
    probe.close()
    assert tail_t and main_t > 0 and n > 64, (main_t, tail_t, n)
    ids, cu = packed(lens[:n], 4, vocab_size)
    assert (np.diff(cu) > 256).sum() >= 3
    return ids, cu, (main_t, tail_t)


def poisoned_runs(enc, ids, cu, fills=(0xFF, 0x00, 0x7F), tokens=False):
    """The batch encoded once per fill byte, every byte of the workspace (and, with `tokens`, of the tokens_out buffer)
    holding that byte before the call: every byte a kernel reads must have been written by the same call.  Asserts that
    the workspace has the size the library asked for, that no result holds a NaN or Inf and that every fill gives the
    same bits; returns the results of the first fill, (embeddings,) or (embeddings, token states)."""
    import torch

    from instacart_next_order_recommendation_amd import _native

    args = (torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), int(np.diff(cu).max()))
    enc.encode_packed(*args)  # sizes the workspace
    ws = enc._ws_by_stream[torch.cuda.current_stream().cuda_stream]  # the caller's stream's block
    assert ws.numel() == _native.lib().icrec_encode_workspace_bytes(enc._h, int(cu[-1]), cu.size - 1)
    buf = torch.empty((int(cu[-1]), enc.shape.hidden), dtype=torch.float32, device="cuda") if tokens else None
    first = None
    for fill in fills:
        ws.fill_(fill)
        if tokens:
            buf.view(torch.uint8).fill_(fill)
            emb, tok = enc.encode_packed(*args, return_tokens=True, tokens_out=buf)
            assert tok.data_ptr() == buf.data_ptr()
            got = (emb.cpu().numpy(), tok.cpu().numpy())
        else:
            got = (enc.encode_packed(*args).cpu().numpy(),)
        first = got if first is None else first
        for a, b in zip(got, first):
            assert np.isfinite(a).all(), f"byte 0x{fill:02X} leaked into the results"
            np.testing.assert_array_equal(a, b, err_msg=f"fill 0x{fill:02X} against 0x{fills[0]:02X}")
    return first


def replay_matches_eager(enc, ids, cu, tokens=False):
    """encode_into is capturable: warmed up on a side stream (as fastpath.py does), captured with a workspace of its
    own, then - outputs zeroed, workspace full of 0xFF - replayed ONCE: the graph writes the eager call's bits (with
    `tokens`, also every token's state)."""
    import torch

    d_ids, d_cu = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    n, T, mx = cu.size - 1, int(cu[-1]), int(np.diff(cu).max())
    eager = enc.encode_packed(d_ids, d_cu, mx, return_tokens=tokens)
    eager = [e.cpu().numpy() for e in (eager if tokens else (eager,))]
    out = torch.zeros((n, enc.shape.hidden), dtype=torch.float32, device="cuda")
    buf = torch.zeros((T, enc.shape.hidden), dtype=torch.float32, device="cuda") if tokens else None
    ws = torch.empty(enc._ws_by_stream[torch.cuda.current_stream().cuda_stream].numel(), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        enc.encode_into(d_ids, d_cu, n, T, mx, out, ws, tokens=buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enc.encode_into(d_ids, d_cu, n, T, mx, out, ws, tokens=buf)
    out.zero_(); ws.fill_(0xFF)
    if tokens:
        buf.zero_()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), eager[0])
    if tokens:
        np.testing.assert_array_equal(buf.cpu().numpy(), eager[1])
