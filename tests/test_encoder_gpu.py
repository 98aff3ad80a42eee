"""HIP encoder (through the C ABI) against the CPU oracle and the transformers.BertModel goldens."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle
from tests.encoder_harness import EMB_TOL, make_encoder, packed, poisoned_runs, round_plus_remainder, run

pytestmark = pytest.mark.gpu

# north_star: cosine scores within 1e-4 of the fp32 reference
COS_TOL = 1e-4


@pytest.fixture(scope="module", params=["f32", "f16x3"])
def encoder(request, minilm_weights):
    """Both GEMM modes: exact f32 MFMA, and the 3-term f16 split (fp32-level accuracy by construction:
    <= 3*2^-22 relative per product; measured max |d emb| vs the oracle is printed by the tests)."""
    import torch

    assert torch.cuda.is_available()
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    return DeviceEncoder(minilm_weights, gemm_mode=request.param)


def test_golden_short_batch(encoder, golden_encoder):
    g = golden_encoder
    emb = run(encoder, g["ids"], g["cu_seqlens"])
    print(f"[{encoder.gemm_mode}] max|emb - oracle| = {np.abs(emb - g['oracle_embeddings']).max():.3e}")
    assert np.abs(emb - g["oracle_embeddings"]).max() < EMB_TOL
    assert np.abs(emb - g["hf_embeddings"]).max() < EMB_TOL          # transformers.BertModel output
    assert np.abs((emb * g["hf_embeddings"]).sum(1) - 1).max() < COS_TOL


def test_golden_long_sequences(encoder, golden_encoder):
    g = golden_encoder
    emb = run(encoder, g["ids_long"], g["cu_seqlens_long"])
    print(f"[{encoder.gemm_mode}] long: max|emb - oracle| = {np.abs(emb - g['oracle_embeddings_long']).max():.3e}")
    assert np.abs(emb - g["oracle_embeddings_long"]).max() < EMB_TOL
    assert np.abs(emb - g["hf_embeddings_long"]).max() < EMB_TOL


@pytest.mark.parametrize("lens", [[1], [2, 1, 3], [31, 32, 33], [63, 64, 65, 5], [127, 128, 129], [255, 256, 17],
                                  [159, 160, 161], [191, 192, 193, 96], [223, 224, 225]])
def test_ragged_lengths_vs_oracle(encoder, minilm_weights, lens):
    """Tile-boundary lengths for every attention bucket (1 / 2 / 3-4 / 5-6 / 7-8 key tiles), mixed in one batch."""
    ids, cu = packed(lens, sum(lens), 30522)
    want = oracle.encode(minilm_weights, oracle.make_cfg(), ids, cu)
    got = run(encoder, ids, cu)
    assert np.abs(got - want).max() < EMB_TOL


def test_batch_invariance_bitwise(encoder):
    """A sequence encodes to the same bits alone and inside a batch (packed, no cross-talk)."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    ids, cu = syn.synthetic_token_batch(6, seed=21, mean_len=40, std_len=30, lo=2, hi=150)
    full = run(encoder, ids, cu)
    for s in [0, 3, 5]:
        one = run(encoder, ids[cu[s]:cu[s + 1]].copy(), np.array([0, cu[s + 1] - cu[s]], np.int32))
        np.testing.assert_array_equal(one[0], full[s])


def test_attention_bucket_boundaries_alone_equal_in_batch(encoder):
    """Batches put sequences of 5-6 key tiles through the 6-wave kernel, a lone sequence of the same length goes
    through the 8-tile one (and 3-4 tiles through the 4-tile one either way): the same bits on both sides of every
    bucket boundary."""
    lens = [96, 97, 128, 129, 160, 161, 192, 193, 224, 256]
    ids, cu = packed(lens, 5, 30522)
    full = run(encoder, ids, cu)
    for s, n in enumerate(lens):
        one = run(encoder, ids[cu[s]:cu[s + 1]].copy(), np.array([0, n], np.int32))
        np.testing.assert_array_equal(one[0], full[s], err_msg=f"length {n}")


def test_small_and_batch_gemm_paths_agree_bitwise(encoder, minilm_weights, monkeypatch):
    """Calls of up to 3,584 tokens take the latency-form kernels (32-token x 64-feature workgroups, a launch per GEMM),
    larger batches the layer kernel (one 64-token workgroup per CU): a request must encode to the same bits through
    either (same per-output MFMA chains, same LayerNorm tree) - alone, inside a 6,000-token batch, and inside a
    2,400-token batch whichever of the two forms that batch is given (ICREC_SMALL_M at encoder creation)."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    ids, cu = syn.synthetic_token_batch(60, seed=33, mean_len=100, std_len=40, lo=5, hi=256)
    assert cu[-1] > 3584 + 512
    full = run(encoder, ids, cu)
    for s in [0, 7, 23, 59]:
        n = int(cu[s + 1] - cu[s])
        one = run(encoder, ids[cu[s]:cu[s + 1]].copy(), np.array([0, n], np.int32))
        np.testing.assert_array_equal(one[0], full[s])
    mid_ids, mid_cu = ids[:cu[24]].copy(), cu[:25].copy()
    assert 1024 < mid_cu[-1] <= 3584
    mid = run(encoder, mid_ids, mid_cu)                       # latency form
    np.testing.assert_array_equal(mid, full[:24])
    # the same 2,400 tokens through the layer kernel
    batch_form = make_encoder(monkeypatch, minilm_weights, syn.BertShape(), encoder.gemm_mode, ICREC_SMALL_M=512)
    np.testing.assert_array_equal(run(batch_form, mid_ids, mid_cu), mid)
    batch_form.close()


def test_n_normalize_variants(minilm_weights):
    """n_normalize = 0 (raw mean pool) and 1 match the oracle; 2 is the default path."""
    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    ids, cu = syn.synthetic_token_batch(2, seed=3, mean_len=10, std_len=3, lo=3, hi=20)
    for nn in (0, 1):
        shape = syn.BertShape(n_normalize=nn)
        enc = DeviceEncoder(minilm_weights, shape)
        got = run(enc, ids, cu)
        want = oracle.encode(minilm_weights, oracle.cfg_for(shape), ids, cu)
        assert np.abs(got - want).max() < (2e-5 if nn == 0 else EMB_TOL)
        enc.close()


def test_encode_ids_chunking(encoder):
    """encode_ids splits long inputs into several calls and keeps input order."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    ids, cu = syn.synthetic_token_batch(40, seed=9, mean_len=20, std_len=8, lo=4, hi=40)
    seqs = [ids[cu[i]:cu[i + 1]].tolist() for i in range(40)]
    a = encoder.encode_ids(seqs).cpu().numpy()
    b = encoder.encode_ids(seqs, max_tokens_per_call=100).cpu().numpy()
    np.testing.assert_array_equal(a, b)


def test_bad_arguments_raise(encoder, minilm_weights):
    import torch
    from instacart_next_order_recommendation_amd._native import IcrecError
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    with pytest.raises(ValueError):
        DeviceEncoder(minilm_weights[:-1])
    ids = torch.zeros(300, dtype=torch.int32).cuda()
    cu = torch.tensor([0, 300], dtype=torch.int32).cuda()
    with pytest.raises(IcrecError):
        encoder.encode_packed(ids, cu, 300)  # longer than max_seq_length 256
    with pytest.raises(ValueError):
        encoder.encode_ids([[1, 2, 40000]])  # id outside the vocab


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_wide_dynamic_range(mode):
    """Weights 4x larger than BERT's init and LayerNorm gains of ~3: hidden activations reach tens,
    FFN intermediates hundreds, attention is sharply peaked; tiny-magnitude weights ride along in the
    same matrices.  The f16x3 split must stay at fp32-level agreement with the oracle."""
    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    shape = syn.BertShape(vocab_size=2048, layers=2)
    w = syn.synthetic_bert_weights(shape, seed=9, std=0.2)
    sd = syn.blob_to_state_dict(w, shape)           # views into w
    for name, a in sd.items():
        if name.endswith("LayerNorm.weight"):
            a *= 3.0
        if name.endswith("intermediate.dense.weight"):
            a[::7] *= 1e-4                            # rows of very small weights next to large ones
    ids, cu = syn.synthetic_token_batch(5, seed=2, mean_len=60, std_len=40, lo=3, hi=200, vocab_size=2048)
    want, hid = oracle.encode(w, oracle.cfg_for(shape), ids, cu, return_hidden=True)
    assert np.abs(hid).max() > 5.0                   # the stress actually stresses
    enc = DeviceEncoder(w, shape, gemm_mode=mode)
    got = run(enc, ids, cu)
    err = np.abs(got - want).max()
    print(f"[{mode}] wide-range max|emb - oracle| = {err:.3e}, max|hidden| = {np.abs(hid).max():.1f}")
    assert err < EMB_TOL
    enc.close()


def test_two_stream_split_is_bitwise_identical(encoder):
    """encode_packed with cu_host splits a large batch over two HIP streams: same bits as one call."""
    import torch
    from instacart_next_order_recommendation_amd import synthetic as syn

    ids, cu = syn.synthetic_token_batch(300, seed=4, mean_len=120, std_len=50, lo=4, hi=256)
    i_d, c_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    mx = int(np.diff(cu).max())
    one = encoder.encode_packed(i_d, c_d, mx).cpu().numpy()
    for _ in range(2):
        two = encoder.encode_packed(i_d, c_d, mx, cu_host=cu).cpu().numpy()
        np.testing.assert_array_equal(one, two)


@pytest.mark.parametrize("n_seqs", [19, 60, 400])
def test_fused_layer_kernels_equal_unfused_bitwise(minilm_weights, monkeypatch, n_seqs):
    """Batches above 3,584 tokens (60 and 400 sequences here; the 19 take the latency-form kernels, whose LayerNorms are
    folded into the GEMMs - also compared) run the activation-resident QKV kernel, attention with the longest-first dispatch
    order, attention-out + residual + LN and the whole FFN block (up, GELU, down, residual, LN) as fused kernels.
    An encoder created under ICREC_FUSE=0 (the switch is read once, at icrec_encoder_create) runs the UNFUSED
    reference chain: slab-ring QKV, attention in batch order, separate GEMM / LayerNorm launches.  Same per-output
    MFMA chains and the same LayerNorm order => identical bits (400 sequences: several rounds of workgroups)."""
    import torch

    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    enc = DeviceEncoder(minilm_weights, gemm_mode="f16x3")
    ref = make_encoder(monkeypatch, minilm_weights, syn.BertShape(), ICREC_FUSE=0)
    ids, cu = syn.synthetic_token_batch(n_seqs, seed=5, mean_len=90, std_len=60, lo=3, hi=256)
    assert int(cu[-1]) > {19: 512, 60: 3584, 400: 2 * 64 * 256}[n_seqs]
    mx = int(np.diff(cu).max())
    args = (torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), mx)
    fused = enc.encode_packed(*args).cpu().numpy()
    other = ref.encode_packed(*args).cpu().numpy()
    np.testing.assert_array_equal(fused, other)
    monkeypatch.setenv("ICREC_FUSE", "0")   # set AFTER creation: not read on the hot path, nothing changes
    np.testing.assert_array_equal(enc.encode_packed(*args).cpu().numpy(), fused)
    enc.close()
    ref.close()


@pytest.mark.parametrize("lens", [[99], [1], [33, 1, 32, 31, 64, 200], [256, 255], [150] * 22 + [7, 201]])
def test_small_batches_with_layernorms_folded_into_the_gemms_bitwise(minilm_weights, monkeypatch, lens):
    """Up to 3,584 tokens the two LayerNorms of a layer are the prologues of the GEMMs that consume them
    (wt_linear_lnin_kernel: FFN-up, the next layer's QKV projection; the last layer's FFN LayerNorm stays a kernel) -
    11 graph nodes fewer per request.  ICREC_FUSE=0 keeps the separate ln_wt_kernel launches: same arithmetic thread for
    thread => identical bits; rows of a 32-token block past the end of the batch never reach a real row."""
    import torch

    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    enc = DeviceEncoder(minilm_weights, gemm_mode="f16x3")
    ref = make_encoder(monkeypatch, minilm_weights, syn.BertShape(), ICREC_FUSE=0)
    rng = np.random.default_rng(len(lens))
    ids = rng.integers(1000, 30000, size=int(np.sum(lens))).astype(np.int32)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    assert int(cu[-1]) <= 3584
    args = (torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), int(max(lens)))
    got = enc.encode_packed(*args).cpu().numpy()
    want = ref.encode_packed(*args).cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got, want)
    enc.close(); ref.close()


def test_side_stream_changes_nothing(minilm_weights, monkeypatch):
    """A batch of whole 64-token-per-CU rounds + a short remainder: the remainder's small-batch kernels and the short
    attention buckets run on the library's side stream (fork / join by events inside icrec_encode).
    An encoder created under ICREC_SIDE_STREAM=0 keeps every kernel on the caller's stream: same bits, and repeated calls stay identical."""
    import torch

    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    enc = DeviceEncoder(minilm_weights, gemm_mode="f16x3")
    ids, cu = syn.synthetic_token_batch(400, seed=11, mean_len=90, std_len=60, lo=3, hi=256)
    n, main_t, tail_t = round_plus_remainder(enc, cu, 1, np.inf, first=64)
    assert tail_t and main_t % (64 * 256) == 0 and n >= 64, (main_t, tail_t, n)
    ids, cu = ids[: cu[n]], cu[: n + 1]
    mx = int(np.diff(cu).max())
    assert mx > 128  # a long attention bucket exists: the shorter ones go to the side stream
    args = (torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), mx)
    a = enc.encode_packed(*args).cpu().numpy()
    b = enc.encode_packed(*args).cpu().numpy()
    enc_one_stream = make_encoder(monkeypatch, minilm_weights, syn.BertShape(), ICREC_SIDE_STREAM=0)
    c = enc_one_stream.encode_packed(*args).cpu().numpy()
    enc_one_stream.close()
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
    # no remainder rule: the same tokens as a partial round of the batch kernels
    enc_no_tail = make_encoder(monkeypatch, minilm_weights, syn.BertShape(), ICREC_TAIL_M=0)
    np.testing.assert_array_equal(enc_no_tail.encode_packed(*args).cpu().numpy(), a)
    enc_no_tail.close()
    # the remainder's sequences encode to the same bits on their own (small-batch kernels on the caller's stream)
    s0 = int(np.searchsorted(cu, main_t, side="right")) - 1
    sub_cu = (cu[s0:] - cu[s0]).astype(np.int32)
    np.testing.assert_array_equal(run(enc, ids[cu[s0]:], sub_cu), a[s0:])
    enc.close()


@pytest.mark.parametrize("shape", ["short_batch", "long_batch", "single"])
def test_stream_workspace_contents_never_leak_into_results(minilm_weights, shape):
    """The caller-owned workspace may hold anything (here: NaN bit patterns everywhere) — every byte a kernel reads
    must have been written by the same icrec_encode call.  Poisoned and zeroed workspaces give identical bits."""
    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    enc = DeviceEncoder(minilm_weights, gemm_mode="f16x3")
    if shape == "short_batch":      # catalog-like: 700 short sequences, batch kernels, short attention bucket only
        ids, cu = syn.synthetic_token_batch(700, seed=3, mean_len=25, std_len=6, lo=8, hi=40)
    elif shape == "long_batch":     # mixed lengths incl. the long bucket and a remainder through the small kernels
        ids, cu = syn.synthetic_token_batch(130, seed=4, mean_len=128, std_len=60, lo=1, hi=256)
    else:
        ids, cu = syn.synthetic_token_batch(1, seed=5, mean_len=70, std_len=1, lo=69, hi=71)
    poisoned_runs(enc, ids, cu)
    enc.close()
