"""Sequences of 257-512 tokens on the GPU: encoders whose ceiling was raised with icrec_encoder_set_max_seqlen, the
9-16-key-tile attention bucket in both arithmetic modes (single sequences, mixed batches, the batch forms and the
two-stream paths), bit-for-bit no change at 256 tokens or fewer, and the recommender end to end on a model served
at max_seq_length 512 (and at 300, its max_position)."""
from __future__ import annotations

import json

import numpy as np
import pytest

from tests.encoder_harness import EMB_TOL, make_encoder, oracle_rows, packed, run
from tests.recommender_harness import synthetic_world, torch_cuda  # noqa: F401  (torch_cuda: fixture)
from tests.test_long_sequences import long_contexts

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32"]


def test_ceiling_bounds(monkeypatch, minilm_weights):
    import torch

    from instacart_next_order_recommendation_amd import _native
    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd._native import IcrecError
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    L = _native.lib()
    shape = syn.BertShape()
    enc = DeviceEncoder(minilm_weights, shape)
    assert enc.max_seq_length == 256
    for bad in (0, -1, 513):
        with pytest.raises(IcrecError):
            _native.check(L.icrec_encoder_set_max_seqlen(enc._h, bad), "icrec_encoder_set_max_seqlen")
    ids, cu = packed([512], 1, 30522)
    ids_d, cu_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    with pytest.raises(IcrecError):  # the default ceiling refuses 512 tokens ...
        enc.encode_packed(ids_d, cu_d, 512)
    with pytest.raises(ValueError):
        enc.encode_ids([ids.tolist()])
    enc.close()
    raised = DeviceEncoder(minilm_weights, shape)  # the setter itself, before the first encode
    _native.check(L.icrec_encoder_set_max_seqlen(raised._h, 512), "icrec_encoder_set_max_seqlen")
    one = raised.encode_packed(ids_d, cu_d, 512).cpu().numpy()  # ... which a 512 ceiling accepts
    raised.close()
    with pytest.raises(IcrecError):
        DeviceEncoder(minilm_weights, shape, max_seq_length=513)
    big = make_encoder(monkeypatch, minilm_weights, shape, max_seq_length=512)
    assert big.max_seq_length == 512
    np.testing.assert_array_equal(big.encode_ids([ids.tolist()]).cpu().numpy(), one)
    assert np.abs(one - oracle_rows(minilm_weights, shape, ids, cu)).max() < EMB_TOL
    big.close()
    # under max_position 300 the ceiling stops at 300
    short = syn.BertShape(vocab_size=2048, max_position=300)
    w = syn.synthetic_bert_weights(short, seed=5)
    with pytest.raises(IcrecError):
        DeviceEncoder(w, short, max_seq_length=301)
    e300 = DeviceEncoder(w, short, max_seq_length=300)
    ids3 = (ids[:300] % 2048).copy()
    got = run(e300, ids3, np.array([0, 300], np.int32))
    assert np.abs(got - oracle_rows(w, short, ids3, np.array([0, 300], np.int32))).max() < EMB_TOL
    e300.close()


@pytest.mark.parametrize("mode", MODES)
def test_single_sequences_vs_oracle(monkeypatch, minilm_weights, mode):
    from instacart_next_order_recommendation_amd import synthetic as syn

    lens = [257, 288, 289, 300, 384, 480, 511, 512]
    ids, cu = packed(lens, 7, 30522)
    shape = syn.BertShape()
    want = oracle_rows(minilm_weights, shape, ids, cu)
    enc = make_encoder(monkeypatch, minilm_weights, shape, mode, max_seq_length=512)
    for s, n in enumerate(lens):
        got = run(enc, ids[cu[s]:cu[s + 1]].copy(), np.array([0, n], np.int32))[0]
        err = float(np.abs(got - want[s]).max())
        print(f"[{mode}] {n} tokens alone: max|emb - oracle| = {err:.3e}")
        assert err < EMB_TOL, (n, err)
    enc.close()


def _mixed(seed):
    """Every tile boundary from 1 to 512 tokens, plus 56 short sequences: 70 sequences, the batch forms (dispatch
    order, attention buckets split over two streams)."""
    rng = np.random.default_rng(seed)
    lens = [512, 511, 481, 480, 300, 289, 288, 257, 256, 200, 129, 65, 33, 1] + rng.integers(3, 25, 56).tolist()
    return packed(lens, seed, 30522)


@pytest.mark.parametrize("mode", MODES)
def test_mixed_batch_vs_oracle(monkeypatch, minilm_weights, mode):
    from instacart_next_order_recommendation_amd import synthetic as syn

    ids, cu = _mixed(seed=11)
    assert cu.size - 1 >= 64 and 3584 < cu[-1] < 8192  # past ICREC_SMALL_M's default: the layer kernel by default
    shape = syn.BertShape()
    want = oracle_rows(minilm_weights, shape, ids, cu)
    forms = [("layer", {})]
    if mode == "f16x3":
        forms += [("latency", {"ICREC_SMALL_M": 8192}), ("layer_unfused", {"ICREC_FUSE": 0}),
                  ("latency_unfused", {"ICREC_SMALL_M": 8192, "ICREC_FUSE": 0}), ("one_stream", {"ICREC_SIDE_STREAM": 0})]
    got = {}
    for form, env in forms:
        enc = make_encoder(monkeypatch, minilm_weights, shape, mode, max_seq_length=512, **env)
        got[form] = run(enc, ids, cu)
        enc.close()
        err = float(np.abs(got[form] - want).max())
        print(f"[{mode}] mixed batch, {form}: max|emb - oracle| = {err:.3e}")
        assert err < EMB_TOL, (form, err)
    for form in got:
        np.testing.assert_array_equal(got[form], got["layer"], err_msg=form)


def _large(seed):
    """300 sequences, ~40k tokens (both halves past DeviceEncoder's two-stream thresholds), with sequences of
    257-512 tokens spread over both halves."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    _, cu = syn.synthetic_token_batch(300, seed=seed, mean_len=110, std_len=60, lo=1, hi=256)
    lens = np.diff(cu)
    long_at = np.arange(3, 300, 12)
    lens[long_at] = np.linspace(257, 512, long_at.size).astype(np.int64)
    return packed(lens.tolist(), seed, 30522)


def test_large_batch_two_stream_paths(monkeypatch, minilm_weights):
    """f16x3: default, ICREC_SMALL_M=512 and ICREC_FUSE=0, each one call and two-stream (DeviceEncoder's halves):
    all bitwise equal; every long sequence encoded alone gives its batch row bit for bit; a sample of rows against
    the oracle.  f32: the sample against the oracle."""
    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    ids, cu = _large(seed=21)
    n, lens = cu.size - 1, np.diff(cu)
    assert n >= 2 * DeviceEncoder.SPLIT_MIN_SEQS and cu[n // 2] >= DeviceEncoder.SPLIT_MIN_TOKENS
    assert cu[-1] - cu[n // 2] >= DeviceEncoder.SPLIT_MIN_TOKENS
    assert (lens[: n // 2] > 256).any() and (lens[n // 2:] > 256).any()
    sample = [int(r) for r in np.flatnonzero(lens > 256)[::5]] + [int(np.argmax(lens)), 0, 1, n - 1]
    shape = syn.BertShape()
    want = oracle_rows(minilm_weights, shape, ids, cu, sample)
    got = {}
    for form, env in [("default", {}), ("layer", {"ICREC_SMALL_M": 512}), ("unfused", {"ICREC_FUSE": 0})]:
        enc = make_encoder(monkeypatch, minilm_weights, shape, max_seq_length=512, **env)
        for two in (False, True):
            got[(form, two)] = run(enc, ids, cu, cu_host=cu if two else None)
        if form == "default":
            for s in np.flatnonzero(lens > 256):
                alone = run(enc, ids[cu[s]:cu[s + 1]].copy(), np.array([0, lens[s]], np.int32))
                np.testing.assert_array_equal(alone[0], got[(form, False)][s], err_msg=f"sequence {s} ({lens[s]} tokens)")
        enc.close()
    ref = got[("default", False)]
    for key, emb in got.items():
        np.testing.assert_array_equal(emb, ref, err_msg=str(key))
    err = float(np.abs(ref[sample] - want).max())
    print(f"[f16x3] large batch: max|emb - oracle| over {len(sample)} rows = {err:.3e}")
    assert err < EMB_TOL
    enc = make_encoder(monkeypatch, minilm_weights, shape, "f32", max_seq_length=512)
    e32 = run(enc, ids, cu, cu_host=cu)
    enc.close()
    err = float(np.abs(e32[sample] - want).max())
    print(f"[f32] large batch: max|emb - oracle| over {len(sample)} rows = {err:.3e}")
    assert err < EMB_TOL


@pytest.mark.parametrize("mode", MODES)
def test_no_change_at_256_tokens_or_fewer(monkeypatch, minilm_weights, mode):
    """A batch of 256 tokens or fewer per sequence encodes to the same bits under a 512 ceiling as under the default."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    rng = np.random.default_rng(5)
    ids, cu = packed([256, 200, 129, 65, 64, 33, 32, 31, 1] + rng.integers(3, 25, 61).tolist(), 5, 30522)
    shape = syn.BertShape()
    default = make_encoder(monkeypatch, minilm_weights, shape, mode)
    raised = make_encoder(monkeypatch, minilm_weights, shape, mode, max_seq_length=512)
    assert default.max_seq_length == 256 and raised.max_seq_length == 512
    np.testing.assert_array_equal(run(raised, ids, cu), run(default, ids, cu))
    one = ids[: cu[1]].copy(), cu[:2].copy()
    np.testing.assert_array_equal(run(raised, *one), run(default, *one))
    default.close(); raised.close()


@pytest.fixture(scope="module", params=[512, 300], ids=["max_seq_length512", "max_position300"])
def long_world(request, tmp_path_factory, torch_cuda):
    from instacart_next_order_recommendation_amd import synthetic as syn

    shape = syn.BertShape(vocab_size=len(syn.synthetic_vocab()), max_position=request.param)
    w = synthetic_world(tmp_path_factory.mktemp(f"rec{request.param}"), 300, model_seed=1, shape=shape)
    sb = w.model_dir / "sentence_bert_config.json"
    sb.write_text(json.dumps({**json.loads(sb.read_text()), "max_seq_length": 512}))
    return {"model_dir": w.model_dir, "corpus_path": w.corpus_path, "limit": request.param,
            "queries": long_contexts(6, seed=request.param)}


def test_recommender_end_to_end_long_contexts(long_world, monkeypatch):
    """Contexts of 300-512 tokens: recommend() on the graph path, recommend() without it and recommend_batch() agree
    (ids exact, scores bitwise); the top-10 against the oracle's encode + search on the same token ids."""
    from oracle import oracle

    from instacart_next_order_recommendation_amd.encoder import pack_token_ids
    from instacart_next_order_recommendation_amd.model_io import load_model_dir
    from instacart_next_order_recommendation_amd.recommender import Recommender

    rec = Recommender(long_world["model_dir"], long_world["corpus_path"])
    limit = long_world["limit"]
    assert rec.model.max_seq_length == limit and rec.model.encoder.max_seq_length == limit
    queries = long_world["queries"]
    toks = rec.model.tokenizer(queries)
    assert min(len(t) for t in toks) >= 300 and max(len(t) for t in toks) == limit
    assert rec._fast is not None and all(rec._fast.supports(len(t), 10, 2) for t in toks)
    excl = [set(), {"1", "2"}, None, set(rec.product_ids[:30]), set(), {"7"}]
    graph = [rec.recommend(q, 10, excl[i]) for i, q in enumerate(queries)]
    assert rec._fast._graphs and max(b for b, _ in rec._fast._graphs) == limit  # the long bucket was captured
    batch = rec.recommend_batch(queries, 10, excl)
    monkeypatch.setenv("ICREC_USE_GRAPH", "0")
    eager_rec = Recommender(long_world["model_dir"], long_world["corpus_path"])
    assert eager_rec._fast is None
    eager = [eager_rec.recommend(q, 10, excl[i]) for i, q in enumerate(queries)]
    assert graph == batch == eager
    # the oracle on the recommender's own token ids; embeddings within 5e-6, so ids agree except across near-ties
    shape = rec.model.shape
    cfg = oracle.cfg_for(shape)
    w = load_model_dir(rec.model_dir).weights
    ids, cu, _ = pack_token_ids(toks, limit)
    q_emb = oracle.encode(w, cfg, ids, cu)
    assert np.abs(rec.model.encoder.encode_ids(toks).cpu().numpy() - q_emb).max() < EMB_TOL
    pids, cu_p, _ = pack_token_ids(rec.model.tokenizer(rec.product_texts))
    P = oracle.encode(w, cfg, pids, cu_p)
    assert np.abs(rec.product_embeddings - P).max() < EMB_TOL
    row = {p: i for i, p in enumerate(rec.product_ids)}
    idx, sc = oracle.search(q_emb, P, 10, [[row[p] for p in (e or set()) if p in row] for e in excl])
    for i in range(len(queries)):
        want = [(rec.product_ids[j], float(s)) for j, s in zip(idx[i], sc[i]) if j >= 0]
        assert len(graph[i]) == len(want) == 10
        for (gp, gs), (wp, ws) in zip(graph[i], want):
            assert abs(gs - ws) < 1e-4
            if gp != wp:
                j = [p for p, _ in want].index(gp) if gp in [p for p, _ in want] else None
                assert j is not None and abs(want[j][1] - ws) < 2e-5, (i, gp, wp)
