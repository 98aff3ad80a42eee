"""CLS-pooled encoders on the GPU (icrec_encoder_set_pooling, DeviceEncoder(pooling="cls")): the embeddings against the
fp32 and float64 references of tests/cls_pooling.py, the pruned last layer of f16x3 mode against the full one bit for
bit in every dispatch form, CLS embeddings against the token rows of the same encoder, mean-pooled encoders untouched,
poisoned workspaces, the ABI's refusals, and a BGE-shaped model directory served end to end."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import cls_pooling as cp
from tests import token_states as ts
from tests.encoder_harness import (EMB_TOL, FORMS, long_rounds_plus_remainder, make_encoder, packed, poisoned_runs,
                                   replay_matches_eager, run)
from tests.recommender_harness import synthetic_world

pytestmark = pytest.mark.gpu

MODES = ("f32", "f16x3")


def _with_n_normalize(shape, n):
    from dataclasses import replace

    return replace(shape, n_normalize=n)


# ---------------------------------------------------------------- 1. against the references
@pytest.mark.parametrize("batch", list(cp.BATCHES))
@pytest.mark.parametrize("kind", ts.KINDS)
@pytest.mark.parametrize("hidden,layers", cp.SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_cls_embeddings_against_the_references(monkeypatch, mode, hidden, layers, kind, batch):
    """E_gpu <= margin x E_ref (tests/token_states.py), per-row rms and max abs, for n_normalize 1 and 2; f32 mode also
    within EMB_TOL of the fp32 oracle's CLS embedding.  Prints the ratios before it asserts
    (profiles/cls_pooling_errors.md holds the measured ones)."""
    r = cp.reference(kind, hidden, layers, batch)
    for n in cp.N_NORMALIZE:
        enc = make_encoder(monkeypatch, r["w"], _with_n_normalize(r["s"], n), mode, max_seq_length=r["max_len"], pooling="cls")
        assert enc.pooling == "cls"
        emb = run(enc, r["ids"], r["cu"])
        enc.close()
        assert emb.shape == r["cls64"][n].shape and emb.dtype == np.float32 and np.isfinite(emb).all()
        ts.check(f"cls embeddings mode={mode} hidden={hidden} layers={layers} weights={kind} batch={batch} n_normalize={n}",
                 emb, r["cls64"][n], r["cls32"][n], ts.MARGINS[(mode, hidden, kind)])
        if mode == "f32":
            assert np.abs(emb - r["cls32"][n]).max() < EMB_TOL


# ---------------------------------------------------------------- 2. same bits in every form
def _three_forms(monkeypatch, w, shape, ids, cu, max_seq_length=None, **env):
    """The CLS embeddings of one batch from the pruned last layer, from the full one (ICREC_CLS_PRUNE=0) and from the
    call that also returns every token (full last layer, by contract): asserted bitwise equal; returns them and the
    pruned encoder (caller closes it)."""
    pruned = make_encoder(monkeypatch, w, shape, max_seq_length=max_seq_length, pooling="cls", **env)
    full = make_encoder(monkeypatch, w, shape, max_seq_length=max_seq_length, pooling="cls", ICREC_CLS_PRUNE=0, **env)
    a = run(pruned, ids, cu)
    b = run(full, ids, cu)
    c, tok = run(pruned, ids, cu, return_tokens=True)
    d, tok_full = run(full, ids, cu, return_tokens=True)
    full.close()
    assert np.isfinite(a).all()
    np.testing.assert_array_equal(a, b, err_msg=f"pruned vs ICREC_CLS_PRUNE=0 {env}")
    np.testing.assert_array_equal(a, c, err_msg=f"pruned vs return_tokens {env}")
    np.testing.assert_array_equal(a, d, err_msg=f"pruned vs ICREC_CLS_PRUNE=0 return_tokens {env}")
    np.testing.assert_array_equal(tok, tok_full)
    return a, pruned


@pytest.mark.parametrize("hidden", [384, 768])
def test_pruned_full_and_token_forms_agree_bitwise_large_batch(monkeypatch, hidden):
    """Whole rounds of 64 tokens per CU plus a remainder (the side stream's range), sequences of up to 512 tokens, 2
    layers: the three forms under the default dispatch, ICREC_FUSE=0, ICREC_SIDE_STREAM=0, and ICREC_SMALL_M values that
    put the n_seqs compact rows in the latency form (default: n_seqs < 3,584) and in the batch form (64 < n_seqs) - all
    the same bits; every sequence of more than 256 tokens encoded alone equals its batch row."""
    s = ts.shape(hidden, 2)
    w = ts.weights("sharp", s)
    ids, cu, split = long_rounds_plus_remainder(monkeypatch, w, s, ts.VOCAB)
    lens = np.diff(cu)
    got = {}
    for form, env in FORMS + [("compact_batch_form", {"ICREC_SMALL_M": 64}),
                              ("compact_batch_form_unfused", {"ICREC_SMALL_M": 64, "ICREC_FUSE": 0})]:
        got[form], enc = _three_forms(monkeypatch, w, s, ids, cu, max_seq_length=512, **env)
        if form == "default":
            assert enc.batch_split(int(cu[-1])) == split
            for i in np.flatnonzero(lens > 256):
                alone = run(enc, ids[cu[i]:cu[i + 1]].copy(), np.array([0, lens[i]], np.int32))
                np.testing.assert_array_equal(alone[0], got[form][i], err_msg=f"sequence {i} ({lens[i]} tokens) alone")
        enc.close()
    for form, emb in got.items():
        np.testing.assert_array_equal(emb, got["default"], err_msg=form)


@pytest.mark.parametrize("lens", [[5, 33, 128, 256, 1, 2, 64, 97], [300, 512, 257, 1, 40, 129, 200, 31], [70], [1], [512]],
                         ids=["8_seqs", "8_seqs_long", "single_70", "single_1", "single_512"])
@pytest.mark.parametrize("hidden,layers", cp.SHAPES)
def test_pruned_full_and_token_forms_agree_bitwise_small(monkeypatch, hidden, layers, lens):
    """A batch of 8 sequences and single sequences (one token: n_seqs == total_tokens, the plain path): the three
    forms under the default (latency form, LayerNorms folded at hidden 384), ICREC_FUSE=0, ICREC_SIDE_STREAM=0 and
    ICREC_SMALL_M=4 (everything, the 8 compact rows included, in the batch form) - the same bits; each sequence
    encoded alone equals its batch row."""
    s = ts.shape(hidden, layers)
    w = ts.weights("sharp", s)
    ids, cu = packed(lens, 6, ts.VOCAB)
    got = {}
    for form, env in FORMS + [("batch_form", {"ICREC_SMALL_M": 4}), ("batch_form_unfused", {"ICREC_SMALL_M": 4, "ICREC_FUSE": 0})]:
        got[form], enc = _three_forms(monkeypatch, w, s, ids, cu, max_seq_length=512, **env)
        if form == "default" and len(lens) > 1:
            for i, n in enumerate(lens):
                alone = run(enc, ids[cu[i]:cu[i + 1]].copy(), np.array([0, n], np.int32))
                np.testing.assert_array_equal(alone[0], got[form][i], err_msg=f"sequence {i} ({n} tokens) alone")
        enc.close()
    for form, emb in got.items():
        np.testing.assert_array_equal(emb, got["default"], err_msg=form)


# ---------------------------------------------------------------- 3. CLS is the token row
@pytest.mark.parametrize("n_norm", [0, 1, 2])
@pytest.mark.parametrize("hidden,layers", [(384, 6), (768, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_cls_embedding_is_the_normalised_first_token_row(monkeypatch, mode, hidden, layers, n_norm):
    """oracle.normalize_rows applied n_normalize times to rows cu[:-1] of the token states IS the embedding, bit for bit:
    the kernel normalises in the oracle's order with correctly rounded divide and sqrt.  Both with the tokens of the same
    call and (f16x3: the pruned layer) of a call that returned none.  One-token sequences: the CLS encoder and the mean
    encoder agree bitwise."""
    from oracle import oracle

    r = cp.reference("sharp", hidden, layers, "to256")
    s = _with_n_normalize(r["s"], n_norm)
    enc = make_encoder(monkeypatch, r["w"], s, mode, pooling="cls")
    emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
    plain = run(enc, r["ids"], r["cu"])
    want = np.ascontiguousarray(tok[r["cu"][:-1]])
    for _ in range(n_norm):
        want = oracle.normalize_rows(want)
    np.testing.assert_array_equal(emb, want)
    np.testing.assert_array_equal(plain, want)
    mean = make_encoder(monkeypatch, r["w"], s, mode, pooling="mean")
    assert mean.pooling == "mean"
    mean_emb, mean_tok = run(mean, r["ids"], r["cu"], return_tokens=True)
    np.testing.assert_array_equal(mean_tok, tok)  # the token states do not depend on the pooling mode
    one = np.flatnonzero(np.diff(r["cu"]) == 1)
    assert one.size >= 1
    np.testing.assert_array_equal(mean_emb[one], emb[one])
    many = np.flatnonzero(np.diff(r["cu"]) >= 2)
    assert (np.abs(mean_emb[many] - emb[many]).max(axis=1) > 1e-3).all()
    # a batch of one-token sequences only (n_seqs == total_tokens: nothing to prune)
    ids1, cu1 = packed([1] * 5, 9, ts.VOCAB)
    np.testing.assert_array_equal(run(enc, ids1, cu1), run(mean, ids1, cu1))
    enc.close(); mean.close()


# ---------------------------------------------------------------- 4. nothing moved for mean pooling
@pytest.mark.parametrize("mode", MODES)
def test_mean_encoder_is_untouched(monkeypatch, mode):
    """A mean-pooled encoder's workspace size is the sum of icrec_encode's six regions, as it always was - computed here
    from the shape, and equal for an encoder that never calls the setter, one that sets MEAN explicitly and one set back
    from CLS; set_pooling(MEAN) changes no bit of the output.  A CLS f16x3 encoder may ask for more (its compact rows),
    an f32 one asks for the same."""
    from instacart_next_order_recommendation_amd import _native

    L = _native.lib()
    r = cp.reference("sharp", 384, 6, "to256")
    s, n, T = r["s"], r["cu"].size - 1, int(r["cu"][-1])
    al = lambda b: (b + 255) & ~255  # noqa: E731
    regions = al(T * s.hidden * 4) * 4 + al(T * 3 * s.hidden * 4) + al(T * s.intermediate * 4)
    never = make_encoder(monkeypatch, r["w"], s, mode)  # (encoder_harness: DeviceEncoder without a pooling argument)
    assert L.icrec_encoder_pooling(never._h) == _native.POOL_MEAN
    assert L.icrec_encode_workspace_bytes(never._h, T, n) == regions
    before = run(never, r["ids"], r["cu"])
    explicit = make_encoder(monkeypatch, r["w"], s, mode)
    _native.check(L.icrec_encoder_set_pooling(explicit._h, _native.POOL_MEAN), "icrec_encoder_set_pooling")
    assert L.icrec_encode_workspace_bytes(explicit._h, T, n) == regions
    np.testing.assert_array_equal(run(explicit, r["ids"], r["cu"]), before)
    np.testing.assert_array_equal(run(never, r["ids"], r["cu"]), before)
    _native.check(L.icrec_encoder_set_pooling(explicit._h, _native.POOL_CLS), "icrec_encoder_set_pooling")
    assert L.icrec_encoder_pooling(explicit._h) == _native.POOL_CLS
    cls_bytes = L.icrec_encode_workspace_bytes(explicit._h, T, n)
    assert cls_bytes >= regions if mode == "f16x3" else cls_bytes == regions
    _native.check(L.icrec_encoder_set_pooling(explicit._h, _native.POOL_MEAN), "icrec_encoder_set_pooling")
    assert L.icrec_encode_workspace_bytes(explicit._h, T, n) == regions
    never.close(); explicit.close()


def test_encode_workspace_bound_is_exact(monkeypatch):
    """icrec_encode_ex on a 2-layer hidden-384 f16x3 encoder, sequences of 5, 33 and 64 tokens, for a mean-pooled, a
    CLS-pooled and a CLS-pooled ICREC_CLS_PRUNE=0 handle: exactly icrec_encode_workspace_bytes bytes are enough and give
    the bits of a larger workspace, one byte less is ICREC_ENOMEM.  The pruned handle asks for more than the mean-pooled
    one (its compact rows), the unpruned one for the same."""
    import torch

    from instacart_next_order_recommendation_amd import _native

    L = _native.lib()
    s = ts.shape(384, 2)
    w = ts.weights("sharp", s)
    ids, cu = packed([5, 33, 64], 3, ts.VOCAB)
    n, T = cu.size - 1, int(cu[-1])
    d_ids, d_cu = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    need = {}
    for name, kw in (("mean", {}), ("cls", {"pooling": "cls"}), ("cls_full", {"pooling": "cls", "ICREC_CLS_PRUNE": 0})):
        enc = make_encoder(monkeypatch, w, s, **kw)
        need[name] = int(L.icrec_encode_workspace_bytes(enc._h, T, n))
        assert need[name] > 0

        def encode(ws, nbytes):
            out = torch.zeros((n, s.hidden), dtype=torch.float32, device="cuda")
            rc = L.icrec_encode_ex(enc._h, _native.ptr(d_ids), _native.ptr(d_cu), n, T, 64, _native.ptr(out), None,
                                   _native.ptr(ws), nbytes, _native.stream_ptr(enc.device))
            torch.cuda.synchronize()
            return rc, out.cpu().numpy()

        roomy = torch.zeros(2 * need[name] + 4096, dtype=torch.uint8, device="cuda")
        rc, want = encode(roomy, roomy.numel())
        assert rc == 0 and np.isfinite(want).all() and np.abs(want).max() > 0
        exact = torch.zeros(need[name], dtype=torch.uint8, device="cuda")
        rc, got = encode(exact, need[name])
        assert rc == 0, L.icrec_last_error()
        np.testing.assert_array_equal(got, want, err_msg=name)
        rc, untouched = encode(exact, need[name] - 1)
        assert rc == -3 and b"workspace" in L.icrec_last_error()  # ICREC_ENOMEM
        assert not untouched.any()  # a refused call launches nothing
        enc.close()
    assert need["cls"] > need["mean"] == need["cls_full"]


# ---------------------------------------------------------------- 5. poisoned workspace
@pytest.mark.parametrize("shape", ["short_batch", "long_batch", "eight", "single"])
@pytest.mark.parametrize("hidden", [384, 768])
def test_poisoned_workspace_never_reaches_the_cls_embeddings(monkeypatch, hidden, shape):
    """Every workspace byte - the compact rows' regions and the context rows no CLS query wrote included - holds a NaN
    pattern before a pruned call: no NaN reaches `out`, and the bits are those of a zeroed workspace."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    s = ts.shape(hidden, 2)
    enc = make_encoder(monkeypatch, ts.weights("sharp", s), s, pooling="cls")
    kw = dict(vocab_size=ts.VOCAB)
    if shape == "short_batch":
        ids, cu = syn.synthetic_token_batch(700, seed=3, mean_len=25, std_len=6, lo=8, hi=40, **kw)
    elif shape == "long_batch":
        ids, cu = syn.synthetic_token_batch(130, seed=4, mean_len=128, std_len=60, lo=1, hi=256, **kw)
    elif shape == "eight":
        ids, cu = packed([5, 33, 128, 256, 1, 2, 64, 97], 2, ts.VOCAB)
    else:
        ids, cu = packed([70], 5, ts.VOCAB)
    poisoned_runs(enc, ids, cu)
    enc.close()


def test_pruned_call_under_graph_capture(monkeypatch):
    """The pruned call is capturable: a replayed graph over a poisoned workspace of its own writes the eager bits."""
    r = cp.reference("sharp", 384, 6, "to256")
    enc = make_encoder(monkeypatch, r["w"], r["s"], pooling="cls")
    replay_matches_eager(enc, r["ids"], r["cu"])
    enc.close()


# ---------------------------------------------------------------- 6. ABI refusals
def test_set_pooling_refusals(monkeypatch):
    from instacart_next_order_recommendation_amd import _native
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    L = _native.lib()
    assert L.icrec_encoder_pooling(None) == -1
    assert L.icrec_encoder_set_pooling(None, _native.POOL_CLS) == -1  # ICREC_EINVAL
    assert b"icrec_encoder_set_pooling" in L.icrec_last_error() and b"NULL" in L.icrec_last_error()
    s = ts.shape(384, 1)
    w = ts.weights("standard", s)
    enc = make_encoder(monkeypatch, w, s)
    for bad in (2, -1, 7):
        assert L.icrec_encoder_set_pooling(enc._h, bad) == -1
        assert b"mode" in L.icrec_last_error() and str(bad).encode() in L.icrec_last_error()
        assert L.icrec_encoder_pooling(enc._h) == _native.POOL_MEAN  # a refused call changes nothing
    assert L.icrec_encoder_set_pooling(enc._h, _native.POOL_CLS) == 0
    assert L.icrec_encoder_pooling(enc._h) == _native.POOL_CLS
    enc.close()
    with pytest.raises(ValueError):
        DeviceEncoder(w, s, pooling="max")
    assert C.sizeof(_native.BertCfg) == 40  # the mode lives on the handle, not in icrec_bert_cfg


# ---------------------------------------------------------------- 7. through Recommender
def test_bge_shaped_model_dir_through_recommender(tmp_path):
    """A synthetic model directory of bge-small-en-v1.5's shape (hidden 384, 12 layers, 12 heads of 32, intermediate
    1,536) with Pooling(cls): recommend() on the graph path, recommend_batch() and MonitoredRecommender.recommend()
    return the oracle's top-k over the oracle's CLS embeddings of the catalog."""
    from oracle import oracle

    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.encoder import pack_token_ids
    from instacart_next_order_recommendation_amd.model_io import load_model_dir
    from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender, Recommender

    shape = syn.BertShape(vocab_size=len(syn.synthetic_vocab()), layers=12)
    model_dir, corpus_path, _ = synthetic_world(tmp_path, 300, model_seed=8, shape=shape, pooling="cls")
    queries = syn.synthetic_user_contexts(5, seed=9) + ["[+1d w0h1] Milk."]
    excl = [set(), {"1", "2"}, None, {"no-such-id"}, set(str(i) for i in range(1, 40)), set()]

    rec = Recommender(model_dir, corpus_path)
    assert rec.model.pooling == "cls" and rec.model.encoder.pooling == "cls" and rec._fast is not None
    assert rec.model.shape.layers == 12 and rec.model.shape.n_normalize == 2
    loaded = load_model_dir(rec.model_dir)
    w, cfg = loaded.weights, oracle.cfg_for(loaded.shape)

    def oracle_cls(texts):
        ids, cu, _ = pack_token_ids(rec.model.tokenizer(texts))
        _, hid = oracle.encode(w, cfg, ids, cu, return_hidden=True)
        emb = np.ascontiguousarray(hid[cu[:-1]])
        for _ in range(loaded.shape.n_normalize):
            emb = oracle.normalize_rows(emb)
        return emb

    P, q_emb = oracle_cls(rec.product_texts), oracle_cls(queries)
    assert np.abs(rec.product_embeddings - P).max() < EMB_TOL
    assert np.abs(rec.model.encode(queries) - q_emb).max() < EMB_TOL
    # normalize_embeddings=False: the second encoder (one normalisation fewer) is CLS-pooled too
    unnorm = rec.model.encode(queries, normalize_embeddings=False)
    assert rec.model._encoder_no_flag.pooling == "cls" and np.abs(unnorm - q_emb).max() < EMB_TOL
    row = {p: i for i, p in enumerate(rec.product_ids)}
    idx, sc = oracle.search(q_emb, P, 10, [[row[p] for p in (e or set()) if p in row] for e in excl])
    want = [[(rec.product_ids[j], float(v)) for j, v in zip(idx[i], sc[i]) if j >= 0] for i in range(len(queries))]

    graph = [rec.recommend(q, 10, excl[i]) for i, q in enumerate(queries)]
    assert rec._fast._graphs  # the single-request graphs were captured with the CLS encoder
    batch = rec.recommend_batch(queries, 10, excl)
    mon = MonitoredRecommender(model_dir, corpus_path)
    monitored = [mon.recommend(q, top_k=10, user_id="u", exclude_product_ids=excl[i]) for i, q in enumerate(queries)]
    assert graph == batch == monitored
    for i in range(len(queries)):
        assert len(graph[i]) == len(want[i]) == 10
        for (gp, gs), (wp, ws) in zip(graph[i], want[i]):
            assert abs(gs - ws) < 1e-4
            if gp != wp:  # embeddings within EMB_TOL of the oracle's: ids agree except across near-ties
                j = [p for p, _ in want[i]].index(gp) if gp in [p for p, _ in want[i]] else None
                assert j is not None and abs(want[i][j][1] - ws) < 2e-5, (i, gp, wp)
