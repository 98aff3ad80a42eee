"""The relative-position attention bias on the GPU (icrec_encoder_set_attention_bias, DeviceEncoder(attention_bias=)):
token states and embeddings against the float64 / float32 reference (oracle/float64_reference.py), the same bits in every
dispatch form, CLS pooling with a bias, the setter's semantics, poisoned workspaces, graph capture, and a synthetic MPNet
model directory served end to end."""
from __future__ import annotations

import numpy as np
import pytest

from tests import relative_bias as tb
from tests import token_states as ts
from tests.encoder_harness import FORMS, long_rounds_plus_remainder, make_encoder, packed, poisoned_runs, replay_matches_eager, run
from tests.recommender_harness import synthetic_world

pytestmark = pytest.mark.gpu

MODES = ("f32", "f16x3")


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("batch", list(tb.BATCHES))
@pytest.mark.parametrize("table_name", tb.TABLES + ("none",))
@pytest.mark.parametrize("kind", ts.KINDS)
@pytest.mark.parametrize("hidden,layers", tb.SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_token_states_and_embeddings_against_the_reference(monkeypatch, mode, hidden, layers, kind, table_name, batch):
    """E_gpu <= margin x E_ref for every token's state and for the embeddings, E_ref being the float32 helper's error on
    the same inputs; "none" runs a bias-free encoder through the same helper under token_states.MARGINS (the helper's own
    check, token states only).  Prints the ratios before it asserts (profiles/attention_bias_errors.md holds the measured
    ones)."""
    r = tb.reference(kind, hidden, layers, batch, table_name)
    enc = make_encoder(monkeypatch, r["w"], r["s"], mode, max_seq_length=r["max_len"], attention_bias=r["table"])
    emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
    plain = run(enc, r["ids"], r["cu"])
    enc.close()
    assert tok.shape == r["h64"].shape and np.isfinite(tok).all() and np.isfinite(emb).all()
    np.testing.assert_array_equal(plain, emb)  # icrec_encode and icrec_encode_ex: the same launches
    case = f"mode={mode} hidden={hidden} layers={layers} weights={kind} table={table_name} batch={batch}"
    ts.check(f"tokens {case}", tok, r["h64"], r["h32"], tb.margins(r, mode), r["cu"])
    if r["table"] is not None:
        ts.check(f"embeddings {case}", emb, r["e64"], r["e32"], tb.margins(r, mode, "embeddings"))


# ---------------------------------------------------------------- 2. same bits in every form
def _same_bits_in_every_form(monkeypatch, w, s, table, ids, cu, alone):
    got = {}
    for form, env in FORMS + [("batch_form", {"ICREC_SMALL_M": 4})]:
        enc = make_encoder(monkeypatch, w, s, max_seq_length=512, attention_bias=table, **env)
        emb, tok = run(enc, ids, cu, return_tokens=True)
        got[form] = (run(enc, ids, cu), tok)
        np.testing.assert_array_equal(emb, got[form][0], err_msg=form)
        if form == "default":
            lens = np.diff(cu)
            for i in alone:
                one, one_tok = run(enc, ids[cu[i]:cu[i + 1]].copy(), np.array([0, lens[i]], np.int32), return_tokens=True)
                np.testing.assert_array_equal(one[0], got[form][0][i], err_msg=f"sequence {i} ({lens[i]} tokens) alone")
                np.testing.assert_array_equal(one_tok, got[form][1][cu[i]:cu[i + 1]], err_msg=f"sequence {i} alone, tokens")
        enc.close()
    assert np.isfinite(got["default"][0]).all()
    for form, (emb, tok) in got.items():  # the reference for "same bits" is the default form
        np.testing.assert_array_equal(emb, got["default"][0], err_msg=form)
        np.testing.assert_array_equal(tok, got["default"][1], err_msg=form)


@pytest.mark.parametrize("table_name", tb.TABLES)
@pytest.mark.parametrize("hidden,layers", tb.SHAPES)
def test_same_bits_in_every_form_small_batch(monkeypatch, hidden, layers, table_name):
    """Sixteen sequences on every key-tile edge up to 512 tokens, f16x3: the default dispatch, ICREC_FUSE=0,
    ICREC_SIDE_STREAM=0 and ICREC_SMALL_M=4 write the same bits, and every sequence alone equals its batch row."""
    s = ts.shape(hidden, layers)
    lens = tb.BATCHES["to512"][0] + tb.BATCHES["to256"][0]
    ids, cu = packed(lens, 23, ts.VOCAB)
    _same_bits_in_every_form(monkeypatch, ts.weights("sharp", s), s, tb.table(table_name, s.heads), ids, cu,
                             alone=range(len(lens)))


@pytest.mark.parametrize("hidden", [384, 768])
def test_same_bits_in_every_form_rounds_plus_remainder(monkeypatch, hidden):
    """Whole rounds of 64 tokens per CU plus a remainder (the side stream's range) with sequences of up to 512 tokens, 2
    layers, dense table: the four forms write the same bits; every sequence longer than 256 alone equals its batch row."""
    s = ts.shape(hidden, 2)
    w = ts.weights("sharp", s)
    table = tb.table("dense", s.heads)
    ids, cu, _ = long_rounds_plus_remainder(monkeypatch, w, s, ts.VOCAB, attention_bias=table)
    long = np.flatnonzero(np.diff(cu) > 256)
    _same_bits_in_every_form(monkeypatch, w, s, table, ids, cu, alone=long)


# ---------------------------------------------------------------- 3. CLS pooling with a bias
@pytest.mark.parametrize("batch", list(tb.BATCHES))
@pytest.mark.parametrize("hidden,layers", tb.SHAPES)
def test_cls_pooling_with_a_bias(monkeypatch, hidden, layers, batch):
    """The pruned last layer (query block 0 only), ICREC_CLS_PRUNE=0 and the token-returning call give the same bits, the
    CLS embedding is the first token's row, and it meets the bound against the reference's first-token rows."""
    from oracle import oracle

    r = tb.reference("sharp", hidden, layers, batch, "dense")
    kw = dict(max_seq_length=r["max_len"], pooling="cls", attention_bias=r["table"])
    pruned = make_encoder(monkeypatch, r["w"], r["s"], **kw)
    full = make_encoder(monkeypatch, r["w"], r["s"], ICREC_CLS_PRUNE=0, **kw)
    a = run(pruned, r["ids"], r["cu"])
    b = run(full, r["ids"], r["cu"])
    c, tok = run(pruned, r["ids"], r["cu"], return_tokens=True)
    pruned.close(); full.close()
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
    rows = np.ascontiguousarray(tok[r["cu"][:-1]])
    for _ in range(r["s"].n_normalize):
        rows = oracle.normalize_rows(rows)
    np.testing.assert_array_equal(a, rows)
    n = r["s"].n_normalize
    ts.check(f"cls embeddings hidden={hidden} layers={layers} batch={batch}", a, r["cls64"][n], r["cls32"][n],
             tb.margins(r, "f16x3", "embeddings"))


# ---------------------------------------------------------------- 4. setter semantics
@pytest.mark.parametrize("mode", MODES)
def test_setter_semantics(monkeypatch, mode):
    """Set then cleared = never set, bit for bit; the workspace size does not know the bias; wrong heads, a NaN and an Inf
    are refused with ICREC_EINVAL and change neither has_attention_bias nor the output."""
    import ctypes as C

    from instacart_next_order_recommendation_amd import _native

    L = _native.lib()
    r = tb.reference("sharp", 384, 1, "to256", "dense")
    s, n, T = r["s"], r["cu"].size - 1, int(r["cu"][-1])
    never = make_encoder(monkeypatch, r["w"], s, mode)
    enc = make_encoder(monkeypatch, r["w"], s, mode)
    ws_bytes = L.icrec_encode_workspace_bytes(never._h, T, n)
    before = run(never, r["ids"], r["cu"])
    enc.set_attention_bias(r["table"])
    assert enc.has_attention_bias and L.icrec_encode_workspace_bytes(enc._h, T, n) == ws_bytes
    biased = run(enc, r["ids"], r["cu"])
    assert np.abs(biased - before).max() > 1e-3

    def refused(t, heads, word):
        t = np.ascontiguousarray(t, np.float32)
        assert L.icrec_encoder_set_attention_bias(enc._h, t.ctypes.data_as(C.c_void_p), heads) == -1  # ICREC_EINVAL
        assert b"icrec_encoder_set_attention_bias" in L.icrec_last_error() and word in L.icrec_last_error()
        assert L.icrec_encoder_has_attention_bias(enc._h) == 1
        np.testing.assert_array_equal(run(enc, r["ids"], r["cu"]), biased)

    refused(r["table"], 11, b"heads")
    refused(np.zeros((16, tb.N_OFFSETS), np.float32), 16, b"heads")
    for bad in (np.nan, np.inf, -np.inf):
        t = r["table"].copy()
        t[7, 900] = bad
        refused(t, 12, b"finite")
    with pytest.raises(ValueError):
        enc.set_attention_bias(np.zeros((12, 1024), np.float32))
    enc.set_attention_bias(None)
    assert not enc.has_attention_bias and L.icrec_encode_workspace_bytes(enc._h, T, n) == ws_bytes
    np.testing.assert_array_equal(run(enc, r["ids"], r["cu"]), before)
    # a refused table on an encoder without one leaves it without one
    assert L.icrec_encoder_set_attention_bias(enc._h, r["table"].ctypes.data_as(C.c_void_p), 3) == -1
    assert L.icrec_encoder_has_attention_bias(enc._h) == 0
    np.testing.assert_array_equal(run(enc, r["ids"], r["cu"]), before)
    assert C.sizeof(_native.BertCfg) == 40  # the table lives on the handle, not in icrec_bert_cfg
    never.close(); enc.close()


# ---------------------------------------------------------------- 5. poisoned workspace
@pytest.mark.parametrize("batch", list(tb.BATCHES))
@pytest.mark.parametrize("hidden", [384, 768])
def test_poisoned_workspace_never_reaches_the_embeddings(monkeypatch, hidden, batch):
    r = tb.reference("sharp", hidden, 1 if hidden == 384 else 2, batch, "dense")
    enc = make_encoder(monkeypatch, r["w"], r["s"], max_seq_length=r["max_len"], attention_bias=r["table"])
    poisoned_runs(enc, r["ids"], r["cu"])
    enc.close()


# ---------------------------------------------------------------- 6. graph capture
def test_biased_encode_under_graph_capture(monkeypatch):
    """A captured biased encode, replayed once over a poisoned workspace of its own, writes the eager bits."""
    r = tb.reference("sharp", 384, 6, "to256", "dense")
    enc = make_encoder(monkeypatch, r["w"], r["s"], attention_bias=r["table"])
    replay_matches_eager(enc, r["ids"], r["cu"])
    enc.close()


# ---------------------------------------------------------------- 7. end to end
E2E_SEEDS = dict(model=8, catalog=42, queries=9)  # chosen on the CPU: see e2e_reference
E2E_TOP_K, E2E_MIN_RANKS, NEAR_TIE = 20, 10, 1e-5


def e2e_reference(model_dir, product_texts, queries):
    """The float64 pipeline (tokenise, oracle/float64_reference.py in float64, cosine scores, descending order, lower row
    first on ties) and the float32 reference's embeddings.  Per query: the top-20 rows and how many leading ranks stand
    before the first near-tie (adjacent reference scores within 1e-5)."""
    import torch

    from instacart_next_order_recommendation_amd.encoder import pack_token_ids
    from instacart_next_order_recommendation_amd.model_io import load_model_dir
    from oracle import float64_reference as f64

    m = load_model_dir(model_dir)
    out = {}
    for name, texts in (("P", product_texts), ("Q", queries)):
        ids, cu, _ = pack_token_ids(m.tokenizer(texts))
        out[name + "64"] = f64.encode(m.weights, m.shape, ids, cu, attention_bias=m.attention_bias)[1]
        out[name + "32"] = f64.encode(m.weights, m.shape, ids, cu, dtype=torch.float32, attention_bias=m.attention_bias)[1]
    scores = out["Q64"] @ out["P64"].T
    order = np.argsort(-scores, axis=1, kind="stable")[:, :E2E_TOP_K + 1]
    top = np.take_along_axis(scores, order, axis=1)
    gaps = top[:, :-1] - top[:, 1:]
    out["rows"] = order[:, :E2E_TOP_K]
    out["ranks"] = [int(np.flatnonzero(g < NEAR_TIE)[0]) if (g < NEAR_TIE).any() else E2E_TOP_K for g in gaps]
    return out


def e2e_inputs(tmp_path):
    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.model_io import synthetic_mpnet_vocab

    shape = syn.BertShape(vocab_size=len(synthetic_mpnet_vocab()), layers=2, type_vocab=1, ln_eps=1e-5, **ts.WIDTHS[768])
    model_dir, corpus_path, _ = synthetic_world(tmp_path, 300, model_seed=E2E_SEEDS["model"], shape=shape,
                                                catalog_seed=E2E_SEEDS["catalog"], architecture="mpnet")
    queries = syn.synthetic_user_contexts(5, seed=E2E_SEEDS["queries"]) + ["[+1d w0h1] Milk."]
    return model_dir, corpus_path, queries


def test_mpnet_model_dir_through_recommender(tmp_path):
    """A synthetic MPNet directory (hidden 768, 2 layers) and a 300-product catalog through Recommender and
    MonitoredRecommender: both encoders carry the bias, catalog and query embeddings meet the bound against the float64
    helper, recommend() on the graph path equals recommend_batch() bit for bit, and the top-20 ids are the float64
    pipeline's up to its first near-tie - at least 10 ranks for every query."""
    from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender, Recommender

    model_dir, corpus_path, queries = e2e_inputs(tmp_path)
    rec = Recommender(model_dir, corpus_path)
    assert rec.model.encoder.has_attention_bias and rec._fast is not None
    assert rec.model.shape.ln_eps == 1e-5 and rec.model.shape.max_position == 512 and rec.model.shape.type_vocab == 1
    ref = e2e_reference(rec.model_dir, rec.product_texts, queries)
    assert min(ref["ranks"]) >= E2E_MIN_RANKS, ref["ranks"]
    # the directory's weights are neither of token_states' two sets: the wider of their two margins at this width
    m = tuple(max(ts.EMB_MARGINS[("f16x3", 768, k)][i] for k in ts.KINDS) for i in range(2))
    ts.check("end to end, catalog embeddings", rec.product_embeddings, ref["P64"], ref["P32"], m)
    ts.check("end to end, query embeddings", rec.model.encode(queries), ref["Q64"], ref["Q32"], m)
    unnorm = rec.model.encode(queries, normalize_embeddings=False)
    assert rec.model._encoder_no_flag.has_attention_bias
    ts.check("end to end, normalize_embeddings=False", unnorm, ref["Q64"], ref["Q32"], m)  # (unit rows either way)

    graph = [rec.recommend(q, E2E_TOP_K) for q in queries]
    assert rec._fast._graphs  # the single-request graphs were captured with the biased encoder
    batch = rec.recommend_batch(queries, E2E_TOP_K)
    mon = MonitoredRecommender(model_dir, corpus_path)
    assert mon.model.encoder.has_attention_bias
    monitored = [mon.recommend(q, top_k=E2E_TOP_K, user_id="u") for q in queries]
    assert graph == batch == monitored
    for i in range(len(queries)):
        want = [rec.product_ids[j] for j in ref["rows"][i]]
        got = [p for p, _ in graph[i]]
        assert len(got) == E2E_TOP_K
        assert got[:ref["ranks"][i]] == want[:ref["ranks"][i]], (i, ref["ranks"][i], got, want)
