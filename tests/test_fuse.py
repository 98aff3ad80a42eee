"""Rank fusion without a GPU: the definition's numpy statement (tests/fuse_reference.py) on a hand-worked case and
its stated consequences, rrf_weights, fusion_plan on a Recommender made with __new__, icrec_fuse_select's argument
checks (ICREC_EINVAL before any HIP call) and the new command-line flags."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import cli
from instacart_next_order_recommendation_amd.recommender import PLAIN, RequestPlan, fusion_plan
from instacart_next_order_recommendation_amd.search import rrf_weights
from tests import fuse_reference as ref
from tests.test_request_plan import PER_QUERY, recommender

MAX_K = 128


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the definition
def test_hand_worked_case():
    A, B = np.array([[5, 2, 9]]), np.array([[2, 7, 5]])
    t = rrf_weights(3)
    idx, sc, pos = ref.fuse_select(A, B, t, t, 4, 10)
    # 2: 1/62 + 1/61, 5: 1/61 + 1/63, 7: 1/62, 9: 1/63
    assert idx.tolist() == [[2, 5, 7, 9]]
    want = [np.float32(t[1] + t[0]), np.float32(t[0] + t[2]), t[1], t[2]]
    assert bits(sc[0]).tolist() == bits(want).tolist()
    assert sc[0, 0] > sc[0, 1] > sc[0, 2] > sc[0, 3]
    assert pos.tolist() == [[[1, 0], [0, 2], [-1, 1], [2, -1]]]
    ones = np.ones(3, np.float32)
    idx, sc, pos = ref.fuse_select(A, B, ones, ones, 6, 10)
    assert idx.tolist() == [[2, 5, 7, 9, -1, -1]]  # the tie rule: the lower id first; top_k exceeds the union
    assert sc.tolist() == [[2.0, 2.0, 1.0, 1.0, 0.0, 0.0]]
    assert pos.tolist() == [[[1, 0], [0, 2], [-1, 1], [2, -1], [-1, -1], [-1, -1]]]


def test_live_entry_rules():
    t = rrf_weights(4)
    # out of range, gated off (0 and negative), excluded; a gated-off first occurrence does not hide the second
    idx, sc, pos = ref.fuse_select([[10, -3, 4, 4]], [[7, 7, 1 << 40, 3]], t, t, 4, 10, a_gate=np.array([[1, 1, 0, 5]], np.int32),
                                   b_gate=np.array([[-2, 1, 1, 1]], np.int32), exclude=[[3]])
    assert idx.tolist() == [[7, 4, -1, -1]]
    assert pos[0, :2].tolist() == [[-1, 1], [3, -1]]
    assert bits(sc[0, :2]).tolist() == bits([t[1], t[3]]).tolist()
    # an id above 2^31 - 1 cannot be excluded; weights that are NaN, negative, -0 count as +0, +inf stays
    w = np.array([np.nan, -1.0, -0.0, np.inf], np.float32)
    big = 2**31 + 5
    idx, sc, _ = ref.fuse_select([[1, 2, 3, big]], [[9, 9, 9, 9]], w, np.zeros(4, np.float32), 5, 2**32 - 1, exclude=[[2]])
    assert idx.tolist() == [[big, 1, 3, 9, -1]]
    assert bits(sc[0]).tolist() == bits([np.inf, 0.0, 0.0, 0.0, 0.0]).tolist()  # never -0, never NaN


def random_lists(rng, Q, k, n_ids):
    L = rng.integers(0, n_ids, (Q, k)).astype(np.int64)
    L[rng.random((Q, k)) < 0.15] = -1
    return L


@pytest.mark.parametrize("seed", range(4))
def test_swapping_the_lists_swaps_only_the_position_columns(seed):
    rng = np.random.default_rng(seed)
    Q, ka, kb, n_ids = 9, int(rng.integers(1, 40)), int(rng.integers(1, 40)), 50
    A, B = random_lists(rng, Q, ka, n_ids), random_lists(rng, Q, kb, n_ids)
    ga, gb = rng.integers(-1, 3, (Q, ka)).astype(np.int32), rng.integers(-1, 3, (Q, kb)).astype(np.int32)
    wa, wb = rrf_weights(ka, 3.0, 0.7), rng.standard_normal(kb).astype(np.float32)
    ex = [rng.integers(0, n_ids, 5).tolist() for _ in range(Q)]
    top_k = int(rng.integers(1, ka + kb + 3))
    one = ref.fuse_select(A, B, wa, wb, top_k, n_ids, ga, gb, ex)
    two = ref.fuse_select(B, A, wb, wa, top_k, n_ids, gb, ga, ex)
    np.testing.assert_array_equal(one[0], two[0])
    np.testing.assert_array_equal(bits(one[1]), bits(two[1]))
    np.testing.assert_array_equal(one[2], two[2][:, :, ::-1])
    assert not np.isnan(one[1]).any() and not (bits(one[1]) == 0x80000000).any()


def test_a_dead_b_list_leaves_a_in_its_order():
    rng = np.random.default_rng(7)
    Q, k, n_ids = 6, 30, 40
    A = random_lists(rng, Q, k, n_ids)
    B = np.full((Q, 5), -1, np.int64)
    B[1] = [3, 4, 5, 6, 7]  # dead by its gate
    gb = np.ones((Q, 5), np.int32)
    gb[1] = 0
    t = rrf_weights(k)
    assert (np.diff(t) < 0).all() and (t > 0).all()
    idx, sc, pos = ref.fuse_select(A, B, t, np.ones(5, np.float32), k, n_ids, b_gate=gb)
    for q in range(Q):
        live = list(dict.fromkeys(int(v) for v in A[q] if v >= 0))
        assert idx[q, :len(live)].tolist() == live and (idx[q, len(live):] == -1).all()
        at = [int(np.flatnonzero(A[q] == v)[0]) for v in live]
        assert bits(sc[q, :len(live)]).tolist() == bits(t[at]).tolist()
        assert pos[q, :len(live), 0].tolist() == at and (pos[q, :, 1] == -1).all()


# ---------------------------------------------------------------- rrf_weights
def test_rrf_weights_values_and_errors():
    for depth, c, w in ((1, 60.0, 1.0), (128, 60.0, 1.0), (7, 0.0, 2.5), (5, -0.5, 0.0), (3, 1e30, 1e38)):
        t = rrf_weights(depth, c, w)
        assert t.dtype == np.float32 and t.shape == (depth,)
        want = np.array([np.float32(np.float64(w) / (np.float64(c) + j + 1)) for j in range(depth)], np.float32)
        assert bits(t).tolist() == bits(want).tolist()
    assert rrf_weights(2).tolist() == [np.float32(1 / 61), np.float32(1 / 62)]
    for bad in (0, MAX_K + 1, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="depth"):
            rrf_weights(bad)
    for bad in (-1.0, -2, float("nan"), float("inf"), float("-inf"), "x"):
        with pytest.raises(ValueError, match="c must be finite"):
            rrf_weights(3, bad)
    for bad in (-0.5, float("nan"), "heavy", None):
        with pytest.raises(ValueError, match="weight must be a number >= 0"):
            rrf_weights(3, 60.0, bad)


# ---------------------------------------------------------------- fusion_plan
class Cf:
    """What _plan looks at: that there is one."""


def fusing_recommender(bare: bool = False):
    rec = recommender(bare)
    rec._cf = Cf()
    return rec


def entry_points(rec, kw):
    """The three calls with recommend's options `kw`, the per-query ones (history among them) wrapped for the batch forms."""
    batch = {name: [v] if name in PER_QUERY + ("history",) else v for name, v in kw.items()}
    calls = [lambda: rec.recommend("milk", 10, **kw), lambda: rec.recommend_batch(["milk"], 10, **batch)]
    if "probes" not in kw:  # (recommend_batch_timed has no probes keyword)
        calls.append(lambda: rec.recommend_batch_timed(["milk"], 10, **batch))
    return calls


def test_history_none_is_the_plain_plan():
    rec = fusing_recommender()
    assert rec._plan(2, 10, history=None) is PLAIN
    assert rec._plan(2, 10, history=[None, None]) is PLAIN
    assert rec._plan(2, 10, history=None, cf_weight=3.0, rrf_c=1.0) is PLAIN  # the two are read with a history only
    assert recommender()._plan(1, 10, history=[None]) is PLAIN  # also without cf
    assert fusion_plan(None, 1.0, 60.0, False, 1, 10, None, 6) is None


def test_what_a_fusing_plan_holds():
    rec = fusing_recommender()
    plan = rec._plan(2, 3, history=[["2", "nope", 5], None], cf_weight=0.5, rrf_c=10)
    assert plan == RequestPlan(fuse=([["2", "nope", "5"], []], 0.5, 10.0, 6)) and not plan.plain  # min(128, 12) of 6 products
    assert rec._plan(1, 2, history=[[]], candidates=4) == RequestPlan(width=4, fuse=([[]], 1.0, 60.0, 4))
    assert rec._plan(1, 2, history=[()], candidates=100).fuse[3] == 6  # clipped to the catalog
    assert rec._plan(1, 2, history=[["1"]], diversity=0).fuse is not None  # diversity 0 asks nothing
    assert RequestPlan(None, None, None, False, None, None, None, None) == RequestPlan()  # the positional order stands


COMBINED = [(dict(aisles=["a0"]), "aisles"), (dict(departments=["d0"]), "departments"), (dict(within="store"), "within"),
            (dict(boosts={"1": 1.0}), "boosts"), (dict(only_boosted=True), "boosts"), (dict(diversity=0.5), "diversity"),
            (dict(probes=2), "probes"), (dict(max_per_aisle=1), "max_per_aisle"), (dict(max_per_department=2), "max_per_department")]


@pytest.mark.parametrize("kw,what", COMBINED, ids=[w + str(i) for i, (_, w) in enumerate(COMBINED)])
def test_history_refuses_every_other_feature_before_the_model_is_used(kw, what):
    rec = fusing_recommender()
    text = f"history cannot be combined with {what}: the CF list is the best of the WHOLE catalog"
    for call in entry_points(rec, dict(kw, history=["1"])):
        with pytest.raises(ValueError, match=re.escape(text)):
            call()


BAD = [(dict(history=["1"], cf_weight=-1.0), "cf_weight must be a number >= 0, got -1.0"),
       (dict(history=["1"], cf_weight=float("nan")), "cf_weight must be a number >= 0"),
       (dict(history=["1"], cf_weight="x"), "cf_weight must be a number >= 0, got 'x'"),
       (dict(history=["1"], rrf_c=-1), "rrf_c must be finite and > -1, got -1"),
       (dict(history=["1"], rrf_c=float("inf")), "rrf_c must be finite and > -1"),
       (dict(history=["1"], rrf_c=float("nan")), "rrf_c must be finite and > -1"),
       (dict(history="12"), "history must be an iterable of product ids, not a string or a mapping"),
       (dict(history={"1": 1.0}), "history must be an iterable of product ids, not a string or a mapping"),
       (dict(history=["1"], candidates=5), "candidates must be in [top_k = 10, 128], got 5")]


@pytest.mark.parametrize("kw,text", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_fusion_arguments_raise_before_the_model_is_used(kw, text):
    rec = fusing_recommender()
    for call in entry_points(rec, kw):
        with pytest.raises(ValueError, match=re.escape(text)):
            call()


def test_history_needs_cf_and_one_entry_per_query():
    for call in entry_points(recommender(), dict(history=[])):
        with pytest.raises(ValueError, match="history needs a recommender built with cf"):
            call()
    rec = fusing_recommender()
    with pytest.raises(ValueError, match="history has 1 entries for 2 queries"):
        rec.recommend_batch(["milk", "bread"], 10, history=[["1"]])
    with pytest.raises(ValueError, match="history of a batch is a sequence with one entry per query"):
        rec.recommend_batch(["milk"], 10, history="1")
    for call in entry_points(rec, dict(history=["1", "2"])):  # a good request reaches the model
        with pytest.raises(AssertionError, match="model.tokenizer used"):
            call()


def test_remove_products_is_refused_with_cf_and_the_constructor_checks_the_ids():
    rec = fusing_recommender()
    before = list(rec.product_ids)
    with pytest.raises(ValueError, match="remove_products renumbers catalog rows"):
        rec.remove_products(["1"])
    assert rec.product_ids == before
    cf = Cf()
    cf.corpus_ids = before[:-1]
    with pytest.raises(ValueError, match="cf.corpus_ids must be the catalog's product_ids"):
        rec._set_cf(cf)
    cf.corpus_ids = before[::-1]
    with pytest.raises(ValueError, match="cf.corpus_ids must be the catalog's product_ids"):
        rec._set_cf(cf)
    cf.corpus_ids = list(before)
    rec._set_cf(cf)
    assert rec._cf is cf


# ---------------------------------------------------------------- the C entry point's argument checks
@pytest.fixture(scope="module")
def native():
    from instacart_next_order_recommendation_amd import _native

    if not _native.LIB_PATH.exists():
        _native.build()
    return _native


def test_fuse_select_validates_arguments_without_a_gpu(native):
    lib = native.lib()
    buf = (C.c_int64 * 1024)()  # never read: every call below is refused before any HIP call
    p = C.cast(buf, C.c_void_p)
    good = dict(a_idx=p, a_gate=None, ka=3, a_w=p, b_idx=p, b_gate=None, kb=4, b_w=p, n_queries=1, n_ids=10, excl_idx=None,
                excl_off=None, top_k=2, out_idx=p, out_score=p, out_pos=None, device=0, stream=None)

    def call(**change):
        return lib.icrec_fuse_select(*{**good, **change}.values())

    bad = [dict(a_idx=None), dict(b_idx=None), dict(a_w=None), dict(b_w=None), dict(out_idx=None), dict(out_score=None),
           dict(excl_idx=p), dict(excl_off=p), dict(n_queries=0), dict(n_queries=-1), dict(ka=0), dict(ka=MAX_K + 1), dict(kb=0),
           dict(kb=MAX_K + 1), dict(top_k=0), dict(top_k=MAX_K + 1), dict(n_ids=0), dict(n_ids=-1), dict(n_ids=2**32)]
    for change in bad:
        assert call(**change) == -1, change  # ICREC_EINVAL
        assert b"icrec_fuse_select" in lib.icrec_last_error(), change
    assert b"n_ids" in lib.icrec_last_error()


# ---------------------------------------------------------------- the command lines
def test_recommend_flags_parse_and_refuse():
    args = cli.build_parser().parse_args(["--cf-data-dir", "d", "--cf-processed-dir", "p", "--history", "12", "--history", "7",
                                          "--cf-weight", "0.5", "--rrf-c", "10"])
    assert args.history == ["12", "7"] and args.cf_weight == 0.5 and args.rrf_c == 10.0
    assert str(args.cf_data_dir) == "d" and str(args.cf_processed_dir) == "p" and cli.fusion_args(args) is True
    plain = cli.build_parser().parse_args([])
    assert plain.history is None and plain.cf_weight == 1.0 and plain.rrf_c == 60.0 and cli.fusion_args(plain) is False
    for argv, text in ((["--history", "1"], "--history needs --cf-data-dir and --cf-processed-dir"),
                       (["--cf-data-dir", "d"], "--cf-data-dir and --cf-processed-dir go together"),
                       (["--cf-processed-dir", "p", "--history", "1"], "go together")):
        with pytest.raises(SystemExit, match=text):
            cli.main(argv)
    dirs = ["--cf-data-dir", "d", "--cf-processed-dir", "p", "--history", "1"]
    for extra, flag in ((["--aisle", "x"], "--aisle"), (["--department", "x"], "--department"), (["--diversity", "0.5"], "--diversity"),
                        (["--ann-lists", "4", "--probes", "2"], "--probes"), (["--boost", "3=1"], "--boost"),
                        (["--only-boosted"], "--only-boosted"), (["--product-sets", "f", "--within", "s"], "--within"),
                        (["--max-per-aisle", "1"], "--max-per-aisle"), (["--max-per-department", "1"], "--max-per-department")):
        with pytest.raises(SystemExit, match=f"--history cannot be combined with {flag}"):
            cli.main(dirs + extra)


def test_baselines_hybrid_flag_parses_and_refuses():
    for only in ("--content-only", "--cf-only"):
        with pytest.raises(SystemExit, match="--hybrid fuses the two baselines"):
            cli.baselines_main(["--hybrid", only, "--processed-dir", "/nonexistent"])
    with pytest.raises(SystemExit, match="--cf-weight takes a weight >= 0"):
        cli.baselines_main(["--hybrid", "--cf-weight", "-1", "--processed-dir", "/nonexistent"])
    with pytest.raises(SystemExit, match="--cf-weight takes a weight >= 0"):
        cli.baselines_main(["--hybrid", "--rrf-c", "-1", "--processed-dir", "/nonexistent"])
    with pytest.raises(SystemExit, match="holds no eval_queries.json"):  # the flags are accepted: the next check speaks
        cli.baselines_main(["--hybrid", "--cf-weight", "2", "--rrf-c", "10", "--processed-dir", "/nonexistent"])
