"""Composed queries without a GPU: the properties of the reference definition (tests/compose_reference.py), every
ICREC_EINVAL of icrec_compose_queries with a message that names the argument, term_csr's order, and compose_plan /
Recommender._plan on a recommender made with __new__ (test_request_plan's)."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.recommender import PLAIN, RequestPlan, compose_plan, compose_terms
from instacart_next_order_recommendation_amd.search import term_csr
from tests import compose_reference as ref
from tests.test_request_plan import recommender

F32 = np.float32


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(11)
    return rng.standard_normal((40, 64)).astype(F32)


# ---------------------------------------------------------------- the reference's own properties
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_one_term_of_weight_one_without_a_base_is_the_stored_row(rows, storage):
    p_hat = ref.stored_rows(rows, storage)
    for r in (0, 17, 39):
        np.testing.assert_array_equal(ref.compose_one(p_hat, None, None, [r], [1.0], 1), p_hat[r])
        np.testing.assert_array_equal(ref.compose_one(p_hat, None, None, [r], None, 4), p_hat[r])


def test_liked_rows_pull_the_query_toward_their_sum(rows):
    rng = np.random.default_rng(5)
    p_hat = ref.stored_rows(rows)

    def cos(x, y):
        x, y = x.astype(np.float64), y.astype(np.float64)
        return float(x @ y / (np.linalg.norm(x) * np.linalg.norm(y)))

    for _ in range(20):
        base = rng.standard_normal(64).astype(F32)
        n = int(rng.integers(1, 9))
        t_rows = rng.integers(0, 40, n)
        t_w = rng.uniform(0.05, 2.0, n).astype(F32)
        target = (t_w[:, None].astype(np.float64) * p_hat[t_rows].astype(np.float64)).sum(0)
        out = ref.compose_one(p_hat, base, None, t_rows, t_w, n)
        q_hat = ref.compose_one(p_hat, base, None, [], [], 0)
        assert cos(out, target) >= cos(q_hat, target)


def test_an_invalid_term_equals_an_absent_term(rows):
    p_hat = ref.stored_rows(rows)
    base = np.linspace(-1, 1, 64, dtype=F32)
    good = [(3, 0.5), (9, -0.25), (3, 1.5)]
    want = ref.compose_lists(p_hat, base[None], [good])
    bad = [(-1, 1.0), (40, 1.0), (2**31 - 1, 1.0), (5, np.nan), (6, np.inf), (7, -np.inf)]
    for at in range(len(good) + 1):
        for b in bad:
            mixed = good[:at] + [b] + good[at:]
            np.testing.assert_array_equal(ref.compose_lists(p_hat, base[None], [mixed]), want)
    assert not ref.term_valid(40, 1.0, 40) and ref.term_valid(39, -2.0, 40) and ref.term_valid(0, 0.0, 40)
    # the weight of the base that is not finite counts as 0; max_terms cuts the list; a reversed segment is empty
    for a in (np.inf, -np.inf, np.nan):
        np.testing.assert_array_equal(ref.compose_one(p_hat, base, a, [], [], 0), ref.compose_one(p_hat, base, 0.0, [], [], 0))
    np.testing.assert_array_equal(ref.compose_one(p_hat, base, None, [3, 9, 3], [0.5, -0.25, 1.5], 2),
                                  ref.compose_one(p_hat, base, None, [3, 9], [0.5, -0.25], 2))
    out = ref.compose(p_hat, None, None, [2, 0, 2], np.array([1, 2], np.int32), None, 8)
    assert not out[0].any()
    np.testing.assert_array_equal(out[1], (p_hat[1] + p_hat[2]).astype(F32))


def test_term_order_matters_in_bits_and_the_reference_honours_it():
    # 1 + 2^-24 + 2^-24: each small term alone is rounded away (ties to even), the two first are not
    p_hat = np.array([[1.0], [2.0 ** -24]], F32)  # (not unit rows: the property is the accumulation's, not the rows')
    big_first = ref.compose_one(p_hat, None, None, [0, 1, 1], None, 3)
    small_first = ref.compose_one(p_hat, None, None, [1, 1, 0], None, 3)
    assert big_first[0] == F32(1.0) and small_first[0] == F32(1.0) + F32(2.0 ** -23) and big_first[0] != small_first[0]
    # the product is rounded before the sum: 3 * (1 + 2^-23) is not a float32, and a fused multiply-add keeps its tail
    p_hat = np.array([[1.0 + 2.0 ** -23]], F32)
    acc = ref.compose_one(p_hat, None, None, [0, 0], [-3.0, 3.0], 2)
    assert acc[0] == 0.0


# ---------------------------------------------------------------- argument checks of the C entry point
def test_every_einval_names_its_argument():
    lib = _native.lib()
    mem = (C.c_char * 256)()  # stands for every non-NULL pointer: a refused call dereferences none of them
    p = C.cast(mem, C.c_void_p)
    ok = dict(idx=p, base=p, base_w=p, n=2, off=p, rows=p, w=p, max_terms=4, out=p)

    def call(**kw):
        a = {**ok, **kw}
        rc = lib.icrec_compose_queries(a["idx"], a["base"], a["base_w"], a["n"], a["off"], a["rows"], a["w"], a["max_terms"],
                                       a["out"], None)
        return rc, lib.icrec_last_error().decode()

    for kw, text in ((dict(idx=None), "idx"), (dict(off=None), "term_off"), (dict(out=None), "out"),
                     (dict(rows=None), "term_rows"), (dict(n=0), "n_queries"), (dict(n=-3), "n_queries"),
                     (dict(max_terms=-1), "max_terms"), (dict(max_terms=_native.ICREC_MAX_TERMS + 1), "max_terms"),
                     (dict(base=None, base_w=None, max_terms=0, rows=None), "base"),
                     (dict(base=None), "base_w")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("icrec_compose_queries:") and text in msg, (kw, rc, msg)
    assert _native.ICREC_MAX_TERMS == 1024
    header = (_native._PKG.parent / "include" / "icrec.h").read_text()
    assert re.search(r"#define\s+ICREC_MAX_TERMS\s+1024\b", header)


# ---------------------------------------------------------------- term_csr
def test_term_csr_keeps_the_given_order():
    off, rows, w = term_csr([[(9, 0.5), (2, -1.0), (9, 0.25)], None, {7: 1.0, 3: 2.0}, []], 4)
    assert off.tolist() == [0, 3, 3, 5, 5] and off.dtype == np.int32
    assert rows.tolist() == [9, 2, 9, 7, 3] and rows.dtype == np.int32
    assert w.tolist() == [0.5, -1.0, 0.25, 1.0, 2.0] and w.dtype == np.float32
    off, rows, w = term_csr([None, None], 2)
    assert off.tolist() == [0, 0, 0] and rows.size == 1 and w.size == 1  # never a NULL pointer
    term_csr([[(i, 1.0) for i in range(_native.ICREC_MAX_TERMS)]], 1)
    with pytest.raises(ValueError, match="more than ICREC_MAX_TERMS = 1024"):
        term_csr([[(i, 1.0) for i in range(_native.ICREC_MAX_TERMS + 1)]], 1)
    with pytest.raises(ValueError, match="terms has 1 entries for 2 queries"):
        term_csr([None], 2)


# ---------------------------------------------------------------- compose_plan and Recommender._plan
PID_TO_ROW = {str(i + 1): i for i in range(6)}


def test_compose_terms_weights_and_order():
    assert compose_terms(["3", "nope", "1"], ["6"], 1.0, 0.5, PID_TO_ROW) == [(2, 0.5), (0, 0.5), (5, -0.5)]
    assert compose_terms({"2": 0.75, "5": 0.0}, {"1": 2.0}, 9.0, 9.0, PID_TO_ROW) == [(1, 0.75), (4, 0.0), (0, -2.0)]
    assert compose_terms(iter(["4"]), None, 3.0, 0.5, PID_TO_ROW) == [(3, 3.0)]
    assert compose_terms(None, ["1", "2", "3", "4"], 1.0, 1.0, PID_TO_ROW) == [(0, -0.25), (1, -0.25), (2, -0.25), (3, -0.25)]
    for like, unlike in ((None, None), ([], []), (["nope"], {"neither": 1.0}), ({}, None)):
        assert compose_terms(like, unlike, 1.0, 0.5, PID_TO_ROW) is None


BAD = [
    (dict(like="12"), "like must be a mapping product id -> weight or an iterable of product ids, not a string"),
    (dict(unlike="12"), "unlike must be a mapping product id -> weight or an iterable of product ids, not a string"),
    (dict(like={"1": -1.0}), "the like weight of '1' must be a finite number >= 0, got -1.0"),
    (dict(unlike={"1": float("nan")}), "the unlike weight of '1' must be a finite number >= 0, got nan"),
    (dict(like={"1": float("inf")}), "the like weight of '1' must be a finite number >= 0, got inf"),
    (dict(like={"1": "heavy"}), "the like weight of '1' must be a finite number >= 0, got 'heavy'"),
    (dict(like=["1"], like_weight=-2), "like_weight must be a finite number >= 0, got -2"),
    (dict(unlike=["1"], unlike_weight=float("inf")), "unlike_weight must be a finite number >= 0, got inf"),
    (dict(like=["1"], query_weight=float("nan")), "query_weight must be a finite number >= 0, got nan"),
    (dict(like=["1", "2"], unlike=["3", "1"]), "product id '1' is in both like and unlike"),
    (dict(like=["1", "2", "1"]), "product id '1' is named twice in like"),
    (dict(unlike=["nope", "nope"]), "product id 'nope' is named twice in unlike"),
]


@pytest.mark.parametrize("kw,text", BAD, ids=[t[:40] for _, t in BAD])
def test_bad_arguments_raise_their_text_before_the_model_is_used(kw, text):
    rec = recommender()
    batch = {name: [v] if name in ("like", "unlike") else v for name, v in kw.items()}
    calls = [lambda: rec.recommend("milk", 10, **kw), lambda: rec.recommend_batch(["milk"], 10, **batch),
             lambda: rec.recommend_batch_timed(["milk"], 10, **batch)]
    for call in calls:
        with pytest.raises(ValueError, match=re.escape(text)):
            call()


def test_too_many_known_ids_and_the_batch_forms():
    many = {str(i): i for i in range(_native.ICREC_MAX_TERMS + 1)}
    ids = list(many)
    assert len(compose_terms(ids[:-1], None, 1.0, 0.5, many)) == _native.ICREC_MAX_TERMS
    with pytest.raises(ValueError, match="1025 like / unlike products exceed the limit 1024"):
        compose_terms(ids[:600], ids[600:], 1.0, 0.5, many)
    rec = recommender()
    for name in ("like", "unlike"):
        for bad in ("12", {"1": 1.0}, iter([["1"], None])):
            with pytest.raises(ValueError, match=f"{name} of a batch is a sequence with one entry per query"):
                rec.recommend_batch(["milk", "eggs"], 10, **{name: bad})
        with pytest.raises(ValueError, match=f"{name} has 1 entries for 2 queries"):
            rec.recommend_batch_timed(["milk", "eggs"], 10, **{name: [["1"]]})
    with pytest.raises(ValueError, match="in both like and unlike"):
        compose_plan([["2"]], [["2"]], 1.0, 1.0, 0.5, 1, PID_TO_ROW)
    for name in ("like", "unlike", "query_weight", "unlike_weight"):
        with pytest.raises(ValueError, match=f"recommend_from_products takes no {name}"):
            rec.recommend_from_products(["1"], 5, **{name: 1.0})
    with pytest.raises(ValueError, match="not a string"):
        rec.recommend_from_products("12", 5)
    with pytest.raises(ValueError, match="diversity must be"):
        rec.recommend_from_products(["1"], 5, diversity=2)
    assert rec.recommend_from_products(["nope"], 5) == [] and rec.recommend_from_products([], 5, aisles=["a0"]) == []
    with pytest.raises(KeyError):
        rec.similar_products("nope")
    seen = []  # good arguments reach the search without token ids: no text, no encoder
    rec._encode_search = lambda ids, cu, k, ex, plan: seen.append((ids, cu, k, ex, plan)) or (np.array([[4, -1]]), np.ones((1, 2), F32))
    assert rec.similar_products("3", 2, within="stock") == [("5", 1.0)]
    assert seen == [(None, None, 2, [[2]], RequestPlan(sets=[[1]], compose=[(0.0, [(2, 1.0)])]))]


def test_what_compose_plan_returns_and_when_a_plan_stays_plain():
    assert compose_plan(None, None, 1.0, 1.0, 0.5, 2, PID_TO_ROW) is None
    assert compose_plan([None, []], [["nope"], None], 1.0, 1.0, 0.5, 2, PID_TO_ROW) is None
    assert compose_plan([["2", "1"], None], [{"3": 4.0}, ["nope"]], 0.25, 1.0, 0.5, 2, PID_TO_ROW) == \
        [(0.25, [(1, 0.5), (0, 0.5), (2, -4.0)]), None]
    rec = recommender()
    for kw in (dict(like=[None, None]), dict(like=[[], None], unlike=[None, []]), dict(unlike=[["nope"], {"neither": 1.0}]),
               dict(query_weight=3.0, like_weight=2.0, unlike_weight=0.0), dict(like=[["nope"], None], candidates=20)):
        plan = rec._plan(2, 10, **kw)
        assert plan.plain and plan is PLAIN, kw
    plan = rec._plan(2, 3, like=[["2"], None], unlike=[None, None], query_weight=2)
    assert not plan.plain and plan == RequestPlan(compose=[(2.0, [(1, 1.0)]), None])
    assert RequestPlan(None, None, None, False, None, None, None, None, None) == PLAIN  # positional construction as before
    # compose_plan is the LAST check: every other bad argument is named before a bad `like`
    with pytest.raises(ValueError, match="boosts given as ids needs boost_weight"):
        rec._plan(1, 10, boosts=[["1"]], like=["12"])
    with pytest.raises(ValueError, match="like of a batch"):
        rec._plan(1, 10, like="12")
    # like / unlike compose with the options that exclude each other
    plan = rec._plan(1, 3, like=[["1"]], probes=2, diversity=0.5)
    assert plan.probes == 2 and plan.compose == [(1.0, [(0, 1.0)])]
    with pytest.raises(AssertionError, match="model.tokenizer used"):
        rec.recommend("milk", 10, like=["1"], unlike={"2": 0.5}, aisles=["a0"], max_per_aisle=1)
    with pytest.raises(AssertionError, match="model.tokenizer used"):
        rec.recommend_batch(["milk"], 10, like=[["1"]], unlike=[{"2": 0.5}], within=["store"])
