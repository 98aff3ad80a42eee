"""Recommender._plan / RequestPlan without a GPU: on a Recommender made with __new__ (six products, facets, two product
sets, a stub IVF index of 4 lists) - when a plan is plain, what it holds, that every bad argument raises its text from
recommend, recommend_batch and recommend_batch_timed before the model is touched, and the facet-code loop the update
and add plans share at the 256th and 257th name."""
from __future__ import annotations

import re

import numpy as np
import pytest

from instacart_next_order_recommendation_amd.recommender import (Recommender, RequestPlan, product_add_plan,
                                                                 product_update_plan)

PER_QUERY = ("aisles", "departments", "within", "boosts")


class NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"model.{name} used before the arguments were checked")


class Ann:
    n_lists = 4


def recommender(bare: bool = False) -> Recommender:
    """Products "1".."6" on rows 0..5; unless bare: aisles a0..a2, departments d0 / d1, the sets store = rows 0-2 and
    stock = rows 1-3, an IVF index of 4 lists."""
    rec = Recommender.__new__(Recommender)
    rec.model = NoModel()
    rec.product_ids = [str(i + 1) for i in range(6)]
    rec._pid_to_row = {p: i for i, p in enumerate(rec.product_ids)}
    if not bare:
        rec.aisles, rec.departments = ["a0", "a1", "a2"], ["d0", "d1"]
        rec.product_sets = ["store", "stock"]
        rec._set_member = np.array([[1, 1, 1, 0, 0, 0], [0, 1, 1, 1, 0, 0]], bool)
        rec._ann = Ann()
    return rec


def test_plain_exactly_when_nothing_is_asked():
    rec = recommender()
    assert RequestPlan().plain and rec._plan(2, 10).plain
    off = dict(aisles=[None, [None, None]], departments=[None, [None, None]], diversity=[None, 0, 0.0], candidates=[None],
               boosts=[None, [None, None], [{}, []], [{"no such product": 1.0}, None]], boost_weight=[None, 0.5],
               only_boosted=[False], probes=[None], within=[None, [None, None]], max_per_aisle=[None],
               max_per_department=[None])
    for name, values in off.items():
        for v in values:
            assert rec._plan(2, 10, **{name: v}).plain, (name, v)
    assert rec._plan(2, 10, **{name: values[-1] for name, values in off.items()}).plain
    # `candidates` alone asks nothing either: it is the width of a diversified or capped request
    assert rec._plan(2, 10, candidates=20).plain
    assert rec._plan(2, 10) is rec._plan(1, 5, candidates=20, boosts=[{}], diversity=0)  # one shared plan for all of them
    on = [dict(aisles=[["a0"], None]), dict(aisles=[None, []]), dict(departments=[None, "d1"]), dict(diversity=0.3),
          dict(diversity=1), dict(boosts=[{"1": 1.0}, None]), dict(boosts=[None, ["2"]], boost_weight=0.0),
          dict(only_boosted=True), dict(probes=2), dict(within=["store", None]), dict(within=[None, ["store", "stock"]]),
          dict(max_per_aisle=1), dict(max_per_department=2)]
    for kw in on:
        assert not rec._plan(2, 10, **kw).plain, kw


def test_what_a_plan_holds():
    rec = recommender()
    plan = rec._plan(2, 3, aisles=[["a2", "a0"], None], departments=[None, None], within=["stock", None], diversity=0.25,
                     candidates=5, max_per_department=2)
    assert plan == RequestPlan(allow=[([2, 0], None), None], sets=[[1], None], caps=(0, 2), mmr=(0.75, 5), width=5)
    assert rec._plan(1, 3, probes=4, diversity=0.5) == RequestPlan(probes=4, mmr=(0.5, 6))  # min(128, 4 * 3) of 6 products
    plan = rec._plan(1, 3, only_boosted=True)
    assert plan.boost == [{}] and plan.only_boosted and not plan.plain
    with pytest.raises(AttributeError):
        plan.caps = (1, 1)  # frozen


def test_boosted_rows_outside_the_querys_sets_are_dropped_at_plan_time():
    rec = recommender()
    boosts = [{"1": 1.0, "5": 2.0}, {"2": 1.0, "4": 1.5}, {"6": 3.0}]
    plan = rec._plan(3, 2, boosts=boosts, within=["store", ["store", "stock"], None])
    assert plan.boost == [{0: 1.0}, {1: 1.0}, {5: 3.0}] and plan.sets == [[0], [0, 1], None] and not plan.only_boosted
    assert rec._plan(3, 2, boosts=boosts).boost == [{0: 1.0, 4: 2.0}, {1: 1.0, 3: 1.5}, {5: 3.0}]
    plan = rec._plan(1, 2, boosts=[["4", "5"]], boost_weight=0.5, only_boosted=True, within=["stock"])
    assert plan.boost == [{3: 0.5}] and plan.only_boosted


# (the options as recommend takes them, the text of the ValueError)
BAD = [
    (dict(probes=0), "probes must be an integer in [1, 4], got 0"),
    (dict(probes=2, aisles=["a0"]), "probes cannot be combined with aisles: the IVF search takes exclusions and diversity only"),
    (dict(probes=2, max_per_aisle=1), "probes cannot be combined with max_per_aisle"),
    (dict(max_per_aisle=0), "max_per_aisle must be an integer >= 1, got 0"),
    (dict(max_per_department=True), "max_per_department must be an integer >= 1, got True"),
    (dict(within="nope"), "unknown product set 'nope'"),
    (dict(within=["store"] * 5), "within names 5 product sets, more than 4"),
    (dict(diversity=1.5), "diversity must be in [0, 1], got 1.5"),
    (dict(candidates=5), "candidates must be in [top_k = 10, 128], got 5"),
    (dict(aisles=["a1", "nope"]), "unknown aisle 'nope'"),
    (dict(departments="nope"), "unknown department 'nope'"),
    (dict(boosts="12"), "boosts must be a mapping product id -> weight or an iterable of product ids, not a string"),
    (dict(boosts=["1"]), "boosts given as ids needs boost_weight"),
    (dict(boosts={"1": -1.0}), "the boost weight of '1' must be a number >= 0, got -1.0"),
    (dict(boost_weight="heavy"), "boost_weight must be a number >= 0, got 'heavy'"),
]
BAD_BARE = [
    (dict(probes=2), "probes needs a recommender built with ann_lists"),
    (dict(max_per_aisle=2), "max_per_aisle / max_per_department need a catalog with aisle / department facets"),
    (dict(within="store"), "within needs a recommender built with product_sets"),
    (dict(aisles=["a0"]), "this catalog has no aisle / department facets"),
]


def entry_points(rec, kw):
    """The three calls with recommend's options `kw`, the per-query ones wrapped for the batch forms."""
    batch = {name: [v] if name in PER_QUERY else v for name, v in kw.items()}
    calls = [lambda: rec.recommend("milk", 10, **kw), lambda: rec.recommend_batch(["milk"], 10, **batch)]
    if "probes" not in kw:  # (recommend_batch_timed has no probes keyword)
        calls.append(lambda: rec.recommend_batch_timed(["milk"], 10, **batch))
    return calls


@pytest.mark.parametrize("bare,kw,text", [(False, *b) for b in BAD] + [(True, *b) for b in BAD_BARE],
                         ids=[t[:40] for _, t in BAD + BAD_BARE])
def test_bad_arguments_raise_their_text_before_the_model_is_used(bare, kw, text):
    rec = recommender(bare)
    for call in entry_points(rec, kw):
        with pytest.raises(ValueError, match=re.escape(text)):
            call()


def test_good_arguments_reach_the_model_and_top_k_is_checked_first():
    rec = recommender()
    for call in entry_points(rec, dict(aisles=["a0"], within="store", boosts={"1": 1.0}, diversity=0.5, max_per_aisle=1)):
        with pytest.raises(AssertionError, match="model.tokenizer used"):
            call()
    with pytest.raises(ValueError, match="top_k=129 exceeds the kernel limit 128"):
        rec.recommend("milk", 129, max_per_aisle=0)
    with pytest.raises(ValueError, match="top_k=129 exceeds the kernel limit 128"):
        rec.recommend_batch_timed(["milk"], 129, max_per_aisle=0)
    assert rec.recommend_batch([], 129, diversity=0.5) == []  # no query: options checked, top_k not
    with pytest.raises(ValueError, match="diversity"):
        rec.recommend_batch([], 129, diversity=1.5)
    with pytest.raises(ValueError, match="aisles has 1 entries for 0 queries"):  # the facets are options like the others
        rec.recommend_batch([], 10, aisles=[["a0"]])
    with pytest.raises(TypeError):
        rec.recommend_batch_timed(["milk"], 10, probes=2)


def test_the_first_bad_argument_in_plan_order_is_named():
    rec = recommender()
    bad = dict(probes=9, max_per_aisle=0, within=["nope"], diversity=2, aisles=[["nope"]], boosts=[["1"]])
    # probes with aisles is ann_plan's own complaint; then each next check once the one before it is satisfied
    for name, text in (("probes", "probes cannot be combined with aisles"), ("max_per_aisle", "max_per_aisle must be"),
                       ("within", "unknown product set"), ("diversity", "diversity must be"), ("aisles", "unknown aisle"),
                       ("boosts", "boosts given as ids needs boost_weight")):
        with pytest.raises(ValueError, match=text):
            rec._plan(1, 10, **bad)
        del bad[name]
    assert rec._plan(1, 10, **bad).plain


def test_update_and_add_plans_share_the_facet_codes_at_the_256th_and_257th_name():
    aisles, departments = [f"a{i}" for i in range(255)], ["d0"]
    pid_to_row, texts = {"1": 0, "2": 1}, ["Product: x. Aisle: a0. Department: d0."] * 2

    def text(aisle, department="d0"):
        return f"Product: new. Aisle: {aisle}. Department: {department}."

    for plan, ids in ((lambda m: product_update_plan(m, pid_to_row, texts, aisles, departments), ("1", "2")),
                      (lambda m: product_add_plan(m, pid_to_row, aisles, departments), ("8", "9"))):
        keys, new_texts, codes, a, d = plan({ids[0]: text("a7", "d1"), ids[1]: text("the 256th")})
        by_key = dict(zip(keys, codes.tolist()))
        first, second = (0, 1) if ids == ("1", "2") else ids  # (the update plan returns rows)
        assert by_key[first] == [7, 1] and by_key[second] == [255, 0] and codes.dtype == np.uint8
        assert a == aisles + ["the 256th"] and d == ["d0", "d1"] and len(aisles) == 255 and departments == ["d0"]  # copies
        with pytest.raises(ValueError, match=re.escape("'one more' would be the 257th aisle name; a facet has 256 values")):
            plan({ids[0]: text("the 256th"), ids[1]: text("one more")})
    many = [f"d{i}" for i in range(256)]
    with pytest.raises(ValueError, match=re.escape("'d256' would be the 257th department name; a facet has 256 values")):
        product_add_plan({"8": text("a0", "d256")}, pid_to_row, aisles, many)
    with pytest.raises(ValueError, match=re.escape("'d256' would be the 257th department name; a facet has 256 values")):
        product_update_plan({"1": text("a0", "d256")}, pid_to_row, texts, aisles, many)
    # each plan's own text for a text that does not parse; a catalog without facets parses nothing
    with pytest.raises(ValueError, match="the new text of row 1 is not in the 'Product: .. Aisle: .. Department: ..' format"):
        product_update_plan({"2": "milk"}, pid_to_row, texts, aisles, departments)
    with pytest.raises(ValueError, match="the text of product '8' is not in the 'Product: .. Aisle: .. Department: ..' format"):
        product_add_plan({"8": "milk"}, pid_to_row, aisles, departments)
    assert product_update_plan({"2": "milk"}, pid_to_row, texts, None, None) == ([1], ["milk"], None, None, None)
    assert product_add_plan({"8": "milk"}, pid_to_row, None, None) == (["8"], ["milk"], None, None, None)
