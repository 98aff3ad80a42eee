"""Recommender.recommend(..., within=) end to end on the GPU, on the default world of tests/recommender_harness.py (a
synthetic 2-layer model directory, a 700-product synthetic catalog) and four product sets.  A request inside product
sets equals, ids and scores, the request that excludes every product outside them."""
from __future__ import annotations

import json

import pytest
import yaml

from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender
from tests.recommender_harness import (QUERIES, assert_batch_equals_single_calls, forbid_gpu_work, graph_replays,  # noqa: F401
                                       synthetic_world, torch_cuda)

pytestmark = pytest.mark.gpu

N = 700
SETS = {
    "store-1": [str(i) for i in range(1, N + 1) if i % 5 < 2] + ["no such product"],   # about 40 % of the catalog
    "store-2": [str(i) for i in range(1, N + 1) if i % 3 == 0],
    "in-stock": [str(i) for i in range(1, N + 1) if i % 7 != 0],
    "tiny": ["3", "30", "300"],
}


@pytest.fixture(scope="module")
def world(tmp_path_factory, torch_cuda):
    tmp = tmp_path_factory.mktemp("rowset_rec")
    w = synthetic_world(tmp, N)
    sets_path = tmp / "product_sets.json"
    sets_path.write_text(json.dumps(SETS))
    r = MonitoredRecommender(w.model_dir, w.corpus_path, use_index=False, product_sets=sets_path)   # the JSON file form
    assert r._fast is not None and r._index.n_rowsets == 4 and r.product_sets == list(SETS)
    return r, sets_path


@pytest.fixture()
def rec(world):
    return world[0]


def outside(rec, *names, sets=SETS):
    """The ids of every product that is not in all of the named sets."""
    inside = set(rec.product_ids)
    for name in names:
        inside &= set(sets[name])
    return set(rec.product_ids) - inside


def test_within_returns_members_and_equals_the_exclusion_of_the_rest(rec):
    for q in QUERIES:
        got = rec.recommend(q, 20, within="store-1")
        assert len(got) == 20 and all(p in SETS["store-1"] for p, _ in got)
        assert got == rec.recommend(q, 20, exclude_product_ids=outside(rec, "store-1"))
        assert got == rec.recommend(q, 20, within=["store-1"])
        two = rec.recommend(q, 20, within=["store-1", "in-stock"])                      # the intersection
        assert two and all(p in SETS["store-1"] and p in SETS["in-stock"] for p, _ in two)
        assert two == rec.recommend(q, 20, exclude_product_ids=outside(rec, "store-1", "in-stock"))
        tiny = rec.recommend(q, 20, within="tiny")
        assert sorted(p for p, _ in tiny) == ["3", "30", "300"]
        assert rec.recommend(q, 20, within=["tiny", "in-stock", "store-2", "store-1"]) == \
            rec.recommend(q, 20, exclude_product_ids=outside(rec, "tiny", "in-stock", "store-2", "store-1"))
        drop = {p for p, _ in got[:3]}
        less = rec.recommend(q, 20, exclude_product_ids=drop, within="store-1")
        assert less == rec.recommend(q, 20, exclude_product_ids=outside(rec, "store-1") | drop) and not drop & {p for p, _ in less}
        assert rec.recommend(q, 20, within=[]) == rec.recommend(q, 20) == rec.recommend(q, 20, within=None)


def test_within_composes_with_aisles_diversity_and_boosts(rec):
    out = outside(rec, "store-1", "in-stock")
    w = ["store-1", "in-stock"]
    a = [rec.aisles[0], rec.aisles[2], rec.aisles[5]]
    for q in QUERIES[:3]:
        assert rec.recommend(q, 10, within=w, aisles=a) == rec.recommend(q, 10, exclude_product_ids=out, aisles=a)
        assert rec.recommend(q, 10, within=w, diversity=0.4) == rec.recommend(q, 10, exclude_product_ids=out, diversity=0.4)
        far = [p for p, _ in rec.recommend(q, 80)][-12:]                                # some inside the sets, some not
        assert 0 < len(set(far) - out) < len(far)
        boosts = {p: 1.5 + 0.1 * i for i, p in enumerate(far)}
        got = rec.recommend(q, 20, within=w, boosts=boosts)
        assert got == rec.recommend(q, 20, exclude_product_ids=out, boosts=boosts)
        assert not {p for p, _ in got} & out and {p for p, _ in got} >= set(far) - out
        only = rec.recommend(q, 20, within=w, boosts=boosts, only_boosted=True)
        assert only == rec.recommend(q, 20, exclude_product_ids=out, boosts=boosts, only_boosted=True)
        assert {p for p, _ in only} == set(far) - out
        both = rec.recommend(q, 10, within=w, boosts=far, boost_weight=0.7, diversity=0.3, aisles=None)
        assert both == rec.recommend(q, 10, exclude_product_ids=out, boosts=far, boost_weight=0.7, diversity=0.3)


def test_batch_with_per_query_within(rec):
    within = ["store-1", None, ["store-2", "in-stock"], "tiny", []]
    excl = [None, None, {"3", "6", "9"}, {"30"}, None]
    batch = assert_batch_equals_single_calls(rec, QUERIES, 20, excl, within=within)
    assert batch[1] == rec.recommend(QUERIES[1], 20) and sorted(p for p, _ in batch[3]) == ["3", "300"]
    assert batch[2] == rec.recommend(QUERIES[2], 20, exclude_product_ids=outside(rec, "store-2", "in-stock") | excl[2])
    assert rec.recommend_batch(QUERIES, 20, excl, within=[None] * 5) == rec.recommend_batch(QUERIES, 20, excl)
    rec.last_metrics = None
    got = rec.recommend(QUERIES[0], 20, user_id="u7", within="store-2")
    assert rec.last_metrics.user_id == "u7" and rec.last_metrics.num_recommendations == len(got) == 20


def test_bad_within_raises_before_any_gpu_work(rec, monkeypatch):
    forbid_gpu_work(rec, monkeypatch)
    with pytest.raises(ValueError, match="no such set"):
        rec.recommend(QUERIES[0], 20, within="no such set")
    with pytest.raises(ValueError, match="more than 4"):
        rec.recommend(QUERIES[0], 20, within=["store-1", "store-2", "in-stock", "tiny", "store-1"])
    with pytest.raises(ValueError, match="no such set"):
        rec.recommend_batch(QUERIES[:2], 20, within=[None, ["store-1", "no such set"]])
    with pytest.raises(ValueError, match="entries"):
        rec.recommend_batch(QUERIES[:2], 20, within=["store-1"])
    with pytest.raises(ValueError, match="ann_lists|within"):
        rec.recommend(QUERIES[0], 20, within="store-1", probes=2)


def test_requests_without_within_stay_on_the_graph_path(rec, monkeypatch):
    calls = graph_replays(rec, monkeypatch)
    plain = rec.recommend(QUERIES[0], 20)
    assert len(calls) == 1
    assert rec.recommend(QUERIES[0], 20, within="store-1") != plain and len(calls) == 1
    assert rec.recommend(QUERIES[0], 20, within=None) == plain and len(calls) == 2


def test_update_product_set_takes_effect_on_the_next_request(rec):
    q = QUERIES[2]
    before = rec.recommend(q, 20, within="in-stock")
    other = rec.recommend(q, 20, within="store-2")
    sold_out = {p for p, _ in before[:5]}
    members = [p for p in SETS["in-stock"] if p not in sold_out] + ["unknown id"]
    try:
        rec.update_product_set("in-stock", members)
        now = {**SETS, "in-stock": members}
        after = rec.recommend(q, 20, within="in-stock")
        assert not sold_out & {p for p, _ in after}
        assert after == rec.recommend(q, 20, exclude_product_ids=outside(rec, "in-stock", sets=now))
        assert rec.recommend(q, 20, within="store-2") == other                           # only that set's requests change
        boosts = {p: 2.0 for p in sold_out}                                              # the host's copy follows: sold-out boosts are dropped
        assert rec.recommend(q, 20, within="in-stock", boosts=boosts) == after
        with pytest.raises(ValueError, match="no such set"):
            rec.update_product_set("no such set", members)
    finally:
        rec.update_product_set("in-stock", SETS["in-stock"])
    assert rec.recommend(q, 20, within="in-stock") == before


def test_recommender_without_product_sets_refuses_within(rec):
    other = type(rec)(rec.model_dir, rec.corpus_path, use_index=False)
    assert other.product_sets is None and other._index.n_rowsets == 0
    assert len(other.recommend(QUERIES[0], 5)) == 5
    with pytest.raises(ValueError, match="product_sets"):
        other.recommend(QUERIES[0], 5, within="store-1")
    with pytest.raises(ValueError, match="product_sets"):
        other.recommend_batch(QUERIES[:2], 5, within=[None, "store-1"])
    with pytest.raises(ValueError, match="product_sets"):
        other.update_product_set("store-1", ["1"])
    mapped = type(rec)(rec.model_dir, rec.corpus_path, use_index=False, product_sets=SETS)   # the mapping form
    assert mapped.recommend(QUERIES[0], 5, within="tiny") == rec.recommend(QUERIES[0], 5, within="tiny")


def test_cli_flags(world, tmp_path, capsys):
    from instacart_next_order_recommendation_amd import cli

    rec, sets_path = world
    cfg = tmp_path / "inference.yaml"
    cfg.write_text(yaml.safe_dump({"model_dir": str(rec.model_dir), "corpus": str(rec.corpus_path), "use_index": False,
                                   "top_k": 5, "query": QUERIES[0]}))
    assert cli.main(["--config", str(cfg), "--json", "--product-sets", str(sets_path), "--within", "store-1", "--within", "in-stock"]) == 0
    rows = [json.loads(ln) for ln in capsys.readouterr().out.splitlines()]
    assert [(r["product_id"], r["score"]) for r in rows] == rec.recommend(QUERIES[0], 5, within=["store-1", "in-stock"])
    with pytest.raises(SystemExit, match="--product-sets"):
        cli.main(["--config", str(cfg), "--within", "store-1"])
    with pytest.raises(SystemExit, match="does not exist"):
        cli.main(["--config", str(cfg), "--product-sets", str(tmp_path / "missing.json"), "--within", "store-1"])
    with pytest.raises(SystemExit, match="no such set"):
        cli.main(["--config", str(cfg), "--product-sets", str(sets_path), "--within", "no such set"])
