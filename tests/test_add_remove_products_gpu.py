"""Recommender.add_products / remove_products end to end on the GPU, on the default world of tests/recommender_harness.py:
a synthetic 2-layer model directory, a 700-product synthetic catalog with aisle / department facets, two product sets,
and a second recommender with an IVF index.  After five products were added and seven removed, every kind of request
answers exactly as a new recommender answers it that was built on a corpus file written in the edited recommender's row
order."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender, text_facets
from instacart_next_order_recommendation_amd.search import IvfIndex
from tests.recommender_harness import graph_replays, no_gpu, synthetic_world, torch_cuda, write_corpus  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N = 700
SETS = {
    "store-1": [str(i) for i in range(1, N + 1) if i % 5 < 2],
    "in-stock": [str(i) for i in range(1, N + 1) if i % 7 != 0],
}
NEW_AISLE = "aisle 999 winter shelf"
# the first row, the last row (an added product), a member of both sets, a member of none, three more
REMOVED = ["1", "705", "5", "7", "300", "301", "699"]


def name_of(text):
    return text[len("Product: "):text.rfind(". Aisle: ")]


def make_additions(corpus):
    a3, d3 = text_facets(corpus["3"])
    a9, d9 = text_facets(corpus["9"])
    return {
        "701": f"Product: Crimson Harvest Granola. Aisle: {a3}. Department: {d3}.",
        "702": f"Product: Midnight Fennel Tonic. Aisle: {NEW_AISLE}. Department: {d3}.",
        "703": f"Product: Slow Amber Marmalade. Aisle: {a9}. Department: {d9}.",
        "704": corpus["100"],                                                             # another product's text: a tie
        "705": f"Product: Quiet Harbor Crackers. Aisle: {a9}. Department: {d9}.",
    }


@pytest.fixture(scope="module")
def world(tmp_path_factory, torch_cuda):
    tmp = tmp_path_factory.mktemp("add_remove_products")
    model_dir, corpus_path, corpus = synthetic_world(tmp, N)
    additions = make_additions(corpus)
    queries = syn.synthetic_user_contexts(4, seed=9) + [
        f"[+1d w0h1] {name_of(corpus['100'])}.", "[+1d w0h1] Crimson Harvest Granola.",
        f"[+2d w3h9] {name_of(corpus['1'])}, {name_of(corpus['300'])}, Midnight Fennel Tonic."]

    rec = MonitoredRecommender(model_dir, corpus_path, use_index=False, product_sets=SETS)
    ann = MonitoredRecommender(model_dir, corpus_path, use_index=False, ann_lists=8)
    assert rec._fast is not None and rec._index.storage.endswith("filter")
    before = [rec.recommend(q, 20) for q in queries]                                      # graphs captured BEFORE the edits
    for r in (rec, ann):
        r.add_products(additions)
        r.remove_products(REMOVED)
    edited_path = write_corpus(tmp / "edited", {pid: rec.pid_to_text[pid] for pid in rec.product_ids})   # rec's row order
    fresh = MonitoredRecommender(model_dir, edited_path, use_index=False, product_sets=SETS)
    return {"rec": rec, "ann": ann, "fresh": fresh, "queries": queries, "additions": additions, "corpus": corpus,
            "before": before}


def test_host_state_follows(world):
    rec, ann, fresh, corpus = world["rec"], world["ann"], world["fresh"], world["corpus"]
    n = N + 5 - 7
    assert len(rec.product_ids) == len(rec.product_texts) == len(rec.pid_to_text) == len(rec._pid_to_row) == n
    assert rec._index.n_rows == n and rec._index.capacity == 2 * N and rec.product_embeddings.shape[0] == n
    assert rec.product_ids == fresh.product_ids == ann.product_ids and rec.product_texts == fresh.product_texts
    assert rec._pid_to_row == fresh._pid_to_row and rec.pid_to_text == fresh.pid_to_text
    assert not set(REMOVED) & set(rec.product_ids) and {"701", "702", "703", "704"} <= set(rec.product_ids)
    # the plan: 705 products, 7 removed -> rows 698 .. 704 leave; the holes 0, 4, 6, 299, 300 take the survivors behind
    assert rec.product_ids[:7] == ["700", "2", "3", "4", "701", "6", "702"] and rec.product_ids[299:301] == ["703", "704"]
    assert rec.product_embeddings.tobytes() == fresh.product_embeddings.tobytes()
    assert rec.aisles[-1] == NEW_AISLE and rec.aisles[:-1] == list(dict.fromkeys(text_facets(t)[0] for t in corpus.values()))
    assert set(fresh.aisles) <= set(rec.aisles) and set(fresh.departments) <= set(rec.departments)
    np.testing.assert_array_equal(rec._set_member, fresh._set_member)
    assert rec._set_member.shape == (2, n) and not rec._set_member[:, rec._pid_to_row["701"]].any()
    assert (rec._index.export() == fresh._index.export()).all()
    for got, want in zip(rec._index.export_filter(), fresh._index.export_filter()):
        assert (got.view(torch.int16) == want.view(torch.int16)).all()


def test_requests_answer_as_a_new_recommender(world, monkeypatch):
    rec, fresh, queries, additions = world["rec"], world["fresh"], world["queries"], world["additions"]
    fast = rec._fast_path()
    calls = graph_replays(rec, monkeypatch)
    got = [rec.recommend(q, 20) for q in queries]
    assert calls and all(c is fast for c in calls)                                        # the graph path, captured again
    assert got == [fresh.recommend(q, 20) for q in queries] and got != world["before"]
    assert rec.recommend_batch(queries, 20) == fresh.recommend_batch(queries, 20) == got
    assert not set(REMOVED) & {p for g in got for p, _ in g}
    all_of_them = rec.recommend_batch(queries, 128)
    assert all_of_them == fresh.recommend_batch(queries, 128)
    assert not set(REMOVED) & {p for g in all_of_them for p, _ in g}
    # a removed id in an exclusion list or a boost list is an id the catalog does not have: skipped
    excl = [{p for p, _ in g[:3]} | {"300", "1"} for g in got]
    assert rec.recommend_batch(queries, 20, excl) == fresh.recommend_batch(queries, 20, excl)
    assert rec.recommend(queries[0], 20, exclude_product_ids={"300", "705"}) == got[0]
    boosts = {"702": 0.5, "300": 5.0, "17": 1.0, "3": 0.1, "705": 2.0}
    for q in queries[3:]:
        assert rec.recommend(q, 20, boosts=boosts) == fresh.recommend(q, 20, boosts=boosts)
        only = rec.recommend(q, 20, boosts=boosts, only_boosted=True)
        assert only == fresh.recommend(q, 20, boosts=boosts, only_boosted=True)
        assert {p for p, _ in only} == {"702", "17", "3"}
    # a query equal to an added product's text returns that product first; 704 carries product 100's text: a tie
    for pid in ("701", "702", "703"):
        assert rec.recommend(additions[pid], 5)[0][0] == pid
    tie = rec.recommend(additions["704"], 5)
    assert [p for p, _ in tie[:2]] == ["100", "704"] and tie[0][1] == tie[1][1] and tie == fresh.recommend(additions["704"], 5)


def test_facets_sets_caps_and_diversity(world):
    rec, fresh, queries, corpus = world["rec"], world["fresh"], world["queries"], world["corpus"]
    a3 = text_facets(corpus["3"])[0]
    for q in queries[3:]:
        new = rec.recommend(q, 20, aisles=[NEW_AISLE])
        assert new == fresh.recommend(q, 20, aisles=[NEW_AISLE]) and [p for p, _ in new] == ["702"]
        a = [a3, NEW_AISLE, rec.aisles[0]]
        assert rec.recommend(q, 20, aisles=a) == fresh.recommend(q, 20, aisles=a)
        assert "701" in {p for p, _ in rec.recommend(q, 128, aisles=[a3])}
        d = [rec.departments[1], rec.departments[0]]
        assert rec.recommend(q, 20, departments=d) == fresh.recommend(q, 20, departments=d)
        for w in ("store-1", "in-stock", ["store-1", "in-stock"]):
            got = rec.recommend(q, 128, within=w)
            assert got == fresh.recommend(q, 128, within=w)
            assert not {"701", "702", "703", "704", "5"} & {p for p, _ in got}            # the new products join no set
        assert rec.recommend(q, 20, max_per_aisle=1) == fresh.recommend(q, 20, max_per_aisle=1)
        assert rec.recommend(q, 20, max_per_aisle=2, max_per_department=3) == \
            fresh.recommend(q, 20, max_per_aisle=2, max_per_department=3)
        assert rec.recommend(q, 10, diversity=0.4) == fresh.recommend(q, 10, diversity=0.4)
    moved = rec.recommend(queries[0], 5, within="store-1", boosts={"700": 0.0, "701": 0.0, "7": 0.0}, only_boosted=True)
    assert [p for p, _ in moved] == ["700"]                                               # a moved product stays in its set
    a = [[NEW_AISLE], None, [a3]]
    assert rec.recommend_batch(queries[:3], 20, aisles=a) == fresh.recommend_batch(queries[:3], 20, aisles=a)
    rec.update_product_set("store-1", ["701", "2", "300"])                                # an added product joins a set
    fresh.update_product_set("store-1", ["701", "2", "300"])
    try:
        got = rec.recommend(queries[5], 20, within="store-1")
        assert got == fresh.recommend(queries[5], 20, within="store-1") and {p for p, _ in got} == {"701", "2"}
    finally:
        rec.update_product_set("store-1", SETS["store-1"])
        fresh.update_product_set("store-1", SETS["store-1"])


def test_probes_after_the_ivf_was_built_again(world):
    ann, fresh, queries = world["ann"], world["fresh"], world["queries"]
    assert ann._ann is not None and ann._ann.n_lists == 8
    fresh._ann = IvfIndex(fresh._index, ann._ann.centroids)
    try:
        for q in queries:
            exact = fresh.recommend(q, 20)
            assert ann.recommend(q, 20) == exact
            assert ann.recommend(q, 20, probes=8) == exact
            assert ann.recommend(q, 20, probes=2) == fresh.recommend(q, 20, probes=2)
        assert ann.recommend_batch(queries, 20, probes=2) == fresh.recommend_batch(queries, 20, probes=2)
    finally:
        fresh._ann.close()
        fresh._ann = None


def test_a_bad_edit_changes_nothing(world, monkeypatch):
    rec, queries = world["rec"], world["queries"]
    answers = [rec.recommend(q, 20) for q in queries]
    ids, texts, aisles = list(rec.product_ids), list(rec.product_texts), list(rec.aisles)
    stored = rec._index.export().clone()
    monkeypatch.setattr(type(rec._index), "append_rows", no_gpu)
    monkeypatch.setattr(type(rec._index), "remove_rows", no_gpu)
    monkeypatch.setattr(type(rec.model), "encode", no_gpu)
    good = "Product: Plain Oats. Aisle: one more new aisle. Department: dept novel."
    with pytest.raises(ValueError, match="already"):
        rec.add_products({"800": good, "2": good})
    with pytest.raises(ValueError, match="format"):
        rec.add_products({"800": good, "801": "Plain oats, 500 g"})
    with pytest.raises(ValueError, match="unknown product id"):
        rec.remove_products(["2", "300"])                                                 # 300 was removed before
    with pytest.raises(ValueError, match="twice"):
        rec.remove_products(["2", "2"])
    with pytest.raises(ValueError, match="every product"):
        rec.remove_products(list(rec.product_ids))
    rec.add_products({})
    rec.remove_products([])
    monkeypatch.undo()
    assert rec.product_ids == ids and rec.product_texts == texts and rec.aisles == aisles
    assert (rec._index.export() == stored).all()
    assert [rec.recommend(q, 20) for q in queries] == answers
