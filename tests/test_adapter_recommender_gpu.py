"""Recommender(adapter=) / set_adapter / fit_adapter end to end on the GPU, on the default world of
tests/recommender_harness.py: a request with an adapter equals encode, the reference's apply and DeviceIndex.search by
hand, bit for bit, on the graph path and in a batch; a zero adapter and no adapter are the plain recommender; training
the installed adapter needs no re-capture; like= and aisles= compose with it; queries made of stored rows ignore it."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.adapter import QueryAdapter
from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender
from instacart_next_order_recommendation_amd.search import facet_masks
from tests import adapter_reference as ref
from tests.adapter_harness import by_hand
from tests.recommender_harness import (QUERIES, as_results, assert_batch_equals_single_calls, graph_replays, synthetic_world,
                                       torch_cuda)  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return synthetic_world(tmp_path_factory.mktemp("adapter_rec"))


@pytest.fixture(scope="module")
def shared_rec(world, torch_cuda):
    r = MonitoredRecommender(world.model_dir, world.corpus_path, use_index=False)
    assert r._fast is not None and r._adapter is None and len(r.product_ids) == 700
    return r


@pytest.fixture(scope="module")
def plain(shared_rec):
    """What the recommender answers without an adapter, recorded before any test sets one."""
    excl = [None, {shared_rec.product_ids[3]}, None, None, set(shared_rec.product_ids[:50])]
    return excl, [shared_rec.recommend(q, 10, exclude_product_ids=e) for q, e in zip(QUERIES, excl)], \
        shared_rec.recommend_batch(QUERIES, 10, excl)


@pytest.fixture
def rec(shared_rec, plain):
    yield shared_rec
    shared_rec.set_adapter(None)


def random_delta(dim, seed=1, size=0.5):
    return (np.random.default_rng(seed).standard_normal((dim, dim)) * (size / np.sqrt(dim))).astype(np.float32)


def adapter_of(rec, delta) -> QueryAdapter:
    ad = QueryAdapter(rec._index.dim, rec.device)
    ad.load_state({"delta": delta})
    return ad


def test_requests_go_through_the_adapter_bit_for_bit(rec, plain, monkeypatch):
    excl, plain_single, _ = plain
    delta = random_delta(rec._index.dim)
    rec.set_adapter(adapter_of(rec, delta))
    replays = graph_replays(rec, monkeypatch)
    got = [rec.recommend(q, 10, exclude_product_ids=e) for q, e in zip(QUERIES, excl)]
    assert len(replays) == len(QUERIES)  # every plain request still replays a captured graph
    for q, e, g, p in zip(QUERIES, excl, got, plain_single):
        assert g == by_hand(rec, delta, q, 10, e) and len(g) == 10
        assert [pid for pid, _ in g] != [pid for pid, _ in p]  # and an adapter of this size changes the ranking
    batch = assert_batch_equals_single_calls(rec, QUERIES, 10, excl)
    assert batch == got
    assert list(rec.recommend_batches([QUERIES[:3], QUERIES[3:]], 10, [excl[:3], excl[3:]])) == [got[:3], got[3:]]
    # the un-captured single request (graphs off) is the same request
    monkeypatch.setattr(rec, "_fast_path", lambda: None)
    assert [rec.recommend(q, 10, exclude_product_ids=e) for q, e in zip(QUERIES, excl)] == got
    assert rec.last_metrics.similarity_compute_time_ms > 0


def test_zero_adapter_and_no_adapter_are_the_plain_recommender(rec, plain, world, monkeypatch, tmp_path):
    excl, plain_single, plain_batch = plain
    rec.set_adapter(QueryAdapter(rec._index.dim, rec.device))
    assert [rec.recommend(q, 10, exclude_product_ids=e) for q, e in zip(QUERIES, excl)] == plain_single
    assert rec.recommend_batch(QUERIES, 10, excl) == plain_batch
    rec.set_adapter(adapter_of(rec, random_delta(rec._index.dim)))
    assert rec.recommend_batch(QUERIES, 10, excl) != plain_batch
    rec.set_adapter(None)
    launched = []
    monkeypatch.setattr(QueryAdapter, "apply_into", lambda *a: launched.append(a))
    assert [rec.recommend(q, 10, exclude_product_ids=e) for q, e in zip(QUERIES, excl)] == plain_single
    assert rec.recommend_batch(QUERIES, 10, excl) == plain_batch and not launched
    monkeypatch.undo()
    # a file as the constructor's argument; an adapter of another width is refused
    delta = random_delta(rec._index.dim, seed=2)
    adapter_of(rec, delta).save(tmp_path / "adapter.npz")
    other = MonitoredRecommender(world.model_dir, world.corpus_path, use_index=False, adapter=tmp_path / "adapter.npz")
    assert other.recommend(QUERIES[0], 10) == by_hand(other, delta, QUERIES[0], 10)
    with pytest.raises(ValueError, match="wide"):
        rec.set_adapter(QueryAdapter(64, rec.device))
    assert rec._adapter is None


def test_fit_adapter_trains_in_place_without_a_recapture(rec, monkeypatch):
    rng = np.random.default_rng(3)
    contexts = syn.synthetic_user_contexts(48, seed=5)
    pairs = [(c, rec.product_ids[int(r)]) for c, r in zip(contexts, rng.integers(0, 700, 48))]
    with pytest.raises(ValueError, match="unknown product id"):
        rec.fit_adapter(pairs + [("x", "no-such-product")])
    assert rec._adapter is None
    first = rec.fit_adapter(pairs, epochs=2, batch_size=16, negatives=32, lr=1e-2)  # trains a new adapter and installs it
    ad = rec._adapter
    assert ad is not None and len(first) == 6 and ad.steps == 6 and np.isfinite(first).all()
    replays = graph_replays(rec, monkeypatch)
    assert rec.recommend(QUERIES[0], 10) == by_hand(rec, ad.state()["delta"], QUERIES[0], 10)
    captured = dict(rec._fast_path()._graphs)
    assert captured
    more = rec.fit_adapter(pairs, epochs=3, batch_size=16, lr=1e-2)  # the installed one, in place
    assert rec._adapter is ad and ad.steps == 6 + 9 and np.mean(more) < np.mean(first[:3])
    delta = ad.state()["delta"]
    assert rec.recommend(QUERIES[0], 10) == by_hand(rec, delta, QUERIES[0], 10)
    assert len(replays) == 2 and all(rec._fast_path()._graphs[key] is c for key, c in captured.items())


def test_like_and_aisles_compose_with_the_adapter(rec):
    delta = random_delta(rec._index.dim, seed=4)
    rec.set_adapter(adapter_of(rec, delta))
    query, liked = QUERIES[1], [rec.product_ids[10], rec.product_ids[333]]
    aisle = rec.aisles[2]
    q = torch.from_numpy(ref.apply(delta, rec.model.encode([query]))).to(rec.device)
    composed = rec._index.compose_queries(q, [[(10, 0.5), (333, 0.5)]], [1.0])
    idx, sc = rec._index.search(composed, 10)
    assert rec.recommend(query, 10, like=liked) == as_results(rec, idx[0].cpu().numpy(), sc[0].cpu().numpy())
    allow = facet_masks([([2], None)], 1, rec._index.n_facets, rec.device)
    idx, sc = rec._index.search(composed, 10, None, allow)
    got = rec.recommend(query, 10, like=liked, aisles=[aisle])
    assert got == as_results(rec, idx[0].cpu().numpy(), sc[0].cpu().numpy()) and got
    assert all(f". Aisle: {aisle}. " in rec.pid_to_text[p] for p, _ in got)


def test_queries_made_of_stored_rows_ignore_the_adapter(rec):
    pid, basket = rec.product_ids[42], [rec.product_ids[r] for r in (5, 17, 600)]
    want = rec.similar_products(pid, 10), rec.recommend_from_products(basket, 10)
    rec.set_adapter(adapter_of(rec, random_delta(rec._index.dim, seed=6)))
    assert (rec.similar_products(pid, 10), rec.recommend_from_products(basket, 10)) == want
