"""Rank fusion end to end on the GPU: HybridBaseline on tests/golden/cf_small against tests/fuse_reference.py's fusion
of the two baselines' own lists, and Recommender(cf=...).recommend(..., history=) on a synthetic 2-layer model and a
catalog of 300 with seeded baskets against the reference's fusion of DeviceIndex.search and the CF ranking
(tests/cf_cases.numpy_rank) - with exclusions, in a batch, without a history, with an empty one, and after
add_products / update_products.  Both tests assert, on the reference's positions, that their data exercises the merge."""
from __future__ import annotations

import random

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.baselines import ContentBasedBaseline, HybridBaseline, ItemItemCFBaseline
from instacart_next_order_recommendation_amd.ir_metrics import compute_ir_metrics_rows, load_eval_data, relevant_csr
from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir
from instacart_next_order_recommendation_amd.recommender import Recommender
from instacart_next_order_recommendation_amd.search import rrf_weights
from tests import fuse_reference as ref
from tests.cf_cases import FIXTURE, numpy_rank
from tests.recommender_harness import (as_results, assert_batch_equals_single_calls, synthetic_world, torch_cuda,  # noqa: F401
                                       two_layer_shape)

pytestmark = pytest.mark.gpu


def assert_merge_is_exercised(pos, idx, n_queries):
    """On the reference's positions of the returned ids: some id is live in A only, some in B only, some in both, and
    at most a quarter of the queries have no live B entry at all."""
    pos, live = np.asarray(pos), np.asarray(idx) >= 0
    in_a, in_b = (pos[:, :, 0] >= 0) & live, (pos[:, :, 1] >= 0) & live
    assert (in_a & ~in_b).any() and (in_b & ~in_a).any() and (in_a & in_b).any()
    dead_b = int((~in_b.any(axis=1)).sum())
    assert dead_b * 4 <= n_queries, (dead_b, n_queries)


# ---------------------------------------------------------------- HybridBaseline
def test_hybrid_baseline_on_the_cf_fixture(tmp_path, torch_cuda):
    queries, corpus, relevant = load_eval_data(FIXTURE / "processed")
    cb = ContentBasedBaseline(queries, corpus, write_synthetic_model_dir(tmp_path / "m", seed=6, shape=two_layer_shape()))
    cf = ItemItemCFBaseline(FIXTURE / "data", FIXTURE / "processed")
    n = len(cb.product_ids)
    assert n == 60 and len(queries) >= 30
    row_of = {p: j for j, p in enumerate(cb.product_ids)}
    for depth, cf_weight, rrf_c in ((10, 1.0, 60.0), (60, 0.5, 10.0)):
        hy = HybridBaseline(cb, cf, depth=depth, cf_weight=cf_weight, rrf_c=rrf_c)
        a_rows, qids = cb.rank_rows(depth)
        b_rows, b_sc = cf.rank_rows_scores(qids, depth)
        want = ref.fuse_select(a_rows.cpu().numpy(), b_rows.cpu().numpy(), rrf_weights(depth, rrf_c), rrf_weights(depth, rrf_c, cf_weight),
                               depth, n, b_gate=b_sc.cpu().numpy())
        if depth == 10:  # (at depth 60 list A is the whole corpus: nothing is in B only)
            assert_merge_is_exercised(want[2], want[0], len(qids))
        got, got_q = hy.rank_rows()
        assert got_q == qids == list(queries)
        np.testing.assert_array_equal(got.cpu().numpy(), want[0])
        two_passes, _ = hy.rank_rows(depth, queries_per_pass=16)  # one pass ragged
        np.testing.assert_array_equal(two_passes.cpu().numpy(), want[0])
        ranked = hy.rank_all(depth)
        assert ranked == {q: [cb.product_ids[j] for j in want[0][i] if j >= 0] for i, q in enumerate(qids)}
        off, rel = relevant_csr(qids, relevant, row_of, cb.device)
        assert hy.evaluate(relevant) == compute_ir_metrics_rows(torch_cuda.from_numpy(want[0]).to(cb.device), off, rel)
    assert hy.evaluate(relevant, depth=10) != cb.evaluate(relevant, depth=10)
    with pytest.raises(ValueError, match="depth must be in"):
        HybridBaseline(cb, cf, depth=129)
    other = ItemItemCFBaseline.from_arrays([], {}, cb.product_ids[::-1])
    with pytest.raises(ValueError, match="same product ids in the same order"):
        HybridBaseline(cb, other)
    # ad-hoc histories rank like the stored ones, and the existing query-id form is unchanged
    hist = [sorted(cf.eval_order_to_history[q]) + ["no-such-product"] for q in qids]
    rows_csr, sc_csr = cf.rank_rows_scores(cf.history_csr_from(hist), 10)
    rows_ids, sc_ids = cf.rank_rows_scores(qids, 10)
    assert torch_cuda.equal(rows_csr, rows_ids) and torch_cuda.equal(sc_csr, sc_ids)


# ---------------------------------------------------------------- Recommender(cf=)
N_PRODUCTS, N_BASKETS = 300, 400
QUERIES = syn.synthetic_user_contexts(7, seed=9) + ["[+1d w0h1] Milk."]


def seeded_baskets(ids):
    """400 baskets of 3 .. 12 products of the catalog, skewed so that neighbours in id order are bought together."""
    rng = random.Random(5)
    out = []
    for _ in range(N_BASKETS):
        centre = rng.randrange(len(ids))
        out.append([ids[(centre + rng.randrange(-20, 21)) % len(ids)] for _ in range(rng.randrange(3, 13))])
    return out


def seeded_histories(ids):
    """One history per query of QUERIES: 2 .. 9 catalog products; one query has none, one names an unknown product too."""
    rng = random.Random(6)
    out = [rng.sample(ids, rng.randrange(2, 10)) for _ in QUERIES]
    out[3] = []
    out[5] = out[5] + ["no-such-product"]
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory, torch_cuda):
    model_dir, corpus_path, corpus = synthetic_world(tmp_path_factory.mktemp("hybrid_rec"), N_PRODUCTS)
    ids = list(corpus)
    baskets = seeded_baskets(ids)
    cf = ItemItemCFBaseline.from_arrays(baskets, {}, ids)
    rec = Recommender(model_dir, corpus_path, use_index=False, cf=cf)
    item_baskets = [[rec._pid_to_row[p] for p in b] for b in baskets]
    return rec, item_baskets, seeded_histories(ids)


def expected(rec, item_baskets, queries, histories, top_k, exclude=None, w=None, cf_weight=1.0, rrf_c=60.0, n_cf=N_PRODUCTS):
    """The reference's fusion of DeviceIndex.search on the recommender's own query embeddings and numpy_rank over the
    baskets -> ([per query [(product id, fused score)]], the reference's positions, its indices)."""
    n = len(rec.product_ids)
    w = w or min(128, 4 * top_k, n)
    ex = None if exclude is None else [[rec._pid_to_row[p] for p in (e or ()) if p in rec._pid_to_row] for e in exclude]
    a = rec._index.search(rec.model.encode_to_device(list(queries)), w, ex)[0].cpu().numpy()
    items = [[rec._pid_to_row[p] for p in h if p in rec._pid_to_row and rec._pid_to_row[p] < n_cf] for h in histories]
    ranked = numpy_rank(item_baskets, items, n_cf, w)
    b, b_sc = np.asarray([r for r, _ in ranked], np.int64), np.asarray([s for _, s in ranked], np.int32)
    idx, sc, pos = ref.fuse_select(a, b, rrf_weights(w, rrf_c), rrf_weights(w, rrf_c, cf_weight), top_k, n, b_gate=b_sc, exclude=ex)
    return [as_results(rec, idx[i], sc[i]) for i in range(len(queries))], pos, idx


def test_recommend_with_history_equals_the_reference(world):
    rec, baskets, histories = world
    want, pos, idx = expected(rec, baskets, QUERIES, histories, 10)
    assert_merge_is_exercised(pos, idx, len(QUERIES))
    for i, q in enumerate(QUERIES):
        got = rec.recommend(q, 10, history=histories[i])
        assert got == want[i] and len(got) == 10, i
    # with exclusions: the best fused results and the history itself are dropped from both lists
    drop = [{p for p, _ in want[i][:3]} | set(histories[i]) for i in range(len(QUERIES))]
    want_ex, _, _ = expected(rec, baskets, QUERIES, histories, 10, exclude=drop)
    for i, q in enumerate(QUERIES):
        got = rec.recommend(q, 10, exclude_product_ids=drop[i], history=histories[i])
        assert got == want_ex[i] and not drop[i] & {p for p, _ in got}, i
    # the width, the weight and the constant
    want_w, _, _ = expected(rec, baskets, QUERIES[:3], histories[:3], 5, w=77, cf_weight=0.25, rrf_c=3.0)
    for i in range(3):
        assert rec.recommend(QUERIES[i], 5, history=histories[i], candidates=77, cf_weight=0.25, rrf_c=3.0) == want_w[i]
    assert want_w != expected(rec, baskets, QUERIES[:3], histories[:3], 5, w=77)[0]


def test_batch_rows_equal_the_single_requests(world):
    rec, baskets, histories = world
    excl = [None, {"1", "2", "3"}, None, {"10"}, None, None, set(histories[6]), None]
    batch = assert_batch_equals_single_calls(rec, QUERIES, 10, excl, history=histories)
    assert batch == expected(rec, baskets, QUERIES, histories, 10, exclude=excl)[0]
    # in a batch that fuses, a None entry counts as []
    some, same = [histories[0], None, histories[2]], [histories[0], [], histories[2]]
    assert rec.recommend_batch(QUERIES[:3], 10, history=some) == rec.recommend_batch(QUERIES[:3], 10, history=same)
    # the CF passes are cut by the workspace bound: one query per pass gives the same rows
    rec.CF_PASS_BYTES = 1
    try:
        assert rec.recommend_batch(QUERIES, 10, excl, history=histories) == batch
    finally:
        del rec.CF_PASS_BYTES


def test_no_history_is_the_plain_request_and_an_empty_one_the_content_order(world):
    rec, baskets, histories = world
    for q in QUERIES[:3]:
        plain = rec.recommend(q, 10)
        assert rec.recommend(q, 10, history=None) == plain  # the same score bits: floats compare exactly
        assert rec.recommend(q, 10, history=None, cf_weight=5.0, rrf_c=1.0) == plain
        for empty in ([], ["no-such-product"]):
            fused = rec.recommend(q, 10, history=empty)
            assert [p for p, _ in fused] == [p for p, _ in plain]
            assert [s for _, s in fused] == [float(t) for t in rrf_weights(10)]
    assert rec.recommend_batch(QUERIES[:3], 10, history=[None] * 3) == rec.recommend_batch(QUERIES[:3], 10)
    assert rec.recommend_batch(QUERIES[:3], 10, history=None) == rec.recommend_batch(QUERIES[:3], 10)


def test_catalog_edits_with_cf(world):
    """Last: it edits the module's recommender.  remove_products is refused with nothing changed; after add_products
    and update_products the fused results match the reference built from the edited catalog (the CF candidates stay
    the first 300 rows; a new row can come from the content list only)."""
    rec, baskets, histories = world
    before = (list(rec.product_ids), list(rec.product_texts), rec.product_embeddings.copy())
    plain = rec.recommend(QUERIES[0], 10, history=histories[0])
    with pytest.raises(ValueError, match="remove_products renumbers catalog rows"):
        rec.remove_products([rec.product_ids[4]])
    assert (rec.product_ids, rec.product_texts) == before[:2] and np.array_equal(rec.product_embeddings, before[2])
    assert rec.recommend(QUERIES[0], 10, history=histories[0]) == plain
    extra = syn.synthetic_catalog(N_PRODUCTS + 40)
    rec.add_products({p: t for p, t in extra.items() if p not in rec._pid_to_row})
    changed = [p for p, _ in plain[:2]] + [rec.product_ids[7]]
    rec.update_products({p: extra[str(N_PRODUCTS + 1 + j)] for j, p in enumerate(changed)})
    assert len(rec.product_ids) == N_PRODUCTS + 40
    want = expected(rec, baskets, QUERIES, histories, 10)[0]
    assert [rec.recommend(q, 10, history=histories[i]) for i, q in enumerate(QUERIES)] == want
    want, pos, idx = expected(rec, baskets, QUERIES, histories, 30)  # 120 wide: deep enough to meet the new rows
    assert rec.recommend_batch(QUERIES, 30, history=histories) == want
    assert (idx >= N_PRODUCTS).any()  # an added product is returned: from the content list alone
    assert (pos[idx >= N_PRODUCTS][:, 1] == -1).all()
