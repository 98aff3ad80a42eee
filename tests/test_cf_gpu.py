"""icrec_cf_rank / icrec_cf_rank_all against tests/cf_reference.py: exact rows and exact integer scores, at shapes
chosen to break the tiling (a tile is 16, 8 or 4 queries; a wavefront serves 16 column entries of a candidate at a time;
the top-k sorts chunks of 1,024 keys and merges them; the full sort leaves LDS above 8,192 keys)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import cf_cases, cf_reference

pytestmark = pytest.mark.gpu

KS = (1, 20, 100, 128)


def check_against_reference(cf, baskets, histories, n_cand, ks=KS):
    want_all = cf_reference.cf_rank(baskets, histories, n_cand)
    got_all = cf.rank_all(histories)
    for q, (rows, _) in enumerate(want_all):
        assert got_all[q] == rows + [-1] * (n_cand - len(rows)), f"rank_all, query {q}"
    for k in ks:
        got_rows, got_scores = cf.rank(histories, k)
        for q, (rows, sc) in enumerate(want_all):
            pad = max(0, k - len(rows))
            assert got_rows[q] == rows[:k] + [-1] * pad, f"rank k={k}, query {q}"
            assert got_scores[q] == sc[:k] + [0] * pad, f"rank scores k={k}, query {q}"


# (n_candidates, extra non-corpus items, n_orders, Q)
SHAPES = [(1, 0, 1, 1), (1, 37, 257, 17), (63, 0, 257, 33), (63, 37, 5000, 17), (1000, 37, 257, 33), (1000, 0, 5000, 17),
          (1000, 37, 1, 1),
          (9000, 37, 257, 5),   # 16,384 keys per query: 16 top-k chunks to merge, bitonic stages in global memory
          # icrec_cf_create scans the basket lengths (n_orders of them) and the column lengths (n_items) in chunks of
          # 1,024: the shapes above give each array a length below 64 and one above 2,048 that is no multiple of 1,024
          # (orders 1 and 5,000, items 1 and 9,037); here both are one full chunk exactly
          (1000, 24, 1024, 5)]


@pytest.mark.parametrize("n_cand,extra,n_orders,Q", SHAPES)
def test_rank_matches_reference(n_cand, extra, n_orders, Q):
    n_items = n_cand + extra
    baskets = cf_cases.synthetic_baskets(n_orders, n_items, seed=n_cand + n_orders)
    histories = cf_cases.synthetic_histories(Q, n_items, seed=Q)
    cf = cf_cases.DeviceCF(baskets, n_items, n_cand)
    try:
        lib = cf.n.lib()
        assert lib.icrec_cf_orders(cf.h) == n_orders and lib.icrec_cf_items(cf.h) == n_items
        assert lib.icrec_cf_candidates(cf.h) == n_cand and lib.icrec_cf_nnz(cf.h) == sum(len(set(b)) for b in baskets)
        check_against_reference(cf, baskets, histories, n_cand)
    finally:
        cf.close()


@pytest.mark.parametrize("tile", [8, 4])
def test_narrow_tiles_rank_the_same(tile, monkeypatch):
    monkeypatch.setenv("ICREC_CF_TILE", str(tile))
    baskets = cf_cases.synthetic_baskets(257, 100, seed=3)
    histories = cf_cases.synthetic_histories(33, 100, seed=4)
    cf = cf_cases.DeviceCF(baskets, 100, 63)
    try:
        assert cf.n.lib().icrec_cf_tile(cf.h) == tile
        check_against_reference(cf, baskets, histories, 63, ks=(20,))
    finally:
        cf.close()


def test_large_catalog_falls_back_to_a_narrower_tile():
    """100,000 items do not fit 16 membership bits each in LDS: the tile narrows to 8 on its own."""
    n_items = 100_000
    baskets = [[0, 5, 99_999, 70_000], [5, 99_999], [70_000, 62, 1], [99_999, 62, 62, 0], []]
    histories = [[99_999], [5, 70_000], [], [1, 2, 3], [0, 62, 99_999]] * 2
    cf = cf_cases.DeviceCF(baskets, n_items, 63)
    try:
        assert cf.n.lib().icrec_cf_tile(cf.h) == 8
        check_against_reference(cf, baskets, histories, 63, ks=(20,))
    finally:
        cf.close()


@pytest.fixture(scope="module")
def small():
    baskets = cf_cases.synthetic_baskets(300, 137, seed=11)
    cf = cf_cases.DeviceCF(baskets, 137, 100)
    yield cf, baskets
    cf.close()


def test_empty_history_gives_corpus_order_with_zero_scores(small):
    cf, _ = small
    rows, scores = cf.rank([[]], 20)
    assert rows == [list(range(20))] and scores == [[0] * 20]


def test_history_that_cannot_cooccur(small):
    cf, baskets = small
    unbought = [p for p in range(137) if not any(p in b for b in baskets)]
    histories = [list(range(100, 137)), unbought[:3] if unbought else [], [100]]
    check_against_reference(cf, baskets, histories, 100, ks=(20,))


def test_history_covering_all_but_five_candidates_pads(small):
    cf, baskets = small
    keep = {3, 17, 42, 64, 99}
    hist = [p for p in range(100) if p not in keep]
    rows, scores = cf.rank([hist], 20)
    assert sorted(rows[0][:5]) == sorted(keep) and rows[0][5:] == [-1] * 15 and scores[0][5:] == [0] * 15
    check_against_reference(cf, baskets, [hist], 100, ks=(20,))


def test_equal_scores_rank_by_row():
    baskets = [list(range(50)) for _ in range(7)] + [[50, 51]]      # candidates 0..49 all score the same
    cf = cf_cases.DeviceCF(baskets, 60, 55)
    try:
        rows, scores = cf.rank([[10, 52]], 55)
        assert rows[0] == [p for p in range(50) if p != 10] + [50, 51, 53, 54] + [-1, -1] and scores[0][:49] == [7] * 49
        check_against_reference(cf, baskets, [[10, 52], [50], []], 55, ks=(1, 55))
    finally:
        cf.close()


def test_scores_above_2_pow_24_stay_exact():
    """60,000 baskets hold 300 history items and candidate a = row 1; candidate b = row 0 is in 59,999 of them and in one
    more basket with only 299 of the history items.  Closed form: a scores 60,000 * 300 = 18,000,000, b scores
    59,999 * 300 + 299 = 17,999,999.  float32 rounds both to 18,000,000 and would put b (the lower row) first."""
    a, b, H = 1, 0, 300
    hist = np.arange(2, 2 + H, dtype=np.int32)
    full = np.concatenate([[a, b], hist]).astype(np.int32)
    n_full = 59_999
    items = np.concatenate([np.tile(full, n_full), np.concatenate([[a], hist]).astype(np.int32),
                            np.concatenate([[b], hist[:H - 1]]).astype(np.int32)])
    lens = np.array([len(full)] * n_full + [1 + H, H], np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    cf = cf_cases.DeviceCF((off, items), 2 + H, 2)
    try:
        rows, scores = cf.rank([hist.tolist()], 2)
        print(rows, scores)
        assert scores[0] == [18_000_000, 17_999_999] and rows[0] == [a, b]
        assert cf.rank_all([hist.tolist()]) == [[a, b]]
    finally:
        cf.close()


def test_rank_under_graph_capture_equals_eager(small):
    import torch

    cf, baskets = small
    histories = cf_cases.synthetic_histories(17, 137, seed=5)
    off, items = cf.hist(histories)
    rows, scores, ws = cf.rank_buffers(17, 20)
    cf.rank_into(off, items, 17, 20, rows, scores, ws)
    torch.cuda.synchronize()
    eager = (rows.clone(), scores.clone())
    rows.fill_(-7)
    scores.fill_(-7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cf.rank_into(off, items, 17, 20, rows, scores, ws)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(rows, eager[0]) and torch.equal(scores, eager[1])
    want = cf_reference.cf_rank(baskets, histories, 100, 20)
    assert rows.cpu().tolist() == [w[0] for w in want]


def test_fixture_end_to_end_equals_upstream():
    from instacart_next_order_recommendation_amd.baselines import ItemItemCFBaseline

    rec = cf_cases.load_fixture()
    cf = ItemItemCFBaseline(cf_cases.FIXTURE / "data", cf_cases.FIXTURE / "processed")
    try:
        qids = list(rec["rankings"].keys())
        assert cf.rank_all(eval_query_ids=qids, queries_per_pass=7) == rec["rankings"]
        top = cf.rank_all(eval_query_ids=qids, depth=20)
        assert top == {q: r[:20] for q, r in rec["rankings"].items()}
        assert set(cf.rank_all()) == set(qids)
        rows, order = cf.rank_rows(depth=20, eval_query_ids=qids)
        assert order == qids and tuple(rows.shape) == (len(qids), 20)
    finally:
        cf.close()
