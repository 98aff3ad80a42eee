"""icrec_cf_rank / icrec_cf_rank_all at the paths the real workload runs and tests/test_cf_gpu.py is too small for: pass
A's order loop past its first trip, membership words that fill the LDS at each tile width, 16-bit weights near 65,535,
the two refusals made after the build, history ids outside the catalog, 65,535 queries and a 512-list merge.  Exact
rows and exact integer scores against cf_cases.numpy_rank, which tests/test_cf.py holds equal to cf_reference.cf_rank."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import cf_cases

pytestmark = pytest.mark.gpu

A_THREADS = 1024   # orders per workgroup and trip of pass A (CF_A_THREADS)


def want_arrays(want, n_cand, k=None):
    """numpy_rank's (rows, scores) per query as the arrays the device calls fill: the best k, or every candidate."""
    n = n_cand if k is None else k
    rows = np.array([(r + [-1] * n)[:n] for r, _ in want], np.int64)
    scores = np.array([(s + [0] * n)[:n] for _, s in want], np.int64)
    return rows, scores


def assert_rows_equal(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} queries differ, first {bad[0]}: got {got[bad[0]][:12]}, want {want[bad[0]][:12]}"


def check_against_numpy(cf, baskets, distinct, n_cand, ks, pick=None):
    """The device's answers for histories [distinct[i] for i in pick] against numpy_rank of the distinct ones."""
    pick = np.arange(len(distinct)) if pick is None else np.asarray(pick)
    histories = [distinct[i] for i in pick]
    want = cf_cases.numpy_rank(baskets, distinct, n_cand)
    off, items = cf.hist(histories)
    Q = len(histories)
    rows, ws = cf.rank_all_buffers(Q)
    cf.rank_all_into(off, items, Q, rows, ws)
    assert_rows_equal(rows.cpu().numpy(), want_arrays(want, n_cand)[0][pick], "rank_all")
    del rows, ws
    for k in ks:
        rows, scores, ws = cf.rank_buffers(Q, k)
        cf.rank_into(off, items, Q, k, rows, scores, ws)
        want_rows, want_scores = want_arrays(want, n_cand, k)
        assert_rows_equal(rows.cpu().numpy(), want_rows[pick], f"rank rows k={k}")
        assert_rows_equal(scores.cpu().numpy().astype(np.int64), want_scores[pick], f"rank scores k={k}")


def native():
    from instacart_next_order_recommendation_amd import _native

    return _native


def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------ 1. pass A's order loop beyond its first trip
@pytest.mark.parametrize("tile", [4, 16])
def test_order_loop_runs_past_its_first_trip(tile, monkeypatch):
    """cf_keys cuts the orders into slices = min((2 n_cu + n_tiles - 1) / n_tiles, ceil(n_orders / 1024)), the division
    rounding down, and a workgroup walks them with a stride of slices * 1024.  With about n_cu tiles that is 2 slices
    (256 CUs: 767 / 256), and 9,001 orders take five trips; in production every order goes through the stride.  Tile 4:
    Q = 4 n_cu - 3, a ragged last tile of one query.  Tile 16: Q = 16 n_cu + 1, one tile more, its query alone in it."""
    if tile == 4:
        monkeypatch.setenv("ICREC_CF_TILE", "4")
    Q = tile * n_cu() - 3 if tile == 4 else tile * n_cu() + 1
    n_orders, n_items, n_cand = 9001, 100, 63
    n_tiles = (Q + tile - 1) // tile
    slices = min((2 * n_cu() + n_tiles - 1) // n_tiles, (n_orders + A_THREADS - 1) // A_THREADS)
    trips = -(-n_orders // (slices * A_THREADS))
    print(f"n_cu {n_cu()}, Q {Q}, {n_tiles} tiles, {slices} slices, {trips} trips")
    assert slices * A_THREADS < n_orders and trips >= 3
    baskets = cf_cases.synthetic_baskets(n_orders, n_items, seed=21, lengths=(0, 1, 2, 5, 9))
    distinct = cf_cases.synthetic_histories(67, n_items, seed=22)     # 67 is prime: no two tiles hold the same queries
    cf = cf_cases.DeviceCF(baskets, n_items, n_cand)
    try:
        assert cf.n.lib().icrec_cf_tile(cf.h) == tile
        check_against_numpy(cf, baskets, distinct, n_cand, ks=(20,), pick=np.arange(Q) % 67)
    finally:
        cf.close()


# ------------------------------------------------------------------ 2. membership words that fill the LDS
def edge_baskets(n_items):
    """40 baskets over ids at both ends of the catalog; one is empty, one holds an id twice."""
    pool = [0, 1, 2, 30, 31, 32, 33, n_items // 2, n_items // 2 + 1, n_items - 34, n_items - 33, n_items - 32, n_items - 3,
            n_items - 2, n_items - 1]
    rng = random.Random(n_items)
    baskets = [rng.sample(pool, 1 + o % 7) for o in range(36)]
    baskets += [[], [n_items - 1, 0, n_items - 1, 31], [n_items - 1, n_items - 2], [0, 31, n_items - 2, n_items - 1]]
    return baskets, pool


@pytest.mark.parametrize("n_items,tile", [(81_920, 16), (81_921, 8), (163_840, 8), (163_841, 4), (327_680, 4)])
def test_full_lds_at_each_tile(n_items, tile):
    """At 81,920 / 163,840 / 327,680 items pass A launches with all 163,840 bytes of LDS and the top item's bits are
    the highest of the last word; one item more narrows the tile.  Every item is a candidate, so the top items are
    ranked, and at the last size 524,288 keys per query are sorted and 512 chunk lists merged."""
    baskets, pool = edge_baskets(n_items)
    rng = random.Random(tile)
    histories = [sorted(rng.sample(pool, 1 + q % 5)) for q in range(tile + 1)]
    histories[0] = []
    histories[tile - 1] = sorted(set(histories[tile - 1]) | {n_items - 1, 31})   # bit T-1 of the top item: bit 31 when it is odd
    histories[tile] = [0, 31, n_items - 2]                                       # alone in the second tile
    cf = cf_cases.DeviceCF(baskets, n_items, n_items)
    try:
        assert cf.n.lib().icrec_cf_tile(cf.h) == tile
        check_against_numpy(cf, baskets, histories, n_items, ks=(1, 128))
    finally:
        cf.close()


# ------------------------------------------------------------------ 3. weights that need all 16 bits
def csr(baskets):
    lens = np.array([len(b) for b in baskets], np.int64)
    off = np.zeros(len(baskets) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, np.concatenate(baskets).astype(np.int32)


def test_weights_of_65534_in_either_half_word():
    """X = {0} + {2..65,535} (65,535 distinct items, the limit) three times, Y = {1} + {2..65,534}, H = {2..65,535}:
    w(X, H) = 65,534 and w(Y, H) = 65,533 need bit 15.  Closed form: candidate 0 scores 3 * 65,534 = 196,602, which a
    16-bit sum would not hold, candidate 1 scores 65,533; for the history {2} they score 3 and 1.  H first and H second
    put the large weight into the low and into the high half of the packed word, beside a weight of 1."""
    n_items = 65_600
    X = np.concatenate([[0], np.arange(2, 65_536)])
    Y = np.concatenate([[1], np.arange(2, 65_535)])
    assert len(X) == 65_535
    baskets = csr([X, np.concatenate([X, X[100:4100]]), X, Y])
    H = list(range(2, 65_536))
    cf = cf_cases.DeviceCF(baskets, n_items, 2)
    try:
        assert cf.n.lib().icrec_cf_nnz(cf.h) == 3 * 65_535 + 65_534
        for histories, closed in (([H, [2]], [[196_602, 65_533], [3, 1]]), ([[2], H], [[3, 1], [196_602, 65_533]])):
            want = cf_cases.numpy_rank(baskets, histories, 2)
            assert [sc for _, sc in want] == closed and [r for r, _ in want] == [[0, 1], [0, 1]]
            rows, scores = cf.rank(histories, 2)
            print(rows, scores)
            assert scores == closed and rows == [[0, 1], [0, 1]]
            assert cf.rank_all(histories) == [[0, 1], [0, 1]]
    finally:
        cf.close()


def test_basket_of_65536_distinct_items_is_refused():
    X = np.concatenate([[0], np.arange(2, 65_537)])
    assert len(X) == 65_536
    with pytest.raises(native().IcrecError, match=r"status -1\b.*a basket of 65536 distinct items \(limit 65535\)"):
        cf_cases.DeviceCF(csr([X, X[:5]]), 65_600, 2)
    assert b"a basket of 65536 distinct items" in native().lib().icrec_last_error()


# ------------------------------------------------------------------ 4. longest basket x most frequent item against 2^31 - 1
def bound_baskets(n_single):
    """One basket of the 65,535 items 0..65,534 and n_single orders that hold item 0 alone."""
    return csr([np.arange(65_535)] + [np.zeros(1, np.int64)] * n_single)


def test_largest_product_that_fits_31_bits_ranks():
    baskets = bound_baskets(32_766)          # item 0 in 32,767 orders: 65,535 * 32,767 = 2,147,385,345 < 2^31 - 1
    assert 65_535 * 32_767 == 2_147_385_345 < 2 ** 31 - 1
    histories = [list(range(3, 65_535))]
    cf = cf_cases.DeviceCF(baskets, 65_535, 4)
    try:
        want = cf_cases.numpy_rank(baskets, histories, 4)
        assert want == [([0, 1, 2], [65_532] * 3)]
        rows, scores = cf.rank(histories, 4)
        assert (rows, scores) == ([want[0][0] + [-1]], [want[0][1] + [0]])
        assert cf.rank_all(histories) == [want[0][0] + [-1]]
    finally:
        cf.close()


def test_product_of_2_pow_31_is_refused():
    assert 65_535 * 32_769 >= 2 ** 31 - 1    # item 0 in 32,769 orders
    with pytest.raises(native().IcrecError, match=r"status -1\b.*31 bits \(longest basket 65535 x most frequent item 32769\)"):
        cf_cases.DeviceCF(bound_baskets(32_768), 65_535, 4)


# ------------------------------------------------------------------ 5. history ids outside the catalog
@pytest.fixture(scope="module")
def small():
    baskets = cf_cases.synthetic_baskets(300, 137, seed=11)
    cf = cf_cases.DeviceCF(baskets, 137, 100)
    yield cf, baskets
    cf.close()


def test_history_ids_outside_the_catalog_count_for_nothing(small):
    cf, baskets = small
    dirty = [[-7, -1, 3, 50, 137, 2 ** 31 - 1], [-1], [137], [-2 ** 31, 0, 99, 136, 138], [3, 50]]
    clean = [[p for p in h if 0 <= p < 137] for h in dirty]
    assert clean[0] == [3, 50] and clean[1] == clean[2] == []
    for k in (20, 100):
        assert cf.rank(dirty, k) == cf.rank(clean, k)
    assert cf.rank_all(dirty) == cf.rank_all(clean)
    check_against_numpy(cf, baskets, dirty, 100, ks=(20, 100))


# ------------------------------------------------------------------ 6. as many queries as the ABI accepts
def test_65535_queries_and_one_more_refused():
    import torch

    n_items, n_cand, Q = 100, 63, 65_535
    baskets = cf_cases.synthetic_baskets(257, n_items, seed=31)
    distinct = cf_cases.synthetic_histories(64, n_items, seed=32)
    cf = cf_cases.DeviceCF(baskets, n_items, n_cand)
    try:
        check_against_numpy(cf, baskets, distinct, n_cand, ks=(20,), pick=np.arange(Q) % 64)
        n, lib = cf.n, cf.n.lib()
        assert lib.icrec_cf_rank_workspace_bytes(cf.h, Q + 1, 20) == 0 and lib.icrec_cf_rank_all_workspace_bytes(cf.h, Q + 1) == 0
        off, items = cf.hist(distinct)
        buf = torch.zeros(4096, dtype=torch.uint8, device=cf.device)    # refused before anything is read or written
        stream = n.stream_ptr(cf.device)
        assert lib.icrec_cf_rank(cf.h, n.ptr(off), n.ptr(items), Q + 1, 20, n.ptr(buf), n.ptr(buf), n.ptr(buf), buf.numel(), stream) == -1
        assert b"icrec_cf_rank: n_queries must be in [1, 65535] (got 65536)" in lib.icrec_last_error()
        assert lib.icrec_cf_rank_all(cf.h, n.ptr(off), n.ptr(items), Q + 1, n.ptr(buf), n.ptr(buf), buf.numel(), stream) == -1
        assert b"icrec_cf_rank_all: n_queries must be in [1, 65535] (got 65536)" in lib.icrec_last_error()
        torch.cuda.synchronize()
        assert int(buf.sum()) == 0
    finally:
        cf.close()


# ------------------------------------------------------------------ 7. the complete order under graph capture
def test_rank_all_under_graph_capture_equals_eager(small):
    import torch

    cf, baskets = small
    histories = cf_cases.synthetic_histories(17, 137, seed=5)
    off, items = cf.hist(histories)
    rows, ws = cf.rank_all_buffers(17)
    cf.rank_all_into(off, items, 17, rows, ws)
    torch.cuda.synchronize()
    eager = rows.clone()
    rows.fill_(-7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cf.rank_all_into(off, items, 17, rows, ws)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(rows, eager)
    want = cf_cases.numpy_rank(baskets, histories, 100)
    assert rows.cpu().tolist() == [r + [-1] * (100 - len(r)) for r, _ in want]
