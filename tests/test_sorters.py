"""The numpy side of the sorter tests (tests/test_sorters_gpu.py), without a GPU: pack_keys / unpack_keys against the
bit layout of csrc/common.h's make_key / store_key, merge_reference against the oracle's merge, stream_plan and
merge_form against hand-computed plans, block_merge_candidates on lists small enough to count by hand, and the
conditions on the crafted catalogs that make merge_block_kernel's ranking loop take a second and a third trip."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle
from tests import sorter_cases as sc
from tests.search_harness import (block_merge_candidates, merge_form, merge_reference, pack_keys, search_plan,
                                  stream_plan, tiled_plan, unpack_keys)

F32_EDGES = np.asarray([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.1754944e-38, -1.1754944e-38,
                        3.4028235e38, -3.4028235e38, np.inf, -np.inf, 1.0, -1.0, 0.3], np.float32)
ROW_EDGES = np.asarray([0, 1, 2 ** 31, 2 ** 32 - 2], np.int64)


def test_keys_round_trip_bit_exactly():
    scores, rows = np.meshgrid(F32_EDGES, ROW_EDGES, indexing="ij")
    keys = pack_keys(scores, rows)
    assert keys.dtype == np.uint64 and keys.shape == scores.shape and (keys != 0).all()
    idx, back = unpack_keys(keys)
    assert idx.dtype == np.int64 and back.dtype == np.float32
    np.testing.assert_array_equal(idx, rows)
    np.testing.assert_array_equal(back.view(np.uint32), scores.astype(np.float32).view(np.uint32))   # the BITS: -0 stays -0
    # the layout, spelled out once: +1.0 = 0x3F800000 gets its sign bit set, -1.0 = 0xBF800000 is inverted
    assert int(pack_keys(np.float32(1.0), 5)) == (0xBF800000 << 32) | (0xFFFFFFFF - 5)
    assert int(pack_keys(np.float32(-1.0), 2 ** 32 - 2)) == (0x407FFFFF << 32) | 1
    pad_idx, pad_score = unpack_keys(np.zeros(3, np.uint64))
    assert pad_idx.tolist() == [-1] * 3 and pad_score.view(np.uint32).tolist() == [0] * 3


def test_key_order_is_score_descending_then_row_ascending():
    rng = np.random.default_rng(1)
    scores = np.concatenate([rng.standard_normal(3000, dtype=np.float32), rng.choice(F32_EDGES, 1000)])
    scores = rng.permutation(np.where(scores == 0, np.float32(0.0), scores))    # no -0 here: see below
    scores[::5] = scores[3]                                                     # 800 equal scores: the row decides
    pool = np.unique(rng.integers(0, 2 ** 32 - 1, size=2 * scores.size))          # distinct rows
    pool = rng.permutation(pool[~np.isin(pool, ROW_EDGES)])[:scores.size - ROW_EDGES.size]
    rows = rng.permutation(np.concatenate([pool, ROW_EDGES]))
    by_key = np.argsort(pack_keys(scores, rows))[::-1]
    np.testing.assert_array_equal(by_key, np.lexsort((rows, -scores.astype(np.float64))))
    # -0.0 is BELOW +0.0 as a key, whatever the rows (the search kernels add +0 before they pack; pack_keys does not)
    assert pack_keys(np.float32(-0.0), 0) < pack_keys(np.float32(0.0), 2 ** 32 - 2)
    assert pack_keys(np.float32(-1e-45), 0) < pack_keys(np.float32(-0.0), 2 ** 32 - 2)


@pytest.mark.parametrize("n_lists,Q,k", [(1, 2, 5), (7, 3, 20), (300, 2, 128)])
def test_merge_reference_is_the_oracles_merge(n_lists, Q, k):
    """Full lists (no pads: there both are defined), with ties across lists."""
    rng = np.random.default_rng(n_lists)
    scores = rng.choice(rng.standard_normal(50, dtype=np.float32), size=(n_lists, Q, k))
    scores = -np.sort(-scores, axis=2)
    rows = np.broadcast_to((np.arange(n_lists)[:, None, None] * 1000 + np.arange(k)[None, None, :]), scores.shape)
    got = merge_reference(pack_keys(scores, rows), k)
    want = oracle.merge(rows, scores)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_merge_reference_pads():
    keys = np.zeros((3, 1, 4), np.uint64)
    keys[2, 0, :2] = np.sort(pack_keys(np.asarray([0.5, -2.0], np.float32), np.asarray([9, 4])))[::-1]
    idx, score = merge_reference(keys, 4)
    assert idx.tolist() == [[9, 4, -1, -1]] and score.tolist() == [[0.5, -2.0, 0.0, 0.0]]


def test_stream_plan_and_merge_form_pins():
    """At 256 CUs, worked out by hand: 3 * 256 = 768 chunks wanted, at most 1,024, at most one per tile of 256 rows."""
    assert stream_plan(65_536, 1, 256) == ("stream", 256, 1, 1, 1, 256)
    assert stream_plan(65_537, 2, 256) == ("stream", 256, 2, 1, 1, 257)
    assert stream_plan(300, 1, 256) == ("stream", 256, 1, 1, 1, 2)
    assert stream_plan(2_000_000, 8, 256) == ("stream", 256, 8, 1, 11, 711)     # 7,813 tiles >= 1,536; ceil(7813 / 768) = 11
    assert stream_plan(2_000_000, 9, 256) is None
    assert stream_plan(49_688, 3, 256) is None and stream_plan(49_688, 2, 256)[5] == 195
    assert stream_plan(2_000_000, 4, 400)[4:] == (8, 977)                       # 1,200 wanted, capped at 1,024
    assert search_plan(49_688, 4, 20, 256) == tiled_plan(49_688, 4, 20, 256) == ("small", 256, 32, 1, 1, 195)
    assert merge_form(256, 1, 16) == "block" and merge_form(256, 1, 17) == "wave4" and merge_form(257, 1, 8) == "wave16"
    assert merge_form(195, 4, 21) == "block" and merge_form(195, 4, 22) == "wave4" and merge_form(195, 5, 20) == "wave4"
    assert merge_form(32, 2, 128) == "block" and merge_form(1024, 1, 1) == "wave16"
    assert merge_form(64, 1, 20, block=False) == "wave4"


def test_block_merge_candidates_by_hand():
    """Four lists of 2 rows, k = 2: heads 9, 7, 5, 1 -> h = 7; lists 0 and 1 hold 9, 8, 7 (6 < 7 ends list 1) -> C = 3.
    With row 0 inadmissible the heads are 8, 7, 5, 1, h = 7 still, C = 2.  k = 5 > the 4 lists: h = 0, all 8 keys."""
    s = np.asarray([9, 8, 7, 6, 5, 4, 1, 0.5], np.float32)
    assert block_merge_candidates(s, 2, 2, 1) == 3
    cut = s.copy()
    cut[0] = -np.inf
    assert block_merge_candidates(cut, 2, 2, 1) == 2
    assert block_merge_candidates(s, 5, 2, 1) == 8 and block_merge_candidates(cut, 5, 1, 2) == 7
    assert block_merge_candidates(s, 1, 2, 2) == 1          # two lists of 4 rows, k = 1: the best key alone
    # equal scores: the earlier row is the larger key; chunk heads are rows 0 and 2, h = key of row 2, C = 3 (rows 0, 1, 2)
    assert block_merge_candidates(np.ones(4, np.float32), 2, 2, 1) == 3


@pytest.mark.parametrize("name", list(sc.SEARCH_CASES))
def test_crafted_catalogs_meet_their_conditions(name):
    """The cases of test_sorters_gpu at 256 CUs: the plan gives the list count and the merge form each case names, and
    the number of keys merge_block_kernel ranks (block_merge_candidates, on float32 numpy scores of the admissible
    rows) is where the case needs it - C >= 513 for the many-candidates cases (three trips of the ranking loop), C > 256
    at 195 lists x k = 20 and 21 of the ascending catalog, C <= 256 for its random-order twin."""
    _, n, dim, storage, Qs, forms, kernel, n_lists, conditions, none_query = sc.SEARCH_CASES[name]
    P, q = sc.search_case_inputs(name)
    assert P.shape == (n, dim) and q.shape == (sc.MAX_Q, dim) and n <= 66_000 and dim in (32, 64)
    rows = oracle.round_bf16(oracle.normalize_rows(P)) if storage == "bf16" else P
    S = sc.numpy_scores(rows, q)
    excl = sc.search_case_exclusions(name, S)
    assert excl[none_query] == [] and all(len(e) >= 10 for i, e in enumerate(excl) if i != none_query)
    for i, e in enumerate(excl):
        S[i, e] = -np.inf
    for Q in Qs:
        for k, form in forms.items():
            plan = search_plan(n, Q, k, 256)
            assert (plan[0], plan[5]) == (kernel, n_lists) and merge_form(n_lists, Q, k) == form
            C = [block_merge_candidates(S[i], k, plan[1], plan[4]) for i in range(Q)]
            print(f"{name} Q {Q} k {k}: plan {plan}, {form}, C {C}")
            assert all(sc.holds(c, conditions.get(k)) for c in C), (C, conditions.get(k))
    if name == "edge-stream-257":
        np.testing.assert_array_equal(P[-1], q[0])
        assert S[0].argmax() == n - 1


@pytest.mark.parametrize("pattern", sc.MERGE_PATTERNS)
def test_merge_case_keys_are_well_formed(pattern):
    """Sorted descending per (list, query), unique per query, pads only at the tail - and what each pattern promises."""
    for n_lists, Q, k in [(1, 5, 128), (65, 4, 128), (257, 5, 20), (64, 4, 1)]:
        keys = sc.merge_case_keys(pattern, n_lists, Q, k, seed=n_lists)
        assert keys.shape == (n_lists, Q, k) and keys.dtype == np.uint64
        before, after = keys[:, :, :-1], keys[:, :, 1:]
        assert ((after < before) | ((after == 0) & (before == 0))).all()
        real = keys != 0
        for i in range(Q):
            mine = keys[:, i][real[:, i]]
            assert np.unique(mine).size == mine.size
        per_query = real.sum(axis=(0, 2))
        if pattern == "short":
            assert (per_query < k).all()
        if pattern == "last-list":
            assert not real[:-1].any() and real[-1].all()
        if pattern == "pad-lists":
            assert not real[::3].any() and real[1::3, :, 0].all()
        if pattern == "edge-values":
            idx, score = unpack_keys(keys)
            assert idx.min() >= 4_000_000_000 and np.isinf(score).any() and (score.view(np.uint32) == 0x80000000).any()
        if pattern == "ties":
            _, score = merge_reference(keys, k)
            assert k == 1 or (np.diff(score, axis=1) == 0).any()
