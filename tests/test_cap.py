"""Caps per aisle and department without a device: the numpy reference (tests/cap_reference.py) against a brute-force
walk, the round scheme against the one-pass greedy walk of the complete ranking, the recommender's argument checks,
and icrec_cap_select's refusals, which come before any HIP call."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import cli
from instacart_next_order_recommendation_amd.recommender import ann_plan, cap_plan
from instacart_next_order_recommendation_amd.search import cap_pairs, facet_masks
from tests import cap_reference as ref
from tests.search_harness import admitted_matrix

ICREC_EINVAL = -1


@pytest.fixture(scope="module")
def native():
    from instacart_next_order_recommendation_amd import _native

    if not _native.LIB_PATH.exists():
        _native.build()
    return _native


# ---------------------------------------------------------------- the reference against a brute-force walk
def test_lazy_ranking_is_the_full_ranking():
    """cap_reference._ranked, whose long-list branch ranks the head first, against full_ranking of the same rows: ties
    across the bar, -0 beside +0, all rows equal, and a head longer than, equal to and shorter than the list."""
    from tests.search_harness import full_ranking

    rng = np.random.default_rng(5)
    for n, head, values in ((300, 8, 7), (300, 8, 1), (33, 8, 3), (32, 8, 5), (500, 16, 40), (64, 1, 2)):
        s = rng.integers(-values, values + 1, n).astype(np.float32) * np.float32(0.25)
        s[rng.random(n) < 0.2] *= np.float32(-0.0) if values > 1 else np.float32(1)        # some zeros of either sign
        rows = np.flatnonzero(rng.random(n) < 0.8)
        want = rows[full_ranking(s[rows])]
        np.testing.assert_array_equal(np.fromiter(ref._ranked(s, rows, head=head), np.int64), want)
        np.testing.assert_array_equal(np.fromiter(ref._ranked(s, rows), np.int64), want)


def brute_force(F, cand, caps, top_k):
    """One query without priors, pads or duplicates, written the other way round: candidate j is kept iff, for every
    capped facet, fewer than cap of the KEPT candidates before it share its value - decided from the kept set, with
    no running tables."""
    kept: list[int] = []
    for j, c in enumerate(cand):
        if len(kept) == top_k:
            break
        if all(cap <= 0 or sum(F[cand[i], f] == F[c, f] for i in kept) < cap for f, cap in enumerate(caps[:F.shape[1]])):
            kept.append(j)
    return kept


def test_reference_equals_brute_force():
    rng = np.random.default_rng(1)
    for trial in range(60):
        n_facets = 1 + trial % 2
        F = rng.integers(0, [6, 3][:n_facets], (200, n_facets)).astype(np.uint8)
        k = int(rng.integers(1, 129))
        cand = rng.choice(200, k, replace=False).astype(np.int64)
        score = rng.standard_normal(k).astype(np.float32)
        caps = [int(rng.choice([-5, 0, 1, 2, 7])), int(rng.choice([0, 1, 3, 2**31 - 1]))]
        top_k = int(rng.integers(1, 129))
        idx, sc, state, nxt = ref.cap_select(F, cand[None], score[None], caps, top_k)
        kept = brute_force(F, cand, caps, top_k)
        assert list(idx[0, :len(kept)]) == list(cand[kept]) and (idx[0, len(kept):] == -1).all()
        np.testing.assert_array_equal(sc[0, :len(kept)].view(np.uint32), score[kept].view(np.uint32))
        assert (sc[0, len(kept):] == 0).all()
        assert list(state[0]) == [len(kept), int(len(kept) == top_k)]
        # the next masks: exactly the values that are full are closed
        for f in range(n_facets):
            full = {int(v) for v in range(256) if caps[f] > 0 and sum(F[cand[kept], f] == v) >= caps[f]}
            assert set(np.flatnonzero(~admitted_matrix(np.arange(256, dtype=np.uint8)[:, None], nxt[:, f:f + 1])[0])) == full


def test_priors_pads_duplicates_and_shards():
    F = np.array([[0, 0], [0, 1], [1, 0], [1, 1], [0, 0], [2, 1]], np.uint8)
    off = 1000
    cand = np.array([[off + 4, -1, off + 1, off + 4, off + 99, 3, off + 2, off + 5]], np.int64)
    score = np.arange(8, dtype=np.float32)[None] + 1
    # no caps: every valid candidate once, the pad makes it done
    idx, sc, state, nxt = ref.cap_select(F, cand, score, [0, -3], 6, row_offset=off)
    assert list(idx[0]) == [off + 4, off + 1, off + 2, off + 5, -1, -1] and list(sc[0]) == [1, 3, 7, 8, 0, 0]
    assert list(state[0]) == [4, 1] and (nxt == 0xFFFFFFFF).all()
    # one per aisle, with row 0 (aisle 0) and an out-of-shard row as priors; n_prior is clamped to top_k
    prior_idx = np.array([[off + 0, 7, -1, -1]], np.int64)
    prior_sc = np.array([[9.0, 8.0, 0, 0]], np.float32)
    idx, sc, state, nxt = ref.cap_select(F, cand, score, [1, 0], 4, [2], prior_idx, prior_sc, row_offset=off)
    assert list(idx[0]) == [off + 0, 7, off + 2, off + 5] and list(sc[0]) == [9, 8, 7, 8] and list(state[0]) == [4, 1]
    assert nxt[0, 0, 0] == 0xFFFFFFFF & ~0b111 and (nxt[0, 1] == 0xFFFFFFFF).all()
    idx, _, state, _ = ref.cap_select(F, cand, score, [1, 0], 2, [9], prior_idx, prior_sc, row_offset=off)
    assert list(idx[0]) == [off + 0, 7] and list(state[0]) == [2, 1]
    # a negative n_prior is no prior; without a pad and short of top_k the query is not done
    idx, _, state, _ = ref.cap_select(F, cand[:, 2:4], score[:, 2:4], [1, 0], 2, [-3], prior_idx, prior_sc, row_offset=off)
    assert list(idx[0]) == [off + 1, -1] and list(state[0]) == [1, 0]
    # a candidate that is already a prior pick is skipped, not counted twice
    idx, _, state, _ = ref.cap_select(F, np.array([[off + 0, off + 2]]), score[:, :2], [0, 2], 3, [1], prior_idx, prior_sc,
                                      row_offset=off)
    assert list(idx[0]) == [off + 0, off + 2, -1] and list(state[0]) == [2, 0]


# ---------------------------------------------------------------- the rounds are the one-pass walk
@pytest.mark.parametrize("seed", range(6))
def test_rounds_equal_the_greedy_walk_of_the_full_ranking(seed):
    rng = np.random.default_rng(100 + seed)
    n, Q = 700, 12
    F = np.stack([rng.integers(0, 134, n), rng.integers(0, 21, n)], axis=1).astype(np.uint8)
    if seed % 3 == 2:
        F = F[:, :1]
    # a produce shopper: the best rows are mostly one aisle and one department, with runs of tied scores
    scores = rng.standard_normal((Q, n)).astype(np.float32)
    hot = rng.choice(n, 300, replace=False)
    F[hot[:200], 0] = 7
    F[hot, -1] = 3
    scores[:, hot] += np.float32(3.0)
    scores = np.round(scores * 8) / 8  # ties
    scores[0, :5] = [0.0, -0.0, 0.0, -0.0, 0.0]
    excl = [rng.choice(n, int(rng.integers(0, 60)), replace=False).tolist() for _ in range(Q)]
    allow = [None if i % 3 == 0 else ([v for v in range(134) if v % 5 != i % 5], None)[:F.shape[1]] for i in range(Q)]
    masks = facet_masks(allow, Q, F.shape[1])
    admit = rng.random((Q, n)) < 0.9
    caps = np.stack([rng.choice([0, 1, 2, 3], Q), rng.choice([0, 1, 2, 5], Q)], axis=1)
    caps[1] = [2, 5]
    seen = set()
    for top_k, width in ((20, 20), (20, 80), (5, 128), (33, 64), (128, 128), (1, 1)):
        want = ref.greedy_walk(scores, F, caps, top_k, excl, admit & admitted_matrix(F, masks))
        idx, sc, rounds = ref.capped_rounds(scores, F, caps, top_k, width, excl, admit, masks)
        np.testing.assert_array_equal(idx, want[0])
        np.testing.assert_array_equal(sc.view(np.uint32), want[1].view(np.uint32))
        seen.add(rounds)
        for q in range(Q):  # the caps hold
            rows = idx[q][idx[q] >= 0]
            for f in range(F.shape[1]):
                if caps[q, f] > 0:
                    assert np.bincount(F[rows, f], minlength=1).max(initial=0) <= caps[q, f]
    assert max(seen) >= 2  # some case needed a continuation round


def test_uncapped_rounds_are_the_plain_search():
    rng = np.random.default_rng(3)
    scores = rng.standard_normal((4, 300)).astype(np.float32)
    F = rng.integers(0, 9, (300, 2)).astype(np.uint8)
    from tests.search_harness import select_from_scores

    idx, sc, rounds = ref.capped_rounds(scores, F, [0, -1], 20, 40)
    want = select_from_scores(scores, 20)
    np.testing.assert_array_equal(idx, want[0])
    np.testing.assert_array_equal(sc, want[1])
    assert rounds == 1


# ---------------------------------------------------------------- the host's argument checks
def test_cap_plan():
    assert cap_plan(None, None, True) is None and cap_plan(None, None, False) is None
    assert cap_plan(2, None, True) == (2, 0) and cap_plan(None, 5, True) == (0, 5) and cap_plan(np.int64(1), 128, True) == (1, 128)
    for bad in (0, -1, 1.5, 2.0, "2", True, 2**31):
        with pytest.raises(ValueError, match="max_per_aisle"):
            cap_plan(bad, None, True)
        with pytest.raises(ValueError, match="max_per_department"):
            cap_plan(1, bad, True)
    with pytest.raises(ValueError, match="facets"):
        cap_plan(2, None, False)


def test_ann_plan_refuses_caps():
    assert ann_plan(None, 16, max_per_aisle=2, max_per_department=1) is None  # no probes: nothing to refuse
    assert ann_plan(4, 16, max_per_aisle=None, max_per_department=None) == 4
    with pytest.raises(ValueError, match="max_per_aisle"):
        ann_plan(4, 16, max_per_aisle=2)
    with pytest.raises(ValueError, match="max_per_department"):
        ann_plan(4, 16, max_per_department=1)


def test_cap_pairs():
    assert cap_pairs((2, None), 3).tolist() == [[2, 0]] * 3 and cap_pairs([1, 5], 1).dtype == np.int32
    assert cap_pairs([[1, 0], [-4, 2**31 - 1]], 2).tolist() == [[1, 0], [0, 2**31 - 1]]
    for bad in ([1], [1, 2, 3], [[1, 2]] * 3, [1.5, 2]):
        with pytest.raises(ValueError, match="caps"):
            cap_pairs(bad, 2)


def test_cli_flags():
    args = cli.build_parser().parse_args(["--max-per-aisle", "2", "--max-per-department", "5"])
    assert args.max_per_aisle == 2 and args.max_per_department == 5
    none = cli.build_parser().parse_args([])
    assert none.max_per_aisle is None and none.max_per_department is None
    assert "--max-per-aisle" in cli.__doc__ and "--max-per-department" in cli.__doc__


# ---------------------------------------------------------------- the C entry point
def test_symbol_declared_exported_and_bound(native):
    header = (Path(__file__).resolve().parents[1] / "include" / "icrec.h").read_text()
    assert " icrec_cap_select(" in header and "icrec_cap_select" in native.EXPORTS
    assert len(native.lib().icrec_cap_select.argtypes) == 14


def test_argument_checks_need_no_device(native):
    """Every refusal comes before the first HIP call: a NULL pointer, the shapes, an index without facets."""
    lib = native.lib()
    buf = np.zeros(4096, np.int64)  # readable zeros behind every pointer; as a handle: an index without facets
    p = buf.ctypes.data

    def call(h=p, cand=p, sc=p, nq=2, k=16, caps=p, prior=p, allow=p, top_k=4, oi=p, osc=p, st=p, nxt=p):
        return lib.icrec_cap_select(h, cand, sc, nq, k, caps, prior, allow, top_k, oi, osc, st, nxt, None)

    for null in ("h", "cand", "sc", "caps", "oi", "osc", "st"):
        assert call(**{null: None}) == ICREC_EINVAL, null
        assert b"NULL" in lib.icrec_last_error()
    for bad, word in ((dict(nq=0), b"n_queries"), (dict(nq=-2), b"n_queries"), (dict(k=0), b"k must"), (dict(k=129), b"k must"),
                      (dict(top_k=0), b"top_k"), (dict(top_k=129), b"top_k")):
        assert call(**bad) == ICREC_EINVAL, bad
        assert word in lib.icrec_last_error(), (bad, lib.icrec_last_error())
    # the optional pointers may be NULL and top_k may exceed k: the next refusal is the handle's missing facets
    assert call(prior=None, allow=None, nxt=None, k=4, top_k=128) == ICREC_EINVAL
    assert b"no facets" in lib.icrec_last_error()
    assert not buf.any()
