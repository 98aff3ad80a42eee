"""MMR re-selection without a device: the numpy reference's own properties (tests/mmr_reference.py), the two C entry
points are declared, exported and bound, their argument checks answer before any GPU work, and the recommender's
diversity / candidates arguments are checked on the host."""
from __future__ import annotations

import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from instacart_next_order_recommendation_amd.recommender import diversity_plan
from oracle import oracle
from tests import mmr_reference as ref

MMR_SYMBOLS = ("icrec_mmr_select_workspace_bytes", "icrec_mmr_select")
ICREC_EINVAL, ICREC_ENOMEM = -1, -3


@pytest.fixture(scope="module")
def native():
    from instacart_next_order_recommendation_amd import _native

    if not _native.LIB_PATH.exists():
        _native.build()
    return _native


@pytest.fixture(scope="module")
def case():
    """2,000 x 64 clustered rows, 6 queries near rows of the catalog, the oracle's top-40."""
    rng = np.random.default_rng(11)
    centres = rng.standard_normal((25, 64)).astype(np.float32)
    P = centres[rng.integers(0, 25, 2000)] + np.float32(0.35) * rng.standard_normal((2000, 64)).astype(np.float32)
    q = P[rng.choice(2000, 6, replace=False)] + np.float32(0.1) * rng.standard_normal((6, 64)).astype(np.float32)
    idx, sc = oracle.search(q, P, 40)
    return P, ref.stored_rows(P), idx, sc


# ---------------------------------------------------------------- the reference's own properties
def test_lambda_one_is_the_identity(case):
    _, p_hat, idx, sc = case
    for top_k in (1, 17, 40):
        for q in range(idx.shape[0]):
            assert ref.select_positions(p_hat, idx[q], sc[q], top_k, 1.0) == list(range(top_k))
        got = ref.mmr_select(p_hat, idx, sc, top_k, 1.0)
        np.testing.assert_array_equal(got[0], idx[:, :top_k])
        np.testing.assert_array_equal(got[1], sc[:, :top_k])


@pytest.mark.parametrize("lam", [0.7, 0.3])
def test_diversified_lists_differ_from_the_plain_order(case, lam):
    _, p_hat, idx, sc = case
    got_idx, got_rel = ref.mmr_select(p_hat, idx, sc, 10, lam)
    for q in range(idx.shape[0]):
        assert got_idx[q, 0] == idx[q, 0]  # the first pick is the best match
        assert set(got_idx[q]) != set(idx[q, :10]), q
        assert len(set(got_idx[q])) == 10 and set(got_idx[q]) <= set(idx[q])
        np.testing.assert_array_equal(got_rel[q], sc[q][[list(idx[q]).index(i) for i in got_idx[q]]])


def test_lambda_zero_takes_no_duplicate_while_a_distinct_row_is_left():
    rng = np.random.default_rng(5)
    P = rng.standard_normal((30, 32)).astype(np.float32)
    P[[3, 9, 21]] = P[0]   # four copies of one row
    P[[14, 15]] = P[7]     # three of another
    p_hat = ref.stored_rows(P)
    cand = np.arange(30, dtype=np.int64)[None, :]
    rel = rng.standard_normal((1, 30)).astype(np.float32)
    distinct = 30 - 3 - 2
    picks = ref.select_positions(p_hat, cand[0], rel[0], 30, 0.0)
    assert sorted(picks) == list(range(30))
    assert picks[0] == int(np.argmax(rel[0]))
    seen = [tuple(P[j]) for j in picks[:distinct]]
    assert len(set(seen)) == distinct  # every distinct row once before any copy returns


def test_pads_and_invalid_candidates():
    rng = np.random.default_rng(6)
    P = rng.standard_normal((10, 32)).astype(np.float32)
    p_hat = ref.stored_rows(P)
    off = 1000
    cand = np.array([[off + 4, -1, off + 12, off - 1, off + 9, off + 4, 3, -1],
                     [-1, -1, off + 10, 5, -1, off + 99, -1, -1]], np.int64)
    rel = rng.standard_normal(cand.shape).astype(np.float32)
    idx, out = ref.mmr_select(p_hat, cand, rel, 5, 0.5, row_offset=off)
    assert sorted(idx[0, :3]) == [off + 4, off + 4, off + 9] and list(idx[0, 3:]) == [-1, -1]  # a row listed twice is two candidates
    assert list(out[0, 3:]) == [0.0, 0.0] and set(out[0, :3]) == {rel[0, 0], rel[0, 4], rel[0, 5]}
    assert (idx[1] == -1).all() and (out[1] == 0).all()  # no valid candidate at all


def test_nan_sorts_last_and_ties_go_to_the_lower_position():
    v = np.array([np.nan, 1.0, 2.0, np.nan, 2.0, -0.0], np.float32)
    every = np.ones(6, bool)
    assert ref.ordered_first(v, every) == 2
    assert ref.ordered_first(v, np.array([1, 0, 0, 1, 0, 0], bool)) == 0
    assert ref.ordered_first(v, np.array([1, 0, 0, 1, 0, 1], bool)) == 5
    assert ref.ordered_first(np.array([0.0, -0.0], np.float32), np.ones(2, bool)) == 0
    assert ref.ordered_first(np.array([-0.0, 0.0], np.float32), np.ones(2, bool)) == 0
    assert ref.ordered_first(v, np.zeros(6, bool)) == -1


# ---------------------------------------------------------------- the C entry points
def test_symbols_declared_exported_and_bound(native):
    header = (Path(__file__).resolve().parents[1] / "include" / "icrec.h").read_text()
    lib = native.lib()
    for name in MMR_SYMBOLS:
        assert f"ICREC_API" in header and f" {name}(" in header, name
        assert name in native.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.icrec_mmr_select.argtypes[6] is C.c_float


def test_workspace_bytes_bad_arguments(native):
    lib = native.lib()
    assert lib.icrec_mmr_select_workspace_bytes(None, 4, 20) == 0
    fake = np.zeros(64, np.int64)  # stands in for a handle: the shape is refused before it would be looked at
    h = fake.ctypes.data
    for nq, k in ((0, 20), (-1, 20), (4, 0), (4, 129)):
        assert lib.icrec_mmr_select_workspace_bytes(h, nq, k) == 0
    assert lib.icrec_mmr_select_workspace_bytes(h, 3, 128) >= 3 * 128 * 128 * 4


def test_argument_checks_need_no_device(native):
    """Every refusal comes before the first HIP call: a NULL pointer, the shape, lambda, a short workspace."""
    lib = native.lib()
    buf = np.zeros(4096, np.int64)  # readable memory behind every pointer, the handle included; none is dereferenced
    p = buf.ctypes.data
    big = 1 << 30

    def call(h=p, cand=p, rel=p, nq=2, k=16, top_k=4, lam=0.5, oi=p, orel=p, ws=p, nbytes=big):
        return lib.icrec_mmr_select(h, cand, rel, nq, k, top_k, lam, oi, orel, ws, nbytes, None)

    for null in ("h", "cand", "rel", "oi", "orel", "ws"):
        assert call(**{null: None}) == ICREC_EINVAL, null
        assert b"NULL" in lib.icrec_last_error()
    for bad, word in ((dict(nq=0), b"n_queries"), (dict(k=0), b"k must"), (dict(k=129, top_k=4), b"k must"),
                      (dict(top_k=0), b"top_k"), (dict(top_k=17), b"top_k"), (dict(lam=-0.1), b"lambda"),
                      (dict(lam=1.5), b"lambda"), (dict(lam=math.nan), b"lambda")):
        assert call(**bad) == ICREC_EINVAL, bad
        assert word in lib.icrec_last_error(), (bad, lib.icrec_last_error())
    need = lib.icrec_mmr_select_workspace_bytes(p, 2, 16)
    assert call(nbytes=need - 1) == ICREC_ENOMEM
    assert b"workspace" in lib.icrec_last_error()


# ---------------------------------------------------------------- the recommender's arguments
def test_diversity_plan():
    assert diversity_plan(None, None, 10, 700) is None
    assert diversity_plan(0, None, 10, 700) is None and diversity_plan(0.0, 64, 10, 700) is None
    assert diversity_plan(0.5, None, 10, 700) == (0.5, 40)
    assert diversity_plan(1, None, 50, 700) == (0.0, 128)
    assert diversity_plan(0.25, 64, 10, 700) == (0.75, 64)
    assert diversity_plan(0.5, None, 10, 25) == (0.5, 25)       # clipped to the catalog
    assert diversity_plan(0.5, None, 10, 6) == (0.5, 6)         # ... and never below the clipped top_k
    assert diversity_plan(0.5, 10, 10, 700) == (0.5, 10)
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="diversity"):
            diversity_plan(bad, None, 10, 700)
    for bad in (9, 129, 0):
        with pytest.raises(ValueError, match="candidates"):
            diversity_plan(0.5, bad, 10, 700)
        with pytest.raises(ValueError, match="candidates"):
            diversity_plan(None, bad, 10, 700)
