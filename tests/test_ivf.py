"""The IVF index without a GPU: tests/ivf_reference.py against the oracle it restates, the layout's properties, and the
argument checks of the recommender, the command line and the C ABI that run before any device call."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import _native, cli
from instacart_next_order_recommendation_amd.recommender import ann_plan
from oracle import oracle
from tests import ivf_reference as ref
from tests.search_harness import distinct_exclusions


@pytest.fixture(scope="module")
def small():
    """1,500 x 64 rows around 12 centroids drawn from them, 9 queries near rows of the catalog."""
    rng = np.random.default_rng(21)
    P = rng.standard_normal((1500, 64)).astype(np.float32)
    Cn = P[rng.choice(1500, 12, replace=False)].copy()
    q = P[rng.choice(1500, 9, replace=False)] + np.float32(0.3) * rng.standard_normal((9, 64)).astype(np.float32)
    return P, Cn, q


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_all_lists_probed_is_the_exact_search(small, storage):
    P, Cn, q = small
    rng = np.random.default_rng(3)
    for excl in (None, distinct_exclusions(rng, 1500, 9)):
        for k in (1, 20):
            want = oracle.search(q, P, k, excl, row_offset=7, storage=storage)
            got = ref.search(q, P, Cn, k, 12, excl, row_offset=7, storage=storage)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])


def test_recall_grows_with_the_probes(small):
    """The probed set at nprobe is a prefix of the one at nprobe + 1: per query, the exact top-k rows found never
    decrease."""
    P, Cn, q = small
    exact = oracle.search(q, P, 20)[0]
    a = ref.assign(ref.stored_rows(P), Cn)
    found_before = np.zeros(len(q), int)
    for nprobe in range(1, 13):
        pr = ref.probes(q, Cn, nprobe)
        if nprobe > 1:
            np.testing.assert_array_equal(pr[:, :-1], ref.probes(q, Cn, nprobe - 1))
        idx = ref.search(q, P, Cn, 20, nprobe, assignment=a)[0]
        found = np.asarray([np.isin(exact[i], idx[i]).sum() for i in range(len(q))])
        assert (found >= found_before).all()
        found_before = found
    assert (found_before == 20).all()


def test_layout_is_a_permutation_sorted_inside_each_list(small):
    P, Cn, _ = small
    a = ref.assign(ref.stored_rows(P), Cn)
    perm, off = ref.layout(a, 12)
    assert perm.dtype == np.int32 and off.dtype == np.int64
    np.testing.assert_array_equal(np.sort(perm), np.arange(1500))
    assert off[0] == 0 and off[-1] == 1500 and (np.diff(off) >= 0).all()
    for l in range(12):
        rows = perm[off[l]:off[l + 1]]
        assert (a[rows] == l).all() and (np.diff(rows) > 0).all()


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_crafted_catalog_preconditions(storage):
    a = ref.crafted_preconditions(storage)
    perm, off = ref.layout(a, len(ref.CRAFTED_COUNTS))
    np.testing.assert_array_equal(np.diff(off), ref.CRAFTED_COUNTS)


# ---------------------------------------------------------------- argument checks that need no device
def test_probes_argument_combinations():
    assert ann_plan(None, None) is None and ann_plan(None, 16, aisles=["a"]) is None
    assert ann_plan(4, 16) == 4 and ann_plan(16, 16) == 16
    with pytest.raises(ValueError, match="ann_lists"):
        ann_plan(4, None)
    for kw, what in (({"aisles": ["produce"]}, "aisles"), ({"departments": []}, "departments"),
                     ({"boosts": {"1": 0.5}}, "boosts"), ({"only_boosted": True}, "boosts")):
        with pytest.raises(ValueError, match=f"probes cannot be combined with {what}"):
            ann_plan(4, 16, **kw)
    for bad in (0, -1, 17, 2.5, True):
        with pytest.raises(ValueError, match="probes must be an integer"):
            ann_plan(bad, 16)
    with pytest.raises(ValueError, match=r"\[1, 128\]"):
        ann_plan(129, 4096)  # ICREC_MAX_K bounds the probes of a large index
    assert ann_plan(128, 4096) == 128


def test_cli_parses_ann_lists_and_probes():
    ap = cli.build_parser()
    assert cli.ann_args(ap.parse_args(["--ann-lists", "64", "--probes", "8"])) == (64, 8)
    assert cli.ann_args(ap.parse_args([])) == (None, None)
    for argv in (["--probes", "8"], ["--ann-lists", "64"], ["--ann-lists", "4", "--probes", "5"],
                 ["--ann-lists", "4", "--probes", "0"]):
        with pytest.raises(SystemExit):
            cli.ann_args(ap.parse_args(argv))
    with pytest.raises(SystemExit):
        ap.parse_args(["--probes", "many"])


def test_ivf_entry_points_validate_arguments():
    """The IVF entry points reject bad arguments without touching a GPU."""
    if not _native.LIB_PATH.exists():
        _native.build()
    lib = _native.lib()
    h = C.c_void_p()
    assert lib.icrec_ivf_create(None, None, 4, C.byref(h)) == -1
    assert b"icrec_ivf_create" in lib.icrec_last_error()
    assert lib.icrec_ivf_lists(None) == -1
    assert lib.icrec_ivf_destroy(None) == 0
    assert lib.icrec_ivf_layout(None, None, None, None) == -1
    assert lib.icrec_ivf_search_workspace_bytes(None, 1, 20, 4) == 0
    assert lib.icrec_ivf_search(None, None, 1, 20, 4, None, None, None, None, None, 0, None) == -1
    assert b"icrec_ivf_search" in lib.icrec_last_error()
