"""Shared by the search GPU tests (test_search_gpu, test_search_dims_gpu, test_sharded_gpu, the search tests of
test_baseline_sizes_gpu): the imports and the GPU fixture, the check of an index against the oracle, the random
exclusion lists (one function per draw sequence), shard cutting, the tie-block catalog, the launch timers, the
properties of a result list and the memoised bench catalog.  One definition each; importing this needs no GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native, search, synthetic  # noqa: F401  (re-exported)
from instacart_next_order_recommendation_amd.search import DeviceIndex, merge_topk
from instacart_next_order_recommendation_amd.sharded import (  # noqa: F401  (re-exported)
    HipShardBackend, NativeComm, ShardedSearch, exclusions_to_shard_csr, shard_bounds)
from oracle import oracle
from tests.encoder_harness import n_cu  # noqa: F401  (re-exported: one definition for both harnesses)


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


# ---------------------------------------------------------------- an index against the oracle
def assert_search(out, want):
    """out = (idx, score) device tensors of a search or merge; want = the expected numpy pair.  Bit-equal."""
    np.testing.assert_array_equal(out[0].cpu().numpy(), want[0])
    np.testing.assert_array_equal(out[1].cpu().numpy(), want[1])


def check(ix, q, P, k, excl=None, *, partial=False):
    """ix.search(q, k, excl) equals the oracle over the host rows P the index was made from, indices and scores, with
    the index's own row storage and row offset; partial=True: its partial lists + merge_topk give the same.  Returns
    the expected pair.  The oracle's offset and storage are read from ix, not from what the test gave the constructor:
    a constructor that mangled them consistently would pass here - test_edge_cases and the golden sharded tests pin
    the offset on their own."""
    want = oracle.search(q, P, k, excl, row_offset=ix.row_offset,
                         storage="bf16" if ix.storage.startswith("bf16") else "f32")
    assert_search(ix.search(q, k, excl), want)
    if partial:
        assert_search(merge_topk(ix.search_partial(q, k, excl).unsqueeze(0), k), want)
    return want


def assert_ranked_lists(idx, sc, lo, hi, k):
    """Every list of a [Q, k] result: scores non-increasing, rows strictly increasing where scores tie, rows unique
    and inside [lo, hi)."""
    idx = idx.cpu().numpy() if isinstance(idx, torch.Tensor) else idx
    sc = sc.cpu().numpy() if isinstance(sc, torch.Tensor) else sc
    assert idx.shape == sc.shape and idx.shape[1] == k
    assert (idx >= lo).all() and (idx < hi).all()
    assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all()
    d = np.diff(sc, axis=1)
    assert (d <= 0).all()
    assert (np.diff(idx, axis=1)[d == 0] > 0).all()


def full_ranking(scores_row):
    """The complete ranking of one score row under the library's total order: score descending, row ascending."""
    return np.lexsort((np.arange(scores_row.size), -scores_row.astype(np.float64)))


# ---------------------------------------------------------------- random exclusion lists, one per draw sequence
def distinct_exclusions(rng, n, nq, cap=40, every=1):
    """Per query 0 .. min(n, cap) - 1 distinct rows in draw order; with every > 1 only queries 0, every, 2 every, ...
    draw a list and the others get [] without touching the generator."""
    return [rng.choice(n, size=int(rng.integers(0, min(n, cap))), replace=False).tolist() if i % every == 0 else []
            for i in range(nq)]


def sorted_exclusions(rng, n, nq, must=None, cap=40):
    """Per query 0 .. min(n, cap) distinct rows (the count's upper bound is INCLUSIVE), united with must[i], sorted."""
    out = []
    for i in range(nq):
        e = set(rng.choice(n, size=int(rng.integers(0, min(n, cap) + 1)), replace=False).tolist())
        if must is not None:
            e |= set(must[i].tolist())
        out.append(sorted(e))
    return out


def redrawn_exclusions(rng, n, nq, cap, none_every):
    """Per query 0 .. cap - 1 rows drawn WITH replacement, duplicates dropped, sorted; queries 0, none_every,
    2 none_every, ... get [] without touching the generator."""
    return [sorted(set(rng.integers(0, n, size=int(rng.integers(0, cap))).tolist())) if i % none_every else []
            for i in range(nq)]


# ---------------------------------------------------------------- shards
def local_exclusions(excl, lo, hi):
    """Global exclusion lists cut to the shard of rows [lo, hi) and rebased to its local rows."""
    return [[r - lo for r in e if lo <= r < hi] for e in excl]


def sharded_partial_keys(P, q, k, excl, bounds, storage="f32"):
    """One index per row shard bounds[r] .. bounds[r + 1] of P (host array or device tensor), each searched for its
    partial lists under its cut of the global exclusions -> keys [n_shards, Q, k], rank-major as an all-gather lays
    them down.  storage: one name, or a callable r -> name."""
    keys = []
    for r, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        shard = DeviceIndex(P[lo:hi], row_offset=lo, storage=storage(r) if callable(storage) else storage)
        keys.append(shard.search_partial(q, k, local_exclusions(excl, lo, hi)))
        shard.close()
    return torch.stack(keys)


# ---------------------------------------------------------------- catalogs
def tie_block_catalog(rng, n, dim, n_dup=300, n_near=200, *, draw_f32=False):
    """n random rows of which n_dup are one identical row (more than any candidate list holds) and n_near others sit
    1e-6 beside it -> (P, base_row).  draw_f32 picks the generator's float32 normals (test_search_dims_gpu) instead of
    float64 normals rounded to float32 (test_search_gpu): different streams, so each caller keeps its own."""
    def normal(shape):
        if draw_f32:
            return rng.standard_normal(shape, dtype=np.float32)
        return rng.standard_normal(shape).astype(np.float32)

    P = normal((n, dim))
    base_row = normal(dim)
    dup = rng.choice(n, n_dup, replace=False)
    P[dup] = base_row
    near = rng.choice(np.setdiff1d(np.arange(n), dup), n_near, replace=False)
    P[near] = base_row + 1e-6 * normal((n_near, dim))
    return P, base_row


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def bench_catalog():
    """bench.py's catalog, 49,688 x 384 unit rows - generated once per process (the counter-based generator is slow)
    and read-only: a test that writes into it copies it first.  The flag stops numpy writes only: torch.from_numpy
    warns once and shares the memory, so an in-place torch write through such a tensor would not be caught."""
    return _frozen(synthetic.synthetic_embeddings(49688, 384, seed=1))


@functools.lru_cache(maxsize=None)
def bench_queries(n, seed):
    """n query rows for bench_catalog(), once per process and read-only."""
    return _frozen(synthetic.synthetic_embeddings(n, 384, seed=seed))


# ---------------------------------------------------------------- launch timers
def timed(fn):
    """fn() once with the library's launch timers on -> (result, {slot: (avg ms, launches)}); slot 0 = search kernels,
    4 = the guarded exact pass behind a filter pass (include/icrec.h, icrec_timing_query).  The timers are off again
    afterwards, also when fn raises."""
    torch.cuda.synchronize()
    _native.timing_reset()
    _native.timing_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _native.timing_enable(False)
    return out, {s: _native.timing_query(s) for s in (0, 4)}
