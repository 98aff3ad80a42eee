"""icrec_index_write_rows / _write_facets / _export_filter on the GPU: after a write the handle is, bit for bit, the handle
icrec_index_create_ex makes from the edited matrix - the stored rows, the filter planes or fragments - for every row
storage, at rows on the edges of the 32-row fragment tiles and the 256-row rounds (n = 1,061 = 4 x 256 + 32 + 5), with
ids outside the index in the list; searches find the new rows through every kernel family; captured graphs follow the
write; facet words change alone; an IVF built again from its centroids equals a new one."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.search import DeviceIndex, IvfIndex, facet_masks
from tests.search_harness import (admitted_matrix, assert_search, check, select_from_scores, sorted_exclusions,
                                  torch_cuda)  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N = 1061
EDGES = [0, 31, 32, 255, 256, 1023, 1024, 1055, 1056, 1060]
CASES = [("f32", 32, N), ("f32", 96, N), ("f32", 384, N), ("f32", 4096, 70), ("bf16", 64, N), ("bf16", 384, N),
         ("f32+filter", 128, N), ("f32+filter", 384, N), ("bf16+filter", 128, N), ("bf16+filter", 384, N)]
CASE_IDS = [f"{s}-{d}" for s, d, _ in CASES]
FILTER = [c for c in CASES if c[0].endswith("filter")]
K = 20


def new_rows(rng, m, dim):
    """m rows with norms from 1e-3 to 1e3, of which row 1 is all zero and row 2 has a norm below 1e-12."""
    X = rng.standard_normal((m, dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X *= np.logspace(-3, 3, m, dtype=np.float32)[rng.permutation(m)][:, None]
    X[1] = 0.0
    X[2] *= np.float32(1e-14) / np.linalg.norm(X[2])
    assert 0 < np.linalg.norm(X[2].astype(np.float64)) < 1e-12
    return X


def id_list(rng, n, seed_rows=EDGES):
    """The written ids as the kernel gets them: -5 in front, the edge rows the index has and 40 random others
    ascending, n and 2^31 - 1 behind -> (the whole list int32, the positions of its valid entries)."""
    edges = [r for r in seed_rows if r < n]
    others = rng.choice(np.setdiff1d(np.arange(n), edges), 40, replace=False)
    valid = np.sort(np.concatenate([edges, others])).astype(np.int64)
    ids = np.concatenate([[-5], valid, [n, 2**31 - 1]]).astype(np.int32)
    return ids, np.arange(1, 1 + valid.size)


def bits(t):
    """A device tensor's elements as unsigned integers of their width, on the host."""
    a = t.cpu().contiguous()
    return a.view({2: torch.int16, 4: torch.int32}[a.element_size()]).numpy()


def assert_same_index(ix, fresh):
    np.testing.assert_array_equal(bits(ix.export()), bits(fresh.export()))
    if ix.storage.endswith("filter"):
        for got, want in zip(ix.export_filter(), fresh.export_filter()):
            np.testing.assert_array_equal(bits(got), bits(want))


@functools.lru_cache(maxsize=None)
def world(storage, dim, n):
    """One written index per case, kept for the module: P the rows it was made from, ids / X what was written (with the
    out-of-range entries), E the edited host matrix, fresh = a new index of the same storage over E."""
    rng = np.random.default_rng(1000 + dim + len(storage))
    P = rng.standard_normal((n, dim)).astype(np.float32)
    ids, pos = id_list(rng, n)
    X = new_rows(rng, ids.size, dim)          # (its zero row and its tiny row, entries 1 and 2, go to rows the index has)
    E = P.copy()
    E[ids[pos]] = X[pos]
    ix = DeviceIndex(P, storage=storage)
    ix.write_rows(torch.from_numpy(ids).to(ix.device), X)   # a device list: the host form refuses ids outside the index
    fresh = DeviceIndex(E, storage=storage)
    return P, ids, pos, X, E, ix, fresh


@pytest.mark.parametrize("storage,dim,n", CASES, ids=CASE_IDS)
def test_written_index_is_the_fresh_index(torch_cuda, storage, dim, n):
    P, ids, pos, X, E, ix, fresh = world(storage, dim, n)
    assert_same_index(ix, fresh)
    stored = ix.export().cpu().numpy()
    assert pos[0] == 1 and not X[1].any() and not stored[ids[1]].any()                    # the all-zero row stays zero
    untouched = np.setdiff1d(np.arange(n), ids[pos])
    before = DeviceIndex(P, storage=storage)
    np.testing.assert_array_equal(bits(ix.export())[untouched], bits(before.export())[untouched])
    before.close()


@pytest.mark.parametrize("storage,dim,n", CASES, ids=CASE_IDS)
def test_searches_find_the_written_rows(torch_cuda, storage, dim, n):
    """Queries beside the new rows: the rewritten rows are their best hits, their old contents are far away."""
    P, ids, pos, X, E, ix, fresh = world(storage, dim, n)
    rng = np.random.default_rng(7)
    k = min(K, n)
    for Q in (1, 40) + ((256,) if storage.endswith("filter") else ()):
        target = ids[pos][np.arange(Q) % pos.size] if Q > 1 else ids[pos][[5]]
        scale = np.maximum(np.linalg.norm(E[target], axis=1, keepdims=True), 1e-30).astype(np.float32)
        q = (E[target] / scale + np.float32(0.05 / np.sqrt(dim)) * rng.standard_normal((Q, dim))).astype(np.float32)
        want = check(ix, q, E, k)
        hit = want[0][:, 0] == target
        assert hit.mean() > 0.9, hit.mean()                                               # (all but the zero row's queries)
        excl = sorted_exclusions(rng, n, Q, must=[np.asarray([t] if i % 2 == 0 else [], np.int64) for i, t in enumerate(target)])
        check(ix, q, E, k, excl)


@pytest.mark.parametrize("storage,dim,n", CASES, ids=CASE_IDS)
def test_every_row_one_row_no_row(torch_cuda, storage, dim, n):
    rng = np.random.default_rng(11)
    P = rng.standard_normal((n, dim)).astype(np.float32)
    ix = DeviceIndex(P, storage=storage)
    try:
        E = new_rows(rng, n, dim)                                                         # m = n: a re-trained model
        ix.write_rows(np.arange(n), E)
        assert_same_index(ix, DeviceIndex(E, storage=storage))
        E1 = E.copy()                                                                     # m = 1, host ids
        E1[n - 1] = rng.standard_normal(dim).astype(np.float32)
        ix.write_rows([n - 1], E1[n - 1:n])
        fresh = DeviceIndex(E1, storage=storage)
        assert_same_index(ix, fresh)
        ix.write_rows([], np.zeros((0, dim), np.float32))                                 # m = 0
        assert _native.lib().icrec_index_write_rows(ix._h, None, None, 0, None) == 0
        assert _native.lib().icrec_index_write_rows(ix._h, None, None, 1, None) == -1     # a NULL pointer with m > 0
        ix.write_rows([5, 3], E1[[5, 3]])                                                 # host ids out of order: sorted with their rows
        assert_same_index(ix, fresh)
    finally:
        ix.close()


GRAPH_CASES = [("f32", 384, (1, 40)), ("f32+filter", 128, (256,)), ("bf16+filter", 384, (1, 256))]


@pytest.mark.parametrize("storage,dim,Qs", GRAPH_CASES, ids=[f"{s}-{d}" for s, d, _ in GRAPH_CASES])
def test_graphs_follow_a_write(torch_cuda, storage, dim, Qs):
    rng = np.random.default_rng(13)
    P = rng.standard_normal((N, dim)).astype(np.float32)
    ids, pos = id_list(rng, N)
    X = new_rows(rng, ids.size, dim)
    E = P.copy()
    E[ids[pos]] = X[pos]
    ids2, pos2 = id_list(rng, N, seed_rows=[1, 30, 33, 254, 257, 1022, 1025, 1054, 1057, 1059])
    assert ids2.size == ids.size                                                          # the buffers keep their size
    X2 = new_rows(rng, ids.size, dim)
    E2 = E.copy()
    E2[ids2[pos2]] = X2[pos2]
    ix = DeviceIndex(P, storage=storage)
    old, fresh, fresh2 = DeviceIndex(P, storage=storage), DeviceIndex(E, storage=storage), DeviceIndex(E2, storage=storage)
    ids_d, rows_d = torch.from_numpy(ids).to(ix.device), torch.from_numpy(X).to(ix.device)
    try:
        for Q in Qs:
            target = ids[pos][(np.arange(Q) + 5) % pos.size]                              # (a single query: not the zero row's)
            q = (E[target] / np.maximum(np.linalg.norm(E[target], axis=1, keepdims=True), 1e-30)
                 + 0.05 / np.sqrt(dim) * rng.standard_normal((Q, dim))).astype(np.float32)
            qd = torch.from_numpy(q).to(ix.device)
            idx = torch.empty((Q, K), dtype=torch.int64, device=ix.device)
            sc = torch.empty((Q, K), dtype=torch.float32, device=ix.device)
            ws = torch.empty(int(_native.lib().icrec_search_workspace_bytes(ix._h, Q, K)), dtype=torch.uint8, device=ix.device)
            ix.write_rows(np.arange(N), P)                                                # back to the old rows
            ix.search_into(qd, K, None, None, idx, sc, ws=ws)                             # first launches outside the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ix.search_into(qd, K, None, None, idx, sc, ws=ws)
            g.replay()
            torch.cuda.synchronize()
            assert_search((idx, sc), [t.cpu().numpy() for t in old.search(qd, K)])
            ix.write_rows_into(ids_d, rows_d)                                             # same stream as the replays
            g.replay()
            torch.cuda.synchronize()
            assert_search((idx, sc), [t.cpu().numpy() for t in fresh.search(qd, K)])
            assert (idx.cpu().numpy()[:, 0] == target).mean() > 0.9

            # the write and the search in one graph, then other ids and rows in the same buffers
            ix.write_rows(np.arange(N), P)
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                ix.write_rows_into(ids_d, rows_d)
                ix.search_into(qd, K, None, None, idx, sc, ws=ws)
            g2.replay()
            torch.cuda.synchronize()
            assert_search((idx, sc), [t.cpu().numpy() for t in fresh.search(qd, K)])
            ids_d.copy_(torch.from_numpy(ids2))
            rows_d.copy_(torch.from_numpy(X2))
            g2.replay()
            torch.cuda.synchronize()
            assert_same_index(ix, fresh2)
            assert_search((idx, sc), [t.cpu().numpy() for t in fresh2.search(qd, K)])
            ids_d.copy_(torch.from_numpy(ids))
            rows_d.copy_(torch.from_numpy(X))
    finally:
        for i in (ix, old, fresh, fresh2):
            i.close()


# ---------------------------------------------------------------- facets
FACET_ROWS = [0, 255, 256, 511, 1023, 1024, 1055, 1056, 1060]   # tile edges and the ragged last tile


def test_write_facets_changes_those_words_alone(torch_cuda):
    rng = np.random.default_rng(17)
    dim = 384
    P = rng.standard_normal((N, dim)).astype(np.float32)
    F = np.stack([rng.integers(0, 120, N), rng.integers(0, 21, N)], axis=1).astype(np.uint8)
    ix = DeviceIndex(P, storage="f32+filter")
    plain = DeviceIndex(P)
    try:
        ix.set_facets(F)
        Fe = F.copy()
        Fe[FACET_ROWS] = np.stack([np.full(len(FACET_ROWS), 200), 30 + np.arange(len(FACET_ROWS))], axis=1).astype(np.uint8)
        order = rng.permutation(len(FACET_ROWS))                                          # host ids in any order
        ix.write_facets(np.asarray(FACET_ROWS)[order], Fe[FACET_ROWS][order])
        for Q in (1, 40, 256):
            q = rng.standard_normal((Q, dim)).astype(np.float32)
            qd = torch.from_numpy(q).to(ix.device)
            kinds = [([200], None), (None, [30, 38, 3]), (list(range(0, 120, 2)) + [200], list(range(0, 40))), None, ([7], [5])]
            allow = [kinds[i % len(kinds)] for i in range(Q)]
            masks = facet_masks(allow, Q, 2)
            S = plain.scores(qd).cpu().numpy()
            want = select_from_scores(S, K, admit=admitted_matrix(Fe, masks))
            assert_search(ix.search(qd, K, allow=facet_masks(allow, Q, 2, ix.device)), want)
            assert sorted(want[0][0][want[0][0] >= 0].tolist()) == FACET_ROWS             # aisle 200: the rewritten rows alone
        # refusals change nothing: unsorted or repeated rows, a row outside the index, an index without facets
        lib = _native.lib()
        two = np.asarray([[1, 1], [2, 2]], np.uint8)
        for bad in ([5, 3], [3, 3], [3, N], [-1, 3]):
            rows = np.asarray(bad, np.int32)
            assert lib.icrec_index_write_facets(ix._h, rows.ctypes.data_as(C.c_void_p), two.ctypes.data_as(C.c_void_p), 2) == -1
        assert lib.icrec_index_write_facets(plain._h, np.asarray([3, 5], np.int32).ctypes.data_as(C.c_void_p),
                                            two.ctypes.data_as(C.c_void_p), 2) == -1
        assert b"no facets" in lib.icrec_last_error() and plain.n_facets == 0
        with pytest.raises(ValueError, match="named twice"):
            ix.write_facets([3, 3], two)
        with pytest.raises(_native.IcrecError, match="no facets"):
            plain.write_facets([3, 5], two)
        q = rng.standard_normal((40, dim)).astype(np.float32)
        allow = [([1, 2, 200], None)] * 40
        S = plain.scores(torch.from_numpy(q).to(ix.device)).cpu().numpy()
        assert_search(ix.search(q, K, allow=facet_masks(allow, 40, 2, ix.device)),
                      select_from_scores(S, K, admit=admitted_matrix(Fe, facet_masks(allow, 40, 2))))
        # one facet per row
        plain.set_facets(F[:, :1])
        plain.write_facets(FACET_ROWS, Fe[FACET_ROWS, :1])
        allow = [([200],)] * 3
        got = plain.search(q[:3], K, allow=facet_masks(allow, 3, 1, ix.device))
        assert_search(got, select_from_scores(S[:3], K, admit=admitted_matrix(Fe[:, :1], facet_masks(allow, 3, 1))))
    finally:
        ix.close()
        plain.close()


# ---------------------------------------------------------------- IVF
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_ivf_rebuilt_from_its_centroids_is_a_new_ivf(torch_cuda, storage):
    rng = np.random.default_rng(19)
    dim = 384
    P = rng.standard_normal((N, dim)).astype(np.float32)
    ids, pos = id_list(rng, N)
    X = new_rows(rng, ids.size, dim)
    E = P.copy()
    E[ids[pos]] = X[pos]
    cent = rng.standard_normal((8, dim)).astype(np.float32)
    ix, fresh = DeviceIndex(P, storage=storage), DeviceIndex(E, storage=storage)
    ivf = IvfIndex(ix, cent)
    try:
        ix.write_rows(ids[pos], X[pos])
        ivf.rebuild()
        new = IvfIndex(fresh, cent)
        for got, want in zip(ivf.layout(), new.layout()):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
        target = ids[pos][np.arange(40) % pos.size]
        q = (E[target] / np.maximum(np.linalg.norm(E[target], axis=1, keepdims=True), 1e-30)
             + 0.05 / np.sqrt(dim) * rng.standard_normal((40, dim))).astype(np.float32)
        excl = sorted_exclusions(rng, N, 40)
        for probes in (1, 3, 8):
            for e in (None, excl):
                assert_search(ivf.search(q, K, probes, e), [t.cpu().numpy() for t in new.search(q, K, probes, e)])
        assert_search(ivf.search(q, K, 8, excl), [t.cpu().numpy() for t in ix.search(q, K, excl)])
        check(ix, q, E, K, excl)
        new.close()
    finally:
        ivf.close()
        ix.close()
        fresh.close()
