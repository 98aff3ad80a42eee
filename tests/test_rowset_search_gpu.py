"""icrec_search_in_sets on the GPU.  One specification for every case: the result is bit-identical, indices and scores,
to the plain search with exclusion lists equal to the given exclusions united with every inadmissible row - checked
against the CPU oracle AND against ix.search on the device with those lists (tests/rowset_cases.py)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd.search import facet_masks, rowset_bits, rowset_ids
from tests.rowset_cases import (EMPTY, FIVE, FULL, HALF, INT32_MAX, KINDS, N, N_SETS, ONE, ONEPCT, SEVEN, TWELVE,
                                admitted_by_sets, check_in_sets, index_with_sets, mixed_ids, resident_lds_sets,
                                standard_sets)
from tests.search_harness import (FILTER_MIN_Q, LDS_MAX, DeviceIndex, _native, assert_search, filter_list_len, n_cu, oracle,
                                  sorted_exclusions, stream_plan, tie_block_catalog, tiled_plan)
from tests.search_harness import torch_cuda  # noqa: F401  (fixture)
from tests.test_facet_search_gpu import facets, mixed_allow, small_catalog

pytestmark = pytest.mark.gpu

FORMS = [(1, 20), (2, 20), (20, 20), (50, 20), (100, 20), (20, 100)]  # stream 1, stream 2, CfgSmall, CfgMid, CfgBig, CfgSmall by k


def dev(ids, ix):
    return torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(ix.device)


# ---------------------------------------------------------------- every launch form at the smallest shape that reaches it
@pytest.mark.parametrize("mode", ["sets", "sets+excl", "sets+masks", "sets+masks+excl"])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [64, 384])
def test_launch_forms(torch_cuda, dim, storage, mode):
    assert [tiled_plan(N, Q, k, n_cu())[0] for Q, k in FORMS[2:]] == ["small", "mid", "big", "small"]
    assert [stream_plan(N, Q, n_cu())[2] for Q, _ in FORMS[:2]] == [1, 2] and N % 128 and N % 256
    assert len(KINDS) == 17 and max(len(kd) for kd in KINDS) == 4
    P, q = small_catalog(dim)
    member, F = standard_sets(), facets()
    ix = index_with_sets(P, member, storage, F if "masks" in mode else None)
    for Q, k in FORMS:
        rng = np.random.default_rng(Q * 1000 + k)
        excl = sorted_exclusions(rng, N, Q) if "excl" in mode else None
        allow = mixed_allow(rng, F, Q) if "masks" in mode else None
        for start in ((0, 9) if Q <= 2 else (0,)):   # the one or two queries of a streaming launch: several kinds
            check_in_sets(ix, q[:Q], P, k, member, mixed_ids(Q, start), excl, F, allow)
    ix.close()


@pytest.mark.parametrize("catalog", ["random", "ties"])
@pytest.mark.parametrize("dim", [384, 128], ids=["resident", "staged"])
@pytest.mark.parametrize("storage", ["f32+filter", "bf16+filter"])
def test_filter_storages(torch_cuda, storage, dim, catalog):
    """Q = 300 takes the f16 filter pass (resident fragments at dim 384, staged planes otherwise) and the verification.
    "ties": 300 identical rows of which every other one is in the set, and queries beside them - more equal scores
    among members than a candidate list holds, so the guarded exact pass decides, and it must apply the same sets: ties
    come out by row number among members only."""
    Q, k = 300, 20
    assert Q >= FILTER_MIN_Q and resident_lds_sets(filter_list_len(k)) <= LDS_MAX   # the filter pass is taken
    rng = np.random.default_rng(dim + len(storage))
    member = standard_sets().copy()
    if catalog == "random":
        P, q = small_catalog(dim)
    else:
        P, base = tie_block_catalog(rng, N, dim, draw_f32=True)
        q = rng.standard_normal((Q, dim), dtype=np.float32)
        q[:200] = base + 0.05 * q[:200]
        dup = np.flatnonzero((P == base).all(axis=1))
        member[HALF, dup] = False
        member[HALF, dup[::2]] = True   # alternate copies
        near = np.setdiff1d(np.flatnonzero(np.abs(P - base).max(axis=1) < 1e-4), dup)
        member[HALF, near] = False      # the rows 1e-6 beside the copies: the copies alone are the set's best matches
        assert len(dup) == 300 and len(near) == 200 and member[HALF, dup].sum() == 150 > filter_list_len(k)
    F = facets()
    ix = index_with_sets(P, member, storage, F)
    ids = mixed_ids(Q)
    idx, _ = check_in_sets(ix, q, P, k, member, ids)
    for excl, allow in ((sorted_exclusions(rng, N, Q), None), (None, mixed_allow(rng, F, Q))):
        check_in_sets(ix, q, P, k, member, ids, excl, F, allow)
    if catalog == "ties":
        for i in [i for i in range(0, 200) if i % 17 in (0, 4)]:   # KINDS 0 and 4: HALF alone
            rows = idx[i][idx[i] >= 0]
            assert member[HALF, rows].all()
            np.testing.assert_array_equal(rows, dup[::2][:k])   # equal scores: the k lowest member copies, by row
    ix.close()


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_streaming_kernel_four_and_eight_queries(torch_cuda, storage):
    """Q = 4 and 8 stream once every block has two tiles: n just above 2 * 3 * n_cu * 256 rows (make_plan)."""
    dim = 64 if storage == "bf16" else 32
    n = 2 * 3 * n_cu() * 256 + 293
    for Q in (4, 8):
        plan = stream_plan(n, Q, n_cu())
        assert plan is not None and plan[2] == Q and plan[4] >= 2 and n % 256
    rng = np.random.default_rng(n_cu())
    P = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((8, dim), dtype=np.float32)
    member = standard_sets(n, 12)
    F = facets(n, seed=6)
    ix = index_with_sets(P, member, storage, F)
    within = [[HALF], [ONEPCT, HALF], [-1], [N_SETS], [FIVE], [TWELVE, SEVEN, FULL, -7], [INT32_MAX], [ONE, ONE]]
    for Q in (4, 8):
        ids = rowset_ids(within[8 - Q:], Q, 4)
        check_in_sets(ix, q[:Q], P, 20, member, ids, sorted_exclusions(rng, n, Q))
        check_in_sets(ix, q[:Q], P, 20, member, ids, None, F, [[None, [int(F[5, 1]), int(F[6, 1])]]] * Q)
    ix.close()


@pytest.mark.parametrize("storage,Q", [("f32", 1), ("bf16", 2), ("f32", 6), ("bf16", 40), ("f32", 70), ("f32+filter", 300),
                                       ("bf16+filter", 300)])
def test_scarcity(torch_cuda, storage, Q):
    """Fewer admissible rows than k: -1 / 0.0 pads after them.  5, 7, 0 and 12 admissible rows - and an open query
    beside them that is not touched."""
    P, q = small_catalog(384)
    member = standard_sets()
    cases = [([FIVE], 5), ([TWELVE, SEVEN], 7), ([FIVE, SEVEN], 0), ([TWELVE], 12), ([-1], 20), ([N_SETS + 3], 0)]
    ids = rowset_ids([cases[i % len(cases)][0] for i in range(Q)], Q, 2)
    ix = index_with_sets(P, member, storage)
    idx, sc = check_in_sets(ix, q[:Q], P, 20, member, ids)
    for i in range(Q):
        n_real = cases[i % len(cases)][1]
        assert (idx[i, :n_real] >= 0).all() and (idx[i, n_real:] == -1).all() and (sc[i, n_real:] == 0.0).all()
    plain = ix.search(q[:Q], 20)
    for i in range(4, Q, len(cases)):
        np.testing.assert_array_equal(plain[0][i].cpu().numpy(), idx[i])
        np.testing.assert_array_equal(plain[1][i].cpu().numpy(), sc[i])
    ix.close()


# ---------------------------------------------------------------- identities
@pytest.mark.parametrize("storage", ["f32", "bf16", "f32+filter", "bf16+filter"])
def test_open_slots_and_full_sets_are_the_plain_search(torch_cuda, storage):
    """sets=None, all -1 ids and a full set give ix.search's bits, with and without exclusions and masks, with a row
    offset of 1,000,000; 1 .. 4 slots per query with padding -1 slots give equal results."""
    P, q = small_catalog(384)
    member, F = standard_sets(), facets()
    rng = np.random.default_rng(3)
    ix = index_with_sets(P, member, storage, F, row_offset=1_000_000)
    for Q in (1, 50, 300):
        excl = sorted_exclusions(rng, N, Q)
        masks = facet_masks(mixed_allow(rng, F, Q), Q, 2, ix.device)
        for ex, al in ((None, None), (excl, None), (excl, masks)):
            plain = ix.search(q[:Q], 20, ex, allow=al)
            assert int(plain[0].max()) >= 1_000_000
            open_ids = dev(rowset_ids([None] * Q, Q, 3), ix)
            full_ids = dev(rowset_ids([[FULL, -1, FULL]] * Q, Q), ix)
            for got in (ix.search(q[:Q], 20, ex, allow=al, sets=None), ix.search(q[:Q], 20, ex, allow=al, sets=open_ids),
                        ix.search(q[:Q], 20, ex, allow=al, sets=full_ids)):
                assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        within = [[HALF] if i % 3 else [ONEPCT] for i in range(Q)]
        first = ix.search(q[:Q], 20, excl, sets=dev(rowset_ids(within, Q, 1), ix))
        for m in (2, 3, 4):
            got = ix.search(q[:Q], 20, excl, sets=dev(rowset_ids(within, Q, m), ix))
            assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
        check_in_sets(ix, q[:Q], P, 20, member, rowset_ids(within, Q, 1), excl)
    ix.close()


def test_rowsets_set_replaced_written_and_removed(torch_cuda):
    P, q = small_catalog(64)
    member = standard_sets()
    ix = DeviceIndex(P)
    ids = dev(rowset_ids([[HALF], [ONEPCT], None], 3), ix)
    with pytest.raises(_native.IcrecError, match=r"status -1"):     # never had sets
        ix.search(q[:3], 20, sets=ids)
    W = (N + 31) // 32
    with pytest.raises(_native.IcrecError, match=r"status -1"):
        ix.write_rowset(0, np.zeros(W, np.uint32))
    ix.set_rowsets(rowset_bits(member, N))
    want = check_in_sets(ix, q[:3], P, 20, member, ids.cpu().numpy())
    lib = _native.lib()
    one = np.zeros(W, np.uint32)
    for bad in (0, 65536, -1):                                       # refused ...
        assert lib.icrec_index_set_rowsets(ix._h, one.ctypes.data, bad) == -1
        assert ix.n_rowsets == N_SETS
    assert_search(ix.search(q[:3], 20, sets=ids), want)             # ... and the previous sets stay in force
    for bad in (-1, N_SETS):
        with pytest.raises(_native.IcrecError, match=r"status -1"):
            ix.write_rowset(bad, one)
    with pytest.raises(_native.IcrecError, match=r"status -1"):     # sets_per_query = 5
        lib_ids = torch.full((3, 5), -1, dtype=torch.int32, device=ix.device)
        idx = torch.empty((3, 20), dtype=torch.int64, device=ix.device)
        sc = torch.empty((3, 20), dtype=torch.float32, device=ix.device)
        ws = ix._workspace(3, 20)
        _native.check(lib.icrec_search_in_sets(ix._h, _native.ptr(torch.from_numpy(q[:3].copy()).to(ix.device)), 3, 20, None,
                                               None, None, _native.ptr(lib_ids), 5, _native.ptr(idx), _native.ptr(sc),
                                               _native.ptr(ws), ws.numel(), _native.stream_ptr(ix.device)), "icrec_search_in_sets")
    # write_rowset: only that set's queries change; bits past n_rows in the last word are ignored
    changed = member.copy()
    changed[HALF] = ~member[HALF]
    bits = rowset_bits(changed[HALF:HALF + 1], N)[0]
    bits[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(N % 32)
    ix.write_rowset(HALF, bits)
    got = check_in_sets(ix, q[:3], P, 20, changed, ids.cpu().numpy())
    assert not np.array_equal(got[0][0], want[0][0])
    np.testing.assert_array_equal(got[0][1:], want[0][1:])
    np.testing.assert_array_equal(got[1][1:], want[1][1:])
    # replaced by fewer sets: the new members decide, and an id the old sets had now admits nothing
    two = np.ascontiguousarray(member[[ONEPCT, HALF]])
    ix.set_rowsets(rowset_bits(two, N))
    assert ix.n_rowsets == 2
    out = check_in_sets(ix, q[:3], P, 20, two, np.asarray([[0], [1], [HALF]], np.int32))
    assert (out[0][2] == -1).all()
    ix.set_rowsets(None)
    assert ix.n_rowsets == 0
    with pytest.raises(_native.IcrecError, match=r"status -1"):
        ix.search(q[:3], 20, sets=ids)
    assert_search(ix.search(q[:4], 20), oracle.search(q[:4], P, 20))  # the plain search never looked at them
    assert lib.icrec_index_rowsets(None) == -1
    ix.close()


# ---------------------------------------------------------------- workspace and capture
@pytest.mark.parametrize("storage,Q", [("f32", 2), ("f32", 100), ("bf16+filter", 300)])
def test_workspace_contents_do_not_matter(torch_cuda, storage, Q):
    P, q = small_catalog(384)
    member = standard_sets()
    ix = index_with_sets(P, member, storage)
    lib = _native.lib()
    need = int(lib.icrec_search_in_sets_workspace_bytes(ix._h, Q, 20))
    assert need == int(lib.icrec_search_workspace_bytes(ix._h, Q, 20)) > 0
    assert lib.icrec_search_in_sets_workspace_bytes(ix._h, 0, 20) == 0 == lib.icrec_search_in_sets_workspace_bytes(ix._h, Q, 129)
    assert lib.icrec_search_in_sets_workspace_bytes(None, Q, 20) == 0
    ids = mixed_ids(Q)
    qd = torch.from_numpy(q[:Q].copy()).to(ix.device)
    outs = []
    for fill in (0, 0xFF):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=ix.device)
        idx = torch.empty((Q, 20), dtype=torch.int64, device=ix.device)
        sc = torch.empty((Q, 20), dtype=torch.float32, device=ix.device)
        ix.search_into(qd, 20, None, None, idx, sc, ws=ws, sets=dev(ids, ix))
        outs.append((idx, sc))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert_search(outs[0], check_in_sets(ix, q[:Q], P, 20, member, ids))
    ix.close()


def test_captured_graph_follows_the_id_buffer_and_a_rewritten_set(torch_cuda):
    """search_into(..., sets=ids) captured at Q = 1; the replay after the id buffer was rewritten in place returns the
    NEW ids' result, and the replay after write_rowset the new members': the kernels read both when they run."""
    P, q = small_catalog(384)
    member = standard_sets().copy()
    ix = index_with_sets(P, member, "f32")
    ids = dev(np.asarray([[HALF, -1]], np.int32), ix)
    qd = torch.from_numpy(q[:1].copy()).to(ix.device)
    idx = torch.empty((1, 20), dtype=torch.int64, device=ix.device)
    sc = torch.empty((1, 20), dtype=torch.float32, device=ix.device)
    ws = torch.empty(int(_native.lib().icrec_search_in_sets_workspace_bytes(ix._h, 1, 20)), dtype=torch.uint8, device=ix.device)
    ix.search_into(qd, 20, None, None, idx, sc, ws=ws, sets=ids)  # first launch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ix.search_into(qd, 20, None, None, idx, sc, ws=ws, sets=ids)
    idx.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    first = check_in_sets(ix, q[:1], P, 20, member, np.asarray([[HALF, -1]], np.int32))
    assert_search((idx, sc), first)
    ids.copy_(dev(np.asarray([[ONEPCT, HALF]], np.int32), ix))
    g.replay()
    torch.cuda.synchronize()
    second = check_in_sets(ix, q[:1], P, 20, member, np.asarray([[ONEPCT, HALF]], np.int32))
    assert_search((idx, sc), second)
    assert not np.array_equal(second[0], first[0])
    member[ONEPCT] = ~member[HALF] | member[TWELVE]
    torch.cuda.synchronize()
    ix.write_rowset(ONEPCT, rowset_bits(member[ONEPCT:ONEPCT + 1], N)[0])
    g.replay()
    torch.cuda.synchronize()
    third = check_in_sets(ix, q[:1], P, 20, member, np.asarray([[ONEPCT, HALF]], np.int32))
    assert_search((idx, sc), third)
    assert not np.array_equal(third[0], second[0])
    assert admitted_by_sets(member, [[ONEPCT, HALF]]).sum() == (member[TWELVE] & member[HALF]).sum()
    ix.close()
