"""The sorters of csrc/sort.hip at their lane, slot and segment edges, bit for bit against numpy: merge_block_kernel
through icrec_search (its eligibility edge, a ranking loop of several trips, pads), merge_kernel<4> / <16> through
icrec_merge_topk (63 .. 1,024 lists, empty lists, pad tails, rows near 2^32), and the bitonic ranking of icrec_rank_all
around its first global stage.  Every search case asserts which merge it runs (merge_form on the restated plan, the plan
pinned to the library's by its workspace size); every output has poisoned guard words behind it.  No tolerances."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import sorter_cases as sc
from tests.search_harness import (DeviceIndex, _native, assert_plan_is_the_librarys, assert_search,
                                  block_merge_candidates, full_ranking, merge_form, merge_reference, merge_topk, n_cu,
                                  oracle, search, search_plan)
from tests.search_harness import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
GUARD = 64  # guard words behind every output
ROW_OFFSET = sc.ROW_OFFSET


def poisoned(n, dtype):
    return torch.full((n + GUARD,), 7.0 if dtype == torch.float32 else POISON, dtype=dtype, device="cuda")


def assert_guards(buf, n):
    torch.cuda.synchronize()
    fill = 7.0 if buf.dtype == torch.float32 else POISON
    assert bool((buf[n:] == fill).all()), "a kernel wrote behind its output"


def guarded_search(ix, qd, k, excl):
    """ix.search on outputs with guard words behind them -> (idx [Q, k], score [Q, k]) device tensors."""
    Q = int(qd.shape[0])
    ei, eo = search.exclusion_csr(excl, Q, ix.device)
    idx, score = poisoned(Q * k, torch.int64), poisoned(Q * k, torch.float32)
    ix.search_into(qd, k, ei, eo, idx[:Q * k].view(Q, k), score[:Q * k].view(Q, k))
    assert_guards(idx, Q * k)
    assert_guards(score, Q * k)
    return idx[:Q * k].view(Q, k), score[:Q * k].view(Q, k)


def assert_runs(ix, Q, k, kernel, n_lists, form):
    """The search of Q queries at k on ix takes the kernel `kernel`, leaves n_lists lists per query and merges them
    with `form` - on THIS device's CU count - and the library cuts the rows the same way.  -> the plan."""
    plan = search_plan(ix.n_rows, Q, k, n_cu())
    assert (plan[0], plan[5]) == (kernel, n_lists), (plan, n_cu())
    assert_plan_is_the_librarys(ix, Q, k, plan)
    assert merge_form(n_lists, Q, k) == form, (n_lists, Q, k)
    return plan


# ---------------------------------------------------------------- merge_block_kernel and its edge, through icrec_search
@pytest.mark.parametrize("name", list(sc.SEARCH_CASES))
def test_search_merge_forms_vs_oracle(torch_cuda, name):
    """One crafted catalog of tests/sorter_cases.py at each of its query counts and list lengths: the merge form the case
    names (asserted), the number of keys merge_block_kernel has to rank (from the oracle's scores of the admissible
    rows: more than 256 means a second trip of its ranking loop, 513 and more a third), exclusion lists that take some
    of every query's very best rows but leave one query alone, and the result equal to the oracle's, indices and
    scores."""
    _, n, dim, storage, Qs, forms, kernel, n_lists, conditions, none_query = sc.SEARCH_CASES[name]
    P, q = sc.search_case_inputs(name)
    rows = oracle.normalize_rows(P)
    if storage == "bf16":
        rows = oracle.round_bf16(rows)
    S = oracle.scores(oracle.normalize_rows(q), rows)
    excl = sc.search_case_exclusions(name, S)
    assert excl[none_query] == []
    admissible = S.copy()
    for i, e in enumerate(excl):
        admissible[i, e] = -np.inf
    ix = DeviceIndex(P, storage=storage, row_offset=ROW_OFFSET)
    qd = torch.tensor(q).cuda()
    for Q in Qs:
        for k, form in forms.items():
            plan = assert_runs(ix, Q, k, kernel, n_lists, form)
            C = [block_merge_candidates(admissible[i], k, plan[1], plan[4]) for i in range(Q)]
            print(f"\n{name}: Q {Q}, k {k}, plan {plan}, {form}, keys to rank per query {C}")
            assert all(sc.holds(c, conditions.get(k)) for c in C), (C, conditions.get(k))
            got = guarded_search(ix, qd[:Q], k, excl[:Q])
            want = oracle.search(q[:Q], P, k, excl[:Q], row_offset=ROW_OFFSET, storage=storage)
            assert_search(got, want)
            if name == "edge-stream-257":   # the one row of list 256, the last list of the last lane slot in use
                assert int(got[0][0, 0]) == ROW_OFFSET + n - 1
    ix.close()


def test_search_block_merge_pads(torch_cuda):
    """merge_block_kernel where fewer than k rows are left: two lists of which 100 rows are admissible at k = 128 (100
    rows, then 28 pads (-1, 0.0)), a catalog of 5 rows at k = 20 for 4 queries, and a query whose exclusions empty the
    whole second tile of four - a list of pads between full lists."""
    rng = np.random.default_rng(41)
    # (rows, queries, k, kernel, lists, exclusion lists)
    keep = sorted(rng.choice(300, 100, replace=False).tolist())
    cases = [
        (300, 2, 128, "stream", 2, [sorted(set(range(300)) - set(keep)), []]),
        (5, 4, 20, "small", 1, [[], [], [1, 3], [0, 1, 2, 3, 4]]),
        (1000, 1, 20, "stream", 4, [list(range(256, 512)) + [7, 600]]),
        (1000, 2, 20, "stream", 4, [[5], list(range(250, 520))]),
    ]
    for n, Q, k, kernel, n_lists, excl in cases:
        P = rng.standard_normal((n, 32), dtype=np.float32)
        q = rng.standard_normal((Q, 32), dtype=np.float32)
        ix = DeviceIndex(P, row_offset=ROW_OFFSET)
        assert_runs(ix, Q, k, kernel, n_lists, "block")
        got = guarded_search(ix, torch.tensor(q).cuda(), k, excl)
        want = oracle.search(q, P, k, excl, row_offset=ROW_OFFSET)
        assert_search(got, want)
        left = [min(k, n - len(e)) for e in excl]
        assert n != 300 or left == [100, 128]
        for i in range(Q):   # the oracle's answer is the one meant: real rows, then (-1, 0.0)
            assert (want[0][i, :left[i]] >= ROW_OFFSET).all() and (want[0][i, left[i]:] == -1).all()
            assert (want[1][i, left[i]:].view(np.uint32) == 0).all()
        ix.close()


# ---------------------------------------------------------------- merge_kernel<4> / <16> through icrec_merge_topk
@pytest.mark.parametrize("n_lists,Q,k", [(n_lists, Q, k) for n_lists, pairs in sc.MERGE_SHAPES.items() for Q, k in pairs])
def test_merge_topk_vs_reference(torch_cuda, n_lists, Q, k):
    """icrec_merge_topk on crafted key lists, every content pattern of sorter_cases.merge_case_keys at every shape,
    against the plain descending sort of all of a query's keys."""
    assert merge_form(n_lists, Q, k, block=False) == ("wave4" if n_lists <= 256 else "wave16")
    for pattern in sc.MERGE_PATTERNS:
        keys = sc.merge_case_keys(pattern, n_lists, Q, k, seed=n_lists * 1000 + Q * 10 + len(pattern))
        want = merge_reference(keys, k)
        if pattern == "last-list":
            assert (want[0] // k == n_lists - 1).all()       # rows name their list
        if pattern == "short":
            assert (want[0][:, -1] == -1).all()
        got = merge_topk(torch.from_numpy(keys.view(np.int64)).cuda(), k)
        np.testing.assert_array_equal(got[0].cpu().numpy(), want[0], err_msg=pattern)
        np.testing.assert_array_equal(got[1].cpu().numpy().view(np.uint32), want[1].view(np.uint32), err_msg=pattern)


def test_merge_topk_refusals(torch_cuda):
    """n_lists of 0 and 1,025, k of 0 and 129, n_queries of 0: ICREC_EINVAL, and nothing is launched (the outputs keep
    their poison)."""
    L = _native.lib()
    keys = torch.zeros(1025 * 129, dtype=torch.int64, device="cuda")
    idx, score = poisoned(129, torch.int64), poisoned(129, torch.float32)
    for n_lists, Q, k in [(0, 1, 20), (1025, 1, 20), (4, 1, 0), (4, 1, 129), (4, 0, 20)]:
        rc = L.icrec_merge_topk(_native.ptr(keys), n_lists, Q, k, _native.ptr(idx), _native.ptr(score), 0,
                                _native.stream_ptr(keys.device))
        assert rc == -1, (n_lists, Q, k, rc)                 # ICREC_EINVAL (include/icrec.h)
    assert_guards(idx, 0)
    assert_guards(score, 0)


# ---------------------------------------------------------------- the bitonic ranking of icrec_rank_all
def guarded_rank_all(ix, qd):
    L = _native.lib()
    Q, n = int(qd.shape[0]), ix.n_rows
    ws = torch.empty(int(L.icrec_rank_all_workspace_bytes(ix._h, Q)), dtype=torch.uint8, device="cuda")
    out = poisoned(Q * n, torch.int64)
    _native.check(L.icrec_rank_all(ix._h, _native.ptr(qd), Q, _native.ptr(out), _native.ptr(ws), ws.numel(),
                                   _native.stream_ptr(ix.device)), "icrec_rank_all")
    assert_guards(out, Q * n)     # n rows per query, not the P keys of the sort
    return out[:Q * n].view(Q, n).cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 8191, 8193, 16384, 16385])
def test_rank_all_segment_edges(torch_cuda, n):
    """The complete ranking where the sort changes shape: one and two keys, one LDS segment with one pad (8,191), two
    segments and one global stage with 8,191 pads that all have to end behind the real keys (8,193) or none (16,384),
    four segments (16,385).  Rows 3, 17 and n - 1 are one row: equal scores, the row decides."""
    rng = np.random.default_rng(n)
    P = rng.standard_normal((n, 32), dtype=np.float32)
    if n > 17:
        P[[3, 17, n - 1]] = P[3]
    q = rng.standard_normal((2, 32), dtype=np.float32)
    S = oracle.scores(oracle.normalize_rows(q), oracle.normalize_rows(P))
    ix = DeviceIndex(P, row_offset=ROW_OFFSET)
    got = guarded_rank_all(ix, torch.tensor(q).cuda())
    ix.close()
    for i in range(2):
        np.testing.assert_array_equal(got[i], ROW_OFFSET + full_ranking(S[i]))
        if n > 17:
            at = [int(np.flatnonzero(got[i] == ROW_OFFSET + r)[0]) for r in (3, 17, n - 1)]
            assert at[1] == at[0] + 1 and at[2] == at[0] + 2


def test_rank_all_equal_scores_across_segments(torch_cuda):
    """16,385 copies of one row: every score of a query is the same, so only the low 32 key bits order the keys, within
    and across the four LDS segments, and the 16,383 pads stay behind all of them."""
    n = 16385
    rng = np.random.default_rng(9)
    P = np.repeat(rng.standard_normal((1, 32), dtype=np.float32), n, axis=0)
    q = rng.standard_normal((2, 32), dtype=np.float32)
    S = oracle.scores(oracle.normalize_rows(q), oracle.normalize_rows(P))
    assert (S == S[:, :1]).all()
    ix = DeviceIndex(P, row_offset=ROW_OFFSET)
    got = guarded_rank_all(ix, torch.tensor(q).cuda())
    ix.close()
    for i in range(2):
        np.testing.assert_array_equal(got[i], ROW_OFFSET + np.arange(n))
