"""The tiled search kernels where a block walks several row tiles: the WARM regime of TopK::offer (threshold = k-th
key, candidate queues of 16 or 64 slots, deferred merges, overflow into the next merge iteration, the forced merge at
the block's last tile) under every tile variant, merge_queue (with and without the e1 half of the list) and
merge_queue2, fp32 and bf16 rows, and the guarded exact pass behind a filter pass.  Every catalog is sized from the
CU count so that each block has at least 3 tiles and the last tile is ragged; every result is checked bit for bit:
a sample of queries against the oracle, ALL queries against the selection of tests.search_harness.select_from_scores
on the device's own score matrix (the EMIT arm, which does not touch the selection and is itself checked against the
oracle on the sample).  No tolerances."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests.search_harness import (DeviceIndex, assert_plan_is_the_librarys, assert_search, direction_catalog,
                                  first_pass_offers, merge_topk, n_cu, oracle, select_from_scores, tie_run_catalog,
                                  tiled_plan, timed, warm_tile_beaters)
from tests.search_harness import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ORACLE_FMAS = 2_000_000_000   # per oracle call, as in test_search_dims_gpu
ROW_OFFSET = 1000
MAX_Q = 1024
# arm: (queries, the k values, row width, tile variant, slots of a query's candidate queue, tie run length > every k)
ARMS = {
    "big-merge2":   (1024, (1, 32), 384, "big", 16, 41),     # CfgBig, merge_queue2
    "mid-merge":    (1024, (33, 64), 384, "mid", 16, 137),   # CfgMid, merge_queue without the e1 half
    "small-e1":     (512, (65, 128), 384, "small", 64, 137),  # CfgSmall, merge_queue with e1, 64-slot queues
    "mid-merge2":   (64, (20,), 64, "mid", 16, 41),          # CfgMid, merge_queue2; one query tile: chunk count at its cap
    "small-k32":    (32, (32,), 64, "small", 64, 41),        # CfgSmall, k <= 32 (64-slot queues: merge_queue)
}
ORDERS = ["random", "ascending", "descending", "ties"]


def arm_shape(Q, k, variant):
    """(n_rows, plan) for a batch of Q queries at list length k: the smallest catalog of about 3 tiles per block whose
    plan has at least 3 tiles in every block but possibly the last, at least 2 in the last (so the ragged last tile is
    a WARM tile), and a last tile of BM - 27 rows.  plan = tiled_plan's tuple."""
    _, BM, BN, n_qtiles, _, _ = tiled_plan(1, Q, k, n_cu())
    want = min(max(2 * n_cu() // n_qtiles, 1), 256)
    n_tiles = 3 * want + 2
    while True:
        n = (n_tiles - 1) * BM + BM - 27
        plan = tiled_plan(n, Q, k, n_cu())
        tpc, n_chunks = plan[4], plan[5]
        if n_tiles - (n_chunks - 1) * tpc >= 2:
            break
        n_tiles += 1
    # the preconditions of every case, before anything runs on the device
    assert plan[0] == variant, (plan, variant)
    assert tpc >= 3, plan
    assert n % BM not in (0, BM - 1) and (n + BM - 1) // BM == n_tiles
    assert n_chunks >= 5 and n + ROW_OFFSET < 2 ** 31
    return n, plan


@functools.lru_cache(maxsize=None)
def catalog(order, n, dim, BM, tpc, run_len):
    """One catalog with MAX_Q queries per (ordering, shape) and module run; arms of one shape share it and take the
    first Q queries -> (P, q, runs, near, stray); runs and near are empty and
    stray is None off "ties"."""
    seed = ORDERS.index(order) * 1000 + dim
    if order == "ties":
        return tie_run_catalog(n, dim, MAX_Q, BM, tpc, run_len, seed)
    if order == "random":   # independent rows and queries: every query has a ranking of its own
        rng = np.random.default_rng(seed)
        P, q = rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((MAX_Q, dim), dtype=np.float32)
        P.flags.writeable = q.flags.writeable = False
    else:
        P, q = direction_catalog(order, n, dim, MAX_Q, seed)
    return P, q, [], np.zeros(0, np.int64), None


def query_sample(Q, BN, rng):
    """24 queries (fewer for a batch of 32): the first and last query of the first and last query tile, one of an
    interior tile if there is one, queries 2, 5 and 8 (which exclude whole tie runs or the head of one), the rest
    random - but never query 1, whose list under "descending" breaks that ordering's condition on purpose."""
    n_qtiles = (Q + BN - 1) // BN
    last0 = (n_qtiles - 1) * BN
    must = {0, min(BN, Q) - 1, last0, Q - 1, 2, 5, 8}
    if n_qtiles > 2:
        must.add((n_qtiles // 2) * BN + BN // 2)
    rest = [i for i in rng.permutation(Q).tolist() if i not in must and i != 1]
    return sorted(must | set(rest[: 24 - len(must)]))


def exclusion_lists(top8, runs, n, rng):
    """Two thirds of the queries (i % 3 != 0) exclude their own best, third and sixth row and 10 random rows; under
    "ties" query 2, 14, 26, ... also excludes the whole of run 0, query 5, 17, 29, ... runs 0 and 1, and query 8, 20,
    32, ... all but the last 10 copies of run 0: 3 in the block's cold tile, 7 in its second tile, which a warm tile
    then has to take on a score equal to copies already listed.  -> (lists, the excluded true top rows of all
    queries)."""
    excl, top_rows = [], []
    for i in range(top8.shape[0]):
        if i % 3 == 0:
            excl.append([])
            continue
        mine = top8[i, [0, 2, 5]].tolist()
        top_rows.extend(mine)
        e = set(mine) | set(rng.choice(n, 10, replace=False).tolist())
        if runs and i % 12 in (2, 5):
            e |= set(range(*runs[0]))
        if runs and i % 12 == 5:
            e |= set(range(*runs[1]))
        if runs and i % 12 == 8:
            e |= set(range(runs[0][0], runs[0][1] - 10))
        excl.append(sorted(e))
    return excl, np.asarray(top_rows)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("arm", list(ARMS))
def test_warm_tiles_vs_oracle_and_score_matrix(torch_cuda, arm, order, storage):
    """One arm of the selection (ARMS) under one ordering of the catalog, at each k of the arm.
    random:     independent normal rows and queries, every query with a ranking of its own; most warm tiles offer a few
                candidates, which wait in the queues for a trigger or for the forced merge at the block's last tile.
    ascending:  every query's score grows with the row: in every warm tile of every block at least 2 * qcap rows beat
                the k-th best of the block's earlier rows (asserted from the oracle's scores of the sample), so every
                warm tile floods the queues and the overflow loop iterates.
    descending: the first tile of a block holds its whole answer: NO row of a later tile beats the block's k-th best
                (asserted likewise); later tiles must offer nothing and lose nothing.
    ties:       three runs of one duplicated row, each longer than k, across a tile boundary inside a block, across a
                block boundary and inside the ragged last tile, plus near rows and one stray copy that only the cold
                tile's second pass can pick up: row order decides (tie_run_catalog).
    Exclusions: two thirds of the queries exclude some of their own best rows (exclusion_lists); outside "descending"
    at least one of these lies in a warm tile.  Under "descending" every best row lies in a block's first tile - that
    is what the ordering means - so there the same assertion is made the other way round, and query 1 (never sampled)
    excludes most of the catalog's first tile instead: its list is still short when block 0 reaches its second tile,
    whose first 4 rows it excludes too - rows that an exclusion ignored in a later tile would put into its answer."""
    Q, ks, dim, variant, qcap, run_len = ARMS[arm]
    n, plan = arm_shape(Q, ks[0], variant)
    _, BM, BN, n_qtiles, tpc, n_chunks = plan
    for k in ks:
        assert arm_shape(Q, k, variant) == (n, plan)   # one catalog, one plan for the arm's k values
        assert k <= run_len - 7                        # the copies of run 0 in the cold tile (tie_run_catalog)
    P, q, runs, near, stray = catalog(order, n, dim, BM, tpc, run_len)
    q = q[:Q]
    rng = np.random.default_rng(len(arm) + 10 * ORDERS.index(order))
    sample = query_sample(Q, BN, rng)
    assert len(sample) * n * dim <= ORACLE_FMAS
    print(f"\n{arm} {order} {storage}: n_cu {n_cu()}, {n} rows x {dim}, {Q} queries, plan {plan}, "
          f"{n - (n_chunks - 1) * tpc * BM} rows in the last block, sample of {len(sample)}")

    rows = oracle.normalize_rows(P)
    if storage == "bf16":
        rows = oracle.round_bf16(rows)
    ref = oracle.scores(oracle.normalize_rows(q[sample]), rows)       # [sample, n], the oracle's chains
    ix = DeviceIndex(P, storage=storage, row_offset=ROW_OFFSET)
    for k in ks:
        assert_plan_is_the_librarys(ix, Q, k, plan)
    qd = torch.tensor(q).cuda()
    S = ix.scores(qd).cpu().numpy()                                   # the EMIT arm: no selection involved
    np.testing.assert_array_equal(S[sample], ref)

    # exclusions from the true top rows: the oracle's on the sample, the score matrix's on the rest
    top8 = select_from_scores(S, 8)[0]
    top8[sample] = oracle.search(q[sample], P, 8, storage=storage)[0]
    excl, top_rows = exclusion_lists(top8, runs, n, rng)
    warm = (top_rows // BM) % tpc != 0
    if order == "descending":
        assert not warm.any()
        later = set(range(BM, BM + 4))
        excl[1] = sorted(set(excl[1]) | set(range(BM - max(min(ks) - 4, 0))) | later)
        for k in ks:   # without the 4 rows of the second tile, some of them are in the answer
            ignored = select_from_scores(S[1:2], k, [sorted(set(excl[1]) - later)])[0]
            assert np.isin(ignored, sorted(later)).any()
    else:
        assert warm.any()
    if order == "ties":
        assert any(set(range(*runs[0])) <= set(excl[i]) for i in sample)
        (a0, b0), (a1, b1), (a2, b2) = runs
        assert a0 // BM + 1 == (b0 - 1) // BM and a0 // (BM * tpc) == (b0 - 1) // (BM * tpc)      # tile boundary in a block
        assert a1 // (BM * tpc) + 1 == (b1 - 1) // (BM * tpc)                                      # block boundary
        assert a2 // BM == (b2 - 1) // BM == (n - 1) // BM and (a2 // BM) % tpc != 0               # ragged, warm tile

    admissible = ref.copy()
    for j, i in enumerate(sample):
        admissible[j, excl[i]] = -np.inf
    sample_excl = [excl[i] for i in sample]
    for k in ks:
        if order in ("ascending", "descending"):
            counts, exists = warm_tile_beaters(admissible, k, BM, tpc)
            counts = counts[:, exists]
            print(f"k {k}: rows of a warm tile above the block's k-th best so far: {counts.min()} .. {counts.max()}")
            if order == "ascending":
                assert counts.min() >= 2 * qcap, (counts.min(), qcap)
            else:
                assert counts.max() == 0, counts.max()
        if order == "ties" and k > 1:
            # the stray copy in block 1's cold tile, from the oracle's scores: its lane does not offer it in the first
            # pass, and the k-th best of what the first pass does offer is another copy (same score, higher row) - the
            # stray then enters in the second pass on a score EQUAL to the threshold's, ahead of every other copy
            cold = slice(tpc * BM, tpc * BM + BM)
            assert stray == cold.start + 17
            equal = 0
            for j in range(len(sample)):
                offered = first_pass_offers(ref[j, cold], k, BM) & np.isfinite(admissible[j, cold])
                best = np.sort(admissible[j, cold][offered])[::-1]
                equal += bool(not offered[17] and np.isfinite(admissible[j, stray]) and best.size >= k
                              and best[k - 1] == ref[j, stray])
            print(f"k {k}: the stray copy equals the threshold of the second pass for {equal} of {len(sample)} sampled queries")
            assert equal >= len(sample) // 2
        idx, sc = ix.search(qd, k, excl)
        want = select_from_scores(S, k, excl, ROW_OFFSET)
        assert_search((idx, sc), want)
        assert_search(merge_topk(ix.search_partial(qd, k, excl).unsqueeze(0), k), want)
        assert_search((idx[sample], sc[sample]),
                      oracle.search(q[sample], P, k, sample_excl, row_offset=ROW_OFFSET, storage=storage))
    ix.close()


@pytest.mark.parametrize("base", ["f32", "bf16"])
def test_guarded_exact_pass_over_several_tiles(torch_cuda, base):
    """The tie-run catalog of the CfgBig arm behind a filter pass, 1,024 queries, k = 20: the runs are longer than the
    filter's candidate lists (k + 12), so the verify pass cannot prove these queries and the exact pass runs with its
    run flag set - over blocks of several tiles.  Equal to the plain index on all queries and to the oracle on the
    sample; timer slot 4 records one launch whose time is a multiple of what the same storage's slot 4 takes on the
    random catalog of the same shape, where the verify pass proves every list and the guarded pass exits at once."""
    Q, _, dim, variant, _, run_len = ARMS["big-merge2"]
    k = 20
    n, plan = arm_shape(Q, k, variant)
    _, BM, BN, _, tpc, _ = plan
    assert arm_shape(Q, ARMS["big-merge2"][1][0], variant) == (n, plan) and k < run_len   # the arm's own catalogs
    rng = np.random.default_rng(5)
    sample = query_sample(Q, BN, rng)
    fb = {}
    for order in ("random", "ties"):
        P, q, runs, _, _ = catalog(order, n, dim, BM, tpc, run_len)
        qd = torch.tensor(q).cuda()
        plain = DeviceIndex(P, storage=base, row_offset=ROW_OFFSET)
        # inputs only: which rows to exclude (the lists are checked against the oracle below, whatever they hold)
        excl, _ = exclusion_lists(plain.search(qd, 8)[0].cpu().numpy() - ROW_OFFSET, runs, n, rng)
        pi, ps = plain.search(qd, k, excl)
        plain.close()
        fx = DeviceIndex(P, storage=base + "+filter", row_offset=ROW_OFFSET)
        fx.search(qd, k, excl)                                         # first launches out of the timed region
        (fi, fs), t = timed(lambda: fx.search(qd, k, excl))
        fx.close()
        assert torch.equal(fi, pi) and torch.equal(fs, ps)
        assert_search((fi[sample], fs[sample]), oracle.search(q[sample], P, k, [excl[i] for i in sample],
                                                              row_offset=ROW_OFFSET, storage=base))
        fb[order], n_fb = t[4]
        assert n_fb == 1
    print(f"\nguarded exact pass, {base}, plan {plan}: {fb['ties']:.4f} ms on the tie runs, {fb['random']:.4f} ms on "
          f"the random catalog")
    assert fb["ties"] > 3 * fb["random"], fb
