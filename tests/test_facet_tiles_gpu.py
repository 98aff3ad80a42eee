"""The FACET arms of the selecting kernels where a block walks several row tiles: the hand-over of the facet words from
tile to tile through the two halves of TopK::ftile (blocks with odd and even tile counts, the ragged last tile as a warm
tile), warm lanes that test each candidate's row against the masks while the queues flood, queries that turn warm in the
middle of a block's walk or stay cold to its end, equal scores of which only some copies are admitted, under every tile
variant and both merges, fp32 and bf16 rows - and the filter storages over several rounds per block: resident and staged
pass, 32- and 16-slot queues, the guarded exact pass under masks, blocks of more than RES_QCAP_MAX_ROUNDS rounds and the
LDS edge of the faceted resident pass.  Catalogs, plans and exclusions are those of tests/test_search_tiles_gpu.py (sized
from the CU count); every result is checked bit for bit: ALL queries against select_from_scores on the device's own
score matrix with the admitted rows as a bool matrix (or, for a filter storage, against the plain storage's faceted
search), a sample against the oracle with the exclusions united with every rejected row.  No tolerances."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd.search import exclusion_csr, facet_masks
from tests.search_harness import (FILTER_MIN_Q, LDS_MAX, RES_QCAP_MAX_ROUNDS, DeviceIndex, _native, admitted_matrix,
                                  admitted_per_tile, assert_search, direction_catalog, filter_list_len, filter_plan, n_cu,
                                  oracle, resident_lds, select_from_scores, tiled_plan, timed, warm_tile_beaters)
from tests.search_harness import torch_cuda  # noqa: F401  (fixture)
from tests.test_search_tiles_gpu import (ARMS, ORACLE_FMAS, ROW_OFFSET, arm_shape, catalog, exclusion_lists,
                                         query_sample)

pytestmark = pytest.mark.gpu

N_AISLES, N_DEPTS = 134, 21
LAST_TILE, THIRD_TILE = 200, 201          # aisle values: on the rows of the ragged last tile; on 5 rows of each block's third tile
EVERY_THIRD = list(range(0, N_AISLES, 3))
KINDS = "abcdefgh"                        # the mask kinds (kind_allow); kind_of deals them to the queries
LANE_PAIRS = [(i, i + 32) for i in range(8)]   # (q, q + 32): the two queries of one lane at TN = 2, one pair per kind pair
TIE_RUN = {"big-merge2": 71, "small-k32": 137}  # tie runs longer than the plain test's: half a run is more than k
MOST = 0.9                                # the share of blocks (or warm tiles) a statistical precondition must hold in


# ---------------------------------------------------------------- facets and masks, against the blocks a kernel walks
@functools.lru_cache(maxsize=None)
def tile_facets(n, BM, tpc, runs=()):
    """uint8 [n, 2], read-only: aisle uniform over 134 values and department over 21 (seed 5); aisle LAST_TILE on every
    row of the ragged last tile, THIRD_TILE on 5 rows of the third tile of every block of tpc tiles of BM rows (not in
    the last tile).  runs (the tie catalog's): the copies of each run alternate between aisle 0, which EVERY_THIRD
    admits, and aisle 1, which it rejects."""
    rng = np.random.default_rng(5)
    F = np.stack([rng.integers(0, N_AISLES, n), rng.integers(0, N_DEPTS, n)], axis=1).astype(np.uint8)
    n_tiles = (n + BM - 1) // BM
    F[(n_tiles - 1) * BM:, 0] = LAST_TILE
    for t in range(2, n_tiles - 1, tpc):
        F[t * BM + rng.choice(BM, 5, replace=False), 0] = THIRD_TILE
    third = F[:, 0] == THIRD_TILE
    for lo, hi in runs:
        F[lo:hi:2, 0] = 0
        F[lo + 1:hi:2, 0] = 1
    F[third, 0] = THIRD_TILE
    F.flags.writeable = False
    return F


def rare_aisles(F, block, count=8):
    """The `count` aisles from 2 on (0 and 1 mark the tie runs) whose fullest block of `block` rows holds the fewest of
    their rows: under a mask of one of them every block stays cold to its end."""
    n = F.shape[0]
    n_blocks = (n + block - 1) // block
    per = np.bincount(F[:, 0].astype(np.int64) * n_blocks + np.arange(n) // block, minlength=256 * n_blocks)
    fullest = per.reshape(256, n_blocks)[2:N_AISLES].max(axis=1)
    return (2 + np.argsort(fullest, kind="stable")[:count]).tolist()


def first_departments(F, BM, tpc, k):
    """The smallest m for which, under a mask of departments 0 .. m - 1, MOST blocks hold fewer than k admitted rows in
    their first tile and at least k in their first tpc - 1 tiles: cold at first, warm before the walk ends."""
    for m in range(1, N_DEPTS):
        per = admitted_per_tile(F[:, 1] < m, BM, tpc)
        if ((per[:, 0] < k) & (per[:, :tpc - 1].sum(axis=1) >= k)).mean() >= MOST:
            return m
    raise AssertionError(f"no department count turns a query warm in mid-walk at k = {k}, tiles of {BM} rows")


def kind_of(i, kinds=KINDS):
    """Query i's mask kind.  The kinds cycle by query, shifted by one for every 32 queries: where a lane holds two
    queries (TN = 2: CfgBig, CfgMid, CfgRes; TopK::myq, q and q + 32 of one 64-query span) they are of neighbouring
    kinds - a beside b, ..., d (open, warm) beside e (nothing, cold for ever), h beside a - and every query tile mixes
    all kinds.  (A plain i % 8 would give both queries of every lane the same kind.)"""
    return kinds[(i + i // 32) % len(kinds)]


def first_of(kind, kinds=KINDS):
    return next(i for i in range(32) if kind_of(i, kinds) == kind)


def kind_allow(i, rare, m, n_facets=2, kinds=KINDS):
    """Query i's constraint (facet_masks' input).  a: one rare aisle; b: the first m departments; c: every third aisle
    and all departments; d: open; e: nothing; f: the ragged last tile's aisle; g: the third tiles' aisle; h: the
    bit-position edges of both facets.  A one-facet index keeps the aisle entry only."""
    c = {"a": [[rare[(i // 8) % len(rare)]], None], "b": [None, list(range(m))], "c": [EVERY_THIRD, list(range(N_DEPTS))],
         "d": None, "e": [[], []], "f": [[LAST_TILE], None], "g": [[THIRD_TILE], None],
         "h": [[255, 0, 32], [31, 255, 1]]}[kind_of(i, kinds)]
    return c if c is None else c[:n_facets]


def one_cold_one_warm(adm_a, adm_b, BM, tpc, k):
    """adm_a[p], adm_b[p]: the admissible rows (bool [n]) of the two queries of lane pair p -> bool [pairs]: at the
    start of the second or third tile of some block (but the last, which may be short) one of them has fewer than k
    admissible rows of the block behind it - its list is not full, it is cold - and the other at least k: warm.  The
    lane then builds TopK::admitted for the cold query and filters the warm query's candidates through the same map."""
    cold = [np.cumsum(admitted_per_tile(a, BM, tpc), axis=-1)[:, :-1, :2] < k for a in (adm_a, adm_b)]
    return (cold[0] != cold[1]).any(axis=(1, 2))


def assert_mixed_lanes(adm_of, BM, tpc, ks, what):
    """adm_of(q) -> query q's admissible rows, exclusions taken out.  For every k some pair of LANE_PAIRS has one cold
    and one warm query in mid-walk, the pair (d, e) always."""
    a = np.stack([adm_of(q) for q, _ in LANE_PAIRS])
    b = np.stack([adm_of(q) for _, q in LANE_PAIRS])
    for k in ks:
        mixed = one_cold_one_warm(a, b, BM, tpc, k)
        print(f"{what} k {k}: lanes with one cold and one warm query in mid-walk, by kind pair: "
              f"{[kind_of(p) + kind_of(q) for (p, q), ok in zip(LANE_PAIRS, mixed) if ok]}")
        assert mixed[first_of("d")], (k, mixed)


def faceted_inputs(F, Q, BM, tpc, ks, check="abcfg", kinds=KINDS):
    """-> (allow, masks uint32 [Q, n_facets, 8]) for Q queries over facets F, and the preconditions of the kinds named
    in `check`, asserted from the inputs before anything runs on the device (ks: the list lengths; blocks of tpc tiles
    of BM rows).  a: in EVERY block fewer admitted rows than the largest k - cold for the whole walk.  b: in MOST
    blocks cold in the first tile, warm before the last (first_departments; two facets only).  c: in MOST blocks at
    least k admitted rows in the first tile, for every k a third of a tile can reach.  f: every admitted row lies in the
    last tile, which is ragged and not its block's first.  g: only third tiles hold admitted rows, 5 each."""
    n, n_facets = F.shape
    kmax = max(ks)
    rare = rare_aisles(F, BM * tpc)
    m = first_departments(F, BM, tpc, kmax) if n_facets == 2 and "b" in check else 1
    allow = [kind_allow(i, rare, m, n_facets, kinds) for i in range(Q)]
    masks = facet_masks(allow, Q, n_facets)
    n_tiles = (n + BM - 1) // BM
    # one query per kind; of kind a, whose queries take the rare aisles in turn, those among the first 64
    one = {kd: admitted_matrix(F, masks[[i for i in range(min(Q, 64)) if kind_of(i, kinds) == kd][:None if kd == "a" else 1]])
           for kd in kinds}
    if "a" in check:
        for row in one["a"]:
            assert admitted_per_tile(row, BM, tpc).sum(axis=1).max() < kmax
    if "c" in check:
        first = admitted_per_tile(one["c"][0], BM, tpc)[:, 0]
        for k in ks:
            if 3 * k <= BM:
                assert (first >= k).mean() >= MOST, (k, first)
    if "f" in check:
        rows = np.flatnonzero(one["f"][0])
        assert rows.size and rows.min() >= (n_tiles - 1) * BM and n % BM and (n_tiles - 1) % tpc != 0
    if "g" in check:
        per = admitted_per_tile(one["g"][0], BM, tpc)
        assert per[:, [j for j in range(tpc) if j != 2]].sum() == 0
        assert (per[:-1, 2] == 5).all() and per[-1, 2] in (0, 5)
    assert one["d"].all() and (kinds != KINDS or (not one["e"].any() and one["h"].any()))
    print(f"masks: kinds {kinds}, rare aisles {rare}, first {m} departments")
    return allow, masks


def usable_exclusions(top8, runs, n, rng):
    """exclusion_lists on a faceted top-8, whose lists may end in -1 pads: the pads are not rows."""
    excl, top_rows = exclusion_lists(top8, runs, n, rng)
    return [[r for r in e if r >= 0] for e in excl], top_rows[top_rows >= 0]


def union_lists(admit_rows, excl, queries):
    """Per query of `queries` its exclusions united with every row its masks reject (admit_rows: their rows of the
    admitted matrix): what the oracle excludes."""
    return [np.union1d(np.flatnonzero(~a), np.asarray(excl[i], np.int64)) for a, i in zip(admit_rows, queries)]


# ---------------------------------------------------------------- the exact tiled kernels
CASES = [(arm, order, "f32") for arm in ARMS for order in ("random", "ascending", "ties")] + \
        [(arm, order, "bf16") for arm in ("big-merge2", "small-e1") for order in ("random", "ascending", "ties")]


def run_tiled_case(arm, order, storage, n_facets=2, kinds=KINDS):
    Qa, ks, dim, variant, qcap, run_len = ARMS[arm]
    run_len = TIE_RUN.get(arm, run_len)
    Q = Qa - 3                                             # the last query tile is partial: padding queries, zero masks
    n, plan = arm_shape(Q, ks[0], variant)
    _, BM, BN, n_qtiles, tpc, n_chunks = plan
    assert Q % BN and (n, plan) == arm_shape(Qa, ks[0], variant)   # the plain test's catalog and plan
    for k in ks:
        assert arm_shape(Q, k, variant) == (n, plan) and k <= run_len - 7
    P, q, runs, _, stray = catalog(order, n, dim, BM, tpc, run_len)
    q = q[:Q]
    F = np.ascontiguousarray(tile_facets(n, BM, tpc, tuple(runs))[:, :n_facets])
    rng = np.random.default_rng(len(arm) + 10 * len(order) + n_facets)
    sample = set(query_sample(Q, BN, rng))
    if n > 100_000:            # the host's share: a list of up to n rejected rows per sampled query; the device shape stays
        sample = set(sorted(sample)[::2]) | {0, Q - 1}
    lanes = BN >= 64           # TN = 2: the pairs of LANE_PAIRS share their lanes (CfgSmall holds one query per lane)
    sample = sorted(sample | {2, 3} | ({q for pair in LANE_PAIRS for q in pair} if lanes else set()))
    assert len(sample) * n * dim <= ORACLE_FMAS and {kind_of(i, kinds) for i in sample} >= set("cd")
    print(f"\n{arm} {order} {storage} {n_facets} facet(s): n_cu {n_cu()}, {n} rows x {dim}, {Q} queries, plan {plan}, "
          f"{n - (n_chunks - 1) * tpc * BM} rows in the last block, sample of {len(sample)}")
    allow, masks = faceted_inputs(F, Q, BM, tpc, ks, "c" if kinds != KINDS else "abcfg" if n_facets == 2 else "acfg", kinds)
    admit = admitted_matrix(F, masks)
    if kinds != KINDS:
        # no query that stays cold: in MOST blocks every query's list is full after two tiles (13 rows to spare for its
        # exclusions; a third of one tile of 128 is about 43 rows), so the block is warm from its third tile on - one
        # pass per tile, merges on their triggers
        two = admitted_per_tile(admit[[first_of(kd, kinds) for kd in kinds]], BM, tpc)[:, :, :2].sum(axis=2)
        assert tpc >= 3 and ((two >= max(ks) + 13).all(axis=0)).mean() >= MOST, two

    rows = oracle.normalize_rows(P)
    if storage == "bf16":
        rows = oracle.round_bf16(rows)
    ref = oracle.scores(oracle.normalize_rows(q[sample]), rows)
    ix = DeviceIndex(P, storage=storage, row_offset=ROW_OFFSET)
    ix.set_facets(F)
    assert ix.n_facets == n_facets
    qd = torch.tensor(q).cuda()
    dm = facet_masks(allow, Q, n_facets, ix.device)
    S = ix.scores(qd).cpu().numpy()                        # the EMIT arm: no selection, no facets
    np.testing.assert_array_equal(S[sample], ref)

    # exclusions from each query's best ADMITTED rows (the score matrix is the oracle's on the sample, just checked)
    excl, top_rows = usable_exclusions(select_from_scores(S, 8, admit=admit)[0], runs, n, rng)
    assert ((top_rows // BM) % tpc != 0).any()             # some excluded best row lies in a warm tile
    if lanes and kinds == KINDS:
        def adm_of(i):
            a = admit[i].copy()
            a[excl[i]] = False
            return a
        assert_mixed_lanes(adm_of, BM, tpc, ks, arm)
    if order == "ties":
        # kind c admits every second copy of a run.  Run 0 lies in ONE block, across a tile boundary, with admitted and
        # rejected copies on both sides, and its admitted copies alone are more than k: the block's list cannot hold
        # them all, and row order has to decide among admitted copies inside the FACET arm, not only in the merge of
        # the blocks' lists.  Not at k = 128 (small-e1): a run is at most BM - 57 = 199 copies (tie_run_catalog), half
        # of it at most 100; there the copies of one block all fit and only the count over all runs exceeds k.
        dup = (P == P[stray]).all(axis=1)
        c_row = admit[first_of("c")]
        assert max(ks) < c_row[dup].sum() < dup.sum(), (c_row[dup].sum(), dup.sum())
        a0, b0 = runs[0]
        cut = (a0 // BM + 1) * BM
        assert a0 < cut < b0 and a0 // (BM * tpc) == (b0 - 1) // (BM * tpc)
        for part in (c_row[a0:cut], c_row[cut:b0]):
            assert part.any() and not part.all()
        in_run0 = int(c_row[a0:b0].sum())
        print(f"ties: {in_run0} of the {b0 - a0} copies of run 0 are admitted under kind c")
        assert [k for k in ks if in_run0 <= k] == ([128] if arm == "small-e1" else []), (in_run0, ks)

    admissible = np.where(admit[sample], ref, -np.inf).astype(np.float32)
    for j, i in enumerate(sample):
        admissible[j, excl[i]] = -np.inf
    union = union_lists(admit[sample], excl, sample)
    for k in ks:
        if order == "ascending":
            # warm masked queries flood the queues: rows of a warm tile above the block's k-th best admissible row so far.
            # d (open): at least 2 qcap in every warm tile, as in the plain test.  c (a third of the rows; none in the
            # last tile, whose aisle it rejects): 2 qcap in MOST warm tiles where a third of a tile is that many, else
            # (the 64-slot arms: 85 of 256 rows against 128) more than qcap - still an overflow and a second iteration
            counts, exists = warm_tile_beaters(admissible, k, BM, tpc)
            tile = np.arange(n_chunks)[:, None] * tpc + np.arange(1, tpc)[None, :]
            d = counts[[j for j, i in enumerate(sample) if kind_of(i, kinds) == "d"]][:, exists]
            c = counts[[j for j, i in enumerate(sample) if kind_of(i, kinds) == "c"]][:, exists & (tile < (n + BM - 1) // BM - 1)]
            bound_c = 2 * qcap if BM * len(EVERY_THIRD) // N_AISLES >= 2 * qcap else qcap + 1
            print(f"k {k}: rows of a warm tile above the block's k-th best so far: open {d.min()} .. {d.max()}, "
                  f"every third aisle {c.min()} .. {c.max()} (bound {bound_c})")
            assert d.min() >= 2 * qcap, (d.min(), qcap)
            assert (c >= bound_c).mean() >= MOST, (c.min(), bound_c)
        got = ix.search(qd, k, excl, allow=dm)
        assert_search(got, select_from_scores(S, k, excl, ROW_OFFSET, admit=admit))
        assert_search((got[0][sample], got[1][sample]),
                      oracle.search(q[sample], P, k, union, row_offset=ROW_OFFSET, storage=storage))
    ix.close()


@pytest.mark.parametrize("arm,order,storage", CASES)
def test_faceted_warm_tiles_vs_oracle_and_score_matrix(torch_cuda, arm, order, storage):
    """One arm of the selection under masks, over blocks of at least 3 tiles with a ragged last tile, at each k of the
    arm.  The eight mask kinds (kind_allow) cycle by query (kind_of), exclusions of the queries' own best admitted rows lie
    on top for two thirds of them, and the last query tile is partial.  Where a lane holds two queries they are of
    different kinds, and a lane with one cold and one warm query in mid-walk is asserted from the inputs and sampled
    (assert_mixed_lanes).  Kinds a and e are in every query tile and never fill their lists, so every block here is cold
    (flags[2]) in every tile: two passes and a forced merge per tile - the warm blocks' single pass and trigger-based
    merges under masks are test_faceted_warm_blocks_take_one_pass's.
    random:    every query with a ranking of its own.
    ascending: every query's score grows with the row, so an open or a third-of-the-aisles query finds more candidates
               than its queue holds in every warm tile and the offer loop iterates, with the per-candidate mask test in it.
    ties:      the tie-run catalog; under kind c only every second copy of a run is admitted, across a tile boundary too:
               row order decides among the admitted copies only.  The runs of big-merge2 and small-k32 are longer than
               the plain test's (TIE_RUN), so that the admitted half of run 0 alone exceeds k."""
    run_tiled_case(arm, order, storage)


@pytest.mark.parametrize("arm,order", [("big-merge2", "ascending"), ("mid-merge", "random")])
def test_faceted_warm_blocks_take_one_pass(torch_cuda, arm, order):
    """Only kinds c and d, alternating within every lane: no query stays cold, so after a block's first tile no lane
    sets flags[2] once the lists are full - after two tiles at the latest, asserted from the facets - and offer() takes
    the warm block's path under FACET: one pass per tile, queues merged when a trigger fires or at the last tile, every
    candidate through facet_admits."""
    run_tiled_case(arm, order, "f32", kinds="cd")


def test_faceted_warm_tiles_on_a_one_facet_index(torch_cuda):
    """The CfgBig arm once more on an index with aisles only: the second facet's words are all ones in LDS."""
    run_tiled_case("big-merge2", "random", "f32", n_facets=1)


# ---------------------------------------------------------------- the filter storages over several rounds
def filter_rows(Q, rounds, extra):
    """A catalog of rounds * blocks + extra tiles of 256 rows, the last of 229, blocks = what the resident pass wants
    for Q queries (one per CU and query tile): `rounds` rounds per block, or one more when extra > 0."""
    blocks = min(max(n_cu() // ((Q + 63) // 64), 1), 256)
    return (rounds * blocks + extra - 1) * 256 + 229


def filter_case_inputs(order, n, dim, Q, BM, tpc, kp, base, rng, check, run_len=64):
    """Catalog, facets, masks and exclusions of one filter case -> (P, q, qd device queries, F, masks, dm device masks,
    excl, plain index with the facets set).  The exclusions come from the plain storage's own faceted top 8: inputs
    only."""
    P, q, runs, _, _ = catalog(order, n, dim, BM, tpc, run_len)
    q = q[:Q]
    F = tile_facets(n, BM, tpc, tuple(runs))
    allow, masks = faceted_inputs(F, Q, BM, tpc, (kp,), check)
    plain = DeviceIndex(P, storage=base, row_offset=ROW_OFFSET)
    plain.set_facets(F)
    qd = torch.tensor(q).cuda()
    dm = facet_masks(allow, Q, 2, plain.device)
    top8 = plain.search(qd, 8, allow=dm)[0].cpu().numpy()
    excl, _ = usable_exclusions(np.where(top8 >= 0, top8 - ROW_OFFSET, -1), runs, n, rng)
    return P, q, qd, F, masks, dm, excl, plain


def assert_sample_is_the_oracles(got, sample, q, P, k, F, masks, excl, base, lanes=None):
    """lanes = (BM, tiles per block, list length, name): the sample holds LANE_PAIRS, and assert_mixed_lanes holds."""
    admit = admitted_matrix(F, masks[sample])
    if lanes:
        def adm_of(i):
            a = admit[sample.index(i)].copy()
            a[excl[i]] = False
            return a
        assert_mixed_lanes(adm_of, lanes[0], lanes[1], (lanes[2],), lanes[3])
    assert_search((got[0][sample], got[1][sample]),
                  oracle.search(q[sample], P, k, union_lists(admit, excl, sample), row_offset=ROW_OFFSET, storage=base))


@pytest.mark.parametrize("k", [20, 40], ids=["k20-32slots-merge2", "k40-16slots-merge"])
@pytest.mark.parametrize("dim", [384, 128], ids=["resident", "staged"])
@pytest.mark.parametrize("base", ["f32", "bf16"])
def test_faceted_filter_pass_over_several_rounds(torch_cuda, base, dim, k):
    """1,024 queries behind a filter pass whose blocks walk about 4 rounds (resident, dim 384) or tiles (staged), random,
    ascending and tie-run catalogs, the mask kinds and exclusions of the tiled test.  k = 20: lists of 32, 32-slot
    queues in the resident pass, merge_queue2; k = 40: lists of 56, 16-slot queues, merge_queue.  Equal to the plain
    storage's faceted search on all queries and to the oracle on a sample.  The tie runs (64 copies, 32 of them under
    kind c, three runs of one score) are longer than the candidate lists, so the verify pass cannot prove those queries
    and the guarded exact pass runs its FACET arm over blocks of several tiles: timer slot 4 records one launch, more
    than 3 times as long as on the random catalog, where it exits at once."""
    Q, resident = 1024, dim == 384
    assert Q >= FILTER_MIN_Q
    kp = filter_list_len(k)
    n = filter_rows(Q, 3, 2)
    BM, n_qtiles, tpc, n_chunks = filter_plan(n, Q, n_cu(), resident)
    ex = tiled_plan(n, Q, k, n_cu())
    assert 3 <= tpc <= 5 and n_chunks >= 5 and n % BM and ex[4] >= 2, (tpc, n_chunks, ex)
    assert (kp, kp <= 32) == ((32, True) if k == 20 else (56, False)) and tpc <= RES_QCAP_MAX_ROUNDS
    assert resident_lds(kp, True) <= LDS_MAX
    rng = np.random.default_rng(k + dim)
    sample = sorted(set(query_sample(Q, 64, rng)) | {q for pair in LANE_PAIRS for q in pair})
    print(f"\n{base}+filter dim {dim} k {k}: n_cu {n_cu()}, {n} rows, filter plan {(BM, n_qtiles, tpc, n_chunks)}, "
          f"lists of {kp}, guarded exact plan {ex}")
    fb = {}
    for order in ("random", "ascending", "ties"):
        P, q, qd, F, masks, dm, excl, plain = filter_case_inputs(order, n, dim, Q, BM, tpc, kp, base, rng,
                                                                  "abcfg" if 3 * kp <= BM else "abfg")
        pi, ps = plain.search(qd, k, excl, allow=dm)
        plain.close()
        fx = DeviceIndex(P, storage=base + "+filter", row_offset=ROW_OFFSET)
        fx.set_facets(F)
        fx.search(qd, k, excl, allow=dm)                                   # first launches out of the timed region
        (fi, fs), t = timed(lambda: fx.search(qd, k, excl, allow=dm))
        fx.close()
        assert torch.equal(fi, pi) and torch.equal(fs, ps)
        # the resident pass holds two queries per lane (the staged pass one): mixed lanes against ITS rounds and lists
        assert_sample_is_the_oracles((fi, fs), sample, q, P, k, F, masks, excl, base,
                                     (BM, tpc, kp, f"{order} resident pass") if resident else None)
        fb[order], n_fb = t[4]
        assert n_fb == 1
    print(f"guarded exact pass under masks: {fb['ties']:.4f} ms on the tie runs, {fb['random']:.4f} ms on the random catalog")
    assert fb["ties"] > 3 * fb["random"], fb


def long_catalog(order, n, Q):
    if order == "ascending":
        return direction_catalog(order, n, 384, Q, 4096)
    rng = np.random.default_rng(4096)
    P, q = rng.standard_normal((n, 384), dtype=np.float32), rng.standard_normal((Q, 384), dtype=np.float32)
    P.flags.writeable = q.flags.writeable = False
    return P, q


@pytest.mark.parametrize("order", ["random", "ascending"])
def test_faceted_resident_pass_over_long_blocks(torch_cuda, order):
    """4,096 queries leave the resident pass 4 blocks per query tile at 256 CUs: 66 rounds each, past
    RES_QCAP_MAX_ROUNDS, where the queues drop from 32 to 16 slots at lists of 32 (k = 20).  Equal to the plain storage's
    faceted search on all queries, to the oracle on 8."""
    Q, k = 4096, 20
    kp = filter_list_len(k)
    n = filter_rows(Q, 66, 0)
    BM, n_qtiles, tpc, n_chunks = filter_plan(n, Q, n_cu(), True)
    assert kp <= 32 and tpc > RES_QCAP_MAX_ROUNDS and n % BM, (kp, tpc)
    print(f"\nlong blocks, {order}: n_cu {n_cu()}, {n} rows, filter plan {(BM, n_qtiles, tpc, n_chunks)}, lists of {kp}")
    P, q = long_catalog(order, n, Q)
    F = tile_facets(n, BM, tpc)
    allow, masks = faceted_inputs(F, Q, BM, tpc, (kp,), "fg")
    rng = np.random.default_rng(66)
    sample = [2, 3, 34, 35, 63, Q - 64, int(rng.integers(64, Q - 64)), Q - 1]   # lanes (c, d) and (d, e) among them
    assert len(sample) * n * 384 <= ORACLE_FMAS
    plain = DeviceIndex(P, storage="f32", row_offset=ROW_OFFSET)
    plain.set_facets(F)
    qd = torch.tensor(q).cuda()
    dm = facet_masks(allow, Q, 2, plain.device)
    top8 = plain.search(qd, 8, allow=dm)[0].cpu().numpy()
    excl, _ = usable_exclusions(np.where(top8 >= 0, top8 - ROW_OFFSET, -1), [], n, rng)
    pi, ps = plain.search(qd, k, excl, allow=dm)
    plain.close()
    fx = DeviceIndex(P, storage="f32+filter", row_offset=ROW_OFFSET)
    fx.set_facets(F)
    (fi, fs), t = timed(lambda: fx.search(qd, k, excl, allow=dm))
    fx.close()
    assert t[4][1] == 1                                                    # the filter path ran
    assert torch.equal(fi, pi) and torch.equal(fs, ps)
    assert_sample_is_the_oracles((fi, fs), sample, q, P, k, F, masks, excl, "f32")
    admit = admitted_matrix(F, masks[[3, 35]])
    admit[0, excl[3]] = admit[1, excl[35]] = False
    assert one_cold_one_warm(admit[:1], admit[1:], BM, tpc, kp).all()      # the lane of queries 3 (open) and 35 (nothing)


def test_faceted_resident_pass_at_its_lds_edge(torch_cuda):
    """300 queries, dim 384, f32+filter, blocks of about 4 rounds.  Lists of k + 12 (rounded up to 8) keys: at k = 84
    the faceted resident pass carves 161,552 B of the 163,840 B of LDS, its largest; at k = 85 and 92 (lists of 104)
    the masks' 5,120 B no longer fit, the faceted call takes the exact kernels while the plain call still filters; at
    k = 93 both are exact.  Which path ran shows in timer slot 4: the guarded exact pass is launched behind a filter
    pass only.  At each k: the faceted search (into a workspace of exactly icrec_search_faceted_workspace_bytes) equals
    select_from_scores on all queries and the oracle on the sample; allow=None and all-ones masks equal the plain
    search, which equals select_from_scores without the masks."""
    Q, dim = 300, 384
    n = filter_rows(Q, 3, 2)
    BM, n_qtiles, tpc, n_chunks = filter_plan(n, Q, n_cu(), True)
    assert 3 <= tpc <= 5 and n % BM, (tpc, n_chunks)
    assert resident_lds(filter_list_len(84), True) == 161_552 <= LDS_MAX
    for k in (85, 92):
        assert resident_lds(filter_list_len(k), False) <= LDS_MAX < resident_lds(filter_list_len(k), True)
    assert resident_lds(filter_list_len(93), False) > LDS_MAX
    print(f"\nLDS edge: n_cu {n_cu()}, {n} rows, filter plan {(BM, n_qtiles, tpc, n_chunks)}, exact plan at k = 93 "
          f"{tiled_plan(n, Q, 93, n_cu())}")
    rng = np.random.default_rng(84)
    P = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((Q, dim), dtype=np.float32)
    q[::7] = P[rng.integers(0, n, q[::7].shape[0])] + 0.3 * q[::7]
    F = tile_facets(n, BM, tpc)
    allow, masks = faceted_inputs(F, Q, BM, tpc, (filter_list_len(84),), "abcfg")
    admit = admitted_matrix(F, masks)
    sample = sorted(set(query_sample(Q, 64, rng)) | {q for pair in LANE_PAIRS for q in pair})
    ix = DeviceIndex(P, storage="f32+filter", row_offset=ROW_OFFSET)
    ix.set_facets(F)
    qd = torch.tensor(q).cuda()
    dm = facet_masks(allow, Q, 2, ix.device)
    ones = facet_masks([None] * Q, Q, 2, ix.device)
    S = ix.scores(qd).cpu().numpy()
    np.testing.assert_array_equal(S[sample], oracle.scores(oracle.normalize_rows(q[sample]), oracle.normalize_rows(P)))
    excl, _ = usable_exclusions(select_from_scores(S, 8, admit=admit)[0], [], n, rng)
    ei, eo = exclusion_csr(excl, Q, ix.device)
    union = union_lists(admit[sample], excl, sample)

    def adm_of(i):
        a = admit[i].copy()
        a[excl[i]] = False
        return a
    assert_mixed_lanes(adm_of, BM, tpc, (filter_list_len(84),), "LDS edge")
    lib = _native.lib()
    for k in (84, 85, 92, 93):
        need = int(lib.icrec_search_faceted_workspace_bytes(ix._h, Q, k))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=ix.device)
        idx = torch.empty((Q, k), dtype=torch.int64, device=ix.device)
        sc = torch.empty((Q, k), dtype=torch.float32, device=ix.device)
        _, t = timed(lambda: ix.search_into(qd, k, ei, eo, idx, sc, ws=ws, allow=dm))
        plain, tp = timed(lambda: ix.search(qd, k, excl))
        print(f"k {k}: lists of {filter_list_len(k)}, workspace {need} B, guarded-pass launches faceted {t[4][1]}, plain {tp[4][1]}")
        assert (t[4][1], tp[4][1]) == (int(k <= 84), int(k <= 92))
        assert_search((idx, sc), select_from_scores(S, k, excl, ROW_OFFSET, admit=admit))
        assert_search((idx[sample], sc[sample]), oracle.search(q[sample], P, k, union, row_offset=ROW_OFFSET))
        assert_search(plain, select_from_scores(S, k, excl, ROW_OFFSET))
        for got in (ix.search(qd, k, excl, allow=None), ix.search(qd, k, excl, allow=ones)):
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    ix.close()
