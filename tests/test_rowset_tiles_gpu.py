"""The SETS arms of the selecting kernels where a block walks several row tiles: the hand-over of the set words from
tile to tile through the two halves of TopK::stile (blocks with odd and even tile counts, the ragged last tile as a warm
tile), queries that stay cold to the end of a block's walk under a set with fewer than k members per block, queries that
turn warm in mid-walk, both beside open queries on the same lanes, tie runs of which only alternate copies are members,
under every tile variant and both merges - and the filter storages over several rounds per block: resident and staged
pass, 32- and 16-slot queues, the guarded exact pass under sets, blocks of more than RES_QCAP_MAX_ROUNDS rounds and the
LDS edge of the set-restricted resident pass.  Catalogs, plans and exclusions are those of tests/test_search_tiles_gpu.py
(sized from the CU count); every result is checked bit for bit: ALL queries against select_from_scores on the device's
own score matrix with the admitted rows as a bool matrix (or, for a filter storage, against the plain storage's
set-restricted search), a sample against the oracle with the exclusions united with every inadmissible row."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd.search import exclusion_csr, facet_masks, rowset_bits, rowset_ids
from tests.rowset_cases import admitted_by_sets, resident_lds_sets
from tests.search_harness import (FILTER_MIN_Q, LDS_MAX, RES_QCAP_MAX_ROUNDS, DeviceIndex, _native, admitted_per_tile,
                                  assert_search, filter_list_len, filter_plan, n_cu, oracle, resident_lds,
                                  select_from_scores, tiled_plan, timed)
from tests.search_harness import torch_cuda  # noqa: F401  (fixture)
from tests.test_facet_tiles_gpu import (LANE_PAIRS, TIE_RUN, filter_rows, first_of, kind_of, long_catalog,
                                        one_cold_one_warm, usable_exclusions)
from tests.test_search_tiles_gpu import ARMS, ORACLE_FMAS, ROW_OFFSET, arm_shape, catalog, query_sample

pytestmark = pytest.mark.gpu

SPARSE, MID, THIRD, HALF, LAST, FULL = range(6)   # the sets of tile_sets, by id
N_TILE_SETS = 6
KINDS = "abcdefgh"


@functools.lru_cache(maxsize=None)
def tile_sets(n, BM, tpc, kmax, runs=()):
    """bool [6, n], read-only, against the blocks of tpc tiles of BM rows a kernel walks.  SPARSE: 3 rows of every block
    - fewer than k members per block.  MID: ceil(0.6 kmax) rows of every tile (every row of a shorter last tile) - fewer
    than kmax members in a block's first tile, at least kmax in its first two.  THIRD: a third of the rows, none in the
    ragged last tile; of each tie run (the tie catalog's) the alternate copies.  HALF: half of the rows.  LAST: only
    the rows of the ragged last tile.  FULL: every row."""
    rng = np.random.default_rng(17)
    m = np.zeros((N_TILE_SETS, n), bool)
    n_tiles = (n + BM - 1) // BM
    for lo in range(0, n, BM * tpc):
        m[SPARSE, lo + rng.choice(min(BM * tpc, n - lo), 3, replace=False)] = True
    per_tile = -(-6 * kmax // 10)
    for t in range(n_tiles):
        size = min(BM, n - t * BM)
        m[MID, t * BM + rng.choice(size, min(per_tile, size), replace=False)] = True
    m[THIRD] = rng.random(n) < 1 / 3
    m[THIRD, (n_tiles - 1) * BM:] = False
    for lo, hi in runs:
        m[THIRD, lo:hi:2] = True
        m[THIRD, lo + 1:hi:2] = False
    m[HALF] = rng.random(n) < 0.5
    m[LAST, (n_tiles - 1) * BM:] = True
    m[FULL] = True
    m.flags.writeable = False
    return m


def kind_slots(i):
    """Query i's slots by its kind (test_facet_tiles_gpu.kind_of: neighbouring kinds on the two queries of a lane).
    a: SPARSE, cold to the end; b: MID, warm in mid-walk; c: THIRD; d: open; e: an id past the last set, nothing;
    f: the ragged last tile; g: two sets, HALF and THIRD; h: four slots with FULL, a duplicate and a negative id."""
    return {"a": [SPARSE], "b": [MID], "c": [-1, THIRD], "d": [-1], "e": [N_TILE_SETS], "f": [LAST], "g": [HALF, THIRD],
            "h": [FULL, MID, -3, MID]}[kind_of(i)]


def set_inputs(member, Q, BM, tpc, ks):
    """-> (ids int32 [Q, 4], admit bool [Q, n]) and the preconditions of the kinds, asserted from the inputs before
    anything runs on the device."""
    n = member.shape[1]
    kmax = max(ks)
    n_tiles = (n + BM - 1) // BM
    ids = rowset_ids([kind_slots(i) for i in range(Q)], Q, 4)
    admit = admitted_by_sets(member, ids)
    per = {kd: admitted_per_tile(admit[first_of(kd)], BM, tpc) for kd in KINDS}
    assert per["a"].sum(axis=1).max() == 3 < max(kmax, 4)                       # cold to the end of every block (k >= 4)
    full_blocks = per["b"][:-1]
    assert (full_blocks[:, 0] < kmax).all() and (full_blocks[:, :2].sum(axis=1) >= kmax).all() and tpc >= 3   # warm in mid-walk
    for k in ks:
        if 3 * k <= BM // 2:
            assert (per["c"][:-1, 0] >= k).mean() >= 0.9                          # warm after the first tile
    rows = np.flatnonzero(admit[first_of("f")])
    assert rows.size == n - (n_tiles - 1) * BM and rows.min() == (n_tiles - 1) * BM and n % BM and (n_tiles - 1) % tpc != 0
    assert admit[first_of("d")].all() and not admit[first_of("e")].any()
    np.testing.assert_array_equal(admit[first_of("g")], member[HALF] & member[THIRD])
    np.testing.assert_array_equal(admit[first_of("h")], member[MID])
    return ids, admit


def assert_mixed_lanes(admit, excl, BM, tpc, ks):
    """The lane pairs (q, q + 32): for every k the pair (d, e) - an open query beside one that nothing admits - has one
    cold and one warm query at the start of a block's second or third tile; so has (a, b) or (b, c) once MID is warm."""
    def adm(i):
        a = admit[i].copy()
        a[excl[i]] = False
        return a
    a = np.stack([adm(p) for p, _ in LANE_PAIRS])
    b = np.stack([adm(p) for _, p in LANE_PAIRS])
    for k in ks:
        mixed = one_cold_one_warm(a, b, BM, tpc, k)
        pairs = [kind_of(p) + kind_of(q) for (p, q), ok in zip(LANE_PAIRS, mixed) if ok]
        print(f"k {k}: lanes with one cold and one warm query in mid-walk, by kind pair: {pairs}")
        assert mixed[first_of("d")], (k, mixed)
        assert k < 4 or mixed[first_of("a")], (k, mixed)                          # SPARSE (cold) beside MID (warm in mid-walk)


def union_lists(admit_rows, excl, queries):
    return [np.union1d(np.flatnonzero(~a), np.asarray(excl[i], np.int64)) for a, i in zip(admit_rows, queries)]


def dev(ids):
    return torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda()


# ---------------------------------------------------------------- the exact tiled kernels
CASES = [(arm, order, "f32") for arm in ARMS for order in ("random", "ties")] + \
        [("big-merge2", "ascending", "f32"), ("small-e1", "ascending", "f32"), ("big-merge2", "random", "bf16"),
         ("small-e1", "ties", "bf16")]


def odd_shape(Q, k):
    """(n_rows, plan): the smallest catalog of at least 3 tiles per block whose blocks walk an ODD number of tiles, with
    a last block of at least 2 tiles and a ragged last tile (arm_shape's catalogs give blocks of 4 and 2 at 256 CUs)."""
    _, BM, _, n_qtiles, _, _ = tiled_plan(1, Q, k, n_cu())
    want = min(max(2 * n_cu() // n_qtiles, 1), 256)
    for n_tiles in range(2 * want + 1, 6 * want):
        n = (n_tiles - 1) * BM + BM - 27
        plan = tiled_plan(n, Q, k, n_cu())
        tpc, n_chunks = plan[4], plan[5]
        if tpc >= 3 and tpc % 2 == 1 and n_tiles - (n_chunks - 1) * tpc >= 2:
            return n, plan
    raise AssertionError("no catalog with an odd tile count per block")


def test_sets_over_blocks_of_an_odd_tile_count(torch_cuda):
    """The hand-over alternates between the two halves of TopK::stile; the arms' catalogs give every block an even
    number of tiles (asserted: where that changes, this test still adds the odd count).  100 queries on CfgBig over
    blocks of 3 tiles, the last block shorter, the ragged last tile a warm tile; all queries against select_from_scores
    on the device's own score matrix, a sample against the oracle."""
    Q, k, dim = 100, 20, 64
    n, plan = odd_shape(Q, k)
    variant, BM, BN, n_qtiles, tpc, n_chunks = plan
    last = (n + BM - 1) // BM - (n_chunks - 1) * tpc
    assert variant == "big" and tpc % 2 == 1 and tpc >= 3 and last >= 2 and n % BM, plan
    even = set()
    for arm, (Qa, ks, _, v, _, _) in ARMS.items():
        na, pa = arm_shape(Qa - 3, ks[0], v)
        even |= {pa[4], (na + pa[1] - 1) // pa[1] - (pa[5] - 1) * pa[4]}
    print(f"\nodd tile counts: n_cu {n_cu()}, {n} rows, plan {plan}, {last} tiles in the last block; the arms' blocks: {sorted(even)}")
    assert {c % 2 for c in even | {tpc, last}} == {0, 1}
    rng = np.random.default_rng(tpc)
    P = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((Q, dim), dtype=np.float32)
    member = tile_sets(n, BM, tpc, k)
    ids, admit = set_inputs(member, Q, BM, tpc, (k,))
    sample = sorted({0, 1, 2, 3, 32, 33, 34, 35, Q - 1} | {p for pair in LANE_PAIRS for p in pair})
    assert len(sample) * n * dim <= ORACLE_FMAS
    ix = DeviceIndex(P, row_offset=ROW_OFFSET)
    ix.set_rowsets(rowset_bits(member, n))
    qd = torch.tensor(q).cuda()
    S = ix.scores(qd).cpu().numpy()
    np.testing.assert_array_equal(S[sample], oracle.scores(oracle.normalize_rows(q[sample]), oracle.normalize_rows(P)))
    excl, _ = usable_exclusions(select_from_scores(S, 8, admit=admit)[0], [], n, rng)
    assert_mixed_lanes(admit, excl, BM, tpc, (k,))
    got = ix.search(qd, k, excl, sets=dev(ids))
    assert_search(got, select_from_scores(S, k, excl, ROW_OFFSET, admit=admit))
    assert_search((got[0][sample], got[1][sample]),
                  oracle.search(q[sample], P, k, union_lists(admit[sample], excl, sample), row_offset=ROW_OFFSET))
    ix.close()


@pytest.mark.parametrize("arm,order,storage", CASES)
def test_sets_over_warm_tiles_vs_oracle_and_score_matrix(torch_cuda, arm, order, storage):
    """One arm of the selection under sets, over blocks of at least 3 tiles with a ragged last tile, at each k of the
    arm.  The eight kinds of slots (kind_slots) cycle by query, exclusions of the queries' own best admitted rows lie on
    top for two thirds of them, and the last query tile is partial.  ties: only alternate copies of each run are in
    THIRD, across a tile boundary too: row order decides among the member copies only."""
    Qa, ks, dim, variant, qcap, run_len = ARMS[arm]
    run_len = TIE_RUN.get(arm, run_len)
    Q = Qa - 3                                             # the last query tile is partial: padding queries admit nothing
    n, plan = arm_shape(Q, ks[0], variant)
    _, BM, BN, n_qtiles, tpc, n_chunks = plan
    assert Q % BN
    for k in ks:
        assert arm_shape(Q, k, variant) == (n, plan) and k <= run_len - 7
    P, q, runs, _, stray = catalog(order, n, dim, BM, tpc, run_len)
    q = q[:Q]
    member = tile_sets(n, BM, tpc, max(ks), tuple(runs))
    rng = np.random.default_rng(len(arm) + 10 * len(order))
    lanes = BN >= 64           # TN = 2: the pairs of LANE_PAIRS share their lanes (CfgSmall holds one query per lane)
    sample = set(query_sample(Q, BN, rng))
    if n > 100_000:
        sample = set(sorted(sample)[::2]) | {0, Q - 1}
    sample = sorted(sample | {2, 3} | ({p for pair in LANE_PAIRS for p in pair} if lanes else set()))
    assert len(sample) * n * dim <= ORACLE_FMAS
    last = (n + BM - 1) // BM - (n_chunks - 1) * tpc
    print(f"\n{arm} {order} {storage}: n_cu {n_cu()}, {n} rows x {dim}, {Q} queries, plan {plan}, {last} tiles in the "
          f"last block, sample of {len(sample)}")
    ids, admit = set_inputs(member, Q, BM, tpc, ks)

    rows = oracle.normalize_rows(P)
    if storage == "bf16":
        rows = oracle.round_bf16(rows)
    ref = oracle.scores(oracle.normalize_rows(q[sample]), rows)
    ix = DeviceIndex(P, storage=storage, row_offset=ROW_OFFSET)
    ix.set_rowsets(rowset_bits(member, n))
    qd = torch.tensor(q).cuda()
    S = ix.scores(qd).cpu().numpy()                        # the EMIT arm: no selection, no sets
    np.testing.assert_array_equal(S[sample], ref)
    excl, top_rows = usable_exclusions(select_from_scores(S, 8, admit=admit)[0], runs, n, rng)
    assert ((top_rows // BM) % tpc != 0).any()             # some excluded best row lies in a warm tile
    if lanes:
        assert_mixed_lanes(admit, excl, BM, tpc, ks)
    if order == "ties":
        dup = (P == P[stray]).all(axis=1)
        c_row = admit[first_of("c")]
        a0, b0 = runs[0]
        cut = (a0 // BM + 1) * BM
        assert a0 < cut < b0 and a0 // (BM * tpc) == (b0 - 1) // (BM * tpc)      # run 0: one block, across a tile boundary
        for part in (c_row[a0:cut], c_row[cut:b0]):
            assert part.any() and not part.all()
        assert 0 < c_row[dup].sum() < dup.sum()
    union = union_lists(admit[sample], excl, sample)
    dids = dev(ids)
    for k in ks:
        got = ix.search(qd, k, excl, sets=dids)
        assert_search(got, select_from_scores(S, k, excl, ROW_OFFSET, admit=admit))
        assert_search((got[0][sample], got[1][sample]),
                      oracle.search(q[sample], P, k, union, row_offset=ROW_OFFSET, storage=storage))
    ix.close()


# ---------------------------------------------------------------- the filter storages over several rounds
def filter_case(order, n, dim, Q, BM, tpc, kp, base, rng):
    """-> (P, q, qd, member, ids, admit, excl, plain index with the sets): the exclusions come from the plain storage's
    own set-restricted top 8."""
    P, q, runs, _, _ = catalog(order, n, dim, BM, tpc, 64)
    q = q[:Q]
    member = tile_sets(n, BM, tpc, kp, tuple(runs))
    ids, admit = set_inputs(member, Q, BM, tpc, (kp,))
    plain = DeviceIndex(P, storage=base, row_offset=ROW_OFFSET)
    plain.set_rowsets(rowset_bits(member, n))
    qd = torch.tensor(q).cuda()
    top8 = plain.search(qd, 8, sets=dev(ids))[0].cpu().numpy()
    excl, _ = usable_exclusions(np.where(top8 >= 0, top8 - ROW_OFFSET, -1), runs, n, rng)
    return P, q, qd, member, ids, admit, excl, plain


@pytest.mark.parametrize("base,dim,k", [("f32", 384, 20), ("f32", 384, 40), ("f32", 128, 20), ("f32", 128, 40), ("bf16", 384, 20)],
                         ids=["f32-resident-k20-32slots", "f32-resident-k40-16slots", "f32-staged-k20", "f32-staged-k40",
                              "bf16-resident-k20"])
def test_sets_behind_a_filter_pass_over_several_rounds(torch_cuda, base, dim, k):
    """1,024 queries behind a filter pass whose blocks walk about 4 rounds (resident, dim 384) or tiles (staged), random
    and tie-run catalogs, the kinds of slots and the exclusions of the tiled test.  Equal to the plain storage's
    set-restricted search on all queries and to the oracle on a sample.  The member copies of the tie runs are more than
    a candidate list holds, so the verify pass cannot prove those queries and the guarded exact pass runs its SETS arm
    over blocks of several tiles: timer slot 4 records its one launch."""
    Q, resident = 1024, dim == 384
    assert Q >= FILTER_MIN_Q
    kp = filter_list_len(k)
    n = filter_rows(Q, 3, 2)
    BM, n_qtiles, tpc, n_chunks = filter_plan(n, Q, n_cu(), resident)
    ex = tiled_plan(n, Q, k, n_cu())
    assert 3 <= tpc <= 5 and n_chunks >= 5 and n % BM and ex[4] >= 2, (tpc, n_chunks, ex)
    assert (kp, kp <= 32) == ((32, True) if k == 20 else (56, False)) and tpc <= RES_QCAP_MAX_ROUNDS
    assert resident_lds_sets(kp) <= LDS_MAX
    rng = np.random.default_rng(k + dim)
    sample = sorted(set(query_sample(Q, 64, rng)) | {p for pair in LANE_PAIRS for p in pair})
    print(f"\n{base}+filter dim {dim} k {k}: n_cu {n_cu()}, {n} rows, filter plan {(BM, n_qtiles, tpc, n_chunks)}, "
          f"lists of {kp}, guarded exact plan {ex}")
    for order in ("random", "ties"):
        P, q, qd, member, ids, admit, excl, plain = filter_case(order, n, dim, Q, BM, tpc, kp, base, rng)
        dids = dev(ids)
        pi, ps = plain.search(qd, k, excl, sets=dids)
        plain.close()
        if resident:
            assert_mixed_lanes(admit, excl, BM, tpc, (kp,))
        fx = DeviceIndex(P, storage=base + "+filter", row_offset=ROW_OFFSET)
        fx.set_rowsets(rowset_bits(member, n))
        (fi, fs), t = timed(lambda: fx.search(qd, k, excl, sets=dids))
        fx.close()
        assert t[4][1] == 1                                                   # the filter path ran
        assert torch.equal(fi, pi) and torch.equal(fs, ps)
        assert_search((fi[sample], fs[sample]),
                      oracle.search(q[sample], P, k, union_lists(admit[sample], excl, sample), row_offset=ROW_OFFSET, storage=base))


def test_sets_in_the_resident_pass_over_long_blocks(torch_cuda):
    """4,096 queries leave the resident pass 4 blocks per query tile at 256 CUs: 66 rounds each, past
    RES_QCAP_MAX_ROUNDS, where the queues drop from 32 to 16 slots at lists of 32 (k = 20).  Equal to the plain storage's
    set-restricted search on all queries, to the oracle on 8."""
    Q, k = 4096, 20
    kp = filter_list_len(k)
    n = filter_rows(Q, 66, 0)
    BM, n_qtiles, tpc, n_chunks = filter_plan(n, Q, n_cu(), True)
    assert kp <= 32 and tpc > RES_QCAP_MAX_ROUNDS and n % BM, (kp, tpc)
    print(f"\nlong blocks: n_cu {n_cu()}, {n} rows, filter plan {(BM, n_qtiles, tpc, n_chunks)}, lists of {kp}")
    P, q = long_catalog("random", n, Q)
    member = tile_sets(n, BM, tpc, kp)
    ids, admit = set_inputs(member, Q, BM, tpc, (kp,))
    rng = np.random.default_rng(66)
    sample = [2, 3, 34, 35, 63, Q - 64, int(rng.integers(64, Q - 64)), Q - 1]   # lanes (c, d) and (d, e) among them
    assert len(sample) * n * 384 <= ORACLE_FMAS
    plain = DeviceIndex(P, storage="f32", row_offset=ROW_OFFSET)
    plain.set_rowsets(rowset_bits(member, n))
    qd = torch.tensor(q).cuda()
    dids = dev(ids)
    top8 = plain.search(qd, 8, sets=dids)[0].cpu().numpy()
    excl, _ = usable_exclusions(np.where(top8 >= 0, top8 - ROW_OFFSET, -1), [], n, rng)
    pi, ps = plain.search(qd, k, excl, sets=dids)
    plain.close()
    fx = DeviceIndex(P, storage="f32+filter", row_offset=ROW_OFFSET)
    fx.set_rowsets(rowset_bits(member, n))
    (fi, fs), t = timed(lambda: fx.search(qd, k, excl, sets=dids))
    fx.close()
    assert t[4][1] == 1                                                    # the filter path ran
    assert torch.equal(fi, pi) and torch.equal(fs, ps)
    assert_search((fi[sample], fs[sample]),
                  oracle.search(q[sample], P, k, union_lists(admit[sample], excl, sample), row_offset=ROW_OFFSET))


def test_set_restricted_resident_pass_at_its_lds_edge(torch_cuda):
    """300 queries, dim 384, f32+filter, blocks of about 4 rounds.  Lists of k + 12 (rounded up to 8) keys: the
    set-restricted resident pass adds 64 x 16 B of slots and 2 x 8 x 64 x 4 B of set words to the faceted pass's LDS, so
    it fits up to k = 76 (lists of 88: 162,576 B of 163,840 B) and from k = 77 (lists of 96) the set-restricted call takes
    the exact kernels, while a faceted call without set ids still filters up to k = 84 and the plain call up to k = 92.
    Which path ran shows in timer slot 4: the guarded exact pass is launched behind a filter pass only.  At each k the
    set-restricted search (into a workspace of exactly icrec_search_in_sets_workspace_bytes) equals select_from_scores
    on all queries and the oracle on the sample."""
    Q, dim = 300, 384
    n = filter_rows(Q, 3, 2)
    BM, n_qtiles, tpc, n_chunks = filter_plan(n, Q, n_cu(), True)
    assert 3 <= tpc <= 5 and n % BM, (tpc, n_chunks)
    assert resident_lds_sets(filter_list_len(76)) == 162_576 <= LDS_MAX < resident_lds_sets(filter_list_len(77))
    assert resident_lds(filter_list_len(84), True) <= LDS_MAX < resident_lds(filter_list_len(85), True)
    rng = np.random.default_rng(76)
    P = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((Q, dim), dtype=np.float32)
    q[::7] = P[rng.integers(0, n, q[::7].shape[0])] + 0.3 * q[::7]
    member = tile_sets(n, BM, tpc, filter_list_len(76))
    ids, admit = set_inputs(member, Q, BM, tpc, (filter_list_len(76),))
    sample = sorted(set(query_sample(Q, 64, rng)) | {p for pair in LANE_PAIRS for p in pair})
    ix = DeviceIndex(P, storage="f32+filter", row_offset=ROW_OFFSET)
    ix.set_rowsets(rowset_bits(member, n))
    ix.set_facets(np.zeros((n, 1), np.uint8))
    qd = torch.tensor(q).cuda()
    dids = dev(ids)
    ones = facet_masks([None] * Q, Q, 1, ix.device)
    S = ix.scores(qd).cpu().numpy()
    np.testing.assert_array_equal(S[sample], oracle.scores(oracle.normalize_rows(q[sample]), oracle.normalize_rows(P)))
    excl, _ = usable_exclusions(select_from_scores(S, 8, admit=admit)[0], [], n, rng)
    ei, eo = exclusion_csr(excl, Q, ix.device)
    union = union_lists(admit[sample], excl, sample)
    assert_mixed_lanes(admit, excl, BM, tpc, (filter_list_len(76),))
    lib = _native.lib()
    for k in (76, 77, 84, 85):
        need = int(lib.icrec_search_in_sets_workspace_bytes(ix._h, Q, k))
        assert need == int(lib.icrec_search_workspace_bytes(ix._h, Q, k)) > 0
        ws = torch.empty(need, dtype=torch.uint8, device=ix.device)
        idx = torch.empty((Q, k), dtype=torch.int64, device=ix.device)
        sc = torch.empty((Q, k), dtype=torch.float32, device=ix.device)
        _, t = timed(lambda: ix.search_into(qd, k, ei, eo, idx, sc, ws=ws, sets=dids))
        faceted, tf = timed(lambda: ix.search(qd, k, excl, allow=ones))
        print(f"k {k}: lists of {filter_list_len(k)}, workspace {need} B, guarded-pass launches in sets {t[4][1]}, faceted {tf[4][1]}")
        assert (t[4][1], tf[4][1]) == (int(k <= 76), int(k <= 84))
        assert_search((idx, sc), select_from_scores(S, k, excl, ROW_OFFSET, admit=admit))
        assert_search((idx[sample], sc[sample]), oracle.search(q[sample], P, k, union, row_offset=ROW_OFFSET))
        assert_search(faceted, select_from_scores(S, k, excl, ROW_OFFSET))
    ix.close()
