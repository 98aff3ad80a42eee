"""Shared by the search GPU tests (test_search_gpu, test_search_dims_gpu, test_sharded_gpu, the search tests of
test_baseline_sizes_gpu): the imports and the GPU fixture, the check of an index against the oracle, the random
exclusion lists (one function per draw sequence), shard cutting, the tie-block catalog, the launch timers, the
properties of a result list, the memoised bench catalog, the launch plans and the selection in numpy, which rows
a query's facet masks admit, the packed ranking keys and the merges in numpy, and the restatement of the exclusion
exchange's CSR.  One definition each; importing this needs no GPU."""
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


# ---------------------------------------------------------------- the tiled kernels' launch plan and selection, in numpy
TILE_VARIANTS = {"big": (128, 128), "mid": (256, 64), "small": (256, 32)}  # (BM rows, BN queries): CfgBig / CfgMid / CfgSmall


def tiled_plan(n_rows, Q, k, n_cu):
    """csrc/search.hip's make_plan with allow_stream false, and its plan_chunks, restated with the same integer
    arithmetic -> (variant, BM, BN, n_qtiles, tiles_per_chunk, n_chunks).  Block (chunk, query tile) of a tiled kernel
    walks row tiles chunk * tiles_per_chunk ... of BM rows each; its selection is warm from the second tile on."""
    variant = "big" if Q > 64 and k <= 32 else "mid" if Q > 32 and k <= 64 else "small"
    BM, BN = TILE_VARIANTS[variant]
    n_qtiles = (Q + BN - 1) // BN
    n_row_tiles = (n_rows + BM - 1) // BM
    want = min(max(2 * n_cu // n_qtiles, 1), 256)
    want = min(want, n_row_tiles)
    tiles_per_chunk = (n_row_tiles + want - 1) // want
    n_chunks = (n_row_tiles + tiles_per_chunk - 1) // tiles_per_chunk
    return variant, BM, BN, n_qtiles, tiles_per_chunk, n_chunks


def stream_plan(n_rows, Q, n_cu, stream_max_q=8):
    """csrc/search.hip's make_plan with allow_stream true, the branch of variant 3 (stream_search_kernel), and its
    plan_chunks, restated with the same integer arithmetic -> ("stream", 256, BN, 1, tiles_per_chunk, n_chunks), the
    tuple of tiled_plan; None where make_plan takes a tiled kernel instead: more than stream_max_q queries (8 unless
    ICREC_STREAM_MAX_Q said otherwise when the index was made), or 3 .. 8 queries over fewer than 6 tiles of 256 rows
    per CU.  One block per chunk, one sorted list per chunk and query, at most 1,024 chunks (MERGE_MAX_LISTS)."""
    BM = 256
    n_row_tiles = (n_rows + BM - 1) // BM
    if not (Q <= stream_max_q and (Q <= 2 or n_row_tiles >= 2 * 3 * n_cu)):
        return None
    BN = 1 if Q <= 1 else 2 if Q <= 2 else 4 if Q <= 4 else 8
    want = min(max(3 * n_cu, 1), 1024)
    want = min(want, n_row_tiles)
    tiles_per_chunk = (n_row_tiles + want - 1) // want
    n_chunks = (n_row_tiles + tiles_per_chunk - 1) // tiles_per_chunk
    return "stream", BM, BN, 1, tiles_per_chunk, n_chunks


def search_plan(n_rows, Q, k, n_cu):
    """The plan icrec_search takes on a plain (f32 or bf16) index: stream_plan where it applies, else tiled_plan."""
    return stream_plan(n_rows, Q, n_cu) or tiled_plan(n_rows, Q, k, n_cu)


MERGE_BLOCK_KEYS, MERGE_MAX_LISTS = 16 * 256, 1024   # csrc/sort.hip, csrc/common.h


def merge_form(n_lists, Q, k, block=True):
    """Which kernel of csrc/sort.hip merges n_lists lists of k keys for Q queries: "block" (merge_block_kernel,
    launch_merge_block's condition), else launch_merge's arm, "wave4" (merge_kernel<4>, up to 256 lists) or "wave16"
    (merge_kernel<16>).  block=False: a caller that never tries the block merge (icrec_merge_topk; a search does)."""
    assert 1 <= n_lists <= MERGE_MAX_LISTS
    if block and Q <= 4 and n_lists <= 256 and n_lists * k <= MERGE_BLOCK_KEYS:
        return "block"
    return "wave4" if n_lists <= 256 else "wave16"


def plan_workspace_bytes(plan, dim, k):
    """Plan::ws_q + Plan::ws_partial of make_plan for a plan tuple: [queries, padded to whole tiles | one list of k keys
    per chunk and padded query], each part rounded up to 256 B."""
    _, _, BN, n_qtiles, _, n_chunks = plan
    up = lambda v: (v + 255) & ~255  # noqa: E731
    Qpad = n_qtiles * BN
    return up(Qpad * dim * 4) + up(n_chunks * Qpad * k * 8)


def assert_plan_is_the_librarys(ix, Q, k, plan):
    """plan is the one a search of Q queries at k takes on the plain (f32 or bf16) index ix, and the library cuts the
    rows as the restated plans do: icrec_search_workspace_bytes returns, for an index without filter planes, the larger
    of its tiled plan's and its streaming plan's workspace (the same plan twice where no streaming kernel applies),
    each laid out as plan_workspace_bytes says - the library's own BN and chunk counts, against tiled_plan's and
    stream_plan's.  This restates icrec_search_workspace_bytes and make_plan in csrc/search.hip: when that layout
    changes, this function changes with it.  (Where a search streams, the tiled plan's lists of 32 padded queries are
    the larger part: the streaming plan's chunk count then shows in the sum only where it is the larger one.)"""
    tiled = tiled_plan(ix.n_rows, Q, k, n_cu())
    stream = stream_plan(ix.n_rows, Q, n_cu())
    assert plan == (stream or tiled), (plan, stream, tiled)
    want = max(plan_workspace_bytes(p, ix.dim, k) for p in (tiled, stream) if p is not None)
    got = int(_native.lib().icrec_search_workspace_bytes(ix._h, Q, k))
    assert got == want, (got, want, plan)


def select_from_scores(scores, k, excl=None, row_offset=0, admit=None):
    """The library's selection on a complete [Q, n] float32 score matrix: per query the k best rows that its list
    excl[i] (local rows, as oracle.search takes them) does not name, score descending and row ascending among equal
    scores -> (idx int64 [Q, k], score float32 [Q, k]), idx = row_offset + row, padded with (-1, 0) where fewer than k
    rows are admissible - oracle.search's conventions.  Each (score, row) becomes one integer that grows with the
    score and, among equal scores, falls with the row; -0 counts as +0; scores must not be NaN.  admit: bool [Q, n],
    False = the row is inadmissible for that query, exactly like a row its exclusion list names (facet masks over a
    large catalog, where the rejected rows as lists would be millions of Python ints)."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    Q, n = s.shape
    assert admit is None or (admit.dtype == np.bool_ and admit.shape == (Q, n)), "admit: bool [Q, n]"
    idx = np.full((Q, k), -1, np.int64)
    sc = np.zeros((Q, k), np.float32)
    m = min(k, n)
    low = np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)
    for lo in range(0, Q, 64):  # blocks of queries: the keys of 64 x n scores at a time
        blk = s[lo:lo + 64] + np.float32(0.0)
        u = blk.view(np.uint32)
        ordered = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
        keys = (ordered.astype(np.uint64) << np.uint64(32)) | low[None, :]
        if excl is not None:
            for i in range(blk.shape[0]):
                e = np.asarray(sorted(set(int(v) for v in excl[lo + i])), np.int64)
                keys[i, e[(e >= 0) & (e < n)]] = 0  # below every real key
        if admit is not None:
            keys[~admit[lo:lo + 64]] = 0
        top = np.sort(np.partition(keys, n - m, axis=1)[:, n - m:], axis=1)[:, ::-1]
        real = top != 0
        rows = (np.uint64(0xFFFFFFFF) - (top & np.uint64(0xFFFFFFFF))).astype(np.int64)
        rows[~real] = 0
        idx[lo:lo + 64, :m] = np.where(real, row_offset + rows, -1)
        sc[lo:lo + 64, :m] = np.where(real, np.take_along_axis(blk, rows, axis=1), np.float32(0.0))
    return idx, sc


def warm_tile_beaters(scores, k, BM, tiles_per_chunk):
    """For every block of tiles_per_chunk row tiles of BM rows and every tile after the block's first: how many of the
    tile's rows score above the k-th best of the block's earlier rows - what a warm tile has to offer.  (A later row
    that only EQUALS that score loses on the row number and is not counted.)  scores: [S, n] float32 with inadmissible
    rows at -inf -> (counts int [S, n_chunks, tiles_per_chunk - 1], exists bool [n_chunks, tiles_per_chunk - 1])."""
    S, n = scores.shape
    n_tiles = (n + BM - 1) // BM
    n_chunks = (n_tiles + tiles_per_chunk - 1) // tiles_per_chunk
    padded = np.full((S, n_chunks * tiles_per_chunk * BM), -np.inf, np.float32)
    padded[:, :n] = scores
    blocks = padded.reshape(S, n_chunks, tiles_per_chunk, BM)
    counts = np.zeros((S, n_chunks, tiles_per_chunk - 1), np.int64)
    for j in range(1, tiles_per_chunk):
        earlier = blocks[:, :, :j].reshape(S, n_chunks, j * BM)
        kth = np.partition(earlier, j * BM - k, axis=2)[:, :, j * BM - k]
        counts[:, :, j - 1] = (blocks[:, :, j] > kth[:, :, None]).sum(axis=2)
    tile = np.arange(n_chunks)[:, None] * tiles_per_chunk + np.arange(1, tiles_per_chunk)[None, :]
    return counts, tile < n_tiles


def first_pass_offers(tile_scores, k, BM):
    """What the first pass of TopK::offer offers for one query from a COLD tile of BM rows (csrc/search.hip): the
    scores of tile row r sit in the lane group (r // 64, r % 8 // 4) - wave r // 64 owns 64 rows, acc_row gives each
    half of the wavefront alternate runs of 4 - so 2 * BM / 64 lanes hold 32 scores each, and each lane offers its
    scores down to its m-th largest distinct one, m = ceil(k / lanes) + 1 (every score if it has fewer).  Excluded
    rows count here; they are dropped afterwards.  tile_scores: [BM] float32 -> bool [BM]."""
    r = np.arange(BM)
    group = (r // 64) * 2 + (r % 8) // 4
    lanes = 2 * BM // 64
    m = -(-k // lanes) + 1
    offered = np.zeros(BM, bool)
    for g in range(lanes):
        mine = tile_scores[group == g]
        distinct = np.unique(mine)[::-1]
        t = distinct[m - 1] if distinct.size >= m else -np.inf
        offered[group == g] = mine >= t
    return offered


# ---------------------------------------------------------------- packed ranking keys and their merges, in numpy
def pack_keys(scores, rows):
    """csrc/common.h's make_key: (orderable(score bits) << 32) | (0xFFFFFFFF - row), uint64, where orderable flips
    every bit of a negative score and sets the sign bit of the others - a larger key is a better hit under (score
    descending, row ascending).  scores: float32, rows: integers in [0, 2^32 - 2], broadcast against each other.  The
    score's bits are taken as they are: -0.0 packs below +0.0 (the search kernels add +0 first; this does not)."""
    s, r = np.broadcast_arrays(np.asarray(scores, np.float32), np.asarray(rows))
    assert r.dtype.kind in "iu" and (r >= 0).all() and (r <= 0xFFFFFFFE).all()
    u = np.ascontiguousarray(s).view(np.uint32).ravel()
    ordered = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ((ordered.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - r.astype(np.uint64).ravel())).reshape(s.shape)


def unpack_keys(keys):
    """csrc/common.h's store_key: keys uint64 -> (idx int64, score float32) with the score's BITS as they were packed;
    key 0, the pad, gives (-1, 0.0)."""
    keys = np.ascontiguousarray(keys, np.uint64)
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    u = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7FFFFFFF), ~hi)
    score = np.ascontiguousarray(u).view(np.float32)
    idx = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    pad = keys == 0
    return np.where(pad, np.int64(-1), idx), np.where(pad, np.float32(0.0), score)


def merge_reference(keys, k):
    """The k-way merge on keys uint64 [n_lists, Q, k]: per query ALL its keys sorted as descending integers, the first k
    kept and decoded with unpack_keys -> (idx int64 [Q, k], score float32 [Q, k]).  Pads (key 0) sort last."""
    keys = np.ascontiguousarray(keys, np.uint64)
    n_lists, Q, kk = keys.shape
    assert kk == k
    per_query = keys.transpose(1, 0, 2).reshape(Q, n_lists * k)
    return unpack_keys(np.sort(per_query, axis=1)[:, ::-1][:, :k])


def block_merge_candidates(scores_row, k, BM, tiles_per_chunk):
    """How many keys C merge_block_kernel (csrc/sort.hip) ranks for one query: the rows are cut into chunks of
    tiles_per_chunk tiles of BM rows, each chunk gives its k best keys as one sorted list (fewer where it has fewer
    admissible rows); h is the k-th largest list head, or 0 if fewer than k lists are non-empty; C counts the keys
    >= h in the lists whose head is >= h.  The kernel's ranking loop takes a second trip iff C > 256.
    scores_row: float32 [n], inadmissible rows at -inf; -0 counts as +0, as in the search kernels."""
    s = np.ascontiguousarray(scores_row, np.float32)
    n = s.size
    keys = pack_keys(s + np.float32(0.0), np.arange(n))
    keys[np.isneginf(s)] = 0
    block = BM * tiles_per_chunk
    n_chunks = (n + block - 1) // block
    padded = np.zeros(n_chunks * max(block, k), np.uint64).reshape(n_chunks, -1)
    for c in range(n_chunks):
        mine = keys[c * block:(c + 1) * block]
        padded[c, :mine.size] = mine
    lists = np.sort(padded, axis=1)[:, ::-1][:, :k]
    heads = lists[:, 0]
    real = np.sort(heads[heads != 0])[::-1]
    h = real[k - 1] if real.size >= k else np.uint64(0)
    taken = lists[(heads != 0) & (heads >= h)]
    return int(((taken != 0) & (taken >= h)).sum())


# ---------------------------------------------------------------- the exclusion exchange's CSR, in numpy
def csr_restatement(off_all, rows_all, cap, row_lo, row_hi):
    """numpy restatement of comm.hip's excl_sanitize / count / scan / fill: offsets clamped to [0, cap] and made
    non-decreasing by a running maximum, then per gathered query (rank-major) the ids inside [row_lo, row_hi), rebased."""
    world, n1 = off_all.shape
    off = np.maximum.accumulate(np.clip(off_all.astype(np.int64), 0, cap), axis=1)
    csr_off, csr_idx = [0], []
    for r in range(world):
        for i in range(n1 - 1):
            seg = rows_all[r, off[r, i]:off[r, i + 1]].astype(np.int64)
            seg = seg[(seg >= row_lo) & (seg < row_hi)] - row_lo
            csr_idx.extend(seg.tolist())
            csr_off.append(len(csr_idx))
    return np.asarray(csr_off, np.int32), np.asarray(csr_idx, np.int32)


# ---------------------------------------------------------------- facets: which rows a query's allow masks admit
def admitted_matrix(F, masks):
    """include/icrec.h's definition of a faceted search: row r is admissible for query i iff, for EVERY facet f, bit
    v & 31 of word v >> 5 of masks[i, f] is set, v = F[r, f].  F: uint8 [n, n_facets], masks: uint32 [Q, n_facets, 8]
    (search.facet_masks without a device) -> bool [Q, n]."""
    F, masks = np.asarray(F), np.asarray(masks)
    assert F.dtype == np.uint8 and F.ndim == 2 and masks.dtype == np.uint32 and masks.shape[1:] == (F.shape[1], 8)
    ok = np.ones((masks.shape[0], F.shape[0]), bool)
    for f in range(F.shape[1]):
        v = F[:, f].astype(np.int64)
        word, bit = v >> 5, (v & 31).astype(np.uint32)
        for lo in range(0, masks.shape[0], 256):  # blocks of queries: 256 x n words at a time
            ok[lo:lo + 256] &= ((masks[lo:lo + 256, f][:, word] >> bit[None, :]) & np.uint32(1)).astype(bool)
    return ok


def admitted_per_tile(admit_row, BM, tiles_per_chunk):
    """One query's admitted rows (bool [n]) counted per row tile of the blocks a tiled kernel walks: int [n_chunks,
    tiles_per_chunk], entry [c, j] = admitted rows in tile c * tiles_per_chunk + j of BM rows (0 for a tile past the
    catalog's last).  Several queries at once, bool [..., n], give [..., n_chunks, tiles_per_chunk].  Computed from the
    inputs only: the preconditions of the faceted multi-tile tests."""
    admit_row = np.asarray(admit_row, bool)
    n = admit_row.shape[-1]
    n_tiles = (n + BM - 1) // BM
    n_chunks = (n_tiles + tiles_per_chunk - 1) // tiles_per_chunk
    padded = np.zeros(admit_row.shape[:-1] + (n_chunks * tiles_per_chunk * BM,), bool)
    padded[..., :n] = admit_row
    return padded.reshape(admit_row.shape[:-1] + (n_chunks, tiles_per_chunk, BM)).sum(axis=-1)


# ---------------------------------------------------------------- the filter pass's launch plan, in numpy
FILTER_MIN_Q, RES_QCAP_MAX_ROUNDS, LDS_MAX = 256, 64, 160 * 1024   # csrc/search.hip's constants of the same names


def filter_list_len(k):
    """Length of the filter pass's candidate lists for a search of k: k + 12, rounded up to a multiple of 8."""
    return (k + 12 + 7) & ~7


def filter_plan(n_rows, Q, n_cu, resident):
    """csrc/search.hip's make_filter_plan, the part that cuts the rows: the resident form (dim 384) walks rounds of 256
    rows with one block per CU, the staged form tiles of 128 rows with two; 64 queries per tile in both
    -> (BM, n_qtiles, tiles_per_chunk, n_chunks)."""
    BM = 256 if resident else 128
    n_qtiles = (Q + 63) // 64
    n_row_tiles = (n_rows + BM - 1) // BM
    want = min(max((1 if resident else 2) * n_cu // n_qtiles, 1), 256)
    want = min(want, n_row_tiles)
    tiles_per_chunk = (n_row_tiles + want - 1) // want
    return BM, n_qtiles, tiles_per_chunk, (n_row_tiles + tiles_per_chunk - 1) // tiles_per_chunk


def resident_lds(kp, facet):
    """Dynamic LDS of the resident filter pass at list length kp (resident_smem / TopK<CfgRes, true, FACET>::bytes in
    csrc/search.hip): two query planes of 64 x 768 B | 64 thresholds (8 B) and queue counters (4 B) | 16 B of flags |
    FACET: 64 queries' masks of 2 x 8 words and 2 x 256 facet words of 2 B | 64 lists of kp keys | 64 queues sized for
    a block of ONE round: 32 slots up to kp = 32, else 16.  The pass is taken while this is at most LDS_MAX."""
    return 2 * 64 * 768 + 64 * (8 + 4) + 16 + (64 * 2 * 8 * 4 + 2 * 256 * 2 if facet else 0) + 64 * kp * 8 \
        + 64 * (32 if kp <= 32 else 16) * 8


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


def direction_catalog(order, n, dim, nq, seed):
    """Rows u + t d + noise along a unit direction d (u a unit vector across it), t from -1 to 1, and nq queries
    d + 0.02 noise: every query's score t / sqrt(1 + t^2) grows with t.  order "ascending": t grows with the row number,
    "descending": falls, "random": shuffled.  The row noise is 1 / n per component, about half the score step between
    neighbouring rows at the flat ends of the curve (0.35 * 2 / n): neighbours swap places, a tile does not overlap
    the tile before it.  -> (P [n, dim], q [nq, dim]), float32, read-only."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal(dim).astype(np.float32)
    d /= np.linalg.norm(d)
    u = rng.standard_normal(dim).astype(np.float32)
    u -= u.dot(d) * d
    u /= np.linalg.norm(u)
    t = np.linspace(-1.0, 1.0, n, dtype=np.float32)
    if order == "descending":
        t = t[::-1]
    elif order == "random":
        t = rng.permutation(t)
    else:
        assert order == "ascending", order
    P = u[None, :] + t[:, None] * d[None, :] + np.float32(1.0 / n) * rng.standard_normal((n, dim), dtype=np.float32)
    q = d[None, :] + np.float32(0.02) * rng.standard_normal((nq, dim), dtype=np.float32)
    return _frozen(P), _frozen(q)


def tie_run_catalog(n, dim, nq, BM, tiles_per_chunk, run_len, seed):
    """Random rows with three runs of run_len copies of ONE row b, placed against the blocks of tiles_per_chunk tiles
    of BM rows that a tiled kernel walks: run 0 has its first run_len - 7 copies at the end of block 1's first tile
    and 7 in its second, run 1 starts 7 rows before the middle block boundary and goes on in the next block, run 2
    lies inside the last, ragged tile.  The queries are b + w + 0.05 noise with w a unit vector across b, and 47 near
    rows b + g w sit in block 1: for 0 < g < 1 such a row scores above b for every query, for g < 0 below it (fp32
    rows; bfloat16 rounding blurs the smallest steps).  16 near rows, 8 above b and 8 below, lie in the block's third
    tile.  31 lie in its first tile at the rows r < 64 with r % 8 < 4 - the 32 scores that ONE lane holds per query
    (first_pass_offers) - n_above of them above b, n_above = 20 for runs longer than 128 and 10 otherwise: more than
    the m scores a lane offers in the first pass of a cold tile at every k the tiled kernels take up to run_len - 7.
    The 32nd of those rows, r = 17, is one more copy of b, the stray: its lane does not offer it in the first pass,
    while the run_len - 7 >= k copies of run 0 in the same tile, top scores of their own lanes, are all offered.  The
    k-th key after the first pass is then a copy of b with a HIGHER row number than the stray, which enters in the
    second pass on a score EQUAL to the threshold's and belongs in front of every other copy.  Near rows, stray and
    runs are every query's best matches, and among the equal scores only the row number decides.
    -> (P, q, [(first row, end row) of each run], near rows, the stray's row), read-only."""
    rng = np.random.default_rng(seed)
    n_tiles = (n + BM - 1) // BM
    n_chunks = (n_tiles + tiles_per_chunk - 1) // tiles_per_chunk
    block = tiles_per_chunk * BM
    assert 7 < run_len <= BM - 57 and BM >= 128 and n_chunks >= 5 and tiles_per_chunk >= 3
    starts = [block + BM - (run_len - 7), (n_chunks // 2) * block - 7, (n_tiles - 1) * BM + 11]
    runs = [(s, s + run_len) for s in starts]
    assert runs[0][0] >= block + 64 and runs[2][1] <= n
    P = rng.standard_normal((n, dim), dtype=np.float32)
    base = rng.standard_normal(dim, dtype=np.float32)
    w = rng.standard_normal(dim).astype(np.float32)
    w -= w.dot(base) / base.dot(base) * base
    w /= np.linalg.norm(w)
    for lo, hi in runs:
        P[lo:hi] = base
    n_above = 20 if run_len > 128 else 10
    lane = rng.permutation([r for r in range(64) if r % 8 < 4 and r != 17])        # 31 rows of one lane
    third = rng.permutation(2 * BM + 5 + 7 * np.arange(16))                           # 16 rows of the third tile
    # g > 0, best first, dealt in turn to the third tile (8) and the lane (n_above); g < 0 likewise (8 and the rest)
    up = 0.8 * np.arange(n_above + 8, 0, -1) / (n_above + 8)
    down = -0.8 * np.arange(1, 31 - n_above + 8 + 1) / (31 - n_above + 8)
    rows_up = [third[i // 2] if i % 2 == 0 and i < 16 else None for i in range(n_above + 8)]
    rest = iter(lane[:n_above])
    rows_up = [r if r is not None else next(rest) for r in rows_up]
    rows_down = [third[8 + i // 2] if i % 2 == 0 and i < 16 else None for i in range(31 - n_above + 8)]
    rest = iter(lane[n_above:])
    rows_down = [r if r is not None else next(rest) for r in rows_down]
    near = block + np.asarray(rows_up + rows_down)
    P[near] = base[None, :] + np.concatenate([up, down]).astype(np.float32)[:, None] * w[None, :]
    stray = block + 17
    P[stray] = base
    q = (base + w)[None, :] + np.float32(0.05) * rng.standard_normal((nq, dim), dtype=np.float32)
    return _frozen(P), _frozen(q), runs, near, stray


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
