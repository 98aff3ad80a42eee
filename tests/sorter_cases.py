"""The crafted searches of tests/test_sorters_gpu.py that reach merge_block_kernel (csrc/sort.hip) and its eligibility
edge, with the conditions on their inputs, and the key lists of the direct icrec_merge_topk cases.  numpy only:
tests/test_sorters.py checks the conditions without a GPU (at 256 CUs), the GPU test asserts them again from the
oracle's scores and the device's CU count."""
from __future__ import annotations

import functools

import numpy as np

from tests.search_harness import _frozen, direction_catalog, pack_keys, select_from_scores

MAX_Q = 4
ROW_OFFSET = 1000

# name: (catalog order, rows, width, row storage, the query counts, {k: merge form}, kernel, lists, the condition on C
#        per k (None: none), the query WITHOUT an exclusion list)
# C = block_merge_candidates: merge_block_kernel's ranking loop takes a second trip iff C > 256, a third iff C > 512.
SEARCH_CASES = {
    # eligibility edge behind the streaming kernel: 256 lists x 16 keys fill the block merge's 4,096 slots exactly
    "edge-stream-256": ("random", 65_536, 32, "f32", (1, 2), {16: "block", 17: "wave4"}, "stream", 256, {}, 1),
    # 257 lists: merge_kernel<16>; list 256 is ONE row, a copy of query 0 (which therefore excludes nothing)
    "edge-stream-257": ("random+copy", 65_537, 32, "f32", (1, 2), {8: "wave16"}, "stream", 257, {}, 0),
    # eligibility edge behind CfgSmall (Qpad = 32, so the lists' query stride is not Q) at the product's 195 lists
    "edge-tiled-ascending": ("ascending", 49_688, 32, "f32", (3, 4), {20: "block", 21: "block", 22: "wave4"}, "small",
                             195, {20: ">256", 21: ">256"}, 1),
    "edge-tiled-random": ("random", 49_688, 32, "f32", (3, 4), {20: "block", 21: "block", 22: "wave4"}, "small", 195,
                          {20: "<=256", 21: "<=256"}, 1),
    # many candidates: (k - 1) k + 1 = 4,033 of the 4,096 keys, and ALL keys where there are fewer lists than k
    "many-64x64-ascending": ("ascending", 64 * 256, 64, "f32", (1, 2), {64: "block"}, "stream", 64, {64: ">=513"}, 1),
    "many-64x64-descending": ("descending", 64 * 256, 64, "f32", (1, 2), {64: "block"}, "stream", 64, {64: ">=513"}, 1),
    "many-32x128-ascending": ("ascending", 32 * 256, 32, "f32", (1, 2), {128: "block"}, "stream", 32, {128: ">=513"}, 1),
    "many-32x128-descending": ("descending", 32 * 256, 32, "f32", (1, 2), {128: "block"}, "stream", 32, {128: ">=513"}, 1),
    "many-64x64-ascending-bf16": ("ascending", 64 * 256, 64, "bf16", (1, 2), {64: "block"}, "stream", 64, {64: ">=513"}, 1),
}


def holds(C, condition):
    return {">=513": C >= 513, ">256": C > 256, "<=256": C <= 256, None: True}[condition]


@functools.lru_cache(maxsize=None)
def search_case_inputs(name):
    """(P [n, dim], q [MAX_Q, dim]) of one case, float32 and read-only; a case of Q queries takes the first Q."""
    order, n, dim = SEARCH_CASES[name][:3]
    seed = 7000 + sorted(SEARCH_CASES).index(name)
    if order == "random+copy":
        P, q = direction_catalog("random", n - 1, dim, MAX_Q, seed)
        return _frozen(np.concatenate([P, q[:1]])), q
    return direction_catalog(order, n, dim, MAX_Q, seed)


def search_case_exclusions(name, scores):
    """One list per query from the [MAX_Q, n] score matrix of the case: every query excludes its own best, third and
    sixth row and 10 random rows, but the case's one query that excludes nothing."""
    n, none_query = SEARCH_CASES[name][1], SEARCH_CASES[name][9]
    rng = np.random.default_rng(len(name))
    top8 = select_from_scores(scores, 8)[0]
    return [[] if i == none_query else
            sorted(set(top8[i, [0, 2, 5]].tolist()) | set(rng.choice(n, 10, replace=False).tolist()))
            for i in range(scores.shape[0])]


def numpy_scores(P, q):
    """Cosine scores [Q, n] in plain float32 numpy (normalise, then one matrix product): not the library's chains,
    close enough for conditions on the inputs that hold with a wide margin."""
    unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), np.float32(1e-12))  # noqa: E731
    return (unit(np.asarray(q, np.float32)) @ unit(np.asarray(P, np.float32)).T).astype(np.float32)


# ---------------------------------------------------------------- icrec_merge_topk: shapes and key lists
# n_lists: the (Q, k) pairs; 64 s + lane boundaries of the tournament, the template arms' edge at 256, the cap at 1,024
MERGE_SHAPES = {
    1: [(1, 1), (5, 128)],
    2: [(3, 20), (4, 1)],
    63: [(1, 20), (9, 128)],
    64: [(3, 128), (4, 20)],
    65: [(5, 1), (4, 128)],
    255: [(3, 20), (1, 128)],
    256: [(9, 20), (4, 128)],
    257: [(5, 20), (4, 1)],
    1023: [(3, 128), (4, 20)],
    1024: [(9, 20), (1, 128), (5, 1)],
}
MERGE_PATTERNS = ("ties", "last-list", "short", "pad-lists", "edge-values")
SPECIAL_SCORES = np.asarray([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38,
                             3.4028235e38, -3.4028235e38, 1.1754944e-38, 1.0, -1.0], np.float32)


def merge_case_keys(pattern, n_lists, Q, k, seed):
    """keys uint64 [n_lists, Q, k] for icrec_merge_topk: per (list, query) sorted descending, unique per query, pads
    (key 0) at the tail.  Rows are base + list * k + slot, so a row names its list.
    ties:        every list full; scores drawn from 5 values, so among thousands of equal scores the row decides
    last-list:   every list empty except list n_lists - 1, whose k keys are the answer
    short:       fewer than k real keys in total (none at k = 1), scattered over the lists: the answer ends in pads
    pad-lists:   every third list (0, 3, ...) all pads, the others cut to a random length 1 .. k
    edge-values: every list full; rows from 4,000,000,000; scores include +-0, +-inf, denormals, the largest and the
                 smallest normal numbers"""
    rng = np.random.default_rng(seed)
    shape = (n_lists, Q, k)
    base = 4_000_000_000 if pattern == "edge-values" else 0
    rows = base + (np.arange(n_lists, dtype=np.int64)[:, None, None] * k + np.arange(k, dtype=np.int64)[None, None, :])
    if pattern == "ties":
        scores = rng.choice(np.asarray([-0.5, 0.25, 0.25000003, 0.75, 0.0], np.float32), size=shape)
    elif pattern == "edge-values":
        scores = np.where(rng.random(shape) < 0.5, rng.choice(SPECIAL_SCORES, size=shape),
                          rng.standard_normal(shape, dtype=np.float32))
    else:
        scores = rng.standard_normal(shape, dtype=np.float32)
    keys = np.sort(pack_keys(scores, rows), axis=2)[:, :, ::-1].copy()
    length = np.full((n_lists, Q), k, np.int64)
    if pattern == "last-list":
        length[:-1] = 0
    elif pattern == "short":
        length[:] = 0
        for i in range(Q):
            total = int(rng.integers(0, k))   # 0 .. k - 1 real keys
            np.add.at(length[:, i], rng.integers(0, n_lists, size=total), 1)
    elif pattern == "pad-lists":
        length = rng.integers(1, k + 1, size=(n_lists, Q))
        length[::3] = 0
    keys[np.arange(k)[None, None, :] >= length[:, :, None]] = 0
    return keys
