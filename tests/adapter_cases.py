"""Shared inputs of the adapter step's tests: the candidate lists of tests/test_adapter_gpu.py and the cases of
tests/test_adapter_edges_gpu.py - each names the path of csrc/adapt.hip it aims at, and tests/test_adapter_cases.py shows
without a GPU that it gets there - with their float64 and float32 references (tests/adapter_harness.py), computed once.
Importing this needs no GPU."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import adapter_reference as ref
from tests.adapter_harness import _frozen, small_delta, unit_rows
from tests.adapter_harness import references as references_of

# csrc/adapt.hip's tiling, restated: logits_kernel has one workgroup of WAVES waves per ANCHOR_TILE anchors, wave w walks
# the candidate tiles ct % WAVES == w of CAND_TILE candidates, sweep 2 sums GROUP_TILES tiles (GROUP candidates) as one
# chain, a wave owns the feature tiles t % WAVES == w of FEATURE_TILE features (at most MAX_OWN_TILES of them);
# grad_kernel adds blocks of GRAD_BLOCK anchors, its last workgroup the anchors' losses
ANCHOR_TILE, CAND_TILE, GROUP_TILES, GRAD_BLOCK, WAVES, FEATURE_TILE, MAX_OWN_TILES = 32, 32, 4, 64, 4, 32, 8
GROUP = GROUP_TILES * CAND_TILE
MAX_DIM, MAX_BATCH, MAX_CANDIDATES = 1024, 1024, 8192  # include/icrec.h's ICREC_ADAPTER_MAX_*
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1


def candidates(kind, rng, B, C, n_rows):
    """The candidate rows of a case: distinct rows, or one of the special lists (B >= 8, C >= B + 4)."""
    cand = rng.choice(n_rows, C, replace=False) if C <= n_rows else rng.integers(0, n_rows, C)
    if kind == "repeated positives":
        cand[1] = cand[0]
        cand[B - 1] = cand[0]
        cand[5] = cand[4]
    elif kind == "negative equals a positive":
        cand[B] = cand[2]
        cand[B + 1] = cand[2]
        cand[C - 1] = cand[B - 1]
    elif kind == "ids out of range":
        cand[B] = -1
        cand[B + 2] = n_rows
        cand[C - 1] = 2**31 - 1
    elif kind == "positive out of range":
        cand[0] = n_rows
        cand[3] = -1
        cand[B - 1] = -(2**31)
    else:
        assert kind == "plain"
    return cand.astype(np.int64)


def masked_id_mix(rng, B, C, n_rows):
    """Every masking rule in one list (B >= 8, C >= B + 4): rows drawn with repeats, ids out of range among the positives
    and the negatives, a repeated positive, negatives that are copies of positives, rows n_rows - 1 and n_rows."""
    cand = rng.integers(0, n_rows, C).astype(np.int64)
    cand[4::17] = -1
    cand[6::29] = n_rows
    cand[1] = cand[0]
    cand[B + 1] = cand[2]
    cand[C - 1] = cand[B - 1]
    cand[B], cand[B + 2] = n_rows - 1, n_rows
    return cand


# ---------------------------------------------------------------- the masked-tile list
# B = 96 anchors are three anchor tiles, C = 416 candidates are thirteen candidate tiles in groups [0, 128), [128, 256),
# [256, 384) and [384, 416).  What the list holds, by position:
MASKED_B, MASKED_C, MASKED_ROWS = 96, 416, 1000
UNCOUNTED_ANCHOR_TILE = 1        # anchors 32 .. 63: every positive out of range (which also masks candidate tile 1 wholly)
MASKED_TILES = (1, 5)            # candidate tiles with nothing in range: all of wave 1's but tile 9 ..
MASKED_GROUP = 2                 # .. which lies in this group of 128: wave 1 meets no candidate at all
#: (position j, anchor i): cand[j] is a copy of anchor i's positive
COPY_OTHER_WAVE = (100, 5)       # tile 3 (wave 3) of the positive's own group
COPY_OTHER_GROUP = (229, 10)     # tile 7 (wave 3), group 1
COPY_LAST_GROUP = (391, 80)      # tile 12 (wave 0), group 3, of a positive in tile 2 (wave 2)
COPY_IS_A_POSITIVE = (70, 3)     # anchor 70's positive is anchor 3's: two anchor tiles, each masks the other's


def masked_tile_candidates(rng, n_rows=MASKED_ROWS):
    """The list above: distinct rows of (0, n_rows - 1) everywhere else, rows 0 and n_rows - 1 as positives and as
    negatives' neighbours, and a few single ids out of range inside tiles that are otherwise in range."""
    B, C = MASKED_B, MASKED_C
    cand = rng.choice(np.arange(1, n_rows - 1), C, replace=False).astype(np.int64)
    bad = np.resize(np.asarray([-1, n_rows, n_rows + 1, INT32_MAX, INT32_MIN, -7, 2 * n_rows], np.int64), C)
    for t in MASKED_TILES:
        cand[t * CAND_TILE:(t + 1) * CAND_TILE] = bad[t * CAND_TILE:(t + 1) * CAND_TILE]
    cand[MASKED_GROUP * GROUP:(MASKED_GROUP + 1) * GROUP] = bad[MASKED_GROUP * GROUP:(MASKED_GROUP + 1) * GROUP]
    assert UNCOUNTED_ANCHOR_TILE in MASKED_TILES and ANCHOR_TILE == CAND_TILE
    cand[0], cand[B - 1] = 0, n_rows - 1           # the first and the last row of the index, as positives
    cand[B + 3], cand[C - 1] = n_rows - 1, n_rows  # .. and the last row beside the first one behind it
    cand[7], cand[B + 5], cand[C - 2] = -1, n_rows, -1   # single masked ids inside live tiles (anchor 7 is not counted)
    for j, i in (COPY_OTHER_WAVE, COPY_OTHER_GROUP, COPY_LAST_GROUP, COPY_IS_A_POSITIVE):
        cand[j] = cand[i]
    return cand


# ---------------------------------------------------------------- the cases
class Case(NamedTuple):
    name: str
    aim: str          # the path of adapt.hip the case is there for
    storage: str
    dim: int
    B: int
    C: int
    n_rows: int
    scales: tuple = (30.0,)
    cand: str = "plain"       # "plain" | "masked tiles"
    delta: float = 0.05       # D's entries are delta / sqrt(dim) x a standard normal
    norms: tuple = (1.0, 1.0)  # the anchors' lengths run log-evenly between these, shuffled


EDGE_CASES = (
    Case("batch-limit", "every anchor tile, 16 anchor blocks, ls[1024]", "f32", 32, 1024, 1024, 3000),
    Case("both-limits", "the benchmarked shape at the narrowest rows", "f32", 32, 1024, 8192, 10000),
    Case("batch-off-its-edges", "B = 4 * 64 + 1: one anchor in the 9th tile and in the 5th block", "bf16", 64, 257, 300, 3000),
    Case("widest-f32", "own feature tiles tt = 0 .. 7, a second group of one tile", "f32", 1024, 33, 130, 600),
    Case("widest-bf16", "own feature tiles tt = 0 .. 7, a second group of one tile", "bf16", 1024, 33, 130, 600),
    Case("wide-f32", "f32 rows wider than 384: tt = 0 .. 5", "f32", 768, 40, 257, 1000),
    Case("narrow-bf16", "bf16 rows narrower than 384: waves 2 and 3 own no feature tile", "bf16", 64, 33, 40, 3000),
    Case("one-anchor", "B = 1 with real negatives: 63 idle anchor lanes, pu clamped to B - 1", "f32", 64, 1, 200, 3000),
    Case("masked-tiles-f32", "masked tiles, groups and anchor tiles, far copies of positives", "f32", 96, MASKED_B, MASKED_C,
         MASKED_ROWS, (30.0, 100.0), "masked tiles"),
    Case("masked-tiles-bf16", "masked tiles, groups and anchor tiles, far copies of positives", "bf16", 128, MASKED_B,
         MASKED_C, MASKED_ROWS, (30.0, 100.0), "masked tiles"),
    Case("trained-size-D", "a D of the size training produces: z is not about a", "f32", 384, 65, 100, 3000, delta=0.5),
    Case("anchor-norms", "anchors of lengths 1e-3 .. 1e3: the loss is defined through n_i", "f32", 384, 65, 100, 3000,
         norms=(1e-3, 1e3)),
)
CASE_BY_NAME = {c.name: c for c in EDGE_CASES}
STEPS = [(c.name, s) for c in EDGE_CASES for s in c.scales]  # every (case, scale) the GPU test runs


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """(P float32 [n_rows, dim] as given to the index, the rows it stores, anchors [B, dim], D [dim, dim], cand int64 [C])
    of a case, drawn from a seed that is the case's position in EDGE_CASES; read-only."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng(9000 + EDGE_CASES.index(c))
    P = unit_rows(rng, c.n_rows, c.dim)
    anchors = unit_rows(rng, c.B, c.dim)
    if c.norms != (1.0, 1.0):
        lengths = np.geomspace(c.norms[0], c.norms[1], c.B)
        anchors = (anchors * rng.permutation(lengths)[:, None]).astype(np.float32)
    delta = (small_delta(rng, c.dim) * np.float32(c.delta / 0.05)).astype(np.float32)
    cand = masked_tile_candidates(rng, c.n_rows) if c.cand == "masked tiles" else candidates("plain", rng, c.B, c.C, c.n_rows)
    assert cand.shape == (c.C,)
    return _frozen(P, ref.stored_rows(P, c.storage), anchors, delta, cand)


references = functools.partial(references_of, "pairs", inputs)  # (name, scale) -> float64 and float32 loss and gradient
