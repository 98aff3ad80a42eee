"""Shared inputs of the whole-catalog adapter step's tests: csrc/adapt.hip's split rule restated, the cases of
tests/test_adapter_catalog_gpu.py - each names the path it aims at, and tests/test_adapter_catalog.py shows without a GPU
that it gets there - and their float64 and float32 references (tests/adapter_harness.py), computed once.  Importing this needs no GPU."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import adapter_reference as ref
from tests.adapter_cases import ANCHOR_TILE, INT32_MAX, INT32_MIN, MAX_BATCH
from tests.adapter_harness import _frozen, small_delta, unit_rows
from tests.adapter_harness import references as references_of

# csrc/adapt.hip's cut of the catalog, restated: the rows are walked in groups of GROUP (a 32-row tile per wave); the
# middle kernels run on (anchor tiles x splits) workgroups, as many splits as bring that product to TARGET_WORKGROUPS,
# at most MAX_SPLITS and at most one per group; every split is the same whole number of groups.
GROUP, TARGET_WORKGROUPS, MAX_SPLITS = 128, 512, 512
CATALOG_ROWS = 49688  # the catalog this project serves


def plan(B: int, n_rows: int) -> tuple[int, int]:
    """(n_splits, rows_per_split) of a catalog step: icrec_adapter_catalog_plan."""
    groups = -(-n_rows // GROUP)
    tiles = -(-B // ANCHOR_TILE)
    want = min(-(-TARGET_WORKGROUPS // tiles), MAX_SPLITS, groups)
    per_split = -(-groups // want)
    return -(-groups // per_split), per_split * GROUP


def last_split_rows(B: int, n_rows: int) -> int:
    n_splits, per_split = plan(B, n_rows)
    return n_rows - (n_splits - 1) * per_split


class Case(NamedTuple):
    name: str
    aim: str          # the path of adapt.hip the case is there for
    storage: str
    dim: int
    B: int
    n_rows: int
    scales: tuple = (30.0,)
    labels: str = "plain"  # "plain" | "edges" | "far maximum"


CASES = (
    Case("one-tile", "one split, one group, less than one tile of rows: three waves without a tile", "f32", 32, 2, 5),
    Case("two-splits", "two splits of one group, the second 72 rows", "f32", 32, 40, 200),
    Case("whole-splits", "three splits, every one exactly a group", "f32", 96, 33, 384),
    Case("one-row-over", "a last split of 1 row", "f32", 96, 33, 385),
    Case("one-row-short", "a last split one row short of full", "f32", 96, 33, 383),
    Case("most-splits", "the maximum number of splits, 512; the last one three rows short", "f32", 32, 2, 512 * GROUP - 3),
    Case("f32-384", "the served width, three anchor tiles, 24 splits", "f32", 384, 65, 3000, (30.0, 20.0, 100.0)),
    Case("bf16-384", "the served width in bf16", "bf16", 384, 31, 3000),
    Case("bf16-768", "six feature tiles per wave", "bf16", 768, 40, 1500, (30.0, 100.0)),
    Case("widest-f32", "own feature tiles tt = 0 .. 7; four features per finishing thread", "f32", 1024, 33, 700),
    Case("widest-bf16", "own feature tiles tt = 0 .. 7; four features per finishing thread", "bf16", 1024, 33, 700),
    Case("batch-limit", "every anchor tile; splits of two groups; the merge kernel's 1,024 threads all busy", "f32", 32, 1024, 3000),
    Case("batch-off-its-edges", "B = 4 * 64 + 1: one anchor in the 9th tile; waves 2 and 3 own no feature tile", "bf16", 64, 257, 2100),
    Case("one-anchor", "B = 1: 63 idle anchor lanes, pu clamped to B - 1", "f32", 64, 1, 2100),
    Case("catalog-f32", "the catalog's size: splits of three groups, the last one 56 rows into its first group", "f32", 384, 65, CATALOG_ROWS),
    Case("catalog-bf16", "the catalog's size in bf16", "bf16", 384, 65, CATALOG_ROWS),
    Case("labels-f32", "positives at rows 0 and n_rows - 1, shared, out of range; an anchor tile with nobody counted", "f32", 96,
         70, 385, (30.0,), "edges"),
    Case("labels-bf16", "the same labels over bf16 rows", "bf16", 64, 70, 2100, (30.0,), "edges"),
    Case("far-maximum-f32", "the best row in the last split and the positive in the first, and the reverse", "f32", 96, 33, 3000,
         (30.0, 100.0), "far maximum"),
    Case("far-maximum-bf16", "the same over bf16 rows", "bf16", 128, 33, 3000, (100.0,), "far maximum"),
)
CASE_BY_NAME = {c.name: c for c in CASES}
STEPS = [(c.name, s) for c in CASES for s in c.scales]  # every (case, scale) the GPU test runs

#: "edges" (B >= 64): what the labels hold, by anchor
SHARED = (2, 3, 4, 66)                # anchors with one positive, in two anchor tiles
UNCOUNTED = {6: "n_rows", 7: -1, 8: INT32_MAX, 9: INT32_MIN}
UNCOUNTED_ANCHOR_TILE = 1             # anchors 32 .. 63: nobody counted
# "far maximum": row n_rows - 1 is a copy of anchor 0's u and anchor 0's positive is row 5; row 7 is a copy of anchor 1's
# u and anchor 1's positive is row n_rows - 10


def edge_labels(rng, B, n_rows):
    pos = rng.integers(1, n_rows - 1, B).astype(np.int64)
    pos[0], pos[1] = 0, n_rows - 1
    for i in SHARED:
        pos[i] = pos[SHARED[0]]
    for i, v in UNCOUNTED.items():
        pos[i] = n_rows if v == "n_rows" else v
    lo = UNCOUNTED_ANCHOR_TILE * ANCHOR_TILE
    pos[lo:lo + ANCHOR_TILE] = np.resize(np.asarray([-1, n_rows, n_rows + 1, INT32_MAX, INT32_MIN, -7], np.int64), ANCHOR_TILE)
    return pos


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """(P float32 [n_rows, dim] as given to the index, the rows it stores, anchors [B, dim], D [dim, dim], pos int64 [B])
    of a case, drawn from a seed that is the case's position in CASES; read-only."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng(12000 + CASES.index(c))
    P = unit_rows(rng, c.n_rows, c.dim)
    anchors, delta = unit_rows(rng, c.B, c.dim), small_delta(rng, c.dim)
    if c.labels == "edges":
        pos = edge_labels(rng, c.B, c.n_rows)
    else:
        pos = rng.integers(0, c.n_rows, c.B).astype(np.int64)
    if c.labels == "far maximum":  # rows that are copies of an anchor's u, far from its positive
        z = ref.apply(delta, anchors)
        u = z / np.linalg.norm(z, axis=1, keepdims=True)
        last = c.n_rows - 1
        assert plan(c.B, c.n_rows)[0] >= 8 and 7 < plan(c.B, c.n_rows)[1]
        P[last], pos[0] = u[0], 5
        P[7], pos[1] = u[1], last - 9
    return _frozen(P, ref.stored_rows(P, c.storage), anchors, delta, pos)


references = functools.partial(references_of, "catalog", inputs)  # (name, scale) -> float64 and float32 loss and gradient

assert all(c.B <= MAX_BATCH for c in CASES)
