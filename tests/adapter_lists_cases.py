"""Shared inputs of the tests of icrec_adapter_step_lists: the cases - each names the path of csrc/adapt.hip's
lists_plan_kernel / lists_kernel it aims at, and tests/test_adapter_lists.py shows without a GPU, from the reference's
masks, that it gets there - with their float64 and float32 references (tests/adapter_harness.py), computed once.
Importing this needs no GPU."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import adapter_reference as ref
from tests.adapter_harness import _frozen, small_delta, unit_rows
from tests.adapter_harness import references as references_of

# csrc/adapt.hip's shape of the step, restated: a wave of lists_kernel scores SCORE_DEPTH entries at once and the four
# waves walk the list in strides of WAVES * SCORE_DEPTH; a lane sums entries lane, lane + 64, ..; sweep 2 loads DEPTH
# entries at once and adds groups of GROUP; grad_kernel adds blocks of GRAD_BLOCK anchors
WAVES, SCORE_DEPTH, DEPTH, GROUP, GRAD_BLOCK = 4, 4, 8, 128, 64
MAX_LIST, MAX_BATCH = 1024, 1024  # include/icrec.h's ICREC_ADAPTER_MAX_LIST, ICREC_ADAPTER_MAX_BATCH
GAINS = np.asarray([0, 0, 0, 0, 1, 2, 4], np.float32)  # the default gains of the four event types, mostly impressions
EDGE_LENGTHS = (1, 2, 63, 64, 65, 100)


class Case(NamedTuple):
    name: str
    aim: str          # the path the case is there for
    storage: str
    dim: int
    B: int
    n_rows: int
    lists: str        # the builder below
    L: int = 100      # the (longest) list
    scales: tuple = (30.0,)
    delta: float = 0.05
    max_len: int = 0  # 0: the longest list


CASES = (
    Case("w32-f32", "8 pieces of a row: 56 lanes of a scoring wave own nothing", "f32", 32, 33, 600, "uniform"),
    Case("w96-f32", "24 pieces; lists of 63: a last scoring group of 3, a partial sweep-2 round", "f32", 96, 65, 600, "uniform", 63),
    Case("w384-f32", "96 pieces: lanes 0-31 own two; B = 4 * 64 + 1; lists of 65", "f32", 384, 257, 2048, "uniform", 65, (30.0, 100.0)),
    Case("w1024-f32", "256 pieces: every thread of sweep 2 owns one, a lane four", "f32", 1024, 33, 300, "uniform", 64),
    Case("w64-bf16", "B = 1: one workgroup, counted = 1; 8 pieces of 8 features", "bf16", 64, 1, 600, "uniform"),
    Case("w384-bf16", "every kind of dropped entry and segment in one batch", "bf16", 384, 65, 600, "mixed", 100, (30.0, 100.0)),
    Case("w768-bf16", "96 pieces of 8 features; lists of 2", "bf16", 768, 33, 600, "uniform", 2),
    Case("edge-lengths", "lists of 1, 2, 63, 64, 65 and 100 in one batch", "f32", 96, 33, 600, "lengths"),
    Case("head-only", "segments of 150 read to max_len = 100: what lies behind the head is poison", "f32", 96, 33, 600, "long heads",
         150, max_len=100),
    Case("batch-limit", "B = 1,024: every block of grad_kernel, 1,024 flags counted", "f32", 32, 1024, 3000, "uniform", 8),
    Case("list-limit", "L = 1,024: LDS arrays full, eight sweep-2 groups, 16 entries per lane", "f32", 32, 4, 2048, "uniform", 1024),
    Case("trained-size-D", "a D of the size training produces: z is not about a", "f32", 384, 65, 2048, "uniform", 100, delta=0.5),
)
CASE_BY_NAME = {c.name: c for c in CASES}
STEPS = [(c.name, s) for c in CASES for s in c.scales]


def uniform_lists(rng, B, L, n_rows):
    """B lists of L distinct in-range rows with gains from GAINS, at least one positive gain each."""
    rows = np.stack([rng.choice(n_rows, L, replace=False) for _ in range(B)])
    gains = rng.choice(GAINS, (B, L))
    gains[np.arange(B), rng.integers(0, L, B)] = 4.0
    return ref.uniform_csr(rows, gains)


def length_lists(rng, B, n_rows):
    """Lists whose lengths cycle through EDGE_LENGTHS (a list of one entry has loss and gradient zero)."""
    off, rows, target = [0], [], []
    for i in range(B):
        L = EDGE_LENGTHS[i % len(EDGE_LENGTHS)]
        rows.extend(rng.choice(n_rows, L, replace=False))
        g = rng.choice(GAINS, L)
        g[rng.integers(0, L)] = 2.0
        target.extend(g)
        off.append(len(rows))
    return np.asarray(off, np.int64), np.asarray(rows, np.int64), np.asarray(target, np.float32), max(EDGE_LENGTHS)


#: anchors of the mixed batch by what their list holds
MIXED = {"empty": 3, "reversed": 5, "all zero targets": 7, "all dropped": 9, "edge rows": 11, "bad targets": 13,
         "duplicate": 15, "one live among dropped": 17, "probabilities": 19}


def mixed_lists(rng, B, L, n_rows):
    """Mixed lengths 1 .. L, and at the anchors of MIXED: an empty segment, a segment whose end lies before its start,
    targets 0 everywhere, no live entry at all, rows 0 / n_rows - 1 / n_rows / -1, targets NaN / -1 / +inf / -0.0, a row
    listed twice, one live entry among dropped ones, a teacher's probabilities."""
    off, rows, target = np.zeros(B + 1, np.int64), [], []
    for i in range(B):
        n = int(rng.integers(1, L + 1))
        r = rng.choice(n_rows, n, replace=False).astype(np.int64)
        g = rng.choice(GAINS, n).astype(np.float32)
        g[rng.integers(0, n)] = 1.0
        if i == MIXED["empty"]:
            r, g = r[:0], g[:0]
        elif i == MIXED["all zero targets"]:
            g[:] = 0.0
        elif i == MIXED["all dropped"]:
            r[::2], g[1::2] = n_rows, np.nan
        elif i == MIXED["edge rows"]:
            r, g = np.concatenate([[0, n_rows - 1, n_rows, -1, 2**31 - 1, -(2**31)], r]), np.concatenate([[2, 1, 4, 4, 4, 4], g])
        elif i == MIXED["bad targets"]:
            r = np.concatenate([r, rng.choice(n_rows, 5, replace=False)])
            g = np.concatenate([g, [np.nan, -1.0, np.inf, -np.inf, -0.0]])
        elif i == MIXED["duplicate"]:
            r, g = np.concatenate([r, r[:2]]), np.concatenate([g, [4.0, 0.0]])
        elif i == MIXED["one live among dropped"]:
            r, g = np.asarray([-1, 5, n_rows, 7], np.int64), np.asarray([1.0, 3.0, 1.0, np.nan], np.float32)
        elif i == MIXED["probabilities"]:
            g = rng.dirichlet(np.ones(n)).astype(np.float32)
        if i == MIXED["reversed"]:  # its end lies 3 entries BEFORE its start, and nothing is appended for it: the next
            off[i + 1] = off[i] - 3  # segment begins there, so its first three entries are the tail of the one before
            continue
        rows.extend(r)
        target.extend(g)
        off[i + 1] = len(rows)
    rows, target = np.asarray(rows, np.int64), np.asarray(target, np.float32)
    assert off.max() <= len(rows) and off.min() >= 0
    return off, rows, target, int(np.clip(np.diff(off), 0, None).max())


def long_head_lists(rng, B, L, n_rows, max_len):
    """Segments of L > max_len entries: the head as uniform_lists draws it, behind it rows out of range and in range
    with huge gains, which would change everything if they were read."""
    off, rows, target, _ = uniform_lists(rng, B, L, n_rows)
    rows, target = rows.reshape(B, L).copy(), target.reshape(B, L).copy()
    target[:, max_len:] = 1e6
    rows[:, max_len::2] = n_rows + 5
    return off, rows.reshape(-1), target.reshape(-1), max_len


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """(P float32 [n_rows, dim] as given to the index, the rows it stores, anchors [B, dim], D [dim, dim], the lists
    (off, rows, target, max_len)) of a case, drawn from a seed that is the case's position in CASES; read-only."""
    c = CASE_BY_NAME[name]
    rng = np.random.default_rng(7000 + CASES.index(c))
    P = unit_rows(rng, c.n_rows, c.dim)
    anchors = unit_rows(rng, c.B, c.dim)
    delta = (small_delta(rng, c.dim) * np.float32(c.delta / 0.05)).astype(np.float32)
    if c.lists == "uniform":
        lists = uniform_lists(rng, c.B, c.L, c.n_rows)
    elif c.lists == "lengths":
        lists = length_lists(rng, c.B, c.n_rows)
    elif c.lists == "mixed":
        lists = mixed_lists(rng, c.B, c.L, c.n_rows)
    else:
        assert c.lists == "long heads"
        lists = long_head_lists(rng, c.B, c.L, c.n_rows, c.max_len)
    _frozen(P, anchors, delta, *lists[:3])
    return P, _frozen(ref.stored_rows(P, c.storage))[0], anchors, delta, lists


references = functools.partial(references_of, "lists", inputs)  # (name, scale) -> float64 and float32 loss and gradient
