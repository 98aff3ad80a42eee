"""Shared inputs of the adapter step's tests: the seeded catalog / anchor / D draws, the candidate lists of
tests/test_adapter_gpu.py, the cases of tests/test_adapter_edges_gpu.py - each names the path of csrc/adapt.hip it aims
at, and tests/test_adapter_cases.py shows without a GPU that it gets there - their float64 and float32 references,
computed once, and the one comparison of a device step with them.  Importing this needs no GPU."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

from tests import adapter_reference as ref
from tests.token_states import check

# csrc/adapt.hip's tiling, restated: logits_kernel has one workgroup of WAVES waves per ANCHOR_TILE anchors, wave w walks
# the candidate tiles ct % WAVES == w of CAND_TILE candidates, sweep 2 sums GROUP_TILES tiles (GROUP candidates) as one
# chain, a wave owns the feature tiles t % WAVES == w of FEATURE_TILE features (at most MAX_OWN_TILES of them);
# grad_kernel adds blocks of GRAD_BLOCK anchors, its last workgroup the anchors' losses
ANCHOR_TILE, CAND_TILE, GROUP_TILES, GRAD_BLOCK, WAVES, FEATURE_TILE, MAX_OWN_TILES = 32, 32, 4, 64, 4, 32, 8
GROUP = GROUP_TILES * CAND_TILE
MAX_DIM, MAX_BATCH, MAX_CANDIDATES = 1024, 1024, 8192  # include/icrec.h's ICREC_ADAPTER_MAX_*
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def small_delta(rng, d):
    return (rng.standard_normal((d, d)) * (0.05 / np.sqrt(d))).astype(np.float32)


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


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


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


@functools.lru_cache(maxsize=None)
def references(name: str, scale: float):
    """(float64 loss, float64 gradient, float32 loss, float32 gradient) of a case by tests/adapter_reference.py."""
    _, rows, anchors, delta, cand = inputs(name)
    want = ref.loss_and_grad(delta, anchors, rows, cand, scale, torch.float64)
    ref32 = ref.loss_and_grad(delta, anchors, rows, cand, scale, torch.float32)
    _frozen(want[1], ref32[1])
    return want[0], want[1], ref32[0], ref32[1]


# ---------------------------------------------------------------- the comparison
def loss_floor(want_loss: float) -> float:
    """Half a float32 ulp of the loss: a float32 value is in general that far off, whatever luck the float32
    reference had on one draw."""
    return float(np.spacing(np.float32(abs(want_loss)))) / 2


def check_step(what: str, loss: float, grad: np.ndarray, want_loss, want_grad, ref_loss, ref_grad, margin) -> None:
    """A device step's loss and gradient against the float64 reference: prints the RATIO lines, then asserts
    E_gpu <= margin x E_ref for the gradient's worst row rms, its max-abs and the loss (E_ref the float32 reference's
    error on the same input, for the loss never below half a float32 ulp)."""
    assert np.isfinite(loss) and np.isfinite(grad).all(), what
    e_ref = max(abs(ref_loss - want_loss), loss_floor(want_loss))
    e_gpu = abs(loss - want_loss)
    print(f"RATIO {what} loss: E_gpu {e_gpu:.3e}, E_ref {e_ref:.3e}, ratio {e_gpu / e_ref:.2f} (margin {margin})")
    check(what + " grad", grad, want_grad, ref_grad, (margin, margin))
    assert e_gpu <= margin * e_ref, what


# ---------------------------------------------------------------- AdamW
#: lr, beta1, beta2, eps, weight_decay as the float arguments the C ABI carries
ADAMW_HYPER = tuple(float(np.float32(x)) for x in (1e-2, 0.9, 0.999, 1e-8, 0.01))


def adamw_inputs(d: int):
    """(P [500, d], anchors [40, d], cand int64 [64], D, m, v) of the tile-mapping test at width d: random moments of the
    sizes tests/test_adapter_gpu.py's AdamW test uses, for a step from t = 7."""
    rng = np.random.default_rng(47 + d)
    P, anchors = unit_rows(rng, 500, d), unit_rows(rng, 40, d)
    cand = rng.choice(500, 64, replace=False).astype(np.int64)
    delta = small_delta(rng, d)
    m = (rng.standard_normal((d, d)) * 1e-3).astype(np.float32)
    v = (rng.random((d, d)) * 1e-5).astype(np.float32)
    return P, anchors, cand, delta, m, v


def adamw_float32(delta, m, v, t, g, lr, b1, b2, eps, wd):
    """grad_kernel's epilogue in numpy float32, one rounding per operation, with the host's double bias corrections
    rounded to float32 as icrec_adapter_step passes them -> (delta, m, v) after step t + 1."""
    F = np.float32
    delta, m, v, g = (np.asarray(a, F) for a in (delta, m, v, g))
    t1 = float(t + 1)
    omb1, omb2, decay = F(1.0 - b1), F(1.0 - b2), F(1.0 - lr * wd)
    bc1, sbc2 = F(1.0 - b1 ** t1), F(np.sqrt(1.0 - b2 ** t1))
    m1 = m + (g - m) * omb1
    v1 = v * F(b2) + omb2 * g * g
    p = delta * decay - (F(lr) / bc1) * (m1 / (np.sqrt(v1) / sbc2 + F(eps)))
    assert p.dtype == m1.dtype == v1.dtype == F
    return p, m1, v1


def adamw_bound_use(before: dict, g: np.ndarray, after: dict):
    """How much of its bound each element of an AdamW step uses, against the float64 formula (ref.adamw) ->
    (D under the bound below, m, v, D under test_adapter_gpu's form of the bound, t).  The bound is that test's: eight
    roundings in the formula, each half an ulp of a magnitude bounded by the terms added - derived, not measured.  For m
    the terms added are |m| + (1 - beta1) |g - m|, for v beta2 |v| + (1 - beta2) g^2, for D |D| and the Adam term.  The
    Adam term is k m1, k = (lr / bc1) / (sqrt(v_hat) + eps), and m1 is rounded relative to the terms IT is added from,
    not to itself, so its magnitude here is k (|m| + (1 - beta1) |g - m|): the same value as test_adapter_gpu's |term|
    wherever m and (g - m)(1 - beta1) have one sign (always at m = 0), larger only where they cancel - there |k m1|
    does not cover m1's own rounding (tests/test_adapter_cases.py: the formula in IEEE float32 on the host misses that
    form on some hundred of the 1,048,576 elements at d = 1024, and meets this one everywhere)."""
    lr, b1, b2, eps, wd = ADAMW_HYPER
    delta, m, v = before["delta"], before["m"], before["v"]
    want_delta, want_m, want_v, t, term = ref.adamw(delta, m, v, before["t"], g, lr, b1, b2, eps, wd)
    u = 8 * 2.0**-24
    g64, m64 = g.astype(np.float64), m.astype(np.float64)
    added_to_m = np.abs(m64) + (1 - b1) * np.abs(g64 - m64)
    k = (lr / (1.0 - b1 ** t)) / (np.sqrt(want_v) / np.sqrt(1.0 - b2 ** t) + eps)
    tiny = np.finfo(np.float64).tiny  # (0 / 0 where nothing is added and nothing is off: an element without gradient)
    err = np.abs(after["delta"] - want_delta)
    return (err / np.maximum(u * (np.abs(delta) + k * added_to_m), tiny),
            np.abs(after["m"] - want_m) / np.maximum(u * added_to_m, tiny),
            np.abs(after["v"] - want_v) / np.maximum(u * (b2 * np.abs(v) + (1 - b2) * g64 ** 2), tiny),
            err / np.maximum(u * (np.abs(delta) + np.abs(term)), tiny), t)


def assert_adamw(before: dict, g: np.ndarray, after: dict) -> None:
    """`after` is torch's AdamW step on `before` with gradient g within adamw_bound_use's bounds."""
    use_delta, use_m, use_v, _, t = adamw_bound_use(before, g, after)
    assert after["t"] == t == before["t"] + 1
    assert use_delta.max() <= 1 and use_m.max() <= 1 and use_v.max() <= 1, (use_delta.max(), use_m.max(), use_v.max())
