"""tests/adapter_cases.py without a GPU: every case of tests/test_adapter_edges_gpu.py reaches the path of csrc/adapt.hip
it names - shown from tests/adapter_reference.masks and plain arithmetic on the kernels' tile sizes - has a counted
anchor, a finite float64 reference and a float32 reference whose gradient error is positive (tests/token_states.check
divides by it)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native
from tests import adapter_cases as ac
from tests import adapter_harness as h
from tests import adapter_reference as ref
from tests.token_states import row_errors


def tiles(n, tile):
    return -(-n // tile)


def case_masks(name):
    c = ac.CASE_BY_NAME[name]
    cand = ac.inputs(name)[4]
    return c, cand, ref.masks(cand, c.B, c.n_rows)


def wholly_masked(valid, width):
    """The multiples of `width` at which `width` candidates in a row are all out of range (whole tiles only)."""
    return [t for t in range(valid.size // width) if not valid[t * width:(t + 1) * width].any()]


def test_the_tile_sizes_are_the_kernels():
    src = (_native._PKG / "csrc" / "adapt.hip").read_text()
    for text in ("constexpr int ANCHOR_TILE = 32;", "constexpr int GRAD_BLOCK = 64;", "constexpr int LOGIT_THREADS = 256;",
                 "for (int g = 0; g < n_ct; g += LOGIT_WAVES)", "const int n_ct = (C + 31) / 32;", "const int n_ft = K / 32;"):
        assert text in src, text
    assert (ac.ANCHOR_TILE, ac.CAND_TILE, ac.GROUP_TILES, ac.GRAD_BLOCK, ac.WAVES, ac.FEATURE_TILE) == (32, 32, 4, 64, 4, 32)
    assert ac.GROUP == 128 and ac.MAX_OWN_TILES == ac.MAX_DIM // ac.FEATURE_TILE // ac.WAVES == 8


def test_the_shapes_are_the_listed_ones():
    got = {(c.storage, c.dim, c.B, c.C) for c in ac.EDGE_CASES}
    assert got == {("f32", 32, 1024, 1024), ("f32", 32, 1024, 8192), ("bf16", 64, 257, 300), ("f32", 1024, 33, 130),
                   ("bf16", 1024, 33, 130), ("f32", 768, 40, 257), ("bf16", 64, 33, 40), ("f32", 64, 1, 200),
                   ("f32", 96, 96, 416), ("bf16", 128, 96, 416), ("f32", 384, 65, 100)}
    assert len(ac.EDGE_CASES) == 12 and len(ac.CASE_BY_NAME) == 12
    for c in ac.EDGE_CASES:
        assert c.scales == ((30.0, 100.0) if c.cand == "masked tiles" else (30.0,)), c.name
        assert 1 <= c.B <= ac.MAX_BATCH and c.B <= c.C <= ac.MAX_CANDIDATES and c.dim % 32 == 0 and 32 <= c.dim <= ac.MAX_DIM
        P, rows, anchors, delta, cand = ac.inputs(c.name)
        assert P.shape == rows.shape == (c.n_rows, c.dim) and anchors.shape == (c.B, c.dim) and cand.shape == (c.C,)
        assert delta.shape == (c.dim, c.dim) and ac.inputs(c.name)[4] is cand  # drawn once


def test_each_shape_reaches_the_path_it_names():
    c = ac.CASE_BY_NAME
    for name in ("batch-limit", "both-limits"):
        assert c[name].B == ac.MAX_BATCH and tiles(c[name].B, ac.ANCHOR_TILE) == 32 and tiles(c[name].B, ac.GRAD_BLOCK) == 16
        assert c[name].dim == 32  # the narrowest rows
    assert c["both-limits"].C == ac.MAX_CANDIDATES and c["batch-limit"].C == c["batch-limit"].B
    edge = c["batch-off-its-edges"]
    assert edge.B == 4 * ac.GRAD_BLOCK + 1 and edge.B % ac.ANCHOR_TILE == 1 and tiles(edge.B, ac.ANCHOR_TILE) == 9
    assert edge.C % ac.CAND_TILE and tiles(edge.C, ac.CAND_TILE) % ac.GROUP_TILES  # a ragged tile in a ragged group
    for name in ("widest-f32", "widest-bf16"):
        w = c[name]
        own = [t // ac.WAVES for t in range(w.dim // ac.FEATURE_TILE)]
        assert w.dim == ac.MAX_DIM and max(own) == ac.MAX_OWN_TILES - 1 == 7 and 6 in own
        assert tiles(w.C, ac.CAND_TILE) == ac.GROUP_TILES + 1 and w.B == ac.ANCHOR_TILE + 1
    assert c["wide-f32"].storage == "f32" and c["wide-f32"].dim > 384 and (c["wide-f32"].dim // 32 - 1) // ac.WAVES == 5
    narrow = c["narrow-bf16"]
    assert narrow.storage == "bf16" and narrow.dim < 384 and narrow.dim // ac.FEATURE_TILE < ac.WAVES
    one = c["one-anchor"]
    valid, masked, counted = ref.masks(ac.inputs("one-anchor")[4], 1, one.n_rows)
    assert one.B == 1 and counted.all() and (~masked[0]).sum() == one.C > ac.GROUP
    _, _, _, big, _ = ac.inputs("trained-size-D")
    _, _, _, small, _ = ac.inputs("widest-f32")
    assert 0.45 < big.std() * np.sqrt(384) < 0.55 and 0.045 < small.std() * np.sqrt(1024) < 0.055
    lengths = np.linalg.norm(ac.inputs("anchor-norms")[2].astype(np.float64), axis=1)
    assert lengths.min() == pytest.approx(1e-3, rel=1e-5) and lengths.max() == pytest.approx(1e3, rel=1e-5)
    assert np.linalg.norm(ac.inputs("trained-size-D")[2].astype(np.float64), axis=1) == pytest.approx(1.0, rel=1e-6)


@pytest.mark.parametrize("name", ["masked-tiles-f32", "masked-tiles-bf16"])
def test_the_masked_list_reaches_every_masking_path(name):
    c, cand, (valid, masked, counted) = case_masks(name)
    B, C, n = c.B, c.C, c.n_rows
    n_ct = tiles(C, ac.CAND_TILE)
    assert (B, C) == (96, 416) and n_ct == 13
    # a wholly masked candidate tile: 32 candidates at a multiple of 32, all outside [0, n_rows), not the last tile
    dead_tiles = wholly_masked(valid, ac.CAND_TILE)
    for t in ac.MASKED_TILES:
        at = cand[t * 32:(t + 1) * 32]
        assert t in dead_tiles and t < n_ct - 1 and ((at < 0) | (at >= n)).all() and masked[:, t * 32:(t + 1) * 32].all()
    # a wholly masked group: 128 candidates at a multiple of 128; with it wave 1 meets no candidate at all
    assert wholly_masked(valid, ac.GROUP) == [ac.MASKED_GROUP] and (ac.MASKED_GROUP + 1) * ac.GROUP <= C
    by_wave = {w: [t for t in range(n_ct) if t % ac.WAVES == w] for w in range(ac.WAVES)}
    assert all(t in dead_tiles for t in by_wave[1]) and all(any(t not in dead_tiles for t in by_wave[w]) for w in (0, 2, 3))
    # a tile with nothing in range before and after tiles that have some, within one wave's walk (-inf joins a finite maximum)
    assert by_wave[2][:3] == [2, 6, 10] and 2 not in dead_tiles and 6 not in dead_tiles and 10 in dead_tiles
    # an uncounted anchor tile with counted anchors in the tiles on both sides
    t = ac.UNCOUNTED_ANCHOR_TILE
    assert not counted[32 * t:32 * t + 32].any() and counted[32 * (t - 1):32 * t].any() and counted[32 * (t + 1):32 * (t + 2)].any()
    assert 32 * (t + 2) <= B and 0 < counted.sum() < B - 32  # (single uncounted anchors elsewhere too)

    def copy(j, i):
        assert i < B and counted[i] and j != i and cand[j] == cand[i] and masked[i, j] and valid[j]
        assert not masked[(i + 1) % 32, j]  # .. and not for a neighbour in anchor tile 0, whose positive is another row
        return j // ac.CAND_TILE, i // ac.CAND_TILE

    tj, ti = copy(*ac.COPY_OTHER_WAVE)      # another wave's tile
    assert tj != ti and tj % ac.WAVES != ti % ac.WAVES and tj // ac.GROUP_TILES == ti // ac.GROUP_TILES
    for pair in (ac.COPY_OTHER_GROUP, ac.COPY_LAST_GROUP):  # another group of 128 (and another wave)
        tj, ti = copy(*pair)
        assert tj // ac.GROUP_TILES != ti // ac.GROUP_TILES and tj % ac.WAVES != ti % ac.WAVES
    assert ac.COPY_LAST_GROUP[0] // ac.GROUP == n_ct // ac.GROUP_TILES == 3  # the ragged last group
    j, i = ac.COPY_IS_A_POSITIVE            # a copy that is another anchor's positive, in another anchor tile
    copy(j, i)
    copy(i, j)
    assert j < B and j // ac.ANCHOR_TILE != i // ac.ANCHOR_TILE
    # the bounds of the index: rows 0 and n_rows - 1 count, n_rows and -1 do not
    for row, ok in ((0, True), (n - 1, True), (n, False), (-1, False), (ac.INT32_MAX, False), (ac.INT32_MIN, False)):
        at = np.flatnonzero(cand == row)
        assert at.size and (valid[at] == ok).all() and masked[:, at].all() != ok, row
    assert (cand[:B] == 0).any() and (cand[:B] == n - 1).any() and (cand[B:] == n - 1).any()  # as positives and as a negative
    live = [tt for tt in range(n_ct) if tt not in dead_tiles]
    assert any(not valid[tt * 32:(tt + 1) * 32].all() for tt in live)  # single masked ids inside tiles that are in range


@pytest.mark.parametrize("name,scale", ac.STEPS, ids=[f"{n}-{s:g}" for n, s in ac.STEPS])
def test_references_are_finite_and_the_float32_error_is_positive(name, scale):
    c, cand, (valid, masked, counted) = case_masks(name)
    assert counted.any() and (~masked[counted]).sum(axis=1).min() >= 2  # every counted anchor has a negative
    want_loss, want_grad, ref_loss, ref_grad = ac.references(name, scale)
    assert np.isfinite(want_loss) and np.isfinite(want_grad).all() and np.isfinite(ref_loss) and np.isfinite(ref_grad).all()
    assert want_loss > 0 and np.abs(want_grad).max() > 0
    e_rms, e_abs = row_errors(ref_grad, want_grad)
    assert e_rms > 0 and e_abs > 0
    assert max(abs(ref_loss - want_loss), h.loss_floor(want_loss)) > 0
    assert ac.references(name, scale)[1] is want_grad and not want_grad.flags.writeable  # computed once, left unchanged


def test_the_masked_id_mix_holds_every_rule():
    B, C, n = 65, 300, 300
    cand = ac.masked_id_mix(np.random.default_rng(1), B, C, n)
    valid, masked, counted = ref.masks(cand, B, n)
    assert (cand == -1).any() and (cand == n).any() and (cand == n - 1).any() and 0 < counted.sum() < B
    assert not valid[:B].all() and not valid[B:].all()
    copies = masked & valid[None, :]
    assert copies[:, :B].any() and copies[:, B:].any()  # a repeated positive, and a negative that is a positive's copy


@pytest.mark.parametrize("d", [32, 1024])
def test_the_adamw_bound_is_one_ieee_float32_meets(d):
    """The AdamW bound of the GPU tests, on the kernel's formula in numpy float32: met everywhere; test_adapter_gpu's
    form of it (|term| for the Adam term's magnitude) is the same number wherever m and (g - m)(1 - beta1) do not cancel
    and is missed by correct float32 arithmetic where they do, at d = 1024."""
    P, anchors, cand, delta, m, v = h.adamw_inputs(d)
    g = ref.loss_and_grad(delta, anchors, ref.stored_rows(P), cand, 30.0, torch.float32)[1].astype(np.float32)
    before = {"delta": delta, "m": m, "v": v, "t": 7}
    p, m1, v1 = h.adamw_float32(delta, m, v, 7, g, *h.ADAMW_HYPER)
    after = {"delta": p, "m": m1, "v": v1, "t": 8}
    use_delta, use_m, use_v, use_plain, t = h.adamw_bound_use(before, g, after)
    print(f"AdamW d{d}: bound use D {use_delta.max():.2f} m {use_m.max():.2f} v {use_v.max():.2f}; "
          f"with |term|: {use_plain.max():.2f}, {(use_plain > 1).sum()} of {use_plain.size} elements over")
    h.assert_adamw(before, g, after)
    assert t == 8 and (use_plain >= use_delta * (1 - 1e-9)).all()
    same_sign = m.astype(np.float64) * (g.astype(np.float64) - m) >= 0
    assert same_sign.any() and np.allclose(use_plain[same_sign], use_delta[same_sign], rtol=1e-6)
    if d == 1024:
        assert (use_plain > 1).sum() > 100 and use_plain.max() > 8
    # a wrong bias correction (t instead of t + 1) is far outside it
    wrong = h.adamw_float32(delta, m, v, 6, g, *h.ADAMW_HYPER)
    assert h.adamw_bound_use(before, g, {"delta": wrong[0], "m": wrong[1], "v": wrong[2], "t": 8})[0].max() > 1000
