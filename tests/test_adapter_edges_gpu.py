"""icrec_adapter_step at the limits include/icrec.h states and on the paths of csrc/adapt.hip the first test file stops
short of: the cases of tests/adapter_cases.py (tests/test_adapter_cases.py shows without a GPU which path each reaches)
under tests/adapter_harness.py's rule and margins, the filter storages and a row offset on the bits, steps after index edits on
the same handle, AdamW's tile mapping at the narrowest and the widest D and its first steps from zero moments, and
determinism at B = 1024, C = 8192."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd.search import DeviceIndex, apply_moves, removal_moves
from tests import adapter_cases as ac
from tests import adapter_harness as h
from tests import adapter_reference as ref
from tests.adapter_harness import DEV, adapter_with, bits
from tests.search_harness import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- loss and gradient at the limits and on the masked paths
@pytest.mark.parametrize("name,scale", ac.STEPS, ids=[f"{n}-{s:g}" for n, s in ac.STEPS])
def test_loss_and_gradient_of_the_edge_cases(torch_cuda, name, scale):
    h.check_case("pairs", ac, name, scale)


# ---------------------------------------------------------------- storages and the row offset
def test_filter_storages_and_a_row_offset_give_the_same_bits(torch_cuda):
    rng = np.random.default_rng(41)
    d, B, C, n_rows = 384, 65, 300, 300
    P = h.unit_rows(rng, n_rows, d)
    anchors, delta = h.unit_rows(rng, B, d), h.small_delta(rng, d)
    cand = ac.masked_id_mix(rng, B, C, n_rows)
    valid, masked, counted = ref.masks(cand, B, n_rows)
    assert 0 < counted.sum() < B and not valid[B:].all() and (masked & valid[None, :]).any()
    got = {}
    for storage, row_offset in (("f32", 0), ("bf16", 0), ("f32+filter", 0), ("bf16+filter", 0), ("f32", 12345), ("bf16", 12345)):
        ix = DeviceIndex(P, DEV, row_offset=row_offset, storage=storage)
        ad = adapter_with(delta)
        try:
            loss, grad = h.device_step("pairs", ix, ad, anchors, cand)
            assert loss > 0 and np.abs(grad).max() > 0
            got[storage, row_offset] = bits(loss, grad)
        finally:
            ad.close()
            ix.close()
    assert got["f32+filter", 0] == got["f32", 0]
    assert got["bf16+filter", 0] == got["bf16", 0]
    assert got["bf16", 0][0] != got["f32", 0][0] and got["bf16", 0][1] != got["f32", 0][1]
    assert got["f32", 12345] == got["f32", 0] and got["bf16", 12345] == got["bf16", 0]  # candidates are local rows


# ---------------------------------------------------------------- after index edits
@pytest.mark.parametrize("storage", ["f32", "bf16+filter"])
def test_after_index_edits_on_the_same_handle(torch_cuda, storage):
    rng = np.random.default_rng(43)
    d, B, C, n0 = 384, 65, 300, 300
    M = rng.standard_normal((n0, d)).astype(np.float32)
    anchors, delta = h.unit_rows(rng, B, d), h.small_delta(rng, d)
    ix = DeviceIndex(M, DEV, storage=storage)
    ad = adapter_with(delta)
    try:
        def check(what, dropped=None):
            n = ix.n_rows
            assert n == M.shape[0]
            cand = ac.masked_id_mix(rng, B, C, n)  # names n - 1 and n behind the positives
            cand[9], cand[10] = n - 1, n           # .. and as positives: the last row counts, the one behind it does not
            if dropped is not None:
                cand[11] = dropped                 # the last row before the removal
            valid, _, counted = ref.masks(cand, B, n)
            assert counted[9] and not counted[10] and valid[B] and not valid[B + 2]
            assert dropped is None or (dropped >= n and not counted[11])
            h.check_against_reference("pairs", f"adapter {storage} d{d} B{B} C{C} {what}", ix, ad, anchors, delta,
                                      ref.stored_rows(M, storage), cand, storage)
            return cand, counted

        check("fresh")
        ids = [n0 - 1, 3, 150]
        new = (rng.standard_normal((3, d)) * 4).astype(np.float32)
        ix.write_rows(ids, new)
        M[ids] = new
        check("after write_rows")
        extra = rng.standard_normal((400, d)).astype(np.float32)
        ix.append_rows(extra)  # past the capacity: every pointer of the handle changes
        assert ix.capacity > n0
        M = np.concatenate([M, extra])
        cand, counted = check("after append_rows")
        assert (cand == n0 + 399).any() and cand.max() == n0 + 400
        old_last = M.shape[0] - 1
        assert cand[9] == old_last and counted[9]  # counted as a positive now ..
        gone = [0, 5, old_last, 350]
        dst, src = ix.remove_rows(gone)
        new_n, want_dst, want_src = removal_moves(M.shape[0], gone)
        assert dst.tolist() == want_dst.tolist() and src.tolist() == want_src.tolist()
        M = apply_moves(M, new_n, dst, src)
        check("after remove_rows", dropped=old_last)  # .. and out of range after the removal
    finally:
        ad.close()
        ix.close()


# ---------------------------------------------------------------- AdamW
HYPER, assert_adamw = h.ADAMW_HYPER, h.assert_adamw


@pytest.mark.parametrize("d", [32, 1024])
def test_adamw_tile_mapping_at_one_tile_and_at_1024_tiles(torch_cuda, d):
    P, anchors, cand, delta, m, v = h.adamw_inputs(d)
    ix = DeviceIndex(P, DEV, storage="f32")
    anchors, cand = torch.from_numpy(anchors).to(DEV), torch.from_numpy(cand)
    ad = adapter_with(delta, m, v, 7)
    try:
        before = ad.state()
        grad = torch.empty((d, d), dtype=torch.float32, device=DEV)
        ad.step(ix, anchors, cand, HYPER[0], HYPER[1:3], HYPER[3], HYPER[4], grad_out=grad)
        g = grad.cpu().numpy()
        assert np.abs(g).max() > 0 and (g != 0).mean() > 0.99  # every tile of dD has values
        after = ad.state()
        assert after["t"] == 8 and ad.steps == 8
        assert_adamw(before, g, after)
        assert (after["delta"] != before["delta"]).mean() > 0.99  # every tile was updated
        few = anchors[:5]  # the transposed copy followed: apply reads it (a handful of queries - the reference loops over c)
        assert np.array_equal(ad.apply(few).cpu().numpy(), ref.apply(after["delta"], few.cpu().numpy()))
    finally:
        ad.close()
        ix.close()


@pytest.mark.parametrize("start", ["zero D", "small D"])
def test_adamw_first_steps_from_zero_moments(torch_cuda, start):
    rng = np.random.default_rng(53)
    d, B, C, dead = 96, 40, 64, 17
    decay = np.float32(1.0 - HYPER[0] * HYPER[4])
    ix = DeviceIndex(h.unit_rows(rng, 500, d), DEV, storage="f32")
    delta = np.zeros((d, d), np.float32) if start == "zero D" else h.small_delta(rng, d)
    ad = adapter_with(delta)  # m = v = 0, t = 0: where training starts
    try:
        for t in (1, 2, 3):
            a = h.unit_rows(rng, B, d)
            a[:, dead] = 0.0  # dD[r][dead] = sum_i dz_i[r] * 0: exactly zero in every step
            cand = torch.from_numpy(rng.choice(500, C, replace=False))
            before = ad.state()
            assert before["t"] == t - 1 and (t > 1 or not (before["m"].any() or before["v"].any()))
            grad = torch.empty((d, d), dtype=torch.float32, device=DEV)
            ad.step(ix, torch.from_numpy(a).to(DEV), cand, HYPER[0], HYPER[1:3], HYPER[3], HYPER[4], grad_out=grad)
            g = grad.cpu().numpy()
            after = ad.state()
            assert after["t"] == t and ad.steps == t
            assert_adamw(before, g, after)
            live = np.arange(d) != dead
            assert not g[:, dead].any() and (g[:, live] != 0).mean() > 0.99
            # no gradient: the moments stay zero and D only decays, one float32 multiplication by the float32 factor
            assert not after["m"][:, dead].any() and not after["v"][:, dead].any()
            assert np.array_equal(after["delta"][:, dead], before["delta"][:, dead] * decay)
            assert (after["delta"][:, live] != before["delta"][:, live]).mean() > 0.99
            assert np.array_equal(ad.apply(torch.from_numpy(a[:5]).to(DEV)).cpu().numpy(), ref.apply(after["delta"], a[:5]))
    finally:
        ad.close()
        ix.close()


# ---------------------------------------------------------------- determinism
def test_step_is_deterministic_at_the_limits(torch_cuda):
    name = "both-limits"
    c = ac.CASE_BY_NAME[name]
    assert (c.B, c.C) == (ac.MAX_BATCH, ac.MAX_CANDIDATES)
    P, _, anchors, delta, cand = ac.inputs(name)
    rng = np.random.default_rng(59)
    m, v = h.small_delta(rng, c.dim), np.abs(h.small_delta(rng, c.dim))
    h.check_determinism("pairs", P, c.storage, anchors, cand, delta, m, v)
