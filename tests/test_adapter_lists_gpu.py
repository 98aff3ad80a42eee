"""icrec_adapter_step_lists on the GPU against tests/adapter_reference.py's loss_and_grad_lists: the cases of
tests/adapter_lists_cases.py within margin x the float32 reference's own error (measured ratios and the margins' choice:
profiles/adapter_errors.md), the values that are exactly zero, the filter storages on the bits, the shared one-hot list
against icrec_adapter_step, determinism, AdamW, a step after remove_rows, the argument checks that need a device, and the
learning task with graded lists end to end through icrec_search.  What the three kinds of step are tested for alike has
its one body in tests/adapter_harness.py."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.search import DeviceIndex, apply_moves
from tests import adapter_harness as h
from tests import adapter_lists_cases as lc
from tests import adapter_reference as ref
from tests.adapter_harness import DEV, adapter_with, bits
from tests.search_harness import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- loss and gradient
@pytest.mark.parametrize("name,scale", lc.STEPS, ids=[f"{n}-{s:g}" for n, s in lc.STEPS])
def test_loss_and_gradient_of_the_cases(torch_cuda, name, scale):
    h.check_case("lists", lc, name, scale)


def test_values_that_are_exactly_zero(torch_cuda):
    nan, inf = float("nan"), float("inf")

    def one_counted_among_others(ix, ad, anchors):
        # one anchor with a real list beside four that are not counted: the mean is that anchor's loss alone
        real = [(1, 1.0), (2, 0.0), (3, 2.0)]
        alone = ad.loss_and_grad_lists(ix, anchors[2:3], [real])
        among = ad.loss_and_grad_lists(ix, anchors, [[], [(7, 0.0)], real, [(50, 1.0)], [(4, nan)]])
        assert float(alone[0].cpu()) > 0 and torch.equal(alone[0], among[0]) and torch.equal(alone[1], among[1])

    h.check_exact_zeros("lists", 50, 5, (
        ("one-entry lists", 5, [[(7, 1.0)], [(0, 4.0)], [(49, 0.5)], [(7, 1e-30)], [(3, 2.0)]]),
        ("one live entry among dropped ones", 5, [[(-1, 1.0), (7, 3.0), (50, 1.0)], [(2, nan), (3, 1.0)], [(4, 1.0), (5, -1.0)],
                                                  [(6, inf), (8, 2.0)], [(9, 2.0)]]),
        ("nobody counted", 5, [[(7, 0.0), (8, 0.0)], [], [(50, 1.0), (-1, 2.0)], [(3, nan), (4, -1.0), (5, inf)], [(6, 0.0)]])),
        one_counted_among_others)


def test_filter_storages_give_the_same_bits(torch_cuda):
    name = "w384-bf16"
    P, _, anchors, delta, lists = lc.inputs(name)
    got = {}
    for storage in ("f32", "bf16", "f32+filter", "bf16+filter"):
        ix = DeviceIndex(P, DEV, storage=storage)
        ad = adapter_with(delta)
        try:
            loss, grad = h.device_step("lists", ix, ad, anchors, lists)
            assert loss > 0 and np.abs(grad).max() > 0
            got[storage] = bits(loss, grad)
        finally:
            ad.close()
            ix.close()
    assert got["f32+filter"] == got["f32"] and got["bf16+filter"] == got["bf16"]
    assert got["bf16"][0] != got["f32"][0] and got["bf16"][1] != got["f32"][1]


# ---------------------------------------------------------------- the shared one-hot list
def test_shared_one_hot_list_against_the_pair_step(torch_cuda):
    rng = np.random.default_rng(61)
    d, B, C, n_rows = 384, 33, 64, 600
    P = h.unit_rows(rng, n_rows, d)
    anchors, delta = h.unit_rows(rng, B, d), h.small_delta(rng, d)
    cand = rng.choice(n_rows, C, replace=False).astype(np.int64)  # distinct and in range: the pair step masks nothing
    one_hot = np.zeros((B, C), np.float32)
    one_hot[np.arange(B), np.arange(B)] = 1.0
    lists = ref.uniform_csr(np.tile(cand, (B, 1)), one_hot)
    stored = ref.stored_rows(P, "f32")
    want = ref.loss_and_grad(delta, anchors, stored, cand, 30.0, torch.float64)
    ref32 = ref.loss_and_grad(delta, anchors, stored, cand, 30.0, torch.float32)
    want_lists = ref.loss_and_grad_lists(delta, anchors, stored, *lists, 30.0, torch.float64)
    assert abs(want_lists[0] - want[0]) <= 1e-12 and np.abs(want_lists[1] - want[1]).max() <= 1e-12
    ix = DeviceIndex(P, DEV, storage="f32")
    ad = adapter_with(delta)
    try:
        for kind, targets in (("lists", lists), ("pairs", cand)):  # both against the PAIR step's references
            loss, grad = h.device_step(kind, ix, ad, anchors, targets)
            h.check_step(f"adapter {kind} f32 d{d} B{B} C{C} shared one-hot list", loss, grad, *want, *ref32,
                         h.KINDS[kind].margins[("f32", d)])
    finally:
        ad.close()
        ix.close()


# ---------------------------------------------------------------- determinism, AdamW
@pytest.mark.parametrize("name", ["w384-bf16", "list-limit"])
def test_step_is_deterministic(torch_cuda, name):
    c = lc.CASE_BY_NAME[name]
    P, _, anchors, delta, lists = lc.inputs(name)
    rng = np.random.default_rng(59)
    m, v = h.small_delta(rng, c.dim), np.abs(h.small_delta(rng, c.dim))
    h.check_determinism("lists", P, c.storage, anchors, lists, delta, m, v)


def test_adamw_step_matches_the_float64_formula(torch_cuda):
    P, anchors, _, delta, m, v = h.adamw_inputs(96)
    lists = lc.uniform_lists(np.random.default_rng(67), anchors.shape[0], 30, P.shape[0])
    _, g, _ = h.check_adamw("lists", P, anchors, lists, delta, m, v)
    assert (g != 0).mean() > 0.99


# ---------------------------------------------------------------- after an index edit
def test_step_after_remove_rows_on_the_same_handle(torch_cuda):
    rng = np.random.default_rng(71)
    d, B, L, n0 = 384, 33, 40, 300
    M = rng.standard_normal((n0, d)).astype(np.float32)
    anchors, delta = h.unit_rows(rng, B, d), h.small_delta(rng, d)
    ix = DeviceIndex(M, DEV, storage="f32")
    ad = adapter_with(delta)
    try:
        def lists_naming(last):
            off, rows, target, max_len = lc.uniform_lists(rng, B, L, last)  # rows below `last`
            rows = rows.copy()
            rows[0], rows[1], target = last, last - 1, target.copy()       # the last row, with gains, in anchor 0's list ..
            target[0], target[1] = 4.0, 2.0
            rows[L:2 * L], target[L:2 * L] = last, 1.0                     # .. and as anchor 1's whole list
            return off, rows, target, max_len

        def check(what, lists):
            h.check_against_reference("lists", f"adapter lists f32 d{d} B{B} L{L} {what}", ix, ad, anchors, delta,
                                      ref.stored_rows(M, "f32"), lists, "f32")

        lists = lists_naming(n0 - 1)
        _, _, _, live, counted = ref.masks_lists(*lists, n0)
        assert live[0, 0] and counted.all()
        check("fresh", lists)
        gone = [0, 5, n0 - 1, 150]
        dst, src = ix.remove_rows(gone)
        M = apply_moves(M, n0 - len(gone), dst, src)
        assert ix.n_rows == M.shape[0] == n0 - 4
        _, _, _, live, counted = ref.masks_lists(*lists, ix.n_rows)  # the same lists: the removed last row is out of range now
        assert not live[0, 0] and counted[0] and not counted[1] and counted.sum() == B - 1
        check("after remove_rows", lists)
    finally:
        ad.close()
        ix.close()


# ---------------------------------------------------------------- argument checks that need a device
def test_argument_checks(torch_cuda):
    rng = np.random.default_rng(8)
    ix = DeviceIndex(h.unit_rows(rng, 40, 64), DEV, storage="f32")
    anchors = torch.from_numpy(h.unit_rows(rng, 4, 64)).to(DEV)
    lists = [[(1, 1.0), (2, 0.0)]] * 4
    ad = adapter_with(h.small_delta(rng, 64))
    try:
        off, rows, target, max_len = ad._csr(lists, 4)
        for bad in (0, 1025, -1):
            with pytest.raises(_native.IcrecError, match="max_len must be in"):
                ad.loss_and_grad_lists(ix, anchors, (off, rows, target, bad))
        with pytest.raises(ValueError, match="4 anchors for 3 lists"):
            ad.loss_and_grad_lists(ix, anchors, lists[:3])
        with pytest.raises(ValueError, match="4 anchors for 2 lists"):
            ad.loss_and_grad_lists(ix, anchors, (off[:3], rows, target, max_len))
        h.check_shared_arguments("lists", ix, ad, anchors, tuple(t.cpu().numpy() for t in (off, rows, target)) + (max_len,))
        L = _native.lib()
        need = int(L.icrec_adapter_step_lists_workspace_bytes(ad._h, 4))
        assert need > 0 and L.icrec_adapter_step_lists_workspace_bytes(ad._h, 0) == 0
        assert L.icrec_adapter_step_lists_workspace_bytes(ad._h, 1025) == 0
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        loss = torch.empty(1, device=DEV)

        def call(off_p, rows_p, target_p, ws_bytes):
            return L.icrec_adapter_step_lists(ix._h, ad._h, _native.ptr(anchors), 4, off_p, rows_p, target_p, max_len, 30.0, 0.0,
                                              0.9, 0.999, 1e-8, 0.0, 0, _native.ptr(loss), None, _native.ptr(ws), ws_bytes, None)

        o, r, t = _native.ptr(off), _native.ptr(rows), _native.ptr(target)
        for args in ((o, None, t), (o, r, None)):  # the two arrays behind list_off
            assert call(*args, need) == -1 and b"NULL" in L.icrec_last_error()
        assert call(o, r, t, need) == 0 and float(loss.cpu()) > 0
        assert ad.steps == 0  # no refused call took a step
    finally:
        ad.close()
        ix.close()


# ---------------------------------------------------------------- learning, end to end
def test_adapter_learns_from_graded_lists_end_to_end(torch_cuda):
    """Held-out recall@10 through icrec_search after 100 steps on lists of 128 (the positive at gain 4, its two nearest
    rows at gain 1, 125 random rows at gain 0): at most 0.05 before, and after at least the float64 reference loop's
    (run here: 0.870, loss 11.44 -> 2.50) minus 0.03 - 31 of the 1,024 held-out queries."""
    task = ref.learning_task()
    P, a_train, p_train, a_held, p_held = task
    rows, gains = ref.task_lists(P, p_train, np.random.default_rng(5))
    assert rows.shape == gains.shape == (ref.TASK_TRAIN, ref.TASK_LIST)
    D64, ref_losses = ref.train_reference(P, a_train, rows, gains)
    stored = ref.stored_rows(P, "f32")
    ref_before = ref.recall_at(ref.top_rows(a_held, stored, 10), p_held)
    ref_after = ref.recall_at(ref.top_rows(a_held + a_held @ D64.T, stored, 10), p_held)
    print(f"reference recall@10 {ref_before:.4f} -> {ref_after:.4f}, loss {ref_losses[0]:.3f} -> {ref_losses[-1]:.3f}")
    assert ref_after > 0.8 and ref_losses[-1] < 0.5 * ref_losses[0]

    a_dev = torch.from_numpy(a_train).to(DEV)
    rows_dev, gains_dev = torch.from_numpy(rows).to(DEV, torch.int32), torch.from_numpy(gains).to(DEV)
    off = torch.arange(ref.TASK_BATCH + 1, dtype=torch.int32, device=DEV) * ref.TASK_LIST
    ix, ad, after, losses, _ = h.train_on_task(
        "lists", task, lambda at: (off, rows_dev[at].reshape(-1), gains_dev[at].reshape(-1), ref.TASK_LIST))
    try:
        assert after >= ref_after - 0.03 and abs(losses[0] - ref_losses[0]) < 1e-3 * ref_losses[0]
        # lists_loss: the held-out number, over two batches (1,024 + 476), is the weighted mean of the two
        n = 1500
        whole = ad.lists_loss(ix, a_dev[:n], (torch.arange(n + 1, dtype=torch.int32, device=DEV) * ref.TASK_LIST,
                                              rows_dev[:n].reshape(-1), gains_dev[:n].reshape(-1), ref.TASK_LIST))
        want = ref.per_anchor_losses(ad.state()["delta"], a_train[:n], stored, *ref.uniform_csr(rows[:n], gains[:n]), ref.TASK_SCALE)[0]
        assert abs(whole - float(want.mean())) <= 1e-5 * float(want.mean())
        # fit_lists: reproducible from its seed, drop_last, the schedule's first step has lr 0
        lists = [list(zip(r.tolist(), g.tolist())) for r, g in zip(rows[:300], gains[:300])]
        h.check_fit_is_reproducible(lambda fitted: fitted.fit_lists(ix, a_dev[:300], lists, epochs=2, batch_size=128, lr=5e-3,
                                                                    seed=4), 2 * (300 // 128))
    finally:
        ad.close()
        ix.close()
