"""icrec_adapter_step_catalog on the GPU against tests/adapter_reference.py's loss_and_grad_catalog: the loss and its
gradient within margin x the float32 reference's own error (tests/adapter_harness.check_step's convention; measured ratios
and the margins' choice: profiles/adapter_catalog_errors.md) on the cases of tests/adapter_catalog_cases.py, the labels'
rules, the index after every kind of edit, determinism, AdamW, the argument checks, and the learning task end to end.
What the three kinds of step are tested for alike has its one body in tests/adapter_harness.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.search import DeviceIndex
from tests import adapter_catalog_cases as cases
from tests import adapter_harness as h
from tests import adapter_reference as ref
from tests.adapter_harness import DEV, adapter_with, loss_floor, small_delta, unit_rows
from tests.search_harness import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

MARGINS = h.KINDS["catalog"].margins


def device_plan(ad, B, n_rows):
    n_splits, per_split = C.c_int32(0), C.c_int64(0)
    _native.check(_native.lib().icrec_adapter_catalog_plan(ad._h, B, n_rows, C.byref(n_splits), C.byref(per_split)), "plan")
    return n_splits.value, per_split.value


# ---------------------------------------------------------------- loss and gradient
@pytest.mark.parametrize("name,scale", cases.STEPS, ids=lambda v: str(v))
def test_loss_and_gradient_within_margin_of_the_float32_reference(torch_cuda, name, scale):
    def split_rule(ad, c):  # the library cuts the catalog as tests/adapter_catalog_cases.plan restates it
        assert device_plan(ad, c.B, c.n_rows) == cases.plan(c.B, c.n_rows)

    h.check_case("catalog", cases, name, scale, split_rule)


def test_nobody_counted_is_exactly_zero(torch_cuda):
    h.check_exact_zeros("catalog", 300, 40, [(pos, len(pos), torch.tensor(pos)) for pos in
                                             ([300], [-1, 300, 2**31 - 1, -2**31, 2**40], [-1] * 40)])


# ---------------------------------------------------------------- index states
@pytest.mark.parametrize("storage", ["f32+filter", "bf16+filter"])
def test_the_rows_the_index_holds_after_every_kind_of_edit(torch_cuda, storage):
    """One handle: as built, after write_rows, after reserve far beyond n_rows, after append_rows past the capacity, after
    remove_rows - each time the step is the reference's over exactly the rows [0, n_rows) the index then holds."""
    rng = np.random.default_rng(31)
    d, B, scale = 64, 40, 30.0
    P = unit_rows(rng, 300, d) * np.float32(1.7)  # any norm: the index normalises
    ix = DeviceIndex(P, DEV, storage=storage)
    delta = small_delta(rng, d)
    ad = adapter_with(delta)
    anchors = unit_rows(rng, B, d)

    def agree(what, pos):
        assert ix.n_rows == P.shape[0]
        h.check_against_reference("catalog", f"catalog {storage} {what}", ix, ad, anchors, delta, ref.stored_rows(P, storage),
                                  pos, storage, scale)

    pos = rng.integers(0, 300, B).astype(np.int64)
    pos[:3] = (0, 299, 299)
    agree("as built", pos)
    ids = np.asarray([0, 5, 131, 299])
    new = (unit_rows(rng, 4, d) * np.float32(0.3)).astype(np.float32)
    ix.write_rows(ids, new)
    P = P.copy()
    P[ids] = new
    agree("after write_rows", pos)
    ix.reserve(5000)
    assert ix.capacity == 5000
    pos_far = pos.copy()
    pos_far[3], pos_far[4] = 300, 4999  # inside the capacity, behind n_rows: not counted, and no such row is a candidate
    agree("after reserve", pos_far)
    more = unit_rows(rng, 4900, d)
    assert ix.append_rows(more) == range(300, 5200) and ix.capacity >= 5200
    P = np.concatenate([P, more])
    pos_new = pos.copy()
    pos_new[3], pos_new[4] = 300, 5199
    agree("after append_rows", pos_new)
    gone = np.asarray([5199, 7, 4000])
    dst, src = ix.remove_rows(gone)
    P = P.copy()
    P[dst] = P[src]
    P = P[:5197]
    pos_new[5] = 5197  # the first row behind the new end: it still lies in the arrays
    agree("after remove_rows", pos_new)  # pos_new[4] names the removed last row: not counted
    ix.close()


# ---------------------------------------------------------------- bits
def test_the_same_inputs_give_the_same_bits(torch_cuda):
    for name in ("f32-384", "batch-limit"):
        c = cases.CASE_BY_NAME[name]
        P, _, anchors, delta, pos = cases.inputs(name)
        m, v = small_delta(np.random.default_rng(1), c.dim), np.abs(small_delta(np.random.default_rng(2), c.dim))
        h.check_determinism("catalog", P, c.storage, anchors, pos, delta, m, v)


# ---------------------------------------------------------------- update
@pytest.mark.parametrize("d", [32, 1024])
def test_adamw_step_on_the_steps_own_gradient(torch_cuda, d):
    rng = np.random.default_rng(70 + d)
    P, anchors = unit_rows(rng, 500, d), unit_rows(rng, 40, d)
    pos = rng.integers(0, 500, 40)
    m = (rng.standard_normal((d, d)) * 1e-3).astype(np.float32)
    v = (rng.random((d, d)) * 1e-5).astype(np.float32)
    h.check_adamw("catalog", P, anchors, pos, small_delta(rng, d), m, v)


# ---------------------------------------------------------------- arguments
def test_argument_checks_and_catalog_loss(torch_cuda):
    rng = np.random.default_rng(8)
    P = unit_rows(rng, 700, 64)
    ix = DeviceIndex(P, DEV, storage="f32")
    delta = small_delta(rng, 64)
    ad = adapter_with(delta)
    anchors = torch.from_numpy(unit_rows(rng, 4, 64)).to(DEV)
    pos = torch.tensor([1, 2, 3, 4])
    h.check_shared_arguments("catalog", ix, ad, anchors, pos.numpy())
    with pytest.raises(_native.IcrecError, match="B must be in"):
        ad.loss_and_grad_catalog(ix, anchors.repeat(257, 1), torch.zeros(1028, dtype=torch.int64))
    with pytest.raises(ValueError, match="4 anchors for 3 positives"):
        ad.loss_and_grad_catalog(ix, anchors, pos[:3])
    L = _native.lib()
    assert L.icrec_adapter_step_catalog_workspace_bytes(ad._h, ix._h, 0) == 0
    assert L.icrec_adapter_step_catalog_workspace_bytes(ad._h, ix._h, 1025) == 0
    assert L.icrec_adapter_step_catalog_workspace_bytes(None, ix._h, 4) == 0
    assert L.icrec_adapter_step_catalog_workspace_bytes(ad._h, None, 4) == 0
    n_splits, per_split = C.c_int32(0), C.c_int64(0)
    for B, n_rows in ((0, 10), (1025, 10), (4, 0)):
        assert L.icrec_adapter_catalog_plan(ad._h, B, n_rows, C.byref(n_splits), C.byref(per_split)) == -1
    assert L.icrec_adapter_catalog_plan(None, 4, 10, C.byref(n_splits), C.byref(per_split)) == -1
    assert L.icrec_adapter_catalog_plan(ad._h, 4, 10, None, C.byref(per_split)) == -1
    assert ad.steps == 0  # no refused call took a step
    # catalog_loss: 2,500 held-out pairs in three batches, some of them not counted, against the float64 reference
    held = unit_rows(rng, 2500, 64)
    labels = rng.integers(0, 700, 2500).astype(np.int64)
    labels[::97] = -1
    labels[1024:1030] = 700
    want = ref.mean_loss_catalog(delta, held, ref.stored_rows(P, "f32"), labels, 20.0)
    ref32 = ref.loss_and_grad_catalog(delta, held, ref.stored_rows(P, "f32"), labels, 20.0, torch.float32)[0]
    ad.scale = 20.0
    got = ad.catalog_loss(ix, torch.from_numpy(held).to(DEV), labels)
    e_ref = max(abs(ref32 - want), loss_floor(want))
    print(f"RATIO catalog_loss: E_gpu {abs(got - want):.3e}, E_ref {e_ref:.3e}, ratio {abs(got - want) / e_ref:.2f}")
    assert isinstance(got, float) and abs(got - want) <= MARGINS[("f32", 64)] * e_ref
    assert ad.catalog_loss(ix, torch.from_numpy(held).to(DEV), labels, scale=30.0) != got
    assert ad.catalog_loss(ix, torch.from_numpy(held[:3]).to(DEV), [-1, 700, 2**40]) == 0.0
    ix.close()


# ---------------------------------------------------------------- learning, end to end
def test_catalog_steps_learn_the_rotation_end_to_end(torch_cuda):
    """The thresholds tests/test_adapter_gpu.py holds the list step to: held-out recall@10 through icrec_search at most
    0.05 before and at least 0.9 after 100 steps, the loss at least halved."""
    task = ref.learning_task()
    p_train, a_held, p_held = task[2], task[3], task[4]
    p_dev, held = torch.from_numpy(p_train).to(DEV, torch.int32), torch.from_numpy(a_held).to(DEV)
    ix, ad, after, losses, (held_before, held_after) = h.train_on_task(
        "catalog", task, lambda at: p_dev[at], lambda ix, ad: ad.catalog_loss(ix, held, p_held))
    print(f"held-out {held_before:.3f} -> {held_after:.3f}")
    assert after >= 0.9 and losses[-1] < 0.5 * losses[0] and held_after < 0.5 * held_before
    # fit(negatives="all"): reproducible from its seed, drop_last, every step a catalog step
    a_dev = torch.from_numpy(task[1]).to(DEV)
    h.check_fit_is_reproducible(lambda fitted: fitted.fit(ix, a_dev[:1000], p_train[:1000], epochs=2, batch_size=128,
                                                          negatives="all", lr=5e-3, seed=4), 2 * (1000 // 128))
    ad.close()
    ix.close()


def test_recommender_fit_adapter_with_all_negatives(torch_cuda, tmp_path):
    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender
    from tests.recommender_harness import synthetic_world

    world = synthetic_world(tmp_path)
    rec = MonitoredRecommender(world.model_dir, world.corpus_path, use_index=False)
    rng = np.random.default_rng(3)
    contexts = syn.synthetic_user_contexts(48, seed=5)
    pairs = [(c, rec.product_ids[int(r)]) for c, r in zip(contexts, rng.integers(0, 700, 48))]
    first = rec.fit_adapter(pairs, epochs=2, batch_size=16, negatives="all", lr=1e-2)
    ad = rec._adapter
    assert ad is not None and len(first) == 6 and ad.steps == 6 and np.isfinite(first).all()
    more = rec.fit_adapter(pairs, epochs=3, batch_size=16, negatives="all", lr=1e-2)
    assert rec._adapter is ad and ad.steps == 15 and np.mean(more) < np.mean(first[:3])
    with pytest.raises(ValueError, match="negatives"):
        rec.fit_adapter(pairs, negatives="some")
