"""icrec_adapter_* on the GPU against tests/adapter_reference.py: apply bit for bit, the loss and its gradient within
margin x the float32 reference's own error (tests/token_states.check's convention; measured ratios and the margins'
choice: profiles/adapter_errors.md), determinism, AdamW against the float64 formula, the argument checks that need a
device, and the learning task end to end through icrec_search.  What the three kinds of step are tested for alike has
its one body in tests/adapter_harness.py."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.adapter import QueryAdapter
from instacart_next_order_recommendation_amd.search import DeviceIndex
from tests import adapter_harness as h
from tests import adapter_reference as ref
from tests.adapter_cases import candidates
from tests.adapter_harness import DEV, adapter_with, small_delta, unit_rows
from tests.search_harness import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- apply
@pytest.mark.parametrize("d", [32, 96, 384, 768, 1024])
def test_apply_is_bit_exact_and_batch_independent(torch_cuda, d):
    rng = np.random.default_rng(d)
    q = rng.standard_normal((300, d)).astype(np.float32)
    delta = small_delta(rng, d) * 4
    want = ref.apply(delta, q)
    ad = adapter_with(delta)
    q_dev = torch.from_numpy(q).to(DEV)
    for n in (1, 2, 63, 65, 300):
        got = ad.apply(q_dev[:n]).cpu().numpy()
        assert np.array_equal(got, want[:n]), n
    for i in (0, 1, 62, 64, 299):  # a row applied alone has the bits it has inside the batch
        assert np.array_equal(ad.apply(q_dev[i:i + 1]).cpu().numpy()[0], want[i]), i
    zero = QueryAdapter(d, DEV)
    assert zero.steps == 0 and not zero.state()["delta"].any()
    assert np.array_equal(zero.apply(q_dev).cpu().numpy(), q)
    out = torch.empty_like(q_dev[:5])
    ad.apply_into(q_dev[:5], out)
    assert np.array_equal(out.cpu().numpy(), want[:5])
    with pytest.raises(_native.IcrecError, match="out must not be q"):
        ad.apply_into(q_dev, q_dev)
    with pytest.raises(ValueError):
        ad.apply(q_dev[:, :d - 1])


# ---------------------------------------------------------------- loss and gradient
CASES = [  # (dim, B, C, storage, scale, kind)
    (32, 2, 2, "f32", 30.0, "plain"),
    (96, 33, 33, "f32", 30.0, "plain"),
    (384, 64, 64, "f32", 30.0, "plain"),
    (384, 65, 100, "f32", 30.0, "plain"),
    (64, 256, 1024, "f32", 30.0, "plain"),
    (768, 40, 257, "bf16", 30.0, "plain"),
    (384, 31, 8192, "bf16", 30.0, "plain"),
    (384, 65, 100, "f32", 20.0, "plain"),
    (384, 65, 100, "f32", 100.0, "plain"),  # overflows exp unless the row maximum is subtracted
    (768, 40, 257, "bf16", 100.0, "plain"),
    (96, 33, 40, "f32", 30.0, "repeated positives"),
    (96, 33, 40, "f32", 30.0, "negative equals a positive"),
    (96, 33, 40, "f32", 30.0, "ids out of range"),
    (96, 33, 40, "f32", 30.0, "positive out of range"),
    (384, 31, 8192, "bf16", 30.0, "ids out of range"),
]


@pytest.mark.parametrize("dim,B,C,storage,scale,kind", CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_loss_and_gradient_within_margin_of_the_float32_reference(torch_cuda, dim, B, C, storage, scale, kind):
    rng = np.random.default_rng(dim * 7 + B)
    n_rows = 10000 if C > 3000 else 3000
    P = unit_rows(rng, n_rows, dim)
    rows = ref.stored_rows(P, storage)
    anchors, delta = unit_rows(rng, B, dim), small_delta(rng, dim)
    cand = candidates(kind, rng, B, C, n_rows)
    ix = DeviceIndex(P, DEV, storage=storage)
    ad = adapter_with(delta)
    what = f"adapter {storage} d{dim} B{B} C{C} scale {scale:g} {kind}"
    h.check_against_reference("pairs", what, ix, ad, anchors, delta, rows, cand, storage, scale)
    assert ad.steps == 0 and np.array_equal(ad.state()["delta"], delta)  # loss_and_grad changes nothing
    ix.close()


def test_gradients_that_are_exactly_zero(torch_cuda):
    h.check_exact_zeros("pairs", 50, 5, [(cand, B, torch.tensor(cand)) for B, cand in  # .., nobody counted (twice)
                                         ((1, [7]), (5, [9, 9, 9, 9, 9]), (3, [-1, 50, 99]), (2, [50, 3]))])


def test_step_is_deterministic(torch_cuda):
    rng = np.random.default_rng(6)
    d, B, C = 384, 65, 300
    P, anchors = unit_rows(rng, 1000, d), unit_rows(rng, B, d)
    cand = rng.integers(-1, 1001, C)
    delta, m, v = small_delta(rng, d), small_delta(rng, d), np.abs(small_delta(rng, d))
    h.check_determinism("pairs", P, "f32", anchors, cand, delta, m, v)


def test_adamw_step_matches_the_float64_formula(torch_cuda):
    rng = np.random.default_rng(7)
    d, B, C = 96, 40, 64
    P, anchors = unit_rows(rng, 500, d), unit_rows(rng, B, d)
    cand = rng.choice(500, C, replace=False)
    delta = small_delta(rng, d)
    m = (rng.standard_normal((d, d)) * 1e-3).astype(np.float32)
    v = (rng.random((d, d)) * 1e-5).astype(np.float32)
    use = h.adamw_bound_use(*h.check_adamw("pairs", P, anchors, cand, delta, m, v))
    assert use[3].max() <= 1  # the inline form of D's bound, which this test held before assert_adamw's


def test_argument_checks_and_state_round_trip(torch_cuda, tmp_path):
    rng = np.random.default_rng(8)
    ix = DeviceIndex(unit_rows(rng, 40, 64), DEV, storage="f32")
    anchors = torch.from_numpy(unit_rows(rng, 4, 64)).to(DEV)
    cand = torch.tensor([1, 2, 3, 4])
    ad = adapter_with(small_delta(rng, 64))
    h.check_shared_arguments("pairs", ix, ad, anchors, cand.numpy())
    with pytest.raises(_native.IcrecError, match=r"C must be in \[B"):
        ad.loss_and_grad(ix, anchors, cand[:3])
    with pytest.raises(_native.IcrecError, match="C must be in"):
        ad.loss_and_grad(ix, anchors, torch.zeros(8193, dtype=torch.int64))
    with pytest.raises(_native.IcrecError, match="B must be in"):
        ad.loss_and_grad(ix, anchors.repeat(257, 1), torch.zeros(1028, dtype=torch.int64))
    L = _native.lib()
    assert L.icrec_adapter_step_workspace_bytes(ad._h, 4, 4) > 0 and L.icrec_adapter_step_workspace_bytes(ad._h, 4, 3) == 0
    assert ad.steps == 0  # no refused call took a step
    # state -> file -> a new adapter: the same delta, scale and steps, and the same apply
    ad.step(ix, anchors, cand, 1e-3)
    ad.scale = 20.0
    ad.save(tmp_path / "a.npz")
    back = QueryAdapter.load(tmp_path / "a.npz", DEV)
    assert back.dim == 64 and back.scale == 20.0 and back.steps == 1
    assert np.array_equal(back.state()["delta"], ad.state()["delta"]) and not back.state()["m"].any()
    assert torch.equal(back.apply(anchors), ad.apply(anchors))
    ix.close()


# ---------------------------------------------------------------- learning, end to end
def test_adapter_learns_the_rotation_end_to_end(torch_cuda):
    """Held-out recall@10 through icrec_search: at most 0.05 before, at least 0.9 after 100 steps (the float64
    reference reaches 1.0: tests/test_adapter.py)."""
    task = ref.learning_task()
    p_train = task[2]
    p_dev = torch.from_numpy(p_train).to(DEV, torch.int32)
    ix, ad, after, losses, _ = h.train_on_task("pairs", task, lambda at: p_dev[at])
    assert after >= 0.9 and losses[-1] < 0.5 * losses[0]
    # fit: reproducible from its seed, drop_last, the schedule's first step has lr 0 and leaves delta at zero
    a_dev = torch.from_numpy(task[1]).to(DEV)
    h.check_fit_is_reproducible(lambda fitted: fitted.fit(ix, a_dev[:1000], p_train[:1000], epochs=2, batch_size=128,
                                                          negatives=64, lr=5e-3, seed=4), 2 * (1000 // 128))
    ad.close()
    ix.close()
