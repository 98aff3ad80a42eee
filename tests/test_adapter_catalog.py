"""The whole-catalog adapter step without a GPU: its reference against the list step's reference, the split rule and
the paths the GPU cases reach, fit_plan and the command line with negatives "all", and the learning task by the
reference alone."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import adapter, cli
from tests import adapter_catalog_cases as cases
from tests import adapter_reference as ref
from tests.adapter_harness import small_delta, unit_rows


def world(B=6, n_rows=40, d=16, seed=0):
    rng = np.random.default_rng(seed)
    return ref.stored_rows(unit_rows(rng, n_rows, d)), unit_rows(rng, B, d).astype(np.float64), small_delta(rng, d).astype(np.float64)


def as_list(pos, n_rows):
    """[the positives ..., every other row ...]: the catalog as the list step's candidate list."""
    return np.concatenate([pos, np.setdiff1d(np.arange(n_rows), pos)])


def test_reference_is_the_list_reference_over_the_whole_catalog_when_positives_are_distinct():
    rows, anchors, delta = world()
    pos = np.array([3, 39, 0, 12, 7, 20])
    loss, grad = ref.loss_and_grad_catalog(delta, anchors, rows, pos, 30.0)
    want_loss, want_grad = ref.loss_and_grad(delta, anchors, rows, as_list(pos, 40), 30.0)
    assert loss == pytest.approx(want_loss, rel=1e-13)
    np.testing.assert_allclose(grad, want_grad, rtol=1e-10, atol=1e-15)
    # an anchor that is not counted has neither a loss nor a gradient: the others' mean is over the counted ones
    out = pos.copy()
    out[1], out[4] = 40, -1
    kept = [0, 2, 3, 5]
    loss, grad = ref.loss_and_grad_catalog(delta, anchors, rows, out, 30.0)
    want_loss, want_grad = ref.loss_and_grad_catalog(delta, anchors[kept], rows, pos[kept], 30.0)
    assert loss == pytest.approx(want_loss, rel=1e-13)
    np.testing.assert_allclose(grad, want_grad, rtol=1e-10, atol=1e-15)
    loss, grad = ref.loss_and_grad_catalog(delta, anchors, rows, np.array([-1, 40, 99, 2**31 - 1, -2**31, 41]), 30.0)
    assert loss == 0.0 and not grad.any()


def test_a_shared_positive_is_not_masked_unlike_the_list_rule():
    rows, anchors, delta = world()
    pos = np.array([3, 3, 0, 12, 7, 20])  # anchors 0 and 1 share row 3
    loss, grad = ref.loss_and_grad_catalog(delta, anchors, rows, pos, 30.0)
    # the list rule masks anchor 1's copy of row 3 for anchor 0 and the reverse; with the copy dropped from the list
    # instead, the list IS the catalog once more, and only then do the two agree
    cand = np.concatenate([pos, np.setdiff1d(np.arange(40), pos)])
    masked_loss, masked_grad = ref.loss_and_grad(delta, anchors, rows, cand, 30.0)
    assert abs(masked_loss - loss) > 1e-6 * loss and np.abs(masked_grad - grad).max() > 1e-6 * np.abs(grad).max()
    # written out: plain cross-entropy, every row once for every anchor
    z = anchors + anchors @ delta.T
    u = z / np.linalg.norm(z, axis=1, keepdims=True)
    s = 30.0 * u @ rows.astype(np.float64).T
    per = np.log(np.exp(s - s.max(1, keepdims=True)).sum(1)) + s.max(1) - s[np.arange(6), pos]
    assert loss == pytest.approx(per.mean(), rel=1e-13)


def test_gradient_is_the_derivative_of_the_loss():
    rows, anchors, delta = world(B=4, n_rows=9, d=4, seed=2)
    pos = np.array([3, 3, 8, 9])
    _, grad = ref.loss_and_grad_catalog(delta, anchors, rows, pos, 30.0)
    h = 1e-6
    for r in range(4):
        for c in range(4):
            up, down = delta.copy(), delta.copy()
            up[r, c] += h
            down[r, c] -= h
            fd = (ref.loss_and_grad_catalog(up, anchors, rows, pos, 30.0)[0] - ref.loss_and_grad_catalog(down, anchors, rows, pos, 30.0)[0]) / (2 * h)
            assert abs(fd - grad[r, c]) <= 1e-6 * max(1.0, abs(grad[r, c])), (r, c)


# ---------------------------------------------------------------- the plan
def test_split_rule():
    G = cases.GROUP
    assert cases.plan(1, 1) == (1, G) and cases.plan(1024, 1) == (1, G)
    # B = 32 and B = 1,024 over the catalog: 389 and 512 workgroups for the 256 CUs
    assert cases.plan(32, cases.CATALOG_ROWS) == (389, G) and cases.plan(1024, cases.CATALOG_ROWS) == (16, 25 * G)
    for B in (1, 31, 32, 33, 256, 1000, 1024):
        for n_rows in (1, 127, 128, 129, 5000, cases.CATALOG_ROWS, 10**7):
            n_splits, per_split = cases.plan(B, n_rows)
            assert 1 <= n_splits <= cases.MAX_SPLITS and per_split % G == 0
            assert (n_splits - 1) * per_split < n_rows <= n_splits * per_split  # no empty split, every row in one


def test_each_gpu_case_reaches_the_path_it_names():
    by = cases.CASE_BY_NAME

    def cut(name):
        c = by[name]
        return cases.plan(c.B, c.n_rows) + (cases.last_split_rows(c.B, c.n_rows),)

    G = cases.GROUP
    assert cut("one-tile") == (1, G, 5)                       # one split
    assert cut("two-splits") == (2, G, 72)                    # two splits
    assert cut("most-splits") == (cases.MAX_SPLITS, G, G - 3)  # the maximum number of splits
    assert cut("whole-splits") == (3, G, G)                   # exactly whole
    assert cut("one-row-over") == (4, G, 1)                   # a last split of 1 row
    assert cut("one-row-short") == (3, G, G - 1)              # a last split one row short of full
    assert cut("batch-limit") == (12, 2 * G, 184)             # splits of more than one group
    assert cut("catalog-f32") == cut("catalog-bf16") == (130, 3 * G, 152)
    assert cut("f32-384")[0] == 24 and cut("widest-f32") == (6, G, 60) and cut("one-anchor") == (17, G, 52)
    for name in ("labels-f32", "labels-bf16"):
        c = by[name]
        pos = cases.inputs(name)[4]
        counted = ref.counted_labels(pos, c.n_rows)
        lo = cases.UNCOUNTED_ANCHOR_TILE * 32
        assert c.B > lo + 32 and not counted[lo:lo + 32].any() and counted[lo + 32:].all()
        assert pos[0] == 0 and pos[1] == c.n_rows - 1 and len({int(pos[i]) for i in cases.SHARED}) == 1
        assert [int(pos[i]) for i in cases.UNCOUNTED] == [c.n_rows, -1, 2**31 - 1, -2**31] and not counted[6:10].any()
    for name in ("far-maximum-f32", "far-maximum-bf16"):
        c = by[name]
        _, rows, anchors, delta, pos = cases.inputs(name)
        n_splits, per_split = cases.plan(c.B, c.n_rows)
        z = ref.apply(delta, anchors)
        best = np.argmax((z / np.linalg.norm(z, axis=1, keepdims=True)) @ rows.T, axis=1)
        split = lambda r: int(r) // per_split  # noqa: E731
        assert (split(best[0]), split(pos[0])) == (n_splits - 1, 0) and (split(best[1]), split(pos[1])) == (0, n_splits - 1)
    assert {(c.storage, c.dim) for c in cases.CASES} >= {("f32", 384), ("bf16", 384), ("f32", 1024), ("bf16", 1024)}
    assert {s for c in cases.CASES for s in c.scales} == {20.0, 30.0, 100.0}


# ---------------------------------------------------------------- host arguments
def test_fit_plan_and_the_command_line_accept_all():
    assert adapter.fit_plan(1000, 5, 64, "all", 1e-3, 0.01, 30.0) == adapter.fit_plan(1000, 5, 64, 0, 1e-3, 0.01, 30.0)
    assert adapter.fit_plan(5000, 1, 1024, "all", 1e-3, 0.01, 30.0) == (1024, 4, 4, 0)  # no list, so no limit on its length
    for bad in ("ALL", "some", "", None, 1.5, True, -1, 8193):
        with pytest.raises(ValueError, match="negatives must be an integer in"):
            adapter.fit_plan(100, 1, 64, bad, 1e-3, 0.01, 30.0)
    with pytest.raises(ValueError, match="exceeds the limit"):
        adapter.fit_plan(100, 1, 1024, 7169, 1e-3, 0.01, 30.0)
    with pytest.raises(ValueError, match="batch_size"):
        adapter.fit_plan(100, 1, 1025, "all", 1e-3, 0.01, 30.0)
    assert cli.negatives_arg("all") == "all" and cli.negatives_arg("0") == 0 and cli.negatives_arg("7936") == 7936
    for bad in ("ALL", "1.5", ""):
        with pytest.raises(ValueError):
            cli.negatives_arg(bad)


# ---------------------------------------------------------------- learning
def test_reference_with_catalog_steps_solves_the_learning_task():
    """tests/test_adapter.py's task and thresholds, every step against all 2,048 rows."""
    P, a_train, p_train, a_held, p_held = ref.learning_task()
    rows = ref.stored_rows(P)
    d = ref.TASK_DIM
    delta, m, v, t = np.zeros((d, d)), np.zeros((d, d)), np.zeros((d, d)), 0
    assert ref.recall_at(ref.top_rows(a_held, rows, 10), p_held) <= 0.05
    losses = []
    for step in range(ref.TASK_STEPS):
        at = ref.task_batch(step)
        loss, grad = ref.loss_and_grad_catalog(delta, a_train[at], rows, p_train[at], ref.TASK_SCALE, torch.float64)
        delta, m, v, t, _ = ref.adamw(delta, m, v, t, grad, ref.TASK_LR, weight_decay=ref.TASK_DECAY)
        losses.append(loss)
    after = ref.recall_at(ref.top_rows(ref.apply(delta, a_held), rows, 10), p_held)
    print(f"recall@10 -> {after:.4f}, loss {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert after >= 0.99 and losses[-1] < 0.5 * losses[0]
