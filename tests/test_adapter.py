"""The query adapter without a GPU: tests/adapter_reference.py against central differences and its own masking rules,
the identity at delta = 0, the adapter file's round trip, the learning schedule, fit_adapter's argument checks on a
Recommender made with __new__, and the learning task of tests/test_adapter_gpu.py solved by the reference alone."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native, adapter
from instacart_next_order_recommendation_amd.recommender import Recommender, adapter_pairs_plan
from tests import adapter_reference as ref
from tests.recommender_harness import forbid_gpu_work


def world(d=8, n_rows=12, B=5, seed=0):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n_rows, d))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    anchors = rng.standard_normal((B, d))
    anchors /= np.linalg.norm(anchors, axis=1, keepdims=True)
    delta = rng.standard_normal((d, d)) * (0.3 / np.sqrt(d))
    return rows, anchors, delta


def test_gradient_matches_central_differences():
    rows, anchors, delta = world()
    cand = np.array([3, 7, 3, 12, 0, 7, 9, -1, 5])  # a repeated positive, a negative equal to a positive, two ids out of range
    loss, grad = ref.loss_and_grad(delta, anchors, rows, cand, 30.0)
    assert np.isfinite(loss) and np.abs(grad).max() > 1e-3
    h = 1e-6
    for r in range(delta.shape[0]):
        for c in range(delta.shape[1]):
            up, down = delta.copy(), delta.copy()
            up[r, c] += h
            down[r, c] -= h
            fd = (ref.loss_and_grad(up, anchors, rows, cand, 30.0)[0] - ref.loss_and_grad(down, anchors, rows, cand, 30.0)[0]) / (2 * h)
            assert abs(fd - grad[r, c]) <= 1e-6 * max(1.0, abs(grad[r, c])), (r, c, fd, grad[r, c])


def plain_loss(delta, anchors, rows, cand, scale, keep):
    """The loss written out with loops: keep[i] lists the candidate positions anchor i's softmax runs over."""
    z = anchors + anchors @ delta.T
    u = z / np.linalg.norm(z, axis=1, keepdims=True)
    per = []
    for i, js in keep.items():
        s = scale * np.array([u[i] @ rows[cand[j]] for j in js])
        per.append(np.log(np.exp(s - s.max()).sum()) + s.max() - scale * (u[i] @ rows[cand[i]]))
    return float(np.mean(per))


def test_masking_rules():
    rows, anchors, delta = world(B=3)
    # a second copy of anchor 0's positive (position 3) is masked for anchor 0 only
    cand = np.array([4, 5, 6, 4, 8])
    want = plain_loss(delta, anchors, rows, cand, 30.0, {0: [0, 1, 2, 4], 1: [0, 1, 2, 3, 4], 2: [0, 1, 2, 3, 4]})
    assert ref.loss_and_grad(delta, anchors, rows, cand, 30.0)[0] == pytest.approx(want, rel=1e-12)
    # two anchors with the same positive: each masks the other's copy
    cand = np.array([4, 4, 6])
    want = plain_loss(delta, anchors, rows, cand, 30.0, {0: [0, 2], 1: [1, 2], 2: [0, 1, 2]})
    assert ref.loss_and_grad(delta, anchors, rows, cand, 30.0)[0] == pytest.approx(want, rel=1e-12)
    # candidates out of range are masked for everybody
    cand = np.array([4, 5, 6, -1, 12])
    want = plain_loss(delta, anchors, rows, cand, 30.0, {i: [0, 1, 2] for i in range(3)})
    assert ref.loss_and_grad(delta, anchors, rows, cand, 30.0)[0] == pytest.approx(want, rel=1e-12)
    # an anchor whose own positive is out of range is not counted and has no gradient: the loss is the other two's,
    # over the candidates that are left, and moving that anchor changes nothing
    cand = np.array([4, 12, 6, 7])
    want = plain_loss(delta, anchors, rows, cand, 30.0, {0: [0, 2, 3], 2: [0, 2, 3]})
    loss, grad = ref.loss_and_grad(delta, anchors, rows, cand, 30.0)
    assert loss == pytest.approx(want, rel=1e-12)
    moved = anchors.copy()
    moved[1] = -moved[1][::-1]
    loss2, grad2 = ref.loss_and_grad(delta, moved, rows, cand, 30.0)
    assert loss2 == loss and np.array_equal(grad2, grad)
    # nobody counted: loss 0, gradient 0
    loss, grad = ref.loss_and_grad(delta, anchors, rows, np.array([-1, 12, 99, 3]), 30.0)
    assert loss == 0.0 and not grad.any()
    # one anchor, one candidate, and every positive the same row with C = B: the gradient is exactly zero
    for cand in (np.array([4]), np.array([4, 4, 4])):
        loss, grad = ref.loss_and_grad(delta, anchors[:len(cand)], rows, cand, 30.0)
        assert loss == 0.0 and not grad.any()


def test_apply_is_the_two_rounding_chain_and_the_identity_at_zero():
    rng = np.random.default_rng(1)
    q = rng.standard_normal((5, 32)).astype(np.float32)
    delta = (rng.standard_normal((32, 32)) * 0.05).astype(np.float32)
    got = ref.apply(delta, q)
    assert got.dtype == np.float32
    for n in (0, 4):
        for r in (0, 31):
            acc = np.float32(0)
            for c in range(32):
                acc = np.float32(acc + np.float32(delta[r, c] * q[n, c]))
            assert got[n, r] == np.float32(q[n, r] + acc)
    np.testing.assert_allclose(got, q + q @ delta.T, rtol=0, atol=1e-5)
    assert np.array_equal(ref.apply(np.zeros((32, 32), np.float32), q), q)
    # a row has the same bits alone and inside the batch
    assert np.array_equal(ref.apply(delta, q[3:4])[0], got[3])


def test_adamw_reference_is_torchs():
    rng = np.random.default_rng(2)
    delta, m, g = (rng.standard_normal((4, 4)) for _ in range(3))
    v = rng.random((4, 4))
    p = torch.nn.Parameter(torch.tensor(delta))
    opt = torch.optim.AdamW([p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.tensor(m), "exp_avg_sq": torch.tensor(v)}
    p.grad = torch.tensor(g)
    opt.step()
    new_delta, new_m, new_v, t, _ = ref.adamw(delta, m, v, 7, g, 1e-2)
    assert t == 8
    np.testing.assert_allclose(new_delta, p.detach().numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(new_m, opt.state[p]["exp_avg"].numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(new_v, opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-13, atol=0)


def test_adapter_file_round_trip(tmp_path):
    delta = np.random.default_rng(3).standard_normal((32, 32)).astype(np.float32)
    path = tmp_path / "adapter.npz"
    adapter.write_adapter_file(path, delta, 20.0, 123)
    assert path.exists() and not (tmp_path / "adapter.npz.npz").exists()
    got, scale, steps = adapter.read_adapter_file(path)
    assert np.array_equal(got, delta) and got.dtype == np.float32 and (scale, steps) == (20.0, 123)
    with np.load(path) as z:
        assert sorted(z.files) == ["delta", "dim", "scale", "steps"] and int(z["dim"]) == 32
    np.savez(tmp_path / "other.npz", delta=delta)
    with pytest.raises(ValueError, match="not an adapter file"):
        adapter.read_adapter_file(tmp_path / "other.npz")
    with pytest.raises(ValueError, match="square"):
        adapter.write_adapter_file(path, delta[:, :16], 30.0, 0)
    bad = delta.copy()
    bad[0, 0] = np.nan
    adapter.write_adapter_file(path, bad, 30.0, 0)
    with pytest.raises(ValueError, match="finite"):
        adapter.read_adapter_file(path)


def test_schedule_and_fit_plan():
    # warm-up over the first 10 % of the steps from 0, then a cosine to (almost) zero
    total, warmup = 100, 10
    f = [adapter.schedule(s, total, warmup) for s in range(total)]
    assert f[0] == 0.0 and f[5] == 0.5 and f[10] == 1.0 and all(a > b for a, b in zip(f[10:], f[11:])) and 0 < f[-1] < 1e-3
    assert adapter.schedule(0, 5, 0) == 1.0
    # drop_last, unless there is less than one batch
    assert adapter.fit_plan(1000, 5, 64, 0, 1e-3, 0.01, 30.0) == (64, 15, 75, 7)
    assert adapter.fit_plan(10, 3, 64, 0, 1e-3, 0.01, 30.0) == (10, 1, 3, 0)
    for kw, text in ((dict(n_pairs=0), "at least one"), (dict(epochs=0), "epochs"), (dict(batch_size=1025), "batch_size"),
                     (dict(batch_size=True), "batch_size"), (dict(negatives=-1), "negatives"),
                     (dict(batch_size=1024, negatives=7169), "exceeds the limit"), (dict(lr=float("nan")), "lr"),
                     (dict(lr=-1.0), "lr"), (dict(weight_decay=float("inf")), "weight_decay"), (dict(scale="x"), "scale")):
        args = dict(n_pairs=100, epochs=1, batch_size=64, negatives=0, lr=1e-3, weight_decay=0.01, scale=30.0)
        with pytest.raises(ValueError, match=text):
            adapter.fit_plan(**{**args, **kw})


class NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"model.{name} used before the arguments were checked")


class StubPath:
    def run(self, *a, **kw):
        raise AssertionError("unused")


def test_fit_adapter_checks_its_arguments_before_any_gpu_work(monkeypatch):
    rec = Recommender.__new__(Recommender)
    rec.model = NoModel()
    rec.product_ids = [str(i + 1) for i in range(6)]
    rec._pid_to_row = {p: i for i, p in enumerate(rec.product_ids)}
    rec._fast_path = lambda: StubPath()
    forbid_gpu_work(rec, monkeypatch)
    good = [("milk and eggs", "1"), ("bread", "6")]
    assert adapter_pairs_plan(good, rec._pid_to_row, 5, 64, 0, 1e-3, 0.01, 30.0) == (["milk and eggs", "bread"], [0, 5])
    for pairs, kw, text in (([("milk", "7")], {}, "unknown product id '7' in pair 0"),
                            (good + [("tea", "no such")], {}, "unknown product id 'no such' in pair 2"),
                            ("milk", {}, "sequence of"), ({"milk": "1"}, {}, "sequence of"), ([("milk",)], {}, "pair 0 is not"),
                            (["m1"], {}, "pair 0 is not"), ([(3, "1")], {}, "must be a string"), ([], {}, "at least one"),
                            (good, dict(epochs=0), "epochs"), (good, dict(batch_size=0), "batch_size"),
                            (good, dict(negatives=9000), "negatives"), (good, dict(lr=float("nan")), "lr"),
                            (good, dict(scale=float("inf")), "scale")):
        with pytest.raises(ValueError, match=text):
            rec.fit_adapter(pairs, **kw)
    with pytest.raises(AssertionError, match="model.encode_to_device used"):  # good arguments reach the encoder
        rec.fit_adapter(good)


def test_command_line_reads_pairs_and_the_adapter_path(tmp_path):
    from instacart_next_order_recommendation_amd import cli

    pairs = tmp_path / "pairs.jsonl"
    pairs.write_text('{"anchor": "milk and eggs", "positive": 17}\n\n{"anchor": "bread", "positive": "p9", "extra": 1}\n')
    assert cli.read_pairs(pairs) == [("milk and eggs", "17"), ("bread", "p9")]
    for bad, line in (('{"anchor": "x"}\n', 1), ('{"anchor": "x", "positive": "1"}\nnot json\n', 2), ('["x", "1"]\n', 1),
                      ('{"anchor": 3, "positive": "1"}\n', 1)):
        pairs.write_text(bad)
        with pytest.raises(ValueError, match=f"pairs.jsonl:{line}"):
            cli.read_pairs(pairs)
    cfg_path = tmp_path / "inference.yaml"
    cfg_path.write_text("model_dir: m\ncorpus: c.json\n")
    cfg = cli.read_settings(cfg_path)
    assert cfg["adapter_path"] is None and cli.adapter_file(cfg, None) is None
    (tmp_path / "a.npz").write_bytes(b"")
    cfg_path.write_text(f"model_dir: m\ncorpus: c.json\nadapter_path: {tmp_path / 'a.npz'}\n")
    cfg = cli.read_settings(cfg_path)
    assert cli.adapter_file(cfg, None) == tmp_path / "a.npz"
    (tmp_path / "b.npz").write_bytes(b"")
    assert cli.adapter_file(cfg, tmp_path / "b.npz") == tmp_path / "b.npz"  # the command line beats the config
    with pytest.raises(SystemExit, match="does not exist"):
        cli.adapter_file(cfg, tmp_path / "missing.npz")
    args = cli.build_parser().parse_args(["--adapter", "x.npz"])
    assert str(args.adapter) == "x.npz" and cli.build_parser().parse_args([]).adapter is None
    with pytest.raises(SystemExit, match="pairs file"):
        cfg_path.write_text(f"model_dir: m\ncorpus: {cfg_path}\n")
        cli.main(["fit-adapter", "--config", str(cfg_path), "--pairs", str(tmp_path / "none.jsonl"), "--out", str(tmp_path / "o.npz")])


def test_entry_points_validate_arguments_without_a_gpu():
    """The C entry points refuse bad arguments before any HIP call."""
    lib = _native.lib()
    h = C.c_void_p()
    for dim in (0, 16, 48, 1056, -32):
        assert lib.icrec_adapter_create(dim, 0, C.byref(h)) == -1 and not h.value
        assert b"multiple of 32" in lib.icrec_last_error()
    assert lib.icrec_adapter_create(64, 0, None) == -1
    assert lib.icrec_adapter_dim(None) == 0 and lib.icrec_adapter_destroy(None) == 0
    assert lib.icrec_adapter_step_workspace_bytes(None, 4, 4) == 0
    assert lib.icrec_adapter_apply(None, None, 1, None, None) == -1 and b"NULL adapter" in lib.icrec_last_error()
    assert lib.icrec_adapter_set_state(None, None, None, None, 0) == -1
    assert lib.icrec_adapter_get_state(None, None, None, None, None) == -1
    assert lib.icrec_adapter_step(None, None, None, 1, None, 1, 30.0, 0.0, 0.9, 0.999, 1e-8, 0.0, 0, None, None, None, 0, None) == -1
    assert (_native.ICREC_ADAPTER_MAX_DIM, _native.ICREC_ADAPTER_MAX_BATCH, _native.ICREC_ADAPTER_MAX_CANDIDATES) == (1024, 1024, 8192)
    header = (_native._PKG.parent / "include" / "icrec.h").read_text()
    for name in ("ICREC_ADAPTER_MAX_DIM 1024", "ICREC_ADAPTER_MAX_BATCH 1024", "ICREC_ADAPTER_MAX_CANDIDATES 8192"):
        assert f"#define {name}" in header


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_reference_solves_the_learning_task(dtype):
    """The task of test_adapter_gpu's end-to-end test, by the reference alone: held-out recall@10 from (almost) nothing to
    1.0 in 100 AdamW steps."""
    P, a_train, p_train, a_held, p_held = ref.learning_task()
    rows = ref.stored_rows(P)
    d = ref.TASK_DIM
    delta, m, v, t = np.zeros((d, d)), np.zeros((d, d)), np.zeros((d, d)), 0
    before = ref.recall_at(ref.top_rows(a_held, rows, 10), p_held)
    assert before <= 0.05
    losses = []
    for step in range(ref.TASK_STEPS):
        at = ref.task_batch(step)
        loss, grad = ref.loss_and_grad(delta, a_train[at], rows, p_train[at], ref.TASK_SCALE, dtype)
        delta, m, v, t, _ = ref.adamw(delta, m, v, t, grad, ref.TASK_LR, weight_decay=ref.TASK_DECAY)
        losses.append(loss)
    after = ref.recall_at(ref.top_rows(ref.apply(delta, a_held), rows, 10), p_held)
    print(f"recall@10 {before:.4f} -> {after:.4f}, loss {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert after >= 0.99 and losses[-1] < 0.5 * losses[0]
