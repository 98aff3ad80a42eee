"""The adapter's step over per-anchor lists without a GPU: tests/adapter_reference.py's loss_and_grad_lists against the
pair reference on a shared one-hot list and against central differences, that every case of
tests/adapter_lists_cases.py reaches the path it names, impression_csr, the plan function's refusals, the command line's --lists and --gain, and the C entry's
refusals before any HIP call."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native, cli
from instacart_next_order_recommendation_amd.adapter import impression_csr
from instacart_next_order_recommendation_amd.recommender import DEFAULT_GAINS, Recommender, adapter_lists_plan
from tests import adapter_lists_cases as lc
from tests import adapter_reference as ref
from tests.recommender_harness import forbid_gpu_work
from tests.test_adapter import NoModel, StubPath, world


# ---------------------------------------------------------------- the reference
def test_shared_one_hot_list_is_the_pair_loss_in_float64():
    rows, anchors, delta = world(d=8, n_rows=40, B=5)
    rng = np.random.default_rng(1)
    cand = rng.choice(40, 17, replace=False)  # distinct and in range: nothing is masked
    want_loss, want_grad = ref.loss_and_grad(delta, anchors, rows, cand, 30.0)
    one_hot = np.zeros((5, 17), np.float32)
    one_hot[np.arange(5), np.arange(5)] = 3.0  # any positive gain: t = gain / T = 1
    loss, grad = ref.loss_and_grad_lists(delta, anchors, rows, *ref.uniform_csr(np.tile(cand, (5, 1)), one_hot), 30.0)
    assert abs(loss - want_loss) <= 1e-12 and np.abs(grad - want_grad).max() <= 1e-12


def test_gradient_matches_central_differences():
    rows, anchors, delta = world(d=6, n_rows=12, B=4)
    off = np.asarray([0, 4, 4, 9, 7])  # an empty segment and one whose end lies before its start
    lrows = np.asarray([3, 7, 12, 0, 5, 5, -1, 2, 9])
    target = np.asarray([1, 0, 4, 2, 0.5, 2, 1, np.nan, 0], np.float32)
    loss, grad = ref.loss_and_grad_lists(delta, anchors, rows, off, lrows, target, 4, 30.0)
    _, _, _, live, counted = ref.masks_lists(off, lrows, target, 4, 12)
    assert counted.tolist() == [True, False, True, False] and live.sum() == 3 + 2 and np.abs(grad).max() > 1e-3
    h = 1e-6
    for r in range(6):
        for c in range(6):
            up, down = delta.copy(), delta.copy()
            up[r, c] += h
            down[r, c] -= h
            fd = (ref.loss_and_grad_lists(up, anchors, rows, off, lrows, target, 4, 30.0)[0]
                  - ref.loss_and_grad_lists(down, anchors, rows, off, lrows, target, 4, 30.0)[0]) / (2 * h)
            assert abs(fd - grad[r, c]) <= 1e-6 * max(1.0, abs(grad[r, c])), (r, c, fd, grad[r, c])


def test_one_live_entry_and_nobody_counted_are_exactly_zero():
    rows, anchors, delta = world(d=8, n_rows=12, B=3)
    one = (np.asarray([0, 1, 4, 5]), np.asarray([3, -1, 5, 12, 7]), np.asarray([2, 1, 1, 1, 0.5], np.float32), 8)
    loss, grad = ref.loss_and_grad_lists(delta, anchors, rows, *one, 30.0)
    assert ref.masks_lists(*one, 12)[4].all() and loss == 0.0 and np.abs(grad).max() <= 1e-15
    nobody = (np.asarray([0, 2, 2, 4]), np.asarray([3, 4, 12, -1]), np.asarray([0, 0, 1, 1], np.float32), 8)
    assert ref.loss_and_grad_lists(delta, anchors, rows, *nobody, 30.0) == (0.0, pytest.approx(np.zeros((8, 8))))


# ---------------------------------------------------------------- the cases reach their paths
def test_every_case_reaches_the_path_it_names():
    assert len({c.name for c in lc.CASES}) == len(lc.CASES)
    assert {(c.storage, c.dim) for c in lc.CASES} >= {("f32", 32), ("f32", 96), ("f32", 384), ("f32", 1024), ("bf16", 64),
                                                      ("bf16", 384), ("bf16", 768)}
    assert {c.B for c in lc.CASES} >= {1, 33, 65, 257, lc.MAX_BATCH}
    seen_lengths = set()
    for c in lc.CASES:
        _, stored, anchors, delta, lists = lc.inputs(c.name)
        off, rows, target, max_len = lists
        assert off.shape == (c.B + 1,) and 1 <= max_len <= lc.MAX_LIST and off.min() >= 0 and off.max() <= len(rows)
        r, t, read, live, counted = ref.masks_lists(*lists, c.n_rows)
        assert counted.any() and stored.shape == (c.n_rows, c.dim)
        lengths = read.sum(axis=1)
        seen_lengths |= set(lengths.tolist())
        if c.lists == "uniform":
            assert (lengths == c.L).all() and live.all() and counted.all()
        if c.name == "head-only":
            assert (np.diff(off) == 150).all() and (lengths == 100).all() and live.all()
            beyond = target.reshape(c.B, 150)[:, 100:]
            assert (beyond == 1e6).all() and (rows.reshape(c.B, 150)[:, 100::2] >= c.n_rows).all()
        if c.name == "batch-limit":
            assert c.B == lc.MAX_BATCH == 16 * lc.GRAD_BLOCK
        if c.name == "list-limit":
            assert c.L == lc.MAX_LIST == 8 * lc.GROUP and (lengths == lc.MAX_LIST).all()
        if c.name == "edge-lengths":
            assert set(lengths.tolist()) == set(lc.EDGE_LENGTHS)
        if c.lists == "mixed":
            at = lc.MIXED
            assert lengths[at["empty"]] == 0 and off[at["empty"] + 1] == off[at["empty"]]
            assert off[at["reversed"] + 1] < off[at["reversed"]] and lengths[at["reversed"]] == 0
            assert lengths[at["reversed"] + 1] > 3  # the segment behind it begins three entries early
            for name in ("empty", "reversed", "all zero targets", "all dropped"):
                assert not counted[at[name]], name
            assert live[at["all zero targets"]].any() and not live[at["all dropped"]].any()
            assert counted.sum() == c.B - 4
            e = at["edge rows"]
            assert r[e, :6].tolist() == [0, c.n_rows - 1, c.n_rows, -1, 2**31 - 1, -(2**31)]
            assert live[e, :6].tolist() == [True, True, False, False, False, False]
            b, n = at["bad targets"], lengths[at["bad targets"]]
            assert np.isnan(t[b, n - 5]) and t[b, n - 4] == -1 and np.isposinf(t[b, n - 3]) and np.isneginf(t[b, n - 2])
            assert live[b, n - 5:n].tolist() == [False, False, False, False, True]  # -0.0 is >= 0
            d, n = at["duplicate"], lengths[at["duplicate"]]
            assert r[d, n - 2:n].tolist() == r[d, :2].tolist() and live[d, :n].all()
            o = at["one live among dropped"]
            assert live[o, :4].tolist() == [False, True, False, False] and counted[o]
            p = at["probabilities"]
            assert abs(float(t[p].sum()) - 1) < 1e-5 and not np.isin(t[p][live[p]], lc.GAINS).all()
            assert len(set(lengths.tolist())) > 20  # mixed lengths
    assert seen_lengths >= set(lc.EDGE_LENGTHS) | {0, 8, 1024}
    # a lane's chain over entries lane, lane + 64, .. has one term, two terms, sixteen; sweep 2 a partial round and 8 groups
    assert {1, 2, 63, 64, 65, 100, 1024} <= seen_lengths and 63 % lc.DEPTH and 1024 // lc.GROUP == 8


def test_one_live_entry_in_a_case_has_no_loss_of_its_own():
    _, stored, anchors, delta, lists = lc.inputs("edge-lengths")
    losses, counted = ref.per_anchor_losses(delta, anchors, stored, *lists, 30.0)
    lengths = ref.masks_lists(*lists, stored.shape[0])[2].sum(axis=1)
    assert counted.all() and (losses.numpy()[lengths == 1] == 0).all() and (losses.numpy()[lengths > 1] > 0).all()


# ---------------------------------------------------------------- impression_csr
def test_impression_csr():
    off, rows, target, max_len = impression_csr([{3: 1, 7: 0.0}, [(5, 2), (5, 4.5), (9, 0), (5, 1)], [], [(2**40, 1), (-3, 1)]], 4)
    assert (off.dtype, rows.dtype, target.dtype) == (torch.int32, torch.int32, torch.float32)
    assert off.tolist() == [0, 2, 4, 4, 6] and rows.tolist() == [3, 7, 5, 9, -1, -1] and max_len == 2
    assert target.tolist() == [1.0, 0.0, 4.5, 0.0, 1.0, 1.0]  # the duplicated row keeps the larger gain, at its first place
    assert impression_csr([[]], 1)[3] == 1 and impression_csr([[]], 1)[0].tolist() == [0, 0]
    full = [[(r, 1) for r in range(_native.ICREC_ADAPTER_MAX_LIST)]]
    assert impression_csr(full, 1)[3] == _native.ICREC_ADAPTER_MAX_LIST
    with pytest.raises(ValueError, match="the limit is 1024"):
        impression_csr([full[0] + [(5000, 1)]], 1)
    impression_csr([full[0] + [(5, 2)]], 1)  # 1,025 pairs, 1,024 entries
    for bad, text in (("abc", "not a string"), (["abc", [], [], []], "list 0 must be"), ([[(1, 1)]] * 3, "4 anchors for 3 lists")):
        with pytest.raises(ValueError, match=text):
            impression_csr(bad, 4)


# ---------------------------------------------------------------- the plan function, the command line
def test_fit_adapter_lists_checks_its_arguments_before_any_gpu_work(monkeypatch):
    rec = Recommender.__new__(Recommender)
    rec.model = NoModel()
    rec.product_ids = [str(i + 1) for i in range(6)]
    rec._pid_to_row = {p: i for i, p in enumerate(rec.product_ids)}
    rec._fast_path = lambda: StubPath()
    forbid_gpu_work(rec, monkeypatch)
    assert DEFAULT_GAINS == {"impression": 0, "click": 1, "add_to_cart": 2, "purchase": 4}
    good = [("milk and eggs", {"1": "click", "2": "impression", "3": 2.5}), ("bread", {"6": "purchase"})]
    assert adapter_lists_plan(good, rec._pid_to_row, DEFAULT_GAINS, 5, 64, 1e-3, 0.01, 30.0) == \
        (["milk and eggs", "bread"], [[(0, 1.0), (1, 0.0), (2, 2.5)], [(5, 4.0)]])
    assert adapter_lists_plan(good[1:], rec._pid_to_row, {"purchase": 9}, 1, 1, 1e-3, 0.0, 30.0)[1] == [[(5, 9.0)]]
    nan, inf = float("nan"), float("inf")
    for impressions, kw, text in (
            ([("milk", {"7": "click"})], {}, "unknown product id '7' in impression 0"),
            (good + [("tea", {"1": "returned"})], {}, "unknown event 'returned' for product '1' in impression 2"),
            ([("milk", {"1": -1})], {}, "finite number >= 0, got -1 for product '1' in impression 0"),
            ([("milk", {"1": nan})], {}, "finite number >= 0"), ([("milk", {"1": inf})], {}, "finite number >= 0"),
            ([("milk", {"1": True})], {}, "finite number >= 0"),
            (good + [("tea", {"1": "impression", "2": 0})], {}, "impression 2 has no product with a positive gain"),
            (good + [("tea", {})], {}, "impression 2 has no product"),
            (good[1:] + [("tea", {"1": "click"})], dict(where=["f.jsonl:1", "f.jsonl:4"], gains={"click": 0, "purchase": 1}),
             "f.jsonl:4 has no product"),
            (good, dict(gains={"click": -2, "impression": 0, "purchase": 1}), "got -2 for event 'click'"),
            ("milk", {}, "sequence of"), ({"milk": {"1": 1}}, {}, "sequence of"), ([("milk",)], {}, "impression 0 is not"),
            ([("milk", "1")], {}, "impression 0 is not"), ([(3, {"1": 1})], {}, "must be a string"), ([], {}, "at least one"),
            ([("milk", {str(i): 1 for i in range(1025)})], {}, "the limit is 1024"),
            (good, dict(epochs=0), "epochs"), (good, dict(batch_size=2000), "batch_size"), (good, dict(lr=nan), "lr"),
            (good, dict(scale=inf), "scale")):
        with pytest.raises(ValueError, match=text):
            rec.fit_adapter_lists(impressions, **kw)
    with pytest.raises(AssertionError, match="model.encode_to_device used"):  # good arguments reach the encoder
        rec.fit_adapter_lists(good)


def test_command_line_reads_lists_and_gains(tmp_path, capsys):
    path = tmp_path / "lists.jsonl"
    path.write_text('{"anchor": "milk and eggs", "products": {"17": "click", "p9": 2.5}}\n\n'
                    '{"anchor": "bread", "products": {"3": "purchase"}, "request_id": "r1"}\n')
    lists, where = cli.read_lists(path)
    assert lists == [("milk and eggs", {"17": "click", "p9": 2.5}), ("bread", {"3": "purchase"})]
    assert where == [f"{path}:1", f"{path}:3"]
    for bad, line in (('{"anchor": "x"}\n', 1), ('{"anchor": "x", "products": {"1": 1}}\nnot json\n', 2), ('["x", {}]\n', 1),
                      ('{"anchor": 3, "products": {}}\n', 1), ('{"anchor": "x", "products": ["1"]}\n', 1)):
        path.write_text(bad)
        with pytest.raises(ValueError, match=f"lists.jsonl:{line}"):
            cli.read_lists(path)
    assert cli.gain_args(None, DEFAULT_GAINS) == DEFAULT_GAINS
    assert cli.gain_args(["click=0.5", "returned=0"], DEFAULT_GAINS) == {**DEFAULT_GAINS, "click": 0.5, "returned": 0.0}
    for bad in ("click", "click=much", "=3"):
        with pytest.raises(ValueError, match="EVENT=number"):
            cli.gain_args([bad], DEFAULT_GAINS)
    cfg_path = tmp_path / "inference.yaml"
    cfg_path.write_text(f"model_dir: m\ncorpus: {cfg_path}\n")
    base = ["fit-adapter", "--config", str(cfg_path), "--out", str(tmp_path / "o.npz")]
    for extra in ([], ["--pairs", str(path), "--lists", str(path)], ["--pairs", str(path), "--gain", "click=2"]):
        with pytest.raises(SystemExit):
            cli.main(base + extra)
        assert "exactly one of --pairs and --lists" in capsys.readouterr().err or extra[-2:] == ["--gain", "click=2"]
    with pytest.raises(SystemExit, match="lists file"):
        cli.main(base + ["--lists", str(tmp_path / "none.jsonl")])
    path.write_text('{"anchor": "x", "products": {"1": "click"}}\n')
    with pytest.raises(SystemExit, match="EVENT=number"):
        cli.main(base + ["--lists", str(path), "--gain", "click"])


# ---------------------------------------------------------------- the C entry
def test_entry_point_validates_arguments_without_a_gpu():
    lib = _native.lib()
    assert lib.icrec_adapter_step_lists_workspace_bytes(None, 4) == 0
    assert lib.icrec_adapter_step_lists(None, None, None, 1, None, None, None, 1, 30.0, 0.0, 0.9, 0.999, 1e-8, 0.0, 0, None, None,
                                        None, 0, None) == -1
    assert b"icrec_adapter_step_lists: NULL idx" in lib.icrec_last_error()
    assert _native.ICREC_ADAPTER_MAX_LIST == 1024
    header = (_native._PKG.parent / "include" / "icrec.h").read_text()
    assert "#define ICREC_ADAPTER_MAX_LIST 1024" in header
