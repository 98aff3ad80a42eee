"""What the adapter's GPU tests share: the three kinds of step (pairs, catalog, lists) as one table - how a case's
targets go to the device, which QueryAdapter methods and which C entry take them, which function of
tests/adapter_reference.py is the truth and which margins hold - the references of a case, computed once, the one
comparison of a device step with them, AdamW's bounds, and one body for every test the three kinds have alike.
Importing this needs no GPU."""
from __future__ import annotations

import functools
from typing import Callable, NamedTuple

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.adapter import QueryAdapter
from instacart_next_order_recommendation_amd.search import DeviceIndex
from tests import adapter_reference as ref
from tests.token_states import check

DEV = "cuda:0"


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def small_delta(rng, d):
    return (rng.standard_normal((d, d)) * (0.05 / np.sqrt(d))).astype(np.float32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def adapter_with(delta, m=None, v=None, t=0) -> QueryAdapter:
    ad = QueryAdapter(delta.shape[0], DEV)
    ad.load_state({"delta": delta, "m": m, "v": v, "t": t})
    return ad


def bits(loss: float, grad: np.ndarray):
    return np.float32(loss).tobytes(), np.ascontiguousarray(grad, np.float32).tobytes()


def device_lists(lists, device=DEV):
    """A case's lists as QueryAdapter takes them ready made: (off int32, rows int32, target float32, max_len) on `device`;
    a row beyond int32 is out of range for any index: -1."""
    off, rows, target, max_len = lists
    rows = np.where((rows < 0) | (rows > 2**31 - 1), -1, rows)
    return (torch.from_numpy(off.astype(np.int32)).to(device), torch.from_numpy(rows.astype(np.int32)).to(device),
            torch.from_numpy(np.ascontiguousarray(target, np.float32)).to(device), int(max_len))


# ---------------------------------------------------------------- the kinds of step
class Kind(NamedTuple):
    """A case's targets are what its inputs() end with: the candidates, the labels, or the tuple (off, rows, target,
    max_len); as the C entry's middle arguments they are int32 device arrays and counts."""
    loss_and_grad: str    # the QueryAdapter method without an update ..
    step: str             # .. and with one
    entry: str            # the C entry; entry + "_workspace_bytes" sizes its workspace
    list_name: str        # what its messages call the first of its target arrays
    reference: Callable   # tests/adapter_reference.py's (delta, anchors, stored, *targets, scale, dtype) -> (loss, grad)
    to_device: Callable   # host targets -> what the two methods take
    middle: Callable      # to_device's value -> the C entry's arguments between B and scale, tensors for pointers
    workspace_args: Callable  # (adapter handle, index handle, B, middle) -> the arguments of entry_workspace_bytes
    margins: dict         # margin on E_ref per (storage, dim), for the gradient's rms and max-abs error and for the loss


def _rows32(rows):
    return torch.from_numpy(np.asarray(rows)).to(DEV, torch.int32)


KINDS = {
    "pairs": Kind(
        "loss_and_grad", "step", "icrec_adapter_step", "cand_rows", ref.loss_and_grad,
        lambda cand: torch.from_numpy(np.asarray(cand)), lambda cand: (_rows32(cand), int(cand.shape[0])),
        lambda ad, ix, B, middle: (ad, B, middle[1]),
        # the smallest of {2, 3, 4, 6, 8} that leaves 1.5x headroom over the worst ratio measured on the MI355X
        # (profiles/adapter_errors.md)
        {("f32", 32): 2, ("f32", 64): 4, ("f32", 96): 6, ("f32", 384): 6, ("bf16", 384): 6, ("bf16", 768): 6,
         # the pairs only tests/test_adapter_edges_gpu.py runs (worst ratios 1.09, 1.05, 1.08, 1.08, 1.01)
         ("bf16", 64): 2, ("bf16", 128): 2, ("f32", 768): 2, ("f32", 1024): 2, ("bf16", 1024): 2}),
    "catalog": Kind(
        "loss_and_grad_catalog", "step_catalog", "icrec_adapter_step_catalog", "pos_rows", ref.loss_and_grad_catalog,
        lambda pos: torch.from_numpy(np.asarray(pos)), lambda pos: (_rows32(pos),), lambda ad, ix, B, middle: (ad, ix, B),
        # the smallest of {2, 3, 4, 6, 8} that leaves 1.5x headroom over the worst ratio measured on the MI355X
        # (profiles/adapter_catalog_errors.md)
        {("f32", 32): 2, ("f32", 64): 2, ("f32", 96): 2, ("f32", 384): 4, ("f32", 1024): 2,
         ("bf16", 64): 2, ("bf16", 128): 2, ("bf16", 384): 4, ("bf16", 768): 4, ("bf16", 1024): 2}),
    "lists": Kind(
        "loss_and_grad_lists", "step_lists", "icrec_adapter_step_lists", "list_off", ref.loss_and_grad_lists,
        device_lists, lambda lists: lists, lambda ad, ix, B, middle: (ad, B),
        # by profiles/adapter_errors.md's rule from the ratios measured on the MI355X for THIS step (its table
        # "tests/test_adapter_lists_gpu.py"): the smallest of {2, 3, 4, 6, 8} that leaves 1.5x over the worst ratio
        {("f32", 32): 2, ("f32", 96): 2, ("f32", 384): 2, ("f32", 1024): 2, ("bf16", 64): 2, ("bf16", 384): 2,
         ("bf16", 768): 2}),
}


def as_targets(t) -> tuple:
    return t if isinstance(t, tuple) else (t,)


def workspace_bytes(kind: str, ad, ix, B: int, middle) -> int:
    k = KINDS[kind]
    return int(getattr(_native.lib(), k.entry + "_workspace_bytes")(*k.workspace_args(ad._h, ix._h, B, middle)))


@functools.lru_cache(maxsize=None)
def references(kind: str, inputs: Callable, name: str, scale: float):
    """(float64 loss, float64 gradient, float32 loss, float32 gradient) of the case `name` of a case module's inputs()
    by the kind's reference; computed once, read-only."""
    _, stored, anchors, delta, targets = inputs(name)
    want = KINDS[kind].reference(delta, anchors, stored, *as_targets(targets), scale, torch.float64)
    ref32 = KINDS[kind].reference(delta, anchors, stored, *as_targets(targets), scale, torch.float32)
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


def device_step(kind: str, ix, ad, anchors, targets, scale=30.0):
    """The kind's loss_and_grad on host arrays -> (loss float, gradient numpy)."""
    k = KINDS[kind]
    a_dev = torch.from_numpy(np.ascontiguousarray(anchors)).to(DEV)
    loss, grad = getattr(ad, k.loss_and_grad)(ix, a_dev, k.to_device(targets), scale)
    return float(loss.cpu()), grad.cpu().numpy()


def check_against_reference(kind: str, what: str, ix, ad, anchors, delta, stored, targets, storage: str, scale=30.0):
    """A device step on an index whose rows are `stored`, against references made here (an input no case table holds)."""
    k = KINDS[kind]
    want = k.reference(delta, anchors, stored, *as_targets(targets), scale, torch.float64)
    ref32 = k.reference(delta, anchors, stored, *as_targets(targets), scale, torch.float32)
    loss, grad = device_step(kind, ix, ad, anchors, targets, scale)
    check_step(what, loss, grad, *want, *ref32, k.margins[(storage.split("+")[0], delta.shape[0])])
    return loss, grad


# ---------------------------------------------------------------- one body per test the kinds have alike
def check_case(kind: str, cases, name: str, scale: float, before=None) -> None:
    """Loss and gradient of a case of the module `cases` (CASE_BY_NAME, inputs, references) within the kind's margin;
    loss_and_grad changes nothing.  before(adapter, case): what a kind checks beside."""
    c = cases.CASE_BY_NAME[name]
    P, _, anchors, delta, targets = cases.inputs(name)
    ix = DeviceIndex(P, DEV, storage=c.storage)
    ad = adapter_with(delta)
    try:
        if before is not None:
            before(ad, c)
        loss, grad = device_step(kind, ix, ad, anchors, targets, scale)
        what = f"adapter {kind} {c.storage} d{c.dim} B{c.B} scale {scale:g} {name}"
        check_step(what, loss, grad, *cases.references(name, scale), KINDS[kind].margins[(c.storage, c.dim)])
        assert ad.steps == 0 and np.array_equal(ad.state()["delta"], delta)
    finally:
        ad.close()
        ix.close()


def check_exact_zeros(kind: str, n_rows: int, n_anchors: int, batches, beside=None) -> None:
    """Every (what, B, targets as the kind's method takes them) of `batches` has loss 0 and a gradient of zeros, bit
    for bit.  beside(index, adapter, anchors): what a kind checks in the same world."""
    rng = np.random.default_rng(5)
    ix = DeviceIndex(unit_rows(rng, n_rows, 64), DEV, storage="f32")
    ad = adapter_with(small_delta(rng, 64))
    anchors = torch.from_numpy(unit_rows(rng, n_anchors, 64)).to(DEV)
    try:
        for what, B, targets in batches:
            loss, grad = getattr(ad, KINDS[kind].loss_and_grad)(ix, anchors[:B], targets)
            assert float(loss.cpu()) == 0.0 and not grad.cpu().numpy().any(), what
        if beside is not None:
            beside(ix, ad, anchors)
    finally:
        ad.close()
        ix.close()


DETERMINISM_VARIANTS = {kind: ("plain", "again", "no grad_out", "0xFF workspace") for kind in KINDS}


def check_determinism(kind: str, P, storage: str, anchors, targets, delta, m, v) -> None:
    """One step from (delta, m, v, t = 3), four times: as it is, again, without a grad_out, and on a workspace whose
    every byte is 0xFF (every float of it a NaN, every int -1) - the same loss, delta, m, v and gradient bit for bit."""
    k = KINDS[kind]
    d = delta.shape[0]
    ix = DeviceIndex(P, DEV, storage=storage)
    a_dev, t_dev = torch.from_numpy(anchors).to(DEV), k.to_device(targets)
    seen = {}
    try:
        for how in DETERMINISM_VARIANTS[kind]:
            ad = adapter_with(delta, m, v, 3)
            grad = None if how == "no grad_out" else torch.empty((d, d), dtype=torch.float32, device=DEV)
            if how == "0xFF workspace":
                ad._scratch.block(max(workspace_bytes(kind, ad, ix, anchors.shape[0], k.middle(t_dev)), 256)).fill_(0xFF)
            loss = getattr(ad, k.step)(ix, a_dev, t_dev, 1e-3, grad_out=grad)
            state = ad.state()
            seen[how] = (loss.cpu().numpy().tobytes(), state["delta"].tobytes(), state["m"].tobytes(), state["v"].tobytes(),
                         state["t"], None if grad is None else grad.cpu().numpy().tobytes())
            ad.close()
        plain = seen.pop("plain")
        assert plain[4] == 4 and np.frombuffer(plain[0], np.float32)[0] > 0 and np.frombuffer(plain[5], np.float32).any()
        for how, got in seen.items():
            assert got[:5] == plain[:5] and got[5] in (None, plain[5]), how
    finally:
        ix.close()


#: lr, beta1, beta2, eps, weight_decay as the float arguments the C ABI carries: the formula is given the values the call
#: carries (1 - 0.999 differs from 1 - float32(0.999) by 1.3e-5 of itself, far outside any rounding budget)
ADAMW_HYPER = tuple(float(np.float32(x)) for x in (1e-2, 0.9, 0.999, 1e-8, 0.01))


def check_adamw(kind: str, P, anchors, targets, delta, m, v):
    """A step from t = 7 on the kind's own gradient: loss_and_grad leaves the state untouched and returns what the step
    then returns, the update is torch's AdamW within assert_adamw's bounds, and apply reads the new D.  -> (state
    before, gradient, state after), for what a kind asserts beside."""
    k = KINDS[kind]
    d = delta.shape[0]
    ix = DeviceIndex(P, DEV, storage="f32")
    a_dev, t_dev = torch.from_numpy(anchors).to(DEV), k.to_device(targets)
    ad = adapter_with(delta, m, v, 7)
    try:
        want_loss, want_grad = getattr(ad, k.loss_and_grad)(ix, a_dev, t_dev)  # update = 0 leaves the state untouched
        before = ad.state()
        assert before["t"] == ad.steps == 7 and all(np.array_equal(before[n], a) for n, a in (("delta", delta), ("m", m), ("v", v)))
        grad = torch.empty((d, d), dtype=torch.float32, device=DEV)
        lr, b1, b2, eps, wd = ADAMW_HYPER
        loss = getattr(ad, k.step)(ix, a_dev, t_dev, lr, (b1, b2), eps, wd, grad_out=grad)
        assert torch.equal(grad, want_grad) and torch.equal(loss, want_loss)
        g = grad.cpu().numpy()
        assert np.abs(g).max() > 0
        after = ad.state()
        assert ad.steps == 8
        assert_adamw(before, g, after)
        few = a_dev[:5]  # the transposed copy followed: apply reads it (a handful of queries - the reference loops over c)
        assert np.array_equal(ad.apply(few).cpu().numpy(), ref.apply(after["delta"], few.cpu().numpy()))
        return before, g, after
    finally:
        ad.close()
        ix.close()


def check_shared_arguments(kind: str, ix, ad, anchors: torch.Tensor, targets) -> None:
    """What every step entry refuses alike, for 4 anchors of width 64 on the device and their host targets: an index of
    another width, hyper-parameters that are not finite, betas and eps out of range, each NULL pointer, B outside its
    limits, a workspace one byte short - and no refused call took a step."""
    k = KINDS[kind]
    t_dev = k.to_device(targets)
    with pytest.raises(_native.IcrecError, match="the index has dim 64, the adapter 32"):
        getattr(QueryAdapter(32, DEV), k.loss_and_grad)(ix, anchors[:, :32].contiguous(), t_dev)
    step = getattr(ad, k.step)
    for kw in (dict(lr=float("nan")), dict(lr=1e-3, scale=float("inf")), dict(lr=1e-3, weight_decay=float("nan")),
               dict(lr=1e-3, eps=float("inf"))):
        with pytest.raises(_native.IcrecError, match="not finite"):
            step(ix, anchors, t_dev, **kw)
    for kw in (dict(betas=(1.0, 0.999)), dict(eps=-1.0)):
        with pytest.raises(_native.IcrecError, match="beta1 and beta2"):
            step(ix, anchors, t_dev, 1e-3, **kw)
    L = _native.lib()
    middle = k.middle(t_dev)
    need = workspace_bytes(kind, ad, ix, 4, middle)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    loss = torch.empty(1, device=DEV)
    first, rest = _native.ptr(middle[0]), [_native.ptr(a) if isinstance(a, torch.Tensor) else a for a in middle[1:]]

    def call(idx=ix._h, adapter=ad._h, a=_native.ptr(anchors), B=4, p=first, out=_native.ptr(loss), w=_native.ptr(ws), n=need):
        return getattr(L, k.entry)(idx, adapter, a, B, p, *rest, 30.0, 0.0, 0.9, 0.999, 1e-8, 0.0, 0, out, None, w, n, None)

    assert call() == 0
    for kw, text in ((dict(idx=None), b"NULL idx"), (dict(adapter=None), b"NULL adapter"), (dict(a=None), b"NULL anchors"),
                     (dict(p=None), b"NULL anchors or " + k.list_name.encode()), (dict(out=None), b"NULL loss_out"),
                     (dict(w=None), b"NULL workspace"), (dict(B=0), b"B must be in"), (dict(B=1025), b"B must be in"),
                     (dict(n=need - 1), b"workspace")):  # .. a workspace one byte short
        assert call(**kw) == -1 and k.entry.encode() + b": " in L.icrec_last_error() and text in L.icrec_last_error(), kw
    assert ad.steps == 0  # no refused call took a step


def train_on_task(kind: str, task, batch_targets, measure=None):
    """The learning task's TASK_STEPS steps of the kind from D = 0 -> (index, adapter, held-out recall@10 through
    icrec_search afterwards, the per-step losses, measure(index, adapter) before and after); before, the recall is at
    most 0.05.  batch_targets(at): what the kind's step takes for the
    training pairs `at`.  The caller closes the adapter and the index."""
    P, a_train, _, a_held, p_held = task
    ix = DeviceIndex(P, DEV, storage="f32")
    ad = QueryAdapter(ref.TASK_DIM, DEV)
    held, a_dev = torch.from_numpy(a_held).to(DEV), torch.from_numpy(a_train).to(DEV)

    def recall():
        return ref.recall_at(ix.search(ad.apply(held), 10)[0].cpu().numpy(), p_held)

    before, measured = recall(), [measure(ix, ad)] if measure else []
    losses = torch.zeros(ref.TASK_STEPS, device=DEV)
    for step in range(ref.TASK_STEPS):
        at = ref.task_batch(step)
        getattr(ad, KINDS[kind].step)(ix, a_dev[at], batch_targets(at), ref.TASK_LR, weight_decay=ref.TASK_DECAY,
                                      scale=ref.TASK_SCALE, loss_out=losses[step:step + 1])
    after = recall()
    losses = losses.cpu().numpy()
    print(f"recall@10 {before:.4f} -> {after:.4f}, loss {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert before <= 0.05 and ad.steps == ref.TASK_STEPS and np.isfinite(losses).all()
    return ix, ad, after, losses, measured + ([measure(ix, ad)] if measure else [])


def check_fit_is_reproducible(fit, n_steps: int) -> None:
    """fit(a new adapter) -> its losses, twice: the same losses and the same D from the same seed, n_steps steps
    (drop_last), and the loss goes down."""
    runs = []
    for _ in range(2):
        fitted = QueryAdapter(ref.TASK_DIM, DEV)
        got = fit(fitted)
        runs.append((got, fitted.state()["delta"].tobytes()))
        assert len(got) == n_steps and fitted.steps == len(got)
        fitted.close()
    assert runs[0] == runs[1] and runs[0][0][-1] < runs[0][0][0]


def by_hand(rec, delta, query, top_k, exclude=()):
    """A recommender's request by hand: encode, the reference's apply on the host, DeviceIndex.search ->
    [(product id, score)]."""
    from tests.recommender_harness import as_results

    q = ref.apply(delta, rec.model.encode([query]))
    rows = sorted(rec._pid_to_row[p] for p in exclude or ())
    idx, sc = rec._index.search(torch.from_numpy(q).to(rec.device), top_k, [rows])
    return as_results(rec, idx[0].cpu().numpy(), sc[0].cpu().numpy())


# ---------------------------------------------------------------- AdamW
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
    (D under the bound below, m, v, D under the inline form of the bound, t).  The bound: eight roundings in the formula,
    each half an ulp of a magnitude bounded by the terms added - derived, not measured.  For m the terms added are
    |m| + (1 - beta1) |g - m|, for v beta2 |v| + (1 - beta2) g^2, for D |D| and the Adam term.  The Adam term is k m1,
    k = (lr / bc1) / (sqrt(v_hat) + eps), and m1 is rounded relative to the terms IT is added from, not to itself, so
    its magnitude here is k (|m| + (1 - beta1) |g - m|): the same value as the inline form's |term| (the pair step's
    first AdamW test held it at d = 96, and still does) wherever m and (g - m)(1 - beta1) have one sign (always at
    m = 0), larger only where they cancel - there |k m1| does not cover m1's own rounding (tests/test_adapter_cases.py:
    the formula in IEEE float32 on the host misses that form on some hundred of the 1,048,576 elements at d = 1024, and
    meets this one everywhere)."""
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
