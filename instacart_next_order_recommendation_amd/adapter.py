"""A query adapter learned from (context, product) pairs on the GPU (include/icrec.h, icrec_adapter_*).

The reference trains its bi-encoder with MultipleNegativesRankingLoss(scale=30) over (anchor, positive) pairs
(src/training/train_sbert.py).  Here the encoder and the stored product rows stay frozen and a linear map on the query
side, q' = q + D q, is trained with that loss against the rows the index already holds: no product is re-encoded, the
index keeps its bits, and every request option composes with it because only the query vector changes.
"""
from __future__ import annotations

import ctypes as C
import math
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native

DEFAULT_SCALE = 30.0  # the reference's loss_scale
ALL_NEGATIVES = "all"  # fit's negatives= for the whole catalog: every stored row is a candidate, none is drawn


def schedule(step: int, total: int, warmup: int) -> float:
    """The factor on the learning rate at 0-based `step` of `total`: linear warm-up over the first `warmup` steps, then
    a cosine to zero (the reference's warmup_steps = int(0.1 * total), lr_scheduler_type="cosine")."""
    if step < warmup:
        return step / max(1, warmup)
    progress = (step - warmup) / max(1, total - warmup)
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


def fit_plan(n_pairs: int, epochs, batch_size, negatives, lr, weight_decay, scale):
    """QueryAdapter.fit's sizes and hyper-parameters, checked before any GPU work -> (batch, steps per epoch, total steps,
    warm-up steps).  drop_last as the reference has it, unless there is less than one batch: then the pairs are one
    batch.  ValueError: no pair, epochs < 1, batch_size outside [1, ICREC_ADAPTER_MAX_BATCH], negatives neither "all"
    (every stored row, by catalog steps) nor an integer >= 0, batch_size + negatives above
    ICREC_ADAPTER_MAX_CANDIDATES, lr / weight_decay / scale not finite, lr or weight_decay
    negative."""
    def integer(v, what, lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{what} must be an integer in [{lo}, {hi}], got {v!r}")
        return int(v)

    def number(v, what, lo=None):
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float("nan")
        if not math.isfinite(f) or (lo is not None and f < lo):
            raise ValueError(f"{what} must be a finite number" + (f" >= {lo}" if lo is not None else "") + f", got {v!r}")
        return f

    if n_pairs < 1:
        raise ValueError("fit needs at least one (anchor, positive) pair")
    epochs = integer(epochs, "epochs", 1, 2**31 - 1)
    batch_size = integer(batch_size, "batch_size", 1, _native.ICREC_ADAPTER_MAX_BATCH)
    if not (isinstance(negatives, str) and negatives == ALL_NEGATIVES):  # "all": catalog steps, which have no list
        negatives = integer(negatives, "negatives", 0, _native.ICREC_ADAPTER_MAX_CANDIDATES)
    if not isinstance(negatives, str) and batch_size + negatives > _native.ICREC_ADAPTER_MAX_CANDIDATES:
        raise ValueError(f"batch_size + negatives = {batch_size + negatives} exceeds the limit "
                         f"{_native.ICREC_ADAPTER_MAX_CANDIDATES}")
    number(lr, "lr", 0.0)
    number(weight_decay, "weight_decay", 0.0)
    number(scale, "scale")
    batch = min(batch_size, n_pairs)
    per_epoch = n_pairs // batch
    total = epochs * per_epoch
    return batch, per_epoch, total, int(0.1 * total)


def impression_csr(lists, B: int, device: str | torch.device = "cpu"):
    """Per-anchor impression lists -> (off int32 [B + 1], rows int32 [n], target float32 [n], max_len) as tensors on
    `device`: icrec_adapter_step_lists' three arrays and the longest list (at least 1).  Each of the B lists is a
    mapping {row: gain} or a sequence of (row, gain); a row named twice in one list keeps the larger gain, at its first
    place.  A row beyond int32 becomes -1 (out of range for any index); gains are not judged here - the step drops an
    entry whose gain is negative or not finite.  ValueError: a string, not B lists, more than ICREC_ADAPTER_MAX_LIST
    entries in one list."""
    if isinstance(lists, (str, bytes)):
        raise ValueError("lists must be one list of (row, gain) per anchor, not a string")
    lists = list(lists)
    if len(lists) != int(B):
        raise ValueError(f"{int(B)} anchors for {len(lists)} lists")
    off, rows, target = [0], [], []
    for i, entries in enumerate(lists):
        if isinstance(entries, (str, bytes)):
            raise ValueError(f"list {i} must be a mapping row -> gain or a sequence of (row, gain), not a string")
        best: dict[int, float] = {}
        for row, gain in (entries.items() if hasattr(entries, "items") else entries):
            row, gain = int(row), float(gain)
            if row not in best or gain > best[row]:
                best[row] = gain
        if len(best) > _native.ICREC_ADAPTER_MAX_LIST:
            raise ValueError(f"list {i} has {len(best)} entries, the limit is {_native.ICREC_ADAPTER_MAX_LIST}")
        rows.extend(r if 0 <= r <= 2**31 - 1 else -1 for r in best)
        target.extend(best.values())
        off.append(len(rows))
    max_len = max(1, max((b - a for a, b in zip(off, off[1:])), default=1))
    return (torch.tensor(off, dtype=torch.int32, device=device), torch.tensor(rows, dtype=torch.int32, device=device),
            torch.tensor(target, dtype=torch.float32, device=device), max_len)


class _Batch(NamedTuple):
    """A step's anchors and targets, checked against each other by one of QueryAdapter's three builders: the C entry that
    takes them, its arguments between B and scale (a tensor goes as its pointer, kept alive here), its workspace's bytes."""
    name: str
    anchors: torch.Tensor
    args: tuple
    workspace: int


class QueryAdapter:
    """An icrec_adapter: D (fp32, dim x dim, zero when created), AdamW's moments and the step count, on one HIP device.
    The arrays never move, so a captured graph that holds apply_into stays valid while the adapter trains."""

    def __init__(self, dim: int, device: str | torch.device = "cuda:0"):
        self.device = _native.hip_device(device, "QueryAdapter")
        self.dim = int(dim)
        self.scale = DEFAULT_SCALE  # the scale of the loss it was trained with (fit; kept by save / load)
        self._h = C.c_void_p()
        _native.check(_native.lib().icrec_adapter_create(self.dim, self.device.index, C.byref(self._h)), "icrec_adapter_create")
        self._scratch = _native.StreamScratch(self.device)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.lib().icrec_adapter_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # -- apply ---------------------------------------------------------------------------------------
    def _rows(self, q: torch.Tensor, what: str) -> torch.Tensor:
        if not isinstance(q, torch.Tensor):
            q = torch.as_tensor(np.asarray(q, np.float32))
        q = q.to(self.device, torch.float32).contiguous()
        if q.ndim != 2 or q.shape[1] != self.dim or q.shape[0] < 1:
            raise ValueError(f"{what} must be float32 [n >= 1, {self.dim}], got {tuple(q.shape)}")
        return q

    def apply(self, q) -> torch.Tensor:
        """q' = q + D q for queries [n, dim] -> a new device tensor; bit-exact and the same alone or in any batch.  Not
        normalised: every search normalises its queries."""
        q = self._rows(q, "q")
        out = torch.empty_like(q)
        self.apply_into(q, out)
        return out

    def apply_into(self, q: torch.Tensor, out: torch.Tensor) -> None:
        """icrec_adapter_apply on device tensors float32 [n, dim], out not q: one launch on the current stream, no
        scratch - capturable."""
        _native.check(_native.lib().icrec_adapter_apply(self._h, _native.ptr(q), int(q.shape[0]), _native.ptr(out),
                                                        _native.stream_ptr(self.device)), "icrec_adapter_apply")

    # -- training ------------------------------------------------------------------------------------
    def _row_list(self, rows, what: str) -> torch.Tensor:
        """Row numbers as an int32 device list; a row beyond int32 is out of range for any index: -1, not its low 32 bits."""
        if not isinstance(rows, torch.Tensor):
            rows = torch.as_tensor(np.asarray(rows, np.int64))
        if rows.dtype != torch.int32:
            wide = rows.to(torch.int64)
            rows = torch.where((wide < 0) | (wide > 2**31 - 1), torch.full_like(wide, -1), wide)
        rows = rows.to(self.device, torch.int32).contiguous()
        if rows.ndim != 1:
            raise ValueError(f"{what} must be a list of rows, got shape {tuple(rows.shape)}")
        return rows

    def _pairs(self, anchors, cand_rows) -> _Batch:  # a candidate list, candidate i anchor i's positive
        anchors, rows = self._rows(anchors, "anchors"), self._row_list(cand_rows, "cand_rows")
        B, n = int(anchors.shape[0]), int(rows.shape[0])
        return _Batch("icrec_adapter_step", anchors, (rows, n), _native.lib().icrec_adapter_step_workspace_bytes(self._h, B, n))

    def _labels(self, index, anchors, positive_rows) -> _Batch:  # a positive per anchor; its C is the index's row count
        anchors, rows = self._rows(anchors, "anchors"), self._row_list(positive_rows, "positive_rows")
        if rows.shape[0] != anchors.shape[0]:
            raise ValueError(f"{anchors.shape[0]} anchors for {rows.shape[0]} positives")
        return _Batch("icrec_adapter_step_catalog", anchors, (rows,),
                      _native.lib().icrec_adapter_step_catalog_workspace_bytes(self._h, index._h, int(anchors.shape[0])))

    def _lists(self, anchors, csr) -> _Batch:  # _csr's four values
        anchors, (off, rows, target, max_len) = self._rows(anchors, "anchors"), csr
        if off.shape[0] != anchors.shape[0] + 1:
            raise ValueError(f"{anchors.shape[0]} anchors for {off.shape[0] - 1} lists")
        return _Batch("icrec_adapter_step_lists", anchors, (off, rows, target, int(max_len)),
                      _native.lib().icrec_adapter_step_lists_workspace_bytes(self._h, int(anchors.shape[0])))

    def _step(self, index, batch: _Batch, scale, lr=0.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
              update: bool = False, grad_out=None, loss_out=None, want_grad: bool = False):
        """One call of the batch's entry -> (loss float32 [], grad_out).  Without `update` the adapter is not changed;
        want_grad: a new grad_out."""
        ws = self._scratch.block(max(int(batch.workspace), 256))
        loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=self.device)
        if want_grad:
            grad_out = torch.empty((self.dim, self.dim), dtype=torch.float32, device=self.device)
        middle = (_native.ptr(a) if isinstance(a, torch.Tensor) else a for a in batch.args)
        _native.check(getattr(_native.lib(), batch.name)(
            index._h, self._h, _native.ptr(batch.anchors), int(batch.anchors.shape[0]), *middle, float(scale), float(lr),
            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), 1 if update else 0, _native.ptr(loss),
            _native.ptr(grad_out), _native.ptr(ws), ws.numel(), _native.stream_ptr(self.device)), batch.name)
        return loss[0], grad_out

    def _held_out_loss(self, index, batch_of, counted: torch.Tensor, scale) -> float:
        """catalog_loss and lists_loss: batch_of(lo, hi) is the batch of anchors [lo, hi); counted, float64 [n] on the
        device, is 1 where the step counts the anchor."""
        scale = self.scale if scale is None else float(scale)
        n, step = int(counted.shape[0]), _native.ICREC_ADAPTER_MAX_BATCH
        starts = range(0, n, step)
        means = torch.zeros(len(starts), dtype=torch.float32, device=self.device)
        for k, lo in enumerate(starts):
            self._step(index, batch_of(lo, min(lo + step, n)), scale, loss_out=means[k:k + 1])
        per_batch = torch.stack([counted[lo:lo + step].sum() for lo in starts])
        host = torch.stack([means.to(torch.float64), per_batch]).cpu().numpy()  # the one read-back
        total = float(host[1].sum())
        return float((host[0] * host[1]).sum() / total) if total > 0 else 0.0

    def _train(self, index, n: int, batch_of, plan, epochs, lr, weight_decay, scale, seed) -> list[float]:
        """fit's and fit_lists' loop over fit_plan's `plan`; batch_of(at, gen) is the batch of the n examples' subset
        `at` (device indices) and may draw from gen, the seeded CPU generator, after the epoch's shuffle."""
        batch, per_epoch, total, warmup = plan
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        losses = torch.zeros(total, dtype=torch.float32, device=self.device)
        s = 0
        for _ in range(int(epochs)):
            perm = torch.randperm(n, generator=gen)
            for b in range(per_epoch):
                at = perm[b * batch:(b + 1) * batch].to(self.device)
                self._step(index, batch_of(at, gen), scale, float(lr) * schedule(s, total, warmup),
                           weight_decay=weight_decay, update=True, loss_out=losses[s:s + 1])
                s += 1
        self.scale = float(scale)
        return losses.cpu().tolist()

    # -- pairs and the whole catalog -----------------------------------------------------------------
    def loss_and_grad(self, index, anchors, cand_rows, scale: float = DEFAULT_SCALE):
        """(loss float32 [], dD float32 [dim, dim]) on the device, of the anchors [B, dim] against index's stored rows
        cand_rows [C >= B] (candidate i is anchor i's positive); the adapter is not changed."""
        return self._step(index, self._pairs(anchors, cand_rows), scale, want_grad=True)

    def step(self, index, anchors, cand_rows, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01,
             scale: float = DEFAULT_SCALE, grad_out: Optional[torch.Tensor] = None, loss_out: Optional[torch.Tensor] = None):
        """One AdamW step (torch.optim.AdamW's formula) on the batch's gradient -> the batch's loss before the step, a
        float32 [] device tensor (loss_out: a float32 [1] device tensor to write it to).  No host synchronisation."""
        return self._step(index, self._pairs(anchors, cand_rows), scale, lr, betas, eps, weight_decay, True, grad_out, loss_out)[0]

    def loss_and_grad_catalog(self, index, anchors, positive_rows, scale: float = DEFAULT_SCALE):
        """loss_and_grad against the WHOLE catalog: the cross-entropy of anchors [B, dim] over every stored row of index,
        positive_rows [B] the labels (an anchor whose row is outside the index is not counted); no candidate list, no
        sampling.  The adapter is not changed."""
        return self._step(index, self._labels(index, anchors, positive_rows), scale, want_grad=True)

    def step_catalog(self, index, anchors, positive_rows, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                     weight_decay: float = 0.01, scale: float = DEFAULT_SCALE, grad_out: Optional[torch.Tensor] = None,
                     loss_out: Optional[torch.Tensor] = None):
        """step against the whole catalog (loss_and_grad_catalog's loss): one AdamW step -> the batch's loss before the
        step, a float32 [] device tensor.  No host synchronisation."""
        return self._step(index, self._labels(index, anchors, positive_rows), scale, lr, betas, eps, weight_decay, True,
                          grad_out, loss_out)[0]

    def catalog_loss(self, index, anchors, positive_rows, scale: Optional[float] = None) -> float:
        """The exact loss of a held-out set: the mean over its counted pairs of the cross-entropy against every stored
        row.  Batches of at most ICREC_ADAPTER_MAX_BATCH; the batch means are combined, weighted by their counted
        anchors, in double on the host, which is read back once.  scale=None: the adapter's own scale."""
        _, anchors, (pos,), _ = self._labels(index, anchors, positive_rows)  # the whole set, checked as a batch is
        in_range = ((pos >= 0) & (pos < int(index.n_rows))).to(torch.float64)
        return self._held_out_loss(index, lambda lo, hi: self._labels(index, anchors[lo:hi], pos[lo:hi]), in_range, scale)

    def fit(self, index, anchor_embeddings, positive_rows, epochs: int = 5, batch_size: int = 64, negatives=0,
            lr: float = 2e-3, weight_decay: float = 0.01, scale: float = DEFAULT_SCALE, seed: int = 0) -> list[float]:
        """Train on pairs (anchor_embeddings[i], the stored row positive_rows[i]) -> the per-step losses.  Each epoch
        walks a fresh shuffle in batches of batch_size with in-batch negatives plus `negatives` rows drawn from the
        whole index; the shuffles and draws come from a CPU torch.Generator seeded with `seed`, so a run is
        reproducible.  negatives="all": every step is a step_catalog - the exact cross-entropy against every stored
        row, nothing drawn beside the shuffles.  As the reference trains: warm-up over the first 10 % of the steps, then
        a cosine schedule; drop_last (unless there is less than one batch); scale 30.  One read-back, at the end."""
        rows = torch.as_tensor(np.asarray(positive_rows, np.int64))
        if rows.ndim != 1:
            raise ValueError("positive_rows must be a list of rows")
        plan = fit_plan(int(rows.shape[0]), epochs, batch_size, negatives, lr, weight_decay, scale)
        anchors = self._rows(anchor_embeddings, "anchor_embeddings")
        if anchors.shape[0] != rows.shape[0]:
            raise ValueError(f"{anchors.shape[0]} anchors for {rows.shape[0]} positives")
        exact = isinstance(negatives, str)  # fit_plan admitted "all" only
        rows_dev = rows.to(self.device, torch.int32)

        def batch_of(at, gen):
            cand = rows_dev[at]  # the batch's positives: a catalog step's labels, the head of a list step's candidates
            if exact:
                return self._labels(index, anchors[at], cand)
            if negatives:
                extra = torch.randint(0, index.n_rows, (int(negatives),), generator=gen, dtype=torch.int64)
                cand = torch.cat([cand, extra.to(self.device, torch.int32)])
            return self._pairs(anchors[at], cand)

        return self._train(index, int(rows.shape[0]), batch_of, plan, epochs, lr, weight_decay, scale, seed)

    # -- per-anchor lists ----------------------------------------------------------------------------
    def _csr(self, lists, B: int):
        """lists as the step takes them: impression_csr's values on this device, from per-anchor lists or from an
        (off, rows, target, max_len) already made (tensors of any device; kept alive by the caller's tuple)."""
        if isinstance(lists, tuple) and len(lists) == 4 and isinstance(lists[0], torch.Tensor):
            off, rows, target, max_len = lists
        else:
            off, rows, target, max_len = impression_csr(lists, B, self.device)
        off = off.to(self.device, torch.int32).contiguous()
        rows = rows.to(self.device, torch.int32).contiguous()
        target = target.to(self.device, torch.float32).contiguous()
        if off.ndim != 1 or rows.ndim != 1 or target.shape != rows.shape:
            raise ValueError("lists: off, rows and target must be flat, rows and target of one length")
        if rows.numel() == 0:  # nothing listed at all: one dropped entry, so that the arrays exist
            rows, target = rows.new_full((1,), -1), target.new_zeros(1)
            off = torch.zeros_like(off)
        return off, rows, target, int(max_len)

    def loss_and_grad_lists(self, index, anchors, lists, scale: float = DEFAULT_SCALE):
        """(loss float32 [], dD float32 [dim, dim]) of the listwise softmax cross-entropy (include/icrec.h,
        icrec_adapter_step_lists): anchor i against its own list of (stored row of index, gain >= 0) - per anchor a
        mapping or a sequence of pairs, or impression_csr's tuple.  The adapter is not changed."""
        return self._step(index, self._lists(anchors, self._csr(lists, int(np.shape(anchors)[0]))), scale, want_grad=True)

    def step_lists(self, index, anchors, lists, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01,
                   scale: float = DEFAULT_SCALE, grad_out: Optional[torch.Tensor] = None,
                   loss_out: Optional[torch.Tensor] = None):
        """step on loss_and_grad_lists' loss: one AdamW step -> the batch's loss before the step, a float32 [] device
        tensor.  No host synchronisation when `lists` is impression_csr's tuple on this device."""
        batch = self._lists(anchors, self._csr(lists, int(np.shape(anchors)[0])))
        return self._step(index, batch, scale, lr, betas, eps, weight_decay, True, grad_out, loss_out)[0]

    @staticmethod
    def _padded(csr, n_rows: int):
        """A CSR's entries read as [B, max_len] device matrices (rows, targets; -1 / 0 behind a segment's end) and the
        anchors the step counts: T_i, the sum of the live targets, finite and > 0."""
        off, rows, target, max_len = csr
        lo = off[:-1].to(torch.int64)
        length = (off[1:].to(torch.int64) - lo).clamp(0, max_len)
        at = torch.arange(max_len, device=off.device)[None, :]
        inside = at < length[:, None]
        idx = torch.where(inside, lo[:, None] + at, torch.zeros_like(at))
        r = torch.where(inside, rows[idx], torch.full_like(rows[idx], -1))
        t = torch.where(inside, target[idx], torch.zeros_like(target[idx]))
        live = (r >= 0) & (r < int(n_rows)) & torch.isfinite(t) & (t >= 0)
        T = torch.where(live, t, torch.zeros_like(t)).sum(dim=1)
        return r, t, torch.isfinite(T) & (T > 0)

    def _all_lists(self, anchors, what: str, lists):  # a whole set, checked as a batch is: _rows' anchors, _csr's lists
        anchors = self._rows(anchors, what)
        return anchors, self._lists(anchors, self._csr(lists, int(anchors.shape[0]))).args

    def lists_loss(self, index, anchors, lists, scale: Optional[float] = None) -> float:
        """The listwise loss of a held-out set: the mean over its counted anchors.  Batches of at most
        ICREC_ADAPTER_MAX_BATCH; the batch means are combined, weighted by their counted anchors, in double on the
        host, which is read back once.  scale=None: the adapter's own scale."""
        anchors, csr = self._all_lists(anchors, "anchors", lists)
        off, rows, target, max_len = csr
        return self._held_out_loss(
            index, lambda lo, hi: self._lists(anchors[lo:hi], (off[lo:hi + 1].contiguous(), rows, target, max_len)),
            self._padded(csr, index.n_rows)[2].to(torch.float64), scale)

    def fit_lists(self, index, anchor_embeddings, lists, epochs: int = 5, batch_size: int = 64, lr: float = 2e-3,
                  weight_decay: float = 0.01, scale: float = DEFAULT_SCALE, seed: int = 0) -> list[float]:
        """Train on (anchor_embeddings[i], lists[i]) with step_lists -> the per-step losses.  fit's shuffles (a CPU
        torch.Generator seeded with `seed`), warm-up, cosine schedule, drop_last and single read-back; nothing is drawn
        beside the shuffles: an anchor's negatives are the entries of its own list."""
        anchors, csr = self._all_lists(anchor_embeddings, "anchor_embeddings", lists)
        plan = fit_plan(int(anchors.shape[0]), epochs, batch_size, 0, lr, weight_decay, scale)
        max_len = csr[3]
        rows_pad, target_pad, _ = self._padded(csr, index.n_rows)  # a batch is a gather of whole padded lists
        off = torch.arange(plan[0] + 1, dtype=torch.int32, device=self.device) * max_len
        return self._train(index, int(anchors.shape[0]), lambda at, gen: self._lists(
            anchors[at], (off, rows_pad[at].reshape(-1), target_pad[at].reshape(-1), max_len)),
            plan, epochs, lr, weight_decay, scale, seed)

    # -- state ---------------------------------------------------------------------------------------
    @property
    def steps(self) -> int:
        """AdamW steps taken."""
        t = C.c_int64(0)
        _native.check(_native.lib().icrec_adapter_get_state(self._h, None, None, None, C.byref(t)), "icrec_adapter_get_state")
        return int(t.value)

    def state(self) -> dict:
        """{"delta", "m", "v": float32 [dim, dim] host arrays, "t": steps taken}."""
        arrays = {name: np.empty((self.dim, self.dim), np.float32) for name in ("delta", "m", "v")}
        t = C.c_int64(0)
        _native.check(_native.lib().icrec_adapter_get_state(self._h, *(C.c_void_p(a.ctypes.data) for a in arrays.values()),
                                                            C.byref(t)), "icrec_adapter_get_state")
        return {**arrays, "t": int(t.value)}

    def load_state(self, state: dict) -> None:
        """state()'s dictionary back onto the device; "m" and "v" may be missing or None (zeros), "t" defaults to 0."""
        arrays = []
        for name in ("delta", "m", "v"):
            a = state.get(name)
            if a is None:
                if name == "delta":
                    raise ValueError("load_state needs 'delta'")
                arrays.append(None)
                continue
            a = np.ascontiguousarray(np.asarray(a, np.float32))
            if a.shape != (self.dim, self.dim):
                raise ValueError(f"{name} must be [{self.dim}, {self.dim}], got {a.shape}")
            if not np.isfinite(a).all():
                raise ValueError(f"{name} holds values that are not finite")
            arrays.append(a)
        _native.check(_native.lib().icrec_adapter_set_state(
            self._h, *(C.c_void_p(a.ctypes.data if a is not None else 0) for a in arrays), int(state.get("t", 0) or 0)),
            "icrec_adapter_set_state")

    def save(self, path) -> None:
        """An .npz of D, dim, scale and the number of steps (not the moments: a saved adapter is for serving)."""
        write_adapter_file(path, self.state()["delta"], self.scale, self.steps)

    @classmethod
    def load(cls, path, device: str | torch.device = "cuda:0") -> "QueryAdapter":
        delta, scale, steps = read_adapter_file(path)
        adapter = cls(delta.shape[0], device)
        adapter.load_state({"delta": delta, "t": steps})
        adapter.scale = scale
        return adapter


def write_adapter_file(path, delta: np.ndarray, scale: float, steps: int) -> None:
    """The adapter file: an .npz of delta float32 [dim, dim], dim, scale, steps - written to exactly `path`."""
    delta = np.ascontiguousarray(np.asarray(delta, np.float32))
    if delta.ndim != 2 or delta.shape[0] != delta.shape[1]:
        raise ValueError(f"delta must be square, got {delta.shape}")
    with open(Path(path), "wb") as f:
        np.savez(f, delta=delta, dim=np.int64(delta.shape[0]), scale=np.float64(scale), steps=np.int64(steps))


def read_adapter_file(path) -> tuple[np.ndarray, float, int]:
    """-> (delta float32 [dim, dim], scale, steps) of an adapter file.  ValueError: a file without these arrays, a delta
    that is not [dim, dim] or not finite."""
    with np.load(Path(path)) as z:  # allow_pickle stays False
        missing = [name for name in ("delta", "dim", "scale", "steps") if name not in z.files]
        if missing:
            raise ValueError(f"{path}: not an adapter file (no {missing[0]!r})")
        delta, dim, scale, steps = np.asarray(z["delta"], np.float32), int(z["dim"]), float(z["scale"]), int(z["steps"])
    if delta.shape != (dim, dim) or not np.isfinite(delta).all():
        raise ValueError(f"{path}: delta must be a finite [{dim}, {dim}] matrix, got {delta.shape}")
    return delta, scale, steps
