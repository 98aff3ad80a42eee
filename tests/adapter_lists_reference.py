"""The adapter's step over per-anchor lists (include/icrec.h, icrec_adapter_step_lists) restated without a GPU: which
entries are read, live and counted in numpy, the listwise softmax cross-entropy and its gradient from the math in torch
with autograd (the same code in float64 and in float32), and the learning task's lists and training loop that the CPU
and the GPU test share.  Importing this needs no GPU."""
from __future__ import annotations

import numpy as np
import torch

from tests.adapter_reference import (TASK_BATCH, TASK_DECAY, TASK_LR, TASK_SCALE, TASK_STEPS, adamw, learning_task,  # noqa: F401
                                     recall_at, stored_rows, task_batch, top_rows)


def padded(off, rows, target, max_len: int):
    """The entries READ, as [B, L] matrices (L the longest head): anchor i's segment is [off[i], off[i+1]), empty when
    its end lies before its start, and only its first max_len entries are read.  -> (row int64, target float32,
    read bool)."""
    off, rows, target = np.asarray(off, np.int64), np.asarray(rows, np.int64), np.asarray(target, np.float32)
    length = np.clip(off[1:] - off[:-1], 0, int(max_len))
    L = max(1, int(length.max(initial=0)))
    at = np.arange(L)[None, :]
    read = at < length[:, None]
    idx = np.where(read, off[:-1, None] + at, 0)
    return np.where(read, rows[idx], -1), np.where(read, target[idx], np.float32(0)), read


def masks(off, rows, target, max_len: int, n_rows: int):
    """(row [B, L], target [B, L], read, live bool [B, L], counted bool [B]): an entry is live when its row lies in
    [0, n_rows) and its target is finite and >= 0; an anchor is counted iff the sum of its live targets is finite and
    > 0."""
    r, t, read = padded(off, rows, target, max_len)
    with np.errstate(invalid="ignore"):
        live = read & (r >= 0) & (r < n_rows) & np.isfinite(t) & (t >= 0)
    T = np.where(live, t, 0).astype(np.float64).sum(axis=1)
    return r, t, read, live, np.isfinite(T) & (T > 0)


def per_anchor_losses(delta, anchors, stored, off, rows, target, max_len, scale, dtype=torch.float64, D=None):
    """(loss_i of the counted anchors as a torch vector of `dtype`, counted bool [B]); D: a tensor to differentiate by."""
    r, t, _, live, counted = masks(off, rows, target, max_len, stored.shape[0])
    who = np.flatnonzero(counted)
    if D is None:
        D = torch.tensor(np.asarray(delta), dtype=dtype)
    if who.size == 0:
        return torch.zeros(0, dtype=dtype), counted
    A = torch.tensor(np.asarray(anchors)[who], dtype=dtype)
    z = A + A @ D.T
    u = z / z.norm(dim=1, keepdim=True).clamp_min(1e-12)
    live_t = torch.tensor(live[who])
    V = torch.tensor(np.asarray(stored)[np.where(live[who], r[who], 0)], dtype=dtype)  # [counted, L, d]
    s = float(scale) * torch.einsum("bd,bld->bl", u, V)
    tt = torch.tensor(np.where(live[who], t[who], 0), dtype=dtype)
    tt = tt / tt.sum(dim=1, keepdim=True)
    lse = torch.logsumexp(s.masked_fill(~live_t, float("-inf")), dim=1)
    return lse - (tt * torch.where(live_t, s, torch.zeros_like(s))).sum(dim=1), counted


def loss_and_grad(delta, anchors, stored, off, rows, target, max_len, scale, dtype=torch.float64):
    """(loss, d loss / d delta [d, d]) as numpy values of `dtype`'s precision: the mean over the counted anchors of
    logsumexp_e s_e - sum_e t_e s_e over the live entries, differentiated by autograd; (0, zeros) when nobody is counted."""
    D = torch.tensor(np.asarray(delta), dtype=dtype, requires_grad=True)
    losses, counted = per_anchor_losses(delta, anchors, stored, off, rows, target, max_len, scale, dtype, D)
    if not counted.any():
        return 0.0, np.zeros(D.shape, np.float64)
    loss = losses.sum() / int(counted.sum())
    loss.backward()
    return float(loss.detach()), D.grad.numpy().astype(np.float64)


def uniform_csr(row_matrix, target_matrix):
    """[B, L] matrices as a CSR without gaps -> (off int64 [B + 1], rows int64, target float32, max_len = L)."""
    row_matrix, target_matrix = np.asarray(row_matrix, np.int64), np.asarray(target_matrix, np.float32)
    B, L = row_matrix.shape
    return np.arange(B + 1, dtype=np.int64) * L, row_matrix.reshape(-1), target_matrix.reshape(-1), L


# ---------------------------------------------------------------- the learning task with lists
TASK_LIST = 128


def task_lists(P, positives, rng):
    """Each pair's list: its positive at gain 4, the positive's two nearest rows at gain 1, and 125 random rows at
    gain 0 -> (rows int64 [n, 128], gains float32 [n, 128])."""
    P64 = np.asarray(P, np.float64)
    sims = P64 @ P64.T
    np.fill_diagonal(sims, -np.inf)
    near = np.argsort(-sims, axis=1, kind="stable")[:, :2]
    n = len(positives)
    rows = np.concatenate([np.asarray(positives)[:, None], near[positives], rng.integers(0, P.shape[0], (n, TASK_LIST - 3))], axis=1)
    gains = np.zeros((n, TASK_LIST), np.float32)
    gains[:, 0], gains[:, 1:3] = 4.0, 1.0
    return rows.astype(np.int64), gains


def train_reference(P, anchors, rows, gains, steps=TASK_STEPS):
    """The task's loop in float64 on the CPU: `steps` AdamW steps of TASK_BATCH at TASK_LR from D = 0 ->
    (D float64, the per-step losses)."""
    d = P.shape[1]
    stored = stored_rows(P, "f32")
    D, m, v, t = np.zeros((d, d)), np.zeros((d, d)), np.zeros((d, d)), 0
    losses = []
    for step in range(steps):
        at = task_batch(step)
        loss, g = loss_and_grad(D, anchors[at], stored, *uniform_csr(rows[at], gains[at]), TASK_SCALE)
        D, m, v, t, _ = adamw(D, m, v, t, g, TASK_LR, weight_decay=TASK_DECAY)
        losses.append(loss)
    return D, losses
