"""The query adapter (include/icrec.h, icrec_adapter_*) restated without a GPU: apply in numpy float32 with the two
roundings per term; the three steps' losses - over a candidate list, over the whole catalog, over per-anchor lists - and
their gradients from the math in torch with autograd (the same code in float64, the truth, and in float32, E_ref); AdamW
in float64; and the learning task, with pairs and with lists, that the CPU and the GPU tests share.  Importing this needs
no GPU."""
from __future__ import annotations

import numpy as np
import torch

from tests.mmr_reference import stored_rows  # noqa: F401  (re-exported: the rows an index holds for a host matrix)


def apply(delta: np.ndarray, q: np.ndarray) -> np.ndarray:
    """q'[n][r] = q[n][r] + acc, acc the chain over c ascending of acc = acc + (delta[r][c] * q[n][c]): every product
    and every sum one float32 rounding."""
    delta = np.asarray(delta, np.float32)
    q = np.asarray(q, np.float32)
    acc = np.zeros(q.shape, np.float32)
    for c in range(delta.shape[1]):
        acc = acc + (delta[None, :, c] * q[:, c, None]).astype(np.float32)  # float32 throughout: numpy rounds each operation
    return q + acc


def masks(cand: np.ndarray, B: int, n_rows: int):
    """(valid bool [C], masked bool [B, C], counted bool [B]) of a candidate list under the masking rules."""
    cand = np.asarray(cand, np.int64)
    C = cand.shape[0]
    valid = (cand >= 0) & (cand < n_rows)
    copy_of_positive = (cand[None, :] == cand[:B, None]) & (np.arange(C)[None, :] != np.arange(B)[:, None])
    return valid, ~valid[None, :] | copy_of_positive, valid[:B]


def unit_queries(D: torch.Tensor, anchors, dtype) -> torch.Tensor:
    """u = z / max(|z|, 1e-12), z = A + A D^T: the adapted anchors, normalised as every search normalises its queries."""
    A = torch.tensor(np.asarray(anchors), dtype=dtype)
    z = A + A @ D.T
    return z / z.norm(dim=1, keepdim=True).clamp_min(1e-12)


def differentiated(delta, dtype, n_counted: int, loss_of):
    """(loss, d loss / d delta [d, d]) as numpy values of `dtype`'s precision, of loss_of(D), a torch scalar, by
    autograd; nobody counted: (0, zeros), and loss_of is not called."""
    D = torch.tensor(np.asarray(delta), dtype=dtype, requires_grad=True)
    if not n_counted:
        return 0.0, np.zeros(D.shape, np.float64)
    loss = loss_of(D)
    loss.backward()
    return float(loss.detach()), D.grad.numpy().astype(np.float64)


def loss_and_grad(delta, anchors, rows, cand, scale, dtype=torch.float64):
    """icrec_adapter_step's loss of include/icrec.h over the stored rows `rows` (stored_rows(P, storage)) and its
    gradient (differentiated)."""
    cand = np.asarray(cand, np.int64)
    valid, masked, counted = masks(cand, np.shape(anchors)[0], rows.shape[0])

    def loss_of(D):
        u = unit_queries(D, anchors, dtype)
        V = torch.tensor(np.asarray(rows)[np.where(valid, cand, 0)], dtype=dtype)
        s = float(scale) * (u @ V.T)
        who = torch.tensor(np.flatnonzero(counted))
        s_own = s[who, who]
        s_c = s[who].masked_fill(torch.tensor(masked[np.flatnonzero(counted)]), float("-inf"))
        return (torch.logsumexp(s_c, dim=1) - s_own).sum() / int(counted.sum())

    return differentiated(delta, dtype, int(counted.sum()), loss_of)


# ---------------------------------------------------------------- the whole catalog
def counted_labels(pos, n_rows: int) -> np.ndarray:
    """bool [B]: the anchors whose positive lies in [0, n_rows)."""
    pos = np.asarray(pos, np.int64)
    return (pos >= 0) & (pos < n_rows)


def loss_and_grad_catalog(delta, anchors, rows, pos, scale, dtype=torch.float64):
    """icrec_adapter_step_catalog's loss and its gradient (differentiated): cross_entropy(scale * u @ V.T, pos) of anchors
    [B, d] against EVERY row of `rows` (stored_rows(P, storage)), pos [B] the labels.  An anchor whose label is outside
    the rows is not counted.  Nothing is masked."""
    pos = np.asarray(pos, np.int64)
    who = np.flatnonzero(counted_labels(pos, rows.shape[0]))

    def loss_of(D):
        u = unit_queries(D, anchors, dtype)
        V = torch.tensor(np.asarray(rows), dtype=dtype)
        s = float(scale) * (u[torch.tensor(who)] @ V.T)
        return torch.nn.functional.cross_entropy(s, torch.tensor(pos[who]), reduction="mean")

    return differentiated(delta, dtype, who.size, loss_of)


def mean_loss_catalog(delta, anchors, rows, pos, scale) -> float:
    """The float64 loss of a set of any size: catalog_loss's truth."""
    return loss_and_grad_catalog(delta, anchors, rows, pos, scale, torch.float64)[0]


# ---------------------------------------------------------------- per-anchor lists
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


def masks_lists(off, rows, target, max_len: int, n_rows: int):
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
    r, t, _, live, counted = masks_lists(off, rows, target, max_len, stored.shape[0])
    who = np.flatnonzero(counted)
    if D is None:
        D = torch.tensor(np.asarray(delta), dtype=dtype)
    if who.size == 0:
        return torch.zeros(0, dtype=dtype), counted
    u = unit_queries(D, np.asarray(anchors)[who], dtype)
    live_t = torch.tensor(live[who])
    V = torch.tensor(np.asarray(stored)[np.where(live[who], r[who], 0)], dtype=dtype)  # [counted, L, d]
    s = float(scale) * torch.einsum("bd,bld->bl", u, V)
    tt = torch.tensor(np.where(live[who], t[who], 0), dtype=dtype)
    tt = tt / tt.sum(dim=1, keepdim=True)
    lse = torch.logsumexp(s.masked_fill(~live_t, float("-inf")), dim=1)
    return lse - (tt * torch.where(live_t, s, torch.zeros_like(s))).sum(dim=1), counted


def loss_and_grad_lists(delta, anchors, stored, off, rows, target, max_len, scale, dtype=torch.float64):
    """icrec_adapter_step_lists' loss and its gradient (differentiated): the mean over the counted anchors of
    logsumexp_e s_e - sum_e t_e s_e over the live entries."""
    n_counted = int(masks_lists(off, rows, target, max_len, stored.shape[0])[4].sum())
    return differentiated(delta, dtype, n_counted, lambda D: per_anchor_losses(
        delta, anchors, stored, off, rows, target, max_len, scale, dtype, D)[0].sum() / n_counted)


def uniform_csr(row_matrix, target_matrix):
    """[B, L] matrices as a CSR without gaps -> (off int64 [B + 1], rows int64, target float32, max_len = L)."""
    row_matrix, target_matrix = np.asarray(row_matrix, np.int64), np.asarray(target_matrix, np.float32)
    B, L = row_matrix.shape
    return np.arange(B + 1, dtype=np.int64) * L, row_matrix.reshape(-1), target_matrix.reshape(-1), L


def adamw(delta, m, v, t, grad, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01):
    """torch.optim.AdamW's step t + 1 in float64 -> (delta, m, v, t + 1, the Adam term lr * m_hat / (sqrt(v_hat) + eps))."""
    delta, m, v, grad = (np.asarray(a, np.float64) for a in (delta, m, v, grad))
    t = t + 1
    delta = delta * (1.0 - lr * weight_decay)
    m = m + (grad - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * grad * grad
    term = (lr / (1.0 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
    return delta - term, m, v, t, term


# ---------------------------------------------------------------- the learning task
TASK_DIM, TASK_ROWS, TASK_TRAIN, TASK_HELD_OUT = 64, 2048, 4096, 1024
TASK_BATCH, TASK_STEPS, TASK_LR, TASK_DECAY, TASK_SCALE = 256, 100, 5e-3, 0.01, 30.0


def learning_task(seed: int = 11):
    """2,048 unit rows of width 64, a random orthogonal R, 4,096 training and 1,024 held-out pairs whose anchor is
    normalise(v_pos R + (0.5 / sqrt(d)) noise): before training the anchors point nowhere near their positives, and a
    linear map on the query side can undo R.  -> (P float32 [rows, d], train anchors, train positives, held-out anchors,
    held-out positives)."""
    rng = np.random.default_rng(seed)
    d = TASK_DIM
    P = rng.standard_normal((TASK_ROWS, d))
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    R = np.linalg.qr(rng.standard_normal((d, d)))[0]

    def pairs(n):
        pos = rng.integers(0, TASK_ROWS, n)
        a = P[pos] @ R + (0.5 / np.sqrt(d)) * rng.standard_normal((n, d))
        return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32), pos.astype(np.int64)

    train, held = pairs(TASK_TRAIN), pairs(TASK_HELD_OUT)
    return P.astype(np.float32), train[0], train[1], held[0], held[1]


def task_batch(step: int) -> slice:
    """The training pairs of step `step`: consecutive batches of TASK_BATCH, wrapping around."""
    lo = (step * TASK_BATCH) % TASK_TRAIN
    return slice(lo, lo + TASK_BATCH)


def recall_at(found_rows: np.ndarray, positives: np.ndarray) -> float:
    """The share of queries whose positive is among their found rows [n, k]."""
    return float((np.asarray(found_rows) == np.asarray(positives)[:, None]).any(axis=1).mean())


def top_rows(queries: np.ndarray, rows: np.ndarray, k: int) -> np.ndarray:
    """The k best rows of every query by cosine, on the host."""
    q = np.asarray(queries, np.float64)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    return np.argsort(-(q @ np.asarray(rows, np.float64).T), axis=1, kind="stable")[:, :k]


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
        loss, g = loss_and_grad_lists(D, anchors[at], stored, *uniform_csr(rows[at], gains[at]), TASK_SCALE)
        D, m, v, t, _ = adamw(D, m, v, t, g, TASK_LR, weight_decay=TASK_DECAY)
        losses.append(loss)
    return D, losses
