"""The query adapter (include/icrec.h, icrec_adapter_*) restated without a GPU: apply in numpy float32 with the two
roundings per term, the loss and its gradient from the math in torch with autograd (the same code in float64 and in
float32), AdamW in float64, and the learning task the CPU and the GPU test share.  Importing this needs no GPU."""
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


def loss_and_grad(delta, anchors, rows, cand, scale, dtype=torch.float64):
    """(loss, d loss / d delta [d, d]) as numpy values of `dtype`'s precision: the loss of include/icrec.h over the
    stored rows `rows` (stored_rows(P, storage)), differentiated by autograd."""
    D = torch.tensor(np.asarray(delta), dtype=dtype, requires_grad=True)
    A = torch.tensor(np.asarray(anchors), dtype=dtype)
    B = A.shape[0]
    cand = np.asarray(cand, np.int64)
    valid, masked, counted = masks(cand, B, rows.shape[0])
    if not counted.any():
        return 0.0, np.zeros(D.shape, np.float64)
    z = A + A @ D.T
    u = z / z.norm(dim=1, keepdim=True).clamp_min(1e-12)
    V = torch.tensor(np.asarray(rows)[np.where(valid, cand, 0)], dtype=dtype)
    s = float(scale) * (u @ V.T)
    who = torch.tensor(np.flatnonzero(counted))
    s_own = s[who, who]
    s_c = s[who].masked_fill(torch.tensor(masked[np.flatnonzero(counted)]), float("-inf"))
    loss = (torch.logsumexp(s_c, dim=1) - s_own).sum() / int(counted.sum())
    loss.backward()
    return float(loss.detach()), D.grad.numpy().astype(np.float64)


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
