"""The whole-catalog adapter step (include/icrec.h, icrec_adapter_step_catalog) restated without a GPU, from the math:
cross_entropy(scale * u @ V.T, pos) over the counted anchors, differentiated by autograd - the same code in float64
(the truth) and in float32 (E_ref).  apply, the stored rows and AdamW are tests/adapter_reference.py's."""
from __future__ import annotations

import numpy as np
import torch

from tests.adapter_reference import adamw, apply, stored_rows  # noqa: F401  (one definition of each, re-exported)


def counted(pos, n_rows: int) -> np.ndarray:
    """bool [B]: the anchors whose positive lies in [0, n_rows)."""
    pos = np.asarray(pos, np.int64)
    return (pos >= 0) & (pos < n_rows)


def loss_and_grad(delta, anchors, rows, pos, scale, dtype=torch.float64):
    """(loss, d loss / d delta [d, d]) of anchors [B, d] against EVERY row of `rows` (stored_rows(P, storage)), pos [B] the
    labels.  An anchor whose label is outside the rows is not counted; nobody counted: (0, zeros).  Nothing is masked."""
    D = torch.tensor(np.asarray(delta), dtype=dtype, requires_grad=True)
    A = torch.tensor(np.asarray(anchors), dtype=dtype)
    pos = np.asarray(pos, np.int64)
    who = np.flatnonzero(counted(pos, rows.shape[0]))
    if who.size == 0:
        return 0.0, np.zeros(D.shape, np.float64)
    z = A + A @ D.T
    u = z / z.norm(dim=1, keepdim=True).clamp_min(1e-12)
    V = torch.tensor(np.asarray(rows), dtype=dtype)
    s = float(scale) * (u[torch.tensor(who)] @ V.T)
    loss = torch.nn.functional.cross_entropy(s, torch.tensor(pos[who]), reduction="mean")
    loss.backward()
    return float(loss.detach()), D.grad.numpy().astype(np.float64)


def mean_loss(delta, anchors, rows, pos, scale) -> float:
    """The float64 loss of a set of any size: catalog_loss's truth."""
    return loss_and_grad(delta, anchors, rows, pos, scale, torch.float64)[0]
