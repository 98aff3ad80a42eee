"""Shared by tests/test_cls_pooling.py (CPU) and tests/test_cls_pooling_gpu.py: the cases of the CLS-pooling comparison
against the references.

Nothing in oracle/ knows about CLS pooling, and nothing there needs to: Pooling(cls) IS the last hidden state of each
sequence's first token, so the fp32 reference is rows cu[:-1] of `oracle.encode(..., return_hidden=True)` passed
n_normalize times through `oracle.normalize_rows`, and the float64 reference is the same rows of
oracle/float64_reference.py's token states, normalised in float64 (`cls32` / `cls64` of token_states.reference).  The
bound a GPU result must meet is `margin x E_ref` (token_states.check), E_ref being the fp32 reference's own error
against the float64 one on the same inputs.  The margins are token_states.MARGINS, which were measured on per-token
rows: the ratios E_gpu / E_ref of the normalised CLS rows measured on the MI355X (profiles/cls_pooling_errors.md) stay
under every entry divided by 1.5, so none is replaced.
"""
from __future__ import annotations

from tests import token_states as ts

#: (hidden, layers): 6 layers and 1 layer at hidden 384 (with one layer the pruned layer is also layer 0), 2 at 768
SHAPES = [(384, 6), (384, 1), (768, 2)]
#: name -> (sequence lengths of one batch, the encoder's max_seq_length, seed of the ids)
BATCHES = {"to256": ([1, 2, 31, 32, 33, 64, 128, 256], None, 2), "to512": ([257, 300, 512], 512, 3)}
N_NORMALIZE = ts.N_NORMALIZE


def reference(kind: str, hidden: int, layers: int, batch: str) -> dict:
    """token_states.reference of a named case; E_ref is the fp32 C oracle's error."""
    lens, max_len, seed = BATCHES[batch]
    return ts.reference(kind, hidden, layers, lens, seed, max_len)
