"""Shared by tests/test_token_states.py (CPU), tests/test_token_states_gpu.py and tools/fuzz_encoder.py: the two weight
sets, the error metric and the margins of the per-token comparison against oracle/float64_reference.py.

The bound a GPU result must meet is never a number written down here: it is `margin x E_ref`, where E_ref is the error
of the fp32 C oracle against the float64 reference ON THE SAME INPUTS under the same metric (`row_errors`), and
the margin comes from MARGINS, chosen from the ratios measured on the MI355X (profiles/token_state_errors.md).
"""
from __future__ import annotations

import numpy as np

from instacart_next_order_recommendation_amd import synthetic as syn
from tests.encoder_harness import packed

VOCAB = 2048
WIDTHS = {384: dict(hidden=384, heads=12, intermediate=1536), 768: dict(hidden=768, heads=12, intermediate=3072)}
KINDS = ("standard", "sharp")

#: Factor on Wq and Wk of the "sharp" weight set, per (hidden, layers): the smallest 2^(k/4) for which the float64
#: reference's pre-softmax logits have a standard deviation >= 2 in EVERY layer on `calibration_batch()`; found by
#: `find_qk_scale` (tests/test_token_states.py re-runs the search and checks the statistics).
SHARP_QK_SCALE = {(384, 6): 4.0, (384, 2): 4.0, (384, 1): 2.0 ** 1.75, (768, 2): 2.0 ** 1.5}

#: margin on E_ref per (gemm mode, hidden, weight set): (per-token-row rms, max abs).  Each is the smallest of
#: {2, 3, 4, 6, 8} that leaves 1.5x headroom over the worst ratio E_gpu / E_ref measured on the MI355X over every case
#: of tests/test_token_states_gpu.py (profiles/token_state_errors.md holds the ratios).
MARGINS = {
    ("f32", 384, "standard"): (2, 3), ("f32", 384, "sharp"): (2, 3),
    ("f32", 768, "standard"): (2, 2), ("f32", 768, "sharp"): (2, 2),
    ("f16x3", 384, "standard"): (3, 6), ("f16x3", 384, "sharp"): (3, 4),
    ("f16x3", 768, "standard"): (2, 2), ("f16x3", 768, "sharp"): (2, 3),
}


def shape(hidden: int, layers: int) -> syn.BertShape:
    return syn.BertShape(vocab_size=VOCAB, layers=layers, **WIDTHS[hidden])


def weights(kind: str, s: syn.BertShape, seed: int = 17, qk_scale: float | None = None) -> np.ndarray:
    """The weight blob of a set.

    "standard": synthetic_bert_weights at BERT's init, std 0.02 (logits are tiny, softmax is nearly uniform).
    "sharp":    the same generator and seed, then Wq and Wk times SHARP_QK_SCALE (found by find_qk_scale: 4.0 at hidden 384
                with 6 or 2 layers, 3.36 with 1 layer, 2.83 at hidden 768 with 2 layers; logit std 3.1 - 4.1 per layer
                against 0.15 for "standard", the largest softmax weight of a row averages 0.32 - 0.41 against 0.012:
                attention is peaked, not one-hot), every LayerNorm gain replaced by 2^u with u uniform in
                [-1, 1] (gains over [0.5, 2]), biases left as generated (non-zero)."""
    w = syn.synthetic_bert_weights(s, seed=seed, std=0.02)
    if kind == "standard":
        return w
    assert kind == "sharp", kind
    scale = float(qk_scale if qk_scale is not None else SHARP_QK_SCALE[(s.hidden, s.layers)])
    for t, (name, a) in enumerate(syn.blob_to_state_dict(w, s).items()):  # views into w
        if name.endswith(("query.weight", "key.weight")):
            a *= np.float32(scale)
        elif name.endswith("LayerNorm.weight"):
            a[:] = np.exp2(2.0 * syn.uniform(seed + 1, t, a.size) - 1.0).astype(np.float32)
    return w


def calibration_batch():
    """Lengths 5 / 33 / 128 / 256: what the sharp set's Q/K factor is found on."""
    return packed([5, 33, 128, 256], 1, VOCAB)


def logit_stats(w: np.ndarray, s: syn.BertShape, ids, cu):
    """Per layer (std of the pre-softmax logits, mean largest softmax weight of a row) in the float64 reference."""
    from oracle import float64_reference as f64

    stats: list = []
    f64.encode(w, s, ids, cu, stats=stats)
    return stats


def find_qk_scale(s: syn.BertShape, seed: int = 17) -> float:
    """The smallest 2^(k/4), k = 0, 1, ..., under which every layer's logits have std >= 2.1 and every layer's largest
    softmax weight of a row averages at least 0.21 on calibration_batch(): 5 % inside the thresholds the tests assert
    (2 and 0.2), so that those never sit on a rounding edge."""
    ids, cu = calibration_batch()
    for k in range(0, 33):
        scale = float(2.0 ** (k / 4))
        stats = logit_stats(weights("sharp", s, seed, qk_scale=scale), s, ids, cu)
        if min(sd for sd, _ in stats) >= 2.1 and min(pm for _, pm in stats) >= 0.21:
            return scale
    raise AssertionError("no Q/K factor up to 256 gives logits of std 2")


def row_errors(got: np.ndarray, want: np.ndarray):
    """The metric: (largest per-token-row rms error, largest absolute error) of [T, H] hidden states, in float64."""
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    return float(np.sqrt((d * d).mean(axis=1)).max()), float(np.abs(d).max())


def worst_element(got: np.ndarray, want: np.ndarray, cu: np.ndarray) -> str:
    """Names the token whose row is worst (rms) and the worst element of all: sequence, position in it, feature."""
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    cu = np.asarray(cu)
    out = []
    for what, t, f in (("worst row (rms)", int(np.sqrt((d * d).mean(axis=1)).argmax()), None),
                       ("worst element", *map(int, np.unravel_index(np.abs(d).argmax(), d.shape)))):
        if f is None:
            f = int(np.abs(d[t]).argmax())
        seq = int(np.searchsorted(cu, t, side="right")) - 1
        out.append(f"{what}: sequence {seq} (length {int(cu[seq + 1] - cu[seq])}), position {t - int(cu[seq])}, "
                   f"feature {f}, got {float(got[t, f]):.9g}, want {float(want[t, f]):.9g}, "
                   f"row rms error {float(np.sqrt((d[t] ** 2).mean())):.3e}")
    return "; ".join(out)
