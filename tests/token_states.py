"""Shared by the token-state, CLS-pooling and attention-bias tests (CPU and GPU) and tools/fuzz_encoder.py: the two weight
sets, the cases' references (`reference`), the error metric, the margins and the one comparison (`check`) against
oracle/float64_reference.py.

The bound a GPU result must meet is never a number written down here: it is `margin x E_ref`, where E_ref is the error
of an fp32 implementation against the float64 reference ON THE SAME INPUTS under the same metric (`row_errors`) - the
fp32 C oracle, or, where a case has an attention bias (the oracle knows none), the reference's own code in float32 -
and the margin comes from MARGINS (chosen from the ratios measured on the MI355X, profiles/token_state_errors.md) or,
with a bias, TOKEN_MARGINS / EMB_MARGINS (profiles/attention_bias_errors.md).

The value-range tests (tests/test_value_ranges.py, tests/test_value_ranges_gpu.py) add the "heavy" weight set and the
pointwise GELU probes, with RANGE_MARGINS; they stand beside KINDS and the tables above, not in them.
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

#: The weight sets and probe models of the value-range tests (tests/test_value_ranges.py, tests/test_value_ranges_gpu.py);
#: kept out of KINDS, which indexes the margin tables of the bias and CLS tests.
RANGE_KINDS = ("heavy",)

#: What the "heavy" set meets in EVERY layer on `calibration_batch()`: share of pre-GELU values with |u| > 3, share with
#: |u| > 5.75 (where the f16x3 GELU clamps its polynomial's argument), mean over rows of the largest softmax weight.
#: HEAVY_AIMS is what the search asks for, 5 % inside, so that the assertions never sit on a rounding edge;
#: HEAVY_LIMITS (largest |u|, logit std) keep the set in a trained model's range and far from plane saturation.
HEAVY_THRESHOLDS = (0.20, 0.02, 0.90)
HEAVY_AIMS = (0.21, 0.021, 0.92)
HEAVY_LIMITS = (64.0, 128.0)

#: (factor on Wq and Wk, factor on every intermediate.dense.weight) of the "heavy" set, per (hidden, layers); found by
#: `find_heavy_scales` (tests/test_value_ranges.py re-runs the search and checks the conditions).
HEAVY_SCALES = {(384, 6): (16.0, 2.0 ** 2.75), (384, 2): (2.0 ** 3.75, 2.0 ** 2.5), (384, 1): (2.0 ** 3.75, 2.0 ** 2.5),
                (768, 2): (2.0 ** 3.25, 4.0)}

#: margin on E_ref per (gemm mode, hidden, "heavy" | "probe"): (per-token-row rms, max abs).  Each is the smallest of
#: {2, 3, 4, 6, 8, 12, 16} that leaves 1.5x headroom over the worst ratio E_gpu / E_ref measured on the MI355X over every
#: case of tests/test_value_ranges_gpu.py (profiles/token_state_errors.md, "Value ranges", holds the ratios).  The set
#: reaches 16 because, where one term dominates a sum (one-hot P.V, the probes' single-weight GEMM), the planes'
#: 2^-21 relative split error stands a factor 8 above fp32's 2^-24.
RANGE_MARGINS = {
    ("f32", 384, "heavy"): (2, 2), ("f32", 384, "probe"): (2, 2),
    ("f32", 768, "heavy"): (2, 2), ("f32", 768, "probe"): (2, 2),
    ("f16x3", 384, "heavy"): (2, 2), ("f16x3", 384, "probe"): (4, 6),
    ("f16x3", 768, "heavy"): (2, 3), ("f16x3", 768, "probe"): (3, 6),
}


def range_margin(mode: str, hidden: int, kind: str):
    """RANGE_MARGINS' entry of a weight set of the value-range tests: every probe model shares "probe"."""
    return RANGE_MARGINS[(mode, hidden, "probe" if kind in PROBE_KINDS else kind)]


#: margin on E_ref per (gemm mode, hidden, weight set): (per-token-row rms, max abs).  Each is the smallest of
#: {2, 3, 4, 6, 8} that leaves 1.5x headroom over the worst ratio E_gpu / E_ref measured on the MI355X over every case
#: of tests/test_token_states_gpu.py (profiles/token_state_errors.md holds the ratios).
MARGINS = {
    ("f32", 384, "standard"): (2, 3), ("f32", 384, "sharp"): (2, 3),
    ("f32", 768, "standard"): (2, 2), ("f32", 768, "sharp"): (2, 2),
    ("f16x3", 384, "standard"): (3, 6), ("f16x3", 384, "sharp"): (3, 4),
    ("f16x3", 768, "standard"): (2, 2), ("f16x3", 768, "sharp"): (2, 3),
}

#: margin on E_ref per (gemm mode, hidden, weight set): (per-token-row rms, max abs) - TOKEN_MARGINS for the token states
#: of the biased cases, EMB_MARGINS for their pooled rows (mean and CLS embeddings: the reference pools with torch's
#: pairwise mean, the kernels add the tokens in order, so a pooled row's ratios are larger than its tokens').  Each is
#: the smallest of {2, 3, 4, 6, 8} that leaves 1.5x headroom over the worst ratio E_gpu / E_ref measured on the MI355X
#: over every case of tests/test_attention_bias_gpu.py (profiles/attention_bias_errors.md holds the ratios; the worst of
#: all is 5.13, under 8 / 1.5).
TOKEN_MARGINS = {
    ("f32", 384, "standard"): (2, 2), ("f32", 384, "sharp"): (2, 2),
    ("f32", 768, "standard"): (2, 2), ("f32", 768, "sharp"): (2, 2),
    ("f16x3", 384, "standard"): (3, 3), ("f16x3", 384, "sharp"): (3, 4),
    ("f16x3", 768, "standard"): (2, 2), ("f16x3", 768, "sharp"): (2, 2),
}
EMB_MARGINS = {
    ("f32", 384, "standard"): (6, 6), ("f32", 384, "sharp"): (6, 8),
    ("f32", 768, "standard"): (6, 6), ("f32", 768, "sharp"): (4, 6),
    ("f16x3", 384, "standard"): (6, 8), ("f16x3", 384, "sharp"): (6, 8),
    ("f16x3", 768, "standard"): (6, 6), ("f16x3", 768, "sharp"): (6, 6),
}

#: the n_normalize values `reference` prepares CLS / mean embeddings for
N_NORMALIZE = (1, 2)


def shape(hidden: int, layers: int) -> syn.BertShape:
    return syn.BertShape(vocab_size=VOCAB, layers=layers, **WIDTHS[hidden])


def weights(kind: str, s: syn.BertShape, seed: int = 17, qk_scale: float | None = None,
            w1_scale: float | None = None) -> np.ndarray:
    """The weight blob of a set.

    "standard": synthetic_bert_weights at BERT's init, std 0.02 (logits are tiny, softmax is nearly uniform).
    "sharp":    the same generator and seed, then Wq and Wk times SHARP_QK_SCALE (found by find_qk_scale: 4.0 at hidden 384
                with 6 or 2 layers, 3.36 with 1 layer, 2.83 at hidden 768 with 2 layers; logit std 3.1 - 4.1 per layer
                against 0.15 for "standard", the largest softmax weight of a row averages 0.32 - 0.41 against 0.012:
                attention is peaked, not one-hot), every LayerNorm gain replaced by 2^u with u uniform in
                [-1, 1] (gains over [0.5, 2]), biases left as generated (non-zero).
    "heavy":    "sharp" with the larger Q/K factor of HEAVY_SCALES and its factor on every intermediate.dense.weight
                (found by find_heavy_scales: 16 and 6.73 at hidden 384 with 6 layers, 13.5 and 5.66 with 2 or 1, 9.51
                and 4 at hidden 768): the range of a trained checkpoint - per layer the largest softmax weight of a
                row averages 0.93 - 0.96 (logit std 35 - 59), 24 - 34 % of the pre-GELU values lie beyond |u| = 3 and
                2.3 - 6.5 % beyond 5.75, the largest is 12 - 16.
    "probe0" ... "probe3", "probe_large" (one layer): "standard" with the FFN turned into a function evaluator -
                intermediate.dense.weight = 0 and its bias = probe_sweep(kind), so that every token's pre-GELU vector
                IS the sweep (the accumulator is 0 in either GEMM mode); output.dense.weight[f, f + hidden c] = 1 (exact
                in the weight planes) and 0 elsewhere, c = probe_chunk(kind), output.dense.bias = 0: the block's output
                is LN(gelu(sweep[f + hidden c]) + x[f]) per token."""
    w = syn.synthetic_bert_weights(s, seed=seed, std=0.02)
    if kind == "standard":
        return w
    if kind in PROBE_KINDS:
        assert s.layers == 1, "the GELU probes are one-layer models"
        sd = syn.blob_to_state_dict(w, s)  # views into w
        sd["encoder.layer.0.intermediate.dense.weight"][:] = 0.0
        sd["encoder.layer.0.intermediate.dense.bias"][:] = probe_sweep(kind, s)
        w2 = sd["encoder.layer.0.output.dense.weight"]  # [hidden, intermediate]
        w2[:] = 0.0
        f = np.arange(s.hidden)
        w2[f, f + s.hidden * probe_chunk(kind)] = 1.0
        sd["encoder.layer.0.output.dense.bias"][:] = 0.0
        return w
    assert kind == "sharp" or kind in RANGE_KINDS, kind
    if kind == "heavy":
        heavy = HEAVY_SCALES.get((s.hidden, s.layers), (None, None))
        scale = float(qk_scale if qk_scale is not None else heavy[0])
        w1_scale = float(w1_scale if w1_scale is not None else heavy[1])
    else:
        assert w1_scale is None
        scale = float(qk_scale if qk_scale is not None else SHARP_QK_SCALE[(s.hidden, s.layers)])
    for t, (name, a) in enumerate(syn.blob_to_state_dict(w, s).items()):  # views into w
        if name.endswith("LayerNorm.weight"):
            a[:] = np.exp2(2.0 * syn.uniform(seed + 1, t, a.size) - 1.0).astype(np.float32)
    return _scale_qk_w1(w, s, scale, w1_scale if kind == "heavy" else 1.0)


def _scale_qk_w1(w: np.ndarray, s: syn.BertShape, qk_scale: float, w1_scale: float) -> np.ndarray:
    """Wq and Wk times qk_scale, every intermediate.dense.weight times w1_scale, in place."""
    for name, a in syn.blob_to_state_dict(w, s).items():  # views into w
        if name.endswith(("query.weight", "key.weight")):
            a *= np.float32(qk_scale)
        elif name.endswith("intermediate.dense.weight") and w1_scale != 1.0:
            a *= np.float32(w1_scale)
    return w


def calibration_batch():
    """Lengths 5 / 33 / 128 / 256: what the sharp set's Q/K factor is found on."""
    return packed([5, 33, 128, 256], 1, VOCAB)


def logit_stats(w: np.ndarray, s: syn.BertShape, ids, cu):
    """Per layer (std of the pre-softmax logits, mean largest softmax weight of a row) in the float64 reference."""
    return [(st.logit_std, st.mean_max_softmax) for st in layer_stats(w, s, ids, cu)]


def layer_stats(w: np.ndarray, s: syn.BertShape, ids, cu):
    """Per layer the float64 reference's LayerStats: logit std, mean largest softmax weight of a row, the shares of
    pre-GELU values with |u| > 3 and with |u| > 5.75, the largest |u|."""
    from oracle import float64_reference as f64

    stats: list = []
    f64.encode(w, s, ids, cu, stats=stats)
    return stats


def heavy_conditions(stats, aim: bool = False) -> dict:
    """What the "heavy" set must meet in EVERY layer, as name -> bool: HEAVY_THRESHOLDS (with `aim`, HEAVY_AIMS: what
    the search asks for, 5 % inside) and HEAVY_LIMITS."""
    u3, u575, pmax = HEAVY_AIMS if aim else HEAVY_THRESHOLDS
    max_u, max_std = HEAVY_LIMITS
    return {"share |u| > 3": min(st.share_u_gt_3 for st in stats) >= u3,
            "share |u| > 5.75": min(st.share_u_gt_5_75 for st in stats) >= u575,
            "mean max softmax weight": min(st.mean_max_softmax for st in stats) >= pmax,
            "largest |u|": max(st.max_abs_u for st in stats) < max_u,
            "logit std": max(st.logit_std for st in stats) < max_std}


def find_heavy_scales(s: syn.BertShape, seed: int = 17):
    """(Q/K factor, W1 factor) of the "heavy" set, each the smallest 2^(k/4), k = 0, 1, ..., on calibration_batch(),
    the Q/K factor first: one under which every layer's largest softmax weight of a row averages HEAVY_AIMS' 0.92 with
    the W1 factor still 1; then, with that Q/K factor in place, the smallest W1 factor that brings every layer's shares
    of |u| > 3 and > 5.75 to their aims.  A larger FFN output is a less peaked next layer (at 6 layers the W1 factor
    that the shares need takes the last layer's softmax weight from 0.94 to below 0.90), so the pair counts only if
    every layer then meets ALL of heavy_conditions(aim=True); if not, the next Q/K factor is tried."""
    ids, cu = calibration_batch()
    base = weights("heavy", s, seed, qk_scale=1.0, w1_scale=1.0)  # generated once: a factor of 1 changes no bit

    def conditions(qk, w1):
        return heavy_conditions(layer_stats(_scale_qk_w1(base.copy(), s, qk, w1), s, ids, cu), aim=True)

    for qk in (float(2.0 ** (k / 4)) for k in range(0, 33)):
        if not conditions(qk, 1.0)["mean max softmax weight"]:
            continue
        for w1 in (float(2.0 ** (k / 4)) for k in range(0, 33)):
            c = conditions(qk, w1)
            if c["share |u| > 3"] and c["share |u| > 5.75"]:  # both grow with the W1 factor
                if all(c.values()):
                    return qk, w1
                break
    raise AssertionError("no Q/K and W1 factors up to 256 meet the heavy set's conditions")


#: the FFN values of the pointwise GELU probes (`probe_sweep`), beside a grid over [-8, 8]: signed zeros, values whose
#: square underflows, the faults' |u| = 3, the kernel's clamp 5.75 and its fp32 neighbours on both sides
PROBE_SPECIALS = [sg * v for v in (0.0, 1e-30, 1e-8, 3.0, float(np.nextafter(np.float32(5.75), np.float32(0))), 5.75,
                                   float(np.nextafter(np.float32(5.75), np.float32(8)))) for sg in (1.0, -1.0)]
#: the values of the large-value probe
PROBE_LARGE = [10.0, -10.0, 30.0, -30.0, 100.0, -100.0]
#: the probe models: chunk c of the sweep (PROBE_KINDS[c], c < 4) and the large-value probe
PROBE_KINDS = ("probe0", "probe1", "probe2", "probe3", "probe_large")


def probe_sweep(kind: str, s: syn.BertShape) -> np.ndarray:
    """The pre-GELU vector (float32 [intermediate]) every token of a probe model has.  "probe0" ... "probe3": the
    PROBE_SPECIALS and an even grid over [-8, 8], shuffled with a fixed seed so that neighbours on the grid land in
    different chunks of `hidden` values.  "probe_large": the PROBE_LARGE values at the head of a shuffled even grid
    over [-1, 1] - a probe of their own, because a row with a 100 in it has a standard deviation of 4 - 5, by which
    its LayerNorm would scale every other element's error down."""
    rng = np.random.default_rng(29)
    if kind == "probe_large":
        return np.concatenate([PROBE_LARGE, rng.permutation(np.linspace(-1.0, 1.0, s.intermediate - len(PROBE_LARGE)))]
                              ).astype(np.float32)
    grid = np.linspace(-8.0, 8.0, s.intermediate - len(PROBE_SPECIALS))
    return rng.permutation(np.concatenate([PROBE_SPECIALS, grid])).astype(np.float32)


def probe_chunk(kind: str) -> int:
    """Which `hidden` values of the sweep a probe model's FFN-down projection passes on."""
    return 0 if kind == "probe_large" else PROBE_KINDS.index(kind)


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


def normalize_rows(v: np.ndarray, n: int) -> np.ndarray:
    """n times v / max(|v|_2, 1e-12) per row, in v's own precision."""
    for _ in range(n):
        v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), v.dtype.type(1e-12))
    return v


_refs: dict = {}


def reference(kind: str, hidden: int, layers: int, lens, seed: int, max_len=None, table=None, ref32: str = "oracle") -> dict:
    """Weights, inputs and both precisions' results of one case, computed once and shared by every test that runs it;
    the weights and every result are read-only (ids and cu stay writable: torch.from_numpy warns about memory that is not):

    s, w, ids, cu, kind, max_len (the encoder's max_seq_length), table (float32 [heads, 1023] or None);
    h64 / e64      the float64 reference's token states / mean-pooled embeddings;
    h32 / e32      the same from the fp32 implementation whose error is E_ref: the C oracle (ref32 = "oracle", cases
                   without a table only) or the reference's own code in float32 (ref32 = "float32");
    cls64[n] / mean64[n] / cls32[n], n in N_NORMALIZE: the first-token rows of h64, the float64 means of each sequence's
                   rows of h64 and the first-token rows of h32, normalised n times - cls32 by the implementation that
                   made h32 (oracle.normalize_rows, or float32 numpy)."""
    key = (kind, hidden, layers, tuple(lens), seed, max_len, None if table is None else table.tobytes(), ref32)
    if key not in _refs:
        import torch

        from oracle import float64_reference as f64
        from oracle import oracle

        s = shape(hidden, layers)
        w = weights(kind, s)
        ids, cu = packed(lens, seed, VOCAB)
        h64, e64 = f64.encode(w, s, ids, cu, attention_bias=table)
        first = cu[:-1].astype(np.int64)
        if ref32 == "oracle":
            assert table is None, "the C oracle knows no attention bias"
            e32, h32 = oracle.encode(w, oracle.cfg_for(s), ids, cu, return_hidden=True)
            cls32 = {0: np.ascontiguousarray(h32[first])}
            for n in range(1, max(N_NORMALIZE) + 1):
                cls32[n] = oracle.normalize_rows(cls32[n - 1])
        else:
            assert ref32 == "float32", ref32
            h32, e32 = f64.encode(w, s, ids, cu, dtype=torch.float32, attention_bias=table)
            cls32 = {n: normalize_rows(h32[first], n) for n in N_NORMALIZE}
        mean_h = np.stack([h64[a:b].mean(0) for a, b in zip(cu[:-1], cu[1:])])
        r = dict(s=s, w=w, ids=ids, cu=cu, kind=kind, max_len=max_len, table=table, h64=h64, e64=e64, h32=h32, e32=e32,
                 cls64={n: normalize_rows(h64[first], n) for n in N_NORMALIZE},
                 mean64={n: normalize_rows(mean_h, n) for n in N_NORMALIZE},
                 cls32={n: cls32[n] for n in N_NORMALIZE})
        for a in (w, h64, e64, h32, e32, *r["cls64"].values(), *r["mean64"].values(), *r["cls32"].values()):
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def check(what: str, got: np.ndarray, want64: np.ndarray, ref32: np.ndarray, margin, cu=None):
    """Prints `RATIO ...` (E_gpu / E_ref, rms and max abs), then asserts E_gpu <= margin x E_ref for both; with `cu` a
    failure names the worst token and element."""
    e_rms, e_abs = row_errors(ref32, want64)
    g_rms, g_abs = row_errors(got, want64)
    assert e_rms > 0 and e_abs > 0
    print(f"RATIO {what}: E_gpu rms {g_rms:.3e} abs {g_abs:.3e}, E_ref rms {e_rms:.3e} abs {e_abs:.3e}, "
          f"ratio rms {g_rms / e_rms:.2f} abs {g_abs / e_abs:.2f} (margins {margin[0]} / {margin[1]})")
    where = "" if cu is None else worst_element(got, want64, cu)
    assert g_rms <= margin[0] * e_rms and g_abs <= margin[1] * e_abs, (what, where)
