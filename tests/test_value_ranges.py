"""The value ranges of a trained checkpoint, on the CPU: the "heavy" weight set (pre-GELU values beyond |u| = 3 and beyond
the f16x3 GELU's clamp at 5.75 in every layer, near-one-hot attention) and the pointwise GELU probes of
tests/token_states.py are what they claim to be, the fp32 oracle stays well-behaved on them (E_ref, what the GPU bound of
tests/test_value_ranges_gpu.py is built from), and every fault the float64 reference can inject stands at least twice
that GPU bound from the clean result - the three GELU range faults (oracle/float64_reference.py, RANGE_FAULTS) included,
which no input of tests/test_token_states.py reaches.

Measured here (E_ref = oracle against float64, per-token-row rms / max abs):

    heavy, batch [5, 33, 128, 256, 512, 1, 2, 64]:  hidden 384, 6 layers  2.2e-05 / 1.0e-04    1 layer  1.9e-06 / 1.0e-05
                                                    hidden 768, 2 layers  1.2e-05 / 6.4e-05
    probes, [5, 33] tokens:                         1.0 - 1.5e-07 / 4.7 - 7.0e-07 at both widths, every chunk;
                                                    the large-value probe 1.9e-07 / 3.5 - 4.9e-06

and the faults against the GPU bound with the final margins: the three GELU range faults and tanh_gelu stand 33 - 630
times above it on every probe chunk (gelu_erfc_rel_1e-3 the least: 134 - 163 x E_ref), every fault but the two
UNDETECTED entries at least 2.7 times on the heavy set.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import float64_reference as f64
from oracle import oracle
from tests import token_states as ts
from tests.encoder_harness import packed

SHAPES = [(384, 6), (384, 1), (768, 2)]
FAULT_LENS = (5, 33, 128, 256, 512)
MODES = ("f32", "f16x3")
ALL_FAULTS = sorted({**f64.FAULTS, **f64.RANGE_FAULTS})
GELU_FAULTS = sorted(f64.RANGE_FAULTS) + ["tanh_gelu"]
PROBE_LENS = [5, 33]

#: layer counts of the heavy models a fault is tried in, per width: the 2-layer models of the GPU tests' bucket-edge and
#: batch cases, and the 6-layer one.  On the heavy set an error made in an early layer GROWS on its way through the later
#: ones (a row whose two best keys nearly tie picks the other one), E_ref with it - 1.7e-06 row rms on the 586 tokens of
#: the GPU tests' small batch with 1 layer, 1.7e-05 with 6 - so a last-layer fault of a given size is judged against a
#: bound that is 10x larger in the 6-layer model than the same kernel mistake is in the 1- and 2-layer models: with 6
#: layers softmax_f16 and v_f16 in the last layer stand at 0.8 - 2.7 / 1.1 - 5.2 times the GPU bound, with 2 layers at
#: 4.5 - 7 / 6.6 - 16 times.  The kernels are the same in every layer; the 6-layer GPU case is there for the middle
#: layers' code.
HEAVY_MODELS = {384: (2, 6), 768: (2,)}

# Faults that cannot clear 2x the GPU bound ON THE HEAVY SET in any model of the width, with the measured ratio (the
# fault's row-rms distance from the clean hidden state / GPU bound): (fault, where) with `where` a key of WHERE.
WHERE = {"either layer, both widths": lambda layer_of, hidden: True,
         "last layer, hidden 768": lambda layer_of, hidden: layer_of == "last" and hidden == 768}
UNDETECTED = {
    # an eps of 1e-5 moves a row by 5e-6 / its variance, which is of the order of 1: as much as the heavy set's GPU bound
    # (2 x E_ref of 4e-6 and more with 2 layers); asserted on the standard set, in the last layer
    # (tests/test_token_states.py)
    ("ln_eps_1e-5", "either layer, both widths"): "ratio 0.0 - 0.8",
    # |u| > 4 is a tenth of the values and the clamp moves none by more than 1.3e-4: ratio 5 - 7 in the first layer at
    # hidden 768, 10 - 27 and 4.4 - 10 in the first and last at hidden 384 with 2 layers (0.7 - 4 in the last of 6),
    # and 63 - 98 on every probe chunk
    ("gelu_clamp_4", "last layer, hidden 768"): "ratio 1.4 - 2.2 from 33 tokens up (4.4 at 5)",
}


def _listed(fault, layer_of, hidden):
    return any(name == fault and WHERE[where](layer_of, hidden) for name, where in UNDETECTED)


@functools.lru_cache(maxsize=None)
def _model(kind, hidden, layers):
    s = ts.shape(hidden, layers)
    w = ts.weights(kind, s)
    return s, w, f64.Float64Bert(w, s)


@functools.lru_cache(maxsize=None)
def _clean(kind, hidden, layers, lens):
    """Sequences of the given lengths: (ids, cu, clean float64 hidden state, E_ref row rms of the oracle on them)."""
    s, w, m = _model(kind, hidden, layers)
    ids, cu = packed(list(lens), sum(lens), ts.VOCAB)
    clean, _ = m.encode(ids, cu)
    _, hid = oracle.encode(w, oracle.cfg_for(s), ids, cu, return_hidden=True)
    return ids, cu, clean, ts.row_errors(hid, clean)[0]


def _bound(hidden, kind, e_ref):
    """The GPU bound on the row rms: the LARGER of the two modes' margins x E_ref."""
    return max(ts.range_margin(mode, hidden, kind)[0] for mode in MODES) * e_ref


@pytest.mark.parametrize("hidden,layers", SHAPES + [(384, 2)])
def test_heavy_weights_are_heavy(hidden, layers):
    """The factors in HEAVY_SCALES are the ones the search finds; under them EVERY layer meets HEAVY_THRESHOLDS (share of
    |u| > 3 >= 0.20, share of |u| > 5.75 >= 0.02, mean largest softmax weight >= 0.90) and HEAVY_LIMITS (largest |u|
    < 64, logit std < 128) on the calibration batch; the set is the sharp one in everything else."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    s = ts.shape(hidden, layers)
    assert ts.find_heavy_scales(s) == ts.HEAVY_SCALES[(hidden, layers)]
    w = ts.weights("heavy", s)
    stats = ts.layer_stats(w, s, *ts.calibration_batch())
    print(f"hidden {hidden} layers {layers}: per layer {[tuple(round(v, 4) for v in st) for st in stats]}")
    assert len(stats) == layers
    assert all(ts.heavy_conditions(stats).values()), (ts.heavy_conditions(stats), stats)
    for st in stats:  # the same conditions, spelled out
        assert st.share_u_gt_3 >= 0.20 and st.share_u_gt_5_75 >= 0.02 and st.mean_max_softmax >= 0.90, st
        assert st.max_abs_u < 64 and st.logit_std < 128, st
    qk, w1 = ts.HEAVY_SCALES[(hidden, layers)]
    sharp = syn.blob_to_state_dict(ts.weights("sharp", s, qk_scale=1.0), s)
    for name, a in syn.blob_to_state_dict(w, s).items():
        f = qk if name.endswith(("query.weight", "key.weight")) else w1 if name.endswith("intermediate.dense.weight") else 1.0
        np.testing.assert_array_equal(a, sharp[name] * np.float32(f), err_msg=name)


@pytest.mark.parametrize("kind", ts.PROBE_KINDS)
@pytest.mark.parametrize("hidden", [384, 768])
def test_probe_models_evaluate_gelu_pointwise(hidden, kind):
    """Every token's pre-GELU vector is the sweep itself, the FFN-down projection passes on one chunk of `hidden` values
    with weight 1, and the sweeps hold what they claim: the specials, a grid over [-8, 8] whose every chunk has values
    beyond |u| = 3 and beyond 5.75, and the large values alone among small ones."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    s = ts.shape(hidden, 1)
    w = ts.weights(kind, s)
    sweep, c = ts.probe_sweep(kind, s), ts.probe_chunk(kind)
    assert sweep.dtype == np.float32 and sweep.shape == (s.intermediate,)
    sd = syn.blob_to_state_dict(w, s)
    w2 = sd["encoder.layer.0.output.dense.weight"]
    assert w2.sum() == hidden and (w2[np.arange(hidden), np.arange(hidden) + hidden * c] == 1).all()
    assert not sd["encoder.layer.0.intermediate.dense.weight"].any() and not sd["encoder.layer.0.output.dense.bias"].any()
    (st,) = ts.layer_stats(w, s, *packed(PROBE_LENS, 1, ts.VOCAB))
    assert st.max_abs_u == np.abs(sweep).max()
    assert st.share_u_gt_3 == (np.abs(sweep) > 3).mean() and st.share_u_gt_5_75 == (np.abs(sweep) > 5.75).mean()
    chunk = sweep[hidden * c: hidden * (c + 1)]
    if kind == "probe_large":
        assert chunk[:6].tolist() == ts.PROBE_LARGE and np.abs(sweep[6:]).max() <= 1
        return
    assert np.abs(sweep).max() == 8 and (np.abs(chunk) > 5.75).sum() >= 32 and (np.abs(chunk) < 3).sum() >= 32
    bits = set(sweep.view(np.uint32).tolist())
    assert {int(np.float32(v).view(np.uint32)) for v in ts.PROBE_SPECIALS} <= bits
    above, below = np.nextafter(np.float32(5.75), np.float32(8)), np.nextafter(np.float32(5.75), np.float32(0))
    for v in (0.0, -0.0, 1e-30, -1e-30, 1e-8, -1e-8, 3.0, -3.0, 5.75, -5.75, above, -above, below, -below):
        assert int(np.float32(v).view(np.uint32)) in bits, v
    grid = np.sort(sweep)
    assert np.diff(grid).max() <= 16.0 / (s.intermediate - len(ts.PROBE_SPECIALS) - 1) * 1.001


@pytest.mark.parametrize("hidden,layers", SHAPES)
def test_oracle_error_on_the_heavy_set(hidden, layers):
    """E_ref on the heavy set: positive, and pinned only in scale (row rms within 1e-4, max abs within 1e-3 on hidden
    states of rms ~1: fp32 stays well-behaved where attention is one-hot and a fifth of the GELU inputs lie in its
    tails) - the GPU bound uses the measured value."""
    s, w, m = _model("heavy", hidden, layers)
    ids, cu = packed([5, 33, 128, 256, 512, 1, 2, 64], 2, ts.VOCAB)
    want_h, want_e = m.encode(ids, cu)
    emb, hid = oracle.encode(w, oracle.cfg_for(s), ids, cu, return_hidden=True)
    e_rms, e_abs = ts.row_errors(hid, want_h)
    e_emb = float(np.abs(emb - want_e).max())
    print(f"hidden {hidden} layers {layers} heavy: oracle vs float64 row rms {e_rms:.3e} max abs {e_abs:.3e}, "
          f"pooled max abs {e_emb:.3e}; max |h| {np.abs(want_h).max():.1f}, rms {np.sqrt((want_h ** 2).mean()):.2f}")
    assert 0 < e_rms < 1e-4 and e_rms <= e_abs < 1e-3
    assert e_emb < 1e-5


@pytest.mark.parametrize("kind", ts.PROBE_KINDS)
@pytest.mark.parametrize("hidden", [384, 768])
def test_oracle_error_on_the_probes(hidden, kind):
    """E_ref on the probes: positive, and one layer's worth of fp32 roundings (row rms within 1e-6, max abs within 1e-5)."""
    s, w, m = _model(kind, hidden, 1)
    ids, cu = packed(PROBE_LENS, 1, ts.VOCAB)
    want_h, _ = m.encode(ids, cu)
    _, hid = oracle.encode(w, oracle.cfg_for(s), ids, cu, return_hidden=True)
    e_rms, e_abs = ts.row_errors(hid, want_h)
    print(f"hidden {hidden} {kind}: oracle vs float64 row rms {e_rms:.3e} max abs {e_abs:.3e}; "
          f"max |h| {np.abs(want_h).max():.1f}")
    assert 0 < e_rms < 1e-6 and e_rms <= e_abs < 1e-5


@pytest.mark.parametrize("layer_of", ["first", "last"])
@pytest.mark.parametrize("fault", ALL_FAULTS)
@pytest.mark.parametrize("hidden", [384, 768])
def test_every_fault_clears_twice_the_gpu_bound_on_the_heavy_set(hidden, fault, layer_of):
    """One fault in one layer, one sequence of 5 ... 512 tokens of the heavy set: the faulty float64 hidden state must
    stand at least 2x the GPU bound (the LARGER of the two modes' RANGE_MARGINS x E_ref on the same input) from the
    clean one, under the row-rms metric, at EVERY length, in at least one of the width's HEAVY_MODELS - or be listed
    in UNDETECTED and stay below the bar."""
    best = {}
    for layers in HEAVY_MODELS[hidden]:
        layer = 0 if layer_of == "first" else layers - 1
        s, w, m = _model("heavy", hidden, layers)
        for n in FAULT_LENS:
            ids, cu, clean, e_ref = _clean("heavy", hidden, layers, (n,))
            bad, _ = m.encode(ids, cu, fault=(fault, layer))
            ratio = ts.row_errors(bad, clean)[0] / _bound(hidden, "heavy", e_ref)
            print(f"{fault} layer {layer} of {layers} hidden {hidden} heavy length {n}: fault / GPU bound = {ratio:.1f}")
            best[n] = max(best.get(n, 0.0), ratio)
    if _listed(fault, layer_of, hidden):
        assert min(best.values()) < 2.0, f"{fault} is listed as undetectable but clears the bar: {best}"
        return
    assert min(best.values()) >= 2.0, f"{fault} in the {layer_of} layer: fault / GPU bound per length {best}"


@pytest.mark.parametrize("fault", GELU_FAULTS)
@pytest.mark.parametrize("kind", ts.PROBE_KINDS[:4])
@pytest.mark.parametrize("hidden", [384, 768])
def test_gelu_faults_clear_twice_the_gpu_bound_on_every_probe_chunk(hidden, kind, fault):
    """The three GELU range faults and the tanh form, on [5, 33] tokens of every probe chunk (each holds values beyond
    |u| = 3, see test_probe_models_evaluate_gelu_pointwise): at least 2x the GPU bound from the clean hidden state."""
    s, w, m = _model(kind, hidden, 1)
    assert (np.abs(ts.probe_sweep(kind, s)[hidden * ts.probe_chunk(kind):][:hidden]) > 3).any()
    ids, cu, clean, e_ref = _clean(kind, hidden, 1, tuple(PROBE_LENS))
    bad, _ = m.encode(ids, cu, fault=(fault, 0))
    ratio = ts.row_errors(bad, clean)[0] / _bound(hidden, kind, e_ref)
    print(f"{fault} hidden {hidden} {kind}: fault / GPU bound = {ratio:.1f} "
          f"(fault / E_ref = {ratio * _bound(hidden, kind, 1.0):.0f})")
    assert ratio >= 2.0


def test_undetected_table_is_short_and_spares_the_faults_that_matter():
    assert len(UNDETECTED) <= 2
    must = {"gelu_tail_dropped", "softmax_f16", "v_f16", "gelu_f16", "stale_last_row"}
    assert must <= set(ALL_FAULTS) and not must & {name for name, _ in UNDETECTED}
    assert all(name in ALL_FAULTS and where in WHERE for name, where in UNDETECTED)


def test_range_faults_change_only_what_they_say():
    """Where every |u| <= 3 (the standard set) a dropped tail and a clamp at 4 change nothing to speak of - the clamp
    nothing at all; on the heavy set each of the three moves the hidden state; the names are accepted beside FAULTS'."""
    ids, cu = packed([7, 40], 3, ts.VOCAB)
    s, w, m = _model("standard", 384, 1)
    clean, _ = m.encode(ids, cu)
    for fault, tol in (("gelu_tail_dropped", 0.0), ("gelu_clamp_4", 1e-15)):  # erf and erfc forms differ by roundings
        bad, _ = m.encode(ids, cu, fault=(fault, 0))
        assert np.abs(bad - clean).max() <= tol, fault
    s, w, m = _model("heavy", 384, 1)
    clean, _ = m.encode(ids, cu)
    for fault in f64.RANGE_FAULTS:
        assert fault not in f64.FAULTS
        bad, _ = m.encode(ids, cu, fault=(fault, 0))
        assert np.abs(bad - clean).max() > 1e-5, fault
