"""The per-token comparison proves its own teeth, on the CPU: how far the fp32 oracle is from the float64 reference
(E_ref, what the GPU bound is built from), that the "sharp" weight set is as peaked as it claims, and that every fault
the float64 reference can inject moves the last hidden state by at least twice the GPU bound.

Measured here (max over the batch [5, 33, 128, 256, 512, 1, 2, 64]; per-token-row rms / max abs; |h| has rms 1.0-1.2):

    hidden 384, 6 layers   standard 4.6e-07 / 3.0e-06   sharp 1.2e-06 / 2.1e-05   (max |h| 5.3 / 29.6)
    hidden 384, 1 layer    standard 2.2e-07 / 1.3e-06   sharp 2.6e-07 / 3.0e-06
    hidden 768, 2 layers   standard 6.4e-07 / 4.5e-06   sharp 9.3e-07 / 9.9e-06
    pooled embedding       9e-08 ... 2.8e-07 max abs
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

# Faults that cannot clear 2x the GPU bound, with the measured ratio (fault's row-rms distance from the clean hidden
# state / E_ref): a LayerNorm eps of 1e-5 in layer 0 of a multi-layer model rescales rows of variance ~1 by 5e-6, which
# the LayerNorms behind it undo - ratio 1-2 at every length, both widths, both weight sets.  In the LAST layer (and in
# a 1-layer model) the same fault stands 7-26x above E_ref on the standard set and is asserted like the others.
UNDETECTED = {("ln_eps_1e-5", "first layer of several"): "ratio 1-2"}


@functools.lru_cache(maxsize=None)
def _model(kind, hidden, layers):
    s = ts.shape(hidden, layers)
    w = ts.weights(kind, s)
    return s, w, f64.Float64Bert(w, s)


@functools.lru_cache(maxsize=None)
def _clean(kind, hidden, layers, n):
    """One sequence of n tokens: (ids, cu, clean float64 hidden state, E_ref row rms of the oracle on it)."""
    s, w, m = _model(kind, hidden, layers)
    ids, cu = packed([n], n, ts.VOCAB)
    clean, _ = m.encode(ids, cu)
    _, hid = oracle.encode(w, oracle.cfg_for(s), ids, cu, return_hidden=True)
    return ids, cu, clean, ts.row_errors(hid, clean)[0]


@pytest.mark.parametrize("hidden,layers", SHAPES + [(384, 2)])
def test_sharp_weights_are_sharp(hidden, layers):
    """The Q/K factor in SHARP_QK_SCALE is the one the search finds; under it every layer's logits have std >= 2 and
    the largest softmax weight of a row averages above 0.2 but attention is not one-hot; gains span [0.5, 2]; biases
    are non-zero; the standard set is nearly uniform."""
    from instacart_next_order_recommendation_amd import synthetic as syn

    s = ts.shape(hidden, layers)
    assert ts.find_qk_scale(s) == ts.SHARP_QK_SCALE[(hidden, layers)]
    w = ts.weights("sharp", s)
    ids, cu = ts.calibration_batch()
    stats = ts.logit_stats(w, s, ids, cu)
    print(f"hidden {hidden} layers {layers}: (logit std, mean max softmax) per layer {stats}")
    assert len(stats) == layers
    for sd, pmax in stats:
        assert sd >= 2.0 and 0.2 < pmax < 0.9, stats
    for sd, pmax in ts.logit_stats(ts.weights("standard", s), s, ids, cu):
        assert sd < 0.5 and pmax < 0.05
    for name, a in syn.blob_to_state_dict(w, s).items():
        if name.endswith("LayerNorm.weight"):
            assert 0.5 <= a.min() < 0.6 and 1.8 < a.max() <= 2.0, (name, a.min(), a.max())
        if name.endswith(".bias"):
            assert np.abs(a).max() > 0, name


@pytest.mark.parametrize("kind", ts.KINDS)
@pytest.mark.parametrize("hidden,layers", SHAPES)
def test_oracle_error_against_float64(hidden, layers, kind):
    """E_ref: the oracle's last hidden state and pooled embedding against float64.  fp32 arithmetic alone costs a few
    1e-7 per-row rms on hidden states of rms ~1 (a few hundred roundings of 6e-8, added in quadrature, per layer); the
    assertions only pin that scale (within 1e-5 rms, pooled within 1e-6) - the GPU bound uses the measured value."""
    s, w, m = _model(kind, hidden, layers)
    ids, cu = packed([5, 33, 128, 256, 512, 1, 2, 64], 2, ts.VOCAB)
    want_h, want_e = m.encode(ids, cu)
    emb, hid = oracle.encode(w, oracle.cfg_for(s), ids, cu, return_hidden=True)
    e_rms, e_abs = ts.row_errors(hid, want_h)
    e_emb = float(np.abs(emb - want_e).max())
    print(f"hidden {hidden} layers {layers} {kind}: oracle vs float64 row rms {e_rms:.3e} max abs {e_abs:.3e}, "
          f"pooled max abs {e_emb:.3e}; max |h| {np.abs(want_h).max():.1f}, rms {np.sqrt((want_h ** 2).mean()):.2f}")
    assert 0 < e_rms < 1e-5 and e_rms <= e_abs < 1e-4
    assert e_emb < 1e-6
    np.testing.assert_allclose(np.linalg.norm(want_e, axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("layer_of", ["first", "last"])
@pytest.mark.parametrize("fault", sorted(f64.FAULTS))
@pytest.mark.parametrize("hidden,layers", [(384, 6), (768, 2)])
def test_every_fault_clears_twice_the_gpu_bound(hidden, layers, fault, layer_of):
    """One fault in one layer, one sequence of 5 ... 512 tokens: the faulty float64 hidden state must stand at least
    2x the GPU bound (the LARGER of the two modes' margins x E_ref on the same input) from the clean one, under the
    row-rms metric, on at least one weight set - at EVERY length."""
    layer = 0 if layer_of == "first" else layers - 1
    listed = (fault, "first layer of several") in UNDETECTED and layer_of == "first"
    best = {}
    for kind in ts.KINDS:
        s, w, m = _model(kind, hidden, layers)
        margin = max(ts.MARGINS[(mode, hidden, kind)][0] for mode in ("f32", "f16x3"))
        for n in FAULT_LENS:
            ids, cu, clean, e_ref = _clean(kind, hidden, layers, n)
            bad, _ = m.encode(ids, cu, fault=(fault, layer))
            ratio = ts.row_errors(bad, clean)[0] / (margin * e_ref)
            print(f"{fault} layer {layer} hidden {hidden} {kind} length {n}: fault / GPU bound = {ratio:.1f}")
            best[n] = max(best.get(n, 0.0), ratio)
    if listed:
        assert max(best.values()) < 2.0, f"{fault} is listed as undetectable but clears the bar: {best}"
        return
    assert min(best.values()) >= 2.0, f"{fault} in layer {layer}: fault / GPU bound per length {best}"


def test_undetected_list_is_short_and_spares_the_faults_that_matter():
    assert len(UNDETECTED) <= 2
    must = {"x_f16_before_qkv", "softmax_f16", "v_f16", "gelu_f16", "stale_last_row"}
    assert must <= set(f64.FAULTS) and not must & {name for name, _ in UNDETECTED}


def test_faults_change_only_what_they_say():
    """A fault in the last layer leaves a sequence of one token alone where it needs a neighbour (stale row, dropped
    key), and an unknown fault name is refused."""
    s, w, m = _model("sharp", 384, 1)
    ids, cu = packed([1, 7], 3, ts.VOCAB)
    clean, _ = m.encode(ids, cu)
    for fault in ("stale_last_row", "drop_last_key"):
        bad, _ = m.encode(ids, cu, fault=(fault, 0))
        np.testing.assert_array_equal(bad[0], clean[0])
        assert np.abs(bad[1:] - clean[1:]).max() > 1e-4
    bad, _ = m.encode(ids, cu, fault=("stale_last_row", 0))
    np.testing.assert_array_equal(bad[1:7], clean[1:7])  # every row but the sequence's last
    with pytest.raises(ValueError):
        m.encode(ids, cu, fault=("no_such_fault", 0))


def test_encode_ex_validates_arguments_without_a_gpu():
    """icrec_encode_ex refuses NULL handles and a misaligned tokens_out before it touches a device."""
    from instacart_next_order_recommendation_amd import _native

    L = _native.lib()
    assert L.icrec_encode_ex(None, None, None, 1, 1, 1, None, None, None, 0, None) == -1
    assert b"NULL" in L.icrec_last_error()
