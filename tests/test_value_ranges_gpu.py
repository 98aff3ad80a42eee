"""Per-token hidden states of the HIP encoder against the float64 reference at the value ranges of a trained checkpoint:
the "heavy" weight set (near-one-hot attention, a fifth and more of the pre-GELU values beyond |u| = 3, 2 % and more
beyond the f16x3 GELU's clamp at 5.75) in every dispatch form and at every attention bucket edge, and the pointwise GELU
probes (every token's pre-GELU vector is a fixed sweep over [-8, 8] with the clamp's fp32 neighbours, signed zeros and
values whose square underflows, or +-10 / +-30 / +-100) in the small and the batch form of the FFN.

The bound is `margin x E_ref` as in tests/test_token_states_gpu.py, with the margins of ts.RANGE_MARGINS (chosen in
profiles/token_state_errors.md, "Value ranges"); tests/test_value_ranges.py shows on the CPU which mistakes that bound
catches.  Every comparison prints `RATIO ...` before it asserts."""
from __future__ import annotations

import numpy as np
import pytest

from tests import token_states as ts
from tests.encoder_harness import make_encoder, poisoned_runs, run
from tests.test_token_states_gpu import EDGE_LENS, MIXED_LENS, MODES, _batch_lens, _check

pytestmark = pytest.mark.gpu

PROBE_LENS = [5, 33]
# the batch form of the probes: more than 3,584 + 512 tokens; every token has the same pre-GELU vector, so 17 sequences
# of 256 tokens do
PROBE_BATCH_LENS = [256] * 17


def _check_range(what, mode, r, emb, tok, first_seq=0, n_seqs=None):
    _check(what, mode, r, emb, tok, first_seq, n_seqs, margin=ts.range_margin(mode, r["s"].hidden, r["kind"]))


@pytest.mark.parametrize("hidden,layers", [(384, 6), (384, 1), (768, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_heavy_small_batch_every_width(monkeypatch, mode, hidden, layers):
    """The 8 sequences of test_small_batch_every_width on the heavy set: the small / latency forms, whose FFN-up
    epilogue applies the GELU; f16x3 also under ICREC_FUSE=0."""
    r = ts.reference("heavy", hidden, layers, MIXED_LENS, seed=2)
    for env in ({}, {"ICREC_FUSE": 0}) if mode == "f16x3" else ({},):
        enc = make_encoder(monkeypatch, r["w"], r["s"], mode, **env)
        emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
        _check_range(f"small {env}", mode, r, emb, tok)
        enc.close()


@pytest.mark.parametrize("hidden", [384, 768])
@pytest.mark.parametrize("mode", MODES)
def test_heavy_attention_bucket_edges(monkeypatch, mode, hidden):
    """Ceiling 512, 2 layers: a sequence on each side of every key-tile bucket edge, in one batch and each alone, so
    that every attention kernel - the forms that recompute the scores and the masked last key tile among them - sees
    rows where one key carries all the weight and most probabilities underflow."""
    r = ts.reference("heavy", hidden, 2, EDGE_LENS, seed=5)
    enc = make_encoder(monkeypatch, r["w"], r["s"], mode, max_seq_length=512)
    emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
    _check_range("edges mixed", mode, r, emb, tok)
    cu = r["cu"]
    for i, n in enumerate(EDGE_LENS):
        a, b = int(cu[i]), int(cu[i + 1])
        e1, t1 = run(enc, r["ids"][a:b].copy(), np.array([0, n], np.int32), return_tokens=True)
        _check_range(f"length {n} alone", mode, r, e1, t1, i, 1)
    enc.close()


@pytest.mark.parametrize("hidden", [384, 768])
def test_heavy_batch_forms(monkeypatch, hidden):
    """The 60 sequences (> 3,584 + 512 tokens, 2 layers) of test_batch_forms on the heavy set.  Hidden 384: the fused FFN
    kernel, whose software-pipelined producer applies the GELU, the unfused chain and f32.  Hidden 768: the slab-ring
    form, also forced on the batch's first <= 1,500 tokens with ICREC_SMALL_M=512, beside their latency form."""
    r = ts.reference("heavy", hidden, 2, _batch_lens(60, seed=33), seed=3)
    assert r["cu"][-1] > 3584 + 512
    for mode, env in (("f32", {}), ("f16x3", {}), ("f16x3", {"ICREC_FUSE": 0})):
        enc = make_encoder(monkeypatch, r["w"], r["s"], mode, **env)
        emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
        _check_range(f"batch {env}", mode, r, emb, tok)
        enc.close()
    if hidden == 768:
        n = int(np.searchsorted(r["cu"], 1500, side="right")) - 1
        t = int(r["cu"][n])
        assert 1000 < t <= 1500
        for env in ({}, {"ICREC_SMALL_M": 512}):
            enc = make_encoder(monkeypatch, r["w"], r["s"], "f16x3", **env)
            emb, tok = run(enc, r["ids"][:t].copy(), r["cu"][: n + 1].copy(), return_tokens=True)
            _check_range(f"first {t} tokens {env}", "f16x3", r, emb, tok, 0, n)
            enc.close()


@pytest.mark.parametrize("kind", ts.PROBE_KINDS)
@pytest.mark.parametrize("hidden", [384, 768])
def test_gelu_probes(monkeypatch, hidden, kind):
    """LN(gelu(sweep) + x) per token, both modes: [5, 33] tokens (the small form's FFN-up epilogue) and 4,352 tokens
    (the batch form: the fused FFN kernel at hidden 384, the slab ring at 768)."""
    for lens, seed in ((PROBE_LENS, 1), (PROBE_BATCH_LENS, 6)):
        r = ts.reference(kind, hidden, 1, lens, seed=seed)
        assert len(lens) == 2 or r["cu"][-1] > 3584 + 512
        for mode in MODES:
            enc = make_encoder(monkeypatch, r["w"], r["s"], mode)
            emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
            _check_range(f"{kind}, {len(lens)} sequences", mode, r, emb, tok)
            enc.close()


def test_heavy_reads_nothing_stale(monkeypatch):
    """f16x3: a workspace and a tokens_out buffer full of 0xFF, 0x00 or 0x7F give the same token bits - a probability
    that underflows is a written 0 in its planes, not a byte left over from another call."""
    r = ts.reference("heavy", 384, 2, MIXED_LENS, seed=2)
    enc = make_encoder(monkeypatch, r["w"], r["s"], "f16x3")
    emb, tok = poisoned_runs(enc, r["ids"], r["cu"], tokens=True)
    _check_range("poisoned workspace", "f16x3", r, emb, tok)
    enc.close()
