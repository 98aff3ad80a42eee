"""Per-token hidden states of the HIP encoder (DeviceEncoder.encode_packed(return_tokens=True), icrec_encode_ex) against
the float64 reference (oracle/float64_reference.py), at every width, weight set, f16x3 dispatch form and attention
bucket edge.

The bound is `margin x E_ref` (tests/token_states.py): E_ref is the fp32 C oracle's error against the same float64
hidden states on the same inputs - per-token-row rms, with a max-abs check beside it - and the margins are the ones
chosen in profiles/token_state_errors.md.  Every comparison prints `ratio rms / abs` = E_gpu / E_ref before it
asserts; on failure the worst (sequence, position, feature, got, want) is named."""
from __future__ import annotations

import numpy as np
import pytest

from tests import token_states as ts
from tests.encoder_harness import make_encoder, poisoned_runs, replay_matches_eager, round_plus_remainder, run

pytestmark = pytest.mark.gpu

MODES = ("f32", "f16x3")
# every attention bucket edge (key tiles of 32; buckets of 1 / 2 / 3-4 / 5-6 / 7-8 / 9-16 tiles)
EDGE_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225,
             255, 256, 257, 383, 384, 385, 511, 512]
MIXED_LENS = [5, 33, 128, 256, 1, 2, 64, 97]


def _check(what, mode, r, emb, tok, first_seq=0, n_seqs=None, margin=None):
    """tok (sequences [first_seq, first_seq + n_seqs) of r's batch; all by default) against the float64 hidden states
    within margin x E_ref (MARGINS' entry unless `margin` is given), and tok mean-pooled in float64 against emb."""
    s, kind = r["s"], r["kind"]
    n_seqs = r["cu"].size - 1 - first_seq if n_seqs is None else n_seqs
    cu = r["cu"][first_seq: first_seq + n_seqs + 1].astype(np.int64)
    rows = slice(int(cu[0]), int(cu[-1]))
    want, ora = r["h64"][rows], r["h32"][rows]
    cu = cu - cu[0]
    assert tok.shape == want.shape and tok.dtype == np.float32 and np.isfinite(tok).all()
    ts.check(f"token states [{what}] mode={mode} hidden={s.hidden} layers={s.layers} weights={kind} tokens={tok.shape[0]}",
             tok, want, ora, ts.MARGINS[(mode, s.hidden, kind)] if margin is None else margin, cu)
    # The embedding of the same call is the mean of these rows, normalised.  fp32 pooling sums n rows one after the
    # other: |error of the mean| <= n u mean|h| (u = 2^-24); the two normalisations (fmaf chain of H / 64, a 6-step
    # butterfly, sqrt, divide) cost at most 32 more roundings of a component that is <= 1.
    t64 = tok.astype(np.float64)
    u = 2.0 ** -24
    for i in range(cu.size - 1):
        rows_i = t64[cu[i]:cu[i + 1]]
        pooled = rows_i.mean(0)
        norm = np.linalg.norm(pooled)
        v = pooled
        for _ in range(s.n_normalize):
            v = v / max(np.linalg.norm(v), 1e-12)
        tol = rows_i.shape[0] * u * np.abs(rows_i).mean(0) / norm + 32 * u
        assert (np.abs(emb[i] - v) <= tol).all(), (what, mode, i, float(np.abs(emb[i] - v).max()), float(tol.min()))


@pytest.mark.parametrize("kind", ts.KINDS)
@pytest.mark.parametrize("hidden,layers", [(384, 6), (384, 1), (768, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_small_batch_every_width(monkeypatch, mode, hidden, layers, kind):
    """~590 tokens in 8 sequences: the small / latency forms.  6 layers and 1 layer at hidden 384 (layer 0's stand-alone
    QKV, the next-layer QKV prologue / epilogue and the last layer without one are different code), 2 layers at 768.
    f16x3 also under ICREC_FUSE=0 (separate LayerNorm launches)."""
    r = ts.reference(kind, hidden, layers, MIXED_LENS, seed=2)
    for env in ({}, {"ICREC_FUSE": 0}) if mode == "f16x3" else ({},):
        enc = make_encoder(monkeypatch, r["w"], r["s"], mode, **env)
        emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
        _check(f"small {env}", mode, r, emb, tok)
        enc.close()


def _batch_lens(n, seed):
    from instacart_next_order_recommendation_amd import synthetic as syn

    _, cu = syn.synthetic_token_batch(n, seed=seed, mean_len=90, std_len=60, lo=3, hi=256, vocab_size=ts.VOCAB)
    return np.diff(cu).tolist()


@pytest.mark.parametrize("kind", ts.KINDS)
@pytest.mark.parametrize("hidden", [384, 768])
def test_batch_forms(monkeypatch, hidden, kind):
    """60 sequences, > 3,584 tokens, 2 layers.  Hidden 384: the layer kernels (f16x3 default), the unfused slab-ring
    chain (ICREC_FUSE=0) and f32.  Hidden 768: the slab-ring form (default above 3,584 tokens, and forced on the same
    batch's first 1,500 tokens with ICREC_SMALL_M=512), the latency form of those 1,500 tokens, and f32."""
    lens = _batch_lens(60, seed=33)
    r = ts.reference(kind, hidden, 2, lens, seed=3)
    assert r["cu"][-1] > 3584 + 512
    for mode, env in (("f32", {}), ("f16x3", {}), ("f16x3", {"ICREC_FUSE": 0})):
        enc = make_encoder(monkeypatch, r["w"], r["s"], mode, **env)
        emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
        _check(f"batch {env}", mode, r, emb, tok)
        enc.close()
    if hidden == 768:
        n = int(np.searchsorted(r["cu"], 1500, side="right")) - 1
        t = int(r["cu"][n])
        assert 1000 < t <= 1500
        for env in ({}, {"ICREC_SMALL_M": 512}):
            enc = make_encoder(monkeypatch, r["w"], r["s"], "f16x3", **env)
            emb, tok = run(enc, r["ids"][:t].copy(), r["cu"][: n + 1].copy(), return_tokens=True)
            _check(f"first {t} tokens {env}", "f16x3", r, emb, tok, 0, n)
            enc.close()


@pytest.mark.parametrize("kind", ts.KINDS)
@pytest.mark.parametrize("hidden", [384, 768])
def test_rounds_plus_remainder(monkeypatch, hidden, kind):
    """f16x3, 2 layers: a token count that icrec_encode_batch_split cuts into whole rounds (64 tokens per CU) + a
    remainder, which runs through the small-batch kernels on the library's side stream."""
    lens = _batch_lens(400, seed=11)
    cu_all = np.concatenate([[0], np.cumsum(lens)])
    r = ts.reference(kind, hidden, 2, [4], seed=0)
    probe = make_encoder(monkeypatch, r["w"], r["s"], "f16x3")
    n, main_t, tail_t = round_plus_remainder(probe, cu_all, 1, np.inf, first=64)
    probe.close()
    assert tail_t and main_t > 0 and n >= 64, (main_t, tail_t, n)
    r = ts.reference(kind, hidden, 2, lens[:n], seed=4)
    enc = make_encoder(monkeypatch, r["w"], r["s"], "f16x3")
    assert enc.batch_split(int(r["cu"][-1])) == (main_t, tail_t)
    emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
    _check(f"rounds {main_t} + remainder {tail_t}", "f16x3", r, emb, tok)
    enc.close()


@pytest.mark.parametrize("kind", ts.KINDS)
@pytest.mark.parametrize("hidden,layers", [(384, 6), (768, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_attention_bucket_edges(monkeypatch, mode, hidden, layers, kind):
    """Ceiling raised to 512: a sequence on each side of every key-tile bucket edge, all in one batch, then each alone
    (a lone sequence may take another bucket's kernel than the same sequence in a batch)."""
    r = ts.reference(kind, hidden, layers, EDGE_LENS, seed=5)
    enc = make_encoder(monkeypatch, r["w"], r["s"], mode, max_seq_length=512)
    emb, tok = run(enc, r["ids"], r["cu"], return_tokens=True)
    _check("edges mixed", mode, r, emb, tok)
    cu = r["cu"]
    for i, n in enumerate(EDGE_LENS):
        a, b = int(cu[i]), int(cu[i + 1])
        e1, t1 = run(enc, r["ids"][a:b].copy(), np.array([0, n], np.int32), return_tokens=True)
        _check(f"length {n} alone", mode, r, e1, t1, i, 1)
    enc.close()


@pytest.mark.parametrize("hidden,layers", [(384, 6), (768, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_token_output_changes_nothing_and_reads_nothing_stale(monkeypatch, mode, hidden, layers):
    """The embeddings of a call that also returns tokens are those of plain encode_packed bit for bit; a workspace and a
    tokens_out buffer full of 0xFF give the same token bits as zeroed ones."""
    r = ts.reference("sharp", hidden, layers, MIXED_LENS, seed=2)
    enc = make_encoder(monkeypatch, r["w"], r["s"], mode)
    plain = run(enc, r["ids"], r["cu"])
    emb, _ = poisoned_runs(enc, r["ids"], r["cu"], fills=(0xFF, 0x00), tokens=True)
    np.testing.assert_array_equal(emb, plain)
    np.testing.assert_array_equal(run(enc, r["ids"], r["cu"]), plain)
    enc.close()


def test_token_output_under_graph_capture(monkeypatch):
    """icrec_encode_ex is capturable like icrec_encode: a replayed graph writes the same token bits as the eager call."""
    r = ts.reference("sharp", 384, 6, MIXED_LENS, seed=2)
    enc = make_encoder(monkeypatch, r["w"], r["s"], "f16x3")
    replay_matches_eager(enc, r["ids"], r["cu"], tokens=True)
    enc.close()
