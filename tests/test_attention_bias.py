"""The relative-position attention bias without a GPU: the ABI's NULL-handle answers, the MPNet bucket function against
transformers, a synthetic MPNet model directory against transformers.MPNetModel in float64, the native tokenizer with
MPNet's special tokens against the Rust one, and the proof that the float64 reference (oracle/float64_reference.py) would
notice a mirrored, shifted or head-rotated table."""
from __future__ import annotations

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import relative_bias as rb
from instacart_next_order_recommendation_amd import synthetic as syn
from oracle import float64_reference as f64
from tests import relative_bias as tb
from tests import token_states as ts
from tests.encoder_harness import packed
from tests.test_tokenizer import CASES


@pytest.fixture(scope="module")
def lib():
    from instacart_next_order_recommendation_amd import _native

    if not _native.LIB_PATH.exists():
        _native.build()
    return _native.lib()


def test_null_handle(lib):
    t = np.zeros((12, tb.N_OFFSETS), np.float32)
    assert lib.icrec_encoder_set_attention_bias(None, t.ctypes.data, 12) == -1  # ICREC_EINVAL
    assert b"icrec_encoder_set_attention_bias" in lib.icrec_last_error() and b"NULL" in lib.icrec_last_error()
    assert lib.icrec_encoder_set_attention_bias(None, None, 0) == -1
    assert lib.icrec_encoder_has_attention_bias(None) == -1


def test_bucket_function_equals_transformers_at_every_offset():
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder

    off = np.arange(-rb.MAX_OFFSET, rb.MAX_OFFSET + 1)
    want = MPNetEncoder.relative_position_bucket(torch.from_numpy(off)).numpy()
    got = rb.relative_position_bucket(off)
    np.testing.assert_array_equal(got, want)
    assert got.min() == 0 and got.max() == rb.NUM_BUCKETS - 1
    # as compute_position_bias uses it: a [query, key] grid of key - query
    grid = off[rb.MAX_OFFSET:][None, :] - off[rb.MAX_OFFSET:][:, None]
    np.testing.assert_array_equal(rb.relative_position_bucket(grid),
                                  MPNetEncoder.relative_position_bucket(torch.from_numpy(grid)).numpy())
    w = tb.bucket_weight(12)
    t = rb.table_from_buckets(w)
    assert t.shape == (12, tb.N_OFFSETS) and t.dtype == np.float32
    np.testing.assert_array_equal(t[:, rb.MAX_OFFSET + 3], w[got[rb.MAX_OFFSET + 3]])
    np.testing.assert_array_equal(t[5], w[want, 5])


@pytest.mark.parametrize("hidden", [768, 384])
def test_synthetic_mpnet_dir_against_transformers(tmp_path, hidden):
    """write_synthetic_model_dir(architecture="mpnet") -> load_model_dir -> the float64 helper, against
    MPNetModel.from_pretrained of the same directory in float64 on a right-padded batch: two float64 evaluations of one
    formula (3e-16 measured at hidden 128; the bound is 1e-10)."""
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    from instacart_next_order_recommendation_amd.model_io import load_model_dir, synthetic_mpnet_vocab, write_synthetic_model_dir

    n_vocab = len(synthetic_mpnet_vocab())
    shape = syn.BertShape(vocab_size=n_vocab, layers=2, type_vocab=1, ln_eps=1e-5, **ts.WIDTHS[hidden])
    d = write_synthetic_model_dir(tmp_path / "mpnet", seed=4, shape=shape, architecture="mpnet")
    m = load_model_dir(d)
    assert m.shape == shape and m.shape.max_position == 512 and m.shape.ln_eps == 1e-5
    assert m.attention_bias is not None and m.attention_bias.shape == (12, tb.N_OFFSETS)
    assert m.max_seq_length == 256 and m.pooling == "mean"
    lens = [200, 1, 37, 140, 512]
    rng = np.random.default_rng(5)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.integers(4, n_vocab, int(cu[-1])).astype(np.int32)  # (no <pad>: transformers counts positions by it)
    got, _ = f64.encode(m.weights, m.shape, ids, cu, attention_bias=m.attention_bias)

    model = tr.MPNetModel.from_pretrained(str(d), torch_dtype=torch.float64).double().eval()
    padded = np.ones((len(lens), max(lens)), np.int64)  # pad_token_id 1
    mask = np.zeros_like(padded)
    for i, n in enumerate(lens):
        padded[i, :n] = ids[cu[i]:cu[i + 1]]
        mask[i, :n] = 1
    with torch.no_grad():
        out = model(input_ids=torch.from_numpy(padded), attention_mask=torch.from_numpy(mask)).last_hidden_state.numpy()
    want = np.concatenate([out[i, :n] for i, n in enumerate(lens)])
    err = float(np.abs(got - want).max())
    print(f"synthetic MPNet directory, hidden {hidden}: max |helper - transformers| = {err:.2e}")
    assert err < 1e-10
    # the bias is not a no-op in this model
    plain, _ = f64.encode(m.weights, m.shape, ids, cu)
    assert np.abs(plain - want).max() > 1e-3


def test_other_model_types_are_refused_by_name(tmp_path):
    import json

    from instacart_next_order_recommendation_amd.model_io import load_model_dir, write_synthetic_model_dir

    d = write_synthetic_model_dir(tmp_path / "m", shape=syn.BertShape(vocab_size=len(syn.synthetic_vocab()), layers=1))
    cfg = json.loads((d / "config.json").read_text())
    for other in ("roberta", "distilbert", "xlm-roberta"):
        (d / "config.json").write_text(json.dumps({**cfg, "model_type": other}))
        with pytest.raises(ValueError, match=other):
            load_model_dir(d)


def test_native_tokenizer_with_mpnet_specials(tmp_path, lib):
    """The native tokenizer created with MPNet's special-token names agrees with the Rust BertWordPieceTokenizer built
    with the same names, on tests/test_tokenizer.py's corpus and on texts that spell the specials out."""
    from tokenizers.implementations import BertWordPieceTokenizer

    from instacart_next_order_recommendation_amd.model_io import (BERT_SPECIALS, HostTokenizer, special_tokens,
                                                                  write_synthetic_model_dir)

    d = write_synthetic_model_dir(tmp_path / "mpnet", architecture="mpnet",
                                  shape=syn.BertShape(vocab_size=2048, layers=1, type_vocab=1, ln_eps=1e-5))
    sp = special_tokens(d)
    assert sp == {"cls_token": "<s>", "sep_token": "</s>", "unk_token": "<unk>", "pad_token": "<pad>", "mask_token": "<mask>"}
    assert special_tokens(tmp_path) == BERT_SPECIALS
    rust = BertWordPieceTokenizer(str(d / "vocab.txt"), lowercase=True, **sp)._tokenizer
    rust.enable_truncation(max_length=256)
    texts = CASES + ["<s> literal </s> specials <mask> <pad> <unk> <S> </S>", "a<s>b</s>c", "< s > <mask", "milk " * 400]
    texts += syn.synthetic_user_contexts(100, seed=3)
    tok = HostTokenizer(d, 256)
    assert tok.backend == "native"
    got = tok(texts)
    want = [e.ids for e in rust.encode_batch(texts)]
    for t, a, b in zip(texts, got, want):
        assert a == b, (t, a, b)
    vocab = (d / "vocab.txt").read_text().split("\n")
    cls, sep, unk = vocab.index("<s>"), vocab.index("</s>"), vocab.index("<unk>")
    assert (cls, vocab.index("<pad>"), sep, unk) == (0, 1, 2, 3)
    assert tok([""]) == [[cls, sep]] and tok(["<unk>"]) == [[cls, unk, sep]]
    assert len(got[-101]) == 256 and got[-101][0] == cls and got[-101][-1] == sep
    assert HostTokenizer(d, 256, backend="tokenizers")(texts) == got


SENSITIVITY_LENS = [33, 128, 300]


@pytest.mark.parametrize("kind", ts.KINDS)
def test_float64_helper_notices_a_wrong_table(kind):
    """With the dense table mirrored (offset -> -offset), shifted by one offset or rotated by one head, the float64
    helper's token states leave the truth by at least 10x the bound a GPU result must meet (margin x the float32 E_ref),
    on every one of the lengths 33 / 128 / 300: a kernel that indexes the table wrongly cannot pass."""
    import torch

    s = ts.shape(384, 1)
    w = ts.weights(kind, s)
    t = tb.table("dense", s.heads)
    wrong = {"mirrored": np.ascontiguousarray(t[:, ::-1]), "shifted_by_one": np.roll(t, 1, axis=1),
             "rotated_by_one_head": np.roll(t, 1, axis=0)}
    margin = max(max(ts.TOKEN_MARGINS[(mode, 384, kind)]) for mode in ("f32", "f16x3"))
    for n in SENSITIVITY_LENS:
        ids, cu = packed([n], 40 + n, ts.VOCAB)
        h64, _ = f64.encode(w, s, ids, cu, attention_bias=t)
        h32, _ = f64.encode(w, s, ids, cu, dtype=torch.float32, attention_bias=t)
        e_rms, e_abs = ts.row_errors(h32, h64)
        for name, tw in wrong.items():
            bad, _ = f64.encode(w, s, ids, cu, attention_bias=tw)
            b_rms, b_abs = ts.row_errors(bad, h64)
            print(f"{kind} length {n} {name}: rms {b_rms:.3e} = {b_rms / (margin * e_rms):.0f} x bound, "
                  f"abs {b_abs:.3e} = {b_abs / (margin * e_abs):.0f} x bound")
            assert b_rms >= 10 * margin * e_rms and b_abs >= 10 * margin * e_abs, (kind, n, name)
