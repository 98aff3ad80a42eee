"""Models served at max_seq_length above 256 (up to 512, the position-embedding count of every BERT shape the
library accepts) - the host side, no GPU: the model directory's max_seq_length is honoured and the tokenizer
truncates there, the packing helper's limit, the C ABI constant, and the CPU oracle pinned against
transformers.BertModel at 257-512 tokens."""
from __future__ import annotations

import json
import logging
import re
from pathlib import Path

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import synthetic as syn

ROOT = Path(__file__).resolve().parents[1]


def _model_dir(tmp_path, max_seq_length, shape=None):
    from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir

    d = write_synthetic_model_dir(tmp_path / f"m{max_seq_length}", seed=2, shape=shape)
    sb = d / "sentence_bert_config.json"
    sb.write_text(json.dumps({**json.loads(sb.read_text()), "max_seq_length": max_seq_length}))
    return d


def long_contexts(n, seed=3):
    """Synthetic user contexts that tokenise to ~340-800 tokens: three or four heavy users' histories (110-200
    tokens each, bench.py's text-leg settings) joined."""
    ctx = syn.synthetic_user_contexts(4 * n, seed=seed, max_items=40, min_orders=5, max_orders=8, per_order=8)
    return [" ".join(ctx[4 * i: 4 * i + 3 + i % 2]) for i in range(n)]


@pytest.mark.parametrize("n", [384, 512])
def test_model_dir_max_seq_length_is_honoured(tmp_path, n):
    from transformers import BertTokenizer

    from instacart_next_order_recommendation_amd.model_io import load_model_dir

    d = _model_dir(tmp_path, n)
    m = load_model_dir(d)
    assert m.max_seq_length == n and m.tokenizer.max_seq_length == n
    long = m.tokenizer(["milk " * 1000])[0]
    assert len(long) == n and long[0] == 101 and long[-1] == 102  # truncation keeps [CLS] ... [SEP]
    ref = BertTokenizer(str(d / "vocab.txt"), do_lower_case=True)
    texts = long_contexts(12)
    got = m.tokenizer(texts)
    assert max(len(s) for s in got) == n and min(len(s) for s in got) > 256  # both sides of the limit exercised
    for text, ids in zip(texts, got):
        assert ids == ref(text, truncation=True, max_length=n)["input_ids"]
    ids, cu = m.tokenizer.packed(texts)  # the packed form the serving path feeds the encoder
    assert [ids[cu[i]:cu[i + 1]].tolist() for i in range(len(texts))] == got


def test_model_dir_max_seq_length_is_capped_with_a_warning(tmp_path, caplog):
    from instacart_next_order_recommendation_amd.model_io import load_model_dir

    with caplog.at_level(logging.WARNING, logger="instacart_next_order_recommendation_amd.model_io"):
        m = load_model_dir(_model_dir(tmp_path, 1000))
    assert m.max_seq_length == 512
    assert len(m.tokenizer(["milk " * 1000])[0]) == 512
    warned = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "1000" in warned[0].getMessage() and "512" in warned[0].getMessage()


def test_model_dir_max_seq_length_is_capped_at_max_position(tmp_path, caplog):
    from instacart_next_order_recommendation_amd.model_io import load_model_dir

    shape = syn.BertShape(vocab_size=len(syn.synthetic_vocab()), max_position=300)
    with caplog.at_level(logging.WARNING, logger="instacart_next_order_recommendation_amd.model_io"):
        m = load_model_dir(_model_dir(tmp_path, 512, shape))
    assert m.max_seq_length == 300 and len(m.tokenizer(["milk " * 1000])[0]) == 300
    assert any("300" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING)
    # a request under both limits is taken as it is, silently
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="instacart_next_order_recommendation_amd.model_io"):
        assert load_model_dir(_model_dir(tmp_path, 280, shape)).max_seq_length == 280
    assert not [r for r in caplog.records if r.levelno == logging.WARNING]


def test_default_max_seq_length_is_still_256(tmp_path):
    from instacart_next_order_recommendation_amd.model_io import load_model_dir, write_synthetic_model_dir

    d = write_synthetic_model_dir(tmp_path / "m", seed=2)
    (d / "sentence_bert_config.json").unlink()
    assert load_model_dir(d).max_seq_length == 256


def test_pack_token_ids_limit():
    from instacart_next_order_recommendation_amd.encoder import pack_token_ids

    ids, cu, mx = pack_token_ids([[7] * 512, [1, 2]], max_len=512)
    assert mx == 512 and cu.tolist() == [0, 512, 514] and ids.size == 514
    with pytest.raises(ValueError):
        pack_token_ids([[7] * 513], max_len=512)
    with pytest.raises(ValueError):
        pack_token_ids([[7] * 257])  # the default limit stays 256
    assert pack_token_ids([[7] * 256])[2] == 256


def test_max_seqlen_constant_matches_header():
    from instacart_next_order_recommendation_amd import _native, encoder

    header = (ROOT / "include" / "icrec.h").read_text()
    m = re.search(r"#define\s+ICREC_MAX_SEQLEN\s+(\d+)", header)
    assert m and int(m.group(1)) == 512 == _native.ICREC_MAX_SEQLEN == encoder.MAX_SEQ_LEN_LIMIT
    assert "icrec_encoder_set_max_seqlen" in _native.EXPORTS


def test_oracle_matches_transformers_past_256_tokens(minilm_weights):
    """The CPU oracle (the GPU tests' yardstick) has no length limit of its own: against transformers.BertModel at
    257, 300, 384 and 512 tokens."""
    from oracle import oracle
    from oracle.pin_against_libs import hf_encode

    lens = [257, 300, 384, 512]
    rng = np.random.default_rng(257)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.integers(0, 30522, int(cu[-1])).astype(np.int32)
    want, _ = hf_encode(minilm_weights, syn.BertShape(), ids, cu)
    got = oracle.encode(minilm_weights, oracle.make_cfg(), ids, cu)
    err = float(np.abs(got - want).max())
    print(f"oracle vs transformers at {lens} tokens: max|d emb| = {err:.3e}")
    assert err < 1e-6
