"""Read (and, for tests/benchmarks, write) a SentenceTransformer model directory.

The reference loads `SentenceTransformer(str(model_dir))`
(src/inference/serve_recommendations.py:166-170) where model_dir is what
`SentenceTransformer.save` wrote after fine-tuning (src/training/train_sbert.py:139-141):
  modules.json, config.json, model.safetensors, tokenizer files,
  sentence_bert_config.json, 1_Pooling/config.json, 2_Normalize/.
Only local directories are supported (no hub download: there is no network).

Tokenisation is a host stage: the WordPiece tokenizer is built from the directory's
tokenizer.json / vocab.txt with the `tokenizers` package (the same Rust tokenizer the
reference ends up using through transformers, uv.lock:3841).
"""
from __future__ import annotations

import json
import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _native, relative_bias
from .synthetic import BertShape, blob_to_state_dict, state_dict_to_blob, synthetic_bert_weights, synthetic_vocab

logger = logging.getLogger(__name__)

DEFAULT_MAX_SEQ_LENGTH = 256  # configs/train.yaml:11; used when sentence_bert_config.json gives none


@dataclass
class LoadedModel:
    shape: BertShape
    weights: np.ndarray  # flat fp32 blob, include/icrec.h order
    max_seq_length: int
    tokenizer: "HostTokenizer"
    pooling: str = "mean"  # "mean" or "cls": the one mode 1_Pooling/config.json switches on
    attention_bias: Optional[np.ndarray] = None  # MPNet: float32 [heads, 1023] by relative offset (relative_bias.py)


#: the special tokens of a BERT vocabulary: what a directory that names none gets
BERT_SPECIALS = {"cls_token": "[CLS]", "sep_token": "[SEP]", "unk_token": "[UNK]", "pad_token": "[PAD]",
                 "mask_token": "[MASK]"}


def special_tokens(model_dir: Path) -> dict:
    """The directory's special-token names: BERT_SPECIALS overridden by tokenizer_config.json, then by
    special_tokens_map.json (an entry is a string or an AddedToken dict with "content")."""
    out = dict(BERT_SPECIALS)
    for name in ("tokenizer_config.json", "special_tokens_map.json"):
        f = Path(model_dir) / name
        if not f.exists():
            continue
        cfg = json.loads(f.read_text())
        for k in out:
            v = cfg.get(k)
            if isinstance(v, dict):
                v = v.get("content")
            if isinstance(v, str) and v:
                out[k] = v
    return out


class NativeTokenizer:
    """libicrec's C++ WordPiece tokenizer (csrc/tokenizer.cpp): batched, multi-threaded, GIL-free."""

    def __init__(self, vocab_path: Path, lowercase: bool, max_seq_length: int, n_threads: int = 0,
                 specials: Optional[dict] = None):
        """specials: the vocabulary's special-token names (keys of BERT_SPECIALS) when they are not BERT's."""
        import ctypes as C

        from . import _native

        self._C, self._native = C, _native
        h = C.c_void_p()
        if specials is None or specials == BERT_SPECIALS:
            _native.check(_native.lib().icrec_tokenizer_create(str(vocab_path).encode(), 1 if lowercase else 0,
                                                               int(max_seq_length), C.byref(h)), "icrec_tokenizer_create")
        else:
            sp = [specials[k].encode() for k in ("cls_token", "sep_token", "unk_token", "pad_token", "mask_token")]
            _native.check(_native.lib().icrec_tokenizer_create_ex(str(vocab_path).encode(), 1 if lowercase else 0,
                                                                  int(max_seq_length), *sp, C.byref(h)),
                          "icrec_tokenizer_create_ex")
        self._h, self.max_seq_length, self.n_threads = h, max_seq_length, n_threads

    def packed(self, texts: Sequence[str]) -> tuple[np.ndarray, np.ndarray]:
        """texts -> (ids int32[T], cu_seqlens int32[n+1]): the packed form icrec_encode takes, straight from
        icrec_tokenize (no per-sequence Python lists: at 1,024 contexts per batch the list round trip costs
        more host time - under the GIL - than the tokenisation itself)."""
        C = self._C
        n = len(texts)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(1, np.int32)
        arr = (C.c_char_p * n)(*[t.replace("\x00", "").encode("utf-8", "replace") for t in texts])
        cu = np.empty(n + 1, np.int32)
        cap = n * self.max_seq_length
        ids = np.empty(cap, np.int32)
        self._native.check(self._native.lib().icrec_tokenize(self._h, arr, n, ids.ctypes.data_as(C.c_void_p), cap,
                                                             cu.ctypes.data_as(C.c_void_p), self.n_threads),
                           "icrec_tokenize")
        return ids[: int(cu[n])], cu

    def __call__(self, texts: Sequence[str]) -> list[list[int]]:
        ids, cu = self.packed(texts)
        return [ids[cu[i]:cu[i + 1]].tolist() for i in range(len(texts))]

    def __del__(self):  # pragma: no cover
        try:
            self._native.lib().icrec_tokenizer_destroy(self._h)
        except Exception:
            pass


class HostTokenizer:
    """BERT WordPiece tokenisation on the host ([CLS] ... [SEP], truncation to max_seq_length); a directory whose
    tokenizer_config.json / special_tokens_map.json name other specials (MPNet: <s> ... </s>) gets those.

    backend "native" (default when the directory has vocab.txt): libicrec's C++ tokenizer, ~6x the
    throughput of the Rust one on 8 cores (68k vs 11k user contexts/s) — at >50k QPS per GPU the
    tokenizer would otherwise be the bottleneck; agrees with the Rust tokenizer on tests/test_tokenizer.py.
    backend "tokenizers" (ICREC_TOKENIZER=tokenizers, or no vocab.txt): the Rust library the reference
    itself ends up in."""

    def __init__(self, model_dir: Path, max_seq_length: int, backend: str | None = None):
        import os

        model_dir = Path(model_dir)
        tj, vt = model_dir / "tokenizer.json", model_dir / "vocab.txt"
        backend = backend or os.getenv("ICREC_TOKENIZER") or ("native" if vt.exists() else "tokenizers")
        lower = True
        tc = model_dir / "tokenizer_config.json"
        if tc.exists():
            lower = bool(json.loads(tc.read_text()).get("do_lower_case", True))
        self.max_seq_length = max_seq_length
        self.backend = backend
        self.specials = special_tokens(model_dir)
        if backend == "native":
            if not vt.exists():
                raise FileNotFoundError(f"{vt} missing: the native tokenizer needs vocab.txt")
            self._native_tok = NativeTokenizer(vt, lower, max_seq_length, specials=self.specials)
            return
        if backend != "tokenizers":
            raise ValueError(f"unknown tokenizer backend {backend!r}")
        from tokenizers import Tokenizer
        from tokenizers.implementations import BertWordPieceTokenizer

        if tj.exists():
            self._tok = Tokenizer.from_file(str(tj))
        elif vt.exists():
            self._tok = BertWordPieceTokenizer(str(vt), lowercase=lower, **self.specials)._tokenizer
        else:
            raise FileNotFoundError(f"{model_dir} has neither tokenizer.json nor vocab.txt")
        self._tok.no_padding()
        self._tok.enable_truncation(max_length=max_seq_length)

    def __call__(self, texts: Sequence[str]) -> list[list[int]]:
        if self.backend == "native":
            return self._native_tok(texts)
        return [e.ids for e in self._tok.encode_batch(list(texts))]

    def packed(self, texts: Sequence[str]) -> tuple[np.ndarray, np.ndarray]:
        """(ids int32[T], cu_seqlens int32[n+1]) - see NativeTokenizer.packed."""
        if self.backend == "native":
            return self._native_tok.packed(texts)
        seqs = self(texts)
        cu = np.zeros(len(seqs) + 1, np.int32)
        np.cumsum([len(s) for s in seqs], out=cu[1:])
        ids = np.concatenate([np.asarray(s, np.int32) for s in seqs]) if seqs else np.zeros(0, np.int32)
        return ids, cu


def load_model_dir(model_dir: Path | str) -> LoadedModel:
    """Parse config + weights + tokenizer of a local SentenceTransformer directory."""
    from safetensors.numpy import load_file

    d = Path(model_dir)
    if not d.is_dir():
        raise FileNotFoundError(
            f"model_dir {model_dir!r} is not a local directory (hub ids cannot be fetched: no network)")
    cfg = json.loads((d / "config.json").read_text())
    model_type = cfg.get("model_type", "bert")
    if model_type not in ("bert", "mpnet"):
        raise ValueError(f"unsupported model_type {model_type!r}: this encoder serves BERT and MPNet models "
                         "(RoBERTa, DistilBERT and the other families name and arrange their weights differently)")
    mpnet = model_type == "mpnet"
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"unsupported hidden_act {cfg.get('hidden_act')!r} (kernels implement erf-GELU)")
    n_norm = 1  # encode(..., normalize_embeddings=True) at every reference call site
    pooling = "mean"  # sentence-transformers' default when the directory names no mode
    mj = d / "modules.json"
    if mj.exists():
        for m in json.loads(mj.read_text()):
            t = m.get("type", "")
            if t.endswith("Normalize"):
                n_norm += 1
            if t.endswith("Pooling"):
                pc = d / m.get("path", "1_Pooling") / "config.json"
                if pc.exists():
                    p = json.loads(pc.read_text())
                    # exactly one of mean / cls: the other modes (max, mean-sqrt-len, weighted mean, last token) are
                    # not implemented, and any combination of modes widens the output
                    on = {"pooling_mode_mean_tokens": bool(p.get("pooling_mode_mean_tokens", True))}
                    on.update({k: bool(v) for k, v in p.items() if k.startswith("pooling_mode_") and k not in on})
                    chosen = [k for k, v in on.items() if v]
                    served = {"pooling_mode_mean_tokens": "mean", "pooling_mode_cls_token": "cls"}
                    if len(chosen) != 1 or chosen[0] not in served:
                        raise ValueError(f"only mean-token or CLS-token pooling, one of the two, is implemented (got {p})")
                    pooling = served[chosen[0]]
    # MPNet: position ids start at padding_idx + 1 = 2 (rows 0 and 1 of the table are never read: max_position is two
    # less), and there is no token-type table (one zero row stands in)
    shape = BertShape(vocab_size=int(cfg["vocab_size"]), hidden=int(cfg["hidden_size"]),
                      layers=int(cfg["num_hidden_layers"]), heads=int(cfg["num_attention_heads"]),
                      intermediate=int(cfg["intermediate_size"]),
                      max_position=int(cfg["max_position_embeddings"]) - (2 if mpnet else 0),
                      type_vocab=1 if mpnet else int(cfg.get("type_vocab_size", 2)),
                      ln_eps=float(cfg.get("layer_norm_eps", 1e-12)), n_normalize=n_norm)
    st = d / "model.safetensors"
    if not st.exists():
        raise FileNotFoundError(f"{st} missing (pytorch_model.bin pickles are not loaded: only safetensors)")
    sd = load_file(str(st))
    attention_bias = None
    if mpnet:
        if int(cfg.get("pad_token_id", 1)) != 1:
            raise ValueError(f"MPNet with pad_token_id {cfg.get('pad_token_id')}: position ids are taken to start at 2")
        sd, buckets = mpnet_to_bert_state_dict(sd, shape)
        n_buckets = int(cfg.get("relative_attention_num_buckets", relative_bias.NUM_BUCKETS))
        # (transformers buckets offsets into 32 whatever the config says: a table of another size is not an MPNet)
        if buckets.shape != (n_buckets, shape.heads) or n_buckets != relative_bias.NUM_BUCKETS:
            raise ValueError(f"relative_attention_bias.weight is {buckets.shape}, expected "
                             f"({relative_bias.NUM_BUCKETS}, {shape.heads}) (relative_attention_num_buckets={n_buckets})")
        attention_bias = relative_bias.table_from_buckets(buckets)
    weights = state_dict_to_blob(sd, shape)
    max_len = DEFAULT_MAX_SEQ_LENGTH
    sb = d / "sentence_bert_config.json"
    if sb.exists():
        max_len = int(json.loads(sb.read_text()).get("max_seq_length") or max_len)
    # the encoder takes up to ICREC_MAX_SEQLEN (512) tokens, and never more than the model has positions
    limit = min(_native.ICREC_MAX_SEQLEN, shape.max_position)
    if max_len > limit:
        logger.warning("%s asks for max_seq_length %d; this encoder serves at most %d tokens for it: using %d",
                       d, max_len, limit, limit)
        max_len = limit
    return LoadedModel(shape, weights, max_len, HostTokenizer(d, max_len), pooling, attention_bias)


#: MPNet's names of a layer's tensors -> BertModel's (the layer itself is a BERT layer: relative_bias.py has the one
#: term that differs)
_MPNET_TO_BERT = {"attention.attn.q": "attention.self.query", "attention.attn.k": "attention.self.key",
                  "attention.attn.v": "attention.self.value", "attention.attn.o": "attention.output.dense",
                  "attention.LayerNorm": "attention.output.LayerNorm"}


def mpnet_to_bert_state_dict(sd: dict, shape: BertShape) -> tuple[dict, np.ndarray]:
    """An MPNetModel state dict (optional 'mpnet.' prefix) -> (the BertModel-named dict state_dict_to_blob takes, the
    [num_buckets, heads] relative-attention table).  `shape` is the BERT view: max_position two less than the table."""
    sd = {(k[len("mpnet."):] if k.startswith("mpnet.") else k): np.asarray(v) for k, v in sd.items()}
    out = {}
    for k, v in sd.items():
        for a, b in _MPNET_TO_BERT.items():
            if f".{a}." in k:
                k = k.replace(f".{a}.", f".{b}.")
                break
        out[k] = v
    out["embeddings.position_embeddings.weight"] = sd["embeddings.position_embeddings.weight"][2:]
    out["embeddings.token_type_embeddings.weight"] = np.zeros((1, shape.hidden), np.float32)
    return out, np.asarray(out.pop("encoder.relative_attention_bias.weight"), np.float32)


def bert_to_mpnet_state_dict(sd: dict, buckets: np.ndarray, seed: int) -> dict:
    """The inverse, for write_synthetic_model_dir: MPNet names, no token-type table, two seeded rows (never read) in front
    of the position table, the bucket table added."""
    from .synthetic import normalish

    out = {}
    for k, v in sd.items():
        for a, b in _MPNET_TO_BERT.items():
            if f".{b}." in k:
                k = k.replace(f".{b}.", f".{a}.")
                break
        out[k] = v
    del out["embeddings.token_type_embeddings.weight"]
    pos = out["embeddings.position_embeddings.weight"]
    head = normalish(seed, 9_001, 2 * pos.shape[1], 0.05).reshape(2, pos.shape[1])
    out["embeddings.position_embeddings.weight"] = np.concatenate([head, pos]).astype(np.float32)
    out["encoder.relative_attention_bias.weight"] = np.asarray(buckets, np.float32)
    return out


def synthetic_mpnet_vocab() -> list[str]:
    """synthetic_vocab() with MPNet's specials: <s>=0 <pad>=1 </s>=2 <unk>=3 in front, <mask> last, the BERT specials'
    slots filled with unused entries so that every ordinary token keeps its id."""
    v = synthetic_vocab()
    for i, tok in enumerate(v):
        if tok in BERT_SPECIALS.values():
            v[i] = f"[unused_{i}]"
    v[:4] = ["<s>", "<pad>", "</s>", "<unk>"]
    return v + ["<mask>"]


def write_synthetic_model_dir(path: Path | str, seed: int = 0, shape: BertShape | None = None,
                              pooling: str = "mean", architecture: str = "bert") -> Path:
    """Write a SentenceTransformer-layout directory with seeded random weights and the synthetic
    WordPiece vocab (stand-in for the fine-tuned all-MiniLM-L6-v2 that cannot be downloaded here).
    pooling: "mean" or "cls", what 1_Pooling/config.json switches on (all-MiniLM: mean; the BGE family: cls).
    architecture: "bert", or "mpnet" (all-mpnet-base-v2's layout): MPNet-named tensors with a [32, heads] relative-attention
    table uniform in [-4, 4], an MPNet config.json and the vocab with MPNet's specials.  `shape` is then the BERT view
    load_model_dir gives back - type_vocab 1, max_position two less than the written position table, ln_eps 1e-5 - and
    by default BertShape(vocab_size=len(vocab), type_vocab=1, ln_eps=1e-5) at MiniLM's sizes."""
    from safetensors.numpy import save_file

    if pooling not in ("mean", "cls"):
        raise ValueError(f"pooling must be 'mean' or 'cls', got {pooling!r}")
    if architecture not in ("bert", "mpnet"):
        raise ValueError(f"architecture must be 'bert' or 'mpnet', got {architecture!r}")
    mpnet = architecture == "mpnet"
    d = Path(path)
    d.mkdir(parents=True, exist_ok=True)
    vocab = synthetic_mpnet_vocab() if mpnet else synthetic_vocab()
    if shape is None:
        shape = BertShape(vocab_size=len(vocab), type_vocab=1, ln_eps=1e-5) if mpnet else BertShape(vocab_size=len(vocab))
    if shape.vocab_size < len(vocab):
        raise ValueError("shape.vocab_size smaller than the synthetic vocab")
    if mpnet and shape.type_vocab != 1:
        raise ValueError("an MPNet has no token-type table: shape.type_vocab must be 1")
    blob = synthetic_bert_weights(shape, seed=seed)
    sd = blob_to_state_dict(blob, shape)
    config = {"vocab_size": shape.vocab_size, "hidden_size": shape.hidden, "num_hidden_layers": shape.layers,
              "num_attention_heads": shape.heads, "intermediate_size": shape.intermediate, "hidden_act": "gelu",
              "layer_norm_eps": shape.ln_eps}
    if mpnet:
        from .synthetic import uniform

        buckets = (8.0 * uniform(seed, 9_000, relative_bias.NUM_BUCKETS * shape.heads) - 4.0).astype(np.float32)
        sd = bert_to_mpnet_state_dict(sd, buckets.reshape(relative_bias.NUM_BUCKETS, shape.heads), seed)
        config.update({"architectures": ["MPNetModel"], "model_type": "mpnet",
                       "max_position_embeddings": shape.max_position + 2,
                       "relative_attention_num_buckets": relative_bias.NUM_BUCKETS,
                       "pad_token_id": 1, "bos_token_id": 0, "eos_token_id": 2})
        tok_cfg = {"do_lower_case": True, "tokenizer_class": "MPNetTokenizer", "bos_token": "<s>", "eos_token": "</s>",
                   "cls_token": "<s>", "sep_token": "</s>", "unk_token": "<unk>", "pad_token": "<pad>",
                   "mask_token": "<mask>"}
        (d / "special_tokens_map.json").write_text(json.dumps({k: v for k, v in tok_cfg.items() if k.endswith("_token")}))
    else:
        config.update({"architectures": ["BertModel"], "model_type": "bert",
                       "max_position_embeddings": shape.max_position, "type_vocab_size": shape.type_vocab})
        tok_cfg = {"do_lower_case": True, "tokenizer_class": "BertTokenizer"}
    save_file({k: np.ascontiguousarray(v) for k, v in sd.items()}, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps(config, indent=2))
    (d / "vocab.txt").write_text("\n".join(vocab) + "\n")
    (d / "tokenizer_config.json").write_text(json.dumps(tok_cfg))
    (d / "sentence_bert_config.json").write_text(json.dumps({"max_seq_length": 256, "do_lower_case": False}))
    (d / "modules.json").write_text(json.dumps([
        {"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
        {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
        {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}], indent=2))
    (d / "1_Pooling").mkdir(exist_ok=True)
    (d / "1_Pooling" / "config.json").write_text(json.dumps({
        "word_embedding_dimension": shape.hidden, "pooling_mode_cls_token": pooling == "cls",
        "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False}))
    (d / "2_Normalize").mkdir(exist_ok=True)
    return d


# --------------------------------------------------------------------------- cross-encoders (reranker.py)
#: A side of a pair is tokenised on its own and keeps up to this many tokens before the pair is assembled and truncated
#: (assemble_pairs): the pair's truncation needs the sides' real lengths, and no side of up to 2,048 tokens is cut early.
SIDE_MAX_TOKENS = 2048


@dataclass
class LoadedCrossEncoder:
    """A BertForSequenceClassification(num_labels=1) directory: the encoder's blob, and the score head beside it."""

    shape: BertShape
    weights: np.ndarray   # flat fp32 blob, include/icrec.h order (the head is not part of it)
    pooler_w: np.ndarray  # float32 [hidden, hidden], [out, in]
    pooler_b: np.ndarray  # float32 [hidden]
    cls_w: np.ndarray     # float32 [hidden]
    cls_b: np.ndarray     # float32 [1]
    max_seq_length: int
    tokenizer: HostTokenizer  # tokenises ONE side ([CLS] side [SEP], cut at SIDE_MAX_TOKENS only: strip_specials)
    activation: str       # "sigmoid" or "identity": what CrossEncoder.predict applies to the logit


def load_cross_encoder_dir(model_dir: Path | str) -> LoadedCrossEncoder:
    """Parse a local cross-encoder directory (the cross-encoder/ms-marco-MiniLM-L-*-v2 layout: config.json of a
    BertForSequenceClassification with one label, model.safetensors with bert.embeddings.* / bert.encoder.* /
    bert.pooler.dense.* / classifier.*, the tokenizer files).  Anything else raises ValueError naming the field."""
    from safetensors.numpy import load_file

    d = Path(model_dir)
    if not d.is_dir():
        raise FileNotFoundError(
            f"model_dir {model_dir!r} is not a local directory (hub ids cannot be fetched: no network)")
    cfg = json.loads((d / "config.json").read_text())
    if cfg.get("model_type", "bert") != "bert":
        raise ValueError(f"unsupported model_type {cfg.get('model_type')!r}: the reranker serves BERT cross-encoders")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"unsupported hidden_act {cfg.get('hidden_act')!r} (kernels implement erf-GELU)")
    n_labels = len(cfg["id2label"]) if "id2label" in cfg else int(cfg.get("num_labels", 2))
    if "num_labels" in cfg and int(cfg["num_labels"]) != n_labels:
        raise ValueError(f"num_labels {cfg['num_labels']} contradicts id2label of size {n_labels}")
    if n_labels != 1:
        raise ValueError(f"num_labels / id2label of size {n_labels}: only single-logit cross-encoders (num_labels = 1) are served")
    if int(cfg.get("type_vocab_size", 2)) < 2:
        raise ValueError(f"type_vocab_size {cfg.get('type_vocab_size')}: a pair needs two token-type rows")
    act = str(cfg.get("sbert_ce_default_activation_function") or "torch.nn.modules.activation.Sigmoid")
    if not act.endswith(("Sigmoid", "Identity")):
        raise ValueError(f"unsupported sbert_ce_default_activation_function {act!r} (Sigmoid or Identity)")
    shape = BertShape(vocab_size=int(cfg["vocab_size"]), hidden=int(cfg["hidden_size"]),
                      layers=int(cfg["num_hidden_layers"]), heads=int(cfg["num_attention_heads"]),
                      intermediate=int(cfg["intermediate_size"]), max_position=int(cfg["max_position_embeddings"]),
                      type_vocab=int(cfg.get("type_vocab_size", 2)), ln_eps=float(cfg.get("layer_norm_eps", 1e-12)),
                      n_normalize=0)
    st = d / "model.safetensors"
    if not st.exists():
        raise FileNotFoundError(f"{st} missing (pytorch_model.bin pickles are not loaded: only safetensors)")
    sd = load_file(str(st))
    H = shape.hidden
    head = {}
    for name, shp in (("bert.pooler.dense.weight", (H, H)), ("bert.pooler.dense.bias", (H,)),
                      ("classifier.weight", (1, H)), ("classifier.bias", (1,))):
        if name not in sd:
            raise ValueError(f"{name} missing from {st.name}: not a BertForSequenceClassification with a pooler")
        if tuple(sd[name].shape) != shp:
            raise ValueError(f"{name}: expected {shp}, got {tuple(sd[name].shape)}")
        head[name] = np.ascontiguousarray(sd[name], dtype=np.float32)
    weights = state_dict_to_blob(sd, shape)
    limit = min(_native.ICREC_MAX_SEQLEN, shape.max_position)
    max_len = limit  # a cross-encoder reads up to the model's positions (tokenizer_config.json may ask for fewer)
    tc = d / "tokenizer_config.json"
    if tc.exists():
        asked = json.loads(tc.read_text()).get("model_max_length")
        if isinstance(asked, int) and 4 <= asked < max_len:
            max_len = asked
    return LoadedCrossEncoder(shape, weights, head["bert.pooler.dense.weight"], head["bert.pooler.dense.bias"],
                              head["classifier.weight"].reshape(H), head["classifier.bias"], max_len,
                              HostTokenizer(d, SIDE_MAX_TOKENS + 2), "identity" if act.endswith("Identity") else "sigmoid")


def write_synthetic_cross_encoder_dir(path: Path | str, seed: int = 0, shape: BertShape | None = None,
                                      activation: Optional[str] = None, max_length: Optional[int] = None) -> Path:
    """Write a cross-encoder directory (load_cross_encoder_dir's layout) with seeded random weights and the synthetic
    WordPiece vocab.  The encoder's tensors are synthetic_bert_weights(shape, seed) under the `bert.` prefix - its two
    token-type rows are independent draws, so row 1 differs from row 0 -, the pooler ~ N(0, 0.05) with bias ~ N(0, 0.02),
    the classifier ~ N(0, 0.1).  activation: None (no entry: sigmoid), "sigmoid" or "identity";  max_length: the
    tokenizer's model_max_length (default: the model's positions)."""
    from safetensors.numpy import save_file

    from .synthetic import normalish

    if activation not in (None, "sigmoid", "identity"):
        raise ValueError(f"activation must be None, 'sigmoid' or 'identity', got {activation!r}")
    d = Path(path)
    d.mkdir(parents=True, exist_ok=True)
    vocab = synthetic_vocab()
    if shape is None:
        shape = BertShape(vocab_size=len(vocab), n_normalize=0)
    if shape.vocab_size < len(vocab):
        raise ValueError("shape.vocab_size smaller than the synthetic vocab")
    if shape.type_vocab < 2:
        raise ValueError("a cross-encoder needs two token-type rows: shape.type_vocab must be >= 2")
    H = shape.hidden
    sd = {"bert." + k: v for k, v in blob_to_state_dict(synthetic_bert_weights(shape, seed=seed), shape).items()}
    types = sd["bert.embeddings.token_type_embeddings.weight"]
    assert np.abs(types[1] - types[0]).max() > 0
    sd["bert.pooler.dense.weight"] = normalish(seed, 8_001, H * H, 0.05).reshape(H, H)
    sd["bert.pooler.dense.bias"] = normalish(seed, 8_002, H, 0.02)
    sd["classifier.weight"] = normalish(seed, 8_003, H, 0.1).reshape(1, H)
    sd["classifier.bias"] = normalish(seed, 8_004, 1, 0.02)
    config = {"architectures": ["BertForSequenceClassification"], "model_type": "bert", "vocab_size": shape.vocab_size,
              "hidden_size": H, "num_hidden_layers": shape.layers, "num_attention_heads": shape.heads,
              "intermediate_size": shape.intermediate, "hidden_act": "gelu", "layer_norm_eps": shape.ln_eps,
              "max_position_embeddings": shape.max_position, "type_vocab_size": shape.type_vocab,
              "id2label": {"0": "LABEL_0"}, "label2id": {"LABEL_0": 0}}
    if activation is not None:
        config["sbert_ce_default_activation_function"] = "torch.nn.modules." + (
            "linear.Identity" if activation == "identity" else "activation.Sigmoid")
    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps(config, indent=2))
    (d / "vocab.txt").write_text("\n".join(vocab) + "\n")
    tok_cfg = {"do_lower_case": True, "tokenizer_class": "BertTokenizer"}
    if max_length is not None:
        tok_cfg["model_max_length"] = int(max_length)
    (d / "tokenizer_config.json").write_text(json.dumps(tok_cfg))
    return d


def strip_specials(ids: np.ndarray, cu: np.ndarray) -> list[np.ndarray]:
    """HostTokenizer.packed output (`[CLS] tokens [SEP]` back to back) -> each text's tokens without the two specials."""
    return [ids[cu[i] + 1:cu[i + 1] - 1] for i in range(len(cu) - 1)]


def truncate_pair(len_a: int, len_b: int, max_len: int) -> tuple[int, int]:
    """How many tokens of each side of a pair survive truncation to `max_len` ids, three of them special: the
    `longest_first` strategy as the `tokenizers` library (what sentence-transformers' CrossEncoder tokenises with)
    applies it, in closed form.  Tokens go one at a time from the end of the longer side until the pair fits; once the
    sides are level the shorter one - the FIRST on an exact tie - ends with floor(budget / 2) tokens and the other with
    the rest.  (transformers' pure-Python tokenizers break the tie the other way; the Rust library is the one matched.)"""
    budget = max_len - 3
    if budget < 0:
        raise ValueError(f"max_len {max_len} leaves no room for [CLS] [SEP] [SEP]")
    if len_a + len_b <= budget:
        return len_a, len_b
    a_short = len_a <= len_b
    short, long_ = (len_a, len_b) if a_short else (len_b, len_a)
    if 2 * short <= budget:
        long_ = budget - short
    else:
        short, long_ = budget // 2, budget - budget // 2
    return (short, long_) if a_short else (long_, short)


def assemble_pairs(a_ids: Sequence[Sequence[int]], b_ids: Sequence[Sequence[int]], max_len: int, cls_id: int,
                   sep_id: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Pair i = `[CLS] a_ids[i] [SEP] b_ids[i] [SEP]` truncated to max_len (truncate_pair), from the two sides' token ids
    without specials -> (ids int32[T], cu_seqlens int32[n+1], seg_b int32[n]): icrec_score_pairs' packed input, seg_b[i]
    = kept tokens of side a + 2 the position of the first token of type 1."""
    if len(a_ids) != len(b_ids):
        raise ValueError(f"{len(a_ids)} first sides against {len(b_ids)} second sides")
    n = len(a_ids)
    kept = [truncate_pair(len(a), len(b), max_len) for a, b in zip(a_ids, b_ids)]
    cu = np.zeros(n + 1, np.int32)
    np.cumsum([ka + kb + 3 for ka, kb in kept], out=cu[1:])
    ids = np.empty(int(cu[-1]), np.int32)
    seg_b = np.empty(n, np.int32)
    for i, (ka, kb) in enumerate(kept):
        o = int(cu[i])
        ids[o] = cls_id
        ids[o + 1:o + 1 + ka] = a_ids[i][:ka]
        ids[o + 1 + ka] = sep_id
        ids[o + 2 + ka:o + 2 + ka + kb] = b_ids[i][:kb]
        ids[o + 2 + ka + kb] = sep_id
        seg_b[i] = ka + 2
    return ids, cu, seg_b
