"""Shared by the pair-score tests (tests/test_pair_scores.py on the CPU, tests/test_pair_scores_gpu.py on the GPU): the
reference cross-encoder written from the math, the cases, their references (computed once, read-only) and the one
comparison (`check`).

    x_0    = LN((word[id] + type[tt]) + pos[t])       tt = 1 where the position in the sequence is >= seg_b[s], else 0
    layers   as oracle/float64_reference.py (imported: that file hard-codes type[0] and is not edited - PairBert hands it
             a word table of 2 V rows, row id + V * tt = word[id] + type[tt] computed in the working dtype, and a zero
             type table, so its `word + type[0] + pos` IS the line above, rounding for rounding)
    h      = last hidden state of each sequence's first token
    p      = tanh(Wp h + bp)                           BertPooler
    logit  = wc . p + bc                               the classifier of BertForSequenceClassification(num_labels = 1)

In float64 it is the truth.  The same code in float32 with single-accumulator linears (the encoder's and the head's) gives
E_ref, the error an fp32 implementation makes on the same inputs; a GPU result must stay within MARGINS x E_ref.
"""
from __future__ import annotations

import numpy as np
import torch

from instacart_next_order_recommendation_amd import synthetic as syn
from oracle import float64_reference as f64

VOCAB = 2048
WIDTHS = {384: dict(hidden=384, heads=12, intermediate=1536), 768: dict(hidden=768, heads=12, intermediate=3072)}
SHAPES = ((384, 2), (768, 1))  # (hidden, layers)
MODES = ("f32", "f16x3")

#: margin on E_ref per (gemm mode, hidden): the smallest of {2, 3, 4, 6, 8} that leaves 1.5x headroom over the worst ratio
#: E_gpu / E_ref measured on the MI355X over every case of tests/test_pair_scores_gpu.py - MARGINS for the logits of the
#: whole path, HEAD_MARGINS for the head alone (profiles/pair_score_errors.md holds the ratios; tests/token_states.py's rule).
MARGINS = {("f32", 384): 2, ("f32", 768): 2, ("f16x3", 384): 2, ("f16x3", 768): 2}
HEAD_MARGINS = {("f32", 384): 4, ("f32", 768): 4, ("f16x3", 384): 6, ("f16x3", 768): 4}

#: the fixed total lengths of the main batch ([CLS][SEP][SEP] alone; around the 32-token tile; 2, 3, 5 and 8 key tiles)
FIXED_LENS = [3, 31, 32, 33, 64, 65, 129, 256]
N_RANDOM = 62  # + lengths drawn from 5 .. 40: 70 pairs, about 2,000 tokens
#: name -> (lengths, max_seq_length the encoder needs or None for the default 256)
BATCHES = {"to256": None, "to512": 512}


def shape(hidden: int, layers: int) -> syn.BertShape:
    return syn.BertShape(vocab_size=VOCAB, layers=layers, n_normalize=0, **WIDTHS[hidden])


def head_weights(hidden: int, seed: int):
    """(pooler_w [H, H], pooler_b [H], cls_w [H], cls_b [1]) float32: the pooler at the encoder's std 0.05, its
    pre-activations have a standard deviation near 1 (tanh is far from linear there), the classifier N(0, 0.1)."""
    H = hidden
    return (syn.normalish(seed, 8_001, H * H, 0.05).reshape(H, H), syn.normalish(seed, 8_002, H, 0.02),
            syn.normalish(seed, 8_003, H, 0.1), syn.normalish(seed, 8_004, 1, 0.02))


def batch(name: str, seed: int = 7):
    """(ids int32[T], cu int32[n+1], seg_b int32[n]).  seg_b cycles through 2, len - 1 (empty second side), len (no
    type-1 token) and the middle of the sequence; the 3-token pair has seg_b = 2."""
    rng = np.random.default_rng(seed)
    if name == "to256":
        lens = FIXED_LENS + rng.integers(5, 41, N_RANDOM).tolist()
    else:
        assert name == "to512", name
        lens = [257, 512, 40, 300, 7]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.integers(0, VOCAB, int(cu[-1])).astype(np.int32)
    seg_b = np.array([(2, n - 1, n, n // 2)[i % 4] for i, n in enumerate(lens)], np.int32)
    if name == "to512":  # the long ones split mid-sequence and past the 256th token
        seg_b[:2] = (130, 400)
    return ids, cu, seg_b


class PairBert:
    """The cross-encoder of a blob and a head in `dtype` on the CPU; logits(ids, cu, seg_b) -> numpy [n] in `dtype`."""

    def __init__(self, blob: np.ndarray, s: syn.BertShape, head, dtype=torch.float64):
        self.s, self.dtype = s, dtype
        self.bert = f64.Float64Bert(blob, s, dtype)  # (float64: BLAS linears; narrower: single-accumulator)
        p = self.bert.p
        word, typ = p["embeddings.word_embeddings.weight"], p["embeddings.token_type_embeddings.weight"]
        assert typ.shape[0] >= 2
        p["embeddings.word_embeddings.weight"] = torch.cat([word + typ[0], word + typ[1]])
        p["embeddings.token_type_embeddings.weight"] = torch.zeros_like(typ)
        self.head = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype) for a in head]

    def _linear(self, t, weight, bias):
        return t @ weight.T + bias if self.bert.linears == "blas" else f64._single_accumulator_linear(t, weight, bias)

    def head_logits(self, h: np.ndarray, tanh: bool = True) -> np.ndarray:
        """The head alone on rows h [n, H]."""
        wp, bp, wc, bc = self.head
        p = self._linear(torch.from_numpy(np.ascontiguousarray(h)).to(self.dtype), wp, bp)
        if tanh:
            p = torch.tanh(p)
        return self._linear(p, wc[None, :], bc)[:, 0].numpy()

    @torch.no_grad()
    def cls_states(self, ids, cu, seg_b, types: bool = True) -> np.ndarray:
        """Last hidden state [n, H] of each sequence's first token; types=False: every token takes type row 0."""
        cu = np.asarray(cu, np.int64)
        lens = np.diff(cu)
        pos = np.concatenate([np.arange(n) for n in lens])
        start = np.repeat(np.clip(np.asarray(seg_b, np.int64), 0, lens), lens)
        tt = (pos >= start) if types else np.zeros_like(pos, bool)
        h, _ = self.bert.encode(np.asarray(ids, np.int64) + self.s.vocab_size * tt, cu)
        return h[cu[:-1]]

    @torch.no_grad()
    def logits(self, ids, cu, seg_b, types: bool = True, tanh: bool = True) -> np.ndarray:
        return self.head_logits(self.cls_states(ids, cu, seg_b, types), tanh)


def head64(h: np.ndarray, head) -> np.ndarray:
    """The head in numpy float64 on fp32 rows h [n, H] (the head-in-isolation test's truth)."""
    wp, bp, wc, bc = (np.asarray(a, np.float64) for a in head)
    return np.tanh(np.asarray(h, np.float64) @ wp.T + bp) @ wc + bc[0]


_cases: dict = {}


def case(hidden: int, layers: int, name: str) -> dict:
    """One GPU case, computed once and shared (results read-only):
    s, w, head, ids, cu, seg_b, max_len;  l64 / l32: the float64 / float32 logits;  l64_type0, l64_no_tanh: the float64
    logits with every type forced to 0 / without the pooler's tanh (the discrimination test);  whole64 / whole32: the
    logits with seg_b = len for every pair (the head-in-isolation case), whole64_no_tanh: those without the tanh;
    head64: the numpy float64 head on the float32 reference's rows (whole32 against it is the head's own E_ref)."""
    key = (hidden, layers, name)
    if key not in _cases:
        s = shape(hidden, layers)
        w = syn.synthetic_bert_weights(s, seed=23)
        head = head_weights(hidden, seed=23)
        ids, cu, seg_b = batch(name)
        m64, m32 = PairBert(w, s, head), PairBert(w, s, head, torch.float32)
        whole = np.diff(cu).astype(np.int32)
        h64_whole, h32_whole = m64.cls_states(ids, cu, whole), m32.cls_states(ids, cu, whole)
        r = dict(s=s, w=w, head=head, ids=ids, cu=cu, seg_b=seg_b, whole=whole, max_len=BATCHES[name],
                 l64=m64.logits(ids, cu, seg_b), l32=m32.logits(ids, cu, seg_b),
                 l64_type0=m64.head_logits(h64_whole), l64_no_tanh=m64.logits(ids, cu, seg_b, tanh=False),
                 whole64=m64.head_logits(h64_whole), whole32=m32.head_logits(h32_whole),
                 whole64_no_tanh=m64.head_logits(h64_whole, tanh=False),
                 # E_ref of the head alone: whole32 (the float32 head on the float32 rows) against the float64 head on
                 # the SAME float32 rows
                 head64=head64(h32_whole, head))
        for a in r.values():
            if isinstance(a, np.ndarray) and a.dtype.kind == "f":
                a.setflags(write=False)
        w.setflags(write=False)
        _cases[key] = r
    return _cases[key]


def errors(got: np.ndarray, want: np.ndarray) -> float:
    """The metric: the largest absolute error over the batch's logits, in float64."""
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


def check(what: str, got: np.ndarray, want64: np.ndarray, ref32: np.ndarray, margin: float):
    """Prints `RATIO ...` (E_gpu / E_ref), then asserts E_gpu <= margin x E_ref; a failure names the worst pair."""
    e_ref, e_gpu = errors(ref32, want64), errors(got, want64)
    assert e_ref > 0
    print(f"RATIO {what}: E_gpu {e_gpu:.3e}, E_ref {e_ref:.3e}, ratio {e_gpu / e_ref:.2f} (margin {margin})")
    worst = int(np.abs(np.asarray(got, np.float64) - want64).argmax())
    assert e_gpu <= margin * e_ref, (what, f"worst pair {worst}: got {float(got[worst]):.9g}, want {float(want64[worst]):.9g}")
