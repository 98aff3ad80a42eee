"""The encoder written from the math, in torch on the CPU (TEST INFRASTRUCTURE ONLY, like oracle/torch_reference.py).

    x_0   = LN(word[id] + type[0] + pos[t])
    per layer:
      Q, K, V = x Wq^T + bq, x Wk^T + bk, x Wv^T + bv          split into heads of d = hidden / heads
      ctx_h   = softmax(Q_h K_h^T / sqrt(d) + B_h) V_h         over the keys of the token's own sequence
      x       = LN(ctx Wo^T + bo + x)
      x       = LN(gelu_erf(x W1^T + b1) W2^T + b2 + x)        gelu_erf(u) = u/2 (1 + erf(u / sqrt 2))
    pooled  = mean over the sequence's tokens, then n_normalize times v / max(|v|_2, 1e-12)
    LN(v)   = (v - mean) / sqrt(biased var + eps) * gamma + beta
    B_h     = 0, or with an `attention_bias` table (the MPNet family's relative-position bias, float32 [heads, 1023])
              B_h[i, j] = table[h, 511 + (j - i)], the same in EVERY layer

In float64 (the default) it is the truth: nothing follows the fp32 oracle's summation order (oracle/icrec_oracle.c), so
an error shared by the oracle and the kernels that mirror it does not cancel here.  The SAME code in float32 gives E_ref
for the cases the C oracle cannot run (it knows no bias): the error an fp32 implementation makes on the same inputs.
The weights are the fp32 blob (include/icrec.h order, split with synthetic.blob_to_state_dict), widened exactly.

`fault=(name, layer)` makes ONE stage of ONE layer wrong on purpose.  The faults exist only here: tests use them to
prove that a per-token comparison against this reference would notice the mistakes a kernel rewrite can make
(tests/test_token_states.py, tests/test_value_ranges.py).  FAULTS and RANGE_FAULTS list the names.
"""
from __future__ import annotations

import collections
import math
from typing import Optional

import numpy as np
import torch

#: name -> what goes wrong in the chosen layer
FAULTS = {
    "x_f16_before_qkv": "the layer's input activations are rounded to f16 before the Q/K/V projections (a lo plane lost)",
    "softmax_f16": "softmax probabilities are rounded to f16 before P.V",
    "v_f16": "V is rounded to f16",
    "gelu_f16": "the GELU output is rounded to f16 before the FFN-down projection",
    "tanh_gelu": "tanh-approximated GELU instead of the erf form",
    "scale_1pct": "softmax scale 1.01 / sqrt(d)",
    "stale_last_row": "the last token's context row is a copy of the row before it (stale tile row)",
    "drop_last_key": "the last key of each sequence is left out of the softmax",
    "zero_head_last_row": "head 0's context of each sequence's last token is zero",
    "ln_eps_1e-5": "both LayerNorms of the layer use eps 1e-5 instead of the shape's",
}

#: faults of the GELU's value range: what a clamp, a dropped tail or a poor fit of the kernels' erfc polynomial does.
#: Two of them change nothing while |u| <= 3 (every pre-GELU value of the "standard" and "sharp" weight sets), so they
#: stand beside FAULTS, whose entries tests/test_token_states.py requires on those sets, and are asserted where the
#: inputs reach them: the "heavy" set and the GELU probes (tests/test_value_ranges.py).  `fault=` accepts both tables.
RANGE_FAULTS = {
    "gelu_tail_dropped": "gelu(u) = max(u, 0) wherever |u| > 3 (the erfc term dropped outside the middle)",
    "gelu_clamp_4": "the erfc argument is clamped at 4: gelu(u) = max(u, 0) - |u|/2 erfc(min(|u|, 4) / sqrt 2)",
    "gelu_erfc_rel_1e-3": "the erfc term is 1.001 times too large (a poor polynomial fit)",
}

#: what `stats` receives per layer
LayerStats = collections.namedtuple(
    "LayerStats", "logit_std mean_max_softmax share_u_gt_3 share_u_gt_5_75 max_abs_u")

#: how a linear layer adds its K products (Float64Bert's `linears`)
LINEARS = ("blas", "single_accumulator")


def _f16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(t.dtype)


def _single_accumulator_linear(t, weight, bias):
    """t W^T + b with ONE accumulator per output, the K products added in ascending order in the working dtype: what a
    kernel's MFMA chain and a C loop do.  (A BLAS matmul splits K into blocks with an accumulator each and adds the
    blocks at the end: in float32 it errs 2 - 2.5x less at K = 3,072 than any single-accumulator fp32 implementation,
    and E_ref would not be the error such an implementation makes.)"""
    acc = torch.zeros((t.shape[0], weight.shape[0]), dtype=t.dtype)
    tT, wT = t.T.contiguous(), weight.T.contiguous()
    for k in range(tT.shape[0]):
        acc.addcmul_(tT[k][:, None], wT[k][None, :])
    return acc + bias


class Float64Bert:
    """The blob's model in `dtype` on the CPU, with the bias table `attention_bias` (float32 [heads, 1023]) or, with
    None, without one.  `linears`: "blas" (t @ W^T: fast enough for 16k-token batches, and in float64 the order of the
    additions is far below anything measured against it) or "single_accumulator" (_single_accumulator_linear, what
    makes a float32 run err as an fp32 implementation does); by default "blas" in float64 and "single_accumulator" in
    any narrower dtype.  encode() -> (last hidden state [T, H], mean-pooled + normalised [n, H]), both in `dtype`.
    (Named for its default and for the file: in float32 it is still this class.)"""

    def __init__(self, blob: np.ndarray, shape, dtype=torch.float64, attention_bias: Optional[np.ndarray] = None,
                 linears: Optional[str] = None):
        from instacart_next_order_recommendation_amd import relative_bias as rb  # the table's layout only
        from instacart_next_order_recommendation_amd import synthetic as syn  # blob layout only

        self.shape, self.dtype = shape, dtype
        self.linears = linears if linears is not None else ("blas" if dtype == torch.float64 else "single_accumulator")
        if self.linears not in LINEARS:
            raise ValueError(f"linears must be one of {LINEARS}, got {self.linears!r}")
        sd = syn.blob_to_state_dict(np.asarray(blob, np.float32), shape)
        self.p = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd.items()}
        self.max_offset = rb.MAX_OFFSET
        self.table = None
        if attention_bias is not None:
            self.table = torch.from_numpy(np.asarray(attention_bias, np.float32)).to(dtype)
            assert tuple(self.table.shape) == (shape.heads, 2 * rb.MAX_OFFSET + 1), tuple(self.table.shape)

    def _ln(self, v: torch.Tensor, name: str, eps: float) -> torch.Tensor:
        mean = v.mean(-1, keepdim=True)
        var = ((v - mean) ** 2).mean(-1, keepdim=True)
        return (v - mean) / torch.sqrt(var + eps) * self.p[name + ".weight"] + self.p[name + ".bias"]

    def _linear(self, t: torch.Tensor, name: str) -> torch.Tensor:
        weight, bias = self.p[name + ".weight"], self.p[name + ".bias"]
        return t @ weight.T + bias if self.linears == "blas" else _single_accumulator_linear(t, weight, bias)

    @torch.no_grad()
    def encode(self, ids: np.ndarray, cu: np.ndarray, fault: Optional[tuple] = None, stats: Optional[list] = None):
        """ids int[T], cu int[n+1] (packed sequences).  `stats`, when a list, receives one LayerStats per layer: std of
        the pre-softmax logits, mean over rows of the largest softmax weight, the shares of the pre-GELU values u with
        |u| > 3 and with |u| > 5.75, and the largest |u|."""
        s, p = self.shape, self.p
        H, nh = s.hidden, s.heads
        d = H // nh
        fname, flayer = fault if fault is not None else (None, -1)
        if fname is not None and fname not in FAULTS and fname not in RANGE_FAULTS:
            raise ValueError(f"unknown fault {fname!r}")
        ids_t = torch.from_numpy(np.asarray(ids, np.int64))
        cu = np.asarray(cu, np.int64)
        pos = torch.from_numpy(np.concatenate([np.arange(b - a) for a, b in zip(cu[:-1], cu[1:])]))
        x = (p["embeddings.word_embeddings.weight"][ids_t] + p["embeddings.token_type_embeddings.weight"][0]
             + p["embeddings.position_embeddings.weight"][pos])
        x = self._ln(x, "embeddings.LayerNorm", float(s.ln_eps))
        for l in range(s.layers):
            f = fname if l == flayer else None
            q = f"encoder.layer.{l}."
            eps = 1e-5 if f == "ln_eps_1e-5" else float(s.ln_eps)
            xin = _f16(x) if f == "x_f16_before_qkv" else x
            Q, K, V = (self._linear(xin, q + "attention.self." + name) for name in ("query", "key", "value"))
            if f == "v_f16":
                V = _f16(V)
            scale = (1.01 if f == "scale_1pct" else 1.0) / math.sqrt(d)
            ctx = torch.empty_like(x)
            logit_sq, logit_sum, logit_n, pmax_sum, pmax_n = 0.0, 0.0, 0, 0.0, 0
            for a, b in zip(cu[:-1], cu[1:]):
                n = int(b - a)
                qh = Q[a:b].view(n, nh, d).transpose(0, 1)  # [heads, n, d]
                kh = K[a:b].view(n, nh, d).transpose(0, 1)
                vh = V[a:b].view(n, nh, d).transpose(0, 1)
                logits = qh @ kh.transpose(1, 2) * scale     # [heads, n queries, n keys]
                if self.table is not None:
                    at = torch.arange(n)
                    logits = logits + self.table[:, self.max_offset + at[None, :] - at[:, None]]  # key - query
                if f == "drop_last_key" and n > 1:
                    logits[:, :, n - 1] = -math.inf
                prob = torch.softmax(logits, dim=-1)
                if stats is not None:
                    logit_sq += float((logits ** 2).sum()); logit_sum += float(logits.sum()); logit_n += logits.numel()
                    pmax_sum += float(prob.max(-1).values.sum()); pmax_n += nh * n
                if f == "softmax_f16":
                    prob = _f16(prob)
                c = prob @ vh                                # [heads, n, d]
                if f == "zero_head_last_row":
                    c[0, n - 1] = 0.0
                c = c.transpose(0, 1).reshape(n, H)
                if f == "stale_last_row" and n > 1:
                    c[n - 1] = c[n - 2]
                ctx[a:b] = c
            x = self._ln(self._linear(ctx, q + "attention.output.dense") + x, q + "attention.output.LayerNorm", eps)
            u = self._linear(x, q + "intermediate.dense")
            if stats is not None:
                m, au = logit_sum / logit_n, u.abs()
                stats.append(LayerStats(math.sqrt(max(logit_sq / logit_n - m * m, 0.0)), pmax_sum / pmax_n,
                                        float((au > 3.0).double().mean()), float((au > 5.75).double().mean()),
                                        float(au.max())))
            if f == "tanh_gelu":
                g = 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))
            elif f in ("gelu_clamp_4", "gelu_erfc_rel_1e-3"):  # gelu(u) = max(u, 0) - |u|/2 erfc(|u| / sqrt 2)
                t = u.abs().clamp(max=4.0) if f == "gelu_clamp_4" else u.abs()
                erfc = (1.001 if f == "gelu_erfc_rel_1e-3" else 1.0) * torch.erfc(t / math.sqrt(2.0))
                g = u.clamp(min=0.0) - 0.5 * u.abs() * erfc
            elif f == "gelu_tail_dropped":
                g = torch.where(u.abs() > 3.0, u.clamp(min=0.0), 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0))))
            else:
                g = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
            if f == "gelu_f16":
                g = _f16(g)
            x = self._ln(self._linear(g, q + "output.dense") + x, q + "output.LayerNorm", eps)
        emb = torch.stack([x[a:b].mean(0) for a, b in zip(cu[:-1], cu[1:])])
        for _ in range(s.n_normalize):
            emb = emb / emb.norm(dim=1, keepdim=True).clamp(min=1e-12)
        return x.numpy(), emb.numpy()


def encode(blob: np.ndarray, shape, ids: np.ndarray, cu: np.ndarray, fault: Optional[tuple] = None,
           stats: Optional[list] = None, dtype=torch.float64, attention_bias: Optional[np.ndarray] = None,
           linears: Optional[str] = None):
    """One-shot form of Float64Bert(blob, shape, dtype, attention_bias, linears).encode(ids, cu, fault, stats)."""
    return Float64Bert(blob, shape, dtype, attention_bias, linears).encode(ids, cu, fault, stats)
