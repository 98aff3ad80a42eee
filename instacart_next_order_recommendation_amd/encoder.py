"""Host side of the device encoder: SentenceTransformer.encode's GPU work.

The reference calls `self.model.encode(texts, batch_size=64, normalize_embeddings=True)`
(src/inference/serve_recommendations.py:195-200, :213, :246).  Here tokenisation is a
separate host stage (tokenizer.py); this module takes token ids, packs them back to back
(no padding), and runs libicrec's fp32-MFMA BERT forward + pooling (mean, or the [CLS] token's state) + L2-normalise.

torch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native
from ._native import ptr, stream_ptr
from .synthetic import BertShape

DEFAULT_GEMM_MODE = "f16x3"
MAX_SEQ_LEN = 256  # configs/train.yaml:11 (max_seq_length): an encoder's default ceiling
MAX_SEQ_LEN_LIMIT = _native.ICREC_MAX_SEQLEN  # the highest ceiling (icrec_encoder_set_max_seqlen)


def pack_token_ids(seqs: Sequence[Sequence[int]], max_len: int = MAX_SEQ_LEN):
    """List of id lists -> (ids int32[T], cu_seqlens int32[n+1], max_len); sequences longer than `max_len` are refused."""
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
    if len(seqs) == 0 or (lens < 1).any():
        raise ValueError("every sequence needs at least one token")
    if lens.max() > max_len:
        raise ValueError(f"sequence longer than max_seq_length={max_len}; truncate on the host")
    cu = np.zeros(len(seqs) + 1, np.int32)
    np.cumsum(lens, out=cu[1:])
    ids = np.concatenate([np.asarray(s, np.int32) for s in seqs]) if len(seqs) > 1 else np.asarray(seqs[0], np.int32)
    return ids, cu, int(lens.max())


class DeviceEncoder:
    """all-MiniLM-L6-v2-shaped BERT encoder resident on one GPU."""

    SPLIT_MIN_SEQS = 128       # two-stream split only when each half has at least this many sequences ...
    SPLIT_MIN_TOKENS = 16384   # ... and this many tokens (enough blocks to fill the chip on its own)

    def __init__(self, weights: np.ndarray, shape: BertShape = BertShape(), device: str | torch.device = "cuda:0",
                 gemm_mode: Optional[str] = None, max_seq_length: Optional[int] = None, pooling: str = "mean",
                 attention_bias: Optional[np.ndarray] = None):
        """gemm_mode: "f32" (exact f32 MFMA, bit-identical GEMMs) or "f16x3" (3-term split on the f16
        MFMA, fp32-level accuracy, ~4x faster); default from $ICREC_GEMM_MODE, else DEFAULT_GEMM_MODE.
        max_seq_length: the longest sequence the encoder must take, up to min(512, shape.max_position).  The
        ceiling is min(256, shape.max_position) by default and only ever raised: a larger value sets it
        (icrec_encoder_set_max_seqlen), a smaller one keeps the default.  Sequences of up to 256 tokens encode
        to the same bits whatever the ceiling.
        pooling: "mean" (sentence-transformers Pooling(mean), all-MiniLM) or "cls" (Pooling(cls), the BGE family: the
        last hidden state of each sequence's first token), set once here (icrec_encoder_set_pooling).
        attention_bias: float32 [heads, 2 * 512 - 1], the MPNet family's relative-position bias: entry
        [h, 511 + (key - query)] is added to every scaled attention logit of head h in every layer
        (icrec_encoder_set_attention_bias; relative_bias.table_from_buckets makes it from a model's bucket table)."""
        self.device = _native.hip_device(device, "DeviceEncoder")
        self.shape = shape
        L = _native.lib()
        import os

        self.gemm_mode = gemm_mode or os.getenv("ICREC_GEMM_MODE") or DEFAULT_GEMM_MODE
        if self.gemm_mode not in _native.GEMM_MODES:
            raise ValueError(f"gemm_mode must be one of {sorted(_native.GEMM_MODES)}, got {self.gemm_mode!r}")
        if pooling not in _native.POOLING_MODES:
            raise ValueError(f"pooling must be one of {sorted(_native.POOLING_MODES)}, got {pooling!r}")
        self.pooling = pooling
        self._cfg = _native.BertCfg(shape.vocab_size, shape.hidden, shape.layers, shape.heads, shape.intermediate,
                                    shape.max_position, shape.type_vocab, shape.ln_eps, shape.n_normalize,
                                    _native.GEMM_MODES[self.gemm_mode])
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        want = int(L.icrec_encoder_weight_count(C.byref(self._cfg)))
        if w.size != want:
            raise ValueError(f"weight blob has {w.size} floats, expected {want} (layout: include/icrec.h)")
        h = C.c_void_p()
        _native.check(L.icrec_encoder_create(w.ctypes.data_as(C.c_void_p), w.size, C.byref(self._cfg),
                                             self.device.index, C.byref(h)), "icrec_encoder_create")
        self._h = h
        self.max_seq_length = min(MAX_SEQ_LEN, shape.max_position)
        try:
            if pooling != "mean":  # (a mean-pooled encoder makes the calls it always made)
                _native.check(L.icrec_encoder_set_pooling(h, _native.POOLING_MODES[pooling]), "icrec_encoder_set_pooling")
            if attention_bias is not None:  # (an encoder without one makes the calls it always made)
                self.set_attention_bias(attention_bias)
            if max_seq_length is not None and not 1 <= int(max_seq_length) <= self.max_seq_length:
                _native.check(L.icrec_encoder_set_max_seqlen(h, int(max_seq_length)), "icrec_encoder_set_max_seqlen")
                self.max_seq_length = int(max_seq_length)
        except _native.IcrecError:
            self.close()
            raise
        self._ws_by_stream = _native.StreamScratch(self.device)
        self._side: Optional[torch.cuda.Stream] = None

    def set_attention_bias(self, table: Optional[np.ndarray]) -> None:
        """Set (float32 [heads, 2 * 512 - 1]) or, with None, remove the relative-position attention bias.  Like the
        pooling mode it belongs before the first encode; a refused table leaves the encoder as it was."""
        L = _native.lib()
        if table is None:
            _native.check(L.icrec_encoder_set_attention_bias(self._h, None, 0), "icrec_encoder_set_attention_bias")
            return
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != 2 * _native.ICREC_MAX_SEQLEN - 1:
            raise ValueError(f"attention_bias must be [heads, {2 * _native.ICREC_MAX_SEQLEN - 1}], got {t.shape}")
        _native.check(L.icrec_encoder_set_attention_bias(self._h, t.ctypes.data_as(C.c_void_p), t.shape[0]),
                      "icrec_encoder_set_attention_bias")

    @property
    def has_attention_bias(self) -> bool:
        return _native.lib().icrec_encoder_has_attention_bias(self._h) == 1

    def set_score_head(self, pooler_w: Optional[np.ndarray], pooler_b: Optional[np.ndarray] = None,
                       cls_w: Optional[np.ndarray] = None, cls_b: Optional[np.ndarray] = None) -> None:
        """Set a cross-encoder's score head - BertPooler weight float32 [hidden, hidden] ([out, in]) and bias [hidden],
        classifier weight [hidden] and bias [1] - or, with pooler_w None, remove it (icrec_encoder_set_score_head).
        Like the attention bias it belongs before the first compute call; a refused head leaves the encoder as it was."""
        L = _native.lib()
        if pooler_w is None:
            _native.check(L.icrec_encoder_set_score_head(self._h, None, None, None, None), "icrec_encoder_set_score_head")
            return
        H = self.shape.hidden
        arrs = []
        for name, a, shp in (("pooler_w", pooler_w, (H, H)), ("pooler_b", pooler_b, (H,)), ("cls_w", cls_w, (H,)),
                             ("cls_b", cls_b, (1,))):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.size != int(np.prod(shp)) or (name == "pooler_w" and a.shape != shp):
                raise ValueError(f"{name} must be float32 {list(shp)}, got {list(a.shape)}")
            arrs.append(a)
        _native.check(L.icrec_encoder_set_score_head(self._h, *(a.ctypes.data_as(C.c_void_p) for a in arrs)),
                      "icrec_encoder_set_score_head")

    @property
    def has_score_head(self) -> bool:
        return _native.lib().icrec_encoder_has_score_head(self._h) == 1

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.lib().icrec_encoder_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def batch_split(self, total_tokens: int) -> tuple[int, int]:
        """(main_tokens, tail_tokens): how icrec_encode cuts a call of `total_tokens` tokens into whole rounds of
        64 tokens per CU for the batch kernels and a remainder for the small-batch kernels on the library's side
        stream (icrec_encode_batch_split).  The one Python call site of that entry besides bench.py, which keeps a
        raw call of its own."""
        m, t = C.c_int64(0), C.c_int64(0)
        _native.check(_native.lib().icrec_encode_batch_split(self._h, int(total_tokens), C.byref(m), C.byref(t)),
                      "icrec_encode_batch_split")
        return int(m.value), int(t.value)

    def encode_into(self, ids: torch.Tensor, cu: torch.Tensor, n: int, T: int, max_seqlen: int, out: torch.Tensor,
                    ws: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None) -> None:
        """One icrec_encode on the current stream: device int32 ids[T] and cu_seqlens[n+1] -> out float32 [n, hidden].
        `ws`: a workspace the caller owns (a captured graph bakes its address); by default this stream's block.
        `tokens`: float32 [T, hidden] that also receives every token's last hidden state (icrec_encode_ex)."""
        L = _native.lib()
        if ws is None:
            ws = self._ws_by_stream.block(int(L.icrec_encode_workspace_bytes(self._h, T, n)))
        if tokens is None:
            _native.check(L.icrec_encode(self._h, ptr(ids), ptr(cu), n, T, int(max_seqlen), ptr(out), ptr(ws),
                                         ws.numel(), stream_ptr(self.device)), "icrec_encode")
        else:
            _native.check(L.icrec_encode_ex(self._h, ptr(ids), ptr(cu), n, T, int(max_seqlen), ptr(out), ptr(tokens),
                                            ptr(ws), ws.numel(), stream_ptr(self.device)), "icrec_encode_ex")

    def score_into(self, ids: torch.Tensor, cu: torch.Tensor, seg_b: torch.Tensor, n: int, T: int, max_seqlen: int,
                   out: torch.Tensor, ws: Optional[torch.Tensor] = None) -> None:
        """One icrec_score_pairs on the current stream: device int32 ids[T], cu_seqlens[n+1] and seg_b[n] -> out float32
        [n], each pair's raw logit.  `ws`: a workspace the caller owns (a captured graph bakes its address); by default
        this stream's block."""
        L = _native.lib()
        if ws is None:
            ws = self._ws_by_stream.block(int(L.icrec_score_pairs_workspace_bytes(self._h, T, n)))
        _native.check(L.icrec_score_pairs(self._h, ptr(ids), ptr(cu), ptr(seg_b), n, T, int(max_seqlen), ptr(out), ptr(ws),
                                          ws.numel(), stream_ptr(self.device)), "icrec_score_pairs")

    def score_packed(self, ids: torch.Tensor, cu_seqlens: torch.Tensor, seg_b: torch.Tensor, max_seqlen: int,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Packed pairs (int32 ids[T], cu_seqlens[n+1], seg_b[n]: model_io.assemble_pairs) -> float32 [n] raw logits on
        the device, through the score head (set_score_head)."""
        if ids.dtype != torch.int32 or cu_seqlens.dtype != torch.int32 or seg_b.dtype != torch.int32:
            raise TypeError("ids, cu_seqlens and seg_b must be int32")
        ids = ids.to(self.device).contiguous()
        cu = cu_seqlens.to(self.device).contiguous()
        seg = seg_b.to(self.device).contiguous()
        n, T = int(cu.numel()) - 1, int(ids.numel())
        if int(seg.numel()) != n:
            raise ValueError(f"seg_b has {int(seg.numel())} entries for {n} pairs")
        if out is None:
            out = torch.empty((n,), dtype=torch.float32, device=self.device)
        self.score_into(ids, cu, seg, n, T, max_seqlen, out)
        return out

    def encode_packed(self, ids: torch.Tensor, cu_seqlens: torch.Tensor, max_seqlen: int,
                      out: Optional[torch.Tensor] = None, cu_host: Optional[np.ndarray] = None,
                      return_tokens: bool = False, tokens_out: Optional[torch.Tensor] = None):
        """Device tensors in (int32 ids[T], int32 cu_seqlens[n+1]) -> float32 [n, hidden] on the device.

        With `return_tokens` the result is `(emb, tokens)`: tokens float32 [T, hidden] is the last hidden state of
        every token (SentenceTransformer.encode(output_value="token_embeddings")), the very rows the pooling summed;
        `tokens_out` is a contiguous float32 [T, hidden] device tensor to receive them (allocated when None).

        With `cu_host` (the host copy of cu_seqlens) and a large batch, the two halves of the batch run
        concurrently on two HIP streams (own workspaces, fork/join by events): one half's bandwidth-bound
        kernels overlap the other half's MFMA-bound GEMMs (-6 % per batch of 1,024 contexts).  Results are
        identical: every kernel is per-sequence / per-token."""
        if ids.dtype != torch.int32 or cu_seqlens.dtype != torch.int32:
            raise TypeError("ids and cu_seqlens must be int32")
        ids = ids.to(self.device).contiguous()
        cu = cu_seqlens.to(self.device).contiguous()
        n, T = int(cu.numel()) - 1, int(ids.numel())
        if out is None:
            out = torch.empty((n, self.shape.hidden), dtype=torch.float32, device=self.device)
        tok = None
        if return_tokens:
            tok = tokens_out
            if tok is None:
                tok = torch.empty((T, self.shape.hidden), dtype=torch.float32, device=self.device)
            elif (tok.dtype != torch.float32 or tuple(tok.shape) != (T, self.shape.hidden) or not tok.is_contiguous()
                  or tok.device != self.device):
                raise TypeError(f"tokens_out must be a contiguous float32 [{T}, {self.shape.hidden}] tensor on {self.device}")
        if cu_host is None or n < 2 * self.SPLIT_MIN_SEQS or T < 2 * self.SPLIT_MIN_TOKENS:
            self.encode_into(ids, cu, n, T, max_seqlen, out, tokens=tok)
            return (out, tok) if return_tokens else out
        half = n // 2
        t_half = int(cu_host[half])
        # the second half's rebased cu_seqlens, computed per call on the caller's stream (one tiny kernel).  Never
        # cached by address: the allocator hands the next batch's cu tensor the same address, and two different
        # batches with equal n and t_half would then share stale sequence boundaries.
        cu_b = cu[half:] - t_half
        main = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            self.encode_into(ids[t_half:], cu_b, n - half, T - t_half, max_seqlen, out[half:],
                             tokens=None if tok is None else tok[t_half:])
        self.encode_into(ids[:t_half], cu[: half + 1], half, t_half, max_seqlen, out[:half],
                         tokens=None if tok is None else tok[:t_half])
        main.wait_stream(self._side)
        return (out, tok) if return_tokens else out

    def encode_packed_host(self, ids: np.ndarray, cu: np.ndarray, max_tokens_per_call: int = 1 << 18) -> torch.Tensor:
        """Host arrays in the packed form (ids int32[T], cu_seqlens int32[n+1], e.g. HostTokenizer.packed) ->
        embeddings [n, hidden] on the device, in input order; split into calls of at most
        `max_tokens_per_call` tokens."""
        n = int(cu.shape[0]) - 1
        out = torch.empty((n, self.shape.hidden), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        lens = np.diff(cu)
        if (lens < 1).any():
            raise ValueError("every sequence needs at least one token")
        if int(lens.max()) > self.max_seq_length:
            raise ValueError(f"sequence longer than max_seq_length={self.max_seq_length}; truncate on the host")
        if int(ids.min()) < 0 or int(ids.max()) >= self.shape.vocab_size:
            raise ValueError(f"token id out of range [0, {self.shape.vocab_size})")
        start = 0
        while start < n:
            end = int(np.searchsorted(cu, cu[start] + max_tokens_per_call, side="right")) - 1
            end = min(max(end, start + 1), n)
            t0, t1 = int(cu[start]), int(cu[end])
            cu_c = np.ascontiguousarray(cu[start:end + 1] - t0, dtype=np.int32)
            self.encode_packed(torch.from_numpy(np.ascontiguousarray(ids[t0:t1])).to(self.device, non_blocking=True),
                               torch.from_numpy(cu_c).to(self.device, non_blocking=True), int(lens[start:end].max()),
                               out=out[start:end], cu_host=cu_c)
            start = end
        return out

    def encode_ids(self, seqs: Sequence[Sequence[int]], max_tokens_per_call: int = 1 << 18) -> torch.Tensor:
        """Host token-id lists -> embeddings [n, hidden] on the device, in input order: pack_token_ids, then
        encode_packed_host."""
        if len(seqs) == 0:
            return torch.empty((0, self.shape.hidden), dtype=torch.float32, device=self.device)
        ids, cu, _ = pack_token_ids(seqs, self.max_seq_length)
        return self.encode_packed_host(ids, cu, max_tokens_per_call)
