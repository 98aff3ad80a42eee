"""ctypes binding of libicrec.so (include/icrec.h).

The HIP library is the product: there is no CPU or PyTorch fallback.  If the
shared object is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libicrec.so"

ICREC_MAX_K = 128
ICREC_MAX_BOOSTS = 1024
ICREC_MAX_TERMS = 1024
ICREC_ADAPTER_MAX_DIM = 1024
ICREC_ADAPTER_MAX_BATCH = 1024
ICREC_ADAPTER_MAX_CANDIDATES = 8192
ICREC_ADAPTER_MAX_LIST = 1024
ICREC_MAX_FACETS = 2
ICREC_FACET_MASK_WORDS = 8
ICREC_MAX_ROWSETS = 65535
ICREC_MAX_SETS_PER_QUERY = 4
ICREC_MAX_SEQLEN = 512
COMM_ID_BYTES = 128
GEMM_F32, GEMM_F16X3 = 0, 1
GEMM_MODES = {"f32": GEMM_F32, "f16x3": GEMM_F16X3}
POOL_MEAN, POOL_CLS = 0, 1
POOLING_MODES = {"mean": POOL_MEAN, "cls": POOL_CLS}

#: every symbol include/icrec.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "icrec_encoder_weight_count", "icrec_encoder_create", "icrec_encoder_destroy", "icrec_encoder_set_max_seqlen",
    "icrec_encoder_set_pooling", "icrec_encoder_pooling",
    "icrec_encoder_set_attention_bias", "icrec_encoder_has_attention_bias",
    "icrec_encoder_set_score_head", "icrec_encoder_has_score_head",
    "icrec_score_pairs_workspace_bytes", "icrec_score_pairs",
    "icrec_assemble_pairs_workspace_bytes", "icrec_assemble_pairs", "icrec_rerank_select",
    "icrec_encode_workspace_bytes", "icrec_encode", "icrec_encode_ex", "icrec_encode_batch_split",
    "icrec_index_create", "icrec_index_create_ex", "icrec_index_destroy", "icrec_index_rows", "icrec_index_storage",
    "icrec_index_export", "icrec_index_dim", "icrec_index_device",
    "icrec_index_write_rows", "icrec_index_write_facets", "icrec_index_export_filter",
    "icrec_index_capacity", "icrec_index_reserve", "icrec_index_append_rows", "icrec_index_remove_rows",
    "icrec_comm_unique_id", "icrec_comm_init", "icrec_comm_destroy", "icrec_comm_rank", "icrec_comm_world",
    "icrec_search_sharded_workspace_bytes", "icrec_search_sharded",
    "icrec_search_sharded_excl_workspace_bytes", "icrec_search_sharded_excl", "icrec_index_row_offset",
    "icrec_exclusions_to_shard_csr_workspace_bytes", "icrec_exclusions_to_shard_csr",
    "icrec_search_workspace_bytes", "icrec_search", "icrec_search_partial", "icrec_merge_topk",
    "icrec_index_set_facets", "icrec_index_facets", "icrec_search_faceted_workspace_bytes", "icrec_search_faceted",
    "icrec_index_set_rowsets", "icrec_index_write_rowset", "icrec_index_rowsets",
    "icrec_search_in_sets_workspace_bytes", "icrec_search_in_sets",
    "icrec_mmr_select_workspace_bytes", "icrec_mmr_select",
    "icrec_boost_select_workspace_bytes", "icrec_boost_select", "icrec_compose_queries", "icrec_cap_select",
    "icrec_adapter_create", "icrec_adapter_destroy", "icrec_adapter_dim", "icrec_adapter_set_state",
    "icrec_adapter_get_state", "icrec_adapter_apply", "icrec_adapter_step_workspace_bytes", "icrec_adapter_step",
    "icrec_adapter_step_catalog_workspace_bytes", "icrec_adapter_step_catalog", "icrec_adapter_catalog_plan",
    "icrec_adapter_step_lists_workspace_bytes", "icrec_adapter_step_lists",
    "icrec_ivf_create", "icrec_ivf_destroy", "icrec_ivf_lists", "icrec_ivf_layout",
    "icrec_ivf_search_workspace_bytes", "icrec_ivf_search",
    "icrec_scores", "icrec_normalize_rows", "icrec_rank_all_workspace_bytes", "icrec_rank_all",
    "icrec_cf_create", "icrec_cf_destroy", "icrec_cf_orders", "icrec_cf_items", "icrec_cf_candidates", "icrec_cf_nnz",
    "icrec_cf_tile", "icrec_cf_rank_workspace_bytes", "icrec_cf_rank", "icrec_cf_rank_all_workspace_bytes",
    "icrec_cf_rank_all", "icrec_ir_metrics_workspace_bytes", "icrec_ir_metrics", "icrec_fuse_select",
    "icrec_tokenizer_create", "icrec_tokenizer_create_ex", "icrec_tokenizer_destroy", "icrec_tokenizer_vocab_size", "icrec_tokenize",
    "icrec_last_error", "icrec_version",
    "icrec_timing_enable", "icrec_timing_reset", "icrec_timing_query",
]


class IcrecError(RuntimeError):
    """A libicrec call returned a non-zero status."""


class BertCfg(C.Structure):
    """icrec_bert_cfg (include/icrec.h)."""

    _fields_ = [
        ("vocab_size", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32),
        ("heads", C.c_int32), ("intermediate", C.c_int32), ("max_position", C.c_int32),
        ("type_vocab", C.c_int32), ("ln_eps", C.c_float), ("n_normalize", C.c_int32),
        ("gemm_mode", C.c_int32),
    ]


def build(force: bool = False) -> Path:
    """Compile libicrec.so for gfx950 with hipcc (in-tree, next to this file)."""
    csrc = _PKG / "csrc"
    if force:
        subprocess.run(["make", "-C", str(csrc), "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", str(csrc), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libicrec.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """Load libicrec.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise IcrecError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch first: it brings its own libamdhip64 / librccl, and libicrec must resolve to THAT runtime - loaded before
    # torch it binds /opt/rocm's copy instead, the process then holds two HIP runtimes and the second one sees no
    # device ("no ROCm-capable device is detected" from hipSetDevice inside icrec_encoder_create)
    import torch  # noqa: F401

    L = C.CDLL(str(LIB_PATH))
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    sig = {
        "icrec_encoder_weight_count": (sz, [C.POINTER(BertCfg)]),
        "icrec_encoder_create": (C.c_int, [vp, sz, C.POINTER(BertCfg), C.c_int, C.POINTER(vp)]),
        "icrec_encoder_destroy": (C.c_int, [vp]),
        "icrec_encoder_set_max_seqlen": (C.c_int, [vp, i32]),
        "icrec_encoder_set_pooling": (C.c_int, [vp, i32]),
        "icrec_encoder_pooling": (i32, [vp]),
        "icrec_encoder_set_attention_bias": (C.c_int, [vp, vp, i32]),
        "icrec_encoder_has_attention_bias": (i32, [vp]),
        "icrec_encoder_set_score_head": (C.c_int, [vp, vp, vp, vp, vp]),
        "icrec_encoder_has_score_head": (i32, [vp]),
        "icrec_score_pairs_workspace_bytes": (sz, [vp, i64, i32]),
        "icrec_score_pairs": (C.c_int, [vp, vp, vp, vp, i32, i64, i32, vp, vp, sz, vp]),
        "icrec_assemble_pairs_workspace_bytes": (sz, [i32, i32]),
        "icrec_assemble_pairs": (C.c_int, [vp, vp, i32, vp, vp, i64, i64, vp, i32, i32, i32, i32, vp, i64, vp, vp, vp, sz,
                                           C.c_int, vp]),
        "icrec_rerank_select": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, vp, C.c_int, vp]),
        "icrec_encode_workspace_bytes": (sz, [vp, i64, i32]),
        "icrec_encode": (C.c_int, [vp, vp, vp, i32, i64, i32, vp, vp, sz, vp]),
        "icrec_encode_ex": (C.c_int, [vp, vp, vp, i32, i64, i32, vp, vp, vp, sz, vp]),
        "icrec_encode_batch_split": (C.c_int, [vp, i64, C.POINTER(i64), C.POINTER(i64)]),
        "icrec_index_create": (C.c_int, [vp, i64, i32, i64, C.c_int, C.POINTER(vp)]),
        "icrec_index_create_ex": (C.c_int, [vp, i64, i32, i64, C.c_int, i32, C.POINTER(vp)]),
        "icrec_index_storage": (i32, [vp]),
        "icrec_index_dim": (i32, [vp]),
        "icrec_index_device": (i32, [vp]),
        "icrec_comm_unique_id": (C.c_int, [vp]),
        "icrec_comm_init": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "icrec_comm_destroy": (C.c_int, [vp]),
        "icrec_comm_rank": (i32, [vp]),
        "icrec_comm_world": (i32, [vp]),
        "icrec_search_sharded_workspace_bytes": (sz, [vp, vp, i32, i32]),
        "icrec_search_sharded": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
        "icrec_search_sharded_excl_workspace_bytes": (sz, [vp, vp, i32, i32, i32]),
        "icrec_search_sharded_excl": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, sz, vp]),
        "icrec_exclusions_to_shard_csr_workspace_bytes": (sz, [i32, i32]),
        "icrec_exclusions_to_shard_csr": (C.c_int, [vp, vp, i32, i32, i32, i64, i64, vp, vp, vp, sz, C.c_int, vp]),
        "icrec_index_row_offset": (i64, [vp]),
        "icrec_index_destroy": (C.c_int, [vp]),
        "icrec_index_rows": (i64, [vp]),
        "icrec_index_export": (C.c_int, [vp, vp, vp]),
        "icrec_index_write_rows": (C.c_int, [vp, vp, vp, i32, vp]),
        "icrec_index_write_facets": (C.c_int, [vp, vp, vp, i32]),
        "icrec_index_export_filter": (C.c_int, [vp, vp, vp, vp]),
        "icrec_index_capacity": (i64, [vp]),
        "icrec_index_reserve": (C.c_int, [vp, i64]),
        "icrec_index_append_rows": (C.c_int, [vp, vp, i32, vp, vp]),
        "icrec_index_remove_rows": (C.c_int, [vp, vp, i32, vp, vp, vp, vp]),
        "icrec_search_workspace_bytes": (sz, [vp, i32, i32]),
        "icrec_search": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
        "icrec_search_partial": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]),
        "icrec_index_set_facets": (C.c_int, [vp, vp, i32]),
        "icrec_index_facets": (i32, [vp]),
        "icrec_search_faceted_workspace_bytes": (sz, [vp, i32, i32]),
        "icrec_search_faceted": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
        "icrec_index_set_rowsets": (C.c_int, [vp, vp, i32]),
        "icrec_index_write_rowset": (C.c_int, [vp, i32, vp]),
        "icrec_index_rowsets": (i32, [vp]),
        "icrec_search_in_sets_workspace_bytes": (sz, [vp, i32, i32]),
        "icrec_search_in_sets": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, sz, vp]),
        "icrec_mmr_select_workspace_bytes": (sz, [vp, i32, i32]),
        "icrec_mmr_select": (C.c_int, [vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp, sz, vp]),
        "icrec_boost_select_workspace_bytes": (sz, [vp, i32, i32]),
        "icrec_boost_select": (C.c_int, [vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, sz, vp]),
        "icrec_compose_queries": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp]),
        "icrec_cap_select": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "icrec_adapter_create": (C.c_int, [i32, C.c_int, C.POINTER(vp)]),
        "icrec_adapter_destroy": (C.c_int, [vp]),
        "icrec_adapter_dim": (i32, [vp]),
        "icrec_adapter_set_state": (C.c_int, [vp, vp, vp, vp, i64]),
        "icrec_adapter_get_state": (C.c_int, [vp, vp, vp, vp, C.POINTER(i64)]),
        "icrec_adapter_apply": (C.c_int, [vp, vp, i32, vp, vp]),
        "icrec_adapter_step_workspace_bytes": (sz, [vp, i32, i32]),
        "icrec_adapter_step": (C.c_int, [vp, vp, vp, i32, vp, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         C.c_float, i32, vp, vp, vp, sz, vp]),
        "icrec_adapter_step_catalog_workspace_bytes": (sz, [vp, vp, i32]),
        "icrec_adapter_step_catalog": (C.c_int, [vp, vp, vp, i32, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                                 C.c_float, i32, vp, vp, vp, sz, vp]),
        "icrec_adapter_catalog_plan": (C.c_int, [vp, i32, i64, C.POINTER(i32), C.POINTER(i64)]),
        "icrec_adapter_step_lists_workspace_bytes": (sz, [vp, i32]),
        "icrec_adapter_step_lists": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, i32, C.c_float, C.c_float, C.c_float, C.c_float,
                                               C.c_float, C.c_float, i32, vp, vp, vp, sz, vp]),
        "icrec_ivf_create": (C.c_int, [vp, vp, i32, C.POINTER(vp)]),
        "icrec_ivf_destroy": (C.c_int, [vp]),
        "icrec_ivf_lists": (i32, [vp]),
        "icrec_ivf_layout": (C.c_int, [vp, vp, vp, vp]),
        "icrec_ivf_search_workspace_bytes": (sz, [vp, i32, i32, i32]),
        "icrec_ivf_search": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
        "icrec_merge_topk": (C.c_int, [vp, i32, i32, i32, vp, vp, C.c_int, vp]),
        "icrec_scores": (C.c_int, [vp, vp, i32, vp, vp, sz, vp]),
        "icrec_rank_all_workspace_bytes": (sz, [vp, i32]),
        "icrec_rank_all": (C.c_int, [vp, vp, i32, vp, vp, sz, vp]),
        "icrec_cf_create": (C.c_int, [vp, vp, i64, i64, i64, C.c_int, C.POINTER(vp)]),
        "icrec_cf_destroy": (C.c_int, [vp]),
        "icrec_cf_orders": (i64, [vp]),
        "icrec_cf_items": (i64, [vp]),
        "icrec_cf_candidates": (i64, [vp]),
        "icrec_cf_nnz": (i64, [vp]),
        "icrec_cf_tile": (i32, [vp]),
        "icrec_cf_rank_workspace_bytes": (sz, [vp, i32, i32]),
        "icrec_cf_rank": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, sz, vp]),
        "icrec_cf_rank_all_workspace_bytes": (sz, [vp, i32]),
        "icrec_cf_rank_all": (C.c_int, [vp, vp, vp, i32, vp, vp, sz, vp]),
        "icrec_ir_metrics_workspace_bytes": (sz, [i32]),
        "icrec_ir_metrics": (C.c_int, [vp, i32, vp, vp, i32, vp, vp, vp, sz, C.c_int, vp]),
        "icrec_fuse_select": (C.c_int, [vp, vp, i32, vp, vp, vp, i32, vp, i32, i64, vp, vp, i32, vp, vp, vp, C.c_int, vp]),
        "icrec_normalize_rows": (C.c_int, [vp, vp, i64, i32, C.c_float, C.c_int, vp]),
        "icrec_tokenizer_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]),
        "icrec_tokenizer_create_ex": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                                C.c_char_p, C.POINTER(vp)]),
        "icrec_tokenizer_destroy": (C.c_int, [vp]),
        "icrec_tokenizer_vocab_size": (i32, [vp]),
        "icrec_tokenize": (C.c_int, [vp, C.POINTER(C.c_char_p), i32, vp, i64, vp, i32]),
        "icrec_last_error": (C.c_char_p, []),
        "icrec_version": (C.c_char_p, []),
        "icrec_timing_enable": (C.c_int, [C.c_int]),
        "icrec_timing_reset": (C.c_int, []),
        "icrec_timing_query": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(i64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().icrec_last_error().decode("utf-8", "replace")
        raise IcrecError(f"{what} failed (status {rc}): {msg}")


def ptr(t) -> C.c_void_p:
    """A tensor's address as a `void *` argument; NULL for None."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream_ptr(device) -> C.c_void_p:
    """The current stream of a HIP device as a `hipStream_t` argument."""
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def hip_device(device, who: str):
    """`device` as a torch.device with its index filled in; anything but a cuda/HIP device raises."""
    import torch

    dev = torch.device(device)
    if dev.type != "cuda":
        raise IcrecError(f"{who} needs a CUDA/HIP device; there is no CPU fallback")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


class StreamScratch(dict):
    """Grow-only scratch blocks by stream handle, ONE PER STREAM: calls issued on different streams (pipeline.py
    searches on a side stream while the caller may use the same object from its own) never share scratch memory, and
    a block is only ever allocated, used and dropped on the stream it belongs to, so the caching allocator's
    stream-ordered reuse is safe when it grows."""

    def __init__(self, device):
        super().__init__()
        self.device = device

    def block(self, need: int):
        """The current stream's block, at least `need` bytes."""
        import torch

        key = torch.cuda.current_stream(self.device).cuda_stream
        if key not in self or self[key].numel() < need:
            self.pop(key, None)  # the old block is freed before the larger one is allocated
            self[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self[key]


def mmr_select(index_handle, cand_idx, rel, top_k: int, lam: float, out_idx, out_rel, ws, device) -> None:
    """icrec_mmr_select on device tensors: cand_idx int64 [Q, k] and rel float32 [Q, k] in, out_idx int64 [Q, top_k]
    and out_rel float32 [Q, top_k] out, ws a uint8 scratch tensor; asynchronous on `device`'s current stream."""
    Q, k = int(cand_idx.shape[0]), int(cand_idx.shape[1])
    check(lib().icrec_mmr_select(index_handle, ptr(cand_idx), ptr(rel), Q, k, int(top_k), float(lam), ptr(out_idx),
                                 ptr(out_rel), ptr(ws), ws.numel(), stream_ptr(device)), "icrec_mmr_select")


def boost_select(index_handle, q, cand_idx, cand_score, boost_off, boost_rows, boost_w, max_boosts: int, excl_idx,
                 excl_off, allow, top_k: int, out_idx, out_score, ws, device) -> None:
    """icrec_boost_select on device tensors: q float32 [Q, dim], cand_idx int64 [Q, k] and cand_score float32 [Q, k] (both
    None: no candidates), the lists as boost_off int32 [Q+1], boost_rows int32 and boost_w float32 (or None), the search's
    exclusion CSR and allow masks or None, out_idx int64 [Q, top_k] and out_score float32 [Q, top_k] out, ws a uint8
    scratch tensor; asynchronous on `device`'s current stream."""
    Q = int(q.shape[0])
    k = int(cand_idx.shape[1]) if cand_idx is not None else 0
    check(lib().icrec_boost_select(index_handle, ptr(q), Q, ptr(cand_idx), ptr(cand_score), k, ptr(boost_off),
                                   ptr(boost_rows), ptr(boost_w), int(max_boosts), ptr(excl_idx), ptr(excl_off), ptr(allow),
                                   int(top_k), ptr(out_idx), ptr(out_score), ptr(ws), ws.numel(), stream_ptr(device)),
          "icrec_boost_select")


def compose_queries(index_handle, base, base_w, n_queries: int, term_off, term_rows, term_w, max_terms: int, out,
                    device) -> None:
    """icrec_compose_queries on device tensors: base float32 [Q, dim] and base_w float32 [Q] (or None), the terms as
    term_off int32 [Q+1], term_rows int32 and term_w float32 (or None), out float32 [Q, dim]; asynchronous on `device`'s
    current stream."""
    check(lib().icrec_compose_queries(index_handle, ptr(base), ptr(base_w), int(n_queries), ptr(term_off), ptr(term_rows),
                                      ptr(term_w), int(max_terms), ptr(out), stream_ptr(device)), "icrec_compose_queries")


def cap_select(index_handle, cand_idx, cand_score, caps, n_prior, allow, top_k: int, out_idx, out_score, out_state,
               allow_next, device) -> None:
    """icrec_cap_select on device tensors: cand_idx int64 [Q, k] and cand_score float32 [Q, k] in, caps int32
    [Q, ICREC_MAX_FACETS], n_prior int32 [Q] or None, allow uint32 [Q, n_facets, 8] or None, out_idx int64 [Q, top_k] and
    out_score float32 [Q, top_k] (in/out with n_prior), out_state int32 [Q, 2] out, allow_next like allow (or allow
    itself) or None; asynchronous on `device`'s current stream."""
    Q, k = int(cand_idx.shape[0]), int(cand_idx.shape[1])
    check(lib().icrec_cap_select(index_handle, ptr(cand_idx), ptr(cand_score), Q, k, ptr(caps), ptr(n_prior), ptr(allow),
                                 int(top_k), ptr(out_idx), ptr(out_score), ptr(out_state), ptr(allow_next),
                                 stream_ptr(device)), "icrec_cap_select")


def fuse_select(a_idx, a_gate, a_w, b_idx, b_gate, b_w, n_ids: int, excl_idx, excl_off, top_k: int, out_idx, out_score,
                out_pos, device) -> None:
    """icrec_fuse_select on device tensors: a_idx int64 [Q, ka] and b_idx int64 [Q, kb] in, their gates int32 of the
    same shapes or None, a_w float32 [ka] and b_w float32 [kb], the search's exclusion CSR or None, out_idx int64
    [Q, top_k] and out_score float32 [Q, top_k] out, out_pos int32 [Q, top_k, 2] or None; asynchronous on `device`'s
    current stream."""
    Q, ka, kb = int(a_idx.shape[0]), int(a_idx.shape[1]), int(b_idx.shape[1])
    check(lib().icrec_fuse_select(ptr(a_idx), ptr(a_gate), ka, ptr(a_w), ptr(b_idx), ptr(b_gate), kb, ptr(b_w), Q, int(n_ids),
                                  ptr(excl_idx), ptr(excl_off), int(top_k), ptr(out_idx), ptr(out_score), ptr(out_pos),
                                  device.index, stream_ptr(device)), "icrec_fuse_select")


def timing_enable(on: bool) -> None:
    lib().icrec_timing_enable(1 if on else 0)


def timing_reset() -> None:
    lib().icrec_timing_reset()


def timing_query(which: int) -> tuple[float, int]:
    """(average ms, launches) for slot `which` — see icrec_timing_query in include/icrec.h."""
    ms, n = C.c_double(0.0), C.c_int64(0)
    check(lib().icrec_timing_query(which, C.byref(ms), C.byref(n)), "icrec_timing_query")
    return ms.value, n.value
