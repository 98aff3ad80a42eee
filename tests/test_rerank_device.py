"""Device reranking without a GPU: the three entry points are exported and bound, the host-side token bound covers
model_io.assemble_pairs' exact total for every assembly case of tests/rerank_cases.py, the cases reach every arm of the
truncation rule, and the argument refusals - all made before any device call - return ICREC_EINVAL."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.reranker import pair_token_bound
from tests import rerank_cases as rc

SYMBOLS = ["icrec_assemble_pairs_workspace_bytes", "icrec_assemble_pairs", "icrec_rerank_select"]


def test_symbols_are_exported_and_bound():
    lib = _native.lib()
    header = (_native._PKG.parent / "include" / "icrec.h").read_text()
    for name in SYMBOLS:
        assert name in _native.EXPORTS
        assert f" {name}(" in header
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None
    assert len(lib.icrec_assemble_pairs.argtypes) == 20 and len(lib.icrec_rerank_select.argtypes) == 10
    assert lib.icrec_assemble_pairs_workspace_bytes(3, 20) >= 4 * 60
    assert lib.icrec_assemble_pairs_workspace_bytes(0, 20) == 0
    assert lib.icrec_assemble_pairs_workspace_bytes(1, _native.ICREC_MAX_K + 1) == 0


@pytest.mark.parametrize("max_len,k,n_queries", rc.ASSEMBLY_CASES)
def test_the_token_bound_covers_the_exact_total(max_len, k, n_queries):
    c = rc.assembly_case(max_len, k, n_queries)
    cat_max = max(len(s) for s in c["cat_sides"])
    bound = pair_token_bound([len(q) for q in c["q_sides"]], k, cat_max, max_len)
    ids, cu, seg_b = c["want"]
    assert bound >= int(cu[-1]) == ids.size
    assert bound <= n_queries * k * max_len
    assert int(np.diff(cu).max()) <= max(min(max_len, 3 + len(q) + cat_max) for q in c["q_sides"])
    assert int(np.diff(cu).min()) >= 3 and (seg_b >= 2).all()


def test_the_cases_reach_every_arm_of_the_truncation_rule():
    seen = set()
    for max_len, k, n_queries in rc.ASSEMBLY_CASES:
        c = rc.assembly_case(max_len, k, n_queries)
        seen |= {rc.branch(a, b, max_len) for a, b in c["pair_lens"]}
        if n_queries * k >= 63:
            assert (c["cand"] == -1).any() and (c["cand"] > rc.ROW_OFFSET + 100).any() and (c["cand"] < rc.ROW_OFFSET).any()
        assert any(len(q) == 2048 for q in c["q_sides"]) or n_queries < 7
    assert seen >= {"uncut", "product cut", "query cut", "both cut, budget odd", "both cut, budget even", "tie",
                    "empty query side", "empty product side"}


def test_argument_refusals():
    """Every check comes before the first device call, so the refusals need no GPU: the pointers are never read."""
    lib = _native.lib()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)

    def assemble(**kw):
        a = dict(q_ids=p, q_cu=p, n_queries=2, cat_ids=p, cat_cu=p, n_rows=4, row_offset=0, cand=p, k=5, max_len=16, cls=1,
                 sep=2, ids_out=p, ids_cap=160, cu_out=p, seg_b=p, ws=p, ws_bytes=256, device=0, stream=None)
        a.update(kw)
        return lib.icrec_assemble_pairs(*a.values())

    for kw in (dict(k=0), dict(k=_native.ICREC_MAX_K + 1), dict(max_len=2), dict(max_len=_native.ICREC_MAX_SEQLEN + 1),
               dict(n_queries=0), dict(n_queries=-3), dict(n_queries=1 << 24, k=128, max_len=512, ids_cap=1 << 40),
               dict(ids_cap=29), dict(q_ids=None), dict(q_cu=None), dict(cat_ids=None), dict(cat_cu=None), dict(cand=None),
               dict(ids_out=None), dict(cu_out=None), dict(seg_b=None), dict(ws=None)):
        assert assemble(**kw) == -1, kw  # ICREC_EINVAL
        assert b"icrec_assemble_pairs" in lib.icrec_last_error()
    assert assemble(ws_bytes=8) == -3  # ICREC_ENOMEM

    def select(**kw):
        a = dict(logits=p, cand=p, cand_score=None, n_queries=1, k=4, top_k=2, out_idx=p, out_logit=p, device=0, stream=None)
        a.update(kw)
        return lib.icrec_rerank_select(*a.values())

    for kw in (dict(k=0), dict(k=_native.ICREC_MAX_K + 1), dict(top_k=0), dict(top_k=5), dict(n_queries=0), dict(logits=None),
               dict(cand=None), dict(out_idx=None), dict(out_logit=None)):
        assert select(**kw) == -1, kw
        assert b"icrec_rerank_select" in lib.icrec_last_error()
    assert not any(buf)
