"""Item-item CF baseline and IR metrics without a GPU: the plain-Python reference against what the upstream project's
own classes returned on tests/golden/cf_small (tools/make_cf_fixture.py), the CSV loader, and the C ABI's refusals."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import cf_cases, cf_reference

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def rec():
    return cf_cases.load_fixture()


def test_fixture_holds_the_edge_cases(rec):
    baskets = rec["baskets"]
    corpus = set(rec["corpus_ids"])
    assert any(len(b) != len(set(b)) for b in baskets.values())            # a product twice in one order
    assert rec["histories"]["999999"] == []                                 # an eval query orders.csv does not know
    bought = {p for b in baskets.values() for p in b}
    assert bought - corpus and corpus - bought                              # outside the corpus / bought by nobody
    assert sum(1 for h in rec["histories"].values() if not h) >= 2          # ... and a user without a prior order
    assert sum(f.stat().st_size for f in cf_cases.FIXTURE.rglob("*") if f.is_file()) < 200_000


def test_reference_reproduces_upstream_rankings(rec):
    baskets, histories, n_cand, _, qids = cf_cases.fixture_as_items(rec)
    ranked = cf_reference.cf_rank(baskets, histories, n_cand)
    for qid, (rows, _) in zip(qids, ranked):
        assert [rec["corpus_ids"][r] for r in rows] == rec["rankings"][qid], qid


def test_numpy_rank_equals_the_reference(rec):
    """cf_cases.numpy_rank, which the large GPU cases are held against, is the plain-Python reference in matrix form."""
    from tests.test_cf_gpu import SHAPES

    baskets, histories, n_cand, _, _ = cf_cases.fixture_as_items(rec)
    cases = [(baskets, histories, n_cand)]
    for n_cand, extra, n_orders, Q in (SHAPES[2], SHAPES[4]):            # (63, 0, 257, 33) and (1000, 37, 257, 33)
        n_items = n_cand + extra
        baskets = cf_cases.synthetic_baskets(n_orders, n_items, seed=n_cand + n_orders)
        assert any(len(b) != len(set(b)) for b in baskets) and any(not b for b in baskets)
        histories = cf_cases.synthetic_histories(Q, n_items, seed=Q)
        histories[3] = [-3] + histories[3] + [n_items + 5]              # ids outside the catalog count for nothing
        cases.append((baskets, histories, n_cand))
    for baskets, histories, n_cand in cases:
        for k in (None, 1, 20, n_cand + 3):
            assert cf_cases.numpy_rank(baskets, histories, n_cand, k) == cf_reference.cf_rank(baskets, histories, n_cand, k)
        off, items = cf_cases.as_csr(baskets)
        assert cf_cases.numpy_rank((off, items.astype(np.int32)), histories, n_cand) == cf_reference.cf_rank(baskets, histories, n_cand)
    assert cf_cases.numpy_rank([[0, 1], [1, 2]], [[-3, 1, 8]], 3) == cf_reference.cf_rank([[0, 1], [1, 2]], [[1]], 3)


def test_reference_reproduces_upstream_metrics(rec):
    import json

    relevant = {q: set(v) for q, v in json.loads((cf_cases.FIXTURE / "processed" / "eval_relevant_docs.json").read_text()).items()}
    got = cf_reference.ir_metrics(rec["rankings"], relevant)
    n = sum(1 for q in rec["rankings"] if relevant.get(q))
    assert set(got) == set(rec["metrics"]) == set(cf_reference.METRIC_KEYS)
    for key, want in rec["metrics"].items():
        print(key, got[key], want, got[key] - want)
        if key.startswith("accuracy"):
            assert got[key] == want, key
        else:  # the worst case of re-ordering a sum of n terms in [0, 1]
            assert abs(got[key] - want) <= n * 2.0 ** -52, key


def test_csv_loader_reproduces_upstream_selection(rec):
    from instacart_next_order_recommendation_amd.baselines import ItemItemCFBaseline

    got = ItemItemCFBaseline.load_arrays(cf_cases.FIXTURE / "data", cf_cases.FIXTURE / "processed")
    assert got["corpus_ids"] == rec["corpus_ids"]
    assert got["baskets"] == list(rec["baskets"].values())
    assert {q: sorted(h) for q, h in got["histories"].items()} == rec["histories"]


@pytest.fixture(scope="module")
def native():
    from instacart_next_order_recommendation_amd import _native

    if not _native.LIB_PATH.exists():
        _native.build()
    return _native


CF_SYMBOLS = {"icrec_cf_create", "icrec_cf_destroy", "icrec_cf_orders", "icrec_cf_items", "icrec_cf_candidates", "icrec_cf_nnz",
              "icrec_cf_rank_workspace_bytes", "icrec_cf_rank", "icrec_cf_rank_all_workspace_bytes", "icrec_cf_rank_all",
              "icrec_ir_metrics_workspace_bytes", "icrec_ir_metrics"}


def test_abi_additions_declared_and_bound(native):
    header = (ROOT / "include" / "icrec.h").read_text()
    declared = set(re.findall(r"ICREC_API\s+[\w\s\*]+?\b(icrec_\w+)\s*\(", header))
    assert CF_SYMBOLS <= declared and CF_SYMBOLS <= set(native.EXPORTS)
    lib = native.lib()
    for name in CF_SYMBOLS:
        assert getattr(lib, name).argtypes is not None, name


def test_create_refuses_bad_baskets_before_touching_a_device(native):
    lib = native.lib()

    def create(off, items, n_items, n_cand):
        off, items = np.asarray(off, np.int64), np.asarray(items, np.int32)
        h = C.c_void_p()
        rc = lib.icrec_cf_create(off.ctypes.data_as(C.c_void_p), items.ctypes.data_as(C.c_void_p), len(off) - 1, n_items,
                                 n_cand, 0, C.byref(h))
        return rc, lib.icrec_last_error()

    rc, msg = create([0, 2], [0, 5], 5, 5)
    assert rc == -1 and b"outside" in msg
    rc, msg = create([0, 2], [0, -1], 5, 5)
    assert rc == -1 and b"outside" in msg
    rc, msg = create([0, 2, 1], [0, 1], 5, 5)
    assert rc == -1 and b"decreases" in msg
    rc, msg = create([0, 1], [0], 5, 6)
    assert rc == -1 and b"n_candidates" in msg
    rc, msg = create([0, 1], [0], 2 ** 32 + 5, 2 ** 32 + 1)
    assert rc == -1
    rc, msg = create([0, 1], [0], 400_000, 10)   # no tile narrow enough for the LDS membership words
    assert rc == -1 and b"LDS" in msg
    rc, msg = create([0, 1], [0], 327_681, 10)   # one item past the 4-query tile's 163,840 bytes
    assert rc == -1 and b"LDS" in msg
    assert lib.icrec_cf_create(None, None, 1, 1, 1, 0, None) == -1


def test_calls_refuse_bad_arguments_without_a_device(native):
    lib = native.lib()
    assert lib.icrec_cf_orders(None) == 0 and lib.icrec_cf_items(None) == 0
    assert lib.icrec_cf_candidates(None) == 0 and lib.icrec_cf_nnz(None) == 0
    assert lib.icrec_cf_rank_workspace_bytes(None, 4, 20) == 0 and lib.icrec_cf_rank_all_workspace_bytes(None, 4) == 0
    assert lib.icrec_cf_rank(None, None, None, 1, 1, None, None, None, 0, None) == -1
    assert lib.icrec_cf_rank_all(None, None, None, 1, None, None, 0, None) == -1
    assert lib.icrec_cf_destroy(None) == 0
    assert lib.icrec_ir_metrics_workspace_bytes(0) == 0 and lib.icrec_ir_metrics_workspace_bytes(3) == 3 * 9 * 8
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.icrec_ir_metrics(None, 10, p, p, 1, p, None, p, 512, 0, None) == -1
    assert lib.icrec_ir_metrics(p, 0, p, p, 1, p, None, p, 512, 0, None) == -1 and b"depth" in lib.icrec_last_error()
    assert lib.icrec_ir_metrics(p, 129, p, p, 1, p, None, p, 512, 0, None) == -1
    assert lib.icrec_ir_metrics(p, 10, p, p, 0, p, None, p, 512, 0, None) == -1
    assert lib.icrec_ir_metrics(p, 10, p, p, 4, p, None, p, 8, 0, None) == -3   # workspace too small


def test_no_gpu_means_loud_failure(native):
    import torch

    if torch.cuda.is_available():
        return
    from instacart_next_order_recommendation_amd.baselines import ItemItemCFBaseline
    from instacart_next_order_recommendation_amd.ir_metrics import compute_ir_metrics

    with pytest.raises(Exception):
        ItemItemCFBaseline.from_arrays([["a", "b"]], {"q": ["a"]}, ["a", "b"])
    with pytest.raises(native.IcrecError):
        compute_ir_metrics({"q": ["a"]}, {"q": {"a"}}, device="cpu")
