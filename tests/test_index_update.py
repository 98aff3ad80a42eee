"""Rewriting an index in place, the parts that need no GPU: the three entry points are declared, exported and bound and
refuse bad arguments before any HIP call; product_update_plan's checks; DeviceIndex.write_rows' host checks, which
precede every device call."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from instacart_next_order_recommendation_amd.recommender import catalog_facets, product_update_plan

ROOT = Path(__file__).resolve().parents[1]
NEW = ("icrec_index_write_rows", "icrec_index_write_facets", "icrec_index_export_filter")


@pytest.fixture(scope="module")
def native():
    from instacart_next_order_recommendation_amd import _native

    if not _native.LIB_PATH.exists():
        _native.build()
    return _native


def test_symbols_are_declared_exported_and_bound(native):
    header = (ROOT / "include" / "icrec.h").read_text()
    declared = set(re.findall(r"ICREC_API\s+[\w\s\*]+?\b(icrec_\w+)\s*\(", header))
    lib = native.lib()
    for name in NEW:
        assert name in declared and name in native.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.icrec_index_write_rows.argtypes) == 5
    assert len(lib.icrec_index_write_facets.argtypes) == 4
    assert len(lib.icrec_index_export_filter.argtypes) == 4
    assert "12 = icrec_index_write_rows" in header                                       # the timer slot is documented
    ms, n = native.timing_query(12)
    assert (ms, n) == (0.0, 0)
    with pytest.raises(native.IcrecError):
        native.timing_query(13)


def test_refusals_come_before_any_hip_call(native):
    """A NULL handle is refused first, so on a machine without a GPU these return ICREC_EINVAL (-1) and not a HIP
    error; m == 0 on a NULL handle is still a NULL handle."""
    lib = native.lib()
    buf = (C.c_int32 * 4)()
    p = C.cast(buf, C.c_void_p)
    assert lib.icrec_index_write_rows(None, p, p, 1, None) == -1 and b"NULL index" in lib.icrec_last_error()
    assert lib.icrec_index_write_rows(None, p, p, 0, None) == -1
    assert lib.icrec_index_write_rows(None, p, p, -1, None) == -1
    assert lib.icrec_index_write_facets(None, p, p, 1) == -1 and b"NULL index" in lib.icrec_last_error()
    assert lib.icrec_index_write_facets(None, p, p, -1) == -1
    assert lib.icrec_index_export_filter(None, p, p, None) == -1 and b"NULL" in lib.icrec_last_error()


# ---------------------------------------------------------------- product_update_plan
TEXTS = ["Product: Milk. Aisle: dairy. Department: fresh.", "Product: Rye. Aisle: bread. Department: bakery.",
         "Product: Brie. Aisle: dairy. Department: fresh.", "Product: Bun. Aisle: bread. Department: bakery."]
PIDS = {"10": 0, "11": 1, "12": 2, "13": 3}


def catalog():
    aisles, departments, codes = catalog_facets(TEXTS)
    assert aisles == ["dairy", "bread"] and departments == ["fresh", "bakery"]
    return aisles, departments, codes


def test_plan_unknown_id_and_bad_text():
    aisles, departments, _ = catalog()
    with pytest.raises(ValueError, match="unknown product id '99'"):
        product_update_plan({"10": TEXTS[1], "99": TEXTS[0]}, PIDS, TEXTS, aisles, departments)
    with pytest.raises(ValueError, match="format"):
        product_update_plan({"10": "Oat milk, one litre"}, PIDS, TEXTS, aisles, departments)
    with pytest.raises(ValueError, match="format"):
        product_update_plan({"10": "Product: Milk. Aisle: dairy. Department: fresh"}, PIDS, TEXTS, aisles, departments)
    with pytest.raises(ValueError, match="string"):
        product_update_plan({"10": None}, PIDS, TEXTS, aisles, departments)
    with pytest.raises(ValueError, match="mapping"):
        product_update_plan(["10"], PIDS, TEXTS, aisles, departments)
    assert aisles == ["dairy", "bread"] and departments == ["fresh", "bakery"]           # the caller's lists are not touched


def test_plan_appends_new_names_and_keeps_the_old_codes():
    aisles, departments, codes = catalog()
    updates = {"13": "Product: Bun. Aisle: frozen dough. Department: frozen.",            # given out of row order
               "10": "Product: Milk. Aisle: bread. Department: fresh.",
               "12": "Product: Camembert. Aisle: dairy. Department: fresh."}
    rows, texts, new_codes, a2, d2 = product_update_plan(updates, PIDS, TEXTS, aisles, departments)
    assert rows == [0, 2, 3] and texts == [updates["10"], updates["12"], updates["13"]]
    assert a2 == ["dairy", "bread", "frozen dough"] and d2 == ["fresh", "bakery", "frozen"]
    assert new_codes.dtype == np.uint8 and new_codes.tolist() == [[1, 0], [0, 0], [2, 2]]
    assert aisles == ["dairy", "bread"] and departments == ["fresh", "bakery"]           # copies, not the caller's lists
    # the codes of the untouched rows still mean what they meant
    assert [a2[c] for c in codes[:, 0]] == [aisles[c] for c in codes[:, 0]]


def test_plan_the_257th_name():
    aisles = [f"a{i}" for i in range(256)]
    departments = ["d"]
    texts = [f"Product: P. Aisle: a{i}. Department: d." for i in range(256)]
    pids = {str(i): i for i in range(256)}
    rows, _, codes, a2, _ = product_update_plan({"7": "Product: P. Aisle: a255. Department: d."}, pids, texts, aisles, departments)
    assert rows == [7] and codes.tolist() == [[255, 0]] and len(a2) == 256
    with pytest.raises(ValueError, match="257th aisle"):
        product_update_plan({"7": "Product: P. Aisle: one more. Department: d."}, pids, texts, aisles, departments)
    with pytest.raises(ValueError, match="257th department"):
        product_update_plan({"7": "Product: P. Aisle: a1. Department: one more."}, pids, texts, aisles,
                            [f"d{i}" for i in range(256)])


def test_plan_empty_mapping_and_catalog_without_facets():
    aisles, departments, _ = catalog()
    rows, texts, codes, a2, d2 = product_update_plan({}, PIDS, TEXTS, aisles, departments)
    assert rows == [] and texts == [] and codes.shape == (0, 2) and (a2, d2) == (aisles, departments)
    rows, texts, codes, a2, d2 = product_update_plan({"11": "free text, no markers"}, PIDS, TEXTS, None, None)
    assert rows == [1] and texts == ["free text, no markers"] and codes is None and a2 is None and d2 is None
    assert product_update_plan({}, PIDS, TEXTS, None, None) == ([], [], None, None, None)


# ---------------------------------------------------------------- DeviceIndex.write_rows without a device
def bare_index(n_rows=10, dim=32):
    """A DeviceIndex that owns nothing: the host checks read n_rows and dim only, and a check that lets a bad argument
    through fails on the missing device attributes, loudly."""
    from instacart_next_order_recommendation_amd.search import DeviceIndex

    ix = DeviceIndex.__new__(DeviceIndex)
    ix.n_rows, ix.dim = n_rows, dim
    return ix


def test_write_rows_refuses_bad_host_arguments_without_a_device(native):
    ix = bare_index()
    rows = np.ones((3, 32), np.float32)
    with pytest.raises(ValueError, match="named twice"):
        ix.write_rows([4, 2, 4], rows)
    with pytest.raises(ValueError, match="outside"):
        ix.write_rows([1, 2, 10], rows)
    with pytest.raises(ValueError, match="outside"):
        ix.write_rows([-1, 2, 3], rows)
    with pytest.raises(ValueError, match="3 integers"):
        ix.write_rows([1, 2], rows)
    with pytest.raises(ValueError, match="3 integers"):
        ix.write_rows([1.0, 2.0, 3.0], rows)
    with pytest.raises(ValueError, match=r"\[m, 32\]"):
        ix.write_rows([1, 2, 3], np.ones((3, 64), np.float32))
    with pytest.raises(ValueError, match=r"\[m, 32\]"):
        ix.write_rows([1], np.ones(32, np.float32))
    ix.write_rows([], np.ones((0, 32), np.float32))                                      # nothing to write: no device call
    ids, order = ix._sorted_rows([7, 0, 3], 3, "t")
    assert ids.dtype == np.int32 and ids.tolist() == [0, 3, 7] and order.tolist() == [1, 2, 0]
