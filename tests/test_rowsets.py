"""Row sets without a device: the five C entry points are exported, bound and reject a NULL handle, rowset_bits puts
every row's bit where icrec.h says, rowset_ids fills the slots, the header and the binding agree on the two constants,
and the recommender resolves names and filters boost lists on the host, on a stub index."""
from __future__ import annotations

import json
import re
from pathlib import Path

import numpy as np
import pytest

from instacart_next_order_recommendation_amd.recommender import (Recommender, ann_plan, boost_plan, boosts_within,
                                                                 load_product_sets, within_ids, within_plan)
from instacart_next_order_recommendation_amd.search import rowset_bits, rowset_ids
from tests.rowset_cases import EDGE, HALF, KINDS, N, N_SETS, admitted_by_sets, mixed_ids, standard_sets

ROWSET_SYMBOLS = {
    "icrec_index_set_rowsets": "int(void*, void*, int32)",
    "icrec_index_write_rowset": "int(void*, int32, void*)",
    "icrec_index_rowsets": "int32(void*)",
    "icrec_search_in_sets_workspace_bytes": "size_t(void*, int32, int32)",
    "icrec_search_in_sets": "int(void*, void*, int32, int32, void*, void*, void*, void*, int32, void*, void*, void*, size_t, void*)",
}
ICREC_EINVAL = -1


@pytest.fixture(scope="module")
def native():
    from instacart_next_order_recommendation_amd import _native

    if not _native.LIB_PATH.exists():
        _native.build()
    return _native


def test_symbols_exported_and_bound(native):
    import ctypes as C

    lib = native.lib()
    name_of = {C.c_void_p: "void*", C.c_int32: "int32", C.c_size_t: "size_t", C.c_int: "int"}
    if C.c_int is C.c_int32:
        name_of[C.c_int] = "int32"
    for name, sig in ROWSET_SYMBOLS.items():
        assert name in native.EXPORTS, name
        fn = getattr(lib, name)
        got = f"{name_of[fn.restype]}({', '.join(name_of[a] for a in fn.argtypes)})"
        assert got == sig.replace("int(", name_of[C.c_int] + "("), (name, got)


def test_header_and_binding_agree_on_the_constants(native):
    header = (Path(__file__).resolve().parent.parent / "include" / "icrec.h").read_text()
    for name in ("ICREC_MAX_ROWSETS", "ICREC_MAX_SETS_PER_QUERY"):
        m = re.search(rf"^#define {name} (\d+)$", header, re.M)
        assert m and int(m.group(1)) == getattr(native, name), name
    assert native.ICREC_MAX_ROWSETS == 65535 and native.ICREC_MAX_SETS_PER_QUERY == 4
    for name in ROWSET_SYMBOLS:
        assert re.search(rf"ICREC_API \w+ {name}\(", header), name


def test_null_handle(native):
    """Every entry point answers a NULL handle before it touches a GPU."""
    lib = native.lib()
    assert lib.icrec_index_rowsets(None) == -1
    assert lib.icrec_search_in_sets_workspace_bytes(None, 4, 20) == 0
    bits = np.zeros((2, 3), np.uint32)
    p = bits.ctypes.data
    assert lib.icrec_index_set_rowsets(None, p, 2) == ICREC_EINVAL
    assert lib.icrec_index_set_rowsets(None, None, 0) == ICREC_EINVAL
    assert lib.icrec_index_write_rowset(None, 0, p) == ICREC_EINVAL
    assert lib.icrec_search_in_sets(None, p, 1, 1, None, None, None, p, 1, p, p, p, 1 << 20, None) == ICREC_EINVAL
    assert b"NULL" in lib.icrec_last_error()


@pytest.mark.parametrize("n", [64, 70, 2085, 33])
def test_rowset_bits_packing(n):
    """Rows 0, 31, 32 and n - 1, with n % 32 zero and non-zero: bit r & 31 of word r >> 5."""
    rows = sorted({0, 31, 32, n - 1})
    b = rowset_bits([rows, [], range(n), [5, 5, 5]], n)
    W = (n + 31) // 32
    assert b.dtype == np.uint32 and b.shape == (4, W)
    want = np.zeros(W, np.uint64)
    for r in rows:
        want[r >> 5] |= np.uint64(1) << np.uint64(r & 31)
    np.testing.assert_array_equal(b[0], want.astype(np.uint32))
    assert not b[1].any() and int(b[3, 0]) == 1 << 5 and b[3, 1:].sum() == 0
    full = np.full(W, 0xFFFFFFFF, np.uint32)
    if n % 32:
        full[-1] = (1 << (n % 32)) - 1                       # nothing at or past n_rows
    np.testing.assert_array_equal(b[2], full)
    member = np.zeros((4, n), bool)
    member[0, rows] = member[2] = True
    member[3, 5] = True
    np.testing.assert_array_equal(rowset_bits(member, n), b)  # the bool form
    for s in range(4):                                        # and back: bit by bit
        got = (b[s][np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1
        np.testing.assert_array_equal(got.astype(bool), member[s])


def test_rowset_bits_errors():
    with pytest.raises(ValueError, match="outside"):
        rowset_bits([[0, 64]], 64)
    with pytest.raises(ValueError, match="outside"):
        rowset_bits([[-1]], 64)
    with pytest.raises(ValueError, match="bool"):
        rowset_bits(np.zeros((2, 63), bool), 64)
    with pytest.raises(ValueError):
        rowset_bits([[0]], 0)
    assert rowset_bits([], 40).shape == (0, 2)


def test_rowset_ids_filling_and_errors():
    ids = rowset_ids([None, 3, [1, 2], [], (7, 8, 9, 10), np.int32(4)], 6)
    assert ids.dtype == np.int32
    assert ids.tolist() == [[-1] * 4, [3, -1, -1, -1], [1, 2, -1, -1], [-1] * 4, [7, 8, 9, 10], [4, -1, -1, -1]]
    assert rowset_ids([None, None], 2).tolist() == [[-1], [-1]]           # at least one slot
    assert rowset_ids([5, None], 2, 3).tolist() == [[5, -1, -1], [-1, -1, -1]]
    assert rowset_ids([[2**31 - 1, -9]], 1).tolist() == [[2**31 - 1, -9]]    # any int32 is a legal slot
    with pytest.raises(ValueError, match="entries"):
        rowset_ids([None], 2)
    with pytest.raises(ValueError, match="more than"):
        rowset_ids([[1, 2, 3, 4, 5]], 1)
    with pytest.raises(ValueError, match="sets_per_query"):
        rowset_ids([[1, 2]], 1, 1)
    for bad in (0, 5):
        with pytest.raises(ValueError, match="sets_per_query"):
            rowset_ids([None], 1, bad)
    import torch

    t = rowset_ids([[1], None], 2, 2, torch.device("cpu"))
    assert t.dtype == torch.int32 and t.tolist() == [[1, -1], [-1, -1]]


def test_shared_cases_state_the_definition():
    """tests/rowset_cases.py: the sets the search tests use and the slots they deal, against icrec.h's rules."""
    m = standard_sets()
    assert m.shape == (N_SETS, N) and not m.flags.writeable
    assert np.flatnonzero(m[EDGE]).tolist() == [0, 31, 32, 255, 256, N - 1]
    assert 0.4 < m[HALF].mean() < 0.6
    ids = mixed_ids(40)
    assert ids.shape == (40, 4) and ids[:17].tolist() == [kd + [-1] * (4 - len(kd)) for kd in KINDS]
    ok = admitted_by_sets(m, ids)
    assert ok[5].all() and not ok[7].any() and not ok[8].any()            # open; n_sets; 2^31 - 1
    np.testing.assert_array_equal(ok[9], m[EDGE])                          # a negative id is a free slot
    np.testing.assert_array_equal(ok[4], m[HALF])                          # a duplicate counts once
    assert ok[10].sum() == 3 and ok[3].sum() <= 3                          # the intersections


def test_ann_plan_refuses_within_with_probes():
    assert ann_plan(None, 16, within="store-1") is None                   # no probes: nothing to refuse
    assert ann_plan(4, 16, within=None) == 4
    with pytest.raises(ValueError, match="within"):
        ann_plan(4, 16, within="store-1")
    with pytest.raises(ValueError, match="within"):
        ann_plan(4, 16, within=[None, "store-1"])


def test_within_names():
    names = ["store-1", "store-2", "in-stock", "vegan", "kosher"]
    assert within_ids(None, names) is None and within_ids(None, None) is None
    assert within_ids("in-stock", names) == [2] and within_ids(["vegan", "store-1"], names) == [3, 0]
    assert within_ids([], names) == []
    with pytest.raises(ValueError, match="unknown product set 'nope'"):
        within_ids(["store-1", "nope"], names)
    with pytest.raises(ValueError, match="more than 4"):
        within_ids(names, names)
    with pytest.raises(ValueError, match="product_sets"):
        within_ids("store-1", None)
    assert within_plan(None, 3, names) is None and within_plan([None, None], 2, names) is None
    assert within_plan(["vegan", None, ["store-2", "in-stock"]], 3, names) == [[3], None, [1, 2]]
    with pytest.raises(ValueError, match="2 entries for 3"):
        within_plan(["vegan", None], 3, names)
    with pytest.raises(ValueError, match="one entry per query"):
        within_plan("vegan", 1, names)
    with pytest.raises(ValueError, match="product_sets"):
        within_plan([None, "vegan"], 2, None)


def test_load_product_sets(tmp_path):
    table = {"a": ["1", "2"], "b": [], "c": (3, 4)}
    assert load_product_sets(table) == {"a": ["1", "2"], "b": [], "c": ["3", "4"]}
    path = tmp_path / "sets.json"
    path.write_text(json.dumps({"a": ["1"], "b": ["2", "9"]}))
    assert load_product_sets(path) == load_product_sets(str(path)) == {"a": ["1"], "b": ["2", "9"]}
    for bad in ([["1"]], {}, {"a": "123"}, {"a": {"1": 1}}):
        with pytest.raises(ValueError):
            load_product_sets(bad)


class StubIndex:
    """What Recommender._set_product_sets and update_product_set call on a DeviceIndex."""

    def __init__(self):
        self.calls = []

    def set_rowsets(self, bits):
        self.calls.append(("set", np.array(bits)))

    def write_rowset(self, set_id, bits):
        self.calls.append(("write", set_id, np.array(bits)))


def stub_recommender(n=70):
    rec = Recommender.__new__(Recommender)
    rec.product_ids = [str(i + 1) for i in range(n)]
    rec._pid_to_row = {p: i for i, p in enumerate(rec.product_ids)}
    rec._index = StubIndex()
    return rec


def test_recommender_product_sets_on_a_stub_index():
    rec = stub_recommender()
    rec._set_product_sets(None)
    assert rec.product_sets is None and rec._index.calls == []
    rec._set_product_sets({"store": ["1", "32", "33", "70", "not in the catalog"], "stock": [str(i) for i in range(1, 71, 2)]})
    assert rec.product_sets == ["store", "stock"]
    (what, bits), = rec._index.calls
    assert what == "set" and bits.dtype == np.uint32 and bits.shape == (2, 3)
    assert bits[0].tolist() == [(1 << 31) | 1, 1, 1 << 5]                  # rows 0, 31, 32, 69; the unknown id is skipped
    assert rec._set_member.shape == (2, 70) and np.flatnonzero(rec._set_member[0]).tolist() == [0, 31, 32, 69]
    # the host-side boost filtering reads the host's copy
    lists, only = boost_plan([{"1": 1.0, "2": 2.0, "33": 0.5}, ["70", "3"], None], 0.25, False, 3, rec._pid_to_row)
    sets = within_plan(["store", ["store", "stock"], "stock"], 3, rec.product_sets)
    assert boosts_within(lists, sets, rec._set_member) == [{0: 1.0, 32: 0.5}, {}, None]
    assert boosts_within(lists, [None, [], [0]], rec._set_member) == lists    # no constraint: nothing dropped
    # update_product_set: one write_rowset, the host's copy follows
    rec.update_product_set("stock", ["2", "33", "nope"])
    what, set_id, one = rec._index.calls[-1]
    assert (what, set_id) == ("write", 1) and one.shape == (3,) and one.tolist() == [2, 1, 0]
    assert np.flatnonzero(rec._set_member[1]).tolist() == [1, 32]
    assert boosts_within(lists, sets, rec._set_member) == [{0: 1.0, 32: 0.5}, {}, None]
    assert boosts_within([{1: 1.0, 2: 1.0, 32: 1.0}], [[1]], rec._set_member) == [{1: 1.0, 32: 1.0}]
    with pytest.raises(ValueError, match="unknown product set"):
        rec.update_product_set("nope", ["1"])
    with pytest.raises(ValueError):
        rec.update_product_set("stock", "123")
    assert len(rec._index.calls) == 2


def test_cli_arguments():
    from instacart_next_order_recommendation_amd import cli

    args = cli.build_parser().parse_args(["--product-sets", "sets.json", "--within", "store-1", "--within", "in-stock"])
    assert args.product_sets == Path("sets.json") and args.within == ["store-1", "in-stock"]
    assert cli.build_parser().parse_args([]).within is None
    with pytest.raises(SystemExit, match="--product-sets"):
        cli.main(["--within", "store-1"])
