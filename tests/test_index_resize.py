"""Adding and removing rows without a device: the move plan of icrec_index_remove_rows restated in numpy against a
brute-force statement of it, the argument checks of Recommender.add_products / remove_products, and the new entry points
on a NULL handle."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.recommender import product_add_plan, product_remove_plan
from instacart_next_order_recommendation_amd.search import apply_moves, removal_moves


def brute_force(n, ids):
    """Delete the rows `ids` of 0 .. n-1, then fill the holes below new_n from the survivors at or past it, in order ->
    (new_n, the moves as (dst, src) pairs, the old row that ends up in each new row)."""
    removed = set(int(i) for i in ids)
    new_n = n - len(removed)
    content = [None if r in removed else r for r in range(n)]
    moves = []
    for hole in range(new_n):
        if content[hole] is not None:
            continue
        filler = next(r for r in range(new_n, n) if content[r] is not None)
        content[hole], content[filler] = content[filler], None
        moves.append((hole, filler))
    assert all(c is None for c in content[new_n:]) and all(c is not None for c in content[:new_n])
    return new_n, moves, content[:new_n]


def assert_plan(n, ids):
    new_n, dst, src = removal_moves(n, ids)
    want_n, moves, content = brute_force(n, ids)
    assert new_n == want_n
    assert dst.dtype == src.dtype == np.int32
    assert list(zip(dst.tolist(), src.tolist())) == moves
    assert (dst < new_n).all() and (src >= new_n).all() and (src < n).all()
    assert apply_moves(np.arange(n), new_n, dst, src).tolist() == content
    two_d = np.stack([np.arange(n), 10 * np.arange(n)])                       # (a membership matrix: rows along axis 1)
    np.testing.assert_array_equal(apply_moves(two_d, new_n, dst, src, axis=1), np.stack([content, 10 * np.asarray(content)]))


def test_removal_moves_against_brute_force():
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(2, 200))
        m = int(rng.integers(0, n))
        assert_plan(n, rng.permutation(n)[:m])                                # (any order)
    assert_plan(1061, [])                                                     # m = 0
    new_n, dst, src = removal_moves(1061, [])
    assert new_n == 1061 and dst.size == 0 and src.size == 0
    assert_plan(1061, np.arange(1040, 1061))                                  # every id >= new_n: no holes, no moves
    assert removal_moves(1061, np.arange(1040, 1061))[1].size == 0
    assert_plan(1061, np.arange(0, 21))                                       # no tail ids: the last 21 rows all move
    assert removal_moves(1061, np.arange(0, 21))[2].tolist() == list(range(1040, 1061))
    assert_plan(50, np.arange(1, 50))                                         # m = n - 1, row 0 survives
    assert_plan(50, np.arange(0, 49))                                         # m = n - 1, the last row survives
    assert [a.tolist() for a in removal_moves(50, np.arange(0, 49))[1:]] == [[0], [49]]
    assert_plan(1061, [1057, 1058])
    assert_plan(1061, [0, 31, 32, 255, 256, 1023] + list(range(1030, 1061)))


@pytest.mark.parametrize("n,ids,match", [(10, [10], "outside"), (10, [-1], "outside"), (10, [3, 3], "twice"),
                                         (4, [0, 1, 2, 3], "empty"), (10, [1.5], "integers")])
def test_removal_moves_refuses(n, ids, match):
    with pytest.raises(ValueError, match=match):
        removal_moves(n, ids)


TEXT = "Product: {}. Aisle: {}. Department: {}."


def catalog():
    pid_to_row = {"a": 0, "b": 1, "c": 2}
    return pid_to_row, ["tea", "milk"], ["drinks", "dairy"]


def test_product_add_plan():
    pid_to_row, aisles, departments = catalog()
    ids, texts, codes, new_aisles, new_departments = product_add_plan(
        {"x": TEXT.format("Oat milk", "milk", "dairy"), "y": TEXT.format("Kombucha", "fermented", "drinks")},
        pid_to_row, aisles, departments)
    assert ids == ["x", "y"] and texts[1].startswith("Product: Kombucha")
    assert codes.dtype == np.uint8 and codes.tolist() == [[1, 1], [2, 0]]
    assert new_aisles == ["tea", "milk", "fermented"] and new_departments == ["drinks", "dairy"]   # appended behind
    assert aisles == ["tea", "milk"]                                                               # (a copy)
    assert product_add_plan({}, pid_to_row, aisles, departments)[0] == []
    assert product_add_plan({"x": "any text"}, pid_to_row, None, None) == (["x"], ["any text"], None, None, None)


def test_product_add_plan_refuses_with_nothing_changed():
    pid_to_row, aisles, departments = catalog()
    full = [f"aisle {i}" for i in range(256)]
    for additions, names, match in [
            ({"b": TEXT.format("Milk", "milk", "dairy")}, aisles, "already"),
            ({"x": "no markers here"}, aisles, "format"),
            ({"x": 5}, aisles, "string"),
            ([("x", "text")], aisles, "mapping"),
            ({"x": TEXT.format("Thing", "the 257th", "dairy")}, full, "257th aisle")]:
        before = (dict(pid_to_row), list(names), list(departments))
        with pytest.raises(ValueError, match=match):
            product_add_plan(additions, pid_to_row, names, departments)
        assert (pid_to_row, names, departments) == before
    with pytest.raises(ValueError, match="257th department"):
        product_add_plan({"x": TEXT.format("Thing", "milk", "new")}, pid_to_row, aisles, [f"d{i}" for i in range(256)])


def test_product_remove_plan():
    pid_to_row, _, _ = catalog()
    assert product_remove_plan(["c", "a"], pid_to_row) == [2, 0]
    assert product_remove_plan([], pid_to_row) == []
    for ids, match in [(["zzz"], "unknown"), (["a", "a"], "twice"), (["a", "b", "c"], "every product"), ("a", "list")]:
        before = dict(pid_to_row)
        with pytest.raises(ValueError, match=match):
            product_remove_plan(ids, pid_to_row)
        assert pid_to_row == before


def test_null_handle_touches_no_gpu():
    lib = _native.lib()
    assert lib.icrec_index_capacity(None) == 0
    n_moves = C.c_int32(7)
    ids = np.asarray([1, 2], np.int32)
    out = np.zeros((2, 2), np.int32)
    for rc in (lib.icrec_index_reserve(None, 100),
               lib.icrec_index_append_rows(None, None, 1, None, None),
               lib.icrec_index_remove_rows(None, ids.ctypes.data_as(C.c_void_p), 2, out[0].ctypes.data_as(C.c_void_p),
                                           out[1].ctypes.data_as(C.c_void_p), C.byref(n_moves), None)):
        assert rc == -1
        assert b"NULL index" in lib.icrec_last_error()
    assert n_moves.value == 7 and not out.any()
