"""Facets without a device: the four C entry points are exported, bound and reject a NULL handle, facet_masks puts
every value's bit where icrec.h says, and catalog_facets parses the catalog format from the right."""
from __future__ import annotations

import numpy as np
import pytest

from instacart_next_order_recommendation_amd.recommender import catalog_facets
from instacart_next_order_recommendation_amd.search import facet_masks
from instacart_next_order_recommendation_amd.synthetic import synthetic_catalog

FACET_SYMBOLS = ("icrec_index_set_facets", "icrec_index_facets", "icrec_search_faceted_workspace_bytes",
                 "icrec_search_faceted")
ICREC_EINVAL = -1
ONES = 0xFFFFFFFF


@pytest.fixture(scope="module")
def native():
    from instacart_next_order_recommendation_amd import _native

    if not _native.LIB_PATH.exists():
        _native.build()
    return _native


def test_symbols_exported_and_bound(native):
    lib = native.lib()
    for name in FACET_SYMBOLS:
        assert name in native.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert native.ICREC_MAX_FACETS == 2 and native.ICREC_FACET_MASK_WORDS == 8


def test_null_handle(native):
    """Every entry point answers a NULL handle before it touches a GPU."""
    lib = native.lib()
    assert lib.icrec_index_facets(None) == -1
    assert lib.icrec_search_faceted_workspace_bytes(None, 4, 20) == 0
    facets = np.zeros((4, 2), np.uint8)
    assert lib.icrec_index_set_facets(None, facets.ctypes.data, 2) == ICREC_EINVAL
    assert lib.icrec_index_set_facets(None, None, 0) == ICREC_EINVAL
    # non-NULL (never dereferenced) pointers everywhere else: the handle is what is refused
    p = facets.ctypes.data
    assert lib.icrec_search_faceted(None, p, 1, 1, None, None, p, p, p, p, 1 << 20, None) == ICREC_EINVAL
    assert b"NULL" in lib.icrec_last_error()


def test_facet_masks_bit_positions():
    m = facet_masks([[[0], [31]], [[32], [255]], [[0, 31, 32, 255], None], None, [[], [7, 7]]], 5, 2)
    assert m.dtype == np.uint32 and m.shape == (5, 2, 8)
    word = lambda i, f: [int(w) for w in m[i, f]]  # noqa: E731
    assert word(0, 0) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert word(0, 1) == [1 << 31, 0, 0, 0, 0, 0, 0, 0]
    assert word(1, 0) == [0, 1, 0, 0, 0, 0, 0, 0]
    assert word(1, 1) == [0, 0, 0, 0, 0, 0, 0, 1 << 31]
    assert word(2, 0) == [(1 << 31) | 1, 1, 0, 0, 0, 0, 0, 1 << 31]
    assert word(2, 1) == [ONES] * 8                    # a facet left open
    assert word(3, 0) == word(3, 1) == [ONES] * 8      # a query left open
    assert word(4, 0) == [0] * 8                       # [] admits nothing
    assert word(4, 1) == [1 << 7, 0, 0, 0, 0, 0, 0, 0]
    # every value on its own: bit v & 31 of word v >> 5, and nothing else
    for v in range(256):
        one = facet_masks([[[v]]], 1, 1)[0, 0]
        assert int(one[v >> 5]) == 1 << (v & 31) and int(one.astype(np.uint64).sum()) == 1 << (v & 31)


def test_facet_masks_one_facet_and_torch():
    import torch

    t = facet_masks([[[3]], None], 2, 1, "cpu")
    assert t.dtype == torch.uint32 and tuple(t.shape) == (2, 1, 8)
    np.testing.assert_array_equal(t.view(torch.int32).numpy().view(np.uint32), facet_masks([[[3]], None], 2, 1))


@pytest.mark.parametrize("bad", [256, -1, 1000])
def test_facet_masks_rejects_values_outside_a_byte(bad):
    with pytest.raises(ValueError):
        facet_masks([[[1, bad], None]], 1, 2)


def test_facet_masks_rejects_wrong_counts():
    with pytest.raises(ValueError):
        facet_masks([None], 2, 2)
    with pytest.raises(ValueError):
        facet_masks([[[1]]], 1, 2)


def test_catalog_facets_synthetic_catalog():
    texts = list(synthetic_catalog(2000).values())
    aisles, departments, codes = catalog_facets(texts)
    assert len(aisles) == len(set(aisles)) == 134 and len(departments) == len(set(departments)) == 21
    assert codes.dtype == np.uint8 and codes.shape == (2000, 2)
    for text, (a, d) in zip(texts, codes):
        assert text.endswith(f". Aisle: {aisles[a]}. Department: {departments[d]}.")
    # first-appearance order
    assert aisles[0] == aisles[codes[0, 0]] and departments[0] == departments[codes[0, 1]]
    first_seen = [int(np.argmax(codes[:, 0] == a)) for a in range(len(aisles))]
    assert first_seen == sorted(first_seen)


def test_catalog_facets_parses_from_the_right():
    texts = ["Product: Trail Mix. Aisle: fake. Department: bogus. Aisle: nuts seeds. Department: snacks.",
             "Product: Plain. Aisle: nuts seeds. Department: snacks.",
             "Product: Dot. Com. Aisle: tea. Department: beverages."]
    aisles, departments, codes = catalog_facets(texts)
    assert aisles == ["nuts seeds", "tea"] and departments == ["snacks", "beverages"]
    assert codes.tolist() == [[0, 0], [0, 0], [1, 1]]


@pytest.mark.parametrize("bad", ["Product: X. Department: d.", "Product: X. Aisle: a.", "no markers at all",
                                 "Product: X. Department: d. Aisle: a.", "Product: X. Aisle: a. Department: d"])
def test_catalog_facets_malformed_text(bad):
    good = "Product: Y. Aisle: a. Department: d."
    assert catalog_facets([good, good]) is not None
    assert catalog_facets([good, bad, good]) is None


def test_catalog_facets_too_many_values():
    texts = [f"Product: P{i}. Aisle: aisle {i}. Department: d." for i in range(257)]
    assert catalog_facets(texts[:256]) is not None
    assert catalog_facets(texts) is None
    texts = [f"Product: P{i}. Aisle: a. Department: dept {i}." for i in range(257)]
    assert catalog_facets(texts) is None
