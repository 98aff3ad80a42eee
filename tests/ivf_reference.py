"""The IVF index's definition (include/icrec.h, icrec_ivf) in numpy over the oracle, and the crafted catalog of the IVF
tests.  Importing this needs no GPU.

  stored rows   P_stored = oracle.normalize_rows(P), put through oracle.round_bf16 for bf16 storage
  assignment    list(r) = the row oracle.search(P_stored[r], C, 1) returns: the library's own search of the centroids,
                with its query normalisation and its tie rule (the lower list wins)
  layout        perm = the rows in a stable sort by list, list_off = the list boundaries
  probes        probes(q) = the rows of oracle.search(q, C, nprobe)
  search        the library's selection (search_harness.select_from_scores) on the complete score matrix
                oracle.scores(q_hat, P_stored), with only the rows admitted whose list is among the query's probes
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle
from tests import search_harness


def stored_rows(P, storage="f32"):
    """What icrec_index_export returns for an index of P: the normalised rows, rounded to bfloat16 for bf16 storage."""
    rows = oracle.normalize_rows(np.ascontiguousarray(P, np.float32))
    return oracle.round_bf16(rows) if storage.startswith("bf16") else rows


def assign(P_stored, C):
    """list(r) for every stored row: int64 [n]."""
    return oracle.search(P_stored, C, 1)[0][:, 0]


def layout(assignment, n_lists):
    """(perm int32 [n], list_off int64 [n_lists + 1]): the rows sorted by (list, row), and the list boundaries."""
    perm = np.argsort(assignment, kind="stable").astype(np.int32)
    off = np.zeros(n_lists + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(assignment, minlength=n_lists))
    return perm, off


def probes(q, C, nprobe):
    """The nprobe lists each query scans, best first: int64 [Q, nprobe]."""
    return oracle.search(q, C, nprobe)[0]


def search(q, P, C, k, nprobe, excl=None, row_offset=0, storage="f32", assignment=None, scores=None):
    """The IVF search's result (idx int64 [Q, k], score float32 [Q, k]).  assignment: assign(stored_rows(P, storage), C),
    scores: oracle.scores(oracle.normalize_rows(q), stored_rows(P, storage)), where the caller has them already."""
    q = np.ascontiguousarray(q, np.float32)
    if assignment is None or scores is None:
        P_stored = stored_rows(P, storage)
    if assignment is None:
        assignment = assign(P_stored, C)
    if scores is None:
        scores = oracle.scores(oracle.normalize_rows(q), P_stored)
    pr = probes(q, C, nprobe)
    admit = np.zeros(scores.shape, bool)
    for j in range(pr.shape[1]):
        admit |= assignment[None, :] == pr[:, j, None]
    return search_harness.select_from_scores(scores, k, excl, row_offset, admit)


MERGE_MAX_LISTS = search_harness.MERGE_MAX_LISTS


def plan_slices(n_cu, Q, nprobe):
    """csrc/ivf.hip's plan_slices restated: the slices S every probed list of a call is cut into; slice s of a list of
    `tiles` 256-row tiles walks tiles [s * tps, (s + 1) * tps), tps = ceil(tiles / S)."""
    target, items = 2 * n_cu, Q * nprobe
    if items >= target:
        return 1
    return min((target + items - 1) // items, MERGE_MAX_LISTS // nprobe)


# ---------------------------------------------------------------- the crafted catalog
CRAFTED_COUNTS = (1, 255, 256, 257, 0, 1300, 513, 40)   # rows per list; list 4's centroid is a copy of list 2's
CRAFTED_DIM = 64


@functools.lru_cache(maxsize=None)
def crafted_catalog(seed=6):
    """Eight random centroids at dim 64, centroid 4 a copy of centroid 2; rows centroid + 0.05 noise with the per-list
    counts CRAFTED_COUNTS, shuffled: 2,622 rows -> (P [2622, 64], C [8, 64], home int64 [2622]: the centroid each row
    was drawn around), read-only.  Lists of exactly 1, 255, 256 and 257 rows, one of 1,300 (six tiles of 256), an empty
    one: list 4, whose centroid ties with list 2's and loses on the list number."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((len(CRAFTED_COUNTS), CRAFTED_DIM)).astype(np.float32)
    C[4] = C[2]
    home = np.repeat(np.arange(len(CRAFTED_COUNTS)), CRAFTED_COUNTS)
    P = C[home] + np.float32(0.05) * rng.standard_normal((home.size, CRAFTED_DIM)).astype(np.float32)
    order = rng.permutation(home.size)
    P, home = np.ascontiguousarray(P[order]), home[order]
    for a in (P, C, home):
        a.flags.writeable = False
    return P, C, home


def crafted_preconditions(storage="f32"):
    """What the tests rely on, from the reference alone: every row lands in the list it was drawn around (so the lists
    have CRAFTED_COUNTS rows and list 4 is empty), with a best-to-second-best centroid score gap of at least 0.70
    (centroid 4, the copy, left out of the second best of list 2's rows); and a query near centroid 2 probes list 2
    first and the empty list 4 second.  -> the assignment."""
    P, C, home = crafted_catalog()
    P_stored = stored_rows(P, storage)
    a = assign(P_stored, C)
    np.testing.assert_array_equal(a, home)
    np.testing.assert_array_equal(np.bincount(a, minlength=len(CRAFTED_COUNTS)), CRAFTED_COUNTS)
    s = oracle.scores(oracle.normalize_rows(P_stored), oracle.normalize_rows(C))
    best = s[np.arange(a.size), a]
    s[np.arange(a.size), a] = -np.inf
    s[a == 2, 4] = -np.inf
    assert (best - s.max(axis=1)).min() >= 0.70
    np.testing.assert_array_equal(probes(C[2:3] + np.float32(0.01), C, 2), [[2, 4]])
    return a
