"""icrec_boost_select's definition (include/icrec.h) in numpy float32, over the oracle's arithmetic, stated both ways:

  full_catalog   the scores of the whole catalog, oracle.scores(oracle.normalize_rows(q), stored rows), with the valid
                 listed rows' entries replaced by their adjusted scores, selected by search_harness.select_from_scores
                 under the query's exclusions and facet admission - what the feature MEANS;
  post_merge     the valid listed entries merged with a given candidate list - what the library DOES.

With non-negative weights a(r) >= cos(r) for every row, so an unlisted row in the adjusted top-k has fewer than k rows
before it under plain cosine too: post_merge over a search's top-k equals full_catalog (tests/test_boost.py checks it).
A query's list is a pair (rows int array, weights float32 array or None), ascending by row.  Importing this needs no GPU."""
from __future__ import annotations

import numpy as np

from oracle import oracle
from tests import mmr_reference
from tests.search_harness import select_from_scores


def catalog_scores(q, P, storage: str = "f32") -> np.ndarray:
    """icrec_scores' bits: [Q, n] float32, the j-ascending fmaf chain of the normalised queries over the stored rows."""
    return oracle.scores(oracle.normalize_rows(np.ascontiguousarray(q, np.float32)), mmr_reference.stored_rows(P, storage))


def lists_of(boosts, n_queries: int):
    """Per-query None / mapping row -> weight / iterable of rows (what search.boost_csr takes) -> per-query
    (rows int64 ascending, weights float32)."""
    assert len(boosts) == n_queries
    out = []
    for b in boosts:
        pairs = {} if b is None else {int(r): np.float32(v) for r, v in b.items()} if hasattr(b, "items") \
            else {int(r): np.float32(0) for r in b}
        rows = np.asarray(sorted(pairs), np.int64)
        out.append((rows, np.asarray([pairs[int(r)] for r in rows], np.float32)))
    return out


def read_entries(lst, max_boosts):
    """The entries of one list that are read: the first max_boosts (all of them for None); weights None = all 0."""
    rows = np.asarray(lst[0], np.int64)
    w = np.zeros(rows.size, np.float32) if lst[1] is None else np.asarray(lst[1], np.float32)
    m = rows.size if max_boosts is None else min(rows.size, max_boosts)
    return rows[:m], w[:m]


def adjusted_scores(cos: np.ndarray, w: np.ndarray) -> np.ndarray:
    """a = cos, bits unchanged, where the effective weight is 0 (w NaN, negative or zero); else cos + w, one fp32 add."""
    cos, w = np.asarray(cos, np.float32), np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        w_eff = np.where(w >= 0, w, np.float32(0)).astype(np.float32)
        return np.where(w_eff == 0, cos, (cos + w_eff).astype(np.float32)).astype(np.float32)


def _valid_listed(rows, n, excl_i, admit_i):
    ok = (rows >= 0) & (rows < n)
    if excl_i is not None:
        ok &= ~np.isin(rows, np.asarray(sorted(set(int(v) for v in excl_i)), np.int64))
    if admit_i is not None:
        ok[ok] &= admit_i[rows[ok]]
    return ok


def adjusted_catalog(scores, lists, excl=None, admit=None, only=False, max_boosts=None):
    """The ranking a boosted request selects from: scores with the valid listed rows' entries replaced by their adjusted
    scores, and the admission that goes with it (only=True: the listed rows alone) -> (adjusted float32 [Q, n], admit
    bool [Q, n] or None).  full_catalog takes its top_k; a capped walk (cap_reference.greedy_walk) walks all of it."""
    Q, n = scores.shape
    adjusted = np.array(scores, np.float32)
    listed = np.zeros((Q, n), bool)
    for i, lst in enumerate(lists):
        rows, w = read_entries(lst, max_boosts)
        ok = _valid_listed(rows, n, None if excl is None else excl[i], None if admit is None else admit[i])
        adjusted[i, rows[ok]] = adjusted_scores(scores[i, rows[ok]], w[ok])
        listed[i, rows[ok]] = True
    if only:
        admit = listed if admit is None else admit & listed
    return adjusted, admit


def full_catalog(scores, lists, top_k, excl=None, admit=None, only=False, row_offset=0, max_boosts=None):
    """scores: catalog_scores' [Q, n]; lists: per-query (rows, weights); excl: per-query local rows or None; admit: bool
    [Q, n] or None -> (idx int64 [Q, top_k], score float32 [Q, top_k]) with -1 / 0 pads: the top_k of the whole catalog
    under the adjusted scores.  only=True: of the listed rows alone."""
    adjusted, admit = adjusted_catalog(scores, lists, excl, admit, only, max_boosts)
    return select_from_scores(adjusted, top_k, excl, row_offset, admit)


def post_merge(scores, cand_idx, cand_score, lists, top_k, excl=None, admit=None, row_offset=0, max_boosts=None):
    """The definition as the library computes it: cand_idx int64 [Q, k] / cand_score float32 [Q, k] (both None: no
    candidates) merged with the valid listed entries; a candidate whose row is among the entries READ from the list
    is dropped; order: score descending compared as floats (-0 == +0), lower row first."""
    Q, n = scores.shape
    out_idx = np.full((Q, top_k), -1, np.int64)
    out_sc = np.zeros((Q, top_k), np.float32)
    for i, lst in enumerate(lists):
        rows, w = read_entries(lst, max_boosts)
        ok = _valid_listed(rows, n, None if excl is None else excl[i], None if admit is None else admit[i])
        item_rows = [rows[ok]]
        item_sc = [adjusted_scores(scores[i, rows[ok]], w[ok])]
        if cand_idx is not None:
            c = np.asarray(cand_idx[i], np.int64)
            local = c - row_offset
            keep = (c >= 0) & (local >= 0) & (local < n) & ~np.isin(local, rows)
            item_rows.append(local[keep])
            item_sc.append(np.asarray(cand_score[i], np.float32)[keep])
        r, s = np.concatenate(item_rows), np.concatenate(item_sc).astype(np.float32)
        order = np.lexsort((r, -s.astype(np.float64)))[:top_k]
        out_idx[i, :order.size] = row_offset + r[order]
        out_sc[i, :order.size] = s[order]
    return out_idx, out_sc
