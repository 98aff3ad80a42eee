"""icrec_cap_select's definition (include/icrec.h) in plain numpy - one sequential loop per query and the state - the
one-pass greedy capped walk of a complete ranking, and the round scheme that include/icrec.h proves equal to it
(capped_rounds, over tests/search_harness.select_from_scores).  Importing this needs no GPU."""
from __future__ import annotations

import numpy as np

from tests.search_harness import admitted_matrix, full_ranking, select_from_scores

MAX_FACETS, MASK_WORDS = 2, 8  # ICREC_MAX_FACETS, ICREC_FACET_MASK_WORDS


def cap_table(caps, n_queries: int) -> np.ndarray:
    """One pair for all queries, or [n_queries, 2] -> int64 [n_queries, 2]."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(caps, np.int64), (n_queries, MAX_FACETS)))


def cap_select(F, cand, score, caps, top_k, n_prior=None, out_idx=None, out_score=None, allow=None, row_offset=0):
    """The definition.  F: uint8 [n_rows, n_facets], the index's facet values; cand int64 [Q, k], score float32 [Q, k];
    caps int [Q, 2] (or one pair); n_prior int [Q] or None, with out_idx int64 [Q, top_k] / out_score float32
    [Q, top_k] holding the prior picks (they are copied, not written); allow uint32 [Q, n_facets, 8] or None
    -> (idx int64 [Q, top_k], score float32 [Q, top_k], state int32 [Q, 2], allow_next uint32 [Q, n_facets, 8])."""
    F = np.asarray(F)
    cand, score = np.asarray(cand, np.int64), np.asarray(score, np.float32)
    assert F.dtype == np.uint8 and F.ndim == 2 and 1 <= F.shape[1] <= MAX_FACETS and cand.shape == score.shape
    n_rows, n_facets = F.shape
    Q, k = cand.shape
    caps = cap_table(caps, Q)
    idx = np.full((Q, top_k), -1, np.int64)
    sc = np.zeros((Q, top_k), np.float32)
    state = np.zeros((Q, 2), np.int32)
    nxt = np.full((Q, n_facets, MASK_WORDS), 0xFFFFFFFF, np.uint32) if allow is None else np.array(allow, np.uint32)
    assert nxt.shape == (Q, n_facets, MASK_WORDS)
    for q in range(Q):
        count = np.zeros((n_facets, 256), np.int64)
        capped = [f for f in range(n_facets) if caps[q, f] > 0]
        p0 = 0 if n_prior is None else min(max(int(n_prior[q]), 0), top_k)
        picked = []
        for i in range(p0):
            c = int(out_idx[q, i])
            idx[q, i], sc[q, i] = c, out_score[q, i]
            picked.append(c)
            if c >= 0 and 0 <= c - row_offset < n_rows:
                for f in range(n_facets):
                    count[f, F[c - row_offset, f]] += 1
        for j in range(k):
            if len(picked) == top_k:
                break
            c = int(cand[q, j])
            if not (c >= 0 and 0 <= c - row_offset < n_rows) or c in picked:
                continue
            v = F[c - row_offset]
            if all(count[f, v[f]] < caps[q, f] for f in capped):
                idx[q, len(picked)], sc[q, len(picked)] = c, score[q, j]
                picked.append(c)
                for f in range(n_facets):
                    count[f, v[f]] += 1
        state[q] = len(picked), int(len(picked) == top_k or bool((cand[q] < 0).any()))
        for f in capped:
            for v in np.flatnonzero(count[f] >= caps[q, f]):
                nxt[q, f, v >> 5] &= np.uint32(~(1 << (v & 31)) & 0xFFFFFFFF)
    return idx, sc, state, nxt


def _ranked(scores_row, rows, head=4096):
    """`rows` in full_ranking's order, lazily: of a long list first the rows that score above its head-th best, ranked
    among themselves, and the others only if the walk gets that far."""
    if rows.size <= 4 * head:
        yield from rows[full_ranking(scores_row[rows])]
        return
    s = scores_row[rows]
    bar = np.partition(s, rows.size - head)[rows.size - head]
    for part in (rows[s > bar], rows[~(s > bar)]):
        yield from part[full_ranking(scores_row[part])]


def greedy_walk(scores, F, caps, top_k, excl=None, admit=None, row_offset=0):
    """The one-pass statement: per query the complete ranking of its admissible rows (score descending, row ascending,
    -0 as +0; excl[i] and admit [Q, n] as select_from_scores takes them), walked once from the best row down, keeping a
    row iff every capped facet has fewer than cap kept rows of its value -> (idx int64 [Q, top_k], score float32)."""
    scores = np.ascontiguousarray(scores, np.float32)
    F = np.asarray(F)
    Q, n = scores.shape
    caps = cap_table(caps, Q)
    idx = np.full((Q, top_k), -1, np.int64)
    sc = np.zeros((Q, top_k), np.float32)
    for q in range(Q):
        ok = np.ones(n, bool) if admit is None else admit[q].copy()
        if excl is not None:
            e = np.asarray(sorted(set(int(v) for v in excl[q])), np.int64)
            ok[e[(e >= 0) & (e < n)]] = False
        count = np.zeros((F.shape[1], 256), np.int64)
        capped = [f for f in range(F.shape[1]) if caps[q, f] > 0]
        m = 0
        for r in _ranked(scores[q], np.flatnonzero(ok)):
            if m == top_k:
                break
            if all(count[f, F[r, f]] < caps[q, f] for f in capped):
                idx[q, m], sc[q, m] = row_offset + r, scores[q, r] + np.float32(0.0)
                m += 1
                count[np.arange(F.shape[1]), F[r]] += 1
    return idx, sc


def capped_rounds(scores, F, caps, top_k, width, excl=None, admit=None, masks=None, row_offset=0):
    """The round scheme: search `width` wide (select_from_scores under the exclusions, `admit` and the facet masks),
    cap_select with the picks so far as priors, and while a query is not done search it again under the next masks and
    the exclusions united with its picks -> (idx, score, rounds).  masks: uint32 [Q, n_facets, 8] or None."""
    scores = np.ascontiguousarray(scores, np.float32)
    F = np.asarray(F)
    Q, n = scores.shape
    caps = cap_table(caps, Q)
    k = max(min(width, n), min(top_k, n))
    masks = np.full((Q, F.shape[1], MASK_WORDS), 0xFFFFFFFF, np.uint32) if masks is None else np.array(masks, np.uint32)
    excl = [set() for _ in range(Q)] if excl is None else [set(int(v) for v in e) for e in excl]
    idx = np.full((Q, top_k), -1, np.int64)
    sc = np.zeros((Q, top_k), np.float32)
    n_prior = np.zeros(Q, np.int64)
    left = np.arange(Q)
    rounds = 0
    while left.size:
        rounds += 1
        assert rounds <= MAX_FACETS * 256 + 1
        ok = admitted_matrix(F, masks[left])
        if admit is not None:
            ok &= admit[left]
        ex = [sorted(excl[i] | set((idx[i, :n_prior[i]] - row_offset).tolist())) for i in left]
        c_idx, c_sc = select_from_scores(scores[left], k, ex, row_offset, ok)
        idx[left], sc[left], state, masks[left] = cap_select(F, c_idx, c_sc, caps[left], top_k, n_prior[left], idx[left],
                                                             sc[left], masks[left], row_offset)
        n_prior[left] = state[:, 0]
        left = left[state[:, 1] == 0]
    return idx, sc, rounds
