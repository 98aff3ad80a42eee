"""Plain-Python statement of what the CF ranking and the IR metrics compute: the in-repo truth of the GPU tests.

Ranking: score(q, p) = sum over h in history(q) of cooc(p, h), cooc = the number of baskets (de-duplicated) holding
both; candidates of the history are left out; order = score descending, then candidate row ascending.
Metrics: per query, eight values accumulated in rank order in double (Python floats), so that a kernel adding in the
same order has the same bits; means over the queries whose relevant set is not empty.
"""
from __future__ import annotations

import math

METRIC_KEYS = ("accuracy_at_1", "accuracy_at_3", "accuracy_at_5", "accuracy_at_10", "recall_at_10", "mrr_at_10",
               "ndcg_at_10", "map_at_100")
DISCOUNTS = [1.0 / math.log2(i + 2) for i in range(10)]


def cf_scores(baskets, history, n_candidates: int) -> list[int]:
    """Integer scores of candidates 0..n_candidates-1 for one history (any iterable of item numbers)."""
    hist = set(history)
    scores = [0] * n_candidates
    for basket in baskets:
        items = set(basket)
        w = len(items & hist)
        if w:
            for p in items:
                if p < n_candidates:
                    scores[p] += w
    return scores


def cf_rank(baskets, histories, n_candidates: int, k: int | None = None):
    """Per history: (rows, scores) best first.  k=None: every candidate outside the history (the complete order);
    otherwise the best k, padded with row -1 / score 0."""
    out = []
    for history in histories:
        hist = set(history)
        scores = cf_scores(baskets, hist, n_candidates)
        rows = sorted((p for p in range(n_candidates) if p not in hist), key=lambda p: (-scores[p], p))
        sc = [scores[p] for p in rows]
        if k is not None:
            rows, sc = rows[:k], sc[:k]
            rows, sc = rows + [-1] * (k - len(rows)), sc + [0] * (k - len(sc))
        out.append((rows, sc))
    return out


def query_metrics(ranked, relevant) -> list[float] | None:
    """The eight values of one query; None when `relevant` is empty (the query is not counted).  `ranked` ends at its
    first negative entry."""
    relevant = set(relevant)
    if not relevant:
        return None
    ranked = list(ranked)
    for i, r in enumerate(ranked):
        if isinstance(r, int) and r < 0:
            ranked = ranked[:i]
            break
    hits = [r in relevant for r in ranked]
    top10 = hits[:10]
    vals = [1.0 if any(hits[:c]) else 0.0 for c in (1, 3, 5, 10)]
    n10 = sum(top10)
    vals.append(n10 / len(relevant))
    vals.append(next((1.0 / (i + 1) for i, h in enumerate(top10) if h), 0.0))
    dcg = 0.0
    for i, h in enumerate(top10):
        if h:
            dcg += DISCOUNTS[i]
    idcg = 0.0
    for i in range(n10):  # the "ideal" of the definition: the top-10's own hits moved to the front
        idcg += DISCOUNTS[i]
    vals.append(dcg / idcg if idcg > 0 else 0.0)
    cut = ranked[:100]
    s, nh = 0.0, 0
    for j, r in enumerate(cut, start=1):
        if r in relevant:
            nh += 1
            s += nh / j
    vals.append(s / min(len(relevant), len(cut)) if cut else 0.0)
    return vals


def ir_metrics(query_rankings: dict, relevant_docs: dict) -> dict[str, float]:
    """The eight means over the queries of `query_rankings` that have a non-empty relevant set (0.0 when none has)."""
    per = [query_metrics(query_rankings[q], relevant_docs[q]) for q in query_rankings
           if q in relevant_docs and relevant_docs[q]]
    if not per:
        return {key: 0.0 for key in METRIC_KEYS}
    return {key: sum(v[i] for v in per) / len(per) for i, key in enumerate(METRIC_KEYS)}
