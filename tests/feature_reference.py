"""The expected result of a feature sweep case (tests/feature_cases.py), composed from the references each feature
already has - no feature is stated a second time here:

  scores      boost_reference.catalog_scores (the oracle's arithmetic per storage) over the model after the edit script
  admission   rowset_cases.admitted / search_harness.admitted_matrix
  selection   search_harness.select_from_scores, boost_reference.full_catalog, cap_reference.greedy_walk (over
              boost_reference.adjusted_catalog for a capped walk of a boosted ranking), mmr_reference.mmr_select,
              ivf_reference.search

`off` names one request feature to switch off (the binding check of tests/test_feature_cases.py).  Importing this needs
no GPU."""
from __future__ import annotations

import numpy as np

from instacart_next_order_recommendation_amd.search import facet_masks
from tests import boost_reference, cap_reference, ivf_reference, mmr_reference
from tests.rowset_cases import admitted
from tests.search_harness import admitted_matrix, select_from_scores

FEATURES = ("exclusions", "masks", "sets", "boosts", "caps", "lambda", "nprobe")


def base_storage(storage):
    return "bf16" if storage.startswith("bf16") else "f32"


def catalog_scores(q, E, storage):
    return boost_reference.catalog_scores(q, E, base_storage(storage))


def admission(F, M, nq, allow=None, set_ids=None):
    """bool [Q, n]: the rows a query's facet masks and set slots admit; None where the request has neither."""
    if set_ids is not None:
        return admitted(M, set_ids, F, allow)
    if allow is not None:
        return admitted_matrix(F, facet_masks(allow, nq, F.shape[1]))
    return None


def active_features(c):
    """The request features case c carries, by FEATURES' names."""
    on = []
    if c.excl is not None and any(len(e) for e in c.excl):
        on.append("exclusions")
    if c.allow is not None:
        on.append("masks")
    if c.set_ids is not None:
        on.append("sets")
    if c.boosts is not None and any(len(r) for r, _ in c.boosts):
        on.append("boosts")
    if c.caps is not None and (np.asarray(c.caps) > 0).any():
        on.append("caps")
    if c.kind == "diverse" and c.lam != 1.0:
        on.append("lambda")
    if c.kind == "ivf" and c.nprobe < c.C.shape[0]:
        on.append("nprobe")
    return on


def expected(c, off=None):
    """(idx int64 [Q, k'], score float32 [Q, k']) of case c on its model after the script, exactly as for a fresh index.
    For the diverse kind: in selection order, with the relevances."""
    assert off is None or off in FEATURES
    m = c.model
    nq, off_rows = c.q.shape[0], c.row_offset
    excl = None if off == "exclusions" else c.excl
    allow = None if off == "masks" else c.allow
    set_ids = None if off == "sets" else c.set_ids
    empty = (np.zeros(0, np.int64), np.zeros(0, np.float32))
    lists = c.boosts if c.boosts is not None and off != "boosts" else [empty] * nq
    caps = np.zeros((nq, 2), np.int64) if c.caps is None or off == "caps" else c.caps
    admit = admission(m.F, m.M, nq, allow, set_ids)
    s = c.scores
    if c.kind in ("plain", "faceted", "in-sets", "in-sets+faceted"):
        return select_from_scores(s, c.k, excl, off_rows, admit)
    if c.kind in ("boosted", "boosted-only"):
        return boost_reference.full_catalog(s, lists, c.k, excl, admit, c.kind == "boosted-only", off_rows)
    if c.kind == "capped":
        return cap_reference.greedy_walk(s, m.F, caps, c.k, excl, admit, off_rows)
    if c.kind == "capped+boosted":
        adjusted, adm = boost_reference.adjusted_catalog(s, lists, excl, admit)
        return cap_reference.greedy_walk(adjusted, m.F, caps, c.k, excl, adm, off_rows)
    if c.kind == "diverse":
        cand, rel = select_from_scores(s, c.k, excl, off_rows, admit)
        return mmr_reference.mmr_select(mmr_reference.stored_rows(m.E, c.storage), cand, rel, c.top_k,
                                        1.0 if off == "lambda" else c.lam, off_rows)
    assert c.kind == "ivf", c.kind
    return ivf_reference.search(c.q, m.E, c.C, c.k, c.C.shape[0] if off == "nprobe" else c.nprobe, excl, off_rows,
                                base_storage(c.storage), c.assignment, s)
