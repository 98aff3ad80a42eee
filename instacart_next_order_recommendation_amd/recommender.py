"""Drop-in serving objects: Recommender / MonitoredRecommender / EmbeddingIndex.

Same constructor arguments, attributes, return types and error behaviour as the
reference's src/inference/serve_recommendations.py (class Recommender :133-225,
MonitoredRecommender :228-293, EmbeddingIndex :66-130, RecommendationMetrics :52-63),
with the arithmetic moved onto the GPU behind libicrec's C ABI:

    model.encode([query])        -> DeviceEncoder   (icrec_encode)
    cos_sim + argsort + filter   -> DeviceIndex     (icrec_search)
    model.encode(product_texts)  -> DeviceEncoder over the whole catalog at start-up

`recommend_batch` is the one addition: many contexts in one GPU pass (what a
micro-batching server calls); `recommend` is its single-query form.
"""
from __future__ import annotations

import hashlib
import json
import logging
import math
import os
import time
from dataclasses import dataclass, replace
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native
from .adapter import DEFAULT_SCALE, QueryAdapter, fit_plan
from .encoder import DeviceEncoder
from .model_io import LoadedModel, load_model_dir
from .search import (DeviceIndex, IvfIndex, apply_moves, facet_masks, fuse_select, rowset_bits, rowset_ids, rrf_weights,
                     train_centroids)

logger = logging.getLogger(__name__)

# on-disk cache names (reference: src/constants.py:88-92)
INDEX_SUBDIR = ".embedding_index"
MANIFEST_FILENAME = "manifest.json"
EMBEDDINGS_FILENAME = "embeddings.npy"
PRODUCT_IDS_FILENAME = "product_ids.json"


@dataclass
class RecommendationMetrics:
    """Per-request metrics (same seven fields as the reference, :52-63)."""

    user_id: str
    query_embedding_time_ms: float
    similarity_compute_time_ms: float
    total_latency_ms: float
    num_recommendations: int
    top_score: float
    avg_score: float
    timestamp: float


class EmbeddingIndex:
    """On-disk cache of the [N, hidden] fp32 product matrix, byte-compatible with the reference's
    (:66-130): <corpus dir>/.embedding_index/<sha256("model_dir|corpus_path")[:16]>/
    {manifest.json, embeddings.npy, product_ids.json}; valid only for the same corpus path,
    model dir, corpus mtime and product-id list."""

    def __init__(self, corpus_path: Path, model_dir: Path | str):
        self.corpus_path = Path(corpus_path).resolve()
        self.model_dir = model_dir
        digest = hashlib.sha256(f"{self.model_dir!s}|{self.corpus_path!s}".encode()).hexdigest()
        self._dir = self.corpus_path.parent / INDEX_SUBDIR / digest[:16]

    @property
    def directory(self) -> Path:
        return self._dir

    def _manifest_ok(self) -> bool:
        try:
            meta = json.loads((self._dir / MANIFEST_FILENAME).read_text())
            return (meta.get("corpus_path") == str(self.corpus_path)
                    and meta.get("model_dir") == str(self.model_dir)
                    and meta.get("corpus_mtime") == self.corpus_path.stat().st_mtime)
        except (OSError, ValueError):
            return False

    def load(self, product_ids: list[str]) -> Optional[np.ndarray]:
        """Cached matrix, or None on any mismatch / missing file."""
        if not self._manifest_ok():
            return None
        try:
            emb = np.load(self._dir / EMBEDDINGS_FILENAME)  # allow_pickle stays False
            cached_ids = json.loads((self._dir / PRODUCT_IDS_FILENAME).read_text())
        except (OSError, ValueError):
            return None
        if cached_ids != product_ids or len(emb) != len(product_ids):
            return None
        return emb

    def save(self, product_ids: list[str], embeddings: np.ndarray) -> None:
        self._dir.mkdir(parents=True, exist_ok=True)
        try:
            mtime = self.corpus_path.stat().st_mtime
        except OSError:
            mtime = 0
        (self._dir / MANIFEST_FILENAME).write_text(json.dumps({
            "corpus_path": str(self.corpus_path), "model_dir": str(self.model_dir),
            "corpus_mtime": mtime, "n_products": len(product_ids)}, indent=2))
        np.save(self._dir / EMBEDDINGS_FILENAME, np.asarray(embeddings, dtype=np.float32))
        (self._dir / PRODUCT_IDS_FILENAME).write_text(json.dumps(product_ids))
        logger.info("Saved embedding index to %s (%d products)", self._dir, len(product_ids))


def catalog_facets(texts: Sequence[str]):
    """The aisle and the department of every catalog text "Product: {name}. Aisle: {aisle}. Department: {department}."
    (the reference's corpus format), parsed from the right so that a product name may hold the markers itself:
    the department is what follows the last ". Department: " without the final ".", the aisle what lies between the
    last ". Aisle: " before that point and it.  -> (aisle names, department names, codes uint8 [n, 2]), names in
    order of first appearance, codes[i] = (index of text i's aisle, index of its department); None when a text does
    not parse or a facet has more than 256 distinct values (a recommender then has no facets)."""
    names: tuple[dict[str, int], dict[str, int]] = ({}, {})
    codes = np.zeros((len(texts), 2), np.uint8)
    for i, text in enumerate(texts):
        parsed = text_facets(text)
        if parsed is None:
            return None
        for f, value in enumerate(parsed):
            code = names[f].setdefault(value, len(names[f]))
            if code > 255:
                return None
            codes[i, f] = code
    return list(names[0]), list(names[1]), codes


def text_facets(text: str) -> Optional[tuple[str, str]]:
    """(aisle, department) of one catalog text as catalog_facets parses it, or None when it does not parse."""
    d = text.rfind(". Department: ")
    a = text.rfind(". Aisle: ", 0, d) if d >= 0 else -1
    if a < 0 or not text.endswith("."):
        return None
    return text[a + len(". Aisle: "):d], text[d + len(". Department: "):-1]


def _facet_codes(texts, aisles, departments, whose):
    """The facet half of product_update_plan and product_add_plan: texts -> (codes uint8 [m, 2], aisle names, department
    names), (None, None, None) for a catalog without facets (aisles is None).  A name the catalog does not have yet is
    appended to (a copy of) its list, so every existing code stays.  ValueError: a text that does not parse - whose(i)
    names text i in it - and a 257th aisle or department name."""
    if aisles is None:
        return None, None, None
    names = (list(aisles), list(departments))
    code = tuple({name: i for i, name in enumerate(known)} for known in names)
    codes = np.zeros((len(texts), 2), np.uint8)
    for i, text in enumerate(texts):
        parsed = text_facets(text)
        if parsed is None:
            raise ValueError(f"{whose(i)} is not in the 'Product: .. Aisle: .. Department: ..' format of this catalog")
        for f, value in enumerate(parsed):
            if value not in code[f]:
                if len(names[f]) >= 256:
                    raise ValueError(f"{value!r} would be the 257th {'aisle' if f == 0 else 'department'} name; a facet "
                                     "has 256 values")
                code[f][value] = len(names[f])
                names[f].append(value)
            codes[i, f] = code[f][value]
    return codes, names[0], names[1]


def product_update_plan(updates, pid_to_row, product_texts, aisles, departments):
    """Recommender.update_products' argument, checked before any GPU work.  updates: a mapping product id -> new text;
    pid_to_row and product_texts: the catalog's rows and current texts; aisles / departments: its facet names, None for
    a catalog without facets
    -> (rows ascending, their new texts, facet codes uint8 [m, 2] or None without facets, aisle names, department names).
    A name the catalog does not have yet is appended to (a copy of) its list, so every existing code stays what it is
    (catalog_facets numbers by first appearance; a name no product carries any more keeps its code).  An empty
    mapping gives no rows.  ValueError: not a mapping, an id the catalog does not have (add_products adds one),
    a text that is not a string, on a catalog with facets a text that does not parse as
    'Product: .. Aisle: .. Department: ..', a 257th aisle or department name."""
    if not hasattr(updates, "items"):
        raise ValueError("updates must be a mapping product id -> new text")
    pairs = []
    for pid, text in updates.items():
        if pid not in pid_to_row or not 0 <= pid_to_row[pid] < len(product_texts):
            raise ValueError(f"unknown product id {pid!r}: update_products rewrites products the catalog has; "
                             "add_products adds one")
        if not isinstance(text, str):
            raise ValueError(f"the new text of product {pid!r} must be a string, got {type(text).__name__}")
        pairs.append((int(pid_to_row[pid]), text))
    pairs.sort(key=lambda p: p[0])
    rows, texts = [r for r, _ in pairs], [t for _, t in pairs]
    return (rows, texts, *_facet_codes(texts, aisles, departments, lambda i: f"the new text of row {rows[i]}"))


def product_add_plan(additions, pid_to_row, aisles, departments):
    """Recommender.add_products' argument, checked before any GPU work.  additions: a mapping product id -> text;
    pid_to_row: the catalog's rows; aisles / departments: its facet names, None for a catalog without facets
    -> (the new ids in the mapping's order, their texts, facet codes uint8 [m, 2] or None without facets, aisle names,
    department names).  A name the catalog does not have yet is appended behind (a copy of) its list, as
    product_update_plan does.  An empty mapping gives no ids.  ValueError: not a mapping, an id the catalog already has,
    a text that is not a string, on a catalog with facets a text that does not parse, a 257th aisle or department
    name.  (A mapping cannot name an id twice.)"""
    if not hasattr(additions, "items"):
        raise ValueError("additions must be a mapping product id -> text")
    ids, texts = [], []
    for pid, text in additions.items():
        if pid in pid_to_row:
            raise ValueError(f"product id {pid!r} is in the catalog already: update_products gives it a new text")
        if not isinstance(text, str):
            raise ValueError(f"the text of product {pid!r} must be a string, got {type(text).__name__}")
        ids.append(pid)
        texts.append(text)
    return (ids, texts, *_facet_codes(texts, aisles, departments, lambda i: f"the text of product {ids[i]!r}"))


def product_remove_plan(product_ids, pid_to_row) -> list[int]:
    """Recommender.remove_products' argument, checked before any GPU work: a list of product ids -> their rows, in the
    list's order.  ValueError: a string instead of a list, an id the catalog does not have, an id named twice, a list
    that names every product (a catalog is never empty)."""
    if isinstance(product_ids, (str, bytes)) or hasattr(product_ids, "items"):
        raise ValueError("remove_products takes a list of product ids")
    rows, seen = [], set()
    for pid in product_ids:
        if pid not in pid_to_row:
            raise ValueError(f"unknown product id {pid!r}: remove_products removes products the catalog has")
        if pid in seen:
            raise ValueError(f"product id {pid!r} is named twice")
        seen.add(pid)
        rows.append(int(pid_to_row[pid]))
    if rows and len(rows) >= len(pid_to_row):
        raise ValueError("remove_products: removing every product would leave the catalog empty")
    return rows


def diversity_plan(diversity, candidates, top_k: int, n_products: int):
    """A request's `diversity` / `candidates` arguments, checked before any GPU work
    -> None (the plain path: diversity is None or 0) or (lambda, candidate count) for the MMR re-selection.
    diversity must lie in [0, 1] (lambda = 1 - diversity), candidates in [top_k, ICREC_MAX_K]; ValueError otherwise.
    The candidate count defaults to min(ICREC_MAX_K, 4 * top_k) and is clipped to the catalog, never below top_k's own
    clipped width."""
    top_k = max(int(top_k), 1)
    if diversity is not None and not 0.0 <= float(diversity) <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError(f"diversity must be in [0, 1], got {diversity!r}")
    if candidates is not None and not top_k <= int(candidates) <= _native.ICREC_MAX_K:
        raise ValueError(f"candidates must be in [top_k = {top_k}, {_native.ICREC_MAX_K}], got {candidates!r}")
    if diversity is None or float(diversity) == 0.0:
        return None
    n = int(candidates) if candidates is not None else min(_native.ICREC_MAX_K, 4 * top_k)
    return 1.0 - float(diversity), max(min(n, n_products), min(top_k, n_products))


def boost_rows(boosts, boost_weight, only_boosted: bool, pid_to_row) -> Optional[dict[int, float]]:
    """One request's `boosts` / `boost_weight` / `only_boosted` arguments, checked before any GPU work
    -> None (the plain request: nothing to boost and only_boosted false) or {catalog row: weight}, the list
    DeviceIndex.search_boosted takes (empty with only_boosted and nothing known to boost: no result).
    boosts is a mapping product id -> weight, or an iterable of ids that all take boost_weight, which is then required.
    Ids the catalog does not have are skipped, as for exclusions.  ValueError: a string for boosts, a weight (or
    boost_weight) that is not a number >= 0, an iterable without boost_weight, more than ICREC_MAX_BOOSTS known ids."""
    def weight(v, what):
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float("nan")
        if not 0.0 <= f:  # (a NaN fails the comparison)
            raise ValueError(f"{what} must be a number >= 0, got {v!r}")
        return f

    if boost_weight is not None:
        boost_weight = weight(boost_weight, "boost_weight")
    if isinstance(boosts, (str, bytes)):
        raise ValueError("boosts must be a mapping product id -> weight or an iterable of product ids, not a string")
    if boosts is None:
        pairs = {}
    elif hasattr(boosts, "items"):
        pairs = {pid_to_row[p]: weight(v, f"the boost weight of {p!r}") for p, v in boosts.items() if p in pid_to_row}
    else:
        ids = list(boosts)
        if ids and boost_weight is None:
            raise ValueError("boosts given as ids needs boost_weight")
        pairs = {pid_to_row[p]: boost_weight for p in ids if p in pid_to_row}
    if len(pairs) > _native.ICREC_MAX_BOOSTS:
        raise ValueError(f"{len(pairs)} boosted products exceed the limit {_native.ICREC_MAX_BOOSTS}")
    if not pairs and not only_boosted:
        return None
    return pairs


def boost_plan(boosts, boost_weight, only_boosted: bool, n_queries: int, pid_to_row):
    """A batch's boost arguments (boosts: None or one entry per query, each as boost_rows takes it; boost_weight and
    only_boosted: one value for the batch) -> None (the plain path) or (per-query {row: weight} or None, only_boosted)."""
    if boosts is None and boost_weight is None and not only_boosted:
        return None
    if boosts is None:
        boosts = [None] * n_queries
    elif hasattr(boosts, "items") or isinstance(boosts, (str, bytes)):
        raise ValueError("boosts of a batch is a sequence with one entry per query")
    boosts = list(boosts)
    if len(boosts) != n_queries:
        raise ValueError(f"boosts has {len(boosts)} entries for {n_queries} queries")
    lists = [boost_rows(b, boost_weight, only_boosted, pid_to_row) for b in boosts]
    if all(b is None for b in lists):
        return None
    return lists, bool(only_boosted)


def load_product_sets(product_sets) -> dict:
    """Recommender(product_sets=): a mapping set name -> iterable of product ids, or the path of a JSON file of that
    shape -> {name: [product id, ...]} in the mapping's order (the order of the set ids on the index).  ValueError: not
    a mapping, no set at all, more than ICREC_MAX_ROWSETS sets, a set whose members are a string."""
    if isinstance(product_sets, (str, Path)):
        product_sets = json.loads(Path(product_sets).read_text())
    if not hasattr(product_sets, "items"):
        raise ValueError("product_sets must be a mapping set name -> product ids, or a JSON file of that shape")
    if not 1 <= len(product_sets) <= _native.ICREC_MAX_ROWSETS:
        raise ValueError(f"product_sets must hold 1 .. {_native.ICREC_MAX_ROWSETS} sets, got {len(product_sets)}")
    out = {}
    for name, ids in product_sets.items():
        if isinstance(ids, (str, bytes)) or hasattr(ids, "items"):
            raise ValueError(f"the members of product set {name!r} must be a list of product ids")
        out[str(name)] = [str(p) for p in ids]
    return out


def within_ids(within, names) -> Optional[list[int]]:
    """One request's `within` argument, checked before any GPU work -> None (unconstrained) or the ids of the named
    product sets: a set name, or up to ICREC_MAX_SETS_PER_QUERY names (the request sees their intersection; no name
    at all constrains nothing).  names: the recommender's set names in id order, None for a recommender without
    sets.  ValueError: within on a recommender without sets, an unknown name, a fifth name."""
    if within is None:
        return None
    if names is None:
        raise ValueError("within needs a recommender built with product_sets")
    asked = [within] if isinstance(within, str) else list(within)
    if len(asked) > _native.ICREC_MAX_SETS_PER_QUERY:
        raise ValueError(f"within names {len(asked)} product sets, more than {_native.ICREC_MAX_SETS_PER_QUERY}")
    code = {name: i for i, name in enumerate(names)}
    for name in asked:
        if name not in code:
            raise ValueError(f"unknown product set {name!r}")
    return [code[name] for name in asked]


def within_plan(within, n_queries: int, names):
    """A batch's `within` argument (None, or one entry per query, each as within_ids takes it) -> None (no query is
    constrained: the plain path) or the per-query id lists (None for an unconstrained query) rowset_ids takes."""
    if within is None:
        return None
    if isinstance(within, (str, bytes)):
        raise ValueError("within of a batch is a sequence with one entry per query")
    within = list(within)
    if len(within) != n_queries:
        raise ValueError(f"within has {len(within)} entries for {n_queries} queries")
    lists = [within_ids(w, names) for w in within]
    return None if all(ids is None for ids in lists) else lists


def boosts_within(lists, set_ids, member):
    """The host side of `boosts` under `within`: each query's {row: weight} list (boost_plan's; None: no list) without
    the rows outside one of the query's product sets.  icrec_boost_select does not look at row sets, so a listed row
    it is given is a row it may return; with these rows dropped and the candidates searched inside the sets, its
    result is the top k of the admissible rows under cosine + weight.  set_ids: within_plan's per-query id lists,
    member: bool [n_sets, n_rows], the recommender's own copy of the membership."""
    out = []
    for pairs, ids in zip(lists, set_ids):
        if pairs is None or not ids:
            out.append(pairs)
        else:
            out.append({r: w for r, w in pairs.items() if all(member[s, r] for s in ids)})
    return out


def cap_plan(max_per_aisle, max_per_department, has_facets: bool):
    """A request's `max_per_aisle` / `max_per_department` arguments, checked before any GPU work -> None (the plain
    request: both are None) or the caps (aisle, department) DeviceIndex.search_capped takes, 0 for the one that is None.
    Each is a positive integer; ValueError for anything else, and for caps on a catalog without facets."""
    if max_per_aisle is None and max_per_department is None:
        return None
    caps = []
    for what, v in (("max_per_aisle", max_per_aisle), ("max_per_department", max_per_department)):
        if v is None:
            caps.append(0)
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 2**31 - 1:
            raise ValueError(f"{what} must be an integer >= 1, got {v!r}")
        caps.append(int(v))
    if not has_facets:
        raise ValueError("max_per_aisle / max_per_department need a catalog with aisle / department facets (its texts "
                         "are not in the 'Product: .. Aisle: .. Department: ..' format)")
    return caps[0], caps[1]


def ann_plan(probes, n_lists, *, aisles=None, departments=None, boosts=None, only_boosted: bool = False, within=None,
             max_per_aisle=None, max_per_department=None):
    """A request's `probes` argument, checked before any GPU work -> None (the exact search: probes is None) or the
    number of lists the IVF search scans.  n_lists: the lists of the recommender's IvfIndex, None without one
    (Recommender(ann_lists=None)).  ValueError: probes without an IVF index, probes together with aisles, departments,
    boosts, within, max_per_aisle or max_per_department (the IVF scan reads neither facets nor boost lists nor row sets,
    and the rounds of a capped request are exact searches), probes outside
    [1, min(n_lists, ICREC_MAX_K)]."""
    if probes is None:
        return None
    if n_lists is None:
        raise ValueError("probes needs a recommender built with ann_lists")
    for what, given in (("aisles", aisles is not None), ("departments", departments is not None),
                        ("boosts", boosts is not None or bool(only_boosted)), ("within", within is not None),
                        ("max_per_aisle", max_per_aisle is not None),
                        ("max_per_department", max_per_department is not None)):
        if given:
            raise ValueError(f"probes cannot be combined with {what}: the IVF search takes exclusions and diversity only")
    limit = min(int(n_lists), _native.ICREC_MAX_K)
    if isinstance(probes, bool) or int(probes) != probes or not 1 <= int(probes) <= limit:
        raise ValueError(f"probes must be an integer in [1, {limit}], got {probes!r}")
    return int(probes)


def fusion_plan(history, cf_weight, rrf_c, has_cf: bool, n_queries: int, top_k: int, candidates, n_products: int, *,
                aisles=None, departments=None, within=None, boosts=None, only_boosted: bool = False, diversity=None,
                probes=None, max_per_aisle=None, max_per_department=None):
    """A batch's `history` / `cf_weight` / `rrf_c` arguments (history: None or one entry per query, each None or an
    iterable of product ids), checked before any GPU work -> None (the plain path: history is None, or every entry
    is) or (per-query id lists, cf_weight, rrf_c, the width of both lists).  In a batch that fuses, a None entry
    counts as [].  The width is `candidates`, default min(ICREC_MAX_K, 4 * top_k), clipped to the catalog, never below
    top_k's own clipped width.  ValueError: history on a recommender without cf, a string for a history, a count
    mismatch, cf_weight not a number >= 0, rrf_c not finite or <= -1, history together with aisles, departments,
    within, boosts / only_boosted, diversity, probes, max_per_aisle or max_per_department."""
    if history is None:
        return None
    if isinstance(history, (str, bytes)) or hasattr(history, "items"):
        raise ValueError("history of a batch is a sequence with one entry per query")
    history = list(history)
    if len(history) != n_queries:
        raise ValueError(f"history has {len(history)} entries for {n_queries} queries")
    if any(isinstance(h, (str, bytes)) or hasattr(h, "items") for h in history):
        raise ValueError("history must be an iterable of product ids, not a string or a mapping")
    if all(h is None for h in history):
        return None
    if not has_cf:
        raise ValueError("history needs a recommender built with cf (an ItemItemCFBaseline over the same products)")
    for what, given in (("aisles", aisles is not None), ("departments", departments is not None),
                        ("within", within is not None), ("boosts", boosts is not None or bool(only_boosted)),
                        ("diversity", diversity is not None and float(diversity) != 0.0), ("probes", probes is not None),
                        ("max_per_aisle", max_per_aisle is not None),
                        ("max_per_department", max_per_department is not None)):
        if given:
            raise ValueError(f"history cannot be combined with {what}: the CF list is the best of the WHOLE catalog and "
                             "knows no facets, product sets, boosts, caps or IVF lists; it takes exclude_product_ids and "
                             "candidates only")

    def number(v):
        try:
            return float(v)
        except (TypeError, ValueError):
            return float("nan")

    if not 0.0 <= number(cf_weight):  # (a NaN fails the comparison); rrf_weights' own rules, under this call's names
        raise ValueError(f"cf_weight must be a number >= 0, got {cf_weight!r}")
    if not -1.0 < number(rrf_c) < float("inf"):
        raise ValueError(f"rrf_c must be finite and > -1, got {rrf_c!r}")
    top_k = max(int(top_k), 1)
    n = int(candidates) if candidates is not None else min(_native.ICREC_MAX_K, 4 * top_k)
    width = max(min(n, n_products), min(top_k, n_products))
    return [[str(p) for p in (h or ())] for h in history], float(cf_weight), float(rrf_c), width


def compose_terms(like, unlike, like_weight, unlike_weight, pid_to_row) -> Optional[list[tuple[int, float]]]:
    """One request's `like` / `unlike` arguments, checked before any GPU work -> None (the plain request: no known id in
    either) or the terms DeviceIndex.compose_queries takes, [(catalog row, weight), ...]: `like` in the given order,
    then `unlike` with negated weights.  Each is None, an iterable of product ids - its n known ids then take
    like_weight / n each (-unlike_weight / n for unlike: Rocchio's centroids) - or a mapping id -> weight, taken as
    written (negated for unlike).  Ids the catalog does not have are skipped, as boost_rows skips them.  ValueError: a
    string for either, a weight (or like_weight, unlike_weight) that is not a finite number >= 0, an id in both, an id
    twice in one list, more than ICREC_MAX_TERMS known ids in total."""
    def weight(v, what):
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float("nan")
        if not 0.0 <= f < float("inf"):  # (a NaN fails the comparison)
            raise ValueError(f"{what} must be a finite number >= 0, got {v!r}")
        return f

    scale = {"like": weight(like_weight, "like_weight"), "unlike": -weight(unlike_weight, "unlike_weight")}
    terms: list[tuple[int, float]] = []
    seen: dict = {}
    for name, given in (("like", like), ("unlike", unlike)):
        if given is None:
            continue
        if isinstance(given, (str, bytes)):
            raise ValueError(f"{name} must be a mapping product id -> weight or an iterable of product ids, not a string")
        pairs = [(p, weight(v, f"the {name} weight of {p!r}")) for p, v in given.items()] if hasattr(given, "items") \
            else [(p, None) for p in given]
        for p, _ in pairs:
            if seen.get(p) == name:
                raise ValueError(f"product id {p!r} is named twice in {name}")
            if p in seen:
                raise ValueError(f"product id {p!r} is in both like and unlike")
            seen[p] = name
        known = [(pid_to_row[p], v) for p, v in pairs if p in pid_to_row]
        sign = 1.0 if name == "like" else -1.0
        terms.extend((r, scale[name] / len(known) if v is None else sign * v) for r, v in known)
    if len(terms) > _native.ICREC_MAX_TERMS:
        raise ValueError(f"{len(terms)} like / unlike products exceed the limit {_native.ICREC_MAX_TERMS}")
    return terms or None


def compose_plan(like, unlike, query_weight, like_weight, unlike_weight, n_queries: int, pid_to_row):
    """A batch's `like` / `unlike` arguments (each None or one entry per query, each entry as compose_terms takes it;
    query_weight, like_weight and unlike_weight: one value for the batch), checked before any GPU work -> None (the
    plain path: no query has a known id) or per query None or (query_weight, [(row, weight), ...]).  ValueError:
    compose_terms', like / unlike that is not a sequence with one entry per query, query_weight not a finite number
    >= 0."""
    if like is None and unlike is None:
        return None
    lists = {}
    for name, given in (("like", like), ("unlike", unlike)):
        if given is None:
            given = [None] * n_queries
        elif isinstance(given, (str, bytes)) or hasattr(given, "items") or not hasattr(given, "__len__"):
            raise ValueError(f"{name} of a batch is a sequence with one entry per query")
        given = list(given)
        if len(given) != n_queries:
            raise ValueError(f"{name} has {len(given)} entries for {n_queries} queries")
        lists[name] = given
    try:
        a = float(query_weight)
    except (TypeError, ValueError):
        a = float("nan")
    if not 0.0 <= a < float("inf"):
        raise ValueError(f"query_weight must be a finite number >= 0, got {query_weight!r}")
    terms = [compose_terms(lk, ul, like_weight, unlike_weight, pid_to_row) for lk, ul in zip(lists["like"], lists["unlike"])]
    if all(t is None for t in terms):
        return None
    return [None if t is None else (a, t) for t in terms]


def adapter_pairs_plan(pairs, pid_to_row, epochs, batch_size, negatives, lr, weight_decay, scale):
    """Recommender.fit_adapter's arguments, checked before any GPU work: pairs is a sequence of (context text, product
    id) -> (the texts, the catalog rows of their products).  ValueError: a string or a mapping for pairs, an entry that
    is not a (text, id) pair, a context that is not a string, a product id the catalog does not have (a pair teaches
    nothing without its stored row), and fit_plan's: no pair, sizes outside the kernel's limits, a hyper-parameter that
    is not a finite number."""
    if isinstance(pairs, (str, bytes)) or hasattr(pairs, "items"):
        raise ValueError("pairs must be a sequence of (context text, product id)")
    texts, rows = [], []
    for i, pair in enumerate(pairs):
        if isinstance(pair, (str, bytes)) or not hasattr(pair, "__len__") or len(pair) != 2:
            raise ValueError(f"pair {i} is not a (context text, product id) pair: {pair!r}")
        text, pid = pair
        if not isinstance(text, str):
            raise ValueError(f"the context of pair {i} must be a string, got {type(text).__name__}")
        if pid not in pid_to_row:
            raise ValueError(f"unknown product id {pid!r} in pair {i}: an adapter is trained against the catalog's stored rows")
        texts.append(text)
        rows.append(int(pid_to_row[pid]))
    fit_plan(len(texts), epochs, batch_size, negatives, lr, weight_decay, scale)
    return texts, rows


#: the gain of each event a deployed recommender records per shown product (the reference's four event types)
DEFAULT_GAINS = {"impression": 0, "click": 1, "add_to_cart": 2, "purchase": 4}


def adapter_lists_plan(impressions, pid_to_row, gains, epochs, batch_size, lr, weight_decay, scale, where=None):
    """Recommender.fit_adapter_lists' arguments, checked before any GPU work: impressions is a sequence of (context text,
    {product id: event name or number}) -> (the texts, per context its list [(catalog row, gain)]).  An event name is
    looked up in `gains`, a number is the gain itself.  `where`: what names impression i in a message (a file's
    "FILE:line"), else its position.  ValueError: a string or a mapping for impressions, an entry that is not a (text,
    mapping) pair, a context that is not a string, a product id the catalog does not have, an event `gains` does not
    have, a gain that is negative or not finite (in `gains` too), more than ICREC_ADAPTER_MAX_LIST products in one
    list, a list without a positive gain (it teaches nothing), and fit_plan's."""
    if isinstance(impressions, (str, bytes)) or hasattr(impressions, "items"):
        raise ValueError("impressions must be a sequence of (context text, {product id: event or gain})")

    def gain_of(v, what):
        if isinstance(v, str):
            if v not in gains:
                raise ValueError(f"unknown event {v!r} {what} (known: {', '.join(sorted(gains))})")
            v = gains[v]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"a gain must be a finite number >= 0, got {v!r} {what}")
        return float(v)

    for event in gains:
        gain_of(gains[event], f"for event {event!r}")
    texts, lists = [], []
    for i, entry in enumerate(impressions):
        at = where[i] if where is not None else f"impression {i}"
        if isinstance(entry, (str, bytes)) or not hasattr(entry, "__len__") or len(entry) != 2 or not hasattr(entry[1], "items"):
            raise ValueError(f"{at} is not a (context text, {{product id: event or gain}}) pair: {entry!r}")
        text, products = entry
        if not isinstance(text, str):
            raise ValueError(f"{at}: the context must be a string, got {type(text).__name__}")
        if len(products) > _native.ICREC_ADAPTER_MAX_LIST:
            raise ValueError(f"{at} lists {len(products)} products, the limit is {_native.ICREC_ADAPTER_MAX_LIST}")
        entries = []
        for pid, v in products.items():
            if pid not in pid_to_row:
                raise ValueError(f"unknown product id {pid!r} in {at}: an adapter is trained against the catalog's stored rows")
            entries.append((int(pid_to_row[pid]), gain_of(v, f"for product {pid!r} in {at}")))
        if not any(g > 0 for _, g in entries):
            raise ValueError(f"{at} has no product with a positive gain: it teaches nothing")
        texts.append(text)
        lists.append(entries)
    fit_plan(len(texts), epochs, batch_size, 0, lr, weight_decay, scale)
    return texts, lists


@dataclass(frozen=True)
class RequestPlan:
    """What a request asks beyond (queries, top_k, exclusions), checked (Recommender._plan); None / False: not asked."""

    allow: Optional[list] = None  # per query None or (aisle codes, department codes): Recommender._facet_allow
    sets: Optional[list] = None  # per query None or the ids of its product sets: within_plan
    boost: Optional[list] = None  # per query None or {row: weight}, without the rows outside the query's sets
    only_boosted: bool = False  # rank the rows of `boost` alone: no search
    caps: Optional[tuple] = None  # (aisle, department) caps: cap_plan
    mmr: Optional[tuple] = None  # (lambda, candidates): diversity_plan
    probes: Optional[int] = None  # the lists of the IVF index to scan: ann_plan
    width: Optional[int] = None  # the request's raw `candidates`: what DeviceIndex.search_capped searches per round
    fuse: Optional[tuple] = None  # (per-query history ids, cf_weight, rrf_c, the width of both lists): fusion_plan
    compose: Optional[list] = None  # per query None or (query weight, [(row, weight), ...]): compose_plan

    @property
    def plain(self) -> bool:
        """Nothing asked: the search is `DeviceIndex.search(q, k, exclude)`, which the graph path may serve."""
        return (self.allow, self.sets, self.boost, self.caps, self.mmr, self.probes, self.fuse, self.compose) == (None,) * 8


PLAIN = RequestPlan()  # what Recommender._plan returns for every request that asks nothing


class SbertModel:
    """What `self.model` is in the reference (a SentenceTransformer): tokenizer + device encoder
    with an `encode(texts, batch_size, show_progress_bar, normalize_embeddings)` method."""

    def __init__(self, loaded: LoadedModel, device: torch.device):
        self.tokenizer = loaded.tokenizer
        self.max_seq_length = loaded.max_seq_length
        self.shape = loaded.shape
        self.device = device
        self.pooling = loaded.pooling
        self.attention_bias = loaded.attention_bias  # the MPNet family's relative-position table, or None
        self.encoder = DeviceEncoder(loaded.weights, loaded.shape, device, max_seq_length=loaded.max_seq_length,
                                     pooling=loaded.pooling, attention_bias=loaded.attention_bias)
        self._weights = loaded.weights
        self._encoder_no_flag: Optional[DeviceEncoder] = None  # normalize_embeddings=False: one normalisation fewer

    def encode_to_device(self, texts: Sequence[str], tokens_per_call: int = 1 << 18) -> torch.Tensor:
        """Embeddings [n, hidden] left on the GPU (serving path: no host round trip)."""
        return self.encoder.encode_packed_host(*self.tokenizer.packed(texts), max_tokens_per_call=tokens_per_call)

    def encode(self, sentences, batch_size: int = 64, show_progress_bar: bool = False,
               normalize_embeddings: bool = True, **_ignored) -> np.ndarray:
        """SentenceTransformer.encode-compatible: numpy float32 [n, hidden] (or [hidden] for a str).

        The reference pads and runs `batch_size` texts per forward; packed varlen batching makes
        the result independent of batch composition, so `batch_size` only bounds tokens per call."""
        single = isinstance(sentences, str)
        texts = [sentences] if single else list(sentences)
        if not texts:
            return np.zeros((0, self.shape.hidden), np.float32)
        if normalize_embeddings or self.shape.n_normalize < 1:
            enc = self.encoder
        else:
            # the flag's F.normalize is the LAST of the n_normalize passes the device encoder applies (the
            # pipeline's own Normalize module, if any, stays): a second encoder configured with one pass fewer
            if self._encoder_no_flag is None:
                from dataclasses import replace

                self._encoder_no_flag = DeviceEncoder(self._weights, replace(self.shape, n_normalize=self.shape.n_normalize - 1),
                                                      self.device, gemm_mode=self.encoder.gemm_mode,
                                                      max_seq_length=self.max_seq_length, pooling=self.pooling,
                                                      attention_bias=self.attention_bias)
            enc = self._encoder_no_flag
        per_call = max(int(batch_size), 1) * 4096
        emb = enc.encode_packed_host(*self.tokenizer.packed(texts), max_tokens_per_call=per_call).cpu().numpy()
        return emb[0] if single else emb


class Recommender:
    """Two-tower recommender: same surface as the reference's Recommender (:133-225)."""

    _ann: Optional[IvfIndex] = None  # the IVF index beside _index (ann_lists), searched by requests that pass `probes`
    product_sets: Optional[list[str]] = None  # the names of the product sets (product_sets=), in set id order
    _set_member: Optional[np.ndarray] = None  # bool [n_sets, n_products]: the host's copy of the membership
    _emb_block: Optional[np.ndarray] = None  # add_products / remove_products: the block product_embeddings is a view of
    aisles: Optional[list[str]] = None  # the catalog's aisle and department names (_set_facets); None: it has no facets
    departments: Optional[list[str]] = None
    _cf = None  # the ItemItemCFBaseline over the same products (cf=), ranked by requests that pass `history`
    _adapter: Optional[QueryAdapter] = None  # the query adapter every text query goes through (adapter=, set_adapter)
    _fast = None

    def __init__(self, model_dir: Path | str, corpus_path: Path, batch_size: int = 64, use_index: bool = True,
                 ann_lists: int | None = None, product_sets=None, cf=None, adapter=None):
        self.model_dir = self._resolve_model_dir(model_dir)
        self.corpus_path = Path(corpus_path).resolve()
        self.product_ids, self.product_texts = self._load_corpus()
        self.pid_to_text = dict(zip(self.product_ids, self.product_texts))
        self._pid_to_row = {pid: i for i, pid in enumerate(self.product_ids)}
        self._set_cf(cf)
        self.device = self._inference_device()
        self.model = self._load_model()
        self.product_embeddings = self._load_or_build_embeddings(batch_size, use_index)
        # fp32 rows + f16 filter planes: large batches (>= 256 queries) rank on the f16 matrix cores and are verified
        # exactly — same bits out as plain "f32" (ICREC_INDEX_STORAGE=f32 turns the planes off, =bf16 halves the rows)
        self._index = DeviceIndex(self.product_embeddings, self.device,
                                  storage=os.getenv("ICREC_INDEX_STORAGE", "f32+filter"))
        self._set_facets()
        self._set_product_sets(product_sets)
        # ann_lists: an IVF index of that many lists beside the exact one (a second copy of the rows); only requests
        # that pass `probes` search it
        self._ann = IvfIndex(self._index, train_centroids(self._index, int(ann_lists))) if ann_lists else None
        self._fast = None
        if os.getenv("ICREC_USE_GRAPH", "1") != "0":
            from .fastpath import SingleRequestPath

            self._fast = SingleRequestPath(self.model.encoder, self._index)
        if adapter is not None:
            self.set_adapter(adapter)

    # -- construction helpers (names follow the reference) ---------------------------------
    def _resolve_model_dir(self, model_dir: Path | str) -> Path | str:
        p = Path(model_dir)
        return p.resolve() if p.exists() else model_dir

    def _load_corpus(self) -> tuple[list[str], list[str]]:
        """eval_corpus.json: {product_id: text}; key order = row order of the embedding matrix."""
        with open(self.corpus_path) as f:
            corpus = json.load(f)
        ids = list(corpus.keys())
        return ids, [corpus[pid] for pid in ids]

    def _inference_device(self) -> torch.device:
        """INFERENCE_DEVICE env ("cuda", "cuda:1") or the current HIP device.  This build has no
        CPU/MPS path: anything else raises."""
        override = os.getenv("INFERENCE_DEVICE")
        name = override or "cuda"
        dev = torch.device(name)
        if dev.type != "cuda":
            raise _native.IcrecError(f"INFERENCE_DEVICE={name!r}: this build runs on MI355X (cuda/HIP devices) only")
        if not torch.cuda.is_available():
            raise _native.IcrecError("no HIP device visible; the MI355X kernels have no CPU fallback")
        return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())

    def _load_model(self) -> SbertModel:
        logger.info("Using inference device: %s", self.device)
        return SbertModel(load_model_dir(self.model_dir), self.device)

    def _load_or_build_embeddings(self, batch_size: int, use_index: bool) -> np.ndarray:
        index = EmbeddingIndex(self.corpus_path, self.model_dir)
        if use_index:
            cached = index.load(self.product_ids)
            if cached is not None:
                logger.info("Loaded model from %s, corpus %d products (embeddings from index)", self.model_dir,
                            len(self.product_ids))
                return cached
        embeddings = self.model.encode(self.product_texts, batch_size=batch_size, show_progress_bar=True,
                                       normalize_embeddings=True)
        if use_index:
            index.save(self.product_ids, embeddings)
        logger.info("Loaded model from %s, corpus %d products", self.model_dir, len(self.product_ids))
        return embeddings

    def _set_facets(self) -> None:
        """Aisle and department codes of the catalog texts onto the index (a re-index builds a new Recommender and
        so comes through here too); a catalog in another format has none: .aisles / .departments are then None."""
        parsed = catalog_facets(self.product_texts)
        self.aisles, self.departments = (parsed[0], parsed[1]) if parsed else (None, None)
        if parsed:
            self._index.set_facets(parsed[2])

    def _set_cf(self, cf) -> None:
        """cf: an ItemItemCFBaseline whose candidates are numbered like the catalog rows - cf.corpus_ids equal to
        product_ids, the same ids in the same order - or None.  ValueError otherwise, before the model is loaded."""
        if cf is not None and list(cf.corpus_ids) != list(self.product_ids):
            raise ValueError("cf.corpus_ids must be the catalog's product_ids, the same ids in the same order: the CF "
                             "candidates are numbered like the catalog rows")
        self._cf = cf

    def set_adapter(self, adapter) -> None:
        """Install a query adapter - a QueryAdapter, or the path of a file QueryAdapter.save wrote - or remove it (None).
        The adapter is the recommender's, not a request's: every query with a text part (recommend, recommend_batch,
        recommend_batches, recommend_batch_timed) is q' = q + D q right after the encode, before like / unlike compose
        it; recommend_from_products and similar_products, whose queries are stored rows already, do not use it.  With
        None nothing new is launched anywhere.  The captured single-request graphs are dropped and captured again on
        the next request (with the adapter they hold one more node); training the installed adapter in place needs no
        reset.  A set-up call, like update_products.  ValueError: an adapter of another width or on another device."""
        if adapter is not None and not isinstance(adapter, QueryAdapter):
            adapter = QueryAdapter.load(adapter, self.device)
        if adapter is not None and (adapter.dim != self._index.dim or adapter.device != self.device):
            raise ValueError(f"the adapter is {adapter.dim} wide on {adapter.device}, the index {self._index.dim} wide on "
                             f"{self.device}")
        self._adapter = adapter
        if self._fast is not None:
            self._fast.set_adapter(adapter)

    def fit_adapter(self, pairs, epochs: int = 5, batch_size: int = 64, negatives=0, lr: float = 2e-3,
                    weight_decay: float = 0.01, scale: float = DEFAULT_SCALE, seed: int = 0) -> list[float]:
        """Learn the query adapter from (context text, product id) pairs - clicks or purchases on this catalog - with the
        reference's loss (MultipleNegativesRankingLoss, scale 30; QueryAdapter.fit) -> the per-step losses.  The
        contexts are encoded once with the frozen encoder; the positives are catalog products, so their embeddings are
        the index's stored rows and no product is encoded.  The installed adapter is trained further, in place (the
        captured graphs stay and answer from the new weights); without one a new adapter is trained and installed.
        negatives: extra rows drawn from the whole catalog per step, beside the in-batch negatives, or "all": every
        step is the exact cross-entropy against every stored row (QueryAdapter.step_catalog).  ValueError before
        any GPU work: adapter_pairs_plan's - above all a product id the catalog does not have.  A set-up call: never
        while a request is being served."""
        texts, rows = adapter_pairs_plan(pairs, self._pid_to_row, epochs, batch_size, negatives, lr, weight_decay, scale)
        anchors = self.model.encode_to_device(texts)
        return self._train_adapter(lambda adapter: adapter.fit(self._index, anchors, rows, epochs, batch_size, negatives, lr,
                                                               weight_decay, scale, seed))

    def _train_adapter(self, train) -> list[float]:
        """train(adapter) -> losses, on the installed adapter in place, or on a new one that is then installed."""
        adapter = self._adapter if self._adapter is not None else QueryAdapter(self._index.dim, self.device)
        losses = train(adapter)
        torch.cuda.current_stream(self.device).synchronize()  # the graphs replay on a stream of their own
        if adapter is not self._adapter:
            self.set_adapter(adapter)
        return losses

    def fit_adapter_lists(self, impressions, gains=DEFAULT_GAINS, epochs: int = 5, batch_size: int = 64, lr: float = 2e-3,
                          weight_decay: float = 0.01, scale: float = DEFAULT_SCALE, seed: int = 0, where=None) -> list[float]:
        """Learn the query adapter from impression lists - per context the products that were shown and what happened
        to each: (context text, {product id: event name or gain}) - with the listwise softmax cross-entropy
        (QueryAdapter.fit_lists) -> the per-step losses.  An event's gain comes from `gains` (the reference's four event
        types); a context's negatives are its own shown-but-ignored products, nothing is drawn.  The contexts are
        encoded once, no product is encoded, and the installed adapter is trained in place, as fit_adapter does.
        ValueError before any GPU work: adapter_lists_plan's.  A set-up call: never while a request is being served."""
        texts, lists = adapter_lists_plan(impressions, self._pid_to_row, gains, epochs, batch_size, lr, weight_decay, scale, where)
        anchors = self.model.encode_to_device(texts)
        return self._train_adapter(lambda adapter: adapter.fit_lists(self._index, anchors, lists, epochs, batch_size, lr,
                                                                     weight_decay, scale, seed))

    def _member_row(self, product_ids) -> np.ndarray:
        """bool [n_products]: which catalog rows the given product ids name; ids the catalog does not have are skipped."""
        row = np.zeros(len(self.product_ids), bool)
        rows = [self._pid_to_row[p] for p in product_ids if p in self._pid_to_row]
        row[rows] = True
        return row

    def _set_product_sets(self, product_sets) -> None:
        """Named product sets (store assortments, "in stock", "vegan": a product may be in any number of them) onto
        the index as row sets, in the mapping's order; the host keeps the membership (boosts_within reads it).  None:
        the recommender has no sets and `within` raises."""
        self.product_sets, self._set_member = None, None
        if product_sets is None:
            return
        table = load_product_sets(product_sets)
        self._set_member = np.stack([self._member_row(ids) for ids in table.values()])
        self._index.set_rowsets(rowset_bits(self._set_member, len(self.product_ids)))
        self.product_sets = list(table)

    def update_product_set(self, name: str, product_ids) -> None:
        """Replace the members of one product set (an in-stock set that changes through the day); ids the catalog does
        not have are skipped.  The next request sees the new members.  A set-up call on the index: never while a
        request is being served.  ValueError: a recommender without sets, an unknown name."""
        ids = within_ids(name, self.product_sets)
        if ids is None or isinstance(product_ids, (str, bytes)):
            raise ValueError("update_product_set takes a set name and a list of product ids")
        row = self._member_row(product_ids)
        self._index.write_rowset(ids[0], rowset_bits(row[None, :], len(self.product_ids))[0])
        self._set_member[ids[0]] = row

    def update_products(self, updates) -> None:
        """Give products new texts without a re-index: updates is a mapping product id -> new text.  The new texts are
        encoded as the catalog was (normalize_embeddings=True), their rows and filter copies are rewritten on the
        device in place (DeviceIndex.write_rows: afterwards the index is bit for bit the one a new Recommender builds
        from the edited corpus) and, on a catalog with facets, so are their aisle and department codes
        (DeviceIndex.write_facets; a new aisle or department name is appended to .aisles / .departments, the codes of
        the others stay).  product_texts, pid_to_text and product_embeddings follow, and the IVF index of a
        recommender built with ann_lists is built again from its centroids (IvfIndex.rebuild).  No pointer of the
        index changes: the captured single-request graphs stay and answer from the new rows.
        ValueError, with nothing changed: an id the catalog does not have (add_products and remove_products change the
        number of rows), a text that does not parse on a catalog with facets, a 257th aisle or
        department name (product_update_plan).  An empty mapping does nothing.
        The limits: it is a set-up call on the index, never to be made while a request is being served.  The corpus
        file and the on-disk EmbeddingIndex cache are not rewritten: a process started later reads the old texts.  A
        RerankedRecommender built on this recommender keeps its own token store and must be built again.  Product sets
        are untouched: a product's membership is changed with update_product_set."""
        rows, texts, codes, aisles, departments = product_update_plan(updates, self._pid_to_row, self.product_texts,
                                                                       self.aisles, self.departments)
        if not rows:
            return
        emb = self.model.encode(texts, show_progress_bar=False, normalize_embeddings=True)
        self._index.write_rows(rows, emb)
        if codes is not None:
            self._index.write_facets(rows, codes)
        torch.cuda.current_stream(self.device).synchronize()  # the graphs replay on a stream of their own
        if not self.product_embeddings.flags.writeable:
            self.product_embeddings = np.array(self.product_embeddings)
        self.product_embeddings[rows] = emb
        for r, text in zip(rows, texts):
            self.product_texts[r] = text
            self.pid_to_text[self.product_ids[r]] = text
        self.aisles, self.departments = aisles, departments
        if self._ann is not None:
            self._ann.rebuild()

    def _after_resize(self) -> None:
        """The number of rows changed: wait for the device, drop the captured single-request graphs (n_rows is an
        argument of their search kernels, and a reserve moved the arrays) and build the IVF index again from its
        centroids."""
        torch.cuda.current_stream(self.device).synchronize()
        if self._fast is not None:
            self._fast.reset()
        if self._ann is not None:
            self._ann.rebuild()

    def _embedding_block(self, room: int) -> np.ndarray:
        """The host block product_embeddings is a view of the front of, writable and with room for `room` more rows
        (grown by doubling, like the index's capacity): adding and removing products then costs the host what it costs
        the device, the edited rows and not the catalog."""
        n, block = len(self.product_embeddings), self._emb_block
        if block is None or self.product_embeddings.base is not block or block.shape[0] < n + room:
            block = np.empty((max(2 * n, n + room), self.product_embeddings.shape[1]), np.float32)
            block[:n] = self.product_embeddings
            self._emb_block = block
            self.product_embeddings = block[:n]
        return block

    def add_products(self, additions) -> None:
        """Add products without a re-index: additions is a mapping product id -> text.  The texts are encoded as the
        catalog was (normalize_embeddings=True) and appended to the device index in place (DeviceIndex.append_rows,
        which doubles the index's capacity when it is full), on a catalog with facets together with their aisle and
        department codes (a new name is appended behind .aisles / .departments).  The new products take the rows behind
        the last one, in the mapping's order, and join no product set (update_product_set).  product_ids,
        product_texts, pid_to_text, product_embeddings and the host's set membership follow; the captured
        single-request graphs are dropped and captured again on the next request, and the IVF index of a recommender
        built with ann_lists is built again from its centroids.
        ValueError, with nothing changed: an id the catalog already has, a text that does not parse on a catalog with
        facets, a 257th aisle or department name (product_add_plan).  An empty mapping does nothing.
        The limits are update_products': a set-up call, never made while a request is being served; the corpus file
        and the on-disk EmbeddingIndex cache are not rewritten; a RerankedRecommender built on this recommender keeps
        its own token store and must be built again."""
        ids, texts, codes, aisles, departments = product_add_plan(additions, self._pid_to_row, self.aisles, self.departments)
        if not ids:
            return
        emb = np.asarray(self.model.encode(texts, show_progress_bar=False, normalize_embeddings=True), np.float32)
        new_rows = self._index.append_rows(emb, codes)
        block, n = self._embedding_block(len(ids)), len(self.product_ids)
        block[n:n + len(ids)] = emb
        self.product_embeddings = block[:n + len(ids)]
        for r, pid, text in zip(new_rows, ids, texts):
            self.product_ids.append(pid)
            self.product_texts.append(text)
            self.pid_to_text[pid] = text
            self._pid_to_row[pid] = r
        if codes is not None:
            self.aisles, self.departments = aisles, departments
        if self._set_member is not None:
            self._set_member = np.concatenate([self._set_member, np.zeros((self._set_member.shape[0], len(ids)), bool)], axis=1)
        self._after_resize()

    def remove_products(self, product_ids) -> None:
        """Remove products without a re-index: product_ids is a list of ids the catalog has.  Their rows leave the device
        index in place (DeviceIndex.remove_rows): the last surviving rows move into the places of the removed ones, so
        the cost follows the number of removed products, not the catalog.  ROW ORDER: afterwards the rows are in the
        swapped order - .product_ids is the truth, not the corpus file's key order.  product_ids, product_texts,
        pid_to_text, product_embeddings and the host's set membership follow the moves (a moved product stays in its
        sets); aisle and department names stay, also those no product carries any more.  The captured single-request
        graphs are dropped, the IVF index is built again from its centroids.
        ValueError, with nothing changed: an id the catalog does not have, an id named twice, a list that names every
        product (product_remove_plan), a recommender built with cf (the removal renumbers rows, and the CF handle
        cannot follow).  An empty list does nothing.  The limits are add_products'."""
        if self._cf is not None:
            raise ValueError("remove_products renumbers catalog rows, which the cf baseline of this recommender cannot "
                             "follow: build the recommender again")
        rows = product_remove_plan(product_ids, self._pid_to_row)
        if not rows:
            return
        dst, src = self._index.remove_rows(rows)
        new_n = len(self.product_ids) - len(rows)
        for r in rows:
            pid = self.product_ids[r]
            del self.pid_to_text[pid], self._pid_to_row[pid]
        for d, s in zip(dst.tolist(), src.tolist()):
            self.product_ids[d], self.product_texts[d] = self.product_ids[s], self.product_texts[s]
            self._pid_to_row[self.product_ids[d]] = d
        del self.product_ids[new_n:], self.product_texts[new_n:]
        block = self._embedding_block(0)
        block[dst] = block[src]
        self.product_embeddings = block[:new_n]
        if self._set_member is not None:
            self._set_member = apply_moves(self._set_member, new_n, dst, src, axis=1)
        self._after_resize()

    # -- the hot path -------------------------------------------------------------------------
    def _k(self, top_k: int) -> int:
        """The search width for a request's top_k, checked before any GPU work: at least 1 (the reference's loop
        appends before testing len >= top_k, :223-224), at most the catalog."""
        top_k = max(int(top_k), 1)
        if top_k > _native.ICREC_MAX_K:
            raise ValueError(f"top_k={top_k} exceeds the kernel limit {_native.ICREC_MAX_K} "
                             "(the API schema allows at most 100)")
        return min(top_k, len(self.product_ids))

    def _exclusion_rows(self, exclude_product_ids) -> Optional[list[list[int]]]:
        """Per-query product-id sets -> per-query catalog rows, or None when nothing is excluded."""
        if exclude_product_ids is None or not any(exclude_product_ids):
            return None
        return [[self._pid_to_row[p] for p in e if p in self._pid_to_row] if e else [] for e in exclude_product_ids]

    def _facet_allow(self, aisles, departments, n: int):
        """Per-query aisle / department name lists (each None, or n entries of None or an iterable of names) -> the
        per-query constraints facet_masks takes, or None when no query is constrained."""
        if aisles is None and departments is None:
            return None
        if self.aisles is None:
            raise ValueError("this catalog has no aisle / department facets (its texts are not in the "
                             "'Product: .. Aisle: .. Department: ..' format)")
        per_facet = []
        for what, given, known in (("aisle", aisles, self.aisles), ("department", departments, self.departments)):
            if given is None:
                given = [None] * n
            if len(given) != n:
                raise ValueError(f"{what}s has {len(given)} entries for {n} queries")
            code = {name: i for i, name in enumerate(known)}
            col = []
            for names in given:
                if names is None:
                    col.append(None)
                    continue
                names = [names] if isinstance(names, str) else list(names)
                unknown = [x for x in names if x not in code]
                if unknown:
                    raise ValueError(f"unknown {what} {unknown[0]!r}")
                col.append([code[x] for x in names])
            per_facet.append(col)
        if all(a is None and d is None for a, d in zip(*per_facet)):
            return None
        return [None if a is None and d is None else (a, d) for a, d in zip(*per_facet)]

    def _plan(self, n_queries: int, top_k: int, *, aisles=None, departments=None, diversity=None, candidates=None,
              boosts=None, boost_weight=None, only_boosted=False, probes=None, within=None, max_per_aisle=None,
              max_per_department=None, history=None, cf_weight=1.0, rrf_c=60.0, like=None, unlike=None,
              query_weight=1.0, like_weight=1.0, unlike_weight=0.5) -> RequestPlan:
        """A request's options in recommend_batch's form (aisles, departments, boosts, within, like and unlike: None or
        one entry per query), checked before any GPU work -> its RequestPlan; the one caller of the *_plan functions, in
        the order ann, caps, within, diversity, facets, boosts, fusion, compose.  Boosted rows outside a query's product
        sets are dropped here.
        A request that asks nothing gets the shared PLAIN (`candidates` alone asks nothing: it is only a width)."""
        if probes is not None:  # (n_lists is a library call: made for the requests that probe)
            probes = ann_plan(probes, self._ann.n_lists if self._ann else None, aisles=aisles, departments=departments,
                              boosts=boosts, only_boosted=only_boosted, within=within, max_per_aisle=max_per_aisle,
                              max_per_department=max_per_department)
        caps = cap_plan(max_per_aisle, max_per_department, self.aisles is not None)
        sets = within_plan(within, n_queries, self.product_sets)
        mmr = diversity_plan(diversity, candidates, top_k, len(self.product_ids))
        allow = self._facet_allow(aisles, departments, n_queries)
        boost, only = boost_plan(boosts, boost_weight, only_boosted, n_queries, self._pid_to_row) or (None, False)
        fuse = None
        if history is not None:
            fuse = fusion_plan(history, cf_weight, rrf_c, self._cf is not None, n_queries, top_k, candidates,
                               len(self.product_ids), aisles=aisles, departments=departments, within=within, boosts=boosts,
                               only_boosted=only_boosted, diversity=diversity, probes=probes, max_per_aisle=max_per_aisle,
                               max_per_department=max_per_department)
        compose = compose_plan(like, unlike, query_weight, like_weight, unlike_weight, n_queries, self._pid_to_row)
        if (allow, sets, boost, caps, mmr, probes, fuse, compose) == (None,) * 8:
            return PLAIN
        if boost is not None and sets is not None:
            boost = boosts_within(boost, sets, self._set_member)
        return RequestPlan(allow, sets, boost, only, caps, mmr, probes, candidates, fuse, compose)  # (the fields' order; keywords cost 0.3 us)

    def _encode_search(self, ids: np.ndarray, cu: np.ndarray, k: int, ex, plan: RequestPlan, timed: bool = False):
        """Packed token ids -> (idx, scores) host arrays [n, k] through the un-captured encode and search on the
        current stream; timed=True adds (encode ms, search ms) from HIP events around the two.  With an adapter set the
        encoder's vectors go through it first (QueryAdapter.apply); with plan.compose they are then replaced by the
        composed queries (_composed; both count into the search time); ids None (recommend_from_products) runs no encoder at all: the queries are plan.compose's terms
        alone.  The search is three steps:
        1. the SOURCE ranking, w wide: the IVF index's with plan.probes (it takes exclusions only), else
           DeviceIndex.ranked under plan.allow's masks and plan.sets' ids (with plan.boost the listed rows are merged in);
        2. with plan.caps, one round of DeviceIndex.cap_select thins the list at its own width;
        3. with plan.mmr = (lambda, candidates), w = candidates and DeviceIndex.mmr_select re-selects the k results
           from the exact index's rows; without it w = k.
        The exception is caps without mmr: the k results are the capped walk of the WHOLE source ranking, which
        DeviceIndex.search_capped takes in rounds of plan.width candidates (None: its default).
        With plan.fuse the fused list is a fourth kind of source ranking, and the only step (fusion_plan refuses the
        rest): the content search w wide under the exclusions, icrec_cf_rank w wide on the histories, and fuse_select
        with the same exclusions to k (_fused)."""
        n = len(cu) - 1 if ids is not None else len(plan.compose)
        sets = None if plan.sets is None else rowset_ids(plan.sets, n, None, self.device)
        allow = None if plan.allow is None else facet_masks(plan.allow, n, self._index.n_facets, self.device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timed else None
        stream = torch.cuda.current_stream(self.device)
        if ev:
            ev[0].record(stream)
        emb = self.model.encoder.encode_packed_host(ids, cu) if ids is not None else None
        if ev:
            ev[1].record(stream)
        if self._adapter is not None and emb is not None:
            emb = self._adapter.apply(emb)
        if plan.compose is not None:
            emb = self._composed(emb, plan.compose)
        if plan.fuse is not None:
            idx, sc = self._fused(emb, k, ex, plan.fuse)
        elif plan.caps is not None and plan.mmr is None:
            idx, sc = self._index.search_capped(emb, k, plan.caps, plan.width, ex, allow, sets, plan.boost,
                                                only=plan.only_boosted)
        else:
            w = k if plan.mmr is None else plan.mmr[1]
            if plan.probes is not None:
                idx, sc = self._ann.search(emb, w, plan.probes, ex)
            else:
                idx, sc = self._index.ranked(emb, w, ex, allow, sets, plan.boost, plan.only_boosted)
            if plan.caps is not None:
                idx, sc = self._index.cap_select(idx, sc, plan.caps, w)[:2]
            if plan.mmr is not None:
                idx, sc = self._index.mmr_select(idx, sc, k, plan.mmr[0])
        if ev:
            ev[2].record(stream)
        idx, sc = idx.cpu().numpy(), sc.cpu().numpy()  # synchronises the stream
        return (idx, sc, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])) if ev else (idx, sc)

    def _composed(self, emb: Optional[torch.Tensor], compose) -> torch.Tensor:
        """The queries of plan.compose (per query None or (query weight, terms)) on the encoder's vectors emb [n, dim], or
        without a text part when emb is None: DeviceIndex.compose_queries.  A query without terms keeps the encoder's
        own vector, bit for bit: it is then the request it is alone."""
        q = self._index.compose_queries(emb, [c and c[1] for c in compose],
                                        None if emb is None else [c[0] if c else 1.0 for c in compose])
        untouched = [i for i, c in enumerate(compose) if c is None]
        if emb is not None and untouched:
            at = torch.tensor(untouched, dtype=torch.int64, device=self.device)
            q[at] = emb[at]
        return q

    #: the CF workspace one pass of _cf_ranked may allocate, and icrec_cf_rank's own limit on the queries of a call
    CF_PASS_BYTES, CF_PASS_QUERIES = 1 << 30, 65535

    def _cf_ranked(self, histories, w: int):
        """(rows int64 [n, w], scores int32 [n, w]) of icrec_cf_rank on per-query product-id lists, in passes of at
        most CF_PASS_QUERIES queries whose workspace (icrec_cf_rank_workspace_bytes) stays under CF_PASS_BYTES."""
        n = len(histories)
        step = min(n, self.CF_PASS_QUERIES)
        while step > 1 and self._cf.rank_workspace_bytes(step, w) >= self.CF_PASS_BYTES:
            step = (step + 1) // 2
        parts = [self._cf.rank_rows_scores(self._cf.history_csr_from(histories[s:s + step]), w) for s in range(0, n, step)]
        return (parts[0] if len(parts) == 1 else tuple(torch.cat(t) for t in zip(*parts)))

    def _fused(self, emb: torch.Tensor, k: int, ex, fuse):
        """The fused source ranking of plan.fuse = (histories, cf_weight, rrf_c, w): (idx, fused scores) [n, k].  Rows
        that add_products appended lie beyond the CF candidates: CF never lists them, the content list may."""
        histories, cf_weight, rrf_c, w = fuse
        a_idx, _ = self._index.search(emb, w, ex)
        b_idx, b_sc = self._cf_ranked(histories, w)
        a_w = torch.from_numpy(rrf_weights(w, rrf_c, 1.0)).to(self.device)
        b_w = torch.from_numpy(rrf_weights(w, rrf_c, cf_weight)).to(self.device)
        return fuse_select(a_idx, b_idx, a_w, b_w, k, len(self.product_ids), b_gate=b_sc, exclude=ex)

    def _recommend_one(self, query: str, top_k: int, exclude_product_ids, timed: bool = False, **options):
        """One request (options: recommend's keywords): a replayed hipGraph (fastpath.py) when its plan is plain - no
        aisles, departments, product sets, diversity, boosts, probes, caps, history, like or unlike - and a graph supports it, else the
        un-captured path.  -> results; timed=True: (results, encode ms incl. host tokenisation, search ms)."""
        k = self._k(top_k)
        for name in ("aisles", "departments", "within", "boosts", "history", "like", "unlike"):  # the per-query options, in the batch's form
            if options.get(name) is not None:
                options[name] = [options[name]]
        plan = self._plan(1, top_k, **options)
        t0 = time.time()
        ids, cu = self.model.tokenizer.packed([query])
        tok_ms = (time.time() - t0) * 1000
        ex = self._exclusion_rows([exclude_product_ids])
        rows = ex[0] if ex else []
        fast = self._fast_path() if plan.plain else None
        if fast is not None and fast.supports(len(ids), k, len(rows)):
            idx, sc, *ms = fast.run(ids, k, rows, timed=timed)
        else:
            idx, sc, *ms = self._encode_search(ids, cu, k, ex, plan, timed)
            idx, sc = idx[0], sc[0]
        results = self._to_results(idx, sc)
        return (results, tok_ms + ms[0], ms[1]) if timed else results

    def _to_results(self, idx_row: np.ndarray, sc_row: np.ndarray) -> list[tuple[str, float]]:
        return [(self.product_ids[int(i)], float(s)) for i, s in zip(idx_row, sc_row) if i >= 0]

    def recommend_batch(self, queries: Sequence[str], top_k: int = 10,
                        exclude_product_ids: Optional[Sequence[Optional[set[str]]]] = None, *,
                        aisles: Optional[Sequence[Optional[Sequence[str]]]] = None,
                        departments: Optional[Sequence[Optional[Sequence[str]]]] = None,
                        diversity: float | None = None, candidates: int | None = None, boosts=None,
                        boost_weight: float | None = None, only_boosted: bool = False, probes: int | None = None,
                        within=None, max_per_aisle: int | None = None,
                        max_per_department: int | None = None, history=None, cf_weight: float = 1.0,
                        rrf_c: float = 60.0, like=None, unlike=None, query_weight: float = 1.0,
                        like_weight: float = 1.0, unlike_weight: float = 0.5) -> list[list[tuple[str, float]]]:
        """Many contexts in one GPU pass; element i equals recommend(queries[i], ...).  aisles / departments: per
        query None or the admitted names, as recommend takes them.  diversity / candidates: one value for the whole
        batch, as recommend takes them.  boosts: None or one entry per query, each as recommend takes it; boost_weight
        and only_boosted: one value for the whole batch.  probes: one value for the whole batch, as recommend takes it.
        within: None or one entry per query, each None or as recommend takes it.  max_per_aisle / max_per_department: one
        value for the whole batch, as recommend takes them.  history: None or one entry per query, each None or as
        recommend takes it (in a batch that fuses, a None entry counts as []); cf_weight and rrf_c: one value for the
        whole batch.  like / unlike: None or one entry per query, each None or as recommend takes it; query_weight,
        like_weight and unlike_weight: one value for the whole batch."""
        plan = self._plan(len(queries), top_k, aisles=aisles, departments=departments, diversity=diversity,
                          candidates=candidates, boosts=boosts, boost_weight=boost_weight, only_boosted=only_boosted,
                          probes=probes, within=within, max_per_aisle=max_per_aisle, max_per_department=max_per_department,
                          history=history, cf_weight=cf_weight, rrf_c=rrf_c, like=like, unlike=unlike,
                          query_weight=query_weight, like_weight=like_weight, unlike_weight=unlike_weight)
        if not queries:
            return []
        k = self._k(top_k)
        ex = self._exclusion_rows(exclude_product_ids)
        idx, sc = self._encode_search(*self.model.tokenizer.packed(list(queries)), k, ex, plan)
        return [self._to_results(idx[i], sc[i]) for i in range(len(queries))]

    def recommend_batches(self, batches, top_k: int = 10, exclude_product_ids=None):
        """Generator over a stream of query batches: element j equals recommend_batch(batches[j], top_k,
        exclude_product_ids[j]).  Batch j+1 is tokenised on a worker thread while the GPU works on batch j and
        batch j is read back after batch j+1 has been launched (pipeline.py)."""
        from .pipeline import pipelined_search

        k = self._k(top_k)

        def exclude(j):
            return self._exclusion_rows(exclude_product_ids[j]) if exclude_product_ids is not None else None

        search = self._index.search
        if self._adapter is not None:
            adapter = self._adapter

            def search(emb, k, excl):
                return self._index.search(adapter.apply(emb), k, excl)

        for idx, sc in pipelined_search(self.model.tokenizer, self.model.encoder, search, batches, k, exclude):
            yield [self._to_results(idx[i], sc[i]) for i in range(idx.shape[0])]

    def recommend_batch_timed(self, queries: Sequence[str], top_k: int = 10, exclude_product_ids=None, *, aisles=None,
                              departments=None, diversity: float | None = None, candidates: int | None = None,
                              boosts=None, boost_weight: float | None = None, only_boosted: bool = False, within=None,
                              max_per_aisle: int | None = None, max_per_department: int | None = None, history=None,
                              cf_weight: float = 1.0, rrf_c: float = 60.0, like=None, unlike=None,
                              query_weight: float = 1.0, like_weight: float = 1.0, unlike_weight: float = 0.5):
        """recommend_batch plus (embedding ms incl. host tokenisation, similarity ms) from HIP events
        on the launch stream — what the micro-batching server reports as per-request stats.  A diversified batch's
        re-selection, a boosted batch's merge, a capped batch's rounds and a fused batch's CF ranking and fusion count into
        the similarity time."""
        k = self._k(top_k)
        plan = self._plan(len(queries), top_k, aisles=aisles, departments=departments, diversity=diversity,
                          candidates=candidates, boosts=boosts, boost_weight=boost_weight, only_boosted=only_boosted,
                          within=within, max_per_aisle=max_per_aisle, max_per_department=max_per_department,
                          history=history, cf_weight=cf_weight, rrf_c=rrf_c, like=like, unlike=unlike,
                          query_weight=query_weight, like_weight=like_weight, unlike_weight=unlike_weight)
        ex = self._exclusion_rows(exclude_product_ids)
        t0 = time.time()
        ids, cu = self.model.tokenizer.packed(list(queries))
        tok_ms = (time.time() - t0) * 1000
        idx, sc, enc_ms, sim_ms = self._encode_search(ids, cu, k, ex, plan, timed=True)
        return [self._to_results(idx[i], sc[i]) for i in range(len(queries))], tok_ms + enc_ms, sim_ms

    def recommend(self, query: str, top_k: int = 10,
                  exclude_product_ids: set[str] | None = None, *, aisles: Optional[Sequence[str]] = None,
                  departments: Optional[Sequence[str]] = None, diversity: float | None = None,
                  candidates: int | None = None, boosts=None, boost_weight: float | None = None,
                  only_boosted: bool = False, probes: int | None = None, within=None, max_per_aisle: int | None = None,
                  max_per_department: int | None = None, history=None, cf_weight: float = 1.0,
                  rrf_c: float = 60.0, like=None, unlike=None, query_weight: float = 1.0, like_weight: float = 1.0,
                  unlike_weight: float = 0.5) -> list[tuple[str, float]]:
        """Top-k (product_id, score) by cosine similarity, best first (reference :206-225).
        One query = one hipGraph replay (fastpath.py) when ICREC_USE_GRAPH is not "0".
        aisles / departments (keyword-only; names from .aisles / .departments): only products of one of these aisles
        AND one of these departments - the result of excluding every other product.  None leaves a facet open, []
        admits nothing; a name the catalog does not have raises ValueError.  Such a request takes the un-captured
        path.
        diversity in (0, 1] (keyword-only): the top_k are re-selected on the GPU from the `candidates` best matches
        (default min(128, 4 * top_k), at most the catalog) by Maximal Marginal Relevance with lambda = 1 - diversity
        (DeviceIndex.mmr_select): the best match first, then at each step the product with the best trade of cosine
        score against similarity to the products already chosen.  The returned scores are still the cosine scores of
        the chosen products, in SELECTION order - that order is not score-descending.  It composes with
        exclude_product_ids, aisles and departments (they shape the candidates) and takes the un-captured path.
        diversity None or 0 is the plain request: the same launches, the same results.  diversity outside [0, 1] or
        candidates outside [top_k, 128] raises ValueError.
        boosts (keyword-only; "buy it again"): the products this user has bought before, a mapping product id -> weight
        or an iterable of ids that all take boost_weight.  The result is the top_k of the WHOLE catalog under
        cosine + weight for these products and plain cosine for the rest, exactly (DeviceIndex.search_boosted): a
        boosted product is found wherever it ranked before, and the returned scores are the adjusted ones.  Weights
        are numbers >= 0 (at most 1,024 products); ids the catalog does not have are skipped, and an id that is also
        excluded stays excluded.  only_boosted=True ranks the boosted products alone, best first (weight 0: the
        user's history by the model's score).  It composes with exclude_product_ids, aisles and departments; with
        diversity the boosted ranking is `candidates` wide and MMR re-selects from it, with the adjusted scores as the
        relevance.  Such a request takes the un-captured path; boosts None or empty without only_boosted is the plain
        request: the same launches, the same results.  Bad arguments raise ValueError before any GPU work.
        probes (keyword-only; a recommender built with ann_lists): search only the `probes` lists of the IVF index whose
        centroids match the query best (IvfIndex.search): the exact top_k of those lists, approximate only in which
        products it looks at; probes = ann_lists is the exact search's result.  It composes with exclude_product_ids
        and with diversity (the IVF search is then `candidates` wide) and takes the un-captured path; together with
        aisles, departments or boosts, or without ann_lists, it raises ValueError.  probes None is the plain request.
        within (keyword-only; a recommender built with product_sets): a product set's name, or up to four names: only
        products that are in EVERY named set ("sold at this store" and "in stock") - the result of excluding every
        other product (DeviceIndex.search(sets=)).  It composes with exclude_product_ids, aisles, departments and
        diversity through the search, and with boosts / only_boosted: boosted products outside the sets are dropped, and
        the result is the top_k of the products inside them under cosine + weight.  Such a request takes the
        un-captured path.  An unknown name, a fifth name, within on a recommender without product sets or together
        with probes raise ValueError before any GPU work.
        max_per_aisle / max_per_department (keyword-only; positive integers): at most that many products of one aisle /
        of one department in the result.  The result is the walk of the COMPLETE ranking of the admissible products,
        best first, that keeps a product only while its aisle and its department have room - exactly, however deep
        in the ranking the last product lies (DeviceIndex.search_capped: `candidates` products per search, default
        min(128, 4 * top_k); a request whose candidates are used up before top_k products are kept is searched
        again without the aisles and departments that are full).  The order and the scores are the search's own.  It
        composes with exclude_product_ids, aisles, departments and within, and with boosts / only_boosted: the ranking
        that is walked is then the boosted one.  With diversity the caps thin the `candidates`-wide list in one round
        and the re-selection picks from what is left, so the result keeps the caps.  Such a request takes the
        un-captured path; both None is the plain request: the same launches, the same results.  A value that is not an
        integer >= 1, caps on a catalog without facets or together with probes raise ValueError before any GPU work.
        history (keyword-only; a recommender built with cf=): the products of the user's earlier orders, an iterable
        of product ids.  The content search and the item-item CF ranking of the history (icrec_cf_rank) both run
        `candidates` wide (default min(128, 4 * top_k), clipped to the catalog) and are fused by POSITION on the GPU
        (reciprocal rank fusion, icrec_fuse_select): a product's fused score is 1 / (rrf_c + its content position + 1)
        + cf_weight / (rrf_c + its CF position + 1), positions counted from 0 and a list that does not hold the
        product adding 0.  The returned scores are these fused scores, not cosines.  A CF candidate that co-occurs with
        nothing in the history does not vote.  CF never lists a product of the history itself (the reference's rule),
        the content list may: pass them as exclude_product_ids to drop them.  history=None is the plain request: the
        same launches, the same results.  history=[], or ids the CF baskets do not know, takes the fused path with a
        dead CF list: the content order, with fused scores.  It composes with exclude_product_ids and candidates only:
        together with aisles, departments, within, boosts / only_boosted, diversity, probes, max_per_aisle or
        max_per_department it raises ValueError before any GPU work (a CF list is the best of the whole catalog and
        knows none of these constraints), as do history on a recommender without cf, cf_weight not a number >= 0 and
        rrf_c not finite or <= -1.  Such a request takes the un-captured path.
        like / unlike (keyword-only; "more like these, less like those", Rocchio feedback): products the user accepted
        and products the user dismissed, each an iterable of product ids or a mapping product id -> weight >= 0.  The
        query vector is built on the GPU from the catalog's own stored rows, between the encode and the search
        (DeviceIndex.compose_queries): query_weight * the normalised text vector + the sum of weight * row over like,
        in the given order, - the same over unlike.  An iterable of n known ids gives each like_weight / n (unlike:
        unlike_weight / n) - the centroids of Rocchio's formula; a mapping gives the weights as written.  Defaults:
        query_weight 1, like_weight 1, unlike_weight 0.5.  The scores are the cosines of the products with the moved
        vector.  Only the query changes, so it composes with EVERY other option, probes, history (the content list
        of the fusion is searched with the moved vector) and only_boosted included.  Liked products are NOT removed
        from the result - a reorder is a good recommendation here; pass them as exclude_product_ids to drop them.
        Ids the catalog does not have are skipped; like and unlike both None, or without a known id, is the plain
        request: the same launches, the same results.  A string, a weight that is not a finite number >= 0, an id in
        both, an id twice in one list or more than 1,024 known ids raise ValueError before any GPU work.  Such a
        request takes the un-captured path."""
        return self._recommend_one(query, top_k, exclude_product_ids, aisles=aisles, departments=departments,
                                   diversity=diversity, candidates=candidates, boosts=boosts, boost_weight=boost_weight,
                                   only_boosted=only_boosted, probes=probes, within=within, max_per_aisle=max_per_aisle,
                                   max_per_department=max_per_department, history=history, cf_weight=cf_weight,
                                   rrf_c=rrf_c, like=like, unlike=unlike, query_weight=query_weight,
                                   like_weight=like_weight, unlike_weight=unlike_weight)

    def recommend_from_products(self, products, top_k: int = 10, exclude_product_ids: set[str] | None = None,
                                **options) -> list[tuple[str, float]]:
        """Top-k (product_id, score) for a query made of catalog products alone - a basket's or a user's profile: the
        weighted sum of the products' stored rows, built on the GPU (DeviceIndex.compose_queries without a base).  No
        text, no encoder launch.  products takes the forms of recommend's `like`: an iterable of ids (its n known ids
        weigh like_weight / n each, like_weight an option, default 1) or a mapping id -> weight >= 0.  options: recommend's
        other keywords (aisles, within, boosts, diversity, probes, ...; not like / unlike / query_weight).  The
        products themselves are not removed from the result: pass them as exclude_product_ids to drop them.  No known
        id returns []; bad arguments raise ValueError before any GPU work."""
        for name in ("like", "unlike", "query_weight", "unlike_weight"):
            if name in options:
                raise ValueError(f"recommend_from_products takes no {name}: the products are the whole query")
        terms = compose_terms(products, None, options.pop("like_weight", 1.0), 0.0, self._pid_to_row)
        k = self._k(top_k)
        for name in ("aisles", "departments", "within", "boosts", "history"):  # the per-query options, in the batch's form
            if options.get(name) is not None:
                options[name] = [options[name]]
        plan = replace(self._plan(1, top_k, **options), compose=[(0.0, terms)])
        if terms is None:
            return []
        idx, sc = self._encode_search(None, None, k, self._exclusion_rows([exclude_product_ids]), plan)
        return self._to_results(idx[0], sc[0])

    def similar_products(self, product_id, top_k: int = 10, exclude_self: bool = True, **options) -> list[tuple[str, float]]:
        """"Similar items" on a product page: the top-k by cosine similarity with the product's own stored row -
        recommend_from_products({product_id: 1.0}) with the product itself excluded (exclude_self=False keeps it: it
        then comes first, with a score of 1 up to the rounding of its row's norm).  options: recommend_from_products',
        exclude_product_ids included.  KeyError: an id the catalog does not have."""
        if product_id not in self._pid_to_row:
            raise KeyError(product_id)
        exclude = set(options.pop("exclude_product_ids", None) or ())
        if exclude_self:
            exclude.add(product_id)
        return self.recommend_from_products({product_id: 1.0}, top_k, exclude or None, **options)

    def _fast_path(self):
        """The hipGraph single-request path, rebuilt when the index or the model was replaced under it (a captured
        graph bakes the index / encoder handles), or None under ICREC_USE_GRAPH=0."""
        if self._fast is not None and (self._fast.index is not self._index or self._fast.encoder is not self.model.encoder):
            self._fast = type(self._fast)(self.model.encoder, self._index, self._adapter)
        return self._fast


class MonitoredRecommender(Recommender):
    """Recommender with timing; sets last_metrics after each recommend() (reference :228-293).
    Device time comes from HIP events on the launch stream, host tokenisation is added to the
    embedding time (it is part of model.encode in the reference)."""

    def __init__(self, *args, metrics_logger: Optional[logging.Logger] = None, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.metrics_logger = metrics_logger or logging.getLogger("recommender.metrics")
        self.last_metrics: Optional[RecommendationMetrics] = None

    def recommend(self, query: str, top_k: int = 10, user_id: Optional[str] = None,
                  exclude_product_ids: set[str] | None = None, *, aisles: Optional[Sequence[str]] = None,
                  departments: Optional[Sequence[str]] = None, diversity: float | None = None,
                  candidates: int | None = None, boosts=None, boost_weight: float | None = None,
                  only_boosted: bool = False, probes: int | None = None, within=None, max_per_aisle: int | None = None,
                  max_per_department: int | None = None, history=None, cf_weight: float = 1.0,
                  rrf_c: float = 60.0, like=None, unlike=None, query_weight: float = 1.0, like_weight: float = 1.0,
                  unlike_weight: float = 0.5) -> list[tuple[str, float]]:
        """On the graph path the request replays cut at the encode / search seam, with HIP events around the two
        replays (fastpath.py): the three timing fields keep their meaning there.  A diversified request's
        re-selection and a boosted request's merge count into the similarity time."""
        start = time.time()
        results, encode_ms, sim_ms = self._recommend_one(query, top_k, exclude_product_ids, timed=True, aisles=aisles,
                                                         departments=departments, diversity=diversity,
                                                         candidates=candidates, boosts=boosts, boost_weight=boost_weight,
                                                         only_boosted=only_boosted, probes=probes, within=within,
                                                         max_per_aisle=max_per_aisle,
                                                         max_per_department=max_per_department, history=history,
                                                         cf_weight=cf_weight, rrf_c=rrf_c, like=like, unlike=unlike,
                                                         query_weight=query_weight, like_weight=like_weight,
                                                         unlike_weight=unlike_weight)
        self.note_served(results, user_id, encode_ms, sim_ms, (time.time() - start) * 1000)
        return results

    def note_served(self, results: list[tuple[str, float]], user_id: Optional[str], encode_ms: float, sim_ms: float,
                    total_ms: float) -> RecommendationMetrics:
        """Fill last_metrics and emit the `recommendation_served` record for ONE served request (reference
        :268-278).  recommend() calls it per request; the micro-batching server calls it once per request of a
        batch with the batch's timings (api/batcher.py)."""
        n = len(results)
        m = self.last_metrics = RecommendationMetrics(
            user_id=user_id or "anonymous", query_embedding_time_ms=encode_ms, similarity_compute_time_ms=sim_ms,
            total_latency_ms=total_ms, num_recommendations=n, top_score=results[0][1] if results else 0.0,
            avg_score=sum(s for _, s in results) / n if n else 0.0, timestamp=time.time())
        if self.metrics_logger.isEnabledFor(logging.INFO):
            self._log_metrics(m)
        return m

    def _log_metrics(self, m: RecommendationMetrics) -> None:
        self.metrics_logger.info("recommendation_served", extra={
            "user_id": m.user_id, "latency_ms": m.total_latency_ms, "encode_time_ms": m.query_embedding_time_ms,
            "similarity_time_ms": m.similarity_compute_time_ms, "num_results": m.num_recommendations,
            "top_score": m.top_score, "avg_score": m.avg_score})
