"""The seeded cases of the feature sweep (tools/fuzz_features.py, tests/test_feature_cases.py,
tests/test_feature_sweep_gpu.py): cases(seed, count) yields fully specified search requests - catalog, edit script,
request kind, request features, Q and k - each reproducible from (seed, index) alone.  Case `index` has kind
KINDS[index % 10]; its j-th case (j = index // 10) aims at one kernel form, row type and arm in turn, so that a few
dozen cases per kind reach every cell of the table tests/test_feature_cases.py states; everything else is drawn.
A feature is drawn so that it binds: exclusions and boost lists partly from the reference's own ranking of the query,
masks and sets so that between a few rows and most rows are admitted.  Needs no GPU."""
from __future__ import annotations

import itertools

import numpy as np

from instacart_next_order_recommendation_amd.search import rowset_ids
from tests import feature_reference as ref
from tests import ivf_reference
from tests.index_model import Model
from tests.rowset_cases import admitted_by_sets, resident_lds_sets
from tests.search_harness import FILTER_MIN_Q, LDS_MAX, filter_list_len, resident_lds, search_plan, select_from_scores

KINDS = ["plain", "faceted", "in-sets", "in-sets+faceted", "boosted", "boosted-only", "capped", "capped+boosted",
         "diverse", "ivf"]
WIDTHS = [32, 64, 96, 128, 256, 384, 416, 512, 768, 1024, 4096]                     # tools/fuzz_search.py's
QS = [1, 2, 3, 5, 8, 9, 31, 33, 64, 65, 100, 129, 256, 300, 513] + [255, 256, 257]
KS = [1, 2, 5, 10, 20, 32, 33, 64, 100, 116, 117, 128] + [76, 77, 84, 85, 92, 93]   # + the resident filter's LDS limits
NS = [1, 7, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000, 4097, 20000]
SCALES = [1e-3, 1.0, 50.0]
STREAM_N = 6 * 256 * 256 + 1          # the streaming kernel takes 3 .. 8 queries from 6 tiles of 256 rows per CU on
SIZE_LIMIT = 4_000_000 * 384          # nq * n * dim, tools/fuzz_search.py's
WORK = 200_000_000                    # this generator's own, lower bound on nq * n * dim: the CPU reference stays quick
WALK = 100_000                        # and on nq * n where the reference walks rankings in Python (caps)
MMR_WORK = 400_000_000                # and on nq * k * k * dim where it computes a similarity matrix per query (MMR)
ARMS = ["plain", "FACET", "SETS"]
FORMS = ["stream1", "stream2", "stream48", "small", "mid", "big", "staged", "resident", "declined"]
ROW_TYPES = ["f32", "bf16"]
CELLS = list(itertools.product(ARMS, FORMS, ROW_TYPES))
FIXED_ARM = {"plain": "plain", "faceted": "FACET", "in-sets": "SETS", "in-sets+faceted": "SETS"}
FREE_KINDS = ["boosted", "capped", "capped+boosted", "diverse"]
FREE_OFFSET = {"boosted": 0, "capped": 37, "capped+boosted": 27, "diverse": 10}   # each walks CELLS in steps of 7 from here:
#                                                       20 cases per kind reach all 54 cells (7 * 31 = 1 mod 54)
FACET0 = [0, 1, 5, 31, 32, 33, 63, 64, 100, 127, 128, 200, 254, 255]                # values on the mask words' edges
FACET1 = [0, 3, 7, 20, 31, 32, 255]
ASSIGN_PASS_BYTES = 64 << 20          # csrc/ivf.hip's ASSIGN_SLICE_BYTES: rows of one assignment pass = this / (4 dim)


def kernel_form(arm, n, Q, k, dim, storage, n_cu=256):
    """The kernel a search of this shape takes (csrc/search.hip's make_filter_plan and make_plan), one of FORMS."""
    kp = filter_list_len(k)
    if storage.endswith("filter") and Q >= FILTER_MIN_Q and kp <= 128:
        if dim != 384:
            return "staged"
        lds = resident_lds_sets(kp) if arm == "SETS" else resident_lds(kp, arm == "FACET")
        return "resident" if lds <= LDS_MAX else "declined"
    plan = search_plan(n, Q, k, n_cu)
    return {1: "stream1", 2: "stream2"}.get(plan[2], "stream48") if plan[0] == "stream" else plan[0]


class Case:
    """One case; see cases().  model: the catalog after the edit script (tests.index_model.Model); scores: the
    reference's complete score matrix of q over it."""

    def arm(self):
        return "SETS" if self.set_ids is not None else "FACET" if self.allow is not None else "plain"

    def form(self, n_cu=256):
        """The form of the request's (first) search; None for the kinds that run none through DeviceIndex.search."""
        if self.kind in ("boosted-only", "ivf"):
            return None
        return kernel_form(self.arm(), self.model.n, self.q.shape[0], self.search_k(), self.dim, self.storage, n_cu)

    def search_k(self):
        """The k of the request's first search."""
        if self.kind in ("capped", "capped+boosted"):
            k = min(128, 4 * self.k) if self.candidates is None else self.candidates
            return max(min(k, self.model.n), min(self.k, self.model.n))
        return self.k

    def tie_rows(self):
        """The most rows of one score that a query finds at the head of its ranking of the rows it may return: those
        its masks and sets admit and its exclusions do not name.  A query that may return no row has no head."""
        nq, n = self.scores.shape
        ok = ref.admission(self.model.F, self.model.M, nq, self.allow, self.set_ids)
        ok = np.ones((nq, n), bool) if ok is None else ok.copy()
        if self.excl is not None:
            for i, e in enumerate(self.excl):
                ok[i, [r for r in e if 0 <= r < n]] = False
        best = 0
        for i in np.flatnonzero(ok.any(axis=1)):
            s = self.scores[i, ok[i]]
            best = max(best, int((s == s.max()).sum()))
        return best

    def describe(self):
        feats = ",".join(ref.active_features(self)) or "-"
        extra = ""
        if self.kind == "ivf":
            extra = f" n_lists={self.C.shape[0]} nprobe={self.nprobe}"
        if self.kind == "diverse":
            extra = f" top_k={self.top_k} lam={self.lam}"
        if self.kind in ("capped", "capped+boosted"):
            extra = f" candidates={self.candidates}"
        return (f"seed={self.seed} --case {self.index} kind={self.kind} storage={self.storage} dim={self.dim} n0={self.n0} "
                f"n={self.model.n} nq={self.q.shape[0]} k={self.k} off={self.row_offset} scale={self.scale} "
                f"features={feats} script={[op[0] for op in self.script]}{extra}")


def _target(kind, j):
    """(arm or None, form, row type) the j-th case of a kind aims at."""
    if kind in FIXED_ARM:
        shift = 9 if kind == "in-sets+faceted" else 0
        form, rt = list(itertools.product(FORMS, ROW_TYPES))[(j + shift) % 18]
        if kind == "in-sets+faceted" and (form, rt) == ("stream48", "f32"):
            form = "stream2"              # in-sets and a free kind reach the SETS arm's large fp32 catalog twice already
        return FIXED_ARM[kind], form, rt
    if kind in STREAM48_AT and j in STREAM48_AT[kind]:
        return STREAM48_AT[kind][j]
    arm, form, rt = CELLS[(7 * j + FREE_OFFSET[kind]) % len(CELLS)]
    return arm, "stream2" if form == "stream48" and kind in ("capped", "capped+boosted") else form, rt


def _shape(rng, form, rt, arm, tiny):
    """(storage, dim, nq, k, n) drawn for a kernel form."""
    if tiny:
        return rt, int(rng.choice([32, 64] if rt == "f32" else [64])), int(rng.choice([1, 2, 3, 5])), \
            int(rng.choice([1, 2, 5, 10])), int(rng.integers(2, 33))
    k = int(rng.choice(KS))
    n = int(rng.choice(NS))
    storage = rt
    wide = WIDTHS if rt == "f32" else [d for d in WIDTHS if d % 64 == 0]
    dim = int(rng.choice(wide))
    if form in ("stream1", "stream2"):
        nq = 1 if form == "stream1" else 2
    elif form == "stream48":
        nq, n, dim = int(rng.choice([3, 4, 5, 8])), STREAM_N, 32 if rt == "f32" else 64     # the narrowest rows: 50 MB
    elif form in ("small", "mid", "big"):
        if form == "big":
            nq, k = int(rng.choice([q for q in QS if q > 64])), int(rng.choice([v for v in KS if v <= 32]))
        elif form == "mid":
            nq = int(rng.choice([q for q in QS if q > 32]))
            k = int(rng.choice([v for v in KS if (32 < v <= 64) or (nq <= 64 and v <= 64)]))
        else:
            nq = int(rng.choice([q for q in QS if q > 2]))
            if nq > 32:
                k = int(rng.choice([v for v in KS if v > 64]))
    else:
        storage = rt + "+filter"
        nq = int(rng.choice([q for q in QS if q >= 256]))
        dim = 384 if form != "staged" else int(rng.choice([d for d in WIDTHS if d % 64 == 0 and d != 384]))
        limit = {"plain": 92, "FACET": 84, "SETS": 76}[arm]
        k = int(rng.choice([v for v in KS if v <= 116 and (form == "staged" or (v <= limit) == (form == "resident"))]))
    if form in ("small", "mid", "big") and rng.random() < 0.4 and dim % 64 == 0 and (nq < FILTER_MIN_Q or k > 116):
        storage = rt + "+filter"      # a filter storage below the filter's query count, or past its list length
    return storage, dim, nq, k, n


def _edge_ids(rng, n, m):
    """m distinct rows of [0, n): the tile, word and round edges first, random ones after."""
    edges = [r for r in (0, 31, 32, 127, 128, 255, 256, n - 33, n - 32, n - 1) if 0 <= r < n]
    pick = rng.permutation(edges).tolist()[:max(1, m // 2)] + rng.choice(n, min(n, m), replace=False).tolist()
    pick = list(dict.fromkeys(pick))
    return np.asarray(pick[:m], np.int64)


def _rows(rng, m, dim, scale):
    """m random rows.  Beyond a few million components they are random bytes, signed and scaled to unit variance:
    the generator's normals would take longer than the search of the catalog they fill."""
    if m * dim > 4_000_000:
        return np.frombuffer(rng.bytes(m * dim), np.int8).astype(np.float32).reshape(m, dim) * np.float32(scale / 74.0)
    return rng.standard_normal((m, dim), dtype=np.float32) * np.float32(scale)


def _facets(rng, m):
    return np.stack([rng.choice(FACET0, m), rng.choice(FACET1, m)], axis=1).astype(np.uint8)


def _membership(rng, n):
    return np.stack([rng.random(n) < 0.5, rng.random(n) < 0.05, rng.random(n) < 0.9])


def _script(rng, model, scale, may_remove, centre=None, tiny=False):
    """A short edit script, drawn against a model that it edits as it goes: [(op, args...)], the arguments as the
    DeviceIndex methods of the same names take them (write_rowset: a bool membership row; reserve: the capacity)."""
    script = []
    for _ in range(int(rng.integers(1, 5))):
        n = model.n
        op = str(rng.choice(["write_rows", "write_facets", "write_rowset", "reserve", "append_rows", "remove_rows"]))
        if op == "write_rows":
            ids = _edge_ids(rng, n, int(rng.integers(1, min(n, 20) + 1)))
            E = _rows(rng, ids.size, model.dim, scale)
            if centre is not None:
                E = centre[rng.integers(0, centre.shape[0], ids.size)] + np.float32(0.05) * E
            if rng.random() < 0.3:
                E[0] = model.E[int(rng.integers(0, n))]                              # a copy of another row
            model.E[ids] = E
            script.append((op, ids, E))
        elif op == "write_facets":
            ids = _edge_ids(rng, n, int(rng.integers(1, min(n, 40) + 1)))
            F = _facets(rng, ids.size)
            model.F[ids] = F
            script.append((op, ids, F))
        elif op == "write_rowset":
            s = int(rng.integers(0, 3))
            row = model.M[s] ^ (rng.random(n) < 0.1)
            row[_edge_ids(rng, n, min(n, 4))] = True
            model.M[s] = row
            script.append((op, s, row.copy()))
        elif op == "reserve":
            script.append((op, n + int(rng.choice([0, 1, 31, 300]))))
        elif op == "append_rows":
            m = int(rng.choice([1, 2] if tiny else [1, 2, 31, 33, 64]))
            E, F = _rows(rng, m, model.dim, scale), _facets(rng, m)
            if centre is not None:
                E = centre[rng.integers(0, centre.shape[0], m)] + np.float32(0.05) * E
            model.edit_append(E, F)
            script.append((op, E, F))
        elif may_remove and n > 1:
            ids = _edge_ids(rng, n, int(rng.integers(1, min(n - 1, 40) + 1)))
            model.edit_remove(ids)
            script.append((op, ids))
    return script


# The 393,217-row catalogs are the sweep's dearest cases: the kinds whose references walk them in Python leave them
# to these cases of the kinds whose references do not.
STREAM48_AT = {"boosted": {18: ("FACET", "stream48", "f32")}}
ALLOW_CYCLE = ["one", "several", "open", "zero", "both"]       # as test_index_resize_gpu's ALLOW_KINDS cycle
SET_CYCLE = [[0], [-1, 2], [0, 2], [2, 2, 0, -1], [1], [3], [-1, -1], [0, 1, 2, -1]]    # 3: an id the index lacks
CAP_CYCLE = [(1, 1), (0, 2), (2, 1), (0, 0), (1000, 1000), (3, 0)]


def _allow(rng, nq):
    start, out = int(rng.choice([1, 4])), []               # (the first query admits several values: it may be the only one)
    for i in range(nq):
        kind = ALLOW_CYCLE[(start + i) % 5]
        some0 = [v for v in FACET0 if rng.random() < 0.6] or [32]
        some1 = [v for v in FACET1 if rng.random() < 0.7] or [31]
        out.append({"one": ([int(rng.choice(FACET0))], None), "several": (some0, None) if i % 2 else (None, some1),
                    "open": None, "zero": ([], []), "both": (some0, some1)}[kind])
    return out


def _sets(rng, nq):
    start = int(rng.choice([0, 1, 2]))                        # (the first query is in a large set: it may be the only one)
    return rowset_ids([SET_CYCLE[(start + i) % len(SET_CYCLE)] for i in range(nq)], nq, 4)


def _exclusions(rng, n, nq, free_top, pool_top, lifted):
    """Per query: some of the unrestricted top-k, some of the request's own candidates, some random rows; every fourth
    query none, every fourth its best candidate and a row its boost list lifts by 1."""
    out = []
    for i in range(nq):
        if i % 4 == 3:
            out.append([])
            continue
        e = set(rng.choice(n, int(rng.integers(0, min(n, 30) + 1)), replace=False).tolist())
        for top in (free_top[i], pool_top[i]):
            real = top[top >= 0]
            if real.size:
                e |= set(rng.choice(real, int(rng.integers(1, min(real.size, 8) + 1)), replace=False).tolist())
        e = set(sorted(int(v) for v in e)[:max(1, min(60, n))])
        if i % 4 == 0:
            e |= set(int(v) for v in pool_top[i][:1] if v >= 0) | set(int(v) for v in lifted[i][:1])
        out.append(sorted(e))
    return out


def _boosts(rng, n, nq, k, free_rank, pool_rank, in_sets, odd_weights, admit):
    """Per query (rows ascending, weights): rows just outside the unrestricted and the request's own top-k, and random
    ones - none outside the query's sets, as search_boosted requires; every fifth query no list."""
    weights = [0.0, 0.05, 0.5, 1.0, 1.0, np.inf] + ([np.nan, -0.25] if odd_weights else [])
    out = []
    for i in range(nq):
        rows = set()
        if i % 5 != 4:
            rows |= set(rng.choice(n, int(rng.integers(0, min(n, 12) + 1)), replace=False).tolist())
            for rank in (free_rank[i], pool_rank[i]):
                near = rank[k:][rank[k:] >= 0]
                rows |= set(near[:int(rng.integers(1, 9))].tolist())
                rows |= set(rank[:k][rank[:k] >= 0][:int(rng.integers(0, 3))].tolist())
        r = np.asarray(sorted(v for v in rows if in_sets is None or in_sets[i, v]), np.int64)
        w = np.asarray(rng.choice(weights, r.size), np.float32)
        if r.size:
            w[int(rng.integers(0, r.size))] = np.float32(1.0)
            out_of_reach = np.flatnonzero(~admit[i, r]) if admit is not None else []
            if len(out_of_reach):     # a lifted row that the masks reject: first without them
                w[int(rng.choice(out_of_reach))] = np.float32(1.0)
        out.append((r, w))
    return out


def _catalog(rng, n, dim, scale, tie_len, identical=False):
    P = _rows(rng, n, dim, scale)
    dup = None
    if tie_len and n > tie_len + 8:   # blocks of identical and near-identical rows
        dup = rng.choice(n, tie_len, replace=False)
        P[dup] = P[dup[0]] + (0 if identical or rng.random() < 0.7 else 1e-6) * rng.standard_normal((tie_len, dim)).astype(np.float32)
    if rng.random() < 0.1:
        P[rng.integers(0, n)] = 0.0   # a zero row (normalised with the eps clamp)
    return P, dup


def _ivf_catalog(rng, j, tiny):
    """(storage, dim, n, nq, k, C, P, nprobe, may_remove, stray) of the ivf kind's j-th case, by class: j % 20 = 1 and 6
    more rows than one assignment pass at width 4,096 (f32, bf16), j % 5 = 2 a list of 5 tiles of 256 rows probed at S = 4 on 256 CUs
    (64 .. 85 queries of 2 probes, 128 .. 170 of 1), the others drawn shapes."""
    cls = "passes" if j % 20 in (1, 6) else "tiles" if j % 5 == 2 else "drawn"
    storage = ["f32", "bf16", "f32+filter"][(j // 2) % 3]
    k = int(rng.choice(KS))
    if tiny:
        dim, n_lists, nq, k = 64, int(rng.integers(1, 5)), int(rng.choice([1, 3, 5])), int(rng.choice([1, 5, 10]))
        counts = rng.multinomial(int(rng.integers(8, 33)), np.ones(n_lists) / n_lists)
        nprobe = int(rng.integers(1, n_lists + 1))
    elif cls == "passes":
        storage, dim, n_lists = ("f32" if j % 20 == 1 else "bf16"), 4096, 8
        counts = rng.multinomial(int(rng.choice([4097, 4200, 4264])), np.ones(8) / 8)       # under 70 MB of fp32 rows
        nq, nprobe = int(rng.choice([1, 5, 9, 33])), int(rng.choice([1, 2, 3]))
    elif cls == "tiles":
        dim, n_lists = 64, 4
        counts = np.asarray([int(rng.integers(1080, 1230)), 300, 40, 700])
        nq, nprobe = [(64, 2), (129, 1), (65, 2), (128, 1), (85, 2), (170, 1)][int(rng.integers(0, 6))]
    else:
        dim = int(rng.choice([d for d in WIDTHS if d % 64 == 0 and d <= 1024]))
        n_lists = int(rng.choice([1, 2, 3, 8, 16]))
        n = max(n_lists, int(rng.choice([n for n in NS if n > 1])))
        nq = int(rng.choice(QS))
        if nq * n * dim > WORK:
            n = max(n_lists, WORK // (nq * dim))
        counts = rng.multinomial(n - n_lists, rng.dirichlet(np.ones(n_lists))) + 1
        nprobe = min(n_lists, int(rng.choice([1, 2, 3, n_lists])))
    C = rng.standard_normal((n_lists, dim)).astype(np.float32)
    home = rng.permutation(np.repeat(np.arange(n_lists), counts))
    noise = 0.05 if cls == "tiles" else float(rng.choice([0.05, 0.3, 1.0]))
    P = C[home] + _rows(rng, home.size, dim, noise)
    stray = []
    if n_lists > nprobe:      # rows of list b that score above every row near a for a query between a, ... and b (make_case)
        for r in rng.choice(home.size, min(4, home.size), replace=False):
            lists = rng.choice(n_lists, nprobe + 1, replace=False)
            P[r] = C[lists[-1]] + np.float32(0.8) * C[lists[0]]
            stray.append(lists)
    return storage, dim, home.size, nq, k, C, P, nprobe, cls == "drawn" or tiny, stray


def make_case(seed, index, tiny=False):
    rng = np.random.default_rng([int(seed), int(index)])
    c = Case()
    c.seed, c.index, c.kind = int(seed), int(index), KINDS[index % len(KINDS)]
    j = index // len(KINDS)
    c.scale = float(rng.choice(SCALES))
    c.excl = c.allow = c.set_ids = c.boosts = c.caps = c.candidates = c.C = c.assignment = None
    c.lam, c.top_k, c.nprobe, c.target = 1.0, None, None, None
    tie_len, centre, may_remove, stray, forced = 0, None, True, [], False
    # ---- catalog
    if c.kind == "ivf":
        c.storage, c.dim, n, nq, c.k, c.C, P, c.nprobe, may_remove, stray = _ivf_catalog(rng, j, tiny)
        P *= np.float32(c.scale)
        centre = c.C * np.float32(c.scale)
    else:
        if c.kind == "boosted-only":
            arm, form = str(rng.choice(["plain", "FACET"])), str(rng.choice(["small", "mid", "big", "stream1"]))
            rt = ROW_TYPES[j % 2]
        else:
            arm, form, rt = _target(c.kind, j)
        c.target = (arm, form, rt)
        c.storage, c.dim, nq, c.k, n = _shape(rng, form, rt, arm, tiny)
        if c.kind == "boosted-only" and not tiny:
            c.storage = ["f32", "bf16", "f32+filter", "bf16+filter"][j % 4]
            if c.dim % 64:
                c.dim = 64
        if c.kind in ("capped", "capped+boosted", "diverse") and c.k < 5 and not tiny:
            c.k = max(c.k, int(rng.choice([v for v in KS if kernel_form(arm, n, nq, v, c.dim, c.storage) == form] or [c.k])))
        if c.kind in ("diverse", "capped", "capped+boosted") and nq > 256:
            nq = 256                  # the references' MMR loop and capped walk are Python loops per query
        if c.kind == "diverse" and c.dim != 384 and nq * c.k * c.k * c.dim > MMR_WORK:
            fit = [d for d in WIDTHS if d % 64 == 0 and d != 384 and nq * c.k * c.k * d <= MMR_WORK]
            c.dim = int(rng.choice(fit or [64]))          # k x k similarities per query at this width
        walk = c.kind in ("capped", "capped+boosted")
        if walk and n < 31 and not tiny:
            n = int(rng.choice([v for v in NS if v >= 31]))   # a cap binds only where several rows share a facet value
        if form != "stream48":
            if nq * n * c.dim > WORK:
                n = max(1, WORK // (nq * c.dim))
            if walk and nq * n > WALK:
                n = max(1, WALK // nq)
        may_remove = form != "stream48"
        forced = form in ("staged", "resident") and arm != "plain" and not tiny
        if forced or (form in ("staged", "resident") and rng.random() < 0.7):
            tie_len = filter_list_len(c.k) + int(rng.integers(40, 140))   # longer than a filter candidate list, also
            if forced:                                                    # without the rows a query excludes
                n = max(n, tie_len + 50)
        elif n > 40 and rng.random() < 0.4:
            tie_len = min(n // 2, int(rng.integers(2, 300)))
        P, dup = _catalog(rng, n, c.dim, c.scale, tie_len, forced)
    c.n0 = n
    F, M = _facets(rng, n), _membership(rng, n)
    if c.kind != "ivf" and dup is not None and (forced or rng.random() < 0.8):
        F[dup], M[:, dup] = (32, 31), True        # a tie block that most masks and every set admit whole
    c.row_offset = int(rng.choice([0, 0, 12345, 4_000_000_000 - n - 1]))
    model = Model.of(rng, P, F, M)
    c.E0, c.F0, c.M0 = P, F, M
    c.script = _script(rng, model, c.scale, may_remove, centre, tiny or c.dim == 4096) if rng.random() < 0.5 else []
    c.model = model
    n = model.n
    # ---- queries
    q = rng.standard_normal((nq, c.dim)).astype(np.float32)
    if tie_len or rng.random() < 0.3:
        m = max(1, nq // 3)
        near = P[dup[0]] if c.kind != "ivf" and dup is not None else model.E[rng.integers(0, n, m)]   # (the block as built)
        q[:m] = near / np.float32(c.scale) + np.float32(0.02) * q[:m]
    if c.kind == "ivf" and rng.random() < 0.7:
        m = max(1, nq // 2)
        q[nq - m:] = c.C[rng.integers(0, min(2, c.C.shape[0]), m)] + np.float32(0.1) * q[nq - m:]
    for i, lists in enumerate(stray):     # the query a stray row was planted for: its best row lies in a list it does not probe
        q[(3 * i) % nq] = sum(np.float32(1 - 0.1 * t) * c.C[l] for t, l in enumerate(lists))
    if rng.random() < 0.1:
        q[0] = 0.0
    c.q = q
    c.scores = ref.catalog_scores(q, model.E, c.storage)
    # ---- request features
    has = {"masks": c.kind in ("faceted", "in-sets+faceted"), "sets": c.kind in ("in-sets", "in-sets+faceted")}
    if c.kind in FREE_KINDS:
        has["sets"] = c.target[0] == "SETS"
        has["masks"] = c.target[0] == "FACET" or (has["sets"] and rng.random() < 0.5)
    if c.kind == "boosted-only":
        has["masks"] = c.target[0] == "FACET"
    if has["masks"]:
        c.allow = _allow(rng, nq)
    if has["sets"]:
        c.set_ids = _sets(rng, nq)
    admit = ref.admission(model.F, model.M, nq, c.allow, c.set_ids)
    if c.kind == "ivf":
        c.C = np.ascontiguousarray(c.C[:min(c.C.shape[0], n)])
        c.nprobe = min(c.nprobe, c.C.shape[0])
        c.assignment = ivf_reference.assign(ivf_reference.stored_rows(model.E, ref.base_storage(c.storage)), c.C)
        pr = ivf_reference.probes(q, c.C, c.nprobe)
        admit = np.zeros(c.scores.shape, bool)
        for p in range(pr.shape[1]):
            admit |= c.assignment[None, :] == pr[:, p, None]
    wide = min(n, c.k + 32)
    free_rank = select_from_scores(c.scores, wide)[0]
    pool_rank = free_rank if admit is None else select_from_scores(c.scores, wide, admit=admit)[0]
    if c.kind in ("boosted", "boosted-only", "capped+boosted"):
        in_sets = None if c.set_ids is None else admitted_by_sets(model.M, c.set_ids)
        c.boosts = _boosts(rng, n, nq, c.k, free_rank, pool_rank, in_sets, c.kind != "capped+boosted" and j % 2 == 0, admit)
    if rng.random() < 0.6:
        lists = [np.concatenate([a[:c.k], r]) for a, (r, _) in zip(pool_rank, c.boosts)] if c.kind == "boosted-only" \
            else [a[:c.k] for a in pool_rank]
        lifted = [r[w == 1] for r, w in c.boosts] if c.boosts is not None else [[]] * nq
        c.excl = _exclusions(rng, n, nq, [a[:c.k] for a in free_rank], lists, lifted)
    if c.kind in ("capped", "capped+boosted"):
        start = int(rng.integers(0, len(CAP_CYCLE)))
        c.caps = np.asarray([CAP_CYCLE[(start * (i > 0) + i) % len(CAP_CYCLE)] for i in range(nq)], np.int64)
        # the drawn k is the width of the first search; top_k is a part of it
        width, c.k = c.k, max(min(c.k, 5), int(rng.choice([c.k, max(1, c.k // 2), max(1, c.k // 4)])))
        c.candidates = None if min(128, 4 * c.k) == width else width
        if n > 50_000:                # no cap that exhausts a large catalog: the walk would visit every row
            c.caps = np.where(c.caps > 0, np.maximum(c.caps, -(-c.k // 4)), 0)
    if c.kind == "diverse":
        c.lam = float(rng.choice([0.0, 0.3, 0.5, 1.0]))
        c.top_k = int(rng.choice([max(1, c.k // 2), c.k, min(c.k, 5)]))
    return c


def cases(seed, count, kind=None, tiny=False):
    """Cases 0 .. count - 1 of a seed (those of one kind where `kind` names it), one at a time: a case holds its
    catalog, so a list of them would not fit."""
    for index in range(count):
        if kind is None or KINDS[index % len(KINDS)] == kind:
            yield make_case(seed, index, tiny)


def cells_of(c, n_cu):
    """The cells of the coverage table a case hits on a device of n_cu CUs (tests/test_feature_cases.py states them)."""
    out = [("kind x storage", c.kind, c.storage)]
    form = c.form(n_cu)
    if form is not None:
        out.append(("arm x form x rows", c.arm(), form, ref.base_storage(c.storage)))
        if c.arm() != "plain" and (c.dim >= 768 or c.dim < 128):
            out.append(("arm x width", c.arm(), "768+" if c.dim >= 768 else "<128"))
        if c.arm() != "plain" and form in ("staged", "resident") and c.tie_rows() > filter_list_len(c.search_k()):
            out.append(("tie block under masks or sets",))
    if c.script:
        out.append(("kind x edited", c.kind))
    if c.row_offset > 2**31:
        out.append(("kind x offset > 2^31", c.kind))
    if c.kind == "ivf":
        if c.model.n > ASSIGN_PASS_BYTES // (4 * c.dim):
            out.append(("ivf: two assignment passes", ref.base_storage(c.storage)))
        S = ivf_reference.plan_slices(n_cu, c.q.shape[0], c.nprobe)
        sizes = np.bincount(c.assignment, minlength=c.C.shape[0])
        probed = np.unique(ivf_reference.probes(c.q, c.C, c.nprobe))
        tiles = -(-sizes[probed] // 256)
        if (tiles % np.maximum(-(-tiles // S), 1) != 0).any():
            out.append(("ivf: a short last slice", f"S={S}"))
        if S == 4 and (tiles == 5).any():
            out.append(("ivf: 5 tiles at S = 4",))
    return out


# The committed sweep: per kind, the count that `tools/fuzz_features.py COUNT SEED --kind K` runs (every tenth case).
SEED = 7
COUNTS = {kind: 200 for kind in KINDS}
