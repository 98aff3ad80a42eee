"""The feature sweep's case generator and composed reference, without a device: the committed (seed, counts) of
tests/feature_cases.py reach every cell of the coverage table at least twice (kernel forms predicted at 256 CUs), hold
the IVF classes, make every request feature bind, and stay inside tools/fuzz_search.py's size limit; the composed
reference (tests/feature_reference.py) agrees with a brute-force statement of every request kind on tiny catalogs."""
from __future__ import annotations

import collections
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle
from tests import feature_cases as fc
from tests import feature_reference as ref
from tests import ivf_reference

N_CU = 256
STORAGES = ["f32", "bf16", "f32+filter", "bf16+filter"]


@functools.lru_cache(maxsize=None)
def sweep():
    """One pass over the committed cases -> (cells hit, {(kind, feature): [cases that carry it, of which it binds in]},
    the largest nq * n * dim, notes on the IVF classes)."""
    hits = collections.Counter()
    binding = collections.defaultdict(lambda: [0, 0])
    largest, ivf_notes = 0, collections.Counter()
    for kind in fc.KINDS:
        for c in fc.cases(fc.SEED, fc.COUNTS[kind], kind):
            assert c.kind == kind and c.model.n >= 1
            hits.update(fc.cells_of(c, N_CU))
            largest = max(largest, c.q.shape[0] * max(c.n0, c.model.n) * c.dim)
            want = ref.expected(c)
            for feature in ref.active_features(c):
                other = ref.expected(c, off=feature)
                binding[kind, feature][0] += 1
                binding[kind, feature][1] += not (np.array_equal(want[0], other[0]) and np.array_equal(want[1], other[1]))
            if kind == "ivf":
                if c.dim == 4096 and c.model.n > 4096:
                    assert c.model.n * 4096 * 4 < 70_000_000
                    ivf_notes["two passes", ref.base_storage(c.storage)] += 1
                if c.row_offset == 4_000_000_000 - c.n0 - 1:
                    ivf_notes["offset"] += 1
    return hits, dict(binding), largest, ivf_notes


def test_a_case_is_its_seed_and_index():
    a, b = fc.make_case(fc.SEED, 23), fc.make_case(fc.SEED, 23)
    assert a.describe() == b.describe()
    np.testing.assert_array_equal(a.model.E, b.model.E)
    np.testing.assert_array_equal(a.q, b.q)
    assert [c.index for c in fc.cases(fc.SEED, 40, "capped")] == [6, 16, 26, 36]
    assert fc.make_case(fc.SEED, 24).describe() != a.describe()


def test_every_cell_is_hit_twice():
    hits = sweep()[0]
    cells = [("arm x form x rows",) + cell for cell in fc.CELLS]
    cells += [("kind x storage", kind, s) for kind in fc.KINDS for s in STORAGES if not (kind == "ivf" and s == "bf16+filter")]
    cells += [("arm x width", arm, w) for arm in ("FACET", "SETS") for w in ("768+", "<128")]
    cells += [(what, kind) for what in ("kind x edited", "kind x offset > 2^31") for kind in fc.KINDS]
    short = {cell: hits[cell] for cell in cells if hits[cell] < 2}
    assert not short, short
    assert hits[("tie block under masks or sets",)] >= 4


def test_ivf_classes():
    hits, _, _, notes = sweep()
    assert notes["two passes", "f32"] >= 1 and notes["two passes", "bf16"] >= 1
    assert hits[("ivf: two assignment passes", "f32")] + hits[("ivf: two assignment passes", "bf16")] >= 2
    assert hits[("ivf: 5 tiles at S = 4",)] >= 1 and hits[("ivf: a short last slice", "S=4")] >= 1
    assert notes["offset"] >= 1


def test_every_feature_binds():
    binding = sweep()[1]
    admits = {"exclusions": fc.KINDS, "masks": ["faceted", "in-sets+faceted"] + fc.FREE_KINDS + ["boosted-only"],
              "sets": ["in-sets", "in-sets+faceted"] + fc.FREE_KINDS, "boosts": ["boosted", "boosted-only", "capped+boosted"],
              "caps": ["capped", "capped+boosted"], "lambda": ["diverse"], "nprobe": ["ivf"]}
    for feature, kinds in admits.items():
        for kind in kinds:
            carried, bound = binding.get((kind, feature), (0, 0))
            assert carried >= 2, (kind, feature, carried)
            assert bound >= 0.8 * carried, (kind, feature, carried, bound)
    assert set(binding) == {(k, f) for f, kinds in admits.items() for k in kinds}


def test_no_case_exceeds_the_size_limit():
    assert sweep()[2] <= fc.SIZE_LIMIT


# ---------------------------------------------------------------- the composed reference against brute force
def brute_force(c):
    """Case c's expected result stated row by row in plain Python over the score matrix: admission bit by bit, the
    boost rule per listed row, one sort by (score descending, row ascending), the capped walk, the MMR loop."""
    m, nq, n = c.model, c.q.shape[0], c.model.n
    top = c.top_k if c.kind == "diverse" else c.k
    idx, sc = np.full((nq, top), -1, np.int64), np.zeros((nq, top), np.float32)
    p_hat = ivf_reference.stored_rows(m.E, ref.base_storage(c.storage))
    if c.kind == "ivf":
        near = oracle.scores(oracle.normalize_rows(p_hat), oracle.normalize_rows(c.C))
        home = [int(np.flatnonzero(row == row.max())[0]) for row in near]
        cq = oracle.scores(oracle.normalize_rows(c.q), oracle.normalize_rows(c.C))
    for i in range(nq):
        ok = []
        for r in range(n):
            good = c.excl is None or r not in c.excl[i]
            if c.allow is not None and c.allow[i] is not None:
                for f, values in enumerate(c.allow[i]):
                    good &= values is None or int(m.F[r, f]) in values
            if c.set_ids is not None:
                for s in c.set_ids[i]:
                    good &= s < 0 or (s < 3 and bool(m.M[s, r]))
            if c.kind == "ivf":
                probed = sorted(range(c.C.shape[0]), key=lambda l: (-float(cq[i, l]), l))[:c.nprobe]
                good &= home[r] in probed
            ok.append(bool(good))
        score = {r: c.scores[i, r] + np.float32(0) for r in range(n)}
        if c.boosts is not None:
            rows, w = c.boosts[i]
            for r, wr in zip(rows.tolist(), w.tolist()):
                if wr > 0:                                       # (a NaN fails the comparison: the weight counts as 0)
                    score[r] = np.float32(c.scores[i, r] + np.float32(wr))
            if c.kind == "boosted-only":
                ok = [ok[r] and r in rows.tolist() for r in range(n)]
        ranking = sorted((r for r in range(n) if ok[r]), key=lambda r: (-float(score[r]), r))
        if c.kind in ("capped", "capped+boosted"):
            kept, count = [], collections.Counter()
            for r in ranking:
                if all(c.caps[i, f] <= 0 or count[f, int(m.F[r, f])] < c.caps[i, f] for f in range(2)):
                    kept.append(r)
                    for f in range(2):
                        count[f, int(m.F[r, f])] += 1
            ranking = kept
        if c.kind == "diverse":
            cand, picks, lam = ranking[:c.k], [], np.float32(c.lam)
            sim = oracle.scores(p_hat[cand], p_hat[cand]) if cand else None
            while cand and len(picks) < c.top_k:
                best = None
                for j in range(len(cand)):
                    if j in picks:
                        continue
                    v = score[cand[j]] if not picks else \
                        np.float32(lam * score[cand[j]]) - np.float32((np.float32(1) - lam) * max(sim[j, p] for p in picks))
                    if best is None or v > best[0]:
                        best = (v, j)
                if best is None:
                    break
                picks.append(best[1])
            ranking = [cand[j] for j in picks]
        for pos, r in enumerate(ranking[:top]):
            idx[i, pos], sc[i, pos] = c.row_offset + r, score[r]
    return idx, sc


@pytest.mark.parametrize("kind", fc.KINDS)
def test_reference_against_brute_force(kind):
    features = collections.Counter()
    for c in itertools.islice(fc.cases(3, 10_000, kind, tiny=True), 12):
        assert c.model.n <= 40
        want, got = brute_force(c), ref.expected(c)
        np.testing.assert_array_equal(got[0], want[0], err_msg=c.describe())
        np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=c.describe())
        features.update(ref.active_features(c) + ["edited"] * bool(c.script))
    assert features["edited"] >= 2 and features["exclusions"] >= 2, features
