"""DeviceIndex.search_capped on the GPU: its result is the one-pass greedy capped walk of rank_all's complete ranking
restricted to the rows that the query's exclusions, facet masks and row sets admit (with boosts: of the ranking under
the adjusted scores), for 1 and 65 queries on a 1,000 x 64 index; and a catalog that forces a second round."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd.search import facet_masks, rowset_bits, rowset_ids
from tests import cap_reference as ref
from tests.search_harness import DeviceIndex, admitted_matrix, torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N, DIM = 1000, 64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def case(torch_cuda):
    """A clustered catalog whose clusters are aisles (so a query's best rows share few aisles), 5 departments, two
    row sets, 65 queries near rows of the catalog, and per query: exclusions, masks, set ids, caps."""
    rng = np.random.default_rng(17)
    centres = rng.standard_normal((40, DIM)).astype(np.float32)
    cluster = rng.integers(0, 40, N)
    P = centres[cluster] + np.float32(0.3) * rng.standard_normal((N, DIM)).astype(np.float32)
    F = np.stack([cluster * 6 + 15, rng.integers(0, 5, N)], axis=1).astype(np.uint8)  # aisles 15 .. 249, word edges among them
    Q = 65
    q = P[rng.choice(N, Q, replace=False)] + np.float32(0.1) * rng.standard_normal((Q, DIM)).astype(np.float32)
    member = np.stack([np.arange(N) % 2 == 0, np.arange(N) < 700])
    ix = DeviceIndex(P)
    ix.set_facets(F)
    ix.set_rowsets(rowset_bits(member, N))
    excl = [rng.choice(N, int(rng.integers(0, 40)), replace=False).tolist() if i % 2 else [] for i in range(Q)]
    allow = [None if i % 3 == 0 else ([a for a in range(256) if a % 4 != i % 4], None if i % 3 == 1 else [0, 1, 3])
             for i in range(Q)]
    within = [None if i % 4 == 0 else [1] if i % 4 == 1 else [0] if i % 4 == 2 else [0, 1] for i in range(Q)]
    caps = np.stack([rng.choice([0, 1, 2], Q), rng.choice([0, 1, 3], Q)], axis=1)
    caps[0] = (1, 1)
    masks = facet_masks(allow, Q, 2)
    ok = admitted_matrix(F, masks)
    for i, w in enumerate(within):
        for s in w or ():
            ok[i] &= member[s]
    order = ix.rank_all(q).cpu().numpy()          # [Q, N] rows, best first
    scores = ix.scores(q).cpu().numpy()           # [Q, N] icrec_scores' bits
    yield dict(ix=ix, P=P, F=F, q=q, excl=excl, allow=allow, within=within, caps=caps, ok=ok, order=order, scores=scores,
               member=member)
    ix.close()


def walk_of_ranking(order, scores, F, caps, top_k, ok):
    """The one-pass capped walk of each query's complete ranking `order` over the admissible rows `ok`."""
    Q = order.shape[0]
    idx = np.full((Q, top_k), -1, np.int64)
    sc = np.zeros((Q, top_k), np.float32)
    for i in range(Q):
        count = np.zeros((2, 256), np.int64)
        m = 0
        for r in order[i]:
            if m == top_k:
                break
            if ok[i, r] and all(caps[i, f] <= 0 or count[f, F[r, f]] < caps[i, f] for f in (0, 1)):
                idx[i, m], sc[i, m] = r, scores[i, r]
                count[0, F[r, 0]] += 1
                count[1, F[r, 1]] += 1
                m += 1
    return idx, sc


@pytest.mark.parametrize("Q", [1, 65])
def test_equals_the_walk_of_the_complete_ranking(case, Q):
    c = case
    ix, sel = c["ix"], slice(0, Q)
    ok = c["ok"][sel].copy()
    for i in range(Q):
        ok[i, c["excl"][i]] = False
    masks = facet_masks(c["allow"][sel], Q, 2, ix.device)
    sets = rowset_ids(c["within"][sel], Q, None, ix.device)
    rounds = []
    for top_k, width in ((20, None), (20, 20), (7, 128), (50, 50)):
        want = walk_of_ranking(c["order"][sel], c["scores"][sel], c["F"], c["caps"][sel], top_k, ok)
        idx, sc = ix.search_capped(c["q"][sel], top_k, c["caps"][sel], width, c["excl"][sel], masks, sets)
        np.testing.assert_array_equal(idx.cpu().numpy(), want[0])
        np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(want[1]))
        rounds.append(ix.last_cap_rounds)
    assert min(rounds) >= 1 and (Q == 1 or max(rounds) >= 2), rounds
    # no constraint but the caps; and no cap at all is the plain search
    want = walk_of_ranking(c["order"][sel], c["scores"][sel], c["F"], c["caps"][sel], 20, np.ones((Q, N), bool))
    idx, sc = ix.search_capped(c["q"][sel], 20, c["caps"][sel])
    np.testing.assert_array_equal(idx.cpu().numpy(), want[0])
    np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(want[1]))
    idx, sc = ix.search_capped(c["q"][sel], 20, (0, None), 30)
    plain = ix.search(c["q"][sel], 20)
    assert torch.equal(idx, plain[0]) and torch.equal(sc, plain[1]) and ix.last_cap_rounds == 1


@pytest.mark.parametrize("Q", [1, 65])
def test_with_boosts_equals_the_walk_of_the_boosted_ranking(case, Q):
    c = case
    ix, sel = c["ix"], slice(0, Q)
    rng = np.random.default_rng(23)
    ok = c["ok"][sel].copy()
    for i in range(Q):
        ok[i, c["excl"][i]] = False
    masks = facet_masks(c["allow"][sel], Q, 2, ix.device)
    sets = rowset_ids(c["within"][sel], Q, None, ix.device)
    boosts, adjusted = [], c["scores"][sel].copy()
    for i in range(Q):
        if i % 5 == 4:
            boosts.append(None)
            continue
        inside = np.flatnonzero(np.all([c["member"][s] for s in c["within"][i] or ()] or [np.ones(N, bool)], axis=0))
        rows = rng.choice(inside, 30, replace=False)  # (listed rows outside the query's sets are the caller's to drop)
        w = rng.choice([0.0, 0.25, 2.0], 30).astype(np.float32)
        boosts.append({int(r): float(v) for r, v in zip(rows, w)})
        lifted = w != 0
        adjusted[i, rows[lifted]] = adjusted[i, rows[lifted]] + w[lifted]  # one fp32 addition
    for top_k, width in ((20, None), (10, 10)):
        want = ref.greedy_walk(adjusted, c["F"], c["caps"][sel], top_k, admit=ok)
        idx, sc = ix.search_capped(c["q"][sel], top_k, c["caps"][sel], width, c["excl"][sel], masks, sets, boosts=boosts)
        np.testing.assert_array_equal(idx.cpu().numpy(), want[0])
        np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(want[1]))
    # only=True: the listed rows alone, capped
    listed = np.zeros((Q, N), bool)
    for i, b in enumerate(boosts):
        listed[i, list(b or ())] = True
    want = ref.greedy_walk(adjusted, c["F"], c["caps"][sel], 10, admit=ok & listed)
    idx, sc = ix.search_capped(c["q"][sel], 10, c["caps"][sel], 40, c["excl"][sel], masks, sets, boosts=boosts, only=True)
    np.testing.assert_array_equal(idx.cpu().numpy(), want[0])
    np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(want[1]))


def test_forced_second_round(torch_cuda):
    """The 130 rows nearest the query are one aisle: at cap 2 the first round's 128 candidates give exactly 2 picks and
    no pad, so the list is not done and the rows 3 .. 5 come from a further search."""
    rng = np.random.default_rng(29)
    v = rng.standard_normal(DIM).astype(np.float32)
    P = rng.standard_normal((N, DIM)).astype(np.float32)
    near = rng.permutation(N)[:130]
    P[near] = v[None, :] + np.float32(0.05) * rng.standard_normal((130, DIM)).astype(np.float32)
    F = np.stack([rng.integers(10, 100, N), rng.integers(0, 4, N)], axis=1).astype(np.uint8)
    F[near, 0] = 9
    # the precondition, from the inputs alone: every near row scores far above every other row
    cos = (P @ v) / (np.linalg.norm(P, axis=1) * np.linalg.norm(v))
    far = np.setdiff1d(np.arange(N), near)
    assert cos[near].min() > cos[far].max() + 0.2
    ix = DeviceIndex(P, row_offset=500)
    ix.set_facets(F)
    order = ix.rank_all(v).cpu().numpy() - 500
    scores = ix.scores(v).cpu().numpy()
    assert set(order[0, :130]) == set(near)
    first = ix.cap_select(*ix.search(v, 128), (2, 0), 5)
    assert first[2].tolist() == [[2, 0]] and first[0][0, :2].tolist() == (order[0, :2] + 500).tolist()
    want = walk_of_ranking(order, scores, F, np.array([[2, 0]]), 5, np.ones((1, N), bool))
    assert list(want[0][0, :2]) == list(order[0, :2]) and not set(want[0][0, 2:]) & set(near) and (want[0] >= 0).all()
    for width in (128, 5):
        idx, sc = ix.search_capped(v, 5, (2, 0), width)
        assert ix.last_cap_rounds >= 2
        np.testing.assert_array_equal(idx.cpu().numpy(), want[0] + 500)
        np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(want[1]))
    ix.close()
