"""The IVF index on the GPU (icrec_ivf, search.IvfIndex): layout and search against tests/ivf_reference.py, bit for
bit, at the edges of the 256-row tiles and of the slices a list is cut into; graph capture; the centroid trainer; and
Recommender(ann_lists=...)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender, diversity_plan
from instacart_next_order_recommendation_amd.search import DeviceIndex, IvfIndex, train_centroids
from oracle import oracle
from tests import ivf_reference as ref
from tests.recommender_harness import QUERIES, as_results, graph_replays, synthetic_world
from tests.search_harness import (assert_search, distinct_exclusions, n_cu, tie_block_catalog,  # noqa: F401
                                  torch_cuda)

pytestmark = pytest.mark.gpu

ROW_OFFSET = 1000


def slices(Q, nprobe):
    """csrc/ivf.hip's plan_slices: slices per probed list, from Q, nprobe and the CU count."""
    target, items = 2 * n_cu(), Q * nprobe
    return 1 if items >= target else min(-(-target // items), 1024 // nprobe)


def oracle_storage(storage):
    return "bf16" if storage.startswith("bf16") else "f32"


# ---------------------------------------------------------------- the crafted catalog
@pytest.fixture(scope="module", params=["f32", "bf16"])
def crafted(request, torch_cuda):
    storage = request.param
    P, C, _ = ref.crafted_catalog()
    a = ref.crafted_preconditions(storage)
    base = DeviceIndex(P, row_offset=ROW_OFFSET, storage=storage)
    ivf = IvfIndex(base, C)
    yield storage, P, C, a, base, ivf
    ivf.close()
    base.close()


@pytest.fixture(scope="module")
def crafted_queries():
    """70 queries: query i sits near centroid i % 8 (query 2 and 4 near the shared centroid of lists 2 and 4)."""
    _, C, _ = ref.crafted_catalog()
    rng = np.random.default_rng(8)
    return (C[np.arange(70) % 8] + np.float32(0.3) * rng.standard_normal((70, 64)).astype(np.float32)).astype(np.float32)


def test_layout_of_the_crafted_catalog(crafted):
    _, _, C, a, _, ivf = crafted
    assert ivf.n_lists == 8
    perm, off = ivf.layout()
    want = ref.layout(a, 8)
    np.testing.assert_array_equal(perm.cpu().numpy(), want[0])
    np.testing.assert_array_equal(off.cpu().numpy(), want[1])
    assert perm.dtype == torch.int32 and off.dtype == torch.int64


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_layout_at_width_384(torch_cuda, storage):
    rng = np.random.default_rng(31)
    P = rng.standard_normal((5000, 384)).astype(np.float32)
    C = P[rng.choice(5000, 37, replace=False)].copy()
    base = DeviceIndex(P, storage=storage)
    ivf = IvfIndex(base, C)
    perm, off = ivf.layout()
    want = ref.layout(ref.assign(ref.stored_rows(P, storage), C), 37)
    np.testing.assert_array_equal(perm.cpu().numpy(), want[0])
    np.testing.assert_array_equal(off.cpu().numpy(), want[1])
    ivf.close()
    base.close()


@pytest.mark.parametrize("Q", [1, 3, 70])
def test_search_on_the_crafted_catalog(crafted, crafted_queries, Q):
    """Lists of 1, 255, 256, 257 and 1,300 rows and an empty one, at k = 1, 20 and 128 (more than most probed lists
    hold: pads) and 1, 2 and all 8 probes, with a row offset.  One query: every list is cut into many slices of at most
    one tile; 70 queries at 8 probes: one slice per list, so the 1,300-row list's six tiles run the warm-tile path."""
    storage, P, C, a, _, ivf = crafted
    assert slices(1, 8) > 6 and slices(70, 8) == 1
    batches = [crafted_queries[i:i + 1] for i in range(8)] if Q == 1 else [crafted_queries[4:7]] if Q == 3 else [crafted_queries]
    for q in batches:
        for k in (1, 20, 128):
            for nprobe in (1, 2, 8):
                want = ref.search(q, P, C, k, nprobe, None, ROW_OFFSET, oracle_storage(storage), a)
                assert_search(ivf.search(q, k, nprobe), want)
    # the query next to centroid 2 scans list 2 and then the empty list 4; the one next to centroid 0 a single row
    np.testing.assert_array_equal(ref.probes(crafted_queries[2:3], C, 2), [[2, 4]])
    lone = ivf.search(crafted_queries[0:1], 20, 1)[0].cpu().numpy()
    assert (lone[0, 1:] == -1).all() and lone[0, 0] == ROW_OFFSET + int(np.flatnonzero(a == 0)[0])


@pytest.mark.parametrize("storage", ["f32", "bf16", "f32+filter"])
def test_all_probes_equal_the_exact_search(torch_cuda, crafted_queries, storage):
    P, C, _ = ref.crafted_catalog()
    base = DeviceIndex(P, row_offset=ROW_OFFSET, storage=storage)
    ivf = IvfIndex(base, C)
    rng = np.random.default_rng(17)
    for q in (crafted_queries[:1], crafted_queries[:3], crafted_queries):
        excl = distinct_exclusions(rng, len(P), len(q))
        for k in (1, 20, 128):
            got = ivf.search(q, k, 8, excl)
            exact = base.search(q, k, excl)
            assert torch.equal(got[0], exact[0]) and torch.equal(got[1], exact[1])
            assert_search(got, oracle.search(q, P, k, excl, row_offset=ROW_OFFSET, storage=oracle_storage(storage)))
    ivf.close()
    base.close()


def test_exclusions_that_empty_a_list_or_leave_few_rows(crafted, crafted_queries):
    storage, P, C, a, _, ivf = crafted
    q = crafted_queries[7:8]  # near centroid 7: a list of 40 rows
    rows7 = np.flatnonzero(a == 7)
    assert rows7.size == 40 and ref.probes(q, C, 1)[0, 0] == 7
    for excl, nprobe, n_real in (([rows7.tolist()], 1, 0), ([rows7.tolist()], 2, 20), ([rows7[:30].tolist()], 1, 10)):
        want = ref.search(q, P, C, 20, nprobe, excl, ROW_OFFSET, oracle_storage(storage), a)
        assert (want[0] >= 0).sum() == n_real
        assert_search(ivf.search(q, 20, nprobe, excl), want)


# ---------------------------------------------------------------- other catalogs
def test_equal_scores_are_ordered_by_the_original_row(torch_cuda):
    """300 identical rows fall in one list, span more than one tile and meet slice boundaries; among their equal scores
    only the original row number decides, whatever their place in the list."""
    rng = np.random.default_rng(5)
    P, base_row = tie_block_catalog(rng, 4000, 64)
    C = np.concatenate([base_row[None, :], P[rng.choice(4000, 15, replace=False)]]).astype(np.float32)
    a = ref.assign(ref.stored_rows(P), C)
    dup = np.flatnonzero((P == base_row).all(axis=1))
    assert dup.size == 300 and (a[dup] == 0).all() and (a == 0).sum() > 256
    base = DeviceIndex(P)
    ivf = IvfIndex(base, C)
    q = base_row[None, :].copy()
    for nprobe in (1, 16):
        for k in (20, 128):
            want = ref.search(q, P, C, k, nprobe, assignment=a)
            assert (np.diff(want[0][0][want[1][0] == want[1][0][0]]) > 0).all()
            assert_search(ivf.search(q, k, nprobe), want)
    ivf.close()
    base.close()


@pytest.mark.parametrize("dim,storage", [(32, "f32"), (384, "f32"), (384, "bf16"), (768, "f32"), (768, "bf16")])
def test_widths(torch_cuda, dim, storage):
    rng = np.random.default_rng(dim)
    P = rng.standard_normal((3000, dim)).astype(np.float32)
    C = P[rng.choice(3000, 12, replace=False)].copy()
    q = (P[rng.choice(3000, 8, replace=False)] + np.float32(0.2) * rng.standard_normal((8, dim)).astype(np.float32))
    a = ref.assign(ref.stored_rows(P, storage), C)
    base = DeviceIndex(P, storage=storage)
    ivf = IvfIndex(base, C)
    for qq in (q[:1], q):
        assert_search(ivf.search(qq, 20, 3), ref.search(qq, P, C, 20, 3, storage=storage, assignment=a))
    ivf.close()
    base.close()


def test_many_partial_lists(torch_cuda):
    """128 probes of one query: nprobe * S partial lists per query reach the merge's wide arm (more than 256 lists)."""
    assert 128 * slices(1, 128) > 256
    rng = np.random.default_rng(77)
    P = rng.standard_normal((6000, 64)).astype(np.float32)
    C = P[rng.choice(6000, 128, replace=False)].copy()
    q = rng.standard_normal((1, 64)).astype(np.float32)
    base = DeviceIndex(P)
    ivf = IvfIndex(base, C)
    got = ivf.search(q, 20, 128)
    exact = base.search(q, 20)
    assert torch.equal(got[0], exact[0]) and torch.equal(got[1], exact[1])
    assert_search(got, oracle.search(q, P, 20))
    ivf.close()
    base.close()


# ---------------------------------------------------------------- graph capture
def test_search_into_is_graph_capturable(crafted, crafted_queries):
    storage, P, C, a, base, ivf = crafted
    k, nprobe = 20, 2
    qd = torch.from_numpy(crafted_queries[5:6].copy()).to(base.device)
    idx = torch.empty((1, k), dtype=torch.int64, device=base.device)
    sc = torch.empty((1, k), dtype=torch.float32, device=base.device)
    ws = ivf._workspace(1, k, nprobe)
    ivf.search_into(qd, k, nprobe, None, None, idx, sc, ws=ws)  # first launches outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ivf.search_into(qd, k, nprobe, None, None, idx, sc, ws=ws)
    qd.copy_(torch.from_numpy(crafted_queries[6:7].copy()))
    idx.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert_search((idx, sc), ref.search(crafted_queries[6:7], P, C, k, nprobe, None, ROW_OFFSET, oracle_storage(storage), a))


# ---------------------------------------------------------------- the trainer
def test_train_centroids(torch_cuda):
    P = syn.synthetic_embeddings(4000, 64, seed=4)
    base = DeviceIndex(P)

    def mean_best_cosine(cent, rows):
        tmp = DeviceIndex(cent)
        s = tmp.search(rows, 1)[1].mean().item()
        tmp.close()
        return s

    c5 = train_centroids(base, 16, iters=5, sample=64, seed=3)
    again = train_centroids(base, 16, iters=5, sample=64, seed=3)
    assert c5.shape == (16, 64) and c5.dtype == torch.float32 and torch.equal(c5, again)
    assert (torch.linalg.norm(c5.double(), dim=1) - 1).abs().max().item() <= 1e-6
    c0 = train_centroids(base, 16, iters=0, sample=64, seed=3)
    gen = torch.Generator().manual_seed(3)
    sample = base.export()[torch.randperm(4000, generator=gen)[:64 * 16].to(base.device)]
    assert torch.equal(c0, sample[:16])  # the initial centroids are the first rows of the sample
    assert mean_best_cosine(c5, sample) >= mean_best_cosine(c0, sample)
    base.close()


# ---------------------------------------------------------------- the recommender
N_LISTS = 16


@pytest.fixture(scope="module")
def rec(tmp_path_factory, torch_cuda):
    w = synthetic_world(tmp_path_factory.mktemp("ivf_rec"))
    r = MonitoredRecommender(w.model_dir, w.corpus_path, use_index=False, ann_lists=N_LISTS)
    assert r._fast is not None and r._ann.n_lists == N_LISTS
    return r


def test_recommend_with_probes(rec, monkeypatch):
    perm, off = (t.cpu().numpy() for t in rec._ann.layout())
    list_of = np.empty(700, np.int64)
    list_of[perm] = np.repeat(np.arange(N_LISTS), np.diff(off))
    calls = graph_replays(rec, monkeypatch)
    for q in QUERIES:
        plain = rec.recommend(q, 20)
        calls.clear()
        assert rec.recommend(q, 20, probes=None) == plain and len(calls) == 1  # the graph path, as before
        calls.clear()
        assert rec.recommend(q, 20, probes=N_LISTS) == plain and not calls
        one = rec.recommend(q, 20, probes=1)
        assert one and len({list_of[rec._pid_to_row[p]] for p, _ in one}) == 1
        gone = {p for p, _ in plain[:5]}
        kept = rec.recommend(q, 20, exclude_product_ids=gone, probes=N_LISTS)
        assert kept == rec.recommend(q, 20, exclude_product_ids=gone) and not gone & {p for p, _ in kept}
        lam, width = diversity_plan(0.5, None, 20, 700)
        emb = torch.from_numpy(rec.model.encode([q])).to(rec.device)
        idx, sc = rec._index.mmr_select(*rec._ann.search(emb, width, 4), 20, lam)
        assert rec.recommend(q, 20, diversity=0.5, probes=4) == as_results(rec, idx[0].cpu().numpy(), sc[0].cpu().numpy())
    assert rec.recommend_batch(QUERIES, 20, probes=N_LISTS) == rec.recommend_batch(QUERIES, 20)
    assert rec.recommend_batch(QUERIES, 20, probes=2) == [rec.recommend(q, 20, probes=2) for q in QUERIES]
    with pytest.raises(ValueError, match="aisles"):
        rec.recommend(QUERIES[0], 20, probes=2, aisles=[rec.aisles[0]])
    with pytest.raises(ValueError, match="probes must be"):
        rec.recommend(QUERIES[0], 20, probes=N_LISTS + 1)
