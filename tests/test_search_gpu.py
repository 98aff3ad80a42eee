"""HIP search path (through the C ABI) against the CPU oracle — bit-exact scores and indices."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests.conftest import excl_lists
from tests.search_harness import (DeviceIndex, assert_ranked_lists, assert_search, bench_catalog, bench_queries, check,
                                  distinct_exclusions, full_ranking, merge_topk, oracle, pack_keys, search,
                                  sharded_partial_keys, synthetic as syn, tie_block_catalog, timed)
from tests.search_harness import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def test_normalize_rows_bit_exact(torch_cuda, golden_search):
    x = golden_search["P"]
    got = search.normalize_rows(torch.from_numpy(x).cuda()).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.normalize_rows(x))


def test_index_holds_normalized_rows(torch_cuda, golden_search):
    ix = DeviceIndex(golden_search["P"])
    np.testing.assert_array_equal(ix.export().cpu().numpy(), oracle.normalize_rows(golden_search["P"]))


@pytest.mark.parametrize("nq", [1, 16])
def test_scores_bit_exact_vs_oracle(torch_cuda, golden_search, nq):
    """Every cosine score equals the oracle's k-ascending fmaf chain bit for bit, and
    sentence_transformers.util.cos_sim's torch restatement within 1e-4 (north_star)."""
    g = golden_search
    ix = DeviceIndex(g["P"])
    got = ix.scores(g["q"][:nq]).cpu().numpy()
    np.testing.assert_array_equal(got, g["oracle_scores"][:nq])
    assert np.abs(got - g["torch_scores"][:nq]).max() < 1e-4


def test_topk_golden_with_exclusions(torch_cuda, golden_search):
    g = golden_search
    k = int(g["k"])
    excl = excl_lists(g["excl_flat"], g["excl_off"])
    idx, sc = DeviceIndex(g["P"]).search(g["q"], k, excl)
    assert_search((idx, sc), (g["oracle_idx"], g["oracle_topk_scores"]))
    # and against the torch restatement of the reference wherever torch's own order is unambiguous
    amb = g["torch_ambiguous"]
    np.testing.assert_array_equal(idx.cpu().numpy()[~amb], g["torch_idx"][~amb])


def test_tie_policy(torch_cuda, golden_search):
    g = golden_search
    ix = DeviceIndex(g["P_tie"])
    assert_search(ix.search(g["q"][:4], int(g["k"])), (g["oracle_tie_idx"], g["oracle_tie_scores"]))


def test_full_catalog_golden(torch_cuda, golden_search_full):
    g = golden_search_full
    P = syn.synthetic_embeddings(49688, 384, seed=int(g["P_seed"]))
    q = syn.synthetic_embeddings(8, 384, seed=int(g["q_seed"]))
    ix = DeviceIndex(P)
    assert_search(ix.search(q, int(g["k"])), (g["oracle_idx"], g["oracle_topk_scores"]))
    # single query (the /recommend shape) gives the same row
    idx1, sc1 = ix.search(q[3], int(g["k"]))
    np.testing.assert_array_equal(idx1.cpu().numpy()[0], g["oracle_idx"][3])


@pytest.mark.parametrize("nq,k,n", [(1, 1, 33), (3, 7, 257), (40, 20, 1000), (70, 50, 3000), (130, 20, 5000),
                                      (200, 100, 2049), (33, 128, 640)])
def test_shapes_vs_oracle(torch_cuda, nq, k, n):
    """Ragged sizes across all three tile variants, with random exclusion lists."""
    rng = np.random.default_rng(nq * 1000 + k)
    P = rng.standard_normal((n, 384)).astype(np.float32)
    q = rng.standard_normal((nq, 384)).astype(np.float32)
    check(DeviceIndex(P), q, P, k, distinct_exclusions(rng, n, nq))


def test_edge_cases(torch_cuda):
    rng = np.random.default_rng(0)
    P = rng.standard_normal((7, 384)).astype(np.float32)
    q = rng.standard_normal((2, 384)).astype(np.float32)
    ix = DeviceIndex(P)
    for k, excl in [(10, None), (5, [list(range(7)), [0]]), (3, [[], [1, 2, 3]])]:
        check(ix, q, P, k, excl)
    z = np.zeros((1, 384), np.float32)  # zero query: all scores 0, ties resolved by row order
    idx, sc = ix.search(z, 3)
    assert idx.cpu().numpy()[0].tolist() == [0, 1, 2] and (sc.cpu().numpy() == 0).all()
    ix_off = DeviceIndex(P, row_offset=1000)
    idx, _ = ix_off.search(q, 3)
    assert idx.min().item() >= 1000


def test_bad_arguments_raise(torch_cuda):
    from instacart_next_order_recommendation_amd._native import IcrecError

    P = np.ones((4, 384), np.float32)
    ix = DeviceIndex(P)
    with pytest.raises(IcrecError):
        ix.search(P[:1], 0)
    with pytest.raises(IcrecError):
        ix.search(P[:1], 129)
    with pytest.raises(IcrecError):
        DeviceIndex(np.ones((4, 100), np.float32))  # dim not a multiple of 32


def test_sharded_merge_equals_unsharded(torch_cuda, golden_search):
    """Per-shard partial lists + k-way merge == single-index result (the multi-GPU exactness claim)."""
    g = golden_search
    k = int(g["k"])
    excl = excl_lists(g["excl_flat"], g["excl_off"])
    bounds = [0, 100, 356, 700, 1024]  # uneven shards
    keys = sharded_partial_keys(g["P"], g["q"], k, excl, bounds)
    assert_search(merge_topk(keys, k), (g["oracle_idx"], g["oracle_topk_scores"]))


def test_large_batch_properties(torch_cuda):
    """BASELINE config 3 size (1024 x 49,688): size-independent properties — sorted output,
    scores reproduce from the returned rows, k-th score bounds every unreturned row on a sample."""
    P, q = bench_catalog(), bench_queries(1024, 3)
    ix = DeviceIndex(P)
    idx, sc = ix.search(q, 20)
    assert_ranked_lists(idx, sc, 0, 49688, 20)
    # exact check of a sample of queries against the oracle
    sample = [0, 1, 511, 777, 1023]
    assert_search((idx[sample], sc[sample]), oracle.search(q[sample], P, 20))
    # idempotence: same call, same bits
    idx2, sc2 = ix.search(q, 20)
    assert torch.equal(idx, idx2) and torch.equal(sc, sc2)


# ---------------------------------------------------------------- bf16 row storage (BASELINE config 5)
def test_bf16_index_holds_rounded_rows(torch_cuda, golden_search):
    """ICREC_ROWS_BF16: normalise in fp32, then round to bfloat16 (RNE) — bit-identical to the oracle
    and to torch's own fp32 -> bf16 conversion of the same normalised rows."""
    ix = DeviceIndex(golden_search["P"], storage="bf16")
    got = ix.export().cpu().numpy()
    want = oracle.round_bf16(oracle.normalize_rows(golden_search["P"]))
    np.testing.assert_array_equal(got, want)
    t = torch.from_numpy(oracle.normalize_rows(golden_search["P"])).to(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(got, t)


@pytest.mark.parametrize("nq,k,n", [(1, 20, 1024), (3, 7, 257), (40, 20, 1000), (70, 50, 3000), (130, 20, 5000),
                                      (200, 100, 2049)])
def test_bf16_rows_search_vs_oracle(torch_cuda, nq, k, n):
    """bf16 storage changes the stored rows only: indices AND scores stay bit-exact against the oracle
    run on the same rounded rows (all three tile variants, random exclusions)."""
    rng = np.random.default_rng(nq * 977 + k)
    P = rng.standard_normal((n, 384)).astype(np.float32)
    q = rng.standard_normal((nq, 384)).astype(np.float32)
    ix = DeviceIndex(P, storage="bf16")
    check(ix, q, P, k, distinct_exclusions(rng, n, nq))
    # the full score matrix too
    full = ix.scores(q).cpu().numpy()
    np.testing.assert_array_equal(full, oracle.scores(oracle.normalize_rows(q), oracle.round_bf16(oracle.normalize_rows(P))))
    # and it is a faithful approximation of the fp32 catalog: cosine within bf16 rounding of the rows
    ref = oracle.scores(oracle.normalize_rows(q), oracle.normalize_rows(P))
    assert np.abs(full - ref).max() < 2e-3


def test_bf16_rows_full_catalog_sample(torch_cuda):
    """49,688 rows x 1,024 queries in bf16 storage: sorted, unique, and a sample of queries exact vs the oracle."""
    P, q = bench_catalog(), bench_queries(1024, 3)
    ix = DeviceIndex(P, storage="bf16")
    idx, sc = ix.search(q, 20)
    assert_ranked_lists(idx, sc, 0, 49688, 20)
    sample = [0, 5, 512, 1023]
    assert_search((idx[sample], sc[sample]), oracle.search(q[sample], P, 20, storage="bf16"))
    with pytest.raises(ValueError):
        DeviceIndex(P[:4], storage="fp8")


# ---------------------------------------------------------------- small-batch streaming kernel (Q <= 8)
@pytest.fixture(scope="module")
def big_clustered():
    """400,000 clustered rows + 8 queries (numpy generator: the repo's counter-based one takes a minute at this size)."""
    rng = np.random.default_rng(11)
    centres = rng.standard_normal((200, 384)).astype(np.float32)
    P = centres[rng.integers(0, 200, 400_000)] + 0.35 * rng.standard_normal((400_000, 384), dtype=np.float32)
    q = centres[rng.integers(0, 200, 8)] + 0.35 * rng.standard_normal((8, 384), dtype=np.float32)
    return P, q


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("nq,k", [(1, 20), (2, 1), (5, 100), (8, 20)])
def test_stream_kernel_multi_tile_chunks(torch_cuda, big_clustered, storage, nq, k):
    """400,000 rows = 1,563 tiles of 256 rows over <= 768 blocks: every block runs its cold first tile
    (rank by counting) AND warm tiles (threshold + queue + merge), with exclusions that hit the true
    top of each list.  Bit-exact indices and scores against the oracle."""
    n = 400_000
    P, qall = big_clustered
    q = qall[:nq]
    top_i, _ = oracle.search(q, P, 8, storage=storage)
    rng = np.random.default_rng(nq + k)
    excl = [sorted(set(top_i[i, ::2].tolist()) | set(rng.choice(n, 30, replace=False).tolist())) for i in range(nq)]
    excl[0] = []  # one query without exclusions
    # the search itself, and its partial lists + merge (> 256 lists through the 16-lists-per-lane merge)
    check(DeviceIndex(P, storage=storage), q, P, k, excl, partial=True)


def test_merge_many_lists(torch_cuda):
    """icrec_merge_topk with 700 lists (the streaming kernel's chunk count exceeds 256)."""
    rng = np.random.default_rng(3)
    n_lists, Q, k = 700, 3, 20
    sc = rng.standard_normal((n_lists, Q, k)).astype(np.float32)
    sc = -np.sort(-sc, axis=2)
    idx = (np.arange(n_lists)[:, None, None] * 1000 + np.arange(k)[None, None, :] + np.zeros((1, Q, 1), np.int64)).astype(np.int64)
    keys = pack_keys(sc, idx)
    assert_search(merge_topk(torch.from_numpy(keys.view(np.int64)).cuda(), k), oracle.merge(idx, sc))


# ---------------------------------------------------------------- filter + verify (ICREC_ROWS_F32_FILTER)
@pytest.mark.parametrize("nq,k,n", [(256, 20, 1000), (300, 50, 3000), (513, 20, 5000), (384, 100, 2049), (257, 1, 777),
                                      (260, 116, 4000), (256, 120, 3000), (70, 20, 3000)])
@pytest.mark.parametrize("resident", ["1", "0"])
def test_filter_index_is_bit_identical_to_exact(torch_cuda, monkeypatch, resident, nq, k, n):
    """f16x3 filter pass + exact verification returns the exact search's bits (indices, scores), with
    exclusions; k + slack > 128 and batches under 256 queries (last two cases) silently take the exact path.
    Both forms of the filter pass: resident (query planes in LDS, rows as packed fragments - the default) and staged (ICREC_FILTER_RESIDENT=0 at index creation: row-major planes, both operands through LDS)."""
    monkeypatch.setenv("ICREC_FILTER_RESIDENT", resident)
    rng = np.random.default_rng(nq * 31 + k)
    P = rng.standard_normal((n, 384)).astype(np.float32)
    q = rng.standard_normal((nq, 384)).astype(np.float32)
    check(DeviceIndex(P, storage="f32+filter"), q, P, k, distinct_exclusions(rng, n, nq), partial=True)


@pytest.mark.parametrize("order", ["ascending", "random"])
def test_resident_filter_long_blocks_ascending_scores(torch_cuda, order):
    """4,096 queries over 49,688 rows give every block of the resident filter pass 49 rounds.  "ascending": rows ordered
    so that every query's score GROWS with the row number - every round brings 256 rows better than anything the block
    has seen, so every round floods the candidate queues (offers that do not fit wait for the next merge iteration): the
    worst case of the selection.  Result: bit-identical to the exact index on all queries, to the oracle on a sample;
    with exclusion lists that knock out some of the very best rows.  (Written in round 4 for a barrier-free form of the
    selection that was measured and dropped, profiles/r04_search_epoch_mode_ab.txt; kept as the adversarial case.)"""
    rng = np.random.default_rng(17)
    n, nq, k = 49_688, 4096, 20
    d = rng.standard_normal(384).astype(np.float32)
    d /= np.linalg.norm(d)
    u = rng.standard_normal(384).astype(np.float32)
    u -= u.dot(d) * d
    u /= np.linalg.norm(u)
    t = np.linspace(-1.0, 1.0, n, dtype=np.float32)
    if order == "random":
        t = rng.permutation(t)
    P = u[None, :] + t[:, None] * d[None, :] + 0.02 * rng.standard_normal((n, 384)).astype(np.float32)
    q = d[None, :] + 0.02 * rng.standard_normal((nq, 384)).astype(np.float32)
    excl = distinct_exclusions(rng, n, nq, cap=30, every=3)
    if order == "ascending":  # also knock out a few of the very best rows of some queries
        for i in range(0, nq, 7):
            excl[i] = sorted(set(excl[i]) | {n - 1, n - 2, n - 5})
    Pd, qd = torch.from_numpy(P).cuda(), torch.from_numpy(q).cuda()
    fi = DeviceIndex(Pd, storage="f32+filter")
    ei = DeviceIndex(Pd, storage="f32")
    idx, sc = fi.search(qd, k, excl)
    xi, xs = ei.search(qd, k, excl)
    assert torch.equal(idx, xi) and torch.equal(sc, xs)
    sample = [0, 1, 7, 63, 64, 2047, 4095]
    assert_search((idx[sample], sc[sample]), oracle.search(q[sample], P, k, [excl[i] for i in sample]))
    fi.close(); ei.close()


def test_filter_falls_back_when_it_cannot_prove_the_result(torch_cuda):
    """Adversarial ties: 300 identical rows (more than any candidate list holds) are every query's best match,
    plus blocks of near-ties 1e-6 apart.  The verify pass cannot prove these, raises its flag, and the exact
    pass must deliver the oracle's answer (lower row first among equals)."""
    rng = np.random.default_rng(9)
    n, nq, k = 6000, 288, 20
    P, base = tie_block_catalog(rng, n, 384)
    q = base[None, :] + 0.05 * rng.standard_normal((nq, 384)).astype(np.float32)
    check(DeviceIndex(P, storage="f32+filter"), q, P, k)
    # a small catalog where k exceeds the admissible rows (lists not full -> proven complete, pads)
    Ps = P[:30]
    check(DeviceIndex(Ps, storage="f32+filter"), q, Ps, 20, [list(range(0, 30, 2))] * 288)


def test_filter_full_catalog_batch(torch_cuda):
    """BASELINE configs[2] size through the filter path: 1,024 x 49,688, all lists equal to the exact index's —
    and proven by the verify pass alone: the guarded exact pass (timer slot 4) exits at once, whereas the
    adversarial catalog of the previous test makes it run."""
    P, q = bench_catalog(), bench_queries(1024, 3)
    exact = DeviceIndex(P)
    ie, se = exact.search(q, 20)
    fx = DeviceIndex(P, storage="f32+filter")
    fx.search(q, 20)

    def filter_then_exact():
        out = fx.search(q, 20)
        exact.search(q, 20)
        return out

    (fi, fs), t = timed(filter_then_exact)
    assert torch.equal(ie, fi) and torch.equal(se, fs)
    sample = [0, 255, 256, 777, 1023]   # and against the oracle on THIS index, not only against the exact HIP path
    assert_search((fi[sample], fs[sample]), oracle.search(q[sample], P, 20))
    (fallback_ms, n_fb), (exact_ms, _) = t[4], t[0]
    assert n_fb == 1 and fallback_ms < 0.1 * exact_ms, (fallback_ms, exact_ms)  # exited at once: nothing was flagged
    # the adversarial case: the fallback really runs
    rng = np.random.default_rng(9)
    Pd = rng.standard_normal((6000, 384)).astype(np.float32)
    Pd[rng.choice(6000, 300, replace=False)] = Pd[0]
    qd = Pd[0][None, :] + 0.05 * rng.standard_normal((288, 384)).astype(np.float32)
    fd = DeviceIndex(Pd, storage="f32+filter")
    fd.search(qd, 20)
    _, t = timed(lambda: fd.search(qd, 20))
    fb2, _ = t[4]
    assert fb2 > 3 * fallback_ms, (fb2, fallback_ms)


@pytest.mark.parametrize("nq,k,n", [(256, 20, 3000), (300, 50, 5000)])
@pytest.mark.parametrize("resident", ["1", "0"])
def test_bf16_filter_index_is_bit_identical_to_bf16_exact(torch_cuda, monkeypatch, resident, nq, k, n):
    """ICREC_ROWS_BF16_FILTER: filter planes built from the ROUNDED rows, verification and fallback on the bf16 rows
    themselves — same bits as storage="bf16" and as the oracle's bf16 search, incl. a duplicate-row fallback;
    resident and staged form of the filter pass."""
    monkeypatch.setenv("ICREC_FILTER_RESIDENT", resident)
    rng = np.random.default_rng(nq + k)
    P = rng.standard_normal((n, 384)).astype(np.float32)
    P[rng.choice(n, 200, replace=False)] = P[1]  # 200 identical rows: some queries cannot be proven
    q = rng.standard_normal((nq, 384)).astype(np.float32)
    q[: nq // 4] = P[1] + 0.05 * q[: nq // 4]
    ix = DeviceIndex(P, storage="bf16+filter")
    check(ix, q, P, k, distinct_exclusions(rng, n, nq, cap=30))
    np.testing.assert_array_equal(ix.export().cpu().numpy(), oracle.round_bf16(oracle.normalize_rows(P)))


@pytest.mark.parametrize("n,nq,storage", [(49_688, 5, "f32"), (1000, 3, "f32"), (8192, 2, "f32"), (20_001, 4, "bf16"), (7, 2, "f32")])
def test_rank_all_full_order_vs_oracle(torch_cuda, n, nq, storage):
    """icrec_rank_all = the complete argsort(descending) of every score row under the library's total order:
    bit-exact scores (oracle) sorted by (score desc, row asc), duplicate rows included."""
    P = syn.synthetic_embeddings(n, 384, seed=31)
    if n > 100:
        P[17] = P[3]          # exact ties
        P[n - 1] = P[3]
    q = syn.synthetic_embeddings(nq, 384, seed=32)
    ix = DeviceIndex(P, storage=storage, row_offset=1000)
    got = ix.rank_all(torch.from_numpy(q).cuda()).cpu().numpy()
    assert got.shape == (nq, n)
    Pn = oracle.normalize_rows(P)
    if storage == "bf16":
        Pn = oracle.round_bf16(Pn)
    sc = oracle.scores(oracle.normalize_rows(q), Pn)
    for i in range(nq):
        np.testing.assert_array_equal(got[i] - 1000, full_ranking(sc[i]))
    ix.close()
