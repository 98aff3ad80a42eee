"""icrec_ir_metrics against tests/cf_reference.py, which adds in the same rank order with the same host-computed
discounts: every per-query value is compared bit for bit (NDCG included: dcg and idcg are the same two chains of
double additions and one division on both sides), the eight means to Q * 2^-52 (the cross-query sum is a tree on the
device and a left-to-right sum in the reference)."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import cf_reference

pytestmark = pytest.mark.gpu

UNIVERSE = 400


def make_case(Q: int, depth: int, seed: int, all_empty: bool = False):
    """(ranked int64 [Q, depth] with -1 tails, relevant sets): |relevant| cycles 0, 1, 3, 150; every third list is cut to 5
    valid entries, every seventh to none."""
    rng = random.Random(seed)
    ranked = np.full((Q, depth), -1, np.int64)
    relevant = []
    for q in range(Q):
        n_valid = 0 if q % 7 == 6 else (min(5, depth) if q % 3 == 2 else depth)
        ranked[q, :n_valid] = rng.sample(range(UNIVERSE), n_valid)
        relevant.append(set() if all_empty else set(rng.sample(range(UNIVERSE), (0, 1, 3, 150)[q % 4])))
    return ranked, relevant


def run_device(ranked, relevant):
    import torch

    from instacart_next_order_recommendation_amd.ir_metrics import ir_metrics_rows_raw, metrics_from_sums

    off = np.zeros(len(relevant) + 1, np.int64)
    np.cumsum([len(r) for r in relevant], out=off[1:])
    rows = np.asarray([p for r in relevant for p in sorted(r)], np.int64)
    sums, pq = ir_metrics_rows_raw(torch.from_numpy(ranked).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(rows).cuda(),
                                   per_query=True)
    sums = sums.cpu().numpy()
    return sums, pq.cpu().numpy(), metrics_from_sums(sums)


def check(ranked, relevant):
    sums, pq, means = run_device(ranked, relevant)
    Q = len(relevant)
    want = [cf_reference.query_metrics(ranked[q].tolist(), relevant[q]) for q in range(Q)]
    assert sums[8] == sum(1 for w in want if w is not None)
    for q, w in enumerate(want):
        w = [0.0] * 8 if w is None else w
        assert pq[q].tolist() == w, (q, pq[q].tolist(), w)     # bit-equal: == on doubles
    want_means = cf_reference.ir_metrics({q: ranked[q].tolist() for q in range(Q)}, dict(enumerate(relevant)))
    for key in cf_reference.METRIC_KEYS:
        assert abs(means[key] - want_means[key]) <= Q * 2.0 ** -52, key
    return sums, pq, means


# ir_reduce_kernel's thread t adds queries t, t + 1024, ...: from 1,025 queries on some threads add a second value, at
# 2,500 some a third and some only two (depth 10 and 128 only there: the reference is a Python loop)
@pytest.mark.parametrize("depth,Q", [(depth, Q) for Q in (1, 65, 1000) for depth in (1, 10, 100, 128)]
                         + [(depth, Q) for Q in (1024, 1025, 2500) for depth in (10, 128)])
def test_metrics_match_reference(Q, depth):
    ranked, relevant = make_case(Q, depth, seed=Q * 131 + depth)
    if Q == 1:
        relevant = [{int(ranked[0, 0]), 7, 9}]     # the only query counts
    check(ranked, relevant)


def test_all_relevant_sets_empty_gives_zeros():
    ranked, relevant = make_case(65, 10, seed=1, all_empty=True)
    sums, pq, means = check(ranked, relevant)
    assert sums.tolist() == [0.0] * 9 and not pq.any() and means == {k: 0.0 for k in cf_reference.METRIC_KEYS}


def test_hit_at_rank_11_counts_for_map_only():
    ranked = np.arange(100, 228, dtype=np.int64)[None, :100].copy()
    _, pq, _ = check(ranked, [{110, 399}])                     # 110 sits at rank 11
    assert pq[0, :7].tolist() == [0.0] * 7 and pq[0, 7] == (1 / 11) / 2


def test_hit_at_rank_101_counts_for_nothing():
    ranked = np.arange(100, 228, dtype=np.int64)[None, :].copy()
    sums, pq, _ = check(ranked, [{200}])                       # 200 sits at rank 101 of 128
    assert pq[0].tolist() == [0.0] * 8 and sums[8] == 1.0


def test_short_lists_and_large_relevant_sets():
    ranked = np.full((3, 128), -1, np.int64)
    ranked[0, :5] = [4, 8, 15, 16, 23]
    ranked[2, :128] = np.arange(128)
    relevant = [{8, 23, 42}, {1}, set(range(0, 300, 2))]       # 5 valid entries; no valid entry; |relevant| = 150
    _, pq, _ = check(ranked, relevant)
    assert pq[0, 7] == (1 / 2 + 2 / 5) / 3 and pq[1].tolist() == [0.0] * 8
    assert pq[2, 4] == 5 / 150 and pq[2, 0] == 1.0


def test_two_runs_give_identical_bits():
    for Q in (1000, 2500):   # 2,500: the threads of ir_reduce_kernel add two or three values each
        ranked, relevant = make_case(Q, 100, seed=5)
        a, b = run_device(ranked, relevant), run_device(ranked, relevant)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_compute_ir_metrics_on_id_strings():
    from instacart_next_order_recommendation_amd.ir_metrics import compute_ir_metrics

    rankings = {"q1": ["a", "b", "c"], "q2": ["c", "x"], "q3": ["b"], "q4": []}
    relevant = {"q1": {"c", "zz"}, "q2": {"c"}, "q3": set(), "q5": {"a"}, "q4": {"a"}}
    got, want = compute_ir_metrics(rankings, relevant), cf_reference.ir_metrics(rankings, relevant)
    for key in cf_reference.METRIC_KEYS:
        assert abs(got[key] - want[key]) <= 3 * 2.0 ** -52, key
    assert compute_ir_metrics({"q3": ["b"]}, relevant) == {k: 0.0 for k in cf_reference.METRIC_KEYS}


def test_content_based_evaluate_equals_metrics_of_rank_all(tmp_path):
    from instacart_next_order_recommendation_amd import synthetic as syn
    from instacart_next_order_recommendation_amd.baselines import ContentBasedBaseline
    from instacart_next_order_recommendation_amd.ir_metrics import compute_ir_metrics
    from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir

    model_dir = write_synthetic_model_dir(tmp_path / "m", seed=6)
    corpus = syn.synthetic_catalog(300)
    queries = {f"order{i}": q for i, q in enumerate(syn.synthetic_user_contexts(37, seed=8))}
    cb = ContentBasedBaseline(queries, corpus, model_dir)
    rng = random.Random(2)
    pids = list(corpus)
    relevant = {q: set(rng.sample(pids, rng.randint(1, 40))) for q in queries}
    got = cb.evaluate(relevant)
    want = compute_ir_metrics(cb.rank_all(depth=100), relevant)
    assert got == want and got["accuracy_at_10"] > 0
    ref = cf_reference.ir_metrics(cb.rank_all(depth=100), relevant)
    for key in cf_reference.METRIC_KEYS:
        assert abs(got[key] - ref[key]) <= len(queries) * 2.0 ** -52, key
    rows, qids = cb.rank_rows(depth=10, queries_per_pass=16)
    assert qids == list(queries) and tuple(rows.shape) == (37, 10)
