"""icrec_compose_queries on the GPU against tests/compose_reference.py: every comparison is on the bits.  The shapes are
the smallest that reach each path of the kernel - U = 8 stored rows in flight per thread, so term counts 0, 1, U, U + 1,
2U + 1 and a longer list cut by max_terms, and 255, 256, 257, 1,024 and a cut 1,030 at max_terms = ICREC_MAX_TERMS, where
the 256 threads stage a segment in several passes; 16-byte pieces of 4 fp32 or 8 bf16 values over 256 threads, so dims 32 (a
few lanes own a piece), 96 (fp32 only), 384 and 4,096 (a thread walks several pieces); 1, 5 and 1,025 queries - with
term rows and weights the host would refuse, a reversed segment, shards, index edits, the search behind it and a
captured graph."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from instacart_next_order_recommendation_amd import _native
from instacart_next_order_recommendation_amd.search import DeviceIndex, apply_moves, removal_moves
from oracle import oracle
from tests import compose_reference as ref
from tests.search_harness import assert_search, torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

U = 8  # compose.hip's COMPOSE_DEPTH
N_ROWS = 300
INT32_MAX = 2**31 - 1
LENGTHS = (0, 1, U, U + 1, 2 * U + 1, 30)  # the last is cut by max_terms = 2U + 1
MAX_TERMS = 2 * U + 1
STORAGES = ("f32", "bf16", "f32+filter", "bf16+filter")
CASES = [(32, "f32"), (96, "f32")] + [(dim, s) for dim in (384, 4096) for s in STORAGES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def draw_terms(rng, n_rows, Q):
    """A CSR of Q segments whose lengths cycle through LENGTHS, every 11th one reversed (its end 3 entries before its
    start), over rows and weights that include what the host refuses: rows -1, n_rows and INT32_MAX, a row repeated,
    weights NaN, +inf, -inf, 0 and negative."""
    off = [0]
    for i in range(Q):
        off.append(off[-1] - 3 if i % 11 == 7 and off[-1] >= 3 else off[-1] + LENGTHS[i % len(LENGTHS)])
    nnz = max(off) + 1
    rows = rng.integers(0, n_rows, nnz).astype(np.int32)
    w = rng.uniform(-1.5, 1.5, nnz).astype(np.float32)
    rows[3::13], rows[5::17], rows[7::19] = -1, n_rows, INT32_MAX
    rows[2::23] = rows[1::23][:rows[2::23].size]  # the same row twice in a row
    w[4::13], w[6::17], w[8::19], w[9::7] = np.nan, np.inf, -np.inf, 0.0
    return np.asarray(off, np.int32), rows, w


def draw_base(rng, Q, dim):
    """Q rows of any norm, every 9th all zero, and weights a that cycle through 1, 0, -1, inf, 0.5, NaN."""
    base = (rng.standard_normal((Q, dim)) * rng.uniform(0.1, 30.0, (Q, 1))).astype(np.float32)
    base[4::9] = 0.0
    a = np.resize(np.array([1.0, 0.0, -1.0, np.inf, 0.5, np.nan], np.float32), Q)
    return base, a


def run(ix, base, base_w, off, rows, w, max_terms):
    """icrec_compose_queries through DeviceIndex.compose_queries_into on a CSR built here -> numpy [Q, dim]."""
    dev = ix.device

    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    out = torch.full((len(off) - 1, ix.dim), -7.0, dtype=torch.float32, device=dev)
    ix.compose_queries_into(up(base), up(base_w), up(off), up(rows), up(w), max_terms, out)
    return out.cpu().numpy()


def assert_bits(got, want):
    np.testing.assert_array_equal(bits(got), bits(want))


@pytest.mark.parametrize("dim,storage", CASES, ids=[f"{d}-{s}" for d, s in CASES])
def test_bit_equal_for_every_dim_storage_and_batch_size(torch_cuda, dim, storage):
    rng = np.random.default_rng(dim + len(storage))
    P = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    p_hat = ref.stored_rows(P, storage)
    ix = DeviceIndex(P, storage=storage)
    try:
        Q = 1025
        off, rows, w = draw_terms(rng, N_ROWS, Q)
        base, a = draw_base(rng, Q, dim)
        want = ref.compose(p_hat, base, a, off, rows, w, MAX_TERMS)
        assert np.isfinite(want).all()
        assert_bits(run(ix, base, a, off, rows, w, MAX_TERMS), want)
        # the same bits alone and in a batch of 5 (the CSR of a sub-batch is a slice of the offsets: they are absolute)
        for lo, n in ((5, 1), (7, 1), (16, 1), (0, 5), (6, 5)):
            got = run(ix, base[lo:lo + n], a[lo:lo + n], off[lo:lo + n + 1], rows, w, MAX_TERMS)
            assert_bits(got, want[lo:lo + n])
        # base_w NULL: every a = 1; weights NULL: every w = 1; no base: the terms alone, from +0
        assert_bits(run(ix, base[:5], None, off[:6], rows, w, MAX_TERMS), ref.compose(p_hat, base[:5], None, off[:6], rows, w, MAX_TERMS))
        assert_bits(run(ix, base[:5], a[:5], off[:6], rows, None, MAX_TERMS), ref.compose(p_hat, base[:5], a[:5], off[:6], rows, None, MAX_TERMS))
        for n in (1, 5, 13):
            want_terms = ref.compose(p_hat, None, None, off[:n + 1], rows, w, MAX_TERMS)
            assert_bits(run(ix, None, None, off[:n + 1], rows, w, MAX_TERMS), want_terms)
        assert not want_terms[0].any() and want_terms[1].any()  # (a query without terms is the zero vector)
        # max_terms = 0 with a base: a * q_hat alone; max_terms cutting at 1 and at U
        assert_bits(run(ix, base[:13], a[:13], off[:14], None, None, 0), ref.compose(p_hat, base[:13], a[:13], off[:14], rows, w, 0))
        for cut in (1, U):
            assert_bits(run(ix, base[:13], a[:13], off[:14], rows, w, cut), ref.compose(p_hat, base[:13], a[:13], off[:14], rows, w, cut))
        # one term of weight 1 without a base is the stored row, whatever the storage
        one = run(ix, None, None, np.array([0, 1, 2], np.int32), np.array([N_ROWS - 1, 17], np.int32), None, 1)
        assert_bits(one, p_hat[[N_ROWS - 1, 17]])
        assert_bits(ix.export().cpu().numpy()[[N_ROWS - 1, 17]], one)
    finally:
        ix.close()


LIMIT_LENGTHS = (255, 256, 257, _native.ICREC_MAX_TERMS, _native.ICREC_MAX_TERMS + 6)  # the last is cut by max_terms


@pytest.mark.parametrize("dim,storage", [(32, "f32"), (384, "f32"), (384, "bf16")], ids=["32-f32", "384-f32", "384-bf16"])
def test_bit_equal_at_the_term_limit(torch_cuda, dim, storage):
    """max_terms = ICREC_MAX_TERMS: the kernel's 256 threads stage a segment and the pad behind it in a second pass
    that holds only the pad (255, 256 terms) or its last term too (257), and in five passes (1,024 terms and the cut
    1,030); a chain is up to 1,024 terms long."""
    rng = np.random.default_rng(dim + 7 * len(storage))
    P = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    p_hat = ref.stored_rows(P, storage)
    limit = _native.ICREC_MAX_TERMS
    assert limit == 1024 and LIMIT_LENGTHS == (255, 256, 257, 1024, 1030)
    off = np.concatenate([[0], np.cumsum(LIMIT_LENGTHS)]).astype(np.int32)
    Q, nnz = len(LIMIT_LENGTHS), int(off[-1])
    rows = rng.integers(0, N_ROWS, nnz).astype(np.int32)
    w = rng.uniform(-1.5, 1.5, nnz).astype(np.float32)
    rows[3::13], rows[5::17], rows[7::19] = -1, N_ROWS, INT32_MAX
    w[4::13], w[6::17], w[8::19], w[9::7] = np.nan, np.inf, -np.inf, 0.0
    for i, n in enumerate(LIMIT_LENGTHS):  # a term that does not count at the edges of the staging passes and of the limit
        if n > 255:
            rows[off[i] + 255] = -1
        if n > 256:
            rows[off[i] + 256], w[off[i] + 256] = 11, np.nan
        if n > 1023:
            rows[off[i] + 1023] = N_ROWS
    rows[off[Q - 1] + limit:off[Q]] = rng.integers(0, N_ROWS, 6)  # behind the limit: terms that would count, with weights
    w[off[Q - 1] + limit:off[Q]] = 100.0                          # .. nothing could hide
    counted = [sum(ref.term_valid(rows[t], w[t], N_ROWS) for t in range(off[i], min(off[i + 1], off[i] + limit))) for i in range(Q)]
    assert min(counted) > 150 and counted[4] > 600
    base, a = draw_base(rng, Q, dim)
    a[:] = [1.0, 0.0, -1.0, 0.5, 1.0]
    ix = DeviceIndex(P, storage=storage)
    try:
        want = ref.compose(p_hat, base, a, off, rows, w, limit)
        assert np.isfinite(want).all()
        assert (bits(want[4]) != bits(ref.compose(p_hat, base[4:], a[4:], off[4:], rows, w, limit + 6)[0])).any()  # the cut shows
        assert_bits(run(ix, base, a, off, rows, w, limit), want)
        for i in range(Q):  # the same bits alone
            assert_bits(run(ix, base[i:i + 1], a[i:i + 1], off[i:i + 2], rows, w, limit), want[i:i + 1])
        assert_bits(run(ix, None, None, off, rows, w, limit), ref.compose(p_hat, None, None, off, rows, w, limit))
    finally:
        ix.close()


def test_the_filter_storages_give_the_plain_storages_bits(torch_cuda):
    rng = np.random.default_rng(3)
    P = rng.standard_normal((N_ROWS, 384)).astype(np.float32)
    off, rows, w = draw_terms(rng, N_ROWS, 40)
    base, a = draw_base(rng, 40, 384)
    got = {}
    for storage in STORAGES:
        ix = DeviceIndex(P, storage=storage)
        try:
            got[storage] = run(ix, base, a, off, rows, w, MAX_TERMS)
        finally:
            ix.close()
    assert_bits(got["f32+filter"], got["f32"])
    assert_bits(got["bf16+filter"], got["bf16"])
    assert (bits(got["bf16"]) != bits(got["f32"])).any()


@pytest.mark.parametrize("storage", ["f32+filter", "bf16"])
def test_terms_are_local_rows_and_the_search_takes_the_composed_query(torch_cuda, storage):
    rng = np.random.default_rng(17)
    dim, Q, k, row_offset = 384, 6, 20, 1000
    P = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    p_hat = ref.stored_rows(P, storage)
    ix = DeviceIndex(P, row_offset=row_offset, storage=storage)
    try:
        base = rng.standard_normal((Q, dim)).astype(np.float32)
        terms = [None, [(5, 1.0)], {9: 0.5, 3: 0.5, 200: -0.25}, [(299, 1.0), (299, 1.0), (0, -1.0)],
                 [(int(r), 1.0 / 12) for r in rng.integers(0, N_ROWS, 12)], [(7, -1.0)]]
        want = ref.compose_lists(p_hat, base, terms, [1.0, 0.0, 1.0, 0.5, 2.0, 1.0])
        got = ix.compose_queries(base, terms, [1.0, 0.0, 1.0, 0.5, 2.0, 1.0])
        assert_bits(got.cpu().numpy(), want)
        kind = "bf16" if storage.startswith("bf16") else "f32"
        assert_search(ix.search(got, k), oracle.search(want, P, k, row_offset=row_offset, storage=kind))
        # "similar items": the row itself comes first, and excluded it is gone
        idx, _ = ix.search(got[1:2], k)
        assert idx[0, 0].item() == row_offset + 5
        idx, _ = ix.search(got[1:2], k, [[5]])
        assert row_offset + 5 not in idx.cpu().numpy()
        # without a base, and a zero result: a legal query, every score 0, the lowest rows
        profile = ix.compose_queries(None, terms)
        assert_bits(profile.cpu().numpy(), ref.compose_lists(p_hat, None, terms))
        idx, sc = ix.search(profile[:1], 4)
        assert idx.cpu().numpy().tolist() == [[row_offset + i for i in range(4)]] and not sc.cpu().numpy().any()
        # one base weight for all queries, and a single [dim] base
        assert_bits(ix.compose_queries(base, terms, 0.5).cpu().numpy(), ref.compose_lists(p_hat, base, terms, [0.5] * Q))
        assert_bits(ix.compose_queries(base[2], [terms[2]]).cpu().numpy(), ref.compose_lists(p_hat, base[2:3], [terms[2]]))
    finally:
        ix.close()


@pytest.mark.parametrize("storage", ["f32", "bf16+filter"])
def test_after_index_edits_on_the_same_handle(torch_cuda, storage):
    rng = np.random.default_rng(23)
    dim = 384
    M = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    ix = DeviceIndex(M, storage=storage)
    try:
        def check():
            n = ix.n_rows
            assert n == M.shape[0]
            off, rows, w = draw_terms(rng, n, 24)
            rows[0], rows[1] = n - 1, n  # the last row counts, the one behind it does not
            base, a = draw_base(rng, 24, dim)
            assert_bits(run(ix, base, a, off, rows, w, MAX_TERMS), ref.compose(ref.stored_rows(M, storage), base, a, off, rows, w, MAX_TERMS))

        check()
        ids = [299, 3, 150]
        new = (rng.standard_normal((3, dim)) * 4).astype(np.float32)
        ix.write_rows(ids, new)
        M[ids] = new
        check()
        extra = rng.standard_normal((400, dim)).astype(np.float32)
        ix.append_rows(extra)  # past the capacity: every pointer of the handle changes
        assert ix.capacity > N_ROWS
        M = np.concatenate([M, extra])
        check()
        gone = [0, 5, 699, 350]
        dst, src = ix.remove_rows(gone)
        new_n, want_dst, want_src = removal_moves(M.shape[0], gone)
        assert dst.tolist() == want_dst.tolist() and src.tolist() == want_src.tolist()
        M = apply_moves(M, new_n, dst, src)
        check()
    finally:
        ix.close()


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_a_captured_graph_follows_the_rewritten_lists(torch_cuda, storage):
    rng = np.random.default_rng(31)
    dim, Q = 384, 12
    P = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    p_hat = ref.stored_rows(P, storage)
    ix = DeviceIndex(P, storage=storage)
    try:
        dev = ix.device
        off, rows, w = draw_terms(rng, N_ROWS, Q)
        base, a = draw_base(rng, Q, dim)
        d = {name: torch.from_numpy(v).to(dev) for name, v in (("base", base), ("a", a), ("off", off), ("rows", rows), ("w", w))}
        out = torch.zeros((Q, dim), dtype=torch.float32, device=dev)
        ix.compose_queries_into(d["base"], d["a"], d["off"], d["rows"], d["w"], MAX_TERMS, out)  # first launch outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ix.compose_queries_into(d["base"], d["a"], d["off"], d["rows"], d["w"], MAX_TERMS, out)
        out.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        assert_bits(out.cpu().numpy(), ref.compose(p_hat, base, a, off, rows, w, MAX_TERMS))
        # new lists, weights, offsets and bases in the same buffers
        rows2 = np.roll(rows, 5)
        w2 = np.roll(w, 3)
        off2 = np.minimum(off + 2, rows.size - 1).astype(np.int32)
        base2, a2 = draw_base(rng, Q, dim)
        for name, v in (("base", base2), ("a", a2), ("off", off2), ("rows", rows2), ("w", w2)):
            d[name].copy_(torch.from_numpy(v))
        want = ref.compose(p_hat, base2, a2, off2, rows2, w2, MAX_TERMS)
        assert (bits(want) != bits(out.cpu().numpy())).any()
        g.replay()
        torch.cuda.synchronize()
        assert_bits(out.cpu().numpy(), want)
    finally:
        ix.close()
