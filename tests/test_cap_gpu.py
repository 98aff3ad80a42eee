"""icrec_cap_select on the GPU against tests/cap_reference.py, bit for bit - indices, score bits, state and the next
masks - on a 600 x 64 index in fp32 and bf16 storage, at row offsets 0 and 1,000, with one and two facets: 1, 5 and 257
queries, k at the lane edges of the wave (1, 2, 63, 64, 65, 127, 128), top_k 1, k / 2 and k, facet values at the
mask-word edges (0, 31, 32, 255), caps from -5 to 2^31 - 1, prior counts inside and outside [0, top_k], lists with
pads in the middle and at the tail, rows of other shards, a row twice and lists of one value; allow_dev NULL, given,
and aliased with allow_next_dev; sentinels around every output."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import cap_reference as ref
from tests.search_harness import DeviceIndex, _native, torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N, DIM, GUARD = 600, 64, 64
KS = (1, 2, 63, 64, 65, 127, 128)
CAPS = (-5, 0, 1, 2, 127, 128, 2**31 - 1)
VALUES = np.array([0, 31, 32, 255, 7, 200], np.uint8)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def facets():
    """uint8 [600, 2] over six values, the mask-word edges among them; rows 0 .. 149 are all (31, 255)."""
    rng = np.random.default_rng(41)
    F = VALUES[rng.integers(0, VALUES.size, (N, 2))]
    F[:150] = (31, 255)
    F.flags.writeable = False
    return F


def candidate_lists(rng, Q, k, off):
    """Lists of valid rows with, dealt by the query number: a pad in the middle, pads at the tail, rows of other
    shards (below the offset, past the last row, far away), one row twice, all candidates of one value."""
    cand = off + rng.integers(0, N, (Q, k))
    for q in range(Q):
        kind = q % 7
        if kind == 1:
            cand[q, rng.integers(0, k)] = -1 if q % 2 else -9
        elif kind == 2:
            cand[q, k - int(rng.integers(0, k)) - 1:] = -1
        elif kind == 3:
            j = rng.integers(0, k, 3)
            cand[q, j] = [off + N, off - 1 if off else 1 << 40, off + N + 5000]
        elif kind == 4:
            cand[q, rng.integers(0, k)] = cand[q, 0]
        elif kind == 5:
            cand[q] = off + rng.permutation(150)[:k]  # distinct rows of (31, 255)
        elif kind == 6:
            cand[q] = off + rng.permutation(N)[:k]  # distinct rows, no pad: done only at top_k picks
    return cand.astype(np.int64)


def guarded(n, dtype, fill):
    """A device buffer of n elements between two guard zones of `fill` -> (whole buffer, the n elements)."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def run_case(ix, F, rng, Q, k, top_k, mode):
    """One launch against the reference.  mode 0: allow NULL, 1: allow given, 2: allow aliased with allow_next,
    3: allow given and no allow_next."""
    off, nf = ix.row_offset, ix.n_facets
    cand = candidate_lists(rng, Q, k, off)
    score = rng.standard_normal((Q, k)).astype(np.float32)
    score[:, ::5] = -0.0
    caps = rng.choice(CAPS, (Q, 2)).astype(np.int32)
    n_prior = rng.choice([0, 1, top_k - 1, top_k, -3, top_k + 7], Q).astype(np.int32)
    prior_idx = (off + rng.integers(0, N, (Q, top_k))).astype(np.int64)
    prior_idx[rng.random((Q, top_k)) < 0.1] = -1
    prior_idx[rng.random((Q, top_k)) < 0.1] = off + N + 3
    prior_sc = rng.standard_normal((Q, top_k)).astype(np.float32)
    allow = rng.integers(0, 2**32, (Q, nf, 8), dtype=np.uint64).astype(np.uint32) if mode else None
    want = ref.cap_select(F[:, :nf], cand, score, caps, top_k, n_prior, prior_idx, prior_sc, allow, off)

    dev = ix.device
    d_cand, d_score = torch.from_numpy(cand).to(dev), torch.from_numpy(score).to(dev)
    d_caps, d_prior = torch.from_numpy(caps).to(dev), torch.from_numpy(n_prior).to(dev)
    w_idx, o_idx = guarded(Q * top_k, torch.int64, -77)
    w_sc, o_sc = guarded(Q * top_k, torch.float32, 77.0)
    w_st, o_st = guarded(Q * 2, torch.int32, -77)
    w_nx, o_nx = guarded(Q * nf * 8, torch.int32, -77)
    o_idx.copy_(torch.from_numpy(prior_idx).reshape(-1))
    o_sc.copy_(torch.from_numpy(prior_sc).reshape(-1))
    d_allow = None
    if mode == 2:
        o_nx.copy_(torch.from_numpy(allow.view(np.int32)).reshape(-1))
        d_allow = o_nx.view(torch.uint32)
    elif mode:
        d_allow = torch.from_numpy(allow.view(np.int32)).to(dev).view(torch.uint32)
    _native.cap_select(ix._h, d_cand, d_score, d_caps, d_prior, d_allow, top_k, o_idx, o_sc, o_st,
                       None if mode == 3 else o_nx.view(torch.uint32), dev)
    torch.cuda.synchronize()
    what = (Q, k, top_k, mode)
    np.testing.assert_array_equal(o_idx.cpu().numpy().reshape(Q, top_k), want[0], err_msg=str(what))
    np.testing.assert_array_equal(bits(o_sc.cpu().numpy().reshape(Q, top_k)), bits(want[1]), err_msg=str(what))
    np.testing.assert_array_equal(o_st.cpu().numpy().reshape(Q, 2), want[2], err_msg=str(what))
    if mode == 3:
        assert (o_nx == -77).all()
    else:
        np.testing.assert_array_equal(o_nx.cpu().numpy().view(np.uint32).reshape(Q, nf, 8), want[3], err_msg=str(what))
    for whole, fill in ((w_idx, -77), (w_sc, 77.0), (w_st, -77), (w_nx, -77)):  # nothing is written outside an output
        assert (whole[:GUARD] == fill).all() and (whole[-GUARD:] == fill).all(), what
    np.testing.assert_array_equal(d_cand.cpu().numpy(), cand)  # the inputs are read only
    np.testing.assert_array_equal(bits(d_score.cpu().numpy()), bits(score))
    np.testing.assert_array_equal(d_caps.cpu().numpy(), caps)
    if mode in (1, 3):
        np.testing.assert_array_equal(d_allow.view(torch.int32).cpu().numpy().view(np.uint32), allow)
    return want


@pytest.mark.parametrize("n_facets", [1, 2])
@pytest.mark.parametrize("row_offset", [0, 1000])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_against_the_reference(torch_cuda, facets, storage, row_offset, n_facets):
    rng = np.random.default_rng(7 + row_offset + n_facets)
    P = rng.standard_normal((N, DIM)).astype(np.float32)
    ix = DeviceIndex(P, row_offset=row_offset, storage=storage)
    ix.set_facets(np.ascontiguousarray(facets[:, :n_facets]))
    seen_states, case = set(), 0
    for Q in (1, 5, 257):
        for k in KS:
            for top_k in sorted({1, max(k // 2, 1), k}):
                want = run_case(ix, facets, rng, Q, k, top_k, case % 4)
                seen_states |= {tuple(s) for s in want[2][:, 1:].tolist()}
                case += 1
    assert seen_states == {(0,), (1,)}  # lists that were done and lists that were not
    run_case(ix, facets, rng, 5, 5, 128, 1)  # top_k may exceed k: a continuation round at a narrow width
    ix.close()


def test_hand_case_and_every_value_of_one_aisle(torch_cuda, facets):
    """Rows 0 .. 149 are one (aisle, department): cap 2 keeps the list's first two and closes exactly that value."""
    ix = DeviceIndex(np.random.default_rng(1).standard_normal((N, DIM)).astype(np.float32))
    ix.set_facets(np.ascontiguousarray(facets))
    cand = torch.arange(128, dtype=torch.int64, device=ix.device)[None, :].flip(1).contiguous()
    sc = torch.linspace(1, 0, 128, device=ix.device)[None, :].contiguous()
    idx, out, state, nxt = ix.cap_select(cand, sc, (2, None), 5)
    assert idx.tolist() == [[127, 126, -1, -1, -1]] and state.tolist() == [[2, 0]]
    assert bits(out.cpu().numpy()).tolist() == bits(np.array([[sc[0, 0].item(), sc[0, 1].item(), 0, 0, 0]], np.float32)).tolist()
    words = nxt.view(torch.int32).cpu().numpy().view(np.uint32)
    assert words[0, 0, 0] == 0x7FFFFFFF and (words[0, 0, 1:] == 0xFFFFFFFF).all() and (words[0, 1] == 0xFFFFFFFF).all()
    idx, _, state, nxt = ix.cap_select(cand, sc, (None, 3), 5)
    assert idx.tolist() == [[127, 126, 125, -1, -1]] and state.tolist() == [[3, 0]]
    words = nxt.view(torch.int32).cpu().numpy().view(np.uint32)
    assert words[0, 1, 7] == 0x7FFFFFFF and (words[0, 0] == 0xFFFFFFFF).all()
    with pytest.raises(ValueError, match="caps"):
        ix.cap_select(cand, sc, (1, 2, 3), 5)
    ix.set_facets(None)
    with pytest.raises(_native.IcrecError, match="no facets"):
        ix.cap_select(cand, sc, (2, None), 5)
    ix.close()


def test_a_query_alone_equals_the_query_in_a_batch(torch_cuda, facets):
    rng = np.random.default_rng(5)
    ix = DeviceIndex(rng.standard_normal((N, DIM)).astype(np.float32))
    ix.set_facets(np.ascontiguousarray(facets))
    cand = torch.from_numpy(candidate_lists(rng, 70, 100, 0)).to(ix.device)
    sc = torch.from_numpy(rng.standard_normal((70, 100)).astype(np.float32)).to(ix.device)
    caps = rng.choice([1, 2, 3], (70, 2))
    batch = [t.cpu() for t in ix.cap_select(cand, sc, caps, 40)]
    for q in (0, 33, 69):
        alone = ix.cap_select(cand[q:q + 1], sc[q:q + 1], caps[q:q + 1], 40)
        for a, b in zip(alone, batch):
            assert torch.equal(a.cpu().view(torch.int32), b[q:q + 1].view(torch.int32))
    ix.close()


def test_captured_launch_follows_the_caps_buffer(torch_cuda, facets):
    rng = np.random.default_rng(6)
    ix = DeviceIndex(rng.standard_normal((N, DIM)).astype(np.float32))
    ix.set_facets(np.ascontiguousarray(facets))
    cand_h = candidate_lists(rng, 3, 64, 0)
    sc_h = rng.standard_normal((3, 64)).astype(np.float32)
    cand, sc = torch.from_numpy(cand_h).to(ix.device), torch.from_numpy(sc_h).to(ix.device)
    caps = torch.zeros((3, 2), dtype=torch.int32, device=ix.device)
    out_idx = torch.empty((3, 20), dtype=torch.int64, device=ix.device)
    out_sc = torch.empty((3, 20), dtype=torch.float32, device=ix.device)
    state = torch.empty((3, 2), dtype=torch.int32, device=ix.device)
    nxt = torch.empty((3, 2, 8), dtype=torch.int32, device=ix.device).view(torch.uint32)

    def launch():
        ix.cap_select_into(cand, sc, caps, 20, out_idx, out_sc, state, allow_next=nxt)

    launch()  # first launch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    lists = []
    for pair in ((1, 0), (0, 2)):
        caps.copy_(torch.tensor([pair] * 3, dtype=torch.int32))
        out_idx.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        want = ref.cap_select(facets, cand_h, sc_h, pair, 20)
        np.testing.assert_array_equal(out_idx.cpu().numpy(), want[0])
        np.testing.assert_array_equal(bits(out_sc.cpu().numpy()), bits(want[1]))
        np.testing.assert_array_equal(state.cpu().numpy(), want[2])
        np.testing.assert_array_equal(nxt.view(torch.int32).cpu().numpy().view(np.uint32), want[3])
        lists.append(want[0])
    assert not np.array_equal(lists[0], lists[1])
    ix.close()
