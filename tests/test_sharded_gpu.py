"""The whole N>1 product path on the one-GPU box: two ranks (both on cuda:0, gloo rendezvous) run the
real HipShardBackend + ShardedSearch and bench.py's multi-rank flow."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.search_harness import (DeviceIndex, HipShardBackend, NativeComm, ShardedSearch, assert_ranked_lists,
                                  assert_search, bench_catalog, bench_queries, csr_restatement, exclusions_to_shard_csr,
                                  local_exclusions, merge_topk, oracle, redrawn_exclusions, shard_bounds,
                                  sharded_partial_keys, synthetic as syn)

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

WORKER = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["ICREC_ROOT"])
from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.sharded import HipShardBackend, ShardedSearch, shard_bounds
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda:0")
P = syn.synthetic_embeddings(3001, 384, seed=1)
q = syn.synthetic_embeddings(8, 384, seed=2)
b = shard_bounds(3001, world)
lo, hi = b[rank], b[rank + 1]
excl = [[(7 * i) % 3001, 5, 2999] for i in range(8)]
ss = ShardedSearch(HipShardBackend(torch.from_numpy(P[lo:hi]).to(dev), lo, dev), lo, hi)
per = 8 // world
idx, sc = ss.search(torch.from_numpy(q[rank * per:(rank + 1) * per]).to(dev), 20, excl)
np.savez(os.path.join(os.environ["ICREC_OUT"], f"r{rank}.npz"), idx=idx.cpu().numpy(), sc=sc.cpu().numpy())
dist.destroy_process_group()
"""


def _torchrun(args, env_extra, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29517"] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_two_ranks_real_kernels_equal_unsharded(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    r = _torchrun([str(script)], {"ICREC_ROOT": str(ROOT), "ICREC_OUT": str(tmp_path)})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    P = syn.synthetic_embeddings(3001, 384, seed=1)
    q = syn.synthetic_embeddings(8, 384, seed=2)
    excl = [[(7 * i) % 3001, 5, 2999] for i in range(8)]
    wi, ws = oracle.search(q, P, 20, excl)
    for rank in range(2):
        got = np.load(tmp_path / f"r{rank}.npz")
        np.testing.assert_array_equal(got["idx"], wi)
        np.testing.assert_array_equal(got["sc"], ws)


def test_bench_multi_rank_flow_rehearsal(tmp_path):
    """The BARE form the driver uses, `python bench.py --gpus 2 ...` without a launcher: bench.py starts its own two
    ranks as a fresh child (torch.distributed.run), relays rank 0's line and exits with the child's code.  Rehearsal
    mode: both ranks on cuda:0, gloo.  With --full the line carries the configs[4] leg (here 300,000 rows instead of
    10 M) and the verdict of the exchange check, exclusion exchange included.  --dump-outputs: rank 0 writes the timed
    step's outputs for the whole gathered batch, both ranks' query embeddings in rank order."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", ICREC_BENCH_REHEARSAL="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "64",
                        "--rows-10m", "300000", "--dump-outputs", str(tmp_path / "dump"), "--full"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0 and d["rehearsal_not_a_measurement"]
    assert d["config"]["contexts_per_gpu_per_step"] == 64
    assert d["exchange_verified"] is True and d["exclusion_exchange_verified"] is True
    leg = d["configs4_10m_rows"]
    assert leg["queries_per_step"] == 4096 and leg["contexts_encoded_per_gpu"] == 2048 and leg["rows_per_gpu"] == 150000
    assert leg["result_properties_ok"] and leg["qps"] > 0
    assert d["dumped_outputs"]["rows"] == d["dumped_outputs"]["of_rows"] == 128
    emb = np.load(tmp_path / "dump" / "query_embeddings.npy")
    rows = np.load(tmp_path / "dump" / "topk_rows.npy")
    sc = np.load(tmp_path / "dump" / "topk_scores.npy")
    assert emb.shape == (128, 384) and emb.dtype == np.float32
    assert rows.shape == sc.shape == (128, 20) and rows.dtype == np.float64 and sc.dtype == np.float32
    assert ((rows >= 0) & (rows < 49_688) & (rows == np.rint(rows))).all()
    assert np.abs(np.linalg.norm(emb, axis=1) - 1).max() < 1e-5
    assert not np.array_equal(emb[:64], emb[64:])   # rank 1's contexts come from another seed
    P = bench_catalog().astype(np.float64)  # bench.py's catalog: unit rows
    np.testing.assert_allclose(sc, np.einsum("qd,qkd->qk", emb.astype(np.float64), P[rows.astype(np.int64)]), atol=1e-5)


def test_native_rccl_world1_equals_plain_search():
    """icrec_comm_init (a real ncclCommInitRank on one rank) + icrec_search_sharded: both ncclAllGathers run
    on the stream and the result is bit-equal to icrec_search and to the oracle, exclusions included."""
    dev = torch.device("cuda:0")
    P = syn.synthetic_embeddings(6211, 384, seed=1)   # one shard of configs[3] (49,688 / 8 rows)
    q = syn.synthetic_embeddings(512, 384, seed=2)    # 4,096 / 8 queries
    excl = [[(13 * i) % 6211, 5, 6210] if i % 3 == 0 else [] for i in range(512)]
    comm = NativeComm(0, 1, dev, NativeComm.unique_id())
    assert comm.world == 1 and comm.rank == 0
    be = HipShardBackend(torch.from_numpy(P).to(dev), 0, dev)
    ss = ShardedSearch(be, 0, 6211, comm=comm)
    qd = torch.from_numpy(q).to(dev)
    for ex in (None, excl):
        idx, sc = ss.search(qd, 20, ex)
        pi, ps = be.index.search(qd, 20, ex)
        assert torch.equal(idx, pi) and torch.equal(sc, ps)
        assert_search((idx, sc), oracle.search(q, P, 20, ex))
    # a shard with a row offset: global rows come back
    be2 = HipShardBackend(torch.from_numpy(P[1000:3000]).to(dev), 1000, dev)
    ss2 = ShardedSearch(be2, 1000, 3000, comm=comm)
    wi2, ws2 = oracle.search(q[:64], P[1000:3000], 20, [[500, 1999]] * 64)
    assert_search(ss2.search(qd[:64], 20, [[1500, 2999, 5]] * 64), (wi2 + 1000, ws2))
    comm.close()


def test_native_per_rank_exclusions_world1():
    """icrec_search_sharded_excl through a real one-rank RCCL communicator: the exclusions arrive as GLOBAL rows of
    this rank's own queries, are all-gathered (offsets + padded ids), cut to the shard and turned into the local
    CSR on the device - same bits as the replicated form and as the oracle, with a row offset."""
    dev = torch.device("cuda:0")
    P = syn.synthetic_embeddings(6211, 384, seed=1)
    q = syn.synthetic_embeddings(512, 384, seed=2)
    comm = NativeComm(0, 1, dev, NativeComm.unique_id())
    lo, hi = 1000, 5000  # the shard holds global rows [1000, 5000): ids outside it belong to other shards
    be = HipShardBackend(torch.from_numpy(P[lo:hi]).to(dev), lo, dev)
    ss = ShardedSearch(be, lo, hi, comm=comm)
    qd = torch.from_numpy(q).to(dev)
    rng = np.random.default_rng(5)
    excl = redrawn_exclusions(rng, 6211, 512, cap=40, none_every=4)
    idx, sc = ss.search(qd, 20, exclude_local=excl, excl_cap=512 * 40)
    ridx, rsc = ss.search(qd, 20, exclude_global=excl)
    assert torch.equal(idx, ridx) and torch.equal(sc, rsc)
    assert_search((idx, sc), oracle.search(q, P[lo:hi], 20, local_exclusions(excl, lo, hi), row_offset=lo))
    # every query excludes its own best hit: the exchange really reaches the kernel
    pi, ps = ss.search(qd, 20)
    best = pi[:, 0].cpu().tolist()
    idx2, _ = ss.search(qd, 20, exclude_local=[[b] for b in best])
    assert not any(b in row for b, row in zip(best, idx2.cpu().tolist()))
    assert torch.equal(idx2[:, :19], pi[:, 1:])
    # no exclusions at all on this rank (other ranks may still have some): zero offsets
    idx3, sc3 = ss.search(qd, 20, exclude_local=[[] for _ in range(512)])
    assert torch.equal(idx3, pi) and torch.equal(sc3, ps)
    comm.close()


def test_configs3_sizes_4096_queries():
    """BASELINE configs[3] at its own sizes on one GPU: (a) 4,096 queries over the whole 49,688-row catalog (filter
    index, 8-query oracle sample, bit-equal to the exact index); (b) the 4,096 gathered queries over ONE
    6,211-row shard (rows 6,211 .. 12,421) through icrec_search_sharded with a one-rank RCCL communicator."""
    dev = torch.device("cuda:0")
    P, q = bench_catalog(), bench_queries(4096, 2)
    qd = torch.from_numpy(q).to(dev)
    Pd = torch.from_numpy(P).to(dev)
    fi = DeviceIndex(Pd, dev, storage="f32+filter")
    ei = DeviceIndex(Pd, dev, storage="f32")
    idx, sc = fi.search(qd, 20)
    xi, xs = ei.search(qd, 20)
    assert torch.equal(idx, xi) and torch.equal(sc, xs)
    sample = [0, 1, 511, 512, 2047, 2048, 4094, 4095]
    assert_search((idx[sample], sc[sample]), oracle.search(q[sample], P, 20))
    b = shard_bounds(49_688, 8)
    assert b[1] - b[0] == 6211
    lo, hi = b[1], b[2]
    comm = NativeComm(0, 1, dev, NativeComm.unique_id())
    be = HipShardBackend(Pd[lo:hi], lo, dev, storage="f32+filter")
    ss = ShardedSearch(be, lo, hi, comm=comm)
    si, s_sc = ss.search(qd, 20)
    assert_search((si[sample], s_sc[sample]), oracle.search(q[sample], P[lo:hi], 20, row_offset=lo))
    # shard-level property at full size: each list is sorted (score desc, row asc), rows inside the shard
    assert_ranked_lists(si, s_sc, lo, hi, 20)
    comm.close()
    fi.close(); ei.close()


def test_exclusion_exchange_layout_world8_on_one_gpu():
    """The W > 1 branch of icrec_search_sharded_excl without a second GPU: the device-side step
    (icrec_exclusions_to_shard_csr = excl_sanitize / count / scan / fill of csrc/comm.hip) on gathered buffers laid out
    exactly as ncclAllGather lays them down — [8][512 + 1] offsets, [8][cap] ids — at BASELINE configs[3]'s sizes (8
    ranks x 512 local queries, shard 1 of the 49,688-row catalog), lists incl. empty and cap-full ranks, against a
    numpy restatement; then MALFORMED offsets (negative, beyond cap, decreasing — ADVICE r3): never out of bounds,
    equal to the restatement's sanitised reading; and the CSR drives icrec_search to the oracle's result."""
    dev = torch.device("cuda:0")
    W, n_local, cap = 8, 512, 512 * 12
    b = shard_bounds(49_688, W)
    lo, hi = b[1], b[2]
    rng = np.random.default_rng(11)
    off_all = np.zeros((W, n_local + 1), np.int32)
    rows_all = np.zeros((W, cap), np.int32)
    lists = []
    for r in range(W):
        flat = []
        for i in range(n_local):
            if r == 3:          # a rank without any exclusion
                n = 0
            elif r == 5:        # a rank that fills its buffer to the last slot
                n = 12
            else:
                n = int(rng.integers(0, 13)) if i % 7 else 0
            e = sorted(set(rng.integers(0, 49_688, size=n).tolist())) if r != 5 else \
                sorted(rng.choice(49_688, size=12, replace=False).tolist())
            lists.append(e)
            flat.extend(e)
            off_all[r, i + 1] = len(flat)
        assert len(flat) <= cap
        rows_all[r, :len(flat)] = flat
        rows_all[r, len(flat):] = 7          # padding past the last offset must be ignored
    assert off_all[5, -1] == cap
    want_off, want_idx = csr_restatement(off_all, rows_all, cap, lo, hi)
    got_off, got_idx = exclusions_to_shard_csr(torch.from_numpy(off_all).to(dev), torch.from_numpy(rows_all).to(dev), lo, hi)
    np.testing.assert_array_equal(got_off.cpu().numpy(), want_off)
    np.testing.assert_array_equal(got_idx.cpu().numpy()[:want_off[-1]], want_idx)
    # the CSR means what the search expects: gathered queries against the shard, a sample against the oracle
    P, q = bench_catalog(), bench_queries(W * n_local, 2)
    ix = DeviceIndex(torch.from_numpy(P[lo:hi]).to(dev), dev, row_offset=lo)
    idx = torch.empty((W * n_local, 20), dtype=torch.int64, device=dev)
    sc = torch.empty((W * n_local, 20), dtype=torch.float32, device=dev)
    ix.search_into(torch.from_numpy(q).to(dev), 20, got_idx, got_off, idx, sc)
    sample = [0, 1, 511, 512, 513, 1535, 1536, 2560, 2561, 3071, 4095]
    want = oracle.search(q[sample], P[lo:hi], 20, local_exclusions([lists[g] for g in sample], lo, hi), row_offset=lo)
    assert_search((idx[sample], sc[sample]), want)
    ix.close()
    # malformed offsets from "another rank": overlapping full segments, negatives, beyond cap, decreasing runs
    bad = off_all.copy()
    bad[0, :5] = [0, cap, 0, cap, 0]
    bad[1, 1:9] = [-5, 2 * cap, 3, 2, 1, -1, cap + 1, 0]
    bad[2] = bad[2][::-1]
    bad[4, -1] = 2**31 - 1
    want_off, want_idx = csr_restatement(bad, rows_all, cap, lo, hi)
    assert want_off[-1] <= W * cap
    got_off, got_idx = exclusions_to_shard_csr(torch.from_numpy(bad).to(dev), torch.from_numpy(rows_all).to(dev), lo, hi)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got_off.cpu().numpy(), want_off)
    np.testing.assert_array_equal(got_idx.cpu().numpy()[:want_off[-1]], want_idx)


def _scan_case_lists(rng, world, n_local, cap, id_space):
    """Well-formed gathered buffers: rank 0 fills its buffer to the last slot, the last rank of three or more has no
    exclusion at all, the others draw 0 .. 2 cap / n_local ids per query (a fifth of the queries none); the slots past
    a rank's last offset hold 7, which must be ignored."""
    off_all = np.zeros((world, n_local + 1), np.int32)
    rows_all = np.full((world, cap), 7, np.int32)
    for r in range(world):
        if r == 0:
            cuts = np.sort(rng.integers(0, cap + 1, size=n_local - 1))
            counts = np.diff(np.concatenate([[0], cuts, [cap]]))
        elif r == world - 1 and world >= 3:
            counts = np.zeros(n_local, np.int64)
        else:
            counts = rng.integers(0, 2 * cap // n_local + 1, size=n_local) * (rng.random(n_local) < 0.8)
            while counts.sum() > cap:
                counts //= 2
        flat = [np.sort(rng.choice(id_space, size=int(c), replace=False)) for c in counts]
        off_all[r, 1:] = np.cumsum(counts)
        rows_all[r, :off_all[r, -1]] = np.concatenate(flat) if flat else []
    assert off_all[0, -1] == cap
    return off_all, rows_all


@pytest.mark.parametrize("world,n_local", [(1, 1023), (1, 1024), (2, 1025), (3, 2049), (5, 13)])
def test_exclusion_scans_carry_across_chunks(world, n_local):
    """excl_sanitize_kernel walks each rank's n_local + 1 offsets in chunks of 1,024 with a carried running maximum,
    sort.hip's prefix_sum_kernel the world * n_local counts likewise with a carried sum: one full chunk (1,023 + 1 offsets), a chunk
    and one entry, three chunks, counts that are no multiple of 1,024 (3,075 and 6,147) and fewer than one wavefront of
    them (65), against the numpy restatement; cap = 4,096 ids per rank, the shard holds rows 2,000 .. 4,999 of 10,000.
    Then malformed offsets placed so that the carry decides: the maximum in chunk 0 (entry 5 = cap - 7) followed by
    decreasing and negative values through every later chunk; a spike in the last wavefront of chunk 0 that chunk 1
    inherits; a value beyond cap at entry 1,024 exactly, the first of chunk 1.  csr_idx comes back zero-filled from
    the wrapper: the slots past the last offset are still zero."""
    dev = torch.device("cuda:0")
    cap, id_space, lo, hi = 4096, 10_000, 2000, 5000
    rng = np.random.default_rng(world * 10_000 + n_local)
    off_all, rows_all = _scan_case_lists(rng, world, n_local, cap, id_space)
    n1 = n_local + 1
    variants = [("well-formed", off_all)]
    r = world - 2 if world >= 3 else world - 1     # a rank with random lists where there is one
    bad = off_all.copy()
    bad[r, 5] = cap - 7
    bad[r, 6:] = (cap - 8 - 5 * np.arange(n1 - 6)).astype(np.int32)          # below zero from entry 824 on
    variants.append(("maximum in chunk 0", bad))
    if n1 > 1024:
        bad = off_all.copy()
        bad[r, :1000] = np.minimum(bad[r, :1000], cap // 2)
        bad[r, 1000] = cap - 3                                                # wavefront 15 of chunk 0
        bad[r, 1001:] = np.minimum(bad[r, 1001:], cap // 2 - 5)
        bad[r, 1030:1040] = -3
        variants.append(("spike in wavefront 15", bad))
        bad = off_all.copy()
        bad[r, 1024] = cap + 5
        bad[r, 1025:] = (np.arange(n1 - 1025) % 9 - 4).astype(np.int32)
        variants.append(("beyond cap at entry 1,024", bad))
    for what, off in variants:
        want_off, want_idx = csr_restatement(off, rows_all, cap, lo, hi)
        assert want_off[-1] <= world * cap, what
        assert want_off.size == world * n_local + 1
        got_off, got_idx = exclusions_to_shard_csr(torch.from_numpy(off).to(dev), torch.from_numpy(rows_all).to(dev), lo, hi)
        torch.cuda.synchronize()
        got_idx = got_idx.cpu().numpy()
        np.testing.assert_array_equal(got_off.cpu().numpy(), want_off, err_msg=what)
        np.testing.assert_array_equal(got_idx[:want_off[-1]], want_idx, err_msg=what)
        assert got_idx.size == world * cap and not got_idx[want_off[-1]:].any(), what


def test_gathered_partial_keys_layout_world8_on_one_gpu():
    """The W > 1 branch of icrec_search_sharded without a second GPU: keys_all [8, 4096, 20] built from eight
    icrec_search_partial calls over the eight row shards of the 49,688-row catalog (rank-major, exactly what
    ncclAllGather of the per-rank [4096, 20] key blocks lays down) -> icrec_merge_topk == the unsharded index, bit
    for bit on all 4,096 queries, and == the oracle on a sample.  The first and last shards have 6,211 rows each
    (49,688 = 8 x 6,211)."""
    dev = torch.device("cuda:0")
    W, Q, k = 8, 4096, 20
    P, q = bench_catalog(), bench_queries(Q, 2)
    Pd, qd = torch.from_numpy(P).to(dev), torch.from_numpy(q).to(dev)
    b = shard_bounds(49_688, W)
    assert all(b[r + 1] - b[r] == 6211 for r in range(W))
    rng = np.random.default_rng(3)
    excl = redrawn_exclusions(rng, 49_688, Q, cap=30, none_every=3)
    keys_all = sharded_partial_keys(Pd, qd, k, excl, b, storage=lambda r: "f32+filter" if r % 2 else "f32")
    idx, sc = merge_topk(keys_all, k)
    full = DeviceIndex(Pd, dev)
    fi, fs = full.search(qd, k, excl)
    assert torch.equal(idx, fi) and torch.equal(sc, fs)
    sample = [0, 1, 511, 512, 2047, 2048, 4094, 4095]
    assert_search((idx[sample], sc[sample]), oracle.search(q[sample], P, k, [excl[g] for g in sample]))
    # a rank-major slip would not survive: swapping two ranks' blocks changes nothing (the merge is order-free in the
    # rank axis), but reading the buffer query-major does
    wrong, _ = merge_topk(keys_all.permute(1, 0, 2).contiguous().view(W, Q, k), k)
    assert not torch.equal(wrong, fi)
    full.close()
