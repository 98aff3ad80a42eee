#!/usr/bin/env python
"""Time the item-item CF ranking and the IR metrics on the device at an Instacart-like synthetic shape, beside the same
ranking on the host CPU.

  shape    --candidates 49,688 products, --orders ~200 k baskets of mean --basket 10 drawn from a Zipf-like popularity,
           --queries 13,120 histories of mean --history 60
  build    icrec_cf_create, wall ms (upload, de-duplication, transpose)
  rank     icrec_cf_rank at depth 100 and icrec_cf_rank_all, in passes of --pass queries: median ms per pass by HIP
           events after a warm-up pass, and the total over all queries
  metrics  icrec_ir_metrics over the [queries, 100] rows, median ms
  bytes    what passes A and B move per pass, and the fraction of the HBM (8 TB/s) and LDS rates that implies
  host     the same scores by torch sparse products B^T (B H) on --threads CPU threads plus a top-100, over a
           --host-queries slice, scaled to all queries
Prints one JSON line and stores it (default profiles/cf_bench.json).  Needs the GPU: no fallback.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_BYTES_PER_S = 8.0e12
LDS_BYTES_PER_S = 256 * 128 * 2.4e9  # 256 CUs x 128 B/clk x 2.4 GHz


def synthetic(args):
    rng = np.random.default_rng(args.seed)
    pop = 1.0 / np.arange(1, args.candidates + 1) ** 0.9
    pop /= pop.sum()
    lens = np.clip(rng.poisson(args.basket, args.orders), 1, 80).astype(np.int64)
    off = np.zeros(args.orders + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    items = rng.choice(args.candidates, size=int(off[-1]), p=pop).astype(np.int32)   # repeats inside a basket happen
    hl = np.clip(rng.poisson(args.history, args.queries), 0, 400)
    hists = [np.unique(rng.choice(args.candidates, size=int(n), p=pop)).astype(np.int32) for n in hl]
    return off, items, hists


def event_ms(fn, iters: int, warmup: int = 1):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(); fn(); ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--candidates", type=int, default=49_688)
    ap.add_argument("--orders", type=int, default=200_000)
    ap.add_argument("--basket", type=float, default=10.0)
    ap.add_argument("--queries", type=int, default=13_120)
    ap.add_argument("--history", type=float, default=60.0)
    ap.add_argument("--pass", dest="per_pass", type=int, default=1024)
    ap.add_argument("--pass-all", type=int, default=256, help="queries per rank_all pass")
    ap.add_argument("--host-queries", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "cf_bench.json")
    args = ap.parse_args()

    import torch

    import cf_cases
    from instacart_next_order_recommendation_amd import _native
    from instacart_next_order_recommendation_amd.ir_metrics import ir_metrics_rows_raw

    off, items, hists = synthetic(args)
    torch.cuda.init()
    t0 = time.perf_counter()
    cf = cf_cases.DeviceCF((off, items), args.candidates, args.candidates)
    build_ms = (time.perf_counter() - t0) * 1e3
    lib = _native.lib()
    nnz, tile = int(lib.icrec_cf_nnz(cf.h)), int(lib.icrec_cf_tile(cf.h))

    def passes(step):
        return [hists[s:s + step] for s in range(0, len(hists), step)]

    res = {"tool": "cf_bench", "candidates": args.candidates, "orders": args.orders, "queries": args.queries,
           "nnz_raw": int(off[-1]), "nnz": nnz, "tile": tile, "mean_history": float(np.mean([len(h) for h in hists])),
           "build_ms": round(build_ms, 2)}
    # rank, depth 100
    all_rows = []
    per_pass = []
    for i, chunk in enumerate(passes(args.per_pass)):
        hoff, hitems = cf.hist([h.tolist() for h in chunk])
        rows, scores, ws = cf.rank_buffers(len(chunk), 100)
        ms = event_ms(lambda: cf.rank_into(hoff, hitems, len(chunk), 100, rows, scores, ws), iters=3, warmup=1 if i == 0 else 0)
        per_pass.append(statistics.median(ms))
        all_rows.append(rows.clone())
    res["rank100"] = {"queries_per_pass": args.per_pass, "pass_ms_median": round(statistics.median(per_pass), 3),
                      "total_ms": round(sum(per_pass), 2)}
    # rank_all: the first passes only are timed (the rest repeat them), total scaled
    n = lib
    timed = []
    for i, chunk in enumerate(passes(args.pass_all)[:4]):
        hoff, hitems = cf.hist([h.tolist() for h in chunk])
        Q = len(chunk)
        ws = torch.empty(int(n.icrec_cf_rank_all_workspace_bytes(cf.h, Q)), dtype=torch.uint8, device="cuda:0")
        out = torch.empty((Q, args.candidates), dtype=torch.int64, device="cuda:0")

        def run():
            _native.check(n.icrec_cf_rank_all(cf.h, _native.ptr(hoff), _native.ptr(hitems), Q, _native.ptr(out), _native.ptr(ws),
                                              ws.numel(), _native.stream_ptr(torch.device("cuda:0"))), "icrec_cf_rank_all")
        timed.append(statistics.median(event_ms(run, iters=3, warmup=1 if i == 0 else 0)))
        del ws, out
    n_all = len(passes(args.pass_all))
    res["rank_all"] = {"queries_per_pass": args.pass_all, "pass_ms_median": round(statistics.median(timed), 3),
                       "total_ms_scaled": round(statistics.median(timed) * n_all, 2), "passes_timed": len(timed)}
    # metrics over the depth-100 rows
    ranked = torch.cat(all_rows)
    rng = np.random.default_rng(1)
    rel = [np.unique(rng.integers(0, args.candidates, 8)) for _ in range(args.queries)]
    roff = np.zeros(args.queries + 1, np.int64)
    np.cumsum([len(r) for r in rel], out=roff[1:])
    roff_d, rrows_d = torch.from_numpy(roff).cuda(), torch.from_numpy(np.concatenate(rel).astype(np.int64)).cuda()
    res["ir_metrics_ms"] = round(statistics.median(event_ms(lambda: ir_metrics_rows_raw(ranked, roff_d, rrows_d), iters=10)), 4)
    # bytes per pass of the depth-100 ranking
    Q = args.per_pass
    tiles = (Q + tile - 1) // tile
    P = 1 << (args.candidates - 1).bit_length()
    a_bytes = tiles * (nnz * 4 + args.orders * 4) + tiles * args.orders * tile * 2        # baskets read per tile, w written
    b_bytes = tiles * (nnz * 4 + nnz * tile * 2) + Q * P * 8                               # columns + w rows read, keys written
    a_lds = tiles * nnz * 4
    res["bytes_per_pass"] = {"pass_a_global": a_bytes, "pass_b_global": b_bytes, "pass_a_lds_reads": a_lds,
                             "hbm_fraction_if_all_of_pass_ms": round((a_bytes + b_bytes) / (res["rank100"]["pass_ms_median"] * 1e-3)
                                                                     / HBM_BYTES_PER_S, 4),
                             "lds_fraction_if_all_of_pass_ms": round(a_lds / (res["rank100"]["pass_ms_median"] * 1e-3)
                                                                     / LDS_BYTES_PER_S, 5)}
    # the host: B^T (B H) with torch sparse products, top-100, on a slice
    torch.set_num_threads(args.threads)
    order_of = np.repeat(np.arange(args.orders), np.diff(off))
    pairs = np.unique(np.stack([order_of, items.astype(np.int64)]), axis=1)               # de-duplicated incidence
    B = torch.sparse_coo_tensor(torch.from_numpy(pairs), torch.ones(pairs.shape[1]), (args.orders, args.candidates)).coalesce()
    Bc, Bt = B.to_sparse_csr(), B.t().coalesce().to_sparse_csr()
    hq = hists[:args.host_queries]
    H = torch.zeros((args.candidates, len(hq)))
    for j, h in enumerate(hq):
        H[torch.from_numpy(h.astype(np.int64)), j] = 1.0
    t0 = time.perf_counter()
    S = Bt @ (Bc @ H)
    S[H.bool()] = -1.0
    top = torch.topk(S.t(), 100, dim=1)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = all_rows[0][:len(hq)].cpu()
    same_scores = bool(torch.equal(torch.gather(S.t(), 1, got).to(torch.int64), torch.gather(S.t(), 1, top.indices).to(torch.int64)))
    res["host"] = {"threads": args.threads, "queries": len(hq), "slice_ms": round(host_ms, 2),
                   "total_ms_scaled": round(host_ms * args.queries / len(hq), 1), "same_top100_scores_as_device": same_scores}
    res["speedup_rank100_vs_host"] = round(res["host"]["total_ms_scaled"] / res["rank100"]["total_ms"], 1)
    cf.close()
    line = json.dumps(res)
    print(line)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
