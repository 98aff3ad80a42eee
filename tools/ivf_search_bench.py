#!/usr/bin/env python3
"""IVF search against the exact search, on the 10 M x 384 bf16 catalog (BASELINE config 5's shape; 4,096 lists) and on
bench.py's 49,688 x 384 fp32 catalog (256 lists), k = 20, at 1, 8, 32 and 128 probes.

    python tools/ivf_search_bench.py [--catalog both|10m|bench] [--calls 200] [--warmup 20] [--out profiles/ivf_search_bench.json]

The 10 M catalog is clustered unit vectors generated on the device from a seed (8,192 centres + noise; the queries
likewise, from another seed); the small one is synthetic.synthetic_embeddings(49688, 384, seed=1).  Per catalog: the
time to train the centroids and to build the IVF, then for one request (Q = 1) and a batch (Q = 1,024), in ONE process
on ONE index:
  exact   icrec_search: p50 / min / max of --calls calls after --warmup warm-ups, each call between its own pair of HIP
          events; measured before the IVF rows and once more after them (exact_again: the drift of the box)
  ivf     icrec_ivf_search at each nprobe, the same way; recall@20 against icrec_search over the batch's queries; the
          share of the catalog's rows its probed lists hold; and the kernels' own times from the launch timers in a
          separate short window (slot 10 the list scan, slot 0 the coarse search's kernel, slot 3 the whole coarse search)
One JSON line on stdout, also written to --out."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from instacart_next_order_recommendation_amd import _native, synthetic  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex, IvfIndex, train_centroids  # noqa: E402

DIM, K, PROBES, BATCH = 384, 20, (1, 8, 32, 128), 1024
T_SEARCH_KERNEL, T_SEARCH, T_IVF_SCAN = 0, 3, 10


def clustered(n, centres, noise, seed, dev, chunk=1 << 20):
    """n unit rows, row i = normalise(centres[c_i] + noise * g_i / sqrt(dim)), float32 on the device."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n, DIM), dtype=torch.float32, device=dev)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        c = torch.randint(0, centres.shape[0], (m,), generator=gen, device=dev)
        g = torch.randn((m, DIM), generator=gen, device=dev)
        out[lo:lo + m] = torch.nn.functional.normalize(centres[c] + (noise / DIM ** 0.5) * g, dim=1)
    return out


def per_call_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = np.asarray([a.elapsed_time(b) for a, b in ev])
    return {"p50": round(float(np.median(t)), 5), "min": round(float(t.min()), 5), "max": round(float(t.max()), 5), "calls": calls}


def launch_timers(fn, slots, calls=20):
    torch.cuda.synchronize()
    _native.timing_reset()
    _native.timing_enable(True)
    try:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return {name: round(_native.timing_query(slot)[0], 5) for name, slot in slots.items()}
    finally:
        _native.timing_enable(False)


def note(*what):
    """Progress, on stderr: stdout carries the one JSON line."""
    print(*what, file=sys.stderr, flush=True)


def measure(name, rows, queries, storage, n_lists, args, dev):
    n = int(rows.shape[0])
    note(name, "index")
    ix = DeviceIndex(rows, dev, storage=storage)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cent = train_centroids(ix, n_lists)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    note(name, f"centroids trained in {train_s:.1f} s")
    t0 = time.perf_counter()
    ivf = IvfIndex(ix, cent)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    note(name, f"IVF built in {build_s:.1f} s")
    sizes = np.diff(ivf.layout()[1].cpu().numpy())
    cent_ix = DeviceIndex(cent, dev)  # names the lists each query probes
    out = {"catalog": name, "rows": n, "dim": DIM, "storage": storage, "k": K, "n_lists": n_lists,
           "train_centroids_s": round(train_s, 3), "ivf_create_s": round(build_s, 3),
           "list_rows": {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max())}, "shapes": []}
    for Q in (1, BATCH):
        q = queries[:Q].contiguous()
        idx = torch.empty((Q, K), dtype=torch.int64, device=dev)
        sc = torch.empty((Q, K), dtype=torch.float32, device=dev)
        ws = ix._workspace(Q, K)

        def exact():
            ix.search_into(q, K, None, None, idx, sc, ws=ws)

        row = {"Q": Q, "exact_ms": per_call_ms(exact, args.calls, args.warmup),
               "exact_kernels_ms": launch_timers(exact, {"search_kernel": T_SEARCH_KERNEL, "whole_search": T_SEARCH}), "ivf": []}
        want = idx.clone()
        for nprobe in PROBES:
            if nprobe > n_lists:
                continue
            iws = ivf._workspace(Q, K, nprobe)
            iidx, isc = torch.empty_like(idx), torch.empty_like(sc)

            def approx():
                ivf.search_into(q, K, nprobe, None, None, iidx, isc, ws=iws)

            r = {"nprobe": nprobe, "ms": per_call_ms(approx, args.calls, args.warmup),
                 "kernels_ms": launch_timers(approx, {"ivf_scan": T_IVF_SCAN, "coarse_kernel": T_SEARCH_KERNEL,
                                                      "coarse_search": T_SEARCH})}
            hit = (iidx[:, :, None] == want[:, None, :]).any(dim=2).float().mean().item()
            r["recall_at_20"] = round(hit, 4)
            probed = cent_ix.search(q, nprobe)[0].cpu().numpy()
            r["probed_rows_share"] = round(float(sizes[probed].sum(axis=1).mean() / n), 6)
            r["speedup_over_exact"] = round(row["exact_ms"]["p50"] / r["ms"]["p50"], 3)
            row["ivf"].append(r)
            note(name, f"Q={Q} nprobe={nprobe}: {r['ms']['p50']} ms against {row['exact_ms']['p50']} ms exact")
        row["exact_again_ms"] = per_call_ms(exact, args.calls, args.warmup)
        if Q == 1:
            row["under_half_of_exact_where_probed_share_at_most_1_16"] = all(
                r["ms"]["p50"] < 0.5 * row["exact_ms"]["p50"] for r in row["ivf"] if r["probed_rows_share"] <= 1 / 16)
        out["shapes"].append(row)
    cent_ix.close()
    ivf.close()
    ix.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--catalog", choices=("both", "10m", "bench"), default="both")
    ap.add_argument("--rows", type=int, default=10_000_000, help="rows of the large catalog")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "ivf_search_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ivf_search_bench needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    catalogs = []
    if args.catalog in ("both", "bench"):
        rows = torch.from_numpy(synthetic.synthetic_embeddings(49688, DIM, seed=1)).to(dev)
        queries = torch.from_numpy(synthetic.synthetic_embeddings(BATCH, DIM, seed=7)).to(dev)
        catalogs.append(measure("bench 49,688 x 384", rows, queries, "f32", 256, args, dev))
        del rows
    if args.catalog in ("both", "10m"):
        gen = torch.Generator(device=dev).manual_seed(11)
        centres = torch.nn.functional.normalize(torch.randn((8192, DIM), generator=gen, device=dev), dim=1)
        rows = clustered(args.rows, centres, 0.7, 12, dev)
        queries = clustered(BATCH, centres, 0.7, 13, dev)
        catalogs.append(measure(f"clustered {args.rows:,} x 384", rows, queries, "bf16", 4096, args, dev))
        del rows
    result = {"tool": "ivf_search_bench", "device": torch.cuda.get_device_name(0), "calls": args.calls,
              "warmup": args.warmup, "catalogs": catalogs}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
