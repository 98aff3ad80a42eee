#!/usr/bin/env python3
"""What the caps per aisle and department cost, on the bench catalog (49,688 x 384 rows of
synthetic.synthetic_embeddings, "f32" storage) with the aisle and department codes of synthetic.synthetic_catalog (134
aisles, 21 departments; facet_search_bench's facets) at Q = 1 and Q = 1,024.

    python tools/cap_select_bench.py [--rounds 7] [--out profiles/cap_select_bench.json]

The step, timed in ONE process and alternated round by round after a warm-up of every version:
  search_cand      icrec_search at k = 128 (the search that feeds the step)
  cap_select       icrec_cap_select alone on that search's result, 128 candidates -> 20 picks, max_per_aisle = 2
Times are per call, from HIP events around a window of back-to-back calls (about 0.1 s of work); per version the median,
minimum and maximum over the rounds.  The kernel's own time comes from the library's launch timer (icrec_timing_query
slot 11: events around each launch) over a separate run of 200 calls.
Whole requests (DeviceIndex.search_capped at top_k = 20 with its default 80 candidates per round, which reads the states
back between rounds, against DeviceIndex.search at k = 20), host wall clock around call + synchronize, per version the
median, minimum and maximum over --rounds calls, with the histogram of the rounds the capped calls took:
  max_per_aisle_2, max_per_department_1
The synthetic embeddings do not cluster by aisle, so these caps bind less often than on a real catalog, where a
shopper's best matches share few aisles; max_per_department = 1 admits at most 21 products and runs until the
departments are used up.  There is no pass / fail bar: everything is reported as measured.  One JSON line on stdout, also
written to --out."""
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
from instacart_next_order_recommendation_amd.recommender import catalog_facets  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex, cap_pairs  # noqa: E402

N_ROWS, DIM, STORAGE, CANDS, TOP_K = 49688, 384, "f32", 128, 20
T_CAP_SELECT = 11


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def spread(t):
    return {"median": round(float(np.median(t)), 5), "min": round(min(t), 5), "max": round(max(t), 5)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "cap_select_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cap_select_bench needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    ix = DeviceIndex(synthetic.synthetic_embeddings(args.rows, DIM, seed=1), dev, storage=STORAGE)
    aisles, departments, codes = catalog_facets(list(synthetic.synthetic_catalog(args.rows).values()))
    ix.set_facets(codes)

    cases = []
    for Q in (1, 1024):
        q = torch.from_numpy(synthetic.synthetic_embeddings(Q, DIM, seed=7 + Q)).to(dev)
        wide = (torch.empty((Q, CANDS), dtype=torch.int64, device=dev), torch.empty((Q, CANDS), dtype=torch.float32, device=dev))
        wide2 = (torch.empty_like(wide[0]), torch.empty_like(wide[1]))
        out = (torch.empty((Q, TOP_K), dtype=torch.int64, device=dev), torch.empty((Q, TOP_K), dtype=torch.float32, device=dev))
        state = torch.empty((Q, 2), dtype=torch.int32, device=dev)
        nxt = torch.empty((Q, 2, 8), dtype=torch.int32, device=dev).view(torch.uint32)
        caps = cap_pairs((2, None), Q, dev)
        ix.search_into(q, CANDS, None, None, *wide)  # cap_select alone reads this result
        versions = {"search_cand": lambda: ix.search_into(q, CANDS, None, None, *wide2),
                    "cap_select": lambda: ix.cap_select_into(*wide, caps, TOP_K, *out, state, allow_next=nxt)}
        iters = {}
        for name, fn in versions.items():  # warm-up of this shape, and the window length per version
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[name] = int(min(max(100.0 / max(window_ms(fn, 5), 1e-3), 5), 4000))
        ms = {name: [] for name in versions}
        for _ in range(args.rounds):  # alternated: one window of every version per round
            for name, fn in versions.items():
                ms[name].append(window_ms(fn, iters[name]))
        torch.cuda.synchronize()
        _native.timing_reset()
        _native.timing_enable(True)
        try:
            for _ in range(200):
                versions["cap_select"]()
            torch.cuda.synchronize()
        finally:
            _native.timing_enable(False)
        kernel_ms, kernel_n = _native.timing_query(T_CAP_SELECT)
        _native.timing_reset()
        st = state.cpu().numpy()
        row = {"Q": Q, "candidates": CANDS, "top_k": TOP_K, "caps": [2, 0],
               "lists_changed_by_the_cap": int((out[0] != wide[0][:, :TOP_K]).any(dim=1).sum().item()),
               "lists_not_done": int((st[:, 1] == 0).sum())}
        for name, t in ms.items():
            row[name + "_ms"] = dict(spread(t), calls_per_window=iters[name])
        row["cap_select_kernel_ms"] = {"kernel": round(kernel_ms, 5), "launches": int(kernel_n)}
        row["cap_select_over_search_cand"] = round(row["cap_select_ms"]["median"] / row["search_cand_ms"]["median"], 4)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1000

        requests = {"plain_top20": (lambda: ix.search(q, TOP_K), None),
                    "max_per_aisle_2": (lambda: ix.search_capped(q, TOP_K, (2, None)), (2, None)),
                    "max_per_department_1": (lambda: ix.search_capped(q, TOP_K, (None, 1)), (None, 1))}
        row["requests_wall_ms"] = {}
        for name, (fn, pair) in requests.items():
            fn()  # warm-up: workspaces of this shape
            t, hist = [], {}
            for _ in range(args.rounds):
                t.append(wall(fn))
                if pair is not None:
                    hist[str(ix.last_cap_rounds)] = hist.get(str(ix.last_cap_rounds), 0) + 1
            row["requests_wall_ms"][name] = dict(spread(t), **({"rounds_histogram_over_calls": hist} if pair else {}))
        plain = row["requests_wall_ms"]["plain_top20"]["median"]
        for name in ("max_per_aisle_2", "max_per_department_1"):
            row["requests_wall_ms"][name]["over_plain"] = round(row["requests_wall_ms"][name]["median"] / plain, 3)
        cases.append(row)
    # how many rounds single requests take: 256 queries one at a time, per cap
    q = torch.from_numpy(synthetic.synthetic_embeddings(256, DIM, seed=99)).to(dev)
    single = {}
    for name, pair in (("max_per_aisle_2", (2, None)), ("max_per_department_1", (None, 1))):
        hist = {}
        for i in range(256):
            ix.search_capped(q[i:i + 1], TOP_K, pair)
            hist[ix.last_cap_rounds] = hist.get(ix.last_cap_rounds, 0) + 1
        single[name] = {str(r): n for r, n in sorted(hist.items())}
    result = {"tool": "cap_select_bench", "device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM,
              "storage": STORAGE, "aisles": len(aisles), "departments": len(departments), "rounds": args.rounds, "cases": cases,
              "rounds_histogram_of_256_single_requests": single}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    ix.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
