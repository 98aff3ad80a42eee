#!/usr/bin/env python3
"""What the MMR re-selection costs next to the search that feeds it, on the bench catalog (49,688 x 384 rows of
synthetic.synthetic_embeddings, "f32" storage) at Q = 1 and Q = 1,024 for (candidates, top_k) = (80, 20) and (128, 32).

    python tools/mmr_bench.py [--rounds 7] [--out profiles/mmr_bench.json]

Per case, timed in ONE process on one build and alternated round by round after a warm-up of every version:
  search_topk        icrec_search at k = top_k (the plain request)
  search_cand        icrec_search at k = candidates
  search_cand_mmr    that search followed by icrec_mmr_select (the diversified request)
  mmr                icrec_mmr_select alone on that search's result, lambda = 0.5
Times are per call, from HIP events around a window of back-to-back calls (about 0.1 s of work); per version the median,
minimum and maximum over the rounds.  mmr's two kernels come from the library's launch timers (icrec_timing_query slots
5 and 6: events around each launch) over a separate run of 200 calls.  There is no pass / fail bar: mmr_over_search_cand
is reported as measured.  One JSON line on stdout, also written to --out."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from instacart_next_order_recommendation_amd import _native, synthetic  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex  # noqa: E402

N_ROWS, DIM, STORAGE, LAMBDA = 49688, 384, "f32", 0.5
CASES = [(1, 80, 20), (1, 128, 32), (1024, 80, 20), (1024, 128, 32)]  # (Q, candidates, top_k)
T_MMR_GRAM, T_MMR_SELECT = 5, 6


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mmr_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mmr_bench needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    ix = DeviceIndex(synthetic.synthetic_embeddings(args.rows, DIM, seed=1), dev, storage=STORAGE)

    def buffers(Q, k):
        return torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev)

    cases = []
    for Q, cands, top_k in CASES:
        q = torch.from_numpy(synthetic.synthetic_embeddings(Q, DIM, seed=7 + Q)).to(dev)
        plain, wide, wide2, picked, picked2 = buffers(Q, top_k), buffers(Q, cands), buffers(Q, cands), buffers(Q, top_k), buffers(Q, top_k)
        ix.search_into(q, cands, None, None, *wide)  # mmr alone reads this result

        def search_cand_mmr():
            ix.search_into(q, cands, None, None, *wide2)
            ix.mmr_select_into(*wide2, top_k, LAMBDA, *picked2)

        versions = {"search_topk": lambda: ix.search_into(q, top_k, None, None, *plain),
                    "search_cand": lambda: ix.search_into(q, cands, None, None, *wide2),
                    "search_cand_mmr": search_cand_mmr,
                    "mmr": lambda: ix.mmr_select_into(*wide, top_k, LAMBDA, *picked)}
        iters = {}
        for name, fn in versions.items():  # warm-up of this shape, and the window length per version
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[name] = int(min(max(100.0 / max(window_ms(fn, 5), 1e-3), 5), 4000))
        assert torch.equal(picked[0], picked2[0]) and torch.equal(picked[1], picked2[1]), (Q, cands)
        ms = {name: [] for name in versions}
        for _ in range(args.rounds):  # alternated: one window of every version per round
            for name, fn in versions.items():
                ms[name].append(window_ms(fn, iters[name]))
        torch.cuda.synchronize()
        _native.timing_reset()
        _native.timing_enable(True)
        try:
            for _ in range(200):
                versions["mmr"]()
            torch.cuda.synchronize()
        finally:
            _native.timing_enable(False)
        gram_ms, gram_n = _native.timing_query(T_MMR_GRAM)
        select_ms, select_n = _native.timing_query(T_MMR_SELECT)
        _native.timing_reset()
        changed = int((picked[0].sort(dim=1).values != wide[0][:, :top_k].sort(dim=1).values).any(dim=1).sum().item())
        row = {"Q": Q, "candidates": cands, "top_k": top_k, "lambda": LAMBDA, "lists_changed_by_mmr": changed}
        for name, t in ms.items():
            row[name + "_ms"] = {"median": round(float(np.median(t)), 5), "min": round(min(t), 5), "max": round(max(t), 5),
                                 "calls_per_window": iters[name]}
        row["mmr_kernels_ms"] = {"gram": round(gram_ms, 5), "select": round(select_ms, 5), "launches_each": int(min(gram_n, select_n))}
        row["mmr_over_search_cand"] = round(row["mmr_ms"]["median"] / row["search_cand_ms"]["median"], 3)
        row["diversified_over_plain"] = round(row["search_cand_mmr_ms"]["median"] / row["search_topk_ms"]["median"], 3)
        cases.append(row)
    result = {"tool": "mmr_bench", "device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "storage": STORAGE,
              "rounds": args.rounds, "cases": cases}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    ix.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
