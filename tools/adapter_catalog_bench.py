#!/usr/bin/env python3
"""What a whole-catalog adapter step costs beside the list step it stands next to.

    python tools/adapter_catalog_bench.py [--rounds 7] [--out profiles/adapter_catalog_bench.json]

In ONE process, on the bench catalog (49,688 x 384 rows of synthetic.synthetic_embeddings), fp32 and bf16 rows, timed
after a warm-up of every version and alternated round by round:
  catalog  icrec_adapter_step_catalog with update = 1 at B = 32, 256 and 1,024: every stored row a candidate
  list     the unchanged icrec_adapter_step at (B 1,024, C 8,192), the largest list it takes: the yardstick
  fit      QueryAdapter.fit for one epoch of 4,096 pairs at batch_size 256 with negatives "all", 0 and 7,936; host wall
           clock, which includes the shuffles, the draws and the one read-back
step_gflop counts the products - S = U V^T in both sweeps and P V (3 x 2 B C d, C the rows scored), the apply and dD
(2 x 2 B d d); step_tflops is that over the median time, beside the 157 TFLOPS of the f32 MFMA; ns_per_logit is the
median time over the B x C (anchor, row) pairs scored.  catalog_over_list_per_logit compares the catalog step at
B = 1,024 with the list step of the same run and storage: below 1, a scored pair is cheaper in the catalog step.
Times of the steps are per call, from HIP events around a window of back-to-back calls (about 0.1 s of work, at least 5
calls); per version the median, minimum and maximum over the rounds.
There is no pass / fail bar: everything is reported as measured.  One JSON line on stdout, also written to --out."""
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

from instacart_next_order_recommendation_amd import synthetic  # noqa: E402
from instacart_next_order_recommendation_amd.adapter import QueryAdapter  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex  # noqa: E402
from tools.adapter_bench import F32_MFMA_TFLOPS, random_adapter, spread, timed  # noqa: E402

N_ROWS, DIM = 49688, 384
CATALOG_BATCHES, LIST_B, LIST_C = (32, 256, 1024), 1024, 8192
FIT_PAIRS, FIT_BATCH, FIT_NEGATIVES = 4096, 256, ("all", 0, 7936)


def step_entry(kind, storage, B, scored, t, loss):
    gflop = (3 * 2.0 * B * scored * DIM + 2 * 2.0 * B * DIM * DIM) / 1e9
    return {"step": kind, "storage": storage, "dim": DIM, "B": B, "rows_scored": scored, "step_ms": t,
            "step_gflop": round(gflop, 3), "step_tflops": round(gflop / t["median"], 2), "f32_mfma_tflops": F32_MFMA_TFLOPS,
            "ns_per_logit": round(t["median"] * 1e6 / (B * scored), 5), "loss_finite": bool(torch.isfinite(loss).all())}


def storage_cases(args, dev, rows, storage):
    rng = np.random.default_rng(1)
    ix = DeviceIndex(rows, dev, storage=storage)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    versions, shapes = {}, {}
    for B in CATALOG_BATCHES + (LIST_B,):
        anchors = torch.from_numpy(synthetic.synthetic_embeddings(B, DIM, seed=3 + B)).to(dev)
        shapes[B] = anchors
    for B in CATALOG_BATCHES:
        ad = random_adapter(dev)
        pos = torch.from_numpy(rng.integers(0, args.rows, B).astype(np.int32)).to(dev)
        versions[f"catalog {B}"] = (lambda ad=ad, a=shapes[B], p=pos: ad.step_catalog(ix, a, p, 1e-4, loss_out=loss))
    ad_list = random_adapter(dev)
    cand = torch.from_numpy(rng.choice(args.rows, LIST_C, replace=False).astype(np.int32)).to(dev)
    versions["list"] = lambda: ad_list.step(ix, shapes[LIST_B], cand, 1e-4, loss_out=loss)
    t = timed(versions, args.rounds)
    steps = [step_entry("catalog", storage, B, args.rows, t[f"catalog {B}"], loss) for B in CATALOG_BATCHES]
    steps.append(step_entry("list", storage, LIST_B, LIST_C, t["list"], loss))
    ratio = round(steps[len(CATALOG_BATCHES) - 1]["ns_per_logit"] / steps[-1]["ns_per_logit"], 4)
    # fit: one epoch, the same pairs and seed for every setting of negatives
    anchors = torch.from_numpy(synthetic.synthetic_embeddings(FIT_PAIRS, DIM, seed=11)).to(dev)
    positives = rng.integers(0, args.rows, FIT_PAIRS)
    fits = []
    for negatives in FIT_NEGATIVES:
        ms = []
        for r in range(args.rounds + 1):  # the first run is the warm-up
            ad = QueryAdapter(DIM, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = ad.fit(ix, anchors, positives, epochs=1, batch_size=FIT_BATCH, negatives=negatives, lr=1e-3, seed=5)
            if r:
                ms.append((time.perf_counter() - t0) * 1000)
        fits.append({"storage": storage, "pairs": FIT_PAIRS, "batch_size": FIT_BATCH, "negatives": negatives,
                     "steps": len(losses), "epoch_ms": spread(ms), "losses_finite": bool(np.isfinite(losses).all())})
    ix.close()
    return steps, fits, ratio


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "adapter_catalog_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("adapter_catalog_bench needs an MI355X: nothing here is measured without one")
    if args.rounds < 7:
        raise SystemExit("--rounds must be at least 7: the medians are over the rounds")
    dev = torch.device("cuda", 0)
    rows = synthetic.synthetic_embeddings(args.rows, DIM, seed=1)
    result = {"tool": "adapter_catalog_bench", "device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM,
              "rounds": args.rounds, "step": [], "fit": [], "catalog_over_list_per_logit": {}}
    for storage in ("f32", "bf16"):
        steps, fits, ratio = storage_cases(args, dev, rows, storage)
        result["step"] += steps
        result["fit"] += fits
        result["catalog_over_list_per_logit"][storage] = ratio
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
