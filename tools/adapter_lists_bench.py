#!/usr/bin/env python3
"""What an adapter step over per-anchor lists costs, beside the gather it is made of and the pair step next to it.

    python tools/adapter_lists_bench.py [--rounds 7] [--out profiles/adapter_lists_bench.json]

In ONE process, on the bench catalog (49,688 x 384 rows of synthetic.synthetic_embeddings), fp32 and bf16 rows, timed
after a warm-up of every version and alternated round by round, at (B, L) = (256, 100), (1,024, 100), (1,024, 1,024):
  lists    icrec_adapter_step_lists with update = 1: B anchors, each with its own L distinct random rows and gains
  floor    the same call with every list cut to its first entry (max_len = 1): the forward, plan and grad kernels and
           a middle kernel with next to nothing to do - what the step costs beside its two sweeps
  compose  icrec_compose_queries at the same (queries, terms) = (B, L), no base: the same gather ONCE, a weighted sum
           without the dot products
  pair     the unchanged icrec_adapter_step at B = C = 256: the yardstick next to it
middle_ms = lists - floor is the two sweeps of lists_kernel, DERIVED from two timed calls, not a kernel's own time;
middle_over_compose is that over one compose pass - the expectation to confirm or refute was "about two".  gathered
bytes are B x L x dim x the row element's size, read twice by the middle (sweep 1, sweep 2) and once by compose;
*_gbytes_per_s is that over the median time.  Times are per call, from HIP events around a window of back-to-back
calls (about 0.1 s of work, at least 5 calls); per version the median, minimum and maximum over the rounds.
Not measured: each kernel's own time (no kernel trace was taken), lists of mixed lengths or with dropped entries, widths
other than 384, catalogs that do not fit the Infinity Cache, fit_lists' host side.
There is no pass / fail bar: everything is reported as measured.  One JSON line on stdout, also written to --out."""
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
from tools.adapter_bench import random_adapter, timed  # noqa: E402

N_ROWS, DIM = 49688, 384
SHAPES = ((256, 100), (1024, 100), (1024, 1024))
PAIR_B = 256
GAINS = np.asarray([0, 0, 0, 0, 1, 2, 4], np.float32)


def storage_cases(args, dev, rows, storage):
    rng = np.random.default_rng(1)
    ix = DeviceIndex(rows, dev, storage=storage)
    elem = 2 if storage == "bf16" else 4
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    versions, keep = {}, []
    for B, L in SHAPES:
        anchors = torch.from_numpy(synthetic.synthetic_embeddings(B, DIM, seed=3 + B)).to(dev)
        list_rows = np.stack([rng.choice(args.rows, L, replace=False) for _ in range(B)]).astype(np.int32)
        gains = rng.choice(GAINS, (B, L))
        gains[:, 0] = 4.0
        off = torch.arange(B + 1, dtype=torch.int32, device=dev) * L
        r, g = torch.from_numpy(list_rows.reshape(-1)).to(dev), torch.from_numpy(gains.reshape(-1)).to(dev)
        out = torch.empty((B, DIM), dtype=torch.float32, device=dev)
        ad, ad_floor = random_adapter(dev), random_adapter(dev)
        keep.append((anchors, off, r, g, out, ad, ad_floor))
        versions[f"lists {B}x{L}"] = (lambda ad=ad, a=anchors, c=(off, r, g, L): ad.step_lists(ix, a, c, 1e-4, loss_out=loss))
        versions[f"floor {B}x{L}"] = (lambda ad=ad_floor, a=anchors, c=(off, r, g, 1): ad.step_lists(ix, a, c, 1e-4, loss_out=loss))
        versions[f"compose {B}x{L}"] = (lambda B=B, L=L, off=off, r=r, g=g, out=out:
                                        _native.compose_queries(ix._h, None, None, B, off, r, g, L, out, dev))
    ad_pair = random_adapter(dev)
    a_pair = torch.from_numpy(synthetic.synthetic_embeddings(PAIR_B, DIM, seed=3 + PAIR_B)).to(dev)
    cand = torch.from_numpy(rng.choice(args.rows, PAIR_B, replace=False).astype(np.int32)).to(dev)
    versions["pair"] = lambda: ad_pair.step(ix, a_pair, cand, 1e-4, loss_out=loss)
    t = timed(versions, args.rounds)
    steps = []
    for B, L in SHAPES:
        lists, floor, compose = (t[f"{k} {B}x{L}"] for k in ("lists", "floor", "compose"))
        middle = lists["median"] - floor["median"]
        gathered = B * L * DIM * elem
        steps.append({"storage": storage, "dim": DIM, "B": B, "L": L, "lists_ms": lists, "floor_ms": floor, "compose_ms": compose,
                      "middle_ms_derived": round(middle, 5), "middle_over_compose": round(middle / compose["median"], 3),
                      "gathered_mbytes_per_pass": round(gathered / 1e6, 3),
                      "middle_gbytes_per_s": round(2 * gathered / (middle * 1e-3) / 1e9, 1),
                      "compose_gbytes_per_s": round(gathered / (compose["median"] * 1e-3) / 1e9, 1),
                      "loss_finite": bool(torch.isfinite(loss).all())})
    pair = {"storage": storage, "dim": DIM, "B": PAIR_B, "C": PAIR_B, "step_ms": t["pair"]}
    ix.close()
    return steps, pair


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "adapter_lists_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("adapter_lists_bench needs an MI355X: nothing here is measured without one")
    if args.rounds < 7:
        raise SystemExit("--rounds must be at least 7: the medians are over the rounds")
    dev = torch.device("cuda", 0)
    rows = synthetic.synthetic_embeddings(args.rows, DIM, seed=1)
    result = {"tool": "adapter_lists_bench", "device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM,
              "rounds": args.rounds, "step": [], "pair_step": [],
              "not_measured": ["each kernel's own time (middle_ms_derived is lists - floor)", "mixed lengths, dropped entries",
                               "widths other than 384", "catalogs beyond the Infinity Cache", "fit_lists' host side"]}
    for storage in ("f32", "bf16"):
        steps, pair = storage_cases(args, dev, rows, storage)
        result["step"] += steps
        result["pair_step"].append(pair)
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
