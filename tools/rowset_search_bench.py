#!/usr/bin/env python3
"""Set-restricted search against its alternatives, on the bench catalog (49,688 x 384, "f32+filter", k = 20) at Q = 1
and Q = 1,024.

    python tools/rowset_search_bench.py [--calls 200] [--warmup 20] [--out profiles/rowset_search_bench.json]

Legs, timed in ONE process; every call between its own pair of HIP events, the p50 of --calls calls after --warmup:
  plain_before / plain_after   icrec_search, no restriction, timed before and after the other legs (the reference of
                               every ratio is their mean; their difference is the drift of the run)
  faceted_department           icrec_search_faceted, every query under one department of 21 (its own)
  exclusions_store             the only route to a store's result without row sets: icrec_search with every row
                               outside the store in a prebuilt device exclusion CSR
  sets_store                   icrec_search_in_sets, one set of about 40 % of the rows (a store assortment)
  sets_store_and_5pct          that set and a set of 5 % of the rows (two slots: the intersection)
  sets_full                    a set that holds every row
  sets_department              the departments as 21 sets, every query in its own: faceted_department's restriction
                               through a bitmap
exclusions_store and sets_store must return the same bits (asserted), as must faceted_department and
sets_department, and plain and sets_full.  One JSON line on stdout, also written to --out."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from instacart_next_order_recommendation_amd import synthetic  # noqa: E402
from instacart_next_order_recommendation_amd.recommender import catalog_facets  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex, facet_masks, rowset_bits, rowset_ids  # noqa: E402

N_ROWS, DIM, K, STORAGE = 49688, 384, 20, "f32+filter"
STORE, FIVE_PCT, FULL, DEPT0 = 0, 1, 2, 3   # set ids: the departments follow from DEPT0 on


def p50_ms(fn, calls, warmup):
    """The median over `calls` calls of fn, each between its own HIP events, after `warmup` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = np.asarray([a.elapsed_time(b) for a, b in pairs])
    return {"p50": round(float(np.median(t)), 5), "p10": round(float(np.percentile(t, 10)), 5),
            "p90": round(float(np.percentile(t, 90)), 5)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "rowset_search_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rowset_search_bench needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    n = args.rows

    P = synthetic.synthetic_embeddings(n, DIM, seed=1)
    _, departments, codes = catalog_facets(list(synthetic.synthetic_catalog(n).values()))
    rng = np.random.default_rng(40)
    member = np.zeros((DEPT0 + len(departments), n), bool)
    member[STORE] = rng.random(n) < 0.4
    member[FIVE_PCT] = rng.random(n) < 0.05
    member[FULL] = True
    for d in range(len(departments)):
        member[DEPT0 + d] = codes[:, 1] == d
    ix = DeviceIndex(P, dev, storage=STORAGE)
    ix.set_facets(codes)
    ix.set_rowsets(rowset_bits(member, n))

    shapes = []
    for Q in (1, 1024):
        q = torch.from_numpy(synthetic.synthetic_embeddings(Q, DIM, seed=7 + Q)).to(dev)
        legs = ["plain_before", "faceted_department", "exclusions_store", "sets_store", "sets_store_and_5pct", "sets_full",
                "sets_department", "plain_after"]
        out = {v: (torch.empty((Q, K), dtype=torch.int64, device=dev), torch.empty((Q, K), dtype=torch.float32, device=dev))
               for v in legs}
        dept = [(3 + 5 * i) % len(departments) for i in range(Q)]
        masks = facet_masks([[None, [d]] for d in dept], Q, 2, dev)
        rej = np.flatnonzero(~member[STORE]).astype(np.int32)
        ei = torch.from_numpy(np.tile(rej, Q)).to(dev)
        eo = torch.from_numpy((np.arange(Q + 1, dtype=np.int64) * len(rej)).astype(np.int32)).to(dev)
        ids = {"sets_store": rowset_ids([STORE] * Q, Q, 1, dev), "sets_store_and_5pct": rowset_ids([[STORE, FIVE_PCT]] * Q, Q, 2, dev),
               "sets_full": rowset_ids([FULL] * Q, Q, 1, dev), "sets_department": rowset_ids([DEPT0 + d for d in dept], Q, 1, dev)}
        fns = {"plain_before": lambda: ix.search_into(q, K, None, None, *out["plain_before"]),
               "faceted_department": lambda: ix.search_into(q, K, None, None, *out["faceted_department"], allow=masks),
               "exclusions_store": lambda: ix.search_into(q, K, ei, eo, *out["exclusions_store"]),
               "plain_after": lambda: ix.search_into(q, K, None, None, *out["plain_after"])}
        for name, t in ids.items():
            fns[name] = (lambda name=name, t=t: ix.search_into(q, K, None, None, *out[name], sets=t))
        row = {"Q": Q, "excluded_ids": int(ei.numel()), "members": {"store": int(member[STORE].sum()),
                                                                    "store_and_5pct": int((member[STORE] & member[FIVE_PCT]).sum())}}
        for name in legs:
            row[name + "_ms"] = p50_ms(fns[name], args.calls, args.warmup)
        same = lambda a, b: torch.equal(out[a][0], out[b][0]) and torch.equal(out[a][1], out[b][1])  # noqa: E731
        assert same("exclusions_store", "sets_store") and same("faceted_department", "sets_department"), Q
        assert same("plain_before", "sets_full") and same("plain_before", "plain_after"), Q
        plain = (row["plain_before_ms"]["p50"] + row["plain_after_ms"]["p50"]) / 2
        row["plain_drift"] = round(row["plain_after_ms"]["p50"] / row["plain_before_ms"]["p50"], 3)
        for name in legs[1:-1]:
            row[name + "_over_plain"] = round(row[name + "_ms"]["p50"] / plain, 3)
        row["sets_department_over_faceted_department"] = round(row["sets_department_ms"]["p50"] / row["faceted_department_ms"]["p50"], 3)
        row["sets_store_over_exclusions_store"] = round(row["sets_store_ms"]["p50"] / row["exclusions_store_ms"]["p50"], 3)
        shapes.append(row)
        del ei, eo
    result = {"tool": "rowset_search_bench", "device": torch.cuda.get_device_name(0), "rows": n, "dim": DIM, "k": K,
              "storage": STORAGE, "calls": args.calls, "warmup": args.warmup, "shapes": shapes}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    ix.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
