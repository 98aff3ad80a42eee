#!/usr/bin/env python3
"""What rank fusion costs: icrec_fuse_select beside the two calls that feed it, and whole fused requests beside plain
ones.

    python tools/fuse_bench.py [--rounds 7] [--out profiles/fuse_bench.json]

The step, in ONE process, on the bench catalog (49,688 x 384 rows of synthetic.synthetic_embeddings, "f32" storage) and
a synthetic order x product incidence matrix of tools/cf_bench.py's size (49,688 candidates, 200,000 baskets of mean 10
from a Zipf-like popularity, histories of mean 60), at Q = 1 and Q = 1,024 and the shapes 80 + 80 -> 20 and
128 + 128 -> 32; timed after a warm-up of every version and alternated round by round:
  search       icrec_search at k = the list width
  cf_rank      icrec_cf_rank at k = the list width, on the histories
  fuse_select  icrec_fuse_select alone on those two results, rrf_weights tables, the CF scores as B's gate
Times are per call, from HIP events around a window of back-to-back calls (about 0.1 s of work, at least 5 calls); per
version the median, minimum and maximum over the rounds.
Whole requests, on a Recommender over a synthetic catalog of --products products (a 2-layer synthetic model; the CF
baseline over seeded baskets of the same products): recommend(q, 20, history=) against recommend(q, 20) on the
un-captured path (ICREC_USE_GRAPH=0 is not set: the plain single request replays its hipGraph, which is what a plain
request costs), and recommend_batch of 1,024 queries with and without histories; host wall clock around the call, which
returns after the read-back; median, minimum and maximum over --rounds calls after a warm-up call.
There is no pass / fail bar: everything is reported as measured.  One JSON line on stdout, also written to --out."""
from __future__ import annotations

import argparse
import json
import random
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from instacart_next_order_recommendation_amd import synthetic  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex, fuse_select_into, rrf_weights  # noqa: E402

N_ROWS, DIM, STORAGE = 49688, 384, "f32"
SHAPES = ((80, 20), (128, 32))  # (the width of both lists, top_k)


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


def incidence(rng, candidates, orders, basket, queries, history):
    """tools/cf_bench.py's synthetic shape: (off int64, items int32, per-query history arrays)."""
    pop = 1.0 / np.arange(1, candidates + 1) ** 0.9
    pop /= pop.sum()
    lens = np.clip(rng.poisson(basket, orders), 1, 80).astype(np.int64)
    off = np.zeros(orders + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    items = rng.choice(candidates, size=int(off[-1]), p=pop).astype(np.int32)
    hl = np.clip(rng.poisson(history, queries), 0, 400)
    return off, items, [np.unique(rng.choice(candidates, size=int(n), p=pop)).astype(np.int32) for n in hl]


def step_cases(args, dev):
    import cf_cases

    ix = DeviceIndex(synthetic.synthetic_embeddings(args.rows, DIM, seed=1), dev, storage=STORAGE)
    off, items, hists = incidence(np.random.default_rng(0), args.rows, args.orders, 10.0, 1024, 60.0)
    cf = cf_cases.DeviceCF((off, items), args.rows, args.rows)
    cases = []
    for Q in (1, 1024):
        q = torch.from_numpy(synthetic.synthetic_embeddings(Q, DIM, seed=7 + Q)).to(dev)
        hoff, hitems = cf.hist([h.tolist() for h in hists[:Q]])
        for w, top_k in SHAPES:
            a = (torch.empty((Q, w), dtype=torch.int64, device=dev), torch.empty((Q, w), dtype=torch.float32, device=dev))
            b_rows, b_sc, ws = cf.rank_buffers(Q, w)
            out = (torch.empty((Q, top_k), dtype=torch.int64, device=dev), torch.empty((Q, top_k), dtype=torch.float32, device=dev))
            a_w, b_w = (torch.from_numpy(rrf_weights(w)).to(dev) for _ in range(2))
            versions = {"search": lambda: ix.search_into(q, w, None, None, *a),
                        "cf_rank": lambda: cf.rank_into(hoff, hitems, Q, w, b_rows, b_sc, ws),
                        "fuse_select": lambda: fuse_select_into(a[0], b_rows, a_w, b_w, top_k, args.rows, *out, b_gate=b_sc)}
            iters = {}
            for name, fn in versions.items():  # warm-up of this shape (the producers first: fuse reads their results)
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                iters[name] = int(min(max(100.0 / max(window_ms(fn, 5), 1e-3), 5), 4000))
            ms = {name: [] for name in versions}
            for _ in range(args.rounds):  # alternated: one window of every version per round
                for name, fn in versions.items():
                    ms[name].append(window_ms(fn, iters[name]))
            torch.cuda.synchronize()
            row = {"Q": Q, "width": w, "top_k": top_k,
                   "results_per_query": round(float((out[0] >= 0).sum().item()) / Q, 2),
                   "live_cf_entries_per_query": round(float((b_sc > 0).sum().item()) / Q, 2)}
            for name, t in ms.items():
                row[name + "_ms"] = dict(spread(t), calls_per_window=iters[name])
            row["fuse_select_over_search"] = round(row["fuse_select_ms"]["median"] / row["search_ms"]["median"], 4)
            row["fuse_select_over_cf_rank"] = round(row["fuse_select_ms"]["median"] / row["cf_rank_ms"]["median"], 4)
            cases.append(row)
            del ws
    cf.close()
    ix.close()
    return cases


def request_cases(args):
    from instacart_next_order_recommendation_amd.baselines import ItemItemCFBaseline
    from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir
    from instacart_next_order_recommendation_amd.recommender import Recommender

    def wall(fn):
        fn()  # warm-up: workspaces of this shape, the graph capture
        t = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1000)
        return spread(t)

    with tempfile.TemporaryDirectory(prefix="icrec_fuse_bench_") as tmp:
        tmp = Path(tmp)
        shape = synthetic.BertShape(vocab_size=len(synthetic.synthetic_vocab()), layers=2)
        model_dir = write_synthetic_model_dir(tmp / "model", seed=3, shape=shape)
        corpus = synthetic.synthetic_catalog(args.products)
        corpus_path = tmp / "processed" / "eval_corpus.json"
        corpus_path.parent.mkdir()
        corpus_path.write_text(json.dumps(corpus))
        ids = list(corpus)
        rng = random.Random(5)
        baskets = [[ids[min(int(rng.expovariate(8.0 / len(ids))), len(ids) - 1)] for _ in range(rng.randrange(3, 18))]
                   for _ in range(4 * len(ids))]
        rec = Recommender(model_dir, corpus_path, use_index=False, cf=ItemItemCFBaseline.from_arrays(baskets, {}, ids))
        queries = synthetic.synthetic_user_contexts(1024, seed=21)
        histories = [rng.sample(ids[:2000], rng.randrange(1, 40)) for _ in queries]
        out = {"products": args.products, "baskets": len(baskets), "model_layers": 2, "top_k": 20, "width": 80,
               "single_plain_graph_ms": wall(lambda: rec.recommend(queries[0], 20)),
               "single_history_ms": wall(lambda: rec.recommend(queries[0], 20, history=histories[0])),
               "batch_1024_plain_ms": wall(lambda: rec.recommend_batch(queries, 20)),
               "batch_1024_history_ms": wall(lambda: rec.recommend_batch(queries, 20, history=histories))}
        out["single_history_over_plain"] = round(out["single_history_ms"]["median"] / out["single_plain_graph_ms"]["median"], 3)
        out["batch_1024_history_over_plain"] = round(out["batch_1024_history_ms"]["median"] / out["batch_1024_plain_ms"]["median"], 3)
        return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--orders", type=int, default=200_000)
    ap.add_argument("--products", type=int, default=N_ROWS, help="the catalog of the whole-request part")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "fuse_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fuse_bench needs an MI355X: nothing here is measured without one")
    if args.rounds < 7:
        raise SystemExit("--rounds must be at least 7: the medians are over the rounds")
    dev = torch.device("cuda", 0)
    result = {"tool": "fuse_bench", "device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "storage": STORAGE,
              "orders": args.orders, "rounds": args.rounds, "cases": step_cases(args, dev), "requests": request_cases(args)}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
