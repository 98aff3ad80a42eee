#!/usr/bin/env python3
"""What composing a query from stored rows costs: icrec_compose_queries beside the search it feeds, and whole
like / unlike and similar-items requests beside plain ones.

    python tools/compose_bench.py [--rounds 7] [--out profiles/compose_bench.json]

The step, in ONE process, on the bench catalog (49,688 x 384 rows of synthetic.synthetic_embeddings) under the storages
"f32+filter" and "bf16+filter", at Q = 1 and Q = 1,024 queries of 8 / 64 / 1,024 terms each (random rows, weights in
[-1, 1], a text part on every query); timed after a warm-up of every version and alternated round by round:
  compose  icrec_compose_queries alone
  search   icrec_search at k = 20 on the composed queries
Times are per call, from HIP events around a window of back-to-back calls (about 0.1 s of work, at least 5 calls); per
version the median, minimum and maximum over the rounds.  term_gb_per_s is the bytes the terms' stored rows occupy
(Q x terms x dim x 4 or 2) over the median compose time, beside the 6,300 GB/s of HBM traffic the chip sustains; the
catalog (76 MB of fp32 rows, 38 MB of bf16) fits the Infinity Cache, and a window repeats the same lists, so a rate
above the HBM figure is the cache's.
Whole requests, on a Recommender over a synthetic catalog of --products products (a 2-layer synthetic model):
recommend(q, 20, like=64 ids) against recommend(q, 20) on the un-captured path (what ICREC_USE_GRAPH=0 runs) and against
the plain request's hipGraph replay, and similar_products(p, 20) against recommend(q, 20); host wall clock around the
call, which returns after the read-back; median, minimum and maximum over --rounds calls after a warm-up call.
There is no pass / fail bar: everything is reported as measured.  One JSON line on stdout, also written to --out."""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from instacart_next_order_recommendation_amd import synthetic  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex  # noqa: E402

N_ROWS, DIM, K = 49688, 384, 20
STORAGES = ("f32+filter", "bf16+filter")
HBM_GB_PER_S = 6300.0  # the achievable rate, not the 8 TB/s of the data sheet


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


def step_cases(args, dev):
    rows = synthetic.synthetic_embeddings(args.rows, DIM, seed=1)
    rng = np.random.default_rng(0)
    cases = []
    for storage in STORAGES:
        ix = DeviceIndex(rows, dev, storage=storage)
        elem = 2 if storage.startswith("bf16") else 4
        for Q in (1, 1024):
            base = torch.from_numpy(synthetic.synthetic_embeddings(Q, DIM, seed=7 + Q)).to(dev)
            idx = torch.empty((Q, K), dtype=torch.int64, device=dev)
            sc = torch.empty((Q, K), dtype=torch.float32, device=dev)
            out = torch.empty((Q, DIM), dtype=torch.float32, device=dev)
            for n_terms in (8, 64, 1024):
                off = torch.arange(0, (Q + 1) * n_terms, n_terms, dtype=torch.int32, device=dev)
                t_rows = torch.from_numpy(rng.integers(0, args.rows, Q * n_terms).astype(np.int32)).to(dev)
                t_w = torch.from_numpy(rng.uniform(-1.0, 1.0, Q * n_terms).astype(np.float32)).to(dev)
                versions = {"compose": lambda: ix.compose_queries_into(base, None, off, t_rows, t_w, n_terms, out),
                            "search": lambda: ix.search_into(out, K, None, None, idx, sc)}
                iters = {}
                for name, fn in versions.items():  # warm-up of this shape (compose first: the search reads its result)
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    iters[name] = int(min(max(100.0 / max(window_ms(fn, 5), 1e-3), 5), 4000))
                ms = {name: [] for name in versions}
                for _ in range(args.rounds):  # alternated: one window of every version per round
                    for name, fn in versions.items():
                        ms[name].append(window_ms(fn, iters[name]))
                torch.cuda.synchronize()
                row = {"storage": storage, "Q": Q, "terms": n_terms, "term_bytes": Q * n_terms * DIM * elem}
                for name, t in ms.items():
                    row[name + "_ms"] = dict(spread(t), calls_per_window=iters[name])
                row["term_gb_per_s"] = round(row["term_bytes"] / (row["compose_ms"]["median"] * 1e-3) / 1e9, 1)
                row["hbm_gb_per_s"] = HBM_GB_PER_S
                row["compose_over_search"] = round(row["compose_ms"]["median"] / row["search_ms"]["median"], 4)
                cases.append(row)
        ix.close()
    return cases


def request_cases(args):
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

    with tempfile.TemporaryDirectory(prefix="icrec_compose_bench_") as tmp:
        tmp = Path(tmp)
        shape = synthetic.BertShape(vocab_size=len(synthetic.synthetic_vocab()), layers=2)
        model_dir = write_synthetic_model_dir(tmp / "model", seed=3, shape=shape)
        corpus = synthetic.synthetic_catalog(args.products)
        corpus_path = tmp / "processed" / "eval_corpus.json"
        corpus_path.parent.mkdir()
        corpus_path.write_text(json.dumps(corpus))
        ids = list(corpus)
        rec = Recommender(model_dir, corpus_path, use_index=False)
        query = synthetic.synthetic_user_contexts(1, seed=21)[0]
        liked = [ids[int(r)] for r in np.random.default_rng(5).choice(len(ids), 64, replace=False)]
        out = {"products": args.products, "model_layers": 2, "top_k": K, "storage": rec._index.storage,
               "single_plain_graph_ms": wall(lambda: rec.recommend(query, K)),
               "single_like_64_ms": wall(lambda: rec.recommend(query, K, like=liked)),
               "similar_products_ms": wall(lambda: rec.similar_products(ids[7], K))}
        fast, rec._fast = rec._fast, None  # the un-captured plain request: what ICREC_USE_GRAPH=0 runs
        out["single_plain_uncaptured_ms"] = wall(lambda: rec.recommend(query, K))
        rec._fast = fast
        for name, over in (("single_like_64_over_plain_uncaptured", ("single_like_64_ms", "single_plain_uncaptured_ms")),
                           ("single_like_64_over_plain_graph", ("single_like_64_ms", "single_plain_graph_ms")),
                           ("similar_products_over_plain_graph", ("similar_products_ms", "single_plain_graph_ms"))):
            out[name] = round(out[over[0]]["median"] / out[over[1]]["median"], 3)
        return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--products", type=int, default=N_ROWS, help="the catalog of the whole-request part")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "compose_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("compose_bench needs an MI355X: nothing here is measured without one")
    if args.rounds < 7:
        raise SystemExit("--rounds must be at least 7: the medians are over the rounds")
    dev = torch.device("cuda", 0)
    result = {"tool": "compose_bench", "device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "k": K,
              "rounds": args.rounds, "threads_per_query": 256, "rows_in_flight_per_thread": 8,
              "cases": step_cases(args, dev), "requests": request_cases(args)}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
