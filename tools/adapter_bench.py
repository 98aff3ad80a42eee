#!/usr/bin/env python3
"""What the query adapter costs: icrec_adapter_apply beside the search it feeds, one training step, and a whole adapted
request beside the plain one.

    python tools/adapter_bench.py [--rounds 7] [--out profiles/adapter_bench.json]

In ONE process, on the bench catalog (49,688 x 384 rows of synthetic.synthetic_embeddings), timed after a warm-up of
every version and alternated round by round:
  apply   icrec_adapter_apply at n = 1 and n = 1,024 (a random adapter of width 384), beside
  search  icrec_search at k = 20 on the adapted queries, storage "f32+filter"
  step    icrec_adapter_step with update = 1 at (B 256, C 256) and (B 1,024, C 8,192), on fp32 and on bf16 rows; step_gflop
          counts the products - S = U V^T in both sweeps and P V (3 x 2 B C d), the apply and dD (2 x 2 B d d) - and
          step_tflops is that over the median time, beside the 157 TFLOPS of the f32 MFMA
Times are per call, from HIP events around a window of back-to-back calls (about 0.1 s of work, at least 5 calls); per
version the median, minimum and maximum over the rounds.
Whole requests, on a Recommender over a synthetic catalog of --products products (a 2-layer synthetic model):
recommend(q, 20) on the graph path without an adapter and with a random one (one more node in the captured chain); host
wall clock around the call, which returns after the read-back; median, minimum and maximum over --rounds calls after a
warm-up call.
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
from instacart_next_order_recommendation_amd.adapter import QueryAdapter  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex  # noqa: E402

N_ROWS, DIM, K = 49688, 384, 20
F32_MFMA_TFLOPS = 157.3


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


def timed(versions, rounds):
    """{name: callable} -> {name: spread + calls_per_window}: warm-up, then one window of every version per round."""
    iters = {}
    for name, fn in versions.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[name] = int(min(max(100.0 / max(window_ms(fn, 5), 1e-3), 5), 4000))
    ms = {name: [] for name in versions}
    for _ in range(rounds):
        for name, fn in versions.items():
            ms[name].append(window_ms(fn, iters[name]))
    torch.cuda.synchronize()
    return {name: dict(spread(t), calls_per_window=iters[name]) for name, t in ms.items()}


def random_adapter(dev, seed=0) -> QueryAdapter:
    ad = QueryAdapter(DIM, dev)
    ad.load_state({"delta": (np.random.default_rng(seed).standard_normal((DIM, DIM)) * (0.05 / np.sqrt(DIM))).astype(np.float32)})
    return ad


def apply_cases(args, dev, rows):
    ix = DeviceIndex(rows, dev, storage="f32+filter")
    ad = random_adapter(dev)
    cases = []
    for n in (1, 1024):
        q = torch.from_numpy(synthetic.synthetic_embeddings(n, DIM, seed=7 + n)).to(dev)
        out = torch.empty_like(q)
        idx = torch.empty((n, K), dtype=torch.int64, device=dev)
        sc = torch.empty((n, K), dtype=torch.float32, device=dev)
        t = timed({"apply": lambda: ad.apply_into(q, out), "search": lambda: ix.search_into(out, K, None, None, idx, sc)},
                  args.rounds)
        cases.append({"n": n, "apply_ms": t["apply"], "search_ms": t["search"],
                      "apply_over_search": round(t["apply"]["median"] / t["search"]["median"], 4)})
    ix.close()
    return cases


def step_cases(args, dev, rows):
    rng = np.random.default_rng(1)
    cases = []
    for storage in ("f32", "bf16"):
        ix = DeviceIndex(rows, dev, storage=storage)
        for B, n_cand in ((256, 256), (1024, 8192)):
            ad = random_adapter(dev)
            anchors = torch.from_numpy(synthetic.synthetic_embeddings(B, DIM, seed=3 + B)).to(dev)
            cand = torch.from_numpy(rng.choice(args.rows, n_cand, replace=False).astype(np.int32)).to(dev)
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            t = timed({"step": lambda: ad.step(ix, anchors, cand, 1e-4, loss_out=loss)}, args.rounds)["step"]
            gflop = (3 * 2.0 * B * n_cand * DIM + 2 * 2.0 * B * DIM * DIM) / 1e9
            cases.append({"storage": storage, "dim": DIM, "B": B, "C": n_cand, "step_ms": t, "step_gflop": round(gflop, 3),
                          "step_tflops": round(gflop / t["median"], 2), "f32_mfma_tflops": F32_MFMA_TFLOPS,
                          "loss_finite": bool(torch.isfinite(loss).all())})
        ix.close()
    return cases


def request_cases(args):
    from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir
    from instacart_next_order_recommendation_amd.recommender import Recommender

    def wall(fn):
        fn()  # warm-up: the graph capture
        t = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1000)
        return spread(t)

    with tempfile.TemporaryDirectory(prefix="icrec_adapter_bench_") as tmp:
        tmp = Path(tmp)
        shape = synthetic.BertShape(vocab_size=len(synthetic.synthetic_vocab()), layers=2)
        model_dir = write_synthetic_model_dir(tmp / "model", seed=3, shape=shape)
        corpus_path = tmp / "processed" / "eval_corpus.json"
        corpus_path.parent.mkdir()
        corpus_path.write_text(json.dumps(synthetic.synthetic_catalog(args.products)))
        rec = Recommender(model_dir, corpus_path, use_index=False)
        query = synthetic.synthetic_user_contexts(1, seed=21)[0]
        out = {"products": args.products, "model_layers": 2, "top_k": K, "storage": rec._index.storage,
               "single_plain_graph_ms": wall(lambda: rec.recommend(query, K))}
        rec.set_adapter(random_adapter(rec.device))
        out["single_adapted_graph_ms"] = wall(lambda: rec.recommend(query, K))
        out["adapted_over_plain_graph"] = round(out["single_adapted_graph_ms"]["median"] / out["single_plain_graph_ms"]["median"], 3)
        return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--products", type=int, default=10000, help="the catalog of the whole-request part")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "adapter_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("adapter_bench needs an MI355X: nothing here is measured without one")
    if args.rounds < 7:
        raise SystemExit("--rounds must be at least 7: the medians are over the rounds")
    dev = torch.device("cuda", 0)
    rows = synthetic.synthetic_embeddings(args.rows, DIM, seed=1)
    result = {"tool": "adapter_bench", "device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "k": K,
              "rounds": args.rounds, "apply": apply_cases(args, dev, rows), "step": step_cases(args, dev, rows),
              "requests": request_cases(args)}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
