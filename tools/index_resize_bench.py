#!/usr/bin/env python3
"""What adding and removing rows of an index in place costs, beside building it again.

    python tools/index_resize_bench.py [--rounds 7] [--out profiles/index_resize_bench.json] [--big-rows 10000000]

Part 1, icrec_index_append_rows / _remove_rows / _reserve on synthetic rows (normal deviates made on the device), in one
process per catalog, every catalog reserved with headroom first (n_rows + 4,096):
  49,688 x 384 "f32+filter"  and  10 M x 384 "bf16+filter":    m = 1, 64 and 1,024
A round appends m rows and then removes m random rows of the longer index, so the index has n_rows rows again.  Per m and
call: the time of the call's work on the stream from HIP events around it (append: the facet-free write kernel; remove:
the plan's host-to-device copy, the move kernel and the clear kernel) and the host wall clock around call + synchronize,
median / min / max over --rounds rounds after a warm-up round.  `reserve` itself (to n_rows + 8,192 and back to
n_rows + 4,096, wall clock, all rounds), and icrec_index_create_ex of the same catalog from rows already on the device
(DeviceIndex(...): allocation, normalisation, filter copy, synchronize), wall clock, same rounds: the thing they replace.
Part 2, Recommender.add_products and remove_products of 64 products of a 49,688-product synthetic catalog on a synthetic
2-layer model (wall clock, --rounds calls each with fresh ids, after a warm-up pair), beside building a new Recommender
on the same model and catalog (wall clock, once after a warm-up build; use_index=False: every text is encoded).
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
from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir  # noqa: E402
from instacart_next_order_recommendation_amd.recommender import Recommender  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex  # noqa: E402

DIM, HEADROOM = 384, 4096


def spread(t):
    return {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def wall_ms(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1000


def timed(fn, dev):
    """fn() once -> (ms between HIP events around its work on the current stream, host wall ms of call + synchronize)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1000


def resize_case(n_rows, storage, ms_list, rounds, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(n_rows)
    rows = torch.randn((n_rows, DIM), generator=gen, device=dev, dtype=torch.float32)
    create = []
    ix = None
    for _ in range(rounds + 1):  # the first build is the warm-up
        if ix is not None:
            ix.close()
        holder = {}
        create.append(wall_ms(lambda: holder.setdefault("ix", DeviceIndex(rows, dev, storage=storage)), dev))
        ix = holder["ix"]
    ix.reserve(n_rows + HEADROOM)
    reserve = []
    for _ in range(rounds):
        reserve.append(wall_ms(lambda: ix.reserve(n_rows + 2 * HEADROOM), dev))
        reserve.append(wall_ms(lambda: ix.reserve(n_rows + HEADROOM), dev))
    out = {"rows": n_rows, "dim": DIM, "storage": storage, "capacity": ix.capacity,
           "index_create_wall_ms": spread(create[1:]), "reserve_wall_ms": spread(reserve), "resizes": []}
    rng = np.random.default_rng(n_rows)
    for m in ms_list:
        new = torch.randn((m, DIM), generator=gen, device=dev, dtype=torch.float32)
        t = {"append": [], "remove": []}
        for r in range(rounds + 1):  # the first round is the warm-up
            ids = rng.choice(n_rows + m, m, replace=False)
            app = timed(lambda: ix.append_rows(new), dev)
            rem = timed(lambda: ix.remove_rows(ids), dev)
            assert ix.n_rows == n_rows and ix.capacity == n_rows + HEADROOM
            if r:
                t["append"].append(app)
                t["remove"].append(rem)
        entry = {"m": m}
        for what, pairs in t.items():
            entry[what] = {"device_ms": spread([p[0] for p in pairs]), "wall_ms": spread([p[1] for p in pairs]),
                           "wall_over_index_create": round(float(np.median([p[1] for p in pairs])) /
                                                           out["index_create_wall_ms"]["median"], 5)}
        out["resizes"].append(entry)
    ix.close()
    return out


def recommender_case(n_products, n_edits, rounds, dev):
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        shape = synthetic.BertShape(vocab_size=len(synthetic.synthetic_vocab()), layers=2)
        model_dir = write_synthetic_model_dir(tmp / "model", seed=3, shape=shape)
        corpus = synthetic.synthetic_catalog(n_products)
        corpus_path = tmp / "processed" / "eval_corpus.json"
        corpus_path.parent.mkdir()
        corpus_path.write_text(json.dumps(corpus))
        rec = Recommender(model_dir, corpus_path, use_index=False)  # the warm-up build, and the one that is edited
        t0 = time.perf_counter()
        other = Recommender(model_dir, corpus_path, use_index=False)
        torch.cuda.synchronize(dev)
        build_ms = (time.perf_counter() - t0) * 1000
        del other
        rec._index.reserve(n_products + HEADROOM)
        texts = [corpus[p] for p in list(corpus)[:: max(n_products // n_edits, 1)][:n_edits]]
        add, remove = [], []
        for r in range(rounds + 1):  # the first pair is the warm-up
            additions = {f"new-{r}-{i}": t.replace("Product: ", f"Product: Round{r} ", 1) for i, t in enumerate(texts)}
            gone = [rec.product_ids[i] for i in range(r, n_products, max(n_products // n_edits, 1))][:n_edits]
            add.append(wall_ms(lambda: rec.add_products(additions), dev))
            remove.append(wall_ms(lambda: rec.remove_products(gone), dev))
        assert len(rec.product_ids) == n_products == rec._index.n_rows
        return {"products": n_products, "edited": len(texts), "model_layers": 2, "storage": rec._index.storage,
                "add_products_wall_ms": spread(add[1:]), "remove_products_wall_ms": spread(remove[1:]),
                "new_recommender_wall_ms": round(build_ms, 1),
                "add_over_new_recommender": round(float(np.median(add[1:])) / build_ms, 5),
                "remove_over_new_recommender": round(float(np.median(remove[1:])) / build_ms, 5)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--big-rows", type=int, default=10_000_000)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "index_resize_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("index_resize_bench needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    catalogs = [resize_case(49688, "f32+filter", [1, 64, 1024], args.rounds, dev)]
    if args.big_rows > 0:
        catalogs.append(resize_case(args.big_rows, "bf16+filter", [1, 64, 1024], args.rounds, dev))
    result = {"tool": "index_resize_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "resize": catalogs, "add_remove_products": recommender_case(49688, 64, args.rounds, dev)}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
