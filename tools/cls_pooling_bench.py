"""Time icrec_encode (f16x3) under the three pooling forms - mean pooling (every layer over every token), CLS pooling
with the last layer pruned to each sequence's first token, and CLS pooling with ICREC_CLS_PRUNE=0 (full last layer) -
at three shapes: all-MiniLM-L6 (6 layers, hidden 384), bge-small (12 layers, hidden 384) and bge-base (12 layers,
hidden 768), synthetic weights, on bench.py's token batch (1,024 user contexts, seed 1234: ~131 k tokens) and on a
single 128-token request.

The three encoders of a shape are timed in turn, `--reps` times over (each turn: `--steps` calls between two device
events after `--warmup` calls), so that drift of the machine falls on all three alike.  Reported per form: the median
ms per call over the turns, and the turns' min and max - the run-to-run spread that a difference has to exceed.
Prints one JSON line and stores it as profiles/cls_pooling_bench.json.

    python tools/cls_pooling_bench.py [--contexts 1024] [--steps 5] [--warmup 2] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"minilm_l6": dict(hidden=384, layers=6, heads=12, intermediate=1536),
          "bge_small_l12": dict(hidden=384, layers=12, heads=12, intermediate=1536),
          "bge_base_l12": dict(hidden=768, layers=12, heads=12, intermediate=3072)}
FORMS = ("mean", "cls_pruned", "cls_full")


def make(form: str, w, shape):
    """The encoder of a form; ICREC_CLS_PRUNE is read once, at creation."""
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

    os.environ.pop("ICREC_CLS_PRUNE", None)
    if form == "cls_full":
        os.environ["ICREC_CLS_PRUNE"] = "0"
    try:
        return DeviceEncoder(w, shape, gemm_mode="f16x3", pooling="mean" if form == "mean" else "cls")
    finally:
        os.environ.pop("ICREC_CLS_PRUNE", None)


def time_turns(encs: dict, ids, cu, steps: int, warmup: int, reps: int) -> dict:
    """form -> list of ms per call, one per turn; the forms alternate inside every turn."""
    import torch

    n, T, max_len = cu.size - 1, int(cu[-1]), int(np.diff(cu).max())
    ids_d, cu_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    out = torch.empty((n, next(iter(encs.values())).shape.hidden), device="cuda")
    for enc in encs.values():
        for _ in range(warmup):
            enc.encode_into(ids_d, cu_d, n, T, max_len, out)
    torch.cuda.synchronize()
    ms = {form: [] for form in encs}
    for _ in range(reps):
        for form, enc in encs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                enc.encode_into(ids_d, cu_d, n, T, max_len, out)
            t1.record()
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            ms[form].append(t0.elapsed_time(t1) / steps)
    return ms


def summary(turns: list) -> dict:
    return {"ms": round(float(np.median(turns)), 4), "min": round(min(turns), 4), "max": round(max(turns), 4)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--contexts", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cls_pooling_bench.json"))
    args = ap.parse_args()

    import torch

    from instacart_next_order_recommendation_amd import synthetic as syn

    assert torch.cuda.is_available(), "needs a GPU"
    ids, cu = syn.synthetic_token_batch(args.contexts, seed=1234)
    rng = np.random.default_rng(7)
    one_ids = np.concatenate([[101], rng.integers(1000, 30522, 126), [102]]).astype(np.int32)
    one_cu = np.array([0, 128], np.int32)
    res = {"tool": "cls_pooling_bench", "device": torch.cuda.get_device_name(0), "gemm_mode": "f16x3",
           "contexts": args.contexts, "tokens": int(cu[-1]), "max_seqlen": int(np.diff(cu).max()),
           "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "shapes": {}}
    for name, dims in SHAPES.items():
        shape = syn.BertShape(vocab_size=30522, **dims)
        w = syn.synthetic_bert_weights(shape, seed=0)
        encs = {form: make(form, w, shape) for form in FORMS}
        batch = time_turns(encs, ids, cu, args.steps, args.warmup, args.reps)
        single = time_turns(encs, one_ids, one_cu, max(args.steps, 50), max(args.warmup, 5), args.reps)
        for enc in encs.values():
            enc.close()
        r = {"layers": shape.layers, "hidden": shape.hidden,
             "batch": {form: summary(batch[form]) for form in FORMS},
             "single_128_tokens": {form: summary(single[form]) for form in FORMS}}
        for what in ("batch", "single_128_tokens"):
            mean, pruned = r[what]["mean"], r[what]["cls_pruned"]
            r[what]["pruned_saving_ms"] = round(mean["ms"] - pruned["ms"], 4)
            r[what]["pruned_saving_frac"] = round(1.0 - pruned["ms"] / mean["ms"], 4)
            # acceptance: not slower than the mean call of the same run, given the mean call's own spread
            r[what]["pruned_not_slower"] = bool(pruned["ms"] <= mean["ms"] + (mean["max"] - mean["min"]))
        res["shapes"][name] = r
    line = json.dumps(res)
    print(line)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
