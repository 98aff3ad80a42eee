"""Time icrec_encode with and without a relative-position attention bias (icrec_encoder_set_attention_bias), in both
GEMM modes, at two shapes: all-mpnet-base-v2's (hidden 768, 12 layers) and all-MiniLM-L6's (hidden 384, 6 layers),
synthetic weights, a dense table uniform in [-4, 4], on bench.py's token batch (1,024 user contexts, seed 1234: ~131 k
tokens).

The two encoders of a (shape, mode) are timed in turn, `--reps` times over (each turn: `--steps` calls between two
device events after `--warmup` calls), so that drift of the machine falls on both alike.  Reported per form: the median
ms per call over the turns and the turns' min and max - the run-to-run spread a difference has to exceed - and the cost
of the bias per layer, (biased - unbiased) / layers.  With `--kernel-trace` every (shape, mode, form) also runs once in a
fresh child process under `rocprofv3 --kernel-trace --stats`, and the attention kernels' time per layer is read from its
kernel statistics.  Prints one JSON line and stores it as profiles/attention_bias_bench.json.

    python tools/attention_bias_bench.py [--contexts 1024] [--steps 5] [--warmup 2] [--reps 5] [--kernel-trace]
"""
from __future__ import annotations

import argparse
import csv
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"mpnet_base_l12": dict(hidden=768, layers=12, heads=12, intermediate=3072),
          "minilm_l6": dict(hidden=384, layers=6, heads=12, intermediate=1536)}
MODES = ("f16x3", "f32")
FORMS = ("unbiased", "biased")


def make(form: str, w, shape, mode: str):
    from instacart_next_order_recommendation_amd.encoder import DeviceEncoder
    from tests import relative_bias as tb

    return DeviceEncoder(w, shape, gemm_mode=mode, attention_bias=tb.table("dense", shape.heads) if form == "biased" else None)


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


def child(name: str, mode: str, form: str, contexts: int, calls: int) -> None:
    """What runs under rocprofv3: `calls` encodes of one (shape, mode, form), nothing else."""
    import torch

    from instacart_next_order_recommendation_amd import synthetic as syn

    shape = syn.BertShape(vocab_size=30522, **SHAPES[name])
    enc = make(form, syn.synthetic_bert_weights(shape, seed=0), shape, mode)
    ids, cu = syn.synthetic_token_batch(contexts, seed=1234)
    ids_d, cu_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    out = torch.empty((cu.size - 1, shape.hidden), device="cuda")
    for _ in range(calls):
        enc.encode_into(ids_d, cu_d, cu.size - 1, int(cu[-1]), int(np.diff(cu).max()), out)
    torch.cuda.synchronize()
    enc.close()


def attention_ms_per_layer(name: str, mode: str, form: str, contexts: int, calls: int = 3):
    """Sum of the attention kernels' durations per call and layer (ms) from a kernel trace of a child process; a string
    naming what went wrong when the profiler's output could not be read."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--",
               sys.executable, __file__, "--child", name, mode, form, "--contexts", str(contexts), "--calls", str(calls)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return f"rocprofv3 exited {r.returncode}: {r.stderr[-300:]}"
        files = sorted(Path(d).rglob("*kernel_stats.csv"))
        if not files:
            return "no kernel_stats.csv"
        total_ns = 0.0
        for row in csv.DictReader(files[0].open()):
            if "attention" in row.get("Name", "") and "kernel" in row.get("Name", ""):
                total_ns += float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
        return round(total_ns * 1e-6 / calls / SHAPES[name]["layers"], 4)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--contexts", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--child", nargs=3, metavar=("SHAPE", "MODE", "FORM"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attention_bias_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child, args.contexts, args.calls)

    import torch

    from instacart_next_order_recommendation_amd import synthetic as syn

    assert torch.cuda.is_available(), "needs a GPU"
    ids, cu = syn.synthetic_token_batch(args.contexts, seed=1234)
    res = {"tool": "attention_bias_bench", "device": torch.cuda.get_device_name(0), "contexts": args.contexts,
           "tokens": int(cu[-1]), "max_seqlen": int(np.diff(cu).max()), "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "table": "dense, uniform in [-4, 4]", "shapes": {}}
    for name, dims in SHAPES.items():
        shape = syn.BertShape(vocab_size=30522, **dims)
        w = syn.synthetic_bert_weights(shape, seed=0)
        res["shapes"][name] = {"layers": shape.layers, "hidden": shape.hidden}
        for mode in MODES:
            encs = {form: make(form, w, shape, mode) for form in FORMS}
            turns = time_turns(encs, ids, cu, args.steps, args.warmup, args.reps)
            for enc in encs.values():
                enc.close()
            r = {form: summary(turns[form]) for form in FORMS}
            r["bias_cost_ms_per_layer"] = round((r["biased"]["ms"] - r["unbiased"]["ms"]) / shape.layers, 4)
            r["bias_cost_frac"] = round(r["biased"]["ms"] / r["unbiased"]["ms"] - 1.0, 4)
            r["unbiased_spread_ms"] = round(r["unbiased"]["max"] - r["unbiased"]["min"], 4)
            if args.kernel_trace:
                r["attention_kernels_ms_per_layer"] = {form: attention_ms_per_layer(name, mode, form, args.contexts)
                                                       for form in FORMS}
            res["shapes"][name][mode] = r
    line = json.dumps(res)
    print(line)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
