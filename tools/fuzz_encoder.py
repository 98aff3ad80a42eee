#!/usr/bin/env python3
"""Randomised parity sweep of the encoder against the oracle: random batch compositions (1..200 sequences of
1..256 tokens, incl. the 512-token boundary between the small-M and batch GEMM kernels and all four attention
length buckets), both gemm modes; also checks that every sequence encodes to the same bits alone and in the batch,
and every token's last hidden state against the float64 reference (oracle/float64_reference.py) within the margins of
tests/token_states.py x the oracle's own error on the same case.
usage: python tools/fuzz_encoder.py [n_cases] [seed]"""
import sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np, torch
from oracle import oracle as o, float64_reference as f64
from tests import token_states as ts
from instacart_next_order_recommendation_amd import synthetic as syn
from instacart_next_order_recommendation_amd.encoder import DeviceEncoder

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
shape = syn.BertShape()
w = syn.synthetic_bert_weights(shape, seed=0)
cfg = o.cfg_for(shape)
o.set_threads(o.usable_cpus())
encs = {m: DeviceEncoder(w, shape, "cuda:0", gemm_mode=m) for m in ("f16x3", "f32")}
ref64 = f64.Float64Bert(w, shape)
margins = {m: ts.MARGINS[(m, shape.hidden, "standard")] for m in encs}  # per mode the looser of the two weight sets at 384
worst = {m: 0.0 for m in encs}
worst_tok = {m: (0.0, 0.0) for m in encs}  # worst E_gpu / E_ref of the token states: (row rms, max abs)
bad = 0
t0 = time.time()
for case in range(n_cases):
    n = int(rng.choice([1, 2, 3, 7, 20, 60, 200]))
    style = rng.choice(["short", "mixed", "long", "edge"])
    if style == "short": lens = rng.integers(1, 33, n)
    elif style == "long": lens = rng.integers(129, 257, n)
    elif style == "edge": lens = rng.choice([1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256], n)
    else: lens = rng.integers(1, 257, n)
    while lens.sum() > 12000: lens = lens[:-1]
    n = len(lens)
    cu = np.zeros(n + 1, np.int32); cu[1:] = np.cumsum(lens)
    ids = rng.integers(0, shape.vocab_size, int(cu[-1])).astype(np.int32)
    want, ora_h = o.encode(w, cfg, ids, cu, return_hidden=True)
    want_h, _ = ref64.encode(ids, cu)
    e_rms, e_abs = ts.row_errors(ora_h, want_h)
    for m, enc in encs.items():
        got, tok = enc.encode_packed(torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), int(lens.max()),
                                     return_tokens=True)
        got, tok = got.cpu().numpy(), tok.cpu().numpy()
        err = float(np.abs(got - want).max())
        worst[m] = max(worst[m], err)
        g_rms, g_abs = ts.row_errors(tok, want_h)
        worst_tok[m] = (max(worst_tok[m][0], g_rms / e_rms), max(worst_tok[m][1], g_abs / e_abs))
        if not (np.isfinite(tok).all() and g_rms <= margins[m][0] * e_rms and g_abs <= margins[m][1] * e_abs):
            bad += 1
            print(f"MISMATCH case {case} mode={m} n={n} tokens={int(cu[-1])} style={style} token states: "
                  f"E_gpu / E_ref rms {g_rms / e_rms:.2f} abs {g_abs / e_abs:.2f} (margins {margins[m]}); "
                  + ts.worst_element(tok, want_h, cu), flush=True)
        s = int(rng.integers(0, n))
        one = enc.encode_packed(torch.from_numpy(ids[cu[s]:cu[s + 1]].copy()).cuda(),
                                torch.tensor([0, int(lens[s])], dtype=torch.int32).cuda(), int(lens[s])).cpu().numpy()[0]
        if err > 5e-6 or not np.array_equal(one, got[s]) or not np.isfinite(got).all():
            bad += 1
            print(f"MISMATCH case {case} mode={m} n={n} tokens={int(cu[-1])} style={style} err={err:.3g} "
                  f"alone_equal={np.array_equal(one, got[s])}", flush=True)
print(f"{n_cases} cases, {bad} mismatches, worst |d emb| {worst}, worst token-state E_gpu / E_ref (row rms, max abs) "
      f"{ {m: (round(a, 2), round(b, 2)) for m, (a, b) in worst_tok.items()} }, {time.time() - t0:.1f}s")
sys.exit(1 if bad else 0)
