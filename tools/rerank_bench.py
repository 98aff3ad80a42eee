#!/usr/bin/env python
"""Time retrieve -> rerank with the pairs assembled on the device beside the host path, in one process.

A synthetic stack at ms-marco-MiniLM-L-6's shape (hidden 384, 6 layers, both models) over --products synthetic products:
  single   RerankedRecommender.recommend(q, 10) with 100 candidates: p50 wall time of --requests requests after --warmup
           warm-ups, device_assembly=False (the host path) and the device path in alternating blocks; Recommender.recommend
           (q, 100) alone - the retrieval both share - beside them
  batch    recommend_batch of --batch queries x 20 candidates: pairs per second, wall time, the two paths alternating
  kernels  GPU time of icrec_assemble_pairs and icrec_rerank_select on their own, by HIP events, at both shapes
  slack    (ids_cap - cu[-1]) / ids_cap: the rows the host-side token bound makes icrec_score_pairs compute for nothing
Prints one JSON line and stores it (default profiles/rerank_device_bench.json).  Needs the GPU: no fallback.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def p50_blocks(paths: dict, queries: list[str], requests: int, warmup: int, blocks: int = 4) -> dict:
    """p50 / p90 wall ms per path over `requests` calls each, issued in `blocks` alternating blocks."""
    ms = {name: [] for name in paths}
    for name, fn in paths.items():
        for i in range(warmup):
            fn(queries[i % len(queries)])
    at = 0
    for _ in range(blocks):
        for name, fn in paths.items():
            for i in range(requests // blocks):
                q = queries[(at + i) % len(queries)]
                t0 = time.perf_counter()
                fn(q)  # (returns host results: the call has synchronised)
                ms[name].append((time.perf_counter() - t0) * 1e3)
        at += requests // blocks
    return {name: {"p50_ms": round(statistics.median(v), 4), "p90_ms": round(float(np.percentile(v, 90)), 4), "n": len(v)}
            for name, v in ms.items()}


def event_ms(fn, iters: int = 20, warmup: int = 3) -> float:
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(); fn(); ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return round(statistics.median(out), 4)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--products", type=int, default=49688)
    ap.add_argument("--requests", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batch-iters", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rerank_device_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rerank_bench.py needs a GPU: nothing is measured without one")
    from instacart_next_order_recommendation_amd import _native, synthetic as syn
    from instacart_next_order_recommendation_amd.model_io import (truncate_pair, write_synthetic_cross_encoder_dir,
                                                                  write_synthetic_model_dir)
    from instacart_next_order_recommendation_amd.recommender import Recommender
    from instacart_next_order_recommendation_amd.reranker import (CrossEncoderReranker, DeviceReranker, RerankBuffers,
                                                                  RerankedRecommender)

    L = _native.lib()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        n_vocab = len(syn.synthetic_vocab())
        bi_dir = write_synthetic_model_dir(tmp / "bi", seed=8, shape=syn.BertShape(vocab_size=n_vocab, layers=6))
        ce_dir = write_synthetic_cross_encoder_dir(tmp / "ce", seed=9, shape=syn.BertShape(vocab_size=n_vocab, layers=6, n_normalize=0))
        corpus = tmp / "processed" / "eval_corpus.json"
        corpus.parent.mkdir()
        corpus.write_text(json.dumps(syn.synthetic_catalog(a.products)))
        rec = Recommender(bi_dir, corpus, use_index=False)
        rr = CrossEncoderReranker(ce_dir)
    result = {"tool": "rerank_bench", "device": torch.cuda.get_device_name(0), "hidden": 384, "layers": 6, "products": a.products,
              "max_seq_length": rr.max_seq_length, "gemm_mode": rr.encoder.gemm_mode}

    # ---- single request: 100 candidates, top 10
    queries = syn.synthetic_user_contexts(64, seed=21)
    host = RerankedRecommender(rec, rr, candidates=100, device_assembly=False)
    device = RerankedRecommender(rec, rr, candidates=100)
    for q in queries[:8]:
        assert device.recommend(q, 10) == host.recommend(q, 10), "the two paths disagree"
    single = p50_blocks({"retrieval_only": lambda q: rec.recommend(q, 100), "host_assembly": lambda q: host.recommend(q, 10),
                         "device_assembly": lambda q: device.recommend(q, 10)}, queries, a.requests, a.warmup)
    dr = device._device
    q_sides = device._query_sides(queries)
    exact = cap = 0
    for q, side in zip(queries, q_sides):
        ce_bucket = 32
        while ce_bucket < len(side):
            ce_bucket *= 2
        cap += dr.token_bound([ce_bucket], 100)
        exact += sum(3 + sum(truncate_pair(len(side), len(host._product_side[pid]), rr.max_seq_length))
                     for pid, _ in rec.recommend(q, 100))
    single["slack_fraction"] = round((cap - exact) / cap, 4)
    single["mean_pair_tokens"] = round(exact / (100 * len(queries)), 1)
    single["graphs_captured"] = len(device._graphs)
    result["single_request_100_candidates_top_10"] = single

    # ---- batch: --batch queries x 20 candidates
    bq = syn.synthetic_user_contexts(a.batch, seed=22)
    host20 = RerankedRecommender(rec, rr, candidates=20, device_assembly=False)
    device20 = RerankedRecommender(rec, rr, candidates=20)
    assert device20.recommend_batch(bq[:64], 10) == host20.recommend_batch(bq[:64], 10), "the two batch paths disagree"
    secs = {"host_assembly": [], "device_assembly": []}
    for it in range(a.batch_iters + 1):  # the first round of each warms up
        for name, r in (("host_assembly", host20), ("device_assembly", device20)):
            t0 = time.perf_counter()
            r.recommend_batch(bq, 10)
            if it:
                secs[name].append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    rec.recommend_batch(bq, 20)
    retrieval_s = time.perf_counter() - t0
    b_sides = device20._query_sides(bq)
    b_lens = [len(s) for s in b_sides]
    b_cap = dr.token_bound(b_lens, 20)
    found = rec.recommend_batch(bq, 20)
    b_exact = sum(3 + sum(truncate_pair(n, len(host._product_side[pid]), rr.max_seq_length)) for n, f in zip(b_lens, found) for pid, _ in f)
    result[f"batch_{a.batch}x20"] = {
        **{name: {"s": round(statistics.median(v), 4), "s_range": [round(min(v), 4), round(max(v), 4)],
                  "pairs_per_s": round(a.batch * 20 / statistics.median(v), 1)} for name, v in secs.items()},
        "retrieval_only_s": round(retrieval_s, 4), "pairs": a.batch * 20, "bound_tokens": b_cap, "exact_tokens": b_exact,
        "slack_fraction": round((b_cap - b_exact) / b_cap, 4), "calls": len(list(device20._chunks(b_lens, 20)))}

    # ---- the two new calls on their own
    kernels = {}
    for label, sides, k, top in (("1x100", q_sides[:1], 100, 10), (f"{min(a.batch, 256)}x20", b_sides[:256], 20, 10)):
        n = len(sides)
        lens = [len(s) for s in sides]
        bufs = RerankBuffers(dr, n, k, top, dr.token_bound(lens, k))
        cu = np.zeros(n + 1, np.int32)
        np.cumsum(lens, out=cu[1:])
        q_ids = torch.from_numpy(np.concatenate(list(sides) + [np.zeros(1, np.int32)]).astype(np.int32)).cuda()
        q_cu = torch.from_numpy(cu).cuda()
        cand = torch.from_numpy(np.random.default_rng(1).integers(0, a.products, (n, k))).cuda()
        bufs.logits.copy_(torch.randn(n * k, device="cuda"))
        ptr, st = _native.ptr, _native.stream_ptr(dr.device)

        def assemble():
            _native.check(L.icrec_assemble_pairs(ptr(q_ids), ptr(q_cu), n, ptr(dr.cat_ids), ptr(dr.cat_cu), dr.n_rows, 0, ptr(cand), k,
                                                 rr.max_seq_length, rr.cls_id, rr.sep_id, ptr(bufs.ids), bufs.ids_cap, ptr(bufs.cu),
                                                 ptr(bufs.seg_b), ptr(bufs.asm_ws), bufs.asm_ws.numel(), 0, st), "icrec_assemble_pairs")

        def select():
            _native.check(L.icrec_rerank_select(ptr(bufs.logits), ptr(cand), None, n, k, top, ptr(bufs.out_idx), ptr(bufs.out_logit),
                                                0, st), "icrec_rerank_select")

        kernels[label] = {"assemble_pairs_ms": event_ms(assemble), "rerank_select_ms": event_ms(select),
                          "tokens_assembled": int(bufs.cu[-1].item()), "ids_cap": bufs.ids_cap}
    result["calls_alone_by_hip_events"] = kernels
    rr.close()
    line = json.dumps(result)
    print(line)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
