"""Host wall time of single requests through MonitoredRecommender.recommend, per request feature -> one JSON line.

A synthetic 2-layer model, 20,000 products, an IVF index of 16 lists and two product sets; one user context, top 20.
Per case the p50 of 300 requests after 30 warm-ups (ms): `plain_graph` passes no option (the replayed graphs), the
others take the un-captured path; `batch32_diversity` is recommend_batch of 32 queries (p50 of 100).  The requests are
far shorter than a millisecond, so the figures compare host code, not kernels.

    python tools/request_host_bench.py [--package-root DIR] [--label NAME]

--package-root: the checkout whose package is timed (default: this one) - for runs that alternate two checkouts, each
in a process of its own (profiles/request_plan_refactor.md)."""
from __future__ import annotations

import argparse
import json
import logging
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=str(Path(__file__).resolve().parents[1]))
ap.add_argument("--label", default=None)
args = ap.parse_args()
sys.path.insert(0, str(Path(args.package_root).resolve()))

from instacart_next_order_recommendation_amd import synthetic as syn  # noqa: E402
from instacart_next_order_recommendation_amd.model_io import write_synthetic_model_dir  # noqa: E402
from instacart_next_order_recommendation_amd.recommender import MonitoredRecommender  # noqa: E402

N = 20000


def p50(fn, n=330, warm=30):
    lat = []
    for _ in range(n):
        a = time.perf_counter()
        fn()
        lat.append((time.perf_counter() - a) * 1e3)
    return round(float(np.median(lat[warm:])), 4)


def main(root: Path):
    shape = syn.BertShape(vocab_size=len(syn.synthetic_vocab()), layers=2)
    model_dir = write_synthetic_model_dir(root / "model", seed=3, shape=shape)
    (root / "processed").mkdir()
    corpus = root / "processed" / "eval_corpus.json"
    corpus.write_text(json.dumps(syn.synthetic_catalog(N)))
    logging.getLogger("recommender.metrics").setLevel(logging.WARNING)
    sets = {"store": [str(i) for i in range(1, N + 1) if i % 3], "stock": [str(i) for i in range(1, N + 1) if i % 2 == 0]}
    rec = MonitoredRecommender(model_dir, corpus, use_index=False, ann_lists=16, product_sets=sets)
    text = syn.synthetic_user_contexts(4, seed=77)[1]
    cases = {
        "plain_graph": {},
        "diversity": dict(diversity=0.3),
        "max_per_aisle": dict(max_per_aisle=2),
        "departments": dict(departments=rec.departments[:5]),
        "within_boosts": dict(within="store", boosts=rec.product_ids[5:2000:50], boost_weight=0.2),
        "probes": dict(probes=4),
        "caps_diversity": dict(max_per_department=3, diversity=0.3),
    }
    out = {"label": args.label or Path(args.package_root).name}
    for name, kw in cases.items():
        out["p50_ms_" + name] = p50(lambda: rec.recommend(text, 20, user_id="bench", **kw))
    out["p50_ms_batch32_diversity"] = p50(lambda: rec.recommend_batch([text] * 32, 20, diversity=0.3), n=130)
    print(json.dumps(out))


if __name__ == "__main__":
    with tempfile.TemporaryDirectory(prefix="icrec_request_host_") as tmp:
        main(Path(tmp))
