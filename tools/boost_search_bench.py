#!/usr/bin/env python3
"""What boosting a query's listed rows costs next to the search it follows, on the bench catalog (49,688 x 384 rows of
synthetic.synthetic_embeddings, "f32" storage) at k = top_k = 20, Q = 1 and Q = 1,024, lists of 64 and of 1,024 rows per
query (a quarter of each from the query's own top 40, the rest random; weights in [0, 0.6], every 7th 0).

    python tools/boost_search_bench.py [--rounds 7] [--out profiles/boost_search_bench.json]

Per case, timed in ONE process on one build and alternated round by round after a warm-up of every version:
  search          icrec_search at k = 20 (the plain request; unchanged by this feature)
  search_boost    that search followed by icrec_boost_select (the boosted request)
  boost           icrec_boost_select alone on that search's result
  only            icrec_boost_select without candidates (buy it again: the listed rows alone)
Times are per call, from HIP events around a window of back-to-back calls (about 0.1 s of work); per version the median,
minimum and maximum over the rounds.  boost's two kernels come from the library's launch timers (icrec_timing_query
slots 7 and 8: events around each launch) over a separate run of 200 calls.  There is no pass / fail bar:
boost_over_search is reported as measured.  One JSON line on stdout, also written to --out."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from instacart_next_order_recommendation_amd import _native, synthetic  # noqa: E402
from instacart_next_order_recommendation_amd.search import DeviceIndex  # noqa: E402

N_ROWS, DIM, STORAGE, K = 49688, 384, "f32", 20
CASES = [(1, 64), (1, 1024), (1024, 64), (1024, 1024)]  # (Q, listed rows per query)
T_BOOST_SCORE, T_BOOST_SELECT = 7, 8


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def draw_lists(rng, top, n_rows, length):
    """CSR (off int32 [Q+1], rows int32, w float32) of one list of `length` rows per query."""
    rows, w = [], []
    for t in top:
        own = rng.choice(t, min(length // 4, t.size), replace=False)
        rest = rng.choice(n_rows, length, replace=False)
        rest = rest[~np.isin(rest, own)][:length - own.size]
        rows.append(np.sort(np.concatenate([own, rest])))
        x = rng.uniform(0.0, 0.6, length).astype(np.float32)
        x[::7] = 0
        w.append(x)
    off = np.arange(len(top) + 1, dtype=np.int32) * length
    return off, np.concatenate(rows).astype(np.int32), np.concatenate(w)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "boost_search_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("boost_search_bench needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    ix = DeviceIndex(synthetic.synthetic_embeddings(args.rows, DIM, seed=1), dev, storage=STORAGE)
    rng = np.random.default_rng(5)

    def buffers(Q, k):
        return torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev)

    cases = []
    for Q, length in CASES:
        q = torch.from_numpy(synthetic.synthetic_embeddings(Q, DIM, seed=7 + Q)).to(dev)
        plain, plain2, out, out2, only = buffers(Q, K), buffers(Q, K), buffers(Q, K), buffers(Q, K), buffers(Q, K)
        top = ix.search(q, 2 * K)[0].cpu().numpy()
        off, rows, w = (torch.from_numpy(a).to(dev) for a in draw_lists(rng, top, args.rows, length))
        ix.search_into(q, K, None, None, *plain)  # boost alone reads this result

        def boost(cand, dst):
            ix.boost_select_into(q, cand[0], cand[1], off, rows, w, length, K, None, None, None, *dst)

        def search_boost():
            ix.search_into(q, K, None, None, *plain2)
            boost(plain2, out2)

        versions = {"search": lambda: ix.search_into(q, K, None, None, *plain2), "search_boost": search_boost,
                    "boost": lambda: boost(plain, out), "only": lambda: boost((None, None), only)}
        iters = {}
        for name, fn in versions.items():  # warm-up of this shape, and the window length per version
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[name] = int(min(max(100.0 / max(window_ms(fn, 5), 1e-3), 5), 4000))
        assert torch.equal(out[0], out2[0]) and torch.equal(out[1], out2[1]), (Q, length)
        ms = {name: [] for name in versions}
        for _ in range(args.rounds):  # alternated: one window of every version per round
            for name, fn in versions.items():
                ms[name].append(window_ms(fn, iters[name]))
        torch.cuda.synchronize()
        _native.timing_reset()
        _native.timing_enable(True)
        try:
            for _ in range(200):
                versions["boost"]()
            torch.cuda.synchronize()
        finally:
            _native.timing_enable(False)
        score_ms, score_n = _native.timing_query(T_BOOST_SCORE)
        select_ms, select_n = _native.timing_query(T_BOOST_SELECT)
        _native.timing_reset()
        changed = int((out[0] != plain[0]).any(dim=1).sum().item())
        row = {"Q": Q, "listed_rows_per_query": length, "k": K, "top_k": K, "lists_changed_by_boosts": changed}
        for name, t in ms.items():
            row[name + "_ms"] = {"median": round(float(np.median(t)), 5), "min": round(min(t), 5), "max": round(max(t), 5),
                                 "calls_per_window": iters[name]}
        row["boost_kernels_ms"] = {"score": round(score_ms, 5), "select": round(select_ms, 5),
                                   "launches_each": int(min(score_n, select_n))}
        row["boost_over_search"] = round(row["boost_ms"]["median"] / row["search_ms"]["median"], 3)
        row["boosted_over_plain"] = round(row["search_boost_ms"]["median"] / row["search_ms"]["median"], 3)
        cases.append(row)
    result = {"tool": "boost_search_bench", "device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM,
              "storage": STORAGE, "rounds": args.rounds, "cases": cases}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    ix.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
