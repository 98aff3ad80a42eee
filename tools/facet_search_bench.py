#!/usr/bin/env python3
"""Faceted search against its alternatives, on the bench catalog (49,688 x 384, "f32+filter", k = 20) at Q = 1 and
Q = 1,024, with masks that admit everything, one department of 21 and one aisle of 134 (per query its own).

    python tools/facet_search_bench.py [--parent-lib PATH/libicrec.so] [--rounds 7] [--out profiles/facet_search_bench.json]

Versions, timed in ONE process and alternated round by round after a warm-up of every shape:
  a         icrec_search, no restriction (what the restriction costs is c / a)
  a_parent  the same call into a second libicrec.so, built from the parent commit (--parent-lib; left out without it)
  b         the only route to the restricted result without facets: icrec_search with every inadmissible row in a
            prebuilt device exclusion CSR; the host time to build that CSR is reported separately (b_host_csr_ms)
  c         icrec_search_faceted with the masks
b and c must return the same bits (asserted), as must a and a_parent.  Times are per call, from HIP events around a
window of back-to-back calls (at least ~0.1 s of work); per version the median, minimum and maximum over the rounds.
One JSON line on stdout, also written to --out."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from instacart_next_order_recommendation_amd import _native, synthetic  # noqa: E402
from instacart_next_order_recommendation_amd.recommender import catalog_facets  # noqa: E402
from instacart_next_order_recommendation_amd.search import ROW_STORAGE, DeviceIndex, facet_masks  # noqa: E402

N_ROWS, DIM, K, STORAGE = 49688, 384, 20, "f32+filter"


class ParentIndex:
    """The same rows behind a second libicrec.so (the parent commit's build): create, search, destroy."""

    def __init__(self, path: str, rows: torch.Tensor):
        _native.lib()  # torch's HIP runtime first, as for the library under test
        vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
        L = self.L = C.CDLL(path)
        L.icrec_index_create_ex.argtypes, L.icrec_index_create_ex.restype = [vp, i64, i32, i64, C.c_int, i32, C.POINTER(vp)], C.c_int
        L.icrec_search_workspace_bytes.argtypes, L.icrec_search_workspace_bytes.restype = [vp, i32, i32], sz
        L.icrec_search.argtypes, L.icrec_search.restype = [vp, vp, i32, i32, vp, vp, vp, vp, vp, sz, vp], C.c_int
        L.icrec_index_destroy.argtypes, L.icrec_index_destroy.restype = [vp], C.c_int
        self.device = rows.device
        self.h = vp()
        torch.cuda.synchronize()
        rc = L.icrec_index_create_ex(rows.data_ptr(), rows.shape[0], rows.shape[1], 0, rows.device.index, ROW_STORAGE[STORAGE],
                                     C.byref(self.h))
        assert rc == 0, rc
        self.ws = {}

    def search_into(self, q, k, idx, sc):
        Q = q.shape[0]
        if Q not in self.ws:
            self.ws[Q] = torch.empty(self.L.icrec_search_workspace_bytes(self.h, Q, k), dtype=torch.uint8, device=self.device)
        ws = self.ws[Q]
        rc = self.L.icrec_search(self.h, q.data_ptr(), Q, k, None, None, idx.data_ptr(), sc.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream(self.device).cuda_stream)
        assert rc == 0, rc

    def close(self):
        self.L.icrec_index_destroy(self.h)


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent-lib", default=None, help="libicrec.so built from the parent commit (version a_parent)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N_ROWS)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "facet_search_bench.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("facet_search_bench needs an MI355X: nothing here is measured without one")
    dev = torch.device("cuda", 0)
    n = args.rows

    P = synthetic.synthetic_embeddings(n, DIM, seed=1)
    aisles, departments, codes = catalog_facets(list(synthetic.synthetic_catalog(n).values()))
    ix = DeviceIndex(P, dev, storage=STORAGE)
    ix.set_facets(codes)
    parent = ParentIndex(args.parent_lib, torch.from_numpy(P).to(dev)) if args.parent_lib else None

    shapes = []
    for Q in (1, 1024):
        q = torch.from_numpy(synthetic.synthetic_embeddings(Q, DIM, seed=7 + Q)).to(dev)
        out = {v: (torch.empty((Q, K), dtype=torch.int64, device=dev), torch.empty((Q, K), dtype=torch.float32, device=dev))
               for v in "apbc"}
        for mask_name in ("all", "department", "aisle"):
            if mask_name == "all":
                allow = [None] * Q
                admitted = np.ones((Q, n), bool)
            else:
                f, n_values = (1, len(departments)) if mask_name == "department" else (0, len(aisles))
                values = [(3 + 5 * i) % n_values for i in range(Q)]
                allow = [[[v], None] if f == 0 else [None, [v]] for v in values]
                admitted = codes[None, :, f] == np.asarray(values, np.uint8)[:, None]
            masks = facet_masks(allow, Q, 2, dev)
            t0 = time.perf_counter()
            off = np.zeros(Q + 1, np.int32)
            rej = [np.flatnonzero(~row).astype(np.int32) for row in admitted]
            off[1:] = np.cumsum([len(r) for r in rej])
            flat = np.concatenate(rej) if off[-1] else np.zeros(0, np.int32)
            host_csr_ms = (time.perf_counter() - t0) * 1000
            ei, eo = (torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev)) if off[-1] else (None, None)

            versions = {"a": lambda: ix.search_into(q, K, None, None, *out["a"]),
                        "b": lambda: ix.search_into(q, K, ei, eo, *out["b"]),
                        "c": lambda: ix.search_into(q, K, None, None, *out["c"], allow=masks)}
            if parent:
                versions["a_parent"] = lambda: parent.search_into(q, K, *out["p"])
            iters = {}
            for name, fn in versions.items():  # warm-up of this shape, and the window length per version
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                iters[name] = int(min(max(100.0 / max(window_ms(fn, 5), 1e-3), 5), 4000))
            assert torch.equal(out["b"][0], out["c"][0]) and torch.equal(out["b"][1], out["c"][1]), (Q, mask_name)
            if parent:
                assert torch.equal(out["a"][0], out["p"][0]) and torch.equal(out["a"][1], out["p"][1]), (Q, mask_name)
            if mask_name == "all":
                assert torch.equal(out["a"][0], out["c"][0]) and torch.equal(out["a"][1], out["c"][1])
            ms = {name: [] for name in versions}
            for _ in range(args.rounds):  # alternated: one window of every version per round
                for name, fn in versions.items():
                    ms[name].append(window_ms(fn, iters[name]))
            row = {"Q": Q, "mask": mask_name, "excluded_ids_b": int(off[-1]), "b_host_csr_ms": round(host_csr_ms, 3),
                   "found": int((out["c"][0] >= 0).sum().item())}
            for name, t in ms.items():
                row[name + "_ms"] = {"median": round(float(np.median(t)), 5), "min": round(min(t), 5), "max": round(max(t), 5),
                                     "calls_per_window": iters[name]}
            spread = lambda *names: sum(row[x + "_ms"]["max"] - row[x + "_ms"]["min"] for x in names)  # noqa: E731
            row["c_over_a"] = round(row["c_ms"]["median"] / row["a_ms"]["median"], 3)
            row["c_over_b"] = round(row["c_ms"]["median"] / row["b_ms"]["median"], 3)
            row["c_not_slower_than_b"] = bool(row["c_ms"]["median"] <= row["b_ms"]["median"] + spread("b", "c"))
            if parent:
                row["a_over_a_parent"] = round(row["a_ms"]["median"] / row["a_parent_ms"]["median"], 3)
                row["a_not_slower_than_parent"] = bool(row["a_ms"]["median"] <= row["a_parent_ms"]["median"] + spread("a", "a_parent"))
            shapes.append(row)
            del ei, eo, flat, rej
    result = {"tool": "facet_search_bench", "device": torch.cuda.get_device_name(0), "rows": n, "dim": DIM, "k": K,
              "storage": STORAGE, "rounds": args.rounds, "parent_lib": bool(parent), "shapes": shapes,
              "bars_hold": all(r["c_not_slower_than_b"] and r.get("a_not_slower_than_parent", True) for r in shapes)}
    line = json.dumps(result)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
    print(line)
    if parent:
        parent.close()
    ix.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
