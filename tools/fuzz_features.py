#!/usr/bin/env python3
"""Seeded parity sweep over combined request features and index edits (tests/feature_cases.py): every case builds its
DeviceIndex (and IvfIndex), applies its edit script through the public methods, runs its request through search /
search_boosted / search_capped / search_diverse / IvfIndex.search and compares indices and scores bit for bit with the
composed reference (tests/feature_reference.py) on the edited model; MMR: selection order and relevance bits.
A mismatch prints one line with the case's parameters and the --case index that reproduces it, and the sweep goes on;
an exception from the library ends it at once with a non-zero status.
usage: python tools/fuzz_features.py [n_cases] [seed] [--kind K] [--case I]"""
import argparse
import collections
import os
import sys
import time
import traceback
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from instacart_next_order_recommendation_amd.search import IvfIndex, facet_masks, removal_moves, rowset_bits
from tests import feature_cases, feature_reference
from tests.index_model import Model


def apply_script(ix, case):
    """The case's edit script on the index, through the public methods -> False if remove_rows returned other moves
    than removal_moves states (the model was edited by those)."""
    ok, n = True, case.n0
    for op in case.script:
        if op[0] == "write_rows":
            ix.write_rows(op[1], op[2])
        elif op[0] == "write_facets":
            ix.write_facets(op[1], op[2])
        elif op[0] == "write_rowset":
            ix.write_rowset(op[1], rowset_bits(op[2][None, :], n)[0])
        elif op[0] == "reserve":
            ix.reserve(op[1])
        elif op[0] == "append_rows":
            ix.append_rows(op[1], op[2])
            n += op[1].shape[0]
        else:
            new_n, dst, src = removal_moves(n, op[1])
            got = ix.remove_rows(op[1])
            ok &= np.array_equal(got[0], dst) and np.array_equal(got[1], src)
            n = new_n
    return ok and ix.n_rows == n == case.model.n


def boosted(ix, c, masks, sets):
    """search_boosted; where a list carries a weight search.boost_csr refuses (NaN, negative), search_boosted's own two
    steps with the CSR laid out here, so that the weight reaches the kernel."""
    only = c.kind == "boosted-only"
    w_all = np.concatenate([w for _, w in c.boosts]) if c.boosts else np.zeros(0, np.float32)
    if not (np.isnan(w_all) | (w_all < 0)).any():
        return ix.search_boosted(c.q, c.k, [dict(zip(r.tolist(), w.tolist())) for r, w in c.boosts], c.excl, masks, only, sets)
    from instacart_next_order_recommendation_amd.search import exclusion_csr

    Q = c.q.shape[0]
    q = ix._queries(c.q)
    idx, sc = (None, None) if only else ix.search(q, c.k, c.excl, masks, sets)
    off = np.zeros(Q + 1, np.int32)
    off[1:] = np.cumsum([r.size for r, _ in c.boosts])
    rows = np.concatenate([r for r, _ in c.boosts] + [np.zeros(1, np.int64)]).astype(np.int32)
    w = np.concatenate([w for _, w in c.boosts] + [np.zeros(1, np.float32)]).astype(np.float32)
    max_len = max(max(r.size for r, _ in c.boosts), 1 if only else 0)
    ei, eo = exclusion_csr(c.excl, Q, ix.device)
    out_idx = torch.empty((Q, c.k), dtype=torch.int64, device=ix.device)
    out_sc = torch.empty((Q, c.k), dtype=torch.float32, device=ix.device)
    dev = lambda a: torch.from_numpy(a).to(ix.device)  # noqa: E731
    ix.boost_select_into(q, idx, sc, dev(off), dev(rows), dev(w), max_len, c.k, ei, eo, masks, out_idx, out_sc)
    return out_idx, out_sc


def run_case(c):
    """-> (got idx, got score) numpy, scripts_ok."""
    model0 = Model.of(None, c.E0, c.F0, c.M0)
    ix = model0.build(c.storage, row_offset=c.row_offset)
    ivf = None
    # no try / finally: after an exception from the library nothing more touches the device (main ends the process)
    if c.kind == "ivf":
        ivf = IvfIndex(ix, c.C)
    moves_ok = apply_script(ix, c)
    Q = c.q.shape[0]
    masks = None if c.allow is None else facet_masks(c.allow, Q, 2, ix.device)
    sets = None if c.set_ids is None else torch.from_numpy(np.ascontiguousarray(c.set_ids, np.int32)).to(ix.device)
    if c.kind == "ivf":
        if c.script:
            ivf.rebuild()
        out = ivf.search(c.q, c.k, c.nprobe, c.excl)
    elif c.kind in ("boosted", "boosted-only"):
        out = boosted(ix, c, masks, sets)
    elif c.kind in ("capped", "capped+boosted"):
        boosts = None if c.boosts is None else [dict(zip(r.tolist(), w.tolist())) for r, w in c.boosts]
        out = ix.search_capped(c.q, c.k, c.caps, c.candidates, c.excl, masks, sets, boosts)
    elif c.kind == "diverse":
        out = ix.search_diverse(c.q, c.top_k, c.lam, c.k, c.excl, masks, sets)
    else:
        out = ix.search(c.q, c.k, c.excl, masks, sets)
    torch.cuda.synchronize()
    got = out[0].cpu().numpy(), out[1].cpu().numpy(), moves_ok
    if ivf is not None:
        ivf.close()
    ix.close()
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("n_cases", nargs="?", type=int, default=200)
    ap.add_argument("seed", nargs="?", type=int, default=0)
    ap.add_argument("--kind", choices=feature_cases.KINDS)
    ap.add_argument("--case", type=int, help="run this one case of the seed")
    a = ap.parse_args()
    from tests.search_harness import n_cu

    cus = n_cu()
    t0 = time.time()
    ran = bad = 0
    hits = collections.Counter()
    todo = [feature_cases.make_case(a.seed, a.case)] if a.case is not None else feature_cases.cases(a.seed, a.n_cases, a.kind)
    for c in todo:
        want = feature_reference.expected(c)
        try:
            got_idx, got_sc, moves_ok = run_case(c)
        except BaseException:  # a HIP error included: the run ends here, and no destructor frees on the device either
            traceback.print_exc()
            print(f"EXCEPTION in {c.describe()}", flush=True)
            sys.stderr.flush()
            os._exit(2)
        ran += 1
        hits.update(feature_cases.cells_of(c, cus))
        same = moves_ok and np.array_equal(got_idx, want[0]) and \
            np.array_equal(got_sc.view(np.uint32), np.ascontiguousarray(want[1], np.float32).view(np.uint32))
        if not same:
            bad += 1
            if got_idx.shape == want[0].shape and got_sc.shape == want[1].shape:
                what = (f"idx_bad={int((got_idx != want[0]).sum())} "
                        f"score_bad={int((got_sc.view(np.uint32) != want[1].view(np.uint32)).sum())}")
            else:
                what = f"shape {got_idx.shape} for {want[0].shape}"
            print(f"MISMATCH {c.describe()} moves_ok={moves_ok} {what}", flush=True)
    print(f"{ran} cases, {bad} mismatches, {time.time() - t0:.1f} s")
    print(f"cells hit at {cus} CUs:")
    for cell, count in sorted(hits.items(), key=lambda kv: tuple(map(str, kv[0]))):
        print(f"  {' | '.join(map(str, cell))}: {count}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
