"""Shared inputs of the CF tests: the committed upstream fixture and seeded synthetic basket sets."""
from __future__ import annotations

import json
import random
from pathlib import Path

FIXTURE = Path(__file__).resolve().parent / "golden" / "cf_small"


def load_fixture() -> dict:
    return json.loads((FIXTURE / "upstream.json").read_text())


def fixture_as_items(rec: dict):
    """(baskets, histories, n_candidates, item_of, query ids) of the fixture in item numbers: corpus rows first."""
    item_of = {p: j for j, p in enumerate(rec["corpus_ids"])}
    for b in rec["baskets"].values():
        for p in b:
            item_of.setdefault(p, len(item_of))
    baskets = [[item_of[p] for p in b] for b in rec["baskets"].values()]
    qids = list(rec["rankings"].keys())
    histories = [[item_of[p] for p in rec["histories"][q]] for q in qids]
    return baskets, histories, len(rec["corpus_ids"]), item_of, qids


def synthetic_baskets(n_orders: int, n_items: int, seed: int, lengths=(0, 1, 2, 5, 9, 70, 300)) -> list[list[int]]:
    """Baskets whose lengths cycle through `lengths` (capped by what n_items allows), items skewed towards low numbers,
    roughly every fourth basket with an item repeated."""
    rng = random.Random(seed)
    out = []
    for o in range(n_orders):
        n = min(lengths[o % len(lengths)], n_items)
        basket = rng.sample(range(n_items), n) if n * 3 > n_items else list({min(int(rng.expovariate(6.0 / n_items)), n_items - 1)
                                                                            for _ in range(n)})
        if basket and o % 4 == 1:
            basket.insert(rng.randrange(len(basket) + 1), basket[0])
            basket.append(basket[-1])
        out.append(basket)
    return out


def synthetic_histories(n_queries: int, n_items: int, seed: int) -> list[list[int]]:
    rng = random.Random(seed)
    out = []
    for q in range(n_queries):
        n = min((0, 1, 3, 12, 40)[q % 5], n_items)
        out.append(sorted(rng.sample(range(n_items), n)))
    return out


class DeviceCF:
    """icrec_cf_* on item numbers: the thinnest possible wrapper, for the GPU tests."""

    def __init__(self, baskets, n_items: int, n_candidates: int, device="cuda:0"):
        import ctypes as C

        import numpy as np
        import torch

        from instacart_next_order_recommendation_amd import _native

        self.n, self.torch, self.np = _native, torch, np
        self.device = torch.device(device)
        if isinstance(baskets, tuple):      # (off int64, items int32) ready made
            off, items = baskets
        else:
            off = np.zeros(len(baskets) + 1, np.int64)
            np.cumsum([len(b) for b in baskets], out=off[1:])
            items = np.asarray([p for b in baskets for p in b], np.int32)
        self.n_candidates = n_candidates
        self.h = C.c_void_p()
        _native.check(_native.lib().icrec_cf_create(off.ctypes.data_as(C.c_void_p), items.ctypes.data_as(C.c_void_p), len(off) - 1,
                                                    n_items, n_candidates, 0, C.byref(self.h)), "icrec_cf_create")

    def close(self):
        if self.h:
            self.n.lib().icrec_cf_destroy(self.h)
            self.h = None

    def hist(self, histories):
        np, torch = self.np, self.torch
        off = np.zeros(len(histories) + 1, np.int32)
        np.cumsum([len(h) for h in histories], out=off[1:])
        flat = np.asarray([p for h in histories for p in h], np.int32)
        return torch.from_numpy(off).to(self.device), torch.from_numpy(flat).to(self.device)

    def rank_into(self, off, items, Q, k, rows, scores, ws):
        n = self.n
        n.check(n.lib().icrec_cf_rank(self.h, n.ptr(off), n.ptr(items), Q, k, n.ptr(rows), n.ptr(scores), n.ptr(ws), ws.numel(),
                                      n.stream_ptr(self.device)), "icrec_cf_rank")

    def rank_buffers(self, Q, k):
        torch = self.torch
        need = int(self.n.lib().icrec_cf_rank_workspace_bytes(self.h, Q, k))
        assert need > 0
        return (torch.empty((Q, k), dtype=torch.int64, device=self.device), torch.empty((Q, k), dtype=torch.int32, device=self.device),
                torch.empty(need, dtype=torch.uint8, device=self.device))

    def rank(self, histories, k):
        off, items = self.hist(histories)
        rows, scores, ws = self.rank_buffers(len(histories), k)
        self.rank_into(off, items, len(histories), k, rows, scores, ws)
        return rows.cpu().tolist(), scores.cpu().tolist()

    def rank_all(self, histories):
        n, torch = self.n, self.torch
        off, items = self.hist(histories)
        Q = len(histories)
        need = int(n.lib().icrec_cf_rank_all_workspace_bytes(self.h, Q))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        rows = torch.empty((Q, self.n_candidates), dtype=torch.int64, device=self.device)
        n.check(n.lib().icrec_cf_rank_all(self.h, n.ptr(off), n.ptr(items), Q, n.ptr(rows), n.ptr(ws), ws.numel(),
                                          n.stream_ptr(self.device)), "icrec_cf_rank_all")
        return rows.cpu().tolist()
