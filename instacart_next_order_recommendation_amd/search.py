"""Host side of the device index: cos_sim + top-k over a catalog resident in HBM.

Mirrors what the reference does with `self.product_embeddings` in
Recommender.recommend (src/inference/serve_recommendations.py:213-225): the
catalog matrix is uploaded once, L2-normalised once (the reference re-normalises
it inside cos_sim on every call), and every query batch is scored and ranked on
the GPU by libicrec's fused fp32-MFMA score+select kernel.

torch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from . import _native
from ._native import ptr, stream_ptr


def exclusion_csr(exclude: Optional[Sequence[Iterable[int]]], n_queries: int, device: Optional[torch.device] = None,
                  excl_cap: Optional[int] = None, of: str = "queries"):
    """Per-query iterables of row numbers -> (idx int32[nnz], off int32[Q+1]), sorted and unique per query, on
    `device` (numpy arrays without one); (None, None) when nothing is excluded.  With `excl_cap` (the sharded
    exchange's fixed id capacity) idx is zero-padded to excl_cap entries and always returned.  `of` names the
    queries in the count mismatch error."""
    if exclude is None:
        return None, None
    if len(exclude) != n_queries:
        raise ValueError(f"exclude has {len(exclude)} entries for {n_queries} {of}")
    off = np.zeros(n_queries + 1, np.int32)
    flat: list[int] = []
    for i, e in enumerate(exclude):
        flat.extend(sorted(set(int(v) for v in e)))
        off[i + 1] = len(flat)
    if excl_cap is None:
        if not flat:
            return None, None
        idx = np.asarray(flat, np.int32)
    else:
        if len(flat) > excl_cap:
            raise ValueError(f"{len(flat)} excluded rows on this rank exceed excl_cap={excl_cap} "
                             "(the same constant on every rank)")
        idx = np.zeros(excl_cap, np.int32)
        idx[:len(flat)] = flat
    if device is None:
        return idx, off
    return torch.from_numpy(idx).to(device), torch.from_numpy(off).to(device)


def facet_masks(allow, n_queries: int, n_facets: int, device=None):
    """Per-query facet constraints -> the allow masks icrec_search_faceted takes, uint32 [n_queries, n_facets, 8] (a
    torch tensor on `device`, a numpy array without one).  allow[i] is None (query i is unconstrained) or a sequence
    of n_facets entries, each None (that facet is unconstrained: all ones) or an iterable of the admitted values
    0..255 ([] admits nothing).  Bit v & 31 of word v >> 5 admits value v."""
    if len(allow) != n_queries:
        raise ValueError(f"allow has {len(allow)} entries for {n_queries} queries")
    W = _native.ICREC_FACET_MASK_WORDS
    m = np.zeros((n_queries, n_facets, W), np.uint32)
    for i, per_query in enumerate(allow):
        if per_query is None:
            m[i] = 0xFFFFFFFF
            continue
        if len(per_query) != n_facets:
            raise ValueError(f"allow[{i}] has {len(per_query)} entries for {n_facets} facets")
        for f, values in enumerate(per_query):
            if values is None:
                m[i, f] = 0xFFFFFFFF
                continue
            for v in values:
                v = int(v)
                if not 0 <= v <= 255:
                    raise ValueError(f"facet value {v} of allow[{i}][{f}] is outside 0..255")
                m[i, f, v >> 5] |= np.uint32(1 << (v & 31))
    if device is None:
        return m
    return torch.from_numpy(m.view(np.int32)).to(device).view(torch.uint32)


def rowset_bits(members, n_rows: int) -> np.ndarray:
    """Row sets -> the bitmaps icrec_index_set_rowsets takes, uint32 [S, ceil(n_rows / 32)]: bit r & 31 of word r >> 5 of
    set s says that row r is in s.  `members` is a sequence of S iterables of rows 0..n_rows-1, or a bool array
    [S, n_rows]."""
    n_rows = int(n_rows)
    if n_rows < 1:
        raise ValueError(f"n_rows must be >= 1, got {n_rows}")
    W = (n_rows + 31) // 32
    if isinstance(members, np.ndarray) and members.dtype == np.bool_:
        if members.ndim != 2 or members.shape[1] != n_rows:
            raise ValueError(f"a bool membership array must be [S, {n_rows}], got {members.shape}")
        padded = np.zeros((members.shape[0], W * 32), np.uint8)
        padded[:, :n_rows] = members
        return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32)
    bits = np.zeros((len(members), W), np.uint32)
    for s, rows in enumerate(members):
        r = np.unique(np.fromiter((int(v) for v in rows), np.int64))
        if r.size and (r[0] < 0 or r[-1] >= n_rows):
            raise ValueError(f"set {s} names row {int(r[0] if r[0] < 0 else r[-1])}, outside 0..{n_rows - 1}")
        np.bitwise_or.at(bits[s], r >> 5, np.uint32(1) << (r & 31).astype(np.uint32))
    return bits


def rowset_ids(within, n_queries: int, sets_per_query: Optional[int] = None, device=None):
    """Per-query set ids -> the slots icrec_search_in_sets takes, int32 [n_queries, m] filled with -1 (a free slot; a
    torch tensor on `device`, a numpy array without one).  within[i] is None (query i is unconstrained), an int, or up
    to ICREC_MAX_SETS_PER_QUERY ints; m = sets_per_query, or the longest entry (at least 1) without one."""
    if len(within) != n_queries:
        raise ValueError(f"within has {len(within)} entries for {n_queries} queries")
    lists = []
    for i, w in enumerate(within):
        ids = [] if w is None else [int(w)] if isinstance(w, (int, np.integer)) else [int(v) for v in w]
        if len(ids) > _native.ICREC_MAX_SETS_PER_QUERY:
            raise ValueError(f"within[{i}] names {len(ids)} sets, more than ICREC_MAX_SETS_PER_QUERY = "
                             f"{_native.ICREC_MAX_SETS_PER_QUERY}")
        lists.append(ids)
    longest = max((len(ids) for ids in lists), default=0)
    m = max(longest, 1) if sets_per_query is None else int(sets_per_query)
    if not 1 <= m <= _native.ICREC_MAX_SETS_PER_QUERY:
        raise ValueError(f"sets_per_query must be in [1, {_native.ICREC_MAX_SETS_PER_QUERY}], got {m}")
    if longest > m:
        raise ValueError(f"an entry of within names {longest} sets for sets_per_query = {m}")
    out = np.full((n_queries, m), -1, np.int32)
    for i, ids in enumerate(lists):
        out[i, :len(ids)] = ids
    if device is None:
        return out
    return torch.from_numpy(out).to(device)


def boost_csr(boosts, n_queries: int, device: Optional[torch.device] = None):
    """Per-query boost lists -> (off int32[Q+1], rows int32, w float32, max_len): the CSR icrec_boost_select takes, each
    query's rows ascending, on `device` (numpy arrays without one); max_len is the longest list.  boosts[i] is None (no
    list), a mapping row -> weight, or an iterable of rows (weight 0: the rows are ranked, not lifted).  rows and w
    hold at least one entry, so that they are never a NULL pointer.  ValueError: a count mismatch, more than
    ICREC_MAX_BOOSTS rows in one list, a weight that is NaN or negative."""
    if len(boosts) != n_queries:
        raise ValueError(f"boosts has {len(boosts)} entries for {n_queries} queries")
    off = np.zeros(n_queries + 1, np.int32)
    rows: list[int] = []
    w: list[float] = []
    max_len = 0
    for i, b in enumerate(boosts):
        if b is None:
            pairs = {}
        elif hasattr(b, "items"):
            pairs = {int(r): float(v) for r, v in b.items()}
        else:
            pairs = {int(r): 0.0 for r in b}
        if len(pairs) > _native.ICREC_MAX_BOOSTS:
            raise ValueError(f"boosts[{i}] lists {len(pairs)} rows, more than ICREC_MAX_BOOSTS = {_native.ICREC_MAX_BOOSTS}")
        for r in sorted(pairs):
            if not pairs[r] >= 0.0:  # (a NaN fails the comparison)
                raise ValueError(f"boosts[{i}]: the weight of row {r} is {pairs[r]!r}; weights must be >= 0")
            rows.append(r)
            w.append(pairs[r])
        off[i + 1] = len(rows)
        max_len = max(max_len, len(pairs))
    rows_a = np.asarray(rows or [0], np.int32)
    w_a = np.asarray(w or [0.0], np.float32)
    if device is None:
        return off, rows_a, w_a, max_len
    return torch.from_numpy(off).to(device), torch.from_numpy(rows_a).to(device), torch.from_numpy(w_a).to(device), max_len


def term_csr(terms, n_queries: int, device: Optional[torch.device] = None):
    """Per-query term lists -> (off int32[Q+1], rows int32, w float32): the CSR icrec_compose_queries takes, on `device`
    (numpy arrays without one).  terms[i] is None (no term), a mapping row -> weight, or a sequence of (row, weight)
    pairs, which may name a row twice.  ORDER-PRESERVING: a query's terms stay in the order given, because the order
    defines the sum (boost_csr sorts; this must not).  rows and w hold at least one entry, so that they are never a NULL
    pointer.  ValueError: a count mismatch, more than ICREC_MAX_TERMS terms in one list."""
    if len(terms) != n_queries:
        raise ValueError(f"terms has {len(terms)} entries for {n_queries} queries")
    off = np.zeros(n_queries + 1, np.int32)
    rows: list[int] = []
    w: list[float] = []
    for i, t in enumerate(terms):
        pairs = [] if t is None else list(t.items()) if hasattr(t, "items") else list(t)
        if len(pairs) > _native.ICREC_MAX_TERMS:
            raise ValueError(f"terms[{i}] lists {len(pairs)} terms, more than ICREC_MAX_TERMS = {_native.ICREC_MAX_TERMS}")
        for r, v in pairs:
            rows.append(int(r))
            w.append(float(v))
        off[i + 1] = len(rows)
    rows_a = np.asarray(rows or [0], np.int32)
    w_a = np.asarray(w or [0.0], np.float32)
    if device is None:
        return off, rows_a, w_a
    return torch.from_numpy(off).to(device), torch.from_numpy(rows_a).to(device), torch.from_numpy(w_a).to(device)


def cap_pairs(caps, n_queries: int, device=None):
    """Per-facet caps -> the table icrec_cap_select takes, int32 [n_queries, ICREC_MAX_FACETS] (a torch tensor on
    `device`, a numpy array without one).  caps is one sequence of ICREC_MAX_FACETS ints for all queries, or
    [n_queries, ICREC_MAX_FACETS] ints; an entry <= 0 (or None) leaves that facet uncapped."""
    F = _native.ICREC_MAX_FACETS
    c = np.asarray([[0 if v is None else v for v in row] for row in caps] if np.ndim(caps) == 2
                   else [0 if v is None else v for v in caps])
    if c.dtype.kind not in "iu" or c.shape not in ((F,), (n_queries, F)):
        raise ValueError(f"caps must be {F} ints or ints [{n_queries}, {F}], got {c.dtype} {c.shape}")
    c = np.clip(c.astype(np.int64), 0, 2**31 - 1).astype(np.int32)
    out = np.array(np.broadcast_to(c, (n_queries, F)), order="C")  # (a writable copy)
    if device is None:
        return out
    return torch.from_numpy(out).to(device)


def removal_moves(n_rows: int, row_ids):
    """The move plan of icrec_index_remove_rows, without a device: removing the rows `row_ids` (integers in [0, n_rows),
    any order, unique, fewer than n_rows) leaves new_n = n_rows - m rows; the holes (removed rows below new_n, ascending)
    are filled by the surviving rows at or past new_n, ascending -> (new_n, dst int32 [n_moves], src int32 [n_moves]):
    row src[i] becomes row dst[i], every other surviving row keeps its number.  ValueError for an id out of range, a
    duplicate, or a removal that would leave nothing."""
    n_rows = int(n_rows)
    ids = np.asarray(row_ids)
    if ids.size == 0:
        ids = ids.astype(np.int64)
    if ids.ndim != 1 or ids.dtype.kind not in "iu":
        raise ValueError(f"removal_moves: row_ids must be a list of integers, got {ids.dtype} {ids.shape}")
    ids = np.sort(ids.astype(np.int64))
    if ids.size and (ids[0] < 0 or ids[-1] >= n_rows):
        raise ValueError(f"removal_moves: row {int(ids[0] if ids[0] < 0 else ids[-1])} is outside 0..{n_rows - 1}")
    if (np.diff(ids) == 0).any():
        raise ValueError(f"removal_moves: row {int(ids[1:][np.diff(ids) == 0][0])} is named twice")
    if ids.size >= n_rows:
        raise ValueError(f"removal_moves: removing {ids.size} of {n_rows} rows would leave the index empty")
    new_n = n_rows - int(ids.size)
    dst = ids[ids < new_n]
    src = np.setdiff1d(np.arange(new_n, n_rows, dtype=np.int64), ids[ids >= new_n], assume_unique=True)
    return new_n, dst.astype(np.int32), src.astype(np.int32)


def apply_moves(array, new_n: int, dst, src, axis: int = 0):
    """A per-row host array after a removal: entries src moved onto entries dst along `axis`, cut to new_n (a copy)."""
    a = np.array(array, copy=True)
    sel = [slice(None)] * a.ndim
    sel_d, sel_s, cut = list(sel), list(sel), list(sel)
    sel_d[axis], sel_s[axis], cut[axis] = np.asarray(dst, np.int64), np.asarray(src, np.int64), slice(0, int(new_n))
    a[tuple(sel_d)] = a[tuple(sel_s)]
    return np.ascontiguousarray(a[tuple(cut)])


def _out_pair(Q: int, k: int, device):
    """The (idx int64 [Q, k], score float32 [Q, k]) pair a ranking call writes, uninitialised on `device`."""
    return (torch.empty((Q, k), dtype=torch.int64, device=device), torch.empty((Q, k), dtype=torch.float32, device=device))


def _candidates(idx: torch.Tensor, sc: torch.Tensor, device, score: str = "sc", Q=None):
    """A candidate pair as `search` returns it, checked - idx int64 [Q, k], its scores (named `score` in the error)
    float32 [Q, k], with Q rows when Q is given - and contiguous on `device`."""
    if idx.dim() != 2 or idx.dtype != torch.int64 or sc.dtype != torch.float32 or sc.shape != idx.shape \
            or (Q is not None and idx.shape[0] != Q):
        rows = "Q" if Q is None else Q
        raise ValueError(f"idx must be int64 [{rows}, k] and {score} float32 [{rows}, k], got {idx.dtype} {tuple(idx.shape)} "
                         f"and {sc.dtype} {tuple(sc.shape)}")
    return idx.to(device).contiguous(), sc.to(device).contiguous()


def _block(scratch, need: int, shape: str, *args):
    """The current stream's block of `scratch` (a StreamScratch) for a call that needs `need` bytes; 0 is how a
    *_workspace_bytes entry refuses a shape: IcrecError with shape.format(*args)."""
    if need == 0:
        raise _native.IcrecError("bad " + shape.format(*args))
    return scratch.block(need)


ROW_STORAGE = {"f32": 0, "bf16": 1, "f32+filter": 2, "bf16+filter": 3}  # ICREC_ROWS_* in include/icrec.h


class DeviceIndex:
    """A row shard of the product-embedding matrix, normalised and resident on one GPU.

    storage="bf16" keeps the normalised rows as bfloat16 (half the HBM; BASELINE config 5's 10M-row
    catalog); the arithmetic stays the exact fp32 fmaf chain over the widened values.
    storage="f32+filter" keeps fp32 rows plus their f16 hi/lo planes (2x the HBM): batches of >= 256 queries are
    ranked on the f16 matrix cores first and the candidates re-scored exactly — same bits out, several times
    faster on large catalogs (see ICREC_ROWS_F32_FILTER in include/icrec.h)."""

    def __init__(self, embeddings, device: str | torch.device = "cuda:0", row_offset: int = 0,
                 storage: str = "f32"):
        if storage not in ROW_STORAGE:
            raise ValueError(f"storage must be one of {sorted(ROW_STORAGE)}, got {storage!r}")
        self.storage = storage
        self.device = _native.hip_device(device, "DeviceIndex")
        self._ws_by_stream = _native.StreamScratch(self.device)
        self._mmr_ws_by_stream = _native.StreamScratch(self.device)  # its own blocks: growing one never moves a search's
        self._boost_ws_by_stream = _native.StreamScratch(self.device)  # likewise
        L = _native.lib()
        rows = torch.as_tensor(embeddings)
        if rows.dim() != 2:
            raise ValueError("embeddings must be [n_rows, dim]")
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        self.n_rows, self.dim = int(rows.shape[0]), int(rows.shape[1])
        self.row_offset = int(row_offset)
        h = C.c_void_p()
        torch.cuda.synchronize(self.device)
        _native.check(L.icrec_index_create_ex(ptr(rows), self.n_rows, self.dim, self.row_offset, self.device.index,
                                              ROW_STORAGE[storage], C.byref(h)), "icrec_index_create_ex")
        self._h = h

    def set_facets(self, values) -> None:
        """Give every row its facet values, uint8 [n_rows, n_facets] with n_facets 1 or 2 (for a catalog: aisle and
        department codes), or take them away with None.  A set-up call: never while a search on this index runs.
        Only searches that pass `allow` look at them."""
        L = _native.lib()
        if values is None:
            _native.check(L.icrec_index_set_facets(self._h, None, 0), "icrec_index_set_facets")
            return
        v = np.asarray(values)
        if v.dtype != np.uint8 or v.ndim != 2 or v.shape[0] != self.n_rows:
            raise ValueError(f"facets must be uint8 [{self.n_rows}, n_facets], got {v.dtype} {v.shape}")
        v = np.ascontiguousarray(v)
        _native.check(L.icrec_index_set_facets(self._h, v.ctypes.data_as(C.c_void_p), int(v.shape[1])),
                      "icrec_index_set_facets")

    @property
    def n_facets(self) -> int:
        """Facet values per row (0: none set)."""
        return int(_native.lib().icrec_index_facets(self._h))

    def set_rowsets(self, bits) -> None:
        """Give the index its row sets, uint32 [n_sets, ceil(n_rows / 32)] bitmaps over the local rows (rowset_bits
        builds them; for a catalog: one per store assortment, "in stock", "vegan"), or take them away with None.  A
        set-up call: never while a search on this index runs.  Only searches that pass `sets` look at them."""
        L = _native.lib()
        if bits is None:
            _native.check(L.icrec_index_set_rowsets(self._h, None, 0), "icrec_index_set_rowsets")
            return
        b = self._rowset_words(bits, 2)
        _native.check(L.icrec_index_set_rowsets(self._h, b.ctypes.data_as(C.c_void_p), int(b.shape[0])),
                      "icrec_index_set_rowsets")

    def write_rowset(self, set_id: int, bits) -> None:
        """Replace one set's bitmap, uint32 [ceil(n_rows / 32)] (an in-stock set that changes through the day).  A
        set-up call like set_rowsets; a captured graph replayed afterwards follows the new members."""
        b = self._rowset_words(bits, 1)
        _native.check(_native.lib().icrec_index_write_rowset(self._h, int(set_id), b.ctypes.data_as(C.c_void_p)),
                      "icrec_index_write_rowset")

    def _rowset_words(self, bits, ndim: int) -> np.ndarray:
        b = np.asarray(bits)
        W = (self.n_rows + 31) // 32
        if b.dtype != np.uint32 or b.ndim != ndim or b.shape[-1] != W:
            raise ValueError(f"row set bitmaps must be uint32 {'[n_sets, ' if ndim == 2 else '['}{W}], got {b.dtype} {b.shape}")
        return np.ascontiguousarray(b)

    @property
    def n_rowsets(self) -> int:
        """Row sets of the index (0: none set)."""
        return int(_native.lib().icrec_index_rowsets(self._h))

    def _sorted_rows(self, row_ids, m: int, what: str):
        """Host row ids -> (ids int32 ascending, the permutation that sorted them); ValueError for a count other than m,
        an id outside [0, n_rows) or a duplicate.  Needs no device."""
        ids = np.asarray(row_ids.cpu() if isinstance(row_ids, torch.Tensor) else row_ids)
        if ids.size == 0:
            ids = ids.astype(np.int64)
        if ids.ndim != 1 or ids.dtype.kind not in "iu" or ids.shape[0] != m:
            raise ValueError(f"{what}: row_ids must be {m} integers, got {ids.dtype} {ids.shape}")
        ids = ids.astype(np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= self.n_rows):
            bad = int(ids.min() if ids.min() < 0 else ids.max())
            raise ValueError(f"{what}: row {bad} is outside 0..{self.n_rows - 1}")
        order = np.argsort(ids, kind="stable")
        ids = ids[order]
        if (np.diff(ids) == 0).any():
            raise ValueError(f"{what}: row {int(ids[1:][np.diff(ids) == 0][0])} is named twice")
        return ids.astype(np.int32), order

    def write_rows(self, row_ids, embeddings) -> None:
        """Rewrite rows in place (icrec_index_write_rows): embeddings [m, dim] of any norm replace the LOCAL rows
        row_ids, after which the index - stored rows and filter copy - is bit for bit the one built from the edited
        matrix; no pointer of the handle changes, so captured graphs stay valid and search the new rows.  row_ids: m
        host integers in any order (range and duplicates are checked here, ValueError; ids and rows are sorted
        together), or a device int32 tensor [m], ascending and unique, which the kernel reads as it is (entries outside
        the index are skipped).  Asynchronous on the current stream; the caller keeps it from running beside a search
        of this index on another stream.  An IvfIndex over this index does not see the write: IvfIndex.rebuild."""
        rows = torch.as_tensor(embeddings)
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"embeddings must be [m, {self.dim}], got {tuple(rows.shape)}")
        m = int(rows.shape[0])
        if isinstance(row_ids, torch.Tensor) and row_ids.is_cuda:
            if row_ids.dtype != torch.int32 or tuple(row_ids.shape) != (m,):
                raise ValueError(f"device row_ids must be int32 [{m}], got {row_ids.dtype} {tuple(row_ids.shape)}")
            ids_dev = row_ids.to(self.device).contiguous()
        else:
            ids, order = self._sorted_rows(row_ids, m, "write_rows")
            if m == 0:
                return
            rows = rows[torch.from_numpy(order).to(rows.device)]
            ids_dev = torch.from_numpy(ids).to(self.device)
        if m == 0:
            return
        self.write_rows_into(ids_dev, rows.to(device=self.device, dtype=torch.float32).contiguous())

    def write_rows_into(self, ids_dev: torch.Tensor, rows_dev: torch.Tensor) -> None:
        """Allocation-free form of `write_rows` on caller-owned contiguous device buffers (hipGraph-capturable; there is
        no workspace): ids_dev int32 [m] ascending and unique, rows_dev float32 [m, dim].  The kernel reads both when
        it runs: a captured graph follows what the buffers hold at replay."""
        m = int(ids_dev.shape[0])
        if ids_dev.dtype != torch.int32 or ids_dev.dim() != 1 or not ids_dev.is_contiguous() or ids_dev.device != self.device:
            raise ValueError(f"ids_dev must be a contiguous int32 tensor [m] on {self.device}, got {ids_dev.dtype} "
                             f"{tuple(ids_dev.shape)} on {ids_dev.device}")
        if rows_dev.dtype != torch.float32 or tuple(rows_dev.shape) != (m, self.dim) or not rows_dev.is_contiguous() \
                or rows_dev.device != self.device:
            raise ValueError(f"rows_dev must be a contiguous float32 tensor [{m}, {self.dim}] on {self.device}, got "
                             f"{rows_dev.dtype} {tuple(rows_dev.shape)} on {rows_dev.device}")
        _native.check(_native.lib().icrec_index_write_rows(self._h, ptr(rows_dev), ptr(ids_dev), m, stream_ptr(self.device)),
                      "icrec_index_write_rows")

    def write_facets(self, row_ids, values) -> None:
        """Replace the facet values of the LOCAL rows row_ids (host integers, any order, no duplicates) with values,
        uint8 [m, n_facets] (icrec_index_write_facets).  A set-up call like write_rowset; a captured graph replayed
        afterwards follows the new values."""
        v = np.asarray(values)
        if v.dtype != np.uint8 or v.ndim != 2 or v.shape[1] != (self.n_facets or v.shape[1]):
            raise ValueError(f"facet values must be uint8 [m, {self.n_facets}], got {v.dtype} {v.shape}")
        ids, order = self._sorted_rows(row_ids, int(v.shape[0]), "write_facets")
        v = np.ascontiguousarray(v[order])
        _native.check(_native.lib().icrec_index_write_facets(self._h, ids.ctypes.data_as(C.c_void_p),
                                                             v.ctypes.data_as(C.c_void_p), int(ids.shape[0])),
                      "icrec_index_write_facets")

    @property
    def capacity(self) -> int:
        """Rows the index's device arrays are sized for (n_rows until `reserve`)."""
        return int(_native.lib().icrec_index_capacity(self._h))

    def reserve(self, capacity: int) -> None:
        """Size every device array of the index for `capacity` >= n_rows rows (icrec_index_reserve): allocates, copies
        device to device, frees the old arrays.  Nothing a search returns changes.  A set-up call: never while a search
        on this index runs; graphs captured over the index must be captured again, an IvfIndex rebuilt."""
        _native.check(_native.lib().icrec_index_reserve(self._h, int(capacity)), "icrec_index_reserve")

    def append_rows(self, embeddings, facets=None) -> range:
        """Append rows (icrec_index_append_rows): embeddings [m, dim] of any norm become rows n_rows .. n_rows + m - 1,
        stored as a fresh index stores them; facets uint8 [m, n_facets], required exactly when the index has facets.
        The new rows belong to no row set (write_rowset).  A full index reserves max(2 * capacity, n_rows + m) first.
        Returns the range of the new rows and updates n_rows.  A set-up call under `reserve`'s contract; asynchronous
        on the current stream."""
        rows = torch.as_tensor(embeddings)
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"embeddings must be [m, {self.dim}], got {tuple(rows.shape)}")
        m = int(rows.shape[0])
        nf = self.n_facets
        v = None
        if (facets is None) != (nf == 0):
            raise ValueError(f"append_rows: facets must be {'given' if nf else 'None'}: the index has {nf} facets")
        if facets is not None:
            v = np.ascontiguousarray(np.asarray(facets))
            if v.dtype != np.uint8 or v.shape != (m, nf):
                raise ValueError(f"facets must be uint8 [{m}, {nf}], got {v.dtype} {v.shape}")
        if m == 0:
            return range(self.n_rows, self.n_rows)
        cap = self.capacity
        if self.n_rows + m > cap:
            self.reserve(max(2 * cap, self.n_rows + m))
        rows = rows.to(device=self.device, dtype=torch.float32).contiguous()
        _native.check(_native.lib().icrec_index_append_rows(self._h, ptr(rows), m,
                                                            None if v is None else v.ctypes.data_as(C.c_void_p),
                                                            stream_ptr(self.device)), "icrec_index_append_rows")
        first = self.n_rows
        self.n_rows += m
        return range(first, self.n_rows)

    def remove_rows(self, row_ids):
        """Remove the LOCAL rows row_ids (host integers in any order; range and duplicates are checked here, ValueError)
        by swapping survivors from the tail into their places (icrec_index_remove_rows) -> (dst, src) int32 numpy
        arrays: row src[i] is now row dst[i], every other surviving row kept its number, and n_rows shrank by
        len(row_ids) - `removal_moves` states the plan.  The caller applies it to what it keeps per row.  A set-up
        call under `reserve`'s contract; asynchronous on the current stream."""
        ids = np.asarray(row_ids.cpu() if isinstance(row_ids, torch.Tensor) else row_ids)
        ids, _ = self._sorted_rows(ids, int(ids.shape[0]) if ids.ndim == 1 else -1, "remove_rows")
        m = int(ids.shape[0])
        if m >= self.n_rows:
            raise ValueError(f"remove_rows: removing {m} of {self.n_rows} rows would leave the index empty")
        dst, src = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32)
        n_moves = C.c_int32(0)
        ids = np.ascontiguousarray(ids)
        _native.check(_native.lib().icrec_index_remove_rows(self._h, ids.ctypes.data_as(C.c_void_p), m,
                                                            dst.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p),
                                                            C.byref(n_moves), stream_ptr(self.device)),
                      "icrec_index_remove_rows")
        self.n_rows -= m
        return dst[:n_moves.value].copy(), src[:n_moves.value].copy()

    def export_filter(self):
        """The filter copy of a "+filter" storage, (hi, lo) float16 [n_rows, dim] on the device: the values the filter
        pass multiplies, as stored (parity checks only)."""
        hi = torch.empty((self.n_rows, self.dim), dtype=torch.float16, device=self.device)
        lo = torch.empty_like(hi)
        _native.check(_native.lib().icrec_index_export_filter(self._h, ptr(hi), ptr(lo), stream_ptr(self.device)),
                      "icrec_index_export_filter")
        return hi, lo

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.lib().icrec_index_destroy(self._h)
            self._h = None
        self._ws_by_stream.clear()
        self._mmr_ws_by_stream.clear()
        self._boost_ws_by_stream.clear()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _workspace(self, n_queries: int, k: int) -> torch.Tensor:
        """This stream's scratch block, large enough for one search of this shape."""
        need = int(_native.lib().icrec_search_workspace_bytes(self._h, n_queries, k))
        return _block(self._ws_by_stream, need, "search shape: n_queries={}, k={}", n_queries, k)

    def _queries(self, q) -> torch.Tensor:
        q = torch.as_tensor(q)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [Q, {self.dim}], got {tuple(q.shape)}")
        return q.to(device=self.device, dtype=torch.float32).contiguous()

    def _check_allow(self, allow: torch.Tensor, Q: int) -> None:
        nf = self.n_facets  # 0: the library refuses the call (ICREC_EINVAL)
        if allow.dtype != torch.uint32 or allow.device != self.device or not allow.is_contiguous() \
                or tuple(allow.shape) != (Q, nf or allow.shape[1], _native.ICREC_FACET_MASK_WORDS):
            raise ValueError(f"allow must be a contiguous uint32 tensor [{Q}, {nf}, {_native.ICREC_FACET_MASK_WORDS}] "
                             f"on {self.device}, got {allow.dtype} {tuple(allow.shape)} on {allow.device}")

    def _check_sets(self, sets: torch.Tensor, Q: int) -> None:
        if sets.dtype != torch.int32 or sets.device != self.device or not sets.is_contiguous() or sets.dim() != 2 \
                or sets.shape[0] != Q or not 1 <= sets.shape[1] <= _native.ICREC_MAX_SETS_PER_QUERY:
            raise ValueError(f"sets must be a contiguous int32 tensor [{Q}, 1..{_native.ICREC_MAX_SETS_PER_QUERY}] on "
                             f"{self.device}, got {sets.dtype} {tuple(sets.shape)} on {sets.device}")

    # ------------------------------------------------------------------ API
    def search(self, q, k: int, exclude: Optional[Sequence[Iterable[int]]] = None, allow: Optional[torch.Tensor] = None,
               sets: Optional[torch.Tensor] = None):
        """Top-k rows per query: (idx int64[Q,k] with -1 pads, score float32[Q,k]).
        Order: score descending, lower row first on ties.  `exclude`: per-query local rows.  `allow`: the queries'
        facet masks, a device uint32 tensor [Q, n_facets, 8] (facet_masks builds it): only rows whose facet values
        the masks admit are returned - the same bits as excluding every other row.  `sets`: the queries' row set ids,
        a device int32 tensor [Q, 1..4] (rowset_ids builds it): only rows in every named set are returned - again the
        bits of excluding every other row; -1 is a free slot, an id the index does not have admits nothing."""
        q = self._queries(q)
        Q = int(q.shape[0])
        ei, eo = exclusion_csr(exclude, Q, self.device)
        idx, sc = _out_pair(Q, k, self.device)
        self.search_into(q, k, ei, eo, idx, sc, allow=allow, sets=sets)
        return idx, sc

    def search_into(self, q: torch.Tensor, k: int, excl_idx: Optional[torch.Tensor], excl_off: Optional[torch.Tensor],
                    out_idx: torch.Tensor, out_score: torch.Tensor, ws: Optional[torch.Tensor] = None,
                    allow: Optional[torch.Tensor] = None, sets: Optional[torch.Tensor] = None) -> None:
        """Allocation-free form of `search` on caller-owned device buffers (hipGraph-capturable once the
        workspace for this (Q, k) exists, or with `ws` of the caller's own): q float32 [Q, dim],
        out_idx int64 [Q, k], out_score float32 [Q, k].  The kernels read `allow`, `sets` and the index's row sets
        when they run: a captured graph follows what the buffers hold at replay."""
        Q = int(q.shape[0])
        if ws is None:
            ws = self._workspace(Q, k)
        if sets is not None:
            self._check_sets(sets, Q)
            if allow is not None:
                self._check_allow(allow, Q)
            _native.check(_native.lib().icrec_search_in_sets(self._h, ptr(q), Q, k, ptr(excl_idx), ptr(excl_off), ptr(allow),
                                                             ptr(sets), int(sets.shape[1]), ptr(out_idx), ptr(out_score),
                                                             ptr(ws), ws.numel(), stream_ptr(self.device)),
                          "icrec_search_in_sets")
            return
        if allow is not None:
            self._check_allow(allow, Q)
            _native.check(_native.lib().icrec_search_faceted(self._h, ptr(q), Q, k, ptr(excl_idx), ptr(excl_off), ptr(allow),
                                                             ptr(out_idx), ptr(out_score), ptr(ws), ws.numel(),
                                                             stream_ptr(self.device)), "icrec_search_faceted")
            return
        _native.check(_native.lib().icrec_search(self._h, ptr(q), Q, k, ptr(excl_idx), ptr(excl_off), ptr(out_idx),
                                                 ptr(out_score), ptr(ws), ws.numel(), stream_ptr(self.device)),
                      "icrec_search")

    def mmr_select(self, idx: torch.Tensor, rel: torch.Tensor, top_k: int, lam: float):
        """Diversity re-selection of a search result (Maximal Marginal Relevance, icrec_mmr_select): idx int64 [Q, k]
        candidate rows as `search` returns them (-1 pads; rows outside this shard are skipped) and rel float32 [Q, k]
        their relevance (the search scores, or any other: it need not be sorted), both device tensors
        -> (idx int64 [Q, top_k], rel float32 [Q, top_k]) on the device, in SELECTION order: the most relevant
        candidate first, then at each step the candidate that maximises lam * rel - (1 - lam) * (its greatest
        similarity to a row already picked).  lam = 1 keeps the relevance order, lam = 0 only avoids similarity."""
        idx, rel = _candidates(idx, rel, self.device, "rel")
        out_idx, out_rel = _out_pair(int(idx.shape[0]), top_k, self.device)
        self.mmr_select_into(idx, rel, top_k, lam, out_idx, out_rel)
        return out_idx, out_rel

    def mmr_select_into(self, idx: torch.Tensor, rel: torch.Tensor, top_k: int, lam: float, out_idx: torch.Tensor,
                        out_rel: torch.Tensor, ws: Optional[torch.Tensor] = None) -> None:
        """Allocation-free form of `mmr_select` on caller-owned contiguous device buffers (hipGraph-capturable once the
        workspace for this (Q, k) exists, or with `ws` of the caller's own).  The outputs must not alias the inputs."""
        Q, k = int(idx.shape[0]), int(idx.shape[1])
        if ws is None:
            need = int(_native.lib().icrec_mmr_select_workspace_bytes(self._h, Q, k))
            ws = _block(self._mmr_ws_by_stream, need, "mmr_select shape: n_queries={}, k={}", Q, k)
        _native.mmr_select(self._h, idx, rel, top_k, lam, out_idx, out_rel, ws, self.device)

    def search_diverse(self, q, top_k: int, lam: float, candidates: int,
                       exclude: Optional[Sequence[Iterable[int]]] = None, allow: Optional[torch.Tensor] = None,
                       sets: Optional[torch.Tensor] = None):
        """`search(q, candidates, exclude, allow, sets)` followed by `mmr_select(.., top_k, lam)` on its result, without
        a host step in between: the top_k most relevant-yet-diverse of each query's `candidates` best rows, with their
        cosine scores, in selection order (not score-descending)."""
        idx, sc = self.search(q, candidates, exclude, allow, sets)
        return self.mmr_select(idx, sc, top_k, lam)

    def boost_select(self, q, idx: Optional[torch.Tensor], sc: Optional[torch.Tensor], boosts, top_k: int,
                     exclude: Optional[Sequence[Iterable[int]]] = None, allow: Optional[torch.Tensor] = None):
        """Boost each query's listed rows on a search result (icrec_boost_select): q the queries that were searched,
        idx int64 [Q, k] and sc float32 [Q, k] the result of `search(q, k, exclude, allow)` as device tensors (both
        None: no candidates, only the listed rows are ranked), boosts the per-query lists boost_csr takes (local rows)
        -> (idx int64 [Q, top_k], score float32 [Q, top_k]) on the device: the top_k of the WHOLE shard under
        cosine + weight for the listed rows and plain cosine for the others, score descending, -1 / 0 pads.  `exclude`
        and `allow` must be the search's own: a listed row that is excluded or not admitted is never returned."""
        q = self._queries(q)
        Q = int(q.shape[0])
        if (idx is None) != (sc is None):
            raise ValueError("idx and sc must both be given or both be None")
        if idx is not None:
            idx, sc = _candidates(idx, sc, self.device, Q=Q)
        off, rows, w, max_len = boost_csr(boosts, Q, self.device)
        ei, eo = exclusion_csr(exclude, Q, self.device)
        out_idx, out_sc = _out_pair(Q, top_k, self.device)
        self.boost_select_into(q, idx, sc, off, rows, w, max_len if idx is not None else max(max_len, 1), top_k, ei, eo,
                               allow, out_idx, out_sc)
        return out_idx, out_sc

    def boost_select_into(self, q: torch.Tensor, idx: Optional[torch.Tensor], sc: Optional[torch.Tensor],
                          boost_off: torch.Tensor, boost_rows: torch.Tensor, boost_w: Optional[torch.Tensor],
                          max_boosts: int, top_k: int, excl_idx: Optional[torch.Tensor], excl_off: Optional[torch.Tensor],
                          allow: Optional[torch.Tensor], out_idx: torch.Tensor, out_score: torch.Tensor,
                          ws: Optional[torch.Tensor] = None) -> None:
        """Allocation-free form of `boost_select` on caller-owned contiguous device buffers (hipGraph-capturable once the
        workspace for this (Q, max_boosts) exists, or with `ws` of the caller's own): the lists as boost_csr lays them
        out, of which the first max_boosts entries per query are read.  The kernels read the lists, weights and masks
        when they run: a captured graph follows what the buffers hold at replay.  The outputs must not alias the
        inputs."""
        Q = int(q.shape[0])
        if allow is not None:
            self._check_allow(allow, Q)
        if ws is None:
            need = int(_native.lib().icrec_boost_select_workspace_bytes(self._h, Q, max_boosts))
            ws = _block(self._boost_ws_by_stream, need, "boost_select shape: n_queries={}, max_boosts={}", Q, max_boosts)
        _native.boost_select(self._h, q, idx, sc, boost_off, boost_rows, boost_w, max_boosts, excl_idx, excl_off, allow,
                             top_k, out_idx, out_score, ws, self.device)

    def search_boosted(self, q, k: int, boosts, exclude: Optional[Sequence[Iterable[int]]] = None,
                       allow: Optional[torch.Tensor] = None, only: bool = False, sets: Optional[torch.Tensor] = None):
        """`search(q, k, exclude, allow, sets)` followed by `boost_select(.., boosts, k, exclude, allow)` on its result,
        without a host step in between: the k best rows of the shard under cosine + weight.  only=True ranks each
        query's listed rows alone ("buy it again": the history, best first) and runs no search.  `sets` restricts the
        search's candidates only: icrec_boost_select does not look at row sets, so the caller lists no row outside
        the query's sets (the recommender drops them on the host); the result is then the top k of the admissible
        rows under cosine + weight."""
        q = self._queries(q)
        idx, sc = (None, None) if only else self.search(q, k, exclude, allow, sets)
        return self.boost_select(q, idx, sc, boosts, k, exclude, allow)

    def ranked(self, q, k: int, exclude=None, allow=None, sets=None, boosts=None, only: bool = False):
        """The source ranking of a request, k wide: `search`, or with boosts (per-query lists, not None) `search_boosted`."""
        if boosts is None:
            return self.search(q, k, exclude, allow, sets)
        return self.search_boosted(q, k, boosts, exclude, allow, only, sets)

    def compose_queries(self, base, terms, base_weight=None) -> torch.Tensor:
        """Queries composed from the index's stored rows (icrec_compose_queries): out[i] = a[i] * normalised base[i] +
        the sum of weight * stored row over terms[i], in the order given -> float32 [Q, dim] on the device, NOT
        normalised (the searches normalise their queries).  base: the text vectors [Q, dim] (or one, [dim]), or None
        (no text part; Q is then len(terms)); terms: the per-query lists term_csr takes (LOCAL rows, weights of either
        sign), or None with a base; base_weight: None (every a = 1), one number for all queries, or Q numbers.  One
        term of weight 1 without a base is the stored row ("similar items"); positive and negative terms on a base are
        Rocchio feedback; terms alone are a basket's profile."""
        if base is None and terms is None:
            raise ValueError("compose_queries needs a base, terms, or both")
        if base is not None:
            base = self._queries(base)
        Q = int(base.shape[0]) if base is not None else len(terms)
        if Q < 1:
            raise ValueError("compose_queries needs at least one query")
        off, rows, w = term_csr(terms if terms is not None else [None] * Q, Q)
        max_terms = int(np.diff(off).max())
        off, rows, w = (torch.from_numpy(a).to(self.device) for a in (off, rows, w))
        if base is None:
            if base_weight is not None:
                raise ValueError("base_weight needs a base")
            max_terms = max(max_terms, 1)  # (a query without a known term is then the zero vector)
        base_w = None
        if base_weight is not None:
            base_w = torch.as_tensor(base_weight, dtype=torch.float32).reshape(-1)
            if base_w.numel() not in (1, Q):
                raise ValueError(f"base_weight must be one number or {Q} numbers, got {base_w.numel()}")
            base_w = base_w.expand(Q).to(self.device).contiguous()
        out = torch.empty((Q, self.dim), dtype=torch.float32, device=self.device)
        self.compose_queries_into(base, base_w, off, rows, w, max_terms, out)
        return out

    def compose_queries_into(self, base: Optional[torch.Tensor], base_w: Optional[torch.Tensor], off: torch.Tensor,
                             rows: torch.Tensor, w: Optional[torch.Tensor], max_terms: int, out: torch.Tensor) -> None:
        """Allocation-free form of `compose_queries` on caller-owned contiguous device buffers (hipGraph-capturable;
        there is no workspace): base float32 [Q, dim] or None, base_w float32 [Q] or None, the terms as term_csr lays
        them out (w None: every weight is 1), of which the first max_terms entries per query are read, out float32
        [Q, dim].  The kernel reads the lists and weights when it runs: a captured graph follows what the buffers hold
        at replay.  out must not alias base."""
        Q = int(out.shape[0])
        for name, t, dtype, shape in (("base", base, torch.float32, (Q, self.dim)), ("base_w", base_w, torch.float32, (Q,)),
                                      ("off", off, torch.int32, (Q + 1,)), ("rows", rows, torch.int32, None),
                                      ("w", w, torch.float32, None), ("out", out, torch.float32, (Q, self.dim))):
            if t is None:
                continue
            if t.dtype != dtype or t.device != self.device or not t.is_contiguous() or t.dim() != (len(shape) if shape else 1) \
                    or (shape is not None and tuple(t.shape) != shape):
                raise ValueError(f"{name} must be a contiguous {dtype} tensor {list(shape) if shape else '[nnz]'} on "
                                 f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if w is not None and w.shape[0] != rows.shape[0]:
            raise ValueError(f"rows and w must have one entry per term, got {rows.shape[0]} and {w.shape[0]}")
        _native.compose_queries(self._h, base, base_w, Q, off, rows, w, max_terms, out, self.device)

    def cap_select(self, idx: torch.Tensor, sc: torch.Tensor, caps, top_k: int, allow: Optional[torch.Tensor] = None):
        """Caps per facet value on a search result (icrec_cap_select): idx int64 [Q, k] candidate rows as `search`
        returns them (-1 pads; rows outside this shard are skipped) and sc float32 [Q, k] their scores, both device
        tensors, caps as cap_pairs takes them (or its device tensor), allow the masks the candidates were searched with (or None)
        -> (idx int64 [Q, top_k], score float32 [Q, top_k], state int32 [Q, 2], allow_next uint32 [Q, n_facets, 8]) on
        the device: each query's candidates in their order, without those whose aisle (facet 0) or department (facet 1)
        already has its cap of rows before them; state[q] = (picks, done), done = 0 where fewer than top_k rows were
        kept and the list held no pad - a wider or a further search may then find more (search_capped runs those
        rounds); allow_next = allow without the values that are full."""
        idx, sc = _candidates(idx, sc, self.device)
        Q = int(idx.shape[0])
        out_idx, out_sc = _out_pair(Q, top_k, self.device)
        state = torch.empty((Q, 2), dtype=torch.int32, device=self.device)
        allow_next = torch.empty((Q, max(self.n_facets, 1), _native.ICREC_FACET_MASK_WORDS), dtype=torch.int32,
                                 device=self.device).view(torch.uint32)
        caps = caps if isinstance(caps, torch.Tensor) else cap_pairs(caps, Q, self.device)
        self.cap_select_into(idx, sc, caps, top_k, out_idx, out_sc, state, allow=allow, allow_next=allow_next)
        return out_idx, out_sc, state, allow_next

    def cap_select_into(self, idx: torch.Tensor, sc: torch.Tensor, caps: torch.Tensor, top_k: int, out_idx: torch.Tensor,
                        out_score: torch.Tensor, out_state: torch.Tensor, n_prior: Optional[torch.Tensor] = None,
                        allow: Optional[torch.Tensor] = None, allow_next: Optional[torch.Tensor] = None) -> None:
        """Allocation-free form of `cap_select` on caller-owned contiguous device buffers (hipGraph-capturable; there is
        no workspace): caps int32 [Q, 2], out_state int32 [Q, 2].  With n_prior int32 [Q] the first n_prior[q] entries
        of a query's out rows are picks of an earlier round: they stay, count towards the caps, and the walk appends
        behind them.  allow_next may be `allow` itself.  The kernel reads caps, n_prior and allow when it runs."""
        Q = int(idx.shape[0])
        if caps.dtype != torch.int32 or tuple(caps.shape) != (Q, _native.ICREC_MAX_FACETS) or not caps.is_contiguous():
            raise ValueError(f"caps must be a contiguous int32 tensor [{Q}, {_native.ICREC_MAX_FACETS}], got {caps.dtype} "
                             f"{tuple(caps.shape)}")
        if n_prior is not None and (n_prior.dtype != torch.int32 or tuple(n_prior.shape) != (Q,) or not n_prior.is_contiguous()):
            raise ValueError(f"n_prior must be a contiguous int32 tensor [{Q}], got {n_prior.dtype} {tuple(n_prior.shape)}")
        for m in (allow, allow_next):
            if m is not None:
                self._check_allow(m, Q)
        _native.cap_select(self._h, idx, sc, caps, n_prior, allow, top_k, out_idx, out_score, out_state, allow_next,
                           self.device)

    #: rounds the last search_capped needed (1: every query was done after the first search)
    last_cap_rounds = 0

    def search_capped(self, q, top_k: int, caps, candidates: Optional[int] = None,
                      exclude: Optional[Sequence[Iterable[int]]] = None, allow: Optional[torch.Tensor] = None,
                      sets: Optional[torch.Tensor] = None, boosts=None, only: bool = False):
        """The top_k rows per query under caps per facet value, exactly: the greedy walk of the query's complete ranking
        of the admissible rows that keeps a row only while its aisle (facet 0) and department (facet 1) have fewer
        than caps rows before it -> (idx int64 [Q, top_k] with -1 pads, score float32 [Q, top_k]), in the search's
        order.  caps as cap_pairs takes them; exclude, allow and sets as `search` takes them; boosts (and only) as
        search_boosted takes them - the ranking is then the boosted one.
        Round 1 searches `candidates` wide (default min(128, 4 * top_k), clipped to the shard, never below top_k) for
        all queries and walks the lists on the device (cap_select).  A query whose list ran out before top_k rows
        were kept goes into a further round: searched again without its picks and without the aisles and departments
        that are full, walked again with the picks as priors - until no query is left (include/icrec.h has the proof
        that this is the walk of the whole ranking).  Between rounds the host reads the states and the picks of the
        unfinished queries and merges the picks into their exclusion lists.  last_cap_rounds: the rounds it took."""
        q = self._queries(q)
        Q = int(q.shape[0])
        top_k = int(top_k)
        if not 1 <= top_k <= _native.ICREC_MAX_K:
            raise ValueError(f"top_k must be in [1, {_native.ICREC_MAX_K}], got {top_k}")
        k = min(_native.ICREC_MAX_K, 4 * top_k) if candidates is None else int(candidates)
        if not 1 <= k <= _native.ICREC_MAX_K:
            raise ValueError(f"candidates must be in [1, {_native.ICREC_MAX_K}], got {candidates!r}")
        k = max(min(k, self.n_rows), min(top_k, self.n_rows))
        caps = cap_pairs(caps, Q, self.device)
        if exclude is not None and len(exclude) != Q:
            raise ValueError(f"exclude has {len(exclude)} entries for {Q} queries")
        if boosts is not None and len(boosts) != Q:
            raise ValueError(f"boosts has {len(boosts)} entries for {Q} queries")
        out_idx, out_sc, state, allow_next = self.cap_select(*self.ranked(q, k, exclude, allow, sets, boosts, only), caps, top_k,
                                                             allow)
        self.last_cap_rounds = 1
        words = allow_next.view(torch.int32)  # (torch indexes int32, not uint32)
        while True:
            left = torch.nonzero(state[:, 1] == 0)[:, 0]  # (the comparison's result read by nonzero synchronises)
            if left.numel() == 0:
                return out_idx, out_sc
            if self.last_cap_rounds > _native.ICREC_MAX_FACETS * 256 + 1:
                raise _native.IcrecError("search_capped: more rounds than facet values")  # (the proof's bound)
            self.last_cap_rounds += 1
            sub = left.tolist()
            o_idx, o_sc = out_idx[left], out_sc[left]
            picks = o_idx.cpu().numpy() - self.row_offset
            n_prior = state[left, 0].contiguous()
            excl = [sorted(set(int(v) for v in (exclude[i] if exclude is not None else ())) | set(row[row >= 0].tolist()))
                    for i, row in zip(sub, picks)]
            masks = words[left].contiguous().view(torch.uint32)
            st = torch.empty((len(sub), 2), dtype=torch.int32, device=self.device)
            c_idx, c_sc = self.ranked(q[left], k, excl, masks, None if sets is None else sets[left].contiguous(),
                                      None if boosts is None else [boosts[i] for i in sub], only)
            self.cap_select_into(c_idx, c_sc, caps[left].contiguous(), top_k, o_idx, o_sc, st, n_prior, masks, masks)
            out_idx[left], out_sc[left], state[left], words[left] = o_idx, o_sc, st, masks.view(torch.int32)

    def search_partial(self, q, k: int, exclude: Optional[Sequence[Iterable[int]]] = None) -> torch.Tensor:
        """Shard-local sorted lists as packed keys, int64-viewed uint64 [Q,k] (see icrec_search_partial)."""
        q = self._queries(q)
        Q = int(q.shape[0])
        ei, eo = exclusion_csr(exclude, Q, self.device)
        keys = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        ws = self._workspace(Q, k)
        _native.check(_native.lib().icrec_search_partial(self._h, ptr(q), Q, k, ptr(ei), ptr(eo), ptr(keys),
                                                         ptr(ws), ws.numel(), stream_ptr(self.device)),
                      "icrec_search_partial")
        return keys

    def scores(self, q) -> torch.Tensor:
        """Full cosine score matrix [Q, n_rows] (parity checks only; never on the serving path)."""
        q = self._queries(q)
        Q = int(q.shape[0])
        out = torch.empty((Q, self.n_rows), dtype=torch.float32, device=self.device)
        ws = self._workspace(Q, 1)
        _native.check(_native.lib().icrec_scores(self._h, ptr(q), Q, ptr(out), ptr(ws), ws.numel(),
                                                 stream_ptr(self.device)), "icrec_scores")
        return out

    def rank_all(self, q) -> torch.Tensor:
        """The complete ranking of the shard for each query: int64 [Q, n_rows] global rows, best first
        (score descending, lower row first on ties) — `scores.argsort(descending=True)` of the reference's
        evaluation consumers.  Workspace grows with Q * n_rows: call it in passes of a few hundred queries."""
        q = self._queries(q)
        Q = int(q.shape[0])
        L = _native.lib()
        need = int(L.icrec_rank_all_workspace_bytes(self._h, Q))
        if need == 0:
            raise _native.IcrecError(f"bad rank_all shape: n_queries={Q}")
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty((Q, self.n_rows), dtype=torch.int64, device=self.device)
        _native.check(L.icrec_rank_all(self._h, ptr(q), Q, ptr(out), ptr(ws), ws.numel(), stream_ptr(self.device)),
                      "icrec_rank_all")
        return out

    def export(self) -> torch.Tensor:
        """The normalised rows the index holds, [n_rows, dim] fp32 on the device."""
        out = torch.empty((self.n_rows, self.dim), dtype=torch.float32, device=self.device)
        _native.check(_native.lib().icrec_index_export(self._h, ptr(out), stream_ptr(self.device)),
                      "icrec_index_export")
        return out


class IvfIndex:
    """An inverted-file index beside a DeviceIndex (icrec_ivf, include/icrec.h): the rows split into
    n_lists = len(centroids) lists, each row in the list whose centroid the library's own search names for it; a
    search scans only each query's `probes` best lists.  The result is the exact top-k of the probed lists, in
    DeviceIndex.search's bits; with probes == n_lists it is DeviceIndex.search's.  Holds a second copy of the rows (in
    list order); `index` must outlive it.  Creation is a set-up call: never while a call on `index` runs."""

    def __init__(self, index: DeviceIndex, centroids):
        self.index = index
        self.device = index.device
        self._ws_by_stream = _native.StreamScratch(self.device)
        c = torch.as_tensor(centroids)
        if c.dim() != 2 or c.shape[1] != index.dim:
            raise ValueError(f"centroids must be [n_lists, {index.dim}], got {tuple(c.shape)}")
        self.centroids = c.to(device=self.device, dtype=torch.float32).contiguous().clone()  # kept for rebuild()
        self._h = None
        self._create()

    def _create(self) -> None:
        h = C.c_void_p()
        torch.cuda.synchronize(self.device)
        _native.check(_native.lib().icrec_ivf_create(self.index._h, ptr(self.centroids), int(self.centroids.shape[0]),
                                                     C.byref(h)), "icrec_ivf_create")
        self._h = h
        self.n_rows = self.index.n_rows  # the rows of this copy: the index may gain or lose rows until rebuild()

    def rebuild(self) -> None:
        """Destroy the IVF and create it again over the same index with the same centroids: the copy of the rows and
        their assignment as they are after DeviceIndex.write_rows, append_rows or remove_rows, which an IVF does not see
        (after reserve its base's arrays have moved as well).  A set-up call like the
        constructor; a graph captured over the old handle must be captured again."""
        if getattr(self, "_h", None):
            _native.lib().icrec_ivf_destroy(self._h)
            self._h = None
        self._create()

    @property
    def n_lists(self) -> int:
        return int(_native.lib().icrec_ivf_lists(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.lib().icrec_ivf_destroy(self._h)
            self._h = None
        self._ws_by_stream.clear()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def layout(self):
        """(perm int32 [n_rows], list_off int64 [n_lists + 1]) device tensors: the local rows sorted by (list, row) and
        the list boundaries in that order."""
        perm = torch.empty(self.n_rows, dtype=torch.int32, device=self.device)
        off = torch.empty(self.n_lists + 1, dtype=torch.int64, device=self.device)
        _native.check(_native.lib().icrec_ivf_layout(self._h, ptr(perm), ptr(off), stream_ptr(self.device)),
                      "icrec_ivf_layout")
        return perm, off

    def _workspace(self, n_queries: int, k: int, probes: int) -> torch.Tensor:
        """This stream's scratch block, large enough for one search of this shape."""
        need = int(_native.lib().icrec_ivf_search_workspace_bytes(self._h, n_queries, k, probes))
        return _block(self._ws_by_stream, need, "IVF search shape: n_queries={}, k={}, probes={} of {} lists",
                      n_queries, k, probes, self.centroids.shape[0])

    def search(self, q, k: int, probes: int, exclude: Optional[Sequence[Iterable[int]]] = None):
        """The k best rows of each query's `probes` best lists: (idx int64[Q,k] with -1 pads, score float32[Q,k]),
        ordered as DeviceIndex.search orders.  `exclude`: per-query local (original) rows."""
        q = self.index._queries(q)
        Q = int(q.shape[0])
        ei, eo = exclusion_csr(exclude, Q, self.device)
        idx, sc = _out_pair(Q, k, self.device)
        self.search_into(q, k, probes, ei, eo, idx, sc)
        return idx, sc

    def search_into(self, q: torch.Tensor, k: int, probes: int, excl_idx: Optional[torch.Tensor],
                    excl_off: Optional[torch.Tensor], out_idx: torch.Tensor, out_score: torch.Tensor,
                    ws: Optional[torch.Tensor] = None) -> None:
        """Allocation-free form of `search` on caller-owned device buffers (hipGraph-capturable once the workspace for
        this (Q, k, probes) exists, or with `ws` of the caller's own): q float32 [Q, dim], out_idx int64 [Q, k],
        out_score float32 [Q, k]."""
        Q = int(q.shape[0])
        if ws is None:
            ws = self._workspace(Q, k, probes)
        _native.check(_native.lib().icrec_ivf_search(self._h, ptr(q), Q, k, probes, ptr(excl_idx), ptr(excl_off),
                                                     ptr(out_idx), ptr(out_score), ptr(ws), ws.numel(),
                                                     stream_ptr(self.device)), "icrec_ivf_search")


def train_centroids(index: DeviceIndex, n_lists: int, iters: int = 10, sample: int = 64, seed: int = 0) -> torch.Tensor:
    """Centroids for an IvfIndex over `index`, float32 [n_lists, dim] on its device: spherical k-means on at most
    sample * n_lists of the stored rows, chosen by a seeded permutation, whose first n_lists rows are the initial
    centroids.  Each iteration assigns the sample with the library (a temporary DeviceIndex of the centroids, searched
    at k = 1 in chunks of rows) and replaces every centroid by the normalised mean of its members; a list without
    members keeps its centroid.  The sums are taken in float64 over the members in sample order (sorted by list, then
    segment sums): no atomics, so one seed gives the same bits every time on one machine.  torch does the plumbing;
    this is not the hot path."""
    if not 1 <= n_lists <= index.n_rows:
        raise ValueError(f"n_lists must be in [1, {index.n_rows}], got {n_lists}")
    dev = index.device
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    m = min(index.n_rows, int(sample) * n_lists)
    rows = torch.randperm(index.n_rows, generator=gen)[:m].to(dev)
    X = index.export()[rows]  # (the export is a transient fp32 copy of the whole shard, freed on return from here)
    cent = X[:n_lists].clone()
    chunk = 1 << 16
    for _ in range(int(iters)):
        tmp = DeviceIndex(cent, device=dev)
        try:
            assign = torch.cat([tmp.search(X[lo:lo + chunk], 1)[0][:, 0] for lo in range(0, m, chunk)])
        finally:
            tmp.close()
        order = torch.argsort(assign, stable=True)
        counts = torch.bincount(assign, minlength=n_lists)
        csum = torch.cumsum(X[order].to(torch.float64), dim=0)  # a sequential scan per column: order-fixed
        end = torch.cumsum(counts, 0)
        zero = torch.zeros((1, index.dim), dtype=torch.float64, device=dev)
        upto = torch.cat([zero, csum])[end]
        sums = upto - torch.cat([zero, upto[:-1]])
        mean = torch.nn.functional.normalize(sums, p=2, dim=1, eps=1e-12).to(torch.float32)
        cent = torch.where((counts > 0)[:, None], mean, cent)
    return cent.contiguous()


def rrf_weights(depth: int, c: float = 60.0, weight: float = 1.0) -> np.ndarray:
    """The position table of reciprocal rank fusion, float32 [depth]: t[j] = float32(weight / (c + j + 1)), computed
    in float64 and rounded once.  ValueError: depth outside [1, ICREC_MAX_K], c not finite or <= -1 (a position's
    denominator must be positive), weight not a number >= 0."""
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 1 <= int(depth) <= _native.ICREC_MAX_K:
        raise ValueError(f"depth must be an integer in [1, {_native.ICREC_MAX_K}], got {depth!r}")
    def number(v):
        try:
            return float(v)
        except (TypeError, ValueError):
            return float("nan")

    c64, w64 = number(c), number(weight)
    if not (np.isfinite(c64) and c64 > -1.0):
        raise ValueError(f"c must be finite and > -1, got {c!r}")
    if not 0.0 <= w64:  # (a NaN fails the comparison)
        raise ValueError(f"weight must be a number >= 0, got {weight!r}")
    with np.errstate(over="ignore"):
        return (np.float64(w64) / (np.float64(c64) + np.arange(1, int(depth) + 1, dtype=np.float64))).astype(np.float32)


def _fuse_list(idx: torch.Tensor, gate, w, name: str, device, Q=None):
    """One list of fuse_select, checked: idx int64 [Q, k], gate None or int32 [Q, k], w float32 [k] (a tensor, or
    anything numpy converts) -> the three, contiguous on `device`."""
    if idx.dim() != 2 or idx.dtype != torch.int64 or not 1 <= idx.shape[1] <= _native.ICREC_MAX_K \
            or (Q is not None and idx.shape[0] != Q):
        raise ValueError(f"{name}_idx must be int64 [{'Q' if Q is None else Q}, 1..{_native.ICREC_MAX_K}], got {idx.dtype} "
                         f"{tuple(idx.shape)}")
    if gate is not None and (gate.dtype != torch.int32 or gate.shape != idx.shape):
        raise ValueError(f"{name}_gate must be int32 {tuple(idx.shape)}, got {gate.dtype} {tuple(gate.shape)}")
    if not isinstance(w, torch.Tensor):
        w = torch.from_numpy(np.ascontiguousarray(w, np.float32))
    if w.dtype != torch.float32 or tuple(w.shape) != (idx.shape[1],):
        raise ValueError(f"{name}_w must be float32 [{idx.shape[1]}], got {w.dtype} {tuple(w.shape)}")
    return idx.to(device).contiguous(), None if gate is None else gate.to(device).contiguous(), w.to(device).contiguous()


def fuse_select(a_idx: torch.Tensor, b_idx: torch.Tensor, a_w, b_w, top_k: int, n_ids: int,
                a_gate: Optional[torch.Tensor] = None, b_gate: Optional[torch.Tensor] = None,
                exclude: Optional[Sequence[Iterable[int]]] = None, positions: bool = False):
    """Weighted rank fusion of two ranked id lists (icrec_fuse_select): a_idx int64 [Q, ka] and b_idx int64 [Q, kb]
    device tensors as `DeviceIndex.search` and icrec_cf_rank return them (best first, negative = pad), a_w [ka] and
    b_w [kb] the weight of each position (rrf_weights builds them), gates int32 like the lists (an entry counts where
    its gate is > 0; icrec_cf_rank's scores) or None, exclude per-query ids as `search` takes them
    -> (idx int64 [Q, top_k] with -1 pads, fused score float32 [Q, top_k]) on a_idx's device, ordered by
    e_a(position in A) + e_b(position in B) descending, lower id first on ties; with positions=True also
    pos int32 [Q, top_k, 2], each result's positions in A and B (-1: not in that list)."""
    device = _native.hip_device(a_idx.device, "fuse_select")
    a_idx, a_gate, a_w = _fuse_list(a_idx, a_gate, a_w, "a", device)
    Q = int(a_idx.shape[0])
    b_idx, b_gate, b_w = _fuse_list(b_idx, b_gate, b_w, "b", device, Q)
    ei, eo = exclusion_csr(exclude, Q, device)
    out_idx, out_sc = _out_pair(Q, top_k, device)
    pos = torch.empty((Q, top_k, 2), dtype=torch.int32, device=device) if positions else None
    fuse_select_into(a_idx, b_idx, a_w, b_w, top_k, n_ids, out_idx, out_sc, a_gate, b_gate, ei, eo, pos)
    return (out_idx, out_sc, pos) if positions else (out_idx, out_sc)


def fuse_select_into(a_idx: torch.Tensor, b_idx: torch.Tensor, a_w: torch.Tensor, b_w: torch.Tensor, top_k: int, n_ids: int,
                     out_idx: torch.Tensor, out_score: torch.Tensor, a_gate: Optional[torch.Tensor] = None,
                     b_gate: Optional[torch.Tensor] = None, excl_idx: Optional[torch.Tensor] = None,
                     excl_off: Optional[torch.Tensor] = None, out_pos: Optional[torch.Tensor] = None) -> None:
    """Allocation-free form of `fuse_select` on caller-owned contiguous device buffers (hipGraph-capturable; there is
    no workspace): the lists, gates and tables as `fuse_select` describes them, the exclusions as the device CSR
    exclusion_csr builds, out_idx int64 [Q, top_k], out_score float32 [Q, top_k], out_pos int32 [Q, top_k, 2] or None.
    The kernel reads gates, tables and exclusions when it runs."""
    Q = int(a_idx.shape[0])
    for name, t, dtype, shape in (("a_idx", a_idx, torch.int64, (Q, a_idx.shape[1])), ("b_idx", b_idx, torch.int64, (Q, b_idx.shape[1])),
                                  ("a_gate", a_gate, torch.int32, tuple(a_idx.shape)), ("b_gate", b_gate, torch.int32, tuple(b_idx.shape)),
                                  ("a_w", a_w, torch.float32, (a_idx.shape[1],)), ("b_w", b_w, torch.float32, (b_idx.shape[1],)),
                                  ("out_idx", out_idx, torch.int64, (Q, top_k)), ("out_score", out_score, torch.float32, (Q, top_k)),
                                  ("out_pos", out_pos, torch.int32, (Q, top_k, 2))):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
                              or t.device != a_idx.device):
            raise ValueError(f"{name} must be a contiguous {dtype} tensor {tuple(shape)} on {a_idx.device}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    _native.fuse_select(a_idx, a_gate, a_w, b_idx, b_gate, b_w, n_ids, excl_idx, excl_off, top_k, out_idx, out_score, out_pos,
                        a_idx.device)


def merge_topk(keys: torch.Tensor, k: int):
    """Merge sorted partial key lists [n_lists, Q, k] (int64-viewed uint64) into (idx, score) [Q,k]."""
    if keys.dim() != 3 or keys.shape[2] != k:
        raise ValueError("keys must be [n_lists, Q, k]")
    keys = keys.contiguous()
    n_lists, Q = int(keys.shape[0]), int(keys.shape[1])
    idx, sc = _out_pair(Q, k, keys.device)
    _native.check(_native.lib().icrec_merge_topk(ptr(keys), n_lists, Q, k, ptr(idx), ptr(sc), keys.device.index,
                                                 stream_ptr(keys.device)), "icrec_merge_topk")
    return idx, sc


def normalize_rows(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """x / max(|x|_2, eps) row-wise on the device (torch.nn.functional.normalize as cos_sim uses it)."""
    x = x.to(dtype=torch.float32).contiguous()
    out = torch.empty_like(x)
    _native.check(_native.lib().icrec_normalize_rows(ptr(x), ptr(out), x.shape[0], x.shape[1], eps,
                                                     x.device.index, stream_ptr(x.device)), "icrec_normalize_rows")
    return out
