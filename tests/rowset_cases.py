"""Shared by the row set tests (test_rowsets, test_rowset_search_gpu, test_rowset_tiles_gpu,
test_rowset_recommender_gpu): the sets every search test uses, the slots dealt to neighbouring queries, include/icrec.h's
definition of an admissible row restated in numpy, and the one check of a set-restricted search: the result is that of
the plain search with every inadmissible row excluded, bit for bit, against the CPU oracle AND against ix.search with
those lists on the device.  Importing this needs no GPU."""
from __future__ import annotations

import functools

import numpy as np

from instacart_next_order_recommendation_amd.search import facet_masks, rowset_bits, rowset_ids
from tests.search_harness import DeviceIndex, admitted_matrix, assert_search, oracle, resident_lds

N = 2085            # 8 tiles of 256 + 37 rows, 16 tiles of 128 + 37 rows
# the sets of standard_sets, by id
FULL, EMPTY, ONE, EDGE, LAST37, FIVE, SEVEN, TWELVE, ONEPCT, HALF, OVA, OVB = range(12)
N_SETS = 12
INT32_MAX = 2**31 - 1


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def standard_sets(n=N, seed=11):
    """bool [N_SETS, n], read-only: full; empty; one row; the rows at the word and tile edges {0, 31, 32, 255, 256,
    n - 1}; only the rows of the ragged last 256-row tile (37 of them at n = N); 5 rows; 7 rows of the last tile; those
    12 together; about 1 % of the rows; about 50 %; two sets of 30 rows that overlap in exactly 3."""
    rng = np.random.default_rng(seed)
    assert n >= 600 and n % 256
    m = np.zeros((N_SETS, n), bool)
    m[FULL] = True
    m[ONE, int(rng.integers(256, n - 256))] = True
    m[EDGE, [0, 31, 32, 255, 256, n - 1]] = True
    last = (n // 256) * 256
    m[LAST37, last:] = True
    m[FIVE, rng.choice(last - 64, 5, replace=False)] = True
    m[SEVEN, last + rng.choice(n - last, 7, replace=False)] = True
    m[TWELVE] = m[FIVE] | m[SEVEN]
    m[ONEPCT] = rng.random(n) < 0.01
    m[HALF] = rng.random(n) < 0.5
    rows = rng.permutation(n)[:57]
    m[OVA, rows[:30]] = True
    m[OVB, rows[27:]] = True
    assert (m[OVA] & m[OVB]).sum() == 3 and m[TWELVE].sum() == 12 and m[EMPTY].sum() == 0
    return _frozen(m)


# One kind of slots per query, dealt in turn: 17 kinds, so every tile of 32 queries mixes all of them.
KINDS = [
    [-1, HALF],                    # one set (behind a free slot)
    [HALF, ONEPCT],                # two
    [HALF, FULL, OVA],             # three
    [OVA, OVB, FULL, HALF],        # four: 3 rows at most
    [HALF, HALF],                  # a duplicate id counts once
    [-1, -1, -1, -1],              # unconstrained
    [N_SETS - 1],                  # the last id
    [N_SETS],                      # one past it: admits nothing
    [INT32_MAX, HALF],             # never used as an index
    [-5, EDGE],                    # a negative id other than -1 is a free slot
    [OVA, OVB],                    # the intersection of 3 rows
    [EMPTY],
    [ONE],
    [LAST37],
    [FIVE],
    [EDGE, -1, FULL],
    [FULL],
]


def mixed_ids(nq, start=0):
    """int32 [nq, 4]: query i gets KINDS[(start + i) % 17], padded with -1."""
    return rowset_ids([KINDS[(start + i) % len(KINDS)] for i in range(nq)], nq, 4)


def admitted_by_sets(member, ids, n_sets=None):
    """include/icrec.h's slots: a slot with id < 0 constrains nothing, one with id in [0, n_sets) requires the row's
    bit in that set, one with id >= n_sets admits no row.  member: bool [S, n], ids: int [Q, m] -> bool [Q, n]."""
    member, ids = np.asarray(member, bool), np.asarray(ids, np.int64)
    n_sets = member.shape[0] if n_sets is None else n_sets
    ok = np.ones((ids.shape[0], member.shape[1]), bool)
    for i in range(ids.shape[0]):
        for s in ids[i]:
            if s >= n_sets:
                ok[i] = False
            elif s >= 0:
                ok[i] &= member[s]
    return ok


def admitted(member, ids, F=None, allow=None):
    """The rows every slot admits and, with facet values F and per-query constraints `allow` (search.facet_masks'
    input), the masks admit too: bool [Q, n]."""
    ok = admitted_by_sets(member, ids)
    if allow is not None:
        ok &= admitted_matrix(F, facet_masks(allow, ids.shape[0], F.shape[1]))
    return ok


def resident_lds_sets(kp):
    """Dynamic LDS of the set-restricted resident filter pass at list length kp (TopK<CfgRes, true, true, true>::bytes
    in csrc/search.hip): the faceted pass's, plus 64 queries' slots of 16 B and 2 x 8 x 64 set words of 4 B."""
    return resident_lds(kp, True) + 64 * 16 + 2 * 8 * 64 * 4


def index_with_sets(P, member, storage="f32", F=None, **kw):
    ix = DeviceIndex(P, storage=storage, **kw)
    assert ix.n_rowsets == 0
    ix.set_rowsets(rowset_bits(np.asarray(member), P.shape[0]))
    assert ix.n_rowsets == member.shape[0]
    if F is not None:
        ix.set_facets(F)
    return ix


def check_in_sets(ix, q, P, k, member, ids, excl=None, F=None, allow=None):
    """ix.search(q, k, excl, allow=masks, sets=ids) == oracle over excl united with the inadmissible rows == ix.search
    with those lists on the device.  ids: int32 [Q, m] numpy.  Returns the expected pair."""
    import torch

    nq = q.shape[0]
    ok = admitted(member, ids, F, allow)
    union = [(rej if excl is None else np.union1d(rej, np.asarray(excl[i], np.int64))).tolist()
             for i, rej in enumerate(np.flatnonzero(~row) for row in ok)]
    want = oracle.search(q, P, k, union, row_offset=ix.row_offset, storage="bf16" if ix.storage.startswith("bf16") else "f32")
    dev_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(ix.device)
    dev_masks = None if allow is None else facet_masks(allow, nq, F.shape[1], ix.device)
    assert_search(ix.search(q, k, excl, allow=dev_masks, sets=dev_ids), want)
    assert_search(ix.search(q, k, union), want)
    idx = want[0]
    assert ((idx == -1) | ((idx >= ix.row_offset) & (idx < ix.row_offset + ix.n_rows))).all()
    n_real = np.minimum(k, np.asarray([ix.n_rows - len(u) for u in union]))
    assert ((idx >= 0).sum(axis=1) == n_real).all()
    return want
