// stream.h — what the one-thread-per-row streaming kernels share: search.hip's stream_search_kernel (the whole
// catalog, up to 8 queries) and ivf.hip's ivf_scan_kernel (one probed list of one query): the tile geometry, the
// native 16-byte vector their slabs travel in, and the fold of an LDS queue of candidate keys into a sorted list.
#pragma once

#include "common.h"

namespace icrec {

// A block streams tiles of 256 rows through LDS in 128-byte slabs, one row per thread.
constexpr int ST_ROWS = 256, ST_LDB = 144;  // LDS row stride 144 B: conflict-free 16-B reads at one row per lane

typedef float v4f __attribute__((ext_vector_type(4)));

#ifdef __HIPCC__

// Merge the queue of query q into its sorted list; one wavefront, all 64 lanes call this.
// Every element's new position is its rank in the union (keys are unique): a list entry keeps its
// index plus the number of better candidates; candidate i gets (#better candidates) + (#better list
// entries), the latter from a ballot over the lanes holding the list — no search, no extra LDS trips.
__device__ __forceinline__ void merge_queue(u64* list, const u64* queue, int n, int k, int lane) {
    const u64 c = lane < n ? queue[lane] : 0ull;
    const u64 e0 = lane < k ? list[lane] : 0ull;
    const u64 e1 = lane + 64 < k ? list[lane + 64] : 0ull;
    int rc = 0, r0 = 0, r1 = 0, lc = 0;
    for (int i = 0; i < n; ++i) {
        const u64 ci = queue[i];  // LDS broadcast
        rc += ci > c;
        r0 += ci > e0;
        r1 += ci > e1;
        const int better = __popcll(__ballot(e0 > ci)) + (k > 64 ? __popcll(__ballot(e1 > ci)) : 0);
        lc = lane == i ? better : lc;
    }
    const int pc = rc + lc, p0 = lane + r0, p1 = lane + 64 + r1;
    // all reads above are complete (their values are consumed) before any lane writes
    if (lane < n && pc < k) list[pc] = c;
    if (lane < k && p0 < k) list[p0] = e0;
    if (lane + 64 < k && p1 < k) list[p1] = e1;
}

#endif  // __HIPCC__

}  // namespace icrec
