// cf.hip — item-item co-occurrence collaborative filtering (the reference's ItemItemCFBaseline.rank_all,
// src/baselines/collaborative_filtering.py:140-163) without a co-occurrence table.
//
// B is the 0/1 order x item incidence matrix (baskets de-duplicated), H_q the item set of query q's history:
//     score(q, p) = sum_{h in H_q} cooc(p, h) = sum_{o : p in basket_o} w_q[o],   w_q[o] = |basket_o ∩ H_q|
// Pass A (basket-major) computes w for a TILE of T queries at once: the tile's history membership sits in LDS as T
// bits per item, a thread walks one basket and counts per bit.  Pass B (product-major) sums w over a product's
// column; w is stored [tile][order][T] so one column entry serves the whole tile with one contiguous read.  Scores
// are int32 and exact in any summation order; they become keys ((score + 1) << 32) | ~row, the total order of
// make_key's keys with 0 as the pad / "left out" value, and are sorted by sort.hip's sorters (common.h); the CSR
// offsets of the index are sort.hip's prefix sums.
#include <stdlib.h>

#include <vector>

#include "common.h"

namespace icrec {

constexpr int CF_LDS_BYTES = 160 * 1024;  // the membership words of pass A: the whole LDS of a CU
constexpr int CF_A_THREADS = 1024;
constexpr int CF_MAX_BASKET = 65535;      // w is stored as uint16

struct Cf {
    int32_t* b_off = nullptr;    // [n_orders + 1]  de-duplicated baskets, CSR
    int32_t* b_items = nullptr;  // [nnz]
    int32_t* c_off = nullptr;    // [n_items + 1]   the transpose: item -> orders
    int32_t* c_orders = nullptr; // [nnz]
    int64_t n_orders = 0, n_items = 0, n_candidates = 0, nnz = 0;
    int tile = 16;               // queries per tile: 16, 8 or 4 membership bits per item
    int device = 0;
    int n_cu = 256;
};

// ------------------------------------------------------------------ create: de-duplicate, transpose
// One thread per raw basket position: it is kept when no earlier position of its basket holds the same item
// (dict.fromkeys).  Counts the kept positions per order and per item.
__global__ __launch_bounds__(256) void cf_dedup_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ items,
                                                       int64_t n_orders, int64_t nnz, uint8_t* __restrict__ keep,
                                                       int32_t* __restrict__ order_of, int32_t* __restrict__ b_len,
                                                       int32_t* __restrict__ c_len) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = n_orders;  // the last order whose offset is <= e (empty orders share an offset: skip them)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    const int32_t it = items[e];
    bool first = true;
    for (int64_t j = off[lo]; j < e; ++j) first = first && items[j] != it;
    keep[e] = first ? 1 : 0;
    order_of[e] = (int32_t)lo;
    if (first) {
        atomicAdd(&b_len[lo], 1);
        atomicAdd(&c_len[it], 1);
    }
}

// Kept positions go to a free slot of their basket and of their item's column (the order inside either does not
// matter: every sum over them is an integer sum).
__global__ __launch_bounds__(256) void cf_fill_kernel(const int32_t* __restrict__ items, const uint8_t* __restrict__ keep,
                                                      const int32_t* __restrict__ order_of, int64_t nnz,
                                                      const int32_t* __restrict__ b_off, const int32_t* __restrict__ c_off,
                                                      int32_t* __restrict__ b_cur, int32_t* __restrict__ c_cur,
                                                      int32_t* __restrict__ b_items, int32_t* __restrict__ c_orders) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz || !keep[e]) return;
    const int32_t o = order_of[e], it = items[e];
    b_items[b_off[o] + atomicAdd(&b_cur[o], 1)] = it;
    c_orders[c_off[it] + atomicAdd(&c_cur[it], 1)] = o;
}

// ------------------------------------------------------------------ pass A: w[tile][order][T]
// grid (n_tiles, order slices).  LDS: T membership bits per item, item i at bits [i*T, i*T + T) (T divides 32).
template <int T>
__global__ __launch_bounds__(CF_A_THREADS) void cf_weights_kernel(const int32_t* __restrict__ b_off,
                                                                  const int32_t* __restrict__ b_items, int64_t n_orders,
                                                                  int64_t n_items, const int32_t* __restrict__ hist_off,
                                                                  const int32_t* __restrict__ hist_items, int Q,
                                                                  uint16_t* __restrict__ w) {
    extern __shared__ uint32_t mem[];
    const int t = threadIdx.x;
    const int tile = blockIdx.x, q0 = tile * T;
    const int64_t words = (n_items * T + 31) >> 5;
    for (int64_t i = t; i < words; i += CF_A_THREADS) mem[i] = 0u;
    __syncthreads();
    for (int b = 0; b < T && q0 + b < Q; ++b) {
        const int32_t hb = hist_off[q0 + b], he = hist_off[q0 + b + 1];
        for (int32_t e = hb + t; e < he; e += CF_A_THREADS) {
            const int32_t h = hist_items[e];
            if (h >= 0 && (int64_t)h < n_items) {  // an id outside the catalog is skipped, never dereferenced
                const int64_t bit = (int64_t)h * T;
                atomicOr(&mem[bit >> 5], 1u << ((int)(bit & 31) + b));
            }
        }
    }
    __syncthreads();
    constexpr uint32_t MASK = (1u << T) - 1u;
    for (int64_t o = (int64_t)blockIdx.y * CF_A_THREADS + t; o < n_orders; o += (int64_t)gridDim.y * CF_A_THREADS) {
        uint32_t c[T];
#pragma unroll
        for (int b = 0; b < T; ++b) c[b] = 0u;
        const int32_t eb = b_off[o], ee = b_off[o + 1];
        for (int32_t e = eb; e < ee; ++e) {
            const int64_t bit = (int64_t)b_items[e] * T;
            const uint32_t bits = (mem[bit >> 5] >> (int)(bit & 31)) & MASK;
#pragma unroll
            for (int b = 0; b < T; ++b) c[b] += (bits >> b) & 1u;
        }
        uint32_t* dst = reinterpret_cast<uint32_t*>(w + ((size_t)tile * n_orders + o) * T);
#pragma unroll
        for (int b = 0; b < T; b += 2) dst[b >> 1] = c[b] | (c[b + 1] << 16);  // counts <= CF_MAX_BASKET
    }
}

// ------------------------------------------------------------------ pass B: keys[q][p]
// A wavefront per candidate, 64 / (T/4) column entries in flight: lane = (entry slot, part), a part is 4 queries
// (one 8-byte read of w).  Candidates in [n_candidates, P) are the pads of the sort: key 0.
template <int T>
__global__ __launch_bounds__(256) void cf_scores_kernel(const int32_t* __restrict__ c_off, const int32_t* __restrict__ c_orders,
                                                        int64_t n_orders, int64_t n_candidates, int64_t P,
                                                        const uint16_t* __restrict__ w,
                                                        const int32_t* __restrict__ hist_off,
                                                        const int32_t* __restrict__ hist_items, int Q, int gx,
                                                        u64* __restrict__ keys) {
    constexpr int PARTS = T / 4, SLOTS = 64 / PARTS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x / gx, chunk = blockIdx.x - tile * gx;
    const int part = lane % PARTS, slot = lane / PARTS;
    const int q0 = tile * T;
    const uint16_t* wt = w + (size_t)tile * n_orders * T + part * 4;
    for (int64_t p = (int64_t)chunk * 4 + wave; p < P; p += (int64_t)gx * 4) {
        if (p >= n_candidates) {
            if (lane < T && q0 + lane < Q) keys[(size_t)(q0 + lane) * P + p] = 0ull;
            continue;
        }
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        const int32_t eb = c_off[p], ee = c_off[p + 1];
        for (int32_t e = eb + slot; e < ee; e += SLOTS) {
            const uint2 v = *reinterpret_cast<const uint2*>(wt + (size_t)c_orders[e] * T);
            a0 += v.x & 0xFFFFu;
            a1 += v.x >> 16;
            a2 += v.y & 0xFFFFu;
            a3 += v.y >> 16;
        }
#pragma unroll
        for (int m = PARTS; m < 64; m <<= 1) {
            a0 += __shfl_xor(a0, m, 64);
            a1 += __shfl_xor(a1, m, 64);
            a2 += __shfl_xor(a2, m, 64);
            a3 += __shfl_xor(a3, m, 64);
        }
        if (slot == 0) {
            const uint32_t sc[4] = {a0, a1, a2, a3};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = q0 + part * 4 + j;
                if (q >= Q) break;
                int32_t lo = hist_off[q], hi = hist_off[q + 1];  // is p in the (ascending) history?
                while (lo < hi) {
                    const int32_t mid = lo + ((hi - lo) >> 1);
                    if ((int64_t)hist_items[mid] < p) lo = mid + 1; else hi = mid;
                }
                const bool left_out = lo < hist_off[q + 1] && (int64_t)hist_items[lo] == p;
                keys[(size_t)q * P + p] = left_out ? 0ull : (((u64)(sc[j] + 1u) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)p));
            }
        }
    }
}

// ------------------------------------------------------------------ top-k: sorted head of every chunk of CH keys
constexpr int CF_CHUNK_MAX = 8192;  // 64 KB of LDS
__global__ __launch_bounds__(256) void cf_chunk_topk_kernel(const u64* __restrict__ keys, int64_t P, int CH, int Q, int k,
                                                            u64* __restrict__ partial) {
    __shared__ u64 seg[CF_CHUNK_MAX];
    const int t = threadIdx.x, c = blockIdx.x, q = blockIdx.y;
    const u64* src = keys + (size_t)q * P + (size_t)c * CH;
    for (int i = t; i < CH; i += 256) seg[i] = src[i];
    __syncthreads();
    bitonic_sort_lds(seg, CH, t, 256);
    for (int e = t; e < k; e += 256) partial[((size_t)c * Q + q) * k + e] = e < CH ? seg[e] : 0ull;
}

__global__ __launch_bounds__(256) void cf_emit_kernel(const u64* __restrict__ keys, int64_t n, int64_t* __restrict__ out_idx,
                                                      int32_t* __restrict__ out_score) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 key = keys[i];
    out_idx[i] = key ? (int64_t)key_row(key) : -1;
    out_score[i] = key ? (int32_t)((uint32_t)(key >> 32) - 1u) : 0;
}

// ------------------------------------------------------------------ host side
struct CfPlan {
    int n_tiles = 0, CH = 0, n_chunks = 0;
    int64_t P = 0;
    size_t off_keys = 0, off_partial = 0, off_merged = 0, total = 0;  // w sits at offset 0
};

// k == 0: the complete order (no chunk lists).  total == 0: the shape is refused (`why` says so).
static CfPlan cf_plan(const Cf* cf, int Q, int k, const char** why) {
    CfPlan p;
    *why = nullptr;
    p.n_tiles = (Q + cf->tile - 1) / cf->tile;
    p.P = rank_pow2(cf->n_candidates);
    size_t at = align256((size_t)p.n_tiles * cf->n_orders * cf->tile * 2);
    p.off_keys = at;
    at += align256((size_t)Q * p.P * 8);
    if (k > 0) {
        int64_t ch = 1024;
        while (p.P / ch > MERGE_MAX_LISTS && ch < CF_CHUNK_MAX) ch <<= 1;
        if (ch > p.P) ch = p.P;
        if (p.P / ch > MERGE_MAX_LISTS) {
            *why = "more than 8,388,608 candidates: use icrec_cf_rank_all";
            return p;
        }
        p.CH = (int)ch;
        p.n_chunks = (int)(p.P / ch);
        p.off_partial = at;
        at += align256((size_t)p.n_chunks * Q * k * 8);
        p.off_merged = at;
        at += align256((size_t)Q * k * 8);
    }
    p.total = at;
    return p;
}

static int cf_check_call(const char* who, const Cf* cf, const int32_t* hist_off, int Q, const void* out) {
    ICREC_REQUIRE(cf && hist_off && out, "%s: NULL argument", who);
    // a query is a row of the sort's and the chunk kernel's grid
    ICREC_REQUIRE(Q >= 1 && Q <= 65535, "%s: n_queries must be in [1, 65535] (got %d)", who, Q);
    return ICREC_OK;
}

// passes A and B: the keys of every (query, candidate) into the workspace
static int cf_keys(const Cf* cf, const CfPlan& p, const int32_t* hist_off, const int32_t* hist_items, int Q, char* ws,
                   hipStream_t st) {
    uint16_t* w = reinterpret_cast<uint16_t*>(ws);
    u64* keys = reinterpret_cast<u64*>(ws + p.off_keys);
    // enough workgroups to fill the device when the tiles are few; each rebuilds the tile's membership words
    int64_t slices = (2 * cf->n_cu + p.n_tiles - 1) / p.n_tiles;
    const int64_t max_slices = (cf->n_orders + CF_A_THREADS - 1) / CF_A_THREADS;
    slices = slices > max_slices ? max_slices : slices;
    slices = slices < 1 ? 1 : (slices > 65535 ? 65535 : slices);
    const size_t lds = (size_t)((cf->n_items * cf->tile + 31) >> 5) * 4;
    int64_t gx = (p.P + 3) / 4;
    gx = gx > 1024 ? 1024 : gx;
    const dim3 ga(p.n_tiles, (unsigned)slices), gb((unsigned)(p.n_tiles * gx));
#define CF_LAUNCH(T)                                                                                                   \
    do {                                                                                                               \
        hipLaunchKernelGGL(cf_weights_kernel<T>, ga, dim3(CF_A_THREADS), lds, st, (const int32_t*)cf->b_off,           \
                           (const int32_t*)cf->b_items, cf->n_orders, cf->n_items, hist_off, hist_items, Q, w);        \
        hipLaunchKernelGGL(cf_scores_kernel<T>, gb, dim3(256), 0, st, (const int32_t*)cf->c_off,                       \
                           (const int32_t*)cf->c_orders, cf->n_orders, cf->n_candidates, p.P, (const uint16_t*)w,      \
                           hist_off, hist_items, Q, (int)gx, keys);                                                    \
    } while (0)
    if (cf->tile == 16) CF_LAUNCH(16);
    else if (cf->tile == 8) CF_LAUNCH(8);
    else CF_LAUNCH(4);
#undef CF_LAUNCH
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // namespace icrec

using namespace icrec;

extern "C" {

int icrec_cf_create(const int64_t* order_off, const int32_t* order_items, int64_t n_orders, int64_t n_items,
                    int64_t n_candidates, int device, icrec_cf** out) {
    ICREC_REQUIRE(order_off && out, "icrec_cf_create: NULL argument");
    ICREC_REQUIRE(n_orders >= 1 && n_orders < 0x7FFFFFFFll, "icrec_cf_create: n_orders must be in [1, 2^31)");
    ICREC_REQUIRE(n_items >= 1 && n_items < 0x7FFFFFFFll, "icrec_cf_create: n_items must be in [1, 2^31)");
    ICREC_REQUIRE(n_candidates >= 1 && n_candidates <= n_items && n_candidates < 0xFFFFFFFFll,
                  "icrec_cf_create: n_candidates must be in [1, n_items] and < 2^32");
    ICREC_REQUIRE(order_off[0] == 0, "icrec_cf_create: order_off[0] must be 0");
    for (int64_t o = 0; o < n_orders; ++o)
        ICREC_REQUIRE(order_off[o + 1] >= order_off[o], "icrec_cf_create: order_off decreases at order %lld", (long long)o);
    const int64_t nnz = order_off[n_orders];
    ICREC_REQUIRE(nnz < 0x7FFFFFFFll, "icrec_cf_create: 2^31 or more basket entries");
    ICREC_REQUIRE(nnz == 0 || order_items, "icrec_cf_create: NULL order_items");
    for (int64_t e = 0; e < nnz; ++e)
        ICREC_REQUIRE(order_items[e] >= 0 && order_items[e] < n_items,
                      "icrec_cf_create: item %d at position %lld is outside [0, %lld)", order_items[e], (long long)e,
                      (long long)n_items);
    // the widest tile whose membership words fit the LDS; ICREC_CF_TILE narrows it (A/B runs, tests of the narrow forms)
    int tile = 16;
    if (const char* env = getenv("ICREC_CF_TILE")) {
        const int v = atoi(env);
        ICREC_REQUIRE(v == 16 || v == 8 || v == 4, "icrec_cf_create: ICREC_CF_TILE must be 16, 8 or 4 (got %s)", env);
        tile = v;
    }
    while (tile > 4 && ((n_items * tile + 31) >> 5) * 4 > CF_LDS_BYTES) tile >>= 1;
    ICREC_REQUIRE(((n_items * tile + 31) >> 5) * 4 <= CF_LDS_BYTES,
                  "icrec_cf_create: %lld items do not fit the LDS membership words even at a 4-query tile (limit %d)",
                  (long long)n_items, CF_LDS_BYTES * 8 / 4);
    ICREC_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    ICREC_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("icrec_cf_create: device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
        return ICREC_ENODEV;
    }
    Cf* cf = new Cf();
    cf->n_orders = n_orders; cf->n_items = n_items; cf->n_candidates = n_candidates; cf->tile = tile;
    cf->device = device; cf->n_cu = prop.multiProcessorCount;
    // scratch of the build, freed before returning
    int64_t* d_off = nullptr;
    int32_t *d_items = nullptr, *d_order_of = nullptr, *d_blen = nullptr, *d_clen = nullptr, *d_stats = nullptr;
    uint8_t* d_keep = nullptr;
    auto release = [&]() {
        hipFree(d_off); hipFree(d_items); hipFree(d_order_of); hipFree(d_blen); hipFree(d_clen); hipFree(d_stats);
        hipFree(d_keep);
    };
    auto fail = [&](int rc) {
        release();
        icrec_cf_destroy(reinterpret_cast<icrec_cf*>(cf));
        return rc;
    };
    const size_t ne = nnz > 0 ? (size_t)nnz : 1;
    bool ok = hipMalloc(&d_off, (size_t)(n_orders + 1) * 8) == hipSuccess && hipMalloc(&d_items, ne * 4) == hipSuccess &&
              hipMalloc(&d_order_of, ne * 4) == hipSuccess && hipMalloc(&d_keep, ne) == hipSuccess &&
              hipMalloc(&d_blen, (size_t)n_orders * 4) == hipSuccess && hipMalloc(&d_clen, (size_t)n_items * 4) == hipSuccess &&
              hipMalloc(&d_stats, 16) == hipSuccess && hipMalloc(&cf->b_off, (size_t)(n_orders + 1) * 4) == hipSuccess &&
              hipMalloc(&cf->c_off, (size_t)(n_items + 1) * 4) == hipSuccess;
    if (!ok) {
        set_error("icrec_cf_create: hipMalloc failed (%lld orders, %lld items, %lld entries)", (long long)n_orders,
                  (long long)n_items, (long long)nnz);
        return fail(ICREC_ENOMEM);
    }
#define CF_TRY(call)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            set_error("icrec_cf_create: %s failed: %s", #call, hipGetErrorString(e_));                   \
            return fail(ICREC_EHIP);                                                                     \
        }                                                                                                \
    } while (0)
    CF_TRY(hipMemcpy(d_off, order_off, (size_t)(n_orders + 1) * 8, hipMemcpyHostToDevice));
    if (nnz > 0) CF_TRY(hipMemcpy(d_items, order_items, (size_t)nnz * 4, hipMemcpyHostToDevice));
    CF_TRY(hipMemsetAsync(d_blen, 0, (size_t)n_orders * 4, 0));
    CF_TRY(hipMemsetAsync(d_clen, 0, (size_t)n_items * 4, 0));
    const unsigned ge = (unsigned)((nnz + 255) / 256);
    if (nnz > 0)
        hipLaunchKernelGGL(cf_dedup_kernel, dim3(ge), dim3(256), 0, 0, (const int64_t*)d_off, (const int32_t*)d_items, n_orders,
                           nnz, d_keep, d_order_of, d_blen, d_clen);
    launch_prefix_sum(d_blen, n_orders, cf->b_off, d_stats, 0);      // stats[0]: the longest basket
    launch_prefix_sum(d_clen, n_items, cf->c_off, d_stats + 1, 0);  // stats[1]: the most frequent item's column
    CF_TRY(hipGetLastError());
    int32_t stats[2] = {0, 0}, kept = 0;
    CF_TRY(hipMemcpy(stats, d_stats, 8, hipMemcpyDeviceToHost));
    CF_TRY(hipMemcpy(&kept, cf->b_off + n_orders, 4, hipMemcpyDeviceToHost));
    cf->nnz = kept;
    if (stats[0] > CF_MAX_BASKET) {
        set_error("icrec_cf_create: a basket of %d distinct items (limit %d)", stats[0], CF_MAX_BASKET);
        return fail(ICREC_EINVAL);
    }
    // no score exceeds (longest column) x (longest basket); score + 1 must fit 31 bits
    if ((int64_t)stats[0] * stats[1] >= 0x7FFFFFFFll) {
        set_error("icrec_cf_create: scores may not fit 31 bits (longest basket %d x most frequent item %d)", stats[0], stats[1]);
        return fail(ICREC_EINVAL);
    }
    const size_t nk = kept > 0 ? (size_t)kept : 1;
    if (hipMalloc(&cf->b_items, nk * 4) != hipSuccess || hipMalloc(&cf->c_orders, nk * 4) != hipSuccess) {
        set_error("icrec_cf_create: hipMalloc of %zu basket entries failed", nk);
        return fail(ICREC_ENOMEM);
    }
    CF_TRY(hipMemsetAsync(d_blen, 0, (size_t)n_orders * 4, 0));  // the counts become the fill cursors
    CF_TRY(hipMemsetAsync(d_clen, 0, (size_t)n_items * 4, 0));
    if (nnz > 0)
        hipLaunchKernelGGL(cf_fill_kernel, dim3(ge), dim3(256), 0, 0, (const int32_t*)d_items, (const uint8_t*)d_keep,
                           (const int32_t*)d_order_of, nnz, (const int32_t*)cf->b_off, (const int32_t*)cf->c_off, d_blen,
                           d_clen, cf->b_items, cf->c_orders);
    CF_TRY(hipGetLastError());
    CF_TRY(hipStreamSynchronize(0));
    // pass A takes the whole LDS: set the attribute here, outside any capture
    int rc = tile == 16  ? ensure_dynamic_lds((const void*)cf_weights_kernel<16>, CF_LDS_BYTES)
             : tile == 8 ? ensure_dynamic_lds((const void*)cf_weights_kernel<8>, CF_LDS_BYTES)
                         : ensure_dynamic_lds((const void*)cf_weights_kernel<4>, CF_LDS_BYTES);
    if (rc != ICREC_OK) return fail(rc);
#undef CF_TRY
    release();
    *out = reinterpret_cast<icrec_cf*>(cf);
    return ICREC_OK;
}

int icrec_cf_destroy(icrec_cf* h) {
    Cf* cf = reinterpret_cast<Cf*>(h);
    if (!cf) return ICREC_OK;
    hipSetDevice(cf->device);
    hipFree(cf->b_off);
    hipFree(cf->b_items);
    hipFree(cf->c_off);
    hipFree(cf->c_orders);
    delete cf;
    return ICREC_OK;
}

int64_t icrec_cf_orders(const icrec_cf* h) { return h ? reinterpret_cast<const Cf*>(h)->n_orders : 0; }
int64_t icrec_cf_items(const icrec_cf* h) { return h ? reinterpret_cast<const Cf*>(h)->n_items : 0; }
int64_t icrec_cf_candidates(const icrec_cf* h) { return h ? reinterpret_cast<const Cf*>(h)->n_candidates : 0; }
int64_t icrec_cf_nnz(const icrec_cf* h) { return h ? reinterpret_cast<const Cf*>(h)->nnz : 0; }
int32_t icrec_cf_tile(const icrec_cf* h) { return h ? reinterpret_cast<const Cf*>(h)->tile : 0; }

size_t icrec_cf_rank_workspace_bytes(const icrec_cf* h, int32_t n_queries, int32_t k) {
    const Cf* cf = reinterpret_cast<const Cf*>(h);
    if (!cf || n_queries < 1 || n_queries > 65535 || k < 1 || k > ICREC_MAX_K) return 0;
    const char* why;
    return cf_plan(cf, n_queries, k, &why).total;
}

int icrec_cf_rank(icrec_cf* h, const int32_t* hist_off_dev, const int32_t* hist_items_dev, int32_t n_queries, int32_t k,
                  int64_t* out_idx_dev, int32_t* out_score_dev, void* ws, size_t ws_bytes, void* stream) {
    const Cf* cf = reinterpret_cast<const Cf*>(h);
    if (int rc = cf_check_call("icrec_cf_rank", cf, hist_off_dev, n_queries, out_idx_dev)) return rc;
    ICREC_REQUIRE(out_score_dev, "icrec_cf_rank: NULL argument");
    ICREC_REQUIRE(k >= 1 && k <= ICREC_MAX_K, "icrec_cf_rank: k must be in [1, %d] (got %d)", ICREC_MAX_K, k);
    const char* why;
    const CfPlan p = cf_plan(cf, n_queries, k, &why);
    ICREC_REQUIRE(p.total != 0, "icrec_cf_rank: %s", why);
    if (!ws || ws_bytes < p.total) {
        set_error("icrec_cf_rank: workspace too small (%zu < %zu)", ws_bytes, p.total);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(cf->device));
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    if (int rc = cf_keys(cf, p, hist_off_dev, hist_items_dev, n_queries, base, st)) return rc;
    const u64* keys = reinterpret_cast<const u64*>(base + p.off_keys);
    u64* partial = reinterpret_cast<u64*>(base + p.off_partial);
    u64* merged = reinterpret_cast<u64*>(base + p.off_merged);
    hipLaunchKernelGGL(cf_chunk_topk_kernel, dim3(p.n_chunks, n_queries), dim3(256), 0, st, keys, p.P, p.CH, n_queries, k,
                       partial);
    launch_merge(partial, p.n_chunks, n_queries, n_queries, k, nullptr, nullptr, merged, nullptr, st);
    const int64_t n = (int64_t)n_queries * k;
    hipLaunchKernelGGL(cf_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const u64*)merged, n, out_idx_dev,
                       out_score_dev);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

size_t icrec_cf_rank_all_workspace_bytes(const icrec_cf* h, int32_t n_queries) {
    const Cf* cf = reinterpret_cast<const Cf*>(h);
    if (!cf || n_queries < 1 || n_queries > 65535) return 0;
    const char* why;
    return cf_plan(cf, n_queries, 0, &why).total;
}

int icrec_cf_rank_all(icrec_cf* h, const int32_t* hist_off_dev, const int32_t* hist_items_dev, int32_t n_queries,
                      int64_t* out_rows_dev, void* ws, size_t ws_bytes, void* stream) {
    const Cf* cf = reinterpret_cast<const Cf*>(h);
    if (int rc = cf_check_call("icrec_cf_rank_all", cf, hist_off_dev, n_queries, out_rows_dev)) return rc;
    const char* why;
    const CfPlan p = cf_plan(cf, n_queries, 0, &why);
    if (!ws || ws_bytes < p.total) {
        set_error("icrec_cf_rank_all: workspace too small (%zu < %zu)", ws_bytes, p.total);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(cf->device));
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    if (int rc = cf_keys(cf, p, hist_off_dev, hist_items_dev, n_queries, base, st)) return rc;
    launch_rank_sort_emit(reinterpret_cast<u64*>(base + p.off_keys), cf->n_candidates, p.P, n_queries, 0, out_rows_dev, st);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
