// boost.hip — boosting each query's listed rows on a search result (icrec_boost_select): "buy it again".  Up to three
// launches on the caller's stream:
//   normalize_rows_kernel  the queries, as icrec_search normalises them -> the workspace
//   boost_score_kernel     every (query, listed entry): validity, exact cosine, + weight -> the workspace
//   boost_select_kernel    one workgroup per query: listed entries and the remaining candidates, sorted; the best top_k
// The definition (lists, validity, the cosine chain, the adjusted score, the ordering rule) is in include/icrec.h;
// tests/boost_reference.py states it in numpy.
#include <math.h>

#include "index.h"

namespace icrec {
namespace {

constexpr int SCORE_WAVES = 4;        // (query, 32-entry tile) items per scoring workgroup, one wave each
constexpr int SELECT_THREADS = 256;
constexpr int SELECT_MAX_KEYS = 2048;  // the bitonic network's width: 16 KB of LDS
static_assert(ICREC_MAX_BOOSTS + ICREC_MAX_K <= SELECT_MAX_KEYS, "a query's listed entries and candidates are sorted in LDS");
static_assert(ICREC_MAX_BOOSTS % 32 == 0, "the scoring kernel walks a list in tiles of 32 entries");

// A scored entry in the workspace: the adjusted score's bits above the flag VALID, or 0 for an invalid entry.
constexpr u64 SCORED_VALID = 1ull;

// The entries of query q's list that are read: [*start, *start + the result) of boost_rows.
__device__ __forceinline__ int list_len(const int32_t* __restrict__ off, int64_t q, int max_boosts, int* start) {
    const int lo = off[q], hi = off[q + 1];
    *start = lo;
    const int64_t n = (int64_t)hi - lo;
    return n <= 0 ? 0 : (n < max_boosts ? (int)n : max_boosts);
}

// ---------------------------------------------------------------- listed entries -> adjusted scores
// One wave per 32 listed entries of one query: the entries' rows are operand A of v_mfma_f32_32x32x2_f32, the query is
// every column of operand B, so each of the 32 columns of the tile holds the 32 cosines
//   s = 0; for j = 0 .. dim-1: s = fmaf(q_hat[j], p[j], s)
// by common.h's gathered_tile (fmaf(p[j], q_hat[j], s) is the same value); the query's values are one address for the
// whole wave.  Entry r's cosine is taken from column r: the lane r or r + 32 whose accumulator rows (acc_row) include r.
// An invalid entry (row outside the shard, excluded, or refused by the query's facet masks) gets the word 0; its lanes
// read row 0 of the shard instead, so nothing outside the rows is touched.  A tile without a valid entry does no math.
template <bool P16>
__global__ __launch_bounds__(SCORE_WAVES * 64) void boost_score_kernel(
    const void* __restrict__ rows, int K, int64_t n_rows, const float* __restrict__ qn, int Q,
    const int32_t* __restrict__ boost_off, const int32_t* __restrict__ boost_rows, const float* __restrict__ boost_w,
    int max_boosts, int n_tiles, const int32_t* __restrict__ excl_idx, const int32_t* __restrict__ excl_off, FacetArgs fa,
    u64* __restrict__ scored) {
    __shared__ uint32_t amask[SCORE_WAVES * FACET_LDS_WORDS];  // each wave's query's allow masks
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t item = (int64_t)blockIdx.x * SCORE_WAVES + wave;
    const bool live = item < (int64_t)Q * n_tiles;
    const int q = live ? (int)(item / n_tiles) : 0;
    const int t = live ? (int)(item % n_tiles) : 0;
    const bool facet = fa.allow != nullptr;  // the same for every workgroup
    uint32_t* am = amask + wave * FACET_LDS_WORDS;
    if (facet) {
        facet_load_masks(am, fa, q, 1, Q, lane, 64);
        __syncthreads();
    }
    if (!live) return;  // whole waves leave
    int start;
    const int n_b = list_len(boost_off, q, max_boosts, &start);
    if (t * 32 >= n_b) return;  // wave-uniform
    const int e = t * 32 + r;
    int row = 0;
    float w = 0.0f;
    bool valid = false;
    if (e < n_b) {
        row = boost_rows[(int64_t)start + e];
        valid = row >= 0 && row < n_rows;
        if (valid && excl_off != nullptr) valid = !excluded(excl_idx, excl_off[q], excl_off[q + 1], row);
        if (valid && facet) valid = facet_admits(am, 0, fa.rows[row]);
        if (valid && boost_w != nullptr) w = boost_w[(int64_t)start + e];
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    if (__ballot(valid) != 0ull) {  // wave-uniform
        const int64_t lr = valid ? row : 0;
        gathered_tile(acc, static_cast<const row_elem_t<P16>*>(rows) + lr * K, qn + (size_t)q * K, K, h);
    }
    // acc[i]: entry t * 32 + acc_row(i, lane) (operand A) against the query (every column).  Entry r sits in the
    // half of the wave with h == bit 2 of r; lanes r and r + 32 hold the same row, weight and validity.
    if (h != ((r >> 2) & 1) || e >= n_b) return;
    float cosine = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (acc_row(i, lane) == r) cosine = acc[i];
    const float w_eff = w >= 0.0f ? w : 0.0f;  // a NaN or a negative weight counts as 0
    const float a = w_eff == 0.0f ? cosine : __fadd_rn(cosine, w_eff);
    scored[(size_t)q * max_boosts + e] = valid ? (((u64)__float_as_uint(a) << 32) | SCORED_VALID) : 0ull;
}

// ---------------------------------------------------------------- selection
// The ranking key of (score, local row) under icrec_search's order with -0 == +0: make_key of the score + 0.  A score
// of -0 keeps its bits in the output: its row is noted in `nz` (a list that is empty for all practical inputs).
__device__ __forceinline__ u64 order_key(float v, uint32_t row, uint32_t* nz, int* nz_n) {
    if (__float_as_uint(v) == 0x80000000u) nz[atomicAdd(nz_n, 1)] = row;
    return make_key(v + 0.0f, row);
}

// One workgroup per query.  Its n_b scored entries and its k candidates become keys in LDS (invalid ones, and the
// candidates whose row is among the n_b listed rows - a binary search in the sorted list -, become key 0), a bitonic
// network over the next power of two sorts them best first, and the first top_k are written, then the pads.
__global__ __launch_bounds__(SELECT_THREADS) void boost_select_kernel(
    const u64* __restrict__ scored, const int32_t* __restrict__ boost_off, const int32_t* __restrict__ boost_rows,
    int max_boosts, const int64_t* __restrict__ cand_idx, const float* __restrict__ cand_score, int k, int64_t n_rows,
    int64_t row_offset, int top_k, int64_t* __restrict__ out_idx, float* __restrict__ out_score) {
    __shared__ u64 keys[SELECT_MAX_KEYS];
    __shared__ uint32_t nz[ICREC_MAX_BOOSTS + ICREC_MAX_K];
    __shared__ int nz_n;
    const int tid = threadIdx.x;
    const size_t q = blockIdx.x;
    int start = 0;
    const int n_b = max_boosts > 0 ? list_len(boost_off, (int64_t)q, max_boosts, &start) : 0;
    const int n = n_b + (cand_idx != nullptr ? k : 0);
    int P = 64;
    while (P < n) P <<= 1;  // <= SELECT_MAX_KEYS
    if (tid == 0) nz_n = 0;
    __syncthreads();
    for (int i = tid; i < P; i += SELECT_THREADS) {
        u64 key = 0ull;
        if (i < n_b) {
            const u64 s = scored[q * max_boosts + i];
            if (s & SCORED_VALID) key = order_key(__uint_as_float((uint32_t)(s >> 32)), (uint32_t)boost_rows[(int64_t)start + i], nz, &nz_n);
        } else if (i < n) {
            const int j = i - n_b;
            const int64_t lr = local_row(cand_idx[q * k + j], row_offset, n_rows);
            if (lr >= 0 && !(lr <= 0x7FFFFFFFll && excluded(boost_rows, start, start + n_b, (int)lr)))
                key = order_key(cand_score[q * k + j], (uint32_t)lr, nz, &nz_n);
        }
        keys[i] = key;
    }
    __syncthreads();
    bitonic_sort_lds(keys, P, tid, SELECT_THREADS);
    for (int i = tid; i < top_k; i += SELECT_THREADS) {
        const u64 key = i < P ? keys[i] : 0ull;
        int64_t row = -1;
        float s = 0.0f;
        if (key != 0ull) {
            const uint32_t lr = key_row(key);
            row = row_offset + (int64_t)lr;
            s = key_score(key);
            if (s == 0.0f)
                for (int z = 0; z < nz_n; ++z)
                    if (nz[z] == lr) s = -0.0f;
        }
        out_idx[q * top_k + i] = row;
        out_score[q * top_k + i] = s;
    }
}

}  // namespace
}  // namespace icrec

using namespace icrec;

extern "C" {

size_t icrec_boost_select_workspace_bytes(const icrec_index* h, int32_t n_queries, int32_t max_boosts) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    if (!ix || n_queries < 1 || max_boosts < 0 || max_boosts > ICREC_MAX_BOOSTS) return 0;
    if (max_boosts == 0) return 256;  // candidates only: nothing is scored
    return align256((size_t)n_queries * (size_t)ix->dim * sizeof(float)) + align256((size_t)n_queries * max_boosts * sizeof(u64));
}

int icrec_boost_select(icrec_index* h, const float* q_dev, int32_t n_queries, const int64_t* cand_idx_dev,
                       const float* cand_score_dev, int32_t k, const int32_t* boost_off_dev, const int32_t* boost_rows_dev,
                       const float* boost_w_dev, int32_t max_boosts, const int32_t* excl_idx_dev, const int32_t* excl_off_dev,
                       const uint32_t* allow_dev, int32_t top_k, int64_t* out_idx_dev, float* out_score_dev, void* ws,
                       size_t ws_bytes, void* stream) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    ICREC_REQUIRE(ix && q_dev && boost_off_dev && out_idx_dev && out_score_dev && ws, "icrec_boost_select: NULL argument");
    ICREC_REQUIRE(max_boosts >= 0 && max_boosts <= ICREC_MAX_BOOSTS, "icrec_boost_select: max_boosts must be in [0, %d] (got %d)",
                  ICREC_MAX_BOOSTS, max_boosts);
    ICREC_REQUIRE(boost_rows_dev != nullptr || max_boosts == 0, "icrec_boost_select: NULL boost_rows with max_boosts > 0");
    ICREC_REQUIRE((cand_idx_dev == nullptr) == (cand_score_dev == nullptr),
                  "icrec_boost_select: cand_idx and cand_score must both be set or both NULL");
    ICREC_REQUIRE((excl_idx_dev == nullptr) == (excl_off_dev == nullptr),
                  "icrec_boost_select: excl_idx and excl_off must both be set or both NULL");
    ICREC_REQUIRE(n_queries >= 1, "icrec_boost_select: n_queries must be >= 1 (got %d)", n_queries);
    const bool cands = cand_idx_dev != nullptr;
    ICREC_REQUIRE(!cands || (k >= 1 && k <= ICREC_MAX_K), "icrec_boost_select: k must be in [1, %d] (got %d)", ICREC_MAX_K, k);
    ICREC_REQUIRE(top_k >= 1 && top_k <= ICREC_MAX_K && (!cands || top_k <= k),
                  "icrec_boost_select: top_k must be in [1, %d] (got %d)", cands ? k : ICREC_MAX_K, top_k);
    ICREC_REQUIRE(cands || max_boosts > 0, "icrec_boost_select: neither candidates nor listed rows (max_boosts is 0)");
    ICREC_REQUIRE(allow_dev == nullptr || ix->facets != nullptr, "icrec_boost_select: allow masks on an index without facets");
    const int n_tiles = (max_boosts + 31) / 32;
    const int64_t score_blocks = ((int64_t)n_queries * n_tiles + SCORE_WAVES - 1) / SCORE_WAVES;
    ICREC_REQUIRE(score_blocks <= 0x7FFFFFFFll, "icrec_boost_select: %d queries of %d listed rows are too many for one call",
                  n_queries, max_boosts);
    const size_t need = icrec_boost_select_workspace_bytes(h, n_queries, max_boosts);
    if (ws_bytes < need) {
        set_error("icrec_boost_select: workspace too small (%zu < %zu)", ws_bytes, need);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    float* qn = static_cast<float*>(ws);
    u64* scored = reinterpret_cast<u64*>(static_cast<char*>(ws) + align256((size_t)n_queries * (size_t)ix->dim * sizeof(float)));
    if (max_boosts > 0) {
        hipLaunchKernelGGL(normalize_rows_kernel<false>, dim3((unsigned)((n_queries + 3) / 4)), dim3(256), 0, st, q_dev,
                           (void*)qn, (int64_t)n_queries, (int64_t)n_queries, ix->dim, 1e-12f, 0);
        const FacetArgs fa{ix->facets, allow_dev, ix->n_facets};
        ScopedTimer tm(T_BOOST_SCORE, st);
        hipLaunchKernelGGL((rows_are_bf16(ix) ? boost_score_kernel<true> : boost_score_kernel<false>), dim3((unsigned)score_blocks),
                           dim3(SCORE_WAVES * 64), 0, st, (const void*)ix->rows, ix->dim, ix->n_rows, (const float*)qn,
                           n_queries, boost_off_dev, boost_rows_dev, boost_w_dev, max_boosts, n_tiles, excl_idx_dev,
                           excl_off_dev, fa, scored);
    }
    {
        ScopedTimer tm(T_BOOST_SELECT, st);
        hipLaunchKernelGGL(boost_select_kernel, dim3((unsigned)n_queries), dim3(SELECT_THREADS), 0, st, (const u64*)scored,
                           boost_off_dev, boost_rows_dev, max_boosts, cand_idx_dev, cand_score_dev, k, ix->n_rows,
                           ix->row_offset, top_k, out_idx_dev, out_score_dev);
    }
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
