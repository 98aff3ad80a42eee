// mmr.hip — diversity re-selection of a search result on the device (icrec_mmr_select): Maximal Marginal Relevance
// (Carbonell & Goldstein 1998) over each query's k candidates.  Two launches on the caller's stream:
//   mmr_gram_kernel    every query's k x k matrix of candidate-candidate similarities -> the workspace
//   mmr_select_kernel  the greedy picks, one wave per query, the query's matrix in LDS
// The definition (validity, the similarity chain, the three roundings of a pick's value, the ordering rule) is in
// include/icrec.h; tests/mmr_reference.py states it in numpy.
#include <math.h>

#include "index.h"

namespace icrec {
namespace {

constexpr int GRAM_WAVES = 4;      // (query, tile) items per Gram workgroup, one wave each
constexpr int SELECT_THREADS = 256;  // all of them copy the matrix into LDS, the first wave selects
static_assert(ICREC_MAX_K <= 128, "a lane of the selection wave holds two candidates; the matrix is at most 64 KB of LDS");

// ---------------------------------------------------------------- candidate x candidate similarities
// One wave per 32 x 32 tile of a query's matrix, lower triangle of tiles only (tile (ti, tj), tj <= ti, is item
// ti (ti + 1) / 2 + tj of the query); a single request at k = 128 is ten waves on ten compute units.
// G[i][j] = the fp32 chain s = fmaf(row_i[d], row_j[d], s) over d ascending, by common.h's gathered_tile with both
// operands gathered from the stored rows - a tile's 64 rows are read by one wave only.  fmaf(a, b, s) == fmaf(b, a, s),
// so the matrix is bit-symmetric and the transposed entry of an off-diagonal tile is a second store of the same value.
// Entries in the row or column of an invalid candidate are not stored (nor read by the selection); the lanes of such
// a candidate read row 0 of the shard instead of the candidate's row, so nothing outside the rows is touched.
template <bool P16>
__global__ __launch_bounds__(GRAM_WAVES * 64) void mmr_gram_kernel(const void* __restrict__ rows, int K, int64_t n_rows,
                                                                   int64_t row_offset, const int64_t* __restrict__ cand,
                                                                   int Q, int k, int n_tiles, float* __restrict__ G) {
    typedef row_elem_t<P16> Row;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t item = (int64_t)blockIdx.x * GRAM_WAVES + (threadIdx.x >> 6);
    if (item >= (int64_t)Q * n_tiles) return;  // whole waves leave
    const int64_t q = item / n_tiles;
    const int t = (int)(item % n_tiles);
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int ia = ti * 32 + r, ib = tj * 32 + r;
    const int64_t la = ia < k ? local_row(cand[q * k + ia], row_offset, n_rows) : -1;
    const int64_t lb = ib < k ? local_row(cand[q * k + ib], row_offset, n_rows) : -1;
    const unsigned long long valid_a = __ballot(la >= 0), valid_b = __ballot(lb >= 0);
    if (valid_a == 0ull || valid_b == 0ull) return;  // wave-uniform: nothing of this tile is ever read
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    const Row* base = static_cast<const Row*>(rows);
    gathered_tile(acc, base + (la >= 0 ? la : 0) * K, base + (lb >= 0 ? lb : 0) * K, K, h);
    // acc[e]: row ti * 32 + acc_row(e, lane) (operand A), column tj * 32 + r (operand B); both < k when valid
    float* Gq = G + (size_t)q * k * k;
    const bool col_ok = (valid_b >> r) & 1ull;  // (lanes r and r + 32 hold the same candidate)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int ar = acc_row(e, lane);
        if (col_ok && ((valid_a >> ar) & 1ull)) {
            const int i = ti * 32 + ar, j = tj * 32 + r;
            Gq[(size_t)i * k + j] = acc[e];
            if (ti != tj) Gq[(size_t)j * k + i] = acc[e];
        }
    }
}

// ---------------------------------------------------------------- greedy selection
// One workgroup per query: its k x k matrix goes to LDS (every pick reads one row of it, and which row is known only
// after the pick before), then the first wave picks; lane l owns candidates l and l + 64.  A pick is the wave maximum
// of common.h's value_pos_key, key 0 = not a candidate.
__global__ __launch_bounds__(SELECT_THREADS) void mmr_select_kernel(const float* __restrict__ G,
                                                                    const int64_t* __restrict__ cand,
                                                                    const float* __restrict__ rel, int64_t n_rows,
                                                                    int64_t row_offset, int k, int top_k, float lambda,
                                                                    float oml, int64_t* __restrict__ out_idx,
                                                                    float* __restrict__ out_rel) {
    extern __shared__ float g[];  // [k][k]; the entries of invalid candidates are whatever the workspace held
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t q = blockIdx.x;
    const float* Gq = G + q * k * k;
    if ((k & 1) == 0) {  // k * k floats are whole 16-byte groups, and the query's matrix starts on one
        for (int i = tid; i < k * k / 4; i += SELECT_THREADS)
            reinterpret_cast<f32x4*>(g)[i] = reinterpret_cast<const f32x4*>(Gq)[i];
    } else {
        for (int i = tid; i < k * k; i += SELECT_THREADS) g[i] = Gq[i];
    }
    __syncthreads();
    if (tid >= 64) return;
    float rl[2], ms[2];
    int64_t ix[2];
    bool avail[2];  // valid and not yet selected
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s * 64 + lane;
        rl[s] = j < k ? rel[q * k + j] : 0.0f;
        ix[s] = j < k ? cand[q * k + j] : -1;
        avail[s] = local_row(ix[s], row_offset, n_rows) >= 0;
        ms[s] = -INFINITY;
    }
    int t = 0;
    for (; t < top_k; ++t) {
        u64 key = 0ull;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // three roundings, never fused: the two products, then the difference (the first pick is by rel alone)
            const float v = t == 0 ? rl[s] : __fsub_rn(__fmul_rn(lambda, rl[s]), __fmul_rn(oml, ms[s]));
            const u64 ks = avail[s] ? value_pos_key(v, s * 64 + lane) : 0ull;
            key = ks > key ? ks : key;
        }
        key = wave_max_u64(key);
        if (key == 0ull) break;  // wave-uniform: no valid candidate is left
        const int p = (int)(0xFFFFFFFFu - (uint32_t)key);
        if (lane == (p & 63)) {
            const bool hi = p >= 64;
            out_idx[q * top_k + t] = hi ? ix[1] : ix[0];
            out_rel[q * top_k + t] = hi ? rl[1] : rl[0];
            avail[0] = avail[0] && hi;
            avail[1] = avail[1] && !hi;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int j = s * 64 + lane;
            const float sim = j < k ? g[p * k + j] : 0.0f;
            ms[s] = sim > ms[s] ? sim : ms[s];
        }
    }
    for (int i = t + lane; i < top_k; i += 64) {
        out_idx[q * top_k + i] = -1;
        out_rel[q * top_k + i] = 0.0f;
    }
}

bool shape_ok(int32_t n_queries, int32_t k) { return n_queries >= 1 && k >= 1 && k <= ICREC_MAX_K; }

}  // namespace
}  // namespace icrec

using namespace icrec;

extern "C" {

size_t icrec_mmr_select_workspace_bytes(const icrec_index* h, int32_t n_queries, int32_t k) {
    if (!h || !shape_ok(n_queries, k)) return 0;
    return align256((size_t)n_queries * k * k * sizeof(float));
}

int icrec_mmr_select(icrec_index* h, const int64_t* cand_idx_dev, const float* rel_dev, int32_t n_queries, int32_t k,
                     int32_t top_k, float lambda, int64_t* out_idx_dev, float* out_rel_dev, void* ws, size_t ws_bytes,
                     void* stream) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    ICREC_REQUIRE(ix && cand_idx_dev && rel_dev && out_idx_dev && out_rel_dev && ws, "icrec_mmr_select: NULL argument");
    ICREC_REQUIRE(n_queries >= 1, "icrec_mmr_select: n_queries must be >= 1 (got %d)", n_queries);
    ICREC_REQUIRE(k >= 1 && k <= ICREC_MAX_K, "icrec_mmr_select: k must be in [1, %d] (got %d)", ICREC_MAX_K, k);
    ICREC_REQUIRE(top_k >= 1 && top_k <= k, "icrec_mmr_select: top_k must be in [1, k = %d] (got %d)", k, top_k);
    ICREC_REQUIRE(lambda >= 0.0f && lambda <= 1.0f, "icrec_mmr_select: lambda must be in [0, 1] (got %g)", (double)lambda);
    const int tiles = (k + 31) / 32, n_tiles = tiles * (tiles + 1) / 2;
    const int64_t gram_blocks = ((int64_t)n_queries * n_tiles + GRAM_WAVES - 1) / GRAM_WAVES;
    ICREC_REQUIRE(gram_blocks <= 0x7FFFFFFFll, "icrec_mmr_select: %d queries of %d candidates are too many for one call",
                  n_queries, k);
    const size_t need = icrec_mmr_select_workspace_bytes(h, n_queries, k);
    if (ws_bytes < need) {
        set_error("icrec_mmr_select: workspace too small (%zu < %zu)", ws_bytes, need);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    float* G = static_cast<float*>(ws);
    const float oml = 1.0f - lambda;
    {
        ScopedTimer tm(T_MMR_GRAM, st);
        hipLaunchKernelGGL((rows_are_bf16(ix) ? mmr_gram_kernel<true> : mmr_gram_kernel<false>), dim3((unsigned)gram_blocks),
                           dim3(GRAM_WAVES * 64), 0, st, (const void*)ix->rows, ix->dim, ix->n_rows, ix->row_offset,
                           cand_idx_dev, n_queries, k, n_tiles, G);
    }
    {
        ScopedTimer tm(T_MMR_SELECT, st);
        hipLaunchKernelGGL(mmr_select_kernel, dim3((unsigned)n_queries), dim3(SELECT_THREADS), (size_t)k * k * sizeof(float), st,
                           (const float*)G, cand_idx_dev, rel_dev, ix->n_rows, ix->row_offset, k, top_k, lambda, oml,
                           out_idx_dev, out_rel_dev);
    }
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
