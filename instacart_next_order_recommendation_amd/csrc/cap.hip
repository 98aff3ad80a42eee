// cap.hip — per-facet caps on a search result on the device (icrec_cap_select): "at most two products of one aisle,
// at most five of one department".  One launch on the caller's stream, one wave per query:
//   cap_select_kernel  the sequential greedy walk over the query's k candidates, the count tables in LDS
// The definition (validity, prior picks, the walk, the state, the next masks) and the round scheme that makes the
// answer the capped top_k of the whole catalog are in include/icrec.h; tests/cap_reference.py states them in numpy.
#include "index.h"

namespace icrec {
namespace {

constexpr int CAP_VALUES = 256;  // values of one facet byte
static_assert(ICREC_MAX_K <= 128, "a lane of the wave holds two candidates and two picks");
static_assert(ICREC_MAX_FACETS * ICREC_FACET_MASK_WORDS <= 64, "one lane per word of a query's next masks");

// Lane l owns candidates l and l + 64, and picks l and l + 64 (for the test "is this row already picked").  The
// candidates' rows, score bits and facet words go to LDS once, gathered by all lanes; the walk then reads them at
// wave-uniform addresses, so every lane takes the same branches and holds the same `picks`.  Lane 0 alone writes the
// count tables; the barrier of the one-wave workgroup after a write orders it before the next candidate's reads.
// fw of an invalid candidate is FW_INVALID and its facet word is never read.
constexpr uint32_t FW_INVALID = 0xFFFFFFFFu;

__global__ __launch_bounds__(64) void cap_select_kernel(const uint16_t* __restrict__ facets, int n_facets, int64_t n_rows,
                                                        int64_t row_offset, const int64_t* __restrict__ cand,
                                                        const float* __restrict__ cand_score, int k,
                                                        const int32_t* __restrict__ caps,
                                                        const int32_t* __restrict__ n_prior, const uint32_t* allow,
                                                        int top_k, int64_t* __restrict__ out_idx,
                                                        float* __restrict__ out_score, int32_t* __restrict__ out_state,
                                                        uint32_t* allow_next) {
    __shared__ int count[ICREC_MAX_FACETS][CAP_VALUES];
    __shared__ int64_t c_row[ICREC_MAX_K];
    __shared__ uint32_t c_fw[ICREC_MAX_K];
    __shared__ float c_sc[ICREC_MAX_K];
    const int lane = threadIdx.x;
    const size_t q = blockIdx.x;
    for (int i = lane; i < ICREC_MAX_FACETS * CAP_VALUES; i += 64) (&count[0][0])[i] = 0;
    bool pad = false;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = s * 64 + lane;
        if (j < k) {
            const int64_t c = cand[q * k + j];
            const int64_t r = local_row(c, row_offset, n_rows);
            pad = pad || c < 0;
            c_row[j] = c;
            c_fw[j] = r >= 0 ? (uint32_t)facets[r] : FW_INVALID;
            c_sc[j] = cand_score[q * k + j];
        }
    }
    const bool any_pad = __any(pad) != 0;
    int cap[ICREC_MAX_FACETS];
#pragma unroll
    for (int f = 0; f < ICREC_MAX_FACETS; ++f) {
        const int c = caps[q * ICREC_MAX_FACETS + f];
        cap[f] = f < n_facets && c > 0 ? c : 0;  // 0: the facet is not capped
    }
    int p0 = n_prior ? n_prior[q] : 0;
    p0 = p0 < 0 ? 0 : p0 > top_k ? top_k : p0;
    __syncthreads();  // the tables are zero
    int64_t pick[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = s * 64 + lane;
        pick[s] = -1;  // no valid candidate is negative
        if (i < p0) {
            pick[s] = out_idx[q * top_k + i];
            const int64_t r = local_row(pick[s], row_offset, n_rows);
            if (r >= 0) {
                const uint32_t fw = facets[r];
                atomicAdd(&count[0][fw & 255u], 1);
                atomicAdd(&count[1][(fw >> 8) & 255u], 1);
            }
        }
    }
    __syncthreads();  // the candidates and the priors' counts are in LDS
    int picks = p0;
    for (int j = 0; j < k && picks < top_k; ++j) {
        const uint32_t fw = c_fw[j];
        if (fw == FW_INVALID) continue;
        const int64_t c = c_row[j];
        if (__any(pick[0] == c || pick[1] == c)) continue;
        const int v0 = fw & 255u, v1 = (fw >> 8) & 255u;
        const int n0 = count[0][v0], n1 = count[1][v1];
        if ((cap[0] && n0 >= cap[0]) || (cap[1] && n1 >= cap[1])) continue;
        if (lane == (picks & 63)) {
            const bool hi = picks >= 64;
            pick[0] = hi ? pick[0] : c;
            pick[1] = hi ? c : pick[1];
            out_idx[q * top_k + picks] = c;
            out_score[q * top_k + picks] = c_sc[j];
        }
        if (lane == 0) {
            count[0][v0] = n0 + 1;
            count[1][v1] = n1 + 1;
        }
        ++picks;
        __syncthreads();
    }
    for (int i = picks + lane; i < top_k; i += 64) {
        out_idx[q * top_k + i] = -1;
        out_score[q * top_k + i] = 0.0f;
    }
    if (lane < 2) out_state[q * 2 + lane] = lane == 0 ? picks : (picks == top_k || any_pad) ? 1 : 0;
    if (allow_next && lane < n_facets * ICREC_FACET_MASK_WORDS) {
        const int f = lane / ICREC_FACET_MASK_WORDS, w = lane % ICREC_FACET_MASK_WORDS;
        const size_t o = (q * n_facets + f) * ICREC_FACET_MASK_WORDS + w;
        uint32_t m = allow ? allow[o] : ~0u;  // (read before the store: allow_next may be allow)
        if (cap[f])
            for (int b = 0; b < 32; ++b)
                if (count[f][w * 32 + b] >= cap[f]) m &= ~(1u << b);
        allow_next[o] = m;
    }
}

}  // namespace
}  // namespace icrec

using namespace icrec;

extern "C" {

int icrec_cap_select(icrec_index* h, const int64_t* cand_idx_dev, const float* cand_score_dev, int32_t n_queries, int32_t k,
                     const int32_t* caps_dev, const int32_t* n_prior_dev, const uint32_t* allow_dev, int32_t top_k,
                     int64_t* out_idx_dev, float* out_score_dev, int32_t* out_state_dev, uint32_t* allow_next_dev,
                     void* stream) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    ICREC_REQUIRE(ix && cand_idx_dev && cand_score_dev && caps_dev && out_idx_dev && out_score_dev && out_state_dev,
                  "icrec_cap_select: NULL argument");
    ICREC_REQUIRE(n_queries >= 1, "icrec_cap_select: n_queries must be >= 1 (got %d)", n_queries);
    ICREC_REQUIRE(k >= 1 && k <= ICREC_MAX_K, "icrec_cap_select: k must be in [1, %d] (got %d)", ICREC_MAX_K, k);
    ICREC_REQUIRE(top_k >= 1 && top_k <= ICREC_MAX_K, "icrec_cap_select: top_k must be in [1, %d] (got %d)", ICREC_MAX_K,
                  top_k);
    ICREC_REQUIRE(ix->facets && ix->n_facets >= 1, "icrec_cap_select: the index has no facets (icrec_index_set_facets)");
    ICREC_HIP(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    {
        ScopedTimer tm(T_CAP_SELECT, st);
        hipLaunchKernelGGL(cap_select_kernel, dim3((unsigned)n_queries), dim3(64), 0, st, (const uint16_t*)ix->facets,
                           ix->n_facets, ix->n_rows, ix->row_offset, cand_idx_dev, cand_score_dev, k, caps_dev, n_prior_dev,
                           allow_dev, top_k, out_idx_dev, out_score_dev, out_state_dev, allow_next_dev);
    }
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
