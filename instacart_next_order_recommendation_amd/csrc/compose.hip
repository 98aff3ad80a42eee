// compose.hip — queries composed from stored rows (icrec_compose_queries): "similar items", "more like these, less like
// those" (Rocchio feedback), a profile from a basket.  One launch on the caller's stream:
//   compose_kernel  one workgroup per query: q' = a * q_hat + sum of w_j * row_j, the terms in list order
// The definition (the base's normalisation, validity, the two roundings of a term, the order of the sum) is in
// include/icrec.h; tests/compose_reference.py states it in numpy.
#include <math.h>

#include "index.h"

namespace icrec {
namespace {

constexpr int COMPOSE_THREADS = 256;  // 4 waves; a thread owns one 16-byte piece of a row per pass over the features
constexpr int COMPOSE_DEPTH = 8;      // stored rows whose loads a thread issues before the first add
static_assert(ICREC_MAX_TERMS * (sizeof(int32_t) + sizeof(float)) <= 16384, "a query's terms are staged in LDS");

// One workgroup per query.  The per-feature chains acc[j] = acc[j] + (w * p[j]) are independent of each other and
// ordered along the terms, so the parallelism is the features (16 bytes of every stored row per thread: 4 fp32 or 8
// bf16 values; at dim 32 most threads own nothing, at 4,096 a thread walks several pieces) and the loads in flight: a
// thread issues the loads of COMPOSE_DEPTH terms, then adds them in list order.  A query's terms are never split
// over threads.
// The segment is staged in LDS first - the rows coalesced, an invalid term (row outside [0, n_rows), weight not finite)
// as row -1 - so that the main loop's row numbers are LDS reads, not a dependent global load per term.  A term that
// does not count loads row 0 of the index in its place (its own row is never read) and its sum is dropped by a select:
// without a branch between the loads, all COMPOSE_DEPTH of them are in flight before the first wait.
// Wave 0 computes the base's norm in normalize_rows_kernel's lane order (64 strided fmaf partials, the xor butterfly)
// and publishes den through LDS; q_hat[j] = x[j] / den is then that kernel's value.
template <bool P16>
__global__ __launch_bounds__(COMPOSE_THREADS) void compose_kernel(
    const void* __restrict__ rows, int K, int64_t n_rows, const float* __restrict__ base, const float* __restrict__ base_w,
    const int32_t* __restrict__ term_off, const int32_t* __restrict__ term_rows, const float* __restrict__ term_w,
    int max_terms, float* __restrict__ out) {
    typedef row_elem_t<P16> Row;
    constexpr int P = P16 ? 8 : 4;  // features of one piece
    __shared__ int32_t t_row[ICREC_MAX_TERMS + COMPOSE_DEPTH];  // -1: an invalid term, or the pad behind the last one
    __shared__ float t_w[ICREC_MAX_TERMS + COMPOSE_DEPTH];
    __shared__ float den_s;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    int n_t = 0;
    if (max_terms > 0) {
        const int lo = term_off[q], hi = term_off[q + 1];
        const int64_t n = (int64_t)hi - lo;
        n_t = n <= 0 ? 0 : (n < max_terms ? (int)n : max_terms);
        for (int i = tid; i < n_t + COMPOSE_DEPTH; i += COMPOSE_THREADS) {  // (the main loop reads whole groups)
            int row = -1;
            float w = 0.0f;
            if (i < n_t) {
                row = term_rows[(int64_t)lo + i];
                w = term_w != nullptr ? term_w[(int64_t)lo + i] : 1.0f;
                if (!(row >= 0 && row < n_rows && finite_f32(w))) row = -1;
            }
            t_row[i] = row;
            t_w[i] = w;
        }
    }
    if (base != nullptr && tid < 64) {
        const float* xr = base + q * K;
        float s = 0.0f;
        for (int i = tid; i < K; i += 64) {
            const float v = xr[i];
            s = fmaf(v, v, s);
        }
        const float nrm = sqrtf(wave_sum_f32(s));
        if (tid == 0) den_s = nrm > 1e-12f ? nrm : 1e-12f;
    }
    __syncthreads();
    float a = 0.0f, den = 1.0f;
    if (base != nullptr) {
        a = base_w != nullptr ? base_w[q] : 1.0f;
        if (!finite_f32(a)) a = 0.0f;
        den = den_s;
    }
    const Row* stored = static_cast<const Row*>(rows);
    for (int c = tid; c < K / P; c += COMPOSE_THREADS) {  // features c * P .. c * P + P - 1, inside every row
        float acc[P];
#pragma unroll
        for (int j = 0; j < P; ++j) acc[j] = 0.0f;
        if (base != nullptr) {
#pragma unroll
            for (int v = 0; v < P / 4; ++v) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(base + q * K + c * P + 4 * v);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * v + j] = __fmul_rn(a, x[j] / den);
            }
        }
        const Row* col = stored + c * P;
        for (int t0 = 0; t0 < n_t; t0 += COMPOSE_DEPTH) {
            u32x4 piece[COMPOSE_DEPTH];
            int row[COMPOSE_DEPTH];
#pragma unroll
            for (int u = 0; u < COMPOSE_DEPTH; ++u) {  // every load is issued: a term that does not count reads row 0
                row[u] = t_row[t0 + u];
                piece[u] = *reinterpret_cast<const u32x4*>(col + (int64_t)(row[u] < 0 ? 0 : row[u]) * K);
            }
#pragma unroll
            for (int u = 0; u < COMPOSE_DEPTH; ++u) {
                const float w = t_w[t0 + u];
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const float sum = __fadd_rn(acc[j], __fmul_rn(w, piece_value<P16>(piece[u], j)));
                    acc[j] = row[u] < 0 ? acc[j] : sum;  // a select, not a branch: the waits stay counted
                }
            }
        }
#pragma unroll
        for (int v = 0; v < P / 4; ++v) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = acc[4 * v + j];
            *reinterpret_cast<f32x4*>(out + q * K + c * P + 4 * v) = o;
        }
    }
}

}  // namespace
}  // namespace icrec

using namespace icrec;

extern "C" {

int icrec_compose_queries(icrec_index* h, const float* base_dev, const float* base_w_dev, int32_t n_queries,
                          const int32_t* term_off_dev, const int32_t* term_rows_dev, const float* term_w_dev,
                          int32_t max_terms, float* out_dev, void* stream) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    ICREC_REQUIRE(ix != nullptr, "icrec_compose_queries: NULL idx");
    ICREC_REQUIRE(term_off_dev != nullptr, "icrec_compose_queries: NULL term_off");
    ICREC_REQUIRE(out_dev != nullptr, "icrec_compose_queries: NULL out");
    ICREC_REQUIRE(max_terms >= 0 && max_terms <= ICREC_MAX_TERMS, "icrec_compose_queries: max_terms must be in [0, %d] (got %d)",
                  ICREC_MAX_TERMS, max_terms);
    ICREC_REQUIRE(term_rows_dev != nullptr || max_terms == 0, "icrec_compose_queries: NULL term_rows with max_terms > 0");
    ICREC_REQUIRE(n_queries >= 1, "icrec_compose_queries: n_queries must be >= 1 (got %d)", n_queries);
    ICREC_REQUIRE(base_dev != nullptr || max_terms > 0, "icrec_compose_queries: neither base nor terms (max_terms is 0)");
    ICREC_REQUIRE(base_w_dev == nullptr || base_dev != nullptr, "icrec_compose_queries: base_w without base");
    ICREC_HIP(hipSetDevice(ix->device));
    hipLaunchKernelGGL((rows_are_bf16(ix) ? compose_kernel<true> : compose_kernel<false>), dim3((unsigned)n_queries),
                       dim3(COMPOSE_THREADS), 0, (hipStream_t)stream, (const void*)ix->rows, ix->dim, ix->n_rows, base_dev,
                       base_w_dev, term_off_dev, term_rows_dev, term_w_dev, max_terms, out_dev);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
