// metrics.hip — the reference's compute_ir_metrics (src/baselines/metrics.py:122-176) over ranked ROWS on the device:
// Accuracy@1/3/5/10, Recall@10, MRR@10, NDCG@10, MAP@100.  One wavefront per query finds the hit mask (a binary search
// of every ranked row in the query's sorted relevant rows); lane 0 then walks the mask in rank order in double, the
// order the reference's Python loops add in, so every per-query value has the reference's bits.  The means are left
// to the host: the device returns the eight sums over the counted queries and their number, reduced by one fixed tree.
#include <math.h>

#include "common.h"

namespace icrec {

constexpr int IR_VALUES = 8;  // per query: acc@1 acc@3 acc@5 acc@10 recall@10 rr@10 ndcg@10 ap@100
struct IrDiscounts {
    double d[10];  // 1 / log2(i + 2), from the host's libm: the device's log2 never enters
};

__device__ __forceinline__ bool ir_is_relevant(const int64_t* __restrict__ rel, int64_t lo, int64_t hi, int64_t row) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (rel[mid] < row) lo = mid + 1; else hi = mid;
    }
    return lo < end && rel[lo] == row;
}

// pq[q][0..8): the values; pq[q][8]: 1.0 when the query counts (a non-empty relevant set), else 0.0 and zeros
__global__ __launch_bounds__(256) void ir_query_kernel(const int64_t* __restrict__ ranked, int depth,
                                                       const int64_t* __restrict__ rel_off,
                                                       const int64_t* __restrict__ rel_rows, int Q, IrDiscounts disc,
                                                       double* __restrict__ pq, double* __restrict__ out_pq) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const int64_t rb = rel_off[q], re = rel_off[q + 1], nrel = re - rb;
    const int64_t* r = ranked + (size_t)q * depth;
    const int64_t row0 = lane < depth ? r[lane] : -1, row1 = lane + 64 < depth ? r[lane + 64] : -1;
    const u64 neg0 = __ballot(row0 < 0), neg1 = __ballot(row1 < 0);
    // the list ends at its first negative row (or at depth: the rows past it read as -1)
    const int n_valid = neg0 ? __ffsll((long long)neg0) - 1 : (neg1 ? 64 + __ffsll((long long)neg1) - 1 : 128);
    const bool hit0 = lane < n_valid && nrel > 0 && ir_is_relevant(rel_rows, rb, re, row0);
    const bool hit1 = lane + 64 < n_valid && nrel > 0 && ir_is_relevant(rel_rows, rb, re, row1);
    const u64 h0 = __ballot(hit0), h1 = __ballot(hit1);
    if (lane != 0) return;
    double v[IR_VALUES + 1];
    for (int i = 0; i <= IR_VALUES; ++i) v[i] = 0.0;
    if (nrel > 0) {
        v[IR_VALUES] = 1.0;
        v[0] = (h0 & 0x1ull) ? 1.0 : 0.0;
        v[1] = (h0 & 0x7ull) ? 1.0 : 0.0;
        v[2] = (h0 & 0x1Full) ? 1.0 : 0.0;
        v[3] = (h0 & 0x3FFull) ? 1.0 : 0.0;
        const u64 top10 = h0 & 0x3FFull;
        const int hits10 = __popcll(top10);
        v[4] = (double)hits10 / (double)nrel;
        if (top10) v[5] = 1.0 / (double)__ffsll((long long)top10);
        // NDCG@10 as the reference has it: the ideal is the top-10's OWN hits moved to the front
        double dcg = 0.0, idcg = 0.0;
        for (int i = 0; i < 10; ++i)
            if ((top10 >> i) & 1ull) dcg += disc.d[i];
        for (int i = 0; i < hits10; ++i) idcg += disc.d[i];
        if (idcg > 0.0) v[6] = dcg / idcg;
        // AP over the first min(100, valid) entries, divided by min(|relevant|, that cut)
        const int cut = n_valid < 100 ? n_valid : 100;
        double s = 0.0;
        int nh = 0;
        for (int j = 0; j < cut; ++j) {
            const bool hit = j < 64 ? (h0 >> j) & 1ull : (h1 >> (j - 64)) & 1ull;
            if (hit) {
                ++nh;
                s += (double)nh / (double)(j + 1);
            }
        }
        if (cut > 0) v[7] = s / (double)(nrel < cut ? nrel : (int64_t)cut);
    }
    for (int i = 0; i <= IR_VALUES; ++i) pq[(size_t)q * (IR_VALUES + 1) + i] = v[i];
    if (out_pq != nullptr)
        for (int i = 0; i < IR_VALUES; ++i) out_pq[(size_t)q * IR_VALUES + i] = v[i];
}

// sums[c] = sum over q of pq[q][c]: thread t adds q = t, t + 1024, ... in order, then a halving tree over the 1,024
// partial sums.  One workgroup, no atomics: the same bits on every run.
__global__ __launch_bounds__(1024) void ir_reduce_kernel(const double* __restrict__ pq, int Q, double* __restrict__ sums) {
    __shared__ double part[1024];
    const int t = threadIdx.x;
    for (int c = 0; c <= IR_VALUES; ++c) {
        double s = 0.0;
        for (int q = t; q < Q; q += 1024) s += pq[(size_t)q * (IR_VALUES + 1) + c];
        part[t] = s;
        __syncthreads();
        for (int w = 512; w >= 1; w >>= 1) {
            if (t < w) part[t] += part[t + w];
            __syncthreads();
        }
        if (t == 0) sums[c] = part[0];
        __syncthreads();
    }
}

}  // namespace icrec

using namespace icrec;

extern "C" {

size_t icrec_ir_metrics_workspace_bytes(int32_t n_queries) {
    return n_queries < 1 ? 0 : (size_t)n_queries * (IR_VALUES + 1) * sizeof(double);
}

int icrec_ir_metrics(const int64_t* ranked_rows_dev, int32_t depth, const int64_t* rel_off_dev, const int64_t* rel_rows_dev,
                     int32_t n_queries, double* out_sums_dev, double* out_per_query_dev, void* ws, size_t ws_bytes,
                     int device, void* stream) {
    ICREC_REQUIRE(ranked_rows_dev && rel_off_dev && out_sums_dev, "icrec_ir_metrics: NULL argument");
    ICREC_REQUIRE(n_queries >= 1, "icrec_ir_metrics: n_queries must be >= 1 (got %d)", n_queries);
    ICREC_REQUIRE(depth >= 1 && depth <= ICREC_MAX_K, "icrec_ir_metrics: depth must be in [1, %d] (got %d)", ICREC_MAX_K, depth);
    const size_t need = icrec_ir_metrics_workspace_bytes(n_queries);
    if (!ws || ws_bytes < need) {
        set_error("icrec_ir_metrics: workspace too small (%zu < %zu)", ws_bytes, need);
        return ICREC_ENOMEM;
    }
    IrDiscounts disc;
    for (int i = 0; i < 10; ++i) disc.d[i] = 1.0 / log2((double)(i + 2));
    ICREC_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    double* pq = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(ir_query_kernel, dim3((n_queries + 3) / 4), dim3(256), 0, st, ranked_rows_dev, depth, rel_off_dev,
                       rel_rows_dev, n_queries, disc, pq, out_per_query_dev);
    hipLaunchKernelGGL(ir_reduce_kernel, dim3(1), dim3(1024), 0, st, (const double*)pq, n_queries, out_sums_dev);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
