// sort.hip — the sorters of packed 64-bit ranking keys (common.h: make_key; a larger key is a better hit, key 0 is
// the pad), declared in common.h for search.hip and cf.hip: the k-way merge of sorted partial lists (a wave tournament,
// or one workgroup for a single request's few lists) and the complete bitonic sort behind the full rankings; and the
// one-workgroup prefix sums of int32 counts, declared in common.h for cf.hip (CSR offsets and the longest segment) and
// comm.hip (a shard's exclusion CSR).
// Entry points: icrec_merge_topk, icrec_rank_all.
#include "index.h"

namespace icrec {

// ---------------------------------------------------------------- k-way merge of sorted lists
// keys: [n_lists][q_stride][k] sorted descending per (list, query); one wavefront per query
// runs a tournament: every lane holds the heads of up to MERGE_LPL lists.
template <int MERGE_LPL>  // lists per lane: 4 (<= 256 lists) or 16 (<= 1024)
__global__ __launch_bounds__(256) void merge_kernel(const u64* __restrict__ keys, int n_lists, int q_stride, int Q,
                                                    int k, int64_t* __restrict__ out_idx,
                                                    float* __restrict__ out_score, u64* __restrict__ out_keys,
                                                    const int* __restrict__ run_flag = nullptr) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    if (run_flag != nullptr && *run_flag == 0) return;
    u64 head[MERGE_LPL];
    int pos[MERGE_LPL];
#pragma unroll
    for (int s = 0; s < MERGE_LPL; ++s) {
        const int c = lane + 64 * s;
        pos[s] = 0;
        head[s] = c < n_lists ? keys[((size_t)c * q_stride + q) * k] : 0ull;
    }
    for (int e = 0; e < k; ++e) {
        u64 best = 0ull;
#pragma unroll
        for (int s = 0; s < MERGE_LPL; ++s) best = head[s] > best ? head[s] : best;
        const u64 w = wave_max_u64(best);
        if (w != 0ull) {
#pragma unroll
            for (int s = 0; s < MERGE_LPL; ++s) {
                if (head[s] == w) {  // keys are unique: exactly one (lane, s) advances
                    const int c = lane + 64 * s;
                    ++pos[s];
                    head[s] = pos[s] < k ? keys[((size_t)c * q_stride + q) * k + pos[s]] : 0ull;
                }
            }
        }
        if (lane == 0) store_key(w, (size_t)q * k + e, out_idx, out_score, out_keys);
    }
}

// Few queries, few lists (a single request: ~200 partial lists of k): ONE global round trip and three short LDS passes
// instead of k dependent rounds (merge_kernel's every round waits for a global load behind a 12-shuffle wave maximum:
// 12 us of a 0.35 ms request at 195 lists x 20).  A 256-thread workgroup per query:
//   1. all n_lists * k keys (<= MERGE_BLOCK_KEYS) -> LDS, coalesced;
//   2. h = the k-th largest list HEAD (rank by counting over the <= 256 heads): at least k keys are >= h, so the k
//      best keys are all >= h, and only lists whose head is >= h (at most k of them) hold any;
//   3. those lists hand their keys >= h to a candidate array (they are sorted: stop at the first smaller one);
//   4. every candidate's rank by counting; rank r < k goes to output r.  Keys are unique (score bits | row) and 0 is
//      the empty pad, so ranks are exact: the same (score desc, row asc) order and outputs as merge_kernel.
constexpr int MERGE_BLOCK_KEYS = 16 * 256;
__global__ __launch_bounds__(256) void merge_block_kernel(const u64* __restrict__ keys, int n_lists, int q_stride, int Q,
                                                          int k, int64_t* __restrict__ out_idx,
                                                          float* __restrict__ out_score, u64* __restrict__ out_keys) {
    __shared__ __attribute__((aligned(16))) u64 all[MERGE_BLOCK_KEYS];
    __shared__ uint16_t cand[MERGE_BLOCK_KEYS];  // candidates as indices into `all`
    __shared__ u64 h_s;
    __shared__ int ncand;
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int n_keys = n_lists * k;
    if (tid == 0) { h_s = 0ull; ncand = 0; }
#pragma unroll
    for (int s = 0; s < MERGE_BLOCK_KEYS / 256; ++s) {
        const int f = tid + 256 * s;
        if (f < n_keys) {
            const int c = f / k, e = f - c * k;
            all[f] = keys[((size_t)c * q_stride + q) * k + e];
        }
    }
    __syncthreads();
    const u64 head = tid < n_lists ? all[tid * k] : 0ull;
    if (head != 0ull) {
        int r = 0;
        for (int i = 0; i < n_lists; ++i) r += all[i * k] > head ? 1 : 0;  // LDS broadcast reads
        if (r == k - 1) h_s = head;  // unique keys: at most one thread
    }
    __syncthreads();
    const u64 h = h_s;  // 0 when fewer than k lists are non-empty: every key is a candidate
    if (head != 0ull && head >= h) {
        for (int e = 0; e < k; ++e) {
            const u64 v = all[tid * k + e];
            if (v == 0ull || v < h) break;
            cand[atomicAdd(&ncand, 1)] = (uint16_t)(tid * k + e);
        }
    }
    __syncthreads();
    const int C = ncand;
    for (int ci = tid; ci < C; ci += 256) {
        const u64 v = all[cand[ci]];
        int r = 0;
        for (int j = 0; j < C; ++j) r += all[cand[j]] > v ? 1 : 0;
        if (r < k) store_key(v, (size_t)q * k + r, out_idx, out_score, out_keys);
    }
    for (int e = (C < k ? C : k) + tid; e < k; e += 256)  // pads: fewer than k rows left after the exclusions
        store_key(0ull, (size_t)q * k + e, out_idx, out_score, out_keys);
}

// k-way merge of n_lists sorted lists of k keys per query (keys[list][q_stride][k]): 4 lists per lane up to 256 lists
void launch_merge(const u64* keys, int n_lists, int q_stride, int Q, int k, int64_t* out_idx, float* out_score,
                  u64* out_keys, const int* run_flag, hipStream_t st) {
    hipLaunchKernelGGL((n_lists <= 256 ? merge_kernel<4> : merge_kernel<16>), dim3((Q + 3) / 4), dim3(256), 0, st, keys,
                       n_lists, q_stride, Q, k, out_idx, out_score, out_keys, run_flag);
}

// The same merge by merge_block_kernel where it applies; false (nothing launched): the caller takes launch_merge.
bool launch_merge_block(const u64* keys, int n_lists, int q_stride, int Q, int k, int64_t* out_idx, float* out_score,
                        u64* out_keys, hipStream_t st) {
    if (!(Q <= 4 && n_lists <= 256 && (int64_t)n_lists * k <= MERGE_BLOCK_KEYS)) return false;
    hipLaunchKernelGGL(merge_block_kernel, dim3(Q), dim3(256), 0, st, keys, n_lists, q_stride, Q, k, out_idx, out_score,
                       out_keys);
    return true;
}

// ---------------------------------------------------------------- full ranking (offline evaluation consumers)
// The reference's ContentBasedBaseline.rank_all / compare_untrained_vs_trained (src/baselines/content_based.py:58-63,
// scripts/compare_untrained_vs_trained.py:74-85) argsort every score row completely.  One workgroup per query sorts the
// packed keys (orderable(score) << 32 | ~row: the search kernels' total order, score descending then row ascending)
// with a bitonic network: P = next power of two >= n_rows keys per query in global scratch (pads = key 0, which sorts
// last), stages with partner distance < 4,096 run on an 8,192-key segment in LDS, the rest in global memory.
constexpr int RANK_SEG = 8192;  // keys per LDS segment (64 KB)
__global__ __launch_bounds__(1024) void rank_keys_kernel(const float* __restrict__ scores, int64_t n_rows, int64_t P,
                                                         u64* __restrict__ keys) {
    const int64_t qi = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 1024)
        keys[qi * P + i] = i < n_rows ? make_key(scores[qi * n_rows + i], (uint32_t)i) : 0ull;
}

__global__ __launch_bounds__(1024) void rank_sort_kernel(u64* __restrict__ keys, int64_t P) {
    __shared__ u64 seg[RANK_SEG];
    u64* const a = keys + (int64_t)blockIdx.x * P;
    const int t = threadIdx.x;
    const int64_t seg_len = P < RANK_SEG ? P : RANK_SEG, nseg = P / seg_len;
    // the stages j = j_hi, j_hi/2, ..., 1 of size-k merges, for one segment held in LDS (partners stay inside it)
    auto local_stages = [&](int64_t base, int64_t k_lo, int64_t k_hi, int64_t j_cap) {
        for (int64_t i = t; i < seg_len; i += 1024) seg[i] = a[base + i];
        __syncthreads();
        for (int64_t k = k_lo; k <= k_hi; k <<= 1)
            for (int64_t j = (k >> 1) < j_cap ? (k >> 1) : j_cap; j >= 1; j >>= 1) {
                for (int64_t p = t; p < seg_len / 2; p += 1024) {
                    const int64_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    u64 x = seg[i], y = seg[i | j];
                    bitonic_cx(x, y, ((base + i) & k) == 0);
                    seg[i] = x;
                    seg[i | j] = y;
                }
                __syncthreads();
            }
        for (int64_t i = t; i < seg_len; i += 1024) a[base + i] = seg[i];
        __syncthreads();
    };
    for (int64_t sidx = 0; sidx < nseg; ++sidx) local_stages(sidx * seg_len, 2, seg_len, seg_len / 2);  // k <= seg_len
    for (int64_t k = seg_len * 2; k <= P; k <<= 1) {
        for (int64_t j = k >> 1; j >= seg_len; j >>= 1) {  // partners in different segments: global memory
            for (int64_t p = t; p < P / 2; p += 1024) {
                const int64_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                u64 x = a[i], y = a[i | j];
                bitonic_cx(x, y, (i & k) == 0);
                a[i] = x;
                a[i | j] = y;
            }
            __syncthreads();  // one workgroup owns the row; the barrier orders its global writes for its own reads
        }
        for (int64_t sidx = 0; sidx < nseg; ++sidx) local_stages(sidx * seg_len, k, k, seg_len / 2);
    }
}

__global__ __launch_bounds__(256) void rank_emit_kernel(const u64* __restrict__ keys, int64_t n_rows, int64_t P,
                                                        int64_t row_offset, int64_t* __restrict__ out) {
    const int64_t qi = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * 256) {
        const u64 key = keys[qi * P + i];  // key 0: a pad that sorted into the first n_rows (cf.hip's left-out rows)
        out[qi * n_rows + i] = key ? row_offset + (int64_t)key_row(key) : -1;
    }
}

int64_t rank_pow2(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// keys[n_queries][P] (P = rank_pow2(n_rows), pads = key 0) -> sorted descending in place -> out[n_queries][n_rows]
void launch_rank_sort_emit(u64* keys, int64_t n_rows, int64_t P, int n_queries, int64_t row_offset, int64_t* out,
                           hipStream_t st) {
    const unsigned gx = (unsigned)((P + 1023) / 1024 < 64 ? (P + 1023) / 1024 : 64);
    hipLaunchKernelGGL(rank_sort_kernel, dim3(n_queries), dim3(1024), 0, st, keys, P);
    hipLaunchKernelGGL(rank_emit_kernel, dim3(gx * 4, n_queries), dim3(256), 0, st, (const u64*)keys, n_rows, P, row_offset, out);
}

// ---------------------------------------------------------------- prefix sums (cf.hip's CSR offsets, comm.hip's)
// out[0 .. n] = the exclusive prefix sums of len[0 .. n), *max_out = max(0, the largest len): one workgroup on
// common.h's workgroup_scan.  A thread keeps the maximum of what it loaded; the workgroup's maximum is the last
// thread's result of a second, one-chunk scan over those.
__global__ __launch_bounds__(SCAN_THREADS) void prefix_sum_kernel(const int32_t* __restrict__ len, int64_t n,
                                                                  int32_t* __restrict__ out, int32_t* __restrict__ max_out) {
    int m = 0;
    if (n == 0 && threadIdx.x == 0) out[0] = 0;
    workgroup_scan<ScanSum>(
        n,
        [&](int64_t i) {
            const int v = len[i];
            m = v > m ? v : m;
            return v;
        },
        [&](int64_t i, int v, int inc) {
            out[i] = inc - v;
            if (i == n - 1) out[n] = inc;
        });
    if (max_out != nullptr)
        workgroup_scan<ScanMax>(
            SCAN_THREADS, [&](int64_t) { return m; },
            [&](int64_t t, int, int running_max) {
                if (t == SCAN_THREADS - 1) *max_out = running_max;
            });
}

void launch_prefix_sum(const int32_t* len, int64_t n, int32_t* out, int32_t* max_out, hipStream_t st) {
    hipLaunchKernelGGL(prefix_sum_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, len, n, out, max_out);
}

}  // namespace icrec

using namespace icrec;

extern "C" {

size_t icrec_rank_all_workspace_bytes(const icrec_index* h, int32_t n_queries) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    if (!ix || n_queries < 1) return 0;
    const size_t sw = icrec_search_workspace_bytes(h, n_queries, 1);
    if (sw == 0) return 0;
    return align256((size_t)n_queries * ix->n_rows * 4) + align256((size_t)n_queries * rank_pow2(ix->n_rows) * 8) + align256(sw);
}

int icrec_rank_all(icrec_index* h, const float* q_dev, int32_t n_queries, int64_t* out_rows_dev, void* ws,
                   size_t ws_bytes, void* stream) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix && q_dev && out_rows_dev && n_queries >= 1, "icrec_rank_all: bad argument");
    const size_t need = icrec_rank_all_workspace_bytes(h, n_queries);
    if (!ws || ws_bytes < need || need == 0) {
        set_error("icrec_rank_all: workspace too small (%zu < %zu)", ws_bytes, need);
        return ICREC_ENOMEM;
    }
    const int64_t P = rank_pow2(ix->n_rows);
    char* base = reinterpret_cast<char*>(ws);
    float* scores = reinterpret_cast<float*>(base);
    u64* keys = reinterpret_cast<u64*>(base + align256((size_t)n_queries * ix->n_rows * 4));
    char* sws = reinterpret_cast<char*>(keys) + align256((size_t)n_queries * P * 8);
    if (int rc = icrec_scores(h, q_dev, n_queries, scores, sws, ws_bytes - (size_t)(sws - base), stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned gx = (unsigned)((P + 1023) / 1024 < 64 ? (P + 1023) / 1024 : 64);
    hipLaunchKernelGGL(rank_keys_kernel, dim3(gx, n_queries), dim3(1024), 0, st, scores, ix->n_rows, P, keys);
    launch_rank_sort_emit(keys, ix->n_rows, P, n_queries, ix->row_offset, out_rows_dev, st);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

int icrec_merge_topk(const uint64_t* keys_dev, int32_t n_lists, int32_t n_queries, int32_t k, int64_t* out_idx_dev,
                     float* out_score_dev, int device, void* stream) {
    ICREC_REQUIRE(keys_dev && out_idx_dev && out_score_dev, "icrec_merge_topk: NULL argument");
    ICREC_REQUIRE(n_lists >= 1 && n_lists <= MERGE_MAX_LISTS, "icrec_merge_topk: n_lists must be in [1, %d]", MERGE_MAX_LISTS);
    ICREC_REQUIRE(n_queries >= 1 && k >= 1 && k <= ICREC_MAX_K, "icrec_merge_topk: bad n_queries/k");
    ICREC_HIP(hipSetDevice(device));
    launch_merge(reinterpret_cast<const u64*>(keys_dev), n_lists, n_queries, n_queries, k, out_idx_dev, out_score_dev,
                 nullptr, nullptr, (hipStream_t)stream);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
