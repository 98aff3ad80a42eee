// rerank.hip — the device steps around icrec_score_pairs: icrec_search's candidate rows -> packed
// `[CLS] query [SEP] product [SEP]` pairs (icrec_assemble_pairs), and the pairs' logits -> the best top_k candidates
// per query (icrec_rerank_select).  Neither needs an encoder or index handle; nothing here allocates or synchronises.
#include "common.h"

namespace icrec {
namespace {

constexpr int FILL_WAVES = 4;    // pairs per fill workgroup, one wave each
constexpr int SELECT_WAVES = 4;  // queries per select workgroup, one wave each
constexpr int SELECT_SLOTS = (ICREC_MAX_K + 63) / 64;

// ---------------------------------------------------------------- pair lengths
// One thread per pair p = q * k + j: the kept tokens (ka, kb) of the two sides under `longest_first` truncation to
// max_len ids, three of them special (model_io.truncate_pair's closed form: on an exact tie the FIRST side is the shorter
// one).  A candidate that is negative or outside [row_offset, row_offset + n_rows) keeps nothing of either side.
// len[p] = ka + kb + 3, seg_b[p] = ka + 2.
__global__ __launch_bounds__(256) void pair_len_kernel(const int32_t* __restrict__ q_cu, const int32_t* __restrict__ cat_cu,
                                                       int64_t n_rows, int64_t row_offset,
                                                       const int64_t* __restrict__ cand, int n_pairs, int k, int max_len,
                                                       int32_t* __restrict__ len, int32_t* __restrict__ seg_b) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    const int q = p / k;
    const int64_t r = local_row(cand[p], row_offset, n_rows);
    int ka = 0, kb = 0;
    if (r >= 0) {
        int la = q_cu[q + 1] - q_cu[q], lb = cat_cu[r + 1] - cat_cu[r];
        la = la < 0 ? 0 : la;
        lb = lb < 0 ? 0 : lb;
        const int budget = max_len - 3;
        if ((int64_t)la + lb <= budget) {
            ka = la;
            kb = lb;
        } else {
            const bool a_short = la <= lb;
            int sh = a_short ? la : lb, lg;
            if (2 * (int64_t)sh <= budget) {
                lg = budget - sh;
            } else {
                sh = budget / 2;
                lg = budget - sh;
            }
            ka = a_short ? sh : lg;
            kb = a_short ? lg : sh;
        }
    }
    len[p] = ka + kb + 3;
    seg_b[p] = ka + 2;
}

// ---------------------------------------------------------------- cu = exclusive prefix sum of the lengths
// One workgroup walks the pairs by common.h's workgroup_scan.  The sums fit an int32: the entry point refuses
// n_pairs * max_len >= 2^31.
// Safety clamp: pair p keeps its length only while every later pair still has room for three tokens, i.e. while
// S_end[p] + 3 * (n - 1 - p) <= ids_cap (S_end the inclusive sum).  The left side never decreases with p, so the pairs
// from the first failing one - pstar - on all shrink to `[CLS] [SEP] [SEP]`: cu[p] = cu[pstar] + 3 * (p - pstar), seg_b = 2.
// With ids_cap >= 3 * n (checked by the entry point) cu[n] <= ids_cap always.
__global__ __launch_bounds__(SCAN_THREADS) void pair_scan_kernel(const int32_t* __restrict__ len, int n, int64_t ids_cap,
                                                                 int32_t* __restrict__ cu, int32_t* __restrict__ seg_b) {
    __shared__ int total_s, pstar_s, base_s;
    const int tid = threadIdx.x;
    if (tid == 0) pstar_s = n;  // (the scan's barriers stand between this and the one thread that lowers it)
    workgroup_scan<ScanSum>(
        n, [&](int64_t p) { return len[p]; },
        [&](int64_t p, int v, int inc) {
            const int excl = inc - v;
            cu[p] = excl;
            const bool fits = (int64_t)excl + v + 3 * (n - 1 - p) <= ids_cap;
            const bool prev_fits = p == 0 || (int64_t)excl + 3 * (n - p) <= ids_cap;
            if (!fits && prev_fits) {  // exactly one thread: the predicate is monotone
                pstar_s = (int)p;
                base_s = excl;
            }
            if (p == n - 1) total_s = inc;
        });
    __syncthreads();
    const int pstar = pstar_s;
    if (pstar >= n) {
        if (tid == 0) cu[n] = total_s;
        return;
    }
    const int base = base_s;
    for (int p = pstar + tid; p <= n; p += SCAN_THREADS) {
        cu[p] = base + 3 * (p - pstar);
        if (p < n) seg_b[p] = 2;
    }
}

// ---------------------------------------------------------------- ids
// One wave per pair: lane l writes tokens l, l + 64, ... of the pair (4-byte loads from the two sides, 4-byte stores,
// both contiguous across the wave).  ka comes back from seg_b, kb from the pair's length in cu, so the truncation rule
// lives in pair_len_kernel alone (a pair the scan shrank has seg_b 2 and length 3: nothing of either side).
__global__ __launch_bounds__(FILL_WAVES * 64) void pair_fill_kernel(
    const int32_t* __restrict__ q_ids, const int32_t* __restrict__ q_cu, const int32_t* __restrict__ cat_ids,
    const int32_t* __restrict__ cat_cu, int64_t row_offset, const int64_t* __restrict__ cand, int n_pairs, int k,
    int cls_id, int sep_id, const int32_t* __restrict__ cu, const int32_t* __restrict__ seg_b, int32_t* __restrict__ ids_out,
    int64_t ids_cap) {
    const int p = blockIdx.x * FILL_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n_pairs) return;
    const int o = cu[p], n = cu[p + 1] - o;
    const int ka = seg_b[p] - 2, kb = n - 3 - ka;
    const int32_t* a = q_ids + q_cu[p / k];
    const int32_t* b = kb > 0 ? cat_ids + cat_cu[cand[p] - row_offset] : cat_ids;  // (kb > 0: the row was in range)
    for (int t = lane; t < n; t += 64) {
        int v;
        if (t == 0) v = cls_id;
        else if (t <= ka) v = a[t - 1];
        else if (t == ka + 1 || t == n - 1) v = sep_id;
        else v = b[t - ka - 2];
        if ((int64_t)o + t < ids_cap) ids_out[o + t] = v;
    }
}

// ---------------------------------------------------------------- best top_k of k by logit
// One wave per query; lane l owns candidates l and l + 64.  A candidate's rank is the number of candidates ordered
// before it: idx >= 0 before idx < 0 (skipped), then a number before a NaN, then the larger logit (compared as floats:
// -0 == +0, as numpy's stable argsort of the negated scores compares them), then the lower position j.
// Candidate (la, ja) is ordered before (lb, jb) exactly when value_pos_key(la, ja) > value_pos_key(lb, jb) (common.h):
//   one NaN         the NaN's high word is 0, a number's at least 0x007FFFFF: the number's key is greater;
//   two NaNs        both high words are 0 whatever the payloads: the low word decides, greater for the lower j;
//   -0 and +0       v + 0.0f is +0 for both, the high words are equal: the lower j, as for la == lb;
//   +-inf           -inf maps to 0x007FFFFF, below every finite number, +inf to 0xFF800000, above: la > lb as floats;
//   two numbers     the map of the bits is strictly increasing, so la > lb gives the greater high word, and equal
//                   values (two positions of one logit) equal high words and again the lower j;
//   itself          equal keys: not before, as ja < jb is false.
// A skipped candidate's key is 0, which is greater than no key.
__global__ __launch_bounds__(SELECT_WAVES * 64) void rerank_select_kernel(const float* __restrict__ logits,
                                                                          const int64_t* __restrict__ cand, int n_queries,
                                                                          int k, int top_k, int64_t* __restrict__ out_idx,
                                                                          float* __restrict__ out_logit) {
    const int q = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= n_queries) return;  // (whole waves leave: the shuffles below always see 64 lanes)
    float lg[SELECT_SLOTS];
    int64_t ix[SELECT_SLOTS];
    u64 key[SELECT_SLOTS];
    int rank[SELECT_SLOTS];
#pragma unroll
    for (int s = 0; s < SELECT_SLOTS; ++s) {
        const int j = s * 64 + lane;
        lg[s] = j < k ? logits[(size_t)q * k + j] : 0.0f;
        ix[s] = j < k ? cand[(size_t)q * k + j] : -1;
        key[s] = ix[s] >= 0 ? value_pos_key(lg[s], j) : 0ull;
        rank[s] = 0;
    }
    int n_valid = 0;
#pragma unroll
    for (int so = 0; so < SELECT_SLOTS; ++so) {
        for (int lo = 0; lo < 64 && so * 64 + lo < k; ++lo) {  // wave-uniform bounds
            const u64 ok = shfl_u64(key[so], lo);
            if (ok == 0ull) continue;
            ++n_valid;
#pragma unroll
            for (int s = 0; s < SELECT_SLOTS; ++s) rank[s] += ok > key[s] ? 1 : 0;
        }
    }
#pragma unroll
    for (int s = 0; s < SELECT_SLOTS; ++s) {
        if (ix[s] >= 0 && rank[s] < top_k) {
            out_idx[(size_t)q * top_k + rank[s]] = ix[s];
            out_logit[(size_t)q * top_k + rank[s]] = lg[s];
        }
        const int r = s * 64 + lane;  // the slots no candidate took
        if (r >= n_valid && r < top_k) {
            out_idx[(size_t)q * top_k + r] = -1;
            out_logit[(size_t)q * top_k + r] = 0.0f;
        }
    }
}

bool pair_count_ok(int32_t n_queries, int32_t k, int32_t max_len) {
    return n_queries >= 1 && k >= 1 && max_len >= 3 && (int64_t)n_queries * k * max_len < (1ll << 31);
}

}  // namespace
}  // namespace icrec

using namespace icrec;

extern "C" {

size_t icrec_assemble_pairs_workspace_bytes(int32_t n_queries, int32_t k) {
    if (n_queries < 1 || k < 1 || k > ICREC_MAX_K) return 0;
    return align256((size_t)n_queries * k * sizeof(int32_t));
}

int icrec_assemble_pairs(const int32_t* q_ids_dev, const int32_t* q_cu_dev, int32_t n_queries, const int32_t* cat_ids_dev,
                         const int32_t* cat_cu_dev, int64_t n_rows, int64_t row_offset, const int64_t* cand_idx_dev,
                         int32_t k, int32_t max_len, int32_t cls_id, int32_t sep_id, int32_t* ids_out_dev, int64_t ids_cap,
                         int32_t* cu_out_dev, int32_t* seg_b_out_dev, void* ws, size_t ws_bytes, int device, void* stream) {
    ICREC_REQUIRE(q_ids_dev && q_cu_dev && cat_ids_dev && cat_cu_dev && cand_idx_dev && ids_out_dev && cu_out_dev &&
                      seg_b_out_dev && ws,
                  "icrec_assemble_pairs: NULL argument");
    ICREC_REQUIRE(n_queries >= 1, "icrec_assemble_pairs: n_queries must be >= 1 (got %d)", n_queries);
    ICREC_REQUIRE(k >= 1 && k <= ICREC_MAX_K, "icrec_assemble_pairs: k must be in [1, %d] (got %d)", ICREC_MAX_K, k);
    ICREC_REQUIRE(max_len >= 3 && max_len <= ICREC_MAX_SEQLEN, "icrec_assemble_pairs: max_len must be in [3, %d] (got %d)",
                  ICREC_MAX_SEQLEN, max_len);
    ICREC_REQUIRE(pair_count_ok(n_queries, k, max_len),
                  "icrec_assemble_pairs: %d x %d pairs of up to %d tokens overflow an int32 prefix sum", n_queries, k, max_len);
    ICREC_REQUIRE(n_rows >= 0, "icrec_assemble_pairs: n_rows must be >= 0");
    const int n_pairs = n_queries * k;
    ICREC_REQUIRE(ids_cap >= 3 * (int64_t)n_pairs, "icrec_assemble_pairs: ids_cap %lld holds fewer than 3 tokens for each of %d pairs",
                  (long long)ids_cap, n_pairs);
    const size_t need = icrec_assemble_pairs_workspace_bytes(n_queries, k);
    if (ws_bytes < need) {
        set_error("icrec_assemble_pairs: workspace too small (%zu < %zu)", ws_bytes, need);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    int32_t* len = static_cast<int32_t*>(ws);
    hipLaunchKernelGGL(pair_len_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, q_cu_dev, cat_cu_dev, n_rows,
                       row_offset, cand_idx_dev, n_pairs, k, max_len, len, seg_b_out_dev);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, len, n_pairs, ids_cap, cu_out_dev, seg_b_out_dev);
    hipLaunchKernelGGL(pair_fill_kernel, dim3((unsigned)((n_pairs + FILL_WAVES - 1) / FILL_WAVES)), dim3(FILL_WAVES * 64), 0, st,
                       q_ids_dev, q_cu_dev, cat_ids_dev, cat_cu_dev, row_offset, cand_idx_dev, n_pairs, k, cls_id, sep_id,
                       cu_out_dev, seg_b_out_dev, ids_out_dev, ids_cap);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

int icrec_rerank_select(const float* logits_dev, const int64_t* cand_idx_dev, const float* cand_score_dev, int32_t n_queries,
                        int32_t k, int32_t top_k, int64_t* out_idx_dev, float* out_logit_dev, int device, void* stream) {
    (void)cand_score_dev;  // the retrieval order is the position j: the cosine scores are not read
    ICREC_REQUIRE(logits_dev && cand_idx_dev && out_idx_dev && out_logit_dev, "icrec_rerank_select: NULL argument");
    ICREC_REQUIRE(n_queries >= 1, "icrec_rerank_select: n_queries must be >= 1 (got %d)", n_queries);
    ICREC_REQUIRE(k >= 1 && k <= ICREC_MAX_K, "icrec_rerank_select: k must be in [1, %d] (got %d)", ICREC_MAX_K, k);
    ICREC_REQUIRE(top_k >= 1 && top_k <= k, "icrec_rerank_select: top_k must be in [1, k = %d] (got %d)", k, top_k);
    ICREC_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(rerank_select_kernel, dim3((unsigned)((n_queries + SELECT_WAVES - 1) / SELECT_WAVES)),
                       dim3(SELECT_WAVES * 64), 0, (hipStream_t)stream, logits_dev, cand_idx_dev, n_queries, k, top_k,
                       out_idx_dev, out_logit_dev);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
