// fuse.hip — weighted rank fusion of two ranked id lists on the device (icrec_fuse_select): "the content ranking and
// the co-occurrence ranking of the same catalog rows, merged by position".  One launch on the caller's stream:
//   fuse_select_kernel  one workgroup per query: both lists in LDS, liveness, the cross-list match, one sort, top_k
// The definition (live entries, effective weights, the fused score, the ordering rule) is in include/icrec.h;
// tests/fuse_reference.py states it in numpy.
#include "index.h"

namespace icrec {
namespace {

constexpr int FUSE_THREADS = 256;
constexpr int FUSE_SLOTS = 2 * ICREC_MAX_K;  // list A's entries, then list B's
static_assert(FUSE_SLOTS == FUSE_THREADS, "one thread per entry of the two lists");
constexpr uint32_t FUSE_DEAD = 0xFFFFFFFFu;  // no id: n_ids <= 2^32 - 1, so a real id is at most 2^32 - 2

// The position of `id` among slots [lo, hi) of `ids`, or -1.  Every thread of a wave reads the same address in the
// same step, so the LDS serves the scan by broadcast; a list holds a live id at most once.
__device__ __forceinline__ int fuse_find(const uint32_t* ids, int lo, int hi, uint32_t id) {
    int at = -1;
    for (int j = lo; j < hi; ++j)
        if (ids[j] == id) at = j - lo;
    return at;
}

// Slot i < ka is entry i of A, slot ka + j is entry j of B.  Three phases, a barrier between them:
//   1. pass[i] = the entry's id when it is in range, its gate is open and it is not excluded, else FUSE_DEAD;
//      eff[i] = the effective weight of the slot's position.
//   2. live[i] = pass[i] unless an earlier slot of the same list passes with the same id.
//   3. a live A entry looks its id up in B's live slots and owns the key make_key(eA + eB, id); a live B entry owns
//      the key only when A does not list the id alive.  Every other slot of the power-of-two network holds key 0.
// After the sort an output thread finds its id's two positions by the same look-up in `live`: the slot number is the
// position, so no position travels with the key.
__global__ __launch_bounds__(FUSE_THREADS) void fuse_select_kernel(
    const int64_t* __restrict__ a_idx, const int32_t* __restrict__ a_gate, int ka, const float* __restrict__ a_w,
    const int64_t* __restrict__ b_idx, const int32_t* __restrict__ b_gate, int kb, const float* __restrict__ b_w,
    int64_t n_ids, const int32_t* __restrict__ excl_idx, const int32_t* __restrict__ excl_off, int top_k,
    int64_t* __restrict__ out_idx, float* __restrict__ out_score, int32_t* __restrict__ out_pos) {
    __shared__ u64 keys[FUSE_SLOTS];
    __shared__ uint32_t pass[FUSE_SLOTS];
    __shared__ uint32_t live[FUSE_SLOTS];
    __shared__ float eff[FUSE_SLOTS];
    const int tid = threadIdx.x;
    const size_t q = blockIdx.x;
    const int n = ka + kb;
    int P = 64;
    while (P < n) P <<= 1;  // <= FUSE_SLOTS
    const bool in_a = tid < ka;
    const int j = in_a ? tid : tid - ka;  // the entry's position in its list
    if (tid < n) {
        const int64_t id = in_a ? a_idx[q * ka + j] : b_idx[q * kb + j];
        const int32_t* gate = in_a ? a_gate : b_gate;
        bool ok = id >= 0 && id < n_ids;
        if (ok && gate != nullptr) ok = gate[q * (in_a ? ka : kb) + j] > 0;
        if (ok && excl_off != nullptr && id <= 0x7FFFFFFFll) ok = !excluded(excl_idx, excl_off[q], excl_off[q + 1], (int)id);
        const float w = in_a ? a_w[j] : b_w[j];
        pass[tid] = ok ? (uint32_t)id : FUSE_DEAD;
        eff[tid] = w > 0.0f ? w : 0.0f;  // a NaN, a negative value and -0 count as +0
    }
    __syncthreads();
    const int lo = in_a ? 0 : ka;  // the slots of this entry's list
    if (tid < n) {
        const uint32_t id = pass[tid];
        bool first = id != FUSE_DEAD;
        for (int s = lo; s < tid; ++s) first = first && pass[s] != id;
        live[tid] = first ? id : FUSE_DEAD;
    }
    __syncthreads();
    u64 key = 0ull;
    if (tid < n && live[tid] != FUSE_DEAD) {
        const uint32_t id = live[tid];
        const int other = in_a ? fuse_find(live, ka, n, id) : fuse_find(live, 0, ka, id);
        if (in_a)
            key = make_key(__fadd_rn(eff[tid], other >= 0 ? eff[ka + other] : 0.0f), id);
        else if (other < 0)
            key = make_key(__fadd_rn(0.0f, eff[tid]), id);
    }
    if (tid < P) keys[tid] = key;
    __syncthreads();
    bitonic_sort_lds(keys, P, tid, FUSE_THREADS);
    if (tid < top_k) {
        const u64 k = tid < P ? keys[tid] : 0ull;
        const size_t o = q * top_k + tid;
        int pa = -1, pb = -1;
        if (k != 0ull && out_pos != nullptr) {
            pa = fuse_find(live, 0, ka, key_row(k));
            pb = fuse_find(live, ka, n, key_row(k));
        }
        out_idx[o] = k ? (int64_t)key_row(k) : -1;
        out_score[o] = k ? key_score(k) : 0.0f;
        if (out_pos != nullptr) {
            out_pos[2 * o] = pa;
            out_pos[2 * o + 1] = pb;
        }
    }
}

}  // namespace
}  // namespace icrec

using namespace icrec;

extern "C" {

int icrec_fuse_select(const int64_t* a_idx_dev, const int32_t* a_gate_dev, int32_t ka, const float* a_w_dev,
                      const int64_t* b_idx_dev, const int32_t* b_gate_dev, int32_t kb, const float* b_w_dev,
                      int32_t n_queries, int64_t n_ids, const int32_t* excl_idx_dev, const int32_t* excl_off_dev,
                      int32_t top_k, int64_t* out_idx_dev, float* out_score_dev, int32_t* out_pos_dev, int device,
                      void* stream) {
    ICREC_REQUIRE(a_idx_dev && a_w_dev && b_idx_dev && b_w_dev && out_idx_dev && out_score_dev,
                  "icrec_fuse_select: NULL argument");
    ICREC_REQUIRE((excl_idx_dev == nullptr) == (excl_off_dev == nullptr),
                  "icrec_fuse_select: excl_idx and excl_off must both be set or both NULL");
    ICREC_REQUIRE(n_queries >= 1, "icrec_fuse_select: n_queries must be >= 1 (got %d)", n_queries);
    ICREC_REQUIRE(ka >= 1 && ka <= ICREC_MAX_K && kb >= 1 && kb <= ICREC_MAX_K,
                  "icrec_fuse_select: ka and kb must be in [1, %d] (got %d and %d)", ICREC_MAX_K, ka, kb);
    ICREC_REQUIRE(top_k >= 1 && top_k <= ICREC_MAX_K, "icrec_fuse_select: top_k must be in [1, %d] (got %d)", ICREC_MAX_K,
                  top_k);
    ICREC_REQUIRE(n_ids >= 1 && n_ids <= 0xFFFFFFFFll, "icrec_fuse_select: n_ids must be in [1, 2^32 - 1] (got %lld)",
                  (long long)n_ids);
    ICREC_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fuse_select_kernel, dim3((unsigned)n_queries), dim3(FUSE_THREADS), 0, st, a_idx_dev, a_gate_dev, ka,
                       a_w_dev, b_idx_dev, b_gate_dev, kb, b_w_dev, n_ids, excl_idx_dev, excl_off_dev, top_k, out_idx_dev,
                       out_score_dev, out_pos_dev);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
