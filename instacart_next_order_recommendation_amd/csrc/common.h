// common.h — host-side error plumbing, the declarations of sort.hip's key sorters and prefix-sum launcher, and the
// device helpers shared by the gfx950 kernels: ranking keys (search.hip, sort.hip, cf.hip, boost.hip), the
// (value, position) key (mmr.hip, rerank.hip), the shard row rule (mmr.hip, boost.hip, rerank.hip, cap.hip), the LDS
// bitonic network, wave reductions, the workgroup scan (sort.hip, rerank.hip, comm.hip), the fp32 MFMA tile engine
// (search.hip) and the gathered exact-cosine wave tile (mmr.hip, boost.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/icrec.h"

namespace icrec {

void set_error(const char* fmt, ...);

#define ICREC_HIP(call)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            ::icrec::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                               __LINE__);                                                    \
            return ICREC_EHIP;                                                               \
        }                                                                                    \
    } while (0)

#define ICREC_REQUIRE(cond, ...)               \
    do {                                       \
        if (!(cond)) {                         \
            ::icrec::set_error(__VA_ARGS__);   \
            return ICREC_EINVAL;               \
        }                                      \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device function attribute: set it once per (kernel,
// device) under a lock (a second device in the same process, or two threads racing on the first launch, would
// otherwise launch with the 64 KB default and fail).  Uses the calling thread's current device.
int ensure_dynamic_lds(const void* kernel, int bytes);

// hipEvent-based per-kernel timing on the launch stream (bench.py's roofline leg).
struct TimingSlot {
    double total_ms = 0.0;
    int64_t n = 0;
};
enum { T_SEARCH_KERNEL = 0, T_FFN_UP = 1, T_ENCODE = 2, T_SEARCH = 3, T_SEARCH_FALLBACK = 4, T_MMR_GRAM = 5, T_MMR_SELECT = 6,
       T_BOOST_SCORE = 7, T_BOOST_SELECT = 8, T_FFN_UP_SMALL = 9 /* a spare of encoder.hip's */, T_IVF_SCAN = 10, T_CAP_SELECT = 11,
       T_INDEX_WRITE = 12, T_NSLOTS = 13 };
bool timing_on();
// Records [start, stop] around a launch when timing is enabled; resolved lazily at query time.
struct ScopedTimer {
    ScopedTimer(int slot, hipStream_t s) : slot(slot) { start(s); }
    explicit ScopedTimer(int slot) : slot(slot) {}  // idle (nothing recorded) unless start() is called later in its scope
    void start(hipStream_t s);
    ~ScopedTimer();
    int slot;
    hipStream_t stream = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
};

typedef unsigned long long u64;

// Workspace sections start on 256-byte boundaries.
static inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// sort.hip's sorters of packed 64-bit ranking keys (larger key = better hit, key 0 = pad), used by search.hip and cf.hip:
// the k-way merge of n_lists descending lists of k keys per query (keys[list][q_stride][k]; any of the three outputs
// may be NULL, out_score goes with out_idx; run_flag != NULL: nothing is written unless *run_flag != 0 when the kernel
// runs), its single-workgroup form for a few queries with few lists (false, and nothing launched, where that form does
// not apply), and the complete bitonic sort of keys[n_queries][P] in place followed by
// out[q][i] = row_offset + row of the i-th best key, -1 where that key is 0 (P = rank_pow2(n_rows)).
void launch_merge(const u64* keys, int n_lists, int q_stride, int Q, int k, int64_t* out_idx, float* out_score,
                  u64* out_keys, const int* run_flag, hipStream_t st);
bool launch_merge_block(const u64* keys, int n_lists, int q_stride, int Q, int k, int64_t* out_idx, float* out_score,
                        u64* out_keys, hipStream_t st);
int64_t rank_pow2(int64_t n);
void launch_rank_sort_emit(u64* keys, int64_t n_rows, int64_t P, int n_queries, int64_t row_offset, int64_t* out,
                           hipStream_t st);
constexpr int MERGE_MAX_LISTS = 1024;
// sort.hip's prefix sums, used by cf.hip and comm.hip: out[0 .. n] = the exclusive prefix sums of len[0 .. n) (int32,
// wrapping; the callers bound the total), and *max_out = max(0, the largest len) unless max_out is NULL.
void launch_prefix_sum(const int32_t* len, int64_t n, int32_t* out, int32_t* max_out, hipStream_t st);
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#ifdef __HIPCC__

// ------------------------------------------------------------------ ranking keys
// key = (orderable(score) << 32) | (0xFFFFFFFF - row): a larger key is a better hit under
// (score descending, row ascending).  key 0 is the "empty" pad (no real key is 0).
__device__ __forceinline__ u64 make_key(float s, uint32_t row) {
    uint32_t u = __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)u << 32) | (u64)(0xFFFFFFFFu - row);
}
__device__ __forceinline__ float key_score(u64 key) {
    uint32_t u = (uint32_t)(key >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ uint32_t key_row(u64 key) { return 0xFFFFFFFFu - (uint32_t)key; }
// Output slot o of a final list: the key and / or its (row, score); key 0 is the pad (row -1, score 0).
__device__ __forceinline__ void store_key(u64 key, size_t o, int64_t* out_idx, float* out_score, u64* out_keys) {
    if (out_keys) out_keys[o] = key;
    if (out_idx) out_idx[o] = key ? (int64_t)key_row(key) : -1;
    if (out_idx) out_score[o] = key ? key_score(key) : 0.0f;  // out_score is set whenever out_idx is
}

// The key of (value, position j) for a choice among one query's candidates: a larger key is ordered before, under "a
// number before a NaN, then the greater value compared as floats (-0 == +0), then the lower position".  A NaN's high
// word is 0, below every number's (-inf maps to 0x007FFFFF); v + 0.0f turns -0 into +0, after which make_key's map of
// the bits is strictly increasing over the numbers, -inf and +inf included; equal high words leave the order to the
// low word, which falls as j rises.  No real key is 0 (j <= ICREC_MAX_K - 1), so 0 stands for "not a candidate".
__device__ __forceinline__ u64 value_pos_key(float v, int j) {
    uint32_t u = 0u;
    if (v == v) {
        u = __float_as_uint(v + 0.0f);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((u64)u << 32) | (u64)(0xFFFFFFFFu - (uint32_t)j);
}

// Candidate c (a global row, or a negative pad) of an index shard: its local row, or -1 when it is a pad or lies
// outside [row_offset, row_offset + n_rows).
__device__ __forceinline__ int64_t local_row(int64_t c, int64_t row_offset, int64_t n_rows) {
    const int64_t r = c - row_offset;
    return (c >= 0 && r >= 0 && r < n_rows) ? r : -1;
}

// descending bitonic compare-exchange on a[i], a[i ^ j] inside the size-k subsequence containing i
__device__ __forceinline__ void bitonic_cx(u64& lo_slot, u64& hi_slot, bool desc) {
    const u64 a = lo_slot, b = hi_slot;
    const bool swap = desc ? (a < b) : (a > b);
    lo_slot = swap ? b : a;
    hi_slot = swap ? a : b;
}
// keys[0 .. n) in LDS, n a power of two, sorted descending by the whole bitonic network; every one of the workgroup's
// n_threads threads calls it after the barrier that published the keys, and it ends on a barrier.
__device__ __forceinline__ void bitonic_sort_lds(u64* keys, int n, int tid, int n_threads) {
    for (int size = 2; size <= n; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n / 2; i += n_threads) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));  // bit j clear; its partner has it set
                bitonic_cx(keys[lo], keys[lo | j], (lo & size) == 0);
            }
            __syncthreads();
        }
}

// bfloat16 -> fp32 is a 16-bit shift: the low / high half of a 32-bit word of bf16 bits, widened exactly
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl_xor(lo, m, 64);
    hi = __shfl_xor(hi, m, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_u64(u64 v, int src_lane) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl(lo, src_lane, 64);
    hi = __shfl(hi, src_lane, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        u64 o = shfl_xor_u64(v, m);
        v = o > v ? o : v;
    }
    return v;
}
// The fixed reduction order shared with oracle/icrec_oracle.c:wave_sum — butterfly xor 32..1.
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// ------------------------------------------------------------------ workgroup scan
// A workgroup of SCAN_THREADS threads walks i = 0 .. n-1 in chunks of SCAN_THREADS.  Thread t of a chunk takes
// v = load(i) and is handed emit(i, v, inc), inc = Op over load(0) .. load(i): an inclusive scan inside the wave by
// shuffles, the 16 wave totals through LDS, and the carry of the chunks before in a register of every thread (each
// thread folds all 16 totals into it, in wave order, so all threads hold the same carry).  For ScanSum the exclusive
// result is inc - v.  Sums wrap as int32 arithmetic does; the entry points bound them.
// The hazard: no thread may overwrite the wave totals of chunk c before every thread has read them.  Two barriers per
// chunk, and they suffice: the first stands between the reads of chunk c - 1 and the writes of chunk c, the second
// between those writes and the reads of chunk c; nothing else is shared.  The first barrier of the first chunk does
// the same for whatever used the LDS before, so a kernel may scan twice.  Every thread of the workgroup calls it.
constexpr int SCAN_THREADS = 1024;
struct ScanSum {
    static constexpr int identity = 0;
    static __device__ __forceinline__ int op(int a, int b) { return a + b; }
};
struct ScanMax {
    static constexpr int identity = INT32_MIN;
    static __device__ __forceinline__ int op(int a, int b) { return a > b ? a : b; }
};
template <class Op, class Load, class Emit>
__device__ __forceinline__ void workgroup_scan(int64_t n, Load load, Emit emit) {
    __shared__ int wave_tot[SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = Op::identity;
    for (int64_t i0 = 0; i0 < n; i0 += SCAN_THREADS) {
        const int64_t i = i0 + tid;
        const int v = i < n ? load(i) : Op::identity;
        int inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc = Op::op(o, inc);
        }
        __syncthreads();
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        int before = carry;
#pragma unroll
        for (int w = 0; w < SCAN_THREADS / 64; ++w) {
            if (w == wave) before = carry;
            carry = Op::op(carry, wave_tot[w]);
        }
        if (i < n) emit(i, v, Op::op(before, inc));
    }
}

// ------------------------------------------------------------------ fp32 MFMA tile engine
// C[BM x BN] = A[BM rows, K] . B[BN rows, K]^T with v_mfma_f32_32x32x2_f32.  Each output is the
// exact k-ascending chain acc = fmaf(a[k], b[k], acc) from acc = 0 (gfx950's f32 MFMA is a
// k-ordered fmaf chain with one rounding per product), so results are bit-identical to the
// oracle's loops.
//
// Both operands are row-major with K contiguous ("NT" GEMM).  K is walked in slabs of BK = 32
// floats = one 128-B line per row, staged global -> registers -> LDS.  In LDS each group of 8
// consecutive k is stored as [k0 k2 k4 k6 | k1 k3 k5 k7] so that one ds_read_b128 gives a lane
// the four values it feeds to four consecutive MFMA steps (lanes 0-31 supply the even k of a
// step, lanes 32-63 the odd k).  Row stride 36 floats keeps ds_read_b128 conflict-free.
constexpr int BK = 32;
constexpr int LDK = 36;

template <int WAVES_M_, int WAVES_N_, int TM_, int TN_>
struct TileCfg {
    static constexpr int WAVES_M = WAVES_M_, WAVES_N = WAVES_N_, TM = TM_, TN = TN_;
    static constexpr int BM = WAVES_M * TM * 32, BN = WAVES_N * TN * 32;
    static constexpr int THREADS = WAVES_M * WAVES_N * 64;
    static constexpr int A_CHUNKS = BM * 8 / THREADS;  // float4 chunks per thread per slab
    static constexpr int B_CHUNKS = BN * 8 / THREADS;
    static constexpr int LDS_FLOATS = (BM + BN) * LDK;
    static_assert(BM * 8 % THREADS == 0 && BN * 8 % THREADS == 0, "tile/threads mismatch");
};

// A16: operand A (the catalog rows in the search kernel) is stored as bfloat16; a thread's chunk is
// then 16 B = 8 consecutive k (half as many chunks), widened to fp32 when it is written to LDS.
template <class Cfg, bool A16 = false>
struct TileRegs {
    static constexpr int A_N = A16 ? (Cfg::A_CHUNKS + 1) / 2 : Cfg::A_CHUNKS;
    float4 a[A_N];
    float4 b[Cfg::B_CHUNKS];
};

// Issue the global loads of slab `slab` (rows clamped to the last valid row).
template <class Cfg, bool A16 = false>
__device__ __forceinline__ void tile_load(TileRegs<Cfg, A16>& r, const void* __restrict__ Av, int64_t a_row0,
                                          int64_t a_rows, const float* __restrict__ B, int64_t b_row0,
                                          int64_t b_rows, int K, int slab) {
    const int t = threadIdx.x;
    if (A16) {
        static_assert(!A16 || Cfg::BM * 4 % Cfg::THREADS == 0, "tile/threads mismatch (bf16 rows)");
        const uint16_t* A = static_cast<const uint16_t*>(Av);
#pragma unroll
        for (int i = 0; i < TileRegs<Cfg, A16>::A_N; ++i) {
            int id = t + Cfg::THREADS * i;
            int64_t row = a_row0 + (id >> 2);
            row = row < a_rows ? row : a_rows - 1;
            r.a[i] = *reinterpret_cast<const float4*>(A + row * K + slab * BK + (id & 3) * 8);  // raw bits
        }
    } else {
        const float* A = static_cast<const float*>(Av);
#pragma unroll
        for (int i = 0; i < TileRegs<Cfg, A16>::A_N; ++i) {
            int id = t + Cfg::THREADS * i;
            int64_t row = a_row0 + (id >> 3);
            row = row < a_rows ? row : a_rows - 1;
            r.a[i] = *reinterpret_cast<const float4*>(A + row * K + slab * BK + (id & 7) * 4);
        }
    }
#pragma unroll
    for (int i = 0; i < Cfg::B_CHUNKS; ++i) {
        int id = t + Cfg::THREADS * i;
        int64_t row = b_row0 + (id >> 3);
        row = row < b_rows ? row : b_rows - 1;
        r.b[i] = *reinterpret_cast<const float4*>(B + row * K + slab * BK + (id & 7) * 4);
    }
}

// Write the staged slab into LDS in the even/odd-split order.
template <class Cfg, bool A16 = false>
__device__ __forceinline__ void tile_store_lds(const TileRegs<Cfg, A16>& r, float* As, float* Bs) {
    const int t = threadIdx.x;
    if (A16) {
#pragma unroll
        for (int i = 0; i < TileRegs<Cfg, A16>::A_N; ++i) {
            int id = t + Cfg::THREADS * i;
            int row = id >> 2, c = id & 3;
            // word w holds k = 2w (low half) and k = 2w+1 (high half)
            const unsigned w0 = __float_as_uint(r.a[i].x), w1 = __float_as_uint(r.a[i].y),
                           w2 = __float_as_uint(r.a[i].z), w3 = __float_as_uint(r.a[i].w);
            float* p = As + row * LDK + c * 8;
            *reinterpret_cast<float4*>(p) = make_float4(bf16_lo(w0), bf16_lo(w1), bf16_lo(w2), bf16_lo(w3));
            *reinterpret_cast<float4*>(p + 4) = make_float4(bf16_hi(w0), bf16_hi(w1), bf16_hi(w2), bf16_hi(w3));
        }
    } else {
#pragma unroll
        for (int i = 0; i < TileRegs<Cfg, A16>::A_N; ++i) {
            int id = t + Cfg::THREADS * i;
            int row = id >> 3, c = id & 7;
            float* p = As + row * LDK + (c >> 1) * 8 + (c & 1) * 2;
            *reinterpret_cast<float2*>(p) = make_float2(r.a[i].x, r.a[i].z);      // even k
            *reinterpret_cast<float2*>(p + 4) = make_float2(r.a[i].y, r.a[i].w);  // odd k
        }
    }
#pragma unroll
    for (int i = 0; i < Cfg::B_CHUNKS; ++i) {
        int id = t + Cfg::THREADS * i;
        int row = id >> 3, c = id & 7;
        float* p = Bs + row * LDK + (c >> 1) * 8 + (c & 1) * 2;
        *reinterpret_cast<float2*>(p) = make_float2(r.b[i].x, r.b[i].z);
        *reinterpret_cast<float2*>(p + 4) = make_float2(r.b[i].y, r.b[i].w);
    }
}

// One slab of MFMAs for this wave's TM x TN block of 32x32 tiles.
template <class Cfg>
__device__ __forceinline__ void tile_mma(f32x16 (&acc)[Cfg::TM][Cfg::TN], const float* As, const float* Bs,
                                         int wm, int wn, int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
        float4 af[Cfg::TM], bf[Cfg::TN];
#pragma unroll
        for (int i = 0; i < Cfg::TM; ++i)
            af[i] = *reinterpret_cast<const float4*>(As + ((wm * Cfg::TM + i) * 32 + r) * LDK + kq * 8 + h * 4);
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j)
            bf[j] = *reinterpret_cast<const float4*>(Bs + ((wn * Cfg::TN + j) * 32 + r) * LDK + kq * 8 + h * 4);
#pragma unroll
        for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
            for (int j = 0; j < Cfg::TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
            }
    }
}

// Full K loop for one output tile: single LDS buffer, register prefetch of the next slab
// under the current slab's MFMAs.
template <class Cfg, bool A16 = false>
__device__ __forceinline__ void tile_gemm(f32x16 (&acc)[Cfg::TM][Cfg::TN], const void* __restrict__ A,
                                          int64_t a_row0, int64_t a_rows, const float* __restrict__ B,
                                          int64_t b_row0, int64_t b_rows, int K, float* As, float* Bs) {
    TileRegs<Cfg, A16> pre;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const int nslab = K / BK;
    tile_load<Cfg, A16>(pre, A, a_row0, a_rows, B, b_row0, b_rows, K, 0);
    for (int s = 0; s < nslab; ++s) {
        __syncthreads();  // previous slab's LDS reads are done
        tile_store_lds<Cfg, A16>(pre, As, Bs);
        __syncthreads();
        if (s + 1 < nslab) tile_load<Cfg, A16>(pre, A, a_row0, a_rows, B, b_row0, b_rows, K, s + 1);
        tile_mma<Cfg>(acc, As, Bs, wm, wn, lane);
    }
}

// ------------------------------------------------------------------ gathered exact-cosine wave tile
// One wave, one 32 x 32 tile: acc[.] += the chain s = fmaf(a[d], b[d], s) over d = 0 .. K-1 ascending (K a multiple
// of BK) between the row at pa (operand A: lane l gives the row of tile row l & 31) and the row at pb (operand B: the
// row of tile column l & 31), by v_mfma_f32_32x32x2_f32.  No row passes through LDS: per slab of BK values a lane
// reads the slab of each of its two rows straight from global memory in 16-byte loads (128 B of fp32, 64 B of bf16
// bits) and keeps the half that its sixteen MFMA steps consume - step s adds the products of d = 2s and 2s + 1 in
// that order, lanes 0-31 (h = 0) supply the even d and lanes 32-63 (h = 1) the odd d.  The half is chosen as each 16
// bytes arrive, between constant elements (a choice inside the step loop becomes a variable element index); bf16
// values are widened exactly.  The two halves of the wave read the same bytes, which the L1 serves once.
// A storage is float (fp32 values) or uint16_t (bf16 bits); mmr.hip gathers both operands from the index rows,
// boost.hip operand A, with the normalised fp32 query (one address for the whole wave) as operand B.
__device__ __forceinline__ void gathered_half_slab(const float* p, int h, float (&v)[BK / 2]) {
#pragma unroll
    for (int u = 0; u < BK / 4; ++u) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p + 4 * u);
        v[2 * u] = h ? x[1] : x[0];
        v[2 * u + 1] = h ? x[3] : x[2];
    }
}
__device__ __forceinline__ void gathered_half_slab(const uint16_t* p, int h, float (&v)[BK / 2]) {
#pragma unroll
    for (int u = 0; u < BK / 8; ++u) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(p + 8 * u);  // word w: d = 8u + 2w (low half), + 1 (high half)
#pragma unroll
        for (int w = 0; w < 4; ++w) v[4 * u + w] = h ? bf16_hi(x[w]) : bf16_lo(x[w]);
    }
}
template <class TA, class TB>
__device__ __forceinline__ void gathered_tile(f32x16& acc, const TA* __restrict__ pa, const TB* __restrict__ pb, int K,
                                              int h) {
    for (int d0 = 0; d0 < K; d0 += BK) {
        float a[BK / 2], b[BK / 2];
        gathered_half_slab(pa + d0, h, a);
        gathered_half_slab(pb + d0, h, b);
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    }
}

// Row of C held in acc[i][j][e] for this lane: (C/D map of the 32x32 f32 MFMA)
__device__ __forceinline__ int acc_row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }

// XCD-aware block remap: blocks b and b+8 share an XCD (round-robin dispatch), so give each
// XCD a contiguous range of logical ids.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int bid, int nblocks) {
    const int xcd = bid & 7, slot = bid >> 3;
    const int q = nblocks >> 3, r = nblocks & 7;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

#endif  // __HIPCC__

}  // namespace icrec
