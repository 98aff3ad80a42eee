// adapt.hip — a query-side linear adapter learned from (context, product) pairs against the rows the index holds
// (icrec_adapter_*).  The encoder and the stored rows stay frozen; only q' = q + D q changes, so every search composes.
//   apply_kernel    one launch: a workgroup keeps a tile of queries in LDS, a lane owns one output's chain over c
//   forward_kernel  the step's (a): z = apply(a), n = max(|z|, 1e-12), u = z / n
//   the step's (b)  S^T = V U^T on the f32 MFMA over gathered stored rows, in two sweeps over the rows: each anchor's
//                   (maximum, sum), then P recomputed, G = (P - [positive]) / counted and dU^T = V^T G; then dz and one
//                   loss per anchor.  It has two forms, which differ in where a tile row's stored row comes from - a
//                   ROW SOURCE, ListRows or SpanRows - and share everything written over one: score_tile, store_g,
//                   add_group (sweep 2's accumulation, the unit's register budget), merge_halves / merge_waves of
//                   (maximum, sum), for_owned_tiles, row_in_range
//     logits_kernel   the list step (icrec_adapter_step), over ListRows: one workgroup per 32 anchors does both
//                     sweeps over the candidate list and the epilogue
//     catalog_*       the step against the WHOLE catalog (icrec_adapter_step_catalog), over SpanRows: (anchor tiles x
//                     row splits) workgroups - catalog_max_sum_kernel is sweep 1, catalog_merge_kernel the ordered
//                     merge of the splits, catalog_du_kernel sweep 2, catalog_finish_kernel the epilogue
//                   The two sweep 1s and the two epilogues are NOT shared: their sums have different orders, each stated
//                   where it stands
//   grad_kernel     the step's (c): one wave per 32 x 32 tile of dD = dZ^T A, walking the batch in order, AdamW in its
//                   epilogue; one more workgroup sums the anchors' losses: each block of GRAD_BLOCK = 64 anchors is
//                   one chain from zero in index order, the blocks' sums are added in block order - the order of
//                   every other sum of this unit - both levels in double, then the division by the counted anchors
//                   and the mean's one rounding to float32 (as one float32 chain the B = 1,024 losses measured 3.26x
//                   the float32 reference's error at width 32, beside a margin of 2; in two float32 levels a batch
//                   of 65 still measured 6.29x beside a margin of 6: a chain of 64 rounds at the sum's ulp 64 times
//                   and the mean is compared at half of ITS ulp)
//   lists_*         the step over PER-ANCHOR lists with graded targets (icrec_adapter_step_lists): no shared rows, so no
//                   MFMA tile - lists_plan_kernel (the anchors' target sums and flag rows) and lists_kernel (a workgroup
//                   per anchor: two gathered sweeps over its own entries) stand where (b) does
// On the host every step entry runs check_step, launch_forward, its own middle, launch_grad.
// The definitions (the two roundings of apply, the masking rules, the gradient, torch's AdamW) are in include/icrec.h;
// tests/adapter_reference.py states them in numpy and torch.  No floating-point atomics anywhere: every sum has one order.
#include <math.h>

#include <vector>

#include "index.h"

namespace icrec {

struct Adapter {
    float* delta = nullptr;    // [dim][dim] row-major
    float* delta_t = nullptr;  // its transpose: apply's lane r reads delta_t[c][r], coalesced
    float* m = nullptr;        // AdamW's first and second moments
    float* v = nullptr;
    int dim = 0;
    int device = 0;
    int64_t t = 0;             // AdamW steps taken
};

namespace {

constexpr int APPLY_THREADS = 64;  // apply_kernel: one wave, a lane per output
constexpr int APPLY_TILE = 8;      // queries of its tile: each element of D is read once per tile
constexpr int FWD_THREADS = 256;
constexpr int FWD_TILE = 4;        // anchors of a forward workgroup: one per wave for the norms
constexpr int LOGIT_THREADS = 256;
constexpr int LOGIT_WAVES = LOGIT_THREADS / 64;
constexpr int ANCHOR_TILE = 32;
constexpr int GRAD_DEPTH = 8;      // MFMA steps (two anchors each) whose operands grad_kernel loads at once
constexpr int GRAD_BLOCK = 64;     // anchors of one chain of grad_kernel: the sum over the batch has two short levels
static_assert(GRAD_BLOCK % (2 * GRAD_DEPTH) == 0, "a block of anchors is whole groups of steps");
constexpr int MAX_OWN_TILES = ICREC_ADAPTER_MAX_DIM / 32 / LOGIT_WAVES;  // feature tiles of dU^T a wave accumulates
static_assert(ICREC_ADAPTER_MAX_DIM % (32 * LOGIT_WAVES) == 0, "the feature tiles are dealt to the waves");
static_assert(ICREC_ADAPTER_MAX_CANDIDATES * sizeof(int32_t) <= 32768, "a step's checked candidate rows are staged in LDS");
static_assert(ICREC_ADAPTER_MAX_BATCH * sizeof(float) <= 4096, "the anchors' losses are staged in LDS");
constexpr int LOSS_BLOCKS = (ICREC_ADAPTER_MAX_BATCH + GRAD_BLOCK - 1) / GRAD_BLOCK;  // blocks of anchors whose losses a lane sums
static_assert(LOSS_BLOCKS <= 64, "one lane of the last workgroup per block of losses");

// acc[j] = the chain over c = 0 .. d-1 of acc = acc + (D[r][c] * q_j[c]) for the T queries at qs (LDS, [T][d]): two
// roundings per term, c ascending.  dt is D transposed.
template <int T>
__device__ __forceinline__ void apply_chains(const float* __restrict__ dt, int d, int r, const float* qs, float (&acc)[T]) {
#pragma unroll
    for (int j = 0; j < T; ++j) acc[j] = 0.0f;
    for (int c = 0; c < d; c += 4) {
        float w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = dt[(size_t)(c + u) * d + r];
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(qs + j * d + c);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[j] = __fadd_rn(acc[j], __fmul_rn(w[u], x[u]));
        }
    }
}

// Queries q0 .. q0 + T - 1 (zeros behind the last of n) -> LDS.
template <int T>
__device__ __forceinline__ void stage_queries(float* qs, const float* __restrict__ q, int64_t q0, int64_t n, int d, int tid,
                                              int n_threads) {
    for (int i = tid; i < T * d; i += n_threads) {
        const int64_t row = q0 + i / d;
        qs[i] = row < n ? q[row * d + i % d] : 0.0f;
    }
}

__global__ __launch_bounds__(APPLY_THREADS) void apply_kernel(const float* __restrict__ dt, int d, const float* __restrict__ q,
                                                              int64_t n, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float qs[APPLY_TILE * ICREC_ADAPTER_MAX_DIM];
    const int64_t q0 = (int64_t)blockIdx.x * APPLY_TILE;
    stage_queries<APPLY_TILE>(qs, q, q0, n, d, threadIdx.x, APPLY_THREADS);
    __syncthreads();
    const int r = blockIdx.y * APPLY_THREADS + threadIdx.x;
    if (r >= d) return;
    float acc[APPLY_TILE];
    apply_chains<APPLY_TILE>(dt, d, r, qs, acc);
#pragma unroll
    for (int j = 0; j < APPLY_TILE; ++j)
        if (q0 + j < n) out[(q0 + j) * d + r] = __fadd_rn(qs[j * d + r], acc[j]);
}

// z = apply(a) into LDS, then wave w takes anchor w of the tile: n = max(sqrt(sum z^2), 1e-12) in normalize_rows_kernel's
// order (64 strided fmaf partials, the xor butterfly), u = z / n.
__global__ __launch_bounds__(FWD_THREADS) void forward_kernel(const float* __restrict__ dt, int d, const float* __restrict__ a,
                                                              int B, float* __restrict__ U, float* __restrict__ nrm) {
    __shared__ __attribute__((aligned(16))) float as[FWD_TILE * ICREC_ADAPTER_MAX_DIM];
    __shared__ float zs[FWD_TILE * ICREC_ADAPTER_MAX_DIM];
    const int tid = threadIdx.x;
    const int64_t a0 = (int64_t)blockIdx.x * FWD_TILE;
    stage_queries<FWD_TILE>(as, a, a0, B, d, tid, FWD_THREADS);
    __syncthreads();
    for (int r = tid; r < d; r += FWD_THREADS) {
        float acc[FWD_TILE];
        apply_chains<FWD_TILE>(dt, d, r, as, acc);
#pragma unroll
        for (int j = 0; j < FWD_TILE; ++j) zs[j * d + r] = __fadd_rn(as[j * d + r], acc[j]);
    }
    __syncthreads();
    const int lane = tid & 63, j = tid >> 6;
    const int64_t i = a0 + j;
    if (i >= B) return;
    float s = 0.0f;
    for (int c = lane; c < d; c += 64) s = fmaf(zs[j * d + c], zs[j * d + c], s);
    const float len = sqrtf(wave_sum_f32(s));
    const float den = len > 1e-12f ? len : 1e-12f;
    for (int c = lane; c < d; c += 64) U[i * d + c] = zs[j * d + c] / den;
    if (lane == 0) nrm[i] = den;
}

__device__ __forceinline__ float stored_value(const float* p) { return *p; }
__device__ __forceinline__ float stored_value(const uint16_t* p) { return __uint_as_float((uint32_t)*p << 16); }

// (m, l) of a softmax over two disjoint parts: the maximum, and the sums moved onto it; (-inf, 0) is the empty part.
__device__ __forceinline__ void merge_max_sum(float& m, float& l, float m2, float l2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) return;
    l = l * expf(m - M) + l2 * expf(m2 - M);
    m = M;
}

// r names a stored row of an index of n_rows rows.  An anchor is counted iff its positive does, and no other value
// becomes an address.
__device__ __forceinline__ bool row_in_range(int32_t r, int64_t n_rows) { return r >= 0 && (int64_t)r < n_rows; }

// ---------------------------------------------------------------- the step's (b): what its two forms share
// Both forms of (b) - logits_kernel over a candidate list, the catalog_* kernels over every stored row - run on
// workgroups of four waves that hold ONE tile of 32 anchors and walk the rows in groups of four 32-row tiles, tile x of
// a group being wave x's.  A tile S^T[row][anchor] = V U^T is gathered_tile's: operand A the stored row of the lane's
// tile row, operand B the anchor's u, so a lane holds ONE anchor (its column, lane & 31) and sixteen tile rows (acc_row).
// The one thing the two forms do differently is where tile row jr of tile x gets its stored row; a ROW SOURCE says
// that, for one group and this lane's anchor, and everything below is written once over a source:
//   tile_live(x)    does tile x of the group exist
//   row(x, jr)      the stored row of its tile row jr, or -1: the tile row is dropped, and computed on fallback()
//   positive(x, jr) is it the anchor's positive
//   masked(x, jr)   does it stay out of the anchor's softmax
// The sources are passed by value and resolved when the kernel is compiled: nothing branches on the caller.

// The candidate list, checked once into LDS as -1 or the row.  A candidate out of range is masked for everybody, a far
// copy of the anchor's positive for that anchor; a dropped tile row is computed on row 0.
struct ListRows {
    const int32_t* crow;  // LDS: the checked row of candidate j, or -1
    int C, n_ct;          // the candidates and their tiles
    int g;                // the group's first tile
    int i, pos;           // this lane's anchor: candidate i is its positive, pos = crow[i], or -1 when it is not counted
    __device__ __forceinline__ bool tile_live(int x) const { return g + x < n_ct; }
    __device__ __forceinline__ int row(int x, int jr) const {
        const int j = (g + x) * 32 + jr;
        return j < C ? crow[j] : -1;
    }
    __device__ __forceinline__ int fallback() const { return 0; }
    __device__ __forceinline__ bool positive(int x, int jr) const { return (g + x) * 32 + jr == i; }
    __device__ __forceinline__ bool masked(int x, int jr) const {
        const int rj = row(x, jr);
        return rj < 0 || (!positive(x, jr) && rj == pos);
    }
};

// A split [r0, end) of the stored rows: a tile's rows are CONTIGUOUS, tile row jr of the tile at `first` is row
// first + jr.  A row at or behind `end` is computed on the split's first row and dropped by its INDEX - nothing depends
// on what lies behind n_rows - and nothing else is masked.
struct SpanRows {
    int64_t g0, end, r0;  // the group's first row; the end and the first row of the workgroup's split
    int64_t pos;          // the positive of this lane's anchor, or -1 when it is not counted
    __device__ __forceinline__ bool tile_live(int x) const { return g0 + x * 32 < end; }
    __device__ __forceinline__ int64_t row(int x, int jr) const {
        const int64_t r = g0 + x * 32 + jr;
        return r < end ? r : -1;
    }
    __device__ __forceinline__ int64_t fallback() const { return r0; }
    __device__ __forceinline__ bool positive(int x, int jr) const { return g0 + x * 32 + jr == pos; }
    __device__ __forceinline__ bool masked(int x, int jr) const { return row(x, jr) < 0; }
};

// The score tile: tile x of the group against the anchors at pu, this lane's stored row or the fallback row.
template <class Row, class Source>
__device__ __forceinline__ f32x16 score_tile(const Row* __restrict__ stored, const Source src, int x,
                                             const float* __restrict__ pu, int K, int lane) {
    const auto ra = src.row(x, lane & 31);
    f32x16 acc = {};
    gathered_tile(acc, stored + (size_t)(ra < 0 ? src.fallback() : ra) * K, pu, K, lane >> 5);
    return acc;
}

// The two halves of a wave hold (m, l) of the same anchors over different rows: half 0's part first, in both halves.
__device__ __forceinline__ void merge_halves(float& m, float& l, int h) {
    const float m_o = __shfl_xor(m, 32, 64), l_o = __shfl_xor(l, 32, 64);
    float m0 = h ? m_o : m, l0 = h ? l_o : l;
    merge_max_sum(m0, l0, h ? m : m_o, h ? l : l_o);
    m = m0;
    l = l0;
}

// The four waves' merged halves through LDS, in wave order, behind one barrier: every wave leaves with the same pair.
__device__ __forceinline__ void merge_waves(float& m, float& l, float (*m_s)[32], float (*l_s)[32], int w, int h, int l31) {
    merge_halves(m, l, h);
    if (h == 0) {
        m_s[w][l31] = m;
        l_s[w][l31] = l;
    }
    __syncthreads();
    m = m_s[0][l31];
    l = l_s[0][l31];
#pragma unroll
    for (int x = 1; x < LOGIT_WAVES; ++x) merge_max_sum(m, l, m_s[x][l31], l_s[x][l31]);
}

// body(tt, t) for the feature tiles t = w, w + 4, .. of dU^T that wave w owns, tt counting them.
template <class Body>
__device__ __forceinline__ void for_owned_tiles(int w, int K, Body body) {
    const int n_ft = K / 32;
#pragma unroll
    for (int tt = 0; tt < MAX_OWN_TILES; ++tt) {
        const int t = w + tt * LOGIT_WAVES;
        if (t < n_ft) body(tt, t);
    }
}

// Sweep 2's tile: P recomputed from the score tile against the final (M, 1 / L), G = (P - [positive]) / counted left
// in LDS as [tile row][anchor] - where it is operand B of dU^T = V^T G with no lane movement.
template <class Source>
__device__ __forceinline__ void store_g(float (*gs)[32], const f32x16& acc, const Source src, int x, int lane, float scale,
                                        float M, float inv_l, bool counted, float inv_counted) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int jr = acc_row(e, lane);
        const float p = src.masked(x, jr) ? 0.0f : expf(scale * acc[e] - M) * inv_l;
        gs[jr][lane & 31] = counted ? (p - (src.positive(x, jr) ? 1.0f : 0.0f)) * inv_counted : 0.0f;
    }
}

// Sweep 2's accumulation: every wave adds the group's tiles, in order, into the feature tiles of dU^T it owns - operand
// A the stored rows' features t * 32 + (lane & 31), 128 contiguous bytes per row, a dropped row's value replaced by
// zero.  A group's 128 rows are one fmaf chain from zero and the groups' sums are added in group order: two short
// levels instead of one chain of up to 8,192 terms, whose rounding error would grow with its length.  du and du_group
// are the kernels' register budget (eight tiles twice at d = 1,024: 256 VGPRs and most AGPRs, one wave per SIMD, no
// scratch - DESIGN.md 4.23 has the compiler's counts).  Small things decide it, 64-bit index arithmetic in the unrolled
// part and what is hoisted above it among them: ask the compiler (-Rpass-analysis=kernel-resource-usage) after a change.
template <class Row, class Source>
__device__ __forceinline__ void add_group(f32x16 (&du)[MAX_OWN_TILES], const Row* __restrict__ stored, const Source src,
                                          const float (*gs)[32][32], int K, int w, int lane) {
    const int h = lane >> 5, l31 = lane & 31;
    f32x16 du_group[MAX_OWN_TILES] = {};
    for (int x = 0; x < LOGIT_WAVES && src.tile_live(x); ++x) {
        float gb[16];
        size_t off[16];
        bool live[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {  // step s sums over tile rows 2s (lanes 0-31) and 2s + 1 (lanes 32-63)
            const int jr = 2 * s + h;
            const auto r = src.row(x, jr);
            gb[s] = gs[x][jr][l31];
            live[s] = r >= 0;
            off[s] = (size_t)(live[s] ? r : src.fallback()) * K + l31;
        }
        for_owned_tiles(w, K, [&](int tt, int t) {
            float va[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) va[s] = stored_value(stored + off[s] + t * 32);
#pragma unroll
            for (int s = 0; s < 16; ++s)
                du_group[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(live[s] ? va[s] : 0.0f, gb[s], du_group[tt], 0, 0, 0);
        });
    }
#pragma unroll
    for (int tt = 0; tt < MAX_OWN_TILES; ++tt)
#pragma unroll
        for (int e = 0; e < 16; ++e) du[tt][e] += du_group[tt][e];
}

// The list step's (b), all of it: one workgroup per 32 anchors.  A candidate's row number is checked once, into LDS.
// Sweep 1: wave w walks candidate tiles w, w + 4, ..; a lane keeps the RUNNING (maximum, sum) of its anchor over its
// candidates, and the halves and the waves are merged once, at the end.  Sweep 2, per group: wave w's tile -> G, the
// barrier, the group's accumulation.  Epilogue, in MFMA layout: du = scale * acc, the dot u . du over the waves'
// feature tiles through LDS in wave order, dz = (du - u (u . du)) / n.
template <bool P16>
__global__ __launch_bounds__(LOGIT_THREADS) void logits_kernel(const void* __restrict__ rows, int K, int64_t n_rows,
                                                               const float* __restrict__ U, const float* __restrict__ nrm,
                                                               const int32_t* __restrict__ cand, int B, int C, float scale,
                                                               float* __restrict__ dZ, float* __restrict__ loss_i) {
    typedef row_elem_t<P16> Row;
    __shared__ int32_t crow[ICREC_ADAPTER_MAX_CANDIDATES];
    __shared__ float gs[LOGIT_WAVES][32][32];
    __shared__ float m_s[LOGIT_WAVES][32], l_s[LOGIT_WAVES][32], dot_s[LOGIT_WAVES][32], spos[32];
    __shared__ int counted_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const Row* stored = static_cast<const Row*>(rows);
    if (tid == 0) counted_s = 0;
    if (tid < 32) spos[tid] = 0.0f;
    __syncthreads();
    int mine = 0;
    for (int j = tid; j < C; j += LOGIT_THREADS) {
        const int32_t r = cand[j];
        const bool ok = row_in_range(r, n_rows);
        crow[j] = ok ? r : -1;
        mine += (ok && j < B) ? 1 : 0;
    }
    if (mine) atomicAdd(&counted_s, mine);  // an integer count: any order gives the same value
    __syncthreads();
    const int n_counted = counted_s;
    const float inv_counted = n_counted > 0 ? 1.0f / (float)n_counted : 0.0f;
    const int i = blockIdx.x * ANCHOR_TILE + l31;  // this lane's anchor
    const bool in_b = i < B;
    const int pos = in_b ? crow[i] : -1;
    const bool counted = pos >= 0;
    const float* pu = U + (size_t)(in_b ? i : B - 1) * K;
    const int n_ct = (C + 31) / 32;

    float m = -INFINITY, l = 0.0f;
    for (int g = 0; g < n_ct; g += LOGIT_WAVES) {
        const ListRows src{crow, C, n_ct, g, i, pos};
        if (!src.tile_live(w)) break;
        const f32x16 acc = score_tile(stored, src, w, pu, K, lane);
        float sv[16], tm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int jr = acc_row(e, lane);
            const float s = scale * acc[e];
            if (src.positive(w, jr) && in_b) spos[l31] = s;  // one lane of the workgroup meets its anchor's own positive
            sv[e] = src.masked(w, jr) ? -INFINITY : s;
            tm = fmaxf(tm, sv[e]);
        }
        if (tm > -INFINITY) {
            const float nm = fmaxf(m, tm);
            float add = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) add += expf(sv[e] - nm);
            l = l * expf(m - nm) + add;
            m = nm;
        }
    }
    merge_waves(m, l, m_s, l_s, w, h, l31);
    const float M = counted ? m : 0.0f, L = counted ? l : 1.0f;  // not counted: no loss, no gradient, finite arithmetic below
    if (w == 0 && h == 0 && in_b) loss_i[i] = counted ? (M + logf(L)) - spos[l31] : 0.0f;
    const float inv_l = 1.0f / L;

    f32x16 du[MAX_OWN_TILES] = {};
    for (int g = 0; g < n_ct; g += LOGIT_WAVES) {
        const ListRows src{crow, C, n_ct, g, i, pos};
        if (src.tile_live(w)) {
            const f32x16 acc = score_tile(stored, src, w, pu, K, lane);
            store_g(gs[w], acc, src, w, lane, scale, M, inv_l, counted, inv_counted);
        }
        __syncthreads();
        add_group(du, stored, src, gs, K, w, lane);
        __syncthreads();
    }

    float part = 0.0f;
    for_owned_tiles(w, K, [&](int tt, int t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            du[tt][e] = scale * du[tt][e];
            part += pu[t * 32 + acc_row(e, lane)] * du[tt][e];
        }
    });
    {
        const float o = __shfl_xor(part, 32, 64);
        const float both = (h ? o : part) + (h ? part : o);
        if (h == 0) dot_s[w][l31] = both;
    }
    __syncthreads();
    float dot = dot_s[0][l31];
#pragma unroll
    for (int x = 1; x < LOGIT_WAVES; ++x) dot += dot_s[x][l31];
    if (!in_b) return;
    const float den = nrm[i];
    for_owned_tiles(w, K, [&](int tt, int t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int f = t * 32 + acc_row(e, lane);
            dZ[(size_t)i * K + f] = (du[tt][e] - pu[f] * dot) / den;
        }
    });
}


struct AdamW {
    float lr, one_minus_b1, b2, one_minus_b2, eps, decay, bc1, sqrt_bc2;  // decay = 1 - lr * weight_decay
};

// Workgroups 0 .. (K/32)^2 - 1, one wave each: tile (tr, tc) of dD[r][c] = sum over i of dz_i[r] a_i[c], i ascending
// (an MFMA step adds anchors 2s and 2s + 1 in that order; GRAD_BLOCK anchors are one chain, the blocks' sums are added
// in order); with `update`, torch's AdamW on the tile's elements - each
// element of D, its transposed copy, m and v is read and written by one lane.  The last workgroup sums the anchors'
// losses in the same two levels, in double - lane b adds block b's GRAD_BLOCK losses from zero in index order, lane 0
// adds the blocks' sums in block order - and divides by the counted anchors: the mean is rounded to float32 once.
__global__ __launch_bounds__(64) void grad_kernel(const float* __restrict__ dZ, const float* __restrict__ a, int B, int K,
                                                  const int32_t* __restrict__ cand, int64_t n_rows,
                                                  const float* __restrict__ loss_i, float* __restrict__ loss_out,
                                                  float* __restrict__ grad_out, int update, AdamW o, float* __restrict__ delta,
                                                  float* __restrict__ delta_t, float* __restrict__ m, float* __restrict__ v) {
    const int lane = threadIdx.x, h = lane >> 5, l31 = lane & 31;
    const int n_t = K / 32;
    if ((int)blockIdx.x == n_t * n_t) {
        __shared__ float ls[ICREC_ADAPTER_MAX_BATCH];
        __shared__ double bs[LOSS_BLOCKS];
        __shared__ int counted_s;
        if (lane == 0) counted_s = 0;
        __syncthreads();
        int mine = 0;
        for (int i = lane; i < B; i += 64) {
            const int32_t r = cand[i];
            mine += row_in_range(r, n_rows) ? 1 : 0;
            ls[i] = loss_i[i];
        }
        if (mine) atomicAdd(&counted_s, mine);
        __syncthreads();
        const int n_b = (B + GRAD_BLOCK - 1) / GRAD_BLOCK;
        if (lane < n_b) {  // lane b: block b's losses, one chain from zero in index order, in double
            const int b1 = (lane + 1) * GRAD_BLOCK < B ? (lane + 1) * GRAD_BLOCK : B;
            double s = 0.0;
            for (int i = lane * GRAD_BLOCK; i < b1; ++i) s += (double)ls[i];
            bs[lane] = s;
        }
        __syncthreads();
        if (lane == 0) {
            double s = 0.0;
            for (int b = 0; b < n_b; ++b) s += bs[b];  // the blocks' sums in block order
            *loss_out = counted_s > 0 ? (float)(s / (double)counted_s) : 0.0f;  // the mean's one float32 rounding
        }
        return;
    }
    const int tr = blockIdx.x / n_t, tc = blockIdx.x % n_t;
    const float* pz = dZ + tr * 32 + l31;
    const float* pa = a + tc * 32 + l31;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    for (int b0 = 0; b0 < B; b0 += GRAD_BLOCK) {  // a block of anchors is one chain from zero; the blocks are added in order
        f32x16 part;
#pragma unroll
        for (int e = 0; e < 16; ++e) part[e] = 0.0f;
        const int b1 = b0 + GRAD_BLOCK < B ? b0 + GRAD_BLOCK : B;
        for (int i0 = b0; i0 < b1; i0 += 2 * GRAD_DEPTH) {  // the loads of GRAD_DEPTH steps are issued before the first MFMA
            float z[GRAD_DEPTH], x[GRAD_DEPTH];
#pragma unroll
            for (int s = 0; s < GRAD_DEPTH; ++s) {
                const int i = i0 + 2 * s + h;
                z[s] = i < b1 ? pz[(size_t)i * K] : 0.0f;
                x[s] = i < b1 ? pa[(size_t)i * K] : 0.0f;
            }
#pragma unroll
            for (int s = 0; s < GRAD_DEPTH; ++s) part = __builtin_amdgcn_mfma_f32_32x32x2f32(z[s], x[s], part, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] += part[e];
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = tr * 32 + acc_row(e, lane), c = tc * 32 + l31;
        const size_t at = (size_t)r * K + c;
        const float g = acc[e];
        if (grad_out != nullptr) grad_out[at] = g;
        if (update) {
            float p = delta[at] * o.decay;
            const float m1 = m[at] + (g - m[at]) * o.one_minus_b1;
            const float v1 = v[at] * o.b2 + o.one_minus_b2 * g * g;
            p = p - (o.lr / o.bc1) * (m1 / (sqrtf(v1) / o.sqrt_bc2 + o.eps));
            delta[at] = p;
            delta_t[(size_t)c * K + r] = p;
            m[at] = m1;
            v[at] = v1;
        }
    }
}

// ---------------------------------------------------------------- the whole-catalog step (icrec_adapter_step_catalog)
// Every stored row is a candidate, so there is no list: the rows [0, n_rows) are cut into n_splits splits of
// rows_per_split rows (whole groups of CATALOG_GROUP = 128; the last split takes what is left), and the middle of the
// step is a grid of (anchor tiles x splits) workgroups, sized by catalog_plan from (B, n_rows) alone.  Two sweeps, as
// logits_kernel has them, with the merge of the splits between them:
//   catalog_max_sum_kernel  sweep 1: (maximum, sum) of every anchor over the workgroup's split, and the positive's logit
//   catalog_merge_kernel    the splits' pairs merged in split order -> (M, L) per anchor; the counted anchors
//   catalog_du_kernel       sweep 2: P recomputed against (M, L), G = (P - [r == pos]) / counted, the split's part of
//                           dU^T = V^T G, one part per split in the workspace
//   catalog_finish_kernel   the parts added in split order, du = scale * sum, u . du, dz, the anchor's loss
// The tiles are logits_kernel's (a lane holds ONE anchor and sixteen rows of a 32 x 32 tile), but a tile's rows are
// CONTIGUOUS: tile row j of the tile at `first` is row first + j, a row at or behind `end` is computed on the split's
// first row and dropped by its INDEX - nothing depends on what lies behind n_rows.
constexpr int CATALOG_GROUP = 32 * LOGIT_WAVES;   // rows of one chain of a sum over rows: a tile per wave
constexpr int CATALOG_TARGET_WORKGROUPS = 512;    // anchor tiles x splits aimed at: two per CU of a 256-CU chip
constexpr int CATALOG_MAX_SPLITS = 512;
constexpr int MERGE_DEPTH = 8;                    // splits whose values the merging kernels load at once
constexpr int FINISH_THREADS = 256;
constexpr int FINISH_OWN = ICREC_ADAPTER_MAX_DIM / FINISH_THREADS;  // features a finishing thread owns, at most
static_assert(ICREC_ADAPTER_MAX_DIM % FINISH_THREADS == 0, "the features are dealt to the finishing threads");

// The cut of n_rows rows for a batch of B: as many splits as bring anchor tiles x splits to CATALOG_TARGET_WORKGROUPS,
// at most CATALOG_MAX_SPLITS and at most one per group of rows; every split the same whole number of groups, which
// fixes their number.  It depends on nothing but its arguments.
struct CatalogPlan {
    int n_splits;
    int64_t rows_per_split;
};
CatalogPlan catalog_plan(int B, int64_t n_rows) {
    const int64_t n_groups = (n_rows + CATALOG_GROUP - 1) / CATALOG_GROUP;
    const int n_tiles = (B + ANCHOR_TILE - 1) / ANCHOR_TILE;
    int64_t want = (CATALOG_TARGET_WORKGROUPS + n_tiles - 1) / n_tiles;
    if (want > CATALOG_MAX_SPLITS) want = CATALOG_MAX_SPLITS;
    if (want > n_groups) want = n_groups;
    const int64_t groups_per_split = (n_groups + want - 1) / want;
    return CatalogPlan{(int)((n_groups + groups_per_split - 1) / groups_per_split), groups_per_split * CATALOG_GROUP};
}

// The lane's anchor of a catalog workgroup: its positive when it is counted (-1 otherwise: it equals no row).
__device__ __forceinline__ int64_t catalog_positive(const int32_t* __restrict__ pos_rows, int i, int B, int64_t n_rows) {
    if (i >= B) return -1;
    const int32_t r = pos_rows[i];
    return row_in_range(r, n_rows) ? (int64_t)r : -1;
}

// Sweep 1.  Per group of 128 rows wave w takes tile w: a lane's (maximum, sum) over its sixteen rows, then the halves
// and the waves merged PER GROUP into the group's pair, the groups' pairs merged in group order - every wave keeps the
// same running pair.  The pairs of a group are double buffered, so merge_waves' one barrier per group stands between
// its writes and its reads.
template <bool P16>
__global__ __launch_bounds__(LOGIT_THREADS) void catalog_max_sum_kernel(const void* __restrict__ rows, int K, int64_t n_rows,
                                                                        int64_t rows_per_split, const float* __restrict__ U,
                                                                        const int32_t* __restrict__ pos_rows, int B, float scale,
                                                                        float* __restrict__ m_part, float* __restrict__ l_part,
                                                                        float* __restrict__ s_pos) {
    typedef row_elem_t<P16> Row;
    __shared__ float m_s[2][LOGIT_WAVES][32], l_s[2][LOGIT_WAVES][32];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const Row* stored = static_cast<const Row*>(rows);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
    const int64_t end = r0 + rows_per_split < n_rows ? r0 + rows_per_split : n_rows;
    const int i = blockIdx.x * ANCHOR_TILE + l31;  // this lane's anchor
    const bool in_b = i < B;
    const int64_t pos = catalog_positive(pos_rows, i, B, n_rows);
    const float* pu = U + (size_t)(in_b ? i : B - 1) * K;
    float m = -INFINITY, l = 0.0f;
    int buf = 0;
    for (int64_t g0 = r0; g0 < end; g0 += CATALOG_GROUP, buf ^= 1) {
        const SpanRows src{g0, end, r0, pos};
        float gm = -INFINITY, gl = 0.0f;
        if (src.tile_live(w)) {
            const f32x16 acc = score_tile(stored, src, w, pu, K, lane);
            float sv[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int jr = acc_row(e, lane);
                const float s = scale * acc[e];
                const bool out = src.masked(w, jr);
                if (!out && src.positive(w, jr)) s_pos[i] = s;  // one lane of the grid meets a counted anchor's positive
                sv[e] = out ? -INFINITY : s;
                gm = fmaxf(gm, sv[e]);
            }
            if (gm > -INFINITY) {
#pragma unroll
                for (int e = 0; e < 16; ++e) gl += expf(sv[e] - gm);
            }
        }
        merge_waves(gm, gl, m_s[buf], l_s[buf], w, h, l31);
        merge_max_sum(m, l, gm, gl);
    }
    if (w == 0 && h == 0 && in_b) {
        m_part[(size_t)blockIdx.y * B + i] = m;
        l_part[(size_t)blockIdx.y * B + i] = l;
    }
}


// One workgroup: thread i merges anchor i's pairs in split order and the workgroup counts the anchors whose positive is
// in range.  ml[0 .. B) the maxima, ml[B .. 2B) the sums; an anchor that is not counted gets (0, 1), which keeps
// sweep 2's arithmetic finite.
__global__ __launch_bounds__(ICREC_ADAPTER_MAX_BATCH) void catalog_merge_kernel(const float* __restrict__ m_part,
                                                                                const float* __restrict__ l_part, int n_splits,
                                                                                const int32_t* __restrict__ pos_rows, int B,
                                                                                int64_t n_rows, float* __restrict__ ml,
                                                                                int32_t* __restrict__ counted_out) {
    __shared__ int counted_s;
    const int i = threadIdx.x;
    if (i == 0) counted_s = 0;
    __syncthreads();
    const bool counted = catalog_positive(pos_rows, i, B, n_rows) >= 0;
    if (counted) atomicAdd(&counted_s, 1);  // an integer count: any order gives the same value
    if (i < B) {
        float m = -INFINITY, l = 0.0f;
        for (int s0 = 0; s0 < n_splits; s0 += MERGE_DEPTH) {  // the loads of MERGE_DEPTH splits are issued before the first merge
            float pm[MERGE_DEPTH], pl[MERGE_DEPTH];
#pragma unroll
            for (int x = 0; x < MERGE_DEPTH; ++x) {  // behind the last split: the empty part, which changes nothing
                const bool in = s0 + x < n_splits;
                pm[x] = in ? m_part[(size_t)(s0 + x) * B + i] : -INFINITY;
                pl[x] = in ? l_part[(size_t)(s0 + x) * B + i] : 0.0f;
            }
#pragma unroll
            for (int x = 0; x < MERGE_DEPTH; ++x) merge_max_sum(m, l, pm[x], pl[x]);
        }
        ml[i] = counted ? m : 0.0f;
        ml[B + i] = counted ? l : 1.0f;
    }
    __syncthreads();
    if (i == 0) *counted_out = counted_s;
}

// Sweep 2 over the workgroup's split, per group of 128 rows as logits_kernel has it per group of four candidate tiles:
// wave w's tile -> G against the merged (M, L), the barrier, the group's accumulation.  The split's sums go to
// part[split][anchor][feature], unscaled.
template <bool P16>
__global__ __launch_bounds__(LOGIT_THREADS) void catalog_du_kernel(const void* __restrict__ rows, int K, int64_t n_rows,
                                                                   int64_t rows_per_split, const float* __restrict__ U,
                                                                   const float* __restrict__ ml,
                                                                   const int32_t* __restrict__ counted_in,
                                                                   const int32_t* __restrict__ pos_rows, int B, float scale,
                                                                   float* __restrict__ part) {
    typedef row_elem_t<P16> Row;
    __shared__ float gs[LOGIT_WAVES][32][32];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31;
    const Row* stored = static_cast<const Row*>(rows);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
    const int64_t end = r0 + rows_per_split < n_rows ? r0 + rows_per_split : n_rows;
    const int i = blockIdx.x * ANCHOR_TILE + l31;
    const bool in_b = i < B;
    const int64_t pos = catalog_positive(pos_rows, i, B, n_rows);
    const bool counted = pos >= 0;
    const int n_counted = *counted_in;
    const float inv_counted = n_counted > 0 ? 1.0f / (float)n_counted : 0.0f;
    const float M = in_b ? ml[i] : 0.0f;
    const float inv_l = 1.0f / (in_b ? ml[B + i] : 1.0f);
    const float* pu = U + (size_t)(in_b ? i : B - 1) * K;

    f32x16 du[MAX_OWN_TILES] = {};
    for (int64_t g0 = r0; g0 < end; g0 += CATALOG_GROUP) {
        const SpanRows src{g0, end, r0, pos};
        if (src.tile_live(w)) {
            const f32x16 acc = score_tile(stored, src, w, pu, K, lane);
            store_g(gs[w], acc, src, w, lane, scale, M, inv_l, counted, inv_counted);
        }
        __syncthreads();
        add_group(du, stored, src, gs, K, w, lane);
        __syncthreads();
    }
    if (!in_b) return;
    float* out = part + ((size_t)blockIdx.y * B + i) * K;
    for_owned_tiles(w, K, [&](int tt, int t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) out[t * 32 + acc_row(e, lane)] = du[tt][e];
    });
}


// One workgroup per anchor, a thread per feature f = tid, tid + 256, ..: the splits' parts added in split order,
// du = scale * sum; u . du as each thread's chain over its features ascending, the wave's xor butterfly, the four
// waves in wave order; dz = (du - u (u . du)) / n; the anchor's loss (0 when it is not counted: s_pos is then not read).
__global__ __launch_bounds__(FINISH_THREADS) void catalog_finish_kernel(const float* __restrict__ part, int n_splits, int B, int K,
                                                                        const float* __restrict__ U, const float* __restrict__ nrm,
                                                                        const float* __restrict__ ml, const float* __restrict__ s_pos,
                                                                        const int32_t* __restrict__ pos_rows, int64_t n_rows,
                                                                        float scale, float* __restrict__ dZ,
                                                                        float* __restrict__ loss_i) {
    __shared__ float dot_s[FINISH_THREADS / 64];
    const int tid = threadIdx.x, i = blockIdx.x;
    const float* pu = U + (size_t)i * K;
    float du[FINISH_OWN], dot = 0.0f;
#pragma unroll
    for (int o = 0; o < FINISH_OWN; ++o) {
        const int f = tid + o * FINISH_THREADS;
        du[o] = 0.0f;
        if (f < K) {
            float acc = part[(size_t)i * K + f];
            for (int s0 = 1; s0 < n_splits; s0 += MERGE_DEPTH) {  // loads first, then the additions in split order
                float v[MERGE_DEPTH];
#pragma unroll
                for (int x = 0; x < MERGE_DEPTH; ++x) v[x] = s0 + x < n_splits ? part[((size_t)(s0 + x) * B + i) * K + f] : 0.0f;
#pragma unroll
                for (int x = 0; x < MERGE_DEPTH; ++x) acc = s0 + x < n_splits ? acc + v[x] : acc;
            }
            du[o] = scale * acc;
            dot += pu[f] * du[o];
        }
    }
    dot = wave_sum_f32(dot);
    if ((tid & 63) == 0) dot_s[tid >> 6] = dot;
    __syncthreads();
    dot = dot_s[0];
#pragma unroll
    for (int x = 1; x < FINISH_THREADS / 64; ++x) dot += dot_s[x];
    const float den = nrm[i];
#pragma unroll
    for (int o = 0; o < FINISH_OWN; ++o) {
        const int f = tid + o * FINISH_THREADS;
        if (f < K) dZ[(size_t)i * K + f] = (du[o] - pu[f] * dot) / den;
    }
    if (tid == 0) loss_i[i] = catalog_positive(pos_rows, i, B, n_rows) >= 0 ? (ml[i] + logf(ml[B + i])) - s_pos[i] : 0.0f;
}

// ---------------------------------------------------------------- the step over per-anchor lists (icrec_adapter_step_lists)
// Every anchor has its OWN entries (a CSR segment of rows with a target each), so there is no tile of anchors against
// shared rows and no MFMA: the middle is a gathered matrix-vector product per anchor, twice.
//   lists_plan_kernel  a wave per anchor: T, the sum of its live targets, and a flag row - 0 when the anchor is counted,
//                      -1 when it is not - so that grad_kernel's row_in_range recount of the flags is the mean's divisor
//   lists_kernel       a workgroup per anchor: the segment checked once into LDS (a dropped entry as row -1, computed
//                      on row 0 behind a select, as compose_kernel does); sweep 1, a wave per entry, LISTS_SCORE_DEPTH
//                      entries in flight per wave, the scores kept in LDS; (maximum, sum) and the targets' part of the
//                      loss; G into LDS; sweep 2, compose_kernel's inner loop with the weights G; the epilogue
// The orders (include/icrec.h states them): a score is the lane's fmaf chain over its 16-byte pieces lane, lane + 64, ..
// features ascending, then the xor butterfly; a sum over entries in sweep 1 is the lane's chain over entries lane,
// lane + 64, .. then the butterfly (every wave computes the same values, so nothing is broadcast); sweep 2 adds groups
// of LISTS_GROUP entries, each one fmaf chain from zero in list order, in group order - logits_kernel's two levels.
constexpr int LISTS_THREADS = 256;
constexpr int LISTS_WAVES = LISTS_THREADS / 64;
constexpr int LISTS_SCORE_DEPTH = 4;  // entries whose pieces a wave of sweep 1 loads before the first fmaf
constexpr int LISTS_DEPTH = 8;        // entries whose pieces a thread of sweep 2 loads before the first fmaf
constexpr int LISTS_GROUP = 128;      // entries of one chain of sweep 2
static_assert(ICREC_ADAPTER_MAX_DIM / 4 <= LISTS_THREADS, "a thread of sweep 2 owns at most one piece of a row");
static_assert(LISTS_GROUP % LISTS_DEPTH == 0 && LISTS_SCORE_DEPTH <= LISTS_DEPTH, "the pad behind a segment covers both sweeps");

// The entries read of anchor i's segment: its first max_len, none when its end lies before its start.
__device__ __forceinline__ int segment_entries(const int32_t* __restrict__ off, int i, int max_len, int& lo) {
    lo = off[i];
    const int64_t n = (int64_t)off[i + 1] - lo;
    return n <= 0 ? 0 : (n < max_len ? (int)n : max_len);
}

// Is the entry live: a row of the index, a target that is finite and not negative.  Nothing else becomes an address.
__device__ __forceinline__ bool entry_live(int32_t r, float target, int64_t n_rows) {
    return row_in_range(r, n_rows) && finite_f32(target) && target >= 0.0f;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(LISTS_THREADS) void lists_plan_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ rows,
                                                                   const float* __restrict__ target, int B, int max_len,
                                                                   int64_t n_rows, float* __restrict__ T_out,
                                                                   int32_t* __restrict__ flag_out) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * LISTS_WAVES + (threadIdx.x >> 6);
    if (i >= B) return;  // a whole wave
    int lo;
    const int n_e = segment_entries(off, i, max_len, lo);
    float t = 0.0f;
    for (int e = lane; e < n_e; e += 64) {
        const int32_t r = rows[(int64_t)lo + e];
        const float x = target[(int64_t)lo + e];
        t += entry_live(r, x, n_rows) ? x : 0.0f;
    }
    t = wave_sum_f32(t);
    if (lane == 0) {
        T_out[i] = t;
        flag_out[i] = (finite_f32(t) && t > 0.0f) ? 0 : -1;
    }
}

template <bool P16>
__global__ __launch_bounds__(LISTS_THREADS) void lists_kernel(const void* __restrict__ rows, int K, int64_t n_rows,
                                                              const float* __restrict__ U, const float* __restrict__ nrm,
                                                              const int32_t* __restrict__ off, const int32_t* __restrict__ list_rows,
                                                              const float* __restrict__ list_target, int max_len,
                                                              const float* __restrict__ T_in, const int32_t* __restrict__ flag,
                                                              int B, float scale, float* __restrict__ dZ,
                                                              float* __restrict__ loss_i) {
    typedef row_elem_t<P16> Row;
    constexpr int P = P16 ? 8 : 4;  // features of one piece
    __shared__ int32_t e_row[ICREC_ADAPTER_MAX_LIST + LISTS_DEPTH];  // -1: a dropped entry, or the pad behind the last one
    __shared__ float e_t[ICREC_ADAPTER_MAX_LIST];                    // t_e = target / T; 0 for a dropped entry
    __shared__ float e_g[ICREC_ADAPTER_MAX_LIST + LISTS_DEPTH];      // G_e; 0 for a dropped entry and in the pad
    __shared__ float s_s[ICREC_ADAPTER_MAX_LIST];                    // s_e; -inf for a dropped entry
    __shared__ __attribute__((aligned(16))) float us[ICREC_ADAPTER_MAX_DIM];
    __shared__ float dot_s[LISTS_WAVES];
    __shared__ int counted_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = blockIdx.x;
    const int n_pc = K / P;
    float* dz = dZ + (size_t)i * K;
    if (flag[i] != 0) {  // not counted: neither loss nor gradient (the whole workgroup leaves)
        for (int f = tid; f < K; f += LISTS_THREADS) dz[f] = 0.0f;
        if (tid == 0) loss_i[i] = 0.0f;
        return;
    }
    if (tid == 0) counted_s = 0;
    __syncthreads();
    int lo;
    const int n_e = segment_entries(off, i, max_len, lo);
    const float T = T_in[i];  // finite and > 0: the anchor is counted
    for (int e = tid; e < n_e + LISTS_DEPTH; e += LISTS_THREADS) {
        int32_t r = -1;
        float t = 0.0f;
        if (e < n_e) {
            r = list_rows[(int64_t)lo + e];
            const float x = list_target[(int64_t)lo + e];
            const bool live = entry_live(r, x, n_rows);
            r = live ? r : -1;
            t = live ? x / T : 0.0f;
        }
        e_row[e] = r;
        if (e < n_e) e_t[e] = t;
    }
    for (int f = tid; f < K; f += LISTS_THREADS) us[f] = U[(size_t)i * K + f];
    int mine = 0;
    for (int a = tid; a < B; a += LISTS_THREADS) mine += flag[a] == 0 ? 1 : 0;
    if (mine) atomicAdd(&counted_s, mine);  // an integer count: any order gives the same value
    __syncthreads();
    const float inv_counted = 1.0f / (float)counted_s;  // this anchor is one of them

    // sweep 1: wave w scores entries [e0, e0 + LISTS_SCORE_DEPTH), their pieces loaded before the first fmaf
    const Row* stored = static_cast<const Row*>(rows);
    for (int e0 = w * LISTS_SCORE_DEPTH; e0 < n_e; e0 += LISTS_WAVES * LISTS_SCORE_DEPTH) {
        int row[LISTS_SCORE_DEPTH];
        float dot[LISTS_SCORE_DEPTH];
#pragma unroll
        for (int u = 0; u < LISTS_SCORE_DEPTH; ++u) {
            row[u] = e_row[e0 + u];
            dot[u] = 0.0f;
        }
        for (int c = lane; c < n_pc; c += 64) {
            u32x4 piece[LISTS_SCORE_DEPTH];
#pragma unroll
            for (int u = 0; u < LISTS_SCORE_DEPTH; ++u)  // every load is issued: a dropped entry reads row 0
                piece[u] = *reinterpret_cast<const u32x4*>(stored + (int64_t)(row[u] < 0 ? 0 : row[u]) * K + c * P);
            float x[P];
#pragma unroll
            for (int v = 0; v < P / 4; ++v) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(us + c * P + 4 * v);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[4 * v + j] = q[j];
            }
#pragma unroll
            for (int u = 0; u < LISTS_SCORE_DEPTH; ++u)
#pragma unroll
                for (int j = 0; j < P; ++j) dot[u] = fmaf(piece_value<P16>(piece[u], j), x[j], dot[u]);
        }
#pragma unroll
        for (int u = 0; u < LISTS_SCORE_DEPTH; ++u) {
            const float d = wave_sum_f32(dot[u]);
            if (lane == 0 && e0 + u < n_e) s_s[e0 + u] = row[u] < 0 ? -INFINITY : scale * d;
        }
    }
    __syncthreads();

    // the anchor's (maximum, sum) and sum of t_e s_e, the same chains in every wave
    float m = -INFINITY;
    for (int e = lane; e < n_e; e += 64) m = fmaxf(m, s_s[e]);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
    float l = 0.0f;
    double ts = 0.0;
    for (int e = lane; e < n_e; e += 64) {
        const float s = s_s[e];
        l += expf(s - m);  // a dropped entry: exp(-inf) = 0
        if (e_row[e] >= 0) ts += (double)e_t[e] * (double)s;
    }
    l = wave_sum_f32(l);
    ts = wave_sum_f64(ts);
    if (tid == 0) loss_i[i] = (float)(((double)m + log((double)l)) - ts);
    const float inv_l = 1.0f / l;
    for (int e = tid; e < n_e + LISTS_DEPTH; e += LISTS_THREADS)
        e_g[e] = (e < n_e && e_row[e] >= 0) ? (expf(s_s[e] - m) * inv_l - e_t[e]) * inv_counted : 0.0f;
    __syncthreads();

    // sweep 2: thread c owns piece c of every row; du = scale * sum_e G_e v_e
    const int c = tid;
    const bool own = c < n_pc;
    float du[P];
#pragma unroll
    for (int j = 0; j < P; ++j) du[j] = 0.0f;
    if (own) {
        const Row* col = stored + c * P;
        for (int g0 = 0; g0 < n_e; g0 += LISTS_GROUP) {
            float part[P];
#pragma unroll
            for (int j = 0; j < P; ++j) part[j] = 0.0f;
            const int g1 = g0 + LISTS_GROUP < n_e ? g0 + LISTS_GROUP : n_e;
            for (int t0 = g0; t0 < g1; t0 += LISTS_DEPTH) {
                u32x4 piece[LISTS_DEPTH];
                int row[LISTS_DEPTH];
#pragma unroll
                for (int u = 0; u < LISTS_DEPTH; ++u) {
                    row[u] = e_row[t0 + u];
                    piece[u] = *reinterpret_cast<const u32x4*>(col + (int64_t)(row[u] < 0 ? 0 : row[u]) * K);
                }
#pragma unroll
                for (int u = 0; u < LISTS_DEPTH; ++u) {
                    const float g = e_g[t0 + u];
#pragma unroll
                    for (int j = 0; j < P; ++j) {
                        const float sum = fmaf(g, piece_value<P16>(piece[u], j), part[j]);
                        part[j] = row[u] < 0 ? part[j] : sum;  // a select, not a branch: the waits stay counted
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < P; ++j) du[j] += part[j];
        }
    }
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        du[j] = scale * du[j];
        if (own) dot = fmaf(us[c * P + j], du[j], dot);
    }
    dot = wave_sum_f32(dot);
    if (lane == 0) dot_s[w] = dot;
    __syncthreads();
    dot = dot_s[0];
#pragma unroll
    for (int x = 1; x < LISTS_WAVES; ++x) dot += dot_s[x];
    if (!own) return;
    const float den = nrm[i];
#pragma unroll
    for (int v = 0; v < P / 4; ++v) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (du[4 * v + j] - us[c * P + 4 * v + j] * dot) / den;
        *reinterpret_cast<f32x4*>(dz + c * P + 4 * v) = o;
    }
}

bool dim_ok(int32_t dim) { return dim >= 32 && dim <= ICREC_ADAPTER_MAX_DIM && dim % 32 == 0; }

void release(Adapter* ad) {
    (void)hipFree(ad->delta);
    (void)hipFree(ad->delta_t);
    (void)hipFree(ad->m);
    (void)hipFree(ad->v);
    delete ad;
}

// A step's hyper-parameters, as every entry takes them.
struct Hyper {
    float scale, lr, beta1, beta2, eps, weight_decay;
    bool update;
};

// AdamW's constants for step t + 1, the bias corrections in double.
AdamW adamw_of(int64_t t, const Hyper& hp) {
    const double t1 = (double)(t + 1);
    AdamW o{};
    o.lr = hp.lr;
    o.one_minus_b1 = (float)(1.0 - (double)hp.beta1);
    o.b2 = hp.beta2;
    o.one_minus_b2 = (float)(1.0 - (double)hp.beta2);
    o.eps = hp.eps;
    o.decay = (float)(1.0 - (double)hp.lr * (double)hp.weight_decay);
    o.bc1 = (float)(1.0 - pow((double)hp.beta1, t1));
    o.sqrt_bc2 = (float)sqrt(1.0 - pow((double)hp.beta2, t1));
    return o;
}

// The workspace of a step: u [B][dim], dz [B][dim], the norms [B], the losses [B].  col: the bytes of a float per anchor.
struct StepWorkspace {
    size_t col, u, dz, nrm, loss, total;
    StepWorkspace(int dim, int B) : col(align256((size_t)B * sizeof(float))) {
        const size_t rows = align256((size_t)B * dim * sizeof(float));
        u = 0;
        dz = rows;
        nrm = 2 * rows;
        loss = 2 * rows + col;
        total = 2 * rows + 2 * col;
    }
};

// The workspace of a catalog step: the list step's arrays, then the positives' logits [B], (M, L) [2][B], the counted
// anchors, the splits' maxima and sums [n_splits][B] each, and the splits' parts of dU [n_splits][B][dim].
struct CatalogWorkspace {
    StepWorkspace step;
    size_t s_pos, ml, counted, m_part, l_part, part, total;
    CatalogWorkspace(int dim, int B, int n_splits) : step(dim, B) {
        const size_t cols = align256((size_t)n_splits * B * sizeof(float));
        s_pos = step.total;
        ml = s_pos + step.col;
        counted = ml + align256(2 * (size_t)B * sizeof(float));
        m_part = counted + 256;
        l_part = m_part + cols;
        part = l_part + cols;
        total = part + align256((size_t)n_splits * B * dim * sizeof(float));
    }
};

// The workspace of a step over lists: the list step's arrays, then the anchors' target sums [B] and flag rows [B].
struct ListsWorkspace {
    StepWorkspace step;
    size_t t_sum, flag, total;
    ListsWorkspace(int dim, int B) : step(dim, B) {
        t_sum = step.total;
        flag = t_sum + step.col;
        total = flag + step.col;
    }
};

// What the three step entries take alike, and what they do alike with it.  An entry reads: check(), its own checks, its
// workspace's layout, forward(), its own launches from U and nrm to dZ and loss_i, and grad() as its tail.
struct Step {
    const char* fn;  // the entry's name: it opens every message
    const Index* ix;
    Adapter* ad;
    const float* anchors_dev;
    int32_t B;
    Hyper hp;
    float *loss_out_dev, *grad_out_dev;
    char* base;  // the workspace
    size_t workspace_bytes;
    hipStream_t st;
    float *U = nullptr, *dZ = nullptr, *nrm = nullptr, *loss_i = nullptr;  // every workspace begins with them: forward()

    Step(const char* fn, icrec_index* idx, icrec_adapter* h, const float* anchors_dev, int32_t B, const Hyper& hp,
         float* loss_out_dev, float* grad_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream)
        : fn(fn), ix(reinterpret_cast<const Index*>(idx)), ad(reinterpret_cast<Adapter*>(h)), anchors_dev(anchors_dev), B(B),
          hp(hp), loss_out_dev(loss_out_dev), grad_out_dev(grad_out_dev), base(static_cast<char*>(workspace_dev)),
          workspace_bytes(workspace_bytes), st((hipStream_t)stream) {}

    template <class T = float>
    T* at(size_t offset) const { return reinterpret_cast<T*>(base + offset); }

    // What the entries check alike; `list` names the entry's row list, rows_dev.
    int check(const char* list, const int32_t* rows_dev) const {
        ICREC_REQUIRE(ix != nullptr, "%s: NULL idx", fn);
        ICREC_REQUIRE(ad != nullptr, "%s: NULL adapter", fn);
        ICREC_REQUIRE(anchors_dev != nullptr && rows_dev != nullptr, "%s: NULL anchors or %s", fn, list);
        ICREC_REQUIRE(loss_out_dev != nullptr, "%s: NULL loss_out", fn);
        ICREC_REQUIRE(base != nullptr, "%s: NULL workspace", fn);
        ICREC_REQUIRE(ix->dim == ad->dim, "%s: the index has dim %d, the adapter %d", fn, ix->dim, ad->dim);
        ICREC_REQUIRE(ix->device == ad->device, "%s: the index is on device %d, the adapter on %d", fn, ix->device, ad->device);
        ICREC_REQUIRE(ix->n_rows >= 1, "%s: the index has no rows", fn);
        ICREC_REQUIRE(B >= 1 && B <= ICREC_ADAPTER_MAX_BATCH, "%s: B must be in [1, %d] (got %d)", fn, ICREC_ADAPTER_MAX_BATCH, B);
        ICREC_REQUIRE(isfinite(hp.scale) && isfinite(hp.lr) && isfinite(hp.beta1) && isfinite(hp.beta2) && isfinite(hp.eps) &&
                          isfinite(hp.weight_decay),
                      "%s: a hyper-parameter is not finite", fn);
        ICREC_REQUIRE(!hp.update || (hp.beta1 >= 0.0f && hp.beta1 < 1.0f && hp.beta2 >= 0.0f && hp.beta2 < 1.0f && hp.eps >= 0.0f),
                      "%s: beta1 and beta2 must be in [0, 1) and eps >= 0", fn);
        return ICREC_OK;
    }

    // A workspace short of the entry's `total` bytes refused; then the step's (a): u and the norms of the anchors.
    int forward(const StepWorkspace& ws, size_t total) {
        ICREC_REQUIRE(workspace_bytes >= total, "%s: the workspace has %zu bytes, %zu are needed", fn, workspace_bytes, total);
        ICREC_HIP(hipSetDevice(ad->device));
        U = at(ws.u), dZ = at(ws.dz), nrm = at(ws.nrm), loss_i = at(ws.loss);
        hipLaunchKernelGGL(forward_kernel, dim3((unsigned)((B + FWD_TILE - 1) / FWD_TILE)), dim3(FWD_THREADS), 0, st,
                           (const float*)ad->delta_t, ad->dim, anchors_dev, (int)B, U, nrm);
        return ICREC_OK;
    }

    // The step's (c), from the dZ and the losses its (b) left: dD, AdamW when asked for, the mean loss.  rows_dev[0 .. B)
    // are the anchors' positives.  It ends the entry: the launches' error, and the step counted.
    int grad(const int32_t* rows_dev) {
        const int d = ad->dim;
        const AdamW o = hp.update ? adamw_of(ad->t, hp) : AdamW{};
        hipLaunchKernelGGL(grad_kernel, dim3((unsigned)((d / 32) * (d / 32) + 1)), dim3(64), 0, st, (const float*)dZ, anchors_dev,
                           (int)B, d, rows_dev, ix->n_rows, (const float*)loss_i, loss_out_dev, grad_out_dev, hp.update ? 1 : 0, o,
                           ad->delta, ad->delta_t, ad->m, ad->v);
        ICREC_HIP(hipGetLastError());
        if (hp.update) ad->t += 1;
        return ICREC_OK;
    }
};

}  // namespace
}  // namespace icrec

using namespace icrec;

extern "C" {

int icrec_adapter_create(int32_t dim, int device, icrec_adapter** out) {
    ICREC_REQUIRE(out != nullptr, "icrec_adapter_create: NULL out");
    *out = nullptr;
    ICREC_REQUIRE(dim_ok(dim), "icrec_adapter_create: dim must be a multiple of 32 in [32, %d] (got %d)",
                  ICREC_ADAPTER_MAX_DIM, dim);
    ICREC_HIP(hipSetDevice(device));
    Adapter* ad = new Adapter();
    ad->dim = dim;
    ad->device = device;
    const size_t bytes = (size_t)dim * dim * sizeof(float);
    float** arrays[4] = {&ad->delta, &ad->delta_t, &ad->m, &ad->v};
    for (float** p : arrays)
        if (hipMalloc(p, bytes) != hipSuccess || hipMemset(*p, 0, bytes) != hipSuccess) {
            set_error("icrec_adapter_create: hipMalloc of %zu bytes failed", bytes);
            release(ad);
            return ICREC_ENOMEM;
        }
    ICREC_HIP(hipDeviceSynchronize());
    *out = reinterpret_cast<icrec_adapter*>(ad);
    return ICREC_OK;
}

int icrec_adapter_destroy(icrec_adapter* h) {
    Adapter* ad = reinterpret_cast<Adapter*>(h);
    if (ad == nullptr) return ICREC_OK;
    (void)hipSetDevice(ad->device);
    (void)hipDeviceSynchronize();
    release(ad);
    return ICREC_OK;
}

int32_t icrec_adapter_dim(const icrec_adapter* h) { return h ? reinterpret_cast<const Adapter*>(h)->dim : 0; }

int icrec_adapter_set_state(icrec_adapter* h, const float* delta_host, const float* m_host, const float* v_host, int64_t t) {
    Adapter* ad = reinterpret_cast<Adapter*>(h);
    ICREC_REQUIRE(ad != nullptr, "icrec_adapter_set_state: NULL adapter");
    ICREC_REQUIRE(delta_host != nullptr, "icrec_adapter_set_state: NULL delta");
    ICREC_REQUIRE(t >= 0, "icrec_adapter_set_state: t must be >= 0 (got %lld)", (long long)t);
    const int d = ad->dim;
    const size_t n = (size_t)d * d, bytes = n * sizeof(float);
    std::vector<float> tr(n);
    for (int r = 0; r < d; ++r)
        for (int c = 0; c < d; ++c) tr[(size_t)c * d + r] = delta_host[(size_t)r * d + c];
    ICREC_HIP(hipSetDevice(ad->device));
    ICREC_HIP(hipDeviceSynchronize());  // a set-up call: whatever still reads the arrays finishes first
    ICREC_HIP(hipMemcpy(ad->delta, delta_host, bytes, hipMemcpyHostToDevice));
    ICREC_HIP(hipMemcpy(ad->delta_t, tr.data(), bytes, hipMemcpyHostToDevice));
    if (m_host != nullptr) ICREC_HIP(hipMemcpy(ad->m, m_host, bytes, hipMemcpyHostToDevice));
    else ICREC_HIP(hipMemset(ad->m, 0, bytes));
    if (v_host != nullptr) ICREC_HIP(hipMemcpy(ad->v, v_host, bytes, hipMemcpyHostToDevice));
    else ICREC_HIP(hipMemset(ad->v, 0, bytes));
    ICREC_HIP(hipDeviceSynchronize());
    ad->t = t;
    return ICREC_OK;
}

int icrec_adapter_get_state(const icrec_adapter* h, float* delta_host, float* m_host, float* v_host, int64_t* t_out) {
    const Adapter* ad = reinterpret_cast<const Adapter*>(h);
    ICREC_REQUIRE(ad != nullptr, "icrec_adapter_get_state: NULL adapter");
    const size_t bytes = (size_t)ad->dim * ad->dim * sizeof(float);
    ICREC_HIP(hipSetDevice(ad->device));
    ICREC_HIP(hipDeviceSynchronize());
    if (delta_host != nullptr) ICREC_HIP(hipMemcpy(delta_host, ad->delta, bytes, hipMemcpyDeviceToHost));
    if (m_host != nullptr) ICREC_HIP(hipMemcpy(m_host, ad->m, bytes, hipMemcpyDeviceToHost));
    if (v_host != nullptr) ICREC_HIP(hipMemcpy(v_host, ad->v, bytes, hipMemcpyDeviceToHost));
    if (t_out != nullptr) *t_out = ad->t;
    return ICREC_OK;
}

int icrec_adapter_apply(const icrec_adapter* h, const float* q_dev, int32_t n, float* out_dev, void* stream) {
    const Adapter* ad = reinterpret_cast<const Adapter*>(h);
    ICREC_REQUIRE(ad != nullptr, "icrec_adapter_apply: NULL adapter");
    ICREC_REQUIRE(q_dev != nullptr && out_dev != nullptr, "icrec_adapter_apply: NULL q or out");
    ICREC_REQUIRE(q_dev != out_dev, "icrec_adapter_apply: out must not be q");
    ICREC_REQUIRE(n >= 1, "icrec_adapter_apply: n must be >= 1 (got %d)", n);
    ICREC_HIP(hipSetDevice(ad->device));
    const dim3 grid((unsigned)((n + APPLY_TILE - 1) / APPLY_TILE), (unsigned)((ad->dim + APPLY_THREADS - 1) / APPLY_THREADS));
    hipLaunchKernelGGL(apply_kernel, grid, dim3(APPLY_THREADS), 0, (hipStream_t)stream, (const float*)ad->delta_t, ad->dim,
                       q_dev, (int64_t)n, out_dev);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

size_t icrec_adapter_step_workspace_bytes(const icrec_adapter* h, int32_t B, int32_t C) {
    const Adapter* ad = reinterpret_cast<const Adapter*>(h);
    if (ad == nullptr || B < 1 || B > ICREC_ADAPTER_MAX_BATCH || C < B || C > ICREC_ADAPTER_MAX_CANDIDATES) return 0;
    return StepWorkspace(ad->dim, B).total;
}

int icrec_adapter_step(icrec_index* idx, icrec_adapter* h, const float* anchors_dev, int32_t B, const int32_t* cand_rows_dev,
                       int32_t C, float scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int32_t update, float* loss_out_dev, float* grad_out_dev, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
    Step s("icrec_adapter_step", idx, h, anchors_dev, B, Hyper{scale, lr, beta1, beta2, eps, weight_decay, update != 0},
           loss_out_dev, grad_out_dev, workspace_dev, workspace_bytes, stream);
    int rc = s.check("cand_rows", cand_rows_dev);
    if (rc != ICREC_OK) return rc;
    ICREC_REQUIRE(C >= B && C <= ICREC_ADAPTER_MAX_CANDIDATES, "icrec_adapter_step: C must be in [B, %d] (got %d, B %d)",
                  ICREC_ADAPTER_MAX_CANDIDATES, C, B);
    const StepWorkspace ws(s.ad->dim, B);
    rc = s.forward(ws, ws.total);
    if (rc != ICREC_OK) return rc;
    hipLaunchKernelGGL((rows_are_bf16(s.ix) ? logits_kernel<true> : logits_kernel<false>),
                       dim3((unsigned)((B + ANCHOR_TILE - 1) / ANCHOR_TILE)), dim3(LOGIT_THREADS), 0, s.st,
                       (const void*)s.ix->rows, s.ad->dim, s.ix->n_rows, (const float*)s.U, (const float*)s.nrm, cand_rows_dev,
                       (int)B, (int)C, scale, s.dZ, s.loss_i);
    return s.grad(cand_rows_dev);
}


int icrec_adapter_catalog_plan(const icrec_adapter* h, int32_t B, int64_t n_rows, int32_t* n_splits, int64_t* rows_per_split) {
    ICREC_REQUIRE(h != nullptr, "icrec_adapter_catalog_plan: NULL adapter");
    ICREC_REQUIRE(n_splits != nullptr && rows_per_split != nullptr, "icrec_adapter_catalog_plan: NULL n_splits or rows_per_split");
    ICREC_REQUIRE(B >= 1 && B <= ICREC_ADAPTER_MAX_BATCH, "icrec_adapter_catalog_plan: B must be in [1, %d] (got %d)",
                  ICREC_ADAPTER_MAX_BATCH, B);
    ICREC_REQUIRE(n_rows >= 1, "icrec_adapter_catalog_plan: n_rows must be >= 1 (got %lld)", (long long)n_rows);
    const CatalogPlan plan = catalog_plan(B, n_rows);
    *n_splits = plan.n_splits;
    *rows_per_split = plan.rows_per_split;
    return ICREC_OK;
}

size_t icrec_adapter_step_catalog_workspace_bytes(const icrec_adapter* h, const icrec_index* idx, int32_t B) {
    const Adapter* ad = reinterpret_cast<const Adapter*>(h);
    const Index* ix = reinterpret_cast<const Index*>(idx);
    if (ad == nullptr || ix == nullptr || ix->n_rows < 1 || B < 1 || B > ICREC_ADAPTER_MAX_BATCH) return 0;
    return CatalogWorkspace(ad->dim, B, catalog_plan(B, ix->n_rows).n_splits).total;
}

int icrec_adapter_step_catalog(icrec_index* idx, icrec_adapter* h, const float* anchors_dev, int32_t B,
                               const int32_t* pos_rows_dev, float scale, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int32_t update, float* loss_out_dev, float* grad_out_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream) {
    Step s("icrec_adapter_step_catalog", idx, h, anchors_dev, B, Hyper{scale, lr, beta1, beta2, eps, weight_decay, update != 0},
           loss_out_dev, grad_out_dev, workspace_dev, workspace_bytes, stream);
    int rc = s.check("pos_rows", pos_rows_dev);
    if (rc != ICREC_OK) return rc;
    const int64_t n_rows = s.ix->n_rows;  // the rows of this call: the plan, every bound and the count use this one value
    const CatalogPlan plan = catalog_plan(B, n_rows);
    const CatalogWorkspace ws(s.ad->dim, B, plan.n_splits);
    rc = s.forward(ws.step, ws.total);
    if (rc != ICREC_OK) return rc;
    float *s_pos = s.at(ws.s_pos), *ml = s.at(ws.ml), *m_part = s.at(ws.m_part), *l_part = s.at(ws.l_part), *part = s.at(ws.part);
    int32_t* counted = s.at<int32_t>(ws.counted);
    const int d = s.ad->dim;
    const bool p16 = rows_are_bf16(s.ix);
    const dim3 grid((unsigned)((B + ANCHOR_TILE - 1) / ANCHOR_TILE), (unsigned)plan.n_splits);
    hipLaunchKernelGGL((p16 ? catalog_max_sum_kernel<true> : catalog_max_sum_kernel<false>), grid, dim3(LOGIT_THREADS), 0, s.st,
                       (const void*)s.ix->rows, d, n_rows, plan.rows_per_split, (const float*)s.U, pos_rows_dev, (int)B, scale,
                       m_part, l_part, s_pos);
    hipLaunchKernelGGL(catalog_merge_kernel, dim3(1), dim3(ICREC_ADAPTER_MAX_BATCH), 0, s.st, (const float*)m_part,
                       (const float*)l_part, plan.n_splits, pos_rows_dev, (int)B, n_rows, ml, counted);
    hipLaunchKernelGGL((p16 ? catalog_du_kernel<true> : catalog_du_kernel<false>), grid, dim3(LOGIT_THREADS), 0, s.st,
                       (const void*)s.ix->rows, d, n_rows, plan.rows_per_split, (const float*)s.U, (const float*)ml,
                       (const int32_t*)counted, pos_rows_dev, (int)B, scale, part);
    hipLaunchKernelGGL(catalog_finish_kernel, dim3((unsigned)B), dim3(FINISH_THREADS), 0, s.st, (const float*)part, plan.n_splits,
                       (int)B, d, (const float*)s.U, (const float*)s.nrm, (const float*)ml, (const float*)s_pos, pos_rows_dev,
                       n_rows, scale, s.dZ, s.loss_i);
    return s.grad(pos_rows_dev);
}

size_t icrec_adapter_step_lists_workspace_bytes(const icrec_adapter* h, int32_t B) {
    const Adapter* ad = reinterpret_cast<const Adapter*>(h);
    if (ad == nullptr || B < 1 || B > ICREC_ADAPTER_MAX_BATCH) return 0;
    return ListsWorkspace(ad->dim, B).total;
}

int icrec_adapter_step_lists(icrec_index* idx, icrec_adapter* h, const float* anchors_dev, int32_t B,
                             const int32_t* list_off_dev, const int32_t* list_rows_dev, const float* list_target_dev,
                             int32_t max_len, float scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int32_t update, float* loss_out_dev, float* grad_out_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream) {
    Step s("icrec_adapter_step_lists", idx, h, anchors_dev, B, Hyper{scale, lr, beta1, beta2, eps, weight_decay, update != 0},
           loss_out_dev, grad_out_dev, workspace_dev, workspace_bytes, stream);
    int rc = s.check("list_off", list_off_dev);
    if (rc != ICREC_OK) return rc;
    ICREC_REQUIRE(list_rows_dev != nullptr && list_target_dev != nullptr, "icrec_adapter_step_lists: NULL list_rows or list_target");
    ICREC_REQUIRE(max_len >= 1 && max_len <= ICREC_ADAPTER_MAX_LIST, "icrec_adapter_step_lists: max_len must be in [1, %d] (got %d)",
                  ICREC_ADAPTER_MAX_LIST, max_len);
    const int64_t n_rows = s.ix->n_rows;  // the rows of this call: both kernels check against this one value
    const ListsWorkspace ws(s.ad->dim, B);
    rc = s.forward(ws.step, ws.total);
    if (rc != ICREC_OK) return rc;
    float* t_sum = s.at(ws.t_sum);
    int32_t* flag = s.at<int32_t>(ws.flag);
    hipLaunchKernelGGL(lists_plan_kernel, dim3((unsigned)((B + LISTS_WAVES - 1) / LISTS_WAVES)), dim3(LISTS_THREADS), 0, s.st,
                       list_off_dev, list_rows_dev, list_target_dev, (int)B, (int)max_len, n_rows, t_sum, flag);
    hipLaunchKernelGGL((rows_are_bf16(s.ix) ? lists_kernel<true> : lists_kernel<false>), dim3((unsigned)B), dim3(LISTS_THREADS), 0,
                       s.st, (const void*)s.ix->rows, s.ad->dim, n_rows, (const float*)s.U, (const float*)s.nrm, list_off_dev,
                       list_rows_dev, list_target_dev, (int)max_len, (const float*)t_sum, (const int32_t*)flag, (int)B, scale,
                       s.dZ, s.loss_i);
    // the flag rows stand in for the positives: row 0 is in range for a counted anchor, -1 is not
    return s.grad(flag);
}


}  // extern "C"
