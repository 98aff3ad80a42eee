// ivf.hip — an inverted-file (IVF) index over an icrec_index: the rows are split into n_lists lists around centroids
// and a query scans only the nprobe lists whose centroids it matches best.  The result is the exact top-k over the
// union of the probed lists, in icrec_search's bits; with nprobe == n_lists it IS icrec_search's.
// Creation (a set-up call): the centroids become a private fp32 index; every stored row is assigned to the list
// icrec_search(centroid index, stored row, k = 1) names, in passes over slices of the rows; a stable counting sort on
// the host gives perm (the rows by (list, row)) and list_off; the IVF keeps its own copy of the stored rows in perm
// order.  A search is four steps on the caller's stream:
//   normalize_rows_kernel  the queries, as icrec_search normalises them -> the workspace
//   icrec_search           on the centroid index, k = nprobe: the probe lists int64[Q, nprobe]
//   ivf_scan_kernel        one workgroup per (query, probe, slice): the k best keys of its slice of its list
//   launch_merge(_block)   the nprobe * S partial lists of every query -> the outputs
// The definition is in include/icrec.h; tests/ivf_reference.py states it in numpy.
#include <vector>

#include "index.h"
#include "stream.h"

namespace icrec {
namespace {

struct Ivf {
    const Index* base = nullptr;
    icrec_index* cent = nullptr;   // the centroids, ICREC_ROWS_F32, row offset 0
    int n_lists = 0;
    int64_t n_rows = 0;            // the base's rows when the IVF was made (the base may gain or lose rows: icrec_index_append_rows)
    void* rows = nullptr;          // the base's stored rows in perm order, in the base's row element type
    int32_t* perm = nullptr;       // [n_rows] local rows sorted by (list, row)
    int64_t* list_off = nullptr;   // [n_lists + 1]
};

constexpr int64_t ASSIGN_SLICE_BYTES = 64ll << 20;  // fp32 bytes of the rows one assignment pass searches with

// bf16 rows [r0, r0 + n / dim) widened exactly: the queries of one assignment pass
__global__ __launch_bounds__(256) void ivf_widen_kernel(const uint16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = bf16_lo(in[i]);
}

// out row pos = in row perm[pos], in 16-byte pieces (a row is a whole number of 128-byte slabs)
__global__ __launch_bounds__(256) void ivf_gather_kernel(const char* __restrict__ in, const int32_t* __restrict__ perm,
                                                         int64_t n_rows, int row_bytes, char* __restrict__ out) {
    const int per_row = row_bytes / 16;
    const int64_t n = n_rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t pos = i / per_row;
        const int c = (int)(i - pos * per_row);
        *reinterpret_cast<v4f*>(out + pos * row_bytes + c * 16) =
            *reinterpret_cast<const v4f*>(in + (int64_t)perm[pos] * row_bytes + c * 16);
    }
}

// 128-B slab `slab` of the 256 rows at positions pos0 .. pos0 + 255 -> 8 x 16 B per thread (positions clamped to the
// list's last row, hi - 1: nothing outside the list is read)
__device__ __forceinline__ void ivf_load_slab(v4f (&pre)[8], const char* __restrict__ Pb, int64_t pos0, int64_t hi,
                                              int row_bytes, int slab, int tid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + ST_ROWS * i;
        int64_t pos = pos0 + (id >> 3);
        pos = pos < hi ? pos : hi - 1;
        pre[i] = *reinterpret_cast<const v4f*>(Pb + pos * row_bytes + slab * 128 + (id & 7) * 16);
    }
}

// ---------------------------------------------------------------- the scan of one slice of one probed list
// Workgroup (query q, probe p, slice s) of n_queries * nprobe * S: list = probes[q][p], rows at positions
// [list_off[list], list_off[list + 1]) of the gathered copy, cut into tiles of 256 rows; slice s walks tiles
// [s * tps, (s + 1) * tps), tps = ceil(tiles / S).  Loading and arithmetic are stream_search_kernel's at one query:
// 128-byte slabs through LDS, the next slab in flight under the current slab's FMAs, one fp32 chain per thread and
// row, j ascending.  A candidate's key carries its ORIGINAL row, row_base + perm[pos], and the exclusion test runs on
// perm[pos]: the order inside a list and the cut into slices cannot show in the result.  Selection is the streaming
// kernel's: the first tile is ranked by counting, later tiles offer only keys above the running k-th into the LDS
// queue that merge_queue folds into the sorted list.  A slice without tiles writes k pads.
// partial: [p * S + s][Q][k].
template <bool P16>
__global__ __launch_bounds__(ST_ROWS, 2) void ivf_scan_kernel(
    const void* __restrict__ P, const int32_t* __restrict__ perm, const int64_t* __restrict__ list_off, int n_lists,
    int K, const float* __restrict__ Qn /* [Q][K] */, int Q, int k, int nprobe, int S,
    const int64_t* __restrict__ probes /* [Q][nprobe] */, const int32_t* __restrict__ excl_idx,
    const int32_t* __restrict__ excl_off, uint32_t row_base, u64* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* rows_s = smem_raw;
    int* cnt = reinterpret_cast<int*>(smem_raw + ST_ROWS * ST_LDB);
    u64* queue = reinterpret_cast<u64*>(cnt + 4);  // 16-B aligned: the cold path reads it two keys at a time
    u64* list = queue + ST_ROWS;

    constexpr int EPW = P16 ? 2 : 1;      // elements per 32-bit word
    constexpr int SLAB_ELEMS = 32 * EPW;  // 128 B of one row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per_query = nprobe * S;
    const int q = blockIdx.x / per_query, ls = blockIdx.x - q * per_query;  // ls = p * S + s
    const int p = ls / S, s = ls - p * S;
    const int row_bytes = K * (P16 ? 2 : 4);
    const int nslab = K / SLAB_ELEMS;
    const char* Pb = static_cast<const char*>(P);
    u64* out = partial + ((size_t)ls * Q + q) * k;

    const int64_t lst = probes[(size_t)q * nprobe + p];
    int64_t lo = 0, hi = 0;
    if (lst >= 0 && lst < n_lists) { lo = list_off[lst]; hi = list_off[lst + 1]; }  // (a probe is always a list)
    const int tiles = (int)((hi - lo + ST_ROWS - 1) / ST_ROWS);
    const int tps = (tiles + S - 1) / S;
    const int t_begin = s * tps;
    const int t_end = min(tiles, t_begin + tps);
    if (t_begin >= t_end) {  // uniform: an empty list, or a list of fewer tiles than slices
        for (int i = tid; i < k; i += ST_ROWS) out[i] = 0ull;
        return;
    }

    if (tid == 0) cnt[0] = 0;
    for (int i = tid; i < k; i += ST_ROWS) list[i] = 0ull;
    int ex_lo = 0, ex_hi = 0;
    if (excl_off != nullptr) { ex_lo = excl_off[q]; ex_hi = excl_off[q + 1]; }
    u64 mythr = 0ull;
    const float* qv = Qn + (size_t)q * K;

    v4f pre[8];  // native vectors: HIP's float4 struct copies become memcpys that pin the array in scratch
    ivf_load_slab(pre, Pb, lo + (int64_t)t_begin * ST_ROWS, hi, row_bytes, 0, tid);

    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t pos = lo + (int64_t)tile * ST_ROWS + tid;
        const int orig = pos < hi ? perm[pos] : 0;  // in flight under the FMAs
        float acc = 0.0f;
        for (int sl = 0; sl < nslab; ++sl) {
            __syncthreads();  // the previous slab has been consumed (also covers the list/cnt initialisation)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int id = tid + ST_ROWS * i;
                *reinterpret_cast<v4f*>(rows_s + (id >> 3) * ST_LDB + (id & 7) * 16) = pre[i];
            }
            __syncthreads();
            {   // next slab (of this tile or the first of the next one) goes in flight under this slab's FMAs;
                // unconditional — the block's very last iteration re-loads its own slab — so `pre` stays in registers
                const bool wrap = sl + 1 == nslab;
                const int nt = wrap ? min(tile + 1, t_end - 1) : tile, ns = wrap ? 0 : sl + 1;
                ivf_load_slab(pre, Pb, lo + (int64_t)nt * ST_ROWS, hi, row_bytes, ns, tid);
            }
            const char* my = rows_s + tid * ST_LDB;
            const float* qs = qv + (size_t)sl * SLAB_ELEMS;  // block-uniform: scalar loads
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const v4f w = *reinterpret_cast<const v4f*>(my + c * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (P16) {
                        const unsigned u = __float_as_uint(w[e]);
                        const int kk = c * 8 + e * 2;
                        acc = fmaf(qs[kk], bf16_lo(u), acc);
                        acc = fmaf(qs[kk + 1], bf16_hi(u), acc);
                    } else {
                        acc = fmaf(qs[c * 4 + e], w[e], acc);
                    }
                }
            }
        }

        // ---- selection for this tile's 256 scores
        const u64 kx = make_key(acc + 0.0f, row_base + (uint32_t)orig);
        bool take = pos < hi && kx > mythr;
        if (take && ex_hi > ex_lo) take = !excluded(excl_idx, ex_lo, ex_hi, orig);
        const u64 key = take ? kx : 0ull;
        if (tile == t_begin) {
            // cold: rank every key among the tile's 256 by counting; rank r < k goes straight to list[r]
            queue[tid] = key;
            __syncthreads();
            int r = 0;
            for (int i = 0; i < ST_ROWS; i += 2) {
                const ulonglong2 two = *reinterpret_cast<const ulonglong2*>(queue + i);  // LDS broadcast
                r += (two.x > key) + (two.y > key);
            }
            if (key != 0ull && r < k) list[r] = key;
            __syncthreads();
        } else {
            if (key != 0ull) queue[atomicAdd(&cnt[0], 1)] = key;  // <= 256 offers per tile
            __syncthreads();
            if (wave == 0) {
                const int c = cnt[0];
                for (int off = 0; off < c; off += 64) merge_queue(list, queue + off, min(64, c - off), k, lane);
                if (lane == 0) cnt[0] = 0;
            }
            __syncthreads();
        }
        mythr = list[k - 1];
    }

    __syncthreads();
    for (int i = tid; i < k; i += ST_ROWS) out[i] = list[i];
}

size_t scan_smem(int k) { return (size_t)ST_ROWS * ST_LDB + 16 /*cnt*/ + (size_t)ST_ROWS * 8 /*queue*/ + (size_t)k * 8; }

// The slices per probed list of a call, the same for all its lists: enough that the (query, probe, slice) workgroups of
// a single request fill the chip, two per CU (the kernel's launch bound), one once Q * nprobe does that alone; and
// nprobe * S partial lists per query must fit the merge.
int plan_slices(const Ivf* v, int Q, int nprobe) {
    const int64_t target = 2 * (int64_t)v->base->n_cu, items = (int64_t)Q * nprobe;
    if (items >= target) return 1;
    const int64_t want = (target + items - 1) / items, cap = MERGE_MAX_LISTS / nprobe;
    return (int)(want < cap ? want : cap);
}

// Workspace: [normalised queries | probe lists | probe scores | partial lists | the coarse search's own].
struct IvfPlan {
    int S;
    size_t off_probe, off_pscore, off_partial, off_coarse, coarse_bytes, total;
};
IvfPlan make_ivf_plan(const Ivf* v, int Q, int k, int nprobe) {
    IvfPlan p;
    p.S = plan_slices(v, Q, nprobe);
    p.off_probe = align256((size_t)Q * v->base->dim * 4);
    p.off_pscore = p.off_probe + align256((size_t)Q * nprobe * 8);
    p.off_partial = p.off_pscore + align256((size_t)Q * nprobe * 4);
    p.off_coarse = p.off_partial + align256((size_t)nprobe * p.S * Q * k * 8);
    p.coarse_bytes = icrec_search_workspace_bytes(v->cent, Q, nprobe);
    p.total = p.off_coarse + align256(p.coarse_bytes);
    return p;
}

bool search_shape_ok(const Ivf* v, int Q, int k, int nprobe) {
    return v && Q >= 1 && k >= 1 && k <= ICREC_MAX_K && nprobe >= 1 && nprobe <= v->n_lists && nprobe <= ICREC_MAX_K &&
           (int64_t)Q * nprobe * plan_slices(v, Q, nprobe) <= 0x7FFFFFFFll;
}

// list(r) for every row, on the host: passes of icrec_search(centroids, stored rows of a slice, k = 1).
int assign_rows(const Ivf* v, std::vector<int32_t>& assign) {
    const Index* ix = v->base;
    const int64_t n = ix->n_rows;
    int64_t slice = ASSIGN_SLICE_BYTES / ((int64_t)ix->dim * 4);
    slice = slice < 1 ? 1 : slice > n ? n : slice;
    const size_t ws_bytes = icrec_search_workspace_bytes(v->cent, (int32_t)slice, 1);
    float* wide = nullptr;
    int64_t* idx = nullptr;
    float* sc = nullptr;
    void* ws = nullptr;
    auto release = [&]() { (void)hipFree(wide); (void)hipFree(idx); (void)hipFree(sc); (void)hipFree(ws); };
    const bool rows16 = rows_are_bf16(ix);
    if ((rows16 && hipMalloc(&wide, (size_t)slice * ix->dim * 4) != hipSuccess) || hipMalloc(&idx, (size_t)slice * 8) != hipSuccess ||
        hipMalloc(&sc, (size_t)slice * 4) != hipSuccess || hipMalloc(&ws, ws_bytes) != hipSuccess) {
        release();
        set_error("icrec_ivf_create: hipMalloc of the assignment buffers failed");
        return ICREC_ENOMEM;
    }
    std::vector<int64_t> host((size_t)slice);
    assign.resize((size_t)n);
    for (int64_t r0 = 0; r0 < n; r0 += slice) {
        const int64_t m = n - r0 < slice ? n - r0 : slice;
        const float* q = static_cast<const float*>(ix->rows) + r0 * ix->dim;
        if (rows16) {
            const int64_t cnt = m * ix->dim;
            hipLaunchKernelGGL(ivf_widen_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0,
                               static_cast<const uint16_t*>(ix->rows) + r0 * ix->dim, wide, cnt);
            q = wide;
        }
        int rc = icrec_search(v->cent, q, (int32_t)m, 1, nullptr, nullptr, idx, sc, ws, ws_bytes, nullptr);
        if (rc == ICREC_OK && hipMemcpy(host.data(), idx, (size_t)m * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("icrec_ivf_create: copying the assignment to the host failed");
            rc = ICREC_EHIP;
        }
        if (rc != ICREC_OK) { release(); return rc; }
        for (int64_t i = 0; i < m; ++i) assign[(size_t)(r0 + i)] = (int32_t)host[(size_t)i];
    }
    release();
    return ICREC_OK;
}

}  // namespace
}  // namespace icrec

using namespace icrec;

extern "C" {

int icrec_ivf_destroy(icrec_ivf* h) {
    Ivf* v = reinterpret_cast<Ivf*>(h);
    if (!v) return ICREC_OK;
    (void)hipSetDevice(v->base->device);
    icrec_index_destroy(v->cent);
    (void)hipFree(v->rows);
    (void)hipFree(v->perm);
    (void)hipFree(v->list_off);
    delete v;
    return ICREC_OK;
}

int icrec_ivf_create(icrec_index* base, const float* centroids_dev, int32_t n_lists, icrec_ivf** out) {
    const Index* ix = reinterpret_cast<const Index*>(base);
    ICREC_REQUIRE(ix && centroids_dev && out, "icrec_ivf_create: NULL argument");
    ICREC_REQUIRE(n_lists >= 1 && n_lists <= ix->n_rows, "icrec_ivf_create: n_lists must be in [1, n_rows = %lld] (got %d)",
                  (long long)ix->n_rows, n_lists);
    ICREC_REQUIRE(ix->n_rows < 0x80000000ll, "icrec_ivf_create: the base index must have fewer than 2^31 rows");
    ICREC_HIP(hipSetDevice(ix->device));
    Ivf* v = new Ivf();
    v->base = ix;
    v->n_lists = n_lists;
    auto fail = [&](int rc) {
        icrec_ivf_destroy(reinterpret_cast<icrec_ivf*>(v));
        return rc;
    };
    if (int rc = icrec_index_create_ex(centroids_dev, n_lists, ix->dim, 0, ix->device, ICREC_ROWS_F32, &v->cent)) return fail(rc);
    std::vector<int32_t> assign;
    if (int rc = assign_rows(v, assign)) return fail(rc);
    // stable counting sort by list: perm = the rows by (list, row)
    const int64_t n = ix->n_rows;
    std::vector<int64_t> off((size_t)n_lists + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
        if (assign[(size_t)r] < 0 || assign[(size_t)r] >= n_lists) {
            set_error("icrec_ivf_create: row %lld was assigned to list %d of %d", (long long)r, assign[(size_t)r], n_lists);
            return fail(ICREC_EHIP);
        }
        ++off[(size_t)assign[(size_t)r] + 1];
    }
    for (int l = 0; l < n_lists; ++l) off[(size_t)l + 1] += off[(size_t)l];
    std::vector<int32_t> perm((size_t)n);
    {
        std::vector<int64_t> next(off.begin(), off.end() - 1);
        for (int64_t r = 0; r < n; ++r) perm[(size_t)next[(size_t)assign[(size_t)r]]++] = (int32_t)r;
    }
    const int row_bytes = ix->dim * (rows_are_bf16(ix) ? 2 : 4);
    if (hipMalloc(&v->rows, (size_t)n * row_bytes) != hipSuccess || hipMalloc(&v->perm, (size_t)n * 4) != hipSuccess ||
        hipMalloc(&v->list_off, ((size_t)n_lists + 1) * 8) != hipSuccess) {
        set_error("icrec_ivf_create: hipMalloc of the gathered rows (%zu bytes) failed", (size_t)n * row_bytes);
        return fail(ICREC_ENOMEM);
    }
    if (hipMemcpy(v->perm, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->list_off, off.data(), ((size_t)n_lists + 1) * 8, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("icrec_ivf_create: copying the layout to the device failed");
        return fail(ICREC_EHIP);
    }
    hipLaunchKernelGGL(ivf_gather_kernel, dim3(4096), dim3(256), 0, 0, static_cast<const char*>(ix->rows),
                       (const int32_t*)v->perm, n, row_bytes, static_cast<char*>(v->rows));
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) {
        set_error("icrec_ivf_create: gathering the rows failed");
        return fail(ICREC_EHIP);
    }
    v->n_rows = n;
    *out = reinterpret_cast<icrec_ivf*>(v);
    return ICREC_OK;
}

int32_t icrec_ivf_lists(const icrec_ivf* h) { return h ? reinterpret_cast<const Ivf*>(h)->n_lists : -1; }

int icrec_ivf_layout(const icrec_ivf* h, int32_t* perm_dev, int64_t* list_off_dev, void* stream) {
    const Ivf* v = reinterpret_cast<const Ivf*>(h);
    ICREC_REQUIRE(v && perm_dev && list_off_dev, "icrec_ivf_layout: NULL argument");
    ICREC_HIP(hipSetDevice(v->base->device));
    ICREC_HIP(hipMemcpyAsync(perm_dev, v->perm, (size_t)v->n_rows * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    ICREC_HIP(hipMemcpyAsync(list_off_dev, v->list_off, ((size_t)v->n_lists + 1) * 8, hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
    return ICREC_OK;
}

size_t icrec_ivf_search_workspace_bytes(const icrec_ivf* h, int32_t n_queries, int32_t k, int32_t nprobe) {
    const Ivf* v = reinterpret_cast<const Ivf*>(h);
    if (!search_shape_ok(v, n_queries, k, nprobe)) return 0;
    return make_ivf_plan(v, n_queries, k, nprobe).total;
}

int icrec_ivf_search(icrec_ivf* h, const float* q_dev, int32_t n_queries, int32_t k, int32_t nprobe,
                     const int32_t* excl_idx_dev, const int32_t* excl_off_dev, int64_t* out_idx_dev, float* out_score_dev,
                     void* ws, size_t ws_bytes, void* stream) {
    const Ivf* v = reinterpret_cast<const Ivf*>(h);
    ICREC_REQUIRE(v && q_dev && out_idx_dev && out_score_dev, "icrec_ivf_search: NULL argument");
    ICREC_REQUIRE(n_queries >= 1, "icrec_ivf_search: n_queries must be >= 1 (got %d)", n_queries);
    ICREC_REQUIRE(k >= 1 && k <= ICREC_MAX_K, "icrec_ivf_search: k must be in [1, %d] (got %d)", ICREC_MAX_K, k);
    const int max_probe = v->n_lists < ICREC_MAX_K ? v->n_lists : ICREC_MAX_K;
    ICREC_REQUIRE(nprobe >= 1 && nprobe <= max_probe, "icrec_ivf_search: nprobe must be in [1, %d] (got %d)", max_probe, nprobe);
    ICREC_REQUIRE((excl_idx_dev == nullptr) == (excl_off_dev == nullptr),
                  "icrec_ivf_search: excl_idx and excl_off must both be set or both NULL");
    ICREC_REQUIRE(search_shape_ok(v, n_queries, k, nprobe), "icrec_ivf_search: %d queries of %d probes are too many for one call",
                  n_queries, nprobe);
    const IvfPlan p = make_ivf_plan(v, n_queries, k, nprobe);
    if (ws_bytes < p.total || ws == nullptr) {
        set_error("icrec_ivf_search: workspace too small (%zu < %zu)", ws_bytes, p.total);
        return ICREC_ENOMEM;
    }
    const Index* ix = v->base;
    ICREC_HIP(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    char* wb = static_cast<char*>(ws);
    float* qn = reinterpret_cast<float*>(wb);
    int64_t* probes = reinterpret_cast<int64_t*>(wb + p.off_probe);
    float* pscore = reinterpret_cast<float*>(wb + p.off_pscore);
    u64* partial = reinterpret_cast<u64*>(wb + p.off_partial);
    hipLaunchKernelGGL(normalize_rows_kernel<false>, dim3((unsigned)((n_queries + 3) / 4)), dim3(256), 0, st, q_dev, (void*)qn,
                       (int64_t)n_queries, (int64_t)n_queries, ix->dim, 1e-12f, 0);
    // the coarse search takes the queries as given: it normalises them itself, to the same bits
    if (int rc = icrec_search(v->cent, q_dev, n_queries, nprobe, nullptr, nullptr, probes, pscore, wb + p.off_coarse,
                              p.coarse_bytes, stream))
        return rc;
    {
        ScopedTimer tm(T_IVF_SCAN, st);
        hipLaunchKernelGGL((rows_are_bf16(ix) ? ivf_scan_kernel<true> : ivf_scan_kernel<false>),
                           dim3((unsigned)((int64_t)n_queries * nprobe * p.S)), dim3(ST_ROWS), scan_smem(k), st,
                           (const void*)v->rows, (const int32_t*)v->perm, (const int64_t*)v->list_off, v->n_lists, ix->dim,
                           (const float*)qn, n_queries, k, nprobe, p.S, (const int64_t*)probes, excl_idx_dev, excl_off_dev,
                           (uint32_t)ix->row_offset, partial);
    }
    ICREC_HIP(hipGetLastError());
    if (!launch_merge_block(partial, nprobe * p.S, n_queries, n_queries, k, out_idx_dev, out_score_dev, nullptr, st))
        launch_merge(partial, nprobe * p.S, n_queries, n_queries, k, out_idx_dev, out_score_dev, nullptr, nullptr, st);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
