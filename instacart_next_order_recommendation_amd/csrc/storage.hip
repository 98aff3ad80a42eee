// storage.hip — everything that writes, moves, clears, resizes or exports what an index keeps per row; storage.h has
// the layouts and the entry points' contracts.  index.hip checks the arguments and owns the handle; search.hip only reads.
#include <stdlib.h>

#include "storage.h"

namespace icrec {

// The normalised rows as packed fragments (frag_slot), one thread per (fragment, lane); rows past n_rows are zero.
template <bool SRC16>
__global__ __launch_bounds__(256) void pack_rows_kernel(const void* __restrict__ src, int64_t n_rows, int K, int64_t n_frag,
                                                        _Float16* __restrict__ out) {
    const int KS = K / 16;
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < n_frag * 64; id += (int64_t)gridDim.x * 256) {
        const int64_t fr = id >> 6;
        const int lane = (int)(id & 63), r = lane & 31, h = lane >> 5;
        const int64_t rt = fr / KS;
        const int ks = (int)(fr % KS);
        const int64_t row = rt * 32 + r;
        half8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = 0.0f;
            if (row < n_rows) {
                const size_t at = (size_t)row * K + ks * 16 + 8 * h + j;
                v = SRC16 ? bf16_lo(static_cast<const uint16_t*>(src)[at]) : static_cast<const float*>(src)[at];
            }
            _Float16 a, b;
            filter_split<LAYOUT_FRAGS>(v, a, b);
            hi[j] = a;
            lo[j] = b;
        }
        _Float16* at = frag_slot(out, row, 2 * ks + h, K);
        *reinterpret_cast<half8*>(at) = hi;
        *reinterpret_cast<half8*>(at + WT_FRAG) = lo;
    }
}

// Dimension 384 takes the fragments INSTEAD of the planes: against the staged pass 0.26 vs 0.39 ms at 49,688 rows x
// 1,024 queries, 19.6 vs 30.1 ms at 10 M rows (same box, top-20; DESIGN.md has the rest).
int build_filter_storage(Index* ix) {
    FilterStorage& fs = ix->filter;
    const int64_t n_rows = ix->n_rows;  // (== the capacity: a new index)
    const bool rows16 = rows_are_bf16(ix);
    const char* res_env = getenv("ICREC_FILTER_RESIDENT");  // "0": staged form; a number > 1: row limit of the resident form (A/B)
    const int64_t res_max = res_env && atoll(res_env) > 1 ? atoll(res_env) : INT64_MAX;  // (no limit unless set)
    if (ix->dim == 16 * RES_KS && n_rows <= res_max && !(res_env && res_env[0] == '0' && res_env[1] == 0)) {
        const int64_t n_frag = frag_row_tiles(n_rows) * RES_KS;
        if (hipMalloc(&fs.frag, (size_t)n_frag * 2 * WT_FRAG * sizeof(_Float16)) != hipSuccess) {
            set_error("icrec_index_create: hipMalloc of the filter fragments (%zu bytes) failed", (size_t)n_frag * 2 * WT_FRAG * 2);
            return ICREC_ENOMEM;
        }
        hipLaunchKernelGGL((rows16 ? pack_rows_kernel<true> : pack_rows_kernel<false>), dim3(4096), dim3(256), 0, 0,
                           (const void*)ix->rows, n_rows, ix->dim, n_frag, fs.frag);
    } else {
        const size_t n = (size_t)n_rows * ix->dim;
        if (hipMalloc(&fs.plane_hi, n * 2) != hipSuccess || hipMalloc(&fs.plane_lo, n * 2) != hipSuccess) {
            set_error("icrec_index_create: hipMalloc of the filter planes (2 x %zu bytes) failed", n * 2);
            return ICREC_ENOMEM;
        }
        hipLaunchKernelGGL((rows16 ? split_planes_kernel<true> : split_planes_kernel<false>), dim3(4096), dim3(256), 0, 0,
                           (const void*)ix->rows, n, fs.plane_hi, fs.plane_lo, (int*)nullptr);
    }
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

// The instantiations of a kernel template <bool rows are bf16, int LAYOUT>, indexed [rows_are_bf16(ix)][filter_layout(ix)].
#define STORAGE_KERNELS(kernel)                                                                  \
    {{kernel<false, LAYOUT_NONE>, kernel<false, LAYOUT_PLANES>, kernel<false, LAYOUT_FRAGS>},    \
     {kernel<true, LAYOUT_NONE>, kernel<true, LAYOUT_PLANES>, kernel<true, LAYOUT_FRAGS>}}

// ---------------------------------------------------------------- rows rewritten in place (icrec_index_write_rows)
// One wavefront per written row w: row ids[w] (ids == NULL, icrec_index_append_rows: row base + w) becomes what
// icrec_index_create_ex makes of x[w].  The norm is normalize_rows_kernel's, lane for lane (64 strided fmaf partials,
// the xor butterfly, the same division), so the stored bits are a fresh index's.  The STORED values (bf16: rounded,
// widened back) go through LDS, so that a lane then owns 8 consecutive k and every store is 16 bytes: the row itself,
// and from the same values (filter_split) its slice of both planes or chunk c's fragment slot (frag_slot).  A row
// outside [0, n_rows) writes nothing: it is tested before any address is formed.  No other row's bytes are touched.
template <bool OUT16, int LAYOUT>
__global__ __launch_bounds__(256) void write_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ ids, int64_t base,
                                                         int m, void* __restrict__ rowsv, int64_t n_rows, int dim,
                                                         _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                         _Float16* __restrict__ frag) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* st = reinterpret_cast<float*>(smem_raw) + (size_t)wave * dim;  // this wave's stored values
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;
    int64_t row = -1;  // wave-uniform
    if (w < m) {
        const int64_t id = ids ? (int64_t)ids[w] : base + w;
        if (id >= 0 && id < n_rows) row = id;
    }
    if (row >= 0) {
        const float* xr = x + w * dim;
        float acc = 0.0f;
        for (int i = lane; i < dim; i += 64) {
            float v = xr[i];
            acc = fmaf(v, v, acc);
        }
        float nrm = sqrtf(wave_sum_f32(acc));
        float den = nrm > 1e-12f ? nrm : 1e-12f;
        for (int i = lane; i < dim; i += 64) {
            const float v = xr[i] / den;
            st[i] = OUT16 ? bf16_lo(bf16_rne(v)) : v;
        }
    }
    __syncthreads();
    if (row < 0) return;
    for (int c = lane; c < dim / 8; c += 64) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(st + 8 * c), b = *reinterpret_cast<const f32x4*>(st + 8 * c + 4);
        const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        if (OUT16) {
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (__float_as_uint(v[2 * j]) >> 16) | (__float_as_uint(v[2 * j + 1]) & 0xFFFF0000u);
            *reinterpret_cast<u32x4*>(static_cast<uint16_t*>(rowsv) + row * dim + 8 * c) = o;
        } else {
            float* out = static_cast<float*>(rowsv) + row * dim + 8 * c;
            *reinterpret_cast<f32x4*>(out) = a;
            *reinterpret_cast<f32x4*>(out + 4) = b;
        }
        if (LAYOUT == LAYOUT_NONE) continue;
        half8 ph, pl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            _Float16 s, t;
            filter_split<LAYOUT>(v[j], s, t);
            ph[j] = s;
            pl[j] = t;
        }
        if (LAYOUT == LAYOUT_PLANES) {
            *reinterpret_cast<half8*>(hi + row * dim + 8 * c) = ph;
            *reinterpret_cast<half8*>(lo + row * dim + 8 * c) = pl;
        } else {
            _Float16* at = frag_slot(frag, row, c, dim);
            *reinterpret_cast<half8*>(at) = ph;
            *reinterpret_cast<half8*>(at + WT_FRAG) = pl;
        }
    }
}

int write_index_rows(Index* ix, const float* rows_dev, const int32_t* row_ids_dev, int32_t m, int64_t base_row, hipStream_t st) {
    static const decltype(&write_rows_kernel<false, LAYOUT_NONE>) kernels[2][3] = STORAGE_KERNELS(write_rows_kernel);
    hipLaunchKernelGGL(kernels[rows_are_bf16(ix)][filter_layout(ix)], dim3((unsigned)(((int64_t)m + 3) / 4)), dim3(256),
                       (size_t)4 * ix->dim * sizeof(float), st, rows_dev, row_ids_dev, base_row, (int)m, ix->rows,
                       row_ids_dev ? ix->n_rows : base_row + m, ix->dim, ix->filter.plane_hi, ix->filter.plane_lo, ix->filter.frag);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

// ---------------------------------------------------------------- rows moved in place (icrec_index_remove_rows)
// One wavefront per move i: everything the index keeps for row src[i] is copied to row dst[i] as the STORED bits (the
// filter copy is a function of the stored values alone, so nothing is normalised or split again), in 16-byte pieces:
// the row, its slice of both planes or its fragment slots (frag_slot).  Then the facet word and the row's bit in every
// row set: several destinations can share a 32-bit word, so the bit is set or cleared atomically.
// Sources (>= new_n) and destinations (< new_n) are disjoint and each is named once: no wave writes what another reads.
// Nothing is cleared here - a source's word or fragment tile may hold other sources that a later wave still reads;
// clear_rows_kernel runs behind this launch.  A move outside dst < new_n <= src < old_n is skipped before any address
// is formed from it.
template <bool OUT16, int LAYOUT>
__global__ __launch_bounds__(256) void move_rows_kernel(const int32_t* __restrict__ dst, const int32_t* __restrict__ src,
                                                        int n_moves, int64_t new_n, int64_t old_n, void* rowsv, int dim,
                                                        _Float16* hi, _Float16* lo, _Float16* frag, uint16_t* facets,
                                                        uint32_t* sets, int n_sets, int64_t set_words) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_moves) return;
    const int64_t d = dst[w], s = src[w];  // wave-uniform
    if (d < 0 || d >= new_n || s < new_n || s >= old_n) return;
    const int row_chunks = dim * (OUT16 ? 2 : 4) / 16;
    const u32x4* rs = reinterpret_cast<const u32x4*>(static_cast<const char*>(rowsv) + (size_t)s * row_chunks * 16);
    u32x4* rd = reinterpret_cast<u32x4*>(static_cast<char*>(rowsv) + (size_t)d * row_chunks * 16);
    for (int c = lane; c < row_chunks; c += 64) rd[c] = rs[c];
    if (LAYOUT != LAYOUT_NONE) {
        for (int c = lane; c < dim / 8; c += 64) {
            if (LAYOUT == LAYOUT_PLANES) {
                *reinterpret_cast<half8*>(hi + d * dim + 8 * c) = *reinterpret_cast<const half8*>(hi + s * dim + 8 * c);
                *reinterpret_cast<half8*>(lo + d * dim + 8 * c) = *reinterpret_cast<const half8*>(lo + s * dim + 8 * c);
            } else {
                const _Float16* from = frag_slot(frag, s, c, dim);
                _Float16* to = frag_slot(frag, d, c, dim);
                *reinterpret_cast<half8*>(to) = *reinterpret_cast<const half8*>(from);
                *reinterpret_cast<half8*>(to + WT_FRAG) = *reinterpret_cast<const half8*>(from + WT_FRAG);
            }
        }
    }
    if (facets != nullptr && lane == 0) facets[d] = facets[s];
    for (int t = lane; t < n_sets; t += 64) {
        uint32_t* bits = sets + (size_t)t * set_words;
        const uint32_t bit = 1u << (d & 31);
        if ((bits[s >> 5] >> (s & 31)) & 1u) atomicOr(bits + (d >> 5), bit);
        else atomicAnd(bits + (d >> 5), ~bit);
    }
}

// Behind move_rows_kernel: what a fresh index keeps zero past its last row becomes zero again for the rows
// [new_n, old_n) - their fragment slots and facet words (one wavefront per row) and their bits of every row set (the
// whole grid over (set, word) pairs: the word that straddles new_n keeps its low bits).  The stored rows and the planes
// past n_rows are addressed by nothing and stay.  Every slot and word is written by one thread and read by none.
template <bool FRAGS>
__global__ __launch_bounds__(256) void clear_rows_kernel(int64_t new_n, int64_t old_n, int dim, _Float16* frag, uint16_t* facets,
                                                         uint32_t* sets, int n_sets, int64_t set_words) {
    const int lane = threadIdx.x & 63;
    const int64_t row = new_n + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < old_n) {
        if (FRAGS) {
            half8 z;
#pragma unroll
            for (int j = 0; j < 8; ++j) z[j] = (_Float16)0.0f;
            for (int c = lane; c < dim / 8; c += 64) {
                _Float16* at = frag_slot(frag, row, c, dim);
                *reinterpret_cast<half8*>(at) = z;
                *reinterpret_cast<half8*>(at + WT_FRAG) = z;
            }
        }
        if (facets != nullptr && lane == 0) facets[row] = 0;
    }
    const int64_t w0 = new_n >> 5, nw = ((old_n + 31) >> 5) - w0;  // the words that hold a bit of the tail
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nw * n_sets; i += (int64_t)gridDim.x * 256) {
        uint32_t* word = sets + (size_t)(i / nw) * set_words + w0 + i % nw;
        *word = (i % nw == 0 && (new_n & 31)) ? *word & ((1u << (new_n & 31)) - 1u) : 0u;
    }
}

int move_index_rows(Index* ix, const int32_t* dst_dev, const int32_t* src_dev, int32_t n_moves, int64_t new_n, int64_t old_n,
                    hipStream_t st) {
    static const decltype(&move_rows_kernel<false, LAYOUT_NONE>) kernels[2][3] = STORAGE_KERNELS(move_rows_kernel);
    const FilterStorage& fs = ix->filter;
    const int n_sets = ix->rowsets ? ix->n_rowsets : 0;
    const int64_t words = rowset_words(ix->capacity);
    if (n_moves > 0) {
        hipLaunchKernelGGL(kernels[rows_are_bf16(ix)][filter_layout(ix)], dim3((unsigned)(((int64_t)n_moves + 3) / 4)), dim3(256), 0,
                           st, dst_dev, src_dev, (int)n_moves, new_n, old_n, ix->rows, ix->dim, fs.plane_hi, fs.plane_lo, fs.frag,
                           ix->facets, ix->rowsets, n_sets, words);
        ICREC_HIP(hipGetLastError());
    }
    if (fs.frag || ix->facets || n_sets > 0) {
        hipLaunchKernelGGL((fs.frag ? clear_rows_kernel<true> : clear_rows_kernel<false>), dim3((unsigned)((old_n - new_n + 3) / 4)),
                           dim3(256), 0, st, new_n, old_n, ix->dim, fs.frag, ix->facets, ix->rowsets, n_sets, words);
        ICREC_HIP(hipGetLastError());
    }
    return ICREC_OK;
}

// icrec_index_reserve.  A fragment's place depends on its row tile alone, so the live rows are a prefix of the new array; zero behind them.
int reserve_filter_storage(const Index* ix, int64_t capacity, FilterStorage* out) {
    const FilterStorage& fs = ix->filter;
    if (fs.frag) {
        const size_t tile_bytes = (size_t)RES_KS * 2 * WT_FRAG * sizeof(_Float16), bytes = (size_t)frag_row_tiles(capacity) * tile_bytes;
        if (hipMalloc(&out->frag, bytes) != hipSuccess) {
            out->frag = nullptr;
            set_error("icrec_index_reserve: hipMalloc of the filter fragments (%zu bytes) failed", bytes);
            return ICREC_ENOMEM;
        }
        const size_t live = (size_t)((ix->n_rows + 31) / 32) * tile_bytes;  // (<= both arrays: n_rows <= either capacity)
        ICREC_HIP(hipMemcpyAsync(out->frag, fs.frag, live, hipMemcpyDeviceToDevice, 0));
        ICREC_HIP(hipMemsetAsync(reinterpret_cast<char*>(out->frag) + live, 0, bytes - live, 0));
    } else if (fs.plane_hi) {
        const size_t bytes = (size_t)capacity * ix->dim * 2, live = (size_t)ix->n_rows * ix->dim * 2;
        if (hipMalloc(&out->plane_hi, bytes) != hipSuccess) out->plane_hi = nullptr;
        if (out->plane_hi == nullptr || hipMalloc(&out->plane_lo, bytes) != hipSuccess) {
            out->plane_lo = nullptr;
            set_error("icrec_index_reserve: hipMalloc of the filter planes (2 x %zu bytes) failed", bytes);
            return ICREC_ENOMEM;
        }
        ICREC_HIP(hipMemcpyAsync(out->plane_hi, fs.plane_hi, live, hipMemcpyDeviceToDevice, 0));
        ICREC_HIP(hipMemcpyAsync(out->plane_lo, fs.plane_lo, live, hipMemcpyDeviceToDevice, 0));
    }
    return ICREC_OK;
}

// icrec_index_export_filter: the fragments un-packed to row-major planes, one thread per (row, 8 k), from that chunk's slot (frag_slot).
__global__ __launch_bounds__(256) void unpack_rows_kernel(const _Float16* __restrict__ frag, int64_t n_rows, int K,
                                                          _Float16* __restrict__ hi, _Float16* __restrict__ lo) {
    const int chunks = K / 8;
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < n_rows * chunks; id += (int64_t)gridDim.x * 256) {
        const int64_t row = id / chunks;
        const int c = (int)(id % chunks);
        const _Float16* at = frag_slot(frag, row, c, K);
        *reinterpret_cast<half8*>(hi + row * K + 8 * c) = *reinterpret_cast<const half8*>(at);
        *reinterpret_cast<half8*>(lo + row * K + 8 * c) = *reinterpret_cast<const half8*>(at + WT_FRAG);
    }
}

int export_filter_storage(const Index* ix, uint16_t* hi_dev, uint16_t* lo_dev, hipStream_t st) {
    const int64_t n = ix->n_rows * ix->dim;
    if (ix->filter.frag) {
        const int64_t blocks = (n / 8 + 255) / 256;
        hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st,
                           (const _Float16*)ix->filter.frag, ix->n_rows, ix->dim, reinterpret_cast<_Float16*>(hi_dev),
                           reinterpret_cast<_Float16*>(lo_dev));
        ICREC_HIP(hipGetLastError());
    } else {
        ICREC_HIP(hipMemcpyAsync(hi_dev, ix->filter.plane_hi, (size_t)n * 2, hipMemcpyDeviceToDevice, st));
        ICREC_HIP(hipMemcpyAsync(lo_dev, ix->filter.plane_lo, (size_t)n * 2, hipMemcpyDeviceToDevice, st));
    }
    return ICREC_OK;
}

}  // namespace icrec
