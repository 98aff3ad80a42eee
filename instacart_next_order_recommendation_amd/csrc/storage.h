// storage.h — the filter copy an index keeps of its rows (index.h: FilterStorage): its two layouts, the ONE slot rule
// and the ONE conversion of every kernel that writes, moves, clears or un-packs it, and storage.hip's entry points.
// search.hip reads the layouts (staged pass: planes, resident pass: fragments) and splits its queries as the rows are.
#pragma once

#include "gemm_x3.h"
#include "index.h"
#include "wt_gemm.h"

namespace icrec {

// A *_FILTER storage (dim a multiple of FILTER_DIM_STEP: the staged pass walks whole slabs) keeps row-major f16 hi/lo
// planes or, at dim 16 * RES_KS, the resident pass's packed fragments in whole rounds of RES_ROUND_ROWS rows (same bytes).
constexpr int FILTER_DIM_STEP = 64;
constexpr int RES_KS = 24;           // k-steps of 16: the resident pass is built for dim = 384
constexpr int RES_ROUND_ROWS = 256;  // rows a block of the resident pass takes per round
enum FilterLayout { LAYOUT_NONE = 0, LAYOUT_PLANES = 1, LAYOUT_FRAGS = 2 };
static inline FilterLayout filter_layout(const Index* ix) {
    return ix->filter.frag ? LAYOUT_FRAGS : ix->filter.plane_hi ? LAYOUT_PLANES : LAYOUT_NONE;
}
// 32-row tiles in the fragment array of an index of that capacity
static inline int64_t frag_row_tiles(int64_t capacity) { return (capacity + RES_ROUND_ROWS - 1) / RES_ROUND_ROWS * (RES_ROUND_ROWS / 32); }

// storage.hip, for index.hip after its argument checks.  ICREC_ENOMEM or ICREC_EHIP with the error text set; the
// launches go to `st`, those of build and reserve (which allocate) to the null stream.
// icrec_index_create_ex: the filter copy of a new index, in the layout its dim and ICREC_FILTER_RESIDENT choose.
int build_filter_storage(Index* ix);
// icrec_index_write_rows (m >= 1): one launch of write_rows_kernel over rows row_ids_dev[0 .. m) or, with row_ids_dev ==
// NULL (icrec_index_append_rows), over rows base_row .. base_row + m - 1, tested against n_rows = base_row + m.
int write_index_rows(Index* ix, const float* rows_dev, const int32_t* row_ids_dev, int32_t m, int64_t base_row, hipStream_t st);
// icrec_index_remove_rows: everything kept per row moves src[i] -> dst[i] (device arrays of n_moves entries,
// dst < new_n <= src < old_n); then the fragment slots, facet words and row set bits of rows [new_n, old_n) are cleared.
int move_index_rows(Index* ix, const int32_t* dst_dev, const int32_t* src_dev, int32_t n_moves, int64_t new_n, int64_t old_n,
                    hipStream_t st);
// icrec_index_reserve: the handle's filter copy for `capacity` rows into *out, the live rows copied, zero behind them.
// The handle is not changed; after an error the caller frees *out.
int reserve_filter_storage(const Index* ix, int64_t capacity, FilterStorage* out);
// icrec_index_export_filter (the handle has a filter copy): that copy as row-major f16 bits [n_rows, dim] each.
int export_filter_storage(const Index* ix, uint16_t* hi_dev, uint16_t* lo_dev, hipStream_t st);
static inline void free_filter_storage(FilterStorage* fs) {  // (destroy, reserve's commit and its failure path)
    (void)hipFree(fs->plane_hi); (void)hipFree(fs->plane_lo); (void)hipFree(fs->frag);
    *fs = FilterStorage();
}

#ifdef __HIPCC__

// THE FRAGMENT LAYOUT.  The resident pass feeds v_mfma_f32_32x32x16_f16 its A operand straight from memory: fragment
// (32-row tile rt, k-step ks) is 2 * WT_FRAG halfs at (rt * dim / 16 + ks) * 2 * WT_FRAG, the hi plane and WT_FRAG
// behind it the lo plane; lane (h << 5 | r) of a plane holds the 8 halfs of row 32 rt + r at k = 16 ks + 8 h .. + 7.
// So chunk c = 2 ks + h (8 values) of a row has one slot, and frag_slot is the address of its hi part.  Rows past
// n_rows are zero.  (search.hip's r32_frag_off / r32_w_load read whole tiles: the same stride, lane * 8 inside a plane.)
template <class T>  // _Float16 or const _Float16
__device__ __forceinline__ T* frag_slot(T* frag, int64_t row, int c, int dim) {
    return frag + ((row >> 5) * (dim / 16) + (c >> 1)) * (2 * WT_FRAG) + (((c & 1) << 5) | (int)(row & 31)) * 8;
}

// THE CONVERSION of one stored value (bf16 rows: rounded and widened back, so that the filter approximates exactly what
// the exact pass computes): planes hi = f16(x), lo = f16((x - hi) * 2^11) (gemm_x3.h); fragments hi = f16(1024 x),
// lo = f16(1024 x - hi) (wt_gemm.h).
template <int LAYOUT>
__device__ __forceinline__ void filter_split(float v, _Float16& hi, _Float16& lo) {
    if (LAYOUT == LAYOUT_PLANES) split_f16(v, hi, lo);
    else split_scaled(v, WT_SW, hi, lo);
}

// fp32 values -> f16 hi/lo planes: the staged pass's queries per call (search.hip), the rows of a new index
// (storage.hip); clears the fallback flag if given.  SRC16: the source is bfloat16 bits, widened exactly first.
template <bool SRC16>
__global__ __launch_bounds__(256) void split_planes_kernel(const void* __restrict__ src, size_t n, _Float16* __restrict__ hi,
                                                           _Float16* __restrict__ lo, int* __restrict__ flag) {
    if (flag != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = SRC16 ? bf16_lo(static_cast<const uint16_t*>(src)[i]) : static_cast<const float*>(src)[i];
        _Float16 a, b;
        filter_split<LAYOUT_PLANES>(v, a, b);
        hi[i] = a;
        lo[i] = b;
    }
}

#endif  // __HIPCC__

}  // namespace icrec
