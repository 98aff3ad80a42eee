// index.h — what an icrec_index handle points to, shared by index.hip (which creates, edits and destroys it),
// storage.hip (which writes, moves, clears, resizes and exports what it keeps per row; storage.h), search.hip (which
// searches it), sort.hip (icrec_rank_all), mmr.hip, boost.hip and compose.hip (which read its stored rows), cap.hip (which reads its
// facet words), and the device code that index.hip, storage.hip, search.hip and boost.hip share: the row normalisation
// kernel, the exclusion search, the facet test and the row set words.  What needs no handle - the shard row rule, the
// gathered exact-cosine tile that mmr.hip and boost.hip read the stored rows with - is in common.h.
#pragma once

#include <type_traits>

#include "common.h"

namespace icrec {

// The filter pass's copy of the rows of a *_FILTER storage, in one of two layouts (storage.h): both planes, or `frag`.
struct FilterStorage {
    _Float16 *plane_hi = nullptr, *plane_lo = nullptr;  // staged filter pass: row-major f16 hi/lo planes of `rows`
    _Float16* frag = nullptr;                           // resident filter pass (dim 384): frag_row_tiles(capacity) tiles of packed fragments
};

struct Index {
    void* rows = nullptr;  // normalised [n_rows, dim], fp32 or bf16 bits
    FilterStorage filter;
    int storage = ICREC_ROWS_F32;
    int64_t n_rows = 0;
    int64_t capacity = 0;          // rows every array is sized for (>= n_rows; == n_rows until icrec_index_reserve)
    int dim = 0;
    int64_t row_offset = 0;
    int device = 0;
    int n_cu = 256;
    int stream_max_q = 8;          // ICREC_STREAM_MAX_Q at creation
    uint16_t* facets = nullptr;    // icrec_index_set_facets: one word per row, zero padded to whole 256-row tiles of the capacity
    int n_facets = 0;
    uint32_t* rowsets = nullptr;   // icrec_index_set_rowsets: [n_rowsets][rowset_words(capacity)] bitmaps over the local rows
    int n_rowsets = 0;
    // icrec_index_append_rows / _remove_rows: what they copy to the device (facet words, the move plan) goes through this
    // pinned block, so that the copy is asynchronous; stage_event marks the end of the last copy out of it
    void* stage_host = nullptr;
    int32_t* plan_dev = nullptr;   // [2][plan_cap]: the moves' destinations, then their sources
    size_t stage_bytes = 0, plan_cap = 0;
    hipEvent_t stage_event = nullptr;
};

// Words of one row set on the device, for an index of that capacity: ceil(n_rows / 32) bitmap words, zero padded to whole 256-row tiles (8 words per
// tile, the widest tile any search kernel walks), as the facet words are: every tile of every kernel reads inside it.
static inline int64_t rowset_words(int64_t n_rows) { return (n_rows + 255) / 256 * 8; }
// Facet words of an index of that capacity: one per row, zero padded to the same whole 256-row tiles.
static inline int64_t facet_words(int64_t capacity) { return (capacity + 255) / 256 * 256; }

static inline bool rows_are_bf16(const Index* ix) { return ix->storage == ICREC_ROWS_BF16 || ix->storage == ICREC_ROWS_BF16_FILTER; }
// One stored value of `rows` in a kernel templated on "the rows are bf16": bf16 bits or a float.
template <bool P16>
using row_elem_t = std::conditional_t<P16, uint16_t, float>;

#ifdef __HIPCC__

// ---------------------------------------------------------------- a stored row by 16-byte pieces (compose.hip, adapt.hip)
__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// Feature j (0 .. P-1) of the 16 bytes a thread loaded from a stored row: a float, or bf16 bits widened exactly (word w
// holds feature 2w in its low half and 2w + 1 in its high half).
template <bool P16>
__device__ __forceinline__ float piece_value(const u32x4& x, int j) {
    if (P16) return (j & 1) ? bf16_hi(x[j >> 1]) : bf16_lo(x[j >> 1]);
    return __uint_as_float(x[j]);
}

// ---------------------------------------------------------------- row normalisation
// out = x / max(|x|_2, eps) — torch.nn.functional.normalize(p=2, dim=1) as cos_sim applies it.
// One wavefront per row; reduction order = 64 strided fmaf partials + xor butterfly, identical
// to oracle/icrec_oracle.c:wave_sum(mode 2).
// float -> bfloat16 bits, round to nearest even (inputs are finite: normalised rows)
__device__ __forceinline__ uint16_t bf16_rne(float v) {
    const unsigned u = __float_as_uint(v);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// tr_cols > 0 (fp32 only): write the result transposed, out[i * tr_cols + row] (n_out_rows == tr_cols) — the
// k-major query layout of stream_search_kernel.
template <bool OUT16>
__global__ __launch_bounds__(256) void normalize_rows_kernel(const float* __restrict__ x, void* __restrict__ outv,
                                                             int64_t n_rows, int64_t n_out_rows, int dim, float eps,
                                                             int tr_cols = 0) {
    float* out = static_cast<float*>(outv);
    uint16_t* out16 = static_cast<uint16_t*>(outv);
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_out_rows) return;
    if (row >= n_rows) {  // zero padding rows (query tiles are padded to the tile width)
        for (int i = lane; i < dim; i += 64) {
            if (OUT16) out16[row * dim + i] = 0;
            else if (tr_cols > 0) out[(int64_t)i * tr_cols + row] = 0.0f;
            else out[row * dim + i] = 0.0f;
        }
        return;
    }
    const float* xr = x + row * dim;
    float acc = 0.0f;
    for (int i = lane; i < dim; i += 64) {
        float v = xr[i];
        acc = fmaf(v, v, acc);
    }
    float nrm = sqrtf(wave_sum_f32(acc));
    float den = nrm > eps ? nrm : eps;
    for (int i = lane; i < dim; i += 64) {
        const float v = xr[i] / den;
        if (OUT16) out16[row * dim + i] = bf16_rne(v);
        else if (tr_cols > 0) out[(int64_t)i * tr_cols + row] = v;
        else out[row * dim + i] = v;
    }
}

// ---------------------------------------------------------------- exclusion lists and facets
// Is local row `row` in the sorted exclusion segment [lo, hi)?
__device__ __forceinline__ bool excluded(const int32_t* __restrict__ ex, int lo, int hi, int row) {
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        int v = ex[mid];
        if (v == row) return true;
        if (v < row) lo = mid + 1; else hi = mid;
    }
    return false;
}

// ---- facets (icrec_search_faceted): one or two attribute bytes per row against a 256-bit allow mask per query and
// facet.  A row is a candidate only if every facet's mask has the bit of the row's value; like an excluded row it is
// then never offered, so the lists, the merges and the verification see admitted rows only.
// The index keeps a row's bytes in ONE 16-bit word (facet 0 in the low byte; 0 for a facet it does not have), zero
// padded to whole 256-row tiles: every tile of every kernel reads inside the array.  A block keeps its queries' masks
// in LDS as [query][ICREC_MAX_FACETS][8] words: all ones for a facet the index does not have, zero for a padding
// query.  The FACET arm of a kernel is the instantiation whose parameter pack `Facet` holds one FacetArgs; with an
// empty pack the kernel's parameters and code are what they were before facets existed.
struct FacetArgs {
    const uint16_t* rows;   // [n_rows rounded up to 256] facet words
    const uint32_t* allow;  // [Q][n_facets][ICREC_FACET_MASK_WORDS], read when the kernel runs
    int n_facets;
};
constexpr int FACET_LDS_WORDS = ICREC_MAX_FACETS * ICREC_FACET_MASK_WORDS;  // per query
static_assert(ICREC_MAX_FACETS == 2 && ICREC_FACET_MASK_WORDS == 8, "a row's facets are the two bytes of a 16-bit word");

__device__ __forceinline__ FacetArgs facet_args() { return FacetArgs{nullptr, nullptr, 0}; }
__device__ __forceinline__ FacetArgs facet_args(const FacetArgs& fa) { return fa; }

// The masks of queries q0 .. q0 + nq - 1 -> LDS at am; the caller's next barrier publishes them.
__device__ __forceinline__ void facet_load_masks(uint32_t* am, const FacetArgs& fa, int q0, int nq, int Q, int tid,
                                                 int n_threads) {
    for (int i = tid; i < nq * FACET_LDS_WORDS; i += n_threads) {
        const int q = i / FACET_LDS_WORDS, f = i / ICREC_FACET_MASK_WORDS % ICREC_MAX_FACETS, w = i % ICREC_FACET_MASK_WORDS;
        am[i] = q0 + q >= Q      ? 0u
                : f < fa.n_facets ? fa.allow[((size_t)(q0 + q) * fa.n_facets + f) * ICREC_FACET_MASK_WORDS + w]
                                  : ~0u;
    }
}

// Does the mask of the block's query q (in LDS at am) admit a row whose facet word is fw?
__device__ __forceinline__ bool facet_admits(const uint32_t* am, int q, unsigned fw) {
    const unsigned v0 = fw & 255u, v1 = (fw >> 8) & 255u;
    const uint32_t* m = am + q * FACET_LDS_WORDS;
    return ((m[v0 >> 5] >> (v0 & 31)) & (m[ICREC_FACET_MASK_WORDS + (v1 >> 5)] >> (v1 & 31)) & 1u) != 0u;
}

// ---- row sets (icrec_search_in_sets): the index's bitmaps over its local rows, and up to ICREC_MAX_SETS_PER_QUERY set
// ids per query; a row is a candidate only if every slot of its query admits it.  The SETS arm of a kernel is the
// instantiation whose parameter pack holds one SetArgs; it applies the facet test as well (facet.allow == NULL: the
// masks it loads are all ones, facet.rows == NULL: every facet word reads as 0), so the FACET arm and the plain arm
// stay what they were before sets existed.  A block turns each of its queries' slots into SET_FREE (id < 0, or no such
// slot: constrains nothing), SET_NONE (id >= n_sets, or a padding query: admits no row; never used as an index) or
// the id, once; per tile it then ANDs the words of the query's sets into ONE word per (query, 32 rows) in LDS, and the
// per-candidate test is that word and a shift whatever per_query is.  The same id in two slots ANDs the same word twice.
struct SetArgs {
    FacetArgs facet;
    const uint32_t* bits;  // [n_sets][words], words = rowset_words(n_rows)
    const int32_t* ids;    // [Q][per_query], read when the kernel runs
    int n_sets, per_query;
    int64_t words;
};
static_assert(ICREC_MAX_SETS_PER_QUERY == 4, "a query's slots are one int4");
constexpr int SET_FREE = -1, SET_NONE = -2;

__device__ __forceinline__ FacetArgs facet_args(const SetArgs& sa) { return sa.facet; }
__device__ __forceinline__ SetArgs set_args() { return SetArgs{facet_args(), nullptr, nullptr, 0, 0, 0}; }
__device__ __forceinline__ SetArgs set_args(const FacetArgs&) { return set_args(); }
__device__ __forceinline__ SetArgs set_args(const SetArgs& sa) { return sa; }
template <class... A>
constexpr bool has_sets = (std::is_same_v<A, SetArgs> || ... || false);

// The four slots of query q (of Q), as SET_FREE, SET_NONE or a set id in [0, n_sets).
__device__ __forceinline__ int4 set_slots(const SetArgs& sa, int q, int Q) {
    int s[ICREC_MAX_SETS_PER_QUERY];
#pragma unroll
    for (int i = 0; i < ICREC_MAX_SETS_PER_QUERY; ++i) {
        s[i] = q >= Q ? SET_NONE : SET_FREE;
        if (q < Q && i < sa.per_query) {
            const int id = sa.ids[(size_t)q * sa.per_query + i];
            s[i] = id < 0 ? SET_FREE : id >= sa.n_sets ? SET_NONE : id;
        }
    }
    return make_int4(s[0], s[1], s[2], s[3]);
}

// Word gw (rows 32 gw .. 32 gw + 31) of the intersection of the sets in `slots`; gw < words.
__device__ __forceinline__ uint32_t set_word(const uint32_t* __restrict__ bits, int64_t words, const int4& slots, int64_t gw) {
    const int s[ICREC_MAX_SETS_PER_QUERY] = {slots.x, slots.y, slots.z, slots.w};
    uint32_t r = ~0u;
#pragma unroll
    for (int i = 0; i < ICREC_MAX_SETS_PER_QUERY; ++i) {
        if (s[i] == SET_NONE) r = 0u;
        else if (s[i] >= 0) r &= bits[(size_t)s[i] * words + gw];
    }
    return r;
}

#endif  // __HIPCC__

}  // namespace icrec
