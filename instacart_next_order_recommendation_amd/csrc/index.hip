// index.hip — the life cycle of an icrec_index handle (index.h: struct Index): creation with row normalisation,
// facets, row sets, rows and facets rewritten in place, capacity reserved, rows appended and removed in place, export, the
// accessors and destruction; and icrec_normalize_rows.  It checks the arguments and owns the host side (facet words, row
// sets, the move plan); what the handle keeps per row on the device is written by storage.hip (storage.h).
#include <stdlib.h>

#include <new>
#include <vector>

#include "storage.h"

namespace icrec {

// Row i's facet word from the caller's n_facets (1 or 2) bytes per row: facet 0 in the low byte.
static inline uint16_t facet_word(const uint8_t* b, size_t i, int n_facets) { return n_facets == 1 ? b[i] : (uint16_t)(b[2 * i] | (b[2 * i + 1] << 8)); }

// m host row ids, ascending, unique, inside [0, n_rows); `fn`: the entry point, for the error text.
static int check_row_ids(const char* fn, const int32_t* ids, int32_t m, int64_t n_rows) {
    for (int32_t i = 0; i < m; ++i) {
        ICREC_REQUIRE(ids[i] >= 0 && ids[i] < n_rows, "%s: row %d is outside [0, %lld)", fn, ids[i], (long long)n_rows);
        ICREC_REQUIRE(i == 0 || ids[i] > ids[i - 1], "%s: the rows must be ascending and unique", fn);
    }
    return ICREC_OK;
}

// bf16 rows widened back to fp32 (icrec_index_export)
__global__ __launch_bounds__(256) void widen_bf16_kernel(const uint16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = bf16_lo(in[i]);
}

// Largest batch the streaming kernel takes (ICREC_STREAM_MAX_Q=0 disables it; tuning/diagnostic knob), read ONCE,
// when the index is created: a handle never changes its kernels between calls.
static int stream_max_q_from_env() {
    const char* e = getenv("ICREC_STREAM_MAX_Q");
    const int v = e ? atoi(e) : 8;
    return v > 8 ? 8 : v < 0 ? 0 : v;
}

// The index's pinned staging block, at least `bytes`, once the last asynchronous copy out of it has finished
// (icrec_index_append_rows' facet words, icrec_index_remove_rows' plan); NULL with the error text set.
static void* stage_block(Index* ix, size_t bytes) {
    if (ix->stage_event == nullptr && hipEventCreateWithFlags(&ix->stage_event, hipEventDisableTiming) != hipSuccess) {
        ix->stage_event = nullptr;
        set_error("hipEventCreate failed");
        return nullptr;
    }
    if (hipEventSynchronize(ix->stage_event) != hipSuccess) {
        set_error("hipEventSynchronize failed");
        return nullptr;
    }
    if (ix->stage_bytes < bytes) {
        (void)hipHostFree(ix->stage_host);
        ix->stage_host = nullptr;
        ix->stage_bytes = 0;
        if (hipHostMalloc(&ix->stage_host, bytes, hipHostMallocDefault) != hipSuccess) {
            ix->stage_host = nullptr;
            set_error("hipHostMalloc of %zu bytes failed", bytes);
            return nullptr;
        }
        ix->stage_bytes = bytes;
    }
    return ix->stage_host;
}

}  // namespace icrec

using namespace icrec;

extern "C" {

int icrec_index_create_ex(const float* rows_dev, int64_t n_rows, int32_t dim, int64_t row_offset, int device,
                          int32_t storage, icrec_index** out) {
    ICREC_REQUIRE(rows_dev && out, "icrec_index_create: NULL argument");
    ICREC_REQUIRE(n_rows >= 1, "icrec_index_create: n_rows must be >= 1");
    ICREC_REQUIRE(dim >= BK && dim % BK == 0 && dim <= 4096, "icrec_index_create: dim must be a multiple of %d (got %d)", BK, dim);
    ICREC_REQUIRE(row_offset >= 0 && row_offset + n_rows < 0xFFFFFFFFll, "icrec_index_create: row_offset + n_rows must be < 2^32-1");
    ICREC_REQUIRE(storage >= ICREC_ROWS_F32 && storage <= ICREC_ROWS_BF16_FILTER,
                  "icrec_index_create: storage must be one of ICREC_ROWS_F32 (0), _BF16 (1), _F32_FILTER (2), _BF16_FILTER (3), got %d", storage);
    const bool with_planes = storage == ICREC_ROWS_F32_FILTER || storage == ICREC_ROWS_BF16_FILTER;
    const bool rows16 = storage == ICREC_ROWS_BF16 || storage == ICREC_ROWS_BF16_FILTER;
    ICREC_REQUIRE(!with_planes || dim % FILTER_DIM_STEP == 0, "icrec_index_create: the filter planes need dim %% %d == 0 (got %d)",
                  FILTER_DIM_STEP, dim);
    // bf16 rows: the streaming kernel reads 128-byte slabs of 64 values, a final half slab would go unread
    ICREC_REQUIRE(!rows16 || dim % 64 == 0, "icrec_index_create: bf16 rows need dim %% 64 == 0 (got %d)", dim);
    ICREC_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    ICREC_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("icrec_index_create: device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
        return ICREC_ENODEV;
    }
    Index* ix = new Index();
    ix->n_rows = n_rows; ix->capacity = n_rows; ix->dim = dim; ix->row_offset = row_offset; ix->device = device; ix->storage = storage;
    ix->n_cu = prop.multiProcessorCount;
    ix->stream_max_q = stream_max_q_from_env();
    auto fail = [&]() {  // a hipMalloc failed: free what the index holds so far
        icrec_index_destroy(reinterpret_cast<icrec_index*>(ix));
        return ICREC_ENOMEM;
    };
    const size_t bytes = (size_t)n_rows * dim * (rows16 ? 2 : 4);
    hipError_t e = hipMalloc(&ix->rows, bytes);
    if (e != hipSuccess) {
        set_error("icrec_index_create: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        return fail();
    }
    hipLaunchKernelGGL((rows16 ? normalize_rows_kernel<true> : normalize_rows_kernel<false>), dim3((unsigned)((n_rows + 3) / 4)),
                       dim3(256), 0, 0, rows_dev, ix->rows, n_rows, n_rows, dim, 1e-12f, 0);
    ICREC_HIP(hipGetLastError());
    if (with_planes)
        if (int rc = build_filter_storage(ix)) return rc == ICREC_ENOMEM ? fail() : rc;
    ICREC_HIP(hipStreamSynchronize(0));
    *out = reinterpret_cast<icrec_index*>(ix);
    return ICREC_OK;
}

int icrec_index_create(const float* rows_dev, int64_t n_rows, int32_t dim, int64_t row_offset, int device,
                       icrec_index** out) {
    return icrec_index_create_ex(rows_dev, n_rows, dim, row_offset, device, ICREC_ROWS_F32, out);
}

int32_t icrec_index_storage(const icrec_index* h) { return h ? reinterpret_cast<const Index*>(h)->storage : -1; }
int32_t icrec_index_dim(const icrec_index* h) { return h ? reinterpret_cast<const Index*>(h)->dim : 0; }
int32_t icrec_index_device(const icrec_index* h) { return h ? reinterpret_cast<const Index*>(h)->device : -1; }

int icrec_index_destroy(icrec_index* h) {
    Index* ix = reinterpret_cast<Index*>(h);
    if (!ix) return ICREC_OK;
    (void)hipSetDevice(ix->device);
    (void)hipFree(ix->rows); (void)hipFree(ix->facets); (void)hipFree(ix->rowsets); (void)hipFree(ix->plan_dev);
    free_filter_storage(&ix->filter);
    (void)hipHostFree(ix->stage_host);
    if (ix->stage_event) (void)hipEventDestroy(ix->stage_event);
    delete ix;
    return ICREC_OK;
}

int icrec_index_set_facets(icrec_index* h, const uint8_t* facets_host, int32_t n_facets) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix, "icrec_index_set_facets: NULL index");
    ICREC_HIP(hipSetDevice(ix->device));
    if (facets_host == nullptr) {
        ICREC_HIP(hipFree(ix->facets));
        ix->facets = nullptr;
        ix->n_facets = 0;
        return ICREC_OK;
    }
    ICREC_REQUIRE(n_facets >= 1 && n_facets <= ICREC_MAX_FACETS, "icrec_index_set_facets: n_facets must be in [1, %d] (got %d)",
                  ICREC_MAX_FACETS, n_facets);
    // one word per row, zero padded to whole 256-row tiles (the widest tile any search kernel walks) of the capacity
    const size_t padded = (size_t)facet_words(ix->capacity);
    std::vector<uint16_t> words(padded, 0);
    for (int64_t i = 0; i < ix->n_rows; ++i) words[i] = facet_word(facets_host, (size_t)i, n_facets);
    uint16_t* dev = nullptr;
    if (hipMalloc(&dev, padded * 2) != hipSuccess) {
        set_error("icrec_index_set_facets: hipMalloc of %zu bytes failed", padded * 2);
        return ICREC_ENOMEM;
    }
    if (hipMemcpy(dev, words.data(), padded * 2, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev);
        set_error("icrec_index_set_facets: copying the facets to the device failed");
        return ICREC_EHIP;
    }
    (void)hipFree(ix->facets);
    ix->facets = dev;
    ix->n_facets = n_facets;
    return ICREC_OK;
}

int32_t icrec_index_facets(const icrec_index* h) { return h ? reinterpret_cast<const Index*>(h)->n_facets : -1; }

// One set's words as the device keeps them: the caller's ceil(n_rows / 32) words with the bits at or past n_rows
// cleared, zero padded to rowset_words(capacity).
static void pad_rowset(const Index* ix, const uint32_t* src, uint32_t* dst) {
    const int64_t w = (ix->n_rows + 31) / 32, padded = rowset_words(ix->capacity);
    for (int64_t i = 0; i < w; ++i) dst[i] = src[i];
    if (ix->n_rows % 32) dst[w - 1] &= (1u << (ix->n_rows % 32)) - 1u;
    for (int64_t i = w; i < padded; ++i) dst[i] = 0u;
}

int icrec_index_set_rowsets(icrec_index* h, const uint32_t* bits_host, int32_t n_sets) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix, "icrec_index_set_rowsets: NULL index");
    ICREC_HIP(hipSetDevice(ix->device));
    if (bits_host == nullptr) {
        ICREC_HIP(hipFree(ix->rowsets));
        ix->rowsets = nullptr;
        ix->n_rowsets = 0;
        return ICREC_OK;
    }
    ICREC_REQUIRE(n_sets >= 1 && n_sets <= ICREC_MAX_ROWSETS, "icrec_index_set_rowsets: n_sets must be in [1, %d] (got %d)",
                  ICREC_MAX_ROWSETS, n_sets);
    const size_t w = (size_t)((ix->n_rows + 31) / 32), padded = (size_t)rowset_words(ix->capacity);
    std::vector<uint32_t> words;
    try {
        words.resize(padded * n_sets);
    } catch (const std::bad_alloc&) {
        set_error("icrec_index_set_rowsets: no host memory for %zu bytes", padded * n_sets * 4);
        return ICREC_ENOMEM;
    }
    for (int32_t s = 0; s < n_sets; ++s) pad_rowset(ix, bits_host + s * w, words.data() + s * padded);
    uint32_t* dev = nullptr;
    if (hipMalloc(&dev, words.size() * 4) != hipSuccess) {
        set_error("icrec_index_set_rowsets: hipMalloc of %zu bytes failed", words.size() * 4);
        return ICREC_ENOMEM;
    }
    if (hipMemcpy(dev, words.data(), words.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev);
        set_error("icrec_index_set_rowsets: copying the row sets to the device failed");
        return ICREC_EHIP;
    }
    (void)hipFree(ix->rowsets);
    ix->rowsets = dev;
    ix->n_rowsets = n_sets;
    return ICREC_OK;
}

int icrec_index_write_rowset(icrec_index* h, int32_t set, const uint32_t* bits_host) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix && bits_host, "icrec_index_write_rowset: NULL argument");
    ICREC_REQUIRE(ix->rowsets != nullptr, "icrec_index_write_rowset: the index has no row sets");
    ICREC_REQUIRE(set >= 0 && set < ix->n_rowsets, "icrec_index_write_rowset: set must be in [0, %d) (got %d)", ix->n_rowsets, set);
    ICREC_HIP(hipSetDevice(ix->device));
    const size_t padded = (size_t)rowset_words(ix->capacity);
    std::vector<uint32_t> words(padded);
    pad_rowset(ix, bits_host, words.data());
    ICREC_HIP(hipMemcpy(ix->rowsets + (size_t)set * padded, words.data(), padded * 4, hipMemcpyHostToDevice));
    return ICREC_OK;
}

int32_t icrec_index_rowsets(const icrec_index* h) { return h ? reinterpret_cast<const Index*>(h)->n_rowsets : -1; }

int64_t icrec_index_rows(const icrec_index* h) { return h ? reinterpret_cast<const Index*>(h)->n_rows : 0; }
int64_t icrec_index_row_offset(const icrec_index* h) { return h ? reinterpret_cast<const Index*>(h)->row_offset : 0; }

int icrec_index_export(const icrec_index* h, float* rows_dev, void* stream) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    ICREC_REQUIRE(ix && rows_dev, "icrec_index_export: NULL argument");
    const int64_t n = ix->n_rows * ix->dim;
    if (rows_are_bf16(ix)) {
        ICREC_HIP(hipSetDevice(ix->device));
        hipLaunchKernelGGL(widen_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           static_cast<const uint16_t*>(ix->rows), rows_dev, n);
        ICREC_HIP(hipGetLastError());
    } else {
        ICREC_HIP(hipMemcpyAsync(rows_dev, ix->rows, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return ICREC_OK;
}

int icrec_index_write_rows(icrec_index* h, const float* rows_dev, const int32_t* row_ids_dev, int32_t m, void* stream) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix, "icrec_index_write_rows: NULL index");
    ICREC_REQUIRE(m >= 0, "icrec_index_write_rows: m must be >= 0 (got %d)", m);
    if (m == 0) return ICREC_OK;
    ICREC_REQUIRE(rows_dev && row_ids_dev, "icrec_index_write_rows: NULL argument");
    ICREC_HIP(hipSetDevice(ix->device));
    ScopedTimer tm(T_INDEX_WRITE, (hipStream_t)stream);
    return write_index_rows(ix, rows_dev, row_ids_dev, m, 0, (hipStream_t)stream);
}

int64_t icrec_index_capacity(const icrec_index* h) { return h ? reinterpret_cast<const Index*>(h)->capacity : 0; }

int icrec_index_reserve(icrec_index* h, int64_t capacity) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix, "icrec_index_reserve: NULL index");
    ICREC_REQUIRE(capacity >= ix->n_rows, "icrec_index_reserve: capacity %lld is below the index's %lld rows", (long long)capacity,
                  (long long)ix->n_rows);
    ICREC_REQUIRE(ix->row_offset + capacity < 0xFFFFFFFFll, "icrec_index_reserve: row_offset + capacity must be < 2^32-1");
    if (capacity == ix->capacity) return ICREC_OK;
    ICREC_HIP(hipSetDevice(ix->device));
    ICREC_HIP(hipDeviceSynchronize());  // whatever still reads or writes the old arrays, on any stream
    const size_t row_bytes = (size_t)ix->dim * (rows_are_bf16(ix) ? 2 : 4);
    const size_t n_facet_words = (size_t)facet_words(capacity);
    const size_t old_words = (size_t)rowset_words(ix->capacity), new_words = (size_t)rowset_words(capacity);
    void* rows = nullptr;
    uint16_t* facets = nullptr;
    uint32_t* rowsets = nullptr;
    FilterStorage fs;
    auto drop = [&](int rc) {  // the handle keeps its arrays: free the new ones
        (void)hipFree(rows); (void)hipFree(facets); (void)hipFree(rowsets);
        free_filter_storage(&fs);
        return rc;
    };
    if (hipMalloc(&rows, (size_t)capacity * row_bytes) != hipSuccess ||
        (ix->facets && hipMalloc(&facets, n_facet_words * 2) != hipSuccess) ||
        (ix->rowsets && hipMalloc(&rowsets, new_words * 4 * ix->n_rowsets) != hipSuccess)) {
        set_error("icrec_index_reserve: hipMalloc for %lld rows failed", (long long)capacity);
        return drop(ICREC_ENOMEM);
    }
    if (int rc = reserve_filter_storage(ix, capacity, &fs)) return drop(rc);
    hipError_t e = hipMemcpyAsync(rows, ix->rows, (size_t)ix->n_rows * row_bytes, hipMemcpyDeviceToDevice, 0);
    if (e == hipSuccess && facets) {  // the words past n_rows are zero in the old array too
        e = hipMemsetAsync(facets, 0, n_facet_words * 2, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(facets, ix->facets, (size_t)ix->n_rows * 2, hipMemcpyDeviceToDevice, 0);
    }
    if (e == hipSuccess && rowsets) {  // set by set: the stride changes; the live words of a set are a prefix of both strides
        e = hipMemsetAsync(rowsets, 0, new_words * 4 * ix->n_rowsets, 0);
        const size_t live = (size_t)((ix->n_rows + 31) / 32) * 4;
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(rowsets, new_words * 4, ix->rowsets, old_words * 4, live, (size_t)ix->n_rowsets,
                                 hipMemcpyDeviceToDevice, 0);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) {
        set_error("icrec_index_reserve: copying the index failed: %s", hipGetErrorString(e));
        return drop(ICREC_EHIP);
    }
    (void)hipFree(ix->rows); (void)hipFree(ix->facets); (void)hipFree(ix->rowsets);
    free_filter_storage(&ix->filter);
    ix->rows = rows; ix->facets = facets; ix->rowsets = rowsets; ix->filter = fs;
    ix->capacity = capacity;
    return ICREC_OK;
}

int icrec_index_append_rows(icrec_index* h, const float* rows_dev, int32_t m, const uint8_t* facets_host, void* stream) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix, "icrec_index_append_rows: NULL index");
    ICREC_REQUIRE(m >= 0, "icrec_index_append_rows: m must be >= 0 (got %d)", m);
    if (m == 0) return ICREC_OK;
    ICREC_REQUIRE(rows_dev, "icrec_index_append_rows: NULL argument");
    ICREC_REQUIRE(ix->n_rows + m <= ix->capacity, "icrec_index_append_rows: %lld + %d rows exceed the capacity %lld (icrec_index_reserve)",
                  (long long)ix->n_rows, m, (long long)ix->capacity);
    ICREC_REQUIRE(facets_host || !ix->facets, "icrec_index_append_rows: the index has facets, facets_host is required");
    ICREC_REQUIRE(!facets_host || ix->facets, "icrec_index_append_rows: facets_host on an index without facets");
    ICREC_HIP(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    if (ix->facets) {
        uint16_t* words = static_cast<uint16_t*>(stage_block(ix, (size_t)m * 2));
        if (words == nullptr) return ICREC_ENOMEM;
        for (int32_t i = 0; i < m; ++i) words[i] = facet_word(facets_host, (size_t)i, ix->n_facets);
        ICREC_HIP(hipMemcpyAsync(ix->facets + ix->n_rows, words, (size_t)m * 2, hipMemcpyHostToDevice, st));
        ICREC_HIP(hipEventRecord(ix->stage_event, st));
    }
    // the rows' bits of every row set are zero already: the new rows are members of no set
    if (int rc = write_index_rows(ix, rows_dev, nullptr, m, ix->n_rows, st)) return rc;
    ix->n_rows += m;
    return ICREC_OK;
}

int icrec_index_remove_rows(icrec_index* h, const int32_t* row_ids_host, int32_t m, int32_t* dst_out, int32_t* src_out,
                            int32_t* n_moves_out, void* stream) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix, "icrec_index_remove_rows: NULL index");
    ICREC_REQUIRE(m >= 0, "icrec_index_remove_rows: m must be >= 0 (got %d)", m);
    ICREC_REQUIRE(n_moves_out && (m == 0 || (row_ids_host && dst_out && src_out)), "icrec_index_remove_rows: NULL argument");
    ICREC_REQUIRE(m < ix->n_rows, "icrec_index_remove_rows: removing %d of %lld rows would leave the index empty", m,
                  (long long)ix->n_rows);
    if (int rc = check_row_ids("icrec_index_remove_rows", row_ids_host, m, ix->n_rows)) return rc;
    *n_moves_out = 0;
    if (m == 0) return ICREC_OK;
    // the plan: the holes (removed rows below new_n, ascending) take the survivors at or past new_n, ascending
    const int64_t old_n = ix->n_rows, new_n = old_n - m;
    int32_t n_moves = 0;
    while (n_moves < m && row_ids_host[n_moves] < new_n) ++n_moves;  // (ascending: the holes come first)
    ICREC_HIP(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    if (n_moves > 0) {
        int32_t* plan = static_cast<int32_t*>(stage_block(ix, (size_t)n_moves * 8));
        if (plan == nullptr) return ICREC_ENOMEM;
        if (ix->plan_cap < (size_t)n_moves) {
            ICREC_HIP(hipStreamSynchronize(st));  // an earlier removal on this stream may still read the old block
            (void)hipFree(ix->plan_dev);
            ix->plan_dev = nullptr;
            ix->plan_cap = 0;
            if (hipMalloc(&ix->plan_dev, (size_t)n_moves * 8) != hipSuccess) {
                ix->plan_dev = nullptr;
                set_error("icrec_index_remove_rows: hipMalloc of %zu bytes failed", (size_t)n_moves * 8);
                return ICREC_ENOMEM;
            }
            ix->plan_cap = (size_t)n_moves;
        }
        int32_t t = n_moves, i = 0;  // ids[t ..] are the removed rows of the tail
        for (int64_t row = new_n; i < n_moves; ++row) {
            if (t < m && row_ids_host[t] == row) { ++t; continue; }
            plan[i] = row_ids_host[i];
            plan[n_moves + i] = (int32_t)row;
            ++i;
        }
        ICREC_HIP(hipMemcpyAsync(ix->plan_dev, plan, (size_t)n_moves * 8, hipMemcpyHostToDevice, st));
        ICREC_HIP(hipEventRecord(ix->stage_event, st));
        memcpy(dst_out, plan, (size_t)n_moves * 4);
        memcpy(src_out, plan + n_moves, (size_t)n_moves * 4);
    }
    if (int rc = move_index_rows(ix, ix->plan_dev, ix->plan_dev + n_moves, n_moves, new_n, old_n, st)) return rc;
    ix->n_rows = new_n;
    *n_moves_out = n_moves;
    return ICREC_OK;
}

int icrec_index_write_facets(icrec_index* h, const int32_t* row_ids_host, const uint8_t* facets_host, int32_t m) {
    Index* ix = reinterpret_cast<Index*>(h);
    ICREC_REQUIRE(ix, "icrec_index_write_facets: NULL index");
    ICREC_REQUIRE(m >= 0, "icrec_index_write_facets: m must be >= 0 (got %d)", m);
    ICREC_REQUIRE(m == 0 || (row_ids_host && facets_host), "icrec_index_write_facets: NULL argument");
    ICREC_REQUIRE(ix->facets != nullptr, "icrec_index_write_facets: the index has no facets");
    if (int rc = check_row_ids("icrec_index_write_facets", row_ids_host, m, ix->n_rows)) return rc;
    if (m == 0) return ICREC_OK;
    ICREC_HIP(hipSetDevice(ix->device));
    // the words from the first named row to the last: down, patched, up again (a blocking copy each way)
    const int64_t first = row_ids_host[0], count = (int64_t)row_ids_host[m - 1] - first + 1;
    std::vector<uint16_t> words;
    try {
        words.resize((size_t)count);
    } catch (const std::bad_alloc&) {
        set_error("icrec_index_write_facets: no host memory for %zu bytes", (size_t)count * 2);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipMemcpy(words.data(), ix->facets + first, (size_t)count * 2, hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < m; ++i) words[row_ids_host[i] - first] = facet_word(facets_host, (size_t)i, ix->n_facets);
    ICREC_HIP(hipMemcpy(ix->facets + first, words.data(), (size_t)count * 2, hipMemcpyHostToDevice));
    return ICREC_OK;
}

int icrec_index_export_filter(const icrec_index* h, uint16_t* hi_dev, uint16_t* lo_dev, void* stream) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    ICREC_REQUIRE(ix && hi_dev && lo_dev, "icrec_index_export_filter: NULL argument");
    ICREC_REQUIRE(filter_layout(ix) != LAYOUT_NONE, "icrec_index_export_filter: the index's storage has no filter copy");
    ICREC_HIP(hipSetDevice(ix->device));
    return export_filter_storage(ix, hi_dev, lo_dev, (hipStream_t)stream);
}

int icrec_normalize_rows(const float* x_dev, float* out_dev, int64_t n_rows, int32_t dim, float eps, int device,
                         void* stream) {
    ICREC_REQUIRE(x_dev && out_dev && n_rows >= 1 && dim >= 1, "icrec_normalize_rows: bad argument");
    ICREC_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(normalize_rows_kernel<false>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       x_dev, (void*)out_dev, n_rows, n_rows, dim, eps);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
