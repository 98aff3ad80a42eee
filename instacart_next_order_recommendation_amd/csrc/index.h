// index.h — what an icrec_index handle points to, shared by search.hip (which creates, searches and destroys it) and
// mmr.hip (which reads its stored rows).
#pragma once

#include "common.h"

namespace icrec {

struct Index {
    void* rows = nullptr;  // normalised [n_rows, dim], fp32 or bf16 bits
    _Float16* plane_hi = nullptr;  // ICREC_ROWS_F32_FILTER: f16 hi/lo planes of `rows` for the filter pass
    _Float16* plane_lo = nullptr;
    _Float16* frag = nullptr;      // resident filter pass (dim 384, <= RES_MAX_ROWS rows): the rows as packed fragments
    int64_t frag_row_tiles = 0;    // 32-row tiles in `frag` (whole rounds of CfgRes::BM rows)
    int storage = ICREC_ROWS_F32;
    int64_t n_rows = 0;
    int dim = 0;
    int64_t row_offset = 0;
    int device = 0;
    int n_cu = 256;
    int stream_max_q = 8;          // ICREC_STREAM_MAX_Q at creation
    uint16_t* facets = nullptr;    // icrec_index_set_facets: one word per row, zero padded to whole 256-row tiles
    int n_facets = 0;
};

static inline bool rows_are_bf16(const Index* ix) { return ix->storage == ICREC_ROWS_BF16 || ix->storage == ICREC_ROWS_BF16_FILTER; }

}  // namespace icrec
