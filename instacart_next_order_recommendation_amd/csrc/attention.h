// attention.h — what the encoder (encoder.hip) needs from the attention unit (attention.hip): the arguments of one
// layer's attention, the call that runs it - every length bucket, on the caller's stream and, for batches with a long
// bucket, beside it on a side stream - and the two decisions the caller acts on ahead of the layer loop: whether that
// side stream is wanted, and the dispatch order of the workgroups.  Kernels, buckets and launch order: attention.hip.
#pragma once

#include "common.h"

namespace icrec {

// Side stream + event of one caller stream (encoder.hip: side_for creates one per caller stream, never inside a
// capture).  Every fork and join records `ev` and waits on it at once (link), so one event serves them all.
struct SideStream {
    hipStream_t caller = nullptr, side = nullptr;
    hipEvent_t ev = nullptr;
};
// One fork or join: work enqueued on `to` from here on runs behind everything enqueued on `from` so far.
static inline hipError_t link(const SideStream* sd, hipStream_t from, hipStream_t to) {
    const hipError_t err = hipEventRecord(sd->ev, from);
    return err != hipSuccess ? err : hipStreamWaitEvent(to, sd->ev, 0);
}

// One layer's attention over a packed batch: softmax(Q.K^T / sqrt(head_dim) [+ bias]).V per (sequence, head).
struct AttentionArgs {
    const float* qkv;        // [total_tokens][3 * hidden] fp32 rows: Q | K | V
    const int32_t* cu;       // [n_seqs + 1] first row of every sequence
    int n_seqs, max_seqlen;  // (no sequence is longer than max_seqlen)
    int heads, hidden;       // head_dim = hidden / heads: 32 or 64
    // relative-position bias (icrec_encoder_set_attention_bias), or nullptr: [heads][BIAS_LD] floats in log2 units, entry
    // ICREC_MAX_SEQLEN - 1 + (key - query), the last one padding
    static constexpr int BIAS_LD = 2 * ICREC_MAX_SEQLEN;
    const float* bias;
    const int32_t* order;  // attention_dispatch_order's result (f16x3 arithmetic only), or nullptr: natural order
    // The context, [total_tokens][hidden], and with it the arithmetic: fp32 rows `ctx` (exact fp32 products), or with
    // ctx == nullptr the f16 hi / lo planes `ch` / `cl` (f16x3 products).
    float* ctx;
    _Float16 *ch, *cl;
    // f16x3: query block 0 of every (sequence, head) alone - all that the pruned last layer of an encoder reads; the very
    // bits a full launch gives those rows
    bool block0_only;
};

// Whether run_attention would use a side stream for these arguments: 32-dim heads (hidden 384), at least 64 sequences
// and a bucket beyond 128 tokens.  The caller creates the side stream ahead of its layer loop (and none inside a capture).
bool attention_wants_side(const AttentionArgs& a);

// Runs the attention on `st`.  With `sd` (a side stream of st's; only where attention_wants_side) the longest bucket and
// the 5-6-tile bucket run on `st` and the shorter ones beside them on sd->side, forked and joined by two links: on
// return everything is ordered behind `st` again.
int run_attention(const AttentionArgs& a, hipStream_t st, const SideStream* sd);

// order[0 .. n_seqs) <- the sequences by key-tile count, longest first, on `st`.  Whether to order at all is the
// caller's choice: without an order workgroup b serves sequence b / heads.
void attention_dispatch_order(const int32_t* cu, int n_seqs, int32_t* order, hipStream_t st);

}  // namespace icrec
