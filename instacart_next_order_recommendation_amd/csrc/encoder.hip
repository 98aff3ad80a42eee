// encoder.hip — the encoder handle and its forward pass on gfx950: a post-LN BertModel of hidden 384 (32-dim heads) or
// 768 (64-dim heads) over token-packed (varlen) batches, in exact fp32 or in f16x3 arithmetic (gemm_mode), then mean or
// CLS pooling with L2 normalisation (icrec_encode_ex) or the pair score head (icrec_score_pairs).
// Here: the embedding, LayerNorm, fp32 GEMM, pooling, token-output, CLS-gather and score-head kernels; `Encoder`, its
// creation and setters; the workspace layout; the per-layer schedule of both arithmetics (encode_x3, encode_f32) and the
// one forward path (forward) behind the two public entries.  The f16x3 layer kernels are encoder_x3.h's.  Attention -
// its kernels, length buckets, launch order and stream split - is attention.hip's: this file fills an AttentionArgs per
// call and calls run_attention once per layer (attention.h).
//
// Replaces the device work of SentenceTransformer.encode as called at
//   /root/reference/src/inference/serve_recommendations.py:195-200 (catalog index build)
//   /root/reference/src/inference/serve_recommendations.py:213, :246 (per-request query)
// Arithmetic follows transformers/models/bert/modeling_bert.py (tf:) as cited per kernel,
// and oracle/icrec_oracle.c reduction orders where a kernel says "oracle order".
#include <stdlib.h>

#include <mutex>
#include <type_traits>
#include <vector>

#include "attention.h"
#include "wt_gemm.h"
#include "encoder_x3.h"

namespace icrec {

// ---------------------------------------------------------------- small helpers
__device__ __forceinline__ int find_seq(const int32_t* __restrict__ cu, int n_seqs, int t) {
    int lo = 0, hi = n_seqs;  // largest s with cu[s] <= t
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (cu[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// LayerNorm of one 384-wide row held 6 values per lane (element i = lane + 64*j); oracle order.
// SPLIT additionally writes the row as f16 hi/lo planes for the f16x3 GEMMs (wt_gemm.h: split_act).
template <int H, bool SPLIT>
__device__ __forceinline__ void ln_row(float (&v)[H / 64], const float* __restrict__ g, const float* __restrict__ b,
                                       float eps, float* __restrict__ out, _Float16* __restrict__ oh,
                                       _Float16* __restrict__ ol, int lane) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < H / 64; ++j) s = s + v[j];
    const float mean = wave_sum_f32(s) / (float)H;
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < H / 64; ++j) {
        float d = v[j] - mean;
        q = fmaf(d, d, q);
    }
    const float var = wave_sum_f32(q) / (float)H;
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int j = 0; j < H / 64; ++j) {
        const int i = lane + 64 * j;
        const float y = fmaf((v[j] - mean) * rstd, g[i], b[i]);
        if (SPLIT) {  // f16x3 mode: the residual stream exists only as its two planes
            _Float16 hi, lo;
            split_act(y, hi, lo);
            oh[i] = hi;
            ol[i] = lo;
        } else {
            out[i] = y;
        }
    }
}

// ---------------------------------------------------------------- K1: embeddings + LN (tf:98-107)
// SEG (icrec_score_pairs): sequence s is a pair whose second segment starts at position seg_b[s]; its tokens take type
// row 1 (token_type_ids: a run of 0s, then a run of 1s).  Positions lie in [0, len_s), so the comparison clamps
// seg_b[s] to [0, len_s] by itself.  Without SEG every token takes row 0 and seg_b is not read.
template <int H, bool SPLIT, bool SEG = false>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int32_t* __restrict__ ids,
                                                       const int32_t* __restrict__ cu, int n_seqs, int T,
                                                       const float* __restrict__ word, const float* __restrict__ pos,
                                                       const float* __restrict__ type, const float* __restrict__ g,
                                                       const float* __restrict__ b, float eps, int vocab, int max_pos,
                                                       float* __restrict__ x, _Float16* __restrict__ xh,
                                                       _Float16* __restrict__ xl,
                                                       const int32_t* __restrict__ seg_b) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const int s = find_seq(cu, n_seqs, t);
    int id = ids[t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int p = t - cu[s];
    if constexpr (SEG) type += p >= seg_b[s] ? H : 0;
    p = p >= max_pos ? max_pos - 1 : p;
    float v[H / 64];
#pragma unroll
    for (int j = 0; j < H / 64; ++j) {
        const int i = lane + 64 * j;
        v[j] = (word[(size_t)id * H + i] + type[i]) + pos[(size_t)p * H + i];
    }
    ln_row<H, SPLIT>(v, g, b, eps, x + (size_t)t * H, xh + (size_t)t * H, xl + (size_t)t * H, lane);
}

// ---------------------------------------------------------------- residual + LN (tf:292, tf:350)
// x <- LN(a + x); `a` already holds dense(.) + bias.  f32 mode only (f16x3: ln_wt_kernel and the fused kernels).
template <int H>
__global__ __launch_bounds__(256) void add_ln_kernel(const float* __restrict__ a, float* __restrict__ x, int T,
                                                     const float* __restrict__ g, const float* __restrict__ b,
                                                     float eps, _Float16* __restrict__ xh,
                                                     _Float16* __restrict__ xl) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    float v[H / 64];
#pragma unroll
    for (int j = 0; j < H / 64; ++j) {
        const int i = lane + 64 * j;
        v[j] = a[(size_t)t * H + i] + x[(size_t)t * H + i];
    }
    ln_row<H, false>(v, g, b, eps, x + (size_t)t * H, xh + (size_t)t * H, xl + (size_t)t * H, lane);
}

// ---------------------------------------------------------------- GEMM: out = A . W^T + bias [, GELU]
// torch.nn.Linear (tf:175-177 QKV, tf:290 attention output, tf:335 intermediate, tf:348 output).
// GELU is the exact erf form (tf:336, ACT2FN["gelu"]).
__device__ __forceinline__ float gelu_erf(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }

template <class Cfg, bool GELU>
__global__ __launch_bounds__(Cfg::THREADS, 2) void linear_kernel(const float* __restrict__ A, int M, int K,
                                                                 const float* __restrict__ W, int N,
                                                                 const float* __restrict__ bias,
                                                                 float* __restrict__ out, int n_tiles_n) {
    __shared__ __attribute__((aligned(16))) float smem[Cfg::LDS_FLOATS];
    float* As = smem;
    float* Bs = smem + Cfg::BM * LDK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = bid / n_tiles_n, nt = bid % n_tiles_n;  // tiles sharing an A row panel are neighbours
    const int64_t m0 = (int64_t)mt * Cfg::BM, n0 = (int64_t)nt * Cfg::BN;
    f32x16 acc[Cfg::TM][Cfg::TN];
    tile_gemm<Cfg>(acc, A, m0, M, W, n0, N, K, As, Bs);
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
        const int64_t col = n0 + (wn * Cfg::TN + j) * 32 + (lane & 31);
        const float bv = col < N ? bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t row = m0 + (wm * Cfg::TM + i) * 32 + acc_row(e, lane);
                if (row < M && col < N) {
                    float v = acc[i][j][e] + bv;
                    if (GELU) v = gelu_erf(v);
                    out[row * N + col] = v;
                }
            }
    }
}

// ---------------------------------------------------------------- pooling + L2 normalise
// sentence_transformers Pooling(mean): sum_t h_t / clamp(count, 1e-9), or Pooling(cls): h of the sequence's first
// token; then n_norm times x / max(|x|_2, 1e-12) (Normalize module, normalize_embeddings=True).  One workgroup of
// H threads per sequence; norm in oracle order by wave 0.
enum PoolRows { POOL_ROWS_MEAN, POOL_ROWS_CLS, POOL_ROWS_CLS_COMPACT };  // COMPACT: row s IS sequence s's first token

template <int H, bool PLANES>
__global__ __launch_bounds__(H) void pool_norm_kernel(const float* __restrict__ x, const _Float16* __restrict__ xh,
                                                      const _Float16* __restrict__ xl, const int32_t* __restrict__ cu,
                                                      int n_norm, float* __restrict__ out, int rows) {
    // PLANES (f16x3 mode): the hidden state is its two planes, h_t = (float(hi) + float(lo)) / 16 exactly
    auto at = [&](size_t idx) { return PLANES ? ((float)xh[idx] + (float)xl[idx]) * (1.0f / WT_SA) : x[idx]; };
    __shared__ float v[H];
    __shared__ float den_s;
    const int s = blockIdx.x, i = threadIdx.x;
    auto normalize = [&](float val) {  // (the branches that lead here are uniform over the workgroup)
        for (int rep = 0; rep < n_norm; ++rep) {
            v[i] = val;
            __syncthreads();
            if (i < 64) {
                float a = 0.0f;
#pragma unroll
                for (int j = 0; j < H / 64; ++j) a = fmaf(v[i + 64 * j], v[i + 64 * j], a);
                const float nrm = sqrtf(wave_sum_f32(a));
                if (i == 0) den_s = nrm > 1e-12f ? nrm : 1e-12f;
            }
            __syncthreads();
            val = val / den_s;
            __syncthreads();
        }
        out[(size_t)s * H + i] = val;
    };
    auto cls_pool = [&](int row) { normalize(at((size_t)row * H + i)); };
    if (rows == POOL_ROWS_CLS_COMPACT) return cls_pool(s);
    const int t0 = cu[s], t1 = cu[s + 1];
    if (rows == POOL_ROWS_CLS) return cls_pool(t0);
    float acc = 0.0f;
    int t = t0;
    for (; t + 8 <= t1; t += 8) {  // 8 independent loads in flight, summed in ascending token order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = at((size_t)(t + u) * H + i);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + v[u];
    }
    for (; t < t1; ++t) acc = acc + at((size_t)t * H + i);
    float cnt = (float)(t1 - t0);
    cnt = cnt < 1e-9f ? 1e-9f : cnt;
    normalize(acc / cnt);
}

// The last hidden state as fp32 rows (icrec_encode_ex's tokens_out): the very values pool_norm_kernel sums, read the
// same way.  One thread per 4 features; n4 = total_tokens * hidden / 4.
template <bool PLANES>
__global__ __launch_bounds__(256) void tokens_out_kernel(const float* __restrict__ x, const _Float16* __restrict__ xh,
                                                         const _Float16* __restrict__ xl, size_t n4,
                                                         float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v;
    if (PLANES) {
        const half4 hi = *reinterpret_cast<const half4*>(xh + 4 * i), lo = *reinterpret_cast<const half4*>(xl + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ((float)hi[j] + (float)lo[j]) * (1.0f / WT_SA);
    } else {
        v = *reinterpret_cast<const f32x4*>(x + 4 * i);
    }
    *reinterpret_cast<f32x4*>(out + 4 * i) = v;
}

// CLS pooling, pruned last layer: the context planes and the residual (x) planes of each sequence's first token, rows
// cu[s], -> compact [n_seqs, H] planes.  One thread per 8 features (16 bytes of a plane); h8 = H / 8.
__global__ __launch_bounds__(256) void gather_cls_rows_kernel(const _Float16* __restrict__ ch, const _Float16* __restrict__ cl,
                                                              const _Float16* __restrict__ xh, const _Float16* __restrict__ xl,
                                                              const int32_t* __restrict__ cu, int n_seqs, int h8,
                                                              _Float16* __restrict__ cch, _Float16* __restrict__ ccl,
                                                              _Float16* __restrict__ cxh, _Float16* __restrict__ cxl) {
    const int id = blockIdx.x * 256 + threadIdx.x;  // (n_seqs * h8 < 2^31: a workspace for 2^31 / 96 sequences exceeds HBM)
    const int s = id / h8;
    if (s >= n_seqs) return;
    const size_t from = ((size_t)cu[s] * h8 + id % h8) * 8, to = (size_t)id * 8;
    *reinterpret_cast<u32x4*>(cch + to) = *reinterpret_cast<const u32x4*>(ch + from);
    *reinterpret_cast<u32x4*>(ccl + to) = *reinterpret_cast<const u32x4*>(cl + from);
    *reinterpret_cast<u32x4*>(cxh + to) = *reinterpret_cast<const u32x4*>(xh + from);
    *reinterpret_cast<u32x4*>(cxl + to) = *reinterpret_cast<const u32x4*>(xl + from);
}

// ---------------------------------------------------------------- pair score head (icrec_score_pairs)
// BertPooler + classifier of BertForSequenceClassification(num_labels = 1) on the last hidden state h of each sequence's
// first token:  p_j = tanhf(bp[j] + sum_k Wp[j][k] h[k]),  logit = bc + sum_j wc[j] p_j  - every sum ONE fp32 fmaf chain in
// ascending index order, so a pair's logit has the same bits alone, in any batch and from any of the three row sources:
// the x planes (row cu[s]; widened as pool_norm_kernel widens them), the compact rows of the pruned last layer (row s),
// or fp32 x (row cu[s]).
// A workgroup of 384 threads serves HEAD_SEQS sequences: their rows in LDS as hs[k][seq] (one k = HEAD_SEQS contiguous
// floats, read as broadcast 16-byte loads), thread t the outputs j = t (+ 384 at hidden 768) with one accumulator per
// (j, sequence), so that a k-step's weights - wpt is Wp transposed, [in][out]: a wave reads 256 contiguous bytes - are
// fetched from L2 once per HEAD_SEQS sequences, not once per sequence.  Then p in LDS as ps[j][seq] (over hs) and thread
// s < HEAD_SEQS walks sequence s's classifier chain (conflict-free: adjacent lanes, adjacent banks).
template <int H>
constexpr int HEAD_SEQS = 32 * 384 / H;  // 48 KB of rows in LDS, 32 accumulators per thread, at either width

template <int H, bool PLANES>
__global__ __launch_bounds__(384) void score_head_kernel(const float* __restrict__ x, const _Float16* __restrict__ xh,
                                                         const _Float16* __restrict__ xl, const int32_t* __restrict__ cu,
                                                         int n_seqs, bool compact, const float* __restrict__ wpt,
                                                         const float* __restrict__ bp, const float* __restrict__ wc,
                                                         const float* __restrict__ bc, float* __restrict__ scores) {
    constexpr int S = HEAD_SEQS<H>, JPT = H / 384;
    auto at = [&](size_t idx) { return PLANES ? ((float)xh[idx] + (float)xl[idx]) * (1.0f / WT_SA) : x[idx]; };
    __shared__ __attribute__((aligned(16))) float hs[H * S];
    const int tid = threadIdx.x, s0 = blockIdx.x * S;
    for (int i = tid; i < H * S; i += 384) {  // (consecutive threads, consecutive features of one row)
        const int sl = i / H, k = i % H, s = s0 + sl;
        hs[k * S + sl] = s < n_seqs ? at((size_t)(compact ? s : cu[s]) * H + k) : 0.0f;
    }
    __syncthreads();
    float acc[JPT][S];
#pragma unroll
    for (int r = 0; r < JPT; ++r)
#pragma unroll
        for (int sl = 0; sl < S; ++sl) acc[r][sl] = bp[tid + 384 * r];
#pragma unroll 4
    for (int k = 0; k < H; ++k) {
        float w[JPT];
#pragma unroll
        for (int r = 0; r < JPT; ++r) w[r] = wpt[(size_t)k * H + tid + 384 * r];
#pragma unroll
        for (int q = 0; q < S / 4; ++q) {
            const f32x4 h4 = *reinterpret_cast<const f32x4*>(hs + k * S + 4 * q);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < JPT; ++r) acc[r][4 * q + u] = fmaf(w[r], h4[u], acc[r][4 * q + u]);
        }
    }
    __syncthreads();  // every thread is done with hs: ps takes its place
    float* const ps = hs;
#pragma unroll
    for (int r = 0; r < JPT; ++r)
#pragma unroll
        for (int sl = 0; sl < S; ++sl) ps[(tid + 384 * r) * S + sl] = tanhf(acc[r][sl]);
    __syncthreads();
    if (tid < S && s0 + tid < n_seqs) {
        float logit = bc[0];
        for (int j = 0; j < H; ++j) logit = fmaf(wc[j], ps[j * S + tid], logit);
        scores[s0 + tid] = logit;
    }
}

// ---------------------------------------------------------------- host side
constexpr int HID = 384;     // all-MiniLM width: 32-dim heads, the fused layer kernels
constexpr int HID_BASE = 768;  // BERT-base width: 64-dim heads, the unfused chain
// f(h) with the hidden size (HID or HID_BASE: icrec_encoder_create admits no other) as the compile-time constant h()
template <class F>
static auto for_hidden(int hidden, F f) {
    return hidden == HID_BASE ? f(std::integral_constant<int, HID_BASE>{}) : f(std::integral_constant<int, HID>{});
}

struct LayerW {
    float *Wqkv, *bqkv, *Wo, *bo, *g1, *b1n, *W1, *b1, *W2, *b2, *g2, *b2n;
    // the four weight matrices as packed f16 hi/lo fragments (wt_gemm.h; gemm_mode F16X3 only)
    _Float16 *Wqkv_p, *Wo_p, *W1_p, *W2_p;
};
struct Encoder {
    icrec_bert_cfg cfg;
    int device = 0;
    int n_cu = 256;
    int max_seqlen = 256;       // longest sequence icrec_encode accepts (icrec_encoder_set_max_seqlen)
    int pooling = ICREC_POOL_MEAN;  // icrec_encoder_set_pooling
    float* att_bias = nullptr;  // icrec_encoder_set_attention_bias: AttentionArgs::bias, or none
    float* score_head = nullptr;  // icrec_encoder_set_score_head: Wp^T [H in][H out], bp[H], wc[H], bc[1], or none
    float* blob = nullptr;      // the uploaded weight blob
    float* extra = nullptr;     // repacked Wqkv / bqkv
    _Float16* planes = nullptr; // packed weight fragments (F16X3)
    float *word, *pos, *type, *eg, *eb;
    LayerW layers[64];
    // A/B switches, read from the environment ONCE, at icrec_encoder_create (never on the hot path; a test that wants
    // the other form creates a second encoder under the other setting):
    //   ICREC_FUSE=0         the UNFUSED reference chain for batches: slab-ring QKV, attention-out GEMM + LayerNorm,
    //                        FFN-up, FFN-down + LayerNorm as separate launches in natural sequence order (same bits)
    //   ICREC_SIDE_STREAM=0  every kernel on the caller's stream (no side stream for the batch remainder / short buckets)
    //   ICREC_CLS_PRUNE=0    a CLS-pooled f16x3 encoder runs its last layer over every token, like a mean-pooled one,
    //                        instead of over each sequence's first token only (same bits)
    bool fuse = true, side_stream = true, cls_prune = true;
    //   ICREC_SMALL_M=n      token count up to which a call takes the latency-form kernels (32-token x 64-feature
    //                        workgroups, every GEMM a launch of its own) instead of the layer kernel (one 64-token workgroup
    //                        per CU).  Round 4: 3,584 - measured crossover ~4,000 tokens (tools/small_m_sweep.py: 897 tokens
    //                        0.39 ms against 0.79, 2,900 tokens 0.74 against 0.86, 4,485 tokens 0.86 against 0.82); rounds 1-3: 512
    int small_m = 3584;
    //   ICREC_TAIL_M=n       a batch's remainder (tokens beyond whole rounds of one 64-token workgroup per CU) of up to n tokens
    //                        goes through the latency-form kernels on the side stream instead of a partial round (which
    //                        costs every layer kernel ~0.1 ms: +0.57 ms per step).  Round 4: 2,560 - measured on 1,030- /
    //                        1,040- / 1,050-context batches (remainders 650 / 1,839 / 3,117 tokens): 9.83 -> 9.35 ms, 9.86 -> 9.60,
    //                        9.89 -> 9.91 (tools/tail_sweep.sh, profiles/r04_small_m_sweep.txt); rounds 2-3: 512
    int tail_m = 2560;
    // Both are clamped at creation: small_m to [0, SMALL_M_MAX], tail_m to [0, 64 * n_cu - 1] (a remainder is shorter
    // than one round by definition, so a larger value changes nothing).  Every combination is supported and gives the
    // same bits; with tail_m > small_m a remainder longer than small_m takes the layer kernels (activation-resident QKV,
    // fused layer kernel) on the side stream instead of the latency form.
    // Side stream + event of one caller stream (attention.h: SideStream, link): the short remainder of a large batch
    // (batch_tail) and the shorter attention buckets run beside the batch kernels of the same layer instead of behind
    // them.  One set per caller stream (created on first use, kept for the encoder's life), so that concurrent
    // icrec_encode calls on different streams - DeviceEncoder runs the two halves of a batch that way - do not queue
    // behind each other's side work.
    std::mutex side_mu;
    std::vector<SideStream*> sides;
};

static int side_for(Encoder* e, hipStream_t caller, SideStream** out) {
    std::lock_guard<std::mutex> lock(e->side_mu);
    *out = nullptr;
    for (SideStream* sd : e->sides)
        if (sd->caller == caller) { *out = sd; return ICREC_OK; }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (caller && hipStreamIsCapturing(caller, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return ICREC_OK;  // no stream / event creation inside a capture: the call stays on the caller's stream
    SideStream* sd = new SideStream();
    sd->caller = caller;
    ICREC_HIP(hipStreamCreateWithFlags(&sd->side, hipStreamNonBlocking));
    ICREC_HIP(hipEventCreateWithFlags(&sd->ev, hipEventDisableTiming));
    e->sides.push_back(sd);
    *out = sd;
    return ICREC_OK;
}

static size_t weight_count(const icrec_bert_cfg* c) {
    const size_t H = c->hidden, I = c->intermediate;
    const size_t emb = (size_t)c->vocab_size * H + (size_t)c->max_position * H + (size_t)c->type_vocab * H + 2 * H;
    const size_t per = 4 * (H * H + H) + 2 * H + (I * H + I) + (H * I + H) + 2 * H;
    return emb + per * c->layers;
}

struct EncWs {
    size_t x, xs, qkv, ctx, t1, h, total;
};
// post_only: the regions the post-attention chain of T rows works in (no fp32 x, no QKV rows)
static EncWs enc_ws(const icrec_bert_cfg& c, int64_t T, bool post_only = false) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    EncWs w;
    size_t o = 0;
    w.x = o;   o += post_only ? 0 : al((size_t)T * c.hidden * 4);
    w.xs = o;  o += al((size_t)T * c.hidden * 4);        // x as f16 hi/lo planes (F16X3)
    w.qkv = o; o += post_only ? 0 : al((size_t)T * 3 * c.hidden * 4);
    w.ctx = o; o += al((size_t)T * c.hidden * 4);        // fp32 ctx, or its two f16 planes
    w.t1 = o;  o += al((size_t)T * c.hidden * 4);
    w.h = o;   o += al((size_t)T * c.intermediate * 4);  // fp32 h, or its two f16 planes
    w.total = o;
    return w;
}

// The workspace regions of a call (enc_ws): x, ctx and h also as f16 hi/lo planes, the ctx / h planes in their place.
struct EncBufs {
    float *x, *qkv, *ctx, *t1, *h;
    _Float16 *xh, *xl, *ch, *cl, *hh, *hl;
    EncBufs(char* base, const EncWs& w, const icrec_bert_cfg& c, size_t T)
        : x(reinterpret_cast<float*>(base + w.x)), qkv(reinterpret_cast<float*>(base + w.qkv)),
          ctx(reinterpret_cast<float*>(base + w.ctx)), t1(reinterpret_cast<float*>(base + w.t1)),
          h(reinterpret_cast<float*>(base + w.h)), xh(reinterpret_cast<_Float16*>(base + w.xs)), xl(xh + T * c.hidden),
          ch(reinterpret_cast<_Float16*>(ctx)), cl(ch + T * c.hidden), hh(reinterpret_cast<_Float16*>(h)),
          hl(hh + T * c.intermediate) {}
};

// An f16x3 encoder whose caller reads row cu[s] of the last hidden state and nothing else runs its last layer's attention
// for query block 0 of each (sequence, head) and the post-attention chain over n_seqs compact rows (encode_x3), which
// take their scratch from the caller's workspace behind the call's own regions.  A pair's score reads those rows
// whatever the handle's pooling mode; an embedding does under CLS pooling only (pooled: the pooling mode matters).
static bool prunes_last_layer(const Encoder* e, bool pooled) {
    return (!pooled || e->pooling == ICREC_POOL_CLS) && e->cls_prune && e->cfg.gemm_mode == ICREC_GEMM_F16X3;
}

typedef TileCfg<2, 2, 2, 2> GemmBig;  // 128 x 128 output tile, 4 waves
constexpr long long SMALL_M_MAX = 1 << 20;  // ICREC_SMALL_M above this: every call of up to 2^20 tokens takes the latency form

// A non-negative integer knob from the environment, clamped to [0, hi]; `fallback` when unset or not a number.
static int env_knob(const char* name, int fallback, long long hi) {
    const char* s = getenv(name);
    if (!s) return fallback;
    char* end = nullptr;
    const long long v = strtoll(s, &end, 10);
    if (end == s) return fallback;
    return (int)(v < 0 ? 0 : v > hi ? hi : v);
}
// An on/off switch from the environment: on unless its value starts with '0'.
static bool env_switch(const char* name) {
    const char* s = getenv(name);
    return !(s && s[0] == '0');
}

template <bool GELU>
static void launch_linear(const float* A, int M, int K, const float* W, int N, const float* bias, float* out,
                          hipStream_t st) {
    const int mt = (M + GemmBig::BM - 1) / GemmBig::BM, nt = (N + GemmBig::BN - 1) / GemmBig::BN;
    hipLaunchKernelGGL((linear_kernel<GemmBig, GELU>), dim3(mt * nt), dim3(GemmBig::THREADS), 0, st, A, M, K, W, N,
                       bias, out, nt);
}

// f16x3 linear layer through the weights-direct engine.  Single requests / micro-batches (`small`: up to small_m tokens)
// are latency-bound - a handful of workgroups, each walking its K loop at the rate ONE CU's vector L1 pulls fragments
// from L2: they use 32-token x 64-feature workgroups, one 16-feature tile per wave (wt_linear_half_kernel; EPI 1 keeps
// the 32 x 128 form: its small-batch consumer is wt_linear_lnin_kernel), as many workgroups as the shape allows; batches
// use 64-token x 384-feature blocks (3 x 2 tiles per wave).  Per-output arithmetic is the same chain in all of them, so a
// request encodes to the same bits either way.
template <int EPI>
static void launch_wt_linear(const _Float16* Xh, const _Float16* Xl, int T, int K, const _Float16* Wp, int N,
                             const float* bias, float* out, _Float16* oh, _Float16* ol, hipStream_t st, bool small) {
    if (small) {
        if constexpr (EPI == 0 || EPI == 2) {  // 16-feature tiles per wave, twice the workgroups (wt_linear_half_kernel)
            const int nbn = N / 64;
            // FFN-down: weights eight k-steps ahead; K = 384 (or another multiple of 384): six k-steps ahead
            auto kern = K % 256 == 0 && K >= 1024 ? wt_linear_half_kernel<EPI, 8> : wt_linear_half_kernel<EPI, 6>;
            hipLaunchKernelGGL(kern, dim3(((T + 31) / 32) * nbn), dim3(256), 0, st, Xh, Xl, T, K, Wp, N, bias, out,
                               (const _Float16*)oh, (const _Float16*)ol, nbn);
        } else {
            const int nbn = N / 128;
            hipLaunchKernelGGL((wt_linear_kernel<1, 1, 4, EPI>), dim3(((T + 31) / 32) * nbn), dim3(256), 0, st, Xh, Xl, T, K,
                               Wp, N, bias, out, oh, ol, nbn);
        }
    } else {
        const int nbn = N / 384;
        auto kern = wt_linear_kernel<3, 2, 1, EPI>;
        // the residual epilogue reads residual rows of N = hidden features
        if constexpr (EPI == 2) kern = for_hidden(N, [](auto h) { return wt_linear_kernel<3, 2, 1, 2, h()>; });
        hipLaunchKernelGGL(kern, dim3(((T + 63) / 64) * nbn), dim3(256), 0, st, Xh, Xl, T, K, Wp, N, bias, out, oh, ol,
                           nbn);
    }
}

}  // namespace icrec

using namespace icrec;

extern "C" {

size_t icrec_encoder_weight_count(const icrec_bert_cfg* cfg) { return cfg ? weight_count(cfg) : 0; }

int icrec_encoder_create(const float* weights_host, size_t n_floats, const icrec_bert_cfg* cfg, int device,
                         icrec_encoder** out) {
    ICREC_REQUIRE(weights_host && cfg && out, "icrec_encoder_create: NULL argument");
    // The kernels and their dispatch rely on these: every GEMM has K = hidden or K = intermediate, a multiple of 384, and
    // N = hidden, 3 x hidden or intermediate (launch_wt_linear's ring depths and tile splits, the fused FFN's 128-wide
    // chunks); the attention kernels exist for 32-dim heads at hidden 384 and 64-dim heads at hidden 768.
    ICREC_REQUIRE((cfg->hidden == HID && cfg->heads * 32 == HID) || (cfg->hidden == HID_BASE && cfg->heads * 64 == HID_BASE),
                  "icrec_encoder_create: (hidden, heads) must be (384, 12) or (768, 12): head_dim 32 at hidden 384, head_dim 64 "
                  "at hidden 768 (got hidden=%d, heads=%d)", cfg->hidden, cfg->heads);
    ICREC_REQUIRE(cfg->intermediate >= 384 && cfg->intermediate % 384 == 0, "icrec_encoder_create: intermediate size must be a multiple of 384 (got %d)", cfg->intermediate);
    ICREC_REQUIRE(cfg->layers >= 1 && cfg->layers <= 64, "icrec_encoder_create: layers must be in [1,64]");
    ICREC_REQUIRE(cfg->vocab_size >= 1 && cfg->max_position >= 1 && cfg->type_vocab >= 1, "icrec_encoder_create: bad vocab/position sizes");
    ICREC_REQUIRE(cfg->n_normalize >= 0 && cfg->n_normalize <= 4, "icrec_encoder_create: n_normalize must be in [0,4]");
    ICREC_REQUIRE(cfg->gemm_mode == ICREC_GEMM_F32 || cfg->gemm_mode == ICREC_GEMM_F16X3, "icrec_encoder_create: unknown gemm_mode %d", cfg->gemm_mode);
    ICREC_REQUIRE(n_floats == weight_count(cfg), "icrec_encoder_create: weight blob has %zu floats, expected %zu", n_floats, weight_count(cfg));
    ICREC_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    ICREC_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("icrec_encoder_create: device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
        return ICREC_ENODEV;
    }
    Encoder* e = new Encoder();
    e->cfg = *cfg;
    e->device = device;
    e->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    e->max_seqlen = cfg->max_position < 256 ? cfg->max_position : 256;
    e->fuse = env_switch("ICREC_FUSE");
    e->side_stream = env_switch("ICREC_SIDE_STREAM");
    e->cls_prune = env_switch("ICREC_CLS_PRUNE");
    e->small_m = env_knob("ICREC_SMALL_M", e->small_m, SMALL_M_MAX);
    e->tail_m = env_knob("ICREC_TAIL_M", e->tail_m, 64LL * e->n_cu - 1);
    const size_t H = cfg->hidden, I = cfg->intermediate;
    const size_t mat_per_layer = 3 * H * H + H * H + I * H + H * I;
    const bool x3 = cfg->gemm_mode == ICREC_GEMM_F16X3;
    if (hipMalloc(&e->blob, n_floats * 4) != hipSuccess ||
        hipMalloc(&e->extra, (size_t)cfg->layers * (3 * H * H + 3 * H) * 4) != hipSuccess ||
        (x3 && hipMalloc(&e->planes, (size_t)cfg->layers * mat_per_layer * 2 * sizeof(_Float16)) != hipSuccess)) {
        set_error("icrec_encoder_create: hipMalloc failed");
        if (e->blob) (void)hipFree(e->blob);
        if (e->extra) (void)hipFree(e->extra);
        delete e;
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipMemcpy(e->blob, weights_host, n_floats * 4, hipMemcpyHostToDevice));
    float* p = e->blob;
    e->word = p; p += (size_t)cfg->vocab_size * H;
    e->pos = p;  p += (size_t)cfg->max_position * H;
    e->type = p; p += (size_t)cfg->type_vocab * H;
    e->eg = p;   p += H;
    e->eb = p;   p += H;
    float* x = e->extra;
    _Float16* pl = e->planes;
    auto pack = [&](const float* w, int N, int K, _Float16*& out) {  // [N, K] fp32 -> packed hi/lo fragments
        out = pl;
        pl += (size_t)2 * N * K;
        hipLaunchKernelGGL(pack_weights_kernel, dim3(1024), dim3(256), 0, 0, w, N, K, out);
    };
    for (int l = 0; l < cfg->layers; ++l) {
        LayerW& L = e->layers[l];
        L.Wqkv = x; x += 3 * H * H;
        L.bqkv = x; x += 3 * H;
        for (int part = 0; part < 3; ++part) {  // Wq,bq | Wk,bk | Wv,bv are interleaved in the blob
            ICREC_HIP(hipMemcpy(L.Wqkv + part * H * H, p, H * H * 4, hipMemcpyDeviceToDevice)); p += H * H;
            ICREC_HIP(hipMemcpy(L.bqkv + part * H, p, H * 4, hipMemcpyDeviceToDevice)); p += H;
        }
        L.Wo = p; p += H * H; L.bo = p; p += H;
        L.g1 = p; p += H; L.b1n = p; p += H;
        L.W1 = p; p += I * H; L.b1 = p; p += I;
        L.W2 = p; p += H * I; L.b2 = p; p += H;
        L.g2 = p; p += H; L.b2n = p; p += H;
        if (x3) {
            pack(L.Wqkv, (int)(3 * H), (int)H, L.Wqkv_p);
            pack(L.Wo, (int)H, (int)H, L.Wo_p);
            pack(L.W1, (int)I, (int)H, L.W1_p);
            pack(L.W2, (int)H, (int)I, L.W2_p);
        }
    }
    ICREC_HIP(hipGetLastError());
    ICREC_HIP(hipDeviceSynchronize());
    *out = reinterpret_cast<icrec_encoder*>(e);
    return ICREC_OK;
}

int icrec_encoder_destroy(icrec_encoder* h) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    if (!e) return ICREC_OK;
    (void)hipSetDevice(e->device);
    (void)hipFree(e->blob);
    (void)hipFree(e->extra);
    if (e->planes) (void)hipFree(e->planes);
    if (e->att_bias) (void)hipFree(e->att_bias);
    if (e->score_head) (void)hipFree(e->score_head);
    for (SideStream* sd : e->sides) {  // (side_for keeps a side only once its stream and event exist)
        (void)hipStreamSynchronize(sd->side);
        (void)hipStreamDestroy(sd->side);
        (void)hipEventDestroy(sd->ev);
        delete sd;
    }
    delete e;
    return ICREC_OK;
}

int icrec_encoder_set_max_seqlen(icrec_encoder* h, int32_t max_seqlen) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    ICREC_REQUIRE(e, "icrec_encoder_set_max_seqlen: NULL encoder");
    const int hi = e->cfg.max_position < ICREC_MAX_SEQLEN ? e->cfg.max_position : ICREC_MAX_SEQLEN;
    ICREC_REQUIRE(max_seqlen >= 1 && max_seqlen <= hi, "icrec_encoder_set_max_seqlen: max_seqlen must be in [1, %d] (got %d)", hi, max_seqlen);
    e->max_seqlen = max_seqlen;
    return ICREC_OK;
}

int icrec_encoder_set_pooling(icrec_encoder* h, int32_t mode) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    ICREC_REQUIRE(e, "icrec_encoder_set_pooling: NULL encoder");
    ICREC_REQUIRE(mode == ICREC_POOL_MEAN || mode == ICREC_POOL_CLS, "icrec_encoder_set_pooling: mode must be ICREC_POOL_MEAN (0) or ICREC_POOL_CLS (1) (got %d)", mode);
    e->pooling = mode;
    return ICREC_OK;
}

int32_t icrec_encoder_pooling(const icrec_encoder* h) {
    const Encoder* e = reinterpret_cast<const Encoder*>(h);
    return e ? e->pooling : -1;
}

int icrec_encoder_set_attention_bias(icrec_encoder* h, const float* bias_host, int32_t heads) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    ICREC_REQUIRE(e, "icrec_encoder_set_attention_bias: NULL encoder");
    ICREC_HIP(hipSetDevice(e->device));
    if (!bias_host) {  // back to the launches of an encoder that never had one
        if (e->att_bias) ICREC_HIP(hipFree(e->att_bias));
        e->att_bias = nullptr;
        return ICREC_OK;
    }
    ICREC_REQUIRE(heads == e->cfg.heads, "icrec_encoder_set_attention_bias: heads must be %d, the encoder's (got %d)", e->cfg.heads, heads);
    constexpr int N = 2 * ICREC_MAX_SEQLEN - 1;
    // log2 units, like the kernels' scale: the product in double, rounded once
    std::vector<float> tab((size_t)heads * AttentionArgs::BIAS_LD, 0.0f);
    for (int hd = 0; hd < heads; ++hd)
        for (int i = 0; i < N; ++i) {
            const float v = bias_host[(size_t)hd * N + i];
            ICREC_REQUIRE(v - v == 0.0f, "icrec_encoder_set_attention_bias: entry [%d][%d] is not finite", hd, i);
            tab[(size_t)hd * AttentionArgs::BIAS_LD + i] = (float)((double)v * 1.44269504088896340736);
        }
    float* dev = e->att_bias;
    if (!dev && hipMalloc(&dev, tab.size() * 4) != hipSuccess) {
        set_error("icrec_encoder_set_attention_bias: hipMalloc failed");
        return ICREC_ENOMEM;
    }
    const hipError_t err = hipMemcpy(dev, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (err != hipSuccess && !e->att_bias) (void)hipFree(dev);
    ICREC_HIP(err);
    e->att_bias = dev;
    return ICREC_OK;
}

int32_t icrec_encoder_has_attention_bias(const icrec_encoder* h) {
    const Encoder* e = reinterpret_cast<const Encoder*>(h);
    return e ? (e->att_bias != nullptr) : -1;
}

int icrec_encoder_set_score_head(icrec_encoder* h, const float* pooler_w_host, const float* pooler_b_host,
                                 const float* cls_w_host, const float* cls_b_host) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    ICREC_REQUIRE(e, "icrec_encoder_set_score_head: NULL encoder");
    ICREC_HIP(hipSetDevice(e->device));
    if (!pooler_w_host) {  // back to an encoder that never had one
        if (e->score_head) ICREC_HIP(hipFree(e->score_head));
        e->score_head = nullptr;
        return ICREC_OK;
    }
    ICREC_REQUIRE(pooler_b_host && cls_w_host && cls_b_host, "icrec_encoder_set_score_head: NULL bias or classifier with a pooler weight");
    ICREC_REQUIRE(e->cfg.type_vocab >= 2, "icrec_encoder_set_score_head: a pair needs two token-type rows (type_vocab is %d)", e->cfg.type_vocab);
    const size_t H = e->cfg.hidden;
    std::vector<float> host(H * H + 2 * H + 1);  // Wp transposed ([in][out]: score_head_kernel), bp, wc, bc
    float *const bp = host.data() + H * H, *const wc = bp + H;
    for (size_t j = 0; j < H; ++j) {
        for (size_t k = 0; k < H; ++k) {
            const float v = pooler_w_host[j * H + k];
            ICREC_REQUIRE(v - v == 0.0f, "icrec_encoder_set_score_head: pooler weight [%zu][%zu] is not finite", j, k);
            host[k * H + j] = v;
        }
        bp[j] = pooler_b_host[j];
        wc[j] = cls_w_host[j];
        ICREC_REQUIRE(bp[j] - bp[j] == 0.0f, "icrec_encoder_set_score_head: pooler bias [%zu] is not finite", j);
        ICREC_REQUIRE(wc[j] - wc[j] == 0.0f, "icrec_encoder_set_score_head: classifier weight [%zu] is not finite", j);
    }
    wc[H] = cls_b_host[0];
    ICREC_REQUIRE(wc[H] - wc[H] == 0.0f, "icrec_encoder_set_score_head: classifier bias is not finite");
    float* dev = e->score_head;
    if (!dev && hipMalloc(&dev, host.size() * 4) != hipSuccess) {
        set_error("icrec_encoder_set_score_head: hipMalloc failed");
        return ICREC_ENOMEM;
    }
    const hipError_t err = hipMemcpy(dev, host.data(), host.size() * 4, hipMemcpyHostToDevice);
    if (err != hipSuccess && !e->score_head) (void)hipFree(dev);
    ICREC_HIP(err);
    e->score_head = dev;
    return ICREC_OK;
}

int32_t icrec_encoder_has_score_head(const icrec_encoder* h) {
    const Encoder* e = reinterpret_cast<const Encoder*>(h);
    return e ? (e->score_head != nullptr) : -1;
}

// The call's own regions, then (prunes_last_layer) the compact rows' of the pruned last layer; 0 for arguments no call takes.
static size_t workspace_bytes(const Encoder* e, int64_t T, int n_seqs, bool pooled) {
    if (!e || T < 1 || n_seqs < 1) return 0;
    return enc_ws(e->cfg, T).total + (prunes_last_layer(e, pooled) ? enc_ws(e->cfg, n_seqs, true).total : 0);
}

size_t icrec_encode_workspace_bytes(const icrec_encoder* h, int64_t total_tokens, int32_t n_seqs) {
    return workspace_bytes(reinterpret_cast<const Encoder*>(h), total_tokens, n_seqs, true);
}

size_t icrec_score_pairs_workspace_bytes(const icrec_encoder* h, int64_t total_tokens, int32_t n_seqs) {
    return workspace_bytes(reinterpret_cast<const Encoder*>(h), total_tokens, n_seqs, false);
}

// How icrec_encode splits a batch of T tokens (f16x3 mode): [0, T - tail) through the batch kernels in whole rounds of
// one 64-token workgroup per CU, a short remainder [T - tail, T) (tail > 0) through the small-batch kernels.
static int batch_tail(const Encoder* e, int T) {
    const int round_tokens = 64 * e->n_cu;
    return T > round_tokens && T % round_tokens <= e->tail_m ? T % round_tokens : 0;
}

int icrec_encode_batch_split(const icrec_encoder* h, int64_t total_tokens, int64_t* main_tokens, int64_t* tail_tokens) {
    const Encoder* e = reinterpret_cast<const Encoder*>(h);
    ICREC_REQUIRE(e && main_tokens && tail_tokens && total_tokens >= 1 && total_tokens < (1ll << 31), "icrec_encode_batch_split: bad argument");
    *tail_tokens = batch_tail(e, (int)total_tokens);
    *main_tokens = total_tokens - *tail_tokens;
    return ICREC_OK;
}

// Embeddings + LayerNorm, into b.x (fp32) or b.xh / b.xl (f16x3: the residual stream is its two planes).
// seg_b_dev (icrec_score_pairs): each sequence's first position of token type 1 - the kernel's SEG arm; nullptr: type 0.
static void embed(const Encoder* e, const EncBufs& b, const int32_t* ids_dev, const int32_t* cu_dev,
                  const int32_t* seg_b_dev, int n_seqs, int T, hipStream_t st) {
    const icrec_bert_cfg& c = e->cfg;
    const bool x3 = c.gemm_mode == ICREC_GEMM_F16X3;
    auto kern =
        for_hidden(c.hidden, [x3](auto h) { return x3 ? embed_ln_kernel<h(), true> : embed_ln_kernel<h(), false>; });
    if (seg_b_dev)
        kern = for_hidden(c.hidden, [x3](auto h) { return x3 ? embed_ln_kernel<h(), true, true> : embed_ln_kernel<h(), false, true>; });
    hipLaunchKernelGGL(kern, dim3((T + 3) / 4), dim3(256), 0, st, ids_dev, cu_dev, n_seqs, T, e->word, e->pos, e->type, e->eg, e->eb, c.ln_eps, c.vocab_size,
                       c.max_position, b.x, b.xh, b.xl, seg_b_dev);
}

// A token range of an f16x3 call, rows [r0, r0 + n) on stream st, and the form its kernels take, decided once per call.
struct Range {
    int r0, n;
    hipStream_t st;
    bool small;  // n <= small_m: the latency-form GEMMs (launch_wt_linear), every GEMM a launch of its own
    bool layer;  // fuse && !small: the layer kernels (qkv_resident_kernel, one ffn_fused2_kernel per layer)
    bool fold;   // fuse && small: a LayerNorm is the prologue of the GEMM behind it (wt_linear_lnin_kernel)
    // (the layer kernels and the folded LayerNorm exist at hidden 384 only: a hidden-768 model always runs the unfused chain)
    Range(const Encoder* e, int r0, int n, hipStream_t st)
        : r0(r0), n(n), st(st), small(n <= e->small_m), layer(e->fuse && !small && e->cfg.hidden == HID),
          fold(e->fuse && small && e->cfg.hidden == HID) {}
    bool launches_qkv(int l) const { return l == 0 || !layer; }  // (else ffn_fused2_kernel's epilogue computes it)
    bool ffn_ln_to_next(int l, int layers) const { return fold && l + 1 < layers; }  // to the next QKV's prologue
};

// cls: the compact rows' regions when the last layer is pruned to each sequence's first token (prunes_last_layer), else
// nullptr.  The last hidden state is then rows [0, n_seqs) of cls->xh / cls->xl and b's x planes stay one layer behind.
static int encode_x3(Encoder* e, const EncBufs& b, const EncBufs* cls, const int32_t* cu_dev, int n_seqs, int T,
                     int max_seqlen, hipStream_t st) {
    const icrec_bert_cfg& c = e->cfg;
    const int H = c.hidden, I = c.intermediate;
    const auto ln_wt = for_hidden(H, [](auto h) { return ln_wt_kernel<h()>; });
    // Fused batches dispatch their attention workgroups longest sequence first; the order lives in the fp32 x region,
    // which f16x3 mode leaves unused.  The unfused reference chain runs in natural order.
    int32_t* const order = n_seqs >= 64 && e->fuse ? reinterpret_cast<int32_t*>(b.x) : nullptr;
    if (order) attention_dispatch_order(cu_dev, n_seqs, order, st);
    AttentionArgs att = {b.qkv, cu_dev, n_seqs, max_seqlen, c.heads, H, e->att_bias, order, nullptr, b.ch, b.cl, false};
    const bool split_att = e->side_stream && attention_wants_side(att);
    // Token ranges: [0, T_main) goes through the batch kernels in whole rounds of one 64-token workgroup per CU, a short
    // remainder [T_main, T) through the small-batch kernels (same arithmetic, same bits) instead of costing every batch
    // kernel an extra, almost empty round.
    const int T_tail = batch_tail(e, T), T_main = T - T_tail;
    SideStream* sd = nullptr;
    if (e->side_stream && (T_tail || split_att))
        if (int rc_ = side_for(e, st, &sd)) return rc_;
    // The remainder's kernels run on the side stream: its QKV beside the batch QKV, its attention-out / FFN chain beside
    // the batch's.  Attention covers all rows, so it joins both; the side stream's in-order execution keeps its own
    // layers apart.
    const Range main(e, 0, T_main, st), tail(e, T_main, T_tail, sd ? sd->side : st);
    const bool tail_on_side = T_tail && sd;
    if (main.layer || tail.layer) {  // the layer kernels' LDS is above the default limit
        if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(qkv_resident_kernel), QKVR_LDS)) return rc_;
        if (int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(ffn_fused2_kernel), FFN2_LDS)) return rc_;
    }

    auto qkv_stage = [&](const Range& r, int l) {
        const LayerW& L = e->layers[l];
        _Float16 *const xhr = b.xh + (size_t)r.r0 * H, *const xlr = b.xl + (size_t)r.r0 * H;
        float* const qkvr = b.qkv + (size_t)r.r0 * 3 * H;
        if (r.layer) {  // activation-resident form: one 64-token workgroup per CU
            hipLaunchKernelGGL(qkv_resident_kernel, dim3((r.n + 63) / 64), dim3(512), QKVR_LDS, r.st, xhr, xlr, r.n,
                               L.Wqkv_p, L.bqkv, qkvr, 3 * H);
        } else if (l > 0 && r.ffn_ln_to_next(l - 1, c.layers)) {
            // the previous layer's FFN LayerNorm is this kernel's prologue (t1 rows -> planes in LDS and, from the
            // workgroups of feature block 0, to xh / xl): one graph node fewer per layer
            const LayerW& Lp = e->layers[l - 1];
            const int nbn = 3 * H / 64;
            hipLaunchKernelGGL((wt_linear_lnin_kernel<0>), dim3(((r.n + 31) / 32) * nbn), dim3(256), 0, r.st,
                               (const float*)(b.t1 + (size_t)r.r0 * H), r.n, Lp.g2, Lp.b2n, c.ln_eps, xhr, xlr, L.Wqkv_p,
                               3 * H, L.bqkv, qkvr, (_Float16*)nullptr, (_Float16*)nullptr, nbn);
        } else {
            launch_wt_linear<0>(xhr, xlr, r.n, H, L.Wqkv_p, 3 * H, L.bqkv, qkvr, nullptr, nullptr, r.st, r.small);
        }
    };
    auto post_stage = [&](const Range& r, int l, const EncBufs& b) {  // (b: the call's regions, or the compact rows')
        const LayerW& L = e->layers[l];
        float* const t1r = b.t1 + (size_t)r.r0 * H;
        _Float16 *const xhr = b.xh + (size_t)r.r0 * H, *const xlr = b.xl + (size_t)r.r0 * H;
        const _Float16 *const chr = b.ch + (size_t)r.r0 * H, *const clr = b.cl + (size_t)r.r0 * H;
        if (r.layer) {
            // attention-out + residual + LN and the whole FFN block + residual + LN: ONE kernel per half layer
            // (x1 stays on chip between the two LayerNorm sites)
            ScopedTimer tm(T_FFN_UP, r.st);
            // ... and, but for the last layer, the NEXT layer's QKV projection of the rows it has just normalised
            const bool next_qkv = l + 1 < c.layers;
            const LayerW& Ln = e->layers[next_qkv ? l + 1 : l];
            hipLaunchKernelGGL(ffn_fused2_kernel, dim3((r.n + 63) / 64), dim3(512), FFN2_LDS, r.st, xhr, xlr, r.n, I,
                               L.W1_p, L.b1, L.W2_p, L.b2, L.g2, L.b2n, c.ln_eps, chr, clr, L.Wo_p, L.bo, L.g1, L.b1n,
                               next_qkv ? (const _Float16*)Ln.Wqkv_p : (const _Float16*)nullptr, (const float*)Ln.bqkv,
                               b.qkv + (size_t)r.r0 * 3 * H, 3 * H);
            return;
        }
        _Float16 *const hhr = b.hh + (size_t)r.r0 * I, *const hlr = b.hl + (size_t)r.r0 * I;
        launch_wt_linear<2>(chr, clr, r.n, H, L.Wo_p, H, L.bo, t1r, xhr, xlr, r.st, r.small);  // residual: x planes
        if (r.fold) {  // LayerNorm + FFN-up in one node (wt_linear_lnin_kernel)
            const int nbn = I / 64;
            hipLaunchKernelGGL((wt_linear_lnin_kernel<1>), dim3(((r.n + 31) / 32) * nbn), dim3(256), 0, r.st,
                               (const float*)t1r, r.n, L.g1, L.b1n, c.ln_eps, xhr, xlr, L.W1_p, I, L.b1, (float*)nullptr,
                               hhr, hlr, nbn);
        } else {
            hipLaunchKernelGGL(ln_wt, dim3((r.n + 15) / 16), dim3(256), 0, r.st, t1r, r.n, L.g1, L.b1n, c.ln_eps,
                               xhr, xlr);
            ScopedTimer tm(r.small ? T_FFN_UP_SMALL : T_FFN_UP, r.st);
            launch_wt_linear<1>(xhr, xlr, r.n, H, L.W1_p, I, L.b1, nullptr, hhr, hlr, r.st, r.small);
        }
        launch_wt_linear<2>(hhr, hlr, r.n, I, L.W2_p, H, L.b2, t1r, xhr, xlr, r.st, r.small);
        if (!r.ffn_ln_to_next(l, c.layers))
            hipLaunchKernelGGL(ln_wt, dim3((r.n + 15) / 16), dim3(256), 0, r.st, t1r, r.n, L.g2, L.b2n, c.ln_eps,
                               xhr, xlr);
    };

    if (tail_on_side) ICREC_HIP(link(sd, st, sd->side));  // the side stream starts behind the embeddings
    for (int l = 0; l < c.layers; ++l) {
        const bool pruned = cls && l == c.layers - 1;
        if (T_tail && tail.launches_qkv(l)) qkv_stage(tail, l);
        if (main.launches_qkv(l)) qkv_stage(main, l);
        if (tail_on_side) ICREC_HIP(link(sd, sd->side, st));
        att.block0_only = pruned;
        if (int rc_ = run_attention(att, st, split_att ? sd : nullptr)) return rc_;
        if (pruned) {
            // Rows cu[s] of the context (query block 0 wrote them) and of x -> compact rows, then the unfused chain over
            // those n_seqs rows on the caller's stream, in the form their number picks.  The side stream joined above
            // and gets no more work: nothing is left to join before the pooling.
            hipLaunchKernelGGL(gather_cls_rows_kernel, dim3((n_seqs * (H / 8) + 255) / 256), dim3(256), 0, st, b.ch, b.cl,
                               b.xh, b.xl, cu_dev, n_seqs, H / 8, cls->ch, cls->cl, cls->xh, cls->xl);
            Range rows(e, 0, n_seqs, st);
            rows.layer = false;  // (no layer kernel for compact rows: above small_m they take the batch-form GEMMs)
            post_stage(rows, l, *cls);
            return ICREC_OK;
        }
        if (tail_on_side) ICREC_HIP(link(sd, st, sd->side));
        if (T_tail) post_stage(tail, l, b);
        post_stage(main, l, b);
    }
    if (tail_on_side) ICREC_HIP(link(sd, sd->side, st));  // pooling reads every row: the side stream joins here
    return ICREC_OK;
}

static int encode_f32(const Encoder* e, const EncBufs& b, const int32_t* cu_dev, int n_seqs, int T, int max_seqlen,
                      hipStream_t st) {
    const icrec_bert_cfg& c = e->cfg;
    const int H = c.hidden, I = c.intermediate, rows_grid = (T + 3) / 4;
    const auto add_ln = for_hidden(H, [](auto h) { return add_ln_kernel<h()>; });
    const AttentionArgs att = {b.qkv, cu_dev, n_seqs, max_seqlen, c.heads, H, e->att_bias, nullptr, b.ctx, nullptr, nullptr, false};
    for (int l = 0; l < c.layers; ++l) {
        const LayerW& L = e->layers[l];
        launch_linear<false>(b.x, T, H, L.Wqkv, 3 * H, L.bqkv, b.qkv, st);
        if (int rc_ = run_attention(att, st, nullptr)) return rc_;
        launch_linear<false>(b.ctx, T, H, L.Wo, H, L.bo, b.t1, st);
        hipLaunchKernelGGL(add_ln, dim3(rows_grid), dim3(256), 0, st, b.t1, b.x, T, L.g1, L.b1n,
                           c.ln_eps, b.xh, b.xl);
        {
            ScopedTimer tm(T_FFN_UP, st);
            launch_linear<true>(b.x, T, H, L.W1, I, L.b1, b.h, st);
        }
        launch_linear<false>(b.h, T, I, L.W2, H, L.b2, b.t1, st);
        hipLaunchKernelGGL(add_ln, dim3(rows_grid), dim3(256), 0, st, b.t1, b.x, T, L.g2, L.b2n,
                           c.ln_eps, b.xh, b.xl);
    }
    return ICREC_OK;
}

// Where a call left the last hidden state its entry reads: fp32 rows `x` or (f16x3) the planes `xh` / `xl`; sequence s's
// first token is row cu[s] or, compact (the pruned last layer: nothing but those rows exists), row s.
struct LastRows {
    const float* x;
    const _Float16 *xh, *xl;
    bool compact;
};

// The forward pass behind icrec_encode_ex and icrec_score_pairs, after the entry's own argument checks (`who`: its name,
// the prefix of every error message): the shared checks, the workspace, then embeddings (seg_b_dev: see embed) and every
// layer on `st`.  pooled: the entry reads what the handle's pooling mode says, else each sequence's first token alone;
// every_token: it also reads every token's state.  timer: started once the call is admitted, or nullptr.
static int forward(Encoder* e, const char* who, const int32_t* ids_dev, const int32_t* cu_dev, const int32_t* seg_b_dev,
                   int32_t n_seqs, int64_t T64, int32_t max_seqlen, bool pooled, bool every_token, void* ws,
                   size_t ws_bytes, hipStream_t st, ScopedTimer* timer, LastRows* last) {
    ICREC_REQUIRE(n_seqs >= 1 && T64 >= n_seqs && T64 < (1ll << 31), "%s: bad n_seqs/total_tokens (%d, %lld)", who, n_seqs, (long long)T64);
    ICREC_REQUIRE(max_seqlen >= 1 && max_seqlen <= e->max_seqlen, "%s: max_seqlen must be in [1, %d] (got %d)", who, e->max_seqlen, max_seqlen);
    const int T = (int)T64;
    const size_t need = workspace_bytes(e, T, n_seqs, pooled);
    if (!ws || ws_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(e->device));
    if (timer) timer->start(st);
    char* base = reinterpret_cast<char*>(ws);
    const icrec_bert_cfg& c = e->cfg;
    const EncWs w = enc_ws(c, T);
    const EncBufs b(base, w, c, T);
    const EncBufs cls(base + w.total, enc_ws(c, n_seqs, true), c, n_seqs);  // (inside the workspace only if prunes_last_layer)
    // The last layer is pruned to each sequence's first token when nothing else of it is read: not when the caller
    // wants every token's state, and not when every token is a first token (nothing to save).
    const bool pruned = prunes_last_layer(e, pooled) && !every_token && n_seqs < T;
    embed(e, b, ids_dev, cu_dev, seg_b_dev, n_seqs, T, st);
    if (int rc_ = c.gemm_mode == ICREC_GEMM_F16X3 ? encode_x3(e, b, pruned ? &cls : nullptr, cu_dev, n_seqs, T, max_seqlen, st)
                                                  : encode_f32(e, b, cu_dev, n_seqs, T, max_seqlen, st))
        return rc_;
    const EncBufs& r = pruned ? cls : b;
    *last = {r.x, r.xh, r.xl, pruned};
    return ICREC_OK;
}

int icrec_encode(icrec_encoder* h, const int32_t* ids_dev, const int32_t* cu_dev, int32_t n_seqs, int64_t T64,
                 int32_t max_seqlen, float* out_dev, void* ws, size_t ws_bytes, void* stream) {
    return icrec_encode_ex(h, ids_dev, cu_dev, n_seqs, T64, max_seqlen, out_dev, nullptr, ws, ws_bytes, stream);
}

int icrec_encode_ex(icrec_encoder* h, const int32_t* ids_dev, const int32_t* cu_dev, int32_t n_seqs, int64_t T64,
                    int32_t max_seqlen, float* out_dev, float* tokens_out_dev, void* ws, size_t ws_bytes,
                    void* stream) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    ICREC_REQUIRE(e && ids_dev && cu_dev && out_dev, "icrec_encode: NULL argument");
    ICREC_REQUIRE((reinterpret_cast<uintptr_t>(tokens_out_dev) & 15) == 0, "icrec_encode_ex: tokens_out_dev must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ScopedTimer whole(T_ENCODE);  // (forward starts it)
    LastRows last;
    if (int rc_ = forward(e, "icrec_encode", ids_dev, cu_dev, nullptr, n_seqs, T64, max_seqlen, true, tokens_out_dev != nullptr,
                          ws, ws_bytes, st, &whole, &last))
        return rc_;
    const int H = e->cfg.hidden;
    const bool x3 = e->cfg.gemm_mode == ICREC_GEMM_F16X3;
    const auto pool =
        for_hidden(H, [x3](auto h) { return x3 ? pool_norm_kernel<h(), true> : pool_norm_kernel<h(), false>; });
    const int pool_rows = e->pooling != ICREC_POOL_CLS ? POOL_ROWS_MEAN : last.compact ? POOL_ROWS_CLS_COMPACT : POOL_ROWS_CLS;
    hipLaunchKernelGGL(pool, dim3(n_seqs), dim3(H), 0, st, last.x, last.xh, last.xl, cu_dev, e->cfg.n_normalize, out_dev,
                       pool_rows);
    if (tokens_out_dev) {  // hidden is a multiple of 4: every thread's 4 features are 16 (planes: 8) bytes, aligned
        const size_t n4 = (size_t)T64 * H / 4;  // (every token's state is wanted: `last` is every row)
        hipLaunchKernelGGL(x3 ? tokens_out_kernel<true> : tokens_out_kernel<false>, dim3((unsigned)((n4 + 255) / 256)),
                           dim3(256), 0, st, last.x, last.xh, last.xl, n4, tokens_out_dev);
    }
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

int icrec_score_pairs(icrec_encoder* h, const int32_t* ids_dev, const int32_t* cu_dev, const int32_t* seg_b_dev,
                      int32_t n_seqs, int64_t T64, int32_t max_seqlen, float* scores_out_dev, void* ws, size_t ws_bytes,
                      void* stream) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    ICREC_REQUIRE(e && ids_dev && cu_dev && seg_b_dev && scores_out_dev, "icrec_score_pairs: NULL argument");
    ICREC_REQUIRE(e->score_head, "icrec_score_pairs: the encoder has no score head (icrec_encoder_set_score_head)");
    hipStream_t st = (hipStream_t)stream;
    LastRows last;
    if (int rc_ = forward(e, "icrec_score_pairs", ids_dev, cu_dev, seg_b_dev, n_seqs, T64, max_seqlen, false, false, ws,
                          ws_bytes, st, nullptr, &last))
        return rc_;
    const int H = e->cfg.hidden;
    const bool x3 = e->cfg.gemm_mode == ICREC_GEMM_F16X3;
    const float *const wpt = e->score_head, *const bp = wpt + (size_t)H * H, *const wc = bp + H, *const bc = wc + H;
    const auto kern =
        for_hidden(H, [x3](auto h) { return x3 ? score_head_kernel<h(), true> : score_head_kernel<h(), false>; });
    const int per_wg = H == HID_BASE ? HEAD_SEQS<HID_BASE> : HEAD_SEQS<HID>;
    hipLaunchKernelGGL(kern, dim3((n_seqs + per_wg - 1) / per_wg), dim3(384), 0, st, last.x, last.xh, last.xl, cu_dev,
                       n_seqs, last.compact, wpt, bp, wc, bc, scores_out_dev);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
