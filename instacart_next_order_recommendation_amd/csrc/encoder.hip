// encoder.hip — the SentenceTransformer forward on gfx950: BertModel (6 post-LN layers),
// masked mean pooling, L2 normalisation; token-packed (varlen), fp32 throughout, every GEMM
// and both attention products on v_mfma_f32_32x32x2_f32.
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

#include "common.h"
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

// ---------------------------------------------------------------- attention (tf:111-136, 164-203)
// One workgroup = one (sequence, head) and up to sixteen 32-row query blocks (one per wave), for heads of D = 32
// (hidden 384) or D = 64 dims (hidden 768: BERT-base).
// S^T = K.Q^T is computed with keys on the accumulator rows, so each lane ends up with the
// scores of ONE query (column = lane & 31) against 16 keys per 32-key tile.  The softmax is
// then lane-local plus one exchange with lane^32, and the exponentiated accumulator registers
// are fed back unchanged as the A operand of P.V (A[i=query][k=key]): no transpose, no LDS
// round trip.  Key order inside the P.V chain is therefore, per 32-key tile,
//   e = 0..15: key (e&3)+8(e>>2) then key (e&3)+8(e>>2)+4
// and the softmax denominator is the sum of the two half-wave partial sums; the oracle
// (icrec_oracle.c, attention block) accumulates in exactly this order.  A wave's output is D / 32 tiles of 32 x 32
// (dims 32 dt + r of the lane's column).
//
// One launch per length bucket: NKT = max 32-key tiles (1, 2, 4, 6, 8, 16), and as many waves; sequences of
// nlo < nkt <= NKT key tiles belong to the launch.  A workgroup whose sequence belongs to another bucket exits at once,
// so short sequences run with the LDS footprint / occupancy of their own bucket even in a mixed batch.
// K and V of the (sequence, head) live in LDS; each wave's 32 query rows come straight from
// global memory into the B-operand registers.
//
// Key tiles that LDS holds at once: a 32-dim head's K and V fit whole (KC = NKT); a 64-dim head's take twice the LDS, so
// its longest bucket (9-16 tiles, up to 512 keys) is staged in chunks of 8 tiles, twice - K alone for the row maximum,
// then K and V for the exponentials and P.V.  The per-query arithmetic depends neither on the bucket nor on the
// chunking: a sequence gives the same bits whichever launch serves it.
constexpr int att_kc(int D, int NKT) { return D == 64 && NKT > 8 ? 8 : NKT; }

// A row's denominator from the two half-waves' partial sums: half 0's + half 1's, in both halves.
__device__ __forceinline__ float join_halves(float v, int h) {
    const float other = __shfl_xor(v, 32, 64);
    return h == 0 ? v + other : other + v;
}

// Relative-position attention bias (MPNet / T5 style; icrec_encoder_set_attention_bias): the BIAS arm of both kernels
// adds bias[head][key - query] to every scaled logit, in every layer.  The device table holds, per head, ATT_BIAS_LD
// floats in log2 units (pre-multiplied by log2(e), like the scale): entry ICREC_MAX_SEQLEN - 1 + (key - query), the last
// one padding.  A workgroup copies its head's row into LDS (4 KB) ahead of the first staging barrier; a lane owns one
// query, so register e of key tile kt reads entry  att_bias_base(..) + 32 kt + (e & 3) + 8 (e >> 2)  - per tile 16 reads
// at immediate offsets from one address, consecutive lanes on consecutive banks.  Keys and queries past the sequence
// (clamped rows, masked / never stored) stay inside the table: both positions are below ICREC_MAX_SEQLEN.
// The biased logit is ONE fma, scale * s + bias, and the row maximum is taken over it - whatever the bucket, the
// chunking or the dispatch form: the same bits for a sequence alone and inside any batch.
constexpr int ATT_BIAS_LD = 2 * ICREC_MAX_SEQLEN;
__device__ __forceinline__ void att_bias_to_lds(float* dst, const float* __restrict__ bias, int hd, int tid, int nthreads) {
    const f32x4* src = reinterpret_cast<const f32x4*>(bias + (size_t)hd * ATT_BIAS_LD);
    for (int i = tid; i < ATT_BIAS_LD / 4; i += nthreads) reinterpret_cast<f32x4*>(dst)[i] = src[i];
}
// entry of (query qb*32 + r, key acc_row(0, lane)) of key tile 0
__device__ __forceinline__ int att_bias_base(int qb, int lane) {
    return ICREC_MAX_SEQLEN - 1 - (qb * 32 + (lane & 31)) + acc_row(0, lane);
}

// Exact fp32 form (gemm_mode F32): both products on v_mfma_f32_32x32x2_f32, head dims in pairs ascending.
// Output: the fp32 context rows.
template <int D, int NKT, bool BIAS = false>
__global__ __launch_bounds__(NKT * 64) void attention_kernel(const float* __restrict__ qkv,
                                                             const int32_t* __restrict__ cu, int heads, int H,
                                                             float scale_log2e, float* __restrict__ ctx, int nlo,
                                                             const float* __restrict__ bias) {
    constexpr int KC = att_kc(D, NKT);
    constexpr int LDK = D + 4;  // K LDS row stride (even/odd split layout, like the GEMM tiles)
    // Sixteen score tiles do not fit in registers (and 64-dim heads leave room for none): each tile is then computed
    // twice - once for the row maximum, once more for its exponentials, which the P.V product consumes at once.  Same
    // MFMA chain both times, and the denominator and P.V accumulate in the same order as in the all-in-registers form:
    // the same bits.
    constexpr bool RECOMP = D == 64 || NKT > 8;
    __shared__ __attribute__((aligned(16))) float Ks[KC * 32 * LDK];
    __shared__ __attribute__((aligned(16))) float Vs[KC * 32 * D];
    __shared__ float Ls[NKT * 32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x / heads, hd = blockIdx.x % heads;
    const int t0 = cu[s], L = cu[s + 1] - t0;
    const int nkt = (L + 31) >> 5;
    if (nkt > NKT || nkt <= nlo) return;  // another bucket's sequence
    const int ld = 3 * H;
    const int r = lane & 31, h = lane >> 5, qb = wave;
    const bool active = qb < nkt;  // wave-uniform; idle waves still take part in the barriers of the staging
    const float* bt = nullptr;  // this lane's window of the head's bias row (BIAS), visible behind the staging barrier
    if constexpr (BIAS) {
        __shared__ __attribute__((aligned(16))) float Bs[ATT_BIAS_LD];
        att_bias_to_lds(Bs, bias, hd, tid, NKT * 64);
        bt = Bs + att_bias_base(qb, lane);
    }
    float4 qf[D / 8];  // this lane's query row -> B fragments (lane half h supplies the even / odd dims of every pair)
    {
        int qr = qb * 32 + r;
        qr = qr < L ? qr : L - 1;
        const float4* qp = reinterpret_cast<const float4*>(qkv + (size_t)(t0 + qr) * ld + hd * D);
#pragma unroll
        for (int kq = 0; kq < D / 8; ++kq) {
            const float4 a = qp[2 * kq], b = qp[2 * kq + 1];
            qf[kq] = h == 0 ? make_float4(a.x, a.z, b.x, b.z) : make_float4(a.y, a.w, b.y, b.w);
        }
    }
    const bool once = KC == NKT || nkt <= KC;  // the whole sequence fits: staged once, K and V
    // key tiles [c0, c0 + KC) -> LDS (K in the even/odd split layout, V row-major); rows past L are clamped (masked
    // below / never stored)
    auto stage = [&](int c0, bool with_v) {
        if (!once) __syncthreads();  // the previous chunk's readers are done
        const int nk = (nkt - c0 < KC ? nkt - c0 : KC) * 32;
        for (int id = tid; id < nk * (D / 4); id += NKT * 64) {
            const int row = id / (D / 4), c = id % (D / 4);
            const int key = c0 * 32 + row, rr = key < L ? key : L - 1;
            const float* src = qkv + (size_t)(t0 + rr) * ld + hd * D + c * 4;
            const float4 kv = *reinterpret_cast<const float4*>(src + H);
            float* kp = Ks + row * LDK + (c >> 1) * 8 + (c & 1) * 2;
            *reinterpret_cast<float2*>(kp) = make_float2(kv.x, kv.z);
            *reinterpret_cast<float2*>(kp + 4) = make_float2(kv.y, kv.w);
            if (with_v) *reinterpret_cast<float4*>(Vs + row * D + c * 4) = *reinterpret_cast<const float4*>(src + 2 * H);
        }
        __syncthreads();
    };
    // scores of key tile kt (staged from c0) in log2 units (scale * log2(e) folded), tail keys at -inf:
    // t[e] = scale_log2e * sum_d K[kt*32 + krow(e)][d] * Q[qb*32 + r][d]   (BIAS: ... + bias[krow(e) - query], one fma)
    auto score_tile = [&](int kt, int c0) {
        f32x16 t;
#pragma unroll
        for (int e = 0; e < 16; ++e) t[e] = 0.0f;
#pragma unroll
        for (int kq = 0; kq < D / 8; ++kq) {
            const float4 kf = *reinterpret_cast<const float4*>(Ks + ((kt - c0) * 32 + r) * LDK + kq * 8 + h * 4);
            t = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[kq].x, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[kq].y, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[kq].z, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[kq].w, t, 0, 0, 0);
        }
        const bool last = kt == nkt - 1;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            float v;
            if constexpr (BIAS) v = fmaf(t[e], scale_log2e, bt[kt * 32 + (e & 3) + 8 * (e >> 2)]);
            else v = t[e] * scale_log2e;
            if (last && kt * 32 + acc_row(e, lane) >= L) v = -INFINITY;
            t[e] = v;
        }
        return t;
    };
    // O += P.V for key tile kt, with P taken straight from the accumulator registers
    f32x16 o[D / 32];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[dt][e] = 0.0f;
    auto pv_tile = [&](int kt, int c0, const f32x16& p) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = (kt - c0) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
#pragma unroll
            for (int dt = 0; dt < D / 32; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[e], Vs[key * D + 32 * dt + r], o[dt], 0, 0, 0);
        }
    };
    // every key tile of the sequence, chunk by chunk (one chunk when the sequence was staged whole)
    auto for_tiles = [&](bool with_v, auto&& f) {
#pragma unroll
        for (int c0 = 0; c0 < NKT; c0 += KC) {
            if (c0 < nkt) {
                if (!once) stage(c0, with_v);
                if (active) {
                    const int c1 = c0 + KC < nkt ? c0 + KC : nkt;
                    for (int kt = c0; kt < c1; ++kt) f(kt, c0);
                }
            }
        }
    };
    if (once) stage(0, true);
    // p = 2^(v - max); denominator = this half-wave's keys ascending, then the two halves added
    float lsum = 0.0f;
    if constexpr (RECOMP) {
        float mx = -INFINITY;
        for_tiles(false, [&](int kt, int c0) {
            const f32x16 t = score_tile(kt, c0);
#pragma unroll
            for (int e = 0; e < 16; ++e) mx = fmaxf(mx, t[e]);
        });
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        for_tiles(true, [&](int kt, int c0) {
            f32x16 t = score_tile(kt, c0);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = __builtin_amdgcn_exp2f(t[e] - mx);
                t[e] = p;
                lsum = lsum + p;
            }
            pv_tile(kt, c0, t);
        });
    } else if (active) {
        f32x16 sc[NKT];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt < nkt) {
                sc[kt] = score_tile(kt, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sc[kt][e]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt < nkt) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float p = __builtin_amdgcn_exp2f(sc[kt][e] - mx);
                    sc[kt][e] = p;
                    lsum = lsum + p;
                }
            }
        }
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
            if (kt < nkt) pv_tile(kt, 0, sc[kt]);
    }
    if (!active) return;  // (no barrier below)
    lsum = join_halves(lsum, h);
    if (h == 0) Ls[wave * 32 + r] = lsum;
    // ---- normalise rows by their denominator and store (row = query, column = head dim);
    // Ls was written by this wave's own lanes (wave-local LDS ordering makes it visible).
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int qrow = acc_row(e, lane);
        const int tq = qb * 32 + qrow;
        if (tq < L) {
            const float l = Ls[wave * 32 + qrow];
            float* dst = ctx + (size_t)(t0 + tq) * H + hd * D + r;
#pragma unroll
            for (int dt = 0; dt < D / 32; ++dt) dst[32 * dt] = o[dt][e] / l;
        }
    }
}

// ---------------------------------------------------------------- dispatch order of the attention workgroups
// order[0 .. n_seqs) = the sequences sorted by key-tile count, longest first (counting sort over the
// ICREC_MAX_SEQLEN / 32 possible counts; the order inside one count is whatever the atomics give - the workgroups are
// independent, results do not depend on it).  The attention launches map workgroup b to sequence order[b / heads]: each
// bucket's workgroups are then dispatched longest-first with the other buckets' (empty) workgroups behind them instead
// of in between, so a launch does not end on a few long sequences that started last.
__global__ __launch_bounds__(1024) void seq_order_kernel(const int32_t* __restrict__ cu, int n_seqs,
                                                         int32_t* __restrict__ order) {
    constexpr int NB = ICREC_MAX_SEQLEN / 32;  // bin NB - nkt holds the sequences of nkt key tiles
    __shared__ int hist[NB];
    const int tid = threadIdx.x;
    if (tid < NB) hist[tid] = 0;
    __syncthreads();
    auto bin = [&](int s) {
        const int L = cu[s + 1] - cu[s];
        const int nkt = (L + 31) >> 5;
        return NB - (nkt < 1 ? 1 : (nkt > NB ? NB : nkt));
    };
    for (int s0 = tid; s0 < n_seqs; s0 += 1024) atomicAdd(&hist[bin(n_seqs - 1 - s0)], 1);
    __syncthreads();
    if (tid == 0) {  // exclusive prefix sum: hist[b] becomes the first slot of bin b
        int run = 0;
        for (int b = 0; b < NB; ++b) { const int c = hist[b]; hist[b] = run; run += c; }
    }
    __syncthreads();
    for (int s0 = tid; s0 < n_seqs; s0 += 1024) {
        const int s = n_seqs - 1 - s0;
        order[atomicAdd(&hist[bin(s)], 1)] = s;
    }
}

// ---------------------------------------------------------------- attention, f16x3 arithmetic
// Same structure as attention_kernel (one block per (sequence, head), S^T on the accumulator rows, P fed
// back from the accumulators), with both products on the f16 MFMA by the 3-term split of wt_gemm.h (one accumulator,
// the plane scales folded into constants: see the kernel):
//   S^T ~ K_hi.Q_hi + K_hi.Q_lo + K_lo.Q_hi        O ~ P_hi.V_hi + P_hi.V_lo + P_lo.V_hi
// K is staged as hi/lo f16 planes [key][D] with the 16-B chunks of a row XOR-swizzled (att_k_swz), V as row-major hi/lo
// planes [key][D] read through the transposing LDS read; Q (per wave) and P (per tile, straight from the accumulators)
// are split in registers.
// For a 32-key tile and k-step s, slot j of lane-half h is key 4h + (j&3) + 8(2s + (j>>2)) — the keys
// accumulator register e = 8s + j holds — on both operands.
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// ds_read_b64_tr_b16 (gfx950): all 64 lanes must be active; `p` is this lane's Mechanism address (8-byte aligned)
__device__ __forceinline__ half4 lds_read_tr(const _Float16* p) {
    typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    return __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                                         (__attribute__((address_space(3))) fp16x4*)(reinterpret_cast<uintptr_t>(p))));
}

// Swizzle key of a K plane row: 64-B rows (D = 32) repeat their bank pattern every 4 rows, 128-B rows (D = 64) every row.
constexpr int att_k_swz(int D, int row) { return D == 32 ? (row >> 2) & 3 : row & 7; }
// Workgroups per CU the register allocation aims at (32-dim heads; 64-dim heads are bound by their LDS).
constexpr int att_x3_wgs(int D, int NKT) { return D != 32 ? 1 : NKT >= 6 ? 4 : NKT == 4 ? 3 : 1; }

// Output: the context as f16 hi/lo planes (`ch` / `cl`).  order: seq_order_kernel's dispatch order, or nullptr.
// nqb: the query blocks to compute, from block 0 - NKT for all of them; 1 for the last layer of a CLS-pooled encoder,
// which reads each sequence's first row only: every wave still stages K / V and meets every barrier, only wave 0 runs
// the score / softmax / P.V loop and stores its tile, the very bits a full launch gives those rows.
// BIAS: the relative-position bias arm (see att_bias_to_lds), 4 KB of LDS more.
template <int D, int NKT, bool BIAS = false>  // NKT waves, one per 32-row query block
__global__ __launch_bounds__(NKT * 64, att_x3_wgs(D, NKT)) void attention_x3_kernel(
    const float* __restrict__ qkv, const int32_t* __restrict__ cu, int heads, int H, float scale_log2e,
    _Float16* __restrict__ ch, _Float16* __restrict__ cl, const int32_t* __restrict__ order, int nlo, int nqb,
    const float* __restrict__ bias) {
    // Single-accumulator form of the split (wt_gemm.h): every operand is carried as hi/lo f16 planes of 16 x (Q, K, V)
    // or 1024 p (the probabilities), the three products of a k-step accumulate into ONE fp32 tile, and the power-of-two
    // scales are folded into constants: S' = 256 S, O' = 16384 sum_k p_k V_k, l' = 1024 sum_k p_k, O = O' / (16 l').
    // All splits are the 3-instruction form (mask / subtract / v_cvt_pkrtz pairs).
    //
    // Long buckets (NKT >= 6) and 64-dim heads, RECOMP: the score tiles are computed TWICE - once for the row maximum
    // (on the hi x hi products alone, see score_tile), once more in full for the exponentials, each tile consumed by the
    // PV product as soon as it exists - instead of all of them being held in 128 registers between the two passes: 16
    // more MFMAs per wave, and the 32-dim kernel drops under 128 VGPRs; with the output tile parked on the K
    // planes (behind one more barrier) it also drops to 67 KB of LDS - TWO workgroups per CU, so one's staging and
    // barrier phases run under the other's arithmetic.
    constexpr int KC = att_kc(D, NKT), G = D / 4;  // G: 4-dim groups of a row
    constexpr bool RECOMP = D == 64 || NKT >= 6;
    // The two places where the widths differ for speed, not for width.  32-dim heads issue all of a thread's K/V loads
    // before the first one is consumed (PREFETCH) and park each wave's output tile (hi | lo) on the K planes once all waves
    // have left them, to write it out 16 B per lane - 4 store instructions instead of 32 two-byte ones (PARK; the NKT
    // tiles fill the K planes exactly).  64-dim heads stage with a plain loop and store straight from the accumulators.
    constexpr bool PREFETCH = D == 32, PARK = D == 32;
    static_assert(!PARK || KC == NKT, "the parked output tiles need the K planes of all NKT key tiles");
    __shared__ __attribute__((aligned(16))) _Float16 Kbuf[2 * KC * 32 * D];
    _Float16* const Kh = Kbuf;
    _Float16* const Kl = Kbuf + KC * 32 * D;
    // V as it arrives: row-major hi / lo planes [key][D] (one 8-byte store per thread and plane where the
    // transposed image took four 2-byte ones); the P.V product reads its B operand - 4 consecutive keys of one head
    // dimension per lane - with the transposing LDS read (ds_read_b64_tr_b16: per 16-lane group a block of 4 keys x 16
    // dims, lane 4q + p supplying the address of key q, dims 4p..4p+3, lane i receiving dim i of the 4 keys; at D = 32 a
    // 32-lane half covers 4 rows of 64 B = every bank once).
    __shared__ __attribute__((aligned(16))) _Float16 Vh[KC * 32 * D];
    __shared__ __attribute__((aligned(16))) _Float16 Vl[KC * 32 * D];
    __shared__ float Ls[NKT * 32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sidx = blockIdx.x / heads, hd = blockIdx.x % heads;
    const int s = order != nullptr ? order[sidx] : sidx;  // seq_order_kernel: longest first
    const int t0 = cu[s], L = cu[s + 1] - t0;
    const int nkt = (L + 31) >> 5;
    if (nkt > NKT || nkt <= nlo) return;  // another bucket's sequence
    const int ld = 3 * H;
    const int r = lane & 31, h = lane >> 5, qb = wave;
    const bool active = qb < nkt && qb < nqb;  // wave-uniform; idle waves still take part in the barriers
    const float* bt = nullptr;  // this lane's window of the head's bias row (BIAS), visible behind the staging barrier
    if constexpr (BIAS) {
        __shared__ __attribute__((aligned(16))) float Bs[ATT_BIAS_LD];
        att_bias_to_lds(Bs, bias, hd, tid, NKT * 64);
        bt = Bs + att_bias_base(qb, lane);
    }
    half8 qh[D / 16], ql[D / 16];  // B operand of S^T: this lane's query row, dims 16 ks + 8 h .. +7
    {
        int qr = qb * 32 + r;
        qr = qr < L ? qr : L - 1;
        const float* qp = qkv + (size_t)(t0 + qr) * ld + hd * D;
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(qp + 16 * ks + 8 * h);
            const f32x4 b = *reinterpret_cast<const f32x4*>(qp + 16 * ks + 8 * h + 4);
            half4 ah, al, bh, bl;
            split_act4(a, ah, al);
            split_act4(b, bh, bl);
            qh[ks] = half8{ah[0], ah[1], ah[2], ah[3], bh[0], bh[1], bh[2], bh[3]};
            ql[ks] = half8{al[0], al[1], al[2], al[3], bl[0], bl[1], bl[2], bl[3]};
        }
    }
    const bool once = KC == NKT || nkt <= KC;  // the whole sequence fits: staged once, K and V
    // key tiles [c0, c0 + KC) -> the LDS planes; rows past L are clamped (masked below / never stored)
    auto stage = [&](int c0, bool with_v) {
        if (!once) __syncthreads();  // the previous chunk's readers are done
        const int nk = (nkt - c0 < KC ? nkt - c0 : KC) * 32;
        auto src_of = [&](int id) {  // item id = (row, 4-dim group) of the chunk
            const int key = c0 * 32 + id / G, rr = key < L ? key : L - 1;
            return qkv + (size_t)(t0 + rr) * ld + hd * D + (id % G) * 4;
        };
        auto put = [&](int id, const f32x4& k, const f32x4& v) {
            const int row = id / G, c = id % G;
            half4 khi, klo;
            split_act4(k, khi, klo);
            if (with_v) {
                half4 vhi, vlo;
                split_act4(v, vhi, vlo);
                *reinterpret_cast<half4*>(Vh + row * D + c * 4) = vhi;
                *reinterpret_cast<half4*>(Vl + row * D + c * 4) = vlo;
            }
            const int off = row * D + ((((c >> 1) ^ att_k_swz(D, row)) << 3) | ((c & 1) << 2));
            *reinterpret_cast<half4*>(Kh + off) = khi;
            *reinterpret_cast<half4*>(Kl + off) = klo;
        };
        if constexpr (PREFETCH) {
            constexpr int STG = KC * 32 * G / (NKT * 64);
            static_assert(KC * 32 * G % (NKT * 64) == 0, "staging: whole rounds");
            f32x4 kreg[STG], vreg[STG];
#pragma unroll
            for (int it = 0; it < STG; ++it) {
                const float* src = src_of(tid + it * NKT * 64);
                kreg[it] = *reinterpret_cast<const f32x4*>(src + H);
                if (with_v) vreg[it] = *reinterpret_cast<const f32x4*>(src + 2 * H);
            }
#pragma unroll
            for (int it = 0; it < STG; ++it)
                if (tid + it * NKT * 64 < nk * G) put(tid + it * NKT * 64, kreg[it], vreg[it]);
        } else {
            for (int id = tid; id < nk * G; id += NKT * 64) {
                const float* src = src_of(id);
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (with_v) v = *reinterpret_cast<const f32x4*>(src + 2 * H);
                put(id, *reinterpret_cast<const f32x4*>(src + H), v);
            }
        }
        __syncthreads();
    };
    // raw scores S' = 256 S of key tile kt (staged from c0) for this wave's 32 queries, keys beyond the sequence at -inf
    // (only the one tile that has any pays for the selects: uniform branch)
    // hi_only (the row-maxima pass): the hi x hi products alone - a third of the MFMAs.  The
    // softmax does not care which shift it is given as long as the exponentials stay in range; this approximate maximum
    // can sit below the true one by at most 2^-10 |q| |k| in score units, the planes of p' = 2^10 p have 2^6 of head room,
    // and the exponent is clamped for whatever lies beyond (|q| |k| > 2.4e4: two hundred times a BERT head's).
    auto score_tile = [&](int kt, int c0, bool hi_only) {
        f32x16 t;
#pragma unroll
        for (int e = 0; e < 16; ++e) t[e] = 0.0f;
        const int row = (kt - c0) * 32 + r;
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) {
            const int off = row * D + (((2 * ks + h) ^ att_k_swz(D, row)) << 3);
            const half8 kh = *reinterpret_cast<const half8*>(Kh + off);
            const half8 kl = *reinterpret_cast<const half8*>(Kl + off);
            t = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], t, 0, 0, 0);
            if (hi_only) continue;
            t = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], t, 0, 0, 0);
        }
        if (kt == nkt - 1 && kt * 32 + 32 > L) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (kt * 32 + acc_row(e, lane) >= L) t[e] = -INFINITY;
        }
        return t;
    };
    // O' += P'.V for key tile kt: pt is a tile of p' = 1024 p in the accumulator layout; o[dt] holds head dims 32 dt + r
    f32x16 o[D / 32];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[dt][e] = 0.0f;
    auto pv_tile = [&](int kt, int c0, const f32x16& pt) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            half8 ph, pl;
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                half2w a, b;
                split_pair_prescaled(pt[8 * ks + j], pt[8 * ks + j + 1], a, b);
                ph[j] = a[0]; ph[j + 1] = a[1];
                pl[j] = b[0]; pl[j + 1] = b[1];
            }
            // this lane's head dim, keys base .. base+3 and base+8 .. base+11: two transposed 4-key x 16-dim blocks per plane
            const int base = (kt - c0) * 32 + 4 * h + 16 * ks;
#pragma unroll
            for (int dt = 0; dt < D / 32; ++dt) {
                const int tr_at = (base + ((lane & 15) >> 2)) * D + 32 * dt + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
                const half4 v0h = lds_read_tr(Vh + tr_at);
                const half4 v1h = lds_read_tr(Vh + tr_at + 8 * D);
                const half4 v0l = lds_read_tr(Vl + tr_at);
                const half4 v1l = lds_read_tr(Vl + tr_at + 8 * D);
                const half8 vh = {v0h[0], v0h[1], v0h[2], v0h[3], v1h[0], v1h[1], v1h[2], v1h[3]};
                const half8 vl = {v0l[0], v0l[1], v0l[2], v0l[3], v1l[0], v1l[1], v1l[2], v1l[3]};
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, vh, o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, vl, o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pl, vh, o[dt], 0, 0, 0);
            }
        }
    };
    // every key tile of the sequence, chunk by chunk (one chunk when the sequence was staged whole)
    auto for_tiles = [&](bool with_v, auto&& f) {
#pragma unroll
        for (int c0 = 0; c0 < NKT; c0 += KC) {
            if (c0 < nkt) {
                if (!once) stage(c0, with_v);
                if (active) {
#pragma unroll
                    for (int j = 0; j < KC; ++j)
                        if (c0 + j < nkt) f(c0 + j, c0);
                }
            }
        }
    };
    typedef float float2w __attribute__((ext_vector_type(2)));
    const float cs = scale_log2e * (1.0f / 256.0f);  // scores in log2 units from S' = 256 S
    // Softmax on the raw scores (S' = 256 S): the maximum is taken before scaling, and scale, shift and the 2^10 factor
    // of p' = 1024 p go into one fma in front of the exponential: p' = 2^(S' cs - max' cs + 10).
    // BIAS: the logit in log2 units is v = S' cs + bias, one fma; the maximum is taken over v (a maximum over S' alone
    // would let a large bias on a small logit run past every head room), and p' = 2^(v - max + 10).  On the hi x hi
    // maximum of the RECOMP form the exponent clamp still covers what the two dropped products add, as without a bias.
    auto biased = [&](f32x16& t, int kt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) t[e] = fmaf(t[e], cs, bt[kt * 32 + (e & 3) + 8 * (e >> 2)]);
    };
    // row sums l' = sum_k p'_k: two interleaved chains per lane (packed adds), the halves of a row joined by a shuffle
    float2w ls2 = float2w{0.0f, 0.0f};
    auto join_rows = [&]() {
        const float lrow = join_halves(ls2[0] + ls2[1], h);
        if (h == 0) Ls[wave * 32 + r] = lrow;  // read back by this wave's own lanes only
    };
    if (once) stage(0, true);
    if constexpr (RECOMP) {
        float mx = -INFINITY;
        for_tiles(false, [&](int kt, int c0) {
            f32x16 t = score_tile(kt, c0, true);
            if constexpr (BIAS) biased(t, kt);
#pragma unroll
            for (int e = 0; e < 16; ++e) mx = fmaxf(mx, t[e]);
        });
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float shift = BIAS ? 10.0f - mx : fmaf(-mx, cs, 10.0f);
        for_tiles(true, [&](int kt, int c0) {
            f32x16 t = score_tile(kt, c0, false);
            if constexpr (BIAS) {
                biased(t, kt);
#pragma unroll
                for (int e = 0; e < 16; ++e) t[e] = __builtin_amdgcn_exp2f(fminf(t[e] + shift, 15.9f));
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) t[e] = __builtin_amdgcn_exp2f(fminf(fmaf(t[e], cs, shift), 15.9f));
            }
#pragma unroll
            for (int e = 0; e < 16; e += 2) ls2 = ls2 + float2w{t[e], t[e + 1]};
            pv_tile(kt, c0, t);
        });
        if (active) join_rows();
    } else if (active) {
        f32x16 sc[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt < nkt) {
                sc[kt] = score_tile(kt, 0, false);
                if constexpr (BIAS) biased(sc[kt], kt);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt < nkt) {
#pragma unroll
                for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sc[kt][e]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float shift = BIAS ? 10.0f - mx : fmaf(-mx, cs, 10.0f);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt < nkt) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    sc[kt][e] = __builtin_amdgcn_exp2f(BIAS ? sc[kt][e] + shift : fmaf(sc[kt][e], cs, shift));
            }
        }
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt < nkt) {
#pragma unroll
                for (int e = 0; e < 16; e += 2) ls2 = ls2 + float2w{sc[kt][e], sc[kt][e + 1]};
            }
        }
        join_rows();
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
            if (kt < nkt) pv_tile(kt, 0, sc[kt]);
    }
    if (PARK) __syncthreads();  // every wave has left the K planes: they become the output tiles
    if (!active) return;
    // normalise, split into the hi / lo planes and store: PARK row-major into the wave's LDS tile, else to memory
    _Float16* const ob = Kbuf + wave * (2 * 32 * D);
#pragma unroll
    for (int e = 0; e < 16; e += 2) {
        const int q0 = acc_row(e, lane), q1 = acc_row(e + 1, lane);
        const float s0 = 0.0625f * __builtin_amdgcn_rcpf(Ls[wave * 32 + q0]);
        const float s1 = 0.0625f * __builtin_amdgcn_rcpf(Ls[wave * 32 + q1]);
        const int tq0 = qb * 32 + q0, tq1 = qb * 32 + q1;
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
            half2w hi, lo;
            split_pair_prescaled(o[dt][e] * s0 * WT_SA, o[dt][e + 1] * s1 * WT_SA, hi, lo);
            const int c = 32 * dt + r;
            if constexpr (PARK) {
                ob[q0 * D + c] = hi[0];
                ob[q1 * D + c] = hi[1];
                ob[32 * D + q0 * D + c] = lo[0];
                ob[32 * D + q1 * D + c] = lo[1];
            } else {
                if (tq0 < L) {
                    ch[(size_t)(t0 + tq0) * H + hd * D + c] = hi[0];
                    cl[(size_t)(t0 + tq0) * H + hd * D + c] = lo[0];
                }
                if (tq1 < L) {
                    ch[(size_t)(t0 + tq1) * H + hd * D + c] = hi[1];
                    cl[(size_t)(t0 + tq1) * H + hd * D + c] = lo[1];
                }
            }
        }
    }
    if constexpr (PARK) {
#pragma unroll
        for (int t = 0; t < D / 16; ++t) {
            const int id = lane + 64 * t, qrow = id / (D / 8), c8 = (id % (D / 8)) * 8;
            const int tq = qb * 32 + qrow;
            if (tq < L) {
                const size_t at = (size_t)(t0 + tq) * H + hd * D + c8;
                *reinterpret_cast<u32x4*>(ch + at) = *reinterpret_cast<const u32x4*>(ob + qrow * D + c8);
                *reinterpret_cast<u32x4*>(cl + at) = *reinterpret_cast<const u32x4*>(ob + 32 * D + qrow * D + c8);
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
    float* att_bias = nullptr;  // icrec_encoder_set_attention_bias: [heads][ATT_BIAS_LD] in log2 units, or none
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
    // Side stream + events of one caller stream: the short remainder of a large batch (batch_tail) and the shorter
    // attention buckets run beside the batch kernels of the same layer instead of behind them.  One set per caller
    // stream (created on first use, kept for the encoder's life), so that concurrent icrec_encode calls on different
    // streams - DeviceEncoder runs the two halves of a batch that way - do not queue behind each other's side work.
    // Every fork and join records `ev` and waits on it at once (link), so one event serves them all.
    struct Side {
        hipStream_t caller = nullptr, side = nullptr;
        hipEvent_t ev = nullptr;
    };
    std::mutex side_mu;
    std::vector<Side*> sides;
};

static int side_for(Encoder* e, hipStream_t caller, Encoder::Side** out) {
    std::lock_guard<std::mutex> lock(e->side_mu);
    *out = nullptr;
    for (Encoder::Side* sd : e->sides)
        if (sd->caller == caller) { *out = sd; return ICREC_OK; }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (caller && hipStreamIsCapturing(caller, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return ICREC_OK;  // no stream / event creation inside a capture: the call stays on the caller's stream
    Encoder::Side* sd = new Encoder::Side();
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

// A CLS-pooled f16x3 encoder reads row cu[s] of the last hidden state and nothing else: its last layer runs attention for
// query block 0 of each (sequence, head) and the post-attention chain over n_seqs compact rows (encode_x3), which take
// their scratch from the caller's workspace behind the call's own regions.
static bool cls_prunes(const Encoder* e) {
    return e->pooling == ICREC_POOL_CLS && e->cls_prune && e->cfg.gemm_mode == ICREC_GEMM_F16X3;
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

// The attention length buckets, in launch order: 9-16 key tiles first (257-512 tokens: the longest bucket starts first),
// then from the shortest up.  f16x3 batches over 32-dim heads take 5-8 key tiles in two buckets; single sequences, fp32
// and 64-dim heads in one.
// Bucket k serves [ATT_LO[k], ATT_HI[k]] key tiles with the kernel <NKT = ATT_HI[k]> (NKT waves per workgroup).
enum AttBucket { ATT_9_16, ATT_1, ATT_2, ATT_3_4, ATT_5_6, ATT_7_8, ATT_5_8, ATT_N };
constexpr int ATT_LO[ATT_N] = {9, 1, 2, 3, 5, 7, 5}, ATT_HI[ATT_N] = {16, 1, 2, 4, 6, 8, 8};

// Launch, in AttBucket order, the buckets in `mask` (bits 1 << AttBucket) that the call needs: for a batch every bucket
// that can occur for max_seqlen (one whose workgroups all exit costs a few microseconds), else the one that holds it.
// X3: the f16x3 kernel, context out as planes (attention_x3_kernel); otherwise exact fp32 rows (attention_kernel).
// block0_only (X3): query block 0 of every (sequence, head) alone - the pruned last layer of a CLS-pooled encoder.
// bias: the encoder's relative-position table (the kernels' BIAS arm), or nullptr: the launches of an encoder without one.
template <bool X3>
static void launch_attention(unsigned mask, const icrec_bert_cfg& c, const EncBufs& b, const int32_t* cu, int n_seqs,
                             int max_seqlen, const int32_t* order, const float* bias, hipStream_t st,
                             bool block0_only = false) {
    const int nkt_max = (max_seqlen + 31) / 32;
    const int dh = c.hidden / c.heads;  // 32 or 64 (icrec_encoder_create)
    const bool single = n_seqs == 1, split_5_8 = X3 && !single && dh == 32;
    const float sl2e = (1.0f / sqrtf((float)dh)) * 1.44269504088896340736f;
    for (int k = 0; k < ATT_N; ++k) {
        if (!(mask >> k & 1) || (split_5_8 ? k == ATT_5_8 : k == ATT_5_6 || k == ATT_7_8) || nkt_max < ATT_LO[k] ||
            (single && nkt_max > ATT_HI[k]))
            continue;
        const dim3 grid(n_seqs * c.heads), block(ATT_HI[k] * 64);
        if constexpr (X3) {  // (only 32-dim heads split 5-8 key tiles)
#define ICREC_ATT_ROW(K, D, B) {K<D, 16, B>, K<D, 1, B>, K<D, 2, B>, K<D, 4, B>, D == 32 ? K<32, 6, B> : nullptr, D == 32 ? K<32, 8, B> : nullptr, K<D, 8, B>}
            static const decltype(&attention_x3_kernel<32, 1>) kern[2][2][ATT_N] = {
                {ICREC_ATT_ROW(attention_x3_kernel, 32, false), ICREC_ATT_ROW(attention_x3_kernel, 64, false)},
                {ICREC_ATT_ROW(attention_x3_kernel, 32, true), ICREC_ATT_ROW(attention_x3_kernel, 64, true)}};
#undef ICREC_ATT_ROW
            hipLaunchKernelGGL(kern[bias != nullptr][dh == 64][k], grid, block, 0, st, b.qkv, cu, c.heads, c.hidden, sl2e,
                               b.ch, b.cl, order, ATT_LO[k] - 1, block0_only ? 1 : ATT_HI[k], bias);
        } else {
#define ICREC_ATT_ROW(D, B) {attention_kernel<D, 16, B>, attention_kernel<D, 1, B>, attention_kernel<D, 2, B>, attention_kernel<D, 4, B>, nullptr, nullptr, attention_kernel<D, 8, B>}
            static const decltype(&attention_kernel<32, 1>) kern[2][2][ATT_N] = {
                {ICREC_ATT_ROW(32, false), ICREC_ATT_ROW(64, false)}, {ICREC_ATT_ROW(32, true), ICREC_ATT_ROW(64, true)}};
#undef ICREC_ATT_ROW
            hipLaunchKernelGGL(kern[bias != nullptr][dh == 64][k], grid, block, 0, st, b.qkv, cu, c.heads, c.hidden, sl2e,
                               b.ctx, ATT_LO[k] - 1, bias);
        }
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
    {
        const char* fuse_env = getenv("ICREC_FUSE");
        const char* side_env = getenv("ICREC_SIDE_STREAM");
        e->fuse = !(fuse_env && fuse_env[0] == '0');
        e->small_m = env_knob("ICREC_SMALL_M", e->small_m, SMALL_M_MAX);
        e->tail_m = env_knob("ICREC_TAIL_M", e->tail_m, 64LL * e->n_cu - 1);
        e->side_stream = !(side_env && side_env[0] == '0');
        const char* prune_env = getenv("ICREC_CLS_PRUNE");
        e->cls_prune = !(prune_env && prune_env[0] == '0');
    }
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
    for (Encoder::Side* sd : e->sides) {  // (side_for keeps a side only once its stream and event exist)
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
    std::vector<float> tab((size_t)heads * ATT_BIAS_LD, 0.0f);
    for (int hd = 0; hd < heads; ++hd)
        for (int i = 0; i < N; ++i) {
            const float v = bias_host[(size_t)hd * N + i];
            ICREC_REQUIRE(v - v == 0.0f, "icrec_encoder_set_attention_bias: entry [%d][%d] is not finite", hd, i);
            tab[(size_t)hd * ATT_BIAS_LD + i] = (float)((double)v * 1.44269504088896340736);
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

// The call's own regions, then (cls_prunes) the compact rows' of the pruned last layer.
static size_t workspace_bytes(const Encoder* e, int64_t T, int n_seqs) {
    return enc_ws(e->cfg, T).total + (cls_prunes(e) ? enc_ws(e->cfg, n_seqs, true).total : 0);
}

size_t icrec_encode_workspace_bytes(const icrec_encoder* h, int64_t total_tokens, int32_t n_seqs) {
    const Encoder* e = reinterpret_cast<const Encoder*>(h);
    if (!e || total_tokens < 1 || n_seqs < 1) return 0;
    return workspace_bytes(e, total_tokens, n_seqs);
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

// Embeddings + LayerNorm.  f16x3 mode leaves the fp32 x region unused (the residual stream is its two planes): it carries
// the attention dispatch order of batches, returned here (nullptr: workgroup b serves sequence b / heads, as unfused).
// seg_b_dev (icrec_score_pairs): each sequence's first position of token type 1 - the kernel's SEG arm; nullptr: type 0.
static const int32_t* embed(const Encoder* e, const EncBufs& b, const int32_t* ids_dev, const int32_t* cu_dev,
                            const int32_t* seg_b_dev, int n_seqs, int T, hipStream_t st) {
    const icrec_bert_cfg& c = e->cfg;
    const bool x3 = c.gemm_mode == ICREC_GEMM_F16X3;
    int32_t* order = nullptr;
    if (x3 && n_seqs >= 64 && e->fuse) {
        order = reinterpret_cast<int32_t*>(b.x);
        hipLaunchKernelGGL(seq_order_kernel, dim3(1), dim3(1024), 0, st, cu_dev, n_seqs, order);
    }
    auto kern =
        for_hidden(c.hidden, [x3](auto h) { return x3 ? embed_ln_kernel<h(), true> : embed_ln_kernel<h(), false>; });
    if (seg_b_dev)
        kern = for_hidden(c.hidden, [x3](auto h) { return x3 ? embed_ln_kernel<h(), true, true> : embed_ln_kernel<h(), false, true>; });
    hipLaunchKernelGGL(kern, dim3((T + 3) / 4), dim3(256), 0, st, ids_dev, cu_dev, n_seqs, T, e->word, e->pos, e->type, e->eg, e->eb, c.ln_eps, c.vocab_size,
                       c.max_position, b.x, b.xh, b.xl, seg_b_dev);
    return order;
}

// One fork or join: work enqueued on `to` from here on runs behind everything enqueued on `from` so far.
static hipError_t link(const Encoder::Side* sd, hipStream_t from, hipStream_t to) {
    const hipError_t err = hipEventRecord(sd->ev, from);
    return err != hipSuccess ? err : hipStreamWaitEvent(to, sd->ev, 0);
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

// cls: the compact rows' regions when the last layer is pruned to each sequence's first token (cls_prunes), else nullptr.
// The last hidden state is then rows [0, n_seqs) of cls->xh / cls->xl and b's x planes stay one layer behind.
static int encode_x3(Encoder* e, const EncBufs& b, const EncBufs* cls, const int32_t* cu_dev, int n_seqs, int T,
                     int max_seqlen, const int32_t* order, hipStream_t st) {
    const icrec_bert_cfg& c = e->cfg;
    const int H = c.hidden, I = c.intermediate;
    const auto ln_wt = for_hidden(H, [](auto h) { return ln_wt_kernel<h()>; });
    const bool split_att = H == HID && e->side_stream && n_seqs >= 64 && max_seqlen > 128;  // batches with a long bucket
    // Token ranges: [0, T_main) goes through the batch kernels in whole rounds of one 64-token workgroup per CU, a short
    // remainder [T_main, T) through the small-batch kernels (same arithmetic, same bits) instead of costing every batch
    // kernel an extra, almost empty round.
    const int T_tail = batch_tail(e, T), T_main = T - T_tail;
    Encoder::Side* sd = nullptr;
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
        if (split_att && sd) {
            // the long bucket keeps one 8-wave workgroup per CU busy (LDS) with issue slots to spare: the shorter
            // buckets' workgroups run beside it from the side stream instead of after it (sequences of 9-16 key tiles:
            // that bucket goes first, on the caller's stream, ahead of the side stream's)
            ICREC_HIP(link(sd, st, sd->side));
            const unsigned side_buckets = 1u << ATT_1 | 1u << ATT_2 | 1u << ATT_3_4 | 1u << ATT_7_8;
            launch_attention<true>(1u << ATT_9_16, c, b, cu_dev, n_seqs, max_seqlen, order, e->att_bias, st, pruned);
            launch_attention<true>(side_buckets, c, b, cu_dev, n_seqs, max_seqlen, order, e->att_bias, sd->side, pruned);
            launch_attention<true>(1u << ATT_5_6, c, b, cu_dev, n_seqs, max_seqlen, order, e->att_bias, st, pruned);
            ICREC_HIP(link(sd, sd->side, st));
        } else {
            launch_attention<true>(~0u, c, b, cu_dev, n_seqs, max_seqlen, order, e->att_bias, st, pruned);
        }
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
    for (int l = 0; l < c.layers; ++l) {
        const LayerW& L = e->layers[l];
        launch_linear<false>(b.x, T, H, L.Wqkv, 3 * H, L.bqkv, b.qkv, st);
        launch_attention<false>(~0u, c, b, cu_dev, n_seqs, max_seqlen, nullptr, e->att_bias, st);
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
    ICREC_REQUIRE(n_seqs >= 1 && T64 >= n_seqs && T64 < (1ll << 31), "icrec_encode: bad n_seqs/total_tokens (%d, %lld)", n_seqs, (long long)T64);
    ICREC_REQUIRE(max_seqlen >= 1 && max_seqlen <= e->max_seqlen, "icrec_encode: max_seqlen must be in [1, %d] (got %d)", e->max_seqlen, max_seqlen);
    const int T = (int)T64;
    const EncWs w = enc_ws(e->cfg, T);
    const size_t need = workspace_bytes(e, T, n_seqs);
    if (!ws || ws_bytes < need) {
        set_error("icrec_encode: workspace too small (%zu < %zu)", ws_bytes, need);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    ScopedTimer whole(T_ENCODE, st);
    char* base = reinterpret_cast<char*>(ws);
    const icrec_bert_cfg& c = e->cfg;
    const int H = c.hidden;
    const bool x3 = c.gemm_mode == ICREC_GEMM_F16X3;
    const EncBufs b(base, w, c, T);
    // The last layer is pruned to each sequence's first token when nothing else of it is read: not when the caller
    // wants every token's state, and not when every token is a first token (nothing to save).
    const bool pruned = cls_prunes(e) && !tokens_out_dev && n_seqs < T;
    const EncBufs cls(base + w.total, enc_ws(c, n_seqs, true), c, n_seqs);  // (inside the workspace only if cls_prunes)
    const int32_t* order = embed(e, b, ids_dev, cu_dev, nullptr, n_seqs, T, st);
    if (int rc_ = x3 ? encode_x3(e, b, pruned ? &cls : nullptr, cu_dev, n_seqs, T, max_seqlen, order, st)
                     : encode_f32(e, b, cu_dev, n_seqs, T, max_seqlen, st))
        return rc_;
    const auto pool =
        for_hidden(H, [x3](auto h) { return x3 ? pool_norm_kernel<h(), true> : pool_norm_kernel<h(), false>; });
    const EncBufs& last = pruned ? cls : b;  // where the last hidden state of the pooled rows is
    const int pool_rows = e->pooling != ICREC_POOL_CLS ? POOL_ROWS_MEAN : pruned ? POOL_ROWS_CLS_COMPACT : POOL_ROWS_CLS;
    hipLaunchKernelGGL(pool, dim3(n_seqs), dim3(H), 0, st, last.x, last.xh, last.xl, cu_dev, c.n_normalize, out_dev,
                       pool_rows);
    if (tokens_out_dev) {  // hidden is a multiple of 4: every thread's 4 features are 16 (planes: 8) bytes, aligned
        const size_t n4 = (size_t)T * H / 4;
        hipLaunchKernelGGL(x3 ? tokens_out_kernel<true> : tokens_out_kernel<false>, dim3((unsigned)((n4 + 255) / 256)),
                           dim3(256), 0, st, b.x, b.xh, b.xl, n4, tokens_out_dev);
    }
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

// A pair's score reads row cu[s] of the last hidden state and nothing else, whatever the handle's pooling mode: in f16x3
// mode the last layer is pruned as a CLS-pooled encoder's is, its compact rows behind the call's own regions.
static bool score_prunes(const Encoder* e) { return e->cls_prune && e->cfg.gemm_mode == ICREC_GEMM_F16X3; }

size_t icrec_score_pairs_workspace_bytes(const icrec_encoder* h, int64_t total_tokens, int32_t n_seqs) {
    const Encoder* e = reinterpret_cast<const Encoder*>(h);
    if (!e || total_tokens < 1 || n_seqs < 1) return 0;
    return enc_ws(e->cfg, total_tokens).total + (score_prunes(e) ? enc_ws(e->cfg, n_seqs, true).total : 0);
}

int icrec_score_pairs(icrec_encoder* h, const int32_t* ids_dev, const int32_t* cu_dev, const int32_t* seg_b_dev,
                      int32_t n_seqs, int64_t T64, int32_t max_seqlen, float* scores_out_dev, void* ws, size_t ws_bytes,
                      void* stream) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    ICREC_REQUIRE(e && ids_dev && cu_dev && seg_b_dev && scores_out_dev, "icrec_score_pairs: NULL argument");
    ICREC_REQUIRE(e->score_head, "icrec_score_pairs: the encoder has no score head (icrec_encoder_set_score_head)");
    ICREC_REQUIRE(n_seqs >= 1 && T64 >= n_seqs && T64 < (1ll << 31), "icrec_score_pairs: bad n_seqs/total_tokens (%d, %lld)", n_seqs, (long long)T64);
    ICREC_REQUIRE(max_seqlen >= 1 && max_seqlen <= e->max_seqlen, "icrec_score_pairs: max_seqlen must be in [1, %d] (got %d)", e->max_seqlen, max_seqlen);
    const int T = (int)T64;
    const size_t need = icrec_score_pairs_workspace_bytes(h, T, n_seqs);
    if (!ws || ws_bytes < need) {
        set_error("icrec_score_pairs: workspace too small (%zu < %zu)", ws_bytes, need);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    const icrec_bert_cfg& c = e->cfg;
    const int H = c.hidden;
    const bool x3 = c.gemm_mode == ICREC_GEMM_F16X3;
    const EncWs w = enc_ws(c, T);
    const EncBufs b(base, w, c, T);
    const bool pruned = score_prunes(e) && n_seqs < T;  // (every token a first token: nothing to save)
    const EncBufs cls(base + w.total, enc_ws(c, n_seqs, true), c, n_seqs);  // (inside the workspace only if score_prunes)
    const int32_t* order = embed(e, b, ids_dev, cu_dev, seg_b_dev, n_seqs, T, st);
    if (int rc_ = x3 ? encode_x3(e, b, pruned ? &cls : nullptr, cu_dev, n_seqs, T, max_seqlen, order, st)
                     : encode_f32(e, b, cu_dev, n_seqs, T, max_seqlen, st))
        return rc_;
    const EncBufs& last = pruned ? cls : b;
    const float *const wpt = e->score_head, *const bp = wpt + (size_t)H * H, *const wc = bp + H, *const bc = wc + H;
    const auto kern =
        for_hidden(H, [x3](auto h) { return x3 ? score_head_kernel<h(), true> : score_head_kernel<h(), false>; });
    const int per_wg = H == HID_BASE ? HEAD_SEQS<HID_BASE> : HEAD_SEQS<HID>;
    hipLaunchKernelGGL(kern, dim3((n_seqs + per_wg - 1) / per_wg), dim3(384), 0, st, last.x, last.xh, last.xl, cu_dev,
                       n_seqs, pruned, wpt, bp, wc, bc, scores_out_dev);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

}  // extern "C"
