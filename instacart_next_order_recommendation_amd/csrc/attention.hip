// attention.hip — self-attention of the encoder on gfx950 (interface: attention.h): the exact fp32 kernel and the f16x3
// kernel, for 32- and 64-dim heads, with and without a relative-position bias; the dispatch order of their
// workgroups; the length buckets, their launch order and their split over the caller's stream and a side stream.
// Arithmetic follows transformers/models/bert/modeling_bert.py (tf:) and oracle/icrec_oracle.c's attention block.
#include "attention.h"
#include "wt_gemm.h"

namespace icrec {

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
static_assert(ATT_BIAS_LD == AttentionArgs::BIAS_LD, "the row length attention.h documents for the bias table");
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

// ---------------------------------------------------------------- host side: buckets, launches, streams
// The attention length buckets, in launch order: 9-16 key tiles first (257-512 tokens: the longest bucket starts first),
// then from the shortest up.  f16x3 batches over 32-dim heads take 5-8 key tiles in two buckets; single sequences, fp32
// and 64-dim heads in one.
// Bucket k serves [ATT_LO[k], ATT_HI[k]] key tiles with the kernel <NKT = ATT_HI[k]> (NKT waves per workgroup).
enum AttBucket { ATT_9_16, ATT_1, ATT_2, ATT_3_4, ATT_5_6, ATT_7_8, ATT_5_8, ATT_N };
constexpr int ATT_LO[ATT_N] = {9, 1, 2, 3, 5, 7, 5}, ATT_HI[ATT_N] = {16, 1, 2, 4, 6, 8, 8};

// The kernel of one arithmetic - X3: attention_x3_kernel, else attention_kernel (only the one asked for is instantiated) -
// and, for the two buckets that split 5-8 key tiles, the kernel where there is one: f16x3 over 32-dim heads.
template <bool X3, int D, int NKT, bool B>
constexpr auto att_kernel() {
    if constexpr (X3) return attention_x3_kernel<D, NKT, B>;
    else return attention_kernel<D, NKT, B>;
}
template <bool X3, int D, int NKT, bool B>
constexpr decltype(att_kernel<X3, D, 8, B>()) att_split_kernel() {
    if constexpr (X3 && D == 32) return att_kernel<X3, D, NKT, B>();
    else return nullptr;
}

// Launch, in AttBucket order, the buckets in `mask` (bits 1 << AttBucket) that the call needs: for a batch every bucket
// that can occur for max_seqlen (one whose workgroups all exit costs a few microseconds), else the one that holds it.
// X3: the f16x3 kernel, context out as planes (attention_x3_kernel); otherwise exact fp32 rows (attention_kernel).
template <bool X3>
static void launch_attention(unsigned mask, const AttentionArgs& a, hipStream_t st) {
    const int nkt_max = (a.max_seqlen + 31) / 32;
    const int dh = a.hidden / a.heads;  // 32 or 64 (icrec_encoder_create)
    const bool single = a.n_seqs == 1, split_5_8 = X3 && !single && dh == 32;
    const float sl2e = (1.0f / sqrtf((float)dh)) * 1.44269504088896340736f;
#define ICREC_ATT_ROW(D, B) {att_kernel<X3, D, 16, B>(), att_kernel<X3, D, 1, B>(), att_kernel<X3, D, 2, B>(), att_kernel<X3, D, 4, B>(), att_split_kernel<X3, D, 6, B>(), att_split_kernel<X3, D, 8, B>(), att_kernel<X3, D, 8, B>()}
    static const decltype(att_kernel<X3, 32, 1, false>()) kern[2][2][ATT_N] = {
        {ICREC_ATT_ROW(32, false), ICREC_ATT_ROW(64, false)}, {ICREC_ATT_ROW(32, true), ICREC_ATT_ROW(64, true)}};
#undef ICREC_ATT_ROW
    for (int k = 0; k < ATT_N; ++k) {
        if (!(mask >> k & 1) || (split_5_8 ? k == ATT_5_8 : k == ATT_5_6 || k == ATT_7_8) || nkt_max < ATT_LO[k] ||
            (single && nkt_max > ATT_HI[k]))
            continue;
        const dim3 grid(a.n_seqs * a.heads), block(ATT_HI[k] * 64);
        const auto kernel = kern[a.bias != nullptr][dh == 64][k];
        if constexpr (X3)
            hipLaunchKernelGGL(kernel, grid, block, 0, st, a.qkv, a.cu, a.heads, a.hidden, sl2e, a.ch, a.cl, a.order,
                               ATT_LO[k] - 1, a.block0_only ? 1 : ATT_HI[k], a.bias);
        else
            hipLaunchKernelGGL(kernel, grid, block, 0, st, a.qkv, a.cu, a.heads, a.hidden, sl2e, a.ctx, ATT_LO[k] - 1,
                               a.bias);
    }
}

bool attention_wants_side(const AttentionArgs& a) {  // batches with a long bucket, over 32-dim heads
    return a.hidden / a.heads == 32 && a.n_seqs >= 64 && a.max_seqlen > 128;
}

int run_attention(const AttentionArgs& a, hipStream_t st, const SideStream* sd) {
    if (a.ctx) {
        launch_attention<false>(~0u, a, st);
    } else if (!sd) {
        launch_attention<true>(~0u, a, st);
    } else {
        // the long bucket keeps one 8-wave workgroup per CU busy (LDS) with issue slots to spare: the shorter
        // buckets' workgroups run beside it from the side stream instead of after it (sequences of 9-16 key tiles:
        // that bucket goes first, on the caller's stream, ahead of the side stream's)
        ICREC_HIP(link(sd, st, sd->side));
        launch_attention<true>(1u << ATT_9_16, a, st);
        launch_attention<true>(1u << ATT_1 | 1u << ATT_2 | 1u << ATT_3_4 | 1u << ATT_7_8, a, sd->side);
        launch_attention<true>(1u << ATT_5_6, a, st);
        ICREC_HIP(link(sd, sd->side, st));
    }
    return ICREC_OK;
}

void attention_dispatch_order(const int32_t* cu, int n_seqs, int32_t* order, hipStream_t st) {
    hipLaunchKernelGGL(seq_order_kernel, dim3(1), dim3(1024), 0, st, cu, n_seqs, order);
}

}  // namespace icrec
