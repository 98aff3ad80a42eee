// search.hip — cosine scoring fused with per-query top-k selection (no score matrix is ever written): the score +
// select kernels, the filter + verify path, and their planning: what a search launches.  The partial lists are merged
// by sort.hip's sorters (common.h); the index handle's life cycle is index.hip's, and what the handle keeps per row -
// the filter copy this file reads included - is written by storage.hip (storage.h).
//
// Replaces, on the device:
//   sentence_transformers.util.cos_sim(query_emb, product_embeddings)  serve_recommendations.py:214/:250
//   scores.argsort(descending=True)                                      :215/:251
//   the exclusion / top-k Python loop                                    :216-225/:254-262
// of the reference's src/inference/serve_recommendations.py.
#include "common.h"
#include "storage.h"
#include "stream.h"

namespace icrec {

// (row normalisation, the exclusion search and the facet test live in index.h: boost.hip uses them too; split_planes_kernel,
// which splits the staged pass's queries as storage.hip splits the rows, in storage.h)

// ---------------------------------------------------------------- score + select

// (merge_queue, the fold of one query's candidate queue into its sorted list, lives in stream.h: ivf.hip uses it too)

// Two queries per call for k <= 32 and queues of <= 32 slots: lanes 0-31 merge query qa, lanes 32-63 query qb
// (nb == 0: no partner).  Same ranking rule as merge_queue; the ballot's two halves serve the two queries.  Also
// publishes the new thresholds and clears the queue counters.
__device__ __forceinline__ void merge_queue2(u64* list, const u64* queue, int qcap, int qa, int na, int qb, int nb, int k,
                                             int lane, u64* thr, int* cnt) {
    // Two queries per call (k, n <= 32): lanes 0-31 merge query qa, lanes 32-63 query qb.  Lane l holds list entry l and
    // candidate l of its query; every element's new position is its rank in the union (keys are unique):
    //   list entry:  l + #{candidates better than it}
    //   candidate:   #{candidates better than it} + #{list entries better than it}
    // The candidate counts come from ONE pass over the query's queue in LDS (the 32 lanes of a half read the same
    // address: a broadcast), the list count from a binary search (the list is sorted, best first, empty slots = 0 last).
    // (Round 2 broadcast the candidates with v_readlane and counted with ballots: ~5 k cycles per call against ~1 k.)
    const int half = lane >> 5, l = lane & 31;
    const int q = half ? qb : qa, n = half ? nb : na;
    u64* lst = list + (size_t)q * k;
    const u64* qp = queue + (size_t)q * qcap;
    const u64 c = l < n ? qp[l] : 0ull;
    const u64 e0 = l < k ? lst[l] : 0ull;
    int rc = 0, r0 = 0;
    const int nmax = na > nb ? na : nb;
    for (int i0 = 0; i0 < nmax; i0 += 8) {  // eight reads in flight (one dependent read per candidate is all latency)
        u64 ci[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) ci[u] = qp[i0 + u];  // inside the queue (qcap is 16 or 32, nmax <= qcap), possibly stale
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const u64 v = i0 + u < n ? ci[u] : 0ull;  // 0 past this query's own count: compares false everywhere
            rc += v > c;
            r0 += v > e0;
        }
    }
    int lc = 0;  // number of list entries better than c = the first index whose entry is not
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const int probe = lc + step;
        if (probe <= k && lst[probe - 1] > c) lc = probe;
    }
    if (n > 0) {
        const int pc = rc + lc, p0 = l + r0;
        // all reads above are complete (their values are consumed) before any lane writes
        if (l < n && pc < k) lst[pc] = c;
        if (l < k && p0 < k) lst[p0] = e0;
        if (l == 0) { thr[q] = lst[k - 1]; cnt[q] = 0; }
    }
}

// ---- per-query top-k selection, shared by the tiled search kernels
// A block scores tiles of catalog rows against its BN queries; offer() takes one tile's scores in the accumulator map
// of the 32x32 MFMA (acc[TM][TN]: this wave's row tiles wm, query tiles wn) and keeps, per query, the k best
// (score, row) keys seen in a sorted LDS list; write() stores the lists.  The LDS carve follows the kernel's operand
// staging (all offsets multiples of 16 B): thresholds [BN] | queue counters [BN] | flags [4] | FACET: allow masks
// [BN][FACET_LDS_WORDS], facet words of the current and the next tile [2][BM] | SETS: the queries' slots [BN] (int4),
// set words of the current and the next tile [2][BM / 32][BN] | lists [BN][k] | candidate queues [BN][qcap].
//
// Candidate queue entries per query (qcap): 64 for 32-query tiles, 16 for wider ones.  The resident filter pass takes
// 32 when the lists are short (k <= 32) and a block walks few rounds: the first rounds of a block offer 16-48
// candidates per query and would otherwise take two or three offer / merge iterations each - at 49,688 rows x 1,024
// queries those rounds are most of the kernel (0.274 -> 0.229 ms, same box); blocks that walk thousands of rounds
// keep 16 (10 M rows: 1 % faster with it).
constexpr int RES_QCAP_MAX_ROUNDS = 64;

template <class Cfg, bool RESIDENT = false, bool FACET = false, bool SETS = false>
struct TopK {
    static_assert(FACET || !SETS, "the SETS arm applies the facet test too");
    // SETS: one word per (query, 32 rows) of a tile, SET_NSW of them staged by every thread
    static constexpr int SET_TILE_WORDS = Cfg::BM / 32 * Cfg::BN, SET_NSW = SET_TILE_WORDS / Cfg::THREADS;
    static_assert(SET_TILE_WORDS % Cfg::THREADS == 0 && Cfg::THREADS % Cfg::BN == 0, "whole words per thread, all of one query");
    static __host__ __device__ constexpr int qcap(int k, int rounds) {
        return RESIDENT && k <= 32 && rounds <= RES_QCAP_MAX_ROUNDS ? 32 : Cfg::BN <= 32 ? 64 : 16;
    }
    // LDS of the selection, sized for a block of one round (the largest queue)
    static __host__ __device__ size_t bytes(int k) {
        return (size_t)Cfg::BN * (8 /*thr*/ + 4 /*cnt*/) + 16 /*flags*/ + (FACET ? Cfg::BN * FACET_LDS_WORDS * 4 + 2 * Cfg::BM * 2 : 0) +
               (SETS ? Cfg::BN * 16 + 2 * SET_TILE_WORDS * 4 : 0) +
               (size_t)Cfg::BN * k * 8 + (size_t)Cfg::BN * qcap(k, 1) * 8;
    }

    u64* thr;    // per query: the k-th key of its list, the offer threshold (~0: padding query)
    int* cnt;    // per query: candidates in its queue
    int* flags;  // [0],[1]: alternating "some candidate did not fit" flags; [2]: some lane's query is cold
    u64* list;   // [BN][k], sorted best first, 0 = empty slot
    u64* queue;  // [BN][qcap]
    uint32_t* amask;        // FACET: the queries' allow masks
    uint16_t* ftile;        // FACET: [2][BM] facet words of the tile being offered (half fcur) and of the one after it
    const uint16_t* frows;  // FACET: the index's facet words
    int fcur = 0;
    int4* sslot;            // SETS: the queries' slots (set_slots)
    uint32_t* stile;        // SETS: [2][BM / 32][BN] set words, halves as ftile's
    const uint32_t* sbits;  // SETS: the index's bitmaps, swords words each
    int64_t swords;
    int k, qcap_, round = 0;
    // this lane's queries: column (lane & 31) of each of its TN column tiles
    int myq[Cfg::TN];
    u64 mythr[Cfg::TN];
    int ex_lo[Cfg::TN], ex_hi[Cfg::TN];

    // Carves the LDS at `lds`, empties the lists (one barrier) and reads this lane's exclusion segments.  `rounds`: the
    // tiles this block walks (the resident pass's queue capacity depends on it).  FACET: also loads the masks.
    __device__ __forceinline__ TopK(char* lds, int k_, int Q, int q0, const int32_t* excl_off, int rounds = 1,
                                    const FacetArgs& fa = facet_args(), const SetArgs& sa = set_args())
        : frows(fa.rows), sbits(sa.bits), swords(sa.words), k(k_), qcap_(qcap(k_, rounds)) {
        const int tid = threadIdx.x, lane = tid & 63, wn = (tid >> 6) % Cfg::WAVES_N;
        thr = reinterpret_cast<u64*>(lds);
        cnt = reinterpret_cast<int*>(thr + Cfg::BN);
        flags = cnt + Cfg::BN;
        amask = reinterpret_cast<uint32_t*>(flags + 4);
        ftile = reinterpret_cast<uint16_t*>(amask + (FACET ? Cfg::BN * FACET_LDS_WORDS : 0));
        sslot = reinterpret_cast<int4*>(ftile + (FACET ? 2 * Cfg::BM : 0));
        stile = reinterpret_cast<uint32_t*>(sslot + (SETS ? Cfg::BN : 0));
        list = reinterpret_cast<u64*>(stile + (SETS ? 2 * SET_TILE_WORDS : 0));
        queue = list + (size_t)Cfg::BN * k;
        for (int i = tid; i < Cfg::BN; i += Cfg::THREADS) { thr[i] = (q0 + i < Q) ? 0ull : ~0ull; cnt[i] = 0; }
        for (int i = tid; i < Cfg::BN * k; i += Cfg::THREADS) list[i] = 0ull;
        if (tid < 4) flags[tid] = 0;
        if (FACET) facet_load_masks(amask, fa, q0, Cfg::BN, Q, tid, Cfg::THREADS);
        if (SETS)
            for (int i = tid; i < Cfg::BN; i += Cfg::THREADS) sslot[i] = set_slots(sa, q0 + i, Q);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j) {
            myq[j] = (wn * Cfg::TN + j) * 32 + (lane & 31);
            const int gq = q0 + myq[j];
            mythr[j] = gq < Q ? 0ull : ~0ull;  // padding columns never produce candidates
            ex_lo[j] = ex_hi[j] = 0;
            if (excl_off != nullptr && gq < Q) { ex_lo[j] = excl_off[gq]; ex_hi[j] = excl_off[gq + 1]; }
        }
    }

    // One tile of scores: rows row0 + (wm * TM + i) * 32 + acc_row(e, lane) of the catalog (rows >= N are padding).
    // A score is OFFERED (pushed to its query's LDS queue) when it beats the query's threshold.
    //  * warm query (list full): threshold = current k-th best key.  Queues are merged into the
    //    sorted lists only when one is at least half full (or at the block's last tile), so a
    //    stale — lower — threshold only means a few extra offers, never a missed hit.
    //  * cold query (list not full yet, threshold key 0): instead of offering all of the tile's
    //    scores, each lane first offers only its own m largest (m = ceil(k / lanes per query) + 1,
    //    so the lanes together offer >= k), the queues are merged at once, and a second pass
    //    offers whatever else still beats the now-real threshold (usually nothing).
    // FACET: a warm lane tests a candidate's row against its query's mask where it tests the exclusions.  A lane with
    // a cold query first works out which of its (row, query) pairs the masks admit (admitted()) and counts only those
    // towards its m largest and its offers: under a mask that admits a handful of rows per tile a block stays cold
    // for its whole chunk, and would otherwise push every score of every tile through the per-candidate test.
    // Both read the tile's facet words from LDS: offer() of one tile fetches the next tile's words (the block walks
    // consecutive tiles) and stores them before its first barrier, so no candidate waits for a global load; the
    // kernel puts the first tile's there with stage_first_tile().
    // SETS: the tile's set words travel the same way (the next tile's are fetched and ANDed by the threads that stage
    // them); admitted() and the warm lane's test read one word and shift.
    __device__ __forceinline__ void offer(const f32x16 (&acc)[Cfg::TM][Cfg::TN], int64_t row0, int64_t N, uint32_t row_base,
                                          const int32_t* excl_idx, bool last_tile) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int wm = wave / Cfg::WAVES_N;
        const int QCAP = qcap_;
        constexpr int LPQ = 2 * Cfg::WAVES_M;  // lanes holding scores of one query
        const int m_local = (k + LPQ - 1) / LPQ + 1;
        unsigned long long offered = 0ull;
        bool lane_cold = false;
        unsigned long long adm = ~0ull;  // FACET: pend-numbered bits of the admitted (row, query) pairs, once known
        bool adm_known = false;
        const uint16_t* const fw_tile = ftile + fcur * Cfg::BM;
        unsigned next_words = 0u;  // two rows of the next tile per thread (inside the padded array: the tile exists)
        bool next_staged = !FACET || last_tile;
        if (FACET && !last_tile && tid < Cfg::BM / 2 && (!SETS || frows != nullptr))
            next_words = *reinterpret_cast<const unsigned*>(frows + row0 + Cfg::BM + 2 * tid);
        uint32_t next_sw[SETS ? SET_NSW : 1];
        if (SETS && !last_tile) load_set_words(next_sw, row0 + Cfg::BM);
        const uint32_t* const sw_tile = stile + fcur * SET_TILE_WORDS;
        for (int pass = 0; pass < 2; ++pass) {
            if (FACET && pass == 0) {
                bool cold = false;
#pragma unroll
                for (int j = 0; j < Cfg::TN; ++j) cold |= mythr[j] == 0ull;
                if (cold) { adm = admitted(fw_tile, sw_tile, wm, lane); adm_known = true; }
            }
            // pend bit (j*TM+i)*16+e: score e of accumulator tile (i,j) has to be offered
            unsigned long long pend = 0ull;
#pragma unroll
            for (int j = 0; j < Cfg::TN; ++j) {
                float thr_s;
                if (mythr[j] == ~0ull) {
                    thr_s = INFINITY;  // padding column
                } else if (mythr[j] == 0ull && pass == 0) {
                    lane_cold = true;
                    float t = INFINITY;  // t <- m-th largest distinct valid score of this lane
                    for (int it = 0; it < m_local; ++it) {
                        float best = -INFINITY;
#pragma unroll
                        for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
                            for (int e = 0; e < 16; ++e) {
                                const bool valid = row0 + (wm * Cfg::TM + i) * 32 + acc_row(e, lane) < N &&
                                                   (!FACET || (adm >> ((j * Cfg::TM + i) * 16 + e) & 1ull) != 0ull);
                                const float v = acc[i][j][e] + 0.0f;
                                best = (valid && v < t && v > best) ? v : best;
                            }
                        t = best;
                    }
                    thr_s = t;
                } else {
                    thr_s = mythr[j] ? key_score(mythr[j]) : -INFINITY;
                }
#pragma unroll
                for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (acc[i][j][e] + 0.0f >= thr_s) pend |= 1ull << ((j * Cfg::TM + i) * 16 + e);
            }
            pend &= ~offered;
            if (FACET) pend &= adm;
            offered |= pend;
            if (pass == 0 && lane_cold) flags[2] = 1;
            bool more, wg_cold;
            do {
                bool lane_pending = false;
#pragma unroll
                for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
                    for (int i = 0; i < Cfg::TM; ++i) {
                        const int sh = (j * Cfg::TM + i) * 16;
                        unsigned m16 = (unsigned)(pend >> sh) & 0xFFFFu;
                        while (m16) {
                            const int e = __builtin_ctz(m16);
                            m16 &= m16 - 1;
                            float sc = acc[i][j][0];
#pragma unroll
                            for (int t = 1; t < 16; ++t) sc = e == t ? acc[i][j][t] : sc;
                            sc = sc + 0.0f;  // -0 -> +0
                            const int64_t row = row0 + (wm * Cfg::TM + i) * 32 + acc_row(e, lane);
                            bool take = row < N;
                            u64 key = 0ull;
                            if (take) {
                                key = make_key(sc, row_base + (uint32_t)row);
                                take = key > mythr[j];
                            }
                            if (FACET && take && !adm_known) take = facet_admits(amask, myq[j], fw_tile[row - row0]);
                            if (SETS && take && !adm_known)
                                take = (sw_tile[(int)((row - row0) >> 5) * Cfg::BN + myq[j]] >> ((row - row0) & 31) & 1u) != 0u;
                            if (take && ex_hi[j] > ex_lo[j]) take = !excluded(excl_idx, ex_lo[j], ex_hi[j], (int)row);
                            bool settled = true;
                            if (take) {
                                const int slot = atomicAdd(&cnt[myq[j]], 1);
                                if (slot < QCAP) queue[myq[j] * QCAP + slot] = key;
                                else { settled = false; lane_pending = true; }
                            }
                            if (settled) pend &= ~(1ull << (sh + e));
                        }
                    }
                if (lane_pending) flags[round & 1] = 1;
                if (!next_staged) {  // the other half was last read in the previous tile's offer(), which ended on a barrier
                    if (tid < Cfg::BM / 2) reinterpret_cast<unsigned*>(ftile + (fcur ^ 1) * Cfg::BM)[tid] = next_words;
                    if (SETS) store_set_words(next_sw, fcur ^ 1);
                    next_staged = true;
                }
                __syncthreads();
                more = flags[round & 1] != 0;
                wg_cold = flags[2] != 0;
                if (tid == 0) flags[(round + 1) & 1] = 0;
                const bool force = wg_cold || last_tile;
                // each wave merges the queues of its share of the queries (query wave + NW * t is polled by lane t:
                // one LDS read for all of them instead of one dependent read per query)
                constexpr int NW = Cfg::THREADS / 64, QPW = Cfg::BN / NW;
                static_assert(QPW <= 64, "one polling lane per query");
                int myc = lane < QPW ? cnt[wave + NW * lane] : 0;
                myc = myc < QCAP ? myc : QCAP;
                // merge a queue once it holds 8 candidates (a quarter of the 32-entry queues: the room above absorbs a burst
                // without a second offer / merge iteration, the early merge keeps the thresholds fresh)
                const int trig = QCAP >= 32 ? 8 : QCAP / 2;
                unsigned long long need = __ballot(myc > 0 && (force || myc >= trig));
                if (QCAP <= 32 && k <= 32) {
                    while (need) {  // two queries per merge call
                        const int ta = __builtin_ctzll(need);
                        need &= need - 1;
                        const int tb = need ? __builtin_ctzll(need) : -1;
                        if (tb >= 0) need &= need - 1;
                        const int na = __builtin_amdgcn_readlane(myc, ta);
                        const int nb = tb >= 0 ? __builtin_amdgcn_readlane(myc, tb) : 0;
                        merge_queue2(list, queue, QCAP, wave + NW * ta, na, wave + NW * (tb >= 0 ? tb : ta), nb, k, lane, thr,
                                     cnt);
                    }
                } else {
                    while (need) {
                        const int t = __builtin_ctzll(need);
                        need &= need - 1;
                        const int q = wave + NW * t;
                        merge_queue(list + (size_t)q * k, queue + q * QCAP, __builtin_amdgcn_readlane(myc, t), k, lane);
                        if (lane == 0) { thr[q] = list[(size_t)q * k + k - 1]; cnt[q] = 0; }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < Cfg::TN; ++j) mythr[j] = thr[myq[j]];
                ++round;
            } while (more);
            if (!wg_cold) break;  // warm block: one pass (uniform: read between the barriers)
        }
        __syncthreads();
        if (tid == 0) flags[2] = 0;
        if (FACET) fcur ^= 1;
    }

    // FACET: the facet words of the block's first tile -> LDS (one barrier); the block has at least that tile.
    // SETS: and its set words (the slots were published by the constructor's barrier); without facets the words are 0.
    __device__ __forceinline__ void stage_first_tile(int64_t row0) {
        if (threadIdx.x < Cfg::BM / 2)
            reinterpret_cast<unsigned*>(ftile)[threadIdx.x] =
                SETS && frows == nullptr ? 0u : *reinterpret_cast<const unsigned*>(frows + row0 + 2 * threadIdx.x);
        if (SETS) {
            uint32_t sw[SETS ? SET_NSW : 1];
            load_set_words(sw, row0);
            store_set_words(sw, 0);
        }
        __syncthreads();
    }

    // SETS: this thread's SET_NSW words of the tile at row0 (inside the padded bitmaps: the tile exists) - word
    // i = tid + THREADS * u is query i % BN, rows row0 + 32 (i / BN) .. + 31 - and their place in half `half` of stile.
    __device__ __forceinline__ void load_set_words(uint32_t (&sw)[SETS ? SET_NSW : 1], int64_t row0) const {
        const int4 slots = sslot[threadIdx.x % Cfg::BN];
#pragma unroll
        for (int u = 0; u < SET_NSW; ++u)
            sw[u] = set_word(sbits, swords, slots, (row0 >> 5) + (threadIdx.x + Cfg::THREADS * u) / Cfg::BN);
    }
    __device__ __forceinline__ void store_set_words(const uint32_t (&sw)[SETS ? SET_NSW : 1], int half) {
#pragma unroll
        for (int u = 0; u < SET_NSW; ++u) stile[half * SET_TILE_WORDS + threadIdx.x + Cfg::THREADS * u] = sw[u];
    }

    // FACET: bit (j * TM + i) * 16 + e (pend's numbering) is set iff the mask of this lane's query j admits the row of
    // accumulator element e of row tile i.  Elements 4g .. 4g + 3 are four consecutive rows (acc_row) whose facet
    // words (fw_tile: the tile's, in LDS) are one aligned 8-byte read; rows past N hold the array's zero padding and
    // are dropped by the row test.  SETS: and the query's set word of row tile i has the row's bit.
    __device__ __forceinline__ unsigned long long admitted(const uint16_t* fw_tile, const uint32_t* sw_tile, int wm,
                                                           int lane) const {
        unsigned long long bits = 0ull;
#pragma unroll
        for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint2 w = *reinterpret_cast<const uint2*>(fw_tile + (wm * Cfg::TM + i) * 32 + acc_row(4 * g, lane));
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const unsigned fw = ((t & 2 ? w.y : w.x) >> (16 * (t & 1))) & 0xFFFFu;
#pragma unroll
                    for (int j = 0; j < Cfg::TN; ++j)
                        if (facet_admits(amask, myq[j], fw) &&
                            (!SETS || (sw_tile[(wm * Cfg::TM + i) * Cfg::BN + myq[j]] >> acc_row(4 * g + t, lane) & 1u) != 0u))
                            bits |= 1ull << ((j * Cfg::TM + i) * 16 + 4 * g + t);
                }
            }
        return bits;
    }

    // the sorted lists out: partial[chunk][q0 + q][0..k) for the block's BN queries
    __device__ __forceinline__ void write(u64* partial, int chunk, int Qpad, int q0) const {
        for (int i = threadIdx.x; i < Cfg::BN * k; i += Cfg::THREADS) {
            const int q = i / k, e = i % k;
            partial[((size_t)chunk * Qpad + q0 + q) * k + e] = list[(size_t)q * k + e];
        }
    }
};

// Grid of every tiled search kernel: n_chunks * n_qtiles blocks (XCD-remapped).  Block (chunk, qtile) scores catalog
// row tiles [chunk*tiles_per_chunk, ...) against query tile qtile and keeps, per query, the k best (score, row) seen,
// then writes them (sorted, as keys) to partial[chunk][query][0..k).  Consecutive logical ids share a catalog chunk
// (and hence an XCD's L2).
//
// The exact pass: rows in fp32, or (P16) stored as bfloat16 (ICREC_ROWS_BF16) and widened on their way into LDS.
// EMIT = true additionally stores every score to scores_out[q*N + row] (parity checks only).
// run_flag != NULL: the whole grid exits unless *run_flag != 0 (the exact pass behind a filter pass).
// Facet = FacetArgs: the FACET arm; Facet = SetArgs: the SETS arm (no EMIT forms).
template <class Cfg, bool EMIT, bool P16, class... Facet>
__global__ __launch_bounds__(Cfg::THREADS, 2) void search_kernel(
    const void* __restrict__ P, int64_t N, int K, const float* __restrict__ Qn, int Qpad, int Q, int k,
    const int32_t* __restrict__ excl_idx, const int32_t* __restrict__ excl_off, uint32_t row_base, int n_row_tiles,
    int tiles_per_chunk, int n_qtiles, u64* __restrict__ partial, float* __restrict__ scores_out,
    const int* __restrict__ run_flag, Facet... facet) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    if (run_flag != nullptr && *run_flag == 0) return;  // uniform over the grid
    float* As = reinterpret_cast<float*>(smem_raw);
    float* Bs = As + Cfg::BM * LDK;
    const int lane = threadIdx.x & 63, wm = (threadIdx.x >> 6) / Cfg::WAVES_N;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int chunk = bid / n_qtiles, q0 = bid % n_qtiles * Cfg::BN;
    TopK<Cfg, false, sizeof...(Facet) != 0, has_sets<Facet...>> sel(smem_raw + (size_t)Cfg::LDS_FLOATS * 4, k, Q, q0, excl_off, 1,
                                                                    facet_args(facet...), set_args(facet...));
    const int t_begin = chunk * tiles_per_chunk;
    const int t_end = min(n_row_tiles, t_begin + tiles_per_chunk);
    if (sizeof...(Facet) != 0 && t_begin < t_end) sel.stage_first_tile((int64_t)t_begin * Cfg::BM);
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t row0 = (int64_t)tile * Cfg::BM;
        f32x16 acc[Cfg::TM][Cfg::TN];
        tile_gemm<Cfg, P16>(acc, P, row0, N, Qn, q0, Qpad, K, As, Bs);
        if (EMIT) {
#pragma unroll
            for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
                for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int64_t row = row0 + (wm * Cfg::TM + i) * 32 + acc_row(e, lane);
                        const int gq = q0 + sel.myq[j];
                        if (row < N && gq < Q) scores_out[(int64_t)gq * N + row] = acc[i][j][e] + 0.0f;
                    }
        }
        sel.offer(acc, row0, N, row_base, excl_idx, tile == t_end - 1);
    }
    sel.write(partial, chunk, Qpad, q0);
}

// The STAGED filter pass of ICREC_ROWS_F32_FILTER: rows and queries as f16 hi/lo planes (Ph/Pl, Qh/Ql), both staged
// through LDS per tile, scores from three f16 MFMAs per product (gemm_x3.h): within ~1e-7 of the exact chain at 5x its
// MFMA rate, NOT bit-exact; its lists only nominate candidates for verify_kernel.
template <class Cfg, class... Facet>
__global__ __launch_bounds__(Cfg::THREADS, 2) void staged_search_kernel(
    const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl, int64_t N, int K, const _Float16* __restrict__ Qh,
    const _Float16* __restrict__ Ql, int Qpad, int Q, int k, const int32_t* __restrict__ excl_idx,
    const int32_t* __restrict__ excl_off, uint32_t row_base, int n_row_tiles, int tiles_per_chunk, int n_qtiles,
    u64* __restrict__ partial, Facet... facet) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int chunk = bid / n_qtiles, q0 = bid % n_qtiles * Cfg::BN;
    TopK<Cfg, false, sizeof...(Facet) != 0, has_sets<Facet...>> sel(smem_raw + SmemH<Cfg>::BYTES, k, Q, q0, excl_off, 1,
                                                                    facet_args(facet...), set_args(facet...));
    const int t_begin = chunk * tiles_per_chunk;
    const int t_end = min(n_row_tiles, t_begin + tiles_per_chunk);
    if (sizeof...(Facet) != 0 && t_begin < t_end) sel.stage_first_tile((int64_t)t_begin * Cfg::BM);
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t row0 = (int64_t)tile * Cfg::BM;
        f32x16 a0[Cfg::TM][Cfg::TN], a1[Cfg::TM][Cfg::TN], acc[Cfg::TM][Cfg::TN];
        tile_gemm_h<Cfg>(a0, a1, Ph, Pl, row0, N, Qh, Ql, q0, Qpad, K, reinterpret_cast<_Float16*>(smem_raw));
#pragma unroll
        for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
            for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = fmaf(a1[i][j][e], LO_UNSCALE, a0[i][j][e]);
        sel.offer(acc, row0, N, row_base, excl_idx, tile == t_end - 1);
    }
    sel.write(partial, chunk, Qpad, q0);
}

// ---- the RESIDENT filter pass's operands.  This pass keeps the v_mfma_f32_32x32x16_f16 form of the weights-direct
// engine (its selection code is written for the 32x32 accumulator map; the pass is ~3 % of a recommend step): catalog
// rows packed as [32-row tile][16-deep k-step][plane] fragments of 1 KB (storage.h: frag_slot has the layout, and
// r32_frag_off / r32_w_load walk it by the same 2 * WT_FRAG stride, lane * 8 inside a plane).
// (The encoder's linear layers use the 16x16x32 form, wt_gemm.h.)  The query tile's two
// activation planes, [64 queries][384] halfs each, live in LDS for the whole block in the layout of the encoder's
// fused kernels (768-B rows as three XOR-swizzled 256-B sub-rows).
constexpr int RES_XPLANE = 64 * 768;
constexpr int RES_X_BYTES = 2 * RES_XPLANE;

__device__ __forceinline__ size_t r32_frag_off(int nt, int ks, int KS) { return ((size_t)nt * KS + ks) * (2 * WT_FRAG); }
__device__ __forceinline__ void r32_w_load(half8& wh, half8& wl, const _Float16* wp, int ks, unsigned lo8) {
    const _Float16* p = wp + (size_t)ks * (2 * WT_FRAG);
    wh = *reinterpret_cast<const half8*>(p + lo8);
    wl = *reinterpret_cast<const half8*>(p + WT_FRAG + lo8);
}
__device__ __forceinline__ void r32_mma(f32x16 (&acc)[1][2], const half8& wh, const half8& wl, const half8 (&xh)[2],
                                        const half8 (&xl)[2]) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        acc[0][tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh[tt], acc[0][tt], 0, 0, 0);
        acc[0][tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh[tt], acc[0][tt], 0, 0, 0);
        acc[0][tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl[tt], acc[0][tt], 0, 0, 0);
    }
}

// The block's 64 queries q0 .. q0 + 63 (Qpad is a multiple of 64: every row exists), both planes -> LDS at Xs.
// 512 threads.
__device__ __forceinline__ void r32_load_queries(char* Xs, const _Float16* qh, const _Float16* ql, int q0, int tid) {
    u32x4 vh[6], vl[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int id = tid + 512 * i, row = id / 48, c = id - row * 48;
        const int64_t g = (int64_t)(q0 + row) * 384 + c * 8;
        vh[i] = *reinterpret_cast<const u32x4*>(qh + g);
        vl[i] = *reinterpret_cast<const u32x4*>(ql + g);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int id = tid + 512 * i, row = id / 48, c = id - row * 48;
        const int pos = row * 768 + (((c & ~15) | ((c ^ row) & 15)) << 4);
        *reinterpret_cast<u32x4*>(Xs + pos) = vh[i];
        *reinterpret_cast<u32x4*>(Xs + RES_XPLANE + pos) = vl[i];
    }
}

// One 32-row fragment tile (wp) against the block's two 32-query tiles: out[tt] = its scores.  The 8-deep weight ring
// (rwh, rwl) holds k-steps 0-7 of wp on entry and k-steps 0-7 of wpn, the wave's next tile, on return.
__device__ __forceinline__ void r32_tile(f32x16 (&out)[2], const char* Xs, const int (&xb0)[2], half8 (&rwh)[8],
                                         half8 (&rwl)[8], const _Float16* wp, const _Float16* wpn, unsigned lo8) {
    f32x16 S[1][2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int e = 0; e < 16; ++e) S[0][tt][e] = 0.0f;
    half8 fh[2][2], fl[2][2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        fh[0][tt] = *reinterpret_cast<const half8*>(Xs + xb0[tt]);
        fl[0][tt] = *reinterpret_cast<const half8*>(Xs + RES_XPLANE + xb0[tt]);
    }
#pragma unroll
    for (int ks = 0; ks < RES_KS; ++ks) {
        if (ks + 1 < RES_KS) {
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const int pos = (xb0[tt] ^ (((ks + 1) & 7) << 5)) + ((ks + 1) >> 3) * 256;
                fh[(ks + 1) & 1][tt] = *reinterpret_cast<const half8*>(Xs + pos);
                fl[(ks + 1) & 1][tt] = *reinterpret_cast<const half8*>(Xs + RES_XPLANE + pos);
            }
        }
        r32_mma(S, rwh[ks & 7], rwl[ks & 7], fh[ks & 1], fl[ks & 1]);
        if (ks + 8 < RES_KS) r32_w_load(rwh[ks & 7], rwl[ks & 7], wp, ks + 8, lo8);
        else r32_w_load(rwh[ks & 7], rwl[ks & 7], wpn, ks + 8 - RES_KS, lo8);
        __builtin_amdgcn_sched_barrier(0);  // pin the prefetch to its k-step
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) out[j][e] = S[0][j][e] * WT_UNSCALE;
}

// The RESIDENT form of the filter pass (dim = 384): the rows as packed weight fragments (pack_rows_kernel: the 1 KB one
// wave feeds to one MFMA is contiguous), Qh/Ql = the queries' activation planes.  The block's 64 queries are loaded into
// LDS ONCE and stay there for all its row tiles; every wave owns one 32-row tile of each 256-row round and streams its
// fragments L2 -> registers through an 8-deep ring that runs across rounds (the next round's first fragments land
// under the selection): no operand staging barriers at all - the staged pass re-stages both operands through LDS for
// every 128-row tile (two barriers per 64-deep slab).
template <class Cfg, class... Facet>
__global__ __launch_bounds__(Cfg::THREADS, 2) void resident_search_kernel(
    const _Float16* __restrict__ frag, int64_t N, const _Float16* __restrict__ Qh, const _Float16* __restrict__ Ql,
    int Qpad, int Q, int k, const int32_t* __restrict__ excl_idx, const int32_t* __restrict__ excl_off,
    uint32_t row_base, int n_row_tiles, int tiles_per_chunk, int n_qtiles, u64* __restrict__ partial, Facet... facet) {
    static_assert(Cfg::TM == 1 && Cfg::TN == 2 && Cfg::WAVES_N == 1 && Cfg::WAVES_M == 8,
                  "resident pass: 8 waves x (1 row tile x 2 query tiles)");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int chunk = bid / n_qtiles, q0 = bid % n_qtiles * Cfg::BN;
    TopK<Cfg, true, sizeof...(Facet) != 0, has_sets<Facet...>> sel(smem_raw + RES_X_BYTES, k, Q, q0, excl_off, tiles_per_chunk,
                                                                   facet_args(facet...), set_args(facet...));
    const int t_begin = chunk * tiles_per_chunk;
    const int t_end = min(n_row_tiles, t_begin + tiles_per_chunk);
    if (sizeof...(Facet) != 0 && t_begin < t_end) sel.stage_first_tile((int64_t)t_begin * Cfg::BM);

    // query planes -> LDS (once), weight ring of the first round
    r32_load_queries(smem_raw, Qh, Ql, q0, tid);
    int xb0[2];  // this lane's fragment of query tile tt at k-step ks: xb0[tt] ^ ((ks & 7) << 5), + 256 (ks >> 3)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int tok = tt * 32 + (lane & 31);
        xb0[tt] = tok * 768 + (((lane >> 5) ^ (tok & 15)) << 4);
    }
    const unsigned lo8 = lane * 8;
    half8 rwh[8], rwl[8];
    if (t_begin < t_end) {
        const _Float16* const wp0 = frag + r32_frag_off((t_begin * 8 + wave) * Cfg::TM, 0, RES_KS);
#pragma unroll
        for (int d = 0; d < 8; ++d) r32_w_load(rwh[d], rwl[d], wp0, d, lo8);
    }
    __syncthreads();  // queries resident

    f32x16 acc[Cfg::TM][Cfg::TN];
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t row0 = (int64_t)tile * Cfg::BM;
        // the wave's TM fragment tiles (tile * 8 + wave) * TM + i of this round, one after the other; the selection then
        // runs once per round over all of them
#pragma unroll
        for (int i = 0; i < Cfg::TM; ++i) {
            const int rt = (tile * 8 + wave) * Cfg::TM + i;
            // the ring continues into the wave's next tile; past the block's last round: re-read (never consumed)
            const int rn = i + 1 < Cfg::TM ? rt + 1 : (tile + 1 < t_end ? ((tile + 1) * 8 + wave) * Cfg::TM : rt);
            r32_tile(acc[i], smem_raw, xb0, rwh, rwl, frag + r32_frag_off(rt, 0, RES_KS), frag + r32_frag_off(rn, 0, RES_KS), lo8);
        }
        sel.offer(acc, row0, N, row_base, excl_idx, tile == t_end - 1);
    }
    sel.write(partial, chunk, Qpad, q0);
}

// ---------------------------------------------------------------- small-batch streaming search
// For Q <= 8 queries the MFMA kernel above spends 4-32x its useful work on padding columns (its
// narrowest tile is 32 queries wide) and becomes MFMA-bound long before HBM.  This kernel is the
// HBM-bound form (SURVEY §8d "K8a"): one thread per catalog row.  A block streams tiles of 256 rows
// through LDS in 128-byte slabs (coalesced 16-B global loads, next slab in flight under the current
// one's FMAs); each thread walks ITS row of the slab out of LDS and runs one fp32 fmaf chain per
// query, k ascending from 0 — the very chain the f32 MFMA computes, so scores stay bit-identical to
// the oracle.  Query values are block-uniform (scalar loads).  Selection: the block's first tile ranks
// its 256 keys per query by counting (no merges); later tiles offer only keys above the running k-th
// best into a 256-slot LDS queue that merge_queue folds into the sorted list.  (Tile geometry: stream.h.)
template <int NQ>
struct StreamSmem {
    static __host__ __device__ size_t bytes(int k, bool facet = false, bool sets = false) {
        return (size_t)ST_ROWS * ST_LDB + 64 /*thr*/ + 64 /*cnt*/ + (size_t)((NQ * k + 1) & ~1) * 8 + (size_t)NQ * ST_ROWS * 8 +
               (facet ? NQ * FACET_LDS_WORDS * 4 : 0) /*allow masks*/ + (sets ? NQ * (ST_ROWS / 32) * 4 : 0) /*set words of a tile*/;
    }
};

typedef float v2f __attribute__((ext_vector_type(2)));
// acc[j] = fmaf(q[j], p, acc[j]) for the NQ queries of one k; pairs of queries share one packed FMA
// (v_pk_fma_f32: two independent IEEE fmas, so each chain is unchanged).
template <int NQ>
__device__ __forceinline__ void stream_fma(float (&acc)[NQ], const float* __restrict__ q, float p) {
    if (NQ == 1) {
        acc[0] = fmaf(q[0], p, acc[0]);
    } else {
#pragma unroll
        for (int j = 0; j < NQ; j += 2) {
            const v2f a = {acc[j], acc[j + 1]}, qq = {q[j], q[j + 1]}, pp = {p, p};
            const v2f r = __builtin_elementwise_fma(qq, pp, a);
            acc[j] = r.x;
            acc[j + 1] = r.y;
        }
    }
}

// 128-B slab `slab` of the 256 rows of tile `tile` -> 8 x 16 B per thread (rows clamped to the last valid row)
__device__ __forceinline__ void stream_load_slab(v4f (&pre)[8], const char* __restrict__ Pb, int64_t N, int row_bytes,
                                                 int tile, int slab, int tid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + ST_ROWS * i;
        int64_t row = (int64_t)tile * ST_ROWS + (id >> 3);
        row = row < N ? row : N - 1;
        pre[i] = *reinterpret_cast<const v4f*>(Pb + row * row_bytes + slab * 128 + (id & 7) * 16);
    }
}

template <int NQ, bool P16, class... Facet>  // Facet = FacetArgs: the FACET arm, SetArgs: the SETS arm
__global__ __launch_bounds__(ST_ROWS, 2) void stream_search_kernel(
    const void* __restrict__ P, int64_t N, int K, const float* __restrict__ Qn /* [K][NQ], zero-padded columns */, int Q,
    int k, const int32_t* __restrict__ excl_idx, const int32_t* __restrict__ excl_off, uint32_t row_base, int n_row_tiles,
    int tiles_per_chunk, u64* __restrict__ partial, Facet... facet) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr bool FACET = sizeof...(Facet) != 0, SETS = has_sets<Facet...>;
    const FacetArgs fa = facet_args(facet...);
    const SetArgs sa = set_args(facet...);
    char* rows_s = smem_raw;
    u64* thr = reinterpret_cast<u64*>(smem_raw + ST_ROWS * ST_LDB);
    int* cnt = reinterpret_cast<int*>(thr + 8);
    u64* list = reinterpret_cast<u64*>(cnt + 16);
    u64* queue = list + (size_t)((NQ * k + 1) & ~1);  // 16-B aligned: the cold path reads it two keys at a time
    uint32_t* amask = reinterpret_cast<uint32_t*>(queue + NQ * ST_ROWS);  // FACET: [NQ][FACET_LDS_WORDS]
    // SETS: [NQ][8], word (j, w) = the intersection of query j's sets over rows 32 w .. 32 w + 31 of the tile
    uint32_t* swords = amask + NQ * FACET_LDS_WORDS;
    constexpr int SW = ST_ROWS / 32;

    constexpr int EPW = P16 ? 2 : 1;             // elements per 32-bit word
    constexpr int SLAB_ELEMS = 32 * EPW;         // 128 B of one row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = xcd_remap(blockIdx.x, gridDim.x);
    const int row_bytes = K * (P16 ? 2 : 4);
    const int nslab = K / SLAB_ELEMS;
    const char* Pb = static_cast<const char*>(P);

    if (tid < NQ) { thr[tid] = tid < Q ? 0ull : ~0ull; cnt[tid] = 0; }
    for (int i = tid; i < NQ * k; i += ST_ROWS) list[i] = 0ull;
    if (FACET) facet_load_masks(amask, fa, 0, NQ, Q, tid, ST_ROWS);
    int4 slots = make_int4(SET_NONE, SET_NONE, SET_NONE, SET_NONE);  // SETS: thread j * 8 + w stages word (j, w)
    if (SETS && tid < NQ * SW) slots = set_slots(sa, tid / SW, Q);

    u64 mythr[NQ];
    int ex_lo[NQ], ex_hi[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        mythr[j] = j < Q ? 0ull : ~0ull;
        ex_lo[j] = ex_hi[j] = 0;
        if (excl_off != nullptr && j < Q) { ex_lo[j] = excl_off[j]; ex_hi[j] = excl_off[j + 1]; }
    }

    const int t_begin = chunk * tiles_per_chunk;
    const int t_end = min(n_row_tiles, t_begin + tiles_per_chunk);
    v4f pre[8];  // native vectors: HIP's float4 struct copies become memcpys that pin the array in scratch
    stream_load_slab(pre, Pb, N, row_bytes, min(t_begin, n_row_tiles - 1), 0, tid);

    for (int tile = t_begin; tile < t_end; ++tile) {
        // FACET: this thread's row's facet word, in flight under the FMAs (inside the padded array also past N)
        const unsigned fw = FACET && (!SETS || fa.rows != nullptr) ? fa.rows[(int64_t)tile * ST_ROWS + tid] : 0u;
        // SETS: the tile's set words (inside the padded bitmaps); the previous tile's were last read before its
        // selection's barriers, the slab loop's first barrier publishes these
        if (SETS && tid < NQ * SW) swords[tid] = set_word(sa.bits, sa.words, slots, (int64_t)tile * SW + tid % SW);
        float acc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[j] = 0.0f;
        for (int s = 0; s < nslab; ++s) {
            __syncthreads();  // the previous slab has been consumed (also covers the list/thr initialisation)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int id = tid + ST_ROWS * i;
                *reinterpret_cast<v4f*>(rows_s + (id >> 3) * ST_LDB + (id & 7) * 16) = pre[i];
            }
            __syncthreads();
            {   // next slab (of this tile or the first of the next one) goes in flight under this slab's FMAs;
                // unconditional — the block's very last iteration re-loads its own slab — so `pre` stays in registers
                const bool wrap = s + 1 == nslab;
                const int nt = wrap ? min(tile + 1, t_end - 1) : tile, ns = wrap ? 0 : s + 1;
                stream_load_slab(pre, Pb, N, row_bytes, nt, ns, tid);
            }
            const char* my = rows_s + tid * ST_LDB;
            const float* qs = Qn + (size_t)s * SLAB_ELEMS * NQ;  // k-major: the NQ values of one k are adjacent
            // NQ (x2 for bf16 rows) x 8 scalar query values per 16-B piece: unroll only as far as SGPRs allow
#pragma unroll(NQ >= 8 ? 1 : NQ >= 4 ? 2 : 8)
            for (int c = 0; c < 8; ++c) {
                const v4f w = *reinterpret_cast<const v4f*>(my + c * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (P16) {
                        const unsigned u = __float_as_uint(w[e]);
                        const int kk = c * 8 + e * 2;
                        stream_fma<NQ>(acc, qs + kk * NQ, bf16_lo(u));
                        stream_fma<NQ>(acc, qs + (kk + 1) * NQ, bf16_hi(u));
                    } else {
                        stream_fma<NQ>(acc, qs + (c * 4 + e) * NQ, w[e]);
                    }
                }
            }
        }

        // ---- selection for this tile's 256 scores per query
        const int64_t row = (int64_t)tile * ST_ROWS + tid;
        u64 key[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const u64 kx = make_key(acc[j] + 0.0f, row_base + (uint32_t)row);
            bool take = row < N && mythr[j] != ~0ull && kx > mythr[j];
            if (FACET && take) take = facet_admits(amask, j, fw);
            if (SETS && take) take = (swords[j * SW + (tid >> 5)] >> (tid & 31) & 1u) != 0u;
            if (take && ex_hi[j] > ex_lo[j]) take = !excluded(excl_idx, ex_lo[j], ex_hi[j], (int)row);
            key[j] = take ? kx : 0ull;
        }
        if (tile == t_begin) {
            // cold: rank every key among the tile's 256 by counting; rank r < k goes straight to list[r]
#pragma unroll
            for (int j = 0; j < NQ; ++j) queue[j * ST_ROWS + tid] = key[j];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                if (j < Q) {  // uniform
                    int r = 0;
                    const u64* qj = queue + j * ST_ROWS;
                    for (int i = 0; i < ST_ROWS; i += 2) {
                        const ulonglong2 two = *reinterpret_cast<const ulonglong2*>(qj + i);  // LDS broadcast
                        r += (two.x > key[j]) + (two.y > key[j]);
                    }
                    if (key[j] != 0ull && r < k) list[j * k + r] = key[j];
                }
            }
            __syncthreads();
        } else {
#pragma unroll
            for (int j = 0; j < NQ; ++j)
                if (key[j] != 0ull) queue[j * ST_ROWS + atomicAdd(&cnt[j], 1)] = key[j];  // <= 256 offers per tile
            __syncthreads();
            for (int j = wave; j < NQ; j += ST_ROWS / 64) {
                const int c = cnt[j];
                for (int off = 0; off < c; off += 64)
                    merge_queue(list + (size_t)j * k, queue + j * ST_ROWS + off, min(64, c - off), k, lane);
                if (lane == 0) cnt[j] = 0;
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j)
            if (mythr[j] != ~0ull) mythr[j] = list[(size_t)j * k + k - 1];
    }

    __syncthreads();
    for (int i = tid; i < NQ * k; i += ST_ROWS) partial[(size_t)chunk * NQ * k + i] = list[i];
}

// ---------------------------------------------------------------- filter + verify (ICREC_ROWS_F32_FILTER)
// queries -> the engine's activation planes (hi/lo of 16 x, wt_gemm.h: split_act4), row-major [Qpad][K]; clears the flag
__global__ __launch_bounds__(256) void split_queries_act_kernel(const float* __restrict__ src, size_t n4, _Float16* __restrict__ hi,
                                                                _Float16* __restrict__ lo, int* __restrict__ flag) {
    if (flag != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * i);
        half4 a, b;
        split_act4(v, a, b);
        *reinterpret_cast<half4*>(hi + 4 * i) = a;
        *reinterpret_cast<half4*>(lo + 4 * i) = b;
    }
}

// Exact re-scoring of the filter pass's candidates.  cand[q][0..kp): the kp best (approximate score, row) keys of
// query q, sorted; one wavefront per query, two candidates per lane.  Every candidate gets the exact k-ascending
// fp32 fmaf chain (the oracle's arithmetic) from the fp32 rows, candidates are ranked by (exact score desc, row asc)
// and the best k written out.  The result is THE exact top-k iff no row outside the list can reach the k-th exact
// score: outside rows have approx <= the list's last approx score, and |approx - exact| <= eps, so
//     last_approx + eps < exact_kth    (or the list is not full: it then holds every admissible row)
// proves it.  Otherwise *flag is set and the exact search that follows (it exits at once when the flag is clear)
// recomputes the batch.
template <bool P16>  // P16: rows are bfloat16 bits, widened exactly (the arithmetic of the bf16 exact search)
__global__ __launch_bounds__(256) void verify_kernel(const void* __restrict__ Pv, int K, const float* __restrict__ qn,
                                                     const u64* __restrict__ cand, int Q, int kp, int k, uint32_t row_base,
                                                     float eps, int64_t* __restrict__ out_idx, float* __restrict__ out_score,
                                                     u64* __restrict__ out_keys, int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const float* qv = qn + (size_t)q * K;
    u64 ek[2];
    int n_valid = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int c = lane + 64 * s;
        const u64 ck = c < kp ? cand[(size_t)q * kp + c] : 0ull;
        ek[s] = 0ull;
        if (ck != 0ull) {
            const uint32_t grow = key_row(ck);
            float acc = 0.0f;
            if (P16) {
                const uint16_t* pr = static_cast<const uint16_t*>(Pv) + (size_t)(grow - row_base) * K;
                for (int j = 0; j < K; j += 4) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(qv + j);
                    const uint2 w = *reinterpret_cast<const uint2*>(pr + j);
                    acc = fmaf(a[0], bf16_lo(w.x), acc);
                    acc = fmaf(a[1], bf16_hi(w.x), acc);
                    acc = fmaf(a[2], bf16_lo(w.y), acc);
                    acc = fmaf(a[3], bf16_hi(w.y), acc);
                }
            } else {
                const float* pr = static_cast<const float*>(Pv) + (size_t)(grow - row_base) * K;
                for (int j = 0; j < K; j += 4) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(qv + j);
                    const f32x4 b = *reinterpret_cast<const f32x4*>(pr + j);
                    acc = fmaf(a[0], b[0], acc);
                    acc = fmaf(a[1], b[1], acc);
                    acc = fmaf(a[2], b[2], acc);
                    acc = fmaf(a[3], b[3], acc);
                }
            }
            ek[s] = make_key(acc + 0.0f, grow);
        }
        n_valid += __popcll(__ballot(ck != 0ull));
    }
    // rank of each exact key among the candidates (keys are unique: the row is part of the key)
    int rk[2] = {0, 0};
    for (int s = 0; s < 2; ++s)
        for (int l = 0; l < 64; ++l) {
            const u64 o = shfl_u64(ek[s], l);
            rk[0] += o > ek[0];
            rk[1] += o > ek[1];
        }
    // exact k-th best score (rank k-1), if there are that many candidates
    float kth = -INFINITY;
    if (n_valid >= k) {
        float mine = -INFINITY;
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (ek[s] != 0ull && rk[s] == k - 1) mine = key_score(ek[s]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mine = fmaxf(mine, __shfl_xor(mine, m, 64));
        kth = mine;
    }
    if (n_valid == kp && lane == 0) {  // full list: rows outside it exist (or may)
        const float last_approx = key_score(cand[(size_t)q * kp + kp - 1]);
        if (!(last_approx + eps < kth)) atomicOr(flag, 1);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
        if (ek[s] != 0ull && rk[s] < k) store_key(ek[s], (size_t)q * k + rk[s], out_idx, out_score, out_keys);
    for (int e = n_valid + lane; e < k; e += 64)  // pads when the catalog (minus exclusions) is smaller than k
        store_key(0ull, (size_t)q * k + e, out_idx, out_score, out_keys);
}

// ---------------------------------------------------------------- host side
typedef TileCfg<2, 2, 2, 2> CfgBig;    // 128 rows x 128 queries
typedef TileCfg<4, 1, 2, 2> CfgMid;    // 256 rows x  64 queries
typedef TileCfg<4, 1, 2, 1> CfgSmall;  // 256 rows x  32 queries
typedef TileCfg<2, 2, 2, 1> CfgFilter;  // 128 rows x  64 queries, f16 planes (filter pass)
typedef TileCfg<8, 1, 1, 2> CfgRes;     // 256 rows x  64 queries per round, 8 waves (resident filter pass)
static_assert(FILTER_DIM_STEP == HBK, "index.hip admits the dims whose rows the staged pass walks in whole slabs");
static_assert(CfgRes::BM == RES_ROUND_ROWS && RES_XPLANE == 64 * 2 * 16 * RES_KS,
              "storage.hip sizes the fragments in the resident pass's rounds, for the k-steps its query planes hold");

// Filter + verify (ICREC_ROWS_F32_FILTER): batches of at least FILTER_MIN_Q queries are ranked by the f16x3 filter
// pass with FILTER_SLACK extra list entries, then verified exactly.  filter_eps(dim) bounds |filter score - exact score|
// for unit vectors: the f16 split drops <= 3 * 2^-22 per product (Cauchy-Schwarz: <= 7.2e-7 per score) and either
// fp32 accumulation is off by at most dim * 2^-24 from the real dot product, so the difference stays below
// 2 * dim * 2^-24 + 7.2e-7.  The margin is that bound (+1e-6 for the split term and second-order terms), never less
// than 1e-4: exactly 1e-4 up to dim 830 (at 384 the bound is 4.7e-5, 1e-4 covers it twice), 1.2e-4 at 1,024,
// 4.9e-4 at 4,096.
// Below 256 queries the pass's fixed costs (three more launches, longer lists) eat its advantage: measured at
// 49,688 rows Q=64 0.26 ms vs 0.15 ms exact, Q=256 equal, Q=1024 0.61 vs 0.82 ms; at 2M rows Q=256 2.5 vs 4.2 ms,
// Q=1024 7.5 vs 14.5 ms.
constexpr int FILTER_MIN_Q = 256, FILTER_SLACK = 12;
static inline float filter_eps(int dim) {
    const float bound = 2.0f * (float)dim * 0x1p-24f + 1.0e-6f;
    return bound > 1.0e-4f ? bound : 1.0e-4f;
}
static inline int filter_list_len(int k) { int kp = k + FILTER_SLACK; kp = (kp + 7) & ~7; return kp; }

struct Plan {
    int variant;  // 0 big, 1 mid, 2 small, 3 streaming
    int BM, BN, Qpad, n_qtiles, n_row_tiles, tiles_per_chunk, n_chunks;
    size_t smem;  // tiled variants (launch_exact sizes the streaming kernel's)
    size_t ws_q, ws_partial, ws_total;
};

// The rows as n_row_tiles tiles of BM rows, in n_chunks chunks of tiles_per_chunk whole tiles: one chunk per block (of
// each query tile) and one sorted list per chunk and query: `want` chunks, clamped to [1, cap] and to the tile count.
static void plan_chunks(int64_t n_rows, int BM, int want, int cap, int* n_row_tiles, int* tiles_per_chunk, int* n_chunks) {
    *n_row_tiles = (int)((n_rows + BM - 1) / BM);
    want = want < 1 ? 1 : want > cap ? cap : want;
    if (want > *n_row_tiles) want = *n_row_tiles;
    *tiles_per_chunk = (*n_row_tiles + want - 1) / want;
    *n_chunks = (*n_row_tiles + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

// The arm of a search's selecting kernels: ARM_FACET with allow masks, ARM_SETS with set ids (and allow masks or not).
enum Arm { ARM_PLAIN = 0, ARM_FACET = 1, ARM_SETS = 2 };
// Dynamic LDS of the tiled kernels: operand staging, then the selection (TopK; ARM_FACET: with the allow masks and the
// tiles' facet words, ARM_SETS: and the queries' slots and the tiles' set words).
template <class Cfg, bool RESIDENT = false> static size_t topk_bytes(int k, Arm arm) {
    return arm == ARM_SETS    ? TopK<Cfg, RESIDENT, true, true>::bytes(k)
           : arm == ARM_FACET ? TopK<Cfg, RESIDENT, true>::bytes(k)
                              : TopK<Cfg, RESIDENT>::bytes(k);
}
template <class Cfg> static size_t exact_smem(int k, Arm arm) { return (size_t)Cfg::LDS_FLOATS * 4 + topk_bytes<Cfg>(k, arm); }
static size_t staged_smem(int k, Arm arm) { return SmemH<CfgFilter>::BYTES + topk_bytes<CfgFilter>(k, arm); }
static size_t resident_smem(int k, Arm arm) { return RES_X_BYTES + topk_bytes<CfgRes, true>(k, arm); }
constexpr size_t LDS_MAX = 160 * 1024;

// `arm`: the plan of a faceted or set-restricted search - the same tiles and chunks (and hence the same workspace),
// more LDS.
static Plan make_plan(const Index* ix, int Q, int k, bool allow_stream, Arm arm = ARM_PLAIN) {
    Plan p;
    // The streaming kernel pays a per-block cold start (rank 256 keys per query by counting) that only amortises
    // over several tiles: take it for Q <= 2 always, for Q <= 8 once every block has >= 2 tiles (measured at
    // 49,688 rows, f32: Q=8 67 us streaming vs 44 us MFMA; at 2M rows 0.64 ms vs 0.76 ms).
    const int64_t st_tiles = (ix->n_rows + ST_ROWS - 1) / ST_ROWS;
    if (allow_stream && Q <= ix->stream_max_q && (Q <= 2 || st_tiles >= 2 * 3 * (int64_t)ix->n_cu)) {
        // variant 3: stream_search_kernel<NQ>, one block per chunk of 256-row tiles, no query tiling
        p.variant = 3; p.BM = ST_ROWS; p.BN = Q <= 1 ? 1 : Q <= 2 ? 2 : Q <= 4 ? 4 : 8;
        p.smem = 0;
        p.n_qtiles = 1;
        p.Qpad = p.BN;
        // ~3 blocks per CU are resident (LDS)
        plan_chunks(ix->n_rows, p.BM, 3 * ix->n_cu, MERGE_MAX_LISTS, &p.n_row_tiles, &p.tiles_per_chunk, &p.n_chunks);
    } else {
        if (Q > 64 && k <= 32) { p.variant = 0; p.BM = CfgBig::BM; p.BN = CfgBig::BN; p.smem = exact_smem<CfgBig>(k, arm); }
        else if (Q > 32 && k <= 64) { p.variant = 1; p.BM = CfgMid::BM; p.BN = CfgMid::BN; p.smem = exact_smem<CfgMid>(k, arm); }
        else { p.variant = 2; p.BM = CfgSmall::BM; p.BN = CfgSmall::BN; p.smem = exact_smem<CfgSmall>(k, arm); }
        p.n_qtiles = (Q + p.BN - 1) / p.BN;
        p.Qpad = p.n_qtiles * p.BN;
        // one full wave of resident blocks (2 per CU fit by LDS/VGPR), at most 256 chunks
        plan_chunks(ix->n_rows, p.BM, 2 * ix->n_cu / p.n_qtiles, 256, &p.n_row_tiles, &p.tiles_per_chunk, &p.n_chunks);
    }
    p.ws_q = align256((size_t)p.Qpad * ix->dim * 4);
    p.ws_partial = align256((size_t)p.n_chunks * p.Qpad * k * 8);
    p.ws_total = p.ws_q + p.ws_partial;
    return p;
}

// Workspace of the filter + verify path: [qn fp32 | q hi | q lo | flag | candidate keys | partial lists (filter pass,
// then reused by the guarded exact pass)].
struct FilterPlan {
    bool use, resident;
    int kp, Qpad, n_qtiles, n_row_tiles, tiles_per_chunk, n_chunks;
    size_t smem, off_qh, off_ql, off_flag, off_cand, off_partial, ws_total;
};

static FilterPlan make_filter_plan(const Index* ix, int Q, int k, const Plan& exact, Arm arm = ARM_PLAIN) {
    FilterPlan f;
    f.kp = filter_list_len(k);
    f.resident = ix->filter.frag != nullptr;
    f.use = (ix->filter.plane_hi != nullptr || f.resident) && Q >= FILTER_MIN_Q && f.kp <= ICREC_MAX_K;
    // resident form: the query planes leave 64 KB of LDS for the lists (k <= 92); longer lists take the exact search,
    // which is the faster one there anyway (measured at 49,688 rows, Q = 1,024, k = 100: staged filter 2.5 ms, exact 1.5 ms)
    // (with the allow masks of a faceted search: k <= 84; with the set words of a set-restricted one: k <= 76)
    if (f.resident && resident_smem(f.kp, arm) > LDS_MAX) f.use = false;
    if (!f.use) { f.ws_total = 0; return f; }
    f.n_qtiles = (Q + CfgFilter::BN - 1) / CfgFilter::BN;  // 64 queries per tile in both forms
    f.Qpad = f.n_qtiles * CfgFilter::BN;
    // staged form: two 4-wave blocks per CU; resident form: one 8-wave block per CU (its query planes take 96 KB)
    plan_chunks(ix->n_rows, f.resident ? CfgRes::BM : CfgFilter::BM, (f.resident ? 1 : 2) * ix->n_cu / f.n_qtiles, 256,
                &f.n_row_tiles, &f.tiles_per_chunk, &f.n_chunks);
    f.smem = f.resident ? resident_smem(f.kp, arm) : staged_smem(f.kp, arm);
    const int qpad_max = f.Qpad > exact.Qpad ? f.Qpad : exact.Qpad;
    f.off_qh = align256((size_t)qpad_max * ix->dim * 4);
    f.off_ql = f.off_qh + align256((size_t)f.Qpad * ix->dim * 2);
    f.off_flag = f.off_ql + align256((size_t)f.Qpad * ix->dim * 2);
    f.off_cand = f.off_flag + 256;
    f.off_partial = f.off_cand + align256((size_t)Q * f.kp * 8);
    const size_t part_filter = (size_t)f.n_chunks * f.Qpad * f.kp * 8;
    f.ws_total = f.off_partial + align256(part_filter > exact.ws_partial ? part_filter : exact.ws_partial);
    return f;
}

// One launch of a kernel family, timed in slot `timer`: the SETS arm `sets` (sa appended to the arguments) when the
// search has set ids, the FACET arm `facet` (sa.facet appended) when it has allow masks only, the kernel `plain`
// otherwise.  big_lds: the family's dynamic LDS can exceed the 64 KB default.
static inline Arm arm_of(const SetArgs& sa) { return sa.ids ? ARM_SETS : sa.facet.allow ? ARM_FACET : ARM_PLAIN; }
template <class Plain, class FacetArm, class SetsArm, class... Args>
static int launch_arm(Plain plain, FacetArm facet, SetsArm sets, const SetArgs& sa, bool big_lds, int timer, dim3 grid,
                      dim3 block, size_t smem, hipStream_t st, Args... args) {
    const Arm arm = arm_of(sa);
    if (big_lds)
        if (int rc = ensure_dynamic_lds(arm == ARM_SETS    ? reinterpret_cast<const void*>(sets)
                                        : arm == ARM_FACET ? reinterpret_cast<const void*>(facet)
                                                           : reinterpret_cast<const void*>(plain),
                                        160 * 1024))
            return rc;
    ScopedTimer tm(timer, st);
    if (arm == ARM_SETS) hipLaunchKernelGGL(sets, grid, block, smem, st, args..., sa);
    else if (arm == ARM_FACET) hipLaunchKernelGGL(facet, grid, block, smem, st, args..., sa.facet);
    else hipLaunchKernelGGL(plain, grid, block, smem, st, args...);
    return ICREC_OK;
}

// The exact search's kernels for one tile shape or query count and one row format: the plain kernel, its EMIT form
// (tiled kernels only), its FACET arm and its SETS arm.
using SearchFn = decltype(&search_kernel<CfgBig, false, false>);
using StreamFn = decltype(&stream_search_kernel<1, false>);
struct TiledArms {
    SearchFn plain, scores;
    decltype(&search_kernel<CfgBig, false, false, FacetArgs>) facet;
    decltype(&search_kernel<CfgBig, false, false, SetArgs>) sets;
};
struct StreamArms {
    StreamFn plain;
    decltype(&stream_search_kernel<1, false, FacetArgs>) facet;
    decltype(&stream_search_kernel<1, false, SetArgs>) sets;
};
template <class Cfg, bool P16> static TiledArms tiled_arms() {
    return {search_kernel<Cfg, false, P16>, search_kernel<Cfg, true, P16>, search_kernel<Cfg, false, P16, FacetArgs>,
            search_kernel<Cfg, false, P16, SetArgs>};
}
template <int NQ, bool P16> static StreamArms stream_arms() {
    return {stream_search_kernel<NQ, P16>, stream_search_kernel<NQ, P16, FacetArgs>, stream_search_kernel<NQ, P16, SetArgs>};
}

// The exact search of plan p over the index rows (fp32 or bf16): partial lists, or every score into scores_out.  run_flag:
// the guarded pass of the filter path, which has a timer slot of its own.  sa: the FACET or the SETS arms (arm_of; never
// with scores_out).  (Kernel tables: bf16 rows first.)
static int launch_exact(const Index* ix, const Plan& p, const float* qn, int Q, int k, const int32_t* ei,
                        const int32_t* eo, const SetArgs& sa, u64* partial, float* scores_out, const int* run_flag,
                        hipStream_t st) {
    static const TiledArms tiled[2][3] = {{tiled_arms<CfgBig, true>(), tiled_arms<CfgMid, true>(), tiled_arms<CfgSmall, true>()},
                                          {tiled_arms<CfgBig, false>(), tiled_arms<CfgMid, false>(), tiled_arms<CfgSmall, false>()}};
    static const StreamArms stream[4][2] = {{stream_arms<1, true>(), stream_arms<1, false>()},  // NQ = 1, 2, 4, 8
                                            {stream_arms<2, true>(), stream_arms<2, false>()},
                                            {stream_arms<4, true>(), stream_arms<4, false>()},
                                            {stream_arms<8, true>(), stream_arms<8, false>()}};
    const int r = rows_are_bf16(ix) ? 0 : 1;
    int rc;
    if (p.variant == 3) {
        const int nq = p.BN == 1 ? 0 : p.BN == 2 ? 1 : p.BN == 4 ? 2 : 3;
        const bool f = arm_of(sa) != ARM_PLAIN, s = arm_of(sa) == ARM_SETS;
        const size_t smem = nq == 0 ? StreamSmem<1>::bytes(k, f, s) : nq == 1 ? StreamSmem<2>::bytes(k, f, s)
                            : nq == 2 ? StreamSmem<4>::bytes(k, f, s) : StreamSmem<8>::bytes(k, f, s);
        rc = launch_arm(stream[nq][r].plain, stream[nq][r].facet, stream[nq][r].sets, sa, false, T_SEARCH_KERNEL,
                        dim3(p.n_chunks), dim3(ST_ROWS), smem, st, (const void*)ix->rows, ix->n_rows, ix->dim, qn, Q, k, ei, eo, (uint32_t)ix->row_offset,
                        p.n_row_tiles, p.tiles_per_chunk, partial);
    } else {
        const TiledArms& t = tiled[r][p.variant];
        rc = launch_arm(scores_out ? t.scores : t.plain, t.facet, t.sets, sa, true,
                        run_flag == nullptr ? T_SEARCH_KERNEL : T_SEARCH_FALLBACK, dim3(p.n_chunks * p.n_qtiles), dim3(CfgBig::THREADS), p.smem, st, (const void*)ix->rows, ix->n_rows,
                        ix->dim, qn, p.Qpad, Q, k, ei, eo, (uint32_t)ix->row_offset, p.n_row_tiles, p.tiles_per_chunk,
                        p.n_qtiles, partial, scores_out, run_flag);
    }
    if (rc) return rc;
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}
static_assert(CfgBig::THREADS == CfgMid::THREADS && CfgMid::THREADS == CfgSmall::THREADS, "launch_exact: one block size");

// Filter (f16x3 MFMA, approximate) -> merge -> verify (exact chains on the candidates) -> exact search that runs
// only if some query could not be proven.  Same outputs, bit for bit, as the exact search.  The filter pass and the
// guarded exact pass both run the arm of `sa` (arm_of) with the same masks and set ids.
static int run_search_filtered(Index* ix, const FilterPlan& f, const Plan& ex, const float* q, int Q, int k,
                               const int32_t* ei, const int32_t* eo, const SetArgs& sa, int64_t* out_idx,
                               float* out_score, u64* out_keys, void* ws, hipStream_t st) {
    char* base = reinterpret_cast<char*>(ws);
    float* qn = reinterpret_cast<float*>(base);
    _Float16* qh = reinterpret_cast<_Float16*>(base + f.off_qh);
    _Float16* ql = reinterpret_cast<_Float16*>(base + f.off_ql);
    int* flag = reinterpret_cast<int*>(base + f.off_flag);
    u64* cand = reinterpret_cast<u64*>(base + f.off_cand);
    u64* partial = reinterpret_cast<u64*>(base + f.off_partial);
    const int qpad_max = f.Qpad > ex.Qpad ? f.Qpad : ex.Qpad;
    hipLaunchKernelGGL(normalize_rows_kernel<false>, dim3((qpad_max + 3) / 4), dim3(256), 0, st, q, (void*)qn, (int64_t)Q,
                       (int64_t)qpad_max, ix->dim, 1e-12f, 0);
    const size_t nq = (size_t)f.Qpad * ix->dim;
    int rc;
    if (f.resident) {
        hipLaunchKernelGGL(split_queries_act_kernel, dim3((unsigned)((nq / 4 + 255) / 256 < 1024 ? (nq / 4 + 255) / 256 : 1024)),
                           dim3(256), 0, st, (const float*)qn, nq / 4, qh, ql, flag);
        rc = launch_arm(resident_search_kernel<CfgRes>, resident_search_kernel<CfgRes, FacetArgs>,
                        resident_search_kernel<CfgRes, SetArgs>, sa, true, T_SEARCH_KERNEL,
                        dim3(f.n_chunks * f.n_qtiles), dim3(CfgRes::THREADS), f.smem, st, (const _Float16*)ix->filter.frag, ix->n_rows,
                        (const _Float16*)qh, (const _Float16*)ql, f.Qpad, Q, f.kp, ei, eo, (uint32_t)ix->row_offset,
                        f.n_row_tiles, f.tiles_per_chunk, f.n_qtiles, partial);
    } else {
        hipLaunchKernelGGL(split_planes_kernel<false>, dim3((unsigned)((nq + 255) / 256 < 1024 ? (nq + 255) / 256 : 1024)),
                           dim3(256), 0, st, (const void*)qn, nq, qh, ql, flag);
        rc = launch_arm(staged_search_kernel<CfgFilter>, staged_search_kernel<CfgFilter, FacetArgs>,
                        staged_search_kernel<CfgFilter, SetArgs>, sa, true, T_SEARCH_KERNEL,
                        dim3(f.n_chunks * f.n_qtiles), dim3(CfgFilter::THREADS), f.smem, st, (const _Float16*)ix->filter.plane_hi,
                        (const _Float16*)ix->filter.plane_lo, ix->n_rows, ix->dim, (const _Float16*)qh, (const _Float16*)ql, f.Qpad, Q,
                        f.kp, ei, eo, (uint32_t)ix->row_offset, f.n_row_tiles, f.tiles_per_chunk, f.n_qtiles, partial);
    }
    if (rc) return rc;
    ICREC_HIP(hipGetLastError());
    launch_merge(partial, f.n_chunks, f.Qpad, Q, f.kp, nullptr, nullptr, cand, nullptr, st);  // (at most 256 lists)
    hipLaunchKernelGGL((rows_are_bf16(ix) ? verify_kernel<true> : verify_kernel<false>), dim3((Q + 3) / 4), dim3(256), 0,
                       st, (const void*)ix->rows, ix->dim, qn, cand, Q, f.kp, k, (uint32_t)ix->row_offset,
                       filter_eps(ix->dim), out_idx, out_score, out_keys, flag);
    ICREC_HIP(hipGetLastError());
    // exact pass: every workgroup returns at once unless verify raised the flag
    if (int rc2 = launch_exact(ix, ex, qn, Q, k, ei, eo, sa, partial, nullptr, flag, st)) return rc2;
    launch_merge(partial, ex.n_chunks, ex.Qpad, Q, k, out_idx, out_score, out_keys, flag, st);
    ICREC_HIP(hipGetLastError());
    return ICREC_OK;
}

// allow != NULL (icrec_search_faceted): every selecting kernel runs its FACET arm on the index's facets.
// set_ids != NULL (icrec_search_in_sets): every selecting kernel runs its SETS arm on the index's row sets, with the
// allow masks if there are any.
static int run_search(Index* ix, const float* q, int Q, int k, const int32_t* ei, const int32_t* eo, int64_t* out_idx,
                      float* out_score, u64* out_keys, float* scores_out, void* ws, size_t ws_bytes, hipStream_t st,
                      const uint32_t* allow = nullptr, const int32_t* set_ids = nullptr, int sets_per_query = 0) {
    ICREC_REQUIRE(ix && q, "icrec_search: NULL index or queries");
    ICREC_REQUIRE(Q >= 1, "icrec_search: n_queries must be >= 1 (got %d)", Q);
    ICREC_REQUIRE(k >= 1 && k <= ICREC_MAX_K, "icrec_search: k must be in [1, %d] (got %d)", ICREC_MAX_K, k);
    ICREC_REQUIRE((ei == nullptr) == (eo == nullptr), "icrec_search: excl_idx and excl_off must both be set or both NULL");
    ICREC_REQUIRE(allow == nullptr || ix->facets != nullptr, "icrec_search_faceted: allow masks on an index without facets");
    ICREC_REQUIRE(set_ids == nullptr || ix->rowsets != nullptr, "icrec_search_in_sets: set ids on an index without row sets");
    ICREC_REQUIRE(set_ids == nullptr || (sets_per_query >= 1 && sets_per_query <= ICREC_MAX_SETS_PER_QUERY),
                  "icrec_search_in_sets: sets_per_query must be in [1, %d] (got %d)", ICREC_MAX_SETS_PER_QUERY, sets_per_query);
    // (the SETS arm without allow masks: no facet words are read and the masks it loads are all ones)
    const FacetArgs fa = allow ? FacetArgs{ix->facets, allow, ix->n_facets} : FacetArgs{nullptr, nullptr, 0};
    const SetArgs sa{fa, ix->rowsets, set_ids, ix->n_rowsets, sets_per_query, rowset_words(ix->capacity)};
    const Arm arm = arm_of(sa);
    if (scores_out == nullptr && (ix->filter.plane_hi != nullptr || ix->filter.frag != nullptr)) {
        const Plan ex = make_plan(ix, Q, k, false, arm);
        const FilterPlan f = make_filter_plan(ix, Q, k, ex, arm);
        if (f.use) {
            if (ws_bytes < f.ws_total || ws == nullptr) {
                set_error("icrec_search: workspace too small (%zu < %zu)", ws_bytes, f.ws_total);
                return ICREC_ENOMEM;
            }
            ICREC_HIP(hipSetDevice(ix->device));
            ScopedTimer whole(T_SEARCH, st);
            return run_search_filtered(ix, f, ex, q, Q, k, ei, eo, sa, out_idx, out_score, out_keys, ws, st);
        }
    }
    const Plan p = make_plan(ix, Q, k, scores_out == nullptr, arm);
    if (ws_bytes < p.ws_total || ws == nullptr) {
        set_error("icrec_search: workspace too small (%zu < %zu)", ws_bytes, p.ws_total);
        return ICREC_ENOMEM;
    }
    ICREC_HIP(hipSetDevice(ix->device));
    ScopedTimer whole(T_SEARCH, st);
    float* qn = reinterpret_cast<float*>(ws);
    u64* partial = reinterpret_cast<u64*>(reinterpret_cast<char*>(ws) + p.ws_q);
    hipLaunchKernelGGL(normalize_rows_kernel<false>, dim3((p.Qpad + 3) / 4), dim3(256), 0, st, q, (void*)qn, (int64_t)Q,
                       (int64_t)p.Qpad, ix->dim, 1e-12f, p.variant == 3 ? p.Qpad : 0);
    if (int rc = launch_exact(ix, p, qn, Q, k, ei, eo, sa, partial, scores_out, nullptr, st)) return rc;
    if (out_idx || out_keys) {
        if (!launch_merge_block(partial, p.n_chunks, p.Qpad, Q, k, out_idx, out_score, out_keys, st))
            launch_merge(partial, p.n_chunks, p.Qpad, Q, k, out_idx, out_score, out_keys, nullptr, st);
        ICREC_HIP(hipGetLastError());
    }
    return ICREC_OK;
}

}  // namespace icrec

using namespace icrec;

extern "C" {

size_t icrec_search_workspace_bytes(const icrec_index* h, int32_t n_queries, int32_t k) {
    const Index* ix = reinterpret_cast<const Index*>(h);
    if (!ix || n_queries < 1 || k < 1 || k > ICREC_MAX_K) return 0;
    const Plan ex = make_plan(ix, n_queries, k, false);
    const size_t a = ex.ws_total, b = make_plan(ix, n_queries, k, true).ws_total;
    const size_t c = make_filter_plan(ix, n_queries, k, ex).ws_total;
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

int icrec_search(icrec_index* h, const float* q_dev, int32_t n_queries, int32_t k, const int32_t* excl_idx_dev,
                 const int32_t* excl_off_dev, int64_t* out_idx_dev, float* out_score_dev, void* ws, size_t ws_bytes,
                 void* stream) {
    ICREC_REQUIRE(out_idx_dev && out_score_dev, "icrec_search: NULL output");
    return run_search(reinterpret_cast<Index*>(h), q_dev, n_queries, k, excl_idx_dev, excl_off_dev, out_idx_dev,
                      out_score_dev, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream);
}

size_t icrec_search_faceted_workspace_bytes(const icrec_index* h, int32_t n_queries, int32_t k) {
    return icrec_search_workspace_bytes(h, n_queries, k);  // the plans of a faceted search cut the rows the same way
}

int icrec_search_faceted(icrec_index* h, const float* q_dev, int32_t n_queries, int32_t k, const int32_t* excl_idx_dev,
                         const int32_t* excl_off_dev, const uint32_t* allow_dev, int64_t* out_idx_dev, float* out_score_dev,
                         void* ws, size_t ws_bytes, void* stream) {
    ICREC_REQUIRE(out_idx_dev && out_score_dev, "icrec_search_faceted: NULL output");
    return run_search(reinterpret_cast<Index*>(h), q_dev, n_queries, k, excl_idx_dev, excl_off_dev, out_idx_dev,
                      out_score_dev, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream, allow_dev);
}

size_t icrec_search_in_sets_workspace_bytes(const icrec_index* h, int32_t n_queries, int32_t k) {
    return icrec_search_workspace_bytes(h, n_queries, k);  // the plans of a set-restricted search cut the rows the same way
}

int icrec_search_in_sets(icrec_index* h, const float* q_dev, int32_t n_queries, int32_t k, const int32_t* excl_idx_dev,
                         const int32_t* excl_off_dev, const uint32_t* allow_dev, const int32_t* set_ids_dev,
                         int32_t sets_per_query, int64_t* out_idx_dev, float* out_score_dev, void* ws, size_t ws_bytes,
                         void* stream) {
    ICREC_REQUIRE(out_idx_dev && out_score_dev, "icrec_search_in_sets: NULL output");
    return run_search(reinterpret_cast<Index*>(h), q_dev, n_queries, k, excl_idx_dev, excl_off_dev, out_idx_dev,
                      out_score_dev, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream, allow_dev, set_ids_dev,
                      sets_per_query);
}

int icrec_search_partial(icrec_index* h, const float* q_dev, int32_t n_queries, int32_t k, const int32_t* excl_idx_dev,
                         const int32_t* excl_off_dev, uint64_t* out_keys_dev, void* ws, size_t ws_bytes, void* stream) {
    ICREC_REQUIRE(out_keys_dev, "icrec_search_partial: NULL output");
    return run_search(reinterpret_cast<Index*>(h), q_dev, n_queries, k, excl_idx_dev, excl_off_dev, nullptr, nullptr,
                      reinterpret_cast<u64*>(out_keys_dev), nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int icrec_scores(icrec_index* h, const float* q_dev, int32_t n_queries, float* out_dev, void* ws, size_t ws_bytes,
                 void* stream) {
    ICREC_REQUIRE(out_dev, "icrec_scores: NULL output");
    return run_search(reinterpret_cast<Index*>(h), q_dev, n_queries, 1, nullptr, nullptr, nullptr, nullptr, nullptr,
                      out_dev, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
