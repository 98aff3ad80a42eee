/*
 * icrec.h — C ABI of libicrec.so, the MI355X (gfx950) implementation of the
 * reference's SBERT-encode -> cosine-similarity -> top-k hot path.
 *
 * The reference (chen-bowen/instacart_next_order_recommendation) has no FFI of
 * its own: its seam is the Python duck type `Recommender.recommend()`
 * (src/inference/serve_recommendations.py:206-225).  Each entry point below
 * names the reference call it replaces.  The Python host classes in
 * instacart_next_order_recommendation_amd/ bind these symbols with ctypes
 * (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 * Conventions
 *  - every function returns 0 on success, a negative ICREC_E* code on failure;
 *    icrec_last_error() returns a thread-local message for the last failure.
 *  - handles are opaque, owned by the library until the matching *_destroy.
 *  - "dev" pointers are device (HBM) pointers, borrowed for the duration of
 *    the call's stream work; "host" pointers are read before the call returns.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *    work is enqueued asynchronously; nothing here synchronises the device
 *    except *_create/_destroy.
 *  - scratch memory is supplied by the caller (`workspace`), sized by the
 *    matching *_workspace_bytes(); the library never allocates on the hot path
 *    so every call is hipGraph-capturable.
 *  - no torch / C++ types cross this boundary.
 */
#ifndef ICREC_H
#define ICREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* every entry point is exported from libicrec.so (built with -fvisibility=hidden) */
#define ICREC_API __attribute__((visibility("default")))

#define ICREC_VERSION_MAJOR 0
#define ICREC_VERSION_MINOR 1

enum {
    ICREC_OK = 0,
    ICREC_EINVAL = -1,   /* bad argument (shape, NULL, k out of range ...) */
    ICREC_EHIP = -2,     /* a HIP runtime call failed                      */
    ICREC_ENOMEM = -3,   /* workspace too small / allocation failed        */
    ICREC_ENODEV = -4    /* no gfx950 device visible                        */
};

/* k is bounded by the reference's API schema (src/api/schemas.py:34, top_k<=100);
 * the kernels are built for k <= ICREC_MAX_K. */
#define ICREC_MAX_K 128

typedef struct icrec_encoder icrec_encoder;
typedef struct icrec_index icrec_index;
typedef struct icrec_cf icrec_cf;

/* ------------------------------------------------------------------------- */
/* Encoder: replaces SentenceTransformer.encode's device work                 */
/* (serve_recommendations.py:195-200, :213, :246): BertModel forward          */
/* (transformers modeling_bert.py BertEmbeddings/BertLayer), mean pooling,    */
/* L2 normalisation.  Tokenisation stays on the host.                         */
/* ------------------------------------------------------------------------- */

typedef struct icrec_bert_cfg {
    int32_t vocab_size;    /* 30522 for all-MiniLM-L6-v2 and BERT-base        */
    int32_t hidden;        /* 384 (all-MiniLM) or 768 (BERT-base: e5-base-v2,
                              gte-base, bert-base-nli-mean-tokens)            */
    int32_t layers;        /* 6 / 12; in [1, 64]                              */
    int32_t heads;         /* 12: head_dim must be 32 at hidden 384 and 64 at
                              hidden 768; any other (hidden, heads) pair is
                              ICREC_EINVAL                                    */
    int32_t intermediate;  /* 1536 / 3072 (must be a multiple of 384)         */
    int32_t max_position;  /* 512                                            */
    int32_t type_vocab;    /* 2                                              */
    float   ln_eps;        /* 1e-12                                          */
    int32_t n_normalize;   /* how many times x / max(|x|_2, 1e-12) is applied
                              after pooling: 1 for the ST `Normalize` module,
                              +1 for encode(normalize_embeddings=True)       */
    int32_t gemm_mode;     /* ICREC_GEMM_F32: every linear layer on the exact
                              f32 MFMA (bit-identical to the oracle's fmaf
                              chains); ICREC_GEMM_F16X3: linear layers on the
                              f16 MFMA with 3-term operand splitting (fp32-level
                              accuracy, ~2^-21 relative per product; csrc/wt_gemm.h) */
} icrec_bert_cfg;

#define ICREC_GEMM_F32 0
#define ICREC_GEMM_F16X3 1

/* Number of fp32 elements the weight blob must hold for `cfg`.
 * Blob layout (all fp32, row-major, HF `nn.Linear` weights are [out,in]):
 *   word_emb[V,H] pos_emb[P,H] type_emb[Tv,H] emb_ln_g[H] emb_ln_b[H]
 *   then per layer:
 *   Wq[H,H] bq[H] Wk[H,H] bk[H] Wv[H,H] bv[H] Wo[H,H] bo[H] ln1_g[H] ln1_b[H]
 *   W1[I,H] b1[I] W2[H,I] b2[H] ln2_g[H] ln2_b[H]
 * (the BertPooler is not used by mean pooling and is not part of the blob; a cross-encoder's pooler and classifier are
 * set on the handle: icrec_encoder_set_score_head). */
ICREC_API size_t icrec_encoder_weight_count(const icrec_bert_cfg* cfg);

/* Upload weights (host pointer; the library copies them to `device`). */
ICREC_API int icrec_encoder_create(const float* weights_host, size_t n_floats,
                         const icrec_bert_cfg* cfg, int device,
                         icrec_encoder** out);
ICREC_API int icrec_encoder_destroy(icrec_encoder* enc);

/* Longest sequence any encoder can take: every BERT shape has at most 512 position embeddings. */
#define ICREC_MAX_SEQLEN 512

/* Raise (or lower) the longest sequence `enc` accepts, in [1, min(ICREC_MAX_SEQLEN, cfg.max_position)]; anything
 * else returns ICREC_EINVAL.  After icrec_encoder_create the ceiling is min(256, cfg.max_position) (sentence-transformers'
 * default max_seq_length), so a caller that never sets it sees the 256-token limit.  Set it before the first
 * icrec_encode, never while another call on `enc` is running.  Sequences of up to 256 tokens encode to the same bits
 * whatever the ceiling. */
ICREC_API int icrec_encoder_set_max_seqlen(icrec_encoder* enc, int32_t max_seqlen);

/* How the last hidden states become one row per sequence (sentence-transformers' Pooling module). */
#define ICREC_POOL_MEAN 0   /* sentence-transformers Pooling(mean): the default after icrec_encoder_create */
#define ICREC_POOL_CLS  1   /* Pooling(cls): the last hidden state of each sequence's first token */

/* Choose the pooling mode of `enc`; any other value returns ICREC_EINVAL.  Same contract as
 * icrec_encoder_set_max_seqlen: set it before the first icrec_encode, never while another call on `enc` is running.
 * The weights are untouched, and cfg.n_normalize applies after pooling in either mode: in CLS mode out_dev[s] is the
 * last hidden state of token cu_seqlens[s], normalised n_normalize times; tokens_out_dev does not depend on the mode.
 * In f16x3 mode a CLS encoder computes its last layer for the first token of each sequence only (the layer's K and V
 * still cover every token) unless tokens_out_dev asks for every row; the embedding has the same bits either way.
 * ICREC_CLS_PRUNE=0 in the environment at icrec_encoder_create forces the full last layer. */
ICREC_API int icrec_encoder_set_pooling(icrec_encoder* enc, int32_t mode);
/* The pooling mode of `enc`; -1 for a NULL handle. */
ICREC_API int32_t icrec_encoder_pooling(const icrec_encoder* enc);

/* Additive attention bias by relative position (MPNet / T5 style).  bias_host: float[heads][2*ICREC_MAX_SEQLEN - 1],
 * head-major; entry [h][ICREC_MAX_SEQLEN - 1 + (j - i)] is added to the logit of query i against key j of head h
 * (positions inside the token's own sequence), after the 1/sqrt(head_dim) scale and before the softmax, in EVERY layer.
 * NULL removes the bias.  heads must equal cfg.heads; every value must be finite; anything else is ICREC_EINVAL and
 * changes nothing.  Same contract as icrec_encoder_set_pooling: before the first icrec_encode, never while a call on
 * `enc` is running.  A set-up call like icrec_encoder_create: it allocates and copies, and may synchronise the device.
 * The table (kept in log2 units, 4 KB per head) lives on the handle: icrec_bert_cfg, the weight blob and
 * icrec_encode_workspace_bytes do not know it.  An encoder with a bias launches the BIAS arm of the two attention
 * kernels (the head's row in LDS, one fma per logit, the row maximum taken over the biased logits) in every form
 * attention is launched in; one without launches what it always did, to the same bits.  A sequence encodes to the same
 * bits alone and inside any batch, with or without a bias. */
ICREC_API int icrec_encoder_set_attention_bias(icrec_encoder* enc, const float* bias_host, int32_t heads);
ICREC_API int32_t icrec_encoder_has_attention_bias(const icrec_encoder* enc);   /* 0 / 1; -1 for NULL */

/* Score head of a cross-encoder (BertForSequenceClassification with num_labels = 1: the cross-encoder/ms-marco-MiniLM
 * family): the BertPooler and the classifier, applied by icrec_score_pairs to the last hidden state h of each sequence's
 * first token:  p = tanh(pooler_w . h + pooler_b),  logit = cls_w . p + cls_b.
 *   pooler_w_host float[hidden][hidden] row-major [out, in] as nn.Linear stores it;  pooler_b_host float[hidden];
 *   cls_w_host float[hidden];  cls_b_host float[1].
 * pooler_w_host == NULL removes the head.  Every value must be finite and cfg.type_vocab must be >= 2 (a pair's second
 * segment takes token-type row 1); anything else is ICREC_EINVAL and changes nothing.  Same contract as
 * icrec_encoder_set_attention_bias: a set-up call that allocates and copies, before the first compute call, never while a
 * call on `enc` is running.  The head lives on the handle: icrec_bert_cfg, the weight blob, icrec_encoder_weight_count and
 * icrec_encode_workspace_bytes do not know it, and icrec_encode on an encoder with a head launches what it launches on
 * one without, to the same bits. */
ICREC_API int icrec_encoder_set_score_head(icrec_encoder* enc, const float* pooler_w_host, const float* pooler_b_host,
                                 const float* cls_w_host, const float* cls_b_host);
ICREC_API int32_t icrec_encoder_has_score_head(const icrec_encoder* enc);   /* 0 / 1; -1 for NULL */

/* Scratch bytes needed to encode `total_tokens` tokens in `n_seqs` sequences.  Depends on the pooling mode (a CLS
 * encoder adds room for `n_seqs` compact rows): ask after icrec_encoder_set_pooling.  Does not depend on the bias. */
ICREC_API size_t icrec_encode_workspace_bytes(const icrec_encoder* enc,
                                    int64_t total_tokens, int32_t n_seqs);

/* Encode a token-packed batch.
 *   ids_dev        int32[total_tokens]  WordPiece ids, sequences back to back
 *                                       (already truncated to max_seq_length,
 *                                       [CLS]/[SEP] included; no pad tokens)
 *   cu_seqlens_dev int32[n_seqs+1]      prefix sums of sequence lengths
 *   max_seqlen     longest sequence in the batch (<= the encoder's ceiling:
 *                  256 unless icrec_encoder_set_max_seqlen raised it)
 *   out_dev        float[n_seqs, hidden] L2-normalised sentence embeddings (hidden 384 or 768)
 * Padding never enters the math: the reference pads per batch and masks the
 * pad keys to weight exactly 0, so the packed form is the same function.
 * Stream semantics: asynchronous on `stream`; everything the call enqueues is ordered before whatever the caller
 * enqueues on `stream` afterwards.  For large batches (f16x3 mode) part of the work - the short attention buckets, the
 * remainder of icrec_encode_batch_split - runs on a library-owned side stream (one per caller stream, created on
 * first use) that forks from and joins back into `stream` by events inside the call; under stream capture the call
 * stays on `stream` unless that side stream already exists.  Calls on DIFFERENT streams may run concurrently (own
 * workspaces); calls on one encoder must not be issued from several host threads at once. */
ICREC_API int icrec_encode(icrec_encoder* enc,
                 const int32_t* ids_dev, const int32_t* cu_seqlens_dev,
                 int32_t n_seqs, int64_t total_tokens, int32_t max_seqlen,
                 float* out_dev,
                 void* workspace_dev, size_t workspace_bytes, void* stream);

/* icrec_encode, and additionally the last hidden state of every token (what
 * SentenceTransformer.encode(output_value="token_embeddings") returns) when tokens_out_dev != NULL:
 *   tokens_out_dev float[total_tokens, hidden]  row t is token t of the packed batch; 16-byte aligned
 * The rows are the very values mean pooling summed (in f16x3 mode the two f16 planes of the residual stream, widened
 * exactly), written by one extra copy kernel on `stream` behind the pooling kernel.  With tokens_out_dev == NULL this
 * IS icrec_encode: the same launches, the same bits.  Same workspace size either way. */
ICREC_API int icrec_encode_ex(icrec_encoder* enc,
                    const int32_t* ids_dev, const int32_t* cu_seqlens_dev,
                    int32_t n_seqs, int64_t total_tokens, int32_t max_seqlen,
                    float* out_dev, float* tokens_out_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* How icrec_encode will split `total_tokens` (f16x3 mode): main_tokens go through the batch kernels (whole
 * rounds of one 64-token workgroup per CU; at hidden 384 the fused FFN kernel sees exactly this many tokens), tail_tokens — a
 * remainder of at most 512 tokens — through the small-batch kernels.  Same arithmetic either way; bench.py uses
 * it to count the FLOPs of the launches it times. */
ICREC_API int icrec_encode_batch_split(const icrec_encoder* enc, int64_t total_tokens,
                             int64_t* main_tokens, int64_t* tail_tokens);

/* Scratch bytes icrec_score_pairs needs for `total_tokens` tokens in `n_seqs` pairs (0 for a bad argument).  Does not
 * depend on the pooling mode. */
ICREC_API size_t icrec_score_pairs_workspace_bytes(const icrec_encoder* enc, int64_t total_tokens, int32_t n_seqs);

/* Score a token-packed batch of (query, document) pairs: what sentence-transformers' CrossEncoder.predict computes on the
 * device, before its activation function.  Each sequence is `[CLS] query [SEP] document [SEP]`, packed as for icrec_encode.
 *   seg_b_dev      int32[n_seqs]  where each pair's second segment starts: token t of sequence s takes token-type row 1
 *                                 when t - cu_seqlens[s] >= seg_b[s] and row 0 otherwise (BERT's token_type_ids are
 *                                 always a run of 0s, then a run of 1s); seg_b[s] is clamped to [0, length of s]
 *   scores_out_dev float[n_seqs]  the raw logit of each pair (sigmoid or identity is the caller's choice)
 * The layers run as in icrec_encode_ex; only the first token's last hidden state is read, so in f16x3 mode the last layer is
 * computed for the first token of each sequence only, as for a CLS-pooled encoder and whatever the handle's pooling mode
 * (ICREC_CLS_PRUNE=0 at icrec_encoder_create forces the full layer: same bits); the pooling mode and cfg.n_normalize do not
 * enter.  The head is fp32 with one summation order: a pair's logit has the same bits alone and inside any batch.
 * ICREC_EINVAL without a score head; the other argument checks, the stream semantics and graph-capturability are
 * icrec_encode's.  Workspace: icrec_score_pairs_workspace_bytes. */
ICREC_API int icrec_score_pairs(icrec_encoder* enc,
                      const int32_t* ids_dev, const int32_t* cu_seqlens_dev, const int32_t* seg_b_dev,
                      int32_t n_seqs, int64_t total_tokens, int32_t max_seqlen,
                      float* scores_out_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Reranking glue: icrec_search's candidates -> icrec_score_pairs' packed     */
/* input, and the logits -> the final top k, all on the device.  With these    */
/* retrieve -> rerank is icrec_encode, icrec_search, icrec_assemble_pairs,     */
/* icrec_score_pairs, icrec_rerank_select on one stream with no host step in   */
/* between: capturable for one request, batched for many.  Neither call takes  */
/* an encoder or index handle; `device` is the HIP ordinal of the pointers.    */
/* ------------------------------------------------------------------------- */

/* Scratch bytes icrec_assemble_pairs needs (0 for n_queries < 1 or k outside [1, ICREC_MAX_K]). */
ICREC_API size_t icrec_assemble_pairs_workspace_bytes(int32_t n_queries, int32_t k);

/* Assemble pair p = q * k + j = `[CLS] q_side(q)[:ka] [SEP] cat_side(cand[q][j] - row_offset)[:kb] [SEP]` for every
 * query q and candidate j, packed back to back as icrec_score_pairs takes them.
 *   q_ids_dev / q_cu_dev      int32[q_cu[n_queries]] / int32[n_queries+1]  the queries' cross-encoder token ids, without
 *                             specials, packed, and their prefix sums
 *   cat_ids_dev / cat_cu_dev  int32[cat_cu[n_rows]] / int32[n_rows+1]      the same for the catalog's product sides; row r
 *                             is the index's row row_offset + r
 *   cand_idx_dev              int64[n_queries, k]  icrec_search's out_idx (global rows, -1 pads)
 *   max_len                   ids per pair after truncation, in [3, ICREC_MAX_SEQLEN]
 *   ids_out_dev               int32[ids_cap]       the packed ids; entries from cu_out[n_queries*k] on are NOT written
 *   cu_out_dev                int32[n_queries*k+1] exclusive prefix sums of the pair lengths, computed on the device
 *   seg_b_out_dev             int32[n_queries*k]   ka + 2: where each pair's second segment starts
 * (ka, kb) is the `longest_first` truncation of the `tokenizers` library in closed form: nothing is cut when
 * len_a + len_b <= max_len - 3; otherwise the longer side gives way until the sides are level, and from there the shorter
 * side - the FIRST on an exact tie - ends with floor((max_len - 3) / 2) tokens and the other with the rest.
 * A candidate that is negative or outside [row_offset, row_offset + n_rows) becomes the three-token pair
 * `[CLS] [SEP] [SEP]` with seg_b = 2: no sequence is ever empty.
 * Which candidates arrive is known on the device only, so the caller bounds the token count from the host:
 *   ids_cap >= sum over q of k * min(max_len, 3 + len_q + longest product side)
 * and then calls icrec_score_pairs(n_seqs = n_queries*k, total_tokens = ids_cap, max_seqlen = the largest term's
 * min(...)): token rows past cu_out[n_seqs] are computed and ignored (the embedding kernel clamps ids and positions, every
 * other kernel is per row or reads cu_seqlens), and a pair's logit has the bits it has in an exactly sized batch.
 * Every write is clamped to ids_cap: should the lengths not fit, the pairs from the first one that would leave fewer
 * than three tokens for each later pair are all emitted as `[CLS] [SEP] [SEP]` - a safety net a correct bound never meets.
 * ICREC_EINVAL: a NULL pointer, n_queries < 1, k outside [1, ICREC_MAX_K], max_len outside [3, ICREC_MAX_SEQLEN],
 * n_queries * k * max_len >= 2^31 (the prefix sums are int32), ids_cap < 3 * n_queries * k.  ICREC_ENOMEM: workspace. */
ICREC_API int icrec_assemble_pairs(const int32_t* q_ids_dev, const int32_t* q_cu_dev, int32_t n_queries,
                         const int32_t* cat_ids_dev, const int32_t* cat_cu_dev, int64_t n_rows, int64_t row_offset,
                         const int64_t* cand_idx_dev, int32_t k,
                         int32_t max_len, int32_t cls_id, int32_t sep_id,
                         int32_t* ids_out_dev, int64_t ids_cap, int32_t* cu_out_dev, int32_t* seg_b_out_dev,
                         void* workspace_dev, size_t workspace_bytes, int device, void* stream);

/* The best top_k <= k candidates of each query by cross-encoder logit.
 *   logits_dev     float[n_queries, k]      icrec_score_pairs' output for icrec_assemble_pairs' pairs
 *   cand_idx_dev   int64[n_queries, k]      the candidates (icrec_search's out_idx)
 *   cand_score_dev float[n_queries, k]      icrec_search's out_score, or NULL: not read (the retrieval order is the
 *                                           position j), taken so that a caller passes a search result as it is
 *   out_idx_dev    int64[n_queries, top_k]  best first; -1 where fewer than top_k candidates had idx >= 0
 *   out_logit_dev  float[n_queries, top_k]  their raw logits (0 where idx == -1)
 * Order: logit descending (compared as floats), ties by lower retrieval position j, a NaN logit after every number;
 * candidates with idx < 0 are skipped.  The outputs may be pinned host memory.  The model's activation (sigmoid or
 * identity) is the caller's, applied to the top_k returned logits.  Ordering on the logit refines ordering on the
 * activated score: the two differ only where float32 sigmoid maps distinct logits to one value, and there the logit order
 * still separates what the score order leaves to the position.
 * ICREC_EINVAL: a NULL pointer (cand_score_dev excepted), n_queries < 1, k outside [1, ICREC_MAX_K], top_k outside [1, k]. */
ICREC_API int icrec_rerank_select(const float* logits_dev, const int64_t* cand_idx_dev, const float* cand_score_dev,
                        int32_t n_queries, int32_t k, int32_t top_k,
                        int64_t* out_idx_dev, float* out_logit_dev, int device, void* stream);

/* ------------------------------------------------------------------------- */
/* Index + search: replaces cos_sim(query_emb, product_embeddings)            */
/* (serve_recommendations.py:214/:250), scores.argsort(descending=True)       */
/* (:215/:251) and the exclusion/top-k loop (:216-225/:254-262).              */
/* ------------------------------------------------------------------------- */

/* Build an index over a [n_rows, dim] fp32 row-major matrix in device memory.
 * The library keeps its own copy with every row divided by max(|row|_2,1e-12)
 * (what cos_sim does to its second operand on every call in the reference).
 * `row_offset` is added to every returned row index (catalog shards).
 * `dim` must be a multiple of 32 in [32, 4096].                              */
ICREC_API int icrec_index_create(const float* rows_dev, int64_t n_rows, int32_t dim,
                       int64_t row_offset, int device, icrec_index** out);

/* Same, choosing how the normalised rows are kept in HBM (BASELINE config 5: a 10M x 384
 * bf16 catalog, 7.68 GB instead of 15.4 GB):
 *   ICREC_ROWS_F32   the fp32 quotient itself (what icrec_index_create does);
 *   ICREC_ROWS_BF16  the fp32 quotient rounded to bfloat16, round-to-nearest-even.
 * Only the storage changes: scores are still the fp32 fmaf chain over k of
 * q_hat[k] * float(row[k]) on the exact-f32 MFMA, so results are bit-identical to
 * oracle/icrec_oracle.c:icrec_oracle_search_bf16 (same rounded rows, same chain).
 * The bf16 storages (ICREC_ROWS_BF16, ICREC_ROWS_BF16_FILTER) and the filter storages need dim % 64 == 0
 * (bf16 rows are read in 128-byte slabs of 64 values; every real embedding width - 384, 512, 768, 1024 -
 * is one); other widths return ICREC_EINVAL.                                                  */
#define ICREC_ROWS_F32 0
#define ICREC_ROWS_BF16 1
/*   ICREC_ROWS_F32_FILTER  fp32 rows PLUS their f16 hi/lo planes (2x the HBM).  Batches of >= 256 queries
 *                    are first ranked on the f16 matrix cores (3 MFMAs per product, scores within ~1e-7, 5x
 *                    the fp32-MFMA rate) keeping k+12 candidates per query; every candidate is then re-scored
 *                    with the exact fp32 chain and the best k returned.  A query whose (k+12)-th candidate
 *                    is not provably below its exact k-th score (margin max(1e-4, 2 dim 2^-24 + 1e-6):
 *                    1e-4 up to dim 768, 1.2e-4 at 1,024, 4.9e-4 at 4,096) makes the exact search run
 *                    for the batch instead — results are therefore ALWAYS bit-identical to
 *                    ICREC_ROWS_F32, only faster for large catalogs x large batches.                    */
#define ICREC_ROWS_F32_FILTER 2
/*   ICREC_ROWS_BF16_FILTER  the same two-pass search over ICREC_ROWS_BF16 rows: bf16 rows (the exact pass and the
 *                    verification read these) plus f16 hi/lo planes of the rounded rows (3x the bf16 bytes
 *                    in total); bit-identical to ICREC_ROWS_BF16.                                        */
#define ICREC_ROWS_BF16_FILTER 3
ICREC_API int icrec_index_create_ex(const float* rows_dev, int64_t n_rows, int32_t dim,
                          int64_t row_offset, int device, int32_t storage, icrec_index** out);
ICREC_API int icrec_index_destroy(icrec_index* idx);
ICREC_API int64_t icrec_index_rows(const icrec_index* idx);
ICREC_API int64_t icrec_index_row_offset(const icrec_index* idx); /* global number of the shard's first row */
ICREC_API int32_t icrec_index_storage(const icrec_index* idx); /* ICREC_ROWS_* (-1: NULL handle) */
ICREC_API int32_t icrec_index_dim(const icrec_index* idx);     /* embedding width (0: NULL handle)  */
ICREC_API int32_t icrec_index_device(const icrec_index* idx);  /* HIP device ordinal (-1: NULL)     */

/* Copy the normalised rows back out (row-major fp32 [n_rows, dim]; bf16 storage is
 * widened exactly); used by the parity tests and by EmbeddingIndex.save.     */
ICREC_API int icrec_index_export(const icrec_index* idx, float* rows_dev, void* stream);

/* The filter copy of a *_FILTER storage as f16 bits, row-major [n_rows, dim] each: the values the filter pass
 * multiplies, as stored - the hi/lo planes, or for the resident form (dim 384) the packed fragments un-packed (their
 * values carry the fragments' scale, 1024).  hi_dev, lo_dev: DEVICE memory; asynchronous on `stream`.  ICREC_EINVAL for
 * a NULL argument or a storage without a filter copy.  Beside icrec_index_export, for the parity tests: a search's
 * result cannot show a filter copy that is merely stale. */
ICREC_API int icrec_index_export_filter(const icrec_index* idx, uint16_t* hi_dev, uint16_t* lo_dev, void* stream);

/* Rewrite rows of the index in place: a product's text changed, or the encoder was trained again and every row did.
 *   rows_dev     float[m, dim]  the new rows in DEVICE memory, of any norm
 *   row_ids_dev  int32[m]       the LOCAL rows they replace, in DEVICE memory, ascending and unique
 * For every entry i with 0 <= row_ids[i] < n_rows, everything the index keeps for that row becomes what
 * icrec_index_create_ex would have written for it from rows[i], bit for bit: the stored row (the same normalisation in
 * the same reduction order, the same division, the same bfloat16 rounding) and, in the *_FILTER storages, its filter
 * copy in whichever form the handle has - the row's entries of the hi/lo planes, or for dim 384 its lane slots of the
 * packed fragments - made from the STORED (rounded) value.  No other row and no padding row of the fragments changes:
 * after the call the handle is the one icrec_index_create_ex makes from the edited matrix.  Facets, row sets, the row
 * offset and every pointer of the handle stay: a graph captured before the write and replayed after it searches the new
 * rows.
 * An entry outside [0, n_rows) is skipped before any address is formed from it (the ids live in device memory, where
 * the host cannot refuse them).  A list that is not ascending and unique gives an unspecified result for the rows it
 * names, until they are written again, but a memory-safe one: nothing outside the index's arrays is ever written.
 * Asynchronous on `stream` and ordered like any other work on it: no workspace, nothing is allocated, nothing
 * synchronises; capturable into a hipGraph, the ids and the rows being read from device memory when the kernel runs (a
 * replay follows what the two buffers then hold).  The caller must not let it run concurrently with a call on the same
 * index on another stream.  One launch, one wavefront per written row: rewriting all n_rows rows is how a re-trained
 * model is brought in.
 * m == 0 returns ICREC_OK and launches nothing.  ICREC_EINVAL, before any HIP call: a NULL idx, m < 0, a NULL pointer
 * with m > 0.
 * An icrec_ivf over the index owns its copy of the rows and does not see a write (see icrec_ivf_create). */
ICREC_API int icrec_index_write_rows(icrec_index* idx, const float* rows_dev, const int32_t* row_ids_dev,
                                     int32_t m, void* stream);

/* Add and remove rows in place: a catalog gains and loses products every day, and the handle - with its facets, its row
 * sets and everything its users captured or uploaded - lives on.
 *
 * Capacity.  Every array of a handle (the rows, the hi/lo planes or the packed fragments, the facet words, the row set
 * bitmaps) is sized for `capacity` rows, of which the first n_rows exist; icrec_index_create_ex makes capacity ==
 * n_rows.  The fragments hold whole 256-row rounds of the capacity, the facet words whole 256-row tiles of it, and one
 * row set takes ceil(capacity / 256) * 8 words on the device; bits_host of icrec_index_set_rowsets and
 * icrec_index_write_rowset stays ceil(n_rows / 32) words per set.  What a fresh index keeps zero behind its last row
 * stays zero after every call below: the fragment lane slots, the facet words and the row set bits of rows >= n_rows.
 * The stored rows and the planes past n_rows are unspecified; nothing addresses them.  So after any sequence of these
 * calls the handle searches, exports and ranks, bit for bit, as the handle icrec_index_create_ex builds from the
 * resulting matrix (with the resulting facets and sets) does.
 *
 * Contract of icrec_index_reserve, icrec_index_append_rows and icrec_index_remove_rows:
 *   - they are set-up calls: never while a search (or any other call) on the handle runs;
 *   - after the host-side checks, append and remove are asynchronous on `stream` and ordered like other work on it
 *     (they may allocate a staging block the first time, and wait for their own previous copy out of it); reserve
 *     allocates, synchronises the device and returns when the copy is done;
 *   - n_rows is a launch argument of every search kernel, so UNLIKE icrec_index_write_rows: a graph captured before
 *     any of the three calls is INVALID afterwards and must be captured again (reserve changes every pointer as well);
 *     workspace sizes depend on n_rows and are asked for again;
 *   - an icrec_ivf over the handle owns a copy of the rows in list order: destroy it and create it again;
 *   - they work on the LOCAL rows of any handle, whatever its row_offset; keeping the shards of a sharded search
 *     consistent is the caller's business. */
/* Rows the handle's arrays are sized for (0: NULL handle). */
ICREC_API int64_t icrec_index_capacity(const icrec_index* idx);
/* Re-allocate every array of the handle for `capacity` rows (n_rows <= capacity, row_offset + capacity < 2^32 - 1; it
 * may shrink down to n_rows), copy the live contents device to device and free the old arrays.  The storage form (planes
 * or fragments) was chosen at creation and stays.  ICREC_EINVAL for a capacity out of range; ICREC_ENOMEM when an
 * allocation fails - the handle is then unchanged.  capacity == icrec_index_capacity(idx) does nothing. */
ICREC_API int icrec_index_reserve(icrec_index* idx, int64_t capacity);
/* Append m rows: they become rows n_rows .. n_rows + m - 1, normalised and stored exactly as icrec_index_create_ex would
 * store them (icrec_index_write_rows' kernel and arithmetic, lane for lane), with their filter copy.
 *   rows_dev     float[m, dim]             the new rows in DEVICE memory, of any norm
 *   facets_host  uint8[m, n_facets]        HOST pointer, required exactly when the index has facets (copied before
 *                                          the call returns)
 * The new rows are members of no row set (icrec_index_write_rowset makes them members).  n_rows grows on the host when
 * the call is made.  m == 0 returns ICREC_OK and does nothing.  ICREC_EINVAL, changing nothing: a NULL idx, m < 0, NULL
 * rows_dev, n_rows + m > capacity (reserve first), facets_host missing or unexpected. */
ICREC_API int icrec_index_append_rows(icrec_index* idx, const float* rows_dev, int32_t m, const uint8_t* facets_host,
                                      void* stream);
/* Remove m rows by swapping from the tail: O(m) work, whatever n_rows is.
 *   row_ids_host  int32[m]  HOST pointer: LOCAL rows, ascending and unique, inside [0, n_rows); m < n_rows
 *   dst_out, src_out  int32[m]  HOST arrays that receive the move plan;  n_moves_out  int32*  its length
 * The plan.  new_n = n_rows - m.  The holes are the removed ids below new_n, ascending; the fillers are the surviving
 * rows at or past new_n, ascending; there are as many of one as of the other, and filler i moves into hole i:
 * row src_out[i] becomes row dst_out[i], for i < *n_moves_out (<= m).  Every other surviving row keeps its number.
 * Afterwards the handle is bit for bit the one built from the matrix with those moves applied and cut to new_n rows: a
 * move copies the STORED bits of the row (no second normalisation), its entries of the planes or its lane slots of the
 * fragments, its facet word and its bit of every row set; then the fragment slots, facet words and row set bits of the
 * rows [new_n, old n_rows) are cleared, in a second launch behind the moves.  The caller applies the plan to whatever it
 * keeps per row (ids, texts, memberships).  n_rows shrinks on the host when the call is made.
 * m == 0 returns ICREC_OK with *n_moves_out = 0.  ICREC_EINVAL, changing nothing: a NULL argument, m < 0, m >= n_rows, an
 * id outside [0, n_rows), ids that are not ascending and unique. */
ICREC_API int icrec_index_remove_rows(icrec_index* idx, const int32_t* row_ids_host, int32_t m, int32_t* dst_out,
                                      int32_t* src_out, int32_t* n_moves_out, void* stream);

ICREC_API size_t icrec_search_workspace_bytes(const icrec_index* idx, int32_t n_queries,
                                    int32_t k);

/* Top-k search.
 *   q_dev        float[n_queries, dim]  query embeddings (any norm; normalised
 *                                       here exactly as cos_sim does)
 *   excl_idx_dev int32[excl_off[n_queries]] LOCAL row numbers to skip, sorted
 *                ascending and unique within each query's segment (or NULL)
 *   excl_off_dev int32[n_queries+1]     CSR offsets into excl_idx_dev (or NULL)
 *   out_idx_dev  int64[n_queries, k]    row_offset + row, best first; -1 pads
 *                                       when fewer than k rows remain
 *   out_score_dev float[n_queries, k]   cosine scores (0 where idx == -1)
 * Order: score descending, ties by lower row index first.
 * Every score is the fp32 chain s = fmaf(q[j], p[j], s) for j = 0..dim-1,
 * bit-identical to oracle/icrec_oracle.c:icrec_oracle_scores.                */
ICREC_API int icrec_search(icrec_index* idx, const float* q_dev, int32_t n_queries,
                 int32_t k,
                 const int32_t* excl_idx_dev, const int32_t* excl_off_dev,
                 int64_t* out_idx_dev, float* out_score_dev,
                 void* workspace_dev, size_t workspace_bytes, void* stream);

/* Facets: restrict each query to rows whose attributes it allows ("only from these departments").
 * An index may carry n_facets in [1, ICREC_MAX_FACETS] attribute bytes per row (values 0..255); a query carries, per
 * facet, a 256-bit allow mask of ICREC_FACET_MASK_WORDS uint32 words: bit (v & 31) of word (v >> 5) admits value v.
 * A row is admissible for a query iff, for every facet, the bit of the row's value is set - and the row is not in the
 * query's exclusion list; the two compose.  An all-ones mask leaves a facet unconstrained, an all-zero mask admits
 * nothing (the result is all -1 / 0.0 pads, as when exclusions exhaust the catalog).
 * The result of icrec_search_faceted is bit-identical, indices and scores, to icrec_search with exclusion lists equal
 * to the given exclusions united with every inadmissible row, for every row storage and every batch size. */
#define ICREC_MAX_FACETS 2
#define ICREC_FACET_MASK_WORDS 8

/* Set, replace or (facets_host == NULL) remove the index's facets.
 *   facets_host  uint8[n_rows, n_facets]  HOST pointer, row-major; copied to the device before the call returns
 * n_facets outside [1, ICREC_MAX_FACETS] (with a non-NULL facets_host) is ICREC_EINVAL and changes nothing.
 * A set-up call like icrec_encoder_set_attention_bias: it allocates, may synchronise the device, and must never be
 * issued while a call on the index is running.  The rows and their filter planes / fragments are not touched, and
 * icrec_search, icrec_search_partial, icrec_rank_all and icrec_scores ignore the facets. */
ICREC_API int icrec_index_set_facets(icrec_index* idx, const uint8_t* facets_host, int32_t n_facets);
/* Facets per row of the index: 0 when none are set, -1 for a NULL handle. */
ICREC_API int32_t icrec_index_facets(const icrec_index* idx);
/* Replace the facet values of m rows (a product moved to another aisle).
 *   row_ids_host  int32[m]                               HOST pointer: LOCAL rows, ascending and unique
 *   facets_host   uint8[m, icrec_index_facets(idx)]      HOST pointer: their new values
 * Nothing else changes, the zero padding behind the last row included.  ICREC_EINVAL, changing nothing: an index
 * without facets, a row outside [0, n_rows), rows that are not ascending and unique, a NULL argument, m < 0.  A set-up
 * call like icrec_index_write_rowset: it copies, may allocate host memory and synchronise.  A captured graph replayed
 * afterwards follows the new values. */
ICREC_API int icrec_index_write_facets(icrec_index* idx, const int32_t* row_ids_host, const uint8_t* facets_host,
                                       int32_t m);

/* Scratch bytes of icrec_search_faceted (0 for a bad argument); equal to icrec_search_workspace_bytes. */
ICREC_API size_t icrec_search_faceted_workspace_bytes(const icrec_index* idx, int32_t n_queries, int32_t k);

/* icrec_search restricted by facets.
 *   allow_dev    uint32[n_queries, n_facets, ICREC_FACET_MASK_WORDS]  the queries' allow masks in DEVICE memory,
 *                n_facets = icrec_index_facets(idx); or NULL
 * allow_dev == NULL: this IS icrec_search - the same launches, the same bits.  allow_dev != NULL on an index without
 * facets: ICREC_EINVAL.  Otherwise the argument checks, the stream semantics and the graph-capturability are
 * icrec_search's: nothing is allocated, nothing synchronises.  The masks are read from device memory when the kernels
 * run: a captured graph replayed after the caller rewrote the mask buffer follows the new masks. */
ICREC_API int icrec_search_faceted(icrec_index* idx, const float* q_dev, int32_t n_queries, int32_t k,
                         const int32_t* excl_idx_dev, const int32_t* excl_off_dev,
                         const uint32_t* allow_dev,
                         int64_t* out_idx_dev, float* out_score_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* Row sets: restrict each query to named sets of rows ("only products sold at this store", "in stock", "vegan").
 * Unlike a facet, which gives a row exactly one value, a row may belong to any number of sets.  An index may carry
 * n_sets in [1, ICREC_MAX_ROWSETS] row sets, each a bitmap over its LOCAL rows; a query names up to
 * ICREC_MAX_SETS_PER_QUERY of them by id, in slots:
 *   - a slot with id < 0 constrains nothing;
 *   - a slot with id in [0, n_sets) requires the row's bit in that set;
 *   - a slot with id >= n_sets admits no row (such an id is never used as an index: the ids live in device memory,
 *     where the host cannot refuse them, and the rule is memory-safe for every int32);
 *   - the same id in two slots counts once.
 * A row is admissible for a query iff every slot admits it, the facet masks admit it (when allow_dev is given) and it
 * is not in the query's exclusion segment.
 * The result of icrec_search_in_sets is bit-identical, indices and scores, to icrec_search with exclusion lists equal
 * to the given exclusions united with every inadmissible row, for every row storage, every k and every batch size.  A
 * query with no admissible row gets (-1, 0.0) pads; a query whose slots are all < 0 gets icrec_search_faceted's bits. */
#define ICREC_MAX_ROWSETS 65535
#define ICREC_MAX_SETS_PER_QUERY 4

/* Set, replace or (bits_host == NULL) remove the index's row sets.
 *   bits_host  uint32[n_sets][W], W = ceil(n_rows / 32)  HOST pointer; bit (r & 31) of word (r >> 5) of set s says
 *              that local row r is in s.  Bits at or past n_rows in the last word are ignored (the library clears
 *              them).  Copied to the device before the call returns.
 * n_sets outside [1, ICREC_MAX_ROWSETS] (with a non-NULL bits_host) is ICREC_EINVAL and changes nothing; a failed
 * allocation is ICREC_ENOMEM and changes nothing either.
 * A set-up call like icrec_index_set_facets: it allocates, may synchronise the device, and must never be issued while
 * a call on the index is running.  The rows, their filter planes / fragments and the facets are not touched, and
 * icrec_search, icrec_search_faceted (icrec_search_in_sets without set ids), icrec_search_partial, icrec_rank_all,
 * icrec_scores, icrec_ivf_search and icrec_boost_select ignore the sets. */
ICREC_API int icrec_index_set_rowsets(icrec_index* idx, const uint32_t* bits_host, int32_t n_sets);
/* Replace the W words of one set (an in-stock bitmap that changes through the day); bits_host as one set of
 * icrec_index_set_rowsets.  ICREC_EINVAL for `set` outside [0, n_sets) or an index without sets.  A set-up call under
 * the same contract: it copies and may synchronise.  A captured graph replayed afterwards follows the new set. */
ICREC_API int icrec_index_write_rowset(icrec_index* idx, int32_t set, const uint32_t* bits_host);
/* Row sets of the index: 0 when none are set, -1 for a NULL handle. */
ICREC_API int32_t icrec_index_rowsets(const icrec_index* idx);

/* Scratch bytes of icrec_search_in_sets (0 for a bad argument); equal to icrec_search_workspace_bytes. */
ICREC_API size_t icrec_search_in_sets_workspace_bytes(const icrec_index* idx, int32_t n_queries, int32_t k);

/* icrec_search_faceted restricted to row sets.
 *   set_ids_dev     int32[n_queries][sets_per_query]  the queries' slots in DEVICE memory, or NULL
 *   sets_per_query  in [1, ICREC_MAX_SETS_PER_QUERY] (not looked at when set_ids_dev is NULL)
 * set_ids_dev == NULL: this IS icrec_search_faceted - the same launches, the same bits.  ICREC_EINVAL: set_ids_dev !=
 * NULL on an index without sets, sets_per_query out of range; the other argument checks are icrec_search's.
 * Nothing is allocated and nothing synchronises; the call is graph-capturable.  The ids and the bitmaps are read from
 * device memory when the kernels run: a captured graph replayed after the caller rewrote the id buffer, or after
 * icrec_index_write_rowset rewrote a set, follows the new contents. */
ICREC_API int icrec_search_in_sets(icrec_index* idx, const float* q_dev, int32_t n_queries, int32_t k,
                         const int32_t* excl_idx_dev, const int32_t* excl_off_dev,
                         const uint32_t* allow_dev,
                         const int32_t* set_ids_dev, int32_t sets_per_query,
                         int64_t* out_idx_dev, float* out_score_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* Diversity re-selection of a search result: Maximal Marginal Relevance (Carbonell & Goldstein 1998) over each
 * query's k candidates, entirely on the device.  Scratch bytes (0 for a NULL index, n_queries < 1 or k outside
 * [1, ICREC_MAX_K]): the queries' k x k similarity matrices. */
ICREC_API size_t icrec_mmr_select_workspace_bytes(const icrec_index* idx, int32_t n_queries, int32_t k);

/* Pick top_k of each query's k candidates greedily, trading relevance against similarity to what is already picked.
 *   cand_idx_dev  int64[n_queries, k]      icrec_search's out_idx: global rows, -1 pads
 *   rel_dev       float[n_queries, k]      relevance of each candidate (icrec_search's out_score, or cross-encoder
 *                                          logits); need not be sorted
 *   lambda        in [0, 1]                1: relevance only, 0: after the first pick, dissimilarity only
 *   out_idx_dev   int64[n_queries, top_k]  the picks in selection order; -1 pads
 *   out_rel_dev   float[n_queries, top_k]  the chosen candidates' rel, bits unchanged; 0 at pads
 * The definition, which the result follows bit for bit:
 *   Validity.  Candidate j of a query is valid iff cand >= 0 and cand - row_offset lies in [0, n_rows) of idx.  Invalid
 *     candidates are never selected and their rows are never read.  A row that appears twice in a list is two
 *     candidates.
 *   Similarity.  sim(a, b) is the fp32 chain s = 0; for j = 0 .. dim-1: s = fmaf(pa[j], pb[j], s) over the index's
 *     STORED normalised rows (bf16 storage widened exactly; the rows are not normalised again): icrec_scores'
 *     arithmetic with a stored row on the query side.  sim(a, b) and sim(b, a) have the same bits.  The filter planes
 *     and fragments are not used.
 *   Order.  x is ordered before y iff x is a number and y a NaN, else iff x > y (compared as floats, -0 == +0), else
 *     (equal, or both NaN) iff x's position j is lower: icrec_rerank_select's rule.
 *   First pick: the valid candidate whose rel is ordered first.
 *   Later picks: among the valid candidates not yet selected, the one whose
 *         v(c) = (lambda * rel[c]) - (oml * maxsim[c])
 *     is ordered first, where maxsim[c] is the greatest sim(s, c) over the selected s and oml is the float
 *     1.0f - lambda computed on the host.  v takes three fp32 roundings - the two products, then the difference -
 *     and no fused multiply-add.
 *   Termination: after top_k picks, or when no valid candidate is left; the remaining outputs are -1 / 0.0f.
 * lambda = 1 gives the valid candidates in the order of their rel: on an icrec_search result, its first top_k entries.
 * A query's result has the same bits alone and inside any batch, for every row storage.
 * ICREC_EINVAL: a NULL pointer, n_queries < 1, k outside [1, ICREC_MAX_K], top_k outside [1, k], lambda NaN or outside
 * [0, 1].  ICREC_ENOMEM: workspace_bytes < icrec_mmr_select_workspace_bytes.  Nothing is launched on an error.
 * The outputs must not alias the inputs.  Asynchronous on `stream`: nothing is allocated, nothing synchronises, every
 * launch goes to that one stream, and the call can be captured into a hipGraph.  Facets and exclusion lists compose
 * with it through the search whose result it consumes. */
ICREC_API int icrec_mmr_select(icrec_index* idx, const int64_t* cand_idx_dev, const float* rel_dev,
                     int32_t n_queries, int32_t k, int32_t top_k, float lambda,
                     int64_t* out_idx_dev, float* out_rel_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* Boosting each query's listed rows on a search result ("buy it again"): rank the union of a query's candidates and a
 * list of rows the caller names - the products a user has bought before - with a per-row weight added to the listed
 * rows' cosine scores, entirely on the device. */
#define ICREC_MAX_BOOSTS 1024   /* listed rows per query */

/* Scratch bytes of icrec_boost_select (0 for a NULL index, n_queries < 1 or max_boosts outside [0, ICREC_MAX_BOOSTS]):
 * the normalised queries and one 64-bit word per query and listed entry. */
ICREC_API size_t icrec_boost_select_workspace_bytes(const icrec_index* idx, int32_t n_queries, int32_t max_boosts);

/* The best top_k of each query's listed rows and candidates under the adjusted score a(r) = cos(r) + w(r).
 *   q_dev           float[n_queries, dim]     the queries icrec_search takes (not normalised)
 *   cand_idx_dev    int64[n_queries, k]       icrec_search's out_idx: global rows, -1 pads; or NULL (with cand_score_dev):
 *   cand_score_dev  float[n_queries, k]       icrec_search's out_score                     no candidates
 *   boost_off_dev   int32[n_queries+1]        CSR offsets into boost_rows_dev / boost_w_dev
 *   boost_rows_dev  int32[...]                each query's listed LOCAL rows, ascending and unique within its segment
 *                                             (the format of icrec_search's exclusion lists)
 *   boost_w_dev     float[...]                their weights; NULL: every weight is 0
 *   max_boosts      in [0, ICREC_MAX_BOOSTS]  only the first max_boosts entries of a segment are read
 *   excl_idx_dev / excl_off_dev, allow_dev    the exclusion lists and facet masks of icrec_search_faceted, or NULL
 *   out_idx_dev     int64[n_queries, top_k]   row_offset + row, best first; -1 pads
 *   out_score_dev   float[n_queries, top_k]   the adjusted scores; 0 at pads
 * The definition, which the result follows bit for bit:
 *   Lists.  Query i's list is entries [boost_off[i], boost_off[i+1]) of boost_rows_dev, of which the first max_boosts
 *     are read; a segment whose end lies before its start is empty.  A list that is not ascending and unique gives an
 *     unspecified result, but a memory-safe one.
 *   Validity of a listed entry.  0 <= row < n_rows, the row is not in the query's exclusion segment, and with allow_dev
 *     the query's facet masks admit it: icrec_search_faceted's rules.  An invalid entry is never returned and its row is
 *     never read.
 *   Effective weight.  w_eff = w if w >= 0 (+inf included), else 0: a NaN or a negative weight counts as 0 (the weights
 *     live on the device, where the host cannot refuse them; a(r) >= cos(r) then holds for every input).
 *   Cosine.  The query is normalised as icrec_search normalises it; cos is the fp32 chain s = 0; for j = 0 .. dim-1:
 *     s = fmaf(q_hat[j], p[j], s) over the index's STORED row (bf16 storage widened exactly): icrec_scores' bits.  The
 *     filter planes and fragments are not used.
 *   Adjusted score.  a = cos, bits unchanged, when w_eff == 0; otherwise a = cos + w_eff, one fp32 addition.
 *   Candidates.  Candidate j is valid iff cand >= 0 and cand - row_offset lies in [0, n_rows) of idx.  Its score is
 *     cand_score[j] as given; it is not computed again.  A candidate whose row is among the entries read from the
 *     query's list (valid or not) is dropped: the listed entry stands for it.
 *   Result.  The best top_k of {valid listed entries} and {remaining valid candidates}, ordered as icrec_search orders:
 *     score descending compared as floats (-0 == +0), lower row first on ties; then -1 / 0.0f pads.
 * Consequences.  With w_eff >= 0 an unlisted row among the best top_k of the whole catalog under a has fewer than
 * top_k rows before it under plain cosine as well.  So if the candidates are icrec_search(_faceted)'s result for the same
 * q, exclusions, masks and k >= top_k, the result is the top_k of the WHOLE catalog under a.  If all weights are 0 (or
 * boost_w_dev is NULL) it is that search's first top_k entries, bit for bit.  Without candidates only the listed rows
 * are ranked.  A query's result has the same bits alone and inside any batch, for every row storage.
 * ICREC_EINVAL, before any HIP call: a NULL among idx, q_dev, boost_off_dev, the outputs, the workspace; boost_rows_dev
 * NULL with max_boosts > 0; cand_idx_dev and cand_score_dev (excl_idx_dev and excl_off_dev) not both set or both NULL;
 * n_queries < 1; k outside [1, ICREC_MAX_K] when there are candidates; top_k outside [1, ICREC_MAX_K], or top_k > k
 * with candidates; max_boosts outside [0, ICREC_MAX_BOOSTS]; neither candidates nor max_boosts > 0; allow_dev on an index
 * without facets.  ICREC_ENOMEM: workspace_bytes < icrec_boost_select_workspace_bytes.  Nothing is launched on an error.
 * The outputs must not alias the inputs.  Asynchronous on `stream`: nothing is allocated, nothing synchronises, every
 * launch goes to that one stream, and the call can be captured into a hipGraph.  The lists, weights and masks are read
 * from device memory when the kernels run: a replayed graph follows what the buffers hold then. */
ICREC_API int icrec_boost_select(icrec_index* idx, const float* q_dev, int32_t n_queries,
                       const int64_t* cand_idx_dev, const float* cand_score_dev, int32_t k,
                       const int32_t* boost_off_dev, const int32_t* boost_rows_dev, const float* boost_w_dev,
                       int32_t max_boosts,
                       const int32_t* excl_idx_dev, const int32_t* excl_off_dev, const uint32_t* allow_dev,
                       int32_t top_k, int64_t* out_idx_dev, float* out_score_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* Queries composed from stored rows: "similar items" (the query IS a row of the index), "more like these, less like
 * those" (Rocchio feedback: the text's vector moved toward accepted products and away from dismissed ones), a profile
 * from a basket (the weighted sum of its rows, no text at all) - built on the device from the rows the index holds,
 * between icrec_encode and the search.  Only the query vector changes, so everything the searches do composes with it. */
#define ICREC_MAX_TERMS 1024   /* terms read per query */

/* q'[i] = a[i] * q_hat[i] + the sum over query i's terms of w * row, in list order.
 *   base_dev       float[n_queries, dim]     the text part (icrec_encode's output; not normalised), or NULL: none
 *   base_w_dev     float[n_queries]          a, the weight of the text part; NULL: every a = 1
 *   term_off_dev   int32[n_queries+1]        CSR offsets into term_rows_dev / term_w_dev
 *   term_rows_dev  int32[...]                each query's LOCAL rows, in the order given: NOT sorted, the order defines
 *                                            the sum
 *   term_w_dev     float[...]                their weights, of either sign; NULL: every w = 1
 *   max_terms      in [0, ICREC_MAX_TERMS]   only the first max_terms entries of a segment are read
 *   out_dev        float[n_queries, dim]     q'; NOT normalised (icrec_search and its siblings normalise their queries)
 * There is no workspace.  base_dev and out_dev are 16-byte aligned (rows of dim floats are, from an aligned start).
 * The definition, which the result follows bit for bit:
 *   Base.  With base_dev, q_hat is the row normalised as icrec_search normalises a query (normalize_rows_kernel): 64
 *     partial sums s_l = fmaf(x[i], x[i], s_l) over i = l, l + 64, .. ascending, added by the xor butterfly 32 .. 1,
 *     den = max(sqrt(sum), 1e-12), q_hat[j] = x[j] / den.  Then acc[j] = a * q_hat[j], one fp32 multiplication; an a
 *     that is not finite counts as 0.  Without base_dev, acc[j] = +0.
 *   Terms read.  Query i's segment is entries [term_off[i], term_off[i+1]) of term_rows_dev, of which the first
 *     max_terms are read; a segment whose end lies before its start is empty.  The offsets must lie inside the arrays.
 *   Valid term.  0 <= row < n_rows and w is finite.  An invalid term contributes nothing and its row is never read (the
 *     lists live on the device, where the host cannot refuse them): the call is memory-safe for any rows and weights.
 *     A row listed twice is two terms.
 *   Sum.  The valid terms in list order: acc[j] = acc[j] + (w * p[j]), two fp32 roundings - the product, then the sum -
 *     and no fused multiply-add.  p is the index's STORED normalised row (bf16 storage widened exactly).  The filter
 *     planes and fragments are not used.
 *   Result.  out[i][j] = acc[j].
 * A query's result has the same bits alone and inside any batch; the storages F32 and F32_FILTER give the same bits,
 * and so do BF16 and BF16_FILTER.  One term of weight 1 without a base gives the stored row.  A zero result is a legal
 * query: the search scores every row 0 and returns the lowest rows.
 * ICREC_EINVAL, before any HIP call: a NULL among idx, term_off_dev, out_dev; term_rows_dev NULL with max_terms > 0;
 * n_queries < 1; max_terms outside [0, ICREC_MAX_TERMS]; base_dev NULL together with max_terms == 0; base_w_dev set
 * without base_dev.  Nothing is launched on an error.
 * out_dev must not alias base_dev.  Asynchronous on `stream`: nothing is allocated, nothing synchronises, it is ONE
 * launch, and the call can be captured into a hipGraph.  The lists and weights are read from device memory when the
 * kernel runs: a replayed graph follows what the buffers hold then. */
ICREC_API int icrec_compose_queries(icrec_index* idx, const float* base_dev, const float* base_w_dev, int32_t n_queries,
                          const int32_t* term_off_dev, const int32_t* term_rows_dev, const float* term_w_dev,
                          int32_t max_terms, float* out_dev, void* stream);

/* A query adapter learned from (context, product) pairs: the encoder and the stored rows stay frozen, a linear map on
 * the query side is trained with the reference's loss (src/training/train_sbert.py: MultipleNegativesRankingLoss,
 * scale 30) against the rows the index already holds.  Only the query vector changes - q' = q + D q, applied between
 * icrec_encode and icrec_compose_queries / the search - so no product is re-encoded, the index keeps its bits and every
 * search composes with it.
 * An adapter of width d owns D (fp32, d x d, row-major, zero when created), a transposed copy of D for the apply
 * kernel, AdamW's moments m and v, and the step count t.  d is a multiple of 32 in [32, ICREC_ADAPTER_MAX_DIM].  The
 * arrays are never moved after create: a captured graph that holds an icrec_adapter_apply stays valid across training,
 * as one that holds a search does across icrec_index_write_rows, and follows what the arrays hold when it replays.
 *
 * Apply, bit-exact and independent of the batch.  For a query q and each output r:
 *     acc = +0;  for c = 0 .. d-1 in order:  acc = acc + (D[r][c] * q[c]);   q'[r] = q[r] + acc
 *   every product and every sum one fp32 rounding (two per term, as in icrec_compose_queries): no fused multiply-add,
 *   no MFMA.  D = 0 gives q' == q value for value.  q' is not normalised: every search normalises its queries.
 *
 * Loss, over B anchors a_i (fp32 [B, d]) and C >= B candidate rows cand[0 .. C): candidate i is anchor i's positive, the
 * rest are extra negatives; v_j is the STORED row cand[j] (fp32, or bf16 widened exactly).
 *     z_i = apply(a_i),  n_i = max(|z_i|, 1e-12),  u_i = z_i / n_i,  s_ij = scale * (u_i . v_j)
 *     loss = the mean over the counted anchors of (logsumexp_j s_ij - s_ii)
 *   Masked: a candidate outside [0, n_rows), for every anchor; a candidate j != i with cand[j] == cand[i], for anchor i
 *   (a second copy of the anchor's own positive).  An anchor whose own positive is outside the range is not counted and
 *   has no gradient.  No anchor counted: the loss is 0 and the gradient is 0.  A row number that was not checked never
 *   becomes an address: the call is memory-safe for any candidate list.
 * Gradient.  P = softmax_j(s_ij) over the unmasked candidates, G_ij = (P_ij - [i == j]) / counted,
 *     du_i = scale * sum_j G_ij v_j,   dz_i = (du_i - u_i (u_i . du_i)) / n_i,   dD = sum_i dz_i a_i^T
 *   The dot products u . v and the sums over j and i are fp32 fmaf chains (the f32 MFMA) in a fixed order; the row
 *   maximum is subtracted before exp.  There are no floating-point atomics: the same inputs give the same bits.
 * Update (update != 0): torch.optim.AdamW's step t + 1 on D - D = D * (1 - lr * weight_decay),
 *     m = m + (g - m) * (1 - beta1),  v = v * beta2 + (1 - beta2) * g * g,
 *     D = D - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   with the bias corrections computed by the host in double - then t = t + 1. */
#define ICREC_ADAPTER_MAX_DIM 1024
#define ICREC_ADAPTER_MAX_BATCH 1024        /* B in [1, ICREC_ADAPTER_MAX_BATCH] */
#define ICREC_ADAPTER_MAX_CANDIDATES 8192   /* C in [B, ICREC_ADAPTER_MAX_CANDIDATES] */
typedef struct icrec_adapter icrec_adapter;

/* ICREC_EINVAL: a NULL out, a dim that is not a multiple of 32 in [32, ICREC_ADAPTER_MAX_DIM].  Set-up calls, like
 * icrec_index_create: create, destroy, set_state and get_state synchronise the device. */
ICREC_API int icrec_adapter_create(int32_t dim, int device, icrec_adapter** out);
ICREC_API int icrec_adapter_destroy(icrec_adapter* adapter);
ICREC_API int32_t icrec_adapter_dim(const icrec_adapter* adapter);
/* delta_host, m_host, v_host: float[dim, dim] in HOST memory; m_host and v_host may be NULL (set_state: zeros;
 * get_state: not wanted, as may delta_host and t_out).  t >= 0 is the number of AdamW steps taken. */
ICREC_API int icrec_adapter_set_state(icrec_adapter* adapter, const float* delta_host, const float* m_host,
                            const float* v_host, int64_t t);
ICREC_API int icrec_adapter_get_state(const icrec_adapter* adapter, float* delta_host, float* m_host, float* v_host,
                            int64_t* t_out);
/* out[i] = apply(q[i]) for n >= 1 queries, float[n, dim] in DEVICE memory, out_dev != q_dev.  ONE launch on `stream`,
 * no workspace, nothing allocated, nothing synchronises: it can be captured into a hipGraph.  ICREC_EINVAL: a NULL
 * pointer, n < 1, out_dev == q_dev. */
ICREC_API int icrec_adapter_apply(const icrec_adapter* adapter, const float* q_dev, int32_t n, float* out_dev, void* stream);
/* The loss and dD of one batch against idx's stored rows and, with update != 0, the AdamW step.
 *   anchors_dev    float[B, dim]      the anchors (icrec_encode's output)
 *   cand_rows_dev  int32[C]           LOCAL rows of idx; candidate i < B is anchor i's positive
 *   loss_out_dev   float[1]           the loss
 *   grad_out_dev   float[dim, dim]    dD, or NULL: not wanted
 * Workspace: icrec_adapter_step_workspace_bytes(adapter, B, C) bytes on the adapter's device (0 for sizes outside the
 * limits).  Three launches on `stream`; nothing is allocated, nothing synchronises.  The step count and the bias
 * corrections are the host's: they are taken when the call is made.
 * ICREC_EINVAL, before any HIP call: a NULL among idx, adapter, anchors_dev, cand_rows_dev, loss_out_dev, the workspace;
 * an index whose dim or device differs from the adapter's, or without rows; B or C outside the limits; a workspace that
 * is too small; a hyper-parameter that is not finite; with update != 0, a beta outside [0, 1) or a negative eps. */
ICREC_API size_t icrec_adapter_step_workspace_bytes(const icrec_adapter* adapter, int32_t B, int32_t C);
ICREC_API int icrec_adapter_step(icrec_index* idx, icrec_adapter* adapter, const float* anchors_dev, int32_t B,
                       const int32_t* cand_rows_dev, int32_t C, float scale, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int32_t update, float* loss_out_dev, float* grad_out_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same step against the WHOLE catalog: every stored row of idx is a candidate, there is no list and no sampling -
 * plain cross-entropy with labels.
 *   pos_rows_dev   int32[B]           LOCAL rows of idx; pos_rows[i] is anchor i's positive
 *   the other arguments as in icrec_adapter_step
 * Loss.  z, n, u as above.  n_rows is idx's row count when the call is made; the rows between n_rows and the capacity
 * (icrec_index_reserve, icrec_index_remove_rows) are never read as candidates.
 *     s_ir = scale * (u_i . v_r) for every local row r in [0, n_rows), v_r the stored row (fp32, or bf16 widened exactly)
 *     loss = the mean over the counted anchors of (logsumexp_r s_ir - s_i,pos_i)
 *   Anchor i is counted iff pos_rows[i] lies in [0, n_rows); a value that failed that check never becomes an address.
 *   An anchor that is not counted has neither a loss nor a gradient; no anchor counted: the loss is 0 and the gradient
 *   is 0 exactly.  Nothing else is masked: two anchors may share a positive, and a row equal to some anchor's positive
 *   is just that row.
 * Gradient.  P = softmax_r(s_ir), G_ir = (P_ir - [r == pos_i]) / counted, du_i = scale * sum_r G_ir v_r; dz, dD and the
 *   AdamW update as in icrec_adapter_step.
 * Order.  The rows are cut into n_splits splits of rows_per_split rows (the last one shorter), every split but the
 *   last a whole number of groups of 128 rows; icrec_adapter_catalog_plan states the cut, which depends on B and
 *   n_rows only, never on the device.  A sum over rows is: a group of 128 rows one fmaf chain from zero, the groups of
 *   a split added in order, the splits added in split order; the (maximum, sum) pairs of the softmax merge in that
 *   same order.  No floating-point atomics: the same inputs give the same bits.
 * Workspace: icrec_adapter_step_catalog_workspace_bytes(adapter, idx, B) bytes for idx's CURRENT row count (0 for a B
 * outside the limits, a NULL handle or an index without rows); every byte the step reads it has written before.  Six
 * launches on `stream`; nothing is allocated, nothing synchronises.
 * ICREC_EINVAL, before any HIP call: a NULL among idx, adapter, anchors_dev, pos_rows_dev, loss_out_dev, the workspace;
 * an index whose dim or device differs from the adapter's, or without rows; B outside [1, ICREC_ADAPTER_MAX_BATCH]; a
 * workspace that is too small; a hyper-parameter that is not finite; with update != 0, a beta outside [0, 1) or a
 * negative eps.  icrec_adapter_catalog_plan: a NULL pointer, B outside the limits, n_rows < 1. */
ICREC_API size_t icrec_adapter_step_catalog_workspace_bytes(const icrec_adapter* adapter, const icrec_index* idx, int32_t B);
ICREC_API int icrec_adapter_step_catalog(icrec_index* idx, icrec_adapter* adapter, const float* anchors_dev, int32_t B,
                               const int32_t* pos_rows_dev, float scale, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int32_t update, float* loss_out_dev, float* grad_out_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream);
ICREC_API int icrec_adapter_catalog_plan(const icrec_adapter* adapter, int32_t B, int64_t n_rows, int32_t* n_splits,
                               int64_t* rows_per_split);
/* The step over per-anchor lists with graded targets: what a deployed recommender records (per request the products
 * shown and what happened to each) and what a teacher gives (per query its candidates with a score each).  Every
 * anchor has its own candidates and non-negative targets instead of one label: the listwise softmax cross-entropy.
 *   list_off_dev    int32[B+1]  CSR offsets
 *   list_rows_dev   int32[...]  LOCAL rows of idx, per anchor, in any order
 *   list_target_dev float[...]  gains >= 0 (or a teacher's probabilities)
 *   max_len         in [1, ICREC_ADAPTER_MAX_LIST]: entries read per segment
 *   the other arguments as in icrec_adapter_step
 * Entries read.  Anchor i's segment is [list_off[i], list_off[i+1]); only its first max_len entries are read.  A
 *   segment whose end lies before its start is empty.  The offsets must lie inside the arrays (icrec_compose_queries'
 *   convention).
 * Live entry.  An entry is live when 0 <= row < n_rows (n_rows as of the call) and its target is finite and >= 0.  An
 *   entry that is not live contributes nothing, to the softmax or to the targets, and its row is never read.  No
 *   unchecked value becomes an address: the call is memory-safe for any device lists.  A row listed twice is two
 *   entries.
 * Counted anchor.  Anchor i is counted iff T_i, the sum of its live targets, is finite and > 0.  An anchor that is not
 *   counted has neither loss nor gradient.  If no anchor is counted, the loss is 0 and the gradient is exactly 0.
 * Loss.  z, n, u as in icrec_adapter_step.  s_e = scale * (u_i . v_row(e)), on the STORED row (bf16 widened exactly);
 *     t_e = target_e / T_i;   loss_i = logsumexp_e s_e - sum_e t_e s_e, over the live entries
 *   The loss is the mean of loss_i over the counted anchors, summed as icrec_adapter_step sums: two levels in double,
 *   rounded once.
 * Gradient.  P = softmax_e(s_e), G_e = (P_e - t_e) / counted, du_i = scale * sum_e G_e v_e; dz, dD and the AdamW update
 *   are exactly icrec_adapter_step's.
 * Order.  u_i . v is, per lane of a wave of 64, an fmaf chain over the row's 16-byte pieces lane, lane + 64, ..
 *   (4 fp32 or 8 bf16 features each, features ascending), then the xor butterfly 32, 16, .., 1 over the lanes.  T_i,
 *   the softmax's sum (fp32, the maximum subtracted before exp) and sum_e t_e s_e (in double; loss_i is rounded to fp32
 *   once) are each a lane's chain over entries lane, lane + 64, .. in list order, then that butterfly.  The sum over e
 *   of du is, per feature, groups of 128 entries - each one fmaf chain from zero in list order - added in group order.
 *   u . du is an fmaf chain over the features of a piece, the butterfly over a wave's 64 pieces, the four waves in
 *   order.  No floating-point atomics: the same inputs give the same bits.
 * Consequences: a list with one live entry has loss exactly 0 and gradient exactly 0; if every anchor's list is one
 *   shared list of distinct in-range rows and the targets are one-hot at position i, the loss is icrec_adapter_step's
 *   on that candidate list.
 * Workspace: icrec_adapter_step_lists_workspace_bytes(adapter, B) bytes (0 outside the limits / NULL).  Four launches
 *   on `stream`; nothing is allocated, nothing synchronises.
 * ICREC_EINVAL, before any HIP call: icrec_adapter_step's conditions, a NULL among the three list arrays, max_len
 *   outside its range. */
#define ICREC_ADAPTER_MAX_LIST 1024      /* entries read per anchor */
ICREC_API size_t icrec_adapter_step_lists_workspace_bytes(const icrec_adapter* adapter, int32_t B);   /* 0 outside the limits / NULL */
ICREC_API int icrec_adapter_step_lists(icrec_index* idx, icrec_adapter* adapter, const float* anchors_dev, int32_t B,
                             const int32_t* list_off_dev   /* int32[B+1]  CSR offsets                                  */,
                             const int32_t* list_rows_dev  /* int32[...]  LOCAL rows of idx, per anchor, in any order   */,
                             const float*   list_target_dev/* float[...]  gains >= 0 (or a teacher's probabilities)     */,
                             int32_t max_len               /* [1, ICREC_ADAPTER_MAX_LIST]: entries read per segment     */,
                             float scale, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t update,
                             float* loss_out_dev, float* grad_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Caps per facet value on a search result ("at most two products of one aisle, at most five of one department"):
 * walk each query's k candidates in their order and keep a candidate only while every capped facet still has room for
 * its value, entirely on the device.  Unlike a facet mask, which admits or forbids a value, a cap counts; unlike
 * icrec_mmr_select it neither looks at similarities nor changes the order of what it keeps.
 *   cand_idx_dev    int64[n_queries, k]       a search's out_idx: global rows, -1 pads
 *   cand_score_dev  float[n_queries, k]       its out_score
 *   caps_dev        int32[n_queries][ICREC_MAX_FACETS]  caps_dev[q * ICREC_MAX_FACETS + f]; a cap <= 0 constrains nothing
 *   n_prior_dev     int32[n_queries]          picks an earlier round left in the out rows, or NULL (none)
 *   allow_dev       uint32[n_queries, n_facets, ICREC_FACET_MASK_WORDS]  the masks the candidates were searched with,
 *                                             or NULL (all ones); only read to make allow_next_dev
 *   top_k           in [1, ICREC_MAX_K]       picks wanted per query, the priors included; it may exceed k
 *   out_idx_dev     int64[n_queries, top_k]   IN/OUT when n_prior_dev is given, otherwise OUT
 *   out_score_dev   float[n_queries, top_k]   likewise
 *   out_state_dev   int32[n_queries][2]       {picks, done}
 *   allow_next_dev  uint32[n_queries, n_facets, ICREC_FACET_MASK_WORDS] or NULL; may equal allow_dev
 * The definition, which the result follows bit for bit:
 *   Validity.  Candidate j is valid iff cand >= 0 and cand - row_offset lies in [0, n_rows) of idx.  A negative entry
 *     is a PAD; any other invalid entry is skipped.  An invalid candidate's facet word is never read.
 *   Values.  v_f(r) is byte f of the index's facet word of local row r (icrec_index_set_facets), for
 *     f < icrec_index_facets(idx).  A cap on a facet the index does not have is ignored.
 *   Prior picks.  p0 = clamp(n_prior[q], 0, top_k), or 0 when n_prior_dev is NULL.  Entries [0, p0) of the query's out
 *     rows are kept as they are, and each valid one of them adds 1 to count[f][v_f] for every facet.
 *   Walk.  Candidates are taken in position order j = 0 .. k-1, until there are top_k picks.  A valid candidate whose
 *     global row equals an earlier pick, prior or of this call, is skipped.  Otherwise it is KEPT iff
 *     count[f][v_f] < cap[f] for every facet f with cap[f] > 0.  A kept candidate is appended - its index, and
 *     cand_score with its bits unchanged - and its counts go up by one.
 *   Result.  The picks first, then -1 / 0.0f pads.  state = {picks, done}; done = 1 iff picks == top_k or any of the k
 *     candidate entries is a pad: a pad means that the search which made the list ran out of admissible rows.
 *   Next masks (allow_next_dev given).  The query's allow_dev words, or all ones when allow_dev is NULL, with bit v of
 *     facet f cleared for every capped facet f and every value v with count[f][v] >= cap[f].
 * A query's result has the same bits alone and inside any batch, for every row storage and row_offset.
 * Consequence: the capped top_k of the WHOLE catalog, in rounds.  Let O be the order in which icrec_search_in_sets
 * (or icrec_boost_select over it) ranks the rows that a query's exclusions, masks and sets admit, and G the greedy
 * capped walk of all of O: the definition above with O as the candidates.  Run a round - search k wide, then
 * icrec_cap_select with the picks so far as priors - and, while done == 0, repeat with the masks allow_next, the
 * exclusions united with the picks, and k >= top_k - picks.  The final picks are G's first top_k, because
 *   - a round walks a prefix of what is left of O: the walk stops early only at top_k picks, and a list without a pad
 *     that is walked to its end is the k best rows the search admits;
 *   - a row the walk rejected has a value whose count reached its cap, and counts only grow: G rejects it as well, and
 *     it can never be kept later;
 *   - so the next search, which leaves out the picks and every row with a saturated value, lists exactly the unwalked
 *     rows that can still be kept (every walked row is a pick or has a saturated value), in O's order, and walking
 *     them with the counts so far continues G where the round before stopped;
 *   - a round that is not done walked k >= 1 rows to the end and kept fewer than top_k - picks <= k of them, so it
 *     rejected one: at least one more (facet, value) is saturated after it.  The rounds are at most the number of
 *     (facet, value) pairs plus one.
 * With boosts the adjusted scores order O; rows that icrec_boost_select lists but the next masks forbid are dropped by
 * its own validity rule.  The sharded search and icrec_ivf_search are not covered by this argument.
 * ICREC_EINVAL, before any HIP call, and nothing is launched: a NULL among idx, the candidates, caps_dev, the outputs or
 * the state; n_queries < 1; k outside [1, ICREC_MAX_K]; top_k outside [1, ICREC_MAX_K]; an index without facets.
 * Asynchronous on `stream`: one launch of one wave per query, no workspace, nothing is allocated, nothing
 * synchronises, and the call can be captured into a hipGraph.  Caps, priors and masks are read from device memory when
 * the kernel runs.  Apart from allow_next_dev == allow_dev the outputs must not alias the inputs. */
ICREC_API int icrec_cap_select(icrec_index* idx,
                     const int64_t* cand_idx_dev, const float* cand_score_dev, int32_t n_queries, int32_t k,
                     const int32_t* caps_dev, const int32_t* n_prior_dev, const uint32_t* allow_dev,
                     int32_t top_k,
                     int64_t* out_idx_dev, float* out_score_dev, int32_t* out_state_dev,
                     uint32_t* allow_next_dev, void* stream);

/* IVF: an inverted-file index over an icrec_index (the base).  The rows are split into n_lists lists around centroids;
 * a query scans only the nprobe lists whose centroids it matches best.  Approximate in WHICH rows it looks at, exact
 * in everything else.  The definition, which every result follows bit for bit:
 *   Centroid index.  centroids float[n_lists, dim] of any norm go into a private ICREC_ROWS_F32 index with row offset
 *     0, normalised as every index normalises its rows.
 *   Assignment.  list(r) = the row returned by icrec_search(centroid index, stored_row(r), k = 1), stored_row(r) being
 *     what icrec_index_export returns for row r (the normalised fp32 row, or the bf16 row widened exactly): the
 *     library's own search with its own query normalisation and tie rule (the lower list wins).
 *   Layout.  perm int32[n_rows] = the local rows sorted by (list, row); list_off int64[n_lists + 1] = the list
 *     boundaries in perm.  The IVF owns a copy of the stored rows in perm order, in the base's row element type; it
 *     never reads the base's filter planes or fragments.  n_rows < 2^31.
 *   Search(q, k, nprobe, exclusions).  probes(q) = the nprobe rows of icrec_search(centroid index, q, k = nprobe),
 *     without exclusions.  The result is the k best rows r among those with list(r) in probes(q) and r not in q's
 *     exclusion list; each score is s = fmaf(q_hat[j], stored_row(r)[j], s) for j = 0 .. dim-1 with q_hat the query
 *     normalised as icrec_search normalises it: the bits icrec_search gives that row.  Order: score descending (-0
 *     counts as +0), lower ORIGINAL row first on ties.  Outputs row_offset + r and the score; (-1, 0.0) pads where
 *     fewer than k rows qualify.  The result does not depend on the order of rows inside a list, on how a list is cut
 *     into slices or on how many workgroups run.
 * Consequences.  With nprobe == n_lists the result is icrec_search's on the base, bit for bit, for every query, k and
 * exclusion list.  For a fixed query the probed set at nprobe is a prefix of the probed set at nprobe + 1.
 * Every base storage is accepted (the *_FILTER ones included).  The base index must outlive the IVF, which keeps its
 * row_offset, dim, device and row element type. */
typedef struct icrec_ivf icrec_ivf;

/* Build the IVF.  centroids_dev: float[n_lists, dim] in DEVICE memory.  ICREC_EINVAL: a NULL argument, n_lists < 1 or
 * n_lists > n_rows, a base of 2^31 rows or more.  A set-up call like icrec_index_set_facets: it allocates (the
 * gathered rows: as many bytes as the base's rows), synchronises, assigns the rows in passes over slices of them, sorts
 * on the host, and must never be issued while a call on the base index is running.
 * The IVF owns its copy of the rows and their assignment: it does not see icrec_index_write_rows, _append_rows or
 * _remove_rows on the base.  After any of them, destroy it and create it again from the same centroids; until then it
 * answers from the rows (and row numbers) the base had when it was built. */
ICREC_API int icrec_ivf_create(icrec_index* base, const float* centroids_dev, int32_t n_lists, icrec_ivf** out);
ICREC_API int icrec_ivf_destroy(icrec_ivf* ivf);
ICREC_API int32_t icrec_ivf_lists(const icrec_ivf* ivf);                      /* n_lists; -1 for NULL */
/* n_rows = the base's rows when the IVF was built.  perm_dev int32[n_rows] and list_off_dev int64[n_lists + 1] (device memory) <- the layout; asynchronous on `stream`. */
ICREC_API int icrec_ivf_layout(const icrec_ivf* ivf, int32_t* perm_dev, int64_t* list_off_dev, void* stream);
/* Scratch bytes of icrec_ivf_search (0 for a bad argument). */
ICREC_API size_t icrec_ivf_search_workspace_bytes(const icrec_ivf* ivf, int32_t n_queries, int32_t k, int32_t nprobe);
/* The search defined above; q_dev, the exclusion lists (LOCAL original rows, sorted and unique, CSR) and the outputs
 * are icrec_search's.  ICREC_EINVAL, before any launch: a NULL among ivf, q_dev, the outputs; n_queries < 1; k outside
 * [1, ICREC_MAX_K]; nprobe outside [1, min(n_lists, ICREC_MAX_K)]; only one of the two exclusion pointers set.
 * ICREC_ENOMEM: workspace_bytes < icrec_ivf_search_workspace_bytes.  Asynchronous on `stream`: nothing is allocated,
 * nothing synchronises, every launch goes to that one stream, and the call can be captured into a hipGraph. */
ICREC_API int icrec_ivf_search(icrec_ivf* ivf, const float* q_dev, int32_t n_queries, int32_t k, int32_t nprobe,
                     const int32_t* excl_idx_dev, const int32_t* excl_off_dev,
                     int64_t* out_idx_dev, float* out_score_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* Shard-local half of a sharded search: same as icrec_search but emits the
 * sorted partial lists as packed 64-bit keys
 *   key = (orderable(score) << 32) | (0xFFFFFFFF - global_row)
 * so that a larger key is a better hit under (score desc, row asc).
 *   out_keys_dev uint64[n_queries, k], best first; 0 pads.                   */
ICREC_API int icrec_search_partial(icrec_index* idx, const float* q_dev,
                         int32_t n_queries, int32_t k,
                         const int32_t* excl_idx_dev,
                         const int32_t* excl_off_dev,
                         uint64_t* out_keys_dev,
                         void* workspace_dev, size_t workspace_bytes,
                         void* stream);

/* Merge `n_lists` sorted partial lists per query (e.g. the all-gathered
 * per-shard lists, laid out [n_lists, n_queries, k] as an all-gather leaves
 * them) into the final top-k.  Needs no index handle.                        */
ICREC_API int icrec_merge_topk(const uint64_t* keys_dev, int32_t n_lists,
                     int32_t n_queries, int32_t k,
                     int64_t* out_idx_dev, float* out_score_dev,
                     int device, void* stream);

/* Complete ranking of the catalog for each query: what `scores.argsort(descending=True)` returns in the reference's
 * offline evaluation consumers (src/baselines/content_based.py:58-63, scripts/compare_untrained_vs_trained.py:74-85).
 *   out_rows_dev int64[n_queries, n_rows]  row_offset + row, best first: score descending, lower row first on ties
 * (torch.argsort is unstable on ties; this is the library's total order, the same as icrec_search's).  The exact
 * score rows are materialised in the workspace (n_queries * n_rows * 12..20 bytes): callers stream queries in
 * passes (256 queries over 49,688 rows = 0.2 GB).  Not on the serving path.                                       */
ICREC_API size_t icrec_rank_all_workspace_bytes(const icrec_index* idx, int32_t n_queries);
ICREC_API int icrec_rank_all(icrec_index* idx, const float* q_dev, int32_t n_queries, int64_t* out_rows_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* Full score row(s) for parity checks: out[n_queries, n_rows] = q_hat . p_hat.
 * Not on the serving path (the serving kernels never materialise scores).    */
ICREC_API int icrec_scores(icrec_index* idx, const float* q_dev, int32_t n_queries,
                 float* out_dev, void* workspace_dev, size_t workspace_bytes,
                 void* stream);

/* L2-normalise rows in place-compatible fashion: out = x / max(|x|_2, eps).
 * (torch.nn.functional.normalize(p=2, dim=1) as used by cos_sim.)            */
ICREC_API int icrec_normalize_rows(const float* x_dev, float* out_dev, int64_t n_rows,
                         int32_t dim, float eps, int device, void* stream);

/* ------------------------------------------------------------------------- */
/* Item-item co-occurrence collaborative filtering: replaces the reference's  */
/* ItemItemCFBaseline (src/baselines/collaborative_filtering.py:104-163): its  */
/* co-occurrence dict and the |corpus| x |history| lookups of rank_all.        */
/*   score(q, p) = sum over h in history(q) of cooc(p, h)                      */
/*               = sum over the orders o that hold p of |basket_o ∩ history(q)| */
/* so two sparse passes over the order x item incidence matrix rank a whole    */
/* tile of queries and no co-occurrence table exists (csrc/cf.hip).            */
/* ------------------------------------------------------------------------- */

/* Items are numbered 0 .. n_items-1.  The first n_candidates are the corpus rows, the only items that are ranked; the
 * rest occur in baskets and histories only (the reference keeps them as history and never ranks them).
 *   order_off   int64[n_orders+1]  HOST CSR offsets of the baskets (order_off[0] == 0, non-decreasing)
 *   order_items int32[order_off[n_orders]]  HOST item ids; an item may repeat inside a basket
 * On `device` the library builds the de-duplicated baskets (the reference's dict.fromkeys) and their transpose
 * item -> orders (count, prefix sum, fill).  A set-up call: it allocates, copies and synchronises.
 * ICREC_EINVAL, before anything is launched: a NULL pointer, n_orders or n_items outside [1, 2^31), n_candidates outside
 * [1, n_items] or >= 2^32, an item outside [0, n_items), offsets that decrease, 2^31 or more entries, more items than fit
 * the LDS membership words of the narrowest query tile (327,680).  ICREC_EINVAL after the build: a basket of more than
 * 65,535 distinct items, or (longest basket) x (orders of the most frequent item) >= 2^31 - 1, the simple bound under
 * which every score + 1 fits 31 bits.
 * Queries are ranked in tiles of 16, or of 8 or 4 when n_items is above 81,920 / 163,840 (the tile's history
 * membership, one bit per query and item, must fit the 160 KB LDS); ICREC_CF_TILE=16|8|4 in the environment at create
 * narrows the tile (same results). */
ICREC_API int icrec_cf_create(const int64_t* order_off, const int32_t* order_items, int64_t n_orders, int64_t n_items,
                    int64_t n_candidates, int device, icrec_cf** out);
ICREC_API int icrec_cf_destroy(icrec_cf* cf);
ICREC_API int64_t icrec_cf_orders(const icrec_cf* cf);      /* 0 for a NULL handle, like the three below */
ICREC_API int64_t icrec_cf_items(const icrec_cf* cf);
ICREC_API int64_t icrec_cf_candidates(const icrec_cf* cf);
ICREC_API int64_t icrec_cf_nnz(const icrec_cf* cf);         /* basket entries after de-duplication */
ICREC_API int32_t icrec_cf_tile(const icrec_cf* cf);        /* queries per tile: 16, 8 or 4 */

/* Scratch bytes of icrec_cf_rank: n_queries x (n_orders x 2 + next_pow2(n_candidates) x 8) plus the merge lists; 0 for
 * a bad argument.  Callers stream large query sets in passes. */
ICREC_API size_t icrec_cf_rank_workspace_bytes(const icrec_cf* cf, int32_t n_queries, int32_t k);

/* The best k candidates of each query by co-occurrence score.
 *   hist_off_dev   int32[n_queries+1]         CSR offsets into hist_items_dev
 *   hist_items_dev int32[hist_off[n_queries]] each query's history, ascending and unique within its segment (the
 *                                             format of icrec_search's exclusion lists); may be NULL when every
 *                                             history is empty
 *   out_idx_dev    int64[n_queries, k]        candidate rows, best first; -1 pads when fewer than k remain
 *   out_score_dev  int32[n_queries, k]        their scores (0 where idx == -1); exact integers, never a float
 * Candidates that are in the query's history are left out (collaborative_filtering.py:154-155).  A candidate that
 * occurs in no order scores 0 and is still ranked.  Order: score descending, ties by lower row first: the reference's
 * stable sorted(..., key=-score) over corpus order.  A history id outside [0, n_items) is skipped without being
 * dereferenced.  Asynchronous on `stream`, no host synchronisation: hipGraph-capturable like icrec_search.
 * ICREC_EINVAL: a NULL pointer, n_queries outside [1, 65535], k outside [1, ICREC_MAX_K], more than 8,388,608
 * candidates (icrec_cf_rank_all has no such limit).  ICREC_ENOMEM: workspace. */
ICREC_API int icrec_cf_rank(icrec_cf* cf, const int32_t* hist_off_dev, const int32_t* hist_items_dev, int32_t n_queries,
                  int32_t k, int64_t* out_idx_dev, int32_t* out_score_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* The complete order of the candidates for each query (what the reference's rank_all returns):
 *   out_rows_dev int64[n_queries, n_candidates]  best first; the |history ∩ candidates| left-out rows are -1 pads at
 *                                                the tail
 * Same order, history format and stream semantics as icrec_cf_rank. */
ICREC_API size_t icrec_cf_rank_all_workspace_bytes(const icrec_cf* cf, int32_t n_queries);
ICREC_API int icrec_cf_rank_all(icrec_cf* cf, const int32_t* hist_off_dev, const int32_t* hist_items_dev, int32_t n_queries,
                      int64_t* out_rows_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* IR metrics: replaces compute_ir_metrics (src/baselines/metrics.py:122-176)  */
/* over ranked rows that are already on the device (icrec_search's out_idx,    */
/* icrec_cf_rank's out_idx).  Needs no handle.                                 */
/* ------------------------------------------------------------------------- */

/* Per query, in this order: accuracy@1, @3, @5, @10, recall@10, reciprocal rank@10, NDCG@10, average precision@100.
 *   ranked_rows_dev   int64[n_queries, depth]  best first; the first negative row ends a query's list
 *   depth             in [1, ICREC_MAX_K]
 *   rel_off_dev       int64[n_queries+1]       CSR offsets of the relevant rows
 *   rel_rows_dev      int64[rel_off[n_queries]] each query's relevant rows, ascending and unique
 *   out_sums_dev      double[9]                the eight values summed over the queries that count, then their number;
 *                                              the caller divides.  A query with no relevant row does not count.
 *   out_per_query_dev double[n_queries, 8] or NULL  the values of every query (zeros where it does not count)
 * The definitions are the reference's, two quirks included: NDCG@10 divides by the DCG of the top-10's OWN hits moved
 * to the front (not an ideal built from |relevant|; 0 without a hit), and AP@100 sums hits_so_far / j over the hits in
 * the first min(100, valid entries) and divides by min(|relevant|, that many entries).  Everything is double, added in
 * rank order as the reference's loops do; the ten discounts 1 / log2(i + 2) are computed on the host and passed to the
 * kernel.  The sum over queries is one fixed tree without atomics: the same bits on every run.
 * ICREC_EINVAL: a NULL pointer (rel_rows_dev, out_per_query_dev excepted), n_queries < 1, depth out of range.
 * ICREC_ENOMEM: workspace (icrec_ir_metrics_workspace_bytes).  Asynchronous on `stream`, capturable. */
ICREC_API size_t icrec_ir_metrics_workspace_bytes(int32_t n_queries);
ICREC_API int icrec_ir_metrics(const int64_t* ranked_rows_dev, int32_t depth, const int64_t* rel_off_dev,
                     const int64_t* rel_rows_dev, int32_t n_queries, double* out_sums_dev, double* out_per_query_dev,
                     void* workspace_dev, size_t workspace_bytes, int device, void* stream);

/* ------------------------------------------------------------------------- */
/* Rank fusion: two ranked lists of the same ids (icrec_search's out_idx and   */
/* icrec_cf_rank's out_idx over the same corpus rows) merged into one by       */
/* POSITION: a cosine and an integer co-occurrence count share no scale, so    */
/* each list contributes a weight per position (reciprocal rank fusion and its */
/* weighted relatives) and the sums are ranked.  Needs no handle.              */
/* ------------------------------------------------------------------------- */

/*   a_idx_dev     int64[n_queries, ka]       list A: ids, best first, negative = pad
 *   b_idx_dev     int64[n_queries, kb]       list B, likewise; ka, kb in [1, ICREC_MAX_K], they need not be equal
 *   a_gate_dev    int32[n_queries, ka] or NULL, b_gate_dev int32[n_queries, kb] or NULL: an entry counts only where its
 *                                            gate is > 0.  The gate is icrec_cf_rank's out_score: a candidate that
 *                                            co-occurs with nothing in the history is not a recommendation, and an
 *                                            empty history must not vote for corpus rows 0 .. k-1.
 *   a_w_dev       float[ka], b_w_dev float[kb]  the weight of each position, one table per list, shared by all queries;
 *                                            device memory, so no value can be refused by the host
 *   n_ids         in [1, 2^32 - 1]           ids lie in [0, n_ids)
 *   excl_idx_dev / excl_off_dev              icrec_search's exclusion CSR (ascending and unique per segment), or both NULL
 *   top_k         in [1, ICREC_MAX_K]        it may exceed the number of distinct live ids
 *   out_idx_dev   int64[n_queries, top_k]    out_score_dev float[n_queries, top_k]
 *   out_pos_dev   int32[n_queries, top_k, 2] or NULL: the positions in A and in B that produced each result, -1 where
 *                                            the id is not live in that list
 * The definition, which the result follows bit for bit:
 *   Live entry.  Entry j of list L is live iff 0 <= id < n_ids, and its gate is NULL or > 0, and id is not in the query's
 *     exclusion segment (an id above 2^31 - 1 cannot be excluded), and no position j' < j of the same list holds the same
 *     id and passes the three tests before (the first passing occurrence wins: a gated-off first occurrence does not
 *     hide a gated-on second one).  Nothing is read through a dead id.
 *   Effective weight.  e_L(j) = w_L[j] if w_L[j] > 0 (+inf included), else +0.0f: a NaN, a negative value and -0 count
 *     as +0.
 *   Fused score.  f(id) = eA + eB, one fp32 addition; eL is the effective weight of the id's live entry in L, or +0.0f
 *     when it has none.  f is never NaN and never -0.
 *   Result.  The ids with a live entry in A or in B, ordered by f descending compared as floats, lower id first on ties
 *     (the order of icrec_search_partial's keys).  The first top_k are written, then -1 / 0.0f / {-1, -1} pads.
 * Consequences.  Swapping the roles of A and B gives the same out_idx / out_score bits (fp32 addition commutes), with
 * the out_pos columns swapped.  With B entirely dead and a_w strictly decreasing and positive, the result is A's live
 * entries in A's order (f = a_w[j] + 0 = a_w[j]).  A query has the same bits alone and inside any batch.
 * ICREC_EINVAL, before any HIP call, and nothing is launched: a NULL among the lists, the tables, out_idx_dev,
 * out_score_dev; excl_idx_dev and excl_off_dev not both set or both NULL; n_queries < 1; ka, kb or top_k outside
 * [1, ICREC_MAX_K]; n_ids outside [1, 2^32 - 1] (a key holds a 32-bit id).
 * Asynchronous on `stream`: one launch of one workgroup per query, no workspace, nothing is allocated, nothing
 * synchronises, and the call can be captured into a hipGraph.  Gates, tables and exclusions are read from device memory
 * when the kernel runs.  The outputs must not alias the inputs. */
ICREC_API int icrec_fuse_select(
    const int64_t* a_idx_dev, const int32_t* a_gate_dev, int32_t ka, const float* a_w_dev,
    const int64_t* b_idx_dev, const int32_t* b_gate_dev, int32_t kb, const float* b_w_dev,
    int32_t n_queries, int64_t n_ids,
    const int32_t* excl_idx_dev, const int32_t* excl_off_dev,
    int32_t top_k, int64_t* out_idx_dev, float* out_score_dev, int32_t* out_pos_dev,
    int device, void* stream);

/* ------------------------------------------------------------------------- */
/* Multi-GPU exchange (new design, the reference has none:      */
/* serve_recommendations.py:172-181 only picks a device).  One process per    */
/* GPU; the catalog is row-sharded (each rank's icrec_index carries its       */
/* row_offset), queries are data-parallel.  The collectives are RCCL          */
/* all-gathers over xGMI, issued on the caller's stream from inside the       */
/* library (librccl.so.1 is bound with dlopen on first use).                  */
/* ------------------------------------------------------------------------- */
typedef struct icrec_comm icrec_comm;
#define ICREC_COMM_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */

/* Rank 0 creates the rendezvous id (ncclGetUniqueId) into id_out[ICREC_COMM_ID_BYTES] (host memory) and
 * hands the bytes to every other rank by any out-of-band channel (file, socket, MPI, torch store). */
ICREC_API int icrec_comm_unique_id(void* id_out);
/* Collective over all `world` ranks: ncclCommInitRank on `device`.  world == 1 with unique_id == NULL makes a
 * communicator that exchanges nothing (icrec_search_sharded then equals icrec_search). */
ICREC_API int icrec_comm_init(const void* unique_id, int rank, int world, int device, icrec_comm** out);
ICREC_API int icrec_comm_destroy(icrec_comm* comm);
ICREC_API int32_t icrec_comm_rank(const icrec_comm* comm);
ICREC_API int32_t icrec_comm_world(const icrec_comm* comm);

ICREC_API size_t icrec_search_sharded_workspace_bytes(const icrec_index* idx, const icrec_comm* comm,
                                            int32_t n_local_queries, int32_t k);
/* Collective sharded top-k: every rank passes ITS n_local query embeddings (the same n_local on every rank)
 * and gets the global result for all Q = world * n_local queries, in rank-major order:
 *     ncclAllGather(q_local) -> icrec_search_partial over this rank's shard ->
 *     ncclAllGather(partial keys) -> icrec_merge_topk
 *   q_local_dev   float[n_local, dim]
 *   excl_idx_dev / excl_off_dev  CSR of LOCAL row numbers (this shard's rows) to skip for each of the Q
 *                                gathered queries (int32[Q+1] offsets), or NULL
 *   out_idx_dev   int64[Q, k] GLOBAL rows (row_offset + local row), -1 pads;  out_score_dev float[Q, k]
 * The result is bit-identical on every rank and to icrec_search over the unsharded catalog: the union of the
 * per-shard top-k lists contains the global top-k and the (score desc, row asc) order is total. */
ICREC_API int icrec_search_sharded(icrec_index* idx, icrec_comm* comm, const float* q_local_dev,
                         int32_t n_local_queries, int32_t k,
                         const int32_t* excl_idx_dev, const int32_t* excl_off_dev,
                         int64_t* out_idx_dev, float* out_score_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same collective with PER-RANK exclusion lists: the reference takes `exclude_product_ids` per request
 * (serve_recommendations.py:216-225), and with data-parallel front-ends only the rank that received a request
 * knows its list.  Every rank passes the exclusions of ITS n_local queries as GLOBAL row numbers; the library
 * all-gathers them (offsets, then the ids padded to excl_cap) and each rank applies the ones inside its shard:
 *     ncclAllGather(excl_off) + ncclAllGather(excl_rows)  -> shard-local CSR for the Q gathered queries (3 tiny kernels)
 *     then as icrec_search_sharded
 *   excl_rows_dev  int32[excl_cap]  GLOBAL rows, the CSR values of this rank's n_local queries: each query's rows
 *                                   ascending and unique; entries past excl_off[n_local] are ignored
 *   excl_off_dev   int32[n_local+1] offsets into excl_rows_dev (excl_off[n_local] <= excl_cap)
 *   excl_cap       the padded length of every rank's id buffer: the SAME on every rank (a deployment constant, e.g.
 *                  n_local x the API's per-request limit); 8 * world * excl_cap bytes of workspace
 * Offsets are sanitised on the device after the exchange (they arrive from other ranks): clamped to [0, excl_cap] and
 * made non-decreasing by a running maximum, so a rank's segments are disjoint and hold at most excl_cap ids (a malformed
 * list excludes less, never reads or writes out of bounds).
 * Row numbers travel as int32: catalogs of up to 2^31 - 1 rows for THIS exchange (the searches themselves take
 * row offsets to 4 * 10^9; the reference's catalog has 49,688 rows, BASELINE configs[4] 10^7). */
ICREC_API size_t icrec_search_sharded_excl_workspace_bytes(const icrec_index* idx, const icrec_comm* comm,
                                                 int32_t n_local_queries, int32_t k, int32_t excl_cap);
ICREC_API int icrec_search_sharded_excl(icrec_index* idx, icrec_comm* comm, const float* q_local_dev,
                              int32_t n_local_queries, int32_t k,
                              const int32_t* excl_rows_dev, const int32_t* excl_off_dev, int32_t excl_cap,
                              int64_t* out_idx_dev, float* out_score_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream);

/* The device-side step of that exchange on its own, for callers that move the lists with a transport of their own
 * (torch.distributed, MPI) and for testing the gathered layout without a second GPU: the rank-major buffers exactly
 * as ncclAllGather lays them down -> the CSR of LOCAL rows icrec_search / icrec_search_partial take for the shard
 * [row_lo, row_hi).
 *   off_all_dev   int32[world][n_local+1]   per rank: offsets of its n_local queries into its id buffer (not modified;
 *                                           sanitised in a workspace copy as described above)
 *   rows_all_dev  int32[world][excl_cap]    per rank: GLOBAL rows, each query's ascending and unique
 *   csr_off_dev   int32[world*n_local + 1]  out: offsets for the gathered queries (rank-major)
 *   csr_idx_dev   int32[world*excl_cap]     out: rows - row_lo of the ids inside the shard, order kept
 * Workspace: icrec_exclusions_to_shard_csr_workspace_bytes(world, n_local) bytes on `device`. */
ICREC_API size_t icrec_exclusions_to_shard_csr_workspace_bytes(int32_t world, int32_t n_local_queries);
ICREC_API int icrec_exclusions_to_shard_csr(const int32_t* off_all_dev, const int32_t* rows_all_dev, int32_t world,
                                  int32_t n_local_queries, int32_t excl_cap, int64_t row_lo, int64_t row_hi,
                                  int32_t* csr_off_dev, int32_t* csr_idx_dev,
                                  void* workspace_dev, size_t workspace_bytes, int device, void* stream);

/* ------------------------------------------------------------------------- */
/* Host tokenizer: the WordPiece stage of SentenceTransformer.encode           */
/* (serve_recommendations.py:213,:246 -> transformers BertTokenizer ->         */
/* tokenizers 0.22.2).  Pure host code; produces icrec_encode's packed input.  */
/* ------------------------------------------------------------------------- */
typedef struct icrec_tokenizer icrec_tokenizer;

/* vocab_path: BERT vocab.txt (one token per line, id = line number).
 * do_lower_case: lower-case + strip accents (all-MiniLM-L6-v2: 1).
 * max_len: [CLS] + tokens + [SEP] is truncated to this many ids (256). */
ICREC_API int icrec_tokenizer_create(const char* vocab_path, int do_lower_case, int max_len,
                           icrec_tokenizer** out);
/* The same tokenizer for a vocabulary whose special tokens carry other names (MPNet: <s> </s> <unk> <pad> <mask>).
 * cls, sep and unk must be in the vocabulary; pad and mask may be NULL or absent from it.  All five are matched
 * verbatim in the raw text, never split.  The sequence template stays `cls tokens sep`. */
ICREC_API int icrec_tokenizer_create_ex(const char* vocab_path, int do_lower_case, int max_len,
                              const char* cls, const char* sep, const char* unk, const char* pad, const char* mask,
                              icrec_tokenizer** out);
ICREC_API int icrec_tokenizer_destroy(icrec_tokenizer* tok);
ICREC_API int32_t icrec_tokenizer_vocab_size(const icrec_tokenizer* tok);

/* Tokenise n UTF-8, NUL-terminated strings on up to n_threads host threads
 * (<= 0: all cores).  out_cu[n+1] receives the prefix sums of the id counts and
 * is always filled; the ids go to out_ids back to back.  Returns ICREC_ENOMEM
 * when `cap` ids do not suffice (size the buffer from out_cu[n] and retry). */
ICREC_API int icrec_tokenize(const icrec_tokenizer* tok, const char* const* texts, int32_t n,
                   int32_t* out_ids, int64_t cap, int32_t* out_cu, int32_t n_threads);

/* ------------------------------------------------------------------------- */
/* Diagnostics                                                                */
/* ------------------------------------------------------------------------- */
ICREC_API const char* icrec_last_error(void);
ICREC_API const char* icrec_version(void);
/* Average duration (ms) of the dominant kernel over the launches recorded
 * since the last reset, measured with hipEvents on the launch stream.
 * which: 0 = search score+select kernel, 1 = encoder FFN-up GEMM,
 *        2 = whole encode() call, 3 = whole search() call,
 *        4 = the guarded exact pass behind a filter pass (ICREC_ROWS_F32_FILTER):
 *            a few microseconds when every query was proven, a full search
 *            when the fallback ran,
 *        5 = icrec_mmr_select's similarity-matrix kernel, 6 = its selection kernel,
 *        7 = icrec_boost_select's scoring kernel, 8 = its selection kernel,
 *        10 = icrec_ivf_search's list scan kernel (9 is a spare of the encoder's),
 *        11 = icrec_cap_select's kernel,
 *        12 = icrec_index_write_rows' kernel. */
ICREC_API int icrec_timing_enable(int on);
ICREC_API int icrec_timing_reset(void);
ICREC_API int icrec_timing_query(int which, double* avg_ms, int64_t* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* ICREC_H */
