/*
 * fusion_hip.h -- C ABI of libfusion_hip.so: the MI355X (gfx950) scoring + fusion engine
 * behind the reference's src/retrievers/hybrid.py (Ranker / Aggregator).
 *
 * The reference has no FFI layer: its boundary is a Python API.  These
 * entry points are what a Python binding for that path needs; fusion_amd/_lib.py is
 * that binding (ctypes), and INTEGRATION.md shows the stub a maintainer of the
 * reference would add.  Citations are file:line in the reference tree.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _h (host);
 *  - the caller owns every buffer; nothing is allocated, freed or synchronised inside
 *    (graph-capturable): temporary storage comes from a caller-supplied workspace whose
 *    size fz_*_workspace_bytes() reports;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *    asynchronous on it and re-entrant across streams;
 *  - return value: FZ_OK (0) or a negative fz_status; no exceptions cross the boundary;
 *  - score planes are row-major [rows][ld] with ld >= n; ld*4 should be a multiple of 16 B
 *    for full-rate vector access (any ld is accepted).
 *
 * Data model: the reference's RankedLists (list[Q] of list[<=N] of {'corpus_id','score'},
 * hybrid.py:66-75,93-106) is held per system as dense planes indexed by corpus POSITION:
 *   score[q][j] fp32; rank[q][j] int32 = 0-based position of doc j in the system's list,
 *   -1 if absent (PLAID-pruned ColBERT lists, hybrid.py:137); order[q][r] = doc at rank r;
 *   len[q] = list length.  `idx` of hybrid.py:249,252 is `rank`.
 */
#ifndef FUSION_HIP_H
#define FUSION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FZ_OK = 0,
    FZ_ERR_ARG = -1,         /* null / negative / inconsistent argument */
    FZ_ERR_UNSUPPORTED = -2, /* shape outside what the kernels are built for (fails loudly, never falls back) */
    FZ_ERR_HIP = -3,         /* a HIP runtime call failed; fz_last_hip_error() has the code */
    FZ_ERR_WORKSPACE = -4    /* workspace NULL or too small */
} fz_status;

/* Aggregator.transform_scores modes (hybrid.py:235-280) */
typedef enum {
    FZ_NORM_NONE = 0,        /* :280 passthrough */
    FZ_NORM_MINMAX = 1,      /* :254-258 */
    FZ_NORM_ZSCORE = 2,      /* :260-264, unbiased std */
    FZ_NORM_ARCTAN = 3,      /* :266-269 */
    FZ_NORM_PERCENTILE = 4,  /* :271-275 */
    FZ_NORM_NCE = 5          /* :276-277 */
} fz_norm;

typedef enum { FZ_RRF = 0 /* hybrid.py:252 */, FZ_BCF = 1 /* hybrid.py:249 */ } fz_rank_method;

const char* fz_strerror(int status);
int fz_last_hip_error(void);
/* ABI version of this header: bump on any signature change */
int fz_abi_version(void);

/* ---- K1: single-vector scoring (DPR / SPLADE), hybrid.py:101-103 ---------------------- */
/* Y[r] = X[r] / max(||X[r]||_2, 1e-12)   (util.cos_sim's normalisation; splade/base.py:195-196) */
int fz_normalize_rows_f32(const float* X, int rows, int d, int ldx, float* Y, int ldy, void* stream);
/* scores[q][j] = <Qn[q], Dn[j]>  fp32-in/fp32-accumulate MFMA GEMM (torch.mm, splade/base.py:197;
 * util.dot_score, sentence_transformers.py:229).  Qn [Q][ldq], Dn [N][ldd], d = contraction. */
int fz_dot_scores_f32(const float* Qn, int ldq, const float* Dn, int ldd, int Q, int N, int d, float* scores, int lds,
                      void* stream);
/* The same GEMM with the streaming top-k's threshold filter as its epilogue: NO score plane is written; a score that beats its
 * query's threshold tau[q] (or is NaN) is appended, with its document id id_base + corpus row, to the query's candidate list
 * (cand_scores / cand_ids [Q][cap], cand_len [Q] int32, as for fz_topk_filter_append_f32) -- in arrival order, i.e. for
 * fz_topk_fold_f32(unordered = 1).  tau_padded: [round_up(Q, 128)] floats, 16-byte aligned, +inf beyond Q.  Per 1.1 M-document shard
 * the scores would otherwise cross HBM twice (4.5 GB written by the GEMM, read by the filter). */
int fz_dot_scores_filter_f32(const float* Qn, int ldq, const float* Dn, int ldd, int Q, int N, int d, int64_t id_base,
                             const float* tau_padded, float* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap,
                             int32_t* overflow, void* stream);
/* (ABI 20, additive) The dispatch plan of the three entries above and of fz_splade_head_max_f32: what their launcher derives from the shape,
 * the epilogue (epi: 0 score plane, 1 filter, 2 SPLADE pooling with Q = T, N = V) and the device's compute-unit count `cus` -- the launcher
 * itself runs this function.  Host only, no HIP call: it answers on a machine without a GPU (tests/score_cases.py proves its coverage of the
 * launcher's branches through it).  out[FZ_DOT_SCORES_PLAN_FIELDS]:
 *    0 slab_rows   rows riding as a 4-row slab in the 64-row tail tiles (Q % 128 in 65 .. 68, score plane only; FZ_GEMM_SLABS=0 turns it off)
 *    1 slab_row0   first of them                     2 rows       rows left to the tiles
 *    3 QB          whole 128-row query blocks (a last block of more than 96 rows -- SPLADE: of any height -- is padded to one)
 *    4 TN          128-column corpus tiles           5 full       ids (incl. XCD padding ids) run as whole 128 x 128 tiles
 *    6 halves      128 x 64 half tiles of the halved last round
 *    7 tail_ids    ids of the last query block's tiles (0: none)      8 tail_row0  its first row      9 tail_rows  its height: 32, 64 or 96
 *   10 cover7      1: the 7-row-block cover (193 .. 224 rows, score plane only, 11 nP + 12 nQ tiles <= cus)
 *   13 grid        workgroups launched               14 ragged    d % 64 != 0      15 slots  resident workgroups, 2 * cus rounded down to 8
 * All zeros for an empty problem (Q == 0 or N == 0).  Negative sizes, d <= 0, epi outside 0 .. 2, cus <= 0 or out == NULL -> FZ_ERR_ARG;
 * d % 4 != 0, cus < 4 or more tile ids than 2^30 - 1 -> FZ_ERR_UNSUPPORTED, as the entries themselves answer. */
#define FZ_DOT_SCORES_PLAN_FIELDS 16
int fz_dot_scores_plan(int Q, int N, int d, int epi, int cus, int32_t* out);

/* (ABI 20, additive) The same GEMM with a top-n selection as its epilogue: out_scores / out_ids [rows][n] = the n best columns of every row
 * of X . C^T by (score desc, id asc), (-inf, -1) padding when n > K -- bit for bit fz_topk_rows_f32(fz_dot_scores_f32(X, C), n), with no
 * [rows][K] plane written or read (the ColBERT centroid probes, the centroid assignment and k-means' nearest-centroid step; K = 65,536 there).
 * X [rows][ldx], C [K][ldc] float32, finite.  The token rows ride on the GEMM's corpus side: a lane then owns one token per MFMA column
 * block with the centroids in its own accumulator registers, carries the token's running list across the whole walk over the centroid
 * blocks and writes it once; the 4 (or, with few rows, 4 x groups) partial lists of a token meet in one small merge.  No float atomics;
 * (score, id) is a total order, so the result does not depend on the grid, on arrival order or on the device.
 * n <= fz_dot_topn_max() (8), d % 4 == 0 and 16-byte aligned rows, else FZ_ERR_UNSUPPORTED; negative sizes, d <= 0, ld < d, n <= 0 or a null
 * pointer where there is work -> FZ_ERR_ARG; rows == 0 -> FZ_OK, nothing touched; workspace below fz_dot_topn_workspace_bytes(rows, K, n)
 * (0 for an empty problem; never shrinks when rows, K or n grow) -> FZ_ERR_WORKSPACE.  All decided before any HIP call. */
int fz_dot_topn_max(void);
size_t fz_dot_topn_workspace_bytes(int rows, int K, int n);
int fz_dot_topn_f32(const float* X, int ldx, const float* C, int ldc, int rows, int K, int d, int n, float* out_scores, int32_t* out_ids,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- K2: ColBERT late interaction, hybrid.py:108-137 (exact MaxSim) ------ */
/* scores[q][j] = sum_{i<Lq} max_{t in doc j} <Qtok[q][i], Dtok[t]>.
 * Qtok [Q][Lq][dim] fp16; Dtok packed ragged [sumL][dim] fp16, doc j owns rows [Doff[j], Doff[j+1]);
 * Doff [N+1] int64 (device), sumL = Doff[N] (known to the host: rows of Dtok); max_doc_len = upper bound of the
 * document lengths (the reference's doc_maxlen = 512, hybrid.py:129; tokens beyond it are ignored; <= 16384).
 * dim must be 128 (run_colbert.sh:26); Lq in {32, 64, 128} (64: hybrid.py:129).  Empty documents score 0.
 * Special values: dot products are IEEE fp32 (+-inf carried through, inf * 0 and inf - inf give NaN); the maximum over a
 * document's tokens is fmaxf, which DROPS a NaN term -- the formula in plain IEEE arithmetic would propagate it -- and a
 * query token whose dot products with every token of a document are NaN contributes the empty maximum, -inf
 * (tests/test_gpu_maxsim_edges.py::test_special_values).  L2-normalised token vectors never get there. */
int fz_maxsim_f16(const void* Qtok, const void* Dtok, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N,
                  int dim, float* scores, int lds, void* stream);
/* The same score over OCP e4m3fn token storage (csrc/maxsim8.hip), one byte per component.
 * fz_quantize_e4m3_f16: dst[i] = e4m3(src[i] * 2^scale_exp) for n float16 values: the product is exact in float32 and rounded to
 * nearest-even (subnormals in steps of 2^-9, -0 keeps its sign); every |y| that rounds above 448, +-inf included, saturates to +-448
 * (0x7e / 0xfe); NaN -> 0x7f with the sign bit kept.  A fixed function of the float16 value: the same bytes on every device and grid.
 * scale_exp outside [-8, 15], n < 0 or a null pointer with n > 0 -> FZ_ERR_ARG; n == 0 -> FZ_OK.
 * fz_maxsim_e4m3: scores[q][j] = 2^-descale_exp * sum_{i<Lq} max_{t in doc j} <Qtok8[q][i], Dtok8[t]> over the DEQUANTISED bytes: each
 * 128-term dot product is accumulated in float32 by one 16x16x128 block-scaled MFMA with both hardware scales at 2^0, the power-of-two
 * descale (normally the sum of the two quantiser exponents) multiplies the finished sum once and is exact.  Everything else -- Doff,
 * sumL, max_doc_len (<= 16384), dim == 128, Lq in {32, 64, 128}, 16-byte aligned pointers, empty documents, the fmaxf definition for
 * NaN dot products (a 0x7f / 0xff byte is NaN), the order of the argument checks and their status codes -- is fz_maxsim_f16's;
 * |descale_exp| > 32 -> FZ_ERR_ARG. */
int fz_quantize_e4m3_f16(const void* src, int64_t n, int scale_exp, void* dst, void* stream);
int fz_maxsim_e4m3(const void* Qtok8, const void* Dtok8, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N,
                   int dim, int descale_exp, float* scores, int lds, void* stream);
/* The corpus-scale form (csrc/rerank.hip): every query against ITS OWN candidate list, no [Q][N] plane.
 * scores[q][r] = the MaxSim above of query q and document cand[q][r] - id_base, for r < k.  cand [Q][ldc] int64 global ids;
 * cand_len [Q] int32 (NULL: k for every row); id_base = global id of this shard's document 0 (any int64).  Qtok, Dtok, Doff, sumL,
 * max_doc_len, dim, Lq and the special-value definition are fz_maxsim_f16's, and so are the BITS: for every slot whose document
 * is in range, scores[q][r] equals fz_maxsim_f16's scores[q][cand[q][r] - id_base] bit for bit on any input (the same MFMA
 * chain, maximum and summation tree), so the all-pairs route and the candidate route of one system are interchangeable.
 * A slot gets -inf when r >= cand_len[q], when its id is negative or when its position falls outside [0, N) -- which is how a shard
 * answers for a document another shard owns: the shards' planes combine by an element-wise maximum.  An empty document scores 0;
 * duplicate ids in a row are scored independently; columns k .. lds-1 of scores are left untouched.
 * Argument checks in fz_maxsim_f16's order: null pointers where a non-empty tensor is needed, ldc < k, lds < k or negative sizes
 * -> FZ_ERR_ARG; dim, Lq, alignment or max_doc_len > 16384 outside what is built -> FZ_ERR_UNSUPPORTED; Q == 0 or k == 0 -> FZ_OK
 * with nothing launched.  No workspace. */
int fz_maxsim_pairs_f16(const void* Qtok, const void* Dtok, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N,
                        int dim, const int64_t* cand, int ldc, const int32_t* cand_len, int k, int64_t id_base, float* scores,
                        int lds, void* stream);
/* The corpus-scale form over e4m3 token storage (csrc/rerank8.hip): fz_maxsim_pairs_f16's slots over fz_maxsim_e4m3's bytes, 128 B per
 * token and nothing trained.  scores[q][r] = 2^-descale_exp * sum_{i<Lq} max_t <Qtok8[q][i], Dtok8[t]> over the DEQUANTISED bytes of
 * query q and document cand[q][r] - id_base: for every slot whose document is in range, fz_maxsim_e4m3's scores[q][cand[q][r] - id_base]
 * bit for bit on any input (the same one 16x16x128 block-scaled MFMA per 16 x 16 dot products with both hardware scales at 2^0, the same
 * fmaxf maximum from -inf, the same summation tree, the same single exact multiply of the finished sum).  Qtok8 [Q][Lq][128] and Dtok8
 * [sumL][128] are the bytes fz_quantize_e4m3_f16 writes; descale_exp is normally the sum of the two quantiser exponents.
 * Slots as in fz_maxsim_pairs_f16: -inf when r >= cand_len[q], when the id is negative or outside [id_base, id_base + N); 0 for an
 * empty document; duplicates scored independently; columns k .. lds-1 untouched.  A row past the document's end, past max_doc_len or
 * past row sumL - 1 is never read.
 * Argument checks in fz_maxsim_pairs_f16's classes and order: negative sizes, Lq <= 0, ldc < k, lds < k, a null pointer where a
 * non-empty tensor is needed (Dtok8 with sumL != 0 included) or |descale_exp| > 32 -> FZ_ERR_ARG; then dim != 128, Lq outside
 * {32, 64, 128}, Qtok8 or Dtok8 not 16-byte aligned -> FZ_ERR_UNSUPPORTED; then Q == 0 or k == 0 -> FZ_OK with nothing launched; then
 * sumL < 0 or max_doc_len <= 0 -> FZ_ERR_ARG and max_doc_len > 16384 -> FZ_ERR_UNSUPPORTED.  Every refusal comes before the first HIP
 * call.  No workspace. */
int fz_maxsim_pairs_e4m3(const void* Qtok8, const void* Dtok8, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N,
                         int dim, int descale_exp, const int64_t* cand, int ldc, const int32_t* cand_len, int k, int64_t id_base,
                         float* scores, int lds, void* stream);

/* ---- K5a/K6: stable descending row sort ---------------------------------------------- */
/* Python sorted(..., reverse=True) is stable (bm25.py:104, hybrid.py:306).  For each row:
 * the incoming sequence is keys gathered through init_order (NULL = identity, i.e. ties ->
 * ascending corpus position), of length row_len[row] (NULL = n); it is sorted by key
 * descending, ties keeping incoming order; -0.0 == +0.0; NaN first.
 * key_bits 32 (fp32 keys) or 64 (fp64 keys).  Outputs, each nullable:
 *   order[row][r]       payload (corpus position) at output rank r, r < row_len[row]
 *   sorted_keys[row][r] its key (same type as keys)
 *   rank[row][payload]  = r  (inverse permutation; other entries untouched: pre-fill with -1)
 * Any n.  Rows of up to fz_sort_max_n() (fp32 keys) / fz_sort_max_n_f64() (fp64 keys) elements live in the registers of one
 * workgroup (the fast path: LLeQA's 27,942 articles fit both); longer rows are chunk-sorted and ranked across chunks
 * (exact and stable as well, O(n * chunks * log n); row_stats are not produced there). */
int fz_sort_max_n(void);
int fz_sort_max_n_f64(void);
/* workspace: fz_sort_workspace_bytes(key_bits, rows, n) bytes of device memory (0 for fp32 rows that fit one workgroup).
 * fp64 keys are sorted by their high word (4 radix passes) and repaired in place where equal high words hide a low-word
 * inversion; a row with such a run longer than 17 keys is flagged in the workspace and redone by a generic 8-pass launch. */
size_t fz_sort_workspace_bytes(int key_bits, int rows, int n);
/* fp32 rows of 8,193 .. 28,672 columns (the rows a 1,024-thread workgroup sorts) that hold at least 4,096 keys and whose scores are spread like a ranker's -- few ties -- are ordered
 * without the digit passes: BUCKET RANKING (16,384 buckets whose widths follow the row's own density, a counting sort by bucket, each
 * key's rank = its bucket's first slot + the members below it, a neighbour check on the result; csrc/sort.hip).  Rows it does not
 * suit (heavy ties, a crowd of values 24 binades below the row's largest, an overfull bucket, a check it cannot settle) take the digit
 * passes as before; the output is the same permutation either way, bit for bit.  FZ_SORT_BUCKET_RANK=0 in the environment turns it
 * off (A/B runs).  fz_sort_bucket_rank_rows: counts3[0] = rows ordered that way on the current device since the last reset,
 * counts3[1] = of those, rows that needed a swapped pair put back, counts3[2] = rows that started on it and were handed to the digit
 * passes; reset != 0 clears the counters.  Synchronises the device (tests and tools only). */
int fz_sort_bucket_rank_rows(uint64_t* counts3, int reset);
/* Round 6 (ABI 19): the ranking sort of a LEXICAL system (bm25.py:100-106: BM25 / TF-IDF score every document, and every document that
 * shares no term with the query scores exactly 0.0 -- most of a corpus).  fz_sort_rows_desc(keys, 64, NULL, ...) for float64 rows in the
 * identity sequence, through an instantiation in which a row of 8,193 .. 28,672 columns at least 3/8 of whose >= 4,096 keys are +-0.0 leaves
 * the zeros out of the ordering phases: the non-zero keys are compacted into fewer items per thread, sorted, and written around the block
 * of zeros, which keep their sequence order (csrc/sort.hip, ZC).  Same stable permutation and outputs, bit for bit, whatever the rows hold;
 * a row without zeros costs ~5 % more here than through fz_sort_rows_desc, a row of 60 % zeros 20 % less, of 80 % a third less -- which is why
 * the caller says what its rows are.  Needs the order output (its row doubles as scratch); other shapes take fz_sort_rows_desc's path.
 * FZ_SORT_ZERO_COMPACT=0 in the environment turns the instantiation off (A/B runs).  fz_sort_zero_compact_rows: counts2[0] = rows compacted on
 * the current device since the last reset, counts2[1] = rows that went through it with too few zeros; reset != 0 clears.  Synchronises the
 * device (tests and tools only). */
int fz_sort_rows_desc_lexical(const double* keys, const int32_t* row_len, int rows, int n, int ld, int32_t* order, double* sorted_keys,
                              int32_t* rank, float* row_stats, void* workspace, size_t workspace_bytes, void* stream);
int fz_sort_zero_compact_rows(uint64_t* counts2, int reset);
/* row_stats (nullable, [4][rows] fp32): mean | UNBIASED standard deviation | min | max of each list's values as float32 (fp64 keys
 * rounded first) -- torch.mean / torch.std / torch.min / torch.max of hybrid.py:254-262, a by-product of having the row in
 * registers (min and max of a sorted list are its two ends; a NaN sorts first and makes both NaN): with them min-max and z-score
 * fusion of ranked systems is one flat pass that reduces nothing (fz_fuse_nsf_pstats_f32 takes row_stats + k*rows directly).  An
 * empty list gives NaN, NaN, 0, 0.
 * stats_len (nullable, [rows] int32, needs row_stats; fp32 keys only, FZ_ERR_UNSUPPORTED otherwise): the statistics cover only the
 * first stats_len[row] entries of the SORTED list -- a ranking cut to its top-k (PLAID-style short ColBERT lists, hybrid.py:137;
 * return_topk) normalises over the listed documents only. */
int fz_sort_rows_desc(const void* keys, int key_bits, const int32_t* init_order, const int32_t* row_len, int rows, int n,
                      int ld, int32_t* order, void* sorted_keys, int32_t* rank, float* row_stats, const int32_t* stats_len,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Same sort, incoming sequence given the other way round: init_rank[row][j] = position of column j in the incoming
 * sequence (-1 = not in it); restricted to the columns in the sequence it is a bijection onto [0, row_len[row]).
 * This is what a rank plane IS, so the fused-list ordering (ties keep system 0's order) needs no gather:
 * keys and positions are read coalesced and placed through LDS. */
int fz_sort_rows_desc_placed(const void* keys, int key_bits, const int32_t* init_rank, const int32_t* row_len, int rows, int n,
                             int ld, int32_t* order, void* sorted_keys, int32_t* rank, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Rank fusion (K5b below) AS THE LOAD PHASE of the final ordering -- hybrid.py:248-252 (the per-rank terms), :301-304 (the float64 sums in
 * system order) and :306 (the stable descending sort) in one kernel: what fz_fuse_rank_f64 followed by fz_sort_rows_desc[_placed] on its
 * plane returns, bit for bit (order, the fused float64 scores in sorted_scores, rank), without the [rows][ld] float64 plane existing.
 * ranks_h: HOST array of S device rank planes [rows][ld] int32 (-1 = the system does not list the document); lens [S][rows] int32 (device).
 * Incoming sequence (the fused dict's first-insertion order): init_rank (placed; when it is ranks_h[0] itself -- every list full -- that
 * plane is read once), or init_order (gathered; row_len = the number of listed documents), or neither (columns in order).
 * n <= fz_sort_max_n_f64() (FZ_ERR_UNSUPPORTED beyond: use the two calls).  Workspace: fz_sort_rank_fused_workspace_bytes(rows, n, ld) --
 * one flag per row + one float64 row per row, written only for rows whose repair the fast form hands to the generic eight-pass launch
 * (more than 2,048 keys sharing a high key word: not a ranker's scores; reserved, not moved, otherwise). */
size_t fz_sort_rank_fused_workspace_bytes(int rows, int n, int ld);
int fz_sort_rank_fused_desc(const int32_t* const* ranks_h, const int32_t* lens, int S, int method, const int32_t* init_order,
                            const int32_t* init_rank, const int32_t* row_len, int rows, int n, int ld, int32_t* order,
                            double* sorted_scores, int32_t* rank, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostic for the call above: out[r] = 1 / (60 + r + 1) (hybrid.py:252) in float64, r < count <= 2^20 -- fast != 0: the division-free
 * sequence its load phase uses, else the IEEE division of fz_fuse_rank_f64.  The two must agree bit for bit (tests). */
int fz_rrf_terms_f64(int count, int fast, double* out, void* stream);

/* Top-k form of the final ordering (what main() reads of the fused lists: predictions(1000), hybrid.py:537).  Per row: the candidates for the
 * first k places of the sort above -- every column with pos >= 0 whose fused score, rounded to float32, is not below the k-th largest such
 * value (the k best and every tie at the k-th place) -- written in no particular order as cand_cols [rows][cap] (column), cand_vals
 * [rows][cap] (its fused score, same type as `fused`), cand_negpos [rows][cap] (-(float)pos: a descending sort of it is ascending insertion
 * order), cand_len [rows].  pos [rows][ld] = first-insertion position of the column (< 0: in no list; NULL: the column index).  Sorting the
 * candidates by cand_negpos and then, stably, by cand_vals (fz_sort_rows_desc twice, rows of cap keys) gives the first k entries of the
 * full sort exactly.  *overflow (device int32, zeroed by the caller) is set when a row has more than cap candidates (a tie run longer
 * than cap - k at the k-th place): sort that batch in full.  n <= 28,672 (one workgroup holds the row), k <= cap. */
int fz_select_topk_f(const void* fused, int key_bits, const int32_t* pos, int rows, int n, int ld, int k, int cap, int32_t* cand_cols,
                     void* cand_vals, float* cand_negpos, int32_t* cand_len, int32_t* overflow, void* stream);

/* ---- K5b: rank-based fusion, hybrid.py:206-211,248-252,301-304 ------------------------- */
/* fused[q][j] = sum over systems s (in the given order, fp64, starting from 0.0) of
 *   rrf: 1/(60+rank+1)     bcf: (len-rank+1)/len      for rank >= 0;  -inf if j is in no list.
 * ranks_h: HOST array of S device pointers, each [Q][ld] int32; lens [S][Q] int32 (device). */
int fz_fuse_rank_f64(const int32_t* const* ranks_h, const int32_t* lens, int S, int Q, int N, int ld, int method,
                     double* fused, void* stream);

/* ---- K3/K4: normalise -> weight -> sum, hybrid.py:212-214,254-280,291,301-304 --------- */
/* per-row statistics over the valid entries (rank NULL = all valid):
 *   FZ_NORM_MINMAX: stat_a=min stat_b=max;  FZ_NORM_ZSCORE: stat_a=mean stat_b=unbiased std
 *   (fp64 accumulation, rounded to fp32; 1-element rows give std=NaN as torch.std does). */
int fz_row_stats_f32(const float* scores, const int32_t* rank, int rows, int N, int ld, int norm, float* stat_a,
                     float* stat_b, void* stream);
/* fused[q][j] = sum_s fl32( t_s(score_s[q][j]) * fl32(w_s) ), fp32, unfused, in system order
 * (NumPy-2 semantics of hybrid.py:291,304), t_s = the normalisation with that row's statistics;
 * docs absent from every system: -inf (so with S = 1 the output is -inf, NOT 0, wherever the system does not list the document:
 * fz_zero_unlisted_f32 turns such a plane into the input fz_gold_ranks_* expects).  One pass over HBM: each plane is read once.
 * planes_h / ranks_h / distr_h: HOST arrays of S device pointers (ranks_h nullable, entries
 * nullable = all docs present; distr_h needed only for PERCENTILE/NCE: ascending fp32 tables of
 * P_h[s] entries, hybrid.py:272).  w_h: HOST fp64 weights (rounded to fp32 inside).
 * norm = FZ_NORM_NONE is rejected here: use fz_fuse_none_f64 (the reference stays in float64). */
/* valid_bits_h (nullable, entries nullable): per system a validity BITMAP [Q][ldb] uint32 (bit j & 31 of word j >> 5 = doc j is in
 * the list) from fz_rank_to_bitmap -- the fusion passes then read 1 bit instead of a 4-byte rank per document; a system with a
 * bitmap needs no ranks_h entry. */
int fz_rank_to_bitmap(const int32_t* rank, int rows, int N, int ld, uint32_t* bits, int ldb, void* stream);
int fz_fuse_nsf_f32(const float* const* planes_h, const int32_t* const* ranks_h, const double* w_h, int S, int Q, int N,
                    int ld, int norm, const float* const* distr_h, const int32_t* P_h, const uint32_t* const* valid_bits_h, int ldb,
                    float* fused, void* stream);
/* Same result for rows longer than the one-pass kernel holds in registers (N > 32768: fz_fuse_nsf_f32 returns
 * FZ_ERR_UNSUPPORTED): min-max / z-score statistics are supplied by the caller, [S][Q] fp32 each, from fz_row_stats_f32
 * (nullable for the other normalisations).  Two passes over HBM. */
int fz_fuse_nsf_stats_f32(const float* const* planes_h, const int32_t* const* ranks_h, const double* w_h, int S, int Q, int N,
                          int ld, int norm, const float* const* distr_h, const int32_t* P_h, const float* stat_a,
                          const float* stat_b, const uint32_t* const* valid_bits_h, int ldb, float* fused, void* stream);
/* The same flat pass with ONE statistics pointer PER SYSTEM: stat_a_h / stat_b_h are HOST arrays of S device pointers, each [Q] fp32
 * (min | mean and max | unbiased std of that system's lists) -- e.g. straight into the row_stats block its ranking sort wrote
 * (fz_sort_rows_desc): a fusion call then gathers, concatenates and reduces nothing. */
int fz_fuse_nsf_pstats_f32(const float* const* planes_h, const int32_t* const* ranks_h, const double* w_h, int S, int Q, int N,
                           int ld, int norm, const float* const* distr_h, const int32_t* P_h, const float* const* stat_a_h,
                           const float* const* stat_b_h, const uint32_t* const* valid_bits_h, int ldb, float* fused, void* stream);
/* ---- percentile-rank / NCE at the table sizes the reference READS: hybrid.py:412,451 (score_distributions_raw_*_28k.csv: |corpus| + 1 =
 * 27,943 quantiles per system) and :374 (_10k: 10,001).  fz_fuse_nsf_f32 keeps all S tables in LDS up to ~1.4 k entries per system at
 * S = 4 and beyond that searches them in global memory (correct, slow).  These entries keep ONE system's table LDS-resident at a time
 * (up to ~38 k entries) and need a prepared workspace: an aligned copy of every table, its bucket table and -- NCE -- the value of every
 * table index.  Same results as fz_fuse_nsf_f32, bit for bit.
 *   fz_nsf_tables_workspace_bytes: bytes for these table lengths (0: a table is too long for LDS or an argument is bad);
 *   fz_nsf_tables_prepare: fills the workspace from the S ascending device tables (one small launch; the workspace stays valid for
 *     any number of fusion calls with the same tables, lengths and norm);
 *   fz_fuse_nsf_tables_f32: fz_fuse_nsf_f32's arguments + the prepared workspace.  FZ_ERR_UNSUPPORTED when a table does not fit LDS or
 *     the planes are not 16-byte aligned with ld % 4 == 0: fz_fuse_nsf_f32 takes those.  Calls whose tables ALL fit LDS at once run
 *     fz_fuse_nsf_f32's table kernel (the workspace is then not read);
 *   fz_nsf_tables_path: which kernel the call above runs for these shapes and pointers (a fz_tables_path, or FZ_ERR_ARG). */
typedef enum {
    FZ_TABLES_PATH_LDS_ALL = 0,   /* every table LDS-resident for the whole launch (fuse_nsf_table_kernel) */
    FZ_TABLES_PATH_LDS_SWAP = 1,  /* one system's table LDS-resident at a time (fuse_nsf_bigtab_kernel) */
    FZ_TABLES_PATH_ROW = 2        /* not taken by fz_fuse_nsf_tables_f32: fz_fuse_nsf_f32's global-memory search */
} fz_tables_path;
size_t fz_nsf_tables_workspace_bytes(int S, const int32_t* P_h, int norm);
/* byte offset, inside a prepared workspace, of system s's 16-byte header {float first entry; float buckets per unit; int32 probes per
 * search; int32 entries in the fullest bucket} -- diagnostics: the search costs `probes` LDS reads per score (log2 of the fullest bucket of
 * an equi-width bucket table; 3..6 for quantile tables of real score distributions, more for tables with long runs of equal entries).
 * (size_t)-1 on a bad argument. */
size_t fz_nsf_tables_header_offset(int S, const int32_t* P_h, int norm, int s);
int fz_nsf_tables_prepare(const float* const* distr_h, const int32_t* P_h, int S, int norm, void* workspace, size_t workspace_bytes,
                          void* stream);
int fz_fuse_nsf_tables_f32(const float* const* planes_h, const int32_t* const* ranks_h, const double* w_h, int S, int Q, int N,
                           int ld, int norm, const float* const* distr_h, const int32_t* P_h, const uint32_t* const* valid_bits_h,
                           int ldb, float* fused, const void* workspace, size_t workspace_bytes, void* stream);
int fz_nsf_tables_path(const float* const* planes_h, const int32_t* const* ranks_h, int S, int Q, int N, int ld, int norm,
                       const int32_t* P_h, const float* fused);
/* plane[q][j] = 0 where rank[q][j] < 0.  A system adds nothing for a document it does not list (hybrid.py:301-304); the
 * single-system planes of fz_fuse_nsf_f32 hold -inf there (see below), the weight sweep wants 0. */
int fz_zero_unlisted_f32(float* plane, const int32_t* rank, int Q, int N, int ld, void* stream);
/* min / max of RANKED lists without a reduction: a list sorted by score has its maximum first and its minimum last.
 * mn[row] = scores[row][order[row][len-1]], mx[row] = scores[row][order[row][0]], len = lens[row] (NULL = N); an empty list gives
 * 0, 0; a NaN at the head makes both NaN (torch.min / torch.max propagate it, hybrid.py:254-258).  With these,
 * fz_fuse_nsf_stats_f32 is a single flat streaming pass -- the fast form of min-max fusion for systems that come with their
 * order plane. */
int fz_minmax_from_order_f32(const float* scores, const int32_t* order, const int32_t* lens, int rows, int N, int ld,
                             float* mn, float* mx, void* stream);
/* The same for all S systems of a fusion in one launch: planes_h / orders_h HOST arrays of S device planes [Q][ld], lens [S][Q]
 * (device, NULL = N), mn / mx [S][Q] -- the layout fz_fuse_nsf_stats_f32 takes. */
int fz_minmax_from_orders_f32(const float* const* planes_h, const int32_t* const* orders_h, const int32_t* lens, int S, int Q, int N,
                              int ld, float* mn, float* mx, void* stream);
/* 'none' / unknown normalisation: fused[q][j] = sum_s (double)score_s * w_s in fp64 (hybrid.py:280,291,304) */
int fz_fuse_none_f64(const float* const* planes_h, const int32_t* const* ranks_h, const double* w_h, int S, int Q, int N,
                     int ld, double* fused, void* stream);
/* Weight-and-sum with NumPy's scalar promotion, for what the two entries above do not cover (hybrid.py:291,304):
 *   plane_is_f64_h[s] != 0: planes_h[s] is a float64 plane (BM25's Python-float scores, raw scores of a host list) --
 *     the 'none' passthrough keeps them unrounded;
 *   narrow_h[s] != 0: w_s is a weak (Python float) or float32 weight: fl32 product, and a document's sum stays fl32 until
 *     its first float64 product; narrow_h[s] == 0: w_s is an np.float64 (the tuning grid, hybrid.py:405-409): float64.
 * Inputs for the normalised modes are the per-system transformed planes (fz_fuse_nsf_f32 of one system, weight 1).
 * Both arrays nullable (= all float32 planes, all wide: fz_fuse_none_f64). */
int fz_fuse_wsum_f64(const void* const* planes_h, const int32_t* plane_is_f64_h, const int32_t* const* ranks_h,
                     const double* w_h, const int32_t* narrow_h, int S, int Q, int N, int ld, double* fused, void* stream);

/* ---- first-insertion order of the fused dict, hybrid.py:301-304 (tie-break, SURVEY KAT-1) */
/* ins_order[q][0..U[q]) = docs in the order aggregate_scores first inserts them: system by system,
 * each in its rank order, skipping docs already seen.  orders_h: HOST array of S device pointers
 * [Q][ld]; lens [S][Q].  pos (nullable, [Q][ld], pre-filled with -1 by the caller): the inverse, pos[q][doc] = its first-insertion
 * position -- what fz_gold_ranks_* and fz_select_topk_f take.  Workspace: fz_insertion_order_workspace_bytes(Q, N). */
size_t fz_insertion_order_workspace_bytes(int Q, int N);
int fz_insertion_order(const int32_t* const* orders_h, const int32_t* lens, int S, int Q, int N, int ld, int32_t* ins_order,
                       int32_t* U, int32_t* pos, void* workspace, size_t workspace_bytes, void* stream);

/* ---- top-k + shard merge (csrc/topk.hip): sentence_transformers.py:346-364 (chunked score -> topk -> heap) */
/* k best of each row by (score desc, id asc); ids = id_base + column. out [rows][k]; rows with
 * fewer than k columns are padded with (-inf, -1).  k <= fz_topk_max_k(). */
int fz_topk_max_k(void);
size_t fz_topk_workspace_bytes(int rows, int n, int k);
int fz_topk_rows_f32(const float* scores, int rows, int n, int ld, int k, int64_t id_base, float* out_scores,
                     int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 20, additive) What fz_topk_rows_f32 does with a row of n columns at this k: the function the entry itself runs, host arithmetic
 * only, no HIP call, no GPU needed (tests/topk_cases.py proves which branches a shape takes through it).  A row wider than one sort row
 * (35,840) goes through chunk-sort-truncate levels: chunks of 28,672 columns each keep their kk = min(k, 28,672) best.
 * out[FZ_TOPK_ROWS_PLAN_FIELDS]: levels | pad (n < k: the outputs end in (-inf, -1)) | the width the finishing sort reads | then per level
 * l < FZ_TOPK_ROWS_PLAN_LEVELS: its input width, chunks, kk, fill (1: the last chunk holds fewer than kk keys and the level's output is
 * pre-filled with (-inf, -1)); zeros past the last level.  n < 0, k <= 0 or out == NULL -> FZ_ERR_ARG, k > fz_topk_max_k() ->
 * FZ_ERR_UNSUPPORTED, as the entry answers; nothing is written then. */
#define FZ_TOPK_ROWS_PLAN_LEVELS 12
#define FZ_TOPK_ROWS_PLAN_FIELDS 51
int fz_topk_rows_plan(int n, int k, int32_t* out);
/* streaming form of the same loop: merge one more chunk of scores into the running per-row top-k.  Only scores strictly
 * above a row's current k-th best can enter (chunks arrive in ascending id order, so ties lose), so the chunk is filtered
 * in one streaming pass and only the survivors (+ the running list) are sorted.  run_* [rows][k] -> new_* [rows][k]
 * (distinct buffers, sorted by score desc, id asc; (-inf,-1) padding).  *overflow (device int32, zeroed by the caller)
 * is set when a row had more than `cap` survivors: redo that chunk with fz_topk_rows_f32 + fz_topk_merge.
 * PRECONDITION of the streamed forms (this entry, fz_topk_filter_append_f32 + fz_topk_fold_f32): the filter keeps !(score <= tau) with
 * tau = the running list's k-th score, so while the running list is SHORT (fewer than k real entries: (-inf, -1) padding, tau = -inf) a
 * score of exactly -inf in a later chunk is dropped, where fz_topk_rows_f32 of the whole matrix lists it, with its id, ahead of the padding.
 * The streamed forms equal fz_topk_rows_f32 of the whole matrix when every running list is full (k real entries) OR no score is -inf;
 * otherwise they differ exactly in that -inf documents are listed as padding.  The index classes start from a head of >= 8 k documents. */
size_t fz_topk_update_workspace_bytes(int rows, int k, int cap);
int fz_topk_update_f32(const float* scores, int rows, int n, int ld, int64_t id_base, const float* run_scores,
                       const int64_t* run_ids, int k, int cap, float* new_scores, int64_t* new_ids, int32_t* overflow,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same step in two halves, so that several chunks share ONE sort (the sharded search folds 4 times per 1.1 M-document shard
 * instead of once per chunk): fz_topk_filter_append_f32 appends the chunk's scores above tau[row] (or NaN) to the row's candidate
 * list -- ascending id inside the chunk, chunks fed in ascending id order; fz_topk_fold_f32 merges [running k | candidates] into
 * the new running list (ties: running entries first, then ascending id), writes the new threshold tau_out[row] = k-th best
 * (nullable) and empties the candidate lists.  cand_scores / cand_ids [rows][cap], cand_len [rows] int32 (zero before the first
 * call); *overflow becomes 1 if a row's list would exceed cap (the caller then redoes the search exactly).  k + cap <= 35840.
 * unordered != 0: the candidates are in no particular order (fz_dot_scores_filter_f32 appends them as its waves finish); the fold
 * then also puts every run of equal scores that reaches into the first k into ascending id order -- the same lists as from ordered
 * candidates -- and sets *overflow if such a run is longer than it looks at (64 entries past k, 512 in all).
 * (ABI 20, additive) fz_topk_fold_max_k(unordered): the largest k the fold takes -- 5,056 for the unordered form (k + 64 entries of 12 bytes
 * in 60 KiB of LDS), 35,839 otherwise; beyond it, as for k + cap > 35840, fz_topk_fold_f32 answers FZ_ERR_UNSUPPORTED before its first
 * launch: new_*, tau_out, cand_len and *overflow stay as they were. */
int fz_topk_fold_max_k(int unordered);
int fz_topk_filter_append_f32(const float* scores, int rows, int n, int ld, int64_t id_base, const float* tau, float* cand_scores,
                              int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream);
size_t fz_topk_fold_workspace_bytes(int rows, int k, int cap);
int fz_topk_fold_f32(const float* run_scores, const int64_t* run_ids, int rows, int k, const float* cand_scores, const int64_t* cand_ids,
                     int32_t* cand_len, int cap, int unordered, float* new_scores, int64_t* new_ids, float* tau_out, int32_t* overflow,
                     void* workspace, size_t workspace_bytes, void* stream);
/* merge G per-shard lists [G][rows][k] (as all-gathered over RCCL) into the global top-k [rows][k] */
int fz_topk_merge(const float* in_scores, const int64_t* in_ids, int G, int rows, int k, float* out_scores, int64_t* out_ids,
                  void* stream);
/* C1 -- the ONE collective of the corpus-sharded configuration (spec: the heap merge across corpus chunks of
 * sentence_transformers.py:346-364, here across GPUs): ncclAllGather of this rank's [Q][k] (fp32 score, int64 id) lists over
 * `rccl_comm` (an ncclComm_t of `world` ranks, one per GPU) into the workspace, then the local G-way merge -- identical on
 * every rank, ties by ascending global id.  RCCL is resolved at run time (the host process's copy first, then librccl.so);
 * FZ_ERR_UNSUPPORTED when there is none.  Workspace: fz_topk_allgather_workspace_bytes(world, Q, k) device bytes. */
size_t fz_topk_allgather_workspace_bytes(int world, int Q, int k);
int fz_topk_allgather(const float* local_scores, const int64_t* local_ids, int Q, int k, void* rccl_comm, int world,
                      float* out_scores, int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fusion of top-k LISTS: per-query id join (hybrid.py:293-307 on lists of any ids) --------- */
/* What the searches above return -- per query k (score, int64 global id) pairs per system -- fused without any plane over the
 * corpus: one workgroup per query joins the S lists on their ids in LDS (csrc/lists.hip).
 * Inputs, per system s (HOST arrays of S entries): ids_h[s] device [Q][ld_h[s]] int64; lens_h[s] device [Q] int32 (clamped to
 * [0, n_h[s]]; entries past it are padding and are never read); n_h[s] = list width (k), ld_h[s] >= n_h[s] = row stride in elements
 * of ids_h[s] and values_h[s].  Ids are arbitrary int64 and must be distinct inside one list.
 * Outputs, per query, in the fused dict's FIRST-INSERTION order (system 0's entries in list order, then system 1's new ones, ...):
 * out_ids [Q][ld_out] int64, out_scores [Q][ld_out] (float32 for FZ_LISTS_WSUM_F32, float64 otherwise), out_len [Q] = size of the
 * union; columns past out_len are not written.  ld_out >= sum of n_h.  The final ranking is fz_sort_rows_desc on out_scores with
 * row_len = out_len (ties -> ascending column = the reference's tie rule) and a gather of out_ids.
 * Score of a column: 0 + c_s1 + c_s2 + ... over the systems that list the id, in system order, with
 *   FZ_LISTS_RRF       c = 1 / (60 + r + 1), float64 (fz_fuse_rank_f64's bits), r = position in the list;
 *   FZ_LISTS_BCF       c = (n - r + 1) / n, float64, n = the list's length;
 *   FZ_LISTS_WSUM_F32  c = fl32(values_h[s][q][r] * fl32(w_h[s])), float32 sum (fz_fuse_nsf_f32's weighting);
 *   FZ_LISTS_WSUM_F64  fz_fuse_wsum_f64's rule: value_is_f64_h[s] / narrow_h[s] as there (both nullable).
 * values_h / w_h are read by the two WSUM methods only.  sum of n_h <= fz_lists_max_entries() (>= 8192), FZ_ERR_UNSUPPORTED
 * beyond.  Workspace: fz_lists_join_workspace_bytes(S, Q) device bytes; its first int32 is the DUPLICATE FLAG: zeroed by the
 * call, non-zero afterwards when some list held an id twice (the outputs are then unspecified, never out of bounds).
 * Every argument is checked before the first HIP call.  Q == 0 or all n_h == 0: FZ_OK, nothing launched (out_len is left as the
 * caller initialised it: zeros). */
typedef enum { FZ_LISTS_RRF = 0, FZ_LISTS_BCF = 1, FZ_LISTS_WSUM_F32 = 2, FZ_LISTS_WSUM_F64 = 3 } fz_lists_method;
int fz_lists_max_entries(void);
size_t fz_lists_join_workspace_bytes(int S, int Q);
int fz_lists_join(const int64_t* const* ids_h, const int32_t* const* lens_h, const void* const* values_h,
                  const int32_t* value_is_f64_h, const double* w_h, const int32_t* narrow_h, const int32_t* n_h,
                  const int32_t* ld_h, int S, int Q, int method, int64_t* out_ids, void* out_scores, int32_t* out_len,
                  int ld_out, void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 20, additive) The same join to per-system COLUMNS: the form the weight sweep (fz_gold_ranks_*, fz_tune_metrics_f64) takes, for
 * lists over any ids (csrc/lists_tune.hip).  Inputs as for fz_lists_join; values_h[s] device [Q][ld_h[s]] fp32 (the system's
 * normalised scores in list order).  Outputs, per query, all with ONE row stride ld_out >= sum of n_h:
 *   out_ids [Q][ld_out] int64, out_len [Q]   the union's ids in first-insertion order and their number -- fz_lists_join's bytes;
 *                                            out_ids holds -1 from out_len on;
 *   T_h[s]  [Q][ld_out] fp32 (HOST array of S device pointers)   values_h[s][q][r] in the column of ids_h[s][q][r], r < lens;
 *                                            +0.0 in every other element of the row (a system adds nothing for an id it does not list);
 *   pos     [Q][ld_out] int32                c for c < out_len[q], -1 beyond: the first-insertion position, i.e. the tie-break;
 *   gold_col[Q][G] int32                     the column of gold_ids[q][g] (device [Q][G] int64); -1 for a negative id (padding) or
 *                                            an id in no list of the query.  G >= 0; G == 0: both may be NULL.
 * The kernel defines every element of every output row itself (no pre-fill is needed) and two calls give the same bytes.
 * values_h == NULL: an ids / pos / gold-only join -- T_h is not read (with S == 1 the column of an id is its list position).
 * Capacity, duplicate flag (first int32 of the workspace, fz_lists_columns_workspace_bytes(S, Q) device bytes), argument checks
 * and return codes as for fz_lists_join.  Q == 0 or all n_h == 0: FZ_OK, nothing launched, nothing written. */
size_t fz_lists_columns_workspace_bytes(int S, int Q);
int fz_lists_columns(const int64_t* const* ids_h, const int32_t* const* lens_h, const float* const* values_h, const int32_t* n_h,
                     const int32_t* ld_h, int S, int Q, const int64_t* gold_ids, int G, int64_t* out_ids, float* const* T_h,
                     int32_t* pos, int32_t* out_len, int32_t* gold_col, int ld_out, void* workspace, size_t workspace_bytes,
                     void* stream);
/* (ABI 20, additive) PASSAGE lists to DOCUMENT lists, MaxP (csrc/lists_collapse.hip).  A long document is indexed as passages;
 * passage id p + id_base belongs to document group_of[p] + doc_id_base (group_of device [P] int32, non-decreasing).
 * Inputs, ONE list per query in (score desc, id asc) order, one row stride ld >= n for all three planes:
 *   ids [Q][ld] int64, scores [Q][ld] fp32, scores64 [Q][ld] fp64 (nullable: BM25's raw scores), lens [Q] int32 clamped to [0, n];
 *   slots past a row's length are never read.
 * Outputs, per query, one row stride ld_out >= n; column c is the c-th DISTINCT document of the list, which in a ranked list is the
 * MaxP ranking (a document's first occurrence is its best passage; equal scores keep list order):
 *   out_ids [Q][ld_out] int64 the document id, out_scores (and out_scores64, given exactly when scores64 is) the score of the
 *   entry that opened the column -- its own bits --, out_best [Q][ld_out] int64 that entry's passage id, out_len [Q] the number of
 *   distinct documents.  From out_len on the rows hold (-1, -inf, -1) up to ld_out: the kernel defines every element of every
 *   output row itself (no pre-fill is needed) and two calls give the same bytes.
 * n <= fz_lists_max_entries(), FZ_ERR_UNSUPPORTED beyond.  Workspace: fz_lists_collapse_workspace_bytes(Q) device bytes; its first
 * int32 is a FLAG WORD, zeroed by the call: bit 0 = a listed passage id outside [id_base, id_base + P), bit 1 = a row that is not
 * non-increasing, !(s[r-1] >= s[r]) for some 1 <= r < len (NaN included; equal scores and -inf are fine).  With a bit set the
 * outputs are unspecified, never out of bounds.  A repeated DOCUMENT is the normal case and sets nothing.
 * Every argument is checked before the first HIP call.  Q == 0 or n == 0: FZ_OK, nothing launched, nothing written. */
size_t fz_lists_collapse_workspace_bytes(int Q);
int fz_lists_collapse(const int64_t* ids, const float* scores, const double* scores64, const int32_t* lens, int ld, int n, int Q,
                      const int32_t* group_of, int64_t P, int64_t id_base, int64_t doc_id_base, int64_t* out_ids, float* out_scores,
                      double* out_scores64, int64_t* out_best, int32_t* out_len, int ld_out, void* workspace,
                      size_t workspace_bytes, void* stream);
/* (ABI 20, additive) Exact MaxP score of candidate DOCUMENTS: expand, score the passages with any pair kernel, reduce.
 * fz_group_expand: cand [Q][ld] int64 document ids (W per row, ld >= W), cand_len [Q] int32 (nullable = W), CSR poff device [D + 1]
 * int64 (document d owns passages poff[d] .. poff[d + 1] - 1) ->
 *   pcand [Q][ldp] int64   the passage ids (+ id_base), slot 0's passages first, then slot 1's, ...; -1 from pcand_len on;
 *   seg   [Q][W + 1] int32 slot w's passages are pcand[q][seg[w] .. seg[w + 1] - 1];   pcand_len [Q] int32 = seg[q][W].
 * A slot past cand_len, a negative id, an id outside [doc_id_base, doc_id_base + D) or a document without passages gets an empty
 * segment.  A row that needs more than ldp slots sets the flag (first int32 of the workspace, fz_group_expand_workspace_bytes(Q)
 * device bytes, zeroed by the call): its segments are cut at ldp, nothing is written out of bounds.
 * fz_group_max_f32 / _f64: pscores [Q][ld_s] (ld_s >= ldp: the pair kernel's scores of pcand) ->
 *   out [Q][ld_out] the maximum over slot w's segment, the winning entry's own bits; best [Q][ld_out] int64 (the same stride) the
 *   passage id of the FIRST maximum (the lowest passage id among equals); (-inf, -1) for an empty segment and for w >= cand_len.
 * Scores are finite or -inf (the pair kernels' contract).  Arguments are checked before the first HIP call; Q == 0 (or W == 0 for
 * the maximum): FZ_OK, nothing launched. */
size_t fz_group_expand_workspace_bytes(int Q);
int fz_group_expand(const int64_t* cand, int ld, const int32_t* cand_len, int W, int Q, const int64_t* poff, int64_t D,
                    int64_t id_base, int64_t doc_id_base, int64_t* pcand, int ldp, int32_t* seg, int32_t* pcand_len,
                    void* workspace, size_t workspace_bytes, void* stream);
int fz_group_max_f32(const float* pscores, int ld_s, const int64_t* pcand, int ldp, const int32_t* seg, const int32_t* cand_len,
                     int W, int Q, float* out, int64_t* best, int ld_out, void* stream);
int fz_group_max_f64(const double* pscores, int ld_s, const int64_t* pcand, int ldp, const int32_t* seg, const int32_t* cand_len,
                     int W, int Q, double* out, int64_t* best, int ld_out, void* stream);

/* ---- A1: BM25 scoring on device, bm25.py:149-156 -------------------------------------- */
/* scores[q][j] (fp64) = sum over query terms in query order of idf*tf*(k1+1)/(tf+k1*(1-b+b*dl/avgdl)).
 * CSR postings by term (toff [V+1], pdoc, ptf), idf [V] fp64, doc_len [N]; queries as CSR of term
 * ids (qoff [Q+1], qterms; -1 = out of vocabulary).
 * doc_norm (nullable): per-document k1*(1-b+b*dl/avgdl) from fz_bm25_doc_norms_f64 -- the same fp64 bits as the inline
 * sub-expression, computed once per document instead of once per posting. */
int fz_bm25_doc_norms_f64(const int32_t* doc_len, int N, double avgdl, double k1, double b, double* out, void* stream);
/* slice_off (nullable): per-index table [V][NS + 1] int64, NS = ceil(N / fz_bm25_slice_docs()): the first posting of term t whose document
 * is >= s * fz_bm25_slice_docs() (entry NS = toff[t + 1]), from fz_bm25_slice_offsets (a GRAIN of 3,584 documents; a workgroup scores one (query, slice of one or two grains)) -- a workgroup
 * otherwise finds every query term's posting sub-range by two binary searches of ~15 dependent loads each. */
int fz_bm25_slice_docs(void);
int fz_bm25_slice_offsets(const int64_t* toff, const int32_t* pdoc, int V, int N, int64_t* out, void* stream);
int fz_bm25_scores_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int32_t* doc_len,
                       const double* doc_norm, const int64_t* slice_off, double avgdl, double k1, double b, const int64_t* qoff,
                       const int32_t* qterms, int Q, int N, double* scores, int lds, void* stream);
/* The same launch also writing the scores rounded to float32 (scores32 [Q][lds32], nullable) -- the plane the normalisations read
 * (torch.tensor(scores, dtype=float32), hybrid.py:255) -- from the same accumulators: no separate conversion pass over the float64 plane. */
int fz_bm25_scores_f64_f32(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int32_t* doc_len,
                           const double* doc_norm, const int64_t* slice_off, double avgdl, double k1, double b, const int64_t* qoff,
                           const int32_t* qterms, int Q, int N, double* scores, int lds, float* scores32, int lds32, void* stream);

/* Round 6 (ABI 19): the posting-value table.  For a given index and (k1, b) every posting has ONE term value
 *   pval[e] = idf_t * (tf_e * (k1 + 1)) / (tf_e + doc_norm[d_e])      (float64, the expression order of bm25.py:154)
 * -- idf, tf and the length norm are all the index's, nothing in it depends on the query.  fz_bm25_posting_values_f64 tabulates it once
 * (like the idf table; once per (k1, b) of a grid search), fz_bm25_scores_pv_f64_f32 is fz_bm25_scores_f64_f32 whose walk only ADDS the
 * tabulated terms, in query order: the same planes, bit for bit, without a float64 division per (query, posting) -- most of the scoring
 * kernel's time (1024 queries x 27,942 documents: 0.33 -> 0.1x ms).  doc_norm: fz_bm25_doc_norms_f64 (required here). */
int fz_bm25_posting_values_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const double* doc_norm,
                               int V, int64_t nnz, double k1, double* out, void* stream);
int fz_bm25_scores_pv_f64_f32(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                              const int32_t* qterms, int Q, int N, double* scores, int lds, float* scores32, int lds32, void* stream);
/* TFIDF.score (bm25.py:108-115), the base class of the reference's lexical retrievers: scores[q][j] (fp64) = sum over the query's terms,
 * in query order, of tf(t, d) * idf(t) -- the same posting walk without the length norm.  idf [V] is the caller's table (TFIDF's is
 * log10((N + 1) / (df + 1)), bm25.py:86-88; AtireBM25 hands that table to fz_bm25_scores_f64 instead, bm25.py:170-172).  slice_off,
 * scores32: as above, both nullable.  (ABI 19) */
int fz_tfidf_scores_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                        const int64_t* qoff, const int32_t* qterms, int Q, int N, double* scores, int lds, float* scores32, int lds32,
                        void* stream);

/* ---- N1: weight-grid sweep of the linear fusion, hybrid.py:404-426 ------------------------ */
/* Fused ranks of the gold documents for W weight vectors at once, without fusing or sorting:
 * out_ranks[w][q][g] = #{docs that precede gold g in the list Aggregator.fuse(method='nsf') would return with
 * weights[w]} (fused score desc, ties by first-insertion position).  Every metric of run_evaluation is a
 * function of these ranks.  T_h: HOST array of S device planes [Q][ld] holding the NORMALISED scores
 * (fz_fuse_nsf_f32 of one system with weight 1, then -- for a system with a partial list -- fz_zero_unlisted_f32: entries of docs
 * the system does not list MUST be 0, the kernel multiplies them by the weights like any other; fz_fuse_nsf_f32 leaves -inf
 * there); pos [Q][ld] =
 * first-insertion position (-1 = in no list); weights [W][S] fp32; gold [Q][fz_tune_max_gold()] corpus positions
 * (-1 = padding); out_ranks must be zeroed by the caller.  S <= 4. */
int fz_tune_max_gold(void);
int fz_gold_ranks_f32(const float* const* T_h, const int32_t* pos, const float* weights, const int32_t* gold, int S, int W,
                      int Q, int N, int ld, int32_t* out_ranks, void* stream);
/* The same with np.float64 weights [W][S] -- what the reference's own grid holds (np.arange, hybrid.py:405-409): float64
 * products and sums (NumPy promotion of np.float32 * np.float64), ranks by the float64 fused score. */
int fz_gold_ranks_f64w(const float* const* T_h, const int32_t* pos, const double* weights, const int32_t* gold, int S, int W,
                       int Q, int N, int ld, int32_t* out_ranks, void* stream);
/* The metrics of run_evaluation (hybrid.py:24-42 over metrics.py:40-136) of every weight vector, from those ranks, on the device:
 * per query in float64 and in the reference's operation order -- recall@k, MAP@k, MRR@k, nDCG@k (its shifted discount,
 * metrics.py:108), R-precision -- and the mean over the Q queries as an exactly accumulated sum rounded once.
 * ranks [W][Q][G], gold [Q][G], pos [Q][ld] as above (G = fz_tune_max_gold(); a gold document with pos < 0 is in no list and never
 * counts); n_gold [Q] = len(ground_truths), the reference's divisor; idcg [Q] and disc [top+1] (disc[0] = 1, disc[i] = 1/log2(i+1))
 * come from the host, computed as the reference computes them; cuts = the n_recall + n_map + n_mrr + n_ndcg cut-offs in that
 * order.  out [W][M] float64, M = that count + 1 (R-precision last), M <= 24. */
int fz_tune_metrics_f64(const int32_t* ranks, const int32_t* gold, const int32_t* pos, int ld, const int32_t* n_gold, const double* idcg,
                        const double* disc, int top, const int32_t* cuts, int n_recall, int n_map, int n_mrr, int n_ndcg, int W, int Q,
                        double* out, void* stream);

/* ---- A3, sparse form: SPLADE cosine scoring over an inverted index ------------------------------------------------------------------
 * util.semantic_search(query_embeddings, corpus_embeddings, score_function=util.cos_sim) (hybrid.py:103) on SPLADE vectors
 * (splade/splade.py:88-99: a few hundred non-zeros of 32,005) without the dense [N, 32005] matrix: the L2-normalised corpus vectors as
 * postings -- toff [V + 1] (device int64), pdoc / pw [nnz]: (document, weight) of term t in [toff[t], toff[t+1]), documents ascending --
 * and the L2-normalised queries as qoff [Q + 1], qterms / qw: the non-zero terms of query q, ascending.
 *     scores[q][d] = sum over the query's terms t, ascending, of qw * pw        (float32, one rounding per product and per add)
 * = the dense product minus its exact zeros.  slice_off (nullable): fz_sparse_slice_offsets' [V][NS + 1] table, NS = ceil(N /
 * fz_sparse_slice_docs()) -- where every term's postings cross the document slices a workgroup owns.  scores [Q][lds] float32. */
int fz_sparse_slice_docs(void);
int fz_sparse_slice_offsets(const int64_t* toff, const int32_t* pdoc, int V, int N, int64_t* out, void* stream);
int fz_sparse_dot_f32(const int64_t* toff, const int32_t* pdoc, const float* pw, const int64_t* slice_off, const int64_t* qoff,
                      const int32_t* qterms, const float* qw, int Q, int N, float* scores, int lds, void* stream);
/* (ABI 20) The same scores for the documents [doc_lo, doc_hi) of the index only: doc_lo % fz_sparse_slice_docs() == 0, doc_hi a multiple of it
 * or N; scores [Q][lds], lds >= doc_hi - doc_lo, column j = document doc_lo + j -- bit for bit the full plane's column doc_lo + j (same chain of
 * adds per document).  fz_sparse_dot_f32 is this call with [0, N). */
int fz_sparse_dot_range_f32(const int64_t* toff, const int32_t* pdoc, const float* pw, const int64_t* slice_off, const int64_t* qoff,
                            const int32_t* qterms, const float* qw, int Q, int N, int doc_lo, int doc_hi, float* scores, int lds, void* stream);
/* (ABI 20) The corpus-scale SPLADE search step (splade/base.py:199-251's chunked top-k): the same walk over [doc_lo, doc_hi) with the streaming
 * top-k's threshold filter in place of the plane -- NO score plane is written; document d enters query q's candidate list iff
 * !(score <= tau[q]) (greater, or NaN), appended as (score, id_base + d) -- the rule and lists of fz_dot_scores_filter_f32: cand_scores /
 * cand_ids [Q][cap], cand_len [Q] int32 (may run past cap: the excess is dropped and *overflow set to 1), in arrival order, i.e. for
 * fz_topk_fold_f32(unordered = 1).  tau [Q]. */
int fz_sparse_dot_filter_f32(const int64_t* toff, const int32_t* pdoc, const float* pw, const int64_t* slice_off, const int64_t* qoff,
                             const int32_t* qterms, const float* qw, int Q, int N, int doc_lo, int doc_hi, int64_t id_base, const float* tau,
                             float* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream);

/* ---- A1 at corpus scale: the lexical posting walk over a document range, plane or filter epilogue (csrc/bm25_stream.hip; ABI 20, additive) ----
 * The walks of fz_bm25_scores_pv_f64_f32 (BM25 / AtireBM25 from the posting-value table) and fz_tfidf_scores_f64 for the documents
 * [doc_lo, doc_hi) of an index of N documents only.  A workgroup scores one (query, slice) of fz_lexical_slice_docs(tfidf) documents:
 * 3,584 for the posting-value walk (tfidf = 0), 7,168 for TF-IDF (tfidf != 0) -- one or two grains of fz_bm25_slice_docs().
 * doc_lo must be a multiple of that slice, doc_hi a multiple of it or N.  slice_off (nullable): fz_bm25_slice_offsets' table for the WHOLE
 * index (row stride from N); without it every workgroup finds its posting sub-ranges by binary search.  Per document the score is the
 * same chain of float64 adds in query-term order as the full-plane kernels make (terms not de-duplicated, id -1 adds nothing):
 * scores [Q][lds] float64, lds >= doc_hi - doc_lo, column j = document doc_lo + j = the full plane's column doc_lo + j, bit for bit.
 * Checks, in this order: Q < 0, a bad range or lds -> FZ_ERR_ARG; Q == 0 or an empty range -> FZ_OK, nothing launched; then null pointers
 * (every array but slice_off: an index without postings has nothing to walk) -> FZ_ERR_ARG. */
int fz_lexical_slice_docs(int tfidf);
int fz_bm25_scores_range_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, double* scores, int lds, void* stream);
int fz_tfidf_scores_range_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                              const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, double* scores, int lds,
                              void* stream);
/* The same walks with the streaming top-k's threshold filter in place of the plane store -- NO score plane is written.  Document d enters
 * query q's candidate list iff !(score <= tau[q]) (greater, or NaN; tau [Q] float64), appended as (float64 score, int64 id_base + d):
 * cand_scores / cand_ids [Q][cap], cand_len [Q] int32 (the caller zeroes it; it keeps counting past cap), in arrival order.  Nothing is
 * written at or past slot cap; a workgroup that had to drop a candidate sets *overflow to 1.  Checks as above with cap <= 0 among the
 * FZ_ERR_ARG cases and tau, cand_scores, cand_ids, cand_len, overflow among the pointers. */
int fz_bm25_filter_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                          const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base, const double* tau,
                          double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream);
int fz_tfidf_filter_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                        const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base,
                        const double* tau, double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow,
                        void* stream);

/* ---- A1's grid search at corpus scale: the ranks of listed documents as counts on the posting walk (csrc/bm25_count.hip; ABI 20, additive) ----
 * Every metric of the k1 x b sweep (bm25.py:221-237) is a function of the gold documents' ranks, and a rank is a count:
 * rank(g) = #{ d : d is ranked before g } in the stable descending float64 ranking (ties to the ascending id) -- no plane, list or sort.
 * fz_*_doc_scores_*: docs [Q][G] int32 positions in this index -> out [Q][G] float64, the score the walks above give that document for that
 * query, bit for bit (the same chain of adds, found by binary search in each query term's postings); a position < 0 or >= N gives -inf
 * (so shards combine with one MAX).  Checks, in this order: Q < 0, N < 0 or G < 1 -> FZ_ERR_ARG; Q == 0 -> FZ_OK; then null pointers. */
int fz_bm25_doc_scores_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* qoff, const int32_t* qterms, int Q,
                              int N, const int32_t* docs, int G, double* out, void* stream);
int fz_tfidf_doc_scores_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* qoff,
                            const int32_t* qterms, int Q, int N, const int32_t* docs, int G, double* out, void* stream);
/* fz_*_count_*: the range walks above (same range rules, same slice_off) with a counting epilogue.  gold_scores [Q][G] float64 and gold_ids
 * [Q][G] int64 (global ids; < 0: skip this gold) name G documents per query; counts [Q][G] int32 is ADDED to (the caller zeroes it):
 * counts[q][g] += the number of documents d of [doc_lo, doc_hi), with id i = id_base + d and score s, such that s ranks before the gold's
 * score (the float64 sort's key order: descending, -0.0 == +0.0, NaN first), or equals it with i < gold_ids[q][g].  The gold may lie
 * anywhere -- in the range, elsewhere in the index, in another shard; it never counts itself.  Integer adds only: counts over disjoint
 * ranges, chunks and shards sum to the rank, identically in every run.  Checks, in this order: Q < 0, a bad range or G < 1 -> FZ_ERR_ARG;
 * Q == 0 or an empty range -> FZ_OK, nothing launched; then null pointers (every array but slice_off) -> FZ_ERR_ARG. */
int fz_bm25_count_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                         const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base, const double* gold_scores,
                         const int64_t* gold_ids, int G, int32_t* counts, void* stream);
int fz_tfidf_count_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                       const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base,
                       const double* gold_scores, const int64_t* gold_ids, int G, int32_t* counts, void* stream);

/* ---- K2 at corpus scale, first stage: candidate scores from token centroids (csrc/centroid.hip; ABI 20, additive) ------------------------
 * Ranker.multi_vector_search (hybrid.py:108-137) is a first-stage search: colbert-ai generates candidates from token centroids and scores
 * them exactly (fz_maxsim_pairs_f16 is the exact part).  Every document token carries the id of its nearest of K centroids; the index
 * lists, per centroid c, the DISTINCT documents that hold it: cdoc [coff[c], coff[c+1]) (int32, ascending), coff [K + 1] int64.  A query is
 * its probe table, token-major: pc / ps [Q][Lq * nprobe], token i's nprobe best centroids (score desc, id asc) and their scores;
 * pc < 0 pads.  With m_i = the largest ps over token i's probes whose list holds d,
 *     scores[q][d] = ((+0.0 + m_i1) + m_i2) + ...     over the tokens i that hit d, ascending          (float32)
 * A token without a hit adds nothing, a document without any scores +0.0, a negative probe score counts as it is.  The max does not
 * depend on order and the adds have a fixed one: the score is defined bit for bit, the same for a range as for the whole index.  Probe
 * scores must be finite (a non-finite query token is outside the contract).  Lq >= 1, nprobe >= 1, both of any size.
 * A workgroup scores one (query, slice) of fz_centroid_slice_docs() documents: doc_lo must be a multiple of it, doc_hi a multiple or N.
 * slice_off (nullable): fz_centroid_slice_offsets' [K][NS + 1] table for the WHOLE index, NS = max(1, ceil(N / slice)) -- where every
 * centroid's list crosses the slices; without it a workgroup finds its segments by binary search, with the same result.
 * Checks, in this order: negative sizes, Lq < 1, nprobe < 1, a bad range or lds < doc_hi - doc_lo -> FZ_ERR_ARG; Q == 0 or an empty
 * range -> FZ_OK, nothing launched; then null pointers (coff, pc, ps and the outputs) -> FZ_ERR_ARG. */
int fz_centroid_slice_docs(void);
int fz_centroid_slice_offsets(const int64_t* coff, const int32_t* cdoc, int K, int N, int64_t* out, void* stream);
int fz_centroid_scores_range_f32(const int64_t* coff, const int32_t* cdoc, const int64_t* slice_off, const int32_t* pc, const float* ps, int Q,
                                 int Lq, int nprobe, int N, int K, int doc_lo, int doc_hi, float* scores, int lds, void* stream);
/* The same walk with the streaming top-k's threshold filter in place of the plane -- fz_sparse_dot_filter_f32's rule and lists: document d
 * enters query q's candidates iff !(score <= tau[q]), appended as (score, id_base + d); cand_scores / cand_ids [Q][cap], cand_len [Q]
 * int32 (keeps counting past cap: the excess is dropped, nothing is written at or past slot cap and *overflow is set to 1), in arrival
 * order, i.e. for fz_topk_fold_f32(unordered = 1).  cap <= 0 -> FZ_ERR_ARG, checked even when there is nothing to score. */
int fz_centroid_scores_filter_f32(const int64_t* coff, const int32_t* cdoc, const int64_t* slice_off, const int32_t* pc, const float* ps, int Q,
                                  int Lq, int nprobe, int N, int K, int doc_lo, int doc_hi, int64_t id_base, const float* tau,
                                  float* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream);

/* ---- K2 at corpus scale, storage: residual-compressed token rows (csrc/rerank_residual.hip; ABI 20, additive) ---------------------------
 * 'Residual-compressed token rows'.  A token row t is its centroid id codes[t] (int32, the codes of the candidate stage: the nearest of
 * the K rows of C [K][128] float16) and, per dimension, the nbits-wide number of the bucket its residual falls in, nbits in {2, 4},
 * B = 2^nbits buckets: 4 + 16 nbits bytes per token against 256.
 *   buckets     cutoffs [B - 1] float32, non-decreasing; weights [B] float16.  bucket(r) = the number of cutoffs c with r > c: a residual
 *               equal to a cutoff falls in the LOWER bucket, a NaN residual in bucket 0 (for finite r: torch.bucketize(r, cutoffs)).
 *   compress    r = float32(tok[t][j]) - float32(C[code[t]][j]), one IEEE subtraction; b = bucket(r).
 *   decompress  D[t][j] = the IEEE float16 sum, round to nearest even, denormals kept, of C[code[t]][j] and weights[b].  No
 *               renormalisation: D is a fixed function of the stored bytes.
 *   storage     packed [sumL][16 nbits] uint8, FRAGMENT-MAJOR (part of the ABI): storage position s in 0 .. 127 holds dimension
 *                   32 ((s >> 3) & 3) + 8 (s >> 5) + (s & 7);
 *               positions fill ascending bytes and, inside a byte, ascending bit fields (little-endian).  Lane (row l & 15, group
 *               g = l >> 4) of the v_mfma_f32_16x16x32_f16 A operand so finds all four k-steps of a token -- dimensions 32 ks + 8 g + j
 *               = positions 32 g + 8 ks + j -- in ONE aligned piece of the row: 8 bytes at offset 8 g (nbits = 2), 16 bytes at offset
 *               16 g (nbits = 4).
 *   score       fz_maxsim_pairs_residual_f16 gives, for every slot, exactly what fz_maxsim_pairs_f16 gives on D, bit for bit on any
 *               input: the same MFMA mapping, fmaxf from -inf and summation tree, the same -inf / 0 / clamped-length / last-row rules.
 * A stored code outside [0, K) is clamped into it by every kernel here (no address leaves the table whatever the bytes are); callers
 * validate the code range once, when an index is built.  All three are streaming / gather kernels without workspace.
 * fz_residual_compress_f16: packs rows 0 .. n-1 of tok [n][128] float16 with their codes [n] -> packed [n][16 nbits].
 * fz_residual_decompress_f16: rows [row_lo, row_hi) of a shard of sumL rows -> out [row_hi - row_lo][128] float16 (packed and codes are
 * the shard's arrays, indexed by the shard's row; out starts at row_lo): exports part of a shard, and is what the tests compare against.
 * fz_maxsim_pairs_residual_f16: Doff, sumL, max_doc_len, Q, Lq, N, dim, cand, ldc, cand_len, k, id_base, scores and lds as in
 * fz_maxsim_pairs_f16, with (packed, codes, C, weights, K, nbits) in the place of Dtok.
 * Argument checks in fz_maxsim_pairs_f16's order: negative sizes, K < 1, a bad row range, ldc < k, lds < k or a null pointer where a
 * non-empty tensor is needed -> FZ_ERR_ARG; dim != 128, nbits outside {2, 4}, Lq outside {32, 64, 128}, tok / packed / C / Qtok / out
 * not 16-byte aligned, max_doc_len > 16384 -> FZ_ERR_UNSUPPORTED; nothing to do (n == 0, an empty row range, Q == 0 or k == 0) -> FZ_OK
 * with nothing launched. */
int fz_residual_compress_f16(const void* tok, const int32_t* codes, const void* C, const float* cutoffs, int64_t n, int K, int dim, int nbits,
                             void* packed, void* stream);
int fz_residual_decompress_f16(const void* packed, const int32_t* codes, const void* C, const void* weights, int64_t sumL, int64_t row_lo,
                               int64_t row_hi, int K, int dim, int nbits, void* out, void* stream);
int fz_maxsim_pairs_residual_f16(const void* Qtok, const void* packed, const int32_t* codes, const void* C, const void* weights, int K,
                                 int nbits, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N, int dim,
                                 const int64_t* cand, int ldc, const int32_t* cand_len, int k, int64_t id_base, float* scores, int lds,
                                 void* stream);

/* ---- K1 / A3 at corpus scale: single-vector scores of candidate lists (csrc/pairs.hip; ABI 20, additive) -----------------------------------
 * What fz_maxsim_pairs_f16 is to ColBERT, for DPR and SPLADE: every query against ITS OWN candidate list, no [Q][N] plane, so that the
 * top-k lists of several systems can be completed -- every system scores the union of the candidates -- before they are fused.
 * cand [Q][ldc] int64 global ids, cand_len [Q] int32 (NULL: W for every row), id_base = global id of this shard's document 0 (any
 * int64), out [Q][ldo] float32: the slot rules of fz_maxsim_pairs_f16.  out[q][r] = -inf when r >= cand_len[q], when the id is negative
 * or when its position falls outside [0, N); columns W .. ldo-1 are left untouched; duplicate ids are scored independently.  No
 * workspace, no atomics, no host synchronisation.
 * fz_dot_pairs_f32: out[q][r] = <Qn[q], Dn[cand[q][r] - id_base]> with the BITS of fz_dot_scores_f32's scores[q][cand[q][r] - id_base]:
 * the tile stream's chain of fused multiply-adds from +0.0 in its k order (k-tiles of 32, their count rounded up to even, zeros past d;
 * inside a group of 8: 0, 4, 1, 5, 2, 6, 3, 7), on v_mfma_f32_4x4x1_16b_f32.  Qn [Q][ldq], Dn [N][ldd] float32, 16-byte aligned rows.
 * Checks, in this order: a negative size, d <= 0, ldq < d, ldd < d, ldc < W, ldo < W or a null pointer where a non-empty tensor is
 * needed -> FZ_ERR_ARG; d % 4, ldq % 4, ldd % 4, d > 16384 or Qn / Dn not 16-byte aligned -> FZ_ERR_UNSUPPORTED; Q == 0 or W == 0 ->
 * FZ_OK with nothing launched.
 * fz_sparse_dot_pairs_f32: out[q][r] = fz_sparse_dot_f32's scores[q][cand[q][r] - id_base], bit for bit: acc = acc + qw * pw from +0.0
 * over the query's terms in ascending order (one rounding per product and per add), a term whose postings do not hold the document
 * skipped (binary search); a document of the shard that shares no term with the query scores +0.0.  toff / pdoc / pw and qoff / qterms /
 * qw as in fz_sparse_dot_f32 (no slice table).  Checks: a negative size, ldc < W, ldo < W or a null pointer (qoff, cand, out; toff when
 * N > 0) where a non-empty tensor is needed -> FZ_ERR_ARG; Q == 0 or W == 0 -> FZ_OK with nothing launched. */
int fz_dot_pairs_f32(const float* Qn, int ldq, const float* Dn, int ldd, int Q, int N, int d, const int64_t* cand, int ldc,
                     const int32_t* cand_len, int W, int64_t id_base, float* out, int ldo, void* stream);
int fz_sparse_dot_pairs_f32(const int64_t* toff, const int32_t* pdoc, const float* pw, const int64_t* qoff, const int32_t* qterms,
                            const float* qw, int Q, int N, const int64_t* cand, int ldc, const int32_t* cand_len, int W, int64_t id_base,
                            float* out, int ldo, void* stream);

/* ---- pair scores from a FORWARD (document-major) index (csrc/forward.hip; ABI 20, additive) ------------------------------------------------
 * A pair's score is a question about one document, and the forward index holds a document's postings as one contiguous row: foff [N + 1]
 * int64 row offsets, terms ascending inside a row (a stable sort of the inverted postings by document: ops.forward_index).
 * fz_sparse_fwd_pairs_f32: fz_sparse_dot_pairs_f32 with (foff, rows, V) in the place of (toff, pdoc, pw): rows [nnz] of 8-byte
 * {int32 term, float32 weight} postings (8-byte aligned), V the vocabulary size.  out[q][r] equals fz_sparse_dot_pairs_f32's BITS in every
 * slot -- the row walk meets the terms query and document share in the same ascending order, acc = acc + qw * w from +0.0 -- with the same
 * -inf rules; columns W .. ldo-1 are left untouched.  The query's term set is a bitmap over V in LDS, with the count of set bits before
 * each word next to it (a term's place in the query's list is the number of set bits below it: qterms strictly ascending and inside
 * [0, V), as fz_sparse_dot_f32 takes them): V > fz_sparse_fwd_max_vocab() (at least 65,536) is not built; a query may hold any number
 * of terms.  No workspace, no atomics on global memory, no host synchronisation.  Checks, in this order: a negative size, ldc < W, ldo < W or a null pointer (qoff, cand, out; foff when N > 0) where a
 * non-empty tensor is needed -> FZ_ERR_ARG; V beyond the cap or rows not 8-byte aligned -> FZ_ERR_UNSUPPORTED; Q == 0 or W == 0 -> FZ_OK
 * with nothing launched.
 * fz_tfidf_doc_scores_fwd_f64 / fz_bm25_doc_scores_fwd_pv_f64: fz_tfidf_doc_scores_f64 / fz_bm25_doc_scores_pv_f64 with the forward index
 * next to the inverted tables: fterm [nnz] int32 the rows' terms, fpos [nnz] int32 each posting's place e in the inverted arrays (ptf[e],
 * pval[e]).  The same chain -- query order, terms not de-duplicated, -1 adds nothing, acc = acc + term from 0.0 -- and so the same bits;
 * the binary search per query term runs in the document's row, not in the term's posting list.  toff and pdoc are accepted and not
 * read.  Checks: Q < 0, N < 0, G < 1 or (Q > 0) a null pointer among the tables read -> FZ_ERR_ARG; Q == 0 -> FZ_OK. */
int fz_sparse_fwd_max_vocab(void);
int fz_sparse_fwd_pairs_f32(const int64_t* foff, const void* rows, int V, const int64_t* qoff, const int32_t* qterms, const float* qw, int Q,
                            int N, const int64_t* cand, int ldc, const int32_t* cand_len, int W, int64_t id_base, float* out, int ldo,
                            void* stream);
int fz_tfidf_doc_scores_fwd_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* foff,
                                const int32_t* fterm, const int32_t* fpos, const int64_t* qoff, const int32_t* qterms, int Q, int N,
                                const int32_t* docs, int G, double* out, void* stream);
int fz_bm25_doc_scores_fwd_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* foff, const int32_t* fterm,
                                  const int32_t* fpos, const int64_t* qoff, const int32_t* qterms, int Q, int N, const int32_t* docs, int G,
                                  double* out, void* stream);

/* ---- pseudo-relevance feedback: query expansion from top-k lists (csrc/feedback.hip; ABI 20, additive) -------------------------------------
 * Rocchio: q' = alpha * q + sum_r coef[q][r] * d_r over the feedback slots r = 0 .. F-1 of query q, IN SLOT ORDER.  fb_ids [Q][ldf] int64
 * global ids, fb_len [Q] int32 (NULL: F for every query; clamped to [0, F]), coef [Q][ldc] float32, id_base = global id of this index's
 * document 0 (any int64).  A slot is SKIPPED when r >= fb_len[q], fb_ids[q][r] < id_base or fb_ids[q][r] >= id_base + N; the same document
 * in two slots is added twice.  Every product and every add is rounded to float32 once, nothing is fused, and the contributions to one term
 * (dimension) are added in slot order: the bits are defined and two calls give the same bytes.  Weights are finite by contract.
 * fz_sparse_feedback_f32: queries as weighted sparse rows (qoff [Q + 1] int64, qterms int32 unique and ascending inside [0, V), qw float32),
 * documents as the forward rows of fz_sparse_fwd_pairs_f32 (foff [N + 1], rows of 8-byte {int32 term, float32 weight}, terms unique in a row).
 *   1. acc[t] = +0.0 for all t; per query term (t, w): acc[t] = acc[t] + alpha * w, t marked a QUERY term;
 *   2. per counted slot, per posting (t, w) of its document: acc[t] = acc[t] + coef[q][r] * w, t marked TOUCHED;
 *   3. the candidates are the touched terms that are no query terms (a sum that came out as 0 included), ranked by desc_key_f32(acc[t])
 *      ascending -- larger sums first, -0.0 == +0.0 --, ties by ascending term; the first min(m, #candidates) are kept;
 *   4. out_terms [Q][ldo] int32 / out_w [Q][ldo] float32: the query terms and the kept candidates in ascending term order with their
 *      acc[t] bits, out_len[q] of them; columns out_len[q] .. width-1 hold (-1, +0.0).  The kernel writes all `width` columns of every
 *      row and nothing else (no pre-fill is needed).  A row that does not fit `width` is cut there and raises bit 0 of *flag (a device
 *      int32 the call zeroes first).
 *   One workgroup per query; the accumulator is a float32 array over the vocabulary in LDS: V <= fz_sparse_feedback_max_vocab() = 32,768.
 *   Checks, all before the first HIP call: a negative Q / N / F / m / width, ldf < F, ldc < F, ldo < width, V <= 0, V beyond the cap, or
 *   (Q > 0) a null pointer among qoff, out_len, flag, fb_ids / coef (F > 0), out_terms / out_w (width > 0), foff (F > 0 and N > 0)
 *   -> FZ_ERR_ARG; rows not 8-byte aligned -> FZ_ERR_UNSUPPORTED; Q == 0 -> FZ_OK, nothing launched, nothing written.
 * fz_dense_feedback_f32: out[q][j] = alpha * Qn[q][j], then per counted slot out[q][j] = out[q][j] + coef[q][r] * Dn[d][j]; Qn [Q][ldq],
 *   Dn [N][ldd], out [Q][ldo] float32, j < dim (columns dim .. ldo-1 are left untouched); not normalised.  Any strides and alignments are
 *   taken (16-byte vector accesses where ldq, ldd, ldo are multiples of 4 and the three pointers 16-byte aligned).  Checks: a negative
 *   Q / N / F, dim <= 0, ldf < F, ldc < F, ldq / ldd / ldo < dim, or (Q > 0) a null pointer among Qn, out, fb_ids / coef (F > 0),
 *   Dn (F > 0 and N > 0) -> FZ_ERR_ARG; Q == 0 -> FZ_OK.  No workspace, no atomics, no host synchronisation. */
int fz_sparse_feedback_max_vocab(void);
int fz_sparse_feedback_f32(const int64_t* foff, const void* rows, int V, int64_t N, int64_t id_base, const int64_t* qoff, const int32_t* qterms,
                           const float* qw, int Q, const int64_t* fb_ids, int ldf, const int32_t* fb_len, const float* coef, int ldc, int F,
                           float alpha, int m, int32_t* out_terms, float* out_w, int ldo, int width, int32_t* out_len, int32_t* flag,
                           void* stream);
int fz_dense_feedback_f32(const float* Qn, int ldq, const float* Dn, int ldd, int Q, int64_t N, int dim, int64_t id_base,
                          const int64_t* fb_ids, int ldf, const int32_t* fb_len, const float* coef, int ldc, int F, float alpha, float* out,
                          int ldo, void* stream);

/* ---- lexical feedback: weighted posting walks and expansion terms in float64 (csrc/bm25_weighted.hip, csrc/feedback_lexical.hip; ABI 20, additive) ----
 * The weighted walks: the four range entries above (plane and filter, both modes) for queries whose every entry carries a float64 weight,
 * qw [one per entry of qterms] after qterms, every other argument and check as in the unweighted entry (qw among the pointers).  Per
 * document the chain, in entry order j, of acc = acc + qw[j] * val(t_j, d) from +0.0, val(t, d) the unweighted walk's own term for that
 * posting (pval[p], or (double)ptf[p] * idf[t], rounded before the product with qw[j]); an entry with t_j < 0 adds nothing.  With qw all
 * 1.0 the results are the unweighted entries', bit for bit.  fz_lexical_weighted_terms(tfidf): the entries resolved per batch (256 / 128);
 * the batch only groups the entries, the bits do not depend on it. */
int fz_lexical_weighted_terms(int tfidf);
int fz_bm25_scores_range_w_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                  const int32_t* qterms, const double* qw, int Q, int N, int doc_lo, int doc_hi, double* scores, int lds,
                                  void* stream);
int fz_tfidf_scores_range_w_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                const int64_t* qoff, const int32_t* qterms, const double* qw, int Q, int N, int doc_lo, int doc_hi,
                                double* scores, int lds, void* stream);
int fz_bm25_filter_w_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                            const int32_t* qterms, const double* qw, int Q, int N, int doc_lo, int doc_hi, int64_t id_base, const double* tau,
                            double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream);
int fz_tfidf_filter_w_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                          const int64_t* qoff, const int32_t* qterms, const double* qw, int Q, int N, int doc_lo, int doc_hi, int64_t id_base,
                          const double* tau, double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow,
                          void* stream);
/* Expansion terms from feedback lists (fb_ids / fb_len / coef / N / id_base and the slot rules as for fz_sparse_feedback_f32; coef is
 * widened exactly to float64).  Rows: document d's entries [foff[d], foff[d+1]) of fterm (int32, unique inside a row) with the value
 * val(t, d) = pval[fpos[e]] (fz_bm25_feedback_pv_f64), (double)ptf[fpos[e]] * idf[fterm[e]] (fz_tfidf_feedback_f64) or fval[e]
 * (fz_lexical_feedback_rows_f64).  Queries: qoff [Q + 1] int64, qterms int32 with repetitions and -1 entries.
 *   1. capacity: slots are counted in order while the running sum of their row lengths stays within fz_lexical_feedback_max_entries()
 *      (4,096); the first slot that would pass it is skipped with every later slot of the query, and bit 0 of *flag is raised;
 *   2. per counted slot r in order, per entry (t, val) of its row: w[t] = w[t] + coef[q][r] * val, from +0.0; product and add are rounded
 *      once each; a term's additions are made in slot order;
 *   3. candidates: w[t] > 0 and t not among the query's terms; selected: the min(m, #candidates) of largest w, ties to the lower term;
 *   4. out_terms [Q][ldo] int32 / out_w [Q][ldo] float64: the query's entries in their order (repetitions and -1 kept) at weight alpha,
 *      then the selected terms in selection order at beta * (w[t] / w_max), w_max the first selected term's w (the division is rounded,
 *      then the product); out_len[q] entries, columns out_len[q] .. width-1 hold (-1, +0.0).  The kernel writes all `width` columns of
 *      every row and nothing else.  width >= longest query + m by contract; a row that does not fit is cut and raises bit 1 of *flag
 *      (a device int32 the call zeroes first).
 * One workgroup per query; the sums live in an LDS hash table keyed by term, so the vocabulary's size does not matter.  No float atomics:
 * two calls give the same bytes.  Checks, before the first HIP call: a negative Q / N / F / m / width, ldf < F, ldc < F, ldo < width ->
 * FZ_ERR_ARG; Q == 0 -> FZ_OK, nothing launched; then a null pointer among qoff, out_len, flag, fb_ids / coef (F > 0), out_terms / out_w
 * (width > 0), foff (F > 0 and N > 0) -> FZ_ERR_ARG. */
int fz_lexical_feedback_max_entries(void);
int fz_bm25_feedback_pv_f64(const int64_t* foff, const int32_t* fterm, const int32_t* fpos, const double* pval, int64_t N, int64_t id_base,
                            const int64_t* qoff, const int32_t* qterms, int Q, const int64_t* fb_ids, int ldf, const int32_t* fb_len,
                            const float* coef, int ldc, int F, double alpha, double beta, int m, int32_t* out_terms, double* out_w, int ldo,
                            int width, int32_t* out_len, int32_t* flag, void* stream);
int fz_tfidf_feedback_f64(const int64_t* foff, const int32_t* fterm, const int32_t* fpos, const int32_t* ptf, const double* idf, int64_t N,
                          int64_t id_base, const int64_t* qoff, const int32_t* qterms, int Q, const int64_t* fb_ids, int ldf,
                          const int32_t* fb_len, const float* coef, int ldc, int F, double alpha, double beta, int m, int32_t* out_terms,
                          double* out_w, int ldo, int width, int32_t* out_len, int32_t* flag, void* stream);
int fz_lexical_feedback_rows_f64(const int64_t* foff, const int32_t* fterm, const double* fval, int64_t N, int64_t id_base,
                                 const int64_t* qoff, const int32_t* qterms, int Q, const int64_t* fb_ids, int ldf, const int32_t* fb_len,
                                 const float* coef, int ldc, int F, double alpha, double beta, int m, int32_t* out_terms, double* out_w,
                                 int ldo, int width, int32_t* out_len, int32_t* flag, void* stream);

/* ---- cross-encoder pairs assembled from token ids (csrc/crosspack.hip; ABI 20, additive) ---------------------------------------------------
 * The monoBERT rerank (hybrid.py:139-163) over top-k lists: the pair rows "<s> q </s></s> d </s>" of the packed forward are built on the
 * device from the queries' token ids and a token store of the corpus, sharded by document: tok [sumL] int32, Doff [N + 1] int64 (document d
 * of the shard = global id id_base + d holds the first Doff[d+1] - Doff[d] plain tokens of its text, no specials), doc_full_len [N] int32
 * or NULL: the documents' plain lengths before the store cut them (NULL: nothing was cut).  cand / ldc / cand_len / id_base: the slot
 * rules of fz_maxsim_pairs_f16 -- a slot is this shard's iff r < cand_len[q] and 0 <= cand[q][r] - id_base < N, the subtraction in 64 bits.
 * The pair rule, with B = max_length - (2 + nsep) and lq = qlen[q] (the query's plain length before any cut), ld the document's:
 *   FZ_PAIR_LONGEST_FIRST  the `tokenizers` library's longest_first: lq + ld <= B keeps both; else n1 = min(lq, ld), n2 = max(n1, B - n1),
 *                          and if n1 + n2 > B still, n1 = B / 2, n2 = n1 + B % 2; the STRICTLY longer sequence keeps n2 (a tie: the
 *                          document).  The row is bos, query, nsep separators, document, eos.
 *   FZ_PAIR_TAIL           the row is bos + (query ++ nsep separators ++ document)[: max_length - 2] + eos: the separators are ordinary
 *                          tokens and are cut before the document is.
 * A kept count never exceeds what is stored (Lq columns of qtok, the document's stored tokens).
 * fz_pair_plan: one thread per slot; kq / kd / L [Q][W] int32 (contiguous): the kept query and document tokens and the pair's row count
 * L = 2 + kq + separators + kd; all three 0 for a slot that is not this shard's, for which nothing is read.  Checks, in this order: a
 * negative size, ldc < W, an unknown mode, max_length < 2 + nsep or a null pointer (cand, qlen, kq, kd, L; Doff when N > 0) where a
 * non-empty tensor is needed -> FZ_ERR_ARG; nsep > fz_pair_max_sep() (2) or Q * W >= 2^31 -> FZ_ERR_UNSUPPORTED; Q == 0 or W == 0 ->
 * FZ_OK with nothing launched.
 * fz_pair_fill: the packed rows of ONE forward sub-batch: pairs [P] int32 flat slots q * W + r in forward order, cu_rows [P + 1] int32
 * with cu_rows[p+1] - cu_rows[p] = L of pair p and cu_rows[P] <= T, kq / kd the plan's planes, qtok [Q][ldq] int32 (Lq columns), the
 * special ids -> ids [T] and pos_ids [T] int64, what fz_embed_layernorm_f32 takes: pos_ids = pad_idx + 1 + column.  One wave per pair.
 * Token type ids are not written (type 0 everywhere).  A pair whose plan does not fit what is stored (slot outside the plane or the shard,
 * kept counts beyond the row or the document) reads nothing and is written as pad_idx tokens at position pad_idx; the caller guarantees
 * that the stored token ids index inside the embedding table.  Checks, in this order: a negative size or special id, ldc < W, ldq < Lq
 * or (P > 0) a null pointer among pairs, cu_rows, kq, kd, cand, Doff, ids / pos_ids (T > 0), qtok (Lq > 0) -> FZ_ERR_ARG; nsep beyond
 * fz_pair_max_sep() or Q * W >= 2^31 -> FZ_ERR_UNSUPPORTED; P == 0 -> FZ_OK with nothing launched.
 * No workspace, no atomics, no host synchronisation. */
#define FZ_PAIR_LONGEST_FIRST 0
#define FZ_PAIR_TAIL 1
int fz_pair_max_sep(void);
int fz_pair_plan(const int64_t* cand, int ldc, const int32_t* cand_len, int Q, int W, int64_t id_base, const int64_t* Doff,
                 const int32_t* doc_full_len, int N, const int32_t* qlen, int Lq, int max_length, int mode, int nsep, int32_t* kq, int32_t* kd,
                 int32_t* L, void* stream);
int fz_pair_fill(const int32_t* pairs, const int32_t* cu_rows, int P, int T, const int32_t* kq, const int32_t* kd, const int64_t* cand, int ldc,
                 int Q, int W, int64_t id_base, const int32_t* qtok, int ldq, int Lq, const int32_t* tok, const int64_t* Doff, int N, int bos,
                 int sep, int eos, int pad_idx, int nsep, int64_t* ids, int64_t* pos_ids, void* stream);

/* ---- encoder side: the per-sequence parts of SentenceTransformer.encode (hybrid.py:97-102) on PACKED token rows -- */
/* Self-attention of a BERT/CamemBERT layer for ragged sequences without padding: for every sequence and head,
 * out = softmax(q k^T * scale) v in fp32 (MFMA products, online softmax over 16-key tiles), scale > 0.  qkv [T][ld] = fused
 * projection rows (q | k | v, each H*head_dim wide); strips [n_strips][4] int32 (device): (first row of the sequence, its
 * length, first query row of this strip of <= 32 queries, 0) -- one entry per 32 queries of every sequence, the strips of a
 * sequence adjacent, sequences in any order (longest first balances best).  head_dim must be 64; sequence length <= 16384.
 * out [T][ldo], H*head_dim wide. */
int fz_attn_varlen_f32(const float* qkv, int ld, const int32_t* strips, int n_strips, int H, int head_dim, float scale,
                       float* out, int ldo, void* stream);
/* Inside the model forward of model.encode(...) (hybrid.py:101-102): every BERT sub-layer ends with
 * out = LayerNorm(x + res) * gamma + beta over the last dimension d (biased variance, as torch.nn.LayerNorm);
 * res nullable.  d % 4 == 0, d <= 4096. */
int fz_add_layernorm_f32(const float* x, int ldx, const float* res, int ldr, const float* gamma, const float* beta, float eps,
                         int rows, int d, float* out, int ldo, void* stream);
/* The FFN activation of the same forward (hybrid.py:101-102):
 * y = 0.5 x (1 + erf(x / sqrt 2)) elementwise (the exact "gelu" of BERT / CamemBERT, torch.nn.functional.gelu), count floats,
 * count % 4 == 0, 16-byte aligned; y may alias x. */
int fz_gelu_f32(const float* x, float* y, size_t count, void* stream);
/* The same three steps for a MIXED-PRECISION forward -- colbert-ai wraps every query() / doc() of the ColBERT encoder in torch.cuda.amp.autocast
 * (requirements.txt:15; the repository's own ColBERT runs set 'amp': True, multi_dense_biencoder.py:55, and wrap the model in amp.context(),
 * colbert_ir.py:110,124): the Linears take and return float16, these kernels compute in float32 and hand the next Linear its float16 operand.
 *   fz_attn_varlen_f16:       as fz_attn_varlen_f32 with float16 fused-QKV rows in and float16 context rows out (8-byte aligned, ld / ldo in
 *                             elements); scores, softmax and the weighted sum are float32;
 *   fz_attn_varlen_f16_amp:   the same rows in and out, but q k^T and p v as float16 matmuls with float32 accumulation (v_mfma_f32_16x16x32_f16 /
 *                             16x16x16_f16) around a float32 softmax -- the arithmetic autocast gives the attention of a BERT layer; ld and ldo
 *                             multiples of 8 elements, 16-byte aligned rows;
 *   fz_add_layernorm_x16:     x float16 (a Linear's output), res / out float32 (the residual stream), out16 nullable: a float16 copy of out;
 *   fz_gelu_f16:              float16 in and out (float32 arithmetic, as torch.nn.functional.gelu on a float16 tensor), count % 8 == 0. */
int fz_attn_varlen_f16(const void* qkv /* float16 */, int ld, const int32_t* strips, int n_strips, int H, int head_dim, float scale,
                       void* out /* float16 */, int ldo, void* stream);
int fz_attn_varlen_f16_amp(const void* qkv /* float16 */, int ld, const int32_t* strips, int n_strips, int H, int head_dim, float scale,
                           void* out /* float16 */, int ldo, void* stream);
int fz_add_layernorm_x16(const void* x /* float16 */, int ldx, const float* res, int ldr, const float* gamma, const float* beta, float eps,
                         int rows, int d, float* out, int ldo, void* out16 /* float16, nullable */, int ldo16, void* stream);
int fz_gelu_f16(const void* x /* float16 */, void* y /* float16 */, size_t count, void* stream);
/* The embedding block of the same forward (hybrid.py:101-102) on packed rows: out[t] = LayerNorm(word[ids[t]] + pos[pos_ids[t]] + type0) * gamma + beta.
 * word [V][d], pos [Pmax][d], type0 [d] (token type 0 everywhere); ids / pos_ids [rows] int64 (device), the caller guarantees they
 * index inside the tables.  d % 4 == 0, d <= 4096. */
int fz_embed_layernorm_f32(const float* word, const float* pos, const float* type0, const int64_t* ids, const int64_t* pos_ids,
                           const float* gamma, const float* beta, float eps, int rows, int d, float* out, int ldo, void* stream);
/* mean Pooling (sentence_transformers Pooling(mean)): out[b] = mean of rows [cu_rows[b], cu_rows[b+1]) of x; zeros for an
 * empty sequence.  cu_rows [B+1] int32 (device). */
int fz_segment_mean_f32(const float* x, int ldx, const int32_t* cu_rows, int B, int d, float* out, int ldo, void* stream);
/* SPLADE-max pooling (splade/splade.py:88-99: amax over the tokens of log1p(relu(logits))): out[b] = log1p(relu(max of the
 * rows [cu_rows[b], cu_rows[b+1]) of x)) -- the same value, log1p o relu being monotone; 0 for an empty sequence. */
int fz_segment_splade_max_f32(const float* x, int ldx, const int32_t* cu_rows, int B, int d, float* out, int ldo, void* stream);

/* The SPLADE head with the pooling as its epilogue (splade/splade.py:88-99 over the MLM decoder): pool[s][v] = max over the packed rows
 * t in [cu_rows[s], cu_rows[s+1]) of log1p(relu(<X[t], W[v]> + bias[v])) -- the same value as fz_segment_splade_max_f32 over the decoder's
 * logits, but the [T][V] logits (4.2 GB per 64 x 512-token batch, splade.py:94) are never written: the fp32-MFMA tile stream of
 * fz_dot_scores_f32 with a segment-max / atomicMax epilogue.  X [T][ldx] packed hidden rows (after the head's dense + GELU + LayerNorm), W [V][ldw]
 * the decoder weight, bias [V]; pool [nseq][ldp] MUST be zero on entry (0 = log1p(relu(x)) of every x <= 0 and of an empty sequence).
 * d % 4 == 0, 16-byte aligned rows. */
int fz_splade_head_max_f32(const float* X, int ldx, const float* W, int ldw, const float* bias, const int32_t* cu_rows, int nseq, int T, int V,
                           int d, float* pool, int ldp, void* stream);
/* (ABI 20, additive) The same head for the mixed-precision encoders: X16 [T][ldx] and W16 [V][ldw] are float16, the products are accumulated in
 * float32 on the matrix pipe (v_mfma_f32_32x32x16_f16: a product of two float16 values is exact in float32), bias and pool are float32, pool
 * MUST be zero on entry, and no [T][V] plane is written.  The contract of fz_splade_head_max_f32 with one change: d, ldx and ldw must be
 * multiples of 8 and both operand pointers 16-byte aligned (anything else: FZ_ERR_UNSUPPORTED); every argument is judged on the host, in that
 * entry's order, before anything touches the device.  Hidden values are finite by contract: the float16 encoder path lives with the float16
 * range already, and an infinity or NaN in X16 or W16 pools to an unspecified value. */
int fz_splade_head_max_f16(const void* X16, int ldx, const void* W16, int ldw, const float* bias, const int32_t* cu_rows, int nseq, int T, int V,
                           int d, float* pool, int ldp, void* stream);
/* (host only, no HIP call) the tile constants of fz_splade_head_max_f16: output tile rows x cols, the k-tile and the MFMA k-step in halves */
int fz_splade_head_f16_tile(int* rows, int* cols, int* ktile, int* kstep);

/* ---- small utilities ------------------------------------------------------------------ */
int fz_fill_i32(int32_t* p, size_t count, int32_t value, void* stream);
int fz_f64_to_f32(const double* src, float* dst, size_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FUSION_HIP_H */
