// feedback_lexical.hip -- pseudo-relevance feedback for the lexical models (BM25 / AtireBM25 / TF-IDF): expansion terms from a query's own
// top-k list, in float64 (gfx950).  What csrc/feedback.hip's sparse kernel is to SPLADE -- but a word-level vocabulary has millions of
// terms, so the accumulator is not an array over the vocabulary: it is an open-addressing table in LDS keyed by term id.
//
// The arithmetic ('Lexical feedback').  val(t, d) is what the posting walk adds for that posting: pval[p] ('pv'), or
// (double)ptf[p] * idf[t] ('tfidf'), or the row's own value (rows source).  Slot r of query q counts when r < fb_len[q] and its id is one
// of the index's N documents (id_base ..); the same document in two slots counts twice.  Capacity: slots are taken in order while the
// running sum of their row lengths stays within FL_E; the first slot that would pass it is skipped with every later one, bit 0 of the
// flag word is raised.  For every term of a counted row, in slot order: w[t] = w[t] + coef[q][r] * val(t, d_r) from +0.0 (coef widened
// exactly; product and add rounded once each, -ffp-contract=off).  Candidates: w[t] > 0 and t not among the query's terms.  Selected: the
// min(m, C) candidates of largest w, ties to the lower term, emitted in that order after the query's own entries:
//   out row = [the query's entries in their order (repetitions and -1 kept), weight alpha | selected t, weight beta * (w[t] / w_max)],
// w_max the first selected term's w; the division is rounded, then the product.  Columns out_len[q] .. width-1 hold (-1, +0.0).
//
// ONE 1,024-THREAD WORKGROUP PER QUERY.  LDS (102 KiB, dynamic; one workgroup per CU): table [2 FL_E] int32 term per cell (-1: empty;
// lists.h's hash, linear probing, at most half full: a counted row brings at most its length in new terms and the lengths sum to <=
// FL_E), acc [2 FL_E] float64 next to it cell by cell, a "query term" bit per cell, and the offsets, lengths and coefficients of 256
// slots.  A term's cell depends on the arrival order of the inserts; its sum does not, and cells are never emitted: two runs give the
// same bytes.
//   1. slots in batches of FL_SLOTS: thread i resolves slot i (id -> document -> row offsets: two dependent reads for all slots at once),
//      a block scan of the lengths applies the capacity rule.
//   2. thread i takes posting i (+ 1,024 j) of a slot's row: compare-and-swap the term into its cell (integer LDS atomic), then a plain
//      read-modify-write of the cell's sum -- a row's terms are unique, so a cell has one writer per slot -- and a barrier between slots
//      keeps the slot order.  The first 1,024 postings of FL_U rows (term, position, value: three dependent reads) are in flight ahead
//      of their adds.  No float atomics.
//   3. the query's terms are looked up (read only) and their cells marked.
//   4. the candidates' (desc_key_f64(w), term) pairs are compacted -- from registers, over the accumulator's own LDS -- and sorted
//      ascending by a bitonic network over the next power of two >= C (C <= FL_E); the first min(m, C) are the selection.
#include "lists.h"

namespace fz {

constexpr int FL_T = 1024;                 // threads = postings per row chunk
constexpr int FL_NW = FL_T / 64;
constexpr int FL_E = 4096;                 // fz_lexical_feedback_max_entries(): counted row entries per query
constexpr int FL_TABLE = 2 * FL_E;         // cells: a power of two, at most half full
constexpr int FL_OWN = FL_TABLE / FL_T;    // cells a thread reads in step 4
constexpr int FL_SLOTS = 256;              // slots resolved at a time
constexpr int FL_U = 3;                    // rows whose first postings are in flight together (4: the rows source spills 2 SGPRs)
constexpr int32_t FL_EMPTY = -1;
constexpr int32_t FL_CUT = 1;              // flag bit 0: the capacity rule skipped slots
constexpr int32_t FL_NOFIT = 2;            // flag bit 1: a row did not fit `width` (a caller's error: width >= query length + m)
enum { FL_SRC_PV = 0, FL_SRC_TFIDF = 1, FL_SRC_ROWS = 2 };
constexpr size_t FL_LDS = (size_t)FL_TABLE * 8 + (size_t)FL_TABLE * 4 + FL_SLOTS * (8 + 8 + 4) + FL_TABLE / 8 + FL_NW * 4;
static_assert(FL_LDS <= 160 * 1024 && FL_E >= 4096 && FL_E <= 8192, "one CU's LDS");
static_assert((size_t)FL_E * (8 + 4) <= (size_t)FL_TABLE * 8, "the sort's pairs lie over the accumulator");

struct LexFbArgs {
    const int64_t* fb_ids; const int32_t* fb_len; const float* coef;   // [Q][ldf], [Q] or null (= F), [Q][ldc]
    int64_t N, id_base;
    int F, ldf, ldc;
    const int64_t* foff; const int32_t* fterm;                         // row of document d: entries [foff[d], foff[d+1]), terms unique
    const int32_t* fpos; const double* pval; const int32_t* ptf; const double* idf;   // index sources: the entry's posting, its value
    const double* fval;                                                // rows source: the entry's value
    const int64_t* qoff; const int32_t* qterms;
    int32_t* out_terms; double* out_w; int32_t* out_len; int32_t* flag;
    int ldo, width, m;
    double alpha, beta;
};

// exclusive prefix of v over the workgroup's threads and the total; two barriers: wtot is free again on return
__device__ __forceinline__ uint32_t fl_block_scan(uint32_t v, uint32_t* wtot, int lane, int wv, uint32_t& total) {
    const uint32_t incl = wave_incl_scan_u32(v, lane);
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    uint32_t woff = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < FL_NW; ++i) { const uint32_t c = wtot[i]; if (i < wv) woff += c; total += c; }
    __syncthreads();
    return woff + incl - v;
}

template <int SRC>
__device__ __forceinline__ void fl_load(const LexFbArgs& a, int64_t e, int& term, double& val) {
    term = a.fterm[e];
    if constexpr (SRC == FL_SRC_ROWS) val = a.fval[e];
    else if constexpr (SRC == FL_SRC_PV) val = a.pval[a.fpos[e]];
    else val = term >= 0 ? (double)a.ptf[a.fpos[e]] * a.idf[term] : 0.0;   // the walk's own product, rounded
}

// w[term] = w[term] + x; a term's first add starts from +0.0.  One writer per term between two barriers.
__device__ __forceinline__ void fl_add(int32_t* table, double* acc, int term, double x) {
    for (uint32_t h = lj_hash(term, FL_TABLE - 1);; h = (h + 1) & (FL_TABLE - 1)) {
        const int32_t old = atomicCAS(&table[h], FL_EMPTY, term);
        if (old == FL_EMPTY) { acc[h] = 0.0 + x; return; }
        if (old == term) { acc[h] = acc[h] + x; return; }
    }
}

template <int SRC>
__global__ __launch_bounds__(FL_T) void lexical_feedback_kernel(LexFbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fl_smem[];
    double* const acc = reinterpret_cast<double*>(fl_smem);                       // [FL_TABLE]
    int32_t* const table = reinterpret_cast<int32_t*>(acc + FL_TABLE);            // [FL_TABLE]
    int64_t* const s_start = reinterpret_cast<int64_t*>(table + FL_TABLE);        // [FL_SLOTS]
    double* const s_coef = reinterpret_cast<double*>(s_start + FL_SLOTS);         // [FL_SLOTS]
    int* const s_len = reinterpret_cast<int*>(s_coef + FL_SLOTS);                 // [FL_SLOTS]
    uint32_t* const marks = reinterpret_cast<uint32_t*>(s_len + FL_SLOTS);        // [FL_TABLE / 32]
    uint32_t* const wtot = marks + FL_TABLE / 32;                                 // [FL_NW]
    uint64_t* const skey = reinterpret_cast<uint64_t*>(fl_smem);                  // [FL_E], step 4: over acc
    int32_t* const sterm = reinterpret_cast<int32_t*>(skey + FL_E);               // [FL_E]
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;

    for (int i = t; i < FL_TABLE; i += FL_T) table[i] = FL_EMPTY;
    if (t < FL_TABLE / 32) marks[t] = 0u;

    // 1 + 2. the feedback documents, slot after slot
    const int flen = a.N > 0 ? (a.fb_len ? min(max(a.fb_len[q], 0), a.F) : a.F) : 0;
    uint32_t base = 0;                                             // entries counted so far (<= FL_E)
    bool cut = false;
    for (int s0 = 0; s0 < flen && !cut; s0 += FL_SLOTS) {          // block-uniform
        int64_t st = 0; int len = 0; double c = 0.0;
        if (t < FL_SLOTS && s0 + t < flen) {
            const int64_t id = a.fb_ids[(size_t)q * a.ldf + s0 + t];
            const uint64_t d = (uint64_t)id - (uint64_t)a.id_base;
            c = (double)a.coef[(size_t)q * a.ldc + s0 + t];
            if (id >= a.id_base && d < (uint64_t)a.N) {
                st = a.foff[d];
                len = (int)min(max(a.foff[d + 1] - st, (int64_t)0), (int64_t)FL_E + 1);   // (beyond FL_E: never counted)
            }
        }
        uint32_t tot;
        const uint32_t before = fl_block_scan((uint32_t)len, wtot, lane, wv, tot);     // (its barriers close the clears above)
        if (t < FL_SLOTS) {
            s_start[t] = st; s_coef[t] = c;
            s_len[t] = base + before + (uint32_t)len <= (uint32_t)FL_E ? len : 0;     // the prefix only grows: what follows a cut is cut
        }
        cut = base + tot > (uint32_t)FL_E;
        base += tot;
        __syncthreads();
        const int nb = min(flen - s0, FL_SLOTS);
        for (int r0 = 0; r0 < nb; r0 += FL_U) {                    // FL_U rows' first 1,024 entries in flight, added in slot order
            int pt[FL_U]; double pv[FL_U];
#pragma unroll
            for (int u = 0; u < FL_U; ++u) {
                pt[u] = -1; pv[u] = 0.0;
                if (r0 + u < nb && t < s_len[r0 + u]) fl_load<SRC>(a, s_start[r0 + u] + t, pt[u], pv[u]);
            }
#pragma unroll
            for (int u = 0; u < FL_U; ++u) {
                if (r0 + u >= nb) continue;                        // block-uniform
                const int rl = s_len[r0 + u];
                if (rl == 0) continue;                             // block-uniform: nothing written, no barrier owed
                const double cf = s_coef[r0 + u];
                if (pt[u] >= 0) fl_add(table, acc, pt[u], cf * pv[u]);
                for (int k = t + FL_T; k < rl; k += FL_T) {        // a row of more than 1,024 entries
                    int term; double val;
                    fl_load<SRC>(a, s_start[r0 + u] + k, term, val);
                    if (term >= 0) fl_add(table, acc, term, cf * val);
                }
                __syncthreads();                                   // this slot's adds are in before the next slot's read them
            }
        }
    }
    __syncthreads();

    // 3. the query's own terms: their cells are no candidates
    const int64_t q0 = a.qoff[q], nq = a.qoff[q + 1] - q0;
    for (int64_t p = t; p < nq; p += FL_T) {
        const int term = a.qterms[q0 + p];
        if (term < 0) continue;
        for (uint32_t h = lj_hash(term, FL_TABLE - 1);; h = (h + 1) & (FL_TABLE - 1)) {
            const int32_t v = table[h];
            if (v == FL_EMPTY) break;
            if (v == term) { atomicOr(&marks[h >> 5], 1u << (h & 31)); break; }
        }
    }
    __syncthreads();

    // 4. the candidates, compacted and sorted by (w descending, term ascending)
    uint64_t ck[FL_OWN]; int ct[FL_OWN];
    uint32_t ism = 0u;
#pragma unroll
    for (int i = 0; i < FL_OWN; ++i) {
        const int h = t + i * FL_T;
        ct[i] = table[h];
        const double w = ct[i] != FL_EMPTY ? acc[h] : 0.0;
        const bool is = !((marks[h >> 5] >> (h & 31)) & 1u) && w > 0.0;
        ck[i] = desc_key_f64(w);
        ism |= (is ? 1u : 0u) << i;
    }
    uint32_t C;
    uint32_t at = fl_block_scan((uint32_t)__popc(ism), wtot, lane, wv, C);    // (every cell is read before the pairs overwrite it)
    uint32_t P = 1;
    while (P < C) P <<= 1;                                         // <= FL_E: C <= the counted entries
#pragma unroll
    for (int i = 0; i < FL_OWN; ++i)
        if ((ism >> i) & 1u) { skey[at] = ck[i]; sterm[at] = ct[i]; ++at; }
    for (uint32_t i = C + t; i < P; i += FL_T) { skey[i] = ~0ull; sterm[i] = 0x7fffffff; }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = t; i < P; i += FL_T) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t ki = skey[i], kl = skey[l];
                    const int ti = sterm[i], tl = sterm[l];
                    const bool after = ki > kl || (ki == kl && ti > tl);
                    if (after == ((i & k) == 0)) { skey[i] = kl; skey[l] = ki; sterm[i] = tl; sterm[l] = ti; }
                }
            }
            __syncthreads();
        }
    }

    // the expanded query: every element of the row is written
    const uint32_t keep = min((uint32_t)a.m, C);
    int32_t* const orow_t = a.out_terms + (size_t)q * a.ldo;
    double* const orow_w = a.out_w + (size_t)q * a.ldo;
    const int64_t width = a.width;
    for (int64_t p = t; p < nq && p < width; p += FL_T) { orow_t[p] = a.qterms[q0 + p]; orow_w[p] = a.alpha; }
    const double wmax = keep ? desc_key_f64_inv(skey[0]) : 1.0;
    for (uint32_t i = t; i < keep; i += FL_T) {
        const int64_t p = nq + i;
        if (p < width) {
            const double ratio = desc_key_f64_inv(skey[i]) / wmax;
            orow_t[p] = sterm[i]; orow_w[p] = a.beta * ratio;
        }
    }
    const int64_t total = nq + keep, written = total < width ? total : width;
    for (int64_t p = written + t; p < width; p += FL_T) { orow_t[p] = -1; orow_w[p] = 0.0; }
    if (t == 0) {
        a.out_len[q] = (int32_t)written;
        const int32_t bits = (cut ? FL_CUT : 0) | (total > width ? FL_NOFIT : 0);
        if (bits) atomicOr(a.flag, bits);
    }
}

// the host side of the three entries: every check before the first HIP call
template <int SRC>
static int fl_run(LexFbArgs a, int Q, void* stream) {
    if (Q < 0 || a.N < 0 || a.F < 0 || a.ldf < a.F || a.ldc < a.F || a.m < 0 || a.width < 0 || a.ldo < a.width) return FZ_ERR_ARG;
    if (Q == 0) return FZ_OK;
    if (!a.qoff || !a.out_len || !a.flag || (a.width != 0 && (!a.out_terms || !a.out_w)) || (a.F != 0 && (!a.fb_ids || !a.coef)))
        return FZ_ERR_ARG;
    if (a.F != 0 && a.N != 0) {
        if (!a.foff) return FZ_ERR_ARG;
        // (fterm and the value tables may be null for an index without postings: every row is empty then)
    }
    hipStream_t st = as_stream(stream);
    static unsigned long long done = 0ull;
    if (int rc = raise_lds_limit((const void*)lexical_feedback_kernel<SRC>, 160 * 1024, done)) return rc;
    FZ_HIP_TRY(hipMemsetAsync(a.flag, 0, sizeof(int32_t), st));
    lexical_feedback_kernel<SRC><<<Q, FL_T, FL_LDS, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

static LexFbArgs fl_args(const int64_t* foff, const int32_t* fterm, int64_t N, int64_t id_base, const int64_t* qoff, const int32_t* qterms,
                         const int64_t* fb_ids, int ldf, const int32_t* fb_len, const float* coef, int ldc, int F, double alpha, double beta, int m,
                         int32_t* out_terms, double* out_w, int ldo, int width, int32_t* out_len, int32_t* flag) {
    LexFbArgs a{};
    a.fb_ids = fb_ids; a.fb_len = fb_len; a.coef = coef; a.N = N; a.id_base = id_base; a.F = F; a.ldf = ldf; a.ldc = ldc;
    a.foff = foff; a.fterm = fterm; a.qoff = qoff; a.qterms = qterms;
    a.out_terms = out_terms; a.out_w = out_w; a.out_len = out_len; a.flag = flag;
    a.ldo = ldo; a.width = width; a.m = m; a.alpha = alpha; a.beta = beta;
    return a;
}

}  // namespace fz

using namespace fz;

extern "C" int fz_lexical_feedback_max_entries(void) { return FL_E; }

extern "C" int fz_bm25_feedback_pv_f64(const int64_t* foff, const int32_t* fterm, const int32_t* fpos, const double* pval, int64_t N,
                                       int64_t id_base, const int64_t* qoff, const int32_t* qterms, int Q, const int64_t* fb_ids, int ldf,
                                       const int32_t* fb_len, const float* coef, int ldc, int F, double alpha, double beta, int m,
                                       int32_t* out_terms, double* out_w, int ldo, int width, int32_t* out_len, int32_t* flag, void* stream) {
    LexFbArgs a = fl_args(foff, fterm, N, id_base, qoff, qterms, fb_ids, ldf, fb_len, coef, ldc, F, alpha, beta, m, out_terms, out_w, ldo, width,
                          out_len, flag);
    a.fpos = fpos; a.pval = pval;
    return fl_run<FL_SRC_PV>(a, Q, stream);
}

extern "C" int fz_tfidf_feedback_f64(const int64_t* foff, const int32_t* fterm, const int32_t* fpos, const int32_t* ptf, const double* idf,
                                     int64_t N, int64_t id_base, const int64_t* qoff, const int32_t* qterms, int Q, const int64_t* fb_ids,
                                     int ldf, const int32_t* fb_len, const float* coef, int ldc, int F, double alpha, double beta, int m,
                                     int32_t* out_terms, double* out_w, int ldo, int width, int32_t* out_len, int32_t* flag, void* stream) {
    LexFbArgs a = fl_args(foff, fterm, N, id_base, qoff, qterms, fb_ids, ldf, fb_len, coef, ldc, F, alpha, beta, m, out_terms, out_w, ldo, width,
                          out_len, flag);
    a.fpos = fpos; a.ptf = ptf; a.idf = idf;
    return fl_run<FL_SRC_TFIDF>(a, Q, stream);
}

extern "C" int fz_lexical_feedback_rows_f64(const int64_t* foff, const int32_t* fterm, const double* fval, int64_t N, int64_t id_base,
                                            const int64_t* qoff, const int32_t* qterms, int Q, const int64_t* fb_ids, int ldf,
                                            const int32_t* fb_len, const float* coef, int ldc, int F, double alpha, double beta, int m,
                                            int32_t* out_terms, double* out_w, int ldo, int width, int32_t* out_len, int32_t* flag,
                                            void* stream) {
    LexFbArgs a = fl_args(foff, fterm, N, id_base, qoff, qterms, fb_ids, ldf, fb_len, coef, ldc, F, alpha, beta, m, out_terms, out_w, ldo, width,
                          out_len, flag);
    a.fval = fval;
    return fl_run<FL_SRC_ROWS>(a, Q, stream);
}
