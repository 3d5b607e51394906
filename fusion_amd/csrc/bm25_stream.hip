// bm25_stream.hip -- the lexical posting walk (csrc/bm25.hip) over a RANGE of documents, with slices.h's three epilogues: the float64
// score plane of the range; the streaming top-k's threshold filter in its place (no plane at all) -- what csrc/sparse.hip's
// sparse_dot_kernel<FILTER> is to float32 SPLADE, for BM25 / AtireBM25 (posting-value table) and TF-IDF in float64; or, per listed
// ("gold") document, the count of the range's documents that the stable float64 ranking puts before it (BM25.tune's grid search: a gold's
// rank is a COUNT; counts over disjoint ranges, chunks and shards add as integers).  One kernel, the epilogue its template parameter.
//
// Bits: per document the score is the chain of float64 adds, in QUERY-TERM order, that bm25_kernel<MODE> makes (query terms not
// de-duplicated, id -1 adds nothing, BM25_TERMS terms resolved per batch; -ffp-contract=off) whatever the range or the grid: a range's
// scores are the full plane's columns, bit for bit.  The walk is restated here rather than shared with bm25_kernel as a device function
// (csrc/bm25_walk.h holds the constants the two must agree on, and says why).
#include "bm25_walk.h"

namespace fz {

// one workgroup = (query, slice): the shapes bm25_kernel was measured best at -- PVAL 3,584 documents x 512 threads (28 KiB of float64
// accumulators, four workgroups per CU), TFIDF 7,168 x 1,024 (56 KiB: no length norms are kept here).  The per-posting expression,
// BM25_EXPR, has no range form.
struct LexArgs {
    const int64_t* toff; const int32_t* pdoc;
    const int32_t* ptf; const double* idf;     // TFIDF: term frequency per posting, idf per term
    const double* pval;                        // PVAL: the posting's whole term (fz_bm25_posting_values_f64)
    const int64_t* slice_off;                  // nullable [V][r.NS + 1] (fz_bm25_slice_offsets)
    const int64_t* qoff; const int32_t* qterms;
    DocRange r;                                // the documents scored (NS: grains of the index)
    double* scores; int lds;                   // plane epilogue: [Q][lds], column j = document doc_lo + j
    FilterSink<double> f;                      // filter epilogue: no plane
    CountSink c;                               // count epilogue: no plane, no list
};

// grid (slices of [doc_lo, doc_hi), Q): workgroup (x, q) scores global slice doc_lo / slice + x.  EPI: the epilogue (LEX_PLANE / LEX_FILTER /
// LEX_COUNT).  Plane and filter ask for what the launch bounds give anyway (2 / 4 waves per SIMD at least); for the count, 8 waves per SIMD
// is what the LDS allows (four workgroups of 8 waves / two of 16 per CU): without the attribute the epilogue's four group widths take 101
// SGPRs, i.e. 7 waves and a workgroup per CU less -- with it 72, nothing spilled.
template <int MODE, int EPI>
__global__ __launch_bounds__(slice_threads<MODE>()) __attribute__((amdgpu_waves_per_eu(EPI == LEX_COUNT ? 8 : slice_threads<MODE>() / 256, 8)))
void lexical_range_kernel(LexArgs a) {
    constexpr bool PVAL = MODE == BM25_PVAL;
    constexpr int SL = slice_grains<MODE>(), SLICE = slice_docs<MODE>();
    __shared__ __attribute__((aligned(16))) double acc[SLICE];            // the slice's accumulators: 28 / 56 KiB, static (with the term tables under 64 KiB)
    __shared__ int64_t s_e0[BM25_TERMS], s_e1[BM25_TERMS];
    __shared__ double s_w[BM25_TERMS];
    static_assert(sizeof(acc) == (PVAL ? 28 : 56) * 1024, "accumulators only");
    const int q = blockIdx.y;
    int d0, d1;
    const int s = slice_of(a.r, SLICE, d0, d1);
    const int n = d1 - d0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) acc[j] = 0.0;
    const int64_t p0 = a.qoff[q], p1 = a.qoff[q + 1];
    for (int64_t pb = p0; pb < p1; pb += BM25_TERMS) {
        const int nt = (int)((p1 - pb < BM25_TERMS) ? p1 - pb : BM25_TERMS);
        __syncthreads();   // acc zeroed / previous batch's table no longer read
        if ((int)threadIdx.x < nt) {
            const int t = a.qterms[pb + threadIdx.x];
            int64_t e0 = 0, e1 = 0; double w = 0.0;
            if (t >= 0) {     // out of vocabulary: contributes nothing
                if constexpr (!PVAL) w = a.idf[t];
                if (a.slice_off) {
                    const int g0 = s * SL, g1 = g0 + SL < a.r.NS ? g0 + SL : a.r.NS;   // (doc_hi is a whole slice or N: grain g1 starts at d1)
                    const int64_t* so = a.slice_off + (size_t)t * (a.r.NS + 1);
                    e0 = so[g0]; e1 = so[g1];
                } else {
                    e0 = lower_bound_doc(a.pdoc, a.toff[t], a.toff[t + 1], d0);
                    e1 = lower_bound_doc(a.pdoc, e0, a.toff[t + 1], d1);
                }
            }
            s_e0[threadIdx.x] = e0; s_e1[threadIdx.x] = e1; s_w[threadIdx.x] = w;
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k) {          // terms in QUERY ORDER: the reference's addition order
            const int64_t e0 = s_e0[k], e1 = s_e1[k];
            const double w = s_w[k];
            if (e1 <= e0) continue;             // block-uniform
            constexpr int U = 4;                // postings per lane in flight (bm25_kernel's measured choice)
            for (int64_t eb = e0; eb < e1; eb += (int64_t)blockDim.x * U) {
                int doc[U]; double tf[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t e = eb + (int64_t)u * blockDim.x + threadIdx.x;
                    const bool ok = e < e1;
                    doc[u] = ok ? a.pdoc[e] : -1;
                    if constexpr (PVAL) tf[u] = ok ? a.pval[e] : 0.0;
                    else tf[u] = ok ? (double)a.ptf[e] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (doc[u] >= 0) {
                        double term;
                        if constexpr (PVAL) term = tf[u];
                        else term = tf[u] * w;                             // bm25.py:114: score += tf * idf
                        acc[doc[u] - d0] = acc[doc[u] - d0] + term;        // postings of one term hit distinct documents: no race
                    }
                }
            }
            __syncthreads();  // the next term may touch the same documents
        }
    }
    __syncthreads();
    if constexpr (EPI == LEX_PLANE) store_plane(acc, n, a.scores, a.lds, q, d0 - a.r.doc_lo);
    else if constexpr (EPI == LEX_FILTER) filter_candidates(acc, n, d0, q, a.f);
    else count_beaters(acc, n, d0, q, a.c);
}

}  // namespace fz

using namespace fz;

// the index and the queries: what every range entry takes.  The scorer's own fields (ptf / pdoc and idf / pval are the same types) and the
// epilogue's sink are set by name in the entry.
static LexArgs lx_args(const int64_t* toff, const int32_t* pdoc, const int64_t* slice_off, const int64_t* qoff, const int32_t* qterms) {
    LexArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.slice_off = slice_off; a.qoff = qoff; a.qterms = qterms;
    return a;
}

// the host side of the six range entries: sizes, the range and the epilogue's own size; "nothing to do"; the pointers; the launch
template <int MODE, int EPI>
static int lx_run(LexArgs a, int Q, int N, int doc_lo, int doc_hi, void* stream) {
    constexpr bool PVAL = MODE == BM25_PVAL;
    if (Q < 0 || !range_ok(N, doc_lo, doc_hi, slice_docs<MODE>())) return FZ_ERR_ARG;
    if (EPI == LEX_PLANE ? a.lds < doc_hi - doc_lo : EPI == LEX_FILTER ? a.f.cap <= 0 : a.c.G < 1) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;   // empty tensors carry null pointers
    if (!a.toff || !a.pdoc || !(PVAL ? a.pval != nullptr : a.ptf && a.idf) || !a.qoff || !a.qterms) return FZ_ERR_ARG;
    if (EPI == LEX_PLANE ? !a.scores
        : EPI == LEX_FILTER ? !a.f.tau || !a.f.cand_s || !a.f.cand_i || !a.f.cand_len || !a.f.overflow
                            : !a.c.gold_scores || !a.c.gold_ids || !a.c.counts) return FZ_ERR_ARG;
    a.r = doc_range(N, doc_lo, doc_hi, BM25_GRAIN);
    lexical_range_kernel<MODE, EPI><<<slice_grid(a.r, slice_docs<MODE>(), Q), slice_threads<MODE>(), 0, as_stream(stream)>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_lexical_slice_docs(int tfidf) { return tfidf ? slice_docs<BM25_TFIDF>() : slice_docs<BM25_PVAL>(); }

extern "C" int fz_bm25_scores_range_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                           const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, double* scores, int lds, void* stream) {
    LexArgs a = lx_args(toff, pdoc, slice_off, qoff, qterms);
    a.pval = pval; a.scores = scores; a.lds = lds;
    return lx_run<BM25_PVAL, LEX_PLANE>(a, Q, N, doc_lo, doc_hi, stream);
}

extern "C" int fz_tfidf_scores_range_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                         const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, double* scores, int lds,
                                         void* stream) {
    LexArgs a = lx_args(toff, pdoc, slice_off, qoff, qterms);
    a.ptf = ptf; a.idf = idf; a.scores = scores; a.lds = lds;
    return lx_run<BM25_TFIDF, LEX_PLANE>(a, Q, N, doc_lo, doc_hi, stream);
}

extern "C" int fz_bm25_filter_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                     const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base, const double* tau,
                                     double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream) {
    LexArgs a = lx_args(toff, pdoc, slice_off, qoff, qterms);
    a.pval = pval; a.f = {tau, cand_scores, cand_ids, cand_len, overflow, cap, id_base};
    return lx_run<BM25_PVAL, LEX_FILTER>(a, Q, N, doc_lo, doc_hi, stream);
}

extern "C" int fz_tfidf_filter_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                   const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base,
                                   const double* tau, double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow,
                                   void* stream) {
    LexArgs a = lx_args(toff, pdoc, slice_off, qoff, qterms);
    a.ptf = ptf; a.idf = idf; a.f = {tau, cand_scores, cand_ids, cand_len, overflow, cap, id_base};
    return lx_run<BM25_TFIDF, LEX_FILTER>(a, Q, N, doc_lo, doc_hi, stream);
}

extern "C" int fz_bm25_count_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                    const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base, const double* gold_scores,
                                    const int64_t* gold_ids, int G, int32_t* counts, void* stream) {
    LexArgs a = lx_args(toff, pdoc, slice_off, qoff, qterms);
    a.pval = pval; a.c = {gold_scores, gold_ids, counts, G, id_base};
    return lx_run<BM25_PVAL, LEX_COUNT>(a, Q, N, doc_lo, doc_hi, stream);
}

extern "C" int fz_tfidf_count_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                  const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base,
                                  const double* gold_scores, const int64_t* gold_ids, int G, int32_t* counts, void* stream) {
    LexArgs a = lx_args(toff, pdoc, slice_off, qoff, qterms);
    a.ptf = ptf; a.idf = idf; a.c = {gold_scores, gold_ids, counts, G, id_base};
    return lx_run<BM25_TFIDF, LEX_COUNT>(a, Q, N, doc_lo, doc_hi, stream);
}
