// bm25_weighted.hip -- the lexical range walk of csrc/bm25_stream.hip for WEIGHTED queries: every query entry j carries a float64 weight
// qw[j] (an expanded query of csrc/feedback_lexical.hip: the original terms at alpha, the expansion terms at beta * w / w_max).  Plane and
// filter epilogues (slices.h); the count epilogue has no weighted form.
//
// Bits: per document the chain, in ENTRY order, of acc = acc + qw[j] * val(t_j, d) from +0.0, where val is what the unweighted walk adds
// for that posting -- pval[p] ('pv'), or (double)ptf[p] * idf[t] ('tfidf': that product is rounded first, then the one with qw[j]).  An
// entry with t_j < 0 adds nothing; entries are not de-duplicated.  With qw all 1.0 the plane is lexical_range_kernel's, bit for bit.
//
// The walk is restated, not shared (csrc/bm25_walk.h says why; bm25_stream.o stays at its six pinned instantiations): the same slices,
// threads, slice_off / binary-search resolution and posting loop, plus the entry's weight in LDS next to the term tables.  The TF-IDF
// instantiations resolve LEXW_TERMS<BM25_TFIDF> = 128 entries per batch, not 256: 56 KiB of accumulators + four 256-entry 8-byte tables
// would be the whole 64 KiB of static LDS.  The batch size only groups the entries; the order of the adds, hence the bits, is the same.
#include "bm25_walk.h"

namespace fz {

template <int MODE> constexpr int lexw_terms() { return MODE == BM25_PVAL ? BM25_TERMS : BM25_TERMS / 2; }

struct LexWArgs {
    const int64_t* toff; const int32_t* pdoc;
    const int32_t* ptf; const double* idf;     // TFIDF
    const double* pval;                        // PVAL
    const int64_t* slice_off;                  // nullable [V][r.NS + 1]
    const int64_t* qoff; const int32_t* qterms; const double* qw;   // qw: one weight per entry of qterms
    DocRange r;
    double* scores; int lds;                   // plane epilogue
    FilterSink<double> f;                      // filter epilogue
};

template <int MODE, int EPI>
__global__ __launch_bounds__(slice_threads<MODE>()) __attribute__((amdgpu_waves_per_eu(MODE == BM25_PVAL ? 8 : 4, 8)))
void lexical_weighted_kernel(LexWArgs a) {
    constexpr bool PVAL = MODE == BM25_PVAL;
    constexpr int SL = slice_grains<MODE>(), SLICE = slice_docs<MODE>(), TERMS = lexw_terms<MODE>();
    __shared__ __attribute__((aligned(16))) double acc[SLICE];
    __shared__ int64_t s_e0[TERMS], s_e1[TERMS];
    __shared__ double s_w[TERMS], s_q[TERMS];                             // idf (TFIDF) and the entry's weight
    static_assert(sizeof(acc) + 4 * 8 * TERMS <= (PVAL ? 36 : 60) * 1024, "accumulators and four term tables");
    const int q = blockIdx.y;
    int d0, d1;
    const int s = slice_of(a.r, SLICE, d0, d1);
    const int n = d1 - d0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) acc[j] = 0.0;
    const int64_t p0 = a.qoff[q], p1 = a.qoff[q + 1];
    for (int64_t pb = p0; pb < p1; pb += TERMS) {
        const int nt = (int)((p1 - pb < TERMS) ? p1 - pb : TERMS);
        __syncthreads();   // acc zeroed / previous batch's table no longer read
        if ((int)threadIdx.x < nt) {
            const int t = a.qterms[pb + threadIdx.x];
            int64_t e0 = 0, e1 = 0; double w = 0.0;
            if (t >= 0) {     // out of vocabulary: contributes nothing
                if constexpr (!PVAL) w = a.idf[t];
                if (a.slice_off) {
                    const int g0 = s * SL, g1 = g0 + SL < a.r.NS ? g0 + SL : a.r.NS;
                    const int64_t* so = a.slice_off + (size_t)t * (a.r.NS + 1);
                    e0 = so[g0]; e1 = so[g1];
                } else {
                    e0 = lower_bound_doc(a.pdoc, a.toff[t], a.toff[t + 1], d0);
                    e1 = lower_bound_doc(a.pdoc, e0, a.toff[t + 1], d1);
                }
            }
            s_e0[threadIdx.x] = e0; s_e1[threadIdx.x] = e1; s_w[threadIdx.x] = w; s_q[threadIdx.x] = a.qw[pb + threadIdx.x];
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k) {          // entries in QUERY ORDER: the addition order
            const int64_t e0 = s_e0[k], e1 = s_e1[k];
            const double w = s_w[k], qw = s_q[k];
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
                        double val;
                        if constexpr (PVAL) val = tf[u];
                        else val = tf[u] * w;                              // the unweighted walk's term, rounded
                        const double term = qw * val;                      // ... then weighted, rounded again
                        acc[doc[u] - d0] = acc[doc[u] - d0] + term;        // postings of one term hit distinct documents: no race
                    }
                }
            }
            __syncthreads();  // the next entry may touch the same documents
        }
    }
    __syncthreads();
    if constexpr (EPI == LEX_PLANE) store_plane(acc, n, a.scores, a.lds, q, d0 - a.r.doc_lo);
    else filter_candidates(acc, n, d0, q, a.f);
}

}  // namespace fz

using namespace fz;

static LexWArgs lw_args(const int64_t* toff, const int32_t* pdoc, const int64_t* slice_off, const int64_t* qoff, const int32_t* qterms,
                        const double* qw) {
    LexWArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.slice_off = slice_off; a.qoff = qoff; a.qterms = qterms; a.qw = qw;
    return a;
}

// the host side of the four weighted entries: lx_run's checks (csrc/bm25_stream.hip) in its order, with qw among the pointers
template <int MODE, int EPI>
static int lw_run(LexWArgs a, int Q, int N, int doc_lo, int doc_hi, void* stream) {
    static_assert(EPI == LEX_PLANE || EPI == LEX_FILTER, "no weighted count");
    constexpr bool PVAL = MODE == BM25_PVAL;
    if (Q < 0 || !range_ok(N, doc_lo, doc_hi, slice_docs<MODE>())) return FZ_ERR_ARG;
    if (EPI == LEX_PLANE ? a.lds < doc_hi - doc_lo : a.f.cap <= 0) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;   // empty tensors carry null pointers
    if (!a.toff || !a.pdoc || !(PVAL ? a.pval != nullptr : a.ptf && a.idf) || !a.qoff || !a.qterms || !a.qw) return FZ_ERR_ARG;
    if (EPI == LEX_PLANE ? !a.scores : !a.f.tau || !a.f.cand_s || !a.f.cand_i || !a.f.cand_len || !a.f.overflow) return FZ_ERR_ARG;
    a.r = doc_range(N, doc_lo, doc_hi, BM25_GRAIN);
    lexical_weighted_kernel<MODE, EPI><<<slice_grid(a.r, slice_docs<MODE>(), Q), slice_threads<MODE>(), 0, as_stream(stream)>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_lexical_weighted_terms(int tfidf) { return tfidf ? lexw_terms<BM25_TFIDF>() : lexw_terms<BM25_PVAL>(); }

extern "C" int fz_bm25_scores_range_w_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off,
                                             const int64_t* qoff, const int32_t* qterms, const double* qw, int Q, int N, int doc_lo, int doc_hi,
                                             double* scores, int lds, void* stream) {
    LexWArgs a = lw_args(toff, pdoc, slice_off, qoff, qterms, qw);
    a.pval = pval; a.scores = scores; a.lds = lds;
    return lw_run<BM25_PVAL, LEX_PLANE>(a, Q, N, doc_lo, doc_hi, stream);
}

extern "C" int fz_tfidf_scores_range_w_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                           const int64_t* qoff, const int32_t* qterms, const double* qw, int Q, int N, int doc_lo, int doc_hi,
                                           double* scores, int lds, void* stream) {
    LexWArgs a = lw_args(toff, pdoc, slice_off, qoff, qterms, qw);
    a.ptf = ptf; a.idf = idf; a.scores = scores; a.lds = lds;
    return lw_run<BM25_TFIDF, LEX_PLANE>(a, Q, N, doc_lo, doc_hi, stream);
}

extern "C" int fz_bm25_filter_w_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                       const int32_t* qterms, const double* qw, int Q, int N, int doc_lo, int doc_hi, int64_t id_base,
                                       const double* tau, double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow,
                                       void* stream) {
    LexWArgs a = lw_args(toff, pdoc, slice_off, qoff, qterms, qw);
    a.pval = pval; a.f = {tau, cand_scores, cand_ids, cand_len, overflow, cap, id_base};
    return lw_run<BM25_PVAL, LEX_FILTER>(a, Q, N, doc_lo, doc_hi, stream);
}

extern "C" int fz_tfidf_filter_w_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                     const int64_t* qoff, const int32_t* qterms, const double* qw, int Q, int N, int doc_lo, int doc_hi,
                                     int64_t id_base, const double* tau, double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap,
                                     int32_t* overflow, void* stream) {
    LexWArgs a = lw_args(toff, pdoc, slice_off, qoff, qterms, qw);
    a.ptf = ptf; a.idf = idf; a.f = {tau, cand_scores, cand_ids, cand_len, overflow, cap, id_base};
    return lw_run<BM25_TFIDF, LEX_FILTER>(a, Q, N, doc_lo, doc_hi, stream);
}
