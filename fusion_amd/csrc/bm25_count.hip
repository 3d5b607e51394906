// bm25_count.hip -- the ranks of a few listed ("gold") documents per query in the lexical ranking of a corpus of any size, without a
// score plane, a list or a sort: what BM25.tune needs of every (k1, b) pair (every metric of the grid search is a function of the gold
// documents' ranks), and rank(g) = #{ d : d is ranked before g } is a COUNT.  Two kernels, in the two modes that have a range walk:
//   lexical_doc_scores_kernel<MODE>   the float64 scores of the listed documents, by binary search in the query terms' postings;
//   lexical_count_kernel<MODE>        csrc/bm25_stream.hip's walk over a range of documents with slices.h's third epilogue, count_beaters:
//                                     per gold, how many documents of the slice the stable float64 ranking puts before it.
// Counts over disjoint ranges add: ranges, chunks and shards combine by integer sums (bit-reproducible, no float atomics).
//
// Bits: a listed document's score is the walk's chain of float64 adds for that document (query-term order, terms not de-duplicated, id -1
// adds nothing, `acc = acc + term` from 0.0; -ffp-contract=off): the bits of the full plane's entry.  The walk is restated here, not
// shared with lexical_range_kernel as a device function: that moved the TF-IDF instantiations' registers (csrc/bm25_walk.h).
#include "bm25_walk.h"

namespace fz {

struct DocScoreArgs {
    const int64_t* toff; const int32_t* pdoc;
    const int32_t* ptf; const double* idf;     // TFIDF
    const double* pval;                        // PVAL
    const int64_t* qoff; const int32_t* qterms;
    const int32_t* docs;                       // [Q][G] positions in this index; < 0 (or >= N): not in it
    double* out;                               // [Q][G]; -inf for a document that is not in this index
    int N, G; long total;                      // total = Q * G
};

// one thread per (query, listed document)
template <int MODE>
__global__ __launch_bounds__(256) void lexical_doc_scores_kernel(DocScoreArgs a) {
    constexpr bool PVAL = MODE == BM25_PVAL;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int q = (int)(i / a.G);
    const int d = a.docs[i];
    if (d < 0 || d >= a.N) { a.out[i] = -__builtin_inf(); return; }
    double acc = 0.0;
    const int64_t p0 = a.qoff[q], p1 = a.qoff[q + 1];
    for (int64_t p = p0; p < p1; ++p) {        // terms in QUERY ORDER: the walk's addition order
        const int t = a.qterms[p];
        if (t < 0) continue;                   // out of vocabulary: contributes nothing
        const int64_t end = a.toff[t + 1];
        const int64_t e = lower_bound_doc(a.pdoc, a.toff[t], end, d);
        if (e < end && a.pdoc[e] == d) {
            double term;
            if constexpr (PVAL) term = a.pval[e];
            else term = (double)a.ptf[e] * a.idf[t];
            acc = acc + term;
        }
    }
    a.out[i] = acc;
}

struct CountArgs {
    const int64_t* toff; const int32_t* pdoc;
    const int32_t* ptf; const double* idf;     // TFIDF: term frequency per posting, idf per term
    const double* pval;                        // PVAL: the posting's whole term (fz_bm25_posting_values_f64)
    const int64_t* slice_off;                  // nullable [V][r.NS + 1] (fz_bm25_slice_offsets)
    const int64_t* qoff; const int32_t* qterms;
    DocRange r;                                // the documents scored (NS: grains of the index)
    CountSink c;
};

// grid (slices of [doc_lo, doc_hi), Q): lexical_range_kernel's geometry and walk, count_beaters as the epilogue.  8 waves per SIMD is what
// the LDS allows (four workgroups of 8 waves / two of 16 per CU); without the attribute the epilogue's four group widths take 101 SGPRs,
// i.e. 7 waves and a workgroup per CU less -- with it 72, nothing spilled.
template <int MODE>
__global__ __launch_bounds__(slice_threads<MODE>()) __attribute__((amdgpu_waves_per_eu(8, 8))) void lexical_count_kernel(CountArgs a) {
    constexpr bool PVAL = MODE == BM25_PVAL;
    constexpr int SL = slice_grains<MODE>(), SLICE = slice_docs<MODE>();
    __shared__ __attribute__((aligned(16))) double acc[SLICE];            // the slice's accumulators: 28 / 56 KiB, static
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
    count_beaters(acc, n, d0, q, a.c);
}

}  // namespace fz

using namespace fz;

template <int MODE>
static int ds_launch(DocScoreArgs& a, int Q, int G, hipStream_t st) {
    a.G = G; a.total = (long)Q * G;
    lexical_doc_scores_kernel<MODE><<<(unsigned)((a.total + 255) / 256), 256, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

template <int MODE>
static int ct_launch(const CountArgs& a, int Q, hipStream_t st) {
    lexical_count_kernel<MODE><<<slice_grid(a.r, slice_docs<MODE>(), Q), slice_threads<MODE>(), 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_bm25_doc_scores_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* qoff, const int32_t* qterms, int Q,
                                         int N, const int32_t* docs, int G, double* out, void* stream) {
    if (Q < 0 || N < 0 || G < 1) return FZ_ERR_ARG;
    if (Q == 0) return FZ_OK;   // empty tensors carry null pointers
    if (!toff || !pdoc || !pval || !qoff || !qterms || !docs || !out) return FZ_ERR_ARG;
    DocScoreArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.pval = pval; a.qoff = qoff; a.qterms = qterms; a.docs = docs; a.out = out; a.N = N;
    return ds_launch<BM25_PVAL>(a, Q, G, as_stream(stream));
}

extern "C" int fz_tfidf_doc_scores_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* qoff,
                                       const int32_t* qterms, int Q, int N, const int32_t* docs, int G, double* out, void* stream) {
    if (Q < 0 || N < 0 || G < 1) return FZ_ERR_ARG;
    if (Q == 0) return FZ_OK;
    if (!toff || !pdoc || !ptf || !idf || !qoff || !qterms || !docs || !out) return FZ_ERR_ARG;
    DocScoreArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.ptf = ptf; a.idf = idf; a.qoff = qoff; a.qterms = qterms; a.docs = docs; a.out = out; a.N = N;
    return ds_launch<BM25_TFIDF>(a, Q, G, as_stream(stream));
}

static CountArgs ct_args(const int64_t* toff, const int32_t* pdoc, const int64_t* slice_off, const int64_t* qoff, const int32_t* qterms, int N, int doc_lo,
                         int doc_hi, int64_t id_base, const double* gold_scores, const int64_t* gold_ids, int G, int32_t* counts) {
    CountArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.slice_off = slice_off; a.qoff = qoff; a.qterms = qterms;
    a.r = doc_range(N, doc_lo, doc_hi, BM25_GRAIN);
    a.c = {gold_scores, gold_ids, counts, G, id_base};
    return a;
}

extern "C" int fz_bm25_count_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                    const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base, const double* gold_scores,
                                    const int64_t* gold_ids, int G, int32_t* counts, void* stream) {
    if (Q < 0 || !range_ok(N, doc_lo, doc_hi, slice_docs<BM25_PVAL>()) || G < 1) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;   // empty tensors carry null pointers
    if (!toff || !pdoc || !pval || !qoff || !qterms || !gold_scores || !gold_ids || !counts) return FZ_ERR_ARG;
    CountArgs a = ct_args(toff, pdoc, slice_off, qoff, qterms, N, doc_lo, doc_hi, id_base, gold_scores, gold_ids, G, counts);
    a.pval = pval;
    return ct_launch<BM25_PVAL>(a, Q, as_stream(stream));
}

extern "C" int fz_tfidf_count_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                  const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base,
                                  const double* gold_scores, const int64_t* gold_ids, int G, int32_t* counts, void* stream) {
    if (Q < 0 || !range_ok(N, doc_lo, doc_hi, slice_docs<BM25_TFIDF>()) || G < 1) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;
    if (!toff || !pdoc || !ptf || !idf || !qoff || !qterms || !gold_scores || !gold_ids || !counts) return FZ_ERR_ARG;
    CountArgs a = ct_args(toff, pdoc, slice_off, qoff, qterms, N, doc_lo, doc_hi, id_base, gold_scores, gold_ids, G, counts);
    a.ptf = ptf; a.idf = idf;
    return ct_launch<BM25_TFIDF>(a, Q, as_stream(stream));
}
