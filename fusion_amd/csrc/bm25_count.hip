// bm25_count.hip -- the ranks of a few listed ("gold") documents per query in the lexical ranking of a corpus of any size, without a
// score plane, a list or a sort: what BM25.tune needs of every (k1, b) pair (every metric of the grid search is a function of the gold
// documents' ranks), and rank(g) = #{ d : d is ranked before g } is a COUNT.  Two steps, in the two modes that have a range walk:
//   lexical_doc_scores_kernel<MODE>         (this file) the float64 scores of the listed documents, by binary search in the query terms' postings;
//   lexical_range_kernel<MODE, LEX_COUNT>   csrc/bm25_stream.hip's walk over a range of documents with slices.h's third epilogue, count_beaters:
//                                           per gold, how many documents of the slice the stable float64 ranking puts before it.
// Counts over disjoint ranges add: ranges, chunks and shards combine by integer sums (bit-reproducible, no float atomics).
//
// Bits: a listed document's score is the walk's chain of float64 adds for that document (query-term order, terms not de-duplicated, id -1
// adds nothing, `acc = acc + term` from 0.0; -ffp-contract=off): the bits of the full plane's entry.  The counting walk is not a kernel of
// this file: shared with lexical_range_kernel as a device function it moved the TF-IDF instantiations' registers, as that kernel's third
// epilogue it moves none (csrc/bm25_walk.h).
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

}  // namespace fz

using namespace fz;

template <int MODE>
static int ds_launch(DocScoreArgs& a, int Q, int G, hipStream_t st) {
    a.G = G; a.total = (long)Q * G;
    lexical_doc_scores_kernel<MODE><<<(unsigned)((a.total + 255) / 256), 256, 0, st>>>(a);
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
