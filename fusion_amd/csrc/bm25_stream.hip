// bm25_stream.hip -- the lexical posting walk (csrc/bm25.hip) over a RANGE of documents, with two epilogues: the float64 score plane of the
// range, or the streaming top-k's threshold filter in its place (no plane at all) -- what csrc/sparse.hip's sparse_dot_kernel /
// sparse_dot_filter_kernel are to float32 SPLADE, for BM25 / AtireBM25 (posting-value table) and TF-IDF in float64.
//
// Bits: per document the score is the chain of float64 adds, in QUERY-TERM order, that bm25_kernel<MODE> makes (query terms not
// de-duplicated, id -1 adds nothing, BM25_TERMS terms resolved per batch; -ffp-contract=off) whatever the range or the grid: a range's
// scores are the full plane's columns, bit for bit.  The walk is restated here rather than shared with bm25_kernel as a device function, so
// that kernel's code and resource figures stay what they were measured at.
#include "common.h"

namespace fz {

constexpr int LX_GRAIN = 3584;      // = BM25_GRAIN: the granularity of the per-index table of fz_bm25_slice_offsets
constexpr int LX_TERMS = 256;       // = BM25_TERMS
enum { LX_TFIDF = 1, LX_PVAL = 2 }; // = BM25_TFIDF, BM25_PVAL (the per-posting expression, BM25_EXPR, has no range form)

// one workgroup = (query, slice): the shapes bm25_kernel was measured best at -- PVAL 3,584 documents x 512 threads (28 KiB of float64
// accumulators, four workgroups per CU), TFIDF 7,168 x 1,024 (56 KiB: no length norms are kept here)
template <int MODE> constexpr int lx_grains() { return MODE == LX_PVAL ? 1 : 2; }
template <int MODE> constexpr int lx_slice() { return LX_GRAIN * lx_grains<MODE>(); }
template <int MODE> constexpr int lx_threads() { return MODE == LX_PVAL ? 512 : 1024; }
template <int MODE> constexpr size_t lx_lds_bytes() { return (size_t)lx_slice<MODE>() * sizeof(double); }
static_assert(lx_lds_bytes<LX_PVAL>() == 28 * 1024 && lx_lds_bytes<LX_TFIDF>() == 56 * 1024, "accumulators only");

struct LexArgs {
    const int64_t* toff; const int32_t* pdoc;
    const int32_t* ptf; const double* idf;     // TFIDF: term frequency per posting, idf per term
    const double* pval;                        // PVAL: the posting's whole term (fz_bm25_posting_values_f64)
    const int64_t* slice_off;                  // nullable [V][ceil(N / LX_GRAIN) + 1] (fz_bm25_slice_offsets)
    const int64_t* qoff; const int32_t* qterms;
    int N;                                     // documents of the index (the table's row stride comes from it)
    int doc_lo, doc_hi;                        // the documents scored: [doc_lo, doc_hi), doc_lo a whole slice
    double* scores; int lds;                   // plane epilogue: [Q][lds], column j = document doc_lo + j
    // filter epilogue: no plane; what beats tau[q] (or is NaN) goes to query q's candidate list
    const double* tau; double* cand_s; int64_t* cand_i; int32_t* cand_len; int32_t* overflow; int cap;
    int64_t id_base;                           // id of index document 0
};

__device__ __forceinline__ int64_t lx_lower_bound(const int32_t* __restrict__ pdoc, int64_t lo, int64_t hi, int doc) {
    while (lo < hi) {   // first e in [lo, hi) with pdoc[e] >= doc
        const int64_t mid = (lo + hi) >> 1;
        if (pdoc[mid] < doc) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid (slices of [doc_lo, doc_hi), Q): workgroup (x, q) scores global slice doc_lo / slice + x.  FILTER: the epilogue.
template <int MODE, bool FILTER>
__global__ __launch_bounds__(lx_threads<MODE>()) void lexical_range_kernel(LexArgs a) {
    constexpr bool PVAL = MODE == LX_PVAL;
    constexpr int SL = lx_grains<MODE>(), SLICE = lx_slice<MODE>();
    __shared__ __attribute__((aligned(16))) double acc[SLICE];            // the slice's accumulators: 28 / 56 KiB, static (with the term tables under 64 KiB)
    __shared__ int64_t s_e0[LX_TERMS], s_e1[LX_TERMS];
    __shared__ double s_w[LX_TERMS];
    const int q = blockIdx.y;
    const int s = a.doc_lo / SLICE + (int)blockIdx.x;
    const int d0 = s * SLICE;
    const int d1 = (d0 + SLICE < a.doc_hi) ? d0 + SLICE : a.doc_hi;
    const int n = d1 - d0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) acc[j] = 0.0;
    const int64_t p0 = a.qoff[q], p1 = a.qoff[q + 1];
    for (int64_t pb = p0; pb < p1; pb += LX_TERMS) {
        const int nt = (int)((p1 - pb < LX_TERMS) ? p1 - pb : LX_TERMS);
        __syncthreads();   // acc zeroed / previous batch's table no longer read
        if ((int)threadIdx.x < nt) {
            const int t = a.qterms[pb + threadIdx.x];
            int64_t e0 = 0, e1 = 0; double w = 0.0;
            if (t >= 0) {     // out of vocabulary: contributes nothing
                if constexpr (!PVAL) w = a.idf[t];
                if (a.slice_off) {
                    const int ns = (a.N + LX_GRAIN - 1) / LX_GRAIN;          // grains the table was made for
                    const int g0 = s * SL, g1 = g0 + SL < ns ? g0 + SL : ns;  // (doc_hi is a whole slice or N: grain g1 starts at d1)
                    const int64_t* so = a.slice_off + (size_t)t * (ns + 1);
                    e0 = so[g0]; e1 = so[g1];
                } else {
                    e0 = lx_lower_bound(a.pdoc, a.toff[t], a.toff[t + 1], d0);
                    e1 = lx_lower_bound(a.pdoc, e0, a.toff[t + 1], d1);
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
    if constexpr (!FILTER) {
        double* __restrict__ row = a.scores + (size_t)q * a.lds + (d0 - a.doc_lo);
        for (int j = threadIdx.x; j < n; j += blockDim.x) row[j] = acc[j];
    } else {
        // fz_sparse_dot_filter_f32's rule in float64: a document enters query q's candidates iff !(score <= tau[q]).  Per wave and 64
        // documents: ballot, ONE atomicAdd on cand_len[q] for the wave's survivors (none when there are none), each survivor stores at
        // base + its rank in the ballot -- never at or past cap; cand_len keeps counting.
        const double tq = a.tau[q];
        const int lane = threadIdx.x & 63;
        const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;    // lanes under this one
        double* __restrict__ cs = a.cand_s + (size_t)q * a.cap;
        int64_t* __restrict__ ci = a.cand_i + (size_t)q * a.cap;
        bool over = false;
        for (int j0 = 0; j0 < n; j0 += blockDim.x) {                              // wave-uniform trip count: every lane takes part in the ballot
            const int j = j0 + (int)threadIdx.x;
            const double v = j < n ? acc[j] : 0.0;
            const bool keep = j < n && !(v <= tq);
            const unsigned long long bal = __ballot(keep);
            if (bal == 0ull) continue;                                            // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(a.cand_len + q, (int)__popcll(bal));
            base = __shfl(base, 0);
            if (keep) {
                const int pos = base + (int)__popcll(bal & below);
                if (pos < a.cap) {
                    cs[pos] = v;
                    ci[pos] = a.id_base + d0 + j;
                } else over = true;
            }
        }
        if (__syncthreads_or(over) && threadIdx.x == 0) atomicExch(a.overflow, 1);   // one per workgroup
    }
}

template <int MODE>
static bool lx_range_ok(int N, int doc_lo, int doc_hi) {
    constexpr int S = lx_slice<MODE>();
    return N >= 0 && doc_lo >= 0 && doc_lo <= doc_hi && doc_hi <= N && doc_lo % S == 0 && (doc_hi % S == 0 || doc_hi == N);
}

template <int MODE, bool FILTER>
static int lx_launch(const LexArgs& a, int Q, hipStream_t st) {
    constexpr int S = lx_slice<MODE>();
    dim3 grid((unsigned)((a.doc_hi - a.doc_lo + S - 1) / S), (unsigned)Q);
    lexical_range_kernel<MODE, FILTER><<<grid, lx_threads<MODE>(), 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

}  // namespace fz

using namespace fz;

extern "C" int fz_lexical_slice_docs(int tfidf) { return tfidf ? lx_slice<LX_TFIDF>() : lx_slice<LX_PVAL>(); }

extern "C" int fz_bm25_scores_range_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                           const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, double* scores, int lds, void* stream) {
    if (Q < 0 || !lx_range_ok<LX_PVAL>(N, doc_lo, doc_hi) || lds < doc_hi - doc_lo) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;   // empty tensors carry null pointers
    if (!toff || !pdoc || !pval || !qoff || !qterms || !scores) return FZ_ERR_ARG;
    LexArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.pval = pval; a.slice_off = slice_off; a.qoff = qoff; a.qterms = qterms;
    a.N = N; a.doc_lo = doc_lo; a.doc_hi = doc_hi; a.scores = scores; a.lds = lds;
    return lx_launch<LX_PVAL, false>(a, Q, as_stream(stream));
}

extern "C" int fz_tfidf_scores_range_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                         const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, double* scores, int lds,
                                         void* stream) {
    if (Q < 0 || !lx_range_ok<LX_TFIDF>(N, doc_lo, doc_hi) || lds < doc_hi - doc_lo) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;
    if (!toff || !pdoc || !ptf || !idf || !qoff || !qterms || !scores) return FZ_ERR_ARG;
    LexArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.ptf = ptf; a.idf = idf; a.slice_off = slice_off; a.qoff = qoff; a.qterms = qterms;
    a.N = N; a.doc_lo = doc_lo; a.doc_hi = doc_hi; a.scores = scores; a.lds = lds;
    return lx_launch<LX_TFIDF, false>(a, Q, as_stream(stream));
}

extern "C" int fz_bm25_filter_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* slice_off, const int64_t* qoff,
                                     const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base, const double* tau,
                                     double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream) {
    if (Q < 0 || !lx_range_ok<LX_PVAL>(N, doc_lo, doc_hi) || cap <= 0) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;
    if (!toff || !pdoc || !pval || !qoff || !qterms || !tau || !cand_scores || !cand_ids || !cand_len || !overflow) return FZ_ERR_ARG;
    LexArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.pval = pval; a.slice_off = slice_off; a.qoff = qoff; a.qterms = qterms;
    a.N = N; a.doc_lo = doc_lo; a.doc_hi = doc_hi;
    a.tau = tau; a.cand_s = cand_scores; a.cand_i = cand_ids; a.cand_len = cand_len; a.overflow = overflow; a.cap = cap; a.id_base = id_base;
    return lx_launch<LX_PVAL, true>(a, Q, as_stream(stream));
}

extern "C" int fz_tfidf_filter_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* slice_off,
                                   const int64_t* qoff, const int32_t* qterms, int Q, int N, int doc_lo, int doc_hi, int64_t id_base,
                                   const double* tau, double* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow,
                                   void* stream) {
    if (Q < 0 || !lx_range_ok<LX_TFIDF>(N, doc_lo, doc_hi) || cap <= 0) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;
    if (!toff || !pdoc || !ptf || !idf || !qoff || !qterms || !tau || !cand_scores || !cand_ids || !cand_len || !overflow) return FZ_ERR_ARG;
    LexArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.ptf = ptf; a.idf = idf; a.slice_off = slice_off; a.qoff = qoff; a.qterms = qterms;
    a.N = N; a.doc_lo = doc_lo; a.doc_hi = doc_hi;
    a.tau = tau; a.cand_s = cand_scores; a.cand_i = cand_ids; a.cand_len = cand_len; a.overflow = overflow; a.cap = cap; a.id_base = id_base;
    return lx_launch<LX_TFIDF, true>(a, Q, as_stream(stream));
}
