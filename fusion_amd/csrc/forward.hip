// forward.hip -- pair scores from a FORWARD (document-major) index: a pair's score is a question about ONE document, and a document's
// postings are one contiguous row (ops.forward_index: a stable sort of the inverted postings by document, terms ascending in a row).
//
//   fz_sparse_fwd_pairs_f32          out[q][r] = the bits of fz_sparse_dot_pairs_f32's, from rows of {int32 term, float32 weight}
//   fz_tfidf_doc_scores_fwd_f64      the bits of fz_tfidf_doc_scores_f64's
//   fz_bm25_doc_scores_fwd_pv_f64    the bits of fz_bm25_doc_scores_pv_f64's
//
// Sparse.  sparse.hip's chain adds the products of the terms query and document share, in ascending term order; a walk along the
// document's row meets the same terms in the same order, so the sum has the same bits.  The inverted route finds the shared terms by one
// binary search per query term in a posting list of up to N entries (about 700 scattered 4-byte reads per pair); here the row is read
// once, as whole lines:
//   * a workgroup = 4 waves = (query, block of 256 candidate slots); thread i resolves slot i once (id -> row, its offset and length);
//   * the query's term set is a bitmap over V in LDS (4 KB at V = 32,005), cleared and set once per workgroup (LDS atomicOr), and next
//     to it, per bitmap word, the number of set bits before the word (one scan over the workgroup);
//   * a group of 16 lanes owns a candidate: per step each lane loads one 8-byte posting -- 128 contiguous bytes per group; a group has
//     FW_U rows in flight and the next step's loads are issued before this step's postings are looked at (2 x 4 x 128 B per group);
//   * a lane tests its term's bit; on a hit (about 10 of 166 postings) the term's place in the query's list is the number of set bits
//     below it -- the word's count + a popcount: the list is strictly ascending -- so the weight is ONE read of qw (global, tiny,
//     cached), the four of a step in flight together; pr = qw * w with its own rounding (-ffp-contract=off).  Finding the place by a
//     binary search in qterms instead, six dependent reads per hit in front of the adds, took 1.72 ms where this takes 0.93
//     (profiles/r21_forward_pairs_qterm_search.json / r21_forward_pairs.json);
//   * the group adds its hits in lane order, step after step: acc = acc + pr from +0.0, through a ballot of the hit flags and one
//     cross-lane read per hit (the loop is wave-uniform: every lane takes part in the ballot and the read).  No hit adds nothing.
// An absent slot has a row of no postings and stores -inf; a lane past its row's end loads nothing (its row's last line is not read
// twice to keep the load unpredicated: an empty row has no line to read).  No workspace, no atomics on global memory, no host
// synchronisation, no cap on a query's term count.
//
// Lexical.  One thread per (query, listed document), lexical_doc_scores_kernel's chain (query order, terms not de-duplicated, -1 adds
// nothing, acc = acc + term from 0.0); the binary search runs in the document's row of terms -- a few steps inside one or two cache
// lines -- and fpos leads to the posting's place in the inverted tables (ptf, or pval for the current (k1, b)).
//
// Where it stands: DESIGN.md section 'Forward index'.
#include "bm25_walk.h"
#include "pairs.h"

namespace fz {

constexpr int FW_THREADS = 256;
constexpr int FW_SLOTS = 256;                          // candidate slots per workgroup: one per thread while they are resolved
constexpr int FW_GROUP = 16;                           // lanes per candidate row: 16 x 8 B = one 128-byte line per step
constexpr int FW_GROUPS = FW_THREADS / FW_GROUP;
constexpr int FW_PER_GROUP = FW_SLOTS / FW_GROUPS;     // slots a group walks, FW_U at a time
constexpr int FW_U = 4;                                // rows in flight per group (measured: 2 -> 1.00 ms, 4 -> 0.95, 8 -> 1.10 at 96 VGPRs)
constexpr int FW_MAX_V = 32 * 1024 * 8;                // a 32 KiB bitmap + as much for its rank table: two workgroups (+ 3 KiB of slots each) per CU's 160 KiB
static_assert(FW_PER_GROUP % FW_U == 0 && FW_GROUP == 16 && FW_MAX_V >= 65536, "the lane-group arithmetic below");

struct FwdPairsArgs {
    const int64_t* foff; const int2* rows;                         // row of document d: postings [foff[d], foff[d+1]), {term, weight bits}
    const int64_t* qoff; const int32_t* qterms; const float* qw;   // queries: non-zero terms of query q are [qoff[q], qoff[q+1]), ascending
    const int64_t* cand; const int32_t* cand_len;
    float* out;
    int64_t id_base;
    int ldc, ldo, Q, N, V, W, nblocks;
};

__global__ __launch_bounds__(FW_THREADS) void sparse_fwd_pairs_kernel(FwdPairsArgs a) {
    extern __shared__ uint32_t bits[];                             // [words] the query's term set | [words] the set bits before each word
    __shared__ int64_t s_start[FW_SLOTS];
    __shared__ int s_len[FW_SLOTS];                                // -1: an absent slot
    __shared__ uint32_t s_wave[FW_THREADS / 64];
    const int tid = threadIdx.x, l = tid & (FW_GROUP - 1), g = tid >> 4, gbase = tid & 48;   // gbase: the group's first lane in its wave
    const int q = blockIdx.x / a.nblocks;
    const int slot0 = (blockIdx.x % a.nblocks) * FW_SLOTS;
    const int64_t q0 = a.qoff[q];
    const int nq = (int)(a.qoff[q + 1] - q0);
    const int words = (a.V + 31) >> 5;
    uint32_t* const before = bits + words;

    for (int i = tid; i < words; i += FW_THREADS) bits[i] = 0u;
    {
        const int pos = slot0 + tid < a.W ? pair_position(a.cand, a.ldc, a.cand_len, a.id_base, a.N, a.W, q, slot0 + tid) : -1;
        int64_t st = 0; int len = -1;
        if (pos >= 0) { st = a.foff[pos]; len = (int)(a.foff[pos + 1] - st); }
        s_start[tid] = st; s_len[tid] = len;
    }
    __syncthreads();
    for (int p = tid; p < nq; p += FW_THREADS) {
        const int t = a.qterms[q0 + p];
        if ((unsigned)t < (unsigned)a.V) atomicOr(&bits[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    {   // before[w] = the query's terms below 32 w: thread i counts words [i c, (i + 1) c), the counts are scanned over the workgroup
        const int c = (words + FW_THREADS - 1) / FW_THREADS, w0 = tid * c, w1 = w0 + c < words ? w0 + c : words;
        uint32_t mine = 0u;
        for (int w = w0; w < w1; ++w) mine += __popc(bits[w]);
        const uint32_t incl = wave_incl_scan_u32(mine, tid & 63);
        if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
        __syncthreads();
        uint32_t run = incl - mine;
        for (int v = 0; v < (tid >> 6); ++v) run += s_wave[v];
        for (int w = w0; w < w1; ++w) { before[w] = run; run += __popc(bits[w]); }
    }
    __syncthreads();

    for (int b = 0; b < FW_PER_GROUP; b += FW_U) {
        const int first = g * FW_PER_GROUP + b;                    // the group's slots of this round: first .. first + FW_U - 1
        int64_t st[FW_U]; int len[FW_U]; float acc[FW_U];
        int nsteps = 0;
#pragma unroll
        for (int u = 0; u < FW_U; ++u) {
            st[u] = s_start[first + u]; len[u] = s_len[first + u]; acc[u] = 0.0f;
            const int n = (len[u] + FW_GROUP - 1) >> 4;            // (0 for an absent slot)
            nsteps = n > nsteps ? n : nsteps;
        }
        { const int o = __shfl_xor(nsteps, 16); nsteps = o > nsteps ? o : nsteps; }   // the wave's four groups step together
        { const int o = __shfl_xor(nsteps, 32); nsteps = o > nsteps ? o : nsteps; }

        int2 cur[FW_U];
        auto gload = [&](int2 (&dst)[FW_U], int s) __attribute__((always_inline)) {
            const int k = s * FW_GROUP + l;
#pragma unroll
            for (int u = 0; u < FW_U; ++u) {
                dst[u] = make_int2(-1, 0);                         // past the row's end: no term
                if (k < len[u]) dst[u] = a.rows[st[u] + k];
            }
        };
        gload(cur, 0);
        for (int s = 0; s < nsteps; ++s) {                         // wave-uniform
            int2 nxt[FW_U];
            gload(nxt, s + 1);                                     // in flight under this step's tests (nothing past the last step)
            bool hit[FW_U]; float pr[FW_U];
#pragma unroll
            for (int u = 0; u < FW_U; ++u) {                       // the FW_U weight loads of a step are in flight together
                const int term = cur[u].x;
                const bool in = (unsigned)term < (unsigned)a.V;
                const int w = in ? term >> 5 : 0;
                const uint32_t word = bits[w], bit = 1u << (term & 31);
                hit[u] = in && (word & bit);
                pr[u] = 0.0f;
                // the term's place in the query's list = the set bits below it (at most nq - 1, whatever the list holds)
                if (hit[u]) pr[u] = a.qw[q0 + before[w] + __popc(word & (bit - 1u))] * __int_as_float(cur[u].y);
            }
#pragma unroll
            for (int u = 0; u < FW_U; ++u) {
                unsigned m = (unsigned)(__ballot(hit[u]) >> gbase) & 0xffffu;  // the group's hits, lane order = term order
                while (__any(m != 0u)) {                                       // wave-uniform: every lane is there for the cross-lane read
                    const float v = __shfl(pr[u], gbase + (m ? __builtin_ctz(m) : 0));
                    if (m) { acc[u] = acc[u] + v; m &= m - 1u; }
                }
            }
#pragma unroll
            for (int u = 0; u < FW_U; ++u) cur[u] = nxt[u];
        }
#pragma unroll
        for (int u = 0; u < FW_U; ++u)
            if (l == u && slot0 + first + u < a.W) a.out[(size_t)q * a.ldo + slot0 + first + u] = len[u] < 0 ? -INFINITY : acc[u];
    }
}

struct FwdDocScoreArgs {
    const int64_t* foff; const int32_t* fterm; const int32_t* fpos;
    const int32_t* ptf; const double* idf;     // TFIDF
    const double* pval;                        // PVAL
    const int64_t* qoff; const int32_t* qterms;
    const int32_t* docs;                       // [Q][G] positions in this index; < 0 (or >= N): not in it
    double* out;                               // [Q][G]; -inf for a document that is not in this index
    int N, G; long total;                      // total = Q * G
};

// one thread per (query, listed document)
template <int MODE>
__global__ __launch_bounds__(256) void lexical_doc_scores_fwd_kernel(FwdDocScoreArgs a) {
    constexpr bool PVAL = MODE == BM25_PVAL;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int q = (int)(i / a.G);
    const int d = a.docs[i];
    if (d < 0 || d >= a.N) { a.out[i] = -__builtin_inf(); return; }
    double acc = 0.0;
    const int64_t r0 = a.foff[d], r1 = a.foff[d + 1];
    const int64_t p0 = a.qoff[q], p1 = a.qoff[q + 1];
    for (int64_t p = p0; p < p1; ++p) {        // terms in QUERY ORDER: the walk's addition order
        const int t = a.qterms[p];
        if (t < 0) continue;                   // out of vocabulary: contributes nothing
        const int64_t j = lower_bound_doc(a.fterm, r0, r1, t);     // (the search is the same over a row's ascending terms)
        if (j < r1 && a.fterm[j] == t) {
            const int e = a.fpos[j];
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

extern "C" int fz_sparse_fwd_max_vocab(void) { return FW_MAX_V; }

extern "C" int fz_sparse_fwd_pairs_f32(const int64_t* foff, const void* rows, int V, const int64_t* qoff, const int32_t* qterms, const float* qw,
                                       int Q, int N, const int64_t* cand, int ldc, const int32_t* cand_len, int W, int64_t id_base, float* out,
                                       int ldo, void* stream) {
    if (Q < 0 || N < 0 || W < 0 || V < 0 || ldc < W || ldo < W) return FZ_ERR_ARG;
    if ((Q != 0 && W != 0) && (!qoff || !cand || !out)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if ((Q != 0 && W != 0 && N != 0) && !foff) return FZ_ERR_ARG;
    if (V > FW_MAX_V || ((uintptr_t)rows % 8)) return FZ_ERR_UNSUPPORTED;
    if (Q == 0 || W == 0) return FZ_OK;
    FwdPairsArgs a{};
    a.foff = foff; a.rows = static_cast<const int2*>(rows); a.qoff = qoff; a.qterms = qterms; a.qw = qw; a.cand = cand; a.cand_len = cand_len;
    a.out = out; a.id_base = id_base; a.ldc = ldc; a.ldo = ldo; a.Q = Q; a.N = N; a.V = V; a.W = W;
    a.nblocks = (W + FW_SLOTS - 1) / FW_SLOTS;
    const long nblk = (long)Q * a.nblocks;
    if (nblk > 0x7fffffffL) return FZ_ERR_UNSUPPORTED;
    static unsigned long long lds_set = 0ull;
    if (int rc = raise_lds_limit((const void*)sparse_fwd_pairs_kernel, 2 * (FW_MAX_V / 8), lds_set)) return rc;
    const size_t lds_bytes = (size_t)(V > 0 ? (V + 31) / 32 : 1) * 2 * sizeof(uint32_t);      // the bitmap | the set bits before each word
    sparse_fwd_pairs_kernel<<<(unsigned)nblk, FW_THREADS, lds_bytes, as_stream(stream)>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

template <int MODE>
static int fds_launch(FwdDocScoreArgs& a, int Q, int G, hipStream_t st) {
    a.G = G; a.total = (long)Q * G;
    lexical_doc_scores_fwd_kernel<MODE><<<(unsigned)((a.total + 255) / 256), 256, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

// toff and pdoc are the inverted entries' arguments; the forward route does not read them
extern "C" int fz_bm25_doc_scores_fwd_pv_f64(const int64_t* toff, const int32_t* pdoc, const double* pval, const int64_t* foff, const int32_t* fterm,
                                             const int32_t* fpos, const int64_t* qoff, const int32_t* qterms, int Q, int N, const int32_t* docs, int G,
                                             double* out, void* stream) {
    (void)toff; (void)pdoc;
    if (Q < 0 || N < 0 || G < 1) return FZ_ERR_ARG;
    if (Q != 0 && (!pval || !foff || !fterm || !fpos || !qoff || !qterms || !docs || !out)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if (Q == 0) return FZ_OK;
    FwdDocScoreArgs a{};
    a.foff = foff; a.fterm = fterm; a.fpos = fpos; a.pval = pval; a.qoff = qoff; a.qterms = qterms; a.docs = docs; a.out = out; a.N = N;
    return fds_launch<BM25_PVAL>(a, Q, G, as_stream(stream));
}

extern "C" int fz_tfidf_doc_scores_fwd_f64(const int64_t* toff, const int32_t* pdoc, const int32_t* ptf, const double* idf, const int64_t* foff,
                                           const int32_t* fterm, const int32_t* fpos, const int64_t* qoff, const int32_t* qterms, int Q, int N,
                                           const int32_t* docs, int G, double* out, void* stream) {
    (void)toff; (void)pdoc;
    if (Q < 0 || N < 0 || G < 1) return FZ_ERR_ARG;
    if (Q != 0 && (!ptf || !idf || !foff || !fterm || !fpos || !qoff || !qterms || !docs || !out)) return FZ_ERR_ARG;
    if (Q == 0) return FZ_OK;
    FwdDocScoreArgs a{};
    a.foff = foff; a.fterm = fterm; a.fpos = fpos; a.ptf = ptf; a.idf = idf; a.qoff = qoff; a.qterms = qterms; a.docs = docs; a.out = out; a.N = N;
    return fds_launch<BM25_TFIDF>(a, Q, G, as_stream(stream));
}
