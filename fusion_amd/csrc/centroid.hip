// centroid.hip -- the candidate stage of ColBERT's first-stage search at corpus scale (hybrid.py:108-137: colbert-ai generates candidates
// from token centroids, then scores them exactly; the exact part is rerank.hip).
//
// Every document token carries the id of its nearest centroid; per centroid c the index lists the DISTINCT documents that hold it,
// ascending: [coff[c], coff[c+1]) of cdoc.  A query is its probe table, token-major: token i's nprobe best centroids pc[i * nprobe + j]
// (-1 = padding) with their scores ps.  The candidate score of document d is
//      approx(d) = ((+0.0 + m_i1) + m_i2) + ...   over the tokens i, ascending, with at least one probed centroid among d's codes,
//      m_i      = the largest ps over token i's probes whose list holds d
// in float32: a max (order-independent) inside a token, one add per token in a fixed order -- defined bit for bit, the same for a range of
// documents as for the whole index and for any grid.  A token that does not hit adds nothing; an untouched document scores +0.0.
// Probe scores are finite by contract (a NaN's bit pattern has no place in the key order below).
//
// One workgroup = (query, slice of CT_SLICE documents), the structure of sparse.hip's walk with another reduction.  Per token:
//   phase 0  every probe's list segment is walked (one wave per probe) with atomicMax on an LDS array of order-preserving unsigned keys
//            (0 = "no hit"): integer max, so deterministic in any arrival order;
//   barrier
//   phase 1  the same segments again: atomicExch(key, 0) hands a document's key to exactly ONE of the lanes that reach it, and that lane
//            does acc += decode(key) -- no float atomics, and the keys are back to "no hit" for the next token;
//   barrier
// Two barriers per token rather than one per list: inside a slice the lists are short (about 4 entries at 70 tokens per document and
// 65,536 centroids).  The slice-offset table, the document range and the plane and filter epilogues are slices.h's.
#include "slices.h"

namespace fz {

// 3,584 accumulators + 3,584 keys (28 KiB) + the probe table (4 KiB) = 32 KiB of LDS and 256 threads per workgroup: five workgroups
// (20 waves) share a CU's 160 KiB.  The walk is latency-bound -- a token's probes are a handful of short segments, one wave each -- so
// what hides a workgroup's barriers is its neighbours, not its own width.
constexpr int CT_SLICE = 3584;
constexpr int CT_THREADS = 256;
constexpr int CT_PROBES = 256;      // probes whose list ranges are resolved per batch

struct CentroidArgs {
    const int64_t* coff; const int32_t* cdoc;                      // index: documents of centroid c are [coff[c], coff[c+1]), ascending, distinct
    const int64_t* slice_off;                                      // nullable [K][NS + 1]: first entry of centroid c with document >= s * CT_SLICE
    const int32_t* pc; const float* ps;                            // probes [Q][Lq * nprobe], token-major; pc < 0: padding
    int Lq, nprobe, K;
    DocRange r;                                                    // the documents scored (slice_off's row stride is r.NS + 1)
    float* scores; int lds;                                        // plane form: [Q][lds], column j = document doc_lo + j
    FilterSink<float> f;                                           // filter form (fz_centroid_scores_filter_f32): no plane
};

// float -> unsigned key, larger float <=> larger key; no finite float maps to 0, the "no hit" mark
__device__ __forceinline__ uint32_t ct_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ct_key_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// probes [off, off + cnt) of the query's table -> the segment of each one's list inside [d0, d1) and its score's key
__device__ __forceinline__ void ct_resolve(const CentroidArgs& a, const int32_t* __restrict__ pcq, const float* __restrict__ psq, int off, int cnt,
                                           int s, int d0, int d1, int64_t* s_e0, int32_t* s_n, uint32_t* s_k) {
    if ((int)threadIdx.x < cnt) {
        const int c = pcq[off + threadIdx.x];
        int64_t e0 = 0, e1 = 0;
        if (c >= 0 && c < a.K) {
            if (a.slice_off) {
                const int64_t* so = a.slice_off + (size_t)c * (a.r.NS + 1) + s;
                e0 = so[0]; e1 = so[1];
            } else {
                e0 = lower_bound_doc(a.cdoc, a.coff[c], a.coff[c + 1], d0);
                e1 = lower_bound_doc(a.cdoc, e0, a.coff[c + 1], d1);
            }
        }
        s_e0[threadIdx.x] = e0; s_n[threadIdx.x] = e1 > e0 ? (int32_t)(e1 - e0) : 0; s_k[threadIdx.x] = ct_key(psq[off + threadIdx.x]);
    }
}

// one phase over the resolved probes [base, base + cnt) of ONE token: wave w takes probes w, w + waves, ...
template <int PHASE>
__device__ __forceinline__ void ct_segments(const CentroidArgs& a, float* ct_acc, uint32_t* ct_keys, const int64_t* s_e0, const int32_t* s_n,
                                            const uint32_t* s_k, int base, int cnt, int d0, int n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (int p = wave; p < cnt; p += waves) {
        const int len = s_n[base + p];
        const int32_t* __restrict__ seg = a.cdoc + s_e0[base + p];
        const uint32_t k = s_k[base + p];
        for (int x = lane; x < len; x += 64) {
            const int d = seg[x] - d0;
            if ((unsigned)d >= (unsigned)n) continue;       // an index whose lists are not ascending: never leave the slice's arrays
            if (PHASE == 0) atomicMax(ct_keys + d, k);
            else {
                const uint32_t got = atomicExch(ct_keys + d, 0u);
                if (got) ct_acc[d] = ct_acc[d] + ct_key_inv(got);     // the one lane that took the key adds this token's max
            }
        }
    }
}

// The walk of both epilogues: query q against the documents [d0, d1) of global slice s; on return ct_acc[0 .. d1 - d0) holds the scores
// (after a barrier).  nprobe <= CT_PROBES: the table is resolved for CT_PROBES / nprobe whole tokens at a time.  A wider token is
// resolved CT_PROBES probes at a time, once for each phase.
__device__ __forceinline__ void centroid_walk(const CentroidArgs& a, float* ct_acc, uint32_t* ct_keys, int64_t* s_e0, int32_t* s_n, uint32_t* s_k,
                                              int q, int s, int d0, int d1) {
    const int n = d1 - d0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) { ct_acc[j] = 0.0f; ct_keys[j] = 0u; }
    const int P = a.nprobe;
    const int32_t* __restrict__ pcq = a.pc + (size_t)q * a.Lq * P;
    const float* __restrict__ psq = a.ps + (size_t)q * a.Lq * P;
    if (P <= CT_PROBES) {
        const int T = CT_PROBES / P;
        for (int t0 = 0; t0 < a.Lq; t0 += T) {
            const int nt = a.Lq - t0 < T ? a.Lq - t0 : T;
            __syncthreads();   // arrays zeroed / the previous batch's table no longer read
            ct_resolve(a, pcq, psq, t0 * P, nt * P, s, d0, d1, s_e0, s_n, s_k);
            __syncthreads();
            for (int i = 0; i < nt; ++i) {          // tokens in ascending order: the order of the adds
                ct_segments<0>(a, ct_acc, ct_keys, s_e0, s_n, s_k, i * P, P, d0, n);
                __syncthreads();
                ct_segments<1>(a, ct_acc, ct_keys, s_e0, s_n, s_k, i * P, P, d0, n);
                __syncthreads();
            }
        }
    } else {
        for (int i = 0; i < a.Lq; ++i) {
#pragma unroll 1
            for (int phase = 0; phase < 2; ++phase) {
                for (int p0 = 0; p0 < P; p0 += CT_PROBES) {
                    const int cnt = P - p0 < CT_PROBES ? P - p0 : CT_PROBES;
                    __syncthreads();
                    ct_resolve(a, pcq, psq, i * P + p0, cnt, s, d0, d1, s_e0, s_n, s_k);
                    __syncthreads();
                    if (phase == 0) ct_segments<0>(a, ct_acc, ct_keys, s_e0, s_n, s_k, 0, cnt, d0, n);
                    else ct_segments<1>(a, ct_acc, ct_keys, s_e0, s_n, s_k, 0, cnt, d0, n);
                }
                __syncthreads();   // the token's max is complete / its adds are done
            }
        }
    }
    __syncthreads();
}

// One workgroup's work in either form.  FILTER: the streaming top-k's threshold filter in place of the plane store.
template <bool FILTER>
__device__ __forceinline__ void centroid_scores(const CentroidArgs& a) {
    __shared__ __attribute__((aligned(16))) float ct_acc[CT_SLICE];
    __shared__ uint32_t ct_keys[CT_SLICE];
    __shared__ int64_t s_e0[CT_PROBES];
    __shared__ int32_t s_n[CT_PROBES];
    __shared__ uint32_t s_k[CT_PROBES];
    const int q = blockIdx.y;
    int d0, d1;
    const int s = slice_of(a.r, CT_SLICE, d0, d1);
    centroid_walk(a, ct_acc, ct_keys, s_e0, s_n, s_k, q, s, d0, d1);
    if constexpr (FILTER) filter_candidates(ct_acc, d1 - d0, d0, q, a.f);
    else store_plane(ct_acc, d1 - d0, a.scores, a.lds, q, d0 - a.r.doc_lo);
}

__global__ __launch_bounds__(CT_THREADS) void centroid_scores_kernel(CentroidArgs a) { centroid_scores<false>(a); }
__global__ __launch_bounds__(CT_THREADS) void centroid_scores_filter_kernel(CentroidArgs a) { centroid_scores<true>(a); }

}  // namespace fz

using namespace fz;

extern "C" int fz_centroid_slice_docs(void) { return CT_SLICE; }

// fz_sparse_slice_offsets at this walk's grain (CT_SLICE is not SP_SLICE)
extern "C" int fz_centroid_slice_offsets(const int64_t* coff, const int32_t* cdoc, int K, int N, int64_t* out, void* stream) {
    return slice_offsets_launch(coff, cdoc, K, N, CT_SLICE, out, stream);
}

// [doc_lo, doc_hi) of an index of N documents: doc_lo a whole slice, doc_hi a whole slice or N; a probe table of Lq >= 1 tokens x nprobe >= 1
static bool cen_args_ok(int Q, int Lq, int nprobe, int N, int K, int doc_lo, int doc_hi) {
    return Q >= 0 && Lq >= 1 && nprobe >= 1 && (int64_t)Lq * nprobe <= INT32_MAX && K >= 0 &&
           range_ok(N, doc_lo, doc_hi, CT_SLICE);
}

static CentroidArgs cen_args(const int64_t* coff, const int32_t* cdoc, const int64_t* slice_off, const int32_t* pc, const float* ps, int Lq, int nprobe,
                            int K, int N, int doc_lo, int doc_hi) {
    CentroidArgs a{};
    a.coff = coff; a.cdoc = cdoc; a.slice_off = slice_off; a.pc = pc; a.ps = ps; a.Lq = Lq; a.nprobe = nprobe; a.K = K;
    a.r = doc_range(N, doc_lo, doc_hi, CT_SLICE);
    return a;
}

static int cen_launch(const CentroidArgs& a, int Q, bool filter, hipStream_t st) {
    const dim3 grid = slice_grid(a.r, CT_SLICE, Q);
    if (filter) centroid_scores_filter_kernel<<<grid, CT_THREADS, 0, st>>>(a);
    else centroid_scores_kernel<<<grid, CT_THREADS, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_centroid_scores_range_f32(const int64_t* coff, const int32_t* cdoc, const int64_t* slice_off, const int32_t* pc, const float* ps,
                                            int Q, int Lq, int nprobe, int N, int K, int doc_lo, int doc_hi, float* scores, int lds,
                                            void* stream) {
    if (!cen_args_ok(Q, Lq, nprobe, N, K, doc_lo, doc_hi) || lds < doc_hi - doc_lo) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;   // empty tensors carry null pointers
    if (!coff || !pc || !ps || !scores) return FZ_ERR_ARG;
    CentroidArgs a = cen_args(coff, cdoc, slice_off, pc, ps, Lq, nprobe, K, N, doc_lo, doc_hi);
    a.scores = scores; a.lds = lds;
    return cen_launch(a, Q, false, as_stream(stream));
}

extern "C" int fz_centroid_scores_filter_f32(const int64_t* coff, const int32_t* cdoc, const int64_t* slice_off, const int32_t* pc, const float* ps,
                                             int Q, int Lq, int nprobe, int N, int K, int doc_lo, int doc_hi, int64_t id_base, const float* tau,
                                             float* cand_scores, int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream) {
    if (!cen_args_ok(Q, Lq, nprobe, N, K, doc_lo, doc_hi) || cap <= 0) return FZ_ERR_ARG;
    if (Q == 0 || doc_hi == doc_lo) return FZ_OK;
    if (!coff || !pc || !ps || !tau || !cand_scores || !cand_ids || !cand_len || !overflow) return FZ_ERR_ARG;
    CentroidArgs a = cen_args(coff, cdoc, slice_off, pc, ps, Lq, nprobe, K, N, doc_lo, doc_hi);
    a.f = {tau, cand_scores, cand_ids, cand_len, overflow, cap, id_base};
    return cen_launch(a, Q, true, as_stream(stream));
}
