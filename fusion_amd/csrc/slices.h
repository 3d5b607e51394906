// slices.h -- what the "one workgroup = (query, slice of documents)" kernels over an inverted index have in common (bm25.hip,
// bm25_stream.hip, bm25_count.hip, sparse.hip, centroid.hip): the posting search, the per-index slice-offset table, the document range and
// its slice bounds, and the epilogues -- the score plane of the range, the streaming top-k's threshold filter in its place, or (float64)
// the count of the documents ranked before each of a few listed ones.  A scorer supplies its arguments, its walk (the per-posting
// reduction into the slice's LDS accumulators) and its slice size.
#pragma once
#include "common.h"

namespace fz {

__device__ __forceinline__ int64_t lower_bound_doc(const int32_t* __restrict__ pdoc, int64_t lo, int64_t hi, int doc) {
    while (lo < hi) {   // first e in [lo, hi) with pdoc[e] >= doc  (uniform: scalar loads)
        const int64_t mid = (lo + hi) >> 1;
        if (pdoc[mid] < doc) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The per-index table [rows][NS + 1]: out[r][s] = first entry of list r (entries [off[r], off[r+1]) of doc, ascending) whose document is
// >= s * grain; out[r][NS] = off[r + 1].  With it a workgroup reads its posting sub-ranges instead of searching for them.  (A template, so
// that only the files that build a table hold the kernel; static: each its own copy.)
template <typename Doc>
static __global__ void slice_offsets_kernel(const int64_t* __restrict__ off, const Doc* __restrict__ doc, int rows, int NS, int grain,
                                            int64_t* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)rows * (NS + 1)) return;
    const int r = (int)(i / (NS + 1)), s_ = (int)(i % (NS + 1));
    out[i] = s_ == NS ? off[r + 1] : lower_bound_doc(doc, off[r], off[r + 1], s_ * grain);
}

template <typename Doc>
inline int slice_offsets_launch(const int64_t* off, const Doc* doc, int rows, int N, int grain, int64_t* out, void* stream) {
    if (rows < 0 || N < 0) return FZ_ERR_ARG;
    if (rows == 0) return FZ_OK;
    if (!off || !out) return FZ_ERR_ARG;
    const int NS = N > 0 ? (N + grain - 1) / grain : 1;
    const long total = (long)rows * (NS + 1);
    slice_offsets_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(off, doc, rows, NS, grain, out);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

// The documents scored, [doc_lo, doc_hi) of an index of N: doc_lo a whole slice, doc_hi a whole slice or N.  NS: the row stride - 1 of the
// index's slice-offset table, ceil(N / its grain).
struct DocRange { int N, NS, doc_lo, doc_hi; };

inline bool range_ok(int N, int doc_lo, int doc_hi, int slice) {
    return N >= 0 && doc_lo >= 0 && doc_lo <= doc_hi && doc_hi <= N && doc_lo % slice == 0 && (doc_hi % slice == 0 || doc_hi == N);
}
inline DocRange doc_range(int N, int doc_lo, int doc_hi, int grain) { return DocRange{N, (N + grain - 1) / grain, doc_lo, doc_hi}; }
inline dim3 slice_grid(const DocRange& r, int slice, int Q) { return dim3((unsigned)((r.doc_hi - r.doc_lo + slice - 1) / slice), (unsigned)Q); }

// grid (slices of [doc_lo, doc_hi), Q): workgroup (x, q) scores the documents [d0, d1) of global slice doc_lo / SLICE + x, which is returned
__device__ __forceinline__ int slice_of(const DocRange r, int SLICE, int& d0, int& d1) {
    const int s = r.doc_lo / SLICE + (int)blockIdx.x;
    d0 = s * SLICE;
    d1 = (d0 + SLICE < r.doc_hi) ? d0 + SLICE : r.doc_hi;
    return s;
}

// plane epilogue: the slice's n scores to row q of scores [Q][lds], from column col0 (= d0 - doc_lo) on
template <typename T>
__device__ __forceinline__ void store_plane(const T* acc, int n, T* scores, int lds, int q, int col0) {
    T* __restrict__ row = scores + (size_t)q * lds + col0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) row[j] = acc[j];
}

// Where the filter epilogue puts what beats tau[q]: query q's candidate list cand_s / cand_i [Q][cap] of cand_len[q] entries (it counts
// past cap; nothing is stored there, *overflow is set instead).  id_base: the id of index document 0.
template <typename T>
struct FilterSink { const T* tau; T* cand_s; int64_t* cand_i; int32_t* cand_len; int32_t* overflow; int cap; int64_t id_base; };

// filter epilogue (the streaming top-k's rule, fz_dot_scores_filter_f32's): document d0 + j enters query q's candidates iff
// !(acc[j] <= tau[q]) -- a NaN is kept.  Per wave and 64 documents: ballot, ONE atomicAdd on cand_len[q] for the wave's survivors (none
// when there are none -- the usual case once the threshold has settled), each survivor stores at base + its rank in the ballot, never at
// or past cap; cand_len keeps counting.  Candidates arrive in no particular order: fz_topk_fold_*(unordered) restores "ties by ascending
// id".  The overflow flag is raised once per wave that dropped something (__any, lane 0): no barrier and no LDS of the epilogue's own, so a
// kernel's LDS budget -- centroid.hip's is exactly five workgroups per CU -- is its walk's alone.  Whole waves must reach this call.
template <typename T>
__device__ __forceinline__ void filter_candidates(const T* acc, int n, int d0, int q, const FilterSink<T>& f) {
    const T tq = f.tau[q];
    const int lane = threadIdx.x & 63;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;    // lanes under this one
    T* __restrict__ cs = f.cand_s + (size_t)q * f.cap;
    int64_t* __restrict__ ci = f.cand_i + (size_t)q * f.cap;
    bool over = false;
    for (int j0 = 0; j0 < n; j0 += blockDim.x) {                              // wave-uniform trip count: every lane takes part in the ballot
        const int j = j0 + (int)threadIdx.x;
        const T v = j < n ? acc[j] : T(0);
        const bool keep = j < n && !(v <= tq);
        const unsigned long long bal = __ballot(keep);
        if (bal == 0ull) continue;                                            // wave-uniform
        int base = 0;
        if (lane == 0) base = atomicAdd(f.cand_len + q, (int)__popcll(bal));
        base = __shfl(base, 0);
        if (keep) {
            const int pos = base + (int)__popcll(bal & below);
            if (pos < f.cap) {
                cs[pos] = v;
                ci[pos] = f.id_base + d0 + j;
            } else over = true;
        }
    }
    if (__any(over) && lane == 0) atomicExch(f.overflow, 1);                  // one per wave that dropped something
}

// What the counting epilogue compares against and adds to: per query G listed ("gold") documents, as (float64 score, global id) -- an id
// < 0 skips the gold -- and counts [Q][G] int32, ADDED to (the caller zeroes it).  id_base: the id of index document 0.
struct CountSink { const double* gold_scores; const int64_t* gold_ids; int32_t* counts; int G; int64_t id_base; };

constexpr int COUNT_GROUP = 8;   // golds compared per pass over the accumulators, at most (registers: a key and a position each)

// one register group of count_beaters: the ng <= GW golds gs / gi / out point at
template <int GW>
__device__ __forceinline__ void count_group(const double* acc, int n, int d0, const double* __restrict__ gs, const int64_t* __restrict__ gi,
                                            int32_t* __restrict__ out, int ng, int64_t id_base) {
    uint64_t gk[GW]; int gj[GW], cnt[GW];
    bool inside = false;                                                  // a gold's id falls among this slice's: workgroup-uniform
#pragma unroll
    for (int u = 0; u < GW; ++u) {
        gk[u] = 0ull; gj[u] = 0; cnt[u] = 0;                              // skipped / padding: key 0, which nothing is below
        if (u < ng) {
            const int64_t gid = gi[u];
            if (gid >= 0) {
                const int64_t at = gid - id_base - d0;                    // the gold's place in this slice, if it is one of its documents
                gk[u] = desc_key_f64(gs[u]);
                gj[u] = at < 0 ? 0 : (at > n ? n : (int)at);
                inside |= gj[u] > 0 && gj[u] < n;
            }
        }
    }
    if (!inside) {
        // every document's id is on one side of every gold's (the usual slice): "before" is key < gk, or key <= gk = key < gk + 1 where the
        // ids are all lower (no key is 2^64 - 1: the largest, -inf's, is 0xfff0...0) -- one 64-bit compare per (document, gold)
#pragma unroll
        for (int u = 0; u < GW; ++u) gk[u] += gj[u] > 0 ? 1ull : 0ull;
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            const uint64_t k = desc_key_f64(acc[j]);
#pragma unroll
            for (int u = 0; u < GW; ++u) cnt[u] += k < gk[u] ? 1 : 0;
        }
    } else {
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            const uint64_t k = desc_key_f64(acc[j]);
#pragma unroll
            for (int u = 0; u < GW; ++u) cnt[u] += (k < gk[u] || (k == gk[u] && j < gj[u])) ? 1 : 0;
        }
    }
#pragma unroll
    for (int u = 0; u < GW; ++u) {
        const int total = wave_reduce_sum(cnt[u]);
        if ((threadIdx.x & 63) == 0 && total != 0) atomicAdd(out + u, total);   // (total != 0 only where u < ng)
    }
}

// counting epilogue (float64 scores): counts[q][g] += the number of documents d0 + j, j < n, that the stable descending float64 ranking
// (sort_rows_desc: desc_key_f64 ascending, ties to the ascending id) puts BEFORE gold g = (gs, gid): desc_key_f64(acc[j]) <
// desc_key_f64(gs), or equal keys and id_base + d0 + j < gid.  The id test is j < clamp(gid - id_base - d0, 0, n): 32-bit inside the
// slice, and right for a gold of another slice, range or shard (every j, or none); a gold never counts itself.  Golds in register groups
// of at most COUNT_GROUP (1, 2, 4 or 8 wide: a query with one gold pays for one): acc is read once per group, the gold scores and ids are
// uniform (scalar loads).  Per gold a lane-sum over the wave, then one atomicAdd per (wave, gold) with a non-zero count -- integer adds:
// any grid, range split or run gives the same counts.  No LDS and no barrier of the epilogue's own.  Whole waves must reach this call.
__device__ __forceinline__ void count_beaters(const double* acc, int n, int d0, int q, const CountSink& c) {
    const double* gs = c.gold_scores + (size_t)q * c.G;
    const int64_t* gi = c.gold_ids + (size_t)q * c.G;
    int32_t* out = c.counts + (size_t)q * c.G;
    for (int g0 = 0; g0 < c.G; g0 += COUNT_GROUP) {
        const int ng = c.G - g0 < COUNT_GROUP ? c.G - g0 : COUNT_GROUP;
        if (ng > 4) count_group<8>(acc, n, d0, gs + g0, gi + g0, out + g0, ng, c.id_base);
        else if (ng > 2) count_group<4>(acc, n, d0, gs + g0, gi + g0, out + g0, ng, c.id_base);
        else if (ng > 1) count_group<2>(acc, n, d0, gs + g0, gi + g0, out + g0, ng, c.id_base);
        else count_group<1>(acc, n, d0, gs + g0, gi + g0, out + g0, ng, c.id_base);
    }
}

}  // namespace fz
