// lists_collapse.hip -- passage lists to document lists (MaxP), and the exact MaxP score of candidate documents (gfx950).
//
// A long document is indexed as PASSAGES; the corpus-scale searches then return, per query, a top-k list of passages in
// (score desc, id asc) order.  A document's score is that of its best passage (MaxP).  Three kernels:
//
// lists_collapse_kernel: one passage list per query -> one document list.  The walk is the id join's (lists.h: ONE 1,024-THREAD
//   WORKGROUP PER QUERY, chunks of 1,024 entries, the open-addressing table over the row's ids in LDS and its hash, the block scan
//   that turns "new" flags into first-insertion columns), keyed by the DOCUMENT id group_of[passage - id_base] + doc_id_base.  The
//   list is ranked, so a document's first occurrence IS its best passage and the first-insertion order of the documents IS the MaxP
//   ranking: the entry that opens a column copies its own (document id, score bits, passage id) there, and nothing is reduced or
//   sorted afterwards.  Equal scores keep list order = ascending passage id = (group_of non-decreasing) ascending document id.
//
//   The placement step is this file's own, not lj_place: lj_place gives two entries of ONE chunk that carry the same id two columns
//   (that is its duplicate case, and which of them the table then lists depends on which compare-and-swap lands first), and here a
//   repeated document inside a chunk is the normal case and the EARLIEST entry has to win.  Per chunk:
//     1. look the document up (lj_find, read only); an entry whose document is not in the table is a candidate and parks its id
//        in uid[base + thread] -- a provisional column past the row's columns so far (base + live entries <= len <= cap)
//     2. the candidates claim the document's slot: compare-and-swap EMPTY -> provisional column, linear probing; onto a slot that
//        already holds the same document, atomicMin -- the lowest provisional column, i.e. the earliest entry, owns the slot whatever
//        order the atomics arrive in
//     3. the owners are the chunk's new documents: ballot + block scan -> column = base + exclusive prefix; the owner rewrites its
//        slot and uid[column] to the final column and writes the outputs
//   with a barrier after each step and one that closes the chunk.  Two runs give the same bytes.
//   Checks (flag word = first int32 of the workspace): bit 0 a listed passage id outside [id_base, id_base + P) (the entry is
//   skipped), bit 1 a row that is not non-increasing, !(s[r-1] >= s[r]) on scores (and on scores64 when given): NaN included.
//   LDS: lj_plan's for cap = n (ids [n] int64 + table + 16 wave totals).
//
// group_expand_kernel: candidate DOCUMENT ids [Q][W] -> their passages [Q][ldp], slot 0's first, with the segment offsets
//   seg [Q][W + 1]: one 256-thread workgroup per query, a block scan over the slots' passage counts (CSR poff).  The existing pair
//   kernels score the passages; group_max_kernel (one thread per (query, slot)) then takes the maximum over each segment: the winning
//   entry's own bits and the passage id of the FIRST maximum (passages of a segment ascend: the lowest id among equals).
#include "lists.h"

namespace fz {

constexpr int32_t LC_BAD_ID = 1, LC_UNORDERED = 2;   // the flag word's bits
constexpr uint32_t LC_LISTED = 1u << 16;             // every slot carries the one system's bit: lists.h's slot layout

struct CollapseArgs {
    const int32_t* lens[1];                // (lens, n, S, cap, table_size: what lj_open and lj_len read -- one system)
    int n[1];
    int S, cap, table_size;
    const int64_t* ids;                    // [Q][ld] passage ids
    const float* scores;                   // [Q][ld]
    const double* scores64;                // [Q][ld] or null
    const int32_t* group_of;               // [P]
    int64_t P, id_base, doc_id_base;
    int ld, ld_out;
};

__global__ __launch_bounds__(LJ_T) void lists_collapse_kernel(CollapseArgs a, int64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                              double* __restrict__ out_scores64, int64_t* __restrict__ out_best,
                                                              int32_t* __restrict__ out_len, int32_t* __restrict__ flag) {
    constexpr int NW = LJ_T / 64;
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    LjRow j = lj_open(a, q);
    const int len = j.total;
    const size_t irow = (size_t)q * a.ld, orow = (size_t)q * a.ld_out;
    int base = 0;
    int32_t bad = 0;
    for (int r0 = 0; r0 < len; r0 += LJ_T) {           // block-uniform: every barrier below is reached by all threads
        const int r = r0 + t;
        int64_t pid = 0, did = 0;
        uint32_t slot = 0;
        bool cand = false;
        if (r < len) {
            pid = a.ids[irow + r];
            const uint64_t p = (uint64_t)pid - (uint64_t)a.id_base;
            if (p >= (uint64_t)a.P) {
                bad |= LC_BAD_ID;
            } else {
                did = (int64_t)a.group_of[p] + a.doc_id_base;
                cand = lj_find(j, did, slot) == LJ_EMPTY;
                if (cand) j.uid[base + t] = did;          // base + t < r0 + (len - r0) <= cap
            }
            if (r >= 1) {
                if (!(a.scores[irow + r - 1] >= a.scores[irow + r])) bad |= LC_UNORDERED;
                if (a.scores64 && !(a.scores64[irow + r - 1] >= a.scores64[irow + r])) bad |= LC_UNORDERED;
            }
        }
        __syncthreads();
        const uint32_t mine = (uint32_t)(base + t) | LC_LISTED;
        if (cand) {
            for (;;) {                                    // from the empty slot the look-up ended on: what lies before it holds other ids
                const uint32_t old = atomicCAS(&j.table[slot], LJ_EMPTY, mine);
                if (old == LJ_EMPTY) break;
                if (j.uid[old & LJ_COL] == did) { atomicMin(&j.table[slot], mine); break; }
                slot = (slot + 1) & j.mask;
            }
        }
        __syncthreads();
        const bool isnew = cand && j.table[slot] == mine;
        const unsigned long long bal = __ballot(isnew);
        const int below = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) j.wtot[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) { const int c = (int)j.wtot[i]; if (i < wv) woff += c; tot += c; }
        if (isnew) {
            const int col = base + woff + below;          // <= base + t: below the provisional columns still parked, none of which is read again
            j.uid[col] = did;
            j.table[slot] = (uint32_t)col | LC_LISTED;
            out_ids[orow + col] = did;
            out_scores[orow + col] = a.scores[irow + r];
            if (out_scores64) out_scores64[orow + col] = a.scores64[irow + r];
            out_best[orow + col] = pid;
        }
        base += tot;
        __syncthreads();   // the chunk's documents are in place before the next chunk looks them up
    }
    for (int c = base + t; c < a.ld_out; c += LJ_T) {    // base <= len <= n <= ld_out
        out_ids[orow + c] = -1;
        out_scores[orow + c] = -INFINITY;
        if (out_scores64) out_scores64[orow + c] = -(double)INFINITY;
        out_best[orow + c] = -1;
    }
    if (t == 0) out_len[q] = base;
    if (bad) atomicOr(flag, bad);
}

constexpr int GE_T = 256;

__global__ __launch_bounds__(GE_T) void group_expand_kernel(const int64_t* __restrict__ cand, int ld, const int32_t* __restrict__ cand_len,
                                                            int W, const int64_t* __restrict__ poff, int64_t D, int64_t id_base,
                                                            int64_t doc_id_base, int64_t* __restrict__ pcand, int ldp,
                                                            int32_t* __restrict__ seg, int32_t* __restrict__ pcand_len,
                                                            int32_t* __restrict__ flag) {
    constexpr int NW = GE_T / 64;
    __shared__ long long wtot[NW];
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int len = cand_len ? min(max(cand_len[q], 0), W) : W;
    const int64_t* __restrict__ crow = cand + (size_t)q * ld;
    int64_t* __restrict__ prow = pcand + (size_t)q * ldp;
    int32_t* __restrict__ srow = seg + (size_t)q * (W + 1);
    long long run = 0;                                   // the passages of the slots before this chunk (block-uniform)
    for (int w0 = 0; w0 < W; w0 += GE_T) {
        const int w = w0 + t;
        long long first = 0, cnt = 0;
        if (w < len) {
            const int64_t id = crow[w];
            const uint64_t d = (uint64_t)id - (uint64_t)doc_id_base;
            if (id >= 0 && d < (uint64_t)D) {
                first = poff[d];
                cnt = max(poff[d + 1] - first, 0ll);
            }
        }
        long long incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wtot[wv] = incl;
        __syncthreads();
        long long woff = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) { const long long c = wtot[i]; if (i < wv) woff += c; tot += c; }
        const long long at = run + woff + incl - cnt;
        if (w < W) srow[w] = (int32_t)min(at, (long long)ldp);
        for (long long i = 0; i < cnt && at + i < ldp; ++i) prow[at + i] = first + i + id_base;
        run += tot;
        __syncthreads();   // the wave totals are read before the next chunk writes them
    }
    const int filled = (int)min(run, (long long)ldp);
    for (int c = filled + t; c < ldp; c += GE_T) prow[c] = -1;
    if (t == 0) {
        srow[W] = filled;
        pcand_len[q] = filled;
        if (run > ldp) atomicOr(flag, 1);                 // the row's passages do not fit: the segments past ldp are cut short
    }
}

template <typename T>
__global__ __launch_bounds__(256) void group_max_kernel(const T* __restrict__ ps, int ld_s, const int64_t* __restrict__ pcand, int ldp,
                                                        const int32_t* __restrict__ seg, const int32_t* __restrict__ cand_len, int W,
                                                        int Q, T* __restrict__ out, int64_t* __restrict__ best, int ld_out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)Q * W) return;
    const int q = (int)(g / W), w = (int)(g % W);
    T top = -(T)INFINITY;
    int64_t bid = -1;
    if (!cand_len || w < cand_len[q]) {
        const int lo = min(max(seg[(size_t)q * (W + 1) + w], 0), ldp), hi = min(seg[(size_t)q * (W + 1) + w + 1], ldp);
        const T* __restrict__ srow = ps + (size_t)q * ld_s;
        int at = -1;
        for (int i = lo; i < hi; ++i) {
            const T v = srow[i];
            if (at < 0 || v > top) { top = v; at = i; }   // the first maximum, with its own bits
        }
        if (at >= 0) bid = pcand[(size_t)q * ldp + at];
    }
    out[(size_t)q * ld_out + w] = top;
    best[(size_t)q * ld_out + w] = bid;
}

}  // namespace fz

using namespace fz;

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" size_t fz_lists_collapse_workspace_bytes(int Q) { return Q < 0 ? 0 : 16; }   // the flag word (int32 at offset 0)

extern "C" int fz_lists_collapse(const int64_t* ids, const float* scores, const double* scores64, const int32_t* lens, int ld, int n,
                                 int Q, const int32_t* group_of, int64_t P, int64_t id_base, int64_t doc_id_base, int64_t* out_ids,
                                 float* out_scores, double* out_scores64, int64_t* out_best, int32_t* out_len, int ld_out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0) return FZ_ERR_ARG;
    const int32_t n_h[1] = {n}, ld_h[1] = {ld};
    LjPlan plan;
    int rc = lj_plan(n_h, ld_h, 1, Q, ld_out, plan);     // n < 0, ld < n, Q < 0: ARG; n over the capacity: UNSUPPORTED; ld_out < n: ARG
    if (rc != FZ_OK) return rc;
    if (Q == 0 || n == 0) return FZ_OK;                   // nothing to collapse: nothing launched, nothing written
    if (!ids || !scores || !lens || !out_ids || !out_scores || !out_best || !out_len || (P > 0 && !group_of)) return FZ_ERR_ARG;
    if ((scores64 == nullptr) != (out_scores64 == nullptr)) return FZ_ERR_ARG;
    if (!workspace || workspace_bytes < fz_lists_collapse_workspace_bytes(Q)) return FZ_ERR_WORKSPACE;
    CollapseArgs a{};
    a.lens[0] = lens; a.n[0] = n; a.S = 1; a.cap = plan.cap; a.table_size = plan.table_size;
    a.ids = ids; a.scores = scores; a.scores64 = scores64; a.group_of = group_of;
    a.P = P; a.id_base = id_base; a.doc_id_base = doc_id_base; a.ld = ld; a.ld_out = ld_out;
    static unsigned long long done = 0ull;
    int32_t* flag = reinterpret_cast<int32_t*>(workspace);
    hipStream_t st = as_stream(stream);
    rc = lj_prepare((const void*)lists_collapse_kernel, plan.lds, done, flag, st);
    if (rc != FZ_OK) return rc;
    lists_collapse_kernel<<<Q, LJ_T, plan.lds, st>>>(a, out_ids, out_scores, out_scores64, out_best, out_len, flag);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" size_t fz_group_expand_workspace_bytes(int Q) { return Q < 0 ? 0 : 16; }     // the overflow flag (int32 at offset 0)

extern "C" int fz_group_expand(const int64_t* cand, int ld, const int32_t* cand_len, int W, int Q, const int64_t* poff, int64_t D,
                               int64_t id_base, int64_t doc_id_base, int64_t* pcand, int ldp, int32_t* seg, int32_t* pcand_len,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (Q < 0 || W < 0 || ld < W || D < 0 || ldp < 0) return FZ_ERR_ARG;
    if (Q == 0) return FZ_OK;
    if ((W > 0 && !cand) || !poff || (ldp > 0 && !pcand) || !seg || !pcand_len) return FZ_ERR_ARG;
    if (!workspace || workspace_bytes < fz_group_expand_workspace_bytes(Q)) return FZ_ERR_WORKSPACE;
    int32_t* flag = reinterpret_cast<int32_t*>(workspace);
    hipStream_t st = as_stream(stream);
    FZ_HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    group_expand_kernel<<<Q, GE_T, 0, st>>>(cand, ld, cand_len, W, poff, D, id_base, doc_id_base, pcand, ldp, seg, pcand_len, flag);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

template <typename T>
static int group_max(const T* pscores, int ld_s, const int64_t* pcand, int ldp, const int32_t* seg, const int32_t* cand_len, int W, int Q,
                     T* out, int64_t* best, int ld_out, void* stream) {
    if (Q < 0 || W < 0 || ldp < 0 || ld_s < ldp || ld_out < W) return FZ_ERR_ARG;
    if (Q == 0 || W == 0) return FZ_OK;
    if ((ldp > 0 && (!pscores || !pcand)) || !seg || !out || !best) return FZ_ERR_ARG;
    const long long blocks = ((long long)Q * W + 255) / 256;
    if (blocks > 0x7fffffffll) return FZ_ERR_UNSUPPORTED;
    group_max_kernel<T><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(pscores, ld_s, pcand, ldp, seg, cand_len, W, Q, out, best, ld_out);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_group_max_f32(const float* pscores, int ld_s, const int64_t* pcand, int ldp, const int32_t* seg, const int32_t* cand_len,
                                int W, int Q, float* out, int64_t* best, int ld_out, void* stream) {
    return group_max<float>(pscores, ld_s, pcand, ldp, seg, cand_len, W, Q, out, best, ld_out, stream);
}

extern "C" int fz_group_max_f64(const double* pscores, int ld_s, const int64_t* pcand, int ldp, const int32_t* seg, const int32_t* cand_len,
                                int W, int Q, double* out, int64_t* best, int ld_out, void* stream) {
    return group_max<double>(pscores, ld_s, pcand, ldp, seg, cand_len, W, Q, out, best, ld_out, stream);
}
