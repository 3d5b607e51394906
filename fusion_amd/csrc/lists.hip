// lists.hip -- fusion of top-k LISTS: per-query id join (gfx950).
//
// The fusion kernels of fuse.hip work on planes indexed by corpus position.  A corpus-scale search returns something else: per
// query k (score, int64 global id) pairs per system, and per query the union of S such lists is at most S x k ids out of
// millions.  This file joins them where they are: ONE WORKGROUP PER QUERY, the union of the row's ids and an open-addressing
// table over it in LDS, no plane whose width depends on the corpus or on the batch.
//
// Semantics (hybrid.py:293-307, restated by oracle.fuse_lists): the fused dict receives system 0's entries in list order, then
// those of system 1 that no earlier system listed, and so on -- that first-insertion order is the COLUMN order of the outputs,
// so the stable row sort on out_scores with row_len = out_len breaks ties exactly as the reference's sorted() does.  The fused
// score of a column is 0 + c_s1 + c_s2 + ... over the systems that list the id, added in system order.
//
// The walk that turns the lists into columns (steps 1-3, the LDS layout) is lists.h's.  This kernel's step 4, accumulate: a new
// column is written (0 + c), a hit column is read, added to and written back -- entries of one system hit distinct columns, and
// the barrier that closes the chunk orders the systems.  The accumulators live in the output row.
#include "lists.h"

namespace fz {

struct JoinArgs {
    const int64_t* ids[FZ_MAX_SYSTEMS];
    const int32_t* lens[FZ_MAX_SYSTEMS];
    const void* values[FZ_MAX_SYSTEMS];    // wsum: float32 planes, or float64 where bit s of f64_mask is set
    double w[FZ_MAX_SYSTEMS];
    int n[FZ_MAX_SYSTEMS];                 // list width (lens are clamped to it)
    int ld[FZ_MAX_SYSTEMS];                // row stride of ids[s] and values[s], in elements
    int S, ld_out, cap, table_size;
    unsigned f64_mask, narrow_mask;
};

// METHOD: FZ_LISTS_RRF / FZ_LISTS_BCF / FZ_LISTS_WSUM_F32 / FZ_LISTS_WSUM_F64.  ACC = float for WSUM_F32, double otherwise.
template <int METHOD, typename ACC>
__global__ __launch_bounds__(LJ_T) void lists_join_kernel(JoinArgs a, int64_t* __restrict__ out_ids, ACC* __restrict__ out_scores,
                                                          int32_t* __restrict__ out_len, int32_t* __restrict__ dup_flag) {
    const int q = blockIdx.x;
    LjRow j = lj_open(a, q);
    if (j.total == 0) {
        if (threadIdx.x == 0) out_len[q] = 0;
        return;
    }
    int64_t* __restrict__ orow = out_ids + (size_t)q * a.ld_out;
    ACC* __restrict__ srow = out_scores + (size_t)q * a.ld_out;
    const unsigned narrow_eff = a.narrow_mask & ~a.f64_mask;
    int base = 0;
    bool dup = false;
    for (int s = 0; s < a.S; ++s) {
        const int len = lj_len(a, s, q);
        const int64_t* __restrict__ idrow = a.ids[s] + (size_t)q * a.ld[s];
        for (int r0 = 0; r0 < len; r0 += LJ_T) {
            const int r = r0 + threadIdx.x;
            const bool live = r < len;
            const LjPlaced p = lj_place(j, live, live ? idrow[r] : 0, 1u << (16 + s), orow, base, dup);
            const int col = p.col;
            const bool isnew = p.isnew;
            if (live) {
                if constexpr (METHOD == FZ_LISTS_RRF || METHOD == FZ_LISTS_BCF) {
                    double c;
                    if constexpr (METHOD == FZ_LISTS_RRF) c = 1.0 / (double)(60 + r + 1);              // hybrid.py:252
                    else { const double n = (double)len; c = (n - (double)r + 1.0) / n; }              // hybrid.py:249 (sic)
                    srow[col] = (isnew ? 0.0 : srow[col]) + c;
                } else if constexpr (METHOD == FZ_LISTS_WSUM_F32) {
                    const float t = reinterpret_cast<const float*>(a.values[s])[(size_t)q * a.ld[s] + r];
                    const float prod = t * (float)a.w[s];
                    srow[col] = (isnew ? 0.0f : srow[col]) + prod;
                } else {   // fuse_wsum_kernel's promotion rule, per column
                    const bool p64 = (a.f64_mask >> s) & 1u;
                    const bool narrow = (narrow_eff >> s) & 1u;
                    const double v = p64 ? reinterpret_cast<const double*>(a.values[s])[(size_t)q * a.ld[s] + r]
                                         : (double)reinterpret_cast<const float*>(a.values[s])[(size_t)q * a.ld[s] + r];
                    const double w = narrow ? (double)(float)a.w[s] : a.w[s];
                    double prod = v * w;
                    if (narrow) prod = (double)(float)prod;
                    const bool wide = !narrow || (p.before & ~narrow_eff) != 0u;
                    double acc = (isnew ? 0.0 : srow[col]) + prod;
                    if (!wide) acc = (double)(float)acc;
                    srow[col] = acc;
                }
            }
            __syncthreads();   // the inserts and the accumulators of this chunk are in place before the next one looks them up
        }
    }
    if (threadIdx.x == 0) out_len[q] = base;
    if (dup) *dup_flag = 1;
}

}  // namespace fz

using namespace fz;

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" int fz_lists_max_entries(void) { return LJ_MAX_ENTRIES; }

extern "C" size_t fz_lists_join_workspace_bytes(int S, int Q) { return lj_workspace_bytes(S, Q); }

template <int METHOD, typename ACC>
static int launch_join(const JoinArgs& a, int Q, int64_t* out_ids, void* out_scores, int32_t* out_len, int32_t* flag, size_t lds,
                       hipStream_t st) {
    static unsigned long long done = 0ull;
    const int rc = lj_prepare((const void*)lists_join_kernel<METHOD, ACC>, lds, done, flag, st);
    if (rc != FZ_OK) return rc;
    lists_join_kernel<METHOD, ACC><<<Q, LJ_T, lds, st>>>(a, out_ids, reinterpret_cast<ACC*>(out_scores), out_len, flag);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_lists_join(const int64_t* const* ids_h, const int32_t* const* lens_h, const void* const* values_h,
                             const int32_t* value_is_f64_h, const double* w_h, const int32_t* narrow_h, const int32_t* n_h,
                             const int32_t* ld_h, int S, int Q, int method, int64_t* out_ids, void* out_scores, int32_t* out_len,
                             int ld_out, void* workspace, size_t workspace_bytes, void* stream) {
    // (the method before the plan: an unknown method is FZ_ERR_ARG whatever the lists hold)
    if (method != FZ_LISTS_RRF && method != FZ_LISTS_BCF && method != FZ_LISTS_WSUM_F32 && method != FZ_LISTS_WSUM_F64) return FZ_ERR_ARG;
    const bool wsum = method == FZ_LISTS_WSUM_F32 || method == FZ_LISTS_WSUM_F64;
    LjPlan plan;
    const int rc = lj_plan(n_h, ld_h, S, Q, ld_out, plan);
    if (rc != FZ_OK) return rc;
    if (wsum && !w_h) return FZ_ERR_ARG;
    if (Q == 0 || plan.cap == 0) return FZ_OK;    // nothing to join: empty tensors carry null pointers, out_len keeps the caller's zeros
    if (!ids_h || !lens_h || !out_ids || !out_scores || !out_len || (wsum && !values_h)) return FZ_ERR_ARG;
    if (!workspace || workspace_bytes < fz_lists_join_workspace_bytes(S, Q)) return FZ_ERR_WORKSPACE;
    JoinArgs a{};
    a.S = S; a.ld_out = ld_out; a.cap = plan.cap; a.table_size = plan.table_size;
    for (int s = 0; s < S; ++s) {
        if (!lens_h[s] || (n_h[s] > 0 && (!ids_h[s] || (wsum && !values_h[s])))) return FZ_ERR_ARG;
        a.ids[s] = ids_h[s]; a.lens[s] = lens_h[s];
        a.values[s] = wsum ? values_h[s] : nullptr;
        a.w[s] = wsum ? w_h[s] : 0.0;
        a.n[s] = n_h[s]; a.ld[s] = ld_h[s];
        if (method == FZ_LISTS_WSUM_F64) {
            if (value_is_f64_h && value_is_f64_h[s]) a.f64_mask |= 1u << s;
            if (narrow_h && narrow_h[s]) a.narrow_mask |= 1u << s;
        } else if (wsum && value_is_f64_h && value_is_f64_h[s]) {
            return FZ_ERR_ARG;                    // the float32 accumulation takes float32 planes
        }
    }
    int32_t* flag = reinterpret_cast<int32_t*>(workspace);
    hipStream_t st = as_stream(stream);
    const size_t lds = plan.lds;                  // launch_join raises the kernel's LDS limit where needed and zeroes the flag
    switch (method) {
        case FZ_LISTS_RRF: return launch_join<FZ_LISTS_RRF, double>(a, Q, out_ids, out_scores, out_len, flag, lds, st);
        case FZ_LISTS_BCF: return launch_join<FZ_LISTS_BCF, double>(a, Q, out_ids, out_scores, out_len, flag, lds, st);
        case FZ_LISTS_WSUM_F32: return launch_join<FZ_LISTS_WSUM_F32, float>(a, Q, out_ids, out_scores, out_len, flag, lds, st);
        default: return launch_join<FZ_LISTS_WSUM_F64, double>(a, Q, out_ids, out_scores, out_len, flag, lds, st);
    }
}
