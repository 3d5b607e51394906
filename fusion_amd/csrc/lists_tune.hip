// lists_tune.hip -- the weight sweep over top-k LISTS: per-query id join to per-system COLUMNS (gfx950).
//
// Aggregator.tune sweeps the weight grid of hybrid.py:404-426 over planes T_s indexed by corpus position (tune.hip: the fused ranks
// of the gold documents are COUNTED for every weight vector, nothing is fused or sorted).  A corpus-scale search returns lists over
// int64 global ids instead, and a query's union of S lists is at most S x k ids out of millions.  This kernel gives those lists the
// shape the counting kernel takes: per query the union's ids become COLUMNS, in the fused dict's first-insertion order (system 0's
// entries in list order, then those of system 1 no earlier system listed, ... -- hybrid.py:293-307), and every system's values
// are scattered to its own plane over those columns.  gold_ranks_kernel / tune_metrics_kernel then run unchanged, on rows of at
// most S x k columns.
//
// The walk is lists_join_kernel's (lists.h: one workgroup per query, steps 1-3, the LDS layout).  Where the join sums contributions
// into one row, this kernel writes, per query (ld_out = one row stride for all planes):
//   out_ids [ld_out] int64   the union's ids in column order, -1 from out_len on      (fz_lists_join's bytes over a -1 fill)
//   T_s     [ld_out] float32 values_s[r] in the column of ids_s[r], r < len_s; +0.0 everywhere else
//   pos     [ld_out] int32   c for c < out_len, -1 beyond (the column IS the first-insertion position: the tie-break)
//   gold_col[G]      int32   the column of gold_ids[g], looked up in the LDS table after the join; -1: negative id (padding), in no list
// EVERY element has exactly one writer, so no output needs a pre-fill and two runs give the same bytes: a lister writes its value
// into its column while the chunk is in registers; the closing pass -- the thread of column c looks uid[c] up and reads the slot's
// system bits -- writes the zeros of the systems that do not list c, and everything from out_len on.
#include "lists.h"

namespace fz {

struct ColumnsArgs {
    const int64_t* ids[FZ_MAX_SYSTEMS];
    const int32_t* lens[FZ_MAX_SYSTEMS];
    const float* values[FZ_MAX_SYSTEMS];   // all null: an ids / pos / gold-only join (no T plane is touched)
    float* T[FZ_MAX_SYSTEMS];              // [Q][ld_out]
    int n[FZ_MAX_SYSTEMS];                 // list width (lens are clamped to it)
    int ld[FZ_MAX_SYSTEMS];                // row stride of ids[s] and values[s], in elements
    const int64_t* gold_ids;               // [Q][G]
    int32_t* gold_col;                     // [Q][G]
    int S, G, ld_out, cap, table_size, has_values;
};

__global__ __launch_bounds__(LJ_T) void lists_columns_kernel(ColumnsArgs a, int64_t* __restrict__ out_ids, int32_t* __restrict__ pos,
                                                             int32_t* __restrict__ out_len, int32_t* __restrict__ dup_flag) {
    const int q = blockIdx.x;
    LjRow j = lj_open(a, q);
    const size_t orow_off = (size_t)q * a.ld_out;
    int64_t* __restrict__ orow = out_ids + orow_off;
    int base = 0;
    bool dup = false;
    for (int s = 0; s < a.S; ++s) {
        const int len = lj_len(a, s, q);
        const int64_t* __restrict__ idrow = a.ids[s] + (size_t)q * a.ld[s];
        for (int r0 = 0; r0 < len; r0 += LJ_T) {
            const int r = r0 + threadIdx.x;
            const bool live = r < len;
            const LjPlaced p = lj_place(j, live, live ? idrow[r] : 0, 1u << (16 + s), orow, base, dup);
            // the lister is the one writer of (system s, column col): entries of one system hit distinct columns
            if (live && a.has_values) a.T[s][orow_off + p.col] = a.values[s][(size_t)q * a.ld[s] + r];
            __syncthreads();   // the inserts of this chunk are in place before the next one (and the closing pass) looks them up
        }
    }

    // closing pass, one thread per column of the row: the zeros no lister wrote, the positions, the tail from out_len on
    for (int c = threadIdx.x; c < a.ld_out; c += LJ_T) {
        uint32_t listed = 0u;                           // bit s: system s wrote T_s[c]
        if (c < base) {                                 // the id is in the table (under its own or, for a duplicate, its twin's column)
            uint32_t slot;
            const uint32_t v = lj_find(j, j.uid[c], slot);
            if (v != LJ_EMPTY && (int)(v & LJ_COL) == c) listed = (v >> 16) & 0xffu;
        } else {
            orow[c] = -1;
        }
        pos[orow_off + c] = c < base ? c : -1;
        if (a.has_values)
            for (int s = 0; s < a.S; ++s)
                if (!((listed >> s) & 1u)) a.T[s][orow_off + c] = 0.0f;
    }
    // the gold ids' columns: a read-only look-up in the finished table
    for (int g = threadIdx.x; g < a.G; g += LJ_T) {
        const int64_t id = a.gold_ids[(size_t)q * a.G + g];
        int col = -1;
        if (id >= 0 && j.total > 0) {
            uint32_t slot;
            const uint32_t v = lj_find(j, id, slot);
            if (v != LJ_EMPTY) col = (int)(v & LJ_COL);
        }
        a.gold_col[(size_t)q * a.G + g] = col;
    }
    if (threadIdx.x == 0) out_len[q] = base;
    if (dup) *dup_flag = 1;
}

}  // namespace fz

using namespace fz;

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" size_t fz_lists_columns_workspace_bytes(int S, int Q) { return lj_workspace_bytes(S, Q); }

extern "C" int fz_lists_columns(const int64_t* const* ids_h, const int32_t* const* lens_h, const float* const* values_h,
                                const int32_t* n_h, const int32_t* ld_h, int S, int Q, const int64_t* gold_ids, int G,
                                int64_t* out_ids, float* const* T_h, int32_t* pos, int32_t* out_len, int32_t* gold_col, int ld_out,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (G < 0) return FZ_ERR_ARG;
    LjPlan plan;
    int rc = lj_plan(n_h, ld_h, S, Q, ld_out, plan);
    if (rc != FZ_OK) return rc;
    if (Q == 0 || plan.cap == 0) return FZ_OK;    // nothing to join: empty tensors carry null pointers, the outputs keep the caller's fill
    if (!ids_h || !lens_h || !out_ids || !pos || !out_len || (values_h && !T_h) || (G > 0 && (!gold_ids || !gold_col))) return FZ_ERR_ARG;
    if (!workspace || workspace_bytes < fz_lists_columns_workspace_bytes(S, Q)) return FZ_ERR_WORKSPACE;
    ColumnsArgs a{};
    a.S = S; a.G = G; a.ld_out = ld_out; a.has_values = values_h ? 1 : 0;
    a.cap = plan.cap; a.table_size = plan.table_size;
    a.gold_ids = gold_ids; a.gold_col = gold_col;
    for (int s = 0; s < S; ++s) {
        if (!lens_h[s] || (n_h[s] > 0 && (!ids_h[s] || (values_h && !values_h[s]))) || (values_h && !T_h[s])) return FZ_ERR_ARG;
        a.ids[s] = ids_h[s]; a.lens[s] = lens_h[s];
        a.values[s] = values_h ? values_h[s] : nullptr;
        a.T[s] = values_h ? T_h[s] : nullptr;
        a.n[s] = n_h[s]; a.ld[s] = ld_h[s];
    }
    static unsigned long long done = 0ull;
    int32_t* flag = reinterpret_cast<int32_t*>(workspace);
    hipStream_t st = as_stream(stream);
    rc = lj_prepare((const void*)lists_columns_kernel, plan.lds, done, flag, st);
    if (rc != FZ_OK) return rc;
    lists_columns_kernel<<<Q, LJ_T, plan.lds, st>>>(a, out_ids, pos, out_len, flag);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
