// sort.h -- what another translation unit needs from the row sort (sort.hip): the argument block of sort_rows_kernel, its launcher, the
// row capacities, and the argument blocks that several entry points would otherwise spell out field by field (sort.hip, topk.hip).
#pragma once
#include "common.h"

namespace fz {

struct SortArgs {
    const void* keys;            // fp32 or fp64
    const int32_t* init_order;   // nullable [rows][key_row_stride]: column at sequence position r (gather)
    const int32_t* init_rank;    // nullable [rows][key_row_stride]: sequence position of column j, -1 = not in the sequence
                                 //   (same information as init_order, but loaded coalesced and placed through LDS)
    const int32_t* row_len;      // nullable [rows]
    int n_total;                 // elements per row (before chunking)
    long key_row_stride;         // elements between consecutive rows
    int seg_len;                 // element e lives at (e / seg_len) * seg_stride + row*key_row_stride + e % seg_len
    long seg_stride;             //   (seg_len >= n_total -> plain rows)
    int chunks;                  // pseudo-rows per row
    int chunk_len;               // chunk c covers [c*chunk_len, min(n_total,(c+1)*chunk_len))
    int32_t* order;              // nullable
    void* sorted_keys;           // nullable, same type as keys
    int32_t* rank;               // nullable (only chunks == 1)
    long out_row_stride;         // elements between rows of order / sorted_keys
    int out_chunk_stride;        // elements between chunks inside a row
    int out_limit;               // only the first out_limit entries of each pseudo-row are written
    const int32_t* colmap;       // nullable: order value = colmap[row*colmap_row_stride + col]
    long colmap_row_stride;
    const int64_t* idmap;        // nullable: out_ids = idmap[addr(col)] (same segment addressing as keys)
    int64_t id_base;             // else out_ids = id_base + col
    int64_t* out_ids;            // nullable, [rows][out_row_stride] like order
    int32_t* row_flags;          // fp64 keys: [rows*chunks] 1 = the fast form left the row to the generic one
    float* row_stats;            // nullable [4][stats_rows]: mean | unbiased std | min | max of the list's float32 values (the statistics of
    int stats_rows;              //   hybrid.py:254-262), a by-product of having the row in registers; chunks == 1 only
    const int32_t* stats_len;    // nullable [rows]: the statistics cover the first stats_len[row] entries of the SORTED list (a ranking
                                 //   truncated to its top-k: PLAID-style short lists, return_topk); fp32 keys only
    int bucket_rank;             // 1 = rows of a 1024-thread workgroup are ordered by the bucket ranking where it applies (set by the launcher)
    int zero_compact;            // 1 = float64 rows that are mostly exact zeros leave their zeros out of the ordering phases (ZC; set by the launcher)
    int expect_zeros;            // the caller expects such rows (fz_sort_rows_desc_lexical): the launcher picks the SORT_ROWS_ZC instantiation
    // FUSE (fz_sort_rank_fused_desc): there is no key plane -- the float64 key of column j is the rank fusion of hybrid.py:248-252,301-304,
    // formed on load from the S rank planes exactly as fuse_rank_kernel (fuse.hip) forms it: 0.0 + sum over the systems, in system order, of
    // 1/(60 + r + 1) (rrf) or (n - r + 1)/n (bcf) over the systems that list the document (r >= 0); -inf when none does
    const int32_t* fuse_ranks[FZ_MAX_SYSTEMS];   // [rows][key_row_stride] each
    const int32_t* fuse_lens;    // [S][fuse_rows] list lengths (bcf's n)
    int fuse_S, fuse_method, fuse_rows;
    double* fuse_gen_plane;      // [rows][key_row_stride]: where the fused scores of a row the fast form FLAGS are written out for the generic launch
    int fuse_first_is_pos;       // placed form with init_rank == fuse_ranks[0] (every list full: first-insertion order = system 0's ranking):
                                 //   the position just loaded IS system 0's rank, its plane is not read a second time
};

// The longest row one workgroup holds in its registers: T * E of the largest configuration launch_sort has for the key width (float32:
// 1024 x 35, float64: 1024 x 28).  Longer rows: chunk-sort + merge (sort_long_rows), chunk-sort-truncate levels (fz_topk_rows_f32).
constexpr int SORT_ROW_F32 = 35840, SORT_ROW_F64 = 28672;
constexpr int sort_row_max(int key_bits) { return key_bits == 32 ? SORT_ROW_F32 : SORT_ROW_F64; }

// prows workgroups, one per pseudo-row of at most n_chunk keys; kw = key words (1: float32, 2: float64).  Defined in sort.hip.
int launch_sort(const SortArgs& a, int kw, int prows, int n_chunk, hipStream_t st);

// Whole rows of one plane, one workgroup per row: [rows][ld] in, order / sorted_keys / rank (each nullable) [rows][ld] out.
inline SortArgs whole_rows(const void* keys, int n, int ld, int32_t* order, void* sorted_keys, int32_t* rank) {
    SortArgs a{};
    a.keys = keys;
    a.n_total = n; a.key_row_stride = ld; a.seg_len = n; a.seg_stride = 0;
    a.chunks = 1; a.chunk_len = n;
    a.order = order; a.sorted_keys = sorted_keys; a.rank = rank;
    a.out_row_stride = ld; a.out_chunk_stride = 0; a.out_limit = n;
    return a;
}

// One sort row of `len` float32 scores with their ids beside them ([rows][len] each): the first `lim` (score, id) pairs out, [rows][lim].
inline SortArgs id_rows(const float* scores, const int64_t* ids, int len, float* out_scores, int64_t* out_ids, int lim) {
    SortArgs a{};
    a.keys = scores; a.idmap = ids;
    a.n_total = len; a.key_row_stride = len; a.seg_len = len;
    a.chunks = 1; a.chunk_len = len;
    a.sorted_keys = out_scores; a.out_ids = out_ids; a.out_row_stride = lim; a.out_limit = lim;
    return a;
}

// float64 keys: the one flag per row that the fast form leaves for the generic one, in the caller's workspace
inline int take_row_flags(SortArgs& a, int rows, int n, void* workspace, size_t workspace_bytes) {
    if (!workspace || workspace_bytes < fz_sort_workspace_bytes(64, rows, n)) return FZ_ERR_WORKSPACE;
    a.row_flags = (int32_t*)workspace;
    return FZ_OK;
}

// slots that nothing may claim: (-inf, -1), which cannot win.  (static: each file its own copy, as in slices.h)
template <typename K>
static __global__ void fill_absent_kernel(K* keys, int32_t* cols, size_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        keys[i] = (K)(-INFINITY);
        cols[i] = -1;
    }
}

}  // namespace fz
