// lists.h -- the per-query id join of top-k lists, stated once for lists.hip (lists_join_kernel: one fused row) and lists_tune.hip
// (lists_columns_kernel: per-system columns): the workgroup shape, the capacity, the open-addressing table and its hash, the walk
// that turns a query's lists into columns, and the host-side plan of a call.
//
// ONE 1,024-THREAD WORKGROUP PER QUERY.  Per system, per chunk of T = 1024 entries (one entry per thread, kept in registers):
//   1. look the id up (read only, but for one atomic OR on a hit: bit 16 + s of the slot = "system s listed this column";
//      finding the own system's bit already set is a duplicate id inside the list)
//   2. ballot + block scan of the "new" flags -> column = base + exclusive prefix; the id goes to LDS and to out_ids
//   3. the new ids are inserted: compare-and-swap on the slot (EMPTY -> column | own system bit), linear probing; a failed
//      swap onto a slot that holds the same id is a duplicate as well
//   4. the kernel's own use of (entry, column) -- accumulate or scatter -- and the barrier that closes the chunk: the inserts are
//      in place before the next chunk looks them up
// lj_place is steps 1-3.  Columns never depend on the arrival order of the atomics: two runs give the same bytes.
//
// LDS: ids [cap] int64 + table [2 * cap rounded up to a power of two] uint32 + 16 wave totals, cap = min(sum of the list widths,
// 8,192) of the CALL: 128 KB + 64 B at the capacity (one workgroup per CU), 56 KB for three lists of 1,000 (two per CU).
#pragma once
#include "common.h"

namespace fz {

constexpr int LJ_T = 1024;                 // threads per workgroup = entries per chunk
constexpr int LJ_MAX_ENTRIES = 8192;       // fz_lists_max_entries(): FZ_MAX_SYSTEMS x 1,024
constexpr uint32_t LJ_EMPTY = 0xffffffffu;
constexpr uint32_t LJ_COL = 0xffffu;       // low half of a slot: the column; bits 16..23: the systems that list it

__device__ __forceinline__ uint32_t lj_hash(int64_t id, uint32_t mask) {
    // multiplicative (Fibonacci) hashing on the full 64 bits, high half folded in: ids that differ only above bit 32, or by
    // multiples of the table size, spread like any others
    const uint64_t h = (uint64_t)id * 0x9E3779B97F4A7C15ull;
    return (uint32_t)(h >> 40) & mask;
}

struct LjRow {                             // one query's join state
    int64_t* uid;                          // LDS [cap]: the union's ids in column order
    uint32_t* table;                       // LDS [table_size]: the row uses the first mask + 1 slots
    uint32_t* wtot;                        // LDS [LJ_T / 64]: the wave totals of step 2
    uint32_t mask;
    int total;                             // the row's entries: the sum of its clamped lengths
};

template <typename Args>
__device__ __forceinline__ int lj_len(const Args& a, int s, int q) { return min(max(a.lens[s][q], 0), a.n[s]); }

// Carves up the dynamic LDS and clears the row's table.  The table only needs twice the ROW's entries: short rows clear (and probe)
// a short table; an empty row (block-uniform) touches no LDS at all.
template <typename Args>
__device__ __forceinline__ LjRow lj_open(const Args& a, int q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lj_smem[];
    LjRow j;
    j.uid = reinterpret_cast<int64_t*>(lj_smem);
    j.table = reinterpret_cast<uint32_t*>(j.uid + a.cap);
    j.wtot = j.table + a.table_size;
    j.total = 0;
    for (int s = 0; s < a.S; ++s) j.total += lj_len(a, s, q);
    uint32_t tsize = 64;
    while (tsize < 2u * (uint32_t)j.total) tsize <<= 1;   // <= table_size: total <= cap
    j.mask = tsize - 1;
    if (j.total > 0) {
        for (uint32_t i = threadIdx.x; i < tsize; i += LJ_T) j.table[i] = LJ_EMPTY;
        __syncthreads();
    }
    return j;
}

// Probes from the id's home slot: returns the slot word that holds the id, or LJ_EMPTY with `slot` at the empty slot the probe
// ended on.  The table is at most half full: an empty slot is always reached.
__device__ __forceinline__ uint32_t lj_find(const LjRow& j, int64_t id, uint32_t& slot) {
    for (slot = lj_hash(id, j.mask);; slot = (slot + 1) & j.mask) {
        const uint32_t v = j.table[slot];
        if (v == LJ_EMPTY || j.uid[v & LJ_COL] == id) return v;
    }
}

struct LjPlaced {
    int col;                               // the entry's column (-1: not live)
    bool isnew;                            // this entry opened the column
    uint32_t before;                       // the systems that listed the column ahead of this one (bit s)
};

// Steps 1-3 for one chunk entry per thread (live: this thread holds one; sbit = 1 << (16 + s)).  Holds two __syncthreads():
// call it BLOCK-UNIFORMLY -- the chunk loops run on a per-(system, query) length.  base is the row's column count so far.
__device__ __forceinline__ LjPlaced lj_place(const LjRow& j, bool live, int64_t id, uint32_t sbit, int64_t* __restrict__ orow,
                                             int& base, bool& dup) {
    constexpr int NW = LJ_T / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    LjPlaced p{-1, false, 0u};
    uint32_t slot = 0;
    if (live) {
        const uint32_t v = lj_find(j, id, slot);
        if (v != LJ_EMPTY) {
            p.col = (int)(v & LJ_COL);
            const uint32_t old = atomicOr(&j.table[slot], sbit);
            if (old & sbit) dup = true;
            p.before = (old >> 16) & 0xffu;
        }
    }
    p.isnew = live && p.col < 0;
    const unsigned long long bal = __ballot(p.isnew);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) j.wtot[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { const int c = (int)j.wtot[i]; if (i < wv) woff += c; tot += c; }
    if (p.isnew) {
        p.col = base + woff + below;       // < total <= cap <= ld_out: every live entry is counted in total
        j.uid[p.col] = id;
        orow[p.col] = id;
    }
    base += tot;
    __syncthreads();
    if (p.isnew) {
        const uint32_t mine = (uint32_t)p.col | sbit;
        for (;;) {
            const uint32_t old = atomicCAS(&j.table[slot], LJ_EMPTY, mine);
            if (old == LJ_EMPTY) break;
            if (j.uid[old & LJ_COL] == id) { dup = true; break; }   // the same id twice in this chunk: it keeps its own column, unlisted
            slot = (slot + 1) & j.mask;
        }
    }
    return p;
}

// ---- host side: what fz_lists_join and fz_lists_columns plan alike ----------------------------------------------------------
struct LjPlan {
    int cap, table_size;                   // sum of the list widths; 2 * cap rounded up to a power of two (>= 64)
    size_t lds;
};

// The checks both entry points make on the list geometry, in their order (it decides the code an input gets), and the LDS plan.
inline int lj_plan(const int32_t* n_h, const int32_t* ld_h, int S, int Q, int ld_out, LjPlan& p) {
    if (S <= 0 || S > FZ_MAX_SYSTEMS || Q < 0 || !n_h || !ld_h) return FZ_ERR_ARG;
    long long total = 0;
    for (int s = 0; s < S; ++s) {
        if (n_h[s] < 0 || ld_h[s] < n_h[s]) return FZ_ERR_ARG;
        total += n_h[s];
    }
    if (total > LJ_MAX_ENTRIES) return FZ_ERR_UNSUPPORTED;
    if (ld_out < total) return FZ_ERR_ARG;
    p.cap = (int)total;
    p.table_size = 64;
    while (p.table_size < 2 * p.cap) p.table_size <<= 1;
    p.lds = (size_t)p.cap * 8 + (size_t)p.table_size * 4 + (LJ_T / 64) * 4;
    return FZ_OK;
}

inline size_t lj_workspace_bytes(int S, int Q) {
    if (S <= 0 || S > FZ_MAX_SYSTEMS || Q < 0) return 0;
    return 16;   // the duplicate flag (int32 at offset 0)
}

// Before the launch: the kernel may take more than 48 KiB of dynamic LDS (done: the call site's per-device mask), the flag is zero.
inline int lj_prepare(const void* kernel, size_t lds, unsigned long long& done, int32_t* flag, hipStream_t st) {
    if (lds > 48 * 1024) {
        const int rc = raise_lds_limit(kernel, 160 * 1024, done);
        if (rc != FZ_OK) return rc;
    }
    FZ_HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    return FZ_OK;
}

}  // namespace fz
