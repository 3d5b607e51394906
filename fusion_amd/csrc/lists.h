// lists.h -- what the per-query id joins of lists.hip (lists_join_kernel) and lists_tune.hip (lists_columns_kernel) share: the
// workgroup shape, the capacity, the slot layout of the open-addressing table and its hash.
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

}  // namespace fz
