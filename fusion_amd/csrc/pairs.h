// pairs.h -- the slot rule every "query against ITS OWN candidate list" kernel answers by (pairs.hip, forward.hip).
#pragma once
#include "common.h"

namespace fz {

// slot r of query q -> its row in this shard, or -1
__device__ __forceinline__ int pair_position(const int64_t* cand, int ldc, const int32_t* cand_len, int64_t id_base, int N, int W, int q, int r) {
    int klen = W;
    if (cand_len) { klen = cand_len[q]; klen = klen < 0 ? 0 : klen < W ? klen : W; }
    if (r >= klen) return -1;
    const int64_t id = cand[(size_t)q * ldc + r];
    const uint64_t pos = (uint64_t)id - (uint64_t)id_base;
    return (id >= 0 && id >= id_base && pos < (uint64_t)N) ? (int)pos : -1;
}

}  // namespace fz
