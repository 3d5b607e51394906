// rerank.hip -- K2b: exact ColBERT MaxSim of every query against ITS OWN candidate list over float16 token rows.
//
// The kernel is the slot walk of maxsim_pairs.h (its header says what is computed and why it has this shape); this file states only
// how a row block of float16 rows reaches the A-operand registers: straight from global memory, 64 contiguous bytes of 16 rows per
// global_load_dwordx4 of a wave, 4 row blocks in flight.
#include "maxsim_pairs.h"

namespace fz {

constexpr int MP_RB = 4;   // 16-token row blocks loaded before the MFMAs start

struct PlainRows {
    const _Float16* Dtok;     // [sumL][128]

    __device__ __forceinline__ void prologue(int, int) const {}
    // lane l reads row (l & 15) of a row block, dims 32 ks + 8 (l >> 4) .. + 7
    __device__ __forceinline__ const _Float16* doc(int64_t t0, int, int lane) const { return Dtok + (size_t)t0 * MP_DIM + 8 * (lane >> 4); }
    template <int NB>
    __device__ __forceinline__ void load(const _Float16* doc, int c0, int last, int lane, f16x8 (&af)[NB][4]) const {
#pragma unroll
        for (int rb = 0; rb < NB; ++rb) {
            int row = c0 + 16 * rb + (lane & 15);
            row = row < last ? row : last;   // the last partial row block re-reads the last token: the maximum is unchanged
            const _Float16* p = doc + (size_t)row * MP_DIM;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) af[rb][ks] = *reinterpret_cast<const f16x8*>(p + 32 * ks);
        }
    }
};

struct PairsArgs {
    PairSlots s;
    PlainRows rows;
};

// NCB = Lq / 16 column blocks of 16 query tokens.
template <int NCB>
__global__ __launch_bounds__(MP_WAVES * 64) __attribute__((amdgpu_waves_per_eu(NCB == 2 ? 4 : 2)))
void maxsim_pairs_kernel(PairsArgs a) {
    maxsim_pairs_walk<NCB, MP_RB>(a.s, a.rows);
}

}  // namespace fz

using namespace fz;

extern "C" int fz_maxsim_pairs_f16(const void* Qtok, const void* Dtok, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq,
                                   int N, int dim, const int64_t* cand, int ldc, const int32_t* cand_len, int k, int64_t id_base,
                                   float* scores, int lds, void* stream) {
    PairsArgs a{};
    const int rc = pair_slots_args(a.s, !Dtok && sumL != 0,   // an empty token matrix (every document empty) has no pointer to give
                                   (uintptr_t)Dtok % 16, Qtok, Doff, sumL, max_doc_len, Q, Lq, N, dim, cand, ldc, cand_len, k, id_base, scores, lds);
    if (rc != FZ_OK || Q == 0 || k == 0) return rc;
    a.rows.Dtok = reinterpret_cast<const _Float16*>(Dtok);
    const unsigned nblk = (unsigned)Q * a.s.nslices;
    hipStream_t st = as_stream(stream);
    if (Lq == 32) maxsim_pairs_kernel<2><<<nblk, MP_WAVES * 64, 0, st>>>(a);
    else if (Lq == 64) maxsim_pairs_kernel<4><<<nblk, MP_WAVES * 64, 0, st>>>(a);
    else maxsim_pairs_kernel<8><<<nblk, MP_WAVES * 64, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
