// rerank8.hip -- K2d: exact ColBERT MaxSim of every query against ITS OWN candidate list over OCP e4m3 token rows (128 B per token).
//
//     scores[q][r] = 2^-descale_exp * sum_i max_{t < min(len_d, max_doc_len)} <Q8[q, i], D8[t]>,   d = cand[q][r] - id_base,
// bit for bit what fz_maxsim_e4m3 (maxsim8.hip) gives that pair: the same ONE v_mfma_scale_f32_16x16x128_f8f6f4 per 16 x 16 block of
// dot products (both hardware scales E8M0 127, C = 0), the same fmaxf maximum from -inf, the same sum (maxsim_tiles.h's: row16_sum per column block,
// then the pair tree) and the same single multiply by the power of two on the finished sum.
//
// The kernel is the slot walk of maxsim_pairs.h -- read its header first: one workgroup = 4 waves = one (query, 128 slots), lane i
// resolves slot i once per wave (pair_slot_resolve), v_readlane brings it back into SGPRs, the query's B fragments stay resident, rows
// go straight from global memory into the A operand, rows past the document's end are clamped to its last token, no LDS, no barrier.
// Shared with the float16 and the residual kernels, as code: the slot resolution (pair_slot_resolve), the transpose-and-sum epilogue
// (pair_token_sum) and, on the host, pair_slots_args; extracting them left every resource line of rerank.res and rerank_residual.res as
// it was.  The loop over the row blocks is stated here and not as a third `Rows` policy of maxsim_pairs_walk: the fragment is another
// type (32 bytes of one row, not 4 x 8 halves), the MFMA step has no k-chain, and 8 row blocks are in flight where that walk's dispatch is
// written for 4 or 2.  What differs from the float16 walk:
//   * Operand lane map: maxsim8.hip's, on both sides.  Lane l takes row (l & 15) and the two 16-byte chunks g and g + 4 (g = l >> 4) of
//     that row's 128 bytes -- two global_load_dwordx4 per row block and lane; a load of a wave covers 64 contiguous bytes of 16 rows, as
//     in the float16 kernel.  Whatever order the instruction gives the 128 k inside its lane groups, both operands see the same one.
//   * One MFMA per (row block, column block): 4 x fewer than the float16 walk, and 8 VGPRs of B per column block instead of 16.
//   * RB = FZ_MP8_RB row blocks in flight: 8 = the float16 kernel's 16 KiB per wave (64 A VGPRs, 16 loads per lane).  RB = 4 is the
//     variant tools/ablate/maxsim_pairs8_variants.py builds; tools/bench_maxsim_pairs_fp8.py times one against the other, call by call.
// Where it stands: DESIGN.md section 'Candidate-list MaxSim over e4m3 rows' and profiles/r25_maxsim_pairs_fp8.json.
#include "maxsim_pairs.h"

#ifndef FZ_MP8_RB
#define FZ_MP8_RB 8
#endif

namespace fz {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int MP8_RB = FZ_MP8_RB;   // 16-token row blocks loaded before the MFMAs start
static_assert(MP8_RB == 8 || MP8_RB == 4, "the NB dispatch below is written for 8 or 4 row blocks in flight");

struct Pairs8Args {
    PairSlots s;                 // s.Qtok: the e4m3 query bytes [Q][Lq][128]
    const unsigned char* Dtok;   // [sumL][128] e4m3
    float descale;               // 2^-descale_exp
};

// the 32 bytes of one row a lane feeds the instruction with: chunks g and g + 4; p points at chunk g
__device__ __forceinline__ i32x8 row_fragment8(const unsigned char* p) {
    const i32x4 lo = *reinterpret_cast<const i32x4*>(p), hi = *reinterpret_cast<const i32x4*>(p + 64);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// amdgpu_waves_per_eu per Lq, from the resource report (rerank8.res): the most waves per SIMD at which nothing spills.
//   RB = 8:  Lq = 32: 106 VGPRs, 4 waves (5: 2 spilled) | Lq = 64: 168, 3 (4: 57 spilled) | Lq = 128: 246, 2 (3: 53 spilled)
//   RB = 4:  Lq = 32:  68 VGPRs, 7 waves (reached from 4; 8: 17 spilled) | Lq = 64: 116, 4 (5: 14 spilled) | Lq = 128: 156, 3 (4: 26 spilled)
template <int NCB>
constexpr int mp8_waves() { return MP8_RB == 8 ? (NCB == 2 ? 4 : NCB == 4 ? 3 : 2) : (NCB == 8 ? 3 : 4); }

// NCB = Lq / 16 column blocks of 16 query tokens.
template <int NCB>
__global__ __launch_bounds__(MP_WAVES * 64) __attribute__((amdgpu_waves_per_eu(mp8_waves<NCB>())))
void maxsim_pairs8_kernel(Pairs8Args k) {
    const PairSlots& a = k.s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = blockIdx.x / a.nslices;
    const int r_first = (blockIdx.x % a.nslices) * MP_SLICE + w;   // this wave's slots: r_first + MP_WAVES * i
    if (r_first >= a.k) return;                                    // a wave with no candidate in this slice
    const int left = (a.k - r_first + MP_WAVES - 1) / MP_WAVES;
    const int nmine = left < MP_CPW ? left : MP_CPW;

    int64_t my_t0;
    int my_len;
    pair_slot_resolve(a, q, r_first, nmine, lane, my_t0, my_len);

    // ---- B fragments of the query, resident for the whole wave: the chunks g and g + 4 of query token 16 b + (l & 15) ----
    const int chunk = 16 * (lane >> 4);
    i32x8 bq[NCB];
    {
        const unsigned char* src = reinterpret_cast<const unsigned char*>(a.Qtok) + ((size_t)q * NCB * 16 + (lane & 15)) * MP_DIM + chunk;
#pragma unroll
        for (int b = 0; b < NCB; ++b) bq[b] = row_fragment8(src + (size_t)b * 16 * MP_DIM);
    }

    float* const out = a.scores + (size_t)q * a.lds + r_first;
    for (int i = 0; i < nmine; ++i) {
        const int len = __builtin_amdgcn_readlane(my_len, i);
        float* const dst = out + MP_WAVES * i;
        if (len <= 0) {   // absent slot / empty document (sum of an empty max := 0, as in maxsim_tiles.h)
            if (lane == 0) *dst = len < 0 ? -INFINITY : 0.f;
            continue;
        }
        const unsigned char* const doc = k.Dtok + (size_t)readlane64(my_t0, i) * MP_DIM + chunk;
        const int last = len - 1;

        float run[NCB];
#pragma unroll
        for (int b = 0; b < NCB; ++b) run[b] = -INFINITY;

        for (int c0 = 0; c0 < len; c0 += 16 * MP8_RB) {
            const int nb = (len - c0 + 15) >> 4;   // row blocks left (wave-uniform); >= 1
            // NB row blocks: every load is issued before the first MFMA; then NCB x NB independent MFMAs, each column block's folded
            // under the next one's.  The loads stay inside the per-NB branch, as in maxsim_pairs_walk.
            auto body = [&](auto NBc) __attribute__((always_inline)) {
                constexpr int NB = decltype(NBc)::value;
                i32x8 af[NB];
#pragma unroll
                for (int rb = 0; rb < NB; ++rb) {
                    int row = c0 + 16 * rb + (lane & 15);
                    row = row < last ? row : last;   // the last partial row block re-reads the last token: the maximum is unchanged
                    af[rb] = row_fragment8(doc + (size_t)row * MP_DIM);
                }
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    f32x4 acc[NB];
#pragma unroll
                    for (int rb = 0; rb < NB; ++rb)
                        acc[rb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[rb], bq[cb], (f32x4)0.f, 0, 0, 0, 127, 0, 127);
                    float m = run[cb];
#pragma unroll
                    for (int rb = 0; rb < NB; ++rb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) m = fmaxf(m, acc[rb][r]);
                    run[cb] = m;
                }
            };
            if constexpr (MP8_RB == 8) {
                if (nb >= 8) body(std::integral_constant<int, 8>{});
                else if (nb == 7) body(std::integral_constant<int, 7>{});
                else if (nb == 6) body(std::integral_constant<int, 6>{});
                else if (nb == 5) body(std::integral_constant<int, 5>{});
                else if (nb == 4) body(std::integral_constant<int, 4>{});
                else if (nb == 3) body(std::integral_constant<int, 3>{});
                else if (nb == 2) body(std::integral_constant<int, 2>{});
                else body(std::integral_constant<int, 1>{});
            } else {
                if (nb >= 4) body(std::integral_constant<int, 4>{});
                else if (nb == 3) body(std::integral_constant<int, 3>{});
                else if (nb == 2) body(std::integral_constant<int, 2>{});
                else body(std::integral_constant<int, 1>{});
            }
        }

        const float s = pair_token_sum<NCB>(run);
        if (lane == 0) *dst = s * k.descale;   // a power of two on the finished sum: exact
    }
}

}  // namespace fz

using namespace fz;

extern "C" int fz_maxsim_pairs_e4m3(const void* Qtok8, const void* Dtok8, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq,
                                    int N, int dim, int descale_exp, const int64_t* cand, int ldc, const int32_t* cand_len, int k,
                                    int64_t id_base, float* scores, int lds, void* stream) {
    Pairs8Args a{};
    // descale_exp out of range and a missing token matrix are argument errors of this storage: reported in that class's turn
    const int rc = pair_slots_args(a.s, (!Dtok8 && sumL != 0) || descale_exp < -32 || descale_exp > 32, (uintptr_t)Dtok8 % 16, Qtok8, Doff, sumL,
                                   max_doc_len, Q, Lq, N, dim, cand, ldc, cand_len, k, id_base, scores, lds);
    if (rc != FZ_OK || Q == 0 || k == 0) return rc;
    a.Dtok = reinterpret_cast<const unsigned char*>(Dtok8);
    a.descale = ldexpf(1.0f, -descale_exp);
    const unsigned nblk = (unsigned)Q * a.s.nslices;
    hipStream_t st = as_stream(stream);
    if (Lq == 32) maxsim_pairs8_kernel<2><<<nblk, MP_WAVES * 64, 0, st>>>(a);
    else if (Lq == 64) maxsim_pairs8_kernel<4><<<nblk, MP_WAVES * 64, 0, st>>>(a);
    else maxsim_pairs8_kernel<8><<<nblk, MP_WAVES * 64, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
