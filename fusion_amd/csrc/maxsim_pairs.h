// maxsim_pairs.h -- exact ColBERT MaxSim of every query against ITS OWN candidate list (the corpus-scale rerank stage): the slot walk
// of rerank.hip (float16 token rows) and rerank_residual.hip (the 2-/4-bit residual-compressed index), stated once.
//
// scores[q][r] = s(q, cand[q][r] - id_base) with s as in maxsim.hip (the walk of maxsim_tiles.h), bit for bit: the same v_mfma_f32_16x16x32_f16 mapping (A = 16
// document tokens x 32 dims, B = 32 dims x 16 query tokens, k-steps 0..3 from a zero accumulator), the same fmaxf maximum from -inf
// and the same sum (row16_sum per 16-token column block, then the pair tree (b0+b1)+(b2+b3) ...), so a system's all-pairs plane and
// its candidate lists are interchangeable -- and so are the two storages, which differ in nothing but how a row block's A fragments
// reach the registers.
//
// The workload is a gather: every (query, candidate) pair reads its own document, one contiguous run of len x 256 B found through
// Doff, and nothing is shared between pairs but the query (about 18 GB of token rows against 1.2 TFLOP at Q = 1024, k = 1000).
// So the design keeps loads in flight and hangs the MFMAs off them:
//   * a workgroup = 4 waves = one (query, slice of 128 candidate slots); workgroups are query-major, so a query's slices are
//     dispatched next to each other;
//   * every wave keeps the query's B fragments in registers (16 VGPRs per 16-token column block: 32 / 64 / 128 at Lq = 32 / 64 / 128)
//     and walks its own candidates: slots slice + 4 i + w, i < 32.  Lane i resolves candidate i ONCE at the start of the wave
//     (id -> position -> Doff pair -> clamped length: three dependent reads, paid once per wave, not once per candidate); the
//     loop takes them back with v_readlane, so everything that steers it is in SGPRs;
//   * document rows go straight from global memory into the A-operand registers, up to RB row blocks (RB = 4: 64 tokens, 16 KiB, 16
//     global_load_dwordx4 per lane) issued back to back before the first MFMA; other waves of the SIMD cover the latency (no LDS, no
//     barrier: waves of a workgroup never wait for each other);
//   * a row index past the document's last token is CLAMPED to that token: the row block re-reads a real row, the maximum is
//     unchanged and nothing needs a mask; nothing past Doff[pos + 1], past max_doc_len or past row sumL - 1 is ever read.  Row
//     blocks wholly past the end are skipped (wave-uniform).
// Slots: r >= cand_len[q], id < 0 or position outside [0, N) -> -inf (a shard scores what it owns); an empty document -> 0.
//
// The storage is a policy `Rows` with three members, inlined where today's statements stood:
//     void prologue(int w, int lane) const            once per wave, after the early return and before slot resolution
//     Doc  doc(int64_t t0, int w, int lane) const     the handle of the document whose first token row is t0
//     void load<NB>(doc, c0, last, lane, af) const    af[rb][ks] = this lane's A fragments of rows c0 + 16 rb + (lane & 15), clamped to last
//
// rerank8.hip (e4m3 token rows, one block-scaled MFMA per 16 x 16 block) walks the same slots with a loop of its own over another fragment
// type; what it shares is stated once below: pair_slot_resolve, readlane64, pair_token_sum and, on the host, pair_slots_args.
//
// Where it stands: DESIGN.md section 'Candidate-list MaxSim' and profiles/r10_maxsim_pairs.json.
#pragma once
#include <hip/hip_fp16.h>

#include <type_traits>

#include "common.h"

namespace fz {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MP_DIM = 128;
constexpr int MP_WAVES = 4;                  // waves per workgroup
constexpr int MP_CPW = 32;                   // candidate slots per wave (<= 64: one lane resolves one slot)
constexpr int MP_SLICE = MP_WAVES * MP_CPW;  // candidate slots per workgroup
constexpr int MP_MAX_DOC_LEN = 16384;        // as fz_maxsim_f16

// what the walk needs whatever the rows are stored as: the first member of either kernel's argument block
struct PairSlots {
    const _Float16* Qtok;     // [Q][Lq][128]
    const int64_t* Doff;      // [N+1]
    const int64_t* cand;      // [Q][ldc]
    const int32_t* cand_len;  // [Q] or null
    float* scores;            // [Q][lds]
    int64_t sumL, id_base;
    int ldc, lds, Q, N, k, max_doc_len;
    int nslices;              // ceil(k / MP_SLICE)
};

// Lane `lane` of a wave resolves slot r_first + MP_WAVES * lane of query q: first token row and length (-1: absent, 0: empty document).
// The three dependent reads (id -> position -> Doff pair) are paid once per wave; the walk takes the result back with v_readlane.
__device__ __forceinline__ void pair_slot_resolve(const PairSlots& a, int q, int r_first, int nmine, int lane, int64_t& my_t0, int& my_len) {
    my_t0 = 0;
    my_len = -1;
    int klen = a.k;
    if (a.cand_len) { klen = a.cand_len[q]; klen = klen < 0 ? 0 : klen < a.k ? klen : a.k; }
    const int r = r_first + MP_WAVES * lane;
    if (lane < nmine && r < klen) {
        const int64_t id = a.cand[(size_t)q * a.ldc + r];
        const uint64_t pos = (uint64_t)id - (uint64_t)a.id_base;
        if (id >= 0 && id >= a.id_base && pos < (uint64_t)a.N) {
            const int64_t t0 = a.Doff[pos];
            int64_t len = a.Doff[pos + 1] - t0;
            if (len > a.max_doc_len) len = a.max_doc_len;
            if (len > a.sumL - t0) len = a.sumL - t0;   // offsets that disagree with sumL: never read past the last row
            if (t0 < 0 || len < 0) len = 0;
            my_t0 = t0;
            my_len = (int)len;
        }
    }
}

// lane i's 64-bit value, wave-uniform (two v_readlane)
__device__ __forceinline__ int64_t readlane64(int64_t v, int i) {
    return ((int64_t)__builtin_amdgcn_readlane((int)(v >> 32), i) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, i);
}

// End of a document.  run[b]: this lane's partial maximum of column block b (its query token: lane & 15; its rows: 4 (lane >> 4) ..).
// The maximum over the four 16-lane rows, then the sum over the query tokens, in maxsim_tiles.h's order: P / S transpose the column blocks'
// partial maxima onto the rows, row16_sum adds 16 tokens, two swap steps add the blocks in pairs.  Lane 0 holds the score.
template <int NCB>
__device__ __forceinline__ float pair_token_sum(const float (&run)[NCB]) {
    auto P = [&](float A, float B) __attribute__((always_inline)) -> float { swap32(A, B); return fmaxf(A, B); };
    auto S = [&](float X, float Y) __attribute__((always_inline)) -> float { swap16(X, Y); return fmaxf(X, Y); };
    auto blk = [&](int b) __attribute__((always_inline)) -> float { return b < NCB ? run[b < NCB ? b : 0] : -INFINITY; };
    float s0 = row16_sum(S(P(blk(0), blk(2)), P(blk(1), blk(3))));   // rows: column blocks 0, 1, 2, 3
    float o0 = s0;
    swap16(s0, o0);
    s0 += o0;                                                        // rows (0, 1): b0 + b1 | rows (2, 3): b2 + b3
    if constexpr (NCB >= 4) {
        o0 = s0;
        swap32(s0, o0);
        s0 += o0;                                                    // (b0 + b1) + (b2 + b3)
    }
    if constexpr (NCB == 8) {
        float s1 = row16_sum(S(P(blk(4), blk(6)), P(blk(5), blk(7))));
        float o1 = s1;
        swap16(s1, o1);
        s1 += o1;
        o1 = s1;
        swap32(s1, o1);
        s1 += o1;
        s0 += s1;                                                    // ((b0 + b1) + (b2 + b3)) + ((b4 + b5) + (b6 + b7))
    }
    return s0;
}

// NCB = Lq / 16 column blocks of 16 query tokens; RB (4 or 2) 16-token row blocks loaded before the MFMAs start.
template <int NCB, int RB, class Rows>
__device__ __forceinline__ void maxsim_pairs_walk(const PairSlots& a, const Rows& rows) {
    static_assert(RB == 4 || RB == 2, "the NB dispatch below is written for 4 or 2 row blocks in flight");
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = blockIdx.x / a.nslices;
    const int r_first = (blockIdx.x % a.nslices) * MP_SLICE + w;   // this wave's slots: r_first + MP_WAVES * i
    if (r_first >= a.k) return;                                    // a wave with no candidate in this slice
    const int left = (a.k - r_first + MP_WAVES - 1) / MP_WAVES;
    const int nmine = left < MP_CPW ? left : MP_CPW;

    rows.prologue(w, lane);

    int64_t my_t0;
    int my_len;
    pair_slot_resolve(a, q, r_first, nmine, lane, my_t0, my_len);

    // ---- B fragments of the query, resident for the whole wave:
    //      lane l holds B[k = 8 (l >> 4) + j][col = l & 15] = Qtok[q][16 b + (l & 15)][32 ks + 8 (l >> 4) + j] ----
    f16x8 bq[NCB][4];
    {
        const _Float16* src = a.Qtok + ((size_t)q * NCB * 16 + (lane & 15)) * MP_DIM + 8 * (lane >> 4);
#pragma unroll
        for (int b = 0; b < NCB; ++b)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) bq[b][ks] = *reinterpret_cast<const f16x8*>(src + (size_t)b * 16 * MP_DIM + 32 * ks);
    }

    float* const out = a.scores + (size_t)q * a.lds + r_first;
    for (int i = 0; i < nmine; ++i) {
        const int len = __builtin_amdgcn_readlane(my_len, i);
        float* const dst = out + MP_WAVES * i;
        if (len <= 0) {   // absent slot / empty document (sum of an empty max := 0, as in maxsim_tiles.h)
            if (lane == 0) *dst = len < 0 ? -INFINITY : 0.f;
            continue;
        }
        const auto doc = rows.doc(readlane64(my_t0, i), w, lane);
        const int last = len - 1;

        float run[NCB];
#pragma unroll
        for (int b = 0; b < NCB; ++b) run[b] = -INFINITY;

        for (int c0 = 0; c0 < len; c0 += 16 * RB) {
            const int nb = (len - c0 + 15) >> 4;   // row blocks left (wave-uniform); >= 1
            // NB row blocks: every load is issued before the first MFMA; then NB x NCB four-step chains, the row blocks' chains interleaved.
            // The loads stay inside the per-NB branch: one fragment array shared by the branches and filled conditionally spilled.
            auto body = [&](auto NBc) __attribute__((always_inline)) {
                constexpr int NB = decltype(NBc)::value;
                f16x8 af[NB][4];
                rows.template load<NB>(doc, c0, last, lane, af);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    f32x4 acc[NB];
#pragma unroll
                    for (int rb = 0; rb < NB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb][0], bq[cb][0], (f32x4)0.f, 0, 0, 0);
#pragma unroll
                    for (int ks = 1; ks < 4; ++ks)
#pragma unroll
                        for (int rb = 0; rb < NB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb][ks], bq[cb][ks], acc[rb], 0, 0, 0);
                    float m = run[cb];
#pragma unroll
                    for (int rb = 0; rb < NB; ++rb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) m = fmaxf(m, acc[rb][r]);
                    run[cb] = m;
                }
            };
            if constexpr (RB == 4) {
                if (nb >= 4) body(std::integral_constant<int, 4>{});
                else if (nb == 3) body(std::integral_constant<int, 3>{});
                else if (nb == 2) body(std::integral_constant<int, 2>{});
                else body(std::integral_constant<int, 1>{});
            } else {
                if (nb >= 2) body(std::integral_constant<int, 2>{});
                else body(std::integral_constant<int, 1>{});
            }
        }

        const float s0 = pair_token_sum<NCB>(run);
        if (lane == 0) *dst = s0;
    }
}

// The host side both entry points share: the checks in the order of fz_maxsim_f16 (argument errors, then unsupported shapes, then the
// empty batch, then sumL / max_doc_len), and the fill of `s`.  rows_arg / rows_unsupported: what the entry found wrong with its own
// storage arguments, reported in their class's turn.  FZ_OK with Q == 0 or k == 0 means there is nothing to launch.
inline int pair_slots_args(PairSlots& s, bool rows_arg, bool rows_unsupported, const void* Qtok, const int64_t* Doff, int64_t sumL,
                           int max_doc_len, int Q, int Lq, int N, int dim, const int64_t* cand, int ldc, const int32_t* cand_len, int k,
                           int64_t id_base, float* scores, int lds) {
    if (Q < 0 || N < 0 || k < 0 || Lq <= 0 || ldc < k || lds < k) return FZ_ERR_ARG;
    if ((Q != 0 && k != 0) && (!Qtok || !cand || !scores)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if ((Q != 0 && k != 0 && N != 0) && !Doff) return FZ_ERR_ARG;
    if (rows_arg) return FZ_ERR_ARG;
    if (dim != MP_DIM) return FZ_ERR_UNSUPPORTED;
    if (Lq != 32 && Lq != 64 && Lq != 128) return FZ_ERR_UNSUPPORTED;
    if (((uintptr_t)Qtok % 16) || rows_unsupported) return FZ_ERR_UNSUPPORTED;
    if (Q == 0 || k == 0) return FZ_OK;
    if (sumL < 0 || max_doc_len <= 0) return FZ_ERR_ARG;
    if (max_doc_len > MP_MAX_DOC_LEN) return FZ_ERR_UNSUPPORTED;
    s.Qtok = reinterpret_cast<const _Float16*>(Qtok);
    s.Doff = Doff; s.cand = cand; s.cand_len = cand_len; s.scores = scores;
    s.sumL = sumL; s.id_base = id_base; s.ldc = ldc; s.lds = lds; s.Q = Q; s.N = N; s.k = k; s.max_doc_len = max_doc_len;
    s.nslices = (k + MP_SLICE - 1) / MP_SLICE;
    if ((long)Q * s.nslices > 0x7fffffffL) return FZ_ERR_UNSUPPORTED;   // the grid: one workgroup per (query, slice)
    return FZ_OK;
}

}  // namespace fz
