// maxsim_tiles.h -- K2: exact ColBERT late interaction of every query against every document on gfx950: the tile walk of maxsim.hip
// (float16 tokens) and maxsim8.hip (e4m3 tokens), stated once.
//
// Reference: Ranker.multi_vector_search (hybrid.py:108-137) -> colbert-ai Searcher.search_all; the score
// PLAID approximates is   s(q,d) = sum_{i<Lq} max_{t in d} <Q[q][i], D[t]>    on 128-d
// L2-normalised token vectors (run_colbert.sh:26-27), query padded to 64 tokens (hybrid.py:129).
//
// Mapping: a 16x16 MFMA block with A = 16 DOCUMENT tokens (rows), B = 16 QUERY tokens (cols), the 128 dims its k.  The C layout puts the
// query token on the lane (col = lane & 15) and the 16 document tokens in the 4 accumulator registers x 4 lane groups (row = 4 (lane >> 4)
// + r), so
//     max over document tokens = in-lane max of 4 registers per row block (v_max3), the four lane groups combined ONCE per
//                                document by permlane32 / permlane16 swaps that transpose 8 partial-max registers into 2,
//     sum over query tokens    = one 16-lane DPP sum per register + two swap-and-add steps, once per (query, document).
// A workgroup = 8 waves; every wave keeps the B fragments of 2 * BPW column blocks (BPW query blocks of 32 tokens: 2 queries x 64 tokens at
// BPW = 4) in registers for the whole kernel, and all 8 waves consume the same 32-token document tile (two row blocks whose MFMA chains
// interleave), which goes global -> LDS once per workgroup by LDS-DMA (16-B chunks XOR-swizzled by row so that ds_read_b128 of 16 rows is
// conflict-free), a group of four tiles ahead in an 8-slot ring, one barrier per group.  Tiles are aligned to document starts (rows past
// the end are masked to -inf); a document's last tile with at most 16 tokens left runs its first row block only.  Workgroups that share
// a 32-document range run back-to-back on one XCD, so the range (about 2.4 MB of float16 rows) is fetched from HBM once and served from
// that XCD's L2 to the other query groups.
//
// The tile ring and its schedule.  Tile k lives in slot k % MT_RING.  global_load_lds writes lane l of a wave to (wave-uniform LDS base)
// + 16 l, so the swizzle is applied on the GLOBAL side: a lane fetches the chunk whose swizzled position is where it lands.  No staging
// registers, no ds_write, and the loads of a whole group are in flight for a whole group of MFMA work:
//     start of group g:  issue the DMA of group g + 1 (its slots held group g - 1, which every wave has left);
//     end of group g:    __syncthreads() (= vmcnt(0) + barrier): group g + 1 has landed and is visible to all waves.
// hipcc drains vmcnt before every LDS access it can see while a DMA is pending (it cannot tell the slots apart), which would put the
// whole L2 / HBM latency back in front of every tile.  So inside a group NO LDS access is visible to it: the group's tile metadata and
// the next group's token offsets are read before the DMAs are issued, and the A fragments are fetched by ds_read_b128 written as inline
// asm, with their own s_waitcnt lgkmcnt(0).
//
// The token format is a policy `Rows`; its members are inlined where the statements of the two kernels stood:
//     TILE_BYTES, NA, AHEAD                        bytes of a 32-row tile; per-lane A addresses; column blocks whose MFMAs are issued
//                                                  ahead of the folds in a fully loaded wave (the source order each kernel was timed with)
//     B, A                                         a column block's query fragment; a tile's document fragments (both row blocks)
//     load_b(Qtok, tok, live, lane, b)             b = this lane's piece of query token row `tok`, zero where the block is not live
//     dma_tile(a, ring, tok0, base, i, w, lane)    this wave's share of the DMA of the tile at token row tok0 into slot base + i
//     a_addresses(tile_lds, lane, aaddr)           the per-lane LDS byte offsets, computed ONCE: the slot inside the group's half of the
//                                                  ring and the row block go into the instruction's immediate offset, the ring half is
//                                                  toggled once per group, and the tile loop spends no vector instruction on addressing
//     load_a<GI>(aaddr, af)                        ds_read_b128 + s_waitcnt of the tile in slot GI of the group's half
//     dot2(af, b, lo, hi) / dot1(af, b0, b1, x, y) both row blocks against one column block / the first row block against two
//     finish(sum)                                  what is stored for a finished sum
//
// The launch plan is one for both formats: tests/maxsim_cases.launch_plan restates it.
#pragma once
#include <hip/hip_fp16.h>

#include <type_traits>

#include "common.h"

namespace fz {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MT_DIM = 128;
constexpr int MT_WAVES = 8;
constexpr int MT_DOCS_PER_WG = 32;
constexpr int MT_TABLE = MT_DOCS_PER_WG * 16;   // tile-table entries per workgroup (32 documents x 512 tokens)
constexpr int MT_GROUP = 4;                     // tiles per group: one workgroup barrier per group
constexpr int MT_RING = 2 * MT_GROUP;           // LDS tile slots: the group being read + the group being filled

// what the walk needs whatever the tokens are stored as
struct MaxSimTiles {
    const void* Qtok;       // [Q][Lq][128]
    const void* Dtok;       // [sumL][128]; set by the entry, which checks it
    const int64_t* Doff;    // [N+1]
    float* scores; int lds;
    int Q, Lq, N;
    int QB;                 // Lq / 32
    int QG;                 // query groups = ceil(Q*QB / (MT_WAVES*BPW))
    int DR;                 // document ranges = ceil(N / docs_per_wg)
    int docs_per_wg;        // <= MT_DOCS_PER_WG, chosen so that docs_per_wg * ceil(max_doc_len/32) <= MT_TABLE tiles
    int max_doc_len;        // tokens beyond this are ignored (the reference's doc_maxlen, hybrid.py:129)
    int64_t sumL;
};

// One workgroup = 8 waves x (up to) 2 * BPW column blocks of 16 query tokens; see the header.
template <int BPW, class Rows>
__device__ __forceinline__ void maxsim_tiles_walk(const MaxSimTiles& a, const Rows& rows) {
    typedef __attribute__((address_space(3))) unsigned char lds_byte;
    __shared__ __attribute__((aligned(16))) unsigned char tile[MT_RING][Rows::TILE_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: keep what derives from it in SGPRs
    const int x = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int qg = idx % a.QG;
    const int dr = (idx / a.QG) * 8 + x;
    if (dr >= a.DR) return;

    // ---- this wave's queries.  A group covers 8 waves x qpw queries; the queries of a group that is not full (the last one) are
    //      spread evenly over the waves (at Q = 195, Lq = 64: three waves with one query each instead of two waves with 2 + 1), so
    //      that the group's tile stream is not paced by waves that carry a full load next to idle ones ----
    const int qpw = BPW / a.QB;                                 // queries a wave can hold (BPW = 4, Lq = 32 / 64 / 128: 4 / 2 / 1)
    const int q_first = qg * MT_WAVES * qpw;
    const int nq_group = min(a.Q - q_first, MT_WAVES * qpw);
    const int per_wave = (nq_group + MT_WAVES - 1) / MT_WAVES;  // <= qpw
    const int q0 = q_first + w * per_wave;                      // this wave's first query
    const int nq = max(0, min(per_wave, q_first + nq_group - q0));   // ... and how many it has (wave-uniform)
    const int ncb = nq * a.QB * 2;                              // live column blocks (16 query tokens each) of this wave: 0 .. NCB
    const bool wave_has_queries = nq > 0;

    // ---- B fragments: up to NCB column blocks, resident for the whole kernel; the blocks past ncb are zero ----
    constexpr int NCB = 2 * BPW;
    typename Rows::B bq[NCB];
#pragma unroll
    for (int b = 0; b < NCB; ++b) {
        const bool okb = b < ncb;
        const size_t tok = okb ? ((size_t)q0 * a.QB * 2 + b) * 16 + (lane & 15) : 0;   // a query's tokens are consecutive in [Q * Lq]
        Rows::load_b(a.Qtok, tok, okb, lane, bq[b]);
    }

    const int d_begin = dr * a.docs_per_wg;
    const int d_end = (d_begin + a.docs_per_wg < a.N) ? d_begin + a.docs_per_wg : a.N;

    // ---- tile table of this document range, built ONCE into LDS ------------------------------------------
    // (walking Doff[] with scalar global loads per tile put ~0.5 us of load latency on the critical path of every
    //  0.45 us of MFMA work).  Tiles are aligned to document starts; entry k: first token, valid rows, document, last flag.
    __shared__ int64_t s_tok[MT_TABLE + 4];
    __shared__ int s_meta[MT_TABLE + 4];      // doc_local | rows_valid << 8 | last << 16
    __shared__ int s_len[MT_DOCS_PER_WG];
    __shared__ int s_ntiles;
    if (tid < 64) {   // wave 0; lanes >= MT_DOCS_PER_WG idle along
        const int d = d_begin + lane;
        const bool live = lane < a.docs_per_wg && d < d_end;
        const int64_t t0 = live ? a.Doff[d] : 0;
        int len = live ? (int)(a.Doff[d + 1] - t0) : 0;
        if (len > a.max_doc_len) len = a.max_doc_len;   // caller's doc_maxlen (hybrid.py:129)
        const int nt = (len + 31) >> 5;
        int incl = nt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        const int excl = incl - nt;
        for (int i = 0; i < nt; ++i) {
            const int rows_i = (len - 32 * i) < 32 ? (len - 32 * i) : 32;
            s_tok[excl + i] = t0 + 32 * i;
            s_meta[excl + i] = lane | (rows_i << 8) | ((i == nt - 1) ? (1 << 16) : 0);
        }
        if (lane < MT_DOCS_PER_WG) s_len[lane] = live ? len : -1;
        if (lane == 63) s_ntiles = incl;
    }
    __syncthreads();
    const int ntiles = s_ntiles;
    // An empty document scores 0 for every query (sum of an empty max := 0, as in the oracle).
    if (lane < nq)
        for (int i = 0; i < MT_DOCS_PER_WG; ++i)
            if (s_len[i] == 0) a.scores[(size_t)(q0 + lane) * a.lds + d_begin + i] = 0.f;
    if (ntiles == 0) return;   // block-uniform

    // ---- the first group's DMA (schedule: header) ----
    {
        int64_t toks[MT_GROUP];
#pragma unroll
        for (int i = 0; i < MT_GROUP; ++i) toks[i] = s_tok[i < ntiles ? i : 0];
#pragma unroll
        for (int i = 0; i < MT_GROUP; ++i) if (i < ntiles) Rows::dma_tile(a, &tile[0][0], toks[i], 0, i, w, lane);
    }
    __syncthreads();
    uint32_t aaddr[Rows::NA];
    Rows::a_addresses(__builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_byte*)&tile[0][0]), lane, aaddr);

    float run[NCB];
#pragma unroll
    for (int b = 0; b < NCB; ++b) run[b] = -INFINITY;

    for (int k0 = 0; k0 < ntiles; k0 += MT_GROUP) {
      int metas[MT_GROUP];
      {
        int64_t toks[MT_GROUP];
#pragma unroll
        for (int i = 0; i < MT_GROUP; ++i) {
            metas[i] = __builtin_amdgcn_readfirstlane(s_meta[k0 + i < ntiles ? k0 + i : 0]);
            toks[i] = s_tok[k0 + MT_GROUP + i < ntiles ? k0 + MT_GROUP + i : 0];
        }
#pragma unroll
        for (int i = 0; i < MT_GROUP; ++i)
            if (k0 + MT_GROUP + i < ntiles) Rows::dma_tile(a, &tile[0][0], toks[i], (k0 + MT_GROUP) & (MT_RING - 1), i, w, lane);
      }
      // one tile of the group; GI (compile time) = its slot in the group's half of the ring
      auto tile_body = [&](auto GI) __attribute__((always_inline)) {
        const int meta = metas[decltype(GI)::value];
        const int rows_valid = (meta >> 8) & 0xff;
        const bool last_tile_of_doc = (meta >> 16) & 1;
        // a wave without queries (the tail of the last query group) has nothing to multiply: it only keeps feeding the ring and
        // meeting the barriers
        if (!wave_has_queries) return;

        typename Rows::A af;
        Rows::template load_a<decltype(GI)::value>(aaddr, af);

        // ---- NCB column blocks x 2 row blocks; the 8-way max of a column block is 4 v_max3 ----
        auto fold = [&](f32x4 lo, f32x4 hi, int cb) __attribute__((always_inline)) {
            if (rows_valid < 32) {   // wave-uniform: the last tile of a document.  Row of register r: 4 (lane >> 4) + r (+ 16)
                const int r0 = 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r0 + r >= rows_valid) lo[r] = -INFINITY;
                    if (16 + r0 + r >= rows_valid) hi[r] = -INFINITY;
                }
            }
            float m = run[cb];
#pragma unroll
            for (int r = 0; r < 4; ++r) m = fmaxf(m, lo[r]);
#pragma unroll
            for (int r = 0; r < 4; ++r) m = fmaxf(m, hi[r]);
            run[cb] = m;
        };
        if (rows_valid <= 16) {
            // the last tile of a document with at most 16 tokens left: its second row block is all padding -- only the first one's chains
            // run (half the MFMAs of the tile; tiles are aligned to document starts, so on average 16 of a document's rows are padding)
#pragma unroll
            for (int cb = 0; cb < NCB; cb += 2) {
                if (cb < ncb) {
                    f32x4 aL, bL;
                    Rows::dot1(af, bq[cb], bq[cb + 1], aL, bL);
                    const int r0 = 4 * (lane >> 4);
                    float ma = run[cb], mb = run[cb + 1];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        ma = fmaxf(ma, r0 + r < rows_valid ? aL[r] : -INFINITY);
                        mb = fmaxf(mb, r0 + r < rows_valid ? bL[r] : -INFINITY);
                    }
                    run[cb] = ma; run[cb + 1] = mb;
                }
            }
        } else if (ncb == NCB) {   // wave-uniform: the full load (every wave of every full query group)
            // the folds of AHEAD column blocks run under the MFMAs of the next AHEAD
            constexpr int K = Rows::AHEAD;
            f32x4 lo[2 * K], hi[2 * K];
#pragma unroll
            for (int j = 0; j < K; ++j) Rows::dot2(af, bq[j], lo[j], hi[j]);
#pragma unroll
            for (int cb = 0; cb < NCB; cb += K) {
#pragma unroll
                for (int j = cb + K; j < cb + 2 * K && j < NCB; ++j) Rows::dot2(af, bq[j], lo[j % (2 * K)], hi[j % (2 * K)]);
#pragma unroll
                for (int j = cb; j < cb + K; ++j) fold(lo[j % (2 * K)], hi[j % (2 * K)], j);
            }
        } else {            // a partly loaded wave of the last query group: its live column blocks only (pairs: ncb is even)
#pragma unroll
            for (int cb = 0; cb < NCB; cb += 2) {
                if (cb < ncb) {
                    f32x4 aL, aH, bL, bH;
                    Rows::dot2(af, bq[cb], aL, aH);
                    Rows::dot2(af, bq[cb + 1], bL, bH);
                    fold(aL, aH, cb);
                    fold(bL, bH, cb + 1);
                }
            }
        }
        // ---- end of a document: finish the max over the four 16-lane rows and sum over the query tokens, transposing as we go:
        //      P(A, B) (permlane32 swap + max) leaves [A's rows (0|2), (1|3), B's (0|2), (1|3)], S(X, Y) (permlane16 swap + max) of two
        //      such registers leaves one finished column block per 16-lane row -- 8 registers -> 2, then one 16-lane sum per register
        //      and two more swap steps add the rows up.  28 VALU instead of 64 for the block-by-block form.
        if (last_tile_of_doc) {
            auto P = [&](float A, float B) __attribute__((always_inline)) -> float { swap32(A, B); return fmaxf(A, B); };
            auto S = [&](float X, float Y) __attribute__((always_inline)) -> float { swap16(X, Y); return fmaxf(X, Y); };
            const int d = d_begin + (meta & 0xff);
#pragma unroll
            for (int e = 0; e < NCB / 8; ++e) {   // eight column blocks at a time (one pass at BPW = 4)
                float t0 = row16_sum(S(P(run[8 * e + 0], run[8 * e + 2]), P(run[8 * e + 1], run[8 * e + 3])));   // rows: column blocks 0, 1, 2, 3 (sums over their 16 tokens)
                float t1 = row16_sum(S(P(run[8 * e + 4], run[8 * e + 6]), P(run[8 * e + 5], run[8 * e + 7])));   // rows: column blocks 4, 5, 6, 7
                float o0 = t0, o1 = t1;
                swap16(t0, o0); swap16(t1, o1);
                t0 += o0; t1 += o1;                                              // rows (0,1): blocks 0+1 | rows (2,3): blocks 2+3
                if (a.QB == 1) {        // Lq = 32: a query is two column blocks -- lanes 0 and 32 hold two queries per register
                    if ((lane & 31) == 0) {
                        const int h = 4 * e + (lane >> 5);
                        if (h < nq) a.scores[(size_t)(q0 + h) * a.lds + d] = rows.finish(t0);
                        if (2 + h < nq) a.scores[(size_t)(q0 + 2 + h) * a.lds + d] = rows.finish(t1);
                    }
                } else {
                    o0 = t0; o1 = t1;
                    swap32(t0, o0); swap32(t1, o1);
                    t0 += o0; t1 += o1;                                          // all four rows: (b0 + b1) + (b2 + b3)
                    if (lane == 0) {
                        if (a.QB == 2) {                                         // Lq = 64: one query per register
                            if (2 * e < nq) a.scores[(size_t)(q0 + 2 * e) * a.lds + d] = rows.finish(t0);
                            if (2 * e + 1 < nq) a.scores[(size_t)(q0 + 2 * e + 1) * a.lds + d] = rows.finish(t1);
                        } else if (e < nq) a.scores[(size_t)(q0 + e) * a.lds + d] = rows.finish(t0 + t1);   // Lq = 128: eight column blocks a query
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < NCB; ++b) run[b] = -INFINITY;
        }
      };
      if (k0 + 0 < ntiles) { tile_body(std::integral_constant<int, 0>{});
      if (k0 + 1 < ntiles) { tile_body(std::integral_constant<int, 1>{});
      if (k0 + 2 < ntiles) { tile_body(std::integral_constant<int, 2>{});
      if (k0 + 3 < ntiles) { tile_body(std::integral_constant<int, 3>{}); } } } }
      // the next group lives in the other half of the ring
      const uint32_t flip = (k0 & MT_GROUP) ? (uint32_t)(-MT_GROUP * Rows::TILE_BYTES) : (uint32_t)(MT_GROUP * Rows::TILE_BYTES);
#pragma unroll
      for (int j = 0; j < Rows::NA; ++j) aaddr[j] += flip;
      __syncthreads();   // group boundary: the next group's tiles have landed (vmcnt(0)) and everyone has left this group's
    }
}

// The host side both entry points share: the checks in their order (argument errors, then unsupported shapes, then the empty batch,
// then sumL / max_doc_len, then the all-empty corpus, which is a memset), and the fill of `t` except its token pointers.  rows_arg /
// rows_unsupported: what the entry found wrong with its own storage arguments, reported in their class's turn.  FZ_OK with nblk == 0
// means there is nothing to launch.
inline int maxsim_tiles_args(MaxSimTiles& t, unsigned& nblk, int blocks_per_wave, bool rows_arg, bool rows_unsupported, const void* Qtok,
                             const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N, int dim, float* scores, int lds,
                             hipStream_t st) {
    nblk = 0;
    if (Q < 0 || N < 0 || Lq <= 0 || lds < N) return FZ_ERR_ARG;
    if ((Q != 0 && N != 0) && (!Qtok || !Doff || !scores)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if (rows_arg) return FZ_ERR_ARG;
    if (dim != MT_DIM) return FZ_ERR_UNSUPPORTED;
    if (Lq != 32 && Lq != 64 && Lq != 128) return FZ_ERR_UNSUPPORTED;   // a wave's query blocks (a multiple of 4) hold whole queries
    if (((uintptr_t)Qtok % 16) || rows_unsupported) return FZ_ERR_UNSUPPORTED;
    if (Q == 0 || N == 0) return FZ_OK;
    if (sumL < 0 || max_doc_len <= 0) return FZ_ERR_ARG;
    if (max_doc_len > 32 * MT_TABLE) return FZ_ERR_UNSUPPORTED;   // one document must fit the tile table (16,384 tokens)
    if (sumL == 0) {  // every document empty: all scores 0
        FZ_HIP_TRY(hipMemset2DAsync(scores, (size_t)lds * 4, 0, (size_t)N * 4, (size_t)Q, st));
        return FZ_OK;
    }
    t.Qtok = Qtok; t.Doff = Doff; t.scores = scores; t.lds = lds; t.Q = Q; t.Lq = Lq; t.N = N; t.sumL = sumL;
    t.QB = Lq / 32;
    const int blocks_per_wg = MT_WAVES * blocks_per_wave;
    t.QG = (Q * t.QB + blocks_per_wg - 1) / blocks_per_wg;
    t.max_doc_len = max_doc_len;
    const int tiles_per_doc = (max_doc_len + 31) / 32;
    t.docs_per_wg = MT_TABLE / tiles_per_doc < MT_DOCS_PER_WG ? MT_TABLE / tiles_per_doc : MT_DOCS_PER_WG;
    t.DR = (N + t.docs_per_wg - 1) / t.docs_per_wg;
    const long blocks = 8L * t.QG * ((t.DR + 7) / 8);
    if (blocks > 0x7fffffffL) return FZ_ERR_UNSUPPORTED;
    nblk = (unsigned)blocks;
    return FZ_OK;
}

}  // namespace fz
