// maxsim8.hip -- K2 over OCP e4m3 token storage: the fp8 form of maxsim.hip on gfx950's block-scaled matrix instruction.
//
// Two entry points.  fz_quantize_e4m3_f16 is the token quantiser, a FIXED function of the float16 token: y = x * 2^scale_exp (exact in
// float32), rounded to nearest-even onto the e4m3fn grid (subnormals in steps of 2^-9, -0 keeps its sign), saturated to +-448 (inf
// included), NaN -> 0x7f with the sign kept.  Integer arithmetic on the float32 bits, no hardware conversion: the same function compiles
// for the host, and tests/test_gpu_maxsim_fp8.py holds it to a table-driven numpy quantiser on all 65,536 float16 patterns.
//
// fz_maxsim_e4m3 is fz_maxsim_f16 (maxsim.hip: read its header first) with one-byte tokens:
//     scores[q, d] = 2^-descale_exp * sum_i max_{t < min(len_d, max_doc_len)} <Q8[q, i], D8[t]>,
// the 128-term dot product accumulated in float32 by ONE v_mfma_scale_f32_16x16x128_f8f6f4 (A = 16 document tokens, B = 16 query tokens,
// both e4m3, both hardware scales 2^0 = E8M0 127, C = 0).  The descale multiplies the FINISHED sum, once per (query, document), in the
// epilogue; it is a power of two and therefore exact.  (Folding it into the instruction's E8M0 operands would give the same bits for
// finite scores; it was not built, since the one multiply per score is free and the scales of the instruction stay compile-time constants.)
// The launch plan is the float16 kernel's -- 8 waves, 4 query blocks of 32 tokens per wave (8 column blocks, now 64 VGPRs), 32 documents
// per workgroup, 32-row tiles aligned to document starts, groups of 4 tiles in a ring of 8, one barrier per group, the same tile table,
// v_max3 folds, permlane transpose and XCD-aware block mapping -- so tests/maxsim_cases.py's restatement of it holds for both.  What
// differs:
//   * Operand lane map.  A lane's operand is 32 bytes of one row.  Lane l takes row (l & 15) and the two 16-byte chunks g and g + 4
//     (g = l >> 4) of the row's eight -- for the document row AND the query row.  Whatever order the instruction gives the 128 k inside
//     its four lane groups, both operands see the same permutation, so the dot product is the full one.
//   * Tile and swizzle.  A 32-row tile is 4 KiB: row r at byte 128 r, its chunk c at position c ^ ((r >> 1) & 7).  A ds_read_b128 lane
//     group is 16 lanes that cover the 16 rows once, eight of them with lane group g and eight with g ^ 1 (rows 0-3, 12-15 | 4-11); an
//     LDS bank row is 256 B = two tile rows, so the slot is 8 (r & 1) + position.  Rows of one parity have distinct (r >> 1) & 7, the
//     rows 4-11 are the (r >> 1) in {2, 3, 4, 5}, a set closed under xor 1, so the chunks g and g ^ 1 of the two row sets never meet:
//     16 distinct slots, conflict-free (which is why the second chunk is g + 4 and not 2 g + 1: with adjacent chunks the two sets
//     would differ by xor 2 and collide).  Measured: SQ_LDS_BANK_CONFLICT per launch equals the float16 kernel's count to the digit
//     (the shared tile-table prologue), 0.14 % of the LDS cycles -- the A reads add none (profiles/r24_pmc_maxsim_fp8.json).
//   * Tile size: 32-row tiles, kept (the tile table, max_doc_len limit, document-aligned padding and every edge of the float16 kernel
//     stay as they are; 64-row tiles would double the padded rows per document, 16 on average, for no gain in DMA issue).  A tile is
//     256 lanes' worth of 16-byte DMA pieces, so four waves fill it: waves 0-3 the even slots of a group, waves 4-7 the odd ones --
//     two pieces per wave per group where the float16 kernel issues four.
//   * Column blocks per wave: 8, as in the float16 kernel.  The kernel is written for any multiple of 8 (M8_BLOCKS_PER_WAVE = 8 gives
//     16 column blocks in 128 VGPRs and twice the MFMAs per LDS byte); tools/ablate/maxsim8_variants.py builds that variant and
//     tools/bench_maxsim_fp8.py --variant-lib times it against this one, call by call: 48.4 against 52.5 ms at Q = 1024 with equal
//     bits, but 256 VGPRs and 8 of them spilled, and a launch plan of its own -- not shipped.
// Where it stands (profiles/r24_maxsim_fp8.json): 51.5 ms against the float16 kernel's 95.0 at Q = 1024, Lq = 64, N = 27,942 in one
// alternated run = 1.84 x, 2.72 PFLOP/s of the same FLOP count; matrix pipe busy 56 % of the cycles; the VALU folds do not shrink with
// the MFMA count (4.1 other vector instructions per 32-cycle MFMA).
#include <hip/hip_fp16.h>

#include <type_traits>

#include "common.h"

namespace fz {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- the quantiser ---------------------------------------------------------------------------------------------------------------
// float32 (already scaled) -> e4m3fn byte.  Normal range: round the 23-bit mantissa to 3 bits on the integer pattern (a carry runs
// into the exponent as it should); below 2^-6 the grid is uniform with step 2^-9: round |y| * 512 to an integer 0 .. 8 (8 = 0x08, the
// smallest normal).
__host__ __device__ inline unsigned char e4m3_from_f32(float y) {
    union { float f; uint32_t u; } v;
    v.f = y;
    const uint32_t sign = (v.u >> 24) & 0x80u, a = v.u & 0x7fffffffu;
    if (a > 0x7f800000u) return (unsigned char)(sign | 0x7fu);             // NaN
    uint32_t code;
    if (a < 0x3c800000u) {                                                  // |y| < 2^-6
        v.u = a;
        code = (uint32_t)(int)rintf(v.f * 512.0f);                          // exact product, round to nearest even
    } else {
        const uint32_t r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;         // exponent << 3 | mantissa, nearest even
        code = r - ((127u - 7u) << 3);
        if (r > (((127u + 8u) << 3) | 6u)) code = 0x7eu;                    // above 448 (inf included): saturate
    }
    return (unsigned char)(sign | code);
}

__global__ __launch_bounds__(256) void quantize_e4m3_kernel(const _Float16* __restrict__ src, size_t n, float scale, unsigned char* __restrict__ dst,
                                                            int vec) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t done = 0;
    if (vec) {   // src 16-byte and dst 8-byte aligned: eight values per step
        typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
        const size_t n8 = n >> 3;
        for (size_t i = i0; i < n8; i += stride) {
            const f16x8 x = reinterpret_cast<const f16x8*>(src)[i];
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo |= (uint32_t)e4m3_from_f32((float)x[j] * scale) << (8 * j);
                hi |= (uint32_t)e4m3_from_f32((float)x[4 + j] * scale) << (8 * j);
            }
            reinterpret_cast<uint2*>(dst)[i] = make_uint2(lo, hi);
        }
        done = n8 << 3;
    }
    for (size_t i = done + i0; i < n; i += stride) dst[i] = e4m3_from_f32((float)src[i] * scale);
}

// ---- the all-pairs kernel --------------------------------------------------------------------------------------------------------
constexpr int M8_DIM = 128;
constexpr int M8_WAVES = 8;
constexpr int M8_BLOCKS_PER_WAVE = 4;   // query blocks of 32 tokens held per wave
constexpr int M8_DOCS_PER_WG = 32;
constexpr int M8_TILE_BYTES = 32 * M8_DIM;      // 4 KiB
constexpr int M8_TABLE = M8_DOCS_PER_WG * 16;   // tile-table entries per workgroup (32 documents x 512 tokens)
constexpr int M8_GROUP = 4;                     // tiles per group: one workgroup barrier per group
constexpr int M8_RING = 2 * M8_GROUP;           // LDS tile slots: the group being read + the group being filled

struct MaxSim8Args {
    const unsigned char* Qtok;   // [Q][Lq][128] e4m3
    const unsigned char* Dtok;   // [sumL][128] e4m3
    const int64_t* Doff;         // [N+1]
    float* scores; int lds;
    int Q, Lq, N;
    int QB;                 // Lq / 32
    int QG;                 // query groups = ceil(Q*QB / (M8_WAVES*M8_BLOCKS_PER_WAVE))
    int DR;                 // document ranges = ceil(N / docs_per_wg)
    int docs_per_wg;        // <= M8_DOCS_PER_WG, chosen so that docs_per_wg * ceil(max_doc_len/32) <= M8_TABLE tiles
    int max_doc_len;        // tokens beyond this are ignored
    float descale;          // 2^-descale_exp
    int64_t sumL;
};

// One workgroup = 8 waves x (up to) 8 column blocks of 16 query tokens; see the header and maxsim.hip.
__global__ __launch_bounds__(512, 2) void maxsim8_kernel(MaxSim8Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[M8_RING][M8_TILE_BYTES];   // ring of 4 KiB tiles
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: keep what derives from it in SGPRs
    const int x = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int qg = idx % a.QG;
    const int dr = (idx / a.QG) * 8 + x;
    if (dr >= a.DR) return;

    // ---- this wave's queries: the float16 kernel's assignment (a group that is not full is spread evenly over the waves) ----
    const int qpw = M8_BLOCKS_PER_WAVE / a.QB;                 // queries a wave can hold (Lq = 32 / 64 / 128: 4 / 2 / 1)
    const int q_first = qg * M8_WAVES * qpw;
    const int nq_group = min(a.Q - q_first, M8_WAVES * qpw);
    const int per_wave = (nq_group + M8_WAVES - 1) / M8_WAVES;  // <= qpw
    const int q0 = q_first + w * per_wave;                      // this wave's first query
    const int nq = max(0, min(per_wave, q_first + nq_group - q0));   // ... and how many it has (wave-uniform)
    const int ncb = nq * a.QB * 2;                              // live column blocks (16 query tokens each) of this wave: 0 .. 8
    const bool wave_has_queries = nq > 0;

    // ---- B fragments: up to 8 column blocks, resident for the whole kernel (64 VGPRs) ----
    // lane l holds the 16-byte chunks g and g + 4 (g = l >> 4) of query token l & 15 of the block: the same piece the A side reads
    constexpr int NCB = 2 * M8_BLOCKS_PER_WAVE;
    i32x8 bq[NCB];
#pragma unroll
    for (int b = 0; b < NCB; ++b) {
        const bool okb = b < ncb;
        const size_t tok = okb ? ((size_t)q0 * a.QB * 2 + b) * 16 + (lane & 15) : 0;   // a query's tokens are consecutive in [Q * Lq]
        const unsigned char* src = a.Qtok + tok * M8_DIM + 16 * (lane >> 4);
        i32x4 lo = *reinterpret_cast<const i32x4*>(src), hi = *reinterpret_cast<const i32x4*>(src + 64);
        if (!okb) { lo = (i32x4)0; hi = (i32x4)0; }
        bq[b] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }

    const int d_begin = dr * a.docs_per_wg;
    const int d_end = (d_begin + a.docs_per_wg < a.N) ? d_begin + a.docs_per_wg : a.N;

    // ---- tile table of this document range, built ONCE into LDS: entry k = first token, valid rows, document, last flag ----
    __shared__ int64_t s_tok[M8_TABLE + 4];
    __shared__ int s_meta[M8_TABLE + 4];      // doc_local | rows_valid << 8 | last << 16
    __shared__ int s_len[M8_DOCS_PER_WG];
    __shared__ int s_ntiles;
    if (tid < 64) {   // wave 0; lanes >= M8_DOCS_PER_WG idle along
        const int d = d_begin + lane;
        const bool live = lane < a.docs_per_wg && d < d_end;
        const int64_t t0 = live ? a.Doff[d] : 0;
        int len = live ? (int)(a.Doff[d + 1] - t0) : 0;
        if (len > a.max_doc_len) len = a.max_doc_len;
        const int nt = (len + 31) >> 5;
        int incl = nt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        const int excl = incl - nt;
        for (int i = 0; i < nt; ++i) {
            const int rows = (len - 32 * i) < 32 ? (len - 32 * i) : 32;
            s_tok[excl + i] = t0 + 32 * i;
            s_meta[excl + i] = lane | (rows << 8) | ((i == nt - 1) ? (1 << 16) : 0);
        }
        if (lane < M8_DOCS_PER_WG) s_len[lane] = live ? len : -1;
        if (lane == 63) s_ntiles = incl;
    }
    __syncthreads();
    const int ntiles = s_ntiles;
    // An empty document scores 0 for every query (sum of an empty max := 0).
    if (lane < nq)
        for (int i = 0; i < M8_DOCS_PER_WG; ++i)
            if (s_len[i] == 0) a.scores[(size_t)(q0 + lane) * a.lds + d_begin + i] = 0.f;
    if (ntiles == 0) return;   // block-uniform

    // ---- tile ring, filled by LDS-DMA.  Tile k lives in slot k % M8_RING; a tile is 32 rows x 128 B, row r's 16-B chunks XOR-swizzled
    // by (r >> 1) & 7 (header).  global_load_lds writes lane l of a wave to (wave-uniform LDS base) + 16 l, so the swizzle is applied on
    // the GLOBAL side: a wave fills 1 KiB = rows 8p .. 8p+7 (p = w & 3), lane l sits at chunk position l & 7 of row 8p + (l >> 3) and
    // fetches the chunk whose swizzled position that is.  Slot i of a group is filled by the four waves with (w >> 2) == (i & 1).
    // Schedule and the reason for the inline-asm reads: maxsim.hip.
    const int dma_half = w >> 2, dma_part = w & 3;
    auto dma_tile = [&](int64_t tok0, int slot) {
        const int row = 8 * dma_part + (lane >> 3), cpos = lane & 7;
        int64_t tok = tok0 + row;
        tok = tok < a.sumL ? tok : a.sumL - 1;   // rows past the end of the corpus: clamp (they are masked)
        const unsigned char* g = a.Dtok + (size_t)tok * M8_DIM + ((cpos ^ ((row >> 1) & 7)) << 4);
        __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)(&tile[slot][dma_part * 1024]), 16, 0, 0);
    };
    {
        int64_t toks[M8_GROUP];
#pragma unroll
        for (int i = 0; i < M8_GROUP; ++i) toks[i] = s_tok[i < ntiles ? i : 0];
#pragma unroll
        for (int i = 0; i < M8_GROUP; ++i) if (i < ntiles && (i & 1) == dma_half) dma_tile(toks[i], i);
    }
    __syncthreads();
    const uint32_t tile_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&tile[0][0]);

    // A-fragment addresses: lane l reads rows (l & 15) and 16 + (l & 15) (same (r >> 1) & 7 pattern: 16 is a multiple of 16), chunks g
    // and g + 4 at their swizzled positions.  Computed ONCE; slot and row block go into the instruction's immediate offset.
    uint32_t aaddr[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) aaddr[j] = tile_lds + (lane & 15) * 128 + ((((lane >> 4) + 4 * j) ^ ((lane >> 1) & 7)) << 4);

    float run[NCB];
#pragma unroll
    for (int b = 0; b < NCB; ++b) run[b] = -INFINITY;

    for (int k0 = 0; k0 < ntiles; k0 += M8_GROUP) {
      int metas[M8_GROUP];
      {
        int64_t toks[M8_GROUP];
#pragma unroll
        for (int i = 0; i < M8_GROUP; ++i) {
            metas[i] = __builtin_amdgcn_readfirstlane(s_meta[k0 + i < ntiles ? k0 + i : 0]);
            toks[i] = s_tok[k0 + M8_GROUP + i < ntiles ? k0 + M8_GROUP + i : 0];
        }
#pragma unroll
        for (int i = 0; i < M8_GROUP; ++i)
            if (k0 + M8_GROUP + i < ntiles && (i & 1) == dma_half) dma_tile(toks[i], ((k0 + M8_GROUP) & (M8_RING - 1)) + i);
      }
      // one tile of the group; GI (compile time) = its slot in the group's half of the ring
      auto tile_body = [&](auto GI) __attribute__((always_inline)) {
        constexpr int gi = decltype(GI)::value;
        const int meta = metas[gi];
        const int rows_valid = (meta >> 8) & 0xff;
        const bool last_tile_of_doc = (meta >> 16) & 1;
        // a wave without queries (the tail of the last query group) only keeps feeding the ring and meeting the barriers
        if (!wave_has_queries) return;

        i32x4 ah[2][2];   // [row block][chunk]
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ah[rb][j]) : "v"(aaddr[j]), "n"(gi * M8_TILE_BYTES + rb * 2048));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[0][0]), "+v"(ah[0][1]), "+v"(ah[1][0]), "+v"(ah[1][1]));
        const i32x8 a0 = __builtin_shufflevector(ah[0][0], ah[0][1], 0, 1, 2, 3, 4, 5, 6, 7);
        const i32x8 a1 = __builtin_shufflevector(ah[1][0], ah[1][1], 0, 1, 2, 3, 4, 5, 6, 7);

        // ---- 8 column blocks x 2 row blocks, ONE v_mfma_scale_f32_16x16x128_f8f6f4 each (e4m3 x e4m3, both scales 2^0, C = 0); the
        //      8-way max of a column block is 4 v_max3 ------------------------------------------------------------------------------
        auto dot = [&](const i32x8& av, int cb) __attribute__((always_inline)) -> f32x4 {
            return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bq[cb], (f32x4)0.f, 0, 0, 0, 127, 0, 127);
        };
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
            // the last tile of a document with at most 16 tokens left: its second row block is all padding -- the first one only
#pragma unroll
            for (int cb = 0; cb < NCB; cb += 2) {
                if (cb < ncb) {
                    const f32x4 aL = dot(a0, cb), bL = dot(a0, cb + 1);
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
            f32x4 aL, aH, bL, bH;
            aL = dot(a0, 0); aH = dot(a1, 0);
            bL = dot(a0, 1); bH = dot(a1, 1);
#pragma unroll
            for (int cb = 0; cb < NCB; cb += 2) {   // the folds of a pair run under the MFMAs of the next one
                const f32x4 pL = aL, pH = aH, qL = bL, qH = bH;
                if (cb + 2 < NCB) {
                    aL = dot(a0, cb + 2); aH = dot(a1, cb + 2);
                    bL = dot(a0, cb + 3); bH = dot(a1, cb + 3);
                }
                fold(pL, pH, cb);
                fold(qL, qH, cb + 1);
            }
        } else {            // a partly loaded wave of the last query group: its live column blocks only (pairs: ncb is even)
#pragma unroll
            for (int cb = 0; cb < NCB; cb += 2) {
                if (cb < ncb) {
                    const f32x4 aL = dot(a0, cb), aH = dot(a1, cb), bL = dot(a0, cb + 1), bH = dot(a1, cb + 1);
                    fold(aL, aH, cb);
                    fold(bL, bH, cb + 1);
                }
            }
        }
        // ---- end of a document: the float16 kernel's transpose and sums (maxsim.hip), then the descale on the finished sum ----
        if (last_tile_of_doc) {
            auto P = [&](float A, float B) __attribute__((always_inline)) -> float { swap32(A, B); return fmaxf(A, B); };
            auto S = [&](float X, float Y) __attribute__((always_inline)) -> float { swap16(X, Y); return fmaxf(X, Y); };
            const int d = d_begin + (meta & 0xff);
#pragma unroll
            for (int e = 0; e < NCB / 8; ++e) {   // eight column blocks at a time (one pass: NCB = 8)
                float t0 = row16_sum(S(P(run[8 * e + 0], run[8 * e + 2]), P(run[8 * e + 1], run[8 * e + 3])));   // rows: column blocks 0, 1, 2, 3 (sums over their 16 tokens)
                float t1 = row16_sum(S(P(run[8 * e + 4], run[8 * e + 6]), P(run[8 * e + 5], run[8 * e + 7])));   // rows: column blocks 4, 5, 6, 7
                float o0 = t0, o1 = t1;
                swap16(t0, o0); swap16(t1, o1);
                t0 += o0; t1 += o1;                                              // rows (0,1): blocks 0+1 | rows (2,3): blocks 2+3
                if (a.QB == 1) {        // Lq = 32: a query is two column blocks -- lanes 0 and 32 hold two queries per register
                    if ((lane & 31) == 0) {
                        const int h = 4 * e + (lane >> 5);
                        if (h < nq) a.scores[(size_t)(q0 + h) * a.lds + d] = t0 * a.descale;
                        if (2 + h < nq) a.scores[(size_t)(q0 + 2 + h) * a.lds + d] = t1 * a.descale;
                    }
                } else {
                    o0 = t0; o1 = t1;
                    swap32(t0, o0); swap32(t1, o1);
                    t0 += o0; t1 += o1;                                          // all four rows: (b0 + b1) + (b2 + b3)
                    if (lane == 0) {
                        if (a.QB == 2) {                                         // Lq = 64: one query per register
                            if (2 * e < nq) a.scores[(size_t)(q0 + 2 * e) * a.lds + d] = t0 * a.descale;
                            if (2 * e + 1 < nq) a.scores[(size_t)(q0 + 2 * e + 1) * a.lds + d] = t1 * a.descale;
                        } else if (e < nq) a.scores[(size_t)(q0 + e) * a.lds + d] = (t0 + t1) * a.descale;   // Lq = 128: eight column blocks a query
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
      const uint32_t flip = (k0 & M8_GROUP) ? (uint32_t)(-M8_GROUP * M8_TILE_BYTES) : (uint32_t)(M8_GROUP * M8_TILE_BYTES);
      aaddr[0] += flip; aaddr[1] += flip;
      __syncthreads();   // group boundary: the next group's tiles have landed (vmcnt(0)) and everyone has left this group's
    }
}

}  // namespace fz

using namespace fz;

extern "C" int fz_quantize_e4m3_f16(const void* src, int64_t n, int scale_exp, void* dst, void* stream) {
    if (n < 0 || scale_exp < -8 || scale_exp > 15) return FZ_ERR_ARG;
    if (n != 0 && (!src || !dst)) return FZ_ERR_ARG;
    if ((uintptr_t)src % 2) return FZ_ERR_UNSUPPORTED;
    if (n == 0) return FZ_OK;
    const int vec = ((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 8 == 0) ? 1 : 0;
    const int64_t work = vec ? (n + 7) / 8 : n;
    int64_t blocks = (work + 255) / 256;
    if (blocks > 8192) blocks = 8192;   // grid-stride beyond: 32 workgroups per CU
    quantize_e4m3_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(reinterpret_cast<const _Float16*>(src), (size_t)n, ldexpf(1.0f, scale_exp),
                                                                         reinterpret_cast<unsigned char*>(dst), vec);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_maxsim_e4m3(const void* Qtok8, const void* Dtok8, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N,
                              int dim, int descale_exp, float* scores, int lds, void* stream) {
    if (Q < 0 || N < 0 || Lq <= 0 || lds < N) return FZ_ERR_ARG;
    if (descale_exp < -32 || descale_exp > 32) return FZ_ERR_ARG;   // two quantiser exponents of [-8, 15] each fit
    if ((Q != 0 && N != 0) && (!Qtok8 || !Doff || !scores)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if (!Dtok8 && sumL != 0) return FZ_ERR_ARG;   // an empty token matrix (every document empty) has no pointer to give
    if (dim != M8_DIM) return FZ_ERR_UNSUPPORTED;
    if (Lq != 32 && Lq != 64 && Lq != 128) return FZ_ERR_UNSUPPORTED;   // a wave's M8_BLOCKS_PER_WAVE query blocks hold whole queries
    if (((uintptr_t)Qtok8 % 16) || ((uintptr_t)Dtok8 % 16)) return FZ_ERR_UNSUPPORTED;
    if (Q == 0 || N == 0) return FZ_OK;
    hipStream_t st = as_stream(stream);
    if (sumL < 0 || max_doc_len <= 0) return FZ_ERR_ARG;
    if (max_doc_len > 32 * M8_TABLE) return FZ_ERR_UNSUPPORTED;   // one document must fit the tile table (16,384 tokens)
    if (sumL == 0) {  // every document empty: all scores 0
        FZ_HIP_TRY(hipMemset2DAsync(scores, (size_t)lds * 4, 0, (size_t)N * 4, (size_t)Q, st));
        return FZ_OK;
    }
    MaxSim8Args a{};
    a.Qtok = reinterpret_cast<const unsigned char*>(Qtok8);
    a.Dtok = reinterpret_cast<const unsigned char*>(Dtok8);
    a.Doff = Doff; a.scores = scores; a.lds = lds; a.Q = Q; a.Lq = Lq; a.N = N; a.sumL = sumL;
    a.QB = Lq / 32;
    const int blocks_per_wg = M8_WAVES * M8_BLOCKS_PER_WAVE;
    a.QG = (Q * a.QB + blocks_per_wg - 1) / blocks_per_wg;
    a.max_doc_len = max_doc_len;
    a.descale = ldexpf(1.0f, -descale_exp);
    const int tiles_per_doc = (max_doc_len + 31) / 32;
    a.docs_per_wg = M8_TABLE / tiles_per_doc < M8_DOCS_PER_WG ? M8_TABLE / tiles_per_doc : M8_DOCS_PER_WG;
    a.DR = (N + a.docs_per_wg - 1) / a.docs_per_wg;
    const long nblk = 8L * a.QG * ((a.DR + 7) / 8);
    if (nblk > 0x7fffffffL) return FZ_ERR_UNSUPPORTED;
    maxsim8_kernel<<<(unsigned)nblk, 512, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
