// maxsim8.hip -- K2 over OCP e4m3 token storage: the tile walk of maxsim_tiles.h on gfx950's block-scaled matrix instruction.
//
// Two entry points.  fz_quantize_e4m3_f16 is the token quantiser, a FIXED function of the float16 token: y = x * 2^scale_exp (exact in
// float32), rounded to nearest-even onto the e4m3fn grid (subnormals in steps of 2^-9, -0 keeps its sign), saturated to +-448 (inf
// included), NaN -> 0x7f with the sign kept.  Integer arithmetic on the float32 bits, no hardware conversion: the same function compiles
// for the host, and tests/test_gpu_maxsim_fp8.py holds it to a table-driven numpy quantiser on all 65,536 float16 patterns.
//
// fz_maxsim_e4m3 is fz_maxsim_f16 with one-byte tokens, the same walk (maxsim_tiles.h: read its header first) over another policy:
//     scores[q, d] = 2^-descale_exp * sum_i max_{t < min(len_d, max_doc_len)} <Q8[q, i], D8[t]>,
// the 128-term dot product accumulated in float32 by ONE v_mfma_scale_f32_16x16x128_f8f6f4 (A = 16 document tokens, B = 16 query tokens,
// both e4m3, both hardware scales 2^0 = E8M0 127, C = 0).  The descale multiplies the FINISHED sum, once per (query, document), in the
// epilogue; it is a power of two and therefore exact.  (Folding it into the instruction's E8M0 operands would give the same bits for
// finite scores; it was not built, since the one multiply per score is free and the scales of the instruction stay compile-time constants.)
// What the policy states, against the float16 kernel's:
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
//   * Tile size: 32-row tiles, the walk's (64-row tiles would double the padded rows per document, 16 on average, for no gain in DMA
//     issue).  A tile is 256 lanes' worth of 16-byte DMA pieces, so four waves fill it: waves 0-3 the even slots of a group, waves 4-7
//     the odd ones -- two pieces per wave per group where the float16 kernel issues four.
//   * Column blocks per wave: 8, as in the float16 kernel (64 VGPRs here).  The walk is written for any multiple of 8
//     (M8_BLOCKS_PER_WAVE = 8 gives 16 column blocks in 128 VGPRs and twice the MFMAs per LDS byte); tools/ablate/maxsim8_variants.py
//     builds that variant and tools/bench_maxsim_fp8.py --variant-lib times it against this one, call by call: 48.4 against 52.5 ms at
//     Q = 1024 with equal bits, but 256 VGPRs and 8 of them spilled (12 over the shared walk), and a launch plan of its own -- not
//     shipped.
// Where it stands (profiles/r24_maxsim_fp8.json): 51.5 ms against the float16 kernel's 95.0 at Q = 1024, Lq = 64, N = 27,942 in one
// alternated run = 1.84 x, 2.72 PFLOP/s of the same FLOP count; matrix pipe busy 56 % of the cycles; the VALU folds do not shrink with
// the MFMA count (4.1 other vector instructions per 32-cycle MFMA).
#include "maxsim_tiles.h"

namespace fz {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

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

// ---- the all-pairs kernel: maxsim_tiles.h's walk over the policy below ------------------------------------------------------------
constexpr int M8_BLOCKS_PER_WAVE = 4;   // query blocks of 32 tokens held per wave

struct MaxSim8Args {
    MaxSimTiles t;
    float descale;   // 2^-descale_exp
};

struct E4m3Tiles {
    static constexpr int TILE_BYTES = 32 * MT_DIM;   // 4 KiB
    static constexpr int NA = 2;                     // one A address per chunk
    static constexpr int AHEAD = 2;                  // the folds of a pair of column blocks run under the MFMAs of the next pair
    typedef i32x8 B;
    typedef i32x8 A[2];   // [row block]
    float descale;

    // lane l holds the 16-byte chunks g and g + 4 (g = l >> 4) of query token l & 15 of the block: the same piece the A side reads
    static __device__ __forceinline__ void load_b(const void* Qtok, size_t tok, bool live, int lane, B& b) {
        const unsigned char* src = reinterpret_cast<const unsigned char*>(Qtok) + tok * MT_DIM + 16 * (lane >> 4);
        i32x4 lo = *reinterpret_cast<const i32x4*>(src), hi = *reinterpret_cast<const i32x4*>(src + 64);
        if (!live) { lo = (i32x4)0; hi = (i32x4)0; }
        b = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    // Slot i of a group is filled by the four waves with (w >> 2) == (i & 1).  A wave fills 1 KiB = rows 8p .. 8p+7 (p = w & 3): lane l sits
    // at chunk position l & 7 of row 8p + (l >> 3) and fetches the chunk whose swizzled position that is.
    static __device__ __forceinline__ void dma_tile(const MaxSimTiles& a, unsigned char* ring, int64_t tok0, int base, int i, int w, int lane) {
        if ((i & 1) != (w >> 2)) return;
        const int part = w & 3, row = 8 * part + (lane >> 3), cpos = lane & 7;
        int64_t tok = tok0 + row;
        tok = tok < a.sumL ? tok : a.sumL - 1;   // rows past the end of the corpus: clamp (they are masked)
        const unsigned char* g = reinterpret_cast<const unsigned char*>(a.Dtok) + (size_t)tok * MT_DIM + ((cpos ^ ((row >> 1) & 7)) << 4);
        __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)(ring + (base + i) * TILE_BYTES + part * 1024), 16, 0, 0);
    }
    // lane l reads rows (l & 15) and 16 + (l & 15) (same (r >> 1) & 7 pattern: 16 is a multiple of 16), chunks g and g + 4 at their
    // swizzled positions
    static __device__ __forceinline__ void a_addresses(uint32_t tile_lds, int lane, uint32_t (&aaddr)[NA]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) aaddr[j] = tile_lds + (lane & 15) * 128 + ((((lane >> 4) + 4 * j) ^ ((lane >> 1) & 7)) << 4);
    }
    template <int GI>
    static __device__ __forceinline__ void load_a(const uint32_t (&aaddr)[NA], A& af) {
        i32x4 ah[2][2];   // [row block][chunk]
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ah[rb][j]) : "v"(aaddr[j]), "n"(GI * TILE_BYTES + rb * 2048));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[0][0]), "+v"(ah[0][1]), "+v"(ah[1][0]), "+v"(ah[1][1]));
        af[0] = __builtin_shufflevector(ah[0][0], ah[0][1], 0, 1, 2, 3, 4, 5, 6, 7);
        af[1] = __builtin_shufflevector(ah[1][0], ah[1][1], 0, 1, 2, 3, 4, 5, 6, 7);
    }
    // ONE v_mfma_scale_f32_16x16x128_f8f6f4 per 16 x 16 block (e4m3 x e4m3, both scales 2^0, C = 0)
    static __device__ __forceinline__ f32x4 dot(const i32x8& av, const B& b) {
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, b, (f32x4)0.f, 0, 0, 0, 127, 0, 127);
    }
    static __device__ __forceinline__ void dot2(const A& af, const B& b, f32x4& lo, f32x4& hi) { lo = dot(af[0], b); hi = dot(af[1], b); }
    static __device__ __forceinline__ void dot1(const A& af, const B& b0, const B& b1, f32x4& x, f32x4& y) { x = dot(af[0], b0); y = dot(af[0], b1); }
    // the descale on the finished sum
    __device__ __forceinline__ float finish(float sum) const { return sum * descale; }
};

__global__ __launch_bounds__(512, 2) void maxsim8_kernel(MaxSim8Args a) { maxsim_tiles_walk<M8_BLOCKS_PER_WAVE>(a.t, E4m3Tiles{a.descale}); }

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
    MaxSim8Args a{};
    unsigned nblk;
    hipStream_t st = as_stream(stream);
    // descale_exp out of range (two quantiser exponents of [-8, 15] each fit) and a missing token matrix are argument errors of this storage
    const int rc = maxsim_tiles_args(a.t, nblk, M8_BLOCKS_PER_WAVE, (!Dtok8 && sumL != 0) || descale_exp < -32 || descale_exp > 32,
                                     (uintptr_t)Dtok8 % 16, Qtok8, Doff, sumL, max_doc_len, Q, Lq, N, dim, scores, lds, st);
    if (rc != FZ_OK || nblk == 0) return rc;
    a.t.Dtok = Dtok8;
    a.descale = ldexpf(1.0f, -descale_exp);
    maxsim8_kernel<<<nblk, 512, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
