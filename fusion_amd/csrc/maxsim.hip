// maxsim.hip -- K2 over float16 tokens: the tile walk of maxsim_tiles.h (read its header first) on v_mfma_f32_16x16x32_f16.
//
// Operand lane map: A = 16 document tokens (rows) x 32 dims, B = 32 dims x 16 query tokens (cols), four k-steps for the 128 dims from a
// zero accumulator.  Lane l holds B[k = 8 (l >> 4) + j][col = l & 15] = Qtok[token l & 15 of the block][dim 32 ks + 8 (l >> 4) + j]; the 8
// column blocks of a wave are 128 VGPRs.  Tile and swizzle: a tile is 32 rows x 256 B = 8 KiB, row r's 16-B chunks XOR-swizzled by r & 15
// (conflict-free ds_read_b128 of 16 rows x one chunk).  Every wave fills rows 4w .. 4w+3 of every slot.
//
// Where it stands (profiles/r03_pmc_maxsim.json, r03_maxsim_ab.jsonl): 1.42-1.46 PFLOP/s of exact
// sum-of-lengths FLOPs at Q = 1024 = 0.57-0.58 of the 2.5 PF nominal peak, matrix pipe busy 62 % of the SIMD cycles, 1.3 other
// vector instructions per 16-cycle MFMA, LDS conflicts 0.06 % -- what MI355X_MICROARCH.md measures for an LDS-fed 16x16x32 loop
// on random data (1.40-1.43 PF: the chip holds its clock down under matrix load).  What alignment to document starts costs: with
// the LLeQA-shaped lengths of the bench 2.5 % of the row-block slots are padding (7.5 of ~300 rows per document), so tiles
// packed across document boundaries could add at most that much -- 1.43 -> <= 1.47 PF -- for a piece-wise epilogue in every
// tile; not built (round 4, DESIGN.md 'Tried').  The round-2 32x32x16 form is kept as tools/ablate/maxsim_32x32x16.hip.
#include "maxsim_tiles.h"

namespace fz {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int MS_BLOCKS_PER_WAVE = 4;   // query blocks of 32 tokens held per wave

struct F16Tiles {
    static constexpr int TILE_BYTES = 32 * MT_DIM * 2;   // 8 KiB
    static constexpr int NA = 4;                         // one A address per k-step
    static constexpr int AHEAD = 1;                      // the chains of column block cb + 1 are issued before the fold of cb
    typedef f16x8 B[4];      // [k-step]
    typedef f16x8 A[2][4];   // [row block][k-step]

    static __device__ __forceinline__ void load_b(const void* Qtok, size_t tok, bool live, int lane, B& b) {
        const _Float16* src = reinterpret_cast<const _Float16*>(Qtok) + tok * MT_DIM + 8 * (lane >> 4);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            f16x8 v = *reinterpret_cast<const f16x8*>(src + 32 * ks);
            if (!live) v = (f16x8)(_Float16)0;
            b[ks] = v;
        }
    }
    // wave w fills rows 4w .. 4w+3: lane l sits at chunk position l & 15 of row 4w + (l >> 4) and fetches the chunk whose swizzled position that is
    static __device__ __forceinline__ void dma_tile(const MaxSimTiles& a, unsigned char* ring, int64_t tok0, int base, int i, int w, int lane) {
        const int row = 4 * w + (lane >> 4), cpos = lane & 15;
        int64_t tok = tok0 + row;
        tok = tok < a.sumL ? tok : a.sumL - 1;   // rows past the end of the corpus: clamp (they are masked)
        const _Float16* g = reinterpret_cast<const _Float16*>(a.Dtok) + (size_t)tok * MT_DIM + ((cpos ^ (row & 15)) << 3);
        __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)(ring + (base + i) * TILE_BYTES + w * 1024), 16, 0, 0);
    }
    // lane l reads rows (l & 15) and 16 + (l & 15), dims 32 ks + 8 (l >> 4) .. + 7 = chunk 4 ks + (l >> 4) of the row at its swizzled
    // position (16 lanes = 16 rows x one chunk each = 16 distinct positions: conflict-free)
    static __device__ __forceinline__ void a_addresses(uint32_t tile_lds, int lane, uint32_t (&aaddr)[NA]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) aaddr[ks] = tile_lds + (lane & 15) * 256 + (((4 * ks + (lane >> 4)) ^ (lane & 15)) << 4);
    }
    template <int GI>
    static __device__ __forceinline__ void load_a(const uint32_t (&aaddr)[NA], A& af) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[rb][ks]) : "v"(aaddr[ks]), "n"(GI * TILE_BYTES + rb * 4096));
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[0][2]), "+v"(af[0][3]), "+v"(af[1][0]), "+v"(af[1][1]), "+v"(af[1][2]), "+v"(af[1][3]));
    }
    // 2 x 4 k-steps: the two chains interleave (no MFMA waits for the one before it)
    static __device__ __forceinline__ void dot2(const A& af, const B& b, f32x4& lo, f32x4& hi) {
        lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][0], b[0], (f32x4)0.f, 0, 0, 0);
        hi = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1][0], b[0], (f32x4)0.f, 0, 0, 0);
#pragma unroll
        for (int ks = 1; ks < 4; ++ks) {
            lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][ks], b[ks], lo, 0, 0, 0);
            hi = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1][ks], b[ks], hi, 0, 0, 0);
        }
    }
    static __device__ __forceinline__ void dot1(const A& af, const B& b0, const B& b1, f32x4& x, f32x4& y) {
        x = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][0], b0[0], (f32x4)0.f, 0, 0, 0);
        y = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][0], b1[0], (f32x4)0.f, 0, 0, 0);
#pragma unroll
        for (int ks = 1; ks < 4; ++ks) {
            x = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][ks], b0[ks], x, 0, 0, 0);
            y = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][ks], b1[ks], y, 0, 0, 0);
        }
    }
    __device__ __forceinline__ float finish(float sum) const { return sum; }
};

__global__ __launch_bounds__(512, 2) void maxsim_kernel(MaxSimTiles a) { maxsim_tiles_walk<MS_BLOCKS_PER_WAVE>(a, F16Tiles{}); }

}  // namespace fz

using namespace fz;

extern "C" int fz_maxsim_f16(const void* Qtok, const void* Dtok, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N,
                             int dim, float* scores, int lds, void* stream) {
    MaxSimTiles a{};
    unsigned nblk;
    hipStream_t st = as_stream(stream);
    const int rc = maxsim_tiles_args(a, nblk, MS_BLOCKS_PER_WAVE, !Dtok && sumL != 0,   // an empty token matrix (every document empty) has no pointer to give
                                     (uintptr_t)Dtok % 16, Qtok, Doff, sumL, max_doc_len, Q, Lq, N, dim, scores, lds, st);
    if (rc != FZ_OK || nblk == 0) return rc;
    a.Dtok = Dtok;
    maxsim_kernel<<<nblk, 512, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
