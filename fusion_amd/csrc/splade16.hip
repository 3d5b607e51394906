// splade16.hip -- the SPLADE head of the mixed-precision encoder for gfx950: float16 operands, float32 accumulation.
//
//   fz_splade_head_max_f16    pool[s][v] = max over the rows t of sequence s of log1p(relu(<X16[t], W16[v]> + bias[v]))
//   fz_splade_head_f16_tile   (host only) the tile constants below
//
// The float32 head (score.hip, EPI_SPLADE) with the operands halved and v_mfma_f32_32x32x16_f16 in place of v_mfma_f32_32x32x2_f32: products of
// float16 values are exact in float32, the sum runs in float32 on the matrix pipe, and the [T, V] logits are never written.  Hidden values
// are finite by contract (the float16 encoder path lives with the float16 range anyway).
//
// Structure: 128 x 128 output tile per 256-thread workgroup (2 x 2 waves, each 64 x 64 = 2 x 2 MFMA blocks, 64 accumulator VGPRs), k-tile of
// 64 halves = four MFMA k-steps of 16, both operands k-contiguous.  An LDS row holds the k-tile's 128 bytes + 16 bytes of padding (144 B, the
// row stride of score.hip's float32 tiles): the operand fragment of lane l is the 16 bytes at row l & 31, k-offset 8 (l >> 5) halves -- one
// ds_read_b128 per 32 x 16 operand block, conflict-free over consecutive rows at that stride; four reads feed four MFMAs of a k-step.
// Operands travel HBM -> registers one k-tile ahead of the MFMAs and registers -> LDS into the stage read one k-tile ago (two LDS stages, one
// barrier per k-tile).  The grid is persistent (two workgroups per CU) and a workgroup's tiles form ONE stream of k-tiles: the first k-tile of
// the next tile is fetched under the last k-tile of the current one, and a tile's pooling epilogue runs with the next tile's operands already
// in LDS.  Tile ids are XCD-aware as in score.hip: the row blocks of one vocabulary tile are consecutive ids on one XCD (id % 8), so a
// W16 tile is fetched from HBM once and hit in that XCD's L2 afterwards.
#include <algorithm>

#include "common.h"

namespace fz {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float h16acc __attribute__((ext_vector_type(16)));

constexpr int H16_BM = 128, H16_BN = 128;   // output tile: token rows x vocabulary columns
constexpr int H16_BK = 64, H16_KS = 16;     // k-tile and MFMA k-step, in halves
constexpr int H16_LD = H16_BK + 8;          // LDS row: 72 halves = 144 B
constexpr int H16_BUF = (H16_BM + H16_BN) * H16_LD;   // one stage, in halves: [X tile: 128 rows | W tile: 128 rows][H16_LD]

struct Head16Args {
    const _Float16* X; int ldx;   // packed hidden rows [T][ldx]
    const _Float16* W; int ldw;   // vocabulary projection [V][ldw]
    const float* bias;            // [V]
    const int32_t* cu_rows;       // [nseq + 1] first packed row of every sequence
    int nseq, T, V, d;
    int QB, TN, ids;              // 128-row blocks, 128-column vocabulary tiles, tile ids (incl. the XCD padding, which decodes to nothing)
    float* pool; int ldp;         // [nseq][ldp], zero-initialised
};

template <bool RAGGED /* d is not a whole number of k-tiles */>
__global__ __launch_bounds__(256, 2) void splade_head_f16_kernel(Head16Args g) {
    extern __shared__ __attribute__((aligned(16))) _Float16 lds16[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int G = (int)gridDim.x;

    // tile id -> (token row, vocabulary column) of its corner
    auto decode = [&](int b, int& row0, int& col0) -> bool {
        const int x = b & 7, idx = b >> 3;
        const int vt = (idx / g.QB) * 8 + x;
        row0 = (idx % g.QB) * H16_BM;
        col0 = vt * H16_BN;
        return vt < g.TN;
    };
    auto next_tile = [&](int b, int& row0, int& col0) -> int {   // first decodable id >= b of this workgroup's sequence, or -1
        for (; b < g.ids; b += G)
            if (decode(b, row0, col0)) return b;
        return -1;
    };
    int crow, ccol, lrow = 0, lcol = 0;
    int cur_b = next_tile((int)blockIdx.x, crow, ccol);
    if (cur_b < 0) return;

    // staging: thread -> (row = tid / 8 + 32 i, 8 halves at k = 8 (tid % 8)).  Rows past the end are clamped to the last one: their products
    // are computed and never pooled (the epilogue stops at T and at V).  d % 8 == 0: a 16-byte piece lies entirely inside or outside d; one
    // outside re-reads the row's last piece and is zeroed on its way into LDS, which is exact.
    const int srow = tid >> 3, sk = (tid & 7) * 8;
    const _Float16* abase;
    const _Float16* bbase;
    int32_t oa[4], ob[4];      // element offsets inside one operand tile (the host checks 128 * ld against 2^31 bytes)
    auto point_at = [&](int row0, int col0) {
        abase = g.X + (size_t)row0 * g.ldx;
        bbase = g.W + (size_t)col0 * g.ldw;
#pragma unroll
        for (int i = 0; i < 4; ++i) oa[i] = min(srow + 32 * i, g.T - 1 - row0) * g.ldx;
#pragma unroll
        for (int i = 0; i < 4; ++i) ob[i] = min(srow + 32 * i, g.V - 1 - col0) * g.ldw;
    };
    const int KT = (g.d + H16_BK - 1) / H16_BK;
    uint4 ra[4], rb[4];
    auto gload = [&](int kt) __attribute__((always_inline)) {
        int k = kt * H16_BK + sk;
        if constexpr (RAGGED) k = min(k, g.d - 8);
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const uint4*>(abase + oa[i] + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) rb[i] = *reinterpret_cast<const uint4*>(bbase + ob[i] + k);
    };
    auto sstore = [&](int buf, int kt) __attribute__((always_inline)) {   // kt: the k-tile the registers hold
        _Float16* As = lds16 + buf * H16_BUF;
        _Float16* Bs = As + H16_BM * H16_LD;
        const uint32_t m = RAGGED && kt * H16_BK + sk >= g.d ? 0u : ~0u;
        auto keep = [&](uint4 v) { return RAGGED ? make_uint4(v.x & m, v.y & m, v.z & m, v.w & m) : v; };
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(As + (srow + 32 * i) * H16_LD + sk) = keep(ra[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(Bs + (srow + 32 * i) * H16_LD + sk) = keep(rb[i]);
    };

    // operand maps of v_mfma_f32_32x32x16_f16: lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31], j = 0..7
    h16acc acc[2][2];
    const int aoff = (wr * 64 + (lane & 31)) * H16_LD + 8 * (lane >> 5);
    const int boff = H16_BM * H16_LD + (wc * 64 + (lane & 31)) * H16_LD + 8 * (lane >> 5);
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const _Float16* As = lds16 + buf * H16_BUF + aoff;
        const _Float16* Bs = lds16 + buf * H16_BUF + boff;
        // the fragments of k-step ks + 1 are read before the MFMAs of k-step ks: four ds_read_b128 per four MFMAs, one per MFMA gap
        h16x8 a[2][2], b[2][2];
        auto fread = [&](int s, int ks) __attribute__((always_inline)) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[s][mi] = *reinterpret_cast<const h16x8*>(As + mi * 32 * H16_LD + ks * H16_KS);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) b[s][ni] = *reinterpret_cast<const h16x8*>(Bs + ni * 32 * H16_LD + ks * H16_KS);
        };
        fread(0, 0);
#pragma unroll
        for (int ks = 0; ks < H16_BK / H16_KS; ++ks) {
            if (ks + 1 < H16_BK / H16_KS) fread((ks + 1) & 1, ks + 1);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks & 1][mi], b[ks & 1][ni], acc[mi][ni], 0, 0, 0);
        }
    };

    point_at(crow, ccol);
    gload(0);
    sstore(0, 0);
    __syncthreads();
    int buf = 0;
    while (true) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.0f;
        int nxt = -1;
        for (int kt = 0; kt < KT; ++kt) {
            const bool last = kt + 1 == KT;
            if (last) {                                   // the stream goes on with the next tile's first k-tile
                nxt = next_tile(cur_b + G, lrow, lcol);
                if (nxt >= 0) point_at(lrow, lcol);
            }
            const bool more = !last || nxt >= 0;          // workgroup-uniform
            const int lk = last ? 0 : kt + 1;
            if (more) gload(lk);
            compute(buf);
            if (more) sstore(buf ^ 1, lk);                // into the stage read one k-tile ago: its reads all ended before the previous barrier
            __syncthreads();
            buf ^= 1;
        }

        // SPLADE-max pooling, restated from score.hip's EPI_SPLADE epilogue (the C/D layout of the 32x32x16 is that of the 32x32x2: column =
        // lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)).  log1p o relu is monotone: the max over a sequence's rows is taken on the raw
        // dot products, the bias added and the transform applied once per (sequence, column), and the result -- a non-negative float, whose
        // bit pattern orders like an unsigned integer -- goes into the zero-initialised pool by atomicMax.  A wave's 64 rows are cut at the
        // sequence boundaries; per piece: an in-lane max over the accumulator registers whose row lies in the piece, one permlane32 swap to
        // join the lane halves, and one atomic per column from lanes 0-31.
        {
            const int R0 = crow + wr * 64;
            const int Rend = min(R0 + 64, g.T);
            if (R0 < Rend) {      // wave-uniform
                int lo_s = 0, hi_s = g.nseq;             // first sequence that ends after R0
                while (lo_s < hi_s) { const int mid = (lo_s + hi_s) >> 1; if (g.cu_rows[mid + 1] > R0) hi_s = mid; else lo_s = mid + 1; }
                const int h4 = 4 * (lane >> 5);
                for (int sq = lo_s; sq < g.nseq; ++sq) {
                    const int a0 = g.cu_rows[sq], a1 = g.cu_rows[sq + 1];
                    if (a0 >= Rend) break;
                    const int lo = max(a0, R0) - R0, hi = min(a1, Rend) - R0;     // piece [lo, hi) of the wave's rows
                    if (lo >= hi) continue;                                           // (an empty sequence)
                    float m[2] = {-INFINITY, -INFINITY};
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = mi * 32 + (r & 3) + 8 * (r >> 2) + h4;
                            const bool in = row >= lo && row < hi;
#pragma unroll
                            for (int ni = 0; ni < 2; ++ni) m[ni] = fmaxf(m[ni], in ? acc[mi][ni][r] : -INFINITY);
                        }
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        float other = m[ni];
                        swap32(m[ni], other);                 // m = [lo half, lo half], other = [hi half, hi half]
                        const float best = fmaxf(m[ni], other);
                        const int c = ccol + wc * 64 + ni * 32 + (lane & 31);
                        if (lane < 32 && c < g.V) {
                            const float logit = best + g.bias[c];
                            const float v = log1pf(fmaxf(logit, 0.0f));
                            if (v > 0.0f) atomicMax(reinterpret_cast<unsigned int*>(g.pool + (size_t)sq * g.ldp + c), __float_as_uint(v));
                        }
                    }
                }
            }
        }
        if (nxt < 0) break;
        cur_b = nxt; crow = lrow; ccol = lcol;
    }
}

}  // namespace fz

using namespace fz;

extern "C" int fz_splade_head_f16_tile(int* rows, int* cols, int* ktile, int* kstep) {
    if (!rows || !cols || !ktile || !kstep) return FZ_ERR_ARG;
    *rows = H16_BM; *cols = H16_BN; *ktile = H16_BK; *kstep = H16_KS;
    return FZ_OK;
}

extern "C" int fz_splade_head_max_f16(const void* X16, int ldx, const void* W16, int ldw, const float* bias, const int32_t* cu_rows, int nseq, int T,
                                      int V, int d, float* pool, int ldp, void* stream) {
    if (T < 0 || V < 0 || nseq < 0 || d <= 0 || ldx < d || ldw < d || ldp < V) return FZ_ERR_ARG;
    if (T == 0 || V == 0 || nseq == 0) return FZ_OK;
    if (!X16 || !W16 || !bias || !cu_rows || !pool) return FZ_ERR_ARG;
    if ((d % 8) || (ldx % 8) || (ldw % 8) || ((uintptr_t)X16 % 16) || ((uintptr_t)W16 % 16)) return FZ_ERR_UNSUPPORTED;
    // per-lane offsets are signed 32-bit element offsets inside one 128-row operand tile
    if (128.0 * ldx * 2 >= 2147483648.0 || 128.0 * ldw * 2 >= 2147483648.0) return FZ_ERR_UNSUPPORTED;
    Head16Args g{};
    g.X = reinterpret_cast<const _Float16*>(X16); g.ldx = ldx; g.W = reinterpret_cast<const _Float16*>(W16); g.ldw = ldw;
    g.bias = bias; g.cu_rows = cu_rows; g.nseq = nseq; g.T = T; g.V = V; g.d = d; g.pool = pool; g.ldp = ldp;
    g.QB = (T + H16_BM - 1) / H16_BM;
    g.TN = (V + H16_BN - 1) / H16_BN;
    const long ids = 8L * ((g.TN + 7) / 8) * g.QB;
    if (ids > 0x3fffffffL) return FZ_ERR_UNSUPPORTED;
    g.ids = (int)ids;

    static int cus[64];
    int dev = 0;
    FZ_HIP_TRY(hipGetDevice(&dev));
    if (dev >= 64) return FZ_ERR_UNSUPPORTED;
    if (!cus[dev]) FZ_HIP_TRY(hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev));
    const long slots = 2L * cus[dev] / 8 * 8;            // resident workgroups (two per CU), a multiple of the 8 XCDs
    if (slots <= 0) return FZ_ERR_UNSUPPORTED;
    const unsigned grid = (unsigned)std::min(ids, slots);
    constexpr size_t lds_db = 2 * H16_BUF * sizeof(_Float16);
    static unsigned long long lds_set[2] = {0ull, 0ull};
    hipStream_t st = as_stream(stream);
    if (d % H16_BK) {
        if (int rc = raise_lds_limit((const void*)splade_head_f16_kernel<true>, lds_db, lds_set[1])) return rc;
        splade_head_f16_kernel<true><<<grid, 256, lds_db, st>>>(g);
    } else {
        if (int rc = raise_lds_limit((const void*)splade_head_f16_kernel<false>, lds_db, lds_set[0])) return rc;
        splade_head_f16_kernel<false><<<grid, 256, lds_db, st>>>(g);
    }
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
