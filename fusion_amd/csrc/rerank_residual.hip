// rerank_residual.hip -- K2c: the residual-compressed ColBERT token index (include/fusion_hip.h, 'Residual-compressed token rows').
//
// A token row is stored as the id of its nearest centroid (codes [sumL] int32, ops.centroid_assign) and, per dimension, the nbits-wide
// number of the bucket its residual falls in (packed [sumL][16 nbits] uint8).  Decompression is a fixed function of the stored bytes:
//     D[t][j] = float16(C[code[t]][j] + weights[bucket[t][j]])          one IEEE half add, round to nearest even, denormals kept
// and the score of a candidate is EXACTLY fz_maxsim_pairs_f16's over D -- the same MFMA mapping, fmaxf from -inf and summation tree,
// the same -inf / 0 / clamped-length / last-row-clamp rules -- so a compressed shard, the explicitly decompressed matrix and the
// all-pairs plane of that matrix are interchangeable bit for bit.
//
// Storage is fragment-major: storage position s in 0..127 holds dimension 32 ((s >> 3) & 3) + 8 (s >> 5) + (s & 7), positions fill
// ascending bytes and, inside a byte, ascending bit fields.  Lane (row l & 15, group g = l >> 4) of the 16x16x32_f16 A operand needs
// dimensions 32 ks + 8 g + j (ks < 4, j < 8) = positions 32 g + 8 ks + j: ONE aligned piece of the row, 8 bytes at offset 8 g for
// nbits = 2, 16 bytes at offset 16 g for nbits = 4.
//
// fz_maxsim_pairs_residual_f16 is the slot walk of maxsim_pairs.h, the one rerank.hip runs (workgroup = query x 128 slots, B fragments
// resident, one lane resolves one slot per wave, scalar control, no barrier), with another way of filling the A fragments.  Per row
// block a lane loads its row's code, then the four 16-byte centroid fragments the code points at and its residual piece, and decompresses IN PLACE into the fragment registers: the piece's bytes index a table of packed
// half weights (nbits = 2: a byte = 4 positions = 4 halves, ds_read_b64; nbits = 4: a byte = 2 positions = 2 halves, ds_read_b32; 256
// entries, one copy per wave, filled once by the wave that reads it) and v_pk_add_f16 adds them.  The code is clamped into [0, K - 1]
// (v_med3_i32), so no address leaves the table whatever the stored bytes are.  The codes of all row blocks of a round are issued before
// the first fragment load (the fragment is a dependent read).  Lq = 128 keeps 2 row blocks in flight instead of 4: the maximum does not
// depend on the grouping of the row blocks.
#include "maxsim_pairs.h"

namespace fz {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int RR_THREADS = 256;              // the two streaming kernels

// dimension of the first of the 8 storage positions of group G = s >> 3 (they hold 8 consecutive dimensions)
__host__ __device__ constexpr int group_dim(int G) { return 32 * (G & 3) + 8 * (G >> 2); }

// the code clamped into [0, K - 1] (K >= 1, wave-uniform): one v_med3_i32 (hipcc writes min(max()) as two instructions)
__device__ __forceinline__ int clamp_code(int c, int K) {
    int r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(c), "s"(K - 1));
    return r;
}

// ---- compress: one thread per 32-bit word of a packed row (16 positions at nbits = 2, 8 at nbits = 4) --------------------------------
template <int NBITS>
__global__ __launch_bounds__(RR_THREADS)
void residual_compress_kernel(const _Float16* __restrict__ tok, const int32_t* __restrict__ codes, const _Float16* __restrict__ C,
                              const float* __restrict__ cutoffs, int64_t n, int K, uint32_t* __restrict__ packed) {
    constexpr int WPR = 4 * NBITS;         // words per row
    constexpr int GPW = 4 / NBITS;         // groups of 8 positions per word
    const int64_t idx = (int64_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (idx >= n * WPR) return;
    const int64_t t = idx / WPR;
    const int word = (int)(idx % WPR);
    const _Float16* const crow = C + (size_t)clamp_code(codes[t], K) * MP_DIM;
    const _Float16* const trow = tok + (size_t)t * MP_DIM;
    uint32_t bits = 0;
#pragma unroll
    for (int gi = 0; gi < GPW; ++gi) {
        const int d0 = group_dim(word * GPW + gi);
        const f16x8 x = *reinterpret_cast<const f16x8*>(trow + d0);
        const f16x8 c = *reinterpret_cast<const f16x8*>(crow + d0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float r = (float)x[j] - (float)c[j];
            uint32_t b = 0;
#pragma unroll
            for (int i = 0; i < (1 << NBITS) - 1; ++i) b += r > cutoffs[i] ? 1u : 0u;   // a NaN residual: bucket 0
            bits |= b << (NBITS * (8 * gi + j));
        }
    }
    packed[idx] = bits;
}

// ---- decompress rows [row_lo, row_hi): one thread per group of 8 positions (16 bytes of output) --------------------------------------
template <int NBITS>
__global__ __launch_bounds__(RR_THREADS)
void residual_decompress_kernel(const uint8_t* __restrict__ packed, const int32_t* __restrict__ codes, const _Float16* __restrict__ C,
                                const _Float16* __restrict__ weights, int64_t row_lo, int64_t rows, int K, _Float16* __restrict__ out) {
    __shared__ _Float16 sw[1 << NBITS];
    if (threadIdx.x < (1 << NBITS)) sw[threadIdx.x] = weights[threadIdx.x];
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (idx >= rows * 16) return;
    const int64_t t = row_lo + idx / 16;
    const int G = (int)(idx % 16);
    const int d0 = group_dim(G);
    const f16x8 c = *reinterpret_cast<const f16x8*>(C + (size_t)clamp_code(codes[t], K) * MP_DIM + d0);
    const uint8_t* const p = packed + (size_t)t * (16 * NBITS) + G * NBITS;
    uint32_t bits;
    if constexpr (NBITS == 2) bits = *reinterpret_cast<const uint16_t*>(p);
    else bits = *reinterpret_cast<const uint32_t*>(p);
    f16x8 d;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = c[j] + sw[(bits >> (NBITS * j)) & ((1u << NBITS) - 1)];
    *reinterpret_cast<f16x8*>(out + (size_t)(idx / 16) * MP_DIM + d0) = d;
}

// ---- the rerank over compressed rows: maxsim_pairs.h's walk, the rows decompressed on their way into the A operands -----------------
template <int NBITS> struct Piece;
template <> struct Piece<2> { typedef uint2 reg; typedef uint2 entry; };   // 8 bytes of a row; a byte's four half weights
template <> struct Piece<4> { typedef uint4 reg; typedef uint32_t entry; };  // 16 bytes of a row; a byte's two half weights

__device__ __forceinline__ uint32_t pack_halves(_Float16 lo, _Float16 hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, lo) | ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
}

// c (8 halves: dimensions 32 ks + 8 g .. + 7 of the centroid) += the weights the piece's bytes for k-step ks name
__device__ __forceinline__ void add_weights(f16x8& c, const uint2* tab, const uint2 piece, int ks) {
    const uint32_t w = ks < 2 ? piece.x : piece.y;             // bytes 2 ks, 2 ks + 1: positions 8 ks .. 8 ks + 7
    const uint2 lo = tab[(w >> (16 * (ks & 1))) & 0xffu], hi = tab[(w >> (16 * (ks & 1) + 8)) & 0xffu];
    const f16x4 a = __builtin_shufflevector(c, c, 0, 1, 2, 3) + __builtin_bit_cast(f16x4, lo);
    const f16x4 b = __builtin_shufflevector(c, c, 4, 5, 6, 7) + __builtin_bit_cast(f16x4, hi);
    c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ void add_weights(f16x8& c, const uint32_t* tab, const uint4 piece, int ks) {
    const uint32_t w = ks == 0 ? piece.x : ks == 1 ? piece.y : ks == 2 ? piece.z : piece.w;   // bytes 4 ks .. 4 ks + 3
    const f16x2 w0 = __builtin_bit_cast(f16x2, tab[w & 0xffu]), w1 = __builtin_bit_cast(f16x2, tab[(w >> 8) & 0xffu]);
    const f16x2 w2 = __builtin_bit_cast(f16x2, tab[(w >> 16) & 0xffu]), w3 = __builtin_bit_cast(f16x2, tab[w >> 24]);
    const f16x4 a = __builtin_shufflevector(c, c, 0, 1, 2, 3) + __builtin_shufflevector(w0, w1, 0, 1, 2, 3);
    const f16x4 b = __builtin_shufflevector(c, c, 4, 5, 6, 7) + __builtin_shufflevector(w2, w3, 0, 1, 2, 3);
    c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

struct ResidualStore {
    const uint8_t* packed;    // [sumL][16 nbits]
    const int32_t* codes;     // [sumL]
    const _Float16* C;        // [K][128]
    const _Float16* weights;  // [2^nbits]
    int K;
};

template <int NBITS>
struct ResidualRows : ResidualStore {
    typedef typename Piece<NBITS>::reg piece_t;
    typedef typename Piece<NBITS>::entry entry_t;
    static constexpr int ROW_BYTES = 16 * NBITS, PIECE_BYTES = 4 * NBITS;
    struct Doc {
        const int32_t* code;   // the document's codes
        const uint8_t* res;    // this lane's piece of the document's first row
        const _Float16* cbase; // this lane's 8 dimensions of centroid 0
        const entry_t* tab;    // this wave's weight table
    };

    entry_t (*wtab)[256];     // [MP_WAVES][256] in LDS

    // this wave's weight table: entry e = the packed half weights of the 8 / nbits positions byte e holds, ascending bit fields.
    // Written and read by the same wave only: DS operations of a wave complete in order, so no barrier is needed
    __device__ __forceinline__ void prologue(int w, int lane) const {
        entry_t* const tab = wtab[w];
#pragma unroll
        for (int e = lane; e < 256; e += 64) {
            if constexpr (NBITS == 2) {
                tab[e] = make_uint2(pack_halves(weights[e & 3], weights[(e >> 2) & 3]), pack_halves(weights[(e >> 4) & 3], weights[e >> 6]));
            } else {
                tab[e] = pack_halves(weights[e & 15], weights[e >> 4]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __device__ __forceinline__ Doc doc(int64_t t0, int w, int lane) const {
        const int g = lane >> 4;
        return Doc{codes + t0, packed + (size_t)t0 * ROW_BYTES + PIECE_BYTES * g, C + 8 * g, wtab[w]};
    }
    template <int NB>
    __device__ __forceinline__ void load(const Doc& d, int c0, int last, int lane, f16x8 (&af)[NB][4]) const {
        int code[NB];
        piece_t piece[NB];
#pragma unroll
        for (int rb = 0; rb < NB; ++rb) {   // the codes of the whole round first: the fragment loads depend on them
            int row = c0 + 16 * rb + (lane & 15);
            row = row < last ? row : last;   // the last partial row block re-reads the last token: the maximum is unchanged
            code[rb] = d.code[row];
            piece[rb] = *reinterpret_cast<const piece_t*>(d.res + (size_t)row * ROW_BYTES);
        }
#pragma unroll
        for (int rb = 0; rb < NB; ++rb) {
            const _Float16* p = d.cbase + (size_t)clamp_code(code[rb], K) * MP_DIM;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) af[rb][ks] = *reinterpret_cast<const f16x8*>(p + 32 * ks);
        }
#pragma unroll
        for (int rb = 0; rb < NB; ++rb)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) add_weights(af[rb][ks], d.tab, piece[rb], ks);   // decompressed in place
    }
};

struct ResidualPairsArgs {
    PairSlots s;
    ResidualStore rows;
};

// NCB = Lq / 16 column blocks of 16 query tokens; Lq = 128 keeps 2 row blocks in flight instead of 4.
template <int NCB, int NBITS>
__global__ __launch_bounds__(MP_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2)))
void maxsim_residual_kernel(ResidualPairsArgs a) {
    __shared__ typename Piece<NBITS>::entry wtab[MP_WAVES][256];
    maxsim_pairs_walk<NCB, NCB == 8 ? 2 : 4>(a.s, ResidualRows<NBITS>{a.rows, wtab});
}

template <int NBITS>
static void launch_pairs(int Lq, unsigned nblk, hipStream_t st, const ResidualPairsArgs& a) {
    if (Lq == 32) maxsim_residual_kernel<2, NBITS><<<nblk, MP_WAVES * 64, 0, st>>>(a);
    else if (Lq == 64) maxsim_residual_kernel<4, NBITS><<<nblk, MP_WAVES * 64, 0, st>>>(a);
    else maxsim_residual_kernel<8, NBITS><<<nblk, MP_WAVES * 64, 0, st>>>(a);
}

}  // namespace fz

using namespace fz;

extern "C" int fz_residual_compress_f16(const void* tok, const int32_t* codes, const void* C, const float* cutoffs, int64_t n, int K, int dim,
                                        int nbits, void* packed, void* stream) {
    if (n < 0 || K < 1) return FZ_ERR_ARG;
    if (n != 0 && (!tok || !codes || !C || !cutoffs || !packed)) return FZ_ERR_ARG;
    if (dim != MP_DIM) return FZ_ERR_UNSUPPORTED;
    if (nbits != 2 && nbits != 4) return FZ_ERR_UNSUPPORTED;
    if (((uintptr_t)tok % 16) || ((uintptr_t)C % 16) || ((uintptr_t)packed % 16)) return FZ_ERR_UNSUPPORTED;
    if (n == 0) return FZ_OK;
    const int64_t nblk = (n * (4 * nbits) + RR_THREADS - 1) / RR_THREADS;
    if (nblk > 0x7fffffffLL) return FZ_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const _Float16* t = reinterpret_cast<const _Float16*>(tok);
    const _Float16* c = reinterpret_cast<const _Float16*>(C);
    if (nbits == 2) residual_compress_kernel<2><<<(unsigned)nblk, RR_THREADS, 0, st>>>(t, codes, c, cutoffs, n, K, reinterpret_cast<uint32_t*>(packed));
    else residual_compress_kernel<4><<<(unsigned)nblk, RR_THREADS, 0, st>>>(t, codes, c, cutoffs, n, K, reinterpret_cast<uint32_t*>(packed));
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_residual_decompress_f16(const void* packed, const int32_t* codes, const void* C, const void* weights, int64_t sumL,
                                          int64_t row_lo, int64_t row_hi, int K, int dim, int nbits, void* out, void* stream) {
    if (sumL < 0 || K < 1 || row_lo < 0 || row_hi < row_lo || row_hi > sumL) return FZ_ERR_ARG;
    if (row_hi != row_lo && (!packed || !codes || !C || !weights || !out)) return FZ_ERR_ARG;
    if (dim != MP_DIM) return FZ_ERR_UNSUPPORTED;
    if (nbits != 2 && nbits != 4) return FZ_ERR_UNSUPPORTED;
    if (((uintptr_t)packed % 16) || ((uintptr_t)C % 16) || ((uintptr_t)out % 16)) return FZ_ERR_UNSUPPORTED;
    if (row_hi == row_lo) return FZ_OK;
    const int64_t rows = row_hi - row_lo;
    const int64_t nblk = (rows * 16 + RR_THREADS - 1) / RR_THREADS;
    if (nblk > 0x7fffffffLL) return FZ_ERR_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const uint8_t* p = reinterpret_cast<const uint8_t*>(packed);
    const _Float16* c = reinterpret_cast<const _Float16*>(C);
    const _Float16* wt = reinterpret_cast<const _Float16*>(weights);
    _Float16* o = reinterpret_cast<_Float16*>(out);
    if (nbits == 2) residual_decompress_kernel<2><<<(unsigned)nblk, RR_THREADS, 0, st>>>(p, codes, c, wt, row_lo, rows, K, o);
    else residual_decompress_kernel<4><<<(unsigned)nblk, RR_THREADS, 0, st>>>(p, codes, c, wt, row_lo, rows, K, o);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_maxsim_pairs_residual_f16(const void* Qtok, const void* packed, const int32_t* codes, const void* C, const void* weights,
                                            int K, int nbits, const int64_t* Doff, int64_t sumL, int max_doc_len, int Q, int Lq, int N,
                                            int dim, const int64_t* cand, int ldc, const int32_t* cand_len, int k, int64_t id_base,
                                            float* scores, int lds, void* stream) {
    ResidualPairsArgs a{};
    const int rc = pair_slots_args(a.s,
                                   K < 1 || ((Q != 0 && k != 0) && (!C || !weights)) ||
                                       ((!packed || !codes) && sumL != 0),   // an empty shard (every document empty) has no rows to point at
                                   (nbits != 2 && nbits != 4) || ((uintptr_t)packed % 16) || ((uintptr_t)C % 16), Qtok, Doff, sumL, max_doc_len, Q,
                                   Lq, N, dim, cand, ldc, cand_len, k, id_base, scores, lds);
    if (rc != FZ_OK || Q == 0 || k == 0) return rc;
    a.rows = {reinterpret_cast<const uint8_t*>(packed), codes, reinterpret_cast<const _Float16*>(C), reinterpret_cast<const _Float16*>(weights), K};
    const unsigned nblk = (unsigned)Q * a.s.nslices;
    hipStream_t st = as_stream(stream);
    if (nbits == 2) launch_pairs<2>(Lq, nblk, st, a);
    else launch_pairs<4>(Lq, nblk, st, a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
