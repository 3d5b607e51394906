// pairs.hip -- single-vector scores of every query against ITS OWN candidate list (DPR / SPLADE at corpus scale: list completion).
//
//   fz_dot_pairs_f32          out[q][r] = <Qn[q], Dn[cand[q][r] - id_base]>, the bits of fz_dot_scores_f32's plane entry
//   fz_sparse_dot_pairs_f32   out[q][r] = what sparse.hip's walk gives document cand[q][r] - id_base, the bits of fz_sparse_dot_f32's
//
// Slots: r >= cand_len[q], id < 0 or position outside [0, N) -> -inf (a shard scores what it owns), as in rerank.hip.
//
// Dense.  score.hip's gemm_stream accumulates a score as ONE chain of fused multiply-adds from +0.0: k-tiles of 32 in ascending order, the
// count rounded up to even, inside a k-tile four groups of 8 in the order 0, 4, 1, 5, 2, 6, 3, 7 (lanes 0-31 of a 32x32x2 hold k, lanes
// 32-63 k + 4), k's past d as exact zeros (fma(0, 0, acc): the identity but for acc = -0.0, so the padded steps are made here too).  The
// chain is restated the way the straggler slabs restate it, on v_mfma_f32_4x4x1_16b_f32: the query's k-th value in the A operand of all
// 16 blocks, 64 candidate rows in the B lanes, one instruction = one k of 64 pairs; D register 0 of lane l is pair l's score.
//
// The workload is a gather (Q = 1024, W = 3,000, d = 768: 9.4 GB of rows against 5 GFLOP), so the shape is about loads:
//   * a workgroup = 4 waves = (query, block of 256 candidate slots); thread i resolves slot i once (id -> row, bounds);
//   * a k-tile of the block -- 256 rows x 128 B -- is fetched as 2,048 16-byte pieces, 8 per thread, 8 neighbouring lanes on the 8
//     pieces of one row (a whole 128-byte line per row and k-tile), all issued before anything waits: 32 KiB in flight per workgroup,
//     four workgroups per CU;
//   * registers -> LDS (rows padded to 36 floats: ds_read_b128 of consecutive rows is bank-conflict-free, as in score.hip), read back
//     as "lane = candidate"; the next k-tile's loads are issued before the MFMAs of this one;
//   * the query's vector sits in LDS for the whole workgroup, zero-padded to the k-tile count, and is read as a broadcast.
// An absent slot loads row 0 (cached) and stores -inf: no load is predicated.  No atomics, no workspace, no host synchronisation.
//
// Sparse.  One thread = one (query, slot): a binary search per query term (ascending term order) in the term's postings and the walk's
// `acc = acc + w * pw` from +0.0 -- one rounding per product and per add (-ffp-contract=off), terms that do not hold the document skipped.
// lexical_doc_scores_kernel (bm25_count.hip) in float32 with the weight.
//
// Where it stands: DESIGN.md section 'Pair scores and list completion'.
#include "pairs.h"
#include "slices.h"

namespace fz {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DP_THREADS = 256;
constexpr int DP_SLOTS = 256;                    // candidate slots per workgroup: one per thread
constexpr int DP_BK = 32, DP_LDT = DP_BK + 4;    // k-tile, LDS row (36 floats = 144 B)
constexpr int DP_RPT = DP_SLOTS * (DP_BK / 4) / DP_THREADS;   // 16-byte pieces per thread and k-tile: 8
constexpr int DP_MAX_D = 16384;                  // the query's vector must fit LDS next to the tile (36 + 64 KiB)

struct DotPairsArgs {
    const float* Qn; const float* Dn;     // [Q][ldq], [N][ldd]
    const int64_t* cand;                  // [Q][ldc]
    const int32_t* cand_len;              // [Q] or null
    float* out;                           // [Q][ldo]
    int64_t id_base;
    int ldq, ldd, ldc, ldo, Q, N, d, W;
    int nblocks;                          // ceil(W / DP_SLOTS)
    int KT;                               // k-tiles: ceil(d / 64) * 2
};

__global__ __launch_bounds__(DP_THREADS) void dot_pairs_kernel(DotPairsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [DP_SLOTS][DP_LDT] the k-tile | [KT * DP_BK] the query
    float* const qs = lds + DP_SLOTS * DP_LDT;
    int* const s_pos = reinterpret_cast<int*>(lds);               // the slots' rows, until the first k-tile lands
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = blockIdx.x / a.nblocks;
    const int slot = (blockIdx.x % a.nblocks) * DP_SLOTS + tid;

    const int pos = slot < a.W ? pair_position(a.cand, a.ldc, a.cand_len, a.id_base, a.N, a.W, q, slot) : -1;
    s_pos[tid] = pos;
    {
        const float* qv = a.Qn + (size_t)q * a.ldq;
        for (int k = tid * 4; k < a.KT * DP_BK; k += DP_THREADS * 4)   // d % 4 == 0: a float4 is inside or outside
            *reinterpret_cast<float4*>(qs + k) = k < a.d ? *reinterpret_cast<const float4*>(qv + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();

    // staging: thread -> (row = tid / 8 + 32 i, piece = tid % 8)
    const int srow = tid >> 3, sk = (tid & 7) * 4;
    const float* rp[DP_RPT];
#pragma unroll
    for (int i = 0; i < DP_RPT; ++i) {
        const int p = s_pos[srow + 32 * i];
        rp[i] = a.Dn + (size_t)(p < 0 ? 0 : p) * a.ldd + sk;      // an absent slot reads row 0 (N >= 1 here) and stores -inf
    }
    __syncthreads();                                               // s_pos is the tile from here on

    float4 st[DP_RPT];
    // a piece past d re-reads the row's first float4 and is zeroed on its way into LDS: no load is predicated
    auto gload = [&](int kt) __attribute__((always_inline)) {
        const int off = kt * DP_BK + sk < a.d ? kt * DP_BK : -sk;
#pragma unroll
        for (int i = 0; i < DP_RPT; ++i) st[i] = *reinterpret_cast<const float4*>(rp[i] + off);
    };
    auto sstore = [&](int kt) __attribute__((always_inline)) {
        const bool in = kt * DP_BK + sk < a.d;
#pragma unroll
        for (int i = 0; i < DP_RPT; ++i)
            *reinterpret_cast<float4*>(lds + (srow + 32 * i) * DP_LDT + sk) = in ? st[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    };

    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* const mine = lds + (w * 64 + lane) * DP_LDT;      // lane = candidate: its row of the tile
    gload(0);
    for (int kt = 0; kt < a.KT; ++kt) {
        sstore(kt);
        __syncthreads();
        if (kt + 1 < a.KT) gload(kt + 1);                          // (workgroup-uniform) in flight under this k-tile's MFMAs
        const float* const qk = qs + kt * DP_BK;
#pragma unroll
        for (int kg = 0; kg < DP_BK / 8; ++kg) {
            const float4 b0 = *reinterpret_cast<const float4*>(mine + kg * 8), b1 = *reinterpret_cast<const float4*>(mine + kg * 8 + 4);
            const float4 a0 = *reinterpret_cast<const float4*>(qk + kg * 8), a1 = *reinterpret_cast<const float4*>(qk + kg * 8 + 4);
            // the tile stream's k order inside a group of 8: k, then k + 4
            acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.x, b0.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.x, b1.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.y, b0.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.y, b1.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.z, b0.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.z, b1.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.w, b0.w, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.w, b1.w, acc, 0, 0, 0);
        }
        // The accumulator is read behind the loop's exit branch, where hipcc has been seen to leave an MFMA's reader too close
        // (tools/check_mfma_hazards.py): a full-length wait in the block of the last MFMA, 20 of a k-tile's several thousand cycles
        // (behind the loop the register allocator still puts its copy out of the accumulator registers in front of the wait).
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3");
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                           // every wave has read the tile: the next one may land
    }
    // C/D of the 4x4x1: register v = row v of the block, lane = 4 * block + column; every row carries the query
    if (slot < a.W) a.out[(size_t)q * a.ldo + slot] = pos < 0 ? -INFINITY : acc[0];
}

// a shard of no documents owns no slot
__global__ __launch_bounds__(256) void pairs_absent_kernel(float* out, int ldo, int W, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) out[(size_t)(i / W) * ldo + (i % W)] = -INFINITY;
}

struct SparsePairsArgs {
    const int64_t* toff; const int32_t* pdoc; const float* pw;     // index: postings of term t are [toff[t], toff[t+1]), documents ascending
    const int64_t* qoff; const int32_t* qterms; const float* qw;   // queries: non-zero terms of query q are [qoff[q], qoff[q+1]), ascending
    const int64_t* cand; const int32_t* cand_len;
    float* out;
    int64_t id_base;
    int ldc, ldo, Q, N, W, nblocks;
};

// one thread per (query, slot)
__global__ __launch_bounds__(256) void sparse_dot_pairs_kernel(SparsePairsArgs a) {
    const int q = blockIdx.x / a.nblocks;
    const int slot = (blockIdx.x % a.nblocks) * 256 + threadIdx.x;
    if (slot >= a.W) return;
    const int d = pair_position(a.cand, a.ldc, a.cand_len, a.id_base, a.N, a.W, q, slot);
    float* const dst = a.out + (size_t)q * a.ldo + slot;
    if (d < 0) { *dst = -INFINITY; return; }
    float acc = 0.0f;
    const int64_t p0 = a.qoff[q], p1 = a.qoff[q + 1];
    for (int64_t p = p0; p < p1; ++p) {        // terms in ascending vocabulary order: the walk's addition order
        const int t = a.qterms[p];
        const int64_t end = a.toff[t + 1];
        const int64_t e = lower_bound_doc(a.pdoc, a.toff[t], end, d);
        if (e < end && a.pdoc[e] == d) acc = acc + a.qw[p] * a.pw[e];
    }
    *dst = acc;
}

}  // namespace fz

using namespace fz;

extern "C" int fz_dot_pairs_f32(const float* Qn, int ldq, const float* Dn, int ldd, int Q, int N, int d, const int64_t* cand, int ldc,
                                const int32_t* cand_len, int W, int64_t id_base, float* out, int ldo, void* stream) {
    if (Q < 0 || N < 0 || W < 0 || d <= 0 || ldq < d || ldd < d || ldc < W || ldo < W) return FZ_ERR_ARG;
    if ((Q != 0 && W != 0) && (!Qn || !cand || !out)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if ((Q != 0 && W != 0 && N != 0) && !Dn) return FZ_ERR_ARG;
    if ((d % 4) || (ldq % 4) || (ldd % 4) || d > DP_MAX_D) return FZ_ERR_UNSUPPORTED;
    if (((uintptr_t)Qn % 16) || ((uintptr_t)Dn % 16)) return FZ_ERR_UNSUPPORTED;
    if (Q == 0 || W == 0) return FZ_OK;
    hipStream_t st = as_stream(stream);
    if (N == 0) {
        const long total = (long)Q * W;
        pairs_absent_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(out, ldo, W, total);
        FZ_LAUNCH_CHECK();
        return FZ_OK;
    }
    DotPairsArgs a{};
    a.Qn = Qn; a.Dn = Dn; a.cand = cand; a.cand_len = cand_len; a.out = out; a.id_base = id_base;
    a.ldq = ldq; a.ldd = ldd; a.ldc = ldc; a.ldo = ldo; a.Q = Q; a.N = N; a.d = d; a.W = W;
    a.nblocks = (W + DP_SLOTS - 1) / DP_SLOTS;
    a.KT = ((d + 2 * DP_BK - 1) / (2 * DP_BK)) * 2;
    const long nblk = (long)Q * a.nblocks;
    if (nblk > 0x7fffffffL) return FZ_ERR_UNSUPPORTED;
    constexpr size_t lds_max = ((size_t)DP_SLOTS * DP_LDT + DP_MAX_D) * sizeof(float);
    static unsigned long long lds_set = 0ull;
    if (int rc = raise_lds_limit((const void*)dot_pairs_kernel, lds_max, lds_set)) return rc;
    const size_t lds_bytes = ((size_t)DP_SLOTS * DP_LDT + (size_t)a.KT * DP_BK) * sizeof(float);
    dot_pairs_kernel<<<(unsigned)nblk, DP_THREADS, lds_bytes, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_sparse_dot_pairs_f32(const int64_t* toff, const int32_t* pdoc, const float* pw, const int64_t* qoff, const int32_t* qterms,
                                       const float* qw, int Q, int N, const int64_t* cand, int ldc, const int32_t* cand_len, int W,
                                       int64_t id_base, float* out, int ldo, void* stream) {
    if (Q < 0 || N < 0 || W < 0 || ldc < W || ldo < W) return FZ_ERR_ARG;
    if ((Q != 0 && W != 0) && (!qoff || !cand || !out)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if ((Q != 0 && W != 0 && N != 0) && !toff) return FZ_ERR_ARG;
    if (Q == 0 || W == 0) return FZ_OK;
    SparsePairsArgs a{};
    a.toff = toff; a.pdoc = pdoc; a.pw = pw; a.qoff = qoff; a.qterms = qterms; a.qw = qw; a.cand = cand; a.cand_len = cand_len; a.out = out;
    a.id_base = id_base; a.ldc = ldc; a.ldo = ldo; a.Q = Q; a.N = N; a.W = W;
    a.nblocks = (W + 255) / 256;
    const long nblk = (long)Q * a.nblocks;
    if (nblk > 0x7fffffffL) return FZ_ERR_UNSUPPORTED;
    sparse_dot_pairs_kernel<<<(unsigned)nblk, 256, 0, as_stream(stream)>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
