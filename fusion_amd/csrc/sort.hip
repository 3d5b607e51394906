// sort.hip -- stable descending row sort (K5a/K6) for gfx950.  (Top-k over it: topk.hip.)
//
// Reference semantics: Python sorted(items, key=score, reverse=True) is stable
// (bm25.py:104, hybrid.py:306).
//
// Design (MI355X-first): one workgroup owns one row.  A row (<= 35,840 keys) lives entirely in
// the workgroup's registers (E keys per thread, "wave-striped": wave w, item i, lane l holds
// sequence position w*E*64 + i*64 + l), so HBM sees each key once in and once out.  fp32 keys
// take 4 LSD passes; fp64 keys take 4 passes over their HIGH word plus an in-place repair of the
// (short, adjacent) runs of equal high words -- the same permutation as 8 passes.  Each LSD pass
// over an 8-bit digit is
//   1. rank:     per item, the 64 lanes of a wave find their same-digit peers with 8 ballots
//                (wave64 match-any), and bump a wave-private LDS counter (no atomics, stable);
//   2. scan:     256 digits x NW waves counters -> exclusive prefix (digit-major);
//   3. exchange: scatter keys (then the 16-bit payload) through a T*E*4-byte LDS buffer
//                and read them back in striped order.
// Passes whose digit is constant over the row are skipped.  LDS: up to 156 KiB of the CU's
// 160 KiB, i.e. one 1024-thread workgroup per CU.
//
// Round 4: fp32 rows of 8,193 .. 28,672 columns (a 1,024-thread workgroup's rows) with at least 4,096 keys in them that look like a ranker's scores (few ties) skip the digit passes: BUCKET RANKING --
// a counting sort over 16,384 buckets whose widths follow the row's own density, every key's rank = its bucket's first slot + the
// bucket members below it, one neighbour check on the result (see `bucket_rank` in the kernel).  239 instead of 282 vector
// instructions per key and 42 % fewer LDS bank-conflict cycles (profiles/r04_pmc_sort_{bucket,digits}.json): 0.32 instead of 0.37 ms
// per 1024 x 27,942 cosine scores.  Rows it does not suit are found out early and take the digit passes; same permutation either way.
#include <type_traits>

#include "sort.h"

namespace fz {

// rows the bucket ranking ordered | of those, rows whose neighbour check swapped a pair back | rows it gave up on after starting
// (ties, a crowd at the floor, an overfull bucket, a check it could not settle).  Read by fz_sort_bucket_rank_rows (tests, tools).
__device__ unsigned long long g_bucket_rank_rows[3];
// rows whose zeros were compacted away | rows that were looked at and kept whole (too few zeros).  Read by fz_sort_zero_compact_rows.
__device__ unsigned long long g_zero_compact_rows[2];

// Bucket ranking (see sort_rows_kernel): fine / coarse bucket counts and the words of LDS its tables take in the counter area.
constexpr int BR_FINE = 16384, BR_COARSE = 1024, BR_WORDS = BR_FINE / 2 + BR_COARSE + 1024;   // + one bit per slot (bucket starts)
constexpr int BR_MIN_KEYS = 4096, BR_MAX_BUCKET = 128;
constexpr int BR_STRAIGHT = 6;                       // bucket members the rank phase reads without a loop (8: 1 % slower, 4: 3 %)
template <int T, int E, int KW> struct SortLds {
    static constexpr bool br = T == 1024 && KW == 1 && (size_t)(32 + T * E + BR_WORDS) * 4 <= 160 * 1024;
    static constexpr size_t area = (size_t)(T / 64) * 256 * 4 + (KW == 2 ? (size_t)T * E : 0);   // counters (+ fp64: one move byte per slot)
    static constexpr size_t bytes = (size_t)(32 + T * E) * 4 + (br && area < (size_t)BR_WORDS * 4 ? (size_t)BR_WORDS * 4 : area);
};

// 1.0 / x in float64 for an integer-valued x in [1, 2^20]: the division's own Newton-Raphson steps (LLVM lowers an f64 division to
// v_div_scale x2, v_rcp_f64, five v_fma_f64, v_mul_f64, v_div_fmas, v_div_fixup; with a numerator of 1.0 and a denominator that needs no
// scaling the scale / fixup steps are identities and the multiplication is by 1.0) -- seven instructions instead of twelve, the same
// correctly rounded quotient: tests/test_gpu_rank_fused.py compares every x the sort can see (and 2^20 beyond) with the IEEE division.
__device__ __forceinline__ double recip_small_int_f64(double x) {
    double y = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-x, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-x, y, 1.0);       // the residual of the quotient (the numerator is 1.0: q = y)
    return __builtin_fma(e, y, y);
}
__global__ void rrf_terms_kernel(int count, int fast, double* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < count) out[r] = fast ? recip_small_int_f64((double)(60 + r + 1)) : 1.0 / (double)(60 + r + 1);
}

// FUSE: the fused scores of the rows the fast form flagged (practically never: > 2,048 keys sharing a high word), written out as a plain
// float64 row for the generic eight-pass launch -- whose FUSE instantiation (~500 B of scratch per lane) made even an EMPTY launch cost
// 40 us: above ROCr's per-queue scratch limit the dispatch allocates its scratch anew (283 MB of page zeroing per launch, rocprofv3).
// The arithmetic is fuse_rank_kernel's (IEEE division); every other row's workgroup exits at once.
__global__ __launch_bounds__(256) void fuse_flagged_rows_kernel(SortArgs a) {
    const int row = blockIdx.x;                      // one workgroup per row: rows + 1 wave launches to find out that nothing is flagged
    if (a.row_flags[row] == 0) return;
    for (int j = threadIdx.x; j < a.n_total; j += blockDim.x) {
        const size_t off = (size_t)row * a.key_row_stride + j;
        double acc = 0.0;
        bool present = false;
        for (int s = 0; s < a.fuse_S; ++s) {
            const int r = a.fuse_ranks[s][off];
            if (r >= 0) {
                const double n = (double)a.fuse_lens[(size_t)s * a.fuse_rows + row];
                acc = acc + (a.fuse_method == FZ_RRF ? 1.0 / (double)(60 + r + 1) : (n - (double)r + 1.0) / n);
                present = true;
            }
        }
        a.fuse_gen_plane[off] = present ? acc : -(double)INFINITY;
    }
}

// GEN (fp64 only): the generic eight-pass form, run as a second launch for the rows the fast form flags (see below).
// MODE: which of the kernel's many callers an instantiation serves -- what is not served is gone at compile time, and with it the row
// pointers and flags that otherwise stay live from the prologue to the output phase (they were the shipped hot kernels' spills):
//   SORT_ANY   every feature (chunked long rows, segmented top-k lists, column / id maps, id outputs);
//   SORT_ROWS  whole rows of one plane: the rankers' sorts and the final order (identity / gathered / placed sequence, statistics);
//   SORT_FUSE  SORT_ROWS whose float64 keys are formed from rank planes on load (fz_sort_rank_fused_desc), no statistics;
//   SORT_ROWS_ZC  SORT_ROWS for float64 rows the caller expects to be mostly exact zeros (a lexical ranker's scores:
//              fz_sort_rows_desc_lexical): the zeros stay out of the ordering phases (ZC below).  Its own instantiation because the
//              code that serves it costs a row WITHOUT zeros ~5 % (measured: one bit per key in the load phase, a scalar branch per
//              four items in every loop of the ordering phases, a handful of block-uniform branches) -- rows nobody expects zeros in
//              keep the SORT_ROWS kernel as it was.
enum { SORT_ANY = 0, SORT_ROWS = 1, SORT_FUSE = 2, SORT_ROWS_ZC = 3 };
template <int T, int E, int KW, bool GEN, int MODE = SORT_ANY>
__global__ __launch_bounds__(T) void sort_rows_kernel(SortArgs a) {
    constexpr bool FUSE = MODE == SORT_FUSE, LEAN = MODE != SORT_ANY;
    static_assert(!GEN || KW == 2, "the generic form exists for fp64 keys only");
    static_assert(!FUSE || KW == 2, "rank fusion forms float64 keys");
    static_assert(!(FUSE && GEN), "rows the fused fast form flags are sorted by the plain generic form from a materialised score row");
    constexpr int NW = T / 64;
    constexpr uint32_t SENT = 0xffffffffu;
    // ZC -- ZERO COMPACTION (round 6; float64 rows of one plane: BM25's ranking sort).  A lexical score row is mostly EXACT ZEROS (documents
    // that share no term with the query: ~60 % of the LLeQA-shaped bench rows), and a zero needs no sorting: its place in the list is
    // (keys above zero) + (zeros before it in sequence order).  When at least 3/8 of a row of >= 4,096 keys are +-0.0 the load phase's keys
    // are compacted -- the non-zero keys move, in sequence order, into a COMPACT striped layout of Ee = ceil(non-zeros / T) items per thread
    // (rounded up to 4) -- and the digit passes, the run detection, the low-word hand-over and the repair run over Ee items instead of E:
    // their cost is per item slot, whatever the slot holds.  The output phase puts sorted non-zero slot r at list position r (r < P = keys
    // above zero) or r + Z, and every zero at P + its index among the zeros; same stable permutation, bit for bit (a zero ties with nothing
    // but zeros, and those keep their order).  1024 x 27,942 BM25-like rows, 60 % zeros: 0.46 -> 0.2x ms (tools/bench_sort_zeros.py).
    constexpr bool ZC = KW == 2 && !GEN && MODE == SORT_ROWS_ZC && T == 1024 && E >= 16;
    [[maybe_unused]] int Ee = E;                  // items per thread in the ordering phases (ZC rows that were compacted; else E)
    // Loops over the items of the COMPACT layout stop at Ee (a multiple of 4: one scalar branch per four items; ~1 % on a row that kept its
    // zeros.  Instantiating the ordering phases once per path instead -- compacted / whole -- made hipcc spill 176 registers: measured, not kept).
#define ITEM_GUARD(i) if constexpr (ZC) { if ((((i) & 3) == 0) && (i) >= Ee) break; }
    constexpr int LG = (KW == 2) ? 7 : 14;         // global loads in flight per thread before the first use (one HBM latency per group)
    constexpr int LGF = FUSE ? 4 : LG;             // ... in the gathered / plain load phase (FUSE: the per-key sums need the registers)
    constexpr int WALK = 16;                        // longest equal-high-word run the fp64 repair re-sorts in place
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* misc = smem;                         // [32]
    uint32_t* exch = smem + 32;                    // [T*E]
    uint32_t* cnt = smem + 32 + T * E;             // [NW*256] (plain LDS pointer: volatile would lower to flat sc0 sc1 accesses); the bucket
                                                   //   ranking's tables (BR_WORDS words) start here too, over the fp64 move bytes behind it

    // LEAN serves whole rows only (the launcher sees to it): no chunks, segments, column / id maps -- known at compile time
    const int prow = blockIdx.x;
    const int row = LEAN ? prow : prow / a.chunks;
    const int chunk = LEAN ? 0 : prow - row * a.chunks;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int c0 = LEAN ? 0 : chunk * a.chunk_len;
    // this thread's first slot; SLOT_FRESH() makes it opaque again so that the 28 per-item slot numbers are re-derived (one add)
    // in every phase instead of being kept live -- 28 registers -- from the first phase to the last
    int slot0 = w * E * 64 + lane;
#define SLOT_FRESH() asm volatile("" : "+v"(slot0))
    if constexpr (GEN) { if (a.row_flags[prow] == 0) return; }                       // block-uniform: the fast form finished this row
    else if constexpr (KW == 2) { if (threadIdx.x == 0) a.row_flags[prow] = 0; }

    int m_row = a.row_len ? a.row_len[row] : a.n_total;
    m_row = m_row < 0 ? 0 : (m_row > a.n_total ? a.n_total : m_row);
    int m = m_row - c0;
    m = m < 0 ? 0 : (m > a.chunk_len ? a.chunk_len : m);
    const int m_all = m;          // (ZC: `m` becomes the number of non-zero keys for the ordering phases; the output phase works on the whole list)
    // statistics by-product (block-uniform): over the whole list from the load phase, or -- stats_len -- over the first slen entries
    // of the sorted list from the registers of the output phase
    const bool st_on = !FUSE && a.row_stats && (LEAN || a.chunks == 1);
    int slen = (st_on && a.stats_len) ? a.stats_len[row] : m;
    slen = slen < 0 ? 0 : (slen > m ? m : slen);
    const bool st_prefix = st_on && slen < m;
    const bool st_load = !GEN && st_on && !st_prefix;
    if (m == 0) {        // block-uniform: empty (pseudo-)row
        if (st_on && threadIdx.x == 0) {
            a.row_stats[row] = NAN; a.row_stats[a.stats_rows + row] = NAN;     // torch.mean / torch.std of an empty tensor
            a.row_stats[2 * a.stats_rows + row] = 0.f; a.row_stats[3 * a.stats_rows + row] = 0.f;
        }
        return;
    }

    // uniform row bases + 32-bit per-lane indices (saddr+voffset addressing; no 64-bit per-item addresses)
    const size_t krow = (size_t)row * a.key_row_stride;
    const bool seg = !LEAN && a.seg_len < a.n_total;  // block-uniform: segmented rows ([G][rows][k] top-k lists)
    const float* __restrict__ kf = reinterpret_cast<const float*>(a.keys) + krow;
    const uint2* __restrict__ kd = reinterpret_cast<const uint2*>(a.keys) + krow;   // a double as its (low, high) words
    const int32_t* __restrict__ init_row = a.init_order ? a.init_order + krow : nullptr;
    const int32_t* __restrict__ irow = a.init_rank ? a.init_rank + krow : nullptr;
    auto elem = [&](int col) -> long {  // element offset of column `col` relative to the row base
        return seg ? (long)(col / a.seg_len) * a.seg_stride + (col % a.seg_len) : (long)col;
    };
    // outputs
    const int lim = m < a.out_limit ? m : a.out_limit;
    const size_t obase = (size_t)row * a.out_row_stride + (size_t)chunk * a.out_chunk_stride;
    int32_t* __restrict__ o_order = a.order ? a.order + obase : nullptr;
    int64_t* __restrict__ o_ids = (!LEAN && a.out_ids) ? a.out_ids + obase : nullptr;
    float* __restrict__ o_kf = a.sorted_keys ? reinterpret_cast<float*>(a.sorted_keys) + obase : nullptr;
    uint32_t* __restrict__ o_kw = a.sorted_keys ? reinterpret_cast<uint32_t*>(reinterpret_cast<double*>(a.sorted_keys) + obase) : nullptr;   // fp64 keys, word by word
    int32_t* __restrict__ o_rank = a.rank ? a.rank + (size_t)row * a.out_row_stride : nullptr;
    const int32_t* __restrict__ cmap = (!LEAN && a.colmap) ? a.colmap + (size_t)row * a.colmap_row_stride : nullptr;
    const int64_t* __restrict__ imap = (!LEAN && a.idmap) ? a.idmap + krow : nullptr;

    // Register state, TWO words per key at any time (E = 28 keys x 3 words does not fit the 128 VGPRs of a 1024-thread
    // workgroup): fp32 -> ks = the key; fp64 -> ks = the HIGH key word during the passes, the LOW key word afterwards
    // (GEN: low word, four passes, high word, four passes, low word).
    uint32_t ks[E];
    uint32_t meta[E];  // low 16: payload (column inside the chunk); high 16: scratch (offset / destination)

    // fp64 key of the element at column `col` (re-derivable at any time from global memory: L2 / Infinity-Cache hits)
    auto key64 = [&](uint2 v) -> uint64_t { return desc_key_f64(__hiloint2double((int)v.y, (int)v.x)); };
    // FUSE: a key costs S divisions to form, and the fp64 form needs every key's words twice (high words for the passes, low words for
    // the repair).  Scratch use of the row's two outputs, both written by nobody else before the output phase:
    //   ORDER output (`stash`)      the LOW sort words of the load phase, indexed by the column / slot the thread itself loaded (it reads
    //                               back what it wrote; 4 B out + 4 B in per key from L2 / Infinity Cache instead of S divisions), live
    //                               until the low-word phase has published them through LDS (the barrier behind that loop);
    //   SORTED-SCORE output (o_kw)  word p < lim = the HIGH half of the sorted key at rank p, parked compactly at the head of the row once the
    //                               digit passes are done, live until the output phase has read ALL of them back (its s_waitcnt + barrier)
    //                               and stores every entry as one 8-byte word.
    // Placed rows that do not fill the row (entries of `order` beyond the list belong to the caller) and calls without an order output
    // form the low words again instead of parking them.
    uint32_t* const stash = reinterpret_cast<uint32_t*>(a.order ? a.order + obase : nullptr);
    const bool use_stash = FUSE && !GEN && stash != nullptr && (!irow || m == a.n_total);   // block-uniform
    // FUSE: the fused float64 scores of B columns (col < 0: not an element, its value is never used), in two halves so that callers can
    // put other work between them: fuse_issue = the rank loads of the FIRST round (N1 = 0, 1 or 2 systems from `s` on), fuse_finish =
    // the adds in system order from 0.0 like fuse_rank_kernel's -- r0v (r0: system 0's ranks are in the caller's registers: the placed
    // form's positions), the first round, then the remaining systems two at a time (loads, then adds).
    auto fuse_issue = [&](auto bt, auto n1_tag, const int (&col)[decltype(bt)::value], int s, int (&ra)[decltype(bt)::value],
                          int (&rb)[decltype(bt)::value]) __attribute__((always_inline)) {
        constexpr int B = decltype(bt)::value, N1 = decltype(n1_tag)::value;
        if constexpr (FUSE && N1 > 0) {
            const int32_t* __restrict__ pa = a.fuse_ranks[s] + krow;
            const int32_t* __restrict__ pb = a.fuse_ranks[N1 > 1 ? s + 1 : s] + krow;
#pragma unroll
            for (int k = 0; k < B; ++k) { const int c = col[k] < 0 ? 0 : col[k]; ra[k] = pa[c]; if constexpr (N1 > 1) rb[k] = pb[c]; }
        }
    };
    auto fuse_finish = [&](auto bt, auto n1_tag, const int (&col)[decltype(bt)::value], const int (&r0v)[decltype(bt)::value], const bool r0,
                           int s, int (&ra)[decltype(bt)::value], int (&rb)[decltype(bt)::value],
                           uint2 (&out)[decltype(bt)::value]) __attribute__((always_inline)) {
        constexpr int B = decltype(bt)::value, N1 = decltype(n1_tag)::value;
        if constexpr (FUSE) {
            double acc[B];
            uint32_t pres = 0u;
#pragma unroll
            for (int k = 0; k < B; ++k) acc[k] = 0.0;
            auto add = [&](int k, int r, double n) {
                if (r >= 0) {
                    const double c = a.fuse_method == FZ_RRF ? recip_small_int_f64((double)(60 + r + 1))   // hybrid.py:252: 1 / (60 + idx + 1)
                                                             : (n - (double)r + 1.0) / n;                  // hybrid.py:249 (sic)
                    acc[k] = acc[k] + c;
                    pres |= 1u << k;
                }
            };
            auto len_of = [&](int sx) -> double { return a.fuse_method == FZ_BCF ? (double)a.fuse_lens[(size_t)sx * a.fuse_rows + row] : 0.0; };
            if (r0) {
                const double n0 = len_of(0);
#pragma unroll
                for (int k = 0; k < B; ++k) if (col[k] >= 0) add(k, r0v[k], n0);
            }
            if constexpr (N1 > 0) {
                const double na = len_of(s), nb = len_of(N1 > 1 ? s + 1 : s);
#pragma unroll
                for (int k = 0; k < B; ++k) if (col[k] >= 0) { add(k, ra[k], na); if constexpr (N1 > 1) add(k, rb[k], nb); }
            }
            for (int s2 = s + N1; N1 == 2 && s2 < a.fuse_S; s2 += 2) {                          // (block-uniform; S > 3 only)
                const bool two = s2 + 1 < a.fuse_S;
                if (two) fuse_issue(bt, std::integral_constant<int, 2>{}, col, s2, ra, rb); else fuse_issue(bt, std::integral_constant<int, 1>{}, col, s2, ra, rb);
                __builtin_amdgcn_sched_barrier(0);
                const double na = len_of(s2), nb = len_of(two ? s2 + 1 : s2);
#pragma unroll
                for (int k = 0; k < B; ++k) if (col[k] >= 0) { add(k, ra[k], na); if (two) add(k, rb[k], nb); }
            }
#pragma unroll
            for (int k = 0; k < B; ++k) {
                const double v = ((pres >> k) & 1u) ? acc[k] : -(double)INFINITY;
                out[k] = make_uint2((uint32_t)__double2loint(v), (uint32_t)__double2hiint(v));
            }
        }
    };
    // how many systems the first round loads: 2 when there are two left after r0 (one memory round trip for S <= 2 + r0), else 1 or 0
    auto fuse_vals = [&](auto bt, const int (&col)[decltype(bt)::value], const int (&r0v)[decltype(bt)::value], const bool r0,
                         uint2 (&out)[decltype(bt)::value]) __attribute__((always_inline)) {
        constexpr int B = decltype(bt)::value;
        if constexpr (FUSE) {
            const int s = r0 ? 1 : 0, left = a.fuse_S - s;
            int ra[B], rb[B];
            auto go = [&](auto n1_tag) __attribute__((always_inline)) {
                fuse_issue(bt, n1_tag, col, s, ra, rb);
                __builtin_amdgcn_sched_barrier(0);
                fuse_finish(bt, n1_tag, col, r0v, r0, s, ra, rb, out);
            };
            if (left >= 2) go(std::integral_constant<int, 2>{});
            else if (left == 1) go(std::integral_constant<int, 1>{});
            else go(std::integral_constant<int, 0>{});
        }
    };

    if (threadIdx.x < 8) misc[8 + threadIdx.x] = (threadIdx.x == 1 || threadIdx.x == 3) ? 0xffffffffu : 0u;  // [8] = or, [9] = and of the sort words; [10] = max, [11] = min, [12] .. [15] = sums (bucket ranking); ZC: [10] = or, [11] = and of the NON-ZERO keys' words, [12] = keys above zero
    uint32_t orw = 0, andw = 0xffffffffu;
    [[maybe_unused]] uint32_t zm = 0u;                                 // ZC: bit i = this thread's item i holds +-0.0
    const bool zc_try = ZC && a.zero_compact && !irow && !init_row && m >= 4096 && a.order;   // block-uniform (the order output: where the low words are parked)
    if (irow) {
        // placed sequence: column j sits at sequence position init_rank[j].  Keys and positions are read coalesced by
        // column; the sort word, then the payload, are scattered to exch[position] and read back in striped order -- the
        // random walk happens in LDS instead of as 27,942 uncoalesced HBM reads per row.  The positions are read twice
        // (second time from L2) rather than held in 28 registers.
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) exch[(slot0 + i * 64)] = SENT;
        __syncthreads();
        SLOT_FRESH();
        if constexpr (!FUSE) {
#pragma unroll
        for (int i0 = 0; i0 < E; i0 += LG) {
            uint32_t pos_t[LG], lo_t[LG], hi_t[LG];
#pragma unroll
            for (int i = i0; i < (i0 + LG < E ? i0 + LG : E); ++i) {
                const int j = (slot0 + i * 64);
                const bool in = j < a.n_total;
                pos_t[i - i0] = (uint32_t)(in ? irow[j] : -1);
                if (KW == 1) lo_t[i - i0] = __float_as_uint(kf[in ? j : 0]);
                else { const uint2 v = kd[in ? j : 0]; lo_t[i - i0] = v.x; hi_t[i - i0] = v.y; }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = i0; i < (i0 + LG < E ? i0 + LG : E); ++i) {
                const int j = (slot0 + i * 64);
                const uint32_t kw = KW == 1 ? desc_key_f32(__uint_as_float(lo_t[i - i0]))
                                            : (uint32_t)(key64(make_uint2(lo_t[i - i0], hi_t[i - i0])) >> (GEN ? 0 : 32));
                if (j < a.n_total && pos_t[i - i0] < (uint32_t)m) exch[pos_t[i - i0]] = kw;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        } else {
            // FUSE: a batch's keys take S divisions each to form -- the NEXT batch's loads (positions + the first round's ranks) are issued
            // before that arithmetic, not after it: two register stages, the batch loop fully unrolled
            constexpr int NB = (E + LG - 1) / LG;
            const int s0 = a.fuse_first_is_pos ? 1 : 0, left = a.fuse_S - s0;                   // block-uniform
            auto run = [&](auto n1_tag) __attribute__((always_inline)) {
                int col_t[2][LG], pos_i[2][LG], ra[2][LG], rb[2][LG];
                auto issue = [&](int b, int st) __attribute__((always_inline)) {
#pragma unroll
                    for (int k = 0; k < LG; ++k) {
                        const int j = (slot0 + (b * LG + k) * 64);
                        const bool in = b * LG + k < E && j < a.n_total;
                        col_t[st][k] = in ? j : -1;
                        pos_i[st][k] = in ? irow[j] : -1;
                    }
                    fuse_issue(std::integral_constant<int, LG>{}, n1_tag, col_t[st], s0, ra[st], rb[st]);
                };
                issue(0, 0);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const int st = b & 1;
                    if (b + 1 < NB) issue(b + 1, st ^ 1);
                    __builtin_amdgcn_sched_barrier(0);
                    uint2 v_t[LG];
                    fuse_finish(std::integral_constant<int, LG>{}, n1_tag, col_t[st], pos_i[st], a.fuse_first_is_pos != 0, s0, ra[st], rb[st], v_t);
#pragma unroll
                    for (int k = 0; k < LG; ++k) {
                        const int j = col_t[st][k];
                        const uint64_t k64 = key64(v_t[k]);
                        if (!GEN && use_stash && j >= 0) stash[j] = (uint32_t)k64;
                        if (j >= 0 && (uint32_t)pos_i[st][k] < (uint32_t)m) exch[pos_i[st][k]] = (uint32_t)(k64 >> (GEN ? 0 : 32));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if (left >= 2) run(std::integral_constant<int, 2>{});
            else if (left == 1) run(std::integral_constant<int, 1>{});
            else run(std::integral_constant<int, 0>{});
        }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) ks[i] = exch[(slot0 + i * 64)];
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) exch[(slot0 + i * 64)] = 0xffffu;
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i0 = 0; i0 < E; i0 += 2 * LG) {
            uint32_t pos_t[2 * LG];
#pragma unroll
            for (int i = i0; i < (i0 + 2 * LG < E ? i0 + 2 * LG : E); ++i) {
                const int j = (slot0 + i * 64);
                pos_t[i - i0] = (uint32_t)(j < a.n_total ? irow[j] : -1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = i0; i < (i0 + 2 * LG < E ? i0 + 2 * LG : E); ++i) {
                const int j = (slot0 + i * 64);
                if (j < a.n_total && pos_t[i - i0] < (uint32_t)m) exch[pos_t[i - i0]] = (uint32_t)j;   // payload = own column (< 65535)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            meta[i] = exch[(slot0 + i * 64)];
            if (meta[i] != 0xffffu) { orw |= ks[i]; andw &= ks[i]; }   // a real element landed in this slot
        }
        __syncthreads();
    } else {
        double s1 = 0.0, s2 = 0.0, sn = 0.0, x0 = 0.0;   // row statistics (only when a.row_stats, whole-list form)
        if (!FUSE && st_load) {
            float f0;
            if (KW == 1) f0 = kf[elem(init_row ? 0 : c0)];
            else { const uint2 v0 = kd[elem(init_row ? 0 : c0)]; f0 = (float)__hiloint2double((int)v0.y, (int)v0.x); }
            x0 = (f0 == f0 && fabsf(f0) != INFINITY) ? (double)f0 : 0.0;   // any finite sample of the row keeps the one-pass sums stable
        }
        SLOT_FRESH();
#pragma unroll
        for (int i0 = 0; i0 < E; i0 += LGF) {
            uint32_t lo_t[LGF], hi_t[KW == 2 ? LGF : 1];
            [[maybe_unused]] int col_t[FUSE ? LGF : 1];
#pragma unroll
            for (int i = i0; i < (i0 + LGF < E ? i0 + LGF : E); ++i) {
                // branch-free: out-of-range lanes load a safe element (column c0 exists because m > 0) and discard it
                const int p = (slot0 + i * 64);
                const bool valid = p < m;
                int col = valid ? c0 + p : c0;
                if (init_row) col = init_row[col];
                const bool ok = valid && (unsigned)col < (unsigned)a.n_total;
                // payload: the source column (gathered sequence) or the column inside the chunk
                meta[i] = ok ? (uint32_t)(init_row ? col : col - c0) : 0xffffu;
                col = ok ? col : c0;
                if constexpr (FUSE) col_t[i - i0] = ok ? col : -1;
                else if (KW == 1) lo_t[i - i0] = __float_as_uint(kf[elem(col)]);
                else { const uint2 v = kd[elem(col)]; lo_t[i - i0] = v.x; hi_t[KW == 2 ? i - i0 : 0] = v.y; }
            }
            if constexpr (FUSE) {
#pragma unroll
                for (int k = (i0 + LGF < E ? LGF : E - i0); k < LGF; ++k) col_t[k] = -1;
                uint2 v_t[LGF];
                if (init_row) __builtin_amdgcn_sched_barrier(0);
                fuse_vals(std::integral_constant<int, LGF>{}, col_t, col_t, false, v_t);
#pragma unroll
                for (int k = 0; k < LGF; ++k) { lo_t[k] = v_t[k].x; hi_t[k] = v_t[k].y; }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = i0; i < (i0 + LGF < E ? i0 + LGF : E); ++i) {
                const bool ok = meta[i] != 0xffffu;
                uint32_t kw;
                if constexpr (KW == 1) kw = desc_key_f32(__uint_as_float(lo_t[i - i0]));
                else {
                    const uint64_t k64 = key64(make_uint2(lo_t[i - i0], hi_t[KW == 2 ? i - i0 : 0]));
                    kw = (uint32_t)(k64 >> (GEN ? 0 : 32));
                    if constexpr (FUSE && !GEN) { if (use_stash && ok) stash[(slot0 + i * 64)] = (uint32_t)k64; }
                    if constexpr (ZC) zm |= (uint32_t)(ok && ((hi_t[i - i0] << 1) | lo_t[i - i0]) == 0u) << i;   // +-0.0 (all the load phase pays for ZC)
                }
                ks[i] = ok ? kw : SENT;
                orw |= ok ? kw : 0u; andw &= ok ? kw : 0xffffffffu;
                if (st_load) {   // the value as the normalisations see it: float32 (BM25's float64 scores rounded, hybrid.py:261)
                    const float xf = KW == 1 ? __uint_as_float(lo_t[i - i0]) : (float)__hiloint2double((int)hi_t[KW == 2 ? i - i0 : 0], (int)lo_t[i - i0]);
                    const double dd = ok ? (double)xf - x0 : 0.0;
                    s1 += dd; s2 = fma(dd, dd, s2); sn += ok ? 1.0 : 0.0;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();   // misc[8..9] initialised
        if (st_load) {   // block-uniform
            // z-score statistics of the row (torch.mean / torch.std of the float32 scores, hybrid.py:261-262): one pass, shifted by
            // the row's first value, fp64 throughout; wave sums by shuffles, the NW partial triples through the (still unused)
            // counter area, folded in wave order by every thread identically
            s1 = wave_reduce_sum(s1); s2 = wave_reduce_sum(s2); sn = wave_reduce_sum(sn);
            double* red = reinterpret_cast<double*>(cnt);
            if (lane == 0) { red[w] = s1; red[NW + w] = s2; red[2 * NW + w] = sn; }
            __syncthreads();
            if (threadIdx.x == 0) {
                double S1 = 0.0, S2 = 0.0, n = 0.0;
                for (int i = 0; i < NW; ++i) { S1 += red[i]; S2 += red[NW + i]; n += red[2 * NW + i]; }
                const double mean = n > 0.0 ? x0 + S1 / n : (double)NAN;
                const double var = n > 1.0 ? (S2 - S1 * S1 / n) / (n - 1.0) : (double)NAN;
                a.row_stats[row] = (float)mean;
                a.row_stats[a.stats_rows + row] = (float)sqrt(var < 0.0 ? 0.0 : var);
            }
            __syncthreads();
        }
    }
    // which bits of the sort word vary over the row?
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { orw |= __shfl_xor(orw, o, 64); andw &= __shfl_xor(andw, o, 64); }
    if (lane == 0) { atomicOr(&misc[8], orw); atomicAnd(&misc[9], andw); }
    if constexpr (ZC) {
        if (zc_try) {   // (block-uniform) per wave: zeros | non-zero keys << 16 -> misc[16 + w]
            int nin = (m - slot0 + 63) >> 6;                   // this thread's items inside the row (identity sequence: slot < m)
            nin = nin < 0 ? 0 : (nin > E ? E : nin);
            const uint32_t zt = (uint32_t)__popc(zm);
            uint32_t pk = zt | (((uint32_t)nin - zt) << 16);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) pk += __shfl_xor(pk, o, 64);
            if (lane == 0) misc[16 + w] = pk;
        }
    }
    __syncthreads();
    uint32_t diff = misc[8] ^ misc[9];                // bits that vary among the REAL keys: a digit without any is skipped
    // Slots beyond the sequence hold the all-ones sentinel and take part in the wave ballots: a bit may only be left out
    // of the match when it is constant over the sentinels too, i.e. constant ONE.
    bool has_sent = irow || init_row || m < T * E;
    uint32_t diff_match = has_sent ? ~misc[9] : diff;
    // ZC: the row's zeros leave the ordering phases (see the note at ZC's definition)
    [[maybe_unused]] int zc_Z = 0, zc_P = 0, zc_zbase = 0, zc_nzbase = 0;   // zeros in the row | keys above zero | zeros / non-zero keys in the waves before this one
    [[maybe_unused]] bool compacted = false;                    // block-uniform
    if constexpr (ZC) {
        if (zc_try) {
            uint32_t nz_all = 0, z_all = 0, nz_before = 0, z_before = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) {
                const uint32_t c = misc[16 + ww];
                z_all += c & 0xffffu; nz_all += c >> 16;
                if (ww < w) { z_before += c & 0xffffu; nz_before += c >> 16; }
            }
            if (nz_all > 0u && z_all * 8u >= (uint32_t)m * 3u) {
                compacted = true;
                zc_Z = (int)z_all; zc_zbase = (int)z_before; zc_nzbase = (int)nz_before;
                Ee = (((int)nz_all + T - 1) / T + 3) & ~3;
                // The non-zero keys, in sequence order, to COMPACT positions: (non-zero keys of the waves before) + (of this wave's earlier
                // items) + (of the lanes below).  High sort words through LDS; the LOW sort words -- the ordering phases need them once more,
                // after the digit passes -- are formed again here, while the row is still warm in L2 (the whole-row form re-reads all of it
                // from the Infinity Cache / HBM a hundred microseconds later), and parked by compact position in the row's ORDER output,
                // which nobody writes before the output phase.  The payload of the ordering phases is the compact position itself: the
                // columns are handed over once, at the end.
                uint32_t run = nz_before;
                SLOT_FRESH();
#pragma unroll
                for (int i0 = 0; i0 < E; i0 += 7) {
                    uint32_t lo_t[7], hi_t[7], pos_t[7];
#pragma unroll
                    for (int i = i0; i < (i0 + 7 < E ? i0 + 7 : E); ++i) {
                        const int p = slot0 + i * 64;
                        const bool mv = p < m && !((zm >> i) & 1u);
                        const unsigned long long bal = __ballot(mv);
                        const uint32_t pos = run + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                        run += (uint32_t)__popcll(bal);
                        pos_t[i - i0] = mv ? pos : 0xffffffffu;
                        const uint2 v = kd[mv ? p : 0];
                        lo_t[i - i0] = v.x; hi_t[i - i0] = v.y;
                        if (mv) exch[pos] = ks[i];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = i0; i < (i0 + 7 < E ? i0 + 7 : E); ++i)
                        if (pos_t[i - i0] != 0xffffffffu) stash[pos_t[i - i0]] = (uint32_t)key64(make_uint2(lo_t[i - i0], hi_t[i - i0]));
                    __builtin_amdgcn_sched_barrier(0);
                }
                __syncthreads();
                slot0 = w * Ee * 64 + lane;                    // from here to the output phase: the compact layout
                m = (int)nz_all;
                uint32_t orz = 0u, andz = 0xffffffffu, pth = 0u;   // or / and of the non-zero keys' words; keys above zero (sign bit of the sort word clear: NaN, +x, +denormal)
                SLOT_FRESH();
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    ITEM_GUARD(i)
                    const int p = slot0 + i * 64;
                    const bool in = p < m;
                    const uint32_t kw = exch[in ? p : 0];
                    ks[i] = in ? kw : SENT;
                    meta[i] = in ? (uint32_t)p : 0xffffu;       // payload = compact position
                    orz |= in ? kw : 0u; andz &= in ? kw : 0xffffffffu; pth += (in && (int)kw >= 0) ? 1u : 0u;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    orz |= __shfl_xor(orz, o, 64); andz &= __shfl_xor(andz, o, 64); pth += __shfl_xor(pth, o, 64);
                }
                if (lane == 0) { atomicOr(&misc[10], orz); atomicAnd(&misc[11], andz); atomicAdd(&misc[12], pth); }
                __syncthreads();
                zc_P = (int)misc[12];
                const uint32_t orn = misc[10], andn = misc[11];
                diff = orn ^ andn;
                has_sent = m < T * Ee;
                diff_match = has_sent ? ~andn : diff;
            }
            if (threadIdx.x == 0) atomicAdd(&g_zero_compact_rows[compacted ? 0 : 1], 1ull);
        }
    }
    // ZC, compacted row: sorted non-zero slot p stands at list position p (above zero) or p + Z (below zero): where its outputs go
    [[maybe_unused]] auto fpos = [&](int p) -> int { if constexpr (ZC) return (compacted && p >= zc_P) ? p + zc_Z : p; else return p; };

    // One stable LSD pass over the 8-bit digit at `shift` of ks (which travels with the payload).
    // dmask: the digit's bits that vary over the row.
    auto radix_pass = [&](const int shift, const uint32_t dmask) {
        // ---- 1. rank inside the wave ------------------------------------------------
        uint32_t* my = cnt + w * 256;
        my[lane] = 0; my[lane + 64] = 0; my[lane + 128] = 0; my[lane + 192] = 0;
        // FULL (wave-uniform: every bit of the digit varies) is one straight-line block over the 28 items, no scalar branch per bit
        auto rank_items = [&](auto full_tag) {
            constexpr bool FULL = decltype(full_tag)::value;
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) {
                ITEM_GUARD(i)
                const uint32_t kw = ks[i];
                const uint32_t d = (kw >> shift) & 0xffu;
                // wave64 match-any on the digit's VARYING bits (a bit that is constant over the row cannot separate peers;
                // dmask is wave-uniform, the skip is a scalar branch), 4 VALU per bit: sign-extended bit (0 / -1), ballot,
                // and mask &= ~(ballot ^ sext) as one v_bitop3 per 32-lane half
                uint32_t mlo = 0xffffffffu, mhi = 0xffffffffu;
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    if (!FULL && !((dmask >> b) & 1u)) continue;
                    const uint32_t sx = (uint32_t)__builtin_amdgcn_sbfe((int)kw, (unsigned)(shift + b), 1u);
                    const unsigned long long bal = __ballot(sx != 0u);
                    mlo &= ~(((uint32_t)bal) ^ sx);
                    mhi &= ~(((uint32_t)(bal >> 32)) ^ sx);
                }
                const uint32_t below = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
                const uint32_t npeer = __popc(mlo) + __popc(mhi);
                const uint32_t old = my[d];
                if (below == 0) my[d] = old + npeer;
                // bytes {3,2} <- (old+below), bytes {1,0} <- payload : one v_perm_b32
                meta[i] = __builtin_amdgcn_perm(old + below, meta[i], 0x05040100u);
                // opaque to the optimiser: otherwise hipcc keeps old, below, payload and &my[d] in four separate
                // registers per item across the barrier (6.6 VGPRs/item -> scratch spills at E = 28)
                asm volatile("" : "+v"(meta[i]));
            }
        };
        if (dmask == 0xffu) rank_items(std::true_type{}); else rank_items(std::false_type{});
        __syncthreads();
        // ---- 2. exclusive prefix over (digit, wave), digit-major ----------------------
        uint32_t tot = 0, incl = 0;
        if (threadIdx.x < 256) {
            uint32_t run = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) {
                uint32_t c = cnt[ww * 256 + threadIdx.x];
                cnt[ww * 256 + threadIdx.x] = run;
                run += c;
            }
            tot = run;
            incl = wave_incl_scan_u32(tot, lane);
            if (lane == 63) misc[w] = incl;
        }
        __syncthreads();
        if (threadIdx.x < 256) {
            uint32_t base = incl - tot;
            for (int ww = 0; ww < w; ++ww) base += misc[ww];
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) cnt[ww * 256 + threadIdx.x] += base;
        }
        __syncthreads();
        // ---- 3. destination, exchange --------------------------------------------------
        // (sched_barrier every 4 items: without it hipcc hoists all E LDS addresses/values and spills)
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            ITEM_GUARD(i)
            uint32_t kw = ks[i];
            asm volatile("" : "+v"(kw));  // recompute the digit here instead of keeping &my[d] alive per item
            const uint32_t d = (kw >> shift) & 0xffu;
            const uint32_t dst = my[d] + (meta[i] >> 16);
            meta[i] = __builtin_amdgcn_perm(dst, meta[i], 0x05040100u);
            asm volatile("" : "+v"(meta[i]));
            exch[dst] = kw;
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            ITEM_GUARD(i)
            ks[i] = exch[(slot0 + i * 64)];
            if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            ITEM_GUARD(i)
            exch[meta[i] >> 16] = meta[i] & 0xffffu;
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            ITEM_GUARD(i)
            meta[i] = exch[(slot0 + i * 64)];
            if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    };
    // move (ks, payload) to the slots in meta's high halves (a permutation of [0, m)); slots >= m keep theirs
    auto permute_to_meta_hi = [&]() __attribute__((always_inline)) {
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) { ITEM_GUARD(i) if ((slot0 + i * 64) < m) exch[meta[i] >> 16] = ks[i]; }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) { ITEM_GUARD(i) if ((slot0 + i * 64) < m) ks[i] = exch[(slot0 + i * 64)]; }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) { ITEM_GUARD(i) if ((slot0 + i * 64) < m) exch[meta[i] >> 16] = meta[i] & 0xffffu; }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) { ITEM_GUARD(i) if ((slot0 + i * 64) < m) meta[i] = exch[(slot0 + i * 64)]; }
        __syncthreads();
    };
    // fp64: (re)load one key word of every slot's element from global memory, by payload (a gather; rare paths only)
    auto reload_word = [&](bool high) {
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const uint32_t py = meta[i] & 0xffffu;
            const int col = py == 0xffffu ? c0 : (int)py + ((init_row || irow) ? 0 : c0);
            uint2 kv[1];
            if constexpr (FUSE) { const int c1[1] = {col}; fuse_vals(std::integral_constant<int, 1>{}, c1, c1, false, kv); }
            else kv[0] = kd[elem(col)];
            const uint64_t kk = key64(kv[0]);
            ks[i] = py == 0xffffu ? SENT : (high ? (uint32_t)(kk >> 32) : (uint32_t)kk);
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    };

    // ---- bucket ranking: the stable order by the 32-bit sort word WITHOUT the digit passes ------------------------------------------
    // A row of a ranker's scores is a sample of a smooth distribution: spread over 16,384 buckets whose widths follow the row's own
    // density, a key shares its bucket with one or two others, and its rank is the bucket's first slot plus the number of bucket
    // members that precede it -- a handful of comparisons where the four digit passes spend a ballot per key bit.
    //   0. range of the sort words; t(w) = w counted from the row's first word, with the unused exponents between the smallest positive
    //      and negative magnitudes cut out and magnitudes 24 binades under the largest clamped; 1,024 equal COARSE buckets (c = t >> s1);
    //   1. a histogram of 4 keys per thread over the coarse buckets -> coarse bucket c is cut into nsub[c] ~ its share of the keys FINE
    //      buckets: fine(w) = base[c] + floor(frac * nsub[c]), rem(w) = the next 16 bits of that product.  (fine, rem) is a monotone
    //      function of w, exact (distinct words, distinct values) wherever a coarse bucket holds more than a few dozen keys;
    //   2. counting sort by fine bucket: packed 16-bit LDS counters (atomic add), exclusive scan, a second atomic add on the
    //      offsets hands out the slots; a slot holds rem << 16 | sequence position; a bitmap marks the buckets' first slots;
    //   3. the thread of SLOT d counts the members of d's bucket below d's entry: that entry's rank (16 bits per slot);
    //   4. words, then payloads, travel owner -> entry slot -> rank through LDS, and every slot checks its left neighbour: two DISTINCT
    //      words that shared (fine, rem) stand in position order instead of word order;
    //   5. such a pair is swapped back.  Anything else -- three in a row; and before that: rows with heavy ties, a crowd at the floor, a
    //      bucket over BR_MAX_BUCKET keys, holes in the sequence, fewer than three varying key bytes -- is left to the digit passes: the
    //      arrangement is at every point a stable permutation by a coarsening of the word, so they finish it to the same result.
    // All integer arithmetic on the sort word: NaN / inf / signed zeros are whatever desc_key made of them.
    constexpr bool BR = !GEN && SortLds<T, E, KW>::br;
    auto bucket_rank = [&]() __attribute__((always_inline)) -> bool {
      if constexpr (!BR) return false; else {
        uint32_t* cntF = cnt;                       // [BR_FINE / 2]: two 16-bit counters per word (fine bucket 2k low, 2k + 1 high)
        uint32_t* tab = cnt + BR_FINE / 2;          // [BR_COARSE]: sample count, then base << 16 | nsub
        uint32_t* bm = tab + BR_COARSE;             // [T*E/32 + 1]: bit p = slot p is the first of its bucket; bit m closes the last one
        const int t = threadIdx.x;
        auto wg_excl_scan = [&](uint32_t v, uint32_t& total) -> uint32_t {   // exclusive prefix over the workgroup's threads
            const uint32_t incl = wave_incl_scan_u32(v, lane);
            if (lane == 63) misc[16 + w] = incl;
            __syncthreads();
            uint32_t base = 0, tot = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) { const uint32_t x = misc[16 + ww]; base += ww < w ? x : 0u; tot += x; }
            __syncthreads();
            total = tot;
            return base + incl - v;
        };
        // 0. range; holes (a slot below m without an element: placed / gathered sequences only); equal neighbours among a thread's keys
        //    (a row that is half zeros is turned away here, before its samples queue up on one LDS address)
        uint32_t mn = 0xffffffffu, mx = 0u, eq = 0u;
        bool hole = false;
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            if ((slot0 + i * 64) < m) {
                mn = ks[i] < mn ? ks[i] : mn; mx = ks[i] > mx ? ks[i] : mx;
                hole |= (meta[i] & 0xffffu) == 0xffffu;
                if (i > 0) eq += ks[i] == ks[i > 0 ? i - 1 : 0] ? 1u : 0u;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t a1 = __shfl_xor(mn, o, 64), b1 = __shfl_xor(mx, o, 64);
            mn = a1 < mn ? a1 : mn; mx = b1 > mx ? b1 : mx;
            eq += __shfl_xor(eq, o, 64);
        }
        if (lane == 0) { atomicMin(&misc[11], mn); atomicMax(&misc[10], mx); atomicAdd(&misc[13], eq); }   // initialised before the load phase
        {
            uint4* z = reinterpret_cast<uint4*>(cnt);
            for (int x = t; x < BR_WORDS / 4; x += T) z[x] = make_uint4(0u, 0u, 0u, 0u);
        }
        if (__syncthreads_or(hole ? 1 : 0)) return false;
        if (misc[13] > (uint32_t)m / 16u) return false;                // more than ~6 % equal neighbours (block-uniform)
        // The sort word of a float: 0x7fffffff - |bits| for x >= 0, 0x80000000 + |bits| for x < 0 -- between the smallest positive and the
        // smallest negative value of the row lie all the exponents nobody uses.  Magnitudes more than 24 binades below the row's largest are
        // clamped to that floor (they share one bucket value; a stray one is the check's business) and the gap is cut out: t counts sort
        // words from the row's first, over at most 2 x 24 binades.
        const uint32_t w_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)misc[11]), w_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)misc[10]);
        const uint32_t magp = w_lo < 0x80000000u ? 0x7fffffffu - w_lo : 0u, magn = w_hi >= 0x80000000u ? w_hi - 0x80000000u : 0u;
        const uint32_t magmax = magp > magn ? magp : magn;
        constexpr uint32_t FLOOR = 24u << (KW == 1 ? 23 : 20);         // (fp64: the high word, exponent at bit 20)
        const uint32_t eps = magmax > FLOOR ? magmax - FLOOR : 0u;
        const uint32_t zp = 0x7fffffffu - eps, zn = 0x80000000u + eps;
        auto t_of = [&](uint32_t kw, uint32_t base_p, uint32_t base_n) -> uint32_t {   // base_n = base_p + the gap's width
            const bool neg = kw >= 0x80000000u;
            const uint32_t lo = kw < zp ? kw : zp, hi = kw > zn ? kw : zn;
            return (neg ? hi : lo) - (neg ? base_n : base_p);
        };
        const uint32_t tmin = t_of(w_lo, 0u, 2u * eps);
        const uint32_t range = t_of(w_hi, 0u, 2u * eps) - tmin;
        if (range == 0u) return false;              // (every key at the floor)
        const uint32_t tb_p = tmin, tb_n = tmin + 2u * eps;
        const int nbits = 32 - __builtin_clz(range);
        const int s1 = nbits > 10 ? nbits - 10 : 0;
        const uint32_t shl = (uint32_t)(32 - s1) & 31u, fmask = s1 ? 0xffffffffu : 0u;
        // 1. sample: four keys per thread into the coarse histogram -- and into a 2,048-slot hash table of sort words (the still unused
        //    fine counters): a sample that finds its own word there is a TIE.  A row with heavy ties (SPLADE's or BM25's zeros, a few hundred
        //    distinct values) would fill single buckets and serialise the histogram's atomics on single counters: found out here, cheaply
        {
            uint32_t ns = 0, dup = 0;
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; i += (E + 3) / 4) {
                const bool in = (slot0 + i * 64) < m;
                if (in) {
                    atomicAdd(&tab[t_of(ks[i], tb_p, tb_n) >> s1], 1u);
                    dup += atomicExch(&cntF[(ks[i] * 2654435761u) >> 21], ks[i]) == ks[i] ? 1u : 0u;
                }
                ns += (uint32_t)__popcll(__ballot(in));
            }
            dup = wave_reduce_sum(dup);
            if (lane == 0) { atomicAdd(&misc[14], ns); atomicAdd(&misc[15], dup); }
        }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; i += (E + 3) / 4) if ((slot0 + i * 64) < m) cntF[(ks[i] * 2654435761u) >> 21] = 0u;
        if (misc[15] > misc[14] / 32u) return false;                   // (block-uniform)
        {
            static_assert(BR_COARSE == T, "one thread per coarse bucket");
            const uint32_t nsamp = misc[14], mine = tab[t];                               // (at least one sample: m >= BR_MIN_KEYS)
            // a crowd at the floor (a heavy tail, or zeros under larger scores) is one bucket value: the digit passes' business
            const bool at_floor = eps != 0u && ((w_lo < 0x80000000u && (uint32_t)t == (zp - tb_p) >> s1) || (w_hi >= 0x80000000u && (uint32_t)t == (zn - tb_n) >> s1));
            if (__syncthreads_or((at_floor && mine > nsamp / 64u) ? 1 : 0)) return false;
            const float kf = (float)(BR_FINE - BR_COARSE - 16) / (float)nsamp;
            const uint32_t nsub = 1u + (uint32_t)((float)mine * kf);
            uint32_t total;
            const uint32_t base = wg_excl_scan(nsub, total);
            tab[t] = (base << 16) | nsub;
        }
        __syncthreads();
        auto fine_rem = [&](uint32_t kw, uint32_t& fine, uint32_t& rem) {
            const uint32_t tt = t_of(kw, tb_p, tb_n);
            const uint32_t tb = tab[tt >> s1];
            const uint32_t f24 = ((tt << shl) & fmask) >> 8;                              // the position inside the coarse bucket, 24 bits
            const uint64_t prod = (uint64_t)f24 * (uint64_t)(tb & 0xffffu);                // < 2^38 (v_mul_u32_u24 + v_mul_hi_u32_u24)
            fine = (tb >> 16) + (uint32_t)(prod >> 24);
            rem = (uint32_t)(prod >> 8) & 0xffffu;
        };
        // 2. fine histogram, scan, placement
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            if ((slot0 + i * 64) < m) {
                uint32_t fine, rem;
                fine_rem(ks[i], fine, rem);
                atomicAdd(&cntF[fine >> 1], 1u << ((fine & 1u) * 16u));
            }
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        {
            static_assert(BR_FINE == 16 * T, "sixteen fine buckets (eight packed words) per thread");
            uint4* my4 = reinterpret_cast<uint4*>(cntF + 8 * t);
            const uint4 q0 = my4[0], q1 = my4[1];
            uint32_t wv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
            uint32_t tot = 0, big = 0, sq = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t lo = wv[k] & 0xffffu, hi = wv[k] >> 16;
                tot += lo + hi; big = lo > big ? lo : big; big = hi > big ? hi : big;
                sq += lo * lo + hi * hi;
            }
            sq = wave_reduce_sum(sq);
            if (lane == 0) atomicAdd(&misc[12], sq);                   // the ranking's work: sum of squared bucket sizes
            uint32_t total;
            uint32_t run = wg_excl_scan(tot, total);
            uint32_t st0 = run;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t lo = wv[k] & 0xffffu, hi = wv[k] >> 16;
                if (lo) atomicOr(&bm[st0 >> 5], 1u << (st0 & 31u));
                st0 += lo;
                if (hi) atomicOr(&bm[st0 >> 5], 1u << (st0 & 31u));
                st0 += hi;
            }
            if (t == T - 1) atomicOr(&bm[(uint32_t)m >> 5], 1u << ((uint32_t)m & 31u));
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t lo = wv[k] & 0xffffu, hi = wv[k] >> 16;
                wv[k] = run | ((run + lo) << 16);
                run += lo + hi;
            }
            my4[0] = make_uint4(wv[0], wv[1], wv[2], wv[3]); my4[1] = make_uint4(wv[4], wv[5], wv[6], wv[7]);
            if (__syncthreads_or(big > (uint32_t)BR_MAX_BUCKET ? 1 : 0)) return false;
            if (misc[12] > 8u * (uint32_t)m) return false;             // (ties: a few hundred distinct values)
        }
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int p = slot0 + i * 64;
            if (p < m) {
                uint32_t fine, rem;
                fine_rem(ks[i], fine, rem);
                const uint32_t sh = (fine & 1u) * 16u;
                const uint32_t old = atomicAdd(&cntF[fine >> 1], 1u << sh);     // the offset word: start before, end after the last member
                const uint32_t dst = (old >> sh) & 0xffffu;
                exch[dst] = (rem << 16) | (uint32_t)p;
                meta[i] = __builtin_amdgcn_perm(dst, meta[i], 0x05040100u);      // where this key's entry went
            }
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        // 3. rank, slot by slot: the thread of slot d finds d's bucket in the bitmap of bucket starts and counts the members below its
        //    entry -- the lanes of a wave look at 64 consecutive slots, i.e. at the same few buckets (broadcast reads, equal trip counts).
        //    Straight-line for buckets of up to six slots that begin and end within a bitmap word of d's (the rest: rolled loops).
        //    The thread keeps 16 bits per slot: the rank of the entry that sits there.
        static_assert(E % 2 == 0, "two ranks per register");
        uint32_t rk[E / 2];
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int d = slot0 + i * 64;
            const int dd = d < m ? d : 0;
            int wi = dd >> 5;
            const uint32_t mine = exch[dd];
            const uint32_t Wp = wi ? bm[wi - 1] : 0u, W0 = bm[wi], Wn = bm[wi + 1];
            const uint32_t low = (2u << (dd & 31)) - 1u;               // bits 0 .. d & 31
            uint32_t z = W0 & low, z2 = W0 & ~low;
            int ws = wi, we = wi;
            if (z == 0u) { z = Wp; --ws; }
            if (z2 == 0u) { z2 = Wn; ++we; }
            if (z == 0u || z2 == 0u) {                                 // a bucket of more than 32 slots around d (rare)
                while (z == 0u) { --ws; z = bm[ws]; }                  // (bit 0 of word 0 is set: terminates)
                while (z2 == 0u) { ++we; z2 = bm[we]; }                // (bit m is set: terminates)
            }
            const uint32_t st = (uint32_t)(ws * 32 + 31 - __builtin_clz(z));
            const uint32_t en = (uint32_t)(we * 32 + __builtin_ctz(z2));
            uint32_t v[BR_STRAIGHT];
#pragma unroll
            for (int e = 0; e < BR_STRAIGHT; ++e) v[e] = exch[st + e];           // (beyond the bucket: other entries or the words behind exch[]; not counted)
            const uint32_t n = en - st;
            uint32_t r = st;
#pragma unroll
            for (int e = 0; e < BR_STRAIGHT; ++e) r += ((uint32_t)e < n && v[e] < mine) ? 1u : 0u;
            if (n > (uint32_t)BR_STRAIGHT) {
                for (uint32_t j = st + (uint32_t)BR_STRAIGHT; j < en; ++j) r += exch[j] < mine ? 1u : 0u;
            }
            if (i & 1) rk[i >> 1] |= r << 16; else rk[i >> 1] = r;
            if (i & 1) { asm volatile("" : "+v"(rk[i >> 1])); __builtin_amdgcn_sched_barrier(0); }
        }
        __syncthreads();
        // 4. two hops through LDS, words then payloads: owner -> its entry's slot -> that slot's rank.  Then every slot checks its left
        //    neighbour: two DISTINCT words that shared (fine, rem) may stand in position order instead of word order.
        bool bad = false;
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) if ((slot0 + i * 64) < m) exch[meta[i] >> 16] = round ? (meta[i] & 0xffffu) : ks[i];
            __syncthreads();
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) if ((slot0 + i * 64) < m) { if (round) meta[i] = exch[(slot0 + i * 64)]; else ks[i] = exch[(slot0 + i * 64)]; }
            __syncthreads();
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) if ((slot0 + i * 64) < m) exch[(rk[i >> 1] >> ((i & 1) * 16)) & 0xffffu] = round ? meta[i] : ks[i];
            __syncthreads();
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int p = slot0 + i * 64;
                if (p < m) {
                    if (round) meta[i] = exch[p];
                    else { ks[i] = exch[p]; bad |= p > 0 && exch[p > 0 ? p - 1 : 0] > ks[i]; }
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(bad ? 1 : 0)) return true;
        // 5. (about one row in a hundred) an inverted neighbour pair is swapped back; anything a single round of disjoint swaps does not
        //    settle is left to the digit passes
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) if ((slot0 + i * 64) < m) exch[(slot0 + i * 64)] = ks[i];
        __syncthreads();
        bad = false;
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int p = slot0 + i * 64;
            if (p < m) {
                const bool il = p > 0 && exch[p > 0 ? p - 1 : 0] > ks[i], ir = p + 1 < m && ks[i] > exch[p + 1 < m ? p + 1 : p];
                bad |= il && ir;                                         // three in a row: not a swap
                meta[i] = __builtin_amdgcn_perm((uint32_t)(il ? p - 1 : (ir ? p + 1 : p)), meta[i], 0x05040100u);
            }
        }
        if (__syncthreads_or(bad ? 1 : 0)) return false;               // (ks / meta untouched: still a stable arrangement by a coarsening of the word)
        if (t == 0) atomicAdd(&g_bucket_rank_rows[1], 1ull);
        permute_to_meta_hi();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) if ((slot0 + i * 64) < m) exch[(slot0 + i * 64)] = ks[i];
        __syncthreads();
        bad = false;
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int p = slot0 + i * 64;
            if (p < m) bad |= p > 0 && exch[p > 0 ? p - 1 : 0] > ks[i];
        }
        return !__syncthreads_or(bad ? 1 : 0);
      }
    };

    static_assert(KW == 1 || E <= 32, "fp64: per-thread slot masks are 32 bits");
    uint32_t signm = 0u, nanm = 0u;   // fp64: bit i = slot i's key has its (ascending-key) sign bit set / is the NaN key
    uint32_t contm = 0u;              // fp64: bit i = slot i continues the equal-high-word run of the slot before it
    bool ranked = false;              // block-uniform
    if constexpr (BR) {
        const int npass = (int)((diff & 0xffu) != 0u) + (int)((diff & 0xff00u) != 0u) + (int)((diff & 0xff0000u) != 0u) + (int)((diff >> 24) != 0u);
        if (a.bucket_rank && m >= BR_MIN_KEYS && npass >= 3) {          // (two digit passes -- scores within one binade -- are cheaper than the ranking)
            ranked = bucket_rank();
            if (threadIdx.x == 0) atomicAdd(&g_bucket_rank_rows[ranked ? 0 : 2], 1ull);
        }
    }
    if (!ranked) {
        for (int pass = 0; pass < 4; ++pass) {
            if (((diff >> (pass * 8)) & 0xffu) == 0u) continue;  // constant digit among real keys: order unchanged
            radix_pass(pass * 8, (diff_match >> (pass * 8)) & 0xffu);
        }
    }
    if constexpr (GEN) {
        // generic form: the four passes above ran over the LOW key words; now the high words (re-derived from global
        // memory by payload), four more passes, the high halves of the sorted keys, and the low words again for the output
        reload_word(true);
        uint32_t o1 = 0u, a1 = 0xffffffffu;
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) if ((meta[i] & 0xffffu) != 0xffffu) { o1 |= ks[i]; a1 &= ks[i]; }
        __syncthreads();
        if (threadIdx.x == 0) { misc[8] = 0u; misc[9] = 0xffffffffu; }
        __syncthreads();
        atomicOr(&misc[8], o1); atomicAnd(&misc[9], a1);
        __syncthreads();
        const uint32_t dh = misc[8] ^ misc[9], dh_match = has_sent ? ~misc[9] : dh;
        for (int pass = 0; pass < 4; ++pass)
            if (((dh >> (pass * 8)) & 0xffu) != 0u) radix_pass(pass * 8, (dh_match >> (pass * 8)) & 0xffu);
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int p = (slot0 + i * 64);
            const uint32_t asc = ~ks[i];
            const bool nan = ks[i] == 0u, sgn = (asc >> 31) & 1u;
            signm |= (uint32_t)sgn << i; nanm |= (uint32_t)nan << i;
            if (o_kw && p < lim) o_kw[2 * p + 1] = nan ? 0x7ff80000u : (sgn ? (asc & 0x7fffffffu) : ~asc);
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        reload_word(false);
    } else if constexpr (KW == 2) {
        // fp64 keys: the FOUR passes above ordered the rows by the HIGH key word only (sign, exponent, 20 mantissa bits).
        // Two keys that share a high word but differ in the low word may now be out of order -- but they are ADJACENT
        // (a stable sort by the high word leaves each equal-high-word run contiguous and in sequence order), and such
        // a run is almost always 2-3 keys long, except runs of EQUAL keys (BM25's zeros), which need nothing.  So:
        // note which slots continue their left neighbour's run, write the high halves of the sorted keys, swap the
        // high words for the low words (re-derived from global memory by the thread that loaded them, handed over
        // through LDS by payload), and repair the dirty runs in place.  Same permutation as eight LSD passes over the
        // 64-bit key at half the ranking work and a third of the exchanges.  A row the repair cannot take (see below) is
        // flagged instead (row_flags) and redone by the generic eight-pass form of this kernel (GEN), a second launch in
        // which every other row's workgroup exits at once.
        uint32_t* runbits = cnt;   // [T*E/32]: bit (p & 31) of word p >> 5 = "slot p has the same high word as slot p-1"
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) { ITEM_GUARD(i) exch[(slot0 + i * 64)] = ks[i]; }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            ITEM_GUARD(i)
            const int p = (slot0 + i * 64);
            const bool ps = p > 0 && p < m && exch[p - 1] == ks[i];
            contm |= (uint32_t)ps << i;
            const unsigned long long bal = __ballot(ps);
            if (lane == 0) { runbits[(w * Ee + i) * 2] = (uint32_t)bal; runbits[(w * Ee + i) * 2 + 1] = (uint32_t)(bal >> 32); }
            // the sorted key's high half is final now (the repair only moves keys inside runs of EQUAL high words)
            const uint32_t asc = ~ks[i];
            const bool nan = ks[i] == 0u;           // every NaN maps to the all-zero key; no other key has a zero high word
            const bool sgn = (asc >> 31) & 1u;
            signm |= (uint32_t)sgn << i; nanm |= (uint32_t)nan << i;
            // the sorted score's HIGH half is final here, its low half only after the repair: parked COMPACTLY at the head of the row's
            // score output (word p; whole lines) and stored together with the low half as one 8-byte store in the output phase -- two
            // strided 4-byte passes over the row wrote every line of it twice (2 x 229 MB per 1024 x 27,942 batch, rocprofv3 WRITE_SIZE)
            bool parked = false;
            if constexpr (ZC) {
                if (compacted) {   // (block-uniform: a scalar branch, nothing for a row that kept its zeros)
                    parked = true;
                    const int f = p >= zc_P ? p + zc_Z : p;
                    if (o_kw && p < m && f < lim) o_kw[f] = nan ? 0x7ff80000u : (sgn ? (asc & 0x7fffffffu) : ~asc);
                }
            }
            if (!parked) { if (o_kw && p < lim) o_kw[p] = nan ? 0x7ff80000u : (sgn ? (asc & 0x7fffffffu) : ~asc); }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        // ---- low words: re-derived by the thread that loaded the element, published under its payload ----
        constexpr int LGG = 4;   // (7 in flight measured the same)
        bool zc_low = false;     // block-uniform
        if constexpr (ZC) {
            if (compacted) {     // the low words the compaction parked, by compact position: each thread its own slots (coalesced), published under them
                zc_low = true;
                SLOT_FRESH();
#pragma unroll
                for (int i0 = 0; i0 < E; i0 += 4) {
                    if (i0 >= Ee) break;
                    uint32_t lw[4];
#pragma unroll
                    for (int i = i0; i < (i0 + 4 < E ? i0 + 4 : E); ++i) { const int p = slot0 + i * 64; lw[i - i0] = stash[p < m ? p : 0]; }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = i0; i < (i0 + 4 < E ? i0 + 4 : E); ++i) { const int p = slot0 + i * 64; if (p < m) exch[p] = lw[i - i0]; }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (zc_low) {
        } else if (use_stash) {         // FUSE: the low sort words parked by the load phase, by the slot this thread loaded
            SLOT_FRESH();
#pragma unroll
            for (int i0 = 0; i0 < E; i0 += 7) {
                uint32_t lw[7];
                int pay_t[7];
#pragma unroll
                for (int i = i0; i < (i0 + 7 < E ? i0 + 7 : E); ++i) {
                    const int p = (slot0 + i * 64);
                    int pay;   // payload this slot was loaded with (see the re-deriving form below)
                    if (irow) pay = p < a.n_total ? p : -1;
                    else if (init_row) { int col = p < m ? init_row[c0 + p] : -1; pay = (unsigned)col < (unsigned)a.n_total ? col : -1; }
                    else pay = p < m ? p : -1;
                    pay_t[i - i0] = pay;
                    lw[i - i0] = stash[pay < 0 ? 0 : p];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = i0; i < (i0 + 7 < E ? i0 + 7 : E); ++i)
                    if (pay_t[i - i0] >= 0) exch[pay_t[i - i0]] = lw[i - i0];
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
        SLOT_FRESH();
#pragma unroll
        for (int i0 = 0; i0 < E; i0 += LGG) {
            uint32_t lo_t[LGG], hi_t[LGG];
            int pay_t[LGG];
            [[maybe_unused]] int col_t[FUSE ? LGG : 1];
#pragma unroll
            for (int i = i0; i < (i0 + LGG < E ? i0 + LGG : E); ++i) {
                const int p = (slot0 + i * 64);
                int pay, col;   // payload this slot was loaded with, and its column in the row
                if (irow) { pay = p < a.n_total ? p : -1; col = pay; }
                else if (init_row) { col = p < m ? init_row[c0 + p] : -1; col = (unsigned)col < (unsigned)a.n_total ? col : -1; pay = col; }
                else { pay = p < m_all ? p : -1; col = pay < 0 ? -1 : c0 + pay; }
                pay_t[i - i0] = pay;
                if constexpr (FUSE) col_t[i - i0] = col;
                else { const uint2 v = kd[elem(col < 0 ? c0 : col)]; lo_t[i - i0] = v.x; hi_t[i - i0] = v.y; }
            }
            if constexpr (FUSE) {
#pragma unroll
                for (int k = (i0 + LGG < E ? LGG : E - i0); k < LGG; ++k) { col_t[k] = -1; pay_t[k] = -1; }
                uint2 v_t[LGG];
                if (init_row) __builtin_amdgcn_sched_barrier(0);
                fuse_vals(std::integral_constant<int, LGG>{}, col_t, col_t, false, v_t);
#pragma unroll
                for (int k = 0; k < LGG; ++k) { lo_t[k] = v_t[k].x; hi_t[k] = v_t[k].y; }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = i0; i < (i0 + LGG < E ? i0 + LGG : E); ++i)
                if (pay_t[i - i0] >= 0) exch[pay_t[i - i0]] = (uint32_t)key64(make_uint2(lo_t[i - i0], hi_t[i - i0]));
            __builtin_amdgcn_sched_barrier(0);
        }
        }
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            ITEM_GUARD(i)
            const uint32_t py = meta[i] & 0xffffu;
            ks[i] = py != 0xffffu ? exch[py] : SENT;     // from here on ks = the LOW key word
            if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        // ---- repair.  The runs are described completely by LDS state -- runbits ("same high word as the slot before")
        // and the low words by slot in exch[] -- so the work is done by whichever thread is convenient, not by the slots'
        // owners:
        //   1. a misordered neighbour pair inside a run marks the run's head (nearest clear bit to the left) in dirtybits;
        //   2. the thread whose word holds a DIRTY head re-sorts the run: up to WALK + 1 slots by itself (stable counting
        //      sort; the usual case is a pair), leaving every member's move as a signed byte in delta[]; a longer run
        //      (up to 2 T slots) goes on a short list;
        //   3. listed runs are counted by the whole workgroup (slot x of the run: how many members precede it), the new
        //      slot numbers replace the low words in exch[] and delta[] says 0x7e = "look there";
        //   4. every owner moves (low word, payload) to slot p + delta[p] (0x7f: stays).
        // Runs of EQUAL keys (BM25's zeros, ties) are never dirty and cost nothing.  A dirty run longer than 2 T slots,
        // or more than BIGCAP listed runs, flags the row for the generic launch.
        constexpr int NWORDS = T * E / 32, BIGCAP = 64, BIGMAX = 2 * T;
        static_assert(2 * NWORDS + BIGCAP <= NW * 256 && BIGMAX < 4096, "repair state lives in the counter area");
        uint32_t* dirtybits = cnt + NWORDS;
        uint32_t* biglist = cnt + 2 * NWORDS;
        int8_t* delta = reinterpret_cast<int8_t*>(cnt + NW * 256);   // [T*E] bytes
        const int t = threadIdx.x;
        const int nwords = T * Ee / 32;                        // runbits words the run detection wrote (ZC: the compact layout's)
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) { ITEM_GUARD(i) exch[(slot0 + i * 64)] = ks[i]; }
        {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(delta);
#pragma unroll
            for (int i = 0; i < (E + 3) / 4; ++i) { const int x = i * T + t; if (x < T * E / 4) d32[x] = 0x7f7f7f7fu; }
            if (t < NWORDS) dirtybits[t] = 0u;
            if (t == 0) { misc[12] = 0u; misc[13] = 0u; }
        }
        __syncthreads();
        // 1. every owner compares its slot's low word with the left neighbour's (consecutive lanes, consecutive LDS words: the walk
        //    over a runbits word by ONE thread read slots 32 t + k -- one bank for the whole wave -- and cost 25 us per row on rows
        //    with long runs of equal keys, BM25's zeros)
        bool anybad = false;
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            ITEM_GUARD(i)
            const int p = (slot0 + i * 64);
            const bool cont = (contm >> i) & 1u;
            if (__ballot(cont) == 0ull) continue;              // wave-uniform: nobody in this item continues a run
            const uint32_t prev = exch[p > 0 ? p - 1 : 0];
            if (cont && prev > ks[i]) {                        // out of order in the low word (rare): mark the run's head
                anybad = true;
                const int q = p - 1;                           // the head is the nearest clear runbit at or below slot q
                int wd = q >> 5;
                uint32_t z = ~runbits[wd] & ((2u << (q & 31)) - 1u);
                while (z == 0u) { --wd; z = ~runbits[wd]; }    // terminates: slot 0 never continues a run
                const int h = wd * 32 + 31 - __builtin_clz(z);
                atomicOr(&dirtybits[h >> 5], 1u << (h & 31));
            }
        }
        if (__syncthreads_or(anybad ? 1 : 0)) {
            if (t < NWORDS) {
                uint32_t heads = dirtybits[t];
                while (heads) {
                    const int h = 32 * t + __builtin_ctz(heads);
                    heads &= heads - 1;
                    // end of the run: first slot after h whose bit is clear (slots >= m never continue a run)
                    const int e0 = h + 1;
                    int wd = e0 >> 5;
                    uint32_t z = ~runbits[wd] & ~((1u << (e0 & 31)) - 1u);
                    while (z == 0u && wd + 1 < nwords) { ++wd; z = ~runbits[wd]; }
                    const int L = (z ? wd * 32 + __builtin_ctz(z) : nwords * 32) - h;
                    if (L == 2) { delta[h] = 1; delta[h + 1] = -1; }             // a dirty pair: swap
                    else if (L <= WALK + 1) {                                     // stable counting sort by one thread
                        for (int x = 0; x < L; ++x) {
                            const uint32_t vx = exch[h + x];
                            int before = 0;
                            for (int y = 0; y < L; ++y) { const uint32_t vy = exch[h + y]; before += (vy < vx || (vy == vx && y < x)) ? 1 : 0; }
                            delta[h + x] = (int8_t)(before - x);
                        }
                    } else if (L <= BIGMAX) {
                        const uint32_t idx = atomicAdd(&misc[12], 1u);
                        if (idx < (uint32_t)BIGCAP) biglist[idx] = ((uint32_t)h << 12) | (uint32_t)L;
                        else misc[13] = 1u;
                    } else misc[13] = 1u;
                }
            }
            __syncthreads();
            if (misc[13] != 0u) {                              // block-uniform: leave the row to the generic form
                if (t == 0) a.row_flags[prow] = 1;
                return;
            }
            const int nbig = (int)misc[12];
            for (int bi = 0; bi < nbig; ++bi) {
                const uint32_t ent = biglist[bi];
                const int h = (int)(ent >> 12), L = (int)(ent & 0xfffu);
                int npos[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int x = t + r * T;
                    npos[r] = -1;
                    if (x < L) {
                        const uint32_t vx = exch[h + x];
                        int before = 0;
                        for (int y = 0; y < L; ++y) { const uint32_t vy = exch[h + y]; before += (vy < vx || (vy == vx && y < x)) ? 1 : 0; }
                        npos[r] = h + before;
                    }
                }
                __syncthreads();                               // every low word of the run has been read
#pragma unroll
                for (int r = 0; r < 2; ++r)
                    if (npos[r] >= 0) { exch[h + t + r * T] = (uint32_t)npos[r]; delta[h + t + r * T] = 0x7e; }
            }
            __syncthreads();
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) {
                ITEM_GUARD(i)
                const int p = (slot0 + i * 64);
                const int d = p < m ? (int)delta[p] : 0x7f;
                const uint32_t np = d == 0x7f ? (uint32_t)p : (d == 0x7e ? exch[p] : (uint32_t)(p + d));
                meta[i] = __builtin_amdgcn_perm(np, meta[i], 0x05040100u);
                if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();                                   // the slot numbers in exch[] have been read
            permute_to_meta_hi();
        }
    }

    if constexpr (ZC) {
        if (compacted) {
            // the ordering phases carried compact positions: the columns behind them, once.  The threads that loaded the row name their
            // non-zero items' columns by compact position (the compaction's own count, again), the sorted slots pick theirs up.
            uint32_t run = (uint32_t)zc_nzbase;
            const int s_full = w * E * 64 + lane;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int col = s_full + i * 64;
                const bool mv = col < m_all && !((zm >> i) & 1u);
                const unsigned long long bal = __ballot(mv);
                const uint32_t pos = run + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                run += (uint32_t)__popcll(bal);
                if (mv) exch[pos] = (uint32_t)col;
                if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) {
                ITEM_GUARD(i)
                const uint32_t py = meta[i] & 0xffffu;
                meta[i] = py != 0xffffu ? exch[py] : 0xffffu;
            }
            __syncthreads();
        }
    }

    // ---- statistics by-product (block-uniform).  min / max of a list sorted by score are its two ends (a NaN sorts first and makes both
    // NaN, as torch.min / torch.max do): the columns of entries 0 and slen - 1 go through LDS, thread 0 reads their values back (L2 hits).
    // A ranking cut to its first slen entries also takes its mean / unbiased std here: the sorted words go to LDS by rank and are summed by
    // a rolled, strided loop (two live doubles) -- the same sums unrolled over the 28 register-resident keys spilled the sort's hot loops.
    if (st_on) {
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            ITEM_GUARD(i)
            const int p = (slot0 + i * 64);
            const uint32_t col = (meta[i] & 0xffffu) + ((!init_row && !irow) ? (uint32_t)c0 : 0u);
            if constexpr (ZC) {
                if (p < m && fpos(p) == 0) misc[17] = col;
                if (p < m && fpos(p) == slen - 1) misc[18] = col;
            } else {
                if (p == 0) misc[17] = col;
                if (p == slen - 1) misc[18] = col;
            }
        }
        if constexpr (ZC) {   // a list end that is one of the compacted zeros: the thread that loaded that zero names its column (+0.0 or -0.0: the
            if (compacted && (zc_P == 0 || (slen - 1 >= zc_P && slen - 1 < zc_P + zc_Z))) {   // value the whole-row form would read there)
                int zrun = zc_P + zc_zbase;
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const bool zb = (zm >> i) & 1u;
                    const unsigned long long bal = __ballot(zb);
                    const int f = zrun + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                    zrun += (int)__popcll(bal);
                    const uint32_t col = (uint32_t)(w * E * 64 + i * 64 + lane);
                    if (zb && f == 0) misc[17] = col;
                    if (zb && f == slen - 1) misc[18] = col;
                }
            }
        }
        double x0 = 0.0;
        const bool pre = KW == 1 && st_prefix;
        if (pre) {
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) exch[(slot0 + i * 64)] = ks[i];
            __syncthreads();
            const float f0 = desc_key_f32_inv(exch[0]);
            x0 = (f0 == f0 && fabsf(f0) != INFINITY) ? (double)f0 : 0.0;
            double s1 = 0.0, s2 = 0.0;
#pragma unroll 1
            for (int p = threadIdx.x; p < slen; p += T) {
                const double dd = (double)desc_key_f32_inv(exch[p]) - x0;
                s1 += dd; s2 = fma(dd, dd, s2);
            }
            s1 = wave_reduce_sum(s1); s2 = wave_reduce_sum(s2);
            double* red = reinterpret_cast<double*>(cnt);
            if (lane == 0) { red[w] = s1; red[NW + w] = s2; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            auto val = [&](int col) -> float {
                if (FUSE) return 0.f;                        // (the launcher rejects row_stats with rank fusion)
                if (KW == 1) return kf[elem(col)];
                const uint2 v = kd[elem(col)];
                return (float)__hiloint2double((int)v.y, (int)v.x);
            };
            float lo = 0.f, hi = 0.f;
            if (slen > 0) { hi = val((int)misc[17]); lo = val((int)misc[18]); if (hi != hi) lo = hi; }
            a.row_stats[2 * a.stats_rows + row] = lo;
            a.row_stats[3 * a.stats_rows + row] = hi;
            if (pre) {
                const double* red = reinterpret_cast<const double*>(cnt);
                double S1 = 0.0, S2 = 0.0;
                for (int i = 0; i < NW; ++i) { S1 += red[i]; S2 += red[NW + i]; }
                const double n = (double)slen;
                const double mean = n > 0.0 ? x0 + S1 / n : (double)NAN;
                const double var = n > 1.0 ? (S2 - S1 * S1 / n) / (n - 1.0) : (double)NAN;
                a.row_stats[row] = (float)mean;
                a.row_stats[a.stats_rows + row] = (float)sqrt(var < 0.0 ? 0.0 : var);
            }
        }
        __syncthreads();   // exch[] and the counter area are free again
    }

    // ---- output (coalesced: consecutive lanes = consecutive ranks) -------------------------
    // rank = inverse permutation.  Scattering it straight to HBM costs as much as the four radix passes
    // (27,942 random 4-byte writes per row); it is inverted in LDS instead and stored coalesced.
    const bool rank_via_lds = o_rank && !cmap && (LEAN || a.chunks == 1);   // block-uniform
    const bool full_row = (m_all == a.n_total) && !init_row && !irow;   // a gathered/placed sequence may skip columns
    if constexpr (ZC) slot0 = w * E * 64 + lane;       // (the pre-fill covers the row's COLUMNS: the full layout)
    if (rank_via_lds && !full_row) {
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) exch[(slot0 + i * 64)] = 0xffffffffu;   // columns outside the sequence
        __syncthreads();
    }
    if constexpr (ZC) slot0 = w * Ee * 64 + lane;      // (the sorted entries: the layout of the ordering phases)
    [[maybe_unused]] uint32_t hiw[(KW == 2 && !GEN) ? E : 1];
    if constexpr (KW == 2 && !GEN) {
        if (o_kw) {   // (block-uniform) the parked high halves back -- ALL of them, then a barrier: the 8-byte stores below land on the words they were parked in
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) {
                ITEM_GUARD(i)
                const int p = (slot0 + i * 64);
                int f = p < lim ? p : 0;
                if constexpr (ZC) { if (compacted) { const int g = p >= zc_P ? p + zc_Z : p; f = (p < m && g < lim) ? g : 0; } }   // (block-uniform branch)
                hiw[i] = o_kw[f];
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
        SLOT_FRESH();
#pragma unroll
    for (int i = 0; i < E; ++i) {
        ITEM_GUARD(i)
        int p = (slot0 + i * 64);                              // the sorted slot = the list position ...
        if constexpr (ZC) { if (compacted) p = p >= m ? lim : (p >= zc_P ? p + zc_Z : p); }   // ... (compacted row, block-uniform branch: the zeros stand in between)
        if (p < lim) {
            int col = (int)(meta[i] & 0xffffu);
            if (!init_row && !irow) col += c0;
            const int oc = cmap ? cmap[col] : col;  // -1 = padding candidate of a short top-k chunk
            if (o_order) o_order[p] = oc;
            if (o_ids) o_ids[p] = imap ? imap[elem(col)] : (oc < 0 ? (int64_t)-1 : a.id_base + (int64_t)oc);
            if (KW == 1) { if (o_kf) o_kf[p] = desc_key_f32_inv(ks[i]); }
            else if (o_kw) {
                const uint32_t low = ((nanm >> i) & 1u) ? 0u : (((signm >> i) & 1u) ? ~ks[i] : ks[i]);   // low half of desc_key_f64_inv
                if constexpr (!GEN) reinterpret_cast<uint2*>(o_kw)[p] = make_uint2(low, hiw[i]);
                else o_kw[2 * p] = low;                            // (generic form: its high halves went out in their own pass)
            }
            if (rank_via_lds) exch[col] = (uint32_t)p;          // col < n_total <= T*E
            else if (o_rank && oc >= 0) o_rank[oc] = p;
        }
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (ZC) {
        slot0 = w * E * 64 + lane;                             // back to the columns
        if (compacted) {
            // the zeros: list position = (keys above zero) + (zeros before this one in sequence order); value +0.0 (desc_key maps -0.0 there too)
            int zrun = zc_P + zc_zbase;
            SLOT_FRESH();
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const bool zb = (zm >> i) & 1u;
                const unsigned long long bal = __ballot(zb);
                const int p = zrun + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                zrun += (int)__popcll(bal);
                if (zb && p < lim) {
                    const int col = slot0 + i * 64;            // (identity sequence, whole rows: the column is the slot)
                    if (o_order) o_order[p] = col;
                    if (o_kw) reinterpret_cast<uint2*>(o_kw)[p] = make_uint2(0u, 0u);
                    if (rank_via_lds) exch[col] = (uint32_t)p;
                    else if (o_rank) o_rank[col] = p;
                }
                if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (rank_via_lds) {
        __syncthreads();
        SLOT_FRESH();
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int j = (slot0 + i * 64);
            if (j < a.n_total) {
                const uint32_t r = exch[j];
                if (full_row || r != 0xffffffffu) o_rank[j] = (int32_t)r;
            }
        }
    }
}

#undef SLOT_FRESH
#undef ITEM_GUARD

// ---- rows longer than one workgroup holds (the drop-in path must not stop at 28,672 documents) -------------
// chunk-sort (the kernel above, one workgroup per chunk of the SEQUENCE) + cross-chunk ranking: an element's final
// position = its position in its own sorted chunk + for every other chunk the number of elements that precede it there
// (binary search; ties go to the earlier chunk, i.e. to the earlier sequence position: the stable order).  Exact, any n;
// O(n * chunks * log) work, meant for corpora of 10^5..10^6 documents, not for the LLeQA hot path.
struct LongArgs {
    const void* keys; int key_bits; const int32_t* init_order; const int32_t* init_rank; const int32_t* row_len;
    int rows, n; long ld;
    void* seq_keys; int32_t* seq_cols;            // [rows][n] the incoming sequence, materialised (gathered / placed input only)
    const void* ck; const int32_t* cc;            // [rows][n] chunk-sorted keys / columns
    int chunk_len;
    int32_t* order; void* sorted_keys; int32_t* rank; long out_ld;
};

template <typename K>
__global__ void long_seq_kernel(LongArgs a) {
    const int row = blockIdx.y;
    const K* keys = reinterpret_cast<const K*>(a.keys) + (size_t)row * a.ld;
    K* sk = reinterpret_cast<K*>(a.seq_keys) + (size_t)row * a.n;
    int32_t* sc = a.seq_cols + (size_t)row * a.n;
    int m = a.row_len ? a.row_len[row] : a.n;
    m = m < 0 ? 0 : (m > a.n ? a.n : m);
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < a.n; x += gridDim.x * blockDim.x) {
        if (a.init_order) {                                   // slot x <- column init_order[x]
            const int col = x < m ? a.init_order[(size_t)row * a.ld + x] : -1;
            const bool ok = (unsigned)col < (unsigned)a.n;
            sk[x] = ok ? keys[col] : (K)(-INFINITY);
            sc[x] = ok ? col : -1;
        } else {                                              // column x -> slot init_rank[x]
            const int r = a.init_rank[(size_t)row * a.ld + x];
            if ((unsigned)r < (unsigned)m) { sk[r] = keys[x]; sc[r] = x; }
        }
    }
}

template <typename K> struct DescKey;
template <> struct DescKey<float> { typedef uint32_t T; static __device__ __forceinline__ T of(float v) { return desc_key_f32(v); } };
template <> struct DescKey<double> { typedef uint64_t T; static __device__ __forceinline__ T of(double v) { return desc_key_f64(v); } };

template <typename K>
__global__ void long_merge_kernel(LongArgs a) {
    typedef typename DescKey<K>::T U;
    const int row = blockIdx.y;
    int m = a.row_len ? a.row_len[row] : a.n;
    m = m < 0 ? 0 : (m > a.n ? a.n : m);
    const K* ck = reinterpret_cast<const K*>(a.ck) + (size_t)row * a.n;
    const int32_t* cc = a.cc + (size_t)row * a.n;
    const int CH = a.chunk_len, C = (m + CH - 1) / CH;
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < m; x += gridDim.x * blockDim.x) {
        const int c = x / CH, i = x - c * CH;
        const K v = ck[x];
        const U key = DescKey<K>::of(v);
        int pos = i;
        for (int c2 = 0; c2 < C; ++c2) {
            if (c2 == c) continue;
            const K* base = ck + (size_t)c2 * CH;
            const int len = (m - c2 * CH) < CH ? (m - c2 * CH) : CH;
            int lo = 0, hi = len;                              // first index whose key is > key (c2 < c: ties precede) or >= key (c2 > c)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const U k2 = DescKey<K>::of(base[mid]);
                const bool before = c2 < c ? (k2 <= key) : (k2 < key);
                if (before) lo = mid + 1; else hi = mid;
            }
            pos += lo;
        }
        const int col = cc[x];
        if (a.order) a.order[(size_t)row * a.out_ld + pos] = col;
        if (a.sorted_keys) {
            // the key as the short-row kernel writes it back: -0.0 -> +0.0, every NaN -> the canonical quiet NaN
            K o = v;
            if (v != v) o = sizeof(K) == 4 ? (K)__uint_as_float(0x7fc00000u) : (K)__longlong_as_double(0x7ff8000000000000ll);
            else if (v == (K)0) o = (K)0;
            reinterpret_cast<K*>(a.sorted_keys)[(size_t)row * a.out_ld + pos] = o;
        }
        if (a.rank && col >= 0) a.rank[(size_t)row * a.out_ld + col] = pos;
    }
}

struct SortCfg { int T, E; };

static inline bool pick_cfg(int n, int kw, SortCfg& c) {
    if (n <= 1024) c = {256, 4};
    else if (n <= 4096) c = {256, 16};
    else if (n <= 8192) c = {512, 16};
    else if (n <= 16384) c = {1024, 16};
    else if (n <= SORT_ROW_F64) c = {1024, 28};
    else if (n <= SORT_ROW_F32 && kw == 1) c = {1024, 35};
    else return false;
    return true;
}

template <int T, int E, int KW, int MODE = SORT_ANY>
static int launch_cfg(const SortArgs& a, int prows, hipStream_t st) {
    constexpr size_t lds = SortLds<T, E, KW>::bytes;
    static_assert(lds <= 160 * 1024, "LDS budget of one CU");
    static unsigned long long lds_set = 0ull, lds_set_gen = 0ull;   // per (T,E,KW,FUSE) instantiation
    constexpr int GEN_MODE = (MODE == SORT_FUSE || MODE == SORT_ROWS_ZC) ? (T == 1024 ? SORT_ROWS : SORT_ANY) : MODE;   // flagged rows of the fused / zero-compacting form: the plain generic kernel
    if (int rc = raise_lds_limit((const void*)sort_rows_kernel<T, E, KW, false, MODE>, lds, lds_set)) return rc;
    if constexpr (KW == 2)
        if (int rc = raise_lds_limit((const void*)sort_rows_kernel<T, E, 2, true, GEN_MODE>, lds, lds_set_gen)) return rc;
    if (KW == 2 && !a.row_flags) return FZ_ERR_WORKSPACE;
    SortArgs b = a;
    {   // FZ_SORT_BUCKET_RANK=0: digit passes only (A/B runs, tests of the two forms against each other)
        const char* e = getenv("FZ_SORT_BUCKET_RANK");
        b.bucket_rank = (e && e[0] == '0') ? 0 : 1;
        b.zero_compact = 1;   // (FZ_SORT_ZERO_COMPACT=0 keeps the launcher from picking the SORT_ROWS_ZC instantiation at all: launch_sort)
    }
    sort_rows_kernel<T, E, KW, false, MODE><<<prows, T, lds, st>>>(b);
    FZ_LAUNCH_CHECK();
    if constexpr (KW == 2) {   // rows the fast form flagged (a dirty run of > 17 equal high words): generic eight passes; all others exit at once
        SortArgs g = a;
        if constexpr (MODE == SORT_FUSE) {   // their fused scores as a plain row first (every other row: nothing), then sorted like any float64 plane
            if (!a.fuse_gen_plane) return FZ_ERR_WORKSPACE;
            fuse_flagged_rows_kernel<<<(unsigned)prows, 256, 0, st>>>(a);
            FZ_LAUNCH_CHECK();
            g.keys = a.fuse_gen_plane; g.fuse_S = 0;
        }
        sort_rows_kernel<T, E, 2, true, GEN_MODE><<<prows, T, lds, st>>>(g);
        FZ_LAUNCH_CHECK();
    }
    return FZ_OK;
}

int launch_sort(const SortArgs& a, int kw, int prows, int n_chunk, hipStream_t st) {
    SortCfg c;
    if (!pick_cfg(n_chunk, kw, c)) return FZ_ERR_UNSUPPORTED;
    if (a.fuse_S > 0) {   // rank fusion as the load phase (float64 keys, one workgroup per row)
        if (kw != 2 || a.chunks != 1 || a.row_stats) return FZ_ERR_UNSUPPORTED;
#define FZ_SORT_CASE(TT, EE) if (c.T == TT && c.E == EE) return launch_cfg<TT, EE, 2, SORT_FUSE>(a, prows, st);
        FZ_SORT_CASE(256, 4) FZ_SORT_CASE(256, 16) FZ_SORT_CASE(512, 16) FZ_SORT_CASE(1024, 16) FZ_SORT_CASE(1024, 28)
#undef FZ_SORT_CASE
        return FZ_ERR_UNSUPPORTED;
    }
    // whole rows of one plane, 1024-thread configurations (the rankers' sorts and the final order at LLeQA size): the lean instantiation
    static const int lean_env = [] { const char* e = getenv("FZ_SORT_LEAN"); return e ? atoi(e) : -1; }();   // A/B runs: 0 = never, 1 = fp32 rows too
    if (lean_env != 0 && a.chunks == 1 && a.seg_len >= a.n_total && !a.colmap && !a.idmap && !a.out_ids && c.T == 1024) {
        // float64 keys: the lean form holds no spilled register (120 VGPRs; SORT_ANY: 9 spilled) and measures 2.5 % (plain rows) to
        // 7 % (placed rows) faster.  float32 keys stay on SORT_ANY unless FZ_SORT_LEAN=1: hipcc schedules their lean form into MORE
        // spills (122, sixteen reloads inside the pass loop) and it measures 15 % slower (profiles/r05_sort_modes_ab.json)
        const char* zenv = getenv("FZ_SORT_ZERO_COMPACT");   // =0: the plain instantiation for everybody (A/B runs, tests of the two forms; read per launch)
        const bool zc_env = !(zenv && zenv[0] == '0');
        if (kw == 2 && a.expect_zeros && zc_env && a.order && !a.init_order && !a.init_rank) {   // a lexical ranker's rows: the zero-compacting instantiation
            if (c.E == 16) return launch_cfg<1024, 16, 2, SORT_ROWS_ZC>(a, prows, st);
            if (c.E == 28) return launch_cfg<1024, 28, 2, SORT_ROWS_ZC>(a, prows, st);
        }
        if (kw == 2 && c.E == 16) return launch_cfg<1024, 16, 2, SORT_ROWS>(a, prows, st);
        if (kw == 2 && c.E == 28) return launch_cfg<1024, 28, 2, SORT_ROWS>(a, prows, st);
        if (kw == 1 && lean_env == 1 && c.E == 28) return launch_cfg<1024, 28, 1, SORT_ROWS>(a, prows, st);
    }
#define FZ_SORT_CASE(TT, EE)                                                      \
    if (c.T == TT && c.E == EE) return kw == 1 ? launch_cfg<TT, EE, 1>(a, prows, st) : launch_cfg<TT, EE, 2>(a, prows, st);
    FZ_SORT_CASE(256, 4) FZ_SORT_CASE(256, 16) FZ_SORT_CASE(512, 16) FZ_SORT_CASE(1024, 16) FZ_SORT_CASE(1024, 28)
#undef FZ_SORT_CASE
    if (c.T == 1024 && c.E == 35 && kw == 1) return launch_cfg<1024, 35, 1>(a, prows, st);
    static_assert(SORT_ROW_F32 == 1024 * 35 && SORT_ROW_F64 == 1024 * 28, "the row capacities are T * E of the largest configuration per key width");
    return FZ_ERR_UNSUPPORTED;
}

}  // namespace fz

using namespace fz;

extern "C" int fz_sort_bucket_rank_rows(uint64_t* counts3, int reset) {
    if (counts3) {
        unsigned long long h[3];
        FZ_HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_bucket_rank_rows), sizeof h));
        for (int i = 0; i < 3; ++i) counts3[i] = (uint64_t)h[i];
    }
    if (reset) {
        const unsigned long long z[3] = {0ull, 0ull, 0ull};
        FZ_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_bucket_rank_rows), z, sizeof z));
    }
    return FZ_OK;
}

extern "C" int fz_sort_zero_compact_rows(uint64_t* counts2, int reset) {
    if (counts2) {
        unsigned long long h[2];
        FZ_HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_zero_compact_rows), sizeof h));
        counts2[0] = (uint64_t)h[0]; counts2[1] = (uint64_t)h[1];
    }
    if (reset) {
        const unsigned long long z[2] = {0ull, 0ull};
        FZ_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_zero_compact_rows), z, sizeof z));
    }
    return FZ_OK;
}

extern "C" int fz_sort_max_n(void) { return SORT_ROW_F32; }   // single-workgroup rows (the fast path), fp32 keys; fp64 keys: 28672.  Longer rows: chunk-sort + merge
extern "C" int fz_sort_max_n_f64(void) { return SORT_ROW_F64; }


static size_t long_ws_bytes(int key_bits, int rows, int n) {
    const size_t ksz = key_bits / 8;
    const int CH = sort_row_max(key_bits);
    const size_t C = ((size_t)n + CH - 1) / CH;
    return (size_t)rows * n * (ksz + 4) * 2 + (size_t)rows * C * 4 + 512;
}

static int sort_long_rows(const void* keys, int key_bits, const int32_t* init_order, const int32_t* init_rank, const int32_t* row_len,
                          int rows, int n, int ld, int32_t* order, void* sorted_keys, int32_t* rank, void* workspace,
                          size_t workspace_bytes, hipStream_t st) {
    if (!workspace || workspace_bytes < long_ws_bytes(key_bits, rows, n)) return FZ_ERR_WORKSPACE;
    const size_t ksz = key_bits / 8;
    const int CH = sort_row_max(key_bits);
    const int C = (n + CH - 1) / CH;
    char* ws = reinterpret_cast<char*>(workspace);
    void* seq_keys = ws; ws += (size_t)rows * n * ksz;
    void* ck = ws; ws += (size_t)rows * n * ksz;
    int32_t* seq_cols = reinterpret_cast<int32_t*>(ws); ws += (size_t)rows * n * 4;
    int32_t* cc = reinterpret_cast<int32_t*>(ws); ws += (size_t)rows * n * 4;
    int32_t* flags = reinterpret_cast<int32_t*>(ws);
    LongArgs L{};
    L.keys = keys; L.key_bits = key_bits; L.init_order = init_order; L.init_rank = init_rank; L.row_len = row_len;
    L.rows = rows; L.n = n; L.ld = ld; L.seq_keys = seq_keys; L.seq_cols = seq_cols; L.ck = ck; L.cc = cc; L.chunk_len = CH;
    L.order = order; L.sorted_keys = sorted_keys; L.rank = rank; L.out_ld = ld;
    const bool seq = init_order || init_rank;
    dim3 grid((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024), (unsigned)rows);
    if (seq) {
        if (init_rank) {   // slots no column claims: (-inf, -1)
            if (key_bits == 32) fill_absent_kernel<float><<<1024, 256, 0, st>>>((float*)seq_keys, seq_cols, (size_t)rows * n);
            else fill_absent_kernel<double><<<1024, 256, 0, st>>>((double*)seq_keys, seq_cols, (size_t)rows * n);
            FZ_LAUNCH_CHECK();
        }
        if (key_bits == 32) long_seq_kernel<float><<<grid, 256, 0, st>>>(L); else long_seq_kernel<double><<<grid, 256, 0, st>>>(L);
        FZ_LAUNCH_CHECK();
    }
    SortArgs a{};
    a.keys = seq ? seq_keys : keys; a.row_len = row_len;
    a.n_total = n; a.key_row_stride = seq ? n : ld; a.seg_len = n; a.seg_stride = 0;
    a.chunks = C; a.chunk_len = CH;
    a.order = cc; a.sorted_keys = ck; a.out_row_stride = n; a.out_chunk_stride = CH; a.out_limit = CH;
    a.colmap = seq ? seq_cols : nullptr; a.colmap_row_stride = n;
    a.row_flags = flags;
    int rc = launch_sort(a, key_bits / 32, rows * C, CH, st);
    if (rc != FZ_OK) return rc;
    if (key_bits == 32) long_merge_kernel<float><<<grid, 256, 0, st>>>(L); else long_merge_kernel<double><<<grid, 256, 0, st>>>(L);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" size_t fz_sort_workspace_bytes(int key_bits, int rows, int n) {
    if (rows <= 0 || n <= 0) return 0;
    if (n > sort_row_max(key_bits)) return long_ws_bytes(key_bits, rows, n);
    return key_bits == 64 ? (size_t)rows * 4 : 0;
}

extern "C" int fz_sort_rows_desc(const void* keys, int key_bits, const int32_t* init_order, const int32_t* row_len, int rows,
                                 int n, int ld, int32_t* order, void* sorted_keys, int32_t* rank, float* row_stats, const int32_t* stats_len,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if ((key_bits != 32 && key_bits != 64) || rows < 0 || n < 0 || ld < n) return FZ_ERR_ARG;
    if (rows == 0 || n == 0) return FZ_OK;      // nothing to do (empty tensors carry null pointers)
    if (!keys) return FZ_ERR_ARG;
    if (stats_len && !row_stats) return FZ_ERR_ARG;
    if (stats_len && key_bits != 32) return FZ_ERR_UNSUPPORTED;   // prefix statistics come from the sorted fp32 keys in registers (fz_row_stats_f32 otherwise)
    if (n > sort_row_max(key_bits)) {   // longer than one workgroup's registers: chunk-sort + cross-chunk ranking
        if (row_stats) return FZ_ERR_UNSUPPORTED; // the statistics by-product exists for single-workgroup rows only (fz_row_stats_f32 otherwise)
        return sort_long_rows(keys, key_bits, init_order, nullptr, row_len, rows, n, ld, order, sorted_keys, rank, workspace, workspace_bytes,
                              as_stream(stream));
    }
    SortArgs a = whole_rows(keys, n, ld, order, sorted_keys, rank);
    a.init_order = init_order; a.row_len = row_len;
    a.row_stats = row_stats; a.stats_rows = rows; a.stats_len = stats_len;
    if (key_bits == 64) if (int rc = take_row_flags(a, rows, n, workspace, workspace_bytes)) return rc;
    return launch_sort(a, key_bits / 32, rows, n, as_stream(stream));
}

// A lexical ranker's rows (BM25 / TF-IDF scores, bm25.py:100-106: every document that shares no term with the query scores exactly 0.0): the
// same stable descending sort of float64 rows in the identity sequence, through the instantiation that leaves a row's zeros out of the
// ordering phases when they are at least 3/8 of its >= 4,096 keys (ZC in sort_rows_kernel).  Same outputs, bit for bit, as fz_sort_rows_desc.
extern "C" int fz_sort_rows_desc_lexical(const double* keys, const int32_t* row_len, int rows, int n, int ld, int32_t* order, double* sorted_keys,
                                         int32_t* rank, float* row_stats, void* workspace, size_t workspace_bytes, void* stream) {
    if (rows < 0 || n < 0 || ld < n) return FZ_ERR_ARG;
    if (rows == 0 || n == 0) return FZ_OK;
    if (!keys) return FZ_ERR_ARG;
    if (n > SORT_ROW_F64 || n <= 8192)   // rows of other workgroup sizes: nothing to gain, the general entry point
        return fz_sort_rows_desc(keys, 64, nullptr, row_len, rows, n, ld, order, sorted_keys, rank, row_stats, nullptr, workspace, workspace_bytes, stream);
    SortArgs a = whole_rows(keys, n, ld, order, sorted_keys, rank);
    a.row_len = row_len;
    a.row_stats = row_stats; a.stats_rows = rows;
    a.expect_zeros = 1;
    if (int rc = take_row_flags(a, rows, n, workspace, workspace_bytes)) return rc;
    return launch_sort(a, 2, rows, n, as_stream(stream));
}

extern "C" int fz_sort_rows_desc_placed(const void* keys, int key_bits, const int32_t* init_rank, const int32_t* row_len, int rows,
                                        int n, int ld, int32_t* order, void* sorted_keys, int32_t* rank, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if ((key_bits != 32 && key_bits != 64) || rows < 0 || n < 0 || ld < n) return FZ_ERR_ARG;
    if (rows == 0 || n == 0) return FZ_OK;
    if (!keys || !init_rank) return FZ_ERR_ARG;
    if (n > sort_row_max(key_bits))
        return sort_long_rows(keys, key_bits, nullptr, init_rank, row_len, rows, n, ld, order, sorted_keys, rank, workspace, workspace_bytes,
                              as_stream(stream));
    SortArgs a = whole_rows(keys, n, ld, order, sorted_keys, rank);
    a.init_rank = init_rank; a.row_len = row_len;
    if (key_bits == 64) if (int rc = take_row_flags(a, rows, n, workspace, workspace_bytes)) return rc;
    return launch_sort(a, key_bits / 32, rows, n, as_stream(stream));
}

// Rank fusion + final order in one kernel (hybrid.py:248-252 + :301-306): what fz_fuse_rank_f64 followed by fz_sort_rows_desc[_placed] on its
// float64 plane computes -- the same fused scores bit for bit (formed per key on load by the expression of fuse_rank_kernel), the same
// stable order -- without the [rows][ld] float64 plane ever being written or read (229 MB out + 458 MB in at Q = 1024, N = 27,942).
static size_t fused_flags_bytes(int rows) { return ((size_t)rows * 4 + 255) / 256 * 256; }
// row flags + one float64 row per row: where a row the fast form cannot finish (flagged; practically never) gets its fused scores written
// out for the generic launch.  Untouched otherwise: the bytes are reserved, not moved.
extern "C" size_t fz_sort_rank_fused_workspace_bytes(int rows, int n, int ld) {
    if (rows <= 0 || n <= 0 || ld < n) return 0;
    return fused_flags_bytes(rows) + (size_t)rows * ld * 8;
}

extern "C" int fz_sort_rank_fused_desc(const int32_t* const* ranks_h, const int32_t* lens, int S, int method, const int32_t* init_order,
                                       const int32_t* init_rank, const int32_t* row_len, int rows, int n, int ld, int32_t* order,
                                       double* sorted_scores, int32_t* rank, void* workspace, size_t workspace_bytes, void* stream) {
    if (S <= 0 || S > FZ_MAX_SYSTEMS || rows < 0 || n < 0 || ld < n) return FZ_ERR_ARG;
    if (method != FZ_RRF && method != FZ_BCF) return FZ_ERR_ARG;
    if (init_order && init_rank) return FZ_ERR_ARG;
    if (rows == 0 || n == 0) return FZ_OK;
    if (!ranks_h || !lens) return FZ_ERR_ARG;
    if (n > SORT_ROW_F64) return FZ_ERR_UNSUPPORTED;      // longer rows: fz_fuse_rank_f64 + fz_sort_rows_desc (chunk-sort + merge)
    SortArgs a = whole_rows(nullptr, n, ld, order, sorted_scores, rank);   // (no key plane: the keys are formed from the rank planes)
    for (int s = 0; s < S; ++s) {
        if (!ranks_h[s]) return FZ_ERR_ARG;
        a.fuse_ranks[s] = ranks_h[s];
    }
    a.fuse_lens = lens; a.fuse_S = S; a.fuse_method = method; a.fuse_rows = rows;
    a.fuse_first_is_pos = (init_rank && init_rank == ranks_h[0]) ? 1 : 0;
    a.init_order = init_order; a.init_rank = init_rank; a.row_len = row_len;
    if (!workspace || workspace_bytes < fz_sort_rank_fused_workspace_bytes(rows, n, ld)) return FZ_ERR_WORKSPACE;
    a.row_flags = (int32_t*)workspace;
    a.fuse_gen_plane = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + fused_flags_bytes(rows));
    return launch_sort(a, 2, rows, n, as_stream(stream));
}

// Diagnostic: out[r] = 1 / (60 + r + 1) in float64 for r < count -- fast != 0: by the division-free form the fused sort's load phase uses
// (recip_small_int_f64), else by the IEEE division fuse_rank_kernel uses.  Tests compare the two (and NumPy) over every rank.
extern "C" int fz_rrf_terms_f64(int count, int fast, double* out, void* stream) {
    if (count < 0 || count > (1 << 20)) return FZ_ERR_ARG;
    if (count == 0) return FZ_OK;
    if (!out) return FZ_ERR_ARG;
    rrf_terms_kernel<<<(count + 255) / 256, 256, 0, as_stream(stream)>>>(count, fast, out);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
