// topk.hip -- top-k (A12) over the stable descending row sort of sort.hip, for gfx950: whole rows, the streamed update / filter / fold
// of a corpus shard, the merge of per-shard lists, and the candidate selection of the fused-list ordering.
//
// Reference semantics: util.semantic_search / torch.topk + heap merge (hybrid.py:103, sentence_transformers.py:346-364).
// Everything here orders its rows with launch_sort (sort.h); no kernel of this file sorts.
#include <type_traits>

#include "sort.h"

namespace fz {

// pad the tail of top-k outputs with (-inf, -1)
__global__ void topk_pad_kernel(float* out_scores, int64_t* out_ids, int rows, int k, int have) {
    const int r = blockIdx.y;
    for (int i = have + blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
        out_scores[(size_t)r * k + i] = -INFINITY;
        out_ids[(size_t)r * k + i] = -1;
    }
}

// ---- streaming top-k update -------------------------------------------------------------------------------
// After the first chunk of a corpus shard, the running k-th best score tau[row] bounds what can still enter the
// top-k: chunks arrive in ascending id order, so an element tying with tau has a larger id than the current k-th
// entry and loses; only s > tau (or NaN, which sorts first in this build) survives.  For i.i.d. scores the expected
// number of survivors per row is k * chunk / seen: a few hundred.  One workgroup per row streams the chunk (16-B
// loads), compacts the survivors STABLY (ascending column = ascending id) behind the running list, and the ordinary
// row sort then merges [running k | survivors] (ties: running entries first, then ascending id).
// A row with more survivors than `cap` sets *overflow (checked by the caller, who redoes that chunk exactly).
struct FilterArgs {
    const float* scores; int n; long ld;     // chunk [rows][ld]
    int64_t id_base;
    const float* run_scores;                 // [rows][k] current top-k (sorted desc; -inf padding)
    const int64_t* run_ids;                  // [rows][k]
    int k, cap;
    float* buf_scores; int64_t* buf_ids;     // [rows][k + cap]: running list copied to the front, survivors behind
    int32_t* buf_len;                        // [rows] = k + survivors
    int32_t* overflow;                       // set to 1 if any row exceeded cap
    // append form (fz_topk_filter_append_f32): tau != null -> the threshold comes from tau[row], nothing is copied, survivors go
    // behind the buf_len[row] candidates already in buf_* ([rows][cap], k = 0) and buf_len[row] grows by their number
    const float* tau;
};

// Each of the 4 waves owns a CONTIGUOUS stretch of the row (of a round of 65,536 columns), so "ascending column" = wave order, then step order, then lane order:
// pass 1 streams the stretch from HBM and only counts (a 64-bit mask remembers which 256-column steps had a survivor at all);
// one barrier and a 4-entry scan give every wave its output offset; pass 2 revisits the marked steps (L2 / Infinity-Cache hits)
// and writes.  No barrier and no scan inside the streaming loop.
__global__ __launch_bounds__(256) void topk_filter_kernel(FilterArgs a) {
    constexpr int T = 256, NW = T / 64, STEP = 256, SPAN = NW * 64 * STEP;   // columns per outer round: 64 steps per wave
    __shared__ int wtot[NW];
    const int row = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* __restrict__ x = a.scores + (size_t)row * a.ld;
    float* __restrict__ bs = a.buf_scores + (size_t)row * (a.k + a.cap);
    int64_t* __restrict__ bi = a.buf_ids + (size_t)row * (a.k + a.cap);
    float tau;
    int base = 0;
    if (a.tau) { tau = a.tau[row]; base = a.buf_len[row]; }
    else {
        for (int i = threadIdx.x; i < a.k; i += T) { bs[i] = a.run_scores[(size_t)row * a.k + i]; bi[i] = a.run_ids[(size_t)row * a.k + i]; }
        tau = a.run_scores[(size_t)row * a.k + a.k - 1];   // k-th best so far (-inf while the list is short)
    }
    const bool vec = (a.ld % 4 == 0) && ((uintptr_t)a.scores % 16 == 0);
    bool over = false;
    auto load4 = [&](int j0, float (&v)[4]) {
        if (vec && j0 + 3 < a.n) { const float4 f = *reinterpret_cast<const float4*>(x + j0); v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w; }
        else {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (j0 + c < a.n) ? x[j0 + c] : -INFINITY;
        }
    };
    for (int r0 = 0; r0 < a.n; r0 += SPAN) {
        const int nr = min(a.n - r0, SPAN);
        const int steps = (nr + NW * STEP - 1) / (NW * STEP);      // per wave, <= 64
        const int w0 = r0 + w * steps * STEP;                      // this wave's stretch: steps * 256 columns from w0
        // ---- pass 1: count
        int cnt = 0;
        unsigned long long marked = 0ull;
        constexpr int UNR = 8;                                     // 16-byte loads in flight per lane
        auto count_step = [&](int st, const float (&v)[4]) {
            const int j0 = w0 + st * STEP + lane * 4;
            int c = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) c += ((j0 + e < a.n) && !(v[e] <= tau)) ? 1 : 0;   // s > tau, or NaN (sorts first in this build)
            cnt += c;
            if (__ballot(c != 0)) marked |= 1ull << st;            // wave-uniform
        };
        int s0 = 0;
        // whole groups of UNR steps inside the row: plain 16-byte loads under no branch (behind a conditional load hipcc waits
        // for every outstanding one, which turns the group into a chain of single round trips)
        if (vec)
            for (; s0 + UNR <= steps && w0 + (s0 + UNR) * STEP <= a.n; s0 += UNR) {
                float4 f[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) f[u] = *reinterpret_cast<const float4*>(x + w0 + (s0 + u) * STEP + lane * 4);
#pragma unroll
                for (int u = 0; u < UNR; ++u) { const float v[4] = {f[u].x, f[u].y, f[u].z, f[u].w}; count_step(s0 + u, v); }
            }
        for (; s0 < steps; ++s0) {                                 // the ragged end (or unaligned rows)
            float v[4];
            load4(w0 + s0 * STEP + lane * 4, v);
            count_step(s0, v);
        }
        cnt = wave_reduce_sum(cnt);
        __syncthreads();                                           // (the previous round's wtot has been read)
        if (lane == 0) wtot[w] = cnt;
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) { const int c = wtot[i]; if (i < w) off += c; tot += c; }
        // ---- pass 2: the marked steps again, survivors to their slots.  Four marked steps at a time, their loads issued together
        // (one step at a time is a chain of L2 round trips: at 0.4 % survivors two thirds of the steps are marked and this pass
        // took as long as the HBM pass)
        auto place = [&](int st, const float (&v)[4]) {
            const int j0 = w0 + st * STEP + lane * 4;
            // survivors of lower lanes + own earlier ones, from four ballots (no shuffle chain: this runs once per marked step)
            bool keep[4];
            int pos = off, tot_st = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                keep[e] = (j0 + e < a.n) && !(v[e] <= tau);
                const unsigned long long bal = __ballot(keep[e]);
                pos += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                tot_st += __popcll(bal);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (keep[e]) {
                    if (pos < a.cap) { bs[a.k + pos] = v[e]; bi[a.k + pos] = a.id_base + j0 + e; }
                    else over = true;
                    ++pos;
                }
            off += tot_st;
        };
        // a step is "inner" when all its 256 columns exist: plain 16-byte loads; the (at most one) ragged step goes last, guarded
        const int inner = vec ? max(0, min(steps, (a.n - w0) / STEP)) : 0;
        unsigned long long in_m = inner >= 64 ? marked : (marked & ((1ull << inner) - 1ull));
        unsigned long long rest = marked & ~in_m;
        while (in_m) {
            int st[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {          // the group's steps; a short last group repeats its last step (loaded, not placed)
                st[u] = in_m ? __builtin_ctzll(in_m) : st[u > 0 ? u - 1 : 0];
                if (in_m) in_m &= in_m - 1; else st[u] |= 0x40000000;
            }
            float4 f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = *reinterpret_cast<const float4*>(x + w0 + (st[u] & 0xffff) * STEP + lane * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (!(st[u] & 0x40000000)) { const float v[4] = {f[u].x, f[u].y, f[u].z, f[u].w}; place(st[u], v); }
        }
        while (rest) {
            const int st = __builtin_ctzll(rest);
            rest &= rest - 1;
            float v[4];
            load4(w0 + st * STEP + lane * 4, v);
            place(st, v);
        }
        base += tot;
    }
    __syncthreads();   // (append form: every thread has read buf_len[row])
    if (threadIdx.x == 0) a.buf_len[row] = a.k + (base < a.cap ? base : a.cap);
    if (over) atomicExch(a.overflow, 1);
}

// fold: [running k | candidates] of every row side by side for the row sort; afterwards the new threshold and empty candidate lists
__global__ void topk_concat_kernel(const float* run_scores, const int64_t* run_ids, int k, const float* cand_scores, const int64_t* cand_ids,
                                   const int32_t* cand_len, int cap, float* buf_scores, int64_t* buf_ids, int32_t* buf_len) {
    const int row = blockIdx.x;
    const int len = min(cand_len[row], cap);
    float* bs = buf_scores + (size_t)row * (k + cap);
    int64_t* bi = buf_ids + (size_t)row * (k + cap);
    for (int i = threadIdx.x; i < k; i += blockDim.x) { bs[i] = run_scores[(size_t)row * k + i]; bi[i] = run_ids[(size_t)row * k + i]; }
    for (int i = threadIdx.x; i < len; i += blockDim.x) { bs[k + i] = cand_scores[(size_t)row * cap + i]; bi[k + i] = cand_ids[(size_t)row * cap + i]; }
    if (threadIdx.x == 0) buf_len[row] = k + len;
}
__global__ void topk_fold_done_kernel(const float* new_scores, int rows, int k, float* tau, int32_t* cand_len) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    if (tau) tau[row] = new_scores[(size_t)row * k + k - 1];
    cand_len[row] = 0;
}

// ---- top-k form of the fused-list ordering (hybrid.py:306 + main's predictions(1000), :537) -------------------------------------------
// Aggregator.fuse sorts every fused row in full; what main() reads of it is the first 1000 entries.  For that use the row is SELECTED, not
// sorted: one workgroup holds the row's float32 sort keys in registers, bisects the key range for a threshold that at least k and at most
// cap keys do not exceed (one count + workgroup sum per step), and writes the documents at or above it -- the k best, every tie at the
// k-th place and up to cap - k more -- with their fused scores and (negated) first-insertion positions.  Two small row sorts then put
// those candidates into insertion order and, stably, into score order: the first k entries of the full sort, bit for bit.
// float64 fused scores (rrf / bcf / 'none') are selected by their float32 rounding -- rounding is monotone, so the k-th largest rounded
// value is the rounding of the k-th largest value and nothing of the top-k is lost; the candidates keep their float64 scores.
struct SelectArgs {
    const void* fused; int key_bits;   // [rows][ld] float32 (32) or float64 (64)
    const int32_t* pos;                // nullable [rows][ld]: first-insertion position of the column, < 0 = in no list; NULL = the column itself
    int n, ld, k, cap;
    int32_t* cand_cols;                // [rows][cap]
    void* cand_vals;                   // [rows][cap] same type as fused
    float* cand_negpos;                // [rows][cap] -(float)position: descending sort = ascending insertion position
    int32_t* cand_len;                 // [rows]
    int32_t* overflow;                 // set when a row has more than cap candidates (the caller then sorts in full)
};

template <int T, int E, int KW>
__global__ __launch_bounds__(T) void topk_select_kernel(SelectArgs a) {
    constexpr int NW = T / 64;
    __shared__ uint32_t red[2][NW];
    const int row = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t base = (size_t)row * a.ld;
    const float* __restrict__ vf = reinterpret_cast<const float*>(a.fused) + base;
    const double* __restrict__ vd = reinterpret_cast<const double*>(a.fused) + base;
    const int32_t* __restrict__ ps = a.pos ? a.pos + base : nullptr;
    uint32_t key[E];
    uint32_t nvalid = 0u;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int j = w * E * 64 + i * 64 + lane;
        const bool in = j < a.n;
        const int p = in ? (ps ? ps[j] : j) : -1;
        const float v = KW == 1 ? vf[in ? j : 0] : (float)vd[in ? j : 0];
        const bool ok = in && p >= 0;
        key[i] = ok ? desc_key_f32(v) : 0xffffffffu;           // (no real key is all ones: that would be -NaN's pattern, mapped to 0)
        nvalid += ok ? 1u : 0u;
    }
    // wave sums / minima / maxima on the VALU (DPP + permlane swaps: no LDS round trips), partials through parity-buffered LDS slots:
    // one barrier per reduction
    auto wave_u32 = [&](uint32_t v, auto op) __attribute__((always_inline)) -> uint32_t {
        auto dpp = [&](uint32_t x, auto ctrl) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, decltype(ctrl)::value, 0xf, 0xf, true); };
        v = op(v, dpp(v, std::integral_constant<int, 0xB1>{})); v = op(v, dpp(v, std::integral_constant<int, 0x4E>{}));
        v = op(v, dpp(v, std::integral_constant<int, 0x141>{})); v = op(v, dpp(v, std::integral_constant<int, 0x140>{}));
        float x = __uint_as_float(v), o = x;
        swap16(x, o); v = op(__float_as_uint(x), __float_as_uint(o));
        x = __uint_as_float(v); o = x;
        swap32(x, o);
        return op(__float_as_uint(x), __float_as_uint(o));
    };
    auto add_ = [](uint32_t p, uint32_t q) { return p + q; };
    auto min_ = [](uint32_t p, uint32_t q) { return p < q ? p : q; };
    auto max_ = [](uint32_t p, uint32_t q) { return p > q ? p : q; };
    int par = 0;
    auto block_u32 = [&](uint32_t v, auto op, uint32_t ident) __attribute__((always_inline)) -> uint32_t {
        v = wave_u32(v, op);
        if (lane == 0) red[par][w] = v;
        __syncthreads();
        uint32_t t = ident;
#pragma unroll
        for (int i = 0; i < NW; ++i) t = op(t, red[par][i]);
        par ^= 1;
        return t;
    };
    uint32_t kmin = 0xffffffffu, kmax = 0u;
#pragma unroll
    for (int i = 0; i < E; ++i) if (key[i] != 0xffffffffu) { kmin = min_(kmin, key[i]); kmax = max_(kmax, key[i]); }
    const uint32_t total = block_u32(nvalid, add_, 0u);
    kmin = block_u32(kmin, min_, 0xffffffffu);
    kmax = block_u32(kmax, max_, 0u);
    const uint32_t need = (uint32_t)a.k < total ? (uint32_t)a.k : total;   // fewer listed documents than k: all of them
    // A threshold key tau with need <= #{key <= tau} <= cap is all the two sorts behind this kernel need -- not the exact k-th smallest
    // key -- so the bisection over the key range stops at the first midpoint whose count falls into that window (k = 1000 of 27,942,
    // cap = 2 k: 8-12 counts instead of one per key bit).  If no midpoint does (a tie run longer than cap - k at the k-th place) it ends
    // at the smallest key with at least `need` keys at or below it, the count exceeds cap and the overflow flag sends the caller to the
    // full sort.
    uint32_t tau = kmax;
    if (total > (uint32_t)a.cap) {
        uint32_t lo = kmin, hi = kmax;                         // invariant: count(<= hi) >= need
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            uint32_t c = 0;
#pragma unroll
            for (int i = 0; i < E; ++i) c += key[i] <= mid ? 1u : 0u;
            c = block_u32(c, add_, 0u);
            if (c < need) lo = mid + 1;
            else { hi = mid; tau = mid; if (c <= (uint32_t)a.cap) break; }
        }
        if (lo >= hi) tau = hi;
    }
    // candidates: every listed document whose key does not exceed the threshold
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < E; ++i) mine += (need > 0 && key[i] <= tau && key[i] != 0xffffffffu) ? 1u : 0u;
    uint32_t incl = wave_incl_scan_u32(mine, lane);
    __syncthreads();                                           // (the last reduction's slots have been read)
    if (lane == 63) red[0][w] = incl;
    __syncthreads();
    uint32_t off = incl - mine, all = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { if (i < w) off += red[0][i]; all += red[0][i]; }
    if (threadIdx.x == 0) {
        a.cand_len[row] = (int32_t)(all < (uint32_t)a.cap ? all : (uint32_t)a.cap);
        if (all > (uint32_t)a.cap) atomicExch(a.overflow, 1);
    }
    const size_t cb = (size_t)row * a.cap;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        if (need > 0 && key[i] <= tau && key[i] != 0xffffffffu) {
            if (off < (uint32_t)a.cap) {
                const int j = w * E * 64 + i * 64 + lane;
                a.cand_cols[cb + off] = j;
                a.cand_negpos[cb + off] = -(float)(ps ? ps[j] : j);
                if (KW == 1) reinterpret_cast<float*>(a.cand_vals)[cb + off] = vf[j];
                else reinterpret_cast<double*>(a.cand_vals)[cb + off] = vd[j];
            }
            ++off;
        }
    }
}

}  // namespace fz

using namespace fz;

extern "C" int fz_select_topk_f(const void* fused, int key_bits, const int32_t* pos, int rows, int n, int ld, int k, int cap, int32_t* cand_cols,
                                void* cand_vals, float* cand_negpos, int32_t* cand_len, int32_t* overflow, void* stream) {
    if ((key_bits != 32 && key_bits != 64) || rows < 0 || n < 0 || ld < n || k <= 0 || cap < k) return FZ_ERR_ARG;
    if (rows == 0) return FZ_OK;
    if (!cand_len || !overflow) return FZ_ERR_ARG;
    if (n == 0) { FZ_HIP_TRY(hipMemsetAsync(cand_len, 0, (size_t)rows * 4, as_stream(stream))); return FZ_OK; }
    if (!fused || !cand_cols || !cand_vals || !cand_negpos) return FZ_ERR_ARG;
    if (n > 1024 * 28) return FZ_ERR_UNSUPPORTED;   // one workgroup holds the row (and positions stay exact in float32)
    SelectArgs a{fused, key_bits, pos, n, ld, k, cap, cand_cols, cand_vals, cand_negpos, cand_len, overflow};
    hipStream_t st = as_stream(stream);
#define FZ_SEL(TT, EE) { if (key_bits == 32) topk_select_kernel<TT, EE, 1><<<rows, TT, 0, st>>>(a); else topk_select_kernel<TT, EE, 2><<<rows, TT, 0, st>>>(a); }
    if (n <= 256 * 4) FZ_SEL(256, 4)
    else if (n <= 256 * 16) FZ_SEL(256, 16)
    else if (n <= 1024 * 16) FZ_SEL(1024, 16)
    else FZ_SEL(1024, 28)
#undef FZ_SEL
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

// ---- top-k: chunk-sort-truncate levels until one workgroup can finish the row ---------------
static const int TOPK_CHUNK = SORT_ROW_F64;   // the width both key widths share (the chunk sorts here have float32 keys: any width <= SORT_ROW_F32 would do)
extern "C" int fz_topk_max_k(void) { return 8192; }

// The chunk-sort-truncate levels of fz_topk_rows_f32, host arithmetic only: the entry runs the plan it gets from here and
// fz_topk_rows_plan shows it on a machine without a GPU (tests/topk_cases.py lands every branch below through it).
constexpr int TOPK_MAX_LEVELS = 12;   // k <= 8192: a level shrinks its row 3.5 times, 2^31 columns take 9
struct TopkLevel { int width, chunks, kk, fill; };
struct TopkPlan {
    int levels, pad, last;            // pad: n < k, the tail of the outputs is (-inf, -1); last: the width the finishing sort reads
    size_t elems;                     // candidates kept over all levels, per row
    TopkLevel lv[TOPK_MAX_LEVELS];
};
static TopkPlan topk_plan(int n, int k) {
    // level l: width columns -> chunks of TOPK_CHUNK -> kk = min(k, TOPK_CHUNK) survivors per chunk
    TopkPlan p{};
    p.pad = n < k ? 1 : 0;
    int cur = n;
    while (cur > SORT_ROW_F32 && p.levels < TOPK_MAX_LEVELS) {
        TopkLevel& l = p.lv[p.levels++];
        l.width = cur;
        l.chunks = (cur + TOPK_CHUNK - 1) / TOPK_CHUNK;
        l.kk = k < TOPK_CHUNK ? k : TOPK_CHUNK;
        l.fill = cur - (l.chunks - 1) * TOPK_CHUNK < l.kk ? 1 : 0;   // the short last chunk leaves a tail of its kk slots unwritten
        cur = l.chunks * l.kk;
        p.elems += (size_t)cur;
    }
    p.last = cur;
    return p;
}

// out[FZ_TOPK_ROWS_PLAN_FIELDS = 3 + 4 * 12]: levels, pad, last, then (width, chunks, kk, fill) of every level
extern "C" int fz_topk_rows_plan(int n, int k, int32_t* out) {
    if (n < 0 || k <= 0 || !out) return FZ_ERR_ARG;
    if (k > fz_topk_max_k()) return FZ_ERR_UNSUPPORTED;
    const TopkPlan p = topk_plan(n, k);
    if (p.last > SORT_ROW_F32) return FZ_ERR_UNSUPPORTED;
    out[0] = p.levels; out[1] = p.pad; out[2] = p.last;
    for (int l = 0; l < TOPK_MAX_LEVELS; ++l) {
        out[3 + 4 * l] = p.lv[l].width; out[4 + 4 * l] = p.lv[l].chunks; out[5 + 4 * l] = p.lv[l].kk; out[6 + 4 * l] = p.lv[l].fill;
    }
    return FZ_OK;
}

extern "C" size_t fz_topk_workspace_bytes(int rows, int n, int k) {
    if (rows <= 0 || n <= 0 || k <= 0) return 0;
    return (size_t)rows * topk_plan(n, k).elems * 8 + 256;  // fp32 score + int32 column per surviving candidate
}

extern "C" int fz_topk_rows_f32(const float* scores, int rows, int n, int ld, int k, int64_t id_base, float* out_scores,
                                int64_t* out_ids, void* workspace, size_t workspace_bytes, void* stream) {
    if (rows < 0 || n < 0 || ld < n || k <= 0) return FZ_ERR_ARG;
    if (k > fz_topk_max_k()) return FZ_ERR_UNSUPPORTED;
    if (rows == 0) return FZ_OK;
    if (!out_scores || !out_ids || (!scores && n > 0)) return FZ_ERR_ARG;
    const TopkPlan p = topk_plan(n, k);
    if (p.last > SORT_ROW_F32) return FZ_ERR_UNSUPPORTED;
    if (n > 0 && workspace_bytes < fz_topk_workspace_bytes(rows, n, k)) return FZ_ERR_WORKSPACE;
    if (n > SORT_ROW_F32 && !workspace) return FZ_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    const int have = n < k ? n : k;
    if (p.pad) {
        dim3 g((unsigned)((k - have + 255) / 256), (unsigned)rows);
        topk_pad_kernel<<<g, 256, 0, st>>>(out_scores, out_ids, rows, k, have);
        FZ_LAUNCH_CHECK();
    }
    if (n == 0) return FZ_OK;

    const float* cur_keys = scores;
    const int32_t* cur_cols = nullptr;
    long cur_stride = ld;
    char* ws = reinterpret_cast<char*>(workspace);
    for (int l = 0; l < p.levels; ++l) {
        const TopkLevel& lv = p.lv[l];
        const int next = lv.chunks * lv.kk;
        float* nk = reinterpret_cast<float*>(ws); ws += (size_t)rows * next * 4;
        int32_t* nc = reinterpret_cast<int32_t*>(ws); ws += (size_t)rows * next * 4;
        if (lv.fill) {
            // the short last chunk leaves a tail unwritten: make it (-inf, col -1) so it cannot win
            fill_absent_kernel<float><<<1024, 256, 0, st>>>(nk, nc, (size_t)rows * next);
            FZ_LAUNCH_CHECK();
        }
        SortArgs a{};
        a.keys = cur_keys; a.n_total = lv.width; a.key_row_stride = cur_stride; a.seg_len = lv.width; a.chunks = lv.chunks; a.chunk_len = TOPK_CHUNK;
        a.order = nc; a.sorted_keys = nk; a.out_row_stride = next; a.out_chunk_stride = lv.kk; a.out_limit = lv.kk;
        a.colmap = cur_cols; a.colmap_row_stride = cur_stride;
        int rc = launch_sort(a, 1, rows * lv.chunks, TOPK_CHUNK, st);
        if (rc != FZ_OK) return rc;
        cur_keys = nk; cur_cols = nc; cur_stride = next;
    }
    SortArgs a{};
    a.keys = cur_keys; a.n_total = p.last; a.key_row_stride = cur_stride; a.seg_len = p.last; a.chunks = 1; a.chunk_len = p.last;
    a.sorted_keys = out_scores; a.out_ids = out_ids; a.id_base = id_base; a.out_row_stride = k; a.out_limit = have;
    a.colmap = cur_cols; a.colmap_row_stride = cur_stride;
    return launch_sort(a, 1, rows, p.last, st);
}

extern "C" size_t fz_topk_update_workspace_bytes(int rows, int k, int cap) {
    if (rows <= 0 || k <= 0 || cap <= 0) return 0;
    return (size_t)rows * (k + cap) * (4 + 8) + (size_t)rows * 4 + 256;
}

/* One streaming step of the chunked top-k (sentence_transformers.py:346-364): merge a new chunk of scores into the
 * running per-row top-k.  run_* [rows][k] in, new_* [rows][k] out (distinct buffers).  *overflow (device int32,
 * zeroed by the caller) becomes 1 if some row had more than `cap` candidates above its running threshold: the caller
 * must then redo this chunk with fz_topk_rows_f32 + fz_topk_merge (exact, slower).  k + cap <= 35840. */
extern "C" int fz_topk_update_f32(const float* scores, int rows, int n, int ld, int64_t id_base, const float* run_scores,
                                  const int64_t* run_ids, int k, int cap, float* new_scores, int64_t* new_ids, int32_t* overflow,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (rows < 0 || n < 0 || ld < n || k <= 0 || cap <= 0) return FZ_ERR_ARG;
    if ((long)k + cap > SORT_ROW_F32) return FZ_ERR_UNSUPPORTED;
    if (rows == 0) return FZ_OK;                   // empty tensors carry null pointers
    if (!run_scores || !run_ids || !new_scores || !new_ids || !overflow || (!scores && n > 0)) return FZ_ERR_ARG;
    if (!workspace || workspace_bytes < fz_topk_update_workspace_bytes(rows, k, cap)) return FZ_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    FilterArgs f{};
    f.scores = scores; f.n = n; f.ld = ld; f.id_base = id_base; f.run_scores = run_scores; f.run_ids = run_ids; f.k = k; f.cap = cap;
    f.buf_ids = reinterpret_cast<int64_t*>(ws); ws += (size_t)rows * (k + cap) * 8;
    f.buf_scores = reinterpret_cast<float*>(ws); ws += (size_t)rows * (k + cap) * 4;
    f.buf_len = reinterpret_cast<int32_t*>(ws);
    f.overflow = overflow;
    topk_filter_kernel<<<rows, 256, 0, st>>>(f);
    FZ_LAUNCH_CHECK();
    SortArgs a = id_rows(f.buf_scores, f.buf_ids, k + cap, new_scores, new_ids, k);
    a.row_len = f.buf_len;
    return launch_sort(a, 1, rows, k + cap, st);
}

/* The streaming step in two halves, so that several chunks can share one sort: fz_topk_filter_append_f32 appends the chunk's
 * scores above tau[row] (or NaN) to the row's candidate list (ascending id inside the chunk; chunks must be fed in ascending id
 * order); fz_topk_fold_f32 merges [running k | candidates] into the new running list, writes the new threshold
 * tau[row] = k-th best and empties the candidate lists.  cand_* [rows][cap], cand_len [rows] (zeroed before the first call). */
extern "C" int fz_topk_filter_append_f32(const float* scores, int rows, int n, int ld, int64_t id_base, const float* tau, float* cand_scores,
                                         int64_t* cand_ids, int32_t* cand_len, int cap, int32_t* overflow, void* stream) {
    if (rows < 0 || n < 0 || ld < n || cap <= 0) return FZ_ERR_ARG;
    if (rows == 0 || n == 0) return FZ_OK;
    if (!scores || !tau || !cand_scores || !cand_ids || !cand_len || !overflow) return FZ_ERR_ARG;
    FilterArgs f{};
    f.scores = scores; f.n = n; f.ld = ld; f.id_base = id_base; f.k = 0; f.cap = cap; f.tau = tau;
    f.buf_scores = cand_scores; f.buf_ids = cand_ids; f.buf_len = cand_len; f.overflow = overflow;
    topk_filter_kernel<<<rows, 256, 0, as_stream(stream)>>>(f);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

// Candidates that arrive in no particular order (the GEMM's filter epilogue appends them as its waves finish): the score sort is
// stable, so equal scores come out in ARRIVAL order.  The sort therefore writes the first k + TIE_MARGIN entries to a scratch
// list and this pass puts every run of equal scores that reaches into the first k into ascending id order (running-list entries
// have smaller ids than any later candidate, so they stay in front).  A run still open at the end of the scratch list, or longer
// than TIE_RUN_MAX, sets *overflow: the caller redoes the search on the exact path.
constexpr int TIE_MARGIN = 64, TIE_RUN_MAX = 512;

__global__ __launch_bounds__(256) void topk_tiefix_kernel(const float* tmp_s, const int64_t* tmp_i, const int32_t* buf_len, int k, int stride,
                                                          float* out_s, int64_t* out_i, int32_t* overflow) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tie_lds[];
    int64_t* li = reinterpret_cast<int64_t*>(tie_lds);                 // [stride]
    uint32_t* lk = reinterpret_cast<uint32_t*>(li + stride);           // [stride] sort keys of the scores (NaN == NaN, -0 == +0)
    const int row = blockIdx.x;
    const int have = buf_len[row];
    const int L = min(have, stride);
    const float* ts = tmp_s + (size_t)row * stride;
    const int64_t* ti = tmp_i + (size_t)row * stride;
    for (int p = threadIdx.x; p < L; p += blockDim.x) { lk[p] = desc_key_f32(ts[p]); li[p] = ti[p]; }
    __syncthreads();
    float* os = out_s + (size_t)row * k;
    int64_t* oi = out_i + (size_t)row * k;
    bool bad = false;
    for (int p = threadIdx.x; p < max(L, k); p += blockDim.x) {
        if (p >= L) { if (p < k) { os[p] = -INFINITY; oi[p] = -1; } continue; }      // short list: (-inf, -1) padding
        const uint32_t key = lk[p];
        int a = p, b = p + 1;
        while (a > 0 && lk[a - 1] == key && p - a < TIE_RUN_MAX) --a;
        if (a >= k) continue;                                                        // the run lies entirely behind the cut
        while (b < L && lk[b] == key && b - p < TIE_RUN_MAX) ++b;
        if ((a > 0 && lk[a - 1] == key) || (b < L && lk[b] == key) || (b == L && have > L)) { bad = true; continue; }
        const int64_t id = li[p];
        int rank = 0;
        for (int j = a; j < b; ++j) rank += (li[j] < id) || (li[j] == id && j < p);
        const int dst = a + rank;
        if (dst < k) { os[dst] = ts[p]; oi[dst] = id; }
    }
    if (bad) atomicExch(overflow, 1);
}

// The largest k fz_topk_fold_f32 takes: the unordered form holds the first k + TIE_MARGIN entries of a row in LDS (12 bytes each, 60 KiB);
// the ordered form is bound by k + cap <= one sort row alone.
constexpr size_t TIE_LDS_MAX = 60 * 1024;
extern "C" int fz_topk_fold_max_k(int unordered) { return unordered ? (int)(TIE_LDS_MAX / (8 + 4)) - TIE_MARGIN : SORT_ROW_F32 - 1; }

extern "C" size_t fz_topk_fold_workspace_bytes(int rows, int k, int cap) {
    if (rows <= 0 || k <= 0 || cap <= 0) return 0;
    return fz_topk_update_workspace_bytes(rows, k, cap) + (size_t)rows * (k + TIE_MARGIN) * (4 + 8) + 256;
}

extern "C" int fz_topk_fold_f32(const float* run_scores, const int64_t* run_ids, int rows, int k, const float* cand_scores, const int64_t* cand_ids,
                                int32_t* cand_len, int cap, int unordered, float* new_scores, int64_t* new_ids, float* tau_out, int32_t* overflow,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (rows < 0 || k <= 0 || cap <= 0) return FZ_ERR_ARG;
    if ((long)k + cap > SORT_ROW_F32 || k > fz_topk_fold_max_k(unordered)) return FZ_ERR_UNSUPPORTED;   // (before any launch: a refusal leaves everything as it was)
    if (rows == 0) return FZ_OK;
    if (!run_scores || !run_ids || !cand_scores || !cand_ids || !cand_len || !new_scores || !new_ids || (unordered && !overflow)) return FZ_ERR_ARG;
    if (!workspace || workspace_bytes < fz_topk_fold_workspace_bytes(rows, k, cap)) return FZ_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    int64_t* buf_ids = reinterpret_cast<int64_t*>(ws); ws += (size_t)rows * (k + cap) * 8;
    int64_t* tmp_ids = reinterpret_cast<int64_t*>(ws); ws += (size_t)rows * (k + TIE_MARGIN) * 8;
    float* buf_scores = reinterpret_cast<float*>(ws); ws += (size_t)rows * (k + cap) * 4;
    float* tmp_scores = reinterpret_cast<float*>(ws); ws += (size_t)rows * (k + TIE_MARGIN) * 4;
    int32_t* buf_len = reinterpret_cast<int32_t*>(ws);
    topk_concat_kernel<<<rows, 256, 0, st>>>(run_scores, run_ids, k, cand_scores, cand_ids, cand_len, cap, buf_scores, buf_ids, buf_len);
    FZ_LAUNCH_CHECK();
    const int lim = unordered ? k + TIE_MARGIN : k;
    SortArgs a = id_rows(buf_scores, buf_ids, k + cap, unordered ? tmp_scores : new_scores, unordered ? tmp_ids : new_ids, lim);
    a.row_len = buf_len;
    if (int rc = launch_sort(a, 1, rows, k + cap, st)) return rc;
    if (unordered) {
        const size_t lds = (size_t)lim * (8 + 4);                  // <= TIE_LDS_MAX: k <= fz_topk_fold_max_k(1)
        topk_tiefix_kernel<<<rows, 256, lds, st>>>(tmp_scores, tmp_ids, buf_len, k, lim, new_scores, new_ids, overflow);
        FZ_LAUNCH_CHECK();
    }
    topk_fold_done_kernel<<<(rows + 255) / 256, 256, 0, st>>>(new_scores, rows, k, tau_out, cand_len);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_topk_merge(const float* in_scores, const int64_t* in_ids, int G, int rows, int k, float* out_scores,
                             int64_t* out_ids, void* stream) {
    if (G <= 0 || rows < 0 || k <= 0) return FZ_ERR_ARG;
    if (rows != 0 && (!in_scores || !in_ids || !out_scores || !out_ids)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if ((long)G * k > SORT_ROW_F32) return FZ_ERR_UNSUPPORTED;
    if (rows == 0) return FZ_OK;
    SortArgs a = id_rows(in_scores, in_ids, G * k, out_scores, out_ids, k);
    a.key_row_stride = k; a.seg_len = k; a.seg_stride = (long)rows * k;   // the G lists of a row lie a whole [rows][k] plane apart
    return launch_sort(a, 1, rows, G * k, as_stream(stream));
}
