// feedback.hip -- pseudo-relevance feedback (Rocchio): the step between a first search and the second (gfx950).
//
// The first few documents of a query's own top-k list move the query towards them: q' = alpha * q + sum_r coef[r] * d_r over the
// feedback slots r = 0 .. F-1 IN SLOT ORDER.  A slot is skipped when r >= fb_len[q] or its id is not one of this index's N documents
// (id_base .. id_base + N - 1); the same document in two slots is added twice.  Every product and every add is rounded to float32
// once (-ffp-contract=off), and a term's (a dimension's) contributions are always added in slot order: the bits are defined, and two
// runs give the same bytes.  No float atomics anywhere.
//
// sparse_feedback_kernel: ONE 1,024-THREAD WORKGROUP PER QUERY over a forward index (forward.hip's rows of {term, weight bits}).
//   LDS: the accumulator acc [32 * words] float32 over the vocabulary (words = ceil(V / 32); 128 KiB at V = 32,768), a touched bitmap
//   and a query-term bitmap [words] each, the offsets, lengths and coefficients of 256 slots (4 KiB), a 256-bin histogram and 16 wave
//   totals: 141.1 KiB at the cap, one workgroup per CU.  Only the words V needs are cleared.
//   1. acc[t] = +0.0 + alpha * w for the query's terms (unique: one writer per address), their bits set in the query bitmap.
//   2. the slot loop.  Thread i resolves slot i once (id -> document -> row offsets into LDS): two dependent global reads for all the
//      slots together, not per slot.  Then thread i takes posting i (+ 1,024 j) of a slot's row: acc[t] = acc[t] + coef * w -- a row's
//      terms are unique, so a plain LDS read-modify-write has one writer per address -- and sets the term's touched bit (an integer
//      LDS atomic OR).  A barrier between slots keeps a term's additions in slot order; the first 1,024 postings of eight rows are
//      loaded together ahead of their adds (plain loads stay in flight across __syncthreads()), so F slots cost F / 8 memory latencies.
//   3. selection of the min(m, C) best of the C candidates (touched and not a query term) by desc_key_f32(acc) ascending, ties by
//      ascending term.  The candidates are read through the bitmap words, once: a wave takes 64 words, two at a time, lane = (word
//      parity, bit) -- 64 consecutive accumulator words per read, across all banks -- and a lane keeps its 32 keys in registers.  The
//      threshold key is found by four 8-bit histogram passes over them (skipped when every candidate is kept); keys below it are in,
//      and of the ties AT it the lowest terms are, by a block scan of the per-word tie counts.
//   4. emission in ascending term order: thread i owns bitmap word i (words <= 1,024); a block scan of the per-word popcounts of
//      (query terms | admitted candidates) gives its first column.  The rest of the row up to `width` gets (-1, +0.0): the kernel
//      writes every element of its rows and nothing else.  A row that does not fit `width` raises bit 0 of the flag word and is cut.
//
// dense_feedback_kernel: one 256-thread workgroup per query, a thread owns four (VEC = 4: float4 loads where the strides and pointers
//   allow) or one (VEC = 1) dimensions at a time: out = alpha * Qn, then out = out + coef * Dn[d] slot after slot in registers, four row
//   loads in flight.  A skipped slot loads row 0 and keeps the old value by a select (a uniform branch around each load would put a
//   full wait behind every one of them).  No LDS, no barrier.
//
// Where it stands: DESIGN.md section 'Pseudo-relevance feedback'.
#include "common.h"

namespace fz {

constexpr int FB_T = 1024;                 // threads of the sparse kernel = bitmap words it can own = postings per row chunk
constexpr int FB_NW = FB_T / 64;
constexpr int FB_MAX_V = 32 * FB_T;        // fz_sparse_feedback_max_vocab(): 128 KiB of accumulator
constexpr int FB_BINS = 256;
constexpr int FB_SLOTS = 256;              // slots resolved at a time (thread i: slot i), their rows' offsets kept in LDS
constexpr int FB_U = 8;                    // rows whose first postings are in flight together
constexpr int32_t FB_OVERFLOW = 1;         // the flag word's bit 0: a row did not fit `width`
constexpr int FBD_T = 256;                 // threads of the dense kernel
constexpr int FBD_U = 4;                   // its row loads in flight

struct FbSlots {                           // the feedback lists, shared by both kernels
    const int64_t* fb_ids;                 // [Q][ldf]
    const int32_t* fb_len;                 // [Q] or null (= F everywhere)
    const float* coef;                     // [Q][ldc]
    int64_t N, id_base;
    int F, ldf, ldc;
};

// the slots of query q that can count: min(max(fb_len, 0), F); none without documents
__device__ __forceinline__ int fb_slots(const FbSlots& s, int q) {
    if (s.N <= 0) return 0;
    return s.fb_len ? min(max(s.fb_len[q], 0), s.F) : s.F;
}
// id -> the document's position, or -1 for an id outside [id_base, id_base + N)
__device__ __forceinline__ int64_t fb_doc(const FbSlots& s, int64_t id) {
    const uint64_t d = (uint64_t)id - (uint64_t)s.id_base;
    return (id >= s.id_base && d < (uint64_t)s.N) ? (int64_t)d : -1;
}

struct SparseFbArgs {
    FbSlots s;
    const int64_t* foff; const int2* rows;                         // row of document d: postings [foff[d], foff[d+1]), {term, weight bits}
    const int64_t* qoff; const int32_t* qterms; const float* qw;   // query q: terms [qoff[q], qoff[q+1]), unique and ascending
    int32_t* out_terms; float* out_w; int32_t* out_len; int32_t* flag;
    int V, ldo, width, m;
    float alpha;
};

// exclusive prefix of v over the workgroup's threads and the total; two barriers: wtot is free again on return
__device__ __forceinline__ uint32_t fb_block_scan(uint32_t v, uint32_t* wtot, int lane, int wv, uint32_t& total) {
    const uint32_t incl = wave_incl_scan_u32(v, lane);
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    uint32_t woff = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < FB_NW; ++i) { const uint32_t c = wtot[i]; if (i < wv) woff += c; total += c; }
    __syncthreads();
    return woff + incl - v;
}

__global__ __launch_bounds__(FB_T) void sparse_feedback_kernel(SparseFbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fb_smem[];
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int words = (a.V + 31) >> 5;                             // <= FB_T
    float* const acc = reinterpret_cast<float*>(fb_smem);          // [32 * words]
    int64_t* const s_start = reinterpret_cast<int64_t*>(acc + 32 * words);  // [FB_SLOTS] (8-byte aligned: 128 B per word before it)
    uint32_t* const hist = reinterpret_cast<uint32_t*>(s_start + FB_SLOTS);  // [FB_BINS], 16-byte aligned: read as uint4
    uint32_t* const wtot = hist + FB_BINS;                         // [FB_NW]
    int* const s_len = reinterpret_cast<int*>(wtot + FB_NW);       // [FB_SLOTS]
    float* const s_coef = reinterpret_cast<float*>(s_len + FB_SLOTS);       // [FB_SLOTS]
    uint32_t* const touched = reinterpret_cast<uint32_t*>(s_coef + FB_SLOTS);   // [words]
    uint32_t* const qbits = touched + words;                       // [words]

    for (int i = t; i < 8 * words; i += FB_T) reinterpret_cast<float4*>(acc)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t < words) { touched[t] = 0u; qbits[t] = 0u; }
    __syncthreads();

    // 1. the query's own terms
    {
        const int64_t q0 = a.qoff[q], nq = a.qoff[q + 1] - q0;
        for (int64_t p = t; p < nq; p += FB_T) {
            const int term = a.qterms[q0 + p];
            if ((unsigned)term < (unsigned)a.V) {
                acc[term] = acc[term] + a.alpha * a.qw[q0 + p];
                atomicOr(&qbits[term >> 5], 1u << (term & 31));
            }
        }
    }

    // 2. the feedback documents, slot after slot
    const int flen = fb_slots(a.s, q);
    for (int s0 = 0; s0 < flen; s0 += FB_SLOTS) {                  // block-uniform
        // thread i resolves slot s0 + i: id -> document -> row offsets, two dependent reads for ALL the slots of the chunk at once
        if (t < FB_SLOTS) {
            int64_t st = 0; int len = 0; float c = 0.0f;
            if (s0 + t < flen) {
                const int64_t d = fb_doc(a.s, a.s.fb_ids[(size_t)q * a.s.ldf + s0 + t]);
                c = a.s.coef[(size_t)q * a.s.ldc + s0 + t];
                if (d >= 0) { st = a.foff[d]; len = (int)min(max(a.foff[d + 1] - st, (int64_t)0), (int64_t)0x7fffffff); }
            }
            s_start[t] = st; s_len[t] = len; s_coef[t] = c;
        }
        __syncthreads();                                           // (closes step 1 as well)
        const int n = min(flen - s0, FB_SLOTS);
        for (int r0 = 0; r0 < n; r0 += FB_U) {                     // FB_U rows' first 1,024 postings in flight, added in slot order
            int2 p[FB_U];
#pragma unroll
            for (int u = 0; u < FB_U; ++u) {
                p[u] = make_int2(-1, 0);                           // no term
                if (r0 + u < n && t < s_len[r0 + u]) p[u] = a.rows[s_start[r0 + u] + t];
            }
#pragma unroll
            for (int u = 0; u < FB_U; ++u) {
                if (r0 + u < n) {                                  // block-uniform
                    const float c = s_coef[r0 + u];
                    if ((unsigned)p[u].x < (unsigned)a.V) {
                        acc[p[u].x] = acc[p[u].x] + c * __int_as_float(p[u].y);
                        atomicOr(&touched[p[u].x >> 5], 1u << (p[u].x & 31));
                    }
                    const int len = s_len[r0 + u];
                    for (int k = t + FB_T; k < len; k += FB_T) {   // a row of more than 1,024 postings
                        const int2 pk = a.rows[s_start[r0 + u] + k];
                        if ((unsigned)pk.x < (unsigned)a.V) {
                            acc[pk.x] = acc[pk.x] + c * __int_as_float(pk.y);
                            atomicOr(&touched[pk.x >> 5], 1u << (pk.x & 31));
                        }
                    }
                    __syncthreads();                               // this slot's adds are in before the next slot's read them
                }
            }
        }
    }
    __syncthreads();

    // 3. the threshold key of the best `keep` candidates.  A wave takes 64 bitmap words, two at a time: lane = (word parity, bit), so
    // the accumulator is read 64 consecutive words at a time; the 32 keys of a lane stay in registers for all the passes below
    const int b = lane & 31, wbase = wv * 64 + (lane >> 5);
    uint32_t key[32], ism = 0u;                                    // ism bit i: the lane's bit of word wbase + 2 i is a candidate
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int w = wbase + 2 * i;
        const uint32_t cm = w < words ? touched[w] & ~qbits[w] : 0u;
        const bool is = (cm >> b) & 1u;
        key[i] = desc_key_f32(is ? acc[w * 32 + b] : 0.0f);        // w < words: inside the accumulator
        ism |= (is ? 1u : 0u) << i;
    }
    uint32_t ncand;
    fb_block_scan((uint32_t)__popc(ism), wtot, lane, wv, ncand);
    const uint32_t keep = min((uint32_t)a.m, ncand);
    uint32_t prefix = 0u, rem = keep;                              // keep == 0: no key is below 0, no tie is admitted
    if (keep == ncand) {                                           // every candidate: all keys are below this one (only -NaN reaches it)
        prefix = 0xffffffffu; rem = 0u;
    } else if (keep > 0u) {                                        // (block-uniform)
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (t < FB_BINS) hist[t] = 0u;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 32; ++i)
                if (((ism >> i) & 1u) && (pass == 0 || (key[i] >> ((shift + 8) & 31)) == prefix)) atomicAdd(&hist[(key[i] >> shift) & 255u], 1u);
            __syncthreads();
            // every wave finds the bin that holds the rem-th key itself: lane l sums bins 4 l .. 4 l + 3 (at least rem keys are counted)
            const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];
            const uint32_t s = h.x + h.y + h.z + h.w;
            const uint32_t incl = wave_incl_scan_u32(s, lane);
            const unsigned long long reach = __ballot(incl >= rem);
            const int src = reach ? __builtin_ctzll(reach) : 63;
            uint32_t below = __shfl(incl - s, src);
            const uint32_t hx = __shfl(h.x, src), hy = __shfl(h.y, src), hz = __shfl(h.z, src);
            uint32_t bin = 4u * (uint32_t)src;
            if (rem > below + hx) {
                below += hx; ++bin;
                if (rem > below + hy) {
                    below += hy; ++bin;
                    if (rem > below + hz) { below += hz; ++bin; }
                }
            }
            rem -= below;                                          // still >= 1: the rem-th key lies in this bin
            prefix = (prefix << 8) | bin;
            __syncthreads();                                       // the bins are read before the next pass clears them
        }
    }
    // keys below the threshold are in; `rem` of the keys AT it are, the lowest terms first.  From here thread i owns bitmap word i:
    // lanes 2 i and 2 i + 1 of a wave take the two halves of pair i's ballots
    uint32_t myless = 0u, mytie = 0u;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const bool is = (ism >> i) & 1u;
        const unsigned long long bl = __ballot(is && key[i] < prefix), bt = __ballot(is && key[i] == prefix);
        if ((lane >> 1) == i) {
            myless = (lane & 1) ? (uint32_t)(bl >> 32) : (uint32_t)bl;
            mytie = (lane & 1) ? (uint32_t)(bt >> 32) : (uint32_t)bt;
        }
    }
    uint32_t nties;
    const uint32_t tbefore = fb_block_scan((uint32_t)__popc(mytie), wtot, lane, wv, nties);
    uint32_t adm = 0u;
    if (rem > tbefore) {
        uint32_t left = rem - tbefore, mm = mytie;
        while (left != 0u && mm != 0u) { adm |= mm & (0u - mm); mm &= mm - 1u; --left; }
    }

    // 4. the expanded query in ascending term order
    uint32_t outm = (t < words ? qbits[t] : 0u) | myless | adm;
    uint32_t total;
    uint32_t pos = fb_block_scan((uint32_t)__popc(outm), wtot, lane, wv, total);
    int32_t* const orow_t = a.out_terms + (size_t)q * a.ldo;
    float* const orow_w = a.out_w + (size_t)q * a.ldo;
    for (; outm != 0u; outm &= outm - 1u, ++pos) {
        const int term = t * 32 + __builtin_ctz(outm);             // a set bit: term < V, word t < words
        if (pos < (uint32_t)a.width) { orow_t[pos] = term; orow_w[pos] = acc[term]; }
    }
    for (uint32_t c = min(total, (uint32_t)a.width) + t; c < (uint32_t)a.width; c += FB_T) { orow_t[c] = -1; orow_w[c] = 0.0f; }
    if (t == 0) {
        a.out_len[q] = (int32_t)total;
        if (total > (uint32_t)a.width) atomicOr(a.flag, FB_OVERFLOW);
    }
}

struct DenseFbArgs {
    FbSlots s;
    const float* Qn; const float* Dn; float* out;
    int ldq, ldd, ldo, dim;
    float alpha;
};

template <int VEC>
__global__ __launch_bounds__(FBD_T) void dense_feedback_kernel(DenseFbArgs a) {
    const int q = blockIdx.x, t = threadIdx.x;
    const int flen = fb_slots(a.s, q);
    const int64_t* const ids = a.s.fb_ids + (size_t)q * a.s.ldf;
    const float* const cf = a.s.coef + (size_t)q * a.s.ldc;
    const float* const qrow = a.Qn + (size_t)q * a.ldq;
    float* const orow = a.out + (size_t)q * a.ldo;
    const int groups = (a.dim + VEC - 1) / VEC;
    for (int g = t; g < groups; g += FBD_T) {
        const int j = g * VEC;
        const bool whole = j + VEC <= a.dim;                       // only the last group of a row can be short
        auto load = [&](const float* p, float (&v)[VEC]) __attribute__((always_inline)) {
            if constexpr (VEC == 4) {
                if (whole) {
                    const float4 x = *reinterpret_cast<const float4*>(p + j);
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                    return;
                }
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = j + e < a.dim ? p[j + e] : 0.0f;
        };
        float o[VEC];
        load(qrow, o);
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = a.alpha * o[e];
        for (int r0 = 0; r0 < flen; r0 += FBD_U) {                 // (flen > 0: N >= 1, row 0 exists)
            float x[FBD_U][VEC], c[FBD_U];
            bool on[FBD_U];
#pragma unroll
            for (int u = 0; u < FBD_U; ++u) {
                const int r = min(r0 + u, flen - 1);
                const int64_t d = fb_doc(a.s, ids[r]);
                on[u] = r0 + u < flen && d >= 0;
                c[u] = cf[r];
                load(a.Dn + (size_t)(d >= 0 ? d : 0) * a.ldd, x[u]);
            }
#pragma unroll
            for (int u = 0; u < FBD_U; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float sum = o[e] + c[u] * x[u][e];
                    o[e] = on[u] ? sum : o[e];
                }
        }
        if constexpr (VEC == 4) {
            if (whole) {
                *reinterpret_cast<float4*>(orow + j) = make_float4(o[0], o[1], o[2], o[3]);
                continue;
            }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (j + e < a.dim) orow[j + e] = o[e];
    }
}

// the checks both entry points make on the feedback lists
static int fb_slot_args(FbSlots& s, const int64_t* fb_ids, int ldf, const int32_t* fb_len, const float* coef, int ldc, int F, int Q, int64_t N,
                        int64_t id_base) {
    if (Q < 0 || N < 0 || F < 0 || ldf < F || ldc < F) return FZ_ERR_ARG;
    if (Q != 0 && F != 0 && (!fb_ids || !coef)) return FZ_ERR_ARG;
    s.fb_ids = fb_ids; s.fb_len = fb_len; s.coef = coef; s.N = N; s.id_base = id_base; s.F = F; s.ldf = ldf; s.ldc = ldc;
    return FZ_OK;
}

}  // namespace fz

using namespace fz;

extern "C" int fz_sparse_feedback_max_vocab(void) { return FB_MAX_V; }

extern "C" int fz_sparse_feedback_f32(const int64_t* foff, const void* rows, int V, int64_t N, int64_t id_base, const int64_t* qoff,
                                      const int32_t* qterms, const float* qw, int Q, const int64_t* fb_ids, int ldf, const int32_t* fb_len,
                                      const float* coef, int ldc, int F, float alpha, int m, int32_t* out_terms, float* out_w, int ldo,
                                      int width, int32_t* out_len, int32_t* flag, void* stream) {
    SparseFbArgs a{};
    if (int rc = fb_slot_args(a.s, fb_ids, ldf, fb_len, coef, ldc, F, Q, N, id_base)) return rc;
    if (V <= 0 || V > FB_MAX_V || m < 0 || width < 0 || ldo < width) return FZ_ERR_ARG;
    if (Q != 0 && (!qoff || !out_len || !flag || (width != 0 && (!out_terms || !out_w)) || (F != 0 && N != 0 && !foff))) return FZ_ERR_ARG;
    if ((uintptr_t)rows % 8) return FZ_ERR_UNSUPPORTED;
    if (Q == 0) return FZ_OK;
    a.foff = foff; a.rows = static_cast<const int2*>(rows); a.qoff = qoff; a.qterms = qterms; a.qw = qw;
    a.out_terms = out_terms; a.out_w = out_w; a.out_len = out_len; a.flag = flag;
    a.V = V; a.ldo = ldo; a.width = width; a.m = m; a.alpha = alpha;
    const size_t words = (size_t)(V + 31) / 32;
    const size_t lds = words * 32 * sizeof(float) + 2 * words * sizeof(uint32_t) + (FB_BINS + FB_NW) * sizeof(uint32_t) + FB_SLOTS * 16;
    hipStream_t st = as_stream(stream);
    static unsigned long long done = 0ull;
    if (lds > 48 * 1024)
        if (int rc = raise_lds_limit((const void*)sparse_feedback_kernel, 160 * 1024, done)) return rc;
    FZ_HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    sparse_feedback_kernel<<<Q, FB_T, lds, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_dense_feedback_f32(const float* Qn, int ldq, const float* Dn, int ldd, int Q, int64_t N, int dim, int64_t id_base,
                                     const int64_t* fb_ids, int ldf, const int32_t* fb_len, const float* coef, int ldc, int F, float alpha,
                                     float* out, int ldo, void* stream) {
    DenseFbArgs a{};
    if (int rc = fb_slot_args(a.s, fb_ids, ldf, fb_len, coef, ldc, F, Q, N, id_base)) return rc;
    if (dim <= 0 || ldq < dim || ldd < dim || ldo < dim) return FZ_ERR_ARG;
    if (Q != 0 && (!Qn || !out || (F != 0 && N != 0 && !Dn))) return FZ_ERR_ARG;
    if (Q == 0) return FZ_OK;
    a.Qn = Qn; a.Dn = Dn; a.out = out; a.ldq = ldq; a.ldd = ldd; a.ldo = ldo; a.dim = dim; a.alpha = alpha;
    const bool vec = ldq % 4 == 0 && ldd % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)Qn | (uintptr_t)Dn | (uintptr_t)out) % 16 == 0;
    hipStream_t st = as_stream(stream);
    if (vec) dense_feedback_kernel<4><<<Q, FBD_T, 0, st>>>(a);
    else dense_feedback_kernel<1><<<Q, FBD_T, 0, st>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
