// crosspack.hip -- what feeds the cross-encoder's packed forward when the candidates arrive as top-k lists of global ids: the (query,
// document) pair rows "<s> q </s></s> d </s>" assembled on the device from token ids, with no strings and no padded id matrix.
//
//   fz_pair_plan   one thread per slot of the [Q, W] candidate plane: is the slot this shard's (pairs.h), and if so how many query and
//                  document tokens the pair keeps under the tokenizer's truncation rule, and how many rows L the pair takes.
//   fz_pair_fill   one wave per pair of ONE forward sub-batch: ids[T] and pos_ids[T], the two vectors fz_embed_layernorm_f32 takes.
//
// The pair rule is stated once, in pair_keep() below; tests/crosspack_cases.py restates it in numpy and pins it against the installed
// tokenizer.  Integer work only: no LDS, no atomics, no workspace, no host synchronisation inside either entry.
//
// Where it stands: DESIGN.md section 'Cross-encoder rerank over top-k lists'.
#include "pairs.h"

namespace fz {

constexpr int CP_THREADS = 256;
constexpr int CP_WAVES = CP_THREADS / FZ_WAVE;
constexpr int CP_MAX_SEP = 2;                          // separators between the two sequences: 2 (RoBERTa "</s></s>"), 1 (BERT, the hash tokenizer), 0

// The kept token counts of a pair.  lq / ld: the plain lengths of the two sequences BEFORE any cut; B = max_length - (2 + nsep).
//   FZ_PAIR_LONGEST_FIRST  the `tokenizers` library's TruncationStrategy::LongestFirst: if the pair does not fit, the shorter sequence
//                          keeps n1 = min and the longer max(n1, B - n1); if that still does not fit, both take half (the odd token to
//                          the STRICTLY longer one, to the document on a tie).  All nsep separators are always kept.
//   FZ_PAIR_TAIL           one row "q sep.. d" cut at max_length - 2: the separators are ordinary tokens and go before the document does.
__device__ __forceinline__ void pair_keep(int mode, int B, int nsep, int lq, int ld, int& kq, int& ks, int& kd) {
    if (mode == FZ_PAIR_TAIL) {
        const int M = B + nsep;
        kq = lq < M ? lq : M;
        ks = nsep < M - kq ? nsep : M - kq;
        kd = ld < M - kq - ks ? ld : M - kq - ks;
        return;
    }
    ks = nsep;
    if ((int64_t)lq + ld <= B) { kq = lq; kd = ld; return; }
    int64_t n1 = lq < ld ? lq : ld;
    int64_t n2 = n1 > B - n1 ? n1 : B - n1;
    if (n1 + n2 > B) { n1 = B / 2; n2 = n1 + B % 2; }
    const bool query_longer = lq > ld;
    kq = (int)(query_longer ? n2 : n1);
    kd = (int)(query_longer ? n1 : n2);
}

struct PairPlanArgs {
    const int64_t* cand; const int32_t* cand_len; const int64_t* Doff; const int32_t* dfull; const int32_t* qlen;
    int32_t* kq; int32_t* kd; int32_t* L;
    int64_t id_base;
    int ldc, Q, W, N, Lq, B, mode, nsep;
};

__global__ __launch_bounds__(CP_THREADS) void pair_plan_kernel(const PairPlanArgs a) {
    const int64_t slot = (int64_t)blockIdx.x * CP_THREADS + threadIdx.x;
    if (slot >= (int64_t)a.Q * a.W) return;
    const int q = (int)(slot / a.W), r = (int)(slot - (int64_t)q * a.W);
    int kq = 0, ks = 0, kd = 0, L = 0;
    const int d = pair_position(a.cand, a.ldc, a.cand_len, a.id_base, a.N, a.W, q, r);
    if (d >= 0) {                                      // nothing is read for a slot that is not this shard's
        const int64_t held64 = a.Doff[d + 1] - a.Doff[d];
        const int held = held64 < 0 ? 0 : held64 > 0x7fffffff ? 0x7fffffff : (int)held64;
        int ld = a.dfull ? a.dfull[d] : held;          // the length before the store's cut decides who is "longer"
        ld = ld < held ? held : ld;
        int lq = a.qlen[q];
        lq = lq < 0 ? 0 : lq;
        pair_keep(a.mode, a.B, a.nsep, lq, ld, kq, ks, kd);
        kq = kq < a.Lq ? kq : a.Lq;                    // never past what is stored: a row of qtok, the document's kept prefix
        kd = kd < held ? kd : held;
        L = 2 + kq + ks + kd;
    }
    a.kq[slot] = kq; a.kd[slot] = kd; a.L[slot] = L;
}

struct PairFillArgs {
    const int32_t* pairs; const int32_t* cu_rows; const int32_t* kq; const int32_t* kd; const int64_t* cand; const int32_t* qtok;
    const int32_t* tok; const int64_t* Doff;
    int64_t* ids; int64_t* pos;
    int64_t id_base;
    int P, T, ldc, Q, W, ldq, Lq, N, bos, sep, eos, pad, nsep;
};

// One wave per pair, lanes strided over its rows: column c of the pair is <s> | query token c - 1 | separator | document token | </s>,
// position pad + 1 + c.  A pair whose plan does not fit what is stored (a slot outside the plane or the shard, more kept tokens than
// the row or the document holds) reads nothing and gets pad tokens: every id written indexes inside the embedding tables.
__global__ __launch_bounds__(CP_THREADS) void pair_fill_kernel(const PairFillArgs a) {
    const int p = blockIdx.x * CP_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= a.P) return;
    const int r0 = a.cu_rows[p], r1 = a.cu_rows[p + 1];
    if (r0 < 0 || r1 < r0 || r1 > a.T) return;
    const int rows = r1 - r0;
    const int slot = a.pairs[p];
    bool ok = slot >= 0 && (int64_t)slot < (int64_t)a.Q * a.W;
    int q = 0, kq = 0, kd = 0, ks = 0;
    int64_t doc0 = 0;
    if (ok) {
        q = slot / a.W;
        kq = a.kq[slot]; kd = a.kd[slot];
        ks = rows - 2 - kq - kd;
        const int64_t id = a.cand[(size_t)q * a.ldc + (slot - q * a.W)];
        const uint64_t d = (uint64_t)id - (uint64_t)a.id_base;
        ok = kq >= 0 && kd >= 0 && kq <= a.Lq && ks >= 0 && ks <= a.nsep && id >= 0 && id >= a.id_base && d < (uint64_t)a.N;
        if (ok) {
            doc0 = a.Doff[d];
            ok = doc0 >= 0 && (int64_t)kd <= a.Doff[d + 1] - doc0 && (kd == 0 || a.tok != nullptr);
        }
    }
    const int32_t* qrow = a.qtok + (size_t)q * a.ldq;
    const int sep0 = 1 + kq, doc_c0 = sep0 + ks, eos_c = doc_c0 + kd;
    for (int c = lane; c < rows; c += FZ_WAVE) {
        int32_t t;
        if (!ok) t = a.pad;
        else if (c == 0) t = a.bos;
        else if (c < sep0) t = qrow[c - 1];
        else if (c < doc_c0) t = a.sep;
        else if (c < eos_c) t = a.tok[doc0 + (c - doc_c0)];       // consecutive lanes, consecutive tokens: nothing past the kept prefix
        else t = a.eos;
        a.ids[(size_t)r0 + c] = (int64_t)t;
        a.pos[(size_t)r0 + c] = (int64_t)(ok ? a.pad + 1 + c : a.pad);
    }
}

}  // namespace fz

using namespace fz;

extern "C" int fz_pair_max_sep(void) { return CP_MAX_SEP; }

extern "C" int fz_pair_plan(const int64_t* cand, int ldc, const int32_t* cand_len, int Q, int W, int64_t id_base, const int64_t* Doff,
                            const int32_t* doc_full_len, int N, const int32_t* qlen, int Lq, int max_length, int mode, int nsep, int32_t* kq,
                            int32_t* kd, int32_t* L, void* stream) {
    if (Q < 0 || W < 0 || N < 0 || Lq < 0 || nsep < 0 || ldc < W) return FZ_ERR_ARG;
    if (mode != FZ_PAIR_LONGEST_FIRST && mode != FZ_PAIR_TAIL) return FZ_ERR_ARG;
    if ((int64_t)max_length < 2 + (int64_t)nsep) return FZ_ERR_ARG;                      // no room for the specials: B would be negative
    if ((Q != 0 && W != 0) && (!cand || !qlen || !kq || !kd || !L)) return FZ_ERR_ARG;   // empty tensors carry null pointers
    if ((Q != 0 && W != 0 && N != 0) && !Doff) return FZ_ERR_ARG;
    if (nsep > CP_MAX_SEP || (int64_t)Q * W > 0x7fffffffLL) return FZ_ERR_UNSUPPORTED;
    if (Q == 0 || W == 0) return FZ_OK;
    PairPlanArgs a{};
    a.cand = cand; a.cand_len = cand_len; a.Doff = Doff; a.dfull = doc_full_len; a.qlen = qlen; a.kq = kq; a.kd = kd; a.L = L;
    a.id_base = id_base; a.ldc = ldc; a.Q = Q; a.W = W; a.N = N; a.Lq = Lq; a.B = max_length - (2 + nsep); a.mode = mode; a.nsep = nsep;
    const int64_t slots = (int64_t)Q * W;
    pair_plan_kernel<<<(unsigned)((slots + CP_THREADS - 1) / CP_THREADS), CP_THREADS, 0, as_stream(stream)>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}

extern "C" int fz_pair_fill(const int32_t* pairs, const int32_t* cu_rows, int P, int T, const int32_t* kq, const int32_t* kd,
                            const int64_t* cand, int ldc, int Q, int W, int64_t id_base, const int32_t* qtok, int ldq, int Lq,
                            const int32_t* tok, const int64_t* Doff, int N, int bos, int sep, int eos, int pad_idx, int nsep, int64_t* ids,
                            int64_t* pos_ids, void* stream) {
    if (P < 0 || T < 0 || Q < 0 || W < 0 || N < 0 || Lq < 0 || nsep < 0 || ldc < W || ldq < Lq) return FZ_ERR_ARG;
    if (bos < 0 || sep < 0 || eos < 0 || pad_idx < 0) return FZ_ERR_ARG;
    if (P != 0 && (!pairs || !cu_rows || !kq || !kd || !cand || !Doff || (T != 0 && (!ids || !pos_ids)) || (Lq != 0 && !qtok))) return FZ_ERR_ARG;
    if (nsep > CP_MAX_SEP || (int64_t)Q * W > 0x7fffffffLL) return FZ_ERR_UNSUPPORTED;
    if (P == 0) return FZ_OK;
    PairFillArgs a{};
    a.pairs = pairs; a.cu_rows = cu_rows; a.kq = kq; a.kd = kd; a.cand = cand; a.qtok = qtok; a.tok = tok; a.Doff = Doff; a.ids = ids; a.pos = pos_ids;
    a.id_base = id_base; a.P = P; a.T = T; a.ldc = ldc; a.Q = Q; a.W = W; a.ldq = ldq; a.Lq = Lq; a.N = N;
    a.bos = bos; a.sep = sep; a.eos = eos; a.pad = pad_idx; a.nsep = nsep;
    pair_fill_kernel<<<(unsigned)((P + CP_WAVES - 1) / CP_WAVES), CP_THREADS, 0, as_stream(stream)>>>(a);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
}
