"""The NumPy restatement of the pseudo-relevance-feedback arithmetic (include/fusion_hip.h, 'pseudo-relevance feedback') and the case
builders of tests/test_feedback_cpu.py and tests/test_gpu_feedback.py.

Every product and every add is one float32 operation (NumPy float32 scalars and arrays round once per operation, nothing is fused); a
term's contributions are added in slot order."""
import numpy as np

MAX_V = 32768
F32 = np.float32


def desc_key_f32(x):
    """csrc/common.h desc_key_f32: larger float <=> smaller uint32 key; -0.0 == +0.0; NaN -> 0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    u[u == np.uint32(0x80000000)] = 0
    asc = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    key = ~asc
    key[nan] = 0
    return key.astype(np.uint32)


def slot_docs(fb_ids_row, flen, id_base, N):
    """The slots of one query that count, in order: [(r, d)]."""
    out = []
    for r in range(min(max(int(flen), 0), len(fb_ids_row))):
        i = int(fb_ids_row[r])
        if id_base <= i < id_base + N:
            out.append((r, i - id_base))
    return out


def sparse_feedback_ref(foff, rows, N, V, id_base, qoff, qterms, qw, fb_ids, fb_len, coef, alpha, m, width=None):
    """-> (out_terms [Q, width] int32, out_w [Q, width] float32, out_len [Q] int32, overflow: bool).  rows [nnz, 2] int32 {term, weight
    bits}.  width None: max nq + m capped at V (what ops.sparse_feedback plans)."""
    Q, F = fb_ids.shape
    alpha = F32(alpha)
    wts = np.ascontiguousarray(rows[:, 1]).view(np.float32) if len(rows) else np.zeros(0, np.float32)
    trm = rows[:, 0] if len(rows) else np.zeros(0, np.int32)
    if width is None:
        width = min(int((qoff[1:] - qoff[:-1]).max()) + m, V) if Q else 0
    out_t = np.full((Q, width), -1, np.int32)
    out_w = np.zeros((Q, width), np.float32)
    out_len = np.zeros(Q, np.int32)
    overflow = False
    for q in range(Q):
        acc = np.zeros(V, np.float32)
        isq = np.zeros(V, bool)
        touched = np.zeros(V, bool)
        t = qterms[qoff[q]:qoff[q + 1]]
        acc[t] = acc[t] + alpha * qw[qoff[q]:qoff[q + 1]].astype(np.float32)
        isq[t] = True
        flen = F if fb_len is None else fb_len[q]
        for r, d in slot_docs(fb_ids[q], flen, id_base, N):
            tt = trm[foff[d]:foff[d + 1]]
            acc[tt] = acc[tt] + F32(coef[q, r]) * wts[foff[d]:foff[d + 1]]
            touched[tt] = True
        cand = np.flatnonzero(touched & ~isq)
        keys = desc_key_f32(acc[cand])
        order = np.lexsort((cand, keys))                       # key ascending, then term ascending
        kept = cand[order[:min(m, len(cand))]]
        terms = np.sort(np.concatenate([np.flatnonzero(isq), kept])).astype(np.int32)
        out_len[q] = len(terms)
        if len(terms) > width:
            overflow = True
        n = min(len(terms), width)
        out_t[q, :n] = terms[:n]
        out_w[q, :n] = acc[terms[:n]]
    return out_t, out_w, out_len, overflow


def dense_feedback_ref(Qn, Dn, id_base, fb_ids, fb_len, coef, alpha):
    Q, F = fb_ids.shape
    out = (F32(alpha) * Qn.astype(np.float32)).astype(np.float32)
    for q in range(Q):
        flen = F if fb_len is None else fb_len[q]
        for r, d in slot_docs(fb_ids[q], flen, id_base, Dn.shape[0]):
            out[q] = out[q] + F32(coef[q, r]) * Dn[d]
    return out


def csr_of(out_t, out_w, out_len):
    """The padded planes -> (qoff, qterms, qw)."""
    keep = out_t >= 0
    off = np.zeros(len(out_len) + 1, np.int64)
    off[1:] = np.cumsum(out_len)
    return off, out_t[keep].astype(np.int32), out_w[keep].astype(np.float32)


# ---- case builders -------------------------------------------------------------------------------------------------------------
def full_mantissa(rng, n, signed=False):
    """float32 values in [0.5, 2) with random mantissas (a different order of additions shows in the last bits)."""
    bits = (rng.integers(0, 1 << 23, n, dtype=np.int64) | (rng.integers(126, 128, n, dtype=np.int64) << 23)).astype(np.uint32)
    if signed:
        bits = bits | (rng.integers(0, 2, n, dtype=np.int64).astype(np.uint32) << np.uint32(31))
    return bits.view(np.float32)


def forward_of(doc_rows):
    """[(terms ascending int, weights float32)] -> (foff int64 [N + 1], rows int32 [nnz, 2])."""
    foff = np.zeros(len(doc_rows) + 1, np.int64)
    foff[1:] = np.cumsum([len(t) for t, _ in doc_rows])
    rows = np.zeros((int(foff[-1]), 2), np.int32)
    for d, (t, w) in enumerate(doc_rows):
        rows[foff[d]:foff[d + 1], 0] = t
        rows[foff[d]:foff[d + 1], 1] = np.asarray(w, np.float32).view(np.int32)
    return foff, rows


def random_docs(rng, V, lens, signed=False):
    return [(np.sort(rng.choice(V, size=min(int(n), V), replace=False)).astype(np.int32), full_mantissa(rng, min(int(n), V), signed)) for n in lens]


def queries_of(rows):
    """[(terms, weights)] -> (qoff, qterms, qw)."""
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t, _ in rows])
    qt = np.concatenate([np.asarray(t, np.int32) for t, _ in rows]) if rows else np.zeros(0, np.int32)
    qw = np.concatenate([np.asarray(w, np.float32) for _, w in rows]) if rows else np.zeros(0, np.float32)
    return off, qt.astype(np.int32), qw.astype(np.float32)


def random_case(rng, V, F, row_lens, Q=4, nq=5, id_base=0, signed=False):
    """A random index of len(row_lens) documents, Q queries of up to nq terms (query 1 empty), feedback lists that mix real ids, -1,
    ids below and past the index and a repeated document, mixed fb_len and signed full-mantissa coefficients."""
    docs = random_docs(rng, V, row_lens, signed)
    N = len(docs)
    foff, rows = forward_of(docs)
    qs = []
    for q in range(Q):
        n = 0 if q == 1 else min(int(rng.integers(1, nq + 1)), V)
        qs.append((np.sort(rng.choice(V, size=n, replace=False)), full_mantissa(rng, n, signed)))
    qoff, qterms, qw = queries_of(qs)
    fb_ids = (rng.integers(0, max(N, 1), (Q, F)) + id_base).astype(np.int64)
    if F >= 3:
        fb_ids[0, 1] = -1
        fb_ids[2 % Q, 0] = id_base - 1
        fb_ids[2 % Q, 2] = id_base + N
        fb_ids[0, 2] = fb_ids[0, 0]                            # the same document twice
    fb_len = rng.integers(0, F + 1, Q).astype(np.int32)
    fb_len[0] = F
    if Q > 3:
        fb_len[3] = F + 3                                      # clamped
    coef = full_mantissa(rng, Q * F, True).reshape(Q, F)
    return dict(foff=foff, rows=rows, N=N, V=V, id_base=id_base, qoff=qoff, qterms=qterms, qw=qw, fb_ids=fb_ids, fb_len=fb_len, coef=coef)


def candidates_of(case):
    """The number of candidates per query (touched and not a query term)."""
    out = []
    for q in range(len(case["qoff"]) - 1):
        isq = set(case["qterms"][case["qoff"][q]:case["qoff"][q + 1]].tolist())
        tt = set()
        for _, d in slot_docs(case["fb_ids"][q], case["fb_len"][q], case["id_base"], case["N"]):
            tt |= set(case["rows"][case["foff"][d]:case["foff"][d + 1], 0].tolist())
        out.append(len(tt - isq))
    return out


# ---- the planted-cluster corpus ---------------------------------------------------------------------------------------------------
def planted(seed, V=512, clusters=8, topic=12, per=32, Q=64):
    """V terms, `clusters` clusters of `topic` topic terms (disjoint), `per` documents each: 6 topic terms at k/8, k in 4..8, and 4
    noise terms (outside every topic) at k/8, k in 1..4, L2-normalised.  Q queries of 2 topic terms of cluster q % clusters.
    -> (D [N, V] float32, Qm [Q, V] float32, doc_cluster [N], query_cluster [Q])."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(V)
    topics = perm[:clusters * topic].reshape(clusters, topic)
    noise = perm[clusters * topic:]
    N = clusters * per
    D = np.zeros((N, V), np.float32)
    dc = np.repeat(np.arange(clusters), per)
    for d in range(N):
        D[d, rng.choice(topics[dc[d]], 6, replace=False)] = rng.integers(4, 9, 6) / 8.0
        D[d, rng.choice(noise, 4, replace=False)] = rng.integers(1, 5, 4) / 8.0
    D = (D / np.sqrt((D.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(np.float32)
    Qm = np.zeros((Q, V), np.float32)
    qc = np.arange(Q) % clusters
    for q in range(Q):
        Qm[q, rng.choice(topics[qc[q]], 2, replace=False)] = np.float32(1.0 / np.sqrt(2.0))
    return D, Qm, dc, qc


def rows_of_matrix(M):
    """The non-zero (term, weight) lists of the rows of M: [(terms, weights)]."""
    return [(np.flatnonzero(r).astype(np.int32), r[np.flatnonzero(r)].astype(np.float32)) for r in M]


def topk_ids(S, k):
    """[Q, k] ids by (score desc, id asc)."""
    return np.stack([np.lexsort((np.arange(S.shape[1]), -S[q].astype(np.float64)))[:k] for q in range(S.shape[0])])


def cluster_recall(ids, dc, qc, per):
    return float(np.mean([(dc[ids[q]] == qc[q]).sum() / per for q in range(len(qc))]))


def planted_recall_ref(seed, fb_docs=5, m=8, depth=32):
    """Recall@depth of the query's cluster before and after one feedback round computed with the restatement (alpha = 1, uniform beta = 1)."""
    D, Qm, dc, qc = planted(seed)
    N, V = D.shape
    foff, rows = forward_of(rows_of_matrix(D))
    qoff, qterms, qw = queries_of(rows_of_matrix(Qm))
    first = topk_ids(Qm @ D.T, depth)
    fb_ids = first[:, :fb_docs].astype(np.int64)
    coef = np.full(fb_ids.shape, 1.0 / fb_docs, np.float32)
    ot, ow, ol, _ = sparse_feedback_ref(foff, rows, N, V, 0, qoff, qterms, qw, fb_ids, None, coef, 1.0, m)
    Q2 = np.zeros_like(Qm)
    for q in range(len(qc)):
        Q2[q, ot[q, :ol[q]]] = ow[q, :ol[q]]
    second = topk_ids(Q2 @ D.T, depth)
    per = N // (dc.max() + 1)
    return cluster_recall(first, dc, qc, per), cluster_recall(second, dc, qc, per)
