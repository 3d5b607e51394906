"""Shared by tests/test_passages_cpu.py and tests/test_gpu_passages.py: the cases of the passage -> document layer (fz_lists_collapse,
fz_group_expand, fz_group_max_*) and a NumPy restatement of what the kernels must give.  Every output is a copy of input bits, so the
GPU tests compare bit for bit.

The restatement: collapse walks a row in list order through a dict (the first entry of a document opens its column); expand is the
concatenation of arange(poff[d], poff[d + 1]) over the row's slots; the segment maximum is np.maximum.reduceat with the empty-segment
rule ((-inf, -1)), the best passage the first position that holds the maximum."""
import numpy as np

NEG = -np.inf
CHUNK = 1024            # entries per chunk of the collapse walk (one per thread)
CAPACITY = 8192         # fz_lists_max_entries()
COLLAPSE_N = (1, 1023, 1024, 1025, 2049, 8192)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def collapse_ref(ids, scores, lens, group_of, id_base=0, doc_id_base=0, scores64=None):
    """-> (doc_ids [Q, n] int64, doc_scores [Q, n] float32, doc_scores64 or None, best [Q, n] int64, out_len [Q] int32)."""
    Q, n = ids.shape
    out_ids = np.full((Q, n), -1, np.int64)
    out_sc = np.full((Q, n), NEG, np.float32)
    out_sc64 = np.full((Q, n), NEG, np.float64) if scores64 is not None else None
    best = np.full((Q, n), -1, np.int64)
    out_len = np.zeros(Q, np.int32)
    for q in range(Q):
        opened = {}
        for r in range(min(max(int(lens[q]), 0), n)):
            opened.setdefault(int(group_of[int(ids[q, r]) - id_base]) + doc_id_base, r)
        for c, (d, r) in enumerate(opened.items()):
            out_ids[q, c], out_sc[q, c], best[q, c] = d, scores[q, r], ids[q, r]
            if scores64 is not None:
                out_sc64[q, c] = scores64[q, r]
        out_len[q] = len(opened)
    return out_ids, out_sc, out_sc64, best, out_len


def expand_need(cand, cand_len, poff, doc_id_base=0):
    """The passage slots every row needs: [Q] int64."""
    Q, W = cand.shape
    D = len(poff) - 1
    need = np.zeros(Q, np.int64)
    for q in range(Q):
        for w in range(W if cand_len is None else min(max(int(cand_len[q]), 0), W)):
            d = int(cand[q, w]) - doc_id_base
            if cand[q, w] >= 0 and 0 <= d < D:
                need[q] += poff[d + 1] - poff[d]
    return need


def expand_ref(cand, cand_len, poff, ldp, id_base=0, doc_id_base=0):
    """-> (pcand [Q, ldp] int64, seg [Q, W + 1] int32, pcand_len [Q] int32); every row must fit ldp."""
    Q, W = cand.shape
    D = len(poff) - 1
    pcand = np.full((Q, ldp), -1, np.int64)
    seg = np.zeros((Q, W + 1), np.int32)
    for q in range(Q):
        parts, at = [], 0
        for w in range(W):
            seg[q, w] = at
            d = int(cand[q, w]) - doc_id_base
            if (cand_len is None or w < cand_len[q]) and cand[q, w] >= 0 and 0 <= d < D:
                parts.append(np.arange(poff[d], poff[d + 1], dtype=np.int64) + id_base)
                at += int(poff[d + 1] - poff[d])
        seg[q, W] = at
        assert at <= ldp
        if parts:
            pcand[q, :at] = np.concatenate(parts)
    return pcand, seg, seg[:, W].copy()


def max_ref(pscores, pcand, seg, cand_len=None):
    """-> (out [Q, W] of pscores' dtype, best [Q, W] int64)."""
    Q, W = seg.shape[0], seg.shape[1] - 1
    out = np.full((Q, W), NEG, pscores.dtype)
    best = np.full((Q, W), -1, np.int64)
    for q in range(Q):
        lo, hi = seg[q, :-1].astype(np.int64), seg[q, 1:].astype(np.int64)
        live = hi > lo
        if cand_len is not None:
            live &= np.arange(W) < cand_len[q]
        if not live.any():
            continue
        row = np.append(pscores[q, :seg[q, W]], pscores.dtype.type(NEG))   # reduceat wants every start inside the array
        red = np.maximum.reduceat(row, lo)                            # an empty segment gives row[lo]: overruled below
        out[q, live] = red[live]
        for w in np.flatnonzero(live):
            best[q, w] = pcand[q, lo[w] + int(np.flatnonzero(pscores[q, lo[w]:hi[w]] == red[w])[0])]
    return out, best


def brute_force_maxp(ids, scores, lens, group_of, id_base=0, doc_id_base=0):
    """Per row the documents ranked by (their maximum score desc, position of that maximum asc): list[Q] of (doc_ids, scores, best)."""
    out = []
    for q in range(ids.shape[0]):
        L = int(lens[q])
        docs = group_of[ids[q, :L] - id_base].astype(np.int64) + doc_id_base
        rows = []
        for d in np.unique(docs):
            at = np.flatnonzero(docs == d)
            top = scores[q, at].max()
            first = int(at[np.flatnonzero(scores[q, at] == top)[0]])
            rows.append((first, int(d)))
        rows.sort(key=lambda x: (-float(scores[q, x[0]]), x[0]))
        out.append((np.array([d for _, d in rows], np.int64), np.array([scores[q, r] for r, _ in rows], np.float32),
                    np.array([ids[q, r] for r, _ in rows], np.int64)))
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def random_poff(rng, D, lo=1, hi=8):
    return np.concatenate([[0], np.cumsum(rng.integers(lo, hi + 1, D))]).astype(np.int64)


def group_table(poff):
    return np.repeat(np.arange(len(poff) - 1, dtype=np.int32), np.diff(poff))


def ranked_scores(rng, L, run=1, neg_tail=0):
    """L non-increasing float32 scores: runs of `run` equal values, the last neg_tail of them -inf."""
    s = np.sort(rng.standard_normal((L + run - 1) // run).astype(np.float32))[::-1]
    s = np.repeat(s, run)[:L].copy()
    if neg_tail:
        s[L - neg_tail:] = NEG
    return s


def ranked_rows(rng, Q, n, P, lens, run=1, neg_tail=0, id_base=0):
    """Q lists of distinct passage ids out of P in (score desc, id asc) order; slots past a row's length hold (-1, -inf).
    -> (ids [Q, n] int64, scores [Q, n] float32)."""
    ids = np.full((Q, n), -1, np.int64)
    sc = np.full((Q, n), NEG, np.float32)
    for q in range(Q):
        L = int(lens[q])
        if L == 0:
            continue
        p = rng.choice(P, L, replace=False).astype(np.int64)
        s = ranked_scores(rng, L, run, min(neg_tail, L - 1))
        for a in range(0, L, run):          # inside a run of equal scores the ids ascend
            p[a:a + run] = np.sort(p[a:a + run])
        if neg_tail:
            p[L - min(neg_tail, L - 1):] = np.sort(p[L - min(neg_tail, L - 1):])
        ids[q, :L], sc[q, :L] = p + id_base, s
    return ids, sc


def mixed_lens(rng, Q, n):
    """Rows of length 0, 1 and n in one call, the rest random."""
    lens = rng.integers(0, n + 1, Q).astype(np.int32)
    lens[:3] = (0, 1, n)
    return lens


def repeats_case():
    """n = 2049, one row, strictly descending scores; documents of two passages (2d, 2d + 1).  Four documents repeat: in the same
    wave (slots 3, 5), in another wave of the same chunk (10, 700), in a later chunk (20, 1500), either side of a chunk boundary
    (1023, 1024); every other entry is the first passage of a document of its own."""
    n = 2049
    pairs = [(3, 5), (10, 700), (20, 1500), (CHUNK - 1, CHUNK)]
    ids = np.full((1, n), -1, np.int64)
    doc = 0
    for a, b in pairs:
        ids[0, a], ids[0, b] = 2 * doc, 2 * doc + 1
        doc += 1
    for r in range(n):
        if ids[0, r] < 0:
            ids[0, r] = 2 * doc
            doc += 1
    scores = np.linspace(4.0, -4.0, n, dtype=np.float32)[None, :].copy()
    poff = np.arange(0, 2 * doc + 1, 2, dtype=np.int64)
    return ids, scores, np.array([n], np.int32), poff, n - len(pairs)


def expand_case(rng, Q, W, D=40, pmax=6, doc_id_base=0, distinct=False):
    """Documents with 0, 1 and pmax passages among random ones; candidates with negative ids, ids below and above the documents'
    range and padded slots; cand_len of 0 and W among random ones.  distinct (W <= D): no document twice in a row, as in a union of
    lists.  -> (cand [Q, W] int64, cand_len [Q] int32, poff)."""
    counts = rng.integers(0, pmax + 1, D)
    counts[:3] = (0, 1, pmax)
    poff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if distinct:
        cand = np.stack([np.concatenate([[q % 3], 3 + rng.permutation(D - 3)[:W - 1]]) for q in range(Q)]).astype(np.int64) + doc_id_base
    else:
        cand = rng.integers(0, D, (Q, W)).astype(np.int64) + doc_id_base
    cand[:, 0] = doc_id_base + np.arange(Q) % 3          # the documents with 0, 1 and pmax passages come first somewhere
    kind = rng.integers(0, 10, (Q, W))
    cand[kind == 0] = -1
    cand[kind == 1] = doc_id_base + D + rng.integers(0, 5)
    cand[kind == 2] = doc_id_base - 1 if doc_id_base > 0 else -7
    cand[0, 0] = doc_id_base + 2                         # row 0 (full length) starts with the document of pmax passages
    cand_len = rng.integers(0, W + 1, Q).astype(np.int32)
    cand_len[0] = W
    if Q > 1:
        cand_len[1] = 0
    return cand, cand_len, poff


def tied_scores(rng, shape, dtype):
    """Few distinct values (ties inside a segment are the rule), some -inf."""
    s = rng.integers(-3, 4, shape).astype(dtype) / dtype(4)
    s[rng.random(shape) < 0.1] = NEG
    return s
