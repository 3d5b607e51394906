"""Seeded cases for the forward (document-major) index and its pair scorers (csrc/forward.hip), shared by tests/test_forward_cpu.py and
tests/test_gpu_forward.py: numpy restatements of the build (ops.forward_index) and of the row walk (fz_sparse_fwd_pairs_f32), and a
corpus whose rows are long enough to take a lane group several steps.  Everything here is numpy."""
import numpy as np

import pairs_cases as P

GROUP = 16                           # lanes per candidate row of sparse_fwd_pairs_kernel: postings per step


def forward_build(toff, pdoc, N: int):
    """(foff [N + 1] int64, fterm int32, fpos int32): ops.forward_index restated -- a stable sort of the postings by document."""
    toff, pdoc = np.asarray(toff, dtype=np.int64), np.asarray(pdoc, dtype=np.int32)
    order = np.argsort(pdoc, kind="stable")
    term = np.repeat(np.arange(len(toff) - 1, dtype=np.int32), np.diff(toff))
    foff = np.zeros(N + 1, dtype=np.int64)
    foff[1:] = np.cumsum(np.bincount(pdoc, minlength=N))
    return foff, term[order].astype(np.int32), order.astype(np.int32)


def row_walk(foff, fterm, fw, qoff, qterms, qw, cand, lens, id_base: int, N: int) -> np.ndarray:
    """fz_sparse_fwd_pairs_f32 restated: along the candidate's row (terms ascending), a posting whose term the query holds adds
    qw * w -- acc = acc + product from +0.0, one float32 rounding per product and per add; the -inf rules of pairs_cases.expected."""
    Q, W = cand.shape
    lens = np.full(Q, W) if lens is None else np.asarray(lens)
    out = np.full((Q, W), -np.inf, dtype=np.float32)
    fw = np.asarray(fw, dtype=np.float32)
    for q in range(Q):
        qt, w = qterms[qoff[q]:qoff[q + 1]], np.asarray(qw[qoff[q]:qoff[q + 1]], dtype=np.float32)
        for r in range(min(int(lens[q]), W)):
            d = int(cand[q, r]) - int(id_base)
            if cand[q, r] < 0 or not 0 <= d < N:
                continue
            lo, hi = int(foff[d]), int(foff[d + 1])
            at = np.searchsorted(qt, fterm[lo:hi])
            hit = (at < len(qt)) & (qt[np.minimum(at, max(len(qt) - 1, 0))] == fterm[lo:hi]) if len(qt) else np.zeros(hi - lo, dtype=bool)
            prod = w[at[hit]] * fw[lo:hi][hit]                                        # float32 * float32, each rounded once
            out[q, r] = np.add.accumulate(np.concatenate([np.zeros(1, dtype=np.float32), prod]), dtype=np.float32)[-1]   # strictly in order
    return out


# ---- a corpus of long rows -------------------------------------------------------------------------------------------------------------
LR_V, LR_N = 32005, 300              # V is no multiple of 32: the bitmap's last word is partial
LR_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 64, 166, 700)      # document d holds LR_LENS[d % 11] terms: around every step count of a lane group
LR_SPECIAL = (0, 31, 32, 63, 64, LR_V - 1)                  # the bitmap's word edges and last bit: held by documents and by queries
LR_TWIN_DOC, LR_ORDER_DOC = 10, 2                           # a 700-term document (query 0 is its term set) | the document of query 3
LR_ORDER_TERMS = (100, 200, 300)                            # query 3: weights 1e8, 1, -1e8 on these terms of LR_ORDER_DOC (document weights 1)
LR_Q, LR_TWIN_QUERY, LR_EMPTY_QUERY, LR_WIDE_QUERY, LR_ORDER_QUERY = 6, 0, 1, 2, 3
LR_WIDE_TERMS = 5000


def long_row_corpus(seed: int = 17):
    """(Qm [6, V], Dm [N, V]) float32.  Queries: 0 = the term set of LR_TWIN_DOC (a chain of 700 adds), 1 empty, 2 of 5,000 terms, 3 the
    order probe (1e8 + 1 - 1e8 = 0.0 in term order, 1.0 in any other), 4 and 5 ordinary with the special terms."""
    rng = np.random.default_rng(seed)
    Dm = np.zeros((LR_N, LR_V), dtype=np.float32)
    plain = np.setdiff1d(np.arange(LR_V), LR_SPECIAL + LR_ORDER_TERMS)
    for d in range(LR_N):
        n = LR_LENS[d % len(LR_LENS)]
        fixed = list(LR_SPECIAL) if n >= 64 else [LR_SPECIAL[d % len(LR_SPECIAL)]] if n >= 1 else []
        if d == LR_ORDER_DOC:
            fixed = list(LR_ORDER_TERMS)
        terms = np.concatenate([np.array(fixed, dtype=np.int64), rng.choice(plain, n - len(fixed), replace=False)])
        Dm[d, terms] = rng.random(n).astype(np.float32) + 0.05
    Dm[LR_ORDER_DOC, list(LR_ORDER_TERMS)] = 1.0
    Qm = np.zeros((LR_Q, LR_V), dtype=np.float32)
    twin = np.nonzero(Dm[LR_TWIN_DOC])[0]
    Qm[LR_TWIN_QUERY, twin] = rng.random(len(twin)).astype(np.float32) + 0.05
    wide = np.concatenate([np.array(LR_SPECIAL), rng.choice(plain, LR_WIDE_TERMS - len(LR_SPECIAL), replace=False)])
    Qm[LR_WIDE_QUERY, wide] = rng.random(LR_WIDE_TERMS).astype(np.float32) + 0.05
    Qm[LR_ORDER_QUERY, list(LR_ORDER_TERMS)] = (1e8, 1.0, -1e8)
    for q in (4, 5):
        terms = np.concatenate([np.array(LR_SPECIAL), rng.choice(plain, 40, replace=False), np.nonzero(Dm[9 + 11 * q])[0][::7]])
        Qm[q, terms] = rng.random(len(terms)).astype(np.float32) + 0.05
    return Qm, Dm


def long_row_candidates(seed: int, W: int, id_base: int):
    """(cand [6, W] int64, lens [6] int32): pairs_cases.candidates' mix over the long-row corpus, every row starting with the twin document,
    the order probe's document and one document of every row length."""
    cand, lens = P.candidates(seed, LR_Q, W, LR_N, id_base)
    head = [LR_TWIN_DOC, LR_ORDER_DOC] + [22 + i for i in range(len(LR_LENS))]       # documents 22 .. 32: one of every length
    for q in range(LR_Q):
        n = min(W, len(head))
        cand[q, :n] = id_base + np.array(head[:n])
        lens[q] = W if q < 4 else max(int(lens[q]), min(W, 8))
    return cand, lens


# ---- a lexical corpus ------------------------------------------------------------------------------------------------------------------
def lexical_text(seed: int, n_docs: int, lo: int = 3, hi: int = 40, vocab_size: int = 300):
    """Documents of lo .. hi - 1 words drawn from a Zipf-like vocabulary w0, w1, ...: repeated words inside a document are the rule."""
    rng = np.random.default_rng(seed)
    vocab = np.array([f"w{i}" for i in range(vocab_size)])
    p = 1.0 / np.arange(1, vocab_size + 1); p /= p.sum()
    sizes = rng.integers(lo, hi, n_docs)
    words = rng.choice(vocab, size=int(sizes.sum()), p=p)
    return [" ".join(w) for w in np.split(words, np.cumsum(sizes)[:-1])]


LEX_QUERIES = ["w0 w3 w0 w17", "zzz w1 w1 unseen w2", "", "w5", "w299 w0 w8 w8 w8 w40 w2"]      # a repeated term | out of vocabulary | no term
