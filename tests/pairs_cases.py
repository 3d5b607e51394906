"""Seeded cases for the pair scorers (csrc/pairs.hip: fz_dot_pairs_f32, fz_sparse_dot_pairs_f32), shared by tests/test_pairs_cpu.py and
tests/test_gpu_pairs.py, and a numpy restatement of the sparse chain.  Everything here is numpy: the GPU test moves it to the device."""
import numpy as np

DP_SLOTS = 256                       # candidate slots per workgroup of dot_pairs_kernel (csrc/pairs.hip)
DIMS = (768, 100, 4)                 # a whole number of k-tile pairs | ragged | shorter than one k-tile
WIDTHS = (1, 63, 64, 65, 129, 300)   # ... and one wider than a workgroup's block of slots
QS = (1, 3, 130)
BIG_BASE = 2 ** 33 + 7               # an id_base beyond 2^31
DENORMAL_ROW, ZERO_ROW = 5, 6        # rows of dense_corpus's Dn


def dense_corpus(seed: int, N: int, d: int):
    """(Qn [130, d], Dn [N, d]) float32, rows of unit length but for Dn's DENORMAL_ROW (values around 1e-41) and ZERO_ROW, and query 2,
    which is scaled down until its products with ordinary rows are denormal."""
    rng = np.random.default_rng(seed)
    Qn = rng.standard_normal((max(QS), d)).astype(np.float32)
    Dn = rng.standard_normal((N, d)).astype(np.float32)
    Qn /= np.linalg.norm(Qn, axis=1, keepdims=True)
    Dn /= np.linalg.norm(Dn, axis=1, keepdims=True)
    Dn[DENORMAL_ROW] = (rng.integers(-9000, 9000, d) * 1e-45).astype(np.float32)
    assert np.all(np.abs(Dn[DENORMAL_ROW]) < np.finfo(np.float32).tiny) and np.any(Dn[DENORMAL_ROW] != 0)
    Dn[ZERO_ROW] = 0.0
    Qn[2] *= np.float32(1e-37)
    return Qn, Dn


def candidates(seed: int, Q: int, W: int, N: int, id_base: int):
    """(cand [Q, W] int64, cand_len [Q] int32): ids mostly inside the shard, with negative ids, ids just below id_base and at / past
    id_base + N mixed in, the special rows, one document twice in a row and the same document in different slots of different rows; list
    lengths 0, the middle and W (then random)."""
    rng = np.random.default_rng(seed)
    cand = id_base + rng.integers(0, N, (Q, W)).astype(np.int64)
    odd = rng.random((Q, W))
    cand[odd < 0.04] = -1
    cand[(odd >= 0.04) & (odd < 0.06)] = -(2 ** 40)
    cand[(odd >= 0.06) & (odd < 0.09)] = id_base - 1
    cand[(odd >= 0.09) & (odd < 0.12)] = id_base + N
    cand[(odd >= 0.12) & (odd < 0.14)] = id_base + N + 2 ** 32
    cand[(odd >= 0.14) & (odd < 0.17)] = id_base + DENORMAL_ROW
    cand[(odd >= 0.17) & (odd < 0.20)] = id_base + ZERO_ROW
    for q in range(Q):
        cand[q, (3 * q) % W] = id_base + 11          # the same document in different slots of different rows ...
        if W >= 2:
            cand[q, W - 2:] = id_base + 12           # ... and twice in a row
    lens = rng.integers(0, W + 1, Q).astype(np.int32)
    for q, n in zip(range(Q), (W, 0, (W + 1) // 2)):
        lens[q] = n
    return cand, lens


def expected(plane: np.ndarray, cand: np.ndarray, lens, id_base: int) -> np.ndarray:
    """The contract: a gather from the all-pairs plane [Q, N]; -inf where r >= lens[q] (None: full), the id is negative or it is not one
    of the shard's documents id_base .. id_base + N - 1."""
    Q, W = cand.shape
    N = plane.shape[1]
    lens = np.full(Q, W) if lens is None else np.asarray(lens)
    assert np.abs(cand).max(initial=0) < 2 ** 62 and abs(int(id_base)) < 2 ** 62      # the difference stays inside int64
    pos = cand - np.int64(id_base)
    ok = (cand >= 0) & (pos >= 0) & (pos < N) & (np.arange(W)[None, :] < lens[:, None])
    got = plane[np.arange(Q)[:, None], np.clip(pos, 0, max(N - 1, 0))] if N else np.zeros((Q, W), dtype=plane.dtype)
    return np.where(ok, got, -np.inf).astype(plane.dtype)


# ---- sparse ----------------------------------------------------------------------------------------------------------------------------
SP_V, SP_N = 500, 900
SP_EMPTY_TERMS = (7, 250, 499)       # terms no document holds (queries do)
SP_EMPTY_DOCS = (0, 13, 899)         # documents with no posting at all
SP_LONG_QUERY, SP_EMPTY_QUERY = 1, 2


def sparse_corpus(seed: int, Q: int = 6):
    """(Qm [Q, V], Dm [N, V]) float32, non-negative and sparse as SPLADE vectors are: documents of about 20 terms, queries of about 12;
    query SP_LONG_QUERY has 300 terms, query SP_EMPTY_QUERY none; SP_EMPTY_TERMS / SP_EMPTY_DOCS as named."""
    rng = np.random.default_rng(seed)
    Dm = np.where(rng.random((SP_N, SP_V)) < 0.04, rng.random((SP_N, SP_V)), 0.0).astype(np.float32)
    Qm = np.where(rng.random((Q, SP_V)) < 0.025, rng.random((Q, SP_V)) + 0.1, 0.0).astype(np.float32)
    Qm[SP_LONG_QUERY] = 0.0
    held = np.setdiff1d(np.arange(SP_V), SP_EMPTY_TERMS)                  # 297 terms that documents hold + the 3 that none does = 300
    Qm[SP_LONG_QUERY, rng.choice(held, 297, replace=False)] = rng.random(297).astype(np.float32) + 0.05
    Qm[SP_EMPTY_QUERY] = 0.0
    for q in range(Q):
        if q != SP_EMPTY_QUERY:
            Qm[q, list(SP_EMPTY_TERMS)] = 0.5
    Dm[:, list(SP_EMPTY_TERMS)] = 0.0
    Dm[list(SP_EMPTY_DOCS)] = 0.0
    return Qm, Dm


def inverted(Dm: np.ndarray):
    """(toff [V + 1] int64, pdoc int32, pw float32): the postings of the rows of Dm, documents ascending inside a term (ops.sparse_index)."""
    term, doc = np.nonzero(Dm.T)                                      # term-major, documents ascending
    toff = np.zeros(Dm.shape[1] + 1, dtype=np.int64)
    toff[1:] = np.cumsum(np.bincount(term, minlength=Dm.shape[1]))
    return toff, doc.astype(np.int32), Dm[doc, term].astype(np.float32)


def query_rows(Qm: np.ndarray):
    """(qoff [Q + 1] int64, qterms int32, qw float32): the non-zeros of the rows of Qm, terms ascending (ops.sparse_rows)."""
    q, t = np.nonzero(Qm)
    qoff = np.zeros(Qm.shape[0] + 1, dtype=np.int64)
    qoff[1:] = np.cumsum(np.bincount(q, minlength=Qm.shape[0]))
    return qoff, t.astype(np.int32), Qm[q, t].astype(np.float32)


def sparse_chain(toff, pdoc, pw, qoff, qterms, qw, cand, lens, id_base: int, N: int) -> np.ndarray:
    """fz_sparse_dot_pairs_f32 restated: acc = acc + w * pw from +0.0 over the query's terms in list order, one float32 rounding per product
    and per add, terms whose postings do not hold the document skipped; the -inf rules of `expected`."""
    Q, W = cand.shape
    lens = np.full(Q, W) if lens is None else np.asarray(lens)
    out = np.full((Q, W), -np.inf, dtype=np.float32)
    for q in range(Q):
        for r in range(min(int(lens[q]), W)):
            d = int(cand[q, r]) - int(id_base)
            if cand[q, r] < 0 or not 0 <= d < N:
                continue
            acc = np.float32(0.0)
            for p in range(int(qoff[q]), int(qoff[q + 1])):
                t = int(qterms[p])
                lo, hi = int(toff[t]), int(toff[t + 1])
                e = lo + int(np.searchsorted(pdoc[lo:hi], d, side="left"))
                if e < hi and pdoc[e] == d:
                    acc = np.float32(acc + np.float32(np.float32(qw[p]) * np.float32(pw[e])))
            out[q, r] = acc
    return out


def sparse_candidates(seed: int, toff, pdoc, qoff, qterms, W: int, id_base: int):
    """(cand [Q, W] int64, lens [Q] int32) as `candidates` mixes them, plus -- for every query with terms -- the first and the last entry of
    a posting list of one of its terms, and the documents without postings."""
    Q = len(qoff) - 1
    cand, lens = candidates(seed, Q, W, SP_N, id_base)
    for q in range(Q):
        lens[q] = W if q < 3 else max(int(lens[q]), 8)
        cand[q, 4:4 + len(SP_EMPTY_DOCS)] = id_base + np.array(SP_EMPTY_DOCS)
        held = [int(t) for t in qterms[qoff[q]:qoff[q + 1]] if toff[t + 1] > toff[t]]
        if held:
            t = held[len(held) // 2]
            cand[q, 0], cand[q, 1] = id_base + int(pdoc[toff[t]]), id_base + int(pdoc[toff[t + 1] - 1])
    return cand, lens
