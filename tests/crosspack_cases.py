"""Shared by tests/test_crosspack_cpu.py and tests/test_gpu_crosspack.py (numpy only): the pair rules of csrc/crosspack.hip restated once,
the restated fill (ids / pos / cu_rows of a pair list), and the builders of the cases both files use."""
import numpy as np

LONGEST_FIRST, TAIL = "longest_first", "tail"
Q, W, N = 5, 7, 23
BIG_BASE = 2 ** 33 + 5
# one token per word with either tokenizer (the word-level tokenizer of checkpoint_utils.tiny_tokenizer knows exactly these)
WORDS = ["le", "la", "loi", "article", "code", "civil", "chat", "chien", "droit", "bail", "juge", "peut", "est", "un", "une", "de"]


# ---- the pair rule --------------------------------------------------------------------------------------------------------------------
def budget(max_length: int, nsep: int) -> int:
    return max_length - (2 + nsep)


def keep(mode: str, max_length: int, nsep: int, lq: int, ld: int):
    """(kq, ks, kd): the query tokens, separators and document tokens a pair of plain lengths (lq, ld) keeps."""
    B = budget(max_length, nsep)
    if mode == TAIL:                                    # [bos] + (q ++ [sep] * nsep ++ d)[: max_length - 2] + [eos]
        M = max_length - 2
        kq = min(lq, M)
        ks = min(nsep, M - kq)
        return kq, ks, min(ld, M - kq - ks)
    assert mode == LONGEST_FIRST
    if lq + ld <= B:
        return lq, nsep, ld
    n1, n2 = min(lq, ld), max(lq, ld)
    n2 = max(n1, B - n1)
    if n1 + n2 > B:
        n1 = B // 2
        n2 = n1 + B % 2
    return (n2, nsep, n1) if lq > ld else (n1, nsep, n2)


def owned(cand, cand_len, id_base: int, n_docs: int):
    """[Q, W] bool: r < cand_len[q] and 0 <= id - id_base < N (Python integers: no wrap-around)."""
    Qn, Wn = cand.shape
    out = np.zeros((Qn, Wn), dtype=bool)
    for q in range(Qn):
        klen = Wn if cand_len is None else max(0, min(int(cand_len[q]), Wn))
        for r in range(klen):
            i = int(cand[q, r])
            out[q, r] = i >= 0 and 0 <= i - id_base < n_docs
    return out


def plan(mode, max_length, nsep, cand, cand_len, id_base, held, full, qlen, Lq):
    """The plan kernel: held [N] the stored token counts, full [N] the lengths before the store's cut (None: = held), qlen [Q] the queries'
    lengths before any cut, Lq the columns of their id matrix -> (kq, kd, L) [Q, W] int32."""
    Qn, Wn = cand.shape
    kq, kd, L = (np.zeros((Qn, Wn), dtype=np.int32) for _ in range(3))
    own = owned(cand, cand_len, id_base, len(held))
    for q, r in zip(*np.nonzero(own)):
        d = int(cand[q, r]) - id_base
        a, s, b = keep(mode, max_length, nsep, int(qlen[q]), int(held[d] if full is None else full[d]))
        a, b = min(a, Lq), min(b, int(held[d]))
        kq[q, r], kd[q, r], L[q, r] = a, b, 2 + a + s + b
    return kq, kd, L


def fill(pairs, kq, kd, L, cand, id_base, qtok, tok, Doff, bos, sep, eos, pad):
    """The fill kernel for the pair list `pairs` (flat slots q * W + r): (ids [T], pos [T] int64, cu_rows [P + 1] int32)."""
    Wn = cand.shape[1]
    ids, pos, cu = [], [], [0]
    for s in pairs:
        q, r = divmod(int(s), Wn)
        a, b, rows = int(kq[q, r]), int(kd[q, r]), int(L[q, r])
        d0 = int(Doff[int(cand[q, r]) - id_base])
        row = [bos] + [int(t) for t in qtok[q, :a]] + [sep] * (rows - 2 - a - b) + [int(t) for t in tok[d0: d0 + b]] + [eos]
        assert len(row) == rows
        ids += row
        pos += [pad + 1 + c for c in range(rows)]
        cu.append(cu[-1] + rows)
    return np.array(ids, dtype=np.int64), np.array(pos, dtype=np.int64), np.array(cu, dtype=np.int32)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def text(n: int, salt: int) -> str:
    return " ".join(WORDS[(salt * 7 + j * 3 + j // 16) % 16] for j in range(n))


def doc_lengths(B: int):
    cyc = [0, 1, 2, B // 2, B // 2 + 1, B - 1, B, B + 1, 3 * B]
    return [cyc[d % len(cyc)] for d in range(N)]


def query_lengths(B: int):
    return [0, 1, B // 2, B, B + 3]


def corpus(B: int):
    """(queries, documents): Q and N texts of the lengths above."""
    return [text(n, 100 + q) for q, n in enumerate(query_lengths(B))], [text(n, d) for d, n in enumerate(doc_lengths(B))]


def candidates(id_base: int = BIG_BASE, seed: int = 0):
    """cand [Q, W] int64, cand_len [Q] int32 (W, 0, 3, W, W): every document-length class meets the empty, the full and the over-long query;
    row 0 holds -1 and an id below id_base, row 3 the id id_base + N and a duplicate."""
    rng = np.random.default_rng(seed)
    cand = np.empty((Q, W), dtype=np.int64)
    for q in range(Q):
        cand[q] = id_base + rng.permutation(N)[:W]
    cand[0, 1], cand[0, 3] = -1, id_base - 1
    cand[3, 0], cand[3, 4] = id_base + N, cand[3, 1]
    cand[4] = id_base + np.array([8, 7, 6, 5, 4, 3, 17])          # the over-long query against 3B, B + 1, B, B - 1, B/2 + 1, B/2, 3B
    return cand, np.array([W, 0, 3, W, W], dtype=np.int32)


def pair_strings(slots, cand, id_base, queries, documents):
    return [(queries[int(s) // cand.shape[1]], documents[int(cand.reshape(-1)[int(s)]) - id_base]) for s in slots]


# the end-to-end comparison ranks by score, so its inputs must not tie by construction (a query that fills the row under the 'tail' rule
# leaves no document token: every candidate gets the same row): short queries, and documents that are not empty and differ in their first token
E2E_QUERY_LENGTHS = lambda B: [1, 2, 3, B // 2, B // 2 + 1]      # noqa: E731
E2E_POOL = [d for d in range(1, 16) if d % 9]
E2E_SEED = 0     # with the test's model the reference's closest adjacent scores are 6.4e-3 apart (checked on the CPU model, seeds 0 .. 5)


def e2e_inputs(B: int, id_base: int = BIG_BASE):
    """(queries, cand [Q, W] int64): no row holds a document twice."""
    rng = np.random.default_rng(E2E_SEED)
    cand = np.stack([id_base + rng.permutation(np.array(E2E_POOL))[:W] for _ in range(Q)]).astype(np.int64)
    return [text(n, 100 + q) for q, n in enumerate(E2E_QUERY_LENGTHS(B))], cand
