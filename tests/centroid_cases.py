"""Reference and input builders of the ColBERT candidate-stage tests (test_centroid_cpu.py without a GPU, test_gpu_centroid_search.py on
one).  Not collected by pytest.

The candidate score, restated in numpy.  Every document token carries the id of its nearest centroid; the index lists per centroid c the
distinct documents that hold it, ascending: cdoc[coff[c]: coff[c + 1]].  A query is its probe table pc / ps [Q, Lq * nprobe], token-major
(pc < 0 pads).  With m_i = the largest ps over token i's probes whose list holds d,
    approx(q, d) = ((+0.0 + m_i1) + m_i2) + ...   in float32, over the tokens i that hit d, ascending;  +0.0 without a hit.
The max does not depend on order and the adds have a fixed one, so the score is defined bit for bit."""
import numpy as np

DIM = 128


# ---- the reference -----------------------------------------------------------------------------------------------------------
def approx_plane(coff, cdoc, pc, ps, Lq, nprobe, N):
    """[Q, N] float32: per query and token a hit mask, np.maximum over the token's probes, one float32 add per hit token."""
    coff, cdoc, pc = np.asarray(coff), np.asarray(cdoc), np.asarray(pc)
    ps = np.asarray(ps, dtype=np.float32)
    Q = pc.shape[0]
    assert pc.shape == ps.shape == (Q, Lq * nprobe)
    out = np.zeros((Q, N), dtype=np.float32)
    for q in range(Q):
        acc = np.zeros(N, dtype=np.float32)
        for i in range(Lq):
            hit = np.zeros(N, dtype=bool)
            m = np.full(N, -np.inf, dtype=np.float32)
            for j in range(i * nprobe, (i + 1) * nprobe):
                c = int(pc[q, j])
                if c < 0:
                    continue
                docs = cdoc[int(coff[c]): int(coff[c + 1])]
                m[docs] = np.maximum(m[docs], ps[q, j])
                hit[docs] = True
            acc[hit] = (acc[hit] + m[hit]).astype(np.float32)
        out[q] = acc
    return out


def approx_dense(doc_codes, pc, ps, Lq, nprobe):
    """The formula itself, pair by pair, from every document's set of codes: for a few dozen documents."""
    Q, N = len(pc), len(doc_codes)
    out = np.zeros((Q, N), dtype=np.float32)
    for q in range(Q):
        for d in range(N):
            acc = np.float32(0.0)
            for i in range(Lq):
                got = [np.float32(ps[q][i * nprobe + j]) for j in range(nprobe) if int(pc[q][i * nprobe + j]) in doc_codes[d]]
                if got:
                    acc = np.float32(acc + max(got))
            out[q, d] = acc
    return out


def topk_ref(plane, k, id_base=0):
    """k best per row by (score desc, id asc): ([Q, k] float32, [Q, k] int64), padded with (-inf, -1)."""
    Q, N = plane.shape
    s = np.full((Q, k), -np.inf, dtype=np.float32)
    i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        order = np.lexsort((np.arange(N), -plane[q].astype(np.float64)))[:k]
        s[q, :len(order)], i[q, :len(order)] = plane[q, order], order + id_base
    return s, i


# ---- index builders ----------------------------------------------------------------------------------------------------------
def index_ref(codes, Doff, K):
    """Brute-force set construction: (coff [K + 1] int64, cdoc int32, the documents' code sets)."""
    N = len(Doff) - 1
    doc_codes = [set(int(c) for c in codes[int(Doff[d]): int(Doff[d + 1])]) for d in range(N)]
    lists = [[d for d in range(N) if c in doc_codes[d]] for c in range(K)]
    return index_from_lists(lists) + (doc_codes,)


def index_from_lists(lists):
    coff = np.zeros(len(lists) + 1, dtype=np.int64)
    coff[1:] = np.cumsum([len(l) for l in lists])
    cdoc = np.concatenate([np.asarray(l, dtype=np.int32) for l in lists]) if len(lists) else np.zeros(0, dtype=np.int32)
    return coff, cdoc.astype(np.int32)


def random_lists(rng, N, K, mean=12, full=(1,), empty=(0,), heavy=()):
    """Per centroid an ascending list of distinct documents: mostly short (the shape inside a slice at corpus scale), `full` ones hold every
    document, `empty` ones none, `heavy` ones about a third of them."""
    lists = []
    for c in range(K):
        if c in empty:
            lists.append(np.zeros(0, dtype=np.int32))
        elif c in full:
            lists.append(np.arange(N, dtype=np.int32))
        else:
            n = N // 3 if c in heavy else int(rng.integers(1, 2 * mean))
            lists.append(np.sort(rng.choice(N, size=min(n, N), replace=False)).astype(np.int32))
    return lists


def random_probes(rng, Q, Lq, nprobe, K, scale=1.0):
    """Distinct centroids inside a token, float32 scores of both signs, in descending order inside a token (as centroid_probes gives them)."""
    pc = np.stack([np.concatenate([rng.choice(K, size=nprobe, replace=nprobe > K) for _ in range(Lq)]) for _ in range(Q)]).astype(np.int32)
    ps = rng.normal(0.2, scale, (Q, Lq, nprobe)).astype(np.float32)
    ps = -np.sort(-ps, axis=2)
    return pc, ps.reshape(Q, Lq * nprobe)


def planted_case(rng, N, K, Q, Lq, nprobe):
    """The lists and probe tables of the plane test.  Centroid 0 is empty, centroid 1 holds every document, centroids 2 and 3 share
    document 7 and a run of documents around every slice edge, centroid 4 is heavy.
    query 0: token 0 probes 0 (empty) and 1 (everything) first, so every document is hit; where nprobe >= 4 it also probes 2 and 3: the
             shared documents get the max of the two, not the sum; token 1 (Lq >= 2) probes centroid 2 again: added a second time;
    query 1: never probes centroid 1 and its scores are all negative: a hit document ends below the untouched ones (+0.0);
    query 2: equal scores inside a token, and the last probe of every token is padding (pc = -1) where nprobe >= 2; where nprobe > 256
             (the kernel resolves such a token 256 probes at a time) there is padding inside the token's second batch as well."""
    assert Q == 3 and K > 8
    lists = random_lists(rng, N, K, heavy=(4,))
    shared = np.unique(np.concatenate([[7], np.arange(N // 2 - 3, N // 2 + 3), rng.choice(N, 40, replace=False)])).astype(np.int32)
    lists[2] = np.union1d(lists[2], shared).astype(np.int32)
    lists[3] = np.union1d(lists[3], shared).astype(np.int32)
    pc, ps = random_probes(rng, Q, Lq, nprobe, K)
    pc[1][pc[1] == 1] = 5
    ps[1] = -np.abs(ps[1]) - np.float32(0.125)
    plant = [0, 1, 2, 3][:nprobe]
    pc[0, :len(plant)] = plant
    if len(plant) == 1:
        pc[0, 0] = 1
    if Lq >= 2:
        pc[0, nprobe] = 2
    ps[2] = np.round(ps[2] * 2) / 2          # halves: many equal scores inside a token
    if nprobe >= 2:
        pc[2, nprobe - 1::nprobe] = -1
    if nprobe > 256:                          # a token wider than one 256-probe batch: padding in the middle of its second batch too
        for i in range(Lq):
            pc[2, i * nprobe + 258: i * nprobe + 256 + (nprobe - 256) // 2] = -1
    return lists, pc, ps


# ---- token builders ----------------------------------------------------------------------------------------------------------
def sign_centroids(rng, K):
    """K distinct sign patterns with exactly 32 entries of +-1 in 128: equal norm, so a centroid's unique nearest centroid is itself
    (<c, c> = 32, <c, c'> < 32 for another pattern)."""
    seen, rows = set(), []
    while len(rows) < K:
        v = np.zeros(DIM, dtype=np.float32)
        idx = rng.choice(DIM, 32, replace=False)
        v[idx] = rng.choice([-1.0, 1.0], 32)
        key = v.tobytes()
        if key not in seen:
            seen.add(key)
            rows.append(v)
    return np.stack(rows).astype(np.float16)


def doc_offsets(lens):
    Doff = np.zeros(len(lens) + 1, dtype=np.int64)
    Doff[1:] = np.cumsum(lens)
    return Doff


def clustered_tokens(rng, n, centres, noise=0.35):
    """Unit-norm rows: a centre + noise, normalised; -> (rows float16, the centre of every row)."""
    which = rng.integers(0, len(centres), n)
    x = centres[which].astype(np.float64) + rng.normal(0, noise / np.sqrt(DIM), (n, DIM))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16), which
