"""The lexical family (fusion_amd/retrievers/bm25.py, csrc/bm25.hip) at the boundaries inside its code rather than at the benchmark's sizes:
the 3,584-document grains of the slice-offset table and the 7,168-document slices of the scoring walk, the 28,672-key float64 sort row W
(ops.sort_max_n(float64)) and top_k against W / 2 and W in the hierarchical top-k cut (ranked_positions, BM25.tune), and the cap on the
slice-offset table.  Reference: the CPU oracle (oracle.BM25 / TFIDF / AtireBM25, .scores, .search_all, oracle.Metrics).  Bar: float64
scores and ids bit for bit; metric means within 1e-12."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EDGE_N = [1, 3583, 3584, 3585, 7167, 7168, 7169, 10752, 14336, 14337, 28673]
MARKER_DOCS = [0, 3583, 3584, 7167, 7168, 14335, 14336]     # first / last document of a grain or slice (and N - 1)


def _bits(x) -> np.ndarray:
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int64 if x.dtype == np.float64 else np.int32)


def _edge_corpus(N: int):
    """Short Zipf-like documents; 'every' in every document, 'twice' twice in one document, marker terms ('edge' and one 'edge<d>' per
    marker document, tf 1-3) only in the first / last documents of grains and slices and in document N - 1."""
    rng = np.random.default_rng(1000 + N)
    vocab = np.array([f"w{i}" for i in range(400)])
    p = 1.0 / np.arange(1, 401); p /= p.sum()
    docs = [list(rng.choice(vocab, size=int(rng.integers(1, 9)), p=p)) + ["every"] for _ in range(N)]
    docs[N // 2] += ["twice", "twice"]
    marks = sorted({d for d in MARKER_DOCS if d < N} | {N - 1})
    for d in marks:
        docs[d] += ["edge"] + [f"edge{d}"] * (1 + d % 3)
    docs = [" ".join(rng.permutation(d)) for d in docs]
    queries = [" ".join(rng.choice(vocab, size=int(rng.integers(1, 7)), p=p)) for _ in range(6)]
    queries += ["", "nowhere absent", "w0 w0 w0", " ".join(["edge"] + [f"edge{d}" for d in marks]),
                "every twice", "twice nowhere edge w1", f"edge{marks[-1]} edge{marks[0]} edge{marks[-1]}"]
    return docs, queries


@pytest.mark.parametrize("N", EDGE_N)
def test_scores_at_slice_and_grain_edges(N, oracle):
    """TF-IDF, BM25 at (1.2, 0.75) and (2.0, b = 0) and AtireBM25: the float64 plane with the slice-offset table == without it (the kernel's
    binary search) == the oracle, bit for bit; BM25 also through the posting-value table and the per-posting expression; the float32
    plane of the same launch == the float64 one rounded."""
    from fusion_amd.retrievers.bm25 import BM25, TFIDF, AtireBM25
    docs, queries = _edge_corpus(N)
    models = [(TFIDF(docs), oracle.TFIDF(docs)),
              (BM25(docs, 1.2, 0.75), oracle.BM25(docs, 1.2, 0.75)),
              (BM25(docs, 2.0, 0.0), oracle.BM25(docs, 2.0, 0.0)),
              (AtireBM25(docs, 0.9, 0.4), oracle.AtireBM25(docs, 0.9, 0.4))]
    for m, om in models:
        exp = _bits(om.scores(queries))
        assert m.slice_off is not None
        table = m.slice_off
        forms = [True, False] if isinstance(m, BM25) else [None]
        for pv in forms:
            if pv is not None:
                m.USE_POSTING_VALUES = pv
            for so in (table, None):
                m.slice_off = so
                s64, s32 = m.scores(queries, want_f32=True)
                assert s64.shape == (len(queries), N)
                np.testing.assert_array_equal(_bits(s64), exp, err_msg=f"{m!r} N={N} pval={pv} table={so is not None}")
                assert torch.equal(s32.view(torch.int32), s64.to(torch.float32).view(torch.int32))
            if pv:
                assert m._pval is not None and m._pval.numel() == m.pdoc.numel()
        m.slice_off = table
        if isinstance(m, BM25):
            m.USE_POSTING_VALUES = True


def test_slice_table_cap():
    """Over the cap (here 0 bytes) no slice-offset table is built and the kernel binary-searches: the same bits.  The default cap keeps
    the table of an index of this size."""
    from fusion_amd import ops
    from fusion_amd.retrievers.bm25 import BM25, SLICE_TABLE_MAX_BYTES, TFIDF
    docs, queries = _edge_corpus(14337)
    for cls, args in ((TFIDF, ()), (BM25, (1.2, 0.75))):
        with_table = cls(docs, *args)
        without = cls(docs, *args, slice_table_max_bytes=0)
        assert with_table.slice_off is not None and without.slice_off is None
        assert ops.bm25_slice_table_bytes(len(with_table.vocab), 14337) == with_table.slice_off.numel() * 8 < SLICE_TABLE_MAX_BYTES
        a64, a32 = with_table.scores(queries, want_f32=True)
        b64, b32 = without.scores(queries, want_f32=True)
        assert torch.equal(a64.view(torch.int64), b64.view(torch.int64)) and torch.equal(a32.view(torch.int32), b32.view(torch.int32))


# -- ranked_positions: every regime of top_k against the sort row W ------------------------------------------------------------

N_SPECS = {"W-1": lambda W: W - 1, "W": lambda W: W, "W+1": lambda W: W + 1, "2W+1": lambda W: 2 * W + 1, "3W+1234": lambda W: 3 * W + 1234,
           "2W+17": lambda W: 2 * W + 17}
K_SPECS = {"0": lambda W, N: 0, "1": lambda W, N: 1, "7": lambda W, N: 7, "1000": lambda W, N: 1000, "W/2-1": lambda W, N: W // 2 - 1,
           "W/2": lambda W, N: W // 2, "W/2+1": lambda W, N: W // 2 + 1, "W-1": lambda W, N: W - 1, "W": lambda W, N: W,
           "W+1": lambda W, N: W + 1, "N-1": lambda W, N: N - 1, "N": lambda W, N: N, "N+5": lambda W, N: N + 5}


@pytest.fixture(scope="module")
def cut_cases(oracle):
    """One tie-heavy index per N (one- to five-word documents: few distinct scores, long tie runs across stretch borders; the last query
    scores 0.0 everywhere) and the oracle's full stable ranking, built on first use."""
    from fusion_amd import ops
    from fusion_amd.retrievers.bm25 import BM25
    W = ops.sort_max_n(torch.float64)
    cache = {}

    def get(spec):
        if spec not in cache:
            N = N_SPECS[spec](W)
            rng = np.random.default_rng(N)
            vocab = np.array([f"w{i}" for i in range(600)])
            p = 1.0 / np.arange(3, 603); p /= p.sum()
            docs = [" ".join(rng.choice(vocab, size=int(rng.integers(1, 6)), p=p)) for _ in range(N)]
            queries = [" ".join(rng.choice(vocab, size=int(rng.integers(1, 4)), p=p)) for _ in range(5)] + ["zzz"]
            exp = np.array([[x["corpus_id"] for x in r] for r in oracle.BM25(docs, 1.2, 0.0).search_all(queries, top_k=N)], dtype=np.int64)
            cache[spec] = (N, BM25(docs, 1.2, 0.0), queries, exp)
        return cache[spec]
    return W, get


@pytest.mark.parametrize("k_spec", list(K_SPECS))
@pytest.mark.parametrize("n_spec", ["W-1", "W", "W+1", "2W+1", "3W+1234"])
def test_ranked_positions_in_every_top_k_regime(n_spec, k_spec, cut_cases):
    """[Q, min(top_k, N)] == the first min(top_k, N) corpus ids of the oracle's search_all, for a corpus within one sort row, one over,
    and several rows long, and top_k from 0 past N -- the cut levels, the whole sort of a row longer than W, and both mixed; with the
    default budget and one query per chunk."""
    W, get = cut_cases
    N, m, queries, exp = get(n_spec)
    top_k = K_SPECS[k_spec](W, N)
    kk = min(top_k, N)
    for budget in ({}, {"budget_bytes": 1}):
        got = m.ranked_positions(queries, top_k=top_k, **budget)
        assert got.shape == (len(queries), kk), (N, top_k, budget)
        np.testing.assert_array_equal(got, exp[:, :kk], err_msg=f"N={N} top_k={top_k} {budget}")


# -- BM25.tune beyond one sort row, in budgeted chunks ---------------------------------------------------------------------------

@pytest.mark.parametrize("top_k", [1000, 20000])
@pytest.mark.parametrize("n_spec", ["W-1", "2W+17"])
def test_tune_beyond_one_sort_row(n_spec, top_k, oracle):
    """tune over a 2 x 2 (k1, b) grid == the loop it replaces (update_params -> ranked_positions ids -> oracle.Metrics) within 1e-12, and
    one query per chunk == the default call exactly.  Gold ids: exactly at ranks top_k - 1 and top_k of the first pair's lists, in the
    corpus's last stretch, duplicated, and outside the corpus; recall cut-offs on both sides of top_k."""
    from fusion_amd import ops
    from fusion_amd.retrievers.bm25 import BM25
    W = ops.sort_max_n(torch.float64)
    N = N_SPECS[n_spec](W)
    rng = np.random.default_rng(7 + N + top_k)
    vocab = np.array([f"w{i}" for i in range(900)])
    p = 1.0 / np.arange(2, 902); p /= p.sum()
    docs = [" ".join(rng.choice(vocab, size=int(rng.integers(1, 12)), p=p)) for _ in range(N)]
    queries = [" ".join(rng.choice(vocab, size=int(rng.integers(1, 5)), p=p)) for _ in range(6)] + ["zzz"]
    Q = len(queries)
    ids = np.arange(N, dtype=np.int64) * 3 + 11                            # 4 is not a corpus id
    k1s, bs = [0.9, 2.0], [0.0, 0.75]
    m = BM25(docs, k1s[0], bs[0])
    first = m.ranked_positions(queries, top_k=top_k + 1)
    exp_first = oracle.BM25(docs, k1s[0], bs[0]).search_all(queries, top_k=top_k + 1)
    np.testing.assert_array_equal(first, np.array([[x["corpus_id"] for x in r] for r in exp_first]))
    gold = [sorted({int(x) for x in rng.choice(ids, size=int(rng.integers(1, 4)), replace=False)}) for _ in range(Q)]
    for q in range(Q):
        gold[q] += [int(ids[first[q][top_k - 1]]), int(ids[first[q][top_k]])]   # the last entry kept and the first one cut
    gold[1] += [int(ids[N - 1]), int(ids[(N - 1) // W * W])]                # the last and first documents of the last stretch
    gold[2] += [gold[2][0], 4]                                             # a duplicate label and an id outside the corpus
    gold[3] = [int(ids[first[3][0]])]
    rk = [10, 100, top_k - 1, top_k]
    rows = m.tune(queries, gold, ids=ids, k1_range=k1s, b_range=bs, recall_at_k=rk, top_k=top_k)
    assert (m.k1, m.b) == (k1s[0], bs[0])
    assert list(rows[0]) == ["k1", "b"] + [f"recall@{k}" for k in rk] + ["r-precision"]
    ev = oracle.Metrics(recall_at_k=rk)
    for r, (k1, b) in zip(rows, itertools.product(k1s, bs)):
        m.update_params(k1, b)
        ranked = [[int(ids[j]) for j in row] for row in m.ranked_positions(queries, top_k=top_k)]
        assert len(ranked[0]) == min(top_k, N)
        e = ev.compute_all_metrics(gold, ranked)
        assert (r["k1"], r["b"]) == (k1, b)
        for name, v in e.items():
            assert abs(r[name] - float(v)) <= 1e-12, (N, top_k, k1, b, name, r[name], v)
    m.update_params(k1s[0], bs[0])
    assert m.tune(queries, gold, ids=ids, k1_range=k1s, b_range=bs, recall_at_k=rk, top_k=top_k, budget_bytes=1) == rows
