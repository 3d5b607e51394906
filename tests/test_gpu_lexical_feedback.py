"""Lexical pseudo-relevance feedback on the device (csrc/bm25_weighted.hip, csrc/feedback_lexical.hip and what is built on them) against
the float64 restatement of tests/lexical_feedback_cases.py.  No tolerance anywhere: terms, lengths, float64 weights, ids and scores are
compared bit for bit."""
import numpy as np
import pytest
import torch

import lexical_feedback_cases as lc

pytestmark = pytest.mark.gpu

CLASSES = ("BM25", "AtireBM25", "TFIDF")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    assert o.lexical_feedback_max_entries() == lc.E
    return o


def make(name, docs, **kw):
    from fusion_amd.retrievers import bm25
    cls = getattr(bm25, name)
    return cls(docs, **kw) if name == "TFIDF" else cls(docs, 1.5, 0.75, **kw)


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_MODELS = {}


def model_of(name, n_docs, seed=11):
    """One model per (class, size), shared by the tests that need it."""
    key = (name, n_docs, seed)
    if key not in _MODELS:
        docs = lc.synthetic_text(np.random.default_rng(seed), n_docs, 3, 12, vocab_size=500)
        _MODELS[key] = make(name, docs)
    return _MODELS[key]


def weighted(model, lists, weights):
    from fusion_amd.retrievers.bm25 import WeightedQueries
    off, flat = lc.csr(lists)
    w = np.array([x for ws in weights for x in ws] or [0.0], dtype=np.float64)
    return WeightedQueries(dev(off), dev(flat), dev(w))


def random_queries(rng, V, lengths):
    """Term-id lists of the given lengths with repetitions and -1 entries."""
    out = []
    for n in lengths:
        t = rng.integers(0, V, n)
        if n > 3:
            t[rng.integers(0, n, max(1, n // 9))] = -1
            t[1] = t[0]
        out.append(t.tolist())
    return out


# ---- 1. the weighted walk -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "binary_search"])
@pytest.mark.parametrize("name", ["BM25", "TFIDF"])
def test_unit_weights_give_the_unweighted_plane(name, table, ops):
    mode = "pv" if name == "BM25" else "tfidf"
    S, B = ops.lexical_slice_docs(mode), ops.lexical_weighted_terms(mode)
    rng = np.random.default_rng(3)
    for N in (S - 1, S, S + 1, 2 * S + 1):
        m = model_of(name, N)
        vals, idf = m.lexical_tables()
        V = len(m.vocab)
        off, flat = lc.csr(random_queries(rng, V, [0, 1, B - 1, B, B + 1, 2 * B + 1]))
        qoff, qt = dev(off), dev(flat)
        so = m.slice_off if table else None
        assert (so is not None) == table
        want = ops.lexical_scores_range(mode, m.toff, m.pdoc, vals, idf, qoff, qt, 6, N, slice_off=so)
        got = ops.lexical_scores_range(mode, m.toff, m.pdoc, vals, idf, qoff, qt, 6, N, slice_off=so, qw=torch.ones(flat.size, dtype=torch.float64, device="cuda"))
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{name} N = {N}")
        assert float(want.abs().sum()) > 0


@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "binary_search"])
@pytest.mark.parametrize("name", CLASSES)
def test_random_weights_against_the_restatement(name, table, ops):
    m = model_of(name, 7169 + 40)
    mode = m.lexical_mode()
    B = ops.lexical_weighted_terms(mode)
    rng = np.random.default_rng(9)
    lists = random_queries(rng, len(m.vocab), [0, 1, 7, B + 3, 2 * B + 1])
    weights = []
    for qt in lists:
        w = rng.normal(0, 1, len(qt))
        w[rng.random(len(qt)) < 0.15] = 0.0
        w[rng.random(len(qt)) < 0.1] = 5e-324 * 3                          # subnormal
        w[rng.random(len(qt)) < 0.05] = -0.0
        weights.append(w.tolist())
    wq = weighted(m, lists, weights)
    vals, idf = m.lexical_tables()
    got = ops.lexical_scores_range(mode, m.toff, m.pdoc, vals, idf, wq.qoff, wq.qterms, wq.Q, m.corpus_size,
                                   slice_off=m.slice_off if table else None, qw=wq.qw)
    want = lc.plane_ref(lc.host_index(m), list(zip(lists, weights)))
    np.testing.assert_array_equal(bits(got), bits(want))
    if table:
        np.testing.assert_array_equal(bits(m.scores_weighted(wq)), bits(want))
        with pytest.raises(ValueError, match="finite"):
            ops.lexical_scores_range(mode, m.toff, m.pdoc, vals, idf, wq.qoff, wq.qterms, wq.Q, m.corpus_size, qw=wq.qw * float("inf"))
        with pytest.raises(ValueError, match="weights for"):
            ops.lexical_scores_range(mode, m.toff, m.pdoc, vals, idf, wq.qoff, wq.qterms, wq.Q, m.corpus_size, qw=wq.qw[:-1])


@pytest.fixture(scope="module")
def long_corpus():
    """Just past one float64 sort row, with a run of 300 identical documents (equal scores) for the cut to fall into."""
    rng = np.random.default_rng(21)
    docs = lc.synthetic_text(rng, 35_543, 3, 12, vocab_size=500) + ["tiea tieb"] * 300
    perm = rng.permutation(len(docs))
    return [docs[i] for i in perm]


@pytest.mark.parametrize("name", ["BM25", "TFIDF"])
def test_streamed_equals_plane_route_for_weighted_queries(name, long_corpus, ops):
    assert len(long_corpus) > ops.sort_max_n(torch.float64)
    m = make(name, long_corpus)
    v = m.vocab
    rng = np.random.default_rng(4)
    lists = [[v["tiea"]], [v["tieb"], v["w7"], -1, v["w7"]], rng.integers(0, len(v), 9).tolist(), []]
    weights = [[0.5], [0.25, 1.5, 3.0, -0.5], rng.uniform(-0.2, 2.0, 9).tolist(), []]
    wq = weighted(m, lists, weights)
    k = 100                                                               # inside the run of 300 equal scores of queries 0 and 1
    plane = m.search_topk_weighted(wq, k, streaming=False)
    assert m.last_path == "plane"
    stream = m.search_topk_weighted(wq, k, streaming=True)
    assert m.last_path == "stream"
    ids, sc = lc.topk_ref(lc.plane_ref(lc.host_index(m), list(zip(lists, weights))), k)
    for got, what in ((plane, "plane"), (stream, "stream")):
        np.testing.assert_array_equal(got.ids.cpu().numpy(), ids, err_msg=what)
        np.testing.assert_array_equal(bits(got.scores64), bits(sc), err_msg=what)
        np.testing.assert_array_equal(bits(got.scores), bits(sc.astype(np.float32)), err_msg=what)
        assert got.lens.tolist() == [k] * 4
    assert len(set(sc[0].tolist())) == 1                                  # the cut falls inside a tie run: the lowest ids win


# ---- 2. the feedback kernel against the restatement ---------------------------------------------------------------------------------------
def run_rows(ops, foff, fterm, fval, queries, fb_ids, fb_len, coef, alpha, beta, m, id_base=0, guard=8):
    """fz_lexical_feedback_rows_f64 called directly on guarded buffers -> (terms [Q, width], weights, out_len, flag); asserts that every
    element of the rows was written and nothing beyond `width`."""
    from fusion_amd import _lib
    Q, F = fb_ids.shape
    off, flat = lc.csr(queries)
    width = max([len(q) for q in queries] or [0]) + m
    ldo = width + guard
    out_t = torch.full((Q, ldo), 777, dtype=torch.int32, device="cuda")
    out_w = torch.full((Q, ldo), 123.5, dtype=torch.float64, device="cuda")
    out_len = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    flag = torch.full((1,), 55, dtype=torch.int32, device="cuda")
    t = [dev(x) for x in (foff, fterm, fval, off, flat, fb_ids, coef)]
    flen = None if fb_len is None else dev(np.asarray(fb_len, dtype=np.int32))
    P = ops._ptr
    rc = _lib.lib().fz_lexical_feedback_rows_f64(P(t[0]), P(t[1]), P(t[2]), len(foff) - 1, id_base, P(t[3]), P(t[4]), Q, P(t[5]), F, P(flen),
                                                 P(t[6]), F, F, float(alpha), float(beta), m, P(out_t), P(out_w), ldo, width, P(out_len),
                                                 P(flag), ops._stream(out_t))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out_t[:, width:] == 777).all()) and bool((out_w[:, width:] == 123.5).all()), "written outside width"
    return out_t[:, :width].cpu().numpy(), out_w[:, :width].cpu().numpy(), out_len.cpu().numpy(), int(flag.item())


def assert_rows(got, ref, what=""):
    terms, w, n, flag = got
    exp, eflag = ref
    assert flag == eflag, (what, flag, eflag)
    width = terms.shape[1]
    for q, (et, ew) in enumerate(exp):
        assert n[q] == len(et), (what, q, n[q], len(et))
        np.testing.assert_array_equal(terms[q], np.array(et + [-1] * (width - len(et)), dtype=np.int32), err_msg=f"{what} q{q} terms")
        np.testing.assert_array_equal(bits(w[q]), bits(np.array(ew + [0.0] * (width - len(ew)), dtype=np.float64)), err_msg=f"{what} q{q} weights")


def check_rows(ops, rows, N, queries, fb_ids, fb_len, coef, alpha, beta, m, id_base=0, what=""):
    got = run_rows(ops, *rows, queries, fb_ids, fb_len, coef, alpha, beta, m, id_base)
    assert_rows(got, lc.feedback_ref(*rows, N, id_base, queries, fb_ids, fb_len, coef, alpha, beta, m), what)
    return got


def test_feedback_row_lengths_at_the_wave_and_workgroup_edges(ops):
    rng = np.random.default_rng(31)
    T = lc.FB_THREADS
    lens = [0, 1, 63, 64, 65, T - 1, T, T + 1]                            # 3,265 entries in all
    rows = lc.random_rows(rng, lens, 6000, signed=True)
    ids = np.array([list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0], [5, 5, 6, 0, 1, 1, 2, 3]], dtype=np.int64) + 50
    coef = rng.uniform(0.05, 1.0, ids.shape).astype(np.float32)
    queries = [rows[1][:40].tolist() + [-1, -1], [], [int(rows[1][-1])] * 3]
    for m in (0, 10, 5000):
        check_rows(ops, rows, 8, queries, ids, [8, 8, 7], coef, 1.0, 0.5, m, id_base=50, what=f"m = {m}")


def test_feedback_slot_counts_at_the_depth_and_batch_edges(ops):
    rng = np.random.default_rng(32)
    N, U, S = 300, lc.FB_DEPTH, lc.FB_SLOTS
    rows = lc.random_rows(rng, rng.integers(0, 13, N), 900)
    queries = [rng.integers(0, 900, 5).tolist(), [], [-1]]
    for F in (0, 1, U - 1, U, U + 1, S - 1, S, S + 1):
        ids = rng.integers(-2, N + 2, (3, F)).astype(np.int64)           # a few ids outside the index: skipped slots
        coef = rng.uniform(0.05, 1.0, (3, F)).astype(np.float32)
        check_rows(ops, rows, N, queries, ids, [F, max(F - 1, 0), F], coef, 0.75, 0.5, 12, what=f"F = {F}")
        check_rows(ops, rows, N, queries, ids, None, coef, 0.75, 0.5, 12, what=f"F = {F}, no fb_len")


def test_feedback_capacity_rule(ops):
    rng = np.random.default_rng(33)
    E = lc.E
    half = E // 2
    rows = lc.random_rows(rng, [half, half - 1, 1, 2, 0, E, E + 1, 1], 3 * E)
    #          slots -> entries            flag
    cases = [([1, 0], E - 1, 0), ([0, 1, 2], E, 0), ([0, 1, 4, 2], E, 0), ([0, 1, 3, 2, 7], E - 1, 1), ([0, 1, 2, 7, 4], E, 1), ([5], E, 0),
             ([5, 4, 2], E, 1), ([6, 2], 0, 1), ([0, 6, 2], half, 1)]
    F = 5
    ids = np.full((len(cases), F), -1, dtype=np.int64)
    for q, (slots, _, _) in enumerate(cases):
        ids[q, :len(slots)] = slots
    coef = rng.uniform(0.05, 1.0, ids.shape).astype(np.float32)
    queries = [[int(rows[1][0])]] * len(cases)
    ref = lc.feedback_ref(*rows, 8, 0, queries, ids, None, coef, 1.0, 0.5, 20)
    assert ref[1] == lc.CUT
    got = run_rows(ops, *rows, queries, ids, None, coef, 1.0, 0.5, 20)
    assert_rows(got, ref)
    for q, (slots, _, flag) in enumerate(cases):                         # each query on its own: its own flag
        one = run_rows(ops, *rows, queries[:1], ids[q:q + 1], None, coef[q:q + 1], 1.0, 0.5, 20)
        assert one[3] == flag, (q, slots)
        assert_rows(one, lc.feedback_ref(*rows, 8, 0, queries[:1], ids[q:q + 1], None, coef[q:q + 1], 1.0, 0.5, 20), f"case {q}")
    # every counted term selected, at the capacity: C = E candidates sorted
    big = run_rows(ops, *rows, [[]], np.array([[5]], dtype=np.int64), None, np.ones((1, 1), np.float32), 1.0, 1.0, E + 3)
    assert_rows(big, lc.feedback_ref(*rows, 8, 0, [[]], np.array([[5]], dtype=np.int64), None, np.ones((1, 1), np.float32), 1.0, 1.0, E + 3))
    assert big[2][0] == E


def test_feedback_selection_edges(ops):
    rng = np.random.default_rng(34)
    foff, fterm, fval = lc.random_rows(rng, [30, 25, 40, 7], 200)
    rows = (foff, fterm, fval)
    ids = np.array([[0, 1, 2, 3]], dtype=np.int64)
    coef = rng.uniform(0.1, 1.0, (1, 4)).astype(np.float32)
    ref, _ = lc.feedback_ref(*rows, 4, 0, [[3, 3]], ids, None, coef, 1.0, 0.5, 1000)
    C = len(ref[0][0]) - 2
    assert 10 < C <= 102
    for m in (0, 1, C - 1, C, C + 1):                                     # C = m + 1, C = m, C < m
        check_rows(ops, rows, 4, [[3, 3]], ids, None, coef, 1.0, 0.5, m, what=f"m = {m}")
    # C = 0: every term of the rows is the query's own, or its sum is not positive
    check_rows(ops, (foff, fterm, -fval), 4, [[]], ids, None, coef, 1.0, 0.5, 10, what="all negative")
    assert check_rows(ops, rows, 4, [sorted(set(fterm.tolist()))], ids, None, coef, 1.0, 0.5, 10, what="all query terms")[2][0] == len(set(fterm.tolist()))
    # all candidates equal: the lowest terms win, in ascending order
    eq = (foff, fterm, np.ones_like(fval))
    one = np.array([[0, 2]], dtype=np.int64)                              # rows 0 and 2
    ref, _ = lc.feedback_ref(*eq, 4, 0, [[]], one, None, np.full((1, 2), 0.5, np.float32), 1.0, 0.5, 10)
    if len(set(fterm[:30].tolist()) & set(fterm[55:95].tolist())) == 0:
        assert ref[0][0] == sorted(set(fterm[:30].tolist()) | set(fterm[55:95].tolist()))[:10] and set(ref[0][1]) == {0.5}
    check_rows(ops, eq, 4, [[]], one, None, np.full((1, 2), 0.5, np.float32), 1.0, 0.5, 10, what="all equal")
    # a tie run across the cut: three strong terms, then a run of equal sums
    tv = np.ones_like(fval); tv[[2, 11, 17]] = [4.0, 3.0, 2.0]
    for m in (2, 3, 4, 9):
        check_rows(ops, (foff, fterm, tv), 4, [[]], ids[:, :1], None, np.ones((1, 1), np.float32), 1.0, 0.5, m, what=f"tie run, m = {m}")


def test_feedback_slot_rules_cancellation_and_empty_queries(ops):
    # terms 1 .. 6; documents: A, its negation B, and C
    A, B, Cd = {1: 1.5, 2: 2.0, 3: 0.25}, {1: -1.5, 2: -2.0, 5: 1.0}, {2: 1.0, 6: 3.0, 4: -1.0}
    docs = [A, B, Cd, {}]
    foff = np.zeros(5, dtype=np.int64); np.cumsum([len(d) for d in docs], out=foff[1:])
    rows = (foff, np.array([t for d in docs for t in d], dtype=np.int32), np.array([v for d in docs for v in d.values()]))
    ids = np.array([[10, 11, 12, 13],      # A + B: terms 1 and 2 cancel to exactly 0.0 and are no candidates
                    [10, 10, 12, 10],      # a document in two (three) slots counts each time
                    [9, 14, -1, 12],       # skipped slots: ids outside [id_base, id_base + N)
                    [10, 11, 12, 13],      # fb_len = 0: no slot -- the original entries at alpha only
                    [12, 10, 11, 13],      # an empty query
                    [13, 13, 13, 13]], dtype=np.int64)
    coef = np.full(ids.shape, 0.5, dtype=np.float32)
    queries = [[7], [3, 3, -1], [6], [1, -1, 1], [], [2]]
    got = check_rows(ops, rows, 4, queries, ids, [2, 4, 4, 0, 4, 4], coef, 0.75, 2.0, 5, id_base=10)
    assert got[0][0].tolist()[:3] == [7, 5, 3] and got[1][3].tolist()[:3] == [0.75] * 3 and got[2][3] == 3 and got[2][5] == 1
    again = run_rows(ops, *rows, queries, ids, [2, 4, 4, 0, 4, 4], coef, 0.75, 2.0, 5, id_base=10)
    for a, b in zip(got[:3], again[:3]):                                  # two runs give the same bytes
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", CLASSES)
def test_index_sources_against_the_restatement(name, ops):
    """The rows read through the forward index (fpos -> pval, or ptf and idf); BM25's idf is negative for the commonest words here: such terms
    are never selected.  Two runs give the same bytes."""
    from fusion_amd.planes import RankedTopk
    m = model_of(name, 3000)
    ix = lc.host_index(m)
    if name == "BM25":                                                   # (AtireBM25's and TF-IDF's idf is positive)
        assert (m.idf_host <= 0).any() and (ix["val"] < 0).any()
    rng = np.random.default_rng(35)
    Q, k = 12, 20
    ids = rng.integers(0, 3000, (Q, k)).astype(np.int64)
    ids[0, 1] = ids[0, 0]
    sc = -np.sort(-rng.uniform(0, 9, (Q, k)), axis=1)
    lens = rng.integers(0, k + 1, Q).astype(np.int32); lens[:2] = [k, 0]
    topk = RankedTopk(ids=dev(ids), scores=dev(sc.astype(np.float32)), lens=dev(lens), scores64=dev(sc))
    queries = [" ".join(f"w{i}" for i in rng.integers(0, 40, n)) for n in rng.integers(0, 6, Q)]
    queries[3] += " zzz"
    qt = [[m.vocab.get(w, -1) for w in q.split()] for q in queries]
    rows = lc.forward_rows(ix)
    for weighting in ("uniform", "score"):
        from fusion_amd.feedback import coefficients
        fb_ids, fb_len, coef = coefficients(topk, 7, 1.0, weighting)
        ref, flags = lc.feedback_ref(*rows, 3000, 0, qt, fb_ids.cpu().numpy(), fb_len.cpu().numpy(), coef.cpu().numpy(), 1.0, 0.5, 6)
        wq = m.feedback(queries, topk, fb_docs=7, fb_terms=6, weighting=weighting)
        again = m.feedback(queries, topk, fb_docs=7, fb_terms=6, weighting=weighting)
        assert wq.flags == flags == 0
        off = np.cumsum([0] + [len(t) for t, _ in ref])
        assert wq.qoff.cpu().tolist() == off.tolist()
        assert wq.qterms.cpu().tolist() == [t for ts, _ in ref for t in ts]
        np.testing.assert_array_equal(bits(wq.qw), bits(np.array([x for _, ws in ref for x in ws])))
        assert torch.equal(wq.qterms, again.qterms) and torch.equal(wq.qw.view(torch.int64), again.qw.view(torch.int64))
    words = m.expansion_words(wq)
    assert [w for w, _ in words[3]][:len(queries[3].split())] == [w if w in m.vocab else None for w in queries[3].split()]


# ---- 3. search_feedback -------------------------------------------------------------------------------------------------------------------
def assert_same_lists(got, want, what):
    np.testing.assert_array_equal(got.ids.cpu().numpy(), want.ids.cpu().numpy(), err_msg=f"{what}: ids")
    np.testing.assert_array_equal(bits(got.scores64), bits(want.scores64), err_msg=f"{what}: scores64")
    np.testing.assert_array_equal(bits(got.scores), bits(want.scores), err_msg=f"{what}: scores")
    assert got.lens.tolist() == want.lens.tolist(), what


@pytest.mark.parametrize("name", CLASSES)
def test_search_feedback_is_its_three_steps_and_the_restatements_lists(name, ops):
    m = model_of(name, 3000)
    queries = ["w3 w17 w40", "w5", "w2 w2 zzz w9", ""]
    k = 50
    got = m.search_feedback(queries, k, fb_docs=8, fb_terms=7, alpha=0.9, beta=0.4)
    first = m.search_topk(queries, k)
    wq = m.feedback(queries, first, fb_docs=8, fb_terms=7, alpha=0.9, beta=0.4)
    assert_same_lists(got, m.search_topk_weighted(wq, k), "three steps")
    qt = [[m.vocab.get(w, -1) for w in q.split()] for q in queries]
    rfirst, ids, sc, exp = lc.search_feedback_ref(lc.host_index(m), qt, k, 8, 7, 0.9, 0.4)
    np.testing.assert_array_equal(first.ids.cpu().numpy(), rfirst)
    assert wq.qterms.cpu().tolist()[:sum(len(t) for t, _ in exp)] == [t for ts, _ in exp for t in ts]
    np.testing.assert_array_equal(got.ids.cpu().numpy(), ids)
    np.testing.assert_array_equal(bits(got.scores64), bits(sc))
    assert len(exp[0][0]) == 3 + 7 and exp[3][0] and exp[3][1][0] == 0.4      # (an empty query expands from its list's first documents too)
    # alpha = 1, fb_terms = 0: the first search's lists
    assert_same_lists(m.search_feedback(queries, k, alpha=1.0, fb_terms=0), first, "alpha = 1, fb_terms = 0")
    assert_same_lists(m.search_feedback(queries, k, streaming=False, alpha=1.0, fb_terms=0), first, "plane route")


def test_ranker_bm25_search_with_feedback(ops):
    from fusion_amd.retrievers.hybrid import Ranker
    rng = np.random.default_rng(41)
    docs = lc.synthetic_text(rng, 700, 3, 12, vocab_size=300)
    corpus = {1000 + 3 * i: d for i, d in enumerate(docs)}
    queries = ["w3 w17", "w5 w5 w1", "zzz"]
    fbk = dict(fb_docs=6, fb_terms=5, alpha=1.0, beta=0.5)
    rs = Ranker.bm25_search(queries, corpus, False, 1.5, 0.75, as_device=True, feedback=fbk)
    m = make("BM25", docs)
    want = m.search_feedback(queries, len(docs), **fbk)
    np.testing.assert_array_equal(rs.order.cpu().numpy()[:, :len(docs)], want.ids.cpu().numpy())
    np.testing.assert_array_equal(bits(torch.gather(rs.scores64, 1, rs.order.long())), bits(want.scores64))
    cut = Ranker.bm25_search(queries, corpus, False, 1.5, 0.75, return_topk=10, feedback=fbk)
    assert [[e["corpus_id"] for e in row] for row in cut] == (1000 + 3 * want.ids[:, :10].cpu().numpy()).tolist()
    # feedback=None takes today's path: the same as a call without the keyword
    a = Ranker.bm25_search(queries, corpus, False, 1.5, 0.75, as_device=True, feedback=None)
    b = Ranker.bm25_search(queries, corpus, False, 1.5, 0.75, as_device=True)
    assert torch.equal(a.order, b.order) and torch.equal(a.scores64.view(torch.int64), b.scores64.view(torch.int64)) and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
    assert not torch.equal(rs.order, b.order)


# ---- 4. the expansions do not depend on the number of shards ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["BM25", "TFIDF"])
def test_expansions_are_the_same_for_one_two_and_three_shards(name, ops):
    from fusion_amd import feedback as fb
    from fusion_amd.distributed import ShardedLexicalIndex, shard_bounds
    from fusion_amd.retrievers.bm25 import LexicalStats, WeightedQueries
    rng = np.random.default_rng(51)
    docs = lc.synthetic_text(rng, 900, 3, 12, vocab_size=400)
    queries = ["w3 w17 w40", "w5", "w2 w2 zzz w9", ""]
    whole = make(name, docs)
    first = whole.search_topk(queries, 30)
    kw = dict(fb_docs=9, fb_terms=8, alpha=1.0, beta=0.5)
    want = whole.feedback(queries, first, **kw)
    want_words = whole.expansion_words(want)
    assert sum(len(r) for r in want_words) == sum(len(q.split()) for q in queries) + 8 * 4
    fb_ids, fb_len, coef = fb.coefficients(first, 9, 1.0, "uniform")
    for G in (1, 2, 3):
        bounds = [shard_bounds(len(docs), G, r) for r in range(G)]
        stats = LexicalStats.merge([make(name, docs[lo:hi]).stats() for lo, hi in bounds])
        shards = [ShardedLexicalIndex(make(name, docs[lo:hi], stats=stats, id_base=lo)) for lo, hi in bounds]
        for s in shards:
            s.model.build_forward()
        L = max(int(fb.lexical_row_lengths(s.model, fb_ids).max()) for s in shards)
        terms = values = None
        for s in shards:
            t, v = fb.pack_lexical_rows(s.model, s._term_space()[1], fb_ids, L)
            terms, values = (t, v) if terms is None else (torch.maximum(terms, t), torch.maximum(values, v))
        foff, fterm, fval, slots = fb.lexical_rows(terms, values)
        words, _, _, gid = shards[0]._term_space()
        assert words == list(whole.vocab)                                 # contiguous shards: the whole corpus's own term ids
        off, flat = lc.csr([[gid.get(w, -1) for w in q.split()] for q in queries])
        wq = WeightedQueries(*ops.lexical_feedback_rows(foff, fterm, fval, dev(off), dev(flat), slots, fb_len, coef, 1.0, 0.5, 8))
        assert shards[0].expansion_words(wq) == want_words, G
        assert torch.equal(wq.qterms, want.qterms) and torch.equal(wq.qw.view(torch.int64), want.qw.view(torch.int64)) and torch.equal(wq.qoff, want.qoff)
        # a shard's own walk takes its local ids: the word where it has it, -1 where it lacks it
        local = shards[-1].localize(wq)
        lw = list(shards[-1].model.vocab)
        assert [(lw[t] if t >= 0 else None) for t in local.qterms.cpu().tolist()] == \
            [(w if w in shards[-1].model.vocab else None) for row in want_words for w, _ in row]
    one = ShardedLexicalIndex(whole)
    g = one.global_feedback(queries, first, **kw)
    assert torch.equal(g.qterms, want.qterms) and torch.equal(g.qw.view(torch.int64), want.qw.view(torch.int64))
    assert_same_lists(one.search_feedback(queries, 30, **kw), whole.search_topk_weighted(want, 30), "one shard")


# ---- 5. the planted cluster ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", lc.PLANTED_SEEDS)
def test_planted_cluster_lists_are_the_restatements(seed, ops):
    """tests/test_lexical_feedback_cpu.py shows the recall gain on the restatement alone; here the device's lists ARE the restatement's."""
    docs, queries, cluster = lc.planted_cluster(seed)
    m = make("TFIDF", docs)
    qt = [[m.vocab.get(w, -1) for w in q.split()] for q in queries]
    first, second, sc, _ = lc.search_feedback_ref(lc.host_index(m), qt, lc.PLANTED_K, 10, 10, 1.0, 0.5)
    np.testing.assert_array_equal(m.search_topk(queries, lc.PLANTED_K).ids.cpu().numpy(), first)
    got = m.search_feedback(queries, lc.PLANTED_K)
    np.testing.assert_array_equal(got.ids.cpu().numpy(), second)
    np.testing.assert_array_equal(bits(got.scores64), bits(sc))
    assert sum(lc.cluster_recall(second, cluster)) > sum(lc.cluster_recall(first, cluster))
