"""The streamed lexical top-k (csrc/bm25_stream.hip, ops.TopkStream64, TFIDF.search_topk(streaming=True), ShardedLexicalIndex) against the
route that existed before it: scores() for the kernels, search_topk(streaming=False) for the lists.  No tolerance anywhere: ids, float64
scores and their float32 roundings are compared bit for bit."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CLASSES = ("BM25", "AtireBM25", "TFIDF")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def synthetic_text(rng, n_docs, lo, hi, vocab_size=3000):
    vocab = np.array([f"w{i}" for i in range(vocab_size)])
    p = 1.0 / np.arange(1, vocab_size + 1); p /= p.sum()
    sizes = rng.integers(lo, hi, n_docs)
    words = rng.choice(vocab, size=int(sizes.sum()), p=p)
    cut = np.cumsum(sizes)[:-1]
    return [" ".join(w) for w in np.split(words, cut)]


def make(name, docs, **kw):
    from fusion_amd.retrievers import bm25
    cls = getattr(bm25, name)
    return cls(docs, **kw) if name == "TFIDF" else cls(docs, 1.5, 0.75, **kw)


def bits(t):
    """float tensors as their integer bit patterns (so that -0.0 != 0.0 and NaN == NaN in a comparison)."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_lists(got, want, what):
    np.testing.assert_array_equal(got.ids.cpu().numpy(), want.ids.cpu().numpy(), err_msg=f"{what}: ids")
    np.testing.assert_array_equal(bits(got.scores64), bits(want.scores64), err_msg=f"{what}: scores64")
    np.testing.assert_array_equal(bits(got.scores), bits(want.scores), err_msg=f"{what}: scores")
    assert got.lens.tolist() == want.lens.tolist(), what


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(20)
    docs = synthetic_text(rng, 40_003, 3, 30)
    queries = synthetic_text(rng, 10, 2, 8) + ["zzz qqq", "", " ".join(synthetic_text(rng, 1, 300, 301)[0].split())]
    assert len(queries[-1].split()) == 300 and len(set(queries[-1].split())) < 300      # two term batches, with repeats
    return docs, queries


# ---- 1. a range's plane is the full plane's columns -------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "binary_search"])
@pytest.mark.parametrize("name", CLASSES)
def test_range_plane_equals_the_full_planes_columns(name, table, corpus, ops):
    docs, queries = corpus
    S = ops.lexical_slice_docs("tfidf" if name == "TFIDF" else "pv")
    N = 3 * S + 17
    m = make(name, docs[:N], **({} if table else {"slice_table_max_bytes": 0}))
    assert (m.slice_off is not None) == table
    full = m.scores(queries)
    qoff, flat = m._query_csr(queries)
    src = ops._lexical_source(m, qoff, flat, 0)
    assert src.grain == S and src.unordered and src.mark == "shard_lexical_filter" and src.n == N
    for lo, hi in ((0, S), (S, 3 * S), (2 * S, N), (0, N), (S, S), (N - 17, N)):
        plane, base = src.plane(lo, hi)
        assert base == lo and tuple(plane.shape) == (len(queries), hi - lo) and plane.dtype == torch.float64
        np.testing.assert_array_equal(bits(plane), bits(full[:, lo:hi]), err_msg=f"{name} [{lo}, {hi})")
    assert float(full[10].abs().max()) == 0.0 and float(full[11].abs().max()) == 0.0       # out of vocabulary / empty: all zeros
    with pytest.raises(ValueError):
        src.plane(17, N)                                                                   # off the slice grid


# ---- 2. the filter kernel on its own ----------------------------------------------------------------------------------------------------
def _filter_buffers(Q, cap, tau, guard=4096):
    s = torch.full((Q * cap + guard,), -7.0, dtype=torch.float64, device="cuda")
    i = torch.full((Q * cap + guard,), -7, dtype=torch.int64, device="cuda")
    st = types.SimpleNamespace(tau=tau.contiguous(), cand_s=s[:Q * cap].view(Q, cap), cand_i=i[:Q * cap].view(Q, cap),
                               cand_len=torch.zeros(Q, dtype=torch.int32, device="cuda"), overflow=torch.zeros(1, dtype=torch.int32, device="cuda"))
    return st, s, i


@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "binary_search"])
@pytest.mark.parametrize("name", ["BM25", "TFIDF"])
def test_filter_kernel_alone(name, table, corpus, ops):
    docs, queries = corpus
    S = ops.lexical_slice_docs("tfidf" if name == "TFIDF" else "pv")
    N, ID0 = 3 * S + 17, 2**33
    m = make(name, docs[:N], **({} if table else {"slice_table_max_bytes": 0}))
    full = m.scores(queries)
    Q = len(queries)
    qoff, flat = m._query_csr(queries)
    src = ops._lexical_source(m, qoff, flat, ID0)
    lo, hi = S, N
    n = hi - lo
    # tau = -inf, room for everything: every document of the range, with the plane's bits
    st, _, _ = _filter_buffers(Q, n, torch.full((Q,), float("-inf"), dtype=torch.float64, device="cuda"))
    src.filter(st, lo, hi)
    assert st.cand_len.tolist() == [n] * Q and int(st.overflow) == 0
    by_id = torch.argsort(st.cand_i, dim=1)
    np.testing.assert_array_equal(torch.gather(st.cand_i, 1, by_id).cpu().numpy(), np.broadcast_to(np.arange(ID0 + lo, ID0 + hi), (Q, n)))
    np.testing.assert_array_equal(bits(torch.gather(st.cand_s, 1, by_id)), bits(full[:, lo:hi]))
    # tau = each row's median: exactly {score > tau}
    tau = full[:, lo:hi].median(dim=1).values
    st, _, _ = _filter_buffers(Q, n, tau)
    src.filter(st, lo, hi)
    want = full[:, lo:hi] > tau[:, None]
    assert st.cand_len.tolist() == want.sum(1).tolist() and int(st.overflow) == 0
    for q in range(Q):
        c = int(st.cand_len[q])
        got = st.cand_i[q, :c].sort().values - ID0 - lo
        np.testing.assert_array_equal(got.cpu().numpy(), torch.nonzero(want[q]).flatten().cpu().numpy())
        order = torch.argsort(st.cand_i[q, :c])
        np.testing.assert_array_equal(bits(st.cand_s[q, :c][order]), bits(full[q, lo:hi][want[q]]))
    # cap = 64 with more survivors: nothing at or past cap.  Rows 10 and 11 (no term in the vocabulary: all scores 0.0, none beats tau = 0)
    # stay untouched behind the rows that overflow, as does the guard behind the last row.
    cap = 64
    tau0 = torch.zeros(Q, dtype=torch.float64, device="cuda")
    survivors = (full[:, lo:hi] > 0).sum(1).tolist()
    assert survivors[12] > cap and sum(x > cap for x in survivors) >= 5 and survivors[10:12] == [0, 0]
    st, raw_s, raw_i = _filter_buffers(Q, cap, tau0)
    src.filter(st, lo, hi)
    assert int(st.overflow) == 1 and st.cand_len.tolist() == survivors
    assert bool((raw_s[Q * cap:] == -7.0).all()) and bool((raw_i[Q * cap:] == -7).all())
    for q in range(Q):
        c = min(survivors[q], cap)
        assert bool((st.cand_s[q, c:] == -7.0).all()) and bool((st.cand_i[q, c:] == -7).all())      # slots nobody owned are untouched
        if c:                                                    # what was stored is real: (score, id) pairs of survivors, no id twice
            ids = st.cand_i[q, :c] - ID0
            assert int(ids.min()) >= lo and int(ids.max()) < hi and ids.unique().numel() == c
            np.testing.assert_array_equal(bits(st.cand_s[q, :c]), bits(full[q][ids]))
            assert bool((st.cand_s[q, :c] > 0).all())


def boundary_corpus(S, cap):
    """S + 37 documents (one full slice and a ragged tail) and three one-word queries: every document holds "xx"; exactly cap hold "aa"
    and cap + 1 hold "bb", both over the two slices.  Returns (docs, queries, the documents of "aa", of "bb")."""
    N = S + 37
    rng = np.random.default_rng(9)
    hit1 = np.sort(np.concatenate([rng.choice(S, cap - 20, replace=False), S + rng.choice(37, 20, replace=False)]))
    hit2 = np.sort(np.concatenate([rng.choice(S, cap - 24, replace=False), S + rng.choice(37, 25, replace=False)]))
    words = [["xx"] * int(n) for n in rng.integers(1, 6, N)]
    for d in hit1:
        words[d].append("aa")
    for d in hit2:
        words[d] += ["bb", "bb"]
    return [" ".join(w) for w in words], ["xx", "aa", "bb"], hit1, hit2


@pytest.mark.parametrize("name", ["BM25", "TFIDF"])
def test_filter_at_exactly_cap_and_one_past_it(name, ops):
    """The filter epilogue at the capacity boundary.  Query 0's tau is its row maximum (ties do not enter: the rule is !(score <= tau)):
    no survivor; query 1 has exactly cap survivors above tau = 0, query 2 cap + 1 over both slices.  With query 2 switched off (tau = inf)
    every slot of query 1 is written and the flag stays 0; with it on the flag is 1, the count is cap + 1, and nothing lands at or past
    cap (the guard behind the buffers)."""
    S, cap, ID0 = ops.lexical_slice_docs("tfidf" if name == "TFIDF" else "pv"), 64, 2**34
    docs, queries, hit1, hit2 = boundary_corpus(S, cap)
    N, Q = len(docs), 3
    m = make(name, docs)
    full = m.scores(queries)
    tau = torch.tensor([float(full[0].max()), 0.0, 0.0], dtype=torch.float64, device="cuda")
    keep = [torch.nonzero(~(full[q] <= tau[q])).flatten().cpu().numpy() for q in range(Q)]
    assert [len(x) for x in keep] == [0, cap, cap + 1] and np.array_equal(keep[1], hit1) and np.array_equal(keep[2], hit2)
    assert hit2[0] < S <= hit2[-1] and hit1[0] < S <= hit1[-1]
    qoff, flat = m._query_csr(queries)
    src = ops._lexical_source(m, qoff, flat, ID0)
    off = tau.clone(); off[2] = float("inf")
    st, raw_s, raw_i = _filter_buffers(Q, cap, off, guard=cap)
    src.filter(st, 0, N)
    assert int(st.overflow) == 0 and st.cand_len.tolist() == [0, cap, 0]
    order = torch.argsort(st.cand_i[1])
    np.testing.assert_array_equal(st.cand_i[1][order].cpu().numpy(), hit1 + ID0)                     # every slot written
    np.testing.assert_array_equal(bits(st.cand_s[1][order]), bits(full[1][torch.from_numpy(hit1).cuda()]))
    assert bool((st.cand_s[[0, 2]] == -7.0).all()) and bool((raw_s[Q * cap:] == -7.0).all()) and bool((raw_i[Q * cap:] == -7).all())
    st, raw_s, raw_i = _filter_buffers(Q, cap, tau, guard=cap)
    src.filter(st, 0, N)
    assert int(st.overflow) == 1 and st.cand_len.tolist() == [0, cap, cap + 1]
    np.testing.assert_array_equal(st.cand_i[1].sort().values.cpu().numpy(), hit1 + ID0)
    ids = (st.cand_i[2] - ID0).cpu().numpy()
    assert len(set(ids.tolist())) == cap and set(ids.tolist()) <= set(hit2.tolist())                # cap distinct survivors ...
    np.testing.assert_array_equal(bits(st.cand_s[2]), bits(full[2][torch.from_numpy(ids).cuda()]))  # ... each with its own score
    assert bool((st.cand_s[0] == -7.0).all()) and bool((st.cand_i[0] == -7).all())
    assert bool((raw_s[Q * cap:] == -7.0).all()) and bool((raw_i[Q * cap:] == -7).all())            # nothing at or past cap


# ---- 3. streamed == plane route at the edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["head_plus_1", "three_heads", "40003"])
@pytest.mark.parametrize("name", CLASSES)
def test_streamed_equals_plane_route(name, size, corpus, ops, monkeypatch):
    docs, queries = corpus
    head = {"TFIDF": 14_336}.get(name, 10_752)
    N = {"head_plus_1": head + 1, "three_heads": 3 * head, "40003": 40_003}[size]
    m = make(name, docs[:N])
    assert m.head_docs(1000) == head and m.head_docs(1) == head
    for k in (1, 10, 100, 1000):
        want = m.search_topk(queries, k, streaming=False)
        assert m.last_path == "plane"
        got = m.search_topk(queries, k, streaming=True)
        assert m.last_path == "stream"
        assert_same_lists(got, want, f"{name} N={N} k={k}")
        if N > ops.sort_max_n(torch.float64):
            m.search_topk(queries, k)
            assert m.last_path == "stream"                       # the default beyond one sort row
        with monkeypatch.context() as mp:
            mp.setattr(type(m), "CAP", 256)                      # many folds, overflowed windows
            got = m.search_topk(queries, k, streaming=True)
            assert m.last_path == "stream"
            assert_same_lists(got, want, f"{name} N={N} k={k} CAP=256")


@pytest.mark.parametrize("name,k", [("BM25", 100), ("TFIDF", 80)])
def test_streamed_search_launches_one_kernel_per_planned_piece(name, k, corpus, ops):
    """The marks of a streamed _topk_device are the ones the piece planner predicts (as for the dense and the sparse index): the head's
    plane and the opening of the stream, one shard_lexical_filter per planned piece with a shard_topk_stream after every planned fold, the
    closing fold.  Head + three slices + 17 documents in feeds of two slices, one block of queries; CAP = 256 and k make the first window
    three slices long (128 * head / k rounded down to whole slices: 13,760 -> 10,752 for 'pv', 22,937 -> 21,504 for 'tfidf'), so the
    second feed starts inside it."""
    from helpers import planned_search_marks
    docs, queries = corpus
    S = ops.lexical_slice_docs("tfidf" if name == "TFIDF" else "pv")
    head = {"TFIDF": 14_336}.get(name, 10_752)
    N = head + 3 * S + 17
    m = make(name, docs[:N])
    m.CAP, m.CHUNK = 256, 2 * S
    assert m.head_docs(k) == head and m._streams(k) and len(queries) <= m.STREAM_QUERIES
    exp, folds, inside = planned_search_marks(ops, head, N, m.CHUNK, k, m.CAP, S, "shard_lexical", "shard_lexical_filter")
    assert exp.pop() == "allgather_merge"
    assert folds >= 1 and inside >= 1
    marks = []
    got_s, got_i = m._topk_device(queries, k, streaming=True, mark=marks.append)
    assert m.last_path == "stream" and marks == exp
    want_s, want_i = m._topk_device(queries, k, streaming=False)
    assert m.last_path == "plane"
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i.cpu().numpy())
    np.testing.assert_array_equal(bits(got_s), bits(want_s))


def test_stream_is_not_taken_where_it_cannot_run(corpus, ops):
    from fusion_amd.retrievers.bm25 import BM25
    docs, queries = corpus
    m = BM25(docs[:10_752], 1.5, 0.75)
    m.search_topk(queries, 10, streaming=True)
    assert m.last_path == "plane"                                # N == head: nothing left to stream
    m = BM25(docs[:12_000], 1.5, 0.75)
    m.search_topk(queries, 2000, streaming=True)
    assert m.last_path == "plane"                                # k > head / 8
    m.USE_POSTING_VALUES = False
    m.search_topk(queries, 10, streaming=True)
    assert m.last_path == "plane"                                # the per-posting expression has no range walk
    with pytest.raises(ValueError):
        ops.topk_merge64(torch.zeros((30, 2, 1000), dtype=torch.float64, device="cuda"), torch.zeros((30, 2, 1000), dtype=torch.int64, device="cuda"))


# ---- 4. ties and zeros ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tie_corpus():
    rng = np.random.default_rng(21)
    N = 40_003
    docs = synthetic_text(rng, N, 3, 30)
    common = rng.random(N) < 0.97
    docs = [d + " commun" if c else d for d, c in zip(docs, common)]          # one word in ~97 % of the documents: negative BM25 idf
    borders = {3583, 3584, 7167, 7168, 10_751, 10_752, 14_335, 14_336, 28_671, 28_672, 40_001, 40_002}    # slice, head and sort-row edges
    tied = sorted(borders | set(list(range(5, N, 20))[:2000 - len(borders)]))                              # (the grid 5 + 20 i misses every border)
    assert len(tied) == 2000
    for i in tied:
        docs[i] = "jumeau jumelle jumeau"                                     # 2,000 documents share one text, across head, windows and slices
    rare = [i for i in range(100, N, 997) if i not in set(tied)]
    for i in rare:
        docs[i] = docs[i] + " rarissime"                                      # a word in ~40 documents
    return docs, tied, rare


@pytest.mark.parametrize("name", CLASSES)
def test_ties_and_zeros(name, tie_corpus, ops):
    docs, tied, rare = tie_corpus
    N = len(docs)
    m = make(name, docs)
    queries = ["jumeau", "jumelle jumeau", "rarissime", "inconnu", "commun", "commun rarissime"]
    for k in (100, 1000):
        want = m.search_topk(queries, k, streaming=False)
        got = m.search_topk(queries, k, streaming=True)
        assert m.last_path == "stream"
        assert_same_lists(got, want, f"{name} k={k}")
        ids = got.ids.cpu().numpy()
        sc = got.scores64.cpu().numpy()
        np.testing.assert_array_equal(ids[0], tied[:k])                        # ties come out by ascending id
        np.testing.assert_array_equal(ids[1], tied[:k])
        assert len(set(sc[0].tolist())) == 1 and sc[0, 0] > 0
        assert sorted(ids[2, :len(rare)].tolist()) == rare and bool((sc[2, :len(rare)] > 0).all())
        rest = ids[2, len(rare):]                                              # fewer than k matches: the tail is zeros by ascending id
        assert bool((sc[2, len(rare):] == 0).all())
        np.testing.assert_array_equal(rest, [i for i in range(N) if i not in set(rare)][:k - len(rare)])
        np.testing.assert_array_equal(ids[3], np.arange(k))                    # out of vocabulary: ids 0 .. k-1
        assert bool((sc[3] == 0).all())
        if name == "BM25":                                                     # negative idf: the documents WITHOUT the word lead, with 0.0
            assert m.idf_host[m.vocab["commun"]] < 0
            without = np.array([i for i in range(N) if "commun" not in docs[i].split()])
            np.testing.assert_array_equal(ids[4], without[:k])
            assert bool((sc[4] == 0).all())
            head_zeros = int((without < m.head_docs(k)).sum())
            if k == 1000:
                assert head_zeros < k                                          # the head's k-th best was negative: zeros streamed in


# ---- 5. overflow ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLASSES)
def test_overflowed_windows_are_redone_exactly(name, corpus, ops, monkeypatch):
    docs, queries = corpus
    N = 30_011
    docs = list(docs[:N])
    first = 22_016                                                             # past either head, on no slice edge; 27 % of the corpus (BM25's idf stays positive)
    for i in range(first, N):                                                  # from here on every document matches, later ones better
        docs[i] = "filler " * 6 + "chaud " * (1 + (i - first) * 6 // (N - first))
    m = make(name, docs)
    qs = ["chaud"] + queries[:4]
    monkeypatch.setattr(type(m), "CAP", 256)
    for k in (10, 1000):
        want = m.search_topk(qs, k, streaming=False)
        got = m.search_topk(qs, k, streaming=True)
        assert m.last_path == "stream" and m.last_overflow > 0
        assert_same_lists(got, want, f"{name} k={k}")


# ---- 6. shards --------------------------------------------------------------------------------------------------------------------------
def test_eight_shards_equal_the_whole_index(ops):
    from fusion_amd.distributed import ShardedLexicalIndex, shard_bounds
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.bm25 import BM25, LexicalStats
    from fusion_amd.retrievers.hybrid import Aggregator
    rng = np.random.default_rng(22)
    N, G, ID0 = 90_001, 8, 2**33
    docs = synthetic_text(rng, N, 3, 30)
    queries = synthetic_text(rng, 16, 2, 8) + ["zzz"]
    whole = BM25(docs, 1.5, 0.75, id_base=ID0)
    shards = []
    for r in range(G):
        lo, hi = shard_bounds(N, G, r)
        shards.append((lo, hi, BM25(docs[lo:hi], 1.5, 0.75, device="cpu").stats()))
    stats = LexicalStats.merge([s for _, _, s in shards])
    assert stats == whole.stats()
    marks = []
    for k in (100, 1000):
        want = whole.search_topk(queries, k, streaming=False)
        assert int(want.ids.min()) >= ID0
        via_index = ShardedLexicalIndex(whole).search(queries, k)
        assert_same_lists(via_index, want, f"whole index k={k}")
        parts = []
        for lo, hi, _ in shards:
            idx = ShardedLexicalIndex(BM25(docs[lo:hi], 1.5, 0.75, stats=stats, id_base=ID0 + lo))
            parts.append(idx.local_topk(queries, k, mark=marks.append))
            assert idx.model.last_path == "stream"
        s, i = ops.topk_merge64(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
        got = RankedTopk.from_search(s.to(torch.float32), i, scores64=s)
        assert_same_lists(got, want, f"8 shards k={k}")
    assert {"shard_lexical", "shard_lexical_filter", "shard_topk_stream"} <= set(marks)
    # ... and the list goes into a fusion next to a dense one
    g = torch.Generator(device="cuda").manual_seed(5)
    d_sc = torch.rand((len(queries), 1000), generator=g, device="cuda").sort(dim=1, descending=True).values
    d_ids = ID0 + torch.stack([torch.randperm(N, generator=g, device="cuda")[:1000] for _ in queries])
    dense = RankedTopk.from_search(d_sc, d_ids)
    weights = {"bm25": 0.4, "dpr": 0.6}
    a = Aggregator.fuse_topk({"bm25": got, "dpr": dense}, "rrf", "none", weights, {}, topk=100)
    b = Aggregator.fuse_topk({"bm25": want, "dpr": dense}, "rrf", "none", weights, {}, topk=100)
    assert a.predictions() == b.predictions() and len(a.predictions()) == len(queries)
    assert all(ID0 <= x < ID0 + N for row in a.predictions() for x in row)


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------------
def test_the_same_search_twice_gives_identical_tensors(corpus, ops):
    from fusion_amd.retrievers.bm25 import BM25
    docs, queries = corpus
    m = BM25(docs, 1.5, 0.75)
    a = m.search_topk(queries, 1000, streaming=True)
    b = m.search_topk(queries, 1000, streaming=True)
    assert m.last_path == "stream"
    assert_same_lists(a, b, "second run")
