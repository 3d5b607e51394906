"""Gold ranks as counts on the posting walk (csrc/bm25_count.hip, ops.lexical_doc_scores / lexical_count, TFIDF.doc_scores / count_before /
gold_ranks, BM25.tune(counting=True), ShardedLexicalIndex.gold_ranks) against what existed before them: scores() for the scores, the full
`rank` plane of search_device for the ranks (every corpus here fits one sort row, or the plane route of tune is the yardstick).  No
tolerance anywhere: ranks and counts are integers, scores are compared by their bit patterns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CLASSES = ("BM25", "AtireBM25", "TFIDF")
ID0 = 1 << 33


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def synthetic_text(rng, n_docs, lo, hi, vocab_size=3000):
    """tests/test_gpu_bm25_stream.py's corpus: Zipf-distributed words w0 .. w2999, lo .. hi - 1 words per document."""
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
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int64) if a.dtype.kind == "f" else a


def slice_docs(ops, name):
    return ops.lexical_slice_docs("tfidf" if name == "TFIDF" else "pv")


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(20)
    docs = synthetic_text(rng, 40_003, 3, 30)
    queries = synthetic_text(rng, 10, 2, 8) + ["zzz qqq", "", " ".join(synthetic_text(rng, 1, 300, 301)[0].split()), "w0", "w0 w2999 w0"]
    assert len(queries[12].split()) == 300 and len(set(queries[12].split())) < 300      # two term batches, with repeats
    return docs, queries


OOV, EMPTY = 10, 11      # rows of `queries` whose every score is 0.0


@pytest.fixture(scope="module")
def setups(corpus, ops):
    """(name, table) -> model of N = 3 S + 17 documents, its full float64 plane and rank plane: computed once, never changed."""
    docs, queries = corpus
    cache = {}

    def get(name, table):
        if (name, table) not in cache:
            S = slice_docs(ops, name)
            N = 3 * S + 17
            assert N <= ops.sort_max_n(torch.float64)
            m = make(name, docs[:N], **({} if table else {"slice_table_max_bytes": 0}))
            assert (m.slice_off is not None) == table
            rs = m.search_device(queries)
            full = rs.scores64.clone()
            rank = rs.rank.long().clone()
            assert tuple(full.shape) == (len(queries), N) == tuple(rank.shape)
            assert float(full[OOV].abs().max()) == 0.0 and float(full[EMPTY].abs().max()) == 0.0
            cache[(name, table)] = (m, S, N, full, rank, gold_pool(full, rank, S, N))
        return cache[(name, table)]
    return get


def gold_pool(full, rank, S, N):
    """[Q, 13] positions, a column per class: the rank-0 document, the first document scoring exactly 0.0 (document 0 if none), the
    lowest-scoring document (negative under BM25 for a term most documents hold), document N - 1, one inside the 17-document tail, the
    first and last document of every slice, and -1 (not in the index)."""
    Q, dev = full.shape[0], full.device
    cols = [rank.argmin(1), (full == 0).to(torch.int8).argmax(1), full.argmin(1)]
    cols += [torch.full((Q,), v, dtype=torch.int64, device=dev) for v in (N - 1, N - 9, 0, S - 1, S, 2 * S - 1, 2 * S, 3 * S - 1, 3 * S, -1)]
    pool = torch.stack(cols, 1)
    assert bool((torch.gather(rank, 1, pool[:, :1]) == 0).all())
    return pool


def windows(pool, G):
    """Every column of the pool, G at a time (wrapping round): [Q, G] position tensors."""
    P = pool.shape[1]
    return [pool[:, [(s + i) % P for i in range(G)]].contiguous() for s in range(0, P, G)]


def want_ranks(rank, pos):
    return torch.where(pos >= 0, torch.gather(rank, 1, pos.clamp(min=0)), -1)


# ---- 1. doc_scores has the plane's bits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "binary_search"])
@pytest.mark.parametrize("name", CLASSES)
def test_doc_scores_are_the_planes_entries_bit_for_bit(name, table, setups, corpus):
    _, queries = corpus
    m, S, N, full, rank, pool = setups(name, table)
    got = m.doc_scores(queries, pool)
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(pool.shape)
    want = torch.where(pool >= 0, torch.gather(full, 1, pool.clamp(min=0)), float("-inf"))
    np.testing.assert_array_equal(bits(got), bits(want))
    assert bool(torch.isinf(got[:, -1]).all()) and bool((got[:, -1] < 0).all())         # -1: not in this index
    assert bool((got[:, :-1] != 0).any()) and bool((got[:, 1] == 0).any())
    np.testing.assert_array_equal(bits(m.doc_scores(queries, pool.cpu().numpy())), bits(want))     # a host array is taken too
    with pytest.raises(ValueError):
        m.doc_scores(queries, np.full((len(queries), 2), N))                               # not a position of this index
    with pytest.raises(ValueError):
        m.doc_scores(queries, pool[:3])                                                    # one row per query


# ---- 2. gold_ranks against the full ranking ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 5, 9])
@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "binary_search"])
@pytest.mark.parametrize("name", CLASSES)
def test_gold_ranks_equal_the_rank_plane(name, table, G, setups, corpus):
    _, queries = corpus
    m, S, N, full, rank, pool = setups(name, table)
    if name == "BM25":                       # a term held by more than half the corpus: negative idf, golds with a negative score
        assert m.idf_host[m.vocab["w0"]] < 0
        assert bool((torch.gather(full, 1, pool[:, 2:3]) < 0).any())
    seen = 0
    for pos in windows(pool, G):
        got = m.gold_ranks(queries, pos)
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(queries), G)
        np.testing.assert_array_equal(got.cpu().numpy(), want_ranks(rank, pos).cpu().numpy(), err_msg=f"{name} G={G}")
        for q in (OOV, EMPTY):               # every document ties at 0.0: the rank is the position (-1 stays -1)
            np.testing.assert_array_equal(got[q].cpu().numpy(), pos[q].cpu().numpy())
        seen += int((got == 0).sum())
    assert seen >= len(queries)              # the rank-0 golds came out as rank 0


# ---- 3. the count kernel alone ----------------------------------------------------------------------------------------------------------
def desc_key(s):
    """numpy form of the float64 sort's key (ascending key = descending score; -0.0 == +0.0; NaN first)."""
    u = np.ascontiguousarray(s, dtype=np.float64).view(np.uint64).copy()
    sign = np.uint64(1) << np.uint64(63)
    u[u == sign] = 0
    asc = np.where((u & sign) != 0, ~u, u | sign)
    key = ~asc
    key[np.isnan(s)] = 0
    return key


def count_rule(scores, ids, gs, gid):
    """[Q, G] int64: per (query, gold) the documents (scores [Q, n], ids [n]) ranked before the gold (gs, gid [Q, G]); gid < 0 counts none."""
    k, gk = desc_key(scores)[:, :, None], desc_key(gs)[:, None, :]
    before = (k < gk) | ((k == gk) & (ids[None, :, None] < gid[:, None, :]))
    return np.where(gid >= 0, before.sum(1), 0).astype(np.int64)


@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "binary_search"])
@pytest.mark.parametrize("name", ["BM25", "TFIDF"])
def test_count_kernel_alone(name, table, setups, corpus, ops):
    _, queries = corpus
    m, S, N, full, rank, pool = setups(name, table)
    Q = len(queries)
    mode = m.lexical_mode()
    vals, idf = m.lexical_tables()
    qoff, flat = m._query_csr(queries)
    host = full.cpu().numpy()
    # golds: documents of the index (slice edges, the tail, the rank-0 document), a skipped one, and three that tie the zero-scoring
    # documents (all N of them for the out-of-vocabulary and the empty query) from below id_base, at id_base + N and above it
    doc_cols = np.stack([np.full(Q, S + 5), np.full(Q, N - 1), pool[:, 0].cpu().numpy(), np.full(Q, S), np.full(Q, 2 * S - 1)], 1)
    gs = np.concatenate([np.take_along_axis(host, doc_cols, 1), np.zeros((Q, 4))], 1)
    gid = np.concatenate([ID0 + doc_cols, np.tile(np.array([-1, ID0 - 3, ID0 + N, ID0 + N + 5], dtype=np.int64), (Q, 1))], 1)
    G = gs.shape[1]
    assert G == 9
    gs_d, gid_d = torch.from_numpy(gs).cuda().contiguous(), torch.from_numpy(gid).cuda().contiguous()
    prefill = (7 + torch.arange(Q * G, dtype=torch.int32, device="cuda")).view(Q, G)
    ids = ID0 + np.arange(N, dtype=np.int64)

    def run(lo, hi):
        counts = prefill.clone()
        ops.lexical_count(mode, m.toff, m.pdoc, vals, idf, qoff, flat, Q, N, lo, hi, ID0, gs_d, gid_d, counts, slice_off=m.slice_off)
        return counts.cpu().numpy().astype(np.int64) - prefill.cpu().numpy()

    got = {}
    for lo, hi in ((0, S), (S, 3 * S), (2 * S, N), (0, N), (S, S), (N - 17, N)):
        got[(lo, hi)] = run(lo, hi)
        np.testing.assert_array_equal(got[(lo, hi)], count_rule(host[:, lo:hi], ids[lo:hi], gs, gid), err_msg=f"{name} [{lo}, {hi})")
    whole = got[(0, N)]
    np.testing.assert_array_equal(got[(0, S)] + got[(S, 3 * S)] + got[(N - 17, N)], whole)        # disjoint ranges sum to the whole
    assert not got[(S, S)].any() and not whole[:, 5].any()                                         # nothing to do / a skipped gold
    for q in (OOV, EMPTY):                   # every document ties the 0.0 golds: the id decides, on both sides
        assert whole[q, 6] == 0 and whole[q, 7] == N and whole[q, 8] == N
        np.testing.assert_array_equal(whole[q, :5], doc_cols[q])
    np.testing.assert_array_equal(whole[:, 2], 0)                                                  # the rank-0 document
    np.testing.assert_array_equal(whole[:, :5], np.take_along_axis(rank.cpu().numpy(), doc_cols, 1))
    np.testing.assert_array_equal(run(0, N), whole)                                                # the same call twice
    with pytest.raises(ValueError):
        run(17, N)                                                                                 # off the slice grid


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLASSES)
def test_ties(name, corpus, ops):
    docs, _ = corpus
    S = slice_docs(ops, name)
    N = 3 * S + 17
    rng = np.random.default_rng(21)
    docs = [d + " commun" if c else d for d, c in zip(docs[:N], rng.random(N) < 0.97)]     # negative BM25 idf
    borders = {S - 1, S, 2 * S - 1, 2 * S, 3 * S - 1, 3 * S, N - 2, N - 1}
    tied = sorted(borders | set(range(5, N, 20)))
    for i in tied:
        docs[i] = "jumeau jumelle jumeau"                                                 # hundreds of documents share one text, across slices
    rare = [i for i in range(100, N, 997) if i not in set(tied)]
    for i in rare:
        docs[i] = docs[i] + " rarissime"
    m = make(name, docs)
    queries = ["jumeau", "jumelle jumeau", "rarissime", "inconnu", "commun", "commun rarissime"]
    rank = m.search_device(queries).rank.long()
    gold = [tied[0], tied[len(tied) // 2], tied[-1], S - 1, S, 3 * S, N - 1, 1, rare[0], rare[-1], -1]
    pos = torch.tensor([gold] * len(queries), dtype=torch.int64, device="cuda")
    got = m.gold_ranks(queries, pos)
    np.testing.assert_array_equal(got.cpu().numpy(), want_ranks(rank, pos).cpu().numpy())
    assert got[0, :3].tolist() == [0, len(tied) // 2, len(tied) - 1]                      # ties come out by ascending id
    assert got[3].tolist() == gold                                                         # out of vocabulary: the position


# ---- 5. tune ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_spec,top_k", [("3S+17", 50), ("2W+17", 1000)])
def test_tune_counting_equals_the_plane_route(n_spec, top_k, ops):
    from fusion_amd.retrievers.bm25 import BM25
    W = ops.sort_max_n(torch.float64)
    N = {"3S+17": 3 * 3584 + 17, "2W+17": 2 * W + 17}[n_spec]
    rng = np.random.default_rng(7 + N + top_k)
    docs = synthetic_text(rng, N, 1, 12, vocab_size=900)
    queries = synthetic_text(rng, 6, 1, 5, vocab_size=900) + ["zzz"]
    Q = len(queries)
    ids = np.arange(N, dtype=np.int64) * 3 + 11                            # 4 is not a corpus id
    k1s, bs = [0.9, 2.0], [0.0, 0.75]
    m = BM25(docs, k1s[0], bs[0])
    first = m.ranked_positions(queries, top_k=top_k + 1)
    gold = [sorted({int(x) for x in rng.choice(ids, size=int(rng.integers(1, 4)), replace=False)}) for _ in range(Q)]
    for q in range(Q):
        gold[q] += [int(ids[first[q][top_k - 1]]), int(ids[first[q][top_k]])]   # the last entry kept and the first one cut
    gold[1] += [int(ids[N - 1]), int(ids[(N - 1) // W * W])]
    gold[2] += [gold[2][0], 4]                                             # a duplicate label and an id outside the corpus
    gold[3] = [int(ids[first[3][0]])]
    rk = [10, top_k - 1, top_k, 2 * top_k]                                 # cut-offs on both sides of top_k
    kw = dict(ids=ids, k1_range=k1s, b_range=bs, recall_at_k=rk, top_k=top_k)
    plane = m.tune(queries, gold, counting=False, **kw)
    assert m.last_tune_path == "plane" and (m.k1, m.b) == (k1s[0], bs[0])
    count = m.tune(queries, gold, counting=True, **kw)
    assert m.last_tune_path == "count" and (m.k1, m.b) == (k1s[0], bs[0])
    assert count == plane and len(count) == 4
    assert list(count[0]) == ["k1", "b"] + [f"recall@{k}" for k in rk] + ["r-precision"]
    assert count[0][f"recall@{top_k}"] > count[0][f"recall@{top_k - 1}"] > 0          # the gold at rank top_k - 1 decides a cut-off
    assert m.tune(queries, gold, **kw) == plane
    assert m.last_tune_path == ("count" if N > W else "plane")             # the default: count where the plane route cuts
    m.USE_POSTING_VALUES = False                                           # the per-posting expression has no range walk
    m.tune(queries, gold, counting=True, **kw)
    assert m.last_tune_path == "plane"


# ---- 6. shards --------------------------------------------------------------------------------------------------------------------------
def test_eight_shards_sum_to_the_whole_indexs_ranks(corpus, ops):
    from fusion_amd.distributed import ShardedLexicalIndex, shard_bounds
    from fusion_amd.retrievers.bm25 import BM25, LexicalStats
    docs, queries = corpus
    N, R = len(docs), 8
    whole = BM25(docs, 1.5, 0.75, id_base=ID0)
    rng = np.random.default_rng(23)
    pos = torch.from_numpy(rng.integers(0, N, (len(queries), 5))).cuda()
    pos[:, 0] = torch.tensor([shard_bounds(N, R, q % R)[0] for q in range(len(queries))])     # the first document of a shard
    pos[0, 4] = N - 1
    want = whole.gold_ranks(queries, pos)
    gid = pos + ID0
    bounds = [shard_bounds(N, R, r) for r in range(R)]
    stats = LexicalStats.merge([BM25(docs[lo:hi], 1.5, 0.75, device="cpu").stats() for lo, hi in bounds])
    assert stats == whole.stats()
    models = [BM25(docs[lo:hi], 1.5, 0.75, stats=stats, id_base=ID0 + lo) for lo, hi in bounds]
    parts = []
    for (lo, hi), sm in zip(bounds, models):
        local = pos - lo
        parts.append(sm.doc_scores(queries, torch.where((local >= 0) & (local < hi - lo), local, -1)))
    sc = torch.stack(parts).max(0).values                                  # all_reduce(MAX)
    np.testing.assert_array_equal(bits(sc), bits(whole.doc_scores(queries, pos)))
    counts = torch.zeros_like(pos)
    for sm in models:                                                      # all_reduce(SUM)
        counts += sm.count_before(queries, sc, gid)
    np.testing.assert_array_equal(counts.cpu().numpy(), want.cpu().numpy())
    acc = torch.zeros_like(pos)
    for sm in models:                                                      # ... or one tensor handed from shard to shard
        assert sm.count_before(queries, sc, gid, counts=acc) is acc
    np.testing.assert_array_equal(acc.cpu().numpy(), want.cpu().numpy())
    np.testing.assert_array_equal(ShardedLexicalIndex(whole).gold_ranks(queries, gid).cpu().numpy(), want.cpu().numpy())
    # the whole index's ranks are the ranking's: the first entries of the exact lists stand at their ranks
    top = whole.search_topk(queries, 7, streaming=False).ids - ID0
    np.testing.assert_array_equal(whole.gold_ranks(queries, top).cpu().numpy(), np.broadcast_to(np.arange(7), (len(queries), 7)))


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_identical_tensors(setups, corpus):
    _, queries = corpus
    m, S, N, full, rank, pool = setups("BM25", True)
    a, b = m.gold_ranks(queries, pool), m.gold_ranks(queries, pool)
    assert torch.equal(a, b)
    np.testing.assert_array_equal(bits(m.doc_scores(queries, pool)), bits(m.doc_scores(queries, pool)))
