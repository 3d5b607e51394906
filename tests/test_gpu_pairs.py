"""Pair scores and list completion on the GPU (csrc/pairs.hip, the pair_scores / rerank surface of the sharded indexes,
Aggregator.complete_topk).  No tolerance anywhere: a pair score is compared with a gather from the all-pairs plane of the same system
(ops.dot_scores, ops.sparse_dot, the lexical scores()) as bit patterns, lists by ids and bit patterns."""
import numpy as np
import pytest
import torch

import pairs_cases as P

pytestmark = pytest.mark.gpu

N_DENSE = 700


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    """float tensors as their integer bit patterns: -0.0 != +0.0, and a comparison never meets a NaN"""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits(got), bits(want))


# ---- dense -----------------------------------------------------------------------------------------------------------------------------
_DENSE = {}


def dense_case(ops, d):
    """(Qn, Dn, {Q: the plane ops.dot_scores(Qn[:Q], Dn)}) on the device, built once per d"""
    if d not in _DENSE:
        Qn, Dn = (dev(x) for x in P.dense_corpus(100 + d, N_DENSE, d))
        _DENSE[d] = (Qn, Dn, {Q: ops.dot_scores(Qn[:Q].contiguous(), Dn).clone() for Q in P.QS})
    return _DENSE[d]


def gather(plane, cand, lens, id_base):
    """P.expected on the device: the bits move, nothing is computed"""
    return dev(P.expected(plane.cpu().numpy(), cand, lens, id_base))


@pytest.mark.parametrize("d", P.DIMS)
def test_dense_pairs_carry_the_planes_bits(ops, d):
    """Every (Q, W) of the issue's grid, ids inside and outside the shard, list lengths 0 / middle / full, an id_base beyond 2^31."""
    Qn, Dn, planes = dense_case(ops, d)
    for Q in P.QS:
        for W in P.WIDTHS:
            cand, lens = P.candidates(1000 * Q + W, Q, W, N_DENSE, P.BIG_BASE)
            got = ops.dot_pairs(Qn[:Q].contiguous(), Dn, dev(cand), dev(lens), id_base=P.BIG_BASE)
            assert same_bits(got, gather(planes[Q], cand, lens, P.BIG_BASE)), (d, Q, W)
    # no cand_len = W everywhere; id_base 0
    cand, _ = P.candidates(5, 3, 129, N_DENSE, 0)
    assert same_bits(ops.dot_pairs(Qn[:3].contiguous(), Dn, dev(cand)), gather(planes[3], cand, None, 0))


def test_dense_special_rows_and_repeats(ops):
    Qn, Dn, planes = dense_case(ops, 768)
    plane = planes[130]
    # (the fixture's denormal row, zero row and scaled-down query are checked on the CPU: test_pairs_cpu.py)
    cand = np.tile(np.array([P.DENORMAL_ROW, P.ZERO_ROW, 11, 11, 40, 11], dtype=np.int64), (130, 1))
    cand[1::2] = cand[1::2, ::-1]                                  # the same documents in other slots of other rows
    got = ops.dot_pairs(Qn, Dn, dev(cand))
    assert same_bits(got, gather(plane, cand, None, 0))
    assert same_bits(got[::2, 2], got[::2, 3]) and same_bits(got[::2, 2], got[::2, 5]) and same_bits(got[1::2, 0], got[1::2, 2])
    assert same_bits(got[0::2, 0], plane[0::2, P.DENORMAL_ROW]) and same_bits(got[1::2, 5], plane[1::2, P.DENORMAL_ROW])
    assert same_bits(got[0::2, 1], torch.zeros(65, device="cuda"))  # a row of zeros scores +0.0


def test_dense_strided_views_and_untouched_columns(ops):
    Qn, Dn, planes = dense_case(ops, 100)
    Q, W = 130, 65
    cand, lens = P.candidates(77, Q, W, N_DENSE, P.BIG_BASE)
    wide = torch.full((Q, W + 11), -7, dtype=torch.int64, device="cuda")
    wide[:, 3:3 + W] = dev(cand)
    plane = torch.full((Q, W + 20), 123.0, dtype=torch.float32, device="cuda")
    out = ops.dot_pairs(Qn, Dn, wide[:, 3:3 + W], dev(lens), id_base=P.BIG_BASE, out=plane[:, 9:9 + W])
    assert out.data_ptr() == plane[:, 9:9 + W].data_ptr()
    assert same_bits(plane[:, 9:9 + W], gather(planes[Q], cand, lens, P.BIG_BASE))
    assert bool((plane[:, :9] == 123.0).all()) and bool((plane[:, 9 + W:] == 123.0).all())


def test_dense_repeatable_and_empty(ops):
    Qn, Dn, planes = dense_case(ops, 768)
    cand, lens = P.candidates(9, 130, 300, N_DENSE, P.BIG_BASE)
    c, n = dev(cand), dev(lens)
    a = ops.dot_pairs(Qn, Dn, c, n, id_base=P.BIG_BASE).clone()
    b = ops.dot_pairs(Qn, Dn, c, n, id_base=P.BIG_BASE)
    assert same_bits(a, b)
    # a shard of no documents owns no slot; no queries or no slots: nothing to do
    none = ops.dot_pairs(Qn, Dn[:0], c, n, id_base=P.BIG_BASE)
    assert bool((none == float("-inf")).all())
    assert tuple(ops.dot_pairs(Qn[:0], Dn, c[:0]).shape) == (0, 300) and tuple(ops.dot_pairs(Qn, Dn, c[:, :0]).shape) == (130, 0)


# ---- sparse ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse_case(ops):
    Qm, Dm = P.sparse_corpus(3)
    index = ops.sparse_index(dev(Dm))
    qoff, qterms, qw = ops.sparse_rows(dev(Qm))
    host = P.inverted(Dm) + P.query_rows(Qm)
    for got, want in zip(index.tensors() + (qoff, qterms, qw), host):      # the numpy restatement walks the same lists
        assert np.array_equal(got.cpu().numpy(), want)
    return index, (qoff, qterms, qw), host, ops.sparse_dot(index, qoff, qterms, qw).clone()


def test_sparse_pairs_carry_the_planes_bits(ops, sparse_case):
    index, q, host, plane = sparse_case
    toff, pdoc, _, qoff, qterms, _ = host
    for W in (1, 40, 300):
        cand, lens = P.sparse_candidates(50 + W, toff, pdoc, qoff, qterms, max(W, 8), P.BIG_BASE)
        cand, lens = cand[:, :W] if W < 8 else cand, np.minimum(lens, W)
        got = ops.sparse_dot_pairs(index, *q, dev(cand), dev(lens), id_base=P.BIG_BASE)
        assert same_bits(got, gather(plane, cand, lens, P.BIG_BASE)), W
        if W == 40:   # ... which are the bits of the chain, restated in numpy
            assert same_bits(got, dev(P.sparse_chain(*host, cand, lens, P.BIG_BASE, P.SP_N)))
            # documents without postings score +0.0 (sign bit clear) for every query with a list, and so does everything for the empty query
            empty = got[:, 4:4 + len(P.SP_EMPTY_DOCS)]
            assert bool((bits(empty) == 0).all())
            row = got[P.SP_EMPTY_QUERY]
            assert bool(((bits(row) == 0) | (row == float("-inf"))).all()) and bool((bits(row) == 0).any())
            # first and last entry of a posting list: found, and not zero
            assert bool((got[[0, 1, 3, 4, 5], :2] > 0).all())
    cand, _ = P.sparse_candidates(7, toff, pdoc, qoff, qterms, 65, 0)
    wide = torch.full((cand.shape[0], 80), 5.0, device="cuda")
    ops.sparse_dot_pairs(index, *q, dev(cand), out=wide[:, 2:67])
    assert same_bits(wide[:, 2:67], gather(plane, cand, None, 0)) and bool((wide[:, :2] == 5.0).all()) and bool((wide[:, 67:] == 5.0).all())
    assert bool((ops.sparse_dot_pairs(ops.SparseIndex(index.toff, index.pdoc[:0], index.pw[:0], 0, index.V, slice_off=index.slice_off), *q, dev(cand))
                 == float("-inf")).all())


# ---- the surface of the sharded indexes, and completion ---------------------------------------------------------------------------------
N_CORPUS, ID0, K = 600, 2 ** 33, 50


def synthetic_text(rng, n_docs, lo, hi, vocab_size=400):
    vocab = np.array([f"w{i}" for i in range(vocab_size)])
    p = 1.0 / np.arange(1, vocab_size + 1); p /= p.sum()
    sizes = rng.integers(lo, hi, n_docs)
    words = rng.choice(vocab, size=int(sizes.sum()), p=p)
    return [" ".join(w) for w in np.split(words, np.cumsum(sizes)[:-1])]


class Corpus:
    """One small corpus under three systems, whole and cut into two shards, with everything a test needs of it computed once."""

    def __init__(self, ops):
        from fusion_amd.distributed import ShardedDenseIndex, ShardedLexicalIndex, ShardedSparseIndex, shard_bounds
        from fusion_amd.retrievers.bm25 import BM25, LexicalStats
        rng = np.random.default_rng(41)
        Qn, Dn = P.dense_corpus(42, N_CORPUS, 64)
        self.Q = 5
        self.Qn, Dn = dev(Qn[3:3 + self.Q]), dev(Dn)
        Dm = np.where(rng.random((N_CORPUS, 300)) < 0.05, rng.random((N_CORPUS, 300)), 0.0).astype(np.float32)
        Qm = np.where(rng.random((self.Q, 300)) < 0.04, rng.random((self.Q, 300)), 0.0).astype(np.float32)
        Dm = dev(Dm)
        self.sq = ops.sparse_rows(dev(Qm))
        docs = synthetic_text(rng, N_CORPUS, 3, 30)
        self.queries = synthetic_text(rng, self.Q - 1, 2, 8) + ["zzz"]
        cut = [shard_bounds(N_CORPUS, 2, r) for r in range(2)]
        stats = LexicalStats.merge([BM25(docs[lo:hi], 1.5, 0.75, device="cpu").stats() for lo, hi in cut])
        self.bm25 = BM25(docs, 1.5, 0.75, id_base=ID0)
        self.whole = dict(dense=ShardedDenseIndex(Dn, ID0), sparse=ShardedSparseIndex(ops.sparse_index(Dm), ID0), bm25=ShardedLexicalIndex(self.bm25))
        self.shards = [dict(dense=ShardedDenseIndex(Dn[lo:hi], ID0 + lo), sparse=ShardedSparseIndex(ops.sparse_index(Dm[lo:hi].contiguous()), ID0 + lo),
                            bm25=ShardedLexicalIndex(BM25(docs[lo:hi], 1.5, 0.75, stats=stats, id_base=ID0 + lo))) for lo, hi in cut]
        self.query = dict(dense=(self.Qn,), sparse=self.sq, bm25=(self.queries,))
        self.planes = dict(dense=ops.dot_scores(self.Qn, Dn).clone(), sparse=ops.sparse_dot(self.whole["sparse"].index, *self.sq).clone(),
                           bm25=self.bm25.scores(self.queries).clone())
        self.names = ("dense", "sparse", "bm25")

    def scorers(self, names=None):
        return {n: (lambda U, ulen, n=n: self.whole[n].pair_scores(*self.query[n], U, ulen)) for n in (names or self.names)}

    def search(self, k):
        from fusion_amd.planes import RankedTopk
        out = {}
        for n in self.names:
            r = self.whole[n].search(*self.query[n], k)
            out[n] = r if isinstance(r, RankedTopk) else RankedTopk.from_search(*r)
        return out


@pytest.fixture(scope="module")
def corpus(ops):
    return Corpus(ops)


def test_two_shards_combine_to_the_one_shard_plane(ops, corpus):
    cand, lens = P.candidates(3, corpus.Q, 129, N_CORPUS, ID0)
    c, n = dev(cand), dev(lens)
    for name in corpus.names:
        one = corpus.whole[name].pair_scores(*corpus.query[name], c, n)
        parts = [s[name].pair_scores(*corpus.query[name], c, n) for s in corpus.shards]
        assert one.dtype == (torch.float64 if name == "bm25" else torch.float32)
        assert same_bits(torch.maximum(parts[0], parts[1]), one), name
        assert same_bits(one, gather(corpus.planes[name], cand, lens, ID0)), name
        # every slot is owned by at most one shard
        assert not bool(((parts[0] > float("-inf")) & (parts[1] > float("-inf"))).any())


def test_token_index_pair_scores_is_local_scores_under_a_maximum(ops):
    from fusion_amd.distributed import ShardedTokenIndex
    rng = np.random.default_rng(8)
    N, cut_doc = 200, 90
    off = np.concatenate([[0], np.cumsum(rng.integers(1, 40, N))]).astype(np.int64)
    unit = lambda x: (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)      # noqa: E731
    Dtok, Qtok = dev(unit(rng.standard_normal((int(off[-1]), 128)))).half(), dev(unit(rng.standard_normal((4, 32, 128)))).half()
    Doff = dev(off)
    cand, lens = P.candidates(12, 4, 65, N, ID0)
    c, n = dev(cand), dev(lens)
    whole = ShardedTokenIndex(Dtok, Doff, ID0, max_doc_len=64)
    one = whole.pair_scores(Qtok, c, n)
    assert same_bits(one, whole.local_scores(Qtok, c, n)) and same_bits(one, gather(ops.maxsim(Qtok, Dtok, Doff), cand, lens, ID0))
    rows = int(off[cut_doc])
    parts = [ShardedTokenIndex(Dtok[:rows], Doff[:cut_doc + 1], ID0, max_doc_len=64).pair_scores(Qtok, c, n),
             ShardedTokenIndex(Dtok[rows:], (Doff[cut_doc:] - rows).contiguous(), ID0 + cut_doc, max_doc_len=64).pair_scores(Qtok, c, n)]
    assert same_bits(torch.maximum(parts[0], parts[1]), one)


def test_rerank_of_a_searchs_ids_is_the_searchs_list(ops, corpus):
    for name, want in corpus.search(K).items():
        got = corpus.whole[name].rerank(*corpus.query[name], want.ids)
        assert torch.equal(got.ids, want.ids) and same_bits(got.scores, want.scores) and got.lens.tolist() == want.lens.tolist(), name
        assert (got.scores64 is None) == (want.scores64 is None) and (want.scores64 is None or same_bits(got.scores64, want.scores64)), name
        # from the RankedTopk itself, shuffled, cut to k: the same head; ids no shard owns go last as (-inf, -1)
        perm = torch.randperm(K, device="cuda")
        ids = torch.cat([want.ids[:, perm], torch.full((corpus.Q, 3), ID0 + N_CORPUS + 5, dtype=torch.int64, device="cuda")], 1)
        got = corpus.whole[name].rerank(*corpus.query[name], ids, k=K + 2)
        assert torch.equal(got.ids[:, :K], want.ids) and same_bits(got.scores[:, :K], want.scores) and got.lens.tolist() == [K] * corpus.Q, name
        assert bool((got.ids[:, K:] == -1).all()) and bool((got.scores[:, K:] == float("-inf")).all())


def test_completed_lists_keep_every_listed_score_and_start_with_the_list(ops, corpus):
    from fusion_amd.retrievers.hybrid import Aggregator
    cut = corpus.search(K)
    done = Aggregator.complete_topk(cut, corpus.scorers())
    U = set()
    for name in corpus.names:
        a, b = cut[name], done[name]
        assert b.k == 3 * K and (b.scores64 is not None) == (name == "bm25")
        # the union is the same for every system, and lens = its size
        ids = b.ids.cpu().numpy()
        sets = [frozenset(ids[q, :int(b.lens[q])].tolist()) for q in range(corpus.Q)]
        assert all(-1 not in s and len(s) == int(b.lens[q]) for q, s in enumerate(sets)) and bool((b.ids[:, :K] >= 0).all())
        U.add(tuple(sets))
        assert bool((b.ids[torch.arange(3 * K, device="cuda")[None, :] >= b.lens[:, None]] == -1).all())
        # an exact search's list comes first, bit for bit -- so every listed entry keeps its listed score
        assert torch.equal(b.ids[:, :K], a.ids) and same_bits(b.scores[:, :K], a.scores), name
        if name == "bm25":
            assert same_bits(b.scores64[:, :K], a.scores64)
        # every entry carries the plane's score of its id
        plane = corpus.planes[name]
        want = torch.gather(plane, 1, (b.ids - ID0).clamp(min=0))
        listed = b.ids >= 0
        got = b.scores64 if name == "bm25" else b.scores
        assert torch.equal(bits(got)[listed], bits(want)[listed]), name
        assert same_bits(b.scores, got.to(torch.float32))
    assert len(U) == 1
    # a system without a scorer keeps its list
    part = Aggregator.complete_topk(cut, corpus.scorers(("dense",)))
    assert part["sparse"] is cut["sparse"] and part["bm25"] is cut["bm25"] and torch.equal(part["dense"].ids, done["dense"].ids)


def test_completion_changes_nothing_when_the_lists_are_whole(ops, corpus):
    from fusion_amd.retrievers.hybrid import Aggregator
    whole = corpus.search(N_CORPUS)
    done = Aggregator.complete_topk(whole, corpus.scorers())
    w = dict(dense=0.5, sparse=0.3, bm25=0.2)
    for method, norm in (("nsf", "none"), ("nsf", "min-max"), ("rrf", None)):
        a = Aggregator.fuse_topk(whole, method, norm, w, {})
        b = Aggregator.fuse_topk(done, method, norm, w, {})
        assert a.lens.tolist() == b.lens.tolist() == [N_CORPUS] * corpus.Q
        assert torch.equal(a.ids[:, :N_CORPUS], b.ids[:, :N_CORPUS]) and same_bits(a.scores[:, :N_CORPUS], b.scores[:, :N_CORPUS]), (method, norm)


def test_completed_fusion_is_the_weighted_sum_of_the_planes(ops, corpus):
    """What the cut lists cannot give: under 'none' every document of the union gets w . (its three plane scores), in float64."""
    from fusion_amd.retrievers.hybrid import Aggregator
    cut = corpus.search(K)
    w = dict(dense=0.5, sparse=0.3, bm25=0.2)
    fused = Aggregator.fuse_topk(Aggregator.complete_topk(cut, corpus.scorers()), "nsf", "none", w, {})
    pos = (fused.ids - ID0).clamp(min=0)
    want = torch.zeros(fused.ids.shape, dtype=torch.float64, device="cuda")
    for name in corpus.names:      # the join's own order: 0.0 + v * w, system by system
        want = want + torch.gather(corpus.planes[name], 1, pos).double() * w[name]
    listed = torch.arange(fused.ids.shape[1], device="cuda")[None, :] < fused.lens[:, None]
    assert bool(listed.any(1).all()) and torch.equal(bits(fused.scores)[listed], bits(want)[listed])
    # ... and in descending order of it
    s = fused.scores.masked_fill(~listed, float("-inf"))
    assert bool((s[:, 1:] <= s[:, :-1]).all())
    # the cut lists give something else: a document one system did not list got nothing from it
    plain = Aggregator.fuse_topk(cut, "nsf", "none", w, {})
    assert plain.lens.tolist() == fused.lens.tolist() and not torch.equal(bits(plain.scores[:, :K]), bits(fused.scores[:, :K]))


def test_depth_cuts_the_completed_lists(ops, corpus):
    from fusion_amd.retrievers.hybrid import Aggregator
    cut = corpus.search(K)
    full = Aggregator.complete_topk(cut, corpus.scorers())
    for depth in (1, K + 7, 10 ** 6):
        got = Aggregator.complete_topk(cut, corpus.scorers(), depth=depth)
        keep = min(depth, 3 * K)
        for name in corpus.names:
            a, b = full[name], got[name]
            assert b.k == keep and torch.equal(b.ids, a.ids[:, :keep]) and same_bits(b.scores, a.scores[:, :keep]), (name, depth)
            assert b.lens.tolist() == torch.clamp(a.lens, max=keep).tolist()
            assert (b.scores64 is None) == (a.scores64 is None) and (a.scores64 is None or same_bits(b.scores64, a.scores64[:, :keep]))
    # completed and cut to depth, the lists pass through the other consumers of lists as they are
    labels = [[ID0 + 3 * q, ID0 + 7] for q in range(corpus.Q)]
    got = Aggregator.complete_topk(cut, corpus.scorers(), depth=K)
    perf = Aggregator.tune_topk(got, "min-max", [dict(dense=0.5, sparse=0.3, bm25=0.2)], labels, {})
    assert len(perf) == 1 and Aggregator.evaluate_topk(got["dense"], labels).keys() == perf[0].keys()
