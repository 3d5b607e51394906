"""The forward (document-major) index on the GPU (ops.forward_index, csrc/forward.hip, the route of ops.sparse_dot_pairs and of the
lexical doc_scores, and what follows through the sharded indexes and Aggregator.complete_topk).  No tolerance anywhere: the forward route
is compared with the inverted route, with the numpy restatement and with a gather from the all-pairs plane, as bit patterns."""
import numpy as np
import pytest
import torch

import forward_cases as F
import pairs_cases as P

pytestmark = pytest.mark.gpu


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


def gather(plane, cand, lens, id_base):
    return dev(P.expected(plane.cpu().numpy(), cand, lens, id_base))


class SparseCase:
    """An index with its forward index, the queries, the host lists of both, and the all-pairs plane: built once"""

    def __init__(self, ops, Qm, Dm):
        self.index = ops.sparse_index(dev(Dm))
        self.q = ops.sparse_rows(dev(Qm))
        self.host = P.inverted(Dm) + P.query_rows(Qm)
        self.fhost = F.forward_build(self.host[0], self.host[1], Dm.shape[0])
        self.N = Dm.shape[0]
        self.fwd = self.index.build_forward()
        self.plane = ops.sparse_dot(self.index, *self.q).clone()

    def walk(self, cand, lens, id_base):
        foff, fterm, fpos = self.fhost
        return dev(F.row_walk(foff, fterm, self.host[2][fpos], *self.host[3:], cand, lens, id_base, self.N))


@pytest.fixture(scope="module")
def seeded(ops):
    return SparseCase(ops, *P.sparse_corpus(3))


@pytest.fixture(scope="module")
def long_rows(ops):
    return SparseCase(ops, *F.long_row_corpus())


# ---- the build -------------------------------------------------------------------------------------------------------------------------
def test_the_build_is_the_stable_sort_by_document(ops, seeded, long_rows):
    for case in (seeded, long_rows):
        toff, pdoc, pw = case.host[:3]
        foff, fterm, fpos = case.fhost
        f = ops.forward_index(case.index.toff, case.index.pdoc, case.N)
        assert isinstance(f, ops.ForwardIndex) and (f.N, f.V, f.nnz) == (case.N, case.index.V, len(pdoc))
        for got, want in ((f.foff, foff), (f.fterm, fterm), (f.fpos, fpos)):
            assert got.dtype == torch.from_numpy(want).dtype and got.cpu().numpy().tobytes() == want.tobytes()
        assert f.nbytes == 8 * (case.N + 1) + 8 * len(pdoc)
        s = case.fwd
        assert isinstance(s, ops.SparseForward) and case.index.forward is s and s.nbytes == 8 * (case.N + 1) + 8 * len(pdoc)
        assert s.rows.dtype == torch.int32 and tuple(s.rows.shape) == (len(pdoc), 2) and s.rows.is_contiguous() and s.rows.data_ptr() % 8 == 0
        assert s.foff.cpu().numpy().tobytes() == foff.tobytes() and s.terms().cpu().numpy().tobytes() == fterm.tobytes()
        assert s.weights().cpu().numpy().tobytes() == pw[fpos].tobytes()
        # rows strictly ascending, documents without postings have empty rows
        n = np.diff(foff)
        inner = np.ones(len(fterm), dtype=bool); inner[foff[:-1][n > 0]] = False
        assert (np.diff(fterm.astype(np.int64), prepend=-1)[inner] > 0).all() and (n == np.bincount(pdoc, minlength=case.N)).all()
    assert all(seeded.fhost[0][d] == seeded.fhost[0][d + 1] for d in P.SP_EMPTY_DOCS)
    # an index of no postings; documents past the last posting
    none = ops.forward_index(torch.zeros(6, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 3)
    assert none.foff.tolist() == [0, 0, 0, 0] and none.nnz == 0
    tail = ops.forward_index(seeded.index.toff, seeded.index.pdoc, seeded.N + 5)
    assert tail.foff[-6:].tolist() == [len(seeded.host[1])] * 6
    with pytest.raises(ValueError, match="beyond N"):
        ops.forward_index(seeded.index.toff, seeded.index.pdoc, seeded.N - 5)
    with pytest.raises(ValueError, match="int32"):       # (refused on the count alone: a 2^31-entry view of one element, nothing is read)
        ops.forward_index(seeded.index.toff, torch.zeros(1, dtype=torch.int32, device="cuda").expand(2 ** 31), 1)


# ---- sparse ----------------------------------------------------------------------------------------------------------------------------
def routes_agree(ops, case, cand, lens, id_base, tag):
    c, n = dev(cand), None if lens is None else dev(lens)
    fwd = ops.sparse_dot_pairs(case.index, *case.q, c, n, id_base=id_base, route="forward")
    inv = ops.sparse_dot_pairs(case.index, *case.q, c, n, id_base=id_base, route="inverted")
    assert same_bits(fwd, inv), tag
    assert same_bits(fwd, case.walk(cand, lens, id_base)), tag
    assert same_bits(fwd, gather(case.plane, cand, lens, id_base)), tag
    return fwd


@pytest.mark.parametrize("W", (8, 40, 63, 64, 65, 300))
def test_forward_route_on_the_seeded_corpus(ops, seeded, W):
    toff, pdoc, _, qoff, qterms, _ = seeded.host
    cand, lens = P.sparse_candidates(50 + W, toff, pdoc, qoff, qterms, W, P.BIG_BASE)
    got = routes_agree(ops, seeded, cand, lens, P.BIG_BASE, W)
    local = cand - P.BIG_BASE
    assert lens[:3].tolist() == [W, W, W]
    if W >= 40:      # the mix: negative ids, ids outside the shard, the same document twice in a row
        assert (cand < 0).any() and (local == P.SP_N).any() and (local == -1).any() and (cand[:, -1] == cand[:, -2]).all()
    assert bool((bits(got[:, 4:4 + len(P.SP_EMPTY_DOCS)]) == 0).all())                 # documents without postings: +0.0
    assert bool((got[[0, 1, 3, 4, 5], :2] > 0).all())                                  # first and last entry of a posting list
    if W == 40:
        cand, lens = P.candidates(9, 6, W, P.SP_N, P.BIG_BASE)                         # list lengths 0 / half / W
        assert lens[:3].tolist() == [W, 0, W // 2]
        routes_agree(ops, seeded, cand, lens, P.BIG_BASE, "lens")
        routes_agree(ops, seeded, cand - P.BIG_BASE + 3, None, 3, "no lens")           # (the mix's odd ids stay odd)


@pytest.mark.parametrize("W", (8, 65, 300))
def test_forward_route_on_long_rows(ops, long_rows, W):
    cand, lens = F.long_row_candidates(70 + W, W, P.BIG_BASE)
    got = routes_agree(ops, long_rows, cand, lens, P.BIG_BASE, W)
    assert float(got[F.LR_TWIN_QUERY, 0]) > 50 and bits(got[F.LR_ORDER_QUERY, 1]).item() == 0      # 700 adds | 1e8 + 1 - 1e8 in term order
    row = got[F.LR_EMPTY_QUERY]
    assert bool(((bits(row) == 0) | (row == float("-inf"))).all())


def test_forward_route_leaves_the_columns_past_w_alone_and_repeats(ops, seeded, long_rows):
    for case, mk in ((seeded, lambda: P.sparse_candidates(7, *seeded.host[:2], *seeded.host[3:5], 65, 0)), (long_rows, lambda: F.long_row_candidates(7, 65, 0))):
        cand, lens = mk()
        wide = torch.full((cand.shape[0], 80), 5.0, device="cuda")
        out = ops.sparse_dot_pairs(case.index, *case.q, dev(cand), dev(lens), out=wide[:, 2:67], route="forward")
        assert out.data_ptr() == wide[:, 2:67].data_ptr()
        assert same_bits(wide[:, 2:67], gather(case.plane, cand, lens, 0)) and bool((wide[:, :2] == 5.0).all()) and bool((wide[:, 67:] == 5.0).all())
        a = ops.sparse_dot_pairs(case.index, *case.q, dev(cand), dev(lens), route="forward").clone()
        b = ops.sparse_dot_pairs(case.index, *case.q, dev(cand), dev(lens), route="forward")
        assert same_bits(a, b)
    # a strided candidate view; no queries, no slots, a shard of no documents
    cand, lens = F.long_row_candidates(8, 40, P.BIG_BASE)
    box = torch.full((cand.shape[0], 51), -7, dtype=torch.int64, device="cuda")
    box[:, 3:43] = dev(cand)
    got = ops.sparse_dot_pairs(long_rows.index, *long_rows.q, box[:, 3:43], dev(lens), id_base=P.BIG_BASE, route="forward")
    assert same_bits(got, gather(long_rows.plane, cand, lens, P.BIG_BASE))
    c = dev(cand)
    assert tuple(ops.sparse_dot_pairs(long_rows.index, *long_rows.q, c[:, :0], route="forward").shape) == (F.LR_Q, 0)
    empty = ops.SparseIndex(torch.zeros_like(seeded.index.toff), seeded.index.pdoc[:0], seeded.index.pw[:0], 0, seeded.index.V,
                            slice_off=seeded.index.slice_off)
    empty.build_forward()
    assert empty.forward.foff.tolist() == [0]
    assert bool((ops.sparse_dot_pairs(empty, *seeded.q, dev(P.candidates(1, 6, 9, 5, 0)[0]), route="forward") == float("-inf")).all())


def test_the_default_route_follows_the_switch(ops, seeded, monkeypatch):
    """route=None: the forward route only with the switch on, a forward index and a vocabulary the kernel takes -- seen from what runs."""
    cand, lens = P.sparse_candidates(3, *seeded.host[:2], *seeded.host[3:5], 40, 0)
    want = gather(seeded.plane, cand, lens, 0)
    spoiled = ops.SparseIndex(seeded.index.toff, seeded.index.pdoc, seeded.index.pw, seeded.N, seeded.index.V, slice_off=seeded.index.slice_off)
    spoiled.build_forward()
    spoiled.forward.rows[:, 1] = 0                                  # a forward index whose weights are all +0.0: it shows when it is read
    zero = ops.sparse_dot_pairs(spoiled, *seeded.q, dev(cand), dev(lens), route="forward")
    assert not same_bits(zero, want) and bool(((zero == 0) | (zero == float("-inf"))).all())
    for on in (False, True):
        monkeypatch.setattr(ops, "SPARSE_PAIRS_PREFER_FORWARD", on)
        assert same_bits(ops.sparse_dot_pairs(spoiled, *seeded.q, dev(cand), dev(lens)), zero if on else want), on
        assert same_bits(ops.sparse_dot_pairs(spoiled, *seeded.q, dev(cand), dev(lens), route="inverted"), want)
        plain = ops.SparseIndex(seeded.index.toff, seeded.index.pdoc, seeded.index.pw, seeded.N, seeded.index.V, slice_off=seeded.index.slice_off)
        assert same_bits(ops.sparse_dot_pairs(plain, *seeded.q, dev(cand), dev(lens)), want)          # no forward index: today's route


def test_a_vocabulary_beyond_the_cap_stays_on_the_inverted_route(ops, monkeypatch):
    cap = ops.sparse_fwd_max_vocab()
    assert cap >= 65536
    monkeypatch.setattr(ops, "SPARSE_PAIRS_PREFER_FORWARD", True)
    # 3 documents over V terms, as postings: term 0: (0, 1.0) (2, 0.5)   term V - 1: (1, 2.0) (2, 4.0);   the query: 3.0 and 0.25 on them
    pdoc, pw = dev(np.array([0, 2, 1, 2], dtype=np.int32)), dev(np.array([1.0, 0.5, 2.0, 4.0], dtype=np.float32))
    cand = dev(np.array([[0, 1, 2, 3]], dtype=np.int64))
    for V in (cap + 1, cap):
        toff = torch.full((V + 1,), 2, dtype=torch.int64, device="cuda"); toff[0] = 0; toff[V] = 4
        q = (dev(np.array([0, 2], dtype=np.int64)), dev(np.array([0, V - 1], dtype=np.int32)), dev(np.array([3.0, 0.25], dtype=np.float32)))
        index = ops.SparseIndex(toff, pdoc, pw, 3, V)
        index.build_forward()
        inv = ops.sparse_dot_pairs(index, *q, cand, route="inverted")
        assert inv.tolist() == [[3.0, 0.5, 2.5, float("-inf")]]
        index.forward.rows[:, 1] = 0                                # it shows when the forward index is read
        if V > cap:
            assert same_bits(ops.sparse_dot_pairs(index, *q, cand), inv)
            with pytest.raises(ValueError, match="beyond"):
                ops.sparse_dot_pairs(index, *q, cand, route="forward")
        else:                                                       # at the cap itself the kernel runs: the bitmap's last bit
            assert ops.sparse_dot_pairs(index, *q, cand).tolist() == [[0.0, 0.0, 0.0, float("-inf")]]
            index.build_forward()
            assert same_bits(ops.sparse_dot_pairs(index, *q, cand, route="forward"), inv)


# ---- lexical ---------------------------------------------------------------------------------------------------------------------------
N_LEX = 400


@pytest.fixture(scope="module")
def lexical(ops):
    from fusion_amd.retrievers.bm25 import BM25, TFIDF, AtireBM25
    docs = F.lexical_text(5, N_LEX)
    docs[7] = ""                                                    # a document without postings
    models = dict(tfidf=TFIDF(docs), bm25=BM25(docs, 1.5, 0.75), atire=AtireBM25(docs, 0.9, 0.4))
    for m in models.values():
        assert isinstance(m.build_forward(), ops.ForwardIndex) and m.forward.fpos is not None and m.forward.N == N_LEX
    return docs, models


def positions(G, Q=len(F.LEX_QUERIES)):
    rng = np.random.default_rng(G)
    pos = rng.integers(0, N_LEX, (Q, G)).astype(np.int64)
    pos[rng.random((Q, G)) < 0.1] = -1
    pos[:, 0] = -1 if G > 1 else 7
    if G > 2:
        pos[:, 1], pos[:, 2] = 7, N_LEX - 1
    return pos


@pytest.mark.parametrize("name", ("tfidf", "bm25", "atire"))
def test_lexical_routes_carry_the_planes_bits(ops, lexical, name):
    _, models = lexical
    m = models[name]
    plane = m.scores(F.LEX_QUERIES).clone()
    assert bool((plane != 0).any(1)[[0, 1, 3, 4]].all()) and not bool((plane[2] != 0).any())
    for G in (1, 5, 300):
        pos = positions(G)
        want = torch.where(dev(pos) >= 0, torch.gather(plane, 1, dev(pos).clamp(min=0)), float("-inf"))
        fwd = m.doc_scores(F.LEX_QUERIES, dev(pos), route="forward")
        inv = m.doc_scores(F.LEX_QUERIES, dev(pos), route="inverted")
        assert fwd.dtype == torch.float64 and same_bits(fwd, inv) and same_bits(fwd, want), (name, G)
        assert same_bits(m.doc_scores(F.LEX_QUERIES, pos, route="forward"), want)                      # host positions
        if G > 1:
            assert bool((fwd[:, 0] == float("-inf")).all())
    assert tuple(m.doc_scores([], np.zeros((0, 3), dtype=np.int64), route="forward").shape) == (0, 3)


def test_update_params_needs_nothing_rebuilt(ops, lexical):
    _, models = lexical
    m = models["bm25"]
    pos = dev(positions(300))
    before = m.doc_scores(F.LEX_QUERIES, pos, route="forward").clone()
    keep, fwd_index = (m.k1, m.b), m.forward
    try:
        m.update_params(0.6, 0.2)
        after = m.doc_scores(F.LEX_QUERIES, pos, route="forward")
        assert m.forward is fwd_index and same_bits(after, m.doc_scores(F.LEX_QUERIES, pos, route="inverted"))
        assert same_bits(after, torch.where(pos >= 0, torch.gather(m.scores(F.LEX_QUERIES), 1, pos.clamp(min=0)), float("-inf")))
        assert not same_bits(after, before)
    finally:
        m.update_params(*keep)
    assert same_bits(m.doc_scores(F.LEX_QUERIES, pos, route="forward"), before)


def test_the_lexical_default_follows_the_switch(ops, lexical, monkeypatch):
    from fusion_amd.retrievers.bm25 import BM25, TFIDF
    docs, models = lexical
    m = BM25(docs, 1.5, 0.75)
    pos = dev(positions(5))
    want = models["bm25"].doc_scores(F.LEX_QUERIES, pos, route="inverted")
    assert same_bits(m.doc_scores(F.LEX_QUERIES, pos), want)                                           # no forward index: today's route
    m.build_forward()
    m.forward.fpos.zero_()                                          # every posting now leads to posting 0: it shows when it is read
    wrong = m.doc_scores(F.LEX_QUERIES, pos, route="forward")
    assert not same_bits(wrong, want)
    for on in (False, True):
        monkeypatch.setattr(TFIDF, "PREFER_FORWARD", on)
        assert same_bits(m.doc_scores(F.LEX_QUERIES, pos), wrong if on else want), on
    flat = BM25(docs, 1.5, 0.75)
    flat.USE_POSTING_VALUES = False                                 # a model without a range walk raises as it did
    flat.build_forward()
    for route in (None, "inverted", "forward"):
        with pytest.raises(ValueError, match="no range walk"):
            flat.doc_scores(F.LEX_QUERIES, pos, route=route)


# ---- the sharded surface and completion ------------------------------------------------------------------------------------------------
ID0, K = 2 ** 33, 40


class Corpus:
    """One small corpus under three systems, whole and in two shards; every sparse and lexical index with its forward index"""

    def __init__(self, ops):
        from fusion_amd.distributed import ShardedDenseIndex, ShardedLexicalIndex, ShardedSparseIndex, shard_bounds
        from fusion_amd.retrievers.bm25 import BM25, LexicalStats
        rng = np.random.default_rng(43)
        N = self.N = N_LEX
        Qn, Dn = P.dense_corpus(44, N, 64)
        self.Q = len(F.LEX_QUERIES)
        self.Qn, Dn = dev(Qn[3:3 + self.Q]), dev(Dn)
        Dm = dev(np.where(rng.random((N, 300)) < 0.08, rng.random((N, 300)), 0.0).astype(np.float32))
        self.sq = ops.sparse_rows(dev(np.where(rng.random((self.Q, 300)) < 0.05, rng.random((self.Q, 300)), 0.0).astype(np.float32)))
        docs = F.lexical_text(6, N)
        self.cut = [shard_bounds(N, 2, r) for r in range(2)]
        stats = LexicalStats.merge([BM25(docs[lo:hi], 1.5, 0.75, device="cpu").stats() for lo, hi in self.cut])
        self.whole = dict(dense=ShardedDenseIndex(Dn, ID0), sparse=ShardedSparseIndex(ops.sparse_index(Dm), ID0),
                          bm25=ShardedLexicalIndex(BM25(docs, 1.5, 0.75, id_base=ID0)))
        self.shards = [dict(sparse=ShardedSparseIndex(ops.sparse_index(Dm[lo:hi].contiguous()), ID0 + lo),
                            bm25=ShardedLexicalIndex(BM25(docs[lo:hi], 1.5, 0.75, stats=stats, id_base=ID0 + lo))) for lo, hi in self.cut]
        self.query = dict(dense=(self.Qn,), sparse=self.sq, bm25=(F.LEX_QUERIES,))
        self.planes = dict(sparse=ops.sparse_dot(self.whole["sparse"].index, *self.sq).clone(), bm25=self.whole["bm25"].model.scores(F.LEX_QUERIES).clone())
        self.names = ("dense", "sparse", "bm25")

    def forward(self, build: bool):
        """every sparse / lexical index with (True) or without (False) its forward index"""
        for part in [self.whole] + self.shards:
            if build:
                part["sparse"].build_forward(); part["bm25"].model.build_forward()
            else:
                part["sparse"].index.forward = None; part["bm25"].model.forward = None

    def scorers(self):
        return {n: (lambda U, ulen, n=n: self.whole[n].pair_scores(*self.query[n], U, ulen)) for n in self.names}

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


@pytest.fixture
def forward_preferred(ops, monkeypatch):
    from fusion_amd.retrievers.bm25 import TFIDF
    monkeypatch.setattr(ops, "SPARSE_PAIRS_PREFER_FORWARD", True)
    monkeypatch.setattr(TFIDF, "PREFER_FORWARD", True)


def test_two_shards_combine_to_the_whole_index(ops, corpus, forward_preferred):
    """Through the surface -- local_pair_scores / pair_scores pick the route up -- with a shard built with merged LexicalStats."""
    cand, lens = P.candidates(3, corpus.Q, 129, corpus.N, ID0)
    c, n = dev(cand), dev(lens)
    corpus.forward(False)
    plain = {name: corpus.whole[name].pair_scores(*corpus.query[name], c, n).clone() for name in ("sparse", "bm25")}
    corpus.forward(True)
    try:
        assert isinstance(corpus.whole["sparse"].index.forward, ops.SparseForward) and corpus.shards[1]["bm25"].model.forward.N == corpus.cut[1][1] - corpus.cut[1][0]
        for name in ("sparse", "bm25"):
            one = corpus.whole[name].pair_scores(*corpus.query[name], c, n)
            parts = [s[name].local_pair_scores(*corpus.query[name], c, n) for s in corpus.shards]
            assert same_bits(torch.maximum(parts[0], parts[1]), one), name
            assert same_bits(one, plain[name]) and same_bits(one, gather(corpus.planes[name], cand, lens, ID0)), name
            assert not bool(((parts[0] > float("-inf")) & (parts[1] > float("-inf"))).any())
        # the forward index is what ran: without its rows the sparse scores are gone
        corpus.shards[0]["sparse"].index.forward.rows[:, 1] = 0
        part = corpus.shards[0]["sparse"].local_pair_scores(*corpus.sq, c, n)
        assert bool(((part == 0) | (part == float("-inf"))).all())
        # gold_ranks follows doc_scores
        gold = dev(np.array([[ID0 + 3, ID0 + 250, -1]] * corpus.Q, dtype=np.int64))
        ranks = corpus.whole["bm25"].gold_ranks(F.LEX_QUERIES, gold)
        corpus.forward(False)
        assert torch.equal(ranks, corpus.whole["bm25"].gold_ranks(F.LEX_QUERIES, gold))
    finally:
        corpus.forward(False)


def test_completion_is_the_same_with_forward_indexes(ops, corpus, forward_preferred):
    from fusion_amd.retrievers.hybrid import Aggregator
    corpus.forward(False)
    cut = corpus.search(K)
    want = Aggregator.complete_topk(cut, corpus.scorers())
    corpus.forward(True)
    try:
        got = Aggregator.complete_topk(cut, corpus.scorers())
        ranked = corpus.whole["sparse"].rerank(*corpus.sq, cut["sparse"].ids)
    finally:
        corpus.forward(False)
    for name in corpus.names:
        a, b = want[name], got[name]
        assert b.k == a.k > K and torch.equal(a.ids, b.ids) and same_bits(a.scores, b.scores) and a.lens.tolist() == b.lens.tolist(), name
        assert (a.scores64 is None) == (b.scores64 is None) and (a.scores64 is None or same_bits(a.scores64, b.scores64)), name
    assert torch.equal(ranked.ids, cut["sparse"].ids) and same_bits(ranked.scores, cut["sparse"].scores)
