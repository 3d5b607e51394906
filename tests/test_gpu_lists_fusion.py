"""GPU tests of the top-k list fusion (csrc/lists.hip -> ops.lists_join -> Aggregator.fuse_topk): the reference's own outputs on
every list-form fixture, the corpus-scale shape against the CPU oracle and against the dense device path, the structure edges of
the join, determinism, and the three corpus-scale searches feeding one fusion.  Comparison rule: topk_fuse_util (that of
tests/test_gpu_parity.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from topk_fuse_util import EXACT, METHODS, Case, assert_fused_equal, lists_of

pytestmark = pytest.mark.gpu

ID_BASE = 3 << 31            # a first global id beyond 32 bits
CORPUS = 8_841_823           # mMARCO's passages


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def topk_of(ids, scores, lens):
    """ids [Q, L] int64, scores [Q, L] float64 (host), lens [Q] -> RankedTopk on the device (float32 scores; the float64 ones next to
    them when they are not float32 values, as Aggregator._to_device keeps them)."""
    from fusion_amd.planes import RankedTopk
    s32 = scores.astype(np.float32)
    exact32 = np.array_equal(s32.astype(np.float64), scores, equal_nan=True)
    return RankedTopk(ids=torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).cuda(), scores=torch.from_numpy(s32).cuda(),
                      lens=torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda(),
                      scores64=None if exact32 else torch.from_numpy(np.ascontiguousarray(scores)).cuda())


def systems_of(names, ids, scores, lens, widths=None):
    """[S, Q, L] arrays -> {name: RankedTopk}, system s cut to its own width (default: its longest list, at least 1)."""
    out = {}
    for s, n in enumerate(names):
        k = int(widths[s]) if widths is not None else max(int(lens[s].max(initial=0)), 1)
        out[n] = topk_of(ids[s][:, :k], scores[s][:, :k], lens[s])
    return out


def dict_lists(names, ids, scores, lens, rows):
    return {n: [[{"corpus_id": int(ids[s, q, r]), "score": float(scores[s, q, r])} for r in range(lens[s, q])] for q in rows]
            for s, n in enumerate(names)}


def rows_of(fused, rows=None):
    """FusedTopk -> list of (ids int64, scores float64) for the given queries (all by default), read off the tensors."""
    ids, sc, lens = fused.ids.cpu().numpy(), fused.scores.cpu().numpy().astype(np.float64), fused.lens.cpu().numpy()
    return [(ids[q, :lens[q]], sc[q, :lens[q]]) for q in (range(ids.shape[0]) if rows is None else rows)]


# ---- 1. the reference's outputs on every list-form fixture ------------------------------------------------------------------------
FUSE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "fuse_*.npz")))
TOPK_FILES = sorted(glob.glob(os.path.join(GOLDEN, "topkfuse_*.npz")))


def test_fixture_selection(ops):
    cap = ops.lists_max_entries()
    assert cap >= 8192
    assert sum(Case(p).max_entries() <= cap for p in FUSE_FILES) >= 10 and len(TOPK_FILES) >= 5


@pytest.mark.parametrize("path", FUSE_FILES + TOPK_FILES, ids=[os.path.basename(p)[:-4] for p in FUSE_FILES + TOPK_FILES])
def test_fuse_topk_matches_reference_golden(path, ops, oracle):
    from fusion_amd.retrievers.hybrid import Aggregator
    c = Case(path)
    if c.max_entries() > ops.lists_max_entries():      # a full-corpus fixture (100,591 entries per query): the dense path's ground
        with pytest.raises(ValueError, match=str(ops.lists_max_entries())):
            Aggregator.fuse_topk(systems_of(c.systems, c.ids, c.scores, c.lens), "rrf")
        return
    systems = systems_of(c.systems, c.ids, c.scores, c.lens)
    for pair in METHODS:
        got = Aggregator.fuse_topk(systems, pair[0], pair[1], c.weights, c.distr)
        assert got.scores.dtype == (torch.float64 if pair in {("rrf", "none"), ("bcf", "none"), ("nsf", "none")} else torch.float32)
        exp = c.expected(pair, oracle)
        assert_fused_equal(rows_of(got), exp, pair, os.path.basename(path))
        assert_fused_equal(lists_of(got.to_lists()), exp, pair, os.path.basename(path) + " to_lists")
        for q, l in enumerate(got.to_lists()):          # the reference's types (hybrid.py:258, 307)
            assert all(type(x["score"]) is (float if got.scores.dtype == torch.float64 else np.float32) and type(x["corpus_id"]) is int for x in l)
        cut = Aggregator.fuse_topk(systems, pair[0], pair[1], c.weights, c.distr, topk=7)
        assert cut.ids.shape[1] <= 7 and cut.predictions() == [r[0][:7].tolist() for r in rows_of(got)] == got.predictions(7)


# ---- 2. + 4. the corpus-scale shape ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus_scale():
    """Q = 1024 queries, S = 3 systems, k = 1000: ids out of an 8,841,823-id space offset beyond 2^32, every query's three lists drawn
    from a pool of 2,500 candidates (about 40 % of a list is in another one); BM25-like / cosine-like scores."""
    from oracle.gen_golden import synth_system_scores
    rng = np.random.default_rng(808)
    Q, S, k = 1024, 3, 1000
    names = ["bm25", "dpr", "splade"]
    ids = np.empty((S, Q, k), dtype=np.int64)
    sc = np.empty((S, Q, k), dtype=np.float64)
    for q in range(Q):
        pool = np.unique(rng.integers(0, CORPUS, 2700))
        assert pool.size >= 2500
        pool = rng.permutation(pool)[:2500] + ID_BASE
        for s, n in enumerate(names):
            v = synth_system_scores(rng, n, k, "plain")
            ids[s, q] = pool[rng.permutation(2500)[:k]]
            sc[s, q] = v[np.lexsort((np.arange(k), -v.astype(np.float64)))]
    lens = np.full((S, Q), k, dtype=np.int32)
    weights = {"bm25": 0.5, "dpr": 0.3, "splade": 0.2}
    distr = {n: np.quantile(sc[s, :64].ravel(), np.linspace(0, 1, 101)) for s, n in enumerate(names)}
    return names, ids, sc, lens, weights, distr, systems_of(names, ids, sc, lens)


def test_corpus_scale_matches_oracle_and_dense_path(corpus_scale, ops, oracle):
    from fusion_amd.retrievers.hybrid import Aggregator
    names, ids, sc, lens, weights, distr, systems = corpus_scale
    Q = ids.shape[1]
    sample = sorted(np.random.default_rng(5).choice(Q, size=16, replace=False).tolist())
    sample_lists = dict_lists(names, ids, sc, lens, sample)
    fused = {pair: Aggregator.fuse_topk(systems, pair[0], pair[1], weights, distr) for pair in METHODS}
    for pair, f in fused.items():
        assert f.ids.shape == (Q, 3000) and int(f.lens.min()) >= 1000 and int(f.lens.max()) <= 2500
        exp = lists_of(oracle.fuse_lists(sample_lists, pair[0], pair[1], weights, distr))
        assert_fused_equal(rows_of(f, sample), exp, pair, "oracle")
    # the parent's only route for such lists: dicts -> planes over the block's union of ids -> the dense kernels, 8 queries at a time
    for lo in range(0, 128, 8):
        rows = list(range(lo, lo + 8))
        block = dict_lists(names, ids, sc, lens, rows)
        for pair in METHODS:
            dense = Aggregator.fuse(block, pair[0], pair[1], weights, distr, as_device=True)
            assert dense.order.shape[1] <= 24000
            assert_fused_equal(rows_of(fused[pair], rows), lists_of(dense.to_lists()), pair, f"dense path, queries {lo}..{lo + 7}")


def test_corpus_scale_is_deterministic(corpus_scale):
    from fusion_amd.retrievers.hybrid import Aggregator
    names, ids, sc, lens, weights, distr, systems = corpus_scale
    for pair in METHODS:
        a = Aggregator.fuse_topk(systems, pair[0], pair[1], weights, distr)
        b = Aggregator.fuse_topk(systems, pair[0], pair[1], weights, distr)
        bits = torch.int64 if a.scores.dtype == torch.float64 else torch.int32
        assert torch.equal(a.ids, b.ids) and torch.equal(a.lens, b.lens), pair
        assert torch.equal(a.scores.contiguous().view(bits), b.scores.contiguous().view(bits)), pair


def test_topk_cut_of_the_corpus_scale_lists(corpus_scale):
    from fusion_amd.retrievers.hybrid import Aggregator
    names, ids, sc, lens, weights, distr, systems = corpus_scale
    for pair in (("rrf", "none"), ("nsf", "min-max")):
        full = Aggregator.fuse_topk(systems, pair[0], pair[1], weights, distr)
        cut = Aggregator.fuse_topk(systems, pair[0], pair[1], weights, distr, topk=1000)
        assert cut.ids.shape == (1024, 1000) and bool((cut.lens == 1000).all())
        assert torch.equal(cut.ids, full.ids[:, :1000]) and torch.equal(cut.scores, full.scores[:, :1000])


# ---- 3. structure edges of the join ----------------------------------------------------------------------------------------------
EDGE_PAIRS = [("rrf", "none"), ("bcf", "none"), ("nsf", "none"), ("nsf", "min-max")]      # exact pairs: lists identical, bit for bit


def random_lists(rng, lens_sq, widths, relation="overlap", id_of=None):
    """[S, Q] list lengths -> ([S, Q, L] ids, scores): distinct ids inside a list; `relation` between a query's lists."""
    S, Q = lens_sq.shape
    L = max(int(max(widths)), 1)
    ids = np.full((S, Q, L), -1, dtype=np.int64)
    sc = np.zeros((S, Q, L), dtype=np.float64)
    id_of = id_of or (lambda j: ID_BASE + 7 * j)
    for q in range(Q):
        total = int(lens_sq[:, q].sum())
        universe = rng.permutation(max(2 * total, 8))
        at = 0
        for s in range(S):
            n = int(lens_sq[s, q])
            if relation == "same":
                pick = rng.permutation(universe[:n])
            elif relation == "disjoint":
                pick = universe[at:at + n]; at += n
            else:
                pick = rng.permutation(universe)[:n]
            ids[s, q, :n] = [id_of(int(j)) for j in pick]
            v = np.sort(rng.choice(np.arange(1, 40, dtype=np.float32) / 8, size=n))[::-1]      # few distinct values: ties everywhere
            sc[s, q, :n] = v
    return ids, sc


def check_edge(oracle, lens_sq, widths, relation="overlap", id_of=None, seed=0, strided=False):
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    rng = np.random.default_rng(seed)
    lens_sq = np.asarray(lens_sq, dtype=np.int32)
    S, Q = lens_sq.shape
    names = [f"s{s}" for s in range(S)]
    ids, sc = random_lists(rng, lens_sq, widths, relation, id_of)
    systems = systems_of(names, ids, sc, lens_sq, widths)
    if strided:      # every system a view into a wider tensor, each with another row stride; padding slots hold -1
        for s, n in enumerate(names):
            t = systems[n]
            wide_i = torch.full((Q, t.k + 3 + 5 * s), -1, dtype=torch.int64, device="cuda")
            wide_s = torch.full((Q, t.k + 3 + 5 * s), float("-inf"), dtype=torch.float32, device="cuda")
            wide_i[:, :t.k] = t.ids; wide_s[:, :t.k] = t.scores
            systems[n] = RankedTopk(ids=wide_i[:, :t.k], scores=wide_s[:, :t.k], lens=t.lens)
            assert systems[n].ids.stride(0) != t.k
    weights = {n: 0.25 + 0.125 * s for s, n in enumerate(names)}
    lists = dict_lists(names, ids, sc, lens_sq, range(Q))
    for pair in EDGE_PAIRS:
        got = Aggregator.fuse_topk(systems, pair[0], pair[1], weights, {})
        assert got.lens.tolist() == [len(set(ids[:, q][ids[:, q] >= 0].tolist())) for q in range(Q)]
        assert_fused_equal(rows_of(got), lists_of(oracle.fuse_lists(lists, pair[0], pair[1], weights, {})), pair, f"{lens_sq.tolist()} {relation}")
    return systems


@pytest.mark.parametrize("total", [1, 63, 64, 65, 1024, 1025, 2049])   # a wave's and a chunk's edges, as the columns test has them
def test_join_total_entries_around_one_wave(total, oracle):
    a = (total + 1) // 2
    check_edge(oracle, [[a, total], [total - a, 0]], [max(a, total), max(total - a, 1)], seed=total)


def test_join_at_the_capacity(ops, oracle):
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    cap = ops.lists_max_entries()
    k = cap // 8
    # S = 8 x k = 1024: at the capacity (query 0), one below it (query 1); nothing in common -> union = S x k
    check_edge(oracle, [[k, k - 1]] + [[k, k]] * 7, [k] * 8, relation="disjoint", seed=1)
    check_edge(oracle, [[k, k]] * 8, [k] * 8, relation="same", seed=2)                        # all list the same ids -> union = k
    check_edge(oracle, [[k, 17]] * 8, [k] * 8, seed=3)
    check_edge(oracle, [[cap, cap - 1]], [cap], seed=4)                                       # S = 1: chunks of one list
    over = {f"s{s}": RankedTopk(ids=torch.zeros((2, k + (s == 3)), dtype=torch.int64, device="cuda"),
                                scores=torch.zeros((2, k + (s == 3)), device="cuda"),
                                lens=torch.zeros(2, dtype=torch.int32, device="cuda")) for s in range(8)}
    with pytest.raises(ValueError, match=str(cap + 1)):
        Aggregator.fuse_topk(over, "rrf")


def test_join_single_system_and_empty_lists(oracle):
    from fusion_amd.retrievers.hybrid import Aggregator
    check_edge(oracle, [[10, 1, 0, 7]], [10], seed=5)                                          # S = 1
    check_edge(oracle, [[10, 0, 0], [0, 10, 0], [5, 5, 0]], [10, 10, 10], seed=6)              # one system empty; every system empty
    systems = check_edge(oracle, [[0, 0], [0, 0]], [4, 4], seed=7)                             # nothing listed at all
    none = Aggregator.fuse_topk(systems, "rrf")
    assert none.lens.tolist() == [0, 0] and none.to_lists() == [[], []] and bool((none.ids == -1).all())


def test_join_lists_of_different_k_and_row_strides(oracle):
    check_edge(oracle, [[1000, 640, 1000], [10, 10, 3], [1, 1, 0]], [1000, 10, 1], seed=8, strided=True)
    check_edge(oracle, [[1, 1], [1000, 999], [10, 2]], [1, 1000, 10], seed=9, strided=True)


def test_join_hash_adversarial_ids(oracle):
    check_edge(oracle, [[1000, 500], [1000, 1000], [1000, 7]], [1000] * 3, id_of=lambda j: 16384 * j, seed=10)            # multiples of the table size
    check_edge(oracle, [[1000, 500], [1000, 1000], [1000, 7]], [1000] * 3, id_of=lambda j: (j << 32) | 5, seed=11)        # differ only above bit 32
    check_edge(oracle, [[1000, 500], [1000, 1000]], [1000] * 2, id_of=lambda j: (1 << 62) - (j << 14), seed=12)
    check_edge(oracle, [[64, 64], [64, 3]], [64] * 2, id_of=lambda j: j * 0x61C8864680B583EB % (1 << 63), seed=13)


def test_numpy_float64_weights_and_unknown_method(oracle):
    """NumPy's scalar promotion (hybrid.py:291): an np.float64 weight makes that product and the document's running sum float64 from
    there on, a Python float keeps float32 -- per system, as fz_fuse_wsum_f64 distinguishes them; an unknown method sums the raw
    scores.  Float64 raw scores (BM25's) stay unrounded under 'none'."""
    from fusion_amd.retrievers.hybrid import Aggregator
    rng = np.random.default_rng(21)
    lens = np.array([[300, 40, 0], [200, 300, 5], [1, 300, 7]], dtype=np.int32)
    names = ["a", "b", "c"]
    ids, sc = random_lists(rng, lens, [300] * 3)
    sc[0] = sc[0] * 1.1 + 1e-9 * np.arange(sc.shape[2])[::-1]           # system a: not float32 values, still descending
    systems = systems_of(names, ids, sc, lens, [300] * 3)
    assert systems["a"].scores64 is not None and systems["b"].scores64 is None
    lists = dict_lists(names, ids, sc, lens, range(3))
    for weights in ({"a": np.float64(0.3), "b": np.float64(0.5), "c": np.float64(0.2)},      # the tuning grid's weights: all wide
                    {"a": 0.3, "b": np.float64(0.5), "c": 0.2},                               # float32 sums until the first wide product
                    {"a": np.float64(0.3), "b": 0.5, "c": np.float32(0.2)}):
        for pair in (("nsf", "min-max"), ("nsf", "none"), ("nsf", "no-such-normalisation"), ("no-such-method", None)):
            got = Aggregator.fuse_topk(systems, pair[0], pair[1], weights, {})
            assert got.scores.dtype == torch.float64
            exp = lists_of(oracle.fuse_lists(lists, pair[0], pair[1], weights, {}))
            assert_fused_equal(rows_of(got), exp, ("nsf", "min-max"), f"{pair} {weights}")      # the exact rule: ids and bits


def test_join_reports_a_duplicated_id(ops):
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator

    def system(ids_row, k):
        ids = torch.full((2, k), -1, dtype=torch.int64, device="cuda")
        ids[0, :k] = torch.arange(k, device="cuda") + ID_BASE             # query 0: clean
        ids[1, :len(ids_row)] = torch.tensor(ids_row, dtype=torch.int64, device="cuda")
        return RankedTopk(ids=ids, scores=torch.zeros((2, k), device="cuda"),
                          lens=torch.tensor([k, len(ids_row)], dtype=torch.int32, device="cuda"))

    clean = system([5, 6, 7], 2000)
    assert Aggregator.fuse_topk({"a": clean, "b": clean}, "rrf").lens.tolist() == [2000, 3]
    far = list(range(100, 1600)); far[1400] = far[3]                       # the same id in two chunks of one list
    cases = {"in one chunk": {"a": system([5, 6, 5], 2000)},
             "across chunks": {"a": system(far, 2000)},
             "both already listed by an earlier system": {"a": clean, "b": system([9, 6, 8, 6], 2000)}}
    for what, systems in cases.items():
        with pytest.raises(ValueError, match="same id twice"):
            Aggregator.fuse_topk(systems, "rrf")
        with pytest.raises(ValueError, match="same id twice"):
            Aggregator.fuse_topk(systems, "nsf", "none", {n: 1.0 for n in systems}, {})
    # padding slots are never read as ids: -1 twice past the lengths is no duplicate
    assert Aggregator.fuse_topk({"a": system([5], 2000), "b": system([], 2000)}, "bcf").lens.tolist() == [2000, 1]


# ---- 5. three corpus-scale searches feed one fusion -------------------------------------------------------------------------------
def synthetic_text(rng, n_docs, lo, hi, vocab_size=3000):
    vocab = np.array([f"w{i}" for i in range(vocab_size)])
    p = 1.0 / np.arange(1, vocab_size + 1); p /= p.sum()
    sizes = rng.integers(lo, hi, n_docs)
    words = rng.choice(vocab, size=int(sizes.sum()), p=p)
    cut = np.cumsum(sizes)[:-1]
    return [" ".join(w) for w in np.split(words, cut)]


@pytest.mark.parametrize("N", [5_003, 100_003], ids=["one_sort_row", "beyond_one_sort_row"])
def test_bm25_search_topk_equals_ranked_positions(N, ops):
    from fusion_amd.retrievers.bm25 import BM25
    rng = np.random.default_rng(N)
    docs = synthetic_text(rng, N, 3, 30)
    queries = synthetic_text(rng, 12, 2, 8) + ["zzz"]
    m = BM25(docs, 1.5, 0.75)
    assert (N <= ops.sort_max_n(torch.float64)) == (N == 5_003)
    for k in (10, 1000):
        rt = m.search_topk(queries, k)
        assert rt.ids.is_cuda and rt.ids.dtype == torch.int64 and rt.scores.dtype == torch.float32 and rt.scores64.dtype == torch.float64
        assert tuple(rt.ids.shape) == (len(queries), k) and rt.lens.tolist() == [k] * len(queries)
        pos = m.ranked_positions(queries, k)
        np.testing.assert_array_equal(rt.ids.cpu().numpy(), pos)
        plane = m.scores(queries).cpu().numpy()
        np.testing.assert_array_equal(rt.scores64.cpu().numpy(), np.take_along_axis(plane, pos, axis=1))
        np.testing.assert_array_equal(rt.scores.cpu().numpy(), rt.scores64.cpu().numpy().astype(np.float32))


def test_three_searches_feed_one_fusion(ops, oracle):
    from fusion_amd.distributed import ShardedDenseIndex, ShardedSparseIndex
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.bm25 import BM25
    from fusion_amd.retrievers.hybrid import Aggregator
    N, Q, k, V = 100_003, 24, 100, 1024
    rng = np.random.default_rng(77)
    g = torch.Generator(device="cuda").manual_seed(77)
    # DPR-shaped: unit vectors
    Dn = ops.normalize_rows(torch.randn((N, 64), generator=g, device="cuda"))
    Qn = ops.normalize_rows(torch.randn((Q, 64), generator=g, device="cuda"))
    d_sc, d_ids = ShardedDenseIndex(Dn, ID_BASE).search(Qn, k)
    # SPLADE-shaped: ~24 of V terms per row
    def splade_like(n, nnz):
        cols = torch.randint(0, V, (n, nnz), generator=g, device="cuda")
        w = torch.rand((n, nnz), generator=g, device="cuda") + 0.05
        return torch.zeros((n, V), device="cuda").scatter_reduce_(1, cols, w, reduce="amax")
    index = ops.sparse_index_from_blocks(((r0, ops.normalize_rows(splade_like(min(8192, N - r0), 24))) for r0 in range(0, N, 8192)), V, N=N)
    s_sc, s_ids = ShardedSparseIndex(index, ID_BASE).search(*ops.sparse_rows(splade_like(Q, 8), V), k=k)
    # BM25
    docs = synthetic_text(rng, N, 3, 30)
    queries = synthetic_text(rng, Q, 2, 8)
    bm25 = BM25(docs, 1.5, 0.75).search_topk(queries, k)
    bm25 = RankedTopk(ids=bm25.ids + ID_BASE, scores=bm25.scores, lens=bm25.lens, scores64=bm25.scores64)     # the shards' global ids
    systems = {"bm25": bm25, "dpr": RankedTopk.from_search(d_sc, d_ids), "splade": RankedTopk.from_search(s_sc, s_ids)}
    assert all(t.ids.is_cuda and t.scores.is_cuda and t.lens.is_cuda for t in systems.values())
    assert int(systems["dpr"].lens.min()) == k and int(systems["dpr"].ids.min()) >= ID_BASE
    weights = {"bm25": 0.2, "dpr": 0.5, "splade": 0.3}
    lists = {n: t.to_lists() for n, t in systems.items()}
    assert all(len(lists[n]) == Q for n in lists)
    for pair in (("rrf", "none"), ("nsf", "min-max"), ("nsf", "none")):
        assert pair in EXACT
        got = Aggregator.fuse_topk(systems, pair[0], pair[1], weights, {})
        assert_fused_equal(rows_of(got), lists_of(oracle.fuse_lists(lists, pair[0], pair[1], weights, {})), pair, "three searches")
        top = Aggregator.fuse_topk(systems, pair[0], pair[1], weights, {}, topk=k)
        assert top.predictions() == [r[0][:k].tolist() for r in rows_of(got)]
