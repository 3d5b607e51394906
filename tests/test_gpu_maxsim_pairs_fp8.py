"""Candidate-list MaxSim over e4m3 token rows (csrc/rerank8.hip, ops.maxsim_pairs_e4m3, ShardedTokenIndex.quantize / build_e4m3) on the GPU.

1. Grid inputs (maxsim_pairs_fp8_cases.py: integers, nothing to round in float32 whatever the order): bit equality with the float64
   formula gathered at the candidates; poison rows before, after and inside the corpus, every absent-slot kind, rounds of 1 to 8 row
   blocks, strided candidates and a sentinel-padded score plane, two id bases.
2. The descale: float16 multiples of 1/4 quantised on the device; the bits of the float64 formula over the float16 tokens.
3. Unit-norm tokens: bit equality with the all-pairs e4m3 kernel (ops.maxsim_e4m3 gathered at the candidates), twice.
4. Special values (NaN bytes, saturated rows): the all-pairs e4m3 kernel's bits through the integer view.
5. Empty shapes and the default output plane.
6. ShardedTokenIndex as an e4m3 shard: quantize, rerank (order, ties, lens, padding), two shards against one, build_e4m3 against
   build_centroids + quantize, memory_bytes, dequantized, Ranker.multi_vector_rerank and Aggregator.fuse_topk."""
import numpy as np
import pytest
import torch

import maxsim_cases as M
import maxsim_fp8_cases as F
import maxsim_pairs_fp8_cases as P8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. grid inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc_len", P8.MAX_DOC_LENS)
@pytest.mark.parametrize("Q", P8.QS)
@pytest.mark.parametrize("Lq", M.LQS)
def test_grid_candidates_are_exact(ops, Lq, Q, max_doc_len):
    D8_h, Doff_h = P8.corpus(max_doc_len)
    ref = P8.reference(Lq, Q, max_doc_len)
    Q8, D8, Doff = dev(P8.queries(Lq, Q)), dev(D8_h), dev(Doff_h)
    for k in P8.KS:
        for id_base in P8.ID_BASES:
            cand_h = P8.candidates(Q, k, id_base)
            cand_full = torch.full((Q, k + 3), id_base, dtype=torch.int64, device="cuda")      # ldc = k + 3
            cand_full[:, :k] = dev(cand_h)
            for cl in P8.launches(Q, k):
                out_full = torch.full((Q, k + 5), P8.SENTINEL, dtype=torch.float32, device="cuda")      # lds = k + 5
                got = ops.maxsim_pairs_e4m3(Q8, D8, Doff, cand_full[:, :k], None if cl is None else dev(cl), q_exp=0, d_exp=0, id_base=id_base,
                                            max_doc_len=max_doc_len, out=out_full[:, :k])
                assert got.data_ptr() == out_full.data_ptr()
                exp = P8.expected(ref, cand_h, np.full(Q, k) if cl is None else cl, id_base)
                got_h = out_full.cpu().numpy()
                what = (Lq, Q, max_doc_len, k, id_base, None if cl is None else cl.tolist())
                bad = np.argwhere(got_h[:, :k].view(np.int32) != exp.view(np.int32))
                assert len(bad) == 0, (what, len(bad), [(int(q), int(r), int(cand_h[q, r]), float(got_h[q, r]), float(exp[q, r])) for q, r in bad[:8]])
                assert (got_h[:, k:] == P8.SENTINEL).all(), (what, "padding columns of the score plane were written")


# ---- 2. the descale ------------------------------------------------------------------------------------------------------------------
DESCALE = [c for c in F.DESCALE_CASES if (c.name, c.Lq) in {("lengths", 32), ("end-both", 64)}]
assert len(DESCALE) == 2


@pytest.mark.parametrize("q_exp", (8, 6))
@pytest.mark.parametrize("case", DESCALE, ids=lambda c: c.id)
def test_quarter_tokens_give_the_float16_formula(ops, case, q_exp):
    """Multiples of 1/4 quantise without loss at 2^8 (queries: at 2^6 too), so the score over the bytes, descaled by 2^-(q_exp + 8), is
    the float64 formula over the float16 tokens, bit for bit; the bytes come from the device quantiser."""
    Qh, Dh, Doff = F.quarter_tokens(case)
    ref = F.exact_f32(F.maxsim_ref(Qh, Dh, Doff, case.max_doc_len))
    Q, N = ref.shape
    rng = np.random.default_rng(17)
    cand_h = rng.integers(0, N, (Q, 70)).astype(np.int64)
    cand_h[:, : min(N, 70)] = np.stack([rng.permutation(N)[:70] for _ in range(Q)])[:, : min(N, 70)]
    Q8, D8 = ops.quantize_e4m3(dev(Qh), q_exp), ops.quantize_e4m3(dev(Dh), 8)
    got = ops.maxsim_pairs_e4m3(Q8, D8, dev(Doff), dev(cand_h), q_exp=q_exp, d_exp=8, max_doc_len=case.max_doc_len).cpu().numpy()
    exp = np.take_along_axis(ref, cand_h, axis=1)
    assert np.array_equal(got.view(np.int32), exp.view(np.int32)), (case.id, q_exp, int((got != exp).sum()))
    assert np.abs(exp).max() > 1 and len(np.unique(exp)) > 10
    if q_exp == 8:
        dflt = ops.maxsim_pairs_e4m3(Q8, D8, dev(Doff), dev(cand_h), max_doc_len=case.max_doc_len).cpu().numpy()
        assert np.array_equal(dflt.view(np.int32), exp.view(np.int32)), "the defaults are 8 and 8"


# ---- 3. unit-norm tokens: the all-pairs e4m3 kernel's bits ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unit(ops):
    rng = np.random.default_rng(78)
    lens = rng.integers(0, 121, 2000)
    Dtok, Doff = M.unit_corpus(rng, lens, pre=3, post=9)
    pos = rng.integers(0, 2000, (64, 1000)).astype(np.int64)
    D8 = ops.quantize_e4m3(dev(Dtok), 8)
    return D8, dev(Doff), dev(pos), {Lq: ops.quantize_e4m3(dev(M.unit_queries(np.random.default_rng(Lq + 1), 64, Lq)), 8) for Lq in M.LQS}


@pytest.mark.parametrize("Lq", M.LQS)
def test_unit_norm_bits_equal_the_all_pairs_kernel(ops, unit, Lq):
    D8, Doff, pos, Qs = unit
    plane = ops.maxsim_e4m3(Qs[Lq], D8, Doff, max_doc_len=120)
    want = bits(torch.gather(plane, 1, pos))
    for id_base in (0, 2 ** 40):
        a = ops.maxsim_pairs_e4m3(Qs[Lq], D8, Doff, pos + id_base, id_base=id_base, max_doc_len=120)
        b = ops.maxsim_pairs_e4m3(Qs[Lq], D8, Doff, pos + id_base, id_base=id_base, max_doc_len=120)
        assert torch.equal(bits(a), want), (Lq, id_base, int((bits(a) != want).sum()))
        assert torch.equal(bits(a), bits(b)), "two calls differ"
    assert torch.isfinite(plane).all() and float(plane.abs().max()) > 1.0     # not a comparison of zeros
    # truncation: the same with max_doc_len = 40
    plane40 = ops.maxsim_e4m3(Qs[Lq], D8, Doff, max_doc_len=40)
    for id_base in (0, 2 ** 40):
        got = ops.maxsim_pairs_e4m3(Qs[Lq], D8, Doff, pos + id_base, id_base=id_base, max_doc_len=40)
        assert torch.equal(bits(got), bits(torch.gather(plane40, 1, pos))), (Lq, id_base)


# ---- 4. special values -----------------------------------------------------------------------------------------------------------------
def test_special_values_carry_the_all_pairs_bits(ops):
    Q8, D8, Doff = (dev(x) for x in F.special_bytes())
    plane = ops.maxsim_e4m3(Q8, D8, Doff, q_exp=0, d_exp=0, max_doc_len=512)
    # the all-pairs kernel's own special values (tests/test_gpu_maxsim_fp8.py::test_special_values): a document of NaN rows only gives -inf,
    # a NaN byte's row is skipped, an empty document scores 0; whatever the plane holds is compared through the integer view
    assert torch.isneginf(plane[:, 2]).all() and torch.isfinite(plane[:, 1]).all() and not plane[:, 4].any()
    N = Doff.numel() - 1
    pos = torch.arange(N, device="cuda").repeat(3, 3)[:, torch.randperm(3 * N, generator=torch.Generator().manual_seed(1)).cuda()]
    got = ops.maxsim_pairs_e4m3(Q8, D8, Doff, pos, q_exp=0, d_exp=0, max_doc_len=512)
    assert torch.equal(bits(got), bits(torch.gather(plane, 1, pos)))


# ---- 5. empty shapes -------------------------------------------------------------------------------------------------------------------
def test_default_output_plane_and_empty_shapes(ops):
    D8_h, Doff_h = P8.corpus(512)
    Q8, D8, Doff = dev(P8.queries(64, 2)), dev(D8_h), dev(Doff_h)
    cand = dev(P8.candidates(2, 7, 0))
    got = ops.maxsim_pairs_e4m3(Q8, D8, Doff, cand, q_exp=0, d_exp=0, max_doc_len=512)
    assert got.shape == (2, 7) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.int32), P8.expected(P8.reference(64, 2, 512), cand.cpu().numpy(), [7, 7], 0).view(np.int32))
    # the bytes as torch.float8_e4m3fn tensors
    again = ops.maxsim_pairs_e4m3(Q8.view(torch.float8_e4m3fn), D8.view(torch.float8_e4m3fn), Doff, cand, q_exp=0, d_exp=0, max_doc_len=512)
    assert torch.equal(bits(again), bits(got))
    assert ops.maxsim_pairs_e4m3(Q8, D8, Doff, cand[:, :0]).shape == (2, 0)
    assert ops.maxsim_pairs_e4m3(Q8[:0], D8, Doff, cand[:0]).shape == (0, 7)
    # a shard without documents owns nothing
    none = ops.maxsim_pairs_e4m3(Q8, D8[:0], Doff[:1] * 0, cand)
    assert none.shape == (2, 7) and torch.isneginf(none).all()


# ---- 6. the index and the ranker -----------------------------------------------------------------------------------------------------
def host_list(plane_rows, cand_row, id_base, N):
    """One query's reranked list built on the host from its row of the all-pairs plane: owned candidates in stable descending order."""
    owned = [(float(plane_rows[c - id_base]), r, int(c)) for r, c in enumerate(cand_row) if c >= 0 and 0 <= c - id_base < N]
    owned.sort(key=lambda t: -t[0])      # stable: ties keep candidate order
    return [c for _, _, c in owned], np.array([s for s, _, _ in owned], dtype=np.float32)


TIED = (1003, 1010, 1011, 1012, 1013, 1014)


@pytest.fixture(scope="module")
def tied(ops):
    """A unit-norm corpus in which documents 10..14 share their token rows with document 3 (equal scores for every query), 200 documents;
    with it the all-pairs e4m3 plane of the quantised tokens, the definition of every score below."""
    rng = np.random.default_rng(12)
    lens = rng.integers(1, 90, 200)
    lens[10:15] = lens[3]
    Dtok, Doff = M.unit_corpus(rng, lens)
    for d in range(10, 15):
        Dtok[int(Doff[d]): int(Doff[d + 1])] = Dtok[int(Doff[3]): int(Doff[4])]
    Qtok = M.unit_queries(rng, 6, 64)
    id_base = 1000
    cand = rng.integers(0, 200, (6, 50)).astype(np.int64) + id_base
    cand[:, 5], cand[:, 7], cand[:, 20], cand[:, 33], cand[:, 40] = 1012, 1003, 1010, 1014, 1003      # the tied documents, one of them twice
    cand[1, 9], cand[1, 49] = -1, -1
    cand[2, 11], cand[2, 12] = id_base - 1, id_base + 200
    plane = ops.maxsim_e4m3(ops.quantize_e4m3(dev(Qtok)), ops.quantize_e4m3(dev(Dtok)), dev(Doff), max_doc_len=512).cpu().numpy()
    return Qtok, Dtok, Doff, cand, id_base, plane


def test_quantized_index_scores_and_memory(ops, tied):
    from fusion_amd.distributed import ShardedTokenIndex
    Qtok_h, Dtok_h, Doff_h, cand_h, id_base, plane = tied
    Qtok, Dtok, Doff, cand = dev(Qtok_h), dev(Dtok_h), dev(Doff_h), dev(cand_h)
    sumL = Dtok.shape[0]
    index = ShardedTokenIndex(Dtok, Doff, id_base)
    assert index.memory_bytes()["tokens"] == 256 * sumL
    assert index.quantize() is index and index.Dtok is None and index.d_exp == 8 and index.tok8.dtype == torch.uint8
    assert torch.equal(index.tok8, ops.quantize_e4m3(Dtok)) and index.memory_bytes()["tokens"] == 128 * sumL == index.memory_bytes()["total"]
    want = ops.maxsim_pairs_e4m3(ops.quantize_e4m3(Qtok), ops.quantize_e4m3(Dtok), Doff, cand, id_base=id_base, max_doc_len=512)
    got = index.local_scores(Qtok, cand)
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(index.pair_scores(Qtok, cand)), bits(want))
    assert np.array_equal(got.cpu().numpy().view(np.int32), P8.expected(plane, cand_h, [50] * 6, id_base).view(np.int32))
    assert torch.equal(index.dequantized(), ops.dequantize_e4m3(index.tok8, 8)) and index.dequantized().dtype == torch.float32
    assert torch.equal(index.dequantized(5, 9), ops.dequantize_e4m3(index.tok8[5:9], 8))
    with pytest.raises(ValueError):
        index.quantize()
    # keep_tokens: both matrices resident, the e4m3 one still decides the score; other exponents on both sides
    kept = ShardedTokenIndex(Dtok, Doff, id_base).quantize(6, keep_tokens=True)
    assert kept.Dtok is Dtok and kept.d_exp == 6 and kept.memory_bytes()["tokens"] == 384 * sumL
    kept.q_exp = 7
    want67 = ops.maxsim_pairs_e4m3(ops.quantize_e4m3(Qtok, 7), ops.quantize_e4m3(Dtok, 6), Doff, cand, q_exp=7, d_exp=6, id_base=id_base)
    assert torch.equal(bits(kept.local_scores(Qtok, cand)), bits(want67)) and ShardedTokenIndex.q_exp == 8
    assert not torch.equal(bits(want67), bits(want))


def test_rerank_lists(ops, tied):
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.planes import RankedTopk
    Qtok_h, Dtok_h, Doff_h, cand_h, id_base, plane = tied
    Qtok, cand = dev(Qtok_h), dev(cand_h)
    N = len(Doff_h) - 1
    index = ShardedTokenIndex(dev(Dtok_h), dev(Doff_h), id_base).quantize()
    out = index.rerank(Qtok, cand)
    assert isinstance(out, RankedTopk) and out.ids.dtype == torch.int64 and out.scores.dtype == torch.float32 and out.lens.dtype == torch.int32
    ids, sc, lens = out.ids.cpu().numpy(), out.scores.cpu().numpy(), out.lens.cpu().numpy()
    for q in range(6):
        want_ids, want_sc = host_list(plane[q], cand_h[q], id_base, N)
        n = len(want_ids)
        assert lens[q] == n and n == (50, 48, 48, 50, 50, 50)[q]
        assert ids[q, :n].tolist() == want_ids                                   # descending, ties in candidate order
        assert np.array_equal(sc[q, :n].view(np.int32), want_sc.view(np.int32))
        assert (np.diff(sc[q, :n]) <= 0).all()
        assert (ids[q, n:] == -1).all() and np.isneginf(sc[q, n:]).all()
        tied_at = [i for i, c in enumerate(ids[q, :n]) if c in TIED]             # one run of equal scores ...
        assert len(tied_at) >= 5 and tied_at == list(range(tied_at[0], tied_at[0] + len(tied_at))) and len(set(sc[q, tied_at].tolist())) == 1
        assert ids[q, tied_at].tolist() == [c for c in cand_h[q].tolist() if c in TIED]      # ... in candidate order
    # cut to k, and a RankedTopk as the candidates (its lens cut the rows)
    cut = index.rerank(Qtok, cand, k=10)
    assert torch.equal(cut.ids, out.ids[:, :10]) and torch.equal(bits(cut.scores), bits(out.scores[:, :10])) and (cut.lens == 10).all()
    short = RankedTopk(ids=cand, scores=torch.zeros(cand.shape, device="cuda"), lens=torch.tensor([50, 30, 0, 7, 50, 1], dtype=torch.int32, device="cuda"))
    via = index.rerank(Qtok, short)
    for q, L in enumerate((50, 30, 0, 7, 50, 1)):
        want_ids, _ = host_list(plane[q], cand_h[q, :L], id_base, N)
        assert int(via.lens[q]) == len(want_ids) and via.ids[q, :len(want_ids)].tolist() == want_ids and (via.ids[q, len(want_ids):] == -1).all()


def test_two_shards_give_the_bits_of_one(ops, tied):
    from fusion_amd.distributed import ShardedTokenIndex
    Qtok_h, Dtok_h, Doff_h, cand_h, id_base, _ = tied
    Qtok, cand = dev(Qtok_h), dev(cand_h)
    whole = ShardedTokenIndex(dev(Dtok_h), dev(Doff_h), id_base).quantize().local_scores(Qtok, cand)
    cutd = 77
    t = int(Doff_h[cutd])
    lo = ShardedTokenIndex(dev(Dtok_h[:t]), dev(Doff_h[:cutd + 1]), id_base).quantize()
    hi = ShardedTokenIndex(dev(Dtok_h[t:]), dev(Doff_h[cutd:] - t), id_base + cutd).quantize()
    a, b = lo.local_scores(Qtok, cand), hi.local_scores(Qtok, cand)
    assert not (torch.isfinite(a) & torch.isfinite(b)).any()      # no slot is owned twice
    assert torch.equal(bits(torch.maximum(a, b)), bits(whole))


def test_build_e4m3_equals_build_centroids_and_quantize(ops, tied):
    from fusion_amd.distributed import ShardedTokenIndex
    Qtok_h, Dtok_h, Doff_h, _, id_base, _ = tied
    Qtok, Dtok, Doff = dev(Qtok_h), dev(Dtok_h), dev(Doff_h)
    sumL = Dtok.shape[0]
    C = ops.kmeans_centroids(Dtok, 64, iters=2, seed=1)
    cuts = [0, sumL // 3 + 1, sumL // 3 + 1, 2 * sumL // 3, sumL]      # three blocks and an empty one
    blocks = lambda: (Dtok_h[x:y] for x, y in zip(cuts[:-1], cuts[1:]))      # noqa: E731  host rows: moved to the device block by block
    blocks_t = lambda: (torch.from_numpy(b) for b in blocks())      # noqa: E731
    whole = ShardedTokenIndex(Dtok, Doff, id_base).build_centroids(C).quantize()
    built = ShardedTokenIndex.build_e4m3(blocks_t(), Doff, id_base, C=C)
    assert built.Dtok is None and built.d_exp == 8 and built.packed is None
    assert torch.equal(built.tok8, whole.tok8) and torch.equal(built.codes, whole.codes) and built.codes.dtype == whole.codes.dtype
    assert built.memory_bytes() == whole.memory_bytes() and built.memory_bytes()["tokens"] == 128 * sumL and built.memory_bytes()["candidates"] > 0
    assert torch.equal(built.candidates.index.coff, whole.candidates.index.coff) and torch.equal(built.candidates.index.cdoc, whole.candidates.index.cdoc)
    for k, ncand in ((10, 100), (50, 150)):
        a, b = built.search(Qtok, k=k, nprobe=8, ncand=ncand), whole.search(Qtok, k=k, nprobe=8, ncand=ncand)
        assert torch.equal(a.ids, b.ids) and torch.equal(bits(a.scores), bits(b.scores)) and torch.equal(a.lens, b.lens)
        assert int(a.lens.min()) >= 1
    # without C: the bytes alone; rerank works, search has no candidates to draw
    plain = ShardedTokenIndex.build_e4m3(blocks_t(), Doff, id_base, scale_exp=6)
    assert plain.candidates is None and plain.codes is None and plain.d_exp == 6
    assert torch.equal(plain.tok8, ops.quantize_e4m3(Dtok, 6))
    assert plain.memory_bytes() == dict(tokens=128 * sumL, codes=0, packed=0, candidates=0, total=128 * sumL)
    with pytest.raises(ValueError, match="centroid"):
        plain.search(Qtok, k=10, ncand=100)
    with pytest.raises(ValueError, match="more than"):
        ShardedTokenIndex.build_e4m3(iter([torch.from_numpy(Dtok_h), torch.from_numpy(Dtok_h[:1])]), Doff, id_base)
    with pytest.raises(ValueError, match="token rows"):
        ShardedTokenIndex.build_e4m3(iter([torch.from_numpy(Dtok_h[:-1])]), Doff, id_base)
    with pytest.raises(ValueError):
        whole.compress(2)


@pytest.mark.parametrize("method,norm", [("rrf", None), ("nsf", "min-max")])
def test_reranked_lists_fuse_like_host_built_ones(ops, tied, method, norm):
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    Qtok_h, Dtok_h, Doff_h, _, id_base, plane = tied
    Qtok = dev(Qtok_h)
    N = len(Doff_h) - 1
    rng = np.random.default_rng(3)
    # a dense system's lists over the same shard (distinct ids per list, the last one shorter); ColBERT reranks exactly these candidates
    cand_h = np.zeros((6, 50), dtype=np.int64)
    cand_h[:, :5] = (1012, 1003, 1010, 1014, 1011)      # tied for ColBERT
    for q in range(6):
        rest = [c for c in rng.permutation(N) + id_base if c not in (1012, 1003, 1010, 1014, 1011)]
        cand_h[q, 5:] = rest[:45]
    cand_h[5, 44:] = -1
    dense = RankedTopk.from_search(dev(np.where(cand_h >= 0, -np.sort(-rng.random((6, 50)).astype(np.float32), axis=1), -np.inf).astype(np.float32)),
                                   dev(cand_h))
    colbert = ShardedTokenIndex(dev(Dtok_h), dev(Doff_h), id_base).quantize().rerank(Qtok, dense)
    assert colbert.lens.tolist() == [50, 50, 50, 50, 50, 44]
    h_ids = np.full((6, 50), -1, dtype=np.int64)
    h_sc = np.full((6, 50), -np.inf, dtype=np.float32)
    for q in range(6):
        li, ls = host_list(plane[q], cand_h[q], id_base, N)
        h_ids[q, :len(li)], h_sc[q, :len(li)] = li, ls
    host = RankedTopk.from_search(dev(h_sc), dev(h_ids))
    w = {"dpr": 0.4, "colbert": 0.6}
    got = Aggregator.fuse_topk({"dpr": dense, "colbert": colbert}, method, norm, w, {})
    want = Aggregator.fuse_topk({"dpr": dense, "colbert": host}, method, norm, w, {})
    assert torch.equal(got.lens, want.lens) and torch.equal(got.ids, want.ids)
    assert torch.equal(got.scores.view(torch.int64 if got.scores.dtype == torch.float64 else torch.int32),
                       want.scores.view(torch.int64 if want.scores.dtype == torch.float64 else torch.int32))
    assert int(got.lens.min()) >= 40


def test_ranker_rerank_on_a_quantized_index_equals_the_e4m3_plane(ops):
    from fusion_amd import encoders
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.retrievers.hybrid import Ranker
    enc = encoders.random_init("colbert", size="tiny")
    rng = np.random.default_rng(22)
    words = [f"w{i}" for i in range(300)]
    docs = [" ".join(rng.choice(words, size=int(rng.integers(3, 40)))) for _ in range(120)]
    queries = [" ".join(rng.choice(words, size=int(rng.integers(2, 9)))) for _ in range(5)]
    id_base = 5000
    cand_h = rng.integers(0, 120, (5, 30)).astype(np.int64) + id_base
    cand_h[0, 4] = -1
    index = ShardedTokenIndex.from_encoder(enc, docs, id_base=id_base)
    Dtok, Doff = index.Dtok, index.Doff
    Qtok = enc.encode_queries(queries, batch_size=64)
    plane = ops.maxsim_e4m3(ops.quantize_e4m3(Qtok), ops.quantize_e4m3(Dtok), Doff, max_doc_len=enc.max_doc_length).cpu().numpy()
    index.quantize()
    assert index.N == 120 and index.Dtok is None
    out = Ranker.multi_vector_rerank(queries, index, dev(cand_h), encoder=enc, return_topk=20)
    for q in range(5):
        want_ids, want_sc = host_list(plane[q], cand_h[q], id_base, 120)
        assert int(out.lens[q]) == 20 and out.ids[q].tolist() == want_ids[:20]
        assert np.array_equal(out.scores[q].cpu().numpy().view(np.int32), want_sc[:20].view(np.int32))
