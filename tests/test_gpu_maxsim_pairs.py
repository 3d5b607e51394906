"""Candidate-list MaxSim (csrc/rerank.hip, ops.maxsim_pairs, ShardedTokenIndex, Ranker.multi_vector_rerank) on the GPU.

1. Grid inputs (maxsim_cases.py: nothing to round in fp32): bit equality with the float64 formula gathered at the candidates, poison rows
   before, after and inside the corpus, every absent-slot kind, strided planes with sentinel padding, two id bases.
2. Unit-norm inputs: bit equality with the all-pairs kernel (ops.maxsim gathered at the candidates), twice.
3. Special values (+-inf, inf * 0, inf - inf in the inputs): the all-pairs kernel's bits, compared through the integer view.
4. ShardedTokenIndex.rerank / Ranker.multi_vector_rerank: order, ties, lens and padding, two shards against one, and the lists fused by
   Aggregator.fuse_topk next to a dense system's against the same lists built on the host from the ops.maxsim plane."""
import numpy as np
import pytest
import torch

import maxsim_cases as M
import maxsim_pairs_cases as P

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


def test_branch_table_is_covered():
    hit, by_k, by_m = P.sweep_branches()
    for k, claims in P.K_CLAIMS.items():
        assert set(claims) <= by_k[k], (k, sorted(map(str, set(claims) - by_k[k])))
    for m, claims in P.M_CLAIMS.items():
        assert set(claims) <= by_m[m], (m, sorted(map(str, set(claims) - by_m[m])))
    assert set(P.BRANCHES) <= hit, sorted(map(str, set(P.BRANCHES) - hit))


# ---- 1. grid inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc_len", P.MAX_DOC_LENS)
@pytest.mark.parametrize("Q", P.QS)
@pytest.mark.parametrize("Lq", M.LQS)
def test_grid_candidates_are_exact(ops, Lq, Q, max_doc_len):
    Dtok_h, Doff_h = P.corpus(max_doc_len)
    ref = P.reference(Lq, Q, max_doc_len)
    Qtok, Dtok, Doff = dev(P.queries(Lq, Q)), dev(Dtok_h), dev(Doff_h)
    for k in P.KS:
        for id_base in P.ID_BASES:
            cand_h = P.candidates(Q, k, id_base)
            cand_full = torch.full((Q, k + 3), id_base, dtype=torch.int64, device="cuda")      # ldc = k + 3
            cand_full[:, :k] = dev(cand_h)
            for cl in P.launches(Q, k):
                out_full = torch.full((Q, k + 5), P.SENTINEL, dtype=torch.float32, device="cuda")      # lds = k + 5
                got = ops.maxsim_pairs(Qtok, Dtok, Doff, cand_full[:, :k], None if cl is None else dev(cl), id_base=id_base,
                                       max_doc_len=max_doc_len, out=out_full[:, :k])
                assert got.data_ptr() == out_full.data_ptr()
                exp = P.expected(ref, cand_h, np.full(Q, k) if cl is None else cl, id_base)
                got_h = out_full.cpu().numpy()
                what = (Lq, Q, max_doc_len, k, id_base, None if cl is None else cl.tolist())
                bad = np.argwhere(got_h[:, :k].view(np.int32) != exp.view(np.int32))
                assert len(bad) == 0, (what, len(bad), [(int(q), int(r), int(cand_h[q, r]), float(got_h[q, r]), float(exp[q, r])) for q, r in bad[:8]])
                assert (got_h[:, k:] == P.SENTINEL).all(), (what, "padding columns of the score plane were written")


def test_default_output_plane_and_empty_shapes(ops):
    Dtok_h, Doff_h = P.corpus(512)
    Qtok, Dtok, Doff = dev(P.queries(64, 2)), dev(Dtok_h), dev(Doff_h)
    cand = dev(P.candidates(2, 7, 0))
    got = ops.maxsim_pairs(Qtok, Dtok, Doff, cand, max_doc_len=512)
    assert got.shape == (2, 7) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.int32), P.expected(P.reference(64, 2, 512), cand.cpu().numpy(), [7, 7], 0).view(np.int32))
    assert ops.maxsim_pairs(Qtok, Dtok, Doff, cand[:, :0]).shape == (2, 0)
    assert ops.maxsim_pairs(Qtok[:0], Dtok, Doff, cand[:0]).shape == (0, 7)
    # a shard without documents owns nothing
    none = ops.maxsim_pairs(Qtok, Dtok[:0], Doff[:1] * 0, cand)
    assert torch.isneginf(none).all()


# ---- 2. unit-norm inputs: the all-pairs kernel's bits ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unit():
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 121, 2000)
    Dtok, Doff = M.unit_corpus(rng, lens, pre=3, post=9)
    pos = rng.integers(0, 2000, (64, 1000)).astype(np.int64)
    return dev(Dtok), dev(Doff), dev(pos), {Lq: dev(M.unit_queries(np.random.default_rng(Lq), 64, Lq)) for Lq in M.LQS}


@pytest.mark.parametrize("Lq", M.LQS)
def test_unit_norm_bits_equal_the_all_pairs_kernel(ops, unit, Lq):
    Dtok, Doff, pos, Qs = unit
    plane = ops.maxsim(Qs[Lq], Dtok, Doff, max_doc_len=120)
    want = bits(torch.gather(plane, 1, pos))
    for id_base in (0, 2 ** 40):
        a = ops.maxsim_pairs(Qs[Lq], Dtok, Doff, pos + id_base, id_base=id_base, max_doc_len=120)
        b = ops.maxsim_pairs(Qs[Lq], Dtok, Doff, pos + id_base, id_base=id_base, max_doc_len=120)
        assert torch.equal(bits(a), want), (Lq, id_base, int((bits(a) != want).sum()))
        assert torch.equal(bits(a), bits(b)), "two calls differ"
    assert torch.isfinite(plane).all() and float(plane.abs().max()) > 1.0     # not a comparison of zeros
    # truncation: the same with max_doc_len = 40
    plane40 = ops.maxsim(Qs[Lq], Dtok, Doff, max_doc_len=40)
    assert torch.equal(bits(ops.maxsim_pairs(Qs[Lq], Dtok, Doff, pos, max_doc_len=40)), bits(torch.gather(plane40, 1, pos)))


# ---- 3. special values ---------------------------------------------------------------------------------------------------------------
def test_special_values_carry_the_all_pairs_bits(ops):
    Qtok, Dtok, Doff = (dev(x) for x in M.special_inputs())
    plane = ops.maxsim(Qtok, Dtok, Doff, max_doc_len=512)
    # the all-pairs kernel's own special values (tests/test_gpu_maxsim_edges.py::test_special_values): its fmaxf drops a NaN term, so the
    # plane holds +inf (an inf row met by positive components) and -inf (every term of a document NaN), and no NaN of its own;
    # whatever it holds, NaN payloads included, is compared through the integer view
    assert torch.isposinf(plane).any() and torch.isneginf(plane[:, 3]).all()
    N = Doff.numel() - 1
    pos = torch.arange(N, device="cuda").repeat(4, 3)[:, torch.randperm(3 * N, generator=torch.Generator().manual_seed(1)).cuda()]
    got = ops.maxsim_pairs(Qtok, Dtok, Doff, pos, max_doc_len=512)
    assert torch.equal(bits(got), bits(torch.gather(plane, 1, pos)))


# ---- 4. the index and the ranker ---------------------------------------------------------------------------------------------------
def host_list(plane_rows, cand_row, id_base, N):
    """One query's reranked list built on the host from its row of the ops.maxsim plane: owned candidates in stable descending order."""
    owned = [(float(plane_rows[c - id_base]), r, int(c)) for r, c in enumerate(cand_row) if c >= 0 and 0 <= c - id_base < N]
    owned.sort(key=lambda t: -t[0])      # stable: ties keep candidate order
    return [c for _, _, c in owned], np.array([s for s, _, _ in owned], dtype=np.float32)


@pytest.fixture(scope="module")
def tied():
    """A unit-norm corpus in which documents 10..14 share their token rows with document 3 (equal scores for every query), 200 documents."""
    rng = np.random.default_rng(11)
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
    return Qtok, Dtok, Doff, cand, id_base


def test_rerank_lists(ops, tied):
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.planes import RankedTopk
    Qtok_h, Dtok_h, Doff_h, cand_h, id_base = tied
    Qtok, Dtok, Doff, cand = dev(Qtok_h), dev(Dtok_h), dev(Doff_h), dev(cand_h)
    N = len(Doff_h) - 1
    plane = ops.maxsim(Qtok, Dtok, Doff, max_doc_len=512).cpu().numpy()
    index = ShardedTokenIndex(Dtok, Doff, id_base)
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
        tied_at = [i for i, c in enumerate(ids[q, :n]) if c in (1003, 1010, 1011, 1012, 1013, 1014)]      # one run of equal scores ...
        assert len(tied_at) >= 5 and tied_at == list(range(tied_at[0], tied_at[0] + len(tied_at))) and len(set(sc[q, tied_at].tolist())) == 1
        assert ids[q, tied_at].tolist() == [c for c in cand_h[q].tolist() if c in (1003, 1010, 1011, 1012, 1013, 1014)]      # ... in candidate order
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
    Qtok_h, Dtok_h, Doff_h, cand_h, id_base = tied
    Qtok, cand = dev(Qtok_h), dev(cand_h)
    whole = ShardedTokenIndex(dev(Dtok_h), dev(Doff_h), id_base).local_scores(Qtok, cand)
    cutd = 77
    t = int(Doff_h[cutd])
    lo = ShardedTokenIndex(dev(Dtok_h[:t]), dev(Doff_h[:cutd + 1]), id_base)
    hi = ShardedTokenIndex(dev(Dtok_h[t:]), dev(Doff_h[cutd:] - t), id_base + cutd)
    a, b = lo.local_scores(Qtok, cand), hi.local_scores(Qtok, cand)
    assert not (torch.isfinite(a) & torch.isfinite(b)).any()      # no slot is owned twice
    assert torch.equal(bits(torch.maximum(a, b)), bits(whole))


@pytest.mark.parametrize("method,norm", [("rrf", None), ("nsf", "min-max")])
def test_reranked_lists_fuse_like_host_built_ones(ops, tied, method, norm):
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    Qtok_h, Dtok_h, Doff_h, _, id_base = tied
    Qtok, Dtok, Doff = dev(Qtok_h), dev(Dtok_h), dev(Doff_h)
    N = len(Doff_h) - 1
    rng = np.random.default_rng(3)
    # a dense system's lists over the same shard (distinct ids per list, the last one shorter); ColBERT reranks exactly these candidates
    cand_h = np.stack([rng.permutation(N)[:50] for _ in range(6)]).astype(np.int64) + id_base
    cand_h[:, :5] = (1012, 1003, 1010, 1014, 1011)      # tied for ColBERT
    for q in range(6):
        rest = [c for c in rng.permutation(N) + id_base if c not in (1012, 1003, 1010, 1014, 1011)]
        cand_h[q, 5:] = rest[:45]
    cand_h[5, 44:] = -1
    dense = RankedTopk.from_search(dev(np.where(cand_h >= 0, -np.sort(-rng.random((6, 50)).astype(np.float32), axis=1), -np.inf).astype(np.float32)),
                                   dev(cand_h))
    colbert = ShardedTokenIndex(Dtok, Doff, id_base).rerank(Qtok, dense)
    assert colbert.lens.tolist() == [50, 50, 50, 50, 50, 44]
    plane = ops.maxsim(Qtok, Dtok, Doff, max_doc_len=512).cpu().numpy()
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


def test_ranker_rerank_equals_the_plane_of_multi_vector_search(ops):
    from fusion_amd import encoders
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.retrievers.hybrid import Ranker
    enc = encoders.random_init("colbert", size="tiny")
    rng = np.random.default_rng(21)
    words = [f"w{i}" for i in range(300)]
    docs = [" ".join(rng.choice(words, size=int(rng.integers(3, 40)))) for _ in range(120)]
    queries = [" ".join(rng.choice(words, size=int(rng.integers(2, 9)))) for _ in range(5)]
    id_base = 5000
    corpus = {id_base + i: d for i, d in enumerate(docs)}
    rs = Ranker.multi_vector_search(queries, corpus, "colbert", encoder=enc, as_device=True)      # the [Q, N] plane route
    plane = rs.scores.cpu().numpy()
    cand_h = rng.integers(0, 120, (5, 30)).astype(np.int64) + id_base
    cand_h[0, 4] = -1
    index = ShardedTokenIndex.from_encoder(enc, docs, id_base=id_base)
    assert index.N == 120 and index.max_doc_len == enc.max_doc_length
    out = Ranker.multi_vector_rerank(queries, index, dev(cand_h), encoder=enc, return_topk=20)
    for q in range(5):
        want_ids, want_sc = host_list(plane[q], cand_h[q], id_base, 120)
        assert int(out.lens[q]) == 20 and out.ids[q].tolist() == want_ids[:20]
        assert np.array_equal(out.scores[q].cpu().numpy().view(np.int32), want_sc[:20].view(np.int32))
