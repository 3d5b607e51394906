"""The residual-compressed ColBERT token index on the GPU (csrc/rerank_residual.hip; ops.residual_buckets / residual_compress /
residual_decompress / maxsim_pairs_residual; ShardedTokenIndex.compress / build_compressed).

1. Compress and decompress: the bytes and the float16 bits of the numpy restatement (residual_cases.py), on grid rows whose residuals
   sit exactly on the cutoffs and on unit-norm rows where C + w is not representable; a decompressed row range; stored codes outside
   the table are clamped into it.
2. The rerank kernel on the grid corpus built from random codes and buckets: bit equality with the float64 formula over the restated
   decompression, gathered at maxsim_pairs_cases' candidates, poison everywhere a leak could come from, sentinel padding.
3. Unit-norm rows: the kernel's plane equals ops.maxsim_pairs over residual_decompress's output, as int32 views.
4. ShardedTokenIndex: compress then rerank / search give the lists of an uncompressed index over the decompressed matrix;
   build_compressed from three blocks is compress of the whole; memory_bytes; the lists fused next to a dense system's.
5. Reconstruction error falls from the centroid alone to 2 bits to 4 bits.
6. Two runs of every entry give the same bytes."""
import numpy as np
import pytest
import torch

import maxsim_cases as M
import maxsim_pairs_cases as P
import residual_cases as R

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


def h16(t):
    return t.cpu().numpy().view(np.uint16)


# ---- 1. compress / decompress ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", R.NBITS)
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1000))
def test_compress_and_decompress_bits(ops, n, nbits):
    rng = np.random.default_rng(100 * n + nbits)
    # unit-norm rows, buckets trained on their own residuals: the half add rounds
    tok, Cn, codes = R.unit_index(rng, n)
    if n:
        cutoffs, weights = R.train_buckets(tok.astype(np.float32) - Cn[codes].astype(np.float32), nbits)
    else:
        cutoffs, weights = R.grid_buckets(nbits)
    want_p = R.compress(tok, codes, Cn, cutoffs, nbits)
    want_d = R.decompress(want_p, codes, Cn, weights, nbits)
    got_p = ops.residual_compress(dev(tok), dev(codes), dev(Cn), dev(cutoffs), nbits)
    assert got_p.shape == (n, 16 * nbits) and got_p.dtype == torch.uint8
    assert np.array_equal(got_p.cpu().numpy(), want_p)
    got_d = ops.residual_decompress(got_p, dev(codes), dev(Cn), dev(weights))
    assert got_d.shape == (n, 128) and got_d.dtype == torch.float16
    assert np.array_equal(h16(got_d), want_d.view(np.uint16))
    if n:
        assert (want_d != Cn[codes]).mean() > 0.5                                               # the weights moved the rows ...
        assert (want_d.astype(np.float64) != Cn[codes].astype(np.float64) + weights[R.unpack(want_p, nbits)].astype(np.float64)).any() or n == 1   # ... and the sum rounded
    # a row range: the same rows, starting at row_lo
    for lo, hi in ((0, 0), (n // 3, n - n // 4), (n, n), (max(n - 1, 0), n)):
        part = ops.residual_decompress(got_p, dev(codes), dev(Cn), dev(weights), lo, hi)
        assert part.shape == (hi - lo, 128) and np.array_equal(h16(part), want_d[lo:hi].view(np.uint16)), (lo, hi)
    # grid rows with every residual exactly on a cutoff: the lower bucket
    if n:
        gc, gw = R.grid_buckets(nbits)
        G = R.grid_centroids()
        gcodes = (np.arange(n) % R.K_CLEAN).astype(np.int32)
        which = (np.arange(128)[None, :] + np.arange(n)[:, None]) % len(gc)
        on_cut = (G[gcodes].astype(np.float32) + gc[which]).astype(np.float16)
        p = ops.residual_compress(dev(on_cut), dev(gcodes), dev(G), dev(gc), nbits)
        assert np.array_equal(R.unpack(p.cpu().numpy(), nbits), which)
        assert np.array_equal(p.cpu().numpy(), R.compress(on_cut, gcodes, G, gc, nbits))
        d = ops.residual_decompress(p, dev(gcodes), dev(G), dev(gw))
        assert np.array_equal(h16(d), R.decompress(p.cpu().numpy(), gcodes, G, gw, nbits).view(np.uint16))


@pytest.mark.parametrize("nbits", R.NBITS)
def test_stored_codes_outside_the_table_are_clamped(ops, nbits):
    """The kernels clamp a stored code into [0, K - 1]: the result is that of the clamped code, whatever the bytes say."""
    rng = np.random.default_rng(nbits)
    tok, Cn, codes = R.unit_index(rng, 200, Kc=40)
    wild = codes.copy()
    wild[::3] = -1
    wild[1::3] = 40
    wild[2::7] = 45
    clipped = np.clip(wild, 0, 39).astype(np.int32)
    cutoffs, weights = R.grid_buckets(nbits)
    p = ops.residual_compress(dev(tok), dev(wild), dev(Cn), dev(cutoffs), nbits)
    assert np.array_equal(p.cpu().numpy(), R.compress(tok, clipped, Cn, cutoffs, nbits))
    d = ops.residual_decompress(p, dev(wild), dev(Cn), dev(weights))
    assert np.array_equal(h16(d), R.decompress(p.cpu().numpy(), clipped, Cn, weights, nbits).view(np.uint16))
    Doff = dev(np.arange(0, 201, 8, dtype=np.int64))
    Qtok = dev(M.unit_queries(rng, 3, 32))
    cand = dev(rng.integers(0, 25, (3, 20)).astype(np.int64))
    a = ops.maxsim_pairs_residual(Qtok, p, dev(wild), dev(Cn), dev(weights), Doff, cand)
    b = ops.maxsim_pairs_residual(Qtok, p, dev(clipped), dev(Cn), dev(weights), Doff, cand)
    assert torch.equal(bits(a), bits(b)) and torch.isfinite(a).all()


def test_trained_buckets_follow_the_restatement(ops):
    rng = np.random.default_rng(8)
    tok, Cn, codes = R.unit_index(rng, 3000)
    res = tok.astype(np.float32) - Cn[codes].astype(np.float32)
    got = {}
    for nbits in R.NBITS:
        cutoffs, weights = ops.residual_buckets(dev(tok), dev(Cn), dev(codes), nbits)      # 3,000 rows: the sample is every row
        assert cutoffs.dtype == torch.float32 and weights.dtype == torch.float16 and cutoffs.shape == ((1 << nbits) - 1,) and weights.shape == (1 << nbits,)
        wc, ww = R.train_buckets(res, nbits)
        assert np.array_equal(cutoffs.cpu().numpy().view(np.int32), wc.view(np.int32))
        # the float64 means are summed in another order on the device: equal before the rounding to float16 up to 1e-12, so the float16
        # values agree or are neighbours
        step = np.abs(h16(weights).astype(np.int32) - ww.view(np.uint16).astype(np.int32))
        assert step.max() <= 1, (nbits, weights.tolist(), ww.tolist())
        got[nbits] = cutoffs.cpu().numpy()
        sub, _ = ops.residual_buckets(dev(tok), dev(Cn), dev(codes), nbits, sample=500, seed=3)
        sub2, _ = ops.residual_buckets(dev(tok), dev(Cn), dev(codes), nbits, sample=500, seed=3)
        assert torch.equal(sub, sub2) and not torch.equal(sub, cutoffs)                       # a seeded sample
    assert np.array_equal(got[4][3::4], got[2])                                                # nested cutoffs


# ---- 2. the grid corpus: the float64 formula -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc_len", P.MAX_DOC_LENS)
@pytest.mark.parametrize("nbits", R.NBITS)
@pytest.mark.parametrize("Lq", M.LQS)
def test_grid_candidates_are_exact(ops, Lq, nbits, max_doc_len):
    packed_h, codes_h, Doff_h, _ = R.grid_corpus(nbits, max_doc_len)
    assert tuple(np.diff(Doff_h)) == P.LENS and Doff_h[0] == P.PRE and len(codes_h) == Doff_h[-1] + P.POST
    _, weights_h = R.grid_buckets(nbits)
    packed, codes, Doff, Cd, weights = dev(packed_h), dev(codes_h), dev(Doff_h), dev(R.grid_centroids()), dev(weights_h)
    for Q in R.QS:
        ref = R.grid_reference(Lq, Q, nbits, max_doc_len)
        Qtok = dev(P.queries(Lq, Q))
        for k in R.KS:
            for id_base in P.ID_BASES:
                cand_h = P.candidates(Q, k, id_base)
                cand_full = torch.full((Q, k + 3), id_base, dtype=torch.int64, device="cuda")      # ldc = k + 3
                cand_full[:, :k] = dev(cand_h)
                for cl in P.launches(Q, k):
                    out_full = torch.full((Q, k + 5), P.SENTINEL, dtype=torch.float32, device="cuda")      # lds = k + 5
                    got = ops.maxsim_pairs_residual(Qtok, packed, codes, Cd, weights, Doff, cand_full[:, :k], None if cl is None else dev(cl),
                                                    id_base=id_base, max_doc_len=max_doc_len, out=out_full[:, :k])
                    assert got.data_ptr() == out_full.data_ptr()
                    exp = P.expected(ref, cand_h, np.full(Q, k) if cl is None else cl, id_base)
                    got_h = out_full.cpu().numpy()
                    what = (Lq, nbits, Q, max_doc_len, k, id_base, None if cl is None else cl.tolist())
                    bad = np.argwhere(got_h[:, :k].view(np.int32) != exp.view(np.int32))
                    assert len(bad) == 0, (what, len(bad), [(int(q), int(r), int(cand_h[q, r]), float(got_h[q, r]), float(exp[q, r])) for q, r in bad[:8]])
                    assert (got_h[:, k:] == P.SENTINEL).all(), (what, "padding columns of the score plane were written")


def test_grid_reference_is_not_trivial():
    """The premises of the grid test: clean and guard documents both score, a leaked poison row would show, the weights matter."""
    for nbits in R.NBITS:
        packed, codes, Doff, D = R.grid_corpus(nbits, 512)
        ref = R.grid_reference(32, 5, nbits, 512)
        lens = np.asarray(P.LENS)
        clean = (np.arange(len(lens)) % 2 == 0) & (lens > 0)
        guard = ref[:, (np.arange(len(lens)) % 2 == 1) & (lens > 0)]
        assert np.abs(ref[:, clean]).max() < 256 * 32 and (guard % 256 == 0).all() and (np.abs(guard) >= 256).mean() > 0.9
        centre_only = M.maxsim_ref(P.queries(32, 5), R.grid_centroids()[codes], Doff, 512)
        assert (centre_only[:, clean] != ref[:, clean]).mean() > 0.9
        assert len(np.unique(R.unpack(packed[P.PRE: P.PRE + 1], nbits))) > 1


def test_default_output_plane_and_empty_shapes(ops):
    packed_h, codes_h, Doff_h, _ = R.grid_corpus(2, 512)
    _, weights_h = R.grid_buckets(2)
    packed, codes, Doff, Cd, weights = dev(packed_h), dev(codes_h), dev(Doff_h), dev(R.grid_centroids()), dev(weights_h)
    Qtok = dev(P.queries(64, 2))
    cand = dev(P.candidates(2, 7, 0))
    got = ops.maxsim_pairs_residual(Qtok, packed, codes, Cd, weights, Doff, cand, max_doc_len=512)
    assert got.shape == (2, 7) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.int32), P.expected(R.grid_reference(64, 2, 2, 512), cand.cpu().numpy(), [7, 7], 0).view(np.int32))
    assert ops.maxsim_pairs_residual(Qtok, packed, codes, Cd, weights, Doff, cand[:, :0]).shape == (2, 0)
    assert ops.maxsim_pairs_residual(Qtok[:0], packed, codes, Cd, weights, Doff, cand[:0]).shape == (0, 7)
    none = ops.maxsim_pairs_residual(Qtok, packed[:0], codes[:0], Cd, weights, Doff[:1] * 0, cand)      # a shard without documents owns nothing
    assert torch.isneginf(none).all()
    for bad in (dict(packed=packed[:, :31]), dict(weights=weights[:3]), dict(codes=codes[:-1]), dict(C=Cd[:, :64]), dict(cand=cand[:1])):
        args = dict(packed=packed, codes=codes, C=Cd, weights=weights, cand=cand)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.maxsim_pairs_residual(Qtok, args["packed"], args["codes"], args["C"], args["weights"], Doff, args["cand"])
    for bad in (dict(packed=packed.int()), dict(weights=weights.float()), dict(codes=codes.long()), dict(C=Cd.float())):
        args = dict(packed=packed, codes=codes, C=Cd, weights=weights)
        args.update(bad)
        with pytest.raises(TypeError):
            ops.maxsim_pairs_residual(Qtok, args["packed"], args["codes"], args["C"], args["weights"], Doff, cand)


# ---- 3. unit-norm rows: the uncompressed kernel over the decompressed matrix ---------------------------------------------------------
@pytest.fixture(scope="module")
def unit(ops):
    rng = np.random.default_rng(78)
    lens = rng.integers(0, 121, 1000)
    Dtok_h, Doff_h = M.unit_corpus(rng, lens, pre=3, post=9)
    Cn = rng.normal(0, 1, (R.K, 128))
    Cn = dev((Cn / np.linalg.norm(Cn, axis=1, keepdims=True)).astype(np.float16))
    Dtok, Doff = dev(Dtok_h), dev(Doff_h)
    codes = ops.centroid_assign(Dtok, Cn)
    pos = dev(rng.integers(0, 1000, (16, 300)).astype(np.int64))
    per = {}
    for nbits in R.NBITS:
        cutoffs, weights = ops.residual_buckets(Dtok, Cn, codes, nbits)
        packed = ops.residual_compress(Dtok, codes, Cn, cutoffs, nbits)
        per[nbits] = (packed, weights, ops.residual_decompress(packed, codes, Cn, weights))
    return Doff, Cn, codes, pos, per, {Lq: dev(M.unit_queries(np.random.default_rng(Lq), 16, Lq)) for Lq in M.LQS}, Dtok


@pytest.mark.parametrize("nbits", R.NBITS)
@pytest.mark.parametrize("Lq", M.LQS)
def test_unit_norm_plane_equals_the_uncompressed_kernel_over_the_decompressed_rows(ops, unit, Lq, nbits):
    Doff, Cn, codes, pos, per, Qs, Dtok = unit
    packed, weights, D = per[nbits]
    for id_base, m in ((0, 120), (2 ** 40, 120), (0, 40)):
        want = ops.maxsim_pairs(Qs[Lq], D, Doff, pos + id_base, id_base=id_base, max_doc_len=m)
        a = ops.maxsim_pairs_residual(Qs[Lq], packed, codes, Cn, weights, Doff, pos + id_base, id_base=id_base, max_doc_len=m)
        b = ops.maxsim_pairs_residual(Qs[Lq], packed, codes, Cn, weights, Doff, pos + id_base, id_base=id_base, max_doc_len=m)
        assert torch.equal(bits(a), bits(want)), (Lq, nbits, id_base, m, int((bits(a) != bits(want)).sum()))
        assert torch.equal(bits(a), bits(b)), "two calls differ"
    assert torch.isfinite(want).all() and float(want.abs().max()) > 1.0                      # not a comparison of zeros
    exact = ops.maxsim_pairs(Qs[Lq], Dtok, Doff, pos, max_doc_len=40)
    assert not torch.equal(bits(exact), bits(want))                                             # the code is lossy: D is not Dtok


# ---- 4. the index --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shard(ops):
    """About 2,000 clustered documents, K = 256 centroids (the cluster centres), id_base 5000."""
    rng = np.random.default_rng(31)
    lens = rng.integers(1, 50, 2000)
    lens[7] = 0
    tok, centres = R.clustered_tokens(rng, int(lens.sum()), 256, 0.04)
    Doff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Qtok, _ = R.clustered_tokens(rng, 6 * 32, 256, 0.04)
    return dev(tok), dev(Doff), dev(centres), dev(Qtok.reshape(6, 32, 128)), 5000, rng.integers(0, 2000, (6, 200)).astype(np.int64) + 5000


def same_lists(a, b):
    return torch.equal(a.ids, b.ids) and torch.equal(bits(a.scores), bits(b.scores)) and torch.equal(a.lens, b.lens)


@pytest.mark.parametrize("nbits", R.NBITS)
def test_compressed_index_gives_the_lists_of_the_decompressed_matrix(ops, shard, nbits):
    from fusion_amd.distributed import ShardedTokenIndex
    tok, Doff, Cd, Qtok, id_base, cand_h = shard
    sumL = tok.shape[0]
    index = ShardedTokenIndex(tok, Doff, id_base).build_centroids(Cd)
    assert index.codes.dtype == torch.int32 and index.codes.shape == (sumL,)
    plain_bytes = index.memory_bytes()
    assert plain_bytes["tokens"] == 256 * sumL and plain_bytes["codes"] == 4 * sumL and plain_bytes["packed"] == 0
    assert index.compress(nbits) is index
    assert index.Dtok is None and index.nbits == nbits and index.packed.shape == (sumL, 16 * nbits) and index.N == 2000
    mb = index.memory_bytes()
    ix = index.candidates.index
    cand_bytes = ix.coff.numel() * 8 + ix.cdoc.numel() * 4 + (0 if ix.slice_off is None else ix.slice_off.numel() * 8)
    assert mb == dict(tokens=0, codes=4 * sumL, packed=16 * nbits * sumL, candidates=cand_bytes, total=(4 + 16 * nbits) * sumL + cand_bytes)
    assert mb["codes"] + mb["packed"] == (36 if nbits == 2 else 68) * sumL
    # the uncompressed index over the decompressed matrix, same codes: the same lists
    D = index.decompressed()
    assert torch.equal(D[100:300], index.decompressed(100, 300))
    ref = ShardedTokenIndex(D, Doff, id_base).build_centroids(Cd, codes=index.codes)
    cand = dev(cand_h)
    cand[1, 9], cand[1, 199], cand[2, 11], cand[2, 12] = -1, -1, id_base - 1, id_base + 2000
    assert torch.equal(bits(index.local_scores(Qtok, cand)), bits(ref.local_scores(Qtok, cand)))
    got, want = index.rerank(Qtok, cand), ref.rerank(Qtok, cand)
    assert same_lists(got, want) and got.lens.tolist() == [200, 198, 198, 200, 200, 200]
    assert same_lists(index.rerank(Qtok, cand, k=10), ref.rerank(Qtok, cand, k=10))
    for k, ncand in ((10, None), (100, 300)):
        got, want = index.search(Qtok, k=k, nprobe=256, ncand=ncand), ref.search(Qtok, k=k, nprobe=256, ncand=ncand)
        assert same_lists(got, want) and int(got.lens.min()) == k
    # already compressed: nothing left to compress
    with pytest.raises(ValueError, match="already compressed"):
        index.compress(nbits)
    # given buckets, kept tokens
    kept = ShardedTokenIndex(tok, Doff, id_base).build_centroids(Cd, codes=index.codes).compress(nbits, index.cutoffs, index.weights, keep_tokens=True)
    assert kept.Dtok is tok and torch.equal(kept.packed, index.packed) and kept.memory_bytes()["tokens"] == 256 * sumL
    with pytest.raises(ValueError, match="both"):
        ShardedTokenIndex(tok, Doff, id_base).build_centroids(Cd, codes=index.codes).compress(nbits, cutoffs=index.cutoffs)
    # the code range is validated once, when the index is built
    tampered = ShardedTokenIndex(tok, Doff, id_base).build_centroids(Cd, codes=index.codes)
    tampered.codes = index.codes + 1000
    with pytest.raises(ValueError, match="codes must lie"):
        tampered.compress(nbits)


@pytest.mark.parametrize("nbits", R.NBITS)
def test_build_compressed_from_blocks_equals_compress_of_the_whole(ops, shard, nbits):
    from fusion_amd.distributed import ShardedTokenIndex
    tok, Doff, Cd, Qtok, id_base, cand_h = shard
    whole = ShardedTokenIndex(tok, Doff, id_base).build_centroids(Cd).compress(nbits)
    sumL = tok.shape[0]
    cuts = (0, 1000, sumL // 2 + 7, sumL)
    blocks = (tok[a:b].cpu() if i == 1 else tok[a:b] for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])))      # host and device blocks
    built = ShardedTokenIndex.build_compressed(blocks, Doff, Cd, whole.cutoffs, whole.weights, nbits, id_base)
    assert built.Dtok is None and built.N == 2000 and built.nbits == nbits
    assert torch.equal(built.codes, whole.codes) and torch.equal(built.packed, whole.packed)
    assert torch.equal(built.candidates.index.coff, whole.candidates.index.coff) and torch.equal(built.candidates.index.cdoc, whole.candidates.index.cdoc)
    assert built.memory_bytes() == whole.memory_bytes()
    assert same_lists(built.search(Qtok, k=20, nprobe=256), whole.search(Qtok, k=20, nprobe=256))
    assert same_lists(built.rerank(Qtok, dev(cand_h)), whole.rerank(Qtok, dev(cand_h)))
    with pytest.raises(ValueError, match="token rows"):
        ShardedTokenIndex.build_compressed(iter([tok[:1000]]), Doff, Cd, whole.cutoffs, whole.weights, nbits, id_base)
    with pytest.raises(ValueError, match="token rows"):
        ShardedTokenIndex.build_compressed(iter([tok, tok[:1]]), Doff, Cd, whole.cutoffs, whole.weights, nbits, id_base)


def test_two_compressed_shards_give_the_bits_of_one(ops, shard):
    from fusion_amd.distributed import ShardedTokenIndex
    tok, Doff, Cd, Qtok, id_base, cand_h = shard
    cand = dev(cand_h)
    whole = ShardedTokenIndex(tok, Doff, id_base).build_centroids(Cd).compress(4)
    cutd = 777
    t = int(Doff[cutd])
    lo = ShardedTokenIndex(tok[:t], Doff[:cutd + 1], id_base).build_centroids(Cd).compress(4, whole.cutoffs, whole.weights)
    hi = ShardedTokenIndex(tok[t:], Doff[cutd:] - t, id_base + cutd).build_centroids(Cd).compress(4, whole.cutoffs, whole.weights)
    a, b = lo.local_scores(Qtok, cand), hi.local_scores(Qtok, cand)
    assert not (torch.isfinite(a) & torch.isfinite(b)).any()      # no slot is owned twice
    assert torch.equal(bits(torch.maximum(a, b)), bits(whole.local_scores(Qtok, cand)))


@pytest.mark.parametrize("method,norm", [("rrf", None), ("nsf", "min-max")])
def test_compressed_lists_fuse_next_to_a_dense_system(ops, shard, method, norm):
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    tok, Doff, Cd, Qtok, id_base, _ = shard
    rng = np.random.default_rng(3)
    cand_h = np.stack([rng.permutation(2000)[:50] for _ in range(6)]).astype(np.int64) + id_base
    cand_h[5, 44:] = -1
    dense = RankedTopk.from_search(dev(np.where(cand_h >= 0, -np.sort(-rng.random((6, 50)).astype(np.float32), axis=1), -np.inf).astype(np.float32)),
                                   dev(cand_h))
    index = ShardedTokenIndex(tok, Doff, id_base).build_centroids(Cd).compress(2)
    ref = ShardedTokenIndex(index.decompressed(), Doff, id_base)
    colbert, host = index.rerank(Qtok, dense), ref.rerank(Qtok, dense)
    assert colbert.lens.tolist() == [50, 50, 50, 50, 50, 44] and same_lists(colbert, host)
    w = {"dpr": 0.4, "colbert": 0.6}
    got = Aggregator.fuse_topk({"dpr": dense, "colbert": colbert}, method, norm, w, {})
    want = Aggregator.fuse_topk({"dpr": dense, "colbert": host}, method, norm, w, {})
    assert torch.equal(got.lens, want.lens) and torch.equal(got.ids, want.ids) and int(got.lens.min()) >= 44
    view = torch.int64 if got.scores.dtype == torch.float64 else torch.int32
    assert torch.equal(got.scores.view(view), want.scores.view(view))


# ---- 5. reconstruction -------------------------------------------------------------------------------------------------------------
def test_reconstruction_error_falls_with_the_width(ops):
    """Nested equal-population cuts with bucket means: splitting a bucket at a cut and giving both halves their own mean cannot raise
    the squared error of the training rows, and on noise of any spread it lowers it; the centroid alone is the one-bucket code with
    weight 0 (no numeric threshold: a CPU restatement at these sizes gave ratios of about 6 and 7)."""
    rng = np.random.default_rng(64)
    tok_h, centres = R.clustered_tokens(rng, 20000, 64, 0.04)
    tok, Cd = dev(tok_h), dev(centres)
    codes = ops.centroid_assign(tok, Cd)
    x = tok.double()
    mse = {0: float(((x - Cd[codes.long()].double()) ** 2).mean())}
    for nbits in R.NBITS:
        cutoffs, weights = ops.residual_buckets(tok, Cd, codes, nbits, sample=20000)      # trained on all of its rows
        D = ops.residual_decompress(ops.residual_compress(tok, codes, Cd, cutoffs, nbits), codes, Cd, weights)
        mse[nbits] = float(((x - D.double()) ** 2).mean())
    print("reconstruction MSE:", mse, "ratios:", mse[0] / mse[2], mse[2] / mse[4])
    assert mse[4] < mse[2] < mse[0], mse


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", R.NBITS)
def test_two_runs_give_the_same_bytes(ops, unit, nbits):
    Doff, Cn, codes, pos, per, Qs, Dtok = unit
    runs = []
    for _ in range(2):
        cutoffs, weights = ops.residual_buckets(Dtok, Cn, codes, nbits)
        packed = ops.residual_compress(Dtok, codes, Cn, cutoffs, nbits)
        D = ops.residual_decompress(packed, codes, Cn, weights)
        s = ops.maxsim_pairs_residual(Qs[64], packed, codes, Cn, weights, Doff, pos, max_doc_len=120)
        runs.append((cutoffs, weights.view(torch.int16), packed, D.view(torch.int16), bits(s)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][2], per[nbits][0])
