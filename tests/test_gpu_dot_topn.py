"""dot_topn on the GPU: the top-n selection in the epilogue of the float32 MFMA GEMM returns, bit for bit, what the two kernels
topk_rows(dot_scores(X, C), n) return -- the same chain of fused multiply-adds per score, the same (score desc, id asc) order.

1. random float32 data over every tail class of rows, strip / tile / padding edge of K, n of 1 .. 8 and ragged / single k-tiles of d;
2. ties go to the lowest id at every lane, lane half, wave and tile position -- against numpy on exact grid data, no other kernel involved;
3. long walks (K past 65,536) with one token tile, where the centroid blocks are cut into groups and the merge carries the result;
4. the row chunking of the public functions;  5. centroid_probes / centroid_assign / kmeans_centroids by both routes;
6. ShardedTokenIndex.search end to end by both routes;  7. run to run.
Every comparison is exact equality (scores as int32 bit patterns)."""
import numpy as np
import pytest
import torch

import centroid_cases as CC
import maxsim_cases as M

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


_rand = {}


def rand(rows, d, seed):
    """Fixed-seed float32 rows, made once per shape."""
    key = (rows, d, seed)
    if key not in _rand:
        _rand[key] = dev(np.random.default_rng(seed).normal(0, 1, (rows, d)).astype(np.float32))
    return _rand[key]


def two_kernels(ops, X, C, n):
    s, i = ops.topk_rows(ops.dot_scores(X, C), n)
    return s, i.to(torch.int32)


def same(got, want):
    (gs, gi), (ws, wi) = got, want
    assert gs.dtype == torch.float32 and gi.dtype == torch.int32 and tuple(gs.shape) == tuple(gi.shape) == tuple(ws.shape)
    assert torch.equal(gi, wi)
    assert torch.equal(bits(gs), bits(ws))


# ---- 1. the same bits as the two-kernel route ------------------------------------------------------------------------------------------
ROWS = [1, 33, 64, 67, 97, 128, 129, 195, 257]
KS = [1, 3, 63, 64, 65, 128, 129, 1000, 1031]
NS = [1, 2, 4, 5, 8]
# every rows with five K's, every K with five rows, every n nine times: a 9 x 9 cyclic design, 45 of the 405 combinations
COVER = [(ROWS[a], KS[(a + 2 * b) % 9], NS[(a + b) % 5]) for a in range(9) for b in range(5)]


def test_the_cover_holds_every_value_of_every_axis():
    assert len(set(COVER)) == 45
    assert {c[0] for c in COVER} == set(ROWS) and {c[1] for c in COVER} == set(KS) and {c[2] for c in COVER} == set(NS)
    assert any(n > K for _, K, n in COVER) and any(r == 257 and K >= 1000 for r, K, _ in COVER)


@pytest.mark.parametrize("rows,K,n", COVER)
def test_same_bits_as_dot_scores_then_topk_rows(ops, rows, K, n):
    X, C = rand(rows, 128, 1), rand(K, 128, 2)
    got = ops.dot_topn(X, C, n)
    same(got, two_kernels(ops, X, C, n))
    if n > K:
        assert (got[1][:, K:] == -1).all() and torch.isneginf(got[0][:, K:]).all() and (got[1][:, :K] >= 0).all()


@pytest.mark.parametrize("d", [4, 36, 64, 100, 768])
def test_ragged_and_single_k_tiles(ops, d):
    X, C = rand(129, d, 3), rand(257, d, 4)
    same(ops.dot_topn(X, C, 4), two_kernels(ops, X, C, 4))


# ---- 2. ties -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_rows():
    rng = np.random.default_rng(21)
    return M.grid_queries(rng, 130, 1).reshape(130, 128).astype(np.float32), M.grid_queries(rng, 7, 1).reshape(7, 128).astype(np.float32)


@pytest.mark.parametrize("n", [1, 4, 8])
def test_equal_centroids_resolve_to_the_lowest_ids(ops, grid_rows, n):
    X, V = grid_rows
    C = np.repeat(V[:1], 300, axis=0)
    s, i = ops.dot_topn(dev(X), dev(C), n)
    assert torch.equal(i, torch.arange(n, dtype=torch.int32, device="cuda").expand(130, n))
    want = (X.astype(np.float64) @ V[0].astype(np.float64)).astype(np.float32)      # exact on the grid
    assert np.array_equal(s.cpu().numpy(), np.repeat(want[:, None], n, axis=1))


@pytest.mark.parametrize("n", [1, 4, 8])
def test_seven_vectors_with_period_seven_equal_numpy_lexsort(ops, grid_rows, n):
    X, V = grid_rows
    C = V[np.arange(300) % 7]
    S = X.astype(np.float64) @ C.astype(np.float64).T                                # exact on the grid
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
    want_i = np.stack([np.lexsort((np.arange(300), -S[r]))[:n] for r in range(130)])
    s, i = ops.dot_topn(dev(X), dev(C), n)
    assert np.array_equal(i.cpu().numpy(), want_i.astype(np.int32))
    assert np.array_equal(s.cpu().numpy().astype(np.float64), np.take_along_axis(S, want_i, 1))


# ---- 3. long walks and group splits, 7. run to run ------------------------------------------------------------------------------------------
def test_one_token_tile_against_70001_centroids_and_run_to_run(ops):
    X, C = rand(64, 128, 5), rand(70001, 128, 6)
    got = ops.dot_topn(X, C, 4)
    same(got, two_kernels(ops, X, C, 4))
    assert int(got[1].max()) >= 65536                            # the ids past 65,536 are reached
    again = ops.dot_topn(X, C, 4)
    assert torch.equal(again[1], got[1]) and torch.equal(bits(again[0]), bits(got[0]))


def test_five_token_tiles_against_20000_centroids(ops):
    X, C = rand(640, 128, 7), rand(20000, 128, 8)
    same(ops.dot_topn(X, C, 8), two_kernels(ops, X, C, 8))


# ---- 4. row chunking -------------------------------------------------------------------------------------------------------------------------
def test_chunks_that_are_no_multiple_of_128_rows(ops, monkeypatch):
    rng = np.random.default_rng(9)
    Qtok = dev(rng.normal(0, 1, (3, 100, 128)).astype(np.float16))                  # 300 token rows
    C = dev(rng.normal(0, 1, (500, 128)).astype(np.float16))
    whole = ops.centroid_probes(Qtok, C, 4, fused=True)
    codes = ops.centroid_assign(Qtok.view(300, 128), C, fused=True)
    monkeypatch.setattr(ops, "CENTROID_BLOCK_BYTES", 77 * (4 * 128 + 32 * 4))       # 77 rows per block at n = 4: 77, 77, 77, 69
    assert ops._topn_block_rows(128, 4) == 77 and ops._topn_block_rows(128, 1) not in (128, 256)
    pc, ps = ops.centroid_probes(Qtok, C, 4, fused=True)
    assert torch.equal(pc, whole[0]) and torch.equal(bits(ps), bits(whole[1]))
    assert torch.equal(ops.centroid_assign(Qtok.view(300, 128), C, fused=True), codes)
    assert torch.equal(codes, whole[0].view(300, 4)[:, 0])


# ---- 5. the public functions by both routes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 3])
@pytest.mark.parametrize("p", [1, 2, 5])
def test_centroid_probes_by_both_routes(ops, K, p):
    rng = np.random.default_rng(12)
    Qtok = dev(M.grid_queries(rng, 3, 32))
    C = dev(CC.sign_centroids(rng, 64)[:K])
    pc, ps = ops.centroid_probes(Qtok, C, p, fused=True)
    pc0, ps0 = ops.centroid_probes(Qtok, C, p, fused=False)
    assert tuple(pc.shape) == tuple(ps.shape) == (3, 32 * p) and pc.dtype == torch.int32 and ps.dtype == torch.float32
    assert torch.equal(pc, pc0) and torch.equal(bits(ps), bits(ps0))
    if p > K:
        assert (pc.view(96, p)[:, K:] == -1).all() and torch.isneginf(ps.view(96, p)[:, K:]).all()
    with pytest.raises(ValueError):
        ops.centroid_probes(Qtok, C, ops.dot_topn_max() + 1, fused=True)
    big = ops.centroid_probes(Qtok, C, ops.dot_topn_max() + 1)                      # fused=None above the cap: the two kernels, silently
    assert tuple(big[0].shape) == (3, 32 * (ops.dot_topn_max() + 1))


@pytest.fixture(scope="module")
def clustered():
    rng = np.random.default_rng(6)
    centres = rng.normal(0, 1, (96, 128))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    lens = rng.integers(1, 41, 3000)
    Doff = CC.doc_offsets(lens)
    Dtok, _ = CC.clustered_tokens(rng, int(Doff[-1]), centres)
    Qtok, _ = CC.clustered_tokens(rng, 8 * 32, centres)
    return dev(Qtok.reshape(8, 32, 128)), dev(Dtok), dev(Doff)


def test_centroid_assign_by_both_routes(ops, clustered):
    Dtok = clustered[1][:5000]
    C = dev(np.random.default_rng(13).normal(0, 1, (128, 128)).astype(np.float16))
    a, b = ops.centroid_assign(Dtok, C, fused=True), ops.centroid_assign(Dtok, C, fused=False)
    assert a.dtype == torch.int32 and tuple(a.shape) == (5000,) and torch.equal(a, b)


def test_kmeans_centroids_by_both_routes(ops, clustered):
    Dtok = clustered[1]
    a = ops.kmeans_centroids(Dtok, 128, iters=3, seed=1, sample=20000, fused=True)
    b = ops.kmeans_centroids(Dtok, 128, iters=3, seed=1, sample=20000, fused=False)
    assert a.dtype == torch.float16 and tuple(a.shape) == (128, 128) and torch.equal(a, b)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_search_by_both_routes(ops, clustered, monkeypatch):
    from fusion_amd.distributed import ShardedTokenIndex
    Qtok, Dtok, Doff = clustered
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "CENTROID_FUSED", fused)
        C = ops.kmeans_centroids(Dtok, 128, iters=3, seed=1, sample=20000)
        index = ShardedTokenIndex(Dtok, Doff, 40_000).build_centroids(C)
        outs.append(index.search(Qtok, k=100, nprobe=2, ncand=256))
    a, b = outs
    assert tuple(a.ids.shape) == (8, 100) and a.lens.tolist() == b.lens.tolist() == [100] * 8
    assert torch.equal(a.ids, b.ids) and torch.equal(bits(a.scores), bits(b.scores))
