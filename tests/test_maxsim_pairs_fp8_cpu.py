"""e4m3 candidate-list MaxSim without a GPU: the exactness of the grid reference, the restated loop of csrc/rerank8.hip against
hand-checked cases and the sweep's branch table, the C entry's argument checks (reported before any HIP call), the errors
ops.maxsim_pairs_e4m3 raises before the device, ShardedTokenIndex's host logic of the e4m3 storage on CPU tensors, and the shipped
build's resource report."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import maxsim_fp8_cases as F
import maxsim_pairs_fp8_cases as P8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the grid reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", F.LQS)
def test_grid_reference_is_exact_in_float32_and_in_e4m3(Lq):
    """Clean documents score at most 480 per query token, a guard at least 3,584 - 480: one leaked poison row cannot hide."""
    Q = 5
    for m in P8.MAX_DOC_LENS:
        D8, Doff = P8.corpus(m)          # asserts that the reference quantiser reproduces every value
        Q8 = P8.queries(Lq, Q)
        assert D8.dtype == np.uint8 and Q8.dtype == np.uint8 and D8.shape == (P8.PRE + sum(P8.LENS) + P8.POST, 128) and int(Doff[0]) == P8.PRE
        ref64, ref = P8.reference64(Lq, Q, m), P8.reference(Lq, Q, m)      # exact_f32 asserts float32 holds the float64 formula
        assert ref.dtype == np.float32 and np.array_equal(ref64, np.round(ref64)) and np.abs(ref64).max() < 2 ** 19
        lens = np.asarray(P8.LENS)
        clean, guard = np.arange(P8.N) % 2 == 0, (np.arange(P8.N) % 2 == 1) & (lens > 0)
        assert (ref64[:, clean] <= 480 * Lq).all() and (ref64[:, clean & (lens == 0)] == 0).all()
        assert guard.sum() >= 15 and (ref64[:, guard] >= (3584 - 480) * Lq).all()
        # the poison is where the kernel must not look: before Doff[0], after Doff[N], in the guards and past max_doc_len
        Dv, _ = P8.corpus_values(m)
        bad = Dv[:, F.POISON_DIMS].max(axis=1) == F.POISON8
        assert bad[: P8.PRE].all() and bad[int(Doff[-1]):].all()
        last = int(Doff[-2])
        assert not bad[last: last + m].any() and bad[last + m: int(Doff[-1])].all()


# ---- the loop, restated --------------------------------------------------------------------------------------------------------------
def test_loop_restatement_on_hand_checked_cases():
    assert P8.MP8_RB == 8 and P8.MP_SLICE == 128
    rb = P8.row_blocks
    assert rb(1) == [(1, True)] and rb(16) == [(1, False)] and rb(17) == [(2, True)] and rb(64) == [(4, False)] and rb(65) == [(5, True)]
    assert rb(80) == [(5, False)] and rb(96) == [(6, False)] and rb(97) == [(7, True)] and rb(112) == [(7, False)] and rb(113) == [(8, True)]
    assert rb(128) == [(8, False)] and rb(129) == [(8, False), (1, True)] and rb(130) == [(8, False), (1, True)]
    assert rb(511) == [(8, False)] * 3 + [(8, True)] and rb(512) == [(8, False)] * 4 and rb(530) == [(8, False)] * 4 + [(2, True)]
    assert {n for L in P8.CLEAN if L for n, _ in rb(min(L, 512))} == set(range(1, 9))
    assert P8.N == 49 and P8.LENS[-1] == 530 and all(L in P8.LENS[::2] for L in P8.MORE + P8.M.EDGE_LENS + (0,))
    # the candidate draws of maxsim_pairs_cases over this corpus: every document in row 0 of a k >= N launch, the special slots in place
    cand = P8.candidates(2, 64, 7)
    assert cand.shape == (2, 64) and set(range(7, 7 + P8.N)) - set(cand[0].tolist()) <= {int(c) for c in P8.candidates(2, 65, 7)[0]}
    assert cand[0, 1] == cand[0, 0] and cand[0, 63] == -1 and {int(cand[0, 2]), int(cand[0, 3])} == {6, 7 + P8.N}


def test_sweep_lands_on_every_branch():
    hit, by_k, by_m = P8.sweep_branches()
    for k, claims in P8.K_CLAIMS.items():
        assert set(claims) <= by_k[k], (k, sorted(map(str, set(claims) - by_k[k])))
    for m, claims in P8.M_CLAIMS.items():
        assert set(claims) <= by_m[m], (m, sorted(map(str, set(claims) - by_m[m])))
    assert set(P8.BRANCHES) <= hit, sorted(map(str, set(P8.BRANCHES) - hit))
    assert {("blocks", nb) for nb in range(1, 9)} <= set(P8.BRANCHES)      # RB = 8 ships: rounds of 1 through 8 row blocks
    # the EDGE_LENS documents alone give rounds of 1 to 5 and of 8 row blocks under every max_doc_len of the sweep: 6 and 7 come from the added ones
    edge = {nb for L in P8.M.EDGE_LENS for m in P8.MAX_DOC_LENS for nb, _ in P8.row_blocks(min(L, m))}
    assert edge == {1, 2, 3, 4, 5, 8} and {5, 6, 7, 8} <= {nb for L in P8.MORE for nb, _ in P8.row_blocks(L)}


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def call(L, **kw):
    a = dict(Qtok8=0x1000, Dtok8=0x2000, Doff=0x3000, sumL=100, max_doc_len=512, Q=2, Lq=64, N=10, dim=128, descale_exp=16, cand=0x4000, ldc=8,
             cand_len=None, k=8, id_base=0, scores=0x5000, lds=8)
    a.update(kw)
    p = lambda v: None if not v else C.c_void_p(v)      # noqa: E731
    return L.fz_maxsim_pairs_e4m3(p(a["Qtok8"]), p(a["Dtok8"]), p(a["Doff"]), a["sumL"], a["max_doc_len"], a["Q"], a["Lq"], a["N"], a["dim"],
                                  a["descale_exp"], p(a["cand"]), a["ldc"], p(a["cand_len"]), a["k"], a["id_base"], p(a["scores"]), a["lds"], None)


def test_abi_argument_validation_without_gpu():
    """Every refusal comes before the first HIP call, so the (fake, aligned) pointers are never touched.  Classes in pair_slots_args' order."""
    from fusion_amd import _lib
    L = _lib.lib()
    assert "fz_maxsim_pairs_e4m3" in _lib.EXPORTS and L.fz_abi_version() == 20      # an additive entry: the ABI version stays
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    # 1. negative sizes and leading dimensions
    for name in ("Q", "N", "k"):
        assert call(L, **{name: -1}) == ARG, name
    assert call(L, Lq=0) == ARG and call(L, Lq=-64) == ARG
    assert call(L, ldc=7) == ARG and call(L, lds=7) == ARG
    # 2. null pointers where a non-empty tensor is needed
    for name in ("Qtok8", "Doff", "cand", "scores"):
        assert call(L, **{name: 0}) == ARG, name
    # 3. the storage's own arguments: a token matrix for sumL != 0, the descale exponent as in fz_maxsim_e4m3
    assert call(L, Dtok8=0) == ARG
    for e in (-33, 33, 1000, -(2 ** 31)):
        assert call(L, descale_exp=e) == ARG, e
    for e in (-32, 0, 30, 32):
        assert call(L, descale_exp=e, Q=0) == OK, e
    # 4. shapes outside what is built
    assert call(L, dim=64) == UNS and call(L, dim=256) == UNS
    for Lq in (16, 48, 96, 256):
        assert call(L, Lq=Lq) == UNS, Lq
    assert call(L, Qtok8=0x1008) == UNS and call(L, Dtok8=0x2004) == UNS and call(L, Dtok8=0x2008) == UNS
    # the order: argument errors first, then unsupported shapes, then the empty batch, then sumL / max_doc_len
    assert call(L, dim=64, ldc=7) == ARG and call(L, dim=64, descale_exp=33) == ARG and call(L, Dtok8=0x2004, descale_exp=-33) == ARG
    assert call(L, dim=64, Q=0) == UNS and call(L, Qtok8=0x1008, k=0, ldc=0, lds=0) == UNS
    assert call(L, Q=0, max_doc_len=0) == OK and call(L, k=0, ldc=0, lds=0, max_doc_len=99999) == OK
    # 5. sumL / max_doc_len, once there is work
    assert call(L, sumL=-1) == ARG and call(L, max_doc_len=0) == ARG and call(L, max_doc_len=-5) == ARG
    assert call(L, max_doc_len=16385) == UNS
    # nothing to do: no launch, null pointers welcome
    assert call(L, Q=0, Qtok8=0, cand=0, scores=0, Doff=0) == OK
    assert call(L, k=0, ldc=0, lds=0, Qtok8=0, cand=0, scores=0, Doff=0) == OK
    assert call(L, Q=0, Dtok8=0, sumL=0) == OK


# ---- ops.maxsim_pairs_e4m3: errors raised before anything reaches the device -----------------------------------------------------------
def test_ops_type_and_shape_errors():
    from fusion_amd import ops
    Q8, D8 = torch.zeros((2, 64, 128), dtype=torch.uint8), torch.zeros((10, 128), dtype=torch.uint8)
    Doff, cand = torch.zeros(4, dtype=torch.int64), torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(TypeError, match="Q8.*GPU"):
        ops.maxsim_pairs_e4m3(Q8, D8, Doff, cand)                 # CPU tensors: there is no CPU path
    with pytest.raises(TypeError):
        ops.maxsim_pairs_e4m3(None, D8, Doff, cand)
    with pytest.raises(TypeError):
        ops.maxsim_pairs_e4m3(Q8.view(torch.float8_e4m3fn), D8, Doff, cand)      # the same bytes, still on the CPU
    if not torch.cuda.is_available():
        return
    g = lambda t: t.cuda()      # noqa: E731
    Q8, D8, Doff, cand = g(Q8), g(D8), g(Doff), g(cand)
    ok = dict(Q8=Q8, D8=D8, Doff=Doff, cand=cand)
    for bad in (dict(Q8=Q8.half()), dict(D8=D8.half()), dict(D8=D8.to(torch.int8)), dict(Doff=Doff.int()), dict(cand=cand.int()),
                dict(cand_len=torch.zeros(2, dtype=torch.int64, device="cuda")), dict(out=torch.zeros((2, 5), dtype=torch.float64, device="cuda")),
                dict(cand=cand.cpu())):
        with pytest.raises(TypeError):
            ops.maxsim_pairs_e4m3(**{**ok, **bad})
    for bad in (dict(Q8=Q8[0]), dict(D8=D8[:, :64]), dict(cand=cand[:1]), dict(cand=cand[0]),
                dict(cand_len=torch.zeros(3, dtype=torch.int32, device="cuda")), dict(out=torch.zeros((2, 6), device="cuda")),
                dict(max_doc_len=0), dict(Doff=Doff[:0]), dict(q_exp=16), dict(d_exp=-9), dict(q_exp=8.0), dict(d_exp=True)):
        with pytest.raises(ValueError):
            ops.maxsim_pairs_e4m3(**{**ok, **bad})


# ---- ShardedTokenIndex: the host logic of the third storage, on CPU tensors ------------------------------------------------------------
def cpu_index(rows=10, **kw):
    from fusion_amd.distributed import ShardedTokenIndex
    Doff = torch.tensor([0, 3, 3, rows], dtype=torch.int64)
    return ShardedTokenIndex(torch.zeros((rows, 128), dtype=torch.float16), Doff, 5, **kw)


def test_index_storage_errors_on_cpu_tensors():
    from fusion_amd.distributed import ShardedTokenIndex
    assert ShardedTokenIndex.q_exp == 8 and ShardedTokenIndex.tok8 is None and ShardedTokenIndex.d_exp is None
    # one storage decides the score
    ix = cpu_index()
    ix.packed = torch.zeros((10, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match="compressed"):
        ix.quantize()
    ix = cpu_index()
    ix.Dtok = None
    with pytest.raises(ValueError, match="gone"):
        ix.quantize()
    ix = cpu_index()
    ix.tok8, ix.d_exp = torch.zeros((10, 128), dtype=torch.uint8), 8      # a quantised shard
    with pytest.raises(ValueError, match="already quantised"):
        ix.quantize()
    ix.candidates, ix.codes, ix.centroids = object(), torch.zeros(10, dtype=torch.int32), torch.zeros((4, 128), dtype=torch.float16)
    with pytest.raises(ValueError, match="quantised"):
        ix.compress(2)
    for e in (16, -9, 8.0, None):
        with pytest.raises(ValueError):
            cpu_index().quantize(e)
    with pytest.raises(ValueError, match="not quantised"):
        cpu_index().dequantized()
    # build_e4m3's count checks come before anything is quantised
    Doff = torch.tensor([0, 3, 3, 10], dtype=torch.int64)
    blk = lambda n: torch.zeros((n, 128), dtype=torch.float16)      # noqa: E731
    with pytest.raises(ValueError, match="more than"):
        ShardedTokenIndex.build_e4m3(iter([blk(11)]), Doff, 0, device="cpu")
    with pytest.raises(ValueError, match="hold 0 token rows"):
        ShardedTokenIndex.build_e4m3(iter([]), Doff, 0, device="cpu")
    with pytest.raises(ValueError, match="hold 0 token rows"):
        ShardedTokenIndex.build_e4m3(iter([blk(0), blk(0)]), Doff, 0, device="cpu")
    with pytest.raises(ValueError):
        ShardedTokenIndex.build_e4m3(iter([blk(10)]), Doff, 0, scale_exp=16, device="cpu")
    empty = ShardedTokenIndex.build_e4m3(iter([]), torch.zeros(1, dtype=torch.int64), 3, scale_exp=6, device="cpu", max_doc_len=40)
    assert empty.N == 0 and empty.tok8.shape == (0, 128) and empty.tok8.dtype == torch.uint8 and empty.d_exp == 6 and empty.Dtok is None
    assert empty.id_base == 3 and empty.max_doc_len == 40 and empty.candidates is None


def test_memory_bytes_counts_the_e4m3_rows_under_tokens():
    keys = {"tokens", "codes", "packed", "candidates", "total"}
    ix = cpu_index()
    before = ix.memory_bytes()
    assert set(before) == keys and before["tokens"] == 256 * 10 and before["total"] == 256 * 10
    ix.tok8, ix.d_exp = torch.zeros((10, 128), dtype=torch.uint8), 8      # quantize(keep_tokens=True)
    both = ix.memory_bytes()
    assert set(both) == keys and both["tokens"] == 384 * 10 and both["total"] == 384 * 10
    ix.Dtok = None                                                        # quantize()
    only = ix.memory_bytes()
    assert set(only) == keys and only["tokens"] == 128 * 10 and only["packed"] == 0 and only["total"] == 128 * 10
    ix.codes = torch.zeros(10, dtype=torch.int32)
    assert ix.memory_bytes()["total"] == 128 * 10 + 40


# ---- the shipped build ---------------------------------------------------------------------------------------------------------------
def test_the_e4m3_pairs_kernels_hold_everything_in_registers():
    """The report the compile left next to the objects: rerank8.res holds exactly the three instantiations, nothing spilled; the float16
    and the residual kernels, which share maxsim_pairs.h's helpers with it, spill nothing either."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if not {"rerank8", "rerank", "rerank_residual"} <= set(res):
        pytest.skip("the build left no rerank8.res / rerank.res / rerank_residual.res next to the objects: run `make -C fusion_amd/csrc`")
    mine = {kernel_resources.short(n): r for n, r in res["rerank8"].items()}
    assert sorted(mine) == [f"maxsim_pairs8_kernel<{ncb}>" for ncb in (2, 4, 8)], sorted(mine)      # Lq = 32, 64, 128
    for name, r in mine.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, f"{name}: {r['vgpr_spill']} spilled VGPRs, {r['scratch']} B/lane of scratch"
        assert r["lds"] == 0, f"{name}: the walk uses no LDS"
    plain = {kernel_resources.short(n): r for n, r in res["rerank"].items() if "maxsim_pairs_kernel" in n}
    resid = {kernel_resources.short(n): r for n, r in res["rerank_residual"].items() if "maxsim_residual_kernel" in n}
    assert len(plain) == 3 and len(resid) == 6, (sorted(plain), sorted(resid))
    for name, r in {**plain, **resid}.items():
        assert r["vgpr_spill"] == 0, f"{name}: {r['vgpr_spill']} spilled VGPRs"
