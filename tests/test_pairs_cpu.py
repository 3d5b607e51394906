"""Pair scores and list completion without a GPU: the argument checks of fz_dot_pairs_f32 / fz_sparse_dot_pairs_f32 (reported before any
HIP call), the type and shape errors of ops.dot_pairs / ops.sparse_dot_pairs, the numpy restatement the GPU test compares against on
hand-checked cases, Aggregator.complete_topk's argument errors, and the shipped build's resource report for the new kernels."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import pairs_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def _p(v):
    return None if not v else C.c_void_p(v)


def dense(L, **kw):
    a = dict(Qn=0x1000, ldq=8, Dn=0x2000, ldd=8, Q=2, N=10, d=8, cand=0x4000, ldc=6, cand_len=None, W=6, id_base=0, out=0x5000, ldo=6)
    a.update(kw)
    return L.fz_dot_pairs_f32(_p(a["Qn"]), a["ldq"], _p(a["Dn"]), a["ldd"], a["Q"], a["N"], a["d"], _p(a["cand"]), a["ldc"], _p(a["cand_len"]),
                              a["W"], a["id_base"], _p(a["out"]), a["ldo"], None)


def sparse(L, **kw):
    a = dict(toff=0x1000, pdoc=0x2000, pw=0x3000, qoff=0x4000, qterms=0x5000, qw=0x6000, Q=2, N=10, cand=0x7000, ldc=6, cand_len=None, W=6,
             id_base=0, out=0x8000, ldo=6)
    a.update(kw)
    return L.fz_sparse_dot_pairs_f32(_p(a["toff"]), _p(a["pdoc"]), _p(a["pw"]), _p(a["qoff"]), _p(a["qterms"]), _p(a["qw"]), a["Q"], a["N"],
                                     _p(a["cand"]), a["ldc"], _p(a["cand_len"]), a["W"], a["id_base"], _p(a["out"]), a["ldo"], None)


def test_abi_argument_validation_without_gpu():
    """Every refusal comes before the first HIP call, so the (fake, aligned) pointers are never touched."""
    from fusion_amd import _lib
    L = _lib.lib()
    assert {"fz_dot_pairs_f32", "fz_sparse_dot_pairs_f32"} <= set(_lib.EXPORTS) and L.fz_abi_version() == 20      # additive entries
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    # -- dense: null pointers where a non-empty tensor is needed, leading dimensions, negative sizes
    for name in ("Qn", "Dn", "cand", "out"):
        assert dense(L, **{name: 0}) == ARG, name
    assert dense(L, ldc=5) == ARG and dense(L, ldo=5) == ARG and dense(L, ldq=4) == ARG and dense(L, ldd=4) == ARG
    for name in ("Q", "N", "W"):
        assert dense(L, **{name: -1}) == ARG, name
    assert dense(L, d=0) == ARG and dense(L, d=-8) == ARG
    # shapes outside what is built
    assert dense(L, d=6) == UNS and dense(L, ldq=9, ldd=9) == UNS and dense(L, ldq=10) == UNS and dense(L, ldd=10) == UNS
    assert dense(L, d=16388, ldq=16388, ldd=16388) == UNS and dense(L, d=16384, ldq=16384, ldd=16384, Q=0) == OK
    assert dense(L, Qn=0x1008) == UNS and dense(L, Dn=0x2004) == UNS
    # the order of fz_maxsim_pairs_f16: argument errors, then unsupported shapes, then the empty batch
    assert dense(L, d=6, ldc=5) == ARG
    assert dense(L, d=6, Q=0) == UNS and dense(L, Qn=0x1008, W=0, ldc=0, ldo=0) == UNS
    # nothing to do: no launch, null pointers welcome; a shard of no documents needs no Dn (but would launch: not called here)
    assert dense(L, Q=0, Qn=0, Dn=0, cand=0, out=0) == OK
    assert dense(L, W=0, ldc=0, ldo=0, Qn=0, Dn=0, cand=0, out=0) == OK
    assert dense(L, Q=0, N=0, Dn=0) == OK
    # -- sparse
    for name in ("qoff", "cand", "out", "toff"):
        assert sparse(L, **{name: 0}) == ARG, name
    assert sparse(L, ldc=5) == ARG and sparse(L, ldo=5) == ARG
    for name in ("Q", "N", "W"):
        assert sparse(L, **{name: -1}) == ARG, name
    assert sparse(L, Q=0, ldc=5) == ARG                      # argument errors before the empty batch
    assert sparse(L, Q=0, toff=0, pdoc=0, pw=0, qoff=0, qterms=0, qw=0, cand=0, out=0) == OK
    assert sparse(L, W=0, ldc=0, ldo=0, toff=0, qoff=0, cand=0, out=0) == OK
    assert sparse(L, Q=0, N=0, toff=0) == OK


# ---- ops.dot_pairs / ops.sparse_dot_pairs: errors raised before anything reaches the device --------------------------------------------
def test_ops_type_and_shape_errors():
    from fusion_amd import ops
    Qn, Dn, cand = torch.zeros((2, 8)), torch.zeros((10, 8)), torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(TypeError, match="Qn.*GPU"):
        ops.dot_pairs(Qn, Dn, cand)                          # CPU tensors: there is no CPU path
    with pytest.raises(TypeError):
        ops.dot_pairs(None, Dn, cand)
    with pytest.raises(TypeError, match="SparseIndex"):
        ops.sparse_dot_pairs(None, cand, cand, cand, cand)
    if not torch.cuda.is_available():
        return
    g = lambda t: t.cuda()      # noqa: E731
    Qn, Dn, cand = g(Qn), g(Dn), g(cand)
    ok = dict(Qn=Qn, Dn=Dn, cand=cand)
    for bad in (dict(Qn=Qn.double()), dict(Dn=Dn.half()), dict(cand=cand.int()), dict(cand=cand.cpu()),
                dict(cand_len=torch.zeros(2, dtype=torch.int64, device="cuda")), dict(out=torch.zeros((2, 5), dtype=torch.float64, device="cuda"))):
        with pytest.raises(TypeError):
            ops.dot_pairs(**{**ok, **bad})
    for bad in (dict(Qn=Qn[0]), dict(Dn=Dn[:, :4]), dict(cand=cand[:1]), dict(cand=cand[0]),
                dict(cand_len=torch.zeros(3, dtype=torch.int32, device="cuda")), dict(out=torch.zeros((2, 6), device="cuda"))):
        with pytest.raises(ValueError):
            ops.dot_pairs(**{**ok, **bad})
    Qm, Dm = P.sparse_corpus(1)
    index = ops.sparse_index(g(torch.from_numpy(Dm)))
    qoff, qterms, qw = ops.sparse_rows(g(torch.from_numpy(Qm)))
    cand = torch.zeros((Qm.shape[0], 5), dtype=torch.int64, device="cuda")
    ok = dict(index=index, qoff=qoff, qterms=qterms, qw=qw, cand=cand)
    for bad in (dict(qoff=qoff.int()), dict(qterms=qterms.long()), dict(qw=qw.double()), dict(cand=cand.int()), dict(index=Dm),
                dict(cand_len=torch.zeros(Qm.shape[0], dtype=torch.int64, device="cuda"))):
        with pytest.raises(TypeError):
            ops.sparse_dot_pairs(**{**ok, **bad})
    for bad in (dict(cand=cand[:2]), dict(qw=qw[:-1]), dict(out=torch.zeros((Qm.shape[0], 4), device="cuda"))):
        with pytest.raises(ValueError):
            ops.sparse_dot_pairs(**{**ok, **bad})


# ---- the restatements the GPU test compares against ---------------------------------------------------------------------------------
def test_expectation_gathers_the_reference():
    ref = np.arange(12, dtype=np.float32).reshape(2, 6)
    cand = np.array([[3, 3, -1, 9, 2], [8, 4, 5, 6, 7]], dtype=np.int64)
    inf = -np.inf
    assert P.expected(ref, cand, [5, 3], 3).tolist() == [[0.0, 0.0, inf, inf, inf], [11.0, 7.0, 8.0, inf, inf]]
    big = P.BIG_BASE
    assert P.expected(ref, cand + big, None, 3 + big).tolist() == [[0.0, 0.0, inf, inf, inf], [11.0, 7.0, 8.0, 9.0, 10.0]]
    assert np.isinf(P.expected(ref[:, :0], cand, None, 0)).all()                                      # a shard of no documents owns nothing


def test_sparse_chain_on_a_hand_checked_case():
    # documents 0..3 over 3 terms:   term 0: (1, 0.5) (3, 0.25)   term 1: none   term 2: (0, 2.0) (1, 1.0) (3, 4.0)
    toff = np.array([0, 2, 2, 5]); pdoc = np.array([1, 3, 0, 1, 3], dtype=np.int32); pw = np.array([0.5, 0.25, 2.0, 1.0, 4.0], dtype=np.float32)
    qoff = np.array([0, 3, 3]); qterms = np.array([0, 1, 2], dtype=np.int32); qw = np.array([2.0, 9.0, 0.5], dtype=np.float32)
    cand = np.array([[10, 11, 12, 13, 14, 9, -1], [11] * 7], dtype=np.int64)
    got = P.sparse_chain(toff, pdoc, pw, qoff, qterms, qw, cand, [7, 7], 10, 4)
    inf = -np.inf
    assert got.tolist() == [[1.0, 1.5, 0.0, 2.5, inf, inf, inf], [0.0] * 7]
    assert not np.signbit(got[0, 2]) and not np.signbit(got[1]).any()                                  # +0.0: no shared term / no term
    assert P.sparse_chain(toff, pdoc, pw, qoff, qterms, qw, cand, [2, 0], 10, 4).tolist() == [[1.0, 1.5] + [inf] * 5, [inf] * 7]
    # one rounding per product and per add, in term order: 1e8 + 1 - 1e8 is 0 in float32, in this order
    toff, pdoc, pw = np.array([0, 1, 2, 3]), np.zeros(3, dtype=np.int32), np.array([1e8, 1.0, -1e8], dtype=np.float32)
    one = np.ones(3, dtype=np.float32)
    assert P.sparse_chain(toff, pdoc, pw, np.array([0, 3]), np.arange(3, dtype=np.int32), one, np.array([[0]]), None, 0, 1).tolist() == [[0.0]]


def test_the_seeded_cases_hold_what_they_promise():
    Qn, Dn = P.dense_corpus(1, 700, 100)
    assert Qn.shape == (130, 100) and not Dn[P.ZERO_ROW].any() and 0 < np.abs(Qn[2]).max() < 1e-36
    for W in P.WIDTHS:
        cand, lens = P.candidates(W, 130, W, 700, P.BIG_BASE)
        assert lens[:3].tolist() == [W, 0, (W + 1) // 2] and (cand < 0).any() == (W > 1)
        if W > 2:
            local = cand - P.BIG_BASE
            assert (local == -1).any() and (local == 700).any() and (cand[:, -1] == cand[:, -2]).all()
    assert max(P.WIDTHS) > P.DP_SLOTS and {1, 63, 64, 65, 129} <= set(P.WIDTHS) and P.DIMS == (768, 100, 4) and P.QS == (1, 3, 130)
    Qm, Dm = P.sparse_corpus(3)
    toff, pdoc, pw = P.inverted(Dm)
    qoff, qterms, qw = P.query_rows(Qm)
    n = np.diff(qoff)
    assert n[P.SP_LONG_QUERY] == 300 and n[P.SP_EMPTY_QUERY] == 0
    assert all(toff[t + 1] == toff[t] for t in P.SP_EMPTY_TERMS) and set(P.SP_EMPTY_TERMS) <= set(qterms[qoff[0]:qoff[1]].tolist())
    assert not np.isin(pdoc, P.SP_EMPTY_DOCS).any()
    cand, lens = P.sparse_candidates(4, toff, pdoc, qoff, qterms, 40, P.BIG_BASE)
    t0 = [t for t in qterms[qoff[0]:qoff[1]] if toff[t + 1] > toff[t]]
    assert any(cand[0, 0] - P.BIG_BASE == pdoc[toff[t]] and cand[0, 1] - P.BIG_BASE == pdoc[toff[t + 1] - 1] for t in t0)
    # the chain agrees with the dense product up to rounding
    got = P.sparse_chain(toff, pdoc, pw, qoff, qterms, qw, cand, lens, P.BIG_BASE, P.SP_N)
    want = P.expected((Qm.astype(np.float64) @ Dm.T.astype(np.float64)).astype(np.float32), cand, lens, P.BIG_BASE)
    assert (np.isfinite(got) == np.isfinite(want)).all() and np.allclose(got[np.isfinite(got)], want[np.isfinite(want)], rtol=1e-5, atol=1e-6)


# ---- Aggregator.complete_topk: what it refuses before anything reaches the device ----------------------------------------------------
def test_complete_topk_argument_errors():
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    ids = torch.tensor([[3, 1, -1]], dtype=torch.int64)
    lst = RankedTopk.from_search(torch.tensor([[2.0, 1.0, float("-inf")]]), ids)
    score = lambda U, n: torch.zeros(U.shape)      # noqa: E731
    with pytest.raises(ValueError, match="no system"):
        Aggregator.complete_topk({}, {})
    with pytest.raises(TypeError, match="RankedTopk"):
        Aggregator.complete_topk({"a": (ids, ids)}, {})
    with pytest.raises(KeyError, match="not one of the systems"):
        Aggregator.complete_topk({"a": lst}, {"b": score})
    with pytest.raises(TypeError, match="not callable"):
        Aggregator.complete_topk({"a": lst}, {"a": 3.0})
    for depth in (0, -5):
        with pytest.raises(ValueError, match="depth"):
            Aggregator.complete_topk({"a": lst}, {"a": score}, depth=depth)
    with pytest.raises(ValueError, match="at most 8"):
        Aggregator.complete_topk({str(i): lst for i in range(9)}, {})
    with pytest.raises(TypeError, match="GPU"):      # the join itself has no CPU path
        Aggregator.complete_topk({"a": lst}, {"a": score})


def test_complete_topk_holds_a_scorer_to_its_contract(monkeypatch):
    """With the join stood in for (it has no CPU path), what a scorer returns is checked before anything is ranked: a float32 or float64
    tensor of the union's shape (ops.check_pair_plane, under complete_topk's name for the scorer)."""
    from fusion_amd import ops
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    ids = torch.tensor([[3, 1, -1]], dtype=torch.int64)
    lst = RankedTopk.from_search(torch.tensor([[2.0, 1.0, float("-inf")]]), ids)
    monkeypatch.setattr(ops, "lists_columns", lambda ids, lens, planes: (ids[0], None, None, lens[0], None))
    for bad in (lambda U, n: torch.zeros(U.shape, dtype=torch.float16), lambda U, n: torch.zeros(U.shape, dtype=torch.int64), lambda U, n: [0.0] * 3):
        with pytest.raises(TypeError, match=r"^Aggregator\.complete_topk: the scorer of 'a' must return a float32 or float64 tensor$"):
            Aggregator.complete_topk({"a": lst}, {"a": bad})
    for bad, shape in ((lambda U, n: torch.zeros((1, 2)), (1, 2)), (lambda U, n: torch.zeros(3, dtype=torch.float64), (3,))):
        with pytest.raises(ValueError, match=rf"^Aggregator\.complete_topk: the scorer of 'a' returned {re.escape(str(shape))} for ids \(1, 3\)$"):
            Aggregator.complete_topk({"a": lst}, {"a": bad})
    for good in (torch.zeros((1, 3)), torch.zeros((1, 3), dtype=torch.float64)):
        assert ops.check_pair_plane(good, 1, 3, "x") is good


# ---- the shipped build ---------------------------------------------------------------------------------------------------------------
def test_the_pair_kernels_hold_everything_in_registers(tmp_path):
    """The report the compile left next to the object (fusion_amd/csrc/pairs.res); if the objects predate it, the one source is compiled
    once more into a temporary directory -- never into the tree -- as tests/test_kernel_resources_cpu.py does."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if "pairs" not in res:
        import subprocess
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip("no pairs.res next to the objects and no hipcc to make it: run `make -C fusion_amd/csrc` where ROCm is installed")
        flags = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()
        r = subprocess.run([hipcc, *flags, "-c", os.path.join(ROOT, "fusion_amd", "csrc", "pairs.hip"), "-o", str(tmp_path / "pairs.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        (tmp_path / "pairs.res").write_text(r.stderr)
        res = kernel_resources.load(str(tmp_path))
    mine = {kernel_resources.short(n): r for n, r in res["pairs"].items()}
    assert len(mine) == 3 and any("dot_pairs_kernel" in n and "sparse" not in n for n in mine) and any("sparse_dot_pairs_kernel" in n for n in mine), sorted(mine)
    for name, r in mine.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, f"{name}: {r['vgpr_spill']} spilled VGPRs, {r['scratch']} B/lane of scratch"
    # four workgroups of four waves per CU (the LDS bound at d = 768) need 128 VGPRs or fewer
    dot = next(r for n, r in mine.items() if "dot_pairs_kernel" in n and "sparse" not in n)
    assert dot["vgprs"] + dot.get("agprs", 0) <= 128, dot
