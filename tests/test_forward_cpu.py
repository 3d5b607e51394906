"""The forward index without a GPU: the argument checks of fz_sparse_fwd_pairs_f32 / fz_tfidf_doc_scores_fwd_f64 /
fz_bm25_doc_scores_fwd_pv_f64 (reported before any HIP call), the route and type errors of the ops, the numpy restatements the GPU test
compares against -- on a hand-checked case, and against pairs_cases.sparse_chain byte for byte -- and the build's resource report."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import forward_cases as F
import pairs_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fz_sparse_fwd_max_vocab", "fz_sparse_fwd_pairs_f32", "fz_tfidf_doc_scores_fwd_f64", "fz_bm25_doc_scores_fwd_pv_f64")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def _p(v):
    return None if not v else C.c_void_p(v)


def sparse(L, **kw):
    a = dict(foff=0x1000, rows=0x2000, V=500, qoff=0x4000, qterms=0x5000, qw=0x6000, Q=2, N=10, cand=0x7000, ldc=6, cand_len=None, W=6,
             id_base=0, out=0x8000, ldo=6)
    a.update(kw)
    return L.fz_sparse_fwd_pairs_f32(_p(a["foff"]), _p(a["rows"]), a["V"], _p(a["qoff"]), _p(a["qterms"]), _p(a["qw"]), a["Q"], a["N"],
                                     _p(a["cand"]), a["ldc"], _p(a["cand_len"]), a["W"], a["id_base"], _p(a["out"]), a["ldo"], None)


LEX = dict(toff=0x1000, pdoc=0x2000, vals=0x3000, idf=0x3800, foff=0x4000, fterm=0x5000, fpos=0x6000, qoff=0x7000, qterms=0x8000, Q=2, N=10,
           docs=0x9000, G=3, out=0xa000)


def tfidf(L, **kw):
    a = {**LEX, **kw}
    return L.fz_tfidf_doc_scores_fwd_f64(_p(a["toff"]), _p(a["pdoc"]), _p(a["vals"]), _p(a["idf"]), _p(a["foff"]), _p(a["fterm"]), _p(a["fpos"]),
                                         _p(a["qoff"]), _p(a["qterms"]), a["Q"], a["N"], _p(a["docs"]), a["G"], _p(a["out"]), None)


def bm25(L, **kw):
    a = {**LEX, **kw}
    return L.fz_bm25_doc_scores_fwd_pv_f64(_p(a["toff"]), _p(a["pdoc"]), _p(a["vals"]), _p(a["foff"]), _p(a["fterm"]), _p(a["fpos"]), _p(a["qoff"]),
                                           _p(a["qterms"]), a["Q"], a["N"], _p(a["docs"]), a["G"], _p(a["out"]), None)


def test_abi_argument_validation_without_gpu():
    """Every refusal comes before the first HIP call, so the (fake, aligned) pointers are never touched."""
    from fusion_amd import _lib
    L = _lib.lib()
    assert set(NEW) <= set(_lib.EXPORTS) and L.fz_abi_version() == 20                                 # additive entries
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    assert all(name + "(" in header for name in NEW)
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    cap = L.fz_sparse_fwd_max_vocab()
    assert cap >= 65536 and 2 * (2 * (cap // 8) + 4096) <= 160 * 1024                                   # two workgroups' bitmaps and rank tables in a CU's LDS
    # -- sparse: null pointers where a non-empty tensor is needed, leading dimensions, negative sizes
    for name in ("qoff", "cand", "out", "foff"):
        assert sparse(L, **{name: 0}) == ARG, name
    assert sparse(L, ldc=5) == ARG and sparse(L, ldo=5) == ARG
    for name in ("Q", "N", "W", "V"):
        assert sparse(L, **{name: -1}) == ARG, name
    # shapes outside what is built
    assert sparse(L, V=cap + 1) == UNS and sparse(L, rows=0x2004) == UNS
    # the order of the pair entries: argument errors, then unsupported shapes, then the empty batch
    assert sparse(L, V=cap + 1, ldc=5) == ARG and sparse(L, Q=0, ldc=5) == ARG
    assert sparse(L, V=cap + 1, Q=0) == UNS and sparse(L, V=cap + 1, W=0, ldc=0, ldo=0) == UNS
    # nothing to do: no launch, null pointers welcome
    assert sparse(L, V=cap, Q=0) == OK
    assert sparse(L, Q=0, foff=0, rows=0, qoff=0, qterms=0, qw=0, cand=0, out=0) == OK
    assert sparse(L, W=0, ldc=0, ldo=0, foff=0, qoff=0, cand=0, out=0) == OK
    assert sparse(L, Q=0, N=0, foff=0) == OK
    # -- lexical
    for call, needs in ((tfidf, ("vals", "idf", "foff", "fterm", "fpos", "qoff", "qterms", "docs", "out")),
                        (bm25, ("vals", "foff", "fterm", "fpos", "qoff", "qterms", "docs", "out"))):
        for name in needs:
            assert call(L, **{name: 0}) == ARG, (call.__name__, name)
        assert call(L, Q=-1) == ARG and call(L, N=-1) == ARG and call(L, G=0) == ARG and call(L, G=-2) == ARG
        assert call(L, Q=0, G=0) == ARG                                                                 # argument errors before the empty batch
        assert call(L, Q=0) == OK and call(L, Q=0, **{n: 0 for n in needs}) == OK


# ---- the ops: errors raised before anything reaches the device ------------------------------------------------------------------------
def test_ops_route_and_type_errors():
    from fusion_amd import ops
    from fusion_amd.retrievers.bm25 import BM25, TFIDF
    cand = torch.zeros((2, 5), dtype=torch.int64)
    for bad in ("sideways", "Forward", 1):
        with pytest.raises(ValueError, match="route"):
            ops.sparse_dot_pairs(None, cand, cand, cand, cand, route=bad)                              # the route is looked at first
    for route in (None, "inverted", "forward"):
        with pytest.raises(TypeError, match="SparseIndex"):
            ops.sparse_dot_pairs(None, cand, cand, cand, cand, route=route)
    with pytest.raises(TypeError, match="GPU"):
        ops.forward_index(torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), 5)     # there is no CPU path
    with pytest.raises(TypeError):
        ops.forward_index(None, None, 5)
    assert ops.SparseIndex.forward is None and TFIDF.forward is None and ops.PAIR_ROUTES == (None, "inverted", "forward")
    for model in (TFIDF(["a b", "b c c"], device="cpu"), BM25(["a b", "b c c"], 1.2, 0.7, device="cpu")):
        with pytest.raises(ValueError, match="route"):
            model.doc_scores(["a"], [[0]], route="sideways")
        with pytest.raises(ValueError, match="no forward index"):
            model.doc_scores(["a"], [[0]], route="forward")
        with pytest.raises(TypeError, match="GPU"):
            model.build_forward()
        assert model.forward is None
    with pytest.raises(TypeError, match="ForwardIndex"):
        t = torch.zeros(1)
        ops.lexical_doc_scores_fwd("pv", t, t, t, None, None, t, t, 1, 1, t)
    if not torch.cuda.is_available():
        return
    index = ops.sparse_index(torch.from_numpy(P.sparse_corpus(1)[1]).cuda())
    q = ops.sparse_rows(torch.from_numpy(P.sparse_corpus(1)[0]).cuda())
    cand = torch.zeros((q[0].numel() - 1, 5), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="no forward index"):
        ops.sparse_dot_pairs(index, *q, cand, route="forward")


# ---- the restatements the GPU test compares against ---------------------------------------------------------------------------------
def test_the_restatements_on_a_hand_checked_case():
    # documents 0..3 over 3 terms:   term 0: (1, 0.5) (3, 0.25)   term 1: none   term 2: (0, 2.0) (1, 1.0) (3, 4.0)
    toff = np.array([0, 2, 2, 5]); pdoc = np.array([1, 3, 0, 1, 3], dtype=np.int32); pw = np.array([0.5, 0.25, 2.0, 1.0, 4.0], dtype=np.float32)
    foff, fterm, fpos = F.forward_build(toff, pdoc, 4)
    assert foff.tolist() == [0, 1, 3, 3, 5] and fterm.tolist() == [2, 0, 2, 0, 2] and fpos.tolist() == [2, 0, 3, 1, 4]
    assert foff.dtype == np.int64 and fterm.dtype == np.int32 and fpos.dtype == np.int32
    assert pw[fpos].tolist() == [2.0, 0.5, 1.0, 0.25, 4.0]
    # documents past the last posting and an index of none get empty rows
    assert F.forward_build(toff, pdoc, 6)[0].tolist() == [0, 1, 3, 3, 5, 5, 5]
    assert [x.tolist() for x in F.forward_build(np.zeros(4, dtype=np.int64), pdoc[:0], 2)] == [[0, 0, 0], [], []]
    qoff = np.array([0, 3, 3]); qterms = np.array([0, 1, 2], dtype=np.int32); qw = np.array([2.0, 9.0, 0.5], dtype=np.float32)
    cand = np.array([[10, 11, 12, 13, 14, 9, -1], [11] * 7], dtype=np.int64)
    got = F.row_walk(foff, fterm, pw[fpos], qoff, qterms, qw, cand, [7, 7], 10, 4)
    inf = -np.inf
    assert got.tolist() == [[1.0, 1.5, 0.0, 2.5, inf, inf, inf], [0.0] * 7]
    assert not np.signbit(got[0, 2]) and not np.signbit(got[1]).any()                                  # +0.0: no shared term / no term
    assert F.row_walk(foff, fterm, pw[fpos], qoff, qterms, qw, cand, [2, 0], 10, 4).tolist() == [[1.0, 1.5] + [inf] * 5, [inf] * 7]
    # one rounding per product and per add, in term order: 1e8 + 1 - 1e8 is 0 in float32, in this order (1 in any other)
    toff, pdoc, pw = np.array([0, 1, 2, 3]), np.zeros(3, dtype=np.int32), np.array([1e8, 1.0, -1e8], dtype=np.float32)
    foff, fterm, fpos = F.forward_build(toff, pdoc, 1)
    one = np.ones(3, dtype=np.float32)
    assert F.row_walk(foff, fterm, pw[fpos], np.array([0, 3]), np.arange(3, dtype=np.int32), one, np.array([[0]]), None, 0, 1).tolist() == [[0.0]]
    # a product of -0.0 leaves +0.0: the chain starts from +0.0
    neg = F.row_walk(foff, fterm, np.array([0.0, 0.0, 0.0], dtype=np.float32), np.array([0, 1]), np.zeros(1, dtype=np.int32), -one[:1],
                     np.array([[0]]), None, 0, 1)
    assert neg.tolist() == [[0.0]] and not np.signbit(neg).any()


def _both(Qm, Dm, cand, lens, id_base):
    host = P.inverted(Dm) + P.query_rows(Qm)
    toff, pdoc, pw = host[:3]
    foff, fterm, fpos = F.forward_build(toff, pdoc, Dm.shape[0])
    assert (np.diff(foff) == np.count_nonzero(Dm, axis=1)).all()
    assert all((np.diff(fterm[foff[d]:foff[d + 1]]) > 0).all() for d in range(Dm.shape[0]))           # strictly ascending inside a row
    walk = F.row_walk(foff, fterm, pw[fpos], *host[3:], cand, lens, id_base, Dm.shape[0])
    chain = P.sparse_chain(*host, cand, lens, id_base, Dm.shape[0])
    return walk, chain


def test_the_row_walk_is_the_chain_byte_for_byte():
    Qm, Dm = P.sparse_corpus(3)
    toff, pdoc, _ = P.inverted(Dm)
    qoff, qterms, _ = P.query_rows(Qm)
    for W in (8, 65):
        cand, lens = P.sparse_candidates(50 + W, toff, pdoc, qoff, qterms, W, P.BIG_BASE)
        walk, chain = _both(Qm, Dm, cand, lens, P.BIG_BASE)
        assert walk.tobytes() == chain.tobytes() and np.isfinite(walk).any() and np.isinf(walk).any(), W


def test_the_long_row_case_holds_what_it_promises():
    Qm, Dm = F.long_row_corpus()
    assert Dm.shape == (F.LR_N, F.LR_V) and F.LR_V % 32 and Qm.shape[0] == F.LR_Q
    n = np.count_nonzero(Dm, axis=1)
    assert set(n.tolist()) == set(F.LR_LENS) and all(n[d] == F.LR_LENS[d % 11] for d in range(F.LR_N))
    assert {1, F.GROUP - 1, F.GROUP, F.GROUP + 1, 2 * F.GROUP - 1, 2 * F.GROUP, 2 * F.GROUP + 1} <= set(F.LR_LENS) and max(F.LR_LENS) > 40 * F.GROUP
    nq = np.count_nonzero(Qm, axis=1)
    assert nq[F.LR_TWIN_QUERY] == 700 and nq[F.LR_EMPTY_QUERY] == 0 and nq[F.LR_WIDE_QUERY] == F.LR_WIDE_TERMS and nq[F.LR_ORDER_QUERY] == 3
    assert (np.nonzero(Qm[F.LR_TWIN_QUERY])[0] == np.nonzero(Dm[F.LR_TWIN_DOC])[0]).all()
    for t in F.LR_SPECIAL:
        assert np.count_nonzero(Dm[:, t]) > 20 and np.count_nonzero(Qm[:, t]) >= 3, t
    cand, lens = F.long_row_candidates(5, 33, P.BIG_BASE)
    assert sorted(n[cand[0, 2:13] - P.BIG_BASE].tolist()) == sorted(F.LR_LENS) and lens[:4].tolist() == [33] * 4
    local = cand - P.BIG_BASE
    assert (cand < 0).any() and (local == F.LR_N).any() and (cand[:, 0] == P.BIG_BASE + F.LR_TWIN_DOC).all()
    walk, chain = _both(Qm, Dm, cand, lens, P.BIG_BASE)
    assert walk.tobytes() == chain.tobytes()
    # the order probe: 0.0 in term order; the same three products in another order give 1.0
    assert walk[F.LR_ORDER_QUERY, 1] == 0.0 and np.float32(np.float32(np.float32(1e8) + np.float32(-1e8)) + np.float32(1.0)) == 1.0
    # the twin: 700 shared terms; the empty query: +0.0 for every document of the shard
    assert walk[F.LR_TWIN_QUERY, 0] > 50 and (walk[F.LR_EMPTY_QUERY][np.isfinite(walk[F.LR_EMPTY_QUERY])] == 0).all()
    assert (walk[F.LR_WIDE_QUERY, 2:13] > 0).sum() >= 6                                                # the long rows meet the 5,000-term query


# ---- the shipped build ---------------------------------------------------------------------------------------------------------------
def test_the_forward_kernels_hold_everything_in_registers(tmp_path):
    """The report the compile left next to the object (fusion_amd/csrc/forward.res); if the objects predate it, the one source is compiled
    once more into a temporary directory -- never into the tree -- as tests/test_pairs_cpu.py does."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if "forward" not in res:
        import subprocess
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip("no forward.res next to the objects and no hipcc to make it: run `make -C fusion_amd/csrc` where ROCm is installed")
        flags = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()
        r = subprocess.run([hipcc, *flags, "-c", os.path.join(ROOT, "fusion_amd", "csrc", "forward.hip"), "-o", str(tmp_path / "forward.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        (tmp_path / "forward.res").write_text(r.stderr)
        res = kernel_resources.load(str(tmp_path))
    mine = {kernel_resources.short(n): r for n, r in res["forward"].items()}
    assert len(mine) == 3 and any("sparse_fwd_pairs_kernel" in n for n in mine) and sum("lexical_doc_scores_fwd_kernel" in n for n in mine) == 2, sorted(mine)
    for name, r in mine.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, f"{name}: {r['vgpr_spill']} spilled VGPRs, {r['scratch']} B/lane of scratch"
    # eight waves per SIMD keep 2 x 4 rows per lane group in flight everywhere: 64 VGPRs or fewer
    fwd = next(r for n, r in mine.items() if "sparse_fwd_pairs_kernel" in n)
    assert fwd["vgprs"] + fwd.get("agprs", 0) <= 64, fwd
