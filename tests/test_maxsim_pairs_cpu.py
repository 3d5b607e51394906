"""Candidate-list MaxSim without a GPU: the C entry's argument checks (reported before any HIP call), the type and shape errors of
ops.maxsim_pairs, the plain-Python restatement of the launch arithmetic against hand-checked cases (and the sweep's branch table), and
the shipped build's resource report for the new kernel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import maxsim_pairs_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def call(L, **kw):
    a = dict(Qtok=0x1000, Dtok=0x2000, Doff=0x3000, sumL=100, max_doc_len=512, Q=2, Lq=64, N=10, dim=128, cand=0x4000, ldc=8, cand_len=None,
             k=8, id_base=0, scores=0x5000, lds=8)
    a.update(kw)
    p = lambda v: None if not v else C.c_void_p(v)      # noqa: E731
    return L.fz_maxsim_pairs_f16(p(a["Qtok"]), p(a["Dtok"]), p(a["Doff"]), a["sumL"], a["max_doc_len"], a["Q"], a["Lq"], a["N"], a["dim"],
                                 p(a["cand"]), a["ldc"], p(a["cand_len"]), a["k"], a["id_base"], p(a["scores"]), a["lds"], None)


def test_abi_argument_validation_without_gpu():
    """Every refusal comes before the first HIP call, so the (fake, aligned) pointers are never touched."""
    from fusion_amd import _lib
    L = _lib.lib()
    assert "fz_maxsim_pairs_f16" in _lib.EXPORTS and L.fz_abi_version() == 20      # an additive entry: the ABI version stays
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    # null pointers where a non-empty tensor is needed
    for name in ("Qtok", "Doff", "cand", "scores"):
        assert call(L, **{name: 0}) == ARG, name
    assert call(L, Dtok=0) == ARG                          # sumL != 0 needs a token matrix
    # leading dimensions and negative sizes
    assert call(L, ldc=7) == ARG and call(L, lds=7) == ARG
    for name in ("Q", "N", "k"):
        assert call(L, **{name: -1}) == ARG, name
    assert call(L, Lq=0) == ARG and call(L, Lq=-64) == ARG
    assert call(L, sumL=-1) == ARG and call(L, max_doc_len=0) == ARG and call(L, max_doc_len=-5) == ARG
    # shapes outside what is built
    assert call(L, dim=64) == UNS and call(L, dim=256) == UNS
    for Lq in (16, 48, 96, 256):
        assert call(L, Lq=Lq) == UNS, Lq
    assert call(L, Qtok=0x1008) == UNS and call(L, Dtok=0x2004) == UNS
    assert call(L, max_doc_len=16385) == UNS
    # the order of fz_maxsim_f16: argument errors first, then unsupported shapes, then the empty batch, then sumL / max_doc_len
    assert call(L, dim=64, ldc=7) == ARG
    assert call(L, dim=64, Q=0) == UNS
    assert call(L, Q=0, max_doc_len=0) == OK and call(L, k=0, ldc=0, lds=0, max_doc_len=99999) == OK
    # nothing to do: no launch, null pointers welcome
    assert call(L, Q=0, Qtok=0, cand=0, scores=0, Doff=0) == OK
    assert call(L, k=0, ldc=0, lds=0, Qtok=0, cand=0, scores=0, Doff=0) == OK
    assert call(L, Q=0, Dtok=0, sumL=0) == OK


# ---- ops.maxsim_pairs: errors raised before anything reaches the device ----------------------------------------------------------------
def test_ops_type_and_shape_errors():
    from fusion_amd import ops
    Qtok, Dtok = torch.zeros((2, 64, 128), dtype=torch.float16), torch.zeros((10, 128), dtype=torch.float16)
    Doff, cand = torch.zeros(4, dtype=torch.int64), torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(TypeError, match="Qtok.*GPU"):
        ops.maxsim_pairs(Qtok, Dtok, Doff, cand)                 # CPU tensors: there is no CPU path
    with pytest.raises(TypeError):
        ops.maxsim_pairs(None, Dtok, Doff, cand)
    if not torch.cuda.is_available():
        return
    g = lambda t: t.cuda()      # noqa: E731
    Qtok, Dtok, Doff, cand = g(Qtok), g(Dtok), g(Doff), g(cand)
    for bad in (dict(Qtok=Qtok.float()), dict(Dtok=Dtok.float()), dict(Doff=Doff.int()), dict(cand=cand.int()),
                dict(cand_len=torch.zeros(2, dtype=torch.int64, device="cuda")), dict(out=torch.zeros((2, 5), dtype=torch.float64, device="cuda")),
                dict(cand=cand.cpu())):
        with pytest.raises(TypeError):
            ops.maxsim_pairs(**{**dict(Qtok=Qtok, Dtok=Dtok, Doff=Doff, cand=cand), **bad})
    for bad in (dict(Qtok=Qtok[0]), dict(Dtok=Dtok[:, :64]), dict(cand=cand[:1]), dict(cand=cand[0]),
                dict(cand_len=torch.zeros(3, dtype=torch.int32, device="cuda")), dict(out=torch.zeros((2, 6), device="cuda")),
                dict(max_doc_len=0), dict(Doff=Doff[:0])):
        with pytest.raises(ValueError):
            ops.maxsim_pairs(**{**dict(Qtok=Qtok, Dtok=Dtok, Doff=Doff, cand=cand), **bad})


# ---- the launch arithmetic, restated ---------------------------------------------------------------------------------------------
def test_launch_restatement_on_hand_checked_cases():
    slots = lambda k: [wv["slots"] for wv in P.pairs_plan(k)["waves"]]      # noqa: E731
    assert P.MP_SLICE == 128
    assert slots(1) == [[0], [], [], []]
    assert slots(2) == [[0], [1], [], []]
    assert slots(7) == [[0, 4], [1, 5], [2, 6], [3]]
    assert [len(s) for s in slots(64)] == [16] * 4 and [len(s) for s in slots(65)] == [17, 16, 16, 16]
    assert [len(s) for s in slots(100)] == [25] * 4
    assert [len(s) for s in slots(128)] == [32] * 4 and P.pairs_plan(128)["nslices"] == 1
    p = P.pairs_plan(130)
    assert p["nslices"] == 2 and [wv["slots"] for wv in p["waves"][4:]] == [[128], [129], [], []] and p["waves"][3]["slots"][-1] == 127
    assert P.pairs_plan(1000)["nslices"] == 8 and [len(wv["slots"]) for wv in P.pairs_plan(1000)["waves"][-4:]] == [26] * 4
    for k in (1, 2, 7, 64, 65, 100, 130, 1000):      # every slot is walked exactly once
        assert sorted(r for s in slots(k) for r in s) == list(range(k))
    # (row blocks loaded, last one partial) per round of four
    assert P.row_blocks(1) == [(1, True)] and P.row_blocks(16) == [(1, False)] and P.row_blocks(17) == [(2, True)]
    assert P.row_blocks(48) == [(3, False)] and P.row_blocks(64) == [(4, False)] and P.row_blocks(65) == [(4, False), (1, True)]
    assert P.row_blocks(70) == [(4, False), (1, True)] and P.row_blocks(100) == [(4, False), (3, True)]
    assert P.row_blocks(512) == [(4, False)] * 8 and P.row_blocks(511) == [(4, False)] * 7 + [(4, True)]
    # slots of one row
    st = P.slot_state([5, -1, 4, 15, 7, 5], 5, 5, [3, 0, 600], 512)
    assert st == [("doc", 0, 3), ("absent", "negative-id"), ("absent", "below-id_base"), ("absent", "past-N"), ("doc", 2, 512), ("absent", "past-cand_len")]
    big = 2 ** 33 + 5
    assert P.slot_state([big + 1, big - 1, 1], 3, big, [3, 0], 512) == [("doc", 1, 0), ("absent", "below-id_base"), ("absent", "below-id_base")]


def test_sweep_lands_on_every_branch():
    hit, by_k, by_m = P.sweep_branches()
    for k, claims in P.K_CLAIMS.items():
        assert set(claims) <= by_k[k], (k, sorted(map(str, set(claims) - by_k[k])))
    for m, claims in P.M_CLAIMS.items():
        assert set(claims) <= by_m[m], (m, sorted(map(str, set(claims) - by_m[m])))
    assert set(P.BRANCHES) <= hit, sorted(map(str, set(P.BRANCHES) - hit))
    assert set(P.KS) >= {1, 2, 7, 64, 65, 100} and set(P.QS) == {1, 2, 5, 9} and set(P.MAX_DOC_LENS) == {512, 33, 16, 1}
    assert len(P.LENS) == 39 and P.LENS[-1] > max(P.MAX_DOC_LENS) and all(L in P.LENS[::2] for L in P.M.EDGE_LENS + (0,))


def test_expectation_gathers_the_reference():
    ref = np.arange(12, dtype=np.float32).reshape(2, 6)
    cand = np.array([[3, 3, -1, 9, 2], [8, 4, 5, 6, 7]], dtype=np.int64)
    got = P.expected(ref, cand, [5, 3], 3)
    inf = -np.inf
    assert got.tolist() == [[0.0, 0.0, inf, inf, inf], [11.0, 7.0, 8.0, inf, inf]]


# ---- the shipped build ---------------------------------------------------------------------------------------------------------------
def test_the_pairs_kernel_holds_everything_in_registers(tmp_path):
    """The report the compile left next to the object (fusion_amd/csrc/rerank.res); if the objects predate it, the one source is compiled
    once more into a temporary directory -- never into the tree -- as tests/test_kernel_resources_cpu.py does."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if "rerank" not in res:
        import subprocess
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip("no rerank.res next to the objects and no hipcc to make it: run `make -C fusion_amd/csrc` where ROCm is installed")
        flags = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()
        r = subprocess.run([hipcc, *flags, "-c", os.path.join(ROOT, "fusion_amd", "csrc", "rerank.hip"), "-o", str(tmp_path / "rerank.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        (tmp_path / "rerank.res").write_text(r.stderr)
        res = kernel_resources.load(str(tmp_path))
    mine = {kernel_resources.short(n): r for n, r in res["rerank"].items() if "maxsim_pairs_kernel" in n}
    assert len(mine) == 3, sorted(mine)      # Lq = 32, 64, 128
    for name, r in mine.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, f"{name}: {r['vgpr_spill']} spilled VGPRs, {r['scratch']} B/lane of scratch"
