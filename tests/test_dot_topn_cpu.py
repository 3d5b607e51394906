"""dot_topn (the top-n selection in the probe GEMM's epilogue), host side (no GPU): the entries are exported under ABI 20 and declared in
the header, the workspace plan is monotone, every bad argument and every empty problem is settled before a HIP call, the kernels hold
their lists in registers, and fused=True refuses an nprobe the kernel does not take."""
import os
import sys

import pytest
import torch

from fusion_amd import _lib, ops

ERR, OK, UNSUP, WS = _lib.FZ_ERR_ARG, _lib.FZ_OK, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_ERR_WORKSPACE
one = 16   # any non-null, 16-byte aligned address: every call below is refused (or has nothing to do) before a pointer is touched
NEW = ("fz_dot_topn_max", "fz_dot_topn_workspace_bytes", "fz_dot_topn_f32")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def call(L, X=one, ldx=128, C=one, ldc=128, rows=200, K=300, d=128, n=4, out_s=one, out_i=one, ws=one, wsb=0):
    return L.fz_dot_topn_f32(X, ldx, C, ldc, rows, K, d, n, out_s, out_i, ws, wsb, None)


def test_exports_header_and_abi(L):
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.fz_abi_version() == _lib.ABI_VERSION == 20
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
    assert L.fz_dot_topn_max() >= 8 and ops.dot_topn_max() == L.fz_dot_topn_max()


def test_workspace_is_zero_for_empty_problems_and_never_shrinks(L):
    w = L.fz_dot_topn_workspace_bytes
    for rows, K, n in [(0, 300, 4), (200, 0, 4), (200, 300, 0), (-1, 300, 4), (200, -5, 4), (200, 300, -1)]:
        assert w(rows, K, n) == 0, (rows, K, n)
    assert w(1, 1, 1) > 0
    rows_axis = [1, 64, 127, 128, 129, 255, 256, 257, 383, 385, 1000, 8191, 65535, 65536, 65537, 70000, 1 << 20, 1 << 24]
    K_axis = [1, 127, 128, 129, 1000, 65535, 65536, 65537, 70001, 1 << 20]
    n_axis = list(range(1, L.fz_dot_topn_max() + 1))
    for K in K_axis:
        for n in (1, 8):
            sizes = [w(r, K, n) for r in rows_axis]
            assert sizes == sorted(sizes), ("rows", K, n, sizes)
    for r in rows_axis:
        for n in (1, 8):
            sizes = [w(r, K, n) for K in K_axis]
            assert sizes == sorted(sizes), ("K", r, n, sizes)
        for K in (1, 1000, 70001):
            sizes = [w(r, K, n) for n in n_axis]
            assert sizes == sorted(sizes), ("n", r, K, sizes)
    # at the production shape (65,536 token rows) a row's 4 lists of 8 (score, id) pairs
    assert w(65536, 65536, 8) <= 65536 * 4 * 8 * 8 + 4096


def test_bad_arguments_are_refused_before_any_hip_call(L):
    big = 1 << 40
    assert call(L, wsb=big, rows=-1) == ERR
    assert call(L, wsb=big, K=-1) == ERR
    assert call(L, wsb=big, d=0) == ERR
    assert call(L, wsb=big, d=-4) == ERR
    assert call(L, wsb=big, ldx=124) == ERR                     # ld < d
    assert call(L, wsb=big, ldc=64) == ERR
    assert call(L, wsb=big, n=0) == ERR
    assert call(L, wsb=big, n=-2) == ERR
    assert call(L, wsb=big, X=None) == ERR
    assert call(L, wsb=big, C=None) == ERR
    assert call(L, wsb=big, out_s=None) == ERR
    assert call(L, wsb=big, out_i=None) == ERR
    assert call(L, wsb=big, n=L.fz_dot_topn_max() + 1) == UNSUP
    assert call(L, wsb=big, d=126, ldx=128, ldc=128) == UNSUP   # the GEMM's alignment conditions
    assert call(L, wsb=big, ldx=130) == UNSUP
    assert call(L, wsb=big, ldc=129) == UNSUP
    assert call(L, wsb=big, X=one + 4) == UNSUP
    assert call(L, wsb=big, C=one + 8) == UNSUP
    need = L.fz_dot_topn_workspace_bytes(200, 300, 4)
    assert need > 0
    assert call(L, wsb=need - 1) == WS
    assert call(L, wsb=0) == WS
    assert call(L, ws=None, wsb=need) == WS


def test_nothing_to_do(L):
    assert call(L, rows=0, X=None, C=None, out_s=None, out_i=None, ws=None, wsb=0) == OK
    assert call(L, rows=0) == OK
    assert call(L, rows=0, K=0, C=None) == OK
    assert call(L, rows=0, n=0) == ERR                          # n is judged even when there are no rows


def test_the_kernels_hold_their_lists_in_registers(tmp_path):
    """The compiler's resource report of the shipped build (fusion_amd/csrc/score.res).  Where it is missing, the source is compiled into a
    temporary directory -- never into the tree -- and only a machine without hipcc skips."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if not res or "score" not in res:
        import subprocess
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip("no fusion_amd/csrc/score.res next to the objects and no hipcc to make it")
        flags = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()
        r = subprocess.run([hipcc, *flags, "-c", os.path.join(ROOT, "fusion_amd", "csrc", "score.hip"), "-o", str(tmp_path / "score.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        (tmp_path / "score.res").write_text(r.stderr)
        res = kernel_resources.load(str(tmp_path))
    assert "score" in res, sorted(res)
    flat = {kernel_resources.short(name): k for name, k in res["score"].items()}
    for name in ("dot_topn_kernel", "dot_topn_merge_kernel"):
        hits = [k for k in flat if k == name or k.startswith(name + "<")]
        assert hits, (name, sorted(flat))
        for k in hits:
            assert flat[k]["vgpr_spill"] == 0 and flat[k]["scratch"] == 0, (k, flat[k])
    assert len([k for k in flat if k.startswith("dot_topn_kernel")]) == 2      # whole and ragged k-tiles


def test_fused_true_refuses_an_nprobe_above_the_cap():
    """Decided from nprobe and the library's cap alone, before a tensor is looked at: CPU tensors do."""
    Qtok, C = torch.zeros((1, 4, 128), dtype=torch.float16), torch.zeros((16, 128), dtype=torch.float16)
    with pytest.raises(ValueError, match="dot_topn_max"):
        ops.centroid_probes(Qtok, C, ops.dot_topn_max() + 1, fused=True)
    with pytest.raises(TypeError):                               # within the cap the call goes on to its tensors: no CPU path
        ops.centroid_probes(Qtok, C, ops.dot_topn_max(), fused=True)
    assert ops.CENTROID_FUSED in (True, False)
