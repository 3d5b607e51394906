"""ColBERT candidate stage, host side (no GPU): the new entry points are exported under ABI 20 and reject bad arguments before any HIP
call, ops.centroid_index on CPU tensors equals a brute-force set construction, the numpy restatement the GPU tests compare against equals
the formula pair by pair, and the new kernels hold their state in registers."""
import os
import sys

import numpy as np
import pytest
import torch

import centroid_cases as CC
from fusion_amd import _lib, ops

ERR, OK = _lib.FZ_ERR_ARG, _lib.FZ_OK
one = 16   # any non-null address: every call below is refused (or has nothing to do) before a pointer is touched
NEW = ("fz_centroid_slice_docs", "fz_centroid_slice_offsets", "fz_centroid_scores_range_f32", "fz_centroid_scores_filter_f32")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def G(L):
    return L.fz_centroid_slice_docs()


def rng_call(L, G, Q=1, Lq=4, nprobe=2, N=None, K=9, lo=0, hi=None, scores=one, lds=None, coff=one, pc=one, ps=one):
    N = 3 * G if N is None else N
    hi = N if hi is None else hi
    lds = hi - lo if lds is None else lds
    return L.fz_centroid_scores_range_f32(coff, one, None, pc, ps, Q, Lq, nprobe, N, K, lo, hi, scores, lds, None)


def filt_call(L, G, Q=1, Lq=4, nprobe=2, N=None, K=9, lo=0, hi=None, cap=64, tau=one, cs=one, ci=one, cl=one, ov=one, coff=one, pc=one, ps=one):
    N = 3 * G if N is None else N
    hi = N if hi is None else hi
    return L.fz_centroid_scores_filter_f32(coff, one, None, pc, ps, Q, Lq, nprobe, N, K, lo, hi, 3 << 31, tau, cs, ci, cl, cap, ov, None)


def test_exports_and_abi(L, G):
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.fz_abi_version() == _lib.ABI_VERSION == 20
    assert G == ops.centroid_slice_docs() and G > 0 and G % 64 == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fusion_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name


def test_range_entry_rejects_bad_arguments(L, G):
    assert rng_call(L, G, coff=None) == ERR
    assert rng_call(L, G, pc=None) == ERR
    assert rng_call(L, G, ps=None) == ERR
    assert rng_call(L, G, scores=None) == ERR
    assert rng_call(L, G, Q=-1) == ERR
    assert rng_call(L, G, N=-1, hi=0) == ERR
    assert rng_call(L, G, K=-1) == ERR
    assert rng_call(L, G, Lq=0) == ERR
    assert rng_call(L, G, Lq=-2) == ERR
    assert rng_call(L, G, nprobe=0) == ERR
    assert rng_call(L, G, nprobe=-1) == ERR
    assert rng_call(L, G, Lq=1 << 20, nprobe=1 << 12) == ERR     # Lq * nprobe beyond int32
    assert rng_call(L, G, lo=1) == ERR                           # doc_lo off the slice grain
    assert rng_call(L, G, lo=G + 64, hi=2 * G) == ERR
    assert rng_call(L, G, lo=0, hi=G + 5) == ERR                 # doc_hi neither a whole slice nor N
    assert rng_call(L, G, hi=3 * G + 1) == ERR                   # doc_hi > N
    assert rng_call(L, G, lo=2 * G, hi=G) == ERR                 # doc_hi < doc_lo
    assert rng_call(L, G, lo=-G, hi=G) == ERR
    assert rng_call(L, G, lds=3 * G - 1) == ERR                  # lds < doc_hi - doc_lo
    assert rng_call(L, G, lo=G, hi=2 * G, lds=G - 1) == ERR


def test_range_entry_nothing_to_do(L, G):
    assert rng_call(L, G, lo=G, hi=G, scores=None, coff=None, pc=None, ps=None) == OK    # empty range
    assert rng_call(L, G, lo=3 * G, hi=3 * G) == OK
    assert rng_call(L, G, Q=0, scores=None, coff=None, pc=None, ps=None) == OK          # no queries
    assert rng_call(L, G, N=0, hi=0, lds=0) == OK


def test_filter_entry_rejects_bad_arguments(L, G):
    for name in ("tau", "cs", "ci", "cl", "ov", "coff", "pc", "ps"):
        assert filt_call(L, G, **{name: None}) == ERR, name
    assert filt_call(L, G, cap=0) == ERR
    assert filt_call(L, G, cap=-3) == ERR
    assert filt_call(L, G, cap=0, lo=G, hi=G) == ERR             # cap is checked even when there is nothing to score
    assert filt_call(L, G, lo=100) == ERR
    assert filt_call(L, G, lo=G, hi=2 * G - 1) == ERR
    assert filt_call(L, G, hi=3 * G + 1) == ERR
    assert filt_call(L, G, N=-1, hi=0) == ERR
    assert filt_call(L, G, Q=-1) == ERR
    assert filt_call(L, G, Lq=0) == ERR
    assert filt_call(L, G, nprobe=0) == ERR
    assert filt_call(L, G, K=-1) == ERR


def test_filter_entry_nothing_to_do(L, G):
    assert filt_call(L, G, lo=2 * G, hi=2 * G, tau=None, cs=None, ci=None, cl=None, ov=None) == OK
    assert filt_call(L, G, Q=0, tau=None, cs=None, ci=None, cl=None, ov=None) == OK
    assert filt_call(L, G, N=0, hi=0) == OK


def test_slice_offsets_entry(L):
    assert L.fz_centroid_slice_offsets(one, one, -1, 5, one, None) == ERR
    assert L.fz_centroid_slice_offsets(one, one, 4, -5, one, None) == ERR
    assert L.fz_centroid_slice_offsets(None, one, 4, 5, one, None) == ERR
    assert L.fz_centroid_slice_offsets(one, one, 4, 5, None, None) == ERR
    assert L.fz_centroid_slice_offsets(None, None, 0, 5, None, None) == OK


def test_centroid_index_on_cpu_tensors_is_the_set_construction():
    rng = np.random.default_rng(3)
    K = 23
    lens = rng.integers(1, 12, 60)
    lens[[0, 17, 59]] = 0                                        # empty documents, the first and the last among them
    Doff = CC.doc_offsets(lens)
    codes = rng.integers(0, K, int(Doff[-1])).astype(np.int32)
    codes[codes == 11] = 12                                      # a centroid no token carries
    a = int(Doff[5])
    codes[a: a + int(lens[5])] = 4                               # a document with one repeated code: listed once
    coff, cdoc, doc_codes = CC.index_ref(codes, Doff, K)
    idx = ops.centroid_index(torch.from_numpy(codes), torch.from_numpy(Doff), K)
    assert idx.slice_off is None and idx.N == 60 and idx.K == K
    assert idx.coff.dtype == torch.int64 and idx.cdoc.dtype == torch.int32
    assert np.array_equal(idx.coff.numpy(), coff) and np.array_equal(idx.cdoc.numpy(), cdoc)
    assert coff[12] == coff[11] and lens[5] > 1 and list(cdoc[coff[4]: coff[5]]).count(5) == 1
    assert not any(d in (0, 17, 59) for d in cdoc)
    for c in range(K):
        seg = cdoc[coff[c]: coff[c + 1]]
        assert np.all(np.diff(seg) > 0)
    empty = ops.centroid_index(torch.zeros(0, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), 5)
    assert empty.N == 3 and empty.cdoc.numel() == 0 and empty.coff.tolist() == [0] * 6
    with pytest.raises(ValueError):
        ops.centroid_index(torch.tensor([0, 7], dtype=torch.int32), torch.tensor([0, 2]), 5)      # a code beyond K
    with pytest.raises(ValueError):
        ops.centroid_index(torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0, 1]), 5)      # Doff does not cover the rows


@pytest.mark.parametrize("Lq,nprobe", [(1, 1), (5, 3), (7, 9)])
def test_restatement_equals_the_formula_pair_by_pair(Lq, nprobe):
    rng = np.random.default_rng(100 * Lq + nprobe)
    K, N, Q = 12, 40, 4
    lens = rng.integers(0, 9, N)
    Doff = CC.doc_offsets(lens)
    codes = rng.integers(1, K, int(Doff[-1])).astype(np.int32)   # centroid 0: an empty list
    coff, cdoc, doc_codes = CC.index_ref(codes, Doff, K)
    pc, ps = CC.random_probes(rng, Q, Lq, nprobe, K)
    ps[1] = -np.abs(ps[1]) - np.float32(0.125)
    pc[1, 0] = codes[0]                                          # a centroid some document carries, with a negative score
    ps[2] = np.round(ps[2] * 2) / 2
    if nprobe > 1:
        pc[3, 1::nprobe] = -1
    got = CC.approx_plane(coff, cdoc, pc, ps, Lq, nprobe, N)
    want = CC.approx_dense(doc_codes, pc, ps, Lq, nprobe)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert (got[1] < 0).any() and (got[:, lens == 0] == 0).all()
    s, i = CC.topk_ref(got, N + 3)
    assert (i[:, N:] == -1).all() and np.isneginf(s[:, N:]).all() and all(sorted(r[:N].tolist()) == list(range(N)) for r in i)
    for q in range(Q):
        assert all(s[q, r] > s[q, r + 1] or (s[q, r] == s[q, r + 1] and i[q, r] < i[q, r + 1]) for r in range(N - 1))


def test_search_defaults_and_their_errors():
    from fusion_amd.distributed import ShardedTokenIndex
    assert ShardedTokenIndex.search_defaults(10) == (1, 256)
    assert ShardedTokenIndex.search_defaults(100) == (2, 400)
    assert ShardedTokenIndex.search_defaults(1000) == (4, 3584)
    assert ShardedTokenIndex.search_defaults(5000) == (4, 5000)
    idx = ShardedTokenIndex(torch.zeros((0, 128), dtype=torch.float16), torch.zeros(1, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="centroid"):
        idx.search(torch.zeros((1, 4, 128), dtype=torch.float16), k=10)
    idx.candidates, idx.centroids = object(), object()
    with pytest.raises(ValueError, match="ncand"):
        idx.search(torch.zeros((1, 4, 128), dtype=torch.float16), k=300, ncand=200)


def test_the_centroid_kernels_hold_their_state_in_registers(tmp_path):
    """The compiler's resource report of the shipped build (fusion_amd/csrc/centroid.res).  Where it is missing, the source is compiled
    into a temporary directory -- never into the tree -- and only a machine without hipcc skips."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if not res or "centroid" not in res:
        import subprocess
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip("no fusion_amd/csrc/centroid.res next to the objects and no hipcc to make it")
        flags = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()
        r = subprocess.run([hipcc, *flags, "-c", os.path.join(root, "fusion_amd", "csrc", "centroid.hip"), "-o", str(tmp_path / "centroid.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        (tmp_path / "centroid.res").write_text(r.stderr)
        res = kernel_resources.load(str(tmp_path))
    assert "centroid" in res, sorted(res)
    flat = {kernel_resources.short(name): k for name, k in res["centroid"].items()}
    for name in ("centroid_scores_kernel", "centroid_scores_filter_kernel"):
        assert name in flat, (name, sorted(flat))
        assert flat[name]["vgpr_spill"] == 0 and flat[name]["scratch"] == 0, (name, flat[name])
