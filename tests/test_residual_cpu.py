"""The residual-compressed token index without a GPU: the numpy restatement of the code (residual_cases.py) against hand-checked cases,
the half-add equivalence the decompression rests on, the C entries' argument checks (reported before any HIP call), the errors of the
ops and of ShardedTokenIndex.compress raised before any device work, and the shipped build's resource report: the six instantiations of
the new rerank kernel hold everything in registers, and rerank.res still lists exactly the three kernels it listed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import residual_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", R.NBITS)
def test_pack_unpack_round_trip_and_layout(nbits):
    rng = np.random.default_rng(nbits)
    b = rng.integers(0, 1 << nbits, (37, 128)).astype(np.uint8)
    p = R.pack(b, nbits)
    assert p.shape == (37, 16 * nbits) and p.dtype == np.uint8
    assert np.array_equal(R.unpack(p, nbits), b)
    # one bucket set in one dimension: the byte and the bit field the layout names
    for dim in (0, 7, 8, 31, 32, 40, 127):
        one = np.zeros((1, 128), dtype=np.uint8)
        one[0, dim] = (1 << nbits) - 1
        s = int(np.nonzero(R.POS_DIM == dim)[0][0])
        assert 32 * ((s >> 3) & 3) + 8 * (s >> 5) + (s & 7) == dim
        per = 8 // nbits
        want = np.zeros(16 * nbits, dtype=np.uint8)
        want[s // per] = ((1 << nbits) - 1) << (nbits * (s % per))
        assert np.array_equal(R.pack(one, nbits)[0], want), dim
    # lane (row, group g) of the 16x16x32 A operand: dimensions 32 ks + 8 g + j are positions 32 g + 8 ks + j -- one aligned piece
    for g in range(4):
        for ks in range(4):
            assert R.POS_DIM[32 * g + 8 * ks: 32 * g + 8 * ks + 8].tolist() == list(range(32 * ks + 8 * g, 32 * ks + 8 * g + 8))
    assert R.POS_DIM[:8].tolist() == list(range(8)) and R.POS_DIM[8:16].tolist() == list(range(32, 40)) and R.POS_DIM[32:40].tolist() == list(range(8, 16))


def test_a_residual_on_a_cutoff_falls_in_the_lower_bucket():
    cut = np.array([-0.25, 0.0, 0.25], dtype=np.float32)
    r = np.array([-1.0, -0.25, np.nextafter(np.float32(-0.25), np.float32(1)), 0.0, 0.1, 0.25, np.nextafter(np.float32(0.25), np.float32(1)), np.inf, -np.inf, np.nan],
                 dtype=np.float32)
    assert R.bucket(r, cut).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 0, 0]
    finite = r[np.isfinite(r)]
    assert R.bucket(finite, cut).tolist() == torch.bucketize(torch.from_numpy(finite), torch.from_numpy(cut)).tolist()
    # equal cutoffs (a degenerate training sample) skip a bucket, nothing more
    assert R.bucket(np.array([0.0, 0.5], dtype=np.float32), np.array([0.0, 0.0, 0.0], dtype=np.float32)).tolist() == [0, 3]
    # compress / decompress on grid data with every residual exactly on a cutoff or a weight
    for nbits in R.NBITS:
        cutoffs, weights = R.grid_buckets(nbits)
        Cn = R.grid_centroids()
        codes = np.arange(16, dtype=np.int32)
        on_cut = (Cn[codes].astype(np.float32) + cutoffs[np.arange(128) % len(cutoffs)]).astype(np.float16)
        assert np.array_equal(on_cut.astype(np.float32) - Cn[codes].astype(np.float32), np.broadcast_to(cutoffs[np.arange(128) % len(cutoffs)], (16, 128)))
        got = R.unpack(R.compress(on_cut, codes, Cn, cutoffs, nbits), nbits)
        assert np.array_equal(got, np.broadcast_to(np.arange(128) % len(cutoffs), (16, 128)))      # the lower bucket
        on_w = (Cn[codes].astype(np.float32) + weights.astype(np.float32)[np.arange(128) % len(weights)]).astype(np.float16)
        p = R.compress(on_w, codes, Cn, cutoffs, nbits)
        assert np.array_equal(R.decompress(p, codes, Cn, weights, nbits), on_w)                    # a grid row survives the round trip


def test_half_add_equals_the_float32_sum_rounded_once():
    """float16(float32(a) + float32(b)) -- the kernel's v_pk_add_f16 by IEEE, numpy's and torch's half add in practice -- is the exact
    sum rounded once: the float32 sum of two float16 values is exact unless it needs more than 24 bits, and then double rounding cannot
    land on a float16 tie (checked here against the float64 sum, which is always exact, on pairs from all finite float16 patterns)."""
    rng = np.random.default_rng(16)
    a = rng.integers(0, 1 << 16, 1 << 20).astype(np.uint16).view(np.float16)
    b = rng.integers(0, 1 << 16, 1 << 20).astype(np.uint16).view(np.float16)
    ok = np.isfinite(a) & np.isfinite(b)
    a, b = a[ok], b[ok]
    # denormals, ties and cancellations by construction as well
    a = np.concatenate([a, np.array([6e-8, 6.1e-5, 1.0, 1.0, 2048.0, -1.0, 65504.0, 1024.0], dtype=np.float16)])
    b = np.concatenate([b, np.array([6e-8, -6e-8, 2 ** -11, 3 * 2 ** -11, 1.0, 1.0, 65504.0, 0.375], dtype=np.float16)])
    with np.errstate(over="ignore"):
        via32 = (a.astype(np.float32) + b.astype(np.float32)).astype(np.float16)
        exact = (a.astype(np.float64) + b.astype(np.float64)).astype(np.float16)
        half = a + b
    th = (torch.from_numpy(a) + torch.from_numpy(b)).numpy()
    for got in (via32, half, th):
        assert np.array_equal(got.view(np.uint16), exact.view(np.uint16))
    assert float(exact[-1]) == 1024.0      # a poison centroid + the largest grid weight rounds back to 1024


def test_trained_buckets_are_nested_and_ordered():
    rng = np.random.default_rng(5)
    r = rng.normal(0, 0.05, 40000).astype(np.float32)
    c2, w2 = R.train_buckets(r, 2)
    c4, w4 = R.train_buckets(r, 4)
    assert np.array_equal(c4[3::4], c2)                                  # the 16-bucket cutoffs contain the 4-bucket ones
    for c, w in ((c2, w2), (c4, w4)):
        assert (np.diff(c) >= 0).all() and (np.diff(w.astype(np.float32)) >= 0).all()
        assert (w[:-1].astype(np.float32) <= c).all() and (c <= w[1:].astype(np.float32)).all()
        counts = np.bincount(R.bucket(r, c), minlength=len(w))
        assert counts.min() >= len(r) // len(w) - 1 and counts.max() <= len(r) // len(w) + 1      # equal population
    # an empty bucket takes its lower cutoff, bucket 0 the upper one
    c, w = R.train_buckets(np.array([1.0] * 8, dtype=np.float32), 2)
    assert c.tolist() == [1.0, 1.0, 1.0] and w.tolist() == [1.0, 1.0, 1.0, 1.0]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _p(v):
    return None if not v else C.c_void_p(v)


def pairs(L, **kw):
    a = dict(Qtok=0x1000, packed=0x2000, codes=0x6000, C=0x7000, weights=0x8000, K=300, nbits=2, Doff=0x3000, sumL=100, max_doc_len=512, Q=2,
             Lq=64, N=10, dim=128, cand=0x4000, ldc=8, cand_len=None, k=8, id_base=0, scores=0x5000, lds=8)
    a.update(kw)
    return L.fz_maxsim_pairs_residual_f16(_p(a["Qtok"]), _p(a["packed"]), _p(a["codes"]), _p(a["C"]), _p(a["weights"]), a["K"], a["nbits"],
                                          _p(a["Doff"]), a["sumL"], a["max_doc_len"], a["Q"], a["Lq"], a["N"], a["dim"], _p(a["cand"]), a["ldc"],
                                          _p(a["cand_len"]), a["k"], a["id_base"], _p(a["scores"]), a["lds"], None)


def comp(L, **kw):
    a = dict(tok=0x1000, codes=0x2000, C=0x3000, cutoffs=0x4000, n=10, K=300, dim=128, nbits=2, packed=0x5000)
    a.update(kw)
    return L.fz_residual_compress_f16(_p(a["tok"]), _p(a["codes"]), _p(a["C"]), _p(a["cutoffs"]), a["n"], a["K"], a["dim"], a["nbits"], _p(a["packed"]), None)


def decomp(L, **kw):
    a = dict(packed=0x1000, codes=0x2000, C=0x3000, weights=0x4000, sumL=10, row_lo=0, row_hi=10, K=300, dim=128, nbits=2, out=0x5000)
    a.update(kw)
    return L.fz_residual_decompress_f16(_p(a["packed"]), _p(a["codes"]), _p(a["C"]), _p(a["weights"]), a["sumL"], a["row_lo"], a["row_hi"], a["K"],
                                        a["dim"], a["nbits"], _p(a["out"]), None)


def test_abi_argument_validation_without_gpu():
    """Every refusal comes before the first HIP call, so the (fake, aligned) pointers are never touched."""
    from fusion_amd import _lib
    L = _lib.lib()
    for name in ("fz_residual_compress_f16", "fz_residual_decompress_f16", "fz_maxsim_pairs_residual_f16"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.fz_abi_version() == 20      # additive entries: the ABI version stays
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    # ---- the rerank entry: fz_maxsim_pairs_f16's order
    for name in ("Qtok", "Doff", "cand", "scores", "C", "weights"):
        assert pairs(L, **{name: 0}) == ARG, name
    assert pairs(L, packed=0) == ARG and pairs(L, codes=0) == ARG      # sumL != 0 needs the rows
    assert pairs(L, ldc=7) == ARG and pairs(L, lds=7) == ARG
    for name in ("Q", "N", "k"):
        assert pairs(L, **{name: -1}) == ARG, name
    assert pairs(L, K=0) == ARG and pairs(L, K=-3) == ARG
    assert pairs(L, Lq=0) == ARG and pairs(L, Lq=-64) == ARG
    assert pairs(L, sumL=-1) == ARG and pairs(L, max_doc_len=0) == ARG
    assert pairs(L, dim=64) == UNS and pairs(L, dim=256) == UNS
    for nbits in (0, 1, 3, 8, -2):
        assert pairs(L, nbits=nbits) == UNS, nbits
    for Lq in (16, 48, 96, 256):
        assert pairs(L, Lq=Lq) == UNS, Lq
    assert pairs(L, Qtok=0x1008) == UNS and pairs(L, packed=0x2004) == UNS and pairs(L, C=0x7008) == UNS
    assert pairs(L, max_doc_len=16385) == UNS
    assert pairs(L, dim=64, ldc=7) == ARG and pairs(L, nbits=3, K=0) == ARG      # argument errors first
    assert pairs(L, dim=64, Q=0) == UNS and pairs(L, nbits=3, k=0, ldc=0, lds=0) == UNS
    assert pairs(L, Q=0, max_doc_len=0) == OK and pairs(L, k=0, ldc=0, lds=0, max_doc_len=99999) == OK
    assert pairs(L, Q=0, Qtok=0, cand=0, scores=0, Doff=0, C=0, weights=0) == OK      # empty batches carry null pointers
    assert pairs(L, k=0, ldc=0, lds=0, Qtok=0, cand=0, scores=0, Doff=0) == OK
    assert pairs(L, Q=0, packed=0, codes=0, sumL=0) == OK
    assert pairs(L, nbits=4, Q=0) == OK
    # ---- compress
    for name in ("tok", "codes", "C", "cutoffs", "packed"):
        assert comp(L, **{name: 0}) == ARG, name
    assert comp(L, n=-1) == ARG and comp(L, K=0) == ARG
    assert comp(L, dim=64) == UNS and comp(L, nbits=3) == UNS and comp(L, nbits=8) == UNS
    assert comp(L, tok=0x1008) == UNS and comp(L, C=0x3004) == UNS and comp(L, packed=0x5008) == UNS
    assert comp(L, dim=64, K=0) == ARG
    assert comp(L, n=0, tok=0, codes=0, packed=0) == OK and comp(L, n=0, nbits=4) == OK and comp(L, n=0, nbits=5) == UNS
    # ---- decompress
    for name in ("packed", "codes", "C", "weights", "out"):
        assert decomp(L, **{name: 0}) == ARG, name
    assert decomp(L, sumL=-1) == ARG and decomp(L, K=0) == ARG
    assert decomp(L, row_lo=-1) == ARG and decomp(L, row_lo=5, row_hi=4) == ARG and decomp(L, row_hi=11) == ARG
    assert decomp(L, dim=64) == UNS and decomp(L, nbits=1) == UNS
    assert decomp(L, packed=0x1004) == UNS and decomp(L, C=0x3008) == UNS and decomp(L, out=0x5004) == UNS
    assert decomp(L, row_lo=4, row_hi=4, packed=0, codes=0, out=0) == OK and decomp(L, sumL=0, row_hi=0, packed=0, codes=0, out=0) == OK


# ---- ops and the index: errors raised before anything reaches the device ---------------------------------------------------------------
def test_ops_have_no_cpu_path():
    from fusion_amd import ops
    tok, Cn, codes = torch.zeros((10, 128), dtype=torch.float16), torch.zeros((4, 128), dtype=torch.float16), torch.zeros(10, dtype=torch.int32)
    cut, w = torch.zeros(3), torch.zeros(4, dtype=torch.float16)
    packed = torch.zeros((10, 32), dtype=torch.uint8)
    Qtok, Doff, cand = torch.zeros((2, 64, 128), dtype=torch.float16), torch.zeros(4, dtype=torch.int64), torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(TypeError, match="tokens.*GPU"):
        ops.residual_buckets(tok, Cn, codes)
    with pytest.raises(TypeError, match="tokens.*GPU"):
        ops.residual_compress(tok, codes, Cn, cut)
    with pytest.raises(TypeError, match="packed.*GPU"):
        ops.residual_decompress(packed, codes, Cn, w)
    with pytest.raises(TypeError, match="Qtok.*GPU"):
        ops.maxsim_pairs_residual(Qtok, packed, codes, Cn, w, Doff, cand)
    with pytest.raises(TypeError):
        ops.maxsim_pairs_residual(None, packed, codes, Cn, w, Doff, cand)
    for nbits in (0, 1, 3, 8):
        with pytest.raises(ValueError, match="nbits"):
            ops.residual_compress(tok, codes, Cn, cut, nbits=nbits)
        with pytest.raises(ValueError, match="nbits"):
            ops.residual_buckets(tok, Cn, codes, nbits=nbits)


def test_compress_needs_a_centroid_index():
    from fusion_amd.distributed import ShardedTokenIndex
    index = ShardedTokenIndex(torch.zeros((10, 128), dtype=torch.float16), torch.tensor([0, 4, 10]), 0)      # CPU tensors: nothing may touch them
    with pytest.raises(ValueError, match="build_centroids"):
        index.compress()
    with pytest.raises(ValueError, match="build_centroids"):
        index.compress(nbits=4, cutoffs=torch.zeros(15), weights=torch.zeros(16, dtype=torch.float16))
    assert index.Dtok is not None and index.packed is None
    assert index.memory_bytes() == dict(tokens=10 * 256, codes=0, packed=0, candidates=0, total=10 * 256)
    with pytest.raises(ValueError, match="not compressed"):
        index.decompressed()


# ---- the shipped build ---------------------------------------------------------------------------------------------------------------
FLAGS = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()


def _report(tmp_path, name):
    """The report the compile left next to the object (fusion_amd/csrc/<name>.res); if it is missing, the one source is compiled once more
    into a temporary directory -- never into the tree -- as tests/test_maxsim_pairs_cpu.py does."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if name not in res:
        import subprocess
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip(f"no {name}.res next to the objects and no hipcc to make it: run `make -C fusion_amd/csrc` where ROCm is installed")
        r = subprocess.run([hipcc, *FLAGS, "-c", os.path.join(ROOT, "fusion_amd", "csrc", name + ".hip"), "-o", str(tmp_path / (name + ".o"))],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        (tmp_path / (name + ".res")).write_text(r.stderr)
        res = kernel_resources.load(str(tmp_path))
    return {kernel_resources.short(n): r for n, r in res[name].items()}


def test_the_residual_kernels_hold_everything_in_registers(tmp_path):
    rep = _report(tmp_path, "rerank_residual")
    mine = {n: r for n, r in rep.items() if "maxsim_residual_kernel" in n}
    assert len(mine) == 6, sorted(mine)      # Lq = 32, 64, 128 x nbits = 2, 4
    assert len(rep) == 10, sorted(rep)       # + compress and decompress, two widths each
    for name, r in rep.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, f"{name}: {r['vgpr_spill']} spilled VGPRs, {r['scratch']} B/lane of scratch"
    assert not any("maxsim_pairs_kernel" in n for n in rep)      # the uncompressed kernel lives in rerank.hip alone


def test_the_residual_kernels_keep_their_registers_and_occupancy(tmp_path):
    """The six kernels' VGPRs and waves per SIMD as recorded (DESIGN.md 'One walk, two storages'; the nbits = 4 figures are the ones
    profiles/r23_colbert_residual_shared_walk.json was measured with).  Their walk is csrc/maxsim_pairs.h, shared with rerank.hip: an
    edit there that moves a schedule fails here first, and is then due a measurement, not a new number."""
    rep = _report(tmp_path, "rerank_residual")
    by = {tuple(int(x) for x in n.split("<")[1].split(">")[0].split(",")): r for n, r in rep.items() if "maxsim_residual_kernel" in n}
    assert sorted(by) == [(ncb, nbits) for ncb in (2, 4, 8) for nbits in (2, 4)], sorted(by)
    assert [by[n, 2]["vgprs"] for n in (2, 4, 8)] == [120, 162, 240] and [by[n, 2]["occupancy"] for n in (2, 4, 8)] == [4, 3, 2]
    assert [by[n, 4]["vgprs"] for n in (2, 4, 8)] == [152, 168, 240] and [by[n, 4]["occupancy"] for n in (2, 4, 8)] == [3, 3, 2]


def test_the_uncompressed_rerank_kernels_are_unchanged(tmp_path):
    """The walk rerank.hip shares with the compressed path (csrc/maxsim_pairs.h) costs the plain kernels nothing: the report lists the
    three kernels it listed, with the registers and occupancy they had when the walk was theirs alone (Lq = 32 / 64 / 128: 106 / 168 /
    250 VGPRs, 4 / 3 / 2 waves per SIMD)."""
    rep = _report(tmp_path, "rerank")
    assert len(rep) == 3 and all("maxsim_pairs_kernel" in n for n in rep), sorted(rep)
    by_ncb = {int(n.split("<")[1].split(">")[0]): r for n, r in rep.items()}
    assert sorted(by_ncb) == [2, 4, 8]
    assert [by_ncb[n]["occupancy"] for n in (2, 4, 8)] == [4, 3, 2]
    assert [by_ncb[n]["vgprs"] for n in (2, 4, 8)] == [106, 168, 250]
    for r in by_ncb.values():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0
