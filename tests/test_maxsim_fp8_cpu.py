"""e4m3 MaxSim without a GPU: the reference quantiser of maxsim_fp8_cases.py against torch's float8_e4m3fn cast on every float16
pattern (and its saturation, NaN and tie rules pinned by hand), the exactness claim of the grid inputs, the case table against the
branches it must reach, the C entry points' argument checks (reported before any HIP call), the errors ops raises before anything
reaches the device, and the shipped build's resource report for csrc/maxsim8.hip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import maxsim_fp8_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fz_quantize_e4m3_f16", "fz_maxsim_e4m3")


# ---- the reference quantiser -----------------------------------------------------------------------------------------------------------
def test_table_is_torchs_e4m3fn():
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(t, F.TABLE, equal_nan=True)
    assert np.isnan(F.TABLE[[0x7f, 0xff]]).all() and np.isfinite(np.delete(F.TABLE, [0x7f, 0xff])).all()
    assert F.TABLE[0x7e] == 448 and F.TABLE[0xfe] == -448 and F.TABLE[0x01] == 2.0 ** -9 and np.signbit(F.TABLE[0x80]) and F.TABLE[0x80] == 0


@pytest.mark.parametrize("e", [0, 8, -8, 15, 3, -3])
def test_reference_quantiser_equals_torchs_cast_on_every_float16(e):
    x = F.all_f16_patterns()
    y = torch.from_numpy(x).to(torch.float32) * (2.0 ** e)                   # exact: float32 holds every float16 times 2^[-8, 15]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(y.to(torch.float64).numpy(), x.astype(np.float64) * 2.0 ** e, equal_nan=True)
    ok = (~torch.isnan(y) & (y.abs() <= 448)).numpy()                         # torch's cast does not saturate: above 448 it gives NaN
    assert ok.sum() > 17000                                                   # (at 2^15: everything up to 448 * 2^-15, 17,922 patterns)
    got = F.quantize_ref(x, e)
    exp = y.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(got[ok], exp[ok])


def test_reference_quantiser_saturation_nan_ties_and_signs():
    q = F.quantize_ref
    assert q([448.0, 449.0, 463.9, 464.0, 464.1, 480.0, 512.0, 65504.0, np.inf]).tolist() == [0x7e] * 9
    assert q([-448.0, -464.0, -1e9, -np.inf]).tolist() == [0xfe] * 4
    assert q([np.nan, -np.nan]).tolist() == [0x7f, 0xff]
    assert q([0.0, -0.0]).tolist() == [0x00, 0x80]
    s = 2.0 ** -9                                                             # subnormal step; ties go to the even code
    assert q([0.5 * s, 0.5001 * s, 1.5 * s, 2.5 * s, 7.5 * s, 7.4 * s, -0.5 * s, -1.5 * s]).tolist() == [0, 1, 2, 2, 8, 7, 0x80, 0x82]
    assert q([1.0, 1.0625, 1.1875, 1.125, 416.0, 432.0, 240.0]).tolist() == [0x38, 0x38, 0x3a, 0x39, 0x7d, 0x7e, 0x77]
    assert q([1.0, 2.0 ** -14], 8).tolist() == [0x78, 0x08] and q([65504.0], -8).tolist() == [F.quantize_ref([65504.0 / 256])[0]]
    # 2^15 saturates everything from 2^-6.2 up; 2^-8 flushes the float16 subnormals and more
    x = F.all_f16_patterns()
    x = x[~np.isnan(x)]
    b = q(x, 15)
    big = np.abs(x.astype(np.float64)) * 2.0 ** 15 > 464
    assert big.sum() > 30000 and set((b[big] & 0x7f).tolist()) == {0x7e}
    assert np.array_equal(b[big] >> 7, np.signbit(x[big]).astype(np.uint8))
    tiny = np.abs(x.astype(np.float64)) * 2.0 ** -8 < 2.0 ** -10
    assert tiny.sum() > 20000 and not (q(x, -8)[tiny] & 0x7f).any()


def test_dequantize_inverts_quantize_on_the_grid():
    b = np.delete(np.arange(256, dtype=np.uint8), [0x7f, 0xff])
    for e in (0, 8, -8, 15):
        assert np.array_equal(F.quantize_ref(F.dequantize_ref(b, e), e), b)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_grid_case_is_exact_in_float32_and_in_e4m3(case):
    """float32(ref) == ref, every value survives e4m3, clean documents stay below one leaked row, guards carry the poison."""
    Q8, D8, Doff = F.bytes_of(case)
    ref = F.reference(case)
    F.exact_f32(ref)
    assert np.abs(ref).max() < 2 ** 19
    if case.guards:
        lens = np.asarray(case.lens)
        clean, guard = ref[:, 0::2], ref[:, 1::2]
        assert np.all(clean <= 480 * case.Lq)
        assert np.all(guard[:, lens[1::2] > 0] >= (3584 - 480) * case.Lq)
    b = F.branches_of(case)
    assert set(case.claims) and set(case.claims) <= b, sorted(map(str, set(case.claims) - b))


def test_case_table_reaches_what_it_must():
    hit = set().union(*(F.branches_of(c) for c in F.CASES))
    assert set(F.BRANCHES) <= hit, sorted(map(str, set(F.BRANCHES) - hit))
    R = F.REQUIRED
    assert {c.Lq for c in F.CASES} == set(R["Lq"])
    for Lq in (32, 64):
        assert {h[2] for h in hit if h[:2] == ("load", Lq)} == set(R["loads"])
    assert any((c.Lq, c.Q) == R["Q195"] for c in F.CASES)
    for Lq in R["Lq"]:
        eff = {min(L, c.max_doc_len) for c in F.CASES if c.Lq == Lq for L in c.lens}
        assert set(R["lens"]) <= eff and max(eff) > R["longer_than_ring"]
        assert any(L > c.max_doc_len for c in F.CASES if c.Lq == Lq for L in c.lens)
        assert ("truncated-last", Lq) in hit and ("end", Lq, "Doff[0]>0") in hit
        assert set(R["N"]) <= {len(c.lens) for c in F.CASES if c.Lq == Lq}
        assert {h[2] for h in hit if h[:2] == ("tiles", Lq)} >= {9, 12, 13, 16, 17}                     # past the ring of 8
        assert {h[3] for h in hit if h[:2] == ("docs_per_wg", Lq)} >= {32, 30, 16, 1}
    assert max(len(c.lens) for c in F.CASES) <= R["max_docs"]
    assert len(F.DESCALE_CASES) == 4 and {c.Lq for c in F.DESCALE_CASES} == set(R["Lq"])


def test_quarter_tokens_quantise_without_loss():
    for c in F.DESCALE_CASES:
        Qh, Dh, Doff = F.quarter_tokens(c)
        Qv, Dv, _ = F.values(c)
        assert np.abs(Qh).max() <= 1 and np.abs(Dh[Dh != np.float16(1.75)]).max() <= 1
        for h, v, e in ((Qh, Qv, 8), (Dh, Dv, 8), (Qh, Qv, 6)):
            b = F.quantize_ref(h, e)
            assert np.array_equal(F.dequantize_ref(b, e), h.astype(np.float64))
        assert np.array_equal(F.dequantize_ref(F.quantize_ref(Dh, 8), 0), np.where(Dv == F.POISON8, Dv, Dv * 64))
        F.exact_f32(F.maxsim_ref(Qh, Dh, Doff, c.max_doc_len))


def test_special_bytes_mean_what_the_gpu_test_says():
    Q8, D8, Doff = F.special_bytes()
    Qv, Dv = F.dequantize_ref(Q8), F.dequantize_ref(D8)
    ref = F.maxsim_ref(Qv, Dv, Doff, 512)
    pinned = F.maxsim_fmax_ref(Qv, Dv, Doff)
    assert np.isnan(ref[:, 1]).all() and np.isfinite(pinned[:, 1]).all()            # one NaN row: the formula propagates, fmax skips
    assert np.isnan(ref[:, 2]).all() and np.isneginf(pinned[:, 2]).all()            # every row NaN: the empty maximum per query token
    assert np.abs(Dv[int(Doff[3]): int(Doff[4])]).max() == 448 and np.abs(pinned[:, 3]).max() > 448 * 32
    assert not pinned[:, 4].any()
    for d in (0, 3, 5):
        assert np.array_equal(ref[:, d], pinned[:, d])
    finite = pinned[np.isfinite(pinned)]
    assert np.array_equal(finite.astype(np.float32).astype(np.float64), finite)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def _p(v):
    return None if not v else C.c_void_p(v)


def call(L, **kw):
    a = dict(Qtok=0x1000, Dtok=0x2000, Doff=0x3000, sumL=100, max_doc_len=512, Q=2, Lq=64, N=10, dim=128, descale=16, scores=0x5000, lds=16)
    a.update(kw)
    return L.fz_maxsim_e4m3(_p(a["Qtok"]), _p(a["Dtok"]), _p(a["Doff"]), a["sumL"], a["max_doc_len"], a["Q"], a["Lq"], a["N"], a["dim"],
                            a["descale"], _p(a["scores"]), a["lds"], None)


def test_abi_argument_validation_without_gpu():
    """Every refusal comes before the first HIP call, so the (fake, aligned) pointers are never touched."""
    from fusion_amd import _lib
    L = _lib.lib()
    assert set(NEW) <= set(_lib.EXPORTS) and all(hasattr(L, n) for n in NEW) and L.fz_abi_version() == 20 == _lib.ABI_VERSION   # additive entries
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    for name in ("Qtok", "Doff", "scores"):
        assert call(L, **{name: 0}) == ARG, name
    assert call(L, Dtok=0) == ARG                          # sumL != 0 needs a token matrix
    assert call(L, lds=9) == ARG
    for name in ("Q", "N"):
        assert call(L, **{name: -1}) == ARG, name
    assert call(L, Lq=0) == ARG and call(L, Lq=-64) == ARG
    assert call(L, sumL=-1) == ARG and call(L, max_doc_len=0) == ARG and call(L, max_doc_len=-5) == ARG
    assert call(L, descale=33) == ARG and call(L, descale=-33) == ARG
    assert call(L, dim=64) == UNS and call(L, dim=256) == UNS
    for Lq in (16, 48, 96, 256):
        assert call(L, Lq=Lq) == UNS, Lq
    assert call(L, Qtok=0x1008) == UNS and call(L, Dtok=0x2004) == UNS and call(L, Dtok=0x2001) == UNS
    assert call(L, max_doc_len=16385) == UNS
    # fz_maxsim_f16's order: argument errors first, then unsupported shapes, then the empty batch, then sumL / max_doc_len
    assert call(L, dim=64, lds=9) == ARG
    assert call(L, dim=64, Q=0) == UNS
    assert call(L, Q=0, max_doc_len=0) == OK and call(L, N=0, lds=0, max_doc_len=99999) == OK
    assert call(L, Q=0, Qtok=0, scores=0, Doff=0) == OK and call(L, Q=0, Dtok=0, sumL=0) == OK
    # the quantiser
    quant = lambda src=0x1000, n=64, e=8, dst=0x2000: L.fz_quantize_e4m3_f16(_p(src), n, e, _p(dst), None)      # noqa: E731
    for e in (-9, 16, 127, -128):
        assert quant(e=e) == ARG, e
    assert quant(n=-1) == ARG and quant(src=0) == ARG and quant(dst=0) == ARG
    assert quant(src=0x1001) == UNS
    assert quant(n=0) == OK and quant(n=0, src=0, dst=0) == OK and quant(n=0, e=-8) == OK and quant(n=0, e=15) == OK
    assert quant(n=0, e=16) == ARG


def test_ops_type_and_shape_errors():
    from fusion_amd import ops
    Q8, D8 = torch.zeros((2, 64, 128), dtype=torch.uint8), torch.zeros((10, 128), dtype=torch.uint8)
    Doff = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError, match="Q8.*GPU"):
        ops.maxsim_e4m3(Q8, D8, Doff)                      # CPU tensors: there is no CPU path
    with pytest.raises(TypeError, match="GPU"):
        ops.quantize_e4m3(torch.zeros(8, dtype=torch.float16))
    with pytest.raises(TypeError):
        ops.maxsim_e4m3(None, D8, Doff)
    if not torch.cuda.is_available():
        return
    Q8, D8, Doff = Q8.cuda(), D8.cuda(), Doff.cuda()
    for bad in (dict(Q8=Q8.to(torch.int8)), dict(D8=D8.half()), dict(Doff=Doff.int()), dict(out=torch.zeros((2, 3), dtype=torch.float64, device="cuda"))):
        with pytest.raises(TypeError):
            ops.maxsim_e4m3(**{**dict(Q8=Q8, D8=D8, Doff=Doff), **bad})
    for bad in (dict(Q8=Q8[0]), dict(D8=D8[:, :64]), dict(out=torch.zeros((2, 4), device="cuda")), dict(max_doc_len=0), dict(Doff=Doff[:0]),
                dict(q_exp=16), dict(d_exp=-9), dict(q_exp=8.0)):
        with pytest.raises(ValueError):
            ops.maxsim_e4m3(**{**dict(Q8=Q8, D8=D8, Doff=Doff), **bad})
    with pytest.raises(TypeError):
        ops.quantize_e4m3(Q8)
    for e in (-9, 16):
        with pytest.raises(ValueError):
            ops.quantize_e4m3(D8.half(), e)


def test_ops_table_is_the_reference_table():
    from fusion_amd import ops
    assert np.array_equal(ops.e4m3_table().astype(np.float64), F.TABLE, equal_nan=True)


def test_cli_flag():
    from fusion_amd.retrievers import hybrid
    p = hybrid.build_parser()
    assert p.parse_known_args([])[0].colbert_fp8 is False and p.parse_known_args(["--colbert_fp8"])[0].colbert_fp8 is True


# ---- the shipped build -------------------------------------------------------------------------------------------------------------------
def test_the_fp8_kernels_hold_everything_in_registers(tmp_path):
    """The report the compile left next to the object (fusion_amd/csrc/maxsim8.res); skipped where the build left none."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if "maxsim8" not in res:
        pytest.skip("no maxsim8.res next to the objects: run `make -C fusion_amd/csrc` where ROCm is installed")
    mine = {kernel_resources.short(n): r for n, r in res["maxsim8"].items()}      # (c++filt may leave a _Float16 signature mangled)
    assert len(mine) == 2 and all(any(k in n for n in mine) for k in ("maxsim8_kernel", "quantize_e4m3_kernel")), sorted(mine)
    for name, r in mine.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, f"{name}: {r['vgpr_spill']} spilled VGPRs, {r['scratch']} B/lane of scratch"
