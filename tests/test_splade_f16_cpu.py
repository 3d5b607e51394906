"""The float16 SPLADE head (csrc/splade16.hip) and the encoders' `amp` switch, as far as a machine without a GPU can judge them: the two
exports and the header, the tile constants, the entry's argument checks (all on the host, before any HIP call, in the fp32 entry's order),
the compiler's resource report of the new file, and the precision plumbing of DenseEncoder / SpladeEncoder / random_init / the corpus
cache key / the CLI."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

NEW = ("fz_splade_head_max_f16", "fz_splade_head_f16_tile")


def _p(v):
    return C.c_void_p(v) if v else None


def tile(L):
    v = [C.c_int(-1) for _ in range(4)]
    assert L.fz_splade_head_f16_tile(*[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def test_exports_header_and_abi():
    from fusion_amd import _lib
    L = _lib.lib()
    assert set(NEW) <= set(_lib.EXPORTS) and all(hasattr(L, n) for n in NEW)
    assert L.fz_abi_version() == _lib.ABI_VERSION == 20          # additive entries: the ABI version stays
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    assert all(name + "(" in header for name in NEW)
    assert "finite by contract" in header                         # the float16 range is part of the entry's contract


def test_tile_constants():
    from fusion_amd import _lib
    L = _lib.lib()
    rows, cols, ktile, kstep = tile(L)
    assert min(rows, cols, ktile, kstep) > 0
    assert ktile % kstep == 0 and kstep == 16
    assert L.fz_splade_head_f16_tile(None, None, None, None) == _lib.FZ_ERR_ARG


def head(L, **kw):
    a = dict(X=0x10000, ldx=40, W=0x20000, ldw=40, bias=0x30000, cu=0x40000, nseq=3, T=50, V=70, d=40, pool=0x50000, ldp=72)
    a.update(kw)
    return L.fz_splade_head_max_f16(_p(a["X"]), a["ldx"], _p(a["W"]), a["ldw"], _p(a["bias"]), _p(a["cu"]), a["nseq"], a["T"], a["V"], a["d"],
                                    _p(a["pool"]), a["ldp"], None)


def test_argument_validation_without_gpu():
    """Every refusal comes before the first HIP call, so the (fake) pointers are never touched.  The order is the fp32 entry's: argument
    errors, then the empty problem, then null pointers, then what the kernel does not support."""
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    for name in ("T", "V", "nseq", "d"):
        assert head(L, **{name: -1}) == ARG, name
    assert head(L, d=0) == ARG
    assert head(L, ldx=32) == ARG and head(L, ldw=32) == ARG and head(L, ldp=69) == ARG
    for name in ("X", "W", "bias", "cu", "pool"):
        assert head(L, **{name: 0}) == ARG, name
    # the empty problem: no launch, null pointers welcome -- but a bad size is still a bad size
    empty = dict(X=0, W=0, bias=0, cu=0, pool=0)
    assert head(L, T=0, **empty) == OK and head(L, V=0, ldp=0, **empty) == OK and head(L, nseq=0, **empty) == OK
    assert head(L, T=0, ldx=32) == ARG
    assert head(L, T=0, d=36, ldx=36, ldw=36) == OK              # (unsupported shapes are judged after the empty problem, as in the fp32 entry)
    # float16 rows move as 16-byte pieces: d, ldx, ldw multiples of 8, both operands 16-byte aligned
    assert head(L, d=36) == UNS
    assert head(L, d=16, ldx=20) == UNS and head(L, d=16, ldw=20) == UNS
    assert head(L, X=0x10008) == UNS and head(L, W=0x20008) == UNS
    assert head(L, d=36, X=0) == ARG                              # a null pointer comes first
    assert head(L, ldx=1 << 24, ldw=1 << 24) == UNS               # 128 rows of it pass the 32-bit offsets of a tile


def test_the_kernels_of_the_new_file_hold_no_spilled_register():
    res = kernel_resources.load()
    if not res or "splade16" not in res:
        if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            pytest.skip("no .res reports next to the objects and no hipcc to make them: run `make -C fusion_amd/csrc` where ROCm is installed")
        assert res and "splade16" in res, "no splade16.res next to the objects: build with `make -C fusion_amd/csrc` (the Makefile writes them)"
    kernels = res["splade16"]
    assert len(kernels) >= 2, sorted(kernels)                    # the whole-k-tile and the ragged-d instantiation
    for name, k in kernels.items():
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, f"{kernel_resources.short(name)}: {k['vgpr_spill']} spilled VGPRs, {k['scratch']} B/lane of scratch"


def test_cpu_encoders_never_run_mixed():
    """amp is a GPU path: on the CPU the flag reads False, as CrossEncoder's does."""
    from fusion_amd import encoders
    tok = encoders.HashTokenizer(encoders.TINY["vocab_size"])
    dpr = encoders.DenseEncoder(encoders._backbone(dict(encoders.TINY)), tok, "cpu", amp=True)
    spl = encoders.SpladeEncoder(encoders._backbone(dict(encoders.TINY), mlm=True), tok, "cpu", amp=True)
    assert dpr.amp is False and spl.amp is False
    assert encoders.DenseEncoder(encoders._backbone(dict(encoders.TINY)), tok, "cpu").amp is False
    for kind in ("dpr", "splade"):
        assert encoders.random_init(kind, device="cpu", size="tiny", amp=True).amp is False
        assert encoders.random_init(kind, device="cpu", size="tiny").amp is False
    assert encoders.random_init("colbert", device="cpu", size="tiny", amp=False).amp is False


def test_cache_key_and_cli_carry_the_precision():
    from fusion_amd import encoders
    from fusion_amd.retrievers import hybrid
    docs = ["un", "deux", "trois"]
    assert encoders.corpus_cache_key("ckpt", docs, "dpr") != encoders.corpus_cache_key("ckpt", docs, "dpr-amp16")
    assert encoders.corpus_cache_key("ckpt", docs, "splade") != encoders.corpus_cache_key("ckpt", docs, "splade-amp16")
    p = hybrid.build_parser()
    assert p.parse_known_args([])[0].encoder_amp is False
    assert p.parse_known_args(["--encoder_amp"])[0].encoder_amp is True
    import inspect
    assert inspect.signature(hybrid.Ranker.single_vector_search).parameters["amp"].default is False
    for fn in (encoders.random_init, encoders.from_pretrained):
        assert inspect.signature(fn).parameters["amp"].default is None
