"""CPU-side tests (-m "not gpu") of the weight sweep over top-k lists: the argument checks of fz_lists_columns (all made before the
first HIP call), the wrappers' host-side errors, the topktune_*.npz fixtures against the checker the GPU tests use
(oracle.tune_lists), their generator, and the compiler's resource report of lists_columns_kernel."""
import ctypes as C
import filecmp
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from topk_tune_util import NORMS, TuneCase, defined_rows

TUNE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "topktune_*.npz")))


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def test_abi_is_additive():
    from fusion_amd import _lib
    L = _lib.lib()
    assert L.fz_abi_version() == 20
    assert L.fz_lists_columns_workspace_bytes(3, 1024) >= 4
    assert L.fz_lists_columns_workspace_bytes(0, 4) == 0 and L.fz_lists_columns_workspace_bytes(9, 4) == 0
    assert L.fz_lists_columns_workspace_bytes(2, -1) == 0
    for name in ("fz_lists_columns_workspace_bytes", "fz_lists_columns"):
        assert name in _lib.EXPORTS


def test_lists_columns_rejects_bad_arguments_without_gpu():
    """Null / negative / short-stride / over-capacity arguments are errors before any HIP call; Q == 0 and all-empty lists are FZ_OK
    with nothing launched.  Every pointer is a fake: no call below may get as far as using one."""
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, UNS, OK, WS = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK, _lib.FZ_ERR_WORKSPACE
    cap = L.fz_lists_max_entries()
    fake = 4096
    two = _ptrs(fake, fake)

    def cols(ids=two, lens=two, vals=two, n=_i32(10, 10), ld=_i32(10, 10), S=2, Q=4, gold=fake, G=8, out_ids=fake, T=two, pos=fake,
             out_len=fake, gold_col=fake, ld_out=64, ws=fake, wsb=16):
        return L.fz_lists_columns(ids, lens, vals, n, ld, S, Q, gold, G, out_ids, T, pos, out_len, gold_col, ld_out, ws, wsb, None)

    assert cols(S=0) == ARG and cols(S=-1) == ARG and cols(S=9) == ARG                       # S outside [1, FZ_MAX_SYSTEMS]
    assert cols(Q=-1) == ARG and cols(G=-1) == ARG
    assert cols(n=None) == ARG and cols(ld=None) == ARG
    assert cols(n=_i32(10, -1)) == ARG                                                         # negative width
    assert cols(ld=_i32(10, 9)) == ARG                                                         # row stride below the width
    assert cols(ld_out=19) == ARG                                                              # output rows narrower than the lists together
    assert cols(ids=None) == ARG and cols(lens=None) == ARG
    assert cols(out_ids=None) == ARG and cols(pos=None) == ARG and cols(out_len=None) == ARG
    assert cols(ids=_ptrs(fake, None)) == ARG and cols(lens=_ptrs(None, fake)) == ARG
    assert cols(vals=_ptrs(fake, None)) == ARG                                                 # values for some systems only
    assert cols(T=None) == ARG and cols(T=_ptrs(None, fake)) == ARG                            # values without a plane to scatter them to
    assert cols(gold=None) == ARG and cols(gold_col=None) == ARG                               # G > 0 needs both
    assert cols(ws=None) == WS and cols(wsb=2) == WS
    # capacity: the lists of one query together
    half = cap // 2
    assert cols(n=_i32(half, half + 1), ld=_i32(half, half + 1), ld_out=cap + 64) == UNS
    assert cols(n=_i32(cap, 1), ld=_i32(cap, 1), ld_out=cap + 64) == UNS
    eight = _ptrs(*([fake] * 8))
    assert cols(ids=eight, lens=eight, vals=eight, T=eight, n=_i32(*([1025] * 8)), ld=_i32(*([1025] * 8)), S=8, ld_out=8 * 1025) == UNS
    # nothing to do
    assert cols(Q=0) == OK
    assert cols(Q=0, ids=None, lens=None, vals=None, T=None, gold=None, out_ids=None, pos=None, out_len=None, gold_col=None, ws=None, wsb=0) == OK
    assert cols(n=_i32(0, 0), ld=_i32(0, 0), ld_out=0) == OK
    assert cols(n=_i32(0, 0), ld=_i32(8, 8), ids=None, lens=None, vals=None, T=None, out_ids=None, pos=None, ws=None, wsb=0) == OK


def test_python_wrappers_validate_before_the_device():
    from fusion_amd import ops
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    ids = torch.arange(6, dtype=torch.int64).reshape(2, 3)
    lens = torch.full((2,), 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 8"):
        ops.lists_columns([ids] * 9, [lens] * 9)
    with pytest.raises(ValueError, match="length vectors"):
        ops.lists_columns([ids], [lens, lens])
    with pytest.raises(ValueError, match="value planes"):
        ops.lists_columns([ids], [lens], [ids.float(), ids.float()])
    with pytest.raises(TypeError, match="on the GPU"):
        ops.lists_columns([ids], [lens], [ids.float()], ids)
    rt = RankedTopk.from_search(torch.zeros((2, 3)), ids)
    grid = [{"a": 0.5, "b": 0.5}]
    labels = [[1], [2]]
    with pytest.raises(ValueError, match="at most 8"):
        Aggregator.tune_topk({f"s{i}": rt for i in range(9)}, "min-max", grid, labels, {})
    with pytest.raises(AssertionError, match="varying lenghts"):
        Aggregator.tune_topk({"a": rt, "b": RankedTopk.from_search(torch.zeros((1, 3)), ids[:1])}, "min-max", grid, labels, {})
    with pytest.raises(KeyError):
        Aggregator.tune_topk({"a": rt, "c": rt}, "min-max", grid, labels, {})               # fast path: system c has no weight
    with pytest.raises(KeyError):
        Aggregator.tune_topk({"a": rt, "c": rt}, "none", grid, labels, {})                  # generic path
    with pytest.raises(TypeError, match="on the GPU"):
        Aggregator.tune_topk({"a": rt, "b": rt}, "min-max", grid, labels, {})               # CPU tensors: there is no CPU path
    with pytest.raises(TypeError, match="on the GPU"):
        Aggregator.evaluate_topk(rt, labels)
    with pytest.raises(ValueError, match="labels for 1 queries"):
        Aggregator.evaluate_topk(rt, [[1]])


def test_fixtures_cover_what_they_claim():
    assert len(TUNE_FILES) == 2
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if p not in TUNE_FILES)
    for p in TUNE_FILES:
        c = TuneCase(p)
        assert os.path.getsize(p) <= biggest
        assert 20 <= len(c.weights) <= 30 and c.weights.dtype == np.float64 and (c.weights == 0.0).any()
        assert all(1 <= len(set(g)) <= 5 for g in c.labels) and any(len(set(g)) < len(g) for g in c.labels)
        listed = [[sum(g in set(c.ids[s, q, :c.lens[s, q]].tolist()) for s in range(len(c.systems))) for g in gl] for q, gl in enumerate(c.labels)]
        assert any(n == 0 for l in listed for n in l) and any(n == 1 for l in listed for n in l)       # in no list; in one system's only
        assert (c.lens.sum(0) > 0).all()                                                             # the all-empty query is dropped
    assert any(TuneCase(p).raises == {"min-max"} for p in TUNE_FILES) and any(not TuneCase(p).raises for p in TUNE_FILES)
    # the vectors the reference defines (defined_rows): every one under arctan / percentile-rank / 'none' and, where it does not raise,
    # min-max; the zero-free ones under NCE.  Under z-score NONE: both cases hold a single-entry list in some query (k = 1 systems),
    # whose z-score is NaN -- the z-score sweep is held to the parent's own code in tests/test_gpu_lists_tune.py instead
    for p in TUNE_FILES:
        c = TuneCase(p)
        n = {norm: int(np.count_nonzero(np.ones(len(c.weights), bool)[defined_rows(c, norm)])) for norm in NORMS if norm not in c.raises}
        assert all(n[k] == len(c.weights) for k in ("arctan", "percentile-rank", "none", "min-max") if k in n), n
        assert n["normal-curve-equivalent"] >= 10 and n["z-score"] == 0, n


@pytest.mark.parametrize("path", TUNE_FILES, ids=[os.path.basename(p)[:-4] for p in TUNE_FILES])
def test_oracle_reproduces_the_reference_metrics(path, oracle):
    """oracle.tune_lists on the fixture's dict lists == the reference's stored metrics, every metric of every vector within 1e-12
    (statistics.mean against an exactly rounded sum).  NCE vectors with a zero weight are undefined in the reference (-inf * 0)."""
    c = TuneCase(path)
    seen = 0
    for norm in NORMS:
        if norm in c.raises:
            assert f"metrics__{norm}" not in c.z.files
            continue
        got = oracle.tune_lists(c.lists(), norm, c.grid(), c.labels, c.distr)
        assert all(list(g) == c.metric_names for g in got)
        G = np.array([[float(g[k]) for k in c.metric_names] for g in got])
        assert np.max(np.abs(G - c.z[f"metrics__{norm}"])[defined_rows(c, norm)], initial=0.0) <= 1e-12, norm
        seen += 1
    assert seen >= 5


def test_generator_reproduces_committed_fixtures(tmp_path):
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, "src", "retrievers")):
        pytest.skip("the reference tree is not on this machine")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_topktune.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    made = sorted(os.listdir(tmp_path))
    assert made == [os.path.basename(p) for p in TUNE_FILES]
    for name in made:
        assert filecmp.cmp(os.path.join(tmp_path, name), os.path.join(GOLDEN, name), shallow=False), name


def test_columns_kernel_holds_no_spilled_register(tmp_path):
    """The compiler's resource report of lists_columns_kernel: no spilled VGPR, no scratch (tools/kernel_resources.py on the shipped
    build's lists_tune.res; without it the one source is compiled into a temporary directory, and without hipcc the check is skipped)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load()
    if not res or "lists_tune" not in res:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip("no lists_tune.res next to the objects and no hipcc to make it: run `make -C fusion_amd/csrc` where ROCm is installed")
        flags = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()
        r = subprocess.run([hipcc, *flags, "-c", os.path.join(ROOT, "fusion_amd", "csrc", "lists_tune.hip"), "-o", str(tmp_path / "lists_tune.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        (tmp_path / "lists_tune.res").write_text(r.stderr)
        res = kernel_resources.load(str(tmp_path))
    mine = {kernel_resources.short(n): k for n, k in res["lists_tune"].items()}
    assert list(mine) == ["lists_columns_kernel"], list(mine)
    k = mine["lists_columns_kernel"]
    assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k
