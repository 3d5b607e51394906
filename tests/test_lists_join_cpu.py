"""CPU-side tests (-m "not gpu") of the top-k list fusion: the argument checks of fz_lists_join (all made before the first HIP
call), the list-form fixtures tests/golden/topkfuse_*.npz against the checker the GPU tests use (oracle.fuse_lists), their
generator, and the host side of RankedTopk / FusedTopk."""
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
from topk_fuse_util import EXACT, METHODS, Case, assert_fused_equal, lists_of

TOPK_FILES = sorted(glob.glob(os.path.join(GOLDEN, "topkfuse_*.npz")))


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def test_abi_is_additive():
    from fusion_amd import _lib
    L = _lib.lib()
    assert L.fz_abi_version() == 20
    assert L.fz_lists_max_entries() >= 8192
    assert L.fz_lists_join_workspace_bytes(3, 1024) >= 4
    assert L.fz_lists_join_workspace_bytes(0, 4) == 0 and L.fz_lists_join_workspace_bytes(9, 4) == 0 and L.fz_lists_join_workspace_bytes(2, -1) == 0
    for name in ("fz_lists_max_entries", "fz_lists_join_workspace_bytes", "fz_lists_join"):
        assert name in _lib.EXPORTS


def test_lists_join_rejects_bad_arguments_without_gpu():
    """Null / negative / over-capacity / S > 8 arguments are errors before any HIP call; Q == 0 and all-empty lists are FZ_OK with
    nothing launched."""
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, UNS, OK, WS = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK, _lib.FZ_ERR_WORKSPACE
    cap = L.fz_lists_max_entries()
    fake = 4096                      # a non-null "device pointer": no call below may get as far as using it
    two = _ptrs(fake, fake)
    w2 = (C.c_double * 2)(0.5, 0.5)

    def join(ids=two, lens=two, vals=None, v64=None, w=None, nr=None, n=_i32(10, 10), ld=_i32(10, 10), S=2, Q=4, method=0,
             out_ids=fake, out_sc=fake, out_len=fake, ld_out=64, ws=fake, wsb=16):
        return L.fz_lists_join(ids, lens, vals, v64, w, nr, n, ld, S, Q, method, out_ids, out_sc, out_len, ld_out, ws, wsb, None)

    assert join(S=0) == ARG and join(S=-1) == ARG and join(S=9) == ARG                       # S outside [1, FZ_MAX_SYSTEMS]
    assert join(Q=-1) == ARG
    assert join(n=None) == ARG and join(ld=None) == ARG
    assert join(method=4) == ARG and join(method=-1) == ARG
    assert join(n=_i32(10, -1)) == ARG                                                         # negative width
    assert join(n=_i32(10, 10), ld=_i32(10, 9)) == ARG                                         # row stride below the width
    assert join(ld_out=19) == ARG                                                              # output rows narrower than the lists together
    assert join(ids=None) == ARG and join(lens=None) == ARG
    assert join(out_ids=None) == ARG and join(out_sc=None) == ARG and join(out_len=None) == ARG
    assert join(ids=_ptrs(fake, None)) == ARG and join(lens=_ptrs(None, fake)) == ARG
    assert join(method=2) == ARG and join(method=3, vals=two) == ARG                           # weighted sums need values and weights
    assert join(method=2, vals=None, w=w2) == ARG and join(method=2, vals=_ptrs(fake, None), w=w2) == ARG
    assert join(method=2, vals=two, w=w2, v64=_i32(0, 1)) == ARG                               # the float32 sum takes float32 planes
    assert join(ws=None) == WS and join(wsb=2) == WS
    # capacity: the lists of one query together
    half = cap // 2
    assert join(n=_i32(half, half + 1), ld=_i32(half, half + 1), ld_out=cap + 64) == UNS
    assert join(n=_i32(cap, 1), ld=_i32(cap, 1), ld_out=cap + 64) == UNS
    eight = _ptrs(*([fake] * 8))
    assert join(ids=eight, lens=eight, n=_i32(*([1025] * 8)), ld=_i32(*([1025] * 8)), S=8, ld_out=8 * 1025) == UNS
    # nothing to do
    assert join(Q=0) == OK
    assert join(Q=0, ids=None, lens=None, out_ids=None, out_sc=None, out_len=None, ws=None, wsb=0) == OK   # empty tensors carry null pointers
    assert join(n=_i32(0, 0), ld=_i32(0, 0), ld_out=0) == OK                                    # every list empty: out_len stays the caller's zeros
    assert join(n=_i32(0, 0), ld=_i32(8, 8), ids=None, lens=None, out_ids=None, out_sc=None, ws=None, wsb=0) == OK


def test_python_wrapper_validates_before_the_device():
    """ops.lists_join / Aggregator.fuse_topk: the system count is checked before any tensor is looked at; CPU tensors are refused
    (there is no CPU path)."""
    from fusion_amd import ops
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    ids = torch.arange(6, dtype=torch.int64).reshape(2, 3)
    lens = torch.full((2,), 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 8"):
        ops.lists_join([ids] * 9, [lens] * 9, "rrf")
    with pytest.raises(ValueError, match="unknown method"):
        ops.lists_join([ids], [lens], "sum")
    with pytest.raises(TypeError, match="on the GPU"):
        ops.lists_join([ids], [lens], "rrf")
    rt = RankedTopk.from_search(torch.zeros((2, 3)), ids)
    with pytest.raises(ValueError, match="at most 8"):
        Aggregator.fuse_topk({f"s{i}": rt for i in range(9)}, "rrf")
    with pytest.raises(AssertionError, match="varying lenghts"):
        Aggregator.fuse_topk({"a": rt, "b": RankedTopk.from_search(torch.zeros((1, 3)), ids[:1])}, "rrf")
    with pytest.raises(AttributeError):
        Aggregator.fuse_topk({"a": rt}, "nsf", "min-max", {"a": 1.0}, None)
    with pytest.raises(KeyError):
        Aggregator.fuse_topk({"a": rt}, "nsf", "min-max", {}, {})


def test_fixture_cases_cover_what_they_claim():
    assert len(TOPK_FILES) >= 5
    cases = [Case(p) for p in TOPK_FILES]
    assert {len(c.systems) for c in cases} >= {1, 2, 3, 4, 8}
    assert all(c.max_entries() <= 8192 for c in cases)
    assert max(os.path.getsize(p) for p in TOPK_FILES) <= max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if p not in TOPK_FILES)
    all_ids = np.concatenate([c.ids[c.ids >= 0] for c in cases])
    assert (all_ids > (1 << 32)).any() and (all_ids == (1 << 62)).any() and (all_ids < (1 << 32)).any()
    assert any({1, 10, 1000} <= {int(x) for x in c.lens.max(1)} for c in cases)                     # k of 1, 10, 1000 inside one case
    assert any((c.lens.sum(0) == 0).any() for c in cases)                                           # a query where every list is empty
    assert any(((c.lens == 0).any(0) & (c.lens.sum(0) > 0)).any() for c in cases)                   # some, not all, lists empty
    assert any((c.lens == 1).any() and len(c.systems) == 1 for c in cases)                          # a single-entry list on its own
    assert any("nsf__min-max" in c.raises for c in cases) and all(c.raises <= {"nsf__min-max"} for c in cases)
    tails, ties_in, ties_across, disjoint, identical = False, False, False, False, False
    for c in cases:
        for q in range(c.Q):
            sets = [set(c.ids[s, q, :c.lens[s, q]].tolist()) for s in range(len(c.systems))]
            full = [s for s in sets if s]
            if len(full) >= 2:
                disjoint |= all(not (a & b) for i, a in enumerate(full) for b in full[i + 1:])
                identical |= all(a == full[0] for a in full) and any(
                    c.ids[s, q, :c.lens[s, q]].tolist() != c.ids[0, q, :c.lens[0, q]].tolist() for s in range(1, len(sets)))
            for s in range(len(c.systems)):
                v = c.scores[s, q, :c.lens[s, q]]
                if c.systems[s] == "bm25" and len(v) >= 8:
                    tails |= bool(v[-1] == 0.0 and v[-2] == 0.0 and v[0] > 0.0)
                ties_in |= bool(len(v) >= 2 and (v[:-1] == v[1:]).any() and v[0] != v[-1])
                if s > 0 and len(v) and c.lens[0, q]:
                    ties_across |= bool(np.isin(v[v != 0.0], c.scores[0, q, :c.lens[0, q]]).any())
    assert tails and ties_in and ties_across and disjoint and identical


@pytest.mark.parametrize("path", TOPK_FILES, ids=[os.path.basename(p)[:-4] for p in TOPK_FILES])
def test_oracle_reproduces_topk_fixtures(path, oracle):
    """oracle.fuse_lists -- what the GPU tests check the corpus-scale shapes against -- equals the reference's stored outputs on every
    fixture and pair, under the comparison rule of the GPU tests.  A pair the reference raised on has no stored output: there the
    project's rule must return, over the same union of ids as the other pairs (the GPU tests hold the device path to it)."""
    c = Case(path)
    lists = c.lists()
    seen = 0
    for pair in METHODS:
        got = lists_of(oracle.fuse_lists(lists, pair[0], pair[1], c.weights, c.distr))
        if f"{pair[0]}__{pair[1]}" in c.raises:      # no stored output: the project's rule returns, over the same union as every other pair
            union = c.expected(("rrf", "none"), oracle)
            assert [sorted(g[0].tolist()) for g in got] == [sorted(u[0].tolist()) for u in union]
            continue
        assert_fused_equal(got, c.expected(pair, oracle), pair, os.path.basename(path))
        seen += 1
    assert seen >= len(METHODS) - 1 and seen + len(c.raises) == len(METHODS)
    assert EXACT <= set(METHODS)


def test_generator_reproduces_committed_fixtures(tmp_path):
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, "src", "retrievers")):
        pytest.skip("the reference tree is not on this machine")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_topk.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    made = sorted(os.listdir(tmp_path))
    assert made == [os.path.basename(p) for p in TOPK_FILES]
    for name in made:
        assert filecmp.cmp(os.path.join(tmp_path, name), os.path.join(GOLDEN, name), shallow=False), name


def test_ranked_topk_and_fused_topk_round_trip_on_host():
    from fusion_amd.planes import FusedTopk, RankedTopk
    ids = torch.tensor([[5, (1 << 40) + 3, 1 << 62, -1], [7, -1, -1, -1], [-1, -1, -1, -1]], dtype=torch.int64)
    sc = torch.tensor([[3.5, 2.25, 0.1, float("-inf")], [1.0] + [float("-inf")] * 3, [float("-inf")] * 4], dtype=torch.float32)
    rt = RankedTopk.from_search(sc, ids)
    assert rt.lens.dtype == torch.int32 and rt.lens.tolist() == [3, 1, 0] and (rt.Q, rt.k) == (3, 4)
    lists = rt.to_lists()
    assert [[x["corpus_id"] for x in l] for l in lists] == [[5, (1 << 40) + 3, 1 << 62], [7], []]
    assert [x["score"] for x in lists[0]] == [3.5, 2.25, float(np.float32(0.1))] and all(type(x["score"]) is float for l in lists for x in l)
    s64 = sc.double().clone(); s64[0, 2] = 0.1
    assert RankedTopk.from_search(sc, ids, scores64=s64).to_lists()[0][2]["score"] == 0.1          # the unrounded score, when there is one
    with pytest.raises(TypeError):
        RankedTopk.from_search(sc, ids.int())
    with pytest.raises(ValueError):
        RankedTopk.from_search(sc[:, :3], ids)
    lens = torch.tensor([3, 1, 0], dtype=torch.int32)
    f64 = FusedTopk(ids=ids, scores=sc.double(), lens=lens).to_lists()
    f32 = FusedTopk(ids=ids, scores=sc, lens=lens).to_lists()
    assert [len(l) for l in f64] == [3, 1, 0] and [x["corpus_id"] for x in f64[0]] == [5, (1 << 40) + 3, 1 << 62]
    assert all(type(x["score"]) is float for l in f64 for x in l) and all(type(x["score"]) is np.float32 for l in f32 for x in l)
    assert f32[0][2]["score"] == np.float32(0.1)
    fr = FusedTopk(ids=ids, scores=sc, lens=lens)
    assert fr.predictions() == [[5, (1 << 40) + 3, 1 << 62], [7], []] and fr.predictions(2) == [[5, (1 << 40) + 3], [7], []]
