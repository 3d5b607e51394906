"""CPU-side tests (-m "not gpu") of the passage -> document layer: the new entry points in the header and the binding, every argument
check of fz_lists_collapse / fz_group_expand / fz_group_max_* (all made before the first HIP call, exercised with fake pointers), the
window rule of split_passages, PassageGroups' validation, and the NumPy restatement the GPU tests compare against
(tests/passage_cases.py) checked against a brute-force per-document maximum."""
import ctypes as C
import os

import numpy as np
import pytest

import passage_cases as pc
from conftest import ROOT

NEW = ("fz_lists_collapse_workspace_bytes", "fz_lists_collapse", "fz_group_expand_workspace_bytes", "fz_group_expand",
       "fz_group_max_f32", "fz_group_max_f64")


def test_entries_are_declared_and_abi_is_additive():
    from fusion_amd import _lib
    L = _lib.lib()
    assert L.fz_abi_version() == 20
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and f"{name}(" in header, name
    assert L.fz_lists_collapse_workspace_bytes(1024) >= 4 and L.fz_group_expand_workspace_bytes(1024) >= 4
    assert L.fz_lists_collapse_workspace_bytes(-1) == 0 and L.fz_group_expand_workspace_bytes(-1) == 0
    assert L.fz_lists_max_entries() == pc.CAPACITY


def test_the_passage_kernels_hold_no_spilled_register():
    """hipcc's per-kernel resource report of the shipped build (fusion_amd/csrc/lists_collapse.res, left by the compile)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load().get("lists_collapse")
    if not res:
        pytest.skip("no lists_collapse.res next to the objects: build with `make -C fusion_amd/csrc` where ROCm is installed")
    names = {kernel_resources.short(k).split("<")[0] for k in res}
    assert names == {"lists_collapse_kernel", "group_expand_kernel", "group_max_kernel"}
    for k, r in res.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, f"{k}: {r['vgpr_spill']} spilled VGPRs, {r['scratch']} B/lane of scratch"


def test_lists_collapse_rejects_bad_arguments_without_gpu():
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, UNS, OK, WS = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK, _lib.FZ_ERR_WORKSPACE
    cap = L.fz_lists_max_entries()
    fake = 4096                      # a non-null "device pointer": no call below may get as far as using it

    def call(ids=fake, sc=fake, sc64=None, lens=fake, ld=64, n=50, Q=4, group=fake, P=100, id_base=0, doc_base=0, out_ids=fake, out_sc=fake,
             out_sc64=None, best=fake, out_len=fake, ld_out=64, ws=fake, wsb=16):
        return L.fz_lists_collapse(ids, sc, sc64, lens, ld, n, Q, group, P, id_base, doc_base, out_ids, out_sc, out_sc64, best, out_len,
                                   ld_out, ws, wsb, None)

    for null in ("ids", "sc", "lens", "group", "out_ids", "out_sc", "best", "out_len"):
        assert call(**{null: None}) == ARG, null
    assert call(sc64=fake) == ARG and call(out_sc64=fake) == ARG              # the float64 planes come and go together
    assert call(Q=-1) == ARG and call(n=-1) == ARG and call(P=-1) == ARG
    assert call(ld=49) == ARG                                                  # row stride below the width
    assert call(ld_out=49) == ARG                                              # output rows narrower than the list
    assert call(n=cap + 1, ld=cap + 64, ld_out=cap + 64) == UNS
    assert call(n=cap + 1, ld=cap, ld_out=cap + 64) == ARG                     # the geometry before the capacity, as in fz_lists_join
    assert call(ws=None) == WS and call(wsb=2) == WS
    assert call(Q=0) == OK and call(n=0, ld=0, ld_out=0) == OK
    assert call(Q=0, ids=None, sc=None, lens=None, group=None, out_ids=None, out_sc=None, best=None, out_len=None, ws=None, wsb=0) == OK
    assert call(n=0, ids=None, sc=None, out_ids=None, out_sc=None, best=None, ws=None, wsb=0) == OK


def test_group_expand_and_max_reject_bad_arguments_without_gpu():
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, OK, WS = _lib.FZ_ERR_ARG, _lib.FZ_OK, _lib.FZ_ERR_WORKSPACE
    fake = 4096

    def expand(cand=fake, ld=64, cand_len=None, W=50, Q=4, poff=fake, D=10, pcand=fake, ldp=200, seg=fake, plen=fake, ws=fake, wsb=16):
        return L.fz_group_expand(cand, ld, cand_len, W, Q, poff, D, 0, 0, pcand, ldp, seg, plen, ws, wsb, None)

    for null in ("cand", "poff", "pcand", "seg", "plen"):
        assert expand(**{null: None}) == ARG, null
    assert expand(Q=-1) == ARG and expand(W=-1) == ARG and expand(D=-1) == ARG and expand(ldp=-1) == ARG
    assert expand(ld=49) == ARG
    assert expand(ws=None) == WS and expand(wsb=3) == WS
    assert expand(Q=0) == OK and expand(Q=0, cand=None, poff=None, pcand=None, seg=None, plen=None, ws=None, wsb=0) == OK

    for fn in (L.fz_group_max_f32, L.fz_group_max_f64):
        def gmax(ps=fake, ld_s=200, pcand=fake, ldp=200, seg=fake, cand_len=None, W=50, Q=4, out=fake, best=fake, ld_out=64):
            return fn(ps, ld_s, pcand, ldp, seg, cand_len, W, Q, out, best, ld_out, None)

        for null in ("ps", "pcand", "seg", "out", "best"):
            assert gmax(**{null: None}) == ARG, null
        assert gmax(Q=-1) == ARG and gmax(W=-1) == ARG and gmax(ldp=-1) == ARG
        assert gmax(ld_s=199) == ARG and gmax(ld_out=49) == ARG
        assert gmax(Q=0) == OK and gmax(W=0, ld_out=0) == OK
        assert gmax(Q=0, ps=None, pcand=None, seg=None, out=None, best=None) == OK


def test_python_wrappers_validate_before_the_device():
    import torch
    from fusion_amd import ops
    ids = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(TypeError, match="on the GPU"):
        ops.lists_collapse(ids, torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="on the GPU"):
        ops.group_expand(ids, None, torch.zeros(3, dtype=torch.int64), 8)
    with pytest.raises(TypeError, match="on the GPU"):
        ops.group_max(torch.zeros((2, 8)), torch.zeros((2, 8), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32))


def _windows(n, words, stride=None):
    from fusion_amd.passages import split_passages
    text = " ".join(f"w{i}" for i in range(n))
    passages, poff = split_passages([text], words, stride)
    assert poff.dtype == np.int64 and poff.tolist() == [0, len(passages)]
    return [[int(t[1:]) for t in p.split()] for p in passages]


def test_split_passages_window_rule():
    from fusion_amd.passages import split_passages
    assert _windows(0, 4) == [[]]                                    # an empty text: one empty passage
    assert _windows(1, 4) == [[0]]
    assert _windows(4, 4) == [[0, 1, 2, 3]]
    assert _windows(5, 4) == [[0, 1, 2, 3], [4]]
    # overlap: a window is emitted iff it holds a word the previous one does not
    assert _windows(9, 4, 2) == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7], [6, 7, 8]]
    assert _windows(10, 4, 2) == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7], [6, 7, 8, 9]]
    assert _windows(4, 4, 2) == [[0, 1, 2, 3]] and _windows(3, 4, 2) == [[0, 1, 2]]
    with pytest.raises(ValueError, match="stride"):
        split_passages(["a b c"], 2, 3)
    with pytest.raises(ValueError):
        split_passages(["a b c"], 0)
    with pytest.raises(ValueError):
        split_passages(["a b c"], 2, 0)
    passages, poff = split_passages(["a b  c\nd e", "", "x"], 2)     # str.split(): any whitespace
    assert passages == ["a b", "c d", "e", "", "x"] and poff.tolist() == [0, 3, 4, 5]
    rng = np.random.default_rng(5)
    for _ in range(50):                                              # every word is covered, in order, and no window is redundant
        n, words = int(rng.integers(0, 40)), int(rng.integers(1, 9))
        stride = int(rng.integers(1, words + 1))
        w = _windows(n, words, stride)
        assert sorted(set(sum(w, []))) == list(range(n))
        assert all(len(x) <= words for x in w) and all(x[-1] > y[-1] for x, y in zip(w[1:], w[:-1]))


def test_passage_groups_validates_poff():
    from fusion_amd.passages import PassageGroups
    g = PassageGroups(np.array([0, 2, 2, 5], np.int64), id_base=7, doc_id_base=1 << 40, device="cpu")
    assert (g.D, g.P, g.pmax) == (3, 5, 3) and g.group_of.tolist() == [0, 0, 2, 2, 2] and g.group_of.dtype.is_floating_point is False
    with pytest.raises(ValueError, match="non-decreasing"):
        PassageGroups(np.array([0, 3, 2], np.int64), device="cpu")
    with pytest.raises(ValueError, match="start at 0"):
        PassageGroups(np.array([1, 3, 4], np.int64), device="cpu")
    with pytest.raises(TypeError, match="int64"):
        PassageGroups(np.array([0, 3, 4], np.int32), device="cpu")
    with pytest.raises(ValueError):
        PassageGroups(np.zeros((2, 2), np.int64), device="cpu")


def test_pair_scores_holds_the_passage_scorer_to_its_contract(monkeypatch):
    """With the device steps stood in for, what the passage scorer returns is checked before the maximum is taken: a float32 or float64
    tensor of the expanded ids' shape (ops.check_pair_plane, under pair_scores' name for the scorer)."""
    import torch
    from fusion_amd import ops
    from fusion_amd.passages import PassageGroups
    g = PassageGroups(np.array([0, 2, 2, 5], np.int64), device="cpu")
    docs = torch.tensor([[0, 2], [1, -1]], dtype=torch.int64)                   # ldp = min(W * pmax, P) = 5 passage slots per query
    monkeypatch.setattr(ops, "_dev", lambda t, *a, **k: t)
    monkeypatch.setattr(ops, "group_expand", lambda ids, lens, poff, ldp, **k: (torch.zeros((2, ldp), dtype=torch.int64), None, lens))
    for bad in (lambda ids, lens: torch.zeros(ids.shape, dtype=torch.float16), lambda ids, lens: np.zeros((2, 5), np.float32)):
        with pytest.raises(TypeError, match=r"^PassageGroups\.pair_scores: the passage scorer must return a float32 or float64 tensor$"):
            g.pair_scores(bad, docs)
    with pytest.raises(ValueError, match=r"^PassageGroups\.pair_scores: the passage scorer returned \(2, 4\) for ids \(2, 5\)$"):
        g.pair_scores(lambda ids, lens: torch.zeros((2, 4)), docs)


@pytest.mark.parametrize("run", [1, 5])
def test_restatement_equals_brute_force_maximum(run):
    """collapse_ref (first occurrence in list order) == the per-document maximum ranked by (score desc, position asc) on ranked
    lists; max_ref == a plain loop."""
    rng = np.random.default_rng(11 + run)
    poff = pc.random_poff(rng, 60)
    group = pc.group_table(poff)
    P, Q, n = int(poff[-1]), 6, 150
    lens = pc.mixed_lens(rng, Q, n)
    ids, sc = pc.ranked_rows(rng, Q, n, P, lens, run=run, neg_tail=4, id_base=1000)
    d_ids, d_sc, _, best, out_len = pc.collapse_ref(ids, sc, lens, group, 1000, 77)
    for q, (e_ids, e_sc, e_best) in enumerate(pc.brute_force_maxp(ids, sc, lens, group, 1000, 77)):
        L = int(out_len[q])
        assert L == len(e_ids)
        np.testing.assert_array_equal(d_ids[q, :L], e_ids)
        np.testing.assert_array_equal(d_sc[q, :L], e_sc)
        np.testing.assert_array_equal(best[q, :L], e_best)
        assert (d_ids[q, L:] == -1).all() and (best[q, L:] == -1).all() and (d_sc[q, L:] == -np.inf).all()
    cand, cand_len, poff = pc.expand_case(rng, 5, 33, doc_id_base=9)
    ldp = int(pc.expand_need(cand, cand_len, poff, 9).max())
    pcand, seg, plen = pc.expand_ref(cand, cand_len, poff, ldp, 500, 9)
    assert plen.max() == ldp and (seg[:, -1] == plen).all()
    ps = pc.tied_scores(rng, (5, ldp), np.float32)
    out, best = pc.max_ref(ps, pcand, seg, cand_len)
    for q in range(5):
        for w in range(33):
            s = ps[q, seg[q, w]:seg[q, w + 1]]
            if w >= cand_len[q] or len(s) == 0:
                assert out[q, w] == -np.inf and best[q, w] == -1
            else:
                assert out[q, w] == s.max() and best[q, w] == pcand[q, seg[q, w] + int(np.argmax(s))]
                d = int(cand[q, w]) - 9
                assert pcand[q, seg[q, w]:seg[q, w + 1]].tolist() == list(range(500 + poff[d], 500 + poff[d + 1]))
