"""The top-k kernels (csrc/topk.hip) at every round, stretch, level and tie-run edge, with no tolerance: every comparison is
np.array_equal on ids and on score bit patterns against the NumPy references of topk_cases.py (which test_topk_cases_cpu.py holds to the
oracle on every case).

Operands are views into larger buffers: the row stride exceeds n, the columns [n, ld) and the ghost rows before and after hold +inf, so
a column read past a row's end enters the list instead of hiding.  Outputs are views into sentinel-filled buffers that must come back
untouched outside the documented extent -- for the append form that includes the slots past cap and past cand_len.  id_base lies above
2^33.  The cases land every branch of topk_cases.BRANCHES (test_branch_table_is_covered; the same check runs without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import topk_cases as T

pytestmark = pytest.mark.gpu
MARGIN = 64                       # sentinel cells in front of and behind every output


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def _abi():
    from fusion_amd import _lib
    return _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


class Out:
    """n cells of an output inside a sentinel-filled buffer; `init` presets them (a length, prior candidates)."""

    def __init__(self, n, dtype, fill, init=None):
        self.n, self.fill = n, fill
        host = np.full(n + 2 * MARGIN, fill, dtype=dtype)
        if init is not None:
            host[MARGIN: MARGIN + n] = np.asarray(init).reshape(-1)
        self.before = host.copy()
        self.t = dev(host)
        self.p = ptr(self.t, MARGIN)

    def get(self):
        got = self.t.cpu().numpy()
        assert np.array_equal(T.bits(got[:MARGIN]), T.bits(self.before[:MARGIN])) and \
            np.array_equal(T.bits(got[MARGIN + self.n:]), T.bits(self.before[MARGIN + self.n:])), "cells outside the output were written"
        return got[MARGIN: MARGIN + self.n]

    def untouched(self):
        return np.array_equal(T.bits(self.t.cpu().numpy()), T.bits(self.before))


def same(got, ref):
    return got.dtype == ref.dtype and np.array_equal(T.bits(got).reshape(-1), T.bits(ref).reshape(-1))


def first_diff(got, ref):
    bad = np.flatnonzero(T.bits(got).reshape(-1) != T.bits(ref).reshape(-1))
    return len(bad), [(int(j), got.reshape(-1)[j].item(), ref.reshape(-1)[j].item()) for j in bad[:6]]


def test_branch_table_is_covered():
    first, missing = T.landing()
    assert not missing, missing
    for c in T.ALL_CASES:
        assert set(getattr(c, "claims", ())) <= c.branches(), c.id


# ---- whole rows ------------------------------------------------------------------------------------------------------------------------
def rows_run(x, k, id_base, ws_short=0):
    L, st = _abi()
    rows, n = x.shape
    buf, off, ld = T.framed(x, "aligned")
    d = dev(buf)
    os_, oi = Out(rows * k, np.float32, T.S_GUARD), Out(rows * k, np.int64, T.I_GUARD)
    wsb = int(L.fz_topk_workspace_bytes(rows, n, k))
    ws = torch.full((max(wsb, 16),), 0x7F, dtype=torch.uint8, device="cuda")      # 3.4e38 / column 2,139,062,143: a slot left unwritten would win
    rc = L.fz_topk_rows_f32(ptr(d, off), rows, n, ld, k, id_base, os_.p, oi.p, ptr(ws), wsb - ws_short, st)
    torch.cuda.synchronize()
    return rc, os_, oi


@pytest.mark.parametrize("case", T.ROWS_CASES, ids=lambda c: c.id)
def test_rows_case_is_exact(case):
    x = case.inputs()
    rs, ri = T.topk_ref(x, case.k, T.ID_BASE)
    rc, os_, oi = rows_run(x, case.k, T.ID_BASE)
    assert rc == T.OK
    gs, gi = os_.get().reshape(case.rows, case.k), oi.get().reshape(case.rows, case.k)
    assert same(gi, ri), (case.id, first_diff(gi, ri))
    assert same(gs, rs), (case.id, first_diff(gs, rs))


def test_rows_refusals_leave_the_outputs_untouched():
    x = T.RowsCase(35841, 100, ("ties",)).inputs()
    rc, os_, oi = rows_run(x, T.MAX_K + 1, T.ID_BASE)
    assert rc == T.ERR_UNSUPPORTED and os_.untouched() and oi.untouched()
    rc, os_, oi = rows_run(x, 100, T.ID_BASE, ws_short=1)                # a workspace one byte short
    assert rc == T.ERR_WORKSPACE and os_.untouched() and oi.untouched()
    rc, os_, oi = rows_run(x[:, :50], 100, T.ID_BASE)                    # ... and the same entry taken, padded
    assert rc == T.OK and (oi.get()[50:] == -1).all()


# ---- the filter: append form -----------------------------------------------------------------------------------------------------------
def prior_cells(rows, cap, prior):
    """What the candidate lists hold before the call: `prior[r]` entries per row (score 9000 + slot, id 100 + slot), guard values behind."""
    s, i = np.full((rows, cap), T.S_GUARD, dtype=np.float32), np.full((rows, cap), T.I_GUARD, dtype=np.int64)
    for r in range(rows):
        p = min(int(prior[r]), cap)
        s[r, :p], i[r, :p] = 9000.0 + np.arange(p), 100 + np.arange(p)
    return s, i


def append_run(d, off, ld, rows, n, id_base, tau_d, cs, ci, cl, ov, cap):
    L, st = _abi()
    rc = L.fz_topk_filter_append_f32(ptr(d, off), rows, n, ld, id_base, ptr(tau_d), cs.p, ci.p, cl.p, cap, ov.p, st)
    torch.cuda.synchronize()
    return rc


def append_expected(sc, tau, prior, cap, id_base):
    rows = sc.shape[0]
    es, ei = prior_cells(rows, cap, prior)
    exp, lens, flag = T.filter_expected(sc, tau, prior, cap, id_base)
    for r, (s, i) in enumerate(exp):
        p = int(prior[r])
        es[r, p: p + len(s)], ei[r, p: p + len(s)] = s, i
    return es, ei, lens, flag


@pytest.mark.parametrize("case", T.ALL_FILTER_CASES, ids=lambda c: c.id)
def test_append_case_is_exact_in_every_layout(case):
    tau, sc = case.inputs()
    rows, n, cap = case.rows, case.n, case.cap()
    prior = np.array(case.prior[:rows], dtype=np.int32)
    es, ei, lens, flag = append_expected(sc, tau, prior, cap, T.ID_BASE)
    tau_d = dev(tau)
    for name in T.LAYOUTS:
        buf, off, ld = T.framed(sc, name)
        d = dev(buf)
        assert ((d.data_ptr() + 4 * off) % 16 == 0 and ld % 4 == 0) == T.LAYOUT_VEC[name]
        ps, pi = prior_cells(rows, cap, prior)
        cs, ci = Out(rows * cap, np.float32, T.S_GUARD, ps), Out(rows * cap, np.int64, T.I_GUARD, pi)
        cl, ov = Out(rows, np.int32, T.I_GUARD, prior), Out(1, np.int32, T.I_GUARD, [0])
        assert append_run(d, off, ld, rows, n, T.ID_BASE, tau_d, cs, ci, cl, ov, cap) == T.OK
        gl = cl.get()
        assert np.array_equal(gl, lens), (case.id, name, gl, lens)
        assert int(ov.get()[0]) == flag, (case.id, name)
        gi, gs = ci.get().reshape(rows, cap), cs.get().reshape(rows, cap)
        assert same(gi, ei), (case.id, name, first_diff(gi, ei))           # ascending columns behind the prior entries, guard values past cand_len
        assert same(gs, es), (case.id, name, first_diff(gs, es))


@pytest.mark.parametrize("n1", [3, 65536, 66561])
def test_two_appends_back_to_back(n1):
    """Two pieces of one plane appended one after the other (different prior lengths per row) == one append of the whole."""
    case = T.FilterCase(131077, "planted", taus=("finite", "zero", "neg"), prior=(0, 7, 2))
    tau, sc = case.inputs()
    rows, n, cap = case.rows, case.n, case.cap()
    prior = np.array(case.prior, dtype=np.int32)
    es, ei, lens, flag = append_expected(sc, tau, prior, cap, T.ID_BASE)
    buf, off, ld = T.framed(sc, "slice")
    d, tau_d = dev(buf), dev(tau)
    ps, pi = prior_cells(rows, cap, prior)
    cs, ci = Out(rows * cap, np.float32, T.S_GUARD, ps), Out(rows * cap, np.int64, T.I_GUARD, pi)
    cl, ov = Out(rows, np.int32, T.I_GUARD, prior), Out(1, np.int32, T.I_GUARD, [0])
    assert append_run(d, off, ld, rows, n1, T.ID_BASE, tau_d, cs, ci, cl, ov, cap) == T.OK
    mid = cl.get().copy()
    assert np.array_equal(mid, prior + T.filter_survivors(sc[:, :n1], tau).sum(axis=1)) and len(set(mid.tolist())) == rows
    assert append_run(d, off + n1, ld, rows, n - n1, T.ID_BASE + n1, tau_d, cs, ci, cl, ov, cap) == T.OK
    assert np.array_equal(cl.get(), lens) and int(ov.get()[0]) == flag == 0
    assert same(ci.get().reshape(rows, cap), ei) and same(cs.get().reshape(rows, cap), es)


# ---- the filter: update form -----------------------------------------------------------------------------------------------------------
def update_run(sc, run_s, run_i, cap, name, id_base, ws_short=0):
    L, st = _abi()
    rows, n = sc.shape
    k = run_s.shape[1]
    buf, off, ld = T.framed(sc, name)
    d, rs, ri = dev(buf), dev(run_s), dev(run_i)
    ns, ni = Out(rows * k, np.float32, T.S_GUARD), Out(rows * k, np.int64, T.I_GUARD)
    ov = Out(1, np.int32, T.I_GUARD, [0])
    wsb = int(L.fz_topk_update_workspace_bytes(rows, k, cap))
    ws = torch.empty(wsb + 16, dtype=torch.uint8, device="cuda")
    rc = L.fz_topk_update_f32(ptr(d, off), rows, n, ld, id_base, ptr(rs), ptr(ri), k, cap, ns.p, ni.p, ov.p, ptr(ws), wsb - ws_short, st)
    torch.cuda.synchronize()
    return rc, ns, ni, ov


@pytest.mark.parametrize("n", T.UPDATE_N)
@pytest.mark.parametrize("density", T.UPDATE_DENSITIES)
def test_update_case_is_exact_in_every_layout(n, density):
    case, k, run_s, run_i, tau, sc = T.update_inputs(n, density)
    es, ei = T.update_ref(run_s, run_i, sc, T.ID_BASE)
    for name in T.LAYOUTS:
        rc, ns, ni, ov = update_run(sc, run_s, run_i, case.cap(), name, T.ID_BASE)
        assert rc == T.OK and int(ov.get()[0]) == 0
        gi, gs = ni.get().reshape(case.rows, k), ns.get().reshape(case.rows, k)
        assert same(gi, ei), (n, density, name, first_diff(gi, ei))
        assert same(gs, es), (n, density, name, first_diff(gs, es))


def test_update_overflow_flag_at_cap_and_one_below():
    case, k, run_s, run_i, tau, sc = T.update_inputs(131077, "planted")
    count = int(T.filter_survivors(sc, tau).sum(axis=1).max())
    for cap, flag in ((count, 0), (count - 1, 1)):
        rc, ns, ni, ov = update_run(sc, run_s, run_i, cap, "aligned", T.ID_BASE)
        assert rc == T.OK and int(ov.get()[0]) == flag, (cap, count)
    es, ei = T.update_ref(run_s, run_i, sc, T.ID_BASE)
    rc, ns, ni, ov = update_run(sc, run_s, run_i, count, "aligned", T.ID_BASE)
    assert same(ni.get().reshape(ei.shape), ei) and same(ns.get().reshape(es.shape), es)


# ---- fold --------------------------------------------------------------------------------------------------------------------------------
def fold_run(k, cap, run_s, run_i, cand_s, cand_i, cand_len, unordered, tau0=None, ws_short=0):
    L, st = _abi()
    rows = run_s.shape[0]
    rs, ri, cs, ci = dev(run_s), dev(run_i), dev(cand_s), dev(cand_i)
    cl = Out(rows, np.int32, T.I_GUARD, cand_len)
    ns, ni = Out(rows * k, np.float32, T.S_GUARD), Out(rows * k, np.int64, T.I_GUARD)
    tau = Out(rows, np.float32, T.S_GUARD, tau0)
    ov = Out(1, np.int32, T.I_GUARD, [0])
    wsb = int(L.fz_topk_fold_workspace_bytes(rows, k, cap))
    ws = torch.empty(wsb + 16, dtype=torch.uint8, device="cuda")
    rc = L.fz_topk_fold_f32(ptr(rs), ptr(ri), rows, k, ptr(cs), ptr(ci), cl.p, cap, unordered, ns.p, ni.p, tau.p, ov.p, ptr(ws), wsb - ws_short, st)
    torch.cuda.synchronize()
    assert same(cs.cpu().numpy(), cand_s) and same(ci.cpu().numpy(), cand_i)      # the inputs stay as they were
    return rc, ns, ni, tau, cl, ov


@pytest.mark.parametrize("case", T.FOLD_CASES, ids=lambda c: c.id)
def test_fold_case_is_exact_in_both_forms(case):
    run_s, run_i, cand_s, cand_i, cand_len, perms = case.inputs()
    es, ei, etau, flag, _ = case.expected()
    k, cap, rows = case.k, case.cap, case.rows
    rc, ns, ni, tau, cl, ov = fold_run(k, cap, run_s, run_i, cand_s, cand_i, cand_len, 0)
    assert rc == T.OK and int(ov.get()[0]) == 0 and (cl.get() == 0).all()
    gi, gs = ni.get().reshape(rows, k), ns.get().reshape(rows, k)
    assert same(gi, ei), (case.id, first_diff(gi, ei))
    assert same(gs, es) and same(tau.get(), etau), case.id
    us, ui = cand_s.copy(), cand_i.copy()                                  # the same candidates in a fixed scrambled arrival order
    for r, p in enumerate(perms):
        us[r, : len(p)], ui[r, : len(p)] = cand_s[r, p], cand_i[r, p]
    rc, ns, ni, tau, cl, ov = fold_run(k, cap, run_s, run_i, us, ui, cand_len, 1)
    assert rc == T.OK and (cl.get() == 0).all()
    assert int(ov.get()[0]) == flag, (case.id, "flag", flag)
    ns.get(), ni.get()
    if not flag:
        gi, gs = ni.get().reshape(rows, k), ns.get().reshape(rows, k)
        assert same(gi, ei), (case.id, "unordered", first_diff(gi, ei))
        assert same(gs, es) and same(tau.get(), etau), (case.id, "unordered")


# ---- merge -------------------------------------------------------------------------------------------------------------------------------
def merge_run(s, i, G=None, k=None):
    L, st = _abi()
    g0, rows, k0 = s.shape
    G, k = G or g0, k or k0
    ds, di = dev(s), dev(i)
    os_, oi = Out(rows * k0, np.float32, T.S_GUARD), Out(rows * k0, np.int64, T.I_GUARD)
    rc = L.fz_topk_merge(ptr(ds), ptr(di), G, rows, k, os_.p, oi.p, st)
    torch.cuda.synchronize()
    return rc, os_, oi


@pytest.mark.parametrize("case", T.MERGE_CASES, ids=lambda c: c.id)
def test_merge_case_is_exact(case):
    s, i = case.inputs()
    es, ei = T.merge_ref(s, i)
    rc, os_, oi = merge_run(s, i)
    assert rc == T.OK
    gi, gs = oi.get().reshape(ei.shape), os_.get().reshape(es.shape)
    assert same(gi, ei), (case.id, first_diff(gi, ei))
    assert same(gs, es), (case.id, first_diff(gs, es))


def test_merge_refusals_and_no_rows(ops):
    s, i = np.zeros((1, 1, 8), dtype=np.float32), np.zeros((1, 1, 8), dtype=np.int64)
    for G, k in T.MERGE_REFUSED:                                           # refused on the arguments alone: nothing is read or written
        rc, os_, oi = merge_run(s, i, G=G, k=k)
        assert rc == T.ERR_UNSUPPORTED and os_.untouched() and oi.untouched(), (G, k)
    rc, os_, oi = merge_run(s, i, G=-1)
    assert rc == T.ERR_ARG and os_.untouched()
    L, st = _abi()
    assert L.fz_topk_merge(None, None, 3, 0, 7, None, None, st) == T.OK
    e = ops.topk_merge(torch.empty((3, 0, 7), device="cuda"), torch.empty((3, 0, 7), dtype=torch.int64, device="cuda"))
    assert tuple(e[0].shape) == (0, 7) and tuple(e[1].shape) == (0, 7)


# ---- select ------------------------------------------------------------------------------------------------------------------------------
def guarded_plane(a, fill):
    """a [rows, N] inside a plane of `fill`: 64 columns behind every row and two rows after the last."""
    rows, N = a.shape
    ld = -(-N // 64) * 64 + 64
    p = torch.full((rows + 2, ld), fill, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    p[:rows, :N] = torch.from_numpy(a)
    return p[:rows, :N]


@pytest.mark.parametrize("case", T.SELECT_CASES, ids=lambda c: c.id)
def test_select_case_is_exact(ops, case):
    x, pos = case.inputs()
    k, cap = T.SELECT_K, case.cap
    rows, N = x.shape
    fused = guarded_plane(x, np.inf)                                       # a column read past N: +inf, listed at position 0
    pos_d = None if pos is None else guarded_plane(pos, 0)
    assert ops.as_plane(fused) is fused
    # the raw entry: candidate counts and the flag as the kernel's own bisection gives them (select_sim), nothing written past cap
    L, st = _abi()
    cc, cv = Out(rows * cap, np.int32, T.I_GUARD), Out(rows * cap, x.dtype, T.S_GUARD)
    cn, cl, ov = Out(rows * cap, np.float32, T.S_GUARD), Out(rows, np.int32, T.I_GUARD), Out(1, np.int32, T.I_GUARD, [0])
    rc = L.fz_select_topk_f(ptr(fused), case.bits, None if pos_d is None else ptr(pos_d), rows, N, fused.stride(0), k, cap, cc.p, cv.p, cn.p, cl.p, ov.p, st)
    torch.cuda.synchronize()
    sims = case.sims()
    assert rc == T.OK and int(ov.get()[0]) == int(case.over)
    assert np.array_equal(cl.get(), [min(c, cap) for c, _ in sims]), (case.id, cl.get(), sims)
    gc, gv = cc.get().reshape(rows, cap), cv.get().reshape(rows, cap)
    for r in range(rows):
        m = int(cl.get()[r])
        assert (gc[r, m:] == T.I_GUARD).all() and len(set(gc[r, :m].tolist())) == m
        assert same(gv[r, :m], x[r, gc[r, :m]])                            # the candidates keep their own score bits
    # ops.select_topk widens cap to its candidate planes' row stride: None exactly when a row's count exceeds THAT
    eff = ops._ld(ops.alloc_plane(2, cap, torch.int32, "cuda"))
    assert eff == case.eff_cap      # (test_topk_cases_cpu.py: the cases fill eff_cap exactly, pass it by one, and fall between cap and it)
    got = ops.select_topk(fused, pos_d, k, cap)
    if any(c > eff for c, _ in case.sims(eff)):
        assert got is None, case.id
        return
    assert got is not None and (eff > cap or not case.over), case.id
    cols, sc, lens = (t.cpu().numpy() for t in got)
    ec, es, el = T.select_ref(x, pos, k)
    assert np.array_equal(lens, el), (case.id, lens, el)
    assert np.array_equal(cols, ec), (case.id, first_diff(cols, ec))
    for r in range(rows):
        assert same(sc[r, : el[r]], es[r, : el[r]]), (case.id, r)


def test_select_refuses_a_row_longer_than_one_workgroup(ops):
    N = T.SELECT_MAX_N + 1
    x = np.zeros((1, N), dtype=np.float32)
    assert ops.select_topk(guarded_plane(x, np.inf), None, 10) is None
    L, st = _abi()
    d = dev(x)
    outs = [Out(50, np.int32, T.I_GUARD), Out(50, np.float32, T.S_GUARD), Out(50, np.float32, T.S_GUARD), Out(1, np.int32, T.I_GUARD), Out(1, np.int32, T.I_GUARD, [0])]
    rc = L.fz_select_topk_f(ptr(d), 32, None, 1, N, N, 10, 50, *(o.p for o in outs), st)
    torch.cuda.synchronize()
    assert rc == T.ERR_UNSUPPORTED and all(o.untouched() for o in outs)


# ---- every documented refusal ------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_outputs_lengths_and_thresholds_as_they_were():
    L, st = _abi()
    rows, n, k, cap = 2, 300, 8, 16
    sc = dev(np.zeros((rows, n), dtype=np.float32))
    run_s, run_i = dev(np.zeros((rows, 5057), dtype=np.float32)), dev(np.zeros((rows, 5057), dtype=np.int64))
    big = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    f = lambda: Out(rows * 64, np.float32, T.S_GUARD)
    i64 = lambda: Out(rows * 64, np.int64, T.I_GUARD)
    ln = lambda: Out(rows, np.int32, T.I_GUARD, [3, 5])
    ov = lambda: Out(1, np.int32, T.I_GUARD, [0])

    def check(rc, want, outs, what):
        torch.cuda.synchronize()
        assert rc == want and all(o.untouched() for o in outs), (what, rc, want)

    a, b = f(), i64()
    check(L.fz_topk_rows_f32(ptr(sc), rows, n, n - 1, k, 0, a.p, b.p, ptr(big), big.numel(), st), T.ERR_ARG, (a, b), "rows: ld < n")
    check(L.fz_topk_rows_f32(ptr(sc), rows, n, n, 0, 0, a.p, b.p, ptr(big), big.numel(), st), T.ERR_ARG, (a, b), "rows: k = 0")
    check(L.fz_topk_rows_f32(ptr(sc), rows, n, n, T.MAX_K + 1, 0, a.p, b.p, ptr(big), big.numel(), st), T.ERR_UNSUPPORTED, (a, b), "rows: k")
    c = ov()
    check(L.fz_topk_update_f32(ptr(sc), rows, n, n, 0, ptr(run_s), ptr(run_i), 35000, 841, a.p, b.p, c.p, ptr(big), big.numel(), st), T.ERR_UNSUPPORTED,
          (a, b, c), "update: k + cap")
    check(L.fz_topk_update_f32(ptr(sc), rows, n, n, 0, ptr(run_s), ptr(run_i), k, 0, a.p, b.p, c.p, ptr(big), big.numel(), st), T.ERR_ARG, (a, b, c), "update: cap")
    check(L.fz_topk_update_f32(ptr(sc), rows, n, n, 0, ptr(run_s), ptr(run_i), k, cap, a.p, b.p, c.p, ptr(big),
                               L.fz_topk_update_workspace_bytes(rows, k, cap) - 1, st), T.ERR_WORKSPACE, (a, b, c), "update: workspace")
    tau, cl = Out(rows, np.float32, T.S_GUARD, [1.0, 2.0]), ln()
    check(L.fz_topk_filter_append_f32(ptr(sc), rows, n, n, 0, tau.p, a.p, b.p, cl.p, 0, c.p, st), T.ERR_ARG, (a, b, c, cl, tau), "append: cap")
    check(L.fz_topk_filter_append_f32(ptr(sc), rows, n, n - 1, 0, tau.p, a.p, b.p, cl.p, cap, c.p, st), T.ERR_ARG, (a, b, c, cl, tau), "append: ld")
    check(L.fz_topk_filter_append_f32(ptr(sc), rows, n, n, 0, None, a.p, b.p, cl.p, cap, c.p, st), T.ERR_ARG, (a, b, c, cl, tau), "append: tau")
    cs, ci = dev(np.zeros((rows, cap), dtype=np.float32)), dev(np.zeros((rows, cap), dtype=np.int64))
    ns, ni = Out(rows * 5057, np.float32, T.S_GUARD), Out(rows * 5057, np.int64, T.I_GUARD)
    fold = lambda k_, cap_, unordered, ovp, wsb: L.fz_topk_fold_f32(ptr(run_s), ptr(run_i), rows, k_, ptr(cs), ptr(ci), cl.p, cap_, unordered, ns.p, ni.p,
                                                                     tau.p, ovp, ptr(big), wsb, st)
    outs = (ns, ni, cl, tau, c)
    check(fold(35000, 841, 0, c.p, big.numel()), T.ERR_UNSUPPORTED, outs, "fold: k + cap")
    assert L.fz_topk_fold_workspace_bytes(rows, 5057, cap) <= big.numel()
    check(fold(5057, cap, 1, c.p, big.numel()), T.ERR_UNSUPPORTED, outs, "fold: unordered k beyond fz_topk_fold_max_k")      # once refused after two launches
    check(fold(k, cap, 1, None, big.numel()), T.ERR_ARG, outs, "fold: unordered without a flag")
    check(fold(k, cap, 0, c.p, L.fz_topk_fold_workspace_bytes(rows, k, cap) - 1), T.ERR_WORKSPACE, outs, "fold: workspace")
    check(L.fz_topk_merge(ptr(run_s), ptr(run_i), 0, rows, k, a.p, b.p, st), T.ERR_ARG, (a, b), "merge: G")
    check(L.fz_topk_merge(ptr(run_s), ptr(run_i), 1, rows, T.SORT_ROW_F32 + 1, a.p, b.p, st), T.ERR_UNSUPPORTED, (a, b), "merge: G * k")
    cc, cn = Out(rows * 64, np.int32, T.I_GUARD), f()
    sel = lambda bits_, n_, ld_, k_, cap_: L.fz_select_topk_f(ptr(sc), bits_, None, rows, n_, ld_, k_, cap_, cc.p, a.p, cn.p, cl.p, c.p, st)
    outs = (cc, a, cn, cl, c)
    check(sel(16, n, n, 4, 8), T.ERR_ARG, outs, "select: key bits")
    check(sel(32, n, n - 1, 4, 8), T.ERR_ARG, outs, "select: ld")
    check(sel(32, n, n, 8, 4), T.ERR_ARG, outs, "select: cap < k")
    check(sel(32, T.SELECT_MAX_N + 1, T.SELECT_MAX_N + 1, 4, 8), T.ERR_UNSUPPORTED, outs, "select: n")


def test_topk_stream_refuses_an_unordered_source_beyond_the_fold_s_k(ops):
    k = ops.fold_max_k(True) + 1
    run_s = torch.zeros((2, k), device="cuda")
    run_i = torch.arange(k, device="cuda").repeat(2, 1)
    st = ops.TopkStream(run_s, run_i, seen=k, cap=100)
    Qn, Dn = torch.ones((2, 8), device="cuda"), torch.ones((50, 8), device="cuda")
    with pytest.raises(ValueError, match=str(k - 1)):
        st.feed_gemm(Qn, Dn, k)
    torch.cuda.synchronize()
    assert int(st.cand_len.sum()) == 0 and st.pending == 0 and not st.unordered and int(st.overflow.item()) == 0      # nothing was launched or latched
    st.feed(torch.ones((2, 30), device="cuda"), k)                         # ordered candidates at this k are taken
    bs, bi, over = st.result()
    assert int(over.item()) == 0 and torch.equal(bi[:, :30].cpu(), (k + torch.arange(30)).repeat(2, 1))


# ---- the precondition of the streamed forms --------------------------------------------------------------------------------------------
def test_short_list_and_minus_inf_as_documented(ops):
    """include/fusion_hip.h (fz_topk_update_f32): against a SHORT running list (tau = -inf) a later score of exactly -inf is dropped and
    stays (-inf, -1) padding, where the top-k of the whole matrix lists its id; with a full list, or no -inf score, the streamed forms
    equal the whole-matrix top-k.  Both forms, pinned as stated."""
    k, head, n = 8, 3, 6
    whole = np.array([[1.0, 0.5, 2.0, -np.inf, 4.0, -np.inf, 3.0, -1.0, -np.inf]], dtype=np.float32)
    hs, hi = T.topk_ref(whole[:, :head], k, 0)                             # three real entries, five (-inf, -1)
    ws, wi = T.topk_ref(whole, k, 0)
    stated_i = np.where(np.isneginf(ws), -1, wi)                           # ... the whole-matrix list with its -inf documents as padding
    assert (wi[0, -2:] == [3, 5]).all() and (stated_i[0, -2:] == -1).all()
    piece = dev(whole[:, head:])
    ns, ni, over = ops.topk_update(piece, head, dev(hs), dev(hi), cap=16)
    assert same(ni.cpu().numpy(), stated_i) and same(ns.cpu().numpy(), ws) and int(over.item()) == 0
    st = ops.TopkStream(dev(hs), dev(hi), seen=head, cap=16)
    st.feed(piece, head)
    bs, bi, over = st.result()
    assert same(bi.cpu().numpy(), stated_i) and same(bs.cpu().numpy(), ws) and int(over.item()) == 0
    # a full list: the -inf documents cannot enter either way, the forms agree with the whole matrix
    k = 2
    hs, hi = T.topk_ref(whole[:, :head], k, 0)
    ws, wi = T.topk_ref(whole, k, 0)
    ns, ni, _ = ops.topk_update(piece, head, dev(hs), dev(hi), cap=16)
    assert same(ni.cpu().numpy(), wi) and same(ns.cpu().numpy(), ws)
    # a short list and no -inf score: the whole-matrix list
    k, fin = 8, np.where(np.isneginf(whole), np.float32(-7.0), whole)
    hs, hi = T.topk_ref(fin[:, :head], k, 0)
    ws, wi = T.topk_ref(fin, k, 0)
    ns, ni, _ = ops.topk_update(dev(fin[:, head:]), head, dev(hs), dev(hi), cap=16)
    assert same(ni.cpu().numpy(), wi) and same(ns.cpu().numpy(), ws)


# ---- end to end: one uncut piece of more than a round ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_row():
    """[3, 4,096 + 131,077] scores on a 1/1024 grid (ties), NaN and +-0 entries; the NumPy top-k of the whole rows."""
    rng = np.random.default_rng(6)
    x = (np.round(rng.normal(0, 1, (3, 4096 + 131077)) * 1024) / 1024).astype(np.float32)
    x[1, [5000, 70000, 135172]] = np.nan
    x[2, 4096 + 65535: 4096 + 65537] = x[2].max()                          # the best value on both sides of the piece's round border
    return x, T.topk_ref(x, 10, T.ID_BASE)


def wide(x):
    """x on the device with a row stride that is a multiple of four floats and +inf behind every row: its column slices from a multiple
    of four take the filter's 16-byte path."""
    p = torch.full((x.shape[0] + 1, -(-x.shape[1] // 4) * 4 + 4), float("inf"), device="cuda")
    p[: x.shape[0], : x.shape[1]] = torch.from_numpy(x)
    return p[: x.shape[0], : x.shape[1]]


def test_stream_feed_of_one_uncut_piece(ops, long_row):
    x, (es, ei) = long_row
    k, cap, head = 10, 7168, 4096
    n = x.shape[1] - head
    assert ops.stream_pieces(0, n, head, 0, k, cap) == [(0, n, False)] and n > T.SPAN      # one filter launch over two rounds and 5 columns
    d = wide(x)
    hs, hi = ops.topk_rows(d[:, :head], k, id_base=T.ID_BASE)
    st = ops.TopkStream(hs, hi, seen=head, cap=cap)
    st.feed(d[:, head:], T.ID_BASE + head)
    assert 0 < int(st.cand_len.max()) < cap
    bs, bi, over = st.result()
    assert int(over.item()) == 0 and st.windows_redone == 0
    assert same(bi.cpu().numpy(), ei) and same(bs.cpu().numpy(), es)


def test_topk_update_of_one_piece_of_more_than_a_round(ops, long_row):
    x, (es, ei) = long_row
    k, head = 10, 4096
    d = wide(x)
    hs, hi = ops.topk_rows(d[:, :head], k, id_base=T.ID_BASE)
    ns, ni, over = ops.topk_update(d[:, head:], T.ID_BASE + head, hs, hi, cap=7168)
    assert int(over.item()) == 0 and same(ni.cpu().numpy(), ei) and same(ns.cpu().numpy(), es)
    ws, wi = ops.topk_rows(d, k, id_base=T.ID_BASE)                         # ... and the whole rows in one call (two levels)
    assert same(wi.cpu().numpy(), ei) and same(ws.cpu().numpy(), es)
