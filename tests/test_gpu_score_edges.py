"""The score GEMM (csrc/score.hip) and its filter and SPLADE epilogues, bit for bit at every tile edge.

On grid-valued inputs (score_cases.py: multiples of 1/4) every product and partial sum is exact in fp32 in any order, so the bars are
equalities with the float64 product: np.array_equal over the whole score plane, exact candidate sets with equal score bits for the filter,
torch.equal with the pooling of the exact logits plane for the SPLADE head.  Every operand is a view into a larger buffer with NaN behind
every row and NaN ghost rows around the problem, every output a view into a larger sentinel-filled one that must come back untouched
outside [Q, N].  The cases land every branch of score_cases.BRANCHES on this device (test_branch_table_is_covered: the branch sets come
from fz_dot_scores_plan at the device's CU count; the same check runs at 256 CUs without a GPU in test_score_cases_cpu.py).  A second
part runs the product's inputs (unit-norm rows) for the claim of the kernel's header -- a query's scores do not depend on the tile its
row fell into -- over the multi-round, halved-round and cover launches, at the project's 2e-6 bar against float64."""
import ctypes as C

import numpy as np
import pytest
import torch

import score_cases as S

pytestmark = pytest.mark.gpu
GUARD_I = -7                      # guard value of cand_len / cand_ids cells that the kernel must not touch


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def view(ops, a):
    """a [rows, d] float64 on the grid -> its float32 view inside a NaN-framed device buffer, as ops hands it to the kernel (uncopied)."""
    buf, rows, n = S.framed(a)
    v = dev(buf)[rows, :n]
    assert ops.pad_dim(v) is v and v.stride(0) > n, "the operand would be copied: its NaN frame tests nothing"
    return v


def test_branch_table_is_covered():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    hit = set()
    for c in S.ALL_CASES:
        b = S.branches_of(c, cus)
        assert set(c.claims) <= b, (c.id, cus, sorted(map(str, set(c.claims) - b)))
        hit |= b
    assert set(S.BRANCHES) <= hit, (cus, sorted(map(str, set(S.BRANCHES) - hit)))


# ---- store form: the whole plane, and nothing outside it -------------------------------------------------------------------------------
def store(ops, Qv, Dv, top=2, left=3, bottom=3, right=4):
    """ops.dot_scores into a view of a sentinel-filled plane -> (the [Q, N] scores, the number of cells outside them that changed)."""
    Q, N = Qv.shape[0], Dv.shape[0]
    plane = torch.full((top + Q + bottom, left + N + right), float(S.SENTINEL), dtype=torch.float32, device="cuda")
    out = plane[top: top + Q, left: left + N]
    assert ops.dot_scores(Qv, Dv, out=out) is out
    got = plane.cpu().numpy()
    inner = got[top: top + Q, left: left + N].copy()
    got[top: top + Q, left: left + N] = S.SENTINEL
    return inner, int((got != S.SENTINEL).sum())


@pytest.mark.parametrize("case", S.STORE_CASES, ids=lambda c: c.id)
def test_store_case_is_exact(ops, case):
    A, B = case.inputs()
    ref = S.exact_f32(case.ref(A, B))
    got, outside = store(ops, view(ops, A), view(ops, B))
    bad = np.argwhere(got != ref)
    assert np.array_equal(got, ref), (case.id, len(bad), [(int(q), int(j), float(got[q, j]), float(ref[q, j])) for q, j in bad[:8]])
    assert outside == 0, (case.id, f"{outside} cells outside [Q, N] were written")


# ---- store form on the product's inputs: tile independence ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unit(ops):
    Q, N, d = S.UNIT_SHAPE
    rng = np.random.default_rng(20)
    Qn, Dn = dev(S.unit_rows(rng, Q, d)), dev(S.unit_rows(rng, N, d))
    return Qn, Dn, ops.dot_scores(Qn, Dn)      # two whole blocks + a 32-row tail, more ids than slots: whole tiles, then tail tiles


def test_unit_norm_plane_meets_the_float64_bar(ops, unit):
    Qn, Dn, plane = unit
    err = float((plane.double() - Qn.double() @ Dn.double().T).abs().max())
    print(f"unit-norm {tuple(plane.shape)} x d = {Qn.shape[1]}: max |got - float64| = {err:.3e} (bar 2e-6)")
    assert err <= 2e-6


def test_unit_norm_scores_do_not_depend_on_the_round(ops, unit):
    """The multi-round launch == the halved-round launch of its 256 whole-block rows == column chunks that fit one round."""
    Qn, Dn, plane = unit
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Q, N, d = S.UNIT_SHAPE
    p = S.plan(Q, N, d, S.EPI_STORE, cus)
    assert p["full"] + p["tail_ids"] > p["slots"] and p["tail_ids"] and S.plan(256, N, d, S.EPI_STORE, cus)["halves"] > 0
    assert torch.equal(ops.dot_scores(Qn[:256], Dn), plane[:256]), "halved last round"
    step = 8192
    for lo in range(0, N, step):
        hi = min(lo + step, N)
        pc = S.plan(Q, hi - lo, d, S.EPI_STORE, cus)
        assert pc["full"] + pc["tail_ids"] <= pc["slots"] and not pc["halves"]
        assert torch.equal(ops.dot_scores(Qn, Dn[lo:hi]), plane[:, lo:hi]), ("column chunk", lo, hi)


# (first row, last row + 1, columns): every row of the plane moves into every other row class
ROW_SUBSETS = [(0, 1, None), (256, 257, None), (5, 38, None), (100, 164, None), (60, 127, None), (129, 195, None), (130, 226, None), (0, 100, None),
               (150, 257, None), (64, 192, None), (1, 257, None), (0, 195, None), (64, 257, None), (0, 197, 28000), (57, 257, 28000), (33, 257, 28000)]


@pytest.mark.parametrize("a,b,cols", ROW_SUBSETS)
def test_unit_norm_scores_do_not_depend_on_the_row_class(ops, unit, a, b, cols):
    Qn, Dn, plane = unit
    n = Dn.shape[0] if cols is None else cols
    assert torch.equal(ops.dot_scores(Qn[a:b], Dn[:n]), plane[a:b, :n]), (a, b, n)


def test_row_subsets_reach_every_row_class():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, d = S.UNIT_SHAPE[1:]
    seen = set()
    for a, b, cols in ROW_SUBSETS:
        p = S.plan(b - a, N if cols is None else cols, d, S.EPI_STORE, cus)
        seen.add("cover7" if p["cover7"] else f"slab{p['slab_rows']}" if p["slab_rows"] else f"tail{p['tail_rows']}" if p["tail_rows"] else
                 "padded" if (b - a) % 128 else "halves" if p["halves"] else "whole")
    assert {"cover7", "slab1", "slab2", "slab3", "tail32", "tail64", "tail96", "padded", "halves", "whole"} <= seen, sorted(seen)


# ---- filter epilogue: the raw C ABI, exact candidate sets -------------------------------------------------------------------------------
def _abi():
    from fusion_amd import _lib
    return _lib, _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


def filter_run(Qv, Dv, tau, cap):
    """fz_dot_scores_filter_f32 over guarded buffers -> (cand_s, cand_i, cand_len, overflow) as numpy, guard cells included."""
    _lib, L, st = _abi()
    Q, N, d = Qv.shape[0], Dv.shape[0], Qv.shape[1]
    QP = -(-Q // 128) * 128
    tau_pad = torch.full((QP,), float("inf"), dtype=torch.float32, device="cuda")      # TopkStream._alloc's contract
    tau_pad[:Q] = dev(tau)
    cand_s = torch.full((QP + 1, cap), float(S.SENTINEL), dtype=torch.float32, device="cuda")
    cand_i = torch.full((QP + 1, cap), GUARD_I, dtype=torch.int64, device="cuda")
    cand_len = torch.full((QP + 8,), GUARD_I, dtype=torch.int32, device="cuda")
    cand_len[:Q] = 0
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert tau_pad.data_ptr() % 16 == 0
    rc = L.fz_dot_scores_filter_f32(Qv.data_ptr(), Qv.stride(0), Dv.data_ptr(), Dv.stride(0), Q, N, d, S.ID_BASE, tau_pad.data_ptr(),
                                    cand_s.data_ptr(), cand_i.data_ptr(), cand_len.data_ptr(), cap, overflow.data_ptr(), st)
    assert rc == _lib.FZ_OK
    torch.cuda.synchronize()
    return cand_s.cpu().numpy(), cand_i.cpu().numpy(), cand_len.cpu().numpy(), int(overflow.item())


def filter_check(what, exp, bits, got, Q, cap):
    """exp [Q, N] bool and bits [Q, N] uint32 (the expected scores' bit patterns; NaN cells are compared as NaN) against one run."""
    cand_s, cand_i, cand_len, overflow = got
    n = exp.sum(axis=1)
    assert np.array_equal(cand_len[:Q], n), (what, "cand_len", np.flatnonzero(cand_len[:Q] != n)[:8])
    assert (cand_len[Q:] == GUARD_I).all(), (what, "cand_len cells behind row Q were touched", np.flatnonzero(cand_len[Q:] != GUARD_I)[:8] + Q)
    assert (cand_s[Q:] == S.SENTINEL).all() and (cand_i[Q:] == GUARD_I).all(), (what, "candidate rows behind row Q were touched")
    assert overflow == int((n > cap).any()), (what, "overflow", overflow, int(n.max()), cap)
    nan_bits = np.isnan(bits.view(np.float32))
    for q in range(Q):
        m = min(int(n[q]), cap)
        assert (cand_s[q, m:] == S.SENTINEL).all() and (cand_i[q, m:] == GUARD_I).all(), (what, q, "a slot beyond the list was written")
        ids = cand_i[q, :m] - S.ID_BASE
        order = np.argsort(ids, kind="stable")
        ids, sc = ids[order], cand_s[q, :m][order]
        if n[q] <= cap:
            assert np.array_equal(ids, np.flatnonzero(exp[q])), (what, q, "candidate ids")
        else:                                                # an overflowed row: its first cap slots hold distinct members of the set
            assert len(np.unique(ids)) == m and ids.min() >= 0 and ids.max() < exp.shape[1] and exp[q][ids].all(), (what, q, "overflowed row")
        want, isn = bits[q, ids], nan_bits[q, ids]
        assert np.array_equal(sc.view(np.uint32)[~isn], want[~isn]) and np.isnan(sc[isn]).all(), (what, q, "candidate score bits")


def filter_both_capacities(what, Qv, Dv, tau, exp, bits):
    Q = Qv.shape[0]
    cap = max(int(exp.sum(axis=1).max()), 1)                 # from the reference: everything fits ...
    got = filter_run(Qv, Dv, tau, cap)
    filter_check(what + f" cap={cap}", exp, bits, got, Q, cap)
    assert got[3] == 0
    if cap >= 2:                                             # ... and with one slot less the fullest rows overflow
        got = filter_run(Qv, Dv, tau, cap - 1)
        filter_check(what + f" cap={cap - 1}", exp, bits, got, Q, cap - 1)
        assert got[3] == 1


@pytest.mark.parametrize("case", S.FILTER_CASES, ids=lambda c: c.id)
def test_filter_case_is_exact(ops, case):
    A, B = case.inputs()
    ref = case.ref(A, B)
    tau = case.thresholds(ref)
    filter_both_capacities(case.id, view(ops, A), view(ops, B), tau, case.expected(ref, tau), S.exact_f32(ref).view(np.uint32))


def test_filter_and_store_compute_the_same_chain(ops):
    """Unit-norm rows: with tau at rank 50 of the store plane, the filter's candidates are {plane > tau} with the plane's bits."""
    Q, N, d = 129, 1283, 64
    rng = np.random.default_rng(21)
    Qn, Dn = dev(S.unit_rows(rng, Q, d)), dev(S.unit_rows(rng, N, d))
    plane = ops.dot_scores(Qn, Dn)
    tau = torch.topk(plane, 50, dim=1).values[:, -1].contiguous()
    P, t = plane.cpu().numpy(), tau.cpu().numpy()
    exp = P > t[:, None]
    assert (exp.sum(axis=1) == 49).all()                     # (no ties at rank 50 in these inputs)
    filter_both_capacities("unit-norm", Qn, Dn, t, exp, np.ascontiguousarray(P).view(np.uint32))


# ---- SPLADE epilogue ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.SPLADE_CASES, ids=lambda c: c.id)
def test_splade_case_is_exact(ops, case):
    X, W, bias, cu, _ = case.inputs()
    logits = case.logits(X, W, bias)
    cu_d = dev(cu)
    got = ops.splade_head_max(view(ops, X), view(ops, W), dev(bias.astype(np.float32)), cu_d)
    assert got.shape == (len(cu) - 1, case.V)
    # (a) the same device log1pf on the same float32 argument: the pooling kernel over the exact logits plane, bit for bit
    unfused = ops.segment_splade_max(dev(S.exact_f32(logits)), cu_d)
    bad = (got != unfused).nonzero()
    assert torch.equal(got, unfused), (case.id, len(bad), [(int(s), int(v), float(got[s, v]), float(unfused[s, v])) for s, v in bad[:8]])
    # (b) float64: pooled values stay below 2, where 5e-7 is about two ulps
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - case.pooled(logits, cu)).max())
    print(f"{case.id}: max |got - log1p(relu(.))| = {err:.3e} (bar 5e-7)")
    assert err <= 5e-7
