"""Score fusion at every branch the C ABI dispatches to (csrc/fuse.hip, csrc/tables.hip), against the CPU oracle.

Each case lands one kernel instantiation on purpose, at the edges where launch_nsf / the elementwise launchers change their choice:
the six register-resident row-kernel bins and their VEC / VALID / DMA variants, the persistent walk past one row per workgroup, the
two-pass form for rows longer than 32,768, the unaligned (scalar) paths of the raw C ABI, 5 to 8 systems, and 65,537 grid rows.
Inputs have partial lists, planted ties and one row holding +inf, -inf or NaN.  Bars are the parity suite's: bit for bit for
rrf / bcf / none / wsum / min-max / percentile-rank, NSF_TOL for z-score, arctan and NCE, -inf and NaN in the same places."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import quantile_table
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NSF_TOL = {"min-max": 0.0, "percentile-rank": 0.0, "z-score": 1e-6, "arctan": 1e-6, "normal-curve-equivalent": 1e-4}
NORMS = tuple(NSF_TOL)
TABLED = ("percentile-rank", "normal-curve-equivalent")

# ---- the dispatch table ------------------------------------------------------------------------------------------------------
# launch_nsf (fuse.hip) runs fuse_nsf_row_kernel<NORM, TT, E4, VEC, VALID, DMA> in the first bin (TT threads, E4 float4 per thread)
# whose TT * E4 * 4 columns hold the row; fz_fuse_nsf_f32 reports longer rows unsupported and ops.fuse_nsf takes the two-pass form.
ROW_BINS = ((256, 1), (256, 4), (512, 4), (1024, 4), (1024, 7), (1024, 8))


def row_kernel(N, norm, aligned, partial):
    """(TT, E4, VEC, VALID, DMA) of the row kernel that fz_fuse_nsf_f32 launches, or "two-pass" past 32,768 columns."""
    for tt, e4 in ROW_BINS:
        if N <= tt * e4 * 4:
            if not aligned:                     # ld % 4 != 0 or a base off 16 bytes: scalar loads and stores, one row per workgroup
                return (tt, e4, False, True, False)
            if not partial:                     # full lists: persistent workgroups, next system prefetched into LDS
                return (tt, e4, True, False, True)
            return (tt, e4, True, True, norm != "min-max")   # partial lists: persistent except for min-max
    return "two-pass"                           # row_stats + fuse_nsf_elem4_kernel / fuse_nsf_elem_kernel


# every path listed here is landed on by at least one case below (test_dispatch_table_is_covered checks it)
DISPATCH = {
    **{(tt, e4, True, False, True): "test_row_kernel_bins[full], test_persistent_walk (min-max)" for tt, e4 in ROW_BINS},
    **{(tt, e4, True, True, True): "test_row_kernel_bins[ranks|bits] (not min-max), test_persistent_walk" for tt, e4 in ROW_BINS},
    **{(tt, e4, True, True, False): "test_row_kernel_bins[ranks|bits] (min-max)" for tt, e4 in ROW_BINS},
    **{(tt, e4, False, True, False): "test_c_abi_layouts[odd] (ld = N)" for tt, e4 in ROW_BINS},
    "two-pass": "test_row_kernel_bins (N = 32,769), test_long_rows",
    ("nsf-stats", "vec"): "fuse_nsf_elem4_kernel: test_c_abi_layouts[aligned], test_many_systems_nsf (stats=, orders=)",
    ("nsf-stats", "scalar"): "fuse_nsf_elem_kernel: test_c_abi_layouts[odd|offset]",
    ("wsum", "vec", "plain"): "fuse_wsum_kernel<true, false>: fz_fuse_none_f64 in test_c_abi_layouts[aligned]",
    ("wsum", "vec", "mixed"): "fuse_wsum_kernel<true, true>: fz_fuse_wsum_f64 in test_c_abi_layouts[aligned]",
    ("wsum", "scalar", "plain"): "fuse_wsum_kernel<false, false>: fz_fuse_none_f64 in test_c_abi_layouts[odd|offset]",
    ("wsum", "scalar", "mixed"): "fuse_wsum_kernel<false, true>: fz_fuse_wsum_f64 in test_c_abi_layouts[odd|offset]",
    ("rank", "vec"): "fuse_rank_kernel<true>: test_c_abi_layouts[aligned], test_many_systems_rank",
    ("rank", "scalar"): "fuse_rank_kernel<false>: test_c_abi_layouts[odd|offset]",
    ("tables", "lds-all"): "fuse_nsf_table_kernel: test_eight_tables, test_c_abi_layouts[aligned] (percentile, NCE)",
    ("tables", "lds-swap"): "tables.hip: test_eight_tables",
}

BIN_N = (1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385, 28672, 28673, 32768, 32769)
VALIDITY = ("full", "ranks", "bits")
WALK_Q = (255, 256, 257, 513, 1000)
WALK_N = (1025, 28673)
WALK_NORMS = (("z-score", True), ("arctan", True), ("min-max", False))   # (norm, one partial system)
LAYOUT_CASES = [("aligned", 1001), ("aligned", 28673), ("offset", 1001), ("offset", 28673)] + \
    [("odd", n) for n in (1001, 4095, 8191, 16383, 28671, 28673)]      # odd ld = N: the scalar row kernel in all six bins


def test_dispatch_table_is_covered():
    hit = set()
    for N in BIN_N:
        for norm in NORMS:
            for v in VALIDITY:
                hit.add(row_kernel(N, norm, True, v != "full"))
    for N in WALK_N:
        for norm, partial in WALK_NORMS:
            k = row_kernel(N, norm, True, partial)
            assert k[4], ("the walk cases must take the persistent kernel", N, norm, k)
            hit.add(k)
    for kind, N in LAYOUT_CASES:
        for norm in NORMS:
            if kind == "aligned" and norm in TABLED:   # 101-entry tables on aligned planes: the all-in-LDS table kernel
                continue
            hit.add(row_kernel(N, norm, kind == "aligned", True))
            hit.add(row_kernel(N, norm, kind == "aligned", False))
        form = "vec" if kind == "aligned" else "scalar"
        hit |= {("nsf-stats", form), ("wsum", form, "plain"), ("wsum", form, "mixed"), ("rank", form)}
    hit |= {("tables", "lds-all"), ("tables", "lds-swap")}   # test_eight_tables asserts ops.last_tables_path
    assert hit == set(DISPATCH), (sorted(map(str, set(DISPATCH) - hit)), sorted(map(str, hit - set(DISPATCH))))


# ---- inputs and comparisons ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(oracle):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plane(a):
    from fusion_amd import ops
    t = ops.alloc_plane(a.shape[0], a.shape[1], torch.from_numpy(a[:0]).dtype, "cuda")
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def systems(seed, S, Q, N, partial=None, special=True):
    """S score planes [Q, N] fp32 with the oracle's stable descending rankings (rank and order planes, lens [S, Q]).  Lists of the
    partial systems (odd s by default; system 0 when S == 1) are cut to 90 / 60 / 25 % by row.  Ties: exact zeros (system 0), values
    rounded to 0.1 (system 2), a tie group in every system.  special: the last row of system 0 holds +inf, -inf or NaN."""
    rng = np.random.default_rng(seed)
    if partial is None:
        partial = {0} if S == 1 else set(range(1, S, 2))
    planes, ranks, orders = [], [], []
    lens = np.full((S, Q), N, dtype=np.int32)
    for s in range(S):
        kind = s % 4
        if kind == 0:
            p = np.maximum(0.0, rng.gamma(0.5, 4.0, (Q, N)) - 2.0)
        elif kind == 1:
            p = rng.uniform(-0.2, 0.9, (Q, N))
        elif kind == 2:
            p = np.round(rng.normal(0.0, 1.0, (Q, N)), 1)
        else:
            p = rng.normal(20.0, 4.0, (Q, N))
        p = p.astype(np.float32)
        p[:, rng.integers(0, N, max(1, N // 40))] = p[0, 0]
        if special and s == 0:
            p[Q - 1, rng.integers(0, N)] = (np.inf, -np.inf, np.nan)[seed % 3]
        o, _, r = O.sort_rows_desc(p, want_rank=True)
        if s in partial:
            L = np.maximum(1, (N * np.array([0.9, 0.6, 0.25])[(np.arange(Q) + s) % 3]).astype(np.int32)).astype(np.int32)
            lens[s] = L
            r[r >= L[:, None]] = -1
            o[np.arange(N)[None, :] >= L[:, None]] = -1
        planes.append(p); ranks.append(r.astype(np.int32)); orders.append(o.astype(np.int32))
    return planes, ranks, orders, lens


def tables_for(planes, P):
    return [quantile_table(p[np.isfinite(p)], P).astype(np.float32) for p in planes]


def oracle_nsf(planes, ranks, w, norm, distr=None):
    if norm in TABLED:   # the transform takes no row statistic: fold the rows into short ones, which the oracle's threads share
        Q, N = planes[0].shape
        n, k = Q * N, 512
        pad = -n % k
        fold = lambda a, fill: np.concatenate([a.ravel(), np.full(pad, fill, a.dtype)]).reshape(-1, k)
        e = O.fuse_nsf([fold(p, 0) for p in planes], None if ranks is None else [None if r is None else fold(r, -1) for r in ranks],
                       w, norm, distr)
        return e.ravel()[:n].reshape(Q, N)
    return O.fuse_nsf(planes, ranks, w, norm, distr)


def check_nsf(got, exp, norm, what=""):
    fin = np.isfinite(exp)
    np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=str(what))
    np.testing.assert_array_equal(got[~fin], exp[~fin], err_msg=str(what))   # -inf (in no list) and NaN in the same places
    if NSF_TOL[norm] == 0.0:
        np.testing.assert_array_equal(got, exp, err_msg=str(what))
    else:
        err = np.max(np.abs(got[fin] - exp[fin]), initial=0.0)
        assert err <= NSF_TOL[norm], (what, norm, err)


def same_bits(got, ref, what):
    """bit for bit (+0 is not -0), NaN in the same places (which operand's NaN an instruction passes on is the hardware's choice)"""
    iv = np.int64 if got.dtype == np.float64 else np.int32
    ok = (got.view(iv) == ref.view(iv)) | (np.isnan(got) & np.isnan(ref))
    assert ok.all(), (what, np.argwhere(~ok)[:5].tolist(), got[~ok][:5], ref[~ok][:5])


def bad_rows(got, exp, norm):
    """rows where got and exp disagree under the norm's bar"""
    fin = np.isfinite(exp)
    special = np.where(fin, np.isfinite(got), (got == exp) | (np.isnan(got) & np.isnan(exp)))
    close = np.abs(np.where(fin, got, 0.0).astype(np.float64) - np.where(fin, exp, 0.0)) <= NSF_TOL[norm]
    return np.flatnonzero(~(special & close).all(axis=1))


# ---- 1. row-kernel bins ------------------------------------------------------------------------------------------------------
P_ROW = 4001   # three tables this long do not fit in LDS: with tables=False the row kernel's global-memory search is what runs


@functools.lru_cache(maxsize=2)
def bins_case(N):
    planes, ranks, _, _ = systems(N, 3, 3, N, partial={1, 2})
    return planes, ranks, tables_for(planes, P_ROW)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("validity", VALIDITY)
@pytest.mark.parametrize("N", BIN_N)
def test_row_kernel_bins(ops, N, validity, norm):
    planes, ranks, distr = bins_case(N)
    w = [0.5, 0.3, 0.2]
    tabled = norm in TABLED
    part = None if validity == "full" else [None, ranks[1], ranks[2]]
    rp = None if part is None else [None, plane(ranks[1]), plane(ranks[2])]
    bits = None
    if validity == "bits":
        bits = [None] + [ops.rank_to_bitmap(r) for r in rp[1:]]
        if N <= 32768 or norm not in ("min-max", "z-score"):   # past 32,768 the statistics are taken over the rank planes
            rp = None
    ops.last_tables_path = None
    got = ops.fuse_nsf([plane(p) for p in planes], rp, w, norm, [dev(d) for d in distr] if tabled else None, valid_bits=bits,
                       tables=False).cpu().numpy()
    if tabled:
        assert ops.last_tables_path == "row"
    check_nsf(got, oracle_nsf(planes, part, w, norm, distr if tabled else None), norm, row_kernel(N, norm, True, part is not None))


# ---- 2. the persistent walk --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def walk_case(Q, N):
    """three planes; the partial system's validity: a density per row, row 0 lists nothing, row 1 one column; the last row of
    system 0 holds +inf and NaN"""
    rng = np.random.default_rng(Q * 7 + N)
    planes = [np.maximum(0.0, rng.gamma(0.5, 4.0, (Q, N)) - 2.0).astype(np.float32),
              rng.normal(20.0, 4.0, (Q, N)).astype(np.float32),
              np.round(rng.uniform(-1.0, 1.0, (Q, N)), 2).astype(np.float32)]
    planes[0][Q - 1, 3] = np.inf
    planes[0][Q - 1, N - 2] = np.nan
    valid = rng.random((Q, N)) < rng.uniform(0.05, 1.0, (Q, 1))
    valid[0] = False
    valid[1] = False
    valid[1, N - 1] = True
    return planes, np.where(valid, 0, -1).astype(np.int32)


@pytest.mark.parametrize("S", (1, 2, 3))
@pytest.mark.parametrize("Q", WALK_Q)
@pytest.mark.parametrize("N", WALK_N)
def test_persistent_walk(ops, N, Q, S):
    """DMA row kernels run min(Q, 256) persistent workgroups; workgroup g takes rows g, g + 256, ... and prefetches the next row's
    system 0 while it finishes the current one.  Compared row by row: a failure names the workgroup and the walk step."""
    planes, rank = walk_case(Q, N)
    planes = planes[:S]
    w = [0.45, 0.35, 0.2][:S]
    dp = [plane(p) for p in planes]
    rk = [None] * (S - 1) + [rank]            # the last system is the partial one
    rp = [None] * (S - 1) + [plane(rank)]
    grid = min(Q, 256)
    for norm, partial in WALK_NORMS:
        got = ops.fuse_nsf(dp, rp if partial else None, w, norm).cpu().numpy()
        exp = O.fuse_nsf(planes, rk if partial else None, w, norm)
        bad = bad_rows(got, exp, norm)
        if len(bad):
            q = int(bad[0])
            raise AssertionError(f"{norm}, {row_kernel(N, norm, True, partial)}: {len(bad)} rows differ, first row {q} "
                                 f"(workgroup {q % grid}, walk step {q // grid}): got {got[q][:8]}, expected {exp[q][:8]}")


# ---- 3. five to eight systems --------------------------------------------------------------------------------------------------
MANY_S = (5, 6, 7, 8)
MANY_N = (1000, 27942)


@functools.lru_cache(maxsize=2)
def many_case(S, N):
    return systems(S * 1000 + N, S, 3, N)


def partial_of(ranks, S):
    return [r if s % 2 == 1 else None for s, r in enumerate(ranks)]


def inverse(ins, U, N):
    inv = np.full((ins.shape[0], N), -1, dtype=np.int32)
    for q in range(ins.shape[0]):
        inv[q, ins[q, : U[q]]] = np.arange(U[q], dtype=np.int32)
    return inv


@pytest.mark.parametrize("N", MANY_N)
@pytest.mark.parametrize("S", MANY_S)
def test_many_systems_rank(ops, S, N):
    """fuse_rank, sort_rank_fused (gathered and placed) and insertion_order at 5-8 systems"""
    _, ranks, orders, lens = many_case(S, N)
    rp, L = [plane(r) for r in ranks], dev(lens)
    ins, U = ops.insertion_order([plane(o) for o in orders], L, N)
    e_ins, e_U = O.insertion_order(orders, lens, N)
    np.testing.assert_array_equal(U.cpu().numpy(), e_U)
    g = ins.cpu().numpy()
    for q in range(len(e_U)):
        np.testing.assert_array_equal(g[q, : e_U[q]], e_ins[q, : e_U[q]])
    inv = plane(inverse(e_ins, e_U, N))
    for method in ("rrf", "bcf"):
        f = O.fuse_rank(ranks, lens, method)
        np.testing.assert_array_equal(ops.fuse_rank(rp, L, method).cpu().numpy(), f)
        eo, esk, erk = O.sort_rows_desc(f, init_order=e_ins, row_len=e_U, want_rank=True)
        for form, kw in (("gathered", dict(init_order=ins)), ("placed", dict(init_rank=inv))):
            o, sk, rk = ops.sort_rank_fused(rp, L, method, row_len=U, want_rank=True, **kw)
            np.testing.assert_array_equal(o.cpu().numpy(), eo, err_msg=f"{method} {form}")
            np.testing.assert_array_equal(sk.cpu().numpy(), esk, err_msg=f"{method} {form}")
            np.testing.assert_array_equal(rk.cpu().numpy(), erk, err_msg=f"{method} {form}")


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("N", MANY_N)
@pytest.mark.parametrize("S", MANY_S)
def test_many_systems_nsf(ops, S, N, norm):
    """fuse_nsf at 5-8 systems: full lists, partial lists as rank planes and as bitmaps, min-max from the lists' ends (orders=),
    and statistics handed in (stats=, concatenated and per system)"""
    planes, ranks, orders, lens = many_case(S, N)
    Q = planes[0].shape[0]
    part = partial_of(ranks, S)
    w = np.random.default_rng(S + N).dirichlet(np.ones(S)).tolist()
    tabled = norm in TABLED
    distr = tables_for(planes, 101) if tabled else None
    dd = [dev(d) for d in distr] if tabled else None
    dp = [plane(p) for p in planes]
    rp = [None if r is None else plane(r) for r in part]
    bits = [None if r is None else ops.rank_to_bitmap(r) for r in rp]
    e_full = oracle_nsf(planes, None, w, norm, distr)
    e_part = oracle_nsf(planes, part, w, norm, distr)
    check_nsf(ops.fuse_nsf(dp, None, w, norm, dd).cpu().numpy(), e_full, norm, "full")
    check_nsf(ops.fuse_nsf(dp, rp, w, norm, dd).cpu().numpy(), e_part, norm, "rank planes")
    check_nsf(ops.fuse_nsf(dp, None, w, norm, dd, valid_bits=bits).cpu().numpy(), e_part, norm, "bitmaps")
    if norm == "min-max":
        got = ops.fuse_nsf(dp, rp, w, norm, orders=[plane(o) for o in orders], lens=dev(lens)).cpu().numpy()
        check_nsf(got, e_part, norm, "orders")
    if norm in ("min-max", "z-score"):
        st = [O.row_stats(p, r, norm) for p, r in zip(planes, part)]
        sa, sb = dev(np.concatenate([a for a, _ in st])), dev(np.concatenate([b for _, b in st]))
        check_nsf(ops.fuse_nsf(dp, rp, w, norm, stats=(sa, sb)).cpu().numpy(), e_part, norm, "stats, concatenated")
        per = [(sa[s * Q:(s + 1) * Q].clone(), sb[s * Q:(s + 1) * Q].clone()) for s in range(S)]
        check_nsf(ops.fuse_nsf(dp, None, w, norm, stats=per, valid_bits=bits).cpu().numpy(), e_part, norm, "stats, per system")


def mixed_wsum_inputs(planes, S):
    """float64 planes (odd s) between float32 ones, and narrow weights (even s but 4) between wide ones: a document's sum stays
    float32 until its first wide product, which comes at s = 1 for documents system 1 lists and later for the others"""
    mixed = [p.astype(np.float64) * (1.0 + 2.0 ** -40) if s % 2 == 1 else p for s, p in enumerate(planes)]
    narrow = [s % 2 == 0 and s != 4 for s in range(S)]
    return mixed, narrow


@pytest.mark.parametrize("N", MANY_N)
@pytest.mark.parametrize("S", MANY_S)
def test_many_systems_none_and_wsum(ops, S, N):
    planes, ranks, _, _ = many_case(S, N)
    part = partial_of(ranks, S)
    rp = [None if r is None else plane(r) for r in part]
    w = np.random.default_rng(N - S).uniform(0.05, 1.0, S).tolist()
    got = ops.fuse_none([plane(p) for p in planes], rp, w).cpu().numpy()
    np.testing.assert_array_equal(got, O.fuse_none(planes, part, w))
    mixed, narrow = mixed_wsum_inputs(planes, S)
    got = ops.fuse_wsum([plane(p) for p in mixed], rp, w, narrow=narrow).cpu().numpy()
    np.testing.assert_array_equal(got, O.fuse_wsum(mixed, part, w, narrow))


@pytest.mark.parametrize("norm", TABLED)
@pytest.mark.parametrize("P,path", [(501, "lds-all"), (27943, "lds-swap")])
def test_eight_tables(ops, P, path, norm):
    """eight quantile tables: all of them in LDS at once (8 x 501 entries just fit), or one at a time (27,943 entries each)"""
    planes, ranks, _, _ = many_case(8, 1000)
    part = partial_of(ranks, 8)
    distr = tables_for(planes, P)
    w = np.random.default_rng(P).dirichlet(np.ones(8)).tolist()
    ops.last_tables_path = None
    got = ops.fuse_nsf([plane(p) for p in planes], [None if r is None else plane(r) for r in part], w, norm,
                       [dev(d) for d in distr]).cpu().numpy()
    assert ops.last_tables_path == path
    check_nsf(got, oracle_nsf(planes, part, w, norm, distr), norm, path)


@pytest.mark.parametrize("S,norm,partial", [(5, "min-max", True), (8, "z-score", True), (8, "arctan", False)])
def test_tune_equals_fuse_per_weight_many_systems(ops, S, norm, partial):
    """Aggregator.tune == fuse + sort + Metrics per weight vector, past the four systems of the one-launch sweep"""
    from fusion_amd.planes import RankedSystem
    from fusion_amd.retrievers.hybrid import Aggregator, run_evaluation
    rng = np.random.default_rng(S * 5 + len(norm))
    Q, N = 9, 700
    planes, _, _, lens = systems(S * 5 + len(norm), S, Q, N, partial=None if partial else set(), special=False)
    for p in planes:
        p[:, ::7] = np.round(p[:, ::7], 1)
    ids = np.arange(5000, 5000 + N)
    names = [f"sys{i}" for i in range(S)]
    systems_ = {}
    for n, p, l in zip(names, planes, lens):
        pl = plane(p)
        od, _, rk = ops.sort_rows_desc(pl, want_rank=True)
        L = torch.from_numpy(l).cuda()
        full = bool((l == N).all())
        if not full:
            keep = torch.arange(N, device="cuda").unsqueeze(0) < L.unsqueeze(1)
            rk = torch.where(rk < L.unsqueeze(1), rk, torch.full_like(rk, -1))
            od = torch.where(keep, od, torch.full_like(od, -1))
        systems_[n] = RankedSystem(scores=pl, order=od, rank=rk, lens=L, ids=ids, full=full)
    labels = [rng.choice(ids, size=int(rng.integers(1, 12)), replace=False).tolist() for _ in range(Q)]
    labels[0] = labels[0] + [123456789]
    grid = [dict(zip(names, rng.dirichlet(np.ones(S)).tolist())) for _ in range(3)]
    grid.append({n: (1.0 if i == S - 1 else 0.0) for i, n in enumerate(names)})
    got = Aggregator.tune(systems_, norm, grid, labels, {})
    for w, g in zip(grid, got):
        fused = Aggregator.fuse(systems_, "nsf", norm, w, {}, as_device=True)
        exp = run_evaluation(fused.predictions(1000), labels, print2console=False)
        assert list(g) == list(exp)
        for k in exp:
            assert g[k] == pytest.approx(float(exp[k]), rel=0, abs=1e-12), (w, k)


# ---- 4. more than eight systems ------------------------------------------------------------------------------------------------
def test_nine_systems_are_refused_on_the_device(ops):
    from fusion_amd.retrievers.hybrid import Aggregator
    f = [torch.zeros((2, 5), device="cuda") for _ in range(9)]
    i = [torch.zeros((2, 5), dtype=torch.int32, device="cuda") for _ in range(9)]
    lens = torch.full((9, 2), 5, dtype=torch.int32, device="cuda")
    calls = [lambda: ops.fuse_rank(i, lens, "rrf"), lambda: ops.sort_rank_fused(i, lens, "bcf"),
             lambda: ops.fuse_nsf(f, None, [0.1] * 9, "min-max"), lambda: ops.fuse_none(f, None, [0.1] * 9),
             lambda: ops.fuse_wsum(f, None, [0.1] * 9), lambda: ops.insertion_order(i, lens, 5),
             lambda: Aggregator.fuse({f"s{k}": [[{"corpus_id": 1, "score": 1.0}]] for k in range(9)}, "rrf")]
    for call in calls:
        with pytest.raises(ValueError, match="at most 8"):
            call()


# ---- 5, 6. the raw C ABI at every layout, and no stray writes ------------------------------------------------------------------
class Layout:
    """[Q, N] planes in buffers of Q + 1 rows of ld elements, starting `off` elements in: aligned (ld a multiple of 64), odd (ld = N),
    offset (aligned ld, every base one element past a 16-byte boundary)"""

    def __init__(self, kind, Q, N):
        from fusion_amd import ops
        self.kind, self.Q, self.N = kind, Q, N
        self.ld = N if kind == "odd" else ops.round_up(N, 64)
        self.off = 1 if kind == "offset" else 0
        self.vec = kind == "aligned"

    def buf(self, a=None, dtype=None, fill=0):
        dtype = dtype if a is None else torch.from_numpy(a[:0]).dtype
        b = torch.full((self.off + (self.Q + 1) * self.ld,), fill, dtype=dtype, device="cuda")
        if a is not None:
            self.rows(b).copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return b

    def rows(self, b):
        return b[self.off:self.off + self.Q * self.ld].view(self.Q, self.ld)[:, :self.N]

    def ptr(self, b):
        return None if b is None else b.data_ptr() + self.off * b.element_size()

    def sentinel_out(self, dtype):
        b = self.buf(dtype=dtype, fill=float("nan"))
        return b, b.clone()

    def assert_untouched(self, b, before, width, what):
        """nothing changed outside each row's [0, width): not the row padding, the extra row or the elements before the base"""
        iv = torch.int64 if b.element_size() == 8 else torch.int32
        changed = b.view(iv) != before.view(iv)
        outside = torch.ones_like(changed)
        outside[self.off:self.off + self.Q * self.ld].view(self.Q, self.ld)[:, :width] = False
        n = int((changed & outside).sum())
        assert n == 0, f"{what}: {n} elements written outside the rows' first {width} columns ({self.kind}, ld = {self.ld})"


def _arr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


@pytest.mark.parametrize("kind,N", LAYOUT_CASES)
def test_c_abi_layouts(ops, kind, N):
    """fz_fuse_nsf_f32 (every norm, partial and full), fz_fuse_nsf_stats_f32, fz_fuse_none_f64, fz_fuse_wsum_f64 and fz_fuse_rank_f64
    called through ctypes as a non-Python host binds them, at the three layouts: the oracle's result, the aligned ops
    path's bits, and no write outside [0, N) of a row (the float4 kernels may fill the last float4: [0, round_up(N, 4)))"""
    from fusion_amd import _lib
    L = _lib.lib()
    Q, S = 3, 3
    planes, ranks, _, lens = systems(N + 11, S, Q, N, partial={1, 2})
    part = [None, ranks[1], ranks[2]]
    lay = Layout(kind, Q, N)
    pb = [lay.buf(p) for p in planes]
    rb = [None if r is None else lay.buf(r, fill=-1) for r in part]
    pp, rr = _arr([lay.ptr(b) for b in pb]), _arr([lay.ptr(b) for b in rb])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = [0.5, 0.3, 0.2]
    wc = (C.c_double * S)(*w)
    wide4 = ops.round_up(N, 4) if lay.vec else N       # what the float4 stores of the nsf kernels may cover
    dp = [plane(p) for p in planes]
    rp = [None if r is None else plane(r) for r in part]
    distr = tables_for(planes, 101)
    dd = [dev(d) for d in distr]
    Pc = (C.c_int32 * S)(*[len(d) for d in distr])

    for norm in NORMS:
        tabled = norm in TABLED
        for partial in (False, True):
            what = f"fz_fuse_nsf_f32 {norm} {'partial' if partial else 'full'}"
            out, before = lay.sentinel_out(torch.float32)
            rc = L.fz_fuse_nsf_f32(pp, rr if partial else None, wc, S, Q, N, lay.ld, _lib.NORMS[norm], _arr([d.data_ptr() for d in dd]) if tabled else None,
                                   Pc if tabled else None, None, 0, lay.ptr(out), st)
            assert rc == 0, (what, rc)
            torch.cuda.synchronize()
            lay.assert_untouched(out, before, wide4, what)
            got = lay.rows(out).cpu().numpy()
            check_nsf(got, oracle_nsf(planes, part if partial else None, w, norm, distr if tabled else None), norm, what)
            ref = ops.fuse_nsf(dp, rp if partial else None, w, norm, dd if tabled else None).cpu().numpy()
            same_bits(got, ref, f"{what}: aligned ops path")

    for norm in ("min-max", "z-score"):
        what = f"fz_fuse_nsf_stats_f32 {norm}"
        st_ = [O.row_stats(p, r, norm) for p, r in zip(planes, part)]
        sa, sb = dev(np.concatenate([a for a, _ in st_])), dev(np.concatenate([b for _, b in st_]))
        out, before = lay.sentinel_out(torch.float32)
        rc = L.fz_fuse_nsf_stats_f32(pp, rr, wc, S, Q, N, lay.ld, _lib.NORMS[norm], None, None, sa.data_ptr(), sb.data_ptr(), None, 0,
                                     lay.ptr(out), st)
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        lay.assert_untouched(out, before, wide4, what)
        got = lay.rows(out).cpu().numpy()
        check_nsf(got, O.fuse_nsf(planes, part, w, norm), norm, what)
        ref = ops.fuse_nsf(dp, rp, w, norm, stats=(sa, sb)).cpu().numpy()
        same_bits(got, ref, f"{what}: aligned ops path")

    out, before = lay.sentinel_out(torch.float64)
    assert L.fz_fuse_none_f64(pp, rr, wc, S, Q, N, lay.ld, lay.ptr(out), st) == 0
    torch.cuda.synchronize()
    lay.assert_untouched(out, before, N, "fz_fuse_none_f64")
    got = lay.rows(out).cpu().numpy()
    np.testing.assert_array_equal(got, O.fuse_none(planes, part, w))
    np.testing.assert_array_equal(got, ops.fuse_none(dp, rp, w).cpu().numpy())

    mixed, narrow = mixed_wsum_inputs(planes, S)
    mb = [lay.buf(p) for p in mixed]
    out, before = lay.sentinel_out(torch.float64)
    rc = L.fz_fuse_wsum_f64(_arr([lay.ptr(b) for b in mb]), (C.c_int32 * S)(*[int(p.dtype == np.float64) for p in mixed]), rr, wc,
                            (C.c_int32 * S)(*[int(x) for x in narrow]), S, Q, N, lay.ld, lay.ptr(out), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    lay.assert_untouched(out, before, N, "fz_fuse_wsum_f64")
    got = lay.rows(out).cpu().numpy()
    np.testing.assert_array_equal(got, O.fuse_wsum(mixed, part, w, narrow))
    np.testing.assert_array_equal(got, ops.fuse_wsum([plane(p) for p in mixed], rp, w, narrow=narrow).cpu().numpy())

    rall = [lay.buf(r, fill=-1) for r in ranks]
    lens_d = dev(lens)
    for method in ("rrf", "bcf"):
        out, before = lay.sentinel_out(torch.float64)
        rc = L.fz_fuse_rank_f64(_arr([lay.ptr(b) for b in rall]), lens_d.data_ptr(), S, Q, N, lay.ld, _lib.RANK_METHODS[method],
                                lay.ptr(out), st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        lay.assert_untouched(out, before, N, f"fz_fuse_rank_f64 {method}")
        got = lay.rows(out).cpu().numpy()
        np.testing.assert_array_equal(got, O.fuse_rank(ranks, lens, method))
        np.testing.assert_array_equal(got, ops.fuse_rank([plane(r) for r in ranks], lens_d, method).cpu().numpy())


@pytest.mark.parametrize("P,path", [(101, "lds-all"), (27943, "lds-swap")])
def test_table_kernels_write_only_their_rows(ops, P, path):
    """the quantile-table kernels store float4s: nothing past the last float4 of a row, nothing in the row below"""
    Q, N, S = 3, 1001, 2
    planes, ranks, _, _ = systems(P, S, Q, N)
    distr = [dev(d) for d in tables_for(planes, P)]
    ld = ops.round_up(N, 64)
    for norm in TABLED:
        buf = torch.full((Q + 1, ld), float("nan"), device="cuda")
        before = buf.clone()
        ops.last_tables_path = None
        ops.fuse_nsf([plane(p) for p in planes], [None, plane(ranks[1])], [0.6, 0.4], norm, distr, out=buf[:Q, :N])
        assert ops.last_tables_path == path
        changed = buf.view(torch.int32) != before.view(torch.int32)
        changed[:Q, :ops.round_up(N, 4)] = False
        assert not bool(changed.any()), (norm, path)


# ---- 7. long rows and many rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("N", (32769, 50000))
def test_long_rows(ops, N, norm):
    """rows past the register-resident kernel: row_stats + the flat pass, at five systems, partial lists as rank planes and as
    bitmaps; bitmaps without rank planes are refused where the statistics need them"""
    S = 5
    planes, ranks, _, _ = systems(N + 3, S, 2, N)
    part = partial_of(ranks, S)
    w = np.random.default_rng(N).dirichlet(np.ones(S)).tolist()
    tabled = norm in TABLED
    distr = tables_for(planes, P_ROW) if tabled else None       # too long for LDS: the two-pass form searches them in global memory
    dd = [dev(d) for d in distr] if tabled else None
    dp = [plane(p) for p in planes]
    rp = [None if r is None else plane(r) for r in part]
    bits = [None if r is None else ops.rank_to_bitmap(r) for r in rp]
    e_part = oracle_nsf(planes, part, w, norm, distr)
    check_nsf(ops.fuse_nsf(dp, None, w, norm, dd, tables=False).cpu().numpy(), oracle_nsf(planes, None, w, norm, distr), norm, "full")
    check_nsf(ops.fuse_nsf(dp, rp, w, norm, dd, tables=False).cpu().numpy(), e_part, norm, "rank planes")
    check_nsf(ops.fuse_nsf(dp, rp, w, norm, dd, valid_bits=bits, tables=False).cpu().numpy(), e_part, norm, "bitmaps + rank planes")
    if norm in ("min-max", "z-score"):
        with pytest.raises(ValueError, match="rank planes"):
            ops.fuse_nsf(dp, None, w, norm, valid_bits=bits)
    else:
        check_nsf(ops.fuse_nsf(dp, None, w, norm, dd, valid_bits=bits, tables=False).cpu().numpy(), e_part, norm, "bitmaps")


def test_many_rows(ops):
    """65,537 query rows of 7 columns: every kernel that puts the query on grid y"""
    Q, N, S = 65537, 7, 2
    planes, ranks, _, lens = systems(5, S, Q, N)
    part = partial_of(ranks, S)
    rp = [None if r is None else plane(r) for r in part]
    dp = [plane(p) for p in planes]
    w = [0.7, 0.3]
    np.testing.assert_array_equal(ops.fuse_rank([plane(r) for r in ranks], dev(lens), "rrf").cpu().numpy(), O.fuse_rank(ranks, lens, "rrf"))
    np.testing.assert_array_equal(ops.fuse_none(dp, rp, w).cpu().numpy(), O.fuse_none(planes, part, w))
    mixed, narrow = mixed_wsum_inputs(planes, S)
    np.testing.assert_array_equal(ops.fuse_wsum([plane(p) for p in mixed], rp, w, narrow=narrow).cpu().numpy(),
                                  O.fuse_wsum(mixed, part, w, narrow))
    bits = ops.rank_to_bitmap(rp[1]).cpu().numpy()
    got = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :N].astype(bool)
    np.testing.assert_array_equal(got, ranks[1] >= 0)
    z = plane(planes[1])
    ops.zero_unlisted_(z, rp[1])
    np.testing.assert_array_equal(z.cpu().numpy(), np.where(ranks[1] >= 0, planes[1], np.float32(0)))
    st = [O.row_stats(p, r, "z-score") for p, r in zip(planes, part)]
    stats = (dev(np.concatenate([a for a, _ in st])), dev(np.concatenate([b for _, b in st])))
    check_nsf(ops.fuse_nsf(dp, rp, w, "z-score", stats=stats).cpu().numpy(), O.fuse_nsf(planes, part, w, "z-score"), "z-score", "stats")
