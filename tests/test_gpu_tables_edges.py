"""csrc/tables.hip at every probe, plan and walk edge (tables_cases.py: restatements, designed tables and the case table;
test_tables_cases_cpu.py holds the restatements to the oracle's brute-force scan and proves which edge each case hits).  For every case:
the kernel that took the call, `PreparedTables.search_info()` against the restated bucket table (which bt_lookup instantiation ran),
percentile-rank against `expected` BIT FOR BIT, NCE bit for bit against `expected` over the kernel's own value table (read back from the
workspace at the restated plan's offsets: a nearest entry one off shows, which the suite's 1e-4 on the fused score cannot see at these
table lengths), that value table within 1e-4 of the float64 formula, the same bits from fz_fuse_nsf_f32 (`tables=False`), from validity
bitmaps and from a second call, the frame around the output and the input planes untouched."""
import numpy as np
import pytest
import torch

import tables_cases as T

pytestmark = pytest.mark.gpu

GUARD = np.float32(-54321.0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plane_of(ops, a, pad):
    """A plane whose padding columns [N, ld) hold `pad`: what a kernel reads there must not reach an output."""
    p = ops.alloc_plane(a.shape[0], a.shape[1], torch.from_numpy(a[:0]).dtype, "cuda", fill=pad)
    p.copy_(torch.from_numpy(a))
    return p


def framed_out(Q, N):
    """[Q, N] output inside a guard frame: a row in front, a row behind, and the padding columns."""
    ld = max((N + 63) // 64 * 64, 64)
    base = torch.full((Q + 2, ld), float(GUARD), dtype=torch.float32, device="cuda")
    return base, base[1: Q + 1, :N]


def frame_intact(base, Q, N):
    b = base.cpu().numpy()
    return bool(np.all(b[0] == GUARD) and np.all(b[Q + 1] == GUARD) and np.all(b[1: Q + 1, (N + 3) // 4 * 4:] == GUARD))   # (a row's last float4 is written whole)


def first_difference(got, exp, c):
    """None, or where the planes differ -- with the workgroup and the walk step of the first differing (row, chunk) item."""
    bad = np.argwhere(T.bits(got) != T.bits(exp))
    if not len(bad):
        return None
    q, j = map(int, bad[0])
    wk = T.walk(c.Q, c.N)
    item = q * wk["chunks"] + j // T.BT_COLS
    return (f"{len(bad)} of {got.size} scores differ in {len(np.unique(bad[:, 0]))} rows; first at row {q}, column {j}: got {got[q, j]!r}, expected {exp[q, j]!r}, "
            f"scores {[float(p[q, j]) for p in c.planes]} (item {item}: workgroup {item % wk['grid']}, walk step {item // wk['grid']})")


def read_values(prep, pl, s, P):
    off = T.value_offset(pl, s)
    return prep.workspace[off: off + 4 * P].cpu().numpy().view(np.float32).copy()


@pytest.mark.parametrize("key", list(T.CASES))
def test_case(ops, key):
    c = T.case(key)
    P_d = [dev(t) for t in c.tabs]
    planes = [plane_of(ops, x, float("nan")) for x in c.planes]
    rk = None if c.ranks is None else [None if r is None else plane_of(ops, r, 0) for r in c.ranks]       # padding "listed": it must be masked by the row end
    vb = None if rk is None else [None if r is None else ops.rank_to_bitmap(r) for r in rk]
    problems = []
    for norm in T.norms_of(key):
        pl = c.plan(norm)
        prep = ops.nsf_tables_prepare(P_d, norm)
        V = None
        if c.path == "row":
            assert pl is None and prep is None, (key, norm)
        else:
            assert prep is not None and int(prep.workspace.numel()) == pl["sys_off"][-1], (key, norm)
            info, srs = prep.search_info(), c.searches(norm)
            want = [dict(probes=sr["probes"], fullest_bucket=sr["fullest_bucket"]) for sr in srs]
            if info != want:
                problems.append(f"{norm}: search_info {info}, restated {want}")
            if norm == T.NORMS[1]:
                V = [read_values(prep, pl, s, P) for s, P in enumerate(c.P)]
                for s, P in enumerate(c.P):      # the value table against the float64 formula: the suite's bound for this normalisation
                    ref = T.nce_values(P)
                    err = float(np.max(np.abs(V[s][1:].astype(np.float64) - ref[1:]), initial=0.0))
                    print(f"{key} {norm} system {s}: P = {P}, value table max |V - float64 formula| = {err:.3g}")
                    assert V[s][0] == -np.inf and ref[0] == -np.inf and np.all(np.isfinite(V[s][1:])), (key, s)
                    assert err <= T.NCE_TOL, (key, s, err)
        base, out = framed_out(c.Q, c.N)
        ops.last_tables_path = None
        got_t = ops.fuse_nsf(planes, rk, c.w, norm, P_d, out=out, tables=prep)
        assert ops.last_tables_path == c.path, (key, norm, ops.last_tables_path)
        got = got_t.cpu().numpy()
        if V is None and norm == T.NORMS[1]:     # the global-memory search has no value table to read back: its fused scores within the suite's bound
            exp = c.expected(norm, V=[T.nce_values_f32(P) for P in c.P])
            fin = np.isfinite(exp)
            assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], exp[~fin]) and np.max(np.abs(got[fin] - exp[fin]), initial=0.0) <= T.NCE_TOL
        else:
            diff = first_difference(got, c.expected(norm, V=V), c)
            if diff:
                problems.append(f"{norm}: {diff}")
        if not frame_intact(base, c.Q, c.N):
            problems.append(f"{norm}: the frame around the output was written")
        old = ops.fuse_nsf(planes, rk, c.w, norm, P_d, tables=False).cpu().numpy()       # fz_fuse_nsf_f32: the per-score search
        assert ops.last_tables_path in ("row", "lds-all")
        if not np.array_equal(T.bits(old), T.bits(got)):
            problems.append(f"{norm}: tables=False differs: {first_difference(got, old, c)}")
        if vb is not None:
            bits_ = ops.fuse_nsf(planes, None, c.w, norm, P_d, valid_bits=vb, tables=prep).cpu().numpy()
            if not np.array_equal(T.bits(bits_), T.bits(got)):
                problems.append(f"{norm}: validity bitmaps differ from rank planes: {first_difference(bits_, got, c)}")
        again = ops.fuse_nsf(planes, rk, c.w, norm, P_d).cpu().numpy()                    # tables prepared inside the call
        if not np.array_equal(T.bits(again), T.bits(got)):
            problems.append(f"{norm}: a second call differs: {first_difference(again, got, c)}")
    for x, p in zip(c.planes, planes):
        assert np.array_equal(T.bits(p.cpu().numpy()), T.bits(x)), key
    if rk is not None:
        for r, p in zip(c.ranks, rk):
            assert r is None or np.array_equal(p.cpu().numpy(), r), key
    assert not problems, f"{key} ({T.CASES[key][0]}):\n  " + "\n  ".join(problems)


def test_which_instantiations_the_older_table_cases_reach(ops):
    """search_info() on the tables of test_gpu_tables.py's CASES, as measured (DESIGN.md quotes this): the older suite runs the unrolled
    search at two, three and four probes and the loop (5 - 14 probes), never at one -- which group A now does, next to each class's
    boundary sizes at both parities."""
    import test_gpu_tables as old
    seen = {}
    for S, Q, N, P, kind, partial in old.CASES:
        rng = np.random.default_rng(S * 1000003 + N * 31 + P)
        tabs = old._tables(rng, S, P, kind)
        for norm in T.NORMS:
            info = ops.nsf_tables_prepare([dev(t) for t in tabs], norm).search_info()
            lutb = T.plan([P] * S, norm == T.NORMS[1])["lutb"]
            assert info == [dict(probes=sr["probes"], fullest_bucket=sr["fullest_bucket"]) for sr in (T.search(t, lutb) for t in tabs)]
            seen.setdefault((kind, P), set()).update(T.search(t, lutb)["inst"] for t in tabs)
    print({k: sorted(map(str, v)) for k, v in seen.items()})
    reached = set().union(*seen.values())
    assert reached == {2, 3, 4, "loop"}
    new = {T.search(t, 16384)["inst"] for k in T.group("A") for t in T.case(k).tabs}
    assert new == {1, 2, 3, 4, "loop"}
