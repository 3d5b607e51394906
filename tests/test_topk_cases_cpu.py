"""The case tables of the exact top-k tests (topk_cases.py), checked without a GPU: every NumPy reference equals the oracle
(oracle.topk_rows, oracle.topk_merge, oracle.sort_rows_desc) on every case, filter_walk -- topk_filter_kernel's geometry restated -- is a
partition of [0, n) in ascending column order, the designed inputs are what they are meant to be, every case lands the branches it
claims and their union lands all of topk_cases.BRANCHES (the whole-row branches from fz_topk_rows_plan, the function fz_topk_rows_f32
itself runs), fz_topk_rows_plan and fz_topk_fold_max_k judge their arguments, and the refusals that precede every HIP call leave their
outputs untouched."""
import ctypes as C
import os

import numpy as np
import pytest

import topk_cases as T
from fusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUP = _lib.FZ_OK, _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def same(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(T.bits(got), T.bits(ref))


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_branch_table_is_covered():
    hit = set()
    for c in T.ALL_CASES:
        b = c.branches()
        assert b <= set(T.BRANCHES), (c.id, sorted(map(str, b - set(T.BRANCHES))))
        assert set(getattr(c, "claims", ())) <= b, (c.id, sorted(map(str, set(c.claims) - b)))
        hit |= b
    assert set(T.BRANCHES) <= hit, sorted(map(str, set(T.BRANCHES) - hit))
    first, missing = T.landing()
    assert not missing
    for b in sorted(T.BRANCHES, key=str):
        print(b, "<-", first[b])


def test_the_case_axes_of_the_tables():
    assert {c.n for c in T.ROWS_CASES} >= set(T.ROWS_AXIS_N) | {0, 99, 100, 101} and {c.rows for c in T.ROWS_CASES} == {1, 2, 3}
    assert {(35841, 7169), (35841, 7170), (200705, 8000), (114689, 8192)} <= {(c.n, c.k) for c in T.ROWS_CASES}
    assert {k for c in T.ROWS_CASES for k in c.kinds} == {"ties", "const", "neginf", "special", "borders", "lastchunk"}
    assert max(c.rows * c.n for c in T.ROWS_CASES) == 3 * 200705
    assert {(c.n, c.density) for c in T.FILTER_CASES} == {(n, d) for n in T.FILTER_N for d in T.DENSITIES}
    assert T.FILTER_N == (1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 2049, 8191, 8192, 8193, 65535, 65536, 65537, 66561, 131077)
    assert {t for c in T.MIXED_TAU_CASES for t in c.taus} >= {"finite", "-inf", "+inf", "nan"}
    crossing = {(s["round"], s["wave"]) for c in T.CAP_CASES if c.cross >= 0 for s in T.filter_stretches(c.n)
                if s["w0"] <= c.cols()[c.cross] < s["w0"] + s["ncols"]}
    assert crossing == {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0)}, crossing      # 131,077 = two whole rounds + 5 columns
    assert {c.k for c in T.FOLD_CASES} == {1, 7, 100, 1000, 5056} and {(c.G * c.k) for c in T.MERGE_CASES} >= {T.SORT_ROW_F32}
    assert {c.G for c in T.MERGE_CASES} == {1, 2, 8}
    assert {(c.N, c.bits) for c in T.SELECT_CASES} == {(N, b) for N in T.SELECT_N for b in (32, 64)}
    assert {c.id for c in T.SELECT_CASES} >= {f"select-N{N}-f{b}" for N in T.SELECT_N for b in (32, 64)}


def test_the_constants_are_the_library_s():
    L = _lib.lib()
    assert L.fz_topk_max_k() == T.MAX_K and L.fz_sort_max_n() == T.SORT_ROW_F32 and L.fz_sort_max_n_f64() == T.TOPK_CHUNK == T.SELECT_MAX_N
    assert L.fz_topk_fold_max_k(1) == 60 * 1024 // 12 - T.TIE_MARGIN == 5056 and L.fz_topk_fold_max_k(0) == T.SORT_ROW_F32 - 1
    assert L.fz_topk_fold_max_k(7) == 5056                                # any non-zero `unordered`
    assert max(c.k for c in T.FOLD_CASES) == L.fz_topk_fold_max_k(1)     # the largest k the unordered form takes has a case


# ---- whole rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.ROWS_CASES, ids=lambda c: c.id)
def test_rows_reference_equals_the_oracle(oracle, case):
    x = case.inputs()
    assert x.shape == (case.rows, case.n) and x.dtype == np.float32
    rs, ri = T.topk_ref(x, case.k, T.ID_BASE)
    if case.n:
        os_, oi = oracle.topk_rows(x, case.k, T.ID_BASE)
        assert same(rs, T.canon(os_)) and same(ri, oi), case.id
    have = min(case.n, case.k)
    assert (ri[:, have:] == -1).all() and np.isneginf(rs[:, have:]).all() and (ri[:, :have] >= T.ID_BASE).all()
    for r, kind in enumerate(case.kinds):
        if kind == "const":
            assert np.array_equal(ri[r, :have], T.ID_BASE + np.arange(have))
        if kind == "lastchunk" and case.n > T.SORT_ROW_F32:          # the k best are the last k columns (a pair may straddle the cut): the short last chunk first
            assert ri[r, :have].min() - T.ID_BASE in (case.n - have - 1, case.n - have)
        if kind == "borders" and case.n > T.TOPK_CHUNK and case.k >= 12:      # the tie run of the best value straddles the first chunk border
            assert {T.TOPK_CHUNK - 1, T.TOPK_CHUNK} <= set((ri[r, :12] - T.ID_BASE).tolist())
        if kind in ("ties", "special") and case.n >= 100:
            assert len(np.unique(x[r][~np.isnan(x[r])])) <= 7


def test_rows_plan_against_the_hand_computed_shapes():
    lv = lambda n, k: [(l["width"], l["chunks"], l["kk"], l["fill"]) for l in T.rows_plan(n, k)["lv"]]
    assert T.rows_plan(35840, 8192) == dict(levels=0, pad=0, last=35840, lv=[]) and T.rows_plan(0, 5) == dict(levels=0, pad=1, last=0, lv=[])
    assert lv(35841, 7169) == [(35841, 2, 7169, 0)] and lv(35841, 7170) == [(35841, 2, 7170, 1)]
    assert lv(114688, 8192) == [(114688, 4, 8192, 0)] and lv(114689, 8192) == [(114689, 5, 8192, 1), (40960, 2, 8192, 0)]
    assert lv(200705, 8000) == [(200705, 8, 8000, 1), (64000, 3, 8000, 1)] and T.rows_plan(200705, 8000)["last"] == 24000
    assert lv(57345, 1000) == [(57345, 3, 1000, 1)] and lv(57345, 1) == [(57345, 3, 1, 0)] and lv(57344, 1000) == [(57344, 2, 1000, 0)]
    assert T.rows_plan(2**31 - 1, 8192)["levels"] <= T.PLAN_LEVELS and T.rows_plan(2**31 - 1, 8192)["last"] <= T.SORT_ROW_F32
    L = _lib.lib()
    for n, k in [(200705, 8000), (114689, 8192), (35841, 1), (35840, 8192), (2**31 - 1, 8192)]:      # the workspace is the plan's
        p = T.rows_plan(n, k)
        assert L.fz_topk_workspace_bytes(3, n, k) == 3 * sum(l["chunks"] * l["kk"] for l in p["lv"]) * 8 + 256


def test_rows_plan_is_exported_declared_and_judges_its_arguments():
    L = _lib.lib()
    assert {"fz_topk_rows_plan", "fz_topk_fold_max_k"} <= set(_lib.EXPORTS) and hasattr(L, "fz_topk_rows_plan") and hasattr(L, "fz_topk_fold_max_k")
    assert L.fz_abi_version() == _lib.ABI_VERSION == 20          # additive entries: the ABI version stays
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    assert "int fz_topk_rows_plan(" in header and "int fz_topk_fold_max_k(" in header
    assert f"#define FZ_TOPK_ROWS_PLAN_FIELDS {T.PLAN_FIELDS}" in header and f"#define FZ_TOPK_ROWS_PLAN_LEVELS {T.PLAN_LEVELS}" in header
    assert "fz_topk_rows_plan" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for bad, rc_want in [((-1, 5), ARG), ((100, 0), ARG), ((100, -3), ARG), ((100, T.MAX_K + 1), UNSUP)]:
        rc, f = T.rows_plan_status(*bad)
        assert rc == rc_want and f == [-1] * T.PLAN_FIELDS, bad      # refused, nothing written
    assert T.rows_plan_status(100, 5, out=False)[0] == ARG
    rc, f = T.rows_plan_status(100, T.MAX_K)
    assert rc == OK and f[:3] == [0, 1, 100] and not any(f[3:])      # zeros past the last level


# ---- the filter's geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.FILTER_N + (2, 5, 1026, 65536 + 1024, 3 * T.SPAN + 1))
def test_filter_walk_is_a_partition_in_ascending_order(n):
    w = T.filter_walk(n)
    assert np.array_equal(w["col"], np.arange(n)), n                    # every column once, and in the order the compaction numbers them
    assert np.array_equal(w["col"] // T.SPAN, w["round"]) and w["wave"].max() < T.NW and w["step"].max() < 64 and w["lane"].max() < 64
    for vec in (True, False):
        st = T.filter_stretches(n, vec)
        assert sum(s["ncols"] for s in st) == n and len(st) == T.NW * -(-n // T.SPAN)
        for s in st:
            assert s["steps"] <= 64 and s["groups"] * T.UNR <= s["inner"] <= s["steps"] and (vec or s["inner"] == s["groups"] == 0)
            assert not s["groups"] or s["w0"] + s["groups"] * T.UNR * T.STEP <= n               # the unguarded groups stay inside the row
            if s["ragged"] is not None:                                      # at most one ragged step, and it is the row's end
                assert s["w0"] + s["ncols"] == n and s["ragged"] == s["ncols"] // T.STEP and (not vec or s["ragged"] == s["inner"])
        assert sum(s["ragged"] is not None for s in st) <= 1


def test_the_plants_sit_where_the_issue_says():
    for n in T.FILTER_N:
        p = set(T.filter_plants(n).tolist())
        assert {0, n - 1} <= p and all(0 <= j < n for j in p)
        for s in T.filter_stretches(n):
            if s["ncols"]:
                assert {s["w0"], s["w0"] + s["ncols"] - 1} <= p
                assert {s["w0"] + e for e in range(4) if s["w0"] + e < n} <= p
                if s["ncols"] > T.STEP:
                    assert {s["w0"] + T.STEP - 1, s["w0"] + T.STEP, s["w0"] + 252, s["w0"] + 255} <= p
                if s["groups"]:
                    g = s["w0"] + s["groups"] * T.UNR * T.STEP
                    assert g - 1 in p and (g >= n or g in p)
                if s["ragged"] is not None:
                    assert s["w0"] + s["ragged"] * T.STEP in p
        if n > T.SPAN:
            assert {T.SPAN - 1, T.SPAN} <= p


def test_the_mark_densities_give_every_pass2_group_size():
    """At n = 8,192 (8 whole steps per wave) marksM leaves exactly M marked inner steps in every wave; one survivor per step at 65,536
    marks all 64."""
    for m in (1, 2, 3, 4, 5):
        cols = T.filter_marks(8192, m)
        for s in T.filter_stretches(8192):
            mine = cols[(cols >= s["w0"]) & (cols < s["w0"] + s["ncols"])]
            assert len(mine) == len(np.unique((mine - s["w0"]) // T.STEP)) == m and s["inner"] == 8
    cols = T.filter_marks(65536, None)
    for s in T.filter_stretches(65536):
        mine = cols[(cols >= s["w0"]) & (cols < s["w0"] + s["ncols"])]
        assert len(np.unique((mine - s["w0"]) // T.STEP)) == 64 == s["inner"]
    assert {c.density for c in T.FILTER_CASES} >= {"marks1", "marks2", "marks3", "marks4", "marks5", "every-step", "all"}


@pytest.mark.parametrize("case", T.ALL_FILTER_CASES, ids=lambda c: c.id)
def test_filter_inputs(case):
    tau, sc = case.inputs()
    cols = case.cols()
    sel = T.filter_survivors(sc, tau)
    assert sc.shape == (case.rows, case.n) and sc.dtype == np.float32
    for r, kind in enumerate(case.taus):
        j = np.flatnonzero(sel[r])
        if kind in ("zero", "finite", "neg", "-inf"):
            assert np.array_equal(j, cols), (case.id, r)                 # the planted columns and nothing else
            back = np.delete(sc[r], cols)
            assert (back <= tau[r]).all() and (back == tau[r]).any() or back.size == 0      # the background ties with tau and loses
            if kind == "zero":
                assert np.signbit(back).all() and not np.signbit(tau[r])                   # -0.0 against +0.0
            fin = sc[r, cols][~np.isnan(sc[r, cols])]
            assert (fin == np.nextafter(tau[r], np.float32(np.inf))).all()
            assert np.isnan(sc[r, cols[::2]]).all() and (T.bits(sc[r, cols[::2]]) == 0x7FC00123).all()
        elif kind == "+inf":
            assert np.array_equal(j, cols[::2]) and np.isnan(sc[r, j]).all()
        else:
            assert len(j) == case.n
    exp, lens, flag = T.filter_expected(sc, tau, case.prior, case.cap(), T.ID_BASE)
    if case.cross >= 0:
        assert flag == 1 and lens[0] == case.cap() and len(exp[0][0]) == case.cross
    elif case.slack >= 0:
        assert flag == 0 and lens.max() == case.cap() - case.slack
    else:
        assert flag == 1
    for name in T.LAYOUTS:                                               # the four layouts: what decides the kernel's vector path
        buf, off, ld = T.framed(sc[:, : min(case.n, 300)], name)
        assert ((ld % 4 == 0) and (off % 4 == 0)) == T.LAYOUT_VEC[name] and np.isposinf(buf[:off]).all() and np.isposinf(buf[-T.GHOST:]).all()
        assert T.bits(buf[off + ld: off + ld + min(case.n, 300)]).tolist() == T.bits(sc[1, :300]).tolist()


def test_the_update_cases_are_the_ones_the_tests_run():
    assert {(c.n, c.density) for c in T.UPDATE_CASES} == {(n, d) for n in T.UPDATE_N for d in T.UPDATE_DENSITIES}
    assert all(T.UPDATE_BRANCH in c.branches() for c in T.UPDATE_CASES) and not any(T.UPDATE_BRANCH in c.branches() for c in T.ALL_FILTER_CASES)


@pytest.mark.parametrize("n", T.UPDATE_N)
@pytest.mark.parametrize("density", T.UPDATE_DENSITIES)
def test_update_inputs(oracle, n, density):
    """The update form's reference is oracle.topk_rows of [list scores | chunk] with the list's ids mapped back: the list is full, its
    ids lie below the chunk's, and every survivor shows in the new list."""
    case, k, run_s, run_i, tau, sc = T.update_inputs(n, density)
    assert k + case.cap() <= T.SORT_ROW_F32 and (run_s[:, -1] == tau).all() and (run_i >= 0).all() and run_i.max() < T.ID_BASE
    ns, ni = T.update_ref(run_s, run_i, sc, T.ID_BASE)
    os_, oc = oracle.topk_rows(np.concatenate([run_s, sc], axis=1), k, 0)
    ids = np.where(oc < k, np.take_along_axis(run_i, np.minimum(oc, k - 1), axis=1), T.ID_BASE + oc - k)
    assert same(ns, T.canon(os_)) and same(ni, ids)
    sel = T.filter_survivors(sc, tau)
    for r in range(case.rows):
        assert set((T.ID_BASE + np.flatnonzero(sel[r])).tolist()) <= set(ni[r].tolist())


# ---- fold --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.FOLD_CASES, ids=lambda c: c.id)
def test_fold_reference_equals_the_oracle(oracle, case):
    run_s, run_i, cand_s, cand_i, cand_len, perms = case.inputs()
    ns, ni, tau, flag, met = case.expected()
    k, cap = case.k, case.cap
    assert set(case.claims) <= {("fold", "tie", t) for t in met}, (case.id, met)
    for r in range(case.rows):
        n = min(int(cand_len[r]), cap)
        real = int((run_i[r] >= 0).sum())
        assert (np.diff(cand_i[r, :n]) > 0).all() and (cand_i[r, :n] >= T.ID_BASE).all() and run_i[r].max() < T.ID_BASE      # ascending ids, behind the list's
        assert np.array_equal(T.order_desc(run_s[r, :real], run_i[r, :real]), np.arange(real))                               # the list is a ranked list
        assert (cand_s[r, n:] == T.S_GUARD).all() and sorted(perms[r].tolist()) == list(range(len(perms[r])))
        # oracle.sort_rows_desc: the stable sort of [list | candidates]
        row = np.concatenate([run_s[r], cand_s[r, :n]])[None, :]
        order, keys = oracle.sort_rows_desc(row)
        ids = np.concatenate([run_i[r], cand_i[r, :n]])[order[0, :k]]
        assert same(ns[r], T.canon(keys[0, :k])) and same(ni[r], ids), (case.id, r)
        # ... and the (score, id) order of the whole, padding last: what a search that never streamed would list
        o = T.order_desc(row[0], np.concatenate([run_i[r], cand_i[r, :n]]), pad=np.concatenate([run_i[r], cand_i[r, :n]]) < 0)[:k]
        assert np.array_equal(ni[r], np.concatenate([run_i[r], cand_i[r, :n]])[o]), (case.id, r)
    assert same(tau, ns[:, -1])
    if case.name == "plain":
        assert flag == 0                                                 # short runs only: both forms must give these lists


def test_the_tie_rule_on_hand_made_lists():
    key = lambda *runs: np.concatenate([np.full(n, v, dtype=np.uint32) for v, n in runs])
    k = 100
    distinct = lambda n, base=1000: np.arange(base, base + n, dtype=np.uint32)
    assert T.tie_rule(distinct(300), k) == (0, set())
    assert T.tie_rule(np.concatenate([distinct(99), key((5000, 64)), distinct(137, 6000)]), k) == (0, {"closes-at-k+63:clear"})      # slots 99 .. 162
    assert T.tie_rule(np.concatenate([distinct(99), key((5000, 65)), distinct(136, 6000)]), k) == (1, {"open-at-k+64:flag"})        # slots 99 .. 163
    assert T.tie_rule(np.concatenate([distinct(99), key((5000, 65))]), k) == (0, {"touches-the-end:clear"})                         # have == k + 64
    assert T.tie_rule(np.concatenate([distinct(100), key((5000, 200))]), k) == (0, {"behind-the-cut:clear"})
    assert T.tie_rule(np.concatenate([distinct(10), key((5000, 512)), distinct(600, 6000)]), 1000)[0] == 0
    assert T.tie_rule(np.concatenate([distinct(10), key((5000, 513)), distinct(600, 6000)]), 1000) == (1, {"513:flag"})
    assert T.tie_rule(np.concatenate([distinct(15), key((T.KEY_NEG_INF, 90))]), k) == (0, {"short-list:padding"})


# ---- merge -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.MERGE_CASES, ids=lambda c: c.id)
def test_merge_reference_equals_the_oracle(oracle, case):
    s, i = case.inputs()
    assert s.shape == i.shape == (case.G, case.rows, case.k)
    for g in range(case.G):
        for r in range(case.rows):
            real = int((i[g, r] >= 0).sum())
            assert (i[g, r, real:] == -1).all() and np.isneginf(s[g, r, real:]).all() and (g not in case.empty or real == 0)
            assert np.array_equal(T.order_desc(s[g, r, :real], i[g, r, :real]), np.arange(real))
            assert g == 0 or real == 0 or i[g, r, :real].min() > i[:g, r].max()          # shard g's ids lie above the earlier shards'
    ms, mi = T.merge_ref(s, i)
    os_, oi = oracle.topk_merge(s, i)
    assert same(ms, T.canon(os_)) and same(mi, oi), case.id
    assert all(G * k > T.SORT_ROW_F32 for G, k in T.MERGE_REFUSED) and (1, T.SORT_ROW_F32 + 1) in T.MERGE_REFUSED


# ---- select ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SELECT_CASES, ids=lambda c: c.id)
def test_select_reference_equals_the_oracle(oracle, case):
    x, pos = case.inputs()
    k, cap = T.SELECT_K, case.cap
    assert x.dtype == case.dtype and x.shape == (case.rows, case.N)
    p = np.tile(np.arange(case.N, dtype=np.int32), (case.rows, 1)) if pos is None else pos
    U = (p >= 0).sum(axis=1).astype(np.int32)
    ins = np.full((case.rows, case.N), -1, dtype=np.int32)
    for r in range(case.rows):
        idx = np.flatnonzero(p[r] >= 0)
        assert sorted(p[r, idx].tolist()) == list(range(len(idx)))      # positions dense per row, as the insertion order is
        ins[r, p[r, idx]] = idx
    e_order, e_keys = oracle.sort_rows_desc(x, init_order=ins, row_len=U)
    cols, sc, lens = T.select_ref(x, pos, k)
    kk = min(k, case.N)
    assert np.array_equal(lens, np.minimum(U, k))
    for r in range(case.rows):
        n = int(lens[r])
        assert np.array_equal(cols[r, :n], e_order[r, :n]) and same(sc[r, :n], T.canon(e_keys[r, :n])) and (cols[r, n:] == -1).all(), (case.id, r)
    sims = case.sims()
    for r, kind in enumerate(case.kinds):
        count, met = sims[r]
        if kind == "ties-at-cap" and case.N > cap:
            assert count == (cap + 1 if case.over else cap) and ("tie-overflow" in met) == case.over, (case.id, count, met)
        if kind == "stops-at-cap":
            assert count == cap and "bisect-early-at-cap" in met and U[r] == case.N
            assert T.select_sim(T.desc_key(x[r].astype(np.float32)), k, cap - 1)[0] < cap      # a lower threshold would do too
        if kind == "few-listed":
            assert U[r] == min(k - 3, case.N) and count == U[r]
        if kind == "none-listed":
            assert U[r] == 0 and count == 0
        if kind == "random" and case.bits == 64 and case.N > 1000:
            assert len(np.unique(x[r])) > len(np.unique(x[r].astype(np.float32)))      # float64 scores that round to equal float32 keys
    assert any("tie-overflow" in m for _, m in sims) == case.over
    assert kk <= k


def test_select_cases_sit_on_the_limit_of_the_cap_ops_hands_the_kernel():
    """ops.select_topk rounds a given cap up to a whole plane row (eff_cap).  Both key widths, at an N above 1,024, have a tie run that
    fills eff_cap exactly (a result) and one that is one entry longer (None); the cap-50 cases, whose 51 candidates overflow the raw entry
    and fit the 64 slots ops hands over, stay: they are what exposed the lost slots between cap and the plane's row stride."""
    at, past, between = set(), set(), set()
    for c in T.SELECT_CASES:
        assert c.eff_cap % T.OPS_PLANE_PAD == 0 and 0 <= c.eff_cap - c.cap < T.OPS_PLANE_PAD
        top = max(n for n, _ in c.sims(c.eff_cap))
        if "ties-at-cap" in c.kinds and c.N > 1024:
            (past if top > c.eff_cap else at if top == c.eff_cap else between if top > c.cap else set()).add((c.bits, c.cap))
    assert at >= {(32, 64), (64, 64)} and past >= {(32, 64), (64, 64)} and between >= {(32, 50), (64, 50)}, (at, past, between)


# ---- refusals that precede every HIP call ------------------------------------------------------------------------------------------------
def test_refusals_leave_their_outputs_untouched():
    """Without a GPU only the argument paths can run: statuses that every entry returns before its first HIP call, handed host buffers
    that must come back byte for byte (the GPU file runs the documented refusals of all six entries on device buffers)."""
    L = _lib.lib()
    f = np.full(64, T.S_GUARD, dtype=np.float32)
    i = np.full(64, T.I_GUARD, dtype=np.int64)
    l = np.full(8, T.I_GUARD, dtype=np.int32)
    ws = np.zeros(1 << 16, dtype=np.uint8)
    P = lambda a: C.c_void_p(a.ctypes.data)
    before = [a.copy() for a in (f, i, l)]
    calls = [
        (L.fz_topk_rows_f32(P(f), 1, 8, 8, T.MAX_K + 1, 0, P(f), P(i), P(ws), ws.size, None), UNSUP),
        (L.fz_topk_rows_f32(P(f), 1, 8, 4, 4, 0, P(f), P(i), P(ws), ws.size, None), ARG),
        (L.fz_topk_rows_f32(P(f), 1, 8, 8, 0, 0, P(f), P(i), P(ws), ws.size, None), ARG),
        (L.fz_topk_rows_f32(P(f), 1, 40000, 40000, 8, 0, P(f), P(i), P(ws), L.fz_topk_workspace_bytes(1, 40000, 8) - 1, None), _lib.FZ_ERR_WORKSPACE),
        (L.fz_topk_update_f32(P(f), 1, 8, 8, 0, P(f), P(i), 35000, 841, P(f), P(i), P(l), P(ws), ws.size, None), UNSUP),
        (L.fz_topk_update_f32(P(f), 1, 8, 8, 0, P(f), P(i), 4, 0, P(f), P(i), P(l), P(ws), ws.size, None), ARG),
        (L.fz_topk_update_f32(P(f), 1, 8, 8, 0, P(f), P(i), 4, 4, P(f), P(i), P(l), P(ws), L.fz_topk_update_workspace_bytes(1, 4, 4) - 1, None), _lib.FZ_ERR_WORKSPACE),
        (L.fz_topk_filter_append_f32(P(f), 1, 8, 8, 0, P(f), P(f), P(i), P(l), 0, P(l), None), ARG),
        (L.fz_topk_filter_append_f32(P(f), 1, 8, 4, 0, P(f), P(f), P(i), P(l), 4, P(l), None), ARG),
        (L.fz_topk_filter_append_f32(P(f), 1, 8, 8, 0, None, P(f), P(i), P(l), 4, P(l), None), ARG),
        (L.fz_topk_fold_f32(P(f), P(i), 1, 35000, P(f), P(i), P(l), 841, 0, P(f), P(i), P(f), P(l), P(ws), ws.size, None), UNSUP),
        (L.fz_topk_fold_f32(P(f), P(i), 1, 5057, P(f), P(i), P(l), 4, 1, P(f), P(i), P(f), P(l), P(ws), 1 << 30, None), UNSUP),      # before any launch now
        (L.fz_topk_fold_f32(P(f), P(i), 1, 4, P(f), P(i), P(l), 4, 1, P(f), P(i), P(f), None, P(ws), ws.size, None), ARG),
        (L.fz_topk_fold_f32(P(f), P(i), 1, 4, P(f), P(i), P(l), 4, 0, P(f), P(i), P(f), P(l), P(ws), L.fz_topk_fold_workspace_bytes(1, 4, 4) - 1, None), _lib.FZ_ERR_WORKSPACE),
        (L.fz_topk_merge(P(f), P(i), 1, 1, T.SORT_ROW_F32 + 1, P(f), P(i), None), UNSUP),
        (L.fz_topk_merge(P(f), P(i), 0, 1, 4, P(f), P(i), None), ARG),
        (L.fz_select_topk_f(P(f), 16, None, 1, 8, 8, 2, 4, P(l), P(f), P(f), P(l), P(l), None), ARG),
        (L.fz_select_topk_f(P(f), 32, None, 1, 8, 8, 4, 2, P(l), P(f), P(f), P(l), P(l), None), ARG),
        (L.fz_select_topk_f(P(f), 32, None, 1, T.SELECT_MAX_N + 1, T.SELECT_MAX_N + 1, 2, 4, P(l), P(f), P(f), P(l), P(l), None), UNSUP),
    ]
    for n, (got, want) in enumerate(calls):
        assert got == want, (n, got, want)
    for a, b in zip((f, i, l), before):
        assert np.array_equal(a, b)
    assert L.fz_topk_fold_f32(P(f), P(i), 0, 5056, P(f), P(i), P(l), 4, 1, P(f), P(i), P(f), P(l), P(ws), ws.size, None) == OK      # rows == 0, at the limit


def test_topk_stream_refuses_an_unordered_source_beyond_the_fold_s_k():
    """ops.TopkStream._feed raises before its source's first filter launch (here: before the source is touched at all)."""
    from fusion_amd import ops

    class Stream(ops.TopkStream):
        def __init__(self, k):
            self.k, self.unordered = k, False      # (nothing else: _feed must raise before it touches the stream or the source)

    launched = []
    src = ops._Source(10, lambda *a: launched.append(a), None, unordered=True)
    with pytest.raises(ValueError, match="5056"):
        Stream(5057)._feed(src, 0, 10)
    assert not launched and ops.fold_max_k(True) == 5056 and ops.TopkStream64._fold_limits_k is False and ops.TopkStream._fold_limits_k is True
