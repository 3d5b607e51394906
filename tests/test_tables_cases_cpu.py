"""The case table of the long-table fusion edge tests (tables_cases.py), checked without a GPU: the restated plan equals bt_plan (the
library's host functions) and its thresholds are derived, not quoted; `nearest_first` / `expected` equal the oracle's brute-force scan
(fusion_oracle.c: the first minimum of the float32 distances) bit for bit on every case -- whole planes in groups A, B, C, D, G and H, a
column sample per row in the long rows of E and F; and every case hits what its line says, computed by the restatements: fullest bucket and parity,
the bt_lookup instantiation (all five reached), plateau lengths, the plan on each side of each threshold, a carry of advance().  No case
is skipped or filtered: each test walks its whole group."""
import ctypes as C

import numpy as np
import pytest

import tables_cases as T
from fusion_amd import _lib

# every edge, written out: a case cannot go missing from tables_cases.CASES without this list saying so
EDGES = (
    [f"A-m{m}" for m in (1, 2, 3, 6, 7, 14, 15, 30, 31, 33, 64)] + ["A-m2+m3", "A-m6+m7", "A-m14+m15", "A-m30+m31", "A-m33+m1", "A-m64+m15"] +
    ["B-runs-1to9", "B-runs-33", "B-round-1to5", "B-round-6to33"] +
    [f"C-P{P}" for P in (16084, 16085, 32212, 32213, 36308, 36309, 38356, 38357, 39380, 39381)] +
    ["D-P1+2+10001+39380", "D-P1+2+10001+39380-partial", "D-P3+27943+16085+257", "D-P3+27943+16085+257-partial"] +
    [f"E-N{N}" for N in (1, 2, 3, 4, 5, 7, 31, 33, 28671, 28672, 28673, 28675, 57344, 57345)] +
    [f"F-Q{Q}-N{N}-S{S}-P{P}" for Q, N in ((255, 64), (256, 64), (257, 64), (513, 64), (129, 28673), (86, 57345), (171, 57345)) for S in (1, 2)
     for P in (10001, 20000)] +
    [f"G-P{P}" for P in (10001, 27943, 32749, 39380)] + ["H-denormal", "H-const+ordinary"])


def test_the_case_table_is_the_list_of_edges():
    assert list(T.CASES) == EDGES and len(set(EDGES)) == len(EDGES) == 83
    assert all(isinstance(line, str) and line and callable(build) for line, build in T.CASES.values())
    assert sorted({k[0] for k in T.CASES}) == list(T.GROUPS)
    for k in T.CASES:
        assert T.norms_of(k) == (T.NORMS if k[0] != "F" else (T.NORMS[k.endswith("-P20000")],)), k


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def lib_plan(P, nce):
    L = _lib.lib()
    L.fz_nsf_tables_workspace_bytes.restype = C.c_size_t
    L.fz_nsf_tables_header_offset.restype = C.c_size_t
    S = len(P)
    arr = (C.c_int32 * S)(*P)
    norm = 5 if nce else 4
    nb = int(L.fz_nsf_tables_workspace_bytes(S, arr, norm))
    return nb, [int(L.fz_nsf_tables_header_offset(S, arr, norm, s)) for s in range(S)]


def test_the_restated_plan_is_bt_plan_and_its_thresholds_are_derived():
    one = lambda nce: (lambda P: T.plan([P], nce))
    assert T.plan_threshold(lambda P: T.plan([P], True)["val_in_lds"], hi=30000) == 16084
    for lutb, last in ((16384, 32212), (8192, 36308), (4096, 38356), (2048, 39380)):
        assert T.plan_threshold(lambda P: (one(False)(P) or {"lutb": 0})["lutb"] >= lutb) == last
        for nce in (False, True):
            assert one(nce)(last)["lutb"] == lutb and (one(nce)(last + 1) or {"lutb": 0})["lutb"] == lutb // 2 * (lutb > 2048)
    assert T.plan([39381], False) is None and T.plan([39381], True) is None and T.plan([10001, 39381], False) is None
    assert T.plan([0], False) is None and T.plan([65536], False) is None
    assert {P: (T.plan([P], False) or {"lutb": None})["lutb"] for P in T.PLAN_EDGES} == T.PLAN_LUTB
    assert [T.plan([P], True)["val_in_lds"] for P in (16084, 16085)] == [True, False] and not T.plan([16084], False)["val_in_lds"]
    # P = 39,380: lead + table + tail is a whole number of DMA pieces, so the +inf tail is exactly BT_TAIL entries
    pl = T.plan([39380], False)
    assert pl["Ppad"] == [T.BT_LEAD + 39380 + T.BT_TAIL] and pl["Ppad"][0] % T.BT_PIECE == 0 and pl["lds_bytes"] + 4 * T.BT_PIECE > T.BT_LDS_BUDGET      # one more piece would not fit
    # the library's own bt_plan: workspace size and every system's offset, on every P list the cases use and around each threshold
    lists = [c.P for c in (T.case(k) for k in T.CASES if k[0] in "ABCDGH")] + [[P] for e in T.PLAN_EDGES for P in (e - 1, e, e + 1)] + [[10001] * 8, [1], [1, 39380, 2]]
    for P in lists:
        for nce in (False, True):
            pl = T.plan(P, nce)
            nb, offs = lib_plan(P, nce)
            if pl is None:
                assert nb == 0 and all(o == 2 ** 64 - 1 for o in offs), P
            else:
                assert nb == pl["sys_off"][-1] and offs == pl["sys_off"][:-1], (P, nce)
                assert pl["lds_bytes"] <= T.BT_LDS_BUDGET and all(o % 16 == 0 for o in pl["sys_off"])


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def test_nearest_first_is_the_first_argmin_of_the_float32_distances():
    rng = np.random.default_rng(3)
    for tab in (np.array([0.5]), np.array([0.1, 0.9]), np.array([1.0, 1.0, 1.0]), np.sort(rng.integers(0, 12, 60)) * 0.25, T.rounding_table(300, 7),
                np.sort(np.float32(1.0) + rng.integers(0, 8, 100).astype(np.float32) * np.float32(2.0 ** -23)), T.case("H-denormal").tabs[0][:400]):
        tab = tab.astype(np.float32)
        x = np.concatenate([tab, T.up(tab), T.down(tab), ((tab[:-1].astype(np.float64) + tab[1:]) / 2).astype(np.float32), np.array(T.ROUND_X, dtype=np.float32),
                            rng.uniform(float(tab[0]) - 1, float(tab[-1]) + 1, 200).astype(np.float32), [np.nan, np.inf, -np.inf, -0.0, 0.0]]).astype(np.float32)
        k, run = T.nearest_first(tab, x, lengths=True)
        assert np.array_equal(k, T.nearest_scan(tab, x))
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.abs(tab[:, None] - x[None, :])
            cnt = ((d == d.min(axis=0)) & (tab[:, None] <= x[None, :])).sum(axis=0)
        fin = np.isfinite(x)
        assert np.array_equal(run[fin], cnt[fin]) and not run[~fin].any()


def sample_columns(N, n, key):
    """The columns the brute-force oracle sees: both row ends, both sides of every chunk border, and random ones."""
    if n is None or n >= N:
        return np.arange(N)
    fixed = {0, 1, 2, 3, N - 1, N - 2, N - 3, N - 4, N - 5} | {b + d for b in range(T.BT_COLS, N + 1, T.BT_COLS) for d in (-2, -1, 0, 1)}
    fixed = {j for j in fixed if 0 <= j < N}
    return np.array(sorted(fixed | set(T.rng_of("sample", key).choice(N, n, replace=False).tolist())))


@pytest.mark.parametrize("g", T.GROUPS)
def test_the_restatement_equals_the_oracles_scan_on_every_case(oracle, g):
    """percentile-rank bit for bit: the oracle scans all P entries per score (fusion_oracle.c, `dd < bd`).  NCE goes through the same
    indices; its values are the oracle's own erfinv, so it is held to the suite's 1e-4 and its infinities exactly."""
    keys = T.group(g)
    assert keys
    for key in keys:
        c = T.case(key)
        cols = sample_columns(c.N, c.sample, key)
        assert (c.sample is None) == (g in "ABCDGH" or c.N < 1000), key              # whole planes wherever the scan is affordable
        planes = [np.ascontiguousarray(p[:, cols]) for p in c.planes]
        ranks = None if c.ranks is None else [None if r is None else np.ascontiguousarray(r[:, cols]) for r in c.ranks]
        exp = c.expected(T.NORMS[0])[:, cols]               # (group F: the restatement on the base rows, rotated -- held to the oracle here)
        ref = oracle.fuse_nsf(planes, ranks, c.w, T.NORMS[0], c.tabs)
        bad = np.argwhere(T.bits(exp) != T.bits(ref))
        assert not len(bad), (key, len(bad), bad[:3].tolist(), exp[tuple(bad[0])], ref[tuple(bad[0])])
        if ranks is not None:
            assert np.isneginf(exp).any() == any((np.stack([r for r in ranks if r is not None]) < 0).all(axis=0).ravel()) or len([r for r in ranks if r is None])
        if g in "BDH":
            V = [T.nce_values_f32(P) for P in c.P]
            e2, r2 = c.expected(T.NORMS[1], V=V)[:, cols], oracle.fuse_nsf(planes, ranks, c.w, T.NORMS[1], c.tabs)
            fin = np.isfinite(r2)
            assert np.array_equal(np.isfinite(e2), fin) and np.array_equal(e2[~fin], r2[~fin]) and np.max(np.abs(e2[fin] - r2[fin]), initial=0.0) <= T.NCE_TOL, key


def test_nce_values_follow_the_float64_formula():
    from statistics import NormalDist
    for P in (3, 257, 10001):
        v64, v32, y = T.nce_values(P), T.nce_values_f32(P), T._nce_arg(P)
        assert v64[0] == -np.inf and v32[0] == -np.inf and np.max(np.abs(v64[1:] - v32[1:])) <= 1e-5 and y.dtype == np.float32
        for k in (1, 2, P // 2, P - 1):
            assert abs(v64[k] - (NormalDist().inv_cdf((float(y[k]) + 1.0) / 2.0) * 21.06 + 50.0)) <= 1e-9
        assert np.all(np.diff(v64[1:]) >= 0)


# ---- what each case hits -------------------------------------------------------------------------------------------------------------------
def test_group_a_lands_every_probe_class_at_both_parities_in_bucket_zero_and_in_the_top_bucket():
    inst, parities_P, fewer = set(), set(), set()
    for key in T.group("A"):
        c = T.case(key)
        ms = [int(x) for x in key[2:].replace("m", "").split("+")]
        assert c.S == len(ms) and all(P >= 10001 for P in c.P) and c.plan(T.NORMS[0])["lutb"] == c.plan(T.NORMS[1])["lutb"] == 16384
        for s, m in enumerate(ms):
            tab, des, sr = c.tabs[s], c.des[s], T.search(c.tabs[s], 16384)
            assert sr["inv_w"] == 1.0 and np.array_equal(sr["bk"], np.minimum(np.floor(tab), 16383))      # bucket(x) = floor(x)
            assert sr["fullest_bucket"] == m and sr["probes"] == T.A_PROBES[m] and sr["inst"] == T.A_INST[m]
            full = {b: (first, n) for b, first, n in T.fullest(tab, 16384)}
            if m > 1:
                assert set(full) == set(des.values())                                                      # the background stays below m
            else:
                assert set(des.values()) <= set(full)
            assert full[des["zero"]][0] == 0 and des["zero"] == 0 and des["top"] == 16383 and full[des["top"]][0] == c.P[s] - m
            assert full[des["even"]][0] % 2 == 0 and full[des["odd"]][0] % 2 == 1 and full[des["tight"]][0] % 2 == 1
            for b in des.values():                                                                          # m DISTINCT entries between empty buckets
                e = tab[sr["lut"][b]: sr["lut"][b + 1]]
                assert len(np.unique(e)) == m
                assert b == 0 or sr["lut"][b] == sr["lut"][b - 1]
                if b == des["tight"]:          # its upper neighbour: one entry, at the bucket's floor
                    assert sr["lut"][b + 3] == sr["lut"][b + 2] == sr["lut"][b + 1] + 1 and tab[sr["lut"][b + 1]] == b + 1
                else:
                    assert b == 16383 or sr["lut"][b + 2] == sr["lut"][b + 1]
            # the worst case of the class: a bucket whose first entry sits at an odd index fills ceil(m / 2) pairs' second entries
            f = full[des["odd"]][0]
            assert len([k for k in range(f, f + m) if k % 2 == 1]) == (m + 1) // 2 <= 2 ** sr["probes"] - 1
            assert m == 1 or (m + 1) // 2 > 2 ** (sr["probes"] - 1) - 1                                     # one probe fewer would not reach
            inst.add(sr["inst"]); parities_P.add(c.P[s] % 2)
            # the search itself, restated: with the restated probe count it is nearest_first on every designed score; with the probes of
            # ceil-less pairs = m / 2 (one fewer at the lower end of a class) some score of the tight bucket comes back wrong
            x0 = np.unique(c.planes[s][0][np.isfinite(c.planes[s][0])])
            x0 = np.concatenate([x0[(x0 >= b - 1) & (x0 < b + 2)] for b in des.values()] + [c.planes[s][0][~np.isfinite(c.planes[s][0])]])
            assert np.array_equal(T.lookup_sim(tab, 16384, x0, sr["probes"]), T.nearest_first(tab, x0)), key
            short = max((m // 2).bit_length(), 1)             # (the switch runs one probe where the header says none)
            if short < sr["probes"]:
                wrong = np.flatnonzero(T.lookup_sim(tab, 16384, x0, short) != T.nearest_first(tab, x0))
                assert len(wrong) and np.all(np.floor(x0[wrong]) == des["tight"]), (key, m, x0[wrong])
                fewer.add(m)
            # the designed scores: every entry of every designated bucket is some score's answer, and so are exact ties
            k = T.nearest_first(tab, c.planes[s][0])
            for b in des.values():
                assert set(range(sr["lut"][b], sr["lut"][b + 1])) <= set(k.tolist())
            x = c.planes[s][0]
            with np.errstate(invalid="ignore"):
                ties = np.isfinite(x) & (k + 1 < len(tab)) & (np.abs(tab[k] - x) == np.abs(tab[np.minimum(k + 1, len(tab) - 1)] - x)) & (tab[k] < x)
            assert ties.sum() >= 4 * (m - 1)
            assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x < tab[0]).any() and (x > tab[-1]).any() and np.signbit(x[x == 0]).any()
        if c.S == 2:
            a, b = (T.A_INST[m] for m in ms)
            assert a != b
    assert inst == {1, 2, 3, 4, "loop"} and parities_P == {0, 1} and fewer == {3, 7, 15, 31}      # the odd sizes: where m / 2 pairs need a probe fewer
    assert {T.A_INST[m] for m in T.A_M} == inst and sorted(T.A_M) == [1, 2, 3, 6, 7, 14, 15, 30, 31, 33, 64]    # both sides of 2|3, 6|7, 14|15, 30|31


def test_group_b_lands_every_plateau_length():
    want = set(T.RUN_LENGTHS)
    assert want == set(range(1, 10)) | {33}
    runs_seen, round_seen, insts = set(), set(), set()
    for key in T.group("B"):
        c = T.case(key)
        for s, tab in enumerate(c.tabs):
            sr = T.search(tab, 16384)
            insts.add(sr["inst"])
            k, run = T.nearest_first(tab, c.planes[s][0], lengths=True)
            x = c.planes[s][0]
            if "runs" in key:
                for b, L in c.runs:            # on a run, just above it, between the bucket's two runs: the run's FIRST entry, L entries back
                    for base, xs in ((b + 0.25, (b + 0.25, T.up(b + 0.25), b + 0.3, b + 0.5)), (b + 0.75, (b + 0.75, T.up(b + 0.75), b + 0.9, T.down(b + 1)))):
                        first = int(np.searchsorted(tab, np.float32(base), side="left"))
                        assert np.all(tab[first: first + L] == np.float32(base)) and tab[first - 1] < base < tab[first + L]
                        for xv in xs:
                            at = np.flatnonzero(x == np.float32(xv))
                            assert len(at) and np.all(k[at] == first) and np.all(run[at] == L), (key, b, L, xv)
                    runs_seen.add(L)
            else:
                L = np.flatnonzero(x == np.float32(2.0 ** 30))
                assert len(L) and np.all(np.diff(tab) >= 2.0) and np.sum(np.diff(tab) > 2.0) == 1      # distinct entries, spacing 2.0 but for one gap
                round_seen |= set(run[L].tolist())
                assert np.all(k[L] == len(tab) - run[L])
    assert runs_seen >= want and round_seen == want, (sorted(runs_seen), sorted(round_seen))
    assert {4, "loop"} <= insts                       # the plateau walk behind the unrolled search and behind the loop
    assert T.search(T.case("B-runs-1to9").tabs[0], 16384)["fullest_bucket"] == 18 and T.search(T.case("B-runs-33").tabs[0], 16384)["fullest_bucket"] == 66


def test_group_c_stands_on_both_sides_of_every_plan_threshold():
    seen = {}
    for key in T.group("C"):
        c = T.case(key)
        P = c.P[0]
        pl = [c.plan(n) for n in T.NORMS]
        seen[P] = None if pl[0] is None else (pl[0]["lutb"], pl[1]["val_in_lds"])
        assert (pl[0] is None) == (pl[1] is None) == (c.path == "row") == (P == 39381)
        lutb = T.PLAN_LUTB[P] or 2048
        sr = T.search(c.tabs[0], lutb)
        assert sr["inv_w"] == 1.0 and sr["fullest_bucket"] == T.PLAN_M and sr["inst"] == 4
        top = [f for b, f, n in T.fullest(c.tabs[0], lutb) if b == lutb - 1]
        assert top == [P - T.PLAN_M]                                                               # the designed top bucket
        x = c.planes[0][0]
        assert (x == c.tabs[0][-1]).any() and (x > c.tabs[0][-1]).sum() >= 3 and np.isposinf(x).any()
    assert seen == {16084: (16384, True), 16085: (16384, False), 32212: (16384, False), 32213: (8192, False), 36308: (8192, False), 36309: (4096, False),
                    38356: (4096, False), 38357: (2048, False), 39380: (2048, False), 39381: None}


def test_group_d_mixes_table_lengths_in_one_call():
    for key in T.group("D"):
        c = T.case(key)
        assert tuple(c.P) in T.MIXED_P and c.S == 4 and ((c.ranks is not None) == key.endswith("-partial"))
        for norm in T.NORMS:
            pl = c.plan(norm)
            assert len(set(pl["Ppad"])) >= 3 and pl["tab_cap"] == max(pl["Ppad"]) > min(pl["Ppad"]) == 256 and not pl["val_in_lds"]
            srs = c.searches(norm)
            assert {sr["inst"] for sr in srs} >= {1, "loop"} or min(c.P) > 2                     # short tables: one probe; long ones at few buckets: the loop
        if c.ranks is not None:
            assert [r is not None for r in c.ranks] == [False, False, True, False] and (c.ranks[2] < 0).any()
    assert T.search(T.case("D-P1+2+10001+39380").tabs[0], 2048)["fullest_bucket"] == 1 and T.search(np.float32([0.5]), 2048)["inv_w"] == 0.0


def test_group_e_rows_end_at_every_tail():
    Ns = []
    for key in T.group("E"):
        c = T.case(key)
        Ns.append(c.N)
        assert (c.S, c.Q, c.P) == (2, 3, [10001, 10001]) and c.ranks[0] is None and (c.ranks[1] < 0).any() == (c.N > 1)
        assert c.ranks[1][0, c.N - 1] != c.ranks[1][1, c.N - 1] or c.N == 1                       # the row's last validity bit differs from row to row
    assert tuple(Ns) == T.TAIL_N == (1, 2, 3, 4, 5, 7, 31, 33, 28671, 28672, 28673, 28675, 57344, 57345)
    assert {N % 4 for N in Ns} == {0, 1, 2, 3} and {N % 32 != 0 for N in Ns} == {True, False}
    assert {(N - 1) // T.BT_COLS + 1 for N in Ns} == {1, 2, 3} and T.BT_COLS == 28672


def test_group_f_walks_past_the_grid_and_carries():
    seen = {}
    for key in T.group("F"):
        c = T.case(key)
        wk = T.walk(c.Q, c.N)                      # (asserts (q, c) == divmod(item, chunks) at every step of every workgroup)
        seen[(c.Q, c.N)] = (wk["items"], wk["chunks"], wk["carries"])
        assert wk["grid"] == min(wk["items"], 256) and c.P[0] in (10001, 20000) and c.S in (1, 2)
        assert (wk["carries"] > 0) == ((c.Q, c.N) in T.WALK_CARRY), key
        assert c.plan(T.NORMS[1])["val_in_lds"] == (c.P[0] == 10001)                               # NCE at P = 20,000: values swapped over the table
    assert seen == {(255, 64): (255, 1, 0), (256, 64): (256, 1, 0), (257, 64): (257, 1, 0), (513, 64): (513, 1, 0), (129, 28673): (258, 2, 0),
                    (86, 57345): (258, 3, 0), (171, 57345): (513, 3, seen[(171, 57345)][2])}
    assert seen[(171, 57345)][2] >= 85             # workgroups whose chunk index wraps, with an item behind the wrap


def test_group_g_asks_for_every_quotient():
    for key in T.group("G"):
        c = T.case(key)
        P = c.P[0]
        assert P in T.QUOT_P and c.N == P and c.w == [1.0] and np.all(np.diff(c.tabs[0]) > 0)
        assert np.array_equal(T.nearest_first(c.tabs[0], c.planes[0][0]), np.arange(P))
        exp = c.expected(T.NORMS[0])[0]
        assert np.array_equal(T.bits(exp), T.bits(np.arange(P, dtype=np.float32) / np.float32(P)))
        assert np.array_equal(exp, (np.arange(P, dtype=np.float64) / P).astype(np.float32))        # k and P are exact in float32: the correctly rounded quotient
    assert T.QUOT_P == (10001, 27943, 32749, 39380)


def test_group_h_degenerates_the_bucket_table():
    c = T.case("H-denormal")
    sr = T.search(c.tabs[0], 16384)
    assert sr["inv_w"] == 0.0 and sr["fullest_bucket"] == 10001 and sr["inst"] == "loop" and 2 ** sr["probes"] - 1 >= 5001 and sr["lut"][1] == 10001
    assert len(np.unique(T.nearest_first(c.tabs[0], c.planes[0][0]))) > 150
    c = T.case("H-const+ordinary")
    a, b = c.searches(T.NORMS[0])
    assert a["inv_w"] == 0.0 and a["fullest_bucket"] == 10001 and b["inv_w"] > 0 and b["inst"] != "loop" and np.all(c.tabs[0] == 1.5)
    assert not T.nearest_first(c.tabs[0], c.planes[0]).any()
