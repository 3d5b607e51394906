"""CPU side of the weight-sweep rank kernel's edge tests (tests/tune_cases.py, tests/test_gpu_tune_edges.py): the NumPy reference
against a literal lexsort and against the oracle the rest of the suite trusts, the exactness of the exact family, the rounding
sensitivity of the rounding family, every condition the GPU cases rely on (ties on both sides of a gold across chunks and lane
groups, neighbouring weight vectors that rank differently, unlisted columns that would win, ...), and the coverage table: which
branch set of gold_ranks_kernel every case reaches, and that together they reach all of it."""
import os
import re

import numpy as np
import pytest

import tune_cases as tc
from conftest import GOLDEN, ROOT
from helpers import load_lists

EXACT = [n for n in tc.NAMES if n.split("-")[0] in ("cols", "systems", "slots", "unlisted", "signs") or re.match(r"weights-W\d+-", n)]


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "fusion_amd", "csrc", "tune.hip")).read()
    val = lambda name: int(re.search(rf"\b{name} = (\d+)", src).group(1))
    assert (val("TUNE_G"), val("TUNE_WCHUNK"), val("TUNE_COLS_F32"), val("TUNE_COLS_F64")) == \
        (tc.G, tc.WCHUNK, tc.COLS_F32 // tc.THREADS, tc.COLS_F64 // tc.THREADS)
    assert "__launch_bounds__(256, 2) void gold_ranks_kernel" in src and tc.THREADS == 256 and tc.WAVE == 64


def test_lattice_is_the_references_grid():
    from fusion_amd.retrievers.hybrid import weight_grid
    for S, n in ((2, 21), (3, 231), (4, 1771)):
        names = list("abcd")[:S]
        L = tc.lattice(S)
        assert L.shape == (n, S) and [[w[k] for k in names] for w in weight_grid(names)] == L.tolist()
        assert all(type(x) is np.float64 for x in weight_grid(names)[0].values())


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.NAMES)
def test_reference_equals_a_literal_stable_sort(name):
    """Counting with plain comparisons == the position in np.lexsort(pos, -score, not-NaN) of the listed columns, on every case
    (the long weight lists on their first, last and pass-border vectors)."""
    c = tc.case(name)
    rows = np.arange(c.W) if c.W <= 30 else np.unique(np.clip([0, 1, 510, 511, 512, 513, 1023, 1024, c.W - 1], 0, c.W - 1))
    exp = tc.lexsort_ranks(c.T, c.pos, c.weights[rows], c.gold, c.wide)
    assert np.array_equal(tc.reference(name)[rows], exp)
    ok, _, _ = tc.listed_golds(c.pos, c.gold)
    assert not tc.reference(name)[:, ~ok].any()


def test_reference_on_a_hand_made_row():
    T = [np.array([[1.0, np.nan, 1.0, -0.0, 0.0, np.inf, 5.0, np.nan]], dtype=np.float32)]
    pos = np.array([[3, 1, 0, 2, 4, 5, -1, 6]], dtype=np.int32)
    gold = np.array([[0, 1, 2, 3, 4, 5, 6, 9]], dtype=np.int32)
    for wide in (False, True):      # order: NaN(1) NaN(7) inf(5) 1.0(2) 1.0(0) -0.0(3) +0.0(4); column 6 is in no list, 9 is past the row
        assert tc.gold_ranks_ref(T, pos, np.array([[1.0]]), gold, wide).tolist() == [[[4, 0, 3, 5, 6, 2, 0, 0]]]
        assert tc.gold_ranks_ref(T, pos, np.array([[0.0]]), gold, wide).tolist() == [[[5, 0, 3, 4, 6, 1, 0, 0]]]   # inf * 0 = NaN: 1, 5, 7, then the zeros by pos: 2, 3, 0, 4


def test_reference_equals_the_oracles_fused_lists():
    """On the committed tune fixture (three systems, a partial ColBERT list first): the reference's ranks of the gold ids == their
    positions in oracle.fuse_lists for every ninth weight vector of the grid, np.float64 weights (the wide sweep)."""
    from oracle import oracle
    oracle.build()
    z = np.load(os.path.join(GOLDEN, "tune_seed21_S3_Q4_N257_colbert_first.npz"), allow_pickle=False)
    systems, lists, Q = load_lists(z)
    labels = [[int(x) for x in str(s).split(",")] for s in z["labels"]]
    _, ids, planes, ranks, orders, lens, _ = oracle.lists_to_planes(lists)
    N = planes[0].shape[1]
    assert any((r < 0).any() for r in ranks)
    T = [np.where(ranks[s] >= 0, oracle.fuse_nsf([planes[s]], [ranks[s]], [1.0], "min-max"), np.float32(0.0)) for s in range(len(systems))]
    ins, U = oracle.insertion_order(orders, lens, N)
    pos = np.full((Q, N), -1, dtype=np.int32)
    for q in range(Q):
        pos[q, ins[q, :U[q]]] = np.arange(U[q])
    id2pos = {int(c): j for j, c in enumerate(ids)}
    gold = tc.pad_gold([[id2pos.get(g, -1) for g in dict.fromkeys(gl)] for gl in labels])
    W = z["weights"][::9]
    got = tc.gold_ranks_ref(T, pos, W, gold, wide=True)
    checked = 0
    for wi, wv in enumerate(W):
        fl = oracle.fuse_lists(lists, "nsf", "min-max", {s: np.float64(x) for s, x in zip(systems, wv)}, {})
        for q in range(Q):
            rank_of = {x["corpus_id"]: r for r, x in enumerate(fl[q])}
            for g in range(tc.G):
                if gold[q, g] >= 0 and ids[gold[q, g]] in rank_of:
                    assert got[wi, q, g] == rank_of[ids[gold[q, g]]], (wi, q, g)
                    checked += 1
                else:
                    assert got[wi, q, g] == 0
    assert checked >= 3 * len(W)


# ---- the exact family ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXACT)
def test_exact_family_is_exact_four_ways(name):
    """Narrow == wide == reversed system order == integer arithmetic scaled by 256, score for score and rank for rank."""
    c = tc.case(name)
    Ti = [np.rint(t.astype(np.float64) * 8).astype(np.int64) for t in c.T]
    Wi = np.rint(c.weights * 32).astype(np.int64)
    assert all(np.array_equal(ti / 8.0, t) and np.abs(ti).max() <= 16 for ti, t in zip(Ti, c.T)) and np.array_equal(Wi / 32.0, c.weights)
    assert np.abs(Wi).max(initial=0) <= 32 and c.S <= 4
    rows = np.arange(c.W) if c.W <= 30 else np.arange(0, c.W, 37)
    for w in rows:
        exact = sum(Ti[s] * Wi[w, s] for s in range(c.S)) / 256.0
        for wide in (False, True):
            for order in (None, range(c.S - 1, -1, -1)):
                f = tc.fused(c.T, c.weights[w], wide, order)
                assert np.array_equal(f.astype(np.float64), exact)
    ref = tc.reference(name)[rows]
    for wide in (False, True):
        for order in (None, range(c.S - 1, -1, -1)):
            assert np.array_equal(tc.gold_ranks_ref(c.T, c.pos, c.weights[rows], c.gold, wide, order), ref)


def test_fused_score_is_never_minus_zero():
    """0 + (-0.0) = +0.0: the kernel's fast key has no -0.0 case because a sum that starts at +0 cannot produce one."""
    for name in ("signs-narrow", "signs-wide"):
        c = tc.case(name)
        for w in c.weights:
            f = tc.fused(c.T, w, c.wide)
            assert not np.signbit(f[f == 0]).any()
        assert any(np.signbit(t[t == 0]).any() for t in c.T) and (c.weights < 0).any()


@pytest.mark.parametrize("name", [n for n in tc.NAMES if n.startswith("cols-")])
def test_column_cases_tie_on_both_sides_and_sum_over_workgroups(name):
    c = tc.case(name)
    E = tc.edge_columns(c.N)
    assert sorted(c.gold[0][c.gold[0] >= 0].tolist()) == E and {0, c.N - 1} <= set(E) and len({tuple(r) for r in c.gold.tolist()}) == min(3, 1 + c.N)
    both, cross = tc.tie_census(c)
    if c.N >= 65:
        assert both, "some weight vector leaves no gold with tied columns of smaller and of larger pos"
    assert cross == (name in tc.TIE_CROSSING), "a tie in another chunk and lane group, exactly where the row spans two chunks"
    cols = tc.chunk_cols(c.wide)
    if c.N > cols:      # for every weight vector some gold gets most of its rank from workgroups other than its own
        ok, col, pg = tc.listed_golds(c.pos, c.gold)
        j = np.arange(c.N)
        for w in c.weights:
            f = tc.fused(c.T, w, c.wide)
            before = tc.precedes(f, c.pos, np.take_along_axis(f, col, axis=1), pg)
            away = (before & (j[None, None, :] // cols != (col // cols)[:, :, None])).sum(axis=2)
            assert (ok & (2 * away > before.sum(axis=2))).any()


# ---- the rounding family -------------------------------------------------------------------------------------------------------------
def test_exact_fma_equals_fractions_on_a_sample():
    from fractions import Fraction
    c = tc.case("rounding-S4-wide")
    cols = np.arange(0, c.N, 65)[:64]
    T = [t[:, cols] for t in c.T]
    for w in c.weights[[3, 11, 20]]:
        acc = np.zeros(T[0].shape).ravel().tolist()
        for s in range(c.S):
            acc = [float(Fraction(float(t)) * Fraction(float(w[s])) + Fraction(a)) for t, a in zip(T[s].ravel().tolist(), acc)]
        assert np.array_equal(tc.fused_fma_wide(T, w).ravel(), np.array(acc))


def changed(a, b):
    """Fraction of weight vectors whose [Q, 8] ranks differ."""
    return float(np.mean([not np.array_equal(x, y) for x, y in zip(a, b)]))


@pytest.mark.parametrize("name", tc.ROUNDING)
def test_rounding_family_ranks_depend_on_every_rounding(name):
    """On the reference alone: a fused multiply-add, the reversed system order and the other sweep's width each change the ranks of
    at least a quarter / a quarter / half of the weight vectors, and no two neighbouring vectors rank alike.  S = 2 cannot meet the
    order condition and is held to the opposite: 0 + p0 is exact and p0 + p1 == p1 + p0, so both orders are the same two roundings."""
    c = tc.case(name)
    ref = tc.reference(name)
    args = (c.T, c.pos, c.weights, c.gold, c.wide)
    fma = tc.gold_ranks_ref(*args, fuse=tc.fused_fma_wide if c.wide else tc.fused_fma_narrow)
    rev = tc.gold_ranks_ref(*args, order=range(c.S - 1, -1, -1))
    other = tc.gold_ranks_ref(c.T, c.pos, c.weights, c.gold, not c.wide)
    print(name, "fma", changed(ref, fma), "reversed", changed(ref, rev), "other width", changed(ref, other))
    assert changed(ref, fma) >= 0.25
    assert changed(ref, rev) >= 0.25 if c.S > 2 else changed(ref, rev) == 0.0
    assert changed(ref, other) >= 0.5
    assert np.array_equal(tc.reference(name.replace("wide", "narrow") if c.wide else name.replace("narrow", "wide")), other)


@pytest.mark.parametrize("name", tc.ADJACENT)
def test_neighbouring_weight_vectors_rank_differently(name):
    """What the weight-chunk cases rely on: a vector read at the wrong index, or a count left over from the previous pass over the
    LDS counters (the vector TUNE_WCHUNK earlier), gives other ranks."""
    ref = tc.reference(name)
    assert all(not np.array_equal(ref[w], ref[w + 1]) for w in range(len(ref) - 1))
    assert all(not np.array_equal(ref[w], ref[w - tc.WCHUNK]) and (ref[w] + ref[w - tc.WCHUNK] != ref[w]).any() for w in range(tc.WCHUNK, len(ref)))


# ---- what the single cases promise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", tc.SWEEPS)
def test_gold_slot_cases(sweep):
    a, b, d = (tc.case(f"slots-{x}-{sweep}") for x in "ABC")
    N = a.N
    assert (a.gold[0] == -1).all() and (a.gold[1] >= 0).tolist() == [False, True, False, False, True, False, True, False] and (a.gold[2] >= 0).all()
    assert not tc.reference(a.name)[:, 0].any()
    assert {N, N + 5} <= set(b.gold[0].tolist())
    rb = tc.reference(b.name)
    assert b.gold[1, 1] == b.gold[1, 6] >= 0 and np.array_equal(rb[:, 1, 1], rb[:, 1, 6]) and rb[:, 1, 1].any()
    unl = [g for g in b.gold[2] if g >= 0 and b.pos[2, g] < 0]
    assert len(unl) == 2 and not rb[:, 2, [1, 5]].any()
    rd = tc.reference(d.name)
    U = (d.pos >= 0).sum(axis=1)
    for q, (first, last) in enumerate([(0, 4), (6, 1), (3, 6)]):
        assert (rd[:, q, first] == 0).all() and (rd[:, q, last] == U[q] - 1).all()
    ng = sorted(n for x in (a, b, d) for n in tc.branches(x)["ng"])
    assert ng == [0, 1, 2, 3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("sweep", tc.SWEEPS)
def test_unlisted_columns_would_beat_every_gold(sweep):
    c = tc.case(f"unlisted-{sweep}")
    ok, col, _ = tc.listed_golds(c.pos, c.gold)
    assert 0.30 <= (c.pos[:2] < 0).mean() <= 0.37 and (c.pos[2] >= 0).sum() == 1 and (c.weights > 0).all()
    for w in c.weights:
        f = tc.fused(c.T, w, c.wide)
        for q in range(2):
            assert f[q][c.pos[q] < 0].min() > f[q][col[q][ok[q]]].max()
    ref = tc.reference(c.name)
    assert not ref[:, 2].any() and not ref[:, 1, 6:].any() and ok[2].tolist() == [False, True] + [False] * 6
    listed_all = tc.gold_ranks_ref(c.T, np.where(c.pos < 0, 1 << 20, c.pos), c.weights, c.gold, c.wide)
    assert (listed_all[:, :2][:, ok[:2]] >= ref[:, :2][:, ok[:2]] + (c.pos[:2] < 0).sum(axis=1).min()).all()


@pytest.mark.parametrize("sweep", tc.SWEEPS)
def test_signs_case(sweep):
    c = tc.case(f"signs-{sweep}")
    assert (tc.fused(c.T, c.weights[0], c.wide)[0] < 0).all()
    f1 = tc.fused(c.T, c.weights[3], c.wide)[1]
    assert (f1 < 0).any() and (f1 > 0).any() and (f1 == 0).any()
    assert not c.weights[1].any() and np.array_equal(tc.reference(c.name)[1], np.take_along_axis(c.pos, c.gold.astype(np.int64), axis=1))
    assert all(not t[2].any() for t in c.T) and np.array_equal(tc.reference(c.name)[:, 2], np.broadcast_to(c.pos[2, c.gold[2]], (c.W, tc.G)))


@pytest.mark.parametrize("name", [n for n in tc.NAMES if n.startswith("nonfinite-")])
def test_nonfinite_case(name):
    c = tc.case(name)
    cols = tc.chunk_cols(c.wide)
    odd = ~np.all([np.isfinite(t) for t in c.T], axis=0)
    assert all(np.isposinf(t).any() and np.isneginf(t).any() and np.isnan(t).any() for t in (c.T[0],)) and np.abs(c.weights).max() <= 1
    g0, g1, g2 = (c.gold[q][c.gold[q] >= 0] for q in range(3))
    assert odd[0, : cols].any() and (g0 < cols).all() and odd[0, g0].any()                       # in the golds' own chunk
    assert not odd[1, : 8000].any() and odd[1, 8000:].any() and (g1 < cols).all() and 8000 // cols > 0   # only in another chunk
    assert np.isnan(c.T[0][2, g2[0]]) and np.isposinf(c.T[0][2, g2[1]]) and np.isneginf(c.T[0][2, g2[2]])       # the gold itself
    f = [tc.fused(c.T, w, c.wide) for w in c.weights]
    assert np.isnan(f[0][0, 7 + 8]) and np.isinf(c.T[c.S - 1][0, 7 + 8]) and c.weights[0, c.S - 1] == 0            # 0 * inf
    assert np.isnan(f[2][0, 7 + 6]) and c.T[0][0, 13] == np.inf and c.T[c.S - 1][0, 13] == -np.inf                 # inf + -inf
    assert all(np.isfinite(x[~odd]).all() for x in f)
    ref = tc.reference(name)
    nan_listed = lambda w, q: int((np.isnan(f[w][q]) & (c.pos[q] >= 0)).sum())
    assert c.pos[2, 4500] < c.pos[2, 40] < c.pos[2, 8100]
    for w in range(c.W):                  # the NaN gold: behind exactly the NaN columns of smaller pos; a finite or infinite gold: behind every NaN
        if np.isnan(f[w][2, 40]):
            assert ref[w, 2, 0] == int((np.isnan(f[w][2]) & (c.pos[2] >= 0) & (c.pos[2] < c.pos[2, 40])).sum()) >= 1
        assert ref[w, 1, 0] >= nan_listed(w, 1) and ref[w, 1, 0] > 0
    assert tc.branches(c)["special"] == {True, False}


@pytest.mark.parametrize("sweep", tc.SWEEPS)
def test_low_bits_case(sweep):
    c = tc.case(f"lowbits-{sweep}")
    cols = c.gold[0][c.gold[0] >= 0]
    for w in c.weights[:3]:
        n, d = tc.fused(c.T, w, False), tc.fused(c.T, w, True)
        assert len(set(n[0, cols[:3]].tolist())) == 1 and len(set(n[0, cols[3:]].tolist())) == 1            # tied in float32 ...
        assert len(set(d[0, cols].tolist())) == 6                                                          # ... and not in float64
    d = tc.fused(c.T, c.weights[0], True)[2, cols].view(np.uint64)
    assert len(set((d[:3] >> np.uint64(32)).tolist())) == 1 and len(set((d[3:] >> np.uint64(32)).tolist())) == 1 and len(set(d.tolist())) == 6
    assert d[0] >> np.uint64(63) == 0 and d[3] >> np.uint64(63) == 1                                        # both branches of the fast key
    wide = tc.case("lowbits-wide")
    assert not np.array_equal(tc.reference("lowbits-narrow")[:, [0, 2]], tc.reference("lowbits-wide")[:, [0, 2]])
    # row 1: the gold's copies sit in two waves of the wide sweep's second chunk; no other wave of the row holds a key equal to a gold's
    ok, col, _ = tc.listed_golds(wide.pos, wide.gold)
    f = tc.fused(wide.T, wide.weights[0], True)[1]
    eq = np.flatnonzero(np.isin(f, f[col[1][ok[1]]]))
    assert sorted(eq.tolist()) == sorted([5, 130, 2048 + 70, 2500, 4000])
    assert tc.second_pass_census(wide) == {True, False} and tc.tie_census(wide)[0]


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_branch():
    table = {n: tc.branches(tc.case(n)) for n in tc.NAMES}
    for sweep, chunks in (("narrow", {1, 2, 3}), ("wide", {1, 2, 3, 4, 5})):
        mine = [b for b in table.values() if b["sweep"] == sweep]
        assert {b["chunks"] for b in mine} == chunks
        assert {b["passes"] for b in mine} == {1, 2, 3, 4}
        assert set().union(*(b["ng"] for b in mine)) == set(range(tc.G + 1))
        assert set().union(*(b["special"] for b in mine)) == {True, False}
        assert set().union(*(b["second_pass"] for b in mine)) == ({True, False} if sweep == "wide" else set())
        # the long weight lists span more than one workgroup per pass on the wide sweep, and the pass borders sit where W says
        assert {(b["passes"], b["chunks"]) for n, b in table.items() if n.startswith("weights-") and b["sweep"] == sweep} == \
            {(p, 2 if sweep == "wide" else 1) for p in (1, 2, 3, 4)}
    assert [table[f"weights-W{w}-wide"]["passes"] for w in tc.WEIGHT_WS] == [1, 1, 1, 1, 2, 2, 3]
    assert [table[f"cols-N{n}-narrow"]["chunks"] for n in tc.COLUMN_NS] == [1] * 12 + [2, 2, 3]
    assert [table[f"cols-N{n}-wide"]["chunks"] for n in tc.COLUMN_NS] == [1] * 9 + [2, 2, 2, 3, 4, 5]
    assert len(tc.NAMES) == len(set(tc.NAMES)) and all(tc.case(n).Q == 3 for n in tc.NAMES)
    for n in tc.NAMES:                  # three different rows: a wrong row offset shows
        c = tc.case(n)
        assert c.N == 1 or not (np.array_equal(c.T[0][0], c.T[0][1]) or np.array_equal(c.T[0][1], c.T[0][2]))
