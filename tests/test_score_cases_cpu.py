"""The case tables of the exact score-GEMM tests (score_cases.py), checked without a GPU: every case lands the branches it claims and their
union lands every branch of score_cases.BRANCHES -- derived from fz_dot_scores_plan, the function the launcher itself runs, at 256 compute
units -- the tiles of every plan store each cell of [Q, N] exactly once, the float64 references are exactly representable in float32, the
operand views reach the kernels uncopied, and fz_dot_scores_plan judges its arguments."""
import os
import subprocess
import sys

import numpy as np
import pytest

import score_cases as S
from fusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUP = _lib.FZ_OK, _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_branch_table_is_covered():
    hit = set()
    for c in S.ALL_CASES:
        b = S.branches_of(c, S.CPU_CUS)
        assert b <= set(S.BRANCHES), (c.id, sorted(map(str, b - set(S.BRANCHES))))      # no branch name outside the table
        assert set(c.claims) <= b, (c.id, sorted(map(str, set(c.claims) - b)))
        hit |= b
    assert set(S.BRANCHES) <= hit, sorted(map(str, set(S.BRANCHES) - hit))
    first, missing = S.landing(S.ALL_CASES, S.CPU_CUS)
    assert not missing
    for b in sorted(S.BRANCHES, key=str):              # (pytest -s: which case lands which branch)
        print(b, "<-", first[b])


def test_the_case_axes_of_the_tables():
    ids = {c.id for c in S.ALL_CASES}
    for Q in (1, 32, 33, 64, 65, 66, 67, 68, 69, 96, 97, 127, 128, 129, 160, 192, 193, 194, 195, 196, 224, 225, 257):
        assert f"rows-store-Q{Q}-N257-d36" in ids, Q
    for N in (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1283):
        assert any(c.epi == S.EPI_STORE and c.N == N and c.name == "cols" for c in S.CASES), N
    for d in (4, 28, 32, 36, 60, 64, 68, 124, 128, 132, 192, 196):
        assert {c.Q for c in S.CASES if c.epi == S.EPI_STORE and c.name == "k" and c.d == d} == set(S.K_ROWS), d
    f = S.FILTER_CASES
    assert {1, 33, 64, 65, 96, 97, 128, 129, 160, 257} <= {c.Q for c in f} and {1, 127, 128, 129, 1283} <= {c.N for c in f}
    assert {4, 36, 64, 68, 132} <= {c.d for c in f}
    assert {(c.Q, c.nan) for c in f if c.nan} == {(Q, k) for Q in (33, 97, 129) for k in ("corpus", "query")}
    assert all(c.N <= 1283 for c in f if c.nan)
    assert {c.V for c in S.SPLADE_CASES} >= {1, 63, 64, 65, 127, 128, 129, 509} and {c.d for c in S.SPLADE_CASES} >= {8, 36, 64, 68}


@pytest.mark.parametrize("case", S.ALL_CASES, ids=lambda c: c.id)
def test_the_tiles_of_a_plan_store_every_cell_once(case):
    """tiles_of (the kernel's id -> tile map over the library's plan) covers [Q, N] exactly once: no cell twice, none left out."""
    p = S.plan(case.Q, case.N, case.d, case.epi, S.CPU_CUS)
    cnt = S.cover_count(p, case.Q, case.N)
    assert cnt.min() == 1 and cnt.max() == 1, (case.id, p, int(cnt.min()), int(cnt.max()))
    assert p["grid"] == len({t[0] for t in S.tiles_of(p)})      # every workgroup launched has an id to start from


def test_the_cover_limit_cases_sit_on_the_limit():
    at = lambda Q, N: S.plan(Q, N, 8, S.EPI_STORE, S.CPU_CUS)
    assert at(197, S.COVER_LAST_N)["cover7"] == 1 and at(197, S.COVER_LAST_N + 1)["cover7"] == 0
    assert at(197, S.COVER_LAST_N)["nP"] + at(197, S.COVER_LAST_N)["nQ"] == S.CPU_CUS
    p = at(195, S.COVER_LAST_N)     # 195 rows ride as 192 + a 3-row slab: the cover never sees them while the slabs are on
    assert (p["cover7"], p["slab_rows"], p["slab_row0"], p["rows"], p["tail_rows"]) == (0, 3, 192, 192, 64)


# ---- references ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_the_reference_is_exact_in_float32(case):
    A, B = case.inputs()
    for M in (A, B):
        v = M[~np.isnan(M)]
        assert np.array_equal(v * 4, np.round(v * 4)) and np.abs(v).max() <= 2
    ref = case.ref(A, B)
    assert ref.shape == (case.Q, case.N) and np.array_equal(ref, ref.astype(np.float32), equal_nan=True)
    # ... and is the sum of the products in any order: here one term at a time, in float64
    slow = np.zeros_like(ref)
    for k in range(case.d):
        slow += A[:, k: k + 1] * B[None, :, k]
    assert np.array_equal(slow, ref, equal_nan=True)
    assert int(np.isnan(ref).sum()) == {"": 0, "corpus": case.Q, "query": case.N}[case.nan]
    if case.epi == S.EPI_FILTER:
        tau = case.thresholds(ref)
        exp = case.expected(ref, tau)
        n = exp.sum(axis=1)
        if case.tau == "rank40":
            assert n.max() <= 39 and n.min() >= 1
        elif not case.nan:
            for q in range(case.Q):
                t = float(tau[q])
                if np.isposinf(t) or t == ref[q].max():
                    assert n[q] == 0
                elif np.isneginf(t):
                    assert n[q] == case.N
                elif case.N >= 127:
                    assert (ref[q] == t).sum() >= 2 and 0 < n[q] < case.N, (q, t)       # ties with tau stay out, something enters
            if case.Q >= 4:
                assert {0, case.N} <= set(n.tolist()) and np.isposinf(tau).any() and np.isneginf(tau).any()
        elif case.nan == "corpus":
            assert n.min() >= 1                                  # the NaN document enters every list, at tau = +inf too
        else:
            assert n[-1] == case.N


@pytest.mark.parametrize("case", S.SPLADE_CASES, ids=lambda c: c.id)
def test_splade_inputs(case):
    X, W, bias, cu, marks = case.inputs()
    T, V, d = case.T, case.V, case.d
    assert X.shape == (T, d) and W.shape == (V, d) and bias.shape == (V,) and cu[0] == 0 and cu[-1] == T and (np.diff(cu) >= 0).all()
    assert ((X != 0).sum(axis=1) <= 4).all() and np.abs(X).max() <= 1 and np.abs(W).max() <= 1 and np.abs(bias).max() <= 2
    for M in (X, W, bias):
        assert np.array_equal(M * 4, np.round(M * 4))
    assert (X != 0).any(axis=0).all(), "a k that no row touches"
    assert (X[:, -4:] != 0).all(axis=1).any(), "no row fills the last float4 before d"
    logits = case.logits(X, W, bias)
    assert np.array_equal(logits, logits.astype(np.float32)) and np.abs(logits).max() <= 6
    # the layout: a cut on every offset of the tile, one-row and empty sequences, a sequence over three tiles, a padded last block
    lens = np.diff(cu)
    assert {int(c) % 128 for c in cu} == set(range(128)) and {128, 256, 384} <= set(cu.tolist())
    assert T % 128 or T == 1024          # the last block is padded (the half-tile shape of the issue, T = 1024, is run beside T = 1085)
    assert (lens == 1).sum() >= 3
    empty = lens == 0
    assert empty[:2].all() and empty[-2:].all() and any(empty[i: i + 3].all() for i in range(2, len(lens) - 4))
    assert any(a // 128 + 2 <= (b - 1) // 128 for a, b in zip(cu[:-1], cu[1:]) if b > a), "no sequence spans three tiles"
    # the marks: the row before and the row after a cut hold the maximum (>= 2) of a column of their own, >= 1 above every row of the tiles around
    inner = sorted({int(c) for c in cu if 0 < c < T})
    assert len({v for _, _, v in marks}) == len(marks) == min(2 * len(inner), V - 2 if V >= 8 else V)
    if V >= 2 * len(inner) + 2:
        assert {(c, r) for c, r, _ in marks} == {(c, r) for c in inner for r in (c - 1, c)}
    for _, r, v in marks:
        col = logits[:, v].copy()
        top = col[r]
        col[r] = -np.inf
        assert top >= 2 and top >= col.max() and top - col[max(r - 127, 0): r + 128].max() >= 1, (r, v, top, col.max())
    pooled = case.pooled(logits, cu)
    assert pooled.max() < 2 and (pooled[lens == 0] == 0).all()
    if V >= 8:
        assert (logits[:, V - 1] < 0).all() and (pooled[:, V - 1] == 0).all()
        assert (logits[:, V - 2] == 0.25).all() and not (X @ W[V - 2]).any()


def test_unit_rows_are_unit_norm():
    x = S.unit_rows(np.random.default_rng(0), 50, 64)
    assert x.dtype == np.float32 and np.allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_framed_views_are_not_copied_by_pad_dim():
    """The NaN padding tests something only if the views reach the kernel as they are: d % 4 == 0, a row stride % 4 == 0, a 16-byte
    aligned base and a unit inner stride are all that ops.pad_dim asks for (CPU tensors: pad_dim looks at strides and pointers only)."""
    import torch
    from fusion_amd import ops
    for d in (4, 36, 68, 196):
        for before in (0, 1, 2, 3):
            buf, rows, n = S.framed(S.grid(np.random.default_rng(d), 5, d), before=before)
            assert np.isnan(buf[: rows.start]).all() and np.isnan(buf[rows.stop:]).all() and np.isnan(buf[:, n:]).all()
            t = torch.from_numpy(buf)
            base = t.data_ptr() % 16      # (numpy's own allocation: judge the view relative to it)
            v = t[rows, :n]
            assert v.stride(0) == d + 4 and v.stride(0) % 4 == 0 and (v.data_ptr() - t.data_ptr()) % 16 == 0
            if base == 0:
                assert ops.pad_dim(v) is v


# ---- fz_dot_scores_plan ----------------------------------------------------------------------------------------------------------------
def test_plan_is_exported_declared_and_additive():
    L = _lib.lib()
    assert "fz_dot_scores_plan" in _lib.EXPORTS and hasattr(L, "fz_dot_scores_plan")
    assert L.fz_abi_version() == _lib.ABI_VERSION == 20          # an additive entry: the ABI version stays
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    assert "fz_dot_scores_plan(" in header and f"#define FZ_DOT_SCORES_PLAN_FIELDS {len(S.PLAN_FIELDS)}" in header


def test_plan_judges_its_arguments():
    st = lambda *a, **k: S.plan_status(*a, **k)[0]
    assert st(195, 1000, 64, 0, 256) == OK
    for bad in [(-1, 1000, 64, 0, 256), (195, -1, 64, 0, 256), (195, 1000, 0, 0, 256), (195, 1000, -4, 0, 256), (195, 1000, 64, -1, 256),
                (195, 1000, 64, 3, 256), (195, 1000, 64, 0, 0), (195, 1000, 64, 0, -8)]:
        rc, f = S.plan_status(*bad)
        assert rc == ARG and f == [-1] * len(S.PLAN_FIELDS), bad      # refused, nothing written
    assert st(195, 1000, 64, 0, 256, out=False) == ARG
    assert st(195, 1000, 62, 0, 256) == UNSUP                        # the GEMM's d % 4 == 0
    assert st(128, 1000, 64, 0, 3) == UNSUP and st(128, 1000, 64, 0, 4) == OK      # fewer than 8 resident slots
    assert st(1 << 24, 1 << 24, 64, 0, 256) == UNSUP                 # more tile ids than 2^30 - 1
    for Q, N in [(0, 1000), (195, 0), (0, 0)]:                        # an empty problem launches nothing
        rc, f = S.plan_status(Q, N, 64, 1, 256)
        assert rc == OK and f == [0] * len(S.PLAN_FIELDS)


def test_plan_fields_at_the_production_shapes():
    p = S.plan(195, 27942, 768, S.EPI_STORE, 256)        # the LLeQA test batch: one whole block, 64-row tail tiles with a 3-row slab
    assert p == dict(slab_rows=3, slab_row0=192, rows=192, QB=1, TN=219, full=224, halves=0, tail_ids=224, tail_row0=128, tail_rows=64,
                     cover7=0, nP=0, nQ=0, grid=448, ragged=0, slots=512)
    p = S.plan(201, 27942, 768, S.EPI_STORE, 256)        # the dev batch: the cover, one workgroup per CU
    assert (p["cover7"], p["nP"], p["nQ"], p["grid"], p["slab_rows"]) == (1, 146, 110, 256, 0)
    assert S.plan(201, 27942, 768, S.EPI_FILTER, 256)["cover7"] == 0 and S.plan(201, 27942, 768, S.EPI_SPLADE, 256)["cover7"] == 0
    p = S.plan(1024, 1_100_000, 768, S.EPI_FILTER, 256)  # a dense shard: 8 blocks x 8,594 corpus tiles (8,600 ids), the last round halved
    assert (p["QB"], p["TN"], p["full"] + p["halves"] // 2, p["grid"]) == (8, 8594, 8 * 8600, 512) and 0 < p["halves"] <= 512
    p = S.plan(700, 32005, 768, S.EPI_SPLADE, 256)       # SPLADE: the last block is padded, never a tail
    assert (p["QB"], p["tail_ids"], p["tail_rows"], p["slab_rows"]) == (6, 0, 0, 0)
    assert S.plan(195, 1000, 100, 0, 256)["ragged"] == 1 and S.plan(195, 1000, 128, 0, 256)["ragged"] == 0
    for cus in (8, 64, 104, 256, 304):                   # the cover's limit and the slots follow the device
        assert S.plan(200, 192 * cus, 64, 0, cus)["cover7"] == 0 and S.plan(200, 90 * cus, 64, 0, cus)["cover7"] == 1
        assert S.plan(128, 1000, 64, 0, cus)["slots"] == 2 * cus // 8 * 8


def test_plan_honours_the_slab_switch():
    """FZ_GEMM_SLABS=0 (read once per process: a child, with nothing but the library loaded) sends the 65 .. 68-row classes to the 96-row
    tail tiles and 193 .. 196 rows to the cover."""
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); o = (ctypes.c_int32 * 16)(); "
            "assert L.fz_dot_scores_plan(195, 27942, 768, 0, 256, o) == 0; print(o[0], o[9], o[10]); "
            "assert L.fz_dot_scores_plan(67, 1000, 64, 0, 256, o) == 0; print(o[0], o[9], o[10])")
    for env, want in (("0", "0 96 1\n0 96 0\n"), ("1", "3 64 0\n3 64 0\n")):
        r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH], env=dict(os.environ, FZ_GEMM_SLABS=env), capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == want, (env, r.stdout, r.stderr[-500:])
