"""The yardstick of test_gpu_encoder_edges.py, checked without a GPU: every float32 expectation of encoder_cases.py against the float64
formula of the same operation, the premises that make the attention inputs exact, and the restated launch arithmetic that tells which
tile, lane, lap and slab a case lands on."""
import numpy as np
import pytest

import encoder_cases as E


@pytest.fixture(scope="module")
def built():
    return {c.family: c.build() for c in E.ATTN_CASES}


# ---- attention ---------------------------------------------------------------------------------------------------------------
def test_codes_and_the_base2_constant_are_exact():
    u = E.CODES
    assert u.shape == (128, 64) and np.array_equal(np.abs(u), np.full_like(u, 4.0))
    assert np.array_equal(u.astype(np.float16).astype(np.float64), u)
    g = u @ u.T
    assert np.array_equal(np.diag(g), np.full(128, 1024.0))
    off = g[~np.eye(128, dtype=bool)]
    assert off.max() == 0 and set(np.unique(off)) == {0.0, -1024.0}
    c = E.SCALE_LOG2E
    assert c.dtype == np.float32 and float(np.float32(1024) * c) == 1024.0 * float(c)          # 1024 c is exact: the winner's exponent is 0
    gap = np.float32(0) * c - np.float32(1024) * c
    assert float(gap) <= -184.66 and np.exp2(gap, dtype=np.float32) == 0                        # every other key: exp2 = 0 exactly in float32
    assert np.exp2(np.float32(0)) == 1


@pytest.mark.parametrize("case", E.ATTN_CASES, ids=lambda c: c.id)
def test_attention_expectation_is_the_float64_softmax(built, case):
    b = built[case.family]
    named = b["named"]
    qkv = b["qkv"]
    assert np.isnan(qkv[~named]).all() and np.isfinite(qkv[named]).all()
    assert np.array_equal(qkv[named].astype(np.float16).astype(np.float64), qkv[named])         # the float16 kernels see the same numbers
    v = qkv[named][:, 2 * E.HID:]
    assert np.array_equal(v, np.round(v)) and np.abs(v).max() == 8
    ref = E.attn_ref(qkv, b["starts"], b["lengths"])
    exp = b["expected"]
    assert np.isfinite(ref[named]).all() and np.isnan(ref[~named]).all()
    if case.family == "uniform":
        assert E.within_two_roundings(exp[named], ref[named])                                    # 2^-23 |y|: see within_two_roundings
        assert not np.array_equal(exp[named], ref[named].astype(np.float32)), "the two roundings never show: the formula is not tested"
    else:
        assert np.array_equal(ref[named].astype(np.float32), exp[named])
        assert np.array_equal(exp[named] * 2, np.round(exp[named] * 2))
    assert np.array_equal(exp[named].astype(np.float16).astype(np.float32), exp[named]) or case.family == "uniform"
    # the expectation tells the sequences, heads and rows apart: a row written from another key, head or sequence differs
    assert len(np.unique(exp[named], axis=0)) >= (0.95 * named.sum() if case.family == "one-hot" else len(b["lengths"]))


def test_pair_family_averages_two_different_rows(built):
    b = built["pair"]
    qkv = b["qkv"]
    n = 0
    for (s, h), (j, j2) in b["pairs"].items():
        t0 = b["starts"][s]
        k = qkv[t0: t0 + b["lengths"][s], E.HID + h * 64: E.HID + (h + 1) * 64]
        v = qkv[t0: t0 + b["lengths"][s], 2 * E.HID + h * 64: 2 * E.HID + (h + 1) * 64]
        assert j != j2 and np.array_equal(k[j], k[j2]) and not np.array_equal(v[j], v[j2])
        assert sum(np.array_equal(k[j], row) for row in k) == 2
        hits = b["win"][s, h] == j
        assert hits.any()
        n += int(hits.sum())
    assert len(b["pairs"]) == (len(E.NAMED_LENS) - 1) * E.H and n > 1000


def test_attention_layout_and_strips(built):
    from fusion_amd import ops
    for b in built.values():
        assert sorted(b["lengths"]) == list(E.NAMED_LENS) and b["lengths"] != list(E.NAMED_LENS)
        ends = [t0 + L for t0, L in zip(b["starts"], b["lengths"])]
        assert [g[0] for g in b["ghosts"]] == ends and all(1 <= g[1] <= 17 for g in b["ghosts"])
        assert b["starts"][1:] == [a + n for a, n in b["ghosts"][:-1]] and sum(b["ghosts"][-1]) == b["T"]     # a ghost between any two, and at the end
        assert b["T"] < 5000
        strips, _ = ops.attn_strips(b["lengths"], cu_rows=np.asarray(b["starts"]))
        assert strips.dtype == np.int32 and np.array_equal(strips, E.strips_of(b["lengths"], b["starts"]))
        rows = {int(t0) + q for t0, L, q0, _ in strips for q in range(q0, min(q0 + 32, L))}
        assert rows == set(np.flatnonzero(b["named"]))                                          # the table names the named rows, and only them


def test_attention_branch_table_is_covered(built):
    hit = set()
    for c in E.ATTN_CASES:
        hit |= E.attn_branches_of(c, built[c.family])
    assert set(E.ATTN_BRANCHES) <= hit, sorted(map(str, set(E.ATTN_BRANCHES) - hit))
    one = E.attn_branches_of(E.ATTN_CASES[0], built["one-hot"])
    assert {k for k in E.ATTN_BRANCHES if k[0] in ("pos", "tile", "alpha", "substrip", "strip")} <= one
    assert {("pair", "same-tile"), ("pair", "cross-tile")} <= E.attn_branches_of(E.ATTN_CASES[1], built["pair"])
    for c in E.ATTN_CASES:      # every family sees every remainder and both `second` states
        assert {k for k in E.ATTN_BRANCHES if k[0] in ("rem", "second", "ghost")} <= E.attn_branches_of(c, built[c.family])


def test_attn_strips_refuses_lengths_the_kernels_cannot_address():
    from fusion_amd import ops
    assert ops.ATTN_MAX_SEQ == E.MAX_SEQ == 16384
    strips, cu = ops.attn_strips([16384, 0, 5])
    assert len(strips) == 512 + 1 and cu.tolist() == [0, 16384, 16384, 16389]
    for bad in ([16385], [3, 16385, 1], [-1], [4, -2, 4], [2 ** 31]):
        with pytest.raises(ValueError, match="attn_strips"):
            ops.attn_strips(bad)
    assert ops.attn_strips([])[0].shape == (0, 4)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
def test_layernorm_widths_land_on_their_edges():
    assert [E.ln_vpl(d) for d in (1024, 1028)] == [4, 16]                               # 1028: the first width of the 16-slot instantiation
    assert E.ln_live_float4(4096) == [16, 16] and E.ln_live_float4(4092) == [16, 15]     # the cap: every slot of every lane live
    assert E.ln_live_float4(1024) == [4, 4] and E.ln_live_float4(1020) == [4, 3] and E.ln_live_float4(1028) == [5, 4]
    assert E.ln_live_float4(252) == [1, 0] and E.ln_live_float4(256) == [1, 1] and E.ln_live_float4(260) == [2, 1] and E.ln_live_float4(4) == [1, 0]
    inside = [d for d in E.LN_WIDTHS if (d // 2) % 4]
    assert inside == [4, 252, 260, 1020, 1028, 4092]                                       # the sign changes inside a float4
    assert all(d > E.LN_MAX_D or d % 4 for d in E.LN_REFUSED) and max(E.LN_WIDTHS) == E.LN_MAX_D
    assert set(E.LN_ROWS) == {1, 3, 4, 5}                                               # one workgroup takes four rows


@pytest.mark.parametrize("d", E.LN_WIDTHS)
def test_layernorm_expectation_is_float64_layer_norm(d):
    gamma, beta = E.ln_params(d)
    kinds = set()
    for eps in (1e-5, 1e-12):
        for rows in E.LN_ROWS:
            for residual in (False, True):
                x, res, target, m_a = E.ln_exact_rows(d, rows, residual)
                kinds |= set(m_a)
                total = x.astype(np.float64) + (0 if res is None else res.astype(np.float64))
                assert np.array_equal(total, target)                                     # x + res is exact ...
                assert np.array_equal(x.astype(np.float16).astype(np.float32), x)        # ... and x is exact in float16 (the x16 kernel)
                for (m, a), row in zip(m_a, target):
                    assert row.mean() == m and ((row - m) ** 2).mean() == a * a and (a == 0 or d == 4 or len(set(row)) == 2)
                exp = E.ln_expected(m_a, d, gamma, beta, eps)
                ref = E.ln_ref64(target, gamma, beta, eps)
                assert E.within_one_ulp(exp, ref), (d, rows, residual, eps)
                assert np.all((np.abs(exp) >= 2) & (np.abs(exp) < 4))
                for (m, a), row in zip(m_a, exp):
                    if a == 0:
                        assert np.array_equal(row, beta)
    assert kinds == set(E.LN_KINDS)


@pytest.mark.parametrize("d", E.LN_WIDTHS)
def test_embedding_tables_sum_to_exact_rows(d):
    word, pos, type0, m_a_of = E.embed_exact_tables(d)
    V, P = word.shape[0], pos.shape[0]
    gamma, beta = E.ln_params(d)
    seen = set()
    for rows, (ids, pids) in E.EMBED_IDS.items():
        assert len(ids) == len(pids) == rows and V - 1 in ids and P - 1 in pids and max(ids) < V and max(pids) < P
        seen |= {len(set(ids)) < rows or len(set(pids)) < rows}
        t32 = (word[ids] + type0) + pos[pids]                                            # the kernel's order, in float32
        t64 = word[ids].astype(np.float64) + type0.astype(np.float64) + pos[pids].astype(np.float64)
        assert np.array_equal(t32.astype(np.float64), t64)
        m_a = m_a_of(ids, pids)
        assert np.array_equal(t64, np.stack([m + a * E.ln_sign(d) for m, a in m_a]))
        exp = E.ln_expected(m_a, d, gamma, beta, 1e-5)
        ref = E.ln_ref64(t64, gamma, beta, 1e-5)
        assert E.within_one_ulp(exp, ref)
    assert True in seen
    amps = {a for rows, (ids, pids) in E.EMBED_IDS.items() for _, a in m_a_of(ids, pids)}
    assert 0.0 in amps and len(amps) >= 4


# ---- GELU --------------------------------------------------------------------------------------------------------------------
def test_gelu_sizes_take_a_second_ragged_step():
    for n, lap, vec, period in ((E.GELU_N_F32, E.GELU_LAP_F32, 4, E.GELU_PERIOD_F32), (E.GELU_N_F16, E.GELU_LAP_F16, 8, E.GELU_PERIOD_F16)):
        assert n % vec == 0 and n == lap + vec * 37
        blocks, steps, last = E.gelu_laps(n // vec)
        assert (blocks, steps, last) == (256 * 32, 2, 37)                                # the second step: 37 lanes of one wave
        assert period % 2 == 1 and n % period and n // period > 2000
    assert E.gelu_laps(1234 * 3072 // 4)[1] == 1                                         # the parity suite's largest tensor: one step
    assert E.gelu_laps(37000 * 3072 // 4)[1] == 14
    assert len(E.gelu_pattern_f32()) == E.GELU_PERIOD_F32 and len(E.gelu_pattern_f16()) == E.GELU_PERIOD_F16
    assert len(E.gelu_grid_f32()) % 4 == 0 and len(E.gelu_grid_f16()) == 65536


def test_gelu_reference_and_special_values():
    x = E.gelu_grid_f32()
    ref = E.gelu_ref64(x)
    assert np.isnan(ref[np.isnan(x)]).all() and np.isnan(ref[np.isneginf(x)]).all() and np.isposinf(ref[np.isposinf(x)]).all()
    assert np.array_equal(np.isnan(ref), np.isnan(x) | np.isneginf(x))
    assert not ref[x == 0].any() and not ref[(x < -40) & np.isfinite(x)].any()           # 1 + erf underflows to 0: a zero of either sign
    pts = np.array([-3.0, -1.0, -0.5, 0.5, 1.0, 3.0])
    known = np.array([-0.00404969409489, -0.158655253931, -0.154268769363, 0.345731230637, 0.841344746069, 2.99595030591])
    assert np.allclose(E.gelu_ref64(pts), known, rtol=1e-11, atol=0)
    for v in (0.0, 2.0 ** -149, 1e-30, 5.5, 1e30, float(np.finfo(np.float32).max)):
        assert np.float32(v) in x and np.float32(-v) in x
    assert (np.abs(x) <= 8).sum() >= 4096 and np.isposinf(x).any() and np.isneginf(x).any()
    sub = E.gelu_subnormal(x, ref)
    units, mask = E.gelu_units(ref.astype(np.float32), x, ref)
    assert 0 < sub.sum() <= 12 and np.all(np.abs(x[sub]) < 2.0 ** -125) and not (sub & mask).any()
    assert units.max() <= 0.5 / 0.5 and mask.sum() > 4096                                # the correctly rounded result: half an ulp of y <= one unit
    x16 = E.gelu_grid_f16()
    r16 = E.gelu_ref64(x16.astype(np.float64))
    assert np.isfinite(r16[np.isfinite(x16) | np.isposinf(x16)]).sum() == np.isfinite(x16).sum() and not E.gelu_subnormal(x16, r16).any()
    assert np.array_equal(E.f16_half_spacing(np.array([0.0, 1.0, 1.5, 2.0, 2.0 ** -24, 65504.0])),
                          np.array([2.0 ** -25, 2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25, 2.0 ** 4]))


# ---- segment reductions ------------------------------------------------------------------------------------------------------
def test_segment_shapes_land_on_their_paths():
    plans = {s: E.seg_plan(*s) for s in E.SEG_SHAPES}
    assert plans[770, 770] == (False, 4, 2) and plans[1021, 1021] == (False, 4, 253)     # the scalar path, four 256-column slabs
    assert plans[1024, 1024] == (True, 1, 1024) and plans[1028, 1028] == (True, 2, 4) and plans[2052, 2052] == (True, 3, 4)
    assert plans[768, 769] == (False, 3, 256)                                            # an unaligned row pitch forces the scalar path
    assert E.SEG_LENS == (3, 0, 64, 1, 17, 0)


@pytest.mark.parametrize("d,ldx", E.SEG_SHAPES)
def test_segment_mean_expectation_is_the_float64_mean(d, ldx):
    buf, cu = E.seg_inputs(d, ldx)
    x = buf[:, :d]
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() == 8 and cu.tolist() == [0, 3, 3, 67, 68, 85, 85]
    exp, ref = E.seg_mean_expected(x, cu), E.seg_mean_ref64(x, cu)
    assert E.within_two_roundings(exp, ref)
    assert not exp[1].any() and not np.signbit(exp[1]).any() and not np.signbit(exp[5]).any()
    assert np.array_equal(exp[3], x[67]) and np.array_equal(exp[2].astype(np.float64), ref[2])     # L = 1 and L = 64: exact
    assert not np.array_equal(exp[0].astype(np.float64), ref[0])                                  # L = 3: the rounding of 1 / 3 shows
    s = E.seg_splade_ref64(x, cu)
    assert s.min() == 0 and np.isclose(s.max(), np.log1p(8.0)) and not s[1].any()
