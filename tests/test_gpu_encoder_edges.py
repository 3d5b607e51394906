"""The kernels of csrc/encoder.hip at their tile, lane, lap and slab edges, bit for bit wherever the inputs leave no rounding.

Attention (three kernels x three families, one launch each): Hadamard codes make every softmax weight exactly 1 or 0 and V holds small
integers (encoder_cases.py), so every named row must equal the expectation bit for bit; the rows of unnamed NaN sequences between the
named ones, the NaN padding columns of qkv and the sentinel columns / rows of `out` show a read or a store outside the sequence.
LayerNorm, x16 LayerNorm and embed-LayerNorm: constant and balanced rows at every width edge through strided views, bit for bit.
GELU: the second grid-stride step on a periodic input, and every special value against float64 at a bar measured from torch's own
float32 GELU on the same points.  Segment mean on the scalar path and on the later column slabs, bit for bit on integer rows.
test_encoder_cases_cpu.py proves the expectations against float64 and that the cases land on the edges they name."""
import numpy as np
import pytest
import torch

import encoder_cases as E

pytestmark = pytest.mark.gpu

SENTINEL = -1234.0          # exact in float16; no expectation comes near it


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])


def wide(rows, d, pad, dtype, fill=SENTINEL):
    """-> (buffer [rows, d + pad] filled with `fill`, its [:, :d] view)."""
    buf = torch.full((rows, d + pad), fill, dtype=dtype, device="cuda")
    return buf, buf[:, :d]


def assert_bits(got, exp, what):
    bad = np.argwhere(bits(got) != bits(exp))
    assert len(bad) == 0, (what, len(bad), [(int(r), int(c), float(got[r, c]), float(exp[r, c])) for r, c in bad[:8]])


def is_refusal(e):
    from fusion_amd import _lib
    return isinstance(e, ValueError) or (isinstance(e, _lib.FusionHipError) and e.status == _lib.FZ_ERR_UNSUPPORTED)


# ---- A. attention ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn_built():
    return {c.family: c.build() for c in E.ATTN_CASES}


@pytest.mark.parametrize("kernel", ["f32", "f16", "f16_amp"])
@pytest.mark.parametrize("case", E.ATTN_CASES, ids=lambda c: c.id)
def test_attention_exact_inputs(ops, attn_built, case, kernel):
    """fz_attn_varlen_f32 / _f16 / _f16_amp: every named row equals the expectation bit for bit (the float16 outputs: the float32
    expectation rounded once more); ghost rows and padding columns of `out` keep their sentinel; no NaN reaches a named row."""
    b = attn_built[case.family]
    T, W = b["T"], 3 * E.HID
    dt = torch.float32 if kernel == "f32" else torch.float16
    qbuf, qkv = wide(T, W, E.PAD_COLS, dt, float("nan"))
    qkv.copy_(dev(b["qkv"]).to(dt))
    obuf, out = wide(T, E.HID, E.PAD_COLS, dt)
    before = obuf.cpu().numpy()
    strips, _ = ops.attn_strips(b["lengths"], cu_rows=np.asarray(b["starts"]))
    assert len(strips) == sum(-(-L // 32) for L in b["lengths"])
    st = dev(strips)
    assert qkv.stride(0) == W + E.PAD_COLS and out.stride(0) == E.HID + E.PAD_COLS and torch.isnan(qbuf[:, W:]).all()
    if kernel == "f32":
        ops.attn_varlen(qkv, st, E.H, out=out)
    else:
        ops.attn_varlen_f16(qkv, st, E.H, out, amp=kernel == "f16_amp")
    torch.cuda.synchronize()
    got = obuf.cpu().numpy()
    named = b["named"]
    exp = b["expected"] if kernel == "f32" else b["expected"].astype(np.float16)
    assert np.array_equal(bits(got[~named]), bits(before[~named])), "a row that the strip table does not name was written"
    assert np.array_equal(bits(got[:, E.HID:]), bits(before[:, E.HID:])), "a padding column of out was written"
    assert not np.isnan(got[named, : E.HID]).any(), "NaN in a named row: a key or value row outside the sequence was read"
    assert_bits(got[named, : E.HID], exp[named], (case.id, kernel))


# ---- B. LayerNorm ------------------------------------------------------------------------------------------------------------
def _check_ln(got_buf, d, exp, what):
    got = got_buf.cpu().numpy()
    assert np.isfinite(got[:, :d].astype(np.float32)).all(), what
    assert_bits(got[:, :d], exp, what)
    assert np.array_equal(got[:, d:], np.full_like(got[:, d:], SENTINEL)), (what, "a padding column was written")


@pytest.mark.parametrize("d", E.LN_WIDTHS)
def test_layernorm_exact_rows(ops, d):
    """fz_add_layernorm_f32 and fz_add_layernorm_x16 on constant rows (-> beta) and balanced rows (-> the float32 formula of
    encoder_cases.ln_expected), with and without a residual, 1 / 3 / 4 / 5 rows, every operand a column slice of a wider buffer of
    its own width.  out16 == out.half(), and the x16 kernel equals the float32 kernel on the same values."""
    gamma, beta = E.ln_params(d)
    g, b = dev(gamma), dev(beta)
    for rows in E.LN_ROWS:
        for residual in (False, True):
            for eps in ((1e-5, 1e-12) if rows == 5 else (1e-5,)):
                x_np, r_np, _, m_a = E.ln_exact_rows(d, rows, residual)
                exp = E.ln_expected(m_a, d, gamma, beta, eps)
                what = (d, rows, residual, eps)
                _, x = wide(rows, d, 4, torch.float32, float("nan"))
                x.copy_(dev(x_np))
                res = None
                if residual:
                    _, res = wide(rows, d, 8, torch.float32, float("nan"))
                    res.copy_(dev(r_np))
                obuf, out = wide(rows, d, 12, torch.float32)
                assert ops.add_layernorm(x, res, g, b, eps, out=out) is out
                _check_ln(obuf, d, exp, ("f32",) + what)
                _, x16 = wide(rows, d, 20, torch.float16, float("nan"))
                x16.copy_(dev(x_np).half())
                obuf2, out2 = wide(rows, d, 12, torch.float32)
                hbuf, out16 = wide(rows, d, 16, torch.float16)
                ops.add_layernorm_x16(x16, res, g, b, eps, out=out2, out16=out16)
                _check_ln(obuf2, d, exp, ("x16",) + what)
                _check_ln(hbuf, d, exp.astype(np.float16), ("x16 out16",) + what)
                assert torch.equal(out16, out2.half())
                assert torch.equal(ops.add_layernorm_x16(x16, res, g, b, eps), ops.add_layernorm(x16.float(), res, g, b, eps))


@pytest.mark.parametrize("d", E.LN_WIDTHS)
def test_embed_layernorm_exact_rows(ops, d):
    """fz_embed_layernorm_f32 on integer tables whose sums are constant and balanced rows; ids V - 1 and P - 1, repeated ids; rows of
    the out buffer past the batch and its padding columns keep their sentinel."""
    word, pos, type0, m_a_of = E.embed_exact_tables(d)
    gamma, beta = E.ln_params(d)
    w, p, t, g, b = (dev(a) for a in (word, pos, type0, gamma, beta))
    for rows, (ids, pids) in E.EMBED_IDS.items():
        exp = E.ln_expected(m_a_of(ids, pids), d, gamma, beta, 1e-5)
        obuf, out = wide(rows + 2, d, 12, torch.float32)
        assert ops.embed_layernorm(w, p, t, dev(np.array(ids, dtype=np.int64)), dev(np.array(pids, dtype=np.int64)), g, b, 1e-5, out=out) is out
        _check_ln(obuf[:rows], d, exp, ("embed", d, rows))
        assert (obuf[rows:] == SENTINEL).all(), ("embed", d, rows, "a row past the batch was written")


@pytest.mark.parametrize("d", E.LN_WIDTHS)
def test_layernorm_random_rows(ops, d):
    """The parity suite's bar (float64 layer_norm, 5e-6 * max(1, |ref|max)) at every width edge, through the strided views."""
    gen = torch.Generator(device="cuda").manual_seed(d)
    rows = 5
    rn = lambda *s: torch.randn(s, generator=gen, device="cuda")
    gamma, beta = rn(d), rn(d)
    _, x = wide(rows, d, 4, torch.float32)
    _, res = wide(rows, d, 8, torch.float32)
    x.copy_(rn(rows, d) * 3 + 1)
    res.copy_(rn(rows, d))
    _, x16 = wide(rows, d, 20, torch.float16)
    x16.copy_(x.half())
    V, P = 9, 6
    word, pos, type0 = rn(V, d), rn(P, d), rn(d)
    ids, pids = dev(np.array([8, 0, 3, 8, 5], dtype=np.int64)), dev(np.array([5, 5, 0, 2, 1], dtype=np.int64))

    def ln64(t):
        return torch.nn.functional.layer_norm(t, (d,), gamma.double(), beta.double(), 1e-5)

    def check(out, ref, what):
        err, bar = (out.double() - ref).abs().max().item(), 5e-6 * max(1.0, ref.abs().max().item())
        print(f"{what} d={d}: max |out - ref| = {err:.3e} (bar {bar:.1e})")
        assert err <= bar, what

    for r in (None, res):
        add = 0 if r is None else r.double()
        _, out = wide(rows, d, 12, torch.float32)
        check(ops.add_layernorm(x, r, gamma, beta, 1e-5, out=out), ln64(x.double() + add), "add_layernorm")
        check(ops.add_layernorm_x16(x16, r, gamma, beta, 1e-5), ln64(x16.double() + add), "add_layernorm_x16")
    check(ops.embed_layernorm(word, pos, type0, ids, pids, gamma, beta, 1e-5), ln64(word[ids].double() + type0.double() + pos[pids].double()), "embed_layernorm")


@pytest.mark.parametrize("d", E.LN_REFUSED)
def test_layernorm_refusals_leave_the_output_untouched(ops, d):
    """d = 4100 (above the 4096 cap) and d = 6 (d % 4): every LayerNorm entry point refuses before any launch."""
    rows = 3
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    out, out16 = torch.full((rows, d), SENTINEL, device="cuda"), torch.full((rows, d), SENTINEL, dtype=torch.float16, device="cuda")
    ids = torch.zeros(rows, dtype=torch.int64, device="cuda")
    calls = {"add_layernorm": lambda: ops.add_layernorm(z(rows, d), z(rows, d), z(d), z(d), 1e-5, out=out),
             "add_layernorm_x16": lambda: ops.add_layernorm_x16(z(rows, d, dt=torch.float16), None, z(d), z(d), 1e-5, out=out, out16=out16),
             "embed_layernorm": lambda: ops.embed_layernorm(z(2, d), z(2, d), z(d), ids, ids, z(d), z(d), 1e-5, out=out)}
    for what, call in calls.items():
        with pytest.raises(Exception) as ei:
            call()
        assert is_refusal(ei.value), (what, repr(ei.value))
        torch.cuda.synchronize()
        assert (out == SENTINEL).all() and (out16 == SENTINEL).all(), (what, "a refused call wrote to the output")


# ---- C. GELU -----------------------------------------------------------------------------------------------------------------
def _gelu_value_check(x_np, y_np, half):
    """The bar of the value checks.  K_torch = the largest error of torch.nn.functional.gelu (float32, on the device, same points)
    against the float64 expression, in units of 2^-24 |x|; the kernel is held to max(2, 2 K_torch) units -- two erff implementations of
    one design accuracy, and the outer expression's two roundings -- plus, for the float16 kernel, half a float16 spacing of the
    reference (floor 2^-25).  A float32 result below 2^-126 is quantised to 2^-149 whatever |x| is: those few points (|x| < 2^-125)
    are held to one subnormal spacing, the two roundings of 0.5 x (1 + erf), and do not enter K_torch.  -> (K_torch, the kernel's
    worst value in the same units)."""
    x64 = x_np.astype(np.float64)
    ref = E.gelu_ref64(x64)
    t_np = torch.nn.functional.gelu(dev(x_np).float()).cpu().numpy()
    k_units, mask = E.gelu_units(t_np, x64, ref)
    K = float(k_units.max())
    y64 = y_np.astype(np.float64)
    nan = np.isnan(ref)
    assert nan.sum() >= 2 and np.isnan(y64[nan]).all() and not np.isnan(y64[~nan]).any()      # NaN exactly where the expression is NaN: NaN, -inf
    assert np.isposinf(y64[np.isposinf(x64)]).all() and np.isposinf(x64).any()
    zero = ~nan & (ref == 0)
    assert zero.any() and not y64[zero].any()                                                  # a zero of either sign: 0.5 * -9 * (1 + -1) is -0.0 here and there
    allowed = max(2.0, 2.0 * K) * 2.0 ** -24 * np.abs(x64[mask])
    if half:
        allowed = allowed + E.f16_half_spacing(ref[mask])
    err = np.abs(y64[mask] - ref[mask])
    own = float((np.maximum(err - (E.f16_half_spacing(ref[mask]) if half else 0), 0) / (2.0 ** -24 * np.abs(x64[mask]))).max())
    print(f"gelu {'float16' if half else 'float32'}: K_torch = {K:.3f}, kernel = {own:.3f} units of 2^-24 |x| over {int(mask.sum())} points")
    worst = int(np.argmax(err - allowed))
    assert np.all(err <= allowed), (K, own, float(x64[mask][worst]), float(y64[mask][worst]), float(ref[mask][worst]))
    sub = E.gelu_subnormal(x64, ref)
    assert np.all(np.abs(y64[sub] - ref[sub]) <= 2.0 ** -149), (x_np[sub], y_np[sub])
    return K, own


def test_gelu_f32_values(ops):
    """The special-value grid and 4096 points over [-8, 8].  Measured on the MI355X (ROCm 7.2): K_torch = 1.703 and the kernel's own
    worst point 1.703 units of 2^-24 |x| over 4190 points (the two agree to every digit printed: the bar is 3.4 units)."""
    x = E.gelu_grid_f32()
    y = ops.gelu_(dev(x)).cpu().numpy()
    _gelu_value_check(x, y, half=False)


def test_gelu_f16_every_bit_pattern(ops):
    """All 65536 float16 values in one launch.  Measured on the MI355X (ROCm 7.2): K_torch = 1.759 (torch's float32 GELU of the same
    values), and the kernel's worst point lies 0.399 units of 2^-24 |x| beyond half a float16 spacing of the reference (63486 points)."""
    x = E.gelu_grid_f16()
    y = ops.gelu_f16_(dev(x)).cpu().numpy()
    _gelu_value_check(x, y, half=True)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_gelu_second_lap_is_periodic(ops, half):
    """One pass of the capped grid (256 * 32 workgroups) plus 37 lanes: the grid-stride loop takes its second, ragged step.  The input
    is one odd-length pattern tiled, so the output must repeat bit for bit, and its first period must pass the value check."""
    n, period, pattern = (E.GELU_N_F16, E.GELU_PERIOD_F16, E.gelu_pattern_f16()) if half else (E.GELU_N_F32, E.GELU_PERIOD_F32, E.gelu_pattern_f32())
    reps = -(-n // period)
    p = dev(pattern)
    x = p.repeat(reps)[:n].clone()
    y = (ops.gelu_f16_ if half else ops.gelu_)(x)
    assert y.numel() == n
    torch.cuda.synchronize()
    yb = y.view(torch.int16 if half else torch.int32)
    first = yb[:period]
    whole = (n // period) * period
    same = (yb[:whole].view(-1, period) == first).all(dim=1)
    bad = torch.nonzero(~same).flatten()[:4].tolist()
    assert not bad, ("periods that differ from the first", bad, [int(torch.nonzero(yb[k * period: (k + 1) * period] != first)[0]) for k in bad])
    assert torch.equal(yb[whole:], first[: n - whole]), "the ragged tail differs"
    _gelu_value_check(pattern, y[:period].cpu().numpy(), half)


# ---- D. segment reductions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ldx", E.SEG_SHAPES)
def test_segment_mean_exact_and_splade_max(ops, d, ldx):
    """fz_segment_mean_f32 on the scalar path (d % 4, or an unaligned row pitch) and on the second and third column slabs of the vector
    path: integer rows, so float32(sum) * (1 / L) bit for bit and +0.0 for an empty sequence.  fz_segment_splade_max_f32 at the same
    widths and strides: the parity suite's 1e-6 against log1p(relu(x)).amax(0)."""
    buf, cu = E.seg_inputs(d, ldx)
    x = dev(buf)[:, :d]
    assert x.stride(0) == ldx
    got = ops.segment_mean(x, dev(cu)).cpu().numpy()
    assert_bits(got, E.seg_mean_expected(buf[:, :d], cu), ("segment_mean", d, ldx))
    scaled = buf * np.float32(0.37) - np.float32(1.0)              # off the integers, both signs
    got = ops.segment_splade_max(dev(scaled)[:, :d], dev(cu)).cpu().numpy()
    err = float(np.abs(got - E.seg_splade_ref64(scaled[:, :d], cu)).max())
    print(f"segment_splade_max d={d} ldx={ldx}: max |got - ref| = {err:.3e} (bar 1e-6)")
    assert err <= 1e-6
