"""Inputs, references and case tables of the exact encoder-kernel tests (test_gpu_encoder_edges.py on the GPU, test_encoder_cases_cpu.py
without one) for csrc/encoder.hip.  numpy only.  Not collected by pytest.

Attention.  The 128 codes u_c are the rows of the 64 x 64 Sylvester Hadamard matrix and their negatives, times 4: exact in float16,
<u_c, u_c> = 1024, any other pair 0 or -1024.  With scale 1/8 the kernel's base-2 constant is c = float32(0.125f * 1.4426950408889634f), and
1024 c is exact in float32: a key that carries the query's code gets exp2(0) = 1, every other key lies at least 184.66 below it in the base-2
domain and gets exp2 = 0 exactly.  V holds integers in [-8, 8], so every weighted sum is exact in any order, in float32 and through float16
operands alike: on these inputs none of the three kernels has a rounding to hide behind, and the rows around the named sequences
(unnamed "ghost" sequences, padding columns) are NaN, which a read past the sequence turns into a NaN in the output (0 * NaN).

LayerNorm.  A row m + a * (+1 on the first half, -1 on the second) has mean m and variance a * a exactly, in any summation order;
a = 0 (a constant row) normalises to beta.  GELU and the segment reductions: see the sections below."""
import dataclasses
import math

import numpy as np

# ---- attention ---------------------------------------------------------------------------------------------------------------
H, HD = 3, 64
HID = H * HD
PAD_COLS = 8                                                 # the buffers are this much wider than the views handed to ops
NAMED_LENS = tuple(range(1, 81)) + (127, 128)
GHOST_LENS = tuple(range(1, 18))
SCALE = 0.125
SCALE_LOG2E = np.float32(0.125) * np.float32(1.4426950408889634)    # fz_attn_varlen_*: scale * 1.4426950408889634f
TILE, STRIP = 16, 32                                         # keys per tile; queries per strip (two sub-strips of 16)
MAX_SEQ = 16384                                              # include/fusion_hip.h: 32-bit in-sequence byte offsets
FAMILIES = ("one-hot", "pair", "uniform")


def hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


CODES = np.concatenate([4.0 * hadamard(HD), -4.0 * hadamard(HD)])     # [128, 64]


def strips_of(lengths, starts):
    """ops.attn_strips restated: one (first row, L, q0, 0) entry per 32 queries, longest sequences first (stable)."""
    order = sorted(range(len(lengths)), key=lambda b: -lengths[b])
    return np.array([(starts[b], lengths[b], q0, 0) for b in order for q0 in range(0, lengths[b], STRIP)], dtype=np.int32).reshape(-1, 4)


@dataclasses.dataclass(frozen=True)
class AttnCase:
    family: str
    seed: int = 0

    @property
    def id(self):
        return self.family

    def build(self):
        """-> dict: qkv [T, 3 * HID] float64 (NaN in every ghost row), expected [T, HID] float32 (named rows), starts / lengths of the
        named sequences in memory order, ghosts [(first row, length)], named [T] bool, and per (sequence, head) the key each query
        attends (`win`, -1 = all of them) and the pair of keys that share a code (`pairs`)."""
        rng = np.random.default_rng(1000 * FAMILIES.index(self.family) + self.seed)
        lengths = [int(x) for x in rng.permutation(NAMED_LENS)]
        glens = [GHOST_LENS[(i + self.seed) % len(GHOST_LENS)] for i in range(len(lengths))]
        starts, ghosts, row = [], [], 0
        for L, g in zip(lengths, glens):
            starts.append(row)
            ghosts.append((row + L, g))
            row += L + g
        T = row
        qkv = np.full((T, 3 * HID), np.nan)
        exp = np.zeros((T, HID), dtype=np.float32)
        named = np.zeros(T, dtype=bool)
        win, pairs = {}, {}
        for b, (t0, L) in enumerate(zip(starts, lengths)):
            named[t0: t0 + L] = True
            for h in range(H):
                v = rng.integers(-8, 9, (L, HD)).astype(np.float64)
                code = rng.permutation(128)[:L]
                target = np.full(L, -1)
                if self.family == "uniform":
                    code = rng.integers(0, 128, L)
                    q = np.zeros((L, HD))
                    e = (v.sum(axis=0).astype(np.float32) * (np.float32(1) / np.float32(L))).astype(np.float32)
                    e = np.broadcast_to(e, (L, HD))
                else:
                    if self.family == "pair" and L >= 2:
                        j, j2 = (int(x) for x in rng.choice(L, 2, replace=False))
                        same = [x for x in range(j - j % TILE, min(j - j % TILE + TILE, L)) if x != j]
                        if b % 2 == 0 and same:                               # every other sequence: the two keys in one tile
                            j2 = int(rng.choice(same))
                        code[j2] = code[j]
                        pairs[b, h] = (j, j2)
                        others = [x for x in range(L) if x not in (j, j2)]
                        target = np.full(L, j)                                # about half the queries carry the pair's code ...
                        if others:
                            pick = rng.random(L) >= 0.5                       # ... the others that of a single key
                            target[pick] = rng.choice(others, int(pick.sum()))
                        target[int(rng.integers(0, L))] = j
                        e = np.where((target == j)[:, None], (v[j] + v[j2]) * 0.5, v[target])
                    else:
                        target = rng.permutation(L)
                        e = v[target]
                    q = CODES[code[target]]
                win[b, h] = target
                sl = slice(t0, t0 + L)
                qkv[sl, h * HD: (h + 1) * HD] = q
                qkv[sl, HID + h * HD: HID + (h + 1) * HD] = CODES[code]
                qkv[sl, 2 * HID + h * HD: 2 * HID + (h + 1) * HD] = v
                exp[sl, h * HD: (h + 1) * HD] = e
        return dict(qkv=qkv, expected=exp, starts=starts, lengths=lengths, ghosts=ghosts, named=named, win=win, pairs=pairs, T=T)


ATTN_CASES = tuple(AttnCase(f) for f in FAMILIES)


def attn_ref(qkv, starts, lengths, heads=H, scale=SCALE):
    """softmax(q k^T scale) v per named sequence and head in float64; rows outside the named sequences stay NaN."""
    hid = heads * HD
    out = np.full((qkv.shape[0], hid), np.nan)
    for t0, L in zip(starts, lengths):
        for h in range(heads):
            q, k, v = (qkv[t0: t0 + L, i * hid + h * HD: i * hid + (h + 1) * HD] for i in range(3))
            s = (q @ k.T) * scale
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[t0: t0 + L, h * HD: (h + 1) * HD] = (p @ v) / p.sum(axis=1, keepdims=True)
    return out


ATTN_BRANCHES = {
    **{("pos", p): "one-hot: the attended key is key p of its 16-key tile" for p in range(TILE)},
    **{("tile", k): "one-hot: the attended key's tile" for k in ("first", "middle", "last-partial")},
    ("alpha", 0): "one-hot: tiles with a lower maximum came first (the running sums are rescaled by exp2(-184.66) = 0)",
    ("alpha", 1): "one-hot: tiles with a lower maximum follow (alpha = 1, p = 0)",
    **{("substrip", u): "one-hot: the query's 16-query sub-strip of its strip" for u in (0, 1)},
    ("strip", "q0>0"): "one-hot: a query of a later strip of its sequence",
    **{("pair", k): "pair: the two keys of one code" for k in ("same-tile", "cross-tile")},
    **{("rem", r): "L % 16" for r in range(TILE)},
    **{("second", s): "the strip's second 16 queries exist" for s in (True, False)},
    **{("ghost", g): "an unnamed NaN sequence of g rows behind a named one" for g in GHOST_LENS},
}


def attn_branches_of(case, built=None):
    b = built or case.build()
    hit = {("ghost", g) for _, g in b["ghosts"]}
    for L in b["lengths"]:
        hit.add(("rem", L % TILE))
        hit |= {("second", q0 + TILE < L) for q0 in range(0, L, STRIP)}
    if case.family == "one-hot":
        for (s, _), target in b["win"].items():
            L = b["lengths"][s]
            nt = -(-L // TILE)
            for i, j in enumerate(target):
                t = j // TILE
                hit |= {("pos", j % TILE), ("substrip", (i % STRIP) // TILE)}
                if i >= STRIP:
                    hit.add(("strip", "q0>0"))
                if t == 0:
                    hit.add(("tile", "first"))
                elif t < nt - 1:
                    hit.add(("tile", "middle"))
                elif L % TILE:
                    hit.add(("tile", "last-partial"))
                if t > 0:
                    hit.add(("alpha", 0))
                if t < nt - 1:
                    hit.add(("alpha", 1))
    if case.family == "pair":
        hit |= {("pair", "same-tile" if j // TILE == j2 // TILE else "cross-tile") for j, j2 in b["pairs"].values()}
    return hit


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (4, 252, 256, 260, 768, 1020, 1024, 1028, 2048, 4092, 4096)
LN_ROWS = (1, 3, 4, 5)
LN_REFUSED = (4100, 6)
LN_MAX_D = 4096
# (offset m, amplitude a): the constant row, the balanced rows about 0, and two balanced rows about an offset (a mean that is wrong
# by a factor leaves the rows about 0 alone)
LN_KINDS = ((2.0, 0.0), (0.0, 0.5), (0.0, 1.0), (0.0, 2.0), (3.0, 1.0), (-1.0, 0.5))


def ln_vpl(d):
    """float4 per lane of the instantiation fz_add_layernorm_* / fz_embed_layernorm_f32 launches."""
    return 4 if d <= 1024 else 16


def ln_live_float4(d):
    """How many of a lane's VPL float4 slots hold part of the row, for the first and the last lane."""
    nv = d // 4
    return [sum(i * 64 + lane < nv for i in range(ln_vpl(d))) for lane in (0, 63)]


def ln_sign(d):
    s = np.ones(d)
    s[d // 2:] = -1.0
    return s


def ln_params(d, seed=0):
    """Random gamma and beta of either sign with |gamma| in [0.25, 0.375] and |beta| in [2.5, 3.5]: the result lies in [2, 4), where
    float32 values are 4 * 2^-24 apart, and the float32 formula of ln_expected stays within ONE such step of the float64 layer norm for
    certain -- its product +-a * rstd * gamma (< 0.375) carries at most 4.5 relative roundings of 2^-24 (a * a + eps: 1/2 after the
    square root; sqrt, division, * a, * gamma: 1 each), 1.7 * 2^-24 absolute, and the final sum rounds by at most 2 * 2^-24."""
    rng = np.random.default_rng(7000 + d + seed)
    gamma = (rng.uniform(0.25, 0.375, d) * rng.choice([-1.0, 1.0], d)).astype(np.float32)
    beta = (rng.uniform(2.5, 3.5, d) * rng.choice([-1.0, 1.0], d)).astype(np.float32)
    return gamma, beta


def within_one_ulp(exp32, ref64):
    """|exp - ref| <= the float32 spacing at exp."""
    return np.all(np.abs(exp32.astype(np.float64) - ref64) <= np.spacing(np.abs(exp32)).astype(np.float64))


def within_two_roundings(exp32, ref64):
    """|exp - ref| <= 2^-23 |exp|: one ulp in the relative sense, the bound of two correctly rounded float32 operations (2^-24 each).
    Just below a power of two that is up to 1.5 spacings -- float32(6) * float32(1 / 7) is 1.14 spacings off 6 / 7 -- so the spacing at
    exp is not a bound that the two-rounding formula of a mean can meet."""
    return np.all(np.abs(exp32.astype(np.float64) - ref64) <= 2.0 ** -23 * (1 + 2.0 ** -20) * np.abs(exp32.astype(np.float64)))


def ln_expected(m_a, d, gamma, beta, eps):
    """The kernel's float32 arithmetic on a row m + a * sign: mean m and variance a * a exactly, then
    float32(float32(float32(+-a * rstd) * g) + b) with rstd = 1 / sqrt(float32(a * a) + float32(eps))."""
    out = np.empty((len(m_a), d), dtype=np.float32)
    sign = ln_sign(d).astype(np.float32)
    for r, (_, a) in enumerate(m_a):
        a = np.float32(a)
        rstd = np.float32(1) / np.sqrt(np.float32(a * a) + np.float32(eps), dtype=np.float32)
        out[r] = ((sign * a * rstd).astype(np.float32) * gamma).astype(np.float32) + beta
    return out


def ln_exact_rows(d, rows, residual, seed=0):
    """-> (x, res or None, target, m_a): rows of LN_KINDS in rotation; with a residual, x = target - r and res = r for integers r."""
    rng = np.random.default_rng(100 * d + 10 * rows + residual + seed)
    m_a = [LN_KINDS[(r + rows + seed) % len(LN_KINDS)] for r in range(rows)]
    target = np.stack([m + a * ln_sign(d) for m, a in m_a])
    if not residual:
        return target.astype(np.float32), None, target, m_a
    r = rng.integers(-3, 4, (rows, d)).astype(np.float64)
    return (target - r).astype(np.float32), r.astype(np.float32), target, m_a


def ln_ref64(t, gamma, beta, eps):
    t = np.asarray(t, dtype=np.float64)
    mean = t.mean(axis=1, keepdims=True)
    var = ((t - mean) ** 2).mean(axis=1, keepdims=True)
    return (t - mean) / np.sqrt(var + eps) * gamma.astype(np.float64) + beta.astype(np.float64)


def embed_exact_tables(d, seed=0):
    """word [V, d], pos [P, d], type0 [d] of integers and half-integers whose sum (word[i] + type0) + pos[p] is the row
    (c_i + e_p) + (alpha_i + beta_p) * sign.  -> (word, pos, type0, m_a(ids, pos_ids))."""
    rng = np.random.default_rng(300 + d + seed)
    V, P = 7, 6
    c, alpha = rng.integers(-2, 3, V).astype(np.float64), np.array([0, 0.5, 1, 0, 1.5, 0.5, 0])
    e, bet = rng.integers(-2, 3, P).astype(np.float64), np.array([0, 0.5, 0, 1, 0.5, 0])
    n1, n2 = rng.integers(-3, 4, d).astype(np.float64), rng.integers(-3, 4, d).astype(np.float64)
    s = ln_sign(d)
    word = c[:, None] + alpha[:, None] * s - n1
    pos = e[:, None] + bet[:, None] * s + n2
    type0 = n1 - n2

    def m_a(ids, pos_ids):
        return [(c[i] + e[p], alpha[i] + bet[p]) for i, p in zip(ids, pos_ids)]
    return word.astype(np.float32), pos.astype(np.float32), type0.astype(np.float32), m_a


EMBED_IDS = {1: ([6], [5]), 3: ([6, 0, 6], [5, 5, 1]), 4: ([1, 6, 1, 3], [0, 5, 3, 3]), 5: ([6, 2, 2, 4, 0], [5, 1, 5, 4, 0])}   # V - 1, P - 1, repeats


# ---- GELU --------------------------------------------------------------------------------------------------------------------
GELU_LAP_F32 = 256 * 32 * 256 * 4            # floats one pass of the capped grid covers (fz_gelu_f32)
GELU_LAP_F16 = 256 * 32 * 256 * 8            # halves (fz_gelu_f16)
GELU_N_F32, GELU_PERIOD_F32 = GELU_LAP_F32 + 4 * 37, 4099
GELU_N_F16, GELU_PERIOD_F16 = GELU_LAP_F16 + 8 * 37, 8203
F32_MIN_NORMAL = 2.0 ** -126


def gelu_ref64(x):
    """0.5 x (1 + erf(x / sqrt 2)) in float64 (NaN where the expression is NaN: NaN and -inf)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        erf = np.array([math.erf(t) if not math.isnan(t) else math.nan for t in (x / math.sqrt(2.0)).ravel()]).reshape(x.shape)
        return 0.5 * x * (1.0 + erf)


def gelu_special_f32():
    tiny = np.float32(2.0 ** -149)
    base = np.array([0, tiny, 1e-30, 1e-4, 0.5, 1, 2, 3, 4, 5, 5.5, 6, 8, 10, 40, 1e4, 1e30, np.finfo(np.float32).max], dtype=np.float32)
    base = np.concatenate([base, -base])
    inf = np.float32(np.inf)
    with np.errstate(over="ignore"):        # the neighbour above FLT_MAX is +inf
        pts = np.concatenate([base, np.nextafter(base, inf), np.nextafter(base, -inf), np.array([np.inf, -np.inf, np.nan], dtype=np.float32)])
    return pts.astype(np.float32)


def gelu_grid_f32():
    g = np.concatenate([gelu_special_f32(), np.linspace(-8, 8, 4096).astype(np.float32)])
    return np.concatenate([g, np.zeros(-len(g) % 4, dtype=np.float32)])


def gelu_pattern_f32():
    sp = gelu_special_f32()
    return np.concatenate([sp, np.linspace(-8, 8, GELU_PERIOD_F32 - len(sp)).astype(np.float32)])


def gelu_grid_f16():
    return np.arange(65536, dtype=np.uint16).view(np.float16)


def gelu_pattern_f16():
    tiny = np.float16(2.0 ** -24)
    base = np.array([0, tiny, 1e-4, 0.5, 1, 2, 3, 4, 5, 5.5, 6, 8, 10, 40, 1e4, 65504], dtype=np.float16)
    sp = np.concatenate([base, -base, np.array([np.inf, -np.inf, np.nan], dtype=np.float16)])
    return np.concatenate([sp, np.linspace(-8, 8, GELU_PERIOD_F16 - len(sp)).astype(np.float16)])


def gelu_units(y, x, ref):
    """|y - ref| in units of 2^-24 |x| over the points that are judged this way: finite x != 0 whose reference is a normal float32 (or
    zero).  A subnormal result is quantised to 2^-149 whatever |x| is, so those points are held to one subnormal spacing instead
    (gelu_subnormal); -> (units, mask)."""
    x64, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        mask = np.isfinite(x64) & (x64 != 0) & np.isfinite(ref) & ((np.abs(ref) >= F32_MIN_NORMAL) | (ref == 0))
    units = np.zeros(x64.shape)
    units[mask] = np.abs(np.asarray(y, dtype=np.float64)[mask] - ref[mask]) / (2.0 ** -24 * np.abs(x64[mask]))
    return units, mask


def gelu_subnormal(x, ref):
    with np.errstate(invalid="ignore"):
        return np.isfinite(ref) & (ref != 0) & (np.abs(ref) < F32_MIN_NORMAL)


def f16_half_spacing(ref):
    """Half the float16 spacing at |ref|, with the floor 2^-25 (half the subnormal spacing)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    e = np.where(np.isfinite(e), e, -100.0)
    return np.maximum(2.0 ** (e - 11), 2.0 ** -25)


def gelu_laps(n_vec):
    """(blocks launched, grid-stride steps of the first thread, threads live in the last step) for n_vec float4 / half8 items."""
    blocks = min(-(-n_vec // 256), 256 * 32)
    stride = blocks * 256
    steps = -(-n_vec // stride)
    return blocks, steps, n_vec - (steps - 1) * stride


# ---- segment reductions ------------------------------------------------------------------------------------------------------
SEG_LENS = (3, 0, 64, 1, 17, 0)
SEG_SHAPES = ((770, 770), (1021, 1021), (1024, 1024), (1028, 1028), (2052, 2052), (768, 769))     # (d, ldx)


def seg_plan(d, ldx):
    """launch_segment_reduce restated: (vector path, column slabs, columns of the last slab)."""
    vec = d % 4 == 0 and ldx % 4 == 0
    per = 1024 if vec else 256
    slabs = -(-d // per)
    return vec, slabs, d - (slabs - 1) * per


def seg_inputs(d, ldx, seed=0):
    rng = np.random.default_rng(900 + d + ldx + seed)
    T = sum(SEG_LENS)
    buf = rng.integers(-8, 9, (T, ldx)).astype(np.float32)
    cu = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int32)
    return buf, cu


def seg_mean_expected(x, cu):
    """float32(sum) * (float32(1) / float32(L)) per sequence, +0.0 for an empty one: the kernel's two roundings on integer rows."""
    out = np.zeros((len(cu) - 1, x.shape[1]), dtype=np.float32)
    for b in range(len(cu) - 1):
        L = int(cu[b + 1] - cu[b])
        if L:
            out[b] = x[cu[b]: cu[b + 1]].astype(np.float64).sum(axis=0).astype(np.float32) * (np.float32(1) / np.float32(L))
    return out


def seg_mean_ref64(x, cu):
    out = np.zeros((len(cu) - 1, x.shape[1]))
    for b in range(len(cu) - 1):
        if cu[b + 1] > cu[b]:
            out[b] = x[cu[b]: cu[b + 1]].astype(np.float64).mean(axis=0)
    return out


def seg_splade_ref64(x, cu):
    out = np.zeros((len(cu) - 1, x.shape[1]))
    for b in range(len(cu) - 1):
        if cu[b + 1] > cu[b]:
            out[b] = np.log1p(np.maximum(x[cu[b]: cu[b + 1]].astype(np.float64), 0.0)).max(axis=0)
    return out
