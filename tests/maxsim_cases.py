"""Inputs, reference and case table of the exact MaxSim tests (test_gpu_maxsim_edges.py on the GPU, test_maxsim_reference_cpu.py
without one).  Not collected by pytest.

Exact inputs.  Every token component is a multiple of 1/4 in [-1, 1] (fp16 holds it exactly), so every product is a multiple of 1/16,
every partial sum of a 128-term dot product is a multiple of 1/16 below 2^8 and therefore exact in fp32 IN ANY ORDER, and so is the sum
of up to 128 maxima: on such inputs fz_maxsim_f16 has no rounding to hide behind and must equal the float64 formula bit for bit.
"Poison" token rows carry POISON = 1024 in dimension 127, where every query token carries 1 and every clean document token 0: a clean
document scores ~1024 * Lq too high as soon as one masked row, truncated tail or neighbouring row leaks into its maximum (largest
magnitude: 128 * (1024 + 127) < 2^18 with 2^-4 granularity: 22 significant bits, still exact).  Clean documents (even positions)
alternate with guard documents made of poison only (odd positions); rows before Doff[0], rows after Doff[N] and the tail of a document
past max_doc_len are poison too.  Both kinds of document are compared.

The case table restates the launcher's arithmetic of csrc/maxsim_tiles.h in plain Python (launch_plan) and names, for every case, the
branches of the kernel it is there for (branches_of); BRANCHES lists every branch that must be landed on."""
import dataclasses
import zlib

import numpy as np

DIM = 128
POISON = 1024.0
LQS = (32, 64, 128)

# csrc/maxsim_tiles.h (MT_*); the blocks per wave: csrc/maxsim.hip and csrc/maxsim8.hip
MS_WAVES, MS_BLOCKS_PER_WAVE, MS_DOCS_PER_WG, MS_TABLE = 8, 4, 32, 512


# ---- the reference -----------------------------------------------------------------------------------------------------------
def maxsim_ref(Qtok, Dtok, Doff, max_doc_len=None):
    """s(q, d) = sum_i max_{t < min(len_d, max_doc_len)} <Q[q, i], D[Doff[d] + t]> in float64; 0 for an empty document."""
    Qtok, Dtok = np.asarray(Qtok, dtype=np.float64), np.asarray(Dtok, dtype=np.float64)
    Q, Lq, dim = Qtok.shape
    N = len(Doff) - 1
    q2 = Qtok.reshape(Q * Lq, dim)
    out = np.zeros((Q, N), dtype=np.float64)
    for d in range(N):
        a = int(Doff[d])
        L = int(Doff[d + 1]) - a
        if max_doc_len is not None:
            L = min(L, int(max_doc_len))
        if L > 0:
            with np.errstate(invalid="ignore"):
                out[:, d] = (q2 @ Dtok[a: a + L].T).reshape(Q, Lq, L).max(axis=2).sum(axis=1)
    return out


def exact_f32(ref):
    """The reference of a grid case as float32, after asserting that float32 holds it exactly (a case that leaves the exact range fails
    here, not in the comparison with the kernel)."""
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref), "the float64 reference is not exactly representable in float32"
    return r32


def maxsim_fmax_ref(Qtok, Dtok, Doff):
    """The kernel's definition where the float64 formula is NaN (include/fusion_hip.h): a NaN dot product is skipped by the maximum
    (fmaxf), and a query token whose dot products with a document are all NaN contributes -inf."""
    Qtok, Dtok = np.asarray(Qtok, dtype=np.float64), np.asarray(Dtok, dtype=np.float64)
    out = np.zeros((Qtok.shape[0], len(Doff) - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(len(Doff) - 1):
            a, b = int(Doff[d]), int(Doff[d + 1])
            if b > a:
                dots = np.einsum("qik,tk->qit", Qtok, Dtok[a:b])
                out[:, d] = np.fmax.reduce(dots, axis=2, initial=-np.inf).sum(axis=1)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def grid_queries(rng, Q, Lq):
    q = rng.integers(-4, 5, (Q, Lq, DIM)).astype(np.float64) / 4.0
    q[..., DIM - 1] = 1.0
    return q.astype(np.float16)


def grid_corpus(rng, lens, max_doc_len, guards=True, pre=0, post=0, poison=POISON):
    """-> (Dtok [pre + sum(lens) + post, 128] fp16, Doff [N + 1] int64 with Doff[0] = pre)."""
    lens = np.asarray(lens, dtype=np.int64)
    Doff = np.zeros(len(lens) + 1, dtype=np.int64)
    Doff[0] = pre
    Doff[1:] = pre + np.cumsum(lens)
    rows = int(Doff[-1]) + post
    tok = rng.integers(-4, 5, (rows, DIM)).astype(np.float64) / 4.0
    tok[:, DIM - 1] = 0.0
    bad = np.zeros(rows, dtype=bool)
    bad[:pre] = True
    bad[int(Doff[-1]):] = True
    for d, L in enumerate(lens):
        a = int(Doff[d])
        if guards and d % 2 == 1:
            bad[a: a + L] = True
        elif L > max_doc_len:
            bad[a + max_doc_len: a + L] = True
    tok[bad, DIM - 1] = poison
    return tok.astype(np.float16), Doff


def unit_queries(rng, Q, Lq):
    q = rng.normal(0, 1, (Q, Lq, DIM))
    return (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float16)


def unit_corpus(rng, lens, pre=0, post=0):
    lens = np.asarray(lens, dtype=np.int64)
    Doff = np.zeros(len(lens) + 1, dtype=np.int64)
    Doff[0] = pre
    Doff[1:] = pre + np.cumsum(lens)
    tok = rng.normal(0, 1, (int(Doff[-1]) + post, DIM))
    tok /= np.maximum(np.linalg.norm(tok, axis=1, keepdims=True), 1e-6)
    return tok.astype(np.float16), Doff


def special_inputs():
    """Four queries of 32 tokens against six documents: +inf in a row, fp16 maximum values, inf - inf, a query token of zeros."""
    rng = np.random.default_rng(5)
    Lq, Q = 32, 4
    Qtok = grid_queries(rng, Q, Lq).astype(np.float64)
    Qtok[..., 5] = np.abs(Qtok[..., 5]) + 0.25       # dimensions 5 and 6 positive in queries 0, 1, 3 ...
    Qtok[..., 6] = np.abs(Qtok[..., 6]) + 0.25
    Qtok[1, 7] = 0.0                                  # ... query 1 has a token of zeros (inf * 0 = NaN against the inf row)
    Qtok[2, :, 5] = 0.0                               # query 2 meets every +inf with a zero
    Dtok, Doff = grid_corpus(rng, [20, 40, 33, 1, 0, 17], 512, guards=False)
    Dtok = Dtok.astype(np.float64)
    Dtok[int(Doff[0]) + 3, 5] = np.inf                                  # document 0: one row with +inf
    Dtok[int(Doff[1]): int(Doff[2])] = rng.choice([0.0, 65504.0, -65504.0], (40, DIM), p=[0.9, 0.05, 0.05])   # document 1: fp16 maximum values
    Dtok[int(Doff[2]) + 32, 5:7] = (np.inf, -np.inf)                    # document 2: inf - inf in the one row of its last tile
    Dtok[int(Doff[3]), 5:7] = (np.inf, -np.inf)                         # document 3: nothing but such a row
    return Qtok.astype(np.float16), Dtok.astype(np.float16), Doff


def check_special_reference(ref):
    """What the float64 formula gives on special_inputs(): the premises of test_special_values."""
    assert np.isposinf(ref[0, 0]) and np.isposinf(ref[3, 0]) and np.isnan(ref[1, 0]) and np.isnan(ref[2, 0])
    assert np.isnan(ref[:, 2]).all() and np.isnan(ref[:, 3]).all()
    assert np.isfinite(ref[:, 1]).all() and np.abs(ref[:, 1]).max() > 65504 and not ref[:, 4].any() and np.isfinite(ref[:, 5]).all()
    finite = ref[np.isfinite(ref)]
    assert np.array_equal(finite.astype(np.float32).astype(np.float64), finite), "a finite special-value score is not exact in float32"


# ---- the launcher, restated --------------------------------------------------------------------------------------------------
def launch_plan(Q, Lq, lens, max_doc_len):
    """What fz_maxsim_f16 and maxsim_kernel derive from the shapes: the waves' query assignment and every range's tile table."""
    QB = Lq // 32
    qpw = MS_BLOCKS_PER_WAVE // QB
    QG = -(-(Q * QB) // (MS_WAVES * MS_BLOCKS_PER_WAVE))
    docs_per_wg = min(MS_TABLE // (-(-max_doc_len // 32)), MS_DOCS_PER_WG)
    N = len(lens)
    DR = -(-N // docs_per_wg)
    waves = []
    for qg in range(QG):
        q_first = qg * MS_WAVES * qpw
        nq_group = min(Q - q_first, MS_WAVES * qpw)
        per_wave = -(-nq_group // MS_WAVES)
        for w in range(MS_WAVES):
            q0 = q_first + w * per_wave
            nq = max(0, min(per_wave, q_first + nq_group - q0))
            waves.append(dict(qg=qg, w=w, q0=q0, per_wave=per_wave, nq=nq, ncb=nq * QB * 2))
    ranges = []
    for dr in range(DR):
        eff = [min(int(L), max_doc_len) for L in lens[dr * docs_per_wg: (dr + 1) * docs_per_wg]]
        tiles = []    # (document in the range, rows_valid, last tile of the document)
        for i, L in enumerate(eff):
            nt = (L + 31) // 32
            tiles += [(i, min(L - 32 * k, 32), k == nt - 1) for k in range(nt)]
        assert len(tiles) <= MS_TABLE
        ranges.append(dict(first=dr * docs_per_wg, eff=eff, tiles=tiles))
    return dict(QB=QB, qpw=qpw, QG=QG, docs_per_wg=docs_per_wg, N=N, DR=DR, waves=waves, ranges=ranges, blocks=8 * QG * (-(-DR // 8)))


# ---- the branches ------------------------------------------------------------------------------------------------------------
FILL_Q = {32: (1, 2, 3, 4, 5, 8, 9, 17, 25, 31, 32, 33), 64: (1, 2, 3, 8, 9, 15, 16, 17, 19, 25), 128: (1, 7, 8, 9)}
EDGE_LENS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 511, 512)
TILE_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17)
DOCS_PER_WG = {512: 32, 513: 30, 1024: 16, 16384: 1}
TRUNCATE_AT = (1, 16, 17, 32, 33, 100, 512)
MAP_N = {1: 1, 31: 1, 32: 1, 33: 2, 255: 8, 256: 8, 257: 9}    # N -> DR at docs_per_wg = 32

BRANCHES = {
    **{("nq", Lq, nq): "a wave holding nq queries" for Lq in LQS for nq in range(0, 4 // (Lq // 32) + 1)},
    **{("ncb", Lq, ncb): "live column blocks of a wave" for Lq in LQS for ncb in range(0, 9, 2) if ncb % (Lq // 16) == 0},
    **{("load", Lq, k): "tile body: ncb == 8 / the live pairs only / a wave without queries" for Lq in LQS for k in ("full", "partial", "idle")
       if (Lq, k) != (128, "partial")},      # Lq = 128: one query fills a wave
    **{("store32", taken): "Lq = 32 epilogue: 2 + h < nq" for taken in (True, False)},
    **{("store64", taken): "Lq = 64 epilogue: nq > 1" for taken in (True, False)},
    ("full-groups", 3): "three full query groups and a thin one (Q = 195 at Lq = 64)",
    **{("rows", Lq, k): "rows_valid <= 16 (first row block only) / 17..31 (masked in fold) / 32" for Lq in LQS for k in ("half", "masked", "full")},
    **{("len", Lq, L): "document length" for Lq in LQS for L in EDGE_LENS},
    **{("tiles", Lq, T): "tiles of one range: ring wrap and half toggle" for Lq in LQS for T in TILE_COUNTS + (MS_TABLE,)},
    **{("docs_per_wg", Lq, m, d): "launcher: documents per workgroup" for Lq in LQS for m, d in DOCS_PER_WG.items()},
    **{("truncated", Lq, m): "a document longer than max_doc_len" for Lq in LQS for m in TRUNCATE_AT},
    **{("truncated-last", Lq): "the last document of the corpus truncated: its masked rows read its own poisoned tail" for Lq in LQS},
    **{("empty", Lq, k): "an empty document / range" for Lq in LQS for k in ("first", "last", "range", "corpus-last")},
    **{("map", Lq, N, DR): "block mapping at docs_per_wg = 32" for Lq in LQS for N, DR in MAP_N.items()},
    **{("map-idle-block", Lq): "dr >= DR: a workgroup without a range" for Lq in LQS},
    **{("map-DR9-QG2", Lq): "nine ranges, two query groups" for Lq in LQS},
    **{("end", Lq, k): "corpus end" for Lq in LQS for k in ("partial-tile-at-sumL", "rows-beyond-Doff[N]", "Doff[0]>0")},
}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    Lq: int
    Q: int
    lens: tuple
    max_doc_len: int
    claims: tuple                # the branches this case is there for (checked against branches_of on the CPU)
    guards: bool = True
    pre: int = 0
    post: int = 0

    @property
    def id(self):
        return f"{self.name}-Lq{self.Lq}-Q{self.Q}-N{len(self.lens)}-m{self.max_doc_len}"

    def rng(self):
        return np.random.default_rng(zlib.crc32(self.id.encode()))

    def inputs(self, poison=POISON):
        rng = self.rng()
        Qtok = grid_queries(rng, self.Q, self.Lq)
        Dtok, Doff = grid_corpus(rng, self.lens, self.max_doc_len, self.guards, self.pre, self.post, poison)
        return Qtok, Dtok, Doff


def branches_of(c):
    p = launch_plan(c.Q, c.Lq, c.lens, c.max_doc_len)
    Lq, lens, N = c.Lq, c.lens, len(c.lens)
    hit = {("docs_per_wg", Lq, c.max_doc_len, p["docs_per_wg"])}
    for wv in p["waves"]:
        nq, ncb = wv["nq"], wv["ncb"]
        hit |= {("nq", Lq, nq), ("ncb", Lq, ncb), ("load", Lq, "full" if ncb == 8 else "partial" if ncb else "idle")}
        if Lq == 32:
            hit |= {("store32", 2 + h < nq) for h in (0, 1) if h < nq}
        if Lq == 64 and nq:
            hit.add(("store64", nq > 1))
    full_groups = sum(all(wv["ncb"] == 8 for wv in p["waves"] if wv["qg"] == g) for g in range(p["QG"]))
    if full_groups >= 3 and full_groups < p["QG"]:
        hit.add(("full-groups", 3))
    live = [any(L > 0 for L in r["eff"]) for r in p["ranges"]]
    for dr, r in enumerate(p["ranges"]):
        hit.add(("tiles", Lq, len(r["tiles"])))
        hit |= {("rows", Lq, "half" if rv <= 16 else "masked" if rv < 32 else "full") for _, rv, _ in r["tiles"]}
        hit |= {("len", Lq, L) for L in r["eff"]}
        if live[dr]:
            if r["eff"][0] == 0:
                hit.add(("empty", Lq, "first"))
            if r["eff"][-1] == 0:
                hit.add(("empty", Lq, "last"))
        elif 0 < dr < p["DR"] - 1 and live[dr - 1] and live[dr + 1]:
            hit.add(("empty", Lq, "range"))
    if lens[-1] == 0 and any(lens):
        hit.add(("empty", Lq, "corpus-last"))
    if any(L > c.max_doc_len for L in lens):
        hit.add(("truncated", Lq, c.max_doc_len))
    if lens[-1] > c.max_doc_len:
        hit.add(("truncated-last", Lq))
    if p["docs_per_wg"] == MS_DOCS_PER_WG:
        hit.add(("map", Lq, N, p["DR"]))
    if p["DR"] % 8:
        hit.add(("map-idle-block", Lq))
    if p["DR"] == 9 and p["QG"] == 2:
        hit.add(("map-DR9-QG2", Lq))
    if c.post == 0 and 0 < lens[-1] <= c.max_doc_len and lens[-1] % 32:
        hit.add(("end", Lq, "partial-tile-at-sumL"))
    if c.post:
        hit.add(("end", Lq, "rows-beyond-Doff[N]"))
    if c.pre:
        hit.add(("end", Lq, "Doff[0]>0"))
    return hit


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def alternate(clean, guard=(3, 33, 1, 16, 40, 0, 17)):
    """Clean documents at the even positions, guard documents (lengths cycled from `guard`) at the odd ones."""
    out = []
    for i, L in enumerate(clean):
        out += [L, guard[i % len(guard)]]
    return tuple(out)


def _range_of_tiles(rng, T):
    """32 documents whose tile counts sum to T: documents of one to three tiles, then empty ones."""
    lens, left = [], T
    while left:
        c = min(left, int(rng.integers(1, 4)))
        lens.append(32 * (c - 1) + int(rng.integers(1, 33)))
        left -= c
    assert len(lens) <= MS_DOCS_PER_WG
    return lens + [0] * (MS_DOCS_PER_WG - len(lens))


def _thin(Lq):
    """One full query group and a thinly filled one: both the full-load and the partial tile body run."""
    return 8 * (128 // Lq) + 1


def _cases():
    out = []
    for Lq in LQS:
        QB = Lq // 32
        qpw = 4 // QB
        # the filling of the last query group
        fill_lens = alternate((40, 0, 17, 70, 5, 33, 64, 1))
        for Q in FILL_Q[Lq]:
            out.append(Case("fill", Lq, Q, fill_lens, 64, (("load", Lq, "full" if Q % (8 * qpw) == 0 else "idle" if qpw == 1 else "partial"),)))
        if Lq == 64:
            out.append(Case("fill", Lq, 195, fill_lens, 64, (("full-groups", 3), ("load", 64, "full"), ("load", 64, "partial"), ("load", 64, "idle"))))
        # document lengths: rows_valid of the last tile
        out.append(Case("lengths", Lq, _thin(Lq), alternate(EDGE_LENS), 512,
                        tuple(("len", Lq, L) for L in EDGE_LENS) + tuple(("rows", Lq, k) for k in ("half", "masked", "full"))))
        # tiles per range
        rng = np.random.default_rng(1000 + Lq)
        lens = sum((_range_of_tiles(rng, T) for T in TILE_COUNTS), [])
        out.append(Case("tiles", Lq, _thin(Lq), tuple(lens), 512, tuple(("tiles", Lq, T) for T in TILE_COUNTS)))
        out.append(Case("table", Lq, {32: 9, 64: 5, 128: 3}[Lq], (512,) * 32, 512, (("tiles", Lq, MS_TABLE),)))
        # documents per workgroup
        out.append(Case("dpw", Lq, qpw + 1, alternate((512, 30, 0, 100) * 9), 512, (("docs_per_wg", Lq, 512, 32),)))
        out.append(Case("dpw", Lq, qpw + 1, alternate((513, 30, 600, 7, 0, 512, 33) * 4 + (513, 2, 40)), 513,
                        (("docs_per_wg", Lq, 513, 30), ("truncated", Lq, 513))))
        out.append(Case("dpw", Lq, qpw + 1, alternate((1024, 1000, 1500, 5, 0, 33, 700, 64) * 2 + (90,)), 1024, (("docs_per_wg", Lq, 1024, 16),)))
        out.append(Case("dpw", Lq, qpw + 1, alternate((20, 16384, 5, 0, 33), guard=(3, 40)), 16384, (("docs_per_wg", Lq, 16384, 1),)))
        # truncation at max_doc_len; the corpus ends with a truncated clean document whose tail is poison
        for m in TRUNCATE_AT:
            clean = (m + 1, m, m + 40, max(m - 1, 1), 2 * m + 3, m + 15, m + 16, m + 17, 3 * m, m + 31, m + 32, m + 33)
            lens = alternate(clean)[:-1]
            out.append(Case("truncate", Lq, _thin(Lq), lens, m, (("truncated", Lq, m), ("truncated-last", Lq))))
        # empty documents: first / last of a live range, a whole range, the last document of the corpus
        r0 = [0] + [int(x) for x in np.random.default_rng(7).integers(1, 70, 30)] + [0]
        r2 = [int(x) for x in np.random.default_rng(8).integers(0, 70, 19)] + [0]
        out.append(Case("empty", Lq, 8 * qpw + min(3, qpw), tuple(r0 + [0] * 32 + r2), 64, tuple(("empty", Lq, k) for k in ("first", "last", "range", "corpus-last"))))
        # block mapping
        for N, DR in MAP_N.items():
            lens = tuple(int(x) for x in np.random.default_rng(N).integers(0, 70, N))
            if N == 1:
                lens = (37,)
            out.append(Case("map", Lq, qpw + 1, lens, 64, (("map", Lq, N, DR),) + ((("map-idle-block", Lq),) if DR % 8 else ())))
        out.append(Case("map", Lq, _thin(Lq), tuple(int(x) for x in np.random.default_rng(99).integers(0, 70, 260)), 64, (("map-DR9-QG2", Lq),)))
        # corpus end
        end_lens = alternate((40, 33, 64, 1)) + (45,)      # a guard, then a clean last document of 45 tokens: one full and one partial tile
        out.append(Case("end-at-sumL", Lq, _thin(Lq), end_lens, 64, (("end", Lq, "partial-tile-at-sumL"),)))
        out.append(Case("end-tail", Lq, _thin(Lq), end_lens, 64, (("end", Lq, "rows-beyond-Doff[N]"),), post=41))
        out.append(Case("end-head", Lq, _thin(Lq), end_lens, 64, (("end", Lq, "Doff[0]>0"),), pre=37))
        out.append(Case("end-both", Lq, qpw, end_lens, 64, (("end", Lq, "rows-beyond-Doff[N]"), ("end", Lq, "Doff[0]>0")), pre=5, post=3))
    # the production shape of the full load: three full query groups and a thin one over the full tile table
    out.append(Case("table", 64, 195, (512,) * 32, 512, (("tiles", 64, MS_TABLE), ("full-groups", 3))))
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
