"""Inputs, NumPy references and case tables of the exact top-k tests (test_gpu_topk_edges.py on the GPU, test_topk_cases_cpu.py without
one).  numpy only; not collected by pytest.

No tolerance anywhere: a top-k list is ids and score BITS.  The order is the one desc_key_f32 (csrc/common.h) defines -- score
descending, NaN first, -0.0 == +0.0, ties by ascending id -- restated here as np.lexsort((ids, -s)) with NaN in front (`order_desc`) and,
for the fold, as a plain stable Python sort of [running list | candidates] (`fold_ref`).  A score that went through the row sort comes
back as its key's value (-0.0 as +0.0, every NaN as the quiet NaN 0x7fc00000: `canon`); the filter's candidates keep their own bits.
test_topk_cases_cpu.py holds every reference to oracle.topk_rows / topk_merge / sort_rows_desc on every case, so the GPU side compares
the kernels with something that does not come from them.

Which branches a case lands is not claimed, it is computed: for whole rows from fz_topk_rows_plan (the function fz_topk_rows_f32 itself
runs, host only), for the filter from `filter_walk` / `filter_stretches` (topk_filter_kernel's geometry restated: round, wave stretch,
step, lane, element of every column; the CPU file proves the walk a partition of [0, n) in ascending order), for the unordered fold from
`tie_rule` (the conditions of topk_tiefix_kernel), for the selection from `select_sim` (topk_select_kernel's bisection).  BRANCHES lists
what the union of the cases must land."""
import ctypes
import dataclasses
import zlib

import numpy as np

SORT_ROW_F32, TOPK_CHUNK, MAX_K = 35840, 28672, 8192        # csrc/sort.h, csrc/topk.hip (the CPU file checks them against the library)
NW, STEP, UNR = 4, 256, 8                                    # topk_filter_kernel: waves, columns per step, steps per unguarded group
SPAN = NW * 64 * STEP                                        # columns per round
TIE_MARGIN, TIE_RUN_MAX = 64, 512                            # topk_tiefix_kernel
SELECT_MAX_N = 1024 * 28
PLAN_LEVELS = 12
PLAN_FIELDS = 3 + 4 * PLAN_LEVELS
ID_BASE = (1 << 33) + 977                                    # above 2^33: an id kept in 32 bits anywhere comes back wrong
S_GUARD, I_GUARD = np.float32(-54321.0), -7                  # sentinel of output cells the kernels must not touch
QNAN = 0x7FC00000
NAN_PAYLOAD = np.array([0x7FC00123], dtype=np.uint32).view(np.float32)[0]      # a NaN whose bits the filter must hand on unchanged
FRAME = np.float32(np.inf)                                   # behind every row, in the ghost rows: a column read past n enters the list
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- the order -------------------------------------------------------------------------------------------------------------------------
def desc_key(s):
    """desc_key_f32: float32 -> uint32, larger score <=> smaller key; -0.0 == +0.0; every NaN -> 0 (first)."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).copy()
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u[u == np.uint32(0x80000000)] = 0
    asc = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(nan, np.uint32(0), ~asc).astype(np.uint32)


KEY_NEG_INF = int(desc_key(np.array([-np.inf], dtype=np.float32))[0])


def canon(s):
    """A score as the row sort writes it back: -0.0 -> +0.0, every NaN -> the quiet NaN (float32 and float64)."""
    s = np.array(s, copy=True)
    s[s == 0] = 0
    s[np.isnan(s)] = np.array([QNAN], dtype=np.uint32).view(np.float32)[0] if s.dtype == np.float32 else \
        np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
    return s


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def order_desc(s, ids, pad=None):
    """Positions of a list in (score desc, NaN first, -0 == +0, id asc) order; pad (bool): entries that go behind everything."""
    s = np.asarray(s)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s.astype(np.float64))
    keys = (ids, neg, ~nan) if pad is None else (ids, neg, ~nan, pad)
    return np.lexsort(keys)


def topk_ref(scores, k, id_base=0):
    """k best per row -> (scores [rows, k] float32 as the sort writes them, ids [rows, k] int64), (-inf, -1) padding."""
    rows, n = scores.shape
    os_, oi = np.full((rows, k), -np.inf, dtype=np.float32), np.full((rows, k), -1, dtype=np.int64)
    cols = np.arange(n, dtype=np.int64)
    for r in range(rows):
        o = order_desc(scores[r], cols)[:k]
        os_[r, : len(o)], oi[r, : len(o)] = canon(scores[r, o]), id_base + o
    return os_, oi


def merge_ref(in_s, in_i):
    """[G, rows, k] lists -> the k best of each row's G * k entries; (-inf, -1) padding entries last."""
    G, rows, k = in_s.shape
    os_, oi = np.empty((rows, k), dtype=np.float32), np.empty((rows, k), dtype=np.int64)
    for r in range(rows):
        s, i = in_s[:, r].reshape(-1), in_i[:, r].reshape(-1)
        o = order_desc(s, i, pad=i < 0)[:k]
        os_[r], oi[r] = canon(s[o]), i[o]
    return os_, oi


# ---- whole rows: the plan, from the library --------------------------------------------------------------------------------------------
def rows_plan_status(n, k, out=True):
    from fusion_amd import _lib
    buf = (ctypes.c_int32 * PLAN_FIELDS)(*([-1] * PLAN_FIELDS))
    rc = _lib.lib().fz_topk_rows_plan(n, k, buf if out else None)
    return rc, list(buf)


def rows_plan(n, k):
    rc, f = rows_plan_status(n, k)
    assert rc == 0, (n, k, rc)
    lv = [dict(zip(("width", "chunks", "kk", "fill"), f[3 + 4 * l: 7 + 4 * l])) for l in range(f[0])]
    return dict(levels=f[0], pad=f[1], last=f[2], lv=lv)


BRANCHES = {
    **{("rows", "levels", l): "fz_topk_rows_f32: chunk-sort-truncate levels in front of the finishing sort (2: two or more)" for l in (0, 1, 2)},
    **{("rows", "fill", l): "fill_absent_kernel at this level: the last chunk holds fewer than kk keys" for l in (1, 2)},
    ("rows", "pad"): "topk_pad_kernel: n < k",
    **{("filter", "rounds", r): "topk_filter_kernel: one round of 65,536 columns / a second one (base += tot, w0 from r0)" for r in ("one", "several")},
    ("filter", "unr-group"): "a whole group of UNR steps read under no branch", ("filter", "ragged-step"): "a step that ends at n",
    **{("filter", "path", p): "16-byte loads / the scalar path (ld % 4 != 0 or a base off 16 bytes)" for p in ("vector", "scalar")},
    ("filter", "empty-wave"): "a wave whose stretch starts at or past n",
    **{("filter", "pass2-short", m): "pass 2: a last group of m marked steps, the last one repeated" for m in (1, 2, 3)},
    ("filter", "pass2-full"): "pass 2: a whole group of four marked steps", ("filter", "inner64"): "inner >= 64: the mask is taken whole",
    **{("filter", "cap-hit", r): "the survivor that crosses cap lies in the first round / in a later one" for r in ("round1", "round2")},
    ("filter", "prior"): "append form behind candidates already in the list", ("filter", "update"): "fz_topk_update_f32: list copy, k > 0, buf_len",
    ("fold", "ordered"): "the sort writes the new list", ("fold", "unordered"): "k + 64 entries to scratch, topk_tiefix_kernel",
    **{("fold", "tie", t): "topk_tiefix_kernel, a run of equal keys: " + t for t in
       ("closes-at-k+63:clear", "open-at-k+64:flag", "512-inside-k:clear", "513:flag", "behind-the-cut:clear", "touches-the-end:clear", "short-list:padding")},
    ("merge", "at-limit"): "G * k == 35,840",
    **{("select", inst, b): "topk_select_kernel<T, E, KW>" for inst in ("256x4", "256x16", "1024x16", "1024x28") for b in (32, 64)},
    ("select", "bisect-early"): "the bisection stops at a midpoint whose count lies in [need, cap]",
    ("select", "bisect-early-at-cap"): "... with a count of exactly cap, where a lower threshold would do too (c <= cap, not c < cap)",
    ("select", "tie-overflow"): "no midpoint does: the count exceeds cap", ("select", "total<=cap"): "no bisection: every listed document is a candidate",
}


# ---- whole-row cases -------------------------------------------------------------------------------------------------------------------
def row_data(kind, n, rng):
    """One row of float32 scores.  ties: seven values; const; neginf; special: ties with NaN and +-0 pairs; borders: the best value
    sits on both sides of every 28,672-column chunk border (and at both ends) over negative ties; lastchunk: ascending with the column in
    pairs, so the k best are the last k columns."""
    if kind == "const":
        return np.full(n, 0.75, dtype=np.float32)
    if kind == "neginf":
        return np.full(n, -np.inf, dtype=np.float32)
    if kind == "lastchunk":
        return (np.arange(n) // 2).astype(np.float32)
    if kind == "borders":
        s = (rng.integers(-8, 0, n) / 4.0).astype(np.float32)
        for b in list(range(0, n + 1, TOPK_CHUNK)) + [n]:
            s[max(b - 3, 0): min(b + 3, n)] = 2.0
        return s
    s = (rng.integers(-3, 4, n) / 2.0).astype(np.float32)
    if kind == "special":
        z = np.flatnonzero(s == 0)
        s[z[::2]] = -0.0
        s[rng.integers(0, n, max(n // 50, 1))] = np.nan
        s[[0, n - 1]] = np.nan
    else:
        assert kind == "ties", kind
    return s


@dataclasses.dataclass(frozen=True)
class RowsCase:
    n: int
    k: int
    kinds: tuple                 # one data kind per row
    claims: tuple = ()

    rows = property(lambda self: len(self.kinds))

    @property
    def id(self):
        return f"rows-n{self.n}-k{self.k}-" + "+".join(self.kinds)

    def inputs(self):
        return np.stack([row_data(kind, self.n, rng_of(self.id, r)) for r, kind in enumerate(self.kinds)]) if self.n else \
            np.zeros((self.rows, 0), dtype=np.float32)

    def branches(self):
        p = rows_plan(self.n, self.k)
        hit = {("rows", "levels", min(p["levels"], 2))}
        hit |= {("rows", "fill", min(l + 1, 2)) for l, lv in enumerate(p["lv"]) if lv["fill"]}
        if p["pad"]:
            hit.add(("rows", "pad"))
        return hit


T3 = ("ties", "special", "const")
ROWS_CASES = [RowsCase(n, 100, T3) for n in (1, 99, 100, 101)] + [
    RowsCase(0, 5, ("ties",), (("rows", "pad"),)), RowsCase(1, 1, ("ties", "neginf")), RowsCase(2, 1, ("special", "ties")),
    RowsCase(50, 8192, ("ties", "neginf"), (("rows", "pad"),)), RowsCase(5000, 8192, ("special",), (("rows", "pad"),)),
    RowsCase(35840, 1000, ("ties", "special", "lastchunk"), (("rows", "levels", 0),)), RowsCase(35840, 8192, ("ties",)),
    RowsCase(35841, 7169, ("ties", "lastchunk"), (("rows", "levels", 1),)), RowsCase(35841, 7170, ("ties", "lastchunk"), (("rows", "fill", 1),)),
    RowsCase(35841, 1, ("borders", "lastchunk")),
    RowsCase(57344, 1000, ("ties", "borders")), RowsCase(57345, 1000, ("special", "lastchunk", "neginf"), (("rows", "fill", 1),)),
    RowsCase(57345, 1, ("lastchunk", "borders")),
    RowsCase(114688, 8192, ("ties",), (("rows", "levels", 1),)), RowsCase(114689, 8192, ("ties", "lastchunk"), (("rows", "levels", 2), ("rows", "fill", 1))),
    RowsCase(114689, 8192, ("const",)), RowsCase(143360, 8192, ("special",), (("rows", "levels", 2),)),
    RowsCase(200705, 8000, ("ties", "lastchunk", "special"), (("rows", "levels", 2), ("rows", "fill", 1), ("rows", "fill", 2))),
    RowsCase(200705, 1, ("borders",)),
]
ROWS_AXIS_N = (1, 35840, 35841, 57344, 57345, 114688, 114689, 200705)


# ---- the filter's geometry ---------------------------------------------------------------------------------------------------------------
def filter_stretches(n, vec=True):
    """topk_filter_kernel's loop bounds: per (round, wave) its stretch [w0, w0 + steps * 256), the columns of it that exist, the whole UNR
    groups read under no branch, `inner` (steps all of whose columns exist; 0 on the scalar path) and the ragged step, if any."""
    out = []
    for rnd, r0 in enumerate(range(0, n, SPAN)):
        nr = min(n - r0, SPAN)
        steps = (nr + NW * STEP - 1) // (NW * STEP)
        for w in range(NW):
            w0 = r0 + w * steps * STEP
            s0 = 0
            while vec and s0 + UNR <= steps and w0 + (s0 + UNR) * STEP <= n:
                s0 += UNR
            ncols = max(0, min(n - w0, steps * STEP))
            out.append(dict(round=rnd, wave=w, r0=r0, w0=w0, steps=steps, ncols=ncols, groups=s0 // UNR,
                            inner=max(0, min(steps, (n - w0) // STEP)) if vec else 0, ragged=ncols // STEP if ncols % STEP else None))
    return out


def filter_walk(n):
    """Every (round, wave, step, lane, element) the kernel visits whose column j0 + e is below n, in the order the compaction numbers
    them -> dict of int64 arrays (round, wave, step, lane, elem, col)."""
    parts = []
    for s in filter_stretches(n):
        st, lane, e = np.meshgrid(np.arange(s["steps"]), np.arange(64), np.arange(4), indexing="ij")
        col = s["w0"] + st * STEP + lane * 4 + e
        keep = col < n
        parts.append(np.stack([np.full(keep.sum(), s["round"]), np.full(keep.sum(), s["wave"]), st[keep], lane[keep], e[keep], col[keep]]))
    a = np.concatenate(parts, axis=1).astype(np.int64) if parts else np.zeros((6, 0), dtype=np.int64)
    return dict(zip(("round", "wave", "step", "lane", "elem", "col"), a))


def filter_plants(n):
    """The columns where a survivor is planted: ends of every wave stretch of every round, both sides of the step borders next to them,
    lanes 0 and 63 x elements 0 .. 3, the last column of the last whole UNR group and the first after it, the ragged step, n - 1, and both
    sides of every round border."""
    c = {0, n - 1, SPAN - 1, SPAN, 2 * SPAN - 1, 2 * SPAN}
    for s in filter_stretches(n):
        if not s["ncols"]:
            continue
        w0, end = s["w0"], s["w0"] + s["ncols"]
        c |= {w0, end - 1, w0 + STEP - 1, w0 + STEP}
        c |= {w0 + e for e in range(4)} | {w0 + 63 * 4 + e for e in range(4)}
        last_border = w0 + (s["ncols"] - 1) // STEP * STEP
        c |= {last_border - 1, last_border}
        if s["groups"]:
            c |= {w0 + s["groups"] * UNR * STEP - 1, w0 + s["groups"] * UNR * STEP}
        if s["ragged"] is not None:
            c |= {w0 + s["ragged"] * STEP, w0 + s["ragged"] * STEP + 1}
    return np.array(sorted(j for j in c if 0 <= j < n), dtype=np.int64)


def filter_marks(n, m):
    """One survivor in m steps of every wave stretch (all its steps when it has no more, or m is None): the first, the last and steps
    spread between them; lane and element move with the step."""
    c = set()
    for s in filter_stretches(n):
        have = -(-s["ncols"] // STEP)
        if not have:
            continue
        pick = range(have) if m is None or m >= have else sorted({round(i * (have - 1) / max(m - 1, 1)) for i in range(m)})
        for st in pick:
            j = s["w0"] + st * STEP + ((7 * st + 3 * s["wave"]) % 64) * 4 + st % 4
            c.add(j if j < n else s["w0"] + st * STEP)
    return np.array(sorted(c), dtype=np.int64)


DENSITIES = ("planted", "marks1", "marks2", "marks3", "marks4", "marks5", "every-step", "all")


def survivor_cols(n, density):
    if density == "planted":
        return filter_plants(n)
    if density == "all":
        return np.arange(n, dtype=np.int64)
    return filter_marks(n, None if density == "every-step" else int(density[5:]))


def filter_branches(n, cols, vec):
    hit = {("filter", "rounds", "one" if n <= SPAN else "several"), ("filter", "path", "vector" if vec else "scalar")}
    cols = np.asarray(cols)
    for s in filter_stretches(n, vec):
        if not s["ncols"]:
            hit.add(("filter", "empty-wave"))
            continue
        if s["groups"]:
            hit.add(("filter", "unr-group"))
        if s["ragged"] is not None:
            hit.add(("filter", "ragged-step"))
        mine = cols[(cols >= s["w0"]) & (cols < s["w0"] + s["ncols"])]
        marked = np.unique((mine - s["w0"]) // STEP)
        in_m = int((marked < s["inner"]).sum())
        if in_m and s["inner"] >= 64:
            hit.add(("filter", "inner64"))
        if in_m >= 4:
            hit.add(("filter", "pass2-full"))
        if in_m % 4:
            hit.add(("filter", "pass2-short", in_m % 4))
    return hit


LAYOUTS = ("aligned", "offset", "oddld", "slice")
LAYOUT_VEC = {"aligned": True, "offset": False, "oddld": False, "slice": True}
GHOST = 1024                                  # +inf floats behind the last row, at least


def layout(name, rows, n):
    """-> (floats in the buffer, offset of row 0, ld): aligned: ld % 4 == 0 on a 16-byte base; offset: the base one float off; oddld;
    slice: columns [8, 8 + n) of a wider plane (as TopkStream.feed slices its pieces)."""
    ld = -(-n // 4) * 4 + 4
    off = 2 * ld
    if name == "offset":
        off += 1
    elif name == "oddld":
        ld = n + 5 if n % 2 == 0 else n + 4
        off = 2 * ld + (-2 * ld) % 4
    elif name == "slice":
        ld += 24
        off = 2 * ld + 8
    else:
        assert name == "aligned"
    assert ld > n and (ld % 4 == 0) == (name != "oddld") and (off % 4 == 0) == (name != "offset")
    return off + rows * ld + GHOST, off, ld


def framed(scores, name):
    """scores [rows, n] inside a flat +inf buffer in the given layout -> (buffer, offset, ld)."""
    rows, n = scores.shape
    size, off, ld = layout(name, rows, n)
    buf = np.full(size, FRAME, dtype=np.float32)
    for r in range(rows):
        buf[off + r * ld: off + r * ld + n] = scores[r]
    return buf, off, ld


TAU_KINDS = ("zero", "finite", "neg", "-inf", "+inf", "nan")


def filter_row(kind, n, cols):
    """-> (tau, scores [n]): the background equals tau (or is below it), the columns `cols` hold nextafter(tau, +inf) or a NaN.
    zero: tau = +0.0 over a background of -0.0; neg: tau = -2.5 over -2.5 and -inf; -inf: only -FLT_MAX and NaN beat it; +inf: nothing
    but the NaNs survives (cols[::2]); nan: everything survives."""
    up = lambda t: np.nextafter(np.float32(t), np.float32(np.inf))
    s = np.empty(n, dtype=np.float32)
    cols = np.asarray(cols, dtype=np.int64)
    if kind == "zero":
        tau, s[:], plant = np.float32(0.0), -0.0, up(0.0)
    elif kind == "finite":
        tau, s[:], plant = np.float32(1.5), 1.5, up(1.5)
    elif kind == "neg":
        tau, plant = np.float32(-2.5), up(-2.5)
        s[:] = -2.5
        s[1::2] = -np.inf
    elif kind == "-inf":
        tau, s[:], plant = np.float32(-np.inf), -np.inf, up(-np.inf)
    elif kind == "+inf":
        tau, plant = np.float32(np.inf), np.float32(3.0e38)
        s[:] = np.inf
        s[1::3] = 7.0
    else:
        assert kind == "nan"
        tau, plant = np.float32(np.nan), np.float32(-1.0)
        s[:] = (np.arange(n) % 5).astype(np.float32)
    s[cols] = plant
    s[cols[::2]] = NAN_PAYLOAD
    return tau, s


def filter_survivors(scores, tau):
    """[rows, n] bool: column j enters row r's candidates iff !(scores[r, j] <= tau[r])."""
    with np.errstate(invalid="ignore"):
        return ~(scores <= np.asarray(tau, dtype=np.float32)[:, None])


def filter_expected(scores, tau, prior_len, cap, id_base):
    """The append: per row the (score, id) pairs written behind its prior candidates in ascending column order, cut at cap ->
    (list of (scores, ids) per row, new cand_len [rows], overflow flag)."""
    out, lens, flag = [], [], 0
    for r, sel in enumerate(filter_survivors(scores, tau)):
        j = np.flatnonzero(sel)
        room = max(0, cap - int(prior_len[r]))
        flag |= int(len(j) > room)
        out.append((scores[r, j[:room]], id_base + j[:room].astype(np.int64)))
        lens.append(min(int(prior_len[r]) + len(j), cap))
    return out, np.array(lens, dtype=np.int32), flag


@dataclasses.dataclass(frozen=True)
class FilterCase:
    n: int
    density: str
    taus: tuple = ("zero", "finite", "neg")      # one row per threshold kind
    prior: tuple = (0, 2, 5)                     # candidates already in each row's list
    slack: int = 3                               # cap = the largest (prior + survivors) + slack; negative: that many too few
    cross: int = -1                              # >= 0: cap is hit at this survivor of row 0 (see cap_for)

    rows = property(lambda self: len(self.taus))

    @property
    def id(self):
        return f"filter-n{self.n}-{self.density}-" + "+".join(self.taus) + (f"-cross{self.cross}" if self.cross >= 0 else "") + \
            (f"-slack{self.slack}" if self.slack != 3 else "")

    def cols(self):
        return survivor_cols(self.n, self.density)

    def inputs(self):
        """-> (tau [rows], scores [rows, n])."""
        rows = [filter_row(kind, self.n, self.cols()) for kind in self.taus]
        return np.array([t for t, _ in rows], dtype=np.float32), np.stack([s for _, s in rows])

    def cap(self):
        tau, sc = self.inputs()
        cnt = filter_survivors(sc, tau).sum(axis=1)
        if self.cross >= 0:
            return int(self.prior[0]) + self.cross      # row 0: survivor number `cross` (from 0) is the first that finds no room
        return max(1, int((cnt + np.array(self.prior[: self.rows])).max()) + self.slack)

    def branches(self):
        cols = self.cols()
        hit = set()
        for name in LAYOUTS:
            hit |= filter_branches(self.n, cols, LAYOUT_VEC[name])
        if any(self.prior[: self.rows]):
            hit.add(("filter", "prior"))
        tau, sc = self.inputs()
        sel = filter_survivors(sc, tau)
        for r in range(self.rows):
            j = np.flatnonzero(sel[r])
            room = self.cap() - int(self.prior[r])
            if len(j) > room:
                hit.add(("filter", "cap-hit", "round1" if j[max(room, 0)] < SPAN else "round2"))
        return hit


FILTER_N = (1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 2049, 8191, 8192, 8193, 65535, 65536, 65537, 66561, 131077)
FILTER_CASES = [FilterCase(n, d) for n in FILTER_N for d in DENSITIES]
MIXED_TAU_CASES = [FilterCase(n, "planted", taus=("finite", "-inf", "+inf", "nan", "zero"), prior=(1, 0, 3, 2, 0)) for n in (257, 8193, 66561)]


def _cap_cases():
    """n = 131,077 (two rounds), planted: the cap holds exactly (slack 0) and misses by one, and the survivor that finds no room lies in
    each wave of the first round and in the second round."""
    n = 131077
    cols = filter_plants(n)
    out = [FilterCase(n, "planted", taus=("finite", "finite"), prior=(4, 4), slack=0), FilterCase(n, "planted", taus=("finite", "finite"), prior=(4, 4), slack=-1)]
    for s in filter_stretches(n):
        if s["ncols"] and (s["round"] == 0 or s["wave"] == 0):
            first = int(np.searchsorted(cols, s["w0"] + 1))      # the survivor behind the stretch's first one
            out.append(FilterCase(n, "planted", taus=("finite", "zero"), prior=(4, 0), cross=first))
    return out


CAP_CASES = _cap_cases()
ALL_FILTER_CASES = FILTER_CASES + MIXED_TAU_CASES + CAP_CASES
UPDATE_N = FILTER_N                                               # the update form: planted and every-step at every n
UPDATE_DENSITIES = ("planted", "every-step")
UPDATE_BRANCH = ("filter", "update")


@dataclasses.dataclass(frozen=True)
class UpdateCase:
    n: int
    density: str

    @property
    def id(self):
        return f"update-n{self.n}-{self.density}"

    def inputs(self):
        return update_inputs(self.n, self.density)

    def branches(self):
        """The update form's own branch, and what its filter launch shares with the append form (no prior list, no cap hit)."""
        cols = survivor_cols(self.n, self.density)
        return {UPDATE_BRANCH}.union(*(filter_branches(self.n, cols, LAYOUT_VEC[name]) for name in LAYOUTS))


def update_inputs(n, density):
    """fz_topk_update_f32 over the filter's inputs: a FULL running list of k scores equal to tau (ids below the chunk's), k = survivors + 5,
    so every survivor shows in the new list: NaNs first, then nextafter(tau), each in ascending id order, then the list's own entries."""
    case = FilterCase(n, density)
    tau, sc = case.inputs()
    cnt = int(filter_survivors(sc, tau).sum(axis=1).max())
    k = cnt + 5
    run_s = np.repeat(tau[:, None], k, axis=1).astype(np.float32)
    run_i = np.tile(np.arange(k, dtype=np.int64) * 3 + 11, (case.rows, 1))
    return case, k, run_s, run_i, tau, sc


def update_ref(run_s, run_i, sc, id_base):
    """The update's definition: the k best of [running list | chunk], the list's ids being below the chunk's."""
    rows, k = run_s.shape
    n = sc.shape[1]
    os_, oi = np.empty_like(run_s), np.empty_like(run_i)
    for r in range(rows):
        s = np.concatenate([run_s[r], sc[r]])
        i = np.concatenate([run_i[r], id_base + np.arange(n, dtype=np.int64)])
        o = order_desc(s, i, pad=i < 0)[:k]
        os_[r], oi[r] = canon(s[o]), i[o]
    return os_, oi


# ---- fold --------------------------------------------------------------------------------------------------------------------------------
def fold_ref(run_s, run_i, cand_s, cand_i, k):
    """One row: the first k of the STABLE sort of [running list | candidates as they stand] by the score's key -- plain Python."""
    ent = list(zip(desc_key(np.concatenate([run_s, cand_s])).tolist(), np.concatenate([run_s, cand_s]).tolist(), np.concatenate([run_i, cand_i]).tolist()))
    ent = sorted(ent, key=lambda e: e[0])
    top = ent[:k] + [(0, -np.inf, -1)] * (k - len(ent))
    return canon(np.array([e[1] for e in top], dtype=np.float32)), np.array([e[2] for e in top], dtype=np.int64), np.array([e[0] for e in ent], dtype=np.uint32)


def tie_rule(sorted_keys, k):
    """The rule of the comment above TIE_MARGIN, with topk_tiefix_kernel's own conditions: of the first L = min(have, k + 64) sorted
    entries, a run of equal keys that reaches into the first k sets the flag when it is longer than 512 or when it touches slot L - 1
    while more than L entries exist (it may go on).  -> (flag, the outcomes met)."""
    have = len(sorted_keys)
    L = min(have, k + TIE_MARGIN)
    keys = np.asarray(sorted_keys[:L])
    cut = np.flatnonzero(np.diff(keys) != 0) + 1
    flag, met = 0, set()
    for A, B in zip(np.concatenate([[0], cut]), np.concatenate([cut, [L]])):
        A, B = int(A), int(B)
        if B - A < 2:
            continue
        if A >= k:
            met.add("behind-the-cut:clear")
            continue
        if B - A > TIE_RUN_MAX:
            flag = 1
            met.add("513:flag" if B - A == TIE_RUN_MAX + 1 else "long:flag")
        elif B == L and have > L:
            flag = 1
            met.add("open-at-k+64:flag")
        else:
            if B == L and have == L == k + TIE_MARGIN:
                met.add("touches-the-end:clear")
            if B == k + TIE_MARGIN - 1 and have > L:
                met.add("closes-at-k+63:clear")
            if B - A == TIE_RUN_MAX and B <= k:
                met.add("512-inside-k:clear")
            if int(keys[A]) == KEY_NEG_INF and have == L:
                met.add("short-list:padding")
    return flag, met


def fold_row(rng, k, ncand, runs=(), real=None):
    """One row designed from its sorted outcome: real + ncand entries with strictly decreasing scores (multiples of 1/4) but for the
    runs [(A, B, kind)]: "eq" one value, "zero" alternating +0.0 / -0.0, "nan" (A = 0).  `real` of the positions (all k by default; the
    rest of the list is (-inf, -1) padding) belong to the running list -- inside a run the list's entries stand first, as they do in
    [list | candidates] -- with ids below ID_BASE, the others are candidates with distinct ids above it, ascending inside a run.
    -> (run_s [k], run_i [k], cand_s [ncand], cand_i [ncand]) with the candidates in ascending id order."""
    real = k if real is None else real
    m = real + ncand
    zero_at = next((A for A, _, kind in runs if kind == "zero"), None)
    s = ((np.float32(zero_at) if zero_at is not None else np.float32(m + 8)) - np.arange(m, dtype=np.float32)) * np.float32(0.25)
    for A, B, kind in runs:
        assert 0 <= A < B <= m
        if kind == "nan":
            assert A == 0
            s[A:B] = np.nan
        elif kind == "zero":
            s[A:B] = 0.0
            s[A + 1:B:2] = -0.0
        else:
            s[A:B] = s[A]
    from_list = np.zeros(m, dtype=bool)
    from_list[rng.choice(m, real, replace=False)] = True
    cid = ID_BASE + rng.permutation(4 * max(ncand, 1))[:ncand].astype(np.int64)
    for A, B, _ in runs:
        from_list[A:B] = np.arange(B - A) < from_list[A:B].sum()
    ids = np.empty(m, dtype=np.int64)
    ids[from_list] = 5 + 3 * np.arange(real)
    ids[~from_list] = cid
    for A, B, _ in runs:
        c = np.flatnonzero(~from_list[A:B]) + A
        ids[c] = np.sort(ids[c])
    run_s, run_i = np.full(k, -np.inf, dtype=np.float32), np.full(k, -1, dtype=np.int64)
    run_s[:real], run_i[:real] = s[from_list], ids[from_list]
    o = np.argsort(ids[~from_list], kind="stable")
    return run_s, run_i, s[~from_list][o], ids[~from_list][o]


@dataclasses.dataclass(frozen=True)
class FoldCase:
    name: str
    k: int
    cap: int
    rows_spec: tuple             # per row (ncand, runs, real, cand_len as handed to the kernel or None = ncand)
    claims: tuple = ()

    rows = property(lambda self: len(self.rows_spec))

    @property
    def id(self):
        return f"fold-{self.name}-k{self.k}-cap{self.cap}"

    def inputs(self):
        """-> run_s, run_i [rows, k]; cand_s, cand_i [rows, cap] in ascending id order (guard values past a row's candidates);
        cand_len [rows] as handed over (row-wise possibly above cap); perm [rows][ncand]: the scrambled arrival order."""
        k, cap = self.k, self.cap
        R = self.rows
        run_s, run_i = np.empty((R, k), dtype=np.float32), np.empty((R, k), dtype=np.int64)
        cand_s, cand_i = np.full((R, cap), S_GUARD, dtype=np.float32), np.full((R, cap), I_GUARD, dtype=np.int64)
        cand_len, perms = np.empty(R, dtype=np.int32), []
        for r, (ncand, runs, real, clen) in enumerate(self.rows_spec):
            assert ncand <= cap
            rng = rng_of(self.id, r)
            run_s[r], run_i[r], cand_s[r, :ncand], cand_i[r, :ncand] = fold_row(rng, k, ncand, runs, real)
            cand_len[r] = ncand if clen is None else clen
            perms.append(rng.permutation(ncand))
        return run_s, run_i, cand_s, cand_i, cand_len, perms

    def expected(self):
        """-> new_s, new_i [rows, k], tau [rows], the unordered form's flag, the tie outcomes met."""
        run_s, run_i, cand_s, cand_i, cand_len, _ = self.inputs()
        ns, ni = np.empty_like(run_s), np.empty_like(run_i)
        flag, met = 0, set()
        for r in range(self.rows):
            n = min(int(cand_len[r]), self.cap)
            ns[r], ni[r], keys = fold_ref(run_s[r], run_i[r], cand_s[r, :n], cand_i[r, :n], self.k)
            f, m = tie_rule(keys, self.k)
            flag |= f
            met |= m
        return ns, ni, ns[:, -1].copy(), flag, met

    def branches(self):
        return {("fold", "ordered"), ("fold", "unordered")} | {("fold", "tie", t) for t in self.expected()[4] if ("fold", "tie", t) in BRANCHES}


def _fold_cases():
    out = []
    # plain folds: a few short tie runs, candidate counts that differ per row, an empty row, a full row, a length above cap (clamped)
    for k, cap in ((1, 5), (7, 40), (100, 300), (1000, 2000), (5056, 700)):
        few = ((min(3, k - 1), min(5, k + 1), "eq"),) if k > 1 else ()
        out.append(FoldCase("plain", k, cap, ((cap // 2, few, None, None), (0, (), None, None), (cap, few, None, cap + 9), (cap, (), None, None))))
    for k in (100, 1000):
        K = k + TIE_MARGIN
        t = lambda s: (("fold", "tie", s),)
        out += [
            FoldCase("closes63", k, 300, ((200, ((k - 1, K - 1, "eq"),), None, None),), t("closes-at-k+63:clear")),
            FoldCase("open64", k, 300, ((200, ((k - 1, K, "eq"),), None, None),), t("open-at-k+64:flag")),
            FoldCase("open70", k, 300, ((200, ((k - 1, K + 6, "eq"),), None, None),), t("open-at-k+64:flag")),
            FoldCase("behind", k, 700, ((650, ((k, k + 600, "eq"),), None, None),), t("behind-the-cut:clear")),
            FoldCase("end", k, 300, ((TIE_MARGIN, ((k - 1, K, "eq"),), None, None),), t("touches-the-end:clear")),
            FoldCase("zero", k, 300, ((200, ((k - 5, k + 5, "zero"),), None, None),)),
            FoldCase("nan", k, 300, ((200, ((0, 20, "nan"), (k - 3, k + 3, "eq")), None, None),)),
            FoldCase("short", k, 300, ((5, (), 10, None),), t("short-list:padding") if k + 5 - 15 <= TIE_RUN_MAX else ()),
        ]
    k = 1000
    out += [FoldCase("run512", k, 300, ((200, ((300, 812, "eq"),), None, None),), (("fold", "tie", "512-inside-k:clear"),)),
            FoldCase("run513", k, 300, ((200, ((300, 813, "eq"),), None, None),), (("fold", "tie", "513:flag"),)),
            FoldCase("run512cut", k, 300, ((200, ((k - 460, k + 52, "eq"),), None, None),)),
            FoldCase("run513cut", k, 300, ((200, ((k - 460, k + 53, "eq"),), None, None),), (("fold", "tie", "513:flag"),)),
            FoldCase("nan512", k, 300, ((200, ((0, 512, "nan"),), None, None),)), FoldCase("zero513", k, 300, ((200, ((100, 613, "zero"),), None, None),))]
    return out


FOLD_CASES = _fold_cases()


# ---- merge -------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class MergeCase:
    G: int
    rows: int
    k: int
    empty: tuple = ()            # shards that are all padding

    @property
    def id(self):
        return f"merge-G{self.G}-rows{self.rows}-k{self.k}" + ("-empty" + "".join(map(str, self.empty)) if self.empty else "")

    def inputs(self):
        """[G, rows, k] lists, each (score desc, id asc), scores from few values (ties inside and between shards), shard g's ids below
        shard g + 1's, a (-inf, -1) tail of varying length, NaN and +-0 entries."""
        rng = rng_of(self.id)
        G, rows, k = self.G, self.rows, self.k
        s, i = np.full((G, rows, k), -np.inf, dtype=np.float32), np.full((G, rows, k), -1, dtype=np.int64)
        for g in range(G):
            for r in range(rows):
                m = 0 if g in self.empty else k if (g + r) % 3 else max(k - 1 - (7 * g + r) % 5, 0)
                v = (rng.integers(-4, 5, m) / 2.0).astype(np.float32)
                v[rng.random(m) < 0.02] = np.nan
                z = np.flatnonzero(v == 0)
                v[z[::2]] = -0.0
                ids = ID_BASE + g * 4 * k + np.sort(rng.choice(4 * k, m, replace=False)).astype(np.int64)
                o = order_desc(v, ids)
                s[g, r, :m], i[g, r, :m] = v[o], ids[o]
        return s, i

    def branches(self):
        return {("merge", "at-limit")} if self.G * self.k == SORT_ROW_F32 else set()


MERGE_CASES = [MergeCase(1, 3, 100), MergeCase(2, 3, 100), MergeCase(8, 3, 100), MergeCase(8, 2, 1), MergeCase(2, 2, 7, empty=(0,)), MergeCase(8, 2, 50, empty=(0, 3, 7)),
               MergeCase(2, 1, 5, empty=(0, 1)), MergeCase(8, 2, 4480), MergeCase(2, 1, 17920), MergeCase(1, 1, 35840)]
MERGE_REFUSED = [(1, 35841), (3, 11947), (8, 4481)]       # G * k > 35,840


# ---- select ------------------------------------------------------------------------------------------------------------------------------
def select_inst(n):
    return "256x4" if n <= 1024 else "256x16" if n <= 4096 else "1024x16" if n <= 16384 else "1024x28"


def select_sim(keys, k, cap):
    """topk_select_kernel's threshold search over the listed documents' keys -> (candidates, the outcomes met)."""
    keys = np.asarray(keys, dtype=np.uint64)
    total = len(keys)
    need = min(k, total)
    if total == 0:
        return 0, {"total<=cap"}
    tau, met = int(keys.max()), set()
    if total > cap:
        lo, hi = int(keys.min()), int(keys.max())
        while lo < hi:
            mid = lo + ((hi - lo) >> 1)
            c = int((keys <= mid).sum())
            if c < need:
                lo = mid + 1
            else:
                hi = tau = mid
                if c <= cap:
                    met.add("bisect-early")
                    if c == cap:
                        met.add("bisect-early-at-cap")
                    break
        if lo >= hi:
            tau = hi
    else:
        met.add("total<=cap")
    count = int((keys <= tau).sum()) if need else 0
    if count > cap:
        met.add("tie-overflow")
    return count, met


SELECT_K, SELECT_CAP = 10, 50
OPS_PLANE_PAD = 64                            # ops.select_topk rounds a given cap up to a whole candidate-plane row (the GPU file checks it)
SELECT_ROWS = ("random", "ties-at-cap", "few-listed", "none-listed", "special")


def select_row(kind, N, dtype, rng, over=False, cap=SELECT_CAP):
    """-> (scores [N], pos [N] int32): random: normal scores (float64: distinct values that round to equal float32 keys) with NaN, +-inf
    and +-0 entries, 70 % listed;
    ties-at-cap: nine best, then a run of cap - k + 1 equal scores at the k-th place (one more with `over`), the rest below;
    stops-at-cap: distinct scores for which the bisection's first count in [k, cap] is cap itself; few-listed: k - 3 listed documents; none-listed; special: -inf, NaN and +-0 scores among few values."""
    k = SELECT_K
    x = rng.normal(0, 1, N).astype(np.float32).astype(dtype)
    listed = rng.random(N) < 0.7
    if kind == "random":
        if dtype == np.float64:
            x = np.round(x, 2).astype(np.float32).astype(np.float64) + 1e-12 * rng.normal(0, 1, N)
        for v in (np.nan, -np.inf, 0.0, -0.0, np.inf):        # NaN (key 0: the bisection starts there), -inf, a +-0 pair, +inf
            x[rng.integers(0, N, 2)] = v
    elif kind == "stops-at-cap":
        listed[:] = True
        for t in range(4000):                                 # distinct scores whose first midpoint with >= k keys below it has exactly cap
            x = rng_of("stops-at-cap", N, t).normal(0, 1, N).astype(np.float32)
            if len(np.unique(x)) == N and select_sim(desc_key(x), k, cap) == (cap, {"bisect-early", "bisect-early-at-cap"}):
                break
        else:
            raise AssertionError("no row stops the bisection at exactly cap")
        x = x.astype(dtype)
    elif kind == "ties-at-cap":
        listed[:] = True
        run = cap - k + 1 + int(over)
        o = rng.permutation(N)
        x[o] = -1.0 - np.arange(N) / 8.0
        x[o[: k - 1]] = 5.0 + np.arange(min(k - 1, N))[: len(o[: k - 1])]
        x[o[k - 1: k - 1 + run]] = 2.0
    elif kind == "few-listed":
        listed[:] = False
        listed[rng.permutation(N)[: k - 3]] = True
    elif kind == "none-listed":
        listed[:] = False
    else:
        assert kind == "special"
        x = (rng.integers(-2, 3, N) / 2.0).astype(dtype)
        z = np.flatnonzero(x == 0)
        x[z[::2]] = -0.0
        x[rng.random(N) < 0.2] = -np.inf
        x[rng.random(N) < 0.01] = np.nan
        x[N // 2] = np.nan
        if int(listed.sum()) > cap:                       # few values: keep the listed set small enough that total <= cap decides
            listed[np.flatnonzero(listed)[cap - 5:]] = False
    pos = np.full(N, -1, dtype=np.int32)
    idx = np.flatnonzero(listed)
    pos[idx[rng.permutation(len(idx))]] = np.arange(len(idx), dtype=np.int32)
    return x, pos


@dataclasses.dataclass(frozen=True)
class SelectCase:
    N: int
    bits: int
    kinds: tuple = SELECT_ROWS
    over: bool = False           # the tie run is one too long for cap: the raw entry flags it (ops.select_topk: None if too long for eff_cap)
    pos_none: bool = False       # every column listed at its own position
    cap: int = SELECT_CAP

    eff_cap = property(lambda self: -(-self.cap // OPS_PLANE_PAD) * OPS_PLANE_PAD)      # the cap ops.select_topk hands the kernel

    dtype = property(lambda self: np.float32 if self.bits == 32 else np.float64)
    rows = property(lambda self: len(self.kinds))

    @property
    def id(self):
        return f"select-N{self.N}-f{self.bits}" + ("" if self.kinds[0] == "random" else "-" + self.kinds[0]) + ("-over" if self.over else "") + ("-posnone" if self.pos_none else "") + \
            (f"-cap{self.cap}" if self.cap != SELECT_CAP else "")

    def inputs(self):
        rows = [select_row(kind, self.N, self.dtype, rng_of(self.id, r), self.over, self.cap) for r, kind in enumerate(self.kinds)]
        x, pos = np.stack([a for a, _ in rows]), np.stack([p for _, p in rows])
        return x, (None if self.pos_none else pos)

    def sims(self, cap=None):
        cap = self.cap if cap is None else cap
        x, pos = self.inputs()
        out = []
        for r in range(self.rows):
            listed = np.ones(self.N, dtype=bool) if pos is None else pos[r] >= 0
            out.append(select_sim(desc_key(x[r, listed].astype(np.float32)), SELECT_K, cap))
        return out

    def branches(self):
        hit = {("select", select_inst(self.N), self.bits)}
        for _, met in self.sims():
            hit |= {("select", m) for m in met}
        return hit


def select_ref(x, pos, k):
    """The first k of the stable descending sort of each row's listed documents taken in insertion order -> (cols [rows, k] int32 with
    -1 past a row's length, scores [rows, k] as the sort writes them, lens [rows])."""
    rows, N = x.shape
    cols, sc, lens = np.full((rows, k), -1, dtype=np.int32), np.full((rows, k), -np.inf, dtype=x.dtype), np.zeros(rows, dtype=np.int32)
    for r in range(rows):
        p = np.arange(N) if pos is None else pos[r]
        idx = np.flatnonzero(p >= 0)
        o = idx[order_desc(x[r, idx], p[idx])][:k]
        cols[r, : len(o)], sc[r, : len(o)], lens[r] = o, canon(x[r, o]), len(o)
    return cols, sc, lens


SELECT_N = (1, 1023, 1024, 1025, 4096, 4097, 16384, 16385, 28672)
SELECT_CASES = [SelectCase(N, b) for N in SELECT_N for b in (32, 64)] + \
               [SelectCase(N, b, kinds=("random", "ties-at-cap"), over=True) for N in (1025, 16385) for b in (32, 64)] + \
               [SelectCase(1023, b, kinds=("stops-at-cap", "random")) for b in (32, 64)] + \
               [SelectCase(N, b, kinds=("random", "ties-at-cap"), over=o, cap=64) for N in (1025, 16385) for b in (32, 64) for o in (False, True)] + \
               [SelectCase(N, b, kinds=("random", "ties-at-cap"), pos_none=True) for N in (1, 4097, 28672) for b in (32, 64)]


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
UPDATE_CASES = [UpdateCase(n, d) for d in UPDATE_DENSITIES for n in UPDATE_N]      # what the update-form tests of both files run
ALL_CASES = ROWS_CASES + ALL_FILTER_CASES + UPDATE_CASES + FOLD_CASES + MERGE_CASES + SELECT_CASES
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)


def landing(cases=None):
    """branch -> id of the first case that lands it, and the branches no case lands."""
    first = {}
    for c in cases or ALL_CASES:
        for b in c.branches():
            first.setdefault(b, c.id)
    return first, sorted((b for b in BRANCHES if b not in first), key=str)
