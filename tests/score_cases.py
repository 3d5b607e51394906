"""Inputs, float64 references and case tables of the exact score-GEMM tests (test_gpu_score_edges.py on the GPU, test_score_cases_cpu.py
without one).  numpy only; not collected by pytest.

Exact inputs.  Operand entries are multiples of 1/4 in [-2, 2]: a product is a multiple of 1/16 of magnitude <= 4 and a partial sum of up
to 196 of them a multiple of 1/16 below 2^10 -- 14 significant bits, exact in fp32 IN ANY ORDER.  On such inputs csrc/score.hip has no
rounding to hide behind: the score plane, the filter's candidate scores and the SPLADE logits must equal the float64 product bit for bit
(test_score_cases_cpu.py asserts `ref == ref.astype(float32)` for every case, so the exactness does not rest on this paragraph).
The operands are views into larger buffers (`framed`): the row stride exceeds d with NaN behind every row, and NaN "ghost" rows lie
before and after the rows of the problem -- a read past d, or of a row outside the problem that reaches a stored score, turns it into NaN.

Which branches a case lands is not restated from launch_gemm: `plan` asks the library (fz_dot_scores_plan, the function the launcher
itself runs, host only), `tiles_of` follows the kernel's own id -> tile map over that plan, and `branches_of` names what was met.  BRANCHES
lists every branch that the union of the cases must land."""
import ctypes
import dataclasses
import zlib

import numpy as np

EPI_STORE, EPI_FILTER, EPI_SPLADE = 0, 1, 2
EPI_NAME = {EPI_STORE: "store", EPI_FILTER: "filter", EPI_SPLADE: "splade"}
PLAN_FIELDS = ("slab_rows", "slab_row0", "rows", "QB", "TN", "full", "halves", "tail_ids", "tail_row0", "tail_rows", "cover7", "nP", "nQ",
               "grid", "ragged", "slots")
SENTINEL = np.float32(-12345.0)      # no exact score: |score| <= 196 * 4
ID_BASE = 3 << 31
CPU_CUS = 256                        # an MI355X; the GPU tests pass the device's own count


# ---- the plan, from the library ------------------------------------------------------------------------------------------------------
def plan_status(Q, N, d, epi, cus, out=True):
    from fusion_amd import _lib
    buf = (ctypes.c_int32 * len(PLAN_FIELDS))(*([-1] * len(PLAN_FIELDS)))
    rc = _lib.lib().fz_dot_scores_plan(Q, N, d, epi, cus, buf if out else None)
    return rc, list(buf)


def plan(Q, N, d, epi, cus):
    rc, f = plan_status(Q, N, d, epi, cus)
    assert rc == 0, (Q, N, d, epi, cus, rc)
    return dict(zip(PLAN_FIELDS, f))


def tiles_of(p):
    """The device side of a plan: (workgroup, kind, row0, col0, height, width) of every tile id in the order each workgroup visits them
    (dot_scores_kernel's three streams and gemm_stream's decode, cover7's two shapes).  An id of the XCD padding has kind "pad-..."."""
    out = []
    if p["cover7"]:
        out += [(b, "c7-128x192", 0, b * 192, 128, 192) for b in range(p["nP"])]
        out += [(p["nP"] + b, "c7-96x256", 128, b * 256, 96, 256) for b in range(p["nQ"])]
        return out
    G, full, TN, QB = p["grid"], p["full"], p["TN"], p["QB"]

    def whole(wg, b, kind, half):
        x, idx = b & 7, b >> 3
        dt = (idx // QB) * 8 + x
        out.append((wg, kind if dt < TN else "pad-" + kind, (idx % QB) * 128, dt * 128 + half * 64, 128, 128 if kind == "128x128" else 64))

    tail_kind = ("slab" if p["slab_rows"] else "") + f"{p['tail_rows']}x128"
    for wg in range(G):
        for b in range(wg, full, G):
            whole(wg, b, "128x128", 0)
        if wg < p["halves"]:
            whole(wg, full + ((wg >> 4) << 3 | (wg & 7)), "128x64", (wg >> 3) & 1)
        if p["tail_ids"]:
            t = wg
            if t < full:
                t += -(-(full - t) // G) * G
            for b in range(t - full, p["tail_ids"], G):
                out.append((wg, tail_kind if b < TN else "pad-" + tail_kind, p["tail_row0"], b * 128, p["tail_rows"], 128))
    return out


def cover_count(p, Q, N):
    """How often each cell of [Q, N] is stored by the tiles of the plan (the slab rows ride in every real tail tile)."""
    cnt = np.zeros((Q, N), dtype=np.int8)
    for _, kind, r0, c0, h, w in tiles_of(p):
        if kind.startswith("pad-"):
            continue
        cnt[r0: min(r0 + h, p["rows"]), c0: min(c0 + w, N)] += 1
        if kind.startswith("slab"):
            cnt[p["slab_row0"]: p["slab_row0"] + p["slab_rows"], c0: min(c0 + w, N)] += 1
    return cnt


# ---- the branches --------------------------------------------------------------------------------------------------------------------
KINDS = {"store": ("128x128", "128x64", "32x128", "64x128", "96x128", "slab64x128", "c7-128x192", "c7-96x256"),
         "filter": ("128x128", "128x64", "32x128", "64x128", "96x128"),
         "splade": ("128x128", "128x64")}
ROW_CLASSES = {"store": ("tail32", "tail64", "tail96", "slab1", "slab2", "slab3", "slab4", "padded", "whole"),
               "filter": ("tail32", "tail64", "tail96", "padded", "whole")}

BRANCHES = {
    **{("kernel", k, rg): "dot_scores_kernel<RAGGED, EPI> / dot_scores_cover7_kernel<RAGGED>" for k in ("store", "filter", "splade", "cover7") for rg in (False, True)},
    **{("rows", e, cls, behind): "height class of the last query block, alone / behind whole 128-row blocks" for e, cs in ROW_CLASSES.items() for cls in cs
       for behind in (False, True)},
    ("rows", "store", "cover7"): "193 .. 224 rows on the 7-row-block cover",
    ("rows", "splade", "padded"): "SPLADE: a last block of any height is padded to 128 rows", ("rows", "splade", "whole"): "T % 128 == 0",
    ("slab-refused", "filter"): "Q % 128 in 65 .. 68 outside the store form: a 96-row tail",
    ("cover7", "largest-N"): "nP + nQ <= cus holds at N and fails at N + 1", ("cover7", "first-N-refused"): "nP + nQ > cus at N, not at N - 1",
    **{("round", k): "how the ids fill the resident slots" for k in ("single", "exactly-full", "multi-last-over-half", "halves", "whole-then-tail")},
    **{("halves", e, k): "the halved last round: a half tile inside the matrix / on its edge / XCD padding ids inside the round (TN % 8 != 0)"
       for e in EPI_NAME.values() for k in ("whole", "edge", "pad-ids")},
    **{("halves", e, "starts-past-N"): "the last corpus tile holds <= 64 rows: its second half starts past the last corpus row" for e in ("store", "splade")},
    **{("pad-ids", k): "XCD padding ids decode to nothing" for k in ("whole", "tail")},
    **{("kloop", k): "tile loop: plain pairs of k-tiles / the edge pair / the last pair" for k in ("plain", "edge-pair", "last-pair")},
    **{("KT", k): "k-tiles per tile (6: six or more)" for k in (2, 4, 6)},
    ("KT2-both-on-edge",): "d < 64: both k-tiles of the only pair reach past d or are partial",
    **{("ktile", k): "a k-tile of the last two against d" for k in ("whole", "partial", "past-d")},
    **{("epi", e, kind, k): "epilogue of a tile inside the matrix / reaching past its last row or column" for e, ks in KINDS.items() for kind in ks
       for k in ("whole", "edge")},
}


def branches_of(c, cus):
    """The branches case c lands on a device of `cus` compute units."""
    p = plan(c.Q, c.N, c.d, c.epi, cus)
    e = EPI_NAME[c.epi]
    hit = {("kernel", "cover7" if p["cover7"] else e, bool(p["ragged"]))}
    KT = 2 * (-(-c.d // 64))
    hit |= {("KT", min(KT, 6)), ("kloop", "last-pair")}
    if KT >= 4:
        hit.add(("kloop", "edge-pair"))
    if KT >= 6:
        hit.add(("kloop", "plain"))
    for j in (KT - 2, KT - 1):
        hit.add(("ktile", "whole" if 32 * j + 32 <= c.d else "partial" if 32 * j < c.d else "past-d"))
    if KT == 2 and c.d < 64 and c.d != 32:
        hit.add(("KT2-both-on-edge",))
    rem = c.Q % 128
    if c.epi == EPI_SPLADE:
        hit.add(("rows", e, "padded" if rem else "whole"))
    elif p["cover7"]:
        hit.add(("rows", e, "cover7"))
    else:
        if p["slab_rows"]:
            cls, behind = f"slab{p['slab_rows']}", p["QB"] > 0
        elif p["tail_rows"]:
            cls, behind = f"tail{p['tail_rows']}", p["QB"] > 0
        else:
            cls, behind = ("padded" if rem else "whole"), p["QB"] > 1
        hit.add(("rows", e, cls, behind))
        if c.epi == EPI_FILTER and 64 < rem <= 68:
            hit.add(("slab-refused", e))
    if c.epi == EPI_STORE and 196 < c.Q <= 224:
        if p["cover7"] and not plan(c.Q, c.N + 1, c.d, c.epi, cus)["cover7"]:
            hit.add(("cover7", "largest-N"))
        if not p["cover7"] and plan(c.Q, c.N - 1, c.d, c.epi, cus)["cover7"]:
            hit.add(("cover7", "first-N-refused"))
    tiles = tiles_of(p)
    if not p["cover7"]:
        ids = p["full"] + p["halves"] // 2 + p["tail_ids"]
        if ids <= p["slots"]:
            hit.add(("round", "exactly-full" if ids == p["slots"] and not p["tail_ids"] else "single"))
        elif not p["halves"] and not p["tail_ids"] and p["full"] % p["slots"] > p["slots"] // 2:
            hit.add(("round", "multi-last-over-half"))
        if p["halves"]:
            hit.add(("round", "halves"))
        seen_whole = set()
        for wg, kind, r0, c0, h, w in tiles:
            if kind == "128x128":
                seen_whole.add(wg)
            elif kind == "pad-128x128":
                hit.add(("pad-ids", "whole"))
            elif kind == "pad-128x64":
                hit.add(("halves", e, "pad-ids"))
            elif kind.startswith("pad-"):
                hit.add(("pad-ids", "tail"))
            elif kind == "128x64":
                hit.add(("halves", e, "whole" if r0 + h <= p["rows"] and c0 + w <= c.N else "edge"))
                if c0 >= c.N:
                    hit.add(("halves", e, "starts-past-N"))
            elif wg in seen_whole:
                hit.add(("round", "whole-then-tail"))
    for _, kind, r0, c0, h, w in tiles:
        if not kind.startswith("pad-"):
            hit.add(("epi", e, kind, "whole" if r0 + h <= p["rows"] and c0 + w <= c.N else "edge"))
    return hit


def landing(cases, cus):
    """branch -> id of the first case that lands it, and the branches no case lands."""
    first = {}
    for c in cases:
        for b in branches_of(c, cus):
            first.setdefault(b, c.id)
    return first, sorted((b for b in BRANCHES if b not in first), key=str)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def grid(rng, rows, d, lim=8):
    """[rows, d] multiples of 1/4 in [-lim / 4, lim / 4]."""
    return rng.integers(-lim, lim + 1, (rows, d)).astype(np.float64) / 4.0


def framed(a, before=2, after=3, pad=4, fill=np.nan, dtype=np.float32):
    """a [rows, n] inside a larger buffer: `before` / `after` rows and `pad` columns of `fill` around it.  -> (buffer, row slice, n)."""
    rows, n = a.shape
    buf = np.full((before + rows + after, n + pad), fill, dtype=dtype)
    buf[before: before + rows, :n] = a
    return buf, slice(before, before + rows), n


def exact_f32(ref):
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref, equal_nan=True), "the float64 reference is not exactly representable in float32"
    return r32


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    epi: int
    Q: int
    N: int
    d: int
    claims: tuple = ()
    nan: str = ""                # filter: "corpus" (one corpus row holds a NaN), "query" (the last query row does), "" (none)
    tau: str = "mixed"           # filter: thresholds "mixed" per query (tie value / row maximum / -inf / +inf) or "rank40"

    @property
    def id(self):
        return f"{self.name}-{EPI_NAME[self.epi]}-Q{self.Q}-N{self.N}-d{self.d}" + (f"-nan_{self.nan}" if self.nan else "")

    def rng(self):
        return np.random.default_rng(zlib.crc32(self.id.encode()))

    def inputs(self):
        """-> (A [Q, d], B [N, d]) float64 on the grid; the NaN variants carry one NaN element."""
        rng = self.rng()
        A, B = grid(rng, self.Q, self.d), grid(rng, self.N, self.d)
        if self.nan == "corpus":
            B[(self.N * 2) // 3, self.d - 1] = np.nan
        if self.nan == "query":
            A[self.Q - 1, 0] = np.nan
        return A, B

    def ref(self, A, B):
        with np.errstate(invalid="ignore"):
            r = A @ B.T
        if self.nan:                 # (a NaN operand element: 0 * NaN is NaN too -- the whole row / column of the plane)
            r[np.isnan(A).any(axis=1), :] = np.nan
            r[:, np.isnan(B).any(axis=1)] = np.nan
        return r

    def thresholds(self, ref):
        """tau [Q] float32 from the float64 reference."""
        Q, N = ref.shape
        if self.tau == "rank40":
            return np.sort(ref, axis=1)[:, -min(40, N)].astype(np.float32)
        tau = np.empty(Q, dtype=np.float32)
        shift = zlib.crc32(self.id.encode()) % 4
        for q in range(Q):
            row = ref[q][~np.isnan(ref[q])]
            kind = (q + shift) % 4 if Q > 1 else 0
            if kind == 3 or row.size == 0:
                tau[q] = np.inf
            elif kind == 2:
                tau[q] = -np.inf
            elif kind == 1:
                tau[q] = row.max()                     # nothing enters
            else:                                      # a value that several of the row's scores equal (N >= 127), near its upper quartile
                v, n = np.unique(row, return_counts=True)
                tied = v[n >= 2] if (n >= 2).any() else v
                tau[q] = tied[np.argmin(np.abs(tied - np.quantile(row, 0.75)))]
        return tau

    @staticmethod
    def expected(ref, tau):
        """[Q, N] bool: document j enters query q's candidates iff !(ref[q, j] <= tau[q]) (greater, or NaN)."""
        with np.errstate(invalid="ignore"):
            return ~(ref <= tau.astype(np.float64)[:, None])


def unit_rows(rng, rows, d):
    x = rng.normal(0, 1, (rows, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- store and filter cases ------------------------------------------------------------------------------------------------------------
ROWS_ALONE = (1, 32, 33, 64, 65, 66, 67, 68, 69, 96, 97, 127, 128, 129, 160, 192, 193, 194, 195, 196, 197, 224, 225, 257)
ROWS_BEHIND = (256 + 33, 256 + 64, 321, 322, 323, 324, 325, 352, 353, 383, 384)      # the classes that 193 .. 224 (the cover) hide, behind two blocks
COL_EDGES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1283)
K_EDGES = (4, 28, 32, 36, 60, 64, 68, 124, 128, 132, 192, 196)
K_ROWS = (1, 33, 67, 96, 100, 128, 197, 257)      # one representative per row class: 32 / 64 / slab / 96 / padded / whole / cover / block + tail
COVER_LAST_N = 28032                              # at 256 CUs: ceil(N / 192) + ceil(N / 256) = 146 + 110; 28,033 needs 147 + 110

FILTER_ROWS = (1, 33, 64, 65, 96, 97, 128, 129, 160, 192, 193, 225, 257)
FILTER_COLS = (1, 127, 128, 129, 1283)
FILTER_K = (4, 36, 64, 68, 132)
FILTER_NAN_ROWS = (33, 97, 129)


def _cases():
    S, F = EPI_STORE, EPI_FILTER
    out = []
    for Q in ROWS_ALONE + ROWS_BEHIND:
        out.append(Case("rows", S, Q, 257, 36))
    for N in COL_EDGES:
        for Q in (67, 129, 197):
            out.append(Case("cols", S, Q, N, 36))
    for d in K_EDGES:
        for Q in K_ROWS:
            out.append(Case("k", S, Q, 193, d))
    # the round structure, d = 8 (256 CUs: 512 resident slots)
    out.append(Case("round", S, 128, 1283, 8, (("round", "single"),)))
    out.append(Case("round", S, 256, 32768, 8, (("round", "exactly-full"),)))
    out.append(Case("round", S, 384, 33000, 8, (("round", "multi-last-over-half"), ("pad-ids", "whole"))))
    out.append(Case("round", S, 256, 33000, 8, (("round", "halves"), ("halves", "store", "pad-ids"), ("halves", "store", "whole"), ("halves", "store", "edge"),
                                                ("epi", "store", "128x64", "whole"), ("epi", "store", "128x64", "edge"))))
    out.append(Case("round", S, 256, 32960, 8, (("round", "halves"), ("halves", "store", "starts-past-N"))))
    out.append(Case("round", S, 160, 33000, 8, (("round", "whole-then-tail"), ("pad-ids", "tail"))))
    # the cover's width limit; 195 rows (the issue's shape) ride as 192 + a slab and never take the cover, 197 and 224 do
    for Q in (195, 197, 224):
        out.append(Case("cover", S, Q, COVER_LAST_N, 8, (("cover7", "largest-N"),) if Q > 196 else (("rows", "store", "slab3", True),)))
        out.append(Case("cover", S, Q, COVER_LAST_N + 1, 8, (("cover7", "first-N-refused"),) if Q > 196 else (("rows", "store", "slab3", True),)))
    # the filter epilogue
    for Q in FILTER_ROWS:
        out.append(Case("rows", F, Q, 129, 36))
    for N in FILTER_COLS:
        for Q in (33, 129):
            out.append(Case("cols", F, Q, N, 36))
    for d in FILTER_K:
        for Q in (97, 160):
            out.append(Case("k", F, Q, 129, d))
    for Q in FILTER_NAN_ROWS:
        for N in (129, 1283):
            for nan in ("corpus", "query"):
                out.append(Case("nan", F, Q, N, 36, nan=nan))
    out.append(Case("round", F, 256, 33000, 8, (("round", "halves"), ("halves", "filter", "whole"), ("halves", "filter", "edge")), tau="rank40"))
    seen = set()
    return [c for c in out if not (c.id in seen or seen.add(c.id))]


CASES = _cases()
STORE_CASES = [c for c in CASES if c.epi == EPI_STORE]
FILTER_CASES = [c for c in CASES if c.epi == EPI_FILTER]
UNIT_SHAPE = (257, 33000, 64)        # the tile-independence pair: two whole blocks + a 32-row tail over more ids than slots


# ---- SPLADE ---------------------------------------------------------------------------------------------------------------------------
def splade_cuts(T):
    """cu_rows [nseq + 1] over T >= 701 packed rows.  Relative to the 128-row tile a cut falls on every offset 0 .. 128 (rows 0 .. 383:
    offset r sits in tile r % 3, the tile cuts 128, 256 and 384 are cuts too), there are one-row sequences, runs of two and three empty
    sequences at the start, in the middle and at the end, and one sequence (rows 390 .. 689) that spans three tiles."""
    assert T >= 701
    cuts = {128 * (r % 3) + r for r in range(128)} | {128, 256, 384, 390, 690} | {11, 150, 300} | set(range(768, T, 97))
    inner = sorted(c for c in cuts if 0 < c < T)
    cu = [0, 0, 0]
    for c in inner:
        cu += [c] * (4 if c == 256 else 3 if c == 128 else 1)
    return np.array(cu + [T, T, T], dtype=np.int32)


@dataclasses.dataclass(frozen=True)
class SpladeCase:
    T: int
    V: int
    d: int
    claims: tuple = ()
    epi: int = EPI_SPLADE

    @property
    def id(self):
        return f"splade-T{self.T}-V{self.V}-d{self.d}"

    Q = property(lambda self: self.T)
    N = property(lambda self: self.V)

    def window(self, r):
        return (r + np.arange(4)) % self.d      # the (at most) four non-zeros of row r: the positions cycle over all of [0, d)

    def inputs(self):
        """-> X [T, d], W [V, d], bias [V] float64, cu_rows int32, marks [(cut, row, column)].
        General X entries are +-1/4 or +-1/2, so a general logit is at most 4 * 1/2 + 2.  A MARKED (row, column) pair -- the row before and
        the row after a cut, each with a column of its own while the columns last -- has X[row] = +-1 on its window and W[column] equal to
        it there and 0 elsewhere: logit 4 + bias, the column's maximum, at least 1 above every other row less than 128 rows away (at d = 8 the
        8 windows x 16 sign patterns come round again after 128 marked rows: a row that far away may tie)."""
        T, V, d = self.T, self.V, self.d
        rng = np.random.default_rng(zlib.crc32(self.id.encode()))
        cu = splade_cuts(T)
        X = np.zeros((T, d))
        for r in range(T):
            w = self.window(r)[: int(rng.integers(1, 5))]
            X[r, w] = rng.choice([-0.5, -0.25, 0.25, 0.5], len(w))
        W, bias = grid(rng, V, d, lim=4), grid(rng, 1, V)[0]
        free = V - 2 if V >= 8 else V                          # the last two columns are the special ones below
        inner = sorted({int(c) for c in cu if 0 < c < T})
        first = zlib.crc32(self.id.encode()) % len(inner) if free < 2 * len(inner) else 0
        marks, v = [], 0
        for i in range(len(inner)):
            c = inner[(first + i) % len(inner)]
            for r in (c - 1, c):
                if v < free:
                    marks.append((c, r, v))
                    v += 1
        used = {}                                              # marked rows of one window take the 16 sign patterns in turn
        for r in sorted({r for _, r, _ in marks}):
            n = used[r % d] = used.get(r % d, -1) + 1
            X[r] = 0.0
            X[r, self.window(r)] = [1.0 if n >> j & 1 else -1.0 for j in range(4)]
        for _, r, v in marks:
            W[v] = 0.0
            W[v, self.window(r)] = X[r, self.window(r)]
        if V >= 8:
            W[V - 1] = rng.choice([-0.25, 0.25], d); bias[V - 1] = -2.0      # every logit negative: pools to exactly 0
            W[V - 2] = 0.0; bias[V - 2] = 0.25                               # only the bias lifts the column above 0
        return X, W, bias, cu, marks

    @staticmethod
    def logits(X, W, bias):
        return X @ W.T + bias[None, :]

    @staticmethod
    def pooled(logits, cu):
        """float64 reference: pool[s] = log1p(relu(max over the sequence's rows)), 0 for an empty sequence."""
        out = np.zeros((len(cu) - 1, logits.shape[1]))
        for s in range(len(cu) - 1):
            a, b = int(cu[s]), int(cu[s + 1])
            if b > a:
                out[s] = np.log1p(np.maximum(logits[a:b].max(axis=0), 0.0))
        return out


SPLADE_V = (1, 63, 64, 65, 127, 128, 129, 509)
SPLADE_D = (8, 36, 64, 68)
SPLADE_CASES = [SpladeCase(701, V, 36) for V in SPLADE_V] + [SpladeCase(701, 509, d) for d in SPLADE_D if d != 36] + \
               [SpladeCase(1024 + 61, 9000, 8, (("round", "halves"), ("halves", "splade", "whole"), ("halves", "splade", "edge"), ("halves", "splade", "pad-ids"),
                                                ("halves", "splade", "starts-past-N"),
                                                ("epi", "splade", "128x64", "whole"), ("epi", "splade", "128x64", "edge"))),
                SpladeCase(1024, 9100, 8, (("round", "halves"), ("rows", "splade", "whole")))]
ALL_CASES = CASES + SPLADE_CASES
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)
