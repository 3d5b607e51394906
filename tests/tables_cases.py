"""Restatements, designed inputs and the case table of the long-table fusion edge tests (test_gpu_tables_edges.py on the GPU,
test_tables_cases_cpu.py without one): csrc/tables.hip, percentile-rank / normal-curve-equivalent fusion with one system's quantile table
LDS-resident at a time.  numpy only; not collected by pytest.

No tolerance on the fused scores: `expected` is the operation itself -- per system the FIRST index of the minimum float32 distance
(`nearest_first`, hybrid.py:271-275), float32(k) / float32(P) or the value table's entry, times float32(w), summed in float32 in system
order from +0.0 -- and test_tables_cases_cpu.py holds it to the oracle's brute-force scan bit for bit.  NCE takes the kernel's OWN value
table (read back from the workspace at the offsets of the restated plan), so the comparison pins the index; the table itself is held to the
float64 formula separately.

Which branch a case lands is not claimed, it is computed from the restatements below: `plan` (bt_plan: padded lengths, bucket count,
value table in LDS or swapped over the table, workspace offsets), `search` (bt_prepare_kernel's bucket expression and bucket table,
bt_prepare_steps_kernel's probe count, the instantiation the fusion kernel's switch picks), `nearest_first(lengths=True)` (how far bt_plateau_start walks)
and `walk` (the persistent loop's advance(), with its carry).

Designed tables: tab[0] = 0.0 and tab[P - 1] = float(buckets) make the bucket expression floor(x), so a bucket's occupancy is placed entry
by entry: four DESIGNATED buckets of exactly m distinct entries (bucket 0, the top bucket -- it holds tab[P - 1] through the clamp -- one
whose first entry has an even table index and one whose first has an odd one, each between empty buckets) over a background that stays
below m.  Entries are multiples of 1/128 above the bucket's floor, so the midpoint of two neighbours is a float32 and ties exactly."""
import functools
import zlib

import numpy as np

# csrc/tables.hip
BT_T, BT_E4, BT_PIECE, BT_LEAD, BT_TAIL, BT_MAX_UNROLLED = 1024, 7, 256, 4, 40, 4
BT_COLS = BT_T * BT_E4 * 4                                  # 28,672 columns per item
BT_LDS_BUDGET, BT_HDR_BYTES = 160 * 1024 - 256, 256
BT_GRID = 256                                               # persistent workgroups at most
MAX_SYSTEMS = 8
NORMS = ("percentile-rank", "normal-curve-equivalent")
NCE_TOL = 1e-4                                              # the project's bound for this normalisation (test_gpu_tables.py, fuzz_gpu.NSF_TOL)
F32 = np.float32
INF = F32(np.inf)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def up(x):
    return np.nextafter(F32(x), INF)


def down(x):
    return np.nextafter(F32(x), -INF)


# ---- bt_plan ---------------------------------------------------------------------------------------------------------------------------
def plan(P, nce):
    """bt_plan -> None (no plan: fuse_nsf searches the tables in global memory) or dict(Ppad, tab_cap, lutb, lut_floats, val_in_lds,
    lds_bytes, sys_off [S + 1]); a system's block in the workspace is header | table [Ppad] | bucket table [lut_floats] | values [Ppad]."""
    P = [int(p) for p in P]
    if any(p <= 0 or p > 65535 for p in P):
        return None
    Ppad = [(BT_LEAD + p + BT_TAIL + BT_PIECE - 1) // BT_PIECE * BT_PIECE for p in P]
    cap = max(Ppad)
    lutb = 16384
    while lutb >= 2048:
        lf = ((lutb + 1) * 2 + BT_PIECE * 4 - 1) // (BT_PIECE * 4) * BT_PIECE
        if (cap + lf) * 4 <= BT_LDS_BUDGET:
            break
        lutb >>= 1
    else:
        return None
    val_in_lds = bool(nce) and (2 * cap + lf) * 4 <= BT_LDS_BUDGET
    off = [0]
    for pp in Ppad:
        off.append(off[-1] + BT_HDR_BYTES + pp * 4 + lf * 4 + (pp * 4 if nce else 0))
    return dict(Ppad=Ppad, tab_cap=cap, lutb=lutb, lut_floats=lf, val_in_lds=val_in_lds, lds_bytes=((2 if val_in_lds else 1) * cap + lf) * 4, sys_off=off)


def value_offset(pl, s):
    """Byte offset of system s's NCE value table in the workspace."""
    return pl["sys_off"][s] + BT_HDR_BYTES + pl["Ppad"][s] * 4 + pl["lut_floats"] * 4


def plan_threshold(pred, lo=1, hi=65535):
    """The largest P in [lo, hi] for which pred(plan) holds (pred is monotone: true up to a threshold)."""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


# ---- the bucket table --------------------------------------------------------------------------------------------------------------------
def inv_width(tab, lutb):
    tab = np.asarray(tab, dtype=np.float32)
    inv_w = F32(0.0)
    if len(tab) >= 2:
        with np.errstate(over="ignore"):
            d = F32(tab[-1] - tab[0])
            if d > 0 and d < INF:
                inv_w = F32(lutb) / d
        if not inv_w < INF:
            inv_w = F32(0.0)
    return inv_w


def bucket(x, lo, inv_w, lutb):
    """bt_bucket: (int)clamp((x - lo) * inv_w, 0, lutb - 1) in float32; NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, dtype=np.float32) - F32(lo)) * F32(inv_w)
    t = np.where(np.isnan(t), F32(0.0), np.clip(t, F32(0.0), F32(lutb - 1)))
    return t.astype(np.int64)


def search(tab, lutb):
    """The bucket table of one system and what bt_prepare_steps_kernel derives from it -> dict(inv_w, lut [lutb + 1], fullest_bucket,
    probes, inst): lut[b] = first k whose bucket is >= b; probes = the smallest count with 2^probes - 1 >= (m + 1) // 2 pairs;
    inst = the bt_lookup instantiation the switch picks (1 .. 4 unrolled, "loop")."""
    tab = np.asarray(tab, dtype=np.float32)
    inv_w = inv_width(tab, lutb)
    bk = bucket(tab, tab[0], inv_w, lutb)
    assert np.all(np.diff(bk) >= 0)
    lut = np.searchsorted(bk, np.arange(lutb + 1), side="left")
    m = int(np.diff(lut).max())
    pairs = (m + 1) // 2
    steps = 0
    while (1 << steps) - 1 < pairs:
        steps += 1
    inst = "loop" if steps > BT_MAX_UNROLLED else max(steps, 1)
    return dict(inv_w=inv_w, lut=lut, bk=bk, fullest_bucket=m, probes=steps, inst=inst)


def fullest(tab, lutb):
    """The fullest buckets of a table: [(bucket, first table index, entries)]."""
    sr = search(tab, lutb)
    cnt = np.diff(sr["lut"])
    return [(int(b), int(sr["lut"][b]), int(cnt[b])) for b in np.flatnonzero(cnt == cnt.max())]


# ---- the nearest entry -------------------------------------------------------------------------------------------------------------------
def _dist(tab, k, x):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(tab[k] - x)


def nearest_first(tab, x, lengths=False):
    """The FIRST index of the minimum of the float32 distances |tab - x| over an ascending table (hybrid.py:271-275); 0 for NaN and
    +-inf.  Rounding is monotone, so the minimum is taken at the last entry <= x or the first one above it, and the entries at that
    distance are a run of neighbours: its first index is found by bisection, on the scores that have such a run only.
    lengths=True: also how many entries AT OR BELOW x share the minimum (0 when the nearest entry lies above x)."""
    tab = np.asarray(tab, dtype=np.float32)
    shape = np.shape(x)
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    P = len(tab)
    fin = np.isfinite(x)
    xs = np.where(fin, x, tab[0])
    i = np.searchsorted(tab, xs, side="right") - 1             # last entry <= x, or -1
    j = i + 1
    dl = np.where(i >= 0, _dist(tab, np.maximum(i, 0), xs), INF)
    dh = np.where(j < P, _dist(tab, np.minimum(j, P - 1), xs), INF)
    left = dl <= dh
    best = np.where(left, i, j)
    run = np.zeros(len(x), dtype=np.int64)
    run[left] = 1
    walk = np.flatnonzero(left & (i > 0))
    walk = walk[_dist(tab, i[walk] - 1, xs[walk]) == dl[walk]]
    if len(walk):                                              # a run of equal distances ends at i: bisect for its first index
        lo, hi = np.zeros(len(walk), dtype=np.int64), i[walk] - 1
        xw, dw = xs[walk], dl[walk]
        while np.any(lo < hi):
            mid = (lo + hi) >> 1
            open_, on = lo < hi, _dist(tab, mid, xw) == dw
            hi = np.where(open_ & on, mid, hi)
            lo = np.where(open_ & ~on, mid + 1, lo)
        run[walk] = i[walk] - hi + 1
        best[walk] = hi
    best = np.where(fin, best, 0).astype(np.int64)
    if lengths:
        return best.reshape(shape), np.where(fin, run, 0).reshape(shape)
    return best.reshape(shape)


def nearest_scan(tab, x):
    """The definition, literally (small inputs): np.argmin returns the first minimum; an all-NaN column gives 0."""
    tab = np.asarray(tab, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(tab[:, None] - np.asarray(x, dtype=np.float32).reshape(1, -1))
    d = np.where(np.isnan(d), INF, d)
    return np.argmin(d, axis=0).reshape(np.shape(x))


def _nce_arg(P):
    """The float32 argument the reference hands the inverse error function (hybrid.py:275-277 on a float32 tensor): y = 2 ((k / P) / 100) - 1."""
    return F32(2.0) * ((np.arange(P, dtype=np.float32) / F32(P)) / F32(100.0)) - F32(1.0)


def _erfinv_sqrt2(y):
    """erfinv(y) sqrt(2) = the standard normal quantile of (1 + y) / 2 in float64 ((1 + y) / 2 is exact for a float32 y); -inf at y = -1."""
    y = np.asarray(y, dtype=np.float64)
    try:
        from scipy.special import erfinv
        return erfinv(y) * 1.4142135623730951
    except ImportError:                                         # statistics.NormalDist.inv_cdf: Wichura's AS241, ~1e-16
        from statistics import NormalDist
        nd = NormalDist()
        return np.array([-np.inf if v <= -1.0 else nd.inv_cdf((float(v) + 1.0) / 2.0) for v in y])


def nce_values(P):
    """The NCE value of every table index by the float64 formula erfinv(2 (k / P) / 100 - 1) sqrt(2) 21.06 + 50, taken at the argument the
    operation itself forms (`_nce_arg`: the quotient, the / 100 and the 2 p - 1 are float32 steps of the reference, hybrid.py:275-277, and
    part of what is computed; near y = -1 the quantile is steep enough that the same formula on a float64 argument lies up to 1.5e-3 away
    at k = 1 of a 10,001-entry table -- a property of the operation, not of a kernel); V[0] = -inf."""
    return _erfinv_sqrt2(_nce_arg(P)) * 21.06 + 50.0


def nce_values_f32(P):
    """The value table as tables.hip's expression rounds it (float32 affine steps around a float64 erfinv): what the CPU file feeds
    `expected` where no kernel is there to read the table from.  Not bit-exact to the device's erfinv; the GPU file never uses it."""
    return _erfinv_sqrt2(_nce_arg(P)).astype(np.float32) * F32(21.06) + F32(50.0)


def expected(planes, ranks, w, norm, tabs, V=None):
    """The fused plane: per system k = nearest_first, value = float32(k) / float32(P) (percentile-rank) or V[s][k] (NCE),
    prod = float32(value * float32(w_s)), summed in float32 in system order from +0.0; a system that does not list a document
    (rank < 0) adds nothing; a document no system lists gets -inf.  (tables.hip: the arithmetic behind bt_quot and the NCE gather.)"""
    assert norm in NORMS and (norm == NORMS[0]) == (V is None)
    Q, N = planes[0].shape
    acc = np.zeros((Q, N), dtype=np.float32)
    present = np.zeros((Q, N), dtype=bool)
    for s, (x, tab) in enumerate(zip(planes, tabs)):
        k = nearest_first(tab, x)
        val = k.astype(np.float32) / F32(len(tab)) if V is None else np.asarray(V[s], dtype=np.float32)[k]
        with np.errstate(invalid="ignore", over="ignore"):
            prod = (val * F32(w[s])).astype(np.float32)
            listed = np.ones((Q, N), dtype=bool) if ranks is None or ranks[s] is None else ranks[s] >= 0
            acc = np.where(listed, acc + prod, acc).astype(np.float32)
        present |= listed
    return np.where(present, acc, -INF).astype(np.float32)


# ---- the persistent walk -----------------------------------------------------------------------------------------------------------------
def walk(Q, N):
    """fuse_nsf_bigtab_kernel's item walk: workgroup g of grid = min(items, 256) takes items g, g + grid, ... and steps (q, c) by
    (grid / chunks, grid % chunks) with a carry -> dict(items, chunks, grid, carries); asserts (q, c) == divmod(item, chunks) throughout."""
    chunks = (N + BT_COLS - 1) // BT_COLS
    items = Q * chunks
    grid = min(items, BT_GRID)
    dq, dc = divmod(grid, chunks)
    carries = 0
    for g in range(grid):
        q, c = divmod(g, chunks)
        for it in range(g, items, grid):
            assert (q, c) == divmod(it, chunks), (Q, N, g, it)
            q, c = q + dq, c + dc
            if c >= chunks:
                c -= chunks
                q += 1
                carries += it + grid < items                    # a carry whose result is used: another item follows
    return dict(items=items, chunks=chunks, grid=grid, carries=int(carries))


# ---- designed tables -----------------------------------------------------------------------------------------------------------------------
def _fill(b, n, rng, first=None):
    """n distinct float32 entries of bucket b: b + multiples of 1/128 (`first`: one of them, given)."""
    assert 0 <= n <= 128
    f = np.sort(rng.choice(np.arange(1, 128), n - (first is not None), replace=False)) if n else np.zeros(0, dtype=np.int64)
    e = F32(b) + f.astype(np.float32) / F32(128.0)
    return e if first is None else np.sort(np.concatenate([[F32(first)], e]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def designed_table(P, m, lutb=16384, key=0):
    """-> (tab [P] float32 ascending, designated {name: bucket}): tab[0] = 0.0, tab[P - 1] = lutb, so bucket(x) = floor(x).  Buckets
    "zero" (0), "top" (lutb - 1, holds tab[P - 1] through the clamp), "even" and "odd" (first entry at an even / odd table index) hold exactly
    m distinct entries between empty neighbours; "tight" is a second bucket with an odd first index whose upper neighbour holds one
    entry, AT its floor -- the nearest entry of nextafter(b + 1, 0), and the one a search that counted a pair too few cannot reach (between
    empty neighbours the four entries bt_lookup reads around its result make up for one missing pair).  Every other bucket holds fewer
    than m (at most one where P allows it)."""
    rng = rng_of("designed", P, m, lutb, key)
    bE, bT, bO = lutb // 3, lutb // 2, 2 * lutb // 3
    zones = [range(2, bE - 1), range(bE + 2, bT - 1), range(bT + 3, bO - 1), range(bO + 2, lutb - 2)]
    n_bg = P - 5 * m - 1
    assert n_bg >= 0
    total = sum(len(z) for z in zones)
    n = [n_bg * len(z) // total for z in zones]
    n[0] += (m + n[0]) % 2                                      # entries before bucket bE: m + n[0], even
    n[1] += (2 * m + n[0] + n[1] + 1) % 2                       # before bT: 2 m + n[0] + n[1], odd
    n[2] += (3 * m + 1 + n[0] + n[1] + n[2] + 1) % 2            # before bO: 3 m + 1 + n[0] + n[1] + n[2], odd
    n[3] = n_bg - n[0] - n[1] - n[2]
    assert min(n) >= 0
    parts = [_fill(0, m, rng, first=0.0)]
    for z, cnt, des in zip(zones, n, (bE, bT, bO, None)):
        per = np.full(len(z), cnt // len(z))
        per[rng.permutation(len(z))[: cnt % len(z)]] += 1
        assert per.max() < m or per.max() <= 1
        parts += [_fill(b, int(c), rng) for b, c in zip(z, per) if c]
        if des is not None:
            parts.append(_fill(des, m, rng))
        if des == bT:
            parts.append(np.array([bT + 1], dtype=np.float32))
    parts.append(_fill(lutb - 1, m, rng, first=None)[: m - 1] if m > 1 else np.zeros(0, dtype=np.float32))
    parts.append(np.array([lutb], dtype=np.float32))
    tab = np.concatenate(parts).astype(np.float32)
    assert len(tab) == P and np.all(np.diff(tab) >= 0) and tab[0] == 0.0 and tab[-1] == lutb
    return tab, {"zero": 0, "even": bE, "tight": bT, "odd": bO, "top": lutb - 1}


def lookup_sim(tab, lutb, x, probes):
    """bt_lookup, score by score in plain Python (small inputs): from the pair of the bucket's first entry on, `probes` halving probes
    count the pairs whose second entry is <= x; the four entries (C D | A B) around the result and the float32 distances decide; a
    distance equal to the one further left takes the walk to the plateau's first entry.  With the restated probe count this is
    `nearest_first`; with fewer it is what a kernel that under-counts the fullest bucket's pairs would return."""
    tab = np.asarray(tab, dtype=np.float32)
    P = len(tab)
    sr = search(tab, lutb)
    pad = np.concatenate([np.full(BT_LEAD, -INF), tab, np.full(plan([P], False)["Ppad"][0] - BT_LEAD - P, INF)]).astype(np.float32)
    at = lambda k: pad[k + BT_LEAD]
    last_pair = (len(pad) - BT_LEAD) // 2 - 1
    out = []
    for xv in np.asarray(x, dtype=np.float32).reshape(-1):
        if not np.isfinite(xv):
            out.append(0)
            continue
        p = int(sr["lut"][int(bucket(xv, tab[0], sr["inv_w"], lutb))]) >> 1
        for st in range(probes - 1, -1, -1):
            q = min(p + (1 << st) - 1, last_pair)
            if at(2 * q + 1) <= xv:
                p = q + 1
        p = min(p, last_pair)
        a_in = at(2 * p) <= xv
        il = 2 * p if a_in else 2 * p - 1
        dl, dh, dm = abs(at(il) - xv), abs(at(il + 1) - xv), abs(at(il - 1) - xv)
        best = il + 1 if dh < dl else il
        if not dh < dl and dm == dl:
            while best > 0 and abs(at(best - 1) - xv) == dl:
                best -= 1
        out.append(best)
    return np.array(out, dtype=np.int64)


def designed_scores(tab, des, lutb):
    """For each designated bucket: every entry and both float32 neighbours, the midpoint of every adjacent pair (an exact tie: the left entry
    wins) and both of its neighbours, the bucket's floor b and nextafter(b + 1, 0), a score in the empty bucket on each side; once per
    table one float32 below tab[0] and above tab[P - 1], -1.0, -0.0, +inf, -inf, NaN."""
    out = []
    for b in des.values():
        e = tab[(tab >= b) & ((tab < b + 1) | (b == lutb - 1))]
        mid = ((e[:-1].astype(np.float64) + e[1:].astype(np.float64)) / 2).astype(np.float32)
        assert np.array_equal(mid.astype(np.float64) * 2, e[:-1].astype(np.float64) + e[1:])       # the midpoints are float32 values
        out += [e, up(e), down(e), mid, up(mid), down(mid), [F32(b), down(F32(b + 1))]]
        out.append([F32(b) - F32(0.5)] if b else [])
        out.append([F32(b) + F32(1.5)] if b < lutb - 1 else [])
    out.append([down(tab[0]), up(tab[-1]), F32(-1.0), F32(-0.0), INF, -INF, F32(np.nan)])
    return np.concatenate([np.asarray(o, dtype=np.float32) for o in out])


def planes_of(scores, Q, key):
    """[Q, N] from a list of score vectors: row 0 as given, the other rows permuted; shorter vectors wrap around."""
    N = max(len(v) for v in scores)
    out = []
    for s, v in enumerate(scores):
        v = np.resize(v, N)
        out.append(np.stack([v] + [v[rng_of(key, s, q).permutation(N)] for q in range(1, Q)]).astype(np.float32))
    return out


def quantile_like(P, kind, key):
    """An ordinary table: sorted draws shaped like a system's scores (dense where the scores are)."""
    rng = rng_of("quantile", P, kind, key)
    pool = [np.maximum(0.0, rng.gamma(0.5, 4.0, 3 * P) - 2.0) + 1e-3, rng.uniform(-0.2, 0.9, 3 * P), rng.normal(20.0, 4.0, 3 * P),
            np.log1p(np.abs(rng.normal(0, 1, 3 * P)))][kind % 4]
    return np.sort(pool)[np.linspace(0, 3 * P - 1, P).round().astype(np.int64)].astype(np.float32)


def random_scores(tab, Q, N, key, specials=True):
    """Uniform over the table's range and a little beyond, a seventh of the columns ON table entries, some on midpoints of neighbours."""
    rng = rng_of("scores", key, Q, N)
    lo, hi = float(tab[0]), float(tab[-1])
    span = max(hi - lo, 1e-3)
    x = rng.uniform(lo - 0.05 * span, hi + 0.05 * span, (Q, N)).astype(np.float32)
    on = rng.random((Q, N)) < 1 / 7
    k = rng.integers(0, len(tab), (Q, N))
    x[on] = tab[k[on]]
    if len(tab) > 1:
        half = rng.random((Q, N)) < 1 / 50
        kk = np.minimum(k, len(tab) - 2)
        x[half] = ((tab[kk].astype(np.float64) + tab[kk + 1]) / 2).astype(np.float32)[half]
    if specials and N >= 8:
        x[0, :3] = [np.nan, np.inf, -np.inf]
        x[Q - 1, N - 1], x[Q - 1, N - 2] = down(tab[0]), up(tab[-1])
    return x


def partial_rank(Q, N, key):
    """A rank plane of a partial system: ~40 % of the documents absent; the first and the last column of every row differ."""
    rng = rng_of("rank", key, Q, N)
    r = np.where(rng.random((Q, N)) < 0.6, 1, -1).astype(np.int32)
    r[:, 0] = 1
    r[:, N - 1] = -1 if N > 1 else 1
    r[::2, N - 1] = 1
    return r


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
class Case:
    """tabs [S], planes [S] of [Q, N] float32, ranks (None or [S] of None / [Q, N] int32), weights; `path`: the kernel that must take it;
    `sample`: columns per row the CPU file hands the brute-force oracle (None: all)."""

    def __init__(self, tabs, planes, w=None, ranks=None, path="lds-swap", sample=None, des=None, lutb=None):
        self.tabs = [np.ascontiguousarray(t, dtype=np.float32) for t in tabs]
        self.planes = [np.ascontiguousarray(p, dtype=np.float32) for p in planes]
        self.S = len(tabs)
        self.Q, self.N = self.planes[0].shape
        self.w = [1.0] if self.S == 1 and w is None else (w or [0.15, 0.35, 0.3, 0.2, 0.45, 0.25, 0.1, 0.05][: self.S])
        self.ranks, self.path, self.sample, self.des = ranks, path, sample, des
        self.P = [len(t) for t in self.tabs]
        assert all(np.all(np.diff(t) >= 0) for t in self.tabs) and all(p.shape == (self.Q, self.N) for p in self.planes)

    def plan(self, norm):
        return plan(self.P, norm == NORMS[1])

    def searches(self, norm):
        pl = self.plan(norm)
        return None if pl is None else [search(t, pl["lutb"]) for t in self.tabs]

    def expected(self, norm, V=None):
        return expected(self.planes, self.ranks, self.w, norm, self.tabs, V)


A_M = (1, 2, 3, 6, 7, 14, 15, 30, 31, 33, 64)
A_PAIRS = ((2, 3), (6, 7), (14, 15), (30, 31), (33, 1), (64, 15))       # two probe classes in one call: the switch changes between steps
A_P = {m: 10001 + i for i, m in enumerate(A_M)}                            # odd and even P in turn
A_INST = {1: 1, 2: 1, 3: 2, 6: 2, 7: 3, 14: 3, 15: 4, 30: 4, 31: "loop", 33: "loop", 64: "loop"}
A_PROBES = {1: 1, 2: 1, 3: 2, 6: 2, 7: 3, 14: 3, 15: 4, 30: 4, 31: 5, 33: 5, 64: 6}


def _designed_case(ms, Q=2):
    tabs, scores, dess = [], [], []
    for m in ms:
        t, des = designed_table(A_P[m], m)
        tabs.append(t); dess.append(des); scores.append(designed_scores(t, des, 16384))
    return Case(tabs, planes_of(scores, Q, ("A", ms)), des=dess, lutb=16384)


RUN_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 33)


def runs_table(P, lengths, key):
    """A designed table (bucket(x) = floor(x), 16,384 buckets) in which bucket 100 + 3 i holds TWO runs of lengths[i] equal entries, at
    b + 1/4 and b + 3/4, over a background of one entry per bucket -> (tab, [(bucket, length)])."""
    lutb = 16384
    rng = rng_of("runs", P, lengths, key)
    mine = {100 + 3 * i: L for i, L in enumerate(lengths)}
    n_bg = P - 2 - 2 * sum(lengths)
    free = np.array([b for b in range(1, lutb - 1) if not any(abs(b - d) <= 1 for d in mine)])
    bg = np.sort(rng.choice(free, n_bg, replace=False))
    ent = [np.zeros(1), bg + rng.integers(1, 128, n_bg) / 128.0, np.array([float(lutb)])]
    ent += [np.repeat([b + 0.25, b + 0.75], L) for b, L in mine.items()]
    tab = np.sort(np.concatenate(ent)).astype(np.float32)
    assert len(tab) == P
    return tab, sorted(mine.items())


def runs_scores(runs):
    """On each run, just above and just below it, equidistant between the two runs of the bucket (the left run's FIRST entry wins) and a
    float32 to either side of that, in the empty buckets next to it."""
    out = []
    for b, _ in runs:
        a, c, mid = F32(b + 0.25), F32(b + 0.75), F32(b + 0.5)
        out += [a, up(a), down(a), c, up(c), down(c), mid, up(mid), down(mid), F32(b), down(F32(b + 1)), F32(b - 0.5), F32(b + 1.5), F32(b + 0.3), F32(b + 0.9)]
    return np.array(out + [-1.0, 16385.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)


ROUND_X = (2.0 ** 30, 2.0 ** 30 - 64, 2.0 ** 30 + 128, 2.0 ** 30 + 256, 2.0 ** 31, 2.0 ** 29 + 3.0e7, 2.0 ** 28, 4.0e7)


def rounding_table(P, L):
    """Distinct entries near 3e7 at spacing 2.0 whose top L entries share ONE float32 distance from the score 2^30: they are the even
    numbers of (3e7 + 32 - 2 L, 3e7 + 32], the upper end of the distances that round to 2^30 - 3e7 (ulp 64, ties to even); the entries
    below them start 66 lower (at 64 a single top entry's neighbour would tie to the same even distance)."""
    assert 1 <= L <= 33
    top = 3.0e7 + 32 - 2.0 * np.arange(L)[::-1]
    rest = 3.0e7 + 32 - 2.0 * (L - 1) - 66 - 2.0 * np.arange(P - L)[::-1]
    tab = np.concatenate([rest, top])
    assert np.array_equal(tab, tab.astype(np.float32)) and np.all(np.diff(tab) > 0)
    return tab.astype(np.float32)


def rounding_scores(tab, key):
    rng = rng_of("rounding", key)
    k = rng.integers(0, len(tab), 200)
    return np.concatenate([np.array(ROUND_X, dtype=np.float32), tab[k], tab[k] + F32(1.0), tab[-40:], [F32(-2.0 ** 30), F32(0.0), F32(np.nan), INF]]).astype(np.float32)


PLAN_EDGES = (16084, 16085, 32212, 32213, 36308, 36309, 38356, 38357, 39380, 39381)   # each threshold of bt_plan from both sides
PLAN_LUTB = {16084: 16384, 16085: 16384, 32212: 16384, 32213: 8192, 36308: 8192, 36309: 4096, 38356: 4096, 38357: 2048, 39380: 2048, 39381: None}
PLAN_M = 30                                                                  # four unrolled probes: the longest unclamped reach


def _plan_case(P):
    lutb = PLAN_LUTB[P] or 2048
    tab, des = designed_table(P, PLAN_M, lutb)
    sc = designed_scores(tab, des, lutb)
    sc = np.concatenate([sc, [tab[-1], up(tab[-1]), F32(2.0) * tab[-1], INF], random_scores(tab, 1, 300, ("C", P), specials=False)[0]])
    return Case([tab], planes_of([sc], 2, ("C", P)), path="row" if PLAN_LUTB[P] is None else "lds-swap", des=[des], lutb=lutb)


MIXED_P = ((1, 2, 10001, 39380), (3, 27943, 16085, 257))


def _mixed_case(Ps, partial):
    tabs = [quantile_like(P, s, ("D", Ps)) for s, P in enumerate(Ps)]
    Q, N = 3, 1501
    planes = [random_scores(t, Q, N, ("D", Ps, s)) for s, t in enumerate(tabs)]
    ranks = None
    if partial is not None:
        ranks = [None] * len(Ps)
        ranks[partial] = partial_rank(Q, N, ("D", Ps))
    return Case(tabs, planes, ranks=ranks)


TAIL_N = (1, 2, 3, 4, 5, 7, 31, 33, 28671, 28672, 28673, 28675, 57344, 57345)


def _tail_case(N):
    tabs = [quantile_like(10001, s, "E") for s in range(2)]
    Q = 3
    planes = [random_scores(t, Q, N, ("E", N, s)) for s, t in enumerate(tabs)]
    return Case(tabs, planes, ranks=[None, partial_rank(Q, N, ("E", N))], sample=None if N < 1000 else 96)


WALK_SHAPES = ((255, 64), (256, 64), (257, 64), (513, 64), (129, 28673), (86, 57345), (171, 57345))     # (Q, N)
WALK_CARRY = {(171, 57345)}       # three chunks do not divide 256: advance() carries (at 258 items the carry belongs to workgroup 2, which has no second item)


WALK_ROWS = 16


def walk_rows(base, Q):
    """[Q, N] from WALK_ROWS base rows: row q is base row q % 16 rotated by 7 q + q // 16 columns -- no two rows of a case are equal, so a row
    taken for another shows, and what a column-wise operation makes of the plane is the same rotation of what it makes of the base rows."""
    return np.stack([np.roll(base[q % len(base)], 7 * q + q // len(base)) for q in range(Q)])


class WalkCase(Case):
    """Group F: up to 171 rows of 57,345 columns.  `expected` runs the restatement on the base rows and rotates the result (it works column
    by column); test_tables_cases_cpu.py holds THIS to the oracle on the rotated planes."""

    def __init__(self, tabs, base, Q, **kw):
        self.base = base
        super().__init__(tabs, [walk_rows(b, Q) for b in base], **kw)

    def expected(self, norm, V=None):
        return walk_rows(expected(self.base, None, self.w, norm, self.tabs, V), self.Q)


@functools.lru_cache(maxsize=2)
def _walk_inputs(N, P):
    tabs = [quantile_like(P, s, ("F", P)) for s in range(2)]
    return tabs, [random_scores(t, WALK_ROWS, N, ("F", N, P, s)) for s, t in enumerate(tabs)]


def _walk_case(Q, N, S, P):
    tabs, base = _walk_inputs(N, P)
    return WalkCase(tabs[:S], base[:S], Q, w=[1.0] if S == 1 else [0.4, 0.6], sample=48 if N > 64 else None)


QUOT_P = (10001, 27943, 32749, 39380)


def _quot_case(P):
    tab = (np.arange(P, dtype=np.float64) * 0.25 - 1000.0).astype(np.float32)      # strictly increasing, exact
    return Case([tab], [tab.reshape(1, P).copy()], w=[1.0])


def _denormal_case():
    P = 10001
    tab = (np.arange(P, dtype=np.uint32) * np.uint32(7)).view(np.float32)          # 0 ... 7e4 * 2^-149 ~ 1e-40: every entry denormal
    assert tab[0] == 0 and 0.9e-40 < tab[-1] < 1.1e-40
    k = rng_of("denormal").integers(0, P - 1, 150)
    mid = ((tab[k].view(np.uint32) + tab[k + 1].view(np.uint32)) // 2).astype(np.uint32).view(np.float32)
    sc = np.concatenate([tab[k], up(tab[k]), down(tab[k]), mid, tab[:4], tab[-4:], [0.0, -0.0, 1e-40, 2e-40, 1.0, -1.0, np.inf, -np.inf, np.nan]]).astype(np.float32)
    return Case([tab], planes_of([sc], 2, "H-denormal"))


def _const_case():
    tabs = [np.full(10001, 1.5, dtype=np.float32), quantile_like(10001, 1, "H")]
    planes = [random_scores(quantile_like(10001, 3, "H"), 3, 700, ("H", 0)), random_scores(tabs[1], 3, 700, ("H", 1))]
    planes[0][1, :4] = [1.5, up(1.5), down(1.5), 0.0]
    return Case(tabs, planes)


def _cases():
    c = {}
    for m in A_M:
        c[f"A-m{m}"] = (f"designed table, fullest bucket {m} at an even and an odd first index, in bucket 0 and in the top bucket: bt_lookup<{A_INST[m]}>, "
                        f"{A_PROBES[m]} probes, P = {A_P[m]}", functools.partial(_designed_case, (m,)))
    for a, b in A_PAIRS:
        c[f"A-m{a}+m{b}"] = (f"S = 2: bt_lookup<{A_INST[a]}> and bt_lookup<{A_INST[b]}> alternate step by step", functools.partial(_designed_case, (a, b)))
    c["B-runs-1to9"] = ("two runs of 1 .. 9 equal entries per bucket (fullest 18: four unrolled probes): bt_plateau_start's linear part, its hand-over, its bisection",
                        lambda: _runs_case(RUN_LENGTHS[:9]))
    c["B-runs-33"] = ("two runs of 33 equal entries in one bucket (fullest 66: the probe loop) next to runs of 5 and 6", lambda: _runs_case((33, 5, 6)))
    c["B-round-1to5"] = ("S = 5: entries near 3e7 at spacing 2.0, the top 1 .. 5 distinct entries share one float32 distance", lambda: _round_case(RUN_LENGTHS[:5]))
    c["B-round-6to33"] = ("S = 5: the same with 6, 7, 8, 9 and 33 entries on the rounding plateau", lambda: _round_case(RUN_LENGTHS[5:]))
    for P in PLAN_EDGES:
        what = "no plan: the global-memory search ('row')" if PLAN_LUTB[P] is None else f"{PLAN_LUTB[P]} buckets, NCE values {'next to' if P <= 16084 else 'swapped over'} the table"
        c[f"C-P{P}"] = (f"bt_plan at P = {P}: {what}; designed top bucket of {PLAN_M}, scores at and above tab[P - 1]" +
                        (", the +inf tail exactly BT_TAIL = 40 entries" if P == 39380 else ""), functools.partial(_plan_case, P))
    for Ps in MIXED_P:
        for partial in (None, 2):
            c["D-P" + "+".join(map(str, Ps)) + ("-partial" if partial is not None else "")] = (
                f"S = 4 with P = {Ps}: tab_cap from the longest table, last_pair and the DMA lengths from each system's own" +
                (", system 2 partial" if partial is not None else ""), functools.partial(_mixed_case, Ps, partial))
    for N in TAIL_N:
        c[f"E-N{N}"] = (f"row tail at N = {N} (N % 4 = {N % 4}, N % 32 = {N % 32}, {-(-N // BT_COLS)} chunk(s)): tail_ok, chunk_lim, the validity-word clamp; "
                        "system 1 partial", functools.partial(_tail_case, N))
    for Q, N in WALK_SHAPES:
        wk = walk(Q, N)
        for S in (1, 2):
            for P in (10001, 20000):
                c[f"F-Q{Q}-N{N}-S{S}-P{P}"] = (f"{wk['items']} items at {wk['chunks']} chunk(s), {wk['carries']} advance() carries; " +
                                               ("the table stays resident" if S == 1 else "a table swap per step") +
                                               ("; NCE values swapped over the table" if P == 20000 else ""), functools.partial(_walk_case, Q, N, S, P))
    for P in QUOT_P:
        c[f"G-P{P}"] = (f"bt_quot: every k of P = {P} through a strictly increasing table, w = 1.0", functools.partial(_quot_case, P))
    c["H-denormal"] = ("a table 0 ... 1e-40: inv_w overflows, everything in bucket 0, the probe loop over the whole table", _denormal_case)
    c["H-const+ordinary"] = ("a constant table (every distance equal: index 0 by the plateau walk) beside an ordinary one", _const_case)
    return c


def _runs_case(lengths):
    tab, runs = runs_table(10001, tuple(lengths), "B")
    c = Case([tab], planes_of([runs_scores(runs)], 2, ("B", lengths)), lutb=16384)
    c.runs = runs
    return c


def _round_case(lengths):
    tabs = [rounding_table(10001 + i, L) for i, L in enumerate(lengths)]
    return Case(tabs, planes_of([rounding_scores(t, L) for t, L in zip(tabs, lengths)], 2, ("B-round", lengths)))


CASES = _cases()                     # key -> (what the case hits, builder)
GROUPS = "ABCDEFGH"
WALK_NORM = {10001: NORMS[0], 20000: NORMS[1]}       # group F runs percentile-rank at P = 10,001 and NCE at P = 20,000


@functools.lru_cache(maxsize=8)
def case(key):
    return CASES[key][1]()


def group(g):
    return [k for k in CASES if k.startswith(g + "-")]


def norms_of(key):
    return (WALK_NORM[int(key.rsplit("-P", 1)[1])],) if key.startswith("F-") else NORMS
