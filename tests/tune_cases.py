"""Shared by tests/test_tune_cases_cpu.py and tests/test_gpu_tune_edges.py: seeded inputs, case tables and the NumPy reference of the
weight-sweep rank kernel (csrc/tune.hip: gold_ranks_kernel<S, WIDE> behind fz_gold_ranks_f32 / fz_gold_ranks_f64w).

The reference is the operation itself: NumPy's float32 / float64 element-wise products and sums are IEEE-exact, so the fused score of
a column is formed exactly as the kernel forms it (0 + fl(t * w), sequential unfused adds in system order) and the rank of a gold is a
count of plain comparisons.  Every comparison of a kernel output with it is np.array_equal on the whole [W, Q, 8] tensor.

Two input families.  EXACT: T in multiples of 1/8 within [-2, 2], weights in multiples of 1/32 within [-1, 1]: every product is a
multiple of 1/256 below 2, every partial sum of at most four of them below 8 -- exact in float32 and float64 in any order, so ranks
are decided by exact ties and `pos`.  ROUNDING: T = round(normal(0, 1), 2) and the reference's weight lattice (step 0.05, sum 1): the
rank depends on where each rounding happens (the CPU file measures by how much)."""
import functools
import itertools

import numpy as np

# the kernel's geometry, stated once (tune.hip: 256 threads x TUNE_COLS_F32 / TUNE_COLS_F64 columns, TUNE_WCHUNK, TUNE_G)
COLS_F32, COLS_F64, WCHUNK, G = 4096, 2048, 512, 8
THREADS, WAVE = 256, 64

COLUMN_NS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 8193]
WEIGHT_WS = [1, 2, 511, 512, 513, 1024, 1025]
SWEEPS = ["narrow", "wide"]


def chunk_cols(wide: bool) -> int:
    return COLS_F64 if wide else COLS_F32


def chunk_of(j, wide):
    return j // chunk_cols(wide)


def wave_of(j):
    """The 64-lane group that holds column j: a thread's columns are strided by 256 inside the chunk, and both chunk widths are
    multiples of 256."""
    return (j % THREADS) // WAVE


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def fused(T, w, wide, order=None):
    """acc = 0; for s in system order: acc = acc + T[s] * w[s].  Narrow: float32 throughout, the weight rounded to float32 first;
    wide: float64(T) * float64 weight, float64 adds.  One rounding per product and per add, nothing fused."""
    F = np.float64 if wide else np.float32
    acc = np.zeros(T[0].shape, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in (range(len(T)) if order is None else order):
            acc = acc + T[s].astype(F) * F(w[s])
    assert acc.dtype == F
    return acc


def fused_fma_narrow(T, w, wide=False, order=None):
    """What a contracted build would compute on the narrow sweep: the product exact (two float32 factors fit a float64), one rounding
    to float32 per add."""
    acc = np.zeros(T[0].shape, dtype=np.float32)
    for s in (range(len(T)) if order is None else order):
        acc = (acc.astype(np.float64) + T[s].astype(np.float64) * np.float64(np.float32(w[s]))).astype(np.float32)
    return acc


def fused_fma_wide(T, w, wide=True, order=None):
    """What a contracted build would compute on the wide sweep, exactly: fma(t, w, acc) per system.  For T entries that are multiples
    of 2^-30 and weights that are multiples of 2^-57 (asserted) every product and partial sum is an integer multiple of 2^-87:
    Python integers, rounded to float64 once per system by int / int (correctly rounded)."""
    U = 1 << 87
    toint = np.frompyfunc(int, 1, 1)
    acc = np.zeros(T[0].shape, dtype=np.float64)
    for s in (range(len(T)) if order is None else order):
        ti, wi = toint(T[s].astype(np.float64) * 2.0 ** 30), int(float(w[s]) * 2.0 ** 57)
        assert wi / 2.0 ** 57 == float(w[s]) and np.array_equal((ti / (1 << 30)).astype(np.float64), T[s])
        ai = toint(acc * 2.0 ** 87)
        assert np.array_equal((ai / U).astype(np.float64), acc)
        acc = ((ti * wi + ai) / U).astype(np.float64)
    return acc


def precedes(f, pos, fg, pg):
    """f, pos [Q, N]; fg, pg [Q, K] (a gold's fused score and position) -> [Q, K, N]: column j is listed and precedes the gold.
    The order: NaN first, then the larger score (-0.0 == +0.0), then the smaller pos."""
    f, p, fg, pg = f[:, None, :], pos[:, None, :], fg[:, :, None], pg[:, :, None]
    with np.errstate(invalid="ignore"):
        nj, ng = np.isnan(f), np.isnan(fg)
        before = (nj & ~ng) | (f > fg)
        tie = (nj & ng) | (f == fg)
    return (p >= 0) & (before | (tie & (p < pg)))


def listed_golds(pos, gold):
    """-> (ok [Q, K]: 0 <= gold < N and pos[gold] >= 0, col [Q, K] int64 (0 where not ok), pg [Q, K])."""
    N = pos.shape[1]
    ok = (gold >= 0) & (gold < N)
    col = np.where(ok, gold, 0).astype(np.int64)
    pg = np.take_along_axis(pos, col, axis=1)
    return ok & (pg >= 0), col, pg


def gold_ranks_ref(T, pos, weights, gold, wide, order=None, fuse=fused):
    """out[w, q, k] = #{listed j that precede gold[q, k] under weight vector w}; 0 for every slot that holds no listed gold."""
    ok, col, pg = listed_golds(pos, gold)
    out = np.zeros((len(weights),) + gold.shape, dtype=np.int32)
    for wi in range(len(weights)):
        f = fuse(T, weights[wi], wide, order)
        out[wi] = np.where(ok, precedes(f, pos, np.take_along_axis(f, col, axis=1), pg).sum(axis=2), 0)
    return out


def lexsort_ranks(T, pos, weights, gold, wide):
    """The same ranks by materialising and sorting: a literal stable np.lexsort of the listed columns of every row."""
    ok, col, _ = listed_golds(pos, gold)
    out = np.zeros((len(weights),) + gold.shape, dtype=np.int32)
    for wi in range(len(weights)):
        f = fused(T, weights[wi], wide)
        for q in range(pos.shape[0]):
            L = np.flatnonzero(pos[q] >= 0)
            s = f[q, L]
            nan = np.isnan(s)
            key = np.where(nan, 0.0, s) + 0.0                      # -0.0 + 0.0 == +0.0
            order = L[np.lexsort((pos[q, L], -key, ~nan))]         # last key first: NaN, then descending score, then ascending pos
            place = np.full(pos.shape[1], -1, dtype=np.int64)
            place[order] = np.arange(len(order))
            out[wi, q] = np.where(ok[q], place[col[q]], 0)
    return out


@functools.lru_cache(maxsize=None)
def lattice(S, step=0.05):
    """The reference's grid (hybrid.py:405-409): every vector on the step lattice that sums to 1, in itertools.product order."""
    grid = np.arange(0, 1 + step, step)
    return np.array([c for c in itertools.product(grid, repeat=S) if np.isclose(sum(c), 1.0)], dtype=np.float64)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, T, pos, weights, gold, wide):
        self.name, self.wide = name, bool(wide)
        self.T = [np.ascontiguousarray(t, dtype=np.float32) for t in T]
        self.pos = np.ascontiguousarray(pos, dtype=np.int32)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, len(T))
        self.gold = np.ascontiguousarray(gold, dtype=np.int32)
        self.S, (self.Q, self.N), self.W = len(T), self.pos.shape, len(self.weights)
        assert self.gold.shape == (self.Q, G) and all(t.shape == self.pos.shape for t in self.T)
        for q in range(self.Q):       # pos is a first-insertion position: the listed columns hold 0 .. U-1, each once
            p = self.pos[q][self.pos[q] >= 0]
            assert np.array_equal(np.sort(p), np.arange(len(p)))

    def weights_as_passed(self):
        """float64 selects the wide sweep; Python floats reach the narrow one rounded to float32."""
        return self.weights.astype(np.float64 if self.wide else np.float32)

    def reference(self):
        return gold_ranks_ref(self.T, self.pos, self.weights, self.gold, self.wide)


def exact_T(rng, S, Q, N):
    return [(rng.integers(-16, 17, (Q, N)) / 8.0).astype(np.float32) for _ in range(S)]


def exact_weights(rng, W, S):
    return rng.integers(-32, 33, (W, S)) / 32.0


def exact_weights_apart(rng, W):
    """S = 2 exact-family weights in which no vector is a non-negative multiple of its predecessor or of the vector WCHUNK before
    it (such vectors rank every row alike): what lets a misread weight index or a stale LDS counter show."""
    out = []
    while len(out) < W:
        w = rng.integers(-32, 33, 2)
        near = [out[i] for i in (len(out) - 1, len(out) - WCHUNK) if 0 <= i < len(out)]
        if all(w[0] * v[1] != w[1] * v[0] or w[0] * v[0] + w[1] * v[1] < 0 for v in near):
            out.append(w)
    return np.array(out).reshape(W, 2) / 32.0


def rounding_T(rng, S, Q, N):
    return [np.round(rng.normal(0.0, 1.0, (Q, N)), 2).astype(np.float32) for _ in range(S)]


def positions(rng, Q, N, unlisted=0.0, keep=()):
    """Every row's listed columns (a fraction `unlisted` of them in no list, the columns `keep` always listed) in a random
    first-insertion order."""
    pos = np.full((Q, N), -1, dtype=np.int32)
    for q in range(Q):
        on = rng.random(N) >= unlisted
        on[list(keep)] = True
        idx = np.flatnonzero(on)
        pos[q, idx] = rng.permutation(len(idx))
    return pos


def pad_gold(rows):
    gold = np.full((len(rows), G), -1, dtype=np.int32)
    for q, r in enumerate(rows):
        gold[q, :len(r)] = r
    return gold


def edge_columns(N):
    """Column 0, the thread stride, the last column of a chunk and the first of the next (both widths), N - 1."""
    return sorted({c for c in (0, 255, 256, COLS_F64 - 1, COLS_F64, COLS_F32 - 1, COLS_F32, N - 1) if 0 <= c < N})


def set_pos_order(pos, q, cols):
    """Re-deal the positions the (listed) columns `cols` of row q hold so that they ascend in the order given."""
    cols = list(cols)
    assert (pos[q, cols] >= 0).all()
    pos[q, cols] = np.sort(pos[q, cols])


def swap_pos(pos, q, col, target):
    """Column `col` of row q takes position `target`; the column that held it takes col's."""
    other = int(np.flatnonzero(pos[q] == target)[0])
    pos[q, other], pos[q, col] = pos[q, col], target


def plant_ties(T, pos, q, g, wide):
    """Give gold column g of row q two exact fused ties under every weight vector (copies of its T entries): one with a smaller
    pos in another column chunk AND another 64-lane group where the row has such a column (else another lane group, else any
    other column), one with a larger pos in the gold's own chunk."""
    N = pos.shape[1]
    others = [j for j in range(N - 1, -1, -1) if j != g]
    if not others:
        return
    far = [j for j in others if chunk_of(j, wide) != chunk_of(g, wide) and wave_of(j) != wave_of(g)] or \
          [j for j in others if wave_of(j) != wave_of(g)] or others
    a = far[0] if chunk_of(g, wide) == 0 else far[-1]
    near = [j for j in others if j != a and chunk_of(j, wide) == chunk_of(g, wide)]
    near = [j for j in near if wave_of(j) != wave_of(g)] or near
    picked = [a] + near[len(near) // 2: len(near) // 2 + 1]
    for t in T:
        t[q, picked] = t[q, g]
    set_pos_order(pos, q, [a, g] + picked[1:])


def tie_census(c):
    """For every weight vector: is there a listed gold with a tied listed column of smaller pos AND one of larger pos, one of them
    in another column chunk and another 64-lane group than the gold?  -> (both_sides, crossing) as 'for all weight vectors'."""
    ok, col, pg = listed_golds(c.pos, c.gold)
    j = np.arange(c.N)
    both_all, cross_all = True, True
    for w in c.weights:
        f = fused(c.T, w, c.wide)
        fg = np.take_along_axis(f, col, axis=1)
        with np.errstate(invalid="ignore"):
            tie = ((f[:, None, :] == fg[:, :, None]) | (np.isnan(f)[:, None, :] & np.isnan(fg)[:, :, None])) & (c.pos[:, None, :] >= 0)
        tie &= ok[:, :, None] & (j[None, None, :] != col[:, :, None])
        lo, hi = tie & (c.pos[:, None, :] < pg[:, :, None]), tie & (c.pos[:, None, :] > pg[:, :, None])
        far = (chunk_of(j, c.wide)[None, None, :] != chunk_of(col, c.wide)[:, :, None]) & (wave_of(j)[None, None, :] != wave_of(col)[:, :, None])
        both = lo.any(axis=2) & hi.any(axis=2)
        both_all &= bool(both.any())
        cross_all &= bool((both & (tie & far).any(axis=2)).any())
    return both_all, cross_all


def second_pass_census(c, n_weights=3):
    """The wide sweep's tie-break pass runs in a wave iff one of its listed columns holds a key EQUAL to a listed gold's (the
    gold's own wave always does).  -> the set of states {True, False} the case's waves reach, from the reference's scores."""
    ok, col, _ = listed_golds(c.pos, c.gold)
    cols = chunk_cols(True)
    nchunk = -(-c.N // cols)
    seen = set()
    for w in c.weights[:n_weights]:
        f = fused(c.T, w, True)
        fg = np.take_along_axis(f, col, axis=1)
        with np.errstate(invalid="ignore"):
            eq = ((f[:, None, :] == fg[:, :, None]) | (np.isnan(f)[:, None, :] & np.isnan(fg)[:, :, None])) & ok[:, :, None]
        eq = eq.any(axis=1) & (c.pos >= 0)
        full = np.zeros((c.Q, nchunk * cols), dtype=bool)
        full[:, :c.N] = eq
        waves = full.reshape(c.Q, nchunk, cols // THREADS, THREADS // WAVE, WAVE).any(axis=(2, 4))     # [Q, chunk, wave]
        for q in range(c.Q):
            if ok[q].any():
                seen |= set(waves[q].ravel().tolist())
    return seen


def branches(c):
    """The branch set a case reaches: workgroups per row, TUNE_WCHUNK passes, the NG instantiations, the key form, the wide sweep's
    second pass."""
    ok, col, _ = listed_golds(c.pos, c.gold)
    cols = chunk_cols(c.wide)
    nchunk = -(-c.N // cols)
    special = set()
    for q in range(c.Q):
        if not ok[q].any():
            continue               # NG = 0: the workgroup returns before it looks at a score
        gold_odd = any(not np.isfinite(t[q, col[q][ok[q]]]).all() for t in c.T)
        for ch in range(nchunk):
            special.add(bool(gold_odd or any(not np.isfinite(t[q, ch * cols:(ch + 1) * cols]).all() for t in c.T)))
    return dict(sweep="wide" if c.wide else "narrow", chunks=nchunk, passes=-(-c.W // WCHUNK), ng=set(ok.sum(axis=1).tolist()),
                special=special, second_pass=second_pass_census(c) if c.wide else set())


# ---- case builders -----------------------------------------------------------------------------------------------------------------
def _column_case(N, wide):
    """Golds on the edge columns, three different rows; every column listed, so a rank is a sum of the partial counts of all the
    row's workgroups.  Rows with more than one chunk carry planted ties across chunks and lane groups."""
    rng = np.random.default_rng(1000 + N)
    S, Q = 2, 3
    T, pos = exact_T(rng, S, Q, N), positions(rng, Q, N)
    E = edge_columns(N)
    rows = [E, E[::-1], [-1] + E[1::2]]
    plant_ties(T, pos, 0, 255 if N > 255 else E[-1], wide)
    plant_ties(T, pos, 1, N - 1, wide)
    W = np.concatenate([exact_weights(rng, 3, S), [[0.75, -0.5], [0.0, 0.0]]])
    return Case(f"cols-N{N}-{SWEEPS[wide]}", T, pos, W, pad_gold(rows), wide)


def _weights_case(Wn, wide):
    """S = 2, random exact-family weights, N = 2,049: two workgroups per pass on the wide sweep, one on the narrow."""
    rng = np.random.default_rng(2000)                                # the same rows for every W
    S, Q, N = 2, 3, 2049
    T, pos = exact_T(rng, S, Q, N), positions(rng, Q, N, unlisted=0.1, keep=[2048])
    gold = np.stack([rng.choice(np.flatnonzero(pos[q] >= 0), size=G, replace=False) for q in range(Q)])
    gold[1, 5:] = -1
    gold[0, 7] = 2048
    W = exact_weights_apart(np.random.default_rng(2100 + Wn), Wn)
    return Case(f"weights-W{Wn}-{SWEEPS[wide]}", T, pos, W, gold, wide)


def _lattice_case(wide):
    """The whole S = 4 lattice (1,771 vectors, four passes) on rounding-family rows."""
    rng = np.random.default_rng(2200)
    S, Q, N = 4, 3, 2049
    T, pos = rounding_T(rng, S, Q, N), positions(rng, Q, N, unlisted=0.1)
    for t in T:
        t[pos < 0] = 0.0
    gold = np.stack([rng.choice(np.flatnonzero(pos[q] >= 0), size=G, replace=False) for q in range(Q)])
    gold[2, 3:] = -1
    return Case(f"weights-lattice-S4-{SWEEPS[wide]}", T, pos, lattice(4), gold, wide)


def _systems_case(S, wide):
    rng = np.random.default_rng(3000 + S)
    Q, N = 3, 4097
    T, pos = exact_T(rng, S, Q, N), positions(rng, Q, N, unlisted=0.2)
    gold = np.stack([rng.choice(np.flatnonzero(pos[q] >= 0), size=G, replace=False) for q in range(Q)])
    gold[1, ::2] = -1
    W = np.concatenate([exact_weights(rng, 4, S), -np.ones((1, S)), np.zeros((1, S))])
    return Case(f"systems-S{S}-{SWEEPS[wide]}", T, pos, W, gold, wide)


def _slots_case(which, wide):
    """0 to 8 listed golds per query, three per case; padding between real golds, gold == N and N + 5, a gold with pos == -1, one
    column in two slots, a gold that ranks first and one that ranks last."""
    rng = np.random.default_rng(4000 + ord(which))
    S, Q, N = 3, 3, 4097
    T, pos = exact_T(rng, S, Q, N), positions(rng, Q, N, unlisted=0.25)
    L = [np.flatnonzero(pos[q] >= 0) for q in range(Q)]
    U = [np.flatnonzero(pos[q] < 0) for q in range(Q)]
    pick = lambda q, n: rng.choice(L[q], size=n, replace=False).tolist()
    W = exact_weights(rng, 4, S)
    if which == "A":      # NG = 0, 3, 8
        a, b = pick(1, 3), pick(2, 8)
        gold = np.array([[-1] * G, [-1, a[0], -1, -1, a[1], -1, a[2], -1], b])
    elif which == "B":    # NG = 1, 2 (one column twice), 4 (+ a gold no system lists)
        a, b, d = pick(0, 1), pick(1, 1), pick(2, 4)
        gold = np.array([[N, a[0], N + 5] + [-1] * 5, [-1, b[0], -1, -1, -1, -1, b[0], -1], [d[0], U[2][0], d[1], d[2], -1, U[2][-1], d[3], -1]])
    else:                 # NG = 5, 6, 7; positive weights, so +2 everywhere ranks first and -2 everywhere last
        a, b, d = pick(0, 5), pick(1, 6), pick(2, 7)
        gold = np.array([a + [-1] * 3, [-1] + b + [-1], d + [N]])
        W = np.abs(W) + 1 / 32
        for q, (first, last) in enumerate([(a[0], a[4]), (b[5], b[0]), (d[3], d[6])]):
            for t in T:
                t[q, first], t[q, last] = 2.0, -2.0
            swap_pos(pos, q, first, 0)
            swap_pos(pos, q, last, len(L[q]) - 1)
    return Case(f"slots-{which}-{SWEEPS[wide]}", T, pos, W, gold, wide)


def _unlisted_case(wide):
    """pos == -1 on a third of the columns, holding the largest score of every system under positive weights: counted, they would
    beat every gold.  Row 2 lists the gold alone."""
    rng = np.random.default_rng(5000)
    S, Q, N = 2, 3, 4097
    T, pos = exact_T(rng, S, Q, N), positions(rng, Q, N, unlisted=1 / 3)
    for t in T:
        np.clip(t, -2.0, 1.75, out=t)
        t[pos < 0] = 2.0
    gold = np.stack([rng.choice(np.flatnonzero(pos[q] >= 0), size=G, replace=False) for q in range(Q)])
    gold[1, 6:] = np.flatnonzero(pos[1] < 0)[[0, -1]]
    pos[2] = -1
    pos[2, 4096] = 0
    gold[2] = [-1, 4096, 5, -1, -1, -1, -1, -1]
    W = np.abs(exact_weights(rng, 4, S)) + 1 / 32
    return Case(f"unlisted-{SWEEPS[wide]}", T, pos, W, gold, wide)


def _signs_case(wide):
    """Row 0: every fused score negative under the first weight vector; row 1: straddles 0, -0.0 entries; row 2: only +-0.0.
    Weight vectors: positive, all-zero (every listed column ties: rank == pos), negative (-0.0 products), mixed."""
    rng = np.random.default_rng(6000)
    S, Q, N = 3, 3, 4097
    T, pos = exact_T(rng, S, Q, N), positions(rng, Q, N, unlisted=0.1)
    for t in T:
        t[0] = -np.maximum(np.abs(t[0]), 0.125)
        t[1, ::3] = -0.0
        t[2] = np.where(rng.random(N) < 0.5, -0.0, 0.0)
    gold = np.stack([rng.choice(np.flatnonzero(pos[q] >= 0), size=G, replace=False) for q in range(Q)])
    gold[1, 0] = np.flatnonzero(pos[1, ::3] >= 0)[0] * 3           # a gold whose entries are all -0.0
    W = np.array([[0.5, 0.25, 1.0], [0.0, 0.0, 0.0], [-0.5, -1.0, -0.03125], [0.5, -0.5, 0.0], [-0.0, 0.0, -1.0]])
    return Case(f"signs-{SWEEPS[wide]}", T, pos, W, gold, wide)


def _nonfinite_case(S, wide):
    """N = 8,193 (three narrow, five wide workgroups per row).  Row 0: +inf, -inf, NaN and inf / -inf pairs in the golds' own chunk;
    row 1: finite golds in chunk 0, every non-finite entry behind column 8,000 (the golds' workgroup keeps the fast key, the
    others take the full one); row 2: the golds themselves NaN, +inf and -inf, NaN columns on both sides of the NaN gold's pos."""
    rng = np.random.default_rng(7000 + S)
    Q, N = 3, 8193
    odd_cols = [b + 2 * k for b in (7, 900, 8000, 8179) for k in range(7)]
    gold = pad_gold([[5, 300, 2000, 7, 13], [5, 300, 2000, -1, 1], [40, 41, 42, 5000, 8192]])
    T, pos = exact_T(rng, S, Q, N), positions(rng, Q, N, unlisted=0.1, keep=odd_cols + [4500, 8100] + gold[gold >= 0].tolist())
    inf, nan = np.float32(np.inf), np.float32(np.nan)

    def odd(q, base):
        for k, (x, y) in enumerate([(inf, None), (-inf, None), (nan, None), (inf, -inf), (None, inf), (-inf, inf), (None, nan)]):
            j = base + 2 * k
            if x is not None:
                T[0][q, j] = x
            if y is not None:
                T[S - 1][q, j] = y
    odd(0, 7); odd(0, 900); odd(1, 8000); odd(1, 8179)
    T[0][2, [40, 4500, 8100]] = nan
    T[0][2, 41], T[0][2, 42] = inf, -inf
    set_pos_order(pos, 2, [4500, 40, 8100])
    W = np.zeros((6, S))
    W[0, 0], W[1, S - 1], W[2, :], W[3, :], W[4, 0], W[4, S - 1] = 0.5, 0.5, 0.5, -0.25, -0.25, 0.75
    return Case(f"nonfinite-S{S}-{SWEEPS[wide]}", T, pos, W, gold, wide)


TINY = np.float32(2.0 ** -30)


def _low_bits_case(wide):
    """Fused scores that are equal in float32 and different in float64, and doubles that differ only in their low 32 bits, on both
    signs (both branches of the fast key); row 1: exact ties in two waves of two chunks only, every other wave sees no equal key."""
    rng = np.random.default_rng(8000)
    S, Q, N = 2, 3, 4097
    T = [rng.normal(0.0, 1.0, (Q, N)).astype(np.float32) for _ in range(S)]
    pos = positions(rng, Q, N)
    cols = [10, 200, 2100, 4096, 77, 3000]
    for q in (0, 2):
        T[0][q, cols] = [1, 1, 1, -1, -1, -1]
        T[1][q, cols] = [0, TINY, -TINY, 0, TINY, -TINY] if q == 0 else [TINY, TINY / 2, TINY / 4, -TINY, -TINY / 2, -TINY / 4]
    dup = [130, 2048 + 70, 4000]                                    # gold 130: lane group 2 of chunk 0; copies in groups 1 and 2 of the wide sweep's chunk 1
    for t in T:
        t[1, dup[1:]] = t[1, dup[0]]
    set_pos_order(pos, 1, [dup[1], dup[0], dup[2]])
    gold = pad_gold([cols, dup[:1] + [5, 2500], cols[::-1]])
    W = np.array([[1.0, 1.0], [0.5, 0.5], [0.25, 1.0], [1.0, -1.0]])
    return Case(f"lowbits-{SWEEPS[wide]}", T, pos, W, gold, wide)


ROUNDING_STRIDE = {2: 1, 3: 9, 4: 67}     # lattice samples: all 21 vectors, every 9th of 231, every 67th of 1,771 ...


def rounding_sample(S):
    """... and every vector of the 0.2 sub-lattice (6 / 21 / 56 vectors), in lattice order.  Measured on the reference over the whole
    S = 3 lattice, a fused multiply-add changes the float64 sweep's ranks on 12 % of the vectors only (float32 scores under float64
    arithmetic seldom come within an ulp of each other), and those sit on the sub-lattice (14 of its 21 vectors): a strided sample
    alone would leave the wide sweep's contraction nearly unobserved."""
    L = lattice(S)
    sub = (np.rint(L * 20).astype(np.int64) % 4 == 0).all(axis=1)
    return L[sorted(set(np.flatnonzero(sub).tolist()) | set(range(0, len(L), ROUNDING_STRIDE[S])))]


# Golds of the S = 3 and S = 4 rounding rows, found by a search over the REFERENCE alone: per row the four listed columns whose place in
# the float64 ranking moves under the reversed system order on most vectors of the sample, and the four that move most under a
# fused multiply-add.  Random golds leave the wide sweep's order of adds nearly unobserved (5 % of the lattice): float32 scores under
# float64 arithmetic come within an ulp of each other only where an exact decimal tie meets cancelling float32 errors.
ROUNDING_GOLD = {3: [[8, 168, 193, 203, 648, 1431, 2835, 4086], [216, 591, 671, 694, 795, 837, 1188, 2191], [165, 595, 624, 722, 1386, 2837, 3827, 3867]],
                 4: [[28, 960, 1273, 1559, 2695, 2816, 2925, 2942], [794, 813, 1030, 1451, 2425, 2679, 3329, 3614], [305, 469, 733, 833, 1420, 1459, 1664, 3535]]}


def _rounding_case(S, wide):
    rng = np.random.default_rng(9000 + S)
    Q, N = 3, 4097
    T, pos = rounding_T(rng, S, Q, N), positions(rng, Q, N, unlisted=0.1)
    for t in T:
        t[pos < 0] = 0.0
    gold = np.stack([rng.choice(np.flatnonzero(pos[q] >= 0), size=G, replace=False) for q in range(Q)])
    gold = np.array(ROUNDING_GOLD.get(S, gold))
    return Case(f"rounding-S{S}-{SWEEPS[wide]}", T, pos, rounding_sample(S), gold, wide)


def _claim_case(wide):
    """The integer claim's inputs: rounding family, N = 4,097, partial lists (a third of the columns in no list, their T entries 0),
    three lattice vectors."""
    rng = np.random.default_rng(9500)
    S, Q, N = 3, 3, 4097
    T, pos = rounding_T(rng, S, Q, N), positions(rng, Q, N, unlisted=1 / 3)
    for s, t in enumerate(T):
        t[pos < 0] = 0.0
        t[:, s::7] = 0.0                                            # columns a single system does not list
    gold = np.stack([rng.choice(np.flatnonzero(pos[q] >= 0), size=G, replace=False) for q in range(Q)])
    gold[0, 7] = np.flatnonzero(pos[0] < 0)[3]
    return Case(f"claim-{SWEEPS[wide]}", T, pos, lattice(S)[[40, 117, 200]], gold, wide)


BUILDERS = {}
for _wide in (False, True):
    for _n in COLUMN_NS:
        BUILDERS[f"cols-N{_n}-{SWEEPS[_wide]}"] = functools.partial(_column_case, _n, _wide)
    for _w in WEIGHT_WS:
        BUILDERS[f"weights-W{_w}-{SWEEPS[_wide]}"] = functools.partial(_weights_case, _w, _wide)
    BUILDERS[f"weights-lattice-S4-{SWEEPS[_wide]}"] = functools.partial(_lattice_case, _wide)
    for _s in (1, 2, 3, 4):
        BUILDERS[f"systems-S{_s}-{SWEEPS[_wide]}"] = functools.partial(_systems_case, _s, _wide)
    for _x in "ABC":
        BUILDERS[f"slots-{_x}-{SWEEPS[_wide]}"] = functools.partial(_slots_case, _x, _wide)
    BUILDERS[f"unlisted-{SWEEPS[_wide]}"] = functools.partial(_unlisted_case, _wide)
    BUILDERS[f"signs-{SWEEPS[_wide]}"] = functools.partial(_signs_case, _wide)
    for _s in (2, 3):
        BUILDERS[f"nonfinite-S{_s}-{SWEEPS[_wide]}"] = functools.partial(_nonfinite_case, _s, _wide)
    BUILDERS[f"lowbits-{SWEEPS[_wide]}"] = functools.partial(_low_bits_case, _wide)
    for _s in (2, 3, 4):
        BUILDERS[f"rounding-S{_s}-{SWEEPS[_wide]}"] = functools.partial(_rounding_case, _s, _wide)
    BUILDERS[f"claim-{SWEEPS[_wide]}"] = functools.partial(_claim_case, _wide)

NAMES = list(BUILDERS)
TIE_CROSSING = [n for n in NAMES if n.startswith("cols-") and int(n.split("-")[1][1:]) > chunk_cols(n.endswith("wide"))]
ROUNDING = [n for n in NAMES if n.startswith("rounding-")]
ADJACENT = ROUNDING + [n for n in NAMES if n.startswith("weights-")]          # cases that rely on neighbouring vectors ranking differently


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    c = BUILDERS[name]()
    assert c.name == name
    return c


@functools.lru_cache(maxsize=None)
def reference(name) -> np.ndarray:
    """Computed once per process and shared; callers must not write to it."""
    r = case(name).reference()
    r.setflags(write=False)
    return r
