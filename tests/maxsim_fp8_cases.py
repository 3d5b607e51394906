"""Reference quantiser, exact inputs and case table of the e4m3 MaxSim tests (test_gpu_maxsim_fp8.py on the GPU, test_maxsim_fp8_cpu.py
without one).  Not collected by pytest.

The quantiser.  TABLE holds the 256 values of OCP e4m3fn; quantize_ref rounds |x * 2^e| to the nearest of the 127 finite magnitudes by
comparing with the 126 midpoints (a value ON a midpoint goes to the even code), saturates everything above the last midpoint to 448 and
maps NaN to 0x7f, sign kept.  No bit manipulation of the float: it shares nothing with the kernel's integer arithmetic.

Exact inputs.  Every component is an integer in {-2 .. 2} at scale_exp = 0 (exact in e4m3), so every partial sum of a 128-term dot
product is an integer far below 2^24 and exact in float32 IN ANY ORDER: on such inputs fz_maxsim_e4m3 must equal the float64 formula bit
for bit whatever the instruction's internal order of the 128 terms.  "Poison" rows carry POISON8 = 448 in dimensions 120-127, where every
query token carries 1 and every clean document row 0: a clean document scores at most 120 * 4 = 480 per query token, one leaked row
(a masked row, a truncated tail, a neighbour, a clamped row) adds 8 * 448 = 3,584.  Largest magnitude: 128 * (3,584 + 480) < 2^19.
Guard documents, poisoned rows before Doff[0] and after Doff[N] and poisoned tails past max_doc_len follow maxsim_cases.grid_corpus.

The case table.  csrc/maxsim8.hip and the float16 kernel run one tile walk, csrc/maxsim_tiles.h, and so one launch plan (8 waves, 4 query
blocks per wave, 32 documents per workgroup, 32-row tiles, groups of 4 in a ring of 8), so the shapes are maxsim_cases.CASES and maxsim_cases.launch_plan / branches_of / BRANCHES
say which branch a case lands on; REQUIRED spells out what the table must reach at the least."""
import functools

import numpy as np

import maxsim_cases as M

DIM = M.DIM
POISON8 = 448.0
POISON_DIMS = slice(120, 128)
LQS = M.LQS
CASES = M.CASES
BRANCHES = M.BRANCHES
branches_of = M.branches_of
launch_plan = M.launch_plan
maxsim_ref = M.maxsim_ref
maxsim_fmax_ref = M.maxsim_fmax_ref
exact_f32 = M.exact_f32

# csrc/maxsim8.hip walks csrc/maxsim_tiles.h as the float16 kernel does: one plan
assert (M.MS_WAVES, M.MS_BLOCKS_PER_WAVE, M.MS_DOCS_PER_WG, M.MS_TABLE) == (8, 4, 32, 512)
RING_TOKENS = 8 * 32

REQUIRED = dict(
    Lq=(32, 64, 128), loads=("full", "partial", "idle"), Q195=(64, 195), lens=(0, 1, 15, 16, 17, 31, 32, 33), longer_than_ring=RING_TOKENS,
    N=(1, 32, 33, 257), max_docs=400)


# ---- the reference quantiser ---------------------------------------------------------------------------------------------------------
def _table():
    b = np.arange(256)
    e, m = (b >> 3) & 15, (b & 7).astype(np.float64)
    v = np.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * 2.0 ** (e - 7.0))
    v[(b & 0x7f) == 0x7f] = np.nan
    return np.where(b & 0x80, -v, v)


TABLE = _table()                      # float64; TABLE[0x7f], TABLE[0xff]: NaN
_MAG = TABLE[:0x7f]                   # the 127 finite magnitudes, ascending: 0, 2^-9, ..., 448
_MID = (_MAG[:-1] + _MAG[1:]) / 2     # exact in float64
assert _MAG[0x7e] == 448 and _MAG[1] == 2.0 ** -9 and _MAG[8] == 2.0 ** -6 and np.all(np.diff(_MAG) > 0)


def quantize_ref(x, scale_exp=0):
    """e4m3fn bytes of x * 2^scale_exp (x: float16 or anything float64 holds exactly)."""
    with np.errstate(invalid="ignore"):      # signalling NaN patterns
        y = np.asarray(x, dtype=np.float64) * 2.0 ** scale_exp
    mag = np.abs(y)
    nan = np.isnan(y)
    code = np.searchsorted(_MID, np.where(nan, 0.0, mag), side="left")        # midpoints strictly below |y|: above 448 and inf -> 0x7e
    tie = (code < len(_MID)) & (mag == _MID[np.minimum(code, len(_MID) - 1)])
    code = np.where(tie & (code % 2 == 1), code + 1, code)                     # on a midpoint: the even neighbour
    code = np.where(nan, 0x7f, code)
    return (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def dequantize_ref(b, scale_exp=0):
    return TABLE[np.asarray(b, dtype=np.uint8)] * 2.0 ** -scale_exp


def all_f16_patterns():
    """Every float16 bit pattern, as a [512, 128] float16 array."""
    return np.arange(65536, dtype=np.uint16).view(np.float16).reshape(512, 128)


# ---- exact inputs --------------------------------------------------------------------------------------------------------------------
def grid_queries8(rng, Q, Lq):
    q = rng.integers(-2, 3, (Q, Lq, DIM)).astype(np.float64)
    q[..., POISON_DIMS] = 1.0
    return q


def grid_corpus8(rng, lens, max_doc_len, guards=True, pre=0, post=0):
    """-> (values [pre + sum(lens) + post, 128] float64, Doff [N + 1] int64 with Doff[0] = pre): maxsim_cases.grid_corpus with the e4m3
    values and poison."""
    lens = np.asarray(lens, dtype=np.int64)
    Doff = np.zeros(len(lens) + 1, dtype=np.int64)
    Doff[0] = pre
    Doff[1:] = pre + np.cumsum(lens)
    rows = int(Doff[-1]) + post
    tok = rng.integers(-2, 3, (rows, DIM)).astype(np.float64)
    tok[:, POISON_DIMS] = 0.0
    bad = np.zeros(rows, dtype=bool)
    bad[:pre] = True
    bad[int(Doff[-1]):] = True
    for d, L in enumerate(lens):
        a = int(Doff[d])
        if guards and d % 2 == 1:
            bad[a: a + L] = True
        elif L > max_doc_len:
            bad[a + max_doc_len: a + L] = True
    tok[bad, POISON_DIMS] = POISON8
    return tok, Doff


@functools.lru_cache(maxsize=None)
def _case(case_id):
    c = next(c for c in CASES if c.id == case_id)
    rng = c.rng()
    Qv = grid_queries8(rng, c.Q, c.Lq)
    Dv, Doff = grid_corpus8(rng, c.lens, c.max_doc_len, c.guards, c.pre, c.post)
    ref = maxsim_ref(Qv, Dv, Doff, c.max_doc_len)
    for a in (Qv, Dv, Doff, ref):
        a.setflags(write=False)
    return Qv, Dv, Doff, ref


def values(case):
    """(query values, document values, Doff) of a grid case at scale_exp = 0, float64."""
    return _case(case.id)[:3]


def reference(case):
    """The float64 formula over values(case): computed once per case, shared and read-only."""
    return _case(case.id)[3]


def bytes_of(case):
    Qv, Dv, Doff = values(case)
    Q8, D8 = quantize_ref(Qv), quantize_ref(Dv)
    assert np.array_equal(dequantize_ref(Q8), Qv) and np.array_equal(dequantize_ref(D8), Dv), "a grid value is not exact in e4m3"
    return Q8, D8, Doff


def quarter_tokens(case):
    """The grid case as float16 multiples of 1/4 in [-1, 1] (the poison: 448 / 256 = 1.75): values(case) / 4.  Times 2^8 they are
    multiples of 64 up to 128, and 448: exact in e4m3, so quantising them at scale_exp = 8 loses nothing, the integer dot products stay
    below 2^24, and the score must be the bits of the float64 formula over the float16 tokens."""
    Qv, Dv, Doff = values(case)
    Dq = Dv / 4
    Dq[Dv == POISON8] = POISON8 / 256
    return (Qv / 4).astype(np.float16), Dq.astype(np.float16), Doff


DESCALE_CASES = [c for c in CASES if (c.name, c.Lq) in {("lengths", 32), ("fill", 64), ("truncate", 128), ("end-both", 64)}
                 and (c.name != "fill" or c.Q == 195) and (c.name != "truncate" or c.max_doc_len == 33)]


# ---- special values ------------------------------------------------------------------------------------------------------------------
def special_bytes():
    """Three queries of 32 tokens against six documents, as e4m3 bytes at scale_exp = 0: document 1 has one NaN byte in one of its rows
    (that row's dot products are NaN and are skipped), document 2 is NaN in every row (-inf per query token), document 3 holds rows
    saturated at +-448, document 4 is empty; documents 0 and 5 are plain."""
    rng = np.random.default_rng(58)
    Qv = grid_queries8(rng, 3, 32)
    Dv, Doff = grid_corpus8(rng, [20, 40, 33, 18, 0, 17], 512, guards=False)
    Q8, D8 = quantize_ref(Qv), quantize_ref(Dv)
    D8[int(Doff[1]) + 7, 37] = 0x7f
    D8[int(Doff[2]): int(Doff[3]), 5] = 0xff
    D8[int(Doff[3]): int(Doff[4])] = quantize_ref(rng.choice([0.0, 1e6, -1e6], (18, DIM), p=[0.8, 0.1, 0.1]))
    return Q8, D8, Doff
