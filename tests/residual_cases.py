"""The residual code of the compressed ColBERT token index restated in numpy (include/fusion_hip.h 'Residual-compressed token rows';
csrc/rerank_residual.hip), and the inputs of its tests (test_residual_cpu.py without a GPU, test_gpu_residual.py on one).  Not collected
by pytest.  Queries, document lengths, candidate lists, launches and the expectation come from maxsim_cases.py / maxsim_pairs_cases.py,
unchanged.

The grid corpus is built DIRECTLY from random codes and random buckets: centroids on the 1/4 grid in [-1, 1], weights (2 i - 3) / 8
(nbits = 2) or (2 i - 15) / 32 (nbits = 4), cutoffs at the midpoints.  Every decompressed value C + w is then a multiple of 1/32 of
magnitude < 2, exact in float16, and with queries on the 1/4 grid every product is a multiple of 1/128 and every partial sum exact in
float32 in any order: the kernel must equal the float64 formula over the decompressed rows bit for bit.  Poison rows (guard documents,
the rows before Doff[0] and after Doff[N], the tail of every document past max_doc_len -- the truncated last document's included) carry
valid codes that point at centroid rows filled with 1024, and residual bytes 0xFF: they decompress to 1024 in every dimension (1024 + w
rounds to 1024 in float16), so one leaked row moves a score by a multiple of 256."""
import functools

import numpy as np

import maxsim_cases as M
import maxsim_pairs_cases as P

DIM = 128
NBITS = (2, 4)
K_CLEAN, K_POISON = 290, 10          # K = 300, not a power of two; the poison centroid rows come last
K = K_CLEAN + K_POISON
POISON = 1024.0
# the sweep of the grid test: every Lq and width, maxsim_pairs_cases' max_doc_lens and id bases
KS = (1, 7, 65, 130)
QS = (1, 5)

# storage position s -> the dimension it holds
POS_DIM = np.array([32 * ((s >> 3) & 3) + 8 * (s >> 5) + (s & 7) for s in range(DIM)])
assert sorted(POS_DIM.tolist()) == list(range(DIM))


# ---- the code ----------------------------------------------------------------------------------------------------------------------
def bucket(r, cutoffs):
    """The number of cutoffs c with r > c: a residual equal to a cutoff falls in the lower bucket, a NaN residual in bucket 0."""
    r = np.asarray(r, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (r[..., None] > np.asarray(cutoffs, dtype=np.float32)).sum(axis=-1).astype(np.uint8)


def pack(buckets, nbits):
    """buckets [n, 128] by DIMENSION -> [n, 16 nbits] uint8: storage positions fill ascending bytes, inside a byte ascending bit fields."""
    b = np.asarray(buckets, dtype=np.uint8)[:, POS_DIM]
    per = 8 // nbits
    out = np.zeros((b.shape[0], DIM // per), dtype=np.uint8)
    for i in range(per):
        out |= (b[:, i::per] << (nbits * i)).astype(np.uint8)
    return out


def unpack(packed, nbits):
    """[n, 16 nbits] uint8 -> buckets [n, 128] by dimension."""
    per = 8 // nbits
    by_pos = np.zeros((packed.shape[0], DIM), dtype=np.uint8)
    for i in range(per):
        by_pos[:, i::per] = (packed >> (nbits * i)) & ((1 << nbits) - 1)
    out = np.zeros_like(by_pos)
    out[:, POS_DIM] = by_pos
    return out


def compress(tok, codes, C, cutoffs, nbits):
    r = np.asarray(tok, dtype=np.float16).astype(np.float32) - np.asarray(C, dtype=np.float16)[codes].astype(np.float32)
    return pack(bucket(r, cutoffs), nbits)


def decompress(packed, codes, C, weights, nbits):
    """float16(C[code] + weights[bucket]): numpy's half add forms the float32 sum and rounds it once, which is the IEEE half sum
    (test_residual_cpu.py checks that on every kind of finite pair)."""
    return np.asarray(C, dtype=np.float16)[codes] + np.asarray(weights, dtype=np.float16)[unpack(packed, nbits)]


def train_buckets(residuals, nbits):
    """ops.residual_buckets on the given sample values: equal-population cutoffs, float64 bucket means."""
    srt = np.sort(np.asarray(residuals, dtype=np.float32).ravel())
    m, B = len(srt), 1 << nbits
    cutoffs = np.array([srt[(i * m) // B - 1] for i in range(1, B)], dtype=np.float32)
    b = bucket(srt, cutoffs)
    weights = np.zeros(B, dtype=np.float64)
    for i in range(B):
        mine = srt[b == i]
        weights[i] = mine.astype(np.float64).mean() if len(mine) else cutoffs[max(i - 1, 0)]
    return cutoffs, weights.astype(np.float16)


# ---- the grid corpus ---------------------------------------------------------------------------------------------------------------
def grid_buckets(nbits):
    """(cutoffs [B - 1] float32 at the midpoints, weights [B] float16)."""
    B = 1 << nbits
    w = (2.0 * np.arange(B) - (B - 1)) / (8.0 if nbits == 2 else 32.0)
    return ((w[1:] + w[:-1]) / 2).astype(np.float32), w.astype(np.float16)


@functools.lru_cache(maxsize=None)
def grid_centroids():
    C = np.random.default_rng(300).integers(-4, 5, (K, DIM)).astype(np.float64) / 4.0
    C[K_CLEAN:] = POISON
    C = C.astype(np.float16)
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def grid_corpus(nbits, max_doc_len):
    """-> (packed [rows, 16 nbits] uint8, codes [rows] int32, Doff [N + 1] int64, D [rows, 128] float16 = the restated decompression)."""
    rng = np.random.default_rng(9000 + 10 * max_doc_len + nbits)
    lens = np.asarray(P.LENS, dtype=np.int64)
    Doff = np.zeros(len(lens) + 1, dtype=np.int64)
    Doff[0] = P.PRE
    Doff[1:] = P.PRE + np.cumsum(lens)
    rows = int(Doff[-1]) + P.POST
    bad = np.zeros(rows, dtype=bool)
    bad[:P.PRE] = True
    bad[int(Doff[-1]):] = True
    for d, L in enumerate(lens):
        a = int(Doff[d])
        if d % 2 == 1:
            bad[a: a + L] = True
        elif L > max_doc_len:
            bad[a + max_doc_len: a + L] = True
    codes = rng.integers(0, K_CLEAN, rows).astype(np.int32)
    codes[bad] = rng.integers(K_CLEAN, K, int(bad.sum())).astype(np.int32)
    packed = pack(rng.integers(0, 1 << nbits, (rows, DIM)), nbits)
    packed[bad] = 0xFF
    _, weights = grid_buckets(nbits)
    D = decompress(packed, codes, grid_centroids(), weights, nbits)
    assert (D[bad] == POISON).all() and np.abs(D[~bad]).max() < 2
    assert np.array_equal(D[~bad].astype(np.float64), grid_centroids()[codes[~bad]].astype(np.float64) + weights[unpack(packed[~bad], nbits)].astype(np.float64))
    for a in (packed, codes, Doff, D):
        a.setflags(write=False)
    return packed, codes, Doff, D


@functools.lru_cache(maxsize=None)
def grid_reference(Lq, Q, nbits, max_doc_len):
    """[Q, N] float32: exactly the float64 formula over the decompressed rows (computed once per shape and shared)."""
    _, _, Doff, D = grid_corpus(nbits, max_doc_len)
    ref = M.exact_f32(M.maxsim_ref(P.queries(Lq, Q), D, Doff, max_doc_len))
    ref.setflags(write=False)
    return ref


# ---- rounding data -----------------------------------------------------------------------------------------------------------------
def unit_index(rng, n, Kc=K):
    """Unit-norm token rows [n, 128] float16, unit-norm centroids [Kc, 128] float16 and the codes [n] int32 of the largest float32 dot
    product (ties to the lowest id): C + w is not representable in float16 here, so the rounding of the half add matters."""
    tok = rng.normal(0, 1, (n, DIM))
    tok = (tok / np.maximum(np.linalg.norm(tok, axis=1, keepdims=True), 1e-6)).astype(np.float16)
    C = rng.normal(0, 1, (Kc, DIM))
    C = (C / np.linalg.norm(C, axis=1, keepdims=True)).astype(np.float16)
    codes = np.argmax(tok.astype(np.float32) @ C.astype(np.float32).T, axis=1).astype(np.int32) if n else np.zeros(0, dtype=np.int32)
    return tok, C, codes


def clustered_tokens(rng, n, Kc, noise):
    """n unit-norm rows around Kc unit-norm centres (normal noise of the given scale per dimension) -> (tok float16, centres float16)."""
    centres = rng.normal(0, 1, (Kc, DIM))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    tok = centres[rng.integers(0, Kc, n)] + rng.normal(0, noise, (n, DIM))
    tok /= np.linalg.norm(tok, axis=1, keepdims=True)
    return tok.astype(np.float16), centres.astype(np.float16)
