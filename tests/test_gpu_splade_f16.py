"""fz_splade_head_max_f16 (csrc/splade16.hip) and the `amp` switch of the DPR and SPLADE encoders.

The kernel, bit for bit: on score_cases.SpladeCase inputs (multiples of 1/4 in [-2, 2]: every entry is a float16 value, every product and
partial sum exact in float32 in any order) the pooled output equals, by torch.equal, the pooling kernel over the exact float32 logits AND
the float32 head on the same values.  Operands are views into larger buffers with NaN behind every row and NaN ghost rows around the
problem.  The edge shapes derive from the kernel's own tile constants (fz_splade_head_f16_tile).

On random data: two calls give the same bits, and the result lies in a sandwich that needs no constant for log1pf -- with a, w the float16
operands as float64, L = a w^T and B[t, v] = d 2^-23 sum_k |a[t, k] w[v, k]| (float16 products are exact in float32; d - 1 float32
additions in any order err by at most (d - 1) u / (1 - (d - 1) u) <= d u of that sum; u = 2^-23 also covers an accumulator that truncates),
the pooled value lies between fz_segment_splade_max_f32 of (L - B + bias) rounded down to float32 and of (L + B + bias) rounded up.  That
leans only on the device log1pf being non-decreasing.

The encoders: amp=True takes the float16 layers (and, for SPLADE, the float16 head), amp=False is bit-identical to an encoder built
without the argument, and the differences between the two precisions are measured against the float32 encoder, the reference's arithmetic.
The packed forward needs 64-wide heads, which encoders.TINY (16-wide) does not have: the small encoders here are the 2-layer, 2-head,
128-wide shape the cross-encoder tests use, the base-size run goes through random_init."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import score_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tile():
    from fusion_amd import _lib
    v = [C.c_int(-1) for _ in range(4)]
    assert _lib.lib().fz_splade_head_f16_tile(*[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


BM, BN, KT, KS = tile()


def view16(a):
    """a [rows, d] float64 on the grid -> its float16 view inside a NaN-framed device buffer (8 halves of NaN behind every row, NaN ghost rows
    before and after), handed to the kernel uncopied."""
    assert np.array_equal(a.astype(np.float16).astype(np.float64), a), "not float16 values"
    buf, rows, n = S.framed(a, pad=8, dtype=np.float16)
    v = dev(buf)[rows, :n]
    assert v.stride(0) > n and v.data_ptr() % 16 == 0 and v.dtype == torch.float16
    return v


def view32(ops, a):
    buf, rows, n = S.framed(a)
    v = dev(buf)[rows, :n]
    assert ops.pad_dim(v) is v and v.stride(0) > n
    return v


def _exact_shapes():
    shapes = []
    for V in (1, 63, 64, 65, BN - 1, BN, BN + 1, 509):
        shapes.append((701, V, KS + 8))
    for d in (8, KS - 8, KS + 8, KT - 8, KT, KT + 8, 2 * KT + 8):
        shapes.append((701, 509, d))
    shapes += [(6 * BM, 509, KS + 8), (1085, 509, KS + 8)]
    shapes.append((1085, 9000, 8))      # 9 row blocks x 71 (72 with the XCD padding) vocabulary tiles: more ids than the 512 resident workgroups
    out = []
    for s in shapes:
        if s not in out and s[2] > 0:
            out.append(s)
    return out


@pytest.mark.parametrize("T,V,d", _exact_shapes(), ids=lambda v: str(v))
def test_head_is_exact_on_grid_values(ops, T, V, d):
    case = S.SpladeCase(T, V, d)
    X, W, bias, cu, _ = case.inputs()
    logits = case.logits(X, W, bias)
    cu_d, b32 = dev(cu), dev(bias.astype(np.float32))
    got = ops.splade_head_max_f16(view16(X), view16(W), b32, cu_d)
    assert got.shape == (len(cu) - 1, V) and got.dtype == torch.float32
    unfused = ops.segment_splade_max(dev(S.exact_f32(logits)), cu_d)
    bad = (got != unfused).nonzero()
    assert torch.equal(got, unfused), (case.id, len(bad), [(int(s), int(v), float(got[s, v]), float(unfused[s, v])) for s, v in bad[:8]])
    fp32 = ops.splade_head_max(view32(ops, X), view32(ops, W), b32, cu_d)
    assert torch.equal(got, fp32), case.id


def test_head_is_exact_on_dense_grid_values(ops):
    """No zero anywhere: every k position of every lane's fragment carries a non-zero (SpladeCase rows hold at most four).  Sums of at most
    136 products of multiples of 1/4 up to 1 are multiples of 1/16 below 2^8: exact in float32 in any order."""
    T, V, d = 300, 257, 2 * KT + 8
    assert d <= 192
    rng = np.random.default_rng(5)
    vals = np.array([-1.0, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0])
    X, W, bias = rng.choice(vals, (T, d)), rng.choice(vals, (V, d)), S.grid(rng, 1, V)[0]
    cu = np.array([0, 1, 1, 70, 128, 129, 255, 300], dtype=np.int32)
    logits = X @ W.T + bias[None, :]
    cu_d, b32 = dev(cu), dev(bias.astype(np.float32))
    got = ops.splade_head_max_f16(view16(X), view16(W), b32, cu_d)
    assert torch.equal(got, ops.segment_splade_max(dev(S.exact_f32(logits)), cu_d))
    assert torch.equal(got, ops.splade_head_max(view32(ops, X), view32(ops, W), b32, cu_d))
    assert int((got > 0).sum()) > got.numel() // 4      # (the case is not mostly relu's zeros)


def test_python_contract(ops):
    x = torch.zeros((4, 12), dtype=torch.float16, device="cuda")
    w = torch.zeros((5, 12), dtype=torch.float16, device="cuda")
    b = torch.zeros(5, device="cuda")
    cu = torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.splade_head_max_f16(x, w, b, cu)
    with pytest.raises(TypeError):
        ops.splade_head_max_f16(x.float(), w, b, cu)
    x, w = x[:, :8].contiguous(), w[:, :8].contiguous()
    z = ops.splade_head_max_f16(x[:0], w, b, torch.zeros(3, dtype=torch.int32, device="cuda"))
    assert z.shape == (2, 5) and not z.any()
    assert ops.splade_head_max_f16(x, w, b, cu[:1]).shape == (0, 5)
    assert not ops.splade_head_max_f16(x, w, b, cu).any()         # log1p(relu(0)) = 0


# ---- random data -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_case():
    T, V, d = 300, 257, 768
    rng = np.random.default_rng(11)
    a = rng.standard_normal((T, d)).astype(np.float16)
    w = (0.02 * rng.standard_normal((V, d))).astype(np.float16)
    bias = (0.5 * rng.standard_normal(V)).astype(np.float32)
    cu = np.array([0, 37, 128, 129, 250, 300], dtype=np.int32)
    return a, w, bias, cu


def test_two_calls_give_the_same_bits(ops, random_case):
    a, w, bias, cu = random_case
    ad, wd, bd, cud = dev(a), dev(w), dev(bias), dev(cu)
    r = ops.splade_head_max_f16(ad, wd, bd, cud).clone()
    for _ in range(3):
        assert torch.equal(ops.splade_head_max_f16(ad, wd, bd, cud), r)      # atomicMax does not depend on the arrival order


def _round_f32(x, up):
    r = x.astype(np.float32)
    wrong = (r.astype(np.float64) < x) if up else (r.astype(np.float64) > x)
    return np.where(wrong, np.nextafter(r, np.float32(np.inf if up else -np.inf)), r).astype(np.float32)


def test_random_data_lies_in_the_float32_accumulation_sandwich(ops, random_case):
    """See the module docstring: no constant for log1pf, only its monotonicity on the device."""
    a, w, bias, cu = random_case
    d = a.shape[1]
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    L = a64 @ w64.T
    B = d * 2.0 ** -23 * (np.abs(a64) @ np.abs(w64).T)
    lo, hi = _round_f32(L - B + bias[None, :].astype(np.float64), up=False), _round_f32(L + B + bias[None, :].astype(np.float64), up=True)
    assert (lo.astype(np.float64) <= L - B + bias).all() and (hi.astype(np.float64) >= L + B + bias).all()
    cud = dev(cu)
    got = ops.splade_head_max_f16(dev(a), dev(w), dev(bias), cud)
    p_lo, p_hi = ops.segment_splade_max(dev(lo), cud), ops.segment_splade_max(dev(hi), cud)
    width = float((p_hi - p_lo).max())
    below, above = int((got < p_lo).sum()), int((got > p_hi).sum())
    print(f"sandwich: max width {width:.3e}, {below} below, {above} above, {int((got > 0).sum())} of {got.numel()} positive")
    assert below == 0 and above == 0
    assert int((got > 0).sum()) > got.numel() // 4


# ---- the encoders ------------------------------------------------------------------------------------------------------------------------
SMALL = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256)      # 64-wide heads: the padding-free forward takes it


def small(kind, **kw):
    from fusion_amd import encoders
    cfg = dict(encoders.TINY, **SMALL)
    g = torch.random.get_rng_state()
    torch.manual_seed(3)
    try:
        tok = encoders.HashTokenizer(cfg["vocab_size"], cfg["pad_token_id"], cfg["bos_token_id"], cfg["eos_token_id"])
        if kind == "dpr":
            return encoders.DenseEncoder(encoders._backbone(cfg), tok, "cuda", **kw)
        return encoders.SpladeEncoder(encoders._backbone(cfg, mlm=True), tok, "cuda", **kw).calibrate_sparsity(per_token=0.02)
    finally:
        torch.random.set_rng_state(g)


def token_batch(vocab, n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n)
    ids = rng.integers(7, vocab - 1, size=(n, hi))
    ids[:, 0] = 5
    return torch.from_numpy(ids).cuda(), lens


def marks_of(enc, ids, lens):
    seen = []
    out = enc.encode_ids_packed(ids, lens, mark=seen.append)
    return out, seen


def test_small_dpr_follows_the_flag():
    ids, lens = token_batch(512, 37, 3, 40, 1)
    plain, off, on = small("dpr"), small("dpr", amp=False), small("dpr", amp=True)
    assert plain.amp is False and off.amp is False and on.amp is True
    e_plain, _ = marks_of(plain, ids, lens)
    e_off, _ = marks_of(off, ids, lens)
    e_on, _ = marks_of(on, ids, lens)
    assert plain._packed.amp_dtype is None and off._packed.amp_dtype is None and plain._packed.hidden16 is None
    assert on._packed.amp_dtype == torch.float16 and on._packed.hidden16 is not None and on._packed.hidden16.dtype == torch.float16
    assert torch.equal(e_plain, e_off)                               # amp=False is today's encoder, bit for bit
    assert not torch.equal(e_on, e_off) and e_on.dtype == torch.float32
    # encode_ids_corpus goes through the same hook
    assert torch.equal(on.encode_ids_corpus(ids, lens), e_on) and torch.equal(off.encode_ids_corpus(ids, lens), e_off)
    cos = torch.nn.functional.cosine_similarity(e_on, e_off, dim=1)
    print(f"small DPR amp vs fp32: max |delta| {float((e_on - e_off).abs().max()):.3e}, min cosine {float(cos.min()):.6f}")


def test_small_splade_follows_the_flag():
    ids, lens = token_batch(512, 37, 3, 40, 2)
    plain, off, on = small("splade"), small("splade", amp=False), small("splade", amp=True)
    e_plain, m_plain = marks_of(plain, ids, lens)
    e_off, m_off = marks_of(off, ids, lens)
    e_on, m_on = marks_of(on, ids, lens)
    assert torch.equal(e_plain, e_off) and m_plain == m_off
    assert "splade_head_pool" in m_off and "splade_head_pool_f16" not in m_off and off._packed.amp_dtype is None
    assert "splade_head_pool_f16" in m_on and "splade_head_pool" not in m_on and on._packed.amp_dtype == torch.float16
    assert e_on.shape == e_off.shape == (37, 512) and not torch.equal(e_on, e_off)
    # a head that is not fused keeps the float32 head on the float32 stream: only the backbone is mixed
    on.FUSED_HEAD = False
    e_unfused, m_unfused = marks_of(on, ids, lens)
    assert "splade_head_pool" in m_unfused and "splade_head_pool_f16" not in m_unfused and on._packed.amp_dtype == torch.float16
    print(f"small SPLADE amp vs fp32: max |delta| {float((e_on - e_off).abs().max()):.3e} (fused f16 head), "
          f"{float((e_unfused - e_off).abs().max()):.3e} (f32 head on the mixed backbone); non-zeros {int((e_on > 0).sum())} / {int((e_off > 0).sum())}")


# Base-size encoders at 64 queries against a corpus a random-init encoder can separate (test_gpu_tables' ColBERT construction: every gold
# document begins with a prefix of its query's tokens).  The bounds below are 4 x the values MEASURED on an MI355X with these seeds (float16
# rounding noise moves by small factors between seeds; the encoders' other amp tests use margins of this kind), the overlap bound is the
# measured mean top-10 overlap minus 0.05.  The measured values are recorded in DESIGN.md section 3 ("Mixed-precision DPR and SPLADE
# encoders"); the float32 encoder finds 0.73 (DPR) / 0.52 (SPLADE) of the gold documents in its top 10, where chance is 10 / 768.
MEASURED = {
    "dpr": dict(max_abs=1.6823e-03, max_rel=4.8159e-04, cos_abs=1.6272e-05, overlap=0.9969),
    "splade": dict(max_abs=1.6947e-03, max_rel=4.5981e-03, cos_abs=2.1002e-03, overlap=0.9969, nnz_rel=6.25e-02),
}


@pytest.mark.parametrize("kind", ["dpr", "splade"])
def test_base_encoder_amp_against_float32(ops, kind):
    from fusion_amd import encoders
    rng = np.random.default_rng(23)
    N, Q, Lq, Ld, V = 768, 64, 32, 48, 32000
    enc = encoders.random_init(kind, device="cuda", size="base", seed=5, amp=True)
    assert enc.amp is True
    if kind == "splade":
        enc.calibrate_sparsity()
    doc_ids = rng.integers(7, V - 1, size=(N, Ld))
    dlens = rng.integers(30, Ld + 1, N)
    q_ids = rng.integers(7, V - 1, size=(Q, Lq))
    gold = rng.permutation(N)[: 2 * Q].reshape(Q, 2)
    for q in range(Q):
        for g in gold[q]:
            n_shared = int(rng.choice((6, 8, 12, 16, 24)))
            doc_ids[g, 1: 1 + n_shared] = q_ids[q, 1: 1 + n_shared]
    dids, qids, qlens = torch.from_numpy(doc_ids).cuda(), torch.from_numpy(q_ids).cuda(), np.full(Q, Lq)
    emb, scores, seen = {}, {}, {}
    for amp in (True, False):
        enc.amp = amp
        seen[amp] = []
        qe = enc.encode_ids_packed(qids, qlens, mark=seen[amp].append)
        assert enc._packed.amp_dtype == (torch.float16 if amp else None)
        de = enc.encode_ids_corpus(dids, dlens) if kind == "dpr" else enc.encode_ids_packed(dids, dlens)
        emb[amp], scores[amp] = qe, ops.cos_scores(qe, de)
    if kind == "splade":
        assert "splade_head_pool_f16" in seen[True] and "splade_head_pool" in seen[False] and "splade_head_pool_f16" not in seen[False]
    e16, e32, s16, s32 = emb[True], emb[False], scores[True], scores[False]
    max_abs = float((e16 - e32).abs().max())
    max_rel = float((e16 - e32).norm(dim=1).div(e32.norm(dim=1).clamp_min(1e-12)).max())      # per query vector, in the l2 norm
    cos_abs = float((s16 - s32).abs().max())
    t16, t32 = torch.topk(s16, 10, dim=1).indices.cpu().numpy(), torch.topk(s32, 10, dim=1).indices.cpu().numpy()
    overlap = float(np.mean([len(set(a.tolist()) & set(b.tolist())) / 10 for a, b in zip(t16, t32)]))
    found = float(np.mean([len(set(t32[q].tolist()) & set(gold[q].tolist())) / 2 for q in range(Q)]))
    line = f"base {kind} amp vs fp32 at Q = {Q}: max |delta| {max_abs:.4e}, max rel (l2, per query) {max_rel:.4e}, max |delta cos| {cos_abs:.4e}, " \
           f"mean top-10 overlap {overlap:.4f}, fp32 gold in top-10 {found:.4f}"
    m = MEASURED[kind]
    if kind == "splade":
        n16, n32 = (e16 > 0).sum(dim=1).float(), (e32 > 0).sum(dim=1).float()
        nnz_rel = float(((n16 - n32).abs() / n32.clamp_min(1)).max())
        line += f", non-zeros per query {float(n16.mean()):.1f} / {float(n32.mean()):.1f} (max rel diff {nnz_rel:.4e})"
    print(line)
    assert found >= 0.25                                 # the float32 encoder does the task (chance: 0.013): the overlap compares rankings that mean something
    assert max_abs <= 4 * m["max_abs"] and max_rel <= 4 * m["max_rel"] and cos_abs <= 4 * m["cos_abs"]
    assert overlap >= m["overlap"] - 0.05
    if kind == "splade":
        assert nnz_rel <= 4 * m["nnz_rel"]


# ---- Ranker.single_vector_search -----------------------------------------------------------------------------------------------------------
def _texts(rng, n, lo, hi):
    return [" ".join(f"w{int(x)}" for x in rng.integers(0, 400, int(rng.integers(lo, hi)))) for _ in range(n)]


@pytest.mark.parametrize("kind", ["dpr", "splade"])
def test_single_vector_search_with_an_injected_encoder(ops, kind, tmp_path):
    from fusion_amd.retrievers.hybrid import Ranker, _rank_scores
    rng = np.random.default_rng(4)
    docs, queries = _texts(rng, 60, 10, 40), _texts(rng, 7, 3, 12)
    corpus = {100 + i: t for i, t in enumerate(docs)}
    enc = small(kind)
    name = f"synthetic-{kind}"
    # today's lists: the same calls single_vector_search made before it knew about precision
    if kind == "dpr":
        scores = ops.cos_scores(enc.encode(queries, batch_size=64, query_mode=True), enc.encode(docs, batch_size=64, query_mode=False))
    else:
        dn = ops.normalize_rows(ops.pad_dim(enc.encode(docs, batch_size=64, query_mode=False)))
        qe = enc.encode(queries, batch_size=64, query_mode=True)
        if ops.density(dn[:, :enc.dim]) > Ranker.SPARSE_DENSITY:
            scores = ops.dot_scores(ops.normalize_rows(qe), dn)
        else:
            scores = ops.sparse_cos_scores(qe, ops.sparse_index(dn, enc.dim))
    plain = Ranker.single_vector_search(queries, corpus, name, encoder=enc)
    assert plain == _rank_scores(scores, np.array(list(corpus.keys())), None).to_lists()
    # an injected encoder keeps its own setting, whatever `amp` says
    assert Ranker.single_vector_search(queries, corpus, name, encoder=enc, amp=True) == plain
    # the two precisions write different cache files, and a float32 cache answers a float32 run only
    cache = str(tmp_path / "cache")
    assert Ranker.single_vector_search(queries, corpus, name, encoder=enc, cache_dir=cache) == plain
    f32_files = set(os.listdir(cache))
    assert f32_files
    mixed = small(kind, amp=True)
    got = Ranker.single_vector_search(queries, corpus, name, encoder=mixed, cache_dir=cache)
    both = set(os.listdir(cache))
    assert len(both) == 2 * len(f32_files) and f32_files < both
    assert {f.split(".")[0] for f in both - f32_files}.isdisjoint({f.split(".")[0] for f in f32_files})
    assert Ranker.single_vector_search(queries, corpus, name, encoder=enc, cache_dir=cache) == plain      # (served from the float32 files)
    assert len(got) == len(plain) and all(len(a) == len(b) for a, b in zip(got, plain))
