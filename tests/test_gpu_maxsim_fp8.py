"""e4m3 MaxSim on the GPU (csrc/maxsim8.hip): the quantiser on every float16 pattern, the all-pairs kernel bit for bit at every tile,
wave and document-range edge, the descale, unit-norm data at the float16 kernel's bar, special values, and Ranker.multi_vector_search
with fp8=True.

On the grid inputs of maxsim_fp8_cases.py (integers in {-2 .. 2}, poison rows carrying 448 in eight dimensions) every partial sum is an
integer below 2^24, so the bar is np.array_equal with the float64 formula whatever the order of the 128 terms inside the 16x16x128 MFMA:
a wrong tile edge, mask, ring slot, operand lane map or scale moves a score by thousands.  The case table and its branch coverage are
checked without a GPU in test_maxsim_fp8_cpu.py."""
import numpy as np
import pytest
import torch

import maxsim_cases as M
import maxsim_fp8_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()       # (a copy: the shared case arrays are read-only)


def tol(Lq):
    return 1e-4 * max(1, Lq / 32)      # the float16 kernel's bar (test_gpu_maxsim_edges.py)


def run(ops, Q8, D8, Doff, max_doc_len, **kw):
    return ops.maxsim_e4m3(dev(Q8), dev(D8), dev(Doff), max_doc_len=max_doc_len, **kw).cpu().numpy()


def mismatches(got, ref):
    bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    return len(bad), [(int(q), int(d), float(got[q, d]), float(ref[q, d])) for q, d in bad[:8]]


# ---- 1. the quantiser ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [0, 8, -8, 15])
def test_quantiser_on_every_float16_pattern(ops, e):
    x = F.all_f16_patterns()
    ref = F.quantize_ref(x, e)
    got = ops.quantize_e4m3(dev(x), e)
    assert got.dtype == torch.uint8 and tuple(got.shape) == x.shape
    got = got.cpu().numpy()
    bad = np.argwhere(got != ref)
    assert np.array_equal(got, ref), (len(bad), [(hex(int(x.view(np.uint16)[r, c])), int(got[r, c]), int(ref[r, c])) for r, c in bad[:8]])


def test_quantiser_shapes_tails_and_views(ops):
    """Sizes that are no multiple of the eight values a lane takes, a source that is not 16-byte aligned, the default exponent, and
    dequantize_e4m3 / a float8_e4m3fn view of the bytes."""
    x = F.all_f16_patterns().reshape(-1)
    xd = dev(x)
    for n, off in ((1, 0), (7, 0), (9, 0), (1001, 0), (65535, 1), (4099, 3)):
        got = ops.quantize_e4m3(xd[off: off + n]).cpu().numpy()
        assert np.array_equal(got, F.quantize_ref(x[off: off + n], 8)), (n, off)
    assert ops.quantize_e4m3(xd[:0]).numel() == 0
    b = torch.arange(256, dtype=torch.uint8, device="cuda")
    for e in (0, 8, -3):
        exp = F.dequantize_ref(np.arange(256, dtype=np.uint8), e).astype(np.float32)
        assert np.array_equal(ops.dequantize_e4m3(b, e).cpu().numpy(), exp, equal_nan=True)
        assert np.array_equal(ops.dequantize_e4m3(b.view(torch.float8_e4m3fn), e).cpu().numpy(), exp, equal_nan=True)


# ---- 2. grid inputs: equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_grid_case_is_exact(ops, case):
    Q8, D8, Doff = F.bytes_of(case)
    ref = F.exact_f32(F.reference(case))
    got = run(ops, Q8, D8, Doff, case.max_doc_len, q_exp=0, d_exp=0)
    assert np.array_equal(got, ref), (case.id,) + mismatches(got, ref)


def test_float8_tensors_are_taken_as_bytes(ops):
    c = next(c for c in F.CASES if c.name == "end-both" and c.Lq == 64)
    Q8, D8, Doff = F.bytes_of(c)
    ref = F.exact_f32(F.maxsim_ref(*F.values(c), None))
    got = ops.maxsim_e4m3(dev(Q8).view(torch.float8_e4m3fn), dev(D8).view(torch.float8_e4m3fn), dev(Doff), q_exp=0, d_exp=0)   # max_doc_len measured
    assert np.array_equal(got.cpu().numpy(), ref)


# ---- 3. the descale ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_exp,d_exp", [(8, 8), (6, 8)])
@pytest.mark.parametrize("case", F.DESCALE_CASES, ids=lambda c: c.id)
def test_quarter_tokens_give_the_float16_formula(ops, case, q_exp, d_exp):
    """Multiples of 1/4 quantise without loss at 2^8 (queries: at 2^6 too), so the score over the bytes, descaled by 2^-(q_exp + d_exp),
    is the float64 formula over the float16 tokens, bit for bit; the bytes come from the device quantiser."""
    Qh, Dh, Doff = F.quarter_tokens(case)
    ref = F.exact_f32(F.maxsim_ref(Qh, Dh, Doff, case.max_doc_len))
    Q8, D8 = ops.quantize_e4m3(dev(Qh), q_exp), ops.quantize_e4m3(dev(Dh), d_exp)
    assert np.array_equal(Q8.cpu().numpy(), F.quantize_ref(Qh, q_exp)) and np.array_equal(D8.cpu().numpy(), F.quantize_ref(Dh, d_exp))
    got = ops.maxsim_e4m3(Q8, D8, dev(Doff), q_exp=q_exp, d_exp=d_exp, max_doc_len=case.max_doc_len).cpu().numpy()
    assert np.array_equal(got, ref), (case.id,) + mismatches(got, ref)
    if (q_exp, d_exp) == (8, 8):
        assert np.array_equal(ops.maxsim_e4m3(Q8, D8, dev(Doff), max_doc_len=case.max_doc_len).cpu().numpy(), ref), "the defaults are 8 and 8"


def test_negative_and_extreme_descales(ops):
    c = next(c for c in F.CASES if c.name == "end-both" and c.Lq == 32)
    Q8, D8, Doff = F.bytes_of(c)
    ref = F.reference(c)
    for q_exp, d_exp in ((-8, -8), (15, 15), (-8, 3)):
        exp = F.exact_f32(ref * 2.0 ** -(q_exp + d_exp))
        assert np.array_equal(run(ops, Q8, D8, Doff, c.max_doc_len, q_exp=q_exp, d_exp=d_exp), exp), (q_exp, d_exp)


# ---- 4. unit-norm tokens -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Q", [(32, 33), (64, 19), (128, 9)])
def test_unit_norm_tokens_against_the_dequantised_formula(ops, Lq, Q):
    rng = np.random.default_rng(800 + Lq)
    lens = [int(x) for x in rng.integers(1, 201, 40)]
    Qtok = M.unit_queries(rng, Q, Lq)
    Dtok, Doff = M.unit_corpus(rng, lens, pre=3, post=9)
    Q8, D8 = ops.quantize_e4m3(dev(Qtok)), ops.quantize_e4m3(dev(Dtok))
    assert np.array_equal(Q8.cpu().numpy(), F.quantize_ref(Qtok, 8)) and np.array_equal(D8.cpu().numpy(), F.quantize_ref(Dtok, 8))
    ref = F.maxsim_ref(F.dequantize_ref(Q8.cpu().numpy(), 8), F.dequantize_ref(D8.cpu().numpy(), 8), Doff, 512)
    got = ops.maxsim_e4m3(Q8, D8, dev(Doff), max_doc_len=512).cpu().numpy()
    err = float(np.max(np.abs(got - ref)))
    f16 = float(np.max(np.abs(got - F.maxsim_ref(Qtok, Dtok, Doff, 512))))
    print(f"unit-norm e4m3 Lq={Lq} Q={Q}: max |got - ref(dequantised)| = {err:.3e} (bar {tol(Lq):.1e}); against the float16 tokens {f16:.3e}")
    assert err <= tol(Lq)


# ---- 5. special values -------------------------------------------------------------------------------------------------------------------
def test_special_values(ops):
    """A NaN byte makes its row's dot products NaN and the maximum skips them (fmaxf); a document of NaN rows only leaves the empty
    maximum, -inf, per query token; rows saturated at +-448 are ordinary numbers."""
    Q8, D8, Doff = F.special_bytes()
    pinned = F.maxsim_fmax_ref(F.dequantize_ref(Q8), F.dequantize_ref(D8), Doff)
    got = run(ops, Q8, D8, Doff, 512, q_exp=0, d_exp=0).astype(np.float64)
    print("pinned:\n", pinned, "\nkernel:\n", got)
    assert np.array_equal(got, pinned), mismatches(got, pinned)
    assert np.isneginf(got[:, 2]).all() and np.isfinite(got[:, 1]).all() and not got[:, 4].any()


# ---- 6. determinism and the output plane -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", F.LQS)
def test_two_launches_agree_and_padding_is_untouched(ops, Lq):
    c = next(c for c in F.CASES if c.name == "empty" and c.Lq == Lq)
    Q8, D8, Doff = F.bytes_of(c)
    Q, N = c.Q, len(c.lens)
    ref = F.exact_f32(F.reference(c))
    q, d, o = dev(Q8), dev(D8), dev(Doff)
    buf = torch.full((Q + 1, N + 5), float("nan"), dtype=torch.float32, device="cuda")
    out = ops.maxsim_e4m3(q, d, o, q_exp=0, d_exp=0, out=buf[:Q, :N], max_doc_len=c.max_doc_len)
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:Q, :N], ref), "a score is wrong or was not stored (empty documents and thin query groups included)"
    assert np.isnan(got[:Q, N:]).all() and np.isnan(got[Q]).all(), "a store outside [Q, N]"
    again = ops.maxsim_e4m3(q, d, o, q_exp=0, d_exp=0, max_doc_len=c.max_doc_len).cpu().numpy()
    assert np.array_equal(again, got[:Q, :N])
    rng = np.random.default_rng(Lq)
    U8 = ops.quantize_e4m3(dev(M.unit_queries(rng, Q, Lq)))
    D, off = M.unit_corpus(rng, c.lens)
    V8 = ops.quantize_e4m3(dev(D))
    a, b = (ops.maxsim_e4m3(U8, V8, dev(off), max_doc_len=64).cpu().numpy() for _ in range(2))
    assert np.array_equal(a, b), "two calls differ"


# ---- 7. the ColBERT search path ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colbert(ops):
    """A tiny random-init ColBERT encoder, built as test_gpu_maxsim_edges.py builds its own."""
    from fusion_amd import encoders
    cfg = dict(encoders.TINY, hidden_size=128, num_attention_heads=2, intermediate_size=256)
    torch.manual_seed(11)
    tok = encoders.HashTokenizer(cfg["vocab_size"])
    punct = (tok._tok("w3"), tok._tok("w7"))
    enc = encoders.ColbertEncoder(encoders._backbone(cfg), tok, "cuda", punct_ids=punct, amp=False)
    rng = np.random.default_rng(12)
    words = [f"w{i}" for i in range(40)]
    docs = [" ".join(rng.choice(words, int(k))) for k in rng.integers(1, 120, size=70)]
    docs[9], docs[10] = "w3 w7 w3 w3", "w7"
    corpus = {1000 + 3 * i: t for i, t in enumerate(docs)}
    queries = [" ".join(rng.choice(words, int(k))) for k in rng.integers(1, 30, size=9)]
    return enc, corpus, queries


@pytest.mark.parametrize("return_topk", [None, 10])
def test_multi_vector_search_fp8(ops, colbert, return_topk, tmp_path):
    from fusion_amd.retrievers.hybrid import Ranker, _rank_scores
    enc, corpus, queries = colbert
    ids = np.array(list(corpus.keys()))
    Dtok, Doff = (t.cuda() for t in enc.encode_docs(list(corpus.values()), batch_size=64))
    Qtok = enc.encode_queries(queries, batch_size=64).cuda()
    scores8 = ops.maxsim_e4m3(ops.quantize_e4m3(Qtok), ops.quantize_e4m3(Dtok), Doff, max_doc_len=enc.max_doc_length)
    exp8 = _rank_scores(scores8, ids, return_topk).to_lists()
    exp16 = _rank_scores(ops.maxsim(Qtok, Dtok, Doff, max_doc_len=enc.max_doc_length), ids, return_topk).to_lists()
    got8 = Ranker.multi_vector_search(queries, corpus, "random-colbert", return_topk=return_topk, encoder=enc, fp8=True)
    assert got8 == exp8                                                      # ids and scores, identical
    assert len(got8) == len(queries) and all(len(lst) == (return_topk or len(corpus)) for lst in got8)
    for fp8_kw in ({}, dict(fp8=False)):
        assert Ranker.multi_vector_search(queries, corpus, "random-colbert", return_topk=return_topk, encoder=enc, **fp8_kw) == exp16
    assert got8 != exp16, "the e4m3 scores equal the float16 ones on random tokens: the flag does nothing"
    # the cache holds the float16 matrix under the same key: a cache written by one route serves the other
    cache = str(tmp_path)
    assert Ranker.multi_vector_search(queries, corpus, "random-colbert", return_topk=return_topk, encoder=enc, cache_dir=cache) == exp16
    assert Ranker.multi_vector_search(queries, corpus, "random-colbert", return_topk=return_topk, encoder=enc, cache_dir=cache, fp8=True) == exp8
    s8 = scores8.cpu().numpy()
    s16 = ops.maxsim(Qtok, Dtok, Doff, max_doc_len=enc.max_doc_length).cpu().numpy()
    print(f"tiny ColBERT encoder: max |s_e4m3 - s_f16| = {np.abs(s8 - s16).max():.3e}, score range {s16.min():.2f} .. {s16.max():.2f}")
