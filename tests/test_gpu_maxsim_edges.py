"""Exact MaxSim (csrc/maxsim.hip) bit for bit at every tile, wave and document-range edge.

On grid-valued inputs (maxsim_cases.py: multiples of 1/4, poison rows carrying 1024 in one dimension) every product, partial sum and sum
of maxima is exact in fp32 in any order, so the bar is np.array_equal with the float64 formula over the whole [Q, N] plane: a masked
row, a truncated tail, a neighbouring document or a clamped row that leaks into a maximum moves a score by ~1024 * Lq.  The cases land
every branch listed in maxsim_cases.BRANCHES (test_branch_table_is_covered; the same check runs without a GPU in
test_maxsim_reference_cpu.py).  A second sweep runs the product's real inputs (unit-norm fp16 tokens) at the parity suite's bar,
1e-4 * max(1, Lq / 32), and the raw C ABI cases pin strides, refusals and special values."""
import ctypes as C

import numpy as np
import pytest
import torch

import maxsim_cases as M
from helpers import assert_ranked_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tol(Lq):
    return 1e-4 * max(1, Lq / 32)      # test_maxsim_vs_oracle's bar


def run(ops, Qtok, Dtok, Doff, max_doc_len):
    return ops.maxsim(dev(Qtok), dev(Dtok), dev(Doff), max_doc_len=max_doc_len).cpu().numpy()


def test_branch_table_is_covered():
    hit = set()
    for c in M.CASES:
        b = M.branches_of(c)
        assert set(c.claims) <= b, (c.id, sorted(map(str, set(c.claims) - b)))
        hit |= b
    assert set(M.BRANCHES) <= hit, sorted(map(str, set(M.BRANCHES) - hit))


# ---- grid inputs: equality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.id)
def test_grid_case_is_exact(ops, case):
    Qtok, Dtok, Doff = case.inputs()
    ref = M.exact_f32(M.maxsim_ref(Qtok, Dtok, Doff, case.max_doc_len))
    got = run(ops, Qtok, Dtok, Doff, case.max_doc_len)
    bad = np.argwhere(got != ref)
    assert np.array_equal(got, ref), (case.id, len(bad), [(int(q), int(d), float(got[q, d]), float(ref[q, d])) for q, d in bad[:8]])


def test_default_max_doc_len_is_the_longest_document(ops):
    """ops.maxsim without max_doc_len measures it from Doff (here with Doff[0] > 0 and rows beyond Doff[N])."""
    c = next(c for c in M.CASES if c.name == "end-both" and c.Lq == 64)
    Qtok, Dtok, Doff = c.inputs()
    ref = M.exact_f32(M.maxsim_ref(Qtok, Dtok, Doff, None))
    assert np.array_equal(ops.maxsim(dev(Qtok), dev(Dtok), dev(Doff)).cpu().numpy(), ref)


# ---- unit-norm inputs: the parity bar, run-to-run bits -------------------------------------------------------------------------
UNIT_LENS = M.alternate(M.EDGE_LENS, guard=(0, 20, 100, 7)) + (45,)
UNIT_CASES = [(Lq, Q) for Lq in M.LQS for Q in M.FILL_Q[Lq]] + [(64, 195)]


@pytest.mark.parametrize("Lq,Q", UNIT_CASES)
def test_unit_norm_sweep(ops, Lq, Q):
    rng = np.random.default_rng(Lq * 1000 + Q)
    Qtok = M.unit_queries(rng, Q, Lq)
    Dtok, Doff = M.unit_corpus(rng, UNIT_LENS, pre=3, post=9)
    for m in (512, 40):      # every document whole; the longer ones truncated
        ref = M.maxsim_ref(Qtok, Dtok, Doff, m)
        got = run(ops, Qtok, Dtok, Doff, m)
        err = float(np.max(np.abs(got - ref)))
        print(f"unit-norm Lq={Lq} Q={Q} max_doc_len={m}: max |got - ref| = {err:.3e} (bar {tol(Lq):.1e})")
        assert err <= tol(Lq)
        assert np.array_equal(got, run(ops, Qtok, Dtok, Doff, m)), "two calls differ"


# ---- a score does not depend on where its query or document sits ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grid", "unit"])
@pytest.mark.parametrize("Lq", M.LQS)
def test_scores_do_not_depend_on_position(ops, Lq, kind):
    """The plane of Q queries x N documents, then the same pairs with the query alone in its group (another wave, another column
    block), the document alone in its range, and the corpus shifted by five documents and 37 token rows (another place in the range,
    another range, another alignment of the tiles in memory).  Exact on the grid; on unit-norm data it is the kernel's own claim that
    every wave runs the same chain."""
    rng = np.random.default_rng(Lq + (kind == "unit"))
    Q = 2 * 8 * (128 // Lq) - 1
    lens = [int(x) for x in rng.integers(0, 130, 70)]
    lens[3], lens[40] = 0, 512
    if kind == "grid":
        Qtok = M.grid_queries(rng, Q, Lq)
        Dtok, Doff = M.grid_corpus(rng, lens, 512)
    else:
        Qtok = M.unit_queries(rng, Q, Lq)
        Dtok, Doff = M.unit_corpus(rng, lens)
    m = 100      # the 512-token document and a few others are truncated
    plane = run(ops, Qtok, Dtok, Doff, m)
    if kind == "grid":
        assert np.array_equal(plane, M.exact_f32(M.maxsim_ref(Qtok, Dtok, Doff, m)))
    for q in sorted({0, 1, 2, 3, 5, Q // 2, Q - 2, Q - 1}):
        assert np.array_equal(run(ops, Qtok[q: q + 1], Dtok, Doff, m), plane[q: q + 1]), ("query alone", q)
    for d in (0, 1, 3, 31, 32, 40, 63, 64, 69):
        a, b = int(Doff[d]), int(Doff[d + 1])
        one = np.concatenate([Dtok[a:b], Dtok[:1]])     # (a token matrix is never empty here; the extra row is outside the document)
        assert np.array_equal(run(ops, Qtok, one, np.array([0, b - a], dtype=np.int64), m), plane[:, d: d + 1]), ("document alone", d)
    head = [int(x) for x in rng.integers(1, 60, 5)]
    pre = 37
    shifted = np.concatenate([Dtok[: pre + sum(head)], Dtok])      # 37 rows outside any document, five other documents, the corpus
    off2 = np.concatenate([pre + np.concatenate([[0], np.cumsum(head)])[:-1], pre + sum(head) + Doff]).astype(np.int64)
    assert np.array_equal(run(ops, Qtok, shifted, off2, m)[:, 5:], plane), "corpus shifted"


# ---- the raw C ABI -----------------------------------------------------------------------------------------------------------
def _abi():
    from fusion_amd import _lib
    return _lib, _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("Lq", M.LQS)
@pytest.mark.parametrize("pad", ["N+5", "round_up(N,4)+4"])
def test_c_abi_strided_output_is_written_exactly(ops, Lq, pad):
    """lds > N: every [q, d < N] is written -- empty documents and thinly filled query groups included, the buffer starts as NaN --
    and nothing else is: columns >= N and the row after the plane keep their NaN."""
    _lib, L, st = _abi()
    c = next(c for c in M.CASES if c.name == "empty" and c.Lq == Lq)
    Qtok, Dtok, Doff = c.inputs()
    Q, N = c.Q, len(c.lens)
    lds = N + 5 if pad == "N+5" else (N + 3) // 4 * 4 + 4
    ref = M.exact_f32(M.maxsim_ref(Qtok, Dtok, Doff, c.max_doc_len))
    q, d, o = dev(Qtok), dev(Dtok), dev(Doff)
    buf = torch.full((Q + 1, lds), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.fz_maxsim_f16(q.data_ptr(), d.data_ptr(), o.data_ptr(), d.shape[0], c.max_doc_len, Q, Lq, N, 128, buf.data_ptr(), lds, st)
    assert rc == _lib.FZ_OK
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert not np.isnan(got[:Q, :N]).any(), "a score was not stored"
    assert np.array_equal(got[:Q, :N], ref)
    assert np.isnan(got[:Q, N:]).all() and np.isnan(got[Q]).all(), "a store outside [Q, N]"


def test_c_abi_refusals_leave_the_output_untouched(ops):
    """Every documented refusal returns its status before any launch and writes nothing."""
    _lib, L, st = _abi()
    OK, ARG, UNS = _lib.FZ_OK, _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED
    Q, N, lds = 3, 4, 8
    q = torch.zeros((Q * 256 * 128 + 8,), dtype=torch.float16, device="cuda")       # room for Lq = 256 and a base 2 bytes further
    d = torch.zeros((64 * 128 + 8,), dtype=torch.float16, device="cuda")
    o = dev(np.array([0, 10, 30, 30, 64], dtype=np.int64))
    buf = torch.full((Q + 1, lds), float("nan"), dtype=torch.float32, device="cuda")

    def call(Qp=None, Dp=None, sumL=64, m=64, Q_=Q, Lq=64, N_=N, dim=128, lds_=lds):
        rc = L.fz_maxsim_f16(q.data_ptr() if Qp is None else Qp, d.data_ptr() if Dp is None else Dp, o.data_ptr(), sumL, m, Q_, Lq, N_, dim,
                             buf.data_ptr(), lds_, st)
        torch.cuda.synchronize()
        return rc

    assert q.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
    refusals = [("dim 64", dict(dim=64), UNS), ("dim 256", dict(dim=256), UNS)]
    refusals += [(f"Lq {Lq}", dict(Lq=Lq), UNS) for Lq in (16, 48, 96, 256)]
    refusals += [("Dtok 2 bytes off", dict(Dp=d.data_ptr() + 2), UNS), ("Qtok 2 bytes off", dict(Qp=q.data_ptr() + 2), UNS),
                 ("lds < N", dict(lds_=N - 1), ARG), ("max_doc_len 0", dict(m=0), ARG), ("max_doc_len -1", dict(m=-1), ARG),
                 ("max_doc_len 16,385", dict(m=16385), UNS), ("Q = 0", dict(Q_=0), OK), ("N = 0", dict(N_=0, lds_=0), OK)]
    for what, kw, status in refusals:
        assert call(**kw) == status, what
        assert torch.isnan(buf).all(), (what, "wrote to the output")
    # every document empty, no token matrix: exactly [Q, N] of the strided buffer is zero-filled
    assert call(Dp=0, sumL=0) == OK
    got = buf.cpu().numpy()
    assert not got[:Q, :N].any() and np.isnan(got[:Q, N:]).all() and np.isnan(got[Q]).all()


def test_special_values(ops):
    """Defined by the formula in IEEE arithmetic, and exact here (grid queries; the large rows hold 0 and +-65504 only):
      - a query token of zeros adds max_t 0 = 0;
      - fp16 maximum values: products up to 65504 * 1 stay far inside fp32;
      - +inf in a document row: +inf wherever every query component that meets it is positive.
    Where the formula yields NaN (inf * 0, inf - inf) the kernel's maximum drops the NaN term (fmaxf) while the float64 reference
    propagates it: the kernel's value is pinned as include/fusion_hip.h documents it (maxsim_cases.maxsim_fmax_ref)."""
    Qtok, Dtok, Doff = M.special_inputs()
    Q = Qtok.shape[0]
    ref = M.maxsim_ref(Qtok, Dtok, Doff, 512)
    pinned = M.maxsim_fmax_ref(Qtok, Dtok, Doff)
    got = run(ops, Qtok, Dtok, Doff, 512).astype(np.float64)
    print("float64 reference:\n", ref, "\nkernel:\n", got)
    defined = ~np.isnan(ref)
    assert np.array_equal(ref[defined], pinned[defined])                # the two definitions part only where the formula is NaN
    M.check_special_reference(ref)
    assert np.array_equal(got[defined], ref[defined])
    assert np.array_equal(got, pinned, equal_nan=True)
    assert np.isneginf(got[:, 3]).all()                                 # every term NaN: the empty maximum, -inf


# ---- the ColBERT search path, end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colbert(ops):
    from fusion_amd import encoders
    cfg = dict(encoders.TINY, hidden_size=128, num_attention_heads=2, intermediate_size=256)
    torch.manual_seed(11)
    tok = encoders.HashTokenizer(cfg["vocab_size"])
    punct = (tok._tok("w3"), tok._tok("w7"))
    enc = encoders.ColbertEncoder(encoders._backbone(cfg), tok, "cuda", punct_ids=punct, amp=False)
    rng = np.random.default_rng(11)
    words = [f"w{i}" for i in range(40)]
    kept = [w for w in words if tok._tok(w) not in punct]         # (a hashed word may share its id with a skiplist word)
    dropped = [w for w in words if tok._tok(w) in punct]
    n_words = [int(k) for k in rng.integers(1, 120, size=70)]
    docs = [" ".join(rng.choice(words, k)) for k in n_words]
    for i, k in ((5, 126), (20, 127), (33, 300), (69, 200)):      # nothing for the skiplist: the tokenizer cuts them at max_doc_length
        docs[i] = " ".join(rng.choice(kept, k))
    docs[9], docs[10], docs[50] = "w3 w7 w3 w3", "w7", " ".join(rng.choice(dropped, 150))   # punctuation only: bos and eos are left
    corpus = {1000 + 3 * i: t for i, t in enumerate(docs)}
    queries = [" ".join(rng.choice(words, int(k))) for k in rng.integers(1, 30, size=9)]
    return enc, corpus, queries


def _kept_tokens(enc, text):
    ids = [enc.tokenizer._tok(w) for w in text.split()][: enc.max_doc_length - 2]
    return 2 + sum(i not in enc.punct_ids.tolist() for i in ids)


def _reference_lists(enc, corpus, queries, max_doc_len, k):
    Dtok, Doff = enc.encode_docs(list(corpus.values()), batch_size=64)
    Qtok = enc.encode_queries(queries, batch_size=64)
    S = M.maxsim_ref(Qtok.cpu().numpy(), Dtok.cpu().numpy(), Doff.cpu().numpy(), max_doc_len)
    ids = np.array(list(corpus.keys()))
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return Doff.cpu().numpy(), [(ids[o], S[q, o]) for q, o in enumerate(order)]


@pytest.mark.parametrize("return_topk", [None, 10])
def test_multi_vector_search_end_to_end(ops, colbert, return_topk):
    from fusion_amd.retrievers.hybrid import Ranker
    enc, corpus, queries = colbert
    N = len(corpus)
    k = N if return_topk is None else return_topk
    Doff, exp = _reference_lists(enc, corpus, queries, enc.max_doc_length, k)
    lens = np.diff(Doff)
    assert enc.max_doc_length == 128 and enc.max_query_length == 64
    assert lens.tolist() == [_kept_tokens(enc, t) for t in corpus.values()]
    assert lens.max() == enc.max_doc_length and (lens == enc.max_doc_length).sum() >= 3 and (lens == 2).sum() >= 3
    got = Ranker.multi_vector_search(queries, corpus, "random-colbert", return_topk=return_topk, encoder=enc, as_device=False)
    assert len(got) == len(queries)
    for lst, (e_ids, e_sc) in zip(got, exp):
        assert len(lst) == k
        assert_ranked_close([x["corpus_id"] for x in lst], [x["score"] for x in lst], e_ids, e_sc, tol(64), truncated=k < N)


def test_multi_vector_search_truncates_stored_documents(ops, colbert, tmp_path):
    """max_doc_length lowered after the corpus was encoded and cached: the stored documents exceed it, and the ranking is that of the
    documents cut at the new length."""
    from fusion_amd.retrievers.hybrid import Ranker
    enc, corpus, queries = colbert
    N = len(corpus)
    Doff, whole = _reference_lists(enc, corpus, queries, enc.max_doc_length, N)
    _, cut = _reference_lists(enc, corpus, queries, 40, N)
    assert (np.diff(Doff) > 40).sum() >= 10
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(whole, cut)), "the cut does not change any ranking: the case shows nothing"
    first = Ranker.multi_vector_search(queries, corpus, "random-colbert", encoder=enc, cache_dir=str(tmp_path))
    for lst, (e_ids, e_sc) in zip(first, whole):
        assert_ranked_close([x["corpus_id"] for x in lst], [x["score"] for x in lst], e_ids, e_sc, tol(64))
    full = enc.max_doc_length
    try:
        enc.max_doc_length = 40
        got = Ranker.multi_vector_search(queries, corpus, "random-colbert", encoder=enc, cache_dir=str(tmp_path))
    finally:
        enc.max_doc_length = full
    for lst, (e_ids, e_sc) in zip(got, cut):
        assert_ranked_close([x["corpus_id"] for x in lst], [x["score"] for x in lst], e_ids, e_sc, tol(64))
