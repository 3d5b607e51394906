"""GPU tests (-m gpu) of pseudo-relevance feedback: fz_sparse_feedback_f32 at every bitmap-word, row-chunk, slot-count and selection
edge, fz_dense_feedback_f32 on its vector and scalar paths, and both end to end through ShardedSparseIndex / ShardedDenseIndex.
Every comparison is bit for bit against the NumPy restatement of tests/feedback_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import feedback_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = (1 << 33) + 5                                              # an id base beyond 2^33
FILL = 0x55


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, exp, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=what)


def _p(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _raw_sparse(c, alpha, m, width=None):
    """fz_sparse_feedback_f32 on output planes that sit between two guard rows and were filled with a byte pattern beforehand
    -> (out_terms [Q, width], out_w [Q, width], out_len [Q], flag word); the guards and the columns past `width` are checked here."""
    from fusion_amd import _lib
    L = _lib.lib()
    Q, F = c["fb_ids"].shape
    if width is None:
        width = min(int((c["qoff"][1:] - c["qoff"][:-1]).max()) + m, c["V"])
    ldo = max((width + 63) // 64 * 64, 64)
    d = {k: _t(c[k]) for k in ("foff", "rows", "qoff", "qterms", "qw", "fb_ids", "coef")}
    fb_len = None if c["fb_len"] is None else _t(c["fb_len"])
    out_t = torch.full((Q + 2, ldo * 4), FILL, dtype=torch.uint8, device=DEV)
    out_w = torch.full((Q + 2, ldo * 4), FILL, dtype=torch.uint8, device=DEV)
    out_len = torch.full((Q + 2,), 0x55555555, dtype=torch.int32, device=DEV)
    flag = torch.full((3,), 0x55555555, dtype=torch.int32, device=DEV)
    rc = L.fz_sparse_feedback_f32(_p(d["foff"]), _p(d["rows"]), c["V"], c["N"], c["id_base"], _p(d["qoff"]), _p(d["qterms"]), _p(d["qw"]), Q,
                                  _p(d["fb_ids"]), F, _p(fb_len), _p(d["coef"]), F, F, alpha, m, C.c_void_p(out_t[1:].data_ptr()),
                                  C.c_void_p(out_w[1:].data_ptr()), ldo, width, C.c_void_p(out_len[1:].data_ptr()),
                                  C.c_void_p(flag[1:].data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    ot, ow, ol, fl = out_t.cpu().numpy(), out_w.cpu().numpy(), out_len.cpu().numpy(), flag.cpu().numpy()
    for b in (ot, ow):
        assert (b[0] == FILL).all() and (b[-1] == FILL).all(), "a guard row was written"
        assert (b[1:-1, width * 4:] == FILL).all(), "a column past `width` was written"
    assert ol[0] == 0x55555555 and ol[-1] == 0x55555555 and fl[0] == 0x55555555 and fl[2] == 0x55555555
    return (ot[1:-1].view(np.int32)[:, :width], ow[1:-1].view(np.float32)[:, :width], ol[1:-1], int(fl[1]))


def _sparse_equals_ref(c, alpha, m, what=""):
    et, ew, el, over = fc.sparse_feedback_ref(c["foff"], c["rows"], c["N"], c["V"], c["id_base"], c["qoff"], c["qterms"], c["qw"], c["fb_ids"],
                                              c["fb_len"], c["coef"], alpha, m)
    assert not over
    gt, gw, gl, flag = _raw_sparse(c, alpha, m)
    assert flag == 0
    _same(gl, el, f"{what} m={m} out_len")
    _same(gt, et, f"{what} m={m} terms")
    _same(gw, ew, f"{what} m={m} weights")
    return et, ew, el


def _ms(c):
    C0 = fc.candidates_of(c)[0]
    return sorted({0, 1, 4096, max(C0 - 1, 0), C0, C0 + 1})


# ---- sparse: shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 32005, 32767, 32768])
def test_sparse_at_every_bitmap_word_edge(V):
    """Random full-mantissa weights and signed coefficients (another order of additions would show), the vocabulary's last term in a
    query and in a document, m at 0, 1, C - 1, C, C + 1 and 4096."""
    rng = np.random.default_rng(V)
    c = fc.random_case(rng, V, 3, [min(V, n) for n in (5, 40, 1, 0, 17, 200)], Q=5, nq=6, id_base=BIG if V % 2 else 0, signed=True)
    last = np.int32(V - 1)
    if c["qoff"][1] > 0 and last not in c["qterms"][:c["qoff"][1]]:
        c["qterms"][c["qoff"][1] - 1] = last                        # query 0 ends on the last term (terms stay ascending and unique)
    if c["foff"][2] > c["foff"][1] and c["rows"][c["foff"][2] - 1, 0] != last:
        c["rows"][c["foff"][2] - 1, 0] = last                       # so does document 1's row
    for m in _ms(c):
        _sparse_equals_ref(c, 0.75, m, f"V={V}")


@pytest.mark.parametrize("F", [0, 1, 2, 3, 8, 65])
def test_sparse_at_every_slot_count(F):
    rng = np.random.default_rng(10 + F)
    c = fc.random_case(rng, 1025, F, rng.integers(0, 60, 30), Q=6, nq=9, id_base=BIG, signed=True)
    for m in _ms(c):
        _sparse_equals_ref(c, 1.0, m, f"F={F}")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_sparse_at_every_row_length(n):
    """Rows of exactly n postings (the slot loop takes 1,024 per pass) next to short ones."""
    rng = np.random.default_rng(20 + n)
    c = fc.random_case(rng, 32005, 4, [n, 3, n, 166, n], Q=4, nq=37, signed=True)
    c["fb_ids"][0] = [0, 2, 4, 3]
    c["fb_len"][0] = 4
    for m in sorted({0, 32, fc.candidates_of(c)[0], 4096}):
        _sparse_equals_ref(c, 1.0, m, f"row length {n}")


# ---- sparse: selection and slot edge cases ---------------------------------------------------------------------------------------------
def _case(docs, queries, fb_ids, V, fb_len=None, coef=None, id_base=0):
    foff, rows = fc.forward_of(docs)
    qoff, qterms, qw = fc.queries_of(queries)
    fb_ids = np.asarray(fb_ids, np.int64)
    coef = np.ones(fb_ids.shape, np.float32) if coef is None else np.asarray(coef, np.float32)
    return dict(foff=foff, rows=rows, N=len(docs), V=V, id_base=id_base, qoff=qoff, qterms=qterms, qw=qw, fb_ids=fb_ids,
                fb_len=None if fb_len is None else np.asarray(fb_len, np.int32), coef=coef)


def test_all_candidates_equal_the_lowest_terms_win():
    terms = np.arange(3, 1500, 7, dtype=np.int32)
    c = _case([(terms, np.ones(len(terms), np.float32))], [([5], [1.0]), ([], [])], [[0], [0]], 2048)
    for m in (1, 2, 50, len(terms) - 1, len(terms)):
        et, _, el = _sparse_equals_ref(c, 1.0, m)
        assert et[1, :m].tolist() == terms[:m].tolist() and el[1] == m


def test_tie_run_at_the_threshold_across_word_and_wave_boundaries():
    """Terms 20 .. 1100 all sum to 1.0, two terms to 2.0: the tie run at the threshold ends at 31 | 32, 63 | 64 and 1023 | 1024."""
    run = np.arange(20, 1101, dtype=np.int32)
    docs = [(run, np.ones(len(run), np.float32)), (np.array([5, 1500], np.int32), np.array([2.0, 2.0], np.float32))]
    c = _case(docs, [([2000], [0.5])], [[0, 1]], 2048)
    for last in (31, 63, 1023):
        for extra in (-1, 0, 1):
            m = 2 + (last - 20 + 1) + extra
            et, _, el = _sparse_equals_ref(c, 1.0, m, f"tie run ending at {last + extra}")
            # the row: 5, the run's lowest m - 2 terms, 1500, the query's 2000
            assert el[0] == m + 1 and et[0, m - 2] == last + extra and et[0, m - 1:m + 1].tolist() == [1500, 2000]


def test_negative_coefficients_cancellation_and_zero_sums():
    w = fc.full_mantissa(np.random.default_rng(1), 6)
    docs = [(np.array([1, 4, 9, 40], np.int32), np.array([w[0], w[1], -0.0, w[2]], np.float32)),
            (np.array([1, 4, 9, 41], np.int32), np.array([w[0], w[3], 0.0, w[4]], np.float32)),
            (np.array([4, 40], np.int32), np.array([w[5], w[2]], np.float32))]
    # term 1: w - w = +0.0; term 9: products of zeros of either sign; term 40: + w, - w; term 4 is a query term and takes three additions
    c = _case(docs, [([4, 7], [0.5, -0.25])], [[0, 1, 2]], 64, coef=[[1.0, -1.0, -1.0]])
    for m in (0, 1, 2, 3, 4, 5):
        et, ew, el = _sparse_equals_ref(c, -1.5, m)
    assert et[0, :el[0]].tolist() == [1, 4, 7, 9, 40, 41]                  # the zero sums are candidates like any other
    assert ew[0, 0] == 0 and ew[0, 3] == 0 and ew[0, 4] == 0
    assert ew[0, 1] == np.float32(np.float32(np.float32(np.float32(-1.5) * np.float32(0.5)) + w[1]) - w[3]) - w[5]


def test_skipped_slots_and_a_query_left_alone():
    rng = np.random.default_rng(2)
    docs = fc.random_docs(rng, 500, [20, 30, 10])
    qs = [(np.array([3, 77, 499], np.int32), fc.full_mantissa(rng, 3)) for _ in range(5)]
    ids = np.array([[-1, BIG - 1, BIG + 3, -7],                 # every slot outside the index
                    [BIG, BIG + 1, BIG + 2, BIG],                # all counted, one document twice
                    [BIG, BIG + 1, BIG + 2, BIG],                # fb_len 0: none counted
                    [BIG, BIG + 1, BIG + 2, BIG],                # fb_len 2
                    [BIG + 2, -1, BIG + 2, BIG + 3]], np.int64)
    c = _case(docs, qs, ids, 500, fb_len=[4, 9, 0, 2, -3], coef=fc.full_mantissa(rng, 20, True).reshape(5, 4), id_base=BIG)
    et, ew, el = _sparse_equals_ref(c, 0.3, 16)
    for q in (0, 2, 4):                                          # alpha * q, nothing else
        assert el[q] == 3 and et[q, :3].tolist() == [3, 77, 499]
        _same(ew[q, :3], np.float32(0.3) * qs[q][1] + np.float32(0))
    assert el[1] > 3 and el[3] > 3


def test_two_runs_give_the_same_bits_and_the_wrapper_equals_the_planes():
    from fusion_amd import ops
    rng = np.random.default_rng(3)
    c = fc.random_case(rng, 32005, 10, rng.integers(100, 240, 64), Q=8, nq=37, id_base=BIG, signed=True)
    a, b = _raw_sparse(c, 1.0, 32), _raw_sparse(c, 1.0, 32)
    for x, y in zip(a[:3], b[:3]):
        _same(x, y)
    et, ew, el = _sparse_equals_ref(c, 1.0, 32)
    fwd = ops.SparseForward(_t(c["foff"]), _t(c["rows"]), c["N"], c["V"])
    args = (_t(c["qoff"]), _t(c["qterms"]), _t(c["qw"]), _t(c["fb_ids"]), _t(c["fb_len"]), _t(c["coef"]), 1.0, 32)
    for got, exp in zip(ops.sparse_feedback(fwd, c["V"], *args, id_base=BIG), fc.csr_of(et, ew, el)):
        _same(got, exp)
    # normalize=True: the rows' weights are what normalize_rows gives for the padded plane
    noff, nt, nw = ops.sparse_feedback(fwd, c["V"], *args, id_base=BIG, normalize=True)
    norm = ops.normalize_rows(_t(ew))[:, :ew.shape[1]].cpu().numpy()
    _same(nt, et[et >= 0])
    _same(nw, norm[et >= 0])
    with pytest.raises(ValueError, match="sparse_feedback_max_vocab"):
        ops.sparse_feedback(fwd, fc.MAX_V + 1, *args)


def test_a_row_that_does_not_fit_raises_the_flag_and_stays_inside_width():
    rng = np.random.default_rng(4)
    c = fc.random_case(rng, 1025, 3, rng.integers(20, 60, 12), Q=4, nq=6)
    c["fb_len"][:] = 3
    et, ew, el, _ = fc.sparse_feedback_ref(c["foff"], c["rows"], c["N"], c["V"], 0, c["qoff"], c["qterms"], c["qw"], c["fb_ids"], c["fb_len"],
                                           c["coef"], 1.0, 8)
    width = int(el.max()) - 1                                    # one short for the longest row
    xt, xw, xl, over = fc.sparse_feedback_ref(c["foff"], c["rows"], c["N"], c["V"], 0, c["qoff"], c["qterms"], c["qw"], c["fb_ids"],
                                              c["fb_len"], c["coef"], 1.0, 8, width=width)
    assert over
    gt, gw, gl, flag = _raw_sparse(c, 1.0, 8, width=width)       # (the guard and past-width checks are _raw_sparse's)
    assert flag == 1
    _same(gt, xt); _same(gw, xw); _same(gl, xl)
    gt, gw, gl, flag = _raw_sparse(c, 1.0, 8, width=width + 1)
    assert flag == 0
    _same(gt, et[:, :width + 1]); _same(gw, ew[:, :width + 1])


# ---- dense -----------------------------------------------------------------------------------------------------------------------
def _dense_case(rng, dim, F, N=37, Q=5, id_base=BIG):
    Qn = fc.full_mantissa(rng, Q * dim, True).reshape(Q, dim)
    Dn = fc.full_mantissa(rng, N * dim, True).reshape(N, dim)
    ids = (rng.integers(0, N, (Q, F)) + id_base).astype(np.int64)
    if F >= 3:
        ids[0, 1], ids[1, 0], ids[1, 2], ids[2, 2] = -1, id_base - 1, id_base + N, ids[2, 0]
    fb_len = rng.integers(0, F + 1, Q).astype(np.int32)
    fb_len[:3] = F
    fb_len[4] = F + 2
    return Qn, Dn, ids, fb_len, fc.full_mantissa(rng, Q * F, True).reshape(Q, F), id_base


@pytest.mark.parametrize("F", [0, 1, 8, 65])
@pytest.mark.parametrize("dim", [1, 3, 4, 5, 255, 256, 257, 768, 1025])
def test_dense_feedback_vector_and_scalar_paths(dim, F):
    from fusion_amd import ops
    rng = np.random.default_rng(1000 * F + dim)
    Qn, Dn, ids, fb_len, coef, base = _dense_case(rng, dim, F)
    exp = fc.dense_feedback_ref(Qn, Dn, base, ids, fb_len, coef, 0.8)
    tid, tl, tc = _t(ids), _t(fb_len), _t(coef)
    _same(ops.dense_feedback(_t(Qn), _t(Dn), tid, tl, tc, 0.8, id_base=base), exp, "contiguous")
    # padded planes: 16-byte aligned rows whatever the dim (the vector path with a short last group)
    pq, pd = ops.alloc_plane(Qn.shape[0], dim, torch.float32, DEV), ops.alloc_plane(Dn.shape[0], dim, torch.float32, DEV)
    pq.copy_(_t(Qn)); pd.copy_(_t(Dn))
    out = torch.full((Qn.shape[0] + 2, 1088), 7.0, device=DEV)
    got = ops.dense_feedback(pq, pd, tid, None if F == 0 else tl, tc, 0.8, id_base=base, out=out[1:-1, :dim])
    _same(got, exp if F else fc.dense_feedback_ref(Qn, Dn, base, ids, None, coef, 0.8), "planes")
    assert (out[0] == 7).all() and (out[-1] == 7).all() and (out[:, dim:] == 7).all()
    # pointers off the 16-byte grid and row strides that are no multiple of 4: the scalar path
    ld = dim + 3 - (dim + 3) % 4 + 1
    bq, bd = torch.zeros(Qn.shape[0] * ld + 1, device=DEV), torch.zeros(Dn.shape[0] * ld + 1, device=DEV)
    uq, ud = bq[1:].view(-1, ld)[:, :dim], bd[1:].view(-1, ld)[:, :dim]
    uq.copy_(_t(Qn)); ud.copy_(_t(Dn))
    _same(ops.dense_feedback(uq, ud, tid, tl, tc, 0.8, id_base=base), exp, "unaligned")


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _corpus(rng, N, V, per_doc, Q, per_query):
    D = np.zeros((N, V), np.float32)
    for d in range(N):
        D[d, rng.choice(V, per_doc, replace=False)] = fc.full_mantissa(rng, per_doc)
    Qm = np.zeros((Q, V), np.float32)
    for q in range(Q):
        Qm[q, rng.choice(V, per_query, replace=False)] = fc.full_mantissa(rng, per_query)
    return D, Qm


@pytest.mark.parametrize("weighting,normalize", [("uniform", True), ("score", False)])
def test_sparse_search_feedback_equals_the_three_steps(weighting, normalize):
    from fusion_amd import feedback, ops
    from fusion_amd.distributed import ShardedSparseIndex
    from fusion_amd.planes import RankedTopk
    rng = np.random.default_rng(5)
    N, V, Q, k, base = 3000, 1500, 7, 40, 1 << 34
    D, Qm = _corpus(rng, N, V, 30, Q, 6)
    Dn, Qn = ops.normalize_rows(_t(D)), ops.normalize_rows(_t(Qm))
    sh = ShardedSparseIndex(ops.sparse_index(Dn, V), base)
    qoff, qterms, qw = ops.sparse_rows(Qn, V)
    with pytest.raises(ValueError, match="build_forward"):
        sh.feedback(qoff, qterms, qw, RankedTopk.from_search(*sh.search(qoff, qterms, qw, k)))
    fwd = sh.build_forward()
    kw = dict(fb_docs=6, fb_terms=12, alpha=0.9, beta=0.6, weighting=weighting, normalize=normalize)
    got = sh.search_feedback(qoff, qterms, qw, k, **kw)
    # by hand: the first search, the restatement on the host, the second search
    first = RankedTopk.from_search(*sh.search(qoff, qterms, qw, k))
    fb_ids, fb_len, coef = feedback.coefficients(first, 6, 0.6, weighting)
    et, ew, el, over = fc.sparse_feedback_ref(fwd.foff.cpu().numpy(), fwd.rows.cpu().numpy(), N, V, base, qoff.cpu().numpy(), qterms.cpu().numpy(),
                                              qw.cpu().numpy(), fb_ids.cpu().numpy(), fb_len.cpu().numpy(), coef.cpu().numpy(), 0.9, 12)
    assert not over and int(el.max()) > 6
    if normalize:
        ew = ops.normalize_rows(_t(ew))[:, :ew.shape[1]].cpu().numpy()
    eoff, eterms, eqw = fc.csr_of(et, ew, el)
    s2, i2 = sh.search(_t(eoff), _t(eterms), _t(eqw), k)
    _same(got.ids, i2); _same(got.scores, s2)
    for g, e in zip(sh.feedback(qoff, qterms, qw, first, **kw), (eoff, eterms, eqw)):
        _same(g, e)
    assert not torch.equal(got.ids, first.ids)                   # the expansion does move the lists


def test_dense_search_feedback_equals_the_three_steps():
    from fusion_amd import feedback, ops
    from fusion_amd.distributed import ShardedDenseIndex
    from fusion_amd.planes import RankedTopk
    rng = np.random.default_rng(6)
    N, dim, Q, k, base = 2500, 64, 9, 30, 1 << 34
    Dn = ops.normalize_rows(_t(rng.normal(0, 1, (N, dim)).astype(np.float32)))
    Qn = ops.normalize_rows(_t(rng.normal(0, 1, (Q, dim)).astype(np.float32)))
    sh = ShardedDenseIndex(Dn, base)
    got = sh.search_feedback(Qn, k, fb_docs=4, alpha=1.0, beta=0.5, weighting="score")
    first = RankedTopk.from_search(*sh.search(Qn, k))
    fb_ids, fb_len, coef = feedback.coefficients(first, 4, 0.5, "score")
    raw = fc.dense_feedback_ref(Qn.cpu().numpy(), Dn.cpu().numpy(), base, fb_ids.cpu().numpy(), fb_len.cpu().numpy(), coef.cpu().numpy(), 1.0)
    _same(sh.feedback(Qn, first, fb_docs=4, beta=0.5, weighting="score", normalize=False), raw)
    q2 = ops.normalize_rows(_t(raw))
    _same(sh.feedback(Qn, first, fb_docs=4, beta=0.5, weighting="score"), q2)
    s2, i2 = sh.search(q2, k)
    _same(got.ids, i2); _same(got.scores, s2)


@pytest.mark.parametrize("seed", range(5))
def test_planted_cluster_recall_gain_through_the_kernels(seed):
    from fusion_amd import ops
    from fusion_amd.distributed import ShardedSparseIndex
    from fusion_amd.planes import RankedTopk
    D, Qm, dc, qc = fc.planted(seed)
    sh = ShardedSparseIndex(ops.sparse_index(_t(D), D.shape[1]), 0)
    sh.build_forward()
    q = ops.sparse_rows(_t(Qm), D.shape[1])
    first = RankedTopk.from_search(*sh.search(*q, 32))
    second = sh.search_feedback(*q, 32, fb_docs=5, fb_terms=8, alpha=1.0, beta=1.0, weighting="uniform")
    assert int(first.lens.min()) == 32 and int(second.lens.min()) == 32
    before = fc.cluster_recall(first.ids.cpu().numpy(), dc, qc, 32)
    after = fc.cluster_recall(second.ids.cpu().numpy(), dc, qc, 32)
    print(f"seed {seed}: recall@32 {before:.4f} -> {after:.4f}")
    assert after >= before + 0.1
