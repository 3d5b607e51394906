"""GPU tests (-m gpu) of the passage -> document layer: fz_lists_collapse at every chunk edge and repeat position, fz_group_expand /
fz_group_max_* at the block-scan edges, and both end to end through ShardedDenseIndex, Aggregator.complete_topk and fuse_topk.
Every comparison is bit for bit against the NumPy restatement of tests/passage_cases.py: the outputs are copies of input bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import passage_cases as pc
from topk_fuse_util import assert_fused_equal, lists_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG_P, BIG_D = (1 << 33) + 5, (1 << 40) + 7          # id bases beyond 2^31


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, exp, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=what)


def _collapse_equals_ref(ids, sc, lens, group, id_base=0, doc_id_base=0, sc64=None, what=""):
    from fusion_amd import ops
    got = ops.lists_collapse(_t(ids), _t(sc), _t(lens), _t(group), id_base=id_base, doc_id_base=doc_id_base,
                             scores64=None if sc64 is None else _t(sc64))
    exp = pc.collapse_ref(ids, sc, lens, group, id_base, doc_id_base, sc64)
    for g, e, name in zip(got, exp, ("ids", "scores", "scores64", "best", "len")):
        assert (g is None) == (e is None), name
        if e is not None:
            _same(g, e, f"{what} {name}")
    return got


def _raw_collapse(ids, sc, lens, group, id_base=0, doc_id_base=0, sc64=None, fill=0x55):
    """fz_lists_collapse on output planes that sit between two guard rows and were filled with a byte pattern beforehand.
    -> (the whole output buffers, guard rows included, as uint8 arrays; the flag word)."""
    from fusion_amd import _lib
    L = _lib.lib()
    Q, n = ids.shape
    ld_out = (n + 63) // 64 * 64
    d = [_t(ids), _t(sc), _t(lens), _t(group)] + ([_t(sc64)] if sc64 is not None else [])
    bufs = [torch.full((Q + 2, ld_out * w), fill, dtype=torch.uint8, device=DEV) for w in (8, 4, 8, 8)]      # ids, scores, scores64, best
    out_len = torch.full((Q + 2,), 0x55555555, dtype=torch.int32, device=DEV)
    ws = torch.full((16,), fill, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.fz_lists_collapse(p(d[0]), p(d[1]), p(d[4]) if sc64 is not None else None, p(d[2]), n, n, Q, p(d[3]), len(group), id_base,
                             doc_id_base, p(bufs[0][1:]), p(bufs[1][1:]), p(bufs[2][1:]) if sc64 is not None else None, p(bufs[3][1:]),
                             p(out_len[1:]), ld_out, p(ws), 16, None)
    assert rc == 0
    torch.cuda.synchronize()
    out = [b.cpu().numpy() for b in bufs] + [out_len.cpu().numpy()]
    for b in out[:4]:
        assert (b[0] == fill).all() and (b[-1] == fill).all(), "a guard row was written"
    assert out[4][0] == 0x55555555 and out[4][-1] == 0x55555555
    if sc64 is None:
        assert (out[2] == fill).all()
    return out, int(ws[:4].view(torch.int32).item())


# ---- collapse ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with64", [False, True], ids=["f32", "f32+f64"])
@pytest.mark.parametrize("n", pc.COLLAPSE_N)
def test_collapse_at_every_chunk_edge(n, with64):
    """Random passage lists over documents of 1-8 passages, tie runs of 3, -inf tails, rows of length 0, 1 and n mixed in one call,
    id bases beyond 2^31."""
    rng = np.random.default_rng(100 + n)
    poff = pc.random_poff(rng, max(n // 3, 2))
    P, Q = int(poff[-1]), 5
    n_eff = min(n, P)
    lens = np.minimum(pc.mixed_lens(rng, Q, n), n_eff).astype(np.int32)
    if n <= P:
        lens[2] = n
    ids, sc = pc.ranked_rows(rng, Q, n, P, lens, run=3, neg_tail=5, id_base=BIG_P)
    sc64 = None
    if with64:          # float64 scores whose float32 roundings are the scores: distinct bits to carry
        sc64 = sc.astype(np.float64)
        sc64[np.isfinite(sc64)] += 2.0 ** -40
    out = _collapse_equals_ref(ids, sc, lens, pc.group_table(poff), BIG_P, BIG_D, sc64, what=f"n={n}")
    assert int(out[4].max()) > 0 and (n == 1 or int(out[4].max()) < lens.max())        # documents do repeat


def test_collapse_full_width_rows():
    """n = 8192 with every slot used, and enough passages for it."""
    rng = np.random.default_rng(7)
    n = pc.CAPACITY
    poff = pc.random_poff(rng, 2500, 2, 8)
    assert poff[-1] >= n
    lens = np.array([n, n, 17], np.int32)
    ids, sc = pc.ranked_rows(rng, 3, n, int(poff[-1]), lens, run=2)
    _collapse_equals_ref(ids, sc, lens, pc.group_table(poff))


def test_collapse_beyond_capacity_raises():
    from fusion_amd import ops
    n = pc.CAPACITY + 1
    ids = torch.zeros((1, n), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="at most 8192"):
        ops.lists_collapse(ids, torch.zeros((1, n), device=DEV), torch.ones(1, dtype=torch.int32, device=DEV),
                           torch.zeros(4, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("n", [1025, 2049])
def test_collapse_one_document_and_own_documents(n):
    rng = np.random.default_rng(n)
    lens = np.array([n, n - 1, 1, 0], np.int32)
    ids, sc = pc.ranked_rows(rng, 4, n, n, lens, run=4)
    out = _collapse_equals_ref(ids, sc, lens, np.zeros(n, np.int32), what="one document")
    assert out[4].tolist() == [1, 1, 1, 0]
    out = _collapse_equals_ref(ids, sc, lens, np.arange(n, dtype=np.int32), doc_id_base=BIG_D, what="own documents")
    assert out[4].tolist() == lens.tolist()


def test_collapse_repeats_in_wave_chunk_later_chunk_and_across_the_boundary():
    ids, sc, lens, poff, docs = pc.repeats_case()
    out = _collapse_equals_ref(ids, sc, lens, pc.group_table(poff))
    assert int(out[4][0]) == docs
    got = out[0][0].cpu().numpy()
    # slot 3 opens document 0's column, slot 5 opens none (slots 4 and 6 hold documents 7 and 8); two repeats lie before slot 1023,
    # which opens document 3's column, and slot 1024 opens none
    assert got[3:6].tolist() == [0, 7, 8] and got[pc.CHUNK - 3] == 3 and got[pc.CHUNK - 2] == ids[0, pc.CHUNK + 1] // 2


def test_collapse_tie_runs_across_documents_and_the_chunk_boundary():
    """Runs of 7 equal scores: 1022 .. 1028 is one run, over the chunk boundary; inside a run the passages -- and with them the
    documents -- ascend, and documents repeat inside runs."""
    rng = np.random.default_rng(3)
    n = 2049
    poff = pc.random_poff(rng, 500, 3, 8)
    lens = np.array([n, 1030], np.int32)
    ids, sc = pc.ranked_rows(rng, 2, n, int(poff[-1]), lens, run=7)
    assert sc[0, 1022] == sc[0, 1028] and sc[0, 1021] != sc[0, 1022]
    _collapse_equals_ref(ids, sc, lens, pc.group_table(poff))


def test_collapse_document_ids_that_collide_modulo_the_table_size():
    rng = np.random.default_rng(4)
    n = 1025                                        # table of 4,096 slots
    poff = pc.random_poff(rng, 400, 1, 4)
    group = pc.group_table(poff).astype(np.int64) * 8192
    lens = np.array([n, 700], np.int32)
    ids, sc = pc.ranked_rows(rng, 2, n, int(poff[-1]), lens)
    _collapse_equals_ref(ids, sc, lens, group.astype(np.int32), doc_id_base=BIG_D)


def test_collapse_cut_to_k():
    from fusion_amd.passages import PassageGroups
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Ranker
    rng = np.random.default_rng(9)
    poff = pc.random_poff(rng, 40, 1, 5)
    P, n = int(poff[-1]), 60
    lens = np.array([n, 30, 0], np.int32)
    ids, sc = pc.ranked_rows(rng, 3, n, P, lens, id_base=BIG_P)
    sc64 = sc.astype(np.float64) * (1 + 2.0 ** -30)
    groups = PassageGroups(poff, id_base=BIG_P, doc_id_base=BIG_D, device=DEV)
    e_ids, e_sc, e_sc64, e_best, e_len = pc.collapse_ref(ids, sc, lens, pc.group_table(poff), BIG_P, BIG_D, sc64)
    docs = int(e_len.max())
    assert 1 < docs < n
    for k in (1, docs, docs + 5, None):
        topk = RankedTopk(ids=_t(ids), scores=_t(sc), lens=_t(lens), scores64=_t(sc64))
        got, best = Ranker.collapse_passages(topk, groups, return_topk=k)
        kk = n if k is None else min(k, n)
        assert got.k == kk and tuple(best.shape) == (3, kk)
        _same(got.ids, e_ids[:, :kk]); _same(got.scores, e_sc[:, :kk]); _same(got.scores64, e_sc64[:, :kk]); _same(best, e_best[:, :kk])
        _same(got.lens, np.minimum(e_len, kk))
    got, _ = groups.collapse(RankedTopk(ids=_t(ids), scores=_t(sc), lens=_t(lens)), 3)
    assert got.scores64 is None
    with pytest.raises(ValueError, match="at least 1"):
        groups.collapse(RankedTopk(ids=_t(ids), scores=_t(sc), lens=_t(lens)), 0)


def _flag_inputs():
    rng = np.random.default_rng(21)
    n = 1500
    poff = pc.random_poff(rng, 600, 2, 6)
    lens = np.array([n, n], np.int32)
    ids, sc = pc.ranked_rows(rng, 2, n, int(poff[-1]), lens, id_base=100)
    return ids, sc, lens, pc.group_table(poff)


@pytest.mark.parametrize("what", ["id_below", "id_above", "inversion_r1", "inversion_r1024", "nan", "nan64"])
def test_collapse_flags_raise_and_stay_in_bounds(what):
    from fusion_amd import ops
    ids, sc, lens, group = _flag_inputs()
    sc64, bit, match = None, 2, "descending"
    if what == "id_below":
        ids[1, 1200], bit, match = 99, 1, "outside"
    elif what == "id_above":
        ids[0, 7], bit, match = 100 + len(group), 1, "outside"
    elif what == "inversion_r1":
        sc[1, 1] = np.nextafter(sc[1, 0], np.float32(np.inf))
    elif what == "inversion_r1024":
        sc[0, 1024] = np.nextafter(sc[0, 1023], np.float32(np.inf))
        sc[0, 1025:] = np.minimum(sc[0, 1025:], sc[0, 1023])           # ... and only that one
        assert (sc[0, 1:1024] <= sc[0, :1023]).all() and (sc[0, 1025:] <= sc[0, 1024:-1]).all()
    elif what == "nan":
        sc[0, 300] = np.nan
    else:
        sc64 = sc.astype(np.float64)
        sc64[1, 1499] = np.nan
    _, flag = _raw_collapse(ids, sc, lens, group, 100, 0, sc64)
    assert flag == bit
    with pytest.raises(ValueError, match=match):
        ops.lists_collapse(_t(ids), _t(sc), _t(lens), _t(group), id_base=100, scores64=None if sc64 is None else _t(sc64))
    ids, sc, lens, group = _flag_inputs()                                   # equal scores and -inf entries set nothing
    sc[0, 1:40] = sc[0, 0]
    sc[1, 1000:] = -np.inf
    assert _raw_collapse(ids, sc, lens, group, 100, 0)[1] == 0


def test_collapse_defines_every_output_element_and_repeats_its_bytes():
    rng = np.random.default_rng(33)
    n = 1100                                          # ld_out = 1152: the tail past n is the kernel's too
    poff = pc.random_poff(rng, 300, 1, 8)
    lens = np.array([n, 0, 513, 1], np.int32)
    ids, sc = pc.ranked_rows(rng, 4, n, int(poff[-1]), lens, run=2)
    sc64 = sc.astype(np.float64)
    group = pc.group_table(poff)
    a, fa = _raw_collapse(ids, sc, lens, group, sc64=sc64, fill=0x55)
    b, fb = _raw_collapse(ids, sc, lens, group, sc64=sc64, fill=0xAA)
    assert fa == 0 and fb == 0
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x[1:-1], y[1:-1])
    e_ids, e_sc, e_sc64, e_best, e_len = pc.collapse_ref(ids, sc, lens, group, scores64=sc64)
    ld = 1152
    for buf, exp, dt, pad in ((a[0], e_ids, np.int64, -1), (a[1], e_sc, np.float32, -np.inf), (a[2], e_sc64, np.float64, -np.inf),
                              (a[3], e_best, np.int64, -1)):
        rows = np.ascontiguousarray(buf[1:-1]).view(dt).reshape(4, ld)
        _same(rows[:, :n], exp)
        assert (rows[:, n:] == pad).all()
    np.testing.assert_array_equal(a[4][1:-1], e_len)


# ---- expand / max --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("W", [1, 255, 256, 257])
def test_expand_and_max_at_the_scan_edges(W, dtype):
    from fusion_amd import ops
    rng = np.random.default_rng(W)
    Q = 6
    cand, cand_len, poff = pc.expand_case(rng, Q, W, doc_id_base=BIG_D)
    need = pc.expand_need(cand, cand_len, poff, BIG_D)
    ldp = int(need.max())
    assert ldp > 0 and need.min() == 0
    wide = torch.full((Q, W + 3), -5, dtype=torch.int64, device=DEV)          # a strided candidate plane
    wide[:, :W] = _t(cand)
    for lens in (cand_len, None):
        if lens is None:
            ldp = int(pc.expand_need(cand, None, poff, BIG_D).max())
        e_pc, e_seg, e_len = pc.expand_ref(cand, lens, poff, ldp, BIG_P, BIG_D)
        tl = None if lens is None else _t(lens)
        pcand, seg, plen = ops.group_expand(wide[:, :W], tl, _t(poff), ldp, id_base=BIG_P, doc_id_base=BIG_D)     # exactly enough
        _same(pcand, e_pc); _same(seg, e_seg); _same(plen, e_len)
        with pytest.raises(ValueError, match="do not fit"):
            ops.group_expand(wide[:, :W], tl, _t(poff), ldp - 1, id_base=BIG_P, doc_id_base=BIG_D)                  # one short
        pcand2, seg2, plen2 = ops.group_expand(wide[:, :W], tl, _t(poff), ldp + 9, id_base=BIG_P, doc_id_base=BIG_D)
        _same(pcand2[:, :ldp], e_pc); _same(seg2, e_seg); assert (pcand2[:, ldp:] == -1).all()
        ps = pc.tied_scores(rng, (Q, ldp), dtype)
        e_out, e_best = pc.max_ref(ps, e_pc, e_seg, lens)
        out, best = ops.group_max(_t(ps), pcand, seg, tl)
        assert out.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
        _same(out, e_out); _same(best, e_best)
        live = e_best >= 0
        assert live.any() and (~live).any()
        # a tie inside a segment: the lowest passage id
        s0, s1 = e_seg[:, :-1], e_seg[:, 1:]
        tied = [(q, w) for q in range(Q) for w in range(W) if live[q, w] and (ps[q, s0[q, w]:s1[q, w]] == e_out[q, w]).sum() > 1]
        assert tied or W == 1
        for q, w in tied[:20]:
            assert int(best[q, w]) == int(e_pc[q, s0[q, w] + np.flatnonzero(ps[q, s0[q, w]:s1[q, w]] == e_out[q, w])[0]])


def test_pair_scores_in_slot_blocks_equals_one_block():
    """PassageGroups.pair_scores cut into blocks of candidate slots by a small budget gives the bytes of one block.  The candidate
    documents of a row are distinct, as in a union of lists: ldp = min(W * pmax, P) counts on it."""
    from fusion_amd import ops
    from fusion_amd.passages import PassageGroups
    rng = np.random.default_rng(17)
    Q, W, d = 4, 70, 8
    cand, cand_len, poff = pc.expand_case(rng, Q, W, D=100, distinct=True)
    groups = PassageGroups(poff, id_base=300, device=DEV)
    Dn = ops.normalize_rows(torch.from_numpy(rng.standard_normal((groups.P, d)).astype(np.float32)).to(DEV))
    Qn = ops.normalize_rows(torch.from_numpy(rng.standard_normal((Q, d)).astype(np.float32)).to(DEV))
    calls = []

    def scorer(ids, lens):
        calls.append(tuple(ids.shape))
        return ops.dot_pairs(Qn, Dn, ids, lens, id_base=300)

    one = groups.pair_scores(scorer, _t(cand), _t(cand_len))
    assert calls == [(Q, min(W * groups.pmax, groups.P))]
    assert groups.P > 8 * groups.pmax
    groups.BUDGET = 8 * Q * groups.pmax * 8                                    # 8 slots per block
    many = groups.pair_scores(scorer, _t(cand), _t(cand_len))
    assert len(calls) == 1 + (W + 7) // 8
    _same(many[0], one[0]); _same(many[1], one[1])
    plane = ops.dot_scores(Qn, Dn).cpu().numpy()
    e_pc, e_seg, _ = pc.expand_ref(cand, cand_len, poff, W * groups.pmax, 300)
    ps = np.full(e_pc.shape, -np.inf, np.float32)
    for q in range(Q):
        ps[q, :e_seg[q, -1]] = plane[q, e_pc[q, :e_seg[q, -1]] - 300]
    e_out, e_best = pc.max_ref(ps, e_pc, e_seg, cand_len)
    _same(one[0], e_out); _same(one[1], e_best)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """About 120 documents of 1-5 passages of 6 words, d = 8: a dense index over the passages, BM25 over the whole documents."""
    from fusion_amd import ops
    from fusion_amd.distributed import ShardedDenseIndex
    from fusion_amd.passages import PassageGroups, split_passages
    rng = np.random.default_rng(2024)
    vocab = [f"w{i}" for i in range(60)]
    docs = [" ".join(rng.choice(vocab, int(rng.integers(1, 31)))) for _ in range(120)]
    passages, poff = split_passages(docs, 6)
    counts = np.diff(poff)
    assert counts.min() == 1 and counts.max() == 5
    PB, DB = 5000, 70
    groups = PassageGroups(poff, id_base=PB, doc_id_base=DB, device=DEV)
    P, Q, d = len(passages), 5, 8
    Dn = ops.normalize_rows(torch.from_numpy(rng.standard_normal((P, d)).astype(np.float32)).to(DEV))
    Qn = ops.normalize_rows(torch.from_numpy(rng.standard_normal((Q, d)).astype(np.float32)).to(DEV))
    plane = ops.dot_scores(Qn, Dn).cpu().numpy()
    group = pc.group_table(poff)
    maxp = np.full((Q, len(docs)), -np.inf, np.float32)                        # the per-document maximum of the plane
    np.maximum.at(maxp, (np.arange(Q)[:, None], group[None, :]), plane)
    queries = [" ".join(rng.choice(vocab, 4)) for _ in range(Q)]
    return dict(docs=docs, groups=groups, index=ShardedDenseIndex(Dn, PB), Qn=Qn, plane=plane, maxp=maxp, P=P, Q=Q, PB=PB, DB=DB,
                group=group, queries=queries)


def _ranked(scores_row, ids_row):
    """(score desc, id asc)."""
    order = np.lexsort((ids_row, -scores_row.astype(np.float64)))
    return ids_row[order], scores_row[order]


def test_search_then_collapse_equals_the_per_document_maximum(corpus):
    from fusion_amd.planes import RankedTopk
    c = corpus
    s, i = c["index"].search(c["Qn"], k=c["P"])
    docs, best = c["groups"].collapse(RankedTopk.from_search(s, i))
    D = len(c["docs"])
    assert docs.lens.tolist() == [D] * c["Q"]
    for q in range(c["Q"]):
        e_ids, e_sc = _ranked(c["maxp"][q], np.arange(D, dtype=np.int64) + c["DB"])
        _same(docs.ids[q, :D], e_ids, f"q={q}"); _same(docs.scores[q, :D], e_sc, f"q={q}")
        b = best[q, :D].cpu().numpy() - c["PB"]
        assert (c["group"][b] + c["DB"] == e_ids).all() and (c["plane"][q, b] == e_sc).all()
    assert (docs.ids[:, D:] == -1).all() and (best[:, D:] == -1).all()


def test_complete_then_fuse_with_bm25_over_whole_documents(corpus, oracle):
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.bm25 import BM25
    from fusion_amd.retrievers.hybrid import Aggregator
    c = corpus
    k = 20
    s, i = c["index"].search(c["Qn"], k=60)
    dpr, _ = c["groups"].collapse(RankedTopk.from_search(s, i), k)
    bm25 = BM25(c["docs"], 1.5, 0.75, id_base=c["DB"]).search_topk(c["queries"], k)
    systems = {"dpr": dpr, "bm25": bm25}
    scorer = c["groups"].doc_scorer(lambda ids, lens: c["index"].pair_scores(c["Qn"], ids, lens))
    done = Aggregator.complete_topk(systems, {"dpr": scorer})
    fused = Aggregator.fuse_topk(done, "rrf")
    # the document-level lists the fusion must have seen: dpr = the union of both lists ranked by the exact MaxP scores
    d_ids, b_ids, b_len = dpr.ids.cpu().numpy(), bm25.ids.cpu().numpy(), bm25.lens.cpu().numpy()
    dpr_lists, grew = [], False
    for q in range(c["Q"]):
        union = list(dict.fromkeys(d_ids[q, :int(dpr.lens[q])].tolist() + b_ids[q, :int(b_len[q])].tolist()))
        grew |= len(union) > k
        u = np.array(union, np.int64)
        r_ids, r_sc = _ranked(c["maxp"][q, u - c["DB"]], u)
        _same(done["dpr"].ids[q, :len(u)], r_ids, f"q={q}"); _same(done["dpr"].scores[q, :len(u)], r_sc, f"q={q}")
        dpr_lists.append([{"corpus_id": int(a), "score": float(b)} for a, b in zip(r_ids, r_sc)])
    assert grew and done["bm25"] is bm25
    exp = oracle.fuse_lists({"dpr": dpr_lists, "bm25": bm25.to_lists()}, "rrf")
    assert_fused_equal(lists_of(fused.to_lists()), lists_of(exp), ("rrf", "none"), "passages")
