"""CPU-side tests of the lexical feedback (csrc/bm25_weighted.hip, csrc/feedback_lexical.hip, ops.lexical_feedback*, TFIDF.feedback,
ShardedLexicalIndex.feedback): the float64 restatement against hand-worked cases, the wrappers' argument checks, the common term space of
the shards, the pack step over a gloo world of 2, and the compiler's resource reports of the two new objects."""
import os
import socket
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lexical_feedback_cases as lc
from conftest import ROOT

NEW = ("fz_bm25_scores_range_w_pv_f64", "fz_tfidf_scores_range_w_f64", "fz_bm25_filter_w_pv_f64", "fz_tfidf_filter_w_f64",
       "fz_bm25_feedback_pv_f64", "fz_tfidf_feedback_f64", "fz_lexical_feedback_rows_f64", "fz_lexical_feedback_max_entries",
       "fz_lexical_weighted_terms")


# ---- the restatement, by hand ------------------------------------------------------------------------------------------------------------
def _rows(docs):
    """docs: a list of {term: value} -> (foff, fterm, fval)."""
    foff = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=foff[1:])
    return foff, np.array([t for d in docs for t in d], dtype=np.int32), np.array([v for d in docs for v in d.values()], dtype=np.float64)


def test_restatement_on_a_hand_computed_example():
    docs = [{1: 2.0, 4: 1.0, 7: 0.5}, {4: 3.0, 9: 1.0}, {7: 4.0}]
    fb_ids = np.array([[100, 101, 100, 999, 102]], dtype=np.int64)       # document 0 twice, one id outside, slot 4 past fb_len
    coef = np.full((1, 5), 0.25, dtype=np.float32)
    out, flags = lc.feedback_ref(*_rows(docs), 3, 100, [[1, -1, 1]], fb_ids, np.array([4]), coef, 1.0, 0.5, 2)
    # w[4] = 0.25 + 0.75 + 0.25 = 1.25, w[7] = 0.125 + 0.125 = 0.25, w[9] = 0.25 (tie: the lower term), w[1]: the query's own
    assert flags == 0 and out == [([1, -1, 1, 4, 7], [1.0, 1.0, 1.0, 0.5, 0.5 * (0.25 / 1.25)])]
    out, _ = lc.feedback_ref(*_rows(docs), 3, 100, [[1, -1, 1]], fb_ids, np.array([4]), coef, 0.75, 2.0, 9)
    assert out == [([1, -1, 1, 4, 7, 9], [0.75, 0.75, 0.75, 2.0, 2.0 * 0.2, 2.0 * 0.2])]
    # no slot, fb_terms = 0, an empty query
    assert lc.feedback_ref(*_rows(docs), 3, 100, [[5, 5], []], np.zeros((2, 0), np.int64), None, np.zeros((2, 0), np.float32), 1.0, 0.5, 3) == \
        ([([5, 5], [1.0, 1.0]), ([], [])], 0)
    assert lc.feedback_ref(*_rows(docs), 3, 100, [[8]], fb_ids, None, coef, 1.0, 0.5, 0)[0] == [([8], [1.0])]


def test_restatement_never_selects_non_positive_sums():
    docs = [{1: -1.0, 2: 1.0, 3: 0.0}, {2: -1.0, 1: 0.5, 5: 2.0}]
    out, _ = lc.feedback_ref(*_rows(docs), 2, 0, [[]], np.array([[0, 1]], dtype=np.int64), None, np.ones((1, 2), np.float32), 1.0, 1.0, 5)
    assert out == [([5], [1.0])]                                          # w[1] = -0.5, w[2] = 0.0 (cancelled), w[3] = 0.0


def test_restatement_capacity_rule_cuts_at_the_slot_boundary():
    rng = np.random.default_rng(1)
    foff, fterm, fval = lc.random_rows(rng, [6, 3, 2, 4], 50)
    ids = np.array([[0, 1, 2, 3]], dtype=np.int64)
    coef = np.ones((1, 4), np.float32)
    full, f0 = lc.feedback_ref(foff, fterm, fval, 4, 0, [[]], ids, None, coef, 1.0, 1.0, 50, cap=15)
    cut, f1 = lc.feedback_ref(foff, fterm, fval, 4, 0, [[]], ids, None, coef, 1.0, 1.0, 50, cap=10)      # 6 + 3 = 9, + 2 would pass 10
    two, _ = lc.feedback_ref(foff, fterm, fval, 4, 0, [[]], ids[:, :2], None, coef[:, :2], 1.0, 1.0, 50, cap=15)
    assert f0 == 0 and f1 == lc.CUT and cut == two and cut != full       # slot 2 and EVERY later slot (3 would have fitted) are skipped


def test_weighted_plane_restatement_by_hand():
    ix = dict(N=3, V=2, toff=np.array([0, 2, 3]), pdoc=np.array([0, 2, 2], dtype=np.int32), val=np.array([1.5, 2.0, 4.0]))
    plane = lc.plane_ref(ix, [([0, -1, 1, 0], [2.0, 9.0, -0.5, 0.25])])
    assert plane.tolist() == [[1.5 * 2.0 + 0.25 * 1.5, 0.0, (2.0 * 2.0 + -0.5 * 4.0) + 0.25 * 2.0]]
    ids, sc = lc.topk_ref(np.array([[1.0, 2.0, 2.0, -0.0, 0.0]]), 5, id_base=10)
    assert ids.tolist() == [[11, 12, 10, 13, 14]] and sc.tolist() == [[2.0, 2.0, 1.0, 0.0, 0.0]]


@pytest.mark.parametrize("seed", lc.PLANTED_SEEDS)
def test_planted_cluster_recall_gain_is_the_restatements(seed):
    """The restatement alone: recall@k of the cluster after feedback >= before for every seed and query, and > before in total."""
    from fusion_amd.retrievers.bm25 import TFIDF
    docs, queries, cluster = lc.planted_cluster(seed)
    model = TFIDF(docs, device="cpu")
    qt = [[model.vocab.get(w, -1) for w in q.split()] for q in queries]
    first, second, _, exp = lc.search_feedback_ref(lc.host_index(model), qt, lc.PLANTED_K, 10, 10, 1.0, 0.5)
    before, after = lc.cluster_recall(first, cluster), lc.cluster_recall(second, cluster)
    assert all(a >= b for a, b in zip(after, before)), (before, after)
    assert sum(after) > sum(before), (before, after)
    words = list(model.vocab)
    assert all(words[t].startswith("c") for t in exp[1][0][1:4])          # the strongest expansion terms are the cluster's own words


# ---- declarations, resources -------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_abi_is_additive():
    from fusion_amd import _lib, ops
    L = _lib.lib()
    assert L.fz_abi_version() == 20
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and f"{name}(" in header, name
    assert 4096 <= L.fz_lexical_feedback_max_entries() == lc.E == ops.lexical_feedback_max_entries() <= 8192
    assert (ops.lexical_weighted_terms("pv"), ops.lexical_weighted_terms("tfidf")) == (256, 128)
    mk = open(os.path.join(ROOT, "fusion_amd", "csrc", "Makefile")).read()
    assert "bm25_weighted.hip" in mk and "feedback_lexical.hip" in mk


def _resources(obj):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load().get(obj)
    if not res:
        pytest.skip(f"no {obj}.res next to the objects: build with `make -C fusion_amd/csrc` where ROCm is installed")
    return kernel_resources, res


def test_the_weighted_walks_hold_no_spilled_register_and_stay_within_static_lds():
    kr, res = _resources("bm25_weighted")
    assert len(res) == 4 and {kr.short(k).split("<")[0] for k in res} == {"lexical_weighted_kernel"}
    lds = sorted(r["lds"] for r in res.values())
    assert lds == [36 * 1024] * 2 + [60 * 1024] * 2                      # 28 / 56 KiB of accumulators + four 256- / 128-entry 8-byte tables
    for k, r in res.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (k, r)
        assert r["vgprs"] <= 64, (k, r)                                   # eight waves per SIMD, as the unweighted walks


def test_the_feedback_kernels_hold_no_spilled_register():
    kr, res = _resources("feedback_lexical")
    assert len(res) == 3 and {kr.short(k).split("<")[0] for k in res} == {"lexical_feedback_kernel"}
    for k, r in res.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (k, r)
        assert r["vgprs"] <= 128 and r["lds"] == 0, (k, r)                # 1,024 threads; the LDS is dynamic:
    E = lc.E
    assert 2 * E * 8 + 2 * E * 4 + lc.FB_SLOTS * 20 + 2 * E // 8 + 64 <= 160 * 1024      # ... sums, cells, slot tables, marks, wave totals


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_weighted_entries_reject_bad_arguments_without_gpu():
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, OK = _lib.FZ_ERR_ARG, _lib.FZ_OK
    fake = 4096

    def plane(fn, tfidf, qw=fake, Q=2, N=100, lo=0, hi=100, scores=fake, lds=128, toff=fake):
        vals = (fake, fake) if tfidf else (fake,)
        return getattr(L, fn)(toff, fake, *vals, None, fake, fake, qw, Q, N, lo, hi, scores, lds, None)

    def filt(fn, tfidf, qw=fake, Q=2, N=100, lo=0, hi=100, cap=8, tau=fake):
        vals = (fake, fake) if tfidf else (fake,)
        return getattr(L, fn)(fake, fake, *vals, None, fake, fake, qw, Q, N, lo, hi, 0, tau, fake, fake, fake, cap, fake, None)

    for fn, tfidf in (("fz_bm25_scores_range_w_pv_f64", 0), ("fz_tfidf_scores_range_w_f64", 1)):
        assert plane(fn, tfidf, qw=None) == ARG and plane(fn, tfidf, scores=None) == ARG and plane(fn, tfidf, toff=None) == ARG
        assert plane(fn, tfidf, Q=-1) == ARG and plane(fn, tfidf, lds=99) == ARG and plane(fn, tfidf, lo=1) == ARG and plane(fn, tfidf, hi=101) == ARG
        assert plane(fn, tfidf, Q=0, qw=None) == OK and plane(fn, tfidf, hi=0, qw=None) == OK
    for fn, tfidf in (("fz_bm25_filter_w_pv_f64", 0), ("fz_tfidf_filter_w_f64", 1)):
        assert filt(fn, tfidf, qw=None) == ARG and filt(fn, tfidf, tau=None) == ARG and filt(fn, tfidf, cap=0) == ARG
        assert filt(fn, tfidf, Q=0, qw=None) == OK


def test_feedback_entries_reject_bad_arguments_without_gpu():
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, OK = _lib.FZ_ERR_ARG, _lib.FZ_OK
    fake = 4096

    def call(src="rows", foff=fake, N=50, qoff=fake, Q=4, fb_ids=fake, ldf=64, coef=fake, ldc=64, F=10, m=10, out_t=fake, out_w=fake,
             ldo=128, width=100, out_len=fake, flag=fake):
        rows = {"rows": (fake, fake), "pv": (fake, fake, fake), "tfidf": (fake, fake, fake, fake)}[src]
        fn = {"rows": "fz_lexical_feedback_rows_f64", "pv": "fz_bm25_feedback_pv_f64", "tfidf": "fz_tfidf_feedback_f64"}[src]
        return getattr(L, fn)(foff, *rows, N, 0, qoff, fake, Q, fb_ids, ldf, None, coef, ldc, F, 1.0, 0.5, m, out_t, out_w, ldo, width,
                              out_len, flag, None)

    for src in ("rows", "pv", "tfidf"):
        for null in ("foff", "qoff", "fb_ids", "coef", "out_t", "out_w", "out_len", "flag"):
            assert call(src, **{null: None}) == ARG, (src, null)
        assert call(src, Q=-1) == ARG and call(src, N=-1) == ARG and call(src, F=-1) == ARG and call(src, m=-1) == ARG
        assert call(src, width=-1) == ARG and call(src, ldf=9) == ARG and call(src, ldc=9) == ARG and call(src, ldo=99) == ARG
        assert call(src, Q=0) == OK and call(src, Q=0, foff=None, qoff=None, fb_ids=None, coef=None, out_t=None, out_w=None, out_len=None,
                                             flag=None) == OK


def test_python_wrappers_validate_before_the_device():
    from fusion_amd import ops
    from fusion_amd.retrievers.bm25 import BM25, TFIDF, WeightedQueries
    z64, z32, zd = torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(TypeError, match="ForwardIndex"):
        ops.lexical_feedback("pv", None, zd, None, z64, z32, z64, None, zd, 1.0, 0.5, 4)
    with pytest.raises(ValueError, match="mode"):
        ops.lexical_feedback("expr", None, zd, None, z64, z32, z64, None, zd, 1.0, 0.5, 4)
    with pytest.raises(TypeError, match="on the GPU"):
        ops.lexical_feedback_rows(z64, z32, zd, z64, z32, z64, None, zd, 1.0, 0.5, 4)
    with pytest.raises(TypeError, match="on the GPU"):
        ops._lexical_weights("t", z32, zd)
    with pytest.raises(TypeError, match="float64"):
        WeightedQueries(z64, z32, zd.float())
    with pytest.raises(ValueError, match="one entry"):
        WeightedQueries(z64, z32, zd[:2])
    assert WeightedQueries(z64, z32, zd).Q == 2
    model = BM25(["a b", "b c"], 1.5, 0.75, device="cpu")
    model.USE_POSTING_VALUES = False
    wq = WeightedQueries(z64, z32, zd)
    for call in (lambda: model.feedback(["a"], None), lambda: model.scores_weighted(wq), lambda: model.search_topk_weighted(wq, 1)):
        with pytest.raises(ValueError, match="USE_POSTING_VALUES"):
            call()
    tf = TFIDF(["a b", "b c"], device="cpu")
    assert tf.expansion_words(WeightedQueries(torch.tensor([0, 2, 3]), torch.tensor([1, -1, 2], dtype=torch.int32),
                                              torch.tensor([1.0, 1.0, 0.25], dtype=torch.float64))) == [[("b", 1.0), (None, 1.0)], [("c", 0.25)]]


# ---- the shards' common term space -------------------------------------------------------------------------------------------------------
def _shards(docs, bounds, cls="TFIDF"):
    from fusion_amd.retrievers import bm25
    make = (lambda d, **kw: bm25.TFIDF(d, device="cpu", **kw)) if cls == "TFIDF" else (lambda d, **kw: bm25.BM25(d, 1.5, 0.75, device="cpu", **kw))
    parts = [make(docs[lo:hi]) for lo, hi in bounds]
    stats = bm25.LexicalStats.merge([p.stats() for p in parts])
    return lc.host_forward(make(docs)), [lc.host_forward(make(docs[lo:hi], stats=stats, id_base=lo)) for lo, hi in bounds]


def test_global_term_table_is_the_whole_corpus_numbering_for_contiguous_shards():
    from fusion_amd import feedback as fb
    docs = ["a b c", "b d", "e a", "f g b", "c h", "i"]
    whole, shards = _shards(docs, [(0, 2), (2, 5), (5, 6)])
    words, ident = fb.global_term_table(whole)
    assert words == list(whole.vocab) and ident.tolist() == list(range(len(words)))
    for s in shards:
        w, l2g = fb.global_term_table(s)
        assert w == words                                                 # the same table on every shard: the whole corpus's term ids
        assert [w[g] for g in l2g.tolist()] == list(s.vocab)
        g2l = fb.global_to_local(l2g, len(w))
        assert [g2l[whole.vocab[x]] for x in s.vocab] == list(range(len(s.vocab)))
        assert sorted(np.flatnonzero(g2l < 0).tolist()) == sorted(whole.vocab[x] for x in whole.vocab if x not in s.vocab)


# ---- the pack step: pure per shard, MAX combines, gloo world 2 ---------------------------------------------------------------------------
def _pack_case():
    rng = np.random.default_rng(5)
    docs = lc.synthetic_text(rng, 37, 0, 12, vocab_size=40)
    docs[0], docs[18], docs[19] = "", "w1 w2 w2 w3", "w3"
    fb_ids = rng.integers(0, 37, (4, 5)).astype(np.int64)
    fb_ids[0, :3] = [18, 19, 0]
    fb_ids[1, 1], fb_ids[2, 0], fb_ids[3, 2] = -1, 37, fb_ids[3, 1]
    return docs, fb_ids


def _pack(model, fb_ids, width):
    from fusion_amd import feedback as fb
    l2g = torch.from_numpy(fb.global_term_table(model)[1])
    return fb.pack_lexical_rows(model, l2g, torch.from_numpy(fb_ids), width)


def test_pack_lexical_rows_combines_by_max_to_the_whole_index_rows():
    """(TF-IDF: BM25's posting values are tabulated on the device -- tests/test_gpu_lexical_feedback.py packs those.)"""
    from fusion_amd import feedback as fb
    docs, fb_ids = _pack_case()
    whole, shards = _shards(docs, [(0, 19), (19, 30), (30, 37)])
    L = max(int(fb.lexical_row_lengths(s, torch.from_numpy(fb_ids)).max()) for s in [whole] + shards)
    wt, wv = _pack(whole, fb_ids, L)
    parts = [_pack(s, fb_ids, L) for s in shards]
    t, v = parts[0]
    for pt, pv in parts[1:]:
        t, v = torch.maximum(t, pt), torch.maximum(v, pv)
    assert torch.equal(t, wt) and torch.equal(v.view(torch.int64), wv.view(torch.int64))
    # ... and the whole index's pack is its rows, slot by slot, in global term ids
    ix = lc.host_index(whole)
    foff, fterm, fval = lc.forward_rows(ix)
    for q in range(fb_ids.shape[0]):
        for r in range(fb_ids.shape[1]):
            d = int(fb_ids[q, r])
            n = int(foff[d + 1] - foff[d]) if 0 <= d < 37 else 0
            assert wt[q, r, :n].tolist() == fterm[foff[d]:foff[d] + n].tolist() if n else True
            assert wv[q, r, :n].tolist() == fval[foff[d]:foff[d] + n].tolist() if n else True
            assert (wt[q, r, n:] == -1).all() and torch.isneginf(wv[q, r, n:]).all()
    rows = fb.lexical_rows(wt, wv)
    assert rows[0][-1] == rows[1].numel() == rows[2].numel() and rows[3][1, 1] == -1 and rows[3][2, 0] == -1 and rows[3][0, 2] == -1
    with pytest.raises(ValueError, match="width"):
        _pack(whole, fb_ids, L - 1)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _pack_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), OMP_NUM_THREADS="1")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from fusion_amd import feedback as fb
    from fusion_amd.distributed import reduce_max, shard_bounds
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = None
    try:
        docs, fb_ids = _pack_case()
        bounds = [shard_bounds(len(docs), world, r) for r in range(world)]
        model = _shards(docs, bounds)[1][rank]
        ids = torch.from_numpy(fb_ids)
        L = int(reduce_max(fb.lexical_row_lengths(model, ids).max().reshape(1)).item())
        t, v = _pack(model, fb_ids, L)
        out = [reduce_max(t, None, skip_empty=True).numpy(), reduce_max(v, None, skip_empty=True).numpy()]
    finally:
        q.put((rank, out))
        dist.destroy_process_group()


def test_pack_lexical_rows_gloo_world2_equals_one_rank():
    import torch.multiprocessing as mp
    from fusion_amd import feedback as fb
    docs, fb_ids = _pack_case()
    whole = _shards(docs, [(0, len(docs))])[0]
    L = int(fb.lexical_row_lengths(whole, torch.from_numpy(fb_ids)).max())
    wt, wv = _pack(whole, fb_ids, L)
    ctx = mp.get_context("spawn")
    qu, port = ctx.Queue(), _free_port()
    ps = [ctx.Process(target=_pack_worker, args=(r, 2, port, qu)) for r in range(2)]
    for p in ps: p.start()
    try:
        res = [qu.get(timeout=300) for _ in ps]
    finally:
        for p in ps: p.join(60)
        for p in ps:
            if p.is_alive(): p.kill()
    assert sorted(r[0] for r in res) == [0, 1]
    for rank, out in res:
        assert out is not None, rank
        np.testing.assert_array_equal(out[0], wt.numpy(), err_msg=f"rank {rank}: terms")
        np.testing.assert_array_equal(out[1].view(np.int64), wv.numpy().view(np.int64), err_msg=f"rank {rank}: values")
