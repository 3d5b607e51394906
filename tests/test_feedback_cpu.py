"""CPU-side tests (-m "not gpu") of pseudo-relevance feedback: the NumPy restatement of its fixed arithmetic (tests/feedback_cases.py) on
a hand-computed example and on the planted-cluster corpus, the new entry points in the header and the binding, every argument check of
fz_sparse_feedback_f32 / fz_dense_feedback_f32 (all made before the first HIP call, exercised with fake pointers), feedback.coefficients
against a float64 restatement, feedback.gather_rows over a gloo world of 2, and the compiler's resource report of the two kernels."""
import os
import socket
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import feedback_cases as fc
from conftest import ROOT

NEW = ("fz_sparse_feedback_max_vocab", "fz_sparse_feedback_f32", "fz_dense_feedback_f32")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _hand_case():
    # V = 8; query {1: 0.5, 4: 1.0}; documents d0 {1: .25, 2: .5, 6: 1}, d1 {2: .5, 3: .75, 6: -1}, d2 {5: .125}
    foff, rows = fc.forward_of([([1, 2, 6], [0.25, 0.5, 1.0]), ([2, 3, 6], [0.5, 0.75, -1.0]), ([5], [0.125])])
    qoff, qterms, qw = fc.queries_of([([1, 4], [0.5, 1.0])])
    fb_ids = np.array([[100, 101, 107, 102]], np.int64)          # id_base 100: slot 2 is past the index (N = 3), slot 3 past fb_len
    return dict(foff=foff, rows=rows, N=3, V=8, id_base=100, qoff=qoff, qterms=qterms, qw=qw, fb_ids=fb_ids,
                fb_len=np.array([3], np.int32), coef=np.array([[0.5, 0.5, 1.0, 1.0]], np.float32))


def test_restatement_on_a_hand_computed_example():
    c = _hand_case()
    # alpha = 2: acc[1] = 1.0 + .5 * .25 = 1.125, acc[4] = 2.0; acc[2] = .25 + .25 = .5, acc[3] = .375, acc[6] = .5 - .5 = 0.0
    # candidates by sum: 2 (0.5), 3 (0.375), 6 (0.0, still a candidate); document d2's term 5 was never touched
    t, w, n, over = fc.sparse_feedback_ref(**c, alpha=2.0, m=2)
    assert not over and n.tolist() == [4] and t.tolist() == [[1, 2, 3, 4]] and w.tolist() == [[1.125, 0.5, 0.375, 2.0]]
    t, w, n, _ = fc.sparse_feedback_ref(**c, alpha=2.0, m=1)
    assert n.tolist() == [3] and t.tolist() == [[1, 2, 4]] and w.tolist() == [[1.125, 0.5, 2.0]]
    t, w, n, _ = fc.sparse_feedback_ref(**c, alpha=2.0, m=5)      # all three candidates, the zero sum among them; padded to width 7
    assert n.tolist() == [5] and t.tolist() == [[1, 2, 3, 4, 6, -1, -1]] and w.tolist() == [[1.125, 0.5, 0.375, 2.0, 0.0, 0.0, 0.0]]
    t, w, n, _ = fc.sparse_feedback_ref(**c, alpha=2.0, m=0)
    assert t.tolist() == [[1, 4]] and w.tolist() == [[1.125, 2.0]]
    t, w, n, over = fc.sparse_feedback_ref(**c, alpha=2.0, m=2, width=3)
    assert over and n.tolist() == [4] and t.tolist() == [[1, 2, 3]]
    c["fb_len"] = np.array([4], np.int32)                         # slot 3 counts now: term 5 with 1.0 * .125
    t, w, n, _ = fc.sparse_feedback_ref(**c, alpha=2.0, m=4)
    assert t.tolist() == [[1, 2, 3, 4, 5, 6]] and w.tolist() == [[1.125, 0.5, 0.375, 2.0, 0.125, 0.0]]
    Qn = np.array([[1.0, -2.0]], np.float32)
    Dn = np.array([[0.5, 0.25], [4.0, 8.0], [1.0, 1.0]], np.float32)
    out = fc.dense_feedback_ref(Qn, Dn, 100, c["fb_ids"], np.array([3], np.int32), c["coef"], 2.0)
    assert out.tolist() == [[2.0 + 0.25 + 2.0, -4.0 + 0.125 + 4.0]]


def test_desc_key_orders_like_the_device_key():
    x = np.array([np.inf, 3.0, 1.0, 0.0, -0.0, -1.0, -np.inf], np.float32)
    k = fc.desc_key_f32(x)
    assert k[3] == k[4] and (np.diff(k.astype(np.int64))[[0, 1, 2, 4, 5]] > 0).all()
    assert fc.desc_key_f32(np.array([np.nan], np.float32))[0] == 0


def test_ties_go_to_the_lower_term_and_minus_zero_equals_zero():
    foff, rows = fc.forward_of([([0, 3, 5, 7], [1.0, 1.0, 1.0, 1.0]), ([5, 7], [-1.0, 1.0])])
    qoff, qterms, qw = fc.queries_of([([], [])])
    ids = np.array([[0, 1]], np.int64)
    coef = np.array([[1.0, 1.0]], np.float32)
    # sums: 0 -> 1, 3 -> 1, 5 -> +0.0, 7 -> 2
    t, w, n, _ = fc.sparse_feedback_ref(foff, rows, 2, 8, 0, qoff, qterms, qw, ids, None, coef, 1.0, 2)
    assert t.tolist() == [[0, 7]] and w.tolist() == [[1.0, 2.0]]
    t, w, n, _ = fc.sparse_feedback_ref(foff, rows, 2, 8, 0, qoff, qterms, qw, ids, None, coef, 1.0, 3)
    assert t.tolist() == [[0, 3, 7]]
    coef = np.array([[-1.0, -1.0]], np.float32)                  # sums: 0 -> -1, 3 -> -1, 5 -> -1 + 1 = +0.0, 7 -> -2
    t, w, n, _ = fc.sparse_feedback_ref(foff, rows, 2, 8, 0, qoff, qterms, qw, ids, None, coef, 1.0, 2)
    assert t.tolist() == [[0, 5]] and w.tolist() == [[-1.0, 0.0]]


@pytest.mark.parametrize("seed", range(5))
def test_planted_cluster_recall_gain(seed):
    """8 clusters of 32 documents over their own 12 topic terms; a 2-term query misses the cluster's documents that hold neither term
    (recall@32 about 0.8), the 8 strongest terms of its top 5 documents bring them in (1.0)."""
    before, after = fc.planted_recall_ref(seed)
    print(f"seed {seed}: recall@32 {before:.4f} -> {after:.4f}")
    assert after >= before + 0.1


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_abi_is_additive():
    from fusion_amd import _lib, ops
    L = _lib.lib()
    assert L.fz_abi_version() == 20
    header = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and f"{name}(" in header, name
    assert L.fz_sparse_feedback_max_vocab() == fc.MAX_V == ops.sparse_feedback_max_vocab()
    assert "feedback.hip" in open(os.path.join(ROOT, "fusion_amd", "csrc", "Makefile")).read()


def test_the_feedback_kernels_hold_no_spilled_register():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.load().get("feedback")
    if not res:
        pytest.skip("no feedback.res next to the objects: build with `make -C fusion_amd/csrc` where ROCm is installed")
    names = {kernel_resources.short(k).split("<")[0] for k in res}
    assert names == {"sparse_feedback_kernel", "dense_feedback_kernel"}
    for k, r in res.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, f"{k}: {r['vgpr_spill']} spilled VGPRs, {r['scratch']} B/lane of scratch"


def test_sparse_feedback_rejects_bad_arguments_without_gpu():
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, UNS, OK = _lib.FZ_ERR_ARG, _lib.FZ_ERR_UNSUPPORTED, _lib.FZ_OK
    fake = 4096                      # a non-null "device pointer": no call below may get as far as using it

    def call(foff=fake, rows=fake, V=1000, N=50, qoff=fake, qterms=fake, qw=fake, Q=4, fb_ids=fake, ldf=64, fb_len=None, coef=fake, ldc=64,
             F=10, alpha=1.0, m=32, out_t=fake, out_w=fake, ldo=128, width=100, out_len=fake, flag=fake):
        return L.fz_sparse_feedback_f32(foff, rows, V, N, 0, qoff, qterms, qw, Q, fb_ids, ldf, fb_len, coef, ldc, F, alpha, m, out_t, out_w,
                                        ldo, width, out_len, flag, None)

    for null in ("foff", "qoff", "fb_ids", "coef", "out_t", "out_w", "out_len", "flag"):
        assert call(**{null: None}) == ARG, null
    assert call(V=0) == ARG and call(V=-1) == ARG and call(V=fc.MAX_V + 1) == ARG
    assert call(Q=-1) == ARG and call(N=-1) == ARG and call(F=-1) == ARG and call(m=-1) == ARG and call(width=-1) == ARG
    assert call(ldf=9) == ARG and call(ldc=9) == ARG and call(ldo=99) == ARG
    assert call(rows=fake + 4) == UNS                             # postings are read as 8-byte words
    assert call(Q=0) == OK and call(Q=0, V=fc.MAX_V) == OK
    assert call(Q=0, foff=None, rows=None, qoff=None, qterms=None, qw=None, fb_ids=None, coef=None, out_t=None, out_w=None, out_len=None,
                flag=None) == OK
    assert call(Q=0, V=0) == ARG and call(Q=0, V=fc.MAX_V + 1) == ARG          # the vocabulary is judged before anything else is looked at


def test_dense_feedback_rejects_bad_arguments_without_gpu():
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, OK = _lib.FZ_ERR_ARG, _lib.FZ_OK
    fake = 4096

    def call(Qn=fake, ldq=768, Dn=fake, ldd=768, Q=4, N=50, dim=768, fb_ids=fake, ldf=64, fb_len=None, coef=fake, ldc=64, F=10, alpha=1.0,
             out=fake, ldo=768):
        return L.fz_dense_feedback_f32(Qn, ldq, Dn, ldd, Q, N, dim, 0, fb_ids, ldf, fb_len, coef, ldc, F, alpha, out, ldo, None)

    for null in ("Qn", "Dn", "fb_ids", "coef", "out"):
        assert call(**{null: None}) == ARG, null
    assert call(Q=-1) == ARG and call(N=-1) == ARG and call(F=-1) == ARG and call(dim=0) == ARG and call(dim=-4) == ARG
    assert call(ldq=767) == ARG and call(ldd=767) == ARG and call(ldo=767) == ARG and call(ldf=9) == ARG and call(ldc=9) == ARG
    assert call(Q=0) == OK and call(Q=0, Qn=None, Dn=None, fb_ids=None, coef=None, out=None) == OK


def test_python_wrappers_validate_before_the_device():
    from fusion_amd import ops
    from fusion_amd.distributed import ShardedSparseIndex
    z64, zf = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3))
    with pytest.raises(TypeError, match="SparseForward"):
        ops.sparse_feedback(None, 10, z64, z64, zf, z64, None, zf, 1.0, 4)
    fwd = ops.SparseForward(torch.zeros(1, dtype=torch.int64), torch.zeros((0, 2), dtype=torch.int32), 0, 10)
    with pytest.raises(TypeError, match="on the GPU"):
        ops.sparse_feedback(fwd, 10, torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0), z64, None, zf, 1.0, 4)
    with pytest.raises(TypeError, match="on the GPU"):
        ops.dense_feedback(zf, zf, z64, None, zf, 1.0)
    topk = SimpleNamespace()
    with pytest.raises(ValueError, match="build_forward"):
        ShardedSparseIndex(SimpleNamespace(forward=None, V=10, N=0), 0).feedback(None, None, None, topk)
    with pytest.raises(ValueError, match="sparse_feedback_max_vocab"):
        ShardedSparseIndex(SimpleNamespace(forward=fwd, V=fc.MAX_V + 1, N=0), 0).feedback(None, None, None, topk)


# ---- coefficients --------------------------------------------------------------------------------------------------------------------
def _topk(scores, lens):
    from fusion_amd.planes import RankedTopk
    s = torch.tensor(scores, dtype=torch.float32)
    ids = torch.arange(s.numel(), dtype=torch.int64).view(s.shape) + 1000
    return RankedTopk(ids=ids, scores=s, lens=torch.tensor(lens, dtype=torch.int32))


def _one_ulp(got, exp64):
    exp = exp64.astype(np.float32)
    assert got.dtype == np.float32
    assert (np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= np.spacing(np.abs(exp)).astype(np.float64)).all(), (got, exp)


def test_coefficients_uniform_and_score_weighting():
    from fusion_amd.feedback import coefficients
    sc = [[9.5, 7.25, 3.1, 0.7, 0.1], [4.0, 3.0, 2.0, -1.0, -2.0], [1.0, -1.0, 0.0, 0.0, 0.0], [0.3, 0.2, 0.1, 0.0, 0.0]]
    lens = [5, 3, 2, 0]
    topk = _topk(sc, lens)
    s64 = np.asarray(sc, np.float32).astype(np.float64)
    for fb_docs in (3, 5, 9):                                    # 9: more than the lists hold
        F = min(fb_docs, 5)
        ids, flen, coef = coefficients(topk, fb_docs, 0.75, "uniform")
        assert ids.dtype == torch.int64 and flen.dtype == torch.int32 and coef.dtype == torch.float32
        assert tuple(ids.shape) == (4, F) and torch.equal(ids, topk.ids[:, :F])
        assert flen.tolist() == [min(fb_docs, n) for n in lens]
        exp = np.zeros((4, F))
        for q, n in enumerate(flen.tolist()):
            exp[q, :n] = 0.75 / max(n, 1)
        _one_ulp(coef.numpy(), exp)
        _, flen, coef = coefficients(topk, fb_docs, 0.75, "score")
        exp = np.zeros((4, F))
        for q, n in enumerate(flen.tolist()):
            tot = s64[q, :n].sum()
            exp[q, :n] = 0.75 * s64[q, :n] / tot if (np.isfinite(tot) and tot > 0) else 0.75 / max(n, 1)
        _one_ulp(coef.numpy(), exp)
    # the fallback: row 2's listed scores sum to 0, row 3 lists nothing
    _, flen, coef = coefficients(topk, 5, 1.0, "score")
    assert coef[2].tolist() == [0.5, 0.5, 0.0, 0.0, 0.0] and coef[3].tolist() == [0.0] * 5
    inf = _topk([[float("inf"), 1.0], [float("-inf"), float("-inf")]], [2, 2])
    assert coefficients(inf, 2, 1.0, "score")[2].tolist() == [[0.5, 0.5], [0.5, 0.5]]
    assert tuple(coefficients(topk, 0)[0].shape) == (4, 0)
    with pytest.raises(ValueError, match="weighting"):
        coefficients(topk, 3, 1.0, "rank")
    with pytest.raises(ValueError):
        coefficients(topk, -1)
    with pytest.raises(TypeError):
        coefficients(topk.ids, 3)


# ---- gather_rows over two ranks ------------------------------------------------------------------------------------------------------
def _gather_case():
    rng = np.random.default_rng(77)
    V, N, Q, F = 300, 41, 5, 6
    lens = rng.integers(0, 40, N)
    lens[[0, 20, 21, 40]] = [0, 39, 1, 17]                       # (document 20 is rank 0's last, 21 rank 1's first)
    foff, rows = fc.forward_of(fc.random_docs(rng, V, lens, signed=True))
    Dn = rng.normal(0, 1, (N, 7)).astype(np.float32)
    fb_ids = (rng.integers(0, N, (Q, F)) + 500).astype(np.int64)
    fb_ids[0, :4] = [520, 521, 500, 540]
    fb_ids[1, 2] = -1
    fb_ids[2, 0], fb_ids[2, 5] = 499, 541                       # just outside the corpus
    fb_ids[3, 1] = fb_ids[3, 0]
    return V, N, foff, rows, Dn, fb_ids


def _shard_forward(foff, rows, lo, hi, V):
    from fusion_amd import ops
    return ops.SparseForward(torch.from_numpy(foff[lo:hi + 1] - foff[lo]), torch.from_numpy(rows[foff[lo]:foff[hi]].copy()), hi - lo, V)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), OMP_NUM_THREADS="1")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from fusion_amd.distributed import shard_bounds
    from fusion_amd.feedback import gather_rows
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = None
    try:
        V, N, foff, rows, Dn, fb_ids = _gather_case()
        lo, hi = shard_bounds(N, world, rank)
        fwd, slots = gather_rows(_shard_forward(foff, rows, lo, hi, V), torch.from_numpy(fb_ids), 500 + lo)
        drows, dslots = gather_rows(torch.from_numpy(Dn[lo:hi].copy()), torch.from_numpy(fb_ids), 500 + lo)
        out = [t.numpy() for t in (fwd.foff, fwd.rows, slots, drows, dslots)] + [fwd.N, fwd.V]
    finally:
        q.put((rank, out))
        dist.destroy_process_group()


def test_gather_rows_gloo_world2_equals_one_rank():
    import torch.multiprocessing as mp
    from fusion_amd.feedback import gather_rows
    V, N, foff, rows, Dn, fb_ids = _gather_case()
    one = gather_rows(_shard_forward(foff, rows, 0, N, V), torch.from_numpy(fb_ids), 500)
    done = gather_rows(torch.from_numpy(Dn), torch.from_numpy(fb_ids), 500)
    exp = [t.numpy() for t in (one[0].foff, one[0].rows, one[1], done[0], done[1])]
    # the single-rank packing is the rows themselves, slot by slot
    Q, F = fb_ids.shape
    for q in range(Q):
        for r in range(F):
            d = int(fb_ids[q, r]) - 500
            p = q * F + r
            got = exp[1][exp[0][p]:exp[0][p + 1]]
            if 0 <= d < N:
                np.testing.assert_array_equal(got, rows[foff[d]:foff[d + 1]])
                assert exp[2][q, r] == (p if foff[d + 1] > foff[d] else -1) and exp[4][q, r] == p
                np.testing.assert_array_equal(exp[3][p], Dn[d])
            else:
                assert len(got) == 0 and exp[2][q, r] == -1 and exp[4][q, r] == -1
    ctx = mp.get_context("spawn")
    qu = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_gather_worker, args=(r, 2, port, qu)) for r in range(2)]
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
        assert out[5] == Q * F and out[6] == V
        for g, e, name in zip(out[:5], exp, ("foff", "rows", "slots", "dense rows", "dense slots")):
            if name == "dense rows":                                # rows of slots nobody owns are fill on both sides
                g, e = np.where(np.isneginf(g), 0, g), np.where(np.isneginf(e), 0, e)
            np.testing.assert_array_equal(g, e, err_msg=f"rank {rank}: {name}")
