"""ColBERT first-stage search at corpus scale on the GPU (csrc/centroid.hip, ops.centroid_*, ShardedCentroidIndex,
ShardedTokenIndex.search, Ranker.multi_vector_search_topk).

1. The candidate-score plane equals the numpy restatement (centroid_cases.approx_plane) bit for bit: planted lists and probes, with and
   without the slice table, sub-ranges, two runs.
2. The filter entry's candidates are exactly {d : !(plane[d] <= tau)}; ids beyond 2^31; a capacity smaller than the survivors.
3. A shard's streamed top-k == the two-pass one == the top-k of the restatement's plane; forced overflow; three sub-indexes merged; padding.
4. Assignment: copies of equal-norm centroids get their source id back; on random tokens the chosen centroid is a float64 maximum to 1e-6.
5. End to end with nprobe = K on exact-grid inputs: the search returns the ids and score bits of the all-pairs plane's top-k.
6. End to end on clustered unit-norm tokens: every returned score is the all-pairs plane's entry, lists descend, ids come from the
   candidate stage, and the result fuses next to a dense list.
7. Ranker.multi_vector_search_topk == index.search on the encoder's query tokens."""
import numpy as np
import pytest
import torch

import centroid_cases as CC
import maxsim_cases as M
from helpers import planned_search_marks

pytestmark = pytest.mark.gpu

# (Lq, nprobe).  37 * 7 = 259 and 40 * 8 = 320 probes: more than one 256-probe table (the kernel packs whole tokens, 36 and 32 per table).
# nprobe = 300 and 257: a token wider than the table, resolved 256 probes at a time, once per phase (the kernel's other branch).
PLANE_SHAPES = [(1, 1), (5, 3), (64, 4), (37, 7), (40, 8), (2, 300), (3, 257)]
K_PLANE = 301


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


@pytest.fixture(scope="module")
def G(ops):
    return ops.centroid_slice_docs()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def make_index(ops, lists, N, table=True):
    coff_h, cdoc_h = CC.index_from_lists(lists)
    coff, cdoc = dev(coff_h), dev(cdoc_h)
    so = ops.centroid_slice_offsets(coff, cdoc, len(lists), N) if table else None
    return ops.CentroidIndex(coff, cdoc, N, len(lists), so), coff_h, cdoc_h


_plane_cache = {}


def plane_case(G, Lq, nprobe):
    """(lists, pc, ps, N, the restatement's plane) of one shape: computed once, shared, left unchanged."""
    key = (Lq, nprobe)
    if key not in _plane_cache:
        N = 2 * G + 37
        rng = np.random.default_rng(1000 * Lq + nprobe)
        lists, pc, ps = CC.planted_case(rng, N, K_PLANE, 3, Lq, nprobe)
        coff, cdoc = CC.index_from_lists(lists)
        _plane_cache[key] = (lists, pc, ps, N, CC.approx_plane(coff, cdoc, pc, ps, Lq, nprobe, N))
    return _plane_cache[key]


# ---- 1. the plane ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "search"])
@pytest.mark.parametrize("Lq,nprobe", PLANE_SHAPES)
def test_plane_equals_the_restatement_bit_for_bit(ops, G, Lq, nprobe, table):
    lists, pc_h, ps_h, N, ref = plane_case(G, Lq, nprobe)
    # the planted cases are there
    assert len(lists[0]) == 0 and len(lists[1]) == N and 1 in pc_h[0, :nprobe] and not (pc_h[1] == 1).any()
    assert (ref[1] < 0).any() and (ref[1] == 0).any() and (ref[1] <= 0).all()
    assert nprobe < 2 or (pc_h[2].reshape(Lq, nprobe)[:, -1] == -1).all()
    if nprobe > 256:       # padding inside the second batch of every token, and live probes there too
        second = pc_h[2].reshape(Lq, nprobe)[:, 256:]
        assert (second == -1).any(1).all() and (nprobe == 257 or ((second >= 0).any(1).all() and (second == -1).sum() > Lq))
    assert len(np.unique(ps_h[2])) < ps_h[2].size or ps_h[2].size == 1
    index, _, _ = make_index(ops, lists, N, table)
    assert (index.slice_off is not None) == table
    pc, ps = dev(pc_h), dev(ps_h)
    plane = ops.centroid_scores(index, pc, ps, Lq, nprobe)
    assert tuple(plane.shape) == (3, N)
    assert torch.equal(bits(plane), bits(dev(ref)))
    again = ops.centroid_scores(index, pc, ps, Lq, nprobe)
    assert torch.equal(bits(again), bits(plane))
    tail = ops.centroid_scores(index, pc, ps, Lq, nprobe, doc_lo=G)
    assert tuple(tail.shape) == (3, N - G) and torch.equal(bits(tail), bits(plane[:, G:]))
    mid = ops.centroid_scores(index, pc, ps, Lq, nprobe, doc_lo=G, doc_hi=2 * G, out=ops.alloc_plane(3, G, torch.float32, "cuda"))
    assert torch.equal(bits(mid), bits(plane[:, G: 2 * G]))
    with pytest.raises(ValueError):
        ops.centroid_scores(index, pc, ps, Lq, nprobe, doc_lo=G - 64)
    with pytest.raises(ValueError):
        ops.centroid_scores(index, pc, ps, Lq, nprobe, doc_hi=G + 1)


def test_max_not_sum_and_added_twice(ops, G):
    """Two tokens, two probes each, written out by hand: document 7 is in the lists of centroids 2 and 3."""
    N = G + 9
    lists = [np.zeros(0, dtype=np.int32), np.arange(N, dtype=np.int32), np.array([7, 20], dtype=np.int32), np.array([7, G + 1], dtype=np.int32)]
    index, _, _ = make_index(ops, lists, N)
    pc = dev(np.array([[2, 3, 2, 0]], dtype=np.int32))
    ps = dev(np.array([[0.75, 0.5, -0.25, 9.0]], dtype=np.float32))
    got = ops.centroid_scores(index, pc, ps, 2, 2).cpu().numpy()[0]
    want = np.zeros(N, dtype=np.float32)
    want[7], want[20], want[G + 1] = 0.75 - 0.25, 0.75 - 0.25, 0.5     # the max of token 0 (not 1.25), centroid 2 added for both tokens
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- 2. the filter -----------------------------------------------------------------------------------------------------------------
def run_filter(ops, index, pc, ps, Lq, nprobe, lo, hi, id_base, tau, cap, canary=-7.0):
    Q = pc.shape[0]
    cs = torch.full((Q + 1, cap), canary, dtype=torch.float32, device="cuda")       # row Q: what a write at or past cap of row Q - 1 would hit
    ci = torch.full((Q + 1, cap), -99, dtype=torch.int64, device="cuda")
    cl = torch.zeros(Q, dtype=torch.int32, device="cuda")
    ov = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.centroid_filter(index, pc, ps, Lq, nprobe, lo, hi, id_base, tau, cs[:Q], ci[:Q], cl, ov)
    torch.cuda.synchronize()
    return cs.cpu().numpy(), ci.cpu().numpy(), cl.cpu().numpy(), int(ov.item())


@pytest.mark.parametrize("table", [True, False], ids=["slice_off", "search"])
@pytest.mark.parametrize("Lq,nprobe", [(5, 3), (2, 300)])       # a table of whole tokens / a token wider than the table
def test_filter_candidates_are_what_beats_tau(ops, G, Lq, nprobe, table):
    lists, pc_h, ps_h, N, ref = plane_case(G, Lq, nprobe)
    index, _, _ = make_index(ops, lists, N, table)
    pc, ps = dev(pc_h), dev(ps_h)
    id_base = (1 << 33) + 5
    tau_h = np.array([np.median(ref[0]), np.inf, -np.inf], dtype=np.float32)
    for lo, hi in ((0, N), (G, N), (G, 2 * G)):
        cap = N                                                             # the range is no larger than cap: tau = -inf keeps all of it
        cs, ci, cl, ov = run_filter(ops, index, pc, ps, Lq, nprobe, lo, hi, id_base, dev(tau_h), cap)
        assert ov == 0
        for q in range(3):
            keep = np.nonzero(~(ref[q, lo:hi] <= tau_h[q]))[0] + lo
            assert cl[q] == len(keep), (q, lo, hi)
            order = np.argsort(ci[q, :cl[q]])
            assert np.array_equal(ci[q, :cl[q]][order], keep + id_base)
            assert np.array_equal(cs[q, :cl[q]][order].view(np.int32), ref[q, keep].view(np.int32))
            assert (cs[q, cl[q]:] == -7.0).all() and (ci[q, cl[q]:] == -99).all()
        assert cl[1] == 0 and cl[2] == hi - lo and 0 < cl[0] < hi - lo
        assert (cs[3] == -7.0).all() and (ci[3] == -99).all()


def test_filter_overflow_sets_the_flag_and_writes_nothing_past_cap(ops, G):
    Lq, nprobe = 5, 3
    lists, pc_h, ps_h, N, ref = plane_case(G, Lq, nprobe)
    index, _, _ = make_index(ops, lists, N)
    cap, id_base = 48, 1 << 40
    tau = dev(np.full(3, -np.inf, dtype=np.float32))
    cs, ci, cl, ov = run_filter(ops, index, dev(pc_h), dev(ps_h), Lq, nprobe, 0, N, id_base, tau, cap)
    assert ov == 1 and (cl == N).all()                                       # the count runs past cap
    assert (cs[3] == -7.0).all() and (ci[3] == -99).all()                    # the canary row: nothing at or past cap
    for q in range(3):
        d = ci[q] - id_base
        assert len(set(d.tolist())) == cap and d.min() >= 0 and d.max() < N   # cap distinct survivors, each with its own score
        assert np.array_equal(cs[q].view(np.int32), ref[q, d].view(np.int32))


def test_filter_at_exactly_cap_and_one_past_it(ops, G):
    """One full slice and a ragged tail; query q probes centroid q alone.  Query 0 ties tau on every document (no survivor: the rule is
    !(score <= tau)), query 1 has exactly cap survivors, query 2 cap + 1 over both slices.  With query 2 switched off (tau = inf) every
    slot of query 1 is written and the flag stays 0; with it on the flag is 1, the count is cap + 1 and the guard row is untouched."""
    N, cap, id_base = G + 37, 64, (1 << 35) + 3
    rng = np.random.default_rng(7)
    hit1 = np.sort(np.concatenate([rng.choice(G, 44, replace=False), G + rng.choice(37, 20, replace=False)])).astype(np.int32)
    hit2 = np.sort(np.concatenate([rng.choice(G, 40, replace=False), G + rng.choice(37, 25, replace=False)])).astype(np.int32)
    lists = [np.arange(N, dtype=np.int32), hit1, hit2]
    pc_h = np.array([[0, -1], [1, -1], [-1, 2]], dtype=np.int32)
    ps_h = np.array([[0.5, 9.0], [0.75, 9.0], [9.0, 0.75]], dtype=np.float32)
    coff, cdoc = CC.index_from_lists(lists)
    ref = CC.approx_plane(coff, cdoc, pc_h, ps_h, 1, 2, N)
    tau_h = np.full(3, 0.5, dtype=np.float32)
    keep = [np.flatnonzero(~(ref[q] <= tau_h[q])) for q in range(3)]
    assert [len(x) for x in keep] == [0, cap, cap + 1] and keep[2][0] < G <= keep[2][-1] and keep[1][0] < G <= keep[1][-1]
    index, _, _ = make_index(ops, lists, N)
    pc, ps = dev(pc_h), dev(ps_h)
    cs, ci, cl, ov = run_filter(ops, index, pc, ps, 1, 2, 0, N, id_base, dev(np.array([0.5, 0.5, np.inf], dtype=np.float32)), cap)
    assert ov == 0 and cl.tolist() == [0, cap, 0]
    assert np.array_equal(np.sort(ci[1]), keep[1] + id_base) and (cs[1] == 0.75).all()       # every slot written
    assert (cs[[0, 2, 3]] == -7.0).all() and (ci[[0, 2, 3]] == -99).all()
    cs, ci, cl, ov = run_filter(ops, index, pc, ps, 1, 2, 0, N, id_base, dev(tau_h), cap)
    assert ov == 1 and cl.tolist() == [0, cap, cap + 1]
    assert np.array_equal(np.sort(ci[1]), keep[1] + id_base) and (cs[1] == 0.75).all()
    d = ci[2] - id_base
    assert len(set(d.tolist())) == cap and set(d.tolist()) <= set(keep[2].tolist())          # cap distinct survivors ...
    assert np.array_equal(cs[2].view(np.int32), ref[2, d].view(np.int32))                    # ... each with its own score
    assert (cs[[0, 3]] == -7.0).all() and (ci[[0, 3]] == -99).all()                          # nothing for query 0, nothing past cap


# ---- 3. shard search ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shard(ops, G):
    from fusion_amd.distributed import ShardedCentroidIndex
    probe_index = ShardedCentroidIndex(None, 0)
    head = probe_index.head_docs(1000)
    assert head == probe_index.head_docs(1) == probe_index.head_docs(64) and head % G == 0
    N, K, Q, Lq, nprobe = head + 3 * G + 11, 301, 5, 8, 4
    rng = np.random.default_rng(77)
    lists = CC.random_lists(rng, N, K, mean=16, full=(), empty=(0,))
    lists[9] = np.arange(head + G + 100, head + G + 700, dtype=np.int32)     # 600 documents of one late slice ...
    pc, ps = CC.random_probes(rng, Q, Lq, nprobe, K)
    pc[pc == 9] = 10
    pc[:, 0], ps[:, 0] = 9, 50.0                                             # ... that beat everything before them, for every query
    coff, cdoc = CC.index_from_lists(lists)
    ref = CC.approx_plane(coff, cdoc, pc, ps, Lq, nprobe, N)
    # more than 64 and fewer than 1000 documents above zero, some below: k = 1000 ends in the zeros, which fill by ascending id
    assert ((ref > 0).sum(1) > 600).all() and ((ref > 0).sum(1) < 1000).all() and ((ref < 0).sum(1) > 0).all() and ((ref == 0).sum(1) > 1000).all()
    return dict(lists=lists, pc=pc, ps=ps, N=N, K=K, Lq=Lq, nprobe=nprobe, ref=ref, head=head)


@pytest.mark.parametrize("k", [1, 64, 1000])
def test_shard_topk_streamed_two_pass_and_reference_agree(ops, shard, k):
    from fusion_amd.distributed import ShardedCentroidIndex
    s = shard
    id_base = (1 << 35) + 3
    index, _, _ = make_index(ops, s["lists"], s["N"])
    sh = ShardedCentroidIndex(index, id_base)
    q = (dev(s["pc"]), dev(s["ps"]), s["Lq"], s["nprobe"])
    want_s, want_i = CC.topk_ref(s["ref"], k, id_base)
    assert sh._streams(k, s["N"])
    marks = []
    got_s, got_i = sh.local_topk(*q, k, mark=marks.append, streaming=True)
    assert "shard_centroid" in marks and "shard_centroid_filter" in marks
    assert torch.equal(got_i, dev(want_i)) and torch.equal(bits(got_s), bits(dev(want_s)))
    two_s, two_i = sh.two_pass_topk(q, k)
    assert torch.equal(two_i, got_i) and torch.equal(bits(two_s), bits(got_s))
    marks.clear()
    off_s, off_i = sh.local_topk(*q, k, mark=marks.append)                    # the class default: the two-pass route
    assert not sh.STREAMING and "shard_centroid_filter" not in marks and "shard_centroid" in marks
    assert torch.equal(off_i, got_i) and torch.equal(bits(off_s), bits(got_s))
    if k == 1000:
        assert (want_s[:, -1] == 0).all() and (np.diff(want_i[:, -50:], axis=1) > 0).all()      # zeros fill by ascending id
    sh.CAP = 256                                                             # 600 late documents beat the head's k-th best: a window overflows
    low_s, low_i = sh.local_topk(*q, k, streaming=True)
    assert sh.last_overflow > 0
    assert torch.equal(low_i, got_i) and torch.equal(bits(low_s), bits(got_s))


@pytest.mark.parametrize("k", [64, 1000])
def test_three_sub_indexes_merge_to_the_whole(ops, shard, k):
    from fusion_amd.distributed import ShardedCentroidIndex
    s = shard
    base = 5_000_000_000
    want_s, want_i = CC.topk_ref(s["ref"], k, base)
    q = (dev(s["pc"]), dev(s["ps"]), s["Lq"], s["nprobe"])
    cuts = [0, s["head"] + 1234, s["N"] - 500, s["N"]]                       # the last shard is smaller than k = 1000
    parts_s, parts_i = [], []
    for lo, hi in zip(cuts, cuts[1:]):
        sub = [l[(l >= lo) & (l < hi)] - lo for l in s["lists"]]
        index, _, _ = make_index(ops, sub, hi - lo, table=(lo == 0))
        ps_, pi_ = ShardedCentroidIndex(index, base + lo).local_topk(*q, k, streaming=True)     # the first part streams, the others are too small
        parts_s.append(ps_); parts_i.append(pi_)
    if k == 1000:
        assert (parts_i[2][:, 500:] == -1).all() and torch.isneginf(parts_s[2][:, 500:]).all() and (parts_i[2][:, :500] >= 0).all()
    got_s, got_i = ops.topk_merge(torch.stack(parts_s), torch.stack(parts_i))
    assert torch.equal(got_i, dev(want_i)) and torch.equal(bits(got_s), bits(dev(want_s)))
    whole, _, _ = make_index(ops, s["lists"], s["N"])
    one_s, one_i = ShardedCentroidIndex(whole, base).search(*q, k=k)         # one rank: the all-gather merge of a single list
    assert torch.equal(one_i, got_i) and torch.equal(bits(one_s), bits(got_s))


def test_streamed_search_launches_one_kernel_per_planned_piece(ops, shard, G):
    """The marks of a streamed ShardedCentroidIndex.local_topk are the ones the piece planner predicts (as for the dense and the sparse
    index): the head's plane and the opening of the stream, one shard_centroid_filter per planned piece with a shard_topk_stream after
    every planned fold, the closing fold.  Head + three slices + 11 documents in feeds of two slices; k = 100 with CAP = 256 makes the
    first window three slices long (128 * 10,752 / 100, rounded down to whole slices), so the second feed starts inside it."""
    from fusion_amd.distributed import ShardedCentroidIndex
    s = shard
    k, Q, id_base = 100, 3, (1 << 35) + 3
    index, _, _ = make_index(ops, s["lists"], s["N"])
    sh = ShardedCentroidIndex(index, id_base)
    sh.CAP, sh.CHUNK = 256, 2 * G
    head = sh.head_docs(k)
    assert head == s["head"] == 3 * G and s["N"] == head + 3 * G + 11 and sh._streams(k, s["N"])
    exp, folds, inside = planned_search_marks(ops, head, s["N"], sh.CHUNK, k, sh.CAP, G, "shard_centroid", "shard_centroid_filter")
    assert exp.pop() == "allgather_merge"
    assert folds >= 1 and inside >= 1
    marks = []
    got_s, got_i = sh.local_topk(dev(s["pc"][:Q]), dev(s["ps"][:Q]), s["Lq"], s["nprobe"], k, mark=marks.append, streaming=True)
    assert marks == exp
    want_s, want_i = CC.topk_ref(s["ref"][:Q], k, id_base)
    assert torch.equal(got_i, dev(want_i)) and torch.equal(bits(got_s), bits(dev(want_s)))


# ---- 4. assignment -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sign_corpus():
    """600 documents of 1-40 tokens, every token a copy of one of K = 64 equal-norm sign-pattern centroids."""
    rng = np.random.default_rng(4)
    C = CC.sign_centroids(rng, 64)
    lens = rng.integers(1, 41, 600)
    Doff = CC.doc_offsets(lens)
    src = rng.integers(0, 64, int(Doff[-1])).astype(np.int32)
    return C, C[src], Doff, src


def test_assignment_returns_the_source_centroid(ops, sign_corpus, monkeypatch):
    C, Dtok, Doff, src = sign_corpus
    want = dev(src)
    assert torch.equal(ops.centroid_assign(dev(Dtok), dev(C)), want)
    monkeypatch.setattr(ops, "CENTROID_BLOCK_BYTES", 64 * 1024)              # 256 token rows per block: the chunk loop
    assert torch.equal(ops.centroid_assign(dev(Dtok), dev(C)), want)


def test_assignment_picks_a_float64_maximum(ops, sign_corpus):
    C = sign_corpus[0]
    rng = np.random.default_rng(8)
    tok, _ = M.unit_corpus(rng, [2000])
    Cn = (C.astype(np.float64) / np.sqrt(32.0)).astype(np.float16)           # unit-scale centroids
    codes = ops.centroid_assign(dev(tok), dev(Cn)).cpu().numpy()
    dots = tok.astype(np.float64) @ Cn.astype(np.float64).T
    assert codes.dtype == np.int32 and codes.min() >= 0 and codes.max() < 64
    # an fp32 dot of 128 unit-scale terms: its error is far below 1e-6
    assert (dots.max(1) - dots[np.arange(2000), codes] <= 1e-6).all()


def test_kmeans_keeps_the_centroid_of_a_cluster_without_rows(ops):
    """Two distinct token rows, eight centroids: the start holds duplicates, ties go to the lowest id, so at least six clusters lose every
    row -- they must keep their centroid, not become the normalised zero vector."""
    rng = np.random.default_rng(31)
    which = rng.integers(0, 2, 200)
    tok = np.zeros((200, 128), dtype=np.float16)
    tok[np.arange(200), which * 40 + 5] = 1.0                                # axes 5 and 45: unit rows, exact in float16
    C = ops.kmeans_centroids(dev(tok), 8, iters=3, seed=3)
    assert tuple(C.shape) == (8, 128) and bool(torch.isfinite(C).all())
    assert ((C.float().norm(dim=1) - 1).abs() < 2e-3).all()                  # a cluster without rows is not the zero vector
    assert bool((C.float()[:, [5, 45]].abs().sum(1) > 0.99).all()) and bool((C.float().abs().sum(1) < 1.5).all())     # made of the two rows only
    codes = ops.centroid_assign(dev(tok), C).cpu().numpy()
    assert len(set(codes.tolist())) <= 2                                      # two clusters at most hold rows: six kept their centroid


def test_device_index_equals_the_set_construction(ops, sign_corpus, G):
    C, Dtok, Doff, src = sign_corpus
    coff, cdoc, _ = CC.index_ref(src, Doff, 64)
    idx = ops.centroid_index(dev(src), dev(Doff), 64)
    assert np.array_equal(idx.coff.cpu().numpy(), coff) and np.array_equal(idx.cdoc.cpu().numpy(), cdoc)
    assert tuple(idx.slice_off.shape) == (64, 2)
    assert np.array_equal(idx.slice_off.cpu().numpy(), np.stack([coff[:-1], coff[1:]], 1))
    assert ops.centroid_index(dev(src), dev(Doff), 64, slice_table_max_bytes=64).slice_off is None      # above the cap: the kernels search


def test_probes_are_the_best_centroids_token_major(ops, sign_corpus):
    C = sign_corpus[0]
    rng = np.random.default_rng(12)
    Qtok = M.grid_queries(rng, 3, 32)
    S = Qtok.astype(np.float64).reshape(96, 128) @ C.astype(np.float64).T    # exact on the grid
    pc, ps = ops.centroid_probes(dev(Qtok), dev(C), 5)
    assert tuple(pc.shape) == tuple(ps.shape) == (3, 160) and pc.dtype == torch.int32 and ps.dtype == torch.float32
    want_c = np.stack([np.lexsort((np.arange(64), -S[r]))[:5] for r in range(96)])
    assert np.array_equal(pc.cpu().numpy().reshape(96, 5), want_c)
    assert np.array_equal(ps.cpu().numpy().reshape(96, 5).astype(np.float64), np.take_along_axis(S, want_c, 1))
    pc2, ps2 = ops.centroid_probes(dev(Qtok), dev(C[:3]), 5)                 # nprobe > K: padded
    assert (pc2.view(96, 5)[:, 3:] == -1).all() and (pc2.view(96, 5)[:, :3] >= 0).all()


# ---- 5. end to end, exhaustive limit -------------------------------------------------------------------------------------------------
def test_search_with_every_centroid_probed_is_the_exact_search(ops, sign_corpus):
    from fusion_amd.distributed import ShardedTokenIndex
    C, Dtok_h, Doff_h, src = sign_corpus
    rng = np.random.default_rng(5)
    Qtok = dev(M.grid_queries(rng, 6, 32))
    Dtok, Doff = dev(Dtok_h), dev(Doff_h)
    id_base = 7000
    index = ShardedTokenIndex(Dtok, Doff, id_base).build_centroids(dev(C))
    assert torch.equal(index.candidates.index.cdoc, ops.centroid_index(dev(src), Doff, 64).cdoc)
    out = index.search(Qtok, k=50, nprobe=64, ncand=200)
    want_s, want_i = ops.topk_rows(ops.maxsim(Qtok, Dtok, Doff), 50, id_base=id_base)
    assert out.lens.tolist() == [50] * 6
    assert torch.equal(out.ids, want_i) and torch.equal(bits(out.scores), bits(want_s))


# ---- 6. end to end, realistic --------------------------------------------------------------------------------------------------------
def test_search_on_clustered_tokens_returns_exact_scores_of_its_candidates(ops):
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator
    rng = np.random.default_rng(6)
    centres = rng.normal(0, 1, (96, 128))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    lens = rng.integers(1, 41, 3000)
    Doff_h = CC.doc_offsets(lens)
    Dtok_h, _ = CC.clustered_tokens(rng, int(Doff_h[-1]), centres)
    Qtok_h, _ = CC.clustered_tokens(rng, 8 * 32, centres)
    Qtok, Dtok, Doff = dev(Qtok_h.reshape(8, 32, 128)), dev(Dtok_h), dev(Doff_h)
    C = ops.kmeans_centroids(Dtok, 128, iters=3, seed=1, sample=20000)
    assert tuple(C.shape) == (128, 128) and C.dtype == torch.float16
    assert torch.equal(C, ops.kmeans_centroids(Dtok, 128, iters=3, seed=1, sample=20000))      # deterministic for a seed
    assert ((C.float().norm(dim=1) - 1).abs() < 2e-3).all()
    id_base = 40_000
    index = ShardedTokenIndex(Dtok, Doff, id_base).build_centroids(C)
    out = index.search(Qtok, k=100, nprobe=2, ncand=256)
    plane = ops.maxsim(Qtok, Dtok, Doff)
    assert tuple(out.ids.shape) == (8, 100) and out.lens.tolist() == [100] * 8
    local = out.ids - id_base
    assert int(local.min()) >= 0 and int(local.max()) < 3000
    assert torch.equal(bits(out.scores), bits(torch.gather(plane, 1, local)))          # every returned score is exact
    assert (out.scores[:, 1:] <= out.scores[:, :-1]).all()
    pc, ps = ops.centroid_probes(Qtok, C, 2)
    _, cand = index.candidates.search(pc, ps, 32, 2, 256)
    for q in range(8):
        ids = out.ids[q].tolist()
        assert len(set(ids)) == 100 and set(ids) <= set(cand[q].tolist())
    # the 100 best of the candidates, not just any 100
    cs = torch.gather(plane, 1, cand - id_base)
    assert torch.equal(bits(out.scores), bits(torch.sort(cs, dim=1, descending=True).values[:, :100]))
    dense_ids = np.stack([rng.permutation(3000)[:100] for _ in range(8)]).astype(np.int64) + id_base
    dense = RankedTopk.from_search(dev(-np.sort(-rng.random((8, 100)).astype(np.float32), axis=1)), dev(dense_ids))
    fused = Aggregator.fuse_topk({"dpr": dense, "colbert": out}, "rrf", None, {"dpr": 0.5, "colbert": 0.5}, {})
    assert int(fused.lens.min()) >= 100 and int(fused.lens.max()) <= 200
    with pytest.raises(ValueError):
        index.search(Qtok, k=300, ncand=200)
    with pytest.raises(ValueError):
        ShardedTokenIndex(Dtok, Doff, id_base).search(Qtok, k=10)


# ---- 7. the Ranker ---------------------------------------------------------------------------------------------------------------
def test_ranker_search_topk_equals_index_search(ops):
    from fusion_amd import encoders
    from fusion_amd.distributed import ShardedTokenIndex
    from fusion_amd.retrievers.hybrid import Ranker
    enc = encoders.random_init("colbert", size="tiny")
    rng = np.random.default_rng(21)
    words = [f"w{i}" for i in range(300)]
    docs = [" ".join(rng.choice(words, size=int(rng.integers(3, 40)))) for _ in range(120)]
    queries = [" ".join(rng.choice(words, size=int(rng.integers(2, 9)))) for _ in range(5)]
    index = ShardedTokenIndex.from_encoder(enc, docs, id_base=5000)
    index.build_centroids(ops.kmeans_centroids(index.Dtok, 16, iters=2, seed=0))
    out = Ranker.multi_vector_search_topk(queries, index, encoder=enc, return_topk=20, nprobe=2, ncand=40)
    want = index.search(enc.encode_queries(queries, batch_size=64), k=20, nprobe=2, ncand=40)
    assert tuple(out.ids.shape) == (5, 20) and out.lens.tolist() == [20] * 5
    assert torch.equal(out.ids, want.ids) and torch.equal(bits(out.scores), bits(want.scores)) and torch.equal(out.lens, want.lens)
