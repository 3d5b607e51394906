"""Corpus-scale SPLADE search on the device: the posting walk over a document range (fz_sparse_dot_range_f32), the walk with the streaming
top-k filter fused in (fz_sparse_dot_filter_f32, TopkStream.feed_sparse), the sharded index (distributed.ShardedSparseIndex) and the
public surface (SpladeEncoder.index / search, splade/base.py:199-251).  The fused search must return exactly -- ids and score bits -- what
the top-k of the full score plane returns."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import assert_ranked_close, planned_search_marks

pytestmark = pytest.mark.gpu

COS_TOL = 2e-6        # as tests/test_gpu_parity_r2.py
S = 7168
V = 32005
N_BIG = 250_003       # not a multiple of 7,168
N_ALIGNED = 34 * S    # 243,712: a multiple of it
Q_BIG = 195
BASE = 3 << 31        # a shard's first global id beyond 32 bits


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def splade_blocks(seed, N, nnz, block=8192, V=V, dup=True):
    """SPLADE-shaped rows [n, V padded to 4] in blocks, generated on the device: ~nnz Zipf-distributed terms per row with log1p(relu(.))
    weights; with `dup` every row 4096 j + 7 is a copy of row 4096 j + 3 (planted duplicate documents).  Deterministic for a seed."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = 1.0 / torch.arange(1, V + 1, device="cuda", dtype=torch.float64) ** 0.9
    p = (p / p.sum()).float()
    for r0 in range(0, N, block):
        n = min(block, N - r0)
        cols = torch.multinomial(p, n * nnz, replacement=True, generator=g).view(n, nnz)
        w = torch.log1p(torch.clamp(torch.randn((n, nnz), generator=g, device="cuda") + 1.0, min=0.05))
        X = torch.zeros((n, -(-V // 4) * 4), device="cuda")
        X.scatter_reduce_(1, cols, w, reduce="amax")          # (deterministic where a term is drawn twice)
        if dup:
            for j in range(3, n - 4, 4096):
                X[j + 4] = X[j]
        yield r0, X


def build_index(ops, seed, N, nnz=120):
    return ops.sparse_index_from_blocks(splade_blocks(seed, N, nnz), V, N=N)


@pytest.fixture(scope="module")
def big(ops):
    """(index of N_BIG documents, index of its first N_ALIGNED, dense queries [Q_BIG, V], their term lists, the full score plane)."""
    idx = build_index(ops, 11, N_BIG)
    idx_al = build_index(ops, 11, N_ALIGNED)
    Qd = next(splade_blocks(12, Q_BIG, 40, block=Q_BIG, dup=False))[1]
    Qd[0].zero_()                                                      # a query without terms
    counts = (idx.toff[1:] - idx.toff[:-1]).cpu().numpy()
    held = np.flatnonzero(counts > 0)
    rare = int(held[np.argmin(counts[held])])                          # the term the fewest documents hold (fewer than 1000) ...
    assert counts[rare] < 1000
    Qd[1].zero_(); Qd[1, rare] = 0.7                                   # ... and a query that asks only for it
    Qd[2] = Qd[3]                                                      # duplicate queries
    ql = ops.sparse_rows(Qd, V)
    full = ops.sparse_dot(idx, *ql)
    return idx, idx_al, Qd, ql, full, int(counts[rare])


# ---- 1. reference parity: splade/base.py's search on the round-2 fixture ------------------------------------------------------------
@pytest.mark.parametrize("sim", ["cos_sim", "dot_score"])
def test_search_matches_reference(ops, sim):
    from fusion_amd import encoders
    from fusion_amd.distributed import ShardedSparseIndex
    z = np.load(os.path.join(GOLDEN, "search_Q6_N1000_d64.npz"))
    Qe, De = (torch.from_numpy(np.ascontiguousarray(z[n])).cuda() for n in ("Qe", "De"))
    Q, N = Qe.shape[0], De.shape[0]
    if sim == "cos_sim":
        Qn, Dn = ops.normalize_rows(Qe), ops.normalize_rows(De)
        tol = COS_TOL
    else:
        Qn, Dn = Qe, De
        tol = COS_TOL * float(np.max(np.abs(z[f"scores__{sim}__kN_qc100_dc500000"])))
    idx = ops.sparse_index(Dn)
    enc = encoders.random_init("splade", size="tiny")
    enc.similarity = sim
    for cfg in z["configs"]:
        name, k, qc, dc = str(cfg).split(":")
        k, qc, dc = int(k), int(qc), int(dc)
        e_ids, e_sc = z[f"ids__{sim}__{name}"], z[f"scores__{sim}__{name}"]
        shard = ShardedSparseIndex(idx, id_base=0)
        shard.CHUNK = ops.round_up(dc, S)
        c_sc, c_ids = shard.search(*ops.sparse_rows(Qn), k=min(k, N))
        res = enc.search_index(Qe, idx, query_chunk_size=qc, doc_chunk_size=dc, topk=k)
        assert len(res) == Q
        for q in range(Q):
            assert_ranked_close(c_ids[q].cpu().numpy(), c_sc[q].cpu().numpy(), e_ids[q], e_sc[q], tol, truncated=k < N)
            assert len(res[q]) == min(k, N)
            assert_ranked_close([r["doc_id"] for r in res[q]], [r["score"] for r in res[q]], e_ids[q], e_sc[q], tol, truncated=k < N)


# ---- 2. a range's columns are the full plane's, bit for bit ------------------------------------------------------------------------
def test_range_scores_are_the_full_planes_columns(ops, big):
    idx, _, _, ql, full, _ = big
    assert tuple(full.shape) == (Q_BIG, N_BIG)
    nos = ops.SparseIndex(idx.toff, idx.pdoc, idx.pw, idx.N, idx.V, slice_off=idx.slice_off)
    nos.slice_off = None                                               # the binary-search path
    for lo, hi in [(0, S), (S, 2 * S), (5 * S, 9 * S), (34 * S, N_BIG), (14 * S, N_BIG), (0, N_BIG), (7 * S, 7 * S)]:
        for index in (idx, nos):
            part = ops.sparse_dot(index, *ql, doc_lo=lo, doc_hi=hi)
            assert tuple(part.shape) == (Q_BIG, hi - lo)
            assert torch.equal(part, full[:, lo:hi]), (lo, hi, index.slice_off is None)
    assert torch.equal(ops.sparse_dot(nos, *ql), full)
    with pytest.raises(ValueError):
        ops.sparse_dot(idx, *ql, doc_lo=100, doc_hi=S)
    with pytest.raises(ValueError):
        ops.sparse_dot(idx, *ql, doc_lo=0, doc_hi=S + 1)


# ---- 3. fused == exact, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("k", [1, 100, 1000])
def test_fused_topk_equals_the_full_planes_topk(ops, big, k, aligned):
    from fusion_amd.distributed import ShardedSparseIndex
    idx, idx_al, _, ql, full, _ = big
    index = idx_al if aligned else idx
    plane = full[:, :index.N]
    n_rare = int((plane[1] > 0).sum())                                 # documents that hold query 1's one term
    assert 0 < n_rare < 1000
    for id_base in (0, BASE):
        e_sc, e_ids = ops.topk_rows(plane, k, id_base=id_base)
        for cap, chunk in ((7168, 32 * S), (max(2 * k, 256), 5 * S)):   # the shipped sizes; a small cap and chunk: many windows and folds
            shard = ShardedSparseIndex(index, id_base)
            shard.CAP, shard.CHUNK = cap, chunk
            g_sc, g_ids = shard.local_topk(*ql, k)
            assert torch.equal(g_ids, e_ids), (k, id_base, cap)
            assert torch.equal(g_sc, e_sc), (k, id_base, cap)
    g_ids = g_ids.cpu().numpy() - BASE
    g_sc = g_sc.cpu().numpy()
    # a query with no terms: the first k documents, all scoring 0
    assert np.array_equal(g_ids[0], np.arange(k)) and np.all(g_sc[0] == 0.0)
    # one rare term: its documents first, then the zero-score tail in ascending id
    m = min(k, n_rare)
    assert np.all(g_sc[1, :m] > 0.0)
    if k > n_rare:
        tail = g_ids[1, n_rare:]
        assert np.all(g_sc[1, n_rare:] == 0.0) and np.all(np.diff(tail) > 0)
    assert np.array_equal(g_ids[2], g_ids[3]) and np.array_equal(g_sc[2], g_sc[3])


def test_planted_duplicates_rank_next_to_each_other(ops, big):
    """Documents 4096 j + 3 and 4096 j + 7 are copies: equal scores, the lower id first."""
    from fusion_amd.distributed import ShardedSparseIndex
    idx, _, _, ql, full, _ = big
    k = 1000
    shard = ShardedSparseIndex(idx, 0)
    g_sc, g_ids = (t.cpu().numpy() for t in shard.local_topk(*ql, k))
    pf = full.cpu().numpy()
    seen = 0
    for q in range(4, Q_BIG):
        pos = {int(d): r for r, d in enumerate(g_ids[q])}
        for a in range(3, N_BIG - 4, 4096):
            assert pf[q, a] == pf[q, a + 4]
            if a in pos and a + 4 in pos and pf[q, a] > 0.0:
                ra, rb = pos[a], pos[a + 4]
                between = g_sc[q, ra:rb + 1]
                assert rb > ra and np.all(between == g_sc[q, ra])
                seen += 1
    assert seen > 0


def test_k_beyond_the_shard_pads(ops, big):
    from fusion_amd.distributed import ShardedSparseIndex
    idx, _, Qd, _, _, _ = big
    small = ops.sparse_index(Qd[:, :V].contiguous(), V)          # a 195-document shard
    ql = ops.sparse_rows(Qd[:5], V)
    plane = ops.sparse_dot(small, *ql)
    for k in (195, 300, 1000):
        s, i = ShardedSparseIndex(small, 17).local_topk(*ql, k)
        e_s, e_i = ops.topk_rows(plane, k, id_base=17)
        assert torch.equal(s, e_s) and torch.equal(i, e_i)
        if k > 195:
            assert torch.all(i[:, 195:] == -1) and torch.all(torch.isneginf(s[:, 195:]))
    s, i = ShardedSparseIndex(small, 0).local_topk(*ops.sparse_rows(Qd[:0], V), 10)
    assert s.shape == (0, 10) and i.shape == (0, 10)


def test_search_launches_one_kernel_per_planned_piece(ops, big):
    """The marks of ShardedSparseIndex.search are the ones the piece planner predicts: the head, then per CHUNK feed one shard_sparse_filter
    per planned piece and a shard_topk_stream after every planned fold, then the closing fold and the all-gather -- with a small CAP (short
    windows: three planned folds) and a CHUNK that ends inside windows."""
    from fusion_amd.distributed import ShardedSparseIndex
    idx, _, _, ql, full, _ = big
    k = 100
    shard = ShardedSparseIndex(idx, BASE)
    shard.CAP, shard.CHUNK = 256, 5 * S
    assert shard.head_docs(k) == 2 * S
    exp, folds, inside = planned_search_marks(ops, 2 * S, N_BIG, shard.CHUNK, k, shard.CAP, S, "shard_sparse", "shard_sparse_filter")
    assert folds >= 3 and inside >= 1 and exp[-3] == "shard_sparse_filter"      # ... and the shard ends mid-window
    marks = []
    g_sc, g_ids = shard.search(*ql, k=k, mark=marks.append)
    assert marks == exp
    e_sc, e_ids = ops.topk_rows(full, k, id_base=BASE)
    assert torch.equal(g_ids, e_ids) and torch.equal(g_sc, e_sc)


# ---- 4. every window overflows: the exact redo ------------------------------------------------------------------------------------
def test_overflowing_windows_are_redone_exactly(ops):
    from fusion_amd.distributed import ShardedSparseIndex
    N, Q, k = 120_000, 16, 1000

    def rising():
        for r0, X in splade_blocks(21, N, 30, dup=False):
            X[:, 0] = 1.0 + (r0 + torch.arange(X.shape[0], device="cuda", dtype=torch.float32)) * 2e-5   # rises with the document id
            yield r0, X
    idx = ops.sparse_index_from_blocks(rising(), V, N=N)
    Qd = next(splade_blocks(22, Q, 5, block=Q, dup=False))[1]
    Qd *= 1e-3
    Qd[:, 0] = 1.0
    ql = ops.sparse_rows(Qd, V)
    e_sc, e_ids = ops.topk_rows(ops.sparse_dot(idx, *ql), k, id_base=BASE)
    shard = ShardedSparseIndex(idx, BASE)
    g_sc, g_ids = shard.local_topk(*ql, k)
    assert shard.last_overflow > 0
    assert torch.equal(g_ids, e_ids) and torch.equal(g_sc, e_sc)


# ---- 4b. the filter epilogue at the capacity boundary ------------------------------------------------------------------------------
def test_filter_epilogue_at_exactly_cap_and_one_past_it(ops):
    """One full slice and a ragged tail, three one-term queries whose scores are exact by construction (0.25 / 0.5 / 0.75 times 1.0):
    query 0 ties tau everywhere (no survivor: the rule is !(score <= tau)), query 1 has exactly cap survivors, query 2 cap + 1 over both
    slices.  With query 2 switched off (tau = inf) every slot of query 1 is written and the flag stays 0; with it on, the flag is 1, the
    count runs to cap + 1, and nothing lands at or past cap (a guard row behind the buffers)."""
    import types
    N, Q, cap = S + 37, 3, 64
    D = np.zeros((N, 4), dtype=np.float32)
    D[:, 0] = 0.5
    rng = np.random.default_rng(5)
    hit1 = np.sort(np.concatenate([rng.choice(S, 44, replace=False), S + rng.choice(37, 20, replace=False)]))
    hit2 = np.sort(np.concatenate([rng.choice(S, 40, replace=False), S + rng.choice(37, 25, replace=False)]))
    D[hit1, 1] = 0.75
    D[:, 2] = 0.25
    D[hit2, 2] = 0.75
    Qd = np.eye(3, 4, dtype=np.float32)
    ref = Qd @ D.T                                                       # one exact product per entry
    tau_h = np.full(3, 0.5, dtype=np.float32)
    keep = [np.flatnonzero(~(ref[q] <= tau_h[q])) for q in range(Q)]
    assert [len(x) for x in keep] == [0, cap, cap + 1] and keep[2][0] < S <= keep[2][-1] and keep[1][0] < S <= keep[1][-1]
    idx = ops.sparse_index(torch.from_numpy(D).cuda())
    ql = ops.sparse_rows(torch.from_numpy(Qd).cuda())
    assert torch.equal(ops.sparse_dot(idx, *ql).cpu(), torch.from_numpy(ref))
    src = ops._sparse_source(idx, *ql, BASE)

    def run(tau):
        cs = torch.full((Q + 1, cap), -7.0, dtype=torch.float32, device="cuda")        # row Q: the guard
        ci = torch.full((Q + 1, cap), -99, dtype=torch.int64, device="cuda")
        st = types.SimpleNamespace(rows=Q, cap=cap, tau=torch.from_numpy(tau).cuda(), cand_s=cs[:Q], cand_i=ci[:Q],
                                   cand_len=torch.zeros(Q, dtype=torch.int32, device="cuda"), overflow=torch.zeros(1, dtype=torch.int32, device="cuda"))
        src.filter(st, 0, N)
        torch.cuda.synchronize()
        return cs.cpu().numpy(), ci.cpu().numpy(), st.cand_len.cpu().numpy(), int(st.overflow.item())

    cs, ci, cl, ov = run(np.array([0.5, 0.5, np.inf], dtype=np.float32))
    assert ov == 0 and cl.tolist() == [0, cap, 0]
    assert np.array_equal(np.sort(ci[1]), keep[1] + BASE) and (cs[1] == 0.75).all()           # every slot written
    assert (cs[[0, 2, 3]] == -7.0).all() and (ci[[0, 2, 3]] == -99).all()
    cs, ci, cl, ov = run(tau_h)
    assert ov == 1 and cl.tolist() == [0, cap, cap + 1]
    assert np.array_equal(np.sort(ci[1]), keep[1] + BASE) and (cs[1] == 0.75).all()
    d = ci[2] - BASE
    assert len(set(d.tolist())) == cap and set(d.tolist()) <= set(keep[2].tolist())            # cap distinct survivors ...
    assert np.array_equal(cs[2].view(np.int32), ref[2, d].view(np.int32))                      # ... each with its own score
    assert (cs[[0, 3]] == -7.0).all() and (ci[[0, 3]] == -99).all()                            # nothing for query 0, nothing past cap


# ---- 5. shards ---------------------------------------------------------------------------------------------------------------------
def sub_index(ops, idx, a, b):
    """The documents [a, b) of an index as an index of their own (documents renumbered from 0)."""
    term = torch.repeat_interleave(torch.arange(idx.V, device="cuda"), idx.toff[1:] - idx.toff[:-1])
    keep = (idx.pdoc >= a) & (idx.pdoc < b)
    toff = torch.zeros(idx.V + 1, dtype=torch.int64, device="cuda")
    toff[1:] = torch.cumsum(torch.bincount(term[keep], minlength=idx.V), 0)
    return ops.SparseIndex(toff, (idx.pdoc[keep] - a).contiguous(), idx.pw[keep].contiguous(), b - a, idx.V)


def test_shards_merge_to_the_whole_index(ops, big):
    from fusion_amd.distributed import ShardedSparseIndex, shard_bounds
    idx, _, _, ql, _, _ = big
    k = 1000
    whole_s, whole_i = ShardedSparseIndex(idx, BASE).search(*ql, k=k)
    parts_s, parts_i = [], []
    for r in range(8):
        a, b = shard_bounds(N_BIG, 8, r)
        s, i = ShardedSparseIndex(sub_index(ops, idx, a, b), BASE + a).local_topk(*ql, k)
        parts_s.append(s); parts_i.append(i)
    m_s, m_i = ops.topk_merge(torch.stack(parts_s), torch.stack(parts_i))
    assert torch.equal(m_i, whole_i) and torch.equal(m_s, whole_s)


# ---- 6. public surface -------------------------------------------------------------------------------------------------------------
def test_index_from_blocks_equals_index_of_the_dense_rows(ops):
    Dn = ops.normalize_rows(next(splade_blocks(31, 3000, 150, block=3000))[1])
    ref = ops.sparse_index(Dn, V)
    for rows in (1, 1000, 4096):
        got = ops.sparse_index_from_blocks(((r0, Dn[r0: r0 + rows]) for r0 in range(0, 3000, rows)), V)
        assert got.N == ref.N == 3000 and got.V == ref.V
        for a, b in zip((got.toff, got.pdoc, got.pw, got.slice_off), (ref.toff, ref.pdoc, ref.pw, ref.slice_off)):
            assert a.dtype == b.dtype and torch.equal(a, b), rows


def synthetic_texts(rng, n, lo, hi):
    words = [f"w{i}" for i in range(3000)]
    p = 1.0 / np.arange(1, 3001); p /= p.sum()
    return [" ".join(rng.choice(words, size=int(rng.integers(lo, hi)), p=p)) for _ in range(n)]


@pytest.mark.parametrize("sim", ["cos_sim", "dot_score"])
def test_encoder_search_equals_the_dense_reference(ops, sim):
    from fusion_amd import encoders
    enc = encoders.random_init("splade", size="tiny").calibrate_sparsity(per_token=0.01)
    enc.similarity = sim
    rng = np.random.default_rng(5)
    docs, queries = synthetic_texts(rng, 400, 10, 60), synthetic_texts(rng, 24, 3, 10)
    Qe = enc.encode(queries, batch_size=32, query_mode=True)
    De = enc.encode(docs, batch_size=32, query_mode=False)
    assert 0.001 < ops.density(De) < 0.95                              # sparse rows, not empty ones
    S_ref = ops.cos_scores(Qe, De) if sim == "cos_sim" else ops.dot_scores(ops.pad_dim(Qe), ops.pad_dim(De))
    tol = COS_TOL if sim == "cos_sim" else COS_TOL * float(S_ref.abs().max())
    for topk in (10, 100, 400, 1000):
        e_sc, e_ids = (t.cpu().numpy() for t in ops.topk_rows(S_ref, min(topk, len(docs))))
        res = enc.search(queries, docs, batch_size=32, topk=topk)
        assert len(res) == len(queries)
        for q, r in enumerate(res):
            assert len(r) == min(topk, len(docs))
            assert_ranked_close([x["doc_id"] for x in r], [x["score"] for x in r], e_ids[q], e_sc[q], tol, truncated=topk < len(docs))
    idx = enc.index(docs, batch_size=64)
    assert idx.N == len(docs) and idx.V == enc.dim


def test_chunk_sizes_do_not_change_the_result(ops, big):
    from fusion_amd import encoders
    idx, _, Qd, _, _, _ = big
    enc = encoders.random_init("splade", size="tiny")
    enc.similarity = "dot_score"
    Qe = Qd[:40]
    ref = enc.search_index(Qe, idx, topk=100)
    assert len(ref) == 40 and all(len(r) == 100 for r in ref)
    for qc, dc in ((100, 7000), (7, 7168), (1, 500000), (40, 3 * S)):
        assert enc.search_index(Qe, idx, query_chunk_size=qc, doc_chunk_size=dc, topk=100) == ref, (qc, dc)
