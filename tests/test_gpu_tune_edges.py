"""GPU tests of the weight-sweep rank kernel (csrc/tune.hip: gold_ranks_kernel<S, WIDE> behind ops.gold_ranks, fz_gold_ranks_f32 and
fz_gold_ranks_f64w) at every column-chunk, weight-chunk, gold-slot, sign, non-finite and tie edge of tests/tune_cases.py, against the
NumPy reference there (the operation itself: IEEE float32 / float64 products and sums, plain comparisons).  Every rank comparison
is an equality on the whole [W, Q, 8] tensor; the four end-to-end tests at the bottom hold the sweep's callers to the per-vector
fusion routes within the suite's 1e-12 metric bar.  The conditions the cases rely on are asserted in tests/test_tune_cases_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import tune_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    assert int(o._lib.lib().fz_tune_max_gold()) == tc.G
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def poisoned_plane(ops, a, poison):
    """a [Q, N] in an ops.alloc_plane plane of Q + 1 rows: the padding columns of every row and a whole sentinel row behind the
    last one hold `poison` (NaN scores, position 0: a column the kernel must never count)."""
    Q, N = a.shape
    p = ops.alloc_plane(Q + 1, N, torch.from_numpy(a[:0]).dtype, "cuda", fill=poison)
    p[:Q].copy_(torch.from_numpy(a))
    assert p.stride(0) == ops.round_up(N, 64) and p.stride(0) >= N
    return p[:Q]


def sweep(ops, c, layout="padded"):
    if layout == "padded":
        T, pos = [poisoned_plane(ops, t, float("nan")) for t in c.T], poisoned_plane(ops, c.pos, 0)
    else:                   # plain contiguous tensors: ld == N, rows at any alignment
        T, pos = [dev(t) for t in c.T], dev(c.pos)
        assert pos.stride(0) == c.N
    return ops.gold_ranks(T, pos, dev(c.weights_as_passed()), dev(c.gold))


def assert_ranks(got, c, what=""):
    exp = tc.reference(c.name)
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == exp.shape == (c.W, c.Q, tc.G)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        w, q, g = bad[0]
        raise AssertionError(f"{c.name} {what}: {len(bad)} of {exp.size} ranks differ; first at weight vector {w}, query {q}, slot {g} "
                             f"(gold column {c.gold[q, g]}): {got[w, q, g]} != {exp[w, q, g]}; weight vectors hit: {np.unique(bad[:, 0])[:12]}")


# ---- every case of the table, both sweeps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.NAMES)
def test_gold_ranks_equal_the_reference(name, ops):
    """Planes with ld > N (ld == N where N is a multiple of 64), padding and the row behind the last one poisoned."""
    c = tc.case(name)
    assert_ranks(sweep(ops, c), c)


@pytest.mark.parametrize("name", ["cols-N65-narrow", "cols-N65-wide", "cols-N4097-narrow", "cols-N4097-wide", "nonfinite-S2-narrow", "nonfinite-S2-wide",
                                  "weights-W513-wide"])
def test_gold_ranks_with_unpadded_rows(name, ops):
    """ld == N: harmonise takes plain contiguous tensors as they are."""
    c = tc.case(name)
    assert_ranks(sweep(ops, c, layout="contiguous"), c, "ld == N")


@pytest.mark.parametrize("name", ["slots-A-narrow", "slots-B-wide", "weights-W513-narrow", "systems-S4-wide"])
def test_gold_ranks_with_strided_weights_and_gold(name, ops):
    """weights and gold as row-strided views of larger tensors whose other entries would change every rank."""
    c = tc.case(name)
    wbig = torch.full((2 * c.W, c.S), 0.71875, dtype=torch.float64 if c.wide else torch.float32, device="cuda")
    wbig[::2] = dev(c.weights_as_passed())
    gbig = torch.zeros((c.Q, 2 * tc.G), dtype=torch.int32, device="cuda")
    gbig[:, :tc.G] = dev(c.gold)
    w, g = wbig[::2], gbig[:, :tc.G]
    assert not w.is_contiguous() and not g.is_contiguous()
    T, pos = [poisoned_plane(ops, t, float("nan")) for t in c.T], poisoned_plane(ops, c.pos, 0)
    assert_ranks(ops.gold_ranks(T, pos, w, g), c, "strided views")


def test_mixed_row_strides_are_harmonised(ops):
    c = tc.case("cols-N4097-wide")
    T = [poisoned_plane(ops, c.T[0], float("nan")), dev(c.T[1])]          # ld = 4,160 and ld = 4,097 in one call
    assert_ranks(ops.gold_ranks(T, dev(c.pos), dev(c.weights_as_passed()), dev(c.gold)), c, "mixed strides")


@pytest.mark.parametrize("name", ["weights-W513-narrow", "weights-W513-wide", "cols-N8193-wide"])
def test_raw_c_abi_writes_nothing_outside_its_output(name, ops):
    """fz_gold_ranks_* as a non-Python host calls it, `out` inside a larger buffer of sentinels: [W, Q, 8] equals the reference and
    not a word before or behind it changes."""
    from fusion_amd import _lib
    L = _lib.lib()
    c = tc.case(name)
    T, pos = [poisoned_plane(ops, t, float("nan")) for t in c.T], poisoned_plane(ops, c.pos, 0)
    ld, n, guard, SENT = pos.stride(0), c.W * c.Q * tc.G, 4096, 0x5A5A5A5A
    buf = torch.full((guard + n + guard,), SENT, dtype=torch.int32, device="cuda")
    buf[guard:guard + n] = 0
    w, g = dev(c.weights_as_passed()), dev(c.gold)
    P = lambda t: C.c_void_p(t.data_ptr())
    fn = L.fz_gold_ranks_f64w if c.wide else L.fz_gold_ranks_f32
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn((C.c_void_p * c.S)(*[t.data_ptr() for t in T]), P(pos), P(w), P(g), c.S, c.W, c.Q, c.N, ld, C.c_void_p(buf.data_ptr() + 4 * guard), st) == 0
    torch.cuda.synchronize()
    assert_ranks(buf[guard:guard + n].reshape(c.W, c.Q, tc.G), c, "C ABI")
    assert bool((buf[:guard] == SENT).all()) and bool((buf[guard + n:] == SENT).all())


def test_other_wrappers_hold_their_contiguous_copies_too(ops):
    """The defect the strided-views test above found in ops.gold_ranks (two `.contiguous()` copies made inside one argument list: the
    second took the block the first had just released) had two siblings: ops.tune_metrics and ops.topk_update with two strided
    arguments must give the bytes of the contiguous call."""
    from fusion_amd.utils.metrics import MAP_KS, MRR_KS, NDCG_KS, RECALL_KS, gold_rank_tables
    c = tc.case("slots-B-narrow")
    cuts = dict(recall=RECALL_KS, map=MAP_KS, mrr=MRR_KS, ndcg=NDCG_KS)
    n_gold = np.array([1, 2, 5])
    table, idcg, _ = gold_rank_tables(n_gold)
    ranks, gold, pos = dev(tc.reference(c.name).copy()), dev(c.gold), poisoned_plane(ops, c.pos, 0)
    rest = (pos, dev(n_gold.astype(np.int32)), dev(idcg), dev(table), cuts)
    rbig = torch.full((c.W, 2 * c.Q, tc.G), 7, dtype=torch.int32, device="cuda")
    gbig = torch.full((c.Q, 2 * tc.G), 3, dtype=torch.int32, device="cuda")
    rbig[:, ::2], gbig[:, :tc.G] = ranks, gold
    assert not rbig[:, ::2].is_contiguous() and not gbig[:, :tc.G].is_contiguous()
    assert torch.equal(ops.tune_metrics(rbig[:, ::2], gbig[:, :tc.G], *rest), ops.tune_metrics(ranks, gold, *rest))
    rng = np.random.default_rng(5)
    rows, k, n = 3, 8, 300
    first, second = dev(rng.normal(0, 1, (rows, n)).astype(np.float32)), dev(rng.normal(0, 1, (rows, n)).astype(np.float32))
    rs, ri = ops.topk_rows(first, k)
    sbig, ibig = torch.zeros((rows, 2 * k), device="cuda"), torch.zeros((rows, 2 * k), dtype=torch.int64, device="cuda")
    sbig[:, :k], ibig[:, :k] = rs, ri
    a = ops.topk_update(second, n, sbig[:, :k], ibig[:, :k])
    b = ops.topk_update(second, n, rs, ri)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[2]) == int(b[2]) == 0


# ---- argument edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=tc.SWEEPS)
def test_no_weight_vector_gives_an_empty_result(wide, ops):
    c = tc.case(f"cols-N257-{tc.SWEEPS[wide]}")
    w = torch.empty((0, c.S), dtype=torch.float64 if wide else torch.float32, device="cuda")
    out = ops.gold_ranks([dev(t) for t in c.T], dev(c.pos), w, dev(c.gold))
    assert out.shape == (0, c.Q, tc.G) and out.dtype == torch.int32


@pytest.mark.parametrize("wide", [False, True], ids=tc.SWEEPS)
def test_five_systems_are_refused(wide, ops):
    """The sweep is instantiated for 1 - 4 systems: a fifth is FZ_ERR_UNSUPPORTED, never ranks."""
    from fusion_amd._lib import FZ_ERR_UNSUPPORTED, FusionHipError
    c = tc.case(f"systems-S4-{tc.SWEEPS[wide]}")
    T = [dev(t) for t in c.T] + [dev(c.T[0])]
    w = torch.ones((3, 5), dtype=torch.float64 if wide else torch.float32, device="cuda")
    with pytest.raises(FusionHipError) as e:
        ops.gold_ranks(T, dev(c.pos), w, dev(c.gold))
    assert e.value.status == FZ_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", ["weights-W1025-narrow", "weights-W1025-wide", "cols-N8193-narrow", "cols-N8193-wide"])
def test_two_launches_give_the_same_ranks(name, ops):
    """The counts are integer atomics: no launch-to-launch difference, whatever order the workgroups arrive in."""
    c = tc.case(name)
    a, b = sweep(ops, c), sweep(ops, c)
    assert torch.equal(a, b)
    assert_ranks(b, c)


# ---- the integer claim itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=tc.SWEEPS)
def test_ranks_are_those_of_the_materialise_and_sort_path(wide, ops):
    """"Exactly the rank the materialise-and-sort path gives": per weight vector the fused plane from ops.fuse_wsum (narrow flags as
    the sweep's width) sorted by ops.sort_rows_desc in first-insertion order; its rank plane at the gold columns == the sweep's
    ranks.  N = 4,097, a third of the columns in no list."""
    c = tc.case(f"claim-{tc.SWEEPS[wide]}")
    T, pos = [poisoned_plane(ops, t, float("nan")) for t in c.T], poisoned_plane(ops, c.pos, 0)
    got = ops.gold_ranks(T, pos, dev(c.weights_as_passed()), dev(c.gold))
    assert_ranks(got, c)
    ins = np.full((c.Q, c.N), -1, dtype=np.int32)
    U = (c.pos >= 0).sum(axis=1).astype(np.int32)
    for q in range(c.Q):
        listed = np.flatnonzero(c.pos[q] >= 0)
        ins[q, c.pos[q, listed]] = listed
    ok, _, _ = tc.listed_golds(c.pos, c.gold)
    assert 0.3 < (c.pos < 0).mean() < 0.37 and not ok.all() and (c.gold >= 0).all() and (c.gold < c.N).all()
    for wi, w in enumerate(c.weights):
        fused = ops.fuse_wsum(T, None, [float(x) for x in w], narrow=[not wide] * c.S)
        _, _, rank = ops.sort_rows_desc(fused, init_order=dev(ins), row_len=dev(U), want_order=False, want_keys=False, want_rank=True)
        at_gold = torch.gather(rank, 1, dev(c.gold.astype(np.int64))).cpu().numpy()
        assert np.array_equal(np.where(ok, at_gold, 0), got[wi].cpu().numpy()), (wide, wi)
        assert (at_gold[~ok] == -1).all()                          # a gold in no list is not in the sorted sequence at all


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
ROWS = [0, 1, 511, 512, 513, 1023, 1024, 1535, 1536, 1770]


def assert_same_metrics(got, exp, what):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert list(g) == list(e), (what, i)
        worst = max(abs(float(g[k]) - float(e[k])) for k in e)
        assert worst <= 1e-12, (what, i, worst)


@pytest.fixture(scope="module")
def dense_systems(ops):
    """S = 4 ranked lists over 4,100 documents, Q = 3: one system lists 3,000 documents, one document of query 1 is in no list,
    scores rounded so that ties are frequent; golds: listed ones, the unlisted one, one id outside the corpus."""
    from fusion_amd.retrievers.hybrid import Aggregator
    rng = np.random.default_rng(77)
    Q, N, names = 3, 4100, ["bm25", "dpr", "splade", "colbert"]
    ids = np.arange(N) + 70_000
    lists = {}
    for s, n in enumerate(names):
        per_query = []
        for q in range(Q):
            keep = rng.permutation(N)[: 3000 if s == 2 else N]
            if q == 1:
                keep = keep[keep != 4099]
            sc = np.round(rng.normal(0.0, 1.0, len(keep)) * (1 + s), 1 if s == 1 else 2)
            order = np.argsort(-sc, kind="stable")
            per_query.append([{"corpus_id": int(ids[keep[j]]), "score": float(sc[j])} for j in order])
        lists[n] = per_query
    labels = [[int(ids[j]) for j in rng.choice(N - 1, size=4, replace=False)] for _ in range(Q)]
    labels[1] += [int(ids[4099])]                 # in the corpus, in no list of query 1
    labels[2] += [999_999_999]                    # not in the corpus
    systems = Aggregator._to_device(lists)
    assert systems["bm25"].N == N and not systems["splade"].full
    return names, systems, labels


@pytest.mark.parametrize("kind", [np.float64, float], ids=["np_float64_wide", "python_floats_narrow"])
@pytest.mark.parametrize("norm", ["min-max", "z-score"])
def test_tune_over_the_whole_lattice_equals_fusing_per_vector(norm, kind, dense_systems, ops):
    """Aggregator.tune on the full 1,771-vector grid (four passes over the LDS counters, two / three workgroups per row) against
    Aggregator._tune_by_fusing on the vectors at the pass borders alone."""
    from fusion_amd.retrievers.hybrid import Aggregator, weight_grid
    names, systems, labels = dense_systems
    grid = [{n: kind(x) for n, x in w.items()} for w in weight_grid(names)]
    assert len(grid) == 1771 and all(type(x) is kind for x in grid[0].values())
    got = Aggregator.tune(systems, norm, grid, labels, {})
    assert len(got) == len(grid)
    exp = Aggregator._tune_by_fusing(systems, norm, [grid[i] for i in ROWS], labels, {})
    assert_same_metrics([got[i] for i in ROWS], exp, (norm, kind.__name__))
    assert len({tuple(g.values()) for g in got}) > 50              # the rows are not copies of each other


@pytest.mark.parametrize("kind", [np.float64, float], ids=["np_float64_wide", "python_floats_narrow"])
def test_tune_topk_over_a_union_wider_than_one_chunk(kind, ops):
    """Four mostly disjoint lists of 1,100: every query's union is 4,100 columns, more than one workgroup's 4,096 / 2,048."""
    from fusion_amd.retrievers.hybrid import Aggregator, weight_grid
    from test_gpu_lists_tune import per_vector, systems_of
    rng = np.random.default_rng(78)
    S, Q, K = 4, 3, 1100
    names = [f"s{s}" for s in range(S)]
    ids = np.stack([np.stack([(5 << 33) + 1000 * s + rng.permutation(K) for _ in range(Q)]) for s in range(S)])      # [S, Q, K]; neighbours share 100 ids
    sc = -np.sort(-np.round(rng.normal(0.0, 1.0, (S, Q, K)), 2), axis=2)
    lens = np.full((S, Q), K, dtype=np.int32)
    lens[2, 1] = 900
    systems = systems_of(names, ids, sc, lens)
    _, _, _, out_len, _ = ops.lists_columns([systems[n].ids for n in names], [systems[n].lens for n in names], None)
    assert int(out_len[0]) == 4100 > tc.COLS_F32 and int(out_len.min()) > tc.COLS_F64
    labels = [[int(ids[s, q, r]) for s, r in ((0, 3), (1, 1050), (3, 1099), (2, 950))] + [(1 << 50) + q] for q in range(Q)]
    grid = [{n: kind(x) for n, x in w.items()} for w in weight_grid(names)[5::340]]
    assert len(grid) == 6
    got = Aggregator.tune_topk(systems, "min-max", grid, labels, {})
    assert_same_metrics(got, per_vector(systems, "min-max", grid, labels, {}), ("tune_topk", kind.__name__))


def test_twelve_golds_at_two_chunks_take_the_chunked_host_path(dense_systems, ops):
    """More than eight golds per query (two counting launches, host evaluation) at N = 4,100: the metrics are those of the reference's
    ranks over the very planes the sweep reads, through metrics_from_gold_ranks."""
    from fusion_amd.retrievers.hybrid import Aggregator, weight_grid
    from fusion_amd.utils.metrics import metrics_from_gold_ranks
    names, systems, _ = dense_systems
    rng = np.random.default_rng(79)
    S = [systems[n] for n in names]
    Q, N = S[0].Q, S[0].N
    ids = [int(x) for x in S[0].ids]
    nowhere = ids.index(70_000 + 4099)                      # in no list of query 1
    gold_pos = [rng.choice(np.delete(np.arange(N), nowhere), size=12, replace=False).tolist() for _ in range(Q)]
    gold_pos[1][5] = nowhere
    labels = [[ids[j] for j in gl] for gl in gold_pos]
    grid = weight_grid(names)[7::177]
    got = Aggregator.tune(systems, "min-max", grid, labels, {})
    T = Aggregator._normalised_planes(S, "min-max", None, [s.stats("min-max") for s in S], zero_unlisted=True)
    _, _, pos = ops.insertion_order([s.order for s in S], torch.stack([s.lens for s in S]).contiguous(), N, want_pos=True)
    pos_h = pos.cpu().numpy()
    W = np.array([[w[n] for n in names] for w in grid])
    ranks = np.concatenate([tc.gold_ranks_ref([t.cpu().numpy() for t in T], pos_h, W, tc.pad_gold([gl[g0:g0 + tc.G] for gl in gold_pos]), wide=True)[:, :, : 12 - g0]
                            for g0 in (0, tc.G)], axis=2).astype(np.int64)
    listed = np.take_along_axis(pos_h, np.array(gold_pos), axis=1) >= 0
    assert not listed.all() and listed.sum() == 3 * 12 - 1
    ranks = np.where(listed[None], ranks, np.iinfo(np.int64).max)
    exp = metrics_from_gold_ranks(ranks, np.full(Q, 12), (pos_h >= 0).sum(axis=1))
    assert_same_metrics(got, exp, "twelve golds")
