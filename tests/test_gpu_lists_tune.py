"""GPU tests of the weight sweep over top-k lists (csrc/lists_tune.hip -> ops.lists_columns -> Aggregator.tune_topk /
evaluate_topk): the reference's own loop on the topktune_*.npz fixtures, the parent's two routes as yardsticks (one fuse_topk +
run_evaluation per vector; Aggregator.tune on the dict lists), the kernel's outputs against ops.lists_join and NumPy at the wave,
chunk and capacity edges, the gold look-up, determinism and the duplicate flag.  Every metric comparison is within 1e-12: the means
are exactly rounded sums on both sides (statistics.mean against the device's double-double accumulation)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_lists_fusion import ID_BASE, dict_lists, random_lists, systems_of
from topk_tune_util import FIVE, TuneCase, defined_rows, metric_rows

pytestmark = pytest.mark.gpu

TUNE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "topktune_*.npz")))
ABSENT = (1 << 50) + 99          # an id no synthetic list holds


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from fusion_amd import ops as o
    return o


def per_vector(systems, norm, grid, labels, distr):
    """The parent's device route: one fusion + one host evaluation per weight vector."""
    from fusion_amd.retrievers.hybrid import Aggregator, run_evaluation
    return [run_evaluation(Aggregator.fuse_topk(systems, "nsf", norm, w, distr).predictions(1000), labels, print2console=False) for w in grid]


def assert_same_metrics(got, exp, what, rows=slice(None)):
    names = list(exp[0])
    G, E = metric_rows(got, names), np.array([[float(e[k]) for k in names] for e in exp])
    assert all(list(e) == names for e in exp) and G.shape == E.shape, what
    assert np.max(np.abs(G - E)[rows], initial=0.0) <= 1e-12, (what, float(np.max(np.abs(G - E)[rows], initial=0.0)))


# ---- 1. the reference's loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", FIVE)
@pytest.mark.parametrize("path", TUNE_FILES, ids=[os.path.basename(p)[:-4] for p in TUNE_FILES])
def test_tune_topk_matches_reference_loop(path, norm, oracle):
    """tune_topk == the reference's loop (deepcopy -> fuse -> run_evaluation per vector) on the list-form fixtures, every metric of
    every vector the reference defines (topk_tune_util.defined_rows) within 1e-12; where the reference raised (min-max on an empty
    list) the project's own rule holds instead: an empty list contributes nothing (oracle.tune_lists)."""
    from fusion_amd.retrievers.hybrid import Aggregator
    c = TuneCase(path)
    systems = systems_of(c.systems, c.ids, c.scores, c.lens)
    got = Aggregator.tune_topk(systems, norm, c.grid(), c.labels, c.distr)
    assert len(got) == len(c.weights)
    G = metric_rows(got, c.metric_names)
    if norm in c.raises:
        assert_same_metrics(got, oracle.tune_lists(c.lists(), norm, c.grid(), c.labels, c.distr), (path, norm, "oracle"))
        return
    rows = defined_rows(c, norm)
    assert np.max(np.abs(G - c.z[f"metrics__{norm}"])[rows], initial=0.0) <= 1e-12


# ---- 2. the parent's code as yardstick --------------------------------------------------------------------------------------------
def synthetic(S, seed, Q=6):
    """Seeded lists with ties inside and across systems (random_lists: 39 distinct score values), lists of different k, a short
    and an empty list, ids beyond 2^32; labels: listed by several systems, by the LAST system only, by none, repeated, and -1."""
    rng = np.random.default_rng(seed)
    widths = [40, 25, 33, 12, 40, 7, 25, 9][:S]
    lens = np.array([[w] * Q for w in widths], dtype=np.int32)
    lens[0, 1] = 17
    lens[S - 1, 2] = 0
    lens[0, 3] = 0
    names = [f"s{s}" for s in range(S)]
    ids, sc = random_lists(rng, lens, widths)
    labels = []
    for q in range(Q):
        sets = [ids[s, q, :lens[s, q]].tolist() for s in range(S)]
        earlier = set(i for l in sets[:-1] for i in l)
        last_only = [i for i in sets[-1] if i not in earlier]
        pool = [i for l in sets for i in l[:6]]
        gl = [int(pool[int(rng.integers(0, len(pool)))]) for _ in range(int(rng.integers(1, 4)))]
        if last_only:
            gl.append(int(last_only[0]))
        if q % 2:
            gl.append(ABSENT + q)
        labels.append(gl)
    labels[0].append(labels[0][0])          # a repeated label
    labels[1].append(-1)                    # the padding value as a label: in no list
    distr = {n: np.quantile(sc[s][sc[s] > 0], np.linspace(0, 1, 41)) for s, n in enumerate(names)}
    return names, ids, sc, lens, widths, labels, distr


def lattice_sample(names, kind, count=9):
    import itertools
    step = 0.25
    grid = [c for c in itertools.product(np.arange(0, 1 + step, step), repeat=len(names)) if np.isclose(sum(c), 1.0)]
    pick = sorted(set(np.linspace(0, len(grid) - 1, count).round().astype(int).tolist()))
    return [{n: kind(x) for n, x in zip(names, grid[i])} for i in pick]


@pytest.mark.parametrize("kind", [float, np.float64], ids=["python_floats", "np_float64"])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_tune_topk_equals_the_parents_routes(S, kind, ops):
    from fusion_amd.retrievers.hybrid import Aggregator
    names, ids, sc, lens, widths, labels, distr = synthetic(S, 100 + S)
    systems = systems_of(names, ids, sc, lens, widths)
    lists = {n: t.to_lists() for n, t in systems.items()}
    grid = lattice_sample(names, kind)
    assert any(0.0 in w.values() for w in grid) and all(type(x) is kind for w in grid for x in w.values())
    for norm in FIVE:
        got = Aggregator.tune_topk(systems, norm, grid, labels, distr)
        assert_same_metrics(got, per_vector(systems, norm, grid, labels, distr), (S, kind, norm, "per-vector fuse_topk"))
        assert_same_metrics(got, Aggregator.tune(lists, norm, grid, labels, distr), (S, kind, norm, "Aggregator.tune on to_lists()"))


@pytest.mark.parametrize("what", ["S5", "S8", "none", "mixed"])
def test_tune_topk_generic_path(what, ops):
    """More than 4 systems, 'none', and a grid that mixes Python-float and np.float64 weights: one fuse_topk + run_evaluation per vector."""
    from fusion_amd.retrievers.hybrid import Aggregator
    S = {"S5": 5, "S8": 8}.get(what, 3)
    names, ids, sc, lens, widths, labels, distr = synthetic(S, 200 + S)
    systems = systems_of(names, ids, sc, lens, widths)
    lists = {n: t.to_lists() for n, t in systems.items()}
    norm = "none" if what == "none" else "min-max"
    grid = lattice_sample(names, np.float64, count=4)
    if what == "mixed":
        grid = [{n: (float(x) if i % 2 else x) for i, (n, x) in enumerate(w.items())} for w in grid]
        assert len({type(x) for w in grid for x in w.values()}) == 2
    got = Aggregator.tune_topk(systems, norm, grid, labels, distr)
    assert_same_metrics(got, per_vector(systems, norm, grid, labels, distr), (what, "per-vector fuse_topk"))
    assert_same_metrics(got, Aggregator.tune(lists, norm, grid, labels, distr), (what, "Aggregator.tune on to_lists()"))


def test_twelve_golds_take_the_chunked_path(ops):
    from fusion_amd.retrievers.hybrid import Aggregator
    names, ids, sc, lens, widths, labels, distr = synthetic(3, 300)
    assert ops._lib.lib().fz_tune_max_gold() == 8
    labels[4] = [int(x) for x in ids[0, 4, :5]] + [int(x) for x in ids[2, 4, 3:9]] + [ABSENT]      # twelve, some listed twice, one absent
    assert len(dict.fromkeys(labels[4])) == 12
    systems = systems_of(names, ids, sc, lens, widths)
    for kind in (float, np.float64):
        grid = lattice_sample(names, kind, count=5)
        for norm in ("min-max", "percentile-rank"):
            got = Aggregator.tune_topk(systems, norm, grid, labels, distr)
            assert_same_metrics(got, per_vector(systems, norm, grid, labels, distr), (kind, norm, "twelve golds"))


# ---- 3. the kernel against ops.lists_join and NumPy ---------------------------------------------------------------------------------
def full_rows(t):
    """A plane [Q, n] -> its whole rows [Q, ld], padding columns included (the kernel defines them all)."""
    Q = t.shape[0]
    ld = t.stride(0) if Q > 1 else max(-(-t.shape[1] // 64) * 64, 64)
    return torch.as_strided(t, (Q, ld), (ld, 1))


def check_columns(ops, lens_sq, widths, relation="overlap", id_of=None, seed=0, strided=False):
    rng = np.random.default_rng(seed)
    lens_sq = np.asarray(lens_sq, dtype=np.int32)
    S, Q = lens_sq.shape
    ids, _ = random_lists(rng, lens_sq, widths, relation, id_of)
    L = ids.shape[2]
    vals = rng.standard_normal((S, Q, L)).astype(np.float32)
    vals[:, :, ::7] = -0.0
    vals[:, :, 1::11] = -np.inf
    pad = [3 + 5 * s if strided else 0 for s in range(S)]
    d_ids, d_vals, d_lens = [], [], []
    for s in range(S):
        wi = torch.full((Q, widths[s] + pad[s]), -1, dtype=torch.int64, device="cuda")
        wv = torch.full((Q, widths[s] + pad[s]), float("nan"), dtype=torch.float32, device="cuda")
        wi[:, :widths[s]] = torch.from_numpy(ids[s][:, :widths[s]]).cuda()
        wv[:, :widths[s]] = torch.from_numpy(vals[s][:, :widths[s]]).cuda()
        d_ids.append(wi[:, :widths[s]]); d_vals.append(wv[:, :widths[s]])
        d_lens.append(torch.from_numpy(lens_sq[s]).cuda())
    # gold ids: the first and the last entry of every list, an absent id, padding, a negative id, the first entry once more
    G = 2 * S + 4
    gold = np.full((Q, G), -1, dtype=np.int64)
    for q in range(Q):
        for s in range(S):
            if lens_sq[s, q]:
                gold[q, 2 * s] = ids[s, q, 0]
                gold[q, 2 * s + 1] = ids[s, q, lens_sq[s, q] - 1]
        gold[q, 2 * S] = ABSENT
        gold[q, 2 * S + 2] = -7
        gold[q, 2 * S + 3] = gold[q, 0]
    d_gold = torch.from_numpy(gold).cuda()
    out_ids, T, pos, out_len, gold_col = ops.lists_columns(d_ids, d_lens, d_vals, d_gold)
    j_ids, _, j_len = ops.lists_join(d_ids, d_lens, "rrf")
    total = int(sum(widths))
    assert out_ids.shape == (Q, total) and pos.shape == (Q, total) and all(t.shape == (Q, total) for t in T) and gold_col.shape == (Q, G)
    assert len({full_rows(t).shape[1] for t in [out_ids, pos] + T}) == 1
    assert torch.equal(out_len, j_len) and torch.equal(full_rows(out_ids), full_rows(j_ids))        # the join's bytes (over its -1 fill)
    h_ids, h_len = full_rows(out_ids).cpu().numpy(), out_len.cpu().numpy()
    ld = h_ids.shape[1]
    assert h_len.tolist() == [len(set(ids[:, q][ids[:, q] >= 0].tolist())) for q in range(Q)]
    col_of = [{int(i): c for c, i in enumerate(h_ids[q, :h_len[q]])} for q in range(Q)]
    e_pos = np.where(np.arange(ld)[None, :] < h_len[:, None], np.arange(ld, dtype=np.int32)[None, :], np.int32(-1))
    np.testing.assert_array_equal(full_rows(pos).cpu().numpy(), e_pos)
    for s in range(S):
        e = np.zeros((Q, ld), dtype=np.float32)
        for q in range(Q):
            for r in range(lens_sq[s, q]):
                e[q, col_of[q][int(ids[s, q, r])]] = vals[s, q, r]
        np.testing.assert_array_equal(full_rows(T[s]).cpu().numpy().view(np.int32), e.view(np.int32), err_msg=f"T[{s}]")   # bits: +0.0, not -0.0
    e_gold = np.array([[col_of[q].get(int(g), -1) if g >= 0 else -1 for g in gold[q]] for q in range(Q)], dtype=np.int32).reshape(Q, G)
    np.testing.assert_array_equal(gold_col.cpu().numpy(), e_gold)
    # two runs: identical bytes in every output
    again = ops.lists_columns(d_ids, d_lens, d_vals, d_gold)
    for a, b in zip([out_ids, pos] + T, [again[0], again[2]] + again[1]):
        assert torch.equal(full_rows(a).view(torch.int32 if a.dtype != torch.int64 else torch.int64),
                           full_rows(b).view(torch.int32 if b.dtype != torch.int64 else torch.int64))
    assert torch.equal(out_len, again[3]) and torch.equal(gold_col, again[4])
    # the ids-only join: same ids, positions and gold columns, no plane
    o2, T2, p2, l2, g2 = ops.lists_columns(d_ids, d_lens, None, d_gold)
    assert T2 is None and torch.equal(full_rows(o2), full_rows(out_ids)) and torch.equal(full_rows(p2), full_rows(pos))
    assert torch.equal(l2, out_len) and torch.equal(g2, gold_col)


@pytest.mark.parametrize("total", [1, 63, 64, 65, 1024, 1025, 2049])
def test_columns_total_entries_at_wave_and_chunk_edges(total, ops):
    a = (total + 1) // 2
    check_columns(ops, [[a, total], [total - a, 0]], [max(a, total), max(total - a, 1)], seed=total)


def test_columns_at_the_capacity(ops):
    cap = ops.lists_max_entries()
    k = cap // 8
    assert cap == 8 * 1024
    check_columns(ops, [[k, k - 1]] + [[k, k]] * 7, [k] * 8, relation="disjoint", seed=1)      # union = S x k: every column in use
    check_columns(ops, [[k, k]] * 8, [k] * 8, relation="same", seed=2)                          # all list the same ids: union = k
    check_columns(ops, [[cap, cap - 1]], [cap], seed=4)                                         # S = 1: chunks of one list
    over = [torch.zeros((2, k + (s == 3)), dtype=torch.int64, device="cuda") for s in range(8)]
    with pytest.raises(ValueError, match=str(cap + 1)):
        ops.lists_columns(over, [torch.zeros(2, dtype=torch.int32, device="cuda")] * 8)


def test_columns_lists_of_different_k_and_row_strides(ops):
    check_columns(ops, [[1000, 640, 1000], [10, 10, 3], [1, 1, 0]], [1000, 10, 1], seed=8, strided=True)
    check_columns(ops, [[1, 1], [1000, 999], [10, 2]], [1, 1000, 10], seed=9, strided=True)


def test_columns_empty_lists(ops):
    check_columns(ops, [[10, 1, 0, 7]], [10], seed=5)                                           # S = 1, one empty query
    check_columns(ops, [[10, 0, 0], [0, 10, 0], [5, 5, 0]], [10, 10, 10], seed=6)               # one system empty; every system empty
    check_columns(ops, [[0, 0], [0, 0]], [4, 4], seed=7)                                        # nothing listed at all


def test_columns_hash_adversarial_ids(ops):
    check_columns(ops, [[1000, 500], [1000, 1000], [1000, 7]], [1000] * 3, id_of=lambda j: 16384 * j, seed=10)         # multiples of the table size
    check_columns(ops, [[1000, 500], [1000, 1000], [1000, 7]], [1000] * 3, id_of=lambda j: (j << 32) | 5, seed=11)     # differ only above bit 32
    check_columns(ops, [[1000, 500], [1000, 1000]], [1000] * 2, id_of=lambda j: (1 << 62) - (j << 14), seed=12)        # id 1 << 62 among them
    check_columns(ops, [[64, 64], [64, 3]], [64] * 2, id_of=lambda j: j * 0x61C8864680B583EB % (1 << 63), seed=13)


def test_columns_wrong_dtypes_raise(ops):
    ids = torch.arange(6, dtype=torch.int64, device="cuda").reshape(2, 3)
    lens = torch.full((2,), 3, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        ops.lists_columns([ids.int()], [lens])
    with pytest.raises(TypeError):
        ops.lists_columns([ids], [lens.long()])
    with pytest.raises(TypeError):
        ops.lists_columns([ids], [lens], [ids.double()])
    with pytest.raises(TypeError):
        ops.lists_columns([ids], [lens], None, ids.int())
    with pytest.raises(ValueError):
        ops.lists_columns([ids], [lens], [ids.float()[:, :2]])


# ---- 4. duplicates, determinism of the sweep ------------------------------------------------------------------------------------------
def test_a_duplicated_id_raises(ops):
    from fusion_amd.planes import RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator

    def system(ids_row, k):
        ids = torch.full((2, k), -1, dtype=torch.int64, device="cuda")
        ids[0, :k] = torch.arange(k, device="cuda") + ID_BASE             # query 0: clean
        ids[1, :len(ids_row)] = torch.tensor(ids_row, dtype=torch.int64, device="cuda")
        return RankedTopk(ids=ids, scores=torch.zeros((2, k), device="cuda"),
                          lens=torch.tensor([k, len(ids_row)], dtype=torch.int32, device="cuda"))

    clean = system([5, 6, 7], 2000)
    labels = [[ID_BASE], [5]]
    grid = [{"a": 0.5, "b": 0.5}]
    assert len(Aggregator.tune_topk({"a": clean, "b": clean}, "arctan", grid, labels, {})) == 1
    far = list(range(100, 1600)); far[1400] = far[3]                       # the same id in two chunks of one list
    cases = {"in one chunk": {"a": system([5, 6, 5], 2000), "b": clean},
             "across chunks": {"a": system(far, 2000), "b": clean},
             "both already listed by an earlier system": {"a": clean, "b": system([9, 6, 8, 6], 2000)}}
    for what, systems in cases.items():
        S = list(systems.values())
        with pytest.raises(ValueError, match="same id twice"):
            ops.lists_columns([s.ids for s in S], [s.lens for s in S], [s.scores for s in S])
        with pytest.raises(ValueError, match="same id twice"):
            Aggregator.tune_topk(systems, "arctan", grid, labels, {})
    with pytest.raises(ValueError, match="same id twice"):
        Aggregator.evaluate_topk(system([5, 6, 5], 1000), labels)
    # padding slots are never read as ids: -1 twice past the lengths is no duplicate
    assert Aggregator.evaluate_topk(system([5], 1000), labels)["recall@5"] == 1.0


def test_tune_topk_is_deterministic(ops):
    from fusion_amd.retrievers.hybrid import Aggregator
    names, ids, sc, lens, widths, labels, distr = synthetic(4, 400)
    systems = systems_of(names, ids, sc, lens, widths)
    grid = lattice_sample(names, np.float64)
    for norm in ("min-max", "normal-curve-equivalent"):
        a = Aggregator.tune_topk(systems, norm, grid, labels, distr)
        b = Aggregator.tune_topk(systems, norm, grid, labels, distr)
        assert [list(x.items()) for x in a] == [list(x.items()) for x in b] or np.array_equal(
            metric_rows(a, list(a[0])), metric_rows(b, list(a[0])), equal_nan=True)


# ---- 5. evaluate_topk -----------------------------------------------------------------------------------------------------------------
def test_evaluate_topk_equals_run_evaluation(ops):
    from fusion_amd.planes import FusedTopk, RankedTopk
    from fusion_amd.retrievers.hybrid import Aggregator, run_evaluation
    rng = np.random.default_rng(500)
    Q, k = 5, 700
    lens = np.array([[k, 300, 0, 1, k], [k, k, 0, 0, 650], [k, 10, 0, 5, k]], dtype=np.int32)
    names = ["a", "b", "c"]
    ids, sc = random_lists(rng, lens, [k] * 3, relation="disjoint")
    systems = systems_of(names, ids, sc, lens, [k] * 3)
    fused = Aggregator.fuse_topk(systems, "rrf")                          # up to 2,100 entries per query: wider than the 1,000 evaluated
    assert isinstance(fused, FusedTopk) and fused.ids.shape[1] == 3 * k and int(fused.lens.max()) > 1000
    f_ids, f_len = fused.ids.cpu().numpy(), fused.lens.cpu().numpy()

    def labels_for(row_ids, row_len):
        out = []
        for q in range(Q):
            n = int(row_len[q])
            gl = [int(row_ids[q, j]) for j in (0, 4, 9, 99, 999, 1000, n - 1) if 0 <= j < n] + [ABSENT + q]
            out.append(gl)
        out[0] = out[0] + [out[0][0], -1]                                  # a repeated label and the padding value
        return out

    labels = labels_for(f_ids, f_len)
    assert any(int(g) in f_ids[q, 1000:f_len[q]].tolist() for q, gl in enumerate(labels) for g in gl)     # golds at positions >= 1000: never count
    got = Aggregator.evaluate_topk(fused, labels)
    exp = run_evaluation(fused.predictions(1000), labels, print2console=False)
    assert_same_metrics([got], [exp], "FusedTopk wider than 1000")
    rt = systems["a"]
    assert isinstance(rt, RankedTopk) and rt.lens.tolist() == [k, 300, 0, 1, k]                      # full, short and empty lists
    labels = labels_for(rt.ids.cpu().numpy(), rt.lens.cpu().numpy())
    fr = FusedTopk(ids=rt.ids, scores=rt.scores, lens=rt.lens)
    assert_same_metrics([Aggregator.evaluate_topk(rt, labels)], [run_evaluation(fr.predictions(1000), labels, print2console=False)], "RankedTopk")
    labels[4] = [int(x) for x in rt.ids[4, 5:17].tolist()]                                           # twelve golds: the host evaluation
    assert_same_metrics([Aggregator.evaluate_topk(rt, labels)], [run_evaluation(fr.predictions(1000), labels, print2console=False)], "twelve golds")
