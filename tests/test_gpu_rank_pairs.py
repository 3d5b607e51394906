"""distributed.rank_pairs, the one tail that turns (candidate ids, pair scores) into a planes.RankedTopk, pinned directly on a hand-written
[3, 6] plane -- the smallest one that holds everything the tail decides:

  row 0   a NaN (ranks first, as in every sort here), a tied pair whose ids DESCEND in the list (the two tie rules answer differently), one
          -inf slot in the middle of the row, under the id -1;
  row 1   -0.0 next to +0.0 (one key for the sort, two bit patterns for the gather), tied four ways;
  row 2   all -inf: nothing owned, ids with -1 among them.

Both tie rules against a NumPy restatement (np.lexsort for "id", a stable argsort for "list"), every k, row_len, float64, the empties --
and the rule each index class uses, on a corpus with one duplicated document."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
Q, W = 3, 6
IDS = np.array([[10, 9, 4, -1, 7, 3],
                [5, 2, 8, 1, 6, 0],
                [3, -1, 2, -1, 1, 0]], dtype=np.int64)
SC = np.array([[1.0, 2.0, 2.0, -INF, 0.5, NAN],
               [-0.0, 0.0, -0.0, 3.0, 0.0, -1.0],
               [-INF] * 6], dtype=np.float32)
KS = (None, 0, 2, W, W + 3, -1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def restate(ids, sc, k, ties, row_len=None):
    """(ids [Q, k], scores [Q, k] in sc's dtype, lens [Q]): descending score, NaN first, -0.0 == +0.0, ties by id or by list position."""
    k = ids.shape[1] if k is None else max(0, min(k, ids.shape[1]))
    key = np.where(np.isnan(sc), np.inf, sc) + 0.0
    out_i, out_s = np.full((len(ids), k), -1, np.int64), np.full((len(ids), k), -np.inf, sc.dtype)
    lens = np.zeros(len(ids), np.int32)
    for q in range(len(ids)):
        n = ids.shape[1] if row_len is None else int(row_len[q])
        cols = (np.lexsort((ids[q, :n], -key[q, :n])) if ties == "id" else np.argsort(-key[q, :n], kind="stable"))[:k]
        if row_len is None:      # a slot no shard owned is a -inf: they sort last, so the owned ones are a prefix
            cols = cols[~np.isneginf(sc[q, cols])]
        out_i[q, :len(cols)], out_s[q, :len(cols)], lens[q] = ids[q, cols], sc[q, cols], len(cols)
    return out_i, out_s, lens


def check(got, want, wide=False):
    ids, sc, lens = want
    assert got.ids.dtype == torch.int64 and got.scores.dtype == torch.float32 and got.lens.dtype == torch.int32
    assert tuple(got.ids.shape) == tuple(got.scores.shape) == ids.shape and got.lens.tolist() == lens.tolist()
    assert np.array_equal(got.ids.cpu().numpy(), ids)
    assert np.array_equal(bits(got.scores), bits(sc.astype(np.float32)))      # the plane's own bits: -0.0 stays -0.0, the NaN its payload
    assert (got.scores64 is not None) == wide
    if wide:
        assert got.scores64.dtype == torch.float64 and np.array_equal(bits(got.scores64), bits(sc))
    pad = np.arange(ids.shape[1])[None, :] >= lens[:, None]
    assert (ids[pad] == -1).all() and np.isneginf(sc[pad]).all()               # (the restatement's own padding, so the device's)


def test_the_fixture_holds_what_it_claims():
    by_id, by_list = restate(IDS, SC, None, "id"), restate(IDS, SC, None, "list")
    assert by_id[0][0].tolist() == [3, 4, 9, 10, 7, -1] and by_list[0][0].tolist() == [3, 9, 4, 10, 7, -1]      # NaN first; the tied pair
    assert by_id[0][1].tolist() == [1, 2, 5, 6, 8, 0] and by_list[0][1].tolist() == [1, 5, 2, 8, 6, 0]
    assert by_id[2].tolist() == by_list[2].tolist() == [5, 6, 0]
    assert np.signbit(by_id[1][1]).tolist() == [False, False, True, False, True, True]                          # -0.0 and +0.0 interleave


@pytest.mark.parametrize("ties", ["id", "list"])
def test_every_k_matches_the_restatement(ties):
    from fusion_amd.distributed import rank_pairs
    ids, sc = dev(IDS), dev(SC)
    for k in KS:
        got = rank_pairs(ids, sc, k, ties=ties)
        check(got, restate(IDS, SC, k, ties))
        assert got.k == {None: W, 0: 0, 2: 2, W: W, W + 3: W, -1: 0}[k]
    assert torch.equal(rank_pairs(ids, sc).ids, rank_pairs(ids, sc, ties="id").ids)      # the default rule is the searches'
    with pytest.raises(ValueError, match="ties"):
        rank_pairs(ids, sc, ties="score")


@pytest.mark.parametrize("ties", ["id", "list"])
def test_row_len_ranks_and_owns_the_listed_columns(ties):
    """Only the first row_len[q] columns take part, and exactly those are owned -- a listed -inf keeps its id (Aggregator.complete_topk)."""
    from fusion_amd.distributed import rank_pairs
    row_len = np.array([W, 4, W], dtype=np.int32)
    for k in (None, 5, 3):
        want = restate(IDS, SC, k, ties, row_len)
        check(rank_pairs(dev(IDS), dev(SC), k, row_len=dev(row_len), ties=ties), want)
        assert want[2].tolist() == [min(n, W if k is None else k) for n in row_len]
    assert restate(IDS, SC, None, "id", row_len)[0][2].tolist() == [-1, -1, 0, 1, 2, 3]      # all -inf and all listed: by id


@pytest.mark.parametrize("ties", ["id", "list"])
def test_float64_scores_rank_as_float64_and_stay(ties):
    from fusion_amd.distributed import rank_pairs
    sc64 = SC.astype(np.float64)
    sc64[0, 2] += 2.0 ** -40                       # the tied pair is a tie in float32 only
    got = rank_pairs(dev(IDS), dev(sc64), ties=ties)
    check(got, restate(IDS, sc64, None, ties), wide=True)
    assert got.ids[0, :3].tolist() == [3, 4, 9] and got.scores[0, 1] == got.scores[0, 2] and got.scores64[0, 1] > got.scores64[0, 2]
    assert np.array_equal(bits(got.scores), bits(got.scores64.cpu().numpy().astype(np.float32)))


@pytest.mark.parametrize("ties", ["id", "list"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_empty_input_comes_back_k_wide(ties, dtype):
    from fusion_amd.distributed import rank_pairs
    for shape in ((0, W), (Q, 0)):
        for k in (None, 2, -1):
            got = rank_pairs(torch.empty(shape, dtype=torch.int64, device="cuda"), torch.empty(shape, dtype=dtype, device="cuda"), k, ties=ties)
            width = shape[1] if k is None else max(0, min(k, shape[1]))
            assert tuple(got.ids.shape) == tuple(got.scores.shape) == (shape[0], width) and got.lens.tolist() == [0] * shape[0]
            assert got.ids.dtype == torch.int64 and got.scores.dtype == torch.float32 and got.lens.dtype == torch.int32
            assert (got.scores64 is not None) == (dtype == torch.float64) and (got.scores64 is None or tuple(got.scores64.shape) == (shape[0], width))


def test_each_index_class_applies_its_own_tie_rule():
    """One corpus of 8 documents in which document 6 is a copy of document 2, as embeddings and as token rows; the candidates list 6 before 2.
    The dense rerank puts the tied pair in id order, the token rerank leaves it in list order; everything else about the lists agrees with
    rank_pairs on the class's own pair scores."""
    from fusion_amd.distributed import ShardedDenseIndex, ShardedTokenIndex, rank_pairs
    rng = np.random.default_rng(29)
    unit = lambda x: (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)      # noqa: E731
    N, base = 8, 1000
    cand = dev(np.array([[base + 6, base + 5, base + 2, base + 0, base + N, -1], [base + 7, base + 6, base + 1, base + 2, base + 3, base + 4]], np.int64))
    Dn = unit(rng.standard_normal((N, 64)))
    Dn[6] = Dn[2]
    tok = unit(rng.standard_normal((N, 3, 128))).astype(np.float16)
    tok[6] = tok[2]
    dense = ShardedDenseIndex(dev(Dn), base)
    token = ShardedTokenIndex(dev(tok.reshape(N * 3, 128)), dev(np.arange(N + 1, dtype=np.int64) * 3), base, max_doc_len=64)
    Qn, Qtok = dev(unit(rng.standard_normal((2, 64)))), dev(unit(rng.standard_normal((2, 32, 128))).astype(np.float16))
    for index, q, first in ((dense, Qn, base + 2), (token, Qtok, base + 6)):
        got, plane = index.rerank(q, cand), index.pair_scores(q, cand)
        want = rank_pairs(cand, plane, ties=index.TIES)
        assert torch.equal(got.ids, want.ids) and np.array_equal(bits(got.scores), bits(want.scores)) and got.lens.tolist() == [4, 6]
        for row in got.ids.tolist():
            at = row.index(first)
            assert row[at + 1] == 2 * base + 8 - first, (type(index).__name__, row)      # the copy follows at once: a tie, in the class's order
        assert plane[0, 0].item() == plane[0, 2].item() and plane[1, 1].item() == plane[1, 3].item()
    assert (ShardedDenseIndex.TIES, ShardedTokenIndex.TIES) == ("id", "list")
