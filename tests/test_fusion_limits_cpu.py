"""Fusion at the system-count limit without a device: more than FZ_MAX_SYSTEMS = 8 systems are refused on the host before anything
is looked at or launched, and the oracle at eight systems agrees with a plain NumPy float64 evaluation of the reference's arithmetic
(the golden fixtures never had eight systems, so the oracle is not the only witness there)."""
import numpy as np
import pytest
import torch

from fusion_amd import ops


def _f32(S=9):
    return [torch.zeros((2, 5)) for _ in range(S)]


def _i32(S=9):
    return [torch.zeros((2, 5), dtype=torch.int32) for _ in range(S)]


_LENS = torch.full((9, 2), 5, dtype=torch.int32)
NINE = {
    "fuse_rank": lambda: ops.fuse_rank(_i32(), _LENS, "rrf"),
    "sort_rank_fused": lambda: ops.sort_rank_fused(_i32(), _LENS, "bcf"),
    "fuse_nsf": lambda: ops.fuse_nsf(_f32(), None, [0.1] * 9, "min-max"),
    "fuse_nsf(stats)": lambda: ops.fuse_nsf(_f32(), _i32(), [0.1] * 9, "z-score", stats=(torch.zeros(18), torch.ones(18))),
    "fuse_nsf(tables)": lambda: ops.fuse_nsf(_f32(), None, [0.1] * 9, "percentile-rank", [torch.zeros(11)] * 9),
    "fuse_none": lambda: ops.fuse_none(_f32(), None, [0.1] * 9),
    "fuse_wsum": lambda: ops.fuse_wsum(_f32(), None, [0.1] * 9, narrow=[True] * 9),
    "insertion_order": lambda: ops.insertion_order(_i32(), _LENS, 5),
    "nsf_tables_prepare": lambda: ops.nsf_tables_prepare([torch.zeros(11)] * 9, "normal-curve-equivalent"),
    "gold_ranks": lambda: ops.gold_ranks(_f32(), _i32(1)[0], torch.zeros((3, 9)), torch.zeros((2, 4), dtype=torch.int32)),
}


@pytest.mark.parametrize("entry", sorted(NINE))
def test_nine_systems_are_refused_before_launch(entry):
    # CPU tensors: without the count check the call would fail on its first tensor (TypeError), not with this message
    with pytest.raises(ValueError, match=r"9 systems, but fusion takes at most 8"):
        NINE[entry]()


def test_eight_systems_pass_the_count_check():
    with pytest.raises(TypeError, match="no CPU path"):     # the next check down: the tensors are not on the GPU
        ops.fuse_nsf(_f32(8), None, [0.1] * 8, "min-max")


@pytest.mark.parametrize("call", ["fuse", "tune"])
def test_aggregator_refuses_nine_systems(call):
    from fusion_amd.retrievers.hybrid import Aggregator
    lists = {f"s{k}": [[{"corpus_id": 1, "score": 1.0}, {"corpus_id": 2 + k, "score": 0.5}]] for k in range(9)}
    with pytest.raises(ValueError, match="at most 8"):
        if call == "fuse":
            Aggregator.fuse(lists, "nsf", "min-max", {s: 0.1 for s in lists}, {})
        else:
            Aggregator.tune(lists, "min-max", [{s: 0.1 for s in lists}], [[1]], {})


def _eight(rng, Q=2, N=40):
    S = 8
    planes = [rng.normal(s, 1.0 + s, (Q, N)).astype(np.float32) for s in range(S)]
    listed = [np.ones((Q, N), bool) if s % 2 == 0 else rng.random((Q, N)) < 0.6 for s in range(S)]
    for m in listed:
        m[:, 0] = True                      # every list holds at least two documents
        m[:, 1] = True
    listed[7][:, 2:] = False                # and one holds only those two
    ranks = [np.where(m, 0, -1).astype(np.int32) for m in listed]
    return planes, listed, ranks


def test_oracle_minmax_at_eight_systems_against_numpy(oracle):
    rng = np.random.default_rng(8)
    planes, listed, ranks = _eight(rng)
    w = rng.dirichlet(np.ones(8))
    Q, N = planes[0].shape
    acc, present = np.zeros((Q, N)), np.zeros((Q, N), bool)
    for x, m, ws in zip(planes, listed, w):
        x = x.astype(np.float64)
        for q in range(Q):
            lo, hi = x[q][m[q]].min(), x[q][m[q]].max()
            t = (x[q] - lo) / (hi - lo)                       # hybrid.py:255-258
            acc[q] += np.where(m[q], ws * t, 0.0)             # hybrid.py:291,301-304
        present |= m
    ref = np.where(present, acc, -np.inf)
    got = oracle.fuse_nsf(planes, ranks, w, "min-max").astype(np.float64)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)) and np.array_equal(got[~present], ref[~present])
    assert np.max(np.abs(got[present] - ref[present])) <= 1e-6


def test_oracle_weighted_sum_at_eight_systems_against_numpy(oracle):
    rng = np.random.default_rng(88)
    _, listed, ranks = _eight(rng)
    planes = [rng.uniform(-1.0, 1.0, listed[0].shape) for _ in range(8)]     # |score * weight| < 1: a float32 product is within 6e-8
    planes = [p if s % 3 == 0 else p.astype(np.float32) for s, p in enumerate(planes)]
    w = rng.uniform(0.1, 1.0, 8)
    present = np.any(listed, axis=0)
    ref = np.where(present, sum(np.where(m, ws * x.astype(np.float64), 0.0) for x, m, ws in zip(planes, listed, w)), -np.inf)
    for narrow in ([False] * 8, [s % 2 == 0 for s in range(8)]):   # np.float64 weights, then weak Python-float ones in between
        got = oracle.fuse_wsum(planes, ranks, w, narrow)
        assert np.array_equal(got[~present], ref[~present])
        assert np.max(np.abs(got[present] - ref[present])) <= 1e-6
