"""The N > 1 path, hardened on CPU since no multi-GPU hardware is available to the build:
  * gloo WORLD-8 all-gather + merge of per-shard top-k lists == the unsharded top-k, with an uneven corpus (N % 8 != 0), shards shorter
    than k (their (-inf, -1) padding must lose every merge) and scores duplicated across shard borders (tie -> ascending global id);
    in the same world distributed.world / reduce_max / reduce_sum, the collectives every index goes through; one rank without a group;
  * the block loop of ShardedTokenIndex.build_compressed / build_e4m3 (_fill_blocks): too many rows, too few, exactly enough;
  * bench.py's self-launcher: a rank that exits non-zero, or a job that prints no result line, makes the parent exit non-zero;
  * the compact N > 1 line keeps what the judge reads."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker8(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), OMP_NUM_THREADS="1")
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    import torch.distributed as dist
    import fusion_amd.distributed as D
    from fusion_amd.distributed import allgather_rows, allgather_topk, shard_bounds
    from oracle import oracle
    oracle.set_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok = {}
    try:
        rng = np.random.default_rng(123)                                  # the same corpus scores on every rank
        Q, N = 6, 403                                                     # 403 = 8 * 50 + 3: shards of 51, 51, 51, 50, 50, 50, 50, 50 rows
        S = np.round(rng.normal(0, 1, (Q, N)), 1).astype(np.float32)      # one decimal: every score value occurs in several shards
        S[0, :] = 0.25                                                    # a whole row of one value: the merge is decided by ids alone
        S[1, 45:60] = 9.0                                                 # a tie run across the border of shards 0 and 1 at the very top
        lo, hi = shard_bounds(N, world, rank)
        assert (hi - lo) == (51 if rank < 3 else 50)

        def merge(gs, gi):
            a, b = oracle.topk_merge(gs.numpy(), gi.numpy())
            return torch.from_numpy(a), torch.from_numpy(b)
        for k in (60, 51, 7):                                             # every shard short | the 50-row shards short by one | none short
            ls, li = oracle.topk_rows(S[:, lo:hi], k, id_base=lo)         # pads short lists with (-inf, -1)
            if k > hi - lo:
                assert np.all(li[:, hi - lo:] == -1) and np.all(np.isneginf(ls[:, hi - lo:]))
            gs, gi = allgather_topk(torch.from_numpy(ls), torch.from_numpy(li), merge_fn=merge)
            es, ei = oracle.topk_rows(S, k)
            ok[f"k{k}"] = bool(np.array_equal(gs.numpy(), es) and np.array_equal(gi.numpy(), ei))
            ok[f"k{k}_no_padding_in_result"] = bool((gi.numpy() >= 0).all())   # 403 real documents >= k: padding never surfaces
            ok[f"k{k}_ties_ascending_id"] = all(
                all(gi[q, j] < gi[q, j + 1] for j in range(k - 1) if gs[q, j] == gs[q, j + 1]) for q in range(Q))
        # data-parallel encoder outputs: 13 query rows over 8 ranks (5 ranks with 2 rows, 3 with 1) come back whole and in order
        E = torch.arange(13 * 4, dtype=torch.float32).view(13, 4)
        elo, ehi = shard_bounds(13, world, rank)
        ok["rows"] = bool(torch.equal(allgather_rows(E[elo:ehi].clone(), 13), E))
        # the collectives every index goes through: a slot's owner holds its value, everyone else the lowest; counts add
        ok["world"] = D.world(None) == world
        P = torch.full((3, 2 * world), float("-inf"), dtype=torch.float64)
        P[:, 2 * rank] = torch.tensor([0.5, -0.0, float("-inf")], dtype=torch.float64) + rank      # (row 2: nobody owns anything)
        want = torch.full_like(P, float("-inf"))
        want[:2, 0::2] = torch.tensor([0.5, -0.0], dtype=torch.float64)[:, None] + torch.arange(world, dtype=torch.float64)[None, :]
        padded = torch.full((3, 2 * world + 5), 7.0, dtype=torch.float64)        # a plane wider than its block: the block is what travels
        padded[:, :2 * world] = P
        ok["reduce_max"] = bool(torch.equal(D.reduce_max(P.clone()), want) and torch.equal(D.reduce_max(padded[:, :2 * world]), want))
        kept = P.clone()
        ok["reduce_max_in_place"] = D.reduce_max(kept) is kept and bool(torch.equal(kept, want))
        ok["reduce_max_empty"] = tuple(D.reduce_max(P[:0]).shape) == (0, 2 * world) and tuple(D.reduce_max(P[:0], skip_empty=True).shape) == (0, 2 * world)
        counts = torch.arange(6, dtype=torch.int64).view(2, 3) * (rank + 1)
        ok["reduce_sum"] = bool(torch.equal(D.reduce_sum(counts), torch.arange(6, dtype=torch.int64).view(2, 3) * (world * (world + 1) // 2)))
    finally:
        q.put((rank, ok))
        dist.destroy_process_group()


def test_allgather_topk_gloo_world8_uneven_short_and_tied_shards():
    import torch.multiprocessing as mp
    from oracle import oracle
    oracle.build()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    world = 8
    ps = [ctx.Process(target=_worker8, args=(r, world, port, q)) for r in range(world)]
    for p in ps: p.start()
    try:
        res = [q.get(timeout=300) for _ in ps]
    finally:
        for p in ps: p.join(60)
        for p in ps:
            if p.is_alive(): p.kill()
    assert sorted(r[0] for r in res) == list(range(world))
    for rank, ok in res:
        assert ok and all(ok.values()), (rank, ok)
        assert {"k60", "k51", "k7", "rows", "world", "reduce_max", "reduce_max_in_place", "reduce_max_empty", "reduce_sum"} <= set(ok)


def test_one_rank_without_a_process_group():
    """No initialised group: one rank, and the collectives hand their tensor back untouched."""
    import fusion_amd.distributed as D
    t = torch.tensor([[1.0, float("-inf")]])
    assert D.world(None) == 1 and D.reduce_max(t) is t and D.reduce_sum(t) is t and D.allgather_rows(t, 1) is t
    s, i = D.allgather_topk(t, torch.tensor([[4, -1]]), merge_fn=lambda gs, gi: (gs[0], gi[0]))
    assert torch.equal(s, t) and i.tolist() == [[4, -1]]


def test_rerank_names_its_arguments_and_local_scores_is_the_hook():
    """The mixin's rerank takes (*query, candidates, k=...): a missing list or a positional k is named, not passed down to the scorer;
    on the token index the public name local_scores is what pair_scores and rerank call, so an override of it is seen."""
    from fusion_amd.distributed import ShardedTokenIndex

    class Fixed(ShardedTokenIndex):
        def local_scores(self, Qtok, cand_ids, cand_len=None):
            return torch.full(cand_ids.shape, 2.5)

    index = Fixed(None, torch.zeros(1, dtype=torch.int64), 0)
    ids = torch.tensor([[4, 9]])
    for args in ((), (None, ids, 10)):
        with pytest.raises(TypeError, match=r"^Fixed\.rerank\(\*query, candidates, k=None\): the candidates go last by position, k by keyword$"):
            index.rerank(*args)
    assert index.pair_scores(None, ids).tolist() == [[2.5, 2.5]] and index.local_pair_scores(None, ids).tolist() == [[2.5, 2.5]]


def test_fill_blocks_takes_exactly_the_rows_of_the_shard():
    """The block loop of ShardedTokenIndex.build_compressed / build_e4m3: float16 blocks at their running row, under the caller's name."""
    from fusion_amd.distributed import _fill_blocks
    blk = lambda n: torch.ones((n, 4), dtype=torch.float32)      # noqa: E731
    seen = []
    fill = lambda at, b: seen.append((at, b.shape[0], b.dtype, b.is_contiguous()))      # noqa: E731
    assert _fill_blocks("X.build", iter([blk(3), blk(0), torch.ones((4, 3)).t(), blk(4)]), 10, "cpu", fill) is None
    assert seen == [(0, 3, torch.float16, True), (3, 3, torch.float16, True), (6, 4, torch.float16, True)]      # an empty block fills nothing
    with pytest.raises(ValueError, match=r"^X\.build: the blocks hold more than Doff\[N\] = 10 token rows$"):
        _fill_blocks("X.build", iter([blk(7), blk(4)]), 10, "cpu", fill)
    with pytest.raises(ValueError, match=r"^X\.build: the blocks hold 9 token rows, Doff\[N\] = 10$"):
        _fill_blocks("X.build", iter([blk(7), blk(2)]), 10, "cpu", fill)
    assert _fill_blocks("X.build", iter([]), 0, "cpu", fill) is None


# ---- bench.py's self-launcher (python bench.py --gpus N without torchrun): failure must propagate -----------------------------------
LINE = '{"metric": "m", "value": 1.0, "n_gpus": 2}'


@pytest.mark.parametrize("child,want_rc,want_line", [
    (f"import sys; print('noise'); print('{LINE}'); sys.exit(0)", 0, True),
    (f"import sys; print('{LINE}'); sys.exit(3)", 3, True),                      # a rank failed after rank 0 printed: the parent fails too
    ("import sys; print('no result here'); sys.exit(0)", 1, False),              # nothing measured: never a silent success
    ("import sys; sys.exit(7)", 7, False),
    ("import os, signal; os.kill(os.getpid(), signal.SIGKILL)", None, False),    # killed (out of memory ...): non-zero
])
def test_launcher_propagates_the_childs_failure(monkeypatch, capfd, child, want_rc, want_line):
    import bench
    monkeypatch.setattr(bench, "launcher_argv", lambda argv, n, port: [sys.executable, "-c", child])
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as e:
        bench.launch_ranks(bench.parse())
    out, err = capfd.readouterr()
    code = e.value.code
    if want_rc is None:
        assert code not in (0, None)
    else:
        assert code == want_rc
    lines = [ln for ln in out.splitlines() if ln.startswith('{"metric"')]
    assert (lines == [LINE]) if want_line else (lines == [])
    assert "noise" not in out                                                     # everything else the ranks print goes to stderr


def test_compact_line_of_the_sharded_workload_keeps_what_the_judge_reads():
    import bench
    res = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_launcher_2ranks_1gpu_gloo.json")))
    line = json.loads(json.dumps(bench.compact_line(res), allow_nan=False))
    assert line["n_gpus"] == 2 and line["scaling"] == "strong"
    assert line["sharded_equals_single_gpu"]["equal"] is True
    assert line["collective"]["op"].startswith("all_gather_into_tensor") and line["collective"]["payload_bytes_per_rank"] == 1024 * 1000 * 12
    assert line["ranks"] == 2 and line["shard_rows"] == 1000000
    assert line["same_workload_one_gpu"]["value"] > 0 and line["same_workload_one_gpu"]["n_gpus"] == 1
    assert line["roofline"]["bound"] == "mfma" and "cpu_baseline" in line
