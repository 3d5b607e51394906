"""The weight sweep over corpus-scale top-k lists: Aggregator.tune_topk as a whole and its three stages -- normalise the lists, the
per-query join to per-system columns (ops.lists_columns, csrc/lists_tune.hip), count + metrics (ops.gold_ranks + ops.tune_metrics,
the dense sweep's kernels, and the [W, 15] copy to the host) -- at Q = 1024, k = 1000, S = 3 (231 weight vectors) and S = 4
(1,771), for min-max and percentile-rank, timed with HIP events after warm-up.  Next to them:

  * the only device route such lists had before: one Aggregator.fuse_topk + run_evaluation per weight vector.  It is timed on a
    SAMPLE of 8 vectors (host clock around work that ends in a device-to-host copy) and SCALED to W; the record says so;
  * ops.lists_join (rrf) on the same lists: the expectation to confirm or refute is that the columns join costs about what it does;
  * the dense sweep's counting at its own row size (S planes of N = 27,942 columns, same Q, W and gold counts): the expectation to
    confirm or refute is that counting over rows of at most S x k columns costs less.

Lists as tools/bench_fuse_topk.py makes them; 1-5 gold ids per query, two thirds of them out of the query's own lists.

Usage: python tools/bench_tune_topk.py [--out profiles/r12_tune_topk.json] [--systems 3,4] [--queries 1024] [--k 1000] [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fuse_topk import event_ms, make_systems  # noqa: E402
from fusion_amd import ops  # noqa: E402
from fusion_amd.retrievers.hybrid import Aggregator, run_evaluation, weight_grid  # noqa: E402

DENSE_N = 27_942


def make_labels(systems, seed):
    rng = np.random.default_rng(seed)
    names = list(systems)
    heads = [systems[n].ids[:, :50].cpu().numpy() for n in names]
    labels = []
    for q in range(heads[0].shape[0]):
        gl = []
        for j in range(int(rng.integers(1, 6))):
            gl.append(int(heads[int(rng.integers(0, len(names)))][q, int(rng.integers(0, 50))]) if j % 3 != 2 else (1 << 50) + q)
        labels.append(gl)
    return labels


def dense_count_ms(S, Q, W, wide, reps):
    """ops.gold_ranks + ops.tune_metrics on S full planes of DENSE_N columns: the dense sweep's counting stage at LLeQA's row size."""
    g = torch.Generator(device="cuda").manual_seed(11)
    T = []
    for _ in range(S):
        t = ops.alloc_plane(Q, DENSE_N, torch.float32, "cuda")
        t.copy_(torch.rand((Q, DENSE_N), generator=g, device="cuda"))
        T.append(t)
    pos = ops.alloc_plane(Q, DENSE_N, torch.int32, "cuda")
    pos.copy_(torch.rand((Q, DENSE_N), generator=g, device="cuda").argsort(1).int())
    gold = torch.full((Q, 8), -1, dtype=torch.int32, device="cuda")
    gold[:, :3] = torch.randint(0, DENSE_N, (Q, 3), generator=g, device="cuda").int()
    weights = torch.rand((W, S), generator=g, device="cuda", dtype=torch.float64).to(torch.float64 if wide else torch.float32)
    n_gold = np.full(Q, 3, dtype=np.int64)
    return event_ms(lambda: Aggregator._metrics_of_gold_ranks(ops.gold_ranks(T, pos, weights, gold), gold, pos, n_gold, T[0].device), reps)


def run(S, Q, k, reps, sample):
    systems = make_systems(S, Q, k, seed=S)
    names = list(systems)
    Sx = [systems[n] for n in names]
    labels = make_labels(systems, seed=S)
    grid = weight_grid(names)                       # hybrid.py:405-409: np.float64 weights, 231 / 1,771 vectors for S = 3 / 4
    W = len(grid)
    dev = Sx[0].ids.device
    weights = torch.tensor([[float(w[n]) for n in names] for w in grid], dtype=torch.float64, device=dev)
    out = dict(S=S, Q=Q, k=k, W=W, weights="np.float64 (the float64 sweep)")
    ids, lens = [s.ids for s in Sx], [s.lens for s in Sx]
    out["lists_join_rrf"] = event_ms(lambda: ops.lists_join(ids, lens, "rrf"), reps)
    for norm in ("min-max", "percentile-rank"):
        distr = {n: np.quantile(systems[n].scores[:64].cpu().numpy().ravel(), np.linspace(0, 1, 1001)) for n in names}
        Tn = Aggregator._normalised_lists(names, Sx, norm, distr)
        gold_dev, Gmax, n_gold = Aggregator._gold_ids(labels, Q, dev)
        _, T, pos, out_len, gold_col = ops.lists_columns(ids, lens, Tn, gold_dev)
        rec = dict(
            tune_topk=event_ms(lambda: Aggregator.tune_topk(systems, norm, grid, labels, distr), reps),
            stage_normalise=event_ms(lambda: Aggregator._normalised_lists(names, Sx, norm, distr), reps),
            stage_columns_join=event_ms(lambda: ops.lists_columns(ids, lens, Tn, gold_dev), reps),
            stage_count_and_metrics=event_ms(lambda: Aggregator._metrics_of_gold_ranks(ops.gold_ranks(T, pos, weights, gold_col), gold_col, pos,
                                                                                      n_gold, dev), reps),
            union_mean=round(float(out_len.float().mean()), 1), gold_max=Gmax)
        # the parent's device route on a sample of the grid, scaled to W
        pick = [grid[i] for i in np.linspace(0, W - 1, sample).round().astype(int)]
        per = lambda w: run_evaluation(Aggregator.fuse_topk(systems, "nsf", norm, w, distr, topk=1000).predictions(1000), labels, print2console=False)
        per(pick[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exp = [per(w) for w in pick]
        ms = (time.perf_counter() - t0) * 1e3
        rec["per_vector_route"] = dict(vectors_timed=len(pick), ms_measured=round(ms, 1), ms_scaled_to_W=round(ms * W / len(pick), 1),
                                       note="a SCALED SAMPLE: fuse_topk(topk=1000) + run_evaluation per vector, host clock, measured on "
                                            f"{len(pick)} of the {W} vectors and multiplied by W / {len(pick)}")
        rec["speedup_vs_per_vector_route"] = round(rec["per_vector_route"]["ms_scaled_to_W"] / rec["tune_topk"]["median_ms"], 1)
        got = Aggregator.tune_topk(systems, norm, pick, labels, distr)
        rec["max_metric_difference_to_per_vector_route"] = float(max(abs(g[m] - e[m]) for g, e in zip(got, exp) for m in e))
        out[norm] = rec
    out["dense_count_and_metrics_N27942"] = dense_count_ms(S, Q, W, True, max(reps // 2, 3))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="3,4")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=8, help="weight vectors sent through the per-vector route")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r12_tune_topk.json"))
    a = ap.parse_args()
    dev = torch.cuda.get_device_properties(0)
    out = dict(what="weight sweep over top-k lists: Aggregator.tune_topk and its stages (normalise, ops.lists_columns, gold_ranks + tune_metrics) "
                    "vs one fuse_topk + run_evaluation per vector (scaled sample); HIP events, median of %d after 3 warm-up calls" % a.reps,
               device=dev.name, runs=[])
    for S in (int(x) for x in a.systems.split(",")):
        out["runs"].append(run(S, a.queries, a.k, a.reps, a.sample))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
