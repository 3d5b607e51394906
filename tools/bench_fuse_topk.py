"""Fusion of corpus-scale top-k lists: the per-query id join (ops.lists_join, csrc/lists.hip) and the whole Aggregator.fuse_topk
(normalise, join, final row sort, gather) at Q = 1024, k = 1000, S in {2, 3, 4, 8}, for rrf and nsf min-max, timed with HIP events
after warm-up -- next to two yardsticks:

  * the only route such lists had before: Aggregator.fuse(lists as dicts, as_device=True) on blocks of 8 queries (more does not fit
    its planes, which are as wide as the block's union of ids), total for the 1024 queries, host packing included (host clock around
    work that ends in a synchronise);
  * the algorithmic bytes per call -- sum_s len_s x (8 + 4) in, U x (8 + 8) out per query -- over the measured time, as a fraction
    of the 8 TB/s HBM roof (the join is expected to be LDS- and latency-bound, far from it: the fraction is reported, not chased);
  * for orientation, the dense path's analogue of the join at the same row size: insertion_order over S order planes + the float64
    row sort at N = 4,096.

Lists: per query a pool of k (1 + S / 2) candidate ids out of an 8,841,823-id space offset beyond 2^32; every system lists k of
them (BM25-like scores for system 0, cosine-like for the others), so the union grows with S.

Usage: python tools/bench_fuse_topk.py [--out profiles/r08_fuse_topk.json] [--systems 2,3,4,8] [--old-queries 1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusion_amd import ops  # noqa: E402
from fusion_amd.planes import FusedTopk, RankedTopk  # noqa: E402
from fusion_amd.retrievers.hybrid import Aggregator  # noqa: E402

CORPUS = 8_841_823
ID_BASE = 3 << 31
HBM_BYTES_PER_S = 8e12


def make_systems(S, Q, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    torch.manual_seed(seed)
    pool = int(k * (1 + S / 2))
    assert pool * 1009 < CORPUS
    off = torch.randint(0, CORPUS, (Q, 1), generator=g, device="cuda")
    systems = {}
    for s in range(S):
        pick = torch.rand((Q, pool), generator=g, device="cuda").argsort(1)[:, :k]          # k distinct pool slots per query
        ids = (pick * 1009 + off) % CORPUS + ID_BASE                                         # distinct slots -> distinct ids
        if s == 0:   # BM25-like: a gamma body, exact zeros in the tail
            sc = torch.clamp(torch.distributions.Gamma(0.5, 0.25).sample((Q, k)).cuda() - 2.0, min=0.0)
        else:
            sc = torch.rand((Q, k), generator=g, device="cuda") * 1.1 - 0.2
        sc = sc.float().sort(dim=1, descending=True, stable=True).values.contiguous()
        systems[f"s{s}"] = RankedTopk(ids=ids.contiguous(), scores=sc, lens=torch.full((Q,), k, dtype=torch.int32, device="cuda"))
    return systems


def event_ms(f, reps, warm=3):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(median_ms=round(float(np.median(times)), 4), min_ms=round(float(np.min(times)), 4), max_ms=round(float(np.max(times)), 4))


def old_route_ms(systems, method, norm, weights, n_queries, block=8):
    """The dict-list boundary in blocks of `block` queries; returns (total ms for n_queries, the first block's fused lists)."""
    host = {n: t.to_lists() for n, t in systems.items()}
    first = None
    Aggregator.fuse({n: l[:block] for n, l in host.items()}, method, norm, weights, {}, as_device=True)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for lo in range(0, n_queries, block):
        res = Aggregator.fuse({n: l[lo:lo + block] for n, l in host.items()}, method, norm, weights, {}, as_device=True)
        if first is None:
            first = res
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, first


def dense_analogue_ms(S, Q, k, reps, N=4096):
    """insertion_order over S order planes (k of N positions listed per system) + the float64 row sort of an N-wide fused plane."""
    g = torch.Generator(device="cuda").manual_seed(9)
    orders = []
    for _ in range(S):
        o = ops.alloc_plane(Q, N, torch.int32, "cuda", fill=-1)
        o[:, :k] = torch.rand((Q, N), generator=g, device="cuda").argsort(1)[:, :k].int()
        orders.append(o)
    lens = torch.full((S, Q), k, dtype=torch.int32, device="cuda")
    fused = ops.alloc_plane(Q, N, torch.float64, "cuda")
    fused.copy_(torch.rand((Q, N), generator=g, device="cuda", dtype=torch.float64))

    def run():
        ins, U = ops.insertion_order(orders, lens, N)
        ops.sort_rows_desc(fused, init_order=ins, row_len=U)
    return event_ms(run, reps)


def run(S, Q, k, reps, old_queries):
    systems = make_systems(S, Q, k, seed=S)
    names = list(systems)
    ids, lens = [systems[n].ids for n in names], [systems[n].lens for n in names]
    weights = {n: 1.0 / S for n in names}
    out = dict(S=S, Q=Q, k=k, entries_per_query=S * k)
    for method, norm in (("rrf", "none"), ("nsf", "min-max")):
        key = method if method == "rrf" else f"{method}_{norm}"
        if method == "rrf":
            join = lambda: ops.lists_join(ids, lens, "rrf")
        else:   # the join's own share of nsf: it weights and sums float32 planes the normalisation made beforehand (any [Q, k] float32 plane times alike)
            vals = [systems[n].scores for n in names]
            join = lambda: ops.lists_join(ids, lens, "wsum32", vals, [weights[n] for n in names])
        whole = lambda: Aggregator.fuse_topk(systems, method, norm, weights, {})
        j, w = event_ms(join, reps), event_ms(whole, reps)
        fused = whole()
        U = float(fused.lens.float().mean())
        bytes_in, bytes_out = S * k * 12, U * 16
        frac = lambda ms: round((bytes_in + bytes_out) * Q / (ms * 1e-3) / HBM_BYTES_PER_S, 5)
        rec = dict(join=j, fuse_topk=w, union_mean=round(U, 1), algorithmic_bytes_per_query=int(bytes_in + bytes_out),
                   join_fraction_of_8TBs=frac(j["median_ms"]), fuse_topk_fraction_of_8TBs=frac(w["median_ms"]))
        if old_queries:
            old_ms, first = old_route_ms(systems, method, norm, weights, old_queries)
            rec["old_route_ms_measured"] = round(old_ms, 1)
            rec["old_route_queries_measured"] = old_queries
            rec["old_route_ms_per_1024q"] = round(old_ms * 1024 / old_queries, 1)
            rec["speedup_vs_old_route"] = round(rec["old_route_ms_per_1024q"] / (w["median_ms"] * 1024 / Q), 1)
            a, b = first_lists(fused, 8), first.to_lists()
            rec["identical_to_old_route_first_block"] = bool(
                all([x["corpus_id"] for x in p] == [x["corpus_id"] for x in r] and [float(x["score"]) for x in p] == [float(x["score"]) for x in r]
                    for p, r in zip(a, b)))
        out[key] = rec
    out["dense_analogue_insertion_order_plus_f64_sort_N4096"] = dense_analogue_ms(S, Q, k, reps)
    print(json.dumps(out), flush=True)
    return out


def first_lists(fused, n):
    """The first n fused lists as dict lists (the whole batch's would be 1024 x 2,500 dicts for nothing)."""
    return FusedTopk(ids=fused.ids[:n], scores=fused.scores[:n], lens=fused.lens[:n]).to_lists()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="2,3,4,8")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--old-queries", type=int, default=1024, help="queries sent through the dict-list route (0: skip it)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r08_fuse_topk.json"))
    a = ap.parse_args()
    dev = torch.cuda.get_device_properties(0)
    out = dict(what="fusion of top-k lists: per-query id join (ops.lists_join) and the whole Aggregator.fuse_topk vs the dict-list route in blocks "
                    "of 8 queries; HIP events, median of %d after 3 warm-up calls; the old route by the host clock around a synchronise" % a.reps,
               device=dev.name, lists_max_entries=ops.lists_max_entries(), runs=[])
    for S in (int(x) for x in a.systems.split(",")):
        out["runs"].append(run(S, a.queries, a.k, a.reps, min(a.old_queries, a.queries)))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
