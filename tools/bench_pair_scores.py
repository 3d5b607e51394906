"""Pair scores and list completion at the corpus-scale shape (ops.dot_pairs / ops.sparse_dot_pairs, csrc/pairs.hip;
Aggregator.complete_topk): Q = 1024 queries, W = 3,000 candidates each, drawn uniformly (with repetition) from one shard of 1,105,228
passages -- the union of three systems' top-1000 lists.  HIP events, median of --reps calls after warm-up.

  dense    Dn [1,105,228, 768] float32 unit rows (3.4 GB).  The kernel is a gather: every pair reads its own 3 KB row, so the figure is
           gathered bytes (Q x W x d x 4) over time, next to the project's own measured gather kernel -- maxsim_pairs, 18.0 GB of token
           rows in 2.99 ms (profiles/r18_colbert_residual.json, read at run time) -- and the 5.5-5.8 TB/s that MI355X_MICROARCH.md measures
           for whole-row register gathers.  The bits of a sample of rows are compared with ops.dot_scores.
  sparse   the SPLADE-shaped index of tools/bench_splade_search.py (~166 postings per document, ~37 terms per query).
  complete Aggregator.complete_topk + fuse_topk for S = 3 (dense, sparse, a second dense system of d = 384) at depth 2,730, against
           fuse_topk of the cut top-1000 lists; the lists are each system's own search over the shard.

Usage: python tools/bench_pair_scores.py [--out profiles/r20_pair_scores.json] [--only dense|sparse]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fusion_amd import ops  # noqa: E402
from fusion_amd.distributed import ShardedDenseIndex, ShardedSparseIndex  # noqa: E402
from fusion_amd.planes import RankedTopk  # noqa: E402
from fusion_amd.retrievers.hybrid import Aggregator  # noqa: E402
from bench_splade_search import V, splade_blocks  # noqa: E402

GATHER_TBS = (5.5, 5.8)      # MI355X_MICROARCH.md, 'Indexed rows: gather into LDS': whole rows into registers, far beyond the Infinity Cache
ID_BASE = 3 << 31


def unit_rows(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty((n, d), device="cuda")
    step = 1 << 18
    for lo in range(0, n, step):
        x = torch.randn((min(step, n - lo), d), generator=g, device="cuda")
        X[lo:lo + x.shape[0]] = x / x.norm(dim=1, keepdim=True)
    return X


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
    return dict(median_ms=round(float(np.median(times)), 4), min_ms=round(float(np.min(times)), 4), max_ms=round(float(np.max(times)), 4), reps=reps)


def yardstick():
    """maxsim_pairs as measured: (gathered GB, ms) of the uncompressed kernel in profiles/r18_colbert_residual.json."""
    with open(os.path.join(ROOT, "profiles", "r18_colbert_residual.json")) as f:
        r = json.load(f)
    gb, ms = r["corpus"]["gathered_float16_GB"], r["kernel"]["nbits2"]["uncompressed"]["median_ms"]
    return dict(source="profiles/r18_colbert_residual.json", gathered_GB=gb, median_ms=ms, achieved_TBs=round(gb / ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--width", type=int, default=3000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--docs", type=int, default=1_105_228)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--depth", type=int, default=2730)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", choices=("dense", "sparse"), help="one kernel alone, --reps calls (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_pair_scores.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_scores.py measures on the GPU: no device found")
    Q, W, d, N = a.queries, a.width, a.dim, a.docs
    pos = torch.randint(0, N, (Q, W), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    cand = pos + ID_BASE
    out_plane = ops.alloc_plane(Q, W, torch.float32, "cuda")
    rec = dict(what="pair scores over candidate lists (fz_dot_pairs_f32, fz_sparse_dot_pairs_f32) and list completion: HIP events, median of "
                    "%d calls after 3 warm-up calls" % a.reps,
               device=torch.cuda.get_device_properties(0).name, Q=Q, W=W, docs=N, candidates="uniform over the shard, with repetition")

    if a.only != "sparse":
        Dn, Qn = unit_rows(N, d, 1), unit_rows(Q, d, 2)
        dense = lambda: ops.dot_pairs(Qn, Dn, cand, id_base=ID_BASE, out=out_plane)      # noqa: E731
        t = event_ms(dense, a.reps)
        gathered, flops = Q * W * d * 4, 2.0 * Q * W * d
        sec = t["median_ms"] * 1e-3
        ref = yardstick()
        sample = ops.dot_scores(Qn[:4].contiguous(), Dn)
        same = bool(torch.equal(torch.gather(sample, 1, pos[:4]).view(torch.int32), dense()[:4].contiguous().view(torch.int32)))
        del sample
        rec["dense"] = dict(d=d, corpus_GB=round(N * d * 4 / 1e9, 2), gathered_GB=round(gathered / 1e9, 3), GFLOP=round(flops / 1e9, 2), dot_pairs=t,
                            achieved_TBs=round(gathered / sec / 1e12, 3), maxsim_pairs_yardstick=ref,
                            fraction_of_maxsim_pairs_rate=round(gathered / sec / 1e12 / ref["achieved_TBs"], 3),
                            time_from_bytes_ms={f"at_{r}_TBs": round(gathered / (r * 1e12) * 1e3, 4) for r in GATHER_TBS},
                            fraction_of_gather_rate={f"of_{r}_TBs": round(gathered / sec / (r * 1e12), 3) for r in GATHER_TBS},
                            bits_identical_to_dot_scores_on_4_queries=same)
        print(json.dumps(rec["dense"]), flush=True)
        if a.only == "dense":
            return

    idx = ops.sparse_index_from_blocks(splade_blocks(1, N, 200), V, N=N)
    ql = ops.sparse_rows(next(splade_blocks(2, Q, 40, block=Q))[1], V)
    sparse = lambda: ops.sparse_dot_pairs(idx, *ql, cand, id_base=ID_BASE, out=out_plane)      # noqa: E731
    t = event_ms(sparse, a.reps)
    sample = ops.sparse_dot(idx, ql[0][:5].contiguous(), ql[1], ql[2])
    same = bool(torch.equal(torch.gather(sample, 1, pos[:4]).view(torch.int32), sparse()[:4].contiguous().view(torch.int32)))
    del sample
    rec["sparse"] = dict(V=V, nnz=idx.nnz, postings_per_doc=round(idx.nnz / N, 1), query_terms=round(ql[1].numel() / Q, 1), sparse_dot_pairs=t,
                         binary_searches=int(ql[1].numel()) * W, bits_identical_to_sparse_dot_on_4_queries=same)
    print(json.dumps(rec["sparse"]), flush=True)
    if a.only == "sparse":
        return

    # completion: three systems' own top-k lists over the shard, completed to depth and fused, against the fusion of the cut lists
    k = a.k
    D2, Q2 = unit_rows(N, 384, 5), unit_rows(Q, 384, 6)
    index = dict(dpr=ShardedDenseIndex(Dn, ID_BASE), splade=ShardedSparseIndex(idx, ID_BASE), dpr2=ShardedDenseIndex(D2, ID_BASE))
    query = dict(dpr=(Qn,), splade=ql, dpr2=(Q2,))
    cut = {n: RankedTopk.from_search(*index[n].search(*query[n], k)) for n in index}
    scorers = {n: (lambda U, ulen, n=n: index[n].pair_scores(*query[n], U, ulen)) for n in index}
    w = dict(dpr=0.4, splade=0.4, dpr2=0.2)
    done = Aggregator.complete_topk(cut, scorers, depth=a.depth)
    rec["complete"] = dict(S=3, k=k, depth=a.depth, union_mean=round(float(done["dpr"].lens.float().mean()), 1),
                           complete_topk=event_ms(lambda: Aggregator.complete_topk(cut, scorers, depth=a.depth), a.reps))
    for label, method, norm in (("rrf", "rrf", None), ("nsf_min-max", "nsf", "min-max")):
        rec["complete"][label] = dict(
            fuse_topk_cut_lists=event_ms(lambda: Aggregator.fuse_topk(cut, method, norm, w, {}), a.reps),
            complete_plus_fuse_topk=event_ms(lambda: Aggregator.fuse_topk(Aggregator.complete_topk(cut, scorers, depth=a.depth), method, norm, w, {}), a.reps))
    print(json.dumps(rec["complete"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
