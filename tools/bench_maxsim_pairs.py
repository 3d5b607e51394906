"""Exact ColBERT MaxSim over candidate lists (ops.maxsim_pairs, csrc/rerank.hip) at the corpus-scale shape: Q = 1024 queries of 64
tokens, k = 1000 candidates each, drawn uniformly (with repetition) from one shard of 1,105,228 passages, timed with HIP events after
warm-up, median of --reps calls -- next to two yardsticks:

  (a) the time from bytes: the token rows the candidates own (sum of their lengths x 256 B) over the 5.5-5.8 TB/s that
      MI355X_MICROARCH.md measures for whole-row register gathers from a buffer far larger than the Infinity Cache;
  (b) the only route the all-pairs kernel offers: per block of --block queries, gather the block's candidate union into a packed
      sub-corpus, ops.maxsim all pairs of the block against it, gather the wanted scores (host clock around a synchronise: the route
      synchronises by itself, torch.unique sizes its output on the host).  Its scores are compared bit for bit with the pair kernel's.

Also: ShardedTokenIndex.rerank (score + stable row sort + gathers), and rerank + Aggregator.fuse_topk of four lists (ColBERT reranking
the first system's candidates; the other three are synthetic lists as in bench_fuse_topk.py).

Passage lengths ("mMARCO-like", stated, not fitted to the data set): round(lognormal(mu = ln 62, sigma = 0.38)) + 2 marker tokens, clipped to
[8, 180] -- mean about 69 tokens, median 64, 0.3 % at the 180 cap.  Token rows are unit-norm fp16 random vectors.

Usage: python tools/bench_maxsim_pairs.py [--out profiles/r10_maxsim_pairs.json] [--only-kernel]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusion_amd import ops  # noqa: E402
from fusion_amd.distributed import ShardedTokenIndex  # noqa: E402
from fusion_amd.planes import RankedTopk  # noqa: E402
from fusion_amd.retrievers.hybrid import Aggregator  # noqa: E402

GATHER_TBS = (5.5, 5.8)      # MI355X_MICROARCH.md, 'Indexed rows: gather into LDS': whole rows into registers, far beyond the Infinity Cache
ID_BASE = 3 << 31


def make_corpus(N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(N, generator=g, device="cuda", dtype=torch.float64)
    lens = (torch.exp(np.log(62.0) + 0.38 * z).round() + 2).clamp(8, 180).long()
    Doff = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    Doff[1:] = lens.cumsum(0)
    sumL = int(Doff[-1])
    Dtok = torch.empty((sumL, 128), dtype=torch.float16, device="cuda")
    step = 1 << 22
    for lo in range(0, sumL, step):
        x = torch.randn((min(step, sumL - lo), 128), generator=g, device="cuda")
        Dtok[lo:lo + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).half()
    return Dtok, Doff, lens


def make_queries(Q, Lq, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((Q, Lq, 128), generator=g, device="cuda")
    return (x / x.norm(dim=2, keepdim=True)).half()


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


def union_route(Qtok, Dtok, Doff, lens, pos, block, max_doc_len):
    """What the all-pairs kernel alone allows: per block of queries, pack the union of its candidates and score all pairs."""
    Q, k = pos.shape
    out = torch.empty((Q, k), dtype=torch.float32, device="cuda")
    for lo in range(0, Q, block):
        hi = min(Q, lo + block)
        docs, inv = torch.unique(pos[lo:hi], return_inverse=True)
        L = lens[docs]
        off = torch.zeros(docs.numel() + 1, dtype=torch.int64, device="cuda")
        off[1:] = L.cumsum(0)
        rows = torch.arange(int(off[-1]), device="cuda") + torch.repeat_interleave(Doff[docs] - off[:-1], L)
        plane = ops.maxsim(Qtok[lo:hi], Dtok[rows], off, max_doc_len=max_doc_len)
        out[lo:hi] = torch.gather(plane, 1, inv)
    return out


def other_systems(S, Q, k, N, seed):
    """S lists of k distinct ids per query (bench_fuse_topk.py's scheme over this shard's ids)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    pool = int(k * (1 + S / 2))
    off = torch.randint(0, N, (Q, 1), generator=g, device="cuda")
    systems = {}
    for s in range(S):
        pick = torch.rand((Q, pool), generator=g, device="cuda").argsort(1)[:, :k]
        ids = (pick * 1009 + off) % N + ID_BASE
        sc = (torch.rand((Q, k), generator=g, device="cuda") * 1.1 - 0.2).sort(dim=1, descending=True, stable=True).values.contiguous()
        systems[f"s{s}"] = RankedTopk(ids=ids.contiguous(), scores=sc, lens=torch.full((Q,), k, dtype=torch.int32, device="cuda"))
    return systems


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--lq", type=int, default=64)
    ap.add_argument("--docs", type=int, default=1_105_228)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--block", default="16,32", help="query block sizes of the union route (the best is reported as the yardstick)")
    ap.add_argument("--only-kernel", action="store_true", help="the pair kernel alone, --reps calls (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r10_maxsim_pairs.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_maxsim_pairs.py measures on the GPU: no device found")
    Q, k, Lq, N = a.queries, a.k, a.lq, a.docs
    Dtok, Doff, lens = make_corpus(N, 1)
    Qtok = make_queries(Q, Lq, 2)
    pos = torch.randint(0, N, (Q, k), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    cand = pos + ID_BASE
    max_doc_len = 180
    out_plane = ops.alloc_plane(Q, k, torch.float32, "cuda")
    kernel = lambda: ops.maxsim_pairs(Qtok, Dtok, Doff, cand, id_base=ID_BASE, max_doc_len=max_doc_len, out=out_plane)      # noqa: E731
    if a.only_kernel:
        print(json.dumps(dict(maxsim_pairs=event_ms(kernel, a.reps))))
        return

    tokens = int(lens[pos].sum())
    gathered = tokens * 256
    flops = 2.0 * tokens * Lq * 128
    t = event_ms(kernel, a.reps)
    sec = t["median_ms"] * 1e-3
    rec = dict(
        what="exact MaxSim over candidate lists (fz_maxsim_pairs_f16): HIP events, median of %d calls after 3 warm-up calls; the union route by the "
             "host clock around a synchronise, median of 3 passes over all queries" % a.reps,
        device=torch.cuda.get_device_properties(0).name, Q=Q, k=k, Lq=Lq, docs=N, corpus_tokens=int(Doff[-1]), corpus_GB=round(int(Doff[-1]) * 256 / 1e9, 2),
        lengths=dict(distribution="round(lognormal(ln 62, 0.38)) + 2, clipped to [8, 180]", mean=round(float(lens.float().mean()), 2),
                     median=int(lens.median()), max=int(lens.max())),
        candidates="uniform over the shard, with repetition", candidate_tokens=tokens, gathered_GB=round(gathered / 1e9, 3), TFLOP=round(flops / 1e12, 3),
        maxsim_pairs=t, achieved_TBs=round(gathered / sec / 1e12, 3), achieved_PFLOPs=round(flops / sec / 1e15, 4),
        time_from_bytes_ms={f"at_{r}_TBs": round(gathered / (r * 1e12) * 1e3, 4) for r in GATHER_TBS},
        fraction_of_gather_rate={f"of_{r}_TBs": round(gathered / sec / (r * 1e12), 3) for r in GATHER_TBS})
    print(json.dumps(rec), flush=True)

    # (b) the union route on the all-pairs kernel
    got = kernel().clone()
    rec["union_route"] = {}
    for block in (int(x) for x in a.block.split(",")):
        ref = union_route(Qtok, Dtok, Doff, lens, pos, block, max_doc_len)      # warm-up + the comparison
        same = bool(torch.equal(ref.view(torch.int32), got.view(torch.int32)))
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            union_route(Qtok, Dtok, Doff, lens, pos, block, max_doc_len)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        rec["union_route"][f"block_{block}"] = dict(median_ms=round(float(np.median(times)), 2), min_ms=round(min(times), 2), max_ms=round(max(times), 2),
                                                    bits_identical_to_maxsim_pairs=same)
    best = min(v["median_ms"] for v in rec["union_route"].values())
    rec["union_route_best_ms"] = best
    rec["speedup_vs_union_route"] = round(best / t["median_ms"], 1)
    print(json.dumps(rec["union_route"]), flush=True)

    # rerank, and rerank + fusion of four lists
    index = ShardedTokenIndex(Dtok, Doff, ID_BASE, max_doc_len=max_doc_len)
    rec["rerank_uniform_candidates"] = event_ms(lambda: index.rerank(Qtok, cand), a.reps)
    systems = other_systems(3, Q, k, N, 4)
    names = ("dpr", "splade", "bm25")
    systems = {n: s for n, s in zip(names, systems.values())}
    weights = {"dpr": 0.25, "splade": 0.25, "bm25": 0.25, "colbert": 0.25}

    def four(method, norm):
        lists = dict(systems, colbert=index.rerank(Qtok, systems["dpr"]))
        return Aggregator.fuse_topk(lists, method, norm, weights, {})
    rec["rerank_dpr_candidates"] = event_ms(lambda: index.rerank(Qtok, systems["dpr"]), a.reps)
    rec["rerank_plus_fuse_topk_4_lists"] = {"rrf": event_ms(lambda: four("rrf", None), a.reps), "nsf_min-max": event_ms(lambda: four("nsf", "min-max"), a.reps)}
    only = dict(systems, colbert=index.rerank(Qtok, systems["dpr"]))
    rec["fuse_topk_4_lists_alone"] = {"rrf": event_ms(lambda: Aggregator.fuse_topk(only, "rrf", None, weights, {}), a.reps),
                                      "nsf_min-max": event_ms(lambda: Aggregator.fuse_topk(only, "nsf", "min-max", weights, {}), a.reps)}
    rec["fused_union_mean"] = round(float(four("rrf", None).lens.float().mean()), 1)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
