"""Corpus-scale SPLADE search: the fused path (distributed.ShardedSparseIndex.local_topk -- exact head, then the posting walk with the top-k
filter as its epilogue, fz_sparse_dot_filter_f32) against the two-pass path (per chunk a score plane from fz_sparse_dot_range_f32, its top-k,
a merge) on the same synthetic SPLADE-shaped index: ~200 Zipf-distributed terms of 32,005 per document, ~40 per query (bench.splade_like's
shape, generated on the device block by block -- the corpus is never one dense matrix), Q = 1024, k = 1000.

Usage: python tools/bench_splade_search.py [--sizes 1105228,8841823] [--out profiles/r07_splade_search.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusion_amd import ops  # noqa: E402
from fusion_amd.distributed import ShardedSparseIndex  # noqa: E402

V = 32005


def splade_blocks(seed, N, nnz, block=8192, normalise=True):
    """(doc_base, rows) blocks of L2-normalised SPLADE-shaped vectors: ~nnz terms per row drawn from a Zipf(0.9) law over the vocabulary,
    weights log1p(max(N(1, 1), 0.05)) -- bench.splade_like's distribution, drawn with the device's generator."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = 1.0 / torch.arange(1, V + 1, device="cuda", dtype=torch.float64) ** 0.9
    p = (p / p.sum()).float()
    for r0 in range(0, N, block):
        n = min(block, N - r0)
        k = torch.poisson(torch.full((n,), float(nnz), device="cuda"), generator=g).clamp_(min=1).long()
        width = int(k.max())
        cols = torch.multinomial(p, n * width, replacement=True, generator=g).view(n, width)
        w = torch.log1p(torch.clamp(torch.randn((n, width), generator=g, device="cuda") + 1.0, min=0.05))
        w = torch.where(torch.arange(width, device="cuda")[None, :] < k[:, None], w, torch.zeros_like(w))   # row i keeps k[i] draws
        X = torch.zeros((n, -(-V // 4) * 4), device="cuda")
        X.scatter_reduce_(1, cols, w, reduce="amax")
        yield r0, (ops.normalize_rows(X) if normalise else X)


def timed(f, reps):
    f()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def window_stats(shard, ql, k):
    """One instrumented (untimed) fused run: candidates per window at every fold (cand_len read before the fold), folds, windows redone."""
    cands = []
    orig = ops.TopkStream.fold

    def fold(self):
        if self.pending:
            c = self.cand_len.float()
            cands.append(dict(docs=int(self.pending), mean=round(float(c.mean()), 1), max=int(c.max())))
        orig(self)
    ops.TopkStream.fold = fold
    try:
        shard.local_topk(*ql, k)
    finally:
        ops.TopkStream.fold = orig
    return cands, shard.last_overflow


def run(N, Q, k, reps):
    t0 = time.perf_counter()
    idx = ops.sparse_index_from_blocks(splade_blocks(1, N, 200), V, N=N)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    Qn = next(splade_blocks(2, Q, 40, block=Q))[1]
    ql = ops.sparse_rows(Qn, V)
    shard = ShardedSparseIndex(idx, 0)
    fused_ms = timed(lambda: shard.local_topk(*ql, k), reps)
    two_ms = timed(lambda: shard.two_pass_topk(ql, k), reps)
    f_s, f_i = shard.local_topk(*ql, k)
    t_s, t_i = shard.two_pass_topk(ql, k)
    cands, redone = window_stats(shard, ql, k)
    index_bytes = sum(t.numel() * t.element_size() for t in (idx.toff, idx.pdoc, idx.pw, idx.slice_off))
    res = dict(N=N, Q=Q, k=k, V=V, nnz=idx.nnz, postings_per_doc=round(idx.nnz / N, 1), query_terms=round(ql[1].numel() / Q, 1),
               index_bytes=index_bytes, index_build_s=round(build_s, 2), head_docs=shard.head_docs(k), chunk_docs=shard.CHUNK, cap=shard.CAP,
               fused_ms=round(fused_ms, 2), two_pass_ms=round(two_ms, 2), fused_ms_per_1024q=round(fused_ms * 1024 / Q, 2),
               two_pass_ms_per_1024q=round(two_ms * 1024 / Q, 2), speedup=round(two_ms / fused_ms, 3),
               two_pass_plane_bytes_per_chunk=Q * ops.round_up(shard.CHUNK, 64) * 4, folds=len(cands), windows_redone=redone,
               candidates_per_window=cands, identical=bool(torch.equal(f_s, t_s) and torch.equal(f_i, t_i)), timing="best of %d, after one warm-up" % reps)
    print(json.dumps(res), flush=True)
    del idx, shard
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1105228,8841823")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07_splade_search.json"))
    a = ap.parse_args()
    dev = torch.cuda.get_device_properties(0)
    out = dict(what="SPLADE top-k search over an inverted index: fused (posting walk + top-k filter epilogue) vs two-pass (score plane per chunk, "
                    "top-k, merge)", device=dev.name, runs=[])
    for N in (int(x) for x in a.sizes.split(",")):
        out["runs"].append(run(N, a.queries, a.k, a.reps))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
