"""Pair scores through the forward (document-major) index against the inverted route, at the corpus-scale shape of
profiles/r20_pair_scores.json: Q = 1024 queries, W = 3,000 candidates each, uniform (with repetition) over one shard.  Both routes run in
ONE process, alternated call by call; HIP events, median of --reps calls per route after 3 warm-up calls each.

  sparse    the SPLADE-shaped shard of tools/bench_splade_search.py (1,105,228 passages, ~166 postings each; ~37 terms per query):
            ops.sparse_dot_pairs(route='forward') -- fz_sparse_fwd_pairs_f32, a gather of 8-byte posting rows -- against route='inverted';
            milliseconds and gathered row bytes per second, next to the 5.5 TB/s MI355X_MICROARCH.md measures for random whole rows.
  complete  Aggregator.complete_topk for the S = 3 configuration of r20 (dense d = 768, sparse, dense d = 384; depth 2,730) with the
            sparse shard's forward index and without it.
  lexical   BM25.doc_scores at Q = 1024, G = 3,000 uniform positions on the index of tools/bench_bm25_stream.py, both routes.

The decision the numbers feed ('Forward index'): route=None may prefer the sparse forward route only if it takes at most half the
inverted route's time here; the lexical default follows the faster route beyond the run's spread.

Usage: python tools/bench_forward_pairs.py [--out profiles/rNN_forward_pairs.json] [--only sparse|complete|lexical]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fusion_amd import ops  # noqa: E402
from fusion_amd.distributed import ShardedDenseIndex, ShardedSparseIndex  # noqa: E402
from fusion_amd.planes import RankedTopk  # noqa: E402
from fusion_amd.retrievers.bm25 import BM25  # noqa: E402
from fusion_amd.retrievers.hybrid import Aggregator  # noqa: E402
from bench_bm25_stream import zipf_text  # noqa: E402
from bench_pair_scores import ID_BASE, unit_rows  # noqa: E402
from bench_splade_search import V, splade_blocks  # noqa: E402

GATHER_TBS = 5.5      # MI355X_MICROARCH.md, 'Indexed rows: gather into LDS': random 1,152-byte rows into registers, each fetched once


def next_profile() -> str:
    taken = [int(m.group(1)) for f in os.listdir(os.path.join(ROOT, "profiles")) if (m := re.match(r"r(\d+)_", f))]
    return os.path.join(ROOT, "profiles", f"r{max(taken, default=0) + 1:02d}_forward_pairs.json")


def alternate_ms(runs: dict, reps: int, warm: int = 3) -> dict:
    """{name: f} -> {name: times}: every f warmed, then the routes in turn, call by call, so that drift on a shared machine hits all alike"""
    for f in runs.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in runs}
    for _ in range(reps):
        for n, f in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b))
    return {n: dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(np.min(t)), 4), max_ms=round(float(np.max(t)), 4), reps=reps)
            for n, t in times.items()}


def same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int64),
                            b.contiguous().view(torch.int32 if b.element_size() == 4 else torch.int64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--width", type=int, default=3000)
    ap.add_argument("--docs", type=int, default=1_105_228)
    ap.add_argument("--lexical-docs", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--depth", type=int, default=2730)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", choices=("sparse", "complete", "lexical"))
    ap.add_argument("--out", default=None, help="default: the next free profiles/rNN_forward_pairs.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_forward_pairs.py measures on the GPU: no device found")
    Q, W, N = a.queries, a.width, a.docs
    rec = dict(what="pair scores through the forward index against the inverted route, alternated call by call in one process: HIP events, "
                    "median of %d calls per route after 3 warm-up calls" % a.reps,
               device=torch.cuda.get_device_properties(0).name, Q=Q, W=W, candidates="uniform over the shard, with repetition")

    if a.only in (None, "sparse", "complete"):
        pos = torch.randint(0, N, (Q, W), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
        cand = pos + ID_BASE
        idx = ops.sparse_index_from_blocks(splade_blocks(1, N, 200), V, N=N)
        ql = ops.sparse_rows(next(splade_blocks(2, Q, 40, block=Q))[1], V)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fwd = idx.build_forward()
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
    if a.only in (None, "sparse"):
        outs = {r: ops.alloc_plane(Q, W, torch.float32, "cuda") for r in ("forward", "inverted")}
        t = alternate_ms({r: (lambda r=r: ops.sparse_dot_pairs(idx, *ql, cand, id_base=ID_BASE, out=outs[r], route=r)) for r in outs}, a.reps)
        n_rows = fwd.foff[1:] - fwd.foff[:-1]
        gathered = int(n_rows[pos].sum()) * 8
        sec = t["forward"]["median_ms"] * 1e-3
        ratio = t["forward"]["median_ms"] / t["inverted"]["median_ms"]
        rec["sparse"] = dict(docs=N, V=V, nnz=idx.nnz, postings_per_doc=round(idx.nnz / N, 1), longest_row=int(n_rows.max()),
                             query_terms=round(ql[1].numel() / Q, 1), forward_index_bytes=fwd.nbytes,
                             inverted_index_bytes=idx.nnz * 8 + (V + 1) * 8, forward_build_s=round(build_s, 2), sparse_dot_pairs=t,
                             gathered_GB=round(gathered / 1e9, 3), achieved_TBs=round(gathered / sec / 1e12, 3),
                             time_from_bytes_ms_at_5p5_TBs=round(gathered / (GATHER_TBS * 1e12) * 1e3, 4),
                             forward_over_inverted=round(ratio, 4), at_most_half_the_inverted_time=bool(ratio <= 0.5),
                             routes_bit_identical=same_bits(outs["forward"], outs["inverted"]))
        print(json.dumps(rec["sparse"]), flush=True)

    if a.only in (None, "complete"):
        k = a.k
        Dn, Qn, D2, Q2 = unit_rows(N, 768, 1), unit_rows(Q, 768, 2), unit_rows(N, 384, 5), unit_rows(Q, 384, 6)
        index = dict(dpr=ShardedDenseIndex(Dn, ID_BASE), splade=ShardedSparseIndex(idx, ID_BASE), dpr2=ShardedDenseIndex(D2, ID_BASE))
        query = dict(dpr=(Qn,), splade=ql, dpr2=(Q2,))
        cut = {n: RankedTopk.from_search(*index[n].search(*query[n], k)) for n in index}
        scorers = {n: (lambda U, ulen, n=n: index[n].pair_scores(*query[n], U, ulen)) for n in index}
        keep = ops.SPARSE_PAIRS_PREFER_FORWARD
        ops.SPARSE_PAIRS_PREFER_FORWARD = True           # so that the index's forward index alone decides the route, through the real surface

        def complete(with_forward):
            idx.forward = fwd if with_forward else None
            return Aggregator.complete_topk(cut, scorers, depth=a.depth)
        try:
            done = {w: complete(w) for w in (True, False)}
            t = alternate_ms({"with_forward": lambda: complete(True), "without_forward": lambda: complete(False)}, a.reps)
        finally:
            ops.SPARSE_PAIRS_PREFER_FORWARD, idx.forward = keep, fwd
        same = all(bool(torch.equal(done[True][n].ids, done[False][n].ids)) and same_bits(done[True][n].scores, done[False][n].scores) for n in index)
        rec["complete"] = dict(S=3, k=k, depth=a.depth, union_mean=round(float(done[True]["dpr"].lens.float().mean()), 1), complete_topk=t,
                               lists_bit_identical=same)
        print(json.dumps(rec["complete"]), flush=True)
        del Dn, D2, index, cut, done

    if a.only in (None, "lexical"):
        rng = np.random.default_rng(0)
        docs = zipf_text(rng, a.lexical_docs, 20, 200)
        queries = zipf_text(rng, Q, 4, 16)
        m = BM25(docs, 1.5, 0.75)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = m.build_forward()
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        lpos = torch.randint(0, a.lexical_docs, (Q, W), generator=torch.Generator(device="cuda").manual_seed(4), device="cuda")
        got = {}

        def run(route):
            got[route] = m.doc_scores(queries, lpos, route=route)
        t = alternate_ms({r: (lambda r=r: run(r)) for r in ("forward", "inverted")}, a.reps)
        lo, hi = sorted((t["forward"], t["inverted"]), key=lambda x: x["median_ms"])
        rec["lexical"] = dict(model="BM25(1.5, 0.75), posting values", docs=a.lexical_docs, G=W, postings=int(m.pdoc.numel()), vocabulary=len(m.vocab),
                              postings_per_doc=round(m.pdoc.numel() / a.lexical_docs, 1), query_terms=round(float(np.mean([len(q.split()) for q in queries])), 1),
                              forward_index_bytes=f.nbytes, forward_build_s=round(build_s, 2), doc_scores=t,
                              forward_over_inverted=round(t["forward"]["median_ms"] / t["inverted"]["median_ms"], 4),
                              faster_beyond_spread=bool(lo["max_ms"] < hi["min_ms"]), routes_bit_identical=same_bits(got["forward"], got["inverted"]))
        print(json.dumps(rec["lexical"]), flush=True)

    out = a.out or next_profile()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print("wrote", out, flush=True)


if __name__ == "__main__":
    main()
