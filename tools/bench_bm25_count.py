#!/usr/bin/env python3
"""BM25's k1 x b grid search beyond one sort row: gold ranks counted on the posting walk (BM25.tune(counting=True), csrc/bm25_count.hip)
against the plane route (counting=False: the [q, N] float64 plane per pair, cut to its first top_k entries, searched for the golds).
A synthetic stop-word-free corpus of tools/bench_bm25_tune.py's kind at N just above one float64 sort row and at about 1.1 M documents,
Q = 1024, a small (k1, b) grid; the two routes alternated call by call in one process, medians with the maximum alongside; the returned
dicts are compared.  Also the count launch alone against the plane launch of the same range of documents.
Usage: python tools/bench_bm25_count.py [out.json] [Q] [N_large]      (default profiles/r19_bm25_count.json)"""
import json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fusion_amd import ops
from fusion_amd.retrievers.bm25 import BM25

K1S, BS, TOP_K, REPS = [0.9, 1.5, 2.0], [0.4, 0.6, 0.75], 1000, 5


def corpus(rng, N, Q, V=30000, mean_len=40):
    p = 1.0 / np.arange(30, V + 30) ** 1.05; p /= p.sum()          # a Zipf vocabulary WITHOUT its 30 most frequent (stop-word-like) ranks
    vocab = np.array([f"m{i}" for i in range(V)])
    lens = np.clip(rng.normal(mean_len, mean_len / 3, N), 8, 128).astype(np.int64)
    toks = vocab[rng.choice(V, size=int(lens.sum()), p=p)]
    off = np.concatenate([[0], np.cumsum(lens)])
    docs = [" ".join(toks[off[i]:off[i + 1]]) for i in range(N)]
    queries = [" ".join(vocab[rng.choice(V, size=int(rng.integers(4, 12)), p=p)]) for _ in range(Q)]
    gold = [sorted(rng.choice(N, size=int(rng.integers(1, 5)), replace=False).tolist()) for _ in range(Q)]
    return docs, queries, gold


def wall_ms(f):
    torch.cuda.synchronize(); t = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def stats(xs):
    return dict(median_ms=round(statistics.median(xs), 3), max_ms=round(max(xs), 3), runs=len(xs))


def one_size(N, Q):
    rng = np.random.default_rng(N)
    docs, queries, gold = corpus(rng, N, Q)
    t0 = time.perf_counter(); m = BM25(docs, K1S[0], BS[0]); torch.cuda.synchronize()
    res = dict(N=N, Q=Q, pairs=len(K1S) * len(BS), top_k=TOP_K, postings=int(m.pdoc.numel()), index_build_s=round(time.perf_counter() - t0, 2),
               slice_table=m.slice_off is not None)
    kw = dict(k1_range=K1S, b_range=BS, top_k=TOP_K)
    want = m.tune(queries, gold, counting=False, **kw)             # warm-up of both routes, and the results to compare
    got = m.tune(queries, gold, counting=True, **kw)
    assert m.last_tune_path == "count"
    res["same_dicts"] = got == want
    times = {True: [], False: []}
    for _ in range(REPS):
        for counting in (True, False):                             # alternated call by call
            times[counting].append(wall_ms(lambda: m.tune(queries, gold, counting=counting, **kw))[0])
    res["tune_counting"], res["tune_plane"] = stats(times[True]), stats(times[False])
    res["per_pair_ms"] = dict(counting=round(res["tune_counting"]["median_ms"] / res["pairs"], 3), plane=round(res["tune_plane"]["median_ms"] / res["pairs"], 3))
    # one launch: the count epilogue against the plane epilogue over the same documents (one feed of the streamed routes, whole slices)
    Qb = min(Q, m.STREAM_QUERIES)
    qoff, flat = m._query_csr(queries[:Qb])
    pval, _ = m.lexical_tables()
    hi = min(N, ops.stream_chunk(m.CHUNK, ops.lexical_slice_docs("pv")))
    G = 4
    gs = torch.rand((Qb, G), dtype=torch.float64, device="cuda") * 8
    gi = torch.randint(0, N, (Qb, G), dtype=torch.int64, device="cuda")
    counts = torch.zeros((Qb, G), dtype=torch.int32, device="cuda")
    launch = {
        "count": lambda: ops.lexical_count("pv", m.toff, m.pdoc, pval, None, qoff, flat, Qb, N, 0, hi, 0, gs, gi, counts, slice_off=m.slice_off),
        "plane": lambda: ops.bm25_scores_range(m.toff, m.pdoc, pval, qoff, flat, Qb, N, 0, hi, slice_off=m.slice_off),
    }
    lt = {k: [] for k in launch}
    for f in launch.values():
        f()
    for _ in range(4 * REPS):
        for k, f in launch.items():
            lt[k].append(wall_ms(f)[0])
    res["one_launch"] = dict(docs=hi, Q=Qb, G=G, count=stats(lt["count"]), plane=stats(lt["plane"]))
    del m
    torch.cuda.empty_cache()
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r19_bm25_count.json")
    Q = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    N_large = int(sys.argv[3]) if len(sys.argv) > 3 else 1_105_228
    if not torch.cuda.is_available():
        raise SystemExit("bench_bm25_count: needs the GPU (no CPU path)")
    W = ops.sort_max_n(torch.float64)
    res = dict(device=torch.cuda.get_device_name(0), sort_row=W, grid=dict(k1=K1S, b=BS), sizes=[])
    for N in (W + 17, N_large):
        res["sizes"].append(one_size(N, Q))
        print(json.dumps(res["sizes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
