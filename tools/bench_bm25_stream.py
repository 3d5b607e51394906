"""BM25 top-k at corpus scale: the streamed route of TFIDF.search_topk (exact head, then the posting walk with the float64 threshold filter as
its epilogue, ops.TopkStream64) against the plane route (the whole [q, N] float64 plane, cut by the row sort) on the same index, in the same
process, alternating.  Corpus: retrievers.bm25.load_data's synthetic recipe (5,000 Zipf-distributed words, documents of 20-200 words),
drawn in one vectorised pass; Q = 256, k = 1000.  N is whatever --docs says: the index is built on the host (a Python pass over every
token), which is what bounds it -- the N used and the build time are in the output.

Usage: python tools/bench_bm25_stream.py [--docs 200000] [--queries 256] [--k 1000] [--reps 5] [--out profiles/r11_bm25_stream.json]
One process; run it under a time limit.  Times are host clocks around work that ends in a device synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusion_amd.retrievers.bm25 import BM25  # noqa: E402


def zipf_text(rng, n, lo, hi, vocab_size=5000):
    vocab = np.array([f"mot{i}" for i in range(vocab_size)])
    p = 1.0 / np.arange(1, vocab_size + 1); p /= p.sum()
    sizes = rng.integers(lo, hi, n)
    words = rng.choice(vocab, size=int(sizes.sum()), p=p)
    return [" ".join(w) for w in np.split(words, np.cumsum(sizes)[:-1])]


def once(f):
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def mark_split(model, queries, k, streaming):
    """One instrumented (untimed) run: device time between consecutive marks, summed per mark name."""
    ev = [("start", torch.cuda.Event(enable_timing=True))]
    ev[0][1].record()

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        ev.append((name, e))
    model._topk_device(queries, k, streaming=streaming, mark=mark)
    torch.cuda.synchronize()
    split = {}
    for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
        split[name] = split.get(name, 0.0) + a.elapsed_time(b)
    return {n: round(v, 3) for n, v in split.items()}, len(ev) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r11_bm25_stream.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU path"
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    docs = zipf_text(rng, a.docs, 20, 200)
    queries = zipf_text(rng, a.queries, 4, 16)
    text_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    m = BM25(docs, 1.5, 0.75)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    runs = {"stream": lambda: m.search_topk(queries, a.k, streaming=True), "plane": lambda: m.search_topk(queries, a.k, streaming=False)}
    results, paths = {}, {}
    for name, f in runs.items():                      # warm-up of every shape the timed window uses (code objects, allocator)
        _, results[name] = once(f)
        paths[name] = m.last_path
        once(f)
    redone = None
    times = {name: [] for name in runs}
    for _ in range(a.reps):                           # alternating, so that drift on a shared host hits both alike
        for name, f in runs.items():
            ms, _ = once(f)
            times[name].append(ms)
            if name == "stream":
                redone = m.last_overflow
    same = all(bool(torch.equal(getattr(results["stream"], f), getattr(results["plane"], f))) for f in ("ids", "scores64", "scores", "lens"))
    split_s, launches_s = mark_split(m, queries, a.k, True)
    split_p, launches_p = mark_split(m, queries, a.k, False)
    summ = {n: dict(min_ms=round(min(t), 2), median_ms=round(float(np.median(t)), 2), max_ms=round(max(t), 2), all_ms=[round(x, 2) for x in t])
            for n, t in times.items()}
    faster = summ["stream"]["max_ms"] < summ["plane"]["min_ms"]
    out = dict(what="BM25 search_topk: streamed (posting walk + float64 top-k filter epilogue, TopkStream64) vs plane route (whole score plane + "
                    "hierarchical row-sort cut)", device=torch.cuda.get_device_properties(0).name, N=a.docs, Q=a.queries, k=a.k,
               postings=int(m.pdoc.numel()), vocabulary=len(m.vocab), corpus_text_s=round(text_s, 1), index_build_s=round(build_s, 1),
               head_docs=m.head_docs(a.k), chunk_docs=m.CHUNK, cap=m.CAP, paths=paths, times=summ,
               speedup_median=round(summ["plane"]["median_ms"] / summ["stream"]["median_ms"], 3),
               stream_faster_beyond_spread=bool(faster), windows_redone=redone, lists_identical=same,
               marks_stream_ms=split_s, marks_plane_ms=split_p, mark_calls=dict(stream=launches_s, plane=launches_p),
               timing=f"{a.reps} alternating repeats after two warm-up runs each; host clock around a device synchronise")
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
