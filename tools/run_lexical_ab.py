#!/usr/bin/env python3
"""The lexical range walk A/B on one device: lexical_range_kernel's six instantiations (posting values / TF-IDF x plane / filter / count) in
the shipped library against another build of it (the parent commit's), both loaded into ONE process and swapped under fusion_amd._lib call
by call -- other, shipped, other again per repeat, so the other build's two series give its own spread.  Index and queries:
tools/bench_bm25_stream.py's (Zipf text, 20-200 words per document), one launch over the first min(N, CHUNK) documents per call; the
filter's thresholds are each row's k-th best score (a settled stream), the golds' scores their documents' own.  HIP events around INNER
calls; outputs of the two builds compared bit for bit (candidates as sorted id rows: they arrive in no order).
Usage: python tools/run_lexical_ab.py other.so [--docs 200000] [--queries 256] [--reps 15] [--out profiles/r27_lexical_walk_ab.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fusion_amd import _lib, ops  # noqa: E402
from fusion_amd.retrievers.bm25 import BM25  # noqa: E402
from tools.bench_bm25_stream import zipf_text  # noqa: E402

INNER, K, G = 5, 1000, 4


def load(path):
    L = C.CDLL(path)
    for name, (res, args) in _lib._PROTOS.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    assert L.fz_abi_version() == _lib.ABI_VERSION
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_lexical_walk_ab.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU path"
    libs = {"shipped": _lib.lib(), "other": load(os.path.abspath(a.other))}
    rng = np.random.default_rng(0)
    m = BM25(zipf_text(rng, a.docs, 20, 200), 1.5, 0.75)
    queries = zipf_text(rng, a.queries, 4, 16)
    qoff, flat = m._query_csr(queries)
    Q, N, dev = a.queries, m.corpus_size, m.toff.device
    tables = {"pv": m.lexical_tables(), "tfidf": (m.ptf, m.idf)}
    gi = torch.randint(0, N, (Q, G), dtype=torch.int64, device=dev)
    out = dict(what="lexical_range_kernel<MODE, EPI>, one launch per call: the shipped build against the other (parent) build in one process",
               device=torch.cuda.get_device_properties(0).name, N=N, Q=Q, postings=int(m.pdoc.numel()), golds=G, cap=m.CAP,
               timing=f"{a.reps} repeats of (other, shipped, other) after a warm-up of each; HIP events around {INNER} calls, ms per call",
               routes={})
    for mode, (vals, idf) in tables.items():
        hi = min(N, ops.stream_chunk(m.CHUNK, ops.lexical_slice_docs(mode)))
        common = (mode, m.toff, m.pdoc, vals, idf, qoff, flat, Q, N)
        plane = ops.lexical_scores_range(*common, 0, hi, slice_off=m.slice_off)
        tau = torch.topk(plane, K, dim=1).values[:, -1].contiguous()
        gs = torch.gather(plane, 1, gi.clamp(max=hi - 1)).contiguous()
        del plane
        cand_s = torch.empty((Q, m.CAP), dtype=torch.float64, device=dev)
        cand_i = torch.empty((Q, m.CAP), dtype=torch.int64, device=dev)
        cand_len = torch.zeros(Q, dtype=torch.int32, device=dev)
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        counts = torch.zeros((Q, G), dtype=torch.int32, device=dev)

        def run_plane():
            return (ops.lexical_scores_range(*common, 0, hi, slice_off=m.slice_off),)

        def run_filter():
            cand_len.zero_()                                          # (a full row stores nothing more: every call starts empty)
            ops.lexical_filter(*common, 0, hi, 0, tau, cand_s, cand_i, cand_len, overflow, slice_off=m.slice_off)

        def check_filter():
            cand_i.fill_(-1)
            run_filter()
            return cand_len.clone(), torch.sort(cand_i, dim=1).values, overflow.clone()

        def run_count():
            ops.lexical_count(*common, 0, hi, 0, gs, gi, counts, slice_off=m.slice_off)

        def check_count():
            counts.zero_()
            run_count()
            return (counts.clone(),)

        for route, f, check in (("plane", run_plane, run_plane), ("filter", run_filter, check_filter), ("count", run_count, check_count)):
            got = {}
            for name, L in libs.items():                              # warm-up, and the outputs to compare
                _lib._lib = L
                got[name] = check()
            same = all(bool(torch.equal(x, y)) for x, y in zip(got["shipped"], got["other"]))
            del got
            ms = {"other_a": [], "shipped": [], "other_b": []}
            for _ in range(a.reps):
                for series in ms:
                    _lib._lib = libs[series.split("_")[0]]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(INNER):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[series].append(round(e0.elapsed_time(e1) / INNER, 4))
            _lib._lib = libs["shipped"]
            other = ms["other_a"] + ms["other_b"]
            med = {s: round(statistics.median(x), 4) for s, x in ms.items()}
            rec = dict(docs=hi, same_bits=same, runs_ms=ms, median_ms=dict(med, other=round(statistics.median(other), 4)),
                       other_range_ms=[min(other), max(other)], shipped_range_ms=[min(ms["shipped"]), max(ms["shipped"])],
                       other_against_itself_ms=round(abs(med["other_a"] - med["other_b"]), 4),
                       shipped_minus_other_ms=round(med["shipped"] - statistics.median(other), 4))
            out["routes"][f"{mode}_{route}"] = rec
            print(json.dumps({f"{mode}_{route}": {k: v for k, v in rec.items() if k != "runs_ms"}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
