#!/usr/bin/env python
"""tests/golden/topkfuse_*.npz: the reference's Aggregator.fuse on TOP-K-SHAPED lists -- what the corpus-scale searches return:
k entries per query and system over arbitrary int64 global ids -- in the key layout of the fuse_*.npz fixtures
(oracle/gen_golden.py: gen_fuse), through the same loader and packers.

    python tools/gen_golden_topk.py [--out DIR]       (default: tests/golden; needs the reference tree, FUSION_REFERENCE)

One addition to the layout: `raises` lists the "<method>__<normalisation>" pairs for which the reference RAISED on the case
(min-max on an empty list: min() of an empty tensor).  No output is stored for those; the tests hold them to the project's own
rule instead -- an empty list contributes nothing (oracle.fuse_lists).

Cases: S in {1, 2, 3, 4, 8}; k in {1, 10, 1000} mixed inside a case; ids from [0, 2^40) with many above 2^32 and one equal to
2^62; id sets that are disjoint, identical in different orders, and ~30 % overlapping; lists shorter than k, empty lists, a query
where every list is empty; exact score ties inside and across systems; a BM25-like system whose tail is exact zeros; a
single-entry list (its z-score is NaN).
"""
from __future__ import annotations

import argparse
import copy
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.gen_golden import METHODS, load_reference, pack_lists, pack_out, synth_system_scores   # noqa: E402

KINDS = ["bm25", "dpr", "splade", "colbert"]
BIG_ID = 1 << 62

# name, seed, per-system k, Q, how the id sets of a query relate, {(system, query): list length} overrides (default: k)
CASES = [
    ("S1_Q3_single", 50, [10], 3, "overlap", {(0, 1): 1, (0, 2): 7}),
    ("S2_Q4_sets", 51, [10, 10], 4, "by_query", {}),
    ("S3_Q4_kmix", 52, [1000, 10, 1], 4, "overlap", {(0, 1): 640, (1, 2): 3}),
    ("S4_Q4_empty", 53, [10, 1000, 10, 1], 4, "overlap", {(0, 0): 0, (1, 1): 0, (2, 1): 4, (0, 2): 0, (1, 2): 0, (2, 2): 0, (3, 2): 0}),
    ("S8_Q2_kmix", 54, [1000, 10, 1, 1000, 10, 1, 10, 10], 2, "overlap", {(3, 1): 500}),
]


def draw_ids(rng, count):
    """`count` distinct ids: half below 2^33 (some below 2^32), half up to 2^40."""
    got: dict = {}
    while len(got) < count:
        hi = 1 << (33 if len(got) % 2 else 40)
        got[int(rng.integers(0, hi))] = None
    return list(got)


def system_names(S):
    return [KINDS[s] if s < 4 else f"sys{s}" for s in range(S)]


def make_case(seed, ks, Q, mode, lens):
    rng = np.random.default_rng(seed)
    S = len(ks)
    names = system_names(S)
    kmax = max(ks)
    lists = {n: [] for n in names}
    for q in range(Q):
        n_of = [lens.get((s, q), ks[s]) for s in range(S)]
        m = mode if mode != "by_query" else ["disjoint", "identical", "overlap", "disjoint"][q % 4]
        if m == "disjoint":
            pool = draw_ids(rng, sum(n_of))
            cut = np.cumsum([0] + n_of)
            chosen = [pool[cut[s]:cut[s + 1]] for s in range(S)]
        elif m == "identical":
            pool = draw_ids(rng, max(n_of))
            chosen = [[pool[i] for i in rng.permutation(len(pool))[:n_of[s]]] for s in range(S)]
        else:   # every system samples its ids from a universe 1 / 0.3 times its own size: about 30 % of a list is in another one
            pool = draw_ids(rng, max(int(kmax / 0.3), 4))
            chosen = [[pool[i] for i in rng.permutation(min(len(pool), max(int(n_of[s] / 0.3), 4)))[:n_of[s]]] for s in range(S)]
        if q == 0:
            s0 = next((s for s in range(S) if n_of[s] > 0), None)
            if s0 is not None:
                chosen[s0][n_of[s0] // 2] = BIG_ID
        for s, name in enumerate(names):
            kind = KINDS[s % 4]
            sc = synth_system_scores(rng, kind, n_of[s], "ties" if (s + q) % 2 == 0 else "plain")
            if s > 0 and n_of[s] >= 4 and lists[names[0]][q:q + 1] and len(lists[names[0]][q]) >= 2:
                sc[1] = np.float32(lists[names[0]][q][1]["score"])      # the same score value in two systems
            order = np.lexsort((np.arange(len(sc)), -sc.astype(np.float64)))   # a ranked list: descending, ties in draw order
            lists[name].append([{"corpus_id": int(chosen[s][i]), "score": float(sc[i])} for i in order])
    return names, lists


def save_npz(path, blob):
    """np.savez_compressed's format with fixed member timestamps: the same arrays give the same file, byte for byte."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, arr in blob.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arr), allow_pickle=False)


def gen(out_dir):
    Aggregator, _, _ = load_reference()
    made = []
    for tag, seed, ks, Q, mode, lens in CASES:
        names, lists = make_case(seed, ks, Q, mode, lens)
        rng = np.random.default_rng(seed + 1000)
        w = rng.dirichlet(np.ones(len(names)))
        w = np.round(w / 0.05) * 0.05
        w[-1] = max(0.0, 1.0 - w[:-1].sum())
        weights = {s: float(x) for s, x in zip(names, w)}
        distr = {}
        for s in names:
            pool = np.array([x["score"] for q in range(Q) for x in lists[s][q]], dtype=np.float64)
            distr[s] = np.quantile(pool, np.linspace(0, 1, min(101, max(3, len(pool)))))
        in_ids, in_sc, in_len = pack_lists(names, lists, Q)
        blob = {"systems": np.array(names), "in_ids": in_ids, "in_scores": in_sc, "in_len": in_len,
                "weights": np.array([weights[s] for s in names], dtype=np.float64)}
        for s in names:
            blob[f"distr_{s}"] = distr[s]
        raises = []
        for method, norm in METHODS:
            key = f"{method}__{norm}"
            try:
                fused = Aggregator.fuse(copy.deepcopy(lists), method=method, normalization=norm, linear_weights=weights,
                                        percentile_distributions=distr)
            except RuntimeError:
                raises.append(key)
                continue
            o_ids, o_sc, o_len = pack_out(fused, Q)
            blob[f"out_ids__{key}"] = o_ids
            blob[f"out_scores__{key}"] = o_sc
            blob[f"out_len__{key}"] = o_len
        blob["raises"] = np.array(raises, dtype="U64")
        name = f"topkfuse_seed{seed}_{tag}.npz"
        save_npz(os.path.join(out_dir, name), blob)
        made.append(name)
    return made


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    for n in gen(a.out):
        print(n)
