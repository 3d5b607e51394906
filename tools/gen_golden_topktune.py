#!/usr/bin/env python
"""tests/golden/topktune_*.npz: the reference's weight-grid loop (hybrid.py:404-426: per weight vector
Aggregator.fuse(deepcopy(results)) -> run_evaluation) on TOP-K-SHAPED lists, i.e. on the inputs of two committed list-form cases
(tests/golden/topkfuse_*.npz: lists and percentile tables are read from those files).

    python tools/gen_golden_topktune.py [--out DIR]       (default: tests/golden; needs the reference tree, FUSION_REFERENCE)

Stored per case: `queries` (the queries of the topkfuse case the fixture keeps, see below), `labels` (per kept query its gold ids,
comma-separated), `weights` [W, S] (np.float64 lattice vectors of hybrid.py:405-409, a spread of about 25 of them, zeros
included), `metric_names`, `metrics__<normalisation>` [W, 15] for every normalisation the reference evaluated, `nan__<normalisation>` [W] (True: the
reference's fused lists held a NaN score for that vector -- the z-score of a single-entry list, -inf * 0 under NCE -- so that its
sorted() compared NaN keys and the stored ranking is an artefact of the comparison sequence, not a ranking), and `raises`: the
normalisations for which the reference RAISED on the case (min-max on an empty list: min() of an empty tensor).  No metrics are
stored for those; the tests hold them to the project's own rule instead -- an empty list contributes nothing (oracle.tune_lists).

Labels: 1-5 gold ids per query -- ids from the head of some system's list, ids only ONE system lists, ids no system lists, and
in the last query all three kinds and a repeated label.

A query whose lists are ALL empty (query 2 of S4_Q4_empty) is dropped from the fixture: the reference's run_evaluation raises
on an empty prediction list (max() of an empty sequence in the reciprocal rank), whatever the normalisation.
"""
from __future__ import annotations

import argparse
import copy
import itertools
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True

from oracle.gen_golden import load_reference   # noqa: E402
from gen_golden_topk import save_npz   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TUNE_CASES = ["topkfuse_seed52_S3_Q4_kmix", "topkfuse_seed53_S4_Q4_empty"]
NORMS = ["min-max", "z-score", "arctan", "percentile-rank", "normal-curve-equivalent", "none"]
N_VECTORS = 25
ABSENT_ID = (1 << 45) + 12345          # beyond draw_ids' range: in no list


def lattice(names, step=0.05):
    """hybrid.py:405-409, evaluated with the same numpy calls: np.float64 weights."""
    return [{n: w for n, w in zip(names, comb)} for comb in itertools.product(np.arange(0, 1 + step, step), repeat=len(names))
            if np.isclose(sum(comb), 1.0)]


def draw_labels(rng, names, lists, q, at_least=1):
    sets = [[x["corpus_id"] for x in lists[n][q]] for n in names]
    listed_by = {}
    for s, ids in enumerate(sets):
        for i in ids:
            listed_by.setdefault(i, []).append(s)
    head = [i for ids in sets for i in ids[:20]]
    only_one = [i for i, ss in listed_by.items() if len(ss) == 1]
    n = max(int(rng.integers(1, 6)), at_least)
    gold = []
    for j in range(n):
        kind = j % 3
        if kind == 1 and only_one:
            gold.append(int(only_one[int(rng.integers(0, len(only_one)))]))
        elif kind == 2:
            gold.append(ABSENT_ID + 7 * q + j)
        else:
            gold.append(int(head[int(rng.integers(0, len(head)))]))
    return list(dict.fromkeys(gold))


def gen(out_dir):
    Aggregator, _, _ = load_reference()
    from src.retrievers.hybrid import run_evaluation
    made = []
    for case in TUNE_CASES:
        z = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
        names = [str(s) for s in z["systems"]]
        in_ids, in_sc, in_len = z["in_ids"], z["in_scores"], z["in_len"]
        Q = in_ids.shape[1]
        seed = int(case.split("_seed")[1].split("_")[0])
        lists = {n: [[{"corpus_id": int(in_ids[s, q, r]), "score": float(in_sc[s, q, r])} for r in range(in_len[s, q])] for q in range(Q)]
                 for s, n in enumerate(names)}
        keep = [q for q in range(Q) if any(len(lists[n][q]) for n in names)]     # an all-empty query: run_evaluation raises (docstring)
        kept = {n: [lists[n][q] for q in keep] for n in names}
        distr = {n: z[f"distr_{n}"] for n in names}
        rng = np.random.default_rng(seed + 2000)
        labels = [draw_labels(rng, names, kept, q, 3 if q == len(keep) - 1 else 1) for q in range(len(keep))]   # the last query: every kind of label
        labels[-1].append(labels[-1][0])                                          # a repeated label: len(ground_truths) counts it twice
        combos = lattice(names)
        pick = sorted(set(np.linspace(0, len(combos) - 1, N_VECTORS).round().astype(int).tolist()))
        combos = [combos[i] for i in pick]
        blob = {"systems": np.array(names), "queries": np.array(keep, dtype=np.int32),
                "labels": np.array([",".join(str(x) for x in g) for g in labels]),
                "weights": np.array([[w[s] for s in names] for w in combos], dtype=np.float64)}
        mnames, raises = None, []
        for norm in NORMS:
            rows, nan = [], []
            try:
                for w in combos:
                    fused = Aggregator.fuse(copy.deepcopy(kept), method="nsf", normalization=norm, percentile_distributions=distr, linear_weights=w)
                    perf = run_evaluation(predictions=[[x["corpus_id"] for x in r] for r in fused], labels=labels, print2console=False)
                    mnames = mnames or list(perf.keys())
                    assert list(perf.keys()) == mnames
                    rows.append([float(perf[k]) for k in mnames])
                    nan.append(any(x["score"] != x["score"] for r in fused for x in r))
            except RuntimeError:
                raises.append(norm)
                continue
            blob[f"metrics__{norm}"] = np.array(rows, dtype=np.float64)
            blob[f"nan__{norm}"] = np.array(nan, dtype=bool)
        blob["metric_names"] = np.array(mnames)
        blob["raises"] = np.array(raises, dtype="U64")
        name = case.replace("topkfuse_", "topktune_") + ".npz"
        save_npz(os.path.join(out_dir, name), blob)
        made.append(name)
    return made


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    for n in gen(a.out):
        print(n)
