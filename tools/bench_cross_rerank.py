"""The cross-encoder rerank of top-k lists, both routes on the SAME pairs: Q queries x `--depth` candidates each (distinct per query,
uniform over a synthetic corpus), `random_cross_encoder(size="base")` (CamemBERT-base shape, random weights, HashTokenizer).

  search   Ranker.cross_encoder_search: pair strings in, a Python loop over the queries, one predict() per query, every pair tokenised on
           the host, a padded id matrix uploaded per sub-batch
  rerank   Ranker.cross_encoder_rerank: a ShardedTextIndex (the corpus tokenised once, outside the timed calls) and the id plane in;
           fz_pair_plan + one read-back + fz_pair_fill per sub-batch

The two routes are alternated call by call in ONE process (drift on a shared machine hits both alike); a call's wall time ends at a device
synchronisation.  Reported per route: wall time, the device time of the forward (HIP events around every PackedBertForward.hidden_packed:
both routes go through it), for `rerank` the device time of the plan and fill kernels and the host time of tokenising the queries, for
`search` the host time of tokenising all its pairs (measured on its own, outside the alternation: inside predict it overlaps nothing).

Usage: python tools/bench_cross_rerank.py [--queries 64] [--depth 100] [--docs 20000] [--reps 3] [--out profiles/r22_cross_rerank.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fusion_amd import encoders, ops  # noqa: E402
from fusion_amd.distributed import ShardedTextIndex  # noqa: E402
from fusion_amd.retrievers.hybrid import Ranker  # noqa: E402

EVENTS = []      # (name, start, end) of the current call


def timed(name, f):
    def g(*a, **kw):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = f(*a, **kw)
        e.record()
        EVENTS.append((name, s, e))
        return out
    return g


def texts(rng, n, mean, spread, vocab=30000):
    lens = np.clip(rng.normal(mean, spread, n).astype(np.int64), 1, None)
    return [" ".join(f"w{w}" for w in rng.zipf(1.3, int(k)) % vocab) for k in lens]


def call(f):
    EVENTS.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev = {}
    for name, s, e in EVENTS:
        dev[name] = dev.get(name, 0.0) + s.elapsed_time(e)
    return out, wall, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--doc-words", type=int, default=260)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="base", choices=("base", "small"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_cross_rerank.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(22)
    if a.size == "base":
        ce = encoders.random_cross_encoder("cuda", size="base")
    else:               # a small model the packed forward covers (64-wide heads), for trying the tool out
        from transformers import CamembertConfig, CamembertForSequenceClassification
        cfg = dict(encoders.TINY, hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=514)
        ce = encoders.CrossEncoder(CamembertForSequenceClassification(CamembertConfig(num_labels=1, **cfg)), encoders.HashTokenizer(cfg["vocab_size"]), "cuda")
    docs = texts(rng, a.docs, a.doc_words, a.doc_words // 3)
    queries = texts(rng, a.queries, 14, 5)
    cand = np.stack([rng.choice(a.docs, a.depth, replace=False) for _ in range(a.queries)]).astype(np.int64)
    t0 = time.perf_counter()
    index = ShardedTextIndex.from_texts(ce, docs)
    build_s = time.perf_counter() - t0
    cand_d = torch.from_numpy(cand).cuda()
    as_dicts = [{int(i): docs[int(i)] for i in row} for row in cand]
    fwd = ce._packed_forward(getattr(ce.model, ce.model.base_model_prefix))
    fwd.hidden_packed = timed("forward", fwd.hidden_packed)
    ops.pair_plan, ops.pair_fill = timed("plan", ops.pair_plan), timed("fill", ops.pair_fill)
    routes = {"search": lambda: Ranker.cross_encoder_search(queries, as_dicts, None, model=ce),
              "rerank": lambda: Ranker.cross_encoder_rerank(queries, index, cand_d, model=ce)}
    for f in routes.values():      # one warm-up call each
        call(f)
    runs = {n: [] for n in routes}
    last = {}
    for _ in range(a.reps):
        for n, f in routes.items():
            last[n], wall, dev = call(f)
            runs[n].append(dict(wall_s=wall, **{k + "_ms": v for k, v in dev.items()}))
    # host tokenisation on its own
    t0 = time.perf_counter()
    n_tok = 0
    for q, row in zip(queries, as_dicts):
        n_tok += int(ce._pair_ids([(q, d) for d in row.values()], ce.max_length)[1].sum())
    pairs_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ce.tokenizer.encode_plain(queries, ce.max_length - 2)
    queries_s = time.perf_counter() - t0
    got = last["rerank"].ids.cpu().numpy()
    same = float(np.mean([[x["corpus_id"] for x in lst] == got[q, : len(lst)].tolist() for q, lst in enumerate(last["search"])]))
    med = lambda n, k: round(float(np.median([r.get(k, 0.0) for r in runs[n]])), 4)      # noqa: E731
    out = dict(tool="tools/bench_cross_rerank.py", device=torch.cuda.get_device_name(0), model=f"random_cross_encoder(size={a.size!r})",
               queries=a.queries, depth=a.depth, docs=a.docs, pair_tokens=n_tok, tokens_per_pair=round(n_tok / (a.queries * a.depth), 1),
               max_length=ce.max_length, reps=a.reps, index_build_s=round(build_s, 3),
               search=dict(wall_s=med("search", "wall_s"), forward_ms=med("search", "forward_ms"), host_tokenise_pairs_s=round(pairs_s, 4)),
               rerank=dict(wall_s=med("rerank", "wall_s"), forward_ms=med("rerank", "forward_ms"), plan_ms=med("rerank", "plan_ms"),
                           fill_ms=med("rerank", "fill_ms"), host_tokenise_queries_s=round(queries_s, 5)),
               lists_identical_share=same, calls=runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "calls"}))


if __name__ == "__main__":
    main()
