"""Lexical pseudo-relevance feedback (csrc/bm25_weighted.hip, csrc/feedback_lexical.hip) on one synthetic 1.1 M-document BM25 shard,
Q = 1024 and 195, fb_docs = 10, fb_terms = 10:

  (a) the weighted plane and filter launches against the unweighted ones on the same queries with qw = 1.0 (one chunk of documents;
      the expected cost is one float64 multiply per posting): the ratio is reported, not asserted;
  (b) the feedback kernel (ops.lexical_feedback, wrapper included) against a torch restatement: gather the rows, sort by (query, term),
      segment-sum, topk.  The torch route sums in no fixed order: only its timing is taken;
  (c) BM25.search_feedback at k = 1000 split into first search, feedback and second search.

The calls of a group alternate inside one loop (HIP events around each, median over the loop).

Usage: python tools/bench_lexical_feedback.py [--out profiles/r28_lexical_feedback.json] [--docs 1105228] [--queries 1024,195] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_feedback import alternate_ms  # noqa: E402
from fusion_amd import feedback, ops  # noqa: E402
from fusion_amd.retrievers.bm25 import BM25, WeightedQueries  # noqa: E402

FB_DOCS, FB_TERMS, K = 10, 10, 1000


def synthetic_text(rng, n_docs, lo, hi, vocab_size):
    vocab = np.array([f"w{i}" for i in range(vocab_size)])
    p = 1.0 / np.arange(1, vocab_size + 1); p /= p.sum()
    sizes = rng.integers(lo, hi, n_docs)
    words = rng.choice(vocab, size=int(sizes.sum()), p=p)
    return [" ".join(w) for w in np.split(words, np.cumsum(sizes)[:-1])]


def torch_feedback(model, qoff, flat, fb_ids, fb_len, coef, m):
    """The torch restatement of the selection: rows gathered, (query, term) keys sorted, segment sums, topk per query."""
    fwd, pval = model.forward, model.lexical_tables()[0]
    Q, F = fb_ids.shape
    d = fb_ids.clamp(min=0)
    start, lens = fwd.foff[d], fwd.foff[d + 1] - fwd.foff[d]
    lens = torch.where(torch.arange(F, device=d.device)[None, :] < fb_len[:, None], lens, torch.zeros_like(lens))
    L = int(lens.max().item())
    at = torch.arange(L, device=d.device)
    live = at[None, None, :] < lens[:, :, None]
    src = (start[:, :, None] + at[None, None, :])[live]
    qid = torch.arange(Q, device=d.device)[:, None, None].expand(Q, F, L)[live]
    key = qid * fwd.V + fwd.fterm[src].long()
    val = coef.double()[:, :, None].expand(Q, F, L)[live] * pval[fwd.fpos[src].long()]
    key, order = torch.sort(key)
    uniq, inv = torch.unique_consecutive(key, return_inverse=True)
    w = torch.zeros(uniq.numel(), dtype=torch.float64, device=d.device).index_add_(0, inv, val[order])
    plane = torch.full((Q, fwd.V), float("-inf"), dtype=torch.float64, device=d.device)
    plane.view(-1)[uniq] = w
    return torch.topk(plane, m, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r28_lexical_feedback.json")
    ap.add_argument("--docs", type=int, default=1105228)
    ap.add_argument("--queries", default="1024,195")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    rng = np.random.default_rng(28)
    model = BM25(synthetic_text(rng, args.docs, 20, 90, 200_000), 1.5, 0.75)
    model.build_forward()
    mode, (vals, idf) = model.lexical_mode(), model.lexical_tables()
    N, S = model.corpus_size, ops.lexical_slice_docs(model.lexical_mode())
    hi = min(N, 64 * S)
    out = dict(docs=N, postings=int(model.pdoc.numel()), fb_docs=FB_DOCS, fb_terms=FB_TERMS, k=K, reps=args.reps, walk_docs=hi, runs=[])
    for Q in (int(x) for x in args.queries.split(",")):
        queries = synthetic_text(rng, Q, 4, 9, 200_000)
        qoff, flat = model._query_csr(queries)
        ones = torch.ones(flat.numel(), dtype=torch.float64, device="cuda")
        tau = torch.full((Q,), 1e300, dtype=torch.float64, device="cuda")
        cs, ci = torch.empty((Q, 64), dtype=torch.float64, device="cuda"), torch.empty((Q, 64), dtype=torch.int64, device="cuda")
        cl, ov = torch.zeros(Q, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")

        def plane(qw):
            return lambda: ops.lexical_scores_range(mode, model.toff, model.pdoc, vals, idf, qoff, flat, Q, N, 0, hi, slice_off=model.slice_off, qw=qw)

        def filt(qw):
            return lambda: ops.lexical_filter(mode, model.toff, model.pdoc, vals, idf, qoff, flat, Q, N, 0, hi, 0, tau, cs, ci, cl, ov,
                                              slice_off=model.slice_off, qw=qw)
        walk = alternate_ms(dict(plane=plane(None), plane_w=plane(ones), filter=filt(None), filter_w=filt(ones)), args.reps)
        first = model.search_topk(queries, K)
        fb_ids, fb_len, coef = feedback.coefficients(first, FB_DOCS, 1.0, "uniform")
        fb = alternate_ms(dict(
            kernel=lambda: ops.lexical_feedback(mode, model.forward, vals, idf, qoff, flat, fb_ids, fb_len, coef, 1.0, 0.5, FB_TERMS),
            torch=lambda: torch_feedback(model, qoff, flat, fb_ids, fb_len, coef, FB_TERMS)), args.reps)
        wq = model.feedback(queries, first)
        steps = alternate_ms(dict(first=lambda: model.search_topk(queries, K), feedback=lambda: model.feedback(queries, first),
                                  second=lambda: model.search_topk_weighted(wq, K), whole=lambda: model.search_feedback(queries, K)),
                             max(3, args.reps // 4))
        out["runs"].append(dict(Q=Q, walk=walk, plane_ratio=round(walk["plane_w"]["median_ms"] / walk["plane"]["median_ms"], 4),
                                filter_ratio=round(walk["filter_w"]["median_ms"] / walk["filter"]["median_ms"], 4), feedback=fb,
                                search_feedback=steps, expanded_entries=int(wq.qoff[-1]), flags=wq.flags, path=model.last_path))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
