"""Passage lists to document lists (MaxP): ops.lists_collapse (csrc/lists_collapse.hip) at Q = 1024 queries, passage depth 3,000,
documents of 1-8 passages, next to the two routes such a list had before it:

  * the host route: RankedTopk.to_lists(), then per query a dict in list order (first passage of a document = its best), measured on
    --host-queries queries by the host clock and scaled to 1024;
  * a torch-ops route: scatter_reduce(amax) of the scores onto a [queries, D] plane by document, then a descending row sort of the
    plane, in blocks of 256 queries.

The three are called in turn inside one loop (HIP events around each call, median over the loop), and their lists must be equal
(scores are distinct inside a row, so no tie rule is in play).  Then PassageGroups.pair_scores on the collapsed lists (W = 3,000
candidate documents per query) against the plain passage ops.dot_pairs it wraps, with the shares of expand and max.

Usage: python tools/bench_collapse.py [--out profiles/r26_collapse.json] [--queries 1024] [--reps 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusion_amd import ops  # noqa: E402
from fusion_amd.passages import PassageGroups  # noqa: E402
from fusion_amd.planes import RankedTopk  # noqa: E402

ID_BASE, DOC_BASE = 3 << 31, 5 << 33
DOCS, POOL = 20_000, 1_500          # documents in the corpus; consecutive documents a query's passages come from


def make_lists(Q, n, seed):
    rng = np.random.default_rng(seed)
    poff = np.concatenate([[0], np.cumsum(rng.integers(1, 9, DOCS))]).astype(np.int64)
    groups = PassageGroups(poff, id_base=ID_BASE, doc_id_base=DOC_BASE, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    first = torch.randint(0, DOCS - POOL, (Q, 1), generator=g, device="cuda")
    lo, hi = groups.poff[first], groups.poff[first + POOL]
    width = int((hi - lo).min())
    assert width >= n, (width, n)
    pick = torch.rand((Q, width), generator=g, device="cuda").argsort(1)[:, :n]             # n distinct passages of the pool
    ids = (lo + pick + ID_BASE).contiguous()
    r = torch.arange(n, device="cuda", dtype=torch.float32)
    sc = ((n - r)[None, :] + 0.5 * torch.rand((Q, n), generator=g, device="cuda")) / n      # strictly descending, distinct
    topk = RankedTopk(ids=ids, scores=sc.contiguous(), lens=torch.full((Q,), n, dtype=torch.int32, device="cuda"))
    return groups, topk


def alternate_ms(calls: dict, reps, warm=3):
    """Every call once per iteration, in turn; HIP events around each.  -> {name: dict(median_ms, min_ms, max_ms)}."""
    for _ in range(warm):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(np.min(t)), 4), max_ms=round(float(np.max(t)), 4))
            for k, t in times.items()}


def host_route(groups, topk, queries):
    """to_lists(), then the dict walk.  -> (ms for `queries` queries, their document lists)."""
    part = RankedTopk(ids=topk.ids[:queries], scores=topk.scores[:queries], lens=topk.lens[:queries])
    group = groups.group_of.cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = []
    for l in part.to_lists():
        best = {}
        for x in l:
            best.setdefault(int(group[x["corpus_id"] - ID_BASE]) + DOC_BASE, x["score"])
        out.append(best)
    return (time.perf_counter() - t0) * 1e3, out


def torch_route(groups, topk, block=256):
    """scatter_reduce(amax) onto a [block, D] plane + descending row sort.  -> (doc ids [Q, n], scores [Q, n], lens [Q])."""
    Q, n = topk.ids.shape
    ids, sc, lens = [], [], []
    for q0 in range(0, Q, block):
        doc = groups.group_of[topk.ids[q0:q0 + block] - ID_BASE].long()
        plane = torch.full((doc.shape[0], groups.D), float("-inf"), device="cuda")
        plane.scatter_reduce_(1, doc, topk.scores[q0:q0 + block], "amax", include_self=True)
        v, i = plane.sort(dim=1, descending=True, stable=True)
        v, i = v[:, :n], i[:, :n]
        listed = v > float("-inf")
        ids.append(torch.where(listed, i + DOC_BASE, -1)); sc.append(v); lens.append(listed.sum(1, dtype=torch.int32))
    return torch.cat(ids), torch.cat(sc), torch.cat(lens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=3000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-queries", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r26_collapse.json"))
    a = ap.parse_args()
    Q, n = a.queries, a.depth
    groups, topk = make_lists(Q, n, seed=26)
    collapse = lambda: groups.collapse(topk)
    t = alternate_ms(dict(collapse=collapse, torch_ops=lambda: torch_route(groups, topk)), a.reps)
    hq = min(a.host_queries, Q)
    host_route(groups, topk, min(hq, 8))                                                     # warm-up
    host_ms, host_lists = host_route(groups, topk, hq)
    docs, best = collapse()
    t_ids, t_sc, t_len = torch_route(groups, topk)
    L = docs.lens.long()
    live = torch.arange(n, device="cuda")[None, :] < L[:, None]
    equal_torch = bool(torch.equal(docs.lens, t_len) and torch.equal(docs.ids[live], t_ids[live]) and torch.equal(docs.scores[live], t_sc[live]))
    d_ids, d_sc = docs.ids[:hq].cpu().numpy(), docs.scores[:hq].cpu().numpy().astype(np.float64)
    equal_host = all(list(h.keys()) == d_ids[q, :len(h)].tolist() and list(h.values()) == d_sc[q, :len(h)].tolist() and len(h) == int(L[q])
                     for q, h in enumerate(host_lists))
    out = dict(what="MaxP collapse of passage top-k lists (ops.lists_collapse) vs the host route over to_lists() and a torch-ops route "
                    "(scatter_reduce(amax) onto a [256, D] plane + row sort); the device calls alternate inside one loop, HIP events, median of "
                    f"{a.reps} after 3 warm-up rounds; the host route by the host clock on {hq} queries, scaled",
               device=torch.cuda.get_device_properties(0).name, Q=Q, depth=n, documents=groups.D, passages=groups.P, pmax=groups.pmax,
               documents_per_list_mean=round(float(docs.lens.float().mean()), 1),
               collapse=t["collapse"], torch_ops_route=t["torch_ops"], host_route_ms_measured=round(host_ms, 1), host_route_queries=hq,
               host_route_ms_per_1024q=round(host_ms * 1024 / hq, 1), lists_equal_torch_ops=equal_torch, lists_equal_host=bool(equal_host))
    out["speedup_vs_torch_ops"] = round(t["torch_ops"]["median_ms"] / t["collapse"]["median_ms"], 1)
    out["speedup_vs_host"] = round(out["host_route_ms_per_1024q"] / (t["collapse"]["median_ms"] * 1024 / Q), 1)
    # the exact MaxP score of the collapsed lists' documents against the passage pair kernel it wraps
    g = torch.Generator(device="cuda").manual_seed(7)
    Dn = ops.normalize_rows(torch.randn((groups.P, a.dim), generator=g, device="cuda"))
    Qn = ops.normalize_rows(torch.randn((Q, a.dim), generator=g, device="cuda"))
    scorer = lambda ids, lens: ops.dot_pairs(Qn, Dn, ids, lens, id_base=ID_BASE)
    ldp = min(n * groups.pmax, groups.P)
    pcand, seg, plen = ops.group_expand(docs.ids, docs.lens, groups.poff, ldp, id_base=ID_BASE, doc_id_base=DOC_BASE)
    ps = scorer(pcand, plen)
    p = alternate_ms(dict(pair_scores=lambda: groups.pair_scores(scorer, docs.ids, docs.lens),
                          dot_pairs=lambda: scorer(pcand, plen),
                          group_expand=lambda: ops.group_expand(docs.ids, docs.lens, groups.poff, ldp, id_base=ID_BASE, doc_id_base=DOC_BASE),
                          group_max=lambda: ops.group_max(ps, pcand, seg, docs.lens)), a.reps)
    exact, _ = groups.pair_scores(scorer, docs.ids, docs.lens)
    out["pair_scores"] = dict(W=n, dim=a.dim, ldp=ldp, passages_per_query_mean=round(float(plen.float().mean()), 1), **p,
                              overhead_over_dot_pairs=round(p["pair_scores"]["median_ms"] / p["dot_pairs"]["median_ms"], 3),
                              finite_where_listed=bool(torch.isfinite(exact[live]).all()))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
