"""Pseudo-relevance feedback (csrc/feedback.hip) on the synthetic SPLADE-shaped shard of profiles/r07_splade_search.json (about 166
postings per document, 37 terms per query, V = 32,005, N = 1.1 M), Q = 1024 and 195, fb_docs = 10, fb_terms = 32:

  (a) the sparse kernel alone (the C entry on preallocated planes) and ops.sparse_feedback around it (the width read, the flag read,
      the CSR build) against the torch route: dense [Q, V] planes, index_add_ of the gathered postings, topk over the candidates,
      nonzero.  The torch route adds with atomics in no fixed order: its weights are compared within a tolerance, its term sets exactly;
  (b) ops.dense_feedback against torch.einsum over the gathered rows (dim 768);
  (c) ShardedSparseIndex.search_feedback against the two plain searches it contains: the feedback step's share.

The calls of a group alternate inside one loop (HIP events around each, median over the loop).

Usage: python tools/bench_feedback.py [--out profiles/r27_feedback.json] [--docs 1105228] [--queries 1024,195] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_splade_search import V, splade_blocks  # noqa: E402
from fusion_amd import _lib, feedback, ops  # noqa: E402
from fusion_amd.distributed import ShardedSparseIndex  # noqa: E402
from fusion_amd.planes import RankedTopk  # noqa: E402

FB_DOCS, FB_TERMS, K, DIM = 10, 32, 1000, 768


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


def raw_kernel(fwd, q, fb_ids, fb_len, coef, width):
    """The C entry alone, on planes allocated once.  -> (call, out_terms, out_w, out_len)."""
    L = _lib.lib()
    Q = q[0].numel() - 1
    out_t = ops.alloc_plane(Q, width, torch.int32, "cuda")
    out_w = ops.alloc_plane(Q, width, torch.float32, "cuda")
    out_len = torch.zeros(Q, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def call():
        _lib.check(L.fz_sparse_feedback_f32(p(fwd.foff), p(fwd.rows), V, fwd.N, 0, p(q[0]), p(q[1]), p(q[2]), Q, p(fb_ids), fb_ids.stride(0),
                                            p(fb_len), p(coef), coef.stride(0), fb_ids.shape[1], 1.0, FB_TERMS, p(out_t), p(out_w),
                                            out_t.stride(0), width, p(out_len), p(flag), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "fz_sparse_feedback_f32")
    return call, out_t, out_w, out_len


def torch_route(fwd, q, fb_ids, fb_len, coef):
    """Dense [Q, V] planes, index_add_, topk, nonzero.  -> (kept-term mask [Q, V] bool, sums [Q, V])."""
    qoff, qterms, qw = q
    Q, F = fb_ids.shape
    dev = qoff.device
    qrow = torch.repeat_interleave(torch.arange(Q, device=dev), qoff[1:] - qoff[:-1])
    acc = torch.zeros((Q, V), device=dev)
    acc.view(-1).index_add_(0, qrow * V + qterms.long(), qw)
    isq = torch.zeros((Q, V), dtype=torch.bool, device=dev)
    isq.view(-1)[qrow * V + qterms.long()] = True
    live = (torch.arange(F, device=dev)[None, :] < fb_len[:, None]) & (fb_ids >= 0) & (fb_ids < fwd.N)
    d = torch.where(live, fb_ids, torch.zeros_like(fb_ids))
    n = torch.where(live, fwd.foff[d + 1] - fwd.foff[d], torch.zeros_like(d)).view(-1)
    slot = torch.repeat_interleave(torch.arange(Q * F, device=dev), n)
    start = torch.cumsum(n, 0) - n
    src = fwd.foff[d].view(-1)[slot] + (torch.arange(slot.numel(), device=dev) - start[slot])
    at = (slot // F) * V + fwd.rows[src, 0].long()
    acc.view(-1).index_add_(0, at, coef.reshape(-1)[slot] * fwd.rows[src, 1].view(torch.float32))
    touched = torch.zeros((Q, V), dtype=torch.bool, device=dev)
    touched.view(-1)[at] = True
    cand = touched & ~isq
    top = torch.topk(torch.where(cand, acc, torch.full_like(acc, float("-inf"))), FB_TERMS, dim=1)
    keep = isq.clone()
    keep.scatter_(1, top.indices, top.values > float("-inf"))
    keep |= isq
    nz = keep.nonzero()
    return keep, acc, nz


def run(shard, Dn, Q, reps):
    fwd = shard.index.forward
    Qm = next(splade_blocks(2, Q, 40, block=Q))[1]
    q = ops.sparse_rows(Qm, V)
    first = RankedTopk.from_search(*shard.search(*q, K))
    fb_ids, fb_len, coef = feedback.coefficients(first, FB_DOCS, 1.0, "uniform")
    fb_ids, coef = fb_ids.contiguous(), coef.contiguous()
    width = int((q[0][1:] - q[0][:-1]).max()) + FB_TERMS
    kernel, out_t, out_w, out_len = raw_kernel(fwd, q, fb_ids, fb_len, coef, width)
    a = alternate_ms(dict(kernel=kernel,
                          wrapper=lambda: ops.sparse_feedback(fwd, V, *q, fb_ids, fb_len, coef, 1.0, FB_TERMS, normalize=True),
                          torch_route=lambda: torch_route(fwd, q, fb_ids, fb_len, coef)), reps)
    kernel()
    keep, acc, _ = torch_route(fwd, q, fb_ids, fb_len, coef)
    mine = torch.zeros((Q, V), dtype=torch.bool, device="cuda")
    rows = torch.arange(Q, device="cuda")[:, None].expand(-1, width)
    listed = out_t >= 0
    mine[rows[listed], out_t[listed].long()] = True
    same_rows = (mine == keep).all(1)
    err = (out_w[listed] - acc[rows[listed], out_t[listed].long()]).abs().max()
    gathered = int((fwd.foff[fb_ids.clamp(min=0) + 1] - fwd.foff[fb_ids.clamp(min=0)]).sum()) * 8
    res = dict(Q=Q, fb_docs=FB_DOCS, fb_terms=FB_TERMS, query_terms=round(q[1].numel() / Q, 1), width=width,
               expanded_terms_mean=round(float(out_len.float().mean()), 1), gathered_row_bytes=gathered,
               sparse=dict(kernel=a["kernel"], ops_sparse_feedback=a["wrapper"], torch_route=a["torch_route"],
                           kernel_speedup_vs_torch=round(a["torch_route"]["median_ms"] / a["kernel"]["median_ms"], 1),
                           rows_with_the_torch_routes_terms=int(same_rows.sum()), max_abs_weight_difference=float(err)))
    # (b) dense
    g = torch.Generator(device="cuda").manual_seed(3)
    Qn = ops.normalize_rows(torch.randn((Q, DIM), generator=g, device="cuda"))
    live = (torch.arange(FB_DOCS, device="cuda")[None, :] < fb_len[:, None]) & (fb_ids >= 0)
    cm = torch.where(live, coef, torch.zeros_like(coef))
    ein = lambda: Qn + torch.einsum("qf,qfd->qd", cm, Dn[fb_ids.clamp(min=0)])
    b = alternate_ms(dict(kernel=lambda: ops.dense_feedback(Qn, Dn, fb_ids, fb_len, coef, 1.0), einsum=ein), reps)
    res["dense"] = dict(dim=DIM, kernel=b["kernel"], torch_einsum=b["einsum"],
                        max_abs_difference=float((ops.dense_feedback(Qn, Dn, fb_ids, fb_len, coef, 1.0) - ein()).abs().max()))
    # (c) the stage inside search -> feedback -> search
    q2 = shard.feedback(*q, first, fb_docs=FB_DOCS, fb_terms=FB_TERMS)
    c = alternate_ms(dict(first_search=lambda: shard.search(*q, K), feedback=lambda: shard.feedback(*q, first, fb_docs=FB_DOCS, fb_terms=FB_TERMS),
                          second_search=lambda: shard.search(*q2, K),
                          search_feedback=lambda: shard.search_feedback(*q, K, fb_docs=FB_DOCS, fb_terms=FB_TERMS)), max(reps // 2, 3))
    res["search_feedback"] = dict(k=K, **c, expanded_query_terms=round(q2[1].numel() / Q, 1),
                                  feedback_share_of_search_feedback=round(c["feedback"]["median_ms"] / c["search_feedback"]["median_ms"], 4),
                                  feedback_over_first_search=round(c["feedback"]["median_ms"] / c["first_search"]["median_ms"], 4))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1105228)
    ap.add_argument("--queries", default="1024,195")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r27_feedback.json"))
    a = ap.parse_args()
    idx = ops.sparse_index_from_blocks(splade_blocks(1, a.docs, 200), V, N=a.docs)
    shard = ShardedSparseIndex(idx, 0)
    shard.build_forward()
    g = torch.Generator(device="cuda").manual_seed(4)
    Dn = torch.empty((a.docs, DIM), device="cuda")
    for r0 in range(0, a.docs, 65536):
        Dn[r0:r0 + 65536] = ops.normalize_rows(torch.randn((min(65536, a.docs - r0), DIM), generator=g, device="cuda"))
    out = dict(what="pseudo-relevance feedback: fz_sparse_feedback_f32 / fz_dense_feedback_f32 against torch routes, and the stage's share of "
                    f"search -> feedback -> search; calls of a group alternate inside one loop, HIP events, median of {a.reps} after 3 warm-up "
                    "rounds (the search group: half as many)",
               device=torch.cuda.get_device_properties(0).name, N=a.docs, V=V, postings_per_doc=round(idx.nnz / a.docs, 1), runs=[])
    for Q in (int(x) for x in a.queries.split(",")):
        out["runs"].append(run(shard, Dn, Q, a.reps))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
