"""ColBERT first-stage search (ShardedTokenIndex.search: centroid probes -> candidate stage -> exact rerank) on a clustered synthetic
corpus: what the index costs to build, what each stage costs per query batch at one shard's size, and what the candidate stage loses.

Corpus (stated, not fitted to a data set): --centres unit vectors; a document draws 8 of them as its topics and every token is one of
its topics + Gaussian noise, normalised (cosine to its centre about 0.8 at the default --noise); lengths as bench_maxsim_pairs.py draws
them (round(lognormal(ln 62, 0.38)) + 2, clipped to [8, 180]).  A query is --lq tokens drawn the same way from the topics of one
document of the recall corpus, so it has a relevant document.

Two sizes, one corpus:
  * timing at --docs (one shard of mMARCO: 1,105,228 passages) with --centroids centroids, Q = --queries: index build (k-means on a
    sample, assignment, inverted index + slice table), then per (nprobe, ncand) setting the probes, the candidate stage
    (ShardedCentroidIndex.local_topk: the streamed route with its overflowed windows and the two-pass route, alternated; the documents tied
    with a list's cut score), the rerank and the
    whole search -- HIP events, median of --reps calls after a warm-up call of the same shape;
  * recall at --recall-docs (the first documents of the same corpus, their own k-means with --recall-centroids), Q = --recall-queries:
    recall@{10, 100, 1000} of the search's list against the exact all-pairs top-k (ops.maxsim + ops.topk_rows, timed too): the yardstick.
The record is rewritten after every stage, so a run that is cut short leaves what it measured.

--routes measures, instead of all that, the two routes of the centroid GEMM's selection on the same inputs: centroid_probes (Q = --queries,
Lq = --lq, K = --centroids, nprobe 1, 2, 4, 8) and centroid_assign (--assign-rows token rows) by ops.dot_topn (fused=True: the selection is
the GEMM's epilogue) and by dot_scores + topk_rows (fused=False), alternated call by call -- 5 each after a warm-up call for the probes --
with equal results asserted; -> --routes-out.  Its centroids are K token rows of the corpus distribution (the start of k-means): the times
depend on the shapes, not on how well the centroids are trained.

Usage: python tools/bench_colbert_search.py [--out profiles/r13_colbert_search.json]
       python tools/bench_colbert_search.py --routes [--routes-out profiles/r14_centroid_probes.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusion_amd import ops  # noqa: E402
from fusion_amd.distributed import ShardedTokenIndex  # noqa: E402

SETTINGS = [(1, 256), (2, 400), (2, 1000), (4, 1000), (4, 3584), (8, 3584)]      # (nprobe, ncand); the defaults of k = 10 / 100 / 1000 among them
TOPICS = 8


def doc_lengths(N, g):
    z = torch.randn(N, generator=g, device="cuda", dtype=torch.float64)
    return (torch.exp(np.log(62.0) + 0.38 * z).round() + 2).clamp(8, 180).long()


def topic_tokens(centres, topics, noise, g):
    """topics [n] int64 (the centre of every row) -> unit-norm float16 rows: centre + noise."""
    out = torch.empty((topics.numel(), 128), dtype=torch.float16, device="cuda")
    step = 1 << 21
    for lo in range(0, topics.numel(), step):
        t = topics[lo: lo + step]
        x = centres[t] + torch.randn((t.numel(), 128), generator=g, device="cuda") * (noise / np.sqrt(128.0))
        out[lo: lo + t.numel()] = (x / x.norm(dim=1, keepdim=True)).half()
    return out


def make_corpus(N, n_centres, noise, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn((n_centres, 128), generator=g, device="cuda")
    centres /= centres.norm(dim=1, keepdim=True)
    lens = doc_lengths(N, g)
    Doff = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    Doff[1:] = lens.cumsum(0)
    doc_topics = torch.randint(0, n_centres, (N, TOPICS), generator=g, device="cuda")
    doc_of = torch.repeat_interleave(torch.arange(N, device="cuda"), lens)
    pick = torch.randint(0, TOPICS, (doc_of.numel(),), generator=g, device="cuda")
    Dtok = topic_tokens(centres, doc_topics[doc_of, pick], noise, g)
    return Dtok, Doff, lens, centres, doc_topics


def make_queries(Q, Lq, centres, doc_topics, n_docs, noise, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = torch.randint(0, n_docs, (Q,), generator=g, device="cuda")
    pick = torch.randint(0, TOPICS, (Q, Lq), generator=g, device="cuda")
    return topic_tokens(centres, torch.gather(doc_topics[src], 1, pick).reshape(-1), noise, g).view(Q, Lq, 128), src


def event_ms(f, reps, warm=1):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(median_ms=round(float(np.median(times)), 3), min_ms=round(float(np.min(times)), 3), max_ms=round(float(np.max(times)), 3), reps=reps)


def event_ms_alternating(fa, fb, reps):
    """Two routes of the same work compared in one window: a warm-up call of each, then a, b, a, b, ... -- every call between its own events."""
    fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, times in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
    return tuple(dict(median_ms=round(float(np.median(t)), 3), min_ms=round(float(np.min(t)), 3), max_ms=round(float(np.max(t)), 3), reps=reps, alternated=True)
                 for t in (ta, tb))


def tie_runs(cand, pc, ps, Lq, nprobe, cut, rows=64):
    """How many documents of the first chunk score EXACTLY a query's cut score (the last entry of its candidate list): the run of equal
    scores the streamed route's fold has to put in id order.  First `rows` queries; (mean, median, max)."""
    hi = min(cand.index.N, cand._chunk())
    S = ops.centroid_scores(cand.index, pc[:rows].contiguous(), ps[:rows].contiguous(), Lq, nprobe, doc_lo=0, doc_hi=hi)
    n = (S == cut[:rows].unsqueeze(1)).sum(1).float()
    return dict(queries=int(n.numel()), documents=hi, mean=round(float(n.mean()), 1), median=float(n.median()), max=int(n.max()),
                cut_score_is_zero=round(float((cut[:rows] == 0).float().mean()), 3))


def host_s(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, round(time.perf_counter() - t0, 3)


def build(Dtok, Doff, K, iters, sample, seed):
    """-> (index with its centroid stage, build times by the host clock around a synchronise)."""
    C, t_km = host_s(lambda: ops.kmeans_centroids(Dtok, K, iters=iters, seed=seed, sample=sample))
    codes, t_as = host_s(lambda: ops.centroid_assign(Dtok, C))
    index = ShardedTokenIndex(Dtok, Doff, 0, max_doc_len=180)
    _, t_ix = host_s(lambda: index.build_centroids(C, codes=codes))
    ci = index.candidates.index
    per = (ci.coff[1:] - ci.coff[:-1]).float()
    info = dict(centroids=K, kmeans_iters=iters, kmeans_sample=sample, kmeans_s=t_km, assign_s=t_as, inverted_index_s=t_ix,
                entries=int(ci.cdoc.numel()), entries_per_token=round(ci.cdoc.numel() / max(1, Dtok.shape[0]), 3),
                list_len_mean=round(float(per.mean()), 1), list_len_max=int(per.max()), empty_lists=int((per == 0).sum()),
                slice_table_MB=None if ci.slice_off is None else round(ci.slice_off.numel() * 8 / 1e6, 1))
    return index, info


def recall_at(got_ids, want_ids, r):
    hit = (got_ids[:, :r].unsqueeze(2) == want_ids[:, :r].unsqueeze(1)).any(2).sum(1).float()
    return round(float((hit / r).mean()), 4)


def centroid_routes(a):
    """The record of --routes (see the header)."""
    g = torch.Generator(device="cuda").manual_seed(7)
    centres = torch.randn((a.centres, 128), generator=g, device="cuda")
    centres /= centres.norm(dim=1, keepdim=True)
    draw = lambda n: topic_tokens(centres, torch.randint(0, a.centres, (n,), generator=g, device="cuda"), a.noise, g)
    C, Qtok, Dtok = draw(a.centroids), draw(a.queries * a.lq).view(a.queries, a.lq, 128), draw(a.assign_rows)
    rec = dict(what="centroid_probes and centroid_assign by the fused route (ops.dot_topn: top-n selection in the GEMM's epilogue) and by the two-kernel "
                    "route (dot_scores + topk_rows) on the same inputs, alternated call by call after a warm-up call of each; HIP events",
               device=torch.cuda.get_device_properties(0).name, queries=a.queries, Lq=a.lq, centroids=a.centroids, dot_topn_max=ops.dot_topn_max(),
               block_bytes=ops.CENTROID_BLOCK_BYTES, default_fused=ops.CENTROID_FUSED, probes={})

    def dump():
        with open(a.routes_out, "w") as f:
            json.dump(rec, f, indent=1)

    for nprobe in (1, 2, 4, 8):
        f1, f0 = ops.centroid_probes(Qtok, C, nprobe, fused=True), ops.centroid_probes(Qtok, C, nprobe, fused=False)
        same = bool(torch.equal(f1[0], f0[0]) and torch.equal(f1[1].view(torch.int32), f0[1].view(torch.int32)))
        t1, t0 = event_ms_alternating(lambda: ops.centroid_probes(Qtok, C, nprobe, fused=True), lambda: ops.centroid_probes(Qtok, C, nprobe, fused=False), a.reps)
        rec["probes"][f"nprobe{nprobe}"] = dict(fused=t1, two_kernels=t0, same_bits=same, speedup=round(t0["median_ms"] / t1["median_ms"], 2))
        print(json.dumps({f"nprobe{nprobe}": rec["probes"][f"nprobe{nprobe}"]}), flush=True)
        dump()
        assert same, f"the routes differ at nprobe = {nprobe}"
    small = Dtok[: 1 << 16]
    assert torch.equal(ops.centroid_assign(small, C, fused=True), ops.centroid_assign(small, C, fused=False))
    t1, t0 = event_ms_alternating(lambda: ops.centroid_assign(Dtok, C, fused=True), lambda: ops.centroid_assign(Dtok, C, fused=False), 2)
    rec["assign"] = dict(rows=a.assign_rows, fused=t1, two_kernels=t0, speedup=round(t0["median_ms"] / t1["median_ms"], 2),
                         fused_us_per_1000_rows=round(1e3 * t1["median_ms"] / a.assign_rows * 1e3, 3),
                         two_kernels_us_per_1000_rows=round(1e3 * t0["median_ms"] / a.assign_rows * 1e3, 3))
    print(json.dumps({"assign": rec["assign"]}), flush=True)
    dump()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_105_228)
    ap.add_argument("--centroids", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--recall-docs", type=int, default=200_000)
    ap.add_argument("--recall-centroids", type=int, default=16384)
    ap.add_argument("--recall-queries", type=int, default=256)
    ap.add_argument("--lq", type=int, default=64)
    ap.add_argument("--centres", type=int, default=20000)
    ap.add_argument("--noise", type=float, default=0.75)
    ap.add_argument("--kmeans-iters", type=int, default=4)
    ap.add_argument("--kmeans-sample", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r13_colbert_search.json"))
    ap.add_argument("--routes", action="store_true", help="only the fused / two-kernel comparison of centroid_probes and centroid_assign")
    ap.add_argument("--assign-rows", type=int, default=1 << 21)
    ap.add_argument("--routes-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14_centroid_probes.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_colbert_search.py measures on the GPU: no device found")
    if a.routes:
        os.makedirs(os.path.dirname(os.path.abspath(a.routes_out)), exist_ok=True)
        return centroid_routes(a)
    assert a.recall_docs <= a.docs
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rec = dict(what="ColBERT first-stage search on a clustered synthetic corpus: HIP events, median of %d calls after one warm-up call of the same "
                    "shape; build steps by the host clock around a synchronise (one run each)" % a.reps,
               device=torch.cuda.get_device_properties(0).name, slice_docs=ops.centroid_slice_docs(), Lq=a.lq,
               corpus=dict(centres=a.centres, topics_per_document=TOPICS, noise=a.noise,
                           lengths="round(lognormal(ln 62, 0.38)) + 2, clipped to [8, 180]"))

    def dump():
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({k: rec[k] for k in list(rec)[-1:]}), flush=True)

    Dtok, Doff, lens, centres, doc_topics = make_corpus(a.docs, a.centres, a.noise, 1)
    rec["corpus"].update(docs=a.docs, tokens=int(Doff[-1]), GB=round(int(Doff[-1]) * 256 / 1e9, 2), mean_len=round(float(lens.float().mean()), 2))
    tok = Dtok[:4096].float()
    rec["corpus"]["token_cos_to_own_centre_mean"] = round(float((tok @ centres.t()).max(1).values.mean()), 3)
    dump()

    # ---- recall against the exact all-pairs top-k, at the small size ------------------------------------------------------------------
    Nr, Qr = a.recall_docs, a.recall_queries
    Dtok_r, Doff_r = Dtok[: int(Doff[Nr])], Doff[: Nr + 1].clone()
    Qtok_r, src = make_queries(Qr, a.lq, centres, doc_topics, Nr, a.noise, 2)
    (ex_s, ex_i), t_exact = host_s(lambda: ops.topk_rows(ops.maxsim(Qtok_r, Dtok_r, Doff_r, max_doc_len=180), 1000))
    index_r, info_r = build(Dtok_r, Doff_r, a.recall_centroids, a.kmeans_iters, min(a.kmeans_sample, Dtok_r.shape[0]), 3)
    rec["recall"] = dict(docs=Nr, queries=Qr, build=info_r, exact_all_pairs_topk_s=t_exact,
                         source_document_is_exact_top1=round(float((ex_i[:, 0] == src).float().mean()), 4), settings={})
    dump()
    for nprobe, ncand in SETTINGS:
        k = min(1000, ncand)
        out = index_r.search(Qtok_r, k=k, nprobe=nprobe, ncand=ncand)
        # the returned scores are exact: equal to the all-pairs plane's wherever the id is in both lists
        rec["recall"]["settings"][f"nprobe{nprobe}_ncand{ncand}"] = dict(
            k=k, overflowed_windows=index_r.candidates.last_overflow,
            **{f"recall@{r}": recall_at(out.ids, ex_i, r) for r in (10, 100, 1000) if r <= k})
        dump()
    del index_r, Dtok_r, Qtok_r, ex_s, ex_i

    # ---- times at one shard's size ------------------------------------------------------------------------------------------------------
    index, info = build(Dtok, Doff, a.centroids, a.kmeans_iters, a.kmeans_sample, 4)
    rec["shard"] = dict(docs=a.docs, queries=a.queries, build=info, settings={})
    dump()
    Qtok, _ = make_queries(a.queries, a.lq, centres, doc_topics, a.docs, a.noise, 5)
    C, cand = index.centroids, index.candidates
    for nprobe, ncand in SETTINGS:
        k = min(1000, ncand)
        pc, ps = ops.centroid_probes(Qtok, C, nprobe)
        t_probe = event_ms(lambda: ops.centroid_probes(Qtok, C, nprobe), a.reps)
        marks = []
        sc, ids = cand.local_topk(pc, ps, a.lq, nprobe, ncand, mark=marks.append, streaming=True)
        overflowed = cand.last_overflow
        ties = tie_runs(cand, pc, ps, a.lq, nprobe, sc[:, -1].contiguous())
        # the streamed route (exact head, filter launches, folds, overflowed windows redone) against a plane per chunk, top-k, merge
        t_cand, t_two = event_ms_alternating(lambda: cand.local_topk(pc, ps, a.lq, nprobe, ncand, streaming=True),
                                             lambda: cand.local_topk(pc, ps, a.lq, nprobe, ncand, streaming=False), a.reps)
        t_rerank = event_ms(lambda: index.rerank(Qtok, ids, k=k), a.reps)
        t_all = event_ms(lambda: index.search(Qtok, k=k, nprobe=nprobe, ncand=ncand), a.reps)
        rec["shard"]["settings"][f"nprobe{nprobe}_ncand{ncand}"] = dict(
            k=k, probes=t_probe, candidate_stage_streamed=t_cand, candidate_stage_two_pass=t_two, rerank=t_rerank, search=t_all,
            search_candidate_route="streamed" if cand.STREAMING else "two-pass", overflowed_windows=overflowed, streams=cand._streams(ncand, a.docs),
            filter_launches=marks.count("shard_centroid_filter"), plane_launches=marks.count("shard_centroid"), ties_at_the_cut_first_chunk=ties,
            candidates_with_a_hit_mean=round(float((cand.local_topk(pc, ps, a.lq, nprobe, ncand)[0] != 0).sum(1).float().mean()), 1))
        dump()


if __name__ == "__main__":
    main()
