"""The e4m3 ColBERT token index (ops.maxsim_pairs_e4m3, csrc/rerank8.hip; ShardedTokenIndex.quantize / build_e4m3) next to the float16 rows
and the residual code: what the rerank costs, what a shard holds, what the lists lose, what it costs to build.  One process.

  (a) rerank: bench_maxsim_pairs.py's corpus (one shard of 1,105,228 passages of unit-norm random rows) and candidates (Q x k, uniform with
      repetition).  fz_maxsim_pairs_f16, fz_maxsim_pairs_residual_f16 at 2 and 4 bits (bench_colbert_residual.py's set-up: --centroids
      centroids drawn from the rows, the first --assign-docs documents assigned and training the buckets, random codes elsewhere) and
      fz_maxsim_pairs_e4m3 -- the shipped build and, with --variant-lib, the other RB of tools/ablate/maxsim_pairs8_variants.py -- over the
      SAME candidates, ALTERNATED call by call, HIP events, medians of --reps after two warm-up calls of each; gathered bytes per second of
      each (the token bytes the candidates own over the median; the residual routes also gather a centroid row per token).  At every Q of
      --queries.  The variant's plane must equal the shipped kernel's; the e4m3 plane is checked against ops.maxsim_e4m3 on a sample.
  (b) memory: resident bytes of the shard under the three storages (memory_bytes of the index objects; the float16 and residual figures
      of the whole shard follow from bytes per token).
  (c) quality: bench_colbert_search.py's clustered corpus at --recall-docs documents with its own k-means; `search` at the k <= 10 default
      over the e4m3, 2-bit and 4-bit index against the float16 index's lists in the same run: share of queries that keep the first result,
      top-10 overlap.  A synthetic corpus: ranking quality on a trained checkpoint is NOT measured here.
  (d) quantize(): ms for the whole shard (HIP events), and build_e4m3 from 4 device blocks of the first --assign-docs documents by the host
      clock around a synchronise (second call).
The record is rewritten after every stage.  Counters are not taken here: `rocprofv3 --pmc ... -- python tools/bench_maxsim_pairs_fp8.py
--only rerank --queries 1024 --reps 1` in a run of their own.

Usage: python tools/bench_maxsim_pairs_fp8.py [--variant-lib tools/ablate/libfusion_abl_mp8_rb4.so] [--only rerank,memory,quality,build]
       [--out profiles/r25_maxsim_pairs_fp8.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_colbert_search as S  # noqa: E402
import bench_maxsim_fp8 as F8  # noqa: E402
import bench_maxsim_pairs as B  # noqa: E402
from fusion_amd import ops  # noqa: E402
from fusion_amd.distributed import ShardedTokenIndex  # noqa: E402

SHIPPED_RB = 8      # csrc/rerank8.hip: FZ_MP8_RB


def variant_pairs(lib, Q8, D8, Doff, cand, id_base, max_doc_len, descale_exp, out):
    """fz_maxsim_pairs_e4m3 of another build, called as ops.maxsim_pairs_e4m3 calls the shipped one."""
    Q, Lq, dim = Q8.shape
    rc = lib.fz_maxsim_pairs_e4m3(Q8.data_ptr(), D8.data_ptr(), Doff.data_ptr(), D8.shape[0], max_doc_len, Q, Lq, Doff.numel() - 1, dim, descale_exp,
                                  cand.data_ptr(), cand.stride(0), None, cand.shape[1], id_base, out.data_ptr(), out.stride(0),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", default="1024,195")
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--lq", type=int, default=64)
    ap.add_argument("--docs", type=int, default=1_105_228)
    ap.add_argument("--centroids", type=int, default=65536)
    ap.add_argument("--assign-docs", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--recall-docs", type=int, default=200_000)
    ap.add_argument("--recall-centroids", type=int, default=16384)
    ap.add_argument("--recall-queries", type=int, default=256)
    ap.add_argument("--only", default="rerank,memory,quality,build")
    ap.add_argument("--variant-lib", default=None, help="another build of the library (tools/ablate/maxsim_pairs8_variants.py): its "
                    "fz_maxsim_pairs_e4m3 is timed as one more route of the same alternation and its plane compared with the shipped kernel's")
    ap.add_argument("--variant-rb", type=int, default=4, help="the FZ_MP8_RB of --variant-lib (for the record)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "r25_maxsim_pairs_fp8.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_maxsim_pairs_fp8.py measures on the GPU: no device found")
    only = set(a.only.split(","))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    k, Lq, N, K = a.k, a.lq, a.docs, a.centroids
    rec = dict(tool="tools/bench_maxsim_pairs_fp8.py",
               what="e4m3 ColBERT token index against the float16 rows and the residual code: the rerank kernels alternated call by call in one "
                    "process, HIP events, median of %d after two warm-up calls of each; build steps by the host clock around a synchronise" % a.reps,
               device=torch.cuda.get_device_properties(0).name, k=k, Lq=Lq, docs=N, centroids=K, shipped_rb=SHIPPED_RB,
               quality_note="synthetic clustered corpus; ranking quality on a trained checkpoint is not measured")

    def dump(key):
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({key: rec[key]}), flush=True)

    variant = None
    if a.variant_lib:
        variant = C.CDLL(os.path.abspath(a.variant_lib))
        variant.fz_maxsim_pairs_e4m3.restype = C.c_int
        variant.fz_maxsim_pairs_e4m3.argtypes = ([C.c_void_p] * 3 + [C.c_int64] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64,
                                                                                                  C.c_void_p, C.c_int, C.c_void_p])
        rec["variant"] = dict(lib=os.path.basename(a.variant_lib), rb=a.variant_rb)

    if only & {"rerank", "memory", "build"}:
        Dtok, Doff, lens = B.make_corpus(N, 1)
        sumL = Dtok.shape[0]
        g = torch.Generator(device="cuda").manual_seed(3)
        rec["corpus"] = dict(tokens=sumL, float16_GB=round(sumL * 256 / 1e9, 2), e4m3_GB=round(sumL * 128 / 1e9, 2))
        # ---- (d) quantising the shard ------------------------------------------------------------------------------------------------
        D8 = ops.quantize_e4m3(Dtok)
        if "build" in only:
            t_q = F8.summary(F8.alternate({"q": lambda: ops.quantize_e4m3(Dtok)}, 5, warm=1)["q"])
            n_as = min(a.assign_docs, N)
            rows_as = int(Doff[n_as])
            sub_tok, sub_off = Dtok[:rows_as], Doff[: n_as + 1].clone()
            cuts = [rows_as * i // 4 for i in range(5)]
            make = lambda: ShardedTokenIndex.build_e4m3((sub_tok[x:y] for x, y in zip(cuts[:-1], cuts[1:])), sub_off, 0, max_doc_len=180)      # noqa: E731
            make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            built = make()
            torch.cuda.synchronize()
            t_built = round((time.perf_counter() - t0) * 1e3, 3)
            rec["build"] = dict(quantize_whole_shard=t_q, quantize_GBs_of_float16_read=round(sumL * 256 / (t_q["median_ms"] * 1e-3) / 1e9, 1),
                                build_e4m3_4_blocks=dict(docs=n_as, rows=rows_as, host_ms=t_built, same_bytes=bool(torch.equal(built.tok8, D8[:rows_as]))),
                                trained="nothing: no centroid table, no assignment pass, no buckets")
            del built, sub_tok
            dump("build")
        # ---- (b) memory ------------------------------------------------------------------------------------------------------------------
        if "memory" in only:
            e4 = ShardedTokenIndex(None, Doff, 0, max_doc_len=180)
            e4.tok8, e4.d_exp = D8, 8
            rec["memory"] = dict(float16=ShardedTokenIndex(Dtok, Doff, 0, max_doc_len=180).memory_bytes(), e4m3=e4.memory_bytes(),
                                 residual_nbits2=dict(codes=4 * sumL, packed=32 * sumL, total_without_candidate_index=36 * sumL),
                                 residual_nbits4=dict(codes=4 * sumL, packed=64 * sumL, total_without_candidate_index=68 * sumL),
                                 bytes_per_token=dict(float16=256, e4m3=128, residual_nbits2=36, residual_nbits4=68),
                                 note="the residual code also needs the shared centroid table (K x 256 B) and, for its codes, the assignment pass")
            dump("memory")
        # ---- (a) the rerank kernels --------------------------------------------------------------------------------------------------
        if "rerank" in only:
            Cc = Dtok[torch.randperm(sumL, generator=g, device="cuda")[:K]].contiguous()
            n_as = min(a.assign_docs, N)
            rows_as = int(Doff[n_as])
            codes = torch.randint(0, K, (sumL,), generator=g, device="cuda", dtype=torch.int32)
            codes[:rows_as] = ops.centroid_assign(Dtok[:rows_as], Cc)
            packed, weights = {}, {}
            for nbits in (2, 4):
                cutoffs, weights[nbits] = ops.residual_buckets(Dtok[:rows_as], Cc, codes[:rows_as], nbits)
                packed[nbits] = ops.residual_compress(Dtok, codes, Cc, cutoffs, nbits)
            rec["rerank"] = []
            for Q in [int(x) for x in a.queries.split(",")]:
                Qtok = B.make_queries(Q, Lq, 2)
                Q8 = ops.quantize_e4m3(Qtok)
                pos = torch.randint(0, N, (Q, k), generator=g, device="cuda")
                cand = pos + B.ID_BASE
                tokens = int(lens[pos].sum())
                outs = {n: ops.alloc_plane(Q, k, torch.float32, "cuda") for n in ("f16", "nbits2", "nbits4", "e4m3", "variant")}
                routes = {
                    "float16": lambda: ops.maxsim_pairs(Qtok, Dtok, Doff, cand, id_base=B.ID_BASE, max_doc_len=180, out=outs["f16"]),
                    "residual_nbits2": lambda: ops.maxsim_pairs_residual(Qtok, packed[2], codes, Cc, weights[2], Doff, cand, id_base=B.ID_BASE,
                                                                         max_doc_len=180, out=outs["nbits2"]),
                    "residual_nbits4": lambda: ops.maxsim_pairs_residual(Qtok, packed[4], codes, Cc, weights[4], Doff, cand, id_base=B.ID_BASE,
                                                                         max_doc_len=180, out=outs["nbits4"]),
                    f"e4m3_rb{SHIPPED_RB}": lambda: ops.maxsim_pairs_e4m3(Q8, D8, Doff, cand, id_base=B.ID_BASE, max_doc_len=180, out=outs["e4m3"]),
                }
                if variant is not None:
                    routes[f"e4m3_rb{a.variant_rb}"] = lambda: variant_pairs(variant, Q8, D8, Doff, cand, B.ID_BASE, 180, 16, outs["variant"])
                ms = F8.alternate(routes, a.reps)
                per_tok = {"float16": 256, "residual_nbits2": 36, "residual_nbits4": 68}
                row = dict(Q=Q, k=k, Lq=Lq, candidate_tokens=tokens, routes={})
                for name, xs in ms.items():
                    s = F8.summary(xs)
                    b = per_tok.get(name, 128)
                    s.update(bytes_per_token=b, gathered_GB=round(tokens * b / 1e9, 3), gathered_TBs=round(tokens * b / (s["median_ms"] * 1e-3) / 1e12, 3))
                    row["routes"][name] = s
                t16, t8 = row["routes"]["float16"]["median_ms"], row["routes"][f"e4m3_rb{SHIPPED_RB}"]["median_ms"]
                row["e4m3_over_float16"] = round(t8 / t16, 3)
                row["quantize_queries"] = F8.summary(F8.alternate({"q": lambda: ops.quantize_e4m3(Qtok)}, a.reps)["q"])
                # the contract at this size: the all-pairs e4m3 kernel's bits (first 8 queries against the documents they list)
                sub = pos[:8]
                docs, inv = torch.unique(sub, return_inverse=True)
                lo, hi = Doff[docs], Doff[docs + 1]
                rows = torch.cat([torch.arange(int(x), int(y), device="cuda") for x, y in zip(lo.tolist(), hi.tolist())])
                off = torch.zeros(docs.numel() + 1, dtype=torch.int64, device="cuda")
                off[1:] = (hi - lo).cumsum(0)
                plane = ops.maxsim_e4m3(Q8[:8], D8[rows].contiguous(), off, max_doc_len=180)
                row["bits_equal_all_pairs_e4m3_kernel"] = bool(torch.equal(torch.gather(plane, 1, inv).view(torch.int32), outs["e4m3"][:8].contiguous().view(torch.int32)))
                if variant is not None:
                    row["variant_plane_equals_shipped"] = bool(torch.equal(outs["variant"].contiguous().view(torch.int32), outs["e4m3"].contiguous().view(torch.int32)))
                rec["rerank"].append(row)
                dump("rerank")
                del outs, Qtok, Q8, pos, cand
            del packed, codes, Cc
        del Dtok, Doff, D8
        torch.cuda.empty_cache()

    # ---- (c) what the lists lose: the clustered corpus ---------------------------------------------------------------------------------
    if "quality" in only:
        Nr, Qr = a.recall_docs, a.recall_queries
        Dtok, Doff, lens, centres, doc_topics = S.make_corpus(Nr, 20000, 0.75, 1)
        Qtok, _ = S.make_queries(Qr, Lq, centres, doc_topics, Nr, 0.75, 2)
        index, info = S.build(Dtok, Doff, a.recall_centroids, 4, min(2_000_000, Dtok.shape[0]), 3)
        kk = 10
        nprobe, ncand = ShardedTokenIndex.search_defaults(kk)
        want = index.search(Qtok, k=kk, nprobe=nprobe, ncand=ncand)
        rec["quality"] = dict(docs=Nr, queries=Qr, centroids=a.recall_centroids, k=kk, nprobe=nprobe, ncand=ncand, build=info,
                              corpus="bench_colbert_search.py: 20,000 centres, 8 topics per document, noise 0.75 (the corpus of profiles/r18)",
                              against="the float16 index's lists at the same setting, same run",
                              note="synthetic clustered corpus; ranking quality on a trained checkpoint is not measured", storages={})
        base = lambda: ShardedTokenIndex(Dtok, Doff, 0, max_doc_len=180).build_centroids(index.centroids, codes=index.codes)      # noqa: E731
        x = Dtok.float()
        for name, make in (("e4m3", lambda: base().quantize(keep_tokens=True)), ("residual_nbits2", lambda: base().compress(2, keep_tokens=True)),
                           ("residual_nbits4", lambda: base().compress(4, keep_tokens=True))):
            ix = make()
            got = ix.search(Qtok, k=kk, nprobe=nprobe, ncand=ncand)
            D = ix.dequantized() if ix.tok8 is not None else ix.decompressed().float()
            mb = ix.memory_bytes()
            rec["quality"]["storages"][name] = dict(
                top1_kept=round(float((got.ids[:, 0] == want.ids[:, 0]).float().mean()), 4), top10_overlap=S.recall_at(got.ids, want.ids, 10),
                reconstruction_mse=float(((x - D) ** 2).mean()), resident_bytes_without_kept_tokens=mb["total"] - 256 * Dtok.shape[0])
            del ix, D
        dump("quality")


if __name__ == "__main__":
    main()
