"""The residual-compressed ColBERT token index (ops.maxsim_pairs_residual, csrc/rerank_residual.hip; ShardedTokenIndex.compress /
build_compressed) next to the uncompressed one: what it stores, what the rerank costs, what it costs to build and what the lists lose.

  * kernel: bench_maxsim_pairs.py's corpus (one shard of 1,105,228 passages of unit-norm random rows) and candidates (Q = 1024 x k = 1000,
    uniform with repetition), --centroids centroids (token rows of the corpus: the time depends on the shapes, not on the training).  The
    first --assign-docs documents are assigned (ops.centroid_assign) and train the buckets; the other rows get uniformly random codes --
    what the nearest of K random unit vectors is for a random row, and the worst case for the centroid-table gather.  fz_maxsim_pairs_f16
    over the float16 rows and fz_maxsim_pairs_residual_f16 (nbits = 2 and 4) over the same candidates, ALTERNATED call by call in one
    process, HIP events, median of --reps; bytes per token and per shard; the pack kernel over the whole shard;
  * build: compress (buckets + pack) and build_compressed (assign + pack from 4 blocks) of the first --assign-docs documents, by the host
    clock around a synchronise;
  * recall: bench_colbert_search.py's clustered corpus at --recall-docs documents, its own k-means; recall@10 / @100 / @1000 of `search`
    over the nbits = 2 and nbits = 4 index against the UNCOMPRESSED index's lists, at the three default (nprobe, ncand) settings.
The record is rewritten after every stage.

Usage: python tools/bench_colbert_residual.py [--out profiles/r18_colbert_residual.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_colbert_search as S  # noqa: E402
import bench_maxsim_pairs as B  # noqa: E402
from fusion_amd import ops  # noqa: E402
from fusion_amd.distributed import ShardedTokenIndex  # noqa: E402


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--lq", type=int, default=64)
    ap.add_argument("--docs", type=int, default=1_105_228)
    ap.add_argument("--centroids", type=int, default=65536)
    ap.add_argument("--assign-docs", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--recall-docs", type=int, default=200_000)
    ap.add_argument("--recall-centroids", type=int, default=16384)
    ap.add_argument("--recall-queries", type=int, default=256)
    ap.add_argument("--skip-recall", action="store_true")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "r18_colbert_residual.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_colbert_residual.py measures on the GPU: no device found")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    Q, k, Lq, N, K = a.queries, a.k, a.lq, a.docs, a.centroids
    rec = dict(what="residual-compressed ColBERT token index against the uncompressed one: the two rerank kernels alternated call by call, HIP events, "
                    "median of %d after a warm-up call of each; build steps by the host clock around a synchronise (one run each)" % a.reps,
               device=torch.cuda.get_device_properties(0).name, Q=Q, k=k, Lq=Lq, docs=N, centroids=K)

    def dump():
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({key: rec[key] for key in list(rec)[-1:]}), flush=True)

    # ---- the kernels at one shard's size -------------------------------------------------------------------------------------------------
    Dtok, Doff, lens = B.make_corpus(N, 1)
    sumL = Dtok.shape[0]
    Qtok = B.make_queries(Q, Lq, 2)
    g = torch.Generator(device="cuda").manual_seed(3)
    pos = torch.randint(0, N, (Q, k), generator=g, device="cuda")
    cand = pos + B.ID_BASE
    C = Dtok[torch.randperm(sumL, generator=g, device="cuda")[:K]].contiguous()
    n_as = min(a.assign_docs, N)
    rows_as = int(Doff[n_as])
    codes = torch.randint(0, K, (sumL,), generator=g, device="cuda", dtype=torch.int32)
    codes[:rows_as], t_assign = S.host_s(lambda: ops.centroid_assign(Dtok[:rows_as], C))
    tokens = int(lens[pos].sum())
    rec["corpus"] = dict(tokens=sumL, float16_GB=round(sumL * 256 / 1e9, 2), candidate_tokens=tokens, gathered_float16_GB=round(tokens * 256 / 1e9, 3),
                         centroid_table_MiB=round(K * 256 / 2 ** 20, 1), assigned_rows=rows_as, assign_s=t_assign,
                         codes_of_the_other_rows="uniform random")
    dump()
    out_a, out_b = ops.alloc_plane(Q, k, torch.float32, "cuda"), ops.alloc_plane(Q, k, torch.float32, "cuda")
    plain = lambda: ops.maxsim_pairs(Qtok, Dtok, Doff, cand, id_base=B.ID_BASE, max_doc_len=180, out=out_a)      # noqa: E731
    rec["kernel"] = {}
    for nbits in (2, 4):
        (cutoffs, weights), t_buckets = S.host_s(lambda: ops.residual_buckets(Dtok[:rows_as], C, codes[:rows_as], nbits))
        packed = ops.residual_compress(Dtok, codes, C, cutoffs, nbits)
        t_pack = B.event_ms(lambda: ops.residual_compress(Dtok, codes, C, cutoffs, nbits, out=packed), 5, warm=1)
        comp = lambda: ops.maxsim_pairs_residual(Qtok, packed, codes, C, weights, Doff, cand, id_base=B.ID_BASE, max_doc_len=180, out=out_b)      # noqa: E731
        t_plain, t_comp = S.event_ms_alternating(plain, comp, a.reps)
        # the contract at this size: the compressed plane is the uncompressed kernel's over the decompressed rows (first 64 queries' candidates)
        sub = pos[:64]
        D = ops.residual_decompress(packed, codes, C, weights)
        want = ops.maxsim_pairs(Qtok[:64], D, Doff, sub, max_doc_len=180)
        same = bool(torch.equal(want.view(torch.int32), ops.maxsim_pairs_residual(Qtok[:64], packed, codes, C, weights, Doff, sub, max_doc_len=180).view(torch.int32)))
        del D, want
        per_tok = 4 + 16 * nbits
        gathered = tokens * per_tok
        rec["kernel"][f"nbits{nbits}"] = dict(
            uncompressed=t_plain, compressed=t_comp, compressed_over_uncompressed=round(t_comp["median_ms"] / t_plain["median_ms"], 3),
            bytes_per_token=per_tok, shard_GB=round(sumL * per_tok / 1e9, 2), against_float16=round(256 / per_tok, 2),
            gathered_codes_and_residuals_GB=round(gathered / 1e9, 3), gathered_centroid_rows_GB=round(tokens * 256 / 1e9, 3),
            buckets_s=t_buckets, pack_kernel_whole_shard=t_pack, pack_GBs_of_float16_read=round(sumL * 256 / (t_pack["median_ms"] * 1e-3) / 1e9, 1),
            bits_equal_uncompressed_kernel_over_decompressed_rows=same)
        dump()
        del packed
    # ---- build steps on the assigned part --------------------------------------------------------------------------------------------
    rec["build"] = dict(docs=n_as, rows=rows_as)
    sub_tok, sub_off = Dtok[:rows_as], Doff[: n_as + 1].clone()
    for nbits in (2, 4):
        base = ShardedTokenIndex(sub_tok, sub_off, 0, max_doc_len=180).build_centroids(C, codes=codes[:rows_as])
        _, t_compress = S.host_s(lambda: base.compress(nbits, keep_tokens=True))
        cuts = [rows_as * i // 4 for i in range(5)]
        built, t_built = S.host_s(lambda: ShardedTokenIndex.build_compressed((sub_tok[x:y] for x, y in zip(cuts[:-1], cuts[1:])), sub_off, C, base.cutoffs,
                                                                             base.weights, nbits, 0, max_doc_len=180))
        rec["build"][f"nbits{nbits}"] = dict(compress_s=t_compress, build_compressed_4_blocks_s=t_built, memory_bytes=built.memory_bytes(),
                                             same_bytes=bool(torch.equal(built.packed, base.packed) and torch.equal(built.codes, base.codes)))
        del base, built
    dump()
    del Dtok, Doff, codes, C, sub_tok
    torch.cuda.empty_cache()
    if a.skip_recall:
        return

    # ---- what the lists lose: the clustered corpus -------------------------------------------------------------------------------------
    Nr, Qr = a.recall_docs, a.recall_queries
    Dtok, Doff, lens, centres, doc_topics = S.make_corpus(Nr, 20000, 0.75, 1)
    Qtok, _ = S.make_queries(Qr, Lq, centres, doc_topics, Nr, 0.75, 2)
    index, info = S.build(Dtok, Doff, a.recall_centroids, 4, min(2_000_000, Dtok.shape[0]), 3)
    rec["recall"] = dict(docs=Nr, queries=Qr, centroids=a.recall_centroids, corpus="bench_colbert_search.py: 20,000 centres, 8 topics per document, noise 0.75",
                         against="the uncompressed index's lists at the same setting", settings={})
    settings = [(kk,) + ShardedTokenIndex.search_defaults(kk) for kk in (10, 100, 1000)]
    want = {kk: index.search(Qtok, k=kk, nprobe=nprobe, ncand=ncand) for kk, nprobe, ncand in settings}
    x = Dtok.float()
    centre_mse = float(((x - index.centroids[index.codes.long()].float()) ** 2).mean())
    for nbits in (2, 4):
        comp = ShardedTokenIndex(Dtok, Doff, 0, max_doc_len=180).build_centroids(index.centroids, codes=index.codes).compress(nbits, keep_tokens=True)
        mse = float(((x - comp.decompressed().float()) ** 2).mean())
        row = dict(reconstruction_mse=mse, centroid_alone_mse=centre_mse, cutoffs=comp.cutoffs.tolist(), weights=comp.weights.tolist())
        for kk, nprobe, ncand in settings:
            got = comp.search(Qtok, k=kk, nprobe=nprobe, ncand=ncand)
            row[f"k{kk}_nprobe{nprobe}_ncand{ncand}"] = {f"recall@{r}": S.recall_at(got.ids, want[kk].ids, r) for r in (10, 100, 1000) if r <= kk}
            row[f"k{kk}_nprobe{nprobe}_ncand{ncand}"]["top1_equal"] = round(float((got.ids[:, 0] == want[kk].ids[:, 0]).float().mean()), 4)
        rec["recall"]["settings"][f"nbits{nbits}"] = row
        del comp
    dump()


if __name__ == "__main__":
    main()
