#!/usr/bin/env python3
"""ColBERT MaxSim over e4m3 tokens (ops.maxsim_e4m3, csrc/maxsim8.hip) against the float16 kernel (ops.maxsim), one process, one GPU.

  timing   the two kernels at Lq = 64 over N = 27,942 documents of LLeQA-shaped lengths (clip(N(300, 120), 16, 512), as
           tools/bench_kernels.py), Q = 1024 and Q = 195: the routes ALTERNATE call by call after a warm-up, each call timed with its own
           pair of events, medians reported; plus the quantiser over the whole corpus matrix and over the queries.
  quality  (a) unit-norm random tokens, (b) the tokens of a base-size random-init ColBERT encoder over synthetic passages: max and mean
           |s_e4m3 - s_f16|, mean overlap of the two rankings' top 10 and top 100, and how often the top-1 document agrees.

One JSON document -> --out (default profiles/r24_maxsim_fp8.json).  Counters (MFMA busy, VALU issue, LDS bank conflicts) are not taken
here: collect them with `rocprofv3 --pmc ... -- python tools/bench_maxsim_fp8.py --only timing --queries 1024 --reps 1` in a run of their own.
Usage: python tools/bench_maxsim_fp8.py [--reps 9] [--only timing,unit,encoder] [--queries 1024,195] [--passages 3000]
       [--variant-lib tools/ablate/libfusion_abl_m8_cb16.so] [--out FILE]"""
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
from fusion_amd import ops  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(routes: dict, reps: int, warm: int = 2):
    """{name: fn} -> {name: [ms] * reps}, the routes called in turn."""
    for _ in range(warm):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    return ms


def variant_maxsim(lib, Q8, D8, Doff, max_doc_len, descale_exp, out):
    """fz_maxsim_e4m3 of another build, called as ops.maxsim_e4m3 calls the shipped one."""
    Q, Lq, dim = Q8.shape
    rc = lib.fz_maxsim_e4m3(Q8.data_ptr(), D8.data_ptr(), Doff.data_ptr(), D8.shape[0], max_doc_len, Q, Lq, Doff.numel() - 1, dim, descale_exp,
                            out.data_ptr(), out.stride(0), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def summary(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4), n=len(xs))


def lleqa_corpus(N, seed=0):
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.normal(300, 120, N), 16, 512).astype(np.int64)
    off = np.zeros(N + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    g = torch.Generator(device="cuda").manual_seed(2)
    sumL = int(off[-1])
    Dtok = torch.empty((sumL, 128), dtype=torch.float16, device="cuda")
    for c0 in range(0, sumL, 1 << 20):
        c1 = min(sumL, c0 + (1 << 20))
        Dtok[c0:c1] = torch.nn.functional.normalize(torch.randn((c1 - c0, 128), generator=g, device="cuda"), dim=-1).half()
    return Dtok, torch.from_numpy(off).cuda(), g


def quality(Qtok, Dtok, Doff, max_doc_len):
    s16 = ops.maxsim(Qtok, Dtok, Doff, max_doc_len=max_doc_len)
    s8 = ops.maxsim_e4m3(ops.quantize_e4m3(Qtok), ops.quantize_e4m3(Dtok), Doff, max_doc_len=max_doc_len)
    d = (s8 - s16).abs()
    out = dict(Q=int(s16.shape[0]), N=int(s16.shape[1]), max_abs_diff=float(d.max()), mean_abs_diff=float(d.mean()),
               score_mean=float(s16.mean()), score_std_within_query=float(s16.std(dim=1).mean()))
    for k in (10, 100):
        if s16.shape[1] < k:
            continue
        a, b = s16.topk(k, dim=1).indices, s8.topk(k, dim=1).indices
        both = (a.unsqueeze(2) == b.unsqueeze(1)).any(dim=2).float().sum(dim=1) / k
        out[f"top{k}_overlap_mean"] = float(both.mean())
        out[f"top{k}_overlap_min"] = float(both.min())
    out["top1_agree"] = float((s16.argmax(dim=1) == s8.argmax(dim=1)).float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="timing,unit,encoder")
    ap.add_argument("--docs", type=int, default=27942)
    ap.add_argument("--queries", default="1024,195", help="batch sizes of the timing part")
    ap.add_argument("--passages", type=int, default=3000)
    ap.add_argument("--variant-lib", default=None, help="another build of the library (tools/ablate/maxsim8_variants.py): its fz_maxsim_e4m3 "
                    "is timed as a third route of the same alternation and its score plane compared with the shipped kernel's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_maxsim_fp8.json"))
    a = ap.parse_args()
    only = set(a.only.split(","))
    res = dict(tool="tools/bench_maxsim_fp8.py", device=torch.cuda.get_device_name(0), reps=a.reps,
               kernel=dict(instruction="v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 x e4m3, both scales 2^0", tile_rows=32, column_blocks_per_wave=8,
                           variants_not_built=["64-row tiles"], variant_builds="tools/ablate/maxsim8_variants.py (16 column blocks per wave): --variant-lib"))
    Dtok = Doff = None
    variant = None
    if a.variant_lib:
        variant = C.CDLL(os.path.abspath(a.variant_lib))
        variant.fz_maxsim_e4m3.restype = C.c_int
        variant.fz_maxsim_e4m3.argtypes = [C.c_void_p] * 3 + [C.c_int64] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p]
    if only & {"timing", "unit"}:
        Dtok, Doff, g = lleqa_corpus(a.docs)
        sumL, N = int(Dtok.shape[0]), a.docs
    if "timing" in only:
        D8 = ops.quantize_e4m3(Dtok)
        rows = []
        for Q in [int(x) for x in a.queries.split(",")]:
            Qtok = torch.nn.functional.normalize(torch.randn((Q, 64, 128), generator=g, device="cuda"), dim=-1).half()
            Q8 = ops.quantize_e4m3(Qtok)
            o16, o8 = ops.alloc_plane(Q, N, torch.float32, "cuda"), ops.alloc_plane(Q, N, torch.float32, "cuda")
            routes = {"f16": lambda: ops.maxsim(Qtok, Dtok, Doff, out=o16, max_doc_len=512),
                      "e4m3": lambda: ops.maxsim_e4m3(Q8, D8, Doff, out=o8, max_doc_len=512)}
            if variant is not None:
                ov = ops.alloc_plane(Q, N, torch.float32, "cuda")
                routes["e4m3_variant"] = lambda: variant_maxsim(variant, Q8, D8, Doff, 512, 16, ov)
            ms = alternate(routes, a.reps)
            flop = 2.0 * Q * 64 * sumL * 128
            f, e = summary(ms["f16"]), summary(ms["e4m3"])
            rows.append(dict(Q=Q, Lq=64, N=N, sumL=sumL, f16=f, e4m3=e, speedup=round(f["median_ms"] / e["median_ms"], 3),
                             f16_pflops=round(flop / f["median_ms"] / 1e12, 3), e4m3_pflops=round(flop / e["median_ms"] / 1e12, 3),
                             quantize_queries=summary(alternate({"q": lambda: ops.quantize_e4m3(Qtok)}, a.reps)["q"])))
            if variant is not None:
                v = summary(ms["e4m3_variant"])
                rows[-1].update(e4m3_variant=v, variant_lib=os.path.basename(a.variant_lib), variant_over_shipped=round(e["median_ms"] / v["median_ms"], 3),
                                variant_plane_equals_shipped=bool(torch.equal(ov, o8)))
                del ov
            print(json.dumps(rows[-1]), flush=True)
            del o16, o8
        res["timing"] = rows
        qms = summary(alternate({"q": lambda: ops.quantize_e4m3(Dtok)}, a.reps)["q"])
        res["quantize_corpus"] = dict(values=sumL * 128, **qms, gb_per_s=round(sumL * 128 * 3 / qms["median_ms"] / 1e6, 1),
                                      note="includes the allocation of the output tensor; 2 bytes read + 1 written per value")
        print(json.dumps(res["quantize_corpus"]), flush=True)
        del D8
    if "unit" in only:
        Qtok = torch.nn.functional.normalize(torch.randn((195, 64, 128), generator=g, device="cuda"), dim=-1).half()
        res["quality_unit_norm_random"] = quality(Qtok, Dtok, Doff, 512)
        print(json.dumps(res["quality_unit_norm_random"]), flush=True)
    del Dtok, Doff
    torch.cuda.empty_cache()
    if "encoder" in only:
        from fusion_amd import encoders
        from fusion_amd.synth_text import FrenchLike
        rng = np.random.default_rng(24)
        text = FrenchLike(n_words=30000, seed=24)
        docs = [" ".join(text.sentences(rng, int(rng.integers(2, 9)), 8, 30)) for _ in range(a.passages)]
        queries = text.sentences(rng, 195, 6, 24, question=True)
        enc = encoders.random_init("colbert", device="cuda", size="base", seed=24)
        Dt, Do = (t.cuda() for t in enc.encode_docs(docs, batch_size=64))
        Qt = enc.encode_queries(queries, batch_size=64).cuda()
        res["quality_base_random_init_colbert"] = dict(passages=a.passages, tokens=int(Dt.shape[0]), amp=bool(getattr(enc, "amp", False)),
                                                       **quality(Qt, Dt, Do, enc.max_doc_length))
        print(json.dumps(res["quality_base_random_init_colbert"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
