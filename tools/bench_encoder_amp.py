"""The mixed-precision switch of the DPR and SPLADE encoders (`amp=True`) against their float32 defaults, and the float16 SPLADE head
against the float32 one.  Three parts, each with its routes alternated call by call in ONE process (drift on a shared machine hits both
alike), device times from HIP events:

  head     fz_splade_head_max_f32 against fz_splade_head_max_f16 alone at T = 65,536 token rows, V = 32,005, d = 768 on RANDOM data (zeroed
           operands inflate matrix rates), sequences of 300 rows: ms and TFLOP/s (2 T V d per call)
  queries  encode_ids_packed of Q = 1024 queries (token counts ~ N(36, 12) in [4, 64]) for DPR and SPLADE, float32 against amp, with the
           time between the encoders' `mark` calls summed per stage ("encode_gemm", "encode_attn", "splade_head_pool" / "splade_head_pool_f16", ...)
  corpus   one SPLADE corpus sub-batch of 65,536 token rows (documents ~ N(300, 100) tokens in [16, 512]), the same two routes

Encoders are random_init(size="base") (CamemBERT-base shape); hipBLASLt GEMM tuning is left off unless --gemm-tuning is given.

Usage: python tools/bench_encoder_amp.py [--reps 5] [--queries 1024] [--rows 65536] [--skip head,queries,corpus] [--out profiles/r23_encoder_amp.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fusion_amd import encoders, ops  # noqa: E402


def device_ms(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = f()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e)


def staged(f):
    """f(mark) with a HIP event per mark -> (result, total ms, {stage: ms})."""
    evs = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append((name, e))
    s = torch.cuda.Event(enable_timing=True)
    s.record()
    out = f(mark)
    mark("rest")
    torch.cuda.synchronize()
    stages, prev = {}, s
    for name, e in evs:
        stages[name] = stages.get(name, 0.0) + prev.elapsed_time(e)
        prev = e
    return out, s.elapsed_time(evs[-1][1]), {k: round(v, 4) for k, v in stages.items()}


def med(xs):
    return round(float(np.median(xs)), 4)


def bench_head(a):
    T, V, d = a.rows, 32005, 768
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((T, d), generator=g, device="cuda")
    w = 0.02 * torch.randn((V, d), generator=g, device="cuda")
    bias = 0.5 * torch.randn(V, generator=g, device="cuda")
    x16, w16 = x.half(), w.half()
    cu = torch.arange(0, T + 1, 300, dtype=torch.int32)
    if int(cu[-1]) != T:
        cu = torch.cat([cu, torch.tensor([T], dtype=torch.int32)])
    cu = cu.cuda()
    routes = {"f32": lambda: ops.splade_head_max(x, w, bias, cu), "f16": lambda: ops.splade_head_max_f16(x16, w16, bias, cu)}
    last, ms = {}, {n: [] for n in routes}
    for f in routes.values():
        f()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for n, f in routes.items():
            last[n], t = device_ms(f)
            ms[n].append(t)
    flop = 2.0 * T * V * d
    diff = float((last["f16"] - last["f32"]).abs().max())
    return dict(T=T, V=V, d=d, sequences=int(cu.numel() - 1), flop=flop, max_abs_diff_f16_vs_f32=diff,
                **{n: dict(ms=med(v), tflops=round(flop / (med(v) * 1e-3) / 1e12, 1), calls_ms=[round(t, 4) for t in v]) for n, v in ms.items()})


def token_rows(rng, n, mean, spread, lo, hi, vocab=32000):
    lens = np.clip(rng.normal(mean, spread, n).astype(np.int64), lo, hi)
    ids = rng.integers(7, vocab - 1, size=(n, int(lens.max())))
    ids[:, 0] = 5
    return torch.from_numpy(ids).cuda(), lens


def bench_encode(enc, ids, lens, reps):
    runs = {False: [], True: []}
    out = {}
    for amp in (False, True):                       # one warm-up call each (weight conversion, workspace growth)
        enc.amp = amp
        enc.encode_ids_packed(ids, lens)
    torch.cuda.synchronize()
    for _ in range(reps):
        for amp in (False, True):
            enc.amp = amp
            out[amp], total, stages = staged(lambda mark: enc.encode_ids_packed(ids, lens, mark=mark))
            runs[amp].append(dict(total_ms=round(total, 4), **stages))
    res = {}
    for amp, name in ((False, "f32"), (True, "amp")):
        keys = sorted({k for r in runs[amp] for k in r})
        res[name] = {k: med([r.get(k, 0.0) for r in runs[amp]]) for k in keys}
    res["speedup"] = round(res["f32"]["total_ms"] / res["amp"]["total_ms"], 3)
    res["max_abs_diff"] = float((out[True] - out[False]).abs().max())
    res["token_rows"] = int(np.sum(lens))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--skip", default="")
    ap.add_argument("--gemm-tuning", action="store_true", help="encoders.enable_gemm_tuning(): the recorded hipBLASLt solutions of the float32 Linears")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_encoder_amp.json"))
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))
    if a.gemm_tuning:
        encoders.enable_gemm_tuning()
    rng = np.random.default_rng(23)
    out = dict(tool="tools/bench_encoder_amp.py", device=torch.cuda.get_device_name(0), reps=a.reps, gemm_tuning=bool(a.gemm_tuning),
               model='random_init(size="base")')
    if "head" not in skip:
        out["head"] = bench_head(a)
        print(json.dumps({"head": {k: v for k, v in out["head"].items()}}), flush=True)
        torch.cuda.empty_cache()
    for kind in ("dpr", "splade"):
        if "queries" in skip and ("corpus" in skip or kind == "dpr"):
            continue
        enc = encoders.random_init(kind, device="cuda", size="base", seed=5, amp=True)
        if kind == "splade":
            enc.calibrate_sparsity()
        if "queries" not in skip:
            qids, qlens = token_rows(rng, a.queries, 36, 12, 4, 64)
            out[f"{kind}_queries"] = dict(Q=a.queries, **bench_encode(enc, qids, qlens, a.reps))
            print(json.dumps({f"{kind}_queries": out[f"{kind}_queries"]}), flush=True)
        if kind == "splade" and "corpus" not in skip:
            dids, dlens = token_rows(rng, 400, 300, 100, 16, 512)
            keep = int(np.searchsorted(np.cumsum(dlens), a.rows, side="right"))
            dids, dlens = dids[:keep], dlens[:keep]
            out["splade_corpus_subbatch"] = dict(documents=keep, **bench_encode(enc, dids, dlens, max(2, a.reps // 2)))
            print(json.dumps({"splade_corpus_subbatch": out["splade_corpus_subbatch"]}), flush=True)
        del enc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
