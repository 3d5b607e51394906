"""The streamed lexical top-k without a GPU: the four entries of csrc/bm25_stream.hip are exported, declared and refuse bad arguments before any
HIP call; LexicalStats merges to the whole corpus's statistics and a shard built with them has the whole model's idf and avgdl bit for
bit; the new kernels' resource reports (no spills, no scratch, the stated LDS) and bm25_kernel's, which this change must not move."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

ENTRIES = ("fz_bm25_scores_range_pv_f64", "fz_tfidf_scores_range_f64", "fz_bm25_filter_pv_f64", "fz_tfidf_filter_f64")
PV, TFIDF = 3584, 7168          # documents per workgroup slice of the two walks


def test_entries_are_exported_declared_and_additive():
    from fusion_amd import _lib
    L = _lib.lib()
    assert L.fz_abi_version() == 20 and _lib.ABI_VERSION == 20
    hdr = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    for name in ENTRIES + ("fz_lexical_slice_docs",):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} is not declared in include/fusion_hip.h"
    assert L.fz_lexical_slice_docs(0) == PV == L.fz_bm25_slice_docs() and L.fz_lexical_slice_docs(1) == TFIDF == 2 * L.fz_bm25_slice_docs()


P = 4096        # a fake, aligned, never dereferenced device pointer


def _call(L, name, **kw):
    """The entry with valid-looking arguments, overridden by kw (a pointer name -> 0 makes it null)."""
    tfidf, filt = "tfidf" in name, "filter" in name
    S = TFIDF if tfidf else PV
    a = dict(toff=P, pdoc=P, vals=P, idf=P, slice_off=0, qoff=P, qterms=P, Q=3, N=3 * S + 17, doc_lo=S, doc_hi=3 * S + 17, id_base=1 << 33,
             tau=P, cand_s=P, cand_i=P, cand_len=P, cap=64, overflow=P, scores=P, lds=2 * S + 17)
    a.update(kw)
    p = lambda k: C.c_void_p(a[k]) if a[k] else None       # noqa: E731
    args = [p("toff"), p("pdoc"), p("vals")] + ([p("idf")] if tfidf else []) + [p("slice_off"), p("qoff"), p("qterms"), a["Q"], a["N"], a["doc_lo"], a["doc_hi"]]
    if filt:
        args += [a["id_base"], p("tau"), p("cand_s"), p("cand_i"), p("cand_len"), a["cap"], p("overflow")]
    else:
        args += [p("scores"), a["lds"]]
    return getattr(L, name)(*args, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_argument_checks_come_before_any_hip_call_in_the_sparse_entries_order(name):
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, OK = _lib.FZ_ERR_ARG, _lib.FZ_OK
    tfidf, filt = "tfidf" in name, "filter" in name
    S = TFIDF if tfidf else PV
    N = 3 * S + 17
    # 1. sizes and the range
    assert _call(L, name, Q=-1) == ARG and _call(L, name, N=-1, doc_lo=0, doc_hi=0) == ARG
    for lo, hi in ((-S, S), (2 * S, S), (S, N + 1), (17, N), (S, 2 * S + 1), (PV if tfidf else 1, N)):
        assert _call(L, name, doc_lo=lo, doc_hi=hi) == ARG, (lo, hi)
    for lo, hi in ((0, S), (S, 3 * S), (2 * S, N), (0, N)):
        assert _call(L, name, doc_lo=lo, doc_hi=hi, lds=N, Q=0) == OK, (lo, hi)
    if filt:
        assert _call(L, name, cap=0) == ARG and _call(L, name, cap=-5) == ARG
        assert _call(L, name, cap=0, Q=0) == ARG                      # cap is judged before "nothing to do"
    else:
        assert _call(L, name, lds=2 * S + 16) == ARG and _call(L, name, lds=2 * S + 16, Q=0) == ARG
    # 2. nothing to do: FZ_OK with nothing launched, null pointers and all
    nulls = dict(toff=0, pdoc=0, vals=0, idf=0, qoff=0, qterms=0, tau=0, cand_s=0, cand_i=0, cand_len=0, overflow=0, scores=0)
    assert _call(L, name, Q=0, **nulls) == OK
    assert _call(L, name, doc_lo=S, doc_hi=S, **nulls) == OK
    assert _call(L, name, N=0, doc_lo=0, doc_hi=0, lds=0, **nulls) == OK
    # 3. a bad range beats a null pointer; then the pointers
    assert _call(L, name, doc_lo=17, **nulls) == ARG
    required = ["toff", "pdoc", "vals", "qoff", "qterms"] + (["idf"] if tfidf else []) + (["tau", "cand_s", "cand_i", "cand_len", "overflow"] if filt else ["scores"])
    for ptr in required:
        assert _call(L, name, **{ptr: 0}) == ARG, ptr


def _docs(n, seed=3):
    rng = np.random.default_rng(seed)
    vocab = np.array([f"w{i}" for i in range(400)])
    p = 1.0 / np.arange(1, 401); p /= p.sum()
    return [" ".join(rng.choice(vocab, size=int(rng.integers(1, 25)), p=p)) for _ in range(n)]


@pytest.mark.parametrize("name", ["TFIDF", "BM25", "AtireBM25"])
def test_lexical_stats_of_eight_shards_are_the_whole_corpus(name):
    from fusion_amd.distributed import shard_bounds
    from fusion_amd.retrievers import bm25
    cls = getattr(bm25, name)
    mk = (lambda d, **kw: cls(d, device="cpu", **kw)) if name == "TFIDF" else (lambda d, **kw: cls(d, 1.2, 0.6, device="cpu", **kw))
    docs = _docs(1003)
    whole = mk(docs)
    ws = whole.stats()
    assert ws.n_docs == 1003 and ws.total_len == sum(len(d.split()) for d in docs) and ws.df["w0"] == sum("w0" in d.split() for d in docs)
    bounds = [shard_bounds(len(docs), 8, r) for r in range(8)]
    merged = bm25.LexicalStats.merge([mk(docs[lo:hi]).stats() for lo, hi in bounds])
    assert merged == ws and merged.df == ws.df and (merged.n_docs, merged.total_len) == (ws.n_docs, ws.total_len)
    assert merged.avgdl == ws.total_len / ws.n_docs
    for lo, hi in bounds:
        shard = mk(docs[lo:hi], stats=merged, id_base=(1 << 33) + lo)
        assert shard.id_base == (1 << 33) + lo and shard.corpus_size == hi - lo
        for w, t in shard.vocab.items():                              # every shared word: the whole model's idf, bitwise
            assert shard.idf_host[t].tobytes() == whole.idf_host[whole.vocab[w]].tobytes(), w
        if name != "TFIDF":
            assert np.float64(shard.avgdl).tobytes() == np.float64(whole.avgdl).tobytes()
        # postings and vocabulary stay the shard's own
        own = mk(docs[lo:hi])
        assert shard.vocab == own.vocab and np.array_equal(shard.df_host, own.df_host) and np.array_equal(shard._pdoc_host, own._pdoc_host)
        assert np.array_equal(shard._ptf_host, own._ptf_host) and np.array_equal(shard.doc_len_host, own.doc_len_host)


@pytest.mark.parametrize("name", ["TFIDF", "BM25", "AtireBM25"])
def test_without_stats_the_tables_are_the_reference_formulas(name):
    """No `stats`: idf from the index's own N and df, avgdl = statistics.mean of its lengths -- what the constructor made before."""
    import math
    from statistics import mean
    from fusion_amd.retrievers import bm25
    cls = getattr(bm25, name)
    docs = _docs(257, seed=4)
    m = cls(docs, device="cpu") if name == "TFIDF" else cls(docs, 1.2, 0.6, device="cpu")
    assert m.global_stats is None and m.id_base == 0
    N = len(docs)
    df = {}
    for d in docs:
        for w in set(d.split()):
            df[w] = df.get(w, 0) + 1
    for w, t in m.vocab.items():
        want = math.log10((N - df[w] + 0.5) / (df[w] + 0.5)) if name == "BM25" else math.log10((N + 1) / (df[w] + 1))
        assert m.idf_host[t] == want and m.df_host[t] == df[w]
    if name != "TFIDF":
        assert m.avgdl == float(mean(len(d.split()) for d in docs)) == m.stats().avgdl


@pytest.fixture(scope="module")
def resources():
    res = kernel_resources.load()
    if "bm25_stream" not in res or "bm25" not in res:
        pytest.skip("no .res reports next to the objects: run `make -C fusion_amd/csrc` where ROCm is installed")
    return res


def test_range_kernels_hold_everything_in_registers_and_the_stated_lds(resources):
    ks = {kernel_resources.short(n): k for n, k in resources["bm25_stream"].items()}
    # <MODE, EPI>: MODE 1 = BM25_TFIDF, 2 = BM25_PVAL; EPI 0 = LEX_PLANE, 1 = LEX_FILTER, 2 = LEX_COUNT (tests/test_bm25_count_cpu.py's)
    assert sorted(ks) == sorted(f"lexical_range_kernel<{mode}, {epi}>" for mode in (1, 2) for epi in (0, 1, 2))
    ks = {name: k for name, k in ks.items() if not name.endswith(", 2>")}
    tables = 3 * 256 * 8                                              # s_e0, s_e1, s_w: BM25_TERMS entries each
    for name, k in ks.items():
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
        acc = (28 if "<2," in name else 56) * 1024                    # the slice's float64 accumulators: BM25_PVAL 28 KiB, BM25_TFIDF 56 KiB
        extra = k["lds"] - acc - tables
        assert extra == 0 if ", 0>" in name else 0 <= extra <= 256, (name, k["lds"])   # (the filter's workgroup-wide overflow vote)
    # VGPRs, SGPRs, LDS, occupancy of lexical_range_kernel<MODE, bool FILTER> before the count became its third epilogue
    want = {"lexical_range_kernel<2, 0>": (60, 56, 34816, 8), "lexical_range_kernel<1, 0>": (32, 58, 63488, 8),
            "lexical_range_kernel<2, 1>": (60, 66, 34816, 8), "lexical_range_kernel<1, 1>": (33, 67, 63488, 8)}
    assert sorted(want) == sorted(ks)
    for name, (vgprs, sgprs, lds, occupancy) in want.items():
        k = ks[name]
        assert (k["vgprs"], k["sgprs"], k["agprs"], k["lds"], k["occupancy"]) == (vgprs, sgprs, 0, lds, occupancy), (name, k)


def test_bm25_kernel_resources_are_what_they_were(resources):
    ks = {kernel_resources.short(n): k for n, k in resources["bm25"].items()}
    want = {"bm25_kernel<2>": (58, 58), "bm25_kernel<1>": (32, 60), "bm25_kernel<0>": (44, 62)}       # VGPRs, SGPRs before this file existed
    for name, (vgprs, sgprs) in want.items():
        k = ks[name]
        assert (k["vgprs"], k["sgprs"], k["agprs"]) == (vgprs, sgprs, 0), (name, k)
        assert (k["vgpr_spill"], k["sgpr_spill"], k["scratch"], k["lds"], k["occupancy"]) == (0, 0, 0, 6144, 8), (name, k)
