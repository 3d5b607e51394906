"""The gold-rank counting kernels without a GPU: the two entries of csrc/bm25_count.hip and the two count entries of csrc/bm25_stream.hip are
exported, declared and refuse bad arguments before any HIP call, in the order of the other range entries of csrc/bm25_stream.hip; the
kernels' resource reports (no spills, no scratch, the count kernels' LDS exactly the walk's, their registers what they were)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SCORES = ("fz_bm25_doc_scores_pv_f64", "fz_tfidf_doc_scores_f64")
COUNTS = ("fz_bm25_count_pv_f64", "fz_tfidf_count_f64")
ENTRIES = SCORES + COUNTS
PV, TFIDF = 3584, 7168          # documents per workgroup slice of the two walks


def test_entries_are_exported_declared_and_additive():
    from fusion_amd import _lib
    L = _lib.lib()
    assert L.fz_abi_version() == 20 and _lib.ABI_VERSION == 20
    hdr = open(os.path.join(ROOT, "include", "fusion_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} is not declared in include/fusion_hip.h"
    from fusion_amd import ops
    assert callable(ops.lexical_doc_scores) and callable(ops.lexical_count)


P = 4096        # a fake, aligned, never dereferenced device pointer


def _call(L, name, **kw):
    """The entry with valid-looking arguments, overridden by kw (a pointer name -> 0 makes it null)."""
    tfidf, count = "tfidf" in name, "count" in name
    S = TFIDF if tfidf else PV
    a = dict(toff=P, pdoc=P, vals=P, idf=P, slice_off=0, qoff=P, qterms=P, Q=3, N=3 * S + 17, doc_lo=S, doc_hi=3 * S + 17, id_base=1 << 33,
             gold_scores=P, gold_ids=P, G=5, counts=P, docs=P, out=P)
    a.update(kw)
    p = lambda k: C.c_void_p(a[k]) if a[k] else None       # noqa: E731
    args = [p("toff"), p("pdoc"), p("vals")] + ([p("idf")] if tfidf else [])
    if count:
        args += [p("slice_off"), p("qoff"), p("qterms"), a["Q"], a["N"], a["doc_lo"], a["doc_hi"], a["id_base"], p("gold_scores"), p("gold_ids"),
                 a["G"], p("counts")]
    else:
        args += [p("qoff"), p("qterms"), a["Q"], a["N"], p("docs"), a["G"], p("out")]
    return getattr(L, name)(*args, None)


NULLS = dict(toff=0, pdoc=0, vals=0, idf=0, qoff=0, qterms=0, gold_scores=0, gold_ids=0, counts=0, docs=0, out=0)


@pytest.mark.parametrize("name", COUNTS)
def test_count_entries_check_arguments_before_any_hip_call_in_the_range_entries_order(name):
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, OK = _lib.FZ_ERR_ARG, _lib.FZ_OK
    tfidf = "tfidf" in name
    S = TFIDF if tfidf else PV
    N = 3 * S + 17
    # 1. sizes, the range and G
    assert _call(L, name, Q=-1) == ARG and _call(L, name, N=-1, doc_lo=0, doc_hi=0) == ARG
    for lo, hi in ((-S, S), (2 * S, S), (S, N + 1), (17, N), (S, 2 * S + 1), (PV if tfidf else 1, N)):
        assert _call(L, name, doc_lo=lo, doc_hi=hi) == ARG, (lo, hi)
    for lo, hi in ((0, S), (S, 3 * S), (2 * S, N), (0, N)):
        assert _call(L, name, doc_lo=lo, doc_hi=hi, Q=0) == OK, (lo, hi)
    for G in (0, -1):
        assert _call(L, name, G=G) == ARG
        assert _call(L, name, G=G, Q=0) == ARG and _call(L, name, G=G, doc_lo=S, doc_hi=S) == ARG      # G is judged before "nothing to do"
    # 2. nothing to do: FZ_OK with nothing launched, null pointers and all
    assert _call(L, name, Q=0, **NULLS) == OK
    assert _call(L, name, doc_lo=S, doc_hi=S, **NULLS) == OK
    assert _call(L, name, N=0, doc_lo=0, doc_hi=0, **NULLS) == OK
    # 3. a bad range or G beats a null pointer; then the pointers
    assert _call(L, name, doc_lo=17, **NULLS) == ARG and _call(L, name, G=0, **NULLS) == ARG
    for ptr in ["toff", "pdoc", "vals", "qoff", "qterms", "gold_scores", "gold_ids", "counts"] + (["idf"] if tfidf else []):
        assert _call(L, name, **{ptr: 0}) == ARG, ptr


@pytest.mark.parametrize("name", SCORES)
def test_doc_score_entries_check_arguments_before_any_hip_call(name):
    from fusion_amd import _lib
    L = _lib.lib()
    ARG, OK = _lib.FZ_ERR_ARG, _lib.FZ_OK
    assert _call(L, name, Q=-1) == ARG and _call(L, name, N=-1) == ARG
    for G in (0, -1):
        assert _call(L, name, G=G) == ARG and _call(L, name, G=G, Q=0) == ARG
    assert _call(L, name, Q=0, **NULLS) == OK
    assert _call(L, name, Q=-1, **NULLS) == ARG and _call(L, name, G=0, **NULLS) == ARG
    for ptr in ["toff", "pdoc", "vals", "qoff", "qterms", "docs", "out"] + (["idf"] if "tfidf" in name else []):
        assert _call(L, name, **{ptr: 0}) == ARG, ptr


@pytest.fixture(scope="module")
def resources():
    res = kernel_resources.load()
    if "bm25_count" not in res:
        pytest.skip("no .res reports next to the objects: run `make -C fusion_amd/csrc` where ROCm is installed")
    return res


def test_count_kernels_hold_everything_in_registers_and_exactly_the_walks_lds(resources):
    ks = {kernel_resources.short(n): k for n, k in resources["bm25_count"].items()}
    assert sorted(ks) == sorted(f"lexical_doc_scores_kernel<{m}>" for m in (1, 2))
    # the counting walk: csrc/bm25_stream.hip's lexical_range_kernel<MODE, EPI> with EPI = 2 (LEX_COUNT)
    counts = {kernel_resources.short(n): k for n, k in resources["bm25_stream"].items() if kernel_resources.short(n).endswith(", 2>")}
    assert sorted(counts) == sorted(f"lexical_range_kernel<{m}, 2>" for m in (1, 2))
    ks.update(counts)
    tables = 3 * 256 * 8                                              # s_e0, s_e1, s_w: BM25_TERMS entries each
    for name, k in ks.items():
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
        if name in counts:                                            # accumulators + term tables: the epilogue has no LDS of its own
            assert k["lds"] == (28 if "<2," in name else 56) * 1024 + tables, (name, k["lds"])
        else:
            assert k["lds"] == 0, (name, k["lds"])
    # VGPRs, SGPRs, LDS, occupancy of the count when it was a kernel of its own in csrc/bm25_count.hip (waves_per_eu(8, 8): 72 SGPRs, not 101)
    want = {"lexical_range_kernel<2, 2>": (58, 72, 34816, 8), "lexical_range_kernel<1, 2>": (51, 72, 63488, 8)}
    for name, (vgprs, sgprs, lds, occupancy) in want.items():
        k = counts[name]
        assert (k["vgprs"], k["sgprs"], k["agprs"], k["lds"], k["occupancy"]) == (vgprs, sgprs, 0, lds, occupancy), (name, k)
