"""The ctypes binding table is parsed from include/fusion_hip.h (fusion_amd/_lib.py): the parser against hand-stated prototypes, what it
refuses, Python's copies of the header's enumerators, and the library's dynamic symbols against the header's declarations."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from fusion_amd import _lib
from helpers import dynamic_fz_symbols

with open(os.path.join(ROOT, "include", "fusion_hip.h"), encoding="utf-8") as _h:
    HEADER_TEXT = _h.read()
_vp, _i, _i32, _i64, _sz, _d, _f = C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_size_t, C.c_double, C.c_float

# one entry per type the parser must know, stated by hand from the header's text
HAND = {
    "fz_strerror": (C.c_char_p, [_i]),                                    # returns const char*
    "fz_sort_workspace_bytes": (_sz, [_i, _i, _i]),                       # returns size_t
    "fz_abi_version": (_i, []),                                           # (void)
    "fz_fill_i32": (_i, [_vp, _sz, _i32, _vp]),                           # size_t and int32_t by value
    "fz_bm25_doc_norms_f64": (_i, [_vp, _i, _d, _d, _d, _vp, _vp]),       # three doubles
    "fz_sparse_feedback_f32": (_i, [_vp, _vp, _i, _i64, _i64, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _i, _i, _vp,
                                    _vp, _vp]),                          # float and int64_t mid-list
    "fz_dot_scores_filter_f32": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
}


def parse_enumerators(text: str) -> dict:
    """NAME -> int of every `NAME = int` inside an `enum { ... }` and of every `#define NAME int` of a C header."""
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*(?:/\*.*)?$", text, flags=re.M)}
    for body in re.findall(r"\benum\s*\w*\s*\{([^}]*)\}", _lib._strip_header(text)):
        out.update((m.group(1), int(m.group(2))) for m in re.finditer(r"(\w+)\s*=\s*(-?\d+)", body))
    return out


def test_parsed_table_against_hand_stated_prototypes():
    assert _lib.EXPORTS == tuple(_lib._PROTOS) and len(_lib._PROTOS) >= 129
    for name, proto in HAND.items():
        assert _lib._PROTOS[name] == proto, name
    for name, (res, args) in _lib._PROTOS.items():
        assert name.startswith("fz_") and res in (_i, _sz, C.c_char_p) and set(args) <= {_vp, _i, _i32, _i64, _sz, _d, _f}, name


def test_parser_reads_comments_line_breaks_and_arrays():
    text = """
    #define FZ_X 3
    /* int fz_in_a_comment(int a); */
    // int fz_in_a_line_comment(int a);
    typedef enum { FZ_A = 0, FZ_B = 1 } fz_kind;
    const char *fz_name(int status);
    size_t fz_bytes(const int32_t* lens, int n,
                    int64_t base);   /* fz_bytes(lens, n, base) in a trailing comment */
    int fz_none(void);
    int fz_plan(int n, int32_t out[4], const float x, void* stream);
    """
    assert _lib.parse_prototypes(text) == {"fz_name": (C.c_char_p, [_i]), "fz_bytes": (_sz, [_vp, _i, _i64]), "fz_none": (_i, []),
                                           "fz_plan": (_i, [_i, _vp, _f, _vp])}
    # a prototype may be the first thing after an opening brace, or the first thing in the text
    assert _lib.parse_prototypes('extern "C" {\nint fz_first(void);\n}') == {"fz_first": (_i, [])}
    assert _lib.parse_prototypes("int fz_only(int n);") == {"fz_only": (_i, [_i])}


@pytest.mark.parametrize("text, names", [
    ("int fz_f(unsigned n);", "unsigned n"),                              # an unknown by-value type
    ("int fz_f(const float* x, fz_norm norm, void* stream);", "fz_norm norm"),
    ("int fz_f(int);", "int"),                                            # no parameter name: not the header's form
    ("float fz_f(int n);", "float"),                                      # an unknown return type
    ("int fz_f(int (*cb)(int), void* stream);", "fz_f("),                 # a declaration it cannot read
    ("int fz_ok(int n);\nstatic inline int fz_g(int n) { return n; }", "fz_g("),
    ("int fz_ok(int n);\nint x = fz_h (3);", "fz_h("),
])
def test_parser_never_guesses(text, names):
    with pytest.raises(ImportError, match=re.escape(names)):
        _lib.parse_prototypes(text)


def test_python_copies_of_the_header_enumerators():
    from fusion_amd import ops
    E = parse_enumerators(HEADER_TEXT)
    assert {k: E[k] for k in ("FZ_OK", "FZ_ERR_ARG", "FZ_ERR_UNSUPPORTED", "FZ_ERR_HIP", "FZ_ERR_WORKSPACE")} == \
        dict(FZ_OK=_lib.FZ_OK, FZ_ERR_ARG=_lib.FZ_ERR_ARG, FZ_ERR_UNSUPPORTED=_lib.FZ_ERR_UNSUPPORTED, FZ_ERR_HIP=_lib.FZ_ERR_HIP,
             FZ_ERR_WORKSPACE=_lib.FZ_ERR_WORKSPACE)

    def values(prefix):
        return sorted(v for k, v in E.items() if k.startswith(prefix))
    # every enumerator of the typedef has its Python name (FZ_NORM_NONE is the passthrough: no name selects it), value for value
    assert _lib.NORMS == {"min-max": E["FZ_NORM_MINMAX"], "z-score": E["FZ_NORM_ZSCORE"], "arctan": E["FZ_NORM_ARCTAN"],
                          "percentile-rank": E["FZ_NORM_PERCENTILE"], "normal-curve-equivalent": E["FZ_NORM_NCE"]}
    assert values("FZ_NORM_") == sorted([E["FZ_NORM_NONE"], *_lib.NORMS.values()])
    assert _lib.RANK_METHODS == {"rrf": E["FZ_RRF"], "bcf": E["FZ_BCF"]}
    assert ops.LISTS_METHODS == {"rrf": E["FZ_LISTS_RRF"], "bcf": E["FZ_LISTS_BCF"], "wsum32": E["FZ_LISTS_WSUM_F32"], "wsum64": E["FZ_LISTS_WSUM_F64"]}
    assert values("FZ_LISTS_") == sorted(ops.LISTS_METHODS.values())
    assert ops.PAIR_MODES == {"longest_first": E["FZ_PAIR_LONGEST_FIRST"], "tail": E["FZ_PAIR_TAIL"]}
    assert ops.TABLES_PATHS == {E["FZ_TABLES_PATH_LDS_ALL"]: "lds-all", E["FZ_TABLES_PATH_LDS_SWAP"]: "lds-swap", E["FZ_TABLES_PATH_ROW"]: "row"}
    # LEXICAL_MODES: the header names no enumerator for the two walks, only the flag of fz_lexical_slice_docs(int tfidf): 'tfidf' is the
    # mode that sets it, and the two modes are its two values
    assert re.search(r"\bint\s+fz_lexical_slice_docs\s*\(\s*int\s+tfidf\s*\)", HEADER_TEXT)
    assert ops.LEXICAL_MODES["tfidf"] == 1 and sorted(ops.LEXICAL_MODES.values()) == [0, 1]


def test_library_defines_exactly_what_the_header_declares():
    defined = dynamic_fz_symbols(_lib.LIB_PATH)
    declared = set(_lib.EXPORTS)
    assert declared - defined == set(), f"declared in the header, not defined by the library: {sorted(declared - defined)}"
    assert defined - declared == set(), f"defined by the library, not declared in the header: {sorted(defined - declared)}"
