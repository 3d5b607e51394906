"""ctypes binding of libfusion_hip.so (C ABI: include/fusion_hip.h).

There is NO fallback: if the HIP library is missing or fails to load, importing the ops raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# FUSION_AMD_LIB: another build of the same library (the host-sanitized one of `make -C fusion_amd/csrc hostasan`); same ABI check applies
LIB_PATH = os.environ.get("FUSION_AMD_LIB") or os.path.join(_HERE, "libfusion_hip.so")
ABI_VERSION = 20

FZ_OK, FZ_ERR_ARG, FZ_ERR_UNSUPPORTED, FZ_ERR_HIP, FZ_ERR_WORKSPACE = 0, -1, -2, -3, -4
NORMS = {"min-max": 1, "z-score": 2, "arctan": 3, "percentile-rank": 4, "normal-curve-equivalent": 5}
RANK_METHODS = {"rrf": 0, "bcf": 1}


class FusionHipError(RuntimeError):
    def __init__(self, what: str, status: int, detail: str):
        super().__init__(f"{what}: {detail} (fz_status {status})")
        self.status = status


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into libfusion_hip.so (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    args = ["make", "-C", src_dir, "-j4", "-s"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


_lib = None

_HEADER = os.path.join(_HERE, os.pardir, "include", "fusion_hip.h")
_RESTYPES = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}
_BY_VALUE = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float}
_PROTO = re.compile(r"(?:^|[;{}])\s*(int|size_t|const\s+char\s*\*)\s*(fz_\w+)\s*\(([^()]*)\)\s*(?=;)")


def _strip_header(text: str) -> str:
    """The header without /* */ and // comments and without preprocessor lines (none of them is continued with a backslash)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)


def parse_prototypes(text: str) -> dict:
    """name -> (restype, [argtypes]) of every `T fz_name(args);` of a C header, T one of _RESTYPES.  It never guesses: a by-value type outside
    _BY_VALUE raises ImportError, and so does an `fz_name(` that is no such declaration."""
    text = _strip_header(text)
    protos = {}
    for ret, name, params in _PROTO.findall(text):
        params, args = " ".join(params.split()), []
        for prm in ([] if params in ("void", "") else params.split(",")):
            by_value = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s+\w+\s*", prm)
            if "*" in prm or "[" in prm:
                args.append(C.c_void_p)
            elif by_value and by_value.group(1) in _BY_VALUE:
                args.append(_BY_VALUE[by_value.group(1)])
            else:
                raise ImportError(f"fusion_hip.h: unknown by-value parameter {prm.strip()!r} in `{name}({params});`")
        protos[name] = (_RESTYPES[" ".join(ret.split()).replace(" *", "*")], args)
    for m in re.finditer(r"\b(fz_\w+)\s*\(", text):
        if m.group(1) not in protos:
            line = text[text.rfind("\n", 0, m.start()) + 1:].split("\n", 1)[0].strip()
            raise ImportError(f"fusion_hip.h: `{line}` names {m.group(1)}( but is no prototype this binding can read")
    return protos


def _table() -> dict:
    """_PROTOS: the binding table IS the header, parsed once per process on first use, so a prototype cannot drift from its ctypes signature
    (importing this module for build() or its constants reads no header)."""
    if "_PROTOS" not in globals():
        with open(_HEADER, encoding="utf-8") as f:
            protos = parse_prototypes(f.read())
        globals().update(_PROTOS=protos, EXPORTS=tuple(protos))
    return globals()["_PROTOS"]


def __getattr__(name):      # _lib._PROTOS and _lib.EXPORTS before the first lib()
    if name in ("_PROTOS", "EXPORTS"):
        _table()
        return globals()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). fusion_amd has no CPU or PyTorch fallback for the scoring/fusion path.")
        # torch FIRST: PyTorch-ROCm ships its own libamdhip64, and a process must hold ONE HIP runtime -- loaded before torch, this library
        # binds the system's copy, torch then brings its own, and every device pointer torch hands over is foreign to the runtime the kernels
        # launch through (hipErrorNoDevice on the first launch: seen with build() and smoke() in one process)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _table().items():
            f = getattr(L, name)  # AttributeError if the library does not export what the header declares
            f.restype, f.argtypes = res, args
        v = L.fz_abi_version()
        if v != ABI_VERSION:
            raise ImportError(f"libfusion_hip.so ABI {v} != binding ABI {ABI_VERSION}: rebuild")
        _lib = L
    return _lib


def check(status: int, what: str):
    if status != FZ_OK:
        L = lib()
        detail = L.fz_strerror(status).decode()
        if status == FZ_ERR_HIP:
            detail += f" [hipError {L.fz_last_hip_error()}]"
        raise FusionHipError(what, status, detail)
