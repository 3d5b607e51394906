"""torch-tensor wrappers over the C ABI (include/fusion_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every op below passes
raw device pointers + the stream to libfusion_hip.so.  No op has a PyTorch/CPU fallback: a CPU tensor
raises, a missing library raises (see _lib.lib()).

"Plane" = 2-D tensor [rows, n] with stride (ld, 1), ld >= n, ld a multiple of 64 elements so every row
starts on a 256-byte boundary (16-byte vector loads).
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import NORMS, RANK_METHODS, check

_PAD = 64


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def alloc_plane(rows: int, n: int, dtype, device, fill=None) -> torch.Tensor:
    ld = max(round_up(n, _PAD), _PAD)
    base = torch.empty((max(rows, 1), ld), dtype=dtype, device=device) if fill is None else \
        torch.full((max(rows, 1), ld), fill, dtype=dtype, device=device)
    return base[:rows, :n]


def as_plane(t: torch.Tensor) -> torch.Tensor:
    """Return t if rows are 16-byte aligned with unit inner stride, else copy it into a padded plane."""
    assert t.dim() == 2
    esz = t.element_size()
    row_ok = t.shape[0] <= 1 or (t.stride(0) >= t.shape[1] and (t.stride(0) * esz) % 16 == 0)
    if t.stride(1) == 1 and row_ok and t.data_ptr() % 16 == 0:
        return t
    p = alloc_plane(t.shape[0], t.shape[1], t.dtype, t.device)
    p.copy_(t)
    return p


def _ld(t: torch.Tensor) -> int:
    if t.shape[0] > 1:
        return t.stride(0)
    return max(t.stride(0), t.shape[1]) if t.dim() == 2 else t.shape[-1]


def _dev(t: torch.Tensor, dtype=None, what="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{what}: expected a tensor on the GPU (fusion_amd has no CPU path), got {type(t).__name__}"
                        f"{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{what}: expected dtype {dtype}, got {t.dtype}")
    if t.dim() >= 1 and t.numel() > 0 and t.stride(-1) != 1:
        raise ValueError(f"{what}: innermost dimension must be contiguous")
    return t


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need(cond: bool, msg: str):
    """Host-side shape contract of a kernel launch: a mismatch would be an out-of-bounds access on the device."""
    if not cond:
        raise ValueError(msg)


def check_pair_plane(P, Q: int, W: int, who: str) -> torch.Tensor:
    """The contract of a pair scorer's result for ids [Q, W] -- a float32 or float64 tensor of shape (Q, W) -- under the caller's name for
    the scorer (`who`: the start of the message)."""
    if not isinstance(P, torch.Tensor) or P.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who} must return a float32 or float64 tensor")
    if tuple(P.shape) != (Q, W):
        raise ValueError(f"{who} returned {tuple(P.shape)} for ids {(Q, W)}")
    return P


MAX_SYSTEMS = 8   # FZ_MAX_SYSTEMS (csrc/common.h): every fusion kernel's argument block holds this many systems


def _max_systems(S: int, what: str):
    """Host-side system-count contract of the fusion entry points, checked before any tensor is looked at: the C ABI would only
    answer a generic FZ_ERR_ARG."""
    _need(S <= MAX_SYSTEMS, f"{what}: {S} systems, but fusion takes at most {MAX_SYSTEMS} (FZ_MAX_SYSTEMS)")


def _contiguous(what: str, *typed):
    """Every (tensor, dtype, name) is a contiguous device tensor of its dtype: the flat arrays an index or a query batch is made of."""
    for t, dt, name in typed:
        _need(_dev(t, dt, f"{what}({name})").is_contiguous(), f"{what}({name}) must be contiguous")


def _out(what: str, out, shape: tuple, dtype, dev, plane: bool) -> torch.Tensor:
    """An op's `out`: None -> a new tensor of this shape (a padded plane, or plain rows); a caller's -> checked to be one of this shape."""
    if out is None:
        return alloc_plane(*shape, dtype, dev) if plane else torch.empty(shape, dtype=dtype, device=dev)
    _dev(out, dtype, f"{what}(out)")
    _need(tuple(out.shape) == shape, f"{what}(out): expected shape {shape}, got {tuple(out.shape)}")
    return out


def _same_shape(ts, what: str):
    shapes = {tuple(t.shape) for t in ts if t is not None}
    _need(len(shapes) <= 1, f"{what}: planes differ in shape: {sorted(shapes)}")


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


_RESERVED_WS: dict = {}


def _reserved_workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """A workspace that a kernel RESERVES but practically never touches (the fused sort's plane for rows its fast form flags: rows x ld x 8
    bytes, 229 MB at 1024 x 27,942), kept per (device, stream) and grown on demand instead of being taken from the allocator on every call
    (ADVICE r5).  Safe because calls on one stream are ordered and the kernel initialises what it reads (its row flags) itself; another
    stream gets its own buffer."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    ws = _RESERVED_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        _RESERVED_WS.pop(key, None)
        ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
        _RESERVED_WS[key] = ws
    return ws


def _ptr_array(ts):
    A = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        A[i] = None if t is None else t.data_ptr()
    return A


def _same_ld(*ts):
    lds = {_ld(t) for t in ts if t is not None and t.shape[0] > 1}
    if len(lds) > 1:
        raise ValueError(f"planes passed to one call must share the row stride, got {sorted(lds)}")
    return lds.pop() if lds else max(_ld(t) for t in ts if t is not None)


def harmonise(ts: list):
    """One C-ABI call takes ONE row stride for all its planes: copy the odd ones out (None entries pass through)."""
    real = [t for t in ts if t is not None]
    if not real:
        return ts
    rows, n = real[0].shape
    want = max(round_up(n, _PAD), _PAD)
    lds = {_ld(t) for t in real} if rows > 1 else {want}
    if len(lds) == 1 and all(t.data_ptr() % 16 == 0 and t.stride(1) == 1 for t in real):
        return ts
    out = []
    for t in ts:
        if t is None or (rows > 1 and _ld(t) == want and t.data_ptr() % 16 == 0 and t.stride(1) == 1):
            out.append(t)
        else:
            p = alloc_plane(rows, n, t.dtype, t.device)
            p.copy_(t)
            out.append(p)
    return out


# ---------------------------------------------------------------------------------------
# K1 scoring
# ---------------------------------------------------------------------------------------
def pad_dim(X: torch.Tensor, mult: int = 4) -> torch.Tensor:
    """Zero-pad the embedding dimension to a multiple of `mult` floats and 16-byte row alignment
    (zeros change neither norms nor dot products)."""
    d = X.shape[1]
    dp = round_up(d, mult)
    if dp == d and X.stride(0) % 4 == 0 and X.data_ptr() % 16 == 0 and X.stride(1) == 1:
        return X
    Y = torch.zeros((X.shape[0], dp), dtype=X.dtype, device=X.device)
    Y[:, :d] = X
    return Y


def normalize_rows(X: torch.Tensor) -> torch.Tensor:
    """F.normalize(x, p=2, dim=-1) -- reference: util.cos_sim / splade/base.py:195-196."""
    _dev(X, torch.float32, "normalize_rows(X)")
    X = pad_dim(X)
    Y = torch.empty_like(X, memory_format=torch.contiguous_format)
    ldx = X.stride(0) if X.shape[0] > 1 else X.shape[1]
    check(_lib.lib().fz_normalize_rows_f32(_ptr(X), X.shape[0], X.shape[1], ldx, _ptr(Y), Y.shape[1], _stream(X)), "fz_normalize_rows_f32")
    return Y


def dot_scores(Qn: torch.Tensor, Dn: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """scores = Qn @ Dn.T on fp32 MFMA -- reference: torch.mm (splade/base.py:197), util.dot_score."""
    _dev(Qn, torch.float32, "dot_scores(Qn)")
    _dev(Dn, torch.float32, "dot_scores(Dn)")
    Qn, Dn = pad_dim(Qn), pad_dim(Dn)
    if Qn.shape[1] != Dn.shape[1]:
        raise ValueError(f"embedding dims differ: {Qn.shape[1]} vs {Dn.shape[1]}")
    Q, N, d = Qn.shape[0], Dn.shape[0], Qn.shape[1]
    out = _out("dot_scores", out, (Q, N), torch.float32, Qn.device, plane=True)
    check(_lib.lib().fz_dot_scores_f32(_ptr(Qn), Qn.stride(0) if Q > 1 else d, _ptr(Dn), Dn.stride(0) if N > 1 else d, Q, N, d,
                                       _ptr(out), _ld(out), _stream(Qn)), "fz_dot_scores_f32")
    return out


def dot_topn_max() -> int:
    """Largest n of dot_topn: the lists are carried in registers through the GEMM."""
    return int(_lib.lib().fz_dot_topn_max())


def dot_topn(X: torch.Tensor, C: torch.Tensor, n: int):
    """The n best columns of every row of X @ C.T by (score desc, id asc) -> (scores [rows, n] float32, ids [rows, n] int32), (-inf, -1)
    padding when n > K: bit for bit topk_rows(dot_scores(X, C), n), but the selection is the GEMM's epilogue and the [rows, K] plane is never
    written.  n <= dot_topn_max(); X and C finite."""
    _dev(X, torch.float32, "dot_topn(X)")
    _dev(C, torch.float32, "dot_topn(C)")
    _need(X.dim() == 2 and C.dim() == 2, "dot_topn: X [rows, d] and C [K, d] expected")
    n = int(n)
    _need(1 <= n <= dot_topn_max(), f"dot_topn: n = {n} outside 1 .. {dot_topn_max()} (dot_topn_max)")
    X, C = pad_dim(X), pad_dim(C)
    if X.shape[1] != C.shape[1]:
        raise ValueError(f"embedding dims differ: {X.shape[1]} vs {C.shape[1]}")
    rows, K, d = X.shape[0], C.shape[0], X.shape[1]
    os_ = torch.empty((rows, n), dtype=torch.float32, device=X.device)
    oi = torch.empty((rows, n), dtype=torch.int32, device=X.device)
    lib = _lib.lib()
    wsb = int(lib.fz_dot_topn_workspace_bytes(rows, K, n))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=X.device)
    check(lib.fz_dot_topn_f32(_ptr(X), X.stride(0) if rows > 1 else d, _ptr(C), C.stride(0) if K > 1 else d, rows, K, d, n, _ptr(os_), _ptr(oi),
                              _ptr(ws), wsb, _stream(X)), "fz_dot_topn_f32")
    return os_, oi


def cos_scores(Qe: torch.Tensor, De: torch.Tensor) -> torch.Tensor:
    """util.cos_sim as called at hybrid.py:103."""
    return dot_scores(normalize_rows(Qe), normalize_rows(De))


def _pairs_args(what: str, Q: int, dev, cand: torch.Tensor, cand_len, out):
    """The candidate side of the pair scorers: cand [Q, W] int64 (rows may be strided), cand_len [Q] int32 or None, out [Q, W] float32 or
    None (allocated).  -> (cand_len, out, W)."""
    _dev(cand, torch.int64, f"{what}(cand)")
    _need(cand.dim() == 2 and cand.shape[0] == Q, f"{what}: cand must be [Q = {Q}, W], got {tuple(cand.shape)}")
    W = cand.shape[1]
    if cand_len is not None:
        _dev(cand_len, torch.int32, f"{what}(cand_len)")
        _need(tuple(cand_len.shape) == (Q,), f"{what}(cand_len): expected shape {(Q,)}, got {tuple(cand_len.shape)}")
    return cand_len, _out(what, out, (Q, W), torch.float32, dev, plane=True), W


def dot_pairs(Qn: torch.Tensor, Dn: torch.Tensor, cand: torch.Tensor, cand_len: torch.Tensor | None = None, *, id_base: int = 0,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """Dot products of every query with its own candidates (fz_dot_pairs_f32): out[q, r] = dot_scores(Qn, Dn)[q, cand[q, r] - id_base],
    bit for bit, with no [Q, N] plane.  Qn [Q, d], Dn [N, d] float32; cand [Q, W] int64 global ids (rows may be strided), cand_len [Q]
    int32 or None (= W everywhere).  -inf where r >= cand_len[q], the id is negative or the document is not one of this shard's N
    (id_base .. id_base + N - 1).  `out` [Q, W] float32 may be a view of a wider plane: only its W columns are written.  No host
    synchronisation."""
    _dev(Qn, torch.float32, "dot_pairs(Qn)")
    _dev(Dn, torch.float32, "dot_pairs(Dn)")
    _need(Qn.dim() == 2 and Dn.dim() == 2, "dot_pairs: Qn [Q, d] and Dn [N, d] expected")
    Qn, Dn = pad_dim(Qn), pad_dim(Dn)
    if Qn.shape[1] != Dn.shape[1]:
        raise ValueError(f"embedding dims differ: {Qn.shape[1]} vs {Dn.shape[1]}")
    Q, N, d = Qn.shape[0], Dn.shape[0], Qn.shape[1]
    cand_len, out, W = _pairs_args("dot_pairs", Q, Qn.device, cand, cand_len, out)
    check(_lib.lib().fz_dot_pairs_f32(_ptr(Qn), Qn.stride(0) if Q > 1 else d, _ptr(Dn), Dn.stride(0) if N > 1 else d, Q, N, d, _ptr(cand),
                                      _ld(cand), _ptr(cand_len), W, int(id_base), _ptr(out), _ld(out), _stream(Qn)), "fz_dot_pairs_f32")
    return out


# ---------------------------------------------------------------------------------------
# K2 MaxSim
# ---------------------------------------------------------------------------------------
def _token_queries(what: str, Qtok: torch.Tensor, Doff: torch.Tensor, e4m3: bool = False):
    """The query side of the token-store contract, the element type its parameter (float16, or e4m3 bytes: then the tensor is called Q8):
    Qtok [Q, Lq, dim], Doff [N + 1] int64.  -> (Qtok, Doff, (Q, Lq, dim, N)), contiguous."""
    name = "Q8" if e4m3 else "Qtok"
    Qtok = _e4m3_bytes(Qtok, f"{what}({name})") if e4m3 else _dev(Qtok, torch.float16, f"{what}({name})")
    _dev(Doff, torch.int64, f"{what}(Doff)")
    _need(Qtok.dim() == 3, f"{what}: {name} must be [Q, Lq, dim]")
    Qtok, Doff = Qtok.contiguous(), Doff.contiguous()
    Q, Lq, dim = Qtok.shape
    N = Doff.numel() - 1
    _need(N >= 0, f"{what}: Doff must hold N + 1 offsets")
    return Qtok, Doff, (Q, Lq, dim, N)


def _token_rows(what: str, Dtok: torch.Tensor, dim: int, e4m3: bool = False) -> torch.Tensor:
    """The document side: Dtok [sumL, dim] of the same element type (D8 for e4m3 bytes), packed.  -> Dtok, contiguous."""
    name = "D8" if e4m3 else "Dtok"
    Dtok = (_e4m3_bytes(Dtok, f"{what}({name})") if e4m3 else _dev(Dtok, torch.float16, f"{what}({name})")).contiguous()
    _need(Dtok.dim() == 2 and Dtok.shape[1] == dim, f"{what}: {name} must be [sumL, {dim}]")
    return Dtok


def _measured_doc_len(Doff: torch.Tensor, N: int) -> int:
    """max_doc_len's default: the longest document of Doff, at least 1 (one small D2H read)."""
    return max(int((Doff[1:] - Doff[:-1]).max().item()), 1) if N > 0 else 1


def maxsim(Qtok: torch.Tensor, Dtok: torch.Tensor, Doff: torch.Tensor, out: torch.Tensor | None = None,
           max_doc_len: int | None = None) -> torch.Tensor:
    """Exact ColBERT late interaction. Qtok [Q,Lq,128] f16, Dtok [sumL,128] f16 packed, Doff [N+1] int64.
    max_doc_len: upper bound of the document lengths (default: measured from Doff, one small D2H read)."""
    Qtok, Doff, (Q, Lq, dim, N) = _token_queries("maxsim", Qtok, Doff)
    Dtok = _token_rows("maxsim", Dtok, dim)
    out = _out("maxsim", out, (Q, N), torch.float32, Qtok.device, plane=True)
    if max_doc_len is None:
        max_doc_len = _measured_doc_len(Doff, N)
    check(_lib.lib().fz_maxsim_f16(_ptr(Qtok), _ptr(Dtok), _ptr(Doff), int(Dtok.shape[0]), int(max_doc_len), Q, Lq, N, dim, _ptr(out),
                                   _ld(out), _stream(Qtok)), "fz_maxsim_f16")
    return out


E4M3_SCALE_EXP = (-8, 15)   # fz_quantize_e4m3_f16's range of scale_exp


def _e4m3_exp(e, what: str) -> int:
    _need(isinstance(e, (int, np.integer)) and not isinstance(e, bool) and E4M3_SCALE_EXP[0] <= int(e) <= E4M3_SCALE_EXP[1],
          f"{what}: scale exponent {e!r} outside the integers {E4M3_SCALE_EXP[0]} .. {E4M3_SCALE_EXP[1]}")
    return int(e)


def _e4m3_bytes(t: torch.Tensor, what: str) -> torch.Tensor:
    """e4m3 storage is torch.uint8; a torch.float8_e4m3fn tensor is the same bytes."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.float8_e4m3fn:
        t = t.view(torch.uint8)
    return _dev(t, torch.uint8, what)


def quantize_e4m3(x: torch.Tensor, scale_exp: int = 8) -> torch.Tensor:
    """OCP e4m3fn bytes of x * 2^scale_exp (fz_quantize_e4m3_f16): float16 device tensor in, uint8 tensor of the same shape out.  Round to
    nearest-even, subnormals kept, +-448 saturation (inf included), NaN -> 0x7f | sign.  The default 8: L2-normalised components have
    |x| <= 1, so |y| <= 256 < 448, and components down to 2^-14 stay in the normal range."""
    _dev(x, torch.float16, "quantize_e4m3(x)")
    scale_exp = _e4m3_exp(scale_exp, "quantize_e4m3")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(_lib.lib().fz_quantize_e4m3_f16(_ptr(x), x.numel(), scale_exp, _ptr(out), _stream(x)), "fz_quantize_e4m3_f16")
    return out


_E4M3_TABLE: dict = {}


def e4m3_table() -> np.ndarray:
    """The 256 values of OCP e4m3fn as float32 (0x7f / 0xff: NaN)."""
    b = np.arange(256)
    e, m = (b >> 3) & 15, (b & 7).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e - 7.0))
    v[(b & 0x7f) == 0x7f] = np.nan
    return np.where(b & 0x80, -v, v).astype(np.float32)


def dequantize_e4m3(b: torch.Tensor, scale_exp: int = 8) -> torch.Tensor:
    """float32 values of e4m3 bytes, divided by 2^scale_exp: a 256-entry table gather in torch (tests and tools; no kernel)."""
    b = _e4m3_bytes(b, "dequantize_e4m3(b)")
    scale_exp = _e4m3_exp(scale_exp, "dequantize_e4m3")
    key = (b.device, scale_exp)
    if key not in _E4M3_TABLE:
        _E4M3_TABLE[key] = torch.from_numpy(e4m3_table() * np.float32(2.0 ** -scale_exp)).to(b.device)
    return _E4M3_TABLE[key][b.long()]


def maxsim_e4m3(Q8: torch.Tensor, D8: torch.Tensor, Doff: torch.Tensor, *, q_exp: int = 8, d_exp: int = 8, out: torch.Tensor | None = None,
                max_doc_len: int | None = None) -> torch.Tensor:
    """ops.maxsim over e4m3 token bytes (fz_maxsim_e4m3): the exact MaxSim of the dequantised tokens, Q8 [Q, Lq, 128] and D8 [sumL, 128]
    uint8 (or torch.float8_e4m3fn) as quantize_e4m3 wrote them with q_exp and d_exp.  Every dot product is accumulated in float32 on the
    16x16x128 block-scaled MFMA; the finished sum is multiplied by 2^-(q_exp + d_exp)."""
    q_exp, d_exp = _e4m3_exp(q_exp, "maxsim_e4m3(q_exp)"), _e4m3_exp(d_exp, "maxsim_e4m3(d_exp)")
    Q8, Doff, (Q, Lq, dim, N) = _token_queries("maxsim_e4m3", Q8, Doff, e4m3=True)
    D8 = _token_rows("maxsim_e4m3", D8, dim, e4m3=True)
    out = _out("maxsim_e4m3", out, (Q, N), torch.float32, Q8.device, plane=True)
    if max_doc_len is None:
        max_doc_len = _measured_doc_len(Doff, N)
    _need(int(max_doc_len) >= 1, f"maxsim_e4m3: max_doc_len = {max_doc_len} must be positive")
    check(_lib.lib().fz_maxsim_e4m3(_ptr(Q8), _ptr(D8), _ptr(Doff), int(D8.shape[0]), int(max_doc_len), Q, Lq, N, dim, q_exp + d_exp,
                                    _ptr(out), _ld(out), _stream(Q8)), "fz_maxsim_e4m3")
    return out


def _maxsim_pairs_args(what: str, Qtok: torch.Tensor, Doff: torch.Tensor, cand: torch.Tensor, cand_len, out, max_doc_len, e4m3: bool = False):
    """What the candidate-list MaxSim ops check whatever the document rows are stored as: the query side of the token store (_token_queries;
    Doff one-dimensional), the candidate side (_pairs_args) and max_doc_len.  -> (Qtok, Doff, cand_len, out, (Q, Lq, dim, N, k))."""
    Qtok, Doff, (Q, Lq, dim, N) = _token_queries(what, Qtok, Doff, e4m3)
    _need(Doff.dim() == 1, f"{what}: Doff must hold N + 1 offsets")
    cand_len, out, k = _pairs_args(what, Q, Qtok.device, cand, cand_len, out)
    _need(int(max_doc_len) >= 1, f"{what}: max_doc_len must be at least 1")
    return Qtok, Doff, cand_len, out, (Q, Lq, dim, N, k)


def maxsim_pairs(Qtok: torch.Tensor, Dtok: torch.Tensor, Doff: torch.Tensor, cand: torch.Tensor, cand_len: torch.Tensor | None = None, *,
                 id_base: int = 0, max_doc_len: int = 512, out: torch.Tensor | None = None) -> torch.Tensor:
    """Exact MaxSim of every query against its own candidates (fz_maxsim_pairs_f16): out[q, r] = the score ops.maxsim gives query q and
    document cand[q, r] - id_base, bit for bit, with no [Q, N] plane.  cand [Q, k] int64 global ids (rows may be strided), cand_len [Q]
    int32 or None (= k everywhere).  -inf where r >= cand_len[q], the id is negative or the document is not one of this shard's N
    (id_base .. id_base + N - 1); an empty document scores 0.  `out` [Q, k] float32 may be a view of a wider plane: only its k columns
    are written.  No host synchronisation."""
    Qtok, Doff, cand_len, out, (Q, Lq, dim, N, k) = _maxsim_pairs_args("maxsim_pairs", Qtok, Doff, cand, cand_len, out, max_doc_len)
    Dtok = _token_rows("maxsim_pairs", Dtok, dim)
    check(_lib.lib().fz_maxsim_pairs_f16(_ptr(Qtok), _ptr(Dtok), _ptr(Doff), int(Dtok.shape[0]), int(max_doc_len), Q, Lq, N, dim, _ptr(cand),
                                         _ld(cand), _ptr(cand_len), k, int(id_base), _ptr(out), _ld(out), _stream(Qtok)),
          "fz_maxsim_pairs_f16")
    return out


def maxsim_pairs_e4m3(Q8: torch.Tensor, D8: torch.Tensor, Doff: torch.Tensor, cand: torch.Tensor, cand_len: torch.Tensor | None = None, *,
                      q_exp: int = 8, d_exp: int = 8, id_base: int = 0, max_doc_len: int = 512, out: torch.Tensor | None = None) -> torch.Tensor:
    """maxsim_pairs over e4m3 token bytes (fz_maxsim_pairs_e4m3): out[q, r] = the score ops.maxsim_e4m3 gives query q and document
    cand[q, r] - id_base, bit for bit -- the exact MaxSim of the dequantised tokens -- with no [Q, N] plane.  Q8 [Q, Lq, 128] and D8
    [sumL, 128] uint8 (or torch.float8_e4m3fn) as quantize_e4m3 wrote them with q_exp and d_exp; cand, cand_len, id_base, max_doc_len, out
    and the -inf / 0 slots as in maxsim_pairs (rows of cand may be strided, `out` may be a view of a wider plane).  No host
    synchronisation."""
    what = "maxsim_pairs_e4m3"
    q_exp, d_exp = _e4m3_exp(q_exp, f"{what}(q_exp)"), _e4m3_exp(d_exp, f"{what}(d_exp)")
    Q8, Doff, cand_len, out, (Q, Lq, dim, N, k) = _maxsim_pairs_args(what, Q8, Doff, cand, cand_len, out, max_doc_len, e4m3=True)
    D8 = _token_rows(what, D8, dim, e4m3=True)
    check(_lib.lib().fz_maxsim_pairs_e4m3(_ptr(Q8), _ptr(D8), _ptr(Doff), int(D8.shape[0]), int(max_doc_len), Q, Lq, N, dim, q_exp + d_exp,
                                          _ptr(cand), _ld(cand), _ptr(cand_len), k, int(id_base), _ptr(out), _ld(out), _stream(Q8)),
          "fz_maxsim_pairs_e4m3")
    return out


# ---------------------------------------------------------------------------------------
# K5a / K6 sort
# ---------------------------------------------------------------------------------------
def sort_max_n(dtype=torch.float32) -> int:
    return int(_lib.lib().fz_sort_max_n() if dtype == torch.float32 else _lib.lib().fz_sort_max_n_f64())


def sort_rows_desc(keys: torch.Tensor, init_order: torch.Tensor | None = None, row_len: torch.Tensor | None = None,
                   want_order=True, want_keys=True, want_rank=False, init_rank: torch.Tensor | None = None,
                   stats_out: torch.Tensor | None = None, stats_len: torch.Tensor | None = None, covers_all: bool = False,
                   lexical: bool = False):
    """Stable descending row sort (Python sorted(reverse=True): bm25.py:104, hybrid.py:306).
    Incoming sequence: identity (default), `init_order` (column at each sequence position) or `init_rank`
    (sequence position of each column: a rank plane; read coalesced, the fast form).
    Returns (order|None, sorted_keys|None, rank|None); order/sorted_keys entries beyond row_len are -1 / -inf,
    rank entries of elements outside the sequence are -1.
    stats_out: a contiguous fp32 tensor [4, rows] that receives mean | unbiased std | min | max of each list's float32 values as a
    by-product of the sort (identity / init_order sequences, rows that fit one workgroup); stats_len [rows] int32 restricts the
    statistics to the first stats_len[row] entries of the sorted list (a ranking cut to its top-k; fp32 keys only).
    covers_all: the caller vouches that the incoming sequence holds every column of every row (init_rank is a full ranking's rank
    plane, no row_len): the outputs are then written in full and need no -1 / -inf pre-fill (two plane-sized fill launches).
    lexical: the rows are a lexical ranker's float64 scores (BM25 / TF-IDF: mostly exact zeros) in the identity sequence -> the
    zero-compacting instantiation (fz_sort_rows_desc_lexical); same outputs, bit for bit."""
    _dev(keys, None, "sort_rows_desc(keys)")
    if keys.dtype not in (torch.float32, torch.float64):
        raise TypeError("keys must be float32 or float64")
    keys = as_plane(keys)
    rows, n = keys.shape
    ld = _ld(keys)
    dev = keys.device

    if init_order is not None and init_rank is not None:
        raise ValueError("pass init_order or init_rank, not both")
    partial = (row_len is not None or init_order is not None or init_rank is not None) and not covers_all  # some slots may stay unwritten: pre-fill them

    def mk(dtype, fill):
        shape = (max(rows, 1), ld)
        base = torch.full(shape, fill, dtype=dtype, device=dev) if partial else torch.empty(shape, dtype=dtype, device=dev)
        return base[:rows, :n]
    order = mk(torch.int32, -1) if want_order else None
    sk = mk(keys.dtype, float("-inf")) if want_keys else None
    rank = mk(torch.int32, -1) if want_rank else None
    if init_order is not None:
        _dev(init_order, torch.int32, "init_order")
        _need(tuple(init_order.shape) == (rows, n), f"init_order: expected shape {(rows, n)}, got {tuple(init_order.shape)}")
        if _ld(init_order) != ld and rows > 1:
            t = mk(torch.int32, -1)
            t.copy_(init_order)
            init_order = t
    if row_len is not None:
        _dev(row_len, torch.int32, "row_len")
        row_len = row_len.contiguous()
        _need(row_len.numel() == rows, f"row_len: expected {rows} entries, got {row_len.numel()}")
    bits = 32 if keys.dtype == torch.float32 else 64
    lib = _lib.lib()
    wsb = int(lib.fz_sort_workspace_bytes(bits, rows, n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    if init_rank is not None:
        _need(stats_out is None and stats_len is None, "sort_rows_desc: no statistics by-product for a placed sequence")
        _dev(init_rank, torch.int32, "init_rank")
        _need(tuple(init_rank.shape) == (rows, n), f"init_rank: expected shape {(rows, n)}, got {tuple(init_rank.shape)}")
        if _ld(init_rank) != ld and rows > 1:
            t = mk(torch.int32, -1)
            t.copy_(init_rank)
            init_rank = t
        check(lib.fz_sort_rows_desc_placed(_ptr(keys), bits, _ptr(init_rank), _ptr(row_len), rows, n, ld, _ptr(order), _ptr(sk),
                                           _ptr(rank), _ptr(ws), wsb, _stream(keys)), "fz_sort_rows_desc_placed")
    else:
        if stats_out is not None:
            _dev(stats_out, torch.float32, "sort_rows_desc(stats_out)")
            _need(tuple(stats_out.shape) == (4, rows) and stats_out.is_contiguous(), f"sort_rows_desc(stats_out): need a contiguous [4, {rows}] tensor")
        if stats_len is not None:
            _need(stats_out is not None, "sort_rows_desc(stats_len) needs stats_out")
            _dev(stats_len, torch.int32, "sort_rows_desc(stats_len)")
            _need(stats_len.numel() == rows and stats_len.is_contiguous(), f"sort_rows_desc(stats_len): need {rows} contiguous lengths")
        if lexical and bits == 64 and init_order is None and stats_len is None and order is not None:
            check(lib.fz_sort_rows_desc_lexical(_ptr(keys), _ptr(row_len), rows, n, ld, _ptr(order), _ptr(sk), _ptr(rank), _ptr(stats_out),
                                                _ptr(ws), wsb, _stream(keys)), "fz_sort_rows_desc_lexical")
            return order, sk, rank
        check(lib.fz_sort_rows_desc(_ptr(keys), bits, _ptr(init_order), _ptr(row_len), rows, n, ld, _ptr(order), _ptr(sk),
                                    _ptr(rank), _ptr(stats_out), _ptr(stats_len), _ptr(ws), wsb, _stream(keys)), "fz_sort_rows_desc")
    return order, sk, rank


def sort_bucket_rank_rows(reset: bool = False) -> tuple[int, int, int]:
    """(rows the bucket ranking ordered, of those rows with a swapped pair put back, rows it handed to the digit passes) on the current
    device since the last reset (fz_sort_bucket_rank_rows; synchronises the device: tests and tools)."""
    import ctypes
    c = (ctypes.c_uint64 * 3)()
    check(_lib.lib().fz_sort_bucket_rank_rows(ctypes.cast(c, ctypes.c_void_p), 1 if reset else 0), "fz_sort_bucket_rank_rows")
    return int(c[0]), int(c[1]), int(c[2])


def sort_zero_compact_rows(reset: bool = False) -> tuple[int, int]:
    """(float64 rows whose exact zeros were left out of the ordering phases, eligible rows that had too few zeros) on the current device since
    the last reset (fz_sort_zero_compact_rows; synchronises the device: tests and tools)."""
    import ctypes
    c = (ctypes.c_uint64 * 2)()
    check(_lib.lib().fz_sort_zero_compact_rows(ctypes.cast(c, ctypes.c_void_p), 1 if reset else 0), "fz_sort_zero_compact_rows")
    return int(c[0]), int(c[1])


def select_topk(fused: torch.Tensor, pos: torch.Tensor | None, k: int, cap: int | None = None):
    """First k entries of sort_rows_desc(fused, init_rank=pos) without sorting the rows (fz_select_topk_f + two small row sorts): the
    fused lists main() actually reads (predictions(1000), hybrid.py:537).  fused [Q, N] float32 / float64 plane, pos [Q, N] int32 plane =
    first-insertion position of every column (< 0: in no list; None: the column index).  Returns (cols [Q, k] int32 -- -1 past a row's
    length --, scores [Q, k], lens [Q] int32), or None when a row has more than `cap` candidates (a long tie run at the k-th place) or
    the row is longer than one workgroup holds: the caller then sorts in full.  cap (default: k + 1024 rounded up to 1024) is rounded up to
    a multiple of 64."""
    _dev(fused, None, "select_topk(fused)")
    if fused.dtype not in (torch.float32, torch.float64):
        raise TypeError("select_topk(fused): float32 or float64 expected")
    fused = as_plane(fused)
    Q, N = fused.shape
    _need(k > 0, "select_topk: k must be positive")
    if N > sort_max_n(torch.float64) or Q == 0:
        return None
    if pos is not None:
        _dev(pos, torch.int32, "select_topk(pos)")
        _same_shape([fused, pos], "select_topk")
        _need(Q <= 1 or _ld(pos) == _ld(fused), "select_topk: fused and pos must share the row stride")
    # the kernel numbers a row's candidates in rows of `cap` slots, so cap is a whole plane row: a given cap is rounded up to one (a narrower
    # view hid the slots between cap and the row stride from the two sorts below: candidates lost, no flag)
    cap = round_up(int(cap), _PAD) if cap else round_up(k + 1024, 1024)
    dev = fused.device
    cols = alloc_plane(Q, cap, torch.int32, dev)
    vals = alloc_plane(Q, cap, fused.dtype, dev)
    negp = alloc_plane(Q, cap, torch.float32, dev)
    clen = torch.empty(Q, dtype=torch.int32, device=dev)
    over = torch.zeros(1, dtype=torch.int32, device=dev)
    _need(_ld(cols) == _ld(vals) == _ld(negp), "select_topk: candidate planes must share the row stride")
    rc = _lib.lib().fz_select_topk_f(_ptr(fused), 32 if fused.dtype == torch.float32 else 64, _ptr(pos), Q, N, _ld(fused), int(k), _ld(cols), _ptr(cols),
                                     _ptr(vals), _ptr(negp), _ptr(clen), _ptr(over), _stream(fused))
    check(rc, "fz_select_topk_f")
    by_pos, _, _ = sort_rows_desc(negp, row_len=clen, want_keys=False)                 # candidate slots in first-insertion order
    slots, sk, _ = sort_rows_desc(vals, init_order=by_pos, row_len=clen)              # ... then, stably, by fused score
    if int(over.item()) != 0:
        return None
    kk = min(k, cap)
    sel = slots[:, :kk]
    out_cols = torch.where(sel >= 0, torch.gather(cols, 1, sel.clamp(min=0).long()), torch.full_like(sel, -1))
    return out_cols, sk[:, :kk], torch.clamp(clen, max=kk)


# ---------------------------------------------------------------------------------------
# fusion
# ---------------------------------------------------------------------------------------
def fuse_rank(ranks: list[torch.Tensor], lens: torch.Tensor, method: str) -> torch.Tensor:
    """rrf / bcf in float64 (hybrid.py:248-252,301-304). ranks[s] [Q,N] int32 planes, lens [S,Q] int32."""
    _max_systems(len(ranks), "fuse_rank")
    for r in ranks:
        _dev(r, torch.int32, "fuse_rank(ranks)")
    _same_shape(ranks, "fuse_rank")
    ranks = harmonise(list(ranks))
    _dev(lens, torch.int32, "fuse_rank(lens)")
    lens = lens.contiguous()
    Q, N = ranks[0].shape
    _need(tuple(lens.shape) == (len(ranks), Q), f"fuse_rank(lens): expected shape {(len(ranks), Q)}, got {tuple(lens.shape)}")
    ld = _same_ld(*ranks)
    fused = torch.empty((max(Q, 1), ld), dtype=torch.float64, device=ranks[0].device)[:Q, :N]
    check(_lib.lib().fz_fuse_rank_f64(_ptr_array(ranks), _ptr(lens), len(ranks), Q, N, ld, RANK_METHODS[method], _ptr(fused),
                                      _stream(ranks[0])), "fz_fuse_rank_f64")
    return fused


def sort_rank_fused(ranks: list[torch.Tensor], lens: torch.Tensor, method: str, init_order: torch.Tensor | None = None,
                    init_rank: torch.Tensor | None = None, row_len: torch.Tensor | None = None, want_rank: bool = False,
                    covers_all: bool = False):
    """rrf / bcf fusion (hybrid.py:248-252,301-304) and the stable descending sort of the fused scores (hybrid.py:306) in ONE kernel:
    sort_rows_desc(fuse_rank(ranks, lens, method), init_order / init_rank, row_len) without the float64 plane in between
    (fz_sort_rank_fused_desc).  Returns (order, fused scores in list order [float64], rank | None) -- bit-identical to the two calls.
    Rows longer than one workgroup holds raise FusionHipError(FZ_ERR_UNSUPPORTED): callers take the two calls there."""
    _max_systems(len(ranks), "sort_rank_fused")
    for r in ranks:
        _dev(r, torch.int32, "sort_rank_fused(ranks)")
    _same_shape(ranks, "sort_rank_fused")
    first_is_pos = init_rank is not None and init_rank is ranks[0]
    ranks = harmonise(list(ranks))
    if first_is_pos:
        init_rank = ranks[0]
    _dev(lens, torch.int32, "sort_rank_fused(lens)")
    lens = lens.contiguous()
    rows, n = ranks[0].shape
    _need(tuple(lens.shape) == (len(ranks), rows), f"sort_rank_fused(lens): expected shape {(len(ranks), rows)}, got {tuple(lens.shape)}")
    _need(init_order is None or init_rank is None, "sort_rank_fused: pass init_order or init_rank, not both")
    ld = _same_ld(*ranks)
    dev = ranks[0].device
    partial = (row_len is not None or init_order is not None or init_rank is not None) and not covers_all

    def mk(dtype, fill):
        shape = (max(rows, 1), ld)
        base = torch.full(shape, fill, dtype=dtype, device=dev) if partial else torch.empty(shape, dtype=dtype, device=dev)
        return base[:rows, :n]
    order, sk = mk(torch.int32, -1), mk(torch.float64, float("-inf"))
    rank = mk(torch.int32, -1) if want_rank else None
    for name, t in (("init_order", init_order), ("init_rank", init_rank)):
        if t is not None:
            _dev(t, torch.int32, f"sort_rank_fused({name})")
            _need(tuple(t.shape) == (rows, n), f"sort_rank_fused({name}): expected shape {(rows, n)}, got {tuple(t.shape)}")
    if init_order is not None and _ld(init_order) != ld and rows > 1:
        t = mk(torch.int32, -1); t.copy_(init_order); init_order = t
    if init_rank is not None and _ld(init_rank) != ld and rows > 1:
        t = mk(torch.int32, -1); t.copy_(init_rank); init_rank = t
    if row_len is not None:
        _dev(row_len, torch.int32, "sort_rank_fused(row_len)")
        row_len = row_len.contiguous()
        _need(row_len.numel() == rows, f"sort_rank_fused(row_len): expected {rows} entries, got {row_len.numel()}")
    lib = _lib.lib()
    wsb = int(lib.fz_sort_rank_fused_workspace_bytes(rows, n, ld))
    ws = _reserved_workspace(dev, wsb)
    check(lib.fz_sort_rank_fused_desc(_ptr_array(ranks), _ptr(lens), len(ranks), RANK_METHODS[method], _ptr(init_order), _ptr(init_rank),
                                      _ptr(row_len), rows, n, ld, _ptr(order), _ptr(sk), _ptr(rank), _ptr(ws), wsb, _stream(ranks[0])),
          "fz_sort_rank_fused_desc")
    return order, sk, rank


def rrf_terms(count: int, fast: bool, device="cuda") -> torch.Tensor:
    """[count] float64: 1 / (60 + r + 1) as the fused sort forms it (fast) or as fz_fuse_rank_f64 does (IEEE division) -- a diagnostic."""
    out = torch.empty(int(count), dtype=torch.float64, device=device)
    check(_lib.lib().fz_rrf_terms_f64(int(count), 1 if fast else 0, _ptr(out), _stream(out)), "fz_rrf_terms_f64")
    return out


def row_stats(scores: torch.Tensor, rank: torch.Tensor | None, norm: str):
    _dev(scores, torch.float32, "row_stats(scores)")
    rows, N = scores.shape
    a = torch.empty(rows, dtype=torch.float32, device=scores.device)
    b = torch.empty(rows, dtype=torch.float32, device=scores.device)
    if rank is not None:
        _dev(rank, torch.int32, "row_stats(rank)")
        _same_shape([scores, rank], "row_stats")
        scores, rank = harmonise([scores, rank])
        _same_ld(scores, rank)
    check(_lib.lib().fz_row_stats_f32(_ptr(scores), _ptr(rank), rows, N, _ld(scores), NORMS[norm], _ptr(a), _ptr(b), _stream(scores)),
          "fz_row_stats_f32")
    return a, b


def minmax_from_order(scores: torch.Tensor, order: torch.Tensor, lens: torch.Tensor | None, out=None):
    """(min, max) of every ranked list read off its two ends (no reduction): scores / order [Q, N] planes, lens [Q] or None.
    out: optional (mn, mx) fp32 tensors of Q entries to write into."""
    _dev(scores, torch.float32, "minmax_from_order(scores)")
    _dev(order, torch.int32, "minmax_from_order(order)")
    _same_shape([scores, order], "minmax_from_order")
    scores, order = harmonise([scores, order])
    rows, N = scores.shape
    if lens is not None:
        _need(_dev(lens, torch.int32, "minmax_from_order(lens)").numel() == rows and lens.is_contiguous(), f"minmax_from_order: lens must hold {rows} lengths")
    if out is not None:
        mn, mx = out
        _need(mn.numel() == rows and mx.numel() == rows and mn.is_contiguous() and mx.is_contiguous(), f"minmax_from_order(out): need two contiguous tensors of {rows}")
        _dev(mn, torch.float32, "minmax_from_order(out)"); _dev(mx, torch.float32, "minmax_from_order(out)")
    else:
        mn = torch.empty(rows, dtype=torch.float32, device=scores.device)
        mx = torch.empty(rows, dtype=torch.float32, device=scores.device)
    check(_lib.lib().fz_minmax_from_order_f32(_ptr(scores), _ptr(order), _ptr(lens), rows, N, _ld(scores), _ptr(mn), _ptr(mx), _stream(scores)),
          "fz_minmax_from_order_f32")
    return mn, mx


TABLES_PATHS = {0: "lds-all", 1: "lds-swap", 2: "row"}


class PreparedTables:
    """Quantile tables of a percentile-rank / NCE fusion made ready for the kernel that keeps one system's table in LDS at a time
    (fz_nsf_tables_prepare): aligned copies, bucket tables and -- NCE -- the value of every table index, in one workspace tensor.
    Valid for any number of fuse_nsf calls with these tables and this norm (hybrid.py:412,451 read the tables once per process)."""

    def __init__(self, distr: list[torch.Tensor], norm: str, workspace: torch.Tensor):
        self.distr, self.norm, self.workspace = distr, norm, workspace

    def search_info(self) -> list[dict]:
        """Per system: probes per search and entries in the fullest bucket (diagnostics; synchronises)."""
        S = len(self.distr)
        P = (C.c_int32 * S)(*[int(d.numel()) for d in self.distr])
        out = []
        for s in range(S):
            off = int(_lib.lib().fz_nsf_tables_header_offset(S, P, NORMS[self.norm], s))
            h = self.workspace[off:off + 16].cpu().numpy()
            out.append(dict(probes=int(h[8:12].view(np.int32)[0]), fullest_bucket=int(h[12:16].view(np.int32)[0])))
        return out

    def matches(self, distr, norm) -> bool:
        return norm == self.norm and len(distr) == len(self.distr) and all(
            a.data_ptr() == b.data_ptr() and a.numel() == b.numel() for a, b in zip(distr, self.distr))


def nsf_tables_prepare(distr: list[torch.Tensor], norm: str) -> PreparedTables | None:
    """None when a table is too long for LDS (fuse_nsf then searches it in global memory)."""
    _need(norm in ("percentile-rank", "normal-curve-equivalent"), f"nsf_tables_prepare: {norm!r} has no tables")
    _max_systems(len(distr), "nsf_tables_prepare")
    distr = [_dev(d, torch.float32, "distr").contiguous() for d in distr]
    S = len(distr)
    _need(all(d.dim() == 1 and d.numel() > 0 for d in distr), "nsf_tables_prepare: tables must be non-empty 1-d tensors")
    P = (C.c_int32 * S)(*[int(d.numel()) for d in distr])
    lib = _lib.lib()
    nbytes = int(lib.fz_nsf_tables_workspace_bytes(S, P, NORMS[norm]))
    if nbytes == 0:
        return None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=distr[0].device)
    check(lib.fz_nsf_tables_prepare(_ptr_array(distr), P, S, NORMS[norm], _ptr(ws), nbytes, _stream(distr[0])), "fz_nsf_tables_prepare")
    return PreparedTables(distr, norm, ws)


last_tables_path: str | None = None   # which kernel the last percentile-rank / NCE fuse_nsf call ran (tests pin it)


def fuse_nsf(planes: list[torch.Tensor], ranks: list[torch.Tensor | None] | None, weights, norm: str,
             distr: list[torch.Tensor] | None = None, out: torch.Tensor | None = None,
             orders: list[torch.Tensor] | None = None, lens: torch.Tensor | None = None,
             stats=None,
             valid_bits: list[torch.Tensor | None] | None = None,
             tables: PreparedTables | None | bool = None) -> torch.Tensor:
    """normalise -> weight -> sum in one HBM pass (hybrid.py:212-214,254-280,291,301-304).
    orders (+ lens [S, Q]): the systems' order planes, when they are ranked -- min-max then takes every list's minimum and
    maximum from its two ends and the fusion is one flat streaming pass (same bits as the reducing kernel).
    stats: the row statistics (min / max, or mean / unbiased std), when the caller has them -- the fusion is then one flat streaming
    pass.  Either (a, b) = two contiguous [S*Q] fp32 tensors, or a list of S pairs (a_s, b_s) of [Q] fp32 tensors, one per system:
    each ranked system keeps the statistics its ranking sort produced (sort_rows_desc(stats_out=...)), nothing is concatenated.
    valid_bits[s] (optional): the validity of system s as a bitmap (rank_to_bitmap), read instead of its rank plane.
    tables (optional): nsf_tables_prepare(distr, norm) of these very tables, to prepare them once for many calls; False: stay on
    fz_fuse_nsf_f32 whatever the table size (its all-tables-in-LDS kernel or its global-memory search: what tests compare against)."""
    _max_systems(len(planes), "fuse_nsf")
    for p in planes:
        _dev(p, torch.float32, "fuse_nsf(planes)")
    S = len(planes)
    if ranks:
        _need(len(ranks) == S, f"fuse_nsf: {S} planes but {len(ranks)} rank planes")
        for r in ranks:
            if r is not None:
                _dev(r, torch.int32, "fuse_nsf(ranks)")
    _same_shape(list(planes) + (list(ranks) if ranks else []), "fuse_nsf")
    _need(len(weights) == S, f"fuse_nsf: {S} planes but {len(weights)} weights")
    both = harmonise(list(planes) + (list(ranks) if ranks else []))
    planes, ranks = both[:S], (both[S:] if ranks else None)
    Q, N = planes[0].shape
    ld = _same_ld(*planes, *([r for r in ranks if r is not None] if ranks else []))
    dev = planes[0].device
    if out is not None:
        _dev(out, torch.float32, "fuse_nsf(out)")
        _need(tuple(out.shape) == (Q, N) and (Q <= 1 or _ld(out) == ld), f"fuse_nsf(out): expected a [{Q}, {N}] plane with row stride {ld}")
    fused = out if out is not None else torch.empty((max(Q, 1), ld), dtype=torch.float32, device=dev)[:Q, :N]
    w = (C.c_double * S)(*[float(x) for x in weights])
    vb, ldb = None, 0
    if valid_bits is not None and any(b is not None for b in valid_bits):
        _need(len(valid_bits) == S, f"fuse_nsf: {S} planes but {len(valid_bits)} validity bitmaps")
        for b in valid_bits:
            if b is not None:
                _dev(b, torch.int32, "fuse_nsf(valid_bits)")
                _need(b.dim() == 2 and b.shape[0] == Q and b.is_contiguous() and b.shape[1] * 32 >= N, "fuse_nsf(valid_bits): expected contiguous [Q, >= N/32] int32 bitmaps")
        ldbs = {int(b.shape[1]) for b in valid_bits if b is not None}
        _need(len(ldbs) == 1, "fuse_nsf(valid_bits): bitmaps must share their row stride")
        vb, ldb = _ptr_array(valid_bits), ldbs.pop()
    dptr, P = None, None
    if norm in ("percentile-rank", "normal-curve-equivalent"):
        if distr is None or any(d is None for d in distr):
            raise AttributeError("percentile distributions are required for percentile-rank / normal-curve-equivalent")
        _need(len(distr) == S, f"fuse_nsf: {S} planes but {len(distr)} percentile tables")
        distr = [_dev(d, torch.float32, "distr").contiguous() for d in distr]
        dptr = _ptr_array(distr)
        P = (C.c_int32 * S)(*[int(d.numel()) for d in distr])
    lib = _lib.lib()
    if stats is not None and norm in ("min-max", "z-score") and Q > 0 and N > 0 and isinstance(stats, list):
        _need(len(stats) == S, f"fuse_nsf(stats): {S} planes but {len(stats)} statistics pairs")
        for pr in stats:
            for x in pr:
                _dev(x, torch.float32, "fuse_nsf(stats)")
                _need(x.numel() == Q and x.is_contiguous(), f"fuse_nsf(stats): per-system statistics must be contiguous tensors of {Q} entries")
        check(lib.fz_fuse_nsf_pstats_f32(_ptr_array(planes), None if ranks is None else _ptr_array(ranks), w, S, Q, N, ld, NORMS[norm],
                                         dptr, P, _ptr_array([a_ for a_, _ in stats]), _ptr_array([b_ for _, b_ in stats]), vb, ldb, _ptr(fused),
                                         _stream(planes[0])), "fz_fuse_nsf_pstats_f32")
        return fused
    if stats is not None and norm in ("min-max", "z-score") and Q > 0 and N > 0:
        sa, sb = stats
        for x in (sa, sb):
            _dev(x, torch.float32, "fuse_nsf(stats)")
            _need(x.numel() == S * Q and x.is_contiguous(), f"fuse_nsf(stats): need contiguous tensors of {S * Q} entries")
        check(lib.fz_fuse_nsf_stats_f32(_ptr_array(planes), None if ranks is None else _ptr_array(ranks), w, S, Q, N, ld, NORMS[norm],
                                        dptr, P, _ptr(sa), _ptr(sb), vb, ldb, _ptr(fused), _stream(planes[0])), "fz_fuse_nsf_stats_f32")
        return fused
    if norm == "min-max" and orders is not None and Q > 0 and N > 0:
        _need(len(orders) == S, f"fuse_nsf: {S} planes but {len(orders)} order planes")
        if lens is not None:
            _need(tuple(lens.shape) == (S, Q), f"fuse_nsf(lens): expected shape {(S, Q)}, got {tuple(lens.shape)}")
        for o_ in orders:
            _dev(o_, torch.int32, "fuse_nsf(orders)")
        _same_shape(list(planes) + list(orders), "fuse_nsf(orders)")
        allp = harmonise(list(planes) + (list(ranks) if ranks else []) + list(orders))   # one row stride for every plane of the call
        planes, orders = allp[:S], allp[len(allp) - S:]
        ranks = allp[S:2 * S] if ranks else None
        ld = _same_ld(*planes, *orders, *([r for r in ranks if r is not None] if ranks else []))
        if out is None:
            fused = torch.empty((max(Q, 1), ld), dtype=torch.float32, device=dev)[:Q, :N]
        else:
            _need(Q <= 1 or _ld(out) == ld, f"fuse_nsf(out): expected a [{Q}, {N}] plane with row stride {ld}")
        if lens is not None:
            lens = _dev(lens, torch.int32, "fuse_nsf(lens)").contiguous()
        sa = torch.empty(S * Q, dtype=torch.float32, device=dev)
        sb = torch.empty(S * Q, dtype=torch.float32, device=dev)
        check(lib.fz_minmax_from_orders_f32(_ptr_array(planes), _ptr_array(orders), _ptr(lens), S, Q, N, ld, _ptr(sa), _ptr(sb), _stream(planes[0])),
              "fz_minmax_from_orders_f32")
        check(lib.fz_fuse_nsf_stats_f32(_ptr_array(planes), None if ranks is None else _ptr_array(ranks), w, S, Q, N, ld, NORMS[norm],
                                        dptr, P, _ptr(sa), _ptr(sb), vb, ldb, _ptr(fused), _stream(planes[0])), "fz_fuse_nsf_stats_f32")
        return fused
    if dptr is not None and Q > 0 and N > 0:
        # quantile tables: all of them LDS-resident (small tables), one system's at a time (the sizes the reference reads:
        # hybrid.py:412,451 -- 27,943 entries; :374 -- 10,001), or searched in global memory (longer still)
        global last_tables_path
        rp = None if ranks is None else _ptr_array(ranks)
        path = lib.fz_nsf_tables_path(_ptr_array(planes), rp, S, Q, N, ld, NORMS[norm], P, _ptr(fused))
        _need(path in TABLES_PATHS, f"fz_nsf_tables_path: status {path}")
        last_tables_path = TABLES_PATHS[path]
        if tables is False:
            last_tables_path = TABLES_PATHS[0 if path == 0 else 2]
        elif path == 1:
            if tables is None or not tables.matches(distr, norm):
                tables = nsf_tables_prepare(distr, norm)
            check(lib.fz_fuse_nsf_tables_f32(_ptr_array(planes), rp, w, S, Q, N, ld, NORMS[norm], dptr, P, vb, ldb, _ptr(fused),
                                             _ptr(tables.workspace), tables.workspace.numel(), _stream(planes[0])), "fz_fuse_nsf_tables_f32")
            return fused
    rc = lib.fz_fuse_nsf_f32(_ptr_array(planes), None if ranks is None else _ptr_array(ranks), w, S, Q, N, ld, NORMS[norm], dptr, P,
                             vb, ldb, _ptr(fused), _stream(planes[0]))
    if rc == _lib.FZ_ERR_UNSUPPORTED:
        # rows longer than the register-resident kernel holds (N > 32768): statistics pass + elementwise pass
        sa = torch.zeros(S * Q, dtype=torch.float32, device=dev)
        sb = torch.zeros(S * Q, dtype=torch.float32, device=dev)
        if norm in ("min-max", "z-score"):
            for s in range(S):
                _need(vb is None or valid_bits[s] is None or (ranks is not None and ranks[s] is not None),
                      "fuse_nsf: rows longer than 32768 take their statistics over the rank planes: pass ranks next to valid_bits")
                a, b = row_stats(planes[s], None if ranks is None else ranks[s], norm)
                sa[s * Q:(s + 1) * Q] = a
                sb[s * Q:(s + 1) * Q] = b
        rc = lib.fz_fuse_nsf_stats_f32(_ptr_array(planes), None if ranks is None else _ptr_array(ranks), w, S, Q, N, ld, NORMS[norm],
                                       dptr, P, _ptr(sa), _ptr(sb), vb, ldb, _ptr(fused), _stream(planes[0]))
    check(rc, "fz_fuse_nsf_f32")
    return fused


def rank_to_bitmap(rank: torch.Tensor) -> torch.Tensor:
    """Validity bitmap of a rank plane: [Q, ceil(N / 64) * 2] int32, bit (j & 31) of word j >> 5 = (rank[q, j] >= 0).  Built once per
    partial system; the nsf fusion passes then read 1 bit per document instead of the 4-byte rank."""
    _dev(rank, torch.int32, "rank_to_bitmap(rank)")
    rank = as_plane(rank)
    Q, N = rank.shape
    ldb = max(2, (N + 63) // 64 * 2)
    bits = torch.zeros((max(Q, 1), ldb), dtype=torch.int32, device=rank.device)[:Q]
    check(_lib.lib().fz_rank_to_bitmap(_ptr(rank), Q, N, _ld(rank), _ptr(bits), ldb, _stream(rank)), "fz_rank_to_bitmap")
    return bits


def zero_unlisted_(plane: torch.Tensor, rank: torch.Tensor) -> torch.Tensor:
    """plane[q, j] = 0 where rank[q, j] < 0, in place: a system adds nothing for a document it does not list (hybrid.py:301-304)."""
    _dev(plane, torch.float32, "zero_unlisted_(plane)"); _dev(rank, torch.int32, "zero_unlisted_(rank)")
    _same_shape([plane, rank], "zero_unlisted_")
    Q, N = plane.shape
    _need(Q <= 1 or _ld(plane) == _ld(rank), "zero_unlisted_: plane and rank must share the row stride")
    check(_lib.lib().fz_zero_unlisted_f32(_ptr(plane), _ptr(rank), Q, N, _ld(plane), _stream(plane)), "fz_zero_unlisted_f32")
    return plane


def fuse_none(planes: list[torch.Tensor], ranks: list[torch.Tensor | None] | None, weights) -> torch.Tensor:
    """'none' / unknown normalisation: float64 passthrough (hybrid.py:280,291,304)."""
    _max_systems(len(planes), "fuse_none")
    for p in planes:
        _dev(p, torch.float32, "fuse_none(planes)")
    S = len(planes)
    if ranks:
        _need(len(ranks) == S, f"fuse_none: {S} planes but {len(ranks)} rank planes")
        for r in ranks:
            if r is not None:
                _dev(r, torch.int32, "fuse_none(ranks)")
    _same_shape(list(planes) + (list(ranks) if ranks else []), "fuse_none")
    _need(len(weights) == S, f"fuse_none: {S} planes but {len(weights)} weights")
    both = harmonise(list(planes) + (list(ranks) if ranks else []))
    planes, ranks = both[:S], (both[S:] if ranks else None)
    Q, N = planes[0].shape
    ld = _same_ld(*planes, *([r for r in ranks if r is not None] if ranks else []))
    fused = torch.empty((max(Q, 1), ld), dtype=torch.float64, device=planes[0].device)[:Q, :N]
    w = (C.c_double * S)(*[float(x) for x in weights])
    check(_lib.lib().fz_fuse_none_f64(_ptr_array(planes), None if ranks is None else _ptr_array(ranks), w, S, Q, N, ld, _ptr(fused),
                                      _stream(planes[0])), "fz_fuse_none_f64")
    return fused


def is_wide_weight(w) -> bool:
    """NumPy-2 promotion of `np.float32 score * w` (hybrid.py:291): the product is float64 only for an np.float64 weight
    -- which is what the tuning grid holds (np.arange, hybrid.py:405-409); a Python float / int is a weak scalar and
    np.float32 / np.float16 keep float32.  (np.float64 subclasses float, so it is tested by its own type.)"""
    return isinstance(w, (np.float64, np.longdouble))


def fuse_wsum(planes: list[torch.Tensor], ranks: list[torch.Tensor | None] | None, weights, narrow=None) -> torch.Tensor:
    """Weight-and-sum -> float64 plane, with NumPy's scalar promotion (fz_fuse_wsum_f64): planes may be float32 or float64
    (per system); narrow[s] = the weight is weak / float32 (fl32 product; the document's sum stays fl32 until its first
    float64 product).  narrow=None: everything float64 (the 'none' passthrough, hybrid.py:280,291,304)."""
    S = len(planes)
    _max_systems(S, "fuse_wsum")
    for p in planes:
        _dev(p, None, "fuse_wsum(planes)")
        if p.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"fuse_wsum(planes): expected float32 or float64, got {p.dtype}")
    if ranks:
        _need(len(ranks) == S, f"fuse_wsum: {S} planes but {len(ranks)} rank planes")
        for r in ranks:
            if r is not None:
                _dev(r, torch.int32, "fuse_wsum(ranks)")
    _same_shape(list(planes) + (list(ranks) if ranks else []), "fuse_wsum")
    _need(len(weights) == S, f"fuse_wsum: {S} planes but {len(weights)} weights")
    both = harmonise(list(planes) + (list(ranks) if ranks else []))
    planes, ranks = both[:S], (both[S:] if ranks else None)
    Q, N = planes[0].shape
    ld = _same_ld(*planes, *([r for r in ranks if r is not None] if ranks else []))
    fused = torch.empty((max(Q, 1), ld), dtype=torch.float64, device=planes[0].device)[:Q, :N]
    w = (C.c_double * S)(*[float(x) for x in weights])
    p64 = (C.c_int32 * S)(*[int(p.dtype == torch.float64) for p in planes])
    nr = (C.c_int32 * S)(*[int(bool(n)) for n in (narrow if narrow is not None else [False] * S)])
    check(_lib.lib().fz_fuse_wsum_f64(_ptr_array(planes), p64, None if ranks is None else _ptr_array(ranks), w, nr, S, Q, N, ld,
                                      _ptr(fused), _stream(planes[0])), "fz_fuse_wsum_f64")
    return fused


def insertion_order(orders: list[torch.Tensor], lens: torch.Tensor, N: int, want_pos: bool = False):
    """First-insertion order of the fused dict (hybrid.py:301-304). Returns (ins_order [Q,N] int32, U [Q] int32), with want_pos also the
    inverse plane pos [Q,N] int32 (first-insertion position of every document, -1 = in no list)."""
    _max_systems(len(orders), "insertion_order")
    for o in orders:
        _dev(o, torch.int32, "insertion_order(orders)")
    _same_shape(orders, "insertion_order")
    orders = harmonise(list(orders))
    _dev(lens, torch.int32, "insertion_order(lens)")
    lens = lens.contiguous()
    Q = orders[0].shape[0]
    _need(orders[0].shape[1] == N, f"insertion_order: order planes are {orders[0].shape[1]} wide, N = {N}")
    _need(tuple(lens.shape) == (len(orders), Q), f"insertion_order(lens): expected shape {(len(orders), Q)}, got {tuple(lens.shape)}")
    ld = _same_ld(*orders)
    dev = orders[0].device
    ins = torch.full((max(Q, 1), ld), -1, dtype=torch.int32, device=dev)[:Q, :N]
    U = torch.zeros(Q, dtype=torch.int32, device=dev)
    pos = torch.full((max(Q, 1), ld), -1, dtype=torch.int32, device=dev)[:Q, :N] if want_pos else None
    check(_lib.lib().fz_insertion_order(_ptr_array(orders), _ptr(lens), len(orders), Q, N, ld, _ptr(ins), _ptr(U), _ptr(pos), None, 0,
                                        _stream(orders[0])), "fz_insertion_order")
    return (ins, U, pos) if want_pos else (ins, U)


LISTS_METHODS = {"rrf": 0, "bcf": 1, "wsum32": 2, "wsum64": 3}   # fz_lists_method


def lists_max_entries() -> int:
    """The largest sum of list widths one fz_lists_join call takes (the union of a query's ids lives in one workgroup's LDS)."""
    return int(_lib.lib().fz_lists_max_entries())


def _lists_args(what: str, ids, lens, values, f64_ok: bool = False):
    """What lists_join and lists_columns check and marshal alike: S systems' ids [Q, k_s] int64, lens [Q] int32 and (None: no values)
    value planes of the ids' shapes, float32 (or float64 where f64_ok).  A system whose ids and values differ in row stride is made
    contiguous: the C ABI takes one stride per system.  -> (ids, lens, values, Q, total = sum of k_s, n_h, ld_h)."""
    S = len(ids)
    _max_systems(S, what)
    _need(S >= 1, f"{what}: no system")
    _need(len(lens) == S, f"{what}: {S} id lists but {len(lens)} length vectors")
    _need(values is None or len(values) == S, f"{what}: needs {S} value planes")
    ids = [_dev(t, torch.int64, f"{what}(ids)") for t in ids]
    Q = ids[0].shape[0]
    for t in ids:
        _need(t.dim() == 2 and t.shape[0] == Q, f"{what}(ids): every system needs a [{Q}, k] tensor, got {tuple(t.shape)}")
    total = sum(int(t.shape[1]) for t in ids)
    cap = lists_max_entries()
    _need(total <= cap, f"{what}: the lists of one query hold up to {total} entries, a join takes at most {cap} (fz_lists_max_entries)")
    lens = [_dev(t, torch.int32, f"{what}(lens)").contiguous() for t in lens]
    for t in lens:
        _need(t.numel() == Q, f"{what}(lens): expected {Q} lengths, got {t.numel()}")
    if values is not None:
        values = list(values)
        for s, v in enumerate(values):
            _dev(v, None, f"{what}(values)")
            if v.dtype != torch.float32 and not (f64_ok and v.dtype == torch.float64):
                raise TypeError(f"{what}: value planes must be float32{' or float64' if f64_ok else ''}, got {v.dtype}")
            _need(tuple(v.shape) == tuple(ids[s].shape), f"{what}(values): system {s} has ids {tuple(ids[s].shape)} but values {tuple(v.shape)}")
            if _ld(v) != _ld(ids[s]):       # one row stride per system: ids and values side by side
                ids[s], values[s] = ids[s].contiguous(), v.contiguous()
    n_h = (C.c_int32 * S)(*[int(t.shape[1]) for t in ids])
    ld_h = (C.c_int32 * S)(*[max(_ld(t), int(t.shape[1])) for t in ids])
    return ids, lens, values, Q, total, n_h, ld_h


def _lists_no_duplicate(what: str, ws: torch.Tensor):
    """The one flag read of a list join (int32 at offset 0 of its workspace): set where a list holds an id twice."""
    if int(ws[:4].view(torch.int32).item()) != 0:
        raise ValueError(f"{what}: a list holds the same id twice (ids inside one system's list must be distinct)")


def lists_join(ids: list[torch.Tensor], lens: list[torch.Tensor], method: str, values: list[torch.Tensor] | None = None,
               weights=None, narrow=None):
    """Per-query id join of S systems' top-k lists (fz_lists_join; hybrid.py:293-307 on lists of any int64 ids).
    ids[s] [Q, k_s] int64, lens[s] [Q] int32 (entries past a list's length are never read), k_s may differ between systems.
    method: 'rrf' | 'bcf' (contributions from the list positions, float64), 'wsum32' (values[s] [Q, k_s] float32, fl32(value * w),
    float32 sum) or 'wsum64' (values float32 or float64 per system, narrow[s] as in fuse_wsum; float64 sum).
    Returns (out_ids [Q, n] int64, out_scores [Q, n], out_len [Q] int32), n = sum of k_s, the columns in the fused dict's
    first-insertion order: sort_rows_desc(out_scores, row_len=out_len) ranks them with the reference's tie rule.  Columns past
    out_len hold (-1, -inf).  An id listed twice inside one list raises ValueError (one flag read per call)."""
    _need(method in LISTS_METHODS, f"lists_join: unknown method {method!r} (one of {sorted(LISTS_METHODS)})")
    S = len(ids)
    wsum = method in ("wsum32", "wsum64")
    if wsum:
        _need(values is not None and len(values) == S, f"lists_join({method}): needs {S} value planes")
        _need(weights is not None and len(weights) == S, f"lists_join({method}): needs {S} weights")
    ids, lens, vals, Q, total, n_h, ld_h = _lists_args("lists_join", ids, lens, values if wsum else None, f64_ok=method == "wsum64")
    dev = ids[0].device
    ld_out = max(round_up(total, _PAD), _PAD)
    f32 = method == "wsum32"
    out_ids = torch.full((max(Q, 1), ld_out), -1, dtype=torch.int64, device=dev)[:Q, :total]
    out_scores = torch.full((max(Q, 1), ld_out), float("-inf"), dtype=torch.float32 if f32 else torch.float64, device=dev)[:Q, :total]
    out_len = torch.zeros(Q, dtype=torch.int32, device=dev)
    lib = _lib.lib()
    wsb = int(lib.fz_lists_join_workspace_bytes(S, Q))
    ws = torch.zeros(max(wsb, 4), dtype=torch.uint8, device=dev)
    w = (C.c_double * S)(*[float(x) for x in weights]) if wsum else None
    v64 = (C.c_int32 * S)(*[int(v.dtype == torch.float64) for v in vals]) if wsum else None
    nr = (C.c_int32 * S)(*[int(bool(x)) for x in (narrow if narrow is not None else [False] * S)]) if method == "wsum64" else None
    check(lib.fz_lists_join(_ptr_array(ids), _ptr_array(lens), _ptr_array(vals) if wsum else None, v64, w, nr, n_h, ld_h, S, Q,
                            LISTS_METHODS[method], _ptr(out_ids), _ptr(out_scores), _ptr(out_len), ld_out, _ptr(ws), ws.numel(),
                            _stream(ids[0])), "fz_lists_join")
    if Q > 0 and total > 0:
        _lists_no_duplicate("lists_join", ws)
    return out_ids, out_scores, out_len


def lists_columns(ids: list[torch.Tensor], lens: list[torch.Tensor], values: list[torch.Tensor] | None = None,
                  gold_ids: torch.Tensor | None = None):
    """The per-query id join of lists_join, to per-system COLUMNS instead of one fused row (fz_lists_columns): the form gold_ranks /
    tune_metrics take, for top-k lists over any int64 ids.  ids[s] [Q, k_s] int64, lens[s] [Q] int32, values[s] [Q, k_s] float32
    (None: an ids / pos / gold-only join), gold_ids [Q, G] int64 (negative = padding; None: no gold look-up).
    Returns (out_ids [Q, n] int64, T: list of S [Q, n] float32 planes (None without values), pos [Q, n] int32, out_len [Q] int32,
    gold_col [Q, G] int32), n = sum of k_s, every plane with the same row stride.  Column c < out_len[q] is the c-th id of the
    fused dict's first-insertion order: out_ids holds the id (-1 beyond out_len), T[s] system s's value for it (+0.0 where s does
    not list it, and beyond out_len), pos holds c (-1 beyond); gold_col holds the column of each gold id, -1 for padding or an id in
    no list.  An id listed twice inside one list raises ValueError (one flag read per call)."""
    ids, lens, vals, Q, total, n_h, ld_h = _lists_args("lists_columns", ids, lens, values)
    S = len(ids)
    dev = ids[0].device
    if gold_ids is None:
        gold_ids = torch.empty((Q, 0), dtype=torch.int64, device=dev)
    _dev(gold_ids, torch.int64, "lists_columns(gold_ids)")
    _need(gold_ids.dim() == 2 and gold_ids.shape[0] == Q, f"lists_columns(gold_ids): expected a [{Q}, G] tensor, got {tuple(gold_ids.shape)}")
    gold_ids = gold_ids.contiguous()
    G = int(gold_ids.shape[1])
    out_len = torch.empty(Q, dtype=torch.int32, device=dev)
    gold_col = torch.empty((Q, G), dtype=torch.int32, device=dev)
    out_ids = alloc_plane(Q, total, torch.int64, dev)
    pos = alloc_plane(Q, total, torch.int32, dev)
    T = [alloc_plane(Q, total, torch.float32, dev) for _ in range(S)] if vals is not None else None
    if Q == 0 or total == 0:                # nothing to join, nothing launched: the (empty) planes aside, no list holds any id
        out_len.zero_(); gold_col.fill_(-1)
        return out_ids, T, pos, out_len, gold_col
    ld_out = _same_ld(out_ids, pos, *(T or []))
    lib = _lib.lib()
    ws = torch.empty(max(int(lib.fz_lists_columns_workspace_bytes(S, Q)), 4), dtype=torch.uint8, device=dev)
    check(lib.fz_lists_columns(_ptr_array(ids), _ptr_array(lens), _ptr_array(vals) if vals is not None else None, n_h, ld_h, S, Q,
                               _ptr(gold_ids) if G else None, G, _ptr(out_ids), _ptr_array(T) if T is not None else None, _ptr(pos),
                               _ptr(out_len), _ptr(gold_col) if G else None, ld_out, _ptr(ws), ws.numel(), _stream(ids[0])),
          "fz_lists_columns")
    _lists_no_duplicate("lists_columns", ws)
    return out_ids, T, pos, out_len, gold_col


def _flag_word(ws: torch.Tensor) -> int:
    """The one flag read of a call: the int32 at offset 0 of its workspace."""
    return int(ws[:4].view(torch.int32).item())


def lists_collapse(ids: torch.Tensor, scores: torch.Tensor, lens: torch.Tensor, group_of: torch.Tensor, *, id_base: int = 0,
                   doc_id_base: int = 0, scores64: torch.Tensor | None = None):
    """One PASSAGE top-k list per query -> the DOCUMENT list, MaxP (fz_lists_collapse).  ids [Q, n] int64 passage ids in
    (score desc, id asc) order, scores [Q, n] float32, scores64 [Q, n] float64 or None, lens [Q] int32 (entries past a list's length are
    never read); passage id p + id_base belongs to document group_of[p] + doc_id_base (group_of [P] int32, non-decreasing).
    Returns (doc_ids [Q, n] int64, doc_scores [Q, n] float32, doc_scores64 or None, best [Q, n] int64, out_len [Q] int32): column c is
    the c-th distinct document of the list -- in a ranked list its MaxP rank --, with the score bits and the passage id of the document's
    first (= best) entry; (-1, -inf, -1) from out_len on.  ValueError for a passage id outside [id_base, id_base + P), for a row whose
    scores are not non-increasing (NaN included) and for n beyond lists_max_entries() (one flag read per call)."""
    _dev(ids, torch.int64, "lists_collapse(ids)")
    _dev(scores, torch.float32, "lists_collapse(scores)")
    _dev(lens, torch.int32, "lists_collapse(lens)")
    _dev(group_of, torch.int32, "lists_collapse(group_of)")
    _need(ids.dim() == 2, f"lists_collapse(ids): expected a [Q, n] tensor, got {tuple(ids.shape)}")
    Q, n = int(ids.shape[0]), int(ids.shape[1])
    _need(tuple(scores.shape) == (Q, n), f"lists_collapse(scores): ids are {(Q, n)} but scores {tuple(scores.shape)}")
    _need(lens.numel() == Q, f"lists_collapse(lens): expected {Q} lengths, got {lens.numel()}")
    _need(group_of.dim() == 1, f"lists_collapse(group_of): expected a [P] tensor, got {tuple(group_of.shape)}")
    if scores64 is not None:
        _dev(scores64, torch.float64, "lists_collapse(scores64)")
        _need(tuple(scores64.shape) == (Q, n), f"lists_collapse(scores64): ids are {(Q, n)} but scores64 {tuple(scores64.shape)}")
    cap = lists_max_entries()
    _need(n <= cap, f"lists_collapse: the list of one query holds up to {n} entries, a collapse takes at most {cap} (fz_lists_max_entries)")
    planes = [ids, scores] + ([scores64] if scores64 is not None else [])
    if len({max(_ld(t), n) for t in planes}) > 1:      # one row stride for the list's planes
        planes = [t.contiguous() for t in planes]
    ids, scores = planes[0], planes[1]
    scores64 = planes[2] if scores64 is not None else None
    lens, group_of = lens.contiguous(), group_of.contiguous()
    dev = ids.device
    out_ids = alloc_plane(Q, n, torch.int64, dev)
    out_sc = alloc_plane(Q, n, torch.float32, dev)
    out_sc64 = alloc_plane(Q, n, torch.float64, dev) if scores64 is not None else None
    best = alloc_plane(Q, n, torch.int64, dev)
    out_len = torch.zeros(Q, dtype=torch.int32, device=dev)
    if Q == 0 or n == 0:
        return out_ids, out_sc, out_sc64, best, out_len
    ld_out = _same_ld(out_ids, out_sc, best, out_sc64)
    lib = _lib.lib()
    ws = torch.empty(max(int(lib.fz_lists_collapse_workspace_bytes(Q)), 4), dtype=torch.uint8, device=dev)
    check(lib.fz_lists_collapse(_ptr(ids), _ptr(scores), _ptr(scores64), _ptr(lens), max(_ld(ids), n), n, Q, _ptr(group_of),
                                int(group_of.numel()), int(id_base), int(doc_id_base), _ptr(out_ids), _ptr(out_sc), _ptr(out_sc64),
                                _ptr(best), _ptr(out_len), ld_out, _ptr(ws), ws.numel(), _stream(ids)), "fz_lists_collapse")
    flag = _flag_word(ws)
    if flag & 1:
        raise ValueError(f"lists_collapse: a list holds a passage id outside [{int(id_base)}, {int(id_base) + int(group_of.numel())}) "
                         "(the passages of the group table)")
    if flag & 2:
        raise ValueError("lists_collapse: a list is not in descending score order (or holds NaN): MaxP by first occurrence needs a ranked list")
    return out_ids, out_sc, out_sc64, best, out_len


def group_expand(cand: torch.Tensor, cand_len: torch.Tensor | None, poff: torch.Tensor, ldp: int, *, id_base: int = 0,
                 doc_id_base: int = 0):
    """Candidate DOCUMENT ids -> their passages (fz_group_expand).  cand [Q, W] int64 (rows may be strided), cand_len [Q] int32 or None
    (= W everywhere), poff [D + 1] int64: document d + doc_id_base owns passages poff[d] + id_base .. poff[d + 1] + id_base - 1.
    Returns (pcand [Q, ldp] int64 -- slot 0's passages first, then slot 1's, ...; -1 from pcand_len on --, seg [Q, W + 1] int32 segment
    offsets, pcand_len [Q] int32).  A padded slot, a negative or unknown id and a document without passages get an empty segment.
    ValueError when a row needs more than ldp slots (one flag read per call)."""
    _dev(cand, torch.int64, "group_expand(cand)")
    _dev(poff, torch.int64, "group_expand(poff)")
    _need(cand.dim() == 2, f"group_expand(cand): expected a [Q, W] tensor, got {tuple(cand.shape)}")
    _need(poff.dim() == 1 and poff.numel() >= 1, f"group_expand(poff): expected a [D + 1] tensor, got {tuple(poff.shape)}")
    Q, W, ldp = int(cand.shape[0]), int(cand.shape[1]), int(ldp)
    _need(ldp >= 0, f"group_expand: ldp = {ldp} is negative")
    if cand_len is not None:
        _dev(cand_len, torch.int32, "group_expand(cand_len)")
        _need(tuple(cand_len.shape) == (Q,), f"group_expand(cand_len): expected shape {(Q,)}, got {tuple(cand_len.shape)}")
    poff = poff.contiguous()
    dev = cand.device
    pcand = torch.empty((Q, ldp), dtype=torch.int64, device=dev)
    seg = torch.empty((Q, W + 1), dtype=torch.int32, device=dev)
    pcand_len = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q == 0:
        return pcand, seg, pcand_len
    lib = _lib.lib()
    ws = torch.empty(max(int(lib.fz_group_expand_workspace_bytes(Q)), 4), dtype=torch.uint8, device=dev)
    check(lib.fz_group_expand(_ptr(cand), max(_ld(cand), W), _ptr(cand_len), W, Q, _ptr(poff), int(poff.numel()) - 1, int(id_base),
                              int(doc_id_base), _ptr(pcand), ldp, _ptr(seg), _ptr(pcand_len), _ptr(ws), ws.numel(), _stream(cand)),
          "fz_group_expand")
    if _flag_word(ws) != 0:
        raise ValueError(f"group_expand: the passages of one query's candidates do not fit ldp = {ldp} slots")
    return pcand, seg, pcand_len


def group_max(pscores: torch.Tensor, pcand: torch.Tensor, seg: torch.Tensor, cand_len: torch.Tensor | None = None,
              out: torch.Tensor | None = None, best: torch.Tensor | None = None):
    """The maximum over every slot's segment of passage scores (fz_group_max_f32 / _f64).  pscores [Q, ldp] float32 or float64 (the pair
    scores of group_expand's pcand [Q, ldp]), seg [Q, W + 1] int32, cand_len [Q] int32 or None.  Returns (out [Q, W] of pscores' dtype,
    best [Q, W] int64): the winning entry's own bits and the passage id of the first maximum (the lowest passage id among equals);
    (-inf, -1) for an empty segment and for a slot past cand_len.  `out` / `best` may be views into wider planes of one row stride."""
    _dev(pscores, None, "group_max(pscores)")
    if pscores.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"group_max: passage scores must be float32 or float64, got {pscores.dtype}")
    _dev(pcand, torch.int64, "group_max(pcand)")
    _dev(seg, torch.int32, "group_max(seg)")
    _need(pcand.dim() == 2 and seg.dim() == 2 and seg.shape[0] == pcand.shape[0] and seg.shape[1] >= 1,
          f"group_max: pcand [Q, ldp] and seg [Q, W + 1] expected, got {tuple(pcand.shape)} and {tuple(seg.shape)}")
    Q, ldp, W = int(pcand.shape[0]), int(pcand.shape[1]), int(seg.shape[1]) - 1
    _need(tuple(pscores.shape) == (Q, ldp), f"group_max(pscores): pcand is {(Q, ldp)} but the scores are {tuple(pscores.shape)}")
    pcand, seg = pcand.contiguous(), seg.contiguous()
    if cand_len is not None:
        _dev(cand_len, torch.int32, "group_max(cand_len)")
        _need(tuple(cand_len.shape) == (Q,), f"group_max(cand_len): expected shape {(Q,)}, got {tuple(cand_len.shape)}")
    dev = pscores.device
    if out is None:
        out = alloc_plane(Q, W, pscores.dtype, dev)
    if best is None:
        best = alloc_plane(Q, W, torch.int64, dev)
    _dev(out, pscores.dtype, "group_max(out)")
    _dev(best, torch.int64, "group_max(best)")
    _need(tuple(out.shape) == (Q, W) and tuple(best.shape) == (Q, W), f"group_max: out and best must be {(Q, W)}")
    if Q == 0 or W == 0:
        return out, best
    ld_out = _same_ld(out, best)
    fn = _lib.lib().fz_group_max_f32 if pscores.dtype == torch.float32 else _lib.lib().fz_group_max_f64
    check(fn(_ptr(pscores), max(_ld(pscores), ldp), _ptr(pcand), ldp, _ptr(seg), _ptr(cand_len), W, Q, _ptr(out), _ptr(best), ld_out,
             _stream(pscores)), "fz_group_max")
    return out, best


def gold_ranks(T: list[torch.Tensor], pos: torch.Tensor, weights: torch.Tensor, gold: torch.Tensor) -> torch.Tensor:
    """Fused ranks of the gold documents for every weight vector (N1, hybrid.py:404-426).
    T[s] [Q,N] normalised planes, pos [Q,N] int32 insertion positions (-1 absent), weights [W,S] fp32,
    gold [Q,G] int32 corpus positions (-1 pad) -> ranks [W,Q,G] int32 (0 where gold is padding / unlisted: check pos).
    float64 weights select the float64 sweep (np.float64 grid weights: NumPy promotes the products and sums)."""
    _max_systems(len(T), "gold_ranks")
    for t in T:
        _dev(t, torch.float32, "gold_ranks(T)")
    _dev(pos, torch.int32, "gold_ranks(pos)")
    _dev(weights, None, "gold_ranks(weights)")
    if weights.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"gold_ranks(weights): expected float32 or float64, got {weights.dtype}")
    _dev(gold, torch.int32, "gold_ranks(gold)")
    lib = _lib.lib()
    G = int(lib.fz_tune_max_gold())
    _same_shape(list(T) + [pos], "gold_ranks")
    both = harmonise(list(T) + [pos])
    T, pos = both[:-1], both[-1]
    Q, N = T[0].shape
    W, S = weights.shape
    if S != len(T) or gold.shape != (Q, G):
        raise ValueError(f"weights must be [W,{len(T)}] and gold [Q,{G}]")
    ld = _same_ld(*T, pos)
    out = torch.zeros((W, Q, G), dtype=torch.int32, device=T[0].device)
    fn = lib.fz_gold_ranks_f64w if weights.dtype == torch.float64 else lib.fz_gold_ranks_f32
    # the contiguous copies stay referenced until the launch is queued: a copy made inside the argument list dies at once, and the
    # allocator hands its block to the NEXT copy made there (strided weights AND strided gold: the sweep read the golds as weights)
    weights, gold = weights.contiguous(), gold.contiguous()
    check(fn(_ptr_array(T), _ptr(pos), _ptr(weights), _ptr(gold), S, W, Q, N, ld, _ptr(out), _stream(T[0])),
          "fz_gold_ranks")
    return out


def tune_metrics(ranks: torch.Tensor, gold: torch.Tensor, pos: torch.Tensor, n_gold: torch.Tensor, idcg: torch.Tensor,
                 disc: torch.Tensor, cuts: dict[str, list[int]]) -> torch.Tensor:
    """run_evaluation's metrics for every weight vector from the gold ranks of gold_ranks(), on the device (N1).
    ranks [W,Q,G] int32, gold [Q,G] int32, pos [Q,N] int32 plane, n_gold [Q] int32, idcg [Q] float64, disc [top+1] float64,
    cuts = {"recall": [...], "map": [...], "mrr": [...], "ndcg": [...]} -> [W, M] float64, columns in that order + R-precision."""
    _dev(ranks, torch.int32, "tune_metrics(ranks)"); _dev(gold, torch.int32, "tune_metrics(gold)")
    _dev(pos, torch.int32, "tune_metrics(pos)"); _dev(n_gold, torch.int32, "tune_metrics(n_gold)")
    _dev(idcg, torch.float64, "tune_metrics(idcg)"); _dev(disc, torch.float64, "tune_metrics(disc)")
    lib = _lib.lib()
    G = int(lib.fz_tune_max_gold())
    W, Q = ranks.shape[0], ranks.shape[1]
    if ranks.shape != (W, Q, G) or gold.shape != (Q, G) or pos.shape[0] != Q or n_gold.shape != (Q,) or idcg.shape != (Q,):
        raise ValueError("tune_metrics: ranks [W,Q,G], gold [Q,G], pos [Q,N], n_gold [Q], idcg [Q] expected")
    fam = [list(cuts.get(k, [])) for k in ("recall", "map", "mrr", "ndcg")]
    flat = [int(k) for f in fam for k in f]
    if disc.numel() < 1 or any(k < 0 for k in flat):
        raise ValueError("tune_metrics: a discount table and non-negative cut-offs expected")
    pos = as_plane(pos)
    cuts_dev = torch.tensor(flat if flat else [0], dtype=torch.int32, device=ranks.device)
    out = torch.empty((W, len(flat) + 1), dtype=torch.float64, device=ranks.device)
    ranks, gold, n_gold, idcg, disc = (t.contiguous() for t in (ranks, gold, n_gold, idcg, disc))   # referenced until the launch is queued (see gold_ranks)
    check(lib.fz_tune_metrics_f64(_ptr(ranks), _ptr(gold), _ptr(pos), pos.stride(0), _ptr(n_gold),
                                  _ptr(idcg), _ptr(disc), int(disc.numel()) - 1, _ptr(cuts_dev), len(fam[0]),
                                  len(fam[1]), len(fam[2]), len(fam[3]), W, Q, _ptr(out), _stream(ranks)), "fz_tune_metrics_f64")
    return out


# ---------------------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------------------
def topk_rows(scores: torch.Tensor, k: int, id_base: int = 0):
    """k best per row by (score desc, id asc) -> (scores [rows,k] f32, ids [rows,k] int64)."""
    _dev(scores, torch.float32, "topk_rows(scores)")
    rows, n = scores.shape
    dev = scores.device
    os_ = torch.empty((rows, k), dtype=torch.float32, device=dev)
    oi = torch.empty((rows, k), dtype=torch.int64, device=dev)
    lib = _lib.lib()
    wsb = int(lib.fz_topk_workspace_bytes(rows, n, k))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(lib.fz_topk_rows_f32(_ptr(scores), rows, n, _ld(scores), k, int(id_base), _ptr(os_), _ptr(oi), _ptr(ws), wsb, _stream(scores)),
          "fz_topk_rows_f32")
    return os_, oi


def topk_update(scores: torch.Tensor, id_base: int, run_scores: torch.Tensor, run_ids: torch.Tensor, cap: int = 7168,
                overflow: torch.Tensor | None = None):
    """Merge one more chunk of scores into the running top-k (streaming threshold filter + small sort).
    Returns (new_scores, new_ids, overflow_flag_tensor); the caller checks the flag once at the end of the search.
    Precondition (include/fusion_hip.h, fz_topk_update_f32): the running list is full (k real entries) or no score is -inf -- against a
    short list's threshold of -inf a later score of exactly -inf is dropped and stays (-inf, -1) padding, where topk_rows of the whole
    matrix lists its id."""
    _dev(scores, torch.float32, "topk_update(scores)")
    _dev(run_scores, torch.float32, "topk_update(run_scores)")
    _dev(run_ids, torch.int64, "topk_update(run_ids)")
    rows, n = scores.shape
    k = run_scores.shape[1]
    _need(tuple(run_scores.shape) == (rows, k) and tuple(run_ids.shape) == (rows, k), f"topk_update: running lists must be [{rows}, k]")
    dev = scores.device
    lib = _lib.lib()
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
        _dev(overflow, torch.int32, "topk_update(overflow)")
    ns = torch.empty((rows, k), dtype=torch.float32, device=dev)
    ni = torch.empty((rows, k), dtype=torch.int64, device=dev)
    wsb = int(lib.fz_topk_update_workspace_bytes(rows, k, cap))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    run_scores, run_ids = run_scores.contiguous(), run_ids.contiguous()     # referenced until the launch is queued (see gold_ranks)
    check(lib.fz_topk_update_f32(_ptr(scores), rows, n, _ld(scores), int(id_base), _ptr(run_scores), _ptr(run_ids), k, cap,
                                 _ptr(ns), _ptr(ni), _ptr(overflow), _ptr(ws), wsb, _stream(scores)), "fz_topk_update_f32")
    return ns, ni, overflow


@functools.lru_cache(maxsize=None)
def fold_max_k(unordered: bool) -> int:
    """The largest k fz_topk_fold_f32 takes (fz_topk_fold_max_k): 5,056 for candidates in arrival order, 35,839 for ordered ones.  A constant
    of the library: asked once."""
    return int(_lib.lib().fz_topk_fold_max_k(1 if unordered else 0))


def tune_max_gold() -> int:
    """The gold ids per query one launch of the weight sweep's counting kernel takes (fz_tune_max_gold)."""
    return int(_lib.lib().fz_tune_max_gold())


def stream_window(seen: int, k: int, cap: int) -> int:
    """Documents one threshold of a TopkStream may serve: expected candidates k * window / seen <= cap / 2."""
    return max(64, (cap // 2) * seen // k // 64 * 64)


def stream_pieces(lo: int, hi: int, seen: int, pending: int, k: int, cap: int, grain: int = 1):
    """How a TopkStream cuts a source's documents [lo, hi): [(lo, hi, fold after this piece)], ascending and back to back.  The fold window
    (stream_window) is rounded down to whole grains (1, or the sparse kernels' slice), at least one; a piece ends where the window does (or
    at hi, which may be off the grain) and the stream folds there; the bookkeeping -- seen, pending -- is TopkStream's own.  Host arithmetic only."""
    out = []
    while lo < hi:
        win = max(grain, stream_window(seen, k, cap) // grain * grain)
        room = max(grain, (win - pending) // grain * grain)
        end = min(hi, lo + room)
        pending += end - lo
        fold = pending >= win
        if fold:
            seen, pending = seen + pending, 0
        out.append((lo, end, fold))
        lo = end
    return out


class _Source:
    """What a TopkStream is fed from: the scorer of n documents, [lo, hi) in its own numbering, for the stream's queries.  filter(stream, lo,
    hi) launches its filter kernel against the stream's thresholds and candidate buffers; plane(lo, hi) -> (scores [rows, hi - lo], id of
    column 0) is the same piece materialised, for the exact redo of an overflowed window.  grain: pieces start on a multiple of it; unordered:
    candidates arrive in no particular order; mark: the name reported after a launch; held: the stream may keep it (views, no copies)."""

    def __init__(self, n, filter, plane, grain=1, unordered=True, mark=None, held=True):
        self.n, self.filter, self.plane, self.grain, self.unordered, self.mark, self.held = n, filter, plane, grain, unordered, mark, held


def _plane_source(scores, id_base: int, held: bool) -> _Source:
    """A materialised score plane, column c = document id_base + c (TopkStream.feed)."""
    def filter(st, lo, hi):
        check(_lib.lib().fz_topk_filter_append_f32(_ptr(scores[:, lo:hi]), st.rows, hi - lo, _ld(scores), id_base + lo, _ptr(st.tau), _ptr(st.cand_s),
                                                   _ptr(st.cand_i), _ptr(st.cand_len), st.cap, _ptr(st.overflow), _stream(scores)),
              "fz_topk_filter_append_f32")
    return _Source(scores.shape[1], filter, lambda lo, hi: (scores[:, lo:hi], id_base + lo), unordered=False, held=held)


def _gemm_source(Qn, Dn, id_base: int) -> _Source:
    """The GEMM whose epilogue is the filter, row r of Dn = document id_base + r (TopkStream.feed_gemm, ShardedDenseIndex)."""
    Qn, Dn = Qn.contiguous(), Dn.contiguous()

    def filter(st, lo, hi):
        check(_lib.lib().fz_dot_scores_filter_f32(_ptr(Qn), Qn.stride(0), _ptr(Dn[lo:hi]), Dn.stride(0), st.rows, hi - lo, Qn.shape[1], id_base + lo,
                                                  _ptr(st._tau_pad), _ptr(st.cand_s), _ptr(st.cand_i), _ptr(st.cand_len), st.cap, _ptr(st.overflow),
                                                  _stream(Qn)), "fz_dot_scores_filter_f32")
    return _Source(Dn.shape[0], filter, lambda lo, hi: (dot_scores(Qn, Dn[lo:hi]), id_base + lo), mark="shard_gemm_filter")


def _sparse_source(index, qoff, qterms, qw, id_base: int) -> _Source:
    """The posting walk whose epilogue is the filter, document d of the index = id id_base + d (TopkStream.feed_sparse, ShardedSparseIndex)."""
    def filter(st, lo, hi):
        check(_lib.lib().fz_sparse_dot_filter_f32(_ptr(index.toff), _ptr(index.pdoc), _ptr(index.pw), _ptr(index.slice_off), _ptr(qoff), _ptr(qterms),
                                                  _ptr(qw), st.rows, index.N, lo, hi, id_base, _ptr(st.tau), _ptr(st.cand_s), _ptr(st.cand_i),
                                                  _ptr(st.cand_len), st.cap, _ptr(st.overflow), _stream(qoff)), "fz_sparse_dot_filter_f32")
    return _Source(index.N, filter, lambda lo, hi: (sparse_dot(index, qoff, qterms, qw, doc_lo=lo, doc_hi=hi), id_base + lo),
                   grain=sparse_slice_docs(), mark="shard_sparse_filter")


class TopkStream:
    """Running per-row top-k over a stream of score chunks (documents in ascending id order): only scores above a row's
    threshold (its k-th best when the list was last folded) are kept as candidates (fz_topk_filter_append_f32), and candidates
    are folded into the list (fz_topk_fold_f32: one row sort) only when their EXPECTED number -- k * (documents since the fold) /
    (documents before it), for scores in no particular order -- reaches half the candidate capacity.  The windows between folds
    therefore grow geometrically: 4 folds for a 1.1 M-document shard at k = 1000, cap = 7168 after an 8192-document head, however the scoring is chunked.
    `overflow` (device int32) becomes 1 if a row had more than `cap` candidates in a window.  With `exact_on_overflow` (default) the
    flag is read at every fold (one small device -> host read per window: 4 per 1.1 M-document shard) and an overflowed WINDOW is redone
    exactly -- per-piece top-k (fz_topk_rows_f32) merged into the list as it stood before the window -- so a corpus ordered by relevance
    (every window overflows) costs the exact search once, not a wasted streaming pass plus the exact search of the whole shard;
    `windows_redone` counts them.  That needs what the window was fed with: feed_gemm's and feed_sparse's pieces are views of their
    inputs (kept: no copies); feed()'s score buffers are kept only on request (hold=True) -- otherwise, and without exact_on_overflow,
    the flag stays set and the caller redoes the search.  The feeds differ only in their _Source; the loop is _feed's.  The float64
    ranking (TopkStream64) shares all of it, fold's overflow protocol included: a ranking is _alloc, _fold_candidates, plane_topk, _merge.
    Precondition: the list the stream starts from is full (k real entries; the index classes start from a head of >= 8 k documents) or no
    score is -inf -- a short list's threshold is -inf and the filter keeps !(s <= tau), so a later score of exactly -inf stays padding.
    An unordered source (feed_gemm, feed_sparse) needs k <= fold_max_k(True) = 5,056: ValueError before the first filter launch."""

    dtype = torch.float32        # of the lists, the thresholds and the candidate scores
    _fold_writes_tau = True      # fz_topk_fold_f32 rewrites tau and clears cand_len itself
    _can_redo = True             # plane_topk is there for an overflowed window
    _ranking = {}                # what plane_topk takes besides (plane, k, base)
    _fold_limits_k = True        # the fold is fz_topk_fold_f32: k <= fold_max_k(unordered)

    def __init__(self, run_scores: torch.Tensor, run_ids: torch.Tensor, seen: int, cap: int = 7168, exact_on_overflow: bool = True):
        what = type(self).__name__
        _dev(run_scores, self.dtype, f"{what}(run_scores)"); _dev(run_ids, torch.int64, f"{what}(run_ids)")
        rows, k = run_scores.shape
        _need(tuple(run_ids.shape) == (rows, k) and seen > 0 and cap > 0, f"{what}: lists [rows, k], seen > 0, cap > 0 expected")
        dev = run_scores.device
        self.rows, self.k, self.cap = rows, k, int(cap)
        self.best_s, self.best_i = run_scores.contiguous(), run_ids.contiguous()
        self._alloc(dev)
        self.tau.copy_(self.best_s[:, k - 1])
        self.unordered = False           # candidates appended by the fused feeds arrive in no particular order
        self.cand_s = torch.empty((rows, cap), dtype=self.dtype, device=dev)
        self.cand_i = torch.empty((rows, cap), dtype=torch.int64, device=dev)
        self.cand_len = torch.zeros(rows, dtype=torch.int32, device=dev)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        self.seen = int(seen)            # documents folded into (best_s, tau)
        self.pending = 0                 # documents filtered against tau since
        self.exact_on_overflow = bool(exact_on_overflow)
        self.windows_redone = 0
        self._pieces = []                # what the current window was fed with: (source, lo, hi)
        self._unheld = False             # ... and whether some of it was fed without being held (feed(hold=False))
        self.unrepairable = False        # host latch: a window fed WITHOUT hold (or with no plane_topk) overflowed -- nothing the stream holds can
                                         #   repair it, the device flag stays set and the caller redoes the search; later windows are neither read nor redone

    # -- the float32 ranking: the sort kernels' own top-k, fold and merge entries --
    def _alloc(self, dev):
        # tau [rows] and what _fold_candidates works in.  Thresholds are padded to whole 128-query GEMM blocks with +inf (the fused GEMM reads its tile's 128 rows unconditionally)
        self._tau_pad = torch.full((round_up(max(self.rows, 1), 128),), float("inf"), dtype=torch.float32, device=dev)
        self.tau = self._tau_pad[:self.rows]
        wsb = int(_lib.lib().fz_topk_fold_workspace_bytes(self.rows, self.k, self.cap))
        self._ws, self._wsb = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev), wsb

    def _fold_candidates(self):      # the window's candidates folded into the list -> the new (scores, ids)
        ns, ni = torch.empty_like(self.best_s), torch.empty_like(self.best_i)
        check(_lib.lib().fz_topk_fold_f32(_ptr(self.best_s), _ptr(self.best_i), self.rows, self.k, _ptr(self.cand_s), _ptr(self.cand_i),
                                          _ptr(self.cand_len), self.cap, 1 if self.unordered else 0, _ptr(ns), _ptr(ni), _ptr(self.tau),
                                          _ptr(self.overflow), _ptr(self._ws), self._wsb, _stream(self.best_s)), "fz_topk_fold_f32")
        return ns, ni

    @staticmethod
    def plane_topk(scores, k: int, base: int):
        """The exact top-k (scores, ids) of a plane whose column 0 has the id `base`: a search's head, a piece of an overflowed window."""
        return topk_rows(scores, k, id_base=base)

    @staticmethod
    def _merge(s, i, ps, pi):    # a later piece's ranked list onto the running one (ties by ascending id, as everywhere)
        return topk_merge(torch.stack([s, ps]), torch.stack([i, pi]))

    def _feed(self, source, lo: int, hi: int, mark=None):
        """The source's documents [lo, hi), cut at the fold windows (stream_pieces): one filter launch per piece, a fold where planned."""
        unordered = self.unordered or source.unordered
        if self._fold_limits_k and self.k > fold_max_k(unordered):     # (before anything is launched or latched: the fold would refuse this k)
            raise ValueError(f"{type(self).__name__}: k = {self.k} exceeds what the fold of {'unordered' if unordered else 'ordered'} "
                             f"candidates takes ({fold_max_k(unordered)})")
        self.unordered = self.unordered or source.unordered
        for lo, hi, fold in stream_pieces(lo, hi, self.seen, self.pending, self.k, self.cap, source.grain):
            source.filter(self, lo, hi)
            if mark: mark(source.mark)
            if source.held:
                self._pieces.append((source, lo, hi))
            else:
                self._unheld = True          # this window saw scores the stream does not hold: no exact redo for it
            self.pending += hi - lo
            if fold:
                self.fold()
                if mark: mark("shard_topk_stream")

    def feed(self, scores: torch.Tensor, id_base: int, hold: bool = False):
        """scores [rows, n] of documents id_base .. id_base + n - 1.
        hold=False (default): nothing of `scores` is kept -- the caller may overwrite or free the buffer as soon as the call returns; a
        window fed this way cannot be redone, so if it overflows the `overflow` flag STAYS SET and the caller redoes the search
        (ShardedDenseIndex.local_topk does).  hold=True: the stream keeps a view of the piece until the window is folded and redoes an
        overflowed window exactly from it -- only for callers that leave the buffer untouched (and can afford it alive) until then."""
        _dev(scores, torch.float32, "TopkStream.feed(scores)")
        _need(scores.shape[0] == self.rows, "TopkStream.feed: one row per running list")
        self._feed(_plane_source(scores, int(id_base), hold), 0, scores.shape[1])

    def feed_gemm(self, Qn: torch.Tensor, Dn: torch.Tensor, id_base: int, mark=None):
        """Score documents id_base .. id_base + len(Dn) - 1 against the queries and keep what beats the thresholds, in ONE kernel:
        the GEMM's epilogue is the filter, the score plane is never written (fz_dot_scores_filter_f32).  Qn [rows, d], Dn [n, d]
        L2-normalised float32, d % 4 == 0.  The documents are cut at the fold windows, one GEMM launch per piece."""
        _dev(Qn, torch.float32, "TopkStream.feed_gemm(Qn)"); _dev(Dn, torch.float32, "TopkStream.feed_gemm(Dn)")
        _need(Qn.shape[0] == self.rows and Qn.shape[1] == Dn.shape[1] and Qn.shape[1] % 4 == 0, "TopkStream.feed_gemm: [rows, d] x [n, d], d % 4 == 0")
        self._feed(_gemm_source(Qn, Dn, int(id_base)), 0, Dn.shape[0], mark)

    def feed_sparse(self, index, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, doc_lo: int, doc_hi: int, id_base: int, mark=None):
        """Score documents [doc_lo, doc_hi) of a SparseIndex against the queries' term lists and keep what beats the thresholds, in ONE kernel
        per piece (fz_sparse_dot_filter_f32: the inverted-index walk with the filter in place of the plane store).  Document d gets the id
        id_base + d.  The range is cut at the fold windows, rounded down to whole slices; the pieces hold views of the index and the query
        lists, nothing is copied."""
        Q = _sparse_queries(qoff, qterms, qw, "TopkStream.feed_sparse")
        _need(Q == self.rows, "TopkStream.feed_sparse: one query per running list")
        doc_lo, doc_hi = _doc_range("TopkStream.feed_sparse", index.N, sparse_slice_docs(), doc_lo, doc_hi)
        self._feed(_sparse_source(index, qoff, qterms, qw, int(id_base)), doc_lo, doc_hi, mark)

    def fold(self):
        if self.pending == 0:
            return
        ns, ni = self._fold_candidates()
        redone = False
        # The device flag is read at the fold (one small device -> host read per window) for as long as the search can still come out
        # exact: once a window that cannot be redone has overflowed the caller redoes the whole search anyway, so later windows are neither
        # read nor redone (with one sticky device flag every later held window ran the full exact redo for nothing).  Every
        # earlier overflow was either repaired (flag cleared below) or latched, so a non-zero flag here is THIS window's.
        if self.exact_on_overflow and not self.unrepairable and int(self.overflow.item()) != 0:
            if self._unheld or not self._can_redo:
                self.unrepairable = True     # nothing to redo the window from: the flag stays set
            else:
                # a candidate list was cut short (or a tie run was too long to order): this window again, exactly, on top of the list as
                # it stood before it -- per piece: scores -> plane_topk -> _merge
                ns, ni = self.best_s, self.best_i
                for source, lo, hi in self._pieces:
                    sc, base = source.plane(lo, hi)
                    ns, ni = self._merge(ns, ni, *self.plane_topk(sc, self.k, base, **self._ranking))
                self.overflow.zero_()
                self.windows_redone += 1
                redone = True
        if redone or not self._fold_writes_tau:
            self.tau.copy_(ns[:, self.k - 1])
            self.cand_len.zero_()
        self._pieces.clear()
        self._unheld = False
        self.best_s, self.best_i = ns, ni
        self.seen += self.pending
        self.pending = 0

    def result(self):
        self.fold()
        return self.best_s, self.best_i, self.overflow


def stream_head_docs(k: int, grain: int, head_max: int) -> int:
    """Leading documents that get the exact top-k: 8 k, at least 8,192 (a 0.09 ms sort instead of 0.35 at k = 1000, one fold more), whole grains."""
    return round_up(min(head_max, max(8192, -(-8 * k // 4096) * 4096)), grain)


def stream_fits(k: int, cap: int, head: int, n: int, dtype=torch.float32) -> bool:
    """stream_search can run: list + candidates fit one sort row of the ranking's dtype, the head holds 8 k documents, more follow it."""
    return k + cap <= sort_max_n(dtype) and k <= head // 8 and n > head


def stream_chunk(chunk: int, grain: int) -> int:
    return max(grain, chunk // grain * grain)     # documents per feed: whole grains, at least one


def stream_search(src: _Source, k: int, head: int, chunk: int, cap: int, plane_mark: str, mark, cls=TopkStream, **ranking):
    """The streamed search of src.n documents -> (scores [rows, k], ids, windows redone exactly): the first `head` are scored into a plane
    and get the exact top-k, the rest goes through the source's filter in feeds of `chunk` (a stream of class `cls`; **ranking: what its
    constructor and plane_topk take besides).  mark(name) after every launch group: plane_mark, src.mark, 'shard_topk_stream' (top-k work)."""
    S, base = src.plane(0, head); mark(plane_mark)
    bs, bi = cls.plane_topk(S, k, base, **ranking)
    del S
    stream = cls(bs, bi, seen=head, cap=cap, **ranking); mark("shard_topk_stream")
    for c0 in range(head, src.n, chunk):
        stream._feed(src, c0, min(src.n, c0 + chunk), mark)
    best_s, best_i, _ = stream.result(); mark("shard_topk_stream")
    return best_s, best_i, stream.windows_redone


def topk_merge(in_scores: torch.Tensor, in_ids: torch.Tensor):
    """[G,rows,k] per-shard lists -> global top-k [rows,k] (after the RCCL all-gather)."""
    _dev(in_scores, torch.float32, "topk_merge(in_scores)")
    _dev(in_ids, torch.int64, "topk_merge(in_ids)")
    _need(in_scores.dim() == 3 and in_scores.shape == in_ids.shape, "topk_merge: scores and ids must both be [G, rows, k]")
    in_scores, in_ids = in_scores.contiguous(), in_ids.contiguous()
    G, rows, k = in_scores.shape
    os_ = torch.empty((rows, k), dtype=torch.float32, device=in_scores.device)
    oi = torch.empty((rows, k), dtype=torch.int64, device=in_scores.device)
    check(_lib.lib().fz_topk_merge(_ptr(in_scores), _ptr(in_ids), G, rows, k, _ptr(os_), _ptr(oi), _stream(in_scores)), "fz_topk_merge")
    return os_, oi


# ---------------------------------------------------------------------------------------
# BM25
# ---------------------------------------------------------------------------------------
def bm25_doc_norms(doc_len: torch.Tensor, avgdl: float, k1: float, b: float) -> torch.Tensor:
    """k1*(1-b+b*|d|/avgdl) per document (the per-document sub-expression of bm25.py:154), float64."""
    _dev(doc_len, torch.int32, "bm25_doc_norms(doc_len)")
    out = torch.empty(doc_len.numel(), dtype=torch.float64, device=doc_len.device)
    check(_lib.lib().fz_bm25_doc_norms_f64(_ptr(doc_len), doc_len.numel(), float(avgdl), float(k1), float(b), _ptr(out), _stream(doc_len)),
          "fz_bm25_doc_norms_f64")
    return out


# -- the host contract of the inverted-index entries (BM25 / TF-IDF, SPLADE, centroids: their kernels share csrc/slices.h) --
def _n_slices(N: int, slice_docs: int) -> int:
    """Slices of slice_docs documents in an index of N: the NS of its [rows, NS + 1] slice table."""
    return max(1, -(-int(N) // int(slice_docs)))


def _slice_table(what: str, slice_off, rows: int, N: int, kind: str):
    """slice_off is the contiguous [rows, NS + 1] int64 table of ops.<kind>_slice_offsets for N documents."""
    NS = _n_slices(N, getattr(_lib.lib(), f"fz_{kind}_slice_docs")())
    _need(_dev(slice_off, torch.int64, f"{what}(slice_off)").is_contiguous() and tuple(slice_off.shape) == (rows, NS + 1),
          f"{what}(slice_off): expected a contiguous [{rows}, {NS + 1}] table (ops.{kind}_slice_offsets)")


def _slice_offsets(kind: str, off: torch.Tensor, doc: torch.Tensor, rows: int | None, N: int) -> torch.Tensor:
    """[rows, NS + 1] int64: where every list (off [rows + 1] into doc, ascending inside a list) crosses the document slices one workgroup
    scores (fz_<kind>_slice_offsets / fz_<kind>_slice_docs; built once per index, like an idf table)."""
    what, lib = f"{kind}_slice_offsets", _lib.lib()
    _dev(off, torch.int64, f"{what}(offsets)"); _dev(doc, torch.int32, f"{what}(documents)")
    rows = off.numel() - 1 if rows is None else int(rows)
    _need(off.is_contiguous() and doc.is_contiguous() and off.numel() == rows + 1 >= 1, f"{what}: contiguous offsets [{rows + 1}] and documents expected")
    out = torch.empty((rows, _n_slices(N, getattr(lib, f"fz_{kind}_slice_docs")()) + 1), dtype=torch.int64, device=off.device)
    check(getattr(lib, f"fz_{kind}_slice_offsets")(_ptr(off), _ptr(doc), rows, int(N), _ptr(out), _stream(off)), f"fz_{kind}_slice_offsets")
    return out


def _doc_range(what: str, N: int, grain: int, doc_lo: int, doc_hi: int | None):
    """-> (doc_lo, doc_hi) of a range entry: it starts on a multiple of the walk's grain and ends on one or at N (the default)."""
    doc_lo, doc_hi = int(doc_lo), int(N) if doc_hi is None else int(doc_hi)
    _need(0 <= doc_lo <= doc_hi <= N and doc_lo % grain == 0 and (doc_hi % grain == 0 or doc_hi == N),
          f"{what}: [doc_lo, doc_hi) = [{doc_lo}, {doc_hi}) must start on a multiple of {grain} and end on one or at N = {N}")
    return doc_lo, doc_hi


def _cand_buffers(what: str, dtype, Q: int, tau, cand_s, cand_i, cand_len, overflow) -> int:
    """The buffers a filter entry appends to -> cap: cand_s (dtype) / cand_i int64 contiguous [Q, cap >= 1]; tau (dtype) and cand_len int32
    hold at least Q entries (the kernels read the first Q: a caller's guard rows may follow), overflow int32 at least one."""
    _dev(tau, dtype, f"{what}(tau)"); _dev(cand_s, dtype, f"{what}(cand_s)"); _dev(cand_i, torch.int64, f"{what}(cand_i)")
    _dev(cand_len, torch.int32, f"{what}(cand_len)"); _dev(overflow, torch.int32, f"{what}(overflow)")
    cap = cand_s.shape[1] if cand_s.dim() == 2 else 0
    _need(cap >= 1 and cand_s.is_contiguous() and cand_i.is_contiguous() and tuple(cand_s.shape) == (Q, cap) and tuple(cand_i.shape) == (Q, cap)
          and tau.numel() >= Q and cand_len.numel() >= Q and overflow.numel() >= 1,
          f"{what}: tau [Q], cand_s / cand_i [Q, cap >= 1] contiguous, cand_len [Q], overflow [1] expected")
    return cap


def bm25_slice_table_bytes(V: int, N: int) -> int:
    """Device bytes of bm25_slice_offsets' table for V terms over N documents: V x (NS + 1) int64."""
    return int(V) * (_n_slices(N, _lib.lib().fz_bm25_slice_docs()) + 1) * 8


def bm25_slice_offsets(toff: torch.Tensor, pdoc: torch.Tensor, N: int) -> torch.Tensor:
    """Per-index table [V, NS + 1] int64 for bm25_scores(slice_off=...) (fz_bm25_slice_offsets)."""
    return _slice_offsets("bm25", toff, pdoc, None, N)


def bm25_scores(toff, pdoc, ptf, idf, doc_len, avgdl: float, k1: float, b: float, qoff, qterms, Q: int, N: int,
                doc_norm: torch.Tensor | None = None, slice_off: torch.Tensor | None = None, want_f32: bool = False,
                pval: torch.Tensor | None = None):
    """BM25 scores [Q, N] float64 (bm25.py:149-156).  want_f32: also the float32 rounding of the same scores (the plane the normalisations
    read, hybrid.py:255), written by the same launch -> (float64 plane, float32 plane).  pval: the posting-value table of this index for
    this (k1, b) (bm25_posting_values): the walk then adds tabulated terms instead of dividing per posting -- same bits."""
    dev = idf.device
    if pval is not None:
        _contiguous("bm25_scores", (toff, torch.int64, "toff"), (pdoc, torch.int32, "pdoc"), (pval, torch.float64, "pval"), (qoff, torch.int64, "qoff"),
                    (qterms, torch.int32, "qterms"))
        _need(pval.numel() == pdoc.numel() and qoff.numel() == Q + 1, "bm25_scores: pval must hold one value per posting and qoff Q + 1 offsets")
        if slice_off is not None:
            _slice_table("bm25_scores", slice_off, toff.numel() - 1, N, "bm25")
        out = alloc_plane(Q, N, torch.float64, dev)
        out32 = alloc_plane(Q, N, torch.float32, dev) if want_f32 else None
        check(_lib.lib().fz_bm25_scores_pv_f64_f32(_ptr(toff), _ptr(pdoc), _ptr(pval), _ptr(slice_off), _ptr(qoff), _ptr(qterms), Q, N, _ptr(out),
                                                   _ld(out), _ptr(out32), _ld(out32) if want_f32 else 0, _stream(pval)), "fz_bm25_scores_pv_f64_f32")
        return (out, out32) if want_f32 else out
    _contiguous("bm25_scores", (toff, torch.int64, "toff"), (pdoc, torch.int32, "pdoc"), (ptf, torch.int32, "ptf"), (idf, torch.float64, "idf"),
                (doc_len, torch.int32, "doc_len"), (qoff, torch.int64, "qoff"), (qterms, torch.int32, "qterms"))
    _need(toff.numel() == idf.numel() + 1, "bm25_scores: toff must hold V + 1 offsets for idf's V terms")
    _need(pdoc.numel() == ptf.numel(), "bm25_scores: pdoc and ptf differ in length")
    _need(doc_len.numel() == N and qoff.numel() == Q + 1, f"bm25_scores: doc_len must hold {N} lengths and qoff {Q + 1} offsets")
    if doc_norm is not None:
        _need(_dev(doc_norm, torch.float64, "bm25_scores(doc_norm)").numel() == N and doc_norm.is_contiguous(), f"bm25_scores: doc_norm must hold {N} values")
    if slice_off is not None:
        _slice_table("bm25_scores", slice_off, idf.numel(), N, "bm25")
    out = alloc_plane(Q, N, torch.float64, dev)
    out32 = alloc_plane(Q, N, torch.float32, dev) if want_f32 else None
    check(_lib.lib().fz_bm25_scores_f64_f32(_ptr(toff), _ptr(pdoc), _ptr(ptf), _ptr(idf), _ptr(doc_len), _ptr(doc_norm), _ptr(slice_off), float(avgdl),
                                            float(k1), float(b), _ptr(qoff), _ptr(qterms), Q, N, _ptr(out), _ld(out), _ptr(out32),
                                            _ld(out32) if want_f32 else 0, _stream(idf)), "fz_bm25_scores_f64_f32")
    return (out, out32) if want_f32 else out


def bm25_posting_values(toff, pdoc, ptf, idf, doc_norm, k1: float) -> torch.Tensor:
    """[nnz] float64: every posting's BM25 term idf * (tf (k1 + 1)) / (tf + doc_norm[d]) (bm25.py:154) for the (k1, b) doc_norm was made
    with -- per index, like the idf table (fz_bm25_posting_values_f64); bm25_scores(pval=...) then only adds."""
    _contiguous("bm25_posting_values", (toff, torch.int64, "toff"), (pdoc, torch.int32, "pdoc"), (ptf, torch.int32, "ptf"), (idf, torch.float64, "idf"),
                (doc_norm, torch.float64, "doc_norm"))
    _need(toff.numel() == idf.numel() + 1 and pdoc.numel() == ptf.numel(), "bm25_posting_values: toff [V + 1], idf [V], pdoc / ptf [nnz] expected")
    out = torch.empty(pdoc.numel(), dtype=torch.float64, device=idf.device)
    check(_lib.lib().fz_bm25_posting_values_f64(_ptr(toff), _ptr(pdoc), _ptr(ptf), _ptr(idf), _ptr(doc_norm), idf.numel(), pdoc.numel(), float(k1),
                                                _ptr(out), _stream(idf)), "fz_bm25_posting_values_f64")
    return out


def tfidf_scores(toff, pdoc, ptf, idf, qoff, qterms, Q: int, N: int, slice_off: torch.Tensor | None = None, want_f32: bool = False):
    """TF-IDF scores [Q, N] float64 (TFIDF.score, bm25.py:108-115: sum over the query's terms, in query order, of tf * idf); want_f32: also
    their float32 rounding from the same launch."""
    dev = idf.device
    _contiguous("tfidf_scores", (toff, torch.int64, "toff"), (pdoc, torch.int32, "pdoc"), (ptf, torch.int32, "ptf"), (idf, torch.float64, "idf"),
                (qoff, torch.int64, "qoff"), (qterms, torch.int32, "qterms"))
    _need(toff.numel() == idf.numel() + 1 and pdoc.numel() == ptf.numel() and qoff.numel() == Q + 1,
          "tfidf_scores: toff must hold V + 1 offsets for idf's V terms, pdoc / ptf one entry per posting, qoff Q + 1 offsets")
    if slice_off is not None:
        _slice_table("tfidf_scores", slice_off, idf.numel(), N, "bm25")
    out = alloc_plane(Q, N, torch.float64, dev)
    out32 = alloc_plane(Q, N, torch.float32, dev) if want_f32 else None
    check(_lib.lib().fz_tfidf_scores_f64(_ptr(toff), _ptr(pdoc), _ptr(ptf), _ptr(idf), _ptr(slice_off), _ptr(qoff), _ptr(qterms), Q, N,
                                         _ptr(out), _ld(out), _ptr(out32), _ld(out32) if want_f32 else 0, _stream(idf)), "fz_tfidf_scores_f64")
    return (out, out32) if want_f32 else out


# ---------------------------------------------------------------------------------------
# BM25 / TF-IDF at corpus scale: range planes, the filter walk, the float64 stream
# ---------------------------------------------------------------------------------------
LEXICAL_MODES = {"pv": 0, "tfidf": 1}   # the walks csrc/bm25_stream.hip builds: the posting-value table (BM25, AtireBM25) and TF-IDF


def lexical_slice_docs(mode: str) -> int:
    """Documents one workgroup of the range / filter walks scores: 3,584 for 'pv', 7,168 for 'tfidf'; ranges start on a multiple of it."""
    _need(mode in LEXICAL_MODES, f"lexical_slice_docs: mode must be one of {sorted(LEXICAL_MODES)}")
    return int(_lib.lib().fz_lexical_slice_docs(LEXICAL_MODES[mode]))


def _lexical_args(what: str, mode: str, toff, pdoc, vals, idf, qoff, qterms, Q: int, N: int, doc_lo: int, doc_hi, slice_off):
    """The host-side contract the four lexical range entries share -> (doc_lo, doc_hi)."""
    _contiguous(what, (toff, torch.int64, "toff"), (pdoc, torch.int32, "pdoc"), (qoff, torch.int64, "qoff"), (qterms, torch.int32, "qterms"),
                (vals, torch.float64 if mode == "pv" else torch.int32, "pval" if mode == "pv" else "ptf"))
    V = toff.numel() - 1
    _need(V >= 0 and vals.numel() == pdoc.numel() > 0 and qoff.numel() == Q + 1 and qterms.numel() > 0,
          f"{what}: toff [V + 1], one value per posting (at least one), qoff [Q + 1] and a non-empty qterms expected")
    if mode == "tfidf":
        _need(_dev(idf, torch.float64, f"{what}(idf)").is_contiguous() and idf.numel() == V, f"{what}: idf must hold one value per term")
    if slice_off is not None:
        _slice_table(what, slice_off, V, N, "bm25")     # the table's slices are fz_bm25_slice_docs wide, the range's lexical_slice_docs(mode)
    return _doc_range(what, N, lexical_slice_docs(mode), doc_lo, doc_hi)


def _lexical_call(mode: str, stem: str, toff, pdoc, vals, idf, *rest) -> None:
    """The one place the two modes' twin C entries part: fz_bm25_<stem>_pv_f64(toff, pdoc, vals, *rest, stream) for 'pv',
    fz_tfidf_<stem>_f64(toff, pdoc, vals, idf, *rest, stream) for 'tfidf' -- the same argument list with idf after the posting values."""
    name = f"fz_bm25_{stem}_pv_f64" if mode == "pv" else f"fz_tfidf_{stem}_f64"
    values = (_ptr(vals),) if mode == "pv" else (_ptr(vals), _ptr(idf))
    check(getattr(_lib.lib(), name)(_ptr(toff), _ptr(pdoc), *values, *rest, _stream(toff)), name)


def lexical_weighted_terms(mode: str) -> int:
    """Query entries the weighted walks resolve per batch: 256 for 'pv', 128 for 'tfidf' (the batch groups the entries; no bit depends on it)."""
    _need(mode in LEXICAL_MODES, f"lexical_weighted_terms: mode must be one of {sorted(LEXICAL_MODES)}")
    return int(_lib.lib().fz_lexical_weighted_terms(LEXICAL_MODES[mode]))


def _lexical_weights(what: str, qterms, qw) -> torch.Tensor:
    """The weights of a weighted lexical query: float64, contiguous, one per entry of qterms, all finite (one host read)."""
    _need(_dev(qw, torch.float64, f"{what}(qw)").is_contiguous() and qw.dim() == 1, f"{what}(qw) must be a contiguous 1-d tensor")
    _need(qw.numel() == qterms.numel(), f"{what}(qw): {qw.numel()} weights for {qterms.numel()} entries of qterms")
    _need(bool(torch.isfinite(qw).all().item()), f"{what}(qw): every weight must be finite")
    return qw


def lexical_scores_range(mode: str, toff, pdoc, vals, idf, qoff, qterms, Q: int, N: int, doc_lo: int = 0, doc_hi: int | None = None,
                         slice_off: torch.Tensor | None = None, qw: torch.Tensor | None = None) -> torch.Tensor:
    """Columns [doc_lo, doc_hi) of the full float64 plane, bit for bit, without the rest of it (fz_bm25_scores_range_pv_f64 /
    fz_tfidf_scores_range_f64): [Q, doc_hi - doc_lo], column j = document doc_lo + j.  doc_lo a multiple of lexical_slice_docs(mode), doc_hi
    a multiple of it or N.  vals: pval ('pv') or ptf ('tfidf', with idf).  qw (float64, one weight per entry of qterms): the weighted walk
    (fz_bm25_scores_range_w_pv_f64 / fz_tfidf_scores_range_w_f64): entry j adds qw[j] * the unweighted walk's term, in entry order."""
    what = ("bm25" if mode == "pv" else "tfidf") + "_scores_range"      # the public wrappers' names: what a caller reads in an error
    doc_lo, doc_hi = _lexical_args(what, mode, toff, pdoc, vals, idf, qoff, qterms, Q, N, doc_lo, doc_hi, slice_off)
    if qw is not None:
        _lexical_weights(what, qterms, qw)
    out = alloc_plane(Q, doc_hi - doc_lo, torch.float64, toff.device)
    if qw is None:
        _lexical_call(mode, "scores_range", toff, pdoc, vals, idf, _ptr(slice_off), _ptr(qoff), _ptr(qterms), Q, N, doc_lo, doc_hi, _ptr(out), _ld(out))
    else:
        _lexical_call(mode, "scores_range_w", toff, pdoc, vals, idf, _ptr(slice_off), _ptr(qoff), _ptr(qterms), _ptr(qw), Q, N, doc_lo, doc_hi,
                      _ptr(out), _ld(out))
    return out


def bm25_scores_range(toff, pdoc, pval, qoff, qterms, Q: int, N: int, doc_lo: int = 0, doc_hi: int | None = None,
                      slice_off: torch.Tensor | None = None) -> torch.Tensor:
    """lexical_scores_range('pv'): columns [doc_lo, doc_hi) of bm25_scores(pval=...)'s float64 plane; slices of lexical_slice_docs('pv')."""
    return lexical_scores_range("pv", toff, pdoc, pval, None, qoff, qterms, Q, N, doc_lo, doc_hi, slice_off)


def tfidf_scores_range(toff, pdoc, ptf, idf, qoff, qterms, Q: int, N: int, doc_lo: int = 0, doc_hi: int | None = None,
                       slice_off: torch.Tensor | None = None) -> torch.Tensor:
    """lexical_scores_range('tfidf'): columns [doc_lo, doc_hi) of tfidf_scores' float64 plane; slices of lexical_slice_docs('tfidf')."""
    return lexical_scores_range("tfidf", toff, pdoc, ptf, idf, qoff, qterms, Q, N, doc_lo, doc_hi, slice_off)


def lexical_filter(mode: str, toff, pdoc, vals, idf, qoff, qterms, Q: int, N: int, doc_lo: int, doc_hi: int, id_base: int, tau, cand_s, cand_i,
                   cand_len, overflow, slice_off: torch.Tensor | None = None, qw: torch.Tensor | None = None) -> None:
    """The range walk with the threshold filter as its epilogue (fz_bm25_filter_pv_f64 / fz_tfidf_filter_f64): document d of [doc_lo, doc_hi)
    is appended to row q of cand_s / cand_i [Q, cap] as (float64 score, id_base + d) iff !(score <= tau[q]); cand_len [Q] int32 counts on
    past cap, nothing is stored there, `overflow` (int32 [1]) is set.  vals: pval ('pv') or ptf ('tfidf', with idf).  qw: the weighted walk
    (fz_bm25_filter_w_pv_f64 / fz_tfidf_filter_w_f64), as lexical_scores_range takes it."""
    what = "lexical_filter"
    doc_lo, doc_hi = _lexical_args(what, mode, toff, pdoc, vals, idf, qoff, qterms, Q, N, doc_lo, doc_hi, slice_off)
    cap = _cand_buffers(what, torch.float64, Q, tau, cand_s, cand_i, cand_len, overflow)
    if qw is None:
        _lexical_call(mode, "filter", toff, pdoc, vals, idf, _ptr(slice_off), _ptr(qoff), _ptr(qterms), Q, N, doc_lo, doc_hi, int(id_base), _ptr(tau),
                      _ptr(cand_s), _ptr(cand_i), _ptr(cand_len), cap, _ptr(overflow))
    else:
        _lexical_weights(what, qterms, qw)
        _lexical_call(mode, "filter_w", toff, pdoc, vals, idf, _ptr(slice_off), _ptr(qoff), _ptr(qterms), _ptr(qw), Q, N, doc_lo, doc_hi,
                      int(id_base), _ptr(tau), _ptr(cand_s), _ptr(cand_i), _ptr(cand_len), cap, _ptr(overflow))


def _query_blocks(Q: int, block: int):
    return ((lo, min(Q, lo + block)) for lo in range(0, Q, block))


def lexical_doc_scores(mode: str, toff, pdoc, vals, idf, qoff, qterms, Q: int, N: int, docs: torch.Tensor, block: int = 1024) -> torch.Tensor:
    """[Q, G] float64: the score the lexical walks give document docs[q, g] (int32 position in the index) for query q, with the bits of the
    full plane's entry (fz_bm25_doc_scores_pv_f64 / fz_tfidf_doc_scores_f64: a binary search per query term, the walk's chain of adds).
    A position < 0 (or >= N) gives -inf: not a document of this index.  Queries in blocks of `block`."""
    what = "lexical_doc_scores"
    _lexical_args(what, mode, toff, pdoc, vals, idf, qoff, qterms, Q, N, 0, None, None)
    _need(_dev(docs, torch.int32, f"{what}(docs)").is_contiguous() and docs.dim() == 2 and docs.shape[0] == Q and docs.shape[1] >= 1,
          f"{what}: docs must be a contiguous [Q, G >= 1] int32 tensor")
    G = docs.shape[1]
    out = torch.empty((Q, G), dtype=torch.float64, device=toff.device)
    for lo, hi in _query_blocks(Q, block):
        _lexical_call(mode, "doc_scores", toff, pdoc, vals, idf, _ptr(qoff[lo:]), _ptr(qterms), hi - lo, N, _ptr(docs[lo:]), G, _ptr(out[lo:]))
    return out


def lexical_doc_scores_fwd(mode: str, toff, pdoc, vals, idf, forward: "ForwardIndex", qoff, qterms, Q: int, N: int, docs: torch.Tensor,
                           block: int = 1024) -> torch.Tensor:
    """lexical_doc_scores through the index's forward index (fz_bm25_doc_scores_fwd_pv_f64 / fz_tfidf_doc_scores_fwd_f64): the same [Q, G]
    float64 scores bit for bit; the binary search per query term runs in the listed document's row of terms, and forward.fpos leads to
    the posting's value in `vals`.  Queries in blocks of `block`, as lexical_doc_scores takes them."""
    what = "lexical_doc_scores_fwd"
    if not isinstance(forward, ForwardIndex):
        raise TypeError(f"{what}(forward): expected an ops.ForwardIndex, got {type(forward).__name__}")
    _lexical_args(what, mode, toff, pdoc, vals, idf, qoff, qterms, Q, N, 0, None, None)
    _need(forward.N == N and forward.nnz == pdoc.numel(), f"{what}: the forward index must be the one built from these postings")
    _need(_dev(docs, torch.int32, f"{what}(docs)").is_contiguous() and docs.dim() == 2 and docs.shape[0] == Q and docs.shape[1] >= 1,
          f"{what}: docs must be a contiguous [Q, G >= 1] int32 tensor")
    G, f = docs.shape[1], forward
    out = torch.empty((Q, G), dtype=torch.float64, device=toff.device)
    for lo, hi in _query_blocks(Q, block):
        _lexical_call(mode, "doc_scores_fwd", toff, pdoc, vals, idf, _ptr(f.foff), _ptr(f.fterm), _ptr(f.fpos), _ptr(qoff[lo:]), _ptr(qterms), hi - lo,
                      N, _ptr(docs[lo:]), G, _ptr(out[lo:]))
    return out


def lexical_count(mode: str, toff, pdoc, vals, idf, qoff, qterms, Q: int, N: int, doc_lo: int, doc_hi, id_base: int, gold_scores, gold_ids,
                  counts: torch.Tensor, slice_off: torch.Tensor | None = None, block: int = 1024) -> None:
    """The range walk with the counting epilogue (fz_bm25_count_pv_f64 / fz_tfidf_count_f64): counts [Q, G] int32 += per (query, gold) the
    number of documents d of [doc_lo, doc_hi) that the stable float64 ranking puts before the gold (gold_scores [Q, G] float64, gold_ids
    [Q, G] int64 global ids, < 0: skipped): a better score, or the same and id_base + d < the gold's id.  Counts over disjoint ranges (and
    shards) add up to the rank.  vals: pval ('pv') or ptf ('tfidf', with idf).  Queries in blocks of `block` (grid y)."""
    what = "lexical_count"
    doc_lo, doc_hi = _lexical_args(what, mode, toff, pdoc, vals, idf, qoff, qterms, Q, N, doc_lo, doc_hi, slice_off)
    _dev(gold_scores, torch.float64, f"{what}(gold_scores)"); _dev(gold_ids, torch.int64, f"{what}(gold_ids)"); _dev(counts, torch.int32, f"{what}(counts)")
    G = gold_scores.shape[1] if gold_scores.dim() == 2 else 0
    _need(G >= 1 and all(t.is_contiguous() and tuple(t.shape) == (Q, G) for t in (gold_scores, gold_ids, counts)),
          f"{what}: gold_scores, gold_ids and counts must be contiguous [Q, G >= 1] tensors")
    for lo, hi in _query_blocks(Q, block):
        _lexical_call(mode, "count", toff, pdoc, vals, idf, _ptr(slice_off), _ptr(qoff[lo:]), _ptr(qterms), hi - lo, N, doc_lo, doc_hi, int(id_base),
                      _ptr(gold_scores[lo:]), _ptr(gold_ids[lo:]), G, _ptr(counts[lo:]))


def _lexical_source(model, qoff, qterms, id_base: int, qw: torch.Tensor | None = None) -> _Source:
    """The lexical posting walk whose epilogue is the filter (TopkStream64): document d of the model's index = id id_base + d.  model: a
    retrievers.bm25 TFIDF / BM25 / AtireBM25 whose lexical_mode() is 'pv' or 'tfidf' (lexical_tables(): the walk's per-posting values and idf).
    qw: the entries' float64 weights (the weighted walks); None: the unweighted ones."""
    mode = model.lexical_mode()
    _need(mode in LEXICAL_MODES, "_lexical_source: the model's scoring mode has no range walk (BM25.USE_POSTING_VALUES = False)")
    vals, idf = model.lexical_tables()
    Q, N, so = qoff.numel() - 1, model.corpus_size, model.slice_off

    def filter(st, lo, hi):
        lexical_filter(mode, model.toff, model.pdoc, vals, idf, qoff, qterms, Q, N, lo, hi, id_base, st.tau, st.cand_s, st.cand_i, st.cand_len,
                       st.overflow, slice_off=so, qw=qw)

    def plane(lo, hi):
        return lexical_scores_range(mode, model.toff, model.pdoc, vals, idf, qoff, qterms, Q, N, lo, hi, slice_off=so, qw=qw), id_base + lo
    return _Source(N, filter, plane, grain=lexical_slice_docs(mode), unordered=True, mark="shard_lexical_filter")


def _merge_ranked64(best_s, best_i, s, i, seq: torch.Tensor | None = None, seq_len: torch.Tensor | None = None):
    """The first k = best_s.shape[1] entries of the ranking (score desc, id asc) of [best | s]: ONE stable float64 row sort.  best: a ranked
    list whose ids are all below those of (s, i); (s, i): in the sequence `seq` ([rows, m] columns of s, the first seq_len[row] of them) or as
    they stand -- either way entries of equal score must come in ascending-id order, stability then gives the full ranking's tie rule.
    Returns the scores' own bits (gathered through the order, not the sort's canonicalised key plane)."""
    rows, k = best_s.shape
    m, dev = s.shape[1], best_s.device
    keys = as_plane(torch.cat([best_s, s], 1))
    ids = torch.cat([best_i, i], 1)
    init = row_len = None
    if seq is not None:
        init = torch.cat([torch.arange(k, dtype=torch.int32, device=dev).expand(rows, k), seq.to(torch.int32) + k], 1)
        row_len = (seq_len.to(torch.int32) + k).contiguous()
    order, _, _ = sort_rows_desc(keys, init_order=init, row_len=row_len, want_keys=False)
    top = order[:, :k].long()
    return torch.gather(keys, 1, top).contiguous(), torch.gather(ids, 1, top).contiguous()


class TopkStream64(TopkStream):
    """TopkStream for float64 lists, thresholds and candidate scores (BM25 / TF-IDF: the ranking is decided in float64).  The fold needs no
    sort kernel of its own: the running list holds only documents seen earlier -- every id in it is below every candidate's -- and is
    ordered (score desc, id asc); the window's candidates are put in ascending-id order (one argsort of the id slots, unwritten slots last)
    and the stable float64 row sort orders the row [best (k) | candidates (<= cap)] once: ties go to the ascending id, the rule of the full
    ranking.  An overflowed window is redone from its pieces' range planes (`top_positions(plane, k)`: the exact stable top-k of a plane,
    TFIDF._top_positions); without top_positions it cannot be."""

    dtype = torch.float64
    _fold_writes_tau = False     # the fold is torch ops and a row sort: the host rewrites tau and clears cand_len
    _fold_limits_k = False       # ... and has no limit of its own beyond _alloc's k + cap

    def __init__(self, run_scores: torch.Tensor, run_ids: torch.Tensor, seen: int, cap: int = 7168, exact_on_overflow: bool = True,
                 top_positions=None):
        self._ranking, self._can_redo = dict(top_positions=top_positions), top_positions is not None
        super().__init__(run_scores, run_ids, seen, cap, exact_on_overflow)

    def _alloc(self, dev):
        W = sort_max_n(torch.float64)
        _need(self.k + self.cap <= W, f"TopkStream64: k + cap = {self.k + self.cap} exceeds one float64 sort row ({W})")
        self.tau = torch.empty(self.rows, dtype=torch.float64, device=dev)
        self._slot = torch.arange(self.cap, dtype=torch.int32, device=dev)

    def _fold_candidates(self):
        n = torch.clamp(self.cand_len, max=self.cap)
        live = self._slot[None, :] < n[:, None]
        by_id = torch.argsort(torch.where(live, self.cand_i, torch.iinfo(torch.int64).max), dim=1)       # ascending ids, unwritten slots last
        return _merge_ranked64(self.best_s, self.best_i, torch.where(live, self.cand_s, float("-inf")), self.cand_i, seq=by_id, seq_len=n)

    @staticmethod
    def plane_topk(scores, k: int, base: int, top_positions):
        pos = top_positions(scores, min(k, scores.shape[1]))
        return torch.gather(scores, 1, pos), pos + base

    _merge = staticmethod(_merge_ranked64)      # the same [best | piece] stable sort

    def feed_lexical(self, model, qoff: torch.Tensor, qterms: torch.Tensor, doc_lo: int, doc_hi: int, id_base: int, mark=None):
        """Score documents [doc_lo, doc_hi) of a lexical model's index and keep what beats the thresholds, in one kernel per piece."""
        _need(qoff.numel() - 1 == self.rows, "TopkStream64.feed_lexical: one query per running list")
        self._feed(_lexical_source(model, qoff, qterms, int(id_base)), doc_lo, doc_hi, mark)


def topk_merge64(in_scores: torch.Tensor, in_ids: torch.Tensor):
    """[G, rows, k] per-shard float64 lists (each score desc, id asc; shard g's ids all below shard g + 1's; padding = (-inf, -1)) -> the
    global top-k [rows, k]: the shards side by side in rank order -- equal scores then stand in ascending-id order -- one stable float64 row
    sort, the first k.  The scores' own bits come back."""
    _dev(in_scores, torch.float64, "topk_merge64(in_scores)")
    _dev(in_ids, torch.int64, "topk_merge64(in_ids)")
    _need(in_scores.dim() == 3 and in_scores.shape == in_ids.shape, "topk_merge64: scores and ids must both be [G, rows, k]")
    G, rows, k = in_scores.shape
    if G * k > sort_max_n(torch.float64):
        raise ValueError(f"topk_merge64: {G} lists of {k} entries exceed one float64 sort row ({sort_max_n(torch.float64)} keys)")
    if G == 1 or rows == 0 or k == 0:
        return in_scores[0].contiguous(), in_ids[0].contiguous()
    keys = as_plane(in_scores.permute(1, 0, 2).reshape(rows, G * k))
    ids = in_ids.permute(1, 0, 2).reshape(rows, G * k)
    order, _, _ = sort_rows_desc(keys, want_keys=False)
    top = order[:, :k].long()
    return torch.gather(keys, 1, top).contiguous(), torch.gather(ids, 1, top).contiguous()


# ---------------------------------------------------------------------------------------
# A3, sparse form: SPLADE cosine scoring over an inverted index
# ---------------------------------------------------------------------------------------
PAIR_ROUTES = (None, "inverted", "forward")


def _pair_route(what: str, route, forward, why_not: str | None, prefer_forward: bool) -> bool:
    """The route rule of the pair scorers that have a forward index -> True for the forward route.  'forward' without a forward index (or
    with one the kernel does not take: why_not) raises; None takes the forward route only where `prefer_forward` says the measurement
    earned it ('Forward index') and nothing stands against it."""
    if route not in PAIR_ROUTES:
        raise ValueError(f"{what}(route): expected None, 'inverted' or 'forward', got {route!r}")
    if route == "forward":
        _need(forward is not None, f"{what}(route='forward'): the index has no forward index (build_forward())")
        _need(why_not is None, f"{what}(route='forward'): {why_not}")
        return True
    return route is None and prefer_forward and forward is not None and why_not is None


class ForwardIndex:
    """The document-major view of an inverted index: foff [N + 1] int64 row offsets, fterm [nnz] int32 the terms of document d in
    [foff[d], foff[d+1]) (ascending), fpos [nnz] int32 the place of each posting in the inverted arrays -- any per-posting table (pw, ptf,
    BM25's pval for the current (k1, b)) is reached through it."""

    def __init__(self, foff, fterm, fpos, N: int, V: int):
        self.foff, self.fterm, self.fpos, self.N, self.V = foff, fterm, fpos, int(N), int(V)

    @property
    def nnz(self) -> int:
        return int(self.fterm.numel())

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.foff, self.fterm, self.fpos))


def forward_index(toff: torch.Tensor, pdoc: torch.Tensor, N: int) -> ForwardIndex:
    """The forward index of the postings (toff [V + 1] int64, pdoc [nnz] int32, documents ascending inside a term): ONE stable sort of the
    postings by document -- they lie in ascending term order, so terms stay ascending inside a document; a posting's term comes from
    repeat_interleave over toff.  Documents without postings get empty rows."""
    if isinstance(pdoc, torch.Tensor) and pdoc.numel() >= 2 ** 31:      # (on the count alone, before the tensor is looked at)
        raise ValueError(f"forward_index: {pdoc.numel()} postings, but a posting's place is kept as an int32")
    _need(_dev(toff, torch.int64, "forward_index(toff)").is_contiguous() and toff.dim() == 1 and toff.numel() >= 1,
          "forward_index: toff must be a contiguous [V + 1] tensor")
    _need(_dev(pdoc, torch.int32, "forward_index(pdoc)").is_contiguous() and pdoc.dim() == 1, "forward_index: pdoc must be a contiguous [nnz] tensor")
    N, V, nnz = int(N), toff.numel() - 1, pdoc.numel()
    _need(N >= 0, "forward_index: N must not be negative")
    order = torch.sort(pdoc, stable=True).indices
    term = torch.repeat_interleave(torch.arange(V, dtype=torch.int32, device=pdoc.device), toff[1:] - toff[:-1])
    _need(term.numel() == nnz, "forward_index: toff does not describe pdoc's postings")
    counts = torch.bincount(pdoc, minlength=N)
    _need(counts.numel() == N, f"forward_index: pdoc holds a document beyond N = {N}")
    foff = torch.zeros(N + 1, dtype=torch.int64, device=pdoc.device)
    foff[1:] = torch.cumsum(counts, 0)
    return ForwardIndex(foff, term[order].contiguous(), order.int(), N, V)


class SparseForward:
    """A SparseIndex's forward index in the form fz_sparse_fwd_pairs_f32 reads: foff [N + 1] int64 and rows [nnz, 2] int32, row-contiguous
    8-byte postings {term, the bits of the float32 weight} (fpos is not kept: 8 bytes per posting in all)."""

    def __init__(self, foff, rows, N: int, V: int):
        self.foff, self.rows, self.N, self.V = foff, rows, int(N), int(V)

    @property
    def nbytes(self) -> int:
        return self.foff.numel() * 8 + self.rows.numel() * 4

    def terms(self) -> torch.Tensor:
        return self.rows[:, 0]

    def weights(self) -> torch.Tensor:
        return self.rows[:, 1].view(torch.float32)


def sparse_fwd_max_vocab() -> int:
    """The largest vocabulary whose query bitmap fz_sparse_fwd_pairs_f32 holds in LDS."""
    return int(_lib.lib().fz_sparse_fwd_max_vocab())


# route=None of sparse_dot_pairs takes the forward route where an index has one.  The forward index doubles the index's memory, so the
# condition was at most half the inverted route's time at Q = 1024, W = 3,000 on the 1.1 M-passage shard: 0.93 ms against 11.16 ms in
# one run (profiles/r21_forward_pairs.json; DESIGN.md, 'Forward index')
SPARSE_PAIRS_PREFER_FORWARD = True


class SparseIndex:
    """L2-normalised corpus vectors as postings: toff [V + 1] int64, pdoc [nnz] int32 (ascending inside a term), pw [nnz] float32,
    slice_off [V, NS + 1] int64 (fz_sparse_slice_offsets).  N documents over a vocabulary of V terms.  forward: None, or the
    SparseForward build_forward() made."""

    forward = None

    def build_forward(self) -> SparseForward:
        """Build and keep the document-major rows sparse_dot_pairs' forward route reads (8 bytes per posting: the index's size again)."""
        f = forward_index(self.toff, self.pdoc, self.N)
        rows = torch.empty((f.nnz, 2), dtype=torch.int32, device=self.pw.device)
        rows[:, 0] = f.fterm
        rows[:, 1] = self.pw[f.fpos.long()].view(torch.int32)
        self.forward = SparseForward(f.foff, rows, self.N, self.V)
        return self.forward

    def __init__(self, toff, pdoc, pw, N: int, V: int, slice_off=None):
        self.toff, self.pdoc, self.pw, self.N, self.V = toff, pdoc, pw, int(N), int(V)
        self.slice_off = slice_off if slice_off is not None else sparse_slice_offsets(toff, pdoc, self.V, self.N)

    @property
    def nnz(self) -> int:
        return int(self.pdoc.numel())

    def tensors(self):
        return self.toff, self.pdoc, self.pw

    def dense_cached(self) -> torch.Tensor:
        """to_dense(), padded for the GEMM, built once and kept WHILE the index's buffers are the ones it was built from (a rebuilt or
        re-pointed index re-densifies); drop_dense() gives the N x V float32 matrix (3.6 GB at LLeQA size) back."""
        key = (self.toff.data_ptr(), self.pdoc.data_ptr(), self.pw.data_ptr(), self.nnz, self.N, self.V)
        if getattr(self, "_dense_key", None) != key:
            self._dense, self._dense_key = pad_dim(self.to_dense()), key
        return self._dense

    def drop_dense(self) -> None:
        self._dense, self._dense_key = None, None

    def to_dense(self) -> torch.Tensor:
        """The [N, V rounded up to 4] float32 matrix the index was built from (normalised rows)."""
        D = torch.zeros((self.N, round_up(max(self.V, 1), 4)), dtype=torch.float32, device=self.pw.device)
        term = torch.repeat_interleave(torch.arange(self.V, device=self.pw.device), self.toff[1:] - self.toff[:-1])
        D[self.pdoc.long(), term] = self.pw
        return D


def sparse_slice_offsets(toff: torch.Tensor, pdoc: torch.Tensor, V: int, N: int) -> torch.Tensor:
    return _slice_offsets("sparse", toff, pdoc, V, N)


def density(X: torch.Tensor) -> float:
    """Fraction of non-zero entries (one device reduction)."""
    return float(torch.count_nonzero(X).item()) / max(1, X.numel())


def sparse_index_from_blocks(blocks, V: int, N: int | None = None, device=None) -> SparseIndex:
    """Inverted index of a corpus given as row blocks -- an iterable of (doc_base, rows [n, >= V] float32) in ascending document order --
    without the corpus ever being one dense matrix: every block contributes its non-zeros (document, term, weight), then ONE stable sort by
    term puts them in term order, documents staying ascending inside a term; documents no block covers have no postings.  Memory while it
    sorts: 12 bytes per posting for the postings and as much again for the sort's output.  N: documents in all (default: the end of the last
    block)."""
    docs, terms, vals = [], [], []
    end = 0
    for r0, blk in blocks:
        _dev(blk, torch.float32, "sparse_index_from_blocks(rows)")
        _need(int(r0) >= end, "sparse_index_from_blocks: blocks must come in ascending document order")
        device = blk.device
        blk = blk[:, :V]
        nz = blk.nonzero()
        docs.append((nz[:, 0] + int(r0)).int()); terms.append(nz[:, 1].int()); vals.append(blk[nz[:, 0], nz[:, 1]])
        end = int(r0) + blk.shape[0]
    N = end if N is None else int(N)
    _need(N >= end, f"sparse_index_from_blocks: the blocks reach document {end}, beyond N = {N}")
    device = device if device is not None else "cuda"
    doc = torch.cat(docs) if docs else torch.zeros(0, dtype=torch.int32, device=device)
    term = torch.cat(terms) if terms else torch.zeros(0, dtype=torch.int32, device=device)
    val = torch.cat(vals) if vals else torch.zeros(0, dtype=torch.float32, device=device)
    del docs, terms, vals
    order = torch.sort(term, stable=True).indices           # documents were appended ascending: stable keeps them so inside a term
    toff = torch.zeros(V + 1, dtype=torch.int64, device=device)
    toff[1:] = torch.cumsum(torch.bincount(term, minlength=V), 0)
    del term
    return SparseIndex(toff, doc[order].contiguous(), val[order].contiguous(), N, V)


def sparse_index(Dn: torch.Tensor, V: int | None = None, rows: int = 4096) -> SparseIndex:
    """Inverted index of the rows of Dn [N, >= V] (already L2-normalised, e.g. ops.normalize_rows): sparse_index_from_blocks over row blocks
    of Dn."""
    _dev(Dn, torch.float32, "sparse_index(Dn)")
    N = Dn.shape[0]
    V = Dn.shape[1] if V is None else int(V)
    return sparse_index_from_blocks(((r0, Dn[r0: r0 + rows]) for r0 in range(0, N, rows)), V, N=N, device=Dn.device)


def sparse_rows(Qn: torch.Tensor, V: int | None = None):
    """The non-zero (term, weight) lists of the rows of Qn [Q, >= V]: (qoff [Q + 1] int64, qterms int32, qw float32), terms ascending."""
    _dev(Qn, torch.float32, "sparse_rows(Qn)")
    V = Qn.shape[1] if V is None else int(V)
    blk = Qn[:, :V]
    nz = blk.nonzero()                                        # row-major: by query, then ascending term
    qoff = torch.zeros(Qn.shape[0] + 1, dtype=torch.int64, device=Qn.device)
    qoff[1:] = torch.cumsum(torch.bincount(nz[:, 0], minlength=Qn.shape[0]), 0)
    return qoff, nz[:, 1].int().contiguous(), blk[nz[:, 0], nz[:, 1]].contiguous()


def _sparse_queries(qoff, qterms, qw, what):
    for t, dt, name in ((qoff, torch.int64, "qoff"), (qterms, torch.int32, "qterms"), (qw, torch.float32, "qw")):
        _need(_dev(t, dt, f"{what}({name})").is_contiguous(), f"{what}({name}) must be contiguous")
    Q = qoff.numel() - 1
    _need(Q >= 0 and qterms.numel() == qw.numel(), f"{what}: qoff must hold Q + 1 offsets, qterms and qw one entry per non-zero")
    return Q


def sparse_slice_docs() -> int:
    """Documents per workgroup slice of the sparse kernels: document ranges start on a multiple of it."""
    return int(_lib.lib().fz_sparse_slice_docs())


def sparse_dot(index: SparseIndex, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, out: torch.Tensor | None = None,
               doc_lo: int = 0, doc_hi: int | None = None) -> torch.Tensor:
    """scores[q][j] = sum over query q's terms of qw * (document doc_lo + j's weight of that term): [Q, doc_hi - doc_lo] float32 plane
    (default: all N documents).  doc_lo a multiple of sparse_slice_docs(), doc_hi one too or N; a range's columns are the full plane's, bit
    for bit."""
    Q = _sparse_queries(qoff, qterms, qw, "sparse_dot")
    doc_lo, doc_hi = _doc_range("sparse_dot", index.N, sparse_slice_docs(), doc_lo, doc_hi)
    out = _out("sparse_dot", out, (Q, doc_hi - doc_lo), torch.float32, qoff.device, plane=True)
    check(_lib.lib().fz_sparse_dot_range_f32(_ptr(index.toff), _ptr(index.pdoc), _ptr(index.pw), _ptr(index.slice_off), _ptr(qoff), _ptr(qterms),
                                             _ptr(qw), Q, index.N, doc_lo, doc_hi, _ptr(out), _ld(out), _stream(qoff)), "fz_sparse_dot_range_f32")
    return out


def sparse_dot_pairs(index: SparseIndex, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, cand: torch.Tensor,
                     cand_len: torch.Tensor | None = None, *, id_base: int = 0, out: torch.Tensor | None = None, route: str | None = None) -> torch.Tensor:
    """Sparse scores of every query against its own candidates (fz_sparse_dot_pairs_f32): out[q, r] = sparse_dot(index, qoff, qterms,
    qw)[q, cand[q, r] - id_base], bit for bit, with no [Q, N] plane (a binary search per query term and candidate).  The queries as
    sparse_rows gives them (terms ascending); cand, cand_len, id_base, out and the -inf rules as in dot_pairs; a document of the index
    that shares no term with the query scores +0.0.

    route: 'inverted' -- the binary searches in the posting lists; 'forward' -- one walk along the candidate's row of index.forward
    (fz_sparse_fwd_pairs_f32; the same bits), a ValueError without a forward index or with V beyond sparse_fwd_max_vocab(); None --
    the forward route where the index has a forward index the kernel takes (SPARSE_PAIRS_PREFER_FORWARD: it measured 12 times faster),
    the inverted route otherwise: an index without a forward index is scored as before."""
    if route not in PAIR_ROUTES:
        raise ValueError(f"sparse_dot_pairs(route): expected None, 'inverted' or 'forward', got {route!r}")
    if not isinstance(index, SparseIndex):
        raise TypeError(f"sparse_dot_pairs(index): expected an ops.SparseIndex, got {type(index).__name__}")
    fwd, why_not = index.forward, None
    if fwd is not None and index.V > sparse_fwd_max_vocab():
        why_not = f"V = {index.V} is beyond the kernel's bitmap ({sparse_fwd_max_vocab()} terms)"
    forward = _pair_route("sparse_dot_pairs", route, fwd, why_not, SPARSE_PAIRS_PREFER_FORWARD)
    Q = _sparse_queries(qoff, qterms, qw, "sparse_dot_pairs")
    cand_len, out, W = _pairs_args("sparse_dot_pairs", Q, qoff.device, cand, cand_len, out)
    if forward:
        check(_lib.lib().fz_sparse_fwd_pairs_f32(_ptr(fwd.foff), _ptr(fwd.rows), index.V, _ptr(qoff), _ptr(qterms), _ptr(qw), Q, index.N, _ptr(cand),
                                                 _ld(cand), _ptr(cand_len), W, int(id_base), _ptr(out), _ld(out), _stream(qoff)),
              "fz_sparse_fwd_pairs_f32")
        return out
    check(_lib.lib().fz_sparse_dot_pairs_f32(_ptr(index.toff), _ptr(index.pdoc), _ptr(index.pw), _ptr(qoff), _ptr(qterms), _ptr(qw), Q, index.N,
                                             _ptr(cand), _ld(cand), _ptr(cand_len), W, int(id_base), _ptr(out), _ld(out), _stream(qoff)),
          "fz_sparse_dot_pairs_f32")
    return out


# ---------------------------------------------------------------------------------------
# pseudo-relevance feedback (csrc/feedback.hip)
# ---------------------------------------------------------------------------------------
def sparse_feedback_max_vocab() -> int:
    """The largest vocabulary whose accumulator fz_sparse_feedback_f32 holds in LDS."""
    return int(_lib.lib().fz_sparse_feedback_max_vocab())


def _feedback_args(what: str, Q: int, fb_ids, fb_len, coef):
    """The feedback lists of both kernels: fb_ids [Q, F] int64 and coef [Q, F] float32 (rows may be strided), fb_len [Q] int32 or None."""
    _dev(fb_ids, torch.int64, f"{what}(fb_ids)")
    _dev(coef, torch.float32, f"{what}(coef)")
    _need(fb_ids.dim() == 2 and fb_ids.shape[0] == Q, f"{what}: fb_ids must be [Q = {Q}, F], got {tuple(fb_ids.shape)}")
    _need(tuple(coef.shape) == tuple(fb_ids.shape), f"{what}(coef): fb_ids are {tuple(fb_ids.shape)} but coef {tuple(coef.shape)}")
    if fb_len is not None:
        _dev(fb_len, torch.int32, f"{what}(fb_len)")
        _need(tuple(fb_len.shape) == (Q,), f"{what}(fb_len): expected shape {(Q,)}, got {tuple(fb_len.shape)}")
        fb_len = fb_len.contiguous()
    return fb_len, int(fb_ids.shape[1])


def sparse_feedback(forward: SparseForward, V: int, qoff: torch.Tensor, qterms: torch.Tensor, qw: torch.Tensor, fb_ids: torch.Tensor,
                    fb_len: torch.Tensor | None, coef: torch.Tensor, alpha: float, m: int, *, id_base: int = 0, normalize: bool = False):
    """Rocchio expansion of weighted sparse queries from feedback documents (fz_sparse_feedback_f32): q' = alpha * q + sum_r coef[q, r] *
    d_r over the slots r < fb_len[q] whose id is one of the forward index's documents (id_base ..), in slot order; of the terms the
    documents bring in, the m with the largest sums are kept (ties: the lower term), the query's own terms always.  One rounding per
    product and per add: the bits are defined (include/fusion_hip.h states the arithmetic).  The queries as sparse_rows gives them,
    forward a SparseForward over V terms, fb_ids [Q, F] int64, fb_len [Q] int32 or None, coef [Q, F] float32.
    -> (qoff', qterms', qw') in the same form; normalize=True: qw' L2-normalised per query (normalize_rows over the padded rows).
    One host read for the row width (the longest query + m, at most V) and one of the kernel's flag word; ValueError for V beyond
    sparse_feedback_max_vocab()."""
    if not isinstance(forward, SparseForward):
        raise TypeError(f"sparse_feedback(forward): expected an ops.SparseForward, got {type(forward).__name__}")
    Q = _sparse_queries(qoff, qterms, qw, "sparse_feedback")
    fb_len, F = _feedback_args("sparse_feedback", Q, fb_ids, fb_len, coef)
    V, m = int(V), int(m)
    _need(m >= 0, f"sparse_feedback: m = {m} must not be negative")
    _need(1 <= V <= sparse_feedback_max_vocab(),
          f"sparse_feedback: V = {V} is outside 1 .. {sparse_feedback_max_vocab()}, the accumulator the kernel holds (sparse_feedback_max_vocab)")
    _need(forward.V <= V, f"sparse_feedback: the forward index is over {forward.V} terms, more than V = {V}")
    _dev(forward.foff, torch.int64, "sparse_feedback(forward.foff)")
    _dev(forward.rows, torch.int32, "sparse_feedback(forward.rows)")
    _need(forward.foff.is_contiguous() and forward.foff.numel() == forward.N + 1 and forward.rows.is_contiguous(),
          "sparse_feedback: forward.foff must be a contiguous [N + 1] tensor and forward.rows contiguous")
    dev = qoff.device
    nq_max = int((qoff[1:] - qoff[:-1]).max().item()) if Q > 0 else 0      # the one host read of the plan
    width = min(nq_max + m, V)                                             # (a row holds at most V terms)
    out_terms = alloc_plane(Q, width, torch.int32, dev)
    out_w = alloc_plane(Q, width, torch.float32, dev)
    out_len = torch.zeros(Q, dtype=torch.int32, device=dev)
    if Q > 0:
        flag = torch.empty(4, dtype=torch.uint8, device=dev)
        check(_lib.lib().fz_sparse_feedback_f32(_ptr(forward.foff), _ptr(forward.rows), V, forward.N, int(id_base), _ptr(qoff), _ptr(qterms),
                                                _ptr(qw), Q, _ptr(fb_ids), max(_ld(fb_ids), F), _ptr(fb_len), _ptr(coef), max(_ld(coef), F),
                                                F, float(alpha), m, _ptr(out_terms), _ptr(out_w), _same_ld(out_terms, out_w), width,
                                                _ptr(out_len), _ptr(flag), _stream(qoff)), "fz_sparse_feedback_f32")
        if _flag_word(flag) & 1:
            raise ValueError(f"sparse_feedback: an expanded query does not fit {width} terms (query terms out of order or repeated?)")
    if normalize and Q > 0 and width > 0:
        out_w = normalize_rows(out_w)[:, :width]                           # the padding is +0.0: the norm of the expanded query
    kept = out_terms >= 0
    noff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    noff[1:] = torch.cumsum(out_len, 0)
    return noff, out_terms[kept].contiguous(), out_w[kept].contiguous()


def lexical_feedback_max_entries() -> int:
    """The sum of the counted feedback rows' lengths, per query, that the lexical feedback kernels hold (4,096)."""
    return int(_lib.lib().fz_lexical_feedback_max_entries())


LEXICAL_FEEDBACK_CUT = 1     # bit 0 of the flags lexical_feedback returns: the capacity rule skipped slots of some query


def _lexical_feedback_run(what: str, entry: str, rows: tuple, foff, N: int, qoff, qterms, fb_ids, fb_len, coef, alpha: float, beta: float, m: int,
                          id_base: int):
    """What the three lexical feedback entries share: the checks on queries and slots, the output rows, the call, and the expanded
    queries as a CSR -> (qoff', qterms', qw', flags)."""
    _contiguous(what, (qoff, torch.int64, "qoff"), (qterms, torch.int32, "qterms"), (foff, torch.int64, "foff"))
    Q, m, N = qoff.numel() - 1, int(m), int(N)
    _need(Q >= 0 and qoff.dim() == 1 and qterms.dim() == 1, f"{what}: qoff must hold Q + 1 offsets, qterms the queries' entries")
    _need(m >= 0, f"{what}: fb_terms = {m} must not be negative")
    _need(N >= 0 and foff.numel() == N + 1, f"{what}: foff must hold N + 1 = {N + 1} row offsets, got {foff.numel()}")
    _need(math.isfinite(alpha) and math.isfinite(beta), f"{what}: alpha and beta must be finite")
    fb_len, F = _feedback_args(what, Q, fb_ids, fb_len, coef)
    dev = qoff.device
    lens = qoff[1:] - qoff[:-1]
    nq_max = int(lens.max().item()) if Q > 0 else 0                        # the one host read of the plan
    _need(Q == 0 or int(qoff[-1].item()) <= qterms.numel(), f"{what}: qoff runs past qterms")
    width = nq_max + m
    out_terms = alloc_plane(Q, width, torch.int32, dev)
    out_w = alloc_plane(Q, width, torch.float64, dev)
    ldo = max(_ld(out_terms), width)
    if Q > 1:
        _need(_ld(out_w) == ldo, f"{what}: the output planes differ in row stride")
    out_len = torch.zeros(Q, dtype=torch.int32, device=dev)
    flags = 0
    if Q > 0:
        flag = torch.empty(4, dtype=torch.uint8, device=dev)
        check(getattr(_lib.lib(), entry)(_ptr(foff), *rows, N, int(id_base), _ptr(qoff), _ptr(qterms), Q, _ptr(fb_ids), max(_ld(fb_ids), F),
                                         _ptr(fb_len), _ptr(coef), max(_ld(coef), F), F, float(alpha), float(beta), m, _ptr(out_terms),
                                         _ptr(out_w), ldo, width, _ptr(out_len), _ptr(flag), _stream(qoff)), entry)
        flags = _flag_word(flag)
        if flags & 2:
            raise RuntimeError(f"{what}: an expanded query did not fit its row of {width} entries")
    kept = torch.arange(width, device=dev)[None, :] < out_len[:, None]
    noff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    noff[1:] = torch.cumsum(out_len, 0)
    nterms, nw = out_terms[kept].contiguous(), out_w[kept].contiguous()
    if nterms.numel() == 0:                                                # (the walks take a non-empty qterms: TFIDF._query_csr's padding)
        nterms, nw = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    return noff, nterms, nw, flags


def lexical_feedback(mode: str, forward: "ForwardIndex", vals, idf, qoff, qterms, fb_ids, fb_len, coef, alpha: float, beta: float, m: int, *,
                     id_base: int = 0):
    """Expansion terms for lexical queries from their feedback documents (fz_bm25_feedback_pv_f64 / fz_tfidf_feedback_f64; the arithmetic:
    include/fusion_hip.h and DESIGN.md, 'Lexical feedback').  forward: the index's ops.ForwardIndex (fpos kept); vals: pval ('pv') or ptf
    ('tfidf', with idf); the queries as TFIDF._query_csr gives them (repetitions and -1 kept); fb_ids [Q, F] int64, fb_len [Q] int32 or
    None, coef [Q, F] float32 (feedback.coefficients).  w[t] = sum in slot order of coef * val(t, d); of the terms with w > 0 that are not
    the query's the m of largest w (ties: the lower term) follow the query's own entries:
    -> (qoff', qterms', qw' float64, flags): the original entries at alpha, then the selected terms at beta * (w / w_max); flags & 1
    (LEXICAL_FEEDBACK_CUT): some query's rows passed lexical_feedback_max_entries() and its later slots were skipped."""
    what = "lexical_feedback"
    _need(mode in LEXICAL_MODES, f"{what}: mode must be one of {sorted(LEXICAL_MODES)}")
    if not isinstance(forward, ForwardIndex):
        raise TypeError(f"{what}(forward): expected an ops.ForwardIndex, got {type(forward).__name__}")
    _contiguous(what, (forward.fterm, torch.int32, "forward.fterm"), (forward.fpos, torch.int32, "forward.fpos"),
                (vals, torch.float64 if mode == "pv" else torch.int32, "pval" if mode == "pv" else "ptf"))
    _need(forward.fpos.numel() == forward.nnz == vals.numel(), f"{what}: the forward index must be the one built from these postings")
    if mode == "tfidf":
        _need(_dev(idf, torch.float64, f"{what}(idf)").is_contiguous() and idf.numel() >= forward.V, f"{what}: idf must hold one value per term")
    rows = (_ptr(forward.fterm), _ptr(forward.fpos), _ptr(vals)) + ((_ptr(idf),) if mode == "tfidf" else ())
    entry = "fz_bm25_feedback_pv_f64" if mode == "pv" else "fz_tfidf_feedback_f64"
    return _lexical_feedback_run(what, entry, rows, forward.foff, forward.N, qoff, qterms, fb_ids, fb_len, coef, alpha, beta, m, id_base)


def lexical_feedback_rows(foff, fterm, fval, qoff, qterms, fb_ids, fb_len, coef, alpha: float, beta: float, m: int, *, id_base: int = 0):
    """lexical_feedback over rows given directly (fz_lexical_feedback_rows_f64): row d = entries [foff[d], foff[d+1]) of (fterm int32,
    fval float64 = val(t, d)), terms unique inside a row; the term space is the caller's (the sharded route: global term ids)."""
    what = "lexical_feedback_rows"
    _contiguous(what, (fterm, torch.int32, "fterm"), (fval, torch.float64, "fval"), (foff, torch.int64, "foff"))
    _need(fterm.numel() == fval.numel() and foff.numel() >= 1, f"{what}: one value per row entry and N + 1 row offsets expected")
    return _lexical_feedback_run(what, "fz_lexical_feedback_rows_f64", (_ptr(fterm), _ptr(fval)), foff, foff.numel() - 1, qoff, qterms, fb_ids,
                                 fb_len, coef, alpha, beta, m, id_base)


def dense_feedback(Qn: torch.Tensor, Dn: torch.Tensor, fb_ids: torch.Tensor, fb_len: torch.Tensor | None, coef: torch.Tensor, alpha: float, *,
                   id_base: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """Rocchio for dense queries (fz_dense_feedback_f32): out[q] = alpha * Qn[q], then + coef[q, r] * Dn[fb_ids[q, r] - id_base] slot
    after slot with sparse_feedback's slot rules, one rounding per product and per add.  Qn [Q, dim], Dn [N, dim] float32 (any row
    stride), fb_ids [Q, F] int64, fb_len [Q] int32 or None, coef [Q, F] float32 -> [Q, dim] float32, not normalised (normalize_rows)."""
    _dev(Qn, torch.float32, "dense_feedback(Qn)")
    _dev(Dn, torch.float32, "dense_feedback(Dn)")
    _need(Qn.dim() == 2 and Dn.dim() == 2, "dense_feedback: Qn [Q, dim] and Dn [N, dim] expected")
    if Qn.shape[1] != Dn.shape[1]:
        raise ValueError(f"embedding dims differ: {Qn.shape[1]} vs {Dn.shape[1]}")
    Q, N, dim = int(Qn.shape[0]), int(Dn.shape[0]), int(Qn.shape[1])
    _need(dim >= 1, "dense_feedback: dim must be at least 1")
    fb_len, F = _feedback_args("dense_feedback", Q, fb_ids, fb_len, coef)
    out = _out("dense_feedback", out, (Q, dim), torch.float32, Qn.device, plane=True)
    check(_lib.lib().fz_dense_feedback_f32(_ptr(Qn), max(_ld(Qn), dim), _ptr(Dn), max(_ld(Dn), dim), Q, N, dim, int(id_base), _ptr(fb_ids),
                                           max(_ld(fb_ids), F), _ptr(fb_len), _ptr(coef), max(_ld(coef), F), F, float(alpha), _ptr(out),
                                           max(_ld(out), dim), _stream(Qn)), "fz_dense_feedback_f32")
    return out


def sparse_cos_scores(Qe: torch.Tensor, index: SparseIndex, max_query_density: float = 0.05) -> torch.Tensor:
    """Cosine scores of dense query vectors Qe [Q, >= V] against a SparseIndex (whose rows were normalised before indexing).  Queries that are
    not sparse themselves (an untrained head activates half the vocabulary: one barrier per term and query) take the dense GEMM against the
    re-densified corpus instead -- same scores either way."""
    Qn = normalize_rows(pad_dim(Qe))
    if density(Qn[:, :index.V]) > max_query_density:
        # re-densified ONCE per index and kept (N x V float32: 3.6 GB at LLeQA size -- a fresh allocation + scatter per query batch would
        # cost more than the GEMM it feeds); a query encoder that is not sparse stays on this path for every batch
        return dot_scores(Qn, index.dense_cached())
    return sparse_dot(index, *sparse_rows(Qn, index.V))


# ---------------------------------------------------------------------------------------
# K2 at corpus scale, first stage: candidates from token centroids (csrc/centroid.hip)
# ---------------------------------------------------------------------------------------
CENTROID_BLOCK_BYTES = 256 << 20            # what centroid_assign / centroid_probes / kmeans_centroids allocate per block of rows stays below this:
#                                             the float32 score block of the two-kernel route, the float32 rows + list workspace of the fused one
CENTROID_FUSED = True                       # fused=None: dot_topn (selection in the GEMM's epilogue) wherever n <= dot_topn_max(); False: dot_scores + topk_rows
CENTROID_SLICE_TABLE_MAX_BYTES = 1 << 30    # centroid_index builds the [K, NS + 1] slice table only below this size (as retrievers.bm25 does)


class CentroidIndex:
    """Per centroid the DISTINCT local documents that carry it, ascending: coff [K + 1] int64, cdoc int32 -- the shape of SparseIndex
    without weights.  slice_off [K, NS + 1] int64 (fz_centroid_slice_offsets) or None: without it the kernels find their list segments by
    binary search, with the same result."""

    def __init__(self, coff, cdoc, N: int, K: int, slice_off=None):
        self.coff, self.cdoc, self.N, self.K, self.slice_off = coff, cdoc, int(N), int(K), slice_off


def centroid_slice_docs() -> int:
    """Documents per workgroup slice of the centroid kernels: document ranges start on a multiple of it."""
    return int(_lib.lib().fz_centroid_slice_docs())


def _f32_rows(X: torch.Tensor, what: str) -> torch.Tensor:
    _need(isinstance(X, torch.Tensor) and X.dim() == 2 and X.dtype in (torch.float16, torch.float32), f"{what}: a [rows, dim] float16 or float32 tensor expected")
    return X.float().contiguous()


def _centroid_fused(fused, n: int, what: str) -> bool:
    """The route of one call: fused=True demands dot_topn, False the two kernels, None follows CENTROID_FUSED where dot_topn takes n."""
    if fused is None:
        return bool(CENTROID_FUSED) and n <= dot_topn_max()
    if fused:
        _need(n <= dot_topn_max(), f"{what}: fused=True takes at most {dot_topn_max()} entries per row (dot_topn_max), got {n}")
    return bool(fused)


def _topn_block_rows(dim: int, n: int) -> int:
    """Rows per block of the fused route: their float32 copy and dot_topn's workspace (4 lists of n (score, id) pairs per row; below 65,536
    rows it has a floor of that many rows' worth) within CENTROID_BLOCK_BYTES."""
    return max(1, CENTROID_BLOCK_BYTES // (4 * round_up(dim, 4) + 32 * n))


def _nearest(X32: torch.Tensor, C32: torch.Tensor, fused=None) -> torch.Tensor:
    """Row-wise argmax of X32 @ C32.T, ties to the lowest id, in blocks of CENTROID_BLOCK_BYTES: dot_topn(.., 1), or dot_scores + topk_rows(1)."""
    n, K = X32.shape[0], C32.shape[0]
    out = torch.empty(n, dtype=torch.int32, device=X32.device)
    if _centroid_fused(fused, 1, "kmeans_centroids"):
        rows = _topn_block_rows(X32.shape[1], 1)
        for r0 in range(0, n, rows):
            out[r0: r0 + rows] = dot_topn(X32[r0: r0 + rows], C32, 1)[1][:, 0]
        return out
    rows = max(1, CENTROID_BLOCK_BYTES // (4 * round_up(max(K, 1), _PAD)))
    for r0 in range(0, n, rows):
        _, ids = topk_rows(dot_scores(X32[r0: r0 + rows], C32), 1)
        out[r0: r0 + rows] = ids[:, 0]
    return out


def centroid_assign(Dtok: torch.Tensor, C: torch.Tensor, fused=None) -> torch.Tensor:
    """codes [sumL] int32: for every token row of Dtok [sumL, dim] the centroid of C [K, dim] with the largest dot product, ties to the
    lowest id.  Chunked over token rows by a byte budget; the float32 MFMA GEMM on the float32 copies with the selection in its epilogue
    (dot_topn(.., 1); fused: see centroid_probes) or dot_scores, then topk_rows(.., 1) -- the same codes either way: bit-reproducible."""
    _dev(Dtok, None, "centroid_assign(Dtok)"); _dev(C, None, "centroid_assign(C)")
    _need(Dtok.dim() == 2 and C.dim() == 2 and C.shape[0] >= 1 and Dtok.shape[1] == C.shape[1], "centroid_assign: Dtok [sumL, dim] and C [K >= 1, dim] expected")
    _need(Dtok.dtype in (torch.float16, torch.float32), "centroid_assign(Dtok): float16 or float32 expected")
    C32 = _f32_rows(C, "centroid_assign(C)")
    n = Dtok.shape[0]
    out = torch.empty(n, dtype=torch.int32, device=Dtok.device)
    if _centroid_fused(fused, 1, "centroid_assign"):
        rows = _topn_block_rows(Dtok.shape[1], 1)
        for r0 in range(0, n, rows):
            out[r0: r0 + rows] = dot_topn(Dtok[r0: r0 + rows].float().contiguous(), C32, 1)[1][:, 0]
        return out
    rows = max(1, CENTROID_BLOCK_BYTES // (4 * round_up(C.shape[0], _PAD)))
    for r0 in range(0, n, rows):     # the float32 copy of one block of token rows at a time
        _, ids = topk_rows(dot_scores(Dtok[r0: r0 + rows].float().contiguous(), C32), 1)
        out[r0: r0 + rows] = ids[:, 0]
    return out


def kmeans_centroids(tokens: torch.Tensor, K: int, iters: int = 4, seed: int = 0, sample: int | None = None, fused=None) -> torch.Tensor:
    """K unit-norm centroids [K, dim] float16 of the token rows (tokens [n, dim] float16 / float32 on the device, n >= K): seeded Lloyd
    iterations for the dot product (spherical k-means, what colbert-ai trains).  The start is K rows drawn by a generator seeded with
    `seed`, `sample` (optional) trains on that many drawn rows; every step is dot_topn (fused: see centroid_probes; or dot_scores /
    topk_rows) / a one-hot dot_scores -- no float atomics -- so the result is deterministic for a given seed on a given device, the same
    by either route.  A cluster that loses all its rows keeps its centroid.
    Multi-rank callers train on ONE rank and broadcast the centroids (torch.distributed.broadcast): every shard must assign against the
    same table; no collective is built in here."""
    _dev(tokens, None, "kmeans_centroids(tokens)")
    K, n = int(K), tokens.shape[0]
    _need(tokens.dim() == 2 and 1 <= K <= n, f"kmeans_centroids: tokens [n, dim] with n >= K >= 1 expected, got {tuple(tokens.shape)} and K = {K}")
    gen = torch.Generator(device=tokens.device)
    gen.manual_seed(int(seed))
    perm = torch.randperm(n, generator=gen, device=tokens.device)
    m = n if sample is None else max(K, min(n, int(sample)))
    X = _f32_rows(tokens[perm[:m]], "kmeans_centroids(tokens)")
    C = torch.nn.functional.normalize(X[:K].clone(), dim=1)
    dim = X.shape[1]
    blk = max(4, CENTROID_BLOCK_BYTES // (4 * K) // 4 * 4)     # rows per one-hot block [K, blk]
    for _ in range(int(iters)):
        codes = _nearest(X, C, fused).long()
        sums = torch.zeros((K, dim), dtype=torch.float32, device=X.device)
        for r0 in range(0, m, blk):
            r1 = min(m, r0 + blk)
            w = round_up(r1 - r0, 4)
            onehot = torch.zeros((K, w), dtype=torch.float32, device=X.device)
            onehot[codes[r0:r1], torch.arange(r1 - r0, device=X.device)] = 1.0
            Xt = torch.zeros((dim, w), dtype=torch.float32, device=X.device)
            Xt[:, : r1 - r0] = X[r0:r1].t()
            sums = sums + dot_scores(onehot, Xt)                # [K, dim]: the block's per-cluster sums, one fixed-order GEMM
        keep = (sums == 0).all(1, keepdim=True)
        C = torch.where(keep, C, torch.nn.functional.normalize(sums, dim=1))
    return C.to(torch.float16)


def centroid_slice_table_bytes(K: int, N: int) -> int:
    return int(K) * (_n_slices(N, centroid_slice_docs()) + 1) * 8


def centroid_slice_offsets(coff: torch.Tensor, cdoc: torch.Tensor, K: int, N: int) -> torch.Tensor:
    return _slice_offsets("centroid", coff, cdoc, K, N)


def centroid_index(codes: torch.Tensor, Doff: torch.Tensor, K: int, slice_table_max_bytes: int | None = None) -> CentroidIndex:
    """The inverted index of the candidate stage: codes [sumL] (the centroid of every packed token row, centroid_assign), Doff [N + 1]
    int64 -> CentroidIndex.  A document is listed once per centroid however many of its tokens carry it; an empty document is in no list.
    torch ops only, on CPU tensors too (slice_off stays None there).  On the device the slice table is built when it is smaller than
    slice_table_max_bytes (default CENTROID_SLICE_TABLE_MAX_BYTES); above that the kernels search."""
    K, N = int(K), Doff.numel() - 1
    _need(codes.dim() == 1 and Doff.dim() == 1 and N >= 0 and K >= 0, "centroid_index: codes [sumL] and Doff [N + 1] expected")
    _need(N < 2 ** 31, "centroid_index: local document ids are int32")
    dev = codes.device
    lens = (Doff[1:] - Doff[:-1]).to(dev)
    _need(int(lens.sum()) == codes.numel(), "centroid_index: Doff must cover the token rows exactly")
    if codes.numel():
        _need(0 <= int(codes.min()) and int(codes.max()) < K, f"centroid_index: codes must lie in [0, {K})")
    doc = torch.repeat_interleave(torch.arange(N, dtype=torch.int64, device=dev), lens)
    pair = torch.unique(codes.long() * max(N, 1) + doc)          # sorted: by centroid, then document; duplicates gone
    c = torch.div(pair, max(N, 1), rounding_mode="floor")
    coff = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    coff[1:] = torch.cumsum(torch.bincount(c, minlength=K), 0)
    cdoc = (pair - c * max(N, 1)).to(torch.int32).contiguous()
    slice_off = None
    cap = CENTROID_SLICE_TABLE_MAX_BYTES if slice_table_max_bytes is None else int(slice_table_max_bytes)
    if coff.is_cuda and K > 0 and centroid_slice_table_bytes(K, N) < cap:
        slice_off = centroid_slice_offsets(coff, cdoc, K, N)
    return CentroidIndex(coff, cdoc, N, K, slice_off)


def centroid_probes(Qtok: torch.Tensor, C: torch.Tensor, nprobe: int, fused=None):
    """(pc [Q, Lq * nprobe] int32, ps [Q, Lq * nprobe] float32): per query token its nprobe best centroids by (score desc, id asc) and
    their scores <q_i, C_c>, token-major.  fused=True: dot_topn on the float32 copies -- the selection is the GEMM's epilogue and no score
    plane exists (ValueError when nprobe > dot_topn_max()); fused=False: dot_scores + topk_rows over query blocks sized by a byte budget (the
    whole [Q * Lq, K] float32 plane is 17 GB at Q = 1024, K = 65,536); None: CENTROID_FUSED, and the two kernels for an nprobe dot_topn does
    not take.  Same bits by either route.  nprobe > K pads with (pc = -1, ps = -inf): the kernels skip a negative id.  Query tokens must
    be finite: a non-finite probe score is outside the candidate score's contract."""
    use_topn = _centroid_fused(fused, int(nprobe), "centroid_probes")
    _dev(Qtok, torch.float16, "centroid_probes(Qtok)"); _dev(C, None, "centroid_probes(C)")
    _need(Qtok.dim() == 3 and C.dim() == 2 and C.shape[0] >= 1 and Qtok.shape[2] == C.shape[1] and int(nprobe) >= 1,
          "centroid_probes: Qtok [Q, Lq, dim], C [K >= 1, dim] and nprobe >= 1 expected")
    Q, Lq, dim = Qtok.shape
    K, nprobe = C.shape[0], int(nprobe)
    C32 = _f32_rows(C, "centroid_probes(C)")
    rowsT = Q * Lq
    flat = Qtok.reshape(rowsT, dim)
    pc = torch.empty((rowsT, nprobe), dtype=torch.int32, device=Qtok.device)
    ps = torch.empty((rowsT, nprobe), dtype=torch.float32, device=Qtok.device)
    rows = _topn_block_rows(dim, nprobe) if use_topn else max(1, CENTROID_BLOCK_BYTES // (4 * round_up(K, _PAD)))
    for r0 in range(0, rowsT, rows):
        X = flat[r0: r0 + rows].float().contiguous()
        s, i = dot_topn(X, C32, nprobe) if use_topn else topk_rows(dot_scores(X, C32), nprobe)
        ps[r0: r0 + rows] = s
        pc[r0: r0 + rows] = i
    return pc.view(Q, Lq * nprobe), ps.view(Q, Lq * nprobe)


def _centroid_args(what: str, index: CentroidIndex, pc, ps, Lq: int, nprobe: int, doc_lo: int, doc_hi):
    _need(_dev(pc, torch.int32, f"{what}(pc)").is_contiguous() and _dev(ps, torch.float32, f"{what}(ps)").is_contiguous(), f"{what}: pc and ps must be contiguous")
    Lq, nprobe = int(Lq), int(nprobe)
    _need(Lq >= 1 and nprobe >= 1 and pc.dim() == 2 and pc.shape[1] == Lq * nprobe and tuple(ps.shape) == tuple(pc.shape),
          f"{what}: pc and ps must be [Q, Lq * nprobe = {Lq * nprobe}]")
    _dev(index.coff, torch.int64, f"{what}(index.coff)"); _dev(index.cdoc, torch.int32, f"{what}(index.cdoc)")
    _need(index.coff.is_contiguous() and index.cdoc.is_contiguous() and index.coff.numel() == index.K + 1, f"{what}: index.coff must hold K + 1 offsets")
    if index.slice_off is not None:
        _slice_table(what, index.slice_off, index.K, index.N, "centroid")
    return (pc.shape[0], Lq, nprobe) + _doc_range(what, index.N, centroid_slice_docs(), doc_lo, doc_hi)


def centroid_scores(index: CentroidIndex, pc: torch.Tensor, ps: torch.Tensor, Lq: int, nprobe: int, doc_lo: int = 0, doc_hi: int | None = None,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """The candidate scores of documents [doc_lo, doc_hi) (default: all N) for the probe tables of centroid_probes: [Q, doc_hi - doc_lo]
    float32, scores[q][j] = the float32 chain ((+0.0 + m_i1) + m_i2) + ... over the query tokens i, ascending, that hit document
    doc_lo + j, m_i = the largest probe score of token i among the centroids the document carries; +0.0 without a hit.  Defined bit for
    bit: a range's columns are the full plane's.  doc_lo a multiple of centroid_slice_docs(), doc_hi one too or N.  Probe scores must be
    finite (non-finite query tokens are outside the contract)."""
    Q, Lq, nprobe, doc_lo, doc_hi = _centroid_args("centroid_scores", index, pc, ps, Lq, nprobe, doc_lo, doc_hi)
    out = _out("centroid_scores", out, (Q, doc_hi - doc_lo), torch.float32, pc.device, plane=True)
    check(_lib.lib().fz_centroid_scores_range_f32(_ptr(index.coff), _ptr(index.cdoc), _ptr(index.slice_off), _ptr(pc), _ptr(ps), Q, Lq, nprobe, index.N,
                                                  index.K, doc_lo, doc_hi, _ptr(out), _ld(out), _stream(pc)), "fz_centroid_scores_range_f32")
    return out


def centroid_filter(index: CentroidIndex, pc, ps, Lq: int, nprobe: int, doc_lo: int, doc_hi: int, id_base: int, tau, cand_s, cand_i, cand_len,
                    overflow):
    """fz_centroid_scores_filter_f32 on the buffers of a TopkStream (or a test's own): document d of [doc_lo, doc_hi) enters query q's
    candidates iff !(score <= tau[q]), as (score, id_base + d); cand_s / cand_i [Q, cap], cand_len [Q] int32, overflow [1] int32."""
    Q, Lq, nprobe, doc_lo, doc_hi = _centroid_args("centroid_filter", index, pc, ps, Lq, nprobe, doc_lo, doc_hi)
    cap = _cand_buffers("centroid_filter", torch.float32, Q, tau, cand_s, cand_i, cand_len, overflow)
    check(_lib.lib().fz_centroid_scores_filter_f32(_ptr(index.coff), _ptr(index.cdoc), _ptr(index.slice_off), _ptr(pc), _ptr(ps), Q, Lq, nprobe, index.N,
                                                   index.K, doc_lo, doc_hi, int(id_base), _ptr(tau), _ptr(cand_s), _ptr(cand_i), _ptr(cand_len), cap,
                                                   _ptr(overflow), _stream(pc)), "fz_centroid_scores_filter_f32")


def _centroid_source(index: CentroidIndex, pc, ps, Lq: int, nprobe: int, id_base: int) -> _Source:
    """The centroid walk whose epilogue is the filter, document d of the index = id id_base + d (ShardedCentroidIndex)."""
    def filter(st, lo, hi):
        centroid_filter(index, pc, ps, Lq, nprobe, lo, hi, id_base, st.tau, st.cand_s, st.cand_i, st.cand_len, st.overflow)
    return _Source(index.N, filter, lambda lo, hi: (centroid_scores(index, pc, ps, Lq, nprobe, doc_lo=lo, doc_hi=hi), id_base + lo),
                   grain=centroid_slice_docs(), mark="shard_centroid_filter")


# ---------------------------------------------------------------------------------------
# K2c residual-compressed token rows (csrc/rerank_residual.hip; include/fusion_hip.h 'Residual-compressed token rows')
# ---------------------------------------------------------------------------------------
RESIDUAL_NBITS = (2, 4)
RESIDUAL_SAMPLE = 131072     # token rows residual_buckets trains on by default


def _residual_nbits(what: str, nbits) -> int:
    nbits = int(nbits)
    _need(nbits in RESIDUAL_NBITS, f"{what}: nbits must be one of {RESIDUAL_NBITS}, got {nbits}")
    return nbits


def _residual_table(what: str, C: torch.Tensor, codes: torch.Tensor, n: int) -> tuple[torch.Tensor, torch.Tensor]:
    _dev(C, torch.float16, f"{what}(C)"); _dev(codes, torch.int32, f"{what}(codes)")
    _need(C.dim() == 2 and C.shape[0] >= 1 and C.shape[1] == 128, f"{what}: C must be [K >= 1, 128], got {tuple(C.shape)}")
    _need(codes.dim() == 1 and codes.numel() == n, f"{what}: codes must be [{n}] (one per token row), got {tuple(codes.shape)}")
    return C.contiguous(), codes.contiguous()


def _residual_packed(what: str, packed: torch.Tensor, weights: torch.Tensor) -> int:
    _dev(packed, torch.uint8, f"{what}(packed)"); _dev(weights, torch.float16, f"{what}(weights)")
    _need(packed.dim() == 2 and packed.shape[1] in (32, 64) and packed.is_contiguous(),
          f"{what}: packed must be a contiguous [sumL, 16 * nbits] uint8 tensor, got {tuple(packed.shape)}")
    nbits = packed.shape[1] // 16
    _need(weights.dim() == 1 and weights.numel() == 1 << nbits and weights.is_contiguous(),
          f"{what}: weights must be [{1 << nbits}] for rows of {packed.shape[1]} bytes, got {tuple(weights.shape)}")
    return nbits


def residual_check_codes(codes: torch.Tensor, K: int) -> None:
    """ValueError unless every code lies in [0, K): done ONCE when an index is built (one host read).  The kernels clamp a stored code into
    the table in any case, so a bad code can give a wrong score but never a wild address."""
    if codes.numel():
        lo, hi = int(codes.min()), int(codes.max())
        _need(0 <= lo and hi < int(K), f"residual index: codes must lie in [0, {int(K)}), found {lo} .. {hi}")


def residual_buckets(tokens: torch.Tensor, C: torch.Tensor, codes: torch.Tensor, nbits: int = 2, sample: int | None = None, seed: int = 0):
    """(cutoffs [B - 1] float32, weights [B] float16), B = 2^nbits: the buckets of the residual code, trained on the float32 residuals
    tok - C[code] of a seeded sample of token rows (default min(n, RESIDUAL_SAMPLE), drawn as kmeans_centroids draws its sample).  The m
    sample values are sorted; cutoffs[i - 1] = sorted[(i m) // B - 1] (equal-population cuts: the 16-bucket cutoffs contain the 4-bucket
    ones); weights[b] = the float64 mean of the sample values the bucket rule sends to b -- a contiguous run of the sorted sample --
    rounded to float16; an empty bucket takes its lower cutoff, bucket 0 the upper one.  torch ops on the device, no float atomics:
    deterministic for a given seed on a given device.  Multi-rank callers train on ONE rank and broadcast, as for the centroids."""
    nbits = _residual_nbits("residual_buckets", nbits)
    _dev(tokens, None, "residual_buckets(tokens)")
    _need(tokens.dim() == 2 and tokens.shape[1] == 128 and tokens.dtype in (torch.float16, torch.float32) and tokens.shape[0] >= 1,
          f"residual_buckets: tokens must be [n >= 1, 128] float16 or float32, got {tuple(tokens.shape)}")
    n = tokens.shape[0]
    C, codes = _residual_table("residual_buckets", C, codes, n)
    gen = torch.Generator(device=tokens.device)
    gen.manual_seed(int(seed))
    perm = torch.randperm(n, generator=gen, device=tokens.device)
    rows = perm[: min(n, RESIDUAL_SAMPLE if sample is None else max(1, int(sample)))]
    code = codes[rows].long().clamp_(0, C.shape[0] - 1)
    r = (tokens[rows].float() - C[code].float()).flatten()
    r = r[~torch.isnan(r)]
    srt, _ = torch.sort(r)
    m, B = srt.numel(), 1 << nbits
    _need(m >= B, f"residual_buckets: {m} sample values cannot train {B} buckets")
    at = torch.tensor([(i * m) // B - 1 for i in range(1, B)], dtype=torch.int64, device=srt.device)
    cutoffs = srt[at].contiguous()
    # values with bucket <= i are those <= cutoffs[i]: the runs' ends in the sorted sample
    ends = torch.searchsorted(srt, cutoffs, right=True).tolist()
    bounds = [0] + ends + [m]
    weights = torch.empty(B, dtype=torch.float64, device=srt.device)
    for b in range(B):
        s, e = bounds[b], bounds[b + 1]
        weights[b] = srt[s:e].double().mean() if e > s else cutoffs[max(b - 1, 0)].double()
    return cutoffs, weights.to(torch.float16)


def residual_compress(tokens: torch.Tensor, codes: torch.Tensor, C: torch.Tensor, cutoffs: torch.Tensor, nbits: int = 2,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """packed [n, 16 * nbits] uint8 (fz_residual_compress_f16): per token row and dimension the bucket of float32(tok) - float32(C[code]),
    bucket(r) = the number of cutoffs c with r > c, stored fragment-major (include/fusion_hip.h).  tokens [n, 128] float16, codes [n] int32
    (centroid_assign), C [K, 128] float16, cutoffs [2^nbits - 1] float32 non-decreasing.  `out`: n rows of a larger packed tensor."""
    nbits = _residual_nbits("residual_compress", nbits)
    _dev(tokens, torch.float16, "residual_compress(tokens)")
    _need(tokens.dim() == 2 and tokens.shape[1] == 128, f"residual_compress: tokens must be [n, 128], got {tuple(tokens.shape)}")
    n = tokens.shape[0]
    C, codes = _residual_table("residual_compress", C, codes, n)
    _dev(cutoffs, torch.float32, "residual_compress(cutoffs)")
    _need(cutoffs.dim() == 1 and cutoffs.numel() == (1 << nbits) - 1, f"residual_compress: cutoffs must be [{(1 << nbits) - 1}], got {tuple(cutoffs.shape)}")
    tokens, cutoffs = tokens.contiguous(), cutoffs.contiguous()
    if out is None:
        out = torch.empty((n, 16 * nbits), dtype=torch.uint8, device=tokens.device)
    else:
        _dev(out, torch.uint8, "residual_compress(out)")
        _need(tuple(out.shape) == (n, 16 * nbits) and out.is_contiguous(), f"residual_compress(out): a contiguous {(n, 16 * nbits)} tensor expected")
    check(_lib.lib().fz_residual_compress_f16(_ptr(tokens), _ptr(codes), _ptr(C), _ptr(cutoffs), n, C.shape[0], 128, nbits, _ptr(out),
                                              _stream(tokens)), "fz_residual_compress_f16")
    return out


def residual_decompress(packed: torch.Tensor, codes: torch.Tensor, C: torch.Tensor, weights: torch.Tensor, row_lo: int = 0,
                        row_hi: int | None = None) -> torch.Tensor:
    """D [row_hi - row_lo, 128] float16 (fz_residual_decompress_f16): D[t][j] = the float16 sum of C[code[t]][j] and weights[bucket[t][j]],
    rows [row_lo, row_hi) of the shard (default: all).  ops.maxsim_pairs over D is, bit for bit, maxsim_pairs_residual over the bytes."""
    nbits = _residual_packed("residual_decompress", packed, weights)
    n = packed.shape[0]
    C, codes = _residual_table("residual_decompress", C, codes, n)
    row_lo, row_hi = int(row_lo), n if row_hi is None else int(row_hi)
    _need(0 <= row_lo <= row_hi <= n, f"residual_decompress: rows [{row_lo}, {row_hi}) outside 0 .. {n}")
    out = torch.empty((row_hi - row_lo, 128), dtype=torch.float16, device=packed.device)
    check(_lib.lib().fz_residual_decompress_f16(_ptr(packed), _ptr(codes), _ptr(C), _ptr(weights), n, row_lo, row_hi, C.shape[0], 128, nbits,
                                                _ptr(out), _stream(packed)), "fz_residual_decompress_f16")
    return out


def maxsim_pairs_residual(Qtok: torch.Tensor, packed: torch.Tensor, codes: torch.Tensor, C: torch.Tensor, weights: torch.Tensor,
                          Doff: torch.Tensor, cand: torch.Tensor, cand_len: torch.Tensor | None = None, *, id_base: int = 0,
                          max_doc_len: int = 512, out: torch.Tensor | None = None) -> torch.Tensor:
    """maxsim_pairs over a residual-compressed shard (fz_maxsim_pairs_residual_f16): out[q, r] = what maxsim_pairs gives over
    residual_decompress(packed, codes, C, weights), bit for bit, without that matrix ever existing.  packed [sumL, 16 * nbits] uint8,
    codes [sumL] int32, C [K, 128] float16, weights [2^nbits] float16; everything else as maxsim_pairs.  No host synchronisation."""
    what = "maxsim_pairs_residual"
    Qtok, Doff, cand_len, out, (Q, Lq, dim, N, k) = _maxsim_pairs_args(what, Qtok, Doff, cand, cand_len, out, max_doc_len)
    _need(dim == 128, f"{what}: Qtok must be [Q, Lq, 128]")
    nbits = _residual_packed(what, packed, weights)
    sumL = packed.shape[0]
    C, codes = _residual_table(what, C, codes, sumL)
    check(_lib.lib().fz_maxsim_pairs_residual_f16(_ptr(Qtok), _ptr(packed), _ptr(codes), _ptr(C), _ptr(weights), C.shape[0], nbits, _ptr(Doff),
                                                  sumL, int(max_doc_len), Q, Lq, N, dim, _ptr(cand), _ld(cand), _ptr(cand_len), k, int(id_base),
                                                  _ptr(out), _ld(out), _stream(Qtok)), "fz_maxsim_pairs_residual_f16")
    return out


def f64_to_f32(src: torch.Tensor) -> torch.Tensor:
    """Plane-preserving fp64 -> fp32 (what torch.tensor(..., dtype=float32) does to BM25's Python floats, hybrid.py:255)."""
    _dev(src, torch.float64, "f64_to_f32")
    rows, n = src.shape
    ld = _ld(src)
    dst = torch.empty((max(rows, 1), ld), dtype=torch.float32, device=src.device)
    # convert the whole padded buffer when it is one allocation; otherwise row views
    check(_lib.lib().fz_f64_to_f32(_ptr(src), _ptr(dst), rows * ld - (ld - n) if rows > 0 else 0, _stream(src)), "fz_f64_to_f32")
    return dst[:rows, :n]


# ---------------------------------------------------------------------------------------
# encoder side: packed (padding-free) token rows
# ---------------------------------------------------------------------------------------
PAIR_MODES = {"longest_first": 0, "tail": 1}   # FZ_PAIR_LONGEST_FIRST / FZ_PAIR_TAIL (include/fusion_hip.h)


def _pair_store(what: str, tok, Doff, full_len):
    """The token store of the pair kernels: tok [sumL] int32, Doff [N + 1] int64, full_len [N] int32 or None.  -> N."""
    _dev(tok, torch.int32, f"{what}(tok)")
    _dev(Doff, torch.int64, f"{what}(Doff)")
    _need(tok.dim() == 1 and tok.is_contiguous(), f"{what}: tok must be a contiguous [sumL] vector")
    _need(Doff.dim() == 1 and Doff.numel() >= 1 and Doff.is_contiguous(), f"{what}: Doff must hold N + 1 offsets")
    N = Doff.numel() - 1
    if full_len is not None:
        _dev(full_len, torch.int32, f"{what}(full_len)")
        _need(tuple(full_len.shape) == (N,) and full_len.is_contiguous(), f"{what}(full_len): expected shape {(N,)}, got {tuple(full_len.shape)}")
    return N


def _pair_queries(what: str, qtok, qlen):
    _dev(qtok, torch.int32, f"{what}(qtok)")
    _dev(qlen, torch.int32, f"{what}(qlen)")
    _need(qtok.dim() == 2, f"{what}: qtok must be [Q, Lq]")
    Q, Lq = qtok.shape
    _need(tuple(qlen.shape) == (Q,) and qlen.is_contiguous(), f"{what}(qlen): expected shape {(Q,)}, got {tuple(qlen.shape)}")
    return Q, Lq


def pair_plan(cand: torch.Tensor, cand_len: torch.Tensor | None, Doff: torch.Tensor, full_len: torch.Tensor | None, id_base: int,
              qlen: torch.Tensor, Lq: int, max_length: int, mode: str, nsep: int):
    """The plan of a cross-encoder forward over candidate lists (fz_pair_plan): for every slot of cand [Q, W] int64 (global ids, rows may be
    strided; cand_len [Q] int32 or None) -> (kq, kd, L), three contiguous [Q, W] int32 planes: the query and document tokens the pair
    keeps under the tokenizer's truncation rule `mode` ('longest_first' / 'tail', include/fusion_hip.h) and the pair's row count; all 0
    where the slot is not this shard's (past cand_len, a negative id, a document outside id_base .. id_base + N - 1).  qlen [Q] int32:
    the queries' plain lengths before any cut, Lq: the columns of the query id matrix.  No host synchronisation."""
    if mode not in PAIR_MODES:
        raise ValueError(f"pair_plan: mode must be one of {sorted(PAIR_MODES)}, got {mode!r}")
    _dev(cand, torch.int64, "pair_plan(cand)")
    _dev(Doff, torch.int64, "pair_plan(Doff)")
    _dev(qlen, torch.int32, "pair_plan(qlen)")
    _need(cand.dim() == 2 and cand.shape[0] == qlen.numel() and qlen.dim() == 1, f"pair_plan: cand must be [Q = {qlen.numel()}, W], got {tuple(cand.shape)}")
    _need(Doff.dim() == 1 and Doff.numel() >= 1 and Doff.is_contiguous() and qlen.is_contiguous(), "pair_plan: Doff must hold N + 1 offsets")
    Q, W = cand.shape
    N = Doff.numel() - 1
    if cand_len is not None:
        _dev(cand_len, torch.int32, "pair_plan(cand_len)")
        _need(tuple(cand_len.shape) == (Q,) and cand_len.is_contiguous(), f"pair_plan(cand_len): expected shape {(Q,)}, got {tuple(cand_len.shape)}")
    if full_len is not None:
        _dev(full_len, torch.int32, "pair_plan(full_len)")
        _need(tuple(full_len.shape) == (N,) and full_len.is_contiguous(), f"pair_plan(full_len): expected shape {(N,)}, got {tuple(full_len.shape)}")
    plan = torch.empty((3, Q, W), dtype=torch.int32, device=cand.device)
    check(_lib.lib().fz_pair_plan(_ptr(cand), _ld(cand), _ptr(cand_len), Q, W, int(id_base), _ptr(Doff), _ptr(full_len), N, _ptr(qlen), int(Lq),
                                  int(max_length), PAIR_MODES[mode], int(nsep), _ptr(plan[0]), _ptr(plan[1]), _ptr(plan[2]), _stream(cand)),
          "fz_pair_plan")
    return plan[0], plan[1], plan[2]


def pair_fill(pairs: torch.Tensor, cu_rows: torch.Tensor, T: int, kq: torch.Tensor, kd: torch.Tensor, cand: torch.Tensor, id_base: int,
              qtok: torch.Tensor, tok: torch.Tensor, Doff: torch.Tensor, bos: int, sep: int, eos: int, pad_idx: int, nsep: int):
    """The packed rows of one forward sub-batch (fz_pair_fill): pairs [P] int32 flat slots q * W + r of cand [Q, W] in forward order,
    cu_rows [P + 1] int32 (cu_rows[P] = T), kq / kd the planes of pair_plan, qtok [Q, Lq] int32, (tok, Doff) the token store ->
    (ids [T], pos_ids [T]) int64, what embed_layernorm takes: bos, the kept query tokens, the separators, the kept document tokens, eos;
    positions pad_idx + 1 + column.  Every stored token id must index inside the model's embedding table."""
    _dev(pairs, torch.int32, "pair_fill(pairs)")
    _dev(cu_rows, torch.int32, "pair_fill(cu_rows)")
    _dev(cand, torch.int64, "pair_fill(cand)")
    _dev(qtok, torch.int32, "pair_fill(qtok)")
    N = _pair_store("pair_fill", tok, Doff, None)
    P, T = pairs.numel(), int(T)
    _need(pairs.dim() == 1 and cu_rows.dim() == 1 and cu_rows.numel() == P + 1 and pairs.is_contiguous() and cu_rows.is_contiguous(),
          f"pair_fill: pairs [P] and cu_rows [P + 1] expected, got {tuple(pairs.shape)} and {tuple(cu_rows.shape)}")
    _need(cand.dim() == 2 and qtok.dim() == 2 and qtok.shape[0] == cand.shape[0], "pair_fill: cand [Q, W] and qtok [Q, Lq] expected")
    Q, W = cand.shape
    for t_, w_ in ((kq, "kq"), (kd, "kd")):
        _dev(t_, torch.int32, f"pair_fill({w_})")
        _need(tuple(t_.shape) == (Q, W) and t_.is_contiguous(), f"pair_fill({w_}): expected a contiguous {(Q, W)} plane, got {tuple(t_.shape)}")
    _need(T >= 0, "pair_fill: T must not be negative")
    out = torch.empty((2, T), dtype=torch.int64, device=cand.device)
    check(_lib.lib().fz_pair_fill(_ptr(pairs), _ptr(cu_rows), P, T, _ptr(kq), _ptr(kd), _ptr(cand), _ld(cand), Q, W, int(id_base),
                                  _ptr(qtok) if qtok.numel() else None, qtok.stride(0) if Q > 1 else qtok.shape[1], qtok.shape[1],
                                  _ptr(tok) if tok.numel() else None, _ptr(Doff), N, int(bos), int(sep), int(eos), int(pad_idx), int(nsep),
                                  _ptr(out[0]) if T else None, _ptr(out[1]) if T else None, _stream(cand)), "fz_pair_fill")
    return out[0], out[1]


ATTN_MAX_SEQ = 16384


def attn_strips(lengths, cu_rows=None):
    """HOST helper: the strip table fz_attn_varlen_f32 walks -- one (first row, length, first query, 0) entry per 32 queries
    of every sequence, longest sequences first.  Returns (strips int32 [n_strips, 4] numpy, cu_rows int32 [B+1] numpy).
    A sequence holds at most ATTN_MAX_SEQ rows: the kernels' in-sequence byte offsets are 32-bit (include/fusion_hip.h)."""
    import numpy as np
    lengths = np.asarray(lengths, dtype=np.int64)
    _need(lengths.size == 0 or int(lengths.min()) >= 0, "attn_strips: a sequence length is negative")
    _need(lengths.size == 0 or int(lengths.max()) <= ATTN_MAX_SEQ,
          f"attn_strips: a sequence is longer than {ATTN_MAX_SEQ} rows, the most fz_attn_varlen_* addresses")
    if cu_rows is None:
        cu_rows = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum(lengths, out=cu_rows[1:])
    per = (lengths + 31) // 32
    order = np.argsort(-lengths, kind="stable")
    seq = np.repeat(order, per[order])
    first = np.zeros(len(order) + 1, dtype=np.int64)
    np.cumsum(per[order], out=first[1:])
    q0 = (np.arange(len(seq)) - np.repeat(first[:-1], per[order])) * 32
    strips = np.stack([cu_rows[seq], lengths[seq], q0, np.zeros_like(q0)], 1).astype(np.int32)
    return np.ascontiguousarray(strips), cu_rows.astype(np.int32)


def attn_varlen(qkv: torch.Tensor, strips: torch.Tensor, heads: int, scale: float | None = None, out: torch.Tensor | None = None):
    """softmax(q k^T scale) v per sequence and head over packed rows; qkv [T, 3*heads*64] fp32 -> [T, heads*64]."""
    _dev(qkv, torch.float32, "attn_varlen(qkv)")
    _dev(strips, torch.int32, "attn_varlen(strips)")
    T, W = qkv.shape
    if W != 3 * heads * 64:
        raise ValueError(f"attn_varlen: qkv is {W} wide, expected 3*{heads}*64 (head_dim 64 only)")
    if strips.dim() != 2 or strips.shape[1] != 4 or not strips.is_contiguous():
        raise ValueError("attn_varlen: strips must be a contiguous [n_strips, 4] int32 tensor (ops.attn_strips)")
    out = _out("attn_varlen", out, (T, heads * 64), torch.float32, qkv.device, plane=False)
    if scale is not None and not scale > 0:
        raise ValueError("attn_varlen: scale must be positive")
    check(_lib.lib().fz_attn_varlen_f32(_ptr(qkv), qkv.stride(0) if T > 1 else W, _ptr(strips), strips.shape[0], heads, 64,
                                        float(64 ** -0.5 if scale is None else scale), _ptr(out), out.stride(0) if T > 1 else heads * 64,
                                        _stream(qkv)), "fz_attn_varlen_f32")
    return out


def attn_varlen_f16(qkv16: torch.Tensor, strips: torch.Tensor, heads: int, out: torch.Tensor, amp: bool = False) -> torch.Tensor:
    """attn_varlen on float16 fused-QKV rows with the context rows stored as float16 (`out` [T, heads*64] float16): the attention of the
    mixed-precision forward -- float32 scores, softmax and weighted sum between two float16 Linears."""
    _dev(qkv16, torch.float16, "attn_varlen_f16(qkv16)")
    _dev(strips, torch.int32, "attn_varlen_f16(strips)")
    _dev(out, torch.float16, "attn_varlen_f16(out)")
    T, W = qkv16.shape
    if W != 3 * heads * 64:
        raise ValueError(f"attn_varlen_f16: qkv is {W} wide, expected 3*{heads}*64 (head_dim 64 only)")
    if strips.dim() != 2 or strips.shape[1] != 4 or not strips.is_contiguous():
        raise ValueError("attn_varlen_f16: strips must be a contiguous [n_strips, 4] int32 tensor (ops.attn_strips)")
    _need(tuple(out.shape) == (T, heads * 64), f"attn_varlen_f16(out): expected shape {(T, heads * 64)}, got {tuple(out.shape)}")
    fn = _lib.lib().fz_attn_varlen_f16_amp if amp else _lib.lib().fz_attn_varlen_f16     # amp: float16 matmuls (autocast's arithmetic); else float32 throughout
    check(fn(_ptr(qkv16), qkv16.stride(0) if T > 1 else W, _ptr(strips), strips.shape[0], heads, 64, float(64 ** -0.5),
             _ptr(out), out.stride(0) if T > 1 else heads * 64, _stream(qkv16)), "fz_attn_varlen_f16_amp" if amp else "fz_attn_varlen_f16")
    return out


def add_layernorm_x16(x16: torch.Tensor, res: torch.Tensor | None, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                      out: torch.Tensor | None = None, out16: torch.Tensor | None = None):
    """LayerNorm(x16 + res) with a float16 x (a mixed-precision Linear's output), float32 residual and result; out16 (float16, same
    shape) receives a second, rounded copy of the result.  -> out."""
    _dev(x16, torch.float16, "add_layernorm_x16(x16)")
    rows, d = x16.shape
    if res is not None:
        _dev(res, torch.float32, "add_layernorm_x16(res)")
        if res.shape != x16.shape:
            raise ValueError("add_layernorm_x16: x16 and res differ in shape")
    _need(gamma.numel() == d and beta.numel() == d and gamma.is_contiguous() and beta.is_contiguous(), f"add_layernorm_x16: gamma and beta must hold {d} values")
    out = _out("add_layernorm_x16", out, (rows, d), torch.float32, x16.device, plane=False)
    if out16 is not None:
        _dev(out16, torch.float16, "add_layernorm_x16(out16)")
        _need(tuple(out16.shape) == (rows, d), f"add_layernorm_x16(out16): expected shape {(rows, d)}, got {tuple(out16.shape)}")
    ldr = 0 if res is None else (res.stride(0) if rows > 1 else d)
    check(_lib.lib().fz_add_layernorm_x16(_ptr(x16), x16.stride(0) if rows > 1 else d, _ptr(res), ldr, _ptr(_dev(gamma, torch.float32, "gamma")),
                                          _ptr(_dev(beta, torch.float32, "beta")), float(eps), rows, d, _ptr(out), out.stride(0) if rows > 1 else d,
                                          _ptr(out16), 0 if out16 is None else (out16.stride(0) if rows > 1 else d), _stream(x16)), "fz_add_layernorm_x16")
    return out


def gelu_f16_(x: torch.Tensor) -> torch.Tensor:
    """In-place erf-GELU of a contiguous float16 tensor (float32 arithmetic, one rounding: torch.nn.functional.gelu on float16)."""
    _dev(x, torch.float16, "gelu_f16_(x)")
    _need(x.is_contiguous() and x.numel() % 8 == 0, "gelu_f16_: contiguous tensor with a multiple of 8 elements")
    check(_lib.lib().fz_gelu_f16(_ptr(x), _ptr(x), x.numel(), _stream(x)), "fz_gelu_f16")
    return x


def add_layernorm(x: torch.Tensor, res: torch.Tensor | None, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor | None = None):
    """LayerNorm(x + res) over the last dimension, fp32, one HBM pass."""
    _dev(x, torch.float32, "add_layernorm(x)")
    rows, d = x.shape
    if res is not None:
        _dev(res, torch.float32, "add_layernorm(res)")
        if res.shape != x.shape:
            raise ValueError("add_layernorm: x and res differ in shape")
    _need(gamma.numel() == d and beta.numel() == d and gamma.is_contiguous() and beta.is_contiguous(), f"add_layernorm: gamma and beta must hold {d} values")
    out = _out("add_layernorm", out, (rows, d), torch.float32, x.device, plane=False)
    ldr = 0 if res is None else (res.stride(0) if rows > 1 else d)
    check(_lib.lib().fz_add_layernorm_f32(_ptr(x), x.stride(0) if rows > 1 else d, _ptr(res), ldr, _ptr(_dev(gamma, torch.float32, "gamma")),
                                          _ptr(_dev(beta, torch.float32, "beta")), float(eps), rows, d, _ptr(out),
                                          out.stride(0) if rows > 1 else d, _stream(x)), "fz_add_layernorm_f32")
    return out


def gelu_(x: torch.Tensor) -> torch.Tensor:
    """In-place erf-GELU of a contiguous fp32 tensor (torch.nn.functional.gelu's expression)."""
    _dev(x, torch.float32, "gelu_(x)")
    _need(x.is_contiguous() and x.numel() % 4 == 0, "gelu_: contiguous tensor with a multiple of 4 elements")
    check(_lib.lib().fz_gelu_f32(_ptr(x), _ptr(x), x.numel(), _stream(x)), "fz_gelu_f32")
    return x


def embed_layernorm(word: torch.Tensor, pos: torch.Tensor, type0: torch.Tensor, ids: torch.Tensor, pos_ids: torch.Tensor,
                    gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """LayerNorm(word[ids] + pos[pos_ids] + type0) for packed rows, one pass; out may be a [>= rows, d] buffer (first rows written)."""
    for t_, w_ in ((word, "word"), (pos, "pos"), (type0, "type0"), (gamma, "gamma"), (beta, "beta")):
        _need(_dev(t_, torch.float32, f"embed_layernorm({w_})").is_contiguous(), f"embed_layernorm({w_}) must be contiguous")
    _dev(ids, torch.int64, "embed_layernorm(ids)"); _dev(pos_ids, torch.int64, "embed_layernorm(pos_ids)")
    rows, d = ids.numel(), word.shape[1]
    _need(pos_ids.numel() == rows and ids.is_contiguous() and pos_ids.is_contiguous(), "embed_layernorm: ids and pos_ids must be contiguous and equally long")
    _need(pos.shape[1] == d and type0.numel() == d and gamma.numel() == d and beta.numel() == d, f"embed_layernorm: tables and parameters must be {d} wide")
    if out is None:
        out = torch.empty((rows, d), dtype=torch.float32, device=word.device)
    else:
        _dev(out, torch.float32, "embed_layernorm(out)")
        _need(out.dim() == 2 and out.shape[0] >= rows and out.shape[1] == d, f"embed_layernorm(out): need a [>= {rows}, {d}] buffer")
    check(_lib.lib().fz_embed_layernorm_f32(_ptr(word), _ptr(pos), _ptr(type0), _ptr(ids), _ptr(pos_ids), _ptr(gamma), _ptr(beta), float(eps), rows, d,
                                            _ptr(out), out.stride(0) if out.shape[0] > 1 else d, _stream(word)), "fz_embed_layernorm_f32")
    return out


def _segment_reduce(fn: str, x: torch.Tensor, cu_rows: torch.Tensor) -> torch.Tensor:
    _dev(x, torch.float32, f"{fn}(x)")
    _dev(cu_rows, torch.int32, f"{fn}(cu_rows)")
    B, d = cu_rows.numel() - 1, x.shape[1]
    if x.shape[0] == 0:     # every sequence empty (an empty tensor has no data pointer to hand over): zeros by definition
        return torch.zeros((max(B, 0), d), dtype=torch.float32, device=x.device)
    out = torch.empty((max(B, 0), d), dtype=torch.float32, device=x.device)
    check(getattr(_lib.lib(), fn)(_ptr(x), x.stride(0) if x.shape[0] > 1 else d, _ptr(cu_rows), B, d, _ptr(out), d, _stream(x)), fn)
    return out


def splade_head_max(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, cu_rows: torch.Tensor) -> torch.Tensor:
    """SPLADE vocabulary projection with the pooling as its epilogue (splade/splade.py:88-99): x [T, d] packed hidden rows, weight [V, d],
    bias [V], cu_rows [B+1] int32 -> [B, V] fp32 = max over each sequence's rows of log1p(relu(x @ weight.T + bias)); the [T, V] logits
    are never written (fz_splade_head_max_f32: the fp32-MFMA tile stream of dot_scores with a segment-max / atomicMax epilogue)."""
    _dev(x, torch.float32, "splade_head_max(x)"); _dev(weight, torch.float32, "splade_head_max(weight)")
    _dev(bias, torch.float32, "splade_head_max(bias)"); _dev(cu_rows, torch.int32, "splade_head_max(cu_rows)")
    T, d = x.shape
    V = weight.shape[0]
    B = cu_rows.numel() - 1
    _need(weight.dim() == 2 and weight.shape[1] == d and bias.numel() == V and bias.is_contiguous(), f"splade_head_max: weight [V, {d}] and bias [V] expected")
    _need(cu_rows.is_contiguous() and B >= 0, "splade_head_max: cu_rows must hold B + 1 contiguous offsets")
    x, weight = pad_dim(x), pad_dim(weight)
    ldp = max(round_up(V, _PAD), _PAD)
    pool = torch.zeros((max(B, 1), ldp), dtype=torch.float32, device=x.device)[:B, :V]     # zero = log1p(relu(.)) of an empty sequence
    if T == 0 or B == 0:
        return pool
    check(_lib.lib().fz_splade_head_max_f32(_ptr(x), x.stride(0) if T > 1 else x.shape[1], _ptr(weight), weight.stride(0), _ptr(bias), _ptr(cu_rows), B, T, V,
                                            x.shape[1], _ptr(pool), ldp, _stream(x)), "fz_splade_head_max_f32")
    return pool


def splade_head_max_f16(x16: torch.Tensor, weight16: torch.Tensor, bias: torch.Tensor, cu_rows: torch.Tensor) -> torch.Tensor:
    """splade_head_max for the mixed-precision encoders: x16 [T, d] and weight16 [V, d] float16, bias [V] float32, cu_rows [B+1] int32 ->
    [B, V] fp32, products accumulated in float32 (fz_splade_head_max_f16: v_mfma_f32_32x32x16_f16 tiles with the same pooling epilogue).
    d must be a multiple of 8 (ValueError: there is no padding copy); rows 16-byte aligned."""
    _dev(x16, torch.float16, "splade_head_max_f16(x16)"); _dev(weight16, torch.float16, "splade_head_max_f16(weight16)")
    _dev(bias, torch.float32, "splade_head_max_f16(bias)"); _dev(cu_rows, torch.int32, "splade_head_max_f16(cu_rows)")
    _need(x16.dim() == 2 and weight16.dim() == 2, "splade_head_max_f16: x16 [T, d] and weight16 [V, d] expected")
    T, d = x16.shape
    V = weight16.shape[0]
    B = cu_rows.numel() - 1
    _need(weight16.shape[1] == d and bias.numel() == V and bias.is_contiguous(), f"splade_head_max_f16: weight16 [V, {d}] and bias [V] expected")
    _need(cu_rows.is_contiguous() and B >= 0, "splade_head_max_f16: cu_rows must hold B + 1 contiguous offsets")
    _need(d % 8 == 0, f"splade_head_max_f16: d = {d} is not a multiple of 8")
    ldp = max(round_up(V, _PAD), _PAD)
    pool = torch.zeros((max(B, 1), ldp), dtype=torch.float32, device=x16.device)[:B, :V]     # zero = log1p(relu(.)) of an empty sequence
    if T == 0 or B == 0:
        return pool
    check(_lib.lib().fz_splade_head_max_f16(_ptr(x16), x16.stride(0) if T > 1 else d, _ptr(weight16), weight16.stride(0) if V > 1 else d, _ptr(bias),
                                            _ptr(cu_rows), B, T, V, d, _ptr(pool), ldp, _stream(x16)), "fz_splade_head_max_f16")
    return pool


def segment_mean(x: torch.Tensor, cu_rows: torch.Tensor) -> torch.Tensor:
    """Mean over each sequence's rows: x [T, d] fp32, cu_rows [B+1] int32 -> [B, d]."""
    return _segment_reduce("fz_segment_mean_f32", x, cu_rows)


def segment_splade_max(x: torch.Tensor, cu_rows: torch.Tensor) -> torch.Tensor:
    """SPLADE-max pooling: log1p(relu(max over each sequence's rows)): x [T, V] fp32 logits -> [B, V]."""
    return _segment_reduce("fz_segment_splade_max_f32", x, cu_rows)
