"""Corpus-scale SPLADE search, host side (no GPU): the two ABI 20 entry points reject bad arguments before any HIP call, and the piece
planning of TopkStream's feeds cuts a document range into whole grains (slices for feed_sparse, single documents otherwise) that cover it
exactly once."""
import numpy as np
import pytest

from fusion_amd import _lib, ops

ERR, OK = _lib.FZ_ERR_ARG, _lib.FZ_OK
S = 7168
one = 16   # any non-null address: every call below is refused (or has nothing to do) before a pointer is touched


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def rng_call(L, Q=1, N=3 * S, lo=0, hi=None, scores=one, lds=None, toff=one, qoff=one):
    hi = N if hi is None else hi
    lds = hi - lo if lds is None else lds
    return L.fz_sparse_dot_range_f32(toff, one, one, None, qoff, one, one, Q, N, lo, hi, scores, lds, None)


def filt_call(L, Q=1, N=3 * S, lo=0, hi=None, cap=64, tau=one, cs=one, ci=one, cl=one, ov=one, toff=one, qoff=one):
    hi = N if hi is None else hi
    return L.fz_sparse_dot_filter_f32(toff, one, one, None, qoff, one, one, Q, N, lo, hi, 3 << 31, tau, cs, ci, cl, cap, ov, None)


def test_slice_grain(L):
    assert L.fz_sparse_slice_docs() == S and ops.sparse_slice_docs() == S
    assert L.fz_abi_version() == _lib.ABI_VERSION == 20


def test_range_entry_rejects_bad_arguments(L):
    assert rng_call(L, toff=None) == ERR
    assert rng_call(L, qoff=None) == ERR
    assert rng_call(L, scores=None) == ERR
    assert rng_call(L, Q=-1) == ERR
    assert rng_call(L, N=-1, hi=0) == ERR
    assert rng_call(L, lo=1) == ERR                          # doc_lo off the slice grain
    assert rng_call(L, lo=S + 64, hi=2 * S) == ERR
    assert rng_call(L, lo=0, hi=S + 5) == ERR                # doc_hi neither a whole slice nor N
    assert rng_call(L, hi=3 * S + 1) == ERR                  # doc_hi > N
    assert rng_call(L, lo=2 * S, hi=S) == ERR                # doc_hi < doc_lo
    assert rng_call(L, lo=-S, hi=S) == ERR
    assert rng_call(L, lds=3 * S - 1) == ERR                 # lds < doc_hi - doc_lo
    assert rng_call(L, lo=S, hi=2 * S, lds=S - 1) == ERR
    # the old entry keeps its checks
    assert L.fz_sparse_dot_f32(one, one, one, None, one, one, one, 1, 10, one, 9, None) == ERR
    assert L.fz_sparse_dot_f32(None, None, None, None, None, None, None, 1, 1, None, 1, None) == ERR


def test_range_entry_nothing_to_do(L):
    assert rng_call(L, lo=S, hi=S, scores=None, toff=None, qoff=None) == OK          # empty range
    assert rng_call(L, lo=3 * S, hi=3 * S) == OK
    assert rng_call(L, Q=0, scores=None, toff=None, qoff=None) == OK                # no queries
    assert rng_call(L, N=0, hi=0, lds=0) == OK
    assert L.fz_sparse_dot_f32(None, None, None, None, None, None, None, 0, 5, None, 5, None) == OK


def test_filter_entry_rejects_bad_arguments(L):
    for name in ("tau", "cs", "ci", "cl", "ov", "toff", "qoff"):
        assert filt_call(L, **{name: None}) == ERR, name
    assert filt_call(L, cap=0) == ERR
    assert filt_call(L, cap=-3) == ERR
    assert filt_call(L, cap=0, lo=S, hi=S) == ERR            # cap is checked even when there is nothing to score
    assert filt_call(L, lo=100) == ERR
    assert filt_call(L, lo=S, hi=2 * S - 1) == ERR
    assert filt_call(L, hi=3 * S + 1) == ERR
    assert filt_call(L, N=-1, hi=0) == ERR
    assert filt_call(L, Q=-1) == ERR


def test_filter_entry_nothing_to_do(L):
    assert filt_call(L, lo=2 * S, hi=2 * S, tau=None, cs=None, ci=None, cl=None, ov=None) == OK
    assert filt_call(L, Q=0, tau=None, cs=None, ci=None, cl=None, ov=None) == OK
    assert filt_call(L, N=0, hi=0) == OK


@pytest.mark.parametrize("lo,hi,seen,pending,k,cap", [
    (14336, 1_105_228, 14336, 0, 1000, 7168),       # one eighth of mMARCO after the head, k = 1000
    (14336, 250_003, 14336, 0, 100, 7168),
    (14336, 250_003, 14336, 0, 1, 7168),
    (7168, 7168 * 40, 7168, 0, 1000, 64),          # windows shorter than a slice: one slice per piece
    (0, 7168 * 9 + 17, 100, 50, 7, 7168),          # an end off the grain (the index's N)
    (7168 * 3, 7168 * 4, 5000, 4999, 1000, 7168),
    (7168, 7168, 7168, 0, 10, 7168),               # empty
])
def test_sparse_pieces_are_whole_slices_covering_the_range_once(lo, hi, seen, pending, k, cap):
    check_pieces(lo, hi, seen, pending, k, cap, S)


@pytest.mark.parametrize("lo,hi,seen,pending,k,cap", [
    (8192, 1_105_228, 8192, 0, 1000, 7168),        # feed, feed_gemm: the dense shard after its head
    (0, 150_000, 4096, 40_959, 100, 2000),         # pending one document below the window (40,960)
    (5, 30_000, 512, 0, 7, 256),                   # the range ends mid-window
    (0, 10_000, 1, 0, 1000, 64),                   # the 64-document minimum window
    (9, 9, 4096, 3, 100, 2000),                    # empty
])
def test_stream_pieces_at_grain_one_cover_the_range_once(lo, hi, seen, pending, k, cap):
    check_pieces(lo, hi, seen, pending, k, cap, 1)


def check_pieces(lo, hi, seen, pending, k, cap, grain):
    pieces = ops.stream_pieces(lo, hi, seen, pending, k, cap, grain)
    if lo == hi:
        assert pieces == []
        return
    assert pieces[0][0] == lo and pieces[-1][1] == hi
    for (a, b, _), (c, _, _) in zip(pieces, pieces[1:]):
        assert b == c                                      # back to back, ascending
    for a, b, _ in pieces:
        assert a < b and a % grain == 0
        assert (b - a) % grain == 0 or b == hi             # whole grains, the last one may end at the range's end
        assert b - a >= grain or b == hi                   # at least one grain per piece
    # the fold flags replay TopkStream's window bookkeeping (its window rounded down to whole grains): a fold where the window is full,
    # and pieces never cross a window boundary by more than the one-grain minimum
    for a, b, fold in pieces:
        win = max(grain, ops.stream_window(seen, k, cap) // grain * grain)
        room = win - pending
        assert b - a <= max(grain, room)
        pending += b - a
        assert fold == (pending >= win)
        if fold:
            seen, pending = seen + pending, 0


def test_sparse_pieces_windows_grow():
    """After the 14,336-document head at k = 1000 the windows grow geometrically: a 1.1 M-document shard folds a handful of times."""
    pieces = ops.stream_pieces(14336, 1_105_228, 14336, 0, 1000, 7168, S)
    folds = sum(f for _, _, f in pieces) + (not pieces[-1][2])    # + the one TopkStream.result() does on what is left
    assert 3 <= folds <= 8
    sizes = [b - a for a, b, _ in pieces]
    assert sizes[-1] >= sizes[0]


def inline_cut(n, seen, pending, k, cap):
    """The cut TopkStream.feed and feed_gemm made in place before they shared the planner: a piece ends where the window does (or at n),
    and the stream folds when the window is full."""
    out, lo = [], 0
    while lo < n:
        hi = min(n, lo + ops.stream_window(seen, k, cap) - pending)
        pending += hi - lo
        fold = pending >= ops.stream_window(seen, k, cap)
        if fold:
            seen, pending = seen + pending, 0
        out.append((lo, hi, fold))
        lo = hi
    return out


def test_stream_pieces_at_grain_one_are_the_inline_cut():
    rng = np.random.default_rng(7)
    cases = [(0, 4096, 0, 100, 2000),                          # nothing to feed
             (150_000, 4096, 40_959, 100, 2000),               # pending one document below the window (40,960)
             (150_000, 4096, 40_896, 100, 2000),               # ... and one 64-document step below it
             (100_000, 8192, 0, 1000, 7168),                   # the range ends mid-window
             (29_312, 8192, 0, 1000, 7168),                    # ... and exactly on the window's end
             (1_097_036, 8192, 0, 1000, 7168)]                 # one eighth of mMARCO after the dense head
    for _ in range(2000):
        k, cap, seen = int(rng.integers(1, 2001)), int(rng.integers(2, 9001)), int(rng.integers(1, 2_000_000))
        cases.append((int(rng.integers(0, 3_000_000)), seen, int(rng.integers(0, ops.stream_window(seen, k, cap))), k, cap))
    for n, seen, pending, k, cap in cases:
        assert pending < ops.stream_window(seen, k, cap)        # TopkStream's invariant between feeds
        assert ops.stream_pieces(0, n, seen, pending, k, cap, 1) == inline_cut(n, seen, pending, k, cap), (n, seen, pending, k, cap)
        assert ops.stream_pieces(0, n, seen, pending, k, cap) == inline_cut(n, seen, pending, k, cap)          # grain defaults to 1
