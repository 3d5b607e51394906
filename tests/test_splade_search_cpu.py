"""Corpus-scale SPLADE search, host side (no GPU): the two ABI 20 entry points reject bad arguments before any HIP call, and the piece
planning of TopkStream.feed_sparse cuts a document range into whole slices that cover it exactly once."""
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
    pieces = ops.sparse_pieces(lo, hi, seen, pending, k, cap, S)
    if lo == hi:
        assert pieces == []
        return
    assert pieces[0][0] == lo and pieces[-1][1] == hi
    for (a, b, _), (c, _, _) in zip(pieces, pieces[1:]):
        assert b == c                                      # back to back, ascending
    for a, b, _ in pieces:
        assert a < b and a % S == 0
        assert (b - a) % S == 0 or b == hi                 # whole slices, the last one may end at the range's end
        assert b - a >= S or b == hi                        # at least one slice per piece
    # the fold flags replay TopkStream's window bookkeeping (its window rounded down to whole slices): a fold where the window is full,
    # and pieces never cross a window boundary by more than the one-slice minimum
    for a, b, fold in pieces:
        win = max(S, ops.stream_window(seen, k, cap) // S * S)
        room = win - pending
        assert b - a <= max(S, room)
        pending += b - a
        assert fold == (pending >= win)
        if fold:
            seen, pending = seen + pending, 0


def test_sparse_pieces_windows_grow():
    """After the 14,336-document head at k = 1000 the windows grow geometrically: a 1.1 M-document shard folds a handful of times."""
    pieces = ops.sparse_pieces(14336, 1_105_228, 14336, 0, 1000, 7168, S)
    folds = sum(f for _, _, f in pieces) + (not pieces[-1][2])    # + the one TopkStream.result() does on what is left
    assert 3 <= folds <= 8
    sizes = [b - a for a, b, _ in pieces]
    assert sizes[-1] >= sizes[0]
