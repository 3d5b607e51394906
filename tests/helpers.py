"""Shared comparison helpers for the parity tests."""
import numpy as np


def assert_ranked_close(got_ids, got_sc, exp_ids, exp_sc, tol, truncated=False):
    """Two score-descending ranked lists agree: the score SEQUENCES are within `tol` element by element (order
    statistics move by at most the perturbation of the scores), and the ids agree as sets inside every run of
    expected scores that are closer than 2*tol to their neighbour (ties / near-ties: their relative order is
    implementation-defined in the reference -- unsorted topk + heap order, splade/base.py:229-240).  With
    `truncated` (k < N) the last run may have lost members to the cut and is skipped."""
    got_ids, exp_ids = np.asarray(got_ids), np.asarray(exp_ids)
    got_sc, exp_sc = np.asarray(got_sc, dtype=np.float64), np.asarray(exp_sc, dtype=np.float64)
    assert got_ids.shape == exp_ids.shape and got_sc.shape == exp_sc.shape == got_ids.shape
    assert np.max(np.abs(got_sc - exp_sc), initial=0.0) <= tol
    assert np.all(got_sc[:-1] >= got_sc[1:]), "list not sorted by score descending"
    n = len(exp_sc)
    cut = np.flatnonzero(exp_sc[:-1] - exp_sc[1:] > 2 * tol) + 1
    bounds = np.concatenate([[0], cut, [n]])
    for a, b in zip(bounds[:-1], bounds[1:]):
        if truncated and b == n:
            continue
        if b - a == 1:
            assert got_ids[a] == exp_ids[a], (a, got_ids[a], exp_ids[a])
        else:
            assert sorted(got_ids[a:b].tolist()) == sorted(exp_ids[a:b].tolist()), (a, b)


def sparse_to_dense(z, prefix, rows, V):
    X = np.zeros((rows, V), dtype=np.float32)
    X[z[f"{prefix}_row"], z[f"{prefix}_col"]] = z[f"{prefix}_val"]
    return X


def load_lists(z):
    """tests/golden/*.npz (in_ids / in_scores / in_len) -> the reference's RankedLists per system."""
    systems = [str(s) for s in z["systems"]]
    ids, sc, ln = z["in_ids"], z["in_scores"], z["in_len"]
    Q = ids.shape[1]
    lists = {s: [[{"corpus_id": int(ids[si, q, r]), "score": float(sc[si, q, r])} for r in range(ln[si, q])] for q in range(Q)]
             for si, s in enumerate(systems)}
    return systems, lists, Q


def integration_snippet(root):
    """The reference-side ctypes binding printed in INTEGRATION.md section 2 (the fenced python block that defines rrf()), with the
    library name replaced by this tree's libfusion_hip.so."""
    import os
    import re
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", text, re.S)
    code = [b for b in blocks if "def rrf(" in b]
    assert len(code) == 1, "INTEGRATION.md must hold exactly one binding snippet that defines rrf()"
    from fusion_amd import _lib
    return code[0].replace('"libfusion_hip.so"', repr(_lib.LIB_PATH))


def quantile_table(pool, P):
    """np.quantile(pool, np.linspace(0, 1, P)) (linear interpolation) by one sort: numpy's own takes ~40 s for 38,000 quantiles
    (one partition step per quantile)."""
    s = np.sort(np.asarray(pool, dtype=np.float64).ravel())
    pos = np.linspace(0.0, len(s) - 1.0, P)
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(lo + 1, len(s) - 1)
    return s[lo] + (s[hi] - s[lo]) * (pos - lo)


def planned_search_marks(ops, head, n, chunk, k, cap, grain, plane_mark, filter_mark):
    """The marks a streamed sharded search of n documents must report, derived from the piece planner alone: the head's plane and the
    opening of the stream, then per CHUNK-document feed one launch mark per planned piece with the stream's mark after every planned fold,
    then the closing fold and the all-gather.  -> (marks, planned folds, feeds that start inside a window)."""
    marks, folds, inside = [plane_mark, "shard_topk_stream"], 0, 0
    seen, pending = head, 0
    for c0 in range(head, n, chunk):
        inside += pending > 0
        for lo, hi, fold in ops.stream_pieces(c0, min(n, c0 + chunk), seen, pending, k, cap, grain):
            marks.append(filter_mark)
            pending += hi - lo
            if fold:
                marks.append("shard_topk_stream")
                seen, pending, folds = seen + pending, 0, folds + 1
    return marks + ["shard_topk_stream", "allgather_merge"], folds, inside


def dynamic_fz_symbols(path: str) -> set:
    """The fz_* names a shared library defines in its dynamic symbol table (nm -D --defined-only, or ROCm's llvm-nm); skips the calling test
    where neither tool is installed."""
    import os
    import shutil
    import subprocess
    import pytest
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    tools = [shutil.which("nm"), shutil.which("llvm-nm"), os.path.join(rocm, "lib", "llvm", "bin", "llvm-nm"), os.path.join(rocm, "llvm", "bin", "llvm-nm")]
    tool = next((t for t in tools if t and os.path.exists(t)), None)
    if tool is None:
        pytest.skip("neither nm nor llvm-nm is on this machine: the library's dynamic symbol table cannot be read")
    out = subprocess.run([tool, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("fz_")}
