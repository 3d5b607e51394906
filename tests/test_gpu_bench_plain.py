"""bench.py's plain run on the MI355X: the timed steps and the headline only (no instrumented region, roofline, CPU baseline), and
--dump-outputs writes what the last timed step returned -- the same arrays, bit for bit, from two runs with the same arguments.
Each run is a fresh child process at a small shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

Q, N = 48, 3000


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--queries", str(Q), "--corpus", str(N), *extra],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), r.stdout[-2000:]
    return json.loads(lines[0])


def load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.endswith(".npy")}


def test_plain_run_times_the_steps_and_dumps_the_ranked_lists(tmp_path):
    line = run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "queries/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(Q * 1e3 / line["ms_per_step"], rel=1e-9)
    for k in ("stages_ms", "roofline", "cpu_baseline", "parity_sample", "north_star_targets"):
        assert k not in line, k                                                    # --full only
    out = load(tmp_path / "a")
    assert set(out) == {"final_order", "fused_scores", "rows"}
    o, s = out["final_order"], out["fused_scores"]
    assert o.shape == s.shape == (Q, N) and o.dtype == s.dtype == np.float64 and np.array_equal(out["rows"], np.arange(Q))
    assert np.array_equal(np.sort(o, axis=1), np.broadcast_to(np.arange(N, dtype=np.float64), (Q, N)))   # every row a full ranked list
    assert np.all(np.diff(s, axis=1) <= 0) and np.all(s > 0)                                               # RRF scores, descending


def test_dumped_outputs_are_identical_run_to_run(tmp_path):
    # the score / rank / fuse kernels alone (query embeddings from the seeded generator): the inputs are the same, so are the outputs
    for d in ("a", "b"):
        run_bench("--steps", "2", "--warmup", "1", "--no-encode", "--dump-outputs", str(tmp_path / d))
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    assert set(a) == set(b) == {"final_order", "fused_scores", "rows"}
    for n in a:
        assert np.array_equal(a[n], b[n]), n
