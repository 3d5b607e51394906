"""The bench line the driver parses stays compact (round 4's 20 kB line came back `parsed: null`).
Builds the headline dict from RECORDED full results (profiles/*.json hold what bench_detail.json holds) -- no GPU."""
import glob
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")
RECORDED = sorted(p for p in glob.glob(os.path.join(ROOT, "profiles", "r0[2-9]_bench_*.json")) if not p.endswith("_line.json"))   # full records
LINES = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[5-9]_bench_*_line.json")))                                            # compact lines as printed


def _reject_constant(c):
    raise AssertionError(f"non-strict JSON constant {c}")


@pytest.mark.parametrize("path", RECORDED, ids=[os.path.basename(p) for p in RECORDED])
def test_compact_line_from_recorded_detail(path):
    res = json.load(open(path))
    if "metric" not in res:
        pytest.skip("not a bench record")
    line = json.dumps(bench.compact_line(res), allow_nan=False)
    assert len(line) < bench.LINE_BUDGET <= 6000, len(line)
    back = json.loads(line, parse_constant=_reject_constant)
    for k in REQUIRED:
        assert k in back, k
    assert back["value"] == res["value"] and back["ms_per_step"] == res["ms_per_step"]       # the headline keeps every digit
    assert "roofline_all" not in back and "configs_measured" not in back
    if "roofline" in res:
        for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert k in back["roofline"], k
        assert back["roofline"]["frac"] == pytest.approx(res["roofline"]["frac"], rel=1e-3)
        src = back["roofline"].get("traffic_source")
        assert src is None or (src.endswith(".json") and " " not in src)
    if "cpu_baseline" in res:
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in back["cpu_baseline"], k
    for v in back["config"].values():
        assert not isinstance(v, (dict, list)) or len(json.dumps(v)) < 200


@pytest.mark.parametrize("path", LINES, ids=[os.path.basename(p) for p in LINES])
def test_recorded_compact_lines_are_what_the_driver_can_parse(path):
    raw = open(path).read().strip()
    assert "\n" not in raw and len(raw) < bench.LINE_BUDGET
    line = json.loads(raw, parse_constant=_reject_constant)
    for k in REQUIRED:
        assert k in line, k
    assert "roofline_all" not in line and "configs_measured" not in line and line["detail"] == "bench_detail.json"
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    assert {"value", "unit", "cores", "kind", "sample"} <= set(line["cpu_baseline"])


def test_recorded_files_cover_both_workloads():
    names = [os.path.basename(p) for p in RECORDED]
    assert any("default" in n for n in names) and any("mmarco" in n or "launcher" in n for n in names)


def test_non_finite_floats_become_null():
    res = {"metric": "m", "value": 1.0, "ms_per_step": 1.0, "config": {"workload": "w", "x": float("nan")},
           "stages_ms": {"a": float("inf")}, "roofline": {"kernel": "k", "frac": 0.5, "traffic": None, "traffic_source": None}}
    line = json.dumps(bench.compact_line(res), allow_nan=False)
    back = json.loads(line)
    assert back["config"]["x"] is None and back["stages_ms"]["a"] is None


def test_emit_prints_one_stdout_line_and_writes_the_detail(tmp_path, capsys, monkeypatch):
    res = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_default.json")))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bench.emit(res)
    out, err = capsys.readouterr()
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"') and len(lines[0]) < 6000
    assert json.load(open(tmp_path / "bench_detail.json"))["configs_measured"] == res["configs_measured"]
    assert "[bench detail]" in err


# ---- the plain run / --full / --dump-outputs surface (no GPU: parsing and the dump helper on host tensors) ------------------------------
def test_plain_run_is_the_default_and_full_is_opt_in():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    b = bench.parse(["--full", "--dump-outputs", "out_dir", "--no-configs"])
    assert b.full is True and b.dump_outputs == "out_dir" and b.no_configs is True


def test_dump_outputs_writes_every_array_exactly_when_it_fits(tmp_path):
    import numpy as np
    import torch
    order = torch.arange(12, dtype=torch.int32).reshape(3, 4).flip(1)
    scores = torch.tensor([[0.5, 0.25, 0.125, 1 / 3]] * 3, dtype=torch.float64)
    emb = torch.randn(3, 5, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"final_order": order, "fused_scores": scores, "emb": emb})
    o, s, e, rows = (np.load(tmp_path / "d" / f"{n}.npy") for n in ("final_order", "fused_scores", "emb", "rows"))
    assert o.dtype == np.float64 and np.array_equal(o, order.numpy())          # integers: exact in float64
    assert s.dtype == np.float64 and np.array_equal(s, scores.numpy())
    assert e.dtype == np.float32 and np.array_equal(e, emb.numpy())
    assert np.array_equal(rows, np.arange(3))


def test_dump_outputs_samples_the_same_seeded_rows_within_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch
    R, C = 1000, 64
    order = torch.arange(R * C, dtype=torch.int32).reshape(R, C)
    scores = torch.rand((R, C), dtype=torch.float64)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 100 * C * 16)                       # room for 100 rows of both arrays
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"final_order": order, "fused_scores": scores})
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert len(rows) == 100 and np.all(np.diff(rows) > 0) and rows[-1] < R
    o, s = np.load(tmp_path / "a" / "final_order.npy"), np.load(tmp_path / "a" / "fused_scores.npy")
    assert o.nbytes + s.nbytes <= bench.DUMP_BUDGET
    idx = rows.astype(np.int64)
    assert np.array_equal(o, order.numpy()[idx]) and np.array_equal(s, scores.numpy()[idx])       # the same rows of both
    for n in ("rows", "final_order", "fused_scores"):                                             # fixed seed: run to run identical
        assert np.array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy"))


def test_dump_outputs_keeps_the_head_of_a_row_longer_than_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch
    order = torch.arange(4 * 1000, dtype=torch.int32).reshape(4, 1000)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 800)                                # 100 float64 values
    bench.dump_outputs(str(tmp_path), {"final_order": order})
    o = np.load(tmp_path / "final_order.npy")
    assert o.shape == (1, 100) and o.nbytes <= 800
    r = int(np.load(tmp_path / "rows.npy")[0])
    assert np.array_equal(o[0], order.numpy()[r, :100])
