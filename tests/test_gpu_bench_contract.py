"""The benchmark line itself (bench.py, the driver's contract): every key the driver and the judge read is present and
sane, on a tiny configuration so that the test takes seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_line_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "24", "--warmup", "2", "--streams", "8",
                          "--cpu-seconds", "3", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                           # ONE JSON line
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 24 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["unit"] == "frames/s" and d["dtype"] == "f64" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["streams_per_gpu"] == 8
    assert abs(d["value"] - 8 * 24 / (d["ms_per_step"] * 24e-3)) < 0.01 * d["value"]      # value = frames of the job / timed seconds
    r = d["roofline"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] == 1 and c["value"] > 0
    assert d["config"]["streams_tracking_good"] == 8
    assert d["parity_pose_maxdiff_stream0"] is not None and d["parity_pose_maxdiff_stream0"] < 1e-4   # north_star pose tolerance


def _run(args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_config_ba_line():
    """bench.py --config ba: BASELINE configs[2] itself (5 cameras x 300 points, M = 1500, 10 LM iterations) -- SURVEY.md 8(d)'s 316,000 B
    and 1.56 MFLOP per LM trial in the roofline (from the launch's own device counters), the oracle's Compute() latency on one core, and
    problem 0 against the oracle."""
    d = _run(["--config", "ba", "--problems", "64", "--steps", "3", "--warmup", "1", "--cpu-seconds", "2", "--full"])
    assert d["unit"] == "computes/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["config"]["problems_per_gpu"] == 64
    r = d["roofline"]
    assert r["kernel"] == "k_ba_compute" and r["bound"] == "hbm" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5
    assert abs(r["bytes_per_lm_trial"] - 315960) < 0.06 * 315960 and abs(r["flops_per_lm_trial"] - 1.56e6) < 0.06 * 1.56e6      # (a few per cent of the 1500 projections fall outside the image and are not measured)
    assert abs(d["value"] - 64 * 3 / (d["ms_per_step"] * 3e-3)) < 0.01 * d["value"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["compute_latency_ms"] > 0 and c["unit"] == "computes/s"
    p = d["parity_problem0_oracle_vs_device"]
    assert p["accepted"][0] == p["accepted"][1] and p["lm_trials"][0] == p["lm_trials"][1] and p["camera_maxdiff"] < 1e-4


def test_bench_host_frames_line():
    """bench.py --host-frames: the PCIe-inclusive variant through vslam_update (native_update's way); reported apart from the headline."""
    d = _run(["--host-frames", "--streams", "8", "--steps", "6", "--warmup", "2", "--cpu-seconds", "1", "--no-all-cores", "--no-flat-out", "--full"])
    assert d["pcie_inclusive"] and d["pcie_inclusive"]["frames_per_s"] == d["value"] and "host memory" in d["data"]
    assert d["config"]["streams_tracking_good"] == 8 and d["parity_pose_maxdiff_stream0"] < 1e-4
    assert d["per_rank"][0]["rank"] == 0 and abs(d["per_rank"][0]["frames_per_s"] - d["value"]) < 0.01 * d["value"]


def test_bench_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run (no --full) prints the headline line without the --full measurements; --dump-outputs writes the last timed
    step's per-stream state, and two runs with the same arguments write the same arrays (seeded inputs)."""
    dumps = []
    for i in range(2):
        d_ = str(tmp_path / ("run%d" % i))
        d = _run(["--gpus", "1", "--streams", "8", "--steps", "24", "--warmup", "2", "--dump-outputs", d_])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        for k in ("roofline", "cpu_baseline", "stages", "ba_flat_out", "parity_pose_maxdiff_stream0"):
            assert k not in d, k
        assert d["steps"] == 24 and d["warmup"] == 2 and d["unit"] == "frames/s" and d["dtype"] == "f64"
        assert abs(d["value"] - 8 * 24 / (d["ms_per_step"] * 24e-3)) < 0.01 * d["value"]
        assert d["config"]["streams_tracking_good"] == 8
        dumps.append({f: np.load(os.path.join(d_, f)) for f in sorted(os.listdir(d_))})
    a, b = dumps
    assert "pose.npy" in a and a["pose.npy"].shape == (8, 12) and a["pose.npy"].dtype == np.float64
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]), f


def test_bench_frame_ring_refilled_between_segments_computes_the_same(tmp_path):
    """Steps beyond what the device holds: with a ring of 7 frames the 27 frames are played in segments, the ring refilled between
    them, and the last step leaves every stream exactly where the run with all frames resident does."""
    dumps = []
    for ring in (0, 7):
        d_ = str(tmp_path / ("ring%d" % ring))
        d = _run(["--gpus", "1", "--streams", "16", "--steps", "24", "--warmup", "3", "--ring-frames", str(ring), "--dump-outputs", d_])
        assert d["config"]["frame_ring_frames"] == (27 if ring == 0 else 7) and d["steps"] == 24
        assert d["config"]["streams_tracking_good"] == 16
        dumps.append({f: np.load(os.path.join(d_, f)) for f in sorted(os.listdir(d_))})
    a, b = dumps
    assert sorted(a) == sorted(b) and "pose.npy" in a
    for f in a:
        assert np.array_equal(a[f], b[f]), f
