"""The measurement contract of bench.py, checked on the GPU box: one JSON line on stdout with the driver's keys; under --full the
roofline object of the dominant kernel (+ whole-step fraction) and a cpu_baseline object unless it is switched off; a plain run that
times exactly --steps steps and, with --dump-outputs, writes one step from the seeded state, the same in every run.  Short runs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"bench.py must print ONE line on stdout, got {len(lines)}"
    return json.loads(lines[0])


def test_bench_line_contract(cuda):
    d = _run("--full", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-secondary", "--decode-steps", "2", "--sustain-seconds", "0")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "bf16" and d["data"] == "synthetic" and d["unit"] == "image-lines/s"
    assert d["config"]["workload"].startswith("c3") and d["config"]["global_batch"] == 256
    assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]            # whole-job throughput = lines / measured time
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "step_frac", "ms_per_launch"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0.05 < r["frac"] < 1.0 and 0.05 < r["step_frac"] < r["frac"] + 0.3
    assert "filter gradient" in r["kernel"] and "forward" in d["roofline_best"]["kernel"]
    assert d["decode_chars_per_s"] > 1e5 and d["families"]["_sum_ms"] > 0
    assert "cpu_baseline" not in d                                                            # --no-cpu-baseline


def test_bench_other_workloads_run(cuda):
    d = _run("--full", "--workload", "c2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-secondary", "--decode-steps", "0", "--sustain-seconds", "0")
    assert d["dtype"] == "f32" and d["roofline"]["peak"] == 157.3 and d["config"]["img"] == "32x100"
    d = _run("--workload", "c4", "--steps", "24", "--warmup", "2", "--no-cpu-baseline", "--no-secondary", "--decode-steps", "0", "--sustain-seconds", "0")
    assert d["config"]["per_gpu_batch"] == 64 and d["cluster_fallback"] is False and d["value"] > 1000
    d = _run("--dropout", "0.3", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-secondary", "--decode-steps", "0", "--sustain-seconds", "0")
    assert d["dropout"] == 0.3 and d["cluster_fallback"] is False


def test_bench_plain_run_and_reproducible_dump(cuda, tmp_path):
    """A plain run does the headline measurement only.  --dump-outputs writes one step of the timed path from the seeded starting state
    (float32 / float64, under 64 MB): two runs -- of different lengths, on the same batch -- write the same arrays up to the rounding of
    the atomic reductions (measured: loss and running statistics bit-equal, gradients ~1e-7 relative)."""
    import numpy as np
    d = _run("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["full"] is False and d["steps"] == 3 and d["step_ms_events"]["n"] == 3 and d["dtype"] == "bf16"
    assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["roofline"] is None and d["families"] is None and d["decode"] is None and d["sustained"] is None and "cpu_baseline" not in d
    d2 = _run("--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path / "b"))
    assert d2["steps"] == 5
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bn_state.npy", "grad_norms.npy", "grad_params.npy", "loss.npy", "params.npy"], names
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) < 64 * 2**20
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape and np.isfinite(a).all(), f
        diff = np.abs(a.astype(np.float64) - b)
        assert diff.max() <= 1e-5 * np.abs(a).max() and np.linalg.norm(diff) <= 1e-5 * np.linalg.norm(a), (f, diff.max(), np.abs(a).max())
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    assert a["loss"].shape == (1,) and a["loss"][0] > 0 and a["grad_norms"].size == 10 and a["bn_state"].size == 2560
    assert a["params"].shape == a["grad_params"].shape and 0 < a["params"].size <= 1 << 22     # C3: a fixed sample of the 12.2 M parameters
    assert np.abs(a["grad_params"]).max() > 0
