"""bench.py as a program, on the smallest grid (C1): the plain run's result line, --full's
secondary figures, and --dump-outputs: the files hold the state a fresh engine reaches after
W + K steps, whatever the settle phase ran before them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from regcm_amd.config import STATE_FIELDS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
SECONDARY = ("roofline", "kernel_us", "dropin_ms_per_step", "cpu_baseline")


def run_bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_reports_only_the_headline():
    d = run_bench("--steps", "4", "--warmup", "2")
    for k in HEADLINE:
        assert k in d, k
    assert d["steps"] == 4 and d["warmup"] == 2 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["unit"] == "simulated-years/wall-day"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(150.0 / (365.0 * d["ms_per_step"] * 1e-3), rel=1e-12)
    for k in SECONDARY:
        assert k not in d, k


def test_full_run_adds_the_secondary_figures():
    d = run_bench("--steps", "4", "--warmup", "2", "--full", "--prof-steps", "2", "--cpu-budget", "0.3")
    for k in HEADLINE + SECONDARY:
        assert k in d, k
    assert d["dropin_ms_per_step"] > 0
    assert d["roofline"]["kernel"] in d["kernel_us"]
    assert d["cpu_baseline"]["ms_per_step"] > 0


def test_dumped_outputs_are_the_state_after_the_counted_steps(tmp_path, c1_data):
    from regcm_amd.dycore import DynCore
    import bench
    rc, data = c1_data
    data = bench.hold_boundary({"state": dict(data["state"]), "split": data["split"]})   # as the bench steps it
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    run_bench("--steps", "3", "--warmup", "2", "--dump-outputs", a)                     # settles 100 ms
    run_bench("--steps", "3", "--warmup", "2", "--dump-outputs", b, "--settle-ms", "0")
    ref = DynCore(rc, data["split"])
    ref.put_state(data["state"])
    ref.bdyval()
    ref.step(5)
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n in STATE_FIELDS)
    for name in STATE_FIELDS:
        want = ref.get(name).ravel()
        for d in (a, b):
            got = np.load(os.path.join(d, name + ".npy"))
            assert got.dtype == np.float64
            assert np.array_equal(got, want), (name, d)
