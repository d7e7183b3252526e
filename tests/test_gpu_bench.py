"""bench.py's single-GPU line: a plain run is the headline alone (setup, warm-up, the timed steps, the line), --full adds the
secondary measurements, and --dump-outputs writes what the timed call returned, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


SECONDARY = ("cpu_baseline", "jacobi", "strict_arithmetic", "value_strict", "sizes", "minmax", "fast_valid_sweeps")


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_same_outputs_every_time(tmp_path):
    n, K, W = 64, 5, 2
    d = _bench("--size", str(n), "--steps", str(K), "--warmup", str(W), "--arith", "strict", "--dump-outputs", str(tmp_path / "a"))
    assert d["steps"] == K and d["warmup"] == W and d["n_gpus"] == 1 and d["dtype"] == "f64"
    assert d["unit"] == "cell-updates/s" and d["higher_is_better"] is True and "64^3 fp64" in d["metric"]
    cells = K * (n - 2.0) ** 3
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 * K - cells) < 1e-6 * cells  # ms_per_step = one of the K timed steps
    assert not [k for k in SECONDARY if k in d]
    assert d["roofline"]["peak_measured"] is None  # the copy-bandwidth run belongs to --full

    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["phi_plane_zmid", "phi_sample", "phi_sample_index", "rms"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) < 64 << 20
    assert np.array_equal(a["phi_sample_index"], np.arange(n ** 3, dtype=np.float64))  # a small field is written whole
    k = n // 2
    assert np.array_equal(a["phi_plane_zmid"], a["phi_sample"][k * n * n:(k + 1) * n * n].reshape(n, n))
    assert a["rms"].shape == (K,) and np.all(a["rms"] > 0)

    _bench("--size", str(n), "--steps", str(K), "--warmup", str(W), "--arith", "strict", "--dump-outputs", str(tmp_path / "b"))
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert np.array_equal(a["phi_sample"], b["phi_sample"]) and np.array_equal(a["phi_plane_zmid"], b["phi_plane_zmid"])
    assert np.allclose(a["rms"], b["rms"], rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_full_run_adds_the_secondary_measurements():
    d = _bench("--size", "64", "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline")
    assert d["steps"] == 4 and d["ms_per_step"] > 0
    assert d["jacobi"]["value"] > 0 and d["strict_arithmetic"]["gs"]["value"] > 0 and d["value_strict"] > 0
    assert d["minmax"]["gs"]["ms_per_iteration"] > 0 and d["fast_valid_sweeps"]["this_run"]["signs_equal"] is True
    assert d["roofline"]["peak_measured"] > 0


def test_dump_outputs_refuses_multi_gpu_runs_before_any_work():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs", "unused"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "single-GPU runs only" in r.stderr
