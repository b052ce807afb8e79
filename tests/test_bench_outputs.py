"""bench.py's plain run and its --dump-outputs: the headline alone, and what the last timed step computed as .npy files.

Runs on the MI355X box:  python -m pytest tests -m gpu
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    return torch


def _bench_child(extra, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + extra
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_dumps_the_same_outputs_twice(torch_mod, tmp_path):
    """A plain run (no --full) prints the headline without the legs beside it; --dump-outputs writes the states, QP statistics and
    models of the last timed step in float32 / float64, within 64 MB; two runs with the same arguments write the same arrays."""
    args = ["--gpus", "1", "--config", "cfg2", "--steps", "4", "--warmup", "2", "--settle", "6", "--batch", "512", "--spin-seconds", "0"]
    runs = []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        d = _bench_child(args + ["--dump-outputs", str(out)])
        assert d["steps"] == 4 and d["warmup"] == 2 and d["unit"] == "steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["value"] > 0 and abs(d["value"] - 512 * 4 / (d["ms_per_step"] * 4e-3)) < 1e-6 * d["value"]
        assert "cpu_baseline" not in d and "other_configs" not in d["roofline"] and "replicas" not in d["roofline"]
        assert d["config"]["parity_probe"] is None
        runs.append(_load_dir(str(out)))
    a, b = runs
    assert set(a) == {"x", "qp_status", "newton_solves", "model_A", "model_B", "model_C"}
    assert a["x"].shape == (2, 512) and a["model_A"].shape == (512, 20, 20) and a["model_B"].shape == (512, 20, 1)
    assert a["model_C"].shape == (512, 2, 20) and a["qp_status"].shape == (512,)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.isfinite(a["x"]).all() and (a["qp_status"] == 0).all() and a["newton_solves"].sum() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_of_a_large_output_is_a_fixed_sample(torch_mod, tmp_path, monkeypatch):
    """Above the size limit the dump holds a seeded, sorted sample of the trajectories -- the same rows of every per-trajectory array."""
    torch = torch_mod
    import bench

    c = bench.CONFIGS["cfg2"]
    w = bench.workload_inputs("cfg2", c["L"], c["N"])
    loop = bench.Loop("cfg2", w, 256, torch.float64, torch.device("cuda", 0), 0)
    loop.advance(3, 0)
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 200 << 10)
    shapes = bench.dump_outputs(loop, str(tmp_path / "a"))
    got = _load_dir(str(tmp_path / "a"))
    idx = got["trajectory_index"].astype(np.int64)
    assert 0 < len(idx) < 256 and (np.diff(idx) > 0).all() and idx[-1] < 256
    assert sum(v.nbytes for v in got.values()) <= 200 << 10
    assert shapes["model_A"] == (len(idx), 20, 20) and shapes["x"] == (2, len(idx))
    A, _, _ = loop.m.get_model()
    assert np.array_equal(got["model_A"], A.cpu().numpy()[idx])
    assert np.array_equal(got["x"], loop.X.cpu().numpy()[:, idx])
    bench.dump_outputs(loop, str(tmp_path / "b"))
    assert np.array_equal(_load_dir(str(tmp_path / "b"))["trajectory_index"], got["trajectory_index"])
