"""bench.py's command line: the plain run measures the headline figure only, --full adds the extra records, and
--dump-outputs writes the Φ values the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

TOL = 1e-8          # as test_gpu_parity.py


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_cli", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float64_values(tmp_path):
    import torch
    bench = _bench_module()
    v = torch.linspace(-1.0, 1.0, 1000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "out"), v)
    assert sorted(os.listdir(tmp_path / "out")) == ["phi_values.npy"]
    got = np.load(tmp_path / "out" / "phi_values.npy")
    assert got.dtype == np.float64 and np.array_equal(got, v.numpy())


def test_dump_outputs_samples_beyond_the_size_cap(tmp_path, monkeypatch):
    """Above the cap: a fixed sample (the same positions on every run) and its positions, both files within the cap."""
    import torch
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 4096 + 8 * 400)
    v = torch.arange(5000, dtype=torch.float64) * 0.5
    outs = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        bench.dump_outputs(str(d), v)
        assert sorted(os.listdir(d)) == ["phi_values.npy", "phi_values_index.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= bench.DUMP_MAX_BYTES
        vals, idx = np.load(d / "phi_values.npy"), np.load(d / "phi_values_index.npy")
        assert vals.dtype == np.float64 and idx.dtype == np.float64 and len(vals) == len(idx) == 200
        assert np.all(np.diff(idx) > 0) and np.array_equal(vals, v.numpy()[idx.astype(np.int64)])
        outs.append(idx)
    assert np.array_equal(outs[0], outs[1])


def test_bench_rejects_a_step_count_below_one():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_bench_run_counts_its_steps_and_dumps_phi(tmp_path):
    """A plain run times exactly --steps steps, carries none of the --full records, and the dumped Φ of its last step is the
    golden README-chain vector."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 7 and d["roofline"]["kernel_launches"] == 7 and d["ms_per_step"] > 0
    assert d["config"]["unsolved_total"] == 0
    assert "cpu_baseline" not in d and "strong" not in d and d["config"]["oneshot_call"] is None
    g = np.load(os.path.join(GOLDEN, "readme_chain_phi.npz"))
    want = np.concatenate([g["vals_x"], g["vals_u"]])
    got = np.load(out / "phi_values.npy")
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() < TOL
