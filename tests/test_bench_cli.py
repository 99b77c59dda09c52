"""bench.py's command line: a plain run measures the headline alone, ``--full`` adds the runs of
their own, ``--dump-outputs DIR`` writes the last timed step's outputs as float64 ``.npy``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float64_and_caps_the_size(tmp_path, monkeypatch):
    import bench
    arrays = dict(a=np.arange(6, dtype=np.int32).reshape(2, 3), b=np.linspace(0.0, 1.0, 5, dtype=np.float32))
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "whole" / f"{k}.npy")
        assert got.dtype == np.float64 and got.shape == v.shape
        np.testing.assert_array_equal(got, v.astype(np.float64))
    # over the cap: a sample of the flattened entries, the same on every call
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 800)
    big = dict(a=np.arange(200.0), b=np.arange(60.0).reshape(30, 2))
    bench.dump_outputs(str(tmp_path / "s1"), big)
    bench.dump_outputs(str(tmp_path / "s2"), big)
    total = 0
    for k, v in big.items():
        s1, s2 = np.load(tmp_path / "s1" / f"{k}.npy"), np.load(tmp_path / "s2" / f"{k}.npy")
        np.testing.assert_array_equal(s1, s2)
        assert s1.ndim == 1 and 0 < s1.size < v.size and np.all(np.isin(s1, v)) and np.all(np.diff(s1) > 0)
        total += s1.nbytes
    assert total <= 800


@pytest.mark.gpu
def test_plain_run_times_the_given_steps_and_dumps_its_outputs(tmp_path):
    """A plain run: one JSON line whose steps and ms_per_step belong to the timed steps, none of
    the --full measurements, and the dump of the last step's outputs."""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "outer_iters/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    # fixed 100 outer iterations per step: value and ms_per_step describe the same 3 steps
    assert d["config"]["outer_iters_per_step"] == 100
    assert d["value"] == pytest.approx(100 * 1e3 / d["ms_per_step"], rel=1e-9)
    assert d["cpu_baseline"] is None and "natural" not in d and "cold_first_step" not in d
    shapes = dict(xt=(256, 3), u=(256, 30), iters=(128,), global_resid=(100, 2), global_iters=(1,))
    assert sorted(os.listdir(out)) == sorted(f"{k}.npy" for k in shapes)
    for k, shape in shapes.items():
        a = np.load(out / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == shape and np.all(np.isfinite(a))
    assert np.all(np.load(out / "iters.npy") == 100) and np.load(out / "global_iters.npy")[0] == 100
