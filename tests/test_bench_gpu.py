"""GPU: bench.py's command line on the smallest config (ML-100K, fp32: ~2 s a run).  A plain run times exactly
--steps steps, prints the headline line without the side legs and, with --dump-outputs, writes the last
step's weights and stats as float .npy files that a second run with the same arguments reproduces bit for
bit (seeded data, weights and dropout; deterministic kernels).  --full adds the side legs to the same line."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--config", "ml100k", "--dtype", "float32", "--steps", "7", "--warmup", "3"]
SIDE_LEGS = ("cpu_baseline", "full_epoch", "fp32_parity_mode", "configs")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + list(extra), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(gpu, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump"))
    return _bench("--dump-outputs", d), d


@pytest.mark.gpu
def test_plain_line_and_dump(plain):
    line, d = plain
    assert line["steps"] == 7 and line["warmup"] == 3 and line["unit"] == "ratings/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["masked_rmse"] is None and not any(k in line for k in SIDE_LEGS)
    files = sorted(glob.glob(os.path.join(d, "*.npy")))
    arrs = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert set(arrs) == {"W0", "b0", "W1", "b1", "timed_stats", "last_step_stats"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    # ML-100K I-AutoRec: 943 users in, 500 hidden (under the sampling size: whole kernels, Keras layout)
    assert arrs["W0"].shape == (943, 500) and arrs["W1"].shape == (500, 943)
    assert arrs["b0"].shape == (500,) and arrs["b1"].shape == (943,)
    st = arrs["timed_stats"]
    assert st.shape == (7, 4) and (st[:, 0] > 0).all()                               # one row per timed step
    assert np.array_equal(arrs["last_step_stats"][:4], st[-1])
    assert np.abs(arrs["W0"]).max() > 0 and np.abs(arrs["b1"]).max() > 0             # trained, not the zero biases


@pytest.mark.gpu
def test_dump_repeats_bit_for_bit(plain, tmp_path):
    _, d = plain
    _bench("--dump-outputs", str(tmp_path))
    for f in sorted(glob.glob(os.path.join(d, "*.npy"))):
        assert np.array_equal(np.load(f), np.load(str(tmp_path / os.path.basename(f)))), os.path.basename(f)


@pytest.mark.gpu
def test_full_adds_the_side_legs(plain):
    line = _bench("--full")
    assert line["steps"] == 7 and line["masked_rmse"] > 0
    assert "error" not in line["cpu_baseline"] and line["cpu_baseline"]["value"] > 0
    assert line["full_epoch"]["train_py"]["batches"] > 0
    assert set(plain[0]) - {"masked_rmse"} <= set(line)
