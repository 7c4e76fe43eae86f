"""bench.py on the GPU, small: a plain run (`--gpus 1 --steps N --warmup W`)
prints the headline line and none of --full's measurements, and
`--dump-outputs DIR` writes what the last of the W + N steps left with its
caller: the same arrays, bit for bit, as the same trainer stepped W + N times
in this process.  A small `--full` run still reports every companion."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, REPLAY, STEPS, WARMUP, K = 2048, 65536, 4, 2, 2
FULL_ONLY = ("k_sweep", "seeds_per_gpu", "seeds_per_gpu_processes", "variants", "fp32_companion", "roofline",
             "roofline_fused_kernel", "roofline_mfma", "cpu_baseline")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--lanes", str(LANES), "--replay", str(REPLAY), "--k-updates", str(K),
                        *extra], capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_full_run_keeps_the_companion_measurements(dev):
    """--full at a small size, one entry per companion: every measurement that
    moved behind the option is still made and reported."""
    line = _bench("--full", "--no-cpu-baseline", "--k-sweep", "1,2", "--seeds-per-gpu", "2", "--seed-streams", "pool",
                  "--seed-procs", "1,2", "--event-stride", "1")
    assert line["full"] is True and line["steps"] == STEPS
    assert line["value"] == pytest.approx(LANES * 1e3 / line["ms_per_step"], rel=1e-9)
    assert sorted(line["k_sweep"]) == ["1", "2"] and all(v["ms_per_step"] > 0 for v in line["k_sweep"].values())
    assert line["seeds_per_gpu"]["streams"] == "pool" and line["seeds_per_gpu"]["2"]["env_steps_per_s"] > 0
    assert {"1", "2"} <= set(line["seeds_per_gpu_processes"])
    assert len(line["seeds_per_gpu_processes"]["2"]["per_seed_ms_per_step"]) == 2
    assert line["fp32_companion"]["dtype"] == "fp32" and line["fp32_companion"]["ms_per_step"] > 0
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["achieved"] > 0
    assert line["roofline_mfma"]["achieved"] > 0 and line["cpu_baseline"] is None
    assert set(line["config"]["phase_ms_per_step"]) == {"act", "env_kernel", "learn_k"}


def test_plain_run_line_and_dumped_outputs(dev, tmp_path):
    out_dir = tmp_path / "dump"
    line = _bench("--dump-outputs", str(out_dir))
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
    assert line["unit"] == "env steps/sec" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(LANES * 1e3 / line["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    assert "phase_ms_per_step" not in line["config"]

    import bench

    args = argparse.Namespace(config="c2", lanes=LANES, replay=REPLAY, loss="MSE", k_updates=K, precision="bf16",
                              slice_groups=1)
    tr = bench.make_trainer(args, dev, 420)
    for _ in range(WARMUP + STEPS):
        tr.step()
    want = bench.last_step_outputs(tr)
    assert sorted(line["dumped_outputs"]["shapes"]) == sorted(want)
    total = 0
    for name, w in want.items():
        got = np.load(out_dir / f"{name}.npy")
        assert got.dtype in (np.float32, np.float64) and got.dtype == w.dtype, name
        assert np.isfinite(got).all(), name  # the rows' NaN placeholder slots are not written
        assert got.shape == w.shape and np.array_equal(got, w), name
        total += got.nbytes
    assert total <= bench.DUMP_CAP_BYTES
    assert want["obs"].shape == (LANES, 5) and want["learn_stats"].shape == (K, 14)
