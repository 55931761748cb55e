"""`python bench.py --gpus N` must start its own ranks (the driver runs it without a launcher):
N fresh child processes, spawned before the parent touches the GPU; rank 0's JSON line relayed;
non-zero exit when a rank fails."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMD = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--same-device",
       "--batch", "4", "--steps", "8", "--warmup", "0", "--no-cpu-baseline", "--no-prof"]


def _env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_launcher_spawns_ranks_and_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-container check")
    r = subprocess.run(CMD, env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert r.stderr.count("needs a HIP device") == 2  # both ranks started, both refused a CPU run
    assert "ranks failed" in r.stderr


@pytest.mark.gpu
def test_launcher_two_ranks_on_one_gpu_prints_one_json_line():
    r = subprocess.run(CMD, env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 8 and out["config"]["global_batch"] == 8
    assert out["value"] > 0 and out["scaling"] == "weak"


PLAIN = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "4", "--steps", "5", "--warmup", "2"]


def test_dump_shapes_needs_full():
    r = subprocess.run(PLAIN + ["--dump-shapes", os.devnull], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "needs --full" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain run prints the contract's line for exactly --steps timed steps and nothing that --full adds; --dump-outputs
    writes the last timed step's scalars and the weights after it as float32 .npy files (64 MB at most), the same files
    with the same values from a second run with the same arguments."""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        r = subprocess.run(PLAIN + ["--dump-outputs", str(d)], env=_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        out = json.loads(lines[0])
        assert out["steps"] == 5 and out["warmup"] == 2 and out["n_gpus"] == 1
        assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "seq/s" and out["higher_is_better"] is True
        assert out["dtype"] == "f32" and out["metric"].startswith("120-frame seq/sec, phase3")
        assert not {"roofline", "cpu_baseline", "parity_at_bench_size", "other_configs"} & set(out)
        files = sorted(os.listdir(d))
        assert "step.loss_critic.npy" in files and any(f.startswith("gen.") for f in files)
        assert any(f.startswith("critic.") for f in files)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 * 10 ** 6
        arrays = {f: np.load(os.path.join(d, f)) for f in files}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert float(arrays["step.loss_critic.npy"]) == pytest.approx(out["losses_last_step"]["loss_critic"], rel=1e-6)
        dumps.append(arrays)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for f, a in dumps[0].items():
        np.testing.assert_allclose(dumps[1][f], a, rtol=1e-3, atol=1e-4, err_msg=f)


@pytest.mark.gpu
def test_full_run_adds_the_roofline_pass():
    r = subprocess.run(PLAIN + ["--full", "--no-cpu-baseline"], env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 5 and out["roofline"]["achieved"] > 0 and "plain_gemm_4096_tflops" in out["roofline"]
