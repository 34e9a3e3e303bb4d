"""bench.py's plain run and `--dump-outputs`: the row sample on CPU tensors, and one small plain run on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_and_a_fixed_row_sample(tmp_path):
    import bench
    rows = bench.DUMP_ROWS + 1000
    big = torch.arange(rows * 3, dtype=torch.float32).reshape(rows, 3)
    state = torch.arange(5 * rows, dtype=torch.float32).reshape(5, rows)  # channel-major, dumped as its transpose
    arrays = dict(big=big, small=torch.arange(7, dtype=torch.long), flags=torch.tensor([True, False]), state=state.t())
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["big", "flags", "small", "state"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["small"], np.arange(7)) and np.array_equal(got["flags"], [1.0, 0.0])
    assert got["big"].shape == (bench.DUMP_ROWS, 3) and got["state"].shape == (bench.DUMP_ROWS, 5)
    idx = (got["big"][:, 0] / 3).astype(np.int64)  # the sampled rows: distinct, ascending, rows of the input
    assert np.all(np.diff(idx) > 0) and np.array_equal(got["big"], big.numpy()[idx])
    assert np.array_equal(got["state"], state.numpy().T[idx])  # every array of one length gets the same rows
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    assert sum(v.nbytes for v in got.values()) < 64 * 2 ** 20


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """A plain run: the headline fields and `ms_per_step`, none of the `--full` legs, and the last timed
    step's outputs as float32 arrays (all rows at 512 fields)."""
    n, steps = 512, 7
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--fields", str(n), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["steps"] == steps and j["unit"] == "env-steps/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] > 0 and abs(j["value"] - n * steps / (j["ms_per_step"] * 1e-3 * steps)) / j["value"] < 1e-6
    for leg in ("past_l3", "rollout", "sa_step", "ppo", "ppo_dma", "cpu_baseline"):
        assert leg not in j
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) == {"obs", "terminal_obs", "rew", "time_outs", "progress_f", "dones", "progress", "state"}
    assert all(v.dtype == np.float32 and v.shape[0] == n and np.isfinite(v).all() for v in got.values())
    assert got["obs"].shape == (n, 2, 3, 52) and got["rew"].shape == (n, 2, 3, 4) and np.any(got["obs"] != 0)
    # 9 steps from the construction reset: no field's episode is longer than that, and most are that long
    assert 0 < got["progress"].max() <= 9 and np.median(got["progress"]) == got["progress"].max()
