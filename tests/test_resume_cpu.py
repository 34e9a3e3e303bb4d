"""--checkpoint-every / --resume without a GPU: the command line, the state file's format (vss_amd/checkpoint.py:
round trip, weights_only load, atomic write, format version), the compatibility rules, and the owners'
load_state_dict checks as far as they run on CPU tensors."""
import argparse
import math
import os
import random

import numpy as np
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from vss_amd import checkpoint as CK
from vss_amd.flat import FlatAdam
from vss_amd.opponent import OpponentPool


def test_parse_args_defaults_leave_both_off():
    args = P.parse_args([])
    assert args.checkpoint_every == 0
    assert args.resume is None
    args = P.parse_args(["--checkpoint-every", "5", "--resume", "x/state.pt"])
    assert args.checkpoint_every == 5 and args.resume == "x/state.pt"


def test_check_compatible_accepts_equal_args():
    args = P.parse_args(["--env-id", "cma", "--num-envs", "256"])
    assert CK.check_compatible(CK.plain_args(args), args, log=None) == []


STRUCTURAL_CHANGES = {
    "env_id": ["--env-id", "cma"], "num_envs": ["--num-envs", "512"], "num_steps": ["--num-steps", "16"],
    "seed": ["--seed", "2"], "opponent": ["--opponent", "self"], "opponent_pool_slots": ["--opponent-pool-slots", "4"],
    "opponent_pool_size": ["--opponent-pool-size", "2"], "fused_policy": ["--fused-policy", "false"],
    "amp": ["--amp", "bf16"], "cuda": ["--cuda", "false"],
}


def test_the_structural_keys_are_the_documented_ones():
    assert sorted(CK.STRUCTURAL) == sorted(STRUCTURAL_CHANGES)


@pytest.mark.parametrize("key", list(STRUCTURAL_CHANGES))
def test_check_compatible_refuses_a_structural_change_naming_the_key(key):
    saved = CK.plain_args(P.parse_args([]))
    new = P.parse_args(STRUCTURAL_CHANGES[key])
    with pytest.raises(ValueError, match=key) as e:
        CK.check_compatible(saved, new, log=None)
    assert repr(saved[key]) in str(e.value) and repr(getattr(new, key)) in str(e.value)  # both values


def test_the_opponent_is_compared_by_mode_not_by_path():
    saved = CK.plain_args(P.parse_args(["--opponent", "runs/a/agent.pt"]))
    assert "opponent" in CK.check_compatible(saved, P.parse_args(["--opponent", "elsewhere/agent.pt"]), log=None)
    with pytest.raises(ValueError, match="opponent"):
        CK.check_compatible(saved, P.parse_args(["--opponent", "pool"]), log=None)


def test_check_compatible_takes_other_hyperparameters_from_the_new_line_and_reports_each_once():
    saved = CK.plain_args(P.parse_args([]))
    lines = []
    changed = CK.check_compatible(saved, P.parse_args(["--learning-rate", "0.0003", "--num-updates", "9"]), log=lines.append)
    assert changed == ["learning_rate", "num_updates"]
    assert len(lines) == 2 and "learning_rate" in lines[0] and "0.001" in lines[0] and "0.0003" in lines[0]


def sample_state():
    random.seed(11)
    np.random.seed(12)
    np.random.standard_normal(3)  # an odd count: the cached gaussian is part of the state
    return {"f": torch.arange(6, dtype=torch.float32).reshape(2, 3) / 7, "l": torch.tensor([2 ** 40, -1]),
            "i": torch.tensor([1, -2, 3], dtype=torch.int32), "b": torch.tensor([True, False]),
            "nested": [[1, 2.5, "x"], [None, [True]]], "nan": math.nan, "history": [{"winrate": [math.nan, 0.25]}],
            "python": CK.python_rng_state(), "numpy": CK.numpy_rng_state(), "source_hash": "abc"}


def test_save_state_load_state_round_trip(tmp_path):
    state = sample_state()
    py_next, np_next = random.random(), np.random.standard_normal(2)
    path = str(tmp_path / "sub" / "run-state.pt")  # the directory is created
    size = CK.save_state(path, state)
    assert size == os.path.getsize(path)
    assert torch.load(path, map_location="cpu", weights_only=True)["format_version"] == CK.FORMAT_VERSION
    back = CK.load_state(path)
    assert back["format_version"] == CK.FORMAT_VERSION and back["source_hash"] == "abc"
    for k in ("f", "l", "i", "b"):
        assert back[k].dtype == state[k].dtype and torch.equal(back[k], state[k])
    assert back["nested"] == state["nested"]
    assert math.isnan(back["nan"]) and math.isnan(back["history"][0]["winrate"][0]) and back["history"][0]["winrate"][1] == 0.25
    random.seed(0)
    np.random.seed(0)
    random.setstate(CK.python_rng_tuple(back["python"]))
    np.random.set_state(CK.numpy_rng_tuple(back["numpy"]))
    assert random.random() == py_next
    assert np.array_equal(np.random.standard_normal(2), np_next)


def test_save_state_stamps_the_library_source_hash(tmp_path):
    path = str(tmp_path / "s.pt")
    CK.save_state(path, {"x": 1})
    assert CK.load_state(path)["source_hash"] == CK.source_hash() != ""


def test_a_foreign_format_version_is_refused(tmp_path):
    path = str(tmp_path / "s.pt")
    torch.save({"format_version": CK.FORMAT_VERSION + 1, "x": 1}, path)
    with pytest.raises(ValueError, match="format version"):
        CK.load_state(path)
    torch.save({"x": 1}, path)
    with pytest.raises(ValueError, match="format version"):
        CK.load_state(path)


def test_a_failed_write_leaves_the_previous_file_and_no_temporary(tmp_path, monkeypatch):
    path = str(tmp_path / "run-state.pt")
    CK.save_state(path, {"x": 1, "source_hash": "h"})
    before = open(path, "rb").read()

    def failing(obj, f):
        f.write(b"half a file")
        raise OSError("disk full")

    monkeypatch.setattr(CK, "_write", failing)
    with pytest.raises(OSError, match="disk full"):
        CK.save_state(path, {"x": 2, "source_hash": "h"})
    assert open(path, "rb").read() == before
    assert os.listdir(tmp_path) == ["run-state.pt"]


def test_copy_into_checks_shape_and_dtype_and_keeps_the_tensor():
    dst = torch.zeros(2, 3)
    view = dst[1]
    CK.copy_into(dst, torch.ones(2, 3), "t")
    assert view.tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="owner.t"):
        CK.copy_into(dst, torch.ones(3, 2), "owner.t")
    with pytest.raises(ValueError, match="owner.t"):
        CK.copy_into(dst, torch.ones(2, 3, dtype=torch.float64), "owner.t")
    with pytest.raises(ValueError, match="'missing'"):
        CK.copy_entries("owner", {"missing": dst}, {})


def cpu_adam(n=8):
    """A FlatAdam's state without its device: load_state_dict touches only these."""
    opt = FlatAdam.__new__(FlatAdam)
    opt.exp_avg, opt.exp_avg_sq, opt.steps = torch.zeros(n), torch.zeros(n), 0
    opt.param_groups = [{"lr": 1e-3}]
    return opt


def test_flat_adam_state_round_trip_and_shape_check():
    a, b = cpu_adam(), cpu_adam()
    a.exp_avg += 1.5
    a.exp_avg_sq += 0.25
    a.steps, a.param_groups[0]["lr"] = 7, 4e-4
    moments = (b.exp_avg, b.exp_avg_sq)
    b.load_state_dict(a.state_dict())
    assert b.exp_avg is moments[0] and b.exp_avg_sq is moments[1]
    assert torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq)
    assert b.steps == 7 and b.param_groups[0]["lr"] == 4e-4
    with pytest.raises(ValueError, match="FlatAdam.exp_avg"):
        cpu_adam(16).load_state_dict(a.state_dict())


def test_opponent_pool_refuses_a_state_that_does_not_fit_before_touching_a_device():
    pool = OpponentPool.__new__(OpponentPool)
    pool.capacity, pool.count, pool.snapshots = 2, 4, []
    pool.tally = torch.zeros((4, 4), dtype=torch.long)
    snap = {"actor": {}, "version": 0, "totals": [0, 0, 0, 0]}
    good = {"snapshots": [snap, snap], "slots": [1, 1, 0, 1], "counter": 3, "rng": CK.python_rng_state(),
            "tally": torch.zeros((4, 4), dtype=torch.long)}
    with pytest.raises(ValueError, match="OpponentPool.snapshots"):
        pool.load_state_dict(dict(good, snapshots=[snap] * 3))  # more than the capacity
    with pytest.raises(ValueError, match="OpponentPool.slots"):
        pool.load_state_dict(dict(good, slots=[0, 1]))  # another slot count
    with pytest.raises(ValueError, match="OpponentPool.slots"):
        pool.load_state_dict(dict(good, slots=[0, 1, 2, 0]))  # an index past the list
    with pytest.raises(ValueError, match="OpponentPool.tally"):
        pool.load_state_dict(dict(good, tally=torch.zeros((2, 4), dtype=torch.long)))
    with pytest.raises(ValueError, match="'counter'|'snapshots'"):
        pool.load_state_dict({k: v for k, v in good.items() if k != "snapshots"})


def test_world_size_above_one_is_refused_before_any_process_group(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(dist, "init_process_group", lambda *a, **k: pytest.fail("a process group was created"))
    for extra in (["--checkpoint-every", "1"], ["--resume", "nowhere/state.pt"]):
        with pytest.raises(ValueError, match="per-rank state files are not built"):
            P.train(P.parse_args(["--log", "false", "--kernel-warmup", "false"] + extra))


def test_warmup_args_neither_resume_nor_write(monkeypatch):
    from vss_amd import minibatch as MB
    seen = []
    args = P.parse_args(["--checkpoint-every", "2", "--resume", "x/state.pt"])
    MB.warmup_kernels(args, lambda w: seen.append(argparse.Namespace(**vars(w))))
    assert seen[0].checkpoint_every == 0 and seen[0].resume is None
    assert args.checkpoint_every == 2 and args.resume == "x/state.pt"
