"""--checkpoint-every / --resume on the GPU: a run resumed from its state file trains the same bits as the run that
was never interrupted -- agent parameters, Adam moments, env state, Philox counters, a league's snapshots and
totals, per-update history -- in every configuration whose state differs.

Run A trains N updates and writes its state every K-th; the state after update K is copied aside from on_update.
Run B resumes that copy up to N, writing its own state at N.  The two final state files are then compared entry
by entry, bit for bit (what they hold is everything the next update would depend on), beside the returned
parameters and the history's non-timing keys."""
import math
import os
import shutil
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from vss_amd import checkpoint as CK

pytestmark = pytest.mark.gpu
KEYS = ("v_loss", "pg_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "mean_return", "episodes",
        "opponent_version")  # tests/test_gae_train.py's
MIRROR_KEYS = KEYS + ("mean_return_blue", "mean_return_yellow")
POOL_KEYS = KEYS + ("opponent_pool_versions", "opponent_pool_winrate")
COMMON = ["--kernel-warmup", "false", "--log", "false"]
SA = ["--env-id", "sa", "--num-envs", "256", "--num-steps", "8"]
RUN = "ppo_continuous_action_isaacgym_ppo-{env_id}_1"


def same_value(a, b):
    """Equality of history values: NaN equals NaN, lists element by element."""
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a):
        return math.isnan(b)
    return type(a) is type(b) and a == b


def records(hist, keys):
    return [{k: h[k] for k in keys} for h in hist]


def assert_records_equal(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert same_value(x[k], y[k]), f"record {i} {k}: {x[k]!r} != {y[k]!r}"


def assert_bits_equal(a, b, where="state"):
    """Two trees of a state file: the same structure, every tensor the same dtype, shape and bytes."""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape, where
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{where} differs"
    elif isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for k in a:
            assert_bits_equal(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            assert_bits_equal(x, y, f"{where}[{i}]")
    else:
        assert same_value(a, b), f"{where}: {a!r} != {b!r}"


def assert_states_equal(a, b):
    """Everything but the clocks and the command line (the two runs write to different directories)."""
    for k in ("agent", "owners", "rng", "update", "global_step", "format_version", "source_hash"):
        assert_bits_equal(a[k], b[k], k)


Result = namedtuple("Result", "params agent_state hist state_path aside folder")


def train(argv, save_path, copy_at=None):
    """One train(): the parameters, the history, the run's state file, and a copy of it as update `copy_at` wrote it."""
    args = P.parse_args(argv + COMMON + ["--save-path", str(save_path)])
    folder = os.path.join(str(save_path), RUN.format(env_id=args.env_id))
    state_path = os.path.join(folder, RUN.format(env_id=args.env_id) + "-state.pt")
    aside = os.path.join(str(save_path), f"state-after-{copy_at}.pt")

    def on_update(rec, agent):
        if rec["update"] == copy_at:
            shutil.copyfile(state_path, aside)  # the checkpoint is written before on_update

    agent, hist = P.train(args, on_update=on_update if copy_at is not None else None)
    return Result([p.detach().clone() for p in agent.parameters()],
                  {k: v.detach().clone() for k, v in agent.state_dict().items()}, hist, state_path,
                  aside if copy_at is not None else None, folder)


def assert_params_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def interrupted_and_unbroken(argv, tmp_path, updates=4, at=2):
    a = train(argv + ["--num-updates", str(updates), "--checkpoint-every", str(at)], tmp_path / "a", copy_at=at)
    b = train(argv + ["--num-updates", str(updates), "--checkpoint-every", str(at), "--resume", a.aside], tmp_path / "b")
    return a, b


def assert_resumed_equals_unbroken(a, b, keys, updates=4, at=2):
    assert_params_equal(a.params, b.params)
    sa, sb, mid = CK.load_state(a.state_path), CK.load_state(b.state_path), CK.load_state(a.aside)
    assert sa["update"] == sb["update"] == updates and mid["update"] == at
    opt_a, opt_b = sa["owners"]["optimizer"], sb["owners"]["optimizer"]
    assert opt_a["steps"] == opt_b["steps"] > mid["owners"]["optimizer"]["steps"] > 0
    for k in ("exp_avg", "exp_avg_sq"):
        assert_bits_equal(opt_a[k], opt_b[k], f"optimizer.{k}")
    for k in ("state", "rng_counter", "progress_buf"):
        assert_bits_equal(sa["owners"]["env"][k], sb["owners"]["env"][k], f"env.{k}")
    assert_states_equal(sa, sb)  # and every other entry
    assert [h["update"] for h in b.hist] == list(range(1, updates + 1))
    assert_records_equal(records(b.hist[at:], keys), records(a.hist[at:], keys))  # the updates B trained
    assert_records_equal(records(b.hist[:at], keys), records(mid["history"], keys))  # the saved ones
    assert_records_equal(records(b.hist[:at], keys), records(a.hist[:at], keys))
    assert b.hist[at]["global_step"] == a.hist[at]["global_step"] and b.hist[at]["wall_s"] > mid["wall_s"]
    return sa, sb, mid


CASES = {
    "sa": (SA, KEYS),
    "sa-torch-policy": (SA + ["--fused-policy", "false"], KEYS),
    "cma": (["--env-id", "cma", "--num-envs", "256", "--num-steps", "8"], KEYS),
    "dma-mirror": (["--env-id", "dma", "--num-envs", "258", "--num-steps", "8", "--opponent", "mirror"], MIRROR_KEYS),
    "sa-self-older-snapshot": (SA + ["--opponent", "self", "--opponent-update-every", "3"], KEYS),
    "sa-adaptative-lr": (SA + ["--adaptative-lr"], KEYS),
    "sa-anneal-lr": (SA + ["--anneal-lr"], KEYS),
    "sa-target-kl": (SA + ["--target-kl", "0.0001"], KEYS),
}


@pytest.fixture(scope="module")
def sa_runs(tmp_path_factory):
    """The plain SA case's two runs, shared with the tests that only need a state file and run A's result."""
    tmp = tmp_path_factory.mktemp("sa")
    return interrupted_and_unbroken(SA, tmp) + (tmp,)


@pytest.mark.parametrize("case", list(CASES))
def test_resumed_run_equals_the_unbroken_run(case, tmp_path, sa_runs):
    argv, keys = CASES[case]
    a, b = sa_runs[:2] if case == "sa" else interrupted_and_unbroken(argv, tmp_path)
    sa, sb, mid = assert_resumed_equals_unbroken(a, b, keys)
    if case == "sa-self-older-snapshot":  # update 3 refreshed the snapshot; the checkpoint carried update 0's
        assert mid["owners"]["opponent"]["version"] == 0 and sb["owners"]["opponent"]["version"] == 3
    if case == "sa-adaptative-lr":  # the learning rate moved, and it is the moved one that was carried
        assert mid["owners"]["optimizer"]["lr"] != 0.001
    if case == "sa-target-kl":  # epochs broke early: the generator's consumption differs per update
        assert any(h["epochs_run"] < 8 for h in a.hist)
        assert [h["epochs_run"] for h in a.hist] == [h["epochs_run"] for h in b.hist]
    if case == "sa":  # both files of every K-th update, nothing else left in the run's directory
        run = RUN.format(env_id="sa")
        assert sorted(os.listdir(a.folder)) == [f"{run}-agent-u000002.pt", f"{run}-agent-u000004.pt", f"{run}-state.pt"]
        assert all(h["checkpoint_s"] > 0 for h in a.hist[1::2]) and all(h["checkpoint_s"] == 0.0 for h in a.hist[0::2])


def test_resumed_league_equals_the_unbroken_one(tmp_path):
    """--opponent pool with 4 slots and 2 snapshots kept: at the checkpoint a snapshot has already been evicted."""
    argv = ["--env-id", "sa", "--num-envs", "512", "--num-steps", "8", "--opponent", "pool", "--opponent-pool-slots", "4",
            "--opponent-pool-size", "2"]
    a, b = interrupted_and_unbroken(argv, tmp_path)
    sa, sb, mid = assert_resumed_equals_unbroken(a, b, POOL_KEYS)
    pa, pb, pm = (s["owners"]["opponent"] for s in (sa, sb, mid))
    assert [s["version"] for s in pm["snapshots"]] == [1, 2]  # update 0's snapshot has left
    assert [s["version"] for s in pa["snapshots"]] == [s["version"] for s in pb["snapshots"]] == [3, 4]
    assert len(pa["slots"]) == 4 and pa["slots"] == pb["slots"]
    assert [pa["snapshots"][i]["version"] for i in pa["slots"]] == [pb["snapshots"][i]["version"] for i in pb["slots"]]
    assert [s["totals"] for s in pa["snapshots"]] == [s["totals"] for s in pb["snapshots"]]
    assert pa["counter"] == pb["counter"] == 4 * 8 and pa["rng"] == pb["rng"]


def test_resumed_chain_rollout_equals_the_unbroken_one(tmp_path):
    """16,384 rows: the GEMM-chain rollout policy and its sampling tail; checkpoint and resume at update 1."""
    argv = ["--env-id", "sa", "--num-envs", "16384", "--num-steps", "4"]
    a, b = interrupted_and_unbroken(argv, tmp_path, updates=2, at=1)
    assert_resumed_equals_unbroken(a, b, KEYS, updates=2, at=1)


def test_writing_checkpoints_does_not_perturb_the_run(tmp_path):
    argv = SA + ["--num-updates", "3"]
    plain = train(argv, tmp_path / "plain")
    saving = train(argv + ["--checkpoint-every", "1"], tmp_path / "saving")
    assert not os.path.exists(plain.folder)  # the flag off writes nothing
    assert_params_equal(plain.params, saving.params)
    assert_records_equal(records(plain.hist, KEYS), records(saving.hist, KEYS))
    assert all(h["checkpoint_s"] == 0.0 for h in plain.hist) and all(h["checkpoint_s"] > 0.0 for h in saving.hist)
    for h in saving.hist:  # part of the wall clock, outside the two stage clocks
        assert h["wall_s"] >= h["rollout_s"] + h["update_s"] + h["checkpoint_s"]


def test_resume_in_a_fresh_process_writes_the_unbroken_runs_agent(sa_runs):
    a, _, tmp = sa_runs
    script = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "ppo_continuous_action_isaacgym.py")
    out = subprocess.run([sys.executable, script] + SA + ["--num-updates", "4", "--kernel-warmup", "false", "--log", "true",
                                                           "--save-path", str(tmp / "child"), "--resume", a.aside],
                         timeout=600, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    run = RUN.format(env_id="sa")
    final = torch.load(str(tmp / "child" / run / f"{run}-agent.pt"), map_location="cpu", weights_only=True)
    assert final.keys() == a.agent_state.keys()
    for k, v in final.items():
        assert torch.equal(v.view(torch.int32), a.agent_state[k].cpu().view(torch.int32)), k


def test_resume_at_the_end_runs_no_update_and_returns_the_saved_agent(sa_runs, tmp_path):
    a = sa_runs[0]
    r = train(SA + ["--num-updates", "2", "--resume", a.aside], tmp_path)
    mid = CK.load_state(a.aside)
    assert [h["update"] for h in r.hist] == [1, 2]
    assert_records_equal(records(r.hist, KEYS), records(a.hist[:2], KEYS))
    assert r.agent_state.keys() == mid["agent"].keys()
    for k, v in r.agent_state.items():
        assert torch.equal(v.cpu().view(torch.int32), mid["agent"][k].view(torch.int32)), k


def test_the_agent_file_is_the_reference_format(sa_runs):
    from envs._gym import Box
    from vss_amd.opponent import SnapshotOpponent
    a = sa_runs[0]
    path = os.path.join(a.folder, RUN.format(env_id="sa") + "-agent-u000002.pt")
    Env = namedtuple("Env", ["single_observation_space", "single_action_space"])
    agent = P.Agent(Env(Box(-np.inf, np.inf, (52,)), Box(-1.0, 1.0, (2,)))).cuda()
    agent.load_state_dict(torch.load(path, map_location="cuda", weights_only=True), strict=True)
    mid = CK.load_state(a.aside)
    for k, v in agent.state_dict().items():
        assert torch.equal(v.cpu().view(torch.int32), mid["agent"][k].view(torch.int32)), k
    opp = SnapshotOpponent(agent, "x3", seed=3).load(path, version=2)
    assert opp.version == 2
    assert torch.equal(opp.actor.actor_mean[0].weight, agent.actor_mean[0].weight)


@pytest.mark.parametrize("key,argv", [
    ("num_envs", ["--env-id", "sa", "--num-envs", "512", "--num-steps", "8"]),
    ("env_id", ["--env-id", "cma", "--num-envs", "256", "--num-steps", "8"]),
    ("seed", SA + ["--seed", "2"]),
    ("opponent", SA + ["--opponent", "self"]),
])
def test_resume_refuses_another_structure(key, argv, sa_runs, tmp_path):
    with pytest.raises(ValueError, match=key):
        train(argv + ["--num-updates", "4", "--resume", sa_runs[0].aside], tmp_path)


def test_world_size_two_is_refused_before_a_process_group(monkeypatch, tmp_path):
    import torch.distributed as dist
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(dist, "init_process_group", lambda *a, **k: pytest.fail("a process group was created"))
    with pytest.raises(ValueError, match="per-rank state files are not built"):
        train(SA + ["--num-updates", "1", "--checkpoint-every", "1"], tmp_path)
