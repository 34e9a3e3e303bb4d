"""--opponent mirror in the PPO loop: both teams' robots are learner rows of one step (vss_step_mirror)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ppo_continuous_action_isaacgym as P

pytestmark = pytest.mark.gpu
KEYS = ("v_loss", "pg_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "mean_return", "episodes",
        "opponent_version", "mean_return_blue", "mean_return_yellow")
BASE = ["--num-steps", "8", "--num-updates", "3", "--log", "false"]


def run(*extra, env_id="sa", num_envs=256, keys=KEYS):
    args = P.parse_args(["--env-id", env_id, "--num-envs", str(num_envs)] + BASE + list(extra))
    _, hist = P.train(args)
    return [{k: h[k] for k in keys} for h in hist]


@pytest.fixture(scope="module")
def mirror_history():
    # the kernel warm-up on (its default): it re-enters train() with the same --opponent
    return run("--opponent", "mirror")


def test_mirror_trains_both_teams_rows(mirror_history):
    assert len(mirror_history) == 3
    for h in mirror_history:
        assert all(math.isfinite(h[k]) for k in KEYS), h
    assert [h["opponent_version"] for h in mirror_history] == [-1, -1, -1]


def test_mirror_is_deterministic(mirror_history):
    again = run("--opponent", "mirror", "--kernel-warmup", "false")
    assert again == mirror_history


def test_mirror_differs_from_the_ou_opponent(mirror_history):
    """Yellow robot 0 is the policy and its rows are in the batch: other losses from the first update on."""
    ou = run("--opponent", "ou", "--kernel-warmup", "false", keys=("v_loss",))
    assert ou[0]["v_loss"] != mirror_history[0]["v_loss"]


@pytest.mark.parametrize("env_id,num_envs", [("cma", 256), ("dma", 258)])
def test_mirror_other_modes_complete(env_id, num_envs):
    hist = run("--opponent", "mirror", "--kernel-warmup", "false", env_id=env_id, num_envs=num_envs)
    assert [h["opponent_version"] for h in hist] == [-1, -1, -1]
    assert all(math.isfinite(h[k]) for h in hist for k in KEYS)


def make(env_id, num_envs, seed=5):
    from envs.wrappers import make_env
    return make_env(SimpleNamespace(cuda=True, env_id=env_id, num_envs=num_envs, opponent="mirror", seed=seed))


def test_row_count_that_does_not_divide_is_refused():
    with pytest.raises(ValueError, match="multiple of 2"):
        run("--opponent", "mirror", "--num-envs", "255", "--kernel-warmup", "false")
    with pytest.raises(ValueError, match="multiple of 6"):
        make("dma", 256)


def test_a_mirror_wrapper_has_no_opponent():
    from play import TeamZero
    _, env = make("sa", 64)
    with pytest.raises(ValueError):
        env.set_opponent(TeamZero())


@pytest.mark.parametrize("env_id,rows_per_field", [("sa", 2), ("cma", 2), ("dma", 6)])
def test_wrapper_step_is_the_native_mirror_step(env_id, rows_per_field):
    """The wrapper's step equals a direct native_step_mirror call bit for bit; rows are team-major, and the two
    halves of dones, time_outs and progress are equal."""
    n = 35
    rows = n * rows_per_field
    (raw_w, w), (raw_d, _) = make(env_id, rows), make(env_id, rows)
    assert raw_w.num_fields == n and w.ROWS_PER_FIELD == rows_per_field and w.num_envs == rows
    raw_w.max_episode_length = raw_d.max_episode_length = 3
    dev, half = raw_d.device, rows // 2
    width = w.action_space.shape[0]
    io = dict(ou_buf=raw_d.dof_velocity_buf.clone(), obs=torch.zeros((half, 52), device=dev),
              terminal_obs=torch.zeros((half, 52), device=dev), rew=torch.zeros((half, 4), device=dev),
              reward_sum=torch.zeros(half, device=dev), dones_rep=torch.zeros(half, dtype=torch.long, device=dev),
              time_outs=torch.zeros(half, dtype=torch.bool, device=dev), progress_f=torch.zeros(half, device=dev))
    yl = {k: torch.zeros_like(v) for k, v in io.items() if k not in ("ou_buf", "dones_rep")}
    yl["dones"] = torch.zeros_like(io["dones_rep"])
    first = w.reset()["obs"]
    full = raw_d.compute_observations(torch.empty((n, 2, 3, 52), device=dev), n_agents=6)
    R = rows_per_field // 2
    assert torch.equal(first[:half].view(n, R, 52), full[:, 0, :R]) and torch.equal(first[half:].view(n, R, 52), full[:, 1, :R])
    gen = torch.Generator(device=dev).manual_seed(11)
    both = lambda b, y: np.concatenate([b.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32)])
    finished = 0
    for t in range(5):
        a = torch.rand((rows, width), device=dev, generator=gen) * 2.4 - 1.2
        obs, reward, dones, info = w.step(a)
        raw_d.native_step_mirror(w.MODE, a, io, yl)
        torch.cuda.synchronize()
        assert obs["obs"].shape == (rows, 52) and reward.shape == (rows,) and dones.shape == (rows,)
        np.testing.assert_array_equal(obs["obs"].cpu().numpy().view(np.uint32), both(io["obs"], yl["obs"]))
        np.testing.assert_array_equal(info["terminal_observation"].cpu().numpy().view(np.uint32),
                                      both(io["terminal_obs"], yl["terminal_obs"]))
        np.testing.assert_array_equal(info["rews"].cpu().numpy().view(np.uint32), both(io["rew"], yl["rew"]))
        np.testing.assert_array_equal(reward.cpu().numpy().view(np.uint32), both(io["reward_sum"], yl["reward_sum"]))
        np.testing.assert_array_equal(w.action_buf.cpu().numpy().view(np.uint32), io["ou_buf"].cpu().numpy().view(np.uint32))
        assert torch.equal(dones, torch.cat([io["dones_rep"], yl["dones"]]))
        assert torch.equal(info["time_outs"], torch.cat([io["time_outs"], yl["time_outs"]]))
        assert torch.equal(info["progress_buffer"], torch.cat([io["progress_f"], yl["progress_f"]]))
        for v in (dones, info["time_outs"], info["progress_buffer"]):
            assert torch.equal(v[:half], v[half:])
        assert torch.equal(dones[:half].view(n, R)[:, 0], raw_w.reset_buf)
        finished += int(dones.sum())
    assert finished >= rows  # max length 3: every field timed out on the way
