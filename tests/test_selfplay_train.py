"""--opponent self | ou in the PPO loop: a snapshot of the learner drives the yellow team."""
import math

import pytest

import ppo_continuous_action_isaacgym as P

pytestmark = pytest.mark.gpu
KEYS = ("v_loss", "pg_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "mean_return", "episodes",
        "opponent_version")
BASE = ["--num-steps", "8", "--num-updates", "3", "--log", "false"]


def run(*extra, env_id="sa", num_envs=256):
    args = P.parse_args(["--env-id", env_id, "--num-envs", str(num_envs)] + BASE + list(extra))
    _, hist = P.train(args)
    return [{k: h[k] for k in KEYS} for h in hist]


@pytest.fixture(scope="module")
def selfplay_history():
    # the kernel warm-up on (its default): it re-enters train() with the same --opponent
    return run("--opponent", "self", "--opponent-update-every", "2")


def test_selfplay_trains_and_refreshes_the_snapshot(selfplay_history):
    assert len(selfplay_history) == 3
    for h in selfplay_history:
        assert all(math.isfinite(h[k]) for k in KEYS), h
    assert [h["opponent_version"] for h in selfplay_history] == [0, 0, 2]


def test_selfplay_is_deterministic(selfplay_history):
    again = run("--opponent", "self", "--opponent-update-every", "2", "--kernel-warmup", "false")
    assert again == selfplay_history


def test_opponent_ou_is_the_default_path():
    plain = run("--kernel-warmup", "false")
    ou = run("--opponent", "ou", "--kernel-warmup", "false")
    assert plain == ou and [h["opponent_version"] for h in ou] == [-1, -1, -1]


def test_selfplay_differs_from_the_ou_opponent(selfplay_history):
    """The yellow team is the policy, not noise: the learner sees other rewards from the first rollout on."""
    ou = run("--opponent", "ou", "--kernel-warmup", "false")
    assert ou[0]["v_loss"] != selfplay_history[0]["v_loss"]


@pytest.mark.parametrize("env_id,num_envs", [("cma", 256), ("dma", 255)])
def test_selfplay_other_modes_complete(env_id, num_envs):
    hist = run("--opponent", "self", "--opponent-update-every", "2", "--kernel-warmup", "false",
               env_id=env_id, num_envs=num_envs)
    assert [h["opponent_version"] for h in hist] == [0, 0, 2]
    assert all(math.isfinite(h[k]) for h in hist for k in KEYS)
