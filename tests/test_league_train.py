"""--opponent pool in the PPO loop: a league of past snapshots drives the yellow team."""
import math

import pytest

import ppo_continuous_action_isaacgym as P

pytestmark = pytest.mark.gpu
KEYS = ("v_loss", "pg_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "mean_return", "episodes",
        "opponent_version")
LEAGUE = ("opponent_pool_versions", "opponent_pool_winrate")
BASE = ["--num-steps", "8", "--num-updates", "3", "--log", "false"]
POOL = ["--opponent", "pool", "--opponent-update-every", "1", "--opponent-pool-slots", "4"]


def run(*extra, env_id="sa", num_envs=256):
    args = P.parse_args(["--env-id", env_id, "--num-envs", str(num_envs)] + BASE + list(extra))
    _, hist = P.train(args)
    return [{k: h[k] for k in KEYS + LEAGUE if k in h} for h in hist]


def same(a, b):
    """History equality with NaN == NaN (a slot without a finished episode has no win rate)."""
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (math.isnan(a) and math.isnan(b))
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return a == b


def check(hist, count):
    assert len(hist) == 3
    for i, h in enumerate(hist, 1):
        assert all(math.isfinite(h[k]) for k in KEYS), h
        assert len(h["opponent_pool_versions"]) == count and all(0 <= v <= i for v in h["opponent_pool_versions"]), h
        assert len(h["opponent_pool_winrate"]) == count
        # 8-step rollouts end few episodes: a slot's win rate is a share, or NaN where no episode ended
        assert all(math.isnan(w) or 0.0 <= w <= 1.0 for w in h["opponent_pool_winrate"]), h
    assert [h["opponent_version"] for h in hist] == [0, 1, 2]
    # the first max(1, round(0.5 * count)) slots play the newest snapshot
    assert all(h["opponent_pool_versions"][0] == h["opponent_version"] for h in hist)


@pytest.fixture(scope="module")
def league_history():
    # the kernel warm-up on (its default): it re-enters train() with the same --opponent
    return run(*POOL)


def test_pool_trains_and_grows(league_history):
    check(league_history, 4)


def test_pool_is_deterministic(league_history):
    again = run(*POOL, "--kernel-warmup", "false")
    assert same(again, league_history)


def test_pool_differs_from_the_ou_opponent(league_history):
    ou = run("--opponent", "ou", "--kernel-warmup", "false")
    assert ou[0]["v_loss"] != league_history[0]["v_loss"]
    assert all(k not in h for h in ou for k in LEAGUE)


@pytest.mark.parametrize("env_id,num_envs,count", [("cma", 256, 4), ("dma", 255, 2)])
def test_pool_other_modes_complete(env_id, num_envs, count):
    check(run(*POOL, "--kernel-warmup", "false", env_id=env_id, num_envs=num_envs), count)
