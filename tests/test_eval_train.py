"""--eval-every and --opponent scripted in the train loop (vss_amd/arena.py): the arena reports
unbiased per-team results without moving one bit of the training, its evaluations are a pure function of (weights,
--seed, update) -- so two runs and a resumed run report the same -- and the scripted team is a training opponent
like any other, resume included."""
import json
import os
import shutil

import pytest
import torch

import ppo_continuous_action_isaacgym as P

pytestmark = pytest.mark.gpu
KEYS = ("update", "global_step", "v_loss", "pg_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "mean_return",
        "episodes", "opponent_version")
COMMON = ["--kernel-warmup", "false", "--log", "false", "--num-envs", "256", "--num-steps", "8"]
EVAL = ["--eval-every", "1", "--eval-fields", "64"]
TEAMS = ("zero", "ou", "scripted")
RUN = "ppo_continuous_action_isaacgym_ppo-{env_id}_1"


def train(argv, save_path, copy_at=None):
    """(final parameters, history, the state file as update `copy_at` wrote it)"""
    args = P.parse_args(COMMON + argv + ["--save-path", str(save_path)])
    name = RUN.format(env_id=args.env_id)
    state_path = os.path.join(str(save_path), name, name + "-state.pt")
    aside = os.path.join(str(save_path), f"state-after-{copy_at}.pt")

    def on_update(rec, agent):
        if rec["update"] == copy_at:
            shutil.copyfile(state_path, aside)  # the checkpoint is written before on_update

    agent, hist = P.train(args, on_update=on_update if copy_at is not None else None)
    return [p.detach().clone() for p in agent.parameters()], hist, aside


def assert_params_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def training_keys(hist):
    """The history apart from eval, eval_s and the clocks."""
    clocks = ("eval", "eval_s", "sps", "wall_s", "rollout_s", "update_s", "checkpoint_s")
    return json.dumps([{k: v for k, v in h.items() if k not in clocks} for h in hist], sort_keys=True)  # NaN == NaN


@pytest.fixture(scope="module")
def sa_runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("eval")
    argv = ["--env-id", "sa", "--num-updates", "3"]
    return dict(plain=train(argv, root / "plain"), a=train(argv + EVAL, root / "a"), b=train(argv + EVAL, root / "b"),
                root=root, argv=argv)


def test_evaluation_does_not_move_one_bit_of_the_training(sa_runs):
    (p0, h0, _), (p1, h1, _) = sa_runs["plain"], sa_runs["a"]
    assert_params_equal(p0, p1)
    assert training_keys(h0) == training_keys(h1) and [set(KEYS) <= set(h) for h in h1] == [True] * 3
    assert all("eval" not in h and "eval_s" not in h for h in h0)


def test_every_field_counts_once_per_team(sa_runs):
    spent = 0.0
    for h in sa_runs["a"][1]:
        assert tuple(h["eval"]) == TEAMS and h["eval_s"] > 0
        spent += h["rollout_s"] + h["update_s"] + h["eval_s"]
        assert h["wall_s"] >= spent - 1e-3  # eval_s is part of wall_s (and of sps), outside rollout_s and update_s
        for team, r in h["eval"].items():
            assert sorted(r) == ["draws", "length", "losses", "score", "wins"]
            assert r["wins"] + r["losses"] + r["draws"] == 64 and min(r["wins"], r["losses"], r["draws"]) >= 0
            assert r["score"] == (r["wins"] - r["losses"]) / 64
            assert 0 < r["length"] <= 400
            print(h["update"], team, r)


def test_the_same_run_twice_reports_equal_evaluations(sa_runs):
    assert [h["eval"] for h in sa_runs["a"][1]] == [h["eval"] for h in sa_runs["b"][1]]
    evals = [h["eval"] for h in sa_runs["a"][1]]
    assert evals[0] != evals[1] or evals[1] != evals[2]  # and they follow the weights and the update's draws


def test_a_resumed_run_reports_the_unbroken_runs_evaluation(sa_runs):
    root, argv = sa_runs["root"], ["--env-id", "sa"] + EVAL
    pa, ha, aside = train(argv + ["--num-updates", "3", "--checkpoint-every", "1"], root / "ck", copy_at=2)
    pb, hb, _ = train(argv + ["--num-updates", "3", "--checkpoint-every", "1", "--resume", aside], root / "resumed")
    assert [h["update"] for h in hb] == [1, 2, 3]
    assert hb[2]["eval"] == ha[2]["eval"] == sa_runs["a"][1][2]["eval"]
    assert hb[1]["eval"] == ha[1]["eval"]  # carried in the saved history
    assert_params_equal(pa, pb)
    assert_params_equal(pa, sa_runs["plain"][0])  # checkpoints and evaluations together still train the same bits


@pytest.mark.parametrize("env_id", ["sa", "cma"])
def test_opponent_scripted_trains_and_two_runs_are_bit_equal(env_id, tmp_path):
    argv = ["--env-id", env_id, "--num-updates", "2", "--opponent", "scripted"]
    (p0, h0, _), (p1, h1, _) = train(argv, tmp_path / "a"), train(argv, tmp_path / "b")
    assert [h["update"] for h in h0] == [1, 2] and all(h["opponent_version"] == 1 for h in h0)
    assert_params_equal(p0, p1)
    assert training_keys(h0) == training_keys(h1)


def test_opponent_scripted_resumes_bit_equal(tmp_path):
    argv = ["--env-id", "sa", "--opponent", "scripted", "--num-updates", "3", "--checkpoint-every", "1"]
    pa, ha, aside = train(argv, tmp_path / "a", copy_at=2)
    pb, hb, _ = train(argv + ["--resume", aside], tmp_path / "b")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    with pytest.raises(ValueError, match="opponent"):
        train(["--env-id", "sa", "--opponent", "ou", "--num-updates", "3", "--resume", aside], tmp_path / "c")


def test_a_mirror_run_is_evaluated_on_a_plain_wrapper(tmp_path, monkeypatch):
    from envs import wrappers as W
    from vss_amd import arena
    built = []
    init = arena.Arena.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    monkeypatch.setattr(arena.Arena, "__init__", spy)
    _, hist, _ = train(["--env-id", "sa", "--opponent", "mirror", "--num-updates", "1"] + EVAL, tmp_path / "m")
    assert len(built) == 1 and type(built[0].wrapper) is W.SingleAgent and built[0].env.num_fields == 64
    assert tuple(hist[0]["eval"]) == TEAMS
    assert all(r["wins"] + r["losses"] + r["draws"] == 64 for r in hist[0]["eval"].values())
