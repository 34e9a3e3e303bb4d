"""--obs-predict in the train loop (envs/wrappers.py Estimated): 0 is the run without the flag, bit for
bit and wrapper for wrapper; with 1 the run trains for every wrapper, is reproducible, differs from the run with
prediction off, resumes bit-equal, evaluates as a pure function of (weights, seed, update), a policy opponent acts on
the second estimation channel's rows, and perception, estimation and actuation work together."""
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from test_eval_train import EVAL, assert_params_equal, train, training_keys

pytestmark = pytest.mark.gpu
OBS = ["--obs-delay", "2", "--obs-noise-pos", "0.002"]
ON = OBS + ["--obs-predict", "1"]
ACT = ["--act-gain", "0.05", "--act-noise", "0.02", "--act-levels", "127", "--act-deadband", "0.03", "--act-loss", "0.1"]
SA = ["--env-id", "sa", "--num-updates", "3"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("estimate")
    return dict(root=root, plain=train(SA, root / "plain"), zero=train(SA + ["--obs-predict", "0"], root / "zero"),
                off=train(SA + OBS, root / "off"),
                a=train(SA + ON + EVAL + ["--checkpoint-every", "1"], root / "a", copy_at=2),
                b=train(SA + ON + EVAL, root / "b"))


def wrapper_chain(argv):
    from envs.wrappers import make_env
    args = P.parse_args(["--num-envs", "258", "--num-steps", "8"] + argv)
    _, env = make_env(args)
    chain = []
    while hasattr(env, "env"):
        chain.append(type(env).__name__)
        env = env.env
    return chain + [type(env).__name__]


def spy_on(monkeypatch, cls):
    built = []
    init = cls.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    monkeypatch.setattr(cls, "__init__", spy)
    return built


def test_the_flag_given_as_zero_is_the_run_without_it(runs):
    (p0, h0, _), (p1, h1, _) = runs["plain"], runs["zero"]
    assert_params_equal(p0, p1)
    assert training_keys(h0) == training_keys(h1)
    for extra in ([], ["--env-id", "dma"], ["--opponent", "mirror"], OBS, OBS + ACT):
        assert wrapper_chain(extra) == wrapper_chain(extra + ["--obs-predict", "0"]) and "Estimated" not in wrapper_chain(extra)
    for extra in ([], ["--env-id", "dma"], ["--opponent", "mirror"]):
        assert wrapper_chain(extra + ON) == ["Estimated"] + wrapper_chain(extra + OBS)
        assert wrapper_chain(extra + ON + ACT) == ["Actuated", "Estimated"] + wrapper_chain(extra + OBS)  # inside Actuated
    with pytest.raises(ValueError, match="--obs-predict 1 needs --obs-delay"):
        wrapper_chain(["--obs-predict", "1"])


def test_two_estimated_runs_are_bit_equal_and_differ_from_the_run_with_prediction_off(runs):
    (pa, ha, _), (pb, hb, _) = runs["a"], runs["b"]
    assert [h["update"] for h in ha] == [1, 2, 3]
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    assert any(not torch.equal(x, y) for x, y in zip(pa, runs["off"][0]))
    assert any(not torch.equal(x, y) for x, y in zip(pa, runs["plain"][0]))
    assert all(torch.isfinite(x).all() for x in pa)


def test_the_evaluation_is_reported_the_same_twice(runs):
    ea, eb = [h["eval"] for h in runs["a"][1]], [h["eval"] for h in runs["b"][1]]
    assert ea == eb and all(sum(r[k] for k in ("wins", "losses", "draws")) == 64 for e in ea for r in e.values())


def test_a_resumed_estimated_run_is_the_unbroken_run(runs):
    pa, ha, aside = runs["a"]
    argv = SA + ON + EVAL + ["--checkpoint-every", "1"]
    pb, hb, _ = train(argv + ["--resume", aside], runs["root"] / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb) and hb[2]["eval"] == ha[2]["eval"]
    with pytest.raises(ValueError, match="obs_predict"):
        train(SA + OBS + ["--obs-predict", "0", "--resume", aside], runs["root"] / "refused")
    with pytest.raises(ValueError, match="obs_predict"):
        train(SA + OBS + ["--resume", aside], runs["root"] / "refused2")


@pytest.mark.parametrize("argv", [["--env-id", "cma"], ["--env-id", "dma", "--num-envs", "258"],
                                  ["--env-id", "sa", "--opponent", "mirror"],
                                  ["--env-id", "dma", "--num-envs", "258", "--opponent", "mirror"]],
                         ids=["cma", "dma", "mirror-sa", "mirror-dma"])
def test_an_estimated_run_completes_for_every_wrapper(argv, tmp_path, monkeypatch):
    from envs import wrappers as W
    built = spy_on(monkeypatch, W.Estimated)
    params, hist, _ = train(argv + ON + ["--num-updates", "2"], tmp_path / "run")
    assert [h["update"] for h in hist] == [1, 2]
    assert all(torch.isfinite(x).all() for x in params)
    assert all(h["v_loss"] == h["v_loss"] and h["approx_kl"] == h["approx_kl"] for h in hist)
    env = built[-1]
    ch = env.channel
    mirror = "mirror" in argv
    robots = 3 if "dma" in argv else 1
    n = ch.n_fields
    assert tuple(ch.layout) == (robots, robots * n if mirror else 0, robots, 2 if mirror else 1)  # one two-team channel
    assert tuple(ch.layout) == tuple(env.env.channel.layout)[:4] and ch.done_stride == env.env.channel.done_stride == robots
    assert ch.call == env.env.channel.call == 17 and ch.delay == 2 and ch.age.shape == (2 if mirror else 1, n, robots)
    assert int(ch.age.max()) == 2


def test_a_policy_opponent_acts_on_the_second_estimation_channels_rows(tmp_path, monkeypatch):
    from envs import wrappers as W
    from vss_amd import opponent as OPP
    built, seen = spy_on(monkeypatch, W.Estimated), []
    call = OPP.SnapshotOpponent.__call__

    def team_spy(self, act, obs):
        seen.append(obs.data_ptr())
        return call(self, act, obs)

    monkeypatch.setattr(OPP.SnapshotOpponent, "__call__", team_spy)
    argv = ["--env-id", "sa", "--opponent", "self", "--num-updates", "2", "--checkpoint-every", "1"] + ON
    params, hist, aside = train(argv, tmp_path / "self", copy_at=1)
    env = built[-1]
    seen_w = env.env
    ch, yellow = env.channel, env.opponent_channel
    assert type(seen_w) is W.Perceived and seen_w.opponent_channel is not None
    assert yellow is not None and yellow.layout == (3, 0, 3, 1) and ch.layout == (1, 0, 1, 1)
    assert yellow.delay == ch.delay == 2 and yellow.call == ch.call == seen_w.opponent_channel.call == 17
    team = seen_w.env._opponent  # perceived rows in, estimated rows on to the team
    assert type(team) is W._PerceivedTeam and team.channel is seen_w.opponent_channel
    assert type(team.team) is W._EstimatedTeam and team.team.channel is yellow
    assert len(seen) == 16 and set(seen) == {yellow.obs_out.data_ptr()}  # every step's rows: the estimates, never others
    assert yellow.obs_out.data_ptr() not in (seen_w.opponent_channel.obs_out.data_ptr(), seen_w.env._opp_obs.data_ptr())
    assert not torch.equal(yellow.obs_out, seen_w.opponent_channel.obs_out)
    # and the channels are part of the checkpoint: the resumed run ends on the same bits
    pb, hb, _ = train(argv + ["--resume", aside], tmp_path / "resumed")
    assert_params_equal(params, pb)
    assert training_keys(hist) == training_keys(hb)
    # the scripted team sees the truth: no second channel of either kind
    train(["--env-id", "sa", "--opponent", "scripted", "--num-updates", "1"] + ON, tmp_path / "scripted")
    assert built[-1].opponent_channel is None and built[-1].env.opponent_channel is None
    assert type(built[-1].env.env._opponent).__name__ == "TeamScripted"


def test_perception_estimation_and_actuation_together_complete_and_resume_bit_equal(tmp_path, monkeypatch):
    from envs import wrappers as W
    built = spy_on(monkeypatch, W.Actuated)
    argv = ["--env-id", "sa", "--opponent", "self", "--num-updates", "3", "--checkpoint-every", "1"] + ON + ACT
    pa, ha, aside = train(argv, tmp_path / "a", copy_at=2)
    env = built[-1]
    assert type(env.env) is W.Estimated and type(env.env.env) is W.Perceived
    assert env.opponent_channel is not None and env.env.opponent_channel is not None and env.env.env.opponent_channel is not None
    team = env.env.env.env._opponent  # perceived rows in, estimated rows on, actuated commands out
    assert type(team) is W._PerceivedTeam and type(team.team) is W._EstimatedTeam and type(team.team.team) is W._ActuatedTeam
    assert env.channel.call == 24 and env.env.channel.call == 25 and env.env.env.channel.call == 25
    pb, hb, _ = train(argv + ["--resume", aside], tmp_path / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    assert all(torch.isfinite(x).all() for x in pa)
