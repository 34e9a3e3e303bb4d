"""--act-gain / -noise / -levels / -deadband / -loss in the train loop (envs/wrappers.py Actuated): the
flags given as zero are the run without them, bit for bit and wrapper for wrapper; with them on the run trains for every
wrapper, is reproducible, differs from the flags-off run, resumes bit-equal, evaluates as a pure function of (weights,
seed, update), a policy opponent commands through the second channel, and perception and actuation work together."""
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from test_eval_train import EVAL, assert_params_equal, train, training_keys

pytestmark = pytest.mark.gpu
ZERO = ["--act-gain", "0", "--act-noise", "0", "--act-levels", "0", "--act-deadband", "0", "--act-loss", "0"]
ON = ["--act-gain", "0.05", "--act-noise", "0.02", "--act-levels", "127", "--act-deadband", "0.03", "--act-loss", "0.1"]
OBS = ["--obs-delay", "2", "--obs-noise-pos", "0.002", "--obs-noise-ang", "0.02"]
SA = ["--env-id", "sa", "--num-updates", "3"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("actuate")
    return dict(root=root, plain=train(SA, root / "plain"), zero=train(SA + ZERO, root / "zero"),
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


def test_the_flags_given_as_zero_are_the_run_without_them(runs):
    (p0, h0, _), (p1, h1, _) = runs["plain"], runs["zero"]
    assert_params_equal(p0, p1)
    assert training_keys(h0) == training_keys(h1)
    for extra in ([], ["--env-id", "dma"], ["--opponent", "mirror"], OBS):
        assert wrapper_chain(extra) == wrapper_chain(extra + ZERO) and "Actuated" not in wrapper_chain(extra)
        assert wrapper_chain(extra + ON)[0] == "Actuated" and wrapper_chain(extra + ON)[1:] == wrapper_chain(extra)
    assert wrapper_chain(OBS + ON)[:2] == ["Actuated", "Perceived"]  # the outermost
    for one in (["--act-gain", "0.01"], ["--act-noise", "0.01"], ["--act-levels", "7"], ["--act-deadband", "0.01"],
                ["--act-loss", "0.01"]):
        assert wrapper_chain(one)[0] == "Actuated", one


def test_two_actuated_runs_are_bit_equal_and_differ_from_the_flags_off_run(runs):
    (pa, ha, _), (pb, hb, _) = runs["a"], runs["b"]
    assert [h["update"] for h in ha] == [1, 2, 3]
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    assert any(not torch.equal(x, y) for x, y in zip(pa, runs["plain"][0]))
    assert all(torch.isfinite(x).all() for x in pa)


def test_the_evaluation_is_reported_the_same_twice(runs):
    ea, eb = [h["eval"] for h in runs["a"][1]], [h["eval"] for h in runs["b"][1]]
    assert ea == eb and all(sum(r[k] for k in ("wins", "losses", "draws")) == 64 for e in ea for r in e.values())


def test_a_resumed_actuated_run_is_the_unbroken_run(runs):
    pa, ha, aside = runs["a"]
    argv = SA + ON + EVAL + ["--checkpoint-every", "1"]
    pb, hb, _ = train(argv + ["--resume", aside], runs["root"] / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb) and hb[2]["eval"] == ha[2]["eval"]
    with pytest.raises(ValueError, match="act_levels"):
        train(SA + ON[:5] + ["63"] + ON[6:] + ["--resume", aside], runs["root"] / "refused")
    with pytest.raises(ValueError, match="act_"):
        train(SA + ["--resume", aside], runs["root"] / "refused2")


@pytest.mark.parametrize("argv", [["--env-id", "cma"], ["--env-id", "dma", "--num-envs", "258"],
                                  ["--env-id", "sa", "--opponent", "mirror"],
                                  ["--env-id", "dma", "--num-envs", "258", "--opponent", "mirror"]],
                         ids=["cma", "dma", "mirror-sa", "mirror-dma"])
def test_an_actuated_run_completes_for_every_wrapper(argv, tmp_path, monkeypatch):
    from envs import wrappers as W
    built = []
    init = W.Actuated.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    monkeypatch.setattr(W.Actuated, "__init__", spy)
    params, hist, _ = train(argv + ON + ["--num-updates", "2"], tmp_path / "run")
    assert [h["update"] for h in hist] == [1, 2]
    assert all(torch.isfinite(x).all() for x in params)
    assert all(h["v_loss"] == h["v_loss"] and h["approx_kl"] == h["approx_kl"] for h in hist)
    ch = built[-1].channel
    mirror = "mirror" in argv
    robots = 1 if "sa" in argv else 3
    n = ch.n_fields
    want = (robots, robots * n if mirror else 0, robots, 2 if mirror else 1, 0)
    assert tuple(ch.layout) == want and ch.call == 16 and not ch.fresh
    assert ch.done_stride == (3 if "dma" in argv else 1) and ch.rows == n * robots * (2 if mirror else 1)
    assert int(ch.episode.min()) >= 1  # every field began an episode at the start call


def test_a_policy_opponent_commands_through_the_second_channel(tmp_path, monkeypatch):
    from envs import wrappers as W
    from vss_amd import actuate as A
    built, seen = [], []
    init = W.Actuated.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    actuate = A.ActuationChannel.actuate

    def channel_spy(self, cmd, done_prev=None, out=None):
        seen.append((self, self.call, cmd.data_ptr(), None if out is None else out.data_ptr(),
                     None if done_prev is None else done_prev.data_ptr()))
        return actuate(self, cmd, done_prev, out)

    monkeypatch.setattr(W.Actuated, "__init__", spy)
    monkeypatch.setattr(A.ActuationChannel, "actuate", channel_spy)
    argv = ["--env-id", "sa", "--opponent", "self", "--num-updates", "2", "--checkpoint-every", "1"] + ON
    params, hist, aside = train(argv, tmp_path / "self", copy_at=1)
    env = built[-1]
    ch, yellow = env.channel, env.opponent_channel
    assert yellow is not None and yellow.layout == (3, 0, 3, 1, 1) and ch.layout == (1, 0, 1, 1, 0)
    assert yellow.seed == ch.seed and yellow.params == ch.params and yellow.call == ch.call == 16
    assert type(env.env._opponent) is W._ActuatedTeam and env.env._opponent.channel is yellow
    mine = [s for s in seen if s[0] is ch]
    theirs = [s for s in seen if s[0] is yellow]
    assert len(mine) == len(theirs) == 16
    # the same call index and the same dones on both sides, yellow in place on the versus step's opp_act
    assert [s[1] for s in mine] == [s[1] for s in theirs] == list(range(16))
    assert [s[4] for s in mine] == [s[4] for s in theirs] and len({s[4] for s in mine}) == 1
    opp_act = env._opp_act
    assert all(s[2] == s[3] == opp_act.data_ptr() for s in theirs) and all(s[3] is None for s in mine)
    # yellow's entities: what the wheels got is a multiple of 1 / 127 times the yellow gains, plus noise -- the state
    # shows the quantised commands and gains that are not the learner's
    held = yellow.held.cpu()
    assert torch.equal(torch.round(held * 127) / 127, held) and float(held.abs().max()) <= 1.0
    assert not torch.equal(yellow.gain[0, :, 0].cpu(), ch.gain[0, :, 0].cpu())
    import numpy as np
    n = ch.n_fields
    fresh = yellow.episode.cpu().numpy().view(np.uint32)
    zg = np.clip(A.episode_normals(yellow.seed, np.arange(n), fresh), -3, 3).reshape(n, 6, 2)[:, 3:]
    assert np.array_equal(yellow.gain[0].cpu().numpy(), np.float32(1) + np.float32(0.05) * zg)  # entities 3..5
    # and the channels are part of the checkpoint: the resumed run ends on the same bits
    pb, hb, _ = train(argv + ["--resume", aside], tmp_path / "resumed")
    assert_params_equal(params, pb)
    assert training_keys(hist) == training_keys(hb)
    # the scripted team is not actuated: no second channel
    train(["--env-id", "sa", "--opponent", "scripted", "--num-updates", "1"] + ON, tmp_path / "scripted")
    assert built[-1].opponent_channel is None and type(built[-1].env._opponent).__name__ == "TeamScripted"


def test_perception_and_actuation_together_complete_and_resume_bit_equal(tmp_path, monkeypatch):
    from envs import wrappers as W
    built = []
    init = W.Actuated.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    monkeypatch.setattr(W.Actuated, "__init__", spy)
    argv = ["--env-id", "sa", "--opponent", "self", "--num-updates", "3", "--checkpoint-every", "1"] + ON + OBS
    pa, ha, aside = train(argv, tmp_path / "a", copy_at=2)
    env = built[-1]
    assert type(env.env) is W.Perceived and env.opponent_channel is not None and env.env.opponent_channel is not None
    team = env.env.env._opponent  # perceived rows in, actuated commands out
    assert type(team) is W._PerceivedTeam and type(team.team) is W._ActuatedTeam
    assert env.channel.call == 24 and env.env.channel.call == 25
    pb, hb, _ = train(argv + ["--resume", aside], tmp_path / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    assert all(torch.isfinite(x).all() for x in pa)
