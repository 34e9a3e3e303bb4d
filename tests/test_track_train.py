"""--obs-filter-* in the train loop (envs/wrappers.py Tracked): all flags at 0 is the run without them, bit
for bit and wrapper for wrapper; with a gain on the run trains for every wrapper, is reproducible, differs from the run
with the gains off, resumes bit-equal, evaluates as a pure function of (weights, seed, update), a policy opponent acts
on the second tracking channel's rows, and perception, tracking, estimation and actuation work together."""
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from test_estimate_train import spy_on, wrapper_chain
from test_eval_train import EVAL, assert_params_equal, train, training_keys

pytestmark = pytest.mark.gpu
OBS = ["--obs-delay", "2", "--obs-noise-pos", "0.002"]
ZERO = ["--obs-filter-team", "0", "--obs-filter-opp", "0", "--obs-filter-ball", "0"]
ON = OBS + ["--obs-filter-team", "0.2", "--obs-filter-opp", "0.5", "--obs-filter-ball", "0.5"]
PREDICT = ["--obs-predict", "1"]
ACT = ["--act-gain", "0.05", "--act-noise", "0.02", "--act-levels", "127", "--act-deadband", "0.03", "--act-loss", "0.1"]
SA = ["--env-id", "sa", "--num-updates", "3"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("track")
    return dict(root=root, plain=train(SA, root / "plain"), zero=train(SA + ZERO, root / "zero"),
                off=train(SA + OBS, root / "off"),
                a=train(SA + ON + EVAL + ["--checkpoint-every", "1"], root / "a", copy_at=2),
                b=train(SA + ON + EVAL, root / "b"))


def test_all_flags_at_zero_is_the_run_without_them(runs):
    (p0, h0, _), (p1, h1, _) = runs["plain"], runs["zero"]
    assert_params_equal(p0, p1)
    assert training_keys(h0) == training_keys(h1)
    gates = ["--obs-filter-gate-pos", "0.1", "--obs-filter-gate-vel", "0"]  # the gates alone switch nothing on
    for extra in ([], ["--env-id", "dma"], ["--opponent", "mirror"], OBS, OBS + ACT, OBS + PREDICT):
        assert wrapper_chain(extra) == wrapper_chain(extra + ZERO) == wrapper_chain(extra + ZERO + gates)
        assert "Tracked" not in wrapper_chain(extra)
    for extra in ([], ["--env-id", "dma"], ["--opponent", "mirror"]):
        assert wrapper_chain(extra + ON) == ["Tracked"] + wrapper_chain(extra + OBS)
        assert wrapper_chain(extra + ON + PREDICT) == ["Estimated", "Tracked"] + wrapper_chain(extra + OBS)  # filter, then dead-reckon
        assert wrapper_chain(extra + ON + PREDICT + ACT) == ["Actuated", "Estimated", "Tracked"] + wrapper_chain(extra + OBS)
    with pytest.raises(ValueError, match="needs vision noise"):
        wrapper_chain(["--obs-filter-team", "0.2"])
    with pytest.raises(ValueError, match="needs vision noise"):
        wrapper_chain(["--obs-delay", "2", "--obs-filter-team", "0.2"])


def test_two_tracked_runs_are_bit_equal_and_differ_from_the_run_with_the_gains_off(runs):
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


def test_a_resumed_tracked_run_is_the_unbroken_run(runs):
    pa, ha, aside = runs["a"]
    argv = SA + ON + EVAL + ["--checkpoint-every", "1"]
    pb, hb, _ = train(argv + ["--resume", aside], runs["root"] / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb) and hb[2]["eval"] == ha[2]["eval"]
    other = OBS + ["--obs-filter-team", "0.3", "--obs-filter-opp", "0.5", "--obs-filter-ball", "0.5"]
    with pytest.raises(ValueError, match="obs_filter_team"):
        train(SA + other + ["--resume", aside], runs["root"] / "refused")
    with pytest.raises(ValueError, match="obs_filter_team"):
        train(SA + OBS + ["--resume", aside], runs["root"] / "refused2")
    with pytest.raises(ValueError, match="obs_filter_gate_pos"):
        train(SA + ON + ["--obs-filter-gate-pos", "0.05", "--resume", aside], runs["root"] / "refused3")


@pytest.mark.parametrize("argv", [["--env-id", "cma"], ["--env-id", "dma", "--num-envs", "258"],
                                  ["--env-id", "sa", "--opponent", "mirror"],
                                  ["--env-id", "dma", "--num-envs", "258", "--opponent", "mirror"]],
                         ids=["cma", "dma", "mirror-sa", "mirror-dma"])
def test_a_tracked_run_completes_for_every_wrapper(argv, tmp_path, monkeypatch):
    from envs import wrappers as W
    built = spy_on(monkeypatch, W.Tracked)
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
    assert int(ch.age.max()) == 2 and tuple(ch.params) == (0.2, 0.5, 0.5, 0.03, 0.5)
    assert ch.est.shape == ch.age.shape + (52,) and not torch.equal(ch.obs_out, env.env.channel.obs_out)


def test_a_policy_opponent_acts_on_the_second_tracking_channels_rows(tmp_path, monkeypatch):
    from envs import wrappers as W
    from vss_amd import opponent as OPP
    built, seen = spy_on(monkeypatch, W.Tracked), []
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
    assert yellow.params == ch.params
    team = seen_w.env._opponent  # perceived rows in, filtered rows on to the team
    assert type(team) is W._PerceivedTeam and team.channel is seen_w.opponent_channel
    assert type(team.team) is W._TrackedTeam and team.team.channel is yellow
    assert len(seen) == 16 and set(seen) == {yellow.obs_out.data_ptr()}  # every step's rows: the filtered ones, never others
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


def test_all_four_channels_together_complete_and_resume_bit_equal(tmp_path, monkeypatch):
    from envs import wrappers as W
    built = spy_on(monkeypatch, W.Actuated)
    argv = ["--env-id", "sa", "--opponent", "self", "--num-updates", "3", "--checkpoint-every", "1"] + ON + PREDICT + ACT
    pa, ha, aside = train(argv, tmp_path / "a", copy_at=2)
    env = built[-1]
    est, trk, seen_w = env.env, env.env.env, env.env.env.env
    assert type(est) is W.Estimated and type(trk) is W.Tracked and type(seen_w) is W.Perceived
    assert all(w.opponent_channel is not None for w in (env, est, trk, seen_w))
    team = seen_w.env._opponent  # perceived rows in, filtered, then estimated rows on, actuated commands out
    assert type(team) is W._PerceivedTeam and type(team.team) is W._TrackedTeam
    assert type(team.team.team) is W._EstimatedTeam and type(team.team.team.team) is W._ActuatedTeam
    assert env.channel.call == 24 and est.channel.call == 25 and trk.channel.call == 25 and seen_w.channel.call == 25
    assert est.opponent_channel.call == trk.opponent_channel.call == seen_w.opponent_channel.call == 25
    pb, hb, _ = train(argv + ["--resume", aside], tmp_path / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    assert all(torch.isfinite(x).all() for x in pa)
    assert len(open(P.__file__).read().splitlines()) <= 600
