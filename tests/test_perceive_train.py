"""--obs-delay / --obs-noise-* in the train loop (envs/wrappers.py Perceived): the flags given as zero
are the run without them, bit for bit and wrapper for wrapper; with them on the run trains for every wrapper, is
reproducible, differs from the flags-off run, resumes bit-equal, evaluates as a pure function of (weights, seed,
update), and a policy opponent acts on the second channel's rows."""
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from test_eval_train import EVAL, assert_params_equal, train, training_keys

pytestmark = pytest.mark.gpu
ZERO = ["--obs-delay", "0", "--obs-noise-pos", "0", "--obs-noise-vel", "0", "--obs-noise-ang", "0", "--obs-noise-angvel", "0"]
ON = ["--obs-delay", "2", "--obs-noise-pos", "0.002", "--obs-noise-ang", "0.02"]
SA = ["--env-id", "sa", "--num-updates", "3"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("perceive")
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
    for extra in ([], ["--env-id", "dma"], ["--opponent", "mirror"]):
        assert wrapper_chain(extra) == wrapper_chain(extra + ZERO) and "Perceived" not in wrapper_chain(extra)
        assert wrapper_chain(extra + ON)[0] == "Perceived" and wrapper_chain(extra + ON)[1:] == wrapper_chain(extra)
    assert wrapper_chain(["--obs-noise-angvel", "0.1"])[0] == "Perceived"


def test_two_perceived_runs_are_bit_equal_and_differ_from_the_flags_off_run(runs):
    (pa, ha, _), (pb, hb, _) = runs["a"], runs["b"]
    assert [h["update"] for h in ha] == [1, 2, 3]
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    assert any(not torch.equal(x, y) for x, y in zip(pa, runs["plain"][0]))
    assert all(torch.isfinite(x).all() for x in pa)


def test_the_evaluation_is_reported_the_same_twice(runs):
    ea, eb = [h["eval"] for h in runs["a"][1]], [h["eval"] for h in runs["b"][1]]
    assert ea == eb and all(sum(r[k] for k in ("wins", "losses", "draws")) == 64 for e in ea for r in e.values())


def test_a_resumed_perceived_run_is_the_unbroken_run(runs):
    pa, ha, aside = runs["a"]
    argv = SA + ON + EVAL + ["--checkpoint-every", "1"]
    pb, hb, _ = train(argv + ["--resume", aside], runs["root"] / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb) and hb[2]["eval"] == ha[2]["eval"]
    with pytest.raises(ValueError, match="obs_delay"):
        train(SA + ["--obs-delay", "3", "--obs-noise-pos", "0.002", "--obs-noise-ang", "0.02", "--resume", aside],
              runs["root"] / "refused")
    with pytest.raises(ValueError, match="obs_"):
        train(SA + ["--resume", aside], runs["root"] / "refused2")


@pytest.mark.parametrize("argv", [["--env-id", "cma"], ["--env-id", "dma", "--num-envs", "258"],
                                  ["--env-id", "sa", "--opponent", "mirror"],
                                  ["--env-id", "dma", "--num-envs", "258", "--opponent", "mirror"]],
                         ids=["cma", "dma", "mirror-sa", "mirror-dma"])
def test_a_perceived_run_completes_for_every_wrapper(argv, tmp_path):
    params, hist, _ = train(argv + ON + ["--num-updates", "2"], tmp_path / "run")
    assert [h["update"] for h in hist] == [1, 2]
    assert all(torch.isfinite(x).all() for x in params)
    assert all(h["v_loss"] == h["v_loss"] and h["approx_kl"] == h["approx_kl"] for h in hist)


def test_a_policy_opponent_acts_on_the_second_channels_rows(tmp_path, monkeypatch):
    from envs import wrappers as W
    from vss_amd import opponent as OPP
    built, seen = [], []
    init = W.Perceived.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    call = OPP.SnapshotOpponent.__call__

    def team_spy(self, act, obs):
        seen.append(obs.data_ptr())
        return call(self, act, obs)

    monkeypatch.setattr(W.Perceived, "__init__", spy)
    monkeypatch.setattr(OPP.SnapshotOpponent, "__call__", team_spy)
    params, hist, aside = train(["--env-id", "sa", "--opponent", "self", "--num-updates", "2", "--checkpoint-every", "1"] + ON,
                                tmp_path / "self", copy_at=1)
    env = built[-1]
    ch, yellow = env.channel, env.opponent_channel
    assert yellow is not None and yellow.layout == (3, 0, 3, 1, 1) and yellow.seed == ch.seed and yellow.call == ch.call == 17
    assert (yellow.delay, yellow.noise) == (ch.delay, ch.noise) == (2, (0.002, 0.0, 0.02, 0.0))
    assert type(env.env._opponent) is W._PerceivedTeam and env.env._opponent.channel is yellow
    assert len(seen) == 16 and set(seen) == {yellow.obs_out.data_ptr()}  # every step's rows, never the true ones
    assert seen[0] != env.env._opp_obs.data_ptr()
    # one world: the yellow rows' ball is the blue row's, negated, noise included (a field that has not just reset)
    blue, opp = ch.obs_out.cpu(), yellow.obs_out.view(-1, 3, 52).cpu()
    assert torch.equal(opp[:, 0, 0:2], -blue[:, 0:2])
    true = env.env._opp_obs.cpu()
    assert not torch.equal(opp, true)
    # and the channels are part of the checkpoint: the resumed run ends on the same bits
    pb, hb, _ = train(["--env-id", "sa", "--opponent", "self", "--num-updates", "2", "--checkpoint-every", "1", "--resume", aside]
                      + ON, tmp_path / "resumed")
    assert_params_equal(params, pb)
    assert training_keys(hist) == training_keys(hb)
    # the scripted team sees the truth: no second channel
    train(["--env-id", "sa", "--opponent", "scripted", "--num-updates", "1"] + ON, tmp_path / "scripted")
    assert built[-1].opponent_channel is None and type(built[-1].env._opponent).__name__ == "TeamScripted"
