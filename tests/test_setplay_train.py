"""--setplay-* in the train loop (envs/wrappers.py set_setplays): a share of 0 is the run without the
flags, bit for bit and wrapper for wrapper; with a share the run is reproducible, differs, resumes bit-equal and refuses
another mix; every wrapper and a policy opponent (whose rows are staged too) work, all channels work together, and the
arena scores the agent from each play of --eval-setplays as a pure function of (weights, seed, update)."""
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from test_estimate_train import wrapper_chain
from test_eval_train import EVAL, assert_params_equal, train, training_keys

pytestmark = pytest.mark.gpu
SA = ["--env-id", "sa", "--num-updates", "3"]
ZERO = ["--setplay-share", "0", "--setplay-mix", "kickoff:1"]
ON = ["--setplay-share", "0.5", "--setplay-mix", "kickoff:1,free_ball:2,penalty_for:1"]
PLAYS = ["--eval-setplays", "penalty_for,penalty_against", "--eval-teams", "zero,scripted"]
OBS = ["--obs-delay", "2", "--obs-noise-pos", "0.002", "--obs-filter-team", "0.2", "--obs-filter-opp", "0.5",
       "--obs-filter-ball", "0.5", "--obs-predict", "1"]
ACT = ["--act-gain", "0.05", "--act-noise", "0.02", "--act-levels", "127", "--act-deadband", "0.03", "--act-loss", "0.1"]


def spy_on_stagers(monkeypatch):
    from vss_amd import setplay as S
    built, init = [], S.Stager.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    monkeypatch.setattr(S.Stager, "__init__", spy)
    return built


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("setplay")
    return dict(root=root, plain=train(SA, root / "plain"), zero=train(SA + ZERO, root / "zero"),
                a=train(SA + ON + EVAL + PLAYS + ["--checkpoint-every", "1"], root / "a", copy_at=2),
                b=train(SA + ON + EVAL + PLAYS, root / "b"))


def test_a_share_of_zero_is_the_run_without_the_flags(runs):
    (p0, h0, _), (p1, h1, _) = runs["plain"], runs["zero"]
    assert_params_equal(p0, p1)
    assert training_keys(h0) == training_keys(h1)
    for extra in ([], ["--env-id", "dma"], ["--opponent", "mirror"], OBS, OBS + ACT):
        assert wrapper_chain(extra) == wrapper_chain(extra + ZERO) == wrapper_chain(extra + ON)  # no wrapper is added


def test_make_env_attaches_a_stager_only_with_a_share(monkeypatch):
    from envs.wrappers import make_env
    built = spy_on_stagers(monkeypatch)
    for extra in ([], ZERO):
        _, env = make_env(P.parse_args(["--num-envs", "258", "--num-steps", "8"] + extra))
        assert env._setplays is None and not built
    _, env = make_env(P.parse_args(["--num-envs", "258", "--num-steps", "8"] + ON + OBS))
    base = env
    while hasattr(base.env, "env"):
        base = base.env
    st = base._setplays  # inside every channel wrapper
    assert built == [st] and st.call == 1 and st.table.names == ("kickoff", "free_ball", "penalty_for") and st.table.share == 0.5
    assert 0 < int(st.counts.sum()) < 258 and int((st.chosen >= 0).sum()) == int(st.counts.sum())


def test_two_runs_with_set_plays_are_bit_equal_and_differ_from_the_plain_run(runs):
    (pa, ha, _), (pb, hb, _) = runs["a"], runs["b"]
    assert [h["update"] for h in ha] == [1, 2, 3]
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    assert any(not torch.equal(x, y) for x, y in zip(pa, runs["plain"][0]))
    assert all(torch.isfinite(x).all() for x in pa)


def test_the_arena_scores_every_play_the_same_twice_with_every_field_counted_once(runs):
    ea, eb = [h["eval"] for h in runs["a"][1]], [h["eval"] for h in runs["b"][1]]
    assert ea == eb
    for e in ea:
        assert sorted(e) == sorted(["zero", "scripted"] + [f"{t}@{p}" for t in ("zero", "scripted")
                                                           for p in ("penalty_for", "penalty_against")])
        assert all(sum(r[k] for k in ("wins", "losses", "draws")) == 64 for r in e.values())
        assert all(set(r) == {"score", "wins", "losses", "draws", "length"} for r in e.values())
    # the plain entries are those of a run without --eval-setplays
    plain = train(SA + ON + EVAL + ["--eval-teams", "zero,scripted"], runs["root"] / "plain-eval")[1]
    assert [{k: e[k] for k in ("zero", "scripted")} for e in ea] == [h["eval"] for h in plain]


def test_a_resumed_run_is_the_unbroken_run_and_another_mix_is_refused(runs):
    pa, ha, aside = runs["a"]
    argv = SA + ON + EVAL + PLAYS + ["--checkpoint-every", "1"]
    pb, hb, _ = train(argv + ["--resume", aside], runs["root"] / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb) and hb[2]["eval"] == ha[2]["eval"]
    with pytest.raises(ValueError, match="setplay_mix"):
        train(SA + ["--setplay-share", "0.5", "--setplay-mix", "kickoff:1", "--resume", aside], runs["root"] / "refused")
    with pytest.raises(ValueError, match="setplay_share"):
        train(SA + ["--resume", aside], runs["root"] / "refused2")
    with pytest.raises(ValueError, match="setplay_share"):
        train(SA + ["--setplay-share", "0.25"] + ON[2:] + ["--resume", aside], runs["root"] / "refused3")


@pytest.mark.parametrize("argv", [["--env-id", "cma"], ["--env-id", "dma", "--num-envs", "258"],
                                  ["--env-id", "sa", "--opponent", "mirror"],
                                  ["--env-id", "dma", "--num-envs", "258", "--opponent", "mirror"]],
                         ids=["cma", "dma", "mirror-sa", "mirror-dma"])
def test_a_run_with_set_plays_completes_for_every_wrapper(argv, tmp_path, monkeypatch):
    built = spy_on_stagers(monkeypatch)
    params, hist, _ = train(argv + ON + ["--num-updates", "2"], tmp_path / "run")
    assert [h["update"] for h in hist] == [1, 2]
    assert all(torch.isfinite(x).all() for x in params)
    assert all(h["v_loss"] == h["v_loss"] and h["approx_kl"] == h["approx_kl"] for h in hist)
    st = built[-1]
    assert st.call == 17 and int(st.counts.sum()) > 0 and int(st.counts[3:].sum()) == 0


def test_a_policy_opponents_rows_are_staged_too(tmp_path, monkeypatch):
    from vss_amd import setplay as S
    built, views = spy_on_stagers(monkeypatch), []
    stage = S.Stager.stage

    def stage_spy(self, env_state, v, done):
        views.append([tuple(view) for _, view in v])
        stage(self, env_state, v, done)

    monkeypatch.setattr(S.Stager, "stage", stage_spy)
    argv = ["--env-id", "sa", "--opponent", "self", "--num-updates", "2", "--checkpoint-every", "1",
            "--setplay-share", "1", "--setplay-mix", "kickoff,penalty"]
    params, hist, aside = train(argv, tmp_path / "self", copy_at=1)
    assert len(views) == 16 and all(v == [tuple(S.view_sa()), tuple(S.view_opponent())] for v in views)
    assert built[-1].call == 17
    pb, hb, _ = train(argv + ["--resume", aside], tmp_path / "resumed")
    assert_params_equal(params, pb)
    assert training_keys(hist) == training_keys(hb)


def test_all_channels_together_complete_and_resume_bit_equal(tmp_path, monkeypatch):
    built = spy_on_stagers(monkeypatch)
    argv = ["--env-id", "sa", "--opponent", "self", "--num-updates", "3", "--checkpoint-every", "1"] + ON + OBS + ACT
    pa, ha, aside = train(argv, tmp_path / "a", copy_at=2)
    assert built[-1].call == 25
    pb, hb, _ = train(argv + ["--resume", aside], tmp_path / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb)
    assert all(torch.isfinite(x).all() for x in pa)
    assert len(open(P.__file__).read().splitlines()) <= 600
