"""--ref-* in the train loop (envs/wrappers.py set_referee): with the flags at their defaults the run is
the run without them, bit for bit and wrapper for wrapper -- also when the keys are absent from args altogether; with
the flags set the run completes, records referee/* per update (they sum to the referee's counts), the arena reports
its stoppages, a resumed run is the unbroken run, and another threshold is refused."""
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from test_estimate_train import wrapper_chain
from test_eval_train import COMMON, EVAL, assert_params_equal, train, training_keys
from vss_amd import checkpoint as CK

pytestmark = pytest.mark.gpu
SA = ["--env-id", "sa", "--num-updates", "2"]
DEFAULTS = ["--ref-stall-steps", "0", "--ref-area-steps", "0", "--ref-stall-speed", "0.1", "--ref-max-stops", "3"]
# a goal area 0.35 m deep and 1.30 m wide and two steps, so that all three calls occur in 16 steps of 256 fields
ON = ["--ref-stall-steps", "3", "--ref-area-steps", "2", "--ref-area-depth", "0.35", "--ref-area-width", "1.3"]
KEYS = ("referee/free_ball", "referee/penalty_for", "referee/penalty_against", "referee/goal_kick_for",
        "referee/goal_kick_against")


def train_without_the_keys(argv, save_path):
    """test_eval_train.train with the ref_* keys deleted from args: a caller that predates the flags."""
    args = P.parse_args(COMMON + argv + ["--save-path", str(save_path)])
    for k in CK.REFEREE_STRUCTURAL:
        delattr(args, k)
    agent, hist = P.train(args)
    return [p.detach().clone() for p in agent.parameters()], hist


def spy_on_referees(monkeypatch):
    from vss_amd import referee as R
    built, init = [], R.Referee.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    monkeypatch.setattr(R.Referee, "__init__", spy)
    return built


def test_the_defaults_are_the_run_without_the_flags(tmp_path, monkeypatch):
    built = spy_on_referees(monkeypatch)
    for extra in ([], ["--env-id", "dma"], ["--opponent", "mirror"], ["--setplay-share", "0.5"],
                  ["--obs-delay", "2", "--obs-noise-pos", "0.002"]):
        assert wrapper_chain(extra) == wrapper_chain(extra + DEFAULTS) == wrapper_chain(extra + ON)  # no wrapper is added
    assert len(built) == 5                              # only the five chains with the flags set built a referee
    p0, h0, _ = train(SA, tmp_path / "plain")
    p1, h1, _ = train(SA + DEFAULTS, tmp_path / "defaults")
    p2, h2 = train_without_the_keys(SA, tmp_path / "absent")
    assert len(built) == 5
    assert_params_equal(p0, p1)
    assert_params_equal(p0, p2)
    assert training_keys(h0) == training_keys(h1) == training_keys(h2)
    assert not any(k.startswith("referee/") for h in h0 + h1 + h2 for k in h)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("referee")
    built = []
    from vss_amd import referee as R
    init = R.Referee.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self)

    R.Referee.__init__ = spy
    try:
        a = train(SA + ON + EVAL + ["--eval-teams", "zero", "--checkpoint-every", "1"], root / "a", copy_at=1)
    finally:
        R.Referee.__init__ = init
    return dict(root=root, a=a, built=built)


def test_two_updates_run_and_the_record_sums_to_the_counts(runs):
    params, hist, _ = runs["a"]
    training, arena = runs["built"]                     # make_env's, then the arena's own
    assert [h["update"] for h in hist] == [1, 2] and all(torch.isfinite(x).all() for x in params)
    assert all(set(KEYS) <= set(h) and all(isinstance(h[k], int) and h[k] >= 0 for k in KEYS) for h in hist)
    c = training.counts.tolist()
    total = {k: sum(h[k] for h in hist) for k in KEYS}
    assert total == {KEYS[0]: sum(c[:4]), KEYS[1]: c[4], KEYS[2]: c[5], KEYS[3]: c[6], KEYS[4]: c[7]}
    assert training.call_index == 16 and total[KEYS[0]] > 0 and sum(c[4:]) > 0
    print("referee/* per update", [{k: h[k] for k in KEYS} for h in hist])
    # the arena's referee: a key of its own, the same table and parameters; its counts are the last play's
    assert arena.seed != training.seed and arena.params == training.params and arena.n_fields == 64
    for h in hist:
        stops = h["eval"]["zero"]["stoppages"]
        assert len(stops) == 8 and all(isinstance(v, int) for v in stops) and sum(stops[:4]) > 0
    assert hist[-1]["eval"]["zero"]["stoppages"] == arena.counts.tolist()


def test_a_resumed_run_is_the_unbroken_run_and_another_threshold_is_refused(runs):
    pa, ha, aside = runs["a"]
    argv = SA + ON + EVAL + ["--eval-teams", "zero", "--checkpoint-every", "1"]
    pb, hb, _ = train(argv + ["--resume", aside], runs["root"] / "resumed")
    assert_params_equal(pa, pb)
    assert training_keys(ha) == training_keys(hb) and hb[1]["eval"] == ha[1]["eval"]
    assert [{k: h[k] for k in KEYS} for h in ha] == [{k: h[k] for k in KEYS} for h in hb]
    with pytest.raises(ValueError, match="ref_stall_steps"):
        train(SA + ["--ref-stall-steps", "4"] + ON[2:] + EVAL + ["--eval-teams", "zero", "--resume", aside],
              runs["root"] / "refused")
    with pytest.raises(ValueError, match="ref_stall_steps"):
        train(SA + ["--resume", aside], runs["root"] / "refused2")


@pytest.mark.parametrize("argv", [["--env-id", "dma", "--num-envs", "258"], ["--env-id", "sa", "--opponent", "mirror"],
                                  ["--env-id", "sa", "--opponent", "self", "--setplay-share", "0.5"]],
                         ids=["dma", "mirror-sa", "self+setplays"])
def test_a_run_with_a_referee_completes_for_other_wrappers(argv, tmp_path, monkeypatch):
    built = spy_on_referees(monkeypatch)
    params, hist, _ = train(argv + ON + ["--num-updates", "2"], tmp_path / "run")
    assert [h["update"] for h in hist] == [1, 2] and all(torch.isfinite(x).all() for x in params)
    ref = built[-1]
    assert ref.call_index == 16 and int(ref.counts.sum()) == sum(h[k] for h in hist for k in KEYS) > 0
    assert len(open(P.__file__).read().splitlines()) <= 600
