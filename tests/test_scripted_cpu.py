"""The scripted benchmark team without a GPU (include/vss.h vss_scripted_team, vss_amd/scripted.py):
the ABI entry's argument checks, the float32 specification `reference_actions` (range, y-mirror symmetry, known
answers), its strength on the unchanged CPU oracle, and the Python plumbing around it (TeamScripted's state dict,
the checkpoint's structural `scripted` mode, the --eval-every flags)."""
import argparse
import re

import numpy as np
import pytest
import torch

import oracle as O
import ppo_continuous_action_isaacgym as P
from vss_amd import _native as N
from vss_amd import checkpoint as CK
from vss_amd import minibatch as MB
from vss_amd import scripted as S

F32 = np.float32
FAKE = 4096  # non-null, 16-B aligned, never dereferenced: every call below returns before a launch
E_ARG = 1


def call(n_fields=64, version=1, obs=FAKE, obs_stride=156, act=FAKE, act_stride=6):
    return N.load().vss_scripted_team(None, n_fields, version, obs, obs_stride, act, act_stride)


def random_rows(n, seed):
    """Consistent robot-0 rows (n, 52): everything on or near the field, unit headings, actions in [-1, 1]."""
    g = np.random.default_rng(seed)
    rows = np.zeros((n, 52), F32)

    def body(b):
        rows[:, b] = g.uniform(-0.8, 0.8, n)
        rows[:, b + 1] = g.uniform(-0.65, 0.65, n)
        rows[:, b + 2:b + 4] = g.uniform(-1.5, 1.5, (n, 2))

    body(0)
    for k in range(6):
        b = 4 + 9 * k if k < 3 else 31 + 7 * (k - 3)
        body(b)
        yaw = g.uniform(-np.pi, np.pi, n)
        rows[:, b + 4], rows[:, b + 5] = np.cos(yaw), np.sin(yaw)
        rows[:, b + 6] = g.uniform(-20, 20, n)
        if k < 3:
            rows[:, b + 7:b + 9] = g.uniform(-1, 1, (n, 2))
    return rows


def set_robot(rows, k, x, y, c, s):
    b = 4 + 9 * k
    rows[:, b], rows[:, b + 1], rows[:, b + 4], rows[:, b + 5] = x, y, c, s


def edge_rows():
    """Rows at the controller's corners: a robot exactly on its target, the ball exactly on a robot, the ball on
    the goal line (g has length 0 at the goal's centre), and e_f exactly 0 (the target straight to the side)."""
    rows = random_rows(8, 99)
    rows[0, 0:2] = (0.2, 0.1)
    set_robot(rows[0:1], 2, F32(-0.69), F32(0.1), 0.6, 0.8)        # the keeper on its target
    rows[1, 0:2] = (0.3, -0.5)
    set_robot(rows[1:2], 1, F32(-0.30), F32(-0.35), 1.0, 0.0)      # the defender on its (clamped) target
    rows[2, 0:2] = (0.1, 0.2)
    set_robot(rows[2:3], 0, F32(0.1), F32(0.2), 0.0, 1.0)          # the ball on the attacker
    rows[3, 0:2] = (-0.4, 0.0)
    set_robot(rows[3:4], 1, F32(-0.4), F32(0.0), -1.0, 0.0)        # the ball on the defender while it attacks
    rows[4, 0:2] = (0.75, 0.0)                                     # the ball at the goal's centre: g = 0
    rows[5, 0:2] = (0.75, 0.15)                                    # the ball on the goal line
    rows[6, 0:2] = (0.0, 0.1)
    set_robot(rows[6:7], 2, F32(-0.69), F32(0.0), 1.0, 0.0)        # keeper facing +x, target straight left: e_f = 0
    rows[7, 0:2] = (-0.75, 0.0)
    set_robot(rows[7:8], 0, F32(-0.85), F32(0.0), 0.0, -1.0)       # target on the x axis, robot facing -y: e_f = 0
    return rows


def test_the_symbol_is_exported_and_declared_and_the_abi_version_stays():
    assert "vss_scripted_team" in N.EXPORTED
    header = open(N.HEADER).read()
    assert re.search(r"\bint\s+vss_scripted_team\s*\(", header)
    assert re.search(r"#define\s+VSS_SCRIPTED_VERSION\s+1\b", header)
    assert N.load().vss_abi_version() == 2 == N.ABI_VERSION
    assert S.VERSION == 1 == N.SCRIPTED_VERSION


def test_rejected_calls_and_the_zero_size_call():
    assert call(obs=None) == E_ARG and call(act=None) == E_ARG
    assert call(n_fields=0, obs=None) == E_ARG  # checked before the zero-size return
    for off in (4, 8, 12, 1):
        assert call(obs=FAKE + off) == E_ARG, off
    for off in (4, 2, 1):
        assert call(act=FAKE + off) == E_ARG, off
    for stride in (51, 48, 0, -156, 53, 54, 55, 158):
        assert call(obs_stride=stride) == E_ARG, stride
    for stride in (5, 4, 0, -6, 7, 13):
        assert call(act_stride=stride) == E_ARG, stride
    for version in (0, 2, -1):
        assert call(version=version) == E_ARG, version
    assert call(n_fields=-1) == E_ARG
    assert call(n_fields=0) == 0
    assert call(n_fields=0, obs_stride=312, act_stride=12) == 0
    assert call(n_fields=0, version=2) == E_ARG


def test_reference_actions_are_finite_and_within_the_wheel_range():
    rows = np.concatenate([random_rows(5000, 1), edge_rows()])
    a = S.reference_actions(rows)
    assert a.shape == (5008, 3, 2) and a.dtype == F32
    assert np.isfinite(a).all() and np.abs(a).max() <= 1.0
    assert (np.abs(a) > 0.05).mean() > 0.9  # and it moves


def test_the_y_mirror_swaps_each_robots_wheels_bit_for_bit():
    rows = np.concatenate([random_rows(5000, 2), edge_rows()])
    a, m = S.reference_actions(rows), S.reference_actions(S.mirror_rows_y(rows))
    a, m = a + F32(0), m[:, :, ::-1] + F32(0)  # -0 + 0 = +0: the sign of a zero is ignored
    np.testing.assert_array_equal(a.view(np.uint32), np.ascontiguousarray(m).view(np.uint32))
    assert (a[:, :, 0] != a[:, :, 1]).mean() > 0.9  # the swap is seen: most rows turn


def test_it_depends_on_robot_0s_row_alone():
    rows = random_rows(64, 3)
    obs = torch.full((64, 3, 52), float("nan"))
    obs[:, 0] = torch.from_numpy(rows)
    act = torch.zeros((64, 3, 2))
    S.scripted_actions(act, obs)
    np.testing.assert_array_equal(act.numpy().view(np.uint32), S.reference_actions(rows).view(np.uint32))
    # and within the row on the ball's position and the own robots' positions and headings alone
    used = [0, 1] + [4 + 9 * k + q for k in range(3) for q in (0, 1, 4, 5)]
    other = rows.copy()
    other[:, [i for i in range(52) if i not in used]] = np.nan
    np.testing.assert_array_equal(S.reference_actions(other).view(np.uint32), S.reference_actions(rows).view(np.uint32))


def test_unexpressible_layouts_are_refused_naming_the_stride():
    obs, act = torch.zeros((4, 3, 52)), torch.zeros((4, 3, 2))
    with pytest.raises(ValueError, match="stride 157"):
        S.field_strides(act, torch.zeros((4, 157))[:, :52])
    with pytest.raises(ValueError, match="stride 7"):
        S.field_strides(torch.zeros((4, 7))[:, :6].view(4, 3, 2), obs)
    with pytest.raises(ValueError, match="element stride 2"):
        S.field_strides(act, torch.zeros((4, 3, 104))[:, :, ::2])
    with pytest.raises(ValueError, match="strides"):
        S.field_strides(torch.zeros((4, 3, 4))[:, :, :2], obs)
    assert S.field_strides(act, obs) == (156, 6)
    full_obs, full_act = torch.zeros((4, 2, 3, 52)), torch.zeros((4, 2, 3, 2))
    assert S.field_strides(full_act[:, 1], full_obs[:, 1]) == (312, 12)
    assert S.field_strides(act, obs[:, 0]) == (156, 6)


def one_row(ball, robots):
    """A row with the ball at rest at `ball` and own robot k at rest at robots[k] = (x, y, cos, sin)."""
    rows = np.zeros((1, 52), F32)
    rows[0, 0:2] = ball
    for k, (x, y, c, s) in enumerate(robots):
        set_robot(rows, k, x, y, c, s)
    for k in range(3):
        rows[0, 31 + 7 * k: 33 + 7 * k] = (0.5, (-0.3, 0.0, 0.3)[k])
        rows[0, 35 + 7 * k] = -1.0
    return rows


def test_known_answer_the_attacker_behind_the_ball_drives_straight_through_it():
    """Robot 0 at rest at the centre facing +x, the ball 0.3 m ahead of it on the line to the opponent goal."""
    a = S.reference_actions(one_row((0.3, 0.0), [(0.0, 0.0, 1, 0), (-0.3, 0.3, 1, 0), (-0.69, 0.0, 0, 1)]))
    assert a[0, 0, 0] == a[0, 0, 1] and a[0, 0, 0] > 0


def test_known_answer_the_defender_chases_a_ball_deep_in_its_half_like_the_attacker():
    a = S.reference_actions(one_row((-0.3, 0.0), [(0.5, 0.5, 1, 0), (-0.6, 0.0, 1, 0), (-0.69, 0.0, 0, 1)]))
    assert a[0, 1, 0] == a[0, 1, 1] and a[0, 1, 0] > 0


def test_known_answer_the_keeper_on_its_line_drives_towards_the_balls_y():
    """The keeper on its line at y = 0 facing +y, the ball at y = +0.1: forward, both wheels equal."""
    a = S.reference_actions(one_row((0.2, 0.1), [(0.0, 0.0, 1, 0), (-0.3, 0.3, 1, 0), (-0.69, 0.0, 0, 1)]))
    assert a[0, 2, 0] == a[0, 2, 1] and a[0, 2, 0] > 0
    # facing -y it reverses instead of turning round
    b = S.reference_actions(one_row((0.2, 0.1), [(0.0, 0.0, 1, 0), (-0.3, 0.3, 1, 0), (-0.69, 0.0, 0, -1)]))
    assert b[0, 2, 0] == b[0, 2, 1] and b[0, 2, 0] < 0


# ---- strength on the unchanged CPU oracle: FULL mode, goal-only reward ----------------------------------------------

def oracle_match(blue, yellow, n=256, steps=800, seed=1):
    """(episodes, blue wins, blue losses) of `steps` FULL steps on `n` fields; teams: scripted / zero / ou."""
    h = O.HostEnv(n)
    prm = O.params(1.0, 0.0, 0.0, 0.0, 1.0, 400, seed)
    O.reset_dones(h, prm)
    obs = O.compute_obs(h, 6)
    rng = np.random.default_rng(seed)
    ou = np.zeros((n, 2, 3, 2), F32)
    io = O.make_io(n, O.MODE_FULL)
    episodes = wins = losses = 0
    for _ in range(steps):
        act = np.zeros((n, 2, 3, 2), F32)
        for side, kind in ((0, blue), (1, yellow)):
            if kind == "scripted":
                act[:, side] = S.reference_actions(obs[:, 3 * side])
            elif kind == "ou":  # random_ou of envs/wrappers.py on a buffer zeroed at every reset
                prev = ou[:, side]
                ou[:, side] = np.clip(prev - F32(0.1) * prev + rng.normal(0, 0.15, prev.shape).astype(F32), -1, 1)
                act[:, side] = ou[:, side]
        O.step(h, O.MODE_FULL, act.reshape(n, 12), io, prm)
        obs = io["obs"].reshape(n, 6, 52)
        done, goal = h.reset != 0, io["rew"][:, 0]
        episodes += int(done.sum())
        wins += int((done & (goal > 0)).sum())
        losses += int((done & (goal < 0)).sum())
        ou[done] = 0
    return episodes, wins, losses


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("blue,yellow", [("scripted", "zero"), ("scripted", "ou"), ("ou", "scripted")])
def test_strength_the_scripted_side_wins_at_least_twice_as_often_as_it_loses(blue, yellow, seed):
    episodes, wins, losses = oracle_match(blue, yellow, seed=seed)
    own_wins, own_losses = (wins, losses) if blue == "scripted" else (losses, wins)
    print(f"{blue} vs {yellow} seed {seed}: episodes {episodes}, blue wins {wins}, blue losses {losses}")
    assert episodes > 0
    assert own_wins >= 2 * own_losses


# ---- the plumbing ----------------------------------------------------------------------------------------------------

def test_team_scripted_state_dict_round_trip_and_the_refusal_of_another_version():
    from play import Team, TeamScripted, baseline_teams, get_team
    team = get_team("scripted")
    assert isinstance(team, TeamScripted) and isinstance(team, Team) and team.version == 1
    assert team.state_dict() == {"version": 1}
    TeamScripted().load_state_dict(team.state_dict())
    for bad in ({"version": 2}, {"version": None}, {}):
        with pytest.raises(ValueError, match="version"):
            team.load_state_dict(bad)
    assert sorted(baseline_teams(root="no/such/dir")) == ["ou", "zero"]  # what it returned before


def test_team_scripted_on_cpu_tensors_is_the_reference():
    from play import get_team
    rows = random_rows(33, 5)
    obs = torch.zeros((33, 2, 3, 52))
    obs[:, 1, 0] = torch.from_numpy(rows)
    act = torch.full((33, 2, 3, 2), 7.0)
    get_team("scripted")(act[:, 1], obs[:, 1])
    np.testing.assert_array_equal(act[:, 1].numpy().view(np.uint32), S.reference_actions(rows).view(np.uint32))
    assert bool((act[:, 0] == 7.0).all())


def test_scripted_is_a_structural_opponent_mode_of_its_own():
    assert CK.opponent_mode("scripted") == "scripted"
    assert [CK.opponent_mode(v) for v in (None, "ou", "self", "pool", "mirror", "runs/a/agent.pt")] == \
        ["ou", "ou", "self", "pool", "mirror", "checkpoint"]
    saved = CK.plain_args(P.parse_args(["--opponent", "scripted"]))
    for other in ("ou", "self", "runs/a/agent.pt"):
        with pytest.raises(ValueError, match="opponent"):
            CK.check_compatible(saved, P.parse_args(["--opponent", other]), log=None)
        with pytest.raises(ValueError, match="opponent"):
            CK.check_compatible(CK.plain_args(P.parse_args(["--opponent", other])), P.parse_args(["--opponent", "scripted"]),
                                log=None)
    assert CK.check_compatible(saved, P.parse_args(["--opponent", "scripted"]), log=None) == []


def test_eval_every_defaults_and_team_names():
    from vss_amd.arena import parse_teams, score
    args = P.parse_args([])
    assert args.eval_every == 0 and args.eval_fields == 1024 and args.eval_teams == "zero,ou,scripted"
    args = P.parse_args(["--eval-every", "5", "--eval-fields", "64", "--eval-teams", "scripted"])
    assert (args.eval_every, args.eval_fields, args.eval_teams) == (5, 64, "scripted")
    assert parse_teams("zero,ou,scripted") == ["zero", "ou", "scripted"] and parse_teams(" ou , zero ") == ["ou", "zero"]
    for bad in ("", "zero,zero", "self", "zero,base"):
        with pytest.raises(ValueError, match="eval-teams"):
            parse_teams(bad)
    assert score(30, 10, 64) == 20 / 64 and score(0, 0, 0) == 0.0
    assert "eval_every" not in CK.STRUCTURAL  # a resumed run may switch it on, off or to another K


def test_warmup_kernels_clears_eval_every():
    args = P.parse_args(["--eval-every", "2"])
    seen = []
    MB.warmup_kernels(args, lambda w: seen.append(argparse.Namespace(**vars(w))))
    assert seen[0].eval_every == 0 and args.eval_every == 2
