"""The HIP step kernels on the directed edge table (tests/step_edges.py), bit for bit against the oracle.

tests/test_step_edges_cpu.py proves that every entry of the table tells a mutated oracle from the real one;
here the same entries run through vss_step (FULL), vss_rollout, vss_step_versus, vss_step_mirror and the two
replay entries.  Floats are compared as uint32, so -0.0 and denormals count.  The whole expanded table is one
launch; rolling it by 1, 31, 32 and 33 fields moves every case to both ends of a wave and into the tail wave,
and the n = 1 runs leave one lane pair alone in its wave.
"""
import dataclasses

import numpy as np
import pytest
import torch

import oracle as O
import step_edges as E
from test_gpu_replay import DevEnv
from test_mirror_step import full_actions as mirror_full_actions
from test_mirror_step import mirror_io, team_rewards
from test_versus_step import (DEV, F32, assert_env_equal, bits, device_io, full_actions, host_from, make_vss,
                              oracle_params)

pytestmark = pytest.mark.gpu

STEPS = 2
TABLE = E.table()
MAIN = [c for c in TABLE if c.max_len == E.MAX_LEN]
BASE = E.base_cases()


def rolled(cases, k):
    k %= len(cases)
    return cases[-k:] + cases[:-k] if k else list(cases)


def load(env, cases):
    """Write the cases into a fresh env (one field each) and mirror it on the host; (host env, actions)."""
    state, actions, progress = E.pack(cases)
    env.state.copy_(torch.from_numpy(state))
    env.progress_buf.copy_(torch.from_numpy(progress))
    env.reset_buf.zero_()
    env.dof_velocity_buf.zero_()
    return host_from(env), actions


def same(got, want, cases, what):
    """Bitwise equality of two per-field arrays, naming the cases that differ."""
    g, w = bits(got), bits(want)
    g, w = g.reshape(len(cases), -1), w.reshape(len(cases), -1)
    assert g.dtype.itemsize == w.dtype.itemsize
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} fields differ, first {[cases[i].name for i in bad[:6]]}"


def same_env(env, h, cases, msg):
    torch.cuda.synchronize()
    same(env.state.t().contiguous(), np.ascontiguousarray(h.state.T), cases, msg + " state")
    assert_env_equal(env, h, msg)


def step_full_and_compare(env, h, prm, actions, cases, msg):
    n = len(cases)
    obs_dict, rew, reset, extras = env.step(torch.from_numpy(actions).to(DEV))
    io = O.make_io(n, O.MODE_FULL)
    O.step(h, O.MODE_FULL, actions, io, prm)
    same_env(env, h, cases, msg)
    same(obs_dict["obs"], io["obs"], cases, msg + " obs")
    same(extras["terminal_observation"], io["terminal_obs"], cases, msg + " terminal_obs")
    same(rew, io["rew"], cases, msg + " rew")
    same(extras["time_outs"].cpu().numpy().astype(np.uint8), io["time_outs"], cases, msg + " time_outs")
    same(extras["progress_buffer"], io["progress_f"], cases, msg + " progress_f")
    return io


def test_table_is_not_wave_aligned():
    assert 300 <= len(MAIN) <= 6000 and len(MAIN) % 32 != 0 and len(MAIN) % 64 != 0


@pytest.mark.parametrize("roll", [0, 1, 31, 32, 33])
def test_full_step_on_the_packed_table(roll):
    """vss_step FULL, the whole expanded table in one launch, two consecutive steps."""
    cases = rolled(MAIN, roll)
    env = make_vss(len(cases), max_len=E.MAX_LEN)
    h, actions = load(env, cases)
    prm = oracle_params(env)
    seen = dict(reset=0, timeout=0, goal=0)
    for t in range(STEPS):
        io = step_full_and_compare(env, h, prm, actions, cases, f"roll {roll} step {t}")
        seen["reset"] += int(h.reset.sum())
        seen["timeout"] += int(io["time_outs"].sum())
        seen["goal"] += int((io["rew"][:, 0] != 0).sum())
    assert min(seen.values()) > 0, seen  # on the oracle's side: the table did end episodes both ways


@pytest.mark.parametrize("max_len", [1, 2])
def test_full_step_short_episodes(max_len):
    """The max_len 1 and 2 cases, and the whole table again at that length: every field times out at once."""
    own = [c for c in TABLE if c.max_len == max_len]
    assert own
    cases = own + [dataclasses.replace(c, max_len=max_len) for c in MAIN if c.progress < max_len]
    if len(cases) % 32 == 0:  # keep a tail wave
        cases = cases[:-1]
    env = make_vss(len(cases), max_len=max_len)
    h, actions = load(env, cases)
    prm = oracle_params(env)
    for t in range(STEPS + 1):
        step_full_and_compare(env, h, prm, actions, cases, f"max_len {max_len} step {t}")


@pytest.mark.parametrize("group", ["wall", "rr", "br", "yaw", "drive", "goal"])
def test_full_step_one_field_alone(group):
    """n = 1: each base case (robot index 0, first quadrant) alone in its wave, same bar."""
    cases = [c for c in BASE if c.base.split("/")[0] == group]
    assert cases
    envs = {}
    for c in cases:
        env = envs.get(c.max_len) or envs.setdefault(c.max_len, make_vss(1, max_len=c.max_len))
        h, actions = load(env, [c])
        prm = oracle_params(env)
        for t in range(STEPS):
            step_full_and_compare(env, h, prm, actions, [c], f"{c.name} step {t}")


def test_rollout_on_the_packed_table():
    """vss_rollout, K = 2: physics_split's second call site, on the packed table."""
    cases = MAIN
    n = len(cases)
    env = make_vss(n, max_len=E.MAX_LEN)
    h, actions = load(env, cases)
    prm = oracle_params(env)
    acts = torch.from_numpy(np.stack([actions] * STEPS)).to(DEV).view(STEPS, n, 2, 3, 2)
    out = env.rollout(acts)
    torch.cuda.synchronize()
    for k in range(STEPS):
        io = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, actions, io, prm)
        msg = f"rollout step {k}"
        same(out["obs"][k], io["obs"], cases, msg + " obs")
        same(out["terminal_observation"][k], io["terminal_obs"], cases, msg + " terminal_obs")
        same(out["rew"][k], io["rew"], cases, msg + " rew")
        same(out["dones"][k], h.reset, cases, msg + " dones")
        same(out["time_outs"][k].cpu().numpy().astype(np.uint8), io["time_outs"], cases, msg + " time_outs")
        same(out["progress_buffer"][k], io["progress_f"], cases, msg + " progress_f")
    same_env(env, h, cases, "after rollout")


def controlled(cases, ou_robots):
    """The cases that concern no OU-driven robot (every other robot's command comes from the case)."""
    keep = [c for c in cases if not (c.robots & ou_robots)]
    return keep, len(cases) - len(keep)


def compare_team(out, dones, iof, h, mode, a0, cases, msg):
    n = len(cases)
    A = 3 if mode == O.MODE_DMA else 1
    fobs, fterm = iof["obs"].reshape(n, 6, 52), iof["terminal_obs"].reshape(n, 6, 52)
    rew, rsum = team_rewards(mode, iof["rew"].reshape(n, 6, 4), a0, n * A)
    same(out["obs"], np.ascontiguousarray(fobs[:, a0:a0 + A]), cases, msg + " obs")
    same(out["terminal_obs"], np.ascontiguousarray(fterm[:, a0:a0 + A]), cases, msg + " terminal_obs")
    same(out["rew"], rew, cases, msg + " rew")
    same(out["reward_sum"], rsum, cases, msg + " reward_sum")
    same(out["time_outs"].cpu().numpy().astype(np.uint8), np.repeat(iof["time_outs"], A), cases, msg + " time_outs")
    same(out["progress_f"], np.repeat(iof["progress_f"], A), cases, msg + " progress_f")
    if dones is not None:
        same(dones, np.repeat(h.reset, A), cases, msg + " dones")


@pytest.mark.parametrize("mode", [O.MODE_SA, O.MODE_DMA])
def test_versus_step_on_the_packed_table(mode):
    """vss_step_versus: the yellow commands come through the opponent buffer, so all twelve are the case's,
    except SA's blue robots 1-2 (OU-driven): the cases that concern them are left out there."""
    cases, dropped = controlled(MAIN, frozenset({1, 2}) if mode == O.MODE_SA else frozenset())
    assert dropped <= len(MAIN) // 3  # the expansion over the robot index keeps four indices of six
    n = len(cases)
    env = make_vss(n, max_len=E.MAX_LEN)
    h, actions = load(env, cases)
    prm = oracle_params(env)
    learner = np.ascontiguousarray(actions[:, :2] if mode == O.MODE_SA else actions[:, :6].reshape(3 * n, 2))
    opp = np.ascontiguousarray(actions[:, 6:].reshape(n, 3, 2))
    io = device_io(n, mode)
    opp_act, opp_obs = torch.from_numpy(opp).to(DEV), torch.zeros((n, 3, 52), device=DEV)
    exp_ou = np.zeros((n, 12), F32)
    for t in range(STEPS):
        env.native_step_versus(mode, torch.from_numpy(learner).to(DEV), io, opp_act, opp_obs)
        full = full_actions(mode, n, learner, opp, exp_ou, h.ctr.copy(), prm)
        iof = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, full, iof, prm)
        msg = f"versus mode {mode} step {t}"
        same_env(env, h, cases, msg)
        compare_team(io, io["dones_rep"], iof, h, mode, 0, cases, msg)
        same(opp_obs, np.ascontiguousarray(iof["obs"].reshape(n, 6, 52)[:, 3:6]), cases, msg + " opp_obs")
        exp_ou = np.where(h.reset[:, None] != 0, full * F32(0.0), full).astype(F32)
        same(io["ou_buf"], exp_ou, cases, msg + " ou_buf")


@pytest.mark.parametrize("mode", [O.MODE_SA, O.MODE_DMA])
def test_mirror_step_on_the_packed_table(mode):
    """vss_step_mirror: both teams' commands are learner rows.  In SA robots 1-2 of BOTH teams are OU-driven,
    which leaves the cases about robots 0 and 3 alone (every one- and two-robot base case at least once, and
    every ball-only case); DMA runs the whole table."""
    cases, dropped = controlled(MAIN, frozenset({1, 2, 4, 5}) if mode == O.MODE_SA else frozenset())
    assert mode == O.MODE_SA or dropped == 0
    assert {b.name for b in E.BASES if b.k <= 2 and not b.split and b.build(0).max_len == E.MAX_LEN} <= {c.base for c in cases}
    n = len(cases)
    env = make_vss(n, max_len=E.MAX_LEN)
    h, actions = load(env, cases)
    prm = oracle_params(env)
    if mode == O.MODE_SA:
        both = np.stack([actions[:, 0:2], actions[:, 6:8]])
    else:
        both = np.stack([actions[:, :6].reshape(3 * n, 2), actions[:, 6:].reshape(3 * n, 2)])
    both = np.ascontiguousarray(both, F32)
    io, yl = mirror_io(n, mode)
    exp_ou = np.zeros((n, 12), F32)
    for t in range(STEPS):
        env.native_step_mirror(mode, torch.from_numpy(both).to(DEV), io, yl)
        full = mirror_full_actions(mode, n, both[0], both[1], exp_ou, h.ctr.copy(), prm)
        iof = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, full, iof, prm)
        msg = f"mirror mode {mode} step {t}"
        same_env(env, h, cases, msg)
        compare_team(io, io["dones_rep"], iof, h, mode, 0, cases, msg + " blue")
        compare_team(yl, yl["dones"], iof, h, mode, 3, cases, msg + " yellow")
        exp_ou = np.where(h.reset[:, None] != 0, full * F32(0.0), full).astype(F32)
        same(io["ou_buf"], exp_ou, cases, msg + " ou_buf")


# ------------------------------------------------------------------------------------ reset cases
RESET = E.reset_cases()
REPLAY_PRM = dict(w_goal=10.0, w_grad=2.0, w_move=3.0, w_energy=0.0, clip_actions=1.0, seed=1)  # DevEnv's


@pytest.mark.parametrize("case", RESET, ids=[c.name for c in RESET])
def test_reset_dones_replay_on_the_reset_cases(case):
    """vss_reset_dones_replay against oracle_reset_dones with the same injected uniforms."""
    dev = DevEnv(1, O.MODE_FULL)
    dev.reset_dones(case.row[None, :], E.MAX_LEN)
    h = O.HostEnv(1)
    d, keep = O.make_draws(case.row, np.zeros(0, F32))
    O.reset_dones(h, O.params(max_episode_length=E.MAX_LEN, **REPLAY_PRM), d)
    np.testing.assert_array_equal(bits(dev.state), h.state.view(np.uint32), err_msg=case.name)
    np.testing.assert_array_equal(bits(dev.dof), h.dof.view(np.uint32))
    np.testing.assert_array_equal(dev.ctr.cpu().numpy().view(np.uint32), h.ctr)
    np.testing.assert_array_equal(dev.reset.cpu().numpy(), h.reset)


@pytest.mark.parametrize("case", RESET, ids=[c.name for c in RESET])
def test_step_replay_on_the_reset_cases(case):
    """vss_step_replay (FULL): a field that times out in this step and is re-placed from the injected uniforms."""
    f = E.Field().robot(0, 0.1, 0.1, act=(0.5, -0.25)).ball(0.2, -0.1, 0.3, 0.1)
    dev = DevEnv(1, O.MODE_FULL)
    dev.state.copy_(torch.from_numpy(f.s[:, None].copy()))
    dev.reset.zero_()
    actions = f.a[None, :].copy()
    dev.step(actions, case.row[None, :], None, 1)
    h = O.HostEnv(1)
    h.state[:, 0], h.reset[:] = f.s, 0
    io = O.make_io(1, O.MODE_FULL)
    d, keep = O.make_draws(case.row, np.zeros(0, F32))
    O.step(h, O.MODE_FULL, actions, io, O.params(max_episode_length=1, **REPLAY_PRM), d)
    assert h.reset[0] == 1 and io["time_outs"][0] == 1
    np.testing.assert_array_equal(bits(dev.state), h.state.view(np.uint32), err_msg=case.name)
    np.testing.assert_array_equal(dev.reset.cpu().numpy(), h.reset)
    np.testing.assert_array_equal(dev.progress.cpu().numpy(), h.progress)
    np.testing.assert_array_equal(bits(dev.dof), h.dof.view(np.uint32))
    np.testing.assert_array_equal(dev.ctr.cpu().numpy().view(np.uint32), h.ctr)
    for k in ("obs", "terminal_obs", "rew", "progress_f"):
        np.testing.assert_array_equal(bits(dev.io[k]).reshape(-1), io[k].view(np.uint32).reshape(-1), err_msg=f"{case.name} {k}")
    np.testing.assert_array_equal(dev.host("time_outs"), io["time_outs"])
