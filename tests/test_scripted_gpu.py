"""vss_scripted_team on the GPU (csrc/vss_scripted.hip): the kernel equals its float32 specification
vss_amd.scripted.reference_actions bit for bit -- on single rows, in closed loop against the CPU oracle with both
teams driven by it through goals, resets and time-outs, and as the wrapper's opponent -- and writes nothing but its
six floats per field."""
import numpy as np
import pytest
import torch

import oracle as O
from test_scripted_cpu import edge_rows, random_rows
from vss_amd import _native as N
from vss_amd import scripted as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SENTINEL = 0x7FA5A5A5  # tests/test_write_extents.py's quiet-NaN pattern


def make_vss(n, max_len=400, seed=1234):
    from envs.vss import VSS, default_cfg
    cfg = default_cfg(n)
    cfg["env"]["maxEpisodeLength"] = max_len
    cfg["env"]["seed"] = seed
    return VSS(cfg, DEV, DEV, 0, True, False, False)


def host_from(env) -> O.HostEnv:
    h = O.HostEnv(env.num_fields)
    h.state[:] = env.state.cpu().numpy()
    h.progress[:] = env.progress_buf.cpu().numpy()
    h.reset[:] = env.reset_buf.cpu().numpy()
    h.dof[:] = env.dof_velocity_buf.reshape(-1, 12).cpu().numpy()
    h.ctr[:] = env.rng_counter.cpu().numpy().view(np.uint32)
    return h


def oracle_params(env):
    return O.params(env.w_goal, env.w_grad, env.w_move, env.w_energy, env.clip_actions, env.max_episode_length, env.seed)


def assert_env_equal(env, h, msg=""):
    torch.cuda.synchronize()
    np.testing.assert_array_equal(env.state.cpu().numpy().view(np.uint32), h.state.view(np.uint32), err_msg=msg + " state")
    np.testing.assert_array_equal(env.progress_buf.cpu().numpy(), h.progress, err_msg=msg + " progress")
    np.testing.assert_array_equal(env.reset_buf.cpu().numpy(), h.reset, err_msg=msg + " reset")
    np.testing.assert_array_equal(env.dof_velocity_buf.reshape(-1, 12).cpu().numpy().view(np.uint32),
                                  h.dof.view(np.uint32), err_msg=msg + " dof")
    np.testing.assert_array_equal(env.rng_counter.cpu().numpy().view(np.uint32), h.ctr, err_msg=msg + " ctr")


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def rows_for(n):
    """The edge rows first, then random consistent rows."""
    return np.concatenate([edge_rows(), random_rows(max(n, 1), 7000 + n)])[:n]


def kernel_actions(rows, obs_stride, act_stride):
    """The kernel's (n, 3, 2) actions from `rows` placed as robot 0's rows of a layout with the given strides; the
    rest of obs is NaN, the rest of act a sentinel that must survive."""
    n = rows.shape[0]
    obs = torch.full((n, obs_stride), float("nan"), device=DEV)
    obs[:, :52] = torch.from_numpy(rows).to(DEV)
    act = torch.full((n, act_stride), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    S.scripted_actions(act[:, :6].view(n, 3, 2), obs[:, :52])
    torch.cuda.synchronize()
    assert bool((act.view(torch.int32)[:, 6:] == SENTINEL).all())
    return act[:, :6].reshape(n, 3, 2)


@pytest.mark.parametrize("strides", [(156, 6), (312, 12)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_the_kernel_equals_reference_actions_bit_for_bit(n, strides):
    rows = rows_for(n)
    np.testing.assert_array_equal(bits(kernel_actions(rows, *strides)), bits(S.reference_actions(rows)))


@pytest.mark.parametrize("strides", [(156, 6), (312, 12)])
def test_every_edge_row_alone_in_one_lane(strides):
    """n = 1: robot on its target, ball on a robot, ball on the goal line, e_f exactly 0 -- one launch each."""
    rows = edge_rows()
    want = S.reference_actions(rows)
    for i in range(rows.shape[0]):
        np.testing.assert_array_equal(bits(kernel_actions(rows[i:i + 1], *strides)), bits(want[i:i + 1]), err_msg=f"edge row {i}")


@pytest.mark.parametrize("n", [1, 65])
def test_write_extents_and_unread_rows(n):
    """One team's half of (N,2,3,52) / (N,2,3,2) inside guard bands: the other team's six floats per field keep the
    sentinel, the guards stay intact, and rows 1-2 (NaN, like the whole other team) are not read."""
    from test_write_extents import Guarded
    rows = rows_for(n)
    want = bits(S.reference_actions(rows))
    for team in (0, 1):
        fill = torch.full((n, 2, 3, 52), float("nan"), device=DEV)
        fill[:, team, 0] = torch.from_numpy(rows).to(DEV)
        obs, act = Guarded((n, 2, 3, 52), fill=fill), Guarded((n, 2, 3, 2))
        obs.snapshot()
        S.scripted_actions(act.t[:, team], obs.t[:, team])
        torch.cuda.synchronize()
        assert obs.unchanged() and act.guards_intact()
        assert bool((act.t[:, 1 - team].view(torch.int32) == SENTINEL).all()), "the other team's actions were written"
        np.testing.assert_array_equal(bits(act.t[:, team]), want)
    # a contiguous (N,3,52) team block and (N,3,2): every float of act is written
    fill = torch.full((n, 3, 52), float("nan"), device=DEV)
    fill[:, 0] = torch.from_numpy(rows).to(DEV)
    obs, act = Guarded((n, 3, 52), fill=fill), Guarded((n, 3, 2))
    S.scripted_actions(act.t, obs.t)
    torch.cuda.synchronize()
    assert act.guards_intact() and act.covered()
    np.testing.assert_array_equal(bits(act.t), want)


def test_the_binding_refuses_what_the_abi_cannot_express():
    obs, act = torch.zeros((4, 3, 52), device=DEV), torch.zeros((4, 3, 2), device=DEV)
    with pytest.raises(ValueError, match="stride 157"):
        S.scripted_actions(act, torch.zeros((4, 157), device=DEV)[:, :52])
    with pytest.raises(ValueError, match="float32"):
        S.scripted_actions(act, obs.double())
    with pytest.raises(ValueError, match="act is on"):
        S.scripted_actions(act.cpu(), obs)
    with pytest.raises(N.NativeError, match="vss_scripted_team"):
        S.scripted_actions(act, obs, version=2)
    S.scripted_actions(torch.zeros((0, 3, 2), device=DEV), torch.zeros((0, 3, 52), device=DEV))  # no launch


def test_closed_loop_both_teams_against_the_oracle_through_goals_resets_and_a_time_out():
    """A raw FULL env of 67 fields, both teams driven by the kernel for 450 steps (past the time-out at 400), against
    the CPU oracle's FULL step driven by reference_actions from the same state: the actions are bit-equal at every
    step, the whole env state every 50 steps and at the end.  One ulp anywhere in the controller would change a
    wheel command, then the physics, then every later row."""
    n, steps = 67, 450
    env = make_vss(n, max_len=400, seed=4242)
    h, prm = host_from(env), oracle_params(env)
    obs_h = O.compute_obs(h, 6)
    obs = env.reset()["obs"]
    np.testing.assert_array_equal(bits(obs).reshape(n, 6, 52), bits(obs_h))
    act = torch.zeros((n, 2, 3, 2), device=DEV)
    io = O.make_io(n, O.MODE_FULL)
    resets = goals = timeouts = 0
    for t in range(steps):
        S.scripted_actions(act[:, 0], obs[:, 0])
        S.scripted_actions(act[:, 1], obs[:, 1])
        want = np.stack([S.reference_actions(obs_h[:, 0]), S.reference_actions(obs_h[:, 3])], 1)
        np.testing.assert_array_equal(bits(act), bits(want), err_msg=f"actions at step {t}")
        obs = env.step(act)[0]["obs"]
        O.step(h, O.MODE_FULL, want.reshape(n, 12), io, prm)
        obs_h = io["obs"].reshape(n, 6, 52)
        resets += int(h.reset.sum())
        goals += int((np.abs(io["rew"][:, 0]) > 0).sum())
        timeouts += int(io["time_outs"].sum())
        if (t + 1) % 50 == 0 or t + 1 == steps:
            assert_env_equal(env, h, f"step {t}")
            np.testing.assert_array_equal(bits(obs).reshape(n, 6, 52), bits(obs_h), err_msg=f"obs at step {t}")
    assert goals > 0 and timeouts > 0 and resets >= goals


def test_through_the_wrapper_as_the_yellow_team():
    """A CMA wrapper with set_opponent(TeamScripted()), zero learner actions, 120 steps: bit-equal to the oracle's
    FULL step on [0 | reference_actions(the yellow rows)]."""
    from envs.wrappers import CMA
    from play import TeamScripted
    n = 33
    env = make_vss(n, max_len=50, seed=77)
    w = CMA(env)
    w.set_opponent(TeamScripted())
    h, prm = host_from(env), oracle_params(env)
    obs_h = O.compute_obs(h, 6)
    io = O.make_io(n, O.MODE_FULL)
    zero = torch.zeros((n, 6), device=DEV)
    resets = 0
    for t in range(120):
        out, _, dones, info = w.step(zero)
        full = np.zeros((n, 12), F32)
        full[:, 6:] = S.reference_actions(obs_h[:, 3]).reshape(n, 6)
        O.step(h, O.MODE_FULL, full, io, prm)
        obs_h = io["obs"].reshape(n, 6, 52)
        msg = f"step {t}"
        np.testing.assert_array_equal(bits(w._opp_act).reshape(n, 6), bits(full[:, 6:]), err_msg=msg + " opponent actions")
        np.testing.assert_array_equal(bits(out["obs"]), bits(obs_h[:, 0]), err_msg=msg + " obs")
        np.testing.assert_array_equal(bits(info["opponent_obs"]), bits(obs_h[:, 3:6]), err_msg=msg + " opponent obs")
        np.testing.assert_array_equal(dones.cpu().numpy(), h.reset, err_msg=msg + " dones")
        resets += int(h.reset.sum())
    assert_env_equal(env, h, "end")
    assert resets >= 2 * n  # every field timed out twice


def test_play_matches_the_scripted_team_beats_the_zero_team():
    from play import get_team, play_matches
    env = make_vss(256, seed=5)
    env.w_goal, env.w_grad, env.w_move, env.w_energy = 1.0, 0.0, 0.0, 0.0
    score, length = play_matches(env, get_team("scripted"), get_team("zero"), 200)
    print(f"scripted vs zero over 200 matches: score {score:.3f}, length {length:.1f}")
    assert score > 0 and 0 < length <= 400
