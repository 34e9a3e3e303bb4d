"""vss_step_versus: the SA / CMA / DMA step with the yellow team driven by a caller's action buffer.

Free-running and bit-exact against the unchanged CPU oracle: a versus step equals the oracle's FULL
step on [learner | OU (SA: blue robots 1-2) | opponent] actions, sliced to the mode's view.  The OU
values of SA's blue robots 1-2 come from the oracle's own SA step on a scratch field that cannot
finish in one step (the draw depends on the field index and its rng counter only, not on the state).
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O
from vss_amd import _native as N

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


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
    return O.params(env.w_goal, env.w_grad, env.w_move, env.w_energy, env.clip_actions,
                    env.max_episode_length, env.seed)


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
    return a.view(np.uint32) if a.dtype == np.float32 else a


def device_io(n, mode):
    """The mode's vss_step_io tensors plus the versus pair, on the device."""
    rows = 3 * n if mode == O.MODE_DMA else n
    return dict(ou_buf=torch.zeros((n, 12), device=DEV), obs=torch.zeros((rows, 52), device=DEV),
                terminal_obs=torch.zeros((rows, 52), device=DEV), rew=torch.zeros((rows, 4), device=DEV),
                reward_sum=torch.zeros(rows, device=DEV),
                dones_rep=torch.zeros(rows, dtype=torch.long, device=DEV) if mode == O.MODE_DMA else None,
                time_outs=torch.zeros(rows, dtype=torch.bool, device=DEV), progress_f=torch.zeros(rows, device=DEV))


def scratch_env(n, ctr):
    """A field that cannot finish in one step: ball at rest at the origin, robots at x = -+0.3."""
    s = O.HostEnv(n)
    s.reset[:] = 0
    s.ctr[:] = ctr
    for r in range(6):
        s.state[O.CH_RX + r] = -0.3 if r < 3 else 0.3
        s.state[O.CH_RY + r] = (-0.3, 0.0, 0.3)[r % 3]
    return s


def full_actions(mode, n, learner, opp, ou_so_far, ctr, prm):
    """The twelve applied, pre-clamp actions per field of a versus step."""
    full = np.zeros((n, 12), F32)
    full[:, 6:] = opp.reshape(n, 6)
    if mode == O.MODE_SA:
        scratch = scratch_env(n, ctr)
        io_s = O.make_io(n, O.MODE_SA)
        io_s["ou_buf"][:] = ou_so_far
        O.step(scratch, O.MODE_SA, learner, io_s, prm)
        assert scratch.reset.sum() == 0
        full[:, 0:2] = learner
        full[:, 2:6] = io_s["ou_buf"][:, 2:6]
    else:
        full[:, 0:6] = learner.reshape(n, 6)
    return full


@gpu
@pytest.mark.parametrize("mode", [O.MODE_SA, O.MODE_CMA, O.MODE_DMA])
@pytest.mark.parametrize("n", [1, 33, 67])
def test_versus_step_free_running_bit_exact(mode, n):
    max_len = 9 if n == 1 else 40  # n = 1: with 40 the forced goals reset the field before any time-out
    env = make_vss(n, max_len=max_len)
    h = host_from(env)
    prm = oracle_params(env)
    gen = np.random.default_rng(1000 + 10 * n + mode)
    A = 3 if mode == O.MODE_DMA else 1
    rows, width = n * A, (6 if mode == O.MODE_CMA else 2)
    io = device_io(n, mode)
    opp_act = torch.zeros((n, 3, 2), device=DEV)
    opp_obs = torch.zeros((n, 3, 52), device=DEV)
    exp_ou = np.zeros((n, 12), F32)
    resets = goals = timeouts = 0
    for t in range(90):
        a = gen.uniform(-1.2, 1.2, (rows, width)).astype(F32)
        o = gen.uniform(-1.2, 1.2, (n, 3, 2)).astype(F32)
        if t % 17 == 5:  # push some balls into a goal
            k = max(1, n // 8)
            env.ball_pos[:k] = torch.tensor([0.74, 0.05], device=DEV)
            env.ball_vel[:k] = torch.tensor([1.0, 0.0], device=DEV)
            h.state[0, :k], h.state[1, :k], h.state[2, :k], h.state[3, :k] = 0.74, 0.05, 1.0, 0.0
        opp_act.copy_(torch.from_numpy(o))
        env.native_step_versus(mode, torch.from_numpy(a).to(DEV), io, opp_act, opp_obs)

        full = full_actions(mode, n, a, o, exp_ou, h.ctr.copy(), prm)
        iof = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, full, iof, prm)
        msg = f"mode {mode} n {n} step {t}"
        assert_env_equal(env, h, msg)
        fobs, fterm = iof["obs"].reshape(n, 6, 52), iof["terminal_obs"].reshape(n, 6, 52)
        frew = iof["rew"].reshape(n, 6, 4)
        np.testing.assert_array_equal(bits(io["obs"]).reshape(n, A, 52), bits(fobs[:, :A]), err_msg=msg + " obs")
        np.testing.assert_array_equal(bits(io["terminal_obs"]).reshape(n, A, 52), bits(fterm[:, :A]), err_msg=msg + " term")
        np.testing.assert_array_equal(bits(opp_obs), bits(np.ascontiguousarray(fobs[:, 3:6])), err_msg=msg + " opp_obs")
        if mode == O.MODE_CMA:
            rew = (((frew[:, 0] + frew[:, 1]) + frew[:, 2]) / F32(3)).astype(F32)
        else:
            rew = np.ascontiguousarray(frew[:, :A]).reshape(rows, 4)
        rsum = ((rew[:, 0] + rew[:, 1]) + rew[:, 2]) + rew[:, 3]
        np.testing.assert_array_equal(bits(io["rew"]), bits(rew), err_msg=msg + " rew")
        np.testing.assert_array_equal(bits(io["reward_sum"]), bits(rsum), err_msg=msg + " reward_sum")
        np.testing.assert_array_equal(io["time_outs"].cpu().numpy().astype(np.uint8), np.repeat(iof["time_outs"], A),
                                      err_msg=msg + " time_outs")
        np.testing.assert_array_equal(bits(io["progress_f"]), bits(np.repeat(iof["progress_f"], A)), err_msg=msg + " progress")
        if mode == O.MODE_DMA:
            np.testing.assert_array_equal(io["dones_rep"].cpu().numpy(), np.repeat(h.reset, 3), err_msg=msg + " dones_rep")
        exp_ou = np.where(h.reset[:, None] != 0, full * F32(0.0), full).astype(F32)
        np.testing.assert_array_equal(bits(io["ou_buf"]), bits(exp_ou), err_msg=msg + " ou_buf")
        resets += int(h.reset.sum())
        goals += int((np.abs(frew[:, 0, 0]) > 0).sum())
        timeouts += int(iof["time_outs"].sum())
    assert resets > 0 and goals > 0
    if n >= 33 or max_len == 9:
        assert timeouts > 0


@gpu
def test_sa_ou_continuity_with_the_plain_step():
    """From one state and ou_buf, vss_step(SA) and vss_step_versus(SA) leave the same OU values of blue
    robots 1-2 on the fields that finish in neither."""
    n = 67
    envs = [make_vss(n, max_len=40, seed=99) for _ in range(2)]
    gen = np.random.default_rng(3)
    ou0 = torch.from_numpy(gen.uniform(-0.9, 0.9, (n, 12)).astype(F32)).to(DEV)
    a = torch.from_numpy(gen.uniform(-1.2, 1.2, (n, 2)).astype(F32)).to(DEV)
    opp_act = torch.from_numpy(gen.uniform(-1.2, 1.2, (n, 3, 2)).astype(F32)).to(DEV)
    ios = [device_io(n, O.MODE_SA) for _ in range(2)]
    for io in ios:
        io["ou_buf"].copy_(ou0)
    envs[0].native_step(N.MODE_SA, a, ios[0])
    envs[1].native_step_versus(N.MODE_SA, a, ios[1], opp_act, torch.zeros((n, 3, 52), device=DEV))
    keep = ((envs[0].reset_buf == 0) & (envs[1].reset_buf == 0)).cpu().numpy()
    assert keep.sum() > 0
    plain, versus = bits(ios[0]["ou_buf"])[keep, 2:6], bits(ios[1]["ou_buf"])[keep, 2:6]
    np.testing.assert_array_equal(plain, versus)
    assert np.all(plain != bits(ou0)[keep, 2:6])  # the OU process moved them
    # and the yellow slots hold the opponent's actions, not OU values
    np.testing.assert_array_equal(bits(ios[1]["ou_buf"])[keep, 6:], bits(opp_act).reshape(n, 6)[keep])


@gpu
@pytest.mark.parametrize("mode", [O.MODE_SA, O.MODE_CMA, O.MODE_DMA])
def test_versus_step_write_extents(mode):
    """opp_obs and every vss_step_io output inside sentinel guards: the guards stay intact, every
    float output is written in full, and opp_actions is not written."""
    from test_write_extents import Guarded
    n = 33
    env = make_vss(n, max_len=2)  # every field times out and resets at steps 2 and 4
    A = 3 if mode == O.MODE_DMA else 1
    rows, width = n * A, (6 if mode == O.MODE_CMA else 2)
    gen = torch.Generator(device=DEV).manual_seed(mode)
    actions = Guarded((rows, width), fill=torch.rand((rows, width), device=DEV, generator=gen) * 2.4 - 1.2)
    opp_act = Guarded((n, 3, 2), fill=torch.rand((n, 3, 2), device=DEV, generator=gen) * 2.4 - 1.2)
    ou = Guarded((n, 12), fill=torch.zeros((n, 12), device=DEV))
    obs, term, opp_obs = Guarded((rows, 52)), Guarded((rows, 52)), Guarded((n, 3, 52))
    rew, rsum, prog = Guarded((rows, 4)), Guarded((rows,)), Guarded((rows,))
    touts = Guarded((rows,), dtype=torch.bool)
    dones = Guarded((rows,), dtype=torch.long) if mode == O.MODE_DMA else None
    cio = N.VssStepIO(actions.ptr, ou.ptr, obs.ptr, term.ptr, rew.ptr, rsum.ptr, dones.ptr if dones else None,
                      touts.ptr, prog.ptr)
    vio = N.VssVersusIO(opp_act.ptr, opp_obs.ptr)
    prm, st = env._c_params(), env._c_state()
    actions.snapshot()
    opp_act.snapshot()
    for _ in range(4):
        rc = N.load().vss_step_versus(N.stream_of(env.device), n, mode, ctypes.byref(prm), ctypes.byref(st),
                                      ctypes.byref(cio), ctypes.byref(vio))
        assert rc == 0
    torch.cuda.synchronize()
    assert int(env.reset_buf.sum()) == n
    assert actions.unchanged() and opp_act.unchanged()
    outs = [ou, obs, term, opp_obs, rew, rsum, prog, touts] + ([dones] if dones else [])
    for i, g in enumerate(outs):
        assert g.guards_intact(), f"output {i} written outside its extent"
    for i, g in enumerate([ou, obs, term, opp_obs, rew, rsum, prog]):
        assert g.covered(), f"output {i} not written in full"


def test_versus_argument_validation_without_gpu():
    """Null vs and mode FULL are rejected before any HIP call; the struct has the C layout."""
    lib = N.load()
    assert ctypes.sizeof(N.VssVersusIO) == 16
    prm = N.VssParams(10, 2, 3, 0, 1, 400, 1)
    fake = ctypes.c_void_p(16)  # never dereferenced: every call below is rejected first
    st = N.VssState(fake, fake, fake, fake, fake)
    io = N.VssStepIO(*([fake] * 9))
    vs = N.VssVersusIO(fake, fake)
    args = (None, 16, N.MODE_SA, ctypes.byref(prm), ctypes.byref(st), ctypes.byref(io))
    assert lib.vss_step_versus(*args, None) == 1
    assert lib.vss_step_versus(None, 16, N.MODE_FULL, ctypes.byref(prm), ctypes.byref(st), ctypes.byref(io),
                               ctypes.byref(vs)) == 1
    assert lib.vss_step_versus(None, 16, 7, ctypes.byref(prm), ctypes.byref(st), ctypes.byref(io), ctypes.byref(vs)) == 1
    assert lib.vss_step_versus(*args, ctypes.byref(N.VssVersusIO(None, fake))) == 1   # null opp_actions
    assert lib.vss_step_versus(*args, ctypes.byref(N.VssVersusIO(fake, None))) == 1   # null opp_obs
    assert lib.vss_step_versus(*args, ctypes.byref(N.VssVersusIO(ctypes.c_void_p(20), fake))) == 1  # 8-B alignment
    assert lib.vss_step_versus(*args, ctypes.byref(N.VssVersusIO(fake, ctypes.c_void_p(24)))) == 1  # 16-B alignment
