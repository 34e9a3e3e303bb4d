"""vss_step_mirror: the SA / CMA / DMA step with both teams' robots as learner rows.

Free-running and bit-exact against the unchanged CPU oracle: a mirror step equals the oracle's FULL
step on the twelve applied actions [blue learner | OU (SA) | yellow learner | OU (SA)], sliced to
agent 0 / 0..2 for the blue rows and agent 3 / 3..5 for the yellow rows.  SA's OU values (slots 2..5
and 8..11) come from the oracle's own SA step on a scratch field that cannot finish in one step, as in
tests/test_versus_step.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O
from test_versus_step import (DEV, F32, assert_env_equal, bits, device_io, host_from, make_vss, oracle_params,
                              scratch_env)
from vss_amd import _native as N

gpu = pytest.mark.gpu
MODES = [O.MODE_SA, O.MODE_CMA, O.MODE_DMA]


def shape_of(mode, n):
    """(learner rows per field and team, rows per team, action floats per row)."""
    A = 3 if mode == O.MODE_DMA else 1
    return A, n * A, (6 if mode == O.MODE_CMA else 2)


def mirror_io(n, mode):
    """The blue team's vss_step_io tensors (dones_rep in every mode) and the yellow team's, on the device."""
    _, rows, _ = shape_of(mode, n)
    io = device_io(n, mode)
    io["dones_rep"] = torch.zeros(rows, dtype=torch.long, device=DEV)
    yl = dict(obs=torch.zeros((rows, 52), device=DEV), terminal_obs=torch.zeros((rows, 52), device=DEV),
              rew=torch.zeros((rows, 4), device=DEV), reward_sum=torch.zeros(rows, device=DEV),
              dones=torch.zeros(rows, dtype=torch.long, device=DEV),
              time_outs=torch.zeros(rows, dtype=torch.bool, device=DEV), progress_f=torch.zeros(rows, device=DEV))
    return io, yl


def full_actions(mode, n, blue, yellow, ou_so_far, ctr, prm):
    """The twelve applied, pre-clamp actions per field of a mirror step."""
    full = np.zeros((n, 12), F32)
    if mode == O.MODE_SA:
        scratch = scratch_env(n, ctr)
        io_s = O.make_io(n, O.MODE_SA)
        io_s["ou_buf"][:] = ou_so_far
        O.step(scratch, O.MODE_SA, blue, io_s, prm)
        assert scratch.reset.sum() == 0
        full[:] = io_s["ou_buf"]  # slots 2..5 and 8..11: the OU process, as vss_step(SA) runs it
        full[:, 0:2] = blue
        full[:, 6:8] = yellow
    else:
        full[:, 0:6] = blue.reshape(n, 6)
        full[:, 6:12] = yellow.reshape(n, 6)
    return full


def team_rewards(mode, frew, a0, rows):
    """The mode's (rows, 4) reward block and its sums for the team whose first agent is a0."""
    if mode == O.MODE_CMA:
        rew = (((frew[:, a0] + frew[:, a0 + 1]) + frew[:, a0 + 2]) / F32(3)).astype(F32)
    else:
        A = 3 if mode == O.MODE_DMA else 1
        rew = np.ascontiguousarray(frew[:, a0:a0 + A]).reshape(rows, 4)
    return rew, ((rew[:, 0] + rew[:, 1]) + rew[:, 2]) + rew[:, 3]


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 33, 67])
def test_mirror_step_free_running_bit_exact(mode, n):
    max_len = 9 if n == 1 else 40  # n = 1: with 40 the forced goals reset the field before any time-out
    env = make_vss(n, max_len=max_len)
    h = host_from(env)
    prm = oracle_params(env)
    gen = np.random.default_rng(2000 + 10 * n + mode)
    A, rows, width = shape_of(mode, n)
    io, yl = mirror_io(n, mode)
    exp_ou = np.zeros((n, 12), F32)
    resets = goals = timeouts = yellow_goals = 0
    for t in range(90):
        a = gen.uniform(-1.2, 1.2, (2, rows, width)).astype(F32)
        if t % 17 == 5:  # push some balls into a goal: the first k into blue's target, then k into yellow's
            k = max(1, n // 8)
            for lo, sign in ((0, 1.0), (k, -1.0)) if n > 1 else ((0, 1.0 if (t // 17) % 2 == 0 else -1.0),):
                env.ball_pos[lo:lo + k] = torch.tensor([sign * 0.74, 0.05], device=DEV)
                env.ball_vel[lo:lo + k] = torch.tensor([sign * 1.0, 0.0], device=DEV)
                h.state[0, lo:lo + k], h.state[1, lo:lo + k] = sign * 0.74, 0.05
                h.state[2, lo:lo + k], h.state[3, lo:lo + k] = sign * 1.0, 0.0
        env.native_step_mirror(mode, torch.from_numpy(a).to(DEV), io, yl)

        full = full_actions(mode, n, a[0], a[1], exp_ou, h.ctr.copy(), prm)
        iof = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, full, iof, prm)
        msg = f"mode {mode} n {n} step {t}"
        assert_env_equal(env, h, msg)
        fobs, fterm = iof["obs"].reshape(n, 6, 52), iof["terminal_obs"].reshape(n, 6, 52)
        frew = iof["rew"].reshape(n, 6, 4)
        for team, out, a0, dones in (("blue", io, 0, io["dones_rep"]), ("yellow", yl, 3, yl["dones"])):
            m = f"{msg} {team}"
            np.testing.assert_array_equal(bits(out["obs"]).reshape(n, A, 52), bits(np.ascontiguousarray(fobs[:, a0:a0 + A])),
                                          err_msg=m + " obs")
            np.testing.assert_array_equal(bits(out["terminal_obs"]).reshape(n, A, 52),
                                          bits(np.ascontiguousarray(fterm[:, a0:a0 + A])), err_msg=m + " term")
            rew, rsum = team_rewards(mode, frew, a0, rows)
            np.testing.assert_array_equal(bits(out["rew"]), bits(rew), err_msg=m + " rew")
            np.testing.assert_array_equal(bits(out["reward_sum"]), bits(rsum), err_msg=m + " reward_sum")
            np.testing.assert_array_equal(dones.cpu().numpy(), np.repeat(h.reset, A), err_msg=m + " dones")
            np.testing.assert_array_equal(out["time_outs"].cpu().numpy().astype(np.uint8), np.repeat(iof["time_outs"], A),
                                          err_msg=m + " time_outs")
            np.testing.assert_array_equal(bits(out["progress_f"]), bits(np.repeat(iof["progress_f"], A)),
                                          err_msg=m + " progress")
        exp_ou = np.where(h.reset[:, None] != 0, full * F32(0.0), full).astype(F32)
        np.testing.assert_array_equal(bits(io["ou_buf"]), bits(exp_ou), err_msg=msg + " ou_buf")
        resets += int(h.reset.sum())
        goals += int((np.abs(frew[:, 0, 0]) > 0).sum())
        yellow_goals += int((frew[:, 3, 0] > 0).sum())
        timeouts += int(iof["time_outs"].sum())
    # conditions on the oracle's run: the comparison above saw resets, goals for both sides and time-outs
    assert resets > 0 and goals > 0 and yellow_goals > 0
    if n >= 33 or max_len == 9:
        assert timeouts > 0


@gpu
def test_sa_ou_continuity_with_the_plain_step():
    """From one state and ou_buf, vss_step(SA) and vss_step_mirror(SA) leave the same OU values of robots
    1-2 of both teams on the fields that finish in neither; slots 0..1 and 6..7 hold the learners' actions."""
    n = 67
    envs = [make_vss(n, max_len=40, seed=99) for _ in range(2)]
    gen = np.random.default_rng(3)
    ou0 = torch.from_numpy(gen.uniform(-0.9, 0.9, (n, 12)).astype(F32)).to(DEV)
    a = torch.from_numpy(gen.uniform(-1.2, 1.2, (2, n, 2)).astype(F32)).to(DEV)
    io_p = device_io(n, O.MODE_SA)
    io_m, yl = mirror_io(n, O.MODE_SA)
    io_p["ou_buf"].copy_(ou0)
    io_m["ou_buf"].copy_(ou0)
    envs[0].native_step(N.MODE_SA, a[0], io_p)
    envs[1].native_step_mirror(N.MODE_SA, a, io_m, yl)
    keep = ((envs[0].reset_buf == 0) & (envs[1].reset_buf == 0)).cpu().numpy()
    assert keep.sum() > 0
    ou_slots = [2, 3, 4, 5, 8, 9, 10, 11]
    plain, mirror = bits(io_p["ou_buf"])[keep][:, ou_slots], bits(io_m["ou_buf"])[keep][:, ou_slots]
    np.testing.assert_array_equal(plain, mirror)
    assert np.all(plain != bits(ou0)[keep][:, ou_slots])  # the OU process moved them
    np.testing.assert_array_equal(bits(io_m["ou_buf"])[keep, 0:2], bits(a[0])[keep])
    np.testing.assert_array_equal(bits(io_m["ou_buf"])[keep, 6:8], bits(a[1])[keep])


@gpu
@pytest.mark.parametrize("mode", [O.MODE_CMA, O.MODE_DMA])
def test_mirror_blue_half_equals_the_versus_step(mode):
    """GPU against GPU: the blue half of a mirror step is the versus step with opp_actions set to the yellow
    learner's actions, and a DMA step's yellow observations are the versus step's opp_obs."""
    n = 67
    envs = [make_vss(n, max_len=3, seed=7) for _ in range(2)]
    A, rows, width = shape_of(mode, n)
    gen = np.random.default_rng(40 + mode)
    io_v = device_io(n, mode)
    io_m, yl = mirror_io(n, mode)
    opp_obs = torch.zeros((n, 3, 52), device=DEV)
    resets = 0
    for t in range(5):  # max_len 3: every field times out and resets on the way
        a = torch.from_numpy(gen.uniform(-1.2, 1.2, (2, rows, width)).astype(F32)).to(DEV)
        envs[0].native_step_versus(mode, a[0], io_v, a[1].reshape(n, 3, 2).contiguous(), opp_obs)
        envs[1].native_step_mirror(mode, a, io_m, yl)
        torch.cuda.synchronize()
        for k in ("ou_buf", "obs", "terminal_obs", "rew", "reward_sum", "progress_f"):
            np.testing.assert_array_equal(bits(io_m[k]), bits(io_v[k]), err_msg=f"step {t} {k}")
        np.testing.assert_array_equal(io_m["time_outs"].cpu().numpy(), io_v["time_outs"].cpu().numpy())
        np.testing.assert_array_equal(bits(envs[1].state), bits(envs[0].state))
        np.testing.assert_array_equal(envs[1].reset_buf.cpu().numpy(), envs[0].reset_buf.cpu().numpy())
        if mode == O.MODE_DMA:
            np.testing.assert_array_equal(io_m["dones_rep"].cpu().numpy(), io_v["dones_rep"].cpu().numpy())
            np.testing.assert_array_equal(bits(yl["obs"]).reshape(n, 3, 52), bits(opp_obs), err_msg=f"step {t} opp_obs")
        resets += int(envs[1].reset_buf.sum())
    assert resets >= n


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_mirror_step_write_extents(mode):
    """Every io and yl output inside sentinel guards: the guards stay intact, every float output is written in
    full, and neither action buffer is written."""
    from test_write_extents import Guarded
    n = 33
    env = make_vss(n, max_len=2)  # every field times out and resets at steps 2 and 4
    A, rows, width = shape_of(mode, n)
    gen = torch.Generator(device=DEV).manual_seed(mode)
    act_b = Guarded((rows, width), fill=torch.rand((rows, width), device=DEV, generator=gen) * 2.4 - 1.2)
    act_y = Guarded((rows, width), fill=torch.rand((rows, width), device=DEV, generator=gen) * 2.4 - 1.2)
    ou = Guarded((n, 12), fill=torch.zeros((n, 12), device=DEV))
    team = lambda: dict(obs=Guarded((rows, 52)), term=Guarded((rows, 52)), rew=Guarded((rows, 4)), rsum=Guarded((rows,)),
                        prog=Guarded((rows,)), touts=Guarded((rows,), dtype=torch.bool),
                        dones=Guarded((rows,), dtype=torch.long))
    b, y = team(), team()
    cio = N.VssStepIO(act_b.ptr, ou.ptr, b["obs"].ptr, b["term"].ptr, b["rew"].ptr, b["rsum"].ptr, b["dones"].ptr,
                      b["touts"].ptr, b["prog"].ptr)
    yio = N.VssMirrorIO(act_y.ptr, y["obs"].ptr, y["term"].ptr, y["rew"].ptr, y["rsum"].ptr, y["dones"].ptr,
                        y["touts"].ptr, y["prog"].ptr)
    prm, st = env._c_params(), env._c_state()
    act_b.snapshot()
    act_y.snapshot()
    for _ in range(4):
        rc = N.load().vss_step_mirror(N.stream_of(env.device), n, mode, ctypes.byref(prm), ctypes.byref(st),
                                      ctypes.byref(cio), ctypes.byref(yio))
        assert rc == 0
    torch.cuda.synchronize()
    assert int(env.reset_buf.sum()) == n
    assert act_b.unchanged() and act_y.unchanged()
    assert ou.guards_intact() and ou.covered()
    for name, side in (("io", b), ("yl", y)):
        for k, g in side.items():
            assert g.guards_intact(), f"{name} {k} written outside its extent"
        for k in ("obs", "term", "rew", "rsum", "prog"):
            assert side[k].covered(), f"{name} {k} not written in full"
        assert int(side["dones"].t.sum()) == rows and int(side["touts"].t.sum()) == rows


def test_mirror_argument_validation_without_gpu():
    """Null and misaligned members, mode FULL and a missing io->dones_rep are rejected before any HIP call;
    the struct has the C layout."""
    lib = N.load()
    assert ctypes.sizeof(N.VssMirrorIO) == 64
    prm = N.VssParams(10, 2, 3, 0, 1, 400, 1)
    fake = ctypes.c_void_p(16)  # never dereferenced: every call below is rejected first (or launches nothing)
    st = N.VssState(fake, fake, fake, fake, fake)
    io = N.VssStepIO(*([fake] * 9))
    names = [k for k, _ in N.VssMirrorIO._fields_]
    assert names == ["actions", "obs", "terminal_obs", "rew", "reward_sum", "dones", "time_outs", "progress_f"]
    good = [fake] * 8

    def call(mode=N.MODE_SA, n=16, io_=io, yl=N.VssMirrorIO(*good)):
        return lib.vss_step_mirror(None, n, mode, ctypes.byref(prm), ctypes.byref(st), ctypes.byref(io_),
                                   ctypes.byref(yl) if yl is not None else None)

    assert call(yl=None) == 1
    assert call(mode=N.MODE_FULL) == 1
    assert call(mode=7) == 1
    for i in range(8):  # each null member
        assert call(yl=N.VssMirrorIO(*[None if j == i else fake for j in range(8)])) == 1, names[i]
    # each misalignment: 8 B for actions and dones, 16 B for obs, terminal_obs and rew, 4 B for the float vectors
    for name, addr in (("actions", 20), ("dones", 20), ("obs", 24), ("terminal_obs", 24), ("rew", 24),
                       ("reward_sum", 18), ("progress_f", 18)):
        yl = N.VssMirrorIO(*[ctypes.c_void_p(addr) if k == name else fake for k in names])
        assert call(yl=yl) == 1, name
    for mode in (N.MODE_SA, N.MODE_CMA, N.MODE_DMA):  # io->dones_rep is required in every mode
        no_dones = N.VssStepIO(*[None if k == "dones_rep" else fake for k, _ in N.VssStepIO._fields_])
        assert call(mode=mode, io_=no_dones) == 1
    assert call(io_=N.VssStepIO(*[ctypes.c_void_p(20) if k == "actions" else fake for k, _ in N.VssStepIO._fields_])) == 1
    assert call(n=0) == 0  # nothing to do: no launch
