"""The step kernels' prologue (vss_step.hip: load_obs_table / stage_obs_table, load_rows, load_state).

Every kernel issues all of its inputs -- the gather table's words, the wave's action / OU / learner /
opponent rows, the bookkeeping and the state channels -- before its first wait, and writes the table to LDS
next to the rows.  The loads are not predicated: lanes past a wave's last field load that field again.  What
that can break, and the suites of the store paths and the edge table do not single out, everything bit-equal
to the CPU oracle at n <= 65:
  * the table in place before its first reader on every entry: vss_compute_observations for A = 6, 3, 1 at
    n = 1, 33, 65; a K = 3 rollout at n = 33 (staged once; the next step's actions are prefetched behind
    stores); the replay step at n = 33 in all four modes;
  * partial waves, n = 33 and 65 (the last wave holds one field), with distinct values in every record slot
    and every field done in the first step: the reset runs between the two streams, both read the table;
  * a second launch on the same stream right behind the first, with another action buffer, the first's
    outputs cloned in between: a row prefetch that read a stale address would show.
"""
import numpy as np
import pytest
import torch

import oracle as O
import replay_draws as RD
from test_gpu_replay import DevEnv
from test_step_store_paths import MODES, assert_io_equal, rollout_against_oracle, seeded, shape_of, step_io
from test_versus_step import DEV, F32, assert_env_equal, bits, host_from, make_vss, oracle_params

pytestmark = pytest.mark.gpu


def distinct(env, seed):
    """Give every state channel of every field a value of its own: the velocities that a construction
    reset leaves at zero become small distinct numbers, and so does dof_velocity_buf (the action slots of
    an observation record).  Positions and headings stay the reset's (distinct already, and a legal placement)."""
    g = np.random.default_rng(seed)
    n = env.num_fields
    s = env.state.cpu().numpy()
    for ch, k, scale in ((O.CH_RVX, 6, 0.4), (O.CH_RVY, 6, 0.4), (O.CH_RW, 6, 3.0), (O.CH_BALL + 2, 2, 0.5)):  # ball vx, vy
        s[ch:ch + k] = g.uniform(-scale, scale, (k, n)).astype(F32)
    env.state.copy_(torch.from_numpy(s))
    env.dof_velocity_buf.copy_(torch.from_numpy(g.uniform(-1, 1, (n, 12)).astype(F32)).view_as(env.dof_velocity_buf))
    live = np.r_[0:O.CH_RQX, O.CH_RQZ:O.STATE_CHANNELS]
    for f in range(n):
        assert len(np.unique(s[live, f].view(np.uint32))) == live.size, f"field {f}: a state value occurs twice"


# ---- the table in place before its first reader ---------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 65])
@pytest.mark.parametrize("agents", [6, 3, 1])
def test_observe_reads_a_complete_table(agents, n):
    env = make_vss(n, seed=77)
    distinct(env, 7 * n + agents)
    h = host_from(env)
    out = torch.full((n, agents, 52), float("nan"), device=DEV)
    env.compute_observations(out, n_agents=agents)
    np.testing.assert_array_equal(bits(out), O.compute_obs(h, agents).view(np.uint32))


def test_rollout_of_three_steps_stages_the_table_once():
    n, K = 33, 3
    env, h, prm = seeded(n, seed=99)
    distinct(env, 3)
    h = host_from(env)
    acts = np.random.default_rng(31).uniform(-1.2, 1.2, (K, n, 2, 3, 2)).astype(F32)
    out = env.rollout(torch.from_numpy(acts).to(DEV))
    rollout_against_oracle(env, h, prm, out, acts, "rollout K 3")
    assert int(out["dones"].sum()) > 0  # a reset between two steps' streams


def reference_ordered(g, n):
    """One reset_dones call's uniforms for all n fields in the reference's call order (tests/replay_draws.py):
    rejection rounds over the fields still too close, then the yaws, then the ball velocities."""
    flat, close = [], np.arange(n)
    while close.size:
        block = g.random((close.size, 14), dtype=F32)
        flat.append(block.reshape(-1))
        close = close[RD.too_close(block)]
    flat += [g.random(6 * n, dtype=F32), g.random(2 * n, dtype=F32)]
    return np.concatenate(flat)


@pytest.mark.parametrize("mode", MODES)
def test_replay_step_with_every_field_done(mode):
    """vss_step_replay at n = 33, max_len = 1: every field times out and is re-placed from injected draws, so
    the table serves the terminal stream, the reset runs, and the table serves the second stream."""
    n = 33
    src = make_vss(n, seed=5)
    distinct(src, 50 + mode)
    g = np.random.default_rng(500 + mode)
    flat = reference_ordered(g, n)
    rows, rounds = RD.to_rows(flat, np.arange(n), n)
    assert rounds.max() > 1, "no field needed a second rejection round"
    wrapped = mode != O.MODE_FULL
    normals = g.normal(0, 0.15, (n, 12)).astype(F32) if wrapped else None
    ou = g.uniform(-1, 1, (n, 12)).astype(F32)
    _, rrows, width = shape_of(mode, n)
    actions = g.uniform(-1.2, 1.2, (rrows, width)).astype(F32)

    dev = DevEnv(n, mode)
    dev.state.copy_(src.state)
    dev.reset.zero_()
    dev.dof.copy_(src.dof_velocity_buf.reshape(n, 12))
    h = O.HostEnv(n)
    h.state[:], h.reset[:], h.dof[:] = src.state.cpu().numpy(), 0, dev.dof.cpu().numpy()
    want = O.make_io(n, mode)
    if wrapped:
        dev.io["ou_buf"].copy_(torch.from_numpy(ou))
        want["ou_buf"][:] = ou
    dev.step(actions, rows, normals, 1)
    d, keep = O.make_draws(flat, normals.reshape(-1) if wrapped else np.zeros(0, F32))
    O.step(h, mode, actions, want, O.params(10.0, 2.0, 3.0, 0.0, 1.0, 1, 1), d)  # DevEnv.step's parameters
    assert int(h.reset.sum()) == n
    msg = f"replay mode {mode}"
    np.testing.assert_array_equal(bits(dev.state), h.state.view(np.uint32), err_msg=msg + " state")
    np.testing.assert_array_equal(dev.reset.cpu().numpy(), h.reset, err_msg=msg)
    np.testing.assert_array_equal(dev.progress.cpu().numpy(), h.progress, err_msg=msg)
    np.testing.assert_array_equal(bits(dev.dof), h.dof.view(np.uint32), err_msg=msg + " dof")
    np.testing.assert_array_equal(dev.ctr.cpu().numpy().view(np.uint32), h.ctr, err_msg=msg + " ctr")
    keys = ["obs", "terminal_obs", "rew", "progress_f", "time_outs"] + (["reward_sum", "ou_buf"] if wrapped else [])
    if mode == O.MODE_DMA:
        keys.append("dones_rep")
    assert_io_equal(dev.io, {k: want[k] for k in keys}, msg)


# ---- partial waves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [33, 65])
def test_partial_wave_with_every_field_done_in_the_first_step(mode, n):
    env = make_vss(n, max_len=1, seed=11)
    env.reset_buf.zero_()
    distinct(env, 100 * n + mode)
    h, prm = host_from(env), oracle_params(env)
    _, rows, width = shape_of(mode, n)
    io, want = step_io(n, mode), O.make_io(n, mode)
    gen = np.random.default_rng(20 * n + mode)
    if mode != O.MODE_FULL:
        ou = gen.uniform(-1, 1, (n, 12)).astype(F32)
        io["ou_buf"].copy_(torch.from_numpy(ou))
        want["ou_buf"][:] = ou
    for t in range(2):
        a = gen.uniform(-1.2, 1.2, (rows, width)).astype(F32)
        env.native_step(mode, torch.from_numpy(a).to(DEV), io)
        O.step(h, mode, a, want, prm)
        msg = f"mode {mode} n {n} step {t}"
        assert int(h.reset.sum()) == n, msg + ": a field is not done"
        assert_env_equal(env, h, msg)
        assert_io_equal(io, want, msg)


# ---- a second launch right behind the first -------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_second_launch_on_the_stream_reads_its_own_rows(mode):
    n = 33
    env, h, prm = seeded(n, seed=2468)
    distinct(env, 9 + mode)
    h = host_from(env)
    _, rows, width = shape_of(mode, n)
    io, want = step_io(n, mode), O.make_io(n, mode)
    gen = np.random.default_rng(60 + mode)
    a = [gen.uniform(-1.2, 1.2, (rows, width)).astype(F32) for _ in range(2)]
    bufs = [torch.from_numpy(x).to(DEV) for x in a]  # two allocations: the second launch has other addresses
    torch.cuda.synchronize()
    env.native_step(mode, bufs[0], io)
    first = {k: v.clone() for k, v in io.items() if v is not None}  # a copy kernel between the two launches
    env.native_step(mode, bufs[1], io)
    O.step(h, mode, a[0], want, prm)
    assert_io_equal(first, want, f"mode {mode} first launch")
    O.step(h, mode, a[1], want, prm)
    assert_env_equal(env, h, f"mode {mode} second launch")
    assert_io_equal(io, want, f"mode {mode} second launch")
