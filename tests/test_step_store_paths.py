"""The step kernels' store paths (vss_step.hip: wave_rsrc / store16 / store_bodies_wave, the store policy).

Every stream of a step goes out through a buffer resource over exactly the wave's output block, with a
cache policy per store group, and a full wave's state goes out as 16-B stores through LDS.  These are the
shapes at which that addressing can go wrong:
  * n in {1, 31, 32, 33, 65}: one lane, a wave one short of full, full, one over, a third partial wave --
    every mode, the versus and the mirror step and a K = 2 rollout, three steps from a seeded reset with a
    time-out and a reset inside them, every output and the whole state bit-equal to the CPU oracle;
  * every output and state buffer inside 256-B sentinel zones, at n = 1 and 33: the zones stay untouched
    and every byte between them that the contract writes is written;
  * n = 86,566, two fields past the size at which the past-the-Infinity-Cache table starts (256 MiB /
    3,101 B = 86,564.2: the table holds from n = 86,565);
  * visibility of write-through stores: the outputs read by a torch kernel on the launch's stream right
    behind the launch, and by a host copy after a synchronise; the state carried through 50 steps.
"""
import numpy as np
import pytest
import torch

import oracle as O
from test_mirror_step import full_actions as mirror_actions, mirror_io, team_rewards
from test_versus_step import (DEV, F32, assert_env_equal, bits, device_io, full_actions as versus_actions, host_from,
                              make_vss, oracle_params)
from vss_amd import _native as N

gpu = pytest.mark.gpu
SIZES = [1, 31, 32, 33, 65]
WRAPPED = [O.MODE_SA, O.MODE_CMA, O.MODE_DMA]
MODES = [O.MODE_FULL] + WRAPPED
MAX_LEN = 12
STEPS = 3


def shape_of(mode, n):
    """(observation rows per field, output rows, action floats per row)."""
    A = {O.MODE_FULL: 6, O.MODE_DMA: 3}.get(mode, 1)
    R = 3 if mode == O.MODE_DMA else 1
    return A, n * R, {O.MODE_FULL: 12, O.MODE_CMA: 6}.get(mode, 2)


def seeded(n, seed=4321):
    """A freshly reset env with every third field two steps short of its time-out, and its host twin."""
    env = make_vss(n, max_len=MAX_LEN, seed=seed)
    env.reset_buf.zero_()  # still set from the construction reset: the first step would zero the progress
    env.progress_buf[::3] = MAX_LEN - 2
    return env, host_from(env), oracle_params(env)


def step_io(n, mode):
    if mode != O.MODE_FULL:
        return device_io(n, mode)
    return dict(ou_buf=None, obs=torch.zeros((n * 6, 52), device=DEV), terminal_obs=torch.zeros((n * 6, 52), device=DEV),
                rew=torch.zeros((n, 24), device=DEV), reward_sum=torch.zeros(n, device=DEV), dones_rep=None,
                time_outs=torch.zeros(n, dtype=torch.bool, device=DEV), progress_f=torch.zeros(n, device=DEV))


def raw(t):
    """Bit pattern of a tensor or array: floats as uint32, bools as uint8."""
    a = bits(t)
    return a.astype(np.uint8) if a.dtype == np.bool_ else a


def assert_io_equal(got, want, msg):
    for k, w in want.items():
        if w is not None:
            np.testing.assert_array_equal(raw(got[k]).reshape(-1), raw(w).reshape(-1), err_msg=f"{msg} {k}")


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_small_shapes_step_bit_exact_in_stream_order_and_on_the_host(mode, n):
    env, h, prm = seeded(n)
    _, rows, width = shape_of(mode, n)
    io, want = step_io(n, mode), O.make_io(n, mode)
    gen = np.random.default_rng(10 * n + mode)
    resets = timeouts = 0
    for t in range(STEPS):
        a = gen.uniform(-1.2, 1.2, (rows, width)).astype(F32)
        env.native_step(mode, torch.from_numpy(a).to(DEV), io)
        # a torch kernel on the launch's stream, right behind the launch: no synchronise in between
        behind = {k: v.clone() for k, v in io.items() if v is not None}
        state_behind = env.state.clone()
        O.step(h, mode, a, want, prm)
        msg = f"mode {mode} n {n} step {t}"
        assert_env_equal(env, h, msg)  # synchronises, then host copies
        assert_io_equal(io, want, msg + " host copy")
        assert_io_equal(behind, want, msg + " stream order")
        np.testing.assert_array_equal(bits(state_behind), bits(h.state), err_msg=msg + " state, stream order")
        resets += int(h.reset.sum())
        timeouts += int(want["time_outs"].sum())
    assert resets > 0 and timeouts > 0


@gpu
@pytest.mark.parametrize("mode", WRAPPED)
@pytest.mark.parametrize("n", SIZES)
def test_small_shapes_versus_step_bit_exact(mode, n):
    env, h, prm = seeded(n)
    A, rows, width = shape_of(mode, n)
    io = device_io(n, mode)
    opp_obs = torch.zeros((n, 3, 52), device=DEV)
    gen = np.random.default_rng(100 + 10 * n + mode)
    exp_ou = np.zeros((n, 12), F32)
    resets = 0
    for t in range(STEPS):
        a = gen.uniform(-1.2, 1.2, (rows, width)).astype(F32)
        o = gen.uniform(-1.2, 1.2, (n, 3, 2)).astype(F32)
        env.native_step_versus(mode, torch.from_numpy(a).to(DEV), io, torch.from_numpy(o).to(DEV), opp_obs)
        full = versus_actions(mode, n, a, o, exp_ou, h.ctr.copy(), prm)
        iof = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, full, iof, prm)
        msg = f"versus mode {mode} n {n} step {t}"
        assert_env_equal(env, h, msg)
        fobs, fterm = iof["obs"].reshape(n, 6, 52), iof["terminal_obs"].reshape(n, 6, 52)
        rew, rsum = team_rewards(mode, iof["rew"].reshape(n, 6, 4), 0, rows)
        exp_ou = np.where(h.reset[:, None] != 0, full * F32(0.0), full).astype(F32)
        assert_io_equal(dict(io, opp_obs=opp_obs),
                        dict(obs=np.ascontiguousarray(fobs[:, :A]), terminal_obs=np.ascontiguousarray(fterm[:, :A]),
                             opp_obs=np.ascontiguousarray(fobs[:, 3:6]), rew=rew, reward_sum=rsum, ou_buf=exp_ou,
                             time_outs=np.repeat(iof["time_outs"], A), progress_f=np.repeat(iof["progress_f"], A),
                             dones_rep=np.repeat(h.reset, 3) if mode == O.MODE_DMA else None), msg)
        resets += int(h.reset.sum())
    assert resets > 0


@gpu
@pytest.mark.parametrize("mode", WRAPPED)
@pytest.mark.parametrize("n", SIZES)
def test_small_shapes_mirror_step_bit_exact(mode, n):
    env, h, prm = seeded(n)
    A, rows, width = shape_of(mode, n)
    io, yl = mirror_io(n, mode)
    gen = np.random.default_rng(200 + 10 * n + mode)
    exp_ou = np.zeros((n, 12), F32)
    resets = 0
    for t in range(STEPS):
        a = gen.uniform(-1.2, 1.2, (2, rows, width)).astype(F32)
        env.native_step_mirror(mode, torch.from_numpy(a).to(DEV), io, yl)
        full = mirror_actions(mode, n, a[0], a[1], exp_ou, h.ctr.copy(), prm)
        iof = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, full, iof, prm)
        msg = f"mirror mode {mode} n {n} step {t}"
        assert_env_equal(env, h, msg)
        fobs, fterm = iof["obs"].reshape(n, 6, 52), iof["terminal_obs"].reshape(n, 6, 52)
        for team, out, a0, dones_key in (("blue", io, 0, "dones_rep"), ("yellow", yl, 3, "dones")):
            rew, rsum = team_rewards(mode, iof["rew"].reshape(n, 6, 4), a0, rows)
            assert_io_equal(out, {"obs": np.ascontiguousarray(fobs[:, a0:a0 + A]),
                                  "terminal_obs": np.ascontiguousarray(fterm[:, a0:a0 + A]), "rew": rew,
                                  "reward_sum": rsum, dones_key: np.repeat(h.reset, A),
                                  "time_outs": np.repeat(iof["time_outs"], A),
                                  "progress_f": np.repeat(iof["progress_f"], A)}, f"{msg} {team}")
        exp_ou = np.where(h.reset[:, None] != 0, full * F32(0.0), full).astype(F32)
        assert_io_equal(io, dict(ou_buf=exp_ou), msg)
        resets += int(h.reset.sum())
    assert resets > 0


ROLLOUT_KEYS = dict(obs="obs", terminal_observation="terminal_obs", rew="rew", time_outs="time_outs",
                    progress_buffer="progress_f")


def rollout_against_oracle(env, h, prm, out, acts, msg):
    """`out` of env.rollout(acts) and the env's state against K oracle FULL steps."""
    K, n = acts.shape[0], env.num_fields
    for k in range(K):
        io = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, acts[k].reshape(n, 12), io, prm)
        assert_io_equal({g: out[g][k] for g in ROLLOUT_KEYS}, {g: io[o] for g, o in ROLLOUT_KEYS.items()}, f"{msg} step {k}")
        np.testing.assert_array_equal(out["dones"][k].cpu().numpy(), h.reset, err_msg=f"{msg} step {k} dones")
    assert_env_equal(env, h, msg)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_small_shapes_rollout_of_two_steps_bit_exact(n):
    env, h, prm = seeded(n)
    env.progress_buf[::3] = MAX_LEN - 1  # the time-out inside the two steps
    h.progress[:] = env.progress_buf.cpu().numpy()
    acts = np.random.default_rng(300 + n).uniform(-1.2, 1.2, (2, n, 2, 3, 2)).astype(F32)
    out = env.rollout(torch.from_numpy(acts).to(DEV))
    rollout_against_oracle(env, h, prm, out, acts, f"rollout n {n}")
    assert int(out["time_outs"].sum()) > 0


# ---- write extents ---------------------------------------------------------------------------------------
ZONE = 256  # sentinel bytes on each side
FILL = 0xA5


class Carved:
    """A tensor of `shape` and `dtype` carved out of a larger allocation, ZONE sentinel bytes on both sides.
    The allocation starts 512-B aligned, so the window keeps the 16-B alignment the ABI asks for."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        pad = -self.nbytes % 4
        self.backing = torch.full((2 * ZONE + self.nbytes + pad,), FILL, dtype=torch.uint8, device=DEV)
        self.t = self.backing[ZONE:ZONE + self.nbytes].view(dtype).view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def zones_intact(self):
        b = self.backing
        return bool((b[:ZONE] == FILL).all()) and bool((b[ZONE + self.nbytes:] == FILL).all())

    def unwritten(self):
        """Per element of the window: does it still hold the sentinel (4-byte words; bytes for 1-byte types)?"""
        w = self.backing[ZONE:ZONE + self.nbytes]
        if self.t.element_size() == 1:
            return w == FILL
        return w.view(torch.int32) == int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])


def carve_state(env):
    """Move the env's state buffers into carved windows (the values kept); the windows by name."""
    c = {}
    for k in ("state", "progress_buf", "reset_buf", "dof_velocity_buf", "rng_counter"):
        old = getattr(env, k)
        c[k] = Carved(tuple(old.shape), old.dtype, fill=old)
        setattr(env, k, c[k].t)
    c["state"].backing[ZONE:ZONE + c["state"].nbytes].view(N.STATE_CHANNELS, -1)[DEAD] = FILL
    return c


def carve_io(io):
    c = {k: Carved(tuple(v.shape), v.dtype, fill=v if k == "ou_buf" else None) for k, v in io.items() if v is not None}
    return c, {k: (c[k].t if v is not None else None) for k, v in io.items()}


def assert_extents(windows, msg, partly=()):
    for k, w in windows.items():
        assert w.zones_intact(), f"{msg}: {k} written outside its extent"
        if k not in partly:
            assert not bool(w.unwritten().any()), f"{msg}: {k} not written in full"


DEAD = slice(N.CH_RQX, N.CH_RQX + 12)  # the quaternions' x, y channels: planar robots, no step reads or writes them


def assert_state_extents(env, twin, cs, n, msg):
    """The state buffers are read and written, so a sentinel cannot mark their unwritten bytes: every byte
    must equal the run in ordinary allocations instead.  The zones stay intact, and the dead channels, which
    carve_state filled with the sentinel, still hold it."""
    for k, w in cs.items():
        assert w.zones_intact(), f"{msg}: {k} written outside its extent"
    left = cs["state"].unwritten().view(N.STATE_CHANNELS, n)
    assert bool(left[DEAD].all()), f"{msg}: a dead quaternion channel was written"
    live = torch.ones(N.STATE_CHANNELS, dtype=torch.bool, device=DEV)
    live[DEAD] = False
    assert not bool(left[live].any()), f"{msg}: a live state channel holds the sentinel"
    assert torch.equal(env.state[live], twin.state[live]), f"{msg}: state differs from the uncarved run"
    for k in ("progress_buf", "reset_buf", "dof_velocity_buf", "rng_counter"):
        assert torch.equal(getattr(env, k), getattr(twin, k)), f"{msg}: {k} differs from the uncarved run"


@gpu
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("mode,kind", [(m, "step") for m in MODES] + [(m, k) for k in ("versus", "mirror") for m in WRAPPED])
def test_write_extents_with_256_byte_zones(mode, kind, n):
    env, twin = (seeded(n)[0] for _ in range(2))  # the twin steps in ordinary allocations
    cs = carve_state(env)
    A, rows, width = shape_of(mode, n)
    gen = torch.Generator(device=DEV).manual_seed(7 * n + mode)
    teams = 2 if kind == "mirror" else 1
    acts = Carved((teams, rows, width), fill=torch.rand((teams, rows, width), device=DEV, generator=gen) * 2.4 - 1.2)
    opp = Carved((n, 3, 2), fill=torch.rand((n, 3, 2), device=DEV, generator=gen) * 2.4 - 1.2)
    acts_before, opp_before = acts.backing.clone(), opp.backing.clone()
    if kind == "mirror":
        io, yl = mirror_io(n, mode)
        io_t, yl_t = mirror_io(n, mode)
        cy, yl = carve_io(yl)
    else:
        io, io_t = step_io(n, mode), step_io(n, mode)
    ci, io = carve_io(io)
    if kind == "versus":
        opp_obs, opp_obs_t = Carved((n, 3, 52)), torch.zeros((n, 3, 52), device=DEV)
    for t in range(STEPS):
        if kind == "step":
            for e, o in ((env, io), (twin, io_t)):
                e.native_step(mode, acts.t[0], o)
        elif kind == "versus":
            env.native_step_versus(mode, acts.t[0], io, opp.t, opp_obs.t)
            twin.native_step_versus(mode, acts.t[0], io_t, opp.t, opp_obs_t)
        else:
            env.native_step_mirror(mode, acts.t, io, yl)
            twin.native_step_mirror(mode, acts.t, io_t, yl_t)
    torch.cuda.synchronize()
    msg = f"{kind} mode {mode} n {n}"
    assert torch.equal(acts.backing, acts_before) and torch.equal(opp.backing, opp_before), msg + ": an input was written"
    assert_extents(ci, msg)
    assert_state_extents(env, twin, cs, n, msg)
    if kind == "mirror":
        assert_extents(cy, msg + " yl")
        assert_io_equal(yl, yl_t, msg + " yl")
    if kind == "versus":
        assert_extents(dict(opp_obs=opp_obs), msg)
        assert torch.equal(opp_obs.t, opp_obs_t)
    assert_io_equal(io, io_t, msg)
    assert int(twin.progress_buf[0]) == 1  # field 0 timed out in the second step and started over in the third


@gpu
@pytest.mark.parametrize("n", [1, 33])
def test_rollout_write_extents_with_256_byte_zones(n):
    env, twin = (seeded(n)[0] for _ in range(2))
    cs = carve_state(env)
    K = 2
    acts = torch.rand((K, n, 2, 3, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)) * 2.4 - 1.2
    want = twin.rollout(acts)
    co, out = carve_io({k: torch.zeros_like(v) for k, v in want.items()})
    env.rollout(acts, out)
    torch.cuda.synchronize()
    assert_extents(co, f"rollout n {n}")
    assert_state_extents(env, twin, cs, n, f"rollout n {n}")
    assert_io_equal(out, want, f"rollout n {n}")


# ---- past the cache, and the state carried through write-through stores -----------------------------------
@gpu
def test_first_size_past_the_infinity_cache_bit_exact():
    n = 86_566
    assert (256 << 20) // 3101 < n - 1 < (256 << 20) // 3101 + 3  # launch_step's threshold: just past it
    env = make_vss(n, max_len=2, seed=5)
    h, prm = host_from(env), oracle_params(env)
    gen = np.random.default_rng(86)
    io = step_io(n, O.MODE_FULL)
    for t in range(2):  # max_len 2: every field times out and resets in the second step
        a = gen.uniform(-1.0, 1.0, (n, 12)).astype(F32)
        env.native_step(O.MODE_FULL, torch.from_numpy(a).to(DEV), io)
        want = O.make_io(n, O.MODE_FULL)
        O.step(h, O.MODE_FULL, a, want, prm)
        assert_env_equal(env, h, f"step {t}")
        assert_io_equal(io, want, f"step {t}")
    assert int(h.reset.sum()) == n


@gpu
@pytest.mark.parametrize("mode", [O.MODE_FULL, O.MODE_SA])
def test_state_carried_through_50_consecutive_steps(mode):
    n = 33
    env = make_vss(n, max_len=20, seed=50)
    h, prm = host_from(env), oracle_params(env)
    _, rows, width = shape_of(mode, n)
    io, want = step_io(n, mode), O.make_io(n, mode)
    gen = np.random.default_rng(50 + mode)
    acts = gen.uniform(-1.2, 1.2, (50, rows, width)).astype(F32)
    dev_acts = torch.from_numpy(acts).to(DEV)
    for t in range(50):  # 50 launches back to back: the host looks only at the end
        env.native_step(mode, dev_acts[t], io)
    for t in range(50):
        O.step(h, mode, acts[t], want, prm)
    assert_env_equal(env, h, f"mode {mode} after 50 steps")
    assert_io_equal(io, want, f"mode {mode} after 50 steps")
    assert int(h.progress.max()) <= 20 and int(h.progress.min()) < 10  # episodes ended and started on the way
