"""vss_perceive on the GPU (csrc/vss_perceive.hip): the kernel equals vss_amd.perceive.reference_perceive
bit for bit -- outputs, ring and age after every one of 12 calls, for every layout a wrapper uses, delays 0, 1, 3, 15,
every noise class alone, none and all -- writes nothing outside its rows, and the Perceived wrapper's closed loop on a
DMA env (goals, time-outs, resets) is the reference fed with the inner wrapper's true rows."""
import ctypes

import numpy as np
import pytest
import torch

from test_perceive_cpu import ALL_ON, done_patterns, same_bits
from vss_amd import _native as N
from vss_amd import perceive as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SENTINEL = 0x7FA5A5A5  # tests/test_write_extents.py's quiet-NaN pattern
GUARD = 4              # sentinel rows in front of and behind every buffer
CALLS = 12

# name: (layout for n fields, done stride)
LAYOUTS = {
    "sa": (lambda n: PC.layout_sa(), 1),
    "dma": (lambda n: PC.layout_dma(), 3),
    "mirror-sa": (lambda n: PC.layout_mirror(1, n), 1),
    "mirror-dma": (lambda n: PC.layout_mirror(3, n), 3),
    "opponent": (lambda n: PC.layout_opponent(), 3),
    "full-blue": (lambda n: PC.layout_full_blue(), 1),
}
NOISES = [PC.Noise(), PC.Noise(pos=0.002), PC.Noise(vel=0.01), PC.Noise(ang=0.02), PC.Noise(angvel=0.1), ALL_ON]


class Rows:
    """A device buffer of `rows` 52-float rows between two guard bands, everything the sentinel at first."""

    def __init__(self, rows, width=52, dtype=torch.float32):
        self.rows, self.width = rows, width
        self.t = torch.empty(((rows + 2 * GUARD) * width,), dtype=dtype, device=DEV)
        self.fill()

    def fill(self):
        if self.t.dtype == torch.float32:
            self.t.view(torch.int32).fill_(SENTINEL)
        else:
            self.t.fill_(SENTINEL)

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.width * self.t.element_size()

    def body(self):
        return self.t.view(-1, self.width)[GUARD:GUARD + self.rows]

    def host(self):
        """(the body's rows, True when both guard bands still hold the sentinel) on the host."""
        a = self.t.view(-1, self.width).cpu()
        bits = a.view(torch.int32) if a.dtype == torch.float32 else a
        intact = bool((bits[:GUARD] == SENTINEL).all() and (bits[GUARD + self.rows:] == SENTINEL).all())
        return a[GUARD:GUARD + self.rows].numpy(), intact


def is_sentinel(a):
    return np.ascontiguousarray(a, F32).view(np.uint32) == SENTINEL


def run_case(n, layout, done_stride, delay, noise, seed):
    lay = PC.Layout(*layout)
    idx = lay.row_index(n)  # (teams, n, robots)
    span = lay.span(n)
    covered = np.zeros(span, bool)
    covered[idx.reshape(-1)] = True
    g = np.random.default_rng(seed)
    shape = (lay.n_teams, n, lay.robots, 52)
    dones = done_patterns(CALLS, n)
    at = torch.from_numpy(idx.reshape(-1)).to(DEV)
    obs_b, term_b, out_b, tout_b = Rows(span), Rows(span), Rows(span), Rows(span)
    ring_b = Rows((delay + 1) * lay.n_teams * n * lay.robots)
    age_b = Rows(n, 1, torch.int32)
    done_b = Rows((n - 1) * done_stride + 1, 1, torch.long)
    c_lay, c_noise = N.VssPerceiveLayout(*lay), N.VssPerceiveNoise(*noise)
    ring, age = np.zeros((delay + 1,) + shape, F32), np.zeros(n, np.int32)
    lib, stream = N.load(), N.stream_of(torch.device(DEV))
    for t in range(CALLS):
        obs, term = g.standard_normal(shape).astype(F32), g.standard_normal(shape).astype(F32)
        obs[0, 0, 0, 0] = -0.0  # a skipped class copies the sign of zero
        start = t == 0
        obs_b.body()[at] = torch.from_numpy(obs.reshape(-1, 52)).to(DEV)
        term_b.body()[at] = torch.from_numpy(term.reshape(-1, 52)).to(DEV)
        done_b.body()[::done_stride, 0] = torch.from_numpy(dones[t]).to(DEV)
        out_b.fill()
        tout_b.fill()
        rc = lib.vss_perceive(stream, n, ctypes.byref(c_lay), delay, ctypes.byref(c_noise), seed, t, obs_b.ptr,
                              None if start else term_b.ptr, done_b.ptr, done_stride, ring_b.ptr, age_b.ptr, out_b.ptr,
                              None if start else tout_b.ptr)
        assert rc == 0
        want_o, want_t = PC.reference_perceive(obs, None if start else term, dones[t], ring, age, t, delay, noise, seed,
                                               lay.first_team)
        torch.cuda.synchronize()
        tag = (n, tuple(lay), delay, tuple(noise), t)
        got_o, ok = out_b.host()
        assert ok and same_bits(got_o[idx.reshape(-1)], want_o.reshape(-1, 52)), tag
        assert is_sentinel(got_o[~covered]).all(), tag  # rows between a strided layout's rows
        got_t, ok = tout_b.host()
        assert ok, tag
        if start:
            assert is_sentinel(got_t).all(), tag
        else:
            assert same_bits(got_t[idx.reshape(-1)], want_t.reshape(-1, 52)) and is_sentinel(got_t[~covered]).all(), tag
        got_ring, ok = ring_b.host()
        # slots no call has written yet still hold the sentinel; the reference's hold zeros
        written = np.zeros(delay + 1, bool)
        written[[c % (delay + 1) for c in range(t + 1)]] = True
        got_ring = got_ring.reshape(ring.shape)
        assert ok and same_bits(got_ring[written], ring[written]) and is_sentinel(got_ring[~written]).all(), tag
        got_age, ok = age_b.host()
        assert ok and np.array_equal(got_age[:, 0], age), tag
        for b in (obs_b, term_b, done_b):  # the inputs are only read
            assert b.host()[1], tag


@pytest.mark.parametrize("delay", [0, 1, 3, 15])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_kernel_equals_the_reference_bit_for_bit(name, delay):
    make, done_stride = LAYOUTS[name]
    for n in (1, 33, 67):
        for i, noise in enumerate(NOISES):
            run_case(n, make(n), done_stride, delay, noise, seed=(1 << 33) + 1000 * n + i)


def test_more_than_one_workgroup_and_a_team_stride_with_a_gap():
    """641 fields: 11 workgroups at 64 fields per wave, 65 at 10; the yellow block 7 rows further than it must be."""
    n = 641
    run_case(n, PC.Layout(1), 1, 3, ALL_ON, 5)
    run_case(n, PC.Layout(3, 3 * n + 7, 3, 2, 0), 3, 2, ALL_ON, 6)
    run_case(n, PC.Layout(4, 0, 3, 1, 1), 2, 1, ALL_ON, 7)


def test_full_layout_yellow_rows_are_untouched():
    n = 33
    full = torch.randn((n, 2, 3, 52), device=DEV)
    ch = PC.PerceptionChannel(n, PC.layout_full_blue(), 2, ALL_ON, 9, DEV, rows=6 * n)
    ch.obs_out.view(torch.int32).fill_(SENTINEL)
    ch.term_out.view(torch.int32).fill_(SENTINEL)
    out = ch.start(full)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    out2, term2 = ch.perceive(full, full, done)
    torch.cuda.synchronize()
    for o in (out2, term2):
        assert o.shape == full.shape and out.data_ptr() == ch.obs_out.data_ptr()
        assert bool((o[:, 1].contiguous().view(torch.int32) == SENTINEL).all())
        assert not bool((o[:, 0].contiguous().view(torch.int32) == SENTINEL).any())
    assert ch.call == 2 and ch.ring.shape == (3, 1, n, 3, 52) and torch.equal(ch.ring[1, 0], full[:, 0])


def test_the_bindings_refusals():
    n = 8
    with pytest.raises(ValueError, match="delay"):
        PC.PerceptionChannel(n, PC.layout_sa(), 16, PC.Noise(), 1, DEV)
    with pytest.raises(ValueError, match="noise"):
        PC.PerceptionChannel(n, PC.layout_sa(), 1, PC.Noise(pos=-1.0), 1, DEV)
    with pytest.raises(ValueError, match="spans"):
        PC.PerceptionChannel(n, PC.layout_dma(), 1, PC.Noise(), 1, DEV, rows=8)
    with pytest.raises(N.NativeError):
        PC.PerceptionChannel(n, PC.layout_sa(), 1, PC.Noise(), 1, "cpu")
    ch = PC.PerceptionChannel(n, PC.layout_sa(), 1, PC.Noise(), 1, DEV)
    obs = torch.zeros((n, 52), device=DEV)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="obs"):
        ch.start(torch.zeros((n + 1, 52), device=DEV))
    with pytest.raises(ValueError, match="obs"):
        ch.start(obs.double())
    with pytest.raises(ValueError, match="term"):
        ch.perceive(obs, obs[:, :51], done)
    with pytest.raises(ValueError, match="done"):
        ch.perceive(obs, obs, done.int())
    with pytest.raises(ValueError, match="done"):
        ch.perceive(obs, obs, done[:-1])
    with pytest.raises(N.NativeError, match="vss_perceive"):
        ch.perceive(ch.obs_out, obs, done)  # an output as an input: the entry's own refusal
    assert ch.call == 0
    bad = N.VssPerceiveLayout(1, 0, 2, 1, 0)
    sig = N.VssPerceiveNoise(0, 0, 0, 0)
    rc = N.load().vss_perceive(N.stream_of(torch.device(DEV)), n, ctypes.byref(bad), 1, ctypes.byref(sig), 1, 0,
                               obs.data_ptr(), None, done.data_ptr(), 1, ch.ring.data_ptr(), ch.age.data_ptr(),
                               ch.obs_out.data_ptr(), None)
    assert rc == 1


def test_state_dict_round_trip_continues_bit_equal():
    n, g = 33, torch.Generator(device="cpu").manual_seed(3)
    frames = torch.randn((8, n, 3, 52), generator=g).to(DEV)
    dones = (torch.rand((8, n), generator=g) < 0.3).long().repeat_interleave(3, 1).contiguous().to(DEV)

    def channel():
        return PC.PerceptionChannel(n, PC.layout_dma(), 3, ALL_ON, 77, DEV, done_stride=3)

    a = channel()
    a.start(frames[0])
    for t in range(1, 5):
        a.perceive(frames[t], frames[t - 1], dones[t])
    state = a.state_dict()
    assert state["call"] == 5 and sorted(state) == ["age", "call", "obs_out", "ring", "term_out"]
    assert all(v.device.type == "cpu" for k, v in state.items() if k != "call")
    b = channel()
    b.load_state_dict(state)
    for t in range(5, 8):
        oa, ta = a.perceive(frames[t], frames[t - 1], dones[t])
        ob, tb = b.perceive(frames[t], frames[t - 1], dones[t])
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    assert torch.equal(a.ring, b.ring) and torch.equal(a.age, b.age) and a.call == b.call == 8


def test_closed_loop_the_perceived_dma_wrapper_is_the_reference_on_the_true_rows():
    from envs.vss import VSS, default_cfg
    from envs.wrappers import DMA, Perceived
    n, D, seed = 33, 2, 4242
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 1234
    inner = DMA(VSS(cfg, DEV, DEV, 0, True, False, False))
    env = Perceived(inner, D, ALL_ON, seed)
    assert env.channel.layout == PC.layout_dma() and env.channel.done_stride == 3 and env.opponent_channel is None
    ring, age = np.zeros((D + 1, 1, n, 3, 52), F32), np.zeros(n, np.int32)

    def packed(t):
        return t.detach().cpu().numpy().reshape(n, 3, 52)[None]

    got = env.reset()["obs"]
    want, _ = PC.reference_perceive(packed(inner._obs), None, None, ring, age, 0, D, ALL_ON, seed)
    assert same_bits(packed(got), want)
    action = torch.zeros((3 * n, 2), device=DEV)
    early = late = 0
    max_len = int(inner.env.max_episode_length)
    for t in range(1, 451):
        obs, reward, dones, info = env.step(action)
        d = dones.cpu().numpy().reshape(n, 3)
        assert (d == d[:, :1]).all()
        want, want_t = PC.reference_perceive(packed(inner._obs), packed(inner._terminal_obs), d[:, 0], ring, age, t, D,
                                             ALL_ON, seed)
        assert same_bits(packed(obs["obs"]), want), t
        assert same_bits(packed(info["terminal_observation"]), want_t), t
        assert reward is inner._reward and dones is inner._dones and info["rews"] is inner._rews
        assert info["time_outs"] is inner._time_outs and info["progress_buffer"] is inner._progress
        assert np.array_equal(env.channel.age.cpu().numpy(), age), t
        time_outs = info["time_outs"].cpu().numpy().reshape(n, 3)[:, 0]
        early += int((d[:, 0] != 0).sum() - (time_outs & (d[:, 0] != 0)).sum())
        late += int((time_outs & (d[:, 0] != 0)).sum())
    print("closed loop: episodes ended by a goal", early, "by the time-out", late, "episode length", max_len)
    assert early > 0 and late > 0 and env.channel.call == 451
    assert same_bits(env.channel.ring.cpu().numpy(), ring)


def test_play_matches_with_a_channel_on_blues_rows():
    from envs.vss import VSS, default_cfg
    from play import get_team, play_matches
    n = 64
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 77
    cfg["env"]["maxEpisodeLength"] = 60
    env = VSS(cfg, DEV, DEV, 0, True, False, False)
    env.w_goal, env.w_grad, env.w_move, env.w_energy = 1.0, 0.0, 0.0, 0.0
    ch = PC.PerceptionChannel(n, PC.layout_full_blue(), 2, ALL_ON, 5, DEV, rows=6 * n)
    seen = []

    class Blue:
        def __call__(self, act, obs):
            seen.append((obs.data_ptr(), tuple(obs.shape), tuple(obs.stride())))
            act.zero_()

    score, length = play_matches(env, Blue(), get_team("scripted"), 64, chunk=64, perceive=ch)
    assert -1.0 <= score <= 1.0 and 0 < length <= 60
    assert set(seen) == {(ch.obs_out.data_ptr(), (n, 3, 52), (312, 52, 1))} and ch.call == len(seen) + 1
