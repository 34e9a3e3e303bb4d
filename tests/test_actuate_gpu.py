"""vss_actuate on the GPU (csrc/vss_actuate.hip): the kernel equals
vss_amd.actuate.reference_actuate bit for bit -- out, held, gain and episode after every one of 12 calls, for every layout
a wrapper uses, every effect off, alone and all on -- writes nothing outside its commands, works in place, honours a
hand-set gain, and the Actuated wrapper's closed loop on a DMA env (goals, time-outs, resets) is the reference fed with
the same commands, whose output the step consumes."""
import ctypes

import numpy as np
import pytest
import torch

from test_actuate_cpu import ALL_ON, done_patterns, same_bits
from vss_amd import _native as N
from vss_amd import actuate as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SENTINEL = 0x7FA5A5A5  # tests/test_write_extents.py's quiet-NaN pattern
GUARD = 16             # sentinel elements in front of and behind every buffer
CALLS = 12

# name: (layout for n fields, done stride)
LAYOUTS = {
    "sa": (lambda n: A.layout_sa(), 1),
    "team": (lambda n: A.layout_team(), 3),          # CMA (N, 6) / DMA (3 N, 2); DMA's dones are repeated per row
    "opponent": (lambda n: A.layout_opponent(), 1),
    "mirror-sa": (lambda n: A.layout_mirror(1, n), 1),
    "mirror-team": (lambda n: A.layout_mirror(3, n), 3),
    "full-blue": (lambda n: A.layout_full_blue(), 1),  # gaps: the yellow half
    "stride-4-yellow": (lambda n: A.Layout(4, 0, 3, 1, 1), 2),
    "sa-yellow": (lambda n: A.Layout(1, 0, 1, 1, 1), 1),
}
PARAMS = [A.Params(), A.Params(gain_sigma=0.05), A.Params(noise_sigma=0.02), A.Params(deadband=0.03), A.Params(loss_prob=0.1),
          A.Params(levels=127), ALL_ON]


class Buf:
    """A device buffer of `rows` x `width` elements between two guard bands, everything the sentinel at first."""

    def __init__(self, rows, width=2, dtype=torch.float32):
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
        """(the body, True when both guard bands still hold the sentinel) on the host."""
        a = self.t.view(-1, self.width).cpu()
        bits = a.view(torch.int32) if a.dtype == torch.float32 else a
        intact = bool((bits[:GUARD] == SENTINEL).all() and (bits[GUARD + self.rows:] == SENTINEL).all())
        return a[GUARD:GUARD + self.rows].numpy(), intact


def is_sentinel(a):
    return np.ascontiguousarray(a, F32).view(np.uint32) == SENTINEL


def commands(g, shape):
    """Commands that leave [-1, 1] now and then, with both zeros and the range's ends among them."""
    cmd = g.uniform(-1.3, 1.3, shape).astype(F32)
    cmd[0, 0, 0] = (-0.0, 0.0)
    if shape[1] > 1:
        cmd[0, 1, 0] = (1.0, -1.0)
    return cmd


def run_case(n, layout, done_stride, params, seed, in_place=False, set_gain_at=None):
    lay = A.Layout(*layout)
    idx = lay.index(n).reshape(-1)  # (teams, n, robots) flattened
    span = lay.span(n)
    covered = np.zeros(span, bool)
    covered[idx] = True
    g = np.random.default_rng(seed)
    shape = (lay.n_teams, n, lay.robots, 2)
    dones = done_patterns(CALLS, n)
    at = torch.from_numpy(idx).to(DEV)
    cmd_b, out_b = Buf(span), Buf(span)
    held_b, gain_b = Buf(lay.n_teams * n * lay.robots), Buf(lay.n_teams * n * lay.robots)
    ep_b = Buf(n, 1, torch.int32)
    ep_b.body().zero_()
    done_b = Buf((n - 1) * done_stride + 1, 1, torch.long)
    c_lay, c_prm = A.VssActuateLayout(*lay), A.VssActuateParams(*params)
    held, gain, episode = np.zeros(shape, F32), np.ones(shape, F32), np.zeros(n, np.uint32)
    lib, stream = N.load(), N.stream_of(torch.device(DEV))
    for t in range(CALLS):
        cmd = commands(g, shape)
        start = t == 0
        cmd_b.fill()
        cmd_b.body()[at] = torch.from_numpy(cmd.reshape(-1, 2)).to(DEV)
        done_b.body()[::done_stride, 0] = torch.from_numpy(dones[t]).to(DEV)
        out_b.fill()
        if set_gain_at == t:
            mine = g.uniform(0.7, 1.3, shape).astype(F32)
            gain[:] = mine
            gain_b.body().copy_(torch.from_numpy(mine.reshape(-1, 2)).to(DEV))
        dst = cmd_b if in_place else out_b
        rc = lib.vss_actuate(stream, n, ctypes.byref(c_lay), ctypes.byref(c_prm), seed, t, cmd_b.ptr,
                             None if start else done_b.ptr, done_stride, held_b.ptr, gain_b.ptr, ep_b.ptr, dst.ptr)
        assert rc == 0
        want = A.reference_actuate(cmd, None if start else dones[t], held, gain, episode, t, params, seed, lay.first_team)
        torch.cuda.synchronize()
        tag = (n, tuple(lay), tuple(params), t, in_place)
        got, ok = dst.host()
        assert ok and same_bits(got[idx], want.reshape(-1, 2)), tag
        assert is_sentinel(got[~covered]).all(), tag  # floats between a strided layout's commands
        if not in_place:
            src, ok = cmd_b.host()
            assert ok and same_bits(src[idx], cmd.reshape(-1, 2)) and is_sentinel(src[~covered]).all(), tag  # only read
        else:
            assert is_sentinel(out_b.host()[0]).all(), tag
        got_h, ok = held_b.host()
        assert ok and same_bits(got_h, held.reshape(-1, 2)), tag
        got_g, ok = gain_b.host()
        assert ok and same_bits(got_g, gain.reshape(-1, 2)), tag
        got_e, ok = ep_b.host()
        assert ok and np.array_equal(got_e[:, 0].view(np.uint32), episode), tag
        assert done_b.host()[1], tag


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_kernel_equals_the_reference_bit_for_bit(name):
    make, done_stride = LAYOUTS[name]
    for n in (1, 33, 67):
        for i, params in enumerate(PARAMS):
            run_case(n, make(n), done_stride, params, seed=(1 << 33) + 1000 * n + i)


def test_more_than_one_workgroup_and_a_team_stride_with_a_gap():
    """641 fields: three workgroups of 256; the yellow block 7 robots further than it must be."""
    n = 641
    run_case(n, A.Layout(1), 1, ALL_ON, 5)
    run_case(n, A.Layout(3, 3 * n + 7, 3, 2, 0), 3, ALL_ON, 6)
    run_case(n, A.Layout(4, 0, 3, 1, 1), 2, ALL_ON, 7)


@pytest.mark.parametrize("name", ["opponent", "full-blue", "mirror-team"])
def test_in_place_equals_out_of_place(name):
    make, done_stride = LAYOUTS[name]
    for n in (33, 300):
        run_case(n, make(n), done_stride, ALL_ON, seed=77 + n, in_place=True)  # against the same reference


def test_a_hand_set_gain_is_honoured_until_the_next_episode():
    run_case(67, A.layout_team(), 3, A.Params(gain_sigma=0.05), seed=11, set_gain_at=3)
    run_case(67, A.layout_mirror(1, 67), 1, A.Params(), seed=12, set_gain_at=2)
    # through the channel: the caller overwrites ch.gain between calls
    n = 8
    ch = A.ActuationChannel(n, A.layout_sa(), A.Params(gain_sigma=0.1), 3, DEV)
    cmd = torch.full((n, 2), 0.5, device=DEV)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    ch.actuate(cmd)
    ch.gain.copy_(torch.tensor([0.8, 1.25], device=DEV).expand(1, n, 1, 2))
    done[3] = 1
    out = ch.actuate(cmd, done).cpu()
    keep = [f for f in range(n) if f != 3]
    assert torch.equal(out[keep], torch.tensor([0.4, 0.625]).expand(n - 1, 2))
    assert not torch.equal(out[3], torch.tensor([0.4, 0.625])) and torch.equal(cmd.cpu(), torch.full((n, 2), 0.5))
    assert ch.episode.cpu().tolist() == [1, 1, 1, 2, 1, 1, 1, 1] and ch.call == 2


def test_the_bindings_refusals():
    n = 8
    with pytest.raises(ValueError, match="gain"):
        A.ActuationChannel(n, A.layout_sa(), A.Params(gain_sigma=0.5), 1, DEV)
    with pytest.raises(ValueError, match="levels"):
        A.ActuationChannel(n, A.layout_sa(), A.Params(levels=1 << 15), 1, DEV)
    with pytest.raises(ValueError, match="spans"):
        A.ActuationChannel(n, A.layout_team(), A.Params(), 1, DEV, rows=8)
    with pytest.raises(N.NativeError):
        A.ActuationChannel(n, A.layout_sa(), A.Params(), 1, "cpu")
    ch = A.ActuationChannel(n, A.layout_sa(), ALL_ON, 1, DEV)
    cmd = torch.zeros((n, 2), device=DEV)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="cmd"):
        ch.actuate(torch.zeros((n + 1, 2), device=DEV))
    with pytest.raises(ValueError, match="cmd"):
        ch.actuate(cmd.double())
    with pytest.raises(ValueError, match="out"):
        ch.actuate(cmd, out=torch.zeros_like(cmd))
    with pytest.raises(N.NativeError, match="vss_actuate"):
        ch.actuate(ch.held.view(n, 2))  # the state as the commands: the entry's own refusal
    assert ch.call == 0 and ch.fresh
    ch.actuate(cmd)  # the start call reads no done flag
    with pytest.raises(ValueError, match="done_prev"):
        ch.actuate(cmd)
    with pytest.raises(ValueError, match="done_prev"):
        ch.actuate(cmd, done.int())
    with pytest.raises(ValueError, match="done_prev"):
        ch.actuate(cmd, done[:-1])
    assert ch.call == 1
    bad = A.VssActuateLayout(1, 0, 2, 1, 0)
    prm = A.VssActuateParams(0, 0, 0, 0, 0)
    rc = N.load().vss_actuate(N.stream_of(torch.device(DEV)), n, ctypes.byref(bad), ctypes.byref(prm), 1, 0, cmd.data_ptr(),
                              None, 1, ch.held.data_ptr(), ch.gain.data_ptr(), ch.episode.data_ptr(), ch.out.data_ptr())
    assert rc == 1


def test_state_dict_round_trip_continues_bit_equal():
    n, g = 33, torch.Generator(device="cpu").manual_seed(3)
    cmds = (torch.rand((8, 3 * n, 2), generator=g) * 2.4 - 1.2).to(DEV)
    dones = (torch.rand((8, n), generator=g) < 0.3).long().repeat_interleave(3, 1).contiguous().to(DEV)

    def channel():
        return A.ActuationChannel(n, A.layout_team(), ALL_ON, 77, DEV, done_stride=3)

    a = channel()
    for t in range(5):
        a.actuate(cmds[t], dones[t])
    state = a.state_dict()
    assert state["call"] == 5 and state["fresh"] is False
    assert sorted(state) == ["call", "episode", "fresh", "gain", "held", "out"]
    assert all(v.device.type == "cpu" for k, v in state.items() if k not in ("call", "fresh"))
    b = channel()
    assert b.fresh and channel().state_dict()["fresh"] is True
    b.load_state_dict(state)
    assert torch.equal(a.out.view(torch.int32), b.out.view(torch.int32))
    for t in range(5, 8):
        oa, ob = a.actuate(cmds[t], dones[t]), b.actuate(cmds[t], dones[t])
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and oa.data_ptr() != ob.data_ptr()
    assert torch.equal(a.held, b.held) and torch.equal(a.gain, b.gain) and torch.equal(a.episode, b.episode)
    assert a.call == b.call == 8
    a.start(call=0, zero=True)  # afresh: as a new channel
    c = channel()
    assert torch.equal(a.actuate(cmds[0]).view(torch.int32), c.actuate(cmds[0]).view(torch.int32)) and a.call == 1


def test_closed_loop_the_actuated_dma_wrapper_is_the_reference_and_the_step_consumes_it():
    from envs.vss import VSS, default_cfg
    from envs.wrappers import DMA, Actuated
    n, seed = 33, 4242
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 1234
    vss = VSS(cfg, DEV, DEV, 0, True, False, False)
    inner = DMA(vss)
    env = Actuated(inner, ALL_ON, seed)
    assert env.channel.layout == A.layout_team() and env.channel.done_stride == 3 and env.opponent_channel is None
    assert env.ROWS_PER_FIELD == 3 and env.action_buf is inner.action_buf
    held, gain, episode = np.zeros((1, n, 3, 2), F32), np.ones((1, n, 3, 2), F32), np.zeros(n, np.uint32)
    obs = env.reset()
    assert obs["obs"] is inner._obs
    g = torch.Generator(device="cpu").manual_seed(5)
    action = (torch.rand((3 * n, 2), generator=g) * 2.2 - 1.1).to(DEV)  # fixed, non-zero, some beyond the radio's range
    action[:3] = torch.tensor([[0.9, 0.9], [0.8, 0.85], [1.0, 0.7]], device=DEV)  # field 0 drives on: goals happen
    sent = action.clone()
    cmd = action.cpu().numpy().reshape(1, n, 3, 2)
    prev = None
    early = late = 0
    for t in range(450):
        o, reward, dones, info = env.step(action)
        want = A.reference_actuate(cmd, prev, held, gain, episode, t, ALL_ON, seed)
        applied = env.channel.out.cpu().numpy().reshape(1, n, 3, 2)
        assert same_bits(applied, want), t
        d = dones.cpu().numpy().reshape(n, 3)
        assert (d == d[:, :1]).all() and dones is inner._dones and o["obs"] is inner._obs and reward is inner._reward
        prev = d[:, 0].copy()
        # the step recorded what it was given: the clamped applied commands (times zero where the field was reset)
        dof = vss.dof_velocity_buf.cpu().numpy()[:, 0]
        assert np.array_equal(dof, np.clip(applied[0], -1, 1) * (prev == 0)[:, None, None].astype(F32)), t
        time_outs = info["time_outs"].cpu().numpy().reshape(n, 3)[:, 0]
        early += int(((prev != 0) & ~time_outs).sum())
        late += int(((prev != 0) & time_outs).sum())
    print("closed loop: episodes ended by a goal", early, "by the time-out", late)
    assert early > 0 and late > 0 and env.channel.call == 450
    assert torch.equal(action, sent)  # the policy's action tensor is never modified
    assert same_bits(env.channel.held.cpu().numpy(), held) and same_bits(env.channel.gain.cpu().numpy(), gain)
    assert np.array_equal(env.channel.episode.cpu().numpy().view(np.uint32), episode) and episode.max() > 1


def test_play_matches_with_a_channel_on_blues_commands():
    from envs.vss import VSS, default_cfg
    from play import get_team, play_matches
    n = 64
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 77
    cfg["env"]["maxEpisodeLength"] = 60
    env = VSS(cfg, DEV, DEV, 0, True, False, False)
    env.w_goal, env.w_grad, env.w_move, env.w_energy = 1.0, 0.0, 0.0, 0.0
    ch = A.ActuationChannel(n, A.layout_full_blue(), A.Params(levels=4, deadband=0.3), 5, DEV, rows=6 * n)
    seen = []

    class Blue:
        def __call__(self, act, obs):
            act.copy_(torch.tensor([[0.6, -0.2], [0.1, 0.95], [-0.4, 0.3]], device=act.device).expand(n, 3, 2))

    class Yellow:
        def __call__(self, act, obs):
            seen.append(act._base.clone())  # the whole (N, 2, 3, 2) buffer
            act.fill_(0.37)

    score, length = play_matches(env, Blue(), Yellow(), 64, chunk=64, actuate=ch)
    assert -1.0 <= score <= 1.0 and 0 < length <= 60 and ch.call == len(seen) > 0
    want = torch.tensor([[0.5, 0.0], [0.0, 1.0], [-0.5, 0.0]], device=DEV).expand(n, 3, 2)  # rint(4 c) / 4, |r| < 0.3 -> 0
    for buf in seen:  # the action buffer as yellow finds it: blue's half applied in place, its own half never touched
        assert torch.equal(buf[:, 0], want)
        assert bool((buf[:, 1] == 0).all() | (buf[:, 1] == 0.37).all())
    ch.start(call=0, zero=True)
    assert play_matches(env, Blue(), Yellow(), 64, chunk=64, actuate=None)[1] > 0 and ch.call == 0
