"""vss_estimate on the GPU (csrc/vss_estimate.hip): the kernel equals
vss_amd.estimate.reference_estimate bit for bit -- both outputs, the command ring and the ages after every one of 12
calls, for every layout a wrapper uses, delays 0, 1, 3, 15 -- writes nothing outside its rows, and the Estimated
wrapper's closed loop on a perceived DMA env (goals, time-outs, resets) is the reference fed with Perceived's outputs."""
import ctypes

import numpy as np
import pytest
import torch

from test_perceive_cpu import ALL_ON, done_patterns, same_bits
from test_perceive_gpu import SENTINEL, Rows, is_sentinel
from vss_amd import _native as N
from vss_amd import estimate as E
from vss_amd import perceive as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CALLS = 12

# name: (layout for n fields, done stride): §17.2's table, plus a field stride of 4
LAYOUTS = {
    "sa": (lambda n: E.layout_sa(), 1),
    "dma": (lambda n: E.layout_dma(), 3),
    "mirror-sa": (lambda n: E.layout_mirror(1, n), 1),
    "mirror-dma": (lambda n: E.layout_mirror(3, n), 3),
    "opponent": (lambda n: E.layout_opponent(), 3),
    "full-blue": (lambda n: E.layout_full_blue(), 1),
    "stride-4": (lambda n: E.Layout(4, 0, 3, 1), 2),
}


def plausible_rows(g, shape):
    """Rows a camera could deliver: positions on the field, speeds up to 1.5 m/s, unit headings, yaw rates up to
    60 rad/s (w h beyond 0.78 takes sincos_small's reduced path), commands a little beyond [-1, 1].  Everything stays
    finite over 15 steps, so no NaN's sign (the one thing a CPU and a GPU may differ in) can occur."""
    rows = np.zeros(shape + (52,), F32)
    rows[..., 0:2] = g.uniform(-0.7, 0.7, shape + (2,))
    rows[..., 2:4] = g.uniform(-1.5, 1.5, shape + (2,))
    for base in E.OWN + E.OPPONENTS:
        yaw = g.uniform(-np.pi, np.pi, shape)
        rows[..., base:base + 2] = g.uniform(-0.7, 0.7, shape + (2,))
        rows[..., base + 2:base + 4] = g.uniform(-1.5, 1.5, shape + (2,))
        rows[..., base + 4], rows[..., base + 5] = np.cos(yaw), np.sin(yaw)
        rows[..., base + 6] = g.uniform(-60, 60, shape)
    rows[..., list(PC.ACTION_FLOATS)] = g.uniform(-1.2, 1.2, shape + (6,))
    return rows


def run_case(n, layout, done_stride, delay, seed, share=0.7):
    """`share` of the terminal rows are the rows themselves (what perception delivers for a field that is not done:
    the kernel computes one prediction for both), the others differ."""
    lay = E.Layout(*layout)
    idx = lay.row_index(n)  # (teams, n, robots)
    span = lay.span(n)
    covered = np.zeros(span, bool)
    covered[idx.reshape(-1)] = True
    g = np.random.default_rng(seed)
    shape = (lay.n_teams, n, lay.robots)
    m = lay.n_teams * n * lay.robots
    dones = done_patterns(CALLS, n)
    at = torch.from_numpy(idx.reshape(-1)).to(DEV)
    obs_b, term_b, out_b, tout_b = Rows(span), Rows(span), Rows(span), Rows(span)
    hist_b = Rows(max(delay, 1) * m, 6)
    age_b = Rows(m, 1, torch.int32)
    done_b = Rows((n - 1) * done_stride + 1, 1, torch.long)
    c_lay = E.VssEstimateLayout(*lay)
    hist, age = np.zeros((delay,) + shape + (6,), F32), np.zeros(shape, np.int32)
    lib, stream = N.load(), N.stream_of(torch.device(DEV))
    for t in range(CALLS):
        obs = plausible_rows(g, shape)
        term = np.where((g.random(shape) < share)[..., None], obs, plausible_rows(g, shape))
        term[..., 11] = np.where(g.random(shape) < 0.5, term[..., 11], F32(0.25))  # equal but for an own-action float
        obs[0, 0, 0, 0], obs[0, 0, 0, 2] = -0.0, -0.0  # a lead of 0 copies the sign of zero
        start = t == 0
        obs_b.body()[at] = torch.from_numpy(obs.reshape(-1, 52)).to(DEV)
        term_b.body()[at] = torch.from_numpy(term.reshape(-1, 52)).to(DEV)
        done_b.body()[::done_stride, 0] = torch.from_numpy(dones[t]).to(DEV)
        out_b.fill()
        tout_b.fill()
        rc = lib.vss_estimate(stream, n, ctypes.byref(c_lay), delay, t, obs_b.ptr, None if start else term_b.ptr, done_b.ptr,
                              done_stride, hist_b.ptr if delay else None, age_b.ptr, out_b.ptr, None if start else tout_b.ptr)
        assert rc == 0
        want_o, want_t = E.reference_estimate(obs, None if start else term, dones[t], hist, age, t, delay)
        assert np.isfinite(want_o).all() and (start or np.isfinite(want_t).all())
        torch.cuda.synchronize()
        tag = (n, tuple(lay), delay, t)
        got_o, ok = out_b.host()
        assert ok and same_bits(got_o[idx.reshape(-1)], want_o.reshape(-1, 52)), tag
        assert is_sentinel(got_o[~covered]).all(), tag  # rows between a strided layout's rows
        got_t, ok = tout_b.host()
        assert ok, tag
        if start:
            assert is_sentinel(got_t).all(), tag
        else:
            assert same_bits(got_t[idx.reshape(-1)], want_t.reshape(-1, 52)) and is_sentinel(got_t[~covered]).all(), tag
        got_hist, ok = hist_b.host()
        assert ok, tag
        if delay:
            # slots no call has written yet still hold the sentinel; the reference's hold zeros
            written = np.zeros(delay, bool)
            written[[c % delay for c in range(t + 1)]] = True
            got_hist = got_hist.reshape(hist.shape)
            assert same_bits(got_hist[written], hist[written]) and is_sentinel(got_hist[~written]).all(), tag
        else:
            assert is_sentinel(got_hist).all(), tag  # D = 0: hist is not touched
        got_age, ok = age_b.host()
        assert ok and np.array_equal(got_age[:, 0].reshape(shape), age), tag
        for b in (obs_b, term_b, done_b):  # the inputs are only read
            assert b.host()[1], tag


@pytest.mark.parametrize("delay", [0, 1, 3, 15])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_kernel_equals_the_reference_bit_for_bit(name, delay):
    make, done_stride = LAYOUTS[name]
    for n in (1, 33, 67):
        run_case(n, make(n), done_stride, delay, seed=1000 * n + delay)


def test_more_than_one_workgroup_and_a_team_stride_with_a_gap():
    """641 fields: 3 workgroups of 256 rows for SA, 16 for two teams of three; the yellow block 7 rows further than it
    must be; delays 2 and 4 (the three-entry history) and 5 (the fourteen-entry one)."""
    n = 641
    run_case(n, E.Layout(1), 1, 4, 5)
    run_case(n, E.Layout(3, 3 * n + 7, 3, 2), 3, 2, 6)
    run_case(n, E.Layout(4, 0, 3, 1), 2, 5, 7)


def test_full_layout_yellow_rows_are_untouched():
    n = 33
    g = np.random.default_rng(2)
    full = torch.from_numpy(plausible_rows(g, (n, 2, 3))).to(DEV)
    ch = E.EstimationChannel(n, E.layout_full_blue(), 2, DEV, rows=6 * n)
    ch.obs_out.view(torch.int32).fill_(SENTINEL)
    ch.term_out.view(torch.int32).fill_(SENTINEL)
    out = ch.start(full)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    out2, term2 = ch.estimate(full, full, done)
    torch.cuda.synchronize()
    for o in (out2, term2):
        assert o.shape == full.shape and out.data_ptr() == ch.obs_out.data_ptr()
        assert bool((o[:, 1].contiguous().view(torch.int32) == SENTINEL).all())
        assert not bool((o[:, 0].contiguous().view(torch.int32) == SENTINEL).any())
    acts = list(PC.ACTION_FLOATS)
    assert ch.call == 2 and ch.hist.shape == (2, 1, n, 3, 6) and torch.equal(ch.hist[1, 0], full[:, 0][..., acts])
    assert bool((ch.age == 1).all()) and not torch.equal(out2[:, 0], full[:, 0])


def test_the_bindings_refusals():
    n = 8
    with pytest.raises(ValueError, match="delay"):
        E.EstimationChannel(n, E.layout_sa(), 16, DEV)
    with pytest.raises(ValueError, match="spans"):
        E.EstimationChannel(n, E.layout_dma(), 1, DEV, rows=8)
    with pytest.raises(N.NativeError):
        E.EstimationChannel(n, E.layout_sa(), 1, "cpu")
    ch = E.EstimationChannel(n, E.layout_sa(), 1, DEV)
    obs = torch.zeros((n, 52), device=DEV)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="obs"):
        ch.start(torch.zeros((n + 1, 52), device=DEV))
    with pytest.raises(ValueError, match="obs"):
        ch.start(obs.double())
    with pytest.raises(ValueError, match="term"):
        ch.estimate(obs, obs[:, :51], done)
    with pytest.raises(ValueError, match="done"):
        ch.estimate(obs, obs, done.int())
    with pytest.raises(ValueError, match="done"):
        ch.estimate(obs, obs, done[:-1])
    with pytest.raises(N.NativeError, match="vss_estimate"):
        ch.estimate(ch.obs_out, obs, done)  # an output as an input: the entry's own refusal
    assert ch.call == 0
    bad = E.VssEstimateLayout(1, 0, 2, 1)
    rc = N.load().vss_estimate(N.stream_of(torch.device(DEV)), n, ctypes.byref(bad), 1, 0, obs.data_ptr(), None,
                               done.data_ptr(), 1, ch.hist.data_ptr(), ch.age.data_ptr(), ch.obs_out.data_ptr(), None)
    assert rc == 1


def test_state_dict_round_trip_continues_bit_equal():
    n, g = 33, np.random.default_rng(3)
    frames = torch.from_numpy(plausible_rows(g, (8, n, 3))).to(DEV)
    dones = torch.from_numpy((g.random((8, n)) < 0.3).astype(np.int64)).repeat_interleave(3, 1).contiguous().to(DEV)

    def channel():
        return E.EstimationChannel(n, E.layout_dma(), 3, DEV, done_stride=3)

    a = channel()
    a.start(frames[0])
    for t in range(1, 5):
        a.estimate(frames[t], frames[t - 1], dones[t])
    state = a.state_dict()
    assert state["call"] == 5 and sorted(state) == ["age", "call", "hist", "obs_out", "term_out"]
    assert all(v.device.type == "cpu" for k, v in state.items() if k != "call")
    b = channel()
    b.load_state_dict(state)
    for t in range(5, 8):
        oa, ta = a.estimate(frames[t], frames[t - 1], dones[t])
        ob, tb = b.estimate(frames[t], frames[t - 1], dones[t])
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    assert torch.equal(a.hist, b.hist) and torch.equal(a.age, b.age) and a.call == b.call == 8


def test_closed_loop_the_estimated_dma_wrapper_is_the_reference_on_perceiveds_outputs():
    from envs.vss import VSS, default_cfg
    from envs.wrappers import DMA, Estimated, Perceived
    n, D, seed = 33, 2, 4242
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 1234
    inner = DMA(VSS(cfg, DEV, DEV, 0, True, False, False))
    seen = Perceived(inner, D, ALL_ON, seed)
    env = Estimated(seen)
    assert env.channel.layout == E.layout_dma() and env.channel.done_stride == 3 and env.opponent_channel is None
    hist, age = np.zeros((D, 1, n, 3, 6), F32), np.zeros((1, n, 3), np.int32)

    def packed(t):
        return t.detach().cpu().numpy().reshape(n, 3, 52)[None]

    got = env.reset()["obs"]
    want, _ = E.reference_estimate(packed(seen.channel.obs_out), None, None, hist, age, 0, D)
    assert same_bits(packed(got), want) and same_bits(want, packed(seen.channel.obs_out))
    action = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (3 * n, 2)).astype(F32)).to(DEV)  # fixed, non-zero
    early = late = 0
    moved = 0.0
    for t in range(1, 451):
        obs, reward, dones, info = env.step(action)
        d = dones.cpu().numpy().reshape(n, 3)
        assert (d == d[:, :1]).all()
        want, want_t = E.reference_estimate(packed(seen.channel.obs_out), packed(seen.channel.term_out), d[:, 0], hist, age, t, D)
        assert same_bits(packed(obs["obs"]), want), t
        assert same_bits(packed(info["terminal_observation"]), want_t), t
        assert reward is inner._reward and dones is inner._dones and info["rews"] is inner._rews
        assert info["time_outs"] is inner._time_outs and info["progress_buffer"] is inner._progress
        assert np.array_equal(env.channel.age.cpu().numpy(), age), t
        moved = max(moved, float(np.abs(want - packed(seen.channel.obs_out)).max()))
        time_outs = info["time_outs"].cpu().numpy().reshape(n, 3)[:, 0]
        early += int((d[:, 0] != 0).sum() - (time_outs & (d[:, 0] != 0)).sum())
        late += int((time_outs & (d[:, 0] != 0)).sum())
    print("closed loop: episodes ended by a goal", early, "by the time-out", late, "largest change by the estimate", moved)
    assert early > 0 and late > 0 and env.channel.call == 451 and moved > 0.01
    assert same_bits(env.channel.hist.cpu().numpy(), hist)


def test_play_matches_with_perception_and_estimation_channels_on_blues_rows():
    from envs.vss import VSS, default_cfg
    from play import get_team, play_matches
    n = 64
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 77
    cfg["env"]["maxEpisodeLength"] = 60
    env = VSS(cfg, DEV, DEV, 0, True, False, False)
    env.w_goal, env.w_grad, env.w_move, env.w_energy = 1.0, 0.0, 0.0, 0.0
    ch = PC.PerceptionChannel(n, PC.layout_full_blue(), 2, ALL_ON, 5, DEV, rows=6 * n)
    est = E.EstimationChannel(n, E.layout_full_blue(), 2, DEV, rows=6 * n)
    seen = []

    class Blue:
        def __call__(self, act, obs):
            seen.append((obs.data_ptr(), tuple(obs.shape), tuple(obs.stride())))
            act.fill_(0.5)

    score, length = play_matches(env, Blue(), get_team("scripted"), 64, chunk=64, perceive=ch, estimate=est)
    assert -1.0 <= score <= 1.0 and 0 < length <= 60
    assert set(seen) == {(est.obs_out.data_ptr(), (n, 3, 52), (312, 52, 1))} and ch.call == est.call == len(seen) + 1
    assert not torch.equal(est.obs_out, ch.obs_out)
