"""vss_track on the GPU (csrc/vss_track.hip): the kernel equals vss_amd.track.reference_track bit
for bit -- both outputs, the filtered rows, the command ring and the ages after every one of 12 calls, for every layout
a wrapper uses, delays 0, 1, 3, 15, with a kind off, with the gates off, on rows that follow the filter and rows that
jump through each gate -- writes nothing outside its rows, and the Tracked wrapper's closed loop on perceived envs
(goals, time-outs, resets) is the reference fed with Perceived's outputs."""
import ctypes

import numpy as np
import pytest
import torch

from test_perceive_cpu import ALL_ON, done_patterns, same_bits
from test_perceive_gpu import SENTINEL, Rows, is_sentinel
from vss_amd import _native as N
from vss_amd import estimate as E
from vss_amd import perceive as PC
from vss_amd import track as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CALLS = 12
ACTS = list(PC.ACTION_FLOATS)

# name: (layout for n fields, done stride): §17.2's table, plus a field stride of 4
LAYOUTS = {
    "sa": (lambda n: T.layout_sa(), 1),
    "dma": (lambda n: T.layout_dma(), 3),
    "mirror-sa": (lambda n: T.layout_mirror(1, n), 1),
    "mirror-dma": (lambda n: T.layout_mirror(3, n), 3),
    "opponent": (lambda n: T.layout_opponent(), 3),
    "full-blue": (lambda n: T.layout_full_blue(), 1),
    "stride-4": (lambda n: T.Layout(4, 0, 3, 1), 2),
}
# the gates are wide enough for a row that follows the filter (0.075 m and 0.3 m/s per step at the most) to pass
PARAMS = [T.Params(0.2, 0.5, 0.6, 0.2, 1.0), T.Params(0.25, 0.0, 0.5, 0.2, 1.0), T.Params(1.0, 0.3, 0.0, 0.0, 0.0),
          T.Params(0.0, 0.7, 0.0, 0.15, 0.0)]


def first_rows(g, shape):
    """Rows a camera could deliver: positions on the field, speeds up to 1.5 m/s, unit headings, yaw rates up to
    8 rad/s (a few up to 60: w h beyond 0.78 takes sincos_small's reduced path and turns a heading past the gate),
    commands a little beyond [-1, 1].  Everything stays finite, so no NaN's sign can occur."""
    rows = np.zeros(shape + (52,), F32)
    rows[..., 0:2] = g.uniform(-0.7, 0.7, shape + (2,))
    rows[..., 2:4] = g.uniform(-1.5, 1.5, shape + (2,))
    for base in E.OWN + E.OPPONENTS:
        yaw = g.uniform(-np.pi, np.pi, shape)
        rows[..., base:base + 2] = g.uniform(-0.7, 0.7, shape + (2,))
        rows[..., base + 2:base + 4] = g.uniform(-1.5, 1.5, shape + (2,))
        rows[..., base + 4], rows[..., base + 5] = np.cos(yaw), np.sin(yaw)
        rows[..., base + 6] = np.where(g.random(shape) < 0.1, g.uniform(-60, 60, shape), g.uniform(-8, 8, shape))
    rows[..., ACTS] = g.uniform(-1.2, 1.2, shape + (6,))
    return rows


def following_rows(g, est, jump=0.25):
    """The next measurement of rows whose filter state is `est`: the state with noise on every pose (so most bodies
    take the blend), fresh commands, and in `jump` of the rows one body moved through one gate: position, velocity or,
    for a robot, the heading turned round."""
    shape = est.shape[:-1]
    z = est.copy()
    z[..., 0:4] += g.normal(0, [0.002, 0.002, 0.05, 0.05], shape + (4,)).astype(F32)
    for base in E.OWN + E.OPPONENTS:
        z[..., base:base + 4] += g.normal(0, [0.002, 0.002, 0.05, 0.05], shape + (4,)).astype(F32)
        turn = g.normal(0, 0.02, shape)
        c, s = z[..., base + 4].copy(), z[..., base + 5].copy()
        z[..., base + 4], z[..., base + 5] = c * np.cos(turn) - s * np.sin(turn), s * np.cos(turn) + c * np.sin(turn)
        z[..., base + 6] += g.normal(0, 0.5, shape).astype(F32)
    z[..., ACTS] = g.uniform(-1.2, 1.2, shape + (6,))
    bases = np.array((0,) + E.OWN + E.OPPONENTS)
    which = bases[g.integers(0, 7, shape)]
    gate = g.integers(0, 3, shape)
    hit = g.random(shape) < jump
    flat, w, k, h = z.reshape(-1, 52), which.reshape(-1), gate.reshape(-1), hit.reshape(-1)
    for r in np.nonzero(h)[0]:
        if k[r] == 0:
            flat[r, w[r] + g.integers(0, 2)] += F32(g.choice([-0.4, 0.4]))
        elif k[r] == 1:
            flat[r, w[r] + 2 + g.integers(0, 2)] += F32(g.choice([-2.0, 2.0]))
        elif w[r] != 0:
            flat[r, w[r] + 4:w[r] + 6] *= F32(-1.0)
    return z.astype(F32)


def run_case(n, layout, done_stride, delay, params, seed, share=0.7):
    """`share` of the terminal rows are the rows themselves (what perception delivers for a field that is not done),
    the others are another measurement of the same state."""
    lay = T.Layout(*layout)
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
    est_b = Rows(m)
    hist_b = Rows(max(delay, 1) * m, 6)
    age_b = Rows(m, 1, torch.int32)
    done_b = Rows((n - 1) * done_stride + 1, 1, torch.long)
    c_lay, c_prm = T.VssTrackLayout(*lay), T.VssTrackParams(*params)
    est = np.zeros(shape + (52,), F32)
    hist, age = np.zeros((delay,) + shape + (6,), F32), np.zeros(shape, np.int32)
    lib, stream = T.load(), N.stream_of(torch.device(DEV))
    blended = tripped = 0
    for t in range(CALLS):
        start = t == 0
        if start:
            obs = first_rows(g, shape)
            obs[0, 0, 0, 0], obs[0, 0, 0, 2] = -0.0, -0.0  # the start call copies the sign of zero
            term = obs
        else:
            obs = following_rows(g, est)
            term = np.where((g.random(shape) < share)[..., None], obs, following_rows(g, est))
            fresh = np.broadcast_to((dones[t] != 0)[None, :, None], shape)
            obs[fresh] = first_rows(g, shape)[fresh]  # a field that is done delivers its new episode's first row
        obs_b.body()[at] = torch.from_numpy(obs.reshape(-1, 52)).to(DEV)
        term_b.body()[at] = torch.from_numpy(term.reshape(-1, 52)).to(DEV)
        done_b.body()[::done_stride, 0] = torch.from_numpy(dones[t]).to(DEV)
        out_b.fill()
        tout_b.fill()
        rc = lib.vss_track(stream, n, ctypes.byref(c_lay), ctypes.byref(c_prm), delay, t, obs_b.ptr,
                           None if start else term_b.ptr, done_b.ptr, done_stride, est_b.ptr, hist_b.ptr if delay else None,
                           age_b.ptr, out_b.ptr, None if start else tout_b.ptr)
        assert rc == 0
        want_o, want_t = T.reference_track(obs, None if start else term, dones[t], est, hist, age, t, delay, params)
        assert np.isfinite(want_o).all() and (start or np.isfinite(want_t).all())
        torch.cuda.synchronize()
        tag = (n, tuple(lay), delay, tuple(params), t)
        got_o, ok = out_b.host()
        assert ok and same_bits(got_o[idx.reshape(-1)], want_o.reshape(-1, 52)), tag
        assert is_sentinel(got_o[~covered]).all(), tag  # rows between a strided layout's rows
        got_t, ok = tout_b.host()
        assert ok, tag
        if start:
            assert is_sentinel(got_t).all(), tag
        else:
            assert same_bits(got_t[idx.reshape(-1)], want_t.reshape(-1, 52)) and is_sentinel(got_t[~covered]).all(), tag
            for base, width in [(0, 4)] + [(b, 7) for b in E.OWN + E.OPPONENTS]:  # per body: corrected, or the input's floats
                moved = (want_t[..., base:base + width] != term[..., base:base + width]).any(-1)
                blended += int(moved.sum())
                tripped += int((~moved).sum())
        got_est, ok = est_b.host()
        assert ok and same_bits(got_est, est.reshape(-1, 52)) and same_bits(est, want_o), tag
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
    return blended, tripped


@pytest.mark.parametrize("delay", [0, 1, 3, 15])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_kernel_equals_the_reference_bit_for_bit(name, delay):
    make, done_stride = LAYOUTS[name]
    case = list(LAYOUTS).index(name) + [0, 1, 3, 15].index(delay)
    blended = 0
    for i, n in enumerate((1, 33, 67)):
        blended += run_case(n, make(n), done_stride, delay, PARAMS[(case + i) % len(PARAMS)], seed=1000 * n + delay)[0]
    assert blended > 0  # rows that took the filter's path, not only re-initialised ones


def test_more_than_one_workgroup_and_a_team_stride_with_a_gap():
    """641 fields: 3 workgroups of 256 rows for SA, 16 for two teams of three; the yellow block 7 rows further than it
    must be."""
    n = 641
    run_case(n, T.Layout(1), 1, 4, PARAMS[0], 5)
    run_case(n, T.Layout(3, 3 * n + 7, 3, 2), 3, 2, PARAMS[1], 6)
    run_case(n, T.Layout(4, 0, 3, 1), 2, 0, PARAMS[0], 7)


def test_every_gate_and_the_blend_occur_in_the_rows_compared():
    """The generator's jumps do reach each gate: with one gate on at a time, a share of the rows is re-initialised."""
    for params in (T.Params(0.3, 0.3, 0.3, 0.2, 0.0), T.Params(0.3, 0.3, 0.3, 0.0, 1.0), T.Params(0.3, 0.3, 0.3, 0.0, 0.0)):
        blended, tripped = run_case(67, T.layout_dma(), 3, 3, params, 11)
        assert blended > 100 and tripped > 5, (tuple(params), blended, tripped)


def test_full_layout_yellow_rows_are_untouched():
    n = 33
    g = np.random.default_rng(2)
    full = torch.from_numpy(first_rows(g, (n, 2, 3))).to(DEV)
    ch = T.TrackingChannel(n, T.layout_full_blue(), 2, T.Params(0.2, 0.5, 0.5), DEV, rows=6 * n)
    ch.obs_out.view(torch.int32).fill_(SENTINEL)
    ch.term_out.view(torch.int32).fill_(SENTINEL)
    out = ch.start(full)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    nxt = (full + 0.001).contiguous()
    out2, term2 = ch.track(nxt, nxt, done)
    torch.cuda.synchronize()
    for o in (out2, term2):
        assert o.shape == full.shape and out.data_ptr() == ch.obs_out.data_ptr()
        assert bool((o[:, 1].contiguous().view(torch.int32) == SENTINEL).all())
        assert not bool((o[:, 0].contiguous().view(torch.int32) == SENTINEL).any())
    assert ch.call == 2 and ch.hist.shape == (2, 1, n, 3, 6) and torch.equal(ch.hist[1, 0], nxt[:, 0][..., ACTS])
    assert ch.est.shape == (1, n, 3, 52) and torch.equal(ch.est[0], out2[:, 0])
    assert bool((ch.age == 1).all()) and not torch.equal(out2[:, 0], nxt[:, 0])


def test_the_bindings_refusals():
    n = 8
    on = T.Params(0.2, 0.5, 0.5)
    with pytest.raises(ValueError, match="delay"):
        T.TrackingChannel(n, T.layout_sa(), 16, on, DEV)
    with pytest.raises(ValueError, match="spans"):
        T.TrackingChannel(n, T.layout_dma(), 1, on, DEV, rows=8)
    with pytest.raises(ValueError, match="gain_team"):
        T.TrackingChannel(n, T.layout_sa(), 1, T.Params(1.5), DEV)
    with pytest.raises(ValueError, match="gate_vel"):
        T.TrackingChannel(n, T.layout_sa(), 1, T.Params(0.5, gate_vel=-1.0), DEV)
    with pytest.raises(N.NativeError):
        T.TrackingChannel(n, T.layout_sa(), 1, on, "cpu")
    ch = T.TrackingChannel(n, T.layout_sa(), 1, on, DEV)
    obs = torch.zeros((n, 52), device=DEV)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="obs"):
        ch.start(torch.zeros((n + 1, 52), device=DEV))
    with pytest.raises(ValueError, match="obs"):
        ch.start(obs.double())
    with pytest.raises(ValueError, match="term"):
        ch.track(obs, obs[:, :51], done)
    with pytest.raises(ValueError, match="done"):
        ch.track(obs, obs, done.int())
    with pytest.raises(ValueError, match="done"):
        ch.track(obs, obs, done[:-1])
    with pytest.raises(N.NativeError, match="vss_track"):
        ch.track(ch.obs_out, obs, done)  # an output as an input: the entry's own refusal
    with pytest.raises(N.NativeError, match="vss_track"):
        ch.track(ch.est.view(n, 52), obs, done)  # the state as an input
    assert ch.call == 0
    bad = T.VssTrackLayout(1, 0, 2, 1)
    rc = T.load().vss_track(N.stream_of(torch.device(DEV)), n, ctypes.byref(bad), ctypes.byref(ch._prm), 1, 0, obs.data_ptr(),
                            None, done.data_ptr(), 1, ch.est.data_ptr(), ch.hist.data_ptr(), ch.age.data_ptr(),
                            ch.obs_out.data_ptr(), None)
    assert rc == 1


def test_state_dict_round_trip_continues_bit_equal():
    n, g = 33, np.random.default_rng(3)
    first = first_rows(g, (n, 3))
    frames = [first]
    for _ in range(7):
        frames.append(following_rows(g, frames[-1]))
    frames = torch.from_numpy(np.stack(frames)).to(DEV)
    dones = torch.from_numpy((g.random((8, n)) < 0.3).astype(np.int64)).repeat_interleave(3, 1).contiguous().to(DEV)

    def channel():
        return T.TrackingChannel(n, T.layout_dma(), 3, T.Params(0.2, 0.5, 0.5, 0.2, 1.0), DEV, done_stride=3)

    a = channel()
    a.start(frames[0])
    for t in range(1, 5):
        a.track(frames[t], frames[t - 1], dones[t])
    state = a.state_dict()
    assert state["call"] == 5 and sorted(state) == ["age", "call", "est", "hist", "obs_out", "term_out"]
    assert all(v.device.type == "cpu" for k, v in state.items() if k != "call")
    b = channel()
    b.load_state_dict(state)
    for t in range(5, 8):
        oa, ta = a.track(frames[t], frames[t - 1], dones[t])
        ob, tb = b.track(frames[t], frames[t - 1], dones[t])
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    assert torch.equal(a.hist, b.hist) and torch.equal(a.age, b.age) and a.call == b.call == 8
    assert torch.equal(a.est.view(torch.int32), b.est.view(torch.int32)) and not torch.equal(a.est.view(n, 3, 52), frames[7])


def closed_loop(make_inner, robots, predict):
    """450 steps of a perceived env with a fixed action: every step's rows are the references chained on Perceived's
    outputs -- reference_track, then (predict) reference_estimate on its result."""
    from envs.vss import VSS, default_cfg
    from envs.wrappers import Estimated, Perceived, Tracked
    n, D, seed = 33, 2, 4242
    params = T.Params(0.2, 0.5, 0.5)
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 1234
    inner = make_inner(VSS(cfg, DEV, DEV, 0, True, False, False))
    seen = Perceived(inner, D, ALL_ON, seed)
    tracked = Tracked(seen, params)
    env = Estimated(tracked) if predict else tracked
    assert tracked.channel.layout == seen.channel.layout[:4] and tracked.channel.done_stride == robots
    assert tracked.opponent_channel is None and tracked.channel.params == params
    shape = (1, n, robots)
    est, hist, age = np.zeros(shape + (52,), F32), np.zeros((D,) + shape + (6,), F32), np.zeros(shape, np.int32)
    e_hist, e_age = np.zeros((D,) + shape + (6,), F32), np.zeros(shape, np.int32)

    def packed(t):
        return t.detach().cpu().numpy().reshape(n, robots, 52)[None]

    def chained(t, done):
        start = done is None
        want, want_t = T.reference_track(packed(seen.channel.obs_out), None if start else packed(seen.channel.term_out), done,
                                         est, hist, age, t, D, params)
        assert same_bits(packed(tracked.channel.obs_out), want) and (start or same_bits(packed(tracked.channel.term_out), want_t)), t
        filtered = want
        if predict:
            want, want_t = E.reference_estimate(want, want_t, done, e_hist, e_age, t, D)
        return want, want_t, filtered

    got = env.reset()["obs"]
    want, _, _ = chained(0, None)
    assert same_bits(packed(got), want) and same_bits(want, packed(seen.channel.obs_out))
    action = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (robots * n, 2)).astype(F32)).to(DEV)  # fixed, non-zero
    early = late = 0
    moved = 0.0
    for t in range(1, 451):
        obs, reward, dones, info = env.step(action)
        d = dones.cpu().numpy().reshape(n, robots)
        assert (d == d[:, :1]).all()
        want, want_t, filtered = chained(t, d[:, 0])
        assert same_bits(packed(obs["obs"]), want), t
        assert same_bits(packed(info["terminal_observation"]), want_t), t
        assert info["rews"] is inner._rews and info["progress_buffer"] is inner._progress
        assert np.array_equal(tracked.channel.age.cpu().numpy(), age), t
        moved = max(moved, float(np.abs(filtered - packed(seen.channel.obs_out)).max()))
        time_outs = info["time_outs"].cpu().numpy().reshape(n, robots)[:, 0]
        early += int((d[:, 0] != 0).sum() - (time_outs & (d[:, 0] != 0)).sum())
        late += int((time_outs & (d[:, 0] != 0)).sum())
    print("closed loop: episodes ended by a goal", early, "by the time-out", late, "largest change by the filter", moved)
    assert early + late > 0 and tracked.channel.call == 451 and moved > 1e-4
    assert same_bits(tracked.channel.hist.cpu().numpy(), hist) and same_bits(tracked.channel.est.cpu().numpy(), est)
    return early, late


def test_closed_loop_the_tracked_dma_wrapper_is_the_reference_on_perceiveds_outputs():
    from envs.wrappers import DMA
    early, late = closed_loop(DMA, 3, predict=False)
    assert early > 0 and late > 0


def test_closed_loop_estimated_round_tracked_sa_is_the_two_references_chained():
    from envs.wrappers import SingleAgent
    closed_loop(SingleAgent, 1, predict=True)


def test_play_matches_with_perception_tracking_and_estimation_channels_on_blues_rows():
    from envs.vss import VSS, default_cfg
    from play import get_team, play_matches
    n = 64
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 77
    cfg["env"]["maxEpisodeLength"] = 60
    env = VSS(cfg, DEV, DEV, 0, True, False, False)
    env.w_goal, env.w_grad, env.w_move, env.w_energy = 1.0, 0.0, 0.0, 0.0
    ch = PC.PerceptionChannel(n, PC.layout_full_blue(), 2, ALL_ON, 5, DEV, rows=6 * n)
    trk = T.TrackingChannel(n, T.layout_full_blue(), 2, T.Params(0.2, 0.5, 0.5), DEV, rows=6 * n)
    est = E.EstimationChannel(n, E.layout_full_blue(), 2, DEV, rows=6 * n)
    seen = []

    class Blue:
        def __call__(self, act, obs):
            seen.append((obs.data_ptr(), tuple(obs.shape), tuple(obs.stride())))
            act.fill_(0.5)

    score, length = play_matches(env, Blue(), get_team("scripted"), 64, chunk=64, perceive=ch, track=trk, estimate=est)
    assert -1.0 <= score <= 1.0 and 0 < length <= 60
    assert set(seen) == {(est.obs_out.data_ptr(), (n, 3, 52), (312, 52, 1))} and ch.call == trk.call == est.call == len(seen) + 1
    assert not torch.equal(trk.obs_out, ch.obs_out) and not torch.equal(est.obs_out, trk.obs_out)
    seen.clear()
    play_matches(env, Blue(), get_team("scripted"), 64, chunk=64, perceive=ch, track=trk)  # without estimation: the filtered rows
    assert set(seen) == {(trk.obs_out.data_ptr(), (n, 3, 52), (312, 52, 1))}
