"""vss_setplay on the GPU (csrc/vss_setplay.hip): the kernel equals
vss_amd.setplay.reference_setplay bit for bit -- state, rows, chosen and counts after every one of 6 calls, for every
view a wrapper uses and FULL, for done masks that are empty, full, one lane per wave and a lone last field, tables of 1
and 8 plays, shares 0, 0.5 and 1 and `only=` -- writes nothing outside its buffers, its rows are what
vss_compute_observations derives from the state it wrote, and the wrappers' closed loop (goals, time-outs, resets) is
the reference chained on the real step's outputs."""
import ctypes

import numpy as np
import pytest
import torch

from test_perceive_gpu import SENTINEL, Rows, is_sentinel
from test_setplay_cpu import ALL_NAMES, same_bits
from vss_amd import _native as N
from vss_amd import setplay as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CALLS = 6

# name: the views for n fields; "stride-4" has a field stride of 4 and a gapped team stride
VIEWS = {
    "none": lambda n: [],
    "sa": lambda n: [S.view_sa()],
    "dma": lambda n: [S.view_dma()],
    "sa+opp": lambda n: [S.view_sa(), S.view_opponent()],
    "mirror-sa": lambda n: [S.view_mirror(1, n)],
    "mirror-dma": lambda n: [S.view_mirror(3, n)],
    "full": lambda n: [S.view_full()],
    "stride-4": lambda n: [S.View(4, 4 * n + 7, 3, 2, 0)],
}
TABLES = {
    "one": lambda share: S.Table([S.named_play("penalty")], share),
    "five": lambda share: S.Table(S.plays_of_mix("kickoff:1,free_ball:2,penalty_for:1,goal_kick:0.5,breakaway:3"), share),
    "eight": lambda share: S.Table([S.named_play(n)._replace(weight=1.0 + i % 3) for i, n in enumerate(ALL_NAMES[:8])], share),
}


def done_masks(n, g):
    """Per call: None (the start call), no field, every field, one lane per wave, the lone last field, one in ten."""
    one_per_wave = (np.arange(n) % 64 == 5 % max(min(n, 64), 1)).astype(np.int64)
    last = np.zeros(n, np.int64)
    last[-1] = 1
    return [None, np.zeros(n, np.int64), np.ones(n, np.int64), one_per_wave, last, (g.random(n) < 0.1).astype(np.int64)]


def run_case(n, views, table, seed):
    g = np.random.default_rng(seed)
    views = [S.View(*v) for v in views]
    state_b = Rows(58, n)
    view_b = [Rows(v.span(n)) for v in views]
    counts_b, chosen_b, done_b = Rows(8, 1, torch.long), Rows(n, 1, torch.int32), Rows(n, 1, torch.long)
    counts_b.body().zero_()
    state = g.uniform(-0.7, 0.7, (58, n)).astype(F32)
    state_b.body().copy_(torch.from_numpy(state))
    rows, covered = [], []
    for v, b in zip(views, view_b):
        idx = v.row_index(n).reshape(-1)
        r = np.full((v.span(n), 52), 0, F32)
        r.view(np.uint32)[:] = SENTINEL
        r[idx] = g.standard_normal((idx.size, 52)).astype(F32)
        b.body()[torch.from_numpy(idx).to(DEV)] = torch.from_numpy(r[idx]).to(DEV)
        c = np.zeros(v.span(n), bool)
        c[idx] = True
        rows.append(r)
        covered.append(c)
    counts, chosen = np.zeros(8, np.int64), np.zeros(n, np.int32)
    arr = (S.VssSetplayView * 2)()
    for i, (v, b) in enumerate(zip(views, view_b)):
        arr[i] = S.VssSetplayView(b.ptr, *v)
    tab = table.c_table()
    lib, stream = S.load(), N.stream_of(torch.device(DEV))
    staged_total = 0
    for t, done in enumerate(done_masks(n, g)):
        if done is not None:
            done_b.body()[:, 0] = torch.from_numpy(done).to(DEV)
        before = state.copy()
        rc = lib.vss_setplay(stream, n, ctypes.byref(tab), seed, t, None if done is None else done_b.ptr, 1, state_b.ptr,
                             len(views), arr, counts_b.ptr, chosen_b.ptr)
        assert rc == 0
        f = S.reference_setplay(table, seed, t, done, state, list(zip(rows, views)), counts, chosen)
        staged_total += f.size
        got, intact = state_b.host()
        assert intact and same_bits(got, state), (t, "state")
        rest = np.setdiff1d(np.arange(n), f)
        assert same_bits(state[:, rest], before[:, rest])
        for r, c, b in zip(rows, covered, view_b):
            got, intact = b.host()
            assert intact and same_bits(got, r), (t, "rows")
            assert is_sentinel(got[~c]).all()  # rows between the layout's rows are not touched
        got, intact = chosen_b.host()
        assert intact and np.array_equal(got[:, 0], chosen), (t, "chosen")
        assert ((chosen >= 0) == np.isin(np.arange(n), f)).all()
        got, intact = counts_b.host()
        assert intact and np.array_equal(got[:, 0], counts), (t, "counts")
        assert done_b.host()[1]
    assert counts.sum() == staged_total
    return staged_total


@pytest.mark.parametrize("n", [1, 33, 67, 641])
@pytest.mark.parametrize("view", list(VIEWS))
def test_the_kernel_equals_the_reference_for_every_view(n, view):
    staged = run_case(n, VIEWS[view](n), TABLES["five"](0.5), 0xC0FFEE1234 + n)
    assert n < 33 or staged > 0


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("share", [0.0, 0.5, 1.0])
def test_tables_of_one_and_eight_plays_and_every_share(table, share):
    n = 200
    staged = run_case(n, VIEWS["sa+opp"](n), TABLES[table](share), 77)
    want = 2 * n + (n + 63) // 64 + 1  # the start call, every field, one lane per wave, the last field (+ the random mask)
    assert staged == 0 if share == 0.0 else (staged >= want if share == 1.0 else 0 < staged < want + n)


def make_env(n, seed=3):
    from envs.vss import VSS, default_cfg
    cfg = default_cfg(n)
    cfg["env"]["seed"] = seed
    return VSS(cfg=cfg, rl_device=DEV, sim_device=DEV, graphics_device_id=0, headless=True, virtual_screen_capture=False,
               force_render=False)


def test_the_written_rows_are_what_compute_observations_derives_from_the_written_state():
    """The restated compute_obs is pinned to the core's: after every call the FULL rows of every field equal
    vss_compute_observations on the state, bit for bit; and `only=` stages every field with one play."""
    n = 333
    env = make_env(n)
    full = env.compute_observations(torch.empty((n, 2, 3, 52), device=DEV), n_agents=6).clone()
    st = S.Stager(n, TABLES["eight"](0.5), 2026, DEV)
    g = np.random.default_rng(1)
    for t, done in enumerate(done_masks(n, g)):
        if done is None:
            st.start(env.state, [(full, S.view_full())])
        else:
            st.stage(env.state, [(full, S.view_full())], torch.from_numpy(done).to(DEV))
        want = env.compute_observations(torch.empty((n, 2, 3, 52), device=DEV), n_agents=6)
        assert torch.equal(full.view(torch.int32), want.view(torch.int32)), t
    assert st.call == CALLS and int(st.counts.sum()) > n // 2
    for k in (0, 5, 7):
        st.counts.zero_()
        st.start(env.state, [(full, S.view_full())], only=k)
        assert (st.chosen == k).all() and st.counts.tolist() == [n if i == k else 0 for i in range(8)]
        want = env.compute_observations(torch.empty((n, 2, 3, 52), device=DEV), n_agents=6)
        assert torch.equal(full.view(torch.int32), want.view(torch.int32))
        host = env.state.cpu().numpy()
        ref = host.copy()
        S.reference_setplay(st.table.only(k), st.seed, st.call - 1, None, ref)
        assert same_bits(host, ref)


def box_of(play):
    """(anchors (7, 2), r_pos (7, 1)) of a play: an entity lies within r_pos of its anchor on each axis."""
    e = np.asarray(play.entities, np.float64)
    return e[:, 0:2], e[:, 3:4]


def in_its_box(table, k, ball, robots):
    """A staged field lies in play k's box under one of the four mirrorings (robots (6, 2): blue then yellow)."""
    anchors, r = box_of(table.plays[k])
    pos = np.concatenate([ball[None], robots]).astype(np.float64)
    for fx in (False, True):
        for fy in (False, True):
            a = anchors.copy()
            if fy:
                a[:, 1] = -a[:, 1]
            if fx:
                a[:, 0] = -a[:, 0]
                a = a[[0, 4, 5, 6, 1, 2, 3]]
                rr = r[[0, 4, 5, 6, 1, 2, 3]]
            else:
                rr = r
            if (np.abs(pos - a) <= rr + 1e-6).all():
                return True
    return False


class SpyStager(S.Stager):
    """Chains the reference on what the real step left: the state, the rows and the dones before every stage call
    are taken to the host, and the kernel's result is compared with reference_setplay's on them."""

    def attach(self, view_of):
        self.view_of, self.staged, self.kept = view_of, 0, 0
        self.host_counts, self.episodes = np.zeros(8, np.int64), []

    def stage(self, env_state, views, done):
        torch.cuda.synchronize()
        state = env_state.cpu().numpy().copy()
        rows = [r.reshape(-1, 52).cpu().numpy().copy() for r, _ in views]
        d = done.cpu().numpy().copy()
        call = self.call
        super().stage(env_state, views, done)
        before = state.copy()
        chosen = np.zeros(self.n_fields, np.int32)
        f = S.reference_setplay(self.table, self.seed, call, d, state, [(r, v) for r, (_, v) in zip(rows, views)],
                                self.host_counts, chosen)
        assert same_bits(env_state.cpu().numpy(), state)
        for r, (dev_rows, _) in zip(rows, views):
            assert same_bits(dev_rows.reshape(-1, 52).cpu().numpy(), r)
        assert np.array_equal(self.chosen.cpu().numpy(), chosen)
        assert np.array_equal(self.counts.cpu().numpy(), self.host_counts)
        rest = np.setdiff1d(np.arange(self.n_fields), f)
        assert same_bits(state[:, rest], before[:, rest])  # every other episode begins as the step's reset left it
        self.staged += f.size
        self.kept += int(d.sum()) - f.size
        for i in f:
            ball = state[0:2, i]
            robots = np.stack([state[N.CH_RX:N.CH_RX + 6, i], state[N.CH_RY:N.CH_RY + 6, i]], -1)
            assert in_its_box(self.table, chosen[i], ball, robots), (call, i, chosen[i])


@pytest.mark.parametrize("kind", ["sa", "sa-versus", "perceived-dma"])
def test_a_closed_loop_of_450_steps_is_the_reference_chained_on_the_real_step(kind):
    from envs import wrappers as W
    n = 67
    env = make_env(n, seed=11)
    base = W.DMA(env) if kind == "perceived-dma" else W.SingleAgent(env)
    if kind == "sa-versus":  # a team inside the fused step: its rows (opp_obs) are the second view
        from play import get_team
        base.set_opponent(get_team("zero"))
    st = SpyStager(n, TABLES["five"](0.5), S.setplay_seed(11), DEV)
    st.attach(None)
    state0 = env.state.cpu().numpy().copy()
    base.set_setplays(st)
    ref0 = state0.copy()
    f0 = S.reference_setplay(st.table, st.seed, 0, None, ref0)
    st.host_counts += np.bincount(st.chosen.cpu().numpy()[f0], minlength=8)
    assert 0 < f0.size < n and same_bits(env.state.cpu().numpy(), ref0)  # the start call: the first episodes follow the mix
    rows = 3 if kind == "perceived-dma" else 1
    if kind == "sa-versus":
        yellow = env.compute_observations(torch.empty((n, 2, 3, 52), device=DEV), n_agents=6)[:, 1].contiguous()
        assert torch.equal(base._opp_obs.view(torch.int32), yellow.view(torch.int32))
    want = env.compute_observations(torch.empty((n, 2, 3, 52), device=DEV), n_agents=6)[:, 0, :rows].reshape(-1, 52)
    assert torch.equal(base._obs.view(torch.int32), want.contiguous().view(torch.int32))
    w = W.Perceived(base, 2, (0.0, 0.0, 0.0, 0.0), 5) if kind == "perceived-dma" else base
    obs = w.reset()["obs"]
    assert torch.equal(obs.view(torch.int32), base._obs.view(torch.int32))
    gen = torch.Generator(device=DEV).manual_seed(1)
    seen_done = 0
    for _ in range(450):
        action = torch.rand((n * rows, 2), device=DEV, generator=gen) * 2 - 1
        obs_d, _, dones, info = w.step(action)
        d = dones.view(n, rows)[:, 0] != 0
        seen_done += int(d.sum())
        if kind == "perceived-dma" and bool(d.any()):
            # a channel wrapper sees a new episode's first row as it does without set plays: the staged rows themselves
            got, true = obs_d["obs"].view(n, rows, 52)[d], base._obs.view(n, rows, 52)[d]
            assert torch.equal(got.view(torch.int32), true.view(torch.int32))
    assert st.call == 451 and seen_done == st.staged + st.kept and st.staged > 10 and st.kept > 10


def test_binding_refusals_and_a_state_dict_round_trip():
    n = 40
    env = make_env(n)
    st = S.Stager(n, TABLES["five"](1.0), 9, DEV)
    obs = torch.zeros((n, 52), device=DEV)
    done = torch.ones(n, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="state must be"):
        st.start(env.state[:, :-1].contiguous())
    with pytest.raises(ValueError, match="state must be"):
        st.start(env.state.double())
    with pytest.raises(ValueError, match="at most two views"):
        st.start(env.state, [(obs, S.view_sa())] * 3)
    with pytest.raises(ValueError, match="view 0 must be"):
        st.start(env.state, [(obs, S.view_dma())])  # too few rows
    with pytest.raises(ValueError, match="view 0 must be"):
        st.start(env.state, [(obs.cpu(), S.view_sa())])
    for bad in (done[:-1], done.int(), done.cpu(), None):
        with pytest.raises(ValueError, match="done must be"):
            st.stage(env.state, [(obs, S.view_sa())], bad)
    with pytest.raises(N.NativeError, match="invalid argument"):
        st.stage(env.state, [(torch.zeros((n + 8, 52), device=DEV), S.View(1, 0, 2, 1, 0))], done)
    with pytest.raises(ValueError, match="only=9"):
        st.start(env.state, (), only=9)
    with pytest.raises(N.NativeError, match="no CPU path"):
        S.Stager(n, TABLES["five"](1.0), 9, "cpu")
    assert st.call == 0
    st.start(env.state, [(obs, S.view_sa())])
    st.stage(env.state, [(obs, S.view_sa())], done)
    saved = st.state_dict()
    assert sorted(saved) == ["call", "chosen", "counts"] and saved["call"] == 2 and int(saved["counts"].sum()) == 2 * n
    other = S.Stager(n, TABLES["five"](1.0), 9, DEV)
    other.load_state_dict(saved)
    assert other.call == 2 and torch.equal(other.counts, st.counts) and torch.equal(other.chosen, st.chosen)
    a, b = env.state.clone(), env.state.clone()
    st.stage(a, (), done)
    other.stage(b, (), done)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(other.counts, st.counts)
    with pytest.raises(ValueError):
        S.Stager(n + 1, TABLES["five"](1.0), 9, DEV).load_state_dict(saved)
