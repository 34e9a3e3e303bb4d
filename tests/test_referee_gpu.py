"""vss_referee on the GPU (csrc/vss_referee.hip): the kernel equals
vss_amd.referee.reference_referee bit for bit -- state, dof velocities, rows, counters, verdict and counts -- for every
view a wrapper uses and FULL, for a lone lane, a wave's tail, a wave that leaves early, a second workgroup and a tail
behind three, with and without a done mask; writes nothing outside its buffers and nothing of a field it does not
whistle; its rows are what vss_compute_observations derives from the state and dof velocities it wrote; known answers
through the real step; and the wrappers' closed loop is the reference chained on the real step's outputs."""
import ctypes

import numpy as np
import pytest
import torch

from test_perceive_gpu import SENTINEL, Rows, is_sentinel
from test_referee_cpu import ON, scene
from test_setplay_cpu import same_bits
from test_setplay_gpu import make_env
from vss_amd import _native as N
from vss_amd import referee as R
from vss_amd import setplay as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

VIEWS = {
    "sa": lambda n: [R.view_sa()],
    "dma": lambda n: [R.view_dma()],
    "opponent": lambda n: [R.view_opponent()],
    "mirror-sa": lambda n: [R.view_mirror(1, n)],
    "mirror-dma": lambda n: [R.view_mirror(3, n)],
    "full": lambda n: [R.view_full()],
    "sa+opp": lambda n: [R.view_sa(), R.view_opponent()],
}


def build_inputs(n, g, quiet_from=None):
    """(state, dof_vel, counters, the fields built to be whistled): random states; about a tenth of the fields is a
    scene of test_referee_cpu with its counter past the threshold, the first eight of them one per code; the fields
    from `quiet_from` on can not be whistled (the ball fast at the centre, counters 0)."""
    m = n if quiet_from is None else quiet_from
    state = g.uniform(-0.7, 0.7, (58, n)).astype(F32)
    dof = g.uniform(-1, 1, (n, 12)).astype(F32)
    cnt = g.integers(0, 3, (n, 4)).astype(np.int32)
    picked = np.nonzero(g.random(m) < 0.1)[0]
    lead = g.permutation(m)[:8]
    picked = np.concatenate([lead, np.setdiff1d(picked, lead)])
    codes = np.concatenate([np.arange(len(lead)) if len(lead) == 8 else g.integers(0, 8, len(lead)),
                            g.integers(0, 8, len(picked) - len(lead))])
    for f, c in zip(picked, codes):
        state[:, f] = scene(int(c))[:, 0]
        cnt[f] = (9, 9, 9, 0)
    if quiet_from is not None:
        state[0:4, quiet_from:] = np.array([0.0, 0.0, 1.0, 0.0], F32)[:, None]
        cnt[quiet_from:] = 0
    return state, dof, cnt, picked, codes


def run_case(n, views, seed, quiet_from=None, done_on_picked=False, calls=2, prm=ON):
    g = np.random.default_rng(seed)
    views = [R.View(*v) for v in views]
    table = R.RefTable()
    state_b, dof_b, cnt_b = Rows(58, n), Rows(n, 12), Rows(n, 4, torch.int32)
    view_b = [Rows(v.span(n)) for v in views]
    counts_b, verdict_b, done_b = Rows(8, 1, torch.long), Rows(n, 1, torch.int32), Rows(n, 1, torch.long)
    counts_b.body().zero_()
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
    counts, verdict = np.zeros(8, np.int64), np.zeros(n, np.int32)
    arr = (R.VssRefereeView * 2)()
    for i, (v, b) in enumerate(zip(views, view_b)):
        arr[i] = R.VssRefereeView(b.ptr, *v)
    tab, cprm = table.c_table(), prm.c_params()
    lib, stream = R.load(), N.stream_of(torch.device(DEV))
    whistled, seen = 0, set()
    for t in range(calls):
        state, dof, cnt, picked, codes = build_inputs(n, g, quiet_from)
        done = None
        if done_on_picked:      # every field built to be whistled is done, and a tenth of the others
            done = (g.random(n) < 0.1).astype(np.int64)
            done[picked] = 1
        elif t % 2 == 1:        # the odd calls: a tenth of the fields is done, some of the picked among them
            done = (g.random(n) < 0.1).astype(np.int64)
        state_b.body().copy_(torch.from_numpy(state))
        dof_b.body().copy_(torch.from_numpy(dof))
        cnt_b.body().copy_(torch.from_numpy(cnt))
        if done is not None:
            done_b.body()[:, 0] = torch.from_numpy(done).to(DEV)
        before, dof_before, rows_before = state.copy(), dof.copy(), [r.copy() for r in rows]
        rc = lib.vss_referee(stream, n, ctypes.byref(tab), ctypes.byref(cprm), seed, t, None if done is None else done_b.ptr, 1,
                             state_b.ptr, dof_b.ptr, cnt_b.ptr, len(views), arr, counts_b.ptr, verdict_b.ptr)
        assert rc == 0
        f = R.reference_referee(table, prm, seed, t, done, state, dof.reshape(n, 2, 3, 2), cnt, list(zip(rows, views)), counts,
                                verdict)
        whistled += f.size
        seen |= set(verdict[f].tolist())
        if done is not None:
            assert not np.isin(f, np.nonzero(done)[0]).any() and (cnt[done != 0] == 0).all()
        if done_on_picked:
            assert not np.isin(picked, f).any()
        elif done is None and prm.any():
            assert np.isin(picked, f).all() and np.array_equal(verdict[picked], codes)
        if quiet_from is not None:
            assert f.size > 0 and f.max() < quiet_from and (verdict[quiet_from:] == -1).all()
        got, intact = state_b.host()
        assert intact and same_bits(got, state), (t, "state")
        rest = np.setdiff1d(np.arange(n), f)
        assert same_bits(got[:, rest], before[:, rest])       # what is not whistled is byte-equal to before
        got, intact = dof_b.host()
        assert intact and same_bits(got, dof), (t, "dof_vel")
        assert same_bits(got[rest], dof_before[rest]) and same_bits(got[f], np.zeros((f.size, 12), F32))
        for r, r0, c, v, b in zip(rows, rows_before, covered, views, view_b):
            got, intact = b.host()
            assert intact and same_bits(got, r), (t, "rows")
            assert is_sentinel(got[~c]).all()                 # rows between the layout's rows are not touched
            keep = v.row_index(n)[:, rest].reshape(-1)
            assert same_bits(got[keep], r0[keep])
        got, intact = cnt_b.host()
        assert intact and np.array_equal(got, cnt), (t, "counters")
        got, intact = verdict_b.host()
        assert intact and np.array_equal(got[:, 0], verdict), (t, "verdict")
        got, intact = counts_b.host()
        assert intact and np.array_equal(got[:, 0], counts), (t, "counts")
        assert done_b.host()[1]
    assert counts.sum() == whistled
    return whistled, seen


@pytest.mark.parametrize("n", [1, 63, 65, 257, 641])
@pytest.mark.parametrize("view", list(VIEWS))
def test_the_kernel_equals_the_reference_for_every_view(n, view):
    """A lone lane, a wave's tail, a second wave that leaves early (n = 65: field 64 can not be whistled, fields of
    wave 0 are), a second workgroup, three workgroups and a tail."""
    whistled, seen = run_case(n, VIEWS[view](n), 0xBADCA11 + n, quiet_from=64 if n == 65 else None)
    assert whistled >= min(n, 8) and (n < 8 or seen == set(range(8)))


@pytest.mark.parametrize("n", [65, 257])
def test_done_fields_that_would_be_whistled_are_left_alone(n):
    whistled, _ = run_case(n, VIEWS["sa+opp"](n), 99 + n, done_on_picked=True)
    assert whistled < n // 8


def test_with_both_thresholds_zero_nothing_is_ever_written():
    whistled, _ = run_case(257, VIEWS["full"](257), 5, prm=R.Params.of())
    assert whistled == 0


def put_state(env, state):
    env.state.copy_(torch.from_numpy(np.ascontiguousarray(state, dtype=F32)).to(DEV))


def full_rows(env):
    return env.compute_observations(torch.empty((env.num_fields, 2, 3, 52), device=DEV), n_agents=6)


def test_the_written_rows_are_what_compute_observations_derives_from_the_written_state_and_dof_vel():
    """The restated compute_obs is pinned to the core's: after a call the FULL rows of every field equal
    vss_compute_observations on the state and dof_velocity_buf, bit for bit."""
    n = 333
    env = make_env(n)
    g = np.random.default_rng(2)
    state, dof, cnt, picked, codes = build_inputs(n, g)
    put_state(env, state)
    env.dof_velocity_buf.copy_(torch.from_numpy(dof.reshape(n, 2, 3, 2)).to(DEV))
    full = full_rows(env).clone()
    ref = R.Referee(n, R.RefTable(), ON, 2026, DEV)
    ref.counters.copy_(torch.from_numpy(cnt).to(DEV))
    ref.call(env.state, env.dof_velocity_buf, [(full, R.view_full())], None)
    assert torch.equal(full.view(torch.int32), full_rows(env).view(torch.int32))
    v = ref.verdict.cpu().numpy()
    assert np.array_equal(v[picked], codes) and ref.counts.tolist() == np.bincount(v[v >= 0], minlength=8).tolist()
    assert (env.dof_velocity_buf.view(n, 12)[torch.from_numpy(picked).to(DEV)] == 0).all() and ref.call_index == 1


def test_known_answers_through_the_real_step():
    """Zero actions for all twelve wheels, the FULL view.  Fields 0..3: the ball at rest at (+-0.30, +-0.20), the robots
    parked far away: free balls 0..3 after exactly 3 steps, not after 2.  Field 4: two blue robots parked in blue's
    area, the ball at rest in it: code 5 after 2 steps, the role-swapped penalty.  Field 5: the ball at rest at the
    centre with its counter switched off by a done flag every step: never whistled."""
    n = 6
    env = make_env(n)
    state = np.concatenate([scene(0), scene(1), scene(2), scene(3), scene(5), scene(0)], axis=1)
    state[2, 4] = 0.0   # at rest in the area
    state[0:2, 5] = 0.0
    put_state(env, state)
    env.dof_velocity_buf.zero_()
    ref = R.Referee(n, R.RefTable(), ON, 7, DEV)
    off = R.Referee(n, R.RefTable(), R.Params.of(), 7, DEV)
    zero = torch.zeros((n, 2, 3, 2), device=DEV)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    done[5] = 1
    verdicts = []
    for t in range(3):
        obs = env.step(zero)[0]["obs"]
        assert not bool(env.reset_buf.any())
        before = (env.state.clone(), env.dof_velocity_buf.clone(), obs.clone())
        off.call(env.state, env.dof_velocity_buf, [(obs.view(-1, 52), R.view_full())], done)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                   for a, b in zip(before, (env.state, env.dof_velocity_buf, obs)))
        host, dof = env.state.cpu().numpy().copy(), env.dof_velocity_buf.cpu().numpy().copy()
        cnt, rows = ref.counters.cpu().numpy().copy(), obs.view(-1, 52).cpu().numpy().copy()
        ref.call(env.state, env.dof_velocity_buf, [(obs.view(-1, 52), R.view_full())], done)
        R.reference_referee(ref.table, ref.params, ref.seed, t, done.cpu().numpy(), host, dof, cnt, [(rows, R.view_full())])
        assert same_bits(env.state.cpu().numpy(), host) and same_bits(obs.view(-1, 52).cpu().numpy(), rows)
        assert np.array_equal(ref.counters.cpu().numpy(), cnt)
        assert torch.equal(obs.view(torch.int32), full_rows(env).view(torch.int32))
        verdicts.append(ref.verdict.tolist())
    assert verdicts == [[-1] * 6, [-1, -1, -1, -1, 5, -1], [0, 1, 2, 3, -1, -1]]
    assert off.counts.sum() == 0 and (off.verdict == -1).all() and off.counters[:4, 0].tolist() == [3] * 4
    assert ref.counts.tolist() == [1, 1, 1, 1, 0, 1, 0, 0] and ref.counters[:, 3].tolist() == [1, 1, 1, 1, 1, 0]
    st = env.state.cpu().numpy()
    assert same_bits(st[0:2, :4], [[0.375, 0.375, -0.375, -0.375], [0.4, -0.4, 0.4, -0.4]])  # the four marks
    # field 4 after its restart and one more step of rest: yellow takes the penalty towards -x; blue 2 keeps blue's goal
    assert st[0, 4] == F32(-0.375) and st[1, 4] == 0.0
    assert abs(st[N.CH_RX + 2, 4] + 0.68) <= 0.0201 and abs(st[N.CH_RX + 3, 4] + 0.28) <= 0.0101
    assert abs(st[N.CH_RX + 5, 4] - 0.10) <= 0.0301 and abs(st[N.CH_RY + 5, 4] + 0.30) <= 0.0301


class SpyReferee(R.Referee):
    """Chains the reference on what the real step (and the stager) left: the state, the dof velocities, the rows, the
    counters and the dones before every call are taken to the host, and the kernel's result is compared with
    reference_referee's on them."""

    def attach(self, stager=None):
        self.stager, self.host_counts, self.on_done = stager, np.zeros(8, np.int64), 0

    def call(self, env_state, dof_vel, views, done):
        torch.cuda.synchronize()
        state, dof = env_state.cpu().numpy().copy(), dof_vel.cpu().numpy().copy()
        rows = [r.reshape(-1, 52).cpu().numpy().copy() for r, _ in views]
        d, cnt, t = done.cpu().numpy().copy(), self.counters.cpu().numpy().copy(), self.call_index
        if self.stager is not None:  # the order: the step, the set plays, then the referee
            assert self.stager.call == t + 2
        super().call(env_state, dof_vel, views, done)
        before, verdict = state.copy(), np.zeros(self.n_fields, np.int32)
        f = R.reference_referee(self.table, self.params, self.seed, t, d, state, dof, cnt,
                                [(r, v) for r, (_, v) in zip(rows, views)], self.host_counts, verdict)
        assert same_bits(env_state.cpu().numpy(), state) and same_bits(dof_vel.cpu().numpy(), dof)
        for r, (dev_rows, _) in zip(rows, views):
            assert same_bits(dev_rows.reshape(-1, 52).cpu().numpy(), r)
        assert np.array_equal(self.counters.cpu().numpy(), cnt) and np.array_equal(self.verdict.cpu().numpy(), verdict)
        assert np.array_equal(self.counts.cpu().numpy(), self.host_counts)
        rest = np.setdiff1d(np.arange(self.n_fields), f)
        assert same_bits(state[:, rest], before[:, rest]) and not np.isin(f, np.nonzero(d)[0]).any()
        self.on_done += int(d.sum())


# a goal area 0.35 m deep and 1.30 m wide, so that two of a team's three robots stand in one with the ball often enough
LOOP = R.Params.of(stall_steps=3, area_steps=2, area_depth=0.35, area_width=1.30)


@pytest.mark.parametrize("kind", ["sa", "sa-versus", "mirror", "sa+setplays"])
def test_a_closed_loop_of_300_steps_is_the_reference_chained_on_the_real_step(kind):
    """Seed and thresholds were chosen on the CPU: the C oracle's SA step (seed 11, 257 fields, these actions) chained
    with reference_referee under LOOP produced, in 300 steps, 18,684 free balls (4623, 3507, 5248, 5306 per quadrant
    -- a placed ball rests until it is hit, so a mark is called again every third step), 11 and 21 penalties and 18
    and 17 goal kicks, beside 28 finished episodes."""
    from envs import wrappers as W
    n = 257
    env = make_env(n, seed=11)
    base = W.MirrorSingleAgent(env) if kind == "mirror" else W.SingleAgent(env)
    if kind == "sa-versus":  # a team inside the fused step: its rows (opp_obs) are the second view
        from play import get_team
        base.set_opponent(get_team("zero"))
    stager = None
    if kind == "sa+setplays":
        stager = S.Stager(n, S.Table(S.plays_of_mix("kickoff:1,free_ball:2,penalty_for:1"), 0.5), S.setplay_seed(11), DEV)
        base.set_setplays(stager)
    ref = SpyReferee(n, R.RefTable(), LOOP, R.referee_seed(11), DEV)
    ref.attach(stager)
    base.set_referee(ref)
    base.reset()
    g = np.random.default_rng(1)
    rows = 2 if kind == "mirror" else 1
    for _ in range(300):
        action = torch.from_numpy(g.uniform(-1, 1, (n * rows, 2)).astype(F32)).to(DEV)
        _, _, _, info = base.step(action)
        assert info["referee"] is ref.verdict
    c = ref.host_counts
    print(kind, "calls per code", c.tolist(), "done fields", ref.on_done)
    assert ref.call_index == 300 and c[:4].sum() >= 1 and c[4:6].sum() >= 1 and c[6:8].sum() >= 1 and ref.on_done >= 1
    if stager is not None:
        assert stager.call == 301 and int(stager.counts.sum()) > 0
    base.set_referee(None)
    _, _, _, info = base.step(action)
    assert "referee" not in info and ref.call_index == 300


def test_binding_refusals_and_a_state_dict_round_trip():
    n = 40
    env = make_env(n)
    ref = R.Referee(n, R.RefTable(), ON, 9, DEV)
    obs = torch.zeros((n, 52), device=DEV)
    done = torch.zeros(n, dtype=torch.long, device=DEV)
    dof = env.dof_velocity_buf
    with pytest.raises(ValueError, match="state must be"):
        ref.call(env.state[:, :-1].contiguous(), dof, (), done)
    with pytest.raises(ValueError, match="state must be"):
        ref.call(env.state.double(), dof, (), done)
    for bad in (dof[:-1], dof.double(), dof.cpu()):
        with pytest.raises(ValueError, match="dof_vel must be"):
            ref.call(env.state, bad, (), done)
    with pytest.raises(ValueError, match="at most two views"):
        ref.call(env.state, dof, [(obs, R.view_sa())] * 3, done)
    with pytest.raises(ValueError, match="view 0 must be"):
        ref.call(env.state, dof, [(obs, R.view_dma())], done)  # too few rows
    with pytest.raises(ValueError, match="view 0 must be"):
        ref.call(env.state, dof, [(obs.cpu(), R.view_sa())], done)
    for bad in (done[:-1], done.int(), done.cpu()):
        with pytest.raises(ValueError, match="done must be"):
            ref.call(env.state, dof, [(obs, R.view_sa())], bad)
    with pytest.raises(N.NativeError, match="invalid argument"):
        ref.call(env.state, dof, [(torch.zeros((n + 8, 52), device=DEV), R.View(1, 0, 2, 1, 0))], done)
    with pytest.raises(N.NativeError, match="no CPU path"):
        R.Referee(n, R.RefTable(), ON, 9, "cpu")
    with pytest.raises(ValueError, match="whistled again"):
        R.Referee(n, R.RefTable(), R.Params.of(stall_steps=1, area_depth=0.40, area_width=1.0), 9, DEV)
    assert ref.call_index == 0
    put_state(env, np.concatenate([scene(c, 5) for c in range(8)], axis=1))
    ref.counters[:, :3] = 1
    ref.call(env.state, dof, [(obs, R.view_sa())], None)       # done None: no field is done
    ref.call(env.state, dof, [(obs, R.view_sa())], done)
    saved = ref.state_dict()
    assert sorted(saved) == ["call_index", "counters", "counts", "verdict"] and saved["call_index"] == 2
    assert int(saved["counts"].sum()) > 0 and saved["counters"].shape == (n, 4)
    other = R.Referee(n, R.RefTable(), ON, 9, DEV)
    other.load_state_dict(saved)
    assert other.call_index == 2 and all(torch.equal(getattr(other, k), getattr(ref, k)) for k in ("counters", "counts", "verdict"))
    assert other.record() == {k: 0 for k in other.record()} and sum(ref.record().values()) == int(ref.counts.sum())
    a, b, da, db = env.state.clone(), env.state.clone(), dof.clone(), dof.clone()
    ref.call(a, da, (), done)
    other.call(b, db, (), done)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(other.counts, ref.counts)
    assert torch.equal(other.counters, ref.counters) and torch.equal(other.verdict, ref.verdict)
    with pytest.raises(ValueError):
        R.Referee(n + 1, R.RefTable(), ON, 9, DEV).load_state_dict(saved)
