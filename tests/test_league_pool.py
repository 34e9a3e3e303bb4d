"""OpponentPool: slot arithmetic, one launch over several snapshots, the GEMM-chain path, the match tally
through the real step, end_update's bookkeeping and the snapshots' isolation from the learner."""
import ctypes
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import ppo_continuous_action_isaacgym as P
from envs._gym import Box
from vss_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Env = namedtuple("Env", ["single_observation_space", "single_action_space"])


def make_agent(act_dim, seed, logstd=-0.7):
    torch.manual_seed(seed)
    a = P.Agent(Env(Box(-np.inf, np.inf, (52,)), Box(-1.0, 1.0, (act_dim,)))).to(DEV)
    with torch.no_grad():  # non-trivial last layers and log-std (init has 0.01-scaled actor outputs)
        a.actor_mean[8].weight.mul_(50.0)
        a.actor_logstd.fill_(logstd)
        for m in a.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.1, 0.1)
    return a


def make_vss(n, max_len=400, seed=1234, w_goal=None):
    from envs.vss import VSS, default_cfg
    cfg = default_cfg(n)
    cfg["env"]["maxEpisodeLength"] = max_len
    cfg["env"]["seed"] = seed
    if w_goal is not None:
        cfg["env"]["rew_weights"]["goal"] = w_goal
    return VSS(cfg, DEV, DEV, 0, True, False, False)


def pool_of(agents, kind, n_fields, **kw):
    """A pool holding snapshots of `agents` (versions 0, 1, ...), newest last."""
    from vss_amd.opponent import OpponentPool
    pool = OpponentPool(agents[0], kind, n_fields, **kw)
    for v, a in enumerate(agents[1:], 1):
        pool.add(a, v)
    return pool


def test_slot_arithmetic():
    from vss_amd.opponent import OpponentPool, pool_slots
    assert pool_slots(256, 4, 3) == (64, 4)
    assert pool_slots(200, 4, 3) == (64, 4)  # the last slot: 8 fields
    assert pool_slots(5504, 4, 3) == (1536, 4)  # 16,512 rows: the GEMM chain, whole 256-field blocks
    assert pool_slots(5504, 4, 1) == (1408, 4)  # 5,504 rows (cma): below the chain, 64-field blocks
    assert pool_slots(100, 8, 1) == (64, 2)  # fewer slots than asked for
    assert pool_slots(65536, 16, 3) == (4096, 16)
    with pytest.raises(ValueError):
        pool_slots(256, 17, 3)
    pool = OpponentPool(make_agent(2, 1), "x3", 200, slots=4)
    assert (pool.group_fields, pool.count, pool.group_rows, pool.rows) == (64, 4, 192, 600)
    assert pool.versions == [0, 0, 0, 0] and pool.version == 0
    with pytest.raises(ValueError):
        OpponentPool(make_agent(2, 1), "cma", 256)  # a 6-action team needs a 6-action Agent


def test_call_below_chain_size_plays_each_slot_with_its_snapshot():
    """256 fields, x3, 4 slots holding 3 distinct snapshots: the rows of slot q are what an actor-only
    FusedPolicy of that snapshot's actor draws for the same (seed, counter, row)."""
    from vss_amd.policy import FusedPolicy
    agents = [make_agent(2, 30 + i, logstd=-1.0 + 0.3 * i) for i in range(3)]
    n = 256
    pool = pool_of(agents, "x3", n, slots=4, seed=77)
    S = pool.snapshots
    pool.hold([S[2], S[0], S[1], S[0]])
    assert pool.versions == [2, 0, 1, 0]
    obs = torch.randn(n, 3, 52, device=DEV) * 0.7
    act = torch.zeros((n, 3, 2), device=DEV)
    for call in (1, 2):
        pool(act, obs)
        assert pool.counter == call
        got = act.view(n * 3, 2)
        for q, snap in enumerate(pool.slot_snapshots):
            ref = FusedPolicy(agents[snap.version], seed=77, actor_only=True)
            ref.counter = call - 1
            want = ref.act(obs.view(n * 3, 52))
            lo, hi = q * pool.group_rows, (q + 1) * pool.group_rows
            assert torch.equal(got[lo:hi], want[lo:hi]), f"slot {q} call {call}"
    # a non-contiguous action buffer is written through a copy
    wide = torch.zeros((n, 3, 4), device=DEV)
    pool.counter = 1
    pool(wide[:, :, :2], obs)
    assert torch.equal(wide[:, :, :2], act)


def test_call_at_chain_size():
    """5,504 fields x 3 = 16,512 rows: each slot's means are its snapshot's GEMM chain on the slot's row
    slice, bit for bit (slots 0-1 hold the same snapshot and share one chain call), and the actions are
    vss_policy_sample_grouped of those means."""
    from vss_amd import policy as PM
    agents = [make_agent(2, 40 + i, logstd=-1.0 + 0.3 * i) for i in range(3)]
    n = 5504
    pool = pool_of(agents, "x3", n, slots=4, seed=5)
    assert pool.chain_active() and (pool.group_fields, pool.count) == (1536, 4) and pool.rows >= PM.CHAIN_MIN_ROWS
    S = pool.snapshots
    pool.hold([S[2], S[2], S[0], S[1]])
    obs = torch.randn(n, 3, 52, device=DEV) * 0.7
    rows = obs.view(n * 3, 52)
    mean = pool.means_chain(rows)
    for q, snap in enumerate(pool.slot_snapshots):
        lo, hi = q * pool.group_rows, min(pool.rows, (q + 1) * pool.group_rows)
        ref = PM.FusedPolicy(snap.actor, actor_only=True)
        want = ref._chain(snap.actor.actor_mean, rows[lo:hi])
        assert torch.equal(mean[lo:hi], want), f"slot {q}"
        with torch.no_grad():  # and it is that actor's mean (the chain's rounding, as tests/test_opponent.py)
            torch.testing.assert_close(mean[lo:hi], agents[snap.version].actor_mean(rows[lo:hi]), rtol=2e-5, atol=2e-6)
    act = torch.zeros((n, 3, 2), device=DEV)
    pool(act, obs)
    want = torch.empty((pool.rows, 2), device=DEV)
    N.check(N.load().vss_policy_sample_grouped(N.stream_of(torch.device(DEV)), pool.rows, 2, mean.data_ptr(),
                                               ctypes.byref(pool._groups), pool.seed, pool.counter, want.data_ptr()),
            "vss_policy_sample_grouped")
    assert torch.equal(act.view(-1, 2), want)
    assert not torch.equal(act.view(-1, 2), mean)  # noise was added


def test_one_slot_one_snapshot_equals_the_snapshot_opponent():
    from envs.wrappers import SingleAgent
    from vss_amd.opponent import OpponentPool, SnapshotOpponent
    agent = make_agent(2, 3)
    n = 256
    Wa, Wb = SingleAgent(make_vss(n, max_len=12)), SingleAgent(make_vss(n, max_len=12))
    pool = OpponentPool(agent, "x3", n, slots=1, seed=9)
    assert pool.count == 1
    Wa.set_opponent(pool)
    Wb.set_opponent(SnapshotOpponent(agent, "x3", seed=9))
    gen = torch.Generator(device=DEV).manual_seed(4)
    resets = 0
    for t in range(20):
        a = torch.rand((n, 2), device=DEV, generator=gen) * 2.4 - 1.2
        (oa, ra, da, ia), (ob, rb, db, ib) = Wa.step(a), Wb.step(a)
        assert torch.equal(oa["obs"], ob["obs"]) and torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(ia["terminal_observation"], ib["terminal_observation"]), t
        assert torch.equal(ia["opponent_obs"], ib["opponent_obs"]) and torch.equal(Wa.env.state, Wb.env.state), t
        resets += int(da.sum())
    assert resets > 0
    assert int(pool.tally[0, 0]) == resets


@pytest.mark.parametrize("mode", ["sa", "dma"])
def test_tallies_through_the_real_step(mode):
    from envs.wrappers import DMA, SingleAgent
    n, rpf = 256, (3 if mode == "dma" else 1)
    W = (DMA if mode == "dma" else SingleAgent)(make_vss(n, max_len=20))
    pool = pool_of([make_agent(2, 50), make_agent(2, 51)], "x3", n, slots=4, seed=3)
    W.set_opponent(pool)
    learner = make_agent(2, 52)
    want = np.zeros((4, 4), dtype=np.int64)
    gen = torch.Generator(device=DEV).manual_seed(8)
    obs = W.reset()["obs"]
    for t in range(60):
        with torch.no_grad():
            a = learner.actor_mean(obs) + 0.3 * torch.randn((n * rpf, 2), device=DEV, generator=gen)
        o, _, dones, infos = W.step(a)
        obs = o["obs"]
        d = dones.cpu().numpy()[::rpf] != 0
        goal = infos["rews"].cpu().numpy()[::rpf, 0]
        prog = infos["progress_buffer"].cpu().numpy()[::rpf].astype(np.int64)
        q = np.arange(n) // pool.group_fields
        np.add.at(want[:, 0], q[d], 1)
        np.add.at(want[:, 1], q[d & (goal > 0)], 1)
        np.add.at(want[:, 2], q[d & (goal < 0)], 1)
        np.add.at(want[:, 3], q[d], prog[d])
    np.testing.assert_array_equal(pool.tally.cpu().numpy(), want)
    assert (want[:, 0] >= 64 * 2).all()  # 64 fields per slot, three time-outs each at the latest


def test_end_update_bookkeeping():
    from vss_amd.opponent import OpponentPool
    agents = [make_agent(2, 60 + i) for i in range(3)]
    pool = pool_of(agents, "x3", 256, slots=4, capacity=8, latest=0.5, seed=11)
    S = list(pool.snapshots)
    pool.hold([S[2], S[2], S[0], S[1]])
    pool.tally.copy_(torch.tensor([[10, 4, 2, 100], [6, 0, 6, 60], [5, 5, 0, 50], [0, 0, 0, 0]]))
    out = pool.end_update(agents[2], update=3, every=0)  # every = 0: no new snapshot
    assert S[2].totals == [16, 4, 8, 160] and S[0].totals == [5, 5, 0, 50] and S[1].totals == [0, 0, 0, 0]
    assert int(pool.tally.abs().sum()) == 0
    assert out["winrate"][:3] == [(4 + 0.5 * 4) / 10, 0.0, 1.0] and math.isnan(out["winrate"][3])
    assert len(pool.snapshots) == 3 and out["versions"] == pool.versions and len(out["versions"]) == 4
    assert out["versions"][:2] == [2, 2]  # max(1, round(0.5 * 4)) slots hold the newest
    assert all(v in (1, 2) for v in out["versions"][2:])  # version 0 was always beaten: weight 0
    out = pool.end_update(agents[0], update=4, every=2)
    assert pool.version == 4 and len(pool.snapshots) == 4 and out["versions"][:2] == [4, 4]
    out = pool.end_update(agents[0], update=5, every=2)  # 5 % 2 != 0
    assert pool.version == 4 and len(pool.snapshots) == 4
    one = OpponentPool(agents[0], "x3", 256, slots=4, latest=0.0)
    assert one.versions[0] == 0 and max(1, round(0.0 * 4)) == 1  # at least one slot plays the newest


def test_a_full_pool_drops_its_oldest_snapshot():
    agents = [make_agent(2, 70 + i) for i in range(3)]
    pool = pool_of(agents[:1], "x3", 256, slots=4, capacity=2)
    pool.add(agents[1], 1)
    assert [s.version for s in pool.snapshots] == [0, 1]
    pool.add(agents[2], 2)  # the third add (the constructor's was the first) drops version 0
    assert [s.version for s in pool.snapshots] == [1, 2]
    assert all(v in (1, 2) for v in pool.assign())


def test_equal_seeds_and_totals_give_equal_assignments():
    agents = [make_agent(2, 80 + i) for i in range(4)]
    totals = [[20, 2, 15, 1], [20, 10, 5, 1], [0, 0, 0, 0], [9, 3, 3, 1]]
    seen = []
    for seed in (21, 21, 22):
        pool = pool_of(agents, "x3", 1024, slots=16, latest=0.25, seed=seed)
        assert pool.count == 16
        for s, t in zip(pool.snapshots, totals):
            s.totals = list(t)
        seen.append([pool.assign() for _ in range(4)])
        assert all(v[:4] == [3, 3, 3, 3] for v in seen[-1])
    assert seen[0] == seen[1] and seen[0] != seen[2]


def test_a_pool_needs_a_positive_goal_weight():
    from envs.wrappers import SingleAgent
    from vss_amd.opponent import OpponentPool
    agent = make_agent(2, 5)
    W = SingleAgent(make_vss(64, w_goal=0.0))
    with pytest.raises(ValueError, match="w_goal"):
        W.set_opponent(OpponentPool(agent, "x3", 64, slots=1))
    assert W._opponent is None
    with pytest.raises(ValueError, match="fields"):
        SingleAgent(make_vss(64)).set_opponent(OpponentPool(agent, "x3", 128, slots=1))


@pytest.mark.parametrize("kind,act_dim", [("x3", 2), ("cma", 6)])
def test_snapshots_are_isolated_from_the_learner(kind, act_dim):
    from vss_amd.opponent import OpponentPool
    agent = make_agent(act_dim, 90)
    n = 128
    pool = OpponentPool(agent, kind, n, slots=2, seed=13)
    with torch.no_grad():
        for p in agent.parameters():
            p.add_(0.05 * torch.randn_like(p))
    pool.add(agent, 1)
    pool.hold([pool.snapshots[0], pool.snapshots[1]])
    obs = torch.randn(n, 3, 52, device=DEV) * 0.7

    def play():
        pool.counter = 0
        act = torch.zeros((n, 3, 2), device=DEV)
        pool(act, obs)
        return act

    a0 = play()
    with torch.no_grad():  # the learner moves on in place: neither snapshot follows
        for p in agent.parameters():
            p.add_(0.05 * torch.randn_like(p))
    assert torch.equal(play(), a0)
    pool.add(agent, 2)  # a further snapshot does not disturb the slots either, until they are dealt again
    assert torch.equal(play(), a0)
    pool.hold([pool.snapshots[2], pool.snapshots[2]])
    assert not torch.equal(play(), a0)
