"""The league's kernels against the single-actor ones, bit for bit: vss_actor_forward_grouped vs
vss_actor_forward, vss_policy_sample_grouped vs vss_policy_sample, vss_match_tally vs an int64 recount."""
import ctypes
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
GUARD = 64  # floats / counters kept past every output


def make_agent(act_dim, seed, logstd):
    torch.manual_seed(seed)
    a = P.Agent(Env(Box(-np.inf, np.inf, (52,)), Box(-1.0, 1.0, (act_dim,)))).to(DEV)
    with torch.no_grad():  # non-trivial last layers and log-std (init has 0.01-scaled actor outputs)
        a.actor_mean[8].weight.mul_(50.0)
        a.actor_logstd.copy_(torch.linspace(logstd, logstd + 0.3, act_dim, device=DEV).view(1, act_dim))
        for m in a.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.1, 0.1)
    return a


@pytest.fixture(scope="module")
def actors():
    """Four packed actors per action width, different weights and log-stds: (packed, logstd) lists."""
    from vss_amd.policy import FusedPolicy
    out = {}
    for n_act in (2, 6):
        pols = [FusedPolicy(make_agent(n_act, 100 + 10 * n_act + q, -1.2 + 0.4 * q), seed=0) for q in range(4)]
        out[n_act] = pols
    torch.cuda.synchronize()
    return out


def table(count, group_rows, packed, logstds):
    g = N.VssActorGroups()
    g.count, g.group_rows = count, group_rows
    for i in range(count):
        g.actor_packed[i] = None if packed is None else packed[i].data_ptr()
        g.logstd[i] = logstds[i].data_ptr()
    return g


def guarded(rows, width):
    buf = torch.full((rows * width + GUARD,), -77.0, device=DEV)
    return buf, buf[:rows * width].view(rows, width)


# (600, 192): the split kernel (<= 4,096 rows), 4 groups, the last of 24 rows with a partial 16-row block;
# (4300, 1088) / (4500, 1152): policy_kernel's 64-row workgroups, 4 groups, a partial last workgroup;
# (64, 64): one group.  The block-to-row-block mapping (vss_policy.hip grouped_block) has a branch of its own
# for one group, for 2..8 groups (3 groups: unequal shares of the 8 block residues) and for more than 8
# (two groups per residue): (5000, 1728) 3 groups, (720, 64) 12 groups on the split kernel, (4200, 320) 14 groups
# on policy_kernel with a partial last workgroup; the four actors are dealt in turn (neighbours differ)
@pytest.mark.parametrize("rows,group_rows,n_act", [(600, 192, 2), (4300, 1088, 6), (4500, 1152, 2), (64, 64, 2),
                                                   (5000, 1728, 2), (720, 64, 2), (4200, 320, 6)])
def test_grouped_forward_equals_the_single_forward(actors, rows, group_rows, n_act):
    lib, stream = N.load(), N.stream_of(torch.device(DEV))
    count = -(-rows // group_rows)
    pols = [actors[n_act][q % 4] for q in range(count)]
    packed = [p._actor for p in pols]
    logstds = [p.agent.actor_logstd.detach().reshape(-1) for p in pols]
    obs = torch.randn(rows, 52, device=DEV, generator=torch.Generator(device=DEV).manual_seed(rows)) * 0.7
    seed, counter = 0x1234567, 9
    abuf, act = guarded(rows, n_act)
    mbuf, mean = guarded(rows, n_act)
    g = table(count, group_rows, packed, logstds)
    N.check(lib.vss_actor_forward_grouped(stream, rows, n_act, obs.data_ptr(), ctypes.byref(g), seed, counter,
                                          act.data_ptr(), mean.data_ptr()), "vss_actor_forward_grouped")
    for q in range(count):
        want_a, want_m = torch.empty((rows, n_act), device=DEV), torch.empty((rows, n_act), device=DEV)
        N.check(lib.vss_actor_forward(stream, rows, n_act, obs.data_ptr(), packed[q].data_ptr(), logstds[q].data_ptr(),
                                      seed, counter, want_a.data_ptr(), want_m.data_ptr()), "vss_actor_forward")
        lo, hi = q * group_rows, min(rows, (q + 1) * group_rows)
        assert torch.equal(act[lo:hi], want_a[lo:hi]), f"group {q} actions"
        assert torch.equal(mean[lo:hi], want_m[lo:hi]), f"group {q} means"
        if q + 1 < count:  # the groups really differ: the next group's rows are not this actor's
            assert not torch.equal(mean[hi:hi + 16], want_m[hi:hi + 16])
    assert (abuf[rows * n_act:] == -77.0).all() and (mbuf[rows * n_act:] == -77.0).all()
    assert torch.isfinite(act).all()
    # one group over all rows: the whole output is vss_actor_forward's
    g1 = table(1, -(-rows // 64) * 64, packed, logstds)
    a1, m1 = torch.empty((rows, n_act), device=DEV), torch.empty((rows, n_act), device=DEV)
    N.check(lib.vss_actor_forward_grouped(stream, rows, n_act, obs.data_ptr(), ctypes.byref(g1), seed, counter,
                                          a1.data_ptr(), m1.data_ptr()), "vss_actor_forward_grouped")
    w1, wm1 = torch.empty((rows, n_act), device=DEV), torch.empty((rows, n_act), device=DEV)
    N.check(lib.vss_actor_forward(stream, rows, n_act, obs.data_ptr(), packed[0].data_ptr(), logstds[0].data_ptr(),
                                  seed, counter, w1.data_ptr(), wm1.data_ptr()), "vss_actor_forward")
    assert torch.equal(a1, w1) and torch.equal(m1, wm1)


@pytest.mark.parametrize("n_act", [2, 6])
def test_grouped_sampling_equals_the_single_sampling(actors, n_act):
    lib, stream = N.load(), N.stream_of(torch.device(DEV))
    rows, group_rows, count = 16400, 4160, 4
    logstds = [p.agent.actor_logstd.detach().reshape(-1) for p in actors[n_act]]
    mean = torch.randn(rows, n_act, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    seed, counter = 99, 3
    buf, act = guarded(rows, n_act)
    g = table(count, group_rows, None, logstds)  # actor_packed is not read: null
    N.check(lib.vss_policy_sample_grouped(stream, rows, n_act, mean.data_ptr(), ctypes.byref(g), seed, counter,
                                          act.data_ptr()), "vss_policy_sample_grouped")
    want = torch.empty((rows, n_act), device=DEV)
    for q in range(count):
        N.check(lib.vss_policy_sample(stream, rows, n_act, mean.data_ptr(), logstds[q].data_ptr(), seed, counter, None,
                                      want.data_ptr(), None, None), "vss_policy_sample")
        lo, hi = q * group_rows, min(rows, (q + 1) * group_rows)
        assert torch.equal(act[lo:hi], want[lo:hi]), f"group {q}"
        if q + 1 < count:
            assert not torch.equal(act[hi:hi + 64], want[hi:hi + 64])
    assert (buf[rows * n_act:] == -77.0).all()
    # equal log-stds: the whole output is vss_policy_sample's
    g = table(count, group_rows, None, [logstds[1]] * count)
    N.check(lib.vss_policy_sample_grouped(stream, rows, n_act, mean.data_ptr(), ctypes.byref(g), seed, counter,
                                          act.data_ptr()), "vss_policy_sample_grouped")
    N.check(lib.vss_policy_sample(stream, rows, n_act, mean.data_ptr(), logstds[1].data_ptr(), seed, counter, None,
                                  want.data_ptr(), None, None), "vss_policy_sample")
    assert torch.equal(act, want)


def tally_inputs(n_fields, rpf, seed):
    """Synthetic step outputs: dones with probability 0.3, goal rewards from {-10, 0, +10} and a few +-tiny
    values, progress in [1, 400]; with 3 rows per field, rows 1-2 carry values that would change every
    counter if they were read."""
    rng = np.random.default_rng(seed)
    rows = n_fields * rpf
    goal = rng.choice(np.array([-10.0, 0.0, 10.0, 1e-30, -1e-30, 1e-6, -1e-6], dtype=np.float32), size=rows,
                      p=[0.25, 0.3, 0.25, 0.05, 0.05, 0.05, 0.05])
    rew = rng.standard_normal((rows, 4)).astype(np.float32)
    rew[:, 0] = goal
    dones = (rng.random(rows) < 0.3).astype(np.int64)
    progress = rng.integers(1, 401, size=rows).astype(np.float32)
    if rpf == 3:
        lead = np.arange(rows) % 3 == 0
        dones[~lead] = 1 - np.repeat(dones[lead], 3)[~lead]  # the opposite of the field's own flag
        rew[~lead, 0] = -np.repeat(rew[lead, 0], 3)[~lead] + 10.0
        progress[~lead] += 1000.0
    return rew, dones, progress


def recount(n_fields, rpf, group_fields, count, rew, dones, progress):
    out = np.zeros((count, 4), dtype=np.int64)
    r = np.arange(n_fields) * rpf
    q = np.arange(n_fields) // group_fields
    d = dones[r] != 0
    np.add.at(out[:, 0], q[d], 1)
    np.add.at(out[:, 1], q[d & (rew[r, 0] > 0)], 1)
    np.add.at(out[:, 2], q[d & (rew[r, 0] < 0)], 1)
    np.add.at(out[:, 3], q[d], progress[r][d].astype(np.int64))
    return out


# 300 fields in 3 groups of 128; groups of 100: group boundaries inside a wave's 64 fields; 70,000 fields:
# several workgroups on one counter
@pytest.mark.parametrize("n_fields,group_fields,count,rpf", [(300, 128, 3, 1), (300, 128, 3, 3), (300, 100, 3, 3),
                                                             (70000, 35072, 2, 1)])
def test_match_tally_equals_the_recount(n_fields, group_fields, count, rpf):
    lib, stream = N.load(), N.stream_of(torch.device(DEV))
    tally = torch.full((count + 2, 4), -5, dtype=torch.long, device=DEV)  # two guard rows
    tally[:count] = 0
    want = np.zeros((count, 4), dtype=np.int64)
    for call in range(2):  # the second call adds to the first
        rew, dones, progress = tally_inputs(n_fields, rpf, 7 + call)
        t = [torch.from_numpy(x).to(DEV) for x in (rew, dones, progress)]
        N.check(lib.vss_match_tally(stream, n_fields, rpf, group_fields, count, t[0].data_ptr(), t[1].data_ptr(),
                                    t[2].data_ptr(), tally.data_ptr()), "vss_match_tally")
        want += recount(n_fields, rpf, group_fields, count, rew, dones, progress)
        got = tally.cpu().numpy()
        np.testing.assert_array_equal(got[:count], want)
        assert (got[count:] == -5).all()
    assert (want[:, 0] > 0).all() and (want[:, 1] > 0).all() and (want[:, 2] > 0).all()
    assert (want[:, 0] > want[:, 1] + want[:, 2]).all()  # draws too
