"""The rollout policy (csrc/vss_policy.hip, vss_amd/policy.py) against a host specification.

What every training run, opponent and league samples its actions from is pinned here the way the update side is:
  1. the Philox stream and its keying as plain numpy (tests/policy_draws.py), checked on the CPU against the
     Random123 known answers and two edge draws found by a host search;
  2. the draws of every entry point against that specification, row by row and dim by dim;
  3. log-prob and entropy against torch's Normal formulas in fp64, with a per-dim log-std;
  4. one row, one result: every kernel regime (split, both, separate launches, actor-only, critic-only, masked)
     gives a row the same bits, wherever the row lies in the batch;
  5. the write extents of the fused entries.
Tolerances are stated where they are used, in units of 2^-24 (half an fp32 ulp of a value in [1, 2))."""
import copy
import ctypes
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import policy_draws as PD
from test_write_extents import GUARD, SENTINEL, Guarded
from vss_amd.perceive import _philox

gpu = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)  # 0.91893853320467274
EDGE_SEED = 0x9E3779B97F4A7C15
SEED_COUNTERS = [(0, 1), (0xFFFFFFFF00000001, 0xFFFFFFFF), (0xFFFFFFFF00000001, 0x100000000), (2 ** 63 + 5, 2 ** 40 + 3)]


# ---- 1. the host specification (CPU) -----------------------------------------------------------------------------
KNOWN_ANSWERS = [  # Random123 kat_vectors, philox4x32 10: key, counter, output
    ((0, 0), (0, 0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 2, (0xFFFFFFFF,) * 4, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("key,ctr,want", KNOWN_ANSWERS)
def test_philox_known_answers(key, ctr, want):
    """The ten rounds, and the keying: policy_words reaches the same words when (seed, counter, row, pair) are
    chosen so that its key and counter words are the vector's."""
    got = _philox(*(np.array([k], np.uint32) for k in key), *(np.array([c], np.uint32) for c in ctr))
    assert tuple(int(w[0]) for w in got) == want
    seed = key[0] | (key[1] << 32)
    counter = ctr[1] | ((ctr[2] ^ PD.POL) << 32)
    got = PD.policy_words(seed, counter, [ctr[0]], ctr[3])
    assert tuple(int(w[0]) for w in got) == want


def test_every_key_and_counter_word_matters():
    rows = np.arange(64)
    base = np.stack(PD.policy_words(5, 7, rows, 0))
    changed = {
        "seed lo": PD.policy_words(6, 7, rows, 0),
        "seed hi": PD.policy_words(5 + (1 << 32), 7, rows, 0),
        "counter lo": PD.policy_words(5, 8, rows, 0),
        "counter hi": PD.policy_words(5, 7 + (1 << 32), rows, 0),
        "row": PD.policy_words(5, 7, rows + 64, 0),
        "pair": PD.policy_words(5, 7, rows, 2),
    }
    for name, words in changed.items():
        # four fresh 32-bit words per row: none of the 256 survives (a chance match has probability 2^-24)
        assert (np.stack(words) != base).all(), name
    # the rows of one call are distinct draws, and so are the pairs of one row
    z = PD.reference_normals(5, 7, np.arange(4096), 6)
    assert len(np.unique(z)) == z.size
    # the counter's high word is XORed with "POL": counter hi = "POL" is the all-zero counter word
    assert [int(w[0]) for w in PD.policy_words(0, PD.POL << 32, [0], 0)] == list(KNOWN_ANSWERS[0][2])


def test_reference_normals_are_unit_normals_per_dim():
    """The specification itself: every action dim is N(0, 1) and the dims and neighbouring rows are uncorrelated
    (200,000 draws: a moment's standard error is below 0.006, the bounds are five of them)."""
    z = PD.reference_normals(11, 3, np.arange(200_000), 6)
    assert np.abs(z.mean(axis=0)).max() < 0.012 and np.abs(z.std(axis=0) - 1.0).max() < 0.01
    assert np.abs((z ** 4).mean(axis=0) / 3.0 - 1.0).max() < 0.03
    c = np.corrcoef(z, rowvar=False)
    assert np.abs(c - np.eye(6)).max() < 0.012
    assert abs(np.corrcoef(z[:-1, 0], z[1:, 0])[0, 1]) < 0.012


def test_edge_draws_of_the_stream():
    """u1's two ends, found by a host search of the stream with seed 0x9E3779B97F4A7C15, pair 0: the largest radius
    (u1 = 2^-24, never 0) and radius 0 (u1 = 1)."""
    w = PD.policy_words(EDGE_SEED, 84, [30994], 0)
    assert int(w[0][0]) == 0x000000F3
    z, rad = PD.reference_pairs(EDGE_SEED, 84, [30994], 2)
    assert rad[0, 0] == math.sqrt(-2.0 * math.log(2.0 ** -24)) and 5.76 < rad[0, 0] < 5.77
    assert np.isfinite(z).all() and abs(math.hypot(*z[0]) - rad[0, 0]) < 1e-12
    w = PD.policy_words(EDGE_SEED, 178, [49414], 0)
    assert int(w[0][0]) == 0xFFFFFF5E
    z, rad = PD.reference_pairs(EDGE_SEED, 178, [49414], 2)
    assert rad[0, 0] == 0.0 and (z == 0.0).all()


# ---- GPU plumbing ----------------------------------------------------------------------------------------------
Env = namedtuple("Env", ["single_observation_space", "single_action_space"])


def native():
    from vss_amd import _native as N
    return N, N.load(), N.stream_of(torch.device(DEV))


def make_agent(act_dim, seed, logstd):
    """tests/test_league_kernels.py make_agent: non-trivial last layers and a per-dim log-std."""
    import ppo_continuous_action_isaacgym as P
    from envs._gym import Box
    torch.manual_seed(seed)
    a = P.Agent(Env(Box(-np.inf, np.inf, (52,)), Box(-1.0, 1.0, (act_dim,)))).to(DEV)
    with torch.no_grad():
        a.actor_mean[8].weight.mul_(50.0)
        a.actor_logstd.copy_(torch.linspace(logstd, logstd + 0.3, act_dim, device=DEV).view(1, act_dim))
        for m in a.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.1, 0.1)
    return a


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def sample(rows, n_act, mean, logstd, seed, counter, action_in=None):
    """vss_policy_sample: (action, logprob, entropy)."""
    N, lib, st = native()
    a, lp, ent = nan(rows, n_act), nan(rows), nan(rows)
    N.check(lib.vss_policy_sample(st, rows, n_act, mean.data_ptr(), logstd.data_ptr(), seed, counter, N.ptr(action_in),
                                  a.data_ptr(), lp.data_ptr(), ent.data_ptr()), "vss_policy_sample")
    return a, lp, ent


Out = namedtuple("Out", ["action", "logprob", "entropy", "value", "mean"])


def forward(pol, obs, seed, counter, action_in=None):
    """vss_policy_forward over the contiguous rows `obs` with the packed weights of FusedPolicy `pol`."""
    N, lib, st = native()
    rows, n = obs.shape[0], pol.n_act
    assert obs.is_contiguous() and (action_in is None or action_in.is_contiguous())
    o = Out(nan(rows, n), nan(rows), nan(rows), nan(rows), nan(rows, n))
    N.check(lib.vss_policy_forward(st, rows, n, obs.data_ptr(), pol._actor.data_ptr(),
                                   pol.agent.actor_logstd.detach().data_ptr(), pol._critic.data_ptr(), seed, counter,
                                   N.ptr(action_in), o.action.data_ptr(), o.logprob.data_ptr(), o.entropy.data_ptr(),
                                   o.value.data_ptr(), o.mean.data_ptr()), "vss_policy_forward")
    return o


def actor_forward(pol, obs, seed, counter):
    N, lib, st = native()
    rows, n = obs.shape[0], pol.n_act
    a, m = nan(rows, n), nan(rows, n)
    N.check(lib.vss_actor_forward(st, rows, n, obs.data_ptr(), pol._actor.data_ptr(),
                                  pol.agent.actor_logstd.detach().data_ptr(), seed, counter, a.data_ptr(), m.data_ptr()),
            "vss_actor_forward")
    return a, m


def critic_forward(pol, obs, mask=None, out=None):
    """vss_value_forward_masked in its critic-only form (no actor), with or without a row mask."""
    N, lib, st = native()
    rows = obs.shape[0]
    v = nan(rows) if out is None else out
    N.check(lib.vss_value_forward_masked(st, rows, pol.n_act, obs.data_ptr(), None, None, pol._critic.data_ptr(), 0, 0,
                                         None, None, None, None, v.data_ptr(), None, N.ptr(mask)),
            "vss_value_forward_masked")
    return v


def group_table(count, group_rows, packed, logstds):
    N = native()[0]
    g = N.VssActorGroups()
    g.count, g.group_rows = count, group_rows
    for i in range(count):
        g.actor_packed[i] = None if packed is None else packed[i].data_ptr()
        g.logstd[i] = logstds[i].data_ptr()
    return g


def check_draws(action, seed, counter, n_act, mean=None, logstd=None):
    """|action - (mean + scale z_ref)| <= 16 * 2^-24 * (|mean| + scale rad) for every row and dim; returns the
    largest error in units of 2^-24 * (|mean| + scale rad).  The budget: libm logf, the square root, sincosf and the
    multiply (or FMA) at a few half-ulps each."""
    got = action.double().cpu().numpy()
    rows = got.shape[0]
    z, rad = PD.reference_pairs(seed, counter, np.arange(rows), n_act)
    mean = np.zeros_like(z) if mean is None else mean.double().cpu().numpy()
    scale = np.ones(n_act) if logstd is None else np.exp(logstd.double().cpu().numpy().reshape(n_act))
    want = mean + scale * z
    unit = U * (np.abs(mean) + scale * rad)
    err = np.abs(got - want)
    assert np.isfinite(got).all()
    assert (err <= 16.0 * unit).all(), f"worst row {np.unravel_index(np.argmax(err - 16.0 * unit), err.shape)}"
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


# ---- 2. the draws on the GPU ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("seed,counter", SEED_COUNTERS)
@pytest.mark.parametrize("n_act", [2, 6])
def test_sample_draws_match_the_host_specification(n_act, seed, counter):
    """mean 0, logstd 0: the action is z.  Every row and dim within 16 * 2^-24 * rad of the fp64 specification.
    Measured on an MI355X over all cases: the largest error is 2.59 x 2^-24 * rad (the bound is 16)."""
    logstd = torch.zeros(n_act, device=DEV)
    worst = 0.0
    for rows in (1, 255, 256, 257, 1000):
        a, _, _ = sample(rows, n_act, torch.zeros(rows, n_act, device=DEV), logstd, seed, counter)
        worst = max(worst, check_draws(a, seed, counter, n_act))
    print(f"draws n_act={n_act} seed={seed:#x} counter={counter:#x}: max error {worst:.3f} x 2^-24 rad")


@gpu
def test_edge_draws_stay_finite_and_reach_zero():
    """u1 = 2^-24 gives the largest radius, not inf (u1 cannot reach 0); u1 = 1 gives exactly 0 in both dims."""
    logstd = torch.zeros(2, device=DEV)
    a, _, _ = sample(30995, 2, torch.zeros(30995, 2, device=DEV), logstd, EDGE_SEED, 84)
    check_draws(a, EDGE_SEED, 84, 2)
    z = a[30994].double().cpu().numpy()
    rad = math.sqrt(-2.0 * math.log(2.0 ** -24))
    assert np.isfinite(z).all()
    # | |z| - rad | <= |z - z_ref| <= sqrt(2) * the per-dim bound
    assert abs(math.hypot(*z) - rad) <= math.sqrt(2.0) * 16.0 * U * rad
    a, _, _ = sample(49415, 2, torch.zeros(49415, 2, device=DEV), logstd, EDGE_SEED, 178)
    check_draws(a, EDGE_SEED, 178, 2)
    assert (a[49414] == 0.0).all()


@pytest.fixture(scope="module")
def zeroed():
    """Per action width, a FusedPolicy whose actor has a zero output layer and log-std 0: mean 0, action = z."""
    from vss_amd.policy import FusedPolicy
    out = {}
    for n_act in (2, 6):
        agent = make_agent(n_act, 300 + n_act, 0.0)
        with torch.no_grad():
            agent.actor_mean[8].weight.zero_()
            agent.actor_mean[8].bias.zero_()
            agent.actor_logstd.zero_()
        out[n_act] = FusedPolicy(agent, seed=0)
    torch.cuda.synchronize()
    return out


def obs_rows(rows, seed):
    return torch.randn(rows, 52, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 0.7


@gpu
@pytest.mark.parametrize("n_act", [2, 6])
def test_fused_entries_draw_the_bits_of_the_sample_kernel(zeroed, n_act):
    """Split, both and separate launches of vss_policy_forward and both regimes of vss_actor_forward: with a zero
    mean and unit scale their actions are vss_policy_sample's for the same (seed, counter, rows), bit for bit."""
    pol = zeroed[n_act]
    seed, counter = 0xFFFFFFFF00000001, 0x100000007
    obs = obs_rows(8193, 17)
    logstd = torch.zeros(n_act, device=DEV)
    want, _, _ = sample(8193, n_act, torch.zeros(8193, n_act, device=DEV), logstd, seed, counter)
    check_draws(want[:1000], seed, counter, n_act)
    for rows in (1000, 4097, 8193):
        o = forward(pol, obs[:rows], seed, counter)
        assert (o.mean == 0.0).all()
        assert torch.equal(o.action, want[:rows]), f"vss_policy_forward {rows}"
    for rows in (1000, 4097):
        a, m = actor_forward(pol, obs[:rows], seed, counter)
        assert (m == 0.0).all()
        assert torch.equal(a, want[:rows]), f"vss_actor_forward {rows}"


@gpu
def test_grouped_entries_draw_the_bits_of_the_sample_kernel(zeroed):
    """vss_actor_forward_grouped at (600 rows, groups of 192, n_act 2) and vss_policy_sample_grouped at (16,400 rows,
    groups of 4,160, n_act 6), the shapes of tests/test_league_kernels.py: the Philox row is the global row."""
    N, lib, st = native()
    seed, counter = 2 ** 63 + 5, 2 ** 40 + 3
    pol = zeroed[2]
    rows, group_rows, count = 600, 192, 4
    logstd = pol.agent.actor_logstd.detach().reshape(-1)
    g = group_table(count, group_rows, [pol._actor] * count, [logstd] * count)
    obs = obs_rows(rows, 18)
    a = nan(rows, 2)
    N.check(lib.vss_actor_forward_grouped(st, rows, 2, obs.data_ptr(), ctypes.byref(g), seed, counter, a.data_ptr(), None),
            "vss_actor_forward_grouped")
    want, _, _ = sample(rows, 2, torch.zeros(rows, 2, device=DEV), logstd, seed, counter)
    assert torch.equal(a, want)
    check_draws(a, seed, counter, 2)
    rows, group_rows, count = 16400, 4160, 4
    logstd = torch.zeros(6, device=DEV)
    g = group_table(count, group_rows, None, [logstd] * count)
    mean = torch.zeros(rows, 6, device=DEV)
    a = nan(rows, 6)
    N.check(lib.vss_policy_sample_grouped(st, rows, 6, mean.data_ptr(), ctypes.byref(g), seed, counter, a.data_ptr()),
            "vss_policy_sample_grouped")
    want, _, _ = sample(rows, 6, mean, logstd, seed, counter)
    assert torch.equal(a, want)
    check_draws(a, seed, counter, 6)


@gpu
@pytest.mark.parametrize("n_act", [2, 6])
def test_sample_scales_each_dim_by_its_own_logstd(n_act):
    """action = mean + exp(logstd[a]) z[a] against fp64, within 16 * 2^-24 * (|mean| + scale rad): expf, the draw's
    own budget and one multiply-add (the unit may contract it into an FMA).
    Measured on an MI355X: the largest error is 2.67 x 2^-24 * (|mean| + scale rad)."""
    rows, seed, counter = 1000, 77, 5
    logstd = torch.linspace(-1.2, 0.3, n_act, device=DEV)
    mean = torch.randn(rows, n_act, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    a, _, _ = sample(rows, n_act, mean, logstd, seed, counter)
    worst = check_draws(a, seed, counter, n_act, mean, logstd)
    print(f"scaled draws n_act={n_act}: max error {worst:.3f} x 2^-24 (|mean| + scale rad)")


@gpu
def test_fused_policy_counters(monkeypatch):
    """Which call uses which counter, as it is today: the first sampling call of a fresh FusedPolicy draws with
    counter 1, the next with 2; every call through _run's fused path advances the counter -- get_value and
    get_action_and_value with a given action included -- while on the chain path get_value does not (_run_chain
    returns before the increment), so a run's draw sequence depends on VSS_ROLLOUT_POLICY.  get_value_masked never
    advances it."""
    from vss_amd import policy as PM
    seed = 0xFFFFFFFF00000001
    agent = make_agent(2, 41, -1.0)
    logstd = agent.actor_logstd.detach()

    def is_draw(action, obs, counter):
        mean = PM.FusedPolicy(agent, seed=1).actor_mean(obs)  # another object: this one's counter stays
        check_draws(action, seed, counter, 2, mean, logstd)

    monkeypatch.setattr(PM, "ROLLOUT_POLICY", "fused")
    pol = PM.FusedPolicy(agent, seed=seed)
    obs = obs_rows(300, 19)
    assert pol.state_dict()["counter"] == 0
    a, _, _, _ = pol.get_action_and_value(obs)
    assert pol.state_dict()["counter"] == 1
    is_draw(a, obs, 1)
    a = pol.act(obs)
    assert pol.state_dict()["counter"] == 2
    is_draw(a, obs, 2)
    pol.get_value(obs)
    assert pol.state_dict()["counter"] == 3  # the fused path's get_value takes a counter
    pol.get_action_and_value(obs, a)
    assert pol.state_dict()["counter"] == 4  # and so does an evaluation of given actions
    pol.actor_mean(obs)
    assert pol.state_dict()["counter"] == 5
    mask = torch.ones(300, dtype=torch.long, device=DEV)
    pol.get_value_masked(obs, mask, torch.zeros(300, 1, device=DEV))
    assert pol.state_dict()["counter"] == 5
    a, _, _, _ = pol.get_action_and_value(obs)
    assert pol.state_dict()["counter"] == 6
    is_draw(a, obs, 6)
    only = PM.FusedPolicy(agent, seed=seed, actor_only=True)
    a = only.act(obs)
    assert only.state_dict()["counter"] == 1
    is_draw(a, obs, 1)
    only.actor_mean(obs)
    assert only.state_dict()["counter"] == 2

    monkeypatch.setattr(PM, "ROLLOUT_POLICY", "chain")
    pol = PM.FusedPolicy(agent, seed=seed)
    obs = obs_rows(PM.CHAIN_MIN_ROWS, 20)
    assert pol.chain_active(obs.shape[0])
    a, _, _, _ = pol.get_action_and_value(obs)
    assert pol.state_dict()["counter"] == 1
    is_draw(a, obs, 1)
    pol.get_value(obs)
    assert pol.state_dict()["counter"] == 1  # the chain path's get_value takes none
    a = pol.act(obs)
    assert pol.state_dict()["counter"] == 2
    is_draw(a, obs, 2)
    pol.get_action_and_value(obs, a)
    assert pol.state_dict()["counter"] == 3
    pol.actor_mean(obs)
    assert pol.state_dict()["counter"] == 4


# ---- 3. log-prob and entropy against fp64 --------------------------------------------------------------------------
def normal_reference(action, mean, logstd):
    """torch.distributions.Normal in fp64, summed over dims: (logprob, entropy, bound_lp, bound_ent) with the bounds
    8 * 2^-24 * the sum of the absolute terms."""
    a, m, ls = action.double(), mean.double(), logstd.double().reshape(1, -1)
    quad = (a - m) ** 2 / (2.0 * torch.exp(ls) ** 2)
    lp = (-quad - ls - HALF_LOG_2PI).sum(1)
    ent = (0.5 + HALF_LOG_2PI + ls).sum(1).expand_as(lp)
    b_lp = 8.0 * U * (quad + ls.abs() + HALF_LOG_2PI).sum(1)
    b_ent = 8.0 * U * (0.5 + HALF_LOG_2PI + ls.abs()).sum(1).expand_as(lp)
    return lp, ent, b_lp, b_ent


def spread_actions(mean, logstd):
    """mean + k scale with k from {0, +-0.5, +-6}, every k in every dim."""
    rows, n_act = mean.shape
    ks = torch.tensor([0.0, 0.5, -0.5, 6.0, -6.0], device=DEV)
    idx = (torch.arange(rows, device=DEV).view(-1, 1) + torch.arange(n_act, device=DEV).view(1, -1)) % 5
    return (mean + ks[idx] * torch.exp(logstd.reshape(1, -1))).contiguous()


def check_tail(name, lp, ent, action, mean, logstd):
    want_lp, want_ent, b_lp, b_ent = normal_reference(action, mean, logstd)
    e_lp, e_ent = (lp.double() - want_lp).abs(), (ent.double() - want_ent).abs()
    print(f"{name}: logprob error at most {float((e_lp / b_lp).max()) * 8:.3f}, entropy {float((e_ent / b_ent).max()) * 8:.3f} "
          "x 2^-24 x the sum of the absolute terms")
    assert (e_lp <= b_lp).all(), name
    assert (e_ent <= b_ent).all(), name


@gpu
@pytest.mark.parametrize("n_act", [2, 6])
def test_logprob_and_entropy_against_fp64(n_act):
    """Per-dim log-std linspace(-3, 1), actions at mean + {0, +-0.5, +-6} scale, 1000 rows; vss_policy_sample from
    given means and vss_policy_forward from its own mean_out, so only the tail is under test.  Bound:
    8 * 2^-24 * sum over dims of (|quadratic term| + |log scale| + 0.9189) -- the absolute terms, not their possibly
    cancelling sum; the entropy alike.  The log-prob returned with a sampled action equals, bit for bit, the one a
    second call computes from that action.  Measured on an MI355X, in 2^-24 x the sum of the absolute terms (the
    bound is 8): log-prob at most 2.49, entropy at most 0.96."""
    rows = 1000
    logstd = torch.linspace(-3.0, 1.0, n_act, device=DEV)
    mean = torch.randn(rows, n_act, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    action = spread_actions(mean, logstd)
    a, lp, ent = sample(rows, n_act, mean, logstd, 1, 1, action)
    assert torch.equal(a, action)
    check_tail(f"vss_policy_sample n_act={n_act}", lp, ent, action, mean, logstd)
    a, lp, ent = sample(rows, n_act, mean, logstd, 21, 4)
    check_tail(f"vss_policy_sample (sampled) n_act={n_act}", lp, ent, a, mean, logstd)
    a2, lp2, ent2 = sample(rows, n_act, mean, logstd, 21, 4, a)
    assert torch.equal(a2, a) and torch.equal(lp2, lp) and torch.equal(ent2, ent)

    from vss_amd.policy import FusedPolicy
    agent = make_agent(n_act, 50 + n_act, 0.0)
    with torch.no_grad():
        agent.actor_logstd.copy_(logstd.view(1, n_act))
    pol = FusedPolicy(agent, seed=0)
    obs = obs_rows(rows, 21)
    o = forward(pol, obs, 21, 4)
    check_tail(f"vss_policy_forward (sampled) n_act={n_act}", o.logprob, o.entropy, o.action, o.mean, logstd)
    o2 = forward(pol, obs, 21, 4, o.action)
    assert torch.equal(o2.mean, o.mean) and torch.equal(o2.action, o.action)
    assert torch.equal(o2.logprob, o.logprob) and torch.equal(o2.entropy, o.entropy)
    action = spread_actions(o.mean, logstd)
    o3 = forward(pol, obs, 21, 4, action)
    assert torch.equal(o3.mean, o.mean)
    check_tail(f"vss_policy_forward n_act={n_act}", o3.logprob, o3.entropy, action, o3.mean, logstd)


# ---- 4. one row, one result, in every regime ---------------------------------------------------------------------
BUF_ROWS = 8192 + 64 + 37
PREFIXES = (1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193)
# e_k <= M e_t + 1e-7 (test_means_and_values_against_fp64): the largest measured e_k / e_t, 1.10, doubled and
# rounded up
M_FP64 = 3


@pytest.fixture(scope="module")
def regimes():
    """Per action width: the policy, one observation buffer, a fixed action_in, and vss_policy_forward's outputs over
    the whole buffer (two launches, 64-row workgroups), computed once."""
    from vss_amd.policy import FusedPolicy
    out = {}
    for n_act in (2, 6):
        pol = FusedPolicy(make_agent(n_act, 60 + n_act, -1.2), seed=0)
        obs = obs_rows(BUF_ROWS, 22 + n_act)
        act = torch.randn(BUF_ROWS, n_act, device=DEV, generator=torch.Generator(device=DEV).manual_seed(23)) * 0.5
        whole = forward(pol, obs, 0, 0, act)
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in whole)
        out[n_act] = (pol, obs, act, whole)
    return out


def same_rows(name, got, whole, r0=0):
    n = got.mean.shape[0]
    for field in ("mean", "value", "logprob", "entropy"):
        assert torch.equal(getattr(got, field), getattr(whole, field)[r0:r0 + n]), f"{name}: {field}"


@gpu
@pytest.mark.parametrize("n_act", [2, 6])
def test_every_prefix_gives_a_row_the_same_bits(regimes, n_act):
    """policy_split_kernel (up to 4,096 rows), policy_kernel_both (to 8,192) and the two policy_kernel launches
    (above), each with a full and a ragged last wave: mean, value, log-prob and entropy of a row are those of the
    whole buffer's evaluation, so equal across every prefix that holds the row."""
    pol, obs, act, whole = regimes[n_act]
    for rows in PREFIXES:
        same_rows(f"prefix {rows}", forward(pol, obs[:rows], 0, 0, act[:rows]), whole)


@gpu
@pytest.mark.parametrize("n_act", [2, 6])
def test_actor_and_critic_entries_give_the_same_bits(regimes, n_act):
    """vss_actor_forward (actor_split_kernel, policy_kernel) and the critic-only vss_value_forward_masked, without a
    mask and with one, at sizes where vss_policy_forward takes each of its kernels."""
    pol, obs, act, whole = regimes[n_act]
    for rows in (1000, 4096, 4097, BUF_ROWS):
        _, mean = actor_forward(pol, obs[:rows], 3, 9)
        assert torch.equal(mean, whole.mean[:rows]), f"vss_actor_forward {rows}"
    for rows in (1000, 4096, 8193, BUF_ROWS):
        assert torch.equal(critic_forward(pol, obs[:rows]), whole.value[:rows]), f"critic only {rows}"
        mask = (torch.rand(rows, device=DEV, generator=torch.Generator(device=DEV).manual_seed(rows)) < 0.05).long()
        mask[-1] = 1
        out = torch.full((rows,), 7.0, device=DEV)
        critic_forward(pol, obs[:rows], mask, out)
        m = mask.bool()
        assert torch.equal(out[m], whole.value[:rows][m]), f"masked critic {rows}"
        assert (out[~m] == 7.0).all()


@gpu
@pytest.mark.parametrize("n_act", [2, 6])
def test_a_window_gives_each_row_the_bits_of_its_old_position(regimes, n_act):
    """obs[7 : 7 + n]: every row moves to another lane, wave and workgroup; its outputs do not."""
    pol, obs, act, whole = regimes[n_act]
    r0 = 7
    for rows in (1000, 4200, 8250):  # split, both, separate launches
        got = forward(pol, obs[r0:r0 + rows], 0, 0, act[r0:r0 + rows])
        same_rows(f"window {rows}", got, whole, r0)


@gpu
@pytest.mark.parametrize("n_act", [2, 6])
def test_means_and_values_against_fp64(regimes, n_act):
    """Once, at the whole buffer: e = max|out - ref| / max|ref| against the Agent's .double() copy, for the kernel
    (e_k; it uses fast_tanh) and for torch's fp32 forward (e_t).  e_k <= M e_t + 1e-7 with M the ratio measured
    on an MI355X, doubled and rounded up.  Measured (e_k, e_t, ratio): n_act 2 mean 6.66e-7, 6.05e-7, 1.10 and value
    6.27e-7, 6.14e-7, 1.02; n_act 6 mean 5.10e-7, 4.91e-7, 1.04 and value 5.61e-7, 7.29e-7, 0.77: M = 3."""
    pol, obs, act, whole = regimes[n_act]
    agent = pol.agent
    with torch.no_grad():
        ref = copy.deepcopy(agent).double()
        refs = {"mean": ref.actor_mean(obs.double()), "value": ref.get_value(obs.double()).view(-1)}
        torch32 = {"mean": agent.actor_mean(obs), "value": agent.get_value(obs).view(-1)}
    errs = {}
    for name, want in refs.items():
        top = float(want.abs().max())
        e_k = float((getattr(whole, name).double() - want).abs().max()) / top
        e_t = float((torch32[name].double() - want).abs().max()) / top
        print(f"fp64 n_act={n_act} {name}: e_k {e_k:.3e} e_t {e_t:.3e} ratio {e_k / e_t:.3f}")
        errs[name] = (e_k, e_t)
    for name, (e_k, e_t) in errs.items():
        assert e_k <= M_FP64 * e_t + 1e-7, name


# ---- 5. write extents ------------------------------------------------------------------------------------------------
def check_extents(name, call, inputs, outputs, full_outputs):
    for g in inputs:
        g.snapshot()
    rc = call()
    torch.cuda.synchronize()
    assert rc == 0, f"{name}: rc {rc}"
    for i, g in enumerate(inputs):
        assert g.guards_intact() and g.unchanged(), f"{name}: input {i} or its guards were written"
    for i, g in enumerate(outputs):
        assert g.guards_intact(), f"{name}: output {i} written outside its extent"
    for i, g in enumerate(full_outputs):
        assert g.covered(), f"{name}: output {i} not written in full"


def guarded_policy(n_act, seed):
    """Observations aside, what the fused entries read: packed actor, packed critic and log-std in guarded windows."""
    from vss_amd.policy import FusedPolicy
    pol = FusedPolicy(make_agent(n_act, seed, -1.2), seed=0)
    torch.cuda.synchronize()
    actor = Guarded(tuple(pol._actor.shape), fill=pol._actor)
    critic = Guarded(tuple(pol._critic.shape), fill=pol._critic)
    logstd = Guarded((n_act,), fill=pol.agent.actor_logstd.detach().reshape(-1))
    assert actor.ptr % 16 == 0 and critic.ptr % 16 == 0
    return actor, critic, logstd


@gpu
@pytest.mark.parametrize("rows,n_act", [(4097, 2), (8193, 6)])
def test_policy_forward_writes_only_its_outputs(rows, n_act):
    """policy_kernel_both and the two policy_kernel launches, each with one row in its last wave; sampled (every
    output written in full) and with action_in (an input, and still copied to action_out)."""
    N, lib, st = native()
    actor, critic, logstd = guarded_policy(n_act, 70 + n_act)
    obs = Guarded((rows, 52), fill=obs_rows(rows, 24))
    act_in = Guarded((rows, n_act), fill=torch.randn(rows, n_act, device=DEV) * 0.5)
    for given in (False, True):
        outs = [Guarded((rows, n_act)), Guarded((rows,)), Guarded((rows,)), Guarded((rows,)), Guarded((rows, n_act))]
        check_extents(f"vss_policy_forward {rows} action_in={given}",
                      lambda: lib.vss_policy_forward(st, rows, n_act, obs.ptr, actor.ptr, logstd.ptr, critic.ptr, 5, 6,
                                                     act_in.ptr if given else None, *[o.ptr for o in outs]),
                      [obs, actor, critic, logstd, act_in], outs, outs)
        if given:
            assert torch.equal(outs[0].t, act_in.t)


@gpu
@pytest.mark.parametrize("rows", [1000, 4097])
def test_actor_forward_writes_only_its_outputs(rows):
    N, lib, st = native()
    n_act = 6 if rows == 1000 else 2
    actor, _, logstd = guarded_policy(n_act, 80)
    obs = Guarded((rows, 52), fill=obs_rows(rows, 25))
    outs = [Guarded((rows, n_act)), Guarded((rows, n_act))]
    check_extents(f"vss_actor_forward {rows}",
                  lambda: lib.vss_actor_forward(st, rows, n_act, obs.ptr, actor.ptr, logstd.ptr, 5, 6, outs[0].ptr,
                                                outs[1].ptr),
                  [obs, actor, logstd], outs, outs)


@gpu
def test_masked_values_write_exactly_the_masked_rows():
    N, lib, st = native()
    rows = 4096 + 17
    _, critic, _ = guarded_policy(2, 81)
    obs = Guarded((rows, 52), fill=obs_rows(rows, 26))
    m = torch.zeros(rows, dtype=torch.long, device=DEV)
    m[torch.randperm(rows, device=DEV, generator=torch.Generator(device=DEV).manual_seed(27))[:100]] = 1
    m[-3:] = 1
    mask = Guarded((rows,), dtype=torch.long, fill=m)
    value = Guarded((rows,))
    check_extents("vss_value_forward_masked",
                  lambda: lib.vss_value_forward_masked(st, rows, 2, obs.ptr, None, None, critic.ptr, 0, 0, None, None,
                                                       None, None, value.ptr, None, mask.ptr),
                  [obs, critic, mask], [value], [])
    written = value.backing[GUARD:GUARD + rows] != SENTINEL
    assert torch.equal(written, m.bool())
    assert torch.isfinite(value.t[m.bool()]).all()


@gpu
def test_sample_writes_only_its_outputs():
    N, lib, st = native()
    rows, n_act = 257, 6
    mean = Guarded((rows, n_act), fill=torch.randn(rows, n_act, device=DEV))
    logstd = Guarded((n_act,), fill=torch.linspace(-1.2, 0.3, n_act, device=DEV))
    act_in = Guarded((rows, n_act), fill=torch.randn(rows, n_act, device=DEV))
    for given in (False, True):
        outs = [Guarded((rows, n_act)), Guarded((rows,)), Guarded((rows,))]
        check_extents(f"vss_policy_sample action_in={given}",
                      lambda: lib.vss_policy_sample(st, rows, n_act, mean.ptr, logstd.ptr, 5, 6,
                                                    act_in.ptr if given else None, *[o.ptr for o in outs]),
                      [mean, logstd, act_in], outs, outs)


@gpu
@pytest.mark.parametrize("n_out", [1, 2, 6])
def test_mlp_pack_writes_exactly_the_packed_size(n_out):
    N, lib, st = native()
    dims = [52, 256, 512, 512, 256, n_out]
    gen = torch.Generator(device=DEV).manual_seed(28 + n_out)
    ws = [Guarded((dims[i + 1], dims[i]), fill=torch.randn(dims[i + 1], dims[i], device=DEV, generator=gen))
          for i in range(5)]
    bs = [Guarded((dims[i + 1],), fill=torch.randn(dims[i + 1], device=DEV, generator=gen)) for i in range(5)]
    size = lib.vss_mlp_packed_size(n_out)
    assert size == 528 * 1024 + n_out * 256 + 256 + 512 + 512 + 256 + n_out
    packed = Guarded((size,))
    wa = (ctypes.c_void_p * 5)(*[w.ptr for w in ws])
    ba = (ctypes.c_void_p * 5)(*[b.ptr for b in bs])
    check_extents(f"vss_mlp_pack n_out={n_out}", lambda: lib.vss_mlp_pack(st, n_out, wa, ba, packed.ptr),
                  ws + bs, [packed], [packed])
    # a permutation of the parameters plus layer 1's zero padding: nothing lost, nothing invented
    got = packed.t
    assert torch.equal(got[size - n_out:], bs[4].t) and torch.equal(got[size - n_out - 256:size - n_out], bs[3].t)
    stream = got[:528 * 1024]
    total = sum(float(w.t.double().abs().sum()) for w in ws[:4])
    assert abs(float(stream.double().abs().sum()) - total) <= 1e-9 * total
    assert int((stream == 0).sum()) >= 16 * 1024 - 52 * 256
