"""Policy opponents: FusedPolicy.act (actor only), SnapshotOpponent, and the wrappers' set_opponent."""
from collections import namedtuple

import numpy as np
import pytest
import torch

import oracle as O
import ppo_continuous_action_isaacgym as P
from envs._gym import Box

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Env = namedtuple("Env", ["single_observation_space", "single_action_space"])


def make_agent(act_dim, seed):
    torch.manual_seed(seed)
    a = P.Agent(Env(Box(-np.inf, np.inf, (52,)), Box(-1.0, 1.0, (act_dim,)))).to(DEV)
    with torch.no_grad():  # non-trivial last layers and log-std (init has 0.01-scaled actor outputs)
        a.actor_mean[8].weight.mul_(50.0)
        a.actor_logstd.fill_(-0.7)
        for m in a.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.1, 0.1)
    return a


def make_vss(n, max_len=400, seed=1234):
    from envs.vss import VSS, default_cfg
    cfg = default_cfg(n)
    cfg["env"]["maxEpisodeLength"] = max_len
    cfg["env"]["seed"] = seed
    return VSS(cfg, DEV, DEV, 0, True, False, False)


def host_from(env) -> O.HostEnv:
    h = O.HostEnv(env.num_fields)
    h.state[:] = env.state.cpu().numpy()
    h.progress[:] = env.progress_buf.cpu().numpy()
    h.reset[:] = env.reset_buf.cpu().numpy()
    h.dof[:] = env.dof_velocity_buf.reshape(-1, 12).cpu().numpy()
    h.ctr[:] = env.rng_counter.cpu().numpy().view(np.uint32)
    return h


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32) if t.dtype == torch.float32 else t.detach().cpu().numpy()


def scripted_team(act, obs):
    """A deterministic function of the team's observations, past the clamp in places."""
    act.copy_(torch.tanh(obs[:, :, 4:6] * 3.0 + obs[:, :, 0:2]) * 1.2)


# 48 rows: the actor-only split kernel; 8,192: policy_kernel<NACT, true> alone (the full forward runs
# policy_kernel_both there: the action does not depend on which kernel evaluates it; a self-play run
# at 4,095 envs has 12,285 opponent rows on this branch); 16,384 (CHAIN_MIN_ROWS): the GEMM chain +
# vss_policy_sample
@pytest.mark.parametrize("rows", [48, 8192, 16384])
@pytest.mark.parametrize("act_dim", [2, 6])
def test_act_matches_the_full_forward(act_dim, rows):
    from vss_amd import policy as PM
    assert PM.CHAIN_MIN_ROWS == 16384
    agent = make_agent(act_dim, 11 + act_dim)
    full, actor = PM.FusedPolicy(agent, seed=21), PM.FusedPolicy(agent, seed=21)
    obs = torch.randn(rows, 52, device=DEV) * 0.7
    for _ in range(2):  # equal (seed, counter, row): equal action, call after call
        want, _, _, _ = full.get_action_and_value(obs)
        got, mean = actor.act(obs, want_mean=True)
        assert full.counter == actor.counter
        assert torch.equal(got, want)
    with torch.no_grad():
        mean_t = agent.actor_mean(obs)
    torch.testing.assert_close(mean, mean_t, rtol=2e-5, atol=2e-6)
    out = torch.empty((rows, act_dim), device=DEV)
    assert actor.act(obs, out=out) is out
    assert not torch.equal(out, got)  # a fresh draw on every call


def test_actor_only_policy_has_no_critic():
    from vss_amd.opponent import SnapshotOpponent
    opp = SnapshotOpponent(make_agent(2, 1), "x3", seed=1)
    obs = torch.randn(48, 52, device=DEV)
    with pytest.raises(ValueError):
        opp.policy.get_value(obs)
    with pytest.raises(ValueError):
        opp.policy.values_chain(obs)
    with pytest.raises(ValueError):
        opp.policy.get_value_masked(obs, torch.ones(48, dtype=torch.long, device=DEV), torch.zeros(48, 1, device=DEV))
    with torch.no_grad():
        want = opp.actor.actor_mean(obs)
    torch.testing.assert_close(opp.policy.actor_mean(obs), want, rtol=2e-5, atol=2e-6)
    with pytest.raises(ValueError):
        SnapshotOpponent(make_agent(2, 1), "cma")  # a 6-action team needs a 6-action Agent


@pytest.mark.parametrize("kind,act_dim", [("x3", 2), ("cma", 6)])
def test_snapshot_is_isolated_until_sync(kind, act_dim, tmp_path):
    from vss_amd.opponent import SnapshotOpponent
    from vss_amd.policy import FusedPolicy
    agent = make_agent(act_dim, 3)
    opp = SnapshotOpponent(agent, kind, seed=5)
    n = 16
    obs = torch.randn(n, 3, 52, device=DEV) * 0.7
    rows = obs.reshape(n * 3, 52) if kind == "x3" else obs[:, 0, :]

    def play():
        opp.policy.counter = 0  # the same draws every time
        act = torch.zeros((n, 3, 2), device=DEV)
        opp(act, obs)
        return act

    a0 = play()
    assert torch.equal(a0.reshape(-1), FusedPolicy(agent, seed=5).act(rows).reshape(-1))
    torch.save(agent.state_dict(), tmp_path / "agent.pt")
    with torch.no_grad():
        for p in agent.parameters():
            p.add_(0.05 * torch.randn_like(p))
    assert torch.equal(play(), a0)  # the learner moved, the snapshot did not
    opp.sync(agent, version=4)
    a1 = play()
    assert opp.version == 4 and not torch.equal(a1, a0)
    assert torch.equal(a1.reshape(-1), FusedPolicy(agent, seed=5).act(rows).reshape(-1))
    opp.load(str(tmp_path / "agent.pt"))  # back to the saved weights, from a reference-format checkpoint
    assert torch.equal(play(), a0)


@pytest.mark.parametrize("mode", ["sa", "cma", "dma"])
def test_wrapper_with_a_scripted_team_equals_the_direct_call(mode):
    from envs.wrappers import CMA, DMA, SingleAgent
    cls = {"sa": SingleAgent, "cma": CMA, "dma": DMA}[mode]
    n = 67
    env_w, env_d = make_vss(n, max_len=10), make_vss(n, max_len=10)
    W = cls(env_w)
    W.set_opponent(scripted_team)
    h = host_from(env_w)
    want0 = O.compute_obs(h, 6)[:, 3:6]
    np.testing.assert_array_equal(bits(W._opp_obs), want0.view(np.uint32))
    W.reset()
    np.testing.assert_array_equal(bits(W._opp_obs), want0.view(np.uint32))

    A = 3 if mode == "dma" else 1
    rows, width = n * A, (6 if mode == "cma" else 2)
    io = dict(ou_buf=torch.zeros((n, 12), device=DEV), obs=torch.zeros((rows, 52), device=DEV),
              terminal_obs=torch.zeros((rows, 52), device=DEV), rew=torch.zeros((rows, 4), device=DEV),
              reward_sum=torch.zeros(rows, device=DEV),
              dones_rep=torch.zeros(rows, dtype=torch.long, device=DEV) if mode == "dma" else None,
              time_outs=torch.zeros(rows, dtype=torch.bool, device=DEV), progress_f=torch.zeros(rows, device=DEV))
    opp_obs = torch.from_numpy(want0.copy()).to(DEV)
    opp_act = torch.zeros((n, 3, 2), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(17)
    resets = 0
    for t in range(25):
        a = torch.rand((rows, width), device=DEV, generator=gen) * 2.4 - 1.2
        obs, reward, dones, infos = W.step(a)
        scripted_team(opp_act, opp_obs)
        env_d.native_step_versus(cls.MODE, a, io, opp_act, opp_obs)
        msg = f"{mode} step {t}"
        assert infos["opponent_obs"] is W._opp_obs
        for got, want, what in ((obs["obs"], io["obs"], "obs"), (infos["terminal_observation"], io["terminal_obs"], "term"),
                                (infos["opponent_obs"], opp_obs, "opponent_obs"), (reward, io["reward_sum"], "reward"),
                                (infos["rews"], io["rew"], "rews"), (W.action_buf.view(n, 12), io["ou_buf"], "action_buf"),
                                (env_w.state, env_d.state, "state")):
            np.testing.assert_array_equal(bits(got).reshape(-1), bits(want).reshape(-1), err_msg=f"{msg} {what}")
        want_dones = io["dones_rep"] if mode == "dma" else env_d.reset_buf
        assert torch.equal(dones, want_dones) and torch.equal(infos["time_outs"], io["time_outs"])
        resets += int(env_d.reset_buf.sum())
    assert resets > 0


def test_set_opponent_none_restores_the_plain_path():
    from envs.wrappers import SingleAgent
    n = 67
    Wa, Wb = SingleAgent(make_vss(n, max_len=10)), SingleAgent(make_vss(n, max_len=10))
    Wa.set_opponent(scripted_team)
    Wa.set_opponent(None)
    gen = torch.Generator(device=DEV).manual_seed(2)
    for t in range(15):
        a = torch.rand((n, 2), device=DEV, generator=gen) * 2.4 - 1.2
        (oa, ra, da, ia), (ob, rb, db, ib) = Wa.step(a), Wb.step(a)
        assert "opponent_obs" not in ia
        assert torch.equal(oa["obs"], ob["obs"]) and torch.equal(ra, rb) and torch.equal(da, db)
        assert torch.equal(Wa.action_buf, Wb.action_buf) and torch.equal(Wa.env.state, Wb.env.state)
    assert (Wa.action_buf[:, 1] != 0).any()  # the OU process drives yellow again


def test_play_teams_are_accepted_as_opponents(tmp_path):
    from envs.wrappers import SingleAgent
    from play import get_team
    path = str(tmp_path / "agent2.pt")
    torch.save(make_agent(2, 9).state_dict(), path)
    n = 67
    env = make_vss(n, max_len=10)
    W = SingleAgent(env)
    a = torch.zeros((n, 2), device=DEV)
    W.set_opponent(get_team("zero"))
    for _ in range(3):
        W.step(a)
    assert (W.action_buf[:, 1] == 0).all() and (W.action_buf[:, 0, 1:] != 0).any()  # yellow still, blue 1-2 on OU
    W.set_opponent(get_team("ppo-dma", path, DEV))
    for _ in range(3):
        obs, _, dones, infos = W.step(a)
    live = dones == 0
    assert live.any() and torch.equal(W.action_buf[:, 1][live], W._opp_act[live]) and (W._opp_act != 0).any()
    assert torch.isfinite(obs["obs"]).all() and torch.isfinite(infos["opponent_obs"]).all()
