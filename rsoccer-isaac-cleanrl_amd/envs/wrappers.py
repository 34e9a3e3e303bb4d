"""Drop-in wrappers of the reference's envs/wrappers.py, fused into the HIP step.

`SingleAgent`, `CMA` and `DMA` keep the reference's behaviour (envs/wrappers.py:89-180): the
robots the learner does not control are driven by Ornstein-Uhlenbeck noise on the wrapper's
`action_buf` (random_ou, envs/wrappers.py:5-19), the learner's actions overwrite their slots,
the step runs, `action_buf` is zeroed for finished fields, and observations / rewards are sliced
to the learner's view.  Here all of that happens inside the single `vss_step` launch
(VSS_MODE_SA/CMA/DMA): the OU noise is drawn by the kernel's Philox stream, and only the
learner's rows are written to HBM — no (N,2,3,52) observation tensor, no host sync on `dones`.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from vss_amd import _native as N
from vss_amd.checkpoint import copy_entries, entry, to_cpu

from ._gym import Box, Wrapper
from .vss import VSS, default_cfg


def random_ou(prev: torch.Tensor) -> torch.Tensor:
    """One OU step on an action buffer: clamp(prev - 0.1 prev + N(0, 0.15^2), -1, 1).

    Same update as the reference's random_ou (envs/wrappers.py:5-19) in plain torch, for
    callers that drive their own action buffers (e.g. play.py's TeamOU); the wrappers below do
    it inside the HIP step."""
    theta, sigma = 0.1, 0.15
    noise = torch.randn(prev.shape, device=prev.device, dtype=prev.dtype) * sigma
    return (prev - theta * prev + noise).clamp(-1.0, 1.0)


def _local_device() -> str:
    # one process per GPU: LOCAL_RANK; VSS_LOCAL_DEVICE pins it (several ranks on one GPU)
    return f"cuda:{int(os.environ.get('VSS_LOCAL_DEVICE', os.environ.get('LOCAL_RANK', 0)))}"


def make_env(args):
    """(unwrapped VSS, wrapped env) for args.env_id in {sa, cma, dma} (envs/wrappers.py:21-48).

    args.opponent ('ou' when absent) is only validated here: the returned wrapper drives the yellow
    team with OU noise until its set_opponent(team) is called.  Except 'mirror': the mirror wrapper
    of the env_id, in which both teams' robots are learner rows and there is no opponent.  A policy opponent needs the Agent,
    which exists only after the env, so the train loop (or any other caller) builds the team --
    vss_amd.opponent.SnapshotOpponent -- and calls set_opponent itself."""
    assert args.cuda
    cfg = default_cfg(args.num_envs)
    opponent = getattr(args, "opponent", "ou")
    if opponent == "mirror":
        # both teams' robots are learner rows: num_envs counts rows (dma's precedent), 2 R per field
        per_field = 6 if args.env_id == "dma" else 2
        if args.num_envs % per_field != 0:
            raise ValueError(f"--opponent mirror: --num-envs counts learner rows, {per_field} per field for "
                             f"{args.env_id}; {args.num_envs} is not a multiple of {per_field}")
        cfg["env"]["numEnvs"] = args.num_envs // per_field
    elif args.env_id == "dma":
        assert args.num_envs % 3 == 0
        cfg["env"]["numEnvs"] = int(args.num_envs / 3)
    if getattr(args, "seed", None) is not None:
        cfg["env"]["seed"] = int(args.seed) * 1000003 + int(os.environ.get("RANK", 0))
    device = _local_device()
    envs = VSS(cfg=cfg, rl_device=device, sim_device=device, graphics_device_id=0,
               headless=not getattr(args, "capture_video", False),
               virtual_screen_capture=getattr(args, "capture_video", False), force_render=False)
    wrappers = {"sa": SingleAgent, "cma": CMA, "dma": DMA}
    if opponent == "mirror":
        wrappers = {"sa": MirrorSingleAgent, "cma": MirrorCMA, "dma": MirrorDMA}
    elif opponent != "ou" and not (opponent in ("self", "pool", "scripted") or os.path.exists(opponent)):
        raise ValueError(f"--opponent must be ou, self, pool, mirror, scripted or a checkpoint path, got {opponent!r}")
    # the opponent itself (a snapshot of the Agent) is set by the train loop: set_opponent()
    wrapped = wrappers[args.env_id](envs)
    table = setplay_table(args)
    if table is not None:  # --setplay-share > 0: inside every channel wrapper; with 0 the chain is as without the flags
        from vss_amd.setplay import Stager
        wrapped.set_setplays(Stager(envs.num_fields, table, setplay_seed(getattr(args, "seed", None)), envs.device))
    from vss_amd.referee import referee_of_args
    referee = referee_of_args(args, envs.num_fields, envs.device)
    if referee is not None:  # --ref-stall-steps / --ref-area-steps > 0: beside the stager; else the chain is as before
        wrapped.set_referee(referee)
    delay, noise = perception_args(args)
    if delay or noise.any():  # --obs-delay / --obs-noise-*: with all of them zero the chain is as without the flags
        wrapped = Perceived(wrapped, delay, noise, perception_seed(getattr(args, "seed", None)))
    track = tracking_args(args)
    if track.any():  # --obs-filter-*: round Perceived, inside Estimated; with every gain 0 the chain is as without the flags
        wrapped = Tracked(wrapped, track)
    if estimation_args(args):  # --obs-predict 1: between Perceived and the policy; with 0 the chain is as without the flag
        wrapped = Estimated(wrapped)
    params = actuation_args(args)
    if params.any():  # --act-*: the outermost wrapper; with all of them zero the chain is as without the flags
        wrapped = Actuated(wrapped, params, actuation_seed(getattr(args, "seed", None)))
    return envs, wrapped


def setplay_table(args):
    """The set-play table of --setplay-share / --setplay-mix / --setplay-file (vss_amd/setplay.py); None with a share
    of 0, the default."""
    from vss_amd.setplay import table_of_args
    return table_of_args(args)


def setplay_seed(seed, offset: int = 0) -> int:
    """The stager's Philox key, built as perception_seed with a constant of its own; `offset` separates the arena's
    stager (1) from the training's."""
    from vss_amd.setplay import setplay_seed as key
    return key(seed, offset)


def perception_args(args):
    """(delay, Noise) of --obs-delay and --obs-noise-pos / -vel / -ang / -angvel; absent flags are zero."""
    from vss_amd.perceive import Noise
    return int(getattr(args, "obs_delay", 0) or 0), Noise(*(float(getattr(args, f"obs_noise_{k}", 0.0) or 0.0)
                                                           for k in ("pos", "vel", "ang", "angvel")))


def perception_seed(seed, offset: int = 0) -> int:
    """The channel's Philox key from --seed and the rank, with a constant of its own (the env's key is
    seed * 1000003 + rank); `offset` separates the arena's channel from the training's."""
    return (int(seed or 0) * 1000003 + int(os.environ.get("RANK", 0))) * 2654435761 + 0x5EE1_0B5E + int(offset)


def evaluation_channel(args, env, offset: int = 2):
    """evaluate()'s channel over the blue rows of the raw env's FULL layout (play.play_matches), with a key of its
    own; None when the perception flags are all zero."""
    from vss_amd import perceive as P
    delay, noise = perception_args(args)
    if not (delay or noise.any()):
        return None
    n = env.num_fields
    return P.PerceptionChannel(n, P.layout_full_blue(), delay, noise, perception_seed(getattr(args, "seed", None), offset),
                               env.device, rows=n * 6)


def estimation_args(args) -> bool:
    """--obs-predict as a bool; an absent flag is 0.  1 with --obs-delay 0 is refused (checkpoint.check_estimation)."""
    from vss_amd.checkpoint import check_estimation
    return bool(int(getattr(check_estimation(args), "obs_predict", 0) or 0))


def evaluation_estimation(args, env):
    """evaluate()'s estimation channel over the blue rows of the raw env's FULL layout (play.play_matches), applied
    after the perception channel; None when --obs-predict is 0."""
    from vss_amd import estimate as E
    if not estimation_args(args):
        return None
    n = env.num_fields
    return E.EstimationChannel(n, E.layout_full_blue(), perception_args(args)[0], env.device, rows=n * 6)


def tracking_args(args):
    """Params of --obs-filter-team / -opp / -ball / -gate-pos / -gate-vel; absent flags have their defaults (gains 0).
    A gain without vision noise, or a value out of range, is refused (checkpoint.check_tracking)."""
    from vss_amd.checkpoint import TRACKING_DEFAULTS, TRACKING_STRUCTURAL, check_tracking
    from vss_amd.track import Params
    check_tracking(args)
    return Params(*(float(d if getattr(args, k, None) is None else getattr(args, k))
                    for k, d in ((k, TRACKING_DEFAULTS[k]) for k in TRACKING_STRUCTURAL)))


def evaluation_tracking(args, env):
    """evaluate()'s tracking channel over the blue rows of the raw env's FULL layout (play.play_matches), applied
    after the perception channel and before the estimation channel; None when every gain is 0."""
    from vss_amd import track as T
    params = tracking_args(args)
    if not params.any():
        return None
    n = env.num_fields
    return T.TrackingChannel(n, T.layout_full_blue(), perception_args(args)[0], params, env.device, rows=n * 6)


def evaluation_kwargs(args, env) -> dict:
    """evaluate()'s channels as play.play_matches' keyword arguments; None for flags that are all zero."""
    perceive, actuate = evaluation_channels(args, env)
    return dict(perceive=perceive, actuate=actuate, estimate=evaluation_estimation(args, env),
                track=evaluation_tracking(args, env))


def actuation_args(args):
    """Params of --act-gain / -noise / -deadband / -loss / -levels; absent flags are zero."""
    from vss_amd.actuate import Params
    return Params(*(float(getattr(args, f"act_{k}", 0.0) or 0.0) for k in ("gain", "noise", "deadband", "loss")),
                  int(getattr(args, "act_levels", 0) or 0))


def actuation_seed(seed, offset: int = 0) -> int:
    """The actuation channel's Philox key, built as perception_seed with a constant of its own; `offset` separates
    the arena's (1) and evaluate()'s (2) channels from the training's."""
    return (int(seed or 0) * 1000003 + int(os.environ.get("RANK", 0))) * 2654435761 + 0xAC7_0A7E + int(offset)


def evaluation_actuation(args, env, offset: int = 2):
    """evaluate()'s channel over the blue half of the raw env's FULL action buffer (play.play_matches), with a key of
    its own; None when the actuation flags are all zero."""
    from vss_amd import actuate as A
    params = actuation_args(args)
    if not params.any():
        return None
    n = env.num_fields
    return A.ActuationChannel(n, A.layout_full_blue(), params, actuation_seed(getattr(args, "seed", None), offset),
                              env.device, rows=n * 6)


def evaluation_channels(args, env):
    """evaluate()'s (perception channel, actuation channel) for play.play_matches; None for flags that are all zero."""
    return evaluation_channel(args, env), evaluation_actuation(args, env)


class RecordEpisodeStatisticsTorch(Wrapper):
    """Running per-env returns (goal, grad, move, energy) and lengths (envs/wrappers.py:50-87),
    updated by one HIP launch per step (`vss_episode_stats`) instead of seven elementwise ops."""

    def __init__(self, env, device):
        super().__init__(env)
        self.num_envs = getattr(env, "num_envs", 1)
        self.device = N.require_device(device)
        self.episode_returns = None
        self.episode_lengths = None

    def reset(self, **kwargs):
        observations = super().reset(**kwargs)
        n = self.num_envs
        self.episode_returns = torch.zeros((n, 4), dtype=torch.float32, device=self.device)
        self.episode_lengths = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.returned_episode_returns = torch.zeros_like(self.episode_returns)
        self.returned_episode_lengths = torch.zeros_like(self.episode_lengths)
        self.returned_return_sum = torch.zeros(n, dtype=torch.float32, device=self.device)
        return observations

    def _state_tensors(self) -> dict:
        if self.episode_returns is None:
            raise ValueError("RecordEpisodeStatisticsTorch: reset() allocates the statistics; call it first")
        return {k: getattr(self, k) for k in ("episode_returns", "episode_lengths", "returned_episode_returns",
                                              "returned_episode_lengths", "returned_return_sum")}

    def state_dict(self) -> dict:
        """The five running-statistics tensors on the CPU (vss_amd.checkpoint)."""
        return to_cpu(self._state_tensors())

    def load_state_dict(self, state: dict) -> None:
        copy_entries("RecordEpisodeStatisticsTorch", self._state_tensors(), state)

    def step(self, action):
        observations, rewards, dones, infos = super().step(action)
        rews = infos["rews"]
        n = self.num_envs
        if (rews.shape != (n, 4) or rews.dtype != torch.float32 or not rews.is_contiguous()
                or dones.numel() != n or dones.dtype != torch.long or not dones.is_contiguous()):
            raise ValueError("episode statistics expect rews (N, 4) float32 and dones (N,) int64, contiguous")
        N.check(N.load().vss_episode_stats(
            N.stream_of(self.device), n, rews.data_ptr(), dones.data_ptr(), self.episode_returns.data_ptr(),
            self.episode_lengths.data_ptr(), self.returned_episode_returns.data_ptr(),
            self.returned_episode_lengths.data_ptr(), self.returned_return_sum.data_ptr()), "vss_episode_stats")
        r = self.returned_episode_returns
        infos["r"] = {"goal": r[:, 0], "grad": r[:, 1], "move": r[:, 2], "energy": r[:, 3],
                      "return": self.returned_return_sum}
        infos["l"] = self.returned_episode_lengths
        return observations, rewards, dones, infos


def _referee_record(ref, rec: dict, writer=None, step: int = 0) -> None:
    """The train loop's call on a fused or mirror wrapper, once per update: the referee's calls since the last one go
    into `rec` and to the writer as referee/free_ball, /penalty_for, /penalty_against, /goal_kick_for,
    /goal_kick_against ("for": blue's to take) -- one host read of eight counts; nothing without a referee."""
    for k, v in (ref.record() if ref is not None else {}).items():
        rec[k] = v
        if writer is not None:
            writer.add_scalar(k, v, step)


class _FusedWrapper(Wrapper):
    """Common part of SA / CMA / DMA: the OU action buffer and the packed output buffers."""

    MODE = None
    LEARNER_WIDTH = 2  # floats per learner row
    ROWS_PER_FIELD = 1  # learner rows per field

    def __init__(self, env: VSS):
        super().__init__(env)
        self.action_buf = env.dof_velocity_buf.clone()  # (N,2,3,2) OU state
        n, dev = env.num_fields, env.device
        rows = n * self.ROWS_PER_FIELD
        self._obs = torch.zeros((rows, env.num_obs), device=dev)
        self._terminal_obs = torch.zeros_like(self._obs)
        self._rews = torch.zeros((rows, 4), device=dev)
        self._reward = torch.zeros(rows, device=dev)
        if self.ROWS_PER_FIELD == 1:
            self._time_outs, self._progress = env.timeout_buf, env.progress_f_buf
            self._dones = None
        else:
            self._time_outs = torch.zeros(rows, dtype=torch.bool, device=dev)
            self._progress = torch.zeros(rows, device=dev)
            self._dones = torch.zeros(rows, dtype=torch.long, device=dev)
        env.compute_observations(self._obs, n_agents=3 if self.ROWS_PER_FIELD == 3 else 1)
        self._opponent = None  # yellow team policy (set_opponent); None: the kernel's OU process
        self._opp_obs = self._opp_act = None
        self._setplays = None  # vss_amd.setplay.Stager (set_setplays); None: every episode starts from the uniform drop
        self._referee = None  # vss_amd.referee.Referee (set_referee); None: nothing is whistled inside an episode

    def _first_obs(self):
        self.env.compute_observations(self._obs, n_agents=3 if self.ROWS_PER_FIELD == 3 else 1)
        return {"obs": self._obs}

    def _first_opp_obs(self):
        """The yellow robots' observations of the current state (rows [:, 1] of the FULL layout);
        once per reset / set_opponent -- every versus step then writes them itself."""
        env = self.env
        full = torch.empty((env.num_fields, 2, 3, env.num_obs), device=env.device)
        env.compute_observations(full, n_agents=6)
        self._opp_obs.copy_(full[:, 1])

    def _setplay_views(self):
        """The rows a staged field rewrites: the learner's and, with a policy opponent, the versus step's opp_obs."""
        from vss_amd import setplay as S
        views = [(self._obs, S.view_dma() if self.ROWS_PER_FIELD == 3 else S.view_sa())]
        if self._opponent is not None:
            views.append((self._opp_obs, S.view_opponent()))
        return views

    def set_setplays(self, stager=None):
        """Start a share of the episodes from the stager's set plays (vss_amd/setplay.py): one start
        call here, on the fresh fields, so the first episodes follow the mix as well, then one vss_setplay launch
        after every step.  None (the default) restores the uniform drop alone and step() is as before."""
        self._setplays = stager
        if stager is not None:
            stager.start(self.env.state, self._setplay_views())

    def set_referee(self, ref=None):
        """Call free balls, penalties and goal kicks inside the episodes (vss_amd/referee.py): one
        vss_referee launch after every step, after the set plays, over the set plays' views.  None (the default):
        step() is as before."""
        self._referee = ref

    def referee_record(self, rec: dict, writer=None, step: int = 0) -> None:
        _referee_record(self._referee, rec, writer, step)

    def set_opponent(self, team=None):
        """Drive the yellow team with `team` -- play.py's protocol, team(act (N,3,2) written in place,
        obs (N,3,52)) -- inside the fused step (vss_step_versus) instead of OU noise; None (the
        default) restores the OU opponent and step() is the plain path again."""
        if team is not None and hasattr(team, "check_env"):
            team.check_env(self.env)  # e.g. OpponentPool: the field count and a positive goal weight
        self._opponent = team
        if team is None:
            return
        if self._opp_obs is None:
            n, dev = self.env.num_fields, self.env.device
            self._opp_obs = torch.zeros((n, 3, self.env.num_obs), device=dev)
            self._opp_act = torch.zeros((n, 3, 2), device=dev)
        self._first_opp_obs()

    def reset(self, **kwargs):
        self.env.reset(**kwargs)
        if self._opponent is not None:
            self._first_opp_obs()
        return self._first_obs()

    def _state_tensors(self) -> dict:
        own = self.ROWS_PER_FIELD != 1  # else time_outs / progress are the env's buffers, saved with the env
        return dict(action_buf=self.action_buf, obs=self._obs, terminal_obs=self._terminal_obs, rews=self._rews,
                    reward=self._reward, dones=self._dones, time_outs=self._time_outs if own else None,
                    progress=self._progress if own else None, opp_obs=self._opp_obs, opp_act=self._opp_act)

    def state_dict(self) -> dict:
        """The wrapper's own buffers on the CPU (vss_amd.checkpoint): the OU state, the learner's current
        observations (the next rollout's first input) and the other outputs, the opponent's rows when one is
        set.  The env's and the opponent's state are saved by their owners."""
        out = to_cpu({k: t for k, t in self._state_tensors().items() if t is not None})
        if self._setplays is not None:
            out["setplays"] = self._setplays.state_dict()
        if self._referee is not None:
            out["referee"] = self._referee.state_dict()
        return out

    def load_state_dict(self, state: dict) -> None:
        copy_entries(type(self).__name__, self._state_tensors(), state)
        if self._setplays is not None:
            self._setplays.load_state_dict(entry(state, "setplays", type(self).__name__))
        if self._referee is not None:
            self._referee.load_state_dict(entry(state, "referee", type(self).__name__))

    def _rews_view(self):
        return self._rews

    def step(self, action):
        env = self.env
        io = dict(ou_buf=self.action_buf, obs=self._obs, terminal_obs=self._terminal_obs, rew=self._rews,
                  reward_sum=self._reward, dones_rep=self._dones, time_outs=self._time_outs,
                  progress_f=self._progress)
        infos = {"rews": self._rews_view(), "terminal_observation": self._terminal_obs,
                 "time_outs": self._time_outs, "progress_buffer": self._progress}
        if self._opponent is None:
            env.native_step(self.MODE, action, io)
        else:
            self._opponent(self._opp_act, self._opp_obs)
            env.native_step_versus(self.MODE, action, io, self._opp_act, self._opp_obs)
            infos["opponent_obs"] = self._opp_obs
            if hasattr(self._opponent, "observe"):  # a league counts the finished fields' results per slot
                self._opponent.observe(self._rews, env.reset_buf if self._dones is None else self._dones,
                                       self._progress)
        if self._setplays is not None:  # the fields the step has just reset: a share of them from a set play
            self._setplays.stage(env.state, self._setplay_views(), env.reset_buf)
        if self._referee is not None:  # the fields that go on: stoppages; the fields just reset: their counters zeroed
            self._referee.call(env.state, env.dof_velocity_buf, self._setplay_views(), env.reset_buf)
            infos["referee"] = self._referee.verdict
        dones = env.reset_buf if self._dones is None else self._dones
        return {"obs": self._obs}, self._reward, dones, infos


class SingleAgent(_FusedWrapper):
    """Learner = blue robot 0; the other five robots follow OU noise (envs/wrappers.py:89-115)."""

    MODE = N.MODE_SA

    def __init__(self, env):
        super().__init__(env)
        self._action_space = Box(-1.0, 1.0, (env.num_actions,))
        self._observation_space = Box(-np.inf, np.inf, (env.num_obs,))
        self.act_view = self.action_buf[:, 0, 0, :]


class CMA(_FusedWrapper):
    """Centralised multi-agent: one 6-vector drives the blue team (envs/wrappers.py:118-148)."""

    MODE = N.MODE_CMA

    def __init__(self, env):
        super().__init__(env)
        self.num_envs = getattr(env, "num_envs", 1)
        self.device = env.device
        num_actions = env.num_actions * 3
        self._action_space = Box(-1.0, 1.0, (num_actions,))
        self._observation_space = Box(-np.inf, np.inf, (env.num_obs,))
        self.act_view = self.action_buf[:, 0, :, :].view(-1, num_actions)


class DMA(_FusedWrapper):
    """Decentralised multi-agent: each blue robot is one learner row (envs/wrappers.py:151-180)."""

    MODE = N.MODE_DMA
    ROWS_PER_FIELD = 3

    def __init__(self, env):
        setattr(env, "num_environments", getattr(env, "num_envs", 1) * 3)
        super().__init__(env)
        self._action_space = Box(-1.0, 1.0, (env.num_actions,))
        self._observation_space = Box(-np.inf, np.inf, (env.num_obs,))


class _ChannelTeam:
    """A policy team with a yellow channel in front of or behind it: a subclass's __call__ takes the team through
    the channel; everything else (check_env, observe, state, version ...) is the team's own."""
    _own = ("team", "channel")

    def __init__(self, team, channel):
        self.team, self.channel = team, channel

    def __getattr__(self, name):
        if name in self._own:  # not set yet (a copy under construction): no forwarding loop
            raise AttributeError(name)
        return getattr(self.team, name)


class _ChannelWrapper(Wrapper):
    """What Perceived, Tracked, Estimated and Actuated share: a `channel` over the learner's rows or commands, an
    `opponent_channel` (or None) over a policy opponent's, the inner wrapper's opponent buffers, and the checkpoint
    entries, labelled with the class's name."""

    @property
    def _opp_obs(self):
        return self.env._opp_obs

    @property
    def _opp_act(self):
        return self.env._opp_act

    def state_dict(self) -> dict:
        """The inner wrappers' state and the channels' (their device tensors and call counters), on the CPU."""
        out = {"inner": self.env.state_dict(), "channel": self.channel.state_dict()}
        if self.opponent_channel is not None:
            out["opponent_channel"] = self.opponent_channel.state_dict()
        return out

    def load_state_dict(self, state: dict) -> None:
        label = type(self).__name__
        self.env.load_state_dict(entry(state, "inner", label))
        self.channel.load_state_dict(entry(state, "channel", label))
        if self.opponent_channel is not None:
            self.opponent_channel.load_state_dict(entry(state, "opponent_channel", label))


class _PerceivedTeam(_ChannelTeam):
    """Behind the yellow perception channel: the team acts on the perceived opponent rows, whatever rows the step
    hands it."""

    def __call__(self, act, obs):
        self.team(act, self.channel.obs_out.view(obs.shape))


class Perceived(_ChannelWrapper):
    """Observation latency and vision noise round an SA / CMA / DMA or mirror wrapper (vss_amd/perceive.py,
    DESIGN.md §17): `obs` and info["terminal_observation"] become what an overhead camera would have delivered --
    `delay` steps late, Gaussian noise on every pose -- by one vss_perceive launch per step.  Rewards, dones and
    every other info pass through, and the step itself reads and writes the true rows.

    A policy opponent trained on perceived rows (--opponent self, pool or a checkpoint) acts on the output of a
    second channel over the versus step's opp_obs: the same seed and call index, so both teams see one world.
    The scripted team, zero and the kernel's OU process see the truth; info["opponent_obs"] stays true."""

    def __init__(self, env, delay: int, noise, seed: int):
        super().__init__(env)
        from vss_amd import perceive as P
        vss = env.env
        n = vss.num_fields
        mirror = isinstance(env, _MirrorWrapper)
        if mirror:
            layout, stride = P.layout_mirror(env.FIELD_ROWS, n), env.FIELD_ROWS
        elif env.ROWS_PER_FIELD == 3:
            layout, stride = P.layout_dma(), 3
        else:
            layout, stride = P.layout_sa(), 1
        self.delay, self.noise, self.seed = int(delay), P.Noise(*noise), int(seed)
        self.channel = P.PerceptionChannel(n, layout, self.delay, self.noise, self.seed, vss.device, done_stride=stride)
        self.opponent_channel = None
        self.channel.start(env._obs)  # as the inner wrapper's constructor computes its first observation

    def set_opponent(self, team=None, perceived=None):
        """The inner wrapper's set_opponent; `perceived` (default: a SnapshotOpponent or an OpponentPool, i.e.
        a policy that was trained on perceived rows) puts the yellow channel in front of the team."""
        from vss_amd import perceive as P
        from vss_amd.opponent import OpponentPool, SnapshotOpponent
        if perceived is None:
            perceived = isinstance(team, (SnapshotOpponent, OpponentPool))
        if team is None or not perceived:
            self.env.set_opponent(team)
            self.opponent_channel = None
            return
        vss = self.env.env
        ch = P.PerceptionChannel(vss.num_fields, P.layout_opponent(), self.delay, self.noise, self.seed, vss.device,
                                 done_stride=self.channel.done_stride)
        self.env.set_opponent(_PerceivedTeam(team, ch))
        self.opponent_channel = ch
        ch.start(self.env._opp_obs, call=max(self.channel.call - 1, 0))  # the learner's rows' last call: one world

    def reset(self, **kwargs):
        obs = self.env.reset(**kwargs)["obs"]
        if self.opponent_channel is not None:
            self.opponent_channel.start(self.env._opp_obs)
        return {"obs": self.channel.start(obs)}

    def step(self, action):
        obs, reward, dones, infos = self.env.step(action)
        p_obs, p_term = self.channel.perceive(obs["obs"], infos["terminal_observation"], dones)
        if self.opponent_channel is not None:
            # no terminal row on the yellow side: the true rows stand in and the second output is not used
            self.opponent_channel.perceive(self.env._opp_obs, self.env._opp_obs, dones)
        infos = dict(infos, terminal_observation=p_term)
        return {"obs": p_obs}, reward, dones, infos



class _TrackedTeam(_ChannelTeam):
    """Behind the yellow tracking channel: the team acts on the filtered opponent rows, whatever rows it is handed."""

    def __call__(self, act, obs):
        self.team(act, self.channel.obs_out.view(obs.shape))


class Tracked(_ChannelWrapper):
    """A recursive tracker round `Perceived` (vss_amd/track.py): `obs` and info["terminal_observation"]
    become the perceived rows filtered across frames -- the last filtered row moved one step with the project's own
    drive model, then corrected with the new row by a gain per kind of body behind a gate -- by one vss_track launch
    per step, in the delayed frame's own time.  Rewards, dones and every other info pass through.  It goes round
    Perceived and inside Estimated (filter, then dead-reckon to now) and Actuated.

    Where Perceived puts a second channel in front of a policy opponent, a second tracking channel goes behind it,
    exactly as Estimated's: it filters Perceived's opponent_channel.obs_out with the opponent layout, the same call
    index and the same dones, and the team acts on its output.  The mirror wrappers get one two-team channel."""

    def __init__(self, env, params):
        if not isinstance(env, Perceived):
            raise ValueError("Tracked goes round a Perceived wrapper: it filters what the perception channel delivers")
        if not env.noise.any():
            raise ValueError("Tracked goes round a Perceived wrapper with vision noise: with every sigma 0 there is "
                             "nothing to filter")
        super().__init__(env)
        from vss_amd import track as T
        self._base = env.env  # the SA / CMA / DMA or mirror wrapper
        vss = self._base.env
        self.delay, self.noise, self.params = env.delay, env.noise, T.Params(*params).check()
        self.channel = T.TrackingChannel(vss.num_fields, T.of_perception(env.channel.layout), self.delay, self.params,
                                         vss.device, done_stride=env.channel.done_stride)
        self.opponent_channel = None
        self.channel.start(env.channel.obs_out.view(self._base._obs.shape))  # as Perceived's constructor starts its own

    def _perceived_opponent_rows(self):
        return self.env.opponent_channel.obs_out.view(self.env._opp_obs.shape)

    def set_opponent(self, team=None, perceived=None):
        """Perceived's set_opponent; where that puts the yellow perception channel in front of the team (`perceived`,
        default: a SnapshotOpponent or an OpponentPool), the yellow tracking channel goes behind it."""
        from vss_amd import track as T
        from vss_amd.opponent import OpponentPool, SnapshotOpponent
        if perceived is None:
            perceived = isinstance(team, (SnapshotOpponent, OpponentPool))
        if team is None or not perceived:
            self.env.set_opponent(team, perceived=False)
            self.opponent_channel = None
            return
        vss = self._base.env
        ch = T.TrackingChannel(vss.num_fields, T.layout_opponent(), self.delay, self.params, vss.device,
                               done_stride=self.channel.done_stride)
        self.env.set_opponent(_TrackedTeam(team, ch), perceived=True)
        self.opponent_channel = ch
        ch.start(self._perceived_opponent_rows(), call=max(self.channel.call - 1, 0))  # the learner's rows' last call

    def reset(self, **kwargs):
        obs = self.env.reset(**kwargs)["obs"]
        if self.opponent_channel is not None:
            self.opponent_channel.start(self._perceived_opponent_rows())
        return {"obs": self.channel.start(obs)}

    def step(self, action):
        obs, reward, dones, infos = self.env.step(action)
        f_obs, f_term = self.channel.track(obs["obs"], infos["terminal_observation"], dones)
        if self.opponent_channel is not None:
            # no terminal row on the yellow side: the perceived rows stand in and the second output is not used
            rows = self._perceived_opponent_rows()
            self.opponent_channel.track(rows, rows, dones)
        infos = dict(infos, terminal_observation=f_term)
        return {"obs": f_obs}, reward, dones, infos



class _EstimatedTeam(_ChannelTeam):
    """Behind the yellow estimation channel: the team acts on the estimated opponent rows, whatever rows it is
    handed."""

    def __call__(self, act, obs):
        self.team(act, self.channel.obs_out.view(obs.shape))


class Estimated(_ChannelWrapper):
    """Dead reckoning round `Perceived` (vss_amd/estimate.py): `obs` and info["terminal_observation"]
    become the perceived rows rolled forward to the present -- by the rows' age, with the project's own drive model
    and the commands given in the meantime -- by one vss_estimate launch per step.  Rewards, dones and every other
    info pass through.  It goes round Perceived, or round Tracked(Perceived), and inside Actuated.

    Where Perceived puts a second channel in front of a policy opponent, a second estimation channel goes behind
    it: it estimates Perceived's opponent_channel.obs_out with the opponent layout, the same call index and the same
    dones, and the team acts on its output.  The mirror wrappers get one two-team channel."""

    def __init__(self, env):
        if not isinstance(env, (Perceived, Tracked)) or env.delay < 1:
            raise ValueError("Estimated goes round a Perceived wrapper with a delay of at least 1: without latency there "
                             "is nothing to predict")
        super().__init__(env)
        from vss_amd import estimate as E
        self._base = env._base if isinstance(env, Tracked) else env.env  # the SA / CMA / DMA or mirror wrapper
        vss = self._base.env
        self.delay = env.delay
        self.channel = E.EstimationChannel(vss.num_fields, E.of_perception(env.channel.layout), self.delay, vss.device,
                                           done_stride=env.channel.done_stride)
        self.opponent_channel = None
        self.channel.start(env.channel.obs_out.view(self._base._obs.shape))  # as Perceived's constructor starts its own

    def _perceived_opponent_rows(self):
        return self.env.opponent_channel.obs_out.view(self.env._opp_obs.shape)

    def set_opponent(self, team=None, perceived=None):
        """Perceived's set_opponent; where that puts the yellow perception channel in front of the team (`perceived`,
        default: a SnapshotOpponent or an OpponentPool), the yellow estimation channel goes behind it."""
        from vss_amd import estimate as E
        from vss_amd.opponent import OpponentPool, SnapshotOpponent
        if perceived is None:
            perceived = isinstance(team, (SnapshotOpponent, OpponentPool))
        if team is None or not perceived:
            self.env.set_opponent(team, perceived=False)
            self.opponent_channel = None
            return
        vss = self._base.env
        ch = E.EstimationChannel(vss.num_fields, E.layout_opponent(), self.delay, vss.device,
                                 done_stride=self.channel.done_stride)
        self.env.set_opponent(_EstimatedTeam(team, ch), perceived=True)
        self.opponent_channel = ch
        ch.start(self._perceived_opponent_rows(), call=max(self.channel.call - 1, 0))  # the learner's rows' last call

    def reset(self, **kwargs):
        obs = self.env.reset(**kwargs)["obs"]
        if self.opponent_channel is not None:
            self.opponent_channel.start(self._perceived_opponent_rows())
        return {"obs": self.channel.start(obs)}

    def step(self, action):
        obs, reward, dones, infos = self.env.step(action)
        e_obs, e_term = self.channel.estimate(obs["obs"], infos["terminal_observation"], dones)
        if self.opponent_channel is not None:
            # no terminal row on the yellow side: the perceived rows stand in and the second output is not used
            rows = self._perceived_opponent_rows()
            self.opponent_channel.estimate(rows, rows, dones)
        infos = dict(infos, terminal_observation=e_term)
        return {"obs": e_obs}, reward, dones, infos



class _ActuatedTeam(_ChannelTeam):
    """In front of the yellow actuation channel: what the team commands passes the channel in place before the step
    reads it."""
    _own = ("team", "channel", "dones")

    def __init__(self, team, channel, dones):
        self.team, self.channel, self.dones = team, channel, dones

    def __call__(self, act, obs):
        self.team(act, obs)
        self.channel.actuate(act, self.dones, out=act)


class Actuated(_ChannelWrapper):
    """Motor gain, command noise, quantisation, deadband and packet loss between the policy and the step
    (vss_amd/actuate.py): step(action) takes the learner's commands through one vss_actuate launch
    and steps the inner env with what the wheels apply.  `action` itself is not modified (the rollout keeps it for
    the log-prob); observations, rewards, dones and infos pass through.  The outermost env wrapper: outside
    Perceived when both are on.

    A policy opponent (--opponent self, pool or a checkpoint) commands through a second channel over the versus
    step's opp_act, in place: the same seed, call index and dones, yellow's entities -- one world.  The scripted
    team, zero and the kernel's OU process are not actuated.  The mirror wrappers get one two-team channel."""

    def __init__(self, env, params, seed: int):
        super().__init__(env)
        from vss_amd import actuate as A
        base = env
        while isinstance(base, (Perceived, Tracked, Estimated)):  # down to the SA / CMA / DMA or mirror wrapper
            base = base.env
        vss = base.env
        n = vss.num_fields
        if isinstance(base, _MirrorWrapper):
            robots = 3 if base.MODE in (N.MODE_CMA, N.MODE_DMA) else 1
            layout, stride, dones = A.layout_mirror(robots, n), base.FIELD_ROWS, base._dones
        else:
            layout = A.layout_sa() if base.MODE == N.MODE_SA else A.layout_team()
            stride = base.ROWS_PER_FIELD
            dones = vss.reset_buf if base._dones is None else base._dones
        self._base, self._dones_prev = base, dones  # the persistent buffer every step returns as its dones
        self.params, self.seed = A.Params(*params), int(seed)
        self.channel = A.ActuationChannel(n, layout, self.params, self.seed, vss.device, done_stride=stride)
        self.opponent_channel = None

    def set_opponent(self, team=None, actuated=None):
        """The inner wrapper's set_opponent; `actuated` (default: a SnapshotOpponent or an OpponentPool, i.e. a
        policy) puts the yellow channel behind the team."""
        from vss_amd import actuate as A
        from vss_amd.opponent import OpponentPool, SnapshotOpponent
        policy = isinstance(team, (SnapshotOpponent, OpponentPool))
        if actuated is None:
            actuated = policy
        perceived = {"perceived": policy} if isinstance(self.env, (Perceived, Tracked, Estimated)) else {}  # its isinstance sees the team
        if team is None or not actuated:
            self.env.set_opponent(team, **perceived)
            self.opponent_channel = None
            return
        vss = self._base.env
        ch = A.ActuationChannel(vss.num_fields, A.layout_opponent(), self.params, self.seed, vss.device,
                                done_stride=self.channel.done_stride)
        ch.start(call=self.channel.call)  # the learner's channel's next call: one world
        self.env.set_opponent(_ActuatedTeam(team, ch, self._dones_prev), **perceived)
        self.opponent_channel = ch

    def reset(self, **kwargs):
        obs = self.env.reset(**kwargs)
        self.channel.start(call=0, zero=True)
        if self.opponent_channel is not None:
            self.opponent_channel.start(call=0, zero=True)
        return obs

    def step(self, action):
        return self.env.step(self.channel.actuate(action, self._dones_prev))



class _MirrorWrapper(Wrapper):
    """Two-sided self-play (vss_step_mirror): both teams' robots are learner rows of one step.

    Rows are team-major: rows [0, R N) are exactly the plain wrapper's rows (the blue team's), rows
    [R N, 2 R N) the yellow team's in the same order, seen from the yellow side (observations
    team-relative, goal and grad rewards sign-flipped).  Every output is one tensor whose halves
    the kernel writes as the blue and the yellow block.  SA keeps the OU process for robots 1-2 of
    both teams; CMA and DMA have no OU robot left."""

    MODE = None
    FIELD_ROWS = 1      # R: learner rows per field and team
    ROWS_PER_FIELD = 2  # learner rows per field

    def __init__(self, env: VSS):
        super().__init__(env)
        setattr(env, "num_environments", env.num_fields * self.ROWS_PER_FIELD)
        self.action_buf = env.dof_velocity_buf.clone()  # (N,2,3,2): the twelve applied actions (SA: OU state)
        dev = env.device
        rows = env.num_fields * self.ROWS_PER_FIELD
        self._obs = torch.zeros((rows, env.num_obs), device=dev)
        self._terminal_obs = torch.zeros_like(self._obs)
        self._rews = torch.zeros((rows, 4), device=dev)
        self._reward = torch.zeros(rows, device=dev)
        self._time_outs = torch.zeros(rows, dtype=torch.bool, device=dev)
        self._progress = torch.zeros(rows, device=dev)
        self._dones = torch.zeros(rows, dtype=torch.long, device=dev)
        # the halves of each output: the blue team's block (vss_step_io) and the yellow team's (vss_mirror_io)
        h = rows // 2
        blue, yellow = (lambda t: t[:h]), (lambda t: t[h:])
        self._io = dict(ou_buf=self.action_buf, obs=blue(self._obs), terminal_obs=blue(self._terminal_obs),
                        rew=blue(self._rews), reward_sum=blue(self._reward), dones_rep=blue(self._dones),
                        time_outs=blue(self._time_outs), progress_f=blue(self._progress))
        self._yl = dict(obs=yellow(self._obs), terminal_obs=yellow(self._terminal_obs), rew=yellow(self._rews),
                        reward_sum=yellow(self._reward), dones=yellow(self._dones), time_outs=yellow(self._time_outs),
                        progress_f=yellow(self._progress))
        self._setplays = None  # vss_amd.setplay.Stager (set_setplays)
        self._referee = None  # vss_amd.referee.Referee (set_referee)
        self._first_obs()

    def _setplay_views(self):
        from vss_amd import setplay as S
        return [(self._obs, S.view_mirror(self.FIELD_ROWS, self.env.num_fields))]

    def set_setplays(self, stager=None):
        """As _FusedWrapper.set_setplays: both team blocks are one two-team view."""
        self._setplays = stager
        if stager is not None:
            stager.start(self.env.state, self._setplay_views())

    def set_referee(self, ref=None):
        """As _FusedWrapper.set_referee: both team blocks are one two-team view."""
        self._referee = ref

    def referee_record(self, rec: dict, writer=None, step: int = 0) -> None:
        _referee_record(self._referee, rec, writer, step)

    def _first_obs(self):
        env, R = self.env, self.FIELD_ROWS
        full = torch.empty((env.num_fields, 2, 3, env.num_obs), device=env.device)
        env.compute_observations(full, n_agents=6)
        self._obs.view(2, env.num_fields, R, env.num_obs).copy_(full[:, :, :R].transpose(0, 1))
        return {"obs": self._obs}

    def set_opponent(self, team=None):
        raise ValueError("a mirror wrapper has no opponent: both teams are the learner's rows")

    def _state_tensors(self) -> dict:
        return dict(action_buf=self.action_buf, obs=self._obs, terminal_obs=self._terminal_obs, rews=self._rews,
                    reward=self._reward, dones=self._dones, time_outs=self._time_outs, progress=self._progress)

    def state_dict(self) -> dict:
        """The full-row tensors on the CPU (vss_amd.checkpoint); the `_io` / `_yl` halves are views of them."""
        out = to_cpu(self._state_tensors())
        if self._setplays is not None:
            out["setplays"] = self._setplays.state_dict()
        if self._referee is not None:
            out["referee"] = self._referee.state_dict()
        return out

    def load_state_dict(self, state: dict) -> None:
        copy_entries(type(self).__name__, self._state_tensors(), state)
        if self._setplays is not None:
            self._setplays.load_state_dict(entry(state, "setplays", type(self).__name__))
        if self._referee is not None:
            self._referee.load_state_dict(entry(state, "referee", type(self).__name__))

    def reset(self, **kwargs):
        self.env.reset(**kwargs)
        return self._first_obs()

    def step(self, action):
        self.env.native_step_mirror(self.MODE, action, self._io, self._yl)
        if self._setplays is not None:
            self._setplays.stage(self.env.state, self._setplay_views(), self.env.reset_buf)
        infos = {"rews": self._rews, "terminal_observation": self._terminal_obs, "time_outs": self._time_outs,
                 "progress_buffer": self._progress}
        if self._referee is not None:
            self._referee.call(self.env.state, self.env.dof_velocity_buf, self._setplay_views(), self.env.reset_buf)
            infos["referee"] = self._referee.verdict
        return {"obs": self._obs}, self._reward, self._dones, infos


class MirrorSingleAgent(_MirrorWrapper):
    """Learners = blue robot 0 and yellow robot 0; the other four robots follow OU noise."""

    MODE = N.MODE_SA

    def __init__(self, env):
        super().__init__(env)
        self._action_space = Box(-1.0, 1.0, (env.num_actions,))
        self._observation_space = Box(-np.inf, np.inf, (env.num_obs,))


class MirrorCMA(_MirrorWrapper):
    """Centralised multi-agent on both sides: one 6-vector per team and field."""

    MODE = N.MODE_CMA

    def __init__(self, env):
        super().__init__(env)
        self._action_space = Box(-1.0, 1.0, (env.num_actions * 3,))
        self._observation_space = Box(-np.inf, np.inf, (env.num_obs,))


class MirrorDMA(_MirrorWrapper):
    """Decentralised multi-agent on both sides: each of the six robots is one learner row."""

    MODE = N.MODE_DMA
    FIELD_ROWS = 3
    ROWS_PER_FIELD = 6

    def __init__(self, env):
        super().__init__(env)
        self._action_space = Box(-1.0, 1.0, (env.num_actions,))
        self._observation_space = Box(-np.inf, np.inf, (env.num_obs,))
