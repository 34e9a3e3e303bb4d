"""Policy opponents for the fused step (envs/wrappers.py `set_opponent`, include/vss.h `vss_step_versus`).

An opponent follows play.py's Team protocol: `team(act, obs)` writes the yellow team's (N,3,2) actions
into `act` in place from its (N,3,52) observations, so play.py's TeamZero / TeamOU / TeamDMA / TeamCMA
work as opponents unchanged.  `SnapshotOpponent` is the self-play one: a frozen copy of an Agent's
actor, evaluated by its own FusedPolicy (actor only -- no critic is stored, packed or evaluated):

    opp = SnapshotOpponent(agent, kind="x3", seed=...)    # the weights as they are now
    env.set_opponent(opp)
    opp.sync(agent)                                       # later: follow the learner
    opp.load("runs/.../agent.pt")                         # or: a fixed checkpoint (reference format)

kind "x3": a 2-action policy applied to each yellow robot's own observation, 3N rows (the reference's
'ppo-sa-x3' / 'ppo-dma' team, play.py:62-64); kind "cma": a 6-action policy on yellow robot 0's
observation (play.py:57-59).  The yellow observations are mirrored by the env, so a policy trained as
blue plays yellow as is.
"""
from __future__ import annotations

import torch

from .policy import FusedPolicy

KINDS = {"x3": 2, "cma": 6}  # kind -> the policy's action width
KIND_OF_ENV = {"sa": "x3", "dma": "x3", "cma": "cma"}  # --env-id -> the team its Agent makes


@torch.no_grad()
def _clone_mlp(seq):
    """A Sequential of the same layers on fresh storage (the Agent's parameters may be views of one
    flat buffer, vss_amd.flat.FlatGrads: the copy must not share or drag along that buffer)."""
    out = []
    for m in seq:
        if isinstance(m, torch.nn.Linear):
            lin = torch.nn.Linear(m.in_features, m.out_features, device=m.weight.device, dtype=m.weight.dtype)
            lin.weight.copy_(m.weight)
            lin.bias.copy_(m.bias)
            out.append(lin)
        else:
            out.append(type(m)())
    return torch.nn.Sequential(*out)


class _Actor(torch.nn.Module):
    """The actor half of an Agent (same parameter names as its state dict)."""

    def __init__(self, actor_mean, actor_logstd):
        super().__init__()
        self.actor_mean = actor_mean
        self.actor_logstd = torch.nn.Parameter(actor_logstd, requires_grad=False)


class SnapshotOpponent:
    def __init__(self, agent, kind: str = "x3", seed: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
        n_act = int(agent.actor_logstd.shape[-1])
        if n_act != KINDS[kind]:
            raise ValueError(f"a {kind!r} opponent needs a {KINDS[kind]}-action Agent, got {n_act} actions")
        self.kind = kind
        self.actor = _Actor(_clone_mlp(agent.actor_mean), agent.actor_logstd.detach().clone())
        self.actor.requires_grad_(False)
        self.actor.eval()
        # a Philox stream of its own: the caller passes a seed distinct from the learner's FusedPolicy
        self.policy = FusedPolicy(self.actor, seed=seed, actor_only=True)
        self.version = 0  # the caller's label of the weights in use (the train loop: the update index)

    @torch.no_grad()
    def _set(self, state: dict):
        own = self.actor.state_dict()
        for k, dst in own.items():
            src = state[k]
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"{k}: shape {tuple(src.shape)} does not fit the opponent's {tuple(dst.shape)}")
            dst.copy_(src)
        self.policy.refresh()  # packed weights and the chain's bf16 planes

    def sync(self, agent, version: int | None = None):
        """Copy the agent's current actor weights into the snapshot (a local device copy)."""
        self._set({k: v for k, v in agent.state_dict().items() if not k.startswith("critic.")})
        if version is not None:
            self.version = int(version)
        return self

    def load(self, path: str, version: int | None = None):
        """The actor of a checkpoint in the reference's format (torch.save(agent.state_dict()))."""
        self._set(torch.load(path, map_location=self.policy.device, weights_only=True))
        if version is not None:
            self.version = int(version)
        return self

    @torch.no_grad()
    def __call__(self, act, obs):
        n = obs.shape[0]
        rows = obs.reshape(n * 3, 52) if self.kind == "x3" else obs[:, 0, :]
        if act.is_contiguous() and act.dtype == torch.float32:
            self.policy.act(rows, out=act)  # (N,3,2) = 3N rows of 2, or N rows of 6
        else:
            act.copy_(self.policy.act(rows).view(n, 3, 2))
