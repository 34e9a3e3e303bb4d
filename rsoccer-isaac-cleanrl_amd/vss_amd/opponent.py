"""Policy opponents for the fused step (envs/wrappers.py `set_opponent`, include/vss.h `vss_step_versus`).

An opponent follows play.py's Team protocol: `team(act, obs)` writes the yellow team's (N,3,2) actions
into `act` in place from its (N,3,52) observations, so play.py's TeamZero / TeamOU / TeamDMA / TeamCMA
work as opponents unchanged.  `OpponentPool` (below) is the league: several past snapshots at once, each on
its own slice of the fields.  `SnapshotOpponent` is the self-play one: a frozen copy of an Agent's
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

import ctypes
import math
import random

import torch

from . import _native as N
from . import policy as _policy
from .checkpoint import copy_entries, copy_into, entry, python_rng_state, python_rng_tuple, to_cpu
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

    def state_dict(self) -> dict:
        """The frozen actor's weights, their label and the policy's Philox counter (vss_amd.checkpoint)."""
        return {"actor": to_cpu(dict(self.actor.state_dict())), "version": int(self.version),
                "policy": self.policy.state_dict()}

    def load_state_dict(self, state: dict) -> None:
        copy_entries("SnapshotOpponent.actor", dict(self.actor.state_dict()), entry(state, "actor", "SnapshotOpponent"))
        self.policy.refresh()
        self.version = int(entry(state, "version", "SnapshotOpponent"))
        self.policy.load_state_dict(entry(state, "policy", "SnapshotOpponent"))

    @torch.no_grad()
    def __call__(self, act, obs):
        n = obs.shape[0]
        rows = obs.reshape(n * 3, 52) if self.kind == "x3" else obs[:, 0, :]
        if act.is_contiguous() and act.dtype == torch.float32:
            self.policy.act(rows, out=act)  # (N,3,2) = 3N rows of 2, or N rows of 6
        else:
            act.copy_(self.policy.act(rows).view(n, 3, 2))


def pfsp_weights(totals, power: float = 1.0) -> list:
    """Prioritised fictitious self-play: the weight of each snapshot from the learner's results against it,
    (1 - w) ** power with w = (wins + 0.5 draws) / episodes (0.5 where nothing was played); all equal when
    every one of them is 0.  totals: rows of
    [episodes, wins, losses, steps] (lists or a CPU tensor).  Plain host arithmetic."""
    if hasattr(totals, "tolist"):
        totals = totals.tolist()
    out = []
    for row in totals:
        episodes, wins, losses = float(row[0]), float(row[1]), float(row[2])
        w = 0.5 if episodes <= 0 else (wins + 0.5 * (episodes - wins - losses)) / episodes
        out.append(max(0.0, 1.0 - w) ** power)
    return out if any(v > 0 for v in out) else [1.0] * len(out)  # everything won: a uniform draw


def pool_slots(n_fields: int, slots: int, rows_per_field: int):
    """(group_fields, count): the fields cut into at most `slots` slices of whole 64-field blocks (whole
    256-field blocks once the opponent rows reach the GEMM chain, whose row tiles are 256)."""
    if n_fields < 1 or not 1 <= slots <= N.MAX_ACTOR_GROUPS:
        raise ValueError(f"a pool needs n_fields >= 1 and 1 <= slots <= {N.MAX_ACTOR_GROUPS}, got {n_fields}, {slots}")
    chain = _policy.ROLLOUT_POLICY == "chain" and n_fields * rows_per_field >= _policy.CHAIN_MIN_ROWS
    block = 256 if chain else 64
    per_slot = -(-n_fields // slots)
    group_fields = -(-per_slot // block) * block
    return group_fields, -(-n_fields // group_fields)


class _Snapshot:
    """One frozen actor: its own storage, packed weights and bf16 planes (an actor-only FusedPolicy)."""

    def __init__(self, agent, version: int):
        self.actor = _Actor(_clone_mlp(agent.actor_mean), agent.actor_logstd.detach().clone())
        self.actor.requires_grad_(False)
        self.actor.eval()
        self.policy = FusedPolicy(self.actor, actor_only=True)
        self.logstd = self.actor.actor_logstd.detach().reshape(-1).contiguous()
        self.version = int(version)
        self.totals = [0, 0, 0, 0]  # the learner against this snapshot: episodes, wins, losses, steps

    def mean_chain(self, rows):
        return self.policy._chain(self.actor.actor_mean, rows)


class OpponentPool:
    """A league of past snapshots on the yellow team (play.py's Team protocol, like SnapshotOpponent).

    The fields are cut into `count` slots of `group_fields` fields; `assign()` gives each slot a snapshot:
    the first max(1, round(latest * count)) slots the newest, every other slot a draw with replacement by
    pfsp_weights.  All slots are evaluated in one launch (vss_actor_forward_grouped; at chain sizes a GEMM
    chain per run of slots with the same snapshot + one vss_policy_sample_grouped), the results of finished
    episodes are counted per slot on the device (observe: vss_match_tally) and read once per update
    (end_update).  Host-side draws come from a random.Random of the pool's own."""

    def __init__(self, agent, kind: str, n_fields: int, slots: int = 8, capacity: int = 16, latest: float = 0.5,
                 pfsp_power: float = 1.0, seed: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
        n_act = int(agent.actor_logstd.shape[-1])
        if n_act != KINDS[kind]:
            raise ValueError(f"a {kind!r} opponent needs a {KINDS[kind]}-action Agent, got {n_act} actions")
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.kind, self.n_act = kind, n_act
        self.n_fields = int(n_fields)
        self.rows_per_field = 3 if kind == "x3" else 1
        self.group_fields, self.count = pool_slots(self.n_fields, int(slots), self.rows_per_field)
        self.group_rows = self.group_fields * self.rows_per_field
        self.rows = self.n_fields * self.rows_per_field
        self.capacity, self.latest, self.pfsp_power = int(capacity), float(latest), float(pfsp_power)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counter = 0  # one Philox counter per call, as FusedPolicy.act
        self.rng = random.Random(seed)
        self.device = N.require_device(next(agent.parameters()).device)
        self.tally = torch.zeros((self.count, 4), dtype=torch.long, device=self.device)
        self.snapshots = []
        self.add(agent, 0)
        self.assign()

    @property
    def version(self) -> int:
        """The newest snapshot's label."""
        return self.snapshots[-1].version

    @property
    def versions(self) -> list:
        """The label of the snapshot in each slot."""
        return [s.version for s in self.slot_snapshots]

    def add(self, agent, version: int):
        """Append a frozen copy of the agent's actor; a full pool drops its oldest snapshot.  Slots keep the
        snapshot objects they hold until the next assign()."""
        self.snapshots.append(_Snapshot(agent, version))
        if len(self.snapshots) > self.capacity:
            del self.snapshots[0]
        return self

    def assign(self):
        """Deal the slots: the first max(1, round(latest * count)) the newest snapshot, each other one a draw
        by pfsp_weights.  Returns the versions per slot."""
        n_latest = max(1, round(self.latest * self.count))
        held = [self.snapshots[-1]] * min(n_latest, self.count)
        if len(held) < self.count:
            weights = pfsp_weights([s.totals for s in self.snapshots], self.pfsp_power)
            held += self.rng.choices(self.snapshots, weights=weights, k=self.count - len(held))
        return self.hold(held)

    def hold(self, held):
        """Put the given snapshots (one per slot, members of self.snapshots) into the slots."""
        held = list(held)
        if len(held) != self.count or any(s not in self.snapshots for s in held):
            raise ValueError(f"hold() takes {self.count} snapshots of this pool")
        self.slot_snapshots = held
        g = N.VssActorGroups()
        g.count, g.group_rows = self.count, self.group_rows
        for i, s in enumerate(held):
            g.actor_packed[i] = s.policy._actor.data_ptr()
            g.logstd[i] = s.logstd.data_ptr()
        self._groups = g
        return self.versions

    def state_dict(self) -> dict:
        """The whole league (vss_amd.checkpoint): every snapshot's actor weights (log-std among them), label and
        totals in order, the snapshot of each slot as an index into that list, the Philox counter, the host
        generator's state and the device tally.  Taken at an update boundary, after end_update() has dealt the
        slots, every slot holds a member of the list."""
        if any(s not in self.snapshots for s in self.slot_snapshots):
            raise ValueError("OpponentPool.state_dict: a slot holds an evicted snapshot; call it after assign()")
        return {"snapshots": [{"actor": to_cpu(dict(s.actor.state_dict())), "version": int(s.version),
                               "totals": [int(v) for v in s.totals]} for s in self.snapshots],
                "slots": [self.snapshots.index(s) for s in self.slot_snapshots],
                "counter": int(self.counter), "rng": python_rng_state(self.rng.getstate()), "tally": to_cpu(self.tally)}

    def load_state_dict(self, state: dict) -> None:
        """Rebuild the league from a state_dict(): the snapshots on storage of this pool's own, the slots put
        back through hold(), so the kernel's group table points at the live packed weights."""
        saved = entry(state, "snapshots", "OpponentPool")
        slots = [int(i) for i in entry(state, "slots", "OpponentPool")]
        if not 1 <= len(saved) <= self.capacity:
            raise ValueError(f"OpponentPool.snapshots: {len(saved)} saved snapshots, this pool keeps 1 to {self.capacity}")
        if len(slots) != self.count or any(not 0 <= i < len(saved) for i in slots):
            raise ValueError(f"OpponentPool.slots: {slots} does not deal {self.count} slots among {len(saved)} snapshots")
        copy_into(self.tally, entry(state, "tally", "OpponentPool"), "OpponentPool.tally")
        snapshots = []
        for i, sv in enumerate(saved):
            s = self.snapshots[i] if i < len(self.snapshots) else _Snapshot(self.snapshots[0].actor, 0)
            copy_entries(f"OpponentPool.snapshots[{i}].actor", dict(s.actor.state_dict()), entry(sv, "actor", "snapshot"))
            s.policy.refresh()
            s.version = int(entry(sv, "version", "snapshot"))
            totals = [int(v) for v in entry(sv, "totals", "snapshot")]
            if len(totals) != 4:
                raise ValueError(f"OpponentPool.snapshots[{i}].totals: expected 4 counts, got {totals}")
            s.totals = totals
            snapshots.append(s)
        self.snapshots = snapshots
        self.hold([snapshots[i] for i in slots])
        self.counter = int(entry(state, "counter", "OpponentPool"))
        self.rng.setstate(python_rng_tuple(entry(state, "rng", "OpponentPool")))

    def check_env(self, env):
        """Win and loss are read from the sign of the goal reward: that needs a positive goal weight."""
        if float(env.w_goal) <= 0:
            raise ValueError(f"an opponent pool counts wins by the goal reward's sign: w_goal must be > 0, got {env.w_goal}")
        if int(env.num_fields) != self.n_fields:
            raise ValueError(f"the pool was built for {self.n_fields} fields, the env has {env.num_fields}")

    def chain_active(self) -> bool:
        return _policy.ROLLOUT_POLICY == "chain" and self.rows >= _policy.CHAIN_MIN_ROWS

    @torch.no_grad()
    def means_chain(self, rows):
        """(rows, n_act) actor means, each slot's rows by the snapshot it holds: one GEMM chain per run of
        adjacent slots with the same snapshot (slot boundaries are whole 256-row tiles, so a row's mean
        does not depend on how many slots share the call)."""
        mean = torch.empty((self.rows, self.n_act), device=self.device)
        q = 0
        while q < self.count:
            e = q + 1
            while e < self.count and self.slot_snapshots[e] is self.slot_snapshots[q]:
                e += 1
            lo, hi = q * self.group_rows, min(self.rows, e * self.group_rows)
            mean[lo:hi] = self.slot_snapshots[q].mean_chain(rows[lo:hi])
            q = e
        return mean

    @torch.no_grad()
    def __call__(self, act, obs):
        n = obs.shape[0]
        if n != self.n_fields:
            raise ValueError(f"the pool was built for {self.n_fields} fields, got observations of {n}")
        rows = obs.reshape(n * 3, 52) if self.kind == "x3" else obs[:, 0, :]
        if rows.dtype != torch.float32 or not rows.is_contiguous() or rows.device != self.device:
            rows = rows.to(self.device, torch.float32).contiguous()
        direct = act.is_contiguous() and act.dtype == torch.float32 and act.device == self.device
        out = act if direct else torch.empty((self.rows, self.n_act), device=self.device)
        self.counter += 1
        lib, stream = N.load(), N.stream_of(self.device)
        if self.chain_active():
            mean = self.means_chain(rows)
            N.check(lib.vss_policy_sample_grouped(stream, self.rows, self.n_act, mean.data_ptr(), ctypes.byref(self._groups),
                                                  self.seed, self.counter, out.data_ptr()), "vss_policy_sample_grouped")
        else:
            N.check(lib.vss_actor_forward_grouped(stream, self.rows, self.n_act, rows.data_ptr(), ctypes.byref(self._groups),
                                                  self.seed, self.counter, out.data_ptr(), None),
                    "vss_actor_forward_grouped")
        if not direct:
            act.copy_(out.view(n, 3, 2))

    def observe(self, rews, dones, progress_f):
        """After a versus step: count the finished fields' results per slot (one launch, no host sync).
        rews (R, 4), dones (R,) int64, progress_f (R,) of the learner's R = n_fields or 3 n_fields rows."""
        rpf = dones.numel() // self.n_fields
        if (dones.numel() != rpf * self.n_fields or rews.shape != (dones.numel(), 4) or progress_f.numel() != dones.numel()
                or rews.dtype != torch.float32 or dones.dtype != torch.long or progress_f.dtype != torch.float32
                or not (rews.is_contiguous() and dones.is_contiguous() and progress_f.is_contiguous())):
            raise ValueError("observe expects rews (R, 4) float32, dones (R,) int64 and progress_f (R,) float32, contiguous")
        N.check(N.load().vss_match_tally(N.stream_of(self.device), self.n_fields, rpf, self.group_fields, self.count,
                                         rews.data_ptr(), dones.data_ptr(), progress_f.data_ptr(), self.tally.data_ptr()),
                "vss_match_tally")

    def end_update(self, agent, update: int, every: int) -> dict:
        """Once per PPO update: read the device tally (one host read), credit each slot's results to the
        snapshot it held, zero the tally, add a snapshot of `agent` on every `every`-th update, and deal the
        slots again.  Returns the new assignment and the win rate of the update just played, per slot."""
        tally = self.tally.tolist()
        self.tally.zero_()
        winrate = []
        for s, (episodes, wins, losses, steps) in zip(self.slot_snapshots, tally):
            for i, v in enumerate((episodes, wins, losses, steps)):
                s.totals[i] += v
            winrate.append((wins + 0.5 * (episodes - wins - losses)) / episodes if episodes > 0 else math.nan)
        if every > 0 and update % every == 0:
            self.add(agent, update)
        return {"versions": self.assign(), "winrate": winrate}


def make_opponent(args, agent, fused_env, n_fields: int, seed: int):
    """The train loop's yellow team for args.opponent, set on the wrapper (set_opponent); None for 'ou' (the
    kernel's OU process stays) and 'mirror' (both teams' robots are learner rows: no snapshot, no sync, no
    opponent forward).  `seed`: the Philox seed of the opponent's own stream.  With args.kernel_warmup a policy
    opponent runs one forward at this run's own row count outside the clock (under 16,384 opponent rows it is
    the actor-only fused kernel, which the 16,384-env warm-up run does not reach); its Philox counter is put
    back, so the training's draws do not change."""
    mode = getattr(args, "opponent", "ou")
    if mode in ("ou", "mirror"):
        return None
    if mode == "scripted":
        # the scripted benchmark team: a pure function of the yellow observations, one launch per step -- no
        # snapshot, no sync, no warm-up forward; its state dict holds the controller's version alone
        from play import TeamScripted
        opponent = TeamScripted()
        fused_env.set_opponent(opponent)
        return opponent
    if mode == "pool":
        # a league of past snapshots, each on its slice of this rank's fields; the match tallies -- and so the
        # assignments -- are per rank
        opponent = OpponentPool(agent, KIND_OF_ENV[args.env_id], n_fields, slots=getattr(args, "opponent_pool_slots", 8),
                                capacity=getattr(args, "opponent_pool_size", 16),
                                latest=getattr(args, "opponent_pool_latest", 0.5),
                                pfsp_power=getattr(args, "opponent_pfsp_power", 1.0), seed=seed)
        counted = opponent
    else:
        opponent = SnapshotOpponent(agent, KIND_OF_ENV[args.env_id], seed=seed)
        if mode != "self":
            opponent.load(mode)
        counted = opponent.policy
    fused_env.set_opponent(opponent)
    if getattr(args, "kernel_warmup", False):
        counter = counted.counter
        opponent(torch.zeros_like(fused_env._opp_act), fused_env._opp_obs)
        counted.counter = counter
    return opponent
