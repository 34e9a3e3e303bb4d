"""`--eval-every K`: the live agent against fixed yellow teams during training.

Every K-th update rank 0 plays the agent as it is on a second, separate env of `--eval-fields` fields, wrapped
as the run's own `--env-id` (SA / CMA / DMA; never a mirror wrapper), with goal-only rewards, against each team
of `--eval-teams`: 'ou' is the wrapper's plain step (the kernel's OU process), 'zero' and 'scripted' are play.py
teams inside the fused step (set_opponent).  Blue samples its actions as training does, through a FusedPolicy
of the arena's own over the same Agent.

Counting is unbiased.  For each team every field is reset, `max_episode_length` steps run, and only each
field's FIRST episode counts: `first = done & ~seen; seen |= done`, and `first` goes to vss_match_tally as one
group.  Every field finishes by time-out at the latest, so exactly `--eval-fields` episodes are counted per
team and an episode's chance to be counted does not depend on its length (play_matches' "first n_matches
episodes to finish" favours short ones).  Nothing reads the device until the team's tally is read once.

An evaluation is a pure function of (weights, --seed, update): before each team's run the env's rng_counter is
zeroed and the policy's Philox counter is set from the update number.  So the arena owns no state a checkpoint
must carry -- a resumed run reports the evaluations of the unbroken one -- and it touches nothing of the
training: not its env, not its policy's counter, not torch's generators (forked around the run).

`--eval-setplays a,b` (vss_amd/setplay.py): for each team and each named play every field's first episode also starts
from that play -- after reset_dones() a stager of the arena's own (a key of its own, its call index set from the update
number) stages every field with it (`only=`) -- and is recorded as "<team>@<play>".  Later episodes of a field start
from the uniform drop and are not counted.

`--ref-*` (vss_amd/referee.py): when the training has a referee the arena's wrapper has one of its own with the same
table and parameters (key offset 1, its counters zeroed and its call index set from the policy counter before every
play), so an evaluation scores the game that is being trained and stays a pure function of (weights, seed, update);
each result then carries "stoppages", the eight verdict counts of the play.
"""
from __future__ import annotations

import time

import torch

from . import _native as N

TEAMS = ("zero", "ou", "scripted")


def parse_teams(spec) -> list:
    """--eval-teams as a list: comma separated names out of TEAMS, each once, at least one."""
    names = [t.strip() for t in str(spec).split(",") if t.strip()]
    bad = [t for t in names if t not in TEAMS]
    if bad or not names or len(set(names)) != len(names):
        raise ValueError(f"--eval-teams takes distinct names out of {', '.join(TEAMS)}, comma separated; got {spec!r}")
    return names


def parse_setplays(spec) -> list:
    """--eval-setplays as a list of distinct play names (vss_amd/setplay.py named_play checks them); empty: none."""
    names = [t.strip() for t in str(spec or "").split(",") if t.strip()]
    if len(set(names)) != len(names):
        raise ValueError(f"--eval-setplays takes distinct play names, comma separated; got {spec!r}")
    return names


def score(wins: int, losses: int, episodes: int) -> float:
    return (wins - losses) / episodes if episodes > 0 else 0.0


class Arena:
    def __init__(self, args, agent, device):
        from envs.vss import VSS, default_cfg
        from envs.wrappers import CMA, DMA, SingleAgent
        from play import get_team
        from .policy import FusedPolicy
        self.device = N.require_device(device)
        self.teams = parse_teams(getattr(args, "eval_teams", ",".join(TEAMS)))
        n = int(getattr(args, "eval_fields", 1024))
        if n < 1:
            raise ValueError(f"--eval-fields must be at least 1, got {n}")
        if args.env_id not in ("sa", "cma", "dma"):
            raise ValueError(f"--eval-every needs --env-id sa, cma or dma, got {args.env_id!r}")
        cfg = default_cfg(n)
        cfg["env"]["seed"] = int(args.seed) * 1000003 + 500009  # a Philox key of its own (training: seed * 1000003 + rank)
        with torch.random.fork_rng(devices=[self.device]):
            env = VSS(cfg=cfg, rl_device=str(self.device), sim_device=str(self.device), graphics_device_id=0, headless=True,
                      virtual_screen_capture=False, force_render=False)
            env.w_goal, env.w_grad, env.w_move, env.w_energy = 1.0, 0.0, 0.0, 0.0  # as evaluate() sets them
            self.env = env
            self.wrapper = {"sa": SingleAgent, "cma": CMA, "dma": DMA}[args.env_id](env)
            from .referee import referee_of_args
            self.referee = referee_of_args(args, n, self.device, 1)  # None without --ref-*
            if self.referee is not None:
                self.wrapper.set_referee(self.referee)
            # --obs-delay / --obs-noise-*: blue sees perceived rows as in training, through a channel of the arena's
            # own (a key of its own); reset() starts it afresh at call 0 in every play, so it carries no state over
            from envs.wrappers import Perceived, perception_args, perception_seed
            delay, noise = perception_args(args)
            if delay or noise.any():
                self.wrapper = Perceived(self.wrapper, delay, noise, perception_seed(args.seed, 1))
            # --obs-filter-*: the perceived rows filtered across frames, as in training; reset() starts the channel afresh
            from envs.wrappers import Tracked, tracking_args
            if tracking_args(args).any():
                self.wrapper = Tracked(self.wrapper, tracking_args(args))
            # --obs-predict 1: the perceived rows rolled forward, as in training; reset() starts the channel afresh
            from envs.wrappers import Estimated, estimation_args
            if estimation_args(args):
                self.wrapper = Estimated(self.wrapper)
            # --act-*: blue's commands pass a channel of the arena's own; reset() starts it afresh (state zeroed, call 0)
            from envs.wrappers import Actuated, actuation_args, actuation_seed
            params = actuation_args(args)
            if params.any():
                self.wrapper = Actuated(self.wrapper, params, actuation_seed(args.seed, 1))
            self.policy = FusedPolicy(agent, seed=int(args.seed) * 7919 + 15485863, actor_only=True)
        self.opponents = {t: (None if t == "ou" else get_team(t)) for t in self.teams}
        self.setplays, self.stager = parse_setplays(getattr(args, "eval_setplays", "")), None
        if self.setplays:
            from . import setplay as S
            library = dict(S.BUILTIN, **(S.load_file(args.setplay_file) if getattr(args, "setplay_file", None) else {}))
            table = S.Table([S.named_play(name, library) for name in self.setplays], 1.0)
            self.stager = S.Stager(n, table, S.setplay_seed(args.seed, 1), self.device)
        self.n_fields = n
        self.rows_per_field = self.wrapper.ROWS_PER_FIELD
        rows = n * self.rows_per_field
        self.seen = torch.zeros(rows, dtype=torch.long, device=self.device)
        self.first = torch.zeros(rows, dtype=torch.long, device=self.device)
        self.tally = torch.zeros((1, 4), dtype=torch.long, device=self.device)
        self.steps = int(env.max_episode_length)

    @torch.no_grad()
    def play(self, team: str, counter: int, setplay: int | None = None) -> dict:
        """Every field's first episode against `team`, the policy's Philox counter starting above `counter`;
        `setplay`: the index in --eval-setplays of the play every field starts from (None: the uniform drop)."""
        env, w, lib = self.env, self.wrapper, N.load()
        env.rng_counter.zero_()
        env.reset_buf.fill_(1)
        env.reset_dones()
        w.action_buf.zero_()
        if setplay is not None:  # the state alone: reset() below derives every row from it
            self.stager.call = int(counter) & 0xFFFFFFFF
            self.stager.counts.zero_()
            self.stager.start(env.state, (), only=int(setplay))
        if self.referee is not None:
            self.referee.restart(counter)
        w.set_opponent(self.opponents[team])
        obs = w.reset()["obs"]
        self.policy.counter = int(counter)
        self.seen.zero_()
        self.tally.zero_()
        stream = N.stream_of(self.device)
        for _ in range(self.steps):
            obs_d, _, dones, info = w.step(self.policy.act(obs))
            obs = obs_d["obs"]
            torch.bitwise_and(dones, torch.bitwise_not(self.seen), out=self.first)  # done & ~seen on 0 / 1 int64
            self.seen.bitwise_or_(dones)
            N.check(lib.vss_match_tally(stream, self.n_fields, self.rows_per_field, self.n_fields, 1, info["rews"].data_ptr(),
                                        self.first.data_ptr(), info["progress_buffer"].data_ptr(), self.tally.data_ptr()),
                    "vss_match_tally")
        episodes, wins, losses, steps = self.tally[0].tolist()  # the one host read
        out = {"score": score(wins, losses, episodes), "wins": wins, "losses": losses, "draws": episodes - wins - losses,
               "length": steps / episodes if episodes > 0 else 0.0}
        if self.referee is not None:
            out["stoppages"] = self.referee.counts.tolist()
        return out

    def evaluate(self, update: int) -> dict:
        """{team: {score, wins, losses, draws, length}} of the agent's current weights at `update`."""
        with torch.random.fork_rng(devices=[self.device]):
            self.policy.refresh()
            out = {t: self.play(t, (int(update) * len(self.teams) + i) * self.steps) for i, t in enumerate(self.teams)}
            for i, t in enumerate(self.teams):  # counters of their own, above every plain evaluation's
                for j, name in enumerate(self.setplays):
                    at = (int(update) * len(self.teams) + i) * len(self.setplays) + j
                    out[f"{t}@{name}"] = self.play(t, (1 << 40) + at * self.steps, setplay=j)
            return out

    def evaluate_into(self, rec: dict, update: int, writer, start_time: float) -> None:
        """The train loop's call: rec["eval"], rec["eval_s"], the writer's eval/* scalars; rec["wall_s"] and
        rec["sps"] then include the evaluation, as they include checkpoint_s."""
        t0 = time.time()
        rec["eval"] = self.evaluate(update)
        torch.cuda.synchronize(self.device)
        rec["eval_s"] = time.time() - t0
        rec["wall_s"] = time.time() - start_time
        rec["sps"] = int(rec["global_step"] / rec["wall_s"])
        for team, r in rec["eval"].items():
            writer.add_scalar(f"eval/score_{team}", r["score"], rec["global_step"])
            writer.add_scalar(f"eval/length_{team}", r["length"], rec["global_step"])
