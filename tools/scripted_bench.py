"""The scripted team and the evaluation arena, measured.  Writes profiles/scripted_bench.json.

kernel  vss_scripted_team at 65,536 and 4,095 fields, strides (156, 6), beside SnapshotOpponent's forward (the
        yellow team it replaces; kind x3: three rows per field) at the same field count in the same process.
        Device events around `--launches` back-to-back calls after a warm-up; the two arms alternate `--reps`
        times; per call: median (min-max) of the reps.  For the kernel also its share of the 8 TB/s HBM spec on
        the algorithmic 232 B per field (208 read, 24 written).
loop    rollout_s of train() for three updates of 128 steps at sa 65,536 and 4,095 envs with --opponent
        scripted, self and ou, in that order, twice; updates 2-3 of each run.
eval    eval_s per evaluation (three teams) at --eval-fields 1,024 and 16,384 on an untrained sa agent, beside
        ONE play_matches call (blue: the same weights through play.py's TeamSA, yellow: zero) that counts as
        many episodes as one team's evaluation -- the path the arena spares, per team.

Needs a ROCm GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rsoccer-isaac-cleanrl_amd"))

HBM_SPEC = 8.0e12  # bytes/s
BYTES_PER_FIELD = 232


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def device_seconds(torch, fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / launches


def kernel_level(args):
    import numpy as np
    import torch

    import ppo_continuous_action_isaacgym as P
    from envs._gym import Box
    from collections import namedtuple
    from vss_amd import scripted as S
    from vss_amd.opponent import SnapshotOpponent
    Env = namedtuple("Env", ["single_observation_space", "single_action_space"])
    torch.manual_seed(0)
    agent = P.Agent(Env(Box(-np.inf, np.inf, (52,)), Box(-1.0, 1.0, (2,)))).cuda()
    snapshot = SnapshotOpponent(agent, "x3", seed=1)
    out = []
    for n in args.fields:
        g = torch.Generator(device="cuda").manual_seed(n)
        obs = torch.rand((n, 3, 52), device="cuda", generator=g) * 1.2 - 0.6
        act = torch.zeros((n, 3, 2), device="cuda")
        arms = {"scripted": lambda: S.scripted_actions(act, obs), "snapshot": lambda: snapshot(act, obs)}
        for fn in arms.values():
            for _ in range(20):
                fn()
        times = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                times[k].append(device_seconds(torch, fn, args.launches))
        rec = {"fields": n, "launches_per_rep": args.launches,
               **{k: {"per_call_us": summary([t * 1e6 for t in v])} for k, v in times.items()}}
        med = rec["scripted"]["per_call_us"]["median"] * 1e-6
        rec["scripted"]["bytes"] = BYTES_PER_FIELD * n
        rec["scripted"]["share_of_8TBps_spec"] = BYTES_PER_FIELD * n / med / HBM_SPEC
        rec["snapshot_over_scripted"] = rec["snapshot"]["per_call_us"]["median"] / rec["scripted"]["per_call_us"]["median"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def loop_level(args):
    import ppo_continuous_action_isaacgym as P
    out = []
    for n in args.fields:
        runs = {k: [] for k in ("scripted", "self", "ou")}
        for _ in range(2):
            for opp in runs:
                a = P.parse_args(["--env-id", "sa", "--num-envs", str(n), "--num-updates", "3", "--opponent", opp, "--log",
                                  "false", "--kernel-warmup", "false", "--save-path", args.scratch])
                _, hist = P.train(a)
                runs[opp] += [h["rollout_s"] for h in hist[1:]]
        rec = {"envs": n, "updates_timed": "2-3 of each of 2 runs",
               **{k: {"rollout_s": summary(v)} for k, v in runs.items()}}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def eval_level(args):
    from collections import namedtuple

    import numpy as np
    import torch

    import ppo_continuous_action_isaacgym as P
    from envs._gym import Box
    from play import get_team, play_matches
    from vss_amd.arena import Arena
    out = []
    a = P.parse_args(["--env-id", "sa"])
    Env = namedtuple("Env", ["single_observation_space", "single_action_space"])
    torch.manual_seed(1)
    agent = P.Agent(Env(Box(-np.inf, np.inf, (52,)), Box(-1.0, 1.0, (2,)))).cuda()
    os.makedirs(args.scratch, exist_ok=True)
    ckpt = os.path.join(args.scratch, "untrained-agent.pt")
    torch.save(agent.state_dict(), ckpt)
    for n in args.eval_fields:
        a.eval_fields = n
        arena = Arena(a, agent, torch.device("cuda:0"))
        arena.evaluate(0)  # warm-up
        times, res = [], None
        for u in range(1, 4):
            torch.cuda.synchronize()
            t0 = time.time()
            res = arena.evaluate(u)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
        # the path it spares: play_matches on a raw env of as many fields, counting n episodes, per team
        from envs.vss import VSS, default_cfg
        raw = VSS(default_cfg(n), "cuda:0", "cuda:0", 0, True, False, False)
        raw.w_goal, raw.w_grad, raw.w_move, raw.w_energy = 1.0, 0.0, 0.0, 0.0
        blue, yellow = get_team("ppo-sa", ckpt, "cuda:0"), get_team("zero")
        pm = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.time()
            play_matches(raw, blue, yellow, min(n, 1065))
            torch.cuda.synchronize()
            pm.append(time.time() - t0)
        rec = {"eval_fields": n, "teams": arena.teams, "eval_s": summary(times), "last_eval": res,
               "play_matches_one_team": {"episodes_counted": min(n, 1065), "seconds": summary(pm),
                                         "note": "counts among the first 1,065 fields only"}}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sections", default="kernel,loop,eval")
    p.add_argument("--fields", type=int, nargs="+", default=[65536, 4095])
    p.add_argument("--eval-fields", type=int, nargs="+", default=[1024, 16384])
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--scratch", default=os.path.join(REPO, "runs", "scripted_bench"))
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "scripted_bench.json"))
    args = p.parse_args()
    from vss_amd.minibatch import disable_graph_packet_capture
    disable_graph_packet_capture()
    import torch
    result = {"device": torch.cuda.get_device_name(0)}
    for name, fn in (("kernel", kernel_level), ("loop", loop_level), ("eval", eval_level)):
        if name in args.sections.split(","):
            result[name] = fn(args)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
