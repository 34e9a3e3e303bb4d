#!/usr/bin/env python3
"""What --checkpoint-every costs: profiles/resume_bench.json and profiles/resume_bench_line.json.

    python tools/resume_bench.py [--configs sa-4095,sa-65536,sa-65536-pool,dma-196608] [--updates 6] [--passes 2]
    python tools/resume_bench.py --bench-line PARENT_TREE [--pairs 3]

The first form runs train() for `updates` updates with --checkpoint-every 1 and the same run without the flag, in
this process, alternating, `passes` times per configuration, and reports per update, as median (min-max):
checkpoint_s, the state file's size, and rollout_s / update_s of both arms (the flag must not move the two stage
clocks beyond the flag-off arm's own spread).  Each configuration's record is merged into the output file, so the
configurations may be measured in several calls.  The first update of every run (code loading, graph capture) is
left out of the stage clocks' summaries; --kernel-warmup is off in both arms.

The second form takes the default bench line (bench.py --gpus 1 --steps 100 --warmup 10) of a checkout of the parent
commit with its own built library and of this tree, alternating, each in a process of its own.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "rsoccer-isaac-cleanrl_amd")
sys.path.insert(0, PKG)

CONFIGS = {
    "sa-4095": ["--env-id", "sa", "--num-envs", "4095"],
    "sa-65536": ["--env-id", "sa", "--num-envs", "65536"],
    "sa-65536-pool": ["--env-id", "sa", "--num-envs", "65536", "--opponent", "pool"],
    "dma-196608": ["--env-id", "dma", "--num-envs", "196608"],
}


def summary(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "values": list(values)}


def merge(path, key, record):
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out[key] = record
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def checkpoint_cost(a):
    import torch

    import ppo_continuous_action_isaacgym as P
    from vss_amd import _native as N
    from vss_amd import checkpoint as CK

    P.disable_graph_packet_capture()
    N.require_device("cuda:0")  # a measurement without the GPU fails; it does not fall back
    for name in a.configs.split(","):
        argv = CONFIGS[name] + ["--num-updates", str(a.updates), "--log", "false", "--kernel-warmup", "false"]
        arms = {"off": [], "on": []}
        sizes = []
        for p in range(a.passes):
            for arm in ("off", "on") if p % 2 == 0 else ("on", "off"):
                tmp = tempfile.mkdtemp(prefix="resume_bench_")
                try:
                    args = P.parse_args(argv + ["--save-path", tmp] + (["--checkpoint-every", "1"] if arm == "on" else []))

                    def size_of(rec, agent, args=args, arm=arm):
                        if arm == "on":
                            sizes.append(os.path.getsize(CK.checkpoint_paths(args, f"{args.exp_name}_ppo-{args.env_id}_{args.seed}")[0]))

                    _, hist = P.train(args, on_update=size_of)
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)
                arms[arm].append(hist)
                print(f"{name} pass {p} {arm}: update_s {hist[-1]['update_s']:.3f} rollout_s {hist[-1]['rollout_s']:.3f} "
                      f"checkpoint_s {hist[-1]['checkpoint_s']:.3f}", flush=True)
                torch.cuda.empty_cache()
        steady = {arm: [h for hist in runs for h in hist[1:]] for arm, runs in arms.items()}
        rec = {"device": torch.cuda.get_device_name(0), "argv": argv, "updates": a.updates, "passes": a.passes,
               "num_steps": 128, "checkpoint_s": summary([h["checkpoint_s"] for hist in arms["on"] for h in hist]),
               "state_file_bytes": summary(sizes)}
        for k in ("rollout_s", "update_s"):
            off, on = summary([h[k] for h in steady["off"]]), summary([h[k] for h in steady["on"]])
            rec[k] = {"off": off, "on": on, "difference_of_medians": on["median"] - off["median"],
                      "off_spread": off["max"] - off["min"]}
            rec[k]["within_off_spread"] = abs(rec[k]["difference_of_medians"]) <= rec[k]["off_spread"]
        per_update = statistics.median([h["rollout_s"] + h["update_s"] for h in steady["off"]])
        share = rec["checkpoint_s"]["median"] / (per_update + rec["checkpoint_s"]["median"])
        rec["update_wall_s_off_median"] = per_update
        rec["checkpoint_share_of_wall_every_update"] = share
        # K at which the write falls under 1 % of the wall time: c / (K u + c) < 0.01
        rec["k_for_under_1_percent"] = max(1, int(99 * rec["checkpoint_s"]["median"] / per_update) + 1)
        merge(a.out, name, rec)
        print(json.dumps({name: {k: rec[k] for k in ("checkpoint_share_of_wall_every_update", "k_for_under_1_percent")}}),
              flush=True)


def bench_line(a):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "10"]
    trees = {"parent": os.path.abspath(a.bench_line), "this_tree": REPO}
    values = {k: [] for k in trees}
    last = None
    for pair in range(a.pairs):
        for k in ("parent", "this_tree") if pair % 2 == 0 else ("this_tree", "parent"):
            out = subprocess.run(cmd, cwd=trees[k], capture_output=True, text=True, timeout=600, check=True)
            line = json.loads(out.stdout.strip().splitlines()[-1])
            values[k].append(line["ms_per_step"] * 1000)
            last = line if k == "this_tree" else last
            print(f"pair {pair} {k}: {values[k][-1]:.3f} us per step", flush=True)
    parent, tree = summary(values["parent"]), summary(values["this_tree"])
    diff, spread = tree["median"] - parent["median"], parent["max"] - parent["min"]
    rec = {"command": "bench.py --gpus 1 --steps 100 --warmup 10 (the default FULL-step line; no kernel it runs changed)",
           "unit": "us per step (ms_per_step x 1000)",
           "note": "the parent commit from a checkout of its own with its own library and this tree alternate, "
                   "one process each, the first of a pair alternating too",
           "pairs": a.pairs, "parent": parent, "this_tree": tree, "difference_of_medians": diff, "parent_spread": spread,
           "within_parent_spread": abs(diff) <= spread, "last_line_this_tree": last}
    with open(a.line_out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("difference_of_medians", "parent_spread", "within_parent_spread")}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--updates", type=int, default=6)
    p.add_argument("--passes", type=int, default=2)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "resume_bench.json"))
    p.add_argument("--bench-line", default=None, metavar="PARENT_TREE")
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--line-out", default=os.path.join(REPO, "profiles", "resume_bench_line.json"))
    a = p.parse_args()
    if a.bench_line:
        bench_line(a)
    else:
        checkpoint_cost(a)


if __name__ == "__main__":
    main()
