"""The estimation channel, measured.  Writes profiles/estimate_bench.json.

kernel  vss_estimate (a step call, not the start call; 1 % of the fields done, the terminal rows the rows themselves
        elsewhere, as perception delivers them) at 65,536 fields on the SA layout (65,536 rows), the DMA layout
        (196,608) and the mirror DMA layout (393,216), D = 1, 3 and 15, every row at its full age.  Device events
        around `--launches` back-to-back calls after a warm-up; the arms of a layout alternate `--reps` times; per
        call: median (min-max) of the reps, with the algorithmic bytes -- per row two rows read and two written
        (4 x 208 B), the history read (24 (D - 1) B) and written (24 B) and 4 B of age -- and their share of 8 TB/s.
loop    rollout_s of train() for three updates of 128 steps at sa 65,536 envs: flags off on this tree, flags off
        on the tree given with --parent (the parent commit's, built), --obs-delay 2 without and with --obs-predict 1
        on this tree; the arms alternate `--passes` times, each run a fresh process; updates 2-3 of each.

Needs a ROCm GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DELAY = ["--obs-delay", "2"]
PREDICT = DELAY + ["--obs-predict", "1"]
HBM_BYTES_PER_S = 8e12


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


def measure(torch, arms, args):
    for fn in arms.values():
        for _ in range(20):
            fn()
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, fn in arms.items():
            times[k].append(device_seconds(torch, fn, args.launches))
    return {k: summary([t * 1e6 for t in v]) for k, v in times.items()}


def plausible_rows(torch, rows, g):
    """Rows on the field with unit headings, speeds up to 1 m/s, yaw rates up to 25 rad/s, commands in [-1, 1]."""
    r = torch.rand((rows, 52), device="cuda", generator=g) * 2 - 1
    for base in (4, 13, 22, 31, 38, 45):
        yaw = r[:, base + 4] * 3.1415927
        r[:, base + 4], r[:, base + 5] = torch.cos(yaw), torch.sin(yaw)
        r[:, base + 6] *= 25.0
    return r.contiguous()


def kernel_level(args):
    import torch

    from vss_amd import estimate as E
    n = args.fields
    layouts = {"sa": (E.layout_sa(), 1), "dma": (E.layout_dma(), 3), "mirror-dma": (E.layout_mirror(3, n), 3)}
    out = []
    for name, (lay, stride) in layouts.items():
        rows = lay.span(n)
        g = torch.Generator(device="cuda").manual_seed(rows)
        obs = plausible_rows(torch, rows, g)
        done = (torch.rand(n, device="cuda", generator=g) < 0.01).long().repeat_interleave(stride).contiguous()
        arms, sizes = {}, {}
        for delay in (1, 3, 15):  # 15: beyond the issue's arms, what the fourteen-entry form costs
            ch = E.EstimationChannel(n, lay, delay, "cuda", done_stride=stride)
            ch.start(obs)
            arms[f"D{delay}"] = lambda ch=ch: ch.estimate(obs, obs, done)
            sizes[f"D{delay}"] = rows * (4 * 208 + 24 * (delay - 1) + 24 + 4)
        rec = {"layout": name, "fields": n, "rows": rows, "launches_per_rep": args.launches}
        for k, s in measure(torch, arms, args).items():
            rec[k] = {"per_call_us": s, "bytes": sizes[k], "share_of_8_TB_s": sizes[k] / (s["median"] * 1e-6) / HBM_BYTES_PER_S}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def child_train(tree, scratch, flags):
    """In a fresh process: train() of the package in `tree`; prints the rollout_s of updates 2-3 as one JSON line."""
    sys.path.insert(0, os.path.join(tree, "rsoccer-isaac-cleanrl_amd"))
    import ppo_continuous_action_isaacgym as P
    P.disable_graph_packet_capture()
    a = P.parse_args(["--env-id", "sa", "--num-envs", "65536", "--num-updates", "3", "--log", "false", "--save-path", scratch]
                     + flags)
    _, hist = P.train(a)
    print("ROLLOUT_S " + json.dumps([h["rollout_s"] for h in hist[1:]]), flush=True)


def loop_level(args):
    arms = {"flags-off": (REPO, []), "delay": (REPO, DELAY), "delay-predict": (REPO, PREDICT)}
    if args.parent:
        arms = {"flags-off": (REPO, []), "parent": (os.path.abspath(args.parent), []), "delay": (REPO, DELAY),
                "delay-predict": (REPO, PREDICT)}
    runs = {k: [] for k in arms}
    per_pass = {k: [] for k in arms}
    for _ in range(args.passes):
        for k, (tree, flags) in arms.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--child-train", tree, "--scratch", args.scratch, "--"] + flags
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise RuntimeError(f"{k}: the training process ended with {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("ROLLOUT_S ")][-1]
            got = json.loads(line[len("ROLLOUT_S "):])
            runs[k] += got
            per_pass[k].append(statistics.mean(got))
            print(k, got, flush=True)
    rec = {"envs": 65536, "steps": 128, "updates_timed": f"2-3 of each of {args.passes} runs, arms alternating",
           "delay_flags": " ".join(DELAY), "delay_predict_flags": " ".join(PREDICT),
           **{k: {"rollout_s": summary(v), "mean_per_pass": per_pass[k]} for k, v in runs.items()}}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sections", default="kernel,loop")
    p.add_argument("--fields", type=int, default=65536)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--passes", type=int, default=2)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the loop section")
    p.add_argument("--scratch", default=os.path.join(REPO, "runs", "estimate_bench"))
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "estimate_bench.json"))
    p.add_argument("--child-train", default=None, help=argparse.SUPPRESS)
    p.add_argument("rest", nargs="*", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.child_train:
        child_train(args.child_train, args.scratch, args.rest)
        return
    sys.path.insert(0, os.path.join(REPO, "rsoccer-isaac-cleanrl_amd"))
    from vss_amd.minibatch import disable_graph_packet_capture
    disable_graph_packet_capture()
    result = {}
    if "loop" in args.sections.split(","):  # first: its processes run while this one has not opened the GPU
        result["loop"] = loop_level(args)
    import torch
    result["device"] = torch.cuda.get_device_name(0)
    if "kernel" in args.sections.split(","):
        result["kernel"] = kernel_level(args)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
