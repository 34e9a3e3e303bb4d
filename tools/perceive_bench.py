"""The perception channel, measured.  Writes profiles/perceive_bench.json.

kernel  vss_perceive (a step call, not the start call) on the SA layout at 65,536 rows, the DMA layout at 196,608
        rows and the mirror DMA layout at 393,216 rows (65,536 fields each), for delay 0 and 3, noise off and all
        four classes on.  Device events around `--launches` back-to-back calls after a warm-up; the four arms of a
        layout alternate `--reps` times; per call: median (min-max) of the reps, with the algorithmic bytes -- per
        row the true row and the delayed frame (delay 0: the terminal row) read, the ring slot and both outputs
        written, 5 x 208 B, plus the terminal row's six action floats for delay >= 1 and 16 B per field of done
        and age -- and their share of the 8 TB/s HBM spec.
loop    rollout_s of train() for three updates of 128 steps at sa 65,536 envs: flags off on this tree, flags off
        on the tree given with --parent (the parent commit's, built), flags on (--obs-delay 2 and all four noise
        classes) on this tree; the arms alternate `--passes` times, each run a fresh process; updates 2-3 of each.

Needs a ROCm GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_SPEC = 8.0e12  # bytes/s
ROW = 208
ON = ["--obs-delay", "2", "--obs-noise-pos", "0.002", "--obs-noise-vel", "0.01", "--obs-noise-ang", "0.02",
      "--obs-noise-angvel", "0.1"]


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
    import torch

    from vss_amd import perceive as PC
    n = args.fields
    layouts = {"sa": (PC.layout_sa(), 1), "dma": (PC.layout_dma(), 3), "mirror-dma": (PC.layout_mirror(3, n), 3)}
    noise_on = PC.Noise(0.002, 0.01, 0.02, 0.1)
    out = []
    for name, (lay, stride) in layouts.items():
        rows = lay.span(n)
        g = torch.Generator(device="cuda").manual_seed(rows)
        obs = torch.rand((rows, 52), device="cuda", generator=g) * 1.2 - 0.6
        term = torch.rand((rows, 52), device="cuda", generator=g) * 1.2 - 0.6
        done = (torch.rand(n, device="cuda", generator=g) < 0.01).long().repeat_interleave(stride).contiguous()
        arms = {}
        for delay in (0, 3):
            for label, noise in (("off", PC.Noise()), ("on", noise_on)):
                ch = PC.PerceptionChannel(n, lay, delay, noise, 1, "cuda", done_stride=stride)
                ch.start(obs)
                arms[f"delay{delay}-noise-{label}"] = (delay, lambda ch=ch: ch.perceive(obs, term, done))
        for _, fn in arms.values():
            for _ in range(20):
                fn()
        times = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, (_, fn) in arms.items():
                times[k].append(device_seconds(torch, fn, args.launches))
        rec = {"layout": name, "fields": n, "rows": rows, "launches_per_rep": args.launches}
        for k, (delay, _) in arms.items():
            nbytes = rows * (5 * ROW + (24 if delay else 0)) + 16 * n
            s = summary([t * 1e6 for t in times[k]])
            rec[k] = {"per_call_us": s, "bytes": nbytes, "share_of_8TBps_spec": nbytes / (s["median"] * 1e-6) / HBM_SPEC}
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
    arms = {"flags-off": (REPO, []), "flags-on": (REPO, ON)}
    if args.parent:
        arms = {"flags-off": (REPO, []), "parent": (os.path.abspath(args.parent), []), "flags-on": (REPO, ON)}
    runs = {k: [] for k in arms}
    for _ in range(args.passes):
        for k, (tree, flags) in arms.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--child-train", tree, "--scratch", args.scratch, "--"] + flags
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise RuntimeError(f"{k}: the training process ended with {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("ROLLOUT_S ")][-1]
            runs[k] += json.loads(line[len("ROLLOUT_S "):])
    rec = {"envs": 65536, "steps": 128, "updates_timed": f"2-3 of each of {args.passes} runs, arms alternating",
           "flags_on": " ".join(ON), **{k: {"rollout_s": summary(v)} for k, v in runs.items()}}
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
    p.add_argument("--scratch", default=os.path.join(REPO, "runs", "perceive_bench"))
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "perceive_bench.json"))
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
