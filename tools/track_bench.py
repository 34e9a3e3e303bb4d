"""The tracking channel, measured.  Writes profiles/track_bench.json.

kernel  vss_track (a step call, not the start call; 1 % of the fields done, the terminal rows the rows themselves, the
        rows a noisy look at the filter's state so that bodies take the blend) at 65,536 fields on the SA layout
        (65,536 rows), the DMA layout (196,608) and the mirror DMA layout (393,216), D = 0 and 2, every row at its
        full age.  Device events around `--launches` back-to-back calls after a warm-up; the arms of a layout
        alternate `--reps` times; per call: median (min-max) of the reps, with the algorithmic bytes -- per row three
        rows read and three written (6 x 208 B), with a delay the history entry read and written (2 x 24 B), and the
        age read and written (2 x 4 B) -- and their share of 8 TB/s.
loop    rollout_s of train() for three updates of 128 steps at sa 65,536 envs: flags off on this tree, flags off
        on the tree given with --parent (the parent commit's, built), --obs-delay 2 --obs-noise-pos 0.002 without and
        with the filter's gains on this tree; the arms alternate `--passes` times, each run a fresh process; updates
        2-3 of each.

Needs a ROCm GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOISY = ["--obs-delay", "2", "--obs-noise-pos", "0.002"]
FILTER = NOISY + ["--obs-filter-team", "0.2", "--obs-filter-opp", "0.5", "--obs-filter-ball", "0.5"]
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

    from vss_amd import track as T
    n = args.fields
    layouts = {"sa": (T.layout_sa(), 1), "dma": (T.layout_dma(), 3), "mirror-dma": (T.layout_mirror(3, n), 3)}
    out = []
    for name, (lay, stride) in layouts.items():
        rows = lay.span(n)
        g = torch.Generator(device="cuda").manual_seed(rows)
        obs = plausible_rows(torch, rows, g)
        done = (torch.rand(n, device="cuda", generator=g) < 0.01).long().repeat_interleave(stride).contiguous()
        arms, sizes = {}, {}
        look = obs.clone()
        look[:, :4] += 0.001  # a look a little off the state: inside the gates, so the bodies blend
        for delay in (0, 2):
            ch = T.TrackingChannel(n, lay, delay, T.Params(0.2, 0.5, 0.5, 0.2, 1.0), "cuda", done_stride=stride)
            ch.start(obs)
            arms[f"D{delay}"] = lambda ch=ch: ch.track(look, look, done)
            sizes[f"D{delay}"] = rows * (6 * 208 + (48 if delay else 0) + 8)
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
    arms = {"flags-off": (REPO, []), "noisy": (REPO, NOISY), "noisy-filter": (REPO, FILTER)}
    if args.parent:
        arms = {"flags-off": (REPO, []), "parent": (os.path.abspath(args.parent), []), "noisy": (REPO, NOISY),
                "noisy-filter": (REPO, FILTER)}
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
           "noisy_flags": " ".join(NOISY), "noisy_filter_flags": " ".join(FILTER),
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
    p.add_argument("--scratch", default=os.path.join(REPO, "runs", "track_bench"))
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "track_bench.json"))
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
