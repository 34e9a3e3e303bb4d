"""The referee, measured.  Writes profiles/referee_bench.json.

kernel  vss_referee at 65,536 fields with no field whistled (the step loop's case: every ball moving), 1 % whistled and
        every field whistled (a ball at rest and --ref-stall-steps 1: a placed ball rests, so the same fields are
        whistled in every call), on the SA view (one row per field) and the mirror-DMA view (six).  Device events
        around `--launches` back-to-back calls after a warm-up; the arms alternate `--reps` times; per call: median
        (min-max) of the reps, through Referee.call and ("-entry") through the C entry with its arguments built once,
        with the algorithmic bytes -- per field the done flag, the counters and 16 state channels read (8 + 16 + 64 B)
        and the counters and the verdict written (16 + 4 B), per whistled field the 58 state channels (232 B), the dof
        velocities (48 B) and its rows (208 B each) written -- and their share of 8 TB/s.
loop    rollout_s of train() for three updates of 128 steps at sa 65,536 envs: flags off on this tree, flags off on the
        tree given with --parent (the parent commit's, built), and --ref-stall-steps 100 --ref-area-steps 20 on this
        tree; the arms alternate `--passes` times, each run a fresh process; updates 2-3 of each.
bench   `python bench.py --gpus 1 --steps K --warmup W` on this tree and on the parent's, alternately, `--passes` times:
        the FULL step's figure of each pass.

Needs a ROCm GPU; there is no fallback."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFEREE = ["--ref-stall-steps", "100", "--ref-area-steps", "20"]
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


def kernel_level(args):
    import torch

    from vss_amd import referee as R
    n = args.fields
    table, params = R.RefTable(), R.Params.of(stall_steps=1)
    views = {"sa": R.view_sa(), "mirror-dma": R.view_mirror(3, n)}
    out = []
    for name, view in views.items():
        rows_per_field = view.robots * view.n_teams
        g = torch.Generator(device="cuda").manual_seed(n + rows_per_field)
        rows = torch.zeros((view.span(n), 52), device="cuda")
        done = torch.zeros(n, dtype=torch.long, device="cuda")
        resting = {"none": torch.zeros(n, dtype=torch.bool, device="cuda"),
                   "1pct": torch.rand(n, device="cuda", generator=g) < 0.01,
                   "all": torch.ones(n, dtype=torch.bool, device="cuda")}
        arms, sizes, keep = {}, {}, []
        for k, rest in resting.items():
            state = torch.zeros((58, n), device="cuda")
            state[34:40] = 1.0                                         # qw
            state[4:10] = torch.linspace(-0.5, 0.5, 6, device="cuda")[:, None]
            state[10:16] = 0.55                                        # the robots parked, in no area
            state[0], state[1] = 0.3, 0.2
            state[2] = torch.where(rest, 0.0, 1.0)                     # the ball at rest, or moving at 1 m/s
            dof = torch.zeros((n, 2, 3, 2), device="cuda")
            ref = R.Referee(n, table, params, 1234, "cuda")
            ref.call(state, dof, [(rows, view)], done)
            first = int((ref.verdict >= 0).sum())
            arms[k] = lambda ref=ref, state=state, dof=dof: ref.call(state, dof, [(rows, view)], done)
            tab, prm, arr = table.c_table(), params.c_params(), (R.VssRefereeView * 2)()
            arr[0] = R.VssRefereeView(rows.data_ptr(), *view)
            lib, stream = R.load(), torch.cuda.current_stream().cuda_stream
            keep.append((tab, prm, arr, state, dof, ref))
            arms[k + "-entry"] = lambda lib=lib, stream=stream, tab=tab, prm=prm, arr=arr, state=state, dof=dof, ref=ref: \
                lib.vss_referee(stream, n, ctypes.byref(tab), ctypes.byref(prm), 1234, 7, done.data_ptr(), 1, state.data_ptr(),
                                dof.data_ptr(), ref.counters.data_ptr(), 1, arr, ref.counts.data_ptr(), ref.verdict.data_ptr())
            sizes[k] = {"resting_fields": int(rest.sum()), "whistled_first_call": first,
                        "bytes": n * 108 + int(rest.sum()) * (232 + 48 + 208 * rows_per_field)}
        rec = {"view": name, "fields": n, "rows_per_field": rows_per_field, "launches_per_rep": args.launches}
        for k, s in measure(torch, arms, args).items():
            size = sizes.get(k) or sizes[k.rsplit("-", 1)[0]]
            rec[k] = dict(size, per_call_us=s, share_of_8_TB_s=size["bytes"] / (s["median"] * 1e-6) / HBM_BYTES_PER_S)
        for k in resting:  # every call of an arm whistled the fields the first one did
            whistled = int((keep[list(resting).index(k)][5].verdict >= 0).sum())
            assert whistled == sizes[k]["resting_fields"] == sizes[k]["whistled_first_call"], (k, whistled, sizes[k])
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
    print("REFEREE " + json.dumps([{k: v for k, v in h.items() if k.startswith("referee/")} for h in hist]), flush=True)


def loop_level(args):
    arms = {"flags-off": (REPO, []), "referee": (REPO, REFEREE)}
    if args.parent:
        arms = {"flags-off": (REPO, []), "parent": (os.path.abspath(args.parent), []), "referee": (REPO, REFEREE)}
    runs = {k: [] for k in arms}
    per_pass = {k: [] for k in arms}
    calls = []
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
            if k == "referee":
                calls.append(json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("REFEREE ")][-1][len("REFEREE "):]))
            print(k, got, flush=True)
    rec = {"envs": 65536, "steps": 128, "updates_timed": f"2-3 of each of {args.passes} runs, arms alternating",
           "referee_flags": " ".join(REFEREE), "referee_calls_per_update": calls,
           **{k: {"rollout_s": summary(v), "mean_per_pass": per_pass[k]} for k, v in runs.items()}}
    rec["referee_us_per_step"] = (rec["referee"]["rollout_s"]["median"] - rec["flags-off"]["rollout_s"]["median"]) / 128 * 1e6
    print(json.dumps(rec), flush=True)
    return rec


def bench_level(args):
    """bench.py's JSON line on this tree and on the parent's, alternately."""
    trees = {"tree": REPO}
    if args.parent:
        trees["parent"] = os.path.abspath(args.parent)
    lines = {k: [] for k in trees}
    for _ in range(args.passes):
        for k, tree in trees.items():
            res = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup",
                                  str(args.bench_warmup)], cwd=tree, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise RuntimeError(f"{k}: bench.py ended with {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
            lines[k].append(line)
            print(k, json.dumps(line), flush=True)
    return lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sections", default="kernel,loop,bench")
    p.add_argument("--fields", type=int, default=65536)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--passes", type=int, default=2)
    p.add_argument("--bench-steps", type=int, default=100)
    p.add_argument("--bench-warmup", type=int, default=10)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the loop and bench sections")
    p.add_argument("--scratch", default=os.path.join(REPO, "runs", "referee_bench"))
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "referee_bench.json"))
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
    sections = args.sections.split(",")
    if "bench" in sections:  # first, with the loop: their processes run while this one has not opened the GPU
        result["bench"] = bench_level(args)
    if "loop" in sections:
        result["loop"] = loop_level(args)
    import torch
    result["device"] = torch.cuda.get_device_name(0)
    if "kernel" in sections:
        result["kernel"] = kernel_level(args)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
