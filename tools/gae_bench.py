"""Advantages and returns of one rollout: the torch expressions against vss_gae.

Kernel level (default): in ONE process, per shape (T = 128; E = 4,095, 65,536, 196,608, 393,216), two arms
alternate `--reps` times after a warm-up of each:
  torch   the train loop's torch path exactly: TerminalValues.next_values' merge (bool, cat, where), then
          compute_gae -- about 9 T + 8 launches;
  kernel  vss_amd.returns.gae, form B (the merge in the kernel), into preallocated outputs -- one launch.
Each arm is timed twice per rep: a host clock between two device synchronisations (the torch arm is bound by its
enqueue rate, which only the host clock sees whole) and device events around the same work.  The two arms' outputs
are compared bit for bit at every shape.  Reported per arm: median (min-max); for the kernel its bytes
(28 T E + 4 E in form B: five loads and two stores per element, and v_last) and its share of the 8 TB/s HBM spec.

`--variant-lib PATH` (a build of the same sources with another unroll, e.g.
  make -C rsoccer-isaac-cleanrl_amd/csrc GAE_UNROLL=4 OBJ=_obj/u4 OUT=../../tools/_ab/libvss_amd_gae_u4.so
) times the kernel arm alone of the default library and of that one (VSS_LIB_PATH), each in fresh child processes
that alternate, two passes each, and records both.

Loop level (`--loop`): train() at sa 4,095 and 65,536 envs, 6 updates of 128 steps; the default path and
VSS_GAE=torch alternate, two passes each; per update 2-6 the interval that holds this work,
wall_s[u] - wall_s[u-1] - (rollout_s[u] + update_s[u]), median (min-max) per path.

Writes profiles/gae_bench.json (`--out`).  Needs a ROCm GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rsoccer-isaac-cleanrl_amd"))

T = 128
ROWS = (4095, 65536, 196608, 393216)
HBM_SPEC = 8.0e12  # bytes/s


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def make_rollout(torch, E, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + E)
    f = lambda *s: torch.randn(s, device="cuda", generator=g)
    u = torch.rand((T, E), device="cuda", generator=g)
    return dict(rewards=f(T, E), values=f(T, E), term_values=f(T, E), v_last=f(E), next_dones=(u < 0.10).float(),
                next_timeouts=((u < 0.05) | (torch.rand((T, E), device="cuda", generator=g) < 0.02)).float())


def timed(torch, fn):
    """(host seconds between two synchronisations, device seconds between two events) of one fn()."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, e0.elapsed_time(e1) * 1e-3


def kernel_level(args, kernel_only=False):
    import torch

    import ppo_continuous_action_isaacgym as P
    from vss_amd.returns import gae
    gamma, lam = 0.99, 0.95
    out = {}
    for E in args.rows:
        d = make_rollout(torch, E)
        adv, ret = torch.empty((T, E), device="cuda"), torch.empty((T, E), device="cuda")

        def torch_arm():
            with torch.no_grad():
                nv = torch.where(d["next_dones"].bool(), d["term_values"],
                                 torch.cat([d["values"][1:], d["v_last"].view(1, E)], 0))
                return P.compute_gae(d["rewards"], d["values"], nv, d["next_dones"], d["next_timeouts"], gamma, lam)

        def kernel_arm():
            return gae(d["rewards"], d["values"], d["next_dones"], d["next_timeouts"], gamma, lam,
                       term_values=d["term_values"], v_last=d["v_last"], out=(adv, ret))

        arms = {"kernel": kernel_arm} if kernel_only else {"torch": torch_arm, "kernel": kernel_arm}
        for fn in arms.values():  # warm-up: code objects, the allocator's blocks
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        rec = {"T": T, "E": E}
        if not kernel_only:
            a_t, r_t = torch_arm()
            kernel_arm()
            rec["bit_equal"] = bool(torch.equal(a_t.view(torch.int32), adv.view(torch.int32))
                                    and torch.equal(r_t.view(torch.int32), ret.view(torch.int32)))
            del a_t, r_t
        times = {k: {"host_s": [], "device_s": []} for k in arms}
        for _ in range(args.reps):  # the arms alternate
            for k, fn in arms.items():
                h, dv = timed(torch, fn)
                times[k]["host_s"].append(h)
                times[k]["device_s"].append(dv)
        for k in arms:
            rec[k] = {c: summary(v) for c, v in times[k].items()}
        nbytes = 28 * T * E + 4 * E
        rec["kernel"]["bytes"] = nbytes
        rec["kernel"]["share_of_8TBps_spec_device_median"] = nbytes / rec["kernel"]["device_s"]["median"] / HBM_SPEC
        if not kernel_only:
            rec["kernel_not_slower_host"] = rec["kernel"]["host_s"]["median"] <= rec["torch"]["host_s"]["median"]
            rec["kernel_not_slower_device"] = rec["kernel"]["device_s"]["median"] <= rec["torch"]["device_s"]["median"]
        out[str(E)] = rec
        print(json.dumps(rec), flush=True)
        del d, adv, ret
        torch.cuda.empty_cache()
    return out


def loop_level(args):
    import ppo_continuous_action_isaacgym as P
    out = {}
    for E in args.loop_envs:
        runs = {"kernel": [], "torch": []}
        for _ in range(2):  # the paths alternate, two passes each
            for path in ("kernel", "torch"):
                if path == "torch":
                    os.environ["VSS_GAE"] = "torch"
                else:
                    os.environ.pop("VSS_GAE", None)
                a = P.parse_args(["--env-id", "sa", "--num-envs", str(E), "--num-steps", str(T), "--num-updates", "6",
                                  "--log", "false"])
                _, hist = P.train(a)
                gaps = [hist[i]["wall_s"] - hist[i - 1]["wall_s"] - (hist[i]["rollout_s"] + hist[i]["update_s"])
                        for i in range(1, 6)]  # updates 2-6
                runs[path].append({"gap_s": gaps, "rollout_s": [h["rollout_s"] for h in hist[1:]],
                                   "update_s": [h["update_s"] for h in hist[1:]]})
                print(json.dumps({"loop_envs": E, "path": path, "gap_s": gaps}), flush=True)
        os.environ.pop("VSS_GAE", None)
        rec = {"passes": runs}
        for path in runs:
            rec[path] = summary([g for r in runs[path] for g in r["gap_s"]])
        spread = rec["torch"]["max"] - rec["torch"]["min"]
        diff = rec["torch"]["median"] - rec["kernel"]["median"]
        rec["torch_minus_kernel_median_s"] = diff
        rec["torch_spread_s"] = spread
        rec["verdict"] = "gain" if diff > spread else "within noise"
        out[str(E)] = rec
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, nargs="+", default=list(ROWS))
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--unroll", type=int, default=8, help="the library's unroll (a label for the record)")
    p.add_argument("--variant-lib", default=None, help="a variant build under tools/ to time in a child process")
    p.add_argument("--variant-unroll", type=int, default=4, help="the variant's unroll (a label for the record)")
    p.add_argument("--kernel-only", action="store_true", help="time the kernel arm only and print one JSON line")
    p.add_argument("--loop", action="store_true", help="also the loop-level measurement")
    p.add_argument("--loop-envs", type=int, nargs="+", default=[4095, 65536])
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "gae_bench.json"))
    args = p.parse_args()
    if args.reps < 5:
        p.error("--reps: at least 5 alternations")
    import torch
    from vss_amd.minibatch import disable_graph_packet_capture
    disable_graph_packet_capture()  # as the train entry points do, before anything initialises the GPU
    if not torch.cuda.is_available():
        raise SystemExit("gae_bench needs a ROCm GPU")
    if args.kernel_only:
        print("RESULT " + json.dumps(kernel_level(args, kernel_only=True)))
        return
    rec = {"tool": "tools/gae_bench.py", "device": torch.cuda.get_device_name(0), "T": T, "reps": args.reps,
           "unroll": args.unroll, "shapes": kernel_level(args)}
    if args.variant_lib:
        # the two builds' kernel arms alone, each in fresh child processes that alternate (two passes each): the
        # same conditions for both, without the torch arm's traffic between the timed launches
        def child(lib):
            env = dict(os.environ)
            env.pop("VSS_LIB_PATH", None)
            if lib:
                env["VSS_LIB_PATH"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--kernel-only", "--reps", str(args.reps), "--rows"] + \
                [str(e) for e in args.rows]
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit(f"kernel-only run failed ({res.returncode}):\n{res.stderr[-2000:]}")
            line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1]
            return json.loads(line[len("RESULT "):])
        passes = {"default": [], "variant": []}
        for _ in range(2):
            passes["default"].append(child(None))
            passes["variant"].append(child(args.variant_lib))
        rec["unroll_comparison"] = {"default_unroll": args.unroll, "variant_unroll": args.variant_unroll,
                                    "variant_lib": os.path.relpath(args.variant_lib, REPO), "kernel_only_passes": passes}
        for E in rec["shapes"]:
            print(json.dumps({"E": int(E), **{f"{k}_device_us": [round(q[E]["kernel"]["device_s"]["median"] * 1e6, 1) for q in v]
                                               for k, v in passes.items()}}), flush=True)
    else:
        rec["unroll_comparison"] = "not measured"
    rec["loop"] = loop_level(args) if args.loop else "not measured"
    rec["kernel_not_slower_at_any_shape"] = all(s["kernel_not_slower_host"] and s["kernel_not_slower_device"]
                                                for s in rec["shapes"].values())
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
