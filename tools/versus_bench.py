#!/usr/bin/env python3
"""Time the versus step (vss_step_versus: a policy's action buffer drives the yellow team) and the
mirror step (vss_step_mirror: both teams' robots are learner rows) next to the plain wrapped step
(vss_step) of the same mode, and one PPO rollout with --opponent self next to --opponent ou.
Prints one JSON line.

    python tools/versus_bench.py [--fields 65536] [--launches 200] [--rounds 5] [--rollout-steps 128]
    python tools/versus_bench.py --skip-rollout --mirror-rollout sa,cma,dma   # mirror against self, train()

Step times: HIP events around `launches` back-to-back launches with pre-built arguments (no Python
work per launch beyond the ctypes call), after a warm-up of every kernel; plain, versus and mirror
windows alternate `rounds` times on the same fields and the median window is reported with the
spread (min, max).  Bytes per field are the algorithmic HBM bytes of each contract:
the mode's plain bytes (bench.py BYTES); for the versus step + 24 read (opponent actions) + 624
written (the yellow robots' observations); for the mirror step MIRROR_EXTRA below.
`frac_hbm_peak` is bytes over time over 8 TB/s.

Rollout: ppo_continuous_action_isaacgym.train() for two updates of `rollout-steps` steps at `fields`
envs, `rollout_s` of the second update (the first carries first-use costs), once per opponent.
Mirror rollout: train() for three updates per env_id with --opponent mirror and --opponent self at
the same field count (`fields`; dma: half of it), `rollout_s` / `update_s` of every update and the
learner rows per second of rollout.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rsoccer-isaac-cleanrl_amd"))
import torch  # noqa: E402

import ppo_continuous_action_isaacgym as P  # noqa: E402
from envs import wrappers as Wr  # noqa: E402
from envs.vss import VSS, default_cfg  # noqa: E402
from vss_amd import _native as N  # noqa: E402

HBM_PEAK = 8.0e12  # B/s (bench.py)
PLAIN_BYTES = {"sa": 1001, "cma": 1017, "dma": 1923}  # bench.py BYTES
VERSUS_EXTRA = 24 + 624
# the mirror step on top of the plain step, per field: the yellow learner's actions read; its obs and
# terminal obs (208 B per row each), rew 16, reward_sum 4, dones 8, time_outs 1, progress_f 4 per row
# written; SA / CMA also io->dones_rep (8), which the plain DMA step already writes
MIRROR_EXTRA = {"sa": 8 + 1 * (416 + 33) + 8, "cma": 24 + 1 * (416 + 33) + 8, "dma": 24 + 3 * (416 + 33)}


def step_leg(name: str, n: int, launches: int, rounds: int, dev, with_mirror: bool = True) -> dict:
    cfg = default_cfg(n)
    cfg["env"]["seed"] = 1234
    env = VSS(cfg, dev, dev, 0, True, False, False)
    W = {"sa": Wr.SingleAgent, "cma": Wr.CMA, "dma": Wr.DMA}[name](env)
    mode = W.MODE
    rows, width = {"sa": (n, 2), "cma": (n, 6), "dma": (3 * n, 2)}[name]
    gen = torch.Generator(device=dev).manual_seed(99)
    pool = [torch.rand((rows, width), device=dev, generator=gen) * 2 - 1 for _ in range(16)]
    opp_pool = [torch.rand((n, 3, 2), device=dev, generator=gen) * 2 - 1 for _ in range(16)]
    opp_obs = torch.zeros((n, 3, 52), device=dev)
    lib, stream = N.load(), N.stream_of(torch.device(dev))
    prm, st = env._c_params(), env._c_state()
    cios = [N.VssStepIO(a.data_ptr(), W.action_buf.data_ptr(), W._obs.data_ptr(), W._terminal_obs.data_ptr(),
                        W._rews.data_ptr(), W._reward.data_ptr(), N.ptr(W._dones), W._time_outs.data_ptr(),
                        W._progress.data_ptr()) for a in pool]
    vios = [N.VssVersusIO(a.data_ptr(), opp_obs.data_ptr()) for a in opp_pool]
    # the mirror step: the yellow team's rows beside the wrapper's, and dones_rep in every mode
    yl = dict(obs=torch.zeros_like(W._obs), term=torch.zeros_like(W._terminal_obs), rew=torch.zeros_like(W._rews),
              rsum=torch.zeros_like(W._reward), dones=torch.zeros(rows, dtype=torch.long, device=dev),
              touts=torch.zeros(rows, dtype=torch.bool, device=dev), prog=torch.zeros(rows, device=dev))
    dones_b = W._dones if W._dones is not None else torch.zeros(rows, dtype=torch.long, device=dev)
    yl_pool = [torch.rand((rows, width), device=dev, generator=gen) * 2 - 1 for _ in range(16)]
    mcios = [N.VssStepIO(a.data_ptr(), W.action_buf.data_ptr(), W._obs.data_ptr(), W._terminal_obs.data_ptr(),
                         W._rews.data_ptr(), W._reward.data_ptr(), dones_b.data_ptr(), W._time_outs.data_ptr(),
                         W._progress.data_ptr()) for a in pool]
    mios = [N.VssMirrorIO(a.data_ptr(), yl["obs"].data_ptr(), yl["term"].data_ptr(), yl["rew"].data_ptr(),
                          yl["rsum"].data_ptr(), yl["dones"].data_ptr(), yl["touts"].data_ptr(), yl["prog"].data_ptr())
            for a in yl_pool]
    rp, rs = ctypes.byref(prm), ctypes.byref(st)
    rc_, rv = [ctypes.byref(c) for c in cios], [ctypes.byref(v) for v in vios]
    rmc, rm = [ctypes.byref(c) for c in mcios], [ctypes.byref(m) for m in mios]

    def plain(k):
        return lib.vss_step(stream, n, mode, rp, rs, rc_[k % 16])

    def versus(k):
        return lib.vss_step_versus(stream, n, mode, rp, rs, rc_[k % 16], rv[k % 16])

    def mirror(k):
        return lib.vss_step_mirror(stream, n, mode, rp, rs, rmc[k % 16], rm[k % 16])

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(launches):
            if fn(k) != 0:
                raise RuntimeError("launch failed")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches  # us per step

    arms = (("plain", plain), ("versus", versus)) + ((("mirror", mirror),) if with_mirror else ())
    for _, fn in arms:  # warm-up: code objects, the clocks
        for k in range(50):
            fn(k)
    torch.cuda.synchronize()
    t = {key: [] for key, _ in arms}
    for _ in range(rounds):
        for key, fn in arms:
            t[key].append(window(fn))
    out = {}
    per = {"plain": PLAIN_BYTES[name], "versus": PLAIN_BYTES[name] + VERSUS_EXTRA,
           "mirror": PLAIN_BYTES[name] + MIRROR_EXTRA[name]}
    for key, per_field in ((key, per[key]) for key, _ in arms):
        us = statistics.median(t[key])
        out[key] = {"us_per_step": us, "us_min": min(t[key]), "us_max": max(t[key]), "bytes_per_field": per_field,
                    "gb_per_s": per_field * n / (us * 1e-6) / 1e9, "frac_hbm_peak": per_field * n / (us * 1e-6) / HBM_PEAK}
    out["versus_over_plain"] = out["versus"]["us_per_step"] / out["plain"]["us_per_step"]
    out["bytes_ratio"] = out["versus"]["bytes_per_field"] / out["plain"]["bytes_per_field"]
    if with_mirror:  # the yardstick is the versus step of the same mode
        out["mirror_over_versus"] = out["mirror"]["us_per_step"] / out["versus"]["us_per_step"]
        out["mirror_bytes_over_versus"] = out["mirror"]["bytes_per_field"] / out["versus"]["bytes_per_field"]
        out["mirror_over_plain"] = out["mirror"]["us_per_step"] / out["plain"]["us_per_step"]
    return out


def rollout_leg(opponent: str, n: int, steps: int) -> dict:
    args = P.parse_args(["--env-id", "sa", "--num-envs", str(n), "--num-steps", str(steps), "--num-updates", "2",
                         "--log", "false", "--opponent", opponent])
    _, hist = P.train(args)
    return {"rollout_s": hist[-1]["rollout_s"], "update_s": hist[-1]["update_s"], "first_rollout_s": hist[0]["rollout_s"],
            "opponent_version": hist[-1]["opponent_version"]}


def mirror_rollout_leg(env_id: str, fields: int, steps: int) -> dict:
    """train() for three updates with --opponent mirror and --opponent self at the same field count."""
    out = {"fields": fields, "steps": steps}
    for opponent, rows in (("mirror", fields * (6 if env_id == "dma" else 2)), ("self", fields * (3 if env_id == "dma" else 1))):
        args = P.parse_args(["--env-id", env_id, "--num-envs", str(rows), "--num-steps", str(steps), "--num-updates", "3",
                             "--log", "false", "--opponent", opponent])
        _, hist = P.train(args)
        roll = [h["rollout_s"] for h in hist]
        out[opponent] = {"learner_rows": rows, "rollout_s": roll, "update_s": [h["update_s"] for h in hist],
                         "rows_per_s_of_rollout": rows * steps / statistics.median(roll)}
        torch.cuda.empty_cache()
    out["mirror_over_self_rollout_s"] = statistics.median(out["mirror"]["rollout_s"]) / statistics.median(out["self"]["rollout_s"])
    out["mirror_over_self_rows_per_s"] = out["mirror"]["rows_per_s_of_rollout"] / out["self"]["rows_per_s_of_rollout"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--fields", type=int, default=65536)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--rollout-steps", type=int, default=128)
    p.add_argument("--skip-rollout", action="store_true")
    p.add_argument("--skip-step", action="store_true")
    p.add_argument("--no-mirror", action="store_true", help="plain and versus windows only")
    p.add_argument("--mirror-rollout", default="", help="env ids (sa,cma,dma) for the mirror-against-self train() legs")
    a = p.parse_args()
    P.disable_graph_packet_capture()
    N.require_device("cuda:0")  # a measurement without the GPU fails; it does not fall back
    res = {"fields": a.fields, "launches_per_window": a.launches, "rounds": a.rounds, "hbm_peak_gb_per_s": HBM_PEAK / 1e9,
           "device": torch.cuda.get_device_name(0),
           "step": {} if a.skip_step else {m: step_leg(m, a.fields, a.launches, a.rounds, "cuda:0", not a.no_mirror)
                                           for m in ("sa", "cma", "dma")}}
    if not a.skip_rollout:
        res["rollout"] = {"steps": a.rollout_steps, "env_id": "sa",
                          "ou": rollout_leg("ou", a.fields, a.rollout_steps),
                          "self": rollout_leg("self", a.fields, a.rollout_steps)}
        res["rollout"]["self_over_ou"] = res["rollout"]["self"]["rollout_s"] / res["rollout"]["ou"]["rollout_s"]
    if a.mirror_rollout:
        res["mirror_rollout"] = {m: mirror_rollout_leg(m, a.fields // 2 if m == "dma" else a.fields, a.rollout_steps)
                                 for m in a.mirror_rollout.split(",")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
