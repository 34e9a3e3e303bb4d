#!/usr/bin/env python3
"""Time the opponent league's kernels and write one JSON record to profiles/league_bench.json.

    python tools/league_bench.py --build-variant     # once, needs hipcc: the other block mapping (below)
    python tools/league_bench.py [--launches 200] [--rounds 7] [--skip-rollout] [--out profiles/league_bench.json]

Legs:
 1. vss_actor_forward_grouped with 1, 4 and 8 groups at 12,288 rows (policy_kernel's 64-row workgroups: a
    4,095-env self-play run) and 4,096 rows (the split kernel), next to one vss_actor_forward over all rows
    (one weight set: the floor) and to `count` back-to-back vss_actor_forward launches on the row slices
    (what a pool would do without the grouped entry).  Both block-to-row-block mappings are timed: the
    library's (VSS_GROUPED_XCD_MAP as built, 0 = plain) and the other one from a variant build of
    csrc/vss_policy.hip alone, tools/_ab/libvss_policy_xcd<0|1>.so (--build-variant).
 2. 196,608 opponent rows (65,536 fields, x3): OpponentPool's GEMM-chain path with 8 slots -- as assign() deals
    them (half the slots the newest: one chain for them) and with 8 distinct snapshots -- next to
    SnapshotOpponent's single chain.
 3. vss_match_tally at 65,536 fields: the usual few finished fields (1/400) and every field finished.
 4. A 128-step SA rollout of train() with --opponent pool next to --opponent self, at 4,095 and 65,536 envs
    (rollout_s of the second update).

Times are HIP events around `launches` back-to-back launches after a warm-up; the arms of a leg alternate
`rounds` times and the median window is reported with min and max (the spread between windows is the
resolution of every comparison here).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "rsoccer-isaac-cleanrl_amd")
AB = os.path.join(REPO, "tools", "_ab")
sys.path.insert(0, PKG)


def variant_path(xcd: int) -> str:
    return os.path.join(AB, f"libvss_policy_xcd{xcd}.so")


def build_variants():
    os.makedirs(AB, exist_ok=True)
    for xcd in (0, 1):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                        "-Wall", "-mllvm", "-unroll-threshold=1000000", f"-DVSS_GROUPED_XCD_MAP={xcd}", "-shared", "-o",
                        variant_path(xcd), os.path.join(PKG, "csrc", "vss_policy.hip")], check=True)
        print("built", variant_path(xcd))


def summary(ts):
    return {"us": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--build-variant", action="store_true")
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--skip-rollout", action="store_true")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "league_bench.json"))
    a = p.parse_args()
    if a.build_variant:
        build_variants()
        return

    import torch

    import ppo_continuous_action_isaacgym as P
    from vss_amd import _native as N
    from vss_amd.opponent import OpponentPool, SnapshotOpponent

    P.disable_graph_packet_capture()
    dev = N.require_device("cuda:0")  # a measurement without the GPU fails; it does not fall back
    lib, stream = N.load(), N.stream_of(dev)
    u64, i64, i32, VP = ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p

    def window(fn, launches=a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(launches):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches  # us per call

    def rotate(arms: dict, launches=a.launches) -> dict:
        for fn in arms.values():
            for k in range(20):
                fn(k)
        torch.cuda.synchronize()
        ts = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                ts[k].append(window(fn, launches))
        return {k: summary(v) for k, v in ts.items()}

    res = {"device": torch.cuda.get_device_name(0), "launches_per_window": a.launches, "rounds": a.rounds}

    # ---- 1. grouped forward --------------------------------------------------------------------------------
    variants = {}
    for xcd in (0, 1):
        if os.path.exists(variant_path(xcd)):
            L = ctypes.CDLL(variant_path(xcd))
            L.vss_actor_forward_grouped.argtypes = [VP, i64, i32, VP, VP, u64, u64, VP, VP]
            L.vss_actor_forward_grouped.restype = ctypes.c_int
            variants[xcd] = L
    n_act = 2
    size = lib.vss_mlp_packed_size(n_act)
    gen = torch.Generator(device=dev).manual_seed(1)
    packed = [torch.randn(size, device=dev, generator=gen) * 0.05 for _ in range(8)]
    logstd = [torch.full((n_act,), -0.5 - 0.1 * i, device=dev) for i in range(8)]
    res["forward"] = {"variants_timed": sorted(variants), "n_act": n_act}
    for rows in (12288, 4096):
        obs = torch.randn(rows, 52, device=dev, generator=gen) * 0.7
        act, mean = torch.empty(rows, n_act, device=dev), torch.empty(rows, n_act, device=dev)
        leg = {}
        for count in (1, 4, 8):
            gr = rows // count
            g = N.VssActorGroups()
            g.count, g.group_rows = count, gr
            for i in range(count):
                g.actor_packed[i], g.logstd[i] = packed[i].data_ptr(), logstd[i].data_ptr()
            gp = ctypes.byref(g)
            o, ao, p0, l0 = obs.data_ptr(), act.data_ptr(), packed[0].data_ptr(), logstd[0].data_ptr()

            def check(rc):
                if rc != 0:
                    raise RuntimeError(f"launch failed ({rc})")

            def single(k):
                check(lib.vss_actor_forward(stream, rows, n_act, o, p0, l0, 7, k + 1, ao, None))

            def back_to_back(k):
                for i in range(count):
                    check(lib.vss_actor_forward(stream, gr, n_act, o + i * gr * 52 * 4, packed[i].data_ptr(),
                                                logstd[i].data_ptr(), 7, k + 1, ao + i * gr * n_act * 4, None))

            def grouped(k):
                check(lib.vss_actor_forward_grouped(stream, rows, n_act, o, gp, 7, k + 1, ao, None))

            arms = {"single_forward_all_rows": single, "back_to_back_slices": back_to_back, "grouped_library": grouped}
            for xcd, L in variants.items():
                arms[f"grouped_xcd_map_{xcd}"] = (lambda L: lambda k: check(
                    L.vss_actor_forward_grouped(stream, rows, n_act, o, gp, 7, k + 1, ao, None)))(L)
            leg[f"count_{count}"] = rotate(arms)
            # the mappings agree with the library bit for bit
            grouped(0)
            want = act.clone()
            for xcd, L in variants.items():
                act.zero_()
                check(L.vss_actor_forward_grouped(stream, rows, n_act, o, gp, 7, 1, ao, None))
                if not torch.equal(act, want):
                    raise RuntimeError(f"mapping {xcd} changes the output at rows {rows} count {count}")
        res["forward"][f"rows_{rows}"] = leg

    # ---- 2. the chain path at 196,608 rows -----------------------------------------------------------------
    from collections import namedtuple

    import numpy as np
    from envs._gym import Box
    Env = namedtuple("Env", ["single_observation_space", "single_action_space"])
    n = 65536
    agents = []
    for i in range(8):
        torch.manual_seed(i)
        agents.append(P.Agent(Env(Box(-np.inf, np.inf, (52,)), Box(-1.0, 1.0, (2,)))).to(dev))
    pool = OpponentPool(agents[0], "x3", n, slots=8, seed=3)
    for v, ag in enumerate(agents[1:], 1):
        pool.add(ag, v)
    snap = SnapshotOpponent(agents[0], "x3", seed=3)
    obs3 = torch.randn(n, 3, 52, device=dev) * 0.7
    act3 = torch.zeros(n, 3, 2, device=dev)
    dealt = pool.assign()
    chain = {"rows": pool.rows, "count": pool.count, "group_rows": pool.group_rows, "dealt_versions": dealt}
    t = rotate({"snapshot_opponent": lambda k: snap(act3, obs3), "pool_as_dealt": lambda k: pool(act3, obs3)}, 50)
    pool.hold(pool.snapshots[:8])
    t.update(rotate({"pool_8_distinct": lambda k: pool(act3, obs3)}, 50))
    chain.update(t)
    res["chain_196608_rows"] = chain
    del pool, snap, obs3, act3

    # ---- 3. the tally ---------------------------------------------------------------------------------------
    rew = torch.randn(n, 4, device=dev)
    rew[:, 0] = torch.randint(-1, 2, (n,), device=dev).float() * 10
    prog = torch.randint(1, 401, (n,), device=dev).float()
    tally = torch.zeros(8, 4, dtype=torch.long, device=dev)
    few = (torch.rand(n, device=dev) < 1 / 400).long()
    every = torch.ones(n, dtype=torch.long, device=dev)

    def tally_fn(d):
        return lambda k: lib.vss_match_tally(stream, n, 1, n // 8, 8, rew.data_ptr(), d.data_ptr(), prog.data_ptr(),
                                             tally.data_ptr())
    res["tally_65536_fields"] = rotate({"dones_1_in_400": tally_fn(few), "all_done": tally_fn(every)})

    # ---- 4. rollouts ------------------------------------------------------------------------------------------
    if not a.skip_rollout:
        res["rollout"] = {"steps": 128, "env_id": "sa"}
        for envs in (4095, 65536):
            leg = {}
            for opp in ("self", "pool"):
                args = P.parse_args(["--env-id", "sa", "--num-envs", str(envs), "--num-steps", "128", "--num-updates", "3",
                                     "--log", "false", "--opponent", opp])
                _, hist = P.train(args)
                leg[opp] = {"rollout_s": [h["rollout_s"] for h in hist], "update_s": hist[-1]["update_s"],
                            "pool_versions": hist[-1].get("opponent_pool_versions")}
            leg["pool_over_self"] = min(leg["pool"]["rollout_s"][1:]) / min(leg["self"]["rollout_s"][1:])
            res["rollout"][f"envs_{envs}"] = leg

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
