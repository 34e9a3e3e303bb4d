"""The tracking filter over a long horizon, on the CPU: numpy only, no GPU.

tests/test_track_cpu.py measures the filter against the C oracle on contact-free scenes, which last four steps -- the
filter's start-up transient.  This script runs vss_amd.track.reference_track for `--steps` calls on synthetic
contact-free rows whose truth is the drive model itself (estimate.predict_rows, one step per call, the own robots'
commands redrawn every 10 steps; one opponent re-aimed every 10 steps and the ball kicked every 25, which the model
does not know), with Gaussian noise of the given sigmas on every pose, and prints the RMS error of the filtered row
against the truth over the raw row's, per class and kind of body, after the first `--skip` calls."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rsoccer-isaac-cleanrl_amd"))

F = np.float32


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=256)
    p.add_argument("--steps", type=int, default=120)
    p.add_argument("--skip", type=int, default=20)
    p.add_argument("--delay", type=int, default=0)
    p.add_argument("--sigmas", type=float, nargs=4, default=(0.002, 0.05, 0.02, 0.5), metavar=("POS", "VEL", "ANG", "ANGVEL"))
    p.add_argument("--gains", type=float, nargs=3, default=(0.2, 0.5, 0.5), metavar=("TEAM", "OPP", "BALL"))
    p.add_argument("--gates", type=float, nargs=2, default=(0.03, 0.5), metavar=("POS", "VEL"))
    p.add_argument("--seed", type=int, default=1)
    args = p.parse_args()
    from vss_amd import estimate as E
    from vss_amd import track as T
    from vss_amd.perceive import ACTION_FLOATS
    g = np.random.default_rng(args.seed)
    m, D = args.rows, args.delay
    acts = list(ACTION_FLOATS)
    bodies = [(0, False)] + [(b, True) for b in E.OWN + E.OPPONENTS]
    truth = np.zeros((m, 52), F)
    for b, robot in bodies:
        truth[:, b:b + 2] = g.uniform(-0.2, 0.2, (m, 2))
        if robot:
            yaw = g.uniform(-np.pi, np.pi, m)
            truth[:, b + 4], truth[:, b + 5] = np.cos(yaw), np.sin(yaw)
    sig = dict(zip(("pos", "vel", "ang", "angvel"), args.sigmas))
    params = T.Params(*args.gains, *args.gates)
    shape = (1, m, 1)
    est, hist, age = np.zeros(shape + (52,), F), np.zeros((D,) + shape + (6,), F), np.zeros(shape, np.int32)
    none = np.zeros(m, np.int64)
    frames, err = [], {}
    cmd = np.zeros((m, 6), F)
    for t in range(args.steps):
        if t % 10 == 0:
            cmd = g.uniform(-0.3, 0.3, (m, 6)).astype(F)  # slow enough to stay on the field for the whole run
        if t:
            truth[:, acts] = cmd
            truth = E.predict_rows(truth, 1, cmd[:, None, :])
        if t % 10 == 0:  # opponent 0 re-aimed: a new velocity and yaw rate the model cannot know
            truth[:, 33:35] = g.uniform(-0.3, 0.3, (m, 2))
            truth[:, 37] = g.uniform(-5, 5, m)
        if t % 25 == 0:  # the ball kicked
            truth[:, 2:4] = g.uniform(-0.5, 0.5, (m, 2))
        truth[:, acts] = cmd
        frames.append(truth.copy())
        late = frames[max(t - D, 0)].copy()  # perception: the frame of D calls ago with the current commands
        late[:, acts] = cmd
        seen = late.copy()
        for b, robot in bodies:
            seen[:, b:b + 2] += g.normal(0, sig["pos"], (m, 2)).astype(F)
            seen[:, b + 2:b + 4] += g.normal(0, sig["vel"], (m, 2)).astype(F)
            if robot:
                e = g.normal(0, sig["ang"], m)
                c, s = seen[:, b + 4].copy(), seen[:, b + 5].copy()
                seen[:, b + 4], seen[:, b + 5] = c * np.cos(e) - s * np.sin(e), s * np.cos(e) + c * np.sin(e)
                seen[:, b + 6] += g.normal(0, sig["angvel"], m).astype(F)
        rows = seen.reshape(shape + (52,))
        out, _ = T.reference_track(rows, None if t == 0 else rows, none, est, hist, age, t, D, params)
        if t >= args.skip:
            kinds = dict(team=E.OWN, opp=E.OPPONENTS, ball=(0,))
            for kind, bases in kinds.items():
                classes = dict(position=(0, 1), velocity=(2, 3)) if kind == "ball" else \
                    dict(position=(0, 1), velocity=(2, 3), heading=(4, 5), yaw_rate=(6,))
                for name, cols in classes.items():
                    idx = [b + c for b in bases for c in cols]
                    raw, fil = err.setdefault((kind, name), ([], []))
                    raw.append((seen[:, idx].astype(np.float64) - late[:, idx]).ravel())
                    fil.append((out.reshape(m, 52)[:, idx].astype(np.float64) - late[:, idx]).ravel())
    print(f"rows {m}, steps {args.steps} (after the first {args.skip}), D {D}, sigmas {tuple(args.sigmas)}, params {tuple(params)}")
    for (kind, name), (raw, fil) in err.items():
        r, f = (float(np.sqrt(np.mean(np.concatenate(x) ** 2))) for x in (raw, fil))
        print(f"  {kind:5s} {name:9s} filtered {f:.4g} / raw {r:.4g}" + (f" = {f / r:.3f}" if r else ""))


if __name__ == "__main__":
    main()
