"""The scripted benchmark team (include/vss.h `vss_scripted_team`, csrc/vss_scripted.hip).

A deterministic three-role controller -- attacker, defender, keeper -- that is a pure function of robot 0's
52-float observation row of a field: no state, no random draw.  `reference_actions` below is its specification:
float32 numpy, one operation per line, in the kernel's order; the kernel equals it bit for bit
(tests/test_scripted_gpu.py).  Only + - * /, sqrt, fabs, min / max, comparisons and selects occur, every one of
them correctly rounded in both, and nothing is contracted into an FMA.

    scripted_actions(act, obs)      # act (N,3,2) written in place from obs (N,3,52) or (N,52): one launch

A benchmark opponent must not drift: VERSION names this controller, and a change of behaviour gets a new number
(and a new branch in the kernel) instead of replacing 1.

Row layout (envs/vss.py compute_obs): ball x y vx vy [0:4]; own robot k at 4 + 9 k: x y vx vy cos sin w a0 a1
(robot 0's row lists the own robots as 0, 1, 2); opponent k at 31 + 7 k.  The controller reads the ball's
position and the own robots' positions and headings -- 14 of the 52 floats; both teams attack +x in their frame.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

VERSION = N.SCRIPTED_VERSION
F = np.float32

# every constant of controller 1
GOAL_X = F(0.75)        # the opponent goal's centre (GOAL_X, 0)
PUSH = F(0.15)          # behind the ball: aim this far past it along g
BEHIND = F(-0.10)       # otherwise: aim this far short of it along g
LATERAL = F(0.05)       # "behind" needs |lateral offset| below this
KEEPER_X, KEEPER_Y = F(-0.69), F(0.17)
DEFENDER_X, DEFENDER_Y = F(-0.30), F(0.35)
DEFENDER_ATTACKS = F(-0.1)  # the defender is a second attacker while ball_x < this
EPS = F(1e-6)
K_SLOW = F(8.0)         # speed factor min(1, K_SLOW * dist)
K_TURN = F(1.2)
ONE, ZERO = F(1.0), F(0.0)


def _clamp(x, lo, hi):
    return np.minimum(np.maximum(x, lo), hi)


def _attack_target(bx, by, px, py):
    """Behind the ball along g (the unit vector ball -> goal) and laterally close: push through; else get behind."""
    gx = GOAL_X - bx
    gy = ZERO - by
    gn = np.sqrt(gx * gx + gy * gy) + EPS
    hx = gx / gn
    hy = gy / gn
    rx = px - bx
    ry = py - by
    along = rx * hx + ry * hy
    lat = ry * hx - rx * hy
    k = np.where((along < ZERO) & (np.abs(lat) < LATERAL), PUSH, BEHIND).astype(F)
    return bx + k * hx, by + k * hy


def _go_to(px, py, c, s, tx, ty):
    """(left, right) wheels of a robot at p with heading (c, s) towards t; it reverses rather than turning round."""
    dx = tx - px
    dy = ty - py
    ef = dx * c + dy * s
    el = dy * c - dx * s
    dist = np.sqrt(ef * ef + el * el) + EPS
    sg = np.where(ef < ZERO, -ONE, ONE).astype(F)
    v = (sg * (np.abs(ef) / dist)) * np.minimum(ONE, K_SLOW * dist)
    w = (K_TURN * (sg * el)) / dist
    return _clamp(v - w, -ONE, ONE), _clamp(v + w, -ONE, ONE)


def reference_actions(obs_row0) -> np.ndarray:
    """(N, 3, 2) float32 wheel commands of controller 1 from robot 0's rows (N, 52) -- the specification."""
    o = np.ascontiguousarray(obs_row0, dtype=F)
    if o.ndim != 2 or o.shape[1] != 52:
        raise ValueError(f"reference_actions takes robot 0's rows (N, 52), got {o.shape}")
    bx, by = o[:, 0], o[:, 1]
    out = np.empty((o.shape[0], 3, 2), F)
    for r in range(3):
        px, py, c, s = (o[:, 4 + 9 * r + q] for q in (0, 1, 4, 5))
        if r == 2:    # keeper
            tx, ty = np.full_like(bx, KEEPER_X), _clamp(by, -KEEPER_Y, KEEPER_Y)
        else:
            tx, ty = _attack_target(bx, by, px, py)
            if r == 1:  # defender, a second attacker while the ball is deep in the own half
                home = ~(bx < DEFENDER_ATTACKS)
                tx = np.where(home, DEFENDER_X, tx).astype(F)
                ty = np.where(home, _clamp(by, -DEFENDER_Y, DEFENDER_Y), ty).astype(F)
        out[:, r, 0], out[:, r, 1] = _go_to(px, py, c, s, tx, ty)
    return out


def mirror_rows_y(rows) -> np.ndarray:
    """The rows reflected in y: y, v_y, sin and w negated for the ball and all six robots, the own robots'
    last-action pairs swapped.  The controller then swaps each robot's two wheels and changes nothing else."""
    m = np.array(rows, dtype=F, copy=True)
    m[:, [1, 3]] *= F(-1)
    for k in range(3):
        b = 4 + 9 * k
        m[:, [b + 1, b + 3, b + 5, b + 6]] *= F(-1)
        m[:, [b + 7, b + 8]] = m[:, [b + 8, b + 7]]
        b = 31 + 7 * k
        m[:, [b + 1, b + 3, b + 5, b + 6]] *= F(-1)
    return m


def field_strides(act: torch.Tensor, obs: torch.Tensor):
    """(obs_field_stride, act_field_stride) in floats as the ABI takes them, from the tensors' own strides; a
    layout the ABI cannot express raises a ValueError naming the stride."""
    if obs.dim() not in (2, 3) or obs.shape[-1] != 52 or (obs.dim() == 3 and obs.shape[1] != 3):
        raise ValueError(f"obs must be (N, 3, 52) or robot 0's rows (N, 52), got {tuple(obs.shape)}")
    n = obs.shape[0]
    if tuple(act.shape) != (n, 3, 2):
        raise ValueError(f"act must be ({n}, 3, 2), got {tuple(act.shape)}")
    if obs.dtype != torch.float32 or act.dtype != torch.float32:
        raise ValueError(f"obs and act must be float32, got {obs.dtype} and {act.dtype}")
    if obs.stride(-1) != 1:
        raise ValueError(f"obs: a row's 52 floats must be adjacent, got element stride {obs.stride(-1)}")
    if act.stride(2) != 1 or act.stride(1) != 2:
        raise ValueError(f"act: a field's six floats must be adjacent, got strides {tuple(act.stride())}")
    so, sa = (obs.stride(0), act.stride(0)) if n > 1 else (max(obs.stride(0), 52) // 4 * 4, max(act.stride(0), 6) // 2 * 2)
    if so < 52 or so % 4:
        raise ValueError(f"obs: field stride {so} floats; the kernel needs a multiple of 4 that is at least 52")
    if sa < 6 or sa % 2:
        raise ValueError(f"act: field stride {sa} floats; the kernel needs a multiple of 2 that is at least 6")
    return int(so), int(sa)


@torch.no_grad()
def scripted_actions(act: torch.Tensor, obs: torch.Tensor, version: int = VERSION) -> torch.Tensor:
    """Write controller `version`'s (N,3,2) actions into `act` in place from `obs` ((N,3,52), of which only
    [:, 0] is read, or (N,52)): one vss_scripted_team launch on the current stream, no host sync.  The views
    play.py hands over -- one team's half of (N,2,3,52) and (N,2,3,2) -- are taken as they are.  CPU tensors
    go through reference_actions."""
    so, sa = field_strides(act, obs)
    if act.device != obs.device:
        raise ValueError(f"act is on {act.device}, obs on {obs.device}")
    if obs.shape[0] == 0:
        return act
    if act.device.type == "cpu":
        if version != VERSION:
            raise ValueError(f"scripted controller version {version!r}: this build has version {VERSION}")
        rows = obs[:, 0] if obs.dim() == 3 else obs
        act.copy_(torch.from_numpy(reference_actions(rows.numpy())))
        return act
    lib = N.load()
    N.check(lib.vss_scripted_team(N.stream_of(act.device), obs.shape[0], int(version), obs.data_ptr(), so,
                                  act.data_ptr(), sa), "vss_scripted_team")
    return act
