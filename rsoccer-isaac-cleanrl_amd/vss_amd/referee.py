"""The referee (include/vss.h `vss_referee`, csrc/vss_referee.hip).

Set plays (setplay.py) start an episode from a real match's restarts; inside an episode nothing was ever whistled.  The
referee calls three things mid-episode: a free ball when the ball has been stuck for `stall_steps` steps, a penalty when
two defenders have stood in their own goal area with the ball for `area_steps` steps, and a goal kick when two
attackers have.  A whistled field is placed again from the matching play -- setplay.py's placement arithmetic with the
mirrorings decided by the verdict, not drawn -- and its dof velocities and observation rows are rewritten.  A stoppage
is not a done: progress_buf, reset_buf, the rewards and terminal_observation are never touched.  One launch per call,
after the step and after the set plays; `reference_referee` below is its specification: float32 numpy, one operation
per line, in the kernel's order, nothing contracted; the kernel equals it bit for bit (tests/test_referee_gpu.py).

    ref = Referee(n_fields, RefTable(), Params.of(stall_steps=100, area_steps=20), seed, device)
    ref.call(env.state, env.dof_velocity_buf, [(obs, view_sa())], env.reset_buf)   # one launch, no host sync

Per call t and field f, with counters (n, 4) int32 = stall, defend, attack, stops:

    a done field:  the four counters = 0, verdict[f] = -1, nothing else (the reset or the set-play stager owns it)
    v2 = bvx * bvx + bvy * bvy;  stall = v2 < stall_speed_sq ? min(stall + 1, 1 << 30) : 0
    in_area = |bx| > area_x and |by| < area_y;  side = 0 if bx < 0 else 1       # 0: blue's own area (blue defends -x)
    a robot is inside when |x| > area_x and |y| < area_y and (x < 0) == (bx < 0);  nb, ny: blue and yellow robots inside
    def_n = nb if side == 0 else ny;  att_n the other
    defend = in_area and def_n >= 2 ? min(defend + 1, 1 << 30) : 0;  attack likewise with att_n
    while max_stops == 0 or stops < max_stops, the first that holds:
        area_steps > 0 and defend >= area_steps    a penalty for the attackers     4 (blue's, side 1)   5 (yellow's)
        area_steps > 0 and attack >= area_steps    a goal kick for the defenders   6 (blue's, side 0)   7 (yellow's)
        stall_steps > 0 and stall >= stall_steps   a free ball   0 (bx >= 0, by >= 0)  1 (by < 0)  2 (bx < 0)  3 (both)
    flips: free ball flip_x = bx < 0, flip_y = by < 0; penalty flip_x = (code 5); goal kick flip_x = (code 7), flip_y = by < 0
    placement: reference_setplay's, with the words of Philox4x32-10, key (seed lo, seed hi), counter
        (f, t, 11 << 24, 1 + e): block 1 the ball (x y vx vy), block 1 + e entity e = 1..6 (x y yaw); block 0 is not used
    written: the 58 state channels, dof_vel's twelve floats +0.0, the rows of every view (own-action floats +0.0),
        stall = defend = attack = 0, stops += 1, verdict[f] = code, counts[code] += 1

The entry point is libvss_amd.so's, bound from include/vss.h by vss_amd/_native.py like every other: the structs, the
constants and the loader here are `_native`'s under the module's own names, and the views and entities are the set
plays' (one struct each in the header).  There is no fallback: a missing or stale library raises.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N
from . import channel
from . import setplay as S
from .perceive import NUM_OBS, _philox, _sincos_small
# View and the view_* constructors are the set plays' own, re-exported: the two units rewrite the same rows
from .setplay import (CH_RQW, CH_RQX, CH_RQY, CH_RQZ, CH_RVX, CH_RVY, CH_RW, CH_RX, CH_RY, PI, TWO_PI, View, _jitter,
                      full_rows_of_state, view_dma, view_full, view_mirror, view_opponent, view_sa)

F = np.float32
U32 = np.uint32

CODES = N.REFEREE_CODES
VssRefereePlay = N.VssRefereePlay
VssRefereeTable = N.VssRefereeTable
VssRefereeParams = N.VssRefereeParams
VssRefereeEntity = S.VssSetplayEntity  # the header has one entity and one view struct: the set plays'
VssRefereeView = S.VssSetplayView
load = N.load  # the one library's loader under the module's own name, as before

PURPOSE = 11          # the Philox counter's purpose byte (the step 0..6, perception 7, actuation 8 and 9, set plays 10)
CAP = 1 << 30         # a counter stops counting here
PLAYS = ("free_ball", "penalty", "goal_kick")  # the table's three plays, by their names in setplay.BUILTIN
# the training record's entries (per-update differences of counts): "for" favours blue
RECORD = {"free_ball": (0, 1, 2, 3), "penalty_for": (4,), "penalty_against": (5,), "goal_kick_for": (6,),
          "goal_kick_against": (7,)}

# ---- parameters and the table -------------------------------------------------------------------------------------------
class Params(NamedTuple):
    """include/vss.h vss_referee_params, in its order.  `of` builds one from a speed, a depth and a width."""
    stall_speed_sq: float = float(F(0.05) * F(0.05))
    area_x: float = 0.60
    area_y: float = 0.35
    stall_steps: int = 0
    area_steps: int = 0
    max_stops: int = 0

    @classmethod
    def of(cls, stall_steps: int = 0, stall_speed: float = 0.05, area_steps: int = 0, area_depth: float = 0.15,
           area_width: float = 0.70, max_stops: int = 0) -> "Params":
        """From the flags' units: the threshold is F(v) * F(v); the area is `area_depth` deep in front of each goal line
        (|x| = 0.75) and `area_width` wide."""
        v = F(stall_speed)
        return cls(float(v * v), 0.75 - float(area_depth), float(area_width) / 2.0, int(stall_steps), int(area_steps),
                   int(max_stops)).validate()

    def any(self) -> bool:
        return self.stall_steps > 0 or self.area_steps > 0

    def validate(self) -> "Params":
        """ValueError for what vss_referee refuses with VSS_E_ARG (in double on the float32 values)."""
        for name in ("stall_steps", "area_steps", "max_stops"):
            v = getattr(self, name)
            if int(v) != v or not 0 <= int(v) < 2 ** 31:
                raise ValueError(f"referee: {name} must be an integer >= 0, got {v}")
        sq, ax, ay = (float(F(v)) for v in (self.stall_speed_sq, self.area_x, self.area_y))
        if not (math.isfinite(sq) and sq >= 0.0):
            raise ValueError(f"referee: stall_speed_sq must be finite and >= 0, got {self.stall_speed_sq}")
        if not 0.0 < ax < 0.75:
            raise ValueError(f"referee: area_x must be inside (0, 0.75), got {self.area_x}")
        if not 0.0 < ay <= 0.65:
            raise ValueError(f"referee: area_y must be inside (0, 0.65], got {self.area_y}")
        return self

    def c_params(self) -> "VssRefereeParams":
        return VssRefereeParams(float(F(self.stall_speed_sq)), float(F(self.area_x)), float(F(self.area_y)),
                                int(self.stall_steps), int(self.area_steps), int(self.max_stops))


class RefTable:
    """The referee's three plays -- free ball, penalty, goal kick -- each written as blue's own piece in the +y half,
    exactly as setplay.BUILTIN writes them (the defaults).  There are no weights and no flip probabilities here: the
    verdict decides both."""

    def __init__(self, free_ball=None, penalty=None, goal_kick=None):
        given = (free_ball, penalty, goal_kick)
        self.plays = tuple(S.Play(*(S.BUILTIN[name] if p is None else p)) for name, p in zip(PLAYS, given))
        self.validate()

    @classmethod
    def of_library(cls, library: dict | None) -> "RefTable":
        """The plays named free_ball, penalty and goal_kick of a library (setplay.load_file), else the built-ins."""
        library = library or {}
        return cls(*(library.get(name) for name in PLAYS))

    def validate(self, params: Params | None = None) -> "RefTable":
        """Every rule of setplay.Table.validate for each play, and -- so that a restart cannot re-trigger its own
        call -- a free-ball or penalty play whose ball anchor +- r_pos can lie inside a goal area is refused."""
        params = Params() if params is None else params
        ax, ay = float(F(params.area_x)), float(F(params.area_y))
        for k, p in enumerate(self.plays):
            S.Table([p._replace(weight=1.0, p_flip_x=0.0, p_flip_y=0.0)], 1.0)
            x, y, _, r, _ = (float(v) for v in np.asarray(p.entities[0], dtype=F))
            if k < 2 and abs(x) + r > ax and abs(y) - r < ay:
                raise ValueError(f"referee: the ball of {PLAYS[k]} ({x:.3f}, {y:.3f}) +- {r:.3f} can lie inside a goal area "
                                 f"(|x| > {ax:.3f}, |y| < {ay:.3f}): the restart would be whistled again")
        return self

    def arrays(self) -> dict:
        """ent (3, 7, 5), vel (3, 3) float32, as the kernel gets them."""
        return dict(ent=np.asarray([p.entities for p in self.plays], dtype=F),
                    vel=np.asarray([p.ball_vel for p in self.plays], dtype=F))

    def c_table(self) -> "VssRefereeTable":
        a = self.arrays()
        t = VssRefereeTable()
        for k in range(3):
            p = t.play[k]
            for e in range(7):
                p.e[e].x, p.e[e].y, p.e[e].yaw, p.e[e].r_pos, p.e[e].r_yaw = (float(v) for v in a["ent"][k, e])
            p.ball_vx, p.ball_vy, p.r_vel = (float(v) for v in a["vel"][k])
        return t


def params_of_args(args) -> "Params | None":
    """The parameters of --ref-*; None with --ref-stall-steps and --ref-area-steps both 0, the default (absent flags
    are their defaults)."""
    from .checkpoint import REFEREE_DEFAULTS
    v = {k: (d if getattr(args, k, None) is None else getattr(args, k)) for k, d in REFEREE_DEFAULTS.items()}
    if int(v["ref_stall_steps"]) < 0 or int(v["ref_area_steps"]) < 0:
        raise ValueError("--ref-stall-steps and --ref-area-steps must be >= 0")
    if int(v["ref_stall_steps"]) == 0 and int(v["ref_area_steps"]) == 0:
        return None
    return Params.of(v["ref_stall_steps"], v["ref_stall_speed"], v["ref_area_steps"], v["ref_area_depth"],
                     v["ref_area_width"], v["ref_max_stops"])


def table_of_args(args) -> RefTable:
    """--setplay-file, if given, supplies free_ball, penalty and goal_kick by name in place of the built-ins."""
    path = getattr(args, "setplay_file", None) or None
    return RefTable.of_library(S.load_file(path) if path else None)


def referee_of_args(args, n_fields: int, device, offset: int = 0) -> "Referee | None":
    """The referee of --ref-* for `n_fields` fields; None when the flags leave it off."""
    params = params_of_args(args)
    if params is None:
        return None
    return Referee(n_fields, table_of_args(args), params, referee_seed(getattr(args, "seed", None), offset), device)


def referee_seed(seed, offset: int = 0) -> int:
    """The referee's Philox key from --seed and the rank, built as setplay_seed with a constant of its own; `offset`
    separates the arena's referee (1) from the training's."""
    return ((int(seed or 0) * 1000003 + int(os.environ.get("RANK", 0))) * 2654435761 + 0x4EF_E4EE + int(offset)) \
        & 0xFFFFFFFFFFFFFFFF


# ---- the specification ----------------------------------------------------------------------------------------------
def _bump(holds, c):
    return np.where(holds, np.minimum(c + np.int32(1), np.int32(CAP)), np.int32(0)).astype(np.int32)


def reference_referee(table: RefTable, params: Params, seed: int, call: int, done, state: np.ndarray, dof_vel: np.ndarray,
                      counters: np.ndarray, views=(), counts=None, verdict=None):
    """One call -- the specification.  done (n,) or None (no field is done); state (58, n) float32, dof_vel
    (n, 2, 3, 2) float32, counters (n, 4) int32, each view a pair (rows (R, 52) float32, View), counts (8,) int64 and
    verdict (n,) int32 are updated in place.  Returns the indices of the whistled fields."""
    if state.dtype != F or state.ndim != 2 or state.shape[0] != N.STATE_CHANNELS:
        raise ValueError(f"state must be float32 (58, n), got {state.dtype} {state.shape}")
    n = state.shape[1]
    if counters.dtype != np.int32 or counters.shape != (n, 4) or dof_vel.dtype != F or dof_vel.size != n * 12:
        raise ValueError("counters must be int32 (n, 4) and dof_vel float32 (n, 2, 3, 2)")
    prm = params.c_params()  # the float32 values the kernel gets
    sq, ax, ay = F(prm.stall_speed_sq), F(prm.area_x), F(prm.area_y)
    done = np.zeros(n, bool) if done is None else np.asarray(done).reshape(n) != 0
    bx, by, bvx, bvy = state[0], state[1], state[2], state[3]
    # 1. the stall
    v2 = bvx * bvx
    v2 = v2 + bvy * bvy
    stall = _bump(v2 < sq, counters[:, 0])
    # 2. the area tests
    left, low = bx < F(0.0), by < F(0.0)
    in_area = (np.abs(bx) > ax) & (np.abs(by) < ay)
    nb, ny = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for r in range(6):
        x, y = state[CH_RX + r], state[CH_RY + r]
        inside = (np.abs(x) > ax) & (np.abs(y) < ay) & ((x < F(0.0)) == left)
        if r < 3:
            nb += inside
        else:
            ny += inside
    def_n, att_n = np.where(left, nb, ny), np.where(left, ny, nb)
    # 3. the area counters
    defend = _bump(in_area & (def_n >= 2), counters[:, 1])
    attack = _bump(in_area & (att_n >= 2), counters[:, 2])
    stops = counters[:, 3].copy()
    # 4. eligibility, 5. precedence, 6. the codes
    may = np.ones(n, bool) if prm.max_stops == 0 else stops < prm.max_stops
    code = np.full(n, -1, np.int32)
    free = (prm.stall_steps > 0) & (stall >= prm.stall_steps)
    code = np.where(free, np.where(left, 2, 0) + np.where(low, 1, 0), code)
    kick = (prm.area_steps > 0) & (attack >= prm.area_steps)
    code = np.where(kick, np.where(left, 6, 7), code)
    pen = (prm.area_steps > 0) & (defend >= prm.area_steps)
    code = np.where(pen, np.where(left, 5, 4), code)
    code = np.where(may & ~done, code, -1).astype(np.int32)
    whistled = code >= 0
    zero = done | whistled
    counters[:, 0] = np.where(zero, 0, stall)
    counters[:, 1] = np.where(zero, 0, defend)
    counters[:, 2] = np.where(zero, 0, attack)
    counters[:, 3] = np.where(done, 0, np.where(whistled, stops + np.int32(1), stops))
    if verdict is not None:
        verdict[:] = code
    f = np.nonzero(whistled)[0]
    if f.size == 0:
        return f
    # 7. the placement: reference_setplay's arithmetic with the flips decided by the verdict
    cf = code[f]
    sel = np.where(cf < 4, 0, np.where(cf < 6, 1, 2))
    flip_x = np.where(cf < 4, left[f], (cf == 5) | (cf == 7))
    flip_y = np.where(sel == 1, False, low[f])
    a = table.arrays()
    ent, vel = a["ent"][sel], a["vel"][sel]            # (m, 7, 5), (m, 3)
    k0, k1 = U32(int(seed) & 0xFFFFFFFF), U32((int(seed) >> 32) & 0xFFFFFFFF)
    t = U32(int(call) & 0xFFFFFFFF)

    def words(block):
        return _philox(k0, k1, f.astype(np.int64).astype(U32), t, U32(PURPOSE << 24), U32(block))

    w = words(1)
    px0 = ent[:, 0, 0] + _jitter(w[0], ent[:, 0, 3])
    py0 = ent[:, 0, 1] + _jitter(w[1], ent[:, 0, 3])
    pvx = vel[:, 0] + _jitter(w[2], vel[:, 2])
    pvy = vel[:, 1] + _jitter(w[3], vel[:, 2])
    py0 = np.where(flip_y, -py0, py0)
    pvy = np.where(flip_y, -pvy, pvy)
    px0 = np.where(flip_x, -px0, px0)
    pvx = np.where(flip_x, -pvx, pvx)
    px, py, qz, qw = (np.empty((f.size, 6), F) for _ in range(4))
    for e in range(1, 7):
        w = words(1 + e)
        x = ent[:, e, 0] + _jitter(w[0], ent[:, e, 3])
        y = ent[:, e, 1] + _jitter(w[1], ent[:, e, 3])
        yaw = ent[:, e, 2] + _jitter(w[2], ent[:, e, 4])
        y = np.where(flip_y, -y, y)
        yaw = np.where(flip_y, -yaw, yaw)
        x = np.where(flip_x, -x, x)
        yaw = np.where(flip_x, PI - yaw, yaw)
        yaw = np.where(yaw > PI, yaw - TWO_PI, yaw)
        yaw = np.where(yaw < -PI, yaw + TWO_PI, yaw)
        sz, cw = _sincos_small(F(0.5) * yaw)
        px[:, e - 1], py[:, e - 1], qz[:, e - 1], qw[:, e - 1] = x, y, sz, cw
    swap = np.array([3, 4, 5, 0, 1, 2])
    fx = flip_x[:, None]
    px, py = np.where(fx, px[:, swap], px), np.where(fx, py[:, swap], py)
    qz, qw = np.where(fx, qz[:, swap], qz), np.where(fx, qw[:, swap], qw)

    # 8. what is written
    state[0, f], state[1, f], state[2, f], state[3, f] = px0, py0, pvx, pvy
    for r in range(6):
        state[CH_RX + r, f], state[CH_RY + r, f] = px[:, r], py[:, r]
        state[CH_RQX + r, f] = state[CH_RQY + r, f] = F(0.0)
        state[CH_RQZ + r, f], state[CH_RQW + r, f] = qz[:, r], qw[:, r]
        state[CH_RVX + r, f] = state[CH_RVY + r, f] = state[CH_RW + r, f] = F(0.0)
    dof_vel.reshape(n, 12)[f] = F(0.0)
    full = full_rows_of_state(state, f)
    for rows, view in views:
        view = View(*view)
        at = view.row_index(n)[:, f]  # (n_teams, m, robots)
        for b in range(view.n_teams):
            for k in range(view.robots):
                rows[at[b, :, k]] = full[:, view.first_team + b, k]
    if counts is not None:
        counts[:CODES] += np.bincount(cf, minlength=CODES).astype(counts.dtype)
    return f


# ---- the kernel's side ----------------------------------------------------------------------------------------------
class Referee(channel.Channel):
    """The table, the parameters, the key, `counters` (n_fields, 4) int32, `counts` (8,) int64, `verdict` (n_fields,)
    int32 and the host call counter.  call() is one vss_referee launch on the current stream, with no host sync."""

    def __init__(self, n_fields: int, table: RefTable, params: Params, seed: int, device="cuda"):
        self.device = N.require_device(device)
        load()
        self.params = Params(*params).validate()
        self.n_fields, self.table, self.seed = int(n_fields), table.validate(self.params), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counters = torch.zeros((self.n_fields, 4), dtype=torch.int32, device=self.device)
        self.counts = torch.zeros(CODES, dtype=torch.long, device=self.device)
        self.verdict = torch.full((self.n_fields,), -1, dtype=torch.int32, device=self.device)
        self.call_index = 0
        self._where = self.counts.device
        self._tab, self._prm = table.c_table(), self.params.c_params()
        self._view_key, self._view_arr = None, None
        self._reported = [0] * CODES  # counts as the training record last read them

    scalars = {"call_index": int}

    def _views(self, views):
        """(the ctypes array, the count) of the call's views; checked and built once per set of buffers -- the
        wrappers hand over the same ones every step."""
        views = list(views)
        if len(views) > 2:
            raise ValueError(f"referee: at most two views per call, got {len(views)}")
        key = tuple((rows.data_ptr(), rows.numel(), rows.dtype, tuple(view)) for rows, view in views)
        if key == self._view_key:
            return self._view_arr, len(views)
        arr = (VssRefereeView * 2)()
        for i, (rows, view) in enumerate(views):
            view = View(*view)
            need = view.span(self.n_fields)
            if (rows.dtype != torch.float32 or rows.device != self._where or not rows.is_contiguous()
                    or rows.numel() < need * NUM_OBS):
                raise ValueError(f"referee: view {i} must be contiguous float32 with at least {need} rows of {NUM_OBS} "
                                 f"on {self._where}, got {tuple(rows.shape)} {rows.dtype} on {rows.device}")
            arr[i] = VssRefereeView(rows.data_ptr(), int(view.field_stride), int(view.team_stride), int(view.robots),
                                    int(view.n_teams), int(view.first_team))
        self._view_key, self._view_arr = key, arr
        return arr, len(views)

    @torch.no_grad()
    def call(self, env_state: torch.Tensor, dof_vel: torch.Tensor, views, done: torch.Tensor | None) -> None:
        """After a step (and the set plays): `done` (n_fields,) int64 marks the fields the step has just reset; None: no
        field is done."""
        if (env_state.dtype != torch.float32 or env_state.device != self._where or not env_state.is_contiguous()
                or tuple(env_state.shape) != (N.STATE_CHANNELS, self.n_fields)):
            raise ValueError(f"referee: the state must be contiguous float32 ({N.STATE_CHANNELS}, {self.n_fields}) on "
                             f"{self._where}, got {tuple(env_state.shape)} {env_state.dtype} on {env_state.device}")
        if (dof_vel.dtype != torch.float32 or dof_vel.device != self._where or not dof_vel.is_contiguous()
                or dof_vel.numel() != self.n_fields * 12):
            raise ValueError(f"referee: dof_vel must be contiguous float32 ({self.n_fields}, 2, 3, 2) on {self._where}, got "
                             f"{tuple(dof_vel.shape)} {dof_vel.dtype} on {dof_vel.device}")
        if done is not None and (done.dtype != torch.long or done.device != self._where or not done.is_contiguous()
                                 or done.numel() != self.n_fields):
            raise ValueError(f"referee: done must be contiguous int64 ({self.n_fields},) on {self._where}, got "
                             f"{tuple(done.shape)} {done.dtype}")
        arr, n_views = self._views(views)
        rc = load().vss_referee(N.stream_of(self.device), self.n_fields, ctypes.byref(self._tab), ctypes.byref(self._prm),
                                self.seed, self.call_index & 0xFFFFFFFF, N.ptr(done), 1, env_state.data_ptr(),
                                dof_vel.data_ptr(), self.counters.data_ptr(), n_views, arr, self.counts.data_ptr(),
                                self.verdict.data_ptr())
        N.check(rc, "vss_referee")
        self.call_index += 1

    def restart(self, call_index: int = 0) -> None:
        """Counters, counts and verdicts as new, the call index as given: the arena's, before every play."""
        self.counters.zero_()
        self.counts.zero_()
        self.verdict.fill_(-1)
        self.call_index, self._reported = int(call_index) & 0xFFFFFFFF, [0] * CODES

    def _state_tensors(self) -> dict:
        return dict(counters=self.counters, counts=self.counts, verdict=self.verdict)

    def load_state_dict(self, state: dict) -> None:
        super().load_state_dict(state)
        self._reported = self.counts.tolist()

    def record(self) -> dict:
        """{"referee/<name>": calls since the last record()} -- one host read of the eight counts."""
        now = self.counts.tolist()
        diff = [a - b for a, b in zip(now, self._reported)]
        self._reported = now
        return {f"referee/{name}": sum(diff[c] for c in codes) for name, codes in RECORD.items()}
