"""Set plays (include/vss.h `vss_setplay`, csrc/vss_setplay.hip).

The step starts every episode with a uniform drop of the seven bodies (envs/vss.py:267-333).  A VSS match restarts
from a kickoff, one of four free-ball marks, a penalty or a goal kick, with the robots in formation -- situations a
uniform drop almost never produces.  With a set-play table a share of the fields that finished starts the next episode
from a named placement instead: anchor + uniform jitter per entity, then two mirrorings.  One launch per call, after
the step, over the step's own state and observation rows; `reference_setplay` below is its specification: float32
numpy, one operation per line, in the kernel's order, nothing contracted; the kernel equals it bit for bit
(tests/test_setplay_gpu.py).

    st = Stager(n_fields, Table(plays_of_mix("kickoff:1,penalty_for:2"), share=0.5), seed, device)
    st.start(env.state, [(obs, view_sa())])               # reset(): every field counts as done
    st.stage(env.state, [(obs, view_sa())], env.reset_buf)  # after a step: one vss_setplay launch, no host sync

Entities in order: the ball, blue 0..2, yellow 0..2; blue attacks +x.  Per call t and field f that is done (a start
call has no mask: every field), with u = u01(word) of Philox4x32-10, key (seed lo, seed hi), counter
(f, t, 10 << 24, block):

    block 0      w0 u_share   w1 u_play   w2 u_flip_x   w3 u_flip_y
    block 1      the ball:    w0 x        w1 y          w2 vx          w3 vy
    block 1 + e  entity e = 1..6 (B0 B1 B2 Y0 Y1 Y2):   w0 x   w1 y   w2 yaw   (w3 is not used)

    staged = u_share < share                       # a field that is not staged keeps the step's uniform reset
    k = the first play with u_play * W < cum_k     # W, cum_k: float32 running sums computed on the host
    x = ax + ((2 u - 1) * r_pos), y likewise, yaw = ayaw + ((2 u - 1) * r_yaw), ball v = (vx, vy) + ((2 u - 1) * r_vel)
    flip_y (u_flip_y < p_flip_y): y, vy, yaw negated
    flip_x (u_flip_x < p_flip_x): x, vx negated, yaw = pi - yaw, and blue i and yellow i swap their placements
    yaw > pi: yaw - 2 pi;  yaw < -pi: yaw + 2 pi;  (qz, qw) = sincos_small(0.5 * yaw);  qx = qy = 0

The flips come after the jitter, so a mirrored placement is the mirror image of the unmirrored one bit for bit.  The
wrap is part of the specification: sincos_small reduces correctly only for |x| up to about 2.5 pi / 2.  Robot linear
and angular velocities are 0 and the own-action floats of the rows +0.0: the step has already zeroed a finished
field's dof_velocity_buf and OU state.  A staged field's 58 state channels and its rows in every view are written,
chosen[f] = k and counts[k] += 1; every other field's state and rows stay and chosen[f] = -1.

Table.validate guarantees that no play can start in contact (worst-case pair distance >= 0.08 m, K_RR_DIST, above the
uniform reset's own 0.07 m rule) or outside the walls, so there is no rejection loop.

The entry point is libvss_amd.so's, bound from include/vss.h by vss_amd/_native.py like every other: the structs, the
constants and the loader here are `_native`'s under the module's own names.  There is no fallback: a missing or stale
library raises.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N
from . import channel
from .perceive import NUM_OBS, _philox, _sincos_small, _u01

F = np.float32
U32 = np.uint32

MAX_PLAYS = N.SETPLAY_MAX_PLAYS
VssSetplayEntity = N.VssSetplayEntity
VssSetplayPlay = N.VssSetplayPlay
VssSetplayTable = N.VssSetplayTable
VssSetplayView = N.VssSetplayView
load = N.load  # the one library's loader under the module's own name, as before

PURPOSE = 10          # the Philox counter's purpose byte (the step 0..6, perception 7, actuation 8 and 9)
BLOCKS = 8            # Philox blocks per staged field: control, the ball, six robots
ENTITIES = ("ball", "B0", "B1", "B2", "Y0", "Y1", "Y2")
PI, TWO_PI = F(3.1415927), F(6.2831855)
MIN_GAP = 0.08        # K_RR_DIST: the robot-robot contact distance
HALF_ROBOT = (0.71, 0.61)  # the field's half-extents 0.75 and 0.65 minus K_ROBOT_R 0.04
HALF_BALL = (0.75, 0.65)
# include/vss.h VSS_CH_*
CH_RX, CH_RY, CH_RQX, CH_RQY, CH_RQZ, CH_RQW, CH_RVX, CH_RVY, CH_RW = (N.CH_RX, N.CH_RY, N.CH_RQX, N.CH_RQY, N.CH_RQZ,
                                                                      N.CH_RQW, N.CH_RVX, N.CH_RVY, N.CH_RW)

# ---- plays and tables -------------------------------------------------------------------------------------------------
class Play(NamedTuple):
    """A named placement: `entities` seven rows (x, y, yaw, r_pos, r_yaw) for the ball, B0..B2, Y0..Y2 (the ball's
    yaw and r_yaw are not read); `ball_vel` (vx, vy, r_vel); the weight within a table; the flip probabilities."""
    name: str
    entities: tuple
    ball_vel: tuple = (0.0, 0.0, 0.0)
    weight: float = 1.0
    p_flip_x: float = 0.5
    p_flip_y: float = 0.5


class View(NamedTuple):
    """Observation rows to rewrite (include/vss.h vss_setplay_view), strides in 52-float rows."""
    field_stride: int
    team_stride: int = 0
    robots: int = 1
    n_teams: int = 1
    first_team: int = 0

    def span(self, n_fields: int) -> int:
        return channel.span(self, n_fields)

    def row_index(self, n_fields: int) -> np.ndarray:
        return channel.index(self, n_fields)


def view_sa() -> View:
    """SA's and CMA's rows: blue robot 0's view."""
    return View(1)


def view_dma() -> View:
    return View(3, 0, 3)


def view_opponent() -> View:
    """The versus step's opp_obs (N, 3, 52): the yellow rows."""
    return View(3, 0, 3, 1, 1)


def view_mirror(field_rows: int, n_fields: int) -> View:
    return View(field_rows, field_rows * n_fields, field_rows, 2, 0)


def view_full() -> View:
    """FULL's (N, 2, 3, 52) as one two-team view."""
    return View(6, 3, 3, 2, 0)


def _finite(v) -> bool:
    return math.isfinite(float(v))


class Table:
    """1..8 plays and the share of finished fields that are staged.  The cumulative weights are float32 running sums
    computed here and passed to the kernel, so host and device agree without a device-side sum."""

    def __init__(self, plays, share: float = 1.0):
        self.plays = tuple(Play(*p) for p in plays)
        self.share = float(share)
        self.validate()

    @property
    def names(self) -> tuple:
        return tuple(p.name for p in self.plays)

    def cum_weights(self) -> np.ndarray:
        cum = np.zeros(len(self.plays), F)
        run = F(0.0)
        for k, p in enumerate(self.plays):
            run = F(run + F(p.weight))
            cum[k] = run
        return cum

    def validate(self) -> "Table":
        """ValueError for what vss_setplay refuses with VSS_E_ARG (the same rules, in double on the float32
        values the kernel gets)."""
        if not 1 <= len(self.plays) <= MAX_PLAYS:
            raise ValueError(f"set plays: a table holds 1..{MAX_PLAYS} plays, got {len(self.plays)}")
        if not (_finite(self.share) and 0.0 <= self.share <= 1.0):
            raise ValueError(f"set plays: the share must be in [0, 1], got {self.share}")
        for p in self.plays:
            where = f"set play {p.name!r}"
            if not (_finite(p.weight) and float(p.weight) >= 0.0):
                raise ValueError(f"{where}: the weight must be finite and >= 0, got {p.weight}")
            for name, v in (("p_flip_x", p.p_flip_x), ("p_flip_y", p.p_flip_y)):
                if not (_finite(v) and 0.0 <= float(v) <= 1.0):
                    raise ValueError(f"{where}: {name} must be in [0, 1], got {v}")
            if len(p.ball_vel) != 3 or not all(_finite(v) for v in p.ball_vel) or float(p.ball_vel[2]) < 0.0:
                raise ValueError(f"{where}: ball_vel must be finite (vx, vy, r_vel) with r_vel >= 0, got {p.ball_vel}")
            if len(p.entities) != 7 or any(len(e) != 5 for e in p.entities):
                raise ValueError(f"{where}: seven entities of (x, y, yaw, r_pos, r_yaw) are needed")
            rows = np.asarray(p.entities, dtype=F)
            if not np.isfinite(rows).all():
                raise ValueError(f"{where}: a non-finite value")
            d = rows.astype(np.float64)
            for e, (x, y, yaw, r_pos, r_yaw) in enumerate(d):
                who = f"{where}, {ENTITIES[e]}"
                if r_pos < 0.0:
                    raise ValueError(f"{who}: r_pos must be >= 0, got {r_pos}")
                if abs(rows[e, 2]) > PI or not F(0.0) <= rows[e, 4] <= PI:
                    raise ValueError(f"{who}: |yaw| must be <= pi and r_yaw in [0, pi], got {yaw} and {r_yaw}")
                hx, hy = HALF_BALL if e == 0 else HALF_ROBOT
                if abs(x) + r_pos > hx or abs(y) + r_pos > hy:
                    raise ValueError(f"{who}: can leave the field: |x| + r_pos <= {hx} and |y| + r_pos <= {hy} are "
                                     f"needed, got ({x:.3f}, {y:.3f}) +- {r_pos:.3f}")
                for j in range(e):
                    gap = math.hypot(x - d[j, 0], y - d[j, 1]) - math.sqrt(2.0) * (r_pos + d[j, 3])
                    if gap < MIN_GAP:
                        raise ValueError(f"{who} and {ENTITIES[j]}: the worst-case distance {gap:.4f} m is below "
                                         f"{MIN_GAP} m (anchors minus sqrt(2) (r_i + r_j)): the play could start in contact")
        if not float(self.cum_weights()[-1]) > 0.0:
            raise ValueError("set plays: the total weight is 0")
        if not _finite(self.cum_weights()[-1]):
            raise ValueError("set plays: the total weight is not finite")
        return self

    def only(self, k: int) -> "Table":
        """The table that stages every field with play k: share 1, every other weight 0 (the indices stay)."""
        if not 0 <= int(k) < len(self.plays):
            raise ValueError(f"set plays: only={k} is outside 0..{len(self.plays) - 1}")
        return Table([p._replace(weight=1.0 if i == int(k) else 0.0) for i, p in enumerate(self.plays)], 1.0)

    def arrays(self) -> dict:
        """The table as float32 arrays, as the kernel gets it: ent (K, 7, 5), vel (K, 3), cum (K,), flip (K, 2)."""
        return dict(ent=np.asarray([p.entities for p in self.plays], dtype=F),
                    vel=np.asarray([p.ball_vel for p in self.plays], dtype=F), cum=self.cum_weights(),
                    flip=np.asarray([(p.p_flip_x, p.p_flip_y) for p in self.plays], dtype=F), share=F(self.share))

    def c_table(self) -> "VssSetplayTable":
        a = self.arrays()
        t = VssSetplayTable()
        t.count, t.share, t.total_weight = len(self.plays), float(a["share"]), float(a["cum"][-1])
        for k in range(len(self.plays)):
            p = t.play[k]
            for e in range(7):
                p.e[e].x, p.e[e].y, p.e[e].yaw, p.e[e].r_pos, p.e[e].r_yaw = (float(v) for v in a["ent"][k, e])
            p.ball_vx, p.ball_vy, p.r_vel = (float(v) for v in a["vel"][k])
            p.cum_weight, p.p_flip_x, p.p_flip_y = float(a["cum"][k]), float(a["flip"][k, 0]), float(a["flip"][k, 1])
        return t


_PI = math.pi
BUILTIN = {p.name: p for p in (
    Play("kickoff", ((0, 0, 0, 0, 0), (-0.10, 0, 0, .01, .2), (-0.35, .25, 0, .03, .5), (-0.62, 0, 0, .02, .5),
                     (0.25, 0, _PI, .02, .5), (0.35, -.25, _PI, .03, .5), (0.62, 0, _PI, .02, .5))),
    # the flips give the other three marks
    Play("free_ball", ((.375, .4, 0, 0, 0), (.175, .4, 0, .01, .2), (-.10, 0, 0, .03, .5), (-.62, .05, 0, .02, .5),
                       (.575, .4, _PI, .01, .2), (.45, -.10, _PI, .03, .5), (.66, .05, _PI, .02, .5))),
    Play("penalty", ((.375, 0, 0, 0, 0), (.28, 0, 0, .01, .3), (-.10, .30, 0, .03, .5), (-.10, -.30, 0, .03, .5),
                     (-.15, .10, _PI, .02, .5), (-.15, -.10, _PI, .02, .5), (.68, 0, _PI / 2, .02, .3))),
    Play("goal_kick", ((-.60, .10, 0, 0, 0), (-.30, .30, 0, .03, .5), (-.30, -.30, 0, .03, .5), (-.69, .10, 0, 0, .2),
                       (0, 0, _PI, .03, .5), (.20, .30, _PI, .03, .5), (.66, 0, _PI, .02, .5))),
    Play("breakaway", ((.20, 0, 0, .01, 0), (.06, 0, 0, .01, .3), (-.50, .30, 0, .03, .5), (-.50, -.30, 0, .03, .5),
                       (-.20, .20, 0, .03, .5), (-.20, -.20, 0, .03, .5), (.66, 0, _PI, .02, .5))),
)}
DEFAULT_MIX = ",".join(f"{name}:1" for name in BUILTIN)


def named_play(name: str, library: dict | None = None) -> Play:
    """A play by name: a library entry (default: BUILTIN), NAME_for (p_flip_x 0: blue's set piece) or NAME_against
    (p_flip_x 1: the role swap)."""
    library = BUILTIN if library is None else library
    if name in library:
        return library[name]
    for suffix, p in (("_for", 0.0), ("_against", 1.0)):
        if name.endswith(suffix) and name[:-len(suffix)] in library:
            return library[name[:-len(suffix)]]._replace(name=name, p_flip_x=p)
    raise ValueError(f"set plays: no play named {name!r}; known: {', '.join(library)} (and NAME_for, NAME_against)")


def plays_of_mix(mix: str | None = None, library: dict | None = None) -> list:
    """The plays of a mix "name:weight,name:weight" (a missing weight is 1; None or "": every play of the library at
    weight 1)."""
    library = BUILTIN if library is None else library
    if not mix:
        mix = ",".join(library)
    out = []
    for item in (s.strip() for s in str(mix).split(",")):
        if not item:
            raise ValueError(f"set plays: an empty entry in the mix {mix!r}")
        name, _, w = item.partition(":")
        try:
            weight = float(w) if w else 1.0
        except ValueError:
            raise ValueError(f"set plays: the weight of {name!r} in the mix is not a number: {w!r}") from None
        if any(p.name == name.strip() for p in out):
            raise ValueError(f"set plays: {name.strip()!r} is named twice in the mix {mix!r}")
        out.append(named_play(name.strip(), library)._replace(weight=weight))
    return out


def load_file(path: str) -> dict:
    """Custom plays of a JSON file: {"plays": [{"name", "entities": 7 x [x, y, yaw, r_pos, r_yaw], "ball_vel":
    [vx, vy, r_vel], "p_flip_x", "p_flip_y"}]} -- settings only; all but name and entities optional."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or not isinstance(doc.get("plays"), list) or not doc["plays"]:
        raise ValueError(f"{path}: expected an object with a non-empty list \"plays\"")
    library = {}
    for item in doc["plays"]:
        extra = set(item) - {"name", "entities", "ball_vel", "weight", "p_flip_x", "p_flip_y"} if isinstance(item, dict) else {"?"}
        if extra or "name" not in item or "entities" not in item:
            raise ValueError(f"{path}: a play needs name and entities and may have ball_vel, weight, p_flip_x, p_flip_y; "
                             f"got {sorted(item) if isinstance(item, dict) else item!r}")
        name = str(item["name"])
        if name in library or name.endswith(("_for", "_against")):
            raise ValueError(f"{path}: the play name {name!r} is used twice or ends in _for / _against")
        play = Play(name, tuple(tuple(float(v) for v in e) for e in item["entities"]),
                    tuple(float(v) for v in item.get("ball_vel", (0.0, 0.0, 0.0))), float(item.get("weight", 1.0)),
                    float(item.get("p_flip_x", 0.5)), float(item.get("p_flip_y", 0.5)))
        Table([play], 1.0)  # validates
        library[name] = play
    return library


def table_of_args(args) -> "Table | None":
    """The table of --setplay-share / --setplay-mix / --setplay-file; None with a share of 0 (absent flags are their
    defaults).  With a file the mix names the file's plays and the built-ins."""
    share = float(getattr(args, "setplay_share", 0.0) or 0.0)
    if not 0.0 <= share <= 1.0:
        raise ValueError(f"--setplay-share must be in [0, 1], got {share}")
    if share == 0.0:
        return None
    path, mix = getattr(args, "setplay_file", None) or None, getattr(args, "setplay_mix", None) or None
    if path:
        own = load_file(path)
        return Table(plays_of_mix(mix, dict(BUILTIN, **own)) if mix else plays_of_mix(None, own), share)
    return Table(plays_of_mix(mix), share)


def setplay_seed(seed, offset: int = 0) -> int:
    """The stager's Philox key from --seed and the rank, built as envs.wrappers.perception_seed with a constant of
    its own; `offset` separates the arena's stager from the training's."""
    return ((int(seed or 0) * 1000003 + int(os.environ.get("RANK", 0))) * 2654435761 + 0x5E7_91A7 + int(offset)) \
        & 0xFFFFFFFFFFFFFFFF


# ---- the specification ----------------------------------------------------------------------------------------------
def _jitter(word, r):
    t = F(2.0) * _u01(word)
    t = t - F(1.0)
    return t * r


def full_rows_of_state(state: np.ndarray, fields) -> np.ndarray:
    """(len(fields), 2, 3, 52): the FULL rows of the fields' state (58, n) with zero own-action floats, exactly as
    vss_compute_observations lays them out: c = qw^2 - qz^2, s = 2 qw qz, the yellow view negated, own slot j = robot
    (k + j) % 3."""
    s = state[:, fields]
    m = s.shape[1]
    rec = np.zeros((m, 6, 9), F)
    for r in range(6):
        qz, qw = s[CH_RQZ + r], s[CH_RQW + r]
        rec[:, r, 0], rec[:, r, 1] = s[CH_RX + r], s[CH_RY + r]
        rec[:, r, 2], rec[:, r, 3] = s[CH_RVX + r], s[CH_RVY + r]
        rec[:, r, 4] = qw * qw - qz * qz
        rec[:, r, 5] = (F(2.0) * qw) * qz
        rec[:, r, 6] = s[CH_RW + r]
    ball = s[0:4].T
    out = np.empty((m, 2, 3, NUM_OBS), F)
    for team in range(2):
        seen = rec.copy()
        if team:
            seen[:, :, :6] = -seen[:, :, :6]
        for k in range(3):
            out[:, team, k, 0:4] = -ball if team else ball
            for j in range(3):
                out[:, team, k, 4 + 9 * j:13 + 9 * j] = seen[:, 3 * team + (k + j) % 3]
                out[:, team, k, 31 + 7 * j:38 + 7 * j] = seen[:, 3 * (1 - team) + j, :7]
    return out


def reference_setplay(table: Table, seed: int, call: int, done, state: np.ndarray, views=(), counts=None, chosen=None):
    """One call -- the specification.  done (n,) or None (a start call: every field); state (58, n) float32, each
    view a pair (rows (R, 52) float32, View), counts (8,) int64 and chosen (n,) int32 are updated in place.  Returns
    the indices of the staged fields."""
    if state.dtype != F or state.ndim != 2 or state.shape[0] != N.STATE_CHANNELS:
        raise ValueError(f"state must be float32 (58, n), got {state.dtype} {state.shape}")
    n = state.shape[1]
    a = table.arrays()
    K = len(table.plays)
    done = np.ones(n, bool) if done is None else np.asarray(done).reshape(n) != 0
    fields = np.nonzero(done)[0]
    k0, k1 = U32(int(seed) & 0xFFFFFFFF), U32((int(seed) >> 32) & 0xFFFFFFFF)
    t = U32(int(call) & 0xFFFFFFFF)

    def words(ff, block):
        return _philox(k0, k1, ff.astype(np.int64).astype(U32), t, U32(PURPOSE << 24), U32(block))

    w = words(fields, 0)
    staged = _u01(w[0]) < a["share"]
    f = fields[staged]
    if chosen is not None:
        chosen[:] = -1
    if f.size == 0:
        return f
    u_play, u_fx, u_fy = _u01(w[1])[staged], _u01(w[2])[staged], _u01(w[3])[staged]
    up = u_play * a["cum"][-1]
    sel = np.full(f.size, K - 1, np.int32)
    for k in range(K - 2, -1, -1):
        sel = np.where(up < a["cum"][k], np.int32(k), sel)
    ent, vel = a["ent"][sel], a["vel"][sel]            # (m, 7, 5), (m, 3)
    flip_x = u_fx < a["flip"][sel, 0]
    flip_y = u_fy < a["flip"][sel, 1]

    w = words(f, 1)
    bx = ent[:, 0, 0] + _jitter(w[0], ent[:, 0, 3])
    by = ent[:, 0, 1] + _jitter(w[1], ent[:, 0, 3])
    bvx = vel[:, 0] + _jitter(w[2], vel[:, 2])
    bvy = vel[:, 1] + _jitter(w[3], vel[:, 2])
    by = np.where(flip_y, -by, by)
    bvy = np.where(flip_y, -bvy, bvy)
    bx = np.where(flip_x, -bx, bx)
    bvx = np.where(flip_x, -bvx, bvx)
    px, py, qz, qw = (np.empty((f.size, 6), F) for _ in range(4))
    for e in range(1, 7):
        w = words(f, 1 + e)
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

    state[0, f], state[1, f], state[2, f], state[3, f] = bx, by, bvx, bvy
    for r in range(6):
        state[CH_RX + r, f], state[CH_RY + r, f] = px[:, r], py[:, r]
        state[CH_RQX + r, f] = state[CH_RQY + r, f] = F(0.0)
        state[CH_RQZ + r, f], state[CH_RQW + r, f] = qz[:, r], qw[:, r]
        state[CH_RVX + r, f] = state[CH_RVY + r, f] = state[CH_RW + r, f] = F(0.0)
    full = full_rows_of_state(state, f)
    for rows, view in views:
        view = View(*view)
        at = view.row_index(n)[:, f]  # (n_teams, m, robots)
        for b in range(view.n_teams):
            for k in range(view.robots):
                rows[at[b, :, k]] = full[:, view.first_team + b, k]
    if chosen is not None:
        chosen[f] = sel
    if counts is not None:
        counts[:K] += np.bincount(sel, minlength=K).astype(counts.dtype)
    return f


# ---- the kernel's side ----------------------------------------------------------------------------------------------
class Stager(channel.Channel):
    """The table, the key, `counts` (8,) int64, `chosen` (n_fields,) int32 and the host call counter.  start() and
    stage() are one vss_setplay launch each on the current stream, with no host sync."""

    def __init__(self, n_fields: int, table: Table, seed: int, device="cuda"):
        self.device = N.require_device(device)
        load()
        self.n_fields, self.table, self.seed = int(n_fields), table.validate(), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counts = torch.zeros(MAX_PLAYS, dtype=torch.long, device=self.device)
        self.chosen = torch.full((self.n_fields,), -1, dtype=torch.int32, device=self.device)
        self.call = 0
        self._where = self.counts.device
        self._tab = table.c_table()
        self._only = {}
        self._view_key, self._view_arr = None, None

    def _views(self, views):
        """(the ctypes array, the count) of the call's views; checked and built once per set of buffers -- the
        wrappers hand over the same ones every step."""
        views = list(views)
        if len(views) > 2:
            raise ValueError(f"set plays: at most two views per call, got {len(views)}")
        key = tuple((rows.data_ptr(), rows.numel(), rows.dtype, tuple(view)) for rows, view in views)
        if key == self._view_key:
            return self._view_arr, len(views)
        arr = (VssSetplayView * 2)()
        for i, (rows, view) in enumerate(views):
            view = View(*view)
            need = view.span(self.n_fields)
            if (rows.dtype != torch.float32 or rows.device != self._where or not rows.is_contiguous()
                    or rows.numel() < need * NUM_OBS):
                raise ValueError(f"set plays: view {i} must be contiguous float32 with at least {need} rows of {NUM_OBS} "
                                 f"on {self._where}, got {tuple(rows.shape)} {rows.dtype} on {rows.device}")
            arr[i] = VssSetplayView(rows.data_ptr(), int(view.field_stride), int(view.team_stride), int(view.robots),
                                    int(view.n_teams), int(view.first_team))
        self._view_key, self._view_arr = key, arr
        return arr, len(views)

    def _launch(self, tab, env_state, views, done) -> None:
        if (env_state.dtype != torch.float32 or env_state.device != self._where or not env_state.is_contiguous()
                or tuple(env_state.shape) != (N.STATE_CHANNELS, self.n_fields)):
            raise ValueError(f"set plays: the state must be contiguous float32 ({N.STATE_CHANNELS}, {self.n_fields}) on "
                             f"{self._where}, got {tuple(env_state.shape)} {env_state.dtype} on {env_state.device}")
        arr, n_views = self._views(views)
        rc = load().vss_setplay(N.stream_of(self.device), self.n_fields, ctypes.byref(tab), self.seed,
                                self.call & 0xFFFFFFFF, N.ptr(done), 1, env_state.data_ptr(), n_views, arr,
                                self.counts.data_ptr(), self.chosen.data_ptr())
        N.check(rc, "vss_setplay")
        self.call += 1

    @torch.no_grad()
    def start(self, env_state: torch.Tensor, views=(), only: int | None = None) -> None:
        """Every field counts as done; `only=k` stages every field with play k at share 1."""
        tab = self._tab
        if only is not None:
            if only not in self._only:
                self._only[only] = self.table.only(only).c_table()
            tab = self._only[only]
        self._launch(tab, env_state, views, None)

    @torch.no_grad()
    def stage(self, env_state: torch.Tensor, views, done: torch.Tensor) -> None:
        """After a step: the fields whose `done` (n_fields,) int64 is set."""
        if (done is None or done.dtype != torch.long or done.device != self._where or not done.is_contiguous()
                or done.numel() != self.n_fields):
            raise ValueError(f"set plays: done must be contiguous int64 ({self.n_fields},) on {self._where}, got "
                             f"{None if done is None else (tuple(done.shape), done.dtype)}")
        self._launch(self._tab, env_state, views, done)

    def _state_tensors(self) -> dict:
        return dict(counts=self.counts, chosen=self.chosen)
