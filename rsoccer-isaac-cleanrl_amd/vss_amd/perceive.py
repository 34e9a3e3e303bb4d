"""The perception channel (include/vss.h `vss_perceive`, csrc/vss_perceive.hip).

A policy on a real VSS robot sees the overhead camera's poses: a few control steps late and with millimetre-scale
noise.  The channel turns the simulator's true observation rows into such rows -- `delay` steps old, Gaussian noise
on every position, velocity, heading and yaw rate -- in one launch per call.  `reference_perceive` below is its
specification: float32 numpy, one operation per line, in the kernel's order; the kernel equals it bit for bit
(tests/test_perceive_gpu.py).  Only + - * /, sqrt, comparisons, selects and integer operations occur, every one
correctly rounded in both, and nothing is contracted into an FMA.

    ch = PerceptionChannel(n_fields, Layout(...), delay, Noise(...), seed, device)
    rows = ch.start(obs)                          # reset(): ages 0, the ring's current slot, obs + noise
    rows, term_rows = ch.perceive(obs, term, done)  # one step: one vss_perceive launch, no host sync

Row layout (envs/vss.py compute_obs): ball x y vx vy [0:4]; own robot j at 4 + 9 j: x y vx vy cos sin w a0 a1 (for
the row of robot k, own slot j is robot (k + j) % 3 of the row's team); opponent j at 31 + 7 j: x y vx vy cos sin
w.  A yellow row is the blue frame with the ball, positions, velocities, cos and sin negated.

Per call (index t) and field, with the field's `age` (steps since its episode began, saturating at `delay`):
  d = min(age + 1, delay);  R = the true frame of call t - d  (delay >= 1)
  term_out = R with the six own-action floats of `term` -- a robot knows what it commanded;  `term` for delay 0
  age' = done ? 0 : d;  the ring's slot t % (delay + 1) takes `obs`
  obs_out = age' == 0 ? obs : R with the six own-action floats of `obs`
  then the same noise on both: 40 unit normals per (field, call), shared by every row of the field on either team
No frame of an earlier episode is ever read: a field younger than `delay` steps sees its episode's first frame.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N
from . import channel

F = np.float32
U32 = np.uint32
NUM_OBS = 52
MAX_DELAY = N.PERCEIVE_MAX_DELAY
ACTION_FLOATS = (11, 12, 20, 21, 29, 30)  # the own robots' last commands: always the current true row's
PURPOSE = 7                                 # the Philox counter's purpose byte (the step uses 0..6)
DRAWS = 40                                  # unit normals per (field, call)


class Layout(NamedTuple):
    """Where the rows lie (include/vss.h vss_perceive_layout), strides in 52-float rows."""
    field_stride: int
    team_stride: int = 0
    robots: int = 1
    n_teams: int = 1
    first_team: int = 0

    def span(self, n_fields: int) -> int:
        """Rows from the first row to the last one's end."""
        return channel.span(self, n_fields)

    def row_index(self, n_fields: int) -> np.ndarray:
        """(n_teams, n_fields, robots) int64: the row of team block b, field f, robot k."""
        return channel.index(self, n_fields)


class Noise(NamedTuple):
    """Standard deviations: positions (m), velocities (m/s), headings (rad), yaw rates (rad/s)."""
    pos: float = 0.0
    vel: float = 0.0
    ang: float = 0.0
    angvel: float = 0.0

    def any(self) -> bool:
        return any(float(s) != 0.0 for s in self)


# the wrappers' layouts
def layout_sa() -> Layout:
    return Layout(1)


def layout_dma() -> Layout:
    return Layout(3, 0, 3)


def layout_mirror(field_rows: int, n_fields: int) -> Layout:
    return Layout(field_rows, field_rows * n_fields, field_rows, 2, 0)


def layout_opponent() -> Layout:
    """The versus step's opp_obs (N, 3, 52): yellow rows."""
    return Layout(3, 0, 3, 1, 1)


def layout_full_blue() -> Layout:
    """The blue rows of FULL's (N, 2, 3, 52); the yellow rows are neither read nor written."""
    return Layout(6, 0, 3)


def full_rows(ball, robots) -> np.ndarray:
    """The FULL layout's rows (N, 2, 3, 52) of a world, as envs/vss.py compute_obs lays them out: ball (N, 4)
    x y vx vy; robots (N, 6, 9) x y vx vy cos sin w a0 a1 in the blue frame, 0..2 blue, 3..5 yellow."""
    ball, robots = np.asarray(ball, dtype=F), np.asarray(robots, dtype=F)
    n = ball.shape[0]
    flip = np.array([-1, -1, -1, -1, -1, -1, 1, 1, 1], F)
    out = np.empty((n, 2, 3, NUM_OBS), F)
    for team in range(2):
        sgn = F(-1.0) if team else F(1.0)
        seen = robots * flip if team else robots
        for k in range(3):
            out[:, team, k, 0:4] = sgn * ball
            for j in range(3):
                out[:, team, k, 4 + 9 * j:13 + 9 * j] = seen[:, 3 * team + (k + j) % 3]
                out[:, team, k, 31 + 7 * j:38 + 7 * j] = seen[:, 3 * (1 - team) + j, :7]
    return out


# ---- the draws: csrc/vss_numerics.h's Philox, sin / cos / log and unit Box-Muller, one operation per line -------
def _philox(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 on uint32 arrays (key and counter words broadcast together)."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=U32) for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0.astype(np.uint64)
        p1 = np.uint64(0xCD9E8D57) * c2.astype(np.uint64)
        hi0, lo0 = (p0 >> np.uint64(32)).astype(U32), p0.astype(U32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(U32), p1.astype(U32)
        n0 = hi1 ^ c1 ^ k0
        n2 = hi0 ^ c3 ^ k1
        c0, c1, c2, c3 = n0, lo1, n2, lo0
        k0 = (k0 + U32(0x9E3779B9)).astype(U32)
        k1 = (k1 + U32(0xBB67AE85)).astype(U32)
    return c0, c1, c2, c3


def _u01(x):
    return (x >> U32(8)).astype(F) * F(5.9604645e-08)


def _u01_open0(x):
    return ((x >> U32(8)) + U32(1)).astype(F) * F(5.9604645e-08)


def _sincos_poly(r):
    r2 = r * r
    s = r + r * r2 * (F(-0.16666667) + r2 * (F(0.008333334) + r2 * (F(-1.9841270e-4) + r2 * F(2.7557319e-6))))
    c = F(1.0) + r2 * (F(-0.5) + r2 * (F(0.041666668) + r2 * (F(-1.3888889e-3) + r2 * (F(2.4801587e-5)
                                                                                      + r2 * F(-2.7557319e-7)))))
    return s, c


def _sincos_small(x):
    x = np.asarray(x, dtype=F)
    s0, c0 = _sincos_poly(x)
    half = np.where(x >= F(0.0), F(0.5), F(-0.5)).astype(F)
    k = (x * F(0.63661977) + half).astype(np.int32)  # truncates, as the C cast
    kf = k.astype(F)
    r = (x - kf * F(1.5707964)) - kf * F(-4.3711390e-8)
    sr, cr = _sincos_poly(r)
    s = np.where(k == 0, sr, np.where(k == 1, cr, np.where(k == -1, -cr, -sr)))
    c = np.where(k == 0, cr, np.where(k == 1, -sr, np.where(k == -1, sr, -cr)))
    small = np.abs(x) < F(0.78)
    return np.where(small, s0, s).astype(F), np.where(small, c0, c).astype(F)


def _sincos_turn(u):
    v = u * F(4.0)
    q = v.astype(np.int32)
    t = v - q.astype(F)
    r = (t - F(0.5)) * F(1.5707964)
    sr, cr = _sincos_poly(r)
    cp = (cr - sr) * F(0.70710677)
    sp = (cr + sr) * F(0.70710677)
    c = np.where(q == 0, cp, np.where(q == 1, -sp, np.where(q == 2, -cp, sp)))
    s = np.where(q == 0, sp, np.where(q == 1, cp, np.where(q == 2, -sp, -cp)))
    return s.astype(F), c.astype(F)


def _logf_poly(x):
    u = np.ascontiguousarray(x, dtype=F).view(U32)
    e = ((u >> U32(23)) & U32(0xFF)).astype(np.int32) - np.int32(127)
    m = ((u & U32(0x7FFFFF)) | U32(0x3F800000)).view(F)
    big = m > F(1.4142135)
    m = np.where(big, m * F(0.5), m).astype(F)
    e = np.where(big, e + 1, e)
    s = (m - F(1.0)) / (m + F(1.0))
    s2 = s * s
    p = F(2.0) + s2 * (F(0.6666667) + s2 * (F(0.4) + s2 * (F(0.2857143) + s2 * (F(0.22222222) + s2 * F(0.18181819)))))
    return e.astype(F) * F(0.69314718) + s * p


def _box_muller(w1, w2):
    u1 = _u01_open0(w1)
    u2 = _u01(w2)
    rad = np.sqrt(F(-2.0) * _logf_poly(u1))
    sz, cz = _sincos_turn(u2)
    return rad * cz, rad * sz


def unit_normals(seed: int, fields, call: int) -> np.ndarray:
    """(len(fields), 40) float32: the unit normals of each field at `call`.  Block b of the counter
    (field, call, 7 << 24, b) gives pair 2 b from words (w0, w1) and pair 2 b + 1 from (w2, w3); pair p gives
    z[2 p] = rad cos, z[2 p + 1] = rad sin."""
    fields = np.asarray(fields, dtype=np.int64).astype(U32)
    k0, k1 = U32(int(seed) & 0xFFFFFFFF), U32((int(seed) >> 32) & 0xFFFFFFFF)
    z = np.empty((fields.shape[0], DRAWS), F)
    for b in range(DRAWS // 4):
        w = _philox(k0, k1, fields, U32(int(call) & 0xFFFFFFFF), U32(PURPOSE << 24), U32(b))
        z[:, 4 * b + 0], z[:, 4 * b + 1] = _box_muller(w[0], w[1])
        z[:, 4 * b + 2], z[:, 4 * b + 3] = _box_muller(w[2], w[3])
    return z


# ---- the specification ------------------------------------------------------------------------------------------
def _add_robot(v, base, z, e, sgn, noise):
    """Entity e's noise on the seven floats at `base` of rows v (M, 52); z (M, 40); sgn (M,) the rows' frame."""
    pos, vel, ang, angvel = (F(s) for s in noise)
    if pos != 0:
        nx = pos * z[:, 4 + 6 * e]
        ny = pos * z[:, 5 + 6 * e]
        v[:, base + 0] = v[:, base + 0] + sgn * nx
        v[:, base + 1] = v[:, base + 1] + sgn * ny
    if vel != 0:
        nvx = vel * z[:, 6 + 6 * e]
        nvy = vel * z[:, 7 + 6 * e]
        v[:, base + 2] = v[:, base + 2] + sgn * nvx
        v[:, base + 3] = v[:, base + 3] + sgn * nvy
    if ang != 0:
        eps = ang * z[:, 8 + 6 * e]
        se, ce = _sincos_small(eps)
        c = v[:, base + 4].copy()
        s = v[:, base + 5].copy()
        v[:, base + 4] = c * ce - s * se
        v[:, base + 5] = s * ce + c * se
    if angvel != 0:
        nw = angvel * z[:, 9 + 6 * e]
        v[:, base + 6] = v[:, base + 6] + nw


def add_noise(rows: np.ndarray, z: np.ndarray, first_team: int, noise) -> np.ndarray:
    """rows (n_teams, n_fields, robots, 52) with the fields' normals z (n_fields, 40) applied: a copy."""
    out = np.array(rows, dtype=F, copy=True)
    noise = Noise(*noise)
    if not noise.any():
        return out
    pos, vel = F(noise.pos), F(noise.vel)
    for b in range(out.shape[0]):
        team = first_team ^ b
        for k in range(out.shape[2]):
            v = out[b, :, k]  # (n_fields, 52): a view
            sgn = np.full(v.shape[0], -1.0 if team else 1.0, F)
            if pos != 0:
                v[:, 0] = v[:, 0] + sgn * (pos * z[:, 0])
                v[:, 1] = v[:, 1] + sgn * (pos * z[:, 1])
            if vel != 0:
                v[:, 2] = v[:, 2] + sgn * (vel * z[:, 2])
                v[:, 3] = v[:, 3] + sgn * (vel * z[:, 3])
            for j in range(3):
                _add_robot(v, 4 + 9 * j, z, 3 * team + (k + j) % 3, sgn, noise)
            for j in range(3):
                _add_robot(v, 31 + 7 * j, z, 3 * (1 - team) + j, sgn, noise)
    return out


def reference_perceive(obs, term, done, ring, age, call: int, delay: int, noise, seed: int, first_team: int = 0):
    """One call of the channel on packed rows -- the specification.

    obs, term: (n_teams, n_fields, robots, 52) float32 true rows (term None: the start call); done (n_fields,);
    ring (delay + 1, n_teams, n_fields, robots, 52) and age (n_fields,) int32 are updated in place.
    Returns (obs_out, term_out) in the shape of obs; term_out is None for the start call."""
    obs = np.ascontiguousarray(obs, dtype=F)
    if obs.ndim != 4 or obs.shape[-1] != NUM_OBS:
        raise ValueError(f"obs must be (n_teams, n_fields, robots, 52), got {obs.shape}")
    D = int(delay)
    if not 0 <= D <= MAX_DELAY:
        raise ValueError(f"delay must be in 0..{MAX_DELAY}, got {delay}")
    n = obs.shape[1]
    if ring.shape != (D + 1,) + obs.shape or age.shape != (n,) or age.dtype != np.int32:
        raise ValueError(f"ring must be {(D + 1,) + obs.shape} and age ({n},) int32, got {ring.shape} and {age.shape} {age.dtype}")
    slots = D + 1
    slot_w = int(call) % slots
    acts = list(ACTION_FLOATS)
    start = term is None
    term_out = None
    if start:
        age[:] = 0
        fresh = np.ones(n, bool)
        frame = obs
    else:
        term = np.ascontiguousarray(term, dtype=F)
        done = np.asarray(done).reshape(n) != 0
        d = np.minimum(age + 1, D).astype(np.int32)
        slot_r = (slot_w + slots - d) % slots
        # R: each field's frame of call - d (for delay 0 the terminal row stands in: R is not used)
        frame = ring[slot_r, :, np.arange(n)].transpose(1, 0, 2, 3) if D >= 1 else term
        term_out = np.array(frame, dtype=F, copy=True)
        term_out[..., acts] = term[..., acts]
        age[:] = np.where(done, 0, d)
        fresh = age == 0
    ring[slot_w] = obs
    obs_out = np.where(fresh[None, :, None, None], obs, frame).astype(F)
    obs_out[..., acts] = obs[..., acts]
    if Noise(*noise).any():
        z = unit_normals(seed, np.arange(n), call)
        obs_out = add_noise(obs_out, z, first_team, noise)
        if term_out is not None:
            term_out = add_noise(term_out, z, first_team, noise)
    return obs_out, term_out


# ---- the kernel's side --------------------------------------------------------------------------------------------
def _c_layout(layout: Layout) -> N.VssPerceiveLayout:
    return N.VssPerceiveLayout(int(layout.field_stride), int(layout.team_stride), int(layout.robots), int(layout.n_teams),
                               int(layout.first_team))


class PerceptionChannel(channel.Channel):
    """The ring, the ages, the outputs and the host call counter of one set of rows.

    `rows`: the rows of the buffers handed to start() / perceive() (default: the layout's span); the outputs have
    that many rows and are returned in the inputs' shape.  `done_stride`: int64 elements from one field's done
    flag to the next.  Rows the layout does not cover stay zero in the outputs."""

    def __init__(self, n_fields: int, layout, delay: int = 0, noise=Noise(), seed: int = 0, device="cuda",
                 done_stride: int = 1, rows: int | None = None):
        self.device = N.require_device(device)
        self.n_fields, self.layout, self.delay, self.noise = int(n_fields), Layout(*layout), int(delay), Noise(*noise)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.done_stride = int(done_stride)
        if not 0 <= self.delay <= MAX_DELAY:
            raise ValueError(f"observation delay must be in 0..{MAX_DELAY} steps, got {delay}")
        if any(not (float(s) >= 0.0 and float(s) < float("inf")) for s in self.noise):
            raise ValueError(f"observation noise: the standard deviations must be finite and >= 0, got {tuple(self.noise)}")
        self._set_rows(rows)
        lay, dev = self.layout, self.device
        self.ring = torch.zeros((self.delay + 1, lay.n_teams, self.n_fields, lay.robots, NUM_OBS), device=dev)
        self.age = torch.zeros(self.n_fields, dtype=torch.int32, device=dev)
        self.obs_out = torch.zeros((self.rows, NUM_OBS), device=dev)
        self.term_out = torch.zeros((self.rows, NUM_OBS), device=dev)
        self.call = 0
        self._no_done = torch.zeros(1, dtype=torch.long, device=dev)
        self._lay, self._noise = _c_layout(lay), N.VssPerceiveNoise(*(float(s) for s in self.noise))

    def _launch(self, obs, term, done) -> None:
        rc = N.load().vss_perceive(
            N.stream_of(self.device), self.n_fields, ctypes.byref(self._lay), self.delay, ctypes.byref(self._noise),
            self.seed, self.call & 0xFFFFFFFF, obs.data_ptr(), N.ptr(term),
            done.data_ptr(), self.done_stride, self.ring.data_ptr(), self.age.data_ptr(), self.obs_out.data_ptr(),
            None if term is None else self.term_out.data_ptr())
        N.check(rc, "vss_perceive")
        self.call += 1

    @torch.no_grad()
    def start(self, obs: torch.Tensor, call: int = 0) -> torch.Tensor:
        """reset(): every field's age 0, the current slot written, obs + noise returned (call index `call`)."""
        self._check_rows(obs, "obs")
        self.call = int(call)
        self._launch(obs, None, self._no_done)  # the start call reads no done flag
        return self.obs_out.view(obs.shape)

    @torch.no_grad()
    def perceive(self, obs: torch.Tensor, term: torch.Tensor, done: torch.Tensor):
        """One step: (perceived obs, perceived terminal obs) in the inputs' shapes; the buffers are the channel's."""
        self._check_rows(obs, "obs")
        self._check_rows(term, "term")
        self._check_done(done)
        self._launch(obs, term, done)
        return self.obs_out.view(obs.shape), self.term_out.view(term.shape)

    def _state_tensors(self) -> dict:
        return dict(ring=self.ring, age=self.age, obs_out=self.obs_out, term_out=self.term_out)
