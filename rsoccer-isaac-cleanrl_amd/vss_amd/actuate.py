"""The actuation channel (include/vss.h `vss_actuate`, csrc/vss_actuate.hip).

What a policy commands does not reach a real VSS robot's wheels exactly: the radio carries a command in [-1, 1] in a
few bits, a packet is lost now and then (the robot keeps the command it had), small commands do not move a wheel,
and two motors of one robot differ by several percent.  The channel turns the commands of one control step into
the commands the wheels apply, in one launch per call, between the policy and the step.  `reference_actuate` below is
its specification: float32 numpy, one operation per line, in the kernel's order; the kernel equals it bit for bit
(tests/test_actuate_gpu.py).  Only + - * /, rint, comparisons, selects, integer operations and perceive.py's Philox /
Box-Muller (the kernel's: csrc/vss_numerics.h) occur, every one correctly rounded in both, and nothing is contracted
into an FMA.

    ch = ActuationChannel(n_fields, Layout(...), Params(...), seed, device)
    ch.start()                                   # reset(): the next call begins an episode in every field
    applied = ch.actuate(cmd, done_prev)         # one step: one vss_actuate launch, no host sync; cmd is not modified

A command is the two floats (left wheel, right wheel) of one robot.  Per call (index t), field f, team T, robot k
(entity e = 3 T + k) and wheel w (i = 2 e + w), with `fresh` = the previous step ended f's episode, or a start:
  G = fresh ? 1 + gain_sigma * clamp(zg[i], -3, 3) : gain        the episode's wheel gain
  H = fresh ? 0 : held                                            what the robot last received
  c = clamp(cmd, -1, 1);  q = rint(c * levels) / levels           the radio's range and resolution
  r = lost[T] ? H : q                                             one packet per team and step
  m = |r| < deadband ? 0 : r;  out = m * G + noise_sigma * zn[i]
  held' = r;  gain' = G;  episode' = episode + fresh
zn: 12 unit normals of the counter (f, t, 8 << 24, block 0..2); zg: of (f, episode', 9 << 24, block); lost[T]: word
T of block 3 of the step's counter.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N
from . import channel
from .perceive import _box_muller, _philox, _u01

F = np.float32
U32 = np.uint32
MAX_GAIN_SIGMA = 0.3
PURPOSE_STEP = 8      # the Philox counter's purpose byte of the per-step draws (the step uses 0..6, perception 7)
PURPOSE_EPISODE = 9   # ... of the per-episode draws
LOSS_BLOCK = 3
DRAWS = 12            # unit normals per (field, call) and per (field, episode): two per entity

MAX_LEVELS = N.ACTUATE_MAX_LEVELS
VssActuateLayout = N.VssActuateLayout
VssActuateParams = N.VssActuateParams
load = N.load  # the one library's loader under the module's own name, as before


class Layout(NamedTuple):
    """Where the commands lie (include/vss.h vss_actuate_layout), strides in robots (2 floats)."""
    field_stride: int
    team_stride: int = 0
    robots: int = 1
    n_teams: int = 1
    first_team: int = 0

    def span(self, n_fields: int) -> int:
        """Robots from the first command to the last one's end."""
        return channel.span(self, n_fields)

    def index(self, n_fields: int) -> np.ndarray:
        """(n_teams, n_fields, robots) int64: the robot slot of team block b, field f, robot k."""
        return channel.index(self, n_fields)


class Params(NamedTuple):
    """gain_sigma: std of the per-episode wheel gains (0..0.3); noise_sigma: std of the per-step command noise;
    deadband: |command| below it does not move the wheel (0..1); loss_prob: a team's packet is lost (0..1);
    levels: the command is a multiple of 1 / levels (0: not quantised; 127 is an 8-bit signed command)."""
    gain_sigma: float = 0.0
    noise_sigma: float = 0.0
    deadband: float = 0.0
    loss_prob: float = 0.0
    levels: int = 0

    def any(self) -> bool:
        return any(float(s) != 0.0 for s in self)

    def check(self) -> "Params":
        g, s, d, p = (float(F(x)) for x in self[:4])
        if not 0.0 <= g <= float(F(MAX_GAIN_SIGMA)):
            raise ValueError(f"actuation: the gain's standard deviation must be in [0, {MAX_GAIN_SIGMA}], got {self.gain_sigma}")
        if not (0.0 <= s < float("inf")):
            raise ValueError(f"actuation: the command noise's standard deviation must be finite and >= 0, got {self.noise_sigma}")
        if not 0.0 <= d <= 1.0:
            raise ValueError(f"actuation: the deadband must be in [0, 1], got {self.deadband}")
        if not 0.0 <= p < 1.0:
            raise ValueError(f"actuation: the loss probability must be in [0, 1), got {self.loss_prob}")
        if int(self.levels) != self.levels or not 0 <= int(self.levels) <= MAX_LEVELS:
            raise ValueError(f"actuation: levels must be an integer in 0..{MAX_LEVELS}, got {self.levels}")
        return self


# the wrappers' layouts
def layout_sa() -> Layout:
    return Layout(1)


def layout_team() -> Layout:
    """CMA (N, 6) and DMA (3 N, 2): the three blue robots of a field side by side."""
    return Layout(3, 0, 3)


def layout_mirror(field_robots: int, n_fields: int) -> Layout:
    return Layout(field_robots, field_robots * n_fields, field_robots, 2, 0)


def layout_opponent() -> Layout:
    """The versus step's opp_act (N, 3, 2): yellow's commands."""
    return Layout(3, 0, 3, 1, 1)


def layout_full_blue() -> Layout:
    """The blue half of FULL's (N, 2, 3, 2); the yellow half is neither read nor written."""
    return Layout(6, 0, 3)


# ---- the draws ------------------------------------------------------------------------------------------------------
def _key(seed: int):
    return U32(int(seed) & 0xFFFFFFFF), U32((int(seed) >> 32) & 0xFFFFFFFF)


def _normals(seed: int, fields, c1, purpose: int) -> np.ndarray:
    """(len(fields), 12) float32 of the counter (field, c1, purpose << 24, block 0..2), laid out as perceive.py's
    unit_normals: words (w0, w1) of block b give pair 2 b, (w2, w3) pair 2 b + 1; pair p gives z[2 p] = rad cos,
    z[2 p + 1] = rad sin.  Pair p is entity p's: z[2 e] the left wheel's, z[2 e + 1] the right wheel's."""
    fields = np.asarray(fields, dtype=np.int64).astype(U32)
    c1 = np.broadcast_to(np.asarray(c1, dtype=np.int64).astype(U32), fields.shape)
    k0, k1 = _key(seed)
    z = np.empty((fields.shape[0], DRAWS), F)
    for b in range(DRAWS // 4):
        w = _philox(k0, k1, fields, c1, U32(purpose << 24), U32(b))
        z[:, 4 * b + 0], z[:, 4 * b + 1] = _box_muller(w[0], w[1])
        z[:, 4 * b + 2], z[:, 4 * b + 3] = _box_muller(w[2], w[3])
    return z


def step_normals(seed: int, fields, call: int) -> np.ndarray:
    """zn: the 12 unit normals of each field at call index `call`."""
    return _normals(seed, fields, int(call) & 0xFFFFFFFF, PURPOSE_STEP)


def episode_normals(seed: int, fields, episode) -> np.ndarray:
    """zg: the 12 unit normals of each field's episode number (an integer or one per field)."""
    return _normals(seed, fields, np.asarray(episode, dtype=np.int64) & 0xFFFFFFFF, PURPOSE_EPISODE)


def loss_uniforms(seed: int, fields, call: int) -> np.ndarray:
    """(len(fields), 2) float32 in [0, 1): blue's and yellow's packet of each field at `call`; lost where < loss_prob."""
    fields = np.asarray(fields, dtype=np.int64).astype(U32)
    k0, k1 = _key(seed)
    w = _philox(k0, k1, fields, U32(int(call) & 0xFFFFFFFF), U32(PURPOSE_STEP << 24), U32(LOSS_BLOCK))
    return np.stack([_u01(w[0]), _u01(w[1])], 1)


# ---- the specification ----------------------------------------------------------------------------------------------
def reference_actuate(cmd, done_prev, held, gain, episode, call: int, params, seed: int, first_team: int = 0) -> np.ndarray:
    """One call of the channel on packed commands -- the specification.

    cmd: (n_teams, n_fields, robots, 2) float32; done_prev: (n_fields,) the previous step's done flags, None for the
    start call; held, gain (cmd's shape, float32) and episode (n_fields,) uint32 are updated in place.  Returns the
    applied commands in cmd's shape."""
    cmd = np.ascontiguousarray(cmd, dtype=F)
    if cmd.ndim != 4 or cmd.shape[-1] != 2 or cmd.shape[0] not in (1, 2) or cmd.shape[2] not in (1, 3):
        raise ValueError(f"cmd must be (n_teams, n_fields, robots, 2), got {cmd.shape}")
    prm = Params(*params).check()
    n = cmd.shape[1]
    if held.shape != cmd.shape or gain.shape != cmd.shape or held.dtype != F or gain.dtype != F:
        raise ValueError(f"held and gain must be float32 {cmd.shape}, got {held.shape} {held.dtype} and {gain.shape} {gain.dtype}")
    if episode.shape != (n,) or episode.dtype != U32:
        raise ValueError(f"episode must be ({n},) uint32, got {episode.shape} {episode.dtype}")
    gain_sigma, noise_sigma, deadband, loss_prob = (F(x) for x in prm[:4])
    levels = int(prm.levels)
    L = F(levels)
    fields = np.arange(n)
    fresh = np.ones(n, bool) if done_prev is None else np.asarray(done_prev).reshape(n) != 0
    ep = (episode + fresh.astype(U32)).astype(U32)  # wraps
    zn = step_normals(seed, fields, call) if noise_sigma != 0 else None
    zg = episode_normals(seed, fields, ep) if gain_sigma != 0 else None  # used where fresh only
    lost = loss_uniforms(seed, fields, call) < loss_prob if loss_prob > 0 else np.zeros((n, 2), bool)
    out = np.empty_like(cmd)
    for b in range(cmd.shape[0]):
        T = first_team ^ b
        for k in range(cmd.shape[2]):
            e = 3 * T + k
            for w in range(2):
                i = 2 * e + w
                G = gain[b, :, k, w]
                if gain_sigma != 0:
                    z = zg[:, i]
                    zc = np.where(z < F(-3.0), F(-3.0), np.where(z > F(3.0), F(3.0), z)).astype(F)
                    t = gain_sigma * zc
                    G = np.where(fresh, F(1.0) + t, G).astype(F)
                else:
                    G = np.where(fresh, F(1.0), G).astype(F)
                H = np.where(fresh, F(0.0), held[b, :, k, w]).astype(F)
                u = cmd[b, :, k, w]
                c = np.where(u < F(-1.0), F(-1.0), np.where(u > F(1.0), F(1.0), u)).astype(F)
                if levels > 0:
                    s = c * L
                    r_ = np.rint(s)
                    q = r_ / L
                else:
                    q = c
                r = np.where(lost[:, T], H, q).astype(F)
                if deadband > 0:
                    m = np.where(np.abs(r) < deadband, F(0.0), r).astype(F)
                else:
                    m = r
                g = m * G
                if noise_sigma != 0:
                    t = noise_sigma * zn[:, i]
                    o = g + t
                else:
                    o = g
                held[b, :, k, w] = r
                gain[b, :, k, w] = G
                out[b, :, k, w] = o
    episode[:] = ep
    return out


# ---- the kernel's side ----------------------------------------------------------------------------------------------
class ActuationChannel(channel.Channel):
    """held, gain, episode, the output buffer and the host call counter of one set of commands.

    `rows`: the robots (2 floats each) of the buffers handed to actuate() (default: the layout's span); the output has
    that many and is returned in the input's shape; what the layout does not cover stays zero there.  `done_stride`:
    int64 elements from one field's done flag to the next."""
    unit, width = "robots", 2
    scalars = {"call": int, "fresh": bool}  # the call counter and the start flag

    def __init__(self, n_fields: int, layout, params=Params(), seed: int = 0, device="cuda", done_stride: int = 1,
                 rows: int | None = None):
        self.device = N.require_device(device)
        self.n_fields, self.layout, self.params = int(n_fields), Layout(*layout), Params(*params).check()
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.done_stride = int(done_stride)
        self._set_rows(rows)
        lay, dev = self.layout, self.device
        packed = (lay.n_teams, self.n_fields, lay.robots, 2)
        self.held = torch.zeros(packed, device=dev)
        self.gain = torch.ones(packed, device=dev)
        self.episode = torch.zeros(self.n_fields, dtype=torch.int32, device=dev)  # the kernel's uint32, bit for bit
        self.out = torch.zeros((self.rows, 2), device=dev)
        self.call = 0
        self.fresh = True  # the next call is a start call
        self._lay = VssActuateLayout(int(lay.field_stride), int(lay.team_stride), int(lay.robots), int(lay.n_teams),
                                     int(lay.first_team))
        p = self.params
        self._prm = VssActuateParams(float(p.gain_sigma), float(p.noise_sigma), float(p.deadband), float(p.loss_prob),
                                     int(p.levels))

    def start(self, call: int | None = None, zero: bool = False) -> None:
        """The next call is a start call: every field begins an episode.  `call`: set the call index; `zero`: forget
        the episode numbers too (with call=0: afresh, as a new channel)."""
        self.fresh = True
        if call is not None:
            self.call = int(call)
        if zero:
            self.held.zero_()
            self.gain.fill_(1.0)
            self.episode.zero_()

    @torch.no_grad()
    def actuate(self, cmd: torch.Tensor, done_prev: torch.Tensor | None = None, out: torch.Tensor | None = None):
        """One step: the applied commands in `cmd`'s shape, in the channel's own buffer (`cmd` is not modified) or,
        with out=cmd, in place.  `done_prev`: the done flags the previous step returned (not read by a start call)."""
        if (cmd.dtype != torch.float32 or cmd.device != self.out.device or not cmd.is_contiguous()
                or cmd.numel() != self.rows * 2):
            raise ValueError(f"cmd must be {self.rows} contiguous float32 commands of 2 on {self.out.device}, "
                             f"got {tuple(cmd.shape)} {cmd.dtype} on {cmd.device}")
        if out is not None and out is not cmd and out.data_ptr() != cmd.data_ptr():
            raise ValueError("out must be cmd itself (in place) or None (the channel's buffer)")
        dst = self.out if out is None else cmd
        done_ptr = None
        if not self.fresh:
            if not self._done_ok(done_prev):
                raise ValueError(f"done_prev must be contiguous int64 with a flag every {self.done_stride} elements for "
                                 f"{self.n_fields} fields (start() makes the next call a start call)")
            done_ptr = done_prev.data_ptr()
        rc = N.load().vss_actuate(N.stream_of(self.device), self.n_fields, ctypes.byref(self._lay), ctypes.byref(self._prm),
                                self.seed, self.call & 0xFFFFFFFF, cmd.data_ptr(), done_ptr, self.done_stride,
                                self.held.data_ptr(), self.gain.data_ptr(), self.episode.data_ptr(), dst.data_ptr())
        N.check(rc, "vss_actuate")
        self.call += 1
        self.fresh = False
        return dst.view(cmd.shape)

    def _state_tensors(self) -> dict:
        return dict(held=self.held, gain=self.gain, episode=self.episode, out=self.out)
