"""The tracking channel (include/vss.h `vss_track`, csrc/vss_track.hip).

No VSS team feeds single camera frames to its controller: it runs a recursive tracker that predicts with a motion
model and corrects with the new frame.  The perception channel (vss_amd/perceive.py) delivers rows that are late and
noisy; the estimation channel (vss_amd/estimate.py) rolls a late row forward to the present from one frame only.
This channel sits between the two and filters the noise across frames, in the delayed frame's own time: the last
filtered row is moved one control step with the project's drive model (estimate.predict_rows -- the one copy) and
the command that moved that frame, then corrected with the new row, body by body, by a fixed gain per kind of body
behind a gate.  One launch per call; `reference_track` below is its specification: float32 numpy, one operation per
line, in the kernel's order, nothing contracted; the kernel equals it bit for bit (tests/test_track_gpu.py).

    ch = TrackingChannel(n_fields, Layout(...), delay, Params(0.2, 0.5, 0.5), device)
    rows = ch.start(obs)                          # reset(): ages 0, est = obs, the ring's slot
    rows, term_rows = ch.track(obs, term, done)   # one step: one vss_track launch, no host sync

Row layout as estimate.py's.  Every row is filtered in its own frame, independently of every other row: negation
commutes with every operation used, so a yellow row is the negated view and there is no team or world bookkeeping.
State is per row, packed (n_teams, n_fields, robots): `est` the last filtered row, `age` perception's recurrence,
`hist` a ring of the row's own-action floats, the floats of call t in slot t % delay.  Per call t and row:
  a = clamp(age, 0, D);  d = min(a + 1, D);  age' = done ? 0 : d;  adv = 1 - (d - a)
  cmd = D == 0 ? term's own-action floats : hist[(t - d) % D]   # the command that moved frame t-d-1 to frame t-d
  P = adv ? predict_rows(est, 1, cmd) : est
  term_f = update(P, term);  obs_f = done ? obs : update(P, obs)
  est = obs_f;  age = age';  hist[t % D] = obs's own-action floats
adv is 0 while perception re-delivers an episode's first frame (the update then averages the looks) and 1 once the
age is saturated, which needs D calls since the episode's first: the slot read was written by the episode's second
call at the earliest, so no command of an earlier episode is ever used.

The entry point is libvss_amd.so's, bound from include/vss.h by vss_amd/_native.py like every other: the structs, the
constants and the loader here are `_native`'s under the module's own names.  There is no fallback: a missing or stale
library raises.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N
from . import channel
from . import estimate as _E
from .estimate import OPPONENTS, OWN
from .perceive import ACTION_FLOATS, NUM_OBS, _sincos_small

F = np.float32

MAX_DELAY = N.TRACK_MAX_DELAY
VssTrackLayout = N.VssTrackLayout
VssTrackParams = N.VssTrackParams
load = N.load  # the one library's loader under the module's own name, as before


# ---- layouts and parameters -------------------------------------------------------------------------------------------
Layout = _E.Layout  # estimation's layouts: where the rows lie, whichever team's they are
of_perception = _E.of_perception
layout_sa, layout_dma, layout_mirror = _E.layout_sa, _E.layout_dma, _E.layout_mirror
layout_opponent, layout_full_blue = _E.layout_opponent, _E.layout_full_blue


class Params(NamedTuple):
    """The correction's gain per kind of body, each in [0, 1] (0: the kind is not filtered), and the gates in the
    row's units (0: off): a body whose input is further from the prediction is re-initialised from the input."""
    gain_team: float = 0.0
    gain_opp: float = 0.0
    gain_ball: float = 0.0
    gate_pos: float = 0.03
    gate_vel: float = 0.5

    def any(self) -> bool:
        return any(float(g) != 0.0 for g in self[:3])

    def check(self) -> "Params":
        for name, g in zip(self._fields[:3], self[:3]):
            if not 0.0 <= float(g) <= 1.0:  # false for a NaN
                raise ValueError(f"tracking: {name} must be in [0, 1], got {g}")
        for name, g in zip(self._fields[3:], self[3:]):
            if not 0.0 <= float(g) < float("inf"):
                raise ValueError(f"tracking: {name} must be finite and >= 0, got {g}")
        return self


# ---- the specification ----------------------------------------------------------------------------------------------
def _update_body(p, z, base: int, robot: bool, g, gate_pos, gate_vel, keep):
    """The correction of the body at `base` on rows p (the prediction) and z (the input), both (M, 52): the result's
    floats are written into a copy of z's, returned as (M, n) with n = 7 for a robot, 4 for the ball."""
    n = 7 if robot else 4
    zb = z[:, base:base + n]
    pb = p[:, base:base + n]
    o = np.empty_like(zb)
    dx = zb[:, 0] - pb[:, 0]
    dy = zb[:, 1] - pb[:, 1]
    dvx = zb[:, 2] - pb[:, 2]
    dvy = zb[:, 3] - pb[:, 3]
    o[:, 0] = pb[:, 0] + g * dx
    o[:, 1] = pb[:, 1] + g * dy
    o[:, 2] = pb[:, 2] + g * dvx
    o[:, 3] = pb[:, 3] + g * dvy
    trip = np.zeros(z.shape[0], bool)
    if gate_pos > 0:
        trip |= (np.abs(dx) > gate_pos) | (np.abs(dy) > gate_pos)
    if gate_vel > 0:
        trip |= (np.abs(dvx) > gate_vel) | (np.abs(dvy) > gate_vel)
    if robot:
        cp = pb[:, 4]
        sp = pb[:, 5]
        dot = cp * zb[:, 4] + sp * zb[:, 5]
        e = g * (cp * zb[:, 5] - sp * zb[:, 4])
        se, ce = _sincos_small(e)
        c1 = cp * ce - sp * se
        s1 = sp * ce + cp * se
        k = F(1.5) - F(0.5) * (c1 * c1 + s1 * s1)
        o[:, 4] = c1 * k
        o[:, 5] = s1 * k
        o[:, 6] = pb[:, 6] + g * (zb[:, 6] - pb[:, 6])
        trip |= dot < F(0.0)
    take_z = keep | trip | (g == F(0.0))
    return np.where(take_z[:, None], zb, o)


def update_rows(p, z, params, keep=None) -> np.ndarray:
    """update(P, z) on rows (M, 52): every body of z corrected towards z from p by its kind's gain, or z's own floats
    where the gate trips, the gain is 0 or `keep` (M,) is set; the own-action floats are z's.  A copy."""
    prm = Params(*params)
    p = np.ascontiguousarray(p, dtype=F)
    z = np.ascontiguousarray(z, dtype=F)
    keep = np.zeros(z.shape[0], bool) if keep is None else np.asarray(keep, bool)
    gate_pos, gate_vel = F(prm.gate_pos), F(prm.gate_vel)
    out = z.copy()
    with np.errstate(all="ignore"):  # rows that keep z are computed and dropped
        out[:, 0:4] = _update_body(p, z, 0, False, F(prm.gain_ball), gate_pos, gate_vel, keep)
        for base in OWN:
            out[:, base:base + 7] = _update_body(p, z, base, True, F(prm.gain_team), gate_pos, gate_vel, keep)
        for base in OPPONENTS:
            out[:, base:base + 7] = _update_body(p, z, base, True, F(prm.gain_opp), gate_pos, gate_vel, keep)
    return out


def reference_track(obs, term, done, est, hist, age, call: int, delay: int, params):
    """One call of the channel on packed rows -- the specification.

    obs, term: (n_teams, n_fields, robots, 52) float32 perceived rows (term None: the start call); done (n_fields,);
    est (n_teams, n_fields, robots, 52) float32, hist (delay, n_teams, n_fields, robots, 6) float32 and age
    (n_teams, n_fields, robots) int32 are updated in place.  Returns (obs_f, term_f) in the shape of obs; term_f is
    None for the start call."""
    obs = np.ascontiguousarray(obs, dtype=F)
    if obs.ndim != 4 or obs.shape[-1] != NUM_OBS or obs.shape[0] not in (1, 2) or obs.shape[2] not in (1, 3):
        raise ValueError(f"obs must be (n_teams, n_fields, robots, 52), got {obs.shape}")
    D = int(delay)
    if not 0 <= D <= MAX_DELAY:
        raise ValueError(f"delay must be in 0..{MAX_DELAY}, got {delay}")
    prm = Params(*params).check()
    shape = obs.shape[:3]
    if (hist.shape != (D,) + shape + (6,) or hist.dtype != F or age.shape != shape or age.dtype != np.int32
            or est.shape != obs.shape or est.dtype != F or not est.flags.c_contiguous):
        raise ValueError(f"est must be contiguous float32 {obs.shape}, hist float32 {(D,) + shape + (6,)} and age int32 "
                         f"{shape}, got {est.shape} {est.dtype}, {hist.shape} {hist.dtype} and {age.shape} {age.dtype}")
    m = int(np.prod(shape))
    acts = list(ACTION_FLOATS)
    rows = obs.reshape(m, NUM_OBS)
    own = rows[:, acts]
    state = est.reshape(m, NUM_OBS)  # a view
    ring = hist.reshape(D, m, 6)     # a view: hist is contiguous or the reshape would copy
    if D and not np.shares_memory(ring, hist):
        raise ValueError("hist must be contiguous")
    t = int(call)
    term_f = None
    if term is None:
        age[:] = 0
        obs_f = rows.copy()
    else:
        term_rows = np.ascontiguousarray(term, dtype=F).reshape(m, NUM_OBS)
        done_rows = np.broadcast_to((np.asarray(done).reshape(shape[1]) != 0)[None, :, None], shape).reshape(m)
        a = np.clip(age.reshape(m), 0, D)
        d = np.minimum(a + 1, D).astype(np.int32)
        new = np.where(done_rows, 0, d).astype(np.int32)
        adv = 1 - (d - a)
        if D:
            cmd = ring[(t - d) % D, np.arange(m)]
        else:
            cmd = term_rows[:, acts]
        P = _E.predict_rows(state, adv, cmd[:, None, :])  # a row with adv 0 is est bit for bit
        term_f = update_rows(P, term_rows, prm).reshape(obs.shape)
        obs_f = update_rows(P, rows, prm, keep=done_rows)
        age[:] = new.reshape(shape)
    state[:] = obs_f
    if D:
        ring[t % D] = own
    return obs_f.reshape(obs.shape), term_f


# ---- the kernel's side ----------------------------------------------------------------------------------------------
class TrackingChannel(channel.Channel):
    """The filtered rows, the command ring, the ages, the outputs and the host call counter of one set of rows.

    `rows`: the rows of the buffers handed to start() / track() (default: the layout's span); the outputs have that
    many rows and are returned in the inputs' shape.  `done_stride`: int64 elements from one field's done flag to the
    next.  Rows the layout does not cover stay zero in the outputs."""

    def __init__(self, n_fields: int, layout, delay: int = 0, params=Params(), device="cuda", done_stride: int = 1,
                 rows: int | None = None):
        self.device = N.require_device(device)
        load()
        self.n_fields, self.layout, self.delay = int(n_fields), Layout(*layout), int(delay)
        self.params = Params(*params).check()
        self.done_stride = int(done_stride)
        if not 0 <= self.delay <= MAX_DELAY:
            raise ValueError(f"tracking: the delay must be in 0..{MAX_DELAY} steps, got {delay}")
        self._set_rows(rows)
        lay, dev = self.layout, self.device
        packed = (lay.n_teams, self.n_fields, lay.robots)
        self.est = torch.zeros(packed + (NUM_OBS,), device=dev)
        self.hist = torch.zeros((self.delay,) + packed + (6,), device=dev)
        self.age = torch.zeros(packed, dtype=torch.int32, device=dev)
        self.obs_out = torch.zeros((self.rows, NUM_OBS), device=dev)
        self.term_out = torch.zeros((self.rows, NUM_OBS), device=dev)
        self.call = 0
        self._no_done = torch.zeros(1, dtype=torch.long, device=dev)
        self._lay = VssTrackLayout(int(lay.field_stride), int(lay.team_stride), int(lay.robots), int(lay.n_teams))
        self._prm = VssTrackParams(*(float(x) for x in self.params))

    def _launch(self, obs, term, done) -> None:
        rc = load().vss_track(
            N.stream_of(self.device), self.n_fields, ctypes.byref(self._lay), ctypes.byref(self._prm), self.delay,
            self.call & 0xFFFFFFFF, obs.data_ptr(), N.ptr(term), done.data_ptr(), self.done_stride, self.est.data_ptr(),
            self.hist.data_ptr() if self.delay else None, self.age.data_ptr(), self.obs_out.data_ptr(),
            None if term is None else self.term_out.data_ptr())
        N.check(rc, "vss_track")
        self.call += 1

    @torch.no_grad()
    def start(self, obs: torch.Tensor, call: int = 0) -> torch.Tensor:
        """reset(): every row's age 0, est = obs, the current slot written, obs itself returned (call index `call`)."""
        self._check_rows(obs, "obs")
        self.call = int(call)
        self._launch(obs, None, self._no_done)  # the start call reads no done flag
        return self.obs_out.view(obs.shape)

    @torch.no_grad()
    def track(self, obs: torch.Tensor, term: torch.Tensor, done: torch.Tensor):
        """One step: (filtered obs, filtered terminal obs) in the inputs' shapes; the buffers are the channel's."""
        self._check_rows(obs, "obs")
        self._check_rows(term, "term")
        self._check_done(done)
        self._launch(obs, term, done)
        return self.obs_out.view(obs.shape), self.term_out.view(term.shape)

    def _state_tensors(self) -> dict:
        return dict(est=self.est, hist=self.hist, age=self.age, obs_out=self.obs_out, term_out=self.term_out)
