"""The estimation channel (include/vss.h `vss_estimate`, csrc/vss_estimate.hip).

A real VSS team never feeds late camera frames to its controller: it rolls every frame forward by the known latency
with a motion model, which it can do because it knows what it commanded in the meantime.  The perception channel
(vss_amd/perceive.py) delivers rows that are up to `delay` control steps old, whose six own-action floats are the
current step's commands.  This channel turns each such row (state of call t - L) into an estimate of the state at
call t, by running the project's own drive model L times with the commands of calls
t - L + 1 .. t, in one launch per call.  `reference_estimate` below is its specification: float32 numpy, one
operation per line, in the kernel's order; the kernel equals it bit for bit (tests/test_estimate_gpu.py).  Only
+ - * /, comparisons, selects, integer operations and perceive.py's `_sincos_small` (the kernel's: csrc/vss_numerics.h)
occur, every one correctly rounded in both, and nothing is contracted into an FMA.

    ch = EstimationChannel(n_fields, Layout(...), delay, device)
    rows = ch.start(obs)                            # reset(): ages 0, the ring's slot, obs itself
    rows, term_rows = ch.estimate(obs, term, done)  # one step: one vss_estimate launch, no host sync

Row layout (envs/vss.py compute_obs): ball x y vx vy [0:4]; own robot j at 4 + 9 j: x y vx vy cos sin w aL aR;
opponent j at 31 + 7 j: x y vx vy cos sin w.  Every row is estimated in its own frame, independently of every other
row: the 180-degree mirror commutes with the dynamics and negation with every rounding used, so there is no team or
world bookkeeping.  State is per row: `age` follows perception's recurrence, `hist` is a ring of the row's own-action
floats, the floats of call t in slot t % delay.  Per call (index t) and row, with its field's `done`:
  d = min(age + 1, delay);  age' = done ? 0 : d
  term_e = predict(term, lead d,    commands hist[t - d + 1 .. t - 1], then term's own-action floats)
  obs_e  = predict(obs,  lead age', commands hist[t - age' + 1 .. t - 1], then obs's own-action floats)
  hist[t % delay] = obs's own-action floats
A lead is at most the number of calls since the episode's first, so the oldest slot read was written by the episode's
second call: no command of an earlier episode is ever used.  There are no contacts and no walls: a body that would
have hit something is predicted through it.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N
from . import channel
from . import perceive as _P
from .perceive import ACTION_FLOATS, NUM_OBS, _sincos_small

F = np.float32
OWN = (4, 13, 22)        # where own robot j's nine floats begin
OPPONENTS = (31, 38, 45)  # where opponent j's seven floats begin
NSUB = 2                 # substeps per control step, of h = 0.025 s

MAX_DELAY = N.ESTIMATE_MAX_DELAY
VssEstimateLayout = N.VssEstimateLayout
load = N.load  # the one library's loader under the module's own name, as before


class Layout(NamedTuple):
    """Where the rows lie (include/vss.h vss_estimate_layout), strides in 52-float rows: perception's
    layout without first_team -- a row is estimated in its own frame, whichever team's it is."""
    field_stride: int
    team_stride: int = 0
    robots: int = 1
    n_teams: int = 1

    def span(self, n_fields: int) -> int:
        """Rows from the first row to the last one's end."""
        return channel.span(self, n_fields)

    def row_index(self, n_fields: int) -> np.ndarray:
        """(n_teams, n_fields, robots) int64: the row of team block b, field f, robot k."""
        return channel.index(self, n_fields)


def of_perception(layout) -> Layout:
    """A perception layout's rows (DESIGN.md §17.2's table), without its first_team."""
    return Layout(*tuple(layout)[:4])


def layout_sa() -> Layout:
    return of_perception(_P.layout_sa())


def layout_dma() -> Layout:
    return of_perception(_P.layout_dma())


def layout_mirror(field_rows: int, n_fields: int) -> Layout:
    return of_perception(_P.layout_mirror(field_rows, n_fields))


def layout_opponent() -> Layout:
    """The versus step's opp_obs (N, 3, 52): as DMA's rows."""
    return of_perception(_P.layout_opponent())


def layout_full_blue() -> Layout:
    """The blue rows of FULL's (N, 2, 3, 52); the yellow rows are neither read nor written."""
    return of_perception(_P.layout_full_blue())


# ---- the specification ----------------------------------------------------------------------------------------------
def _clamp(x, lim):
    return np.where(x < -lim, -lim, np.where(x > lim, lim, x)).astype(F)


def _substep(v: np.ndarray, tl, tr) -> None:
    """One substep of h = 0.025 on rows v (M, 52), in place; tl, tr: three (M,) wheel-rim targets each.  The drive
    lines are those of oracle/vss_oracle.c physics_field with (c, s) taken from the row."""
    for j, B in enumerate(OWN):
        c = v[:, B + 4]
        s = v[:, B + 5]
        vx = v[:, B + 2]
        vy = v[:, B + 3]
        w = v[:, B + 6]
        vf = c * vx + s * vy
        vl = c * vy - s * vx
        wl = vf - w * F(0.03375)
        wr = vf + w * F(0.03375)
        wl = wl + _clamp(tl[j] - wl, F(0.15))
        wr = wr + _clamp(tr[j] - wr, F(0.15))
        vf = (wl + wr) * F(0.5)
        w = (wr - wl) * F(14.814815)
        vl = vl - _clamp(vl, F(0.171675))
        nvx = c * vf - s * vl
        nvy = s * vf + c * vl
        v[:, B + 6] = w
        v[:, B + 2] = nvx
        v[:, B + 3] = nvy
    v[:, 2] = v[:, 2] * F(0.99625)
    v[:, 3] = v[:, 3] * F(0.99625)
    for B in (0,) + OWN + OPPONENTS:
        v[:, B + 0] = v[:, B + 0] + v[:, B + 2] * F(0.025)
        v[:, B + 1] = v[:, B + 1] + v[:, B + 3] * F(0.025)
    for B in OWN + OPPONENTS:
        c = v[:, B + 4].copy()
        s = v[:, B + 5].copy()
        se, ce = _sincos_small(v[:, B + 6] * F(0.025))
        c1 = c * ce - s * se
        s1 = s * ce + c * se
        k = F(1.5) - F(0.5) * (c1 * c1 + s1 * s1)
        v[:, B + 4] = c1 * k
        v[:, B + 5] = s1 * k


def predict_rows(rows, lead, cmds) -> np.ndarray:
    """rows (M, 52) rolled forward: row m by lead[m] control steps, step i (0-based) with cmds[m, i] (six floats: own
    robot j's left and right wheel at 2 j, 2 j + 1).  lead: an integer or (M,); cmds (M, >= max lead, 6).  A copy; a
    row with lead 0 is unchanged bit for bit, and the own-action floats are the input's."""
    rows = np.array(rows, dtype=F, copy=True)
    if rows.ndim != 2 or rows.shape[1] != NUM_OBS:
        raise ValueError(f"rows must be (M, 52), got {rows.shape}")
    m = rows.shape[0]
    lead = np.broadcast_to(np.asarray(lead, dtype=np.int64), (m,))
    cmds = np.asarray(cmds, dtype=F).reshape(m, -1, 6)
    top = int(lead.max()) if m else 0
    if lead.min(initial=0) < 0 or cmds.shape[1] < top:
        raise ValueError(f"leads must be >= 0 with a command for every step, got leads up to {top} and {cmds.shape[1]} commands")
    with np.errstate(all="ignore"):  # rows past their lead are computed and dropped
        for i in range(top):
            v = rows.copy()
            a = cmds[:, i]
            tl = [(a[:, 2 * j] * F(42.0)) * F(0.024) for j in range(3)]
            tr = [(a[:, 2 * j + 1] * F(42.0)) * F(0.024) for j in range(3)]
            for _ in range(NSUB):
                _substep(v, tl, tr)
            live = i < lead
            rows[live] = v[live]
    return rows


def _commands(own, hist, lead, slot_w: int, delay: int) -> np.ndarray:
    """(M, delay, 6): step i of a row with lead L takes the commands of call t - (L - 1 - i): the ring's for a call
    before t, the row's own-action floats for call t itself."""
    m = own.shape[0]
    cmds = np.zeros((m, max(delay, 1), 6), F)
    for i in range(delay):
        back = lead - 1 - i  # calls before t; negative: the step is not run
        slot = np.where(back >= 1, (slot_w - back) % max(delay, 1), 0)
        cmds[:, i] = np.where((back >= 1)[:, None], hist[slot, np.arange(m)], own)
    return cmds


def reference_estimate(obs, term, done, hist, age, call: int, delay: int):
    """One call of the channel on packed rows -- the specification.

    obs, term: (n_teams, n_fields, robots, 52) float32 perceived rows (term None: the start call); done (n_fields,);
    hist (delay, n_teams, n_fields, robots, 6) float32 and age (n_teams, n_fields, robots) int32 are updated in
    place.  Returns (obs_e, term_e) in the shape of obs; term_e is None for the start call."""
    obs = np.ascontiguousarray(obs, dtype=F)
    if obs.ndim != 4 or obs.shape[-1] != NUM_OBS or obs.shape[0] not in (1, 2) or obs.shape[2] not in (1, 3):
        raise ValueError(f"obs must be (n_teams, n_fields, robots, 52), got {obs.shape}")
    D = int(delay)
    if not 0 <= D <= MAX_DELAY:
        raise ValueError(f"delay must be in 0..{MAX_DELAY}, got {delay}")
    shape = obs.shape[:3]
    if (hist.shape != (D,) + shape + (6,) or hist.dtype != F or age.shape != shape or age.dtype != np.int32):
        raise ValueError(f"hist must be float32 {(D,) + shape + (6,)} and age int32 {shape}, got {hist.shape} {hist.dtype} "
                         f"and {age.shape} {age.dtype}")
    m = int(np.prod(shape))
    acts = list(ACTION_FLOATS)
    rows = obs.reshape(m, NUM_OBS)
    own = rows[:, acts]
    ring = hist.reshape(D, m, 6)  # a view: hist is contiguous or the reshape below would copy
    if D and not np.shares_memory(ring, hist):
        raise ValueError("hist must be contiguous")
    slot_w = int(call) % D if D else 0
    term_e = None
    if term is None:
        age[:] = 0
        obs_e = rows.copy()
    else:
        term_rows = np.ascontiguousarray(term, dtype=F).reshape(m, NUM_OBS)
        done_rows = np.broadcast_to((np.asarray(done).reshape(shape[1]) != 0)[None, :, None], shape).reshape(m)
        a = np.clip(age.reshape(m), 0, D)
        d = np.minimum(a + 1, D).astype(np.int32)
        new = np.where(done_rows, 0, d).astype(np.int32)
        term_e = predict_rows(term_rows, d, _commands(term_rows[:, acts], ring, d, slot_w, D))
        obs_e = predict_rows(rows, new, _commands(own, ring, new, slot_w, D))
        age[:] = new.reshape(shape)
        term_e = term_e.reshape(obs.shape)
    if D:
        ring[slot_w] = own
    return obs_e.reshape(obs.shape), term_e


# ---- the kernel's side ----------------------------------------------------------------------------------------------
class EstimationChannel(channel.Channel):
    """The command ring, the ages, the outputs and the host call counter of one set of rows.

    `rows`: the rows of the buffers handed to start() / estimate() (default: the layout's span); the outputs have that
    many rows and are returned in the inputs' shape.  `done_stride`: int64 elements from one field's done flag to the
    next.  Rows the layout does not cover stay zero in the outputs."""

    def __init__(self, n_fields: int, layout, delay: int = 0, device="cuda", done_stride: int = 1, rows: int | None = None):
        self.device = N.require_device(device)
        self.n_fields, self.layout, self.delay = int(n_fields), Layout(*layout), int(delay)
        self.done_stride = int(done_stride)
        if not 0 <= self.delay <= MAX_DELAY:
            raise ValueError(f"estimation: the delay must be in 0..{MAX_DELAY} steps, got {delay}")
        self._set_rows(rows)
        lay, dev = self.layout, self.device
        packed = (lay.n_teams, self.n_fields, lay.robots)
        self.hist = torch.zeros((self.delay,) + packed + (6,), device=dev)
        self.age = torch.zeros(packed, dtype=torch.int32, device=dev)
        self.obs_out = torch.zeros((self.rows, NUM_OBS), device=dev)
        self.term_out = torch.zeros((self.rows, NUM_OBS), device=dev)
        self.call = 0
        self._no_done = torch.zeros(1, dtype=torch.long, device=dev)
        self._lay = VssEstimateLayout(int(lay.field_stride), int(lay.team_stride), int(lay.robots), int(lay.n_teams))

    def _launch(self, obs, term, done) -> None:
        rc = N.load().vss_estimate(
            N.stream_of(self.device), self.n_fields, ctypes.byref(self._lay), self.delay, self.call & 0xFFFFFFFF,
            obs.data_ptr(), N.ptr(term), done.data_ptr(), self.done_stride,
            self.hist.data_ptr() if self.delay else None, self.age.data_ptr(), self.obs_out.data_ptr(),
            None if term is None else self.term_out.data_ptr())
        N.check(rc, "vss_estimate")
        self.call += 1

    @torch.no_grad()
    def start(self, obs: torch.Tensor, call: int = 0) -> torch.Tensor:
        """reset(): every row's age 0, the current slot written, obs itself returned (call index `call`)."""
        self._check_rows(obs, "obs")
        self.call = int(call)
        self._launch(obs, None, self._no_done)  # the start call reads no done flag
        return self.obs_out.view(obs.shape)

    @torch.no_grad()
    def estimate(self, obs: torch.Tensor, term: torch.Tensor, done: torch.Tensor):
        """One step: (estimated obs, estimated terminal obs) in the inputs' shapes; the buffers are the channel's."""
        self._check_rows(obs, "obs")
        self._check_rows(term, "term")
        self._check_done(done)
        self._launch(obs, term, done)
        return self.obs_out.view(obs.shape), self.term_out.view(term.shape)

    def _state_tensors(self) -> dict:
        return dict(hist=self.hist, age=self.age, obs_out=self.obs_out, term_out=self.term_out)
