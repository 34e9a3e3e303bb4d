"""Directed edge states for the step: rare branches and exact ties — TEST INFRASTRUCTURE, no test here.

The parity tests reach the physics through uniform resets and random actions, so they almost never
enter the rare branches of DESIGN.md §3 (a centre inside a box or a wall, a default normal, the
range-reduction arms of the polynomial sin/cos) and never sit on a tie (`<` against `<=`).  This
table writes such states directly, one field each, as `run_hip` of test_physics_known_answers.py
writes its scenarios.  tests/test_step_edges_cpu.py proves on the CPU that every entry discriminates
(a mutated oracle differs on the entries built for that mutation and on no other), and
tests/test_step_edges_gpu.py runs the HIP kernels on the table bit for bit against the oracle.

How a tie is made to hold *after* the substep's integration (the contacts see x + v h):
  * positional ties use zero velocities and zero actions: x + 0 h is exact;
  * a tie that needs a velocity (an impulse at exactly the touching distance) uses a velocity so
    small that fl(x + fl(v h)) == x: |v h| below half an ulp of the coordinate (5e-8 m/s on
    coordinates of 0.125 m and more).  The ball keeps such a velocity through its damping; a robot
    gets it from a wheel command of 5e-8, which the traction-limited drive turns into 5.04e-8 m/s
    along its heading.  The velocity decides the branch (`vn < 0`) exactly as a large one would;
  * where the tie is a sum of rounded products (d2 == r2) the neighbouring floats of one coordinate
    are searched in numpy float32 with the oracle's own operation order until the tie is hit.

Every base case is expanded mechanically over the robot index it concerns (0..5: robots 0-2 and 3-5
run on different lane halves of physics_split) and over the four sign quadrants (the walls are folded
through |x|, |y|).  A reflection negates positions and velocities, maps the yaw quaternion
(qz, qw) -> (qw, qz) (x) or (-qz, qw) (y), negates the yaw rate and swaps the wheels, all exact in
float32, so a reflected case sits on the reflected tie; it also turns every +0.0 coordinate into -0.0.

Ties that float32 cannot reach (kept here, not dropped silently):
  * goal-post corner with 0 < d <= 1e-9: |x| next to 0.75 moves by 6e-8 and |y| next to 0.2 by 1.5e-8,
    so d is 0 or at least 1.5e-8; only d == 0 (default normal) exists.  The robot-robot twin of this
    threshold is reachable next to the origin and is in the table (rr/tiny_offset).
  * a ball ending a step at |y| == 0.2 with |x| > 0.75 (the goal's `<`): the pocket side face or the
    end wall, resolved last in the step, pushes such a ball to |y| = 0.2 - r or out of the wall.
  * d2 == r2 of the ball against a FACE of the box: d2 = fl(ex ex) with ex on the 2^-28 lattice of lx - 0.035f,
    five ulps of d2 a step, and no ex squares to 0.00045539559f; the face cases take the nearest d2 on either
    side, the corner cases (a sum of two squares) sit on the tie itself.
  * pen == 0 of the robot against the pocket's side face: fl(a + 0.04f) next to 0.2f is always a rounding tie
    whose even neighbour is not 0.2f; only the nearest pen < 0 and pen > 0 exist (the ball reaches 0 there).
  * a clamp has no tie to decide (clamp(x) == x on the limit itself); the drive and action limits are
    pinned by the value on the limit and one ulp past it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

F = np.float32
CH_RX, CH_RY, CH_RQZ, CH_RQW, CH_RVX, CH_RVY, CH_RW = 4, 10, 28, 34, 40, 46, 52
STATE_CHANNELS = 58

# the oracle's constants, as float32 (oracle/vss_oracle.c)
HH = F(0.0125)          # half the substep: the yaw step's half-angle factor
HX, HY, GY, BACK = F(0.75), F(0.65), F(0.2), F(0.85)
BALL_R, BALL_R2, ROBOT_R, HALF = F(0.02134), F(0.00045539559), F(0.04), F(0.035)
RR_DIST, RR_DIST2 = F(0.08), F(0.0064)
HALF_TRACK, INV_TRACK, DV, DL = F(0.03375), F(14.814815), F(0.15), F(0.171675)
WHEEL = (F(42.0), F(0.024))

MAX_LEN = 400          # the episode length of the packed table; cases for 1 and 2 run in launches of their own
TINY_V = F(5e-8)       # below half an ulp of every coordinate >= 0.125 after v * 0.025
TINY_A = F(5e-8)       # wheel command that gives a robot TINY_V * 1.008 along its heading

# bodies that are not part of a case: clear of every case region, of the walls and of each other
PARK = [(-0.6, -0.5), (-0.6, 0.5), (0.0, -0.5), (0.6, -0.5), (0.6, 0.5), (0.3, 0.5)]
BALL_PARK = (-0.45, 0.25)


def ulps(x, k=1):
    """The float32 k ulps above (k > 0) or below (k < 0) x."""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def near(x0, span=2048):
    """The 2 span + 1 float32 neighbours of x0 > 0, nearest first."""
    b = int(np.array([x0], F).view(np.int32)[0])
    ks = np.arange(-span, span + 1)
    ks = ks[np.argsort(np.abs(ks), kind="stable")]
    return (b + ks).astype(np.int32).view(F)


def quat(yaw):
    return F(math.sin(yaw / 2)), F(math.cos(yaw / 2))


# the yaws of the ball-robot cases: 0, pi/2, pi, an odd angle, and an odd angle with qw < 0
SQ = F(math.sqrt(0.5))
YAWS = {"yaw0": (F(0), F(1)), "yaw90": (SQ, SQ), "yaw180": (F(1), F(0)), "yaw_odd": quat(0.7),
        "qw_neg": tuple(-v for v in quat(2.3))}


def heading(q):
    qz, qw = q
    return qw * qw - qz * qz, F(2) * qw * qz


# ------------------------------------------------------------------------------------ one field
class Field:
    def __init__(self):
        s = np.zeros(STATE_CHANNELS, F)
        for r, (x, y) in enumerate(PARK):
            s[CH_RX + r], s[CH_RY + r] = x, y
        s[CH_RQW:CH_RQW + 6] = 1.0
        s[0], s[1] = BALL_PARK
        self.s, self.a, self.progress, self.max_len = s, np.zeros(12, F), 0, MAX_LEN

    def robot(self, r, x, y, q=(F(0), F(1)), vx=0.0, vy=0.0, w=0.0, act=(0.0, 0.0)):
        s = self.s
        s[CH_RX + r], s[CH_RY + r], s[CH_RQZ + r], s[CH_RQW + r] = x, y, q[0], q[1]
        s[CH_RVX + r], s[CH_RVY + r], s[CH_RW + r] = vx, vy, w
        self.a[2 * r], self.a[2 * r + 1] = act
        return self

    def ball(self, x, y, vx=0.0, vy=0.0):
        self.s[0:4] = (x, y, vx, vy)
        return self

    def time(self, progress, max_len=MAX_LEN):
        self.progress, self.max_len = progress, max_len
        return self


@dataclass
class Base:
    name: str
    tags: tuple           # what the case is built for: the CPU test's mutants name these
    k: int                # robots it concerns: members(r)[:k]; 0: none (ball and walls only)
    build: object         # (r) -> Field
    note: str
    split: bool = False   # a pair of r and third(r) instead of r and mate(r)


@dataclass
class Case:
    name: str
    base: str
    tags: tuple
    robots: frozenset
    state: np.ndarray
    actions: np.ndarray
    progress: int
    max_len: int
    note: str = field(repr=False, default="")


BASES: list[Base] = []

# The second and third robot of a case about robot r.  Over r = 0..5 the pairs are (0,3) (1,2) (2,1) (3,4) (4,5)
# (5,0): both orders of a pair, pairs inside either lane half and across them (i < 3 <= j), and robots 1 and 2
# only where r is 1 or 2, so the single-agent step, whose blue robots 1-2 are noise-driven, keeps four of six.
MATE, THIRD = (3, 2, 1, 4, 5, 0), (4, 0, 0, 5, 0, 3)


def mate(r):
    return MATE[r]


def third(r):
    return THIRD[r]


def members(r, k, split=False):
    return ((r, third(r)) if split else (r, mate(r), third(r)))[:k]


def add(name, tags, k, note, split=False):
    def deco(fn):
        assert all(b.name != name for b in BASES), name
        BASES.append(Base(name, tuple(tags), k, fn, note, split))
        return fn
    return deco


def reflect(state, actions, sx, sy):
    """The field reflected through x (sx = -1) and / or y (sy = -1); exact in float32."""
    s, a = state.copy(), actions.copy()
    for ch, sg in ((0, sx), (1, sy), (2, sx), (3, sy)):
        s[ch] = s[ch] * F(sg)
    for r in range(6):
        s[CH_RX + r], s[CH_RVX + r] = s[CH_RX + r] * F(sx), s[CH_RVX + r] * F(sx)
        s[CH_RY + r], s[CH_RVY + r] = s[CH_RY + r] * F(sy), s[CH_RVY + r] * F(sy)
        if sx < 0:
            s[CH_RQZ + r], s[CH_RQW + r] = s[CH_RQW + r], s[CH_RQZ + r]
        if sy < 0:
            s[CH_RQZ + r] = -s[CH_RQZ + r]
        if sx * sy < 0:
            s[CH_RW + r] = -s[CH_RW + r]
            a[2 * r], a[2 * r + 1] = a[2 * r + 1], a[2 * r]
    return s, a


QUADRANTS = [(1, 1), (-1, 1), (1, -1), (-1, -1)]


def expand(base: Base) -> list[Case]:
    out = []
    for r in (range(6) if base.k else (0,)):
        f = base.build(r)
        robots = frozenset(members(r, base.k, base.split))
        for sx, sy in QUADRANTS:
            s, a = reflect(f.s, f.a, sx, sy)
            out.append(Case(f"{base.name}/r{r}/{'+-'[sx < 0]}{'+-'[sy < 0]}", base.name, base.tags, robots,
                            s, a, f.progress, f.max_len, base.note))
    return out


def base_cases() -> list[Case]:
    """Every base case once: robot index 0, first quadrant."""
    out = []
    for b in BASES:
        f = b.build(0)
        out.append(Case(b.name, b.name, b.tags, frozenset(members(0, b.k, b.split)), f.s.copy(), f.a.copy(), f.progress,
                        f.max_len, b.note))
    return out


def table() -> list[Case]:
    return [c for b in BASES for c in expand(b)]


def pack(cases):
    """(58, n) state, (n, 12) actions and (n,) progress of a list of cases with one episode length."""
    assert len({c.max_len for c in cases}) == 1
    state = np.ascontiguousarray(np.stack([c.state for c in cases], axis=1))
    return state, np.stack([c.actions for c in cases]), np.array([c.progress for c in cases], np.int64)


# ------------------------------------------------------------------------------------ walls
def toward(dx, dy):
    """Quaternion of the heading (dx, dy)."""
    return quat(math.atan2(dy, dx))


def place(body, r, x, y, into=None):
    """`body` ("robot": index r, or "ball") at rest at (x, y); `into` = (dx, dy): a sub-ulp velocity that way."""
    f = Field()
    if body == "ball":
        v = (0.0, 0.0) if into is None else (TINY_V * F(into[0]), TINY_V * F(into[1]))
        return f.ball(x, y, *v)
    if into is None:
        return f.robot(r, x, y)
    return f.robot(r, x, y, q=toward(*into), act=(TINY_A, TINY_A))


def corner_tie(rad):
    """(ax, ay) with fl(fl(dx dx) + fl(dy dy)) == fl(rad rad) against the goal-post corner (0.75, 0.2)."""
    r2 = rad * rad
    for fx, fy in ((0.6, 0.8), (0.8, 0.6)):  # the contact direction; some directions have no tie at all
        for ax in near(HX - F(fx) * rad, 256):
            dx = ax - HX
            ays = near(GY - F(fy) * rad, 1024)
            dy = ays - GY
            hit = np.nonzero(dx * dx + dy * dy == r2)[0]
            if hit.size:
                return ax, ays[hit[0]]
    raise AssertionError("no corner tie")


def plane_tie(limit, rad):
    """{"under", "zero", "over"} -> coordinate a: fl(fl(a + rad) - limit) == 0 and its nearest neighbours with
    pen < 0 and pen > 0.  Where a + rad always rounds past the limit (the robot against the pocket's side face:
    every sum is a rounding tie and the even neighbour is never 0.2f) there is no "zero" entry."""
    around = np.sort(near(limit - rad, 64))
    pen = (around + rad) - limit
    out = {"under": around[pen < 0][-1], "over": around[pen > 0][0]}
    if (pen == 0).any():
        out["zero"] = around[pen == 0][0]
    return out


def inexact_normal_x(rad):
    """ax beside the post (dy == 0, d < rad) whose unit normal dx * fl(1 / |dx|) is not exactly -1: the corner
    branch then leaves avx (1 - nx nx) != 0 where the end-wall face would leave 0."""
    for ax in near(HX - F(0.5) * rad, 512):
        dx = ax - HX
        if dx * (F(1) / np.sqrt(dx * dx)) != F(-1):
            return ax
    raise AssertionError("every normal is exact")


def wall_cases(body, rad):
    k = 1 if body == "robot" else 0
    B = body

    def case(name, tags, note, x, y, into=None):
        add(f"wall/{B}/{name}", tags, k, note)(lambda r, x=x, y=y, into=into: place(B, r, x, y, into))

    # |x| exactly 0.75 with |y| below, at and above 0.2
    on_line = ["goal_gt"] if body == "ball" else []  # a ball resting on the goal line inside the mouth
    case("x075_y_below", ["ax_le_hx"] + on_line, "ax == 0.75, corner branch, no contact", HX, 0.1)
    case("x075_y_under_gy", ["ax_le_hx"] + on_line, "ax == 0.75, one ulp under the post: corner, normal -y", HX, ulps(GY, -1))
    case("x075_y_gy", ["ax_le_hx", "corner_default"], "centre exactly on the goal-post corner: d == 0, default normal",
         HX, GY)
    case("x075_y_gy_moving", ["ax_le_hx", "corner_default"], "centre on the corner with a velocity into it", HX, GY,
         into=(1, 1))
    case("x075_y_over_gy", ["ax_le_hx"], "ax == 0.75, one ulp over the post: end wall face", HX, ulps(GY, 1))
    case("x075_y_above", ["ax_le_hx"], "ax == 0.75 facing the end wall", HX, 0.3)
    # |y| exactly 0.2 inside the field (corner branch with dy == 0) and inside the pocket (side face)
    # (position and pen round to the same floats on the corner branch and on the end-wall face; the velocity tells
    # them apart where the corner's unit normal is inexact)
    for i, x in enumerate((0.74, 0.7431, inexact_normal_x(rad))):
        case(f"y_gy_field{i}", ["ay_le_gy_field"], "ay == 0.2 beside the post, field side: corner branch, dy == 0",
             F(x), GY, into=(1, 0))
    for i, x in enumerate((0.76, 0.8)):
        case(f"y_gy_pocket{i}", ["ay_le_gy_pocket"], "ay == 0.2 past the goal line: pocket side face, not the end wall",
             F(x), GY)
    # goal-post corner at d2 just below, at and just above r2, moving into it
    ax, ay = corner_tie(rad)
    for nm, dk in (("below", 1), ("at", 0), ("above", -1)):
        case(f"corner_d2_{nm}", ["corner_lt"], f"goal-post corner, d2 {nm} r2, velocity into the corner", ax,
             ulps(ay, dk), into=(1, 1))
    # centre inside the end wall
    case("in_wall_px_lt_py", ["wall_px_py"], "centre inside the end wall, px < py: out through x", 0.76, 0.26)
    case("in_wall_px_gt_py", ["wall_px_py"], "centre inside the end wall, px > py: out through y", 0.80, 0.21)
    case("in_wall_px_gt_py_moving", ["wall_px_py"], "centre inside the end wall, px > py, moving further in", 0.80, 0.21,
         into=(0, 1))
    case("in_wall_px_lt_py_moving", ["wall_px_py", "end_pen"], "centre inside the end wall, px < py, moving further in", 0.76, 0.26,
         into=(1, 0))
    case("in_wall_px_eq_py", ["wall_px_py"], "centre inside the end wall, px == py (both 2^-6 + r): out through y",
         HX + F(2.0 ** -6), GY + F(2.0 ** -6))
    # side wall and goal back wall at pen == 0 and one ulp either side (moving into the wall)
    ys, xb = plane_tie(HY, rad), plane_tie(BACK, rad)
    for nm in ("under", "zero", "over"):
        if nm in ys:
            case(f"side_pen_{nm}", ["side_pen"], f"side wall, pen one ulp {nm} / exactly 0", -0.2, ys[nm], into=(0, 1))
        if nm in xb:
            case(f"back_pen_{nm}", ["back_pen"], f"goal back wall, pen one ulp {nm} / exactly 0", xb[nm], 0.05, into=(1, 0))
    ye, xp = plane_tie(GY, rad), plane_tie(HX, rad)
    for nm in ("under", "zero", "over"):
        if nm in xp:
            case(f"end_pen_{nm}", ["end_pen"], f"end wall face, pen one ulp {nm} / exactly 0", xp[nm], 0.4, into=(1, 0))
        if nm in ye:
            case(f"pocket_pen_{nm}", ["pocket_pen"], f"pocket side face, pen one ulp {nm} / exactly 0", 0.8, ye[nm], into=(0, 1))
    # two walls in one substep
    case("pocket_side_and_back", [], "pocket side face and back wall in the same substep", 0.83, 0.18)
    case("end_and_side", [], "end wall face and side wall in the same substep", 0.73, 0.63)
    # zeros: the reflections make them -0.0
    case("x_zero", ["zero"], "x == +0.0 / -0.0 (sx of the fold)", 0.0, 0.3)
    case("y_zero", ["zero"], "y == +0.0 / -0.0 (sy of the fold)", 0.35, 0.0)


wall_cases("robot", ROBOT_R)
wall_cases("ball", BALL_R)


# ------------------------------------------------------------------------------------ robot-robot
RR_AT = (F(0.25), F(0.25))


def rr_tie():
    """Robot j's (x, y) with d2 == 0.0064f from RR_AT, in the oracle's operation order, and the direction to it."""
    xi, yi = RR_AT
    for ux, uy in ((0.6, 0.8), (0.8, 0.6), (0.28, 0.96), (0.96, 0.28)):  # some directions have no tie at all
        for xj in near(xi + F(ux) * RR_DIST, 256):
            dx = xj - xi
            yjs = near(yi + F(uy) * RR_DIST, 1024)
            dy = yjs - yi
            hit = np.nonzero(dx * dx + dy * dy == RR_DIST2)[0]
            if hit.size:
                return (ux, uy), xj, yjs[hit[0]]
    raise AssertionError("no robot-robot tie")


def rr_cases():
    (ux, uy), xj, yj = rr_tie()
    for nm, dk in (("below", -1), ("at", 0), ("above", 1)):
        for vn, a in (("approaching", TINY_A), ("separating", -TINY_A), ("still", F(0))):
            def build(r, dk=dk, a=a):
                j = mate(r)
                f = Field()
                f.robot(r, *RR_AT, q=toward(ux, uy), act=(a, a))
                return f.robot(j, xj, ulps(yj, dk), q=toward(-ux, -uy), act=(a, a))
            add(f"rr/d2_{nm}_{vn}", ["rr_lt"], 2, f"robot pair, d2 {nm} 0.0064, {vn}")(build)

    @add("rr/coincident", ["rr_default", "rr_tiny"], 2, "coincident centres: d == 0, default normal (1, 0)")
    def _(r):
        return Field().robot(r, 0.25, 0.1).robot(mate(r), 0.25, 0.1)

    @add("rr/tiny_offset", ["rr_tiny"], 2, "centres 5e-10 apart along y: 0 < d <= 1e-9, default normal")
    def _(r):
        return Field().robot(r, 0.25, 0.0).robot(mate(r), 0.25, F(5e-10))

    @add("rr/denormal_offset", ["rr_tiny", "denormal"], 2, "centres one denormal apart: d2 underflows to 0")
    def _(r):
        return Field().robot(r, 0.25, 0.0).robot(mate(r), 0.25, F(1e-45))

    @add("rr/chain", ["dv", "dl"], 3, "three overlapping robots in a row: the later pair sees the earlier push-out")
    def _(r):
        f = Field()
        for i, j in enumerate(members(r, 3)):
            f.robot(j, 0.1 + 0.07 * i, 0.1 + 0.01 * i, act=(0.5 - 0.5 * i, 0.5 - 0.5 * i))
        return f

    @add("rr/chain_turned", ["dv", "dl"], 3, "a chain of turned robots with the third robot in the middle")
    def _(r):
        f = Field()
        for i, j in enumerate((r, third(r), mate(r))):
            f.robot(j, 0.1 + 0.065 * i, 0.1 - 0.02 * i, q=quat(0.4 * i), act=(0.8 - 0.8 * i, 0.6 - 0.6 * i))
        return f


rr_cases()


# ------------------------------------------------------------------------------------ ball-robot
BR_AT = (F(0.25), F(0.25))


def br_local(q, bx, by, at=BR_AT):
    c, s = heading(q)
    dx, dy = bx - at[0], by - at[1]
    return c * dx + s * dy, c * dy - s * dx


def br_d2(q, bx, by, at=BR_AT):
    lx, ly = br_local(q, bx, by, at)
    ex, ey = lx - np.clip(lx, -HALF, HALF), ly - np.clip(ly, -HALF, HALF)
    return ex * ex + ey * ey


def br_levels(q, lx, ly):
    """{"below", "at", "above"} -> ball (x, y) near the box-frame point (lx, ly) of the robot at BR_AT whose d2
    is the nearest below, exactly at, and the nearest above BALL_R2; "at" is missing where no float reaches it."""
    c, s = (float(v) for v in heading(q))
    x0, y0 = float(BR_AT[0]) + c * lx - s * ly, float(BR_AT[1]) + s * lx + c * ly
    bxs, bys = near(F(x0), 1024)[:, None], near(F(y0), 64)[None, :]
    d2 = br_d2(q, bxs, bys)
    pos = lambda ij: (bxs[ij[0], 0], bys[0, ij[1]])  # noqa: E731
    out = {"below": pos(np.unravel_index(np.argmax(np.where(d2 < BALL_R2, d2, F(0))), d2.shape)),
           "above": pos(np.unravel_index(np.argmin(np.where(d2 > BALL_R2, d2, F(1))), d2.shape))}
    hit = np.argwhere(d2 == BALL_R2)
    if hit.size:
        out["at"] = pos(hit[0])
    return out


def br_cases():
    e, rb = float(HALF) + float(BALL_R), float(BALL_R)
    # Box-frame spots and the normal there.  Against a face d2 = fl(ex ex) with ex on the 2^-28 lattice of
    # lx - 0.035f near 0.02134, 5 ulps of d2 a step, and no ex squares to BALL_R2: the face has no tie in
    # float32, only the nearest d2 on either side.  Off a corner d2 is a sum of two squares and ties exist,
    # though not in every direction.
    spots = {"face": [((e, 0.01), (1.0, 0.0))],
             "corner": [((float(HALF) + ux * rb, float(HALF) + uy * rb), (ux, uy))
                        for ux, uy in ((0.6, 0.8), (0.8, 0.6), (0.28, 0.96), (0.96, 0.28))]}
    for yn, q in YAWS.items():
        c, s = (float(v) for v in heading(q))
        for sn, tries in spots.items():
            levels, nl = next(((lv, nl) for lv, nl in ((br_levels(q, *p), nl) for p, nl in tries) if "at" in lv),
                              (br_levels(q, *tries[0][0]), tries[0][1]))
            assert sn == "face" or "at" in levels, (yn, sn)
            nw = (c * nl[0] - s * nl[1], s * nl[0] + c * nl[1])  # the normal in the world: the ball moves against it
            for nm, (x, y) in levels.items():
                add(f"br/{yn}/{sn}_d2_{nm}", ["br_lt"], 1, f"ball on a {sn} of the box, {yn}, d2 {nm} r2, approaching")(
                    lambda r, q=q, x=x, y=y, nw=nw: Field().robot(r, *BR_AT, q=q).ball(
                        x, y, -TINY_V * F(nw[0]), -TINY_V * F(nw[1])))

        @add(f"br/{yn}/centre", ["br_ly_ge0", "br_px_py"], 1, f"ball centre exactly at the robot's centre, {yn}")
        def _(r, q=q):
            return Field().robot(r, *BR_AT, q=q).ball(*BR_AT)

        for nm, (lx, ly) in (("px_lt_py", (0.02, 0.005)), ("px_lt_py_back", (-0.02, 0.005)), ("px_gt_py", (-0.004, -0.025))):
            @add(f"br/{yn}/inside_{nm}", [], 1, f"ball centre inside the box, {nm}, {yn}")
            def _(r, q=q, lx=lx, ly=ly, c=c, s=s):
                return Field().robot(r, *BR_AT, q=q).ball(float(BR_AT[0]) + c * lx - s * ly, float(BR_AT[1]) + s * lx + c * ly,
                                                          0.1, -0.05)

    # px == py needs lx == ly exactly: axis-aligned boxes, offsets of 2^-7 (exact sums on 0.25)
    for yn in ("yaw0", "yaw180"):
        for sg in (1, -1):
            @add(f"br/{yn}/inside_px_eq_py{'+-'[sg < 0]}", ["br_px_py"], 1, f"ball centre inside the box, px == py, {yn}")
            def _(r, q=YAWS[yn], sg=sg):
                d = F(sg * 2.0 ** -7)
                return Field().robot(r, *BR_AT, q=q).ball(BR_AT[0] + d, BR_AT[1] + d)

    @add("br/edge_yaw0", ["br_edge"], 1, "ball ahead of the face with ly == 0.035: the clamp's own limit, yaw 0")
    def _(r):
        return Field().robot(r, 0.25, 0.0).ball(0.25 + 0.05, HALF, -0.2, 0.0)

    @add("br/edge_yaw90", ["br_edge"], 1, "ball beside the box with |l| == 0.035 on the clamp's limit, yaw pi/2")
    def _(r):
        return Field().robot(r, 0.0, 0.25, q=YAWS["yaw90"]).ball(HALF, 0.25 + 0.05, 0.0, -0.2)

    @add("br/pinch_wall", ["dv", "dl"], 1, "ball pinched between a robot's face and the end wall")
    def _(r):
        return Field().robot(r, 0.68, 0.4, act=(1.0, 1.0), vx=0.5).ball(0.73, 0.405)

    @add("br/pinch_side_wall", ["dv", "dl"], 1, "ball pinched between a turned robot and the side wall")
    def _(r):
        return Field().robot(r, -0.2, 0.575, q=quat(1.2), act=(1.0, 0.7), vx=0.1, vy=0.4).ball(-0.19, 0.625)

    @add("br/two_robots", ["dv", "dl"], 2, "ball touching two robots in one substep")
    def _(r):
        f = Field().robot(r, 0.2, 0.1, act=(0.6, 0.6)).robot(mate(r), 0.31, 0.11, q=quat(2.8), act=(0.4, 0.5))
        return f.ball(0.255, 0.104, 0.05, 0.3)

    @add("br/two_robots_split", ["dv", "dl"], 2, "ball touching robots r and third(r)", split=True)
    def _(r):
        f = Field().robot(r, 0.2, 0.1, q=quat(0.3)).robot(third(r), 0.30, 0.12, q=quat(-2.0), act=(1.0, 1.0))
        return f.ball(0.25, 0.13, -0.3, -0.2)

    @add("br/denormal_under_centre", ["br_ly_ge0", "br_px_py", "denormal"], 1,
         "ball one denormal below the centre of a robot at the origin: ly = -1.4e-45 picks the -y face")
    def _(r):
        return Field().robot(r, 0.0, 0.0).ball(0.0, -F(1e-45))

    @add("br/denormal_over_centre", ["br_px_py", "denormal"], 1, "ball one denormal above the centre of a robot at the origin")
    def _(r):
        return Field().robot(r, 0.0, 0.0).ball(F(1e-45), F(1e-45))


br_cases()


# ------------------------------------------------------------------------------------ yaw step
def post_drive_w(w):
    """The yaw rate after one drive substep of a robot at rest with zero commands (heading (1, 0))."""
    wl, wr = F(0) - w * HALF_TRACK, F(0) + w * HALF_TRACK
    wl = wl + np.clip(F(0) - wl, -DV, DV)
    wr = wr + np.clip(F(0) - wr, -DV, DV)
    return (wr - wl) * INV_TRACK


def yaw_cases():
    def spin(name, tags, note, w):
        # every rate here brakes at the traction limit, so the drive's limit mutant sees these cases too
        add(f"yaw/{name}", list(tags) + ["dv"], 1, note)(lambda r, w=w: Field().robot(r, 0.25, 0.25, w=w))

    # w h/2 just below and at 0.78 in the first substep (the drive takes 4.44 rad/s off first)
    ws = near(F(0.78 / 0.0125 + 4.4444447), 4096)
    x = post_drive_w(ws) * HH
    at = ws[np.nonzero(x == F(0.78))[0][0]]
    below = ws[np.nonzero(x == ulps(0.78, -1))[0][0]]
    spin("x_at_078", ["sincos_078"], "w h/2 == 0.78f in the first substep: first value with range reduction", at)
    spin("x_below_078", ["sincos_078"], "w h/2 one ulp below 0.78f: last value of the plain polynomial", below)
    # k = 1 -> 2 boundary of the reduction: k = (int)(x 0.63661977 + 0.5)
    ws = near(F(2.3561945 / 0.0125 + 4.4444447), 4096)
    ws = np.sort(ws)
    k = (post_drive_w(ws) * HH * F(0.63661977) + F(0.5)).astype(np.int32)
    i = int(np.nonzero(k == 2)[0][0])
    assert k[i - 1] == 1
    spin("k1_last", ["sincos_k2"], "last w whose first substep reduces with k = 1", ws[i - 1])
    spin("k2_first", ["sincos_k2"], "first w whose first substep reduces with k = 2", ws[i])
    for w, what in ((45.0, "below 0.78 after the drive"), (70.0, "k = 1"), (120.0, "k = 1"), (186.0, "k = 1 then 1"),
                    (194.0, "k = 2 then 1 or 2"), (200.0, "k = 2"), (250.0, "k = 2"), (300.0, "k = 2"),
                    (330.0, "beyond: k = 3 takes the default arm"), (400.0, "beyond: k = 3")):
        spin(f"w{int(w)}", ["sincos_k2"] if w >= 190 else [], f"yaw rate {w} rad/s written into the state: {what}", F(w))


yaw_cases()


# ------------------------------------------------------------------------------------ drive
def drive_cases():
    tl = (F(0.5) * WHEEL[0]) * WHEEL[1]
    vs = near(tl - DV, 64)
    v_at = vs[np.nonzero(tl - vs == DV)[0][0]]
    for nm, v in (("at", v_at), ("over", ulps(v_at, -1)), ("under", ulps(v_at, 1)), ("far", F(0.0))):
        add(f"drive/wheel_err_{nm}", ["dv"], 1, f"wheel error {nm} +0.15 on both wheels (-0.15 in the reflections' twins)")(
            lambda r, v=v: Field().robot(r, 0.25, 0.25, vx=v, act=(0.5, 0.5)))
        add(f"drive/wheel_err_neg_{nm}", ["dv"], 1, f"wheel error {nm} -0.15 on both wheels")(
            lambda r, v=v: Field().robot(r, 0.25, 0.25, vx=-v, act=(-0.5, -0.5)))
    for nm, v in (("at", DL), ("over", ulps(DL, 1)), ("under", ulps(DL, -1)), ("far", F(0.4))):
        add(f"drive/slip_{nm}", ["dl"], 1, f"lateral slip {nm} 0.171675")(
            lambda r, v=v: Field().robot(r, 0.25, 0.25, vy=v))
        add(f"drive/slip_neg_{nm}", ["dl"], 1, f"lateral slip {nm} -0.171675")(
            lambda r, v=v: Field().robot(r, 0.25, 0.25, vy=-v))
    for nm, (l, rt) in (("at_clip", (1.0, -1.0)), ("ulp_outside", (ulps(1.0, 1), -ulps(1.0, 1))),
                        ("far_outside", (1.6, -7.0)), ("neg_zero", (-0.0, -0.0)), ("neg_zero_mixed", (-0.0, 0.3))):
        add(f"drive/action_{nm}", ["clip"], 1, f"wheel commands {nm} (clip 1.0)")(
            lambda r, l=l, rt=rt: Field().robot(r, 0.25, 0.25, act=(l, rt)))

    @add("drive/denormal_lateral", ["denormal"], 1, "a lateral velocity of 1e-40 (a denormal) through the slip clamp")
    def _(r):
        return Field().robot(r, 0.0, 0.25, vy=F(1e-40))

    @add("drive/denormal_forward", ["denormal"], 1, "a forward velocity of 1e-40 held by a wheel command of 1e-40")
    def _(r):
        return Field().robot(r, 0.0, 0.25, vx=F(1e-40), act=(F(1e-40), F(1e-40)))


drive_cases()


# ------------------------------------------------------------------------------------ goal, dones, time-outs
def goal_cases():
    def ball(name, tags, note, x, y, progress=0, max_len=MAX_LEN, v=(0.0, 0.0)):
        add(f"goal/{name}", tags, 0, note)(lambda r: Field().ball(x, y, *v).time(progress, max_len))

    ball("on_line", ["goal_gt"], "ball ending at |x| exactly 0.75 inside the mouth: no goal", HX, 0.05)
    ball("ulp_past_line", ["goal_gt"], "ball ending one ulp past 0.75: a goal (both goals through the reflections)",
         ulps(HX, 1), 0.05)
    ball("rolling_in", [], "ball rolling over the line in this step", 0.74, -0.1, v=(1.0, 0.2))
    ball("off_the_post", [], "ball rolling onto the goal-post corner at speed: a real impulse along the corner's normal",
         0.72, 0.19, v=(1.0, 0.3))
    ball("goal_at_len_minus_1", ["timeout_ge", "done_ge"], "goal on the step where progress reaches max_len - 1",
         ulps(HX, 1), 0.05, progress=MAX_LEN - 2)
    ball("goal_at_len", ["done_ge"], "goal on the step where progress reaches max_len", ulps(HX, 1), 0.05,
         progress=MAX_LEN - 1)
    ball("goal_at_len_minus_2", ["timeout_ge"], "goal one step earlier: done, not a time-out", ulps(HX, 1), 0.05,
         progress=MAX_LEN - 3)
    ball("no_goal_at_len_minus_1", ["done_ge"], "progress reaches max_len - 1 without a goal: the episode goes on",
         0.3, 0.05, progress=MAX_LEN - 2)
    ball("timeout", ["done_ge", "timeout_ge"], "progress reaches max_len without a goal: a time-out", 0.3, 0.05,
         progress=MAX_LEN - 1)
    for ml in (1, 2):
        for p in range(ml):
            ball(f"len{ml}_p{p}", ["done_ge", "timeout_ge"], f"max_len {ml}, progress {p}, no goal", 0.3, 0.05, p, ml)
            ball(f"len{ml}_p{p}_goal", ["done_ge", "timeout_ge"], f"max_len {ml}, progress {p}, goal", ulps(HX, 1), 0.05, p, ml)

    ball("denormal_velocity", ["denormal"], "ball velocity of 1e-40 from x == 0: the position becomes a denormal",
         0.0, 0.3, v=(F(1e-40), -F(1e-40)))


goal_cases()


# ------------------------------------------------------------------------------------ reset (injected uniforms)
SCALE_X, SCALE_Y = F(1.5) - F(0.14), F(1.3) - F(0.14)
MIN_DIST = F(0.07)
U24 = F(2.0 ** -24)
MAX_ROUNDS = 64


def spread_round(shift=0):
    """14 uniforms placing the seven bodies far apart; `shift` moves the whole round a little."""
    u = np.zeros((7, 2), F)
    for i in range(7):
        u[i] = (F(0.1) + F(0.125) * F(i) + F(shift) * F(2.0 ** -10), F(0.3) + F(0.05) * F(i % 2))
    return u


def colliding_round(shift):
    u = spread_round(shift)
    u[1] = u[0]  # robot 0 on the ball
    return u


def tail(yaws=(0.1, 0.2, 0.3, 0.4, 0.6, 0.7), vel=(0.25, 0.75)):
    return np.array(list(yaws) + list(vel), F)


def reset_tie():
    """(kx, ky): with the ball at u = (0.5, 0.5), i.e. at the origin, robot 0 drawn at u = 0.5 + k 2^-24 lies at a
    distance of exactly 0.07f, in the oracle's operation order; found on the 24-bit uniform grid."""
    kx = int(round(0.6 * 0.07 / float(SCALE_X) * 2 ** 24)) + np.arange(-256, 257)[:, None]
    ky = int(round(0.8 * 0.07 / float(SCALE_Y) * 2 ** 24)) + np.arange(-256, 257)[None, :]
    half = 2 ** 23
    px = ((kx + half).astype(F) * U24 - F(0.5)) * SCALE_X - F(0)
    py = ((ky + half).astype(F) * U24 - F(0.5)) * SCALE_Y - F(0)
    hit = np.argwhere(np.sqrt(px * px + py * py) == MIN_DIST)
    assert hit.size, "no reset tie"
    return int(kx[hit[0][0], 0]), int(ky[0, hit[0][1]])


@dataclass
class ResetCase:
    name: str
    tags: tuple
    row: np.ndarray   # the field's draws: 14 per round, then 6 yaws and 2 ball velocities
    note: str


def reset_cases() -> list[ResetCase]:
    out = []
    rounds = [colliding_round(i).ravel() for i in range(MAX_ROUNDS)]
    out.append(ResetCase("cap", ("reset_rounds",), np.concatenate(rounds + [tail()]),
                         "64 rounds that all collide: the cap is reached and the colliding placement is accepted"))
    out.append(ResetCase("all_but_last", ("reset_rounds",), np.concatenate(rounds[:-1] + [spread_round(99).ravel(), tail()]),
                         "63 colliding rounds, the 64th is free"))
    out.append(ResetCase("five_rounds", (), np.concatenate(rounds[:4] + [spread_round(7).ravel(), tail()]),
                         "a collision on every round but the last, five rounds"))
    kx, ky = reset_tie()
    for nm, d in (("at", 0), ("closer", -1), ("farther", 1)):
        u = spread_round()
        u[:, 1] += F(0.4)  # the robots 1..5 on a far row; the ball and robot 0 below
        u[0] = (F(0.5), F(0.5))
        u[1] = (F(2 ** 23 + kx + d) * U24, F(2 ** 23 + ky + d) * U24)
        # a second, free round follows: consumed only if this one is rejected
        out.append(ResetCase(f"pair_{nm}_007", ("reset_lt",) if nm == "at" else (),
                             np.concatenate([u.ravel(), spread_round(3).ravel(), tail()]),
                             f"ball and robot 0 {nm} than / exactly 0.07 apart on the 24-bit uniform grid"))
    out.append(ResetCase("yaw_draws", ("reset_yaw",),
                         np.concatenate([spread_round(1).ravel(), tail(yaws=(0.0, 0.5, 1.0 - 2.0 ** -24, 2.0 ** -24, 0.25, 0.75),
                                                                        vel=(0.0, 1.0 - 2.0 ** -24))]),
                         "yaw draws u = 0, 0.5, 1 - 2^-24 (half-angles -pi/2, 0, pi/2) and the ball velocity's ends"))
    return out
