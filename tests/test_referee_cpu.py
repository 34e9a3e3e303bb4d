"""The referee without a GPU (include/vss.h, vss_amd/referee.py): the unit's part of the one header, library
and source stamp, the entry's argument checks on addresses that are never
dereferenced, the parameter and table rules, the float32 specification `reference_referee` on hand-built states -- each
counter at its threshold, the precedence, max_stops, a done field, the >= 0 sides, the other goal's area -- its placement
tied to `reference_setplay` bit for bit, and the flags' plumbing."""
import argparse
import ctypes
import math
import os
import re
import shutil

import numpy as np
import pytest

from test_setplay_cpu import exported, fresh, same_bits, stale_copy_is_refused
from vss_amd import _native as N
from vss_amd import checkpoint as CK
from vss_amd import cheader
from vss_amd import referee as R
from vss_amd import setplay as S

F32 = np.float32
FAKE = 1 << 20  # non-null, 16-B aligned, never dereferenced: every call below returns before a launch
GAP = 1 << 24   # between two fake buffers: further apart than any extent used here
E_ARG, OK = 1, 0
ROW = 52 * 4
ON = R.Params.of(stall_steps=3, area_steps=2)
PARKED = ((-0.30, 0.55), (-0.20, 0.55), (-0.10, 0.55), (0.10, 0.55), (0.20, 0.55), (0.30, 0.55))  # in no area, off the marks


def call(n_fields=64, tab=None, prm=None, done=FAKE, done_stride=1, state=FAKE + GAP, dof=FAKE + 6 * GAP,
         counters=FAKE + 7 * GAP, views=((FAKE + 2 * GAP, 3, 0, 3, 1, 0),), counts=FAKE + 4 * GAP, verdict=FAKE + 5 * GAP,
         null_tab=False, null_prm=False, n_views=None, null_views=False):
    tab = R.RefTable().c_table() if tab is None else tab
    prm = ON.c_params() if prm is None else prm
    arr = (R.VssRefereeView * 2)()
    for i, v in enumerate(views):
        arr[i] = R.VssRefereeView(*v)
    nv = len(views) if n_views is None else n_views
    return R.load().vss_referee(None, n_fields, None if null_tab else ctypes.byref(tab), None if null_prm else ctypes.byref(prm),
                                7, 3, done, done_stride, state, dof, counters, nv, None if null_views else arr, counts, verdict)


# ---- the referee's part of the one ABI and the one library -------------------------------------------------------------
def test_the_header_parses_and_the_library_exports_exactly_its_functions():
    with open(N.HEADER) as f:
        h = cheader.parse(f.read())
    assert [name for name in h.functions if "referee" in name] == ["vss_referee"] and "vss_referee" in N.EXPORTED
    assert sorted(name for name in h.structs if "referee" in name) == ["vss_referee_params", "vss_referee_play", "vss_referee_table"]
    assert {k: v for k, v in h.constants.items() if "REFEREE" in k} == {"VSS_REFEREE_PLAYS": 3, "VSS_REFEREE_CODES": 8}
    assert R.CODES == 8 == N.REFEREE_CODES
    assert (R.VssRefereePlay, R.VssRefereeTable, R.VssRefereeParams) == (N.VssRefereePlay, N.VssRefereeTable, N.VssRefereeParams)
    assert R.VssRefereeView is S.VssSetplayView and R.VssRefereeEntity is S.VssSetplayEntity  # one struct each in the header
    assert ctypes.sizeof(R.VssRefereeEntity) == 20 and ctypes.sizeof(R.VssRefereePlay) == 152
    assert ctypes.sizeof(R.VssRefereeTable) == 456 and ctypes.sizeof(R.VssRefereeParams) == 24
    assert ctypes.sizeof(R.VssRefereeView) == 40
    assert [ctypes.sizeof(h.structs["vss_referee_" + n]) for n in ("play", "table", "params")] == [152, 456, 24]
    assert N.load().vss_referee.argtypes == h.functions["vss_referee"][1]
    if shutil.which("nm"):
        assert exported(N.LIB_PATH, "vss_referee") == ["vss_referee"]
        assert exported(N.LIB_PATH, "vss_") == sorted(h.functions)


def test_the_unit_is_one_of_the_core_librarys_and_nothing_is_packaged_beside_it():
    assert [os.path.basename(p) for p in N.STAMPED].count("vss_referee.hip") == 1
    assert os.path.join(N.CSRC, "vss_referee.hip") in N.STAMPED and os.path.join(N.CSRC, "vss_placement.h") in N.STAMPED
    assert [os.path.join(d, f) for d, _, files in os.walk(N.CSRC) for f in files if f == "Makefile" or f.endswith(".mk")] \
        == [os.path.join(N.CSRC, "Makefile")]
    for name in ("LIB_PATH", "STAMPED", "CSRC", "HEADER", "ABI", "EXPORTED", "ABI_VERSION", "source_hash", "verify_source_hash"):
        assert not hasattr(R, name), name
    assert R.load is N.load  # the module's own name for the one loader
    assert not os.path.exists(os.path.join(os.path.dirname(N.HEADER), "vss_referee.h"))
    assert [d for d in os.listdir(os.path.dirname(N.CSRC)) if d.startswith("csrc")] == ["csrc"]  # no unit beside the core


def test_the_stamp_covers_the_units_sources_and_a_stale_library_is_refused(tmp_path, monkeypatch):
    stale_copy_is_refused("vss_referee.hip", "STEP_FLAGS", tmp_path, monkeypatch)


# ---- the entry's refusals ----------------------------------------------------------------------------------------------
def test_zero_size_and_good_calls_that_stop_before_a_launch():
    assert call(n_fields=0) == OK
    assert call(n_fields=0, done=None) == OK               # no field is done
    assert call(n_fields=0, done=None, done_stride=0) == OK
    assert call(n_fields=0, views=(), counts=None, verdict=None) == OK
    assert call(n_fields=0, views=(), null_views=True) == OK
    assert call(n_fields=0, views=((FAKE + 2 * GAP, 6, 3, 3, 2, 0),)) == OK
    assert call(n_fields=0, views=((FAKE + 2 * GAP, 1, 0, 1, 1, 0), (FAKE + 3 * GAP, 3, 0, 3, 1, 1))) == OK
    assert call(n_fields=0, prm=R.Params().c_params()) == OK  # every call switched off is still a good call


def test_null_pointers_view_shapes_alignment_and_sizes_are_refused():
    for n in (64, 0):
        assert call(n_fields=n, null_tab=True) == E_ARG and call(n_fields=n, null_prm=True) == E_ARG
        assert call(n_fields=n, state=None) == E_ARG and call(n_fields=n, dof=None) == E_ARG
        assert call(n_fields=n, counters=None) == E_ARG
        assert call(n_fields=n, null_views=True) == E_ARG
        assert call(n_fields=n, n_views=3) == E_ARG and call(n_fields=n, n_views=-1) == E_ARG
        assert call(n_fields=n, views=((0, 3, 0, 3, 1, 0),)) == E_ARG
        for bad in ((3, 0, 2, 1, 0), (3, 0, 0, 1, 0), (3, 0, 3, 0, 0), (3, 0, 3, 3, 0), (3, 0, 3, 1, 2), (3, 0, 3, 1, -1),
                    (6, 3, 3, 2, 1), (2, 0, 3, 1, 0), (0, 0, 1, 1, 0), (-1, 0, 1, 1, 0)):
            assert call(n_fields=n, views=((FAKE + 2 * GAP,) + bad,)) == E_ARG, bad
    for off in range(1, 16):
        assert call(views=((FAKE + 2 * GAP + off, 3, 0, 3, 1, 0),)) == E_ARG
        assert call(dof=FAKE + 6 * GAP + off) == E_ARG and call(counters=FAKE + 7 * GAP + off) == E_ARG
        if off % 8:
            assert call(done=FAKE + off) == E_ARG and call(counts=FAKE + 4 * GAP + off) == E_ARG
        if off % 4:
            assert call(state=FAKE + GAP + off) == E_ARG and call(verdict=FAKE + 5 * GAP + off) == E_ARG
    assert call(done_stride=0) == E_ARG and call(done_stride=-1) == E_ARG
    for n in (-1, -2 ** 63, 2 ** 63 - 1, 1 << 60, (1 << 31) * 300):
        assert call(n_fields=n) == E_ARG
    assert call(views=((FAKE + 2 * GAP, 2 ** 63 - 1, 0, 3, 1, 0),)) == E_ARG
    assert call(done_stride=2 ** 63 - 1) == E_ARG
    # two teams: a team stride below a block's span, or past the addressable rows
    for ts in (64 * 3 - 1, 0, -192, 1 << 62):
        assert call(views=((FAKE + 2 * GAP, 3, ts, 3, 2, 0),)) == E_ARG
    # ... or both teams inside one field stride, as FULL's (N, 2, 3, 52): they must not overlap there either
    for fs, ts in ((6, 2), (6, 4), (5, 3), (8, 6)):
        assert call(views=((FAKE + 2 * GAP, fs, ts, 3, 2, 0),)) == E_ARG
    assert call(n_fields=0, views=((FAKE + 2 * GAP, 8, 5, 3, 2, 0),)) == OK


def test_overlapping_buffers_are_refused():
    rows, state, dof, cnt = FAKE + 2 * GAP, FAKE + GAP, FAKE + 6 * GAP, FAKE + 7 * GAP
    assert call(state=rows) == E_ARG and call(state=rows + 191 * ROW) == E_ARG      # state on the rows
    assert call(state=rows - (64 * 58 * 4 - 4)) == E_ARG
    assert call(verdict=rows + 16) == E_ARG and call(counts=rows + 8) == E_ARG
    assert call(verdict=state + 4) == E_ARG and call(counts=state + 64 * 58 * 4 - 8) == E_ARG
    assert call(dof=state + 16) == E_ARG and call(dof=rows - (64 * 48 - 16)) == E_ARG and call(dof=cnt + 64 * 16 - 16) == E_ARG
    assert call(counters=state + 64 * 58 * 4 - 16) == E_ARG and call(counters=rows + 16) == E_ARG
    assert call(counters=dof + 64 * 48 - 16) == E_ARG and call(verdict=dof + 4) == E_ARG and call(counts=cnt + 8) == E_ARG
    assert call(verdict=cnt + 64 * 16 - 4) == E_ARG and call(verdict=FAKE + 4 * GAP + 60) == E_ARG
    for out in ("state", "dof", "counters", "counts", "verdict"):                   # an output on done
        assert call(**{out: FAKE + 16}) == E_ARG, out
    assert call(done=rows + 8) == E_ARG and call(done=dof + 8) == E_ARG and call(done=cnt + 8) == E_ARG
    assert call(views=((rows, 1, 0, 1, 1, 0), (rows + 63 * ROW, 3, 0, 3, 1, 1))) == E_ARG
    assert call(views=((rows, 1, 0, 1, 1, 0), (rows, 3, 0, 3, 1, 1))) == E_ARG
    for out in ("state", "dof", "counters", "counts", "verdict"):                   # equality at any size
        assert call(n_fields=0, **{out: rows}) == E_ARG and call(n_fields=0, **{out: FAKE}) == E_ARG, out
    assert call(n_fields=0, dof=cnt) == E_ARG and call(n_fields=0, counts=FAKE + 5 * GAP) == E_ARG


def bad_params():
    def edit(**kw):
        p = ON.c_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    return [(k, edit(**{k: v})) for k, v in (
        ("stall_steps", -1), ("area_steps", -1), ("max_stops", -1), ("stall_steps", -2 ** 31), ("stall_speed_sq", -0.01),
        ("stall_speed_sq", math.nan), ("stall_speed_sq", math.inf), ("area_x", 0.0), ("area_x", -0.6), ("area_x", 0.75),
        ("area_x", math.nan), ("area_x", math.inf), ("area_y", 0.0), ("area_y", -0.35), ("area_y", 0.66), ("area_y", math.nan))]


def bad_tables():
    """(what, a table the entry must refuse): one per rule, on the raw struct."""
    def edit(fn):
        t = R.RefTable().c_table()
        fn(t)
        return t
    return [("x inf", edit(lambda t: setattr(t.play[0].e[2], "x", math.inf))),
            ("yaw nan", edit(lambda t: setattr(t.play[1].e[2], "yaw", math.nan))),
            ("ball velocity nan", edit(lambda t: setattr(t.play[2], "ball_vx", math.nan))),
            ("r_vel < 0", edit(lambda t: setattr(t.play[0], "r_vel", -1.0))),
            ("r_vel inf", edit(lambda t: setattr(t.play[0], "r_vel", math.inf))),
            ("yaw > pi", edit(lambda t: setattr(t.play[0].e[1], "yaw", 3.2))),
            ("r_yaw > pi", edit(lambda t: setattr(t.play[1].e[1], "r_yaw", 3.2))),
            ("r_yaw < 0", edit(lambda t: setattr(t.play[2].e[1], "r_yaw", -0.1))),
            ("r_pos < 0", edit(lambda t: setattr(t.play[0].e[1], "r_pos", -0.01))),
            ("robot past x", edit(lambda t: setattr(t.play[1].e[6], "x", 0.70))),       # 0.70 + 0.02 > 0.71
            ("robot past y", edit(lambda t: setattr(t.play[1].e[2], "y", 0.59))),       # 0.59 + 0.03 > 0.61
            ("ball past the line", edit(lambda t: setattr(t.play[2].e[0], "x", -0.76))),
            ("a pair too close", edit(lambda t: setattr(t.play[1].e[1], "x", 0.30))),   # 0.075 from the ball
            # the area rule alone: every other rule holds for these three
            ("a free ball in an area", edit(lambda t: (setattr(t.play[0].e[0], "x", 0.62), setattr(t.play[0].e[0], "y", 0.30)))),
            ("a free ball that can reach an area", edit(lambda t: (setattr(t.play[0].e[0], "r_pos", 0.05),
                                                                   setattr(t.play[0].e[0], "x", 0.56),
                                                                   setattr(t.play[0].e[0], "y", 0.20)))),
            ("a penalty in an area", edit(lambda t: (setattr(t.play[1].e[0], "x", 0.61), setattr(t.play[1].e[0], "y", 0.20))))]


def test_every_parameter_and_table_rule_is_refused_before_a_launch():
    for what, prm in bad_params():
        assert call(prm=prm) == E_ARG and call(n_fields=0, prm=prm) == E_ARG, what
    for what, tab in bad_tables():
        assert call(tab=tab) == E_ARG and call(n_fields=0, tab=tab) == E_ARG, what
    # the rules that do not exist here: a goal kick's ball stands on the area's line
    assert call(n_fields=0, prm=R.Params.of(stall_steps=1, area_depth=0.20).c_params()) == OK


def test_validate_in_python_raises_for_the_same_rules():
    for kw in (dict(stall_steps=-1), dict(area_steps=-1), dict(max_stops=-1), dict(stall_speed=math.nan),
               dict(stall_speed=math.inf), dict(area_depth=0.0), dict(area_depth=0.75), dict(area_depth=-0.1),
               dict(area_width=0.0), dict(area_width=1.32), dict(area_width=math.nan)):
        with pytest.raises(ValueError, match="referee"):
            R.Params.of(**kw)
    with pytest.raises(ValueError, match="stall_speed_sq"):
        R.Params(stall_speed_sq=-1.0).validate()
    assert R.Params.of(area_width=1.30).area_y == 0.65 and R.Params().validate() == R.Params()
    for what, prm in bad_params():  # the C rules and the Python rules are the same rules
        with pytest.raises(ValueError):
            R.Params(prm.stall_speed_sq, prm.area_x, prm.area_y, prm.stall_steps, prm.area_steps, prm.max_stops).validate()
    fb, pen = S.BUILTIN["free_ball"], S.BUILTIN["penalty"]

    def ent(p, e, **kw):
        rows = [list(r) for r in p.entities]
        for name, v in kw.items():
            rows[e][("x", "y", "yaw", "r_pos", "r_yaw").index(name)] = v
        return p._replace(entities=tuple(tuple(r) for r in rows))
    for plays in ((ent(fb, 2, x=math.inf),), (ent(fb, 1, yaw=3.2),), (ent(fb, 1, r_pos=-0.01),), (None, ent(pen, 6, x=0.70)),
                  (None, ent(pen, 1, x=0.30)), (fb._replace(ball_vel=(0, 0, -1.0)),), (None, None, ent(fb, 0, x=0.76))):
        with pytest.raises(ValueError):
            R.RefTable(*plays)
    with pytest.raises(ValueError, match="whistled again"):
        R.RefTable(ent(fb, 0, x=0.62, y=0.30))
    with pytest.raises(ValueError, match="whistled again"):
        R.RefTable(ent(fb, 0, x=0.56, y=0.20, r_pos=0.05))   # the anchor is outside, the jitter reaches in
    R.RefTable(ent(fb, 0, x=0.54, y=0.20, r_pos=0.05))
    with pytest.raises(ValueError, match="whistled again"):
        R.RefTable(None, ent(pen, 0, x=0.61, y=0.20))
    with pytest.raises(ValueError, match="whistled again"):
        R.RefTable().validate(R.Params.of(stall_steps=1, area_depth=0.40, area_width=1.0))  # the free-ball mark in a huge area
    tab = R.RefTable()
    assert [p.name for p in tab.plays] == list(R.PLAYS) and tab.validate(ON) is tab
    assert all(tab.plays[k] == S.BUILTIN[name] for k, name in enumerate(R.PLAYS))  # the built-ins are the defaults


# ---- the specification on hand-built states ---------------------------------------------------------------------------
def scene(code, n=1):
    """A state (58, n) in which only verdict `code` can hold: the robots parked, then per code the ball at rest in its
    quadrant (0..3), or moving inside a goal area with two defenders (4, 5) or two attackers (6, 7) standing there."""
    st = fresh(n)
    for r, (x, y) in enumerate(PARKED):
        st[N.CH_RX + r], st[N.CH_RY + r] = x, y
    if code < 4:
        st[0], st[1] = (-0.30 if code & 2 else 0.30), (-0.20 if code & 1 else 0.20)
        return st
    left = code in (5, 6)
    blue = code in (5, 7)       # 5: blue defends its own area; 7: blue crowds yellow's
    sx = -1.0 if left else 1.0
    st[0], st[1], st[2] = sx * 0.70, 0.05, 1.0
    for r, y in zip((0, 1) if blue else (3, 4), (0.20, -0.20)):
        st[N.CH_RX + r], st[N.CH_RY + r] = sx * 0.66, y
    return st


def run(st, counters, prm=ON, done=None, table=None, seed=5, call=0, views=()):
    n = st.shape[1]
    cnt = np.broadcast_to(np.asarray(counters, np.int32), (n, 4)).copy()
    dof, counts, verdict = np.ones((n, 2, 3, 2), F32), np.zeros(8, np.int64), np.full(n, 9, np.int32)
    f = R.reference_referee(R.RefTable() if table is None else table, prm, seed, call, done, st, dof, cnt, views, counts, verdict)
    return f, cnt, dof, counts, verdict


@pytest.mark.parametrize("code", range(8))
def test_each_counter_at_steps_minus_one_gives_its_call_or_goes_to_zero(code):
    which = 0 if code < 4 else (1 if code < 6 else 2)
    at = [0, 0, 0, 0]
    at[which] = (ON.stall_steps if which == 0 else ON.area_steps) - 1
    st = scene(code)
    before = st.copy()
    f, cnt, dof, counts, verdict = run(st, at)
    assert f.tolist() == [0] and verdict.tolist() == [code] and counts.tolist() == [int(k == code) for k in range(8)]
    assert cnt.tolist() == [[0, 0, 0, 1]] and same_bits(dof, np.zeros_like(dof)) and not same_bits(st, before)
    play = R.RefTable().plays[which]
    ax, ay = play.entities[0][0], play.entities[0][1]
    want = (-ax if code in (2, 3, 5, 7) else ax, -ay if code in (1, 3) else ay)  # flip_x, flip_y (the scenes' kicks: by > 0)
    assert same_bits(st[0:2, 0], want)  # the ball's radius is 0: it sits at the mirrored anchor
    assert same_bits(st[N.CH_RVX:N.CH_RW + 6], np.zeros((18, 1), F32))
    # one step short: no call, the counter counts on
    at[which] -= 1 if at[which] else 0
    if at[which] + 1 < (ON.stall_steps if which == 0 else ON.area_steps):
        st = scene(code)
        f, cnt, dof, _, verdict = run(st, at)
        assert f.size == 0 and verdict.tolist() == [-1] and cnt[0, which] == at[which] + 1 and same_bits(st, scene(code))
        assert same_bits(dof, np.ones_like(dof))
    # the condition false: the counter goes to 0 whatever it held
    st = scene(code)
    if which == 0:
        st[2] = 0.06   # above the 0.05 m/s threshold
    else:
        st[N.CH_RY + (0 if code in (5, 7) else 3)] = 0.36  # one of the two leaves the area
    f, cnt, _, counts, verdict = run(st, [50, 50, 50, 0] if which else [50, 0, 0, 0])
    assert f.size == 0 and verdict.tolist() == [-1] and counts.sum() == 0 and cnt[0, which] == 0


def test_two_step_stall_is_not_yet_a_free_ball_and_the_counters_cap():
    st = scene(0)
    f, cnt, *_ = run(st, [1, 0, 0, 0])
    assert f.size == 0 and cnt.tolist() == [[2, 0, 0, 0]]
    f, cnt, *_ = run(st, cnt[0])
    assert f.tolist() == [0] and cnt.tolist() == [[0, 0, 0, 1]]
    off = R.Params.of()                        # every call switched off: the counters still count, to the cap
    _, cnt, *_ = run(scene(0), [R.CAP - 1, 0, 0, 7], prm=off)
    assert cnt.tolist() == [[R.CAP, 0, 0, 7]]
    _, cnt, *_ = run(scene(0), [R.CAP, 0, 0, 7], prm=off)
    assert cnt.tolist() == [[R.CAP, 0, 0, 7]]
    st = scene(5)
    st[2] = 0.0                                # at rest in the area with two defenders: all three conditions
    _, cnt, _, _, verdict = run(st, [R.CAP, R.CAP, 5, 0], prm=off)
    assert cnt.tolist() == [[R.CAP, R.CAP, 0, 0]] and verdict.tolist() == [-1]


def test_the_precedence_is_penalty_then_goal_kick_then_free_ball():
    st = scene(5)
    st[2] = 0.0
    for r, y in ((3, 0.10), (4, -0.10)):       # two attackers join the two defenders, the ball at rest
        st[N.CH_RX + r], st[N.CH_RY + r] = -0.64, y
    assert run(st.copy(), [9, 9, 9, 0])[4].tolist() == [5]
    assert run(st.copy(), [9, 0, 9, 0])[4].tolist() == [6]         # defend one short of 2: the goal kick
    assert run(st.copy(), [9, 0, 0, 0])[4].tolist() == [2]         # both short: the free ball of (bx < 0, by >= 0)
    assert run(st.copy(), [9, 9, 9, 0], prm=R.Params.of(stall_steps=3))[4].tolist() == [2]  # the area calls off
    assert run(st.copy(), [9, 9, 9, 0], prm=R.Params.of(area_steps=2))[4].tolist() == [5]
    assert run(st.copy(), [9, 0, 0, 0], prm=R.Params.of(area_steps=2))[4].tolist() == [-1]  # the free ball off


def test_max_stops_suppresses_the_call_while_the_counters_keep_counting():
    prm = R.Params.of(stall_steps=3, area_steps=2, max_stops=2)
    st = scene(0)
    f, cnt, *_ = run(st, [2, 0, 0, 1], prm=prm)
    assert f.tolist() == [0] and cnt.tolist() == [[0, 0, 0, 2]]
    st = scene(0)
    f, cnt, dof, counts, verdict = run(st, [2, 0, 0, 2], prm=prm)
    assert f.size == 0 and cnt.tolist() == [[3, 0, 0, 2]] and verdict.tolist() == [-1] and counts.sum() == 0
    assert same_bits(st, scene(0)) and same_bits(dof, np.ones_like(dof))
    f, cnt, *_ = run(scene(5), [0, 7, 0, 5], prm=prm)
    assert f.size == 0 and cnt.tolist() == [[0, 8, 0, 5]]


def test_a_done_field_zeroes_its_counters_and_is_never_placed():
    st = np.concatenate([scene(0), scene(5), scene(0), scene(6)], axis=1)
    before = st.copy()
    done = np.array([1, 1, 0, 0])
    f, cnt, dof, counts, verdict = run(st, [9, 9, 9, 3], done=done)
    assert f.tolist() == [2, 3] and verdict.tolist() == [-1, -1, 0, 6] and counts.tolist() == [1, 0, 0, 0, 0, 0, 1, 0]
    assert cnt.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 4], [0, 0, 0, 4]]
    assert same_bits(st[:, :2], before[:, :2]) and same_bits(dof[:2], np.ones_like(dof[:2])) and same_bits(dof[2:], 0 * dof[2:])


def test_zero_takes_the_side_of_the_positive_numbers():
    for bx, by, code in ((0.0, 0.0, 0), (-0.0, -0.0, 0), (0.0, -0.2, 1), (-0.3, 0.0, 2), (-0.3, -0.0, 2)):
        st = scene(0)
        st[0], st[1] = bx, by
        assert run(st, [2, 0, 0, 0])[4].tolist() == [code], (bx, by)


def test_a_robot_in_the_other_goals_area_and_one_on_the_line_do_not_count():
    st = scene(5)                     # the ball in blue's area (x < 0), blue 0 and 1 inside
    st[N.CH_RX + 1] = 0.66            # blue 1 stands in yellow's area instead
    assert run(st.copy(), [0, 1, 1, 0])[1].tolist() == [[0, 0, 0, 0]]
    st = scene(5)
    st[N.CH_RX + 1] = -F32(0.6)       # on the line: |x| > area_x is false
    assert run(st.copy(), [0, 1, 1, 0])[1].tolist() == [[0, 0, 0, 0]]
    st = scene(5)
    st[N.CH_RY + 1] = F32(0.35)       # |y| < area_y is false
    assert run(st.copy(), [0, 1, 1, 0])[1].tolist() == [[0, 0, 0, 0]]
    st = scene(5)
    st[1] = 0.40                      # the ball beside the area: nobody's standing there counts
    assert run(st.copy(), [0, 1, 1, 0])[1].tolist() == [[0, 0, 0, 0]]
    st = scene(5)
    st[N.CH_RX + 2], st[N.CH_RY + 2] = -0.70, 0.0   # a third defender changes nothing; yellow's three far away count as 0
    assert run(st.copy(), [0, 1, 1, 0])[4].tolist() == [5]


def rigid(play):
    """The play with every jitter radius 0."""
    return play._replace(entities=tuple((x, y, yaw, 0.0, 0.0) for x, y, yaw, _, _ in play.entities),
                         ball_vel=(play.ball_vel[0], play.ball_vel[1], 0.0))


@pytest.mark.parametrize("code", range(8))
def test_without_jitter_the_placed_state_is_reference_setplays_with_the_flips_forced(code):
    """Ties the referee's placement to the set plays' placement bit for bit."""
    plays = [rigid(S.BUILTIN[name]) for name in R.PLAYS]
    plays[1] = plays[1]._replace(ball_vel=(0.25, -0.5, 0.0))  # a velocity, so that its two negations show
    n = 3
    st = scene(code, n)
    if code >= 6:
        st[1, 1] = -0.05  # a goal kick from the -y half
    f, cnt, dof, counts, verdict = run(st, [9, 9, 9, 0], table=R.RefTable(*plays))
    assert f.tolist() == [0, 1, 2] and (verdict == code).all()
    which = 0 if code < 4 else (1 if code < 6 else 2)
    for i in range(n):
        flip_x = code in (2, 3, 5, 7)
        flip_y = code in (1, 3) or (code >= 6 and i == 1)
        want = fresh(n)
        table = S.Table([p._replace(p_flip_x=float(flip_x), p_flip_y=float(flip_y)) for p in plays], 0.5).only(which)
        S.reference_setplay(table, 77, 1, None, want)
        assert same_bits(st[:, i], want[:, i]), (code, i)


def test_the_written_rows_are_the_full_rows_of_the_written_state():
    n = 64
    st = np.concatenate([scene(c, 8) for c in range(8)], axis=1)
    g = np.random.default_rng(3)
    st[N.CH_RVX:] = g.standard_normal((18, n)).astype(F32)      # the robots were moving
    full, sa, opp = g.standard_normal((n * 6, 52)).astype(F32), np.zeros((n, 52), F32), np.zeros((n * 3, 52), F32)
    before = full.copy()
    done = (np.arange(n) % 8 == 7).astype(np.int64)
    f, cnt, dof, counts, verdict = run(st, [9, 9, 9, 0], done=done, views=[(full, R.view_full())], seed=11, call=4)
    assert f.size == 56 and counts.tolist() == [7] * 8
    assert same_bits(full.reshape(n, 2, 3, 52)[f], S.full_rows_of_state(st, f))
    rest = np.setdiff1d(np.arange(n), f)
    assert same_bits(full.reshape(n, 6, 52)[rest], before.reshape(n, 6, 52)[rest])
    own = full.reshape(n, 2, 3, 52)[f][..., [11, 12, 20, 21, 29, 30]]
    assert same_bits(own, np.zeros_like(own))  # the own-action floats are +0.0, for yellow too
    # the smaller views are slices of FULL; another call index draws another jitter, the same one the same
    st2 = np.concatenate([scene(c, 8) for c in range(8)], axis=1)
    run(st2, [9, 9, 9, 0], done=done, views=[(sa, R.view_sa()), (opp, R.view_opponent())], seed=11, call=4)
    assert same_bits(st2[:N.CH_RVX], st[:N.CH_RVX]) and same_bits(sa[f], full.reshape(n, 2, 3, 52)[f, 0, 0])
    assert same_bits(opp.reshape(n, 3, 52)[f], full.reshape(n, 2, 3, 52)[f, 1])
    st3 = np.concatenate([scene(c, 8) for c in range(8)], axis=1)
    run(st3, [9, 9, 9, 0], done=done, seed=11, call=5)
    assert not same_bits(st3[N.CH_RX], st2[N.CH_RX])
    # ten thousand restarts of every kind keep clear of each other and are never whistled again at once
    m = 10000
    for code in range(8):
        big = scene(code, m)
        f, cnt, *_ = run(big, [9, 9, 9, 0], seed=2026, call=code)
        assert f.size == m
        pos = np.stack([np.concatenate([big[0:1], big[N.CH_RX:N.CH_RX + 6]]), np.concatenate([big[1:2], big[N.CH_RY:N.CH_RY + 6]])], -1)
        d = np.linalg.norm(pos[:, None].astype(np.float64) - pos[None, :].astype(np.float64), axis=-1)
        d[np.arange(7), np.arange(7)] = 9.0
        assert d.min() >= 0.08
        f2, cnt2, *_ = run(big, cnt, prm=R.Params.of(stall_steps=2, area_steps=1))
        assert f2.size == 0 and (cnt2[:, 1:3] == 0).all(), code  # nobody stands in an area with the ball after a restart


# ---- flags and resume --------------------------------------------------------------------------------------------------
def parse(argv):
    return CK.add_channel_arguments(argparse.ArgumentParser()).parse_args(argv)


def test_flags_defaults_and_what_they_build(tmp_path):
    args = parse([])
    assert [getattr(args, k) for k in CK.REFEREE_STRUCTURAL] == [0, 0.05, 0, 0.15, 0.70, 0] == list(CK.REFEREE_DEFAULTS.values())
    assert R.params_of_args(args) is None and R.params_of_args(argparse.Namespace()) is None
    assert R.params_of_args(parse(["--ref-stall-speed", "0.1", "--ref-max-stops", "3"])) is None  # neither call is on
    p = R.params_of_args(parse(["--ref-stall-steps", "100"]))
    assert p == R.Params(float(F32(0.05) * F32(0.05)), 0.60, 0.35, 100, 0, 0) and p.any()
    p = R.params_of_args(parse(["--ref-area-steps", "20", "--ref-area-depth", "0.2", "--ref-area-width", "0.5",
                                "--ref-stall-speed", "0.1", "--ref-max-stops", "4"]))
    assert p == R.Params(float(F32(0.1) * F32(0.1)), 0.75 - 0.2, 0.25, 0, 20, 4)
    for bad in (["--ref-stall-steps", "-1"], ["--ref-area-steps", "-5"], ["--ref-stall-steps", "5", "--ref-max-stops", "-1"],
                ["--ref-area-steps", "5", "--ref-area-depth", "0.8"], ["--ref-area-steps", "5", "--ref-area-width", "1.4"]):
        with pytest.raises(ValueError):
            R.params_of_args(parse(bad))
    assert R.referee_seed(3) != R.referee_seed(3, 1) != R.referee_seed(4) and 0 <= R.referee_seed(2 ** 40) < 2 ** 64
    assert len({R.referee_seed(3), S.setplay_seed(3)}) == 2
    # --setplay-file supplies the three plays by name
    import json
    own = S.BUILTIN["penalty"]._replace(entities=((.30, 0, 0, 0, 0),) + S.BUILTIN["penalty"].entities[1:])
    own = own._replace(entities=own.entities[:1] + ((.20, 0, 0, .01, .3),) + own.entities[2:])
    path = tmp_path / "plays.json"
    path.write_text(json.dumps({"plays": [{"name": "penalty", "entities": [list(e) for e in own.entities]}]}))
    tab = R.table_of_args(parse(["--setplay-file", str(path)]))
    assert tab.plays[1].entities[0][0] == 0.30 and tab.plays[0] == S.BUILTIN["free_ball"] and tab.plays[2] == S.BUILTIN["goal_kick"]
    assert R.table_of_args(parse([])).plays == R.RefTable().plays


def test_the_flags_are_structural_on_resume():
    assert CK.REFEREE_STRUCTURAL == ("ref_stall_steps", "ref_stall_speed", "ref_area_steps", "ref_area_depth",
                                     "ref_area_width", "ref_max_stops")
    base = dict(env_id="sa", num_envs=8, num_steps=4, seed=1, opponent="ou", cuda=True)
    on = dict(base, ref_stall_steps=100, ref_area_steps=20)
    assert CK.check_compatible(on, dict(on), log=None) == []
    CK.check_compatible(base, dict(base, **CK.REFEREE_DEFAULTS), log=None)   # an absent key counts as its default
    CK.check_compatible(dict(base, **CK.REFEREE_DEFAULTS), base, log=None)
    CK.check_compatible(on, dict(on, ref_stall_speed=0.05, ref_max_stops=0), log=None)
    for other in (dict(on, ref_stall_steps=50), dict(on, ref_area_steps=0), dict(on, ref_stall_speed=0.1),
                  dict(on, ref_area_depth=0.2), dict(on, ref_area_width=0.5), dict(on, ref_max_stops=1), base):
        with pytest.raises(ValueError, match="structural and differs"):
            CK.check_compatible(on, other, log=None)
    with pytest.raises(ValueError, match="ref_stall_steps"):
        CK.check_compatible(base, on, log=None)


def test_the_training_script_keeps_its_line_cap():
    import ppo_continuous_action_isaacgym as P
    with open(P.__file__) as f:
        assert len(f.read().splitlines()) <= 600
