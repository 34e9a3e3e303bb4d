"""The set plays without a GPU (include/vss.h, vss_amd/setplay.py): the unit's part of the one header,
library and source stamp, the entry's argument checks on addresses that are never dereferenced,
Table.validate rule by rule, the float32 specification `reference_setplay` on known answers -- no jitter, each flip
alone, the share and the weights' statistics, the clearance of 10,000 draws per built-in -- and the flags' plumbing."""
import argparse
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vss_amd import _native as N
from vss_amd import checkpoint as CK
from vss_amd import cheader
from vss_amd import setplay as S

F32 = np.float32
FAKE = 1 << 20  # non-null, 16-B aligned, never dereferenced: every call below returns before a launch
GAP = 1 << 24   # between two fake buffers: further apart than any extent used here
E_ARG, OK = 1, 0
ROW = 52 * 4
ALL_NAMES = list(S.BUILTIN) + [f"{n}_{s}" for n in S.BUILTIN for s in ("for", "against")]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fresh(n):
    st = np.zeros((58, n), F32)
    st[N.CH_RQW:N.CH_RQW + 6] = 1.0
    return st


def good_table():
    return S.Table(S.plays_of_mix("kickoff:1,penalty_for:2"), 0.5).c_table()


def call(n_fields=64, tab=None, done=FAKE, done_stride=1, state=FAKE + GAP, views=((FAKE + 2 * GAP, 3, 0, 3, 1, 0),),
         counts=FAKE + 4 * GAP, chosen=FAKE + 5 * GAP, null_tab=False, n_views=None, null_views=False):
    tab = good_table() if tab is None else tab
    arr = (S.VssSetplayView * 2)()
    for i, v in enumerate(views):
        arr[i] = S.VssSetplayView(*v)
    nv = len(views) if n_views is None else n_views
    return S.load().vss_setplay(None, n_fields, None if null_tab else ctypes.byref(tab), 7, 3, done, done_stride, state,
                                nv, None if null_views else arr, counts, chosen)


# ---- the set plays' part of the one ABI and the one library -----------------------------------------------------------
def exported(path, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(1) for m in re.finditer(rf"^\S+\s+T\s+({prefix}\w*)$", out, flags=re.M))


def test_the_header_parses_and_the_library_exports_exactly_its_functions():
    with open(N.HEADER) as f:
        h = cheader.parse(f.read())
    assert [name for name in h.functions if "setplay" in name] == ["vss_setplay"] and "vss_setplay" in N.EXPORTED
    assert sorted(name for name in h.structs if "setplay" in name) == ["vss_setplay_entity", "vss_setplay_play",
                                                                       "vss_setplay_table", "vss_setplay_view"]
    assert {k: v for k, v in h.constants.items() if "SETPLAY" in k} == {"VSS_SETPLAY_MAX_PLAYS": 8}
    assert S.MAX_PLAYS == 8 == N.SETPLAY_MAX_PLAYS
    assert (S.VssSetplayEntity, S.VssSetplayPlay, S.VssSetplayTable, S.VssSetplayView) \
        == (N.VssSetplayEntity, N.VssSetplayPlay, N.VssSetplayTable, N.VssSetplayView)
    assert ctypes.sizeof(S.VssSetplayEntity) == 20 and ctypes.sizeof(S.VssSetplayPlay) == 7 * 20 + 24
    assert ctypes.sizeof(S.VssSetplayTable) == 12 + 8 * 164 and ctypes.sizeof(S.VssSetplayView) == 40
    assert [ctypes.sizeof(h.structs["vss_setplay_" + n]) for n in ("entity", "play", "table", "view")] == [20, 164, 12 + 8 * 164, 40]
    assert [n for n, _ in S.VssSetplayView._fields_] == ["obs"] + [n for n, _ in N.VssPerceiveLayout._fields_]
    assert N.load().vss_setplay.argtypes == h.functions["vss_setplay"][1]
    if shutil.which("nm"):
        assert exported(N.LIB_PATH, "vss_setplay") == ["vss_setplay"]
        assert exported(N.LIB_PATH, "vss_") == sorted(h.functions)


def test_the_unit_is_one_of_the_core_librarys_and_nothing_is_packaged_beside_it():
    assert [os.path.basename(p) for p in N.STAMPED].count("vss_setplay.hip") == 1
    assert os.path.join(N.CSRC, "vss_setplay.hip") in N.STAMPED and os.path.join(N.CSRC, "vss_placement.h") in N.STAMPED
    assert [os.path.join(d, f) for d, _, files in os.walk(N.CSRC) for f in files if f == "Makefile" or f.endswith(".mk")] \
        == [os.path.join(N.CSRC, "Makefile")]
    for name in ("LIB_PATH", "STAMPED", "CSRC", "HEADER", "ABI", "EXPORTED", "ABI_VERSION", "source_hash", "verify_source_hash"):
        assert not hasattr(S, name), name
    assert S.load is N.load  # the module's own name for the one loader
    assert not os.path.exists(os.path.join(os.path.dirname(N.HEADER), "vss_setplay.h"))
    assert [d for d in os.listdir(os.path.dirname(N.CSRC)) if d.startswith("csrc")] == ["csrc"]  # no unit beside the core


def test_the_parser_takes_a_member_of_an_earlier_struct_and_nothing_more():
    h = cheader.parse("typedef struct vss_a { float x, y; } vss_a;\n"
                      "typedef struct vss_b { vss_a one; const vss_a e[3]; int32_t n; vss_a* p; } vss_b;")
    b = h.structs["vss_b"]
    assert [n for n, _ in b._fields_] == ["one", "e", "n", "p"] and ctypes.sizeof(b) == 8 + 24 + 8 + 8
    assert b._fields_[0][1] is h.structs["vss_a"] and b._fields_[3][1] is ctypes.c_void_p
    for text in ("typedef struct vss_b { vss_a one; } vss_b;\ntypedef struct vss_a { float x; } vss_a;",  # defined later
                 "typedef struct vss_b { vss_b self; } vss_b;",
                 "typedef struct vss_a { float x; } vss_a;\nint vss_f(vss_a a);",                        # by value: a parameter
                 "typedef struct vss_a { float x; } vss_a;\nvss_a vss_f(void);",
                 "typedef struct vss_a { float x; } vss_a;\ntypedef struct vss_b { unsigned vss_a one; } vss_b;"):
        with pytest.raises(cheader.HeaderError):
            cheader.parse(text)


def stale_copy_is_refused(name, flags, tmp_path, monkeypatch):
    """A library built before csrc/<name> was edited is refused at load, and the hash a state file records
    (checkpoint.source_hash is N.source_hash) changes with that edit.  `flags`: the word's flag set on the STAMPED line."""
    with open(os.path.join(N.CSRC, "Makefile")) as f:
        text = f.read()
    (line,) = re.findall(r"^STAMPED\s*:=\s*(.*)$", text, flags=re.M)
    assert (name + ":" + flags if flags else name) in line.split()
    assert re.search(r"^STEP_FLAGS := \$\(COMMON\) -ffp-contract=off$", text, re.M) and re.search(r"^resource-usage:", text, re.M)
    at = list(N.STAMPED).index(os.path.join(N.CSRC, name))
    assert all(os.path.isfile(p) for p in N.STAMPED)
    lib = N.load()
    N.verify_source_hash(lib)
    with pytest.raises(N.NativeError, match="built from other sources"):
        N.verify_source_hash(lib, expected="0" * 16)
    before = N.source_hash()
    assert CK.source_hash() == before
    src = os.path.join(tmp_path, name)
    shutil.copy(N.STAMPED[at], src)
    with open(src, "a") as f:
        f.write("// edited after the build\n")
    monkeypatch.setattr(N, "STAMPED", tuple(N.STAMPED[:at]) + (src,) + tuple(N.STAMPED[at + 1:]))
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(N.NativeError, match=r"built from other sources.*rebuild it with.*make -C"):
        N.load()
    assert N.source_hash() != before and CK.source_hash() == N.source_hash()


def test_the_stamp_covers_the_units_sources_and_a_stale_library_is_refused(tmp_path, monkeypatch):
    stale_copy_is_refused("vss_setplay.hip", "STEP_FLAGS", tmp_path, monkeypatch)


def test_the_stamp_covers_the_shared_placement_header(tmp_path, monkeypatch):
    stale_copy_is_refused("vss_placement.h", "", tmp_path, monkeypatch)


# ---- the entry's refusals ----------------------------------------------------------------------------------------------
def test_zero_size_and_good_calls_that_stop_before_a_launch():
    assert call(n_fields=0) == OK
    assert call(n_fields=0, done=None) == OK               # a start call
    assert call(n_fields=0, views=(), counts=None, chosen=None) == OK
    assert call(n_fields=0, views=((FAKE + 2 * GAP, 6, 3, 3, 2, 0),)) == OK
    assert call(n_fields=0, views=((FAKE + 2 * GAP, 1, 0, 1, 1, 0), (FAKE + 3 * GAP, 3, 0, 3, 1, 1))) == OK


def test_null_pointers_view_shapes_alignment_and_sizes_are_refused():
    for n in (64, 0):
        assert call(n_fields=n, null_tab=True) == E_ARG
        assert call(n_fields=n, state=None) == E_ARG
        assert call(n_fields=n, null_views=True) == E_ARG
        assert call(n_fields=n, n_views=3) == E_ARG and call(n_fields=n, n_views=-1) == E_ARG
        assert call(n_fields=n, views=((0, 3, 0, 3, 1, 0),)) == E_ARG
        for bad in ((3, 0, 2, 1, 0), (3, 0, 0, 1, 0), (3, 0, 3, 0, 0), (3, 0, 3, 3, 0), (3, 0, 3, 1, 2), (3, 0, 3, 1, -1),
                    (6, 3, 3, 2, 1), (2, 0, 3, 1, 0), (0, 0, 1, 1, 0), (-1, 0, 1, 1, 0)):
            assert call(n_fields=n, views=((FAKE + 2 * GAP,) + bad,)) == E_ARG, bad
    for off in range(1, 16):
        assert call(views=((FAKE + 2 * GAP + off, 3, 0, 3, 1, 0),)) == E_ARG
        if off % 8:
            assert call(done=FAKE + off) == E_ARG and call(counts=FAKE + 4 * GAP + off) == E_ARG
        if off % 4:
            assert call(state=FAKE + GAP + off) == E_ARG and call(chosen=FAKE + 5 * GAP + off) == E_ARG
    assert call(done_stride=0) == E_ARG and call(done_stride=-1) == E_ARG
    assert call(n_fields=0, done=None, done_stride=0) == OK  # a start call reads no stride
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
    rows = FAKE + 2 * GAP
    assert call(state=rows) == E_ARG and call(state=rows + 191 * ROW) == E_ARG      # state on the rows
    assert call(state=rows - (64 * 58 * 4 - 4)) == E_ARG
    assert call(chosen=rows + 16) == E_ARG and call(counts=rows + 8) == E_ARG
    assert call(chosen=FAKE + GAP + 4) == E_ARG and call(counts=FAKE + GAP + 64 * 58 * 4 - 8) == E_ARG
    assert call(done=FAKE + GAP) == E_ARG and call(done=rows + 8) == E_ARG          # an output on done
    assert call(chosen=FAKE + 8) == E_ARG and call(counts=FAKE + 63 * 8) == E_ARG
    assert call(views=((rows, 1, 0, 1, 1, 0), (rows + 63 * ROW, 3, 0, 3, 1, 1))) == E_ARG
    assert call(views=((rows, 1, 0, 1, 1, 0), (rows, 3, 0, 3, 1, 1))) == E_ARG
    assert call(n_fields=0, state=rows) == E_ARG and call(n_fields=0, done=FAKE + GAP) == E_ARG  # equality at any size


def bad_tables():
    """(what, a table the entry must refuse): one per rule, built past Table.validate on the raw struct."""
    def edit(fn):
        t = good_table()
        fn(t)
        return t
    out = [("count 0", edit(lambda t: setattr(t, "count", 0))), ("count 9", edit(lambda t: setattr(t, "count", 9))),
           ("share nan", edit(lambda t: setattr(t, "share", math.nan))), ("share 1.5", edit(lambda t: setattr(t, "share", 1.5))),
           ("share < 0", edit(lambda t: setattr(t, "share", -0.1))),
           ("flip_x 2", edit(lambda t: setattr(t.play[0], "p_flip_x", 2.0))),
           ("flip_y < 0", edit(lambda t: setattr(t.play[1], "p_flip_y", -0.5))),
           ("cum decreases", edit(lambda t: setattr(t.play[1], "cum_weight", 0.5))),
           ("cum negative", edit(lambda t: setattr(t.play[0], "cum_weight", -1.0))),
           ("total is not the last cum", edit(lambda t: setattr(t, "total_weight", 2.0))),
           ("x inf", edit(lambda t: setattr(t.play[0].e[2], "x", math.inf))),
           ("yaw nan", edit(lambda t: setattr(t.play[0].e[2], "yaw", math.nan))),
           ("ball velocity nan", edit(lambda t: setattr(t.play[0], "ball_vx", math.nan))),
           ("r_vel < 0", edit(lambda t: setattr(t.play[0], "r_vel", -1.0))),
           ("yaw > pi", edit(lambda t: setattr(t.play[0].e[1], "yaw", 3.2))),
           ("r_yaw > pi", edit(lambda t: setattr(t.play[0].e[1], "r_yaw", 3.2))),
           ("r_yaw < 0", edit(lambda t: setattr(t.play[0].e[1], "r_yaw", -0.1))),
           ("r_pos < 0", edit(lambda t: setattr(t.play[0].e[1], "r_pos", -0.01))),
           ("robot past x", edit(lambda t: setattr(t.play[0].e[6], "x", 0.70))),       # 0.70 + 0.02 > 0.71
           ("robot past y", edit(lambda t: setattr(t.play[0].e[2], "y", 0.59))),       # 0.59 + 0.03 > 0.61
           ("ball past the line", edit(lambda t: setattr(t.play[0].e[0], "x", 0.76))),
           ("a pair too close", edit(lambda t: setattr(t.play[0].e[1], "x", -0.08)))]  # 0.08 - sqrt(2) 0.01 < 0.08

    def zero(t):
        t.play[0].cum_weight = t.play[1].cum_weight = t.total_weight = 0.0
    return out + [("total weight 0", edit(zero))]


def test_every_table_rule_is_refused_before_a_launch():
    assert call(n_fields=0, tab=good_table()) == OK
    for what, tab in bad_tables():
        assert call(tab=tab) == E_ARG, what
        assert call(n_fields=0, tab=tab) == E_ARG, what


# ---- Table.validate ------------------------------------------------------------------------------------------------------
def test_validate_accepts_every_builtin_and_its_variants():
    for name in ALL_NAMES:
        tab = S.Table([S.named_play(name)], 1.0)
        assert call(n_fields=0, tab=tab.c_table()) == OK, name
    assert S.named_play("penalty_for").p_flip_x == 0.0 and S.named_play("penalty_against").p_flip_x == 1.0
    assert S.named_play("penalty").p_flip_x == 0.5 == S.named_play("penalty").p_flip_y
    assert sorted(S.BUILTIN) == ["breakaway", "free_ball", "goal_kick", "kickoff", "penalty"]
    # the clearance the issue states: the tightest pair of the built-ins is just above the rule
    gaps = []
    for p in S.BUILTIN.values():
        d = np.asarray(p.entities, np.float64)
        gaps += [math.hypot(*(d[i, :2] - d[j, :2])) - math.sqrt(2) * (d[i, 3] + d[j, 3]) for i in range(7) for j in range(i)]
    assert 0.08 <= min(gaps) < 0.082


def test_validate_rejects_one_counter_example_per_rule():
    k = S.BUILTIN["kickoff"]

    def ent(e, **kw):
        rows = [list(r) for r in k.entities]
        for name, v in kw.items():
            rows[e][("x", "y", "yaw", "r_pos", "r_yaw").index(name)] = v
        return k._replace(entities=tuple(tuple(r) for r in rows))
    bad = [([], 1.0), ([k] * 9, 1.0), ([k], 1.5), ([k], -0.1), ([k], math.nan),
           ([k._replace(weight=-1.0)], 1.0), ([k._replace(weight=0.0)], 1.0), ([k._replace(weight=math.inf)], 1.0),
           ([k._replace(p_flip_x=1.1)], 1.0), ([k._replace(p_flip_y=-0.1)], 1.0), ([k._replace(p_flip_y=math.nan)], 1.0),
           ([k._replace(ball_vel=(math.nan, 0, 0))], 1.0), ([k._replace(ball_vel=(0, 0, -1.0))], 1.0),
           ([ent(2, x=math.inf)], 1.0), ([ent(2, yaw=math.nan)], 1.0), ([ent(1, yaw=3.2)], 1.0), ([ent(1, yaw=-3.2)], 1.0),
           ([ent(1, r_yaw=3.2)], 1.0), ([ent(1, r_yaw=-0.1)], 1.0), ([ent(1, r_pos=-0.01)], 1.0),
           ([ent(6, x=0.70)], 1.0), ([ent(2, y=0.59)], 1.0), ([ent(2, y=-0.59)], 1.0), ([ent(0, x=0.76)], 1.0),
           ([ent(0, y=0.66)], 1.0), ([ent(1, x=-0.08)], 1.0), ([k._replace(entities=k.entities[:6])], 1.0)]
    for plays, share in bad:
        with pytest.raises(ValueError):
            S.Table(plays, share)
    S.Table([k, k._replace(name="again", weight=0.0)], 0.0)  # a zero weight beside a positive one, and share 0, are fine
    with pytest.raises(ValueError, match="could start in contact"):
        S.Table([ent(1, x=-0.08)], 1.0)
    with pytest.raises(ValueError, match="can leave the field"):
        S.Table([ent(6, x=0.70)], 1.0)


# ---- the specification ---------------------------------------------------------------------------------------------------
RIGID = S.Play("rigid", tuple((x, y, yaw, 0.0, 0.0) for x, y, yaw in
                              ((0.1, 0.05, 0.0), (-0.2, 0.1, 0.5), (-0.4, -0.2, -1.0), (-0.6, 0.3, 2.0),
                               (0.3, -0.1, 3.0), (0.5, 0.2, -2.5), (0.65, 0.0, 1.5707964))), (0.25, -0.5, 0.0), 1.0, 0.0, 0.0)


def staged_one(play, seed=5):
    st, rows, chosen, counts = fresh(1), np.zeros((6, 52), F32), np.zeros(1, np.int32), np.zeros(8, np.int64)
    f = S.reference_setplay(S.Table([play], 1.0), seed, 0, None, st, [(rows, S.view_full())], counts, chosen)
    assert f.tolist() == [0] and chosen.tolist() == [0] and counts.tolist() == [1] + [0] * 7
    return st[:, 0], rows.reshape(2, 3, 52)


def yaw_of(st, r):
    return 2.0 * math.atan2(float(st[N.CH_RQZ + r]), float(st[N.CH_RQW + r]))


def test_known_answers_without_jitter_and_with_each_flip_alone():
    e = np.asarray(RIGID.entities, np.float64)
    st, rows = staged_one(RIGID)
    assert same_bits(st[0:4], [0.1, 0.05, 0.25, -0.5])
    assert same_bits(st[N.CH_RX:N.CH_RX + 6], e[1:, 0].astype(F32)) and same_bits(st[N.CH_RY:N.CH_RY + 6], e[1:, 1].astype(F32))
    for r in range(6):
        assert abs(yaw_of(st, r) - e[1 + r, 2]) < 1e-6
    for ch in (N.CH_RQX, N.CH_RQY, N.CH_RVX, N.CH_RVY, N.CH_RW):
        assert same_bits(st[ch:ch + 6], np.zeros(6, F32))  # +0.0
    # the rows: blue 0's view, own slot j = robot j; the own-action floats +0.0; heading c, s
    b0 = rows[0, 0]
    assert same_bits(b0[0:4], st[0:4]) and same_bits(b0[[4, 5]], [-0.2, 0.1]) and same_bits(b0[[13, 14]], [-0.4, -0.2])
    assert same_bits(b0[[31, 32]], [0.3, -0.1]) and same_bits(b0[[11, 12, 20, 21, 29, 30]], np.zeros(6, F32))
    assert abs(b0[8] - math.cos(0.5)) < 1e-6 and abs(b0[9] - math.sin(0.5)) < 1e-6
    assert same_bits(rows[0, 1][[4, 5]], [-0.4, -0.2]) and same_bits(rows[0, 1][[22, 23]], [-0.2, 0.1])  # own slot j = (k + j) % 3
    # the yellow rows are the negated blue view: yellow 0 sees itself at (-0.3, 0.1), the ball at (-0.1, -0.05)
    y0 = rows[1, 0]
    assert same_bits(y0[0:4], [-0.1, -0.05, -0.25, 0.5]) and same_bits(y0[[4, 5]], [-0.3, 0.1])
    assert same_bits(y0[[31, 32]], [0.2, -0.1]) and same_bits(y0[[6, 7]], [-0.0, -0.0]) and same_bits(y0[[10, 11, 12]], [0.0] * 3)

    # flip_y alone: y, vy and yaw negated, nothing else
    sy, _ = staged_one(RIGID._replace(p_flip_y=1.0))
    assert same_bits(sy[[0, 2]], st[[0, 2]]) and same_bits(sy[[1, 3]], -st[[1, 3]])
    assert same_bits(sy[N.CH_RX:N.CH_RX + 6], st[N.CH_RX:N.CH_RX + 6]) and same_bits(sy[N.CH_RY:N.CH_RY + 6], -st[N.CH_RY:N.CH_RY + 6])
    assert same_bits(sy[N.CH_RQZ:N.CH_RQZ + 6], -st[N.CH_RQZ:N.CH_RQZ + 6]) and same_bits(sy[N.CH_RQW:N.CH_RQW + 6], st[N.CH_RQW:N.CH_RQW + 6])

    # flip_x alone: the teams swapped and x negated, bit for bit; yaw -> pi - yaw
    sx, rx = staged_one(RIGID._replace(p_flip_x=1.0))
    swap = [3, 4, 5, 0, 1, 2]
    assert same_bits(sx[[0, 2]], -st[[0, 2]]) and same_bits(sx[[1, 3]], st[[1, 3]])
    assert same_bits(sx[N.CH_RX:N.CH_RX + 6], -st[N.CH_RX:N.CH_RX + 6][swap]) and same_bits(sx[N.CH_RY:N.CH_RY + 6], st[N.CH_RY:N.CH_RY + 6][swap])
    for r in range(6):
        want = math.pi - e[1 + swap[r], 2]
        assert abs(math.remainder(yaw_of(sx, r) - want, 2 * math.pi)) < 1e-6
    assert same_bits(rx[0, 0][[4, 5]], [-0.3, -0.1])  # blue 0 stands where yellow 0 stood, mirrored


def test_a_flipped_staging_mirrors_the_jitter_bit_for_bit():
    """The same draws (one seed, one call) with p_flip_x 0 and 1: positions are the unflipped ones with the teams
    swapped and x negated, exactly -- the flips come after the jitter."""
    n = 512
    out = {}
    for name in ("kickoff_for", "kickoff_against"):
        play = S.named_play(name)._replace(p_flip_y=0.0)
        st = fresh(n)
        S.reference_setplay(S.Table([play], 1.0), 99, 4, None, st)
        out[name] = st
    a, b = out["kickoff_for"], out["kickoff_against"]
    swap = [3, 4, 5, 0, 1, 2]
    assert same_bits(b[0], -a[0]) and same_bits(b[1], a[1])
    assert same_bits(b[N.CH_RX:N.CH_RX + 6], -a[N.CH_RX:N.CH_RX + 6][swap]) and same_bits(b[N.CH_RY:N.CH_RY + 6], a[N.CH_RY:N.CH_RY + 6][swap])
    assert not same_bits(a[N.CH_RX], np.full(n, a[N.CH_RX, 0]))  # there is jitter


def test_the_yellow_rows_are_the_negated_blue_view_and_rows_match_the_state():
    n = 256
    st, rows = fresh(n), np.zeros((n * 6, 52), F32)
    S.reference_setplay(S.Table(S.plays_of_mix(), 1.0), 3, 1, None, st, [(rows, S.view_full())])
    full = rows.reshape(n, 2, 3, 52)
    assert same_bits(full, S.full_rows_of_state(st, np.arange(n)))
    assert same_bits(full[:, 1, 0, 0:4], -full[:, 0, 0, 0:4])
    assert same_bits(full[:, 1, 0, 31:37], -full[:, 0, 0, 4:10]) and same_bits(full[:, 1, 0, 37], full[:, 0, 0, 10])
    # the smaller views are slices of FULL
    sa, dma, opp = np.zeros((n, 52), F32), np.zeros((n * 3, 52), F32), np.zeros((n * 3, 52), F32)
    st2 = fresh(n)
    S.reference_setplay(S.Table(S.plays_of_mix(), 1.0), 3, 1, None, st2, [(sa, S.view_sa()), (opp, S.view_opponent())])
    S.reference_setplay(S.Table(S.plays_of_mix(), 1.0), 3, 1, None, fresh(n), [(dma, S.view_dma())])
    assert same_bits(st2, st) and same_bits(sa, full[:, 0, 0]) and same_bits(opp.reshape(n, 3, 52), full[:, 1])
    assert same_bits(dma.reshape(n, 3, 52), full[:, 0])
    mir = np.zeros((2 * n * 3, 52), F32)
    S.reference_setplay(S.Table(S.plays_of_mix(), 1.0), 3, 1, None, fresh(n), [(mir, S.view_mirror(3, n))])
    assert same_bits(mir.reshape(2, n, 3, 52), full.transpose(1, 0, 2, 3))


@pytest.mark.parametrize("name", list(S.BUILTIN))
def test_ten_thousand_draws_of_a_builtin_keep_clear_and_inside(name):
    n = 10000
    st = fresh(n)
    f = S.reference_setplay(S.Table([S.named_play(name)], 1.0), 2026, 0, None, st)
    assert f.size == n
    pos = np.stack([np.concatenate([st[0:1], st[N.CH_RX:N.CH_RX + 6]]), np.concatenate([st[1:2], st[N.CH_RY:N.CH_RY + 6]])], -1)
    d = np.linalg.norm(pos[:, None].astype(np.float64) - pos[None, :].astype(np.float64), axis=-1)  # (7, 7, n)
    d[np.arange(7), np.arange(7)] = 9.0
    assert d.min() >= 0.08
    assert np.abs(pos[1:, :, 0]).max() <= 0.71 + 1e-6 and np.abs(pos[1:, :, 1]).max() <= 0.61 + 1e-6  # inside the walls
    assert np.abs(pos[0, :, 0]).max() <= 0.75 and np.abs(pos[0, :, 1]).max() <= 0.65
    q = st[N.CH_RQZ:N.CH_RQZ + 6].astype(np.float64) ** 2 + st[N.CH_RQW:N.CH_RQW + 6].astype(np.float64) ** 2
    assert np.abs(np.sqrt(q) - 1.0).max() <= 2 * 2.0 ** -23  # |q| = 1 to 2 ulp
    # both mirrorings occur: the ball of a play with an off-centre ball is seen in every quadrant it can reach
    if name == "free_ball":
        assert {(int(np.sign(x)), int(np.sign(y))) for x, y in zip(st[0], st[1])} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}


def test_the_share_and_the_weights_decide_who_is_staged():
    n = 65536
    plays = S.plays_of_mix("kickoff:1,free_ball:2,penalty_for:1,goal_kick:0,breakaway:4")
    done = (np.arange(n) % 3 != 0).astype(np.int64)
    for share, expect in ((0.0, 0), (1.0, int(done.sum()))):
        st, chosen, counts = fresh(n), np.zeros(n, np.int32), np.zeros(8, np.int64)
        before = st.copy()
        f = S.reference_setplay(S.Table(plays, share), 11, 2, done, st, (), counts, chosen)
        assert f.size == expect == counts.sum() and (chosen[done == 0] == -1).all()
        assert same_bits(st[:, done == 0], before[:, done == 0])
        assert ((chosen >= 0) == (done != 0)).all() if share else (chosen == -1).all()
    st, chosen, counts = fresh(n), np.zeros(n, np.int32), np.zeros(8, np.int64)
    f = S.reference_setplay(S.Table(plays, 0.5), 11, 2, None, st, (), counts, chosen)
    assert abs(f.size / n - 0.5) <= 0.0078  # 4 sigma of a fair coin over 65,536 fields
    assert counts.tolist() == np.bincount(chosen[chosen >= 0], minlength=8).tolist() and counts[3] == 0
    m, w = f.size, np.array([1, 2, 1, 0, 4]) / 8.0
    assert (np.abs(counts[:5] / m - w) <= 4 * np.sqrt(w * (1 - w) / m)).all()
    # another call, other fields; the same call, the same fields
    g = S.reference_setplay(S.Table(plays, 0.5), 11, 3, None, fresh(n))
    h = S.reference_setplay(S.Table(plays, 0.5), 11, 2, None, fresh(n))
    assert not np.array_equal(f, g) and np.array_equal(f, h)
    # only=k: every field, play k, its index kept
    chosen = np.zeros(64, np.int32)
    S.reference_setplay(S.Table(plays, 0.25).only(2), 11, 0, None, fresh(64), (), None, chosen)
    assert (chosen == 2).all()


# ---- flags, the mix, the file, resume ---------------------------------------------------------------------------------------
def parse(argv):
    return CK.add_channel_arguments(argparse.ArgumentParser()).parse_args(argv)


def test_flags_defaults_and_the_mix_grammar():
    args = parse([])
    assert (args.setplay_share, args.setplay_mix, args.setplay_file, args.eval_setplays) == (0.0, None, None, "")
    assert S.table_of_args(args) is None and S.table_of_args(argparse.Namespace()) is None
    tab = S.table_of_args(parse(["--setplay-share", "0.25"]))
    assert tab.names == tuple(S.BUILTIN) and tab.share == 0.25 and tab.cum_weights().tolist() == [1, 2, 3, 4, 5]
    tab = S.table_of_args(parse(["--setplay-share", "1", "--setplay-mix", "kickoff:1, free_ball:2.5,penalty_for"]))
    assert tab.names == ("kickoff", "free_ball", "penalty_for") and tab.cum_weights().tolist() == [1.0, 3.5, 4.5]
    assert tab.plays[2].p_flip_x == 0.0
    for mix in ("nosuch:1", "kickoff:x", "kickoff,,penalty", "kickoff:1,kickoff:2", "kickoff:-1", "kickoff:0",
                ",".join(ALL_NAMES[:9])):
        with pytest.raises(ValueError):
            S.table_of_args(parse(["--setplay-share", "0.5", "--setplay-mix", mix]))
    for share in ("-0.1", "1.5"):
        with pytest.raises(ValueError, match="setplay-share"):
            S.table_of_args(parse(["--setplay-share", share]))
    assert S.setplay_seed(3) != S.setplay_seed(3, 1) != S.setplay_seed(4) and 0 <= S.setplay_seed(2 ** 40) < 2 ** 64
    from envs.wrappers import actuation_seed, perception_seed, setplay_seed
    assert setplay_seed(3, 1) == S.setplay_seed(3, 1) and len({S.setplay_seed(3), perception_seed(3), actuation_seed(3)}) == 3


def test_custom_plays_come_from_a_json_file_of_settings(tmp_path):
    corner = {"name": "corner", "entities": [[0.6, 0.5, 0, 0, 0], [0.45, 0.45, 0, 0.01, 0.2], [0, 0, 0, 0.03, 0.5],
                                             [-0.6, 0, 0, 0.02, 0.5], [0.68, 0.1, 3.0, 0.02, 0.5], [0.3, -0.2, 3.0, 0.03, 0.5],
                                             [0.5, 0.2, 3.0, 0.02, 0.5]], "ball_vel": [0.1, 0, 0.05], "p_flip_x": 0.0}
    path = tmp_path / "plays.json"
    path.write_text(json.dumps({"plays": [corner]}))
    tab = S.table_of_args(parse(["--setplay-share", "0.5", "--setplay-file", str(path)]))
    assert tab.names == ("corner",) and tab.plays[0].ball_vel == (0.1, 0.0, 0.05) and tab.plays[0].p_flip_y == 0.5
    tab = S.table_of_args(parse(["--setplay-share", "0.5", "--setplay-file", str(path), "--setplay-mix", "corner_against:2,kickoff"]))
    assert tab.names == ("corner_against", "kickoff") and tab.plays[0].p_flip_x == 1.0
    for doc in ({}, {"plays": []}, {"plays": [dict(corner, extra=1)]}, {"plays": [dict(corner, name="x_for")]},
                {"plays": [corner, corner]}, {"plays": [dict(corner, entities=corner["entities"][:6])]},
                {"plays": [dict(corner, entities=[[0.74, 0, 0, 0, 0]] + corner["entities"][1:6] + [[0.74, 0, 0, 0, 0]])]}):
        path.write_text(json.dumps(doc))
        with pytest.raises((ValueError, KeyError)):
            S.load_file(str(path))


def test_the_flags_are_structural_on_resume():
    assert CK.SETPLAY_STRUCTURAL == ("setplay_share", "setplay_mix", "setplay_file")
    base = dict(env_id="sa", num_envs=8, num_steps=4, seed=1, opponent="ou", cuda=True)
    on = dict(base, setplay_share=0.5, setplay_mix="kickoff:1,penalty:2", setplay_file=None)
    assert CK.check_compatible(on, dict(on), log=None) == []
    CK.check_compatible(base, dict(base, setplay_share=0.0, setplay_mix=None, setplay_file=None), log=None)
    CK.check_compatible(base, dict(base, setplay_share=0.0), log=None)      # an absent key counts as its default
    CK.check_compatible(dict(base, setplay_mix=None), dict(base, setplay_mix=""), log=None)
    for other in (dict(on, setplay_share=0.25), dict(on, setplay_mix="kickoff:1"), dict(on, setplay_file="plays.json"), base):
        with pytest.raises(ValueError, match="structural and differs"):
            CK.check_compatible(on, other, log=None)
    with pytest.raises(ValueError, match="setplay_share"):
        CK.check_compatible(base, on, log=None)


def test_the_arena_parses_eval_setplays():
    from vss_amd.arena import parse_setplays
    assert parse_setplays("") == [] and parse_setplays(None) == []
    assert parse_setplays("penalty_for, penalty_against") == ["penalty_for", "penalty_against"]
    with pytest.raises(ValueError):
        parse_setplays("penalty,penalty")


def test_the_training_script_keeps_its_line_cap():
    import ppo_continuous_action_isaacgym as P
    with open(P.__file__) as f:
        assert len(f.read().splitlines()) <= 600
