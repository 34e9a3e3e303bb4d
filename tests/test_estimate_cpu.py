"""The estimation channel without a GPU (include/vss.h, vss_amd/estimate.py): its part of the
one ABI (1 function, 1 struct) and of the one library's source stamp, the entry's
argument checks on addresses that are never dereferenced, the float32 specification `reference_estimate` on known
answers -- DESIGN.md §3's table, the episode edges, one world -- and against the project's own physics (the C oracle)
on contact-free scenes, and the flag's plumbing (parse_args, the checkpoint's structural key)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import ppo_continuous_action_isaacgym as P
from test_perceive_cpu import done_patterns, same_bits, world
from vss_amd import _native as N
from vss_amd import checkpoint as CK
from vss_amd import cheader
from vss_amd import estimate as E
from vss_amd import perceive as PC

F32 = np.float32
FAKE = 1 << 20  # non-null, 16-B aligned, never dereferenced: every call below returns before a launch
GAP = 1 << 24   # between two fake buffers: further apart than any extent used here
E_ARG = 1
ACTS = list(PC.ACTION_FLOATS)
ROW = 52 * 4


def call(n_fields=64, lay=(3, 0, 3, 1), delay=2, call_index=0, obs=FAKE, term=FAKE + GAP, done=FAKE + 2 * GAP,
         done_stride=1, hist=FAKE + 3 * GAP, age=FAKE + 5 * GAP, obs_out=FAKE + 6 * GAP, term_out=FAKE + 7 * GAP,
         null_lay=False):
    layout = E.VssEstimateLayout(*lay)
    return N.load().vss_estimate(None, n_fields, None if null_lay else ctypes.byref(layout), delay, call_index, obs, term,
                                 done, done_stride, hist, age, obs_out, term_out)


def state(shape, delay):
    return np.zeros((delay,) + shape + (6,), F32), np.zeros(shape, np.int32)


def run(obs, term, dones, delay):
    """reference_estimate over the calls (call 0 is the start): (obs_e, term_e, age, hist) per call."""
    hist, age = state(obs.shape[1:4], delay)
    out = []
    for t in range(obs.shape[0]):
        o, x = E.reference_estimate(obs[t], None if t == 0 else term[t], None if t == 0 else dones[t], hist, age, t, delay)
        out.append((o, x, age.copy(), hist.copy()))
    return out


def rest_rows(m, yaw=0.0):
    """(m, 52) rows of a world at rest at the origin, every robot heading `yaw`."""
    rows = np.zeros((m, 52), F32)
    for base in E.OWN + E.OPPONENTS:
        rows[:, base + 4], rows[:, base + 5] = F32(np.cos(yaw)), F32(np.sin(yaw))
    return rows


# ---- the channel's part of the one ABI and the one library -------------------------------------------------------------
def exported(path, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(1) for m in re.finditer(rf"^\S+\s+T\s+({prefix}\w*)$", out, flags=re.M))


def test_the_header_declares_vss_estimate_and_its_struct_and_the_library_exports_it():
    with open(N.HEADER) as f:
        h = cheader.parse(f.read())
    assert [name for name in h.functions if "estimate" in name] == ["vss_estimate"] and "vss_estimate" in N.EXPORTED
    assert sorted(name for name in h.structs if "estimate" in name) == ["vss_estimate_layout"]
    assert {k: v for k, v in h.constants.items() if "ESTIMATE" in k} == {"VSS_ESTIMATE_MAX_DELAY": 15}
    assert E.MAX_DELAY == 15 == N.ESTIMATE_MAX_DELAY
    assert E.VssEstimateLayout is N.VssEstimateLayout
    assert ctypes.sizeof(E.VssEstimateLayout) == 24 == ctypes.sizeof(h.structs["vss_estimate_layout"])
    assert N.load().vss_estimate.argtypes == h.functions["vss_estimate"][1]
    if shutil.which("nm"):
        assert exported(N.LIB_PATH, "vss_estimate") == ["vss_estimate"]
        assert exported(N.LIB_PATH, "vss_") == sorted(h.functions)


def test_the_unit_is_one_of_the_core_librarys_and_nothing_is_packaged_beside_it():
    assert [os.path.basename(p) for p in N.STAMPED].count("vss_estimate.hip") == 1
    assert os.path.join(N.CSRC, "vss_estimate.hip") in N.STAMPED
    assert [os.path.join(d, f) for d, _, files in os.walk(N.CSRC) for f in files if f == "Makefile" or f.endswith(".mk")] \
        == [os.path.join(N.CSRC, "Makefile")]
    for name in ("LIB_PATH", "STAMPED", "CSRC", "HEADER", "ABI", "EXPORTED", "ABI_VERSION", "source_hash", "verify_source_hash"):
        assert not hasattr(E, name), name
    assert E.load is N.load  # the module's own name for the one loader
    assert not os.path.exists(os.path.join(os.path.dirname(N.HEADER), "vss_estimate.h"))


def test_the_stamp_covers_the_makefiles_list_and_a_stale_library_is_refused_at_load(tmp_path, monkeypatch):
    """A library built before vss_estimate.hip was edited is refused, and the hash a state file records
    (checkpoint.source_hash is N.source_hash) changes with that edit."""
    with open(os.path.join(N.CSRC, "Makefile")) as f:
        (line,) = re.findall(r"^STAMPED\s*:=\s*(.*)$", f.read(), flags=re.M)
    assert "vss_estimate.hip:STEP_FLAGS" in line.split()
    at = list(N.STAMPED).index(os.path.join(N.CSRC, "vss_estimate.hip"))
    assert all(os.path.isfile(p) for p in N.STAMPED)
    lib = N.load()
    N.verify_source_hash(lib)
    with pytest.raises(N.NativeError, match="built from other sources"):
        N.verify_source_hash(lib, expected="0" * 16)
    before = N.source_hash()
    assert CK.source_hash() == before
    src = os.path.join(tmp_path, "vss_estimate.hip")
    shutil.copy(N.STAMPED[at], src)
    with open(src, "a") as f:
        f.write("// edited after the build\n")
    monkeypatch.setattr(N, "STAMPED", tuple(N.STAMPED[:at]) + (src,) + tuple(N.STAMPED[at + 1:]))
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(N.NativeError, match=r"built from other sources.*make -C"):
        N.load()
    assert N.source_hash() != before and CK.source_hash() == N.source_hash()


# ---- the entry's refusals ----------------------------------------------------------------------------------------------
def test_the_accepted_calls_of_no_fields_and_null_pointers():
    assert call(n_fields=0) == 0
    assert call(n_fields=0, term=None, term_out=None) == 0
    assert call(n_fields=0, lay=(1, 0, 1, 1)) == 0 and call(n_fields=0, lay=(3, 99, 3, 2)) == 0
    assert call(n_fields=0, delay=0, hist=None) == 0 and call(n_fields=0, delay=15) == 0
    for z in (0, 64):
        for bad in ("obs", "done", "age", "obs_out", "hist"):
            assert call(n_fields=z, **{bad: None}) == E_ARG, (z, bad)  # hist: null with delay 2
        assert call(n_fields=z, null_lay=True) == E_ARG
        assert call(n_fields=z, term=None) == E_ARG and call(n_fields=z, term_out=None) == E_ARG  # exactly one of the two


def test_misaligned_pointers_are_rejected():
    rows = dict(obs=FAKE, term=FAKE + GAP, obs_out=FAKE + 6 * GAP, term_out=FAKE + 7 * GAP)
    for name, base in rows.items():
        for off in (4, 8, 12, 1):
            assert call(**{name: base + off}) == E_ARG, (name, off)
    for name, base in dict(done=FAKE + 2 * GAP, hist=FAKE + 3 * GAP).items():
        for off in (4, 1, 2, 7):
            assert call(**{name: base + off}) == E_ARG, (name, off)
        assert call(n_fields=0, **{name: base + 8}) == 0
    for off in (2, 1, 3):
        assert call(age=FAKE + 5 * GAP + off) == E_ARG, off
    assert call(n_fields=0, age=FAKE + 5 * GAP + 4) == 0


def test_an_output_overlapping_an_input_or_another_output_is_rejected():
    obs, term, done, hist, age, obs_out, term_out = (FAKE + i * GAP for i in (0, 1, 2, 3, 5, 6, 7))
    last = 191 * ROW  # 64 fields x 3 robots: 192 rows
    for out in ("obs_out", "term_out"):
        for other in (obs, term):
            assert call(**{out: other}) == E_ARG and call(**{out: other + last}) == E_ARG and call(**{out: other - last}) == E_ARG
        assert call(**{out: done + 16}) == E_ARG and call(**{out: done - last}) == E_ARG
    assert call(term_out=obs_out) == E_ARG and call(term_out=obs_out + last) == E_ARG
    hist_last = 2 * 192 * 24 - 8
    for other in (obs, term, obs_out, term_out):
        assert call(hist=other) == E_ARG and call(hist=other + last) == E_ARG and call(hist=other - hist_last) == E_ARG
        assert call(age=other) == E_ARG and call(age=other + last + 4) == E_ARG and call(age=other - 191 * 4) == E_ARG
    assert call(hist=done + 8) == E_ARG and call(age=done + 8) == E_ARG and call(age=done - 191 * 4) == E_ARG
    assert call(age=hist) == E_ARG and call(age=hist + hist_last + 4) == E_ARG and call(hist=age + 191 * 4 - 4) == E_ARG
    assert call(n_fields=0, obs_out=obs) == E_ARG and call(n_fields=0, hist=term) == E_ARG  # by address at any size


def test_values_out_of_range_are_rejected():
    for delay in (-1, 16, 100, -(1 << 31)):
        assert call(delay=delay) == E_ARG, delay
        assert call(n_fields=0, delay=delay) == E_ARG, delay
    for robots in (0, 2, 4, -1):
        assert call(lay=(4, 0, robots, 1)) == E_ARG, robots
    for teams in (0, 3, -1):
        assert call(lay=(3, 192, 3, teams)) == E_ARG, teams
    for stride in (2, 0, -3):
        assert call(lay=(stride, 0, 3, 1)) == E_ARG, stride
    assert call(lay=(0, 0, 1, 1)) == E_ARG
    for team_stride in (191, 0, -192):  # two teams of 64 fields x 3 robots: a block spans 192
        assert call(lay=(3, team_stride, 3, 2)) == E_ARG, team_stride
    for stride in (0, -1):
        assert call(done_stride=stride) == E_ARG, stride
    assert call(n_fields=-1) == E_ARG
    # sizes that overflow the byte offsets or the grid
    assert call(n_fields=1 << 60) == E_ARG
    assert call(n_fields=1 << 30, lay=(1 << 40, 0, 3, 1)) == E_ARG
    assert call(n_fields=64, lay=(3, 1 << 62, 3, 2)) == E_ARG
    assert call(n_fields=64, done_stride=1 << 62) == E_ARG
    assert call(n_fields=(1 << 31) * 300, lay=(1, 0, 1, 1)) == E_ARG


def test_the_python_side_refuses_the_same_values():
    hist, age = state((1, 4, 1), 2)
    obs = np.zeros((1, 4, 1, 52), F32)
    with pytest.raises(ValueError, match="delay"):
        E.reference_estimate(obs, None, None, hist, age, 0, 16)
    with pytest.raises(ValueError, match="hist"):
        E.reference_estimate(obs, None, None, hist, age, 0, 3)
    with pytest.raises(ValueError, match="obs must be"):
        E.reference_estimate(obs[..., :51], None, None, hist, age, 0, 2)
    with pytest.raises(ValueError, match="command for every step"):
        E.predict_rows(obs[0, :, 0], 3, np.zeros((4, 2, 6), F32))
    with pytest.raises(N.NativeError):
        E.EstimationChannel(4, E.layout_sa(), 2, "cpu")


# ---- the flag ----------------------------------------------------------------------------------------------------------
def test_the_flag_defaults_to_zero_is_structural_and_needs_a_delay():
    from envs.wrappers import estimation_args
    a = P.parse_args([])
    assert a.obs_predict == 0 and estimation_args(a) is False
    b = P.parse_args(["--obs-delay", "2", "--obs-predict", "1"])
    assert b.obs_predict == 1 and estimation_args(b) is True
    assert estimation_args(P.parse_args(["--obs-delay", "2", "--obs-predict", "0"])) is False
    for argv in (["--obs-predict", "1"], ["--obs-predict", "1", "--obs-delay", "0", "--obs-noise-pos", "0.002"]):
        with pytest.raises(ValueError, match=r"--obs-predict 1 needs --obs-delay.*nothing to predict"):
            P.parse_args(argv)
    with pytest.raises(SystemExit):
        P.parse_args(["--obs-delay", "2", "--obs-predict", "2"])
    assert CK.ESTIMATION_STRUCTURAL == ("obs_predict",)
    assert CK.PERCEPTION_STRUCTURAL == ("obs_delay", "obs_noise_pos", "obs_noise_vel", "obs_noise_ang", "obs_noise_angvel")
    off = P.parse_args(["--obs-delay", "2"])
    with pytest.raises(ValueError, match="obs_predict"):
        CK.check_compatible(vars(b), off, log=None)
    with pytest.raises(ValueError, match="obs_predict"):
        CK.check_compatible(vars(off), b, log=None)
    old = {k: v for k, v in vars(off).items() if k != "obs_predict"}  # a state file from before the flag
    assert CK.check_compatible(old, off, log=None) is not None
    with pytest.raises(ValueError, match="obs_predict"):
        CK.check_compatible(old, b, log=None)


def test_the_layouts_are_perceptions_without_the_first_team():
    assert E.layout_sa() == (1, 0, 1, 1) and E.layout_dma() == (3, 0, 3, 1) == E.layout_opponent()
    assert E.layout_mirror(3, 100) == (3, 300, 3, 2) and E.layout_mirror(1, 100) == (1, 100, 1, 2)
    assert E.layout_full_blue() == (6, 0, 3, 1) and E.of_perception(PC.layout_opponent()) == E.layout_opponent()
    assert E.layout_mirror(3, 100).span(100) == 600 and E.layout_full_blue().span(100) == 597
    assert np.array_equal(E.layout_mirror(3, 4).row_index(4), PC.layout_mirror(3, 4).row_index(4))


# ---- reference_estimate: known answers -----------------------------------------------------------------------------------
def test_delay_zero_and_every_lead_zero_case_are_bitwise_copies():
    g = np.random.default_rng(3)
    obs = g.standard_normal((12, 2, 9, 3, 52)).astype(F32)
    term = g.standard_normal((12, 2, 9, 3, 52)).astype(F32)
    obs[:, 0, 0, 0, 0], obs[:, 0, 0, 0, 1], obs[:, 0, 0, 0, 2] = -0.0, 0.0, np.nan
    term[:, 0, 0, 0, 3] = -0.0
    dones = done_patterns(12, 9)
    for t, (o, x, age, hist) in enumerate(run(obs, term, dones, 0)):  # D = 0: copies, no ring
        assert same_bits(o, obs[t]) and (t == 0 or same_bits(x, term[t])) and (age == 0).all() and hist.size == 0
        assert np.signbit(o[0, 0, 0, 0]) and not np.signbit(o[0, 0, 0, 1])
    res = run(obs, term, dones, 3)
    assert same_bits(res[0][0], obs[0]) and res[0][1] is None  # the start call
    for t in range(1, 12):
        fresh = dones[t] != 0  # a row whose field has just reset: lead 0
        assert fresh.any() and same_bits(res[t][0][:, fresh], obs[t][:, fresh]), t
        assert not same_bits(res[t][0][:, ~fresh], obs[t][:, ~fresh]), t
        assert same_bits(res[t][0][..., ACTS], obs[t][..., ACTS]) and same_bits(res[t][1][..., ACTS], term[t][..., ACTS]), t
    assert same_bits(E.predict_rows(obs[0, 0, :, 0], 0, np.zeros((9, 0, 6), F32)), obs[0, 0, :, 0])


def test_a_robot_at_rest_with_zero_commands_stays_put_and_its_heading_stays_a_unit_vector():
    yaws = np.linspace(-3.1, 3.1, 41)
    rows = np.concatenate([rest_rows(1, y) for y in yaws])
    rows[:, 0:2] = (0.3, -0.2)
    out = E.predict_rows(rows, 15, np.zeros((41, 15, 6), F32))
    keep = [i for i in range(52) if not any(i in (b + 4, b + 5) for b in E.OWN + E.OPPONENTS)]
    assert np.array_equal(out[:, keep], rows[:, keep])  # (by value: c * 0 - s * 0 may be -0.0)
    for base in E.OWN + E.OPPONENTS:
        c, s = out[:, base + 4].astype(np.float64), out[:, base + 5].astype(np.float64)
        assert np.abs(np.hypot(c, s) - 1).max() <= 2 ** -23  # 1 ulp of 1
        assert np.abs(c - np.cos(yaws)).max() <= 2e-7 and np.abs(s - np.sin(yaws)).max() <= 2e-7


def test_straight_drive_gains_a_substep_of_traction_up_to_the_wheel_speed():
    """DESIGN.md §3's table: +0.15 m/s per substep up to 42 rad/s x 0.024 m = 1.008 m/s along the heading, within 2e-5."""
    for yaw in (0.0, 0.7, 1.5707964, 3.0, -2.2):
        for sign in (1.0, -1.0):
            rows = rest_rows(1, yaw)
            cmds = np.full((1, 8, 6), sign, F32)
            speeds = []
            for lead in range(9):
                out = E.predict_rows(rows, lead, cmds)
                for base in E.OWN:
                    v = out[0, base + 2:base + 4].astype(np.float64)
                    along = v @ np.array([np.cos(yaw), np.sin(yaw)])
                    assert abs(along - sign * min(0.3 * lead, 1.008)) <= 2e-5 and abs(np.hypot(*v) - abs(along)) <= 2e-5
                    assert abs(out[0, base + 6]) <= 1e-4
                speeds.append(along)
                for base in E.OPPONENTS:  # their commands are unknown: they stay at rest
                    assert same_bits(out[0, base:base + 4], rows[0, base:base + 4]) and out[0, base + 6] == 0
            one = E.predict_rows(rows, 1, cmds)  # one control step: two substeps of +0.15, x = (0.15 + 0.30) h
            assert abs(np.hypot(*one[0, 4:6].astype(np.float64)) - 0.45 * 0.025) <= 1e-7


def test_spin_in_place_reaches_the_wheel_speed_over_the_half_track():
    """§3's table: (-1, +1) -> +29.87 rad/s (CCW), 4.444 rad/s per substep, no translation; within 1e-3 / 2e-4."""
    for sign in (1.0, -1.0):
        rows = rest_rows(1, 0.4)
        cmds = np.tile(np.array([-sign, sign] * 3, F32), (1, 8, 1))
        one = E.predict_rows(rows, 1, cmds)
        assert abs(one[0, 10] - sign * 2 * 0.15 / 0.03375) <= 1e-3
        out = E.predict_rows(rows, 8, cmds)
        for base in E.OWN:
            assert abs(out[0, base + 6] - sign * 2 * 1.008 / 0.0675) <= 1e-3
            assert np.abs(out[0, base:base + 4]).max() <= 2e-4
            c, s = out[0, base + 4].astype(np.float64), out[0, base + 5].astype(np.float64)
            assert abs(np.hypot(c, s) - 1) <= 2 ** -22
        # CCW for (-1, +1): the heading has advanced the way the yaw rate points, by the trapezoid of its ramp
        first = E.predict_rows(rows, 1, cmds)
        turned = np.arctan2(first[0, 9].astype(np.float64), first[0, 8]) - 0.4
        assert abs(turned - sign * (4.4444444 + 8.8888889) * 0.025) <= 2e-4


def test_the_free_ball_follows_the_exact_float_recurrence():
    rows = rest_rows(3)
    rows[:, 0:4] = [(0.1, -0.2, 0.8, -0.3), (-0.4, 0.3, -1.2, 0.05), (0.0, 0.0, 0.0, -0.0)]
    want = rows[:, 0:4].copy()
    for lead in range(1, 16):
        for _ in range(2):
            want[:, 2] = want[:, 2] * F32(0.99625)
            want[:, 3] = want[:, 3] * F32(0.99625)
            want[:, 0] = want[:, 0] + want[:, 2] * F32(0.025)
            want[:, 1] = want[:, 1] + want[:, 3] * F32(0.025)
        out = E.predict_rows(rows, lead, np.ones((3, 15, 6), F32))
        assert same_bits(out[:, 0:4], want), lead
    assert abs(want[0, 2] / 0.8 - 0.99625 ** 30) <= 1e-6  # v0 (1 - 0.15 h)^(t / h), ~ v0 exp(-0.15 t)


def test_opponents_move_at_constant_velocity_and_yaw_rate():
    g = np.random.default_rng(5)
    rows = rest_rows(16)
    for base in E.OPPONENTS:
        rows[:, base:base + 4] = g.uniform(-0.5, 0.5, (16, 4))
        rows[:, base + 6] = g.uniform(-20, 20, 16)
    out = E.predict_rows(rows, 6, g.uniform(-1, 1, (16, 6, 6)).astype(F32))
    for base in E.OPPONENTS:
        assert same_bits(out[:, base + 2:base + 4], rows[:, base + 2:base + 4]) and same_bits(out[:, base + 6], rows[:, base + 6])
        want = rows[:, base:base + 2].astype(np.float64) + 0.3 * rows[:, base + 2:base + 4]
        assert np.abs(out[:, base:base + 2] - want).max() <= 1e-6
        turned = np.arctan2(out[:, base + 5].astype(np.float64), out[:, base + 4]) - 0.3 * rows[:, base + 6]
        assert np.abs(np.sin(turned)).max() <= 1e-5 and np.abs(np.cos(turned) - 1).max() <= 1e-5


def test_episode_edges_every_output_uses_its_own_episodes_commands_only():
    """§17.5's done patterns.  Own robot 0 of every row starts each call at rest at the origin, heading +x, and call
    t's command is (c_t, c_t) with c_t = 0.1 * 2^t / 8192: small enough for the wheels to reach it within a substep,
    so x_e / (0.05 * 1.008) is the sum of the commands used and names the calls bit by bit."""
    D, calls, n = 3, 12, 40
    dones = done_patterns(calls, n)
    code = (0.1 * (1 << np.arange(calls)) / 8192).astype(F32)
    obs = np.zeros((calls, 1, n, 1, 52), F32)
    obs[..., :] = rest_rows(1)[0]
    obs[..., 11] = obs[..., 12] = code[:, None, None, None]
    term = obs.copy()
    unit = 0.05 * 1.008 * 0.1 / 8192
    first = np.zeros(n, int)  # the call of each field's episode's first row
    for t, (o, x, age, hist) in enumerate(run(obs, term, dones, D)):
        prev_first = first.copy()
        if t:
            first = np.where(dones[t] != 0, t, first)
        lead_o = np.minimum(t - first, D)
        assert np.array_equal(age[0, :, 0], lead_o), t
        mask_o = np.rint(o[0, :, 0, 4].astype(np.float64) / unit).astype(int)
        want_o = np.array([sum(1 << c for c in range(t - L + 1, t + 1)) for L in lead_o])
        assert np.array_equal(mask_o, want_o), (t, mask_o, want_o)
        assert all(c > s for L, s in zip(lead_o, first) for c in range(t - L + 1, t + 1) if L)  # after the episode's first call
        if t:
            lead_t = np.minimum(t - prev_first, D)
            assert (lead_t >= 1).all()
            mask_t = np.rint(x[0, :, 0, 4].astype(np.float64) / unit).astype(int)
            want_t = np.array([sum(1 << c for c in range(t - L + 1, t + 1)) for L in lead_t])
            assert np.array_equal(mask_t, want_t), (t, mask_t, want_t)
            assert all(t - L + 1 > s for L, s in zip(lead_t, prev_first))  # the ending episode's calls only
        assert same_bits(hist[t % D, 0, :, 0, :2], np.broadcast_to(code[t], (n, 2)))


def test_one_world_the_three_rows_of_a_team_predict_each_entity_to_the_same_bits():
    n, D, calls = 32, 3, 12
    worlds = [world(n, 20 + t) for t in range(calls)]
    rows = np.stack([PC.full_rows(b, r).transpose(1, 0, 2, 3) for b, r in worlds])  # (calls, 2, n, 3, 52)
    dones = done_patterns(calls, n)
    for t, (o, x, age, hist) in enumerate(run(rows, rows, dones, D)):
        for out in (o,) if x is None else (o, x):
            for k in (1, 2):
                assert same_bits(out[:, :, k, 0:4], out[:, :, 0, 0:4]) and same_bits(out[:, :, k, 31:52], out[:, :, 0, 31:52]), (t, k)
                for e in range(3):  # robot e: own slot e of row 0, own slot (e - k) % 3 of row k
                    j = (e - k) % 3
                    assert same_bits(out[:, :, k, 4 + 9 * j:13 + 9 * j], out[:, :, 0, 4 + 9 * e:13 + 9 * e]), (t, k, e)
        if t >= 3:
            assert not same_bits(o, rows[t])


# ---- against the project's own physics -----------------------------------------------------------------------------------
# Scenes that are contact-free by construction: the seven bodies on distinct points of a 3 x 3 grid 0.45 m apart in x
# and 0.4 m in y (0.3 m and 0.25 m from the walls), robots starting with at most 0.2 m/s along their heading and any yaw
# rate, the ball with at most 0.5 m/s; start + 4 steps.  A robot travels at most 0.147 m in 0.2 s (6 m/s^2 up to
# 1.008 m/s), the ball 0.1 m: pairs stay >= 0.106 m apart, every body's surface >= 0.063 m from a wall.
GRID = [(x, y) for x in (-0.45, 0.0, 0.45) for y in (-0.4, 0.0, 0.4)]
STEPS = 4  # no longer: the scenes stay contact-free by construction only while nobody can reach a neighbour or a wall
PHYS_D = 3
# measured here (the maxima over the 256 fields x 4 calls x 6 rows below) and the bounds: 4 x the maximum, rounded up to
# one significant digit -- the margin covers other seeds of the same scenes.  See DESIGN.md §19.5.
# The only modelling difference is the heading carried as (cos, sin) instead of a quaternion, so the error is a
# rounding-level quantity.  The opponents' figures (their commands are unknown) are reported only.
#   class            predicted, measured   bound     un-predicted delayed row   opponents, predicted
#   position, m      5.96e-08              3e-07     0.125                      0.0886
#   velocity, m/s    4.17e-07              2e-06     0.946                      0.946
#   heading (c, s)   6.11e-07              3e-06     2.0                        1.84
#   yaw rate, rad/s  1.07e-05              5e-05     26.7                       26.7
BOUNDS = dict(position=3e-7, velocity=2e-6, heading=3e-6, yaw_rate=5e-5)


def scenes(n, seed):
    g = np.random.default_rng(seed)
    s = np.zeros((O.STATE_CHANNELS, n), F32)
    yaw = g.uniform(-np.pi, np.pi, (6, n))
    v0 = g.uniform(-0.2, 0.2, (6, n))
    for f in range(n):
        spots = g.permutation(len(GRID))[:7]
        for r in range(6):
            s[O.CH_RX + r, f], s[O.CH_RY + r, f] = GRID[spots[r]]
        s[0, f], s[1, f] = GRID[spots[6]]
    s[O.CH_RQZ:O.CH_RQZ + 6], s[O.CH_RQW:O.CH_RQW + 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    s[O.CH_RVX:O.CH_RVX + 6], s[O.CH_RVY:O.CH_RVY + 6] = v0 * np.cos(yaw), v0 * np.sin(yaw)
    s[O.CH_RW:O.CH_RW + 6] = g.uniform(-25, 25, (6, n))
    speed, heading = g.uniform(0, 0.5, n), g.uniform(-np.pi, np.pi, n)
    s[2], s[3] = speed * np.cos(heading), speed * np.sin(heading)
    # commands over the whole range: constant in the first half of the fields, changing at step 2 or 3 in the second;
    # a quarter of all wheels at exactly -1, 0 or +1
    a = g.uniform(-1, 1, (n, 12)).astype(F32)
    b = g.uniform(-1, 1, (n, 12)).astype(F32)
    for arr in (a, b):
        pick = g.random(arr.shape) < 0.25
        arr[pick] = g.choice(np.array([-1.0, 0.0, 1.0], F32), int(pick.sum()))
    actions = np.repeat(a[None], STEPS, 0)
    switch = g.integers(1, 3, n)
    for f in range(n // 2, n):
        actions[switch[f]:, f] = b[f]
    return s, actions


def rows_of(s, actions):
    """FULL rows (2, n, 3, 52) of an oracle state with the commands that led to it (n, 12), headings as the oracle's
    heading(): (qw^2 - qz^2, 2 qw qz) in float32."""
    n = s.shape[1]
    qz, qw = s[O.CH_RQZ:O.CH_RQZ + 6], s[O.CH_RQW:O.CH_RQW + 6]
    robots = np.stack([s[O.CH_RX:O.CH_RX + 6], s[O.CH_RY:O.CH_RY + 6], s[O.CH_RVX:O.CH_RVX + 6], s[O.CH_RVY:O.CH_RVY + 6],
                       qw * qw - qz * qz, F32(2.0) * qw * qz, s[O.CH_RW:O.CH_RW + 6],
                       actions.reshape(n, 6, 2)[:, :, 0].T, actions.reshape(n, 6, 2)[:, :, 1].T], -1)  # (6, n, 9)
    return PC.full_rows(s[0:4].T, robots.transpose(1, 0, 2)).transpose(1, 0, 2, 3)


def test_against_the_oracles_physics_on_contact_free_scenes():
    n = 256
    s, actions = scenes(n, 11)
    truth = [rows_of(s, np.zeros((n, 12), F32))]
    closest_pair, closest_wall = np.inf, np.inf
    for t in range(STEPS):
        O.simulate(s, np.ascontiguousarray(actions[t]))
        truth.append(rows_of(s, actions[t]))
        x = np.concatenate([s[O.CH_RX:O.CH_RX + 6], s[0:1]]).astype(np.float64)
        y = np.concatenate([s[O.CH_RY:O.CH_RY + 6], s[1:2]]).astype(np.float64)
        dist = np.hypot(x[:, None] - x[None], y[:, None] - y[None]) + 10 * np.eye(7)[:, :, None]
        radius = np.array([0.04] * 6 + [0.02134])[:, None]
        closest_pair = min(closest_pair, dist.min())
        closest_wall = min(closest_wall, (0.75 - np.abs(x) - radius).min(), (0.65 - np.abs(y) - radius).min())
    print("closest pair", closest_pair, "m; closest wall", closest_wall, "m")
    assert closest_pair >= 0.1 and closest_wall >= 0.05  # the condition: no case is left out
    shape = truth[0].shape[:3]
    ring, p_age = np.zeros((PHYS_D + 1,) + truth[0].shape, F32), np.zeros(n, np.int32)
    hist, age = state(shape, PHYS_D)
    none = np.zeros(n, np.int64)
    classes = dict(position=[0, 1] + [b + i for b in E.OWN for i in (0, 1)], velocity=[2, 3] + [b + i for b in E.OWN for i in (2, 3)],
                   heading=[b + i for b in E.OWN for i in (4, 5)], yaw_rate=[b + 6 for b in E.OWN])
    opponents = dict(position=[b + i for b in E.OPPONENTS for i in (0, 1)], velocity=[b + i for b in E.OPPONENTS for i in (2, 3)],
                     heading=[b + i for b in E.OPPONENTS for i in (4, 5)], yaw_rate=[b + 6 for b in E.OPPONENTS])
    worst = dict.fromkeys(classes, 0.0)
    stale = dict.fromkeys(classes, 0.0)
    theirs = dict.fromkeys(classes, 0.0)
    for t in range(STEPS + 1):
        start = t == 0
        seen, seen_t = PC.reference_perceive(truth[t], None if start else truth[t], none, ring, p_age, t, PHYS_D, (0, 0, 0, 0), 0)
        est, est_t = E.reference_estimate(seen, seen_t, none, hist, age, t, PHYS_D)
        assert (age == min(t, PHYS_D)).all() and (start or same_bits(est, est_t))
        for name, cols in classes.items():
            worst[name] = max(worst[name], float(np.abs(est[..., cols].astype(np.float64) - truth[t][..., cols]).max()))
            stale[name] = max(stale[name], float(np.abs(seen[..., cols].astype(np.float64) - truth[t][..., cols]).max()))
            theirs[name] = max(theirs[name], float(np.abs(est[..., opponents[name]].astype(np.float64)
                                                         - truth[t][..., opponents[name]]).max()))
        assert same_bits(est[..., ACTS], truth[t][..., ACTS])
    for name in classes:
        print(f"{name}: predicted {worst[name]:.3g} (bound {BOUNDS[name]:g}), un-predicted delayed row {stale[name]:.3g}, "
              f"opponents (commands unknown, reported only) {theirs[name]:.3g}")
    for name in classes:
        assert worst[name] <= BOUNDS[name], (name, worst[name])
