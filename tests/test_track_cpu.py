"""The tracking channel without a GPU (include/vss.h, vss_amd/track.py): the unit's part of the one header,
library and source stamp, the entry's argument checks on addresses that are never dereferenced, the
flags' plumbing, and the float32 specification `reference_track` on known answers -- bitwise copies, gain 1, each
gate at its threshold, the episode edges, one world -- and against the project's own physics (the C oracle) on
contact-free scenes: without noise the filter stays on the measurement, with noise it is closer to the truth."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import ppo_continuous_action_isaacgym as P
from test_estimate_cpu import STEPS, rest_rows, rows_of, scenes
from test_perceive_cpu import done_patterns, same_bits, world
from vss_amd import _native as N
from vss_amd import checkpoint as CK
from vss_amd import cheader
from vss_amd import estimate as E
from vss_amd import perceive as PC
from vss_amd import track as T

F32 = np.float32
FAKE = 1 << 20  # non-null, 16-B aligned, never dereferenced: every call below returns before a launch
GAP = 1 << 24   # between two fake buffers: further apart than any extent used here
E_ARG = 1
ACTS = list(PC.ACTION_FLOATS)
ROW = 52 * 4
BODIES = [(0, 4)] + [(b, 7) for b in E.OWN + E.OPPONENTS]  # (first float, floats) of the ball, the own robots, the opponents
ON = (0.2, 0.5, 0.5, 0.03, 0.5)


def call(n_fields=64, lay=(3, 0, 3, 1), prm=ON, delay=2, call_index=0, obs=FAKE, term=FAKE + GAP, done=FAKE + 2 * GAP,
         done_stride=1, est=FAKE + 4 * GAP, hist=FAKE + 3 * GAP, age=FAKE + 5 * GAP, obs_out=FAKE + 6 * GAP,
         term_out=FAKE + 7 * GAP, null_lay=False, null_prm=False):
    layout, params = T.VssTrackLayout(*lay), T.VssTrackParams(*prm)
    return T.load().vss_track(None, n_fields, None if null_lay else ctypes.byref(layout), None if null_prm else ctypes.byref(params),
                              delay, call_index, obs, term, done, done_stride, est, hist, age, obs_out, term_out)


def state(shape, delay):
    return np.zeros(shape + (52,), F32), np.zeros((delay,) + shape + (6,), F32), np.zeros(shape, np.int32)


def run(obs, term, dones, delay, params):
    """reference_track over the calls (call 0 is the start): (obs_f, term_f, age, hist, est before the call) per call."""
    est, hist, age = state(obs.shape[1:4], delay)
    out = []
    for t in range(obs.shape[0]):
        before = est.copy()
        o, x = T.reference_track(obs[t], None if t == 0 else term[t], None if t == 0 else dones[t], est, hist, age, t, delay, params)
        assert same_bits(est, o)
        out.append((o, x, age.copy(), hist.copy(), before))
    return out


# ---- the channel's part of the one ABI and the one library -------------------------------------------------------------
def exported(path, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(1) for m in re.finditer(rf"^\S+\s+T\s+({prefix}\w*)$", out, flags=re.M))


def test_the_header_parses_and_the_library_exports_exactly_its_functions():
    with open(N.HEADER) as f:
        h = cheader.parse(f.read())
    assert [name for name in h.functions if "track" in name] == ["vss_track"] and "vss_track" in N.EXPORTED
    assert sorted(name for name in h.structs if "track" in name) == ["vss_track_layout", "vss_track_params"]
    assert {k: v for k, v in h.constants.items() if "TRACK" in k} == {"VSS_TRACK_MAX_DELAY": 15}
    assert T.MAX_DELAY == 15 == N.TRACK_MAX_DELAY
    assert T.VssTrackLayout is N.VssTrackLayout and T.VssTrackParams is N.VssTrackParams
    assert ctypes.sizeof(T.VssTrackLayout) == 24 == ctypes.sizeof(N.VssEstimateLayout) and ctypes.sizeof(T.VssTrackParams) == 20
    assert ctypes.sizeof(h.structs["vss_track_layout"]) == 24 and ctypes.sizeof(h.structs["vss_track_params"]) == 20
    assert [n for n, _ in T.VssTrackLayout._fields_] == [n for n, _ in N.VssEstimateLayout._fields_]
    assert N.load().vss_track.argtypes == h.functions["vss_track"][1]
    if shutil.which("nm"):
        assert exported(N.LIB_PATH, "vss_track") == ["vss_track"]
        assert exported(N.LIB_PATH, "vss_") == sorted(h.functions)


def test_the_unit_is_one_of_the_core_librarys_and_nothing_is_packaged_beside_it():
    assert [os.path.basename(p) for p in N.STAMPED].count("vss_track.hip") == 1
    assert os.path.join(N.CSRC, "vss_track.hip") in N.STAMPED
    assert [os.path.join(d, f) for d, _, files in os.walk(N.CSRC) for f in files if f == "Makefile" or f.endswith(".mk")] \
        == [os.path.join(N.CSRC, "Makefile")]
    for name in ("LIB_PATH", "STAMPED", "CSRC", "HEADER", "ABI", "EXPORTED", "ABI_VERSION", "source_hash", "verify_source_hash"):
        assert not hasattr(T, name), name
    assert T.load is N.load  # the module's own name for the one loader
    assert not os.path.exists(os.path.join(os.path.dirname(N.HEADER), "vss_track.h"))
    assert [d for d in os.listdir(os.path.dirname(N.CSRC)) if d.startswith("csrc")] == ["csrc"]  # no unit beside the core


def test_the_stamp_covers_the_units_list_and_a_stale_library_is_refused_at_load(tmp_path, monkeypatch):
    """A library built before vss_track.hip was edited is refused, and the hash a state file records
    (checkpoint.source_hash is N.source_hash) changes with that edit."""
    with open(os.path.join(N.CSRC, "Makefile")) as f:
        (line,) = re.findall(r"^STAMPED\s*:=\s*(.*)$", f.read(), flags=re.M)
    assert "vss_track.hip:STEP_FLAGS" in line.split()
    at = list(N.STAMPED).index(os.path.join(N.CSRC, "vss_track.hip"))
    assert all(os.path.isfile(p) for p in N.STAMPED)
    lib = N.load()
    N.verify_source_hash(lib)
    with pytest.raises(N.NativeError, match="built from other sources"):
        N.verify_source_hash(lib, expected="0" * 16)
    before = N.source_hash()
    assert CK.source_hash() == before
    src = os.path.join(tmp_path, "vss_track.hip")
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
    assert call(n_fields=0, prm=(0, 0, 0, 0, 0)) == 0 and call(n_fields=0, prm=(1, 1, 1, 3e38, 3e38)) == 0
    for z in (0, 64):
        for bad in ("obs", "done", "age", "obs_out", "hist", "est"):
            assert call(n_fields=z, **{bad: None}) == E_ARG, (z, bad)  # hist: null with delay 2
        assert call(n_fields=z, null_lay=True) == E_ARG and call(n_fields=z, null_prm=True) == E_ARG
        assert call(n_fields=z, term=None) == E_ARG and call(n_fields=z, term_out=None) == E_ARG  # exactly one of the two


def test_misaligned_pointers_are_rejected():
    rows = dict(obs=FAKE, term=FAKE + GAP, est=FAKE + 4 * GAP, obs_out=FAKE + 6 * GAP, term_out=FAKE + 7 * GAP)
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
    obs, term, done, hist, est, age, obs_out, term_out = (FAKE + i * GAP for i in (0, 1, 2, 3, 4, 5, 6, 7))
    last = 191 * ROW  # 64 fields x 3 robots: 192 rows
    for out in ("obs_out", "term_out", "est"):
        for other in (obs, term):
            assert call(**{out: other}) == E_ARG and call(**{out: other + last}) == E_ARG and call(**{out: other - last}) == E_ARG
        assert call(**{out: done + 16}) == E_ARG and call(**{out: done - last}) == E_ARG
    assert call(term_out=obs_out) == E_ARG and call(term_out=obs_out + last) == E_ARG
    assert call(est=obs_out) == E_ARG and call(est=term_out - last) == E_ARG and call(est=obs_out + last) == E_ARG
    hist_last = 2 * 192 * 24 - 8
    for other in (obs, term, obs_out, term_out, est):
        assert call(hist=other) == E_ARG and call(hist=other + last) == E_ARG and call(hist=other - hist_last) == E_ARG
        assert call(age=other) == E_ARG and call(age=other + last + 4) == E_ARG and call(age=other - 191 * 4) == E_ARG
    assert call(hist=done + 8) == E_ARG and call(age=done + 8) == E_ARG and call(age=done - 191 * 4) == E_ARG
    assert call(age=hist) == E_ARG and call(age=hist + hist_last + 4) == E_ARG and call(hist=age + 191 * 4 - 4) == E_ARG
    assert call(n_fields=0, obs_out=obs) == E_ARG and call(n_fields=0, hist=term) == E_ARG  # by address at any size
    assert call(n_fields=0, est=obs) == E_ARG and call(n_fields=0, est=age) == E_ARG


def test_values_out_of_range_are_rejected():
    for delay in (-1, 16, 100, -(1 << 31)):
        assert call(delay=delay) == E_ARG, delay
        assert call(n_fields=0, delay=delay) == E_ARG, delay
    for i in range(3):  # gains outside [0, 1] or not finite
        for bad in (-0.001, 1.001, 2.0, float("nan"), float("inf"), -float("inf")):
            prm = list(ON)
            prm[i] = bad
            assert call(prm=prm) == E_ARG and call(n_fields=0, prm=prm) == E_ARG, (i, bad)
    for i in (3, 4):  # gates negative or not finite
        for bad in (-0.001, float("nan"), float("inf"), -float("inf")):
            prm = list(ON)
            prm[i] = bad
            assert call(prm=prm) == E_ARG and call(n_fields=0, prm=prm) == E_ARG, (i, bad)
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
    est, hist, age = state((1, 4, 1), 2)
    obs = np.zeros((1, 4, 1, 52), F32)
    with pytest.raises(ValueError, match="delay"):
        T.reference_track(obs, None, None, est, hist, age, 0, 16, ON)
    with pytest.raises(ValueError, match="hist"):
        T.reference_track(obs, None, None, est, hist, age, 0, 3, ON)
    with pytest.raises(ValueError, match="est"):
        T.reference_track(obs, None, None, est[..., :51], hist, age, 0, 2, ON)
    with pytest.raises(ValueError, match="obs must be"):
        T.reference_track(obs[..., :51], None, None, est, hist, age, 0, 2, ON)
    for bad in ((1.5, 0, 0), (0, -0.1, 0), (0, 0, float("nan")), (0.2, 0.5, 0.5, -1.0, 0.5), (0.2, 0.5, 0.5, 0.03, float("inf"))):
        with pytest.raises(ValueError, match="gain|gate"):
            T.reference_track(obs, None, None, est, hist, age, 0, 2, T.Params(*bad))
    with pytest.raises(N.NativeError):
        T.TrackingChannel(4, T.layout_sa(), 2, ON, "cpu")


# ---- the flags -----------------------------------------------------------------------------------------------------------
NOISE = ["--obs-noise-pos", "0.002"]


def test_the_flags_default_to_off_are_structural_and_need_noise():
    from envs.wrappers import tracking_args
    a = P.parse_args([])
    assert (a.obs_filter_team, a.obs_filter_opp, a.obs_filter_ball, a.obs_filter_gate_pos, a.obs_filter_gate_vel) == (0.0, 0.0, 0.0, 0.03, 0.5)
    assert tracking_args(a) == T.Params() and not tracking_args(a).any()
    b = P.parse_args(NOISE + ["--obs-filter-team", "0.2", "--obs-filter-opp", "0.5", "--obs-filter-ball", "0.6", "--obs-filter-gate-pos", "0.05"])
    assert tracking_args(b) == T.Params(0.2, 0.5, 0.6, 0.05, 0.5) and tracking_args(b).any()
    assert not tracking_args(P.parse_args(["--obs-filter-gate-vel", "0.7"])).any()  # a gate alone switches nothing on
    for argv in (["--obs-filter-team", "0.2"], ["--obs-delay", "2", "--obs-filter-ball", "0.5"]):
        with pytest.raises(ValueError, match=r"--obs-filter-\* needs vision noise.*nothing to filter"):
            P.parse_args(argv)
    for argv in (["--obs-filter-team", "1.5"], ["--obs-filter-opp", "-0.1"], ["--obs-filter-ball", "nan"]):
        with pytest.raises(ValueError, match=r"must be in \[0, 1\]"):
            P.parse_args(NOISE + argv)
    for argv in (["--obs-filter-gate-pos", "-1"], ["--obs-filter-gate-vel", "inf"]):
        with pytest.raises(ValueError, match="finite and >= 0"):
            P.parse_args(NOISE + argv)
    assert CK.TRACKING_STRUCTURAL == ("obs_filter_team", "obs_filter_opp", "obs_filter_ball", "obs_filter_gate_pos", "obs_filter_gate_vel")
    off = P.parse_args(NOISE)
    on = P.parse_args(NOISE + ["--obs-filter-team", "0.2"])
    other = P.parse_args(NOISE + ["--obs-filter-team", "0.3"])
    gate = P.parse_args(NOISE + ["--obs-filter-team", "0.2", "--obs-filter-gate-vel", "0.4"])
    for saved, new in ((on, off), (off, on), (on, other), (on, gate)):
        with pytest.raises(ValueError, match="obs_filter_(team|gate_vel) is structural"):
            CK.check_compatible(vars(saved), new, log=None)
    assert CK.check_compatible(vars(on), on, log=None) == []
    old = {k: v for k, v in vars(off).items() if not k.startswith("obs_filter")}  # a state file from before the flags
    assert CK.check_compatible(old, off, log=None) is not None  # absent keys count as their defaults, the gates' too
    with pytest.raises(ValueError, match="obs_filter_team"):
        CK.check_compatible(old, on, log=None)
    with pytest.raises(ValueError, match="obs_filter_gate_pos"):
        CK.check_compatible(old, P.parse_args(NOISE + ["--obs-filter-gate-pos", "0.05"]), log=None)
    assert len(open(P.__file__).read().splitlines()) <= 600


def test_the_wrappers_start_up_refusals():
    from envs.wrappers import Estimated, Perceived, Tracked
    with pytest.raises(ValueError, match="Tracked goes round a Perceived wrapper"):
        Tracked(object(), ON)
    quiet = object.__new__(Perceived)  # a Perceived whose four sigmas are all zero: refused before anything is built
    quiet.noise, quiet.delay = PC.Noise(), 2
    with pytest.raises(ValueError, match="nothing to filter"):
        Tracked(quiet, ON)
    late = object.__new__(Tracked)  # Estimated looks through Tracked and keeps its own refusal
    late.delay = 0
    with pytest.raises(ValueError, match="delay of at least 1"):
        Estimated(late)
    with pytest.raises(ValueError, match="delay of at least 1"):
        Estimated(object())


def test_the_layouts_are_estimations():
    assert T.Layout is E.Layout and T.layout_sa() == (1, 0, 1, 1) and T.layout_dma() == (3, 0, 3, 1) == T.layout_opponent()
    assert T.layout_mirror(3, 100) == (3, 300, 3, 2) and T.layout_full_blue() == (6, 0, 3, 1)
    assert T.of_perception(PC.layout_mirror(1, 100)) == (1, 100, 1, 2)


# ---- reference_track: known answers ----------------------------------------------------------------------------------
def test_a_kind_with_gain_zero_and_the_start_call_are_bitwise_copies():
    g = np.random.default_rng(3)
    obs = g.standard_normal((12, 2, 9, 3, 52)).astype(F32)
    term = g.standard_normal((12, 2, 9, 3, 52)).astype(F32)
    obs[:, 0, 0, 0, 0], obs[:, 0, 0, 0, 1], obs[:, 0, 0, 0, 2] = -0.0, 0.0, np.nan          # the ball
    obs[:, 0, 1, 0, 4], obs[:, 0, 1, 0, 8], obs[:, 0, 1, 0, 10] = -0.0, np.nan, -0.0        # own robot 0
    obs[:, 0, 2, 0, 31], obs[:, 0, 2, 0, 36] = np.nan, -0.0                                # opponent 0
    term[:, 0, 0, 0, 3], term[:, 0, 1, 0, 13], term[:, 0, 2, 0, 45] = -0.0, np.nan, -0.0
    dones = done_patterns(12, 9)
    for D in (0, 3):
        res = run(obs, term, dones, D, (0.0, 0.0, 0.0, 0.03, 0.5))  # every kind off: copies, whatever the state
        for t, (o, x, age, hist, _) in enumerate(res):
            assert same_bits(o, obs[t]) and (x is None if t == 0 else same_bits(x, term[t])), (D, t)
            assert np.signbit(o[0, 0, 0, 0]) and not np.signbit(o[0, 0, 0, 1]) and np.isnan(o[0, 0, 0, 2])
    kinds = dict(team=[c for b in E.OWN for c in range(b, b + 7)], opp=list(range(31, 52)), ball=[0, 1, 2, 3])
    with np.errstate(all="ignore"):
        for i, kind in enumerate(("team", "opp", "ball")):
            prm = [0.3, 0.4, 0.5, 0.0, 0.0]
            prm[i] = 0.0
            res = run(obs, term, dones, 3, prm)
            assert same_bits(res[0][0], obs[0]) and res[0][1] is None and (res[0][2] == 0).all()  # the start call
            assert same_bits(res[0][3][0], obs[0][..., ACTS])
            for t in range(1, 12):
                o, x = res[t][0], res[t][1]
                assert same_bits(o[..., kinds[kind]], obs[t][..., kinds[kind]]) and same_bits(x[..., kinds[kind]], term[t][..., kinds[kind]]), (kind, t)
                assert same_bits(o[..., ACTS], obs[t][..., ACTS]) and same_bits(x[..., ACTS], term[t][..., ACTS]), t
                fresh = dones[t] != 0  # a row whose field has just reset takes the new episode's first row
                assert fresh.any() and same_bits(o[:, fresh], obs[t][:, fresh]), t
                assert not same_bits(o[:, ~fresh], obs[t][:, ~fresh]) and not same_bits(x, term[t]), t


def plausible(g, m):
    rows = np.zeros((m, 52), F32)
    rows[:, 0:2], rows[:, 2:4] = g.uniform(-0.7, 0.7, (m, 2)), g.uniform(-1.5, 1.5, (m, 2))
    for base in E.OWN + E.OPPONENTS:
        yaw = g.uniform(-np.pi, np.pi, m)
        rows[:, base:base + 2], rows[:, base + 2:base + 4] = g.uniform(-0.7, 0.7, (m, 2)), g.uniform(-1.5, 1.5, (m, 2))
        rows[:, base + 4], rows[:, base + 5], rows[:, base + 6] = np.cos(yaw), np.sin(yaw), g.uniform(-20, 20, m)
    rows[:, ACTS] = g.uniform(-1, 1, (m, 6))
    return rows


def turned(rows, base, angle):
    c, s = rows[:, base + 4].astype(np.float64), rows[:, base + 5].astype(np.float64)
    rows[:, base + 4], rows[:, base + 5] = c * np.cos(angle) - s * np.sin(angle), s * np.cos(angle) + c * np.sin(angle)


def test_gain_one_with_the_gates_off_returns_the_measurement():
    """p + 1 (z - p): z to within one unit in the last place of z for x, y, vx, vy and the yaw rate (measured here: 0
    on these rows).  The heading is rotated by sin(delta) instead of delta: for |delta| <= 0.1 rad the result is within
    delta^3 / 6 = 1.67e-4 of z's heading, plus rounding (measured: 9.9e-5 at deltas up to 0.09)."""
    g = np.random.default_rng(5)
    m = 4000
    p = plausible(g, m)
    z = p.copy()
    z[:, 0:4] += g.normal(0, [0.002, 0.002, 0.05, 0.05], (m, 4)).astype(F32)
    for base in E.OWN + E.OPPONENTS:
        z[:, base:base + 4] += g.normal(0, [0.002, 0.002, 0.05, 0.05], (m, 4)).astype(F32)
        turned(z, base, np.clip(g.normal(0, 0.03, m), -0.1, 0.1))
        z[:, base + 6] += g.normal(0, 0.5, m).astype(F32)
    z[:, ACTS] = g.uniform(-1, 1, (m, 6))
    o = T.update_rows(p, z, (1.0, 1.0, 1.0, 0.0, 0.0))
    heading = [b + i for b in E.OWN + E.OPPONENTS for i in (4, 5)]
    linear = [c for c in range(52) if c not in heading and c not in ACTS]
    err = np.abs(o.astype(np.float64) - z)
    print("gain 1: largest deviation, linear floats", err[:, linear].max(), "heading", err[:, heading].max())
    assert (err[:, linear] <= np.spacing(np.abs(z[:, linear]))).all()
    assert err[:, heading].max() <= 0.1 ** 3 / 6 + 1e-6
    assert same_bits(o[:, ACTS], z[:, ACTS])


def test_each_gate_trips_exactly_past_its_threshold_and_reinitialises_only_that_body():
    gate_pos, gate_vel = F32(0.03), F32(0.5)
    prm = (0.25, 0.5, 0.75, float(gate_pos), float(gate_vel))
    p = rest_rows(1)  # at the origin, heading +x
    base_z = p.copy()
    for b, n in BODIES:
        base_z[0, b:b + 4] = (0.001, -0.001, 0.01, -0.01)  # every body a little off its prediction: the blend shows
    blend = T.update_rows(p, base_z, prm)
    for b, n in BODIES:
        assert not (blend[0, b:b + n] == base_z[0, b:b + n])[:4].any()

    def only(z, hit):
        out = T.update_rows(p, z, prm)
        for b, n in BODIES:
            if b == hit:
                assert same_bits(out[0, b:b + n], z[0, b:b + n]), (hit, "takes z")
            else:
                assert same_bits(out[0, b:b + n], blend[0, b:b + n]), (hit, b, "every other body as before")

    for b, n in BODIES:
        for col, gate in ((0, gate_pos), (1, gate_pos), (2, gate_vel), (3, gate_vel)):
            for sign in (1, -1):
                z = base_z.copy()
                z[0, b + col] = sign * gate  # exactly at the threshold: p is 0, |z - p| == gate: no trip
                at = T.update_rows(p, z, prm)
                assert not same_bits(at[0, b:b + n], z[0, b:b + n]) and at[0, b + col] != z[0, b + col], (b, col)
                z[0, b + col] = sign * np.nextafter(gate, F32(1.0))  # one unit in the last place beyond it
                only(z, b)
        off = T.update_rows(p, z, prm[:3] + (0.0, 0.0))  # a gate of 0 is off: the last z, far beyond both in vy
        assert not same_bits(off[0, b:b + n], z[0, b:b + n])
        if n == 7:  # the heading gate: c_p c_z + s_p s_z < 0
            z = base_z.copy()
            z[0, b + 4], z[0, b + 5] = 0.0, 1.0  # a right angle: the product is 0, no trip
            assert not same_bits(T.update_rows(p, z, prm)[0, b:b + n], z[0, b:b + n])
            z[0, b + 4] = -1e-6
            only(z, b)
            only_off = T.update_rows(p, z, prm[:3] + (0.0, 0.0))  # and it stays on with the other gates off
            assert same_bits(only_off[0, b:b + n], z[0, b:b + n])


def test_episode_edges_no_command_of_an_earlier_episode_is_ever_used():
    """§17.5's done patterns.  Own robot 0 of every row is measured at rest at the origin, heading +x, at every call,
    and call t's command is (c_t, c_t) with c_t = 0.1 * 2^t / 8192: small enough for the wheels to reach it within a
    substep, so a prediction's vx is 1.008 c of the command it used, whatever it started from, and with a gain of
    0.25 and the gates off the output's vx is 0.75 of it: it names the call.  Where the prediction is not advanced the
    output's vx is 0.75 of the state's."""
    calls, n, g = 12, 40, F32(0.25)
    dones = done_patterns(calls, n)
    code = (0.1 * (1 << np.arange(calls)) / 8192).astype(F32)
    obs = np.zeros((calls, 1, n, 1, 52), F32)
    obs[..., :] = rest_rows(1)[0]
    obs[..., 11] = obs[..., 12] = code[:, None, None, None]
    unit = 0.75 * 1.008 * 0.1 / 8192
    for D in (0, 1, 3):
        first = np.zeros(n, int)  # the call of each field's episode's first row
        advanced = 0
        for t, (o, x, age, hist, before) in enumerate(run(obs, obs.copy(), dones, D, (float(g), 0.0, 0.0, 0.0, 0.0))):
            if t == 0:
                continue
            adv = (t - first) > D  # D calls have passed since the episode's first: the age was saturated
            used = t - D            # the call whose command moves frame t - D - 1 to frame t - D
            vx = x[0, :, 0, 6].astype(np.float64)
            named = np.rint(vx / unit).astype(int)
            if adv.any():
                assert (named[adv] == 1 << used).all(), (D, t, named)
                assert (used > first[adv]).all(), (D, t)  # at least the episode's second call: none of an earlier episode
            held = before[0, :, 0, 6]
            assert same_bits(x[0, ~adv, 0, 6], held[~adv] + g * (F32(0.0) - held[~adv])), (D, t)  # P = est: no command at all
            fresh = dones[t] != 0
            assert same_bits(o[0, fresh, 0], obs[t][0, fresh, 0]) and same_bits(o[0, ~fresh, 0], x[0, ~fresh, 0]), (D, t)
            first = np.where(fresh, t, first)
            assert np.array_equal(age[0, :, 0], np.minimum(t - first, D)), (D, t)
            if D:
                assert same_bits(hist[t % D, 0, :, 0, :2], np.broadcast_to(code[t], (n, 2)))
            advanced += int(adv.sum())
        assert advanced > 0 and (D == 0 or advanced < (calls - 1) * n)


def test_one_world_the_three_rows_of_a_team_filter_each_entity_to_the_same_bits():
    n, D, calls = 32, 3, 12
    ball, robots = world(n, 20)
    g = np.random.default_rng(21)
    rows = []
    for t in range(calls):  # one world drifting a little with fresh commands, so bodies blend; a few jump through a gate
        ball = ball + g.normal(0, 0.002, ball.shape).astype(F32)
        robots = robots.copy()
        robots[..., :4] += g.normal(0, 0.002, robots[..., :4].shape).astype(F32)
        robots[..., 7:9] = g.uniform(-1, 1, robots[..., 7:9].shape)
        jump = g.random(robots.shape[:2]) < 0.1
        robots[jump, 0] += F32(0.3)
        rows.append(PC.full_rows(ball, robots).transpose(1, 0, 2, 3))
    rows = np.stack(rows)  # (calls, 2, n, 3, 52)
    dones = done_patterns(calls, n)
    blended = 0
    for t, (o, x, age, hist, _) in enumerate(run(rows, rows, dones, D, ON)):
        for out in (o,) if x is None else (o, x):
            for k in (1, 2):
                assert same_bits(out[:, :, k, 0:4], out[:, :, 0, 0:4]) and same_bits(out[:, :, k, 31:52], out[:, :, 0, 31:52]), (t, k)
                for e in range(3):  # robot e: own slot e of row 0, own slot (e - k) % 3 of row k
                    j = (e - k) % 3
                    assert same_bits(out[:, :, k, 4 + 9 * j:13 + 9 * j], out[:, :, 0, 4 + 9 * e:13 + 9 * e]), (t, k, e)
        if t:
            blended += int((x != rows[t]).any(-1).sum())
    assert blended > 1000


# ---- against the project's own physics -----------------------------------------------------------------------------------
# test_estimate_cpu.py's contact-free scenes: 256 fields, start + 4 steps, nobody near a neighbour or
# a wall.  Gains 0.2 / 0.5 / 0.5, the default gates, delays 0 and 2.  See DESIGN.md §22.5.
GAINS = (0.2, 0.5, 0.5, 0.03, 0.5)
TEAM = dict(position=[0, 1] + [b + i for b in E.OWN for i in (0, 1)], velocity=[2, 3] + [b + i for b in E.OWN for i in (2, 3)],
            heading=[b + i for b in E.OWN for i in (4, 5)], yaw_rate=[b + 6 for b in E.OWN])
THEIRS = dict(position=[b + i for b in E.OPPONENTS for i in (0, 1)], velocity=[b + i for b in E.OPPONENTS for i in (2, 3)],
              heading=[b + i for b in E.OPPONENTS for i in (4, 5)], yaw_rate=[b + 6 for b in E.OPPONENTS])
# Without noise, the largest distance of the filtered team bodies and ball from the measurement, measured here over the
# 256 fields x 5 calls x 6 rows and both delays, and the bounds: 4 x the maximum, rounded up to one significant digit
# (the prediction differs from the oracle's next frame by §19.5's rounding-level model error, and the update moves the
# output a share of that off the measurement).
#   class            measured    bound
#   position, m      5.96e-08    3e-07
#   velocity, m/s    3.58e-07    2e-06
#   heading (c, s)   4.17e-07    2e-06
#   yaw rate, rad/s  6.68e-06    3e-05
STAYS = dict(position=3e-7, velocity=2e-6, heading=2e-6, yaw_rate=3e-5)
# With the README example's vision noise (--obs-noise-pos 0.002, the other sigmas 0), seeds 1..4: the RMS error of the
# filtered team bodies' and ball's positions against the true delayed row over the raw perceived row's, measured here:
#   D = 0: 0.7433 0.7388 0.7393 0.7461      D = 2: 0.7433 0.7388 0.7393 0.7461
# The bound is the worst seed's ratio x 1.25 = 0.933, below 1.  The classes without noise have a raw error of exactly
# 0; there the filter must stay within STAYS of the truth (measured: the zero-noise figures above).
BENEFIT = 0.7461 * 1.25
SIGMAS = (0.002, 0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def truth():
    """The oracle's true FULL rows of the scenes, frame by frame -- computed once, shared, never written."""
    n = 256
    s, actions = scenes(n, 11)
    frames = [rows_of(s, np.zeros((n, 12), F32))]
    closest_pair, closest_wall = np.inf, np.inf
    for t in range(STEPS):
        O.simulate(s, np.ascontiguousarray(actions[t]))
        frames.append(rows_of(s, actions[t]))
        x = np.concatenate([s[O.CH_RX:O.CH_RX + 6], s[0:1]]).astype(np.float64)
        y = np.concatenate([s[O.CH_RY:O.CH_RY + 6], s[1:2]]).astype(np.float64)
        dist = np.hypot(x[:, None] - x[None], y[:, None] - y[None]) + 10 * np.eye(7)[:, :, None]
        radius = np.array([0.04] * 6 + [0.02134])[:, None]
        closest_pair = min(closest_pair, dist.min())
        closest_wall = min(closest_wall, (0.75 - np.abs(x) - radius).min(), (0.65 - np.abs(y) - radius).min())
    assert closest_pair >= 0.1 and closest_wall >= 0.05  # the condition: no case is left out
    for f in frames:
        f.setflags(write=False)
    return frames


def filtered(truth, D, sigmas, seed):
    """Per call: (the true delayed row, the raw perceived row, the filtered row)."""
    n = truth[0].shape[1]
    ring, p_age = np.zeros((D + 1,) + truth[0].shape, F32), np.zeros(n, np.int32)
    est, hist, age = state(truth[0].shape[:3], D)
    none = np.zeros(n, np.int64)
    out = []
    for t in range(STEPS + 1):
        start = t == 0
        seen, seen_t = PC.reference_perceive(truth[t], None if start else truth[t], none, ring, p_age, t, D, sigmas, seed)
        o, x = T.reference_track(seen, seen_t, none, est, hist, age, t, D, GAINS)
        assert (age == min(t, D)).all() and (start or same_bits(o, x)) and same_bits(o[..., ACTS], truth[t][..., ACTS])
        out.append((truth[max(t - D, 0)], seen, o))
    return out


def test_without_noise_the_filter_stays_on_the_measurement(truth):
    worst = dict.fromkeys(TEAM, 0.0)
    theirs = dict.fromkeys(TEAM, 0.0)
    for D in (0, 2):
        for true, seen, o in filtered(truth, D, (0, 0, 0, 0), 0):
            poses = [c for c in range(52) if c not in ACTS]  # (the own-action floats are the current call's)
            assert same_bits(seen[..., poses], true[..., poses])
            for name in TEAM:
                worst[name] = max(worst[name], float(np.abs(o[..., TEAM[name]].astype(np.float64) - seen[..., TEAM[name]]).max()))
                theirs[name] = max(theirs[name], float(np.abs(o[..., THEIRS[name]].astype(np.float64) - seen[..., THEIRS[name]]).max()))
    for name in TEAM:
        print(f"{name}: off the measurement by {worst[name]:.3g} (bound {STAYS[name]:g}); opponents (commands unknown, "
              f"reported only) {theirs[name]:.3g}")
    for name in TEAM:
        assert worst[name] <= STAYS[name], (name, worst[name])


def rms(parts):
    return float(np.sqrt(np.mean(np.concatenate([p.ravel() for p in parts]) ** 2)))


@pytest.mark.parametrize("D", [0, 2])
def test_with_noise_the_filtered_team_bodies_are_closer_to_the_truth_than_the_raw_row(truth, D):
    for seed in (1, 2, 3, 4):
        raw, fil = {k: [] for k in TEAM}, {k: [] for k in TEAM}
        raw_o, fil_o = {k: [] for k in TEAM}, {k: [] for k in TEAM}
        for true, seen, o in filtered(truth, D, SIGMAS, seed):
            for name in TEAM:
                raw[name].append(seen[..., TEAM[name]].astype(np.float64) - true[..., TEAM[name]])
                fil[name].append(o[..., TEAM[name]].astype(np.float64) - true[..., TEAM[name]])
                raw_o[name].append(seen[..., THEIRS[name]].astype(np.float64) - true[..., THEIRS[name]])
                fil_o[name].append(o[..., THEIRS[name]].astype(np.float64) - true[..., THEIRS[name]])
        ratio = rms(fil["position"]) / rms(raw["position"])
        print(f"D {D} seed {seed}: team and ball position RMS {rms(fil['position']):.3g} m filtered / {rms(raw['position']):.3g} m raw "
              f"= {ratio:.4f} (bound {BENEFIT:.4f}); opponents (reported only) "
              + ", ".join(f"{k} {rms(fil_o[k]):.3g} / {rms(raw_o[k]):.3g}" for k in TEAM))
        assert BENEFIT < 1.0 and ratio <= BENEFIT, (D, seed, ratio)
        for name in ("velocity", "heading", "yaw_rate"):  # no noise on these: raw is exact, the filter stays on it
            assert rms(raw[name]) == 0.0 and max(float(np.abs(p).max()) for p in fil[name]) <= STAYS[name], (D, seed, name)
