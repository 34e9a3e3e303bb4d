"""The actuation channel without a GPU (include/vss.h, vss_amd/actuate.py): its part of the
one ABI (1 function, 2 structs) and of the one library's source stamp, the entry's argument checks on
addresses that are never dereferenced, the float32 specification `reference_actuate` on known answers, the statistics
of its draws, and the flags' plumbing (parse_args, the checkpoint's structural keys)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ppo_continuous_action_isaacgym as P
from vss_amd import _native as N
from vss_amd import actuate as A
from vss_amd import checkpoint as CK
from vss_amd import cheader

F32 = np.float32
FAKE = 1 << 20  # non-null, 8-B aligned, never dereferenced: every call below returns before a launch
GAP = 1 << 24   # between two fake buffers: further apart than any extent used here
E_ARG = 1
ALL_ON = A.Params(0.05, 0.02, 0.03, 0.1, 127)


def call(n_fields=64, lay=(3, 0, 3, 1, 0), prm=(0.0, 0.0, 0.0, 0.0, 0), seed=1, call_index=0, cmd=FAKE, done=FAKE + GAP,
         done_stride=1, held=FAKE + 2 * GAP, gain=FAKE + 3 * GAP, episode=FAKE + 4 * GAP, out=FAKE + 5 * GAP,
         null_lay=False, null_prm=False):
    layout, params = A.VssActuateLayout(*lay), A.VssActuateParams(*prm)
    return N.load().vss_actuate(None, n_fields, None if null_lay else ctypes.byref(layout),
                                None if null_prm else ctypes.byref(params), seed, call_index, cmd, done, done_stride, held,
                                gain, episode, out)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def fresh_state(shape):
    return np.zeros(shape, F32), np.ones(shape, F32), np.zeros(shape[1], np.uint32)


def run(cmds, dones, params, seed=1, first_team=0, set_gain=None):
    """reference_actuate over the calls (call 0 is the start; dones[t] is done_prev of call t): the outputs and
    copies of held, gain and episode after every call.  set_gain: {call: array} written into gain before that call."""
    held, gain, episode = fresh_state(cmds.shape[1:])
    out = []
    for t in range(cmds.shape[0]):
        if set_gain and t in set_gain:
            gain[:] = set_gain[t]
        o = A.reference_actuate(cmds[t], None if t == 0 else dones[t], held, gain, episode, t, params, seed, first_team)
        out.append((o, held.copy(), gain.copy(), episode.copy()))
    return out


def done_patterns(calls, n):
    """done_prev per call: field 0 never; 1 at call 1; 2 on consecutive calls 4 and 5; 3 every call; 4 at calls 2 and
    7; further fields random.  Row 0 is not read (the start call)."""
    m = max(n, 5)
    d = np.zeros((calls, m), np.int64)
    d[1, 1] = 1
    d[4:6, 2] = 1
    d[1:, 3] = 1
    d[[c for c in (2, 7) if c < calls], 4] = 1
    d[1:, 5:] = np.random.default_rng(5).integers(0, 2, (calls - 1, m - 5))
    return np.ascontiguousarray(d[:, :n]) if n >= 5 else np.ascontiguousarray(d[:, [3, 2, 1, 4, 0][:n]])


# ---- the channel's part of the one ABI and the one library -------------------------------------------------------------
def exported(path, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(m.group(1) for m in re.finditer(rf"^\S+\s+T\s+({prefix}\w*)$", out, flags=re.M))


def test_the_header_declares_vss_actuate_and_its_two_structs_and_the_library_exports_it():
    with open(N.HEADER) as f:
        h = cheader.parse(f.read())
    assert [name for name in h.functions if "actuate" in name] == ["vss_actuate"] and "vss_actuate" in N.EXPORTED
    assert sorted(name for name in h.structs if "actuate" in name) == ["vss_actuate_layout", "vss_actuate_params"]
    assert {k: v for k, v in h.constants.items() if "ACTUATE" in k} == {"VSS_ACTUATE_MAX_LEVELS": 32767}
    assert A.MAX_LEVELS == 32767 == N.ACTUATE_MAX_LEVELS
    assert A.VssActuateLayout is N.VssActuateLayout and A.VssActuateParams is N.VssActuateParams
    assert ctypes.sizeof(A.VssActuateLayout) == 32 and ctypes.sizeof(A.VssActuateParams) == 20
    assert ctypes.sizeof(h.structs["vss_actuate_layout"]) == 32 and ctypes.sizeof(h.structs["vss_actuate_params"]) == 20
    assert N.load().vss_actuate.argtypes == h.functions["vss_actuate"][1]
    if shutil.which("nm"):
        assert exported(N.LIB_PATH, "vss_actuate") == ["vss_actuate"]
        assert exported(N.LIB_PATH, "vss_") == sorted(h.functions)


def test_the_unit_is_one_of_the_core_librarys_and_nothing_is_packaged_beside_it():
    assert [os.path.basename(p) for p in N.STAMPED].count("vss_actuate.hip") == 1
    assert os.path.join(N.CSRC, "vss_actuate.hip") in N.STAMPED
    assert [os.path.join(d, f) for d, _, files in os.walk(N.CSRC) for f in files if f == "Makefile" or f.endswith(".mk")] \
        == [os.path.join(N.CSRC, "Makefile")]
    for name in ("LIB_PATH", "STAMPED", "CSRC", "HEADER", "ABI", "EXPORTED", "ABI_VERSION", "source_hash", "verify_source_hash"):
        assert not hasattr(A, name), name
    assert A.load is N.load  # the module's own name for the one loader
    assert not os.path.exists(os.path.join(os.path.dirname(N.HEADER), "vss_actuate.h"))


def test_the_stamp_covers_the_makefiles_list_and_a_stale_library_is_refused_at_load(tmp_path, monkeypatch):
    """A library built before vss_actuate.hip was edited is refused, and the hash a state file records
    (checkpoint.source_hash is N.source_hash) changes with that edit."""
    with open(os.path.join(N.CSRC, "Makefile")) as f:
        (line,) = re.findall(r"^STAMPED\s*:=\s*(.*)$", f.read(), flags=re.M)
    assert "vss_actuate.hip:STEP_FLAGS" in line.split()
    at = list(N.STAMPED).index(os.path.join(N.CSRC, "vss_actuate.hip"))
    assert all(os.path.isfile(p) for p in N.STAMPED)
    lib = N.load()
    N.verify_source_hash(lib)
    with pytest.raises(N.NativeError, match="built from other sources"):
        N.verify_source_hash(lib, expected="0" * 16)
    before = N.source_hash()
    assert CK.source_hash() == before
    src = os.path.join(tmp_path, "vss_actuate.hip")
    shutil.copy(N.STAMPED[at], src)
    with open(src, "a") as f:
        f.write("// edited after the build\n")
    monkeypatch.setattr(N, "STAMPED", tuple(N.STAMPED[:at]) + (src,) + tuple(N.STAMPED[at + 1:]))
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(N.NativeError, match=r"built from other sources.*make -C"):
        N.load()
    assert N.source_hash() != before and CK.source_hash() == N.source_hash()


# ---- the entry's refusals ----------------------------------------------------------------------------------------------
def test_the_accepted_calls_and_null_pointers():
    assert call(n_fields=0) == 0
    assert call(n_fields=0, done=None) == 0
    assert call(n_fields=0, lay=(1, 0, 1, 1, 0)) == 0 and call(n_fields=0, lay=(3, 99, 3, 2, 1)) == 0
    assert call(n_fields=0, out=FAKE) == 0  # in place
    for bad in ("cmd", "held", "gain", "episode", "out"):
        assert call(**{bad: None}) == E_ARG, bad
        assert call(n_fields=0, **{bad: None}) == E_ARG, bad  # checked before the zero-size return
    assert call(null_lay=True) == E_ARG and call(null_prm=True) == E_ARG
    assert call(n_fields=0, null_lay=True) == E_ARG and call(n_fields=0, null_prm=True) == E_ARG


def test_misaligned_pointers_are_rejected():
    for name, base in dict(cmd=FAKE, out=FAKE + 5 * GAP, held=FAKE + 2 * GAP, gain=FAKE + 3 * GAP, done=FAKE + GAP).items():
        for off in (4, 1, 2, 7):
            assert call(**{name: base + off}) == E_ARG, (name, off)
    for off in (2, 1, 3):
        assert call(episode=FAKE + 4 * GAP + off) == E_ARG, off
    assert call(n_fields=0, episode=FAKE + 4 * GAP + 4) == 0 and call(n_fields=0, cmd=FAKE + 8) == 0


def test_overlapping_buffers_are_rejected():
    cmd, done, held, gain, episode, out = (FAKE + i * GAP for i in range(6))
    robot = 8  # bytes; 64 fields x 3 robots: 192 robots
    assert call(out=cmd + 191 * robot) == E_ARG and call(out=cmd - 191 * robot) == E_ARG  # partly on cmd
    for name in ("held", "gain", "episode"):
        for other in (cmd, done, out):
            assert call(**{name: other}) == E_ARG, (name, other)
            assert call(**{name: other + 8}) == E_ARG, (name, other)
    assert call(held=gain) == E_ARG and call(held=episode) == E_ARG and call(gain=episode) == E_ARG
    assert call(gain=held + 191 * robot) == E_ARG and call(episode=held + 191 * robot + 4) == E_ARG
    assert call(held=cmd - 191 * robot) == E_ARG and call(held=out + 191 * robot) == E_ARG
    assert call(episode=done + 63 * 8) == E_ARG and call(episode=done - 63 * 4) == E_ARG
    assert call(n_fields=0, held=gain) == E_ARG and call(n_fields=0, held=cmd) == E_ARG


def test_values_out_of_range_are_rejected():
    inf, nan = float("inf"), float("nan")
    bad = {0: (-1e-9, 0.31, 1.0, inf, nan), 1: (-1e-9, -1.0, inf, -inf, nan), 2: (-1e-9, 1.0001, inf, nan),
           3: (-1e-9, 1.0, 1.5, inf, nan)}
    for i, values in bad.items():
        for v in values:
            prm = [0.0, 0.0, 0.0, 0.0, 0]
            prm[i] = v
            assert call(prm=tuple(prm)) == E_ARG, (i, v)
    for levels in (-1, 32768, 1 << 30, -(1 << 31)):
        assert call(prm=(0.0, 0.0, 0.0, 0.0, levels)) == E_ARG, levels
    for robots in (0, 2, 4, -1):
        assert call(lay=(4, 0, robots, 1, 0)) == E_ARG, robots
    for teams in (0, 3, -1):
        assert call(lay=(3, 192, 3, teams, 0)) == E_ARG, teams
    for first in (-1, 2):
        assert call(lay=(3, 0, 3, 1, first)) == E_ARG, first
    for stride in (2, 0, -3):
        assert call(lay=(stride, 0, 3, 1, 0)) == E_ARG, stride
    assert call(lay=(0, 0, 1, 1, 0)) == E_ARG
    for team_stride in (191, 0, -192):  # two teams of 64 fields x 3 robots: a block spans 192
        assert call(lay=(3, team_stride, 3, 2, 0)) == E_ARG, team_stride
    for stride in (0, -1):
        assert call(done_stride=stride) == E_ARG, stride
        assert call(n_fields=0, done_stride=stride, done=None) == 0  # not read without done_prev
    assert call(n_fields=-1) == E_ARG
    # sizes that overflow the byte offsets, the field counter or the grid
    assert call(n_fields=1 << 60) == E_ARG
    assert call(n_fields=1 << 30, lay=(1 << 40, 0, 3, 1, 0)) == E_ARG
    assert call(n_fields=64, lay=(3, 1 << 62, 3, 2, 0)) == E_ARG
    assert call(n_fields=64, done_stride=1 << 62) == E_ARG
    assert call(n_fields=(1 << 31) * 70, lay=(1, 0, 1, 1, 0)) == E_ARG


def test_the_python_side_refuses_the_same_values():
    for bad in (A.Params(gain_sigma=0.31), A.Params(noise_sigma=-1.0), A.Params(deadband=1.5), A.Params(loss_prob=1.0),
                A.Params(levels=40000), A.Params(levels=-1), A.Params(gain_sigma=float("nan"))):
        with pytest.raises(ValueError, match="actuation"):
            bad.check()
    assert A.Params(0.3, 1.0, 1.0, 0.999, 32767).check()
    with pytest.raises(N.NativeError):
        A.ActuationChannel(4, A.layout_sa(), A.Params(), 0, "cpu")


# ---- reference_actuate: known answers -----------------------------------------------------------------------------------
def test_all_off_is_the_clamp_and_keeps_the_sign_of_zero():
    g = np.random.default_rng(3)
    cmds = g.uniform(-1.6, 1.6, (6, 2, 9, 3, 2)).astype(F32)
    cmds[:, 0, 0, 0, 0] = -0.0
    cmds[:, 0, 0, 0, 1] = 0.0
    cmds[:, 0, 1, 0] = (1.0, -1.0)
    dones = done_patterns(6, 9)
    for t, (o, held, gain, episode) in enumerate(run(cmds, dones, A.Params())):
        want = np.clip(cmds[t], -1, 1)
        assert same_bits(o, want) and same_bits(held, want), t
        assert np.signbit(o[0, 0, 0, 0]) and not np.signbit(o[0, 0, 0, 1])
        assert (gain == 1).all()
        assert (episode == 1 + (dones[1:t + 1] != 0).sum(0)).all(), t


def test_quantisation_gives_255_values_with_half_a_step_of_error_and_ties_to_even():
    u = np.linspace(-1.2, 1.2, 20001).astype(F32)
    cmd = np.broadcast_to(u[None, :, None, None], (1, u.size, 1, 2)).copy()
    held, gain, episode = fresh_state(cmd.shape)
    o = A.reference_actuate(cmd, None, held, gain, episode, 0, A.Params(levels=127), 1)
    values = np.unique(o)
    assert values.size == 255 and values[0] == -1 and values[-1] == 1
    assert np.array_equal(values, np.arange(-127, 128).astype(F32) / F32(127))  # (by value: unique keeps one of +-0)
    c = np.clip(u, -1, 1).astype(np.float64)
    assert np.abs(o[0, :, 0, 0].astype(np.float64) - c).max() <= 0.5 / 127 + 1e-7  # + the float32 rounding of k / 127
    # ties: levels 2 makes c * L exact; 0.25 -> 0.5 -> 0, 0.75 -> 1.5 -> 2 (to even, both ways)
    ties = np.array([0.25, 0.75, -0.25, -0.75, 0.5], F32)
    cmd = np.broadcast_to(ties[None, :, None, None], (1, 5, 1, 2)).copy()
    held, gain, episode = fresh_state(cmd.shape)
    o = A.reference_actuate(cmd, None, held, gain, episode, 0, A.Params(levels=2), 1)
    assert same_bits(o[0, :, 0, 0], np.array([0.0, 1.0, -0.0, -1.0, 0.5], F32))


def test_the_deadband_zeroes_only_what_lies_strictly_inside_it():
    b = F32(0.05)
    u = np.array([0.0, -0.0, 0.04, -0.04, np.nextafter(b, F32(0)), b, -b, np.nextafter(b, F32(1)), 0.5, -1.0], F32)
    cmd = np.broadcast_to(u[None, :, None, None], (1, u.size, 1, 2)).copy()
    held, gain, episode = fresh_state(cmd.shape)
    o = A.reference_actuate(cmd, None, held, gain, episode, 0, A.Params(deadband=float(b)), 1)
    want = np.where(np.abs(u) < b, F32(0.0), u)
    assert same_bits(o[0, :, 0, 0], want) and (want[:5] == 0).all() and not np.signbit(want[:5]).any()
    assert same_bits(o[0, 5:, 0, 0], u[5:])
    assert same_bits(held[0, :, 0, 0], u)  # the robot received the command; only the wheel did not move


def test_a_hand_set_gain_multiplies_and_lasts_until_the_next_episode():
    calls, n = 8, 3
    cmds = np.random.default_rng(1).uniform(-0.9, 0.9, (calls, 1, n, 3, 2)).astype(F32)
    dones = np.zeros((calls, n), np.int64)
    dones[5, 1] = 1  # field 1's episode ends with step 4: call 5 begins its next
    mine = np.random.default_rng(2).uniform(0.8, 1.2, (1, n, 3, 2)).astype(F32)
    res = run(cmds, dones, A.Params(gain_sigma=0.05), set_gain={2: mine})
    for t, (o, held, gain, episode) in enumerate(res):
        drawn = 1 + F32(0.05) * np.clip(A.episode_normals(1, np.arange(n), episode), -3, 3).reshape(1, n, 6, 2)[:, :, :3]
        if t < 2:
            want = drawn
        else:
            want = mine.copy()
            if t >= 5:
                want[0, 1] = drawn[0, 1]
        assert same_bits(gain, want.astype(F32)), t
        assert same_bits(o, cmds[t] * gain), t
    assert not same_bits(res[1][2], np.ones_like(mine)) and (np.abs(res[1][2] - 1) <= 0.15 + 1e-6).all()


def test_with_nearly_every_packet_lost_a_robot_rests_first_and_then_repeats_what_it_last_received():
    calls, n = 40, 64
    cmds = np.random.default_rng(4).uniform(-1, 1, (calls, 2, n, 3, 2)).astype(F32)
    dones = np.zeros((calls, n), np.int64)
    dones[20, ::2] = 1
    for p in (float(np.nextafter(F32(1.0), F32(0))), 0.9):
        res = run(cmds, dones, A.Params(loss_prob=p))
        lost = np.stack([A.loss_uniforms(1, np.arange(n), t) < F32(p) for t in range(calls)])  # (calls, n, 2)
        assert lost.mean() > (0.999 if p > 0.9 else 0.85) and (p > 0.9 or not lost.all())
        last = np.zeros((2, n, 3, 2), F32)
        for t, (o, held, _, _) in enumerate(res):
            if t == 20:
                last[:, ::2] = 0  # the new episode begins at rest
            got = ~lost[t].T[:, :, None, None]
            last = np.where(got, cmds[t], last)
            assert same_bits(o, last) and same_bits(held, last), (p, t)
        assert (res[0][0][lost[0].T] == 0).all() and (res[20][0][:, ::2][lost[20, ::2].T] == 0).all()
        # both wheels of all three robots of a team share the packet
        assert all((np.ptp((o == c).reshape(2, n, 6).astype(int), axis=2) == 0).all() for (o, _, _, _), c in zip(res, cmds))


def test_no_float_of_an_earlier_episode_is_applied():
    """Every command carries its episode's number; with every packet but a few lost and the gains pinned to 1 the
    applied command is the current episode's number or 0 (at rest), never an earlier episode's."""
    calls, n = 12, 40
    dones = done_patterns(calls, n)
    number = 1 + np.concatenate([np.zeros((1, n), int), np.cumsum(dones[1:] != 0, 0)])  # of the episode at call t
    cmds = np.broadcast_to((number / 16.0).astype(F32)[:, None, :, None, None], (calls, 2, n, 3, 2)).copy()
    for p in (0.5, 0.9):
        for t, (o, held, gain, episode) in enumerate(run(cmds, dones, A.Params(loss_prob=p), seed=9)):
            assert (episode == number[t]).all(), t
            ok = (o == cmds[t]) | (o == 0)
            assert ok.all() and same_bits(o, held), (p, t)
            lost = (A.loss_uniforms(9, np.arange(n), t) < F32(p)).T[:, :, None, None]
            first = (np.ones(n, bool) if t == 0 else dones[t] != 0)[None, :, None, None]
            assert (o[np.broadcast_to(lost & first, o.shape)] == 0).all()  # lost on an episode's first step: at rest
            assert same_bits(np.where(lost, 0, o), np.where(lost, 0, cmds[t])), (p, t)


def test_a_zero_parameter_leaves_the_other_effects_as_they_are():
    calls, n = 6, 33
    g = np.random.default_rng(8)
    cmds = g.uniform(-1.3, 1.3, (calls, 2, n, 3, 2)).astype(F32)
    dones = done_patterns(calls, n)
    full = run(cmds, dones, ALL_ON, seed=7)
    assert not same_bits(full[-1][0], np.clip(cmds[-1], -1, 1))
    # without the additive noise: the same received commands and gains, out = deadband(r) * G exactly
    quiet = run(cmds, dones, ALL_ON._replace(noise_sigma=0.0), seed=7)
    for t in range(calls):
        assert same_bits(quiet[t][1], full[t][1]) and same_bits(quiet[t][2], full[t][2]), t
        zn = A.step_normals(7, np.arange(n), t).reshape(n, 2, 3, 2).transpose(1, 0, 2, 3)
        assert same_bits(quiet[t][0] + F32(0.02) * zn, full[t][0]), t
    # without the gains: G = 1, the received commands as before
    plain = run(cmds, dones, ALL_ON._replace(gain_sigma=0.0), seed=7)
    for t in range(calls):
        assert same_bits(plain[t][1], full[t][1]) and (plain[t][2] == 1).all(), t
    # without loss: the same gains; without quantisation or deadband: the same gains and the same lost packets
    for off in (dict(loss_prob=0.0), dict(levels=0), dict(deadband=0.0)):
        other = run(cmds, dones, ALL_ON._replace(**off), seed=7)
        for t in range(calls):
            assert same_bits(other[t][2], full[t][2]), (off, t)
    no_loss = run(cmds, dones, ALL_ON._replace(loss_prob=0.0), seed=7)
    lost = np.stack([A.loss_uniforms(7, np.arange(n), t) < F32(0.1) for t in range(calls)])
    for t in range(calls):
        kept = ~lost[t].T
        assert same_bits(no_loss[t][0][kept], full[t][0][kept]), t
    # one world: a yellow-first channel draws yellow's entities -- block 1 of the two-team run
    yellow = run(cmds[:, 1:], dones, ALL_ON, seed=7, first_team=1)
    for t in range(calls):
        assert same_bits(yellow[t][0][0], full[t][0][1]) and same_bits(yellow[t][2][0], full[t][2][1]), t


# ---- the draws' statistics (seed 1, 4,096 fields; bounds: 4 standard errors) --------------------------------------------
def test_the_step_normals_are_standard_normal_within_four_standard_errors():
    n = 4096
    z = A.step_normals(1, np.arange(n), 0)
    assert z.shape == (n, 12) and z.dtype == F32 and np.isfinite(z).all()
    z64 = z.astype(np.float64)
    m = n * 12
    print("pooled mean", z64.mean(), "std - 1", z64.std() - 1, "worst per-index mean", np.abs(z64.mean(0)).max() * np.sqrt(n), "se")
    assert abs(z64.mean()) <= 4 / np.sqrt(m)               # 0.0180
    assert abs(z64.std() - 1) <= 4 / np.sqrt(2 * m)        # 0.0128
    assert np.abs(z64.mean(0)).max() <= 4 / np.sqrt(n)     # 0.0625 per index
    assert same_bits(A.step_normals(1, [5, 4095], 0), z[[5, 4095]])
    assert not same_bits(A.step_normals(1, np.arange(8), 1), z[:8]) and not same_bits(A.step_normals(2, np.arange(8), 0), z[:8])
    # purposes apart: the episode's draws at the same counter word are others, and neither are perception's
    from vss_amd.perceive import unit_normals
    assert not same_bits(A.episode_normals(1, np.arange(8), 0), z[:8])
    assert not same_bits(unit_normals(1, np.arange(8), 0)[:, :12], z[:8])


def test_the_gain_normals_tail_and_the_loss_rate():
    n = 4096
    zg = A.episode_normals(1, np.arange(n), 1).astype(np.float64)
    share, expect = (np.abs(zg) > 3).mean(), 0.0026998
    print("share of |z| > 3", share)
    assert abs(share - expect) <= 4 * np.sqrt(expect * (1 - expect) / zg.size)
    p = 0.1
    lost = np.stack([A.loss_uniforms(1, np.arange(n), t) < F32(p) for t in range(16)])  # (16, n, 2)
    se = np.sqrt(p * (1 - p) / n)
    print("pooled loss", lost.mean(), "worst cell", np.abs(lost.mean(1) - p).max() / se, "se")
    assert abs(lost.mean() - p) <= 4 * se / np.sqrt(32)    # 0.0033
    assert np.abs(lost.mean(1) - p).max() <= 4 * se         # 0.0188
    u = A.loss_uniforms(1, np.arange(n), 0)
    assert u.dtype == F32 and (u >= 0).all() and (u < 1).all()


# ---- plumbing -------------------------------------------------------------------------------------------------------
def test_the_flags_default_to_zero_and_are_structural():
    from envs.wrappers import actuation_args, actuation_seed, perception_seed
    a = P.parse_args([])
    assert (a.act_gain, a.act_noise, a.act_levels, a.act_deadband, a.act_loss) == (0.0, 0.0, 0, 0.0, 0.0)
    assert not actuation_args(a).any() and actuation_args(a) == A.Params()
    flags = ["--act-gain", "0.05", "--act-noise", "0.02", "--act-levels", "127", "--act-deadband", "0.03", "--act-loss", "0.1"]
    b = P.parse_args(flags)
    assert actuation_args(b) == ALL_ON
    assert actuation_seed(1) != actuation_seed(2) and len({actuation_seed(1), actuation_seed(1, 1), actuation_seed(1, 2)}) == 3
    assert actuation_seed(1) != perception_seed(1)
    assert CK.ACTUATION_STRUCTURAL == ("act_gain", "act_noise", "act_levels", "act_deadband", "act_loss")
    assert CK.PERCEPTION_STRUCTURAL == ("obs_delay", "obs_noise_pos", "obs_noise_vel", "obs_noise_ang", "obs_noise_angvel")
    with pytest.raises(ValueError, match="act_levels"):
        CK.check_compatible(vars(b), P.parse_args(flags[:5] + ["63"] + flags[6:]), log=None)
    with pytest.raises(ValueError, match="act_loss"):
        CK.check_compatible(vars(a), P.parse_args(["--act-loss", "0.01"]), log=None)
    old = {k: v for k, v in vars(a).items() if not k.startswith("act_")}  # a state file from before the flags
    assert CK.check_compatible(old, a, log=None) is not None
    with pytest.raises(ValueError, match="act_gain"):
        CK.check_compatible(old, b, log=None)


def test_the_layouts_of_the_wrappers():
    assert A.layout_sa() == (1, 0, 1, 1, 0) and A.layout_team() == (3, 0, 3, 1, 0)
    assert A.layout_mirror(3, 100) == (3, 300, 3, 2, 0) and A.layout_mirror(1, 100) == (1, 100, 1, 2, 0)
    assert A.layout_opponent() == (3, 0, 3, 1, 1) and A.layout_full_blue() == (6, 0, 3, 1, 0)
    assert A.layout_mirror(3, 100).span(100) == 600 and A.layout_full_blue().span(100) == 597
    idx = A.layout_mirror(3, 4).index(4)
    assert idx.shape == (2, 4, 3) and idx[1, 2, 1] == 12 + 6 + 1
