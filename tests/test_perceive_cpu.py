"""The perception channel without a GPU (include/vss.h vss_perceive, vss_amd/perceive.py): the ABI
entry's argument checks on addresses that are never dereferenced, the float32 specification `reference_perceive`
on known answers (identity, pure delay, the done edge cases, one world for all six rows), the statistics of its
draws, and the flags' plumbing (parse_args, the checkpoint's structural keys)."""
import ctypes
import re

import numpy as np
import pytest

import ppo_continuous_action_isaacgym as P
from vss_amd import _native as N
from vss_amd import checkpoint as CK
from vss_amd import perceive as PC

F32 = np.float32
FAKE = 1 << 20  # non-null, 16-B aligned, never dereferenced: every call below returns before a launch
GAP = 1 << 24   # between two fake buffers: further apart than any extent used here
E_ARG = 1
ACTS = list(PC.ACTION_FLOATS)
ALL_ON = PC.Noise(0.002, 0.01, 0.02, 0.1)


def call(n_fields=64, lay=(3, 0, 3, 1, 0), delay=2, noise=(0.0, 0.0, 0.0, 0.0), seed=1, call_index=0, obs=FAKE,
         term=FAKE + GAP, done=FAKE + 2 * GAP, done_stride=1, ring=FAKE + 3 * GAP, age=FAKE + 5 * GAP,
         obs_out=FAKE + 6 * GAP, term_out=FAKE + 7 * GAP, null_lay=False, null_noise=False):
    layout, sig = N.VssPerceiveLayout(*lay), N.VssPerceiveNoise(*noise)
    return N.load().vss_perceive(None, n_fields, None if null_lay else ctypes.byref(layout), delay,
                                 None if null_noise else ctypes.byref(sig), seed, call_index, obs, term, done, done_stride,
                                 ring, age, obs_out, term_out)


def world(n, seed):
    """A consistent world: (ball (n, 4), robots (n, 6, 9)) with unit headings and commands in [-1, 1]."""
    g = np.random.default_rng(seed)
    ball = np.concatenate([g.uniform(-0.7, 0.7, (n, 2)), g.uniform(-1.5, 1.5, (n, 2))], 1).astype(F32)
    yaw = g.uniform(-np.pi, np.pi, (n, 6))
    robots = np.concatenate([g.uniform(-0.7, 0.7, (n, 6, 2)), g.uniform(-1.5, 1.5, (n, 6, 2)), np.cos(yaw)[..., None],
                             np.sin(yaw)[..., None], g.uniform(-20, 20, (n, 6, 1)), g.uniform(-1, 1, (n, 6, 2))], 2)
    return ball, robots.astype(F32)


def frames(n, calls, seed, teams=1, robots=3):
    """Distinct random true rows per call, packed (calls, teams, n, robots, 52), and terminal rows alike."""
    g = np.random.default_rng(seed)
    shape = (calls, teams, n, robots, 52)
    return g.standard_normal(shape).astype(F32), g.standard_normal(shape).astype(F32)


def run(obs, term, dones, delay, noise=(0, 0, 0, 0), seed=1, first_team=0):
    """reference_perceive over the calls: call 0 is the start; returns the outputs, ages and rings per call."""
    calls, shape = obs.shape[0], obs.shape[1:]
    ring, age = np.zeros((delay + 1,) + shape, F32), np.zeros(shape[1], np.int32)
    out = []
    for t in range(calls):
        o, x = PC.reference_perceive(obs[t], None if t == 0 else term[t], None if t == 0 else dones[t], ring, age, t,
                                     delay, noise, seed, first_team)
        out.append((o, x, age.copy(), ring.copy()))
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def test_the_symbol_is_exported_and_declared_and_the_abi_version_stays():
    assert "vss_perceive" in N.EXPORTED
    header = open(N.HEADER).read()
    assert re.search(r"\bint\s+vss_perceive\s*\(", header)
    assert re.search(r"#define\s+VSS_PERCEIVE_MAX_DELAY\s+15\b", header)
    assert N.load().vss_abi_version() == 2 == N.ABI_VERSION
    assert PC.MAX_DELAY == 15
    assert any(p.endswith("vss_perceive.hip") for p in N.STAMPED)


def test_the_accepted_call_of_no_fields_and_null_pointers():
    assert call(n_fields=0) == 0
    assert call(n_fields=0, term=None, term_out=None) == 0
    assert call(n_fields=0, lay=(1, 0, 1, 1, 0)) == 0 and call(n_fields=0, lay=(3, 99, 3, 2, 1)) == 0
    for bad in ("obs", "done", "ring", "age", "obs_out"):
        assert call(**{bad: None}) == E_ARG, bad
        assert call(n_fields=0, **{bad: None}) == E_ARG, bad  # checked before the zero-size return
    assert call(null_lay=True) == E_ARG and call(null_noise=True) == E_ARG
    assert call(term=None) == E_ARG and call(term_out=None) == E_ARG  # exactly one of the two


def test_misaligned_pointers_are_rejected():
    rows = dict(obs=FAKE, term=FAKE + GAP, ring=FAKE + 3 * GAP, obs_out=FAKE + 6 * GAP, term_out=FAKE + 7 * GAP)
    for name, base in rows.items():
        for off in (4, 8, 12, 1):
            assert call(**{name: base + off}) == E_ARG, (name, off)
    for off in (4, 2, 1):
        assert call(done=FAKE + 2 * GAP + off) == E_ARG, off
    for off in (2, 1, 3):
        assert call(age=FAKE + 5 * GAP + off) == E_ARG, off
    assert call(done=FAKE + 2 * GAP + 8, n_fields=0) == 0 and call(age=FAKE + 5 * GAP + 4, n_fields=0) == 0


def test_an_output_aliasing_an_input_is_rejected():
    obs, term = FAKE, FAKE + GAP
    row = 52 * 4
    assert call(obs_out=obs) == E_ARG and call(obs_out=term) == E_ARG
    assert call(term_out=obs) == E_ARG and call(term_out=term) == E_ARG
    assert call(term_out=FAKE + 6 * GAP) == E_ARG  # the two outputs on each other
    assert call(ring=obs) == E_ARG and call(ring=FAKE + 6 * GAP) == E_ARG
    # overlapping ranges, not only equal addresses: 64 fields x 3 rows
    assert call(obs_out=obs + 191 * row) == E_ARG and call(obs_out=obs - 191 * row) == E_ARG
    assert call(n_fields=0, obs_out=obs) == E_ARG


def test_values_out_of_range_are_rejected():
    for delay in (-1, 16, 100):
        assert call(delay=delay) == E_ARG, delay
    for i in range(4):
        for bad in (-1e-9, -1.0, float("inf"), float("nan")):
            noise = [0.0] * 4
            noise[i] = bad
            assert call(noise=tuple(noise)) == E_ARG, (i, bad)
    for robots in (0, 2, 4, -1):
        assert call(lay=(4, 0, robots, 1, 0)) == E_ARG, robots
    for teams in (0, 3, -1):
        assert call(lay=(3, 192, 3, teams, 0)) == E_ARG, teams
    for first in (-1, 2):
        assert call(lay=(3, 0, 3, 1, first)) == E_ARG, first
    for stride in (2, 0, -3):
        assert call(lay=(stride, 0, 3, 1, 0)) == E_ARG, stride
    assert call(lay=(0, 0, 1, 1, 0)) == E_ARG
    for team_stride in (191, 0, -192):  # two teams of 64 fields x 3 rows: a block spans 192 rows
        assert call(lay=(3, team_stride, 3, 2, 0)) == E_ARG, team_stride
    for stride in (0, -1):
        assert call(done_stride=stride) == E_ARG, stride
    assert call(n_fields=-1) == E_ARG
    # sizes that overflow the byte offsets or the grid
    assert call(n_fields=1 << 60) == E_ARG
    assert call(n_fields=1 << 40, lay=(1 << 30, 0, 3, 1, 0)) == E_ARG
    assert call(n_fields=64, lay=(3, 1 << 62, 3, 2, 0)) == E_ARG
    assert call(n_fields=(1 << 31) * 70, lay=(1, 0, 1, 1, 0)) == E_ARG


# ---- reference_perceive: known answers ---------------------------------------------------------------------------
def test_identity_delay_zero_and_no_noise_reproduces_the_inputs():
    obs, term = frames(7, 5, 3, teams=2)
    dones = np.random.default_rng(0).integers(0, 2, (5, 7))
    for t, (o, x, age, ring) in enumerate(run(obs, term, dones, 0)):
        assert same_bits(o, obs[t]) and (age == 0).all() and same_bits(ring[0], obs[t])
        assert (x is None) if t == 0 else same_bits(x, term[t])


def done_patterns(calls, n):
    """Fields 0..5: never done; done at the start's next call; done on two consecutive calls; done exactly when the
    age reaches D = 3 (and once more later); done every call; done at calls 2 and 5 (younger than D both times).
    Further fields: random.  Fewer than six fields take patterns 3, 2, 1, 4, 5 first."""
    m = max(n, 6)
    d = np.zeros((calls, m), np.int64)
    d[1, 1] = 1
    d[4:6, 2] = 1
    d[3, 3] = 1   # age 1, 2, then the call at which it would reach 3
    d[7, 3] = 1
    d[1:, 4] = 1
    d[[2, 5], 5] = 1
    d[1:, 6:] = np.random.default_rng(5).integers(0, 2, (calls - 1, m - 6))
    return d[:, :n] if n >= 6 else np.ascontiguousarray(d[:, [3, 2, 1, 4, 5][:n]])


def test_pure_delay_gives_the_frame_of_min_age_d_steps_ago_with_the_current_actions():
    D, calls, n = 3, 12, 9
    obs, term = frames(n, calls, 4)
    dones = done_patterns(calls, n)
    birth = np.zeros(n, int)  # the call whose obs is the first frame of the field's episode
    for t, (o, x, age, _) in enumerate(run(obs, term, dones, D)):
        if t > 0:
            # the terminal row belongs to the episode that may just have ended
            d_term = np.minimum(t - birth, D)
            for f in range(n):
                want = obs[t - d_term[f], 0, f].copy()
                want[:, ACTS] = term[t, 0, f][:, ACTS]
                assert same_bits(x[0, f], want), (t, f)
            birth = np.where(dones[t] != 0, t, birth)
        a = np.minimum(t - birth, D)
        assert (age == a).all(), t
        for f in range(n):
            want = obs[t - a[f], 0, f].copy()
            want[:, ACTS] = obs[t, 0, f][:, ACTS]
            assert same_bits(o[0, f], want), (t, f)


def test_no_float_of_the_previous_episode_is_ever_perceived():
    """Every frame carries its episode's number in all 52 floats: the perceived row shows the current episode's only
    (the six own-action floats are the current row's anyway), the terminal row the ending episode's only."""
    D, calls, n = 3, 12, 40
    dones = done_patterns(calls, n)
    episode = np.concatenate([np.zeros((1, n), int), np.cumsum(dones[1:] != 0, 0)])  # of the frame obs[t]
    obs = np.broadcast_to(episode[:, None, :, None, None].astype(F32), (calls, 2, n, 3, 52)).copy()
    term = obs.copy()
    term[1:] = np.broadcast_to((episode[1:] - (dones[1:] != 0))[:, None, :, None, None], term[1:].shape)  # pre-reset
    for t, (o, x, _, _) in enumerate(run(obs, term, dones, D)):
        assert same_bits(o, obs[t]), t
        if t > 0:
            assert same_bits(x, term[t]), t


def test_one_world_every_row_of_a_field_sees_the_same_noisy_entities():
    n = 64
    ball, robots = world(n, 8)
    rows = PC.full_rows(ball, robots).transpose(1, 0, 2, 3)  # (2, n, 3, 52): team-major blocks
    ring, age = np.zeros((3,) + rows.shape, F32), np.zeros(n, np.int32)
    o, _ = PC.reference_perceive(rows, None, None, ring, age, 0, 2, ALL_ON, 11)
    assert not same_bits(o, rows)
    blue, yellow = o[0], o[1]
    for k in range(3):
        assert same_bits(blue[:, k, 0:4], blue[:, 0, 0:4]) and same_bits(yellow[:, k, 0:4], -blue[:, 0, 0:4])
    flip = np.array([-1, -1, -1, -1, -1, -1, 1], F32)
    for e in range(6):  # the entity's seven pose floats in the blue frame, from each of the six rows
        team, r = divmod(e, 3)
        seen = []
        for t, block in ((0, blue), (1, yellow)):
            for k in range(3):
                at = 4 + 9 * ((r - k) % 3) if t == team else 31 + 7 * r
                v = block[:, k, at:at + 7]
                seen.append(v * flip if t else v)
        for v in seen[1:]:
            assert same_bits(v, seen[0]), e
        true = robots[:, e, :7]
        assert np.abs(seen[0][:, :2] - true[:, :2]).max() < 6 * 0.002 and np.abs(seen[0][:, :2] - true[:, :2]).max() > 0
    # and the perceived world is again a consistent one: full_rows of the perceived entities gives the same rows
    pball = blue[:, 0, 0:4]
    probots = robots.copy()
    for e in range(3):
        probots[:, e, :7] = blue[:, 0, 4 + 9 * e:11 + 9 * e]
        probots[:, 3 + e, :7] = blue[:, 0, 31 + 7 * e:38 + 7 * e]
    assert same_bits(PC.full_rows(pball, probots).transpose(1, 0, 2, 3), o)


def test_the_unit_normals_are_standard_normal_within_four_standard_errors():
    z = PC.unit_normals(1, np.arange(4096), 0)
    assert z.shape == (4096, 40) and z.dtype == F32 and np.isfinite(z).all()
    z64 = z.astype(np.float64)
    print("pooled mean", z64.mean(), "std - 1", z64.std() - 1, "max |z|", np.abs(z64).max())
    per = np.maximum(np.abs(z64.mean(0)) / 0.015625, np.abs(z64.std(0) - 1) / (1 / np.sqrt(2 * 4096)))
    print("worst per-index value", per.max(), "standard errors")
    assert abs(z64.mean()) <= 0.0099 and abs(z64.std() - 1) <= 0.0070
    assert np.abs(z64.mean(0)).max() <= 0.0625 and np.abs(z64.std(0) - 1).max() <= 0.0442
    assert 4.0 < np.abs(z64).max() < 6.0
    # other fields, calls and seeds are other draws; the same triple is the same draw
    assert same_bits(PC.unit_normals(1, [5, 4095], 0), z[[5, 4095]])
    assert not same_bits(PC.unit_normals(1, np.arange(8), 1), z[:8])
    assert not same_bits(PC.unit_normals(2, np.arange(8), 0), z[:8])
    assert not same_bits(PC.unit_normals(1 << 32, np.arange(8), 0), PC.unit_normals(0, np.arange(8), 0))


def class_columns():
    """The floats of a row by noise class: positions, velocities, headings (cos, sin), yaw rates; and the rest."""
    pos, vel, ang, angvel = [0, 1], [2, 3], [], []
    for b in [4 + 9 * j for j in range(3)] + [31 + 7 * j for j in range(3)]:
        pos += [b, b + 1]
        vel += [b + 2, b + 3]
        ang += [b + 4, b + 5]
        angvel += [b + 6]
    return dict(pos=pos, vel=vel, ang=ang, angvel=angvel)


def test_a_zero_sigma_leaves_its_class_untouched_and_the_others_as_they_were():
    n = 33
    ball, robots = world(n, 21)
    robots[0, 0, 0] = -0.0  # x + 0 would turn this into +0: a skipped class copies it
    rows = PC.full_rows(ball, robots).transpose(1, 0, 2, 3)
    cols = class_columns()
    assert sorted(sum(cols.values(), []) + ACTS) == list(range(52))

    def out(noise):
        ring, age = np.zeros((1,) + rows.shape, F32), np.zeros(n, np.int32)
        return PC.reference_perceive(rows, None, None, ring, age, 3, 0, noise, 7)[0]

    full = out(ALL_ON)
    for name, c in cols.items():
        assert not same_bits(full[..., c], rows[..., c]), name
    assert same_bits(full[..., ACTS], rows[..., ACTS])
    for i, name in enumerate(cols):
        only = out(PC.Noise(*[s if j == i else 0.0 for j, s in enumerate(ALL_ON)]))
        without = out(PC.Noise(*[0.0 if j == i else s for j, s in enumerate(ALL_ON)]))
        for other, c in cols.items():
            assert same_bits(only[..., c], full[..., c] if other == name else rows[..., c]), (name, other)
            assert same_bits(without[..., c], rows[..., c] if other == name else full[..., c]), (name, other)


# ---- plumbing -----------------------------------------------------------------------------------------------------
def test_the_flags_default_to_zero_and_are_structural():
    a = P.parse_args([])
    assert (a.obs_delay, a.obs_noise_pos, a.obs_noise_vel, a.obs_noise_ang, a.obs_noise_angvel) == (0, 0.0, 0.0, 0.0, 0.0)
    from envs.wrappers import perception_args, perception_seed
    delay, noise = perception_args(a)
    assert delay == 0 and not noise.any()
    b = P.parse_args(["--obs-delay", "2", "--obs-noise-pos", "0.002", "--obs-noise-ang", "0.02"])
    assert perception_args(b) == (2, PC.Noise(0.002, 0.0, 0.02, 0.0))
    assert perception_seed(1) != perception_seed(2) and perception_seed(1) != perception_seed(1, 1)
    assert CK.PERCEPTION_STRUCTURAL == ("obs_delay", "obs_noise_pos", "obs_noise_vel", "obs_noise_ang", "obs_noise_angvel")
    with pytest.raises(ValueError, match="obs_delay"):
        CK.check_compatible(vars(b), P.parse_args(["--obs-delay", "3", "--obs-noise-pos", "0.002", "--obs-noise-ang", "0.02"]),
                            log=None)
    with pytest.raises(ValueError, match="obs_noise_pos"):
        CK.check_compatible(vars(a), P.parse_args(["--obs-noise-pos", "0.001"]), log=None)
    old = {k: v for k, v in vars(a).items() if not k.startswith("obs_")}  # a state file from before the flags
    assert CK.check_compatible(old, a, log=None) is not None


def test_the_layouts_of_the_wrappers():
    assert PC.layout_sa() == (1, 0, 1, 1, 0) and PC.layout_dma() == (3, 0, 3, 1, 0)
    assert PC.layout_mirror(3, 100) == (3, 300, 3, 2, 0) and PC.layout_mirror(1, 100) == (1, 100, 1, 2, 0)
    assert PC.layout_opponent() == (3, 0, 3, 1, 1) and PC.layout_full_blue() == (6, 0, 3, 1, 0)
    assert PC.layout_mirror(3, 100).span(100) == 600 and PC.layout_full_blue().span(100) == 597
    idx = PC.layout_mirror(3, 4).row_index(4)
    assert idx.shape == (2, 4, 3) and idx[1, 2, 1] == 12 + 6 + 1
