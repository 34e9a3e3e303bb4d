"""The directed edge table (tests/step_edges.py) is sensitive: proven on the CPU with mutated oracles.

Each mutant is oracle/vss_oracle.c with ONE text replacement (the old text must occur exactly once, so an
edit of the oracle fails here loudly), compiled with the oracle Makefile's flags into a library of its own
in tmp_path and bound with a second ctypes.CDLL; `oracle._lib` is not touched.  For every mutant the cases
built for it (by tag) must differ from the real oracle in at least one bit of state, rewards, reset_buf,
time_outs, progress or observations over two steps, and every other case must agree on both, so a mutant
is caught by its own cases and by nothing else.

Equivalent mutants, listed and not asserted:
  * `fabsf(x) < 0.78f` -> `0.70f` in oracle_sincosf: between 0.70 and 0.78 the reduction takes k = 0,
    kf = 0 and r = (x - 0) - 0 = x, the same polynomial on the same argument.
  * inside-box `lx >= 0.0f` -> `> 0.0f`: that arm needs px < py, i.e. |lx| > |ly| >= 0, so lx != 0.
  * contact_walls `*x < 0.0f` -> `<= 0.0f`: differs only at x == +-0, where ax == 0 and the sign only
    decides between +0 and -0 products that the kernel and the oracle both leave as they come.
  * goal `fabsf(by) < O_GOAL_HY` -> `<=`: a ball cannot end a step at |y| == 0.2 past the goal line, the
    pocket's side face or the end wall (resolved last) moves it (step_edges.py's header).
  * corner `d > 1e-9f` in contact_walls: 0 < d <= 1e-9 is not reachable next to (0.75, 0.2) in float32.
  * pocket-side `ay <= O_GOAL_HY` -> `<` (the third of the issue's contact_walls list): at ay == 0.2f past the
    goal line the real oracle takes the side face, pen = fl(fl(0.2f + r) - 0.2f), the mutant the "inside the end
    wall" arm with py = fl(0 + r) = r and px > py always, so both set ay = fl(0.2f - pen) and zero avy > 0.
    The two pens differ by two units of r's last place for both radii the step uses (0.04f: 0.2f + r is a
    rounding tie; 0.02134f: it rounds up), and 0.2f - pen rounds both to the same float: 0.16f and 0.17866f
    lie in [0.125, 0.25), where the spacing is four times r's.  Nothing of x enters, so these two sums are
    the whole proof; the cases (wall/*/y_gy_pocket*) stay in the table for the kernel.
"""
import ctypes
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as O
import step_edges as E

ORACLE_DIR = os.path.dirname(os.path.abspath(O.__file__))
STEPS = 2

# (id, old text, new text, tags of the cases built for it).  The first 14 are the survivors of the
# parity suite's inputs that a case can tell apart (13: see above); the rest are one per further threshold the table claims.
MUTANTS = [
    ("walls_ax_le_hx", "if (ax <= O_FIELD_HX) {", "if (ax < O_FIELD_HX) {", {"ax_le_hx"}),
    ("walls_ay_le_gy_field", "if (ay <= O_GOAL_HY) { /* near the goal post corner (0.75, 0.2) */",
     "if (ay < O_GOAL_HY) { /* near the goal post corner (0.75, 0.2) */", {"ay_le_gy_field", "ax_le_hx"}),
    ("walls_px_lt_py", "if (px < py) { ax = ax - px;", "if (px <= py) { ax = ax - px;", {"wall_px_py"}),
    ("walls_corner_lt", "if (d2 < r * r) {", "if (d2 <= r * r) {", {"corner_lt"}),
    ("walls_corner_default", "float nx = -1.0f, ny = 0.0f;", "float nx = 0.0f, ny = -1.0f;", {"corner_default"}),
    ("rr_lt", "if (!(d2 < O_RR_DIST2)) return;", "if (!(d2 <= O_RR_DIST2)) return;", {"rr_lt"}),
    ("rr_default", "float nx = 1.0f, ny = 0.0f;", "float nx = 0.0f, ny = 1.0f;", {"rr_default", "rr_tiny"}),
    ("br_lt", "if (!(d2 < O_BALL_R2)) return;", "if (!(d2 <= O_BALL_R2)) return;", {"br_lt"}),
    ("br_px_lt_py", "if (px < py) { nlx =", "if (px <= py) { nlx =", {"br_px_py"}),
    ("br_ly_ge0", "nly = ly >= 0.0f ? 1.0f : -1.0f;", "nly = ly > 0.0f ? 1.0f : -1.0f;", {"br_ly_ge0"}),
    ("sincos_k2", "default: *s = -sr; *c = -cr; break; /* k = +-2 */", "default: *s = sr; *c = cr; break; /* k = +-2 */",
     {"sincos_k2"}),
    ("reset_rounds", "#define O_MAX_REJECT_ROUNDS 64", "#define O_MAX_REJECT_ROUNDS 8", {"reset_rounds"}),
    ("reset_lt", "< O_MIN_DIST) return 1;", "<= O_MIN_DIST) return 1;", {"reset_lt"}),
    # further thresholds
    ("rr_tiny", "if (d > 1e-9f) { float inv = 1.0f / d; nx = dx * inv; ny = dy * inv; }\n  float half",
     "if (d > 1e-10f) { float inv = 1.0f / d; nx = dx * inv; ny = dy * inv; }\n  float half", {"rr_tiny"}),
    ("goal_rew_gt", "int is_goal = (fabsf(bx) > O_FIELD_HX) && (fabsf(by) < O_GOAL_HY);\n  if (is_goal && bx > 0.0f)",
     "int is_goal = (fabsf(bx) >= O_FIELD_HX) && (fabsf(by) < O_GOAL_HY);\n  if (is_goal && bx > 0.0f)", {"goal_gt"}),
    ("goal_done_gt", "int is_goal = (fabsf(bx) > O_FIELD_HX) && (fabsf(by) < O_GOAL_HY);\n    st->reset_buf",
     "int is_goal = (fabsf(bx) >= O_FIELD_HX) && (fabsf(by) < O_GOAL_HY);\n    st->reset_buf", {"goal_gt"}),
    ("done_ge", "st->progress_buf[f] >= (int64_t)p->max_episode_length) ? 1 : 0;",
     "st->progress_buf[f] > (int64_t)p->max_episode_length) ? 1 : 0;", {"done_ge"}),
    ("timeout_ge", "(st->progress_buf[f] >= (int64_t)p->max_episode_length - 1) && done != 0",
     "(st->progress_buf[f] > (int64_t)p->max_episode_length - 1) && done != 0", {"timeout_ge"}),
    ("side_pen", "O_FIELD_HY; if (pen > 0.0f)", "O_FIELD_HY; if (pen >= 0.0f)", {"side_pen"}),
    ("back_pen", "O_GOAL_BACK_X; if (pen > 0.0f)", "O_GOAL_BACK_X; if (pen >= 0.0f)", {"back_pen"}),
    ("end_pen", "float pen = ax + r - O_FIELD_HX;\n      if (pen > 0.0f)", "float pen = ax + r - O_FIELD_HX;\n      if (pen >= 0.0f)",
     {"end_pen"}),
    ("pocket_pen", "float pen = ay + r - O_GOAL_HY;\n      if (pen > 0.0f)", "float pen = ay + r - O_GOAL_HY;\n      if (pen >= 0.0f)",
     {"pocket_pen"}),
    ("clip_hi", "acts[i] = clampf(acts[i], -p->clip_actions, p->clip_actions);",
     "acts[i] = clampf(acts[i], -p->clip_actions, p->clip_actions * 1.0000001f);", {"clip"}),
    ("clip_lo", "acts[i] = clampf(acts[i], -p->clip_actions, p->clip_actions);",
     "acts[i] = clampf(acts[i], -p->clip_actions * 1.0000001f, p->clip_actions);", {"clip"}),
    ("dv_ulp", "#define O_DV 0.15f ", "#define O_DV 0.15000002f ", {"dv", "clip"}),  # full commands from rest brake too
    ("dl_ulp", "#define O_DL 0.171675f ", "#define O_DL 0.17167501f ", {"dl"}),
]
RESET_MUTANTS = {"reset_rounds", "reset_lt"}


def makefile_cflags():
    text = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    return re.search(r"^CFLAGS \?= (.*)$", text, re.M).group(1).split()


class Lib:
    """A second binding of an oracle library: step and reset_dones over oracle.HostEnv buffers."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        P = ctypes.c_void_p
        L.oracle_step.argtypes = [ctypes.c_int64, ctypes.c_int32, P, P, P, P]
        L.oracle_reset_dones.argtypes = [ctypes.c_int64, P, P, P]
        self.L = L

    def step(self, h, actions, io, prm):
        actions = np.ascontiguousarray(actions, np.float32)
        cio = O.VssStepIO(O._p(actions), None, O._p(io["obs"]), O._p(io["terminal_obs"]), O._p(io["rew"]), None, None,
                          O._p(io["time_outs"]), O._p(io["progress_f"]))
        st = h.c_state()
        assert self.L.oracle_step(h.n, O.MODE_FULL, ctypes.byref(prm), ctypes.byref(st), ctypes.byref(cio), None) == 0

    def reset_dones(self, h, prm, draws):
        st = h.c_state()
        assert self.L.oracle_reset_dones(h.n, ctypes.byref(prm), ctypes.byref(st), ctypes.byref(draws)) == 0


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """{"real": Lib, mutant id: Lib}: the unchanged source and every mutant, each its own library."""
    tmp = tmp_path_factory.mktemp("oracle_mutants")
    src = open(os.path.join(ORACLE_DIR, "vss_oracle.c")).read()
    flags = makefile_cflags()
    jobs = {"real": src}
    for mid, old, new, _ in MUTANTS:
        assert src.count(old) == 1, f"mutant {mid}: its text occurs {src.count(old)} times in vss_oracle.c"
        assert old != new
        jobs[mid] = src.replace(old, new)
    assert len(jobs) == len(MUTANTS) + 1

    def compile_one(item):
        mid, text = item
        d = tmp / mid
        d.mkdir()
        (d / "vss_oracle.c").write_text(text)
        out = d / f"libvss_oracle_{mid}.so"
        subprocess.run(["gcc", *flags, "-I", ORACLE_DIR, "-I", os.path.join(ORACLE_DIR, "..", "include"), "-shared", "-o",
                        str(out), str(d / "vss_oracle.c"), "-lm"], check=True)
        return mid, str(out)

    with ThreadPoolExecutor(8) as ex:
        paths = dict(ex.map(compile_one, jobs.items()))
    return {mid: Lib(p) for mid, p in paths.items()}


def signatures(lib, cases):
    """Per case, every bit the step produces over STEPS steps: (len(cases), words) uint32."""
    sig = [None] * len(cases)
    for ml in sorted({c.max_len for c in cases}):
        idx = [i for i, c in enumerate(cases) if c.max_len == ml]
        state, actions, progress = E.pack([cases[i] for i in idx])
        n = len(idx)
        h = O.HostEnv(n)
        h.state[:], h.progress[:], h.reset[:] = state, progress, 0
        prm = O.params(max_episode_length=ml, seed=1234)
        parts = []
        for _ in range(STEPS):
            io = O.make_io(n, O.MODE_FULL)
            lib.step(h, actions, io, prm)
            parts += [h.state.T.copy().view(np.uint32), io["rew"].view(np.uint32), h.reset.astype(np.uint32)[:, None],
                      io["time_outs"].astype(np.uint32)[:, None], h.progress.astype(np.uint32)[:, None],
                      io["obs"].reshape(n, 312).view(np.uint32), io["terminal_obs"].reshape(n, 312).view(np.uint32),
                      h.dof.view(np.uint32)]
        block = np.concatenate(parts, axis=1)
        for j, i in enumerate(idx):
            sig[i] = block[j]
    return np.stack(sig)


def reset_signature(lib, case):
    h = O.HostEnv(1)
    d, keep = O.make_draws(case.row, np.zeros(0, np.float32))
    lib.reset_dones(h, O.params(seed=1), d)
    return np.concatenate([h.state[:, 0].view(np.uint32), h.ctr, h.dof[0].view(np.uint32),
                           np.array([d.uniform_pos], np.uint32)])


@pytest.fixture(scope="module")
def cases():
    return E.table()


@pytest.fixture(scope="module")
def real_sig(libs, cases):
    return signatures(libs["real"], cases)


def test_table_shape():
    """The table has every group the parity suite leaves thin, unique names, and a wave-unfriendly size."""
    cases = E.table()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert 300 <= len(cases) <= 6000
    groups = {c.base.split("/")[0] for c in cases}
    assert groups == {"wall", "rr", "br", "yaw", "drive", "goal"}
    for b in E.BASES:  # the expansion: six robot indices where a robot is concerned, four quadrants always
        assert sum(c.base == b.name for c in cases) == (24 if b.k else 4), b.name
    tags = {t for c in cases for t in c.tags} | {t for c in E.reset_cases() for t in c.tags}
    for mid, _, _, own in MUTANTS:
        assert own <= tags, (mid, own - tags)
    assert {c.max_len for c in cases} == {E.MAX_LEN, 1, 2}
    assert any(np.signbit(c.state[0]) and c.state[0] == 0 for c in cases)  # a -0.0 coordinate


@pytest.mark.parametrize("mid", [m[0] for m in MUTANTS if m[0] not in RESET_MUTANTS])
def test_mutant_is_caught_by_its_own_cases_only(libs, cases, real_sig, mid):
    own = next(m[3] for m in MUTANTS if m[0] == mid)
    differs = (signatures(libs[mid], cases) != real_sig).any(axis=1)
    tagged = np.array([bool(own & set(c.tags)) for c in cases])
    assert (differs & tagged).any(), f"mutant {mid} survives the cases built for it"
    stray = [cases[i].name for i in np.nonzero(differs & ~tagged)[0]]
    assert not stray, f"mutant {mid} also changes cases not built for it: {stray[:8]}"
    # the expansion matters: the mutant is caught at every robot index and in every quadrant it was expanded to
    hit = [c for c, d in zip(cases, differs) if d]
    assert {c.name.rsplit("/", 2)[2] for c in hit} == {"++", "-+", "+-", "--"}
    if any(c.robots for c in hit):
        assert {c.name.rsplit("/", 2)[1] for c in hit if c.robots} == {f"r{r}" for r in range(6)}


@pytest.mark.parametrize("mid", sorted(RESET_MUTANTS))
def test_reset_mutant_is_caught_by_its_own_cases_only(libs, mid):
    own = next(m[3] for m in MUTANTS if m[0] == mid)
    rc = E.reset_cases()
    differs = [not np.array_equal(reset_signature(libs[mid], c), reset_signature(libs["real"], c)) for c in rc]
    assert any(d for d, c in zip(differs, rc) if own & set(c.tags)), f"mutant {mid} survives"
    assert not [c.name for d, c in zip(differs, rc) if d and not own & set(c.tags)]


def test_reset_mutants_leave_the_step_table_alone(libs, cases, real_sig):
    for mid in sorted(RESET_MUTANTS):
        assert np.array_equal(signatures(libs[mid], cases), real_sig), mid


def test_step_mutants_leave_the_reset_cases_alone(libs):
    rc = E.reset_cases()
    want = [reset_signature(libs["real"], c) for c in rc]
    for mid, _, _, _ in MUTANTS:
        if mid not in RESET_MUTANTS and not mid.startswith("rr_"):  # positions_too_close shares no code with them
            assert all(np.array_equal(reset_signature(libs[mid], c), w) for c, w in zip(rc, want)), mid


def test_second_binding_is_the_real_oracle(libs, cases, real_sig):
    """The tmp_path copy of the unchanged source computes what oracle._lib computes."""
    main = Lib(O.LIB_PATH if os.path.exists(O.LIB_PATH) else O.build())
    assert np.array_equal(signatures(main, cases), real_sig)
    assert O._lib is None or O._lib._name == O.LIB_PATH


def test_reset_cases_consume_what_they_claim(libs):
    rc = {c.name: c for c in E.reset_cases()}
    used = {k: int(reset_signature(libs["real"], c)[-1]) for k, c in rc.items()}
    assert used["cap"] == 64 * 14 + 8 and used["all_but_last"] == 64 * 14 + 8 and used["five_rounds"] == 5 * 14 + 8
    assert used["pair_at_007"] == 22 and used["pair_farther_007"] == 22 and used["pair_closer_007"] == 36
    assert used["yaw_draws"] == 22
    # the cap accepted a colliding placement: robot 0 sits on the ball
    h = O.HostEnv(1)
    d, keep = O.make_draws(rc["cap"].row, np.zeros(0, np.float32))
    libs["real"].reset_dones(h, O.params(seed=1), d)
    assert h.state[0, 0] == h.state[O.CH_RX, 0] and h.state[1, 0] == h.state[O.CH_RY, 0]
    # u = 0, 0.5, 1 - 2^-24: yaws -pi, 0 and just under pi
    h = O.HostEnv(1)
    d, keep = O.make_draws(rc["yaw_draws"].row, np.zeros(0, np.float32))
    libs["real"].reset_dones(h, O.params(seed=1), d)
    yaw = 2 * np.arctan2(h.state[O.CH_RQZ:O.CH_RQZ + 3, 0].astype(np.float64), h.state[O.CH_RQW:O.CH_RQW + 3, 0].astype(np.float64))
    np.testing.assert_allclose(np.abs(yaw), [np.pi, 0.0, np.pi], atol=1e-6)


def test_every_case_keeps_the_invariants(cases):
    """Finite state, unit quaternions within 1e-5, bodies inside the back and side walls, after each of two steps."""
    lib = Lib(O.LIB_PATH if os.path.exists(O.LIB_PATH) else O.build())
    for ml in sorted({c.max_len for c in cases}):
        sub = [c for c in cases if c.max_len == ml]
        state, actions, progress = E.pack(sub)
        h = O.HostEnv(len(sub))
        h.state[:], h.progress[:], h.reset[:] = state, progress, 0
        prm = O.params(max_episode_length=ml, seed=1234)
        for t in range(STEPS):
            io = O.make_io(len(sub), O.MODE_FULL)
            lib.step(h, actions, io, prm)
            s = h.state
            bad = ~np.isfinite(s).all(axis=0) | ~np.isfinite(io["obs"].reshape(len(sub), -1)).all(axis=1)
            assert not bad.any(), [sub[i].name for i in np.nonzero(bad)[0][:8]]
            qn = s[O.CH_RQZ:O.CH_RQZ + 6].astype(np.float64) ** 2 + s[O.CH_RQW:O.CH_RQW + 6].astype(np.float64) ** 2
            bad = (np.abs(qn - 1) >= 1e-5).any(axis=0)
            assert not bad.any(), [sub[i].name for i in np.nonzero(bad)[0][:8]]
            rx, ry = np.abs(s[O.CH_RX:O.CH_RX + 6]), np.abs(s[O.CH_RY:O.CH_RY + 6])
            bad = (rx > 0.85 - 0.04 + 1e-6).any(axis=0) | (ry > 0.65 - 0.04 + 1e-6).any(axis=0)
            bad |= (np.abs(s[0]) > 0.85 - 0.02134 + 1e-6) | (np.abs(s[1]) > 0.65 - 0.02134 + 1e-6)
            assert not bad.any(), [sub[i].name for i in np.nonzero(bad)[0][:8]]
