"""vss_gae on the GPU (csrc/vss_returns.hip, vss_amd/returns.py): a rollout's advantages and returns in one launch
are compute_gae's bit for bit -- both forms, every unroll / tail / lane-count path, the workload's own shape --
and the kernel writes nothing but its two outputs."""
import numpy as np
import pytest
import torch

import ppo_continuous_action_isaacgym as P

pytestmark = pytest.mark.gpu

STEPS = [1, 2, 3, 7, 8, 9, 17]  # below, at and past one unroll group (8, and 4 for the variant build), with a tail
ROWS = [1, 63, 64, 65, 130]  # one lane, a partial wave, a full one, a second workgroup with one live lane, 2 waves + 2
SHAPES = [(T, E) for T in STEPS for E in ROWS] + [(128, 4095)]
SETTINGS = [(0.99, 0.95), (0.997, 0.9), (1.0, 1.0)]


def rollout(T, E, seed=None):
    """Seeded finite normals; ~10 % dones, half of them time-outs too, a few time-outs without a done; dones
    forced at t = 0 and t = T-1 in column 0; from 63 columns on, column 1 is all done and column 2 has none."""
    rng = np.random.default_rng(T * 100_000 + E if seed is None else seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    u = rng.random((T, E))
    dones = u < 0.10
    timeouts = (u < 0.05) | (rng.random((T, E)) < 0.02)
    dones[0, 0] = dones[T - 1, 0] = True
    if E >= 63:
        dones[:, 1] = True
        dones[:, 2] = False
    d = dict(rewards=f(T, E), values=f(T, E), next_values=f(T, E), term_values=f(T, E), v_last=f(E),
             next_dones=dones.astype(np.float32), next_timeouts=timeouts.astype(np.float32))
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def merged(d):
    """Form B's next_values as the train loop's torch path forms them (TerminalValues.next_values)."""
    return torch.where(d["next_dones"].bool(), d["term_values"], torch.cat([d["values"][1:], d["v_last"].view(1, -1)], 0))


def reference(d, next_values, gamma, lam):
    with torch.no_grad():
        return P.compute_gae(d["rewards"], d["values"], next_values, d["next_dones"], d["next_timeouts"], gamma, lam)


def run(d, gamma, lam, form, **kw):
    from vss_amd.returns import gae
    extra = dict(next_values=d["next_values"]) if form == "A" else dict(term_values=d["term_values"], v_last=d["v_last"])
    extra.update(kw)
    return gae(d["rewards"], d["values"], d["next_dones"], d["next_timeouts"], gamma, lam, **extra)


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_bit_equal(got, want, what):
    for name, g, w in zip(("advantages", "returns"), got, want):
        diff = int((bits(g) != bits(w)).sum())
        assert diff == 0, f"{what}: {diff} of {g.numel()} {name} differ"


@pytest.mark.parametrize("gamma,lam", SETTINGS)
@pytest.mark.parametrize("T,E", SHAPES)
def test_both_forms_equal_compute_gae_bit_for_bit(T, E, gamma, lam):
    d = rollout(T, E)
    assert_bit_equal(run(d, gamma, lam, "A"), reference(d, d["next_values"], gamma, lam), "form A")
    assert_bit_equal(run(d, gamma, lam, "B"), reference(d, merged(d), gamma, lam), "form B")


def test_the_inputs_have_the_cases_the_shapes_are_for():
    d = rollout(17, 130)
    dn, to = d["next_dones"].bool(), d["next_timeouts"].bool()
    assert dn[0, 0] and dn[16, 0] and dn[:, 1].all() and not dn[:, 2].any()
    assert (dn & to).any() and (dn & ~to).any() and (~dn & to).any()
    assert 0.05 < float(dn[:, 3:].float().mean()) < 0.15


def test_known_answers():
    """tests/test_ppo.py's hand-computed T = 3, two-env case through the kernel."""
    gamma, lam = 0.9, 0.5
    d = dict(rewards=torch.tensor([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]]),
             values=torch.tensor([[0.5, 0.1], [0.2, 0.3], [0.4, 0.0]]),
             next_values=torch.tensor([[0.2, 0.3], [0.7, 0.9], [1.0, 2.0]]),
             next_dones=torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]),
             next_timeouts=torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0]]))
    d = {k: v.cuda() for k, v in d.items()}
    adv, ret = run(d, gamma, lam, "A")
    want = torch.tensor([[0.8735, 1.502], [0.43, 2.96], [1.5, 1.0]]).cuda()
    torch.testing.assert_close(adv, want, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ret, want + d["values"])
    # the same numbers as form B: the terminal values sit where a row reset, the rest comes from values / v_last
    d["term_values"] = torch.tensor([[9.0, 9.0], [0.7, 9.0], [9.0, 2.0]]).cuda()
    d["values"] = torch.tensor([[0.5, 0.1], [0.2, 0.3], [0.4, 0.0]]).cuda()
    d["v_last"] = torch.tensor([1.0, 9.0]).cuda()
    # values[t + 1] must be the next_values of the rows that did not reset: (0, 0) 0.2, (0, 1) 0.3, (1, 1) 0.9
    d["values"][2, 1] = 0.9
    adv_b, ret_b = run(d, gamma, lam, "B")
    want_b = reference(d, merged(d), gamma, lam)
    assert_bit_equal((adv_b, ret_b), want_b, "form B known answers")
    # env 0 is untouched by the changed values[2][1]: the hand-computed column again
    torch.testing.assert_close(adv_b[:, 0], want[:, 0], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("T,E", [(9, 65), (17, 130)])
def test_form_b_selects_the_terminal_values(T, E):
    """term_values of rows that did not reset are NaN: a select never reads them into a sum."""
    gamma, lam = 0.997, 0.9
    d = rollout(T, E)
    want = reference(d, merged(d), gamma, lam)
    d["term_values"] = torch.where(d["next_dones"].bool(), d["term_values"], torch.full_like(d["term_values"], float("nan")))
    assert torch.isnan(d["term_values"]).any()
    got = run(d, gamma, lam, "B")
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert_bit_equal(got, want, "form B with NaN in the rows that did not reset")


# ---- write extents: every buffer is a window between sentinel guards (as tests/test_write_extents.py) ------------

GUARD = 1 << 14  # int32 words on each side (64 KiB)
SENTINEL = 0x7FA5A5A5  # a quiet-NaN bit pattern


class Guarded:
    def __init__(self, fill=None, shape=None):
        shape = tuple(fill.shape) if fill is not None else shape
        self.words = int(np.prod(shape))
        self.backing = torch.full((2 * GUARD + self.words,), SENTINEL, dtype=torch.int32, device="cuda")
        self.t = self.backing[GUARD:GUARD + self.words].view(torch.float32).view(shape)
        if fill is not None:
            self.t.copy_(fill)
        self.before = self.backing.clone()

    def guards_intact(self):
        b = self.backing
        return bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + self.words:] == SENTINEL).all())

    def unchanged(self):
        return torch.equal(self.backing, self.before)

    def covered(self):
        return not bool((self.backing[GUARD:GUARD + self.words] == SENTINEL).any())


@pytest.mark.parametrize("form", ["A", "B"])
def test_the_kernel_writes_only_its_outputs(form):
    T, E = 9, 65
    gamma, lam = 0.99, 0.95
    plain = rollout(T, E)
    g = {k: Guarded(fill=v) for k, v in plain.items()}
    adv, ret = Guarded(shape=(T, E)), Guarded(shape=(T, E))
    run({k: v.t for k, v in g.items()}, gamma, lam, form, out=(adv.t, ret.t))
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.guards_intact() and buf.unchanged(), f"{name} or its guards were written"
    for name, buf in (("advantages", adv), ("returns", ret)):
        assert buf.guards_intact(), f"{name} written outside its extent"
        assert buf.covered(), f"{name} not written in full"
    want = reference(plain, plain["next_values"] if form == "A" else merged(plain), gamma, lam)
    assert_bit_equal((adv.t, ret.t), want, "guarded buffers")


# ---- the Python layer's checks --------------------------------------------------------------------------------------

def test_out_buffers_are_written_in_place_and_returned():
    d = rollout(7, 65)
    out = (torch.empty(7, 65, device="cuda"), torch.empty(7, 65, device="cuda"))
    got = run(d, 0.99, 0.95, "B", out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert_bit_equal(out, reference(d, merged(d), 0.99, 0.95), "out=")


def test_python_checks_raise():
    from vss_amd.returns import gae
    T, E = 7, 65
    d = rollout(T, E)
    base = dict(rewards=d["rewards"], values=d["values"], next_dones=d["next_dones"], next_timeouts=d["next_timeouts"])

    def call(form="A", **kw):
        a = dict(base, gamma=0.99, lam=0.95)
        a.update(dict(next_values=d["next_values"]) if form == "A" else dict(term_values=d["term_values"], v_last=d["v_last"]))
        a.update(kw)
        return gae(**a)

    call()  # the arguments as they are pass
    call("B")
    for name in ("values", "next_dones", "next_timeouts", "next_values"):  # dtype
        with pytest.raises(TypeError, match=name):
            call(**{name: d[name].double()})
    with pytest.raises(TypeError, match="next_dones"):
        call(next_dones=d["next_dones"].bool())
    with pytest.raises(TypeError, match="v_last"):
        call("B", v_last=d["v_last"].half())
    for name in ("values", "next_dones", "next_timeouts", "next_values"):  # shape
        with pytest.raises(ValueError, match=name):
            call(**{name: d[name][:-1]})
        with pytest.raises(ValueError, match=name):
            call(**{name: d[name].reshape(-1)})
    with pytest.raises(ValueError, match="term_values"):
        call("B", term_values=d["term_values"][:, :-1].contiguous())
    with pytest.raises(ValueError, match="v_last"):
        call("B", v_last=d["v_last"].view(1, E))
    with pytest.raises(ValueError, match="rewards"):
        call(rewards=d["rewards"].reshape(-1))
    with pytest.raises(ValueError, match="values"):  # device
        call(values=d["values"].cpu())
    with pytest.raises(RuntimeError):  # everything on the CPU: there is no CPU path
        gae(*(base[k].cpu() for k in ("rewards", "values", "next_dones", "next_timeouts")), 0.99, 0.95,
            next_values=d["next_values"].cpu())
    wide = torch.randn(T, 2 * E, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):  # a strided view
        call(values=wide[:, :E])
    with pytest.raises(ValueError, match="contiguous"):
        call(next_dones=torch.zeros(E, T, device="cuda").t())
    with pytest.raises(ValueError, match="contiguous"):
        call(out=(wide[:, :E], torch.empty(T, E, device="cuda")))
    with pytest.raises(ValueError):  # the forms
        call(term_values=d["term_values"], v_last=d["v_last"])
    with pytest.raises(ValueError):
        call("B", v_last=None)
    with pytest.raises(ValueError):
        gae(**base, gamma=0.99, lam=0.95)
    with pytest.raises(ValueError, match="finite"):
        call(gamma=float("nan"))
    fresh = lambda: torch.empty(T, E, device="cuda")
    with pytest.raises(ValueError, match="overlaps values"):  # out over an input
        call(out=(d["values"], fresh()))
    with pytest.raises(ValueError, match="overlaps rewards"):
        call(out=(fresh(), d["rewards"]))
    with pytest.raises(ValueError, match="overlaps v_last"):
        big = torch.zeros(T * E + E, device="cuda")
        call("B", v_last=big[T * E - 1:T * E - 1 + E], out=(big[:T * E].view(T, E), fresh()))
    with pytest.raises(ValueError, match="overlaps"):
        both = fresh()
        call(out=(both, both))
    with pytest.raises(TypeError):
        call(out=(fresh().double(), fresh()))
    with pytest.raises(ValueError):
        call(out=(torch.empty(T, E + 1, device="cuda"), fresh()))
