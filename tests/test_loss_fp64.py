"""The three evaluations of the PPO minibatch loss against fp64, row by row, kinks included: vss_ppo_loss and
vss_ppo_loss_direct (csrc/vss_loss.hip) and the x6 GEMM's loss epilogue (vss_linear_tanh_loss_bf16x6 +
vss_ppo_loss_fused_finish), which share csrc/vss_loss_row.h.

The reference's loss that these kernels implement: ppo_continuous_action_isaacgym.py:318-349.

Two references, both on the host:
  * the fp64 statement (_statement): torch fp64 autograd of the reference's expressions with clip, lo and hi
    given explicitly (the fp32 values the ABI receives, widened); torch.max / torch.clamp are the contract at
    the kinks;
  * a numpy fp32 restatement of vss_loss_row.h (_rows with dt = float32): the same expressions in the same
    order, each operation rounded to fp32.  It never goes through the kernels.  It is the yardstick for the
    tolerances and produces the bit-exact logp_old the kink rows need.  (_rows with dt = float64 gives the
    per-row terms of the fp64 statement; a CPU test holds it to the autograd.)

Section 1 (random rows): rows within a band of a kink are moved out of it in fp64 before any kernel runs (band =
8 x the restatement's own error of the quantity in question, asserted <= 1e-4; at most 0.5 % of the rows or 4),
then EVERY row is compared on its own scale and clipfrac as an exact count.  Tolerances: per row 4 x the
restatement's largest error in units of the row's scale (at least 4 U: the restatement cannot do better than
one rounding of the result, and over a handful of rows it can be lucky); sums: that, plus the summation bound
from the kernels' operation counts, one U = 2^-24 of the sum of absolute terms per add.  None is taken from
what the kernels return.  Section 2 (rows placed on the kinks, all values dyadic): exact equality with the
tables of the issue, which the fp64 statement must reproduce.

Figures measured on an MI355X are quoted in the tests' docstrings and in DESIGN.md 5.6, 5.8, 5.9.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vss_amd import _native as N
from vss_amd.loss import N_ACT

from test_write_extents import SENTINEL, Guarded

DEV = "cuda"
U = 2.0 ** -24  # fp32 unit roundoff
F32 = np.float32
F64 = np.float64
K_LOG32 = F32(0.91893853320467274178)  # vss_loss_row.h kLogSqrt2Pi
K_LOG64 = math.log(math.sqrt(2 * math.pi))
NAN = float("nan")


def _lib():
    return N.load()


def _st():
    return N.stream_of(torch.device(DEV))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _nan(*shape):
    """An output buffer that starts as NaN: an element the kernel leaves unwritten shows."""
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def _f(x):
    return float(F32(x))


def _coef(clip=0.2, ent=0.005, vf=4.0, lo=None, hi=None):
    """The coefficients as the fp32 values the ABI's float arguments receive (1 - clip and 1 + clip formed in
    double, then rounded, as the Python wrappers pass them), widened to Python floats."""
    return SimpleNamespace(clip=_f(clip), lo=_f(1 - clip if lo is None else lo), hi=_f(1 + clip if hi is None else hi),
                           ent=_f(ent), vf=_f(vf))


# ---------------------------------------------------------------------------------------------------------
# 0. the two references
# ---------------------------------------------------------------------------------------------------------
def _sum_parts(dt, parts, bias):
    """An output layer's value as the kernels form it: the parts in order, then the bias (bias None: the
    plain entry, whose one part is the output itself)."""
    out = parts[0].astype(dt)
    for q in range(1, parts.shape[0]):
        out = out + parts[q].astype(dt)
    return out if bias is None else out + bias.astype(dt)


def _moments(adv_part, count):
    """(mean, std) as fp32 from the fp64 (sum, sum of squares) parts: m = s / n,
    std = sqrt(max((q - n m^2) / (n - 1), 0)) in fp64, each rounded to fp32 (the header's formula)."""
    s, q = float(adv_part[:, 0].sum()), float(adv_part[:, 1].sum())
    m = s / count
    var = max((q - count * m * m) / (count - 1.0), 0.0)
    return F32(m), F32(math.sqrt(var))


def _normalised(dt, adv, norm):
    """(a - float(m)) / (float(std) + 1e-8f) in dt; norm None: the advantages as given."""
    if norm is None:
        return adv.astype(dt)
    m, sd = norm
    return (adv.astype(dt) - dt(m)) / (dt(sd) + dt(F32(1e-8)))


def _rows(dt, c, cv, logstd, mu, v, x, logp_old, A, R, vo):
    """vss_loss_row.h (actor_consts, actor_row, critic_row) restated in numpy: the same expressions in the same
    order, every operation rounded to dt.  dt = float32: the restatement; dt = float64 (with the doubles'
    log sqrt(2 pi)): the per-row terms of the fp64 statement."""
    n, na = mu.shape
    one, half, two, zero = dt(1), dt(0.5), dt(2), dt(0)
    clip, lo, hi, vf = dt(c.clip), dt(c.lo), dt(c.hi), dt(c.vf)
    klog = K_LOG32 if dt is F32 else dt(K_LOG64)
    inv_n = one / dt(n)
    s = np.exp(logstd.astype(dt))
    var, lsc = s * s, np.log(s)
    dz = x - mu
    nlp = np.zeros(n, dt)
    for a in range(na):
        nlp = nlp + (-(dz[:, a] * dz[:, a]) / (two * var[a]) - lsc[a] - klog)
    logratio = nlp - logp_old
    ratio = np.exp(logratio)
    o = SimpleNamespace(var=var, lsc=lsc, dz=dz, nlp=nlp, ratio=ratio, inv_n=inv_n)
    o.nlr = -logratio
    o.kl = (ratio - one) - logratio
    o.cf = np.abs(ratio - one) > clip
    in_r = (ratio >= lo) & (ratio <= hi)
    rc = np.minimum(np.maximum(ratio, lo), hi)
    p1, p2 = -A * ratio, -A * rc
    o.pg = np.maximum(p1, p2)
    w1 = np.where(p1 > p2, one, np.where(p1 == p2, half, zero))
    w2 = np.where(p2 > p1, one, np.where(p1 == p2, half, zero))
    dratio = w1 * -A + np.where(in_r, w2 * -A, zero)
    o.dnlp = dratio * ratio
    o.gm = (o.dnlp * inv_n)[:, None] * (dz / var)
    o.lg = o.dnlp[:, None] * ((dz * dz) / var - one)
    if cv:
        d = v - vo
        vc = vo + np.minimum(np.maximum(d, -clip), clip)
        eu, ec = v - R, vc - R
        lu, lc = eu * eu, ec * ec
        o.vl = np.maximum(lu, lc)
        wu = np.where(lu > lc, one, np.where(lu == lc, half, zero))
        wc = np.where(lc > lu, one, np.where(lu == lc, half, zero))
        in_v = (d >= -clip) & (d <= clip)
        o.dv = half * (wu * two * eu + np.where(in_v, wc * two * ec, zero))
        o.d, o.lu, o.lc, o.in_v = d, lu, lc, in_v
        o.e_sel = np.where(lu >= lc, eu, ec)
    else:
        e = v - R
        o.vl = e * e
        o.dv = e
        o.e_sel = e
    o.gv = vf * o.dv * inv_n
    for name in ("ratio", "pg", "kl", "gm", "lg", "vl", "gv"):
        assert getattr(o, name).dtype == dt, name
    return o


def _statement(c, cv, logstd, mu, v, x, logp_old, A, R, vo):
    """The fp64 statement: ppo...:318-349 on torch fp64 autograd (vss_amd.loss.reference_loss with lo, hi and
    clip explicit).  Returns the loss, the six statistics and d loss / d (mean, value, logstd)."""
    from torch.distributions.normal import Normal
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F64))  # noqa: E731
    mean, value, ls = t(mu).requires_grad_(), t(v).requires_grad_(), t(logstd).view(1, -1).requires_grad_()
    action, logp_old, adv, returns, values_old = t(x), t(logp_old), t(A), t(R), t(vo)
    probs = Normal(mean, torch.exp(ls.expand_as(mean)), validate_args=False)
    newlogprob = probs.log_prob(action).sum(1)
    entropy = probs.entropy().sum(1)
    logratio = newlogprob - logp_old
    ratio = logratio.exp()
    with torch.no_grad():
        old_approx_kl = (-logratio).mean()
        approx_kl = ((ratio - 1) - logratio).mean()
        clipped = int(((ratio - 1.0).abs() > c.clip).sum())
    pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, c.lo, c.hi)).mean()
    if cv:
        v_unclipped = (value - returns) ** 2
        v_clipped = values_old + torch.clamp(value - values_old, -c.clip, c.clip)
        v_loss = 0.5 * torch.max(v_unclipped, (v_clipped - returns) ** 2).mean()
    else:
        v_loss = 0.5 * ((value - returns) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - c.ent * entropy_loss + v_loss * c.vf
    loss.backward()
    loss, pg_loss, v_loss, entropy_loss = (t.detach() for t in (loss, pg_loss, v_loss, entropy_loss))
    return SimpleNamespace(loss=float(loss), pg=float(pg_loss), v=float(v_loss), ent=float(entropy_loss),
                           old_kl=float(old_approx_kl), kl=float(approx_kl), clipped=clipped,
                           gm=mean.grad.numpy(), gv=value.grad.numpy(), gl=ls.grad.numpy().reshape(-1))


# ---------------------------------------------------------------------------------------------------------
# 1. random rows: the repair, the scales, the tolerances
# ---------------------------------------------------------------------------------------------------------
BAND_MAX = 1e-4
NUDGE = F32(1e-3)


def _finish(k):
    """A drawn case k (fp32 inputs; k.mu(dt) / k.v(dt) the networks' outputs in dt, k.mag_mu / k.mag_v the sums
    of their terms' magnitudes) -> the rows near a kink moved out of the band, both references, the per-row
    scales and the tolerances in units of U."""
    rows, c, cv = k.rows, k.c, k.cv

    def both():
        out = []
        for dt in (F64, F32):
            out.append(_rows(dt, c, cv, k.logstd, k.mu(dt), k.v(dt), k.action.astype(dt), k.logp_old.astype(dt),
                             _normalised(dt, k.adv, k.norm), k.ret.astype(dt), k.val_old.astype(dt)))
        return out

    moved = np.zeros(rows, bool)
    for _ in range(6):
        r64, r32 = both()
        # the bands: 8 x the restatement's own error of the quantity (at least 8 roundings of it)
        band_r = 8 * max(float(np.abs(r32.ratio - r64.ratio).max()), U * float(r64.ratio.max()))
        near_r = (np.abs(r64.ratio - c.lo) < band_r) | (np.abs(r64.ratio - c.hi) < band_r) | \
                 (np.abs(np.abs(r64.ratio - 1) - c.clip) < band_r)
        near_d = near_l = np.zeros(rows, bool)
        band_d = band_l = 0.0
        if cv:
            band_d = 8 * max(float(np.abs(r32.d - r64.d).max()), U * float(np.abs(r64.d).max()))
            near_d = np.abs(np.abs(r64.d) - c.clip) < band_d
            top = np.maximum(r64.lu, r64.lc)
            diff32 = r32.lu.astype(F64) - r32.lc.astype(F64)  # the kernel compares the two fp32 values exactly
            out_v = ~r64.in_v
            if out_v.any():
                band_l = 8 * max(float(np.abs(diff32 - (r64.lu - r64.lc))[out_v].max()), U * float(top[out_v].max()))
            near_l = out_v & (np.abs(r64.lu - r64.lc) < band_l * top)
        assert max(band_r, band_d, band_l) <= BAND_MAX, (band_r, band_d, band_l)
        if not (near_r | near_d | near_l).any():
            break
        moved |= near_r | near_d | near_l
        k.logp_old[near_r] += NUDGE
        k.val_old[near_d | near_l] += NUDGE
        k.ret[near_l] += NUDGE
    else:
        raise AssertionError("rows stay near a kink after six repairs")
    k.bands = (band_r, band_d, band_l)
    # after the repair fp32 rounding flips no branch: the restatement decides every row as fp64 does (inside
    # the value clamp the clipped value is the value up to rounding, and either side gives the same gradient)
    out_v = ~r64.in_v if cv else None
    for what, a, b in (("cf", r64.cf, r32.cf), ("dratio", r64.dnlp == 0, r32.dnlp == 0), ("dv", r64.dv == 0, r32.dv == 0)) + \
            ((("in_v", r64.in_v, r32.in_v), ("lu > lc", (r64.lu > r64.lc)[out_v], (r32.lu > r32.lc)[out_v])) if cv else ()):
        assert np.array_equal(a, b), what
    k.moved = int(moved.sum())
    k.r64, k.r32 = r64, r32
    k.ref = _statement(c, cv, k.logstd, k.mu(F64), k.v(F64), k.action, k.logp_old, _normalised(F64, k.adv, k.norm),
                       k.ret, k.val_old)

    # ---- the rows' scales: |reference| plus the magnitudes of the terms behind it
    r = r64
    absdz, var = np.abs(r.dz), r.var
    edz = k.mag_mu + np.abs(k.action.astype(F64))  # what x - mu is formed from
    T = (r.dz ** 2 / (2 * var) + np.abs(r.lsc) + K_LOG64 + absdz / var * edz).sum(1) + np.abs(k.logp_old) + np.abs(r.nlp)
    one_T = (1 + T)[:, None]
    dn = np.abs(r.dnlp)[:, None]
    k.S = S = SimpleNamespace()
    S.gm = dn * float(r.inv_n) * (absdz / var * one_T + edz / var)
    S.lg = dn * ((r.dz ** 2 / var + 1) * one_T + 2 * absdz * edz / var)
    A = np.abs(_normalised(F64, k.adv, k.norm))
    S.pg = A * r.ratio * (1 + T)
    S.nlr = T
    S.kl = (r.ratio + 1) * (1 + T)
    ev = k.mag_v + np.abs(k.ret) + (np.abs(k.val_old) + c.clip if cv else 0.0)
    S.vl = np.abs(r.e_sel) * (np.abs(r.e_sel) + ev)
    S.gv = np.where(r.dv == 0, 0.0, c.vf * float(r.inv_n) * (np.abs(r.dv) + ev))

    # ---- the restatement's largest error in units of U x scale; a quantity whose scale is 0 must be exactly 0
    k.units, k.restated = SimpleNamespace(), SimpleNamespace()
    refs = dict(gm=k.ref.gm, gv=k.ref.gv, lg=r.lg, pg=r.pg, nlr=r.nlr, kl=r.kl, vl=r.vl)
    for name, want in refs.items():
        got, sc = getattr(r32, name).astype(F64), getattr(S, name)
        assert np.all(got[sc == 0] == 0), name
        e = float((np.abs(got - want)[sc > 0] / (U * sc[sc > 0])).max()) if (sc > 0).any() else 0.0
        setattr(k.restated, name, e)
        setattr(k.units, name, 4 * max(e, 1.0))
    return k


def _draw_tail(k, rng, mu64, v64):
    """The stored rows around the networks' outputs, as tests/test_loss.py::_inputs: the actions one standard
    deviation around the means, log-probs 0.25 around the new ones (ratios over and beyond the clip range),
    old values 0.3 around the new ones (about half the rows beyond the value clamp)."""
    rows, na = k.rows, k.n_act
    sd = np.exp(k.logstd.astype(F64))
    k.action = np.full((k.rows_pad, na), NAN, F32)  # the padding rows are not read
    k.action[:rows] = mu64 + rng.standard_normal((rows, na)) * sd
    dz = k.action[:rows].astype(F64) - mu64
    lp = (-(dz ** 2) / (2 * sd ** 2) - k.logstd.astype(F64) - K_LOG64).sum(1)
    k.logp_old = (lp + rng.standard_normal(rows) * 0.25).astype(F32)
    k.ret = rng.standard_normal(rows).astype(F32)
    k.val_old = (v64 + rng.standard_normal(rows) * 0.3).astype(F32)
    k.action_rows = k.action
    k.action = k.action[:rows]


def _draw_adv(k, rng, adv_mode):
    """The advantages and their normalisation parts.  adv_mode None: as given (normalised on the host in fp32
    when k.host_norm); ("split", p): p parts that split the rows' sums; ("union", p): the parts also hold a
    second rank's rows and adv_count = 2 rows; ("const", p): every advantage 0.1f."""
    rows = k.rows
    adv = (rng.standard_normal(rows) * 2.0 + 0.3).astype(F32)
    k.adv_part, k.adv_count, k.norm = None, 0.0, None
    if adv_mode is None:
        if k.host_norm and rows > 1:
            adv = ((adv - adv.mean()) / (adv.std(ddof=1) + F32(1e-8))).astype(F32)
    else:
        kind, nparts = adv_mode
        if kind == "const":
            adv = np.full(rows, F32(0.1))
        pool = adv.astype(F64)
        if kind == "union":
            pool = np.concatenate([pool, (rng.standard_normal(rows) * 1.5 - 0.4).astype(F32).astype(F64)])
            rng.shuffle(pool)
        # a part = one block's sequential fp64 sums of its rows
        k.adv_part = np.array([[np.cumsum(ch)[-1], np.cumsum(ch * ch)[-1]] if ch.size else [0.0, 0.0]
                               for ch in np.array_split(pool, nparts)])
        k.adv_count = float(pool.size)
        k.norm = _moments(k.adv_part, k.adv_count)
    k.adv = adv


SHAPES = [(1, 1), (1, 256), (255, 256), (256, 256), (257, 512), (1000, 1024), (4133, 4352), (262147, 262400)]


def _base_cases():
    """Three cases per shape: every n_act of N_ACT with both clip_vloss values and with at least three shapes,
    every shape with both clip_vloss values."""
    cases = []
    for s, (rows, rows_pad) in enumerate(SHAPES):
        for j in range(3):
            cases.append((rows, rows_pad, N_ACT[(s + 2 * j) % 6], (s + j) % 2))
    assert {(a, cv) for _, _, a, cv in cases} == {(a, cv) for a in N_ACT for cv in (0, 1)}
    assert {(r, cv) for r, _, _, cv in cases} == {(r, cv) for r, _ in SHAPES for cv in (0, 1)}
    return cases


PLAIN_CASES = _base_cases()
PART_COUNTS = [(1, 1), (4, 4), (5, 3)]
ADV_MODES = [None, ("split", 1), ("split", 63), ("split", 64), ("split", 65), ("split", 256)]


def _direct_cases():
    """The base cases with the part counts and the advantage modes cycled over them (rows = 1 cannot be
    normalised: n - 1 = 0), the data-parallel union and the two constant-advantage cases."""
    cases = []
    for i, (rows, rows_pad, a, cv) in enumerate(PLAIN_CASES):
        mode = ADV_MODES[(i + i // 6) % 6] if rows > 1 else None
        cases.append((rows, rows_pad, a, cv) + PART_COUNTS[i % 3] + (mode,))
    assert {cs[6] for cs in cases} == set(ADV_MODES) and {cs[4:6] for cs in cases} == set(PART_COUNTS)
    cases.append((1000, 1024, 2, 1, 4, 4, ("union", 65)))
    cases.append((256, 256, 2, 1, 4, 4, ("const", 1)))
    cases.append((4096, 4096, 6, 0, 5, 3, ("const", 65)))
    return cases


DIRECT_CASES = _direct_cases()


@functools.lru_cache(maxsize=None)
def _case(rows, rows_pad, n_act, cv, mp=0, vp=0, adv_mode=None):
    """One drawn, repaired and referenced case of section 1 for the two vss_loss.hip entries; mp = 0: the plain
    entry (the outputs themselves, advantages normalised on the host)."""
    rng = np.random.default_rng([rows, n_act, cv, mp, vp] + ([] if adv_mode is None else [7, adv_mode[1]]))
    k = SimpleNamespace(rows=rows, rows_pad=rows_pad, n_act=n_act, cv=cv, c=_coef(), host_norm=mp == 0)
    P, Q = max(mp, 1), max(vp, 1)
    k.logstd = (rng.standard_normal(n_act) * 0.3).astype(F32)
    k.mparts = np.full((P, rows_pad, n_act), NAN, F32)  # the padding rows are not read
    k.vparts = np.full((Q, rows_pad), NAN, F32)
    k.mparts[:, :rows] = rng.standard_normal((P, rows, n_act)) * 0.5 / math.sqrt(P)
    k.vparts[:, :rows] = rng.standard_normal((Q, rows)) / math.sqrt(Q)
    k.mbias = (rng.standard_normal(n_act) * 0.1).astype(F32) if mp else None
    k.vbias = rng.standard_normal(1).astype(F32) if mp else None
    k.mu = lambda dt: _sum_parts(dt, k.mparts[:, :rows], k.mbias)
    k.v = lambda dt: _sum_parts(dt, k.vparts[:, :rows], k.vbias)
    k.mag_mu = np.abs(k.mparts[:, :rows].astype(F64)).sum(0) + (np.abs(k.mbias.astype(F64)) if mp else 0.0)
    k.mag_v = np.abs(k.vparts[:, :rows].astype(F64)).sum(0) + (abs(float(k.vbias[0])) if mp else 0.0)
    _draw_tail(k, rng, k.mu(F64), k.v(F64))
    _draw_adv(k, rng, adv_mode)
    return _finish(k)


def _blocks(rows_pad):
    return min(1024, -(-rows_pad // 256))


def _sum_adds(rows_pad):
    """Adds on the way to one of vss_loss.hip's sums: a thread's ceil(rows_pad / (blocks 256)) rows, 6
    wave-shuffle adds and 3 over the waves per block; the finish's ceil(blocks / 64) + 6."""
    b = _blocks(rows_pad)
    return -(-rows_pad // (b * 256)) + 9 + -(-b // 64) + 6


def _ent_tol(logstd):
    """|entropy - fp64|: per dimension expf and logf within 2 ulp each (4 U relative in s = 4 U absolute in its
    logarithm, 4 U |logstd|), the constant's rounding and the add (2 U of the term); then n_act adds."""
    ls = np.abs(logstd.astype(F64))
    return U * float((4 + 4 * ls + 2 * (1.42 + ls)).sum()) + U * ls.size * float((1.42 + ls).sum())


def _check_sums(k, got, adds, has_bias_grads):
    """The loss, the statistics and the summed gradients against the fp64 statement: the rows' tolerances summed,
    plus `adds` U of the sum of absolute terms, plus 3 U of the result for the final scalings."""
    r, S, un, ref, c, n = k.r64, k.S, k.units, k.ref, k.c, float(k.rows)

    def tol(name, terms=None, axis=None):
        sc, t = getattr(S, name), getattr(r, name) if terms is None else terms
        return getattr(un, name) * U * sc.sum(axis) + adds * U * np.abs(t).sum(axis)

    report = {}

    def check(name, value, want, bound):
        err = np.abs(np.asarray(value, F64) - want)
        report[name] = float((err / np.maximum(bound, 1e-300)).max())
        assert np.all(err <= bound), (name, value, want, float(np.max(err)), float(np.max(bound)))

    t_pg = tol("pg") / n + 3 * U * abs(ref.pg)
    t_v = 0.5 * tol("vl") / n + 3 * U * abs(ref.v)
    t_ent = _ent_tol(k.logstd)
    check("pg_loss", got.stats[0], ref.pg, t_pg)
    check("v_loss", got.stats[1], ref.v, t_v)
    check("entropy_loss", got.stats[2], ref.ent, t_ent)
    check("old_approx_kl", got.stats[3], ref.old_kl, tol("nlr") / n + 3 * U * abs(ref.old_kl))
    check("approx_kl", got.stats[4], ref.kl, tol("kl") / n + 3 * U * abs(ref.kl))
    check("loss", got.loss, ref.loss, t_pg + c.ent * t_ent + c.vf * t_v
          + 3 * U * (abs(ref.pg) + abs(c.ent * ref.ent) + abs(c.vf * ref.v)))
    check("grad_logstd", got.gl, ref.gl, tol("lg", axis=0) / n + 3 * U * (np.abs(ref.gl) + c.ent))
    if has_bias_grads:
        check("grad_mean_bias", got.dbm, ref.gm.sum(0), tol("gm", ref.gm, 0) + U * np.abs(ref.gm.sum(0)))
        check("grad_value_bias", got.dbv, ref.gv.sum(), tol("gv", ref.gv) + U * abs(ref.gv.sum()))
    # clipfrac as a count: after the repair no row is ambiguous
    assert abs(float(got.stats[5]) * n - ref.clipped) < 0.01, (float(got.stats[5]) * n, ref.clipped)
    return report


def _check_row_grads(k, got):
    """grad_mean and grad_value, every row on its own scale; the padding rows exactly zero."""
    rows = k.rows
    gm, gv = got.gm.astype(F64), got.gv.astype(F64)
    assert not np.isnan(gm).any() and not np.isnan(gv).any()
    assert np.all(gm[rows:] == 0) and np.all(gv[rows:] == 0)
    em = np.abs(gm[:rows] - k.ref.gm)
    ev = np.abs(gv[:rows] - k.ref.gv)
    bm, bv = k.units.gm * U * k.S.gm, k.units.gv * U * k.S.gv
    worst = [float((e[b > 0] / (U * s[b > 0])).max()) if (b > 0).any() else 0.0
             for e, b, s in ((em, bm, k.S.gm), (ev, bv, k.S.gv))]
    bad_m, bad_v = np.argwhere(em > bm), np.argwhere(ev > bv)
    assert bad_m.size == 0, ("grad_mean", bad_m[:4].tolist(), worst[0], k.units.gm)
    assert bad_v.size == 0, ("grad_value", bad_v[:4].tolist(), worst[1], k.units.gv)
    return worst


def _run_loss_entry(k, direct, c=None):
    """vss_ppo_loss (direct False) or vss_ppo_loss_direct on the case's inputs: every output starts as NaN, the
    scratch is exactly *_scratch_floats floats between guard words and must be covered."""
    lib, c = _lib(), k.c if c is None else c
    rows, rows_pad, na = k.rows, k.rows_pad, k.n_act
    floats = (lib.vss_ppo_loss_direct_scratch_floats if direct else lib.vss_ppo_loss_scratch_floats)(rows_pad, na)
    assert floats == _blocks(rows_pad) * (5 + na + (na + 1 if direct else 0))
    partial = Guarded((floats,))
    gm, gv, gl = _nan(rows_pad, na), _nan(rows_pad), _nan(na)
    loss, stats, dbm, dbv = _nan(1), _nan(6), _nan(na), _nan(1)
    ins = [_dev(a) for a in (k.logstd, k.action_rows, k.logp_old, k.adv, k.ret, k.val_old)]
    logstd, action, logp, adv, ret, val = (t.data_ptr() for t in ins)
    coefs = (c.clip, c.lo, c.hi, c.ent, c.vf, int(k.cv))
    if direct:
        mp, vp, mb, vb = _dev(k.mparts), _dev(k.vparts), _dev(k.mbias), _dev(k.vbias)
        part = None if k.adv_part is None else _dev(k.adv_part)
        rc = lib.vss_ppo_loss_direct(_st(), rows, rows_pad, na, mp.data_ptr(), k.mparts.shape[0], mb.data_ptr(),
                                     vp.data_ptr(), k.vparts.shape[0], vb.data_ptr(), logstd, action, logp, adv,
                                     None if part is None else part.data_ptr(),
                                     0 if part is None else part.shape[0], k.adv_count, ret, val, *coefs,
                                     gm.data_ptr(), gv.data_ptr(), gl.data_ptr(), dbm.data_ptr(), dbv.data_ptr(),
                                     loss.data_ptr(), stats.data_ptr(), partial.ptr)
    else:
        mean, value = _dev(k.mparts[0]), _dev(k.vparts[0])
        rc = lib.vss_ppo_loss(_st(), rows, rows_pad, na, mean.data_ptr(), logstd, value.data_ptr(), action, logp, adv,
                              ret, val, *coefs, gm.data_ptr(), gv.data_ptr(), gl.data_ptr(), loss.data_ptr(),
                              stats.data_ptr(), partial.ptr)
    torch.cuda.synchronize()
    assert rc == 0
    assert partial.guards_intact() and partial.covered() and int(partial.backing[0]) == SENTINEL
    out = SimpleNamespace(gm=_np(gm), gv=_np(gv), gl=_np(gl), loss=float(loss[0]), stats=_np(stats), dbm=_np(dbm),
                          dbv=float(dbv[0]))
    assert not np.isnan(out.gl).any() and not np.isnan(out.stats).any() and not math.isnan(out.loss)
    if direct:
        assert not np.isnan(out.dbm).any() and not math.isnan(out.dbv)
    return out


def _cap(rows):
    return max(4, int(0.005 * rows))


def _restated_bound(n_act):
    """The restatement's own per-row error in units of U x scale: the scale counts every term's magnitude
    once, and each meets at most the 3 n_act adds of the log-prob's chain plus a handful of roundings of its own."""
    return 3 * n_act + 8


@pytest.mark.parametrize("case", PLAIN_CASES + DIRECT_CASES, ids=str)
def test_restatement_matches_fp64_statement_cpu(case):
    """Without a GPU, for every case of section 1: the bands are <= 1e-4, the repaired rows within the cap
    (0.5 % or 4), the numpy fp64 terms agree with the autograd statement, and the fp32 restatement is within
    (3 n_act + 8) U of every row's scale of the fp64 statement.

    Measured: the restatement's worst row 0.0-1.4 U x scale for the gradients and 2.7 for the value term; the bands
    at most 7.0e-5; at most 74 of 262,147 rows repaired (0.03 %), 0-1 rows at the smaller shapes."""
    k = _case(*case)
    assert max(k.bands) <= BAND_MAX and k.moved <= _cap(k.rows), (k.bands, k.moved)
    ref, r = k.ref, k.r64
    for a, b in ((r.gm, ref.gm), (r.gv, ref.gv), (r.lg.sum(0) * float(r.inv_n) - k.c.ent, ref.gl),
                 (r.pg.mean(), ref.pg), (0.5 * r.vl.mean(), ref.v), (r.nlr.mean(), ref.old_kl), (r.kl.mean(), ref.kl)):
        assert np.all(np.abs(a - b) <= 1e-12 * (np.abs(b) + 1e-3)), (a, b)
    assert int(r.cf.sum()) == ref.clipped == int(k.r32.cf.sum())
    worst = max(vars(k.restated).values())
    print(f"RESTATED {case}: bands {k.bands[0]:.1e} {k.bands[1]:.1e} {k.bands[2]:.1e} moved {k.moved} "
          + " ".join(f"{n}={e:.2f}" for n, e in vars(k.restated).items()))
    assert worst <= _restated_bound(k.n_act), vars(k.restated)
    if k.rows >= 1000:  # the case exercises both sides of every branch
        assert 0.05 < ref.clipped / k.rows < 0.95
        assert not k.cv or 0.3 < float((~r.in_v).mean()) < 0.7


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLAIN_CASES, ids=str)
def test_ppo_loss_matches_fp64_row_by_row_gpu(case):
    """vss_ppo_loss against the fp64 statement: every row's grad_mean / grad_value within 4 x the restatement's
    error on that row's scale, the padding rows exactly 0, the sums within the rows' tolerances plus the
    operation-count bound, clipfrac as an exact count.

    Measured on an MI355X over the 24 cases, in units of U x the row's scale: the worst row of grad_mean 0.96
    (the restatement's own 0.5-1.1, tolerance 4.0-4.3), of grad_value 1.36 (tolerance 5.4): at most a quarter of
    the tolerance.  The sums: entropy_loss up to 0.17 of its bound, every other sum below 0.08 of its."""
    k = _case(*case)
    got = _run_loss_entry(k, False)
    worst = _check_row_grads(k, got)
    rep = _check_sums(k, got, _sum_adds(k.rows_pad), False)
    print(f"PLAIN {case}: rows gm {worst[0]:.2f}/{k.units.gm:.1f} gv {worst[1]:.2f}/{k.units.gv:.1f} U-units; "
          f"sums err/bound " + " ".join(f"{n}={e:.3f}" for n, e in rep.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", DIRECT_CASES, ids=str)
def test_ppo_loss_direct_matches_fp64_row_by_row_gpu(case):
    """vss_ppo_loss_direct against the fp64 statement on the parts summed in order plus the bias and the
    advantages normalised from the fp64 parts (over the union of two ranks' rows where adv_count = 2 rows): the
    checks of the plain entry, and the output biases' gradients against the fp64 column sums.  Constant
    advantages (whose q - n m^2 comes out below 0 in the kernel's order, asserted): grad_mean and pg_loss
    exactly 0, nothing NaN.

    Measured on an MI355X over the 27 cases, in units of U x the row's scale: the worst row of grad_mean 1.44
    (tolerance 5.0), of grad_value 1.54 (tolerance 6.2): at most 0.29 of the tolerance.  The sums: entropy_loss up
    to 0.16 of its bound, every other sum (the bias gradients among them) below 0.07 of its."""
    k = _case(*case)
    got = _run_loss_entry(k, True)
    worst = _check_row_grads(k, got)
    rep = _check_sums(k, got, _sum_adds(k.rows_pad), True)
    if case[6] is not None and case[6][0] == "const":
        assert _unclamped_variance(k.adv_part, k.adv_count) < 0  # only the clamp keeps sqrt from NaN
        assert k.norm[1] == 0 and np.all(got.gm == 0) and got.stats[0] == 0 and np.all(got.dbm == 0)
    print(f"DIRECT {case}: rows gm {worst[0]:.2f}/{k.units.gm:.1f} gv {worst[1]:.2f}/{k.units.gv:.1f} U-units; "
          f"sums err/bound " + " ".join(f"{n}={e:.3f}" for n, e in rep.items()))


def _unclamped_variance(adv_part, n):
    """(q - n m^2) / (n - 1) with s and q summed in adv_moments' order (lanes stride the parts by 64, then the
    wave's butterfly): only additions, so the host's fp64 gives the device's bits; n is a power of two in the
    constant cases, so n m m is exact whether or not the compiler contracts it."""
    lane = np.zeros((64, 2))
    for i, p in enumerate(adv_part):
        lane[i % 64] += p
    for m in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[np.arange(64) ^ m]
    s, q = lane[0]
    mean = s / n
    return (q - n * mean * mean) / (n - 1.0)


def test_constant_advantage_cases_need_the_clamp_cpu():
    """The two constant-advantage cases: m is exactly 0.1f and q - n m^2 < 0 in the kernel's summation order."""
    for case in DIRECT_CASES:
        if case[6] is not None and case[6][0] == "const":
            k = _case(*case)
            assert k.rows & (k.rows - 1) == 0 and k.norm[0] == F32(0.1) and k.norm[1] == 0
            assert _unclamped_variance(k.adv_part, k.adv_count) < 0
            assert np.all(k.ref.gm == 0) and k.ref.pg == 0


# ---------------------------------------------------------------------------------------------------------
# 1b. the fused entry: vss_linear_tanh_loss_bf16x6 (both roles) + vss_ppo_loss_fused_finish
# ---------------------------------------------------------------------------------------------------------
def _fused_blocks(rows_pad, k_in):
    return int(_lib().vss_linear_tanh_loss_blocks_bf16x6(rows_pad, k_in, 256))


@functools.lru_cache(maxsize=None)
def _two_item_rows_pad(k_in):
    """The smallest rows_pad (whole 256-row tiles) at which the launch has fewer blocks than 128-row items, found
    through the entry itself."""
    for rows_pad in range(256, 1 << 20, 256):
        blocks = _fused_blocks(rows_pad, k_in)
        assert 0 < blocks <= rows_pad // 128
        if blocks < rows_pad // 128:
            return rows_pad
    raise AssertionError("no rows_pad below 2^20 makes a block run two items")


FUSED_CASES = [  # (rows, rows_pad or None = the two-item size with rows = rows_pad - 131, k_in, k_out, parts, cv)
    (1, 256, 64, 1, None, 0), (2, 256, 512, 2, 1, 1), (129, 512, 64, 2, 65, 1), (129, 512, 512, 1, 256, 0),
    (300, 512, 512, 2, 256, 0), (300, 512, 64, 1, 65, 1), (512, 512, 64, 2, 1, 0), (512, 512, 512, 1, 65, 1),
    (None, None, 64, 2, 65, 1)]


def _net(rng, rows_pad, k_in, k_out, b_out_scale):
    x = np.tanh(rng.standard_normal((rows_pad, k_in))).astype(F32)
    w = (rng.standard_normal((256, k_in)) / math.sqrt(k_in)).astype(F32)
    b = (rng.standard_normal(256) * 0.1).astype(F32)
    wo = (rng.standard_normal((k_out, 256)) / 16).astype(F32)
    bo = (rng.standard_normal(k_out) * b_out_scale).astype(F32)
    n = SimpleNamespace(x=x, w=w, b=b, wo=wo, bo=bo)
    d = lambda a: torch.from_numpy(a).double()  # noqa: E731
    n.y64 = torch.tanh(d(x) @ d(w).t() + d(b))
    n.out64 = (n.y64 @ d(wo).t() + d(bo)).numpy()
    # torch fp32 on the host: the outputs the restatement takes for the fused cases' bands and tolerances
    t = torch.from_numpy
    n.y32 = torch.addmm(t(b), t(x), t(w).t()).tanh_()
    n.out32 = (n.y32 @ t(wo).t() + t(bo)).numpy()
    n.mag = (n.y64.abs() @ d(wo).abs().t()).numpy() + np.abs(bo.astype(F64))
    return n


def _grad_in(dtype, n, g_rows, rows_pad):
    """(g_out w_out) (1 - y^2) with g_out zero in the padding rows, in torch `dtype`."""
    g = torch.zeros(rows_pad, n.wo.shape[0], dtype=dtype)
    g[:g_rows.shape[0]] = torch.from_numpy(np.ascontiguousarray(g_rows)).to(dtype)
    y = n.y64 if dtype == torch.float64 else n.y32
    wo = torch.from_numpy(n.wo).to(dtype)
    return g, (g @ wo) * (1 - y * y)


@functools.lru_cache(maxsize=None)
def _fused_case(rows, rows_pad, k_in, k_out, nparts, cv):
    if rows_pad is None:
        rows_pad = _two_item_rows_pad(k_in)
        rows = rows_pad - 131
    rng = np.random.default_rng([rows, rows_pad, k_in, k_out, cv])
    k = SimpleNamespace(rows=rows, rows_pad=rows_pad, n_act=k_out, cv=cv, c=_coef(), host_norm=False, k_in=k_in)
    k.actor, k.critic = _net(rng, rows_pad, k_in, k_out, 0.1), _net(rng, rows_pad, k_in, 1, 1.0)
    k.logstd = (rng.standard_normal(k_out) * 0.3).astype(F32)
    k.mu = lambda dt: (k.actor.out64 if dt is F64 else k.actor.out32)[:rows]
    k.v = lambda dt: (k.critic.out64 if dt is F64 else k.critic.out32)[:rows, 0]
    k.mag_mu, k.mag_v = k.actor.mag[:rows], k.critic.mag[:rows, 0]
    _draw_tail(k, rng, k.mu(F64), k.v(F64))
    _draw_adv(k, rng, None if nparts is None else ("split", nparts))
    _finish(k)
    # the fp64 reference and the fp32 yardstick of the launches' outputs
    for net, g64, g32, S in ((k.actor, k.ref.gm, k.r32.gm, k.S.gm), (k.critic, k.ref.gv[:, None], k.r32.gv[:, None],
                                                                   k.S.gv[:, None])):
        g, net.gz64 = _grad_in(torch.float64, net, g64, rows_pad)
        net.cs64, net.dwo64 = net.gz64.sum(0).numpy(), (g.t() @ net.y64).numpy()
        net.abs_dwo = (g.abs().t() @ net.y64.abs()).numpy()
        net.gz64 = net.gz64.numpy()
        # a row's scale: its gradients' scales through the largest output weight of each output
        net.row_scale = (S * np.abs(net.wo.astype(F64)).max(1)).sum(1)
        net.S_g, net.g64 = S, g64
    return k


def _torch_fp32_chain(k):
    """The yardstick tests/test_gemm_x6.py uses, for this chain: torch fp32 on the device evaluating addmm, tanh
    and the output layer of both networks, the restated loss on those outputs (host, numpy fp32) and
    (g_out w_out) (1 - y^2).  Returns the actor's and the critic's grad_in."""
    ys, outs = [], []
    for net in (k.actor, k.critic):
        x, w, b, wo, bo = (_dev(a) for a in (net.x, net.w, net.b, net.wo, net.bo))
        y = torch.addmm(b, x, w.t()).tanh_()
        ys.append((y, wo))
        outs.append(_np(y @ wo.t() + bo))
    r = _rows(F32, k.c, k.cv, k.logstd, outs[0][:k.rows], outs[1][:k.rows, 0], k.action, k.logp_old,
              _normalised(F32, k.adv, k.norm), k.ret, k.val_old)
    gz = []
    for (y, wo), g_rows in zip(ys, (r.gm, r.gv[:, None])):
        g = torch.zeros(k.rows_pad, wo.shape[0], device=DEV)
        g[:k.rows] = _dev(g_rows)
        gz.append(_np(g.mm(wo) * (1 - y * y)).astype(F64))
    return gz


def _row_errors(gz, net, rows):
    """max_j |gz[r, j] - reference| per row in units of the row's scale; a row of scale 0 must be exactly 0."""
    e = np.abs(gz[:rows] - net.gz64[:rows]).max(1)
    sc = net.row_scale
    assert np.all(e[sc == 0] == 0)
    return float((e[sc > 0] / sc[sc > 0]).max()) if (sc > 0).any() else 0.0


def _fused_launch(k, role, net, planes):
    """One vss_linear_tanh_loss_bf16x6 launch on device copies; every output starts as NaN."""
    lib = _lib()
    rows, rows_pad, k_in, k_out = k.rows, k.rows_pad, k.k_in, net.wo.shape[0]
    blocks = _fused_blocks(rows_pad, k_in)
    gz, cs, dw, st = _nan(rows_pad, 256), _nan(blocks, 256), _nan(blocks, k_out, 256), _nan(blocks, 32)
    x, b, wo, bo = (_dev(a) for a in (net.x, net.b, net.wo, net.bo))
    keep = [_dev(a) for a in (k.action_rows, k.logp_old, k.adv, k.logstd, k.ret, k.val_old)]
    act, logp, adv, logstd, ret, val = (t.data_ptr() for t in keep)
    part = None if k.adv_part is None else _dev(k.adv_part)
    c = k.c
    if role == 0:
        rc = lib.vss_linear_tanh_loss_bf16x6(_st(), 0, rows_pad, rows, k_in, 256, x.data_ptr(), b.data_ptr(), k_out,
                                             wo.data_ptr(), bo.data_ptr(), act, logp, adv,
                                             None if part is None else part.data_ptr(),
                                             0 if part is None else part.shape[0], k.adv_count, logstd, None, None,
                                             c.clip, c.lo, c.hi, c.vf, int(k.cv), gz.data_ptr(), cs.data_ptr(),
                                             dw.data_ptr(), st.data_ptr(), planes.data_ptr())
    else:
        rc = lib.vss_linear_tanh_loss_bf16x6(_st(), 1, rows_pad, rows, k_in, 256, x.data_ptr(), b.data_ptr(), 1,
                                             wo.data_ptr(), bo.data_ptr(), None, None, None, None, 0, 0.0, None, ret,
                                             val if k.cv else None, c.clip, c.lo, c.hi, c.vf, int(k.cv),
                                             gz.data_ptr(), cs.data_ptr(), dw.data_ptr(), st.data_ptr(),
                                             planes.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return SimpleNamespace(gz=_np(gz).astype(F64), cs=_np(cs).astype(F64), dw=_np(dw).astype(F64), st=st, blocks=blocks)


def _fused_finish(k, a, cr):
    na = k.n_act
    gl, dbm, dbv, loss, stats = _nan(na), _nan(na), _nan(1), _nan(1), _nan(6)
    logstd = _dev(k.logstd)
    rc = _lib().vss_ppo_loss_fused_finish(_st(), k.rows, na, a.blocks, a.st.data_ptr(), cr.blocks, cr.st.data_ptr(),
                                          logstd.data_ptr(), k.c.ent, k.c.vf, gl.data_ptr(), dbm.data_ptr(),
                                          dbv.data_ptr(), loss.data_ptr(), stats.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return SimpleNamespace(gl=_np(gl), dbm=_np(dbm), dbv=float(dbv[0]), loss=float(loss[0]), stats=_np(stats))


def _planes(w):
    from vss_amd.update import weight_planes
    return weight_planes([(_dev(w), False)])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=str)
def test_fused_loss_matches_fp64_gpu(case):
    """vss_linear_tanh_loss_bf16x6 for the actor and the critic + vss_ppo_loss_fused_finish against fp64 from x,
    W, b, w_out, b_out:
      * grad_in: the error's norm within 1.25 x that of torch fp32 on the same chain (on the device: addmm, tanh,
        output layer, restated loss, (g_out w_out) (1 - y^2)) + 1e-8, as tests/test_gemm_x6.py holds the forward
        and the backward; row by row (on each row's own scale) within 4 x the yardstick's worst row; the padding
        rows exactly 0;
      * the part_cs and part_dwo parts summed in fp64 against the fp64 column sums and g_out^T y, within the
        rows' tolerances plus (items per block + 20) U of the absolute sums (a lane's <= 8 rows, 4 shuffle adds,
        one += per item, <= 8 wave slots);
      * a part_stats block whose items hold only padding rows is all zeros (it starts as NaN), no word of
        part_stats is NaN;
      * the finish's loss, statistics, grad_logstd and bias gradients within the rows' tolerances (from the
        restatement on torch fp32's outputs) plus the adds: 6 + items per block + 1 per block, blocks / 16 + 16
        in the finish.

    Measured on an MI355X over the 9 cases and both roles: grad_in's error norm 9.3e-8 to 7.2e-7 against torch
    fp32's 1.0e-7 to 6.8e-7 on the same data, the kernel at most 1.24 x torch's (one real row) and below it in 15
    of the 18 launches; the worst row 2.8 U x its scale (torch fp32: 3.4).  The finish's sums: entropy_loss up to
    0.22 of its bound, every other sum below 0.10 of its."""
    k = _fused_case(*case)
    rows, rows_pad = k.rows, k.rows_pad
    outs = []
    yard = _torch_fp32_chain(k)
    for role, net in ((0, k.actor), (1, k.critic)):
        net.gz32 = yard[role]
        o = _fused_launch(k, role, net, _planes(net.w))
        outs.append(o)
        items = rows_pad // 128
        per_block = -(-items // o.blocks)
        if case[0] is None:
            assert per_block == 2
        assert not np.isnan(o.gz).any() and not np.isnan(o.cs).any() and not np.isnan(o.dw).any()
        assert np.all(o.gz[rows:] == 0)
        # 1. grad_in against fp64: the norm and the worst row, both against torch fp32's
        ref = net.gz64
        norm = float(np.linalg.norm(ref))
        e6, et = float(np.linalg.norm(o.gz - ref)) / max(norm, 1e-300), float(np.linalg.norm(net.gz32 - ref)) / max(norm, 1e-300)
        r6, rt = _row_errors(o.gz, net, rows), _row_errors(net.gz32, net, rows)
        print(f"FUSED {case} role {role}: norm err {e6:.3e} (torch fp32 {et:.3e}); worst row {r6 / U:.2f} U-units "
              f"(torch fp32 {rt / U:.2f})")
        if norm > 0:
            assert e6 <= 1.25 * et + 1e-8, (e6, et)
        assert r6 <= 4 * rt, (r6, rt)
        # 2. the parts' sums
        adds = per_block + 20
        row_tol = 4 * max(rt, U) * net.row_scale.sum()
        cs_tol = row_tol + adds * U * np.abs(ref).sum(0)
        assert np.all(np.abs(o.cs.sum(0) - net.cs64) <= cs_tol), float((np.abs(o.cs.sum(0) - net.cs64) / cs_tol).max())
        units = k.units.gm if role == 0 else k.units.gv
        dw_tol = ((units + 4) * U * net.S_g.sum(0))[:, None] + adds * U * net.abs_dwo
        assert np.all(np.abs(o.dw.sum(0) - net.dwo64) <= dw_tol), float((np.abs(o.dw.sum(0) - net.dwo64) / dw_tol).max())
        # 3. the blocks' statistics: block b runs the items b, b + blocks, ...; item w holds the rows [128 w, 128 w + 128)
        st = _np(o.st)
        assert not np.isnan(st).any()
        idle = np.arange(o.blocks) * 128 >= rows
        assert np.all(st[idle] == 0)
    a, cr = outs
    got = _fused_finish(k, a, cr)
    per_block = -(-(rows_pad // 128) // a.blocks)
    rep = _check_sums(k, got, 6 + per_block + 1 + -(-a.blocks // 16) + 16, True)
    print(f"FUSED {case} finish: err/bound " + " ".join(f"{n}={e:.3f}" for n, e in rep.items()))


@pytest.mark.parametrize("case", FUSED_CASES, ids=str)
def test_fused_cases_repair_and_restatement_cpu(case):
    """Without a GPU: the fused cases' bands, repaired-row cap and restatement (on torch fp32's outputs, so the
    GEMM's own fp32 error is inside) against the fp64 statement."""
    k = _fused_case(*case)
    assert max(k.bands) <= BAND_MAX and k.moved <= _cap(k.rows), (k.bands, k.moved)
    print(f"RESTATED fused {case}: bands {k.bands} moved {k.moved} "
          + " ".join(f"{n}={e:.2f}" for n, e in vars(k.restated).items()))


# ---------------------------------------------------------------------------------------------------------
# 2. rows placed exactly on the kinks: exact equality
# ---------------------------------------------------------------------------------------------------------
KINK_ROWS = 8  # a power of two: inv_n is exact
KINK_A = np.array([1, -1, 0, 1, -1, 0, 1, -1], F32)
# (clip_lo, clip_hi) -> n x d loss / d ratio for A = +1, -1, 0 (ratio is exactly 1)
POLICY_TABLE = [((0.75, 1.25), (-1, 1, 0)), ((1.0, 1.25), (-1, 1, 0)), ((0.75, 1.0), (-1, 1, 0)),
                ((1.0, 1.0), (-1, 1, 0)), ((1.25, 1.5), (-1, 0, 0)), ((0.5, 0.75), (0, 1, 0))]
# (v, v_old, R) -> dv at clip = 0.25, clip_vloss = 1
VALUE_TABLE = [((1.25, 1.0, 0.0), 1.25),    # d == +clip: a tie, the clamp passes
               ((0.75, 1.0, 0.0), 0.75),    # d == -clip: a tie, the clamp passes
               ((1.5, 1.0, 1.375), 0.0625),  # a tie outside the clamp: half of the unclipped side
               ((1.5, 1.0, 0.0), 1.5),      # the unclipped loss larger
               ((1.5, 1.0, 2.0), 0.0)]      # the clipped loss larger, the clamp blocks
KINK_ENT, KINK_VF, KINK_CLIP = 2.0 ** -7, 0.5, 0.25


def _kink_case(n_act, lo, hi, direct, fused_v=None):
    """Eight rows on the kinks: logstd = 0, x - mu = 0.5 in every dimension, logp_old the restatement's fp32
    newlogprob (so logratio is exactly 0 and ratio exactly 1), A cycling over +1, -1, 0; the value rows
    cycling over VALUE_TABLE.  direct: the outputs split into parts that sum exactly.  fused_v: every row's
    value is this constant (the fused critic's out = b_out), the table's rows shifted by fused_v - v."""
    rows = KINK_ROWS
    k = SimpleNamespace(rows=rows, rows_pad=rows, n_act=n_act, cv=1, host_norm=False, adv_part=None, adv_count=0.0,
                        norm=None, c=_coef(KINK_CLIP, KINK_ENT, KINK_VF, lo, hi))
    k.logstd = np.zeros(n_act, F32)
    mu = np.full((rows, n_act), 0.25, F32)
    tab = np.array([VALUE_TABLE[r % 5][0] for r in range(rows)], F32)
    if fused_v is not None:
        tab = tab + (F32(fused_v) - tab[:, :1])
    v, k.val_old, k.ret = tab[:, 0].copy(), tab[:, 1].copy(), tab[:, 2].copy()
    if direct:
        k.mparts = np.stack([mu + F32(0.25), np.full_like(mu, -0.125), np.full_like(mu, -0.25)])
        k.mbias = np.full(n_act, 0.125, F32)
        k.vparts = np.stack([v - F32(0.75), np.full_like(v, 0.25)])
        k.vbias = np.array([0.5], F32)
    else:
        k.mparts, k.vparts, k.mbias, k.vbias = mu[None], v[None], None, None
    assert np.array_equal(_sum_parts(F32, k.mparts, k.mbias), mu) and np.array_equal(_sum_parts(F32, k.vparts, k.vbias), v)
    k.action_rows = k.action = mu + F32(0.5)
    k.adv = KINK_A.copy()
    zero = np.zeros(rows, F32)
    k.logp_old = _rows(F32, k.c, 1, k.logstd, mu, v, k.action, zero, k.adv, k.ret, k.val_old).nlp
    k.mu_v = (mu, v)
    return k


def _kink_expected(k, pol):
    """The tables as gradients: grad_mean[a] = dratio ratio inv_n 0.5, grad_logstd = sum dratio ratio (0.25 - 1)
    inv_n - ent_coef, grad_value = vf_coef dv inv_n."""
    inv_n = 1.0 / k.rows
    dratio = np.array([pol[{1: 0, -1: 1, 0: 2}[int(a)]] for a in k.adv], F64)
    gm = np.repeat((dratio * inv_n * 0.5)[:, None], k.n_act, 1)
    gl = np.full(k.n_act, dratio.sum() * (0.25 - 1) * inv_n - KINK_ENT)
    gv = np.array([KINK_VF * VALUE_TABLE[r % 5][1] * inv_n for r in range(k.rows)])
    return gm, gl, gv


@pytest.mark.parametrize("n_act", N_ACT)
@pytest.mark.parametrize("bounds,pol", POLICY_TABLE)
def test_fp64_statement_reproduces_the_kink_tables_cpu(n_act, bounds, pol):
    """torch's autograd of max / clamp on the kink rows (ratio exactly 1 in fp64 too) gives both tables, so they
    cannot drift from torch; so do the fp32 restatement and its fp64 twin."""
    k = _kink_case(n_act, *bounds, direct=False)
    gm, gl, gv = _kink_expected(k, pol)
    mu, v = k.mu_v
    # Normal.log_prob's own fp64 log-prob of these rows as logp_old: the exponent is exactly 0
    from torch.distributions.normal import Normal
    lp = Normal(torch.from_numpy(mu).double(), torch.ones(1, dtype=torch.float64)).log_prob(
        torch.from_numpy(k.action).double()).sum(1).numpy()
    ref = _statement(k.c, 1, k.logstd, mu, v, k.action, lp, k.adv, k.ret, k.val_old)
    assert np.array_equal(ref.gm, gm) and np.array_equal(ref.gv, gv) and np.array_equal(ref.gl, gl)
    assert ref.clipped == 0 and ref.old_kl == 0 and ref.kl == 0
    for dt, lp_dt in ((F32, k.logp_old), (F64, None)):
        zero = np.zeros(k.rows, dt)
        args = [k.logstd, mu.astype(dt), v.astype(dt), k.action.astype(dt)]
        tail = [k.adv.astype(dt), k.ret.astype(dt), k.val_old.astype(dt)]
        lp_dt = _rows(dt, k.c, 1, *args, zero, *tail).nlp if lp_dt is None else lp_dt
        r = _rows(dt, k.c, 1, *args, lp_dt, *tail)
        assert np.all(r.ratio == 1)
        assert np.array_equal(r.gm, gm) and np.array_equal(r.gv, gv)
        assert np.array_equal(r.lg.sum(0) * r.inv_n - dt(KINK_ENT), gl)
        assert r.pg.mean() == ref.pg and 0.5 * r.vl.mean() == ref.v


def _kink_reference(k):
    """pg_loss and v_loss of the kink rows (dyadic: exact in fp32 and fp64 alike) from the restatement."""
    mu, v = k.mu_v
    r = _rows(F32, k.c, 1, k.logstd, mu, v, k.action, k.logp_old, k.adv, k.ret, k.val_old)
    assert np.all(r.ratio == 1)
    return float(r.pg.astype(F64).mean()), 0.5 * float(r.vl.astype(F64).mean())


def _check_kink_outputs(k, pol, got, has_bias_grads):
    gm, gl, gv = _kink_expected(k, pol)
    pg, vl = _kink_reference(k)
    assert np.array_equal(got.gm.astype(F64).reshape(gm.shape), gm), (got.gm.tolist(), gm.tolist())
    assert np.array_equal(got.gv.astype(F64).reshape(-1), gv), (got.gv.tolist(), gv.tolist())
    assert np.array_equal(got.gl.astype(F64), gl), (got.gl, gl)
    assert got.stats[0] == pg and got.stats[1] == vl, (got.stats, pg, vl)
    assert got.stats[3] == 0 and got.stats[4] == 0 and got.stats[5] == 0, got.stats
    ent = k.n_act * (0.5 + K_LOG64)
    assert abs(float(got.stats[2]) - ent) <= _ent_tol(k.logstd)
    assert abs(got.loss - (pg - KINK_ENT * ent + KINK_VF * vl)) <= KINK_ENT * _ent_tol(k.logstd) + 3 * U * (abs(pg) + vl + ent)
    if has_bias_grads:
        assert np.array_equal(got.dbm.astype(F64), gm.sum(0)) and got.dbv == gv.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("n_act", N_ACT)
@pytest.mark.parametrize("bounds,pol", POLICY_TABLE)
def test_loss_entries_on_the_kinks_gpu(bounds, pol, n_act, direct):
    """vss_ppo_loss and vss_ppo_loss_direct on rows placed exactly on the kinks (ratio == 1 against six pairs of
    clamp bounds, A in {+1, -1, 0}; the five value rows): every gradient, pg_loss, v_loss and the three ratio
    statistics equal the tables' dyadic numbers exactly.  (If expf(0) != 1 on the device this fails: a finding.)"""
    k = _kink_case(n_act, *bounds, direct=direct)
    _check_kink_outputs(k, pol, _run_loss_entry(k, direct), direct)


@pytest.mark.gpu
@pytest.mark.parametrize("k_out", [1, 2])
@pytest.mark.parametrize("bounds,pol", POLICY_TABLE)
def test_fused_loss_on_the_kinks_gpu(bounds, pol, k_out):
    """The fused entry on the same rows: W = 0 and bias = 0, so y = tanh(0) = 0 and out = b_out for every row
    (the value table shifted to v = 1.5); w_out holds ones for one output on each half of the features, so
    g_out is read back exactly from grad_in; the finish gives the same exact statistics and gradients."""
    k = _kink_case(k_out, *bounds, direct=False, fused_v=1.5)
    k.rows_pad, k.k_in = 256, 64
    pad = lambda a: np.concatenate([a, np.full((256 - k.rows,) + a.shape[1:], NAN, F32)])  # noqa: E731
    k.action_rows = pad(k.action)
    outs = []
    for role, ko, bo in ((0, k_out, np.full(k_out, 0.25, F32)), (1, 1, np.array([1.5], F32))):
        wo = np.zeros((ko, 256), F32)
        for o in range(ko):
            wo[o, o * 128:(o + 1) * 128 if ko == 2 else 256] = 1
        net = SimpleNamespace(x=np.ones((256, 64), F32), w=np.zeros((256, 64), F32), b=np.zeros(256, F32), wo=wo, bo=bo)
        out = _fused_launch(k, role, net, _planes(net.w))
        assert np.all(out.gz[k.rows:] == 0) and not np.isnan(out.gz).any()
        g = np.stack([out.gz[:k.rows, o * 128] for o in range(ko)], 1)
        for o in range(ko):  # every feature of the output's half carries g_out[:, o]
            half = out.gz[:k.rows, o * 128:(o + 1) * 128 if ko == 2 else 256]
            assert np.all(half == g[:, o:o + 1])
        assert np.all(out.dw.sum(0) == 0)  # g_out^T y with y = 0
        outs.append((out, g))
    (a, gm), (cr, gv) = outs
    fin = _fused_finish(k, a, cr)
    fin.gm, fin.gv = gm, gv[:, 0]
    _check_kink_outputs(k, pol, fin, True)
