"""csrc/vss_optim.hip against fp64, kernel by kernel: the gradient norm's partial sums (vss_grad_sq_partials),
the clip + Adam step (vss_adam_step_clipped), FlatAdam over many steps, and the batched partial-sum
reduction (vss_sum_parts); their write extents behind guard words, and the C ABI's refusals (CPU).

The reference's update that these kernels implement (ppo_continuous_action_isaacgym.py:166, 351-354):
loss.backward(), nn.utils.clip_grad_norm_, optim.Adam(eps=1e-5).step().

Every tolerance below is derived from the kernels' operation counts and fp32's unit roundoff U = 2^-24, or
(the parameter update) from a numpy fp32 restatement of the header's formula measured against the same fp64
reference -- never from what the kernels return.  Figures measured on an MI355X are quoted in
test_adam_one_step_matches_fp64_gpu's docstring and in DESIGN.md §5.7.
"""
import ctypes
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from vss_amd import _native as N

from test_write_extents import SENTINEL, Guarded, _run

DEV = "cuda"
U = 2.0 ** -24  # fp32 unit roundoff: one correctly rounded operation's relative error
F32 = np.float32


def _lib():
    return N.load()


def _st():
    return N.stream_of(torch.device(DEV))


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _count_chunk(n):
    """vss_grad_sq_partials' split: count blocks (chunks of at least 4,096 elements, at most 1,024 of them),
    block b owning [b chunk, (b + 1) chunk) with chunk = ceil(n / count)."""
    count = min(1024, -(-n // 4096))
    return count, -(-n // count)


def _log_uniform_normals(rng, n, decades=7.0):
    """Per-element scales log-uniform in [10^-decades, 1]."""
    return 10.0 ** rng.uniform(-decades, 0.0, n)


def _nonzero_f32(x):
    x = x.astype(F32)
    x[x == 0] = F32(1e-3)
    return x


# ---------------------------------------------------------------------------------------------------------
# 1. vss_grad_sq_partials
# ---------------------------------------------------------------------------------------------------------
SQ_N = [1, 255, 256, 257, 4095, 4096, 4097, 8193, 1_048_575, 1_048_577, 4_194_304, 4_194_304 + 5]


def _sq_partials(g):
    """The kernel's partials of the device tensor g (the buffer starts as NaN: an unwritten partial shows)."""
    lib = _lib()
    n = g.numel()
    count = int(lib.vss_grad_sq_partials_count(n))
    assert count == _count_chunk(n)[0]
    partial = torch.full((count,), float("nan"), device=DEV)
    rc = lib.vss_grad_sq_partials(_st(), n, g.data_ptr(), partial.data_ptr())
    _sync()
    assert rc == 0
    return partial


def _sq_bound_factor(chunk):
    """Relative error bound of one partial in units of U: a thread's ceil(chunk / 256) fused multiply-adds
    (one rounding each), 6 wave-shuffle adds and 3 adds over the waves, all on non-negative terms; + 1."""
    return -(-chunk // 256) + 10


@pytest.mark.gpu
@pytest.mark.parametrize("n", SQ_N)
def test_sq_partials_of_ones_are_the_chunk_lengths_gpu(n):
    """g = 1: every partial is an exact integer in fp32 -- block b's is the length of [b chunk, (b + 1) chunk)
    cut at n (0 for a block past the end), and they add up to n."""
    count, chunk = _count_chunk(n)
    part = _np(_sq_partials(torch.ones(n, device=DEV))).astype(np.float64)
    b = np.arange(count, dtype=np.int64)
    want = np.minimum(n, (b + 1) * chunk) - np.minimum(n, b * chunk)
    assert part.shape == (count,)
    assert np.array_equal(part, want.astype(np.float64)), (part[:4], want[:4], part[-4:], want[-4:])
    assert part.sum() == n


@pytest.mark.gpu
@pytest.mark.parametrize("n", SQ_N)
def test_sq_partials_one_hot_lands_in_its_block_gpu(n):
    """One non-zero at index i (the first element, both sides of the first chunk edge, the last element):
    only partial[i // chunk] is non-zero, and it is g[i]^2."""
    count, chunk = _count_chunk(n)
    g = torch.zeros(n, device=DEV)
    for i in sorted({0, chunk - 1, chunk, n - 1}):
        if not 0 <= i < n:
            continue
        g[i] = 3.0
        part = _np(_sq_partials(g))
        g[i] = 0.0
        want = np.zeros(count, dtype=F32)
        want[i // chunk] = 9.0
        assert np.array_equal(part, want), (n, i, np.nonzero(part)[0][:8], part[np.nonzero(part)[0][:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SQ_N)
def test_sq_partials_match_fp64_chunk_sums_gpu(n):
    """Random g over seven decades against the fp64 sums of g^2 per chunk, within the derived bound
    (ceil(chunk / 256) + 10) U sum (all terms non-negative: the error is relative to the sum itself), and
    the same bits on a repeat."""
    count, chunk = _count_chunk(n)
    rng = np.random.default_rng(100 + n % 9973)
    g = (_log_uniform_normals(rng, n) * rng.standard_normal(n)).astype(F32)
    gd = _dev(g)
    first = _sq_partials(gd)
    again = _sq_partials(gd)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    sq = np.zeros(count * chunk)
    sq[:n] = g.astype(np.float64) ** 2
    want = sq.reshape(count, chunk).sum(1)
    err = np.abs(_np(first).astype(np.float64) - want)
    bound = _sq_bound_factor(chunk) * U * want
    print(f"SQ n={n} max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), (n, float((err / np.maximum(bound, 1e-300)).max()))


# ---------------------------------------------------------------------------------------------------------
# 2. vss_adam_step_clipped: one step from a given state
# ---------------------------------------------------------------------------------------------------------
HP = [(1e-3, 0.9, 0.999, 1e-5), (3e-4, 0.0, 0.99, 1e-8), (2.6e-3, 0.5, 0.9, 0.0)]  # (lr, b1, b2, eps)
HPF = [tuple(float(F32(x)) for x in hp) for hp in HP]  # what the ABI's float arguments receive
STEPS = [1, 2, 3, 10, 1000, 100000]
ADAM_N = [1, 257, 4097, 1_048_577]
CLIPS = ["none", "far", "seventh", "tiny"]


def _adam_cases():
    """The cross product steps x hyper-parameters x clip cases, each at one n: every n for the short
    histories, the small ones where the fp64 history of t - 1 steps would take too long."""
    cases = []
    for k, (t, h, c) in enumerate(itertools.product(STEPS, range(len(HP)), CLIPS)):
        ns = ADAM_N[:2] if t == 100000 else ADAM_N[:3] if t == 1000 else ADAM_N
        cases.append((t, ns[(k + k // 4) % len(ns)], h, c))
    for axis, values in ((0, STEPS), (1, ADAM_N), (2, range(len(HP))), (3, CLIPS)):
        assert {c[axis] for c in cases} == set(values)
    return cases


@functools.lru_cache(maxsize=4)
def _history(t, h, n, decades):
    """(g, m, v) in fp32 for step t: m and v from an fp64 Adam run of t - 1 steps over a seeded gradient
    sequence (element i's gradients: scale_i x standard normals, the scales log-uniform over `decades`
    decades up to 1), rounded to fp32 -- zeros at t = 1 -- and g the sequence's t-th gradient."""
    _, b1, b2, _ = HP[h]
    rng = np.random.default_rng(7000 + n)
    scale = _log_uniform_normals(rng, n, decades)
    m, v = np.zeros(n), np.zeros(n)
    left = t - 1
    while left > 0:
        rows = min(left, max(1, (1 << 18) // n))
        for g in scale * rng.standard_normal((rows, n)):
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
        left -= rows
    g = _nonzero_f32(scale * rng.standard_normal(n))
    return g, m.astype(F32), v.astype(F32)


def _adam_fp64(lr, b1, b2, eps, t, g, p, m, v):
    """Adam's step t in fp64 (the header's formula; hyper-parameters as given)."""
    g, p, m, v = (x.astype(np.float64) for x in (g, p, m, v))
    mi = b1 * m + (1 - b1) * g
    vi = b2 * v + (1 - b2) * g * g
    return p - lr / (1 - b1 ** t) * mi / (np.sqrt(vi) / math.sqrt(1 - b2 ** t) + eps), mi, vi


def _adam_restated_fp32(lr, b1, b2, eps, t, g, p, m, v):
    """The header's formula restated in numpy fp32 from fp32 hyper-parameters, operation by operation (a
    reference for the size of fp32's own error, not the code under test)."""
    lr, b1, b2, eps, one = F32(lr), F32(b1), F32(b2), F32(eps), F32(1)
    bc1 = one - np.power(b1, F32(t), dtype=F32)
    bc2 = one - np.power(b2, F32(t), dtype=F32)
    step_size, bc2_sqrt = F32(lr / bc1), np.sqrt(bc2, dtype=F32)
    mi = b1 * m + (one - b1) * g
    vi = b2 * v + (one - b2) * g * g
    denom = np.sqrt(vi) / bc2_sqrt + eps
    out = p - step_size * mi / denom
    assert out.dtype == F32 and mi.dtype == F32 and vi.dtype == F32
    return out, mi, vi


def _adam_call(g, p, m, v, partial, nparts, max_norm, hpf, t, want_norm=True):
    """vss_adam_step_clipped on device copies of the fp32 arrays; returns (g, p, m, v, norm) afterwards."""
    gd, pd, md, vd = (_dev(x) for x in (g, p, m, v))
    norm = torch.full((1,), float("nan"), device=DEV)
    lr, b1, b2, eps = hpf
    rc = _lib().vss_adam_step_clipped(_st(), g.size, nparts, partial.data_ptr(), max_norm, lr, b1, b2, eps, t,
                                      gd.data_ptr(), pd.data_ptr(), md.data_ptr(), vd.data_ptr(),
                                      norm.data_ptr() if want_norm else None)
    _sync()
    assert rc == 0
    return _np(gd), _np(pd), _np(md), _np(vd), float(norm[0])


def _norm_bound_factor(n, nparts=None):
    """Relative error bound of norm_out in units of U: the partials' (section 1) and the step kernel's sum
    of them (a thread's ceil(nparts / 256) adds + 9 + 1) reach the norm halved through the square root,
    + 2 for sqrtf itself."""
    count, chunk = _count_chunk(n)
    nparts = count if nparts is None else nparts
    return (_sq_bound_factor(chunk) + -(-nparts // 256) + 10) / 2 + 2


def _clipped_reference(g, max_norm_f, norm_f):
    """g min(1, max_norm / (norm + 1e-6)) with the coefficient formed as clip_grad_norm_ forms it, in fp32
    (two correctly rounded operations) from the fp32 norm the kernel reported (pinned to fp64 on its own);
    the products in fp64.  With an fp64 coefficient the kernel's two scalar roundings (up to 2 U) and the
    product's half ulp add up to 2.5 ulp in the worst case, so 2 ulp would not be a derived bound."""
    c = F32(max_norm_f) / (F32(norm_f) + F32(1e-6))
    coef = float(min(c, F32(1)))
    return g.astype(np.float64) * coef, coef


def _assert_within_ulps(got, want64, ulps, what):
    ulp = np.spacing(np.abs(want64.astype(F32))).astype(np.float64)
    d = np.abs(got.astype(np.float64) - want64) / ulp
    assert np.all(d <= ulps), (what, float(d.max()))


def _double_hp_bound(t, g, m0, v0, p64f_abs):
    """|update with the reference's double hyper-parameters - update with their fp32 roundings|, elementwise,
    to first order (x 1.01): lr and eps move by U; b -> fp32(b) moves 1 - b^t by at most
    t |bf - b| b^(t-1) / (1 - b^t) relative (half of b2's reaches the update through the square root), m by
    |b1f - b1| (|m| + |g|) and v by |b2f - b2| (v + g^2)."""
    lr, b1, b2, eps = HP[0]
    lrf, b1f, b2f, epsf = HPF[0]
    g, m0, v0 = (x.astype(np.float64) for x in (g, m0, v0))

    def rel_bc(b, bf):
        top = max(b, bf)
        return t * abs(bf - b) * top ** (t - 1) / (1 - top ** t)

    vi = np.minimum(b2 * v0 + (1 - b2) * g * g, b2f * v0 + (1 - b2f) * g * g)
    dm = abs(b1f - b1) * (np.abs(m0) + np.abs(g))
    dv = abs(b2f - b2) * (v0 + g * g)
    den = np.sqrt(vi) / math.sqrt(1 - min(b2, b2f) ** t) + min(eps, epsf)
    rel = 2 * U + rel_bc(b1, b1f) + 0.5 * rel_bc(b2, b2f) + 0.5 * dv / vi
    return 1.01 * (p64f_abs * rel + max(lr, lrf) / (1 - max(b1, b1f) ** t) * dm / den), rel_bc(b2, b2f)


# The restatement's own max |dp| / lr against fp64 over the whole matrix below (3.7e-6, at t = 2 with
# b2 = 0.999, where 1 - powf(b2, t) has lost ~1e-5 relative to cancellation), rounded up: section 3's tau
# is built from it.
RESTATED_MAX = 5e-6


@pytest.mark.gpu
@pytest.mark.parametrize("t,n,h,clip", _adam_cases())
def test_adam_one_step_matches_fp64_gpu(t, n, h, clip):
    """One vss_adam_step_clipped from a given state (p = 0, so that parameter rounding does not hide the
    update) against an fp64 step with the fp32-rounded hyper-parameters the ABI receives:
      * norm_out against the fp64 norm, within ((K1 + K2) / 2 + 2) U (K1 the partials' bound of section 1,
        K2 = ceil(nparts / 256) + 10 the step kernel's sum of them; halved by the square root; 2 for sqrtf);
      * the gradients afterwards: the input's bits without a clip request, else g x coefficient within 2 ulp
        (also where the coefficient is 1: "far");
      * exp_avg, exp_avg_sq within 3 U (|b m| + |(1 - b) g|) resp. 3 U (b v + (1 - b) g^2): at most three
        roundings on the way to each;
      * the parameter as |dp| / lr, within 4 x the numpy fp32 restatement's own max |dp| / lr against the
        same fp64 step, plus U x |update| / lr.
    For the reference's hyper-parameters the same step is also compared with fp64 Adam on the *double*
    values (0.9, 0.999, 1e-3, 1e-5), within the bound the fp32 roundings of the betas give
    (_double_hp_bound) plus the fp32 terms above.
    The tiny-norm case (norm 1e-5, max_norm 1e-6) draws its scales over two decades instead of seven: scaled
    to that norm and clipped by 11, seven decades would put (1 - b2) g^2 among fp32's denormals, where no
    relative bound holds.

    Measured on an MI355X (|dp| / lr, the largest over the configurations and their elements):
      kernel against fp64 with the fp32 hyper-parameters: 3.66e-6 (t = 2, n = 1,048,577, reference's betas);
      the numpy restatement against the same: 3.66e-6 (the same configuration; in 64 of the 72 configurations
      the two maxima agree to the printed digits, the largest ratio kernel / restatement is 1.6);
      per step count, reference's hyper-parameters, kernel (restatement): t = 1: 2.5e-7 (2.5e-7), 2: 3.7e-6
      (3.7e-6), 3: 3.5e-6 (3.2e-6), 10: 3.5e-7 (3.5e-7), 1000: 1.2e-7 (1.2e-7), 100000: 6.4e-8 (6.4e-8);
      (3e-4, 0, 0.99, 1e-8): at most 1.1e-6 (t = 3); (2.6e-3, 0.5, 0.9, 0): at most 3.0e-7.
      kernel against fp64 Adam on the double hyper-parameters: t = 1: 3.0e-7, 2: 8.3e-6, 10: 6.2e-6,
      1000: 2.7e-6 (fp64 on the fp32 roundings against fp64 on the doubles: 4.8e-8, 5.2e-6, 6.0e-6, 2.7e-6;
      the analysis' bound on 1 - b2^t: 1.29e-5, 1.29e-5, 1.28e-5, 7.5e-6 relative).
    """
    hpf = HPF[h]
    lr, b1, b2, eps = hpf
    g, m0, v0 = _history(t, h, n, 2.0 if clip == "tiny" else 7.0)
    if clip == "tiny":  # the whole history scaled to a gradient norm of 1e-5: there + 1e-6 is 9 % of the coefficient
        s = 1e-5 / math.sqrt(float((g.astype(np.float64) ** 2).sum()))
        g, m0, v0 = _nonzero_f32(g * s), (m0 * s).astype(F32), (v0 * (s * s)).astype(F32)
    norm64 = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    max_norm = {"none": -1.0, "far": 1e6 * norm64, "seventh": norm64 / 7, "tiny": 1e-6}[clip]
    max_norm_f = float(F32(max_norm))
    p0 = np.zeros(n, dtype=F32)
    gd = _dev(g)
    partial = _sq_partials(gd)
    g1, p1, m1, v1, norm = _adam_call(g, p0, m0, v0, partial, partial.numel(), max_norm, hpf, t)

    # 1. the norm
    assert abs(norm - norm64) <= _norm_bound_factor(n) * U * norm64, (norm, norm64)
    # 2. the gradients after the call
    if clip == "none":
        assert np.array_equal(g1.view(np.int32), g.view(np.int32))
    else:
        want, coef = _clipped_reference(g, max_norm_f, norm)
        assert (coef == 1.0) == (clip == "far")
        if clip == "tiny":
            assert abs(coef - 1 / 11) < 1e-3  # 1e-6 / (1e-5 + 1e-6): without the + 1e-6 it would be 1 / 10
        _assert_within_ulps(g1, want, 2, "clipped gradients")
    # 3. the moments, from the gradients the kernel used (checked just above)
    p64, m64, v64 = _adam_fp64(lr, b1, b2, eps, t, g1, p0, m0, v0)
    g64 = g1.astype(np.float64)
    assert np.all(np.abs(m1 - m64) <= 3 * U * (np.abs(b1 * m0.astype(np.float64)) + np.abs((1 - b1) * g64)))
    assert np.all(np.abs(v1 - v64) <= 3 * U * (b2 * v0.astype(np.float64) + (1 - b2) * g64 * g64))
    # 4. the parameter
    pr, _, _ = _adam_restated_fp32(lr, b1, b2, eps, t, g1, p0, m0, v0)
    restated = float(np.abs(pr - p64).max()) / lr
    kernel = np.abs(p1 - p64) / lr
    print(f"ADAM t={t} n={n} hp={h} clip={clip} restated={restated:.3e} kernel={float(kernel.max()):.3e} "
          f"update={float(np.abs(p64).max()) / lr:.3f}")
    assert restated <= RESTATED_MAX
    assert np.all(kernel <= 4 * restated + U * np.abs(p64) / lr), float(kernel.max())
    # the reference's double hyper-parameters
    if h == 0:
        p64d, _, _ = _adam_fp64(*HP[0], t, g1, p0, m0, v0)
        bound, rel_bc2 = _double_hp_bound(t, g1, m0, v0, np.abs(p64))
        gap = np.abs(p1 - p64d)
        print(f"GAP t={t} n={n} clip={clip} kernel_vs_double_hp={float(gap.max()) / lr:.3e} "
              f"fp64_f32hp_vs_double_hp={float(np.abs(p64 - p64d).max()) / lr:.3e} rel_bc2_bound={rel_bc2:.3e}")
        assert np.all(np.abs(p64 - p64d) <= bound)  # the analysis itself
        assert np.all(gap <= bound + lr * 4 * restated + U * np.abs(p64))


@pytest.mark.gpu
def test_adam_step_without_norm_out_gpu():
    """norm_out = NULL: the same step, bit for bit, and nothing else is written in its place."""
    n, t, hpf = 4097, 3, HPF[0]
    g, m0, v0 = _history(t, 0, n, 7.0)
    p0 = np.zeros(n, dtype=F32)
    partial = _sq_partials(_dev(g))
    outs = [_adam_call(g, p0, m0, v0, partial, partial.numel(), 0.5, hpf, t, want_norm=w) for w in (True, False)]
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert math.isfinite(outs[0][4]) and math.isnan(outs[1][4])  # the second call's norm buffer was not passed


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [1, 255, 256, 257, 1024])
def test_adam_step_sums_exactly_nparts_partials_gpu(nparts):
    """Hand-filled partials (quarter integers: their sum is exact in fp32 in any order; dropping or
    repeating one moves it by >= 1e-4 relative) with 1e30 behind the last one: norm_out is sqrt(sum) within
    sqrtf's 2 U, and max_norm = norm / 3 pins the coefficient through the gradients (2 ulp)."""
    n = 257
    vals = (np.arange(1024 + 64) % 7 + 1).astype(F32) * F32(0.25)
    vals[nparts:] = F32(1e30)
    want_norm = math.sqrt(float(vals[:nparts].astype(np.float64).sum()))
    rng = np.random.default_rng(nparts)
    g = _nonzero_f32(rng.standard_normal(n))
    z = np.zeros(n, dtype=F32)
    max_norm = want_norm / 3
    g1, _, _, _, norm = _adam_call(g, z, z, z, _dev(vals), nparts, max_norm, HPF[0], 1)
    assert abs(norm - want_norm) <= 2 * U * want_norm, (norm, want_norm)
    want, coef = _clipped_reference(g, float(F32(max_norm)), norm)
    assert abs(coef - 1 / 3) < 1e-5
    _assert_within_ulps(g1, want, 2, "clipped gradients")


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_adam_step_reports_a_non_finite_norm_gpu(bad):
    """One NaN or inf gradient element (in the second partial block): norm_out is not finite, so a diverged
    run shows in the logged norm.  Nothing is asserted about the parameters."""
    n = 4097
    g = np.full(n, 0.01, dtype=F32)
    g[4096] = bad
    z = np.zeros(n, dtype=F32)
    partial = _sq_partials(_dev(g))
    assert not math.isfinite(float(partial[1])) and math.isfinite(float(partial[0]))
    for max_norm in (0.5, -1.0):
        norm = _adam_call(g, z, z, z, partial, partial.numel(), max_norm, HPF[0], 1)[4]
        assert not math.isfinite(norm), norm


# ---------------------------------------------------------------------------------------------------------
# 3. FlatAdam over many steps
# ---------------------------------------------------------------------------------------------------------
FLAT_STEPS = 300
# the per-step parameter figure of section 2: |dp| / lr of one kernel step against fp64 is at most
# 4 x the restatement's + U x |update| / lr, and Adam's |update| / lr stays below (1 - b1) / sqrt(1 - b2) = 3.2
TAU = 4 * RESTATED_MAX + 4 * U


def _flat_adam_run(G, max_norms, lrs):
    """FlatAdam on Linear(52, 70) + Linear(70, 3) (a FlatGrads layout with gaps) through the gradient rows
    G[k]; max_norms[k] None = no clip request.  Returns the layout's mask, the initial parameters, the
    (p, m, v) snapshots every 50 steps, the norms after the clipped steps and whether every unclipped step
    left its gradients alone."""
    import torch.nn as nn
    from vss_amd.flat import FlatAdam, FlatGrads
    torch.manual_seed(0)
    mod = nn.Sequential(nn.Linear(52, 70), nn.Linear(70, 3)).to(DEV)
    flat = FlatGrads(mod, flat_params=True)
    opt = FlatAdam(flat, lr=lrs[0], eps=1e-5)
    n = flat.flat.numel()
    mask = np.zeros(n, dtype=bool)
    for p in flat.params:
        o = (p.data_ptr() - flat.flat_p.data_ptr()) // 4
        mask[o:o + p.numel()] = True
        assert p.grad.data_ptr() == flat.flat.data_ptr() + 4 * o
    p0 = _np(flat.flat_p).copy()
    snaps, norms, untouched = {}, {}, True
    Gd = None if G is None else _dev(G)
    if G is None:
        return mask, p0, snaps, norms, untouched
    for k in range(G.shape[0]):
        opt.param_groups[0]["lr"] = lrs[k]
        flat.flat.copy_(Gd[k])
        if max_norms[k] is not None:
            flat.clip_norm_(max_norms[k])
            opt.step()
            norms[k] = float(opt.norm[0])
        else:
            opt.step()
            untouched = untouched and torch.equal(flat.flat.view(torch.int32), Gd[k].view(torch.int32))
        if (k + 1) % 50 == 0:
            snaps[k] = tuple(_np(x).copy() for x in (flat.flat_p, opt.exp_avg, opt.exp_avg_sq))
    return mask, p0, snaps, norms, untouched


@pytest.mark.gpu
def test_flat_adam_300_steps_match_fp64_gpu():
    """300 FlatAdam steps on seeded fp32 gradients -- lr lowered through param_groups every 50 steps, the
    clip requested on two steps out of three (max_norm twice the typical norm: coefficient 1; half of it: a
    real clip; then a step without a request) -- against fp64 Adam with clip_grad_norm_ semantics on the
    CPU, fed the same gradients:
      * exp_avg / exp_avg_sq within the accumulated forward bound: each step adds section 2's 3 U term and
        the clipped gradient's own error gamma = (norm bound + 3) U relative (twice that for g^2), and keeps
        b times the bound so far;
      * the parameters within sum over the steps of (U max|p| + lr tau), tau the per-step figure of section 2
        (the moments' accumulated relative error, ~3e-6, is well inside tau);
      * FlatAdam.norm after each clipped step within section 2's norm bound;
      * a step without a clip request right after a clipped one leaves its gradients' bits alone;
      * the gaps of flat_p, exp_avg and exp_avg_sq are exactly 0 at the end; two runs end with the same bits."""
    mask, p0, _, _, _ = _flat_adam_run(None, None, [1e-3])
    n = mask.size
    assert n == 4096 and int(mask.sum()) == 52 * 70 + 70 + 70 * 3 + 3 and not mask.all()
    rng = np.random.default_rng(31)
    scale = _log_uniform_normals(rng, n)
    G = (scale * rng.standard_normal((FLAT_STEPS, n))).astype(F32) * mask
    norms64 = np.sqrt((G.astype(np.float64) ** 2).sum(1))
    typ = float(np.median(norms64))
    max_norms = [(2 * typ, 0.5 * typ, None)[k % 3] for k in range(FLAT_STEPS)]
    lrs = [1e-3 * 0.7 ** (k // 50) for k in range(FLAT_STEPS)]
    _, _, snaps, norms, untouched = _flat_adam_run(G, max_norms, lrs)
    _, _, snaps2, norms2, _ = _flat_adam_run(G, max_norms, lrs)

    _, b1, b2, eps = HPF[0]
    gamma = (_norm_bound_factor(n) + 3) * U
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    bm, bv, bp = np.zeros(n), np.zeros(n), 0.0
    clipped = 0
    for k in range(FLAT_STEPS):
        lr = float(F32(lrs[k]))
        g = G[k].astype(np.float64)
        if max_norms[k] is not None:
            mx = float(F32(max_norms[k]))
            assert abs(norms[k] - norms64[k]) <= _norm_bound_factor(n) * U * norms64[k], (k, norms[k], norms64[k])
            coef = min(1.0, mx / (norms64[k] + 1e-6))
            clipped += coef < 1.0
            g = g * coef
            gerr = gamma
        else:
            gerr = 0.0
        bm = b1 * bm + 3 * U * (np.abs(b1 * m) + np.abs((1 - b1) * g)) + (1 - b1) * gerr * np.abs(g)
        bv = b2 * bv + 3 * U * (b2 * v + (1 - b2) * g * g) + (1 - b2) * 2.01 * gerr * g * g
        p, m, v = _adam_fp64(lr, b1, b2, eps, k + 1, g, p, m, v)
        bp += U * float(np.abs(p).max()) + lr * TAU
        if k in snaps:
            pk, mk, vk = snaps[k]
            print(f"FLAT step {k + 1}: dm/bound {float((np.abs(mk - m)[mask] / bm[mask]).max()):.3f} "
                  f"dv/bound {float((np.abs(vk - v)[mask] / bv[mask]).max()):.3f} "
                  f"dp {float(np.abs(pk - p).max()):.3e} bound {bp:.3e}")
            assert np.all(np.abs(mk - m) <= bm) and np.all(np.abs(vk - v) <= bv), k
            assert np.all(np.abs(pk - p) <= bp), (k, float(np.abs(pk - p).max()), bp)
    assert clipped >= FLAT_STEPS // 3 - 5 and len(norms) == 2 * FLAT_STEPS // 3
    assert untouched  # the deferred clip request applied to one step only
    last = FLAT_STEPS - 1
    for a, b in zip(snaps[last], snaps2[last]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
        assert np.all(a[~mask] == 0)
    assert norms == norms2


# ---------------------------------------------------------------------------------------------------------
# 4. vss_sum_parts
# ---------------------------------------------------------------------------------------------------------
PARTS = [1, 2, 3, 4, 5, 28, 29, 31, 32, 33, 35, 36, 63, 64, 65, 257]
VEC4_SHAPES = [(1, 4), (3, 20), (1, 256), (5, 52), (2, 1028)]
SCALAR_SHAPES = [(1, 3), (3, 30), (85, 3), (5, 30), (34, 30)]  # the same element counts, less the vec-4 tail
LEAD = 64  # sentinel words in front of and behind every dst window


class PartsJob:
    """One vss_sum_parts job: `parts` strided (rows, cols) parts inside a random src buffer (starting
    src_off floats into it) and a dst window (dst_off floats past a 16-B aligned word) inside a buffer of
    sentinel words."""

    def __init__(self, gen, parts, rows, cols, src_ld, dst_ld, pad=0, src_off=0, dst_off=0):
        self.parts, self.rows, self.cols, self.src_ld, self.dst_ld = parts, rows, cols, src_ld, dst_ld
        self.stride = rows * src_ld + pad
        self.src_off = src_off
        self.src_buf = torch.randn(src_off + parts * self.stride + 8, device=DEV, generator=gen)
        self.src_before = self.src_buf.clone()
        self.lo = LEAD + dst_off
        self.dst_buf = torch.full((self.lo + rows * dst_ld + LEAD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.src_ptr = self.src_buf.data_ptr() + 4 * src_off
        self.dst_ptr = self.dst_buf.data_ptr() + 4 * self.lo
        assert self.src_buf.data_ptr() % 16 == 0 and self.dst_buf.data_ptr() % 16 == 0

    def src_view(self):
        return torch.as_strided(self.src_buf, (self.parts, self.rows, self.cols), (self.stride, self.src_ld, 1),
                                self.src_off)

    def window(self):
        return self.dst_buf[self.lo:self.lo + self.rows * self.dst_ld].view(self.rows, self.dst_ld)[:, :self.cols]

    def check(self, what):
        """The window against the fp64 sum, elementwise; src unchanged; every word outside the window's
        columns (the rows' padding, the words in front and behind) still the sentinel."""
        src = self.src_view().double()
        want, scale = src.sum(0), src.abs().sum(0)
        got = self.window().view(torch.float32)
        # a running sum takes ceil(parts / 32) parts, then 3 tree levels over the 8 sums and 2 over the waves
        bound = (-(-self.parts // 32) + 5) * U * scale
        assert bool(((got.double() - want).abs() <= bound).all()), what
        assert torch.equal(self.src_buf, self.src_before), what
        written = torch.zeros_like(self.dst_buf, dtype=torch.bool)
        written[self.lo:self.lo + self.rows * self.dst_ld].view(self.rows, self.dst_ld)[:, :self.cols] = True
        assert bool((self.dst_buf[~written] == SENTINEL).all()), what
        return got.clone()


def _launch_parts_jobs(jobs):
    c = len(jobs)
    Pa, I64 = ctypes.c_void_p * c, ctypes.c_int64 * c
    rc = _lib().vss_sum_parts(_st(), c, Pa(*[j.src_ptr for j in jobs]), Pa(*[j.dst_ptr for j in jobs]),
                              I64(*[j.parts for j in jobs]), I64(*[j.stride for j in jobs]),
                              I64(*[j.rows for j in jobs]), I64(*[j.cols for j in jobs]),
                              I64(*[j.src_ld for j in jobs]), I64(*[j.dst_ld for j in jobs]))
    _sync()
    assert rc == 0


def _parts_jobs(lanes, parts, gen):
    jobs = []
    if lanes == 4:  # cols, leading dimensions and the part stride multiples of 4; 16-B aligned pointers
        for r, c in VEC4_SHAPES:
            jobs.append((f"vec4 {r}x{c} contiguous", PartsJob(gen, parts, r, c, c, c)))
            jobs.append((f"vec4 {r}x{c} strided", PartsJob(gen, parts, r, c, c + 4, c + 8, pad=12)))
    else:
        for r, c in SCALAR_SHAPES:
            jobs.append((f"scalar {r}x{c} contiguous", PartsJob(gen, parts, r, c, c, c)))
            jobs.append((f"scalar {r}x{c} strided", PartsJob(gen, parts, r, c, c + 1, c + 2, pad=3)))
        # vec-4 shaped, but src (then dst) starts 4 bytes past a 16-B boundary: the scalar fallback
        jobs.append(("src + 4 B", PartsJob(gen, parts, 3, 20, 24, 28, pad=12, src_off=1)))
        jobs.append(("dst + 4 B", PartsJob(gen, parts, 3, 20, 24, 28, pad=12, dst_off=1)))
    return jobs


@pytest.mark.gpu
@pytest.mark.parametrize("parts", PARTS)
@pytest.mark.parametrize("lanes", [4, 1])
def test_sum_parts_matches_fp64_and_writes_only_its_window_gpu(lanes, parts):
    """Both lane widths at part counts around the 4-wave x 8-sum unroll (32 parts per trip) and its tail, at
    lengths that end inside a block: every element within (ceil(parts / 32) + 5) U sum|parts| of the fp64
    sum (elementwise), the same bits on a repeat, src unchanged, and every dst a window in sentinel words
    of which only the rows' columns are written (row-strided src and dst together among them)."""
    gen = torch.Generator(device=DEV).manual_seed(1000 * lanes + parts)
    jobs = _parts_jobs(lanes, parts, gen)
    _launch_parts_jobs([j for _, j in jobs])
    first = [j.check(f"{what}, {parts} parts") for what, j in jobs]
    _launch_parts_jobs([j for _, j in jobs])
    for (what, j), f in zip(jobs, first):
        assert torch.equal(j.check(what).view(torch.int32), f.view(torch.int32)), what


@pytest.mark.gpu
def test_sum_parts_70_jobs_in_three_launches_gpu():
    """vss_amd.update.sum_parts with 70 jobs (32 + 32 + 6 per launch, sorted by part count inside): 2-D parts
    into 1-D windows and strided 3-D parts into row-strided windows, every job checked as above."""
    from vss_amd.update import sum_parts
    gen = torch.Generator(device=DEV).manual_seed(70)
    jobs = []
    for k in range(70):
        parts, cols = 1 + (7 * k) % 41, (4, 3, 52, 30, 260)[k % 5]
        if k % 2:
            jobs.append(PartsJob(gen, parts, 1, cols, cols, cols))
        else:
            jobs.append(PartsJob(gen, parts, 2 + k % 3, cols, cols + 4, cols + 8, pad=4))
    pairs = []
    for j in jobs:
        out = j.window().view(torch.float32)
        pairs.append((j.src_view()[:, 0] if j.rows == 1 else j.src_view(), out[0] if j.rows == 1 else out))
    sum_parts(pairs)
    _sync()
    for k, j in enumerate(jobs):
        j.check(f"job {k}")


# ---------------------------------------------------------------------------------------------------------
# 5. write extents (GPU) and refusals (CPU)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1_048_577, 257])
def test_optim_entries_write_only_their_outputs_gpu(n):
    """vss_grad_sq_partials reads g and writes exactly `count` partials; vss_adam_step_clipped leaves the
    partials (and, without a clip request, the gradients) alone and writes exactly n elements of p, m and v
    (and of g when it clips) and one float of norm_out: p = m = v = 0 before and g != 0, so a written
    element is non-zero afterwards, and the guard words on both sides of every buffer stay intact."""
    lib, st = _lib(), _st()
    rng = np.random.default_rng(n)
    g0 = _nonzero_f32(rng.standard_normal(n) * 0.1)
    count = int(lib.vss_grad_sq_partials_count(n))
    for clip in (False, True):
        g = Guarded((n,), fill=_dev(g0))
        partial = Guarded((count,))
        _run("vss_grad_sq_partials", lambda: lib.vss_grad_sq_partials(st, n, g.ptr, partial.ptr), [g], [partial],
             [partial])
        p, m, v = (Guarded((n,), fill=torch.zeros(n, device=DEV)) for _ in range(3))
        norm = Guarded((1,))
        max_norm = 0.25 if clip else -1.0  # the norm is ~0.1 sqrt(n) >= 1.6: a real clip
        lr, b1, b2, eps = HPF[0]
        _run(f"vss_adam_step_clipped clip={clip}",
             lambda: lib.vss_adam_step_clipped(st, n, count, partial.ptr, max_norm, lr, b1, b2, eps, 1, g.ptr, p.ptr,
                                               m.ptr, v.ptr, norm.ptr),
             [partial] + ([] if clip else [g]), [g, p, m, v, norm], [norm])
        for name, buf in (("p", p), ("m", m), ("v", v)):
            assert bool((buf.t != 0).all()), f"{name}: not every element written"
        if clip:
            assert bool((g.t != _dev(g0)).all()) and bool((g.t != 0).all()), "g: not every element clipped"
        assert math.isfinite(float(norm.t[0]))


E_ARG = 1
FAKE = 4096  # a pointer that is never dereferenced: every call below is refused before any launch


def test_grad_sq_partials_count_and_refusals_cpu():
    lib = _lib()
    assert lib.vss_grad_sq_partials_count(0) == -1 and lib.vss_grad_sq_partials_count(-5) == -1
    for n, want in ((1, 1), (4096, 1), (4097, 2), (4_194_304, 1024), (2 ** 33, 1024)):
        assert lib.vss_grad_sq_partials_count(n) == want == _count_chunk(n)[0]
    for n in (0, -1):
        assert lib.vss_grad_sq_partials(None, n, FAKE, FAKE) == E_ARG
    assert lib.vss_grad_sq_partials(None, 16, None, FAKE) == E_ARG
    assert lib.vss_grad_sq_partials(None, 16, FAKE, None) == E_ARG


def test_adam_step_refusals_cpu():
    lib = _lib()
    nan = float("nan")
    good = dict(n=16, nparts=1, partial=FAKE, max_norm=0.5, lr=1e-3, b1=0.9, b2=0.999, eps=1e-5, step=1, g=FAKE,
                p=FAKE, m=FAKE, v=FAKE, norm=None)
    bad = [dict(n=0), dict(n=-3), dict(nparts=0), dict(nparts=1025), dict(step=0), dict(eps=-1e-8), dict(eps=nan),
           dict(b1=1.0), dict(b1=-0.1), dict(b1=nan), dict(b2=1.0), dict(b2=-0.1), dict(b2=nan), dict(partial=None),
           dict(g=None), dict(p=None), dict(m=None), dict(v=None)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.vss_adam_step_clipped(None, a["n"], a["nparts"], a["partial"], a["max_norm"], a["lr"], a["b1"],
                                       a["b2"], a["eps"], a["step"], a["g"], a["p"], a["m"], a["v"], a["norm"])
        assert rc == E_ARG, change


def test_sum_parts_refusals_cpu():
    lib = _lib()

    def call(count=1, n_arrays=None, null=None, **change):
        c = max(1, min(count, 40)) if n_arrays is None else n_arrays
        a = dict(src=FAKE, dst=2 * FAKE, parts=2, stride=8, rows=2, cols=4, src_ld=4, dst_ld=4)
        a.update(change)
        Pa, I64 = ctypes.c_void_p * c, ctypes.c_int64 * c
        arrays = [Pa(*[a["src"]] * c), Pa(*[a["dst"]] * c)] + [I64(*[a[k]] * c) for k in
                                                             ("parts", "stride", "rows", "cols", "src_ld", "dst_ld")]
        if null is not None:
            arrays[null] = None
        return lib.vss_sum_parts(None, count, *arrays)

    assert call(count=0) == E_ARG and call(count=33) == E_ARG and call(count=-1) == E_ARG
    for k in range(8):
        assert call(null=k) == E_ARG, k
    for change in (dict(src=None), dict(dst=None), dict(parts=0), dict(rows=0), dict(cols=0), dict(rows=-1),
                   dict(src_ld=3), dict(dst_ld=3),
                   dict(stride=7),  # 2 x 4 contiguous rows need 8: the second part would start inside the first
                   dict(src_ld=6, stride=9),  # rows x src_ld less the last row's padding = 10
                   dict(parts=1, rows=1 << 30, cols=3, src_ld=3, dst_ld=3)):  # 3 x 2^30 / 64 blocks > 2^24
        assert call(**change) == E_ARG, change
    # the block total is taken over the jobs: 32 jobs of 2^19 + 1 blocks each pass 2^24 at the last one
    rows = (1 << 19) + 1
    assert call(count=32, parts=1, rows=rows, cols=256, src_ld=256, dst_ld=256) == E_ARG
