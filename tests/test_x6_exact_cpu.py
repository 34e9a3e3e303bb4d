"""tests/x6_exact.py without a GPU: the split is exact at its edges, both operand families meet the exactness
condition at every shape the GPU tests launch, and the statement `six` is sensitive -- each defect the GPU
comparison is meant to see (a dropped or mis-paired plane product, a shifted K position, a row in the wrong
contraction part) changes the stated share of outputs."""
import numpy as np
import pytest

import x6_exact as X

F32 = np.float32


def _pow2_floor(v):
    return np.ldexp(1.0, np.frexp(np.abs(v).astype(np.float64))[1] - 1)   # 2^e with 2^e <= |v| < 2^(e+1)


def _check_split(v):
    hi, mid, lo = X.split3(v)                       # asserts hi + mid + lo == v and that lo is a bf16
    assert X.is_bf16(hi).all() and X.is_bf16(mid).all()
    nz = v != 0
    e = _pow2_floor(v[nz])
    r1 = v.astype(np.float64) - hi
    assert (np.abs(r1[nz]) <= 2.0 ** -8 * e).all()           # hi is a nearest bf16: within half its ulp
    assert (np.abs(mid[nz]) <= 2.0 ** -8 * e).all()
    assert (np.abs(lo[nz]).astype(np.float64) <= 2.0 ** -16 * e).all()
    assert (hi[~nz] == 0).all() and (mid[~nz] == 0).all() and (lo[~nz] == 0).all()
    return hi, mid, lo


def test_split3_known_values_cpu():
    """RNE ties at the hi and the mid step, residuals of either sign, +-0, powers of two."""
    u = 2.0 ** -7  # a bf16 ulp at 1
    table = [
        # v,                              hi,            mid,                     lo
        (1.0,                             1.0,           0.0,                     0.0),
        (1 + u / 2,                       1.0,           u / 2,                   0.0),          # tie -> even (down)
        (1 + 3 * u / 2,                   1 + 2 * u,     -u / 2,                  0.0),          # tie -> even (up)
        (1 + u / 2 + 2.0 ** -23,          1 + u,         -u / 2,                  2.0 ** -23),   # just above the tie
        (1 + u / 2 - 2.0 ** -23,          1.0,           u / 2,                   -2.0 ** -23),  # just below it
        (1 + 2.0 ** -9 + 2.0 ** -17,      1.0,           2.0 ** -9,               2.0 ** -17),   # mid tie -> even (down)
        (1 + 2.0 ** -9 + 3 * 2.0 ** -17,  1.0,           2.0 ** -9 + 2.0 ** -15,  -2.0 ** -17),  # mid tie -> even (up)
        (1 - 2.0 ** -10,                  1.0,           -2.0 ** -10,             0.0),          # negative residual
        (1.5 - 1.5 * 2.0 ** -9 + 1.5 * 2.0 ** -18, 1.5,  -1.5 * 2.0 ** -9,        1.5 * 2.0 ** -18),
        (2.0 ** -100,                     2.0 ** -100,   0.0,                     0.0),
        (2.0 ** 100,                      2.0 ** 100,    0.0,                     0.0),
    ]
    v = np.array([r[0] for r in table], np.float64)
    assert np.array_equal(v.astype(F32).astype(np.float64), v), "the table's values must be fp32"
    for sign in (1.0, -1.0):
        hi, mid, lo = _check_split((sign * v).astype(F32))
        for c, got in enumerate((hi, mid, lo), 1):
            assert np.array_equal(got.astype(np.float64), sign * np.array([r[c] for r in table])), c
    z = np.array([0.0, -0.0], F32)
    for part in X.split3(z):
        assert (part == 0).all()
    assert np.array_equal(X.bf16_rne(z).view(np.uint32), z.view(np.uint32))  # the sign of zero is kept


def test_split3_around_every_bf16_and_random_cpu():
    """One fp32 ulp either side of bf16 values across the exponent range (residuals of both signs, hi next to
    a binade edge), and random fp32 values of many magnitudes."""
    rng = np.random.default_rng(0)
    b = (rng.integers(0, 1 << 16, 20000, dtype=np.uint32) << np.uint32(16)).view(F32)
    b = b[np.isfinite(b) & (np.abs(b) > 2.0 ** -100) & (np.abs(b) < 2.0 ** 100)]
    pow2 = np.ldexp(F32(1), np.arange(-100, 101)).astype(F32)
    for base in (b, pow2, -pow2):
        for v in (base, np.nextafter(base, F32(np.inf)), np.nextafter(base, F32(-np.inf))):
            hi, mid, lo = _check_split(v)
        assert np.array_equal(X.split3(base)[0], base)
    v = (rng.standard_normal(1 << 20) * np.ldexp(1.0, rng.integers(-60, 60, 1 << 20))).astype(F32)
    _, mid, lo = _check_split(v)
    assert (mid > 0).any() and (mid < 0).any() and (lo > 0).any() and (lo < 0).any()


def test_three_plane_values_split_into_their_parts_cpu():
    """split3 returns exactly (h, m, l): all three planes carry data, every magnitude and sign occurs."""
    v, h, m, l = X.three_plane_values(1 << 16, 1)
    hi, mid, lo = X.split3(v)
    assert np.array_equal(hi, h) and np.array_equal(mid, m) and np.array_equal(lo, l)
    assert set(np.abs(h)) == {1.0, 1.5} and set(np.abs(m) * 2 ** 9) == {1.0, 1.5} and set(np.abs(l) * 2 ** 18) == {1.0, 1.5}
    for part in (h, m, l):
        assert (part > 0).any() and (part < 0).any()
    assert len(np.unique(v)) == 36  # 4 h x (2 + 4) / 2 m x ... : the sign rule leaves 36 values


def test_sparse_positions_cover_every_k_and_tile_cpu():
    for k in X.FB_K + (256,):
        pos = X.sparse3_positions(4 * k, k)
        for s in range(3):
            assert set(pos[:, s]) == set(range(k))   # each of the three nonzeros visits every K position
        S = X.sparse3(4 * k, k, 2)
        assert ((S != 0).sum(1) == 3).all()
        for plane in X.split3(S):
            assert (plane != 0).any(0).all()          # every K position of every plane is hit


@pytest.mark.parametrize("q_dense", [False, True])
@pytest.mark.parametrize("k", X.FB_K)
@pytest.mark.parametrize("n,rows", X.FB_MULTI + X.FB_SINGLE)
def test_three_plane_family_is_exact_at_the_gpu_shapes_cpu(n, rows, k, q_dense):
    bound = X.assert_exact(*X.fb_operands(n, rows, k, q_dense))
    assert bound <= 6.78


@pytest.mark.parametrize("x_dense", [False, True])
@pytest.mark.parametrize("rows", X.WG_ROWS)
@pytest.mark.parametrize("n_out,k_in", X.WG_SHAPES + tuple((256, k) for k in X.FW_K_IN))
def test_three_plane_family_is_exact_at_the_weight_grad_shapes_cpu(n_out, k_in, rows, x_dense):
    parts = X.fw_parts(rows) if k_in <= 64 else X.wg_parts(rows, n_out, k_in)
    starts = X.part_starts(rows, parts)
    assert starts[0] == 0 and starts[-1] == rows and len(set(np.diff(starts))) == 2  # uneven: two part lengths
    x, g = X.wg_operands(rows, n_out, k_in, starts, x_dense)
    assert X.assert_exact_parts(x, g, starts) <= 6.78


@pytest.mark.parametrize("k", [64, 512])
@pytest.mark.parametrize("n,rows", X.FB_MULTI + X.FB_SINGLE)
def test_integer_family_is_exact_at_the_gpu_shapes_cpu(n, rows, k):
    g, wt, y = X.int_backward(rows, k, n, 3)
    X.assert_exact_int(g, wt, y)
    assert set(np.unique(y)) == {0.0, 0.5, -0.5, 1.0, -1.0}
    assert (X.split3(wt)[1] != 0).any()   # the weights reach past 8 bits: their mid plane carries data


def test_the_conditions_refuse_what_is_not_exact_cpu():
    P, Q = X.fb_operands(256, 512, 256, False)
    with pytest.raises(AssertionError):
        X.assert_exact(P, X.dense3(Q.shape, 5))                 # dense x dense: the sums leave the window
    with pytest.raises(AssertionError):
        X.assert_exact(P * F32(1 + 2.0 ** -12), Q)              # terms below 2^-20
    with pytest.raises(AssertionError):
        X.assert_exact(P * F32(2), Q * F32(2))                  # |terms| up to 27
    g, wt, y = X.int_backward(4096, 64, 256, 3)
    with pytest.raises(AssertionError):
        X.assert_exact_int(g, wt, np.full_like(y, 0.25))        # 1 - y^2 = 0.9375
    with pytest.raises(AssertionError):
        X.assert_exact_int(np.ones((98432, 64), F32), wt, np.zeros((98432, 256), F32))  # column sums past 2^24


# ---- the statement and its mutations, at J = 512, K = 256, I = 256 ------------------------------------------

J, K, I = 512, 256, 256


@pytest.fixture(scope="module", params=[False, True], ids=["q_sparse", "q_dense"])
def stated(request):
    P, Q = X.fb_operands(I, J, K, request.param)
    X.assert_exact(P, Q)
    return P, Q, X.six(P, Q)


def test_six_is_fp32_and_differs_from_nine_cpu(stated):
    P, Q, want = stated
    assert X.fp32_representable(want)
    assert np.array_equal(want / X.QUANTUM, np.rint(want / X.QUANTUM)) and np.abs(want).max() < X.WINDOW
    full = X.nine(P, Q)
    assert np.array_equal(full, Q.astype(np.float64) @ P.astype(np.float64).T)  # nine IS the fp64 product
    assert (full.astype(F32) != want.astype(F32)).mean() >= 0.05                # and rounds elsewhere


@pytest.mark.parametrize("drop", range(6))
def test_a_dropped_product_changes_every_output_cpu(stated, drop):
    P, Q, want = stated
    got = X.plane_sum(P, Q, [p for q, p in enumerate(X.SIX) if q != drop])
    assert (got != want).all()


def test_a_mispaired_plane_changes_most_outputs_cpu(stated):
    P, Q, want = stated
    for wrong, right in (((0, 1), (1, 0)), ((1, 0), (0, 1)), ((0, 2), (2, 0)), ((2, 0), (0, 2))):
        pairs = [wrong if p == right else p for p in X.SIX]     # e.g. mid.hi computed as hi.mid
        assert (X.plane_sum(P, Q, pairs) != want).mean() > 0.5


def _shifted(S, vector, src, dst):
    T = S.copy()
    assert T[vector, src] != 0 and T[vector, dst] == 0
    T[vector, dst], T[vector, src] = T[vector, src], 0
    return T


@pytest.mark.parametrize("across_tile", [False, True])
def test_a_shifted_nonzero_changes_its_vectors_outputs_cpu(stated, across_tile):
    """One nonzero of the sparse operand moved by one K position, within a K tile and across a tile boundary
    (31 -> 32): only its contraction vector's outputs change, and (up to the dense operand holding the same value
    at both positions, 1 chance in 36) all of them."""
    P, Q, want = stated
    q_sparse = np.count_nonzero(Q) < np.count_nonzero(P)
    S = Q if q_sparse else P
    vec, src = next((v, t) for v, t in zip(*np.nonzero(S)) if (t % 32 == 31) == across_tile and t + 1 < K
                    and S[v, t + 1] == 0)
    T = _shifted(S, vec, src, src + 1)
    got = X.six(P, T) if q_sparse else X.six(T, Q)
    diff = got != want
    line = diff[vec] if q_sparse else diff[:, vec]
    assert diff.sum() == line.sum() and line.mean() > 0.9


@pytest.mark.parametrize("x_dense", [False, True])
def test_a_pair_in_the_neighbouring_part_changes_both_parts_cpu(x_dense):
    """The weight gradient's partition: the statement over parts whose boundary is one K-tile pair (64 rows) off
    differs in the two parts that meet there, and nowhere else."""
    rows, n_out, k_in, parts = 64 * 37, 256, 128, 8
    starts = X.part_starts(rows, parts)
    x, g = X.wg_operands(rows, n_out, k_in, starts, x_dense)
    X.assert_exact_parts(x, g, starts)
    want = X.six_parts(x, g, starts)
    assert want.shape == (parts, n_out, k_in) and X.fp32_representable(want)
    for s in range(1, parts):
        for step in (64, -64):
            moved = starts.copy()
            moved[s] += step
            diff = (X.six_parts(x, g, moved) != want).reshape(parts, -1).any(1)
            assert diff[s - 1] and diff[s] and diff.sum() == 2
