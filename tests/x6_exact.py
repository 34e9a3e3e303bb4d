"""The x6 GEMMs' arithmetic as a host statement, and operand families on which it is exact.

Plain numpy, no GPU and no built library.  csrc/vss_gemm_x6.hip splits every fp32 operand into three bf16
planes and sums six of the nine plane products in an fp32 accumulator on the matrix core:

    hi = bf16_rne(v),  mid = bf16_rne(v - hi),  lo = v - hi - mid          (split3, the kernel's split8)
    D[j][i] = sum over t of  hh + (hm + mh) + (hl + mm + lh)               (six;  nine adds ml + lm + ll)

How the matrix core rounds is not modelled.  The families below are chosen so that every term is a multiple
of 2^-20 and the absolute terms of an output sum to less than 8: every partial sum, in any order and in any
grouping, then fits fp32's 24 bits, nothing is ever rounded, and the kernel must return `six` bit for bit.

  three-plane family   v = h + m + l with |h| in {1, 1.5}, |m| in {1, 1.5} 2^-9, |l| in {1, 1.5} 2^-18, so
                       that split3(v) = (h, m, l): all three planes of both operands carry data.  A part
                       whose magnitude is the power of two takes the sign of the next larger part (otherwise
                       the larger part would be rounded across a binade and gain bits).  One operand is dense
                       in such values, the other holds exactly 3 of them per contraction vector.
  integer family       for the backward's (1 - y^2) factor and column sums: small integers and
                       y in {0, +-0.5, +-1}, so that 1 - y^2 is 1, 0.75 or 0.

assert_exact / assert_exact_parts / assert_exact_int state the exactness CONDITION on given operands (they
measure nothing of the kernel); the GPU tests call them on what they launch."""
import numpy as np

U32 = np.uint32
QUANTUM = 2.0 ** -20   # every term of an exact family is a multiple of this
WINDOW = 8.0           # and an output's absolute terms sum to less than this: 23 bits in all

# Shapes.  A forward / backward block runs a second work item only when the row tiles outnumber the blocks per
# feature tile (about 256 blocks in all): (n, rows), the smallest such row counts for the 256-feature block
# (n % 256 == 0: 128-row tiles) and the 128-feature block (n = 128, 384: 256-row tiles), and one single-item
# control per block shape.  The GPU tests assert from the library's own counts that they are what they claim.
FB_MULTI = ((256, 49152), (256, 98432), (512, 24704), (128, 65792), (384, 20736))
FB_SINGLE = ((256, 8192), (128, 8192))
FB_K = (64, 128, 512)   # k = 64: an item is one K-tile pair
# weight gradient: (n_out, k_in); row counts with a prime number of K-tile pairs, so the parts are uneven
WG_SHAPES = ((256, 128), (512, 512), (256, 384), (512, 384))
WG_ROWS = (64 * 257, 64 * 1025)
FW_K_IN = (52, 4, 64)   # the first layer's weight gradient (n_out = 256)


def wg_parts(rows, n_out, k_in):
    """Contraction parts of vss_weight_grad_bf16x6 (csrc/vss_gemm_x6.hip wg_plan): enough for the 128 x 256 output
    tiles to fill 256 blocks, at most one per K-tile pair.  The GPU tests compare it with the library's count."""
    return max(1, min(256 // ((k_in // 128) * (n_out // 256)), rows // 64))


def fw_parts(rows):
    """Parts of vss_first_weight_grad_bf16x6 (fw_parts): 8 K-tile pairs per block, at most 256 blocks."""
    return max(1, min(rows // 64 // 8, 256))


# the kept plane products (P's plane, Q's plane): 0 = hi, 1 = mid, 2 = lo
SIX = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))
NINE = SIX + ((1, 2), (2, 1), (2, 2))


def bf16_rne(v):
    """v (fp32) rounded to the nearest bf16, ties to even, as an fp32 array (finite values)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(U32)
    r = (u + U32(0x7FFF) + ((u >> U32(16)) & U32(1))) & U32(0xFFFF0000)
    return r.view(np.float32)


def is_bf16(v):
    return (np.ascontiguousarray(v, dtype=np.float32).view(U32) & U32(0xFFFF)) == 0


def split3(v):
    """(hi, mid, lo) fp32 arrays with hi + mid + lo == v exactly and each a bf16 (the kernel's split8)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    hi = bf16_rne(v)
    r1 = v - hi          # exact in fp32: at most 16 significant bits
    mid = bf16_rne(r1)
    lo = r1 - mid        # exact: at most 8 significant bits
    assert is_bf16(lo).all(), "split3: lo is not a bf16"
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64),
                          v.astype(np.float64)), "split3: hi + mid + lo != v"
    return hi, mid, lo


def plane_sum(P, Q, pairs=SIX):
    """out[j][i] = sum over t and over the (a, b) of `pairs` of P_a[i][t] Q_b[j][t], in fp64.  P (I, K), Q (J, K)."""
    pp = [x.astype(np.float64) for x in split3(P)]
    qq = [x.astype(np.float64) for x in split3(Q)]
    out = np.zeros((Q.shape[0], P.shape[0]), np.float64)
    for a, b in pairs:
        out += qq[b] @ pp[a].T
    return out


def six(P, Q):
    return plane_sum(P, Q, SIX)


def nine(P, Q):
    return plane_sum(P, Q, NINE)


def fp32_representable(x):
    return np.array_equal(x.astype(np.float32).astype(np.float64), x)


# ---- the three-plane family -------------------------------------------------------------------------------

def three_plane_values(count, seed):
    """(v, h, m, l): `count` values of the family (fp32) and the parts they were built from."""
    c = np.random.default_rng(seed).integers(0, 64, count, dtype=np.int64)
    bh, sh, bm, fm, bl, fl = [(c >> i) & 1 for i in range(6)]
    sm = np.where(bh == 1, fm, sh)   # m's sign is free only where |h| = 1.5
    sl = np.where(bm == 1, fl, sm)   # l's sign is free only where |m| = 1.5 2^-9
    h = ((1 - 2 * sh) * (1 + 0.5 * bh)).astype(np.float32)
    m = ((1 - 2 * sm) * (1 + 0.5 * bm) * 2.0 ** -9).astype(np.float32)
    l = ((1 - 2 * sl) * (1 + 0.5 * bl) * 2.0 ** -18).astype(np.float32)
    return (h + m) + l, h, m, l      # exact: 20 significant bits


TABLE = 1048583  # a prime above 2^20: the dense operand repeats a table with this period over its flat index


def dense3(shape, seed):
    """A dense operand of the family.  Flat element e is entry e mod TABLE of a seeded table; the period
    is prime and exceeds every row count in use, so no two rows of an operand are equal."""
    return np.resize(three_plane_values(min(TABLE, int(np.prod(shape))), seed)[0], shape)


def sparse3_positions(vectors, k):
    """(vectors, 3): the nonzero K positions of contraction vector j, (7 j + 83 s) mod k."""
    j = np.arange(vectors, dtype=np.int64)[:, None]
    return (7 * j + 83 * np.arange(3, dtype=np.int64)[None, :]) % k


def sparse3(vectors, k, seed):
    """(vectors, k) fp32 with exactly 3 family values per row, at sparse3_positions."""
    pos = sparse3_positions(vectors, k)
    assert (pos[:, 0] != pos[:, 1]).all() and (pos[:, 0] != pos[:, 2]).all() and (pos[:, 1] != pos[:, 2]).all()
    if k >= 96:
        t = pos // 32
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    out = np.zeros((vectors, k), np.float32)
    out[np.arange(vectors)[:, None], pos] = np.resize(three_plane_values(min(TABLE, 3 * vectors), seed)[0], (vectors, 3))
    return out


def part_starts(rows, parts):
    """The weight gradient's partition (include/vss.h, csrc/vss_gemm_x6.hip kt_lo): part s takes the K-tile
    pairs [s kpairs / parts, (s + 1) kpairs / parts), i.e. the rows 64 times that; (parts + 1,) row offsets."""
    pairs = rows // 64
    return 64 * (np.arange(parts + 1, dtype=np.int64) * pairs // parts)


def sparse3_parts_rows(cols, starts):
    """(parts, cols, 3): the rows of column c's nonzeros in part s.  Nonzero u of column c sits in the part's
    K-tile pair (3 c + u + s) mod pairs, at row (7 c + 19 u + 5 s) mod 64 of it: the nonzeros move through the
    part's pairs and through a pair's rows (both K tiles), and with 3 cols >= pairs every pair holds one."""
    lo, pairs = starts[:-1, None, None], np.diff(starts)[:, None, None] // 64
    c = np.arange(cols, dtype=np.int64)[None, :, None]
    s = np.arange(len(starts) - 1, dtype=np.int64)[:, None, None]
    u = np.arange(3, dtype=np.int64)[None, None, :]
    return lo + 64 * ((3 * c + u + s) % pairs) + (7 * c + 19 * u + 5 * s) % 64


def sparse3_parts(rows, cols, starts, seed):
    """(rows, cols) fp32 whose contraction index is its row: exactly 3 family values per column in each
    part of `starts`; every K-tile pair (64 rows) holds one, so a pair in the wrong part changes outputs."""
    r = sparse3_parts_rows(cols, starts)
    assert (r[..., 0] != r[..., 1]).all() and (r[..., 0] != r[..., 2]).all() and (r[..., 1] != r[..., 2]).all()
    out = np.zeros((rows, cols), np.float32)
    out[r, np.arange(cols)[None, :, None]] = np.resize(three_plane_values(min(TABLE, r.size), seed)[0], r.shape)
    assert (out.reshape(rows // 64, -1) != 0).any(1).all(), "a K-tile pair without a nonzero"
    return out


def fb_operands(n, rows, k, q_dense, seed=0):
    """Forward / backward operands (P (n, k): the weight, Q (rows, k): the activations or gradients): one dense
    in the family, the other with 3 of its values per contraction vector.  q_dense = False puts the dense data
    through the weight-plane path, True through the register-staged path."""
    if q_dense:
        return sparse3(n, k, seed + 1), dense3((rows, k), seed + 2)
    return dense3((n, k), seed + 1), sparse3(rows, k, seed + 2)


def wg_operands(rows, n_out, k_in, starts, x_dense, seed=0):
    """Weight-gradient operands (x (rows, k_in), grad (rows, n_out)) for the parts of `starts`."""
    if x_dense:
        return dense3((rows, k_in), seed + 1), sparse3_parts(rows, n_out, starts, seed + 2)
    return sparse3_parts(rows, k_in, starts, seed + 1), dense3((rows, n_out), seed + 2)


# ---- the exactness condition --------------------------------------------------------------------------------

def _value_stats(X):
    """Per plane, over the DISTINCT values of X (an operand has few): (largest magnitude, the largest power of
    two dividing every entry; inf for a zero plane)."""
    vals = np.unique(np.ascontiguousarray(X, dtype=np.float32).reshape(-1).view(U32)).view(np.float32)
    gmax, quantum = [], []
    for x in split3(vals):
        x = np.abs(x[x != 0]).astype(np.float64)
        if x.size == 0:
            gmax.append(0.0)
            quantum.append(float("inf"))
            continue
        m, e = np.frexp(x)                      # x = m 2^e, m in [0.5, 1) with at most 8 bits (a bf16)
        mi = (m * 256).astype(np.int64)
        assert np.array_equal(mi / 256.0, m)
        gmax.append(float(x.max()))
        quantum.append(float(np.min(np.ldexp((mi & -mi).astype(np.float64), e - 8))))
    return gmax, quantum


def _vector_l1(X, vector_of, vectors):
    """(vectors, 3): per contraction vector and plane, the sum of |plane| over the vector's entries;
    vector_of(flat indices of X's nonzeros) names each entry's vector."""
    flat = np.ascontiguousarray(X, dtype=np.float32).reshape(-1)
    idx = np.flatnonzero(flat)
    vec = vector_of(idx)
    return np.stack([np.bincount(vec, np.abs(x).astype(np.float64), minlength=vectors) for x in split3(flat[idx])], 1)


# the six products grouped by one operand's plane: its hi meets the other's hi + mid + lo, its mid hi + mid,
# its lo hi (SIX is symmetric in the two operands)
_GROUP = ((0, 1, 2), (0, 1), (0,))


def _assert_condition(sides):
    """sides: two (X, vector_of, vectors), one per operand.  Every term a multiple of 2^-20; and for every output
    sum |terms| < 8, bounded as: one operand's per-vector plane sums times the other's largest plane
    magnitudes (an upper bound of every output's own sum; either operand may play the first part, the one with
    fewer nonzeros is tried first).  Returns the bound that held."""
    stats = [_value_stats(s[0]) for s in sides]
    for a, b in SIX:
        q = stats[0][1][a] * stats[1][1][b]
        assert q >= QUANTUM, f"plane product ({a}, {b}) is a multiple of {q} only, not of 2^-20"
    bounds = []
    for me in sorted((0, 1), key=lambda s: np.count_nonzero(sides[s][0])):
        l1, other = _vector_l1(*sides[me]), stats[1 - me][0]
        per_vector = sum(l1[:, a] * sum(other[b] for b in _GROUP[a]) for a in range(3))
        bounds.append(float(per_vector.max()))
        if bounds[-1] < WINDOW:
            return bounds[-1]
    raise AssertionError(f"sum |terms| may reach {min(bounds)} >= 8")


def assert_exact(P, Q):
    """The condition under which D[j][i] = sum_t P[i][t] Q[j][t] over the six products is exact in fp32 in any
    order and grouping.  P (I, K), Q (J, K); a contraction vector is a row.  Returns the bound on sum |terms|."""
    assert P.ndim == 2 and Q.ndim == 2 and P.shape[1] == Q.shape[1]
    k = P.shape[1]
    return _assert_condition([(X, lambda idx: idx // k, X.shape[0]) for X in (P, Q)])


def assert_exact_parts(Pt, Qt, starts):
    """assert_exact for operands whose contraction index is their ROW, Pt (T, I) and Qt (T, J), summed
    separately over the row ranges of `starts` (the weight gradient's parts): a contraction vector is
    (part, column).  Returns the bound."""
    assert Pt.ndim == 2 and Qt.ndim == 2 and Pt.shape[0] == Qt.shape[0] == starts[-1] and starts[0] == 0
    parts = len(starts) - 1

    def side(X):
        c = X.shape[1]
        return X, lambda idx: (np.searchsorted(starts, idx // c, "right") - 1) * c + idx % c, parts * c
    return _assert_condition([side(Pt), side(Qt)])


def six_parts(Pt, Qt, starts, pairs=SIX):
    """(parts, J, I) fp64: plane_sum over each part's rows (the weight gradient's partials)."""
    return np.stack([plane_sum(np.ascontiguousarray(Pt[lo:hi].T), np.ascontiguousarray(Qt[lo:hi].T), pairs)
                     for lo, hi in zip(starts[:-1], starts[1:])])


# ---- the integer family (the backward's epilogue) -------------------------------------------------------------

W_INT = 300  # the weights' range, the scale of tests/test_gemm_x6.py's integer test


def int_backward(rows, k_next, n, seed):
    """(g, wt, y): g (rows, k_next) with 3 entries of +-1 per row, wt (n, k_next) integers in +-300 (beyond a
    bf16's 8 bits: the mid plane carries data), y (rows, n) in {0, +-0.5, +-1} with shares 1/64, 2/64, 61/64:
    most gradients vanish, which keeps the column sums over ~10^5 rows inside fp32."""
    rng = np.random.default_rng(seed)
    pos = sparse3_positions(rows, k_next)
    g = np.zeros((rows, k_next), np.float32)
    g[np.arange(rows)[:, None], pos] = np.resize(rng.integers(0, 2, TABLE, dtype=np.int8) * 2 - 1, (rows, 3))
    wt = rng.integers(-W_INT, W_INT + 1, (n, k_next)).astype(np.float32)
    lut = np.array([0.0, 0.5, -0.5] + [1.0, -1.0] * 31, np.float32)[:64]
    y = np.resize(lut[rng.integers(0, 64, TABLE, dtype=np.int8)], (rows, n))
    return g, wt, y


def assert_exact_int(g, wt, y):
    """The integer family's condition: gz = (g wt^T)(1 - y^2) and its column sums over all rows are exact in fp32
    in any order.  Every |g wt^T| entry is an integer at most max_r sum_t |g| times max |wt|; times 1, 0.75 or 0 it
    is a multiple of 1/4, so 4 |gz| < 2^24 must hold per entry and, for the bias gradient, per column summed
    over the rows.  Returns the largest column's bound, in quarter units."""
    assert np.array_equal(g, np.rint(g)) and np.array_equal(wt, np.rint(wt))
    f = 1.0 - y.astype(np.float64) ** 2
    assert np.isin(f, (0.0, 0.75, 1.0)).all()
    rowabs = np.abs(g).astype(np.float64).sum(1)              # (rows,): sum_t |g[r][t]|
    wmax = float(np.abs(wt).max())
    assert 4 * rowabs.max() * wmax < 2 ** 24
    col = 4 * wmax * (rowabs @ f)                             # (n,) >= 4 sum_r |gz[r][i]|
    assert col.max() < 2 ** 24, f"column sums may reach {col.max() / 4}"
    return float(col.max())
