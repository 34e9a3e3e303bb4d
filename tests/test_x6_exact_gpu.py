"""The x6 GEMMs (csrc/vss_gemm_x6.hip) bit for bit, at the shapes where a block runs several work items.

The operands come from tests/x6_exact.py's families, on which the six-product sum is exact in fp32 in any
order: the kernel must return it at every entry of every item, with no tolerance and no model of the matrix
core's rounding.  The expectation is the fp64 product of the split planes (exact for the same reason), taken on
the GPU by torch.  The C entries are called directly: the 256-feature block takes any multiple of 128 rows.
Where the result is only visible through tanh (the forward), the checks are metamorphic (K permutation, zero
padding, the same rows in single-item chunks) plus the existing fp64 anchor."""
import numpy as np
import pytest
import torch

import x6_exact as X
from test_gemm_x6 import _ops, _rel
from vss_amd import _native as N
from vss_amd.update import weight_planes

F64 = torch.float64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16_rne(v):
    u = v.contiguous().view(torch.int32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & -65536).view(torch.float32)


def split3(v):
    """x6_exact.split3 on a torch tensor (test_torch_split_is_the_host_split_cpu)."""
    hi = _bf16_rne(v)
    r1 = v - hi
    mid = _bf16_rne(r1)
    return hi, mid, r1 - mid


def test_torch_split_is_the_host_split_cpu():
    rng = np.random.default_rng(1)
    v = np.concatenate([X.three_plane_values(4096, 2)[0], np.zeros(2, np.float32),
                        (rng.standard_normal(1 << 16) * np.ldexp(1.0, rng.integers(-40, 40, 1 << 16))).astype(np.float32),
                        rng.integers(-300, 301, 4096).astype(np.float32)])
    for got, want in zip(split3(torch.from_numpy(v)), X.split3(v)):
        assert np.array_equal(got.numpy(), want)


def six(P, Q):
    """x6_exact.six in fp64 on the GPU: out[j][i] over P (I, K), Q (J, K), grouped by Q's plane."""
    ph, pm, pl = (x.to(F64) for x in split3(P))
    qh, qm, ql = (x.to(F64) for x in split3(Q))
    return qh @ (ph + pm + pl).t() + qm @ (ph + pm).t() + ql @ ph.t()


def six_parts(xs, gs, starts):
    """(parts, n_out, k_in) fp64: the six-product sum of grad^T x over each part's rows (x6_exact.six_parts), as
    batched products over the parts padded with zero rows to one length."""
    rows, parts, longest = xs.shape[0], len(starts) - 1, int(np.diff(starts).max())
    idx = np.full((parts, longest), rows, np.int64)   # row `rows`: the zero row appended below
    for s in range(parts):
        idx[s, :starts[s + 1] - starts[s]] = np.arange(starts[s], starts[s + 1])
    idx = _dev(idx)

    def padded(v):
        z = torch.zeros(1, v.shape[1], device=v.device)
        return [torch.cat([x, z])[idx].to(F64) for x in split3(v)]   # (parts, longest, cols) per plane
    xh, xm, xl = padded(xs)
    gh, gm, gl = padded(gs)
    return gh.transpose(1, 2) @ (xh + xm + xl) + gm.transpose(1, 2) @ (xh + xm) + gl.transpose(1, 2) @ xh


# ---- the C entries --------------------------------------------------------------------------------------------

def _scratch(n, k):
    return torch.empty(3 * n * k, device="cuda", dtype=torch.int16)


def forward(x, w, b, planes=None, out=None, w_out=None):
    """vss_linear_tanh_bf16x6, or with w_out (k_out, 256) vss_linear_tanh_out_bf16x6: y, or (y, out_part)."""
    rows, k = x.shape
    n = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous()
    lib, s = N.load(), N.stream_of(x.device)
    y = torch.empty(rows, n, device="cuda") if out is None else out
    wp, pp = (w.data_ptr(), _scratch(n, k)) if planes is None else (None, planes)
    if w_out is None:
        N.check(lib.vss_linear_tanh_bf16x6(s, rows, k, n, x.data_ptr(), wp, b.data_ptr(), y.data_ptr(), pp.data_ptr()),
                "vss_linear_tanh_bf16x6")
        return y
    part = torch.empty(n // 64, rows, w_out.shape[0], device="cuda")
    N.check(lib.vss_linear_tanh_out_bf16x6(s, rows, k, n, x.data_ptr(), wp, b.data_ptr(), y.data_ptr(), w_out.shape[0],
                                           w_out.data_ptr(), part.data_ptr(), pp.data_ptr()), "vss_linear_tanh_out_bf16x6")
    return y, part


def backward(g_next, wt, y, planes=None, out=None):
    """vss_linear_tanh_backward_bf16x6 with wt = W_next^T (n, k_next): (gz, the column-sum parts)."""
    rows, k_next = g_next.shape
    n = wt.shape[0]
    assert g_next.is_contiguous() and wt.is_contiguous() and y.is_contiguous()
    lib, s = N.load(), N.stream_of(y.device)
    gz = torch.empty(rows, n, device="cuda") if out is None else out
    part = torch.empty(lib.vss_linear_tanh_backward_chunks_bf16x6(rows, k_next, n), n, device="cuda")
    wp, pp = (wt.data_ptr(), _scratch(n, k_next)) if planes is None else (None, planes)
    N.check(lib.vss_linear_tanh_backward_bf16x6(s, rows, k_next, n, g_next.data_ptr(), wp, y.data_ptr(), gz.data_ptr(),
                                                part.data_ptr(), pp.data_ptr()), "vss_linear_tanh_backward_bf16x6")
    return gz, part


def tile_rows(n):
    return 128 if n % 256 == 0 else 256   # the block's row tile (include/vss.h: the 256-feature block where n % 256 == 0)


def single_item_rows(k, n):
    """The most rows a call takes with every block running one work item: the library's blocks per feature tile."""
    return N.load().vss_linear_tanh_backward_chunks_bf16x6(1 << 24, k, n) * tile_rows(n)


def assert_items(rows, k, n, multi):
    """The point of a shape, from the library's own plan: the row tiles outnumber the blocks per feature tile
    (some block runs several work items), or for a control do not."""
    lib = N.load()
    blocks = lib.vss_linear_tanh_backward_chunks_bf16x6(rows, k, n)
    assert blocks > 0
    if n == 256:
        assert lib.vss_linear_tanh_loss_blocks_bf16x6(rows, k, n) == blocks
    tiles = rows // tile_rows(n)
    assert (tiles > blocks) == multi, f"{rows} rows x {n}: {tiles} row tiles on {blocks} blocks per feature tile"
    assert not multi or single_item_rows(k, n) < rows


def in_chunks(fn, rows, limit):
    """fn(a, b) over the row ranges of at most `limit` rows."""
    for a in range(0, rows, limit):
        fn(a, min(rows, a + limit))


# ---- forward and backward, three-plane family -------------------------------------------------------------------

FB_CASES = [(n, rows, True) for n, rows in X.FB_MULTI] + [(n, rows, False) for n, rows in X.FB_SINGLE]


@pytest.mark.gpu
@pytest.mark.parametrize("q_dense", [False, True], ids=["w_dense", "x_dense"])
@pytest.mark.parametrize("k", X.FB_K)
@pytest.mark.parametrize("n,rows,multi", FB_CASES)
def test_three_plane_backward_and_forward_gpu(n, rows, multi, k, q_dense):
    """P (n, k) the weight operand, Q (rows, k) the row operand, one dense in the three-plane family and one with 3
    nonzeros per contraction vector.

    Backward with y = 0 (the K loop seen without tanh): gz is `six` bit for bit, by the weight split in the call,
    by planes made from the (k, n) weight with transpose = 1, and by planes made from its transposed copy.
    Forward: y is bit-equal under a permutation of K, under zero padding of K (64 -> 128), and to the same rows
    passed in single-item chunks; and within 4e-6 of tanh(six + b) in fp64 (test_gemm_x6.py's tolerance)."""
    assert_items(rows, k, n, multi)
    Pn, Qn = X.fb_operands(n, rows, k, q_dense)
    X.assert_exact(Pn, Qn)
    P, Q = _dev(Pn), _dev(Qn)
    want = six(P, Q)
    assert torch.equal(want, want.float().to(F64))
    want = want.float()
    y0 = torch.zeros(rows, n, device="cuda")
    p_tr, p_plain = weight_planes([(P.t().contiguous(), True), (P, False)])
    assert torch.equal(p_tr, p_plain)
    for planes in (None, p_tr, p_plain):
        gz, _ = backward(Q, P, y0, planes)
        assert torch.equal(gz, want), float((gz != want).float().mean())
    del gz, y0

    g = torch.Generator(device="cuda").manual_seed(n + k)
    b = torch.randn(n, device="cuda", generator=g) * 0.1
    y = forward(Q, P, b)
    assert _rel(y, torch.tanh(want.to(F64) + b.to(F64)))[0] < 4e-6
    perm = torch.randperm(k, device="cuda", generator=g)
    assert torch.equal(forward(Q[:, perm].contiguous(), P[:, perm].contiguous(), b), y)
    if k == 64:
        assert torch.equal(forward(torch.cat([Q, torch.zeros_like(Q)], 1), torch.cat([P, torch.zeros_like(P)], 1), b), y)
    yc = torch.empty_like(y)
    in_chunks(lambda a, e: forward(Q[a:e], P, b, out=yc[a:e]), rows, single_item_rows(k, n))
    assert torch.equal(yc, y)


# ---- backward, integer family: the (1 - y^2) factor and the bias gradient ------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", [64, 512])
@pytest.mark.parametrize("n,rows,multi", FB_CASES)
def test_integer_backward_and_bias_gradient_gpu(n, rows, multi, k):
    """Integers and y in {0, +-0.5, +-1}: gz = (g W)(1 - y^2) is exact, and so is every partial sum of its column sums
    over the rows: the parts, summed, are the bias gradient exactly -- across the items a block accumulates."""
    assert_items(rows, k, n, multi)
    gn, wn, yn = X.int_backward(rows, k, n, 3)
    X.assert_exact_int(gn, wn, yn)
    g, wt, y = _dev(gn), _dev(wn), _dev(yn)
    want = (g.to(F64) @ wt.to(F64).t()) * (1 - y.to(F64) ** 2)
    assert float(want.abs().sum(0).max()) * 4 < 2 ** 24
    gz, part = backward(g, wt, y)
    assert torch.equal(gz.to(F64), want)
    assert torch.equal(part.to(F64).sum(0), want.sum(0))


# ---- weight gradients: every part, over exactly its rows ---------------------------------------------------------

def _weight_grad_parts(entry, chunks, rows, n_out, k_in, x_dense):
    lib = N.load()
    parts = getattr(lib, chunks)(rows, n_out, k_in)
    starts = X.part_starts(rows, parts)
    xn, gn = X.wg_operands(rows, n_out, k_in, starts, x_dense)
    X.assert_exact_parts(xn, gn, starts)
    x, g = _dev(xn), _dev(gn)
    want = six_parts(x, g, starts)
    assert torch.equal(want, want.float().to(F64))
    got = torch.empty(parts, n_out, k_in, device="cuda")
    N.check(getattr(lib, entry)(N.stream_of(x.device), rows, n_out, k_in, g.data_ptr(), x.data_ptr(), got.data_ptr()), entry)
    bad = (got != want.float()).reshape(parts, -1).any(1).nonzero().flatten().tolist()
    assert not bad, f"parts {bad[:8]} differ from the six-product sum over their rows"
    return parts


@pytest.mark.gpu
@pytest.mark.parametrize("x_dense", [False, True], ids=["g_dense", "x_dense"])
@pytest.mark.parametrize("rows", X.WG_ROWS)
@pytest.mark.parametrize("n_out,k_in", X.WG_SHAPES)
def test_weight_grad_parts_gpu(n_out, k_in, rows, x_dense):
    """vss_weight_grad_bf16x6's partials, not their sum: partial[s] is `six` over the rows
    [s kpairs / S, (s + 1) kpairs / S) 64 and no others (a prime number of K-tile pairs: uneven parts; the sparse
    operand puts a nonzero in every pair, so a pair in the wrong part shows).  At k_in = 384 the grid trim leaves
    some blocks two work items."""
    parts = _weight_grad_parts("vss_weight_grad_bf16x6", "vss_weight_grad_chunks_bf16x6", rows, n_out, k_in, x_dense)
    assert parts == X.wg_parts(rows, n_out, k_in) and (rows // 64) % parts


@pytest.mark.gpu
@pytest.mark.parametrize("x_dense", [False, True], ids=["g_dense", "x_dense"])
@pytest.mark.parametrize("rows", X.WG_ROWS)
@pytest.mark.parametrize("k_in", X.FW_K_IN)
def test_first_weight_grad_parts_gpu(k_in, rows, x_dense):
    """The same for the first layer's vss_first_weight_grad_bf16x6 (one block per part)."""
    parts = _weight_grad_parts("vss_first_weight_grad_bf16x6", "vss_first_weight_grad_chunks_bf16x6", rows, 256, k_in,
                               x_dense)
    assert parts == X.fw_parts(rows) and (rows // 64) % parts


# ---- random full-precision data: the bits do not depend on which item of a block computes them ------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", X.FB_K)
@pytest.mark.parametrize("n,rows", X.FB_MULTI)
def test_multi_item_call_equals_single_item_chunks_gpu(n, rows, k):
    """On random operands the multi-item call and single-item calls on the same rows agree bit for bit: the forward,
    vss_linear_tanh_out_bf16x6 (y and the output parts, n = 256), and the backward's gz.  (The per-output MFMA sequence
    does not depend on the schedule; the backward's column-sum parts do, and are not compared.)"""
    assert_items(rows, k, n, True)
    limit = single_item_rows(k, n)
    x, w, b, _, _ = _ops(rows, k, n, n + k)
    y = forward(x, w, b)
    yc = torch.empty_like(y)
    in_chunks(lambda a, e: forward(x[a:e], w, b, out=yc[a:e]), rows, limit)
    assert torch.equal(yc, y)
    if n == 256:
        g = torch.Generator(device="cuda").manual_seed(k)
        w_out = torch.randn(2, 256, device="cuda", generator=g) / 16
        y2, part = forward(x, w, b, w_out=w_out)
        assert torch.equal(y2, y)

        def chunk(a, e):
            yy, pp = forward(x[a:e], w, b, w_out=w_out)
            assert torch.equal(yy, y[a:e]) and torch.equal(pp, part[:, a:e])
        in_chunks(chunk, rows, limit)
    del yc
    # backward from a k-wide layer into this n-wide tanh layer
    g = torch.Generator(device="cuda").manual_seed(n + k + 1)
    wt = torch.randn(n, k, device="cuda", generator=g) / k ** 0.5
    g_next = torch.randn(rows, k, device="cuda", generator=g) * 1e-3
    gz, _ = backward(g_next, wt, y)
    gc = torch.empty_like(gz)
    in_chunks(lambda a, e: backward(g_next[a:e], wt, y[a:e], out=gc[a:e]), rows, limit)
    assert torch.equal(gc, gz)
