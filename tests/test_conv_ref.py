"""oracle/conv_ref.py against torch in fp64 (CPU).  The references are what tests/test_conv_kernels.py holds the HIP convolution
kernels to; here each is held to F.conv2d and its autograd, at ragged sizes, strides 1-4, dilation 2 and 12 and 1x1, 3x3, 4x4, 5x5
and 7x7 filters, to 1e-12 relative; on integer data the three convolutions agree with torch exactly.  The fused forms are held to
the same conv composed with the torch operators they fuse."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as C
import elementwise_ref as E
import fovealseg_oracle as O
import transformer_ref as R

TOL = 1e-12

# B, H, W, Cin, Cout, k, stride, pad, dil
CASES = [(2, 5, 7, 3, 4, 1, 1, 0, 1), (1, 6, 5, 4, 3, 1, 4, 0, 1), (2, 7, 9, 5, 6, 3, 1, 1, 1), (1, 9, 11, 4, 4, 3, 2, 1, 1),
         (2, 10, 7, 3, 5, 3, 3, 1, 1), (1, 19, 22, 2, 3, 3, 4, 1, 1), (2, 9, 8, 3, 2, 4, 2, 1, 1), (1, 8, 9, 4, 3, 5, 1, 2, 1),
         (2, 13, 15, 2, 3, 5, 2, 2, 1), (1, 23, 17, 3, 4, 7, 2, 3, 1), (1, 11, 13, 3, 2, 7, 1, 3, 1), (2, 10, 9, 4, 3, 3, 1, 2, 2),
         (1, 10, 10, 3, 2, 3, 1, 12, 12), (1, 30, 27, 2, 2, 3, 1, 12, 12), (1, 9, 9, 2, 3, 3, 2, 0, 1), (5, 1, 1, 8, 3, 1, 1, 0, 1)]


def close(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= TOL * max(float(b.abs().max()), 1e-300), err


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def oihw(w):
    return w.permute(3, 2, 0, 1).contiguous()


def data(case, kind):
    B, H, W, Ci, Co, k, st, pad, dil = case
    gen = torch.Generator().manual_seed(sum(case) * 7 + k)
    Ho, Wo = C.out_size(H, k, st, pad, dil), C.out_size(W, k, st, pad, dil)
    if kind == "int":
        mk = lambda *s: torch.randint(-3, 4, s, generator=gen).double()
    else:
        mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    return mk(B, H, W, Ci), mk(k, k, Ci, Co), mk(Co), mk(B, Ho, Wo, Co)


def torch_triple(case, x, w, bias, dy):
    """y, dx, dw of F.conv2d and its autograd in fp64, in the layouts of the references"""
    st, pad, dil = case[6:]
    xt, wt = nchw(x).requires_grad_(), oihw(w).requires_grad_()
    y = F.conv2d(xt, wt, bias, st, pad, dil)
    y.backward(nchw(dy))
    return nhwc(y.detach()), nhwc(xt.grad), wt.grad.permute(2, 3, 1, 0).contiguous()


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("case", CASES)
def test_convs_match_torch(case, kind):
    B, H, W, Ci, Co, k, st, pad, dil = case
    x, w, bias, dy = data(case, kind)
    y_t, dx_t, dw_t = torch_triple(case, x, w, bias, dy)
    y = C.conv2d_fwd(x, w, bias, st, pad, dil)
    dx = C.conv2d_bwd_data(dy, w, H, W, st, pad, dil)
    dw = C.conv2d_bwd_weight(x, dy, k, k, st, pad, dil)
    if kind == "int":
        assert torch.equal(y, y_t) and torch.equal(dx, dx_t) and torch.equal(dw, dw_t)
    else:
        close(y, y_t), close(dx, dx_t), close(dw, dw_t)
    dw0 = torch.arange(dw.numel(), dtype=torch.float64).reshape(dw.shape) % 7 - 3
    assert torch.equal(C.conv2d_bwd_weight(x, dy, k, k, st, pad, dil, dw0=dw0), dw0 + dw)
    # the adjoint identities tie the three to each other: <y, dy> = <x, dx> = <w, dw> (bias aside)
    y0 = C.conv(x, w, st, pad, dil)
    for a in (float((x * dx).sum()), float((w * dw).sum())):
        assert abs(a - float((y0 * dy).sum())) <= 1e-10 * max(float((y0.abs() * dy.abs()).sum()), 1.0)


@pytest.mark.parametrize("case", CASES)
def test_bound_helpers(case):
    """sum|terms| is the same convolution on absolute values (>= |result|, equal for non-negative data); the contraction length
    counts the in-range products: Cin (Cout, pixels) times the taps that reach the element, at most the full count"""
    B, H, W, Ci, Co, k, st, pad, dil = case
    x, w, _, dy = data(case, "float")
    for terms, count, val, full in (
            (C.fwd_terms(x, w, st, pad, dil), C.fwd_count(x, w, st, pad, dil), C.conv(x, w, st, pad, dil), k * k * Ci),
            (C.bwd_data_terms(dy, w, H, W, st, pad, dil), C.bwd_data_count(dy, w, H, W, st, pad, dil),
             C.conv2d_bwd_data(dy, w, H, W, st, pad, dil), k * k * Co),
            (C.bwd_weight_terms(x, dy, k, k, st, pad, dil), C.bwd_weight_count(x, dy, k, k, st, pad, dil),
             C.conv2d_bwd_weight(x, dy, k, k, st, pad, dil), dy.shape[0] * dy.shape[1] * dy.shape[2])):
        assert bool((terms >= val.abs() - 1e-12 * terms).all())
        assert float(count.max()) <= full and float(count.min()) >= 0 and bool((count == count.round()).all())
        assert bool(((count == 0) <= (terms == 0)).all())
    y_t, dx_t, dw_t = torch_triple(case, x.abs(), w.abs(), None, dy.abs())
    close(C.fwd_terms(x, w, st, pad, dil), y_t)
    y_1, dx_1, dw_1 = torch_triple(case, torch.ones_like(x), torch.ones_like(w), None, torch.ones_like(dy))
    assert torch.equal(C.fwd_count(x, w, st, pad, dil), y_1)
    assert torch.equal(C.bwd_data_count(dy, w, H, W, st, pad, dil), F.conv_transpose2d(
        nchw(torch.ones_like(dy)), oihw(torch.ones_like(w)), None, st, pad,
        ((H - 1 + 2 * pad - dil * (k - 1)) % st, (W - 1 + 2 * pad - dil * (k - 1)) % st), 1, dil).permute(0, 2, 3, 1))
    assert torch.equal(C.bwd_weight_count(x, dy, k, k, st, pad, dil), dw_1)


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("rows,Ci,Co", [(1, 3, 2), (17, 16, 16), (75, 20, 37), (300, 5, 132)])
def test_linear_wgrad_matches_torch_autograd(rows, Ci, Co, kind):
    """linear_wgrad_ref / linear_wgrad_terms against the fp64 autograd of F.linear: dW = (w.grad)^T in the [Cin][Cout] layout
    of the C ABI, dbias = bias.grad; the terms are the same pair on absolute values"""
    gen = torch.Generator().manual_seed(rows * 31 + Ci + Co)
    if kind == "int":
        mk = lambda *s: torch.randint(-3, 4, s, generator=gen).double()      # noqa: E731
    else:
        mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)      # noqa: E731
    x, dy = mk(rows, Ci), mk(rows, Co)

    def torch_pair(a, g):
        w, b = torch.zeros(Co, Ci, dtype=torch.float64, requires_grad=True), torch.zeros(Co, dtype=torch.float64, requires_grad=True)
        F.linear(a, w, b).backward(g)
        return w.grad.t().contiguous(), b.grad

    for (dw, db), (dw_t, db_t) in ((C.linear_wgrad_ref(x, dy), torch_pair(x, dy)), (C.linear_wgrad_terms(x, dy), torch_pair(x.abs(), dy.abs()))):
        assert dw.shape == (Ci, Co) and db.shape == (Co,) and dw.dtype == torch.float64
        if kind == "int":
            assert torch.equal(dw, dw_t) and torch.equal(db, db_t)
        else:
            close(dw, dw_t), close(db, db_t)
    tw, tb = C.linear_wgrad_terms(x, dy)
    dw, db = C.linear_wgrad_ref(x, dy)
    assert bool((tw >= dw.abs() - 1e-12 * tw).all()) and bool((tb >= db.abs() - 1e-12 * tb).all())


def test_flip_transpose_is_the_stride_1_bwd_data():
    for case in [c for c in CASES if c[6] == 1]:
        B, H, W, Ci, Co, k, st, pad, dil = case
        x, w, _, dy = data(case, "int")
        assert torch.equal(C.conv(dy, C.flip_transpose(w), 1, dil * (k - 1) - pad, dil), C.conv2d_bwd_data(dy, w, H, W, 1, pad, dil))


@pytest.mark.parametrize("p", [0.0, 0.25, 0.2])
def test_forward_dropout(p):
    case = (2, 7, 9, 5, 6, 3, 1, 1, 1)
    x, w, bias, _ = data(case, "float")
    key = O.layer_key(3, 11)
    y0 = C.conv2d_fwd(x, w, bias, 1, 1, 1)
    y = C.conv2d_fwd(x, w, bias, 1, 1, 1, p, key)
    if p == 0:
        assert torch.equal(y, y0)
        return
    keep = torch.from_numpy(O.dropout_keep_mask_nhwc(y0.numel(), key, float(np.float32(p)))).bool().reshape(y0.shape)
    assert bool(keep.any()) and not bool(keep.all())
    assert torch.equal(y, torch.where(keep, y0 * float(np.float32(1.0) / np.float32(1.0 - float(np.float32(p)))), torch.zeros_like(y0)))
    tot = C.stats_totals(y)
    close(tot[:, 0], y.sum((0, 1, 2))), close(tot[:, 1], (y * y).sum((0, 1, 2)))


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_res", [False, True])
def test_affine_act(act, with_res):
    case = (2, 6, 8, 4, 8, 3, 1, 1, 1)
    x, w, bias, res = data(case, "float")
    gen = torch.Generator().manual_seed(act)
    scale, shift = torch.randn(8, generator=gen, dtype=torch.float64), torch.randn(8, generator=gen, dtype=torch.float64)
    res = res if with_res else None
    v = nhwc(F.conv2d(nchw(x), oihw(w), bias, 1, 1)) * scale + shift
    v = v if res is None else v + res
    want = (v, F.relu(v), F.relu6(v))[act]
    close(C.conv2d_fwd_affine_act(x, w, bias, scale, shift, res, act, 1, 1, 1), want)


def test_residual_droppath():
    case = (4, 4, 8, 8, 12, 1, 1, 0, 1)
    x, w, bias, res = data(case, "float")
    rows = 32                                                       # one sample = one image
    for dp in (0.0, 0.5):
        for p in (0.0, 0.25):
            dkey = next(k for k in range(1, 99) if dp == 0 or 0 < int(R.keep_mask(4, k, dp).sum()) < 4)
            y = C.conv2d_fwd_residual(x, w, bias, res, 1, 0, 1, p, 77, dp, dkey, rows)
            v = C.conv2d_fwd(x, w, bias, 1, 0, 1, p, 77)
            keep = R.keep_mask(4, dkey, dp).double().reshape(4, 1, 1, 1)
            close(y, res + keep * v * R.drop_scale(dp))


@pytest.mark.parametrize("with_bn,with_mask,with_add,with_amask",
                         [(1, 1, 0, 0), (1, 0, 1, 1), (1, 1, 1, 0), (0, 0, 1, 1), (0, 0, 1, 0), (1, 0, 0, 0)])
def test_bwd_data_bnsum(with_bn, with_mask, with_add, with_amask):
    case = (2, 6, 8, 8, 4, 3, 1, 1, 1)
    B, H, W, Ci, Co, k, st, pad, dil = case
    x, w, _, dy = data(case, "float")
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    bn_y, mean, invstd, add = rnd(B, H, W, Ci), rnd(Ci), rnd(Ci).abs() + 0.5, rnd(B, H, W, Ci)
    bits, abits = rnd(B, H, W, Ci) > 0, rnd(B, H, W, Ci) > 0
    dx, S, SX = C.conv2d_bwd_data_bnsum(dy, w, H, W, st, pad, dil, bn_y if with_bn else None, bits if with_mask else None, mean, invstd,
                                        add if with_add else None, abits if with_amask else None)
    want = torch_triple(case, x, w, None, dy)[1]
    if with_add:
        want = want + (add * abits.double() if with_amask else add)
    close(dx, want)
    if not with_bn:
        assert S is None and SX is None
        return
    g = want * bits.double() if with_mask else want
    close(S, g.sum((0, 1, 2)))
    close(SX, (g * (bn_y - mean) * invstd).sum((0, 1, 2)))
    # the sums are those of the stand-alone pass over the stored dx (fs_bn_bwd_partial's slab, summed)
    S2, SX2 = E.bn_bwd_sums(dx.reshape(-1, Ci), (bits if with_mask else torch.ones_like(bits)).reshape(-1, Ci), bn_y.reshape(-1, Ci), mean, invstd)
    assert torch.equal(S, S2) and torch.equal(SX, SX2)


@pytest.mark.parametrize("m,W", [(2, 6), (2, 18), (4, 8), (4, 20)])
def test_wino_terms_bound_the_transform_domain_products(m, W):
    """the transform-domain sum|terms| is at least the direct one (the transforms only add magnitude) and at most the product
    of the three matrices' largest absolute row sums times it -- and on a one-tap filter with a one-pixel image it is the
    hand-computed value"""
    gen = torch.Generator().manual_seed(m * W)
    x, w = torch.randn(2, 5, W, 3, generator=gen, dtype=torch.float64), torch.randn(3, 3, 3, 4, generator=gen, dtype=torch.float64)
    t = C.wino_fwd_terms(x, w, m)
    direct = C.fwd_terms(x, w, 1, 1, 1)
    assert t.shape == direct.shape and bool((t >= direct * (1 - 1e-12)).all())
    k = C.WINO[m]
    # exact identity behind the kernels: A^T [(G g) * (B^T d)] with the SIGNED constants is the convolution; here only their
    # magnitudes are known, so check the hand value: x = delta at (0, 1), w = delta at tap (1, 1) (the centre) -> output (0, 1) = 1
    xd, wd = torch.zeros(1, 1, W, 1, dtype=torch.float64), torch.zeros(3, 3, 1, 1, dtype=torch.float64)
    xd[0, 0, 1, 0], wd[1, 1, 0, 0] = 1.0, 1.0
    BT, G, AT = (torch.tensor(k[n], dtype=torch.float64) for n in ("BT", "G", "AT"))
    hand = AT @ ((G[:, 1]) * (BT[:, 2]))                 # pixel 1 is d_2 of tile 0 (d_t = x[m j - 1 + t]); centre column of G
    assert torch.allclose(C.wino_fwd_terms(xd, wd, m)[0, 0, :m, 0], hand, rtol=0, atol=1e-15)
    dy = torch.randn(2, 5, W, 4, generator=gen, dtype=torch.float64)
    if m == 2:
        tw = C.wino_wgrad_terms(x, dy)
        dw = C.bwd_weight_terms(x, dy, 3, 3, 1, 1, 1)
        assert tw.shape == dw.shape and bool((tw >= dw * (1 - 1e-12)).all())


@pytest.mark.parametrize("m,W", [(2, 6), (2, 18), (4, 8), (4, 20)])
def test_wino_tables_are_the_transform(m, W):
    """A^T [(G g) * (B^T d)] with the SIGNED constants of oracle/conv_ref.py (read off csrc/conv_wino.hip / conv_wino4.hip) is the
    3x3 / stride-1 / pad-1 convolution: on integers with filters that keep G g exact (multiples of 2 for F(2,3), of 24 for F(4,3))
    bit for bit for F(2,3) (F(4,3): to 1e-12, its constants are no binary fractions), on random data to 1e-12.  The bound tables are the absolute values of exactly these."""
    gen = torch.Generator().manual_seed(m + W)
    x = torch.randint(-3, 4, (2, 5, W, 3), generator=gen).double()
    w = torch.randint(-2, 3, (3, 3, 3, 4), generator=gen).double() * (2 if m == 2 else 24)
    if m == 2:
        assert torch.equal(C.wino_conv(x, w, m), C.conv(x, w, 1, 1, 1))
    else:          # 1/6, 1/12 and 1/24 are not fp64 numbers: G g is rounded even where the true value is an integer
        close(C.wino_conv(x, w, m), C.conv(x, w, 1, 1, 1))
    x, w = rnd64(gen, 2, 5, W, 3), rnd64(gen, 3, 3, 3, 4)
    close(C.wino_conv(x, w, m), C.conv(x, w, 1, 1, 1))
    for n in ("BT", "G", "AT"):
        assert torch.equal(torch.tensor(C.WINO[m][n]), torch.tensor(C.WINO_SIGNED[m][n]).abs())


def rnd64(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)
