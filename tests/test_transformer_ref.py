"""oracle/transformer_ref.py against torch in fp64 (CPU).  The references are what tests/test_transformer_kernels.py holds the HIP
kernels to; here each is held to the torch operator it restates, at ragged shapes and with every optional argument, to 1e-12
relative; the adjoint identities on integer data hold exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_ref as R
import fovealseg_oracle as O

TOL = 1e-12


def close(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= TOL * max(float(b.abs().max()), 1e-300), err


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def rint(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def test_abi_constants():
    """the float constants as transformer.hip forms them"""
    assert R.drop_scale(0.0) == 1.0 and R.drop_thresh(0.0) == 0
    assert R.drop_scale(0.25) == float(np.float32(4.0) / np.float32(3.0)) and R.drop_thresh(0.25) == 1 << 30
    p32 = float(np.float32(0.2))
    assert R.drop_scale(0.2) == float(np.float32(1.0) / np.float32(1.0 - p32))
    assert R.drop_thresh(0.2) == int(p32 * 2.0 ** 32) == 858993472
    assert R.abi_float(1e-6) == float(np.float32(1e-6)) != 1e-6
    assert R.abi_float(0.125) == 0.125
    assert bool(R.keep_mask(7, 5, 0.0).all())
    assert np.array_equal(R.keep_mask(1000, 77, 0.2).numpy(), O.dropout_keep_mask_nhwc(1000, 77, p32))


@pytest.mark.parametrize("M,C", [(1, 4), (3, 64), (17, 68), (5, 132), (2, 324), (7, 2048)])
@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("add", [False, True])
def test_layernorm_matches_torch(M, C, offset, add):
    gen = torch.Generator().manual_seed(M * 31 + C)
    eps = R.abi_float(1e-6)
    x = rnd(gen, M, C) + offset
    gamma, beta = 1 + 0.3 * rnd(gen, C), rnd(gen, C)
    g = rnd(gen, M, C)
    addend = rnd(gen, M, C) if add else None
    y, mean, rstd = R.layernorm_fwd(x, gamma, beta, eps)
    dx, dgamma, dbeta = R.layernorm_bwd(g, x, gamma, mean, rstd, addend)
    xt, gt, bt = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yt = F.layer_norm(xt, (C,), gt, bt, eps)
    yt.backward(g)
    close(y, yt.detach())
    close(mean, x.mean(-1))
    close(rstd, 1 / torch.sqrt(x.var(-1, unbiased=False) + eps))
    # (dx is a difference of terms of size |g gamma| rstd: 1e-12 of THAT scale)
    scale = float((g * gamma).abs().max() * rstd.max())
    ref = xt.grad + (addend if add else 0)
    assert float((dx - ref).abs().max()) <= TOL * max(scale, float(ref.abs().max()))
    close(dgamma, gt.grad)
    close(dbeta, bt.grad)


def test_gelu_matches_torch():
    gen = torch.Generator().manual_seed(3)
    x = torch.cat([rnd(gen, 1001) * 2, torch.linspace(-12, 12, 4801, dtype=torch.float64), torch.tensor([0.0, -0.0, 30.0, -30.0, 2.0 ** -126, -2.0 ** -126])])
    g = rnd(gen, x.numel())
    xt = x.clone().requires_grad_(True)
    yt = F.gelu(xt)
    yt.backward(g)
    y, dx = R.gelu_fwd(x), R.gelu_bwd(g, x)
    # F.gelu forms 1 + erf, absolute accuracy 1e-16 |x| in the negative tail; the reference keeps its relative accuracy there
    assert float((y - yt.detach()).abs().max()) <= 1e-14
    assert bool(((y - yt.detach()).abs() <= TOL * yt.detach().abs())[x > -3].all())
    assert float((dx - xt.grad).abs().max()) <= 1e-14 * float(g.abs().max())
    assert bool(((dx - xt.grad).abs() <= TOL * (g.abs() + xt.grad.abs()))[x > -3].all())
    # the negative tail against the asymptotic series x Phi(x) = -phi(x) (1 - 1/x^2 + 3/x^4 - 15/x^6 + ...), error below the next term
    xs = torch.tensor([-8.0, -12.0, -30.0], dtype=torch.float64)
    series = -R.gelu_pdf(xs) * (1 - 1 / xs ** 2 + 3 / xs ** 4 - 15 / xs ** 6)
    assert bool(((R.gelu_fwd(xs) - series).abs() <= 105 / xs ** 8 * series.abs() + 1e-300).all())
    # the same formula in fp32 stays the kernel's expression
    x32 = x.float()
    assert torch.equal(R.gelu_fwd(x32), 0.5 * x32 * (1 + torch.erf(x32 * np.float32(R.INV_SQRT2))))
    assert R.gelu_fwd(x32).dtype == torch.float32 and R.gelu_bwd(g.float(), x32).dtype == torch.float32


@pytest.mark.parametrize("p", [0.2, 0.3])
def test_gelu_dropout_matches_torch(p):
    gen = torch.Generator().manual_seed(4)
    x, g = rnd(gen, 3, 5, 8) * 2, rnd(gen, 3, 5, 8)
    key = O.layer_key(3, 9)
    keep = torch.from_numpy(O.dropout_keep_mask_nhwc(x.numel(), key, R.abi_float(p))).reshape(x.shape)
    assert 0 < int(keep.sum()) < x.numel()
    xt = x.clone().requires_grad_(True)
    yt = F.gelu(xt) * keep * R.drop_scale(p)
    yt.backward(g)
    close(R.gelu_dropout_fwd(x, p, key), yt.detach())
    close(R.gelu_dropout_bwd(g, x, p, key), xt.grad)
    assert bool((R.gelu_dropout_fwd(x, p, key)[~keep] == 0).all())


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 3, 5, 8), (3, 4, 17, 12), (1, 9, 2, 4)])
@pytest.mark.parametrize("use_bias", [False, True])
def test_dwconv3_matches_torch(B, H, W, C, use_bias):
    gen = torch.Generator().manual_seed(B * 100 + H * 10 + W)
    x, w, dy = rnd(gen, B, H, W, C), rnd(gen, C, 9), rnd(gen, B, H, W, C)
    bias = rnd(gen, C) if use_bias else None
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wt = w.reshape(C, 1, 3, 3).clone().requires_grad_(True)
    bt = bias.clone().requires_grad_(True) if use_bias else None
    yt = F.conv2d(xt, wt, bt, 1, 1, 1, C)
    yt.backward(dy.permute(0, 3, 1, 2))
    close(R.dwconv3_fwd(x, w, bias), yt.detach().permute(0, 2, 3, 1))
    close(R.dwconv3_fwd(dy, w, None, flip=True), xt.grad.permute(0, 2, 3, 1))
    close(R.dwconv3_bwd_weight(x, dy), wt.grad.reshape(C, 9))
    if use_bias:
        close(R.dwconv3_bwd_bias(dy), bt.grad)


def test_dwconv3_adjoint_identity_exact_on_integers():
    gen = torch.Generator().manual_seed(8)
    x, g, w = rint(gen, -4, 4, 2, 5, 7, 8), rint(gen, -4, 4, 2, 5, 7, 8), rint(gen, -3, 3, 8, 9)
    lhs = (R.dwconv3_fwd(x, w) * g).sum()
    rhs = (x * R.dwconv3_fwd(g, w, None, flip=True)).sum()
    assert float(lhs) == float(rhs) != 0.0
    # ... and dw is the gradient of that same bilinear form with respect to w
    assert float((R.dwconv3_bwd_weight(x, g) * w).sum()) == float(lhs)


@pytest.mark.parametrize("per_sample,n", [(4, 24), (12, 60), (20, 100)])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("with_x", [True, False])
def test_residual_droppath(per_sample, n, p, with_x):
    gen = torch.Generator().manual_seed(n)
    key = O.layer_key(2, 5)
    x, y = rnd(gen, n), rnd(gen, n)
    nsamp = n // per_sample
    keep = torch.from_numpy(O.dropout_keep_mask_nhwc(nsamp, key, p)).double() if p > 0 else torch.ones(nsamp, dtype=torch.float64)
    ref = (y.reshape(nsamp, per_sample) * keep[:, None] * R.drop_scale(p)).reshape(-1)
    out = R.residual_droppath(x if with_x else None, y, per_sample, p, key)
    close(out, ref + x if with_x else ref)
    # the fused backward = the two passes one after the other
    key2 = O.layer_key(4, 1)
    keep2 = torch.from_numpy(O.dropout_keep_mask_nhwc(n, key2, R.abi_float(0.3))).double()
    close(R.droppath_dropout_bwd(y, per_sample, p, key, 0.3, key2), ref * keep2 * R.drop_scale(0.3))
    close(R.droppath_dropout_bwd(y, per_sample, p, key, 0.0, key2), ref)


UNFOLD_CASES = [(2, 9, 11, 3, 7, 4, 3, 148), (1, 7, 6, 3, 7, 1, 3, 148), (2, 5, 8, 5, 3, 2, 1, 48), (1, 17, 16, 6, 8, 8, 0, 384),
                (2, 6, 5, 8, 2, 2, 0, 40), (1, 22, 18, 4, 4, 4, 0, 64), (2, 3, 3, 4, 1, 1, 0, 4)]


def torch_unfold_rsc(x, k, stride, pad, Kp):
    """F.unfold's (c, r, s) columns re-ordered to (r, s, c) and padded to Kp"""
    B, H, W, C = x.shape
    u = F.unfold(x.permute(0, 3, 1, 2), k, 1, pad, stride)               # (B, C k k, L)
    L = u.shape[-1]
    u = u.reshape(B, C, k * k, L).permute(0, 3, 2, 1).reshape(B * L, k * k * C)
    return torch.cat([u, u.new_zeros(B * L, Kp - k * k * C)], 1)


@pytest.mark.parametrize("B,H,W,C,k,stride,pad,Kp", UNFOLD_CASES)
def test_unfold_fold_match_torch(B, H, W, C, k, stride, pad, Kp):
    gen = torch.Generator().manual_seed(H * 10 + W + k)
    x = rnd(gen, B, H, W, C)
    col = R.unfold(x, k, stride, pad, Kp)
    assert torch.equal(col, torch_unfold_rsc(x, k, stride, pad, Kp))          # pure data movement: exact
    Ho, Wo = R.out_size(H, k, stride, pad), R.out_size(W, k, stride, pad)
    c = rnd(gen, B * Ho * Wo, Kp)
    kk = k * k * C
    ct = c[:, :kk].reshape(B, Ho * Wo, k * k, C).permute(0, 3, 2, 1).reshape(B, C * k * k, Ho * Wo)
    ref = F.fold(ct, (H, W), k, 1, pad, stride).permute(0, 2, 3, 1)
    close(R.fold(c, B, H, W, C, k, stride, pad), ref)
    # adjoint identity on integer data: exact
    xi, ci = rint(gen, -5, 5, B, H, W, C), rint(gen, -5, 5, B * Ho * Wo, Kp)
    assert float((R.unfold(xi, k, stride, pad, Kp) * ci).sum()) == float((xi * R.fold(ci, B, H, W, C, k, stride, pad)).sum())


@pytest.mark.parametrize("B,heads,N,Nk,p", [(1, 1, 1, 1, 0.0), (2, 2, 5, 7, 0.2), (1, 3, 33, 65, 0.0), (3, 1, 9, 130, 0.2)])
@pytest.mark.parametrize("peaked", [False, True])
def test_attention_matches_torch(B, heads, N, Nk, p, peaked):
    gen = torch.Generator().manual_seed(N * 7 + Nk)
    C = heads * 64
    q, k, v, go = rnd(gen, B, N, C), rnd(gen, B, Nk, C), rnd(gen, B, Nk, C), rnd(gen, B, N, C)
    if peaked:
        q = q * 4 + 10
    key = O.layer_key(7, 70)
    scale = 0.125
    qt, kt, vt = (t.clone().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, -1, heads, 64).transpose(1, 2) for t in (qt, kt, vt))
    S = qh @ kh.transpose(-1, -2) * scale
    probs = torch.softmax(S, -1)
    if p > 0:
        keep = torch.from_numpy(O.dropout_keep_mask_nhwc(B * heads * N * Nk, key, R.abi_float(p))).view(B, heads, N, Nk).double()
        probs = probs * keep * R.drop_scale(p)
    ref = (probs @ vh).transpose(1, 2).reshape(B, N, C)
    ref.backward(go)
    o, lse = R.attention_fwd(q, k, v, heads, scale, p, key)
    close(o, ref.detach())
    close(lse, torch.logsumexp(S.detach(), -1).reshape(-1))
    dq, dk, dv = R.attention_bwd(q, k, v, go, heads, scale, p, key)
    close(dv, vt.grad)
    # dq / dk are sums of signed terms P (M dP~ - D): 1e-12 of the terms' scale
    for got, want in ((dq, qt.grad), (dk, kt.grad)):
        assert float((got - want).abs().max()) <= TOL * max(float(want.abs().max()), float(go.abs().max() * v.abs().max() * 64 * k.abs().max()))
    close(R.attention_rowdot(go, o, heads), (go * o).view(B, N, heads, 64).sum(-1).transpose(1, 2).reshape(-1))
