"""oracle/elementwise_ref.py against torch in fp64 (CPU).  The references are what tests/test_elementwise_kernels.py holds the HIP
kernels to; here each is held to the torch operator it restates, at ragged shapes, to 1e-12 relative (indices: exact)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R
import fovealseg_oracle as O

TOL = 1e-12


def close(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= TOL * max(float(b.abs().max()), 1e-300), err


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def nchw(x, B, H, W):          # (M, C) rows -> (B, C, H, W)
    return x.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def rows(x):                   # (B, C, H, W) -> (M, C)
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 3, 5, 20), (3, 7, 2, 132), (1, 1, 3, 8)])
@pytest.mark.parametrize("act,use_res", [(0, False), (1, True), (2, False)])
def test_batchnorm_training_matches_torch(B, H, W, C, act, use_res):
    gen = torch.Generator().manual_seed(B * 100 + C + act)
    M, eps, mom = B * H * W, 1e-5, 0.1
    y = rnd(gen, M, C) * 2 + 3
    gamma, beta = 0.5 + rnd(gen, C).abs(), rnd(gen, C)
    rm, rv = rnd(gen, C), 1 + torch.rand(C, generator=gen, dtype=torch.float64)
    res = rnd(gen, M, C) if use_res else None
    dz = rnd(gen, M, C)

    mean, invstd, rm2, rv2 = R.bn_batch_stats(y, eps, mom, rm, rv)
    out = R.bn_act_fwd(y, mean, invstd, gamma, beta, res, act)
    bits = R.act_bits(out, act)
    S, SX = R.bn_bwd_sums(dz, bits, y, mean, invstd)
    dgamma, dbeta, coef = R.bn_bwd_finalize(S, SX, gamma, mean, invstd, M, True)
    dy, dres = R.bn_bwd_apply(dz, bits, y, coef)

    if M == 1:          # torch refuses one value per channel in training mode; the formulas still hold: var = 0
        close(mean, y[0])
        close(invstd, torch.full((C,), eps ** -0.5, dtype=torch.float64))
        return
    yt = nchw(y, B, H, W).clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rt = nchw(res, B, H, W).clone().requires_grad_(True) if use_res else None
    rmt, rvt = rm.clone(), rv.clone()
    z = F.batch_norm(yt, rmt, rvt, gt, bt, True, mom, eps)
    if use_res:
        z = z + rt
    z = F.relu(z) if act == 1 else (F.relu6(z) if act == 2 else z)
    z.backward(nchw(dz, B, H, W))
    close(out, rows(z.detach()))
    close(rm2, rmt)
    close(rv2, rvt)
    close(mean, rows(yt.detach()).mean(0))
    close(invstd, 1 / torch.sqrt(rows(yt.detach()).var(0, unbiased=False) + eps))
    close(dy, rows(yt.grad))
    close(dgamma, gt.grad)
    close(dbeta, bt.grad)
    if use_res:
        close(dres, rows(rt.grad))
    # the mask layout round-trips
    assert torch.equal(R.unpack_mask(R.pack_mask(bits), M, C), bits)
    # sums -> statistics is the same map as the two-pass form
    m2, _, i2 = R.bn_stats_from_sums(y.sum(0), (y * y).sum(0), M, eps)
    assert float((m2 - mean).abs().max()) <= 1e-12 * float(mean.abs().max())
    assert float((i2 / invstd - 1).abs().max()) <= 1e-10          # E[y^2] - mu^2 in fp64 at |mu| / sigma = 1.5


@pytest.mark.parametrize("drop_p", [0.0, 0.3])
def test_batchnorm_eval_and_dropout_match_torch(drop_p):
    gen = torch.Generator().manual_seed(5)
    B, H, W, C, eps = 2, 5, 3, 24, 1e-5
    M = B * H * W
    y0 = rnd(gen, M, C)
    gamma, beta = 0.5 + rnd(gen, C).abs(), rnd(gen, C)
    rm, rv = rnd(gen, C), 1 + torch.rand(C, generator=gen, dtype=torch.float64)
    dz = rnd(gen, M, C)
    keep = None
    y = y0
    if drop_p > 0:
        keep = torch.from_numpy(O.dropout_keep_mask_nhwc(M * C, 77, drop_p)).reshape(M, C)
        y = y0 * keep / (1 - drop_p)
    mean, invstd = R.bn_eval_prepare(rm, rv, eps)
    scale, shift = R.bn_eval_affine(rm, rv, gamma, beta, eps)
    out = R.bn_act_fwd(y, mean, invstd, gamma, beta, None, 1)
    close(out, R.act_fwd(y * scale + shift, 1))
    bits = R.act_bits(out, 1)
    S, SX = R.bn_bwd_sums(dz, bits, y, mean, invstd)
    dgamma, dbeta, coef = R.bn_bwd_finalize(S, SX, gamma, mean, invstd, M, False)
    dy, _ = R.bn_bwd_apply(dz, bits, y, coef, keep, drop_p)

    y0t = nchw(y0, B, H, W).clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yt = y0t * nchw(keep.double(), B, H, W) / (1 - drop_p) if drop_p > 0 else y0t
    z = F.relu(F.batch_norm(yt, rm.clone(), rv.clone(), gt, bt, False, 0.1, eps))
    z.backward(nchw(dz, B, H, W))
    close(out, rows(z.detach()))
    close(dy, rows(y0t.grad))
    close(dgamma, gt.grad)
    close(dbeta, bt.grad)


def test_add_n_and_relu_bwd():
    gen = torch.Generator().manual_seed(1)
    ts = [rnd(gen, 7, 12) for _ in range(4)]
    close(R.add_n(ts[:2]), ts[0] + ts[1])
    close(R.add_n(ts), ((ts[0] + ts[1]) + ts[2]) + ts[3])
    o = F.relu(ts[0])
    close(R.relu_bwd(ts[1], o), ts[1] * (o > 0))


@pytest.mark.parametrize("th,tw,Ho,Wo", [(3, 5, 6, 20), (5, 4, 5, 8), (2, 3, 6, 9), (1, 1, 4, 3), (4, 6, 64, 6), (3, 2, 7, 5), (5, 5, 5, 5)])
def test_upsample_matches_interpolate(th, tw, Ho, Wo):
    gen = torch.Generator().manual_seed(th * 10 + Wo)
    B, C, Cd, coff = 2, 4, 12, 4
    src = rnd(gen, B, th, tw, C)
    st = src.permute(0, 3, 1, 2).clone().requires_grad_(True)
    up = F.interpolate(st, size=(Ho, Wo), mode="bilinear", align_corners=False)
    close(R.upsample(src, Ho, Wo), up.detach().permute(0, 2, 3, 1))
    dst = rnd(gen, B, Ho, Wo, Cd)
    got = R.upsample_slice_fwd(dst, src, coff)
    assert torch.equal(got[..., :coff], dst[..., :coff]) and torch.equal(got[..., coff + C:], dst[..., coff + C:])
    close(got[..., coff:coff + C], up.detach().permute(0, 2, 3, 1))
    g = rnd(gen, B, Ho, Wo, Cd)
    up.backward(g[..., coff:coff + C].permute(0, 3, 1, 2))
    close(R.upsample_slice_bwd(g, coff, C, th, tw), st.grad.permute(0, 2, 3, 1))
    # every row of the weight matrix sums to one
    close(R.upsample_matrix(th, tw, Ho, Wo).sum(1), torch.ones(Ho * Wo, dtype=torch.float64))


@pytest.mark.parametrize("relu", [0, 1])
def test_hr_fuse_matches_interpolate(relu):
    gen = torch.Generator().manual_seed(9)
    B, C, Ho, Wo = 2, 8, 8, 12
    terms = [rnd(gen, B, Ho, Wo, C), rnd(gen, B, 4, 6, C), rnd(gen, B, 2, 12, C), rnd(gen, B, 1, 3, C)]
    want = sum(t.permute(0, 3, 1, 2) if t.shape[1:3] == (Ho, Wo)
               else F.interpolate(t.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False) for t in terms)
    want = F.relu(want) if relu else want
    close(R.hr_fuse_fwd(terms, Ho, Wo, relu), want.permute(0, 2, 3, 1))
    close(R.hr_fuse_fwd(terms[1:2], Ho, Wo, relu), (F.relu if relu else (lambda a: a))(
        F.interpolate(terms[1].permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False)).permute(0, 2, 3, 1))


MAXPOOL_CFG = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0), (3, 2, 0)]


def maxpool_input(kind, gen, B, H, W, C):
    if kind == "random":
        return rnd(gen, B, H, W, C)
    if kind == "tied":          # a ReLU output: many exact zeros, few distinct values
        return torch.randint(-3, 3, (B, H, W, C), generator=gen).clamp(min=0).double()
    if kind == "constant":
        return torch.full((B, H, W, C), 1.5, dtype=torch.float64)
    x = rnd(gen, B, H, W, C)
    x[:, : H // 2 + 1] = -float("inf")          # whole windows of -inf
    if kind == "nan":
        x[0, H - 1, W - 2, 0] = float("nan")
        x[0, 0, 0, 0] = float("nan")
    return x


@pytest.mark.parametrize("k,s,p", MAXPOOL_CFG)
@pytest.mark.parametrize("H,W", [(10, 11), (7, 8)])
@pytest.mark.parametrize("kind", ["random", "tied", "constant", "neginf", "nan"])
def test_maxpool_matches_torch(k, s, p, H, W, kind):
    gen = torch.Generator().manual_seed(k * 100 + s * 10 + p + H)
    B, C = 2, 3
    x = maxpool_input(kind, gen, B, H, W, C)
    out, arg = R.maxpool_fwd(x, k, s, p)
    xt = x.permute(0, 3, 1, 2).contiguous()
    ot, it = F.max_pool2d(xt, k, s, p, return_indices=True)
    assert torch.equal(torch.nan_to_num(out, nan=1e30), torch.nan_to_num(ot.permute(0, 2, 3, 1), nan=1e30))
    assert torch.equal(arg.long(), it.permute(0, 2, 3, 1))
    if kind in ("random", "tied", "constant"):
        xg = xt.clone().requires_grad_(True)
        og = F.max_pool2d(xg, k, s, p)
        dout = rnd(gen, *og.shape)
        og.backward(dout)
        close(R.maxpool_bwd(dout.permute(0, 2, 3, 1).contiguous(), arg, H, W), xg.grad.permute(0, 2, 3, 1))


def test_maxpool_uncovered_pixels_get_zero():
    gen = torch.Generator().manual_seed(2)
    x = rnd(gen, 1, 10, 11, 2)
    out, arg = R.maxpool_fwd(x, 3, 3, 0)
    dx = R.maxpool_bwd(torch.ones_like(out), arg, 10, 11)
    assert float(dx[:, 9].abs().max()) == 0 and float(dx[:, :, 9:].abs().max()) == 0 and float(dx.sum()) == out.numel()


@pytest.mark.parametrize("B,HW,C", [(1, 1, 1), (5, 37, 51), (2, 100, 8)])
def test_avgpool_matches_torch(B, HW, C):
    gen = torch.Generator().manual_seed(HW)
    x = rnd(gen, B, HW, C)
    xt = x.permute(0, 2, 1).reshape(B, C, HW, 1).clone().requires_grad_(True)
    o = F.avg_pool2d(xt, (HW, 1))
    close(R.avgpool_fwd(x), o.detach().reshape(B, C))
    d = rnd(gen, B, C)
    o.backward(d.reshape(B, C, 1, 1))
    close(R.avgpool_bwd(d, HW), xt.grad.reshape(B, C, HW).permute(0, 2, 1))


@pytest.mark.parametrize("npix,C", [(1, 4), (37, 20), (300, 260)])
def test_mask_head_matches_torch(npix, C):
    gen = torch.Generator().manual_seed(npix)
    x, w, b = rnd(gen, npix, C), rnd(gen, C) / C ** 0.5, rnd(gen, 1)
    xt, wt, bt = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    m = torch.sigmoid(F.conv2d(xt.t().reshape(1, C, npix, 1), wt.reshape(1, C, 1, 1), bt)) - 0.5
    got = R.mask_head_fwd(x, w, b)
    close(got, m.detach().reshape(npix))
    dm = rnd(gen, npix)
    m.backward(dm.reshape(1, 1, npix, 1))
    dx, dw, db = R.mask_head_bwd(dm, got, x, w)
    close(dx, xt.grad)
    close(dw, wt.grad)
    close(db, bt.grad)


@pytest.mark.parametrize("B,K,HW", [(1, 2, 1), (3, 51, 37), (2, 150, 5)])
def test_pred_assemble_matches_autograd(B, K, HW):
    gen = torch.Generator().manual_seed(K)
    cls, m = rnd(gen, B, K), rnd(gen, B, HW)
    ct, mt = cls.clone().requires_grad_(True), m.clone().requires_grad_(True)
    pred = torch.cat([ct[:, :K - 1, None].expand(B, K - 1, HW), (ct[:, K - 1:, None] * mt[:, None, :])], 1)
    assert torch.equal(R.pred_assemble_fwd(cls, m), pred.detach())
    dp = rnd(gen, B, K, HW)
    pred.backward(dp)
    dcls, dm = R.pred_assemble_bwd(dp, cls, m)
    close(dcls, ct.grad)
    close(dm, mt.grad)


@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_adam_matches_torch(wd, gs):
    gen = torch.Generator().manual_seed(3)
    n = 37
    f32 = lambda a: float(np.float32(a))          # noqa: E731  -- the scalars as the C ABI carries them
    lr, b1, b2, eps, wd = f32(2e-5), f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    p = torch.nn.Parameter(rnd(gen, n))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    pr, mr, vr = p.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = rnd(gen, n) * (10.0 ** (step - 3))
        p.grad = g * gs          # grad_scale multiplies the gradient before anything else
        opt.step()
        pr, mr, vr = R.adam_step(pr, g, mr, vr, lr, b1, b2, eps, wd, step, gs)
        close(pr, p.detach())
        close(mr, opt.state[p]["exp_avg"])
        close(vr, opt.state[p]["exp_avg_sq"])
