"""oracle/frontend_ref.py against torch in fp64 (CPU).  The references are what tests/test_frontend_kernels.py holds the HIP kernels
of csrc/frontend.hip and the segmentation loss of csrc/head_loss.hip to; here each is held to the torch operators it restates
(F.interpolate bilinear / area, F.grid_sample, softmax(conv2d(relu)), the min/max-normalised MSE and O.create_grid_f64, each with
autograd, and O.focal_loss / O.dice_loss_multiclass / O.accuracies) at small ragged shapes, to fp64 rounding: 1e-12 relative to
sum|terms| (the `mag` the references return, or the largest reference value where there is none)."""
import pytest
import torch
import torch.nn.functional as F

import frontend_ref as R
import fovealseg_oracle as O

TOL = 1e-12


def close(a, b, mag=None, tol=TOL):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = float(b.abs().max()) if mag is None else mag.double().clamp_min(float(b.abs().max()) * 1e-3)
    err = (a - b).abs()
    assert bool((err <= tol * torch.as_tensor(scale).clamp_min(1e-300)).all()), float(err.max())


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def grad_of(fn, *inputs, cot):
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    return torch.autograd.grad(out, leaves, cot)


GAZE_SHAPES = [(1, 4, 4, 2, 2), (3, 16, 16, 16, 16), (2, 37, 53, 7, 5), (2, 9, 11, 20, 24), (1, 64, 16, 8, 2), (2, 32, 32, 13, 11)]


@pytest.mark.parametrize("B,H,W,hs,ws", GAZE_SHAPES)
def test_gaze_lowres_matches_interpolate(B, H, W, hs, ws):
    gen = torch.Generator().manual_seed(H * W + hs)
    x = rnd(gen, B, 3, H, W)
    focus = torch.rand(B, 2, generator=gen, dtype=torch.float64)
    focus[0] = 0.0
    focus[-1] = 1.0
    out, mag = R.gaze_lowres(x, focus, hs, ws)
    ref = O.lowres_input(x, focus, hs, ws).permute(0, 2, 3, 1)
    close(out[..., :3], ref[..., :3], mag)
    close(out[..., 3:], ref[..., 3:])
    assert torch.equal(out[..., 3], out[..., 4])


@pytest.mark.parametrize("B,HW,C", [(1, 1, 1), (3, 63, 3), (2, 130, 24), (1, 7, 32)])
def test_compress_matches_conv2d(B, HW, C):
    gen = torch.Generator().manual_seed(HW + C)
    s = rnd(gen, B, HW, C)
    s[0, 0, 0] = 0.0
    s[-1, -1, -1] = -0.0
    w, bias, g = rnd(gen, C), rnd(gen, 1), rnd(gen, B, HW)

    def torch_logit(s_, w_, b_):
        return F.conv2d(F.relu(s_.permute(0, 2, 1)[..., None]), w_.view(1, C, 1, 1), b_)[:, 0, :, 0]
    out, mag = R.compress_fwd(s, w, bias)
    close(out, torch_logit(s, w, bias), mag)
    ds_t, dw_t, db_t = grad_of(torch_logit, s, w, bias, cot=g)
    ds, dw, db, mdw, mdb = R.compress_bwd(g, s, w)
    close(ds, ds_t)
    close(dw, dw_t, mdw)
    close(db, db_t, mdb)

    def torch_xs(s_, w_, b_):
        return torch.softmax(torch_logit(s_, w_, b_), dim=1)
    xs, _, _ = R.compress_softmax_fwd(s, w, bias)
    close(xs, torch_xs(s, w, bias))
    ds_t, dw_t, db_t = grad_of(torch_xs, s, w, bias, cot=g)
    ds, dw, db, dl, _ = R.compress_softmax_bwd(g, xs, s, w)
    scale = (xs * g.abs()).sum(1).max()          # the terms of the softmax adjoint
    close(ds, ds_t, scale * w.abs().max() * torch.ones_like(ds))
    close(dw, dw_t, (dl.abs()[..., None] * s.abs()).reshape(-1, C).sum(0) + scale * s.abs().max())
    close(db, db_t, dl.abs().sum().reshape(1) + scale)


@pytest.mark.parametrize("B,H,W,hs,ws", [(1, 2, 2, 2, 2), (2, 7, 9, 3, 4), (1, 13, 16, 5, 4), (2, 40, 64, 3, 8), (1, 33, 51, 8, 8), (1, 2, 64, 1, 2)])
def test_area_pool_matches_interpolate(B, H, W, hs, ws):
    gen = torch.Generator().manual_seed(H + W)
    y = rnd(gen, B, H, W)
    out, mag = R.area_pool(y, hs, ws)
    close(out, F.interpolate(y[:, None], size=(hs, ws), mode="area")[:, 0], mag)


def _torch_edge(xs, t, coef):
    a = (xs - xs.min()) / (xs.max() - xs.min())
    b = (t - t.min()) / (t.max() - t.min())
    return coef * F.mse_loss(a, b)


@pytest.mark.parametrize("n,ties", [(2, 1), (7, 1), (7, 3), (200, 1), (200, 3), (200, 64)])
def test_edge_loss_matches_autograd_with_ties(n, ties):
    gen = torch.Generator().manual_seed(n + ties)
    xs = torch.rand(n, generator=gen, dtype=torch.float64) * 0.5 + 0.25
    t = torch.rand(n, generator=gen, dtype=torch.float64)
    perm = torch.randperm(n, generator=gen)
    k = min(ties, n // 2)
    xs[perm[:k]] = 0.125                # the minimum, k times
    xs[perm[k:2 * k]] = 0.875           # the maximum, k times
    coef, gout = 5.0, 0.37
    loss, stats = R.edge_loss_fwd(xs, t, coef)
    close(loss, _torch_edge(xs, t, coef))
    assert stats.tolist() == [0.125, 0.875, float(t.min()), float(t.max()), float(k), float(k)]
    (dx_t,) = grad_of(lambda a: _torch_edge(a, t, coef), xs, cot=torch.tensor(gout, dtype=torch.float64))
    dx = R.edge_loss_bwd(xs, t, coef, gout)
    close(dx, dx_t, torch.full_like(dx, float(dx_t.abs().sum())))


def test_edge_loss_matches_oracle_edge_loss():
    gen = torch.Generator().manual_seed(5)
    xs = torch.softmax(rnd(gen, 2, 1, 36).reshape(2, -1), 1).reshape(2, 1, 6, 6)
    y = (torch.rand(2, 1, 24, 30, generator=gen) > 0.5).double()
    t, _ = R.area_pool(y[:, 0], 6, 6)
    loss, _ = R.edge_loss_fwd(xs.reshape(-1), t.reshape(-1), 0.05 * 100.0)
    close(loss, O.edge_loss(xs, y, 6, 6, 100.0))


GAUSS_SHAPES = [(2, 2, 1), (3, 5, 2), (9, 7, 3), (9, 7, 6), (20, 17, 30), (12, 3, 20)]


GAUSS_CASES = [(hs, ws, pad, mode) for hs, ws, pad in GAUSS_SHAPES for mode in ("replication", "reflect", "zero")
               if mode != "reflect" or pad <= min(hs, ws) - 1]          # F.pad(mode='reflect') refuses a pad beyond the side


@pytest.mark.parametrize("hs,ws,pad,mode", GAUSS_CASES)
def test_gauss_grid_matches_create_grid_f64(hs, ws, pad, mode):
    gen = torch.Generator().manual_seed(hs * ws + pad)
    B = 2
    xs = torch.softmax(2 * rnd(gen, B, hs * ws), 1).reshape(B, hs, ws)
    g1d = torch.from_numpy(O.gaussian_1d(2 * pad + 1, pad))
    m = {"replication": R.PAD_REPLICATION, "reflect": R.PAD_REFLECT, "zero": R.PAD_ZERO}[mode]
    u, grid, parts = R.gauss_grid_fwd(xs, g1d, pad, m)
    ref = O.create_grid_f64(xs[:, None], pad, mode)
    close(grid, ref, tol=1e-11)
    assert torch.equal(grid, u.clamp(-1, 1))
    # the cotangent is zeroed on the knife edge only (|u| within 1e-9 of 1: reflect puts the border components there); clearly
    # clamped components keep theirs
    cot = rnd(gen, B, hs, ws, 2)
    cot = torch.where(((u.abs() - 1).abs() <= 1e-9), torch.zeros_like(cot), cot)
    (dx_t,) = grad_of(lambda a: O.create_grid_f64(a[:, None], pad, mode), xs, cot=cot)
    dx, bp = R.gauss_grid_bwd(xs, g1d, cot, pad, m)
    mag = bp["absmap"](bp["dp"].abs() + (bp["dax"] * bp["ax"]).abs() / bp["p"] + (bp["day"] * bp["ay"]).abs() / bp["p"], bp["dax"].abs(), bp["day"].abs())
    close(dx, dx_t, mag, tol=1e-11)
    if mode == "replication" and pad >= 20:          # only replicated borders pull the centroid beyond the map
        assert bool(((u.abs() > 1 + 1e-4) & (cot != 0)).any()), "no clearly clamped component carries a cotangent"


@pytest.mark.parametrize("n", [2, 5])
def test_gauss_grid_identity_filter(n):
    xs = torch.full((1, n, n + 1), 0.25, dtype=torch.float64)
    _, grid, _ = R.gauss_grid_fwd(xs, torch.ones(1, dtype=torch.float64), 0)
    gx = 2 * torch.arange(n + 1, dtype=torch.float64) / n - 1
    gy = 2 * torch.arange(n, dtype=torch.float64) / (n - 1) - 1
    close(grid[0, :, :, 0], gx[None, :].expand(n, n + 1))
    close(grid[0, :, :, 1], gy[:, None].expand(n, n + 1))


@pytest.mark.parametrize("h,w,H,W", [(1, 1, 4, 3), (7, 5, 10, 16), (5, 7, 16, 9), (4, 4, 4, 4), (3, 2, 6, 6), (3, 3, 12, 15), (2, 3, 2, 6),
                                     (1, 4, 7, 8), (4, 1, 8, 9), (3, 4, 18, 28)])
def test_grid_upsample_matches_interpolate(h, w, H, W):
    gen = torch.Generator().manual_seed(h * w + H)
    B = 3
    grid = rnd(gen, B, h, w, 2)
    cot = rnd(gen, B, H, W, 2)

    def torch_up(g):
        return F.interpolate(g.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    out, mag = R.grid_upsample_fwd(grid, H, W)
    close(out, torch_up(grid), mag)
    (dg_t,) = grad_of(torch_up, grid, cot=cot)
    dg, dmag = R.grid_upsample_bwd(cot, h, w)
    close(dg, dg_t, dmag)


def special_grid(gen, B, h, w, H, W):
    """random points in [-1, 1] and, spread over the first entries, the edge values of both coordinates"""
    grid = torch.rand(B, h, w, 2, generator=gen, dtype=torch.float64) * 2 - 1
    flat = grid.reshape(-1, 2)
    vals = [-1.0, 1.0, 1 + 1.0 / W, -(1 + 1.0 / W), 3.0, -3.0, 1e6, -1e6]
    for i, v in enumerate(vals):
        if 2 * i + 1 < flat.shape[0]:
            flat[2 * i, 0] = v
            flat[2 * i + 1, 1] = v if abs(v) != 1 + 1.0 / W else v / abs(v) * (1 + 1.0 / H)
    return grid


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 4), (12, 9)])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (6, 7)])
@pytest.mark.parametrize("B,C", [(1, 1), (2, 3)])
def test_grid_sample_matches_torch(H, W, h, w, B, C):
    gen = torch.Generator().manual_seed(H * W + h * w + C)
    x = rnd(gen, B, C, H, W)
    grid = special_grid(gen, B, h, w, H, W)
    # keep every coordinate off the integer lattice (where the gradient with respect to the grid jumps): the half-outside values
    # +-(1 + 1/W) sit on it and are compared in the forward only
    t = R.grid_taps(grid, H, W)
    on_x = (t["ix"] - t["ix"].round()).abs() < 1e-6
    on_y = (t["iy"] - t["iy"].round()).abs() < 1e-6
    cot = rnd(gen, B, C, h, w)

    def torch_gs(x_, g_):
        return F.grid_sample(x_, g_, mode="bilinear", padding_mode="zeros", align_corners=False)
    out, mag = R.grid_sample_fwd(x, grid)
    close(out, torch_gs(x, grid), mag + 1e-9 * x.abs().max())
    dx_t, dg_t = grad_of(torch_gs, x, grid, cot=cot)
    dg, gmag = R.grid_sample_bwd_grid(cot, x, grid)
    keep = torch.stack((~on_x, ~on_y), -1)
    close(torch.where(keep, dg, torch.zeros_like(dg)), torch.where(keep, dg_t, torch.zeros_like(dg)), gmag + 1e-9 * float(dg_t.abs().max() + 1))
    dx, dmag, cnt = R.grid_sample_bwd_input(cot, grid, H, W)
    close(dx, dx_t, dmag + 1e-9 * float(cot.abs().max()))
    assert float(cnt.sum()) == float(sum(int(ok.sum()) for _, _, ok, _ in R._corners(t)))
    lab, v = R.grid_sample_label(x[:, 0], grid)
    v_t = torch_gs(x[:, :1], grid)[:, 0]
    close(v, v_t, mag[:, 0] + 1e-9 * x.abs().max())
    off = (v_t - v_t.round()).abs() > 1e-9          # the truncation is compared away from the integers, where rounding cannot flip it
    assert torch.equal(lab[off], v_t.long()[off]) and torch.equal(lab, torch.trunc(v).long())


def seg_inputs(gen, B, K, HW, kind):
    if kind == "ties":
        pred = torch.randint(-2, 3, (B, K, HW), generator=gen).double()
    elif kind == "saturated":
        pred = torch.where(torch.rand(B, K, HW, generator=gen) > 0.5, 60.0, -60.0).double()
    else:
        pred = rnd(gen, B, K, HW) * 3
    gt = torch.randint(0, K, (B, HW), generator=gen)
    if kind == "absent":
        gt = gt // 2 * 2 % K          # odd classes never occur
    return pred, gt


@pytest.mark.parametrize("gamma", [5.0, 0.0])
@pytest.mark.parametrize("B,K,HW,kind", [(1, 2, 1, "random"), (3, 7, 45, "random"), (2, 51, 40, "absent"), (2, 64, 33, "random"),
                                         (2, 5, 60, "ties"), (2, 7, 45, "saturated")])
def test_seg_loss_matches_oracle_losses(B, K, HW, kind, gamma):
    gen = torch.Generator().manual_seed(K + HW)
    pred, gt = seg_inputs(gen, B, K, HW, kind)
    eps, gout = 1e-7, 0.37
    out, coef, parts = R.seg_loss_fwd(pred, gt, gamma, eps)
    p4, g4 = pred.reshape(B, K, HW, 1), gt.reshape(B, HW, 1)
    fl, dl = O.focal_loss(p4, g4, gamma), O.dice_loss_multiclass(p4, g4, eps)
    close(out[1], fl)
    close(out[2], dl)
    close(out[0], fl + dl)
    acc = O.accuracies(p4, g4, bg=K - 1)          # torch's argmax keeps the first maximal class on the CPU
    close(out[3:], torch.stack([a.double() for a in acc]), tol=1e-6)          # O.accuracies divides in fp32
    if kind == "absent":
        assert bool((coef[1:K:2] == 0).all()) and bool((coef[K + 1::2] == 0).all())
    if kind == "ties":
        assert bool((R.first_argmax(pred) == pred.argmax(1)).all())
        assert float((pred == pred.max(1, keepdim=True).values).sum(1).double().mean()) > 1.2          # ties do occur

    def torch_loss(p_):
        q = p_.reshape(B, K, HW, 1)
        return O.focal_loss(q, g4, gamma) + O.dice_loss_multiclass(q, g4, eps)
    (dp_t,) = grad_of(torch_loss, pred, cot=torch.tensor(gout, dtype=torch.float64))
    dp, bp = R.seg_loss_bwd(pred, gt, coef, gout, gamma)
    close(dp, dp_t, gout * (bp["p"] * (bp["q"].abs() + bp["absdot"]) + bp["fw"] * (bp["onehot"] + bp["p"])))
