"""Plain references of the foveation front-end kernels (csrc/frontend.hip) and of the segmentation loss (csrc/head_loss.hip),
one function per entry point, written from the formulas in include/fovealseg.h.

Every function works on torch tensors in the kernels' layouts and computes in the dtype of its inputs: fp64 inputs give the
reference, fp32 inputs give "the same formula in fp32", which the GPU tests use as the error scale of a correct fp32
evaluation.  Nothing here calls F.interpolate, F.grid_sample, F.pad, F.softmax, conv2d or autograd: those are what
tests/test_frontend_ref.py checks these functions against.  Windows, taps and paddings are explicit loops or index
arithmetic; the backward functions are hand-written adjoints.

Where a test needs sum|terms| for a bound the function returns it as well (`mag`: the same linear map on absolute values).
"""
import math

import torch

PAD_REPLICATION, PAD_REFLECT, PAD_ZERO = 0, 1, 2


def _scalar(v, like):
    return torch.tensor(v, dtype=like.dtype)


# ------------------------------------------------------------------------------------------------
# bilinear interpolation tables (ATen upsample_bilinear2d, align_corners=False)
# ------------------------------------------------------------------------------------------------
def lerp_table(n_in, n_out, dtype, identity_when_equal=False):
    """Per output index d: source position s = max(n_in / n_out * (d + 0.5) - 0.5, 0), taps i0 = floor(s), i1 = min(i0 + 1, n_in - 1),
    weights l1 = s - i0, l0 = 1 - l1.  Returns (i0, i1, l0, l1, s)."""
    d = torch.arange(n_out, dtype=dtype)
    if identity_when_equal and n_in == n_out:
        i = torch.arange(n_out)
        return i, i.clone(), torch.ones(n_out, dtype=dtype), torch.zeros(n_out, dtype=dtype), d
    scale = _scalar(n_in, d) / _scalar(n_out, d)
    s = torch.clamp(scale * (d + 0.5) - 0.5, min=0.0)
    i0 = torch.floor(s).long()
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = s - i0.to(dtype)
    return i0, i1, 1.0 - l1, l1, s


def lerp_matrix(n_in, n_out, dtype, identity_when_equal=False):
    """The table as a dense (n_out, n_in) matrix (both taps added: they coincide at the far border)."""
    i0, i1, l0, l1, _ = lerp_table(n_in, n_out, dtype, identity_when_equal)
    M = torch.zeros(n_out, n_in, dtype=dtype)
    r = torch.arange(n_out)
    M.index_put_((r, i0), l0, accumulate=True)
    M.index_put_((r, i1), l1, accumulate=True)
    return M


def _bilinear(x, hs, ws, identity_when_equal=False):
    """x (..., H, W) -> (..., hs, ws): ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11), in that order"""
    H, W = x.shape[-2:]
    y0, y1, ly0, ly1, _ = lerp_table(H, hs, x.dtype, identity_when_equal)
    x0, x1, lx0, lx1, _ = lerp_table(W, ws, x.dtype, identity_when_equal)
    top, bot = x[..., y0, :], x[..., y1, :]
    ly0, ly1 = ly0[:, None], ly1[:, None]
    return ly0 * (lx0 * top[..., x0] + lx1 * top[..., x1]) + ly1 * (lx0 * bot[..., x0] + lx1 * bot[..., x1])


# ------------------------------------------------------------------------------------------------
# K1: gaze map + low-resolution RGB
# ------------------------------------------------------------------------------------------------
def gaze_lowres(x, focus, hs, ws):
    """fs_gaze_lowres_fwd: x (B,3,H,W), focus (B,2) = (row, col) -> out (B,hs,ws,5): bilinear RGB, then twice the squared
    distance to the focus point over the squared diagonal.  Returns (out, mag) with mag (B,hs,ws,3) the lerp of |x|."""
    B = x.shape[0]
    rgb = _bilinear(x, hs, ws).permute(0, 2, 3, 1)
    mag = _bilinear(x.abs(), hs, ws).permute(0, 2, 3, 1)
    h = focus[:, 0] * (hs - 1)
    w = focus[:, 1] * (ws - 1)
    dy = torch.arange(hs, dtype=x.dtype)[None, :, None] - h[:, None, None]
    dx = torch.arange(ws, dtype=x.dtype)[None, None, :] - w[:, None, None]
    dist = torch.sqrt(dy * dy + dx * dx)
    maxd = _scalar(math.sqrt(float(hs) * hs + float(ws) * ws), x)
    r = dist / maxd
    g = (r * r).expand(B, hs, ws)[..., None]
    return torch.cat((rgb, g, g), dim=3), mag


# ------------------------------------------------------------------------------------------------
# K3: ReLU -> 1x1 conv C -> 1 (-> softmax over the pixels)
# ------------------------------------------------------------------------------------------------
def _relu(s):
    return torch.where(s < 0, torch.zeros_like(s), s)


def compress_fwd(s, w, bias):
    """fs_compress_fwd: s (B,HW,C) -> logits (B,HW) = w . relu(s) + bias.  Returns (out, mag)."""
    r = _relu(s)
    return (r * w).sum(-1) + bias[0], (r * w.abs()).sum(-1) + bias[0].abs()


def compress_bwd(g, s, w):
    """fs_compress_bwd: ds = g w (s > 0), dw = sum g relu(s), db = sum g.  Returns (ds, dw, db, mag_dw, mag_db)."""
    r = _relu(s)
    ds = torch.where(s > 0, g[..., None] * w, torch.zeros_like(s))
    C = s.shape[-1]
    return (ds, (g[..., None] * r).reshape(-1, C).sum(0), g.sum().reshape(1),
            (g.abs()[..., None] * r).reshape(-1, C).sum(0), g.abs().sum().reshape(1))


def compress_softmax_fwd(s, w, bias):
    """fs_compress_softmax_fwd: xs (B,HW) = softmax over HW of the logits.  Returns (xs, logit, mag of the logit)."""
    logit, mag = compress_fwd(s, w, bias)
    m = logit.max(dim=1, keepdim=True).values
    e = torch.exp(logit - m)
    return e / e.sum(dim=1, keepdim=True), logit, mag


def compress_softmax_bwd(g, xs, s, w):
    """fs_compress_softmax_bwd: dlogit = xs (g - sum(g xs)); ds = dlogit w (s > 0); dw = sum dlogit relu(s); db = sum dlogit.
    Returns (ds, dw, db, dlogit, dot)."""
    dot = (g * xs).sum(dim=1, keepdim=True)
    dl = xs * (g - dot)
    ds, dw, db, _, _ = compress_bwd(dl, s, w)
    return ds, dw, db, dl, dot


# ------------------------------------------------------------------------------------------------
# K11: area pool and the min/max-normalised MSE
# ------------------------------------------------------------------------------------------------
def area_windows(n_in, n_out):
    """[floor(o n_in / n_out), ceil((o + 1) n_in / n_out)) for o in range(n_out)"""
    return [((o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)) for o in range(n_out)]


def area_pool(y, hs, ws):
    """fs_area_pool_fwd: y (B,H,W) -> (B,hs,ws), the mean over each window: the rows of a column first, then the columns.
    Returns (out, mag)."""
    B, H, W = y.shape
    out = torch.zeros(B, hs, ws, dtype=y.dtype)
    mag = torch.zeros(B, hs, ws, dtype=y.dtype)
    wx = area_windows(W, ws)
    for oy, (y0, y1) in enumerate(area_windows(H, hs)):
        col = y[:, y0:y1, :].sum(1)
        acol = y[:, y0:y1, :].abs().sum(1)
        for ox, (x0, x1) in enumerate(wx):
            n = (y1 - y0) * (x1 - x0)
            out[:, oy, ox] = col[:, x0:x1].sum(1) / n
            mag[:, oy, ox] = acol[:, x0:x1].sum(1) / n
    return out, mag


def edge_loss_fwd(xs, t, coef):
    """fs_edge_loss_fwd on flat xs, t (n): loss = coef * mean(((xs - min) / (max - min) - (t - tmin) / (tmax - tmin))^2) with
    whole-batch min / max.  Returns (loss, stats) with stats = [xs_min, xs_max, t_min, t_max, n_argmin, n_argmax]."""
    mn, mx, tmn, tmx = xs.min(), xs.max(), t.min(), t.max()
    u = (xs - mn) / (mx - mn)
    v = (t - tmn) / (tmx - tmn)
    d = u - v
    loss = coef * ((d * d).sum() / xs.numel())
    stats = torch.stack((mn, mx, tmn, tmx, (xs == mn).sum().to(xs.dtype), (xs == mx).sum().to(xs.dtype)))
    return loss, stats


def edge_loss_bwd(xs, t, coef, gout):
    """fs_edge_loss_bwd: d loss / d xs times gout.  With g_i = d loss / d u_i = 2 coef gout (u_i - v_i) / n and r = max - min:
    dxs_i = g_i / r  +  [xs_i == min] (sum_j g_j (u_j - 1) / r) / n_argmin  +  [xs_i == max] (-sum_j g_j u_j / r) / n_argmax
    (min and max hand their gradient to every element that attains them in equal shares, as torch's amin / amax do)."""
    n = xs.numel()
    mn, mx, tmn, tmx = xs.min(), xs.max(), t.min(), t.max()
    r = mx - mn
    u = (xs - mn) / r
    v = (t - tmn) / (tmx - tmn)
    g = (2.0 * coef * gout / n) * (u - v)
    is_mn, is_mx = xs == mn, xs == mx
    dmn = (g * (u - 1.0)).sum() / r / is_mn.sum()
    dmx = -(g * u).sum() / r / is_mx.sum()
    return g / r + is_mn.to(xs.dtype) * dmn + is_mx.to(xs.dtype) * dmx


# ------------------------------------------------------------------------------------------------
# K4: padded separable Gaussian centroid -> sampling grid
# ------------------------------------------------------------------------------------------------
def padmap(t, n, mode):
    """source index the padded position t (t = j - pad, any integer tensor) reads; -1 = nothing (zero padding)"""
    if mode == PAD_REPLICATION:
        return t.clamp(0, n - 1)
    if mode == PAD_REFLECT:
        return torch.where(t < 0, -t, torch.where(t > n - 1, 2 * (n - 1) - t, t))
    return torch.where((t < 0) | (t > n - 1), torch.full_like(t, -1), t)


def gauss_matrices(n, pad, g1d, mode):
    """M0[o, x] = sum of g[s] over the taps s of output o whose padded position o + s reads source x,
    M1[o, x] = the same with g[s] c(o + s), c(j) = (j - pad) / (n - 1).  Both (n, n), dtype of g1d."""
    K = 2 * pad + 1
    o = torch.arange(n)[:, None].expand(n, K)
    s = torch.arange(K)[None, :].expand(n, K)
    j = o + s
    src = padmap(j - pad, n, mode)
    keep = src >= 0
    c = (j - pad).to(g1d.dtype) / (n - 1)
    gv = g1d[s]
    M0 = torch.zeros(n, n, dtype=g1d.dtype)
    M1 = torch.zeros(n, n, dtype=g1d.dtype)
    M0.index_put_((o[keep], src[keep]), gv[keep], accumulate=True)
    M1.index_put_((o[keep], src[keep]), (gv * c)[keep], accumulate=True)
    return M0, M1


def _gauss_parts(xs, g1d, pad, mode):
    B, hs, ws = xs.shape
    My0, My1 = gauss_matrices(hs, pad, g1d, mode)
    Mx0, Mx1 = gauss_matrices(ws, pad, g1d, mode)
    p = My0 @ xs @ Mx0.T
    ax = My0 @ xs @ Mx1.T
    ay = My1 @ xs @ Mx0.T
    return (My0, My1, Mx0, Mx1), p, ax, ay


def gauss_grid_fwd(xs, g1d, pad, mode=PAD_REPLICATION):
    """fs_gauss_grid_fwd(_mode): xs (B,hs,ws) -> u (B,hs,ws,2) = (2 ax / p - 1, 2 ay / p - 1) and grid = clamp(u, -1, 1), with
    p = sum g[r] g[s] x~[oy + r][ox + s], ax = the same with c_x(ox + s), ay with c_y(oy + r), x~ the padded map.
    Returns (u, grid, parts) with parts = dict(p, ax, ay, absax, absay): absax / absay the sums of |g g x~ c|."""
    xs = xs.to(g1d.dtype)
    (My0, My1, Mx0, Mx1), p, ax, ay = _gauss_parts(xs, g1d, pad, mode)
    u = torch.stack((ax / p * 2.0 - 1.0, ay / p * 2.0 - 1.0), dim=-1)
    parts = dict(p=p, ax=ax, ay=ay, absax=My0 @ xs.abs() @ Mx1.abs().T, absay=My1.abs() @ xs.abs() @ Mx0.T)
    return u, u.clamp(-1.0, 1.0), parts


def gauss_grid_bwd(xs, g1d, dgrid, pad, mode=PAD_REPLICATION):
    """fs_gauss_grid_bwd(_mode): the adjoint of gauss_grid_fwd; the clamp passes gradient exactly where -1 <= u <= 1.
    Returns (dxs, parts) with parts = dict(dp, dax, day, absmap): absmap(a, b, c) runs the transposed filter on non-negative
    (dp, dax, day)-shaped arguments with the absolute weights."""
    xs = xs.to(g1d.dtype)
    dgrid = dgrid.to(g1d.dtype)
    (My0, My1, Mx0, Mx1), p, ax, ay = _gauss_parts(xs, g1d, pad, mode)
    ux, uy = ax / p * 2.0 - 1.0, ay / p * 2.0 - 1.0
    zero = torch.zeros_like(p)
    dgx = torch.where((ux >= -1.0) & (ux <= 1.0), dgrid[..., 0], zero)
    dgy = torch.where((uy >= -1.0) & (uy <= 1.0), dgrid[..., 1], zero)
    dax, day = 2.0 * dgx / p, 2.0 * dgy / p
    dp = -(dax * ax + day * ay) / p
    dxs = My0.T @ dp @ Mx0 + My0.T @ dax @ Mx1 + My1.T @ day @ Mx0

    def absmap(a, b, c):
        return My0.T @ a @ Mx0 + My0.T @ b @ Mx1.abs() + My1.abs().T @ c @ Mx0
    return dxs, dict(dp=dp, dax=dax, day=day, p=p, ax=ax, ay=ay, absmap=absmap)


# ------------------------------------------------------------------------------------------------
# grid up-sampling
# ------------------------------------------------------------------------------------------------
def grid_upsample_fwd(grid, H, W):
    """fs_grid_upsample_fwd: grid (B,h,w,2) -> (B,H,W,2), bilinear, align_corners=False (equal sizes copy).  Returns (out, mag)."""
    g = grid.permute(0, 3, 1, 2)
    return _bilinear(g, H, W, True).permute(0, 2, 3, 1), _bilinear(g.abs(), H, W, True).permute(0, 2, 3, 1)


def grid_upsample_bwd(g, h, w):
    """fs_grid_upsample_bwd: g (B,H,W,2) -> dgrid (B,h,w,2), the transpose of the forward map.  Returns (dgrid, mag)."""
    B, H, W, _ = g.shape
    Wy = lerp_matrix(h, H, g.dtype, True)
    Wx = lerp_matrix(w, W, g.dtype, True)
    gp = g.permute(0, 3, 1, 2)
    return (Wy.T @ gp @ Wx).permute(0, 2, 3, 1), (Wy.T @ gp.abs() @ Wx).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------
# K5 / K6: grid_sample, bilinear, zeros padding, align_corners=False
# ------------------------------------------------------------------------------------------------
def grid_taps(grid, H, W, dix=0.0, diy=0.0):
    """ix = (gx + 1) W / 2 - 0.5 (+ dix), x0 = floor(ix), w = ix - x0, e = 1 - w; likewise iy, y0, n, s.  Coordinates beyond the
    image by more than a pixel are clamped to x0 = -2 / W + 1 (every tap outside).  Returns a dict."""
    dt = grid.dtype
    ix = (grid[..., 0] + 1.0) * _scalar(W * 0.5, grid) - 0.5 + dix
    iy = (grid[..., 1] + 1.0) * _scalar(H * 0.5, grid) - 0.5 + diy
    fx, fy = torch.floor(ix), torch.floor(iy)
    w, n = ix - fx, iy - fy
    x0 = fx.clamp(-2, W + 1).long()
    y0 = fy.clamp(-2, H + 1).long()
    t = dict(ix=ix, iy=iy, x0=x0, y0=y0, w=w, e=1.0 - w, n=n, s=1.0 - n)
    t["okx0"], t["okx1"] = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
    t["oky0"], t["oky1"] = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    t["dtype"] = dt
    return t


def _corners(t):
    """the four taps as (dy, dx, ok, weight): nw, ne, sw, se"""
    return [(0, 0, t["oky0"] & t["okx0"], t["s"] * t["e"]), (0, 1, t["oky0"] & t["okx1"], t["s"] * t["w"]),
            (1, 0, t["oky1"] & t["okx0"], t["n"] * t["e"]), (1, 1, t["oky1"] & t["okx1"], t["n"] * t["w"])]


def _gather(x, t, dy, dx, ok):
    """x (B,C,H,W), taps over (B,h,w) -> (B,C,h,w): x[b, c, y0 + dy, x0 + dx] where ok, else 0"""
    B, C, H, W = x.shape
    yy = (t["y0"] + dy).clamp(0, H - 1)
    xx = (t["x0"] + dx).clamp(0, W - 1)
    lin = (yy * W + xx).reshape(B, 1, -1).expand(B, C, -1)
    v = x.reshape(B, C, H * W).gather(2, lin).reshape(B, C, *t["x0"].shape[1:])
    return torch.where(ok[:, None], v, torch.zeros_like(v))


def grid_sample_fwd(x, grid, dix=0.0, diy=0.0):
    """fs_grid_sample_fwd: x (B,C,H,W), grid (B,h,w,2) = (x, y) -> out (B,C,h,w) = nw v_nw + ne v_ne + sw v_sw + se v_se.
    Returns (out, mag)."""
    t = grid_taps(grid, x.shape[2], x.shape[3], dix, diy)
    out, mag = 0.0, 0.0
    for dy, dx, ok, wgt in _corners(t):
        v = _gather(x, t, dy, dx, ok)
        out = out + v * wgt[:, None]
        mag = mag + v.abs() * wgt[:, None]
    return out, mag


def grid_sample_label(y, grid):
    """fs_grid_sample_label: y (B,H,W) -> (trunc(sample) as int64, sample), both (B,h,w)"""
    v = grid_sample_fwd(y[:, None], grid)[0][:, 0]
    return torch.trunc(v).long(), v


def grid_sample_bwd_grid(gout, x, grid, dix=0.0, diy=0.0):
    """fs_grid_sample_bwd_grid: gout (B,C,h,w) -> dgrid (B,h,w,2):
    d/dgx = W/2 sum_c gout ((v_ne - v_nw) s + (v_se - v_sw) n),  d/dgy = H/2 sum_c gout ((v_sw - v_nw) e + (v_se - v_ne) w).
    Returns (dgrid, mag)."""
    H, W = x.shape[2:]
    t = grid_taps(grid, H, W, dix, diy)
    (vnw, vne, vsw, vse) = [_gather(x, t, dy, dx, ok) for dy, dx, ok, _ in _corners(t)]
    s, n, e, w = t["s"][:, None], t["n"][:, None], t["e"][:, None], t["w"][:, None]
    gx = (gout * ((vne - vnw) * s + (vse - vsw) * n)).sum(1) * (W * 0.5)
    gy = (gout * ((vsw - vnw) * e + (vse - vne) * w)).sum(1) * (H * 0.5)
    a = gout.abs()
    mx = (a * ((vne.abs() + vnw.abs()) * s + (vse.abs() + vsw.abs()) * n)).sum(1) * (W * 0.5)
    my = (a * ((vsw.abs() + vnw.abs()) * e + (vse.abs() + vne.abs()) * w)).sum(1) * (H * 0.5)
    return torch.stack((gx, gy), -1), torch.stack((mx, my), -1)


def grid_sample_bwd_input(gout, grid, H, W):
    """fs_grid_sample_bwd_input: gout (B,C,h,w) -> dx (B,C,H,W), every tap inside the image adds gout * weight to its pixel.
    Returns (dx, mag, count) with count (B,H,W) the number of taps that land on each pixel."""
    B, C = gout.shape[:2]
    t = grid_taps(grid, H, W)
    dx = torch.zeros(B, C, H * W, dtype=gout.dtype)
    mag = torch.zeros(B, C, H * W, dtype=gout.dtype)
    cnt = torch.zeros(B, H * W, dtype=gout.dtype)
    for dy, dxx, ok, wgt in _corners(t):
        yy = (t["y0"] + dy).clamp(0, H - 1)
        xx = (t["x0"] + dxx).clamp(0, W - 1)
        lin = (yy * W + xx).reshape(B, 1, -1).expand(B, C, -1)
        okf = ok.to(gout.dtype)
        val = (gout * (wgt * okf)[:, None]).reshape(B, C, -1)
        dx.scatter_add_(2, lin, val)
        mag.scatter_add_(2, lin, val.abs())
        cnt.scatter_add_(1, lin[:, 0], okf.reshape(B, -1))
    return dx.reshape(B, C, H, W), mag.reshape(B, C, H, W), cnt.reshape(B, H, W)


# ------------------------------------------------------------------------------------------------
# segmentation loss: focal (pt detached) + multiclass Dice + the four accuracies
# ------------------------------------------------------------------------------------------------
def _log_softmax(pred):
    mx = pred.max(dim=1, keepdim=True).values
    z = pred - mx
    return z - torch.log(torch.exp(z).sum(dim=1, keepdim=True))


def first_argmax(pred):
    """(B,K,HW) -> (B,HW): the first class that attains the maximum"""
    K = pred.shape[1]
    mx = pred.max(dim=1, keepdim=True).values
    k = torch.arange(K)[None, :, None].expand_as(pred)
    return torch.where(pred == mx, k, torch.full_like(k, K)).min(dim=1).values


def seg_counters(pred, gt):
    """the six counters per image (B,6): cls_fg, bin_fg, union_fg, cls_bg, bin_bg, union_bg; background = class K - 1"""
    bg = pred.shape[1] - 1
    am = first_argmax(pred)
    vg, vp, bgg, bgp, eq = gt < bg, am < bg, gt == bg, am == bg, am == gt
    return torch.stack(((vg & eq).sum(1), (vg & (vg == vp)).sum(1), (vg | vp).sum(1),
                        (bgg & eq).sum(1), (bgg & (bgg == bgp)).sum(1), (bgg | bgp).sum(1)), dim=1)


def seg_loss_fwd(pred, gt, gamma, eps):
    """fs_seg_loss_fwd: pred (B,K,HW) logits, gt (B,HW) int64 in [0, K).
    focal = mean(-(1 - pt)^gamma log pt), pt = softmax probability of the true class (a constant in the backward);
    dice  = (1/K) sum over the classes present in gt of 1 - 2 I_k / max(P_k + N_k, eps), with I_k = sum p_k [gt = k],
            P_k = sum p_k, N_k = #[gt = k] over the whole batch;
    acc   = the batch means of cls_fg / (union_fg + 1e-10), bin_fg / (union_fg + 1e-10) and the two fg / bg averages.
    Returns (out (7) = [dice + focal, focal, dice, acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg], coef (2K) = [A_k | B_k] with
    A_k = 2 I_k / den^2 / K (card > eps), B_k = -2 / den / K, both 0 for absent classes, parts)."""
    B, K, HW = pred.shape
    dt = pred.dtype
    logp = _log_softmax(pred)
    p = torch.exp(logp)
    onehot = (gt[:, None, :] == torch.arange(K)[None, :, None]).to(dt)
    logpt = (logp * onehot).sum(1)
    pt = torch.exp(logpt)
    focal = (-(1.0 - pt) ** gamma * logpt).sum() / (B * HW)
    P, I, N = p.sum((0, 2)), (p * onehot).sum((0, 2)), onehot.sum((0, 2))
    card = P + N
    den = card.clamp_min(eps)
    present = N > 0
    zero = torch.zeros_like(P)
    dice = torch.where(present, 1.0 - 2.0 * I / den, zero).sum() / K
    A = torch.where(present & (card > eps), 2.0 * I / (den * den) / K, zero)
    Bc = torch.where(present, -2.0 / den / K, zero)
    c = seg_counters(pred, gt).to(dt)
    ufg, ubg = c[:, 2] + 1e-10, c[:, 5] + 1e-10
    cls_fg, bin_fg, cls_bg, bin_bg = c[:, 0] / ufg, c[:, 1] / ufg, c[:, 3] / ubg, c[:, 4] / ubg
    acc = torch.stack((cls_fg.sum(), bin_fg.sum(), (cls_fg * 0.5 + cls_bg * 0.5).sum(), (bin_fg * 0.5 + bin_bg * 0.5).sum())) / B
    out = torch.cat((torch.stack((dice + focal, focal, dice)), acc))
    return out, torch.cat((A, Bc)), dict(p=p, logp=logp, pt=pt, logpt=logpt, P=P, I=I, N=N, den=den, card=card, present=present)


def seg_loss_bwd(pred, gt, coef, gout, gamma):
    """fs_seg_loss_bwd: dpred (B,K,HW) = gout (p_k (q_k - sum_j p_j q_j) - fw ([k = t] - p_k)), q_k = A_k + [k = t] B_k,
    fw = (1 - pt)^gamma / (B HW).  Returns (dpred, parts)."""
    B, K, HW = pred.shape
    dt = pred.dtype
    logp = _log_softmax(pred)
    p = torch.exp(logp)
    onehot = (gt[:, None, :] == torch.arange(K)[None, :, None]).to(dt)
    q = coef[:K][None, :, None] + onehot * coef[K:][None, :, None]
    dot = (p * q).sum(1, keepdim=True)
    pt = (p * onehot).sum(1, keepdim=True)
    fw = (1.0 - pt) ** gamma / (B * HW)
    dd = p * (q - dot)
    df = -fw * (onehot - p)
    return gout * (dd + df), dict(p=p, logp=logp, q=q, dot=dot, pt=pt, fw=fw, dd=dd, df=df, onehot=onehot,
                                  absdot=(p * q.abs()).sum(1, keepdim=True))
