"""The foveation front-end kernels (csrc/frontend.hip) and the segmentation loss (csrc/head_loss.hip) at the C ABI against the plain
fp64 references of oracle/frontend_ref.py (which tests/test_frontend_ref.py holds to torch on the CPU).

Rules of every case (as in tests/test_elementwise_kernels.py)
  * every output and every scratch buffer is an `Out` of exactly the documented size: guards of sentinel on both sides, the body
    pre-filled with NaN (a marker for integer buffers); after the call the guards are intact and no fill value is left where an
    output is due;
  * inputs are fp64 reference values rounded to fp32;
  * two kinds of data: "int" -- small integers and powers of two, every sum below 2^24, BIT-EQUAL to the reference; "float" --
    random data held to L * 2^-24 * sum|terms| with L counted from the kernel's code beside each check.  Kernels with expf / logf /
    powf / sqrtf (softmax, segmentation loss, gaze map) may instead stay within 4x the error of the same formula in fp32 on the
    CPU (`check(..., ref32=...)`).  The Gaussian-grid kernels accumulate in double: derived bound only.  No bound is taken from
    what a kernel returns;
  * no element is left out of a comparison, except under the knife-edge rule of the Gaussian grid (stated at its test);
  * a rejected call returns FS_ERR_ARG and leaves its outputs untouched.

Interpolation weights.  The bilinear kernels form their source position s in fp32 (a quotient, a product, a subtraction: three
roundings at magnitude s + 1), so a weight may differ from the fp64 one by 3 u (s + 1), and where s sits on an integer the taps one
further out take part with that weight.  `lerp_err` is that perturbation as a matrix; it enters every bound of the bilinear kernels
next to the rounding term L u sum|terms|.  The grid_sample kernels form ix = (gx + 1) W/2 - 0.5 with two roundings: 2 u (|ix| + 1).

Every check prints `[bound] family what ratio`: the largest error as a fraction of its bound (profiles/r17/README.md).
"""
import inspect
import re
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fovealseg  # noqa: E402
import fovealseg_oracle as O  # noqa: E402
import frontend_ref as R  # noqa: E402
from kernel_testing import U, Out, check, dev, exact, f32, randint, randn  # noqa: E402

hip = fovealseg.hip
DEV = "cuda"
F64 = torch.float64
TINY = 2.0 ** -126          # a result below the smallest normal fp32 may be flushed to zero

ENTRY_POINTS = ["fs_gaze_lowres_fwd", "fs_compress_fwd", "fs_compress_bwd", "fs_compress_softmax_fwd", "fs_compress_softmax_bwd",
                "fs_area_pool_fwd", "fs_edge_loss_fwd", "fs_edge_loss_bwd", "fs_gauss_grid_fwd", "fs_gauss_grid_bwd",
                "fs_gauss_grid_fwd_mode", "fs_gauss_grid_bwd_mode", "fs_grid_upsample_fwd", "fs_grid_upsample_bwd", "fs_grid_sample_fwd",
                "fs_grid_sample_label", "fs_grid_sample_bwd_grid", "fs_grid_sample_bwd_input", "fs_seg_loss_fwd", "fs_seg_loss_bwd"]


def test_cases_reach_every_entry_point():
    """host only: every entry point of the family is launched through hip.call somewhere in this file"""
    src = inspect.getsource(sys.modules[__name__])
    called = set(re.findall(r'hip\.call\(\s*"(fs_\w+)"', src))
    assert set(ENTRY_POINTS) <= called, sorted(set(ENTRY_POINTS) - called)


def rand(gen, *shape):
    return f32(torch.rand(*shape, generator=gen, dtype=F64))


def rejected(outs, name, *args):
    with pytest.raises(hip.HipLibraryError, match="rejected"):
        hip.call(name, *args)
    for o in outs:
        assert o.untouched(), name


def offset4(t):
    """a device copy of t (fp32) that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()]
    v.copy_(t.reshape(-1).float())
    assert v.data_ptr() % 16 == 4
    return v


def lerp_err(n_in, n_out, identity=False):
    """|dW| (n_out, n_in) of the header: 3 u (s + 1) on every source within 2 of the position s"""
    if identity and n_in == n_out:
        return torch.zeros(n_out, n_in, dtype=F64)
    s = R.lerp_table(n_in, n_out, F64, identity)[4]
    near = (torch.arange(n_in, dtype=F64)[None, :] - s[:, None]).abs() < 2
    return near.double() * (3 * U * (s + 1))[:, None]


# ================================================================================================
# K1: gaze map + low-resolution RGB
# ================================================================================================
GAZE_CASES = [(1, 4, 4, 2, 2, "00"), (3, 16, 16, 16, 16, "all"), (2, 37, 53, 7, 5, "corners"), (2, 9, 11, 20, 24, "inside"),
              (1, 640, 64, 80, 8, "11"), (2, 32, 32, 13, 11, "00+inside")]


@pytest.mark.parametrize("B,H,W,hs,ws,foc", GAZE_CASES)
def test_gaze_lowres(B, H, W, hs, ws, foc):
    fam = "gaze_lowres"
    gen = torch.Generator().manual_seed(H * W + hs)
    x = randn(gen, B, 3, H, W)
    focus = rand(gen, B, 2)
    if foc in ("00", "all", "corners", "00+inside"):
        focus[0] = 0.0
    if foc in ("11", "all", "corners"):
        focus[-1] = 1.0
    out_o = Out(B * hs * ws * 5)
    xd, fd = dev(x), dev(focus)
    hip.call("fs_gaze_lowres_fwd", hip.ptr(xd), hip.ptr(fd), out_o.ptr, B, H, W, hs, ws)
    got = out_o.get().reshape(B, hs, ws, 5)
    ref, mag = R.gaze_lowres(x, focus, hs, ws)
    ref32, _ = R.gaze_lowres(x.float(), focus.float(), hs, ws)
    # RGB: l0 = 1 - l1 twice, then ly0 (lx0 v00 + lx1 v01) + ly1 (...): two products and an addition inside, a product and an
    # addition outside: 8 roundings on the lerp of |x|; the weights themselves: lerp_err
    Wy, Wx = R.lerp_matrix(H, hs, F64), R.lerp_matrix(W, ws, F64)
    Ey, Ex = lerp_err(H, hs), lerp_err(W, ws)
    ax = x.abs()
    werr = (Ey @ ax @ Wx.T + Wy @ ax @ Ex.T + Ey @ ax @ Ex.T).permute(0, 2, 3, 1)
    check(fam, "rgb", got[..., :3], ref[..., :3], 8 * U * mag + werr)
    # gaze: h = focus (hs - 1) and dy = oy - h round once each: |d dy| <= u (|h| + |dy|), so d2 = dy^2 + dx^2 carries
    # 2 |dy| u (|h| + |dy|) + 2 |dx| u (|w| + |dx|) + 3 u d2; sqrtf, the rounded diagonal, the quotient and the square: 7 u d2
    hh, ww = (focus[:, 0] * (hs - 1))[:, None, None], (focus[:, 1] * (ws - 1))[:, None, None]
    dy = (torch.arange(hs, dtype=F64)[None, :, None] - hh).abs()
    dx = (torch.arange(ws, dtype=F64)[None, None, :] - ww).abs()
    d2 = dy * dy + dx * dx
    e_d2 = 2 * dy * U * (hh.abs() + dy) + 2 * dx * U * (ww.abs() + dx) + 3 * U * d2
    gb = (e_d2 + 7 * U * d2) / (hs * hs + ws * ws)
    check(fam, "gaze", got[..., 3], ref[..., 3], gb, ref32[..., 3])
    exact(fam, "gaze.ch4", got[..., 4], got[..., 3])


# ================================================================================================
# K3: compress, compress + softmax
# ================================================================================================
def compress_inputs(gen, B, HW, C, integer):
    if integer:          # |s w| <= 4, 32 channels; |g relu(s)| <= 8, 7 500 pixels: every sum below 2^24
        s, w, bias = randint(gen, -2, 2, B, HW, C), randint(gen, -2, 2, C), randint(gen, -3, 3, 1)
        g = randint(gen, -4, 4, B, HW)
    else:
        s, w, bias, g = randn(gen, B, HW, C), f32(randn(gen, C) / C ** 0.5), randn(gen, 1), randn(gen, B, HW)
        s = torch.where(torch.rand(B, HW, C, generator=gen) < 0.1, torch.zeros_like(s), s)
    s.reshape(-1)[::7] = -0.0          # exact zeros of both signs: relu'(0) = 0
    s.reshape(-1)[0] = 0.0
    return s, w, bias, g


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 63, 1025, 2500])
@pytest.mark.parametrize("C", [1, 3, 4, 24, 32])
def test_compress(C, HW, B, kind):
    fam = "compress"
    gen = torch.Generator().manual_seed(C * 10000 + HW + B)
    integer = kind == "int"
    s, w, bias, g = compress_inputs(gen, B, HW, C, integer)
    sd, wd, bd, gd = dev(s), dev(w), dev(bias), dev(g)
    out_o = Out(B * HW)
    hip.call("fs_compress_fwd", hip.ptr(sd), hip.ptr(wd), hip.ptr(bd), out_o.ptr, B, HW, C)
    ds_o, dw_o, db_o, scr = Out(B * HW * C), Out(C), Out(1), Out(B * (C + 1))
    hip.call("fs_compress_bwd", hip.ptr(gd), hip.ptr(sd), hip.ptr(wd), ds_o.ptr, dw_o.ptr, db_o.ptr, B, HW, C, scr.ptr)
    scr.get()
    ref, mag = R.compress_fwd(s, w, bias)
    ds_r, dw_r, db_r, mdw, mdb = R.compress_bwd(g, s, w)
    exact(fam, "ds", ds_o.get().reshape(B, HW, C), ds_r.float())          # one correctly rounded product, or 0
    if integer:
        exact(fam, "fwd.int", out_o.get().double().reshape(B, HW), ref)
        exact(fam, "dw.int", dw_o.get().double(), dw_r)
        exact(fam, "db.int", db_o.get().double(), db_r)
    else:
        # C products, C additions in sequence (the first onto 0), the bias
        check(fam, "fwd", out_o.get().reshape(B, HW), ref, (C + 2) * U * mag)
        # per thread ceil(HW / 1024) pixels in sequence, six shuffle stages, 16 waves, B image records, one product each
        L = -(-HW // 1024) + 6 + 16 + B + 1
        check(fam, "dw", dw_o.get(), dw_r, L * U * mdw)
        check(fam, "db", db_o.get(), db_r, L * U * mdb)


def softmax_bound(xs, logit, mag, C, HW):
    """logit: (C + 2) u mag (test_compress).  The exponent l - m carries both logits' errors and its own rounding: d = el + el_max +
    u |l - m|; expf 3 u; the sum of the e (per thread ceil(HW / 1024), six shuffle stages, 16 waves) inherits the xs-weighted mean
    of the d's; the quotient 1 u.  Results below 2^-126 may be flushed."""
    el = (C + 2) * U * mag
    m, am = logit.max(dim=1, keepdim=True)
    d = el + el.gather(1, am) + U * (logit - m).abs()
    Ls = -(-HW // 1024) + 6 + 16
    rel = d + (xs * d).sum(1, keepdim=True) + (3 + 3 + Ls + 1) * U
    return xs * rel + TINY


CSF_HW = [1, 2, 1023, 1025, 6400, 16384]          # 16384: the largest map fs_compress_softmax_fwd accepts (include/fovealseg.h)


@pytest.mark.parametrize("HW", CSF_HW)
@pytest.mark.parametrize("C", [1, 4, 24, 32])
def test_compress_softmax_fwd(C, HW):
    fam = "compress_softmax"
    gen = torch.Generator().manual_seed(C * 100000 + HW)
    B = 2
    s, w, bias, _ = compress_inputs(gen, B, HW, C, False)
    xs_o = Out(B * HW)
    sd, wd, bd = dev(s), dev(w), dev(bias)
    hip.call("fs_compress_softmax_fwd", hip.ptr(sd), hip.ptr(wd), hip.ptr(bd), xs_o.ptr, B, HW, C)
    got = xs_o.get().reshape(B, HW)
    xs, logit, mag = R.compress_softmax_fwd(s, w, bias)
    bound = softmax_bound(xs, logit, mag, C, HW)
    check(fam, f"fwd.C{C}.HW{HW}", got, xs, bound, R.compress_softmax_fwd(s.float(), w.float(), bias.float())[0])
    assert bool(((got.double().sum(1) - 1).abs() <= bound.sum(1) + 1e-12).all())


def underflowing_softmax(gen, B=2, HW=1025, C=4):
    """inputs whose logits spread over more than 104, so that the tail of the fp32 softmax is exactly zero"""
    s, w, bias, _ = compress_inputs(gen, B, HW, C, False)
    w = f32(w * 60)
    return s, w, bias


def test_compress_softmax_fwd_underflow():
    fam = "compress_softmax"
    gen = torch.Generator().manual_seed(7)
    B, HW, C = 2, 1025, 4
    s, w, bias = underflowing_softmax(gen, B, HW, C)
    xs, logit, mag = R.compress_softmax_fwd(s, w, bias)
    assert float((logit.max(1).values - logit.min(1).values).min()) > 104 and bool((xs < 2.0 ** -160).any())
    xs_o = Out(B * HW)
    sd, wd, bd = dev(s), dev(w), dev(bias)
    hip.call("fs_compress_softmax_fwd", hip.ptr(sd), hip.ptr(wd), hip.ptr(bd), xs_o.ptr, B, HW, C)
    got = xs_o.get().reshape(B, HW)
    bound = softmax_bound(xs, logit, mag, C, HW)
    check(fam, "fwd.underflow", got, xs, bound, R.compress_softmax_fwd(s.float(), w.float(), bias.float())[0])
    assert bool((got[xs < 2.0 ** -160] == 0).all()) and int((got == 0).sum()) > 0
    assert bool(((got.double().sum(1) - 1).abs() <= bound.sum(1) + 1e-12).all())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 5, 8, 9, 1023, 6400])
@pytest.mark.parametrize("C", [4, 8, 12, 16, 24, 32])
def test_compress_softmax_bwd(C, HW, B):
    fam = "compress_softmax"
    gen = torch.Generator().manual_seed(C * 100000 + HW * 10 + B)
    s, w, bias, g = compress_inputs(gen, B, HW, C, False)
    xs = f32(R.compress_softmax_fwd(s, w, bias)[0])
    nscr = hip.query("fs_compress_softmax_bwd_scratch_floats", B, C)
    assert nscr == B * 8 * (C + 1)
    ds_o, dw_o, db_o, scr = Out(B * HW * C), Out(C), Out(1), Out(nscr)
    gd, xd, sd, wd = dev(g), dev(xs), dev(s), dev(w)
    hip.call("fs_compress_softmax_bwd", hip.ptr(gd), hip.ptr(xd), hip.ptr(sd), hip.ptr(wd), ds_o.ptr, dw_o.ptr, db_o.ptr, B, HW, C, scr.ptr)
    scr.get()          # slices without pixels (HW < 8) still leave their records
    ds_r, dw_r, db_r, dl, dot = R.compress_softmax_bwd(g, xs, s, w)
    # dot: per thread ceil(HW / 768) products in sequence, six shuffle stages, 12 waves
    Ld = -(-HW // 768) + 6 + 12 + 1
    e_dot = Ld * U * (g * xs).abs().sum(1, keepdim=True)
    # dlogit = xs (g - dot): the difference rounds at |g| + |dot|, the product once
    e_dl = xs * (e_dot + U * (g.abs() + dot.abs())) + U * dl.abs()
    relu = s.clamp_min(0.0)
    check(fam, f"bwd.ds.C{C}.HW{HW}.B{B}", ds_o.get().reshape(B, HW, C), ds_r, (e_dl + U * dl.abs())[..., None] * w.abs())
    # dw: a thread keeps its channel quad over ceil(per Q / 768) pixels of its slice, then the 768 / Q threads of the quad in
    # sequence, then the 8 B records; db: the same walk, a block sum (6 + 12) instead of the thread list
    per, Q = -(-HW // 8), C // 4
    Lw = -(-per * Q // 768) + 768 // Q + 8 * B + 1
    Lb = -(-per * Q // 768) + 6 + 12 + 8 * B
    check(fam, f"bwd.dw.C{C}.HW{HW}.B{B}", dw_o.get(), dw_r,
          ((e_dl + Lw * U * dl.abs())[..., None] * relu).reshape(-1, C).sum(0))
    check(fam, f"bwd.db.C{C}.HW{HW}.B{B}", db_o.get(), db_r, (e_dl + Lb * U * dl.abs()).sum().reshape(1))


def test_compress_rejects():
    z = torch.zeros(4 * 16400 * 36 // 4, device=DEV)
    p = hip.ptr(z)
    for C in (6, 20, 28, 36):          # no multiple of 4, no divisor of 768 / 4 quads, more than 32
        o = [Out(8 * C), Out(C), Out(1), Out(8 * (C + 1))]
        rejected(o, "fs_compress_softmax_bwd", p, p, p, p, o[0].ptr, o[1].ptr, o[2].ptr, 1, 8, C, o[3].ptr)
    C = 8
    zo = offset4(torch.zeros(8 * C + 8))
    for which in ("s", "ds", "w"):          # the float4 walk needs 16-byte pointers
        o = [Out(8 * C + 4), Out(C), Out(1), Out(8 * (C + 1))]
        sp = hip.ptr(zo) if which == "s" else p
        wp = hip.ptr(zo) if which == "w" else p
        dsp = o[0].ptr + 4 if which == "ds" else o[0].ptr
        rejected(o, "fs_compress_softmax_bwd", p, p, sp, wp, dsp, o[1].ptr, o[2].ptr, 1, 8, C, o[3].ptr)
    o = [Out(8), Out(8 * 33), Out(33), Out(1), Out(34)]
    rejected(o, "fs_compress_fwd", p, p, p, o[0].ptr, 1, 8, 33)
    rejected(o, "fs_compress_bwd", p, p, p, o[1].ptr, o[2].ptr, o[3].ptr, 1, 8, 33, o[4].ptr)
    rejected(o, "fs_compress_softmax_fwd", p, p, p, o[0].ptr, 1, 8, 33)
    o = [Out(CSF_HW[-1] + 1)]
    rejected(o, "fs_compress_softmax_fwd", p, p, p, o[0].ptr, 1, CSF_HW[-1] + 1, 4)


# ================================================================================================
# K11: area pool, edge loss
# ================================================================================================
AREA_CASES = [(1, 2, 2, 2, 2), (2, 7, 9, 3, 4), (1, 13, 16, 5, 4), (2, 40, 64, 3, 8), (1, 333, 517, 80, 80), (1, 4, 1100, 2, 300),
              (1, 2, 16384, 1, 2)]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("B,H,W,hs,ws", AREA_CASES)
def test_area_pool(B, H, W, hs, ws, kind):
    fam = "area_pool"
    gen = torch.Generator().manual_seed(H + W)
    y = randint(gen, 0, 1, B, H, W) if kind == "int" else randn(gen, B, H, W)
    out_o = Out(B * hs * ws)
    yd = dev(y)
    hip.call("fs_area_pool_fwd", hip.ptr(yd), out_o.ptr, B, H, W, hs, ws)
    got = out_o.get().reshape(B, hs, ws)
    ref, mag = R.area_pool(y, hs, ws)
    if kind == "int":          # a 0/1 mask: the window sum is an integer below 2^24, the one division is correctly rounded
        exact(fam, f"{H}x{W}.int", got, ref.float())
    else:                      # the rows of a column in sequence, then the columns of the window in sequence, the division
        Lr = max(b - a for a, b in R.area_windows(H, hs))
        Lc = max(b - a for a, b in R.area_windows(W, ws))
        check(fam, f"{H}x{W}", got, ref, (Lr + Lc + 1) * U * mag)
    if (H, W) == (40, 64):          # the plane 4 bytes off a 16-byte boundary: the scalar loop, the same row order, bit-identical
        assert B * H * W % 4 == 0
        out2 = Out(B * hs * ws)
        ym = offset4(y)
        hip.call("fs_area_pool_fwd", hip.ptr(ym), out2.ptr, B, H, W, hs, ws)
        exact(fam, f"{H}x{W}.misaligned.{kind}", out2.get().reshape(B, hs, ws), got)


def test_area_pool_rejects():
    z = torch.zeros(64, device=DEV)
    o = [Out(16)]
    rejected(o, "fs_area_pool_fwd", hip.ptr(z), o[0].ptr, 1, 3, 8, 4, 4)          # H < hs


def tie_positions(n, k):
    """k positions for the minimum and k for the maximum, spread evenly over [0, n): both reach index 0 .. and the last elements (the
    scalar tail behind the float4 body), and for n > 4096 they fall into different workgroups"""
    lo = sorted(set(int(round(i * (n - 1) / max(k - 1, 1))) for i in range(k)))
    taken = set(lo)
    rest = [i for i in range(n) if i not in taken]
    hi = sorted(set(rest[int(round(i * (len(rest) - 1) / max(k - 1, 1)))] for i in range(k)))
    return lo, hi


def edge_bounds(xs, t, coef, gout):
    """u = (x - min) / r: the difference, r and the quotient round once each: 3 u |u|, likewise v; d = u - v adds u |d|.
    forward: d^2 carries 2 |d| e_d + u d^2, the sum runs in double, the mean, its cast and the product with coef: 3 u |loss|.
    backward: k = 2 coef gout / n (3 roundings) and g = k d: e_g = |k| e_d + 4 u |g|; dxs = g / r: e_g / r + 2 u |g / r|;
    the two border sums add fp32 products g (u - 1), g u in double: per term e_g |u - 1| + |g| (3 u |u| + u) + u |g (u - 1)|;
    the shares dmin / dmax: a cast, the rounded r and two quotients (4 u); the final additions 2 u |dxs|."""
    n = xs.numel()
    mn, mx, tmn, tmx = xs.min(), xs.max(), t.min(), t.max()
    r = mx - mn
    u, v = (xs - mn) / r, (t - tmn) / (tmx - tmn)
    d = u - v
    e_d = 3 * U * (u.abs() + v.abs()) + U * d.abs()
    loss = coef * (d * d).sum() / n
    b_loss = coef * (2 * d.abs() * e_d + U * d * d).sum() / n + 3 * U * loss.abs()
    k = 2.0 * coef * gout / n
    g = k * d
    e_g = abs(k) * e_d + 4 * U * g.abs()
    e_main = e_g / r + 2 * U * g.abs() / r
    is_mn, is_mx = xs == mn, xs == mx
    t1 = (e_g * (u - 1).abs() + g.abs() * (3 * U * u.abs() + U) + U * (g * (u - 1)).abs()).sum()
    t2 = (e_g * u.abs() + g.abs() * 3 * U * u.abs() + U * (g * u).abs()).sum()
    dmn = (g * (u - 1)).sum() / r / is_mn.sum()
    dmx = -(g * u).sum() / r / is_mx.sum()
    e_dmn = t1 / r / is_mn.sum() + 4 * U * dmn.abs()
    e_dmx = t2 / r / is_mx.sum() + 4 * U * dmx.abs()
    dxs = g / r + is_mn.double() * dmn + is_mx.double() * dmx
    return b_loss, e_main + is_mn.double() * e_dmn + is_mx.double() * e_dmx + 2 * U * dxs.abs()


def run_edge(fam, what, xs, t, coef, gout, misaligned=False):
    n = xs.numel()
    nst = hip.query("fs_edge_loss_stats_floats", n)
    loss_o, st_o, dxs_o = Out(1), Out(nst), Out(n + 4)
    assert st_o.ptr % 32 == 0
    xd, td = (offset4(xs), offset4(t)) if misaligned else (dev(xs), dev(t))
    god = dev(torch.tensor([gout], dtype=F64))
    dptr = dxs_o.ptr + (4 if misaligned else 0)
    hip.call("fs_edge_loss_fwd", hip.ptr(xd), hip.ptr(td), n, coef, loss_o.ptr, st_o.ptr)
    hip.call("fs_edge_loss_bwd", hip.ptr(xd), hip.ptr(td), n, coef, hip.ptr(god), st_o.ptr, dptr)
    st = st_o.get(complete=False)
    left = torch.isnan(st).nonzero().reshape(-1).tolist()
    assert left == [6, 7], left          # the two pad floats behind the six statistics are nobody's output
    body = dxs_o.get(complete=False)
    lo = 1 if misaligned else 0
    got = body[lo:lo + n]
    assert not bool(torch.isnan(got).any()) and bool(torch.isnan(torch.cat((body[:lo], body[lo + n:]))).all())
    loss_r, st_r = R.edge_loss_fwd(xs, t, coef)
    exact(fam, what + ".stats", st[:6].double(), st_r)
    b_loss, b_dxs = edge_bounds(xs, t, coef, gout)
    check(fam, what + ".loss", loss_o.get(), loss_r.reshape(1), b_loss.reshape(1))
    check(fam, what + ".dxs", got, R.edge_loss_bwd(xs, t, coef, gout), b_dxs)


EDGE_CASES = [(2, 1), (7, 1), (7, 3), (4099, 1), (4099, 3), (4099, 64), (4100, 1), (4100, 3), (4100, 64), (19203, 1), (19203, 3), (19203, 64)]


@pytest.mark.parametrize("n,ties", EDGE_CASES)
def test_edge_loss(n, ties):
    gen = torch.Generator().manual_seed(n + ties)
    xs = f32(rand(gen, n) * 0.5 + 0.25)
    t = rand(gen, n)
    lo, hi = tie_positions(n, min(ties, n // 2))
    xs[lo] = 0.125
    xs[hi] = 0.875
    if n % 4 and ties >= 3:
        assert lo[-1] >= n - n % 4 and hi[-1] >= n - n % 4          # tied elements in the scalar tail behind the float4 body
    run_edge("edge_loss", f"n{n}.ties{ties}", xs, t, 5.0, 0.37)


def test_edge_loss_tail_ties():
    """all three minima in the scalar tail of the last workgroup's stride, the three maxima in the float4 bodies of three workgroups"""
    n = 19203
    gen = torch.Generator().manual_seed(3)
    xs, t = f32(rand(gen, n) * 0.5 + 0.25), rand(gen, n)
    xs[[n - 3, n - 2, n - 1]] = 0.125
    xs[[0, 4 * 256, 4 * 512 + 5]] = 0.875
    run_edge("edge_loss", "tail_ties", xs, t, 5.0, 0.37)


def test_edge_loss_underflowing_softmax_and_offset():
    gen = torch.Generator().manual_seed(7)
    s, w, bias = underflowing_softmax(gen)
    xs = R.compress_softmax_fwd(s.float(), w.float(), bias.float())[0].double().reshape(-1)          # what the fp32 kernel hands on
    assert int((xs == 0).sum()) > 64
    t = rand(gen, xs.numel())
    run_edge("edge_loss", "softmax_tail", xs, t, 5.0, 0.37)
    n = 4100
    xs2, t2 = f32(rand(gen, n) * 0.5 + 0.25), rand(gen, n)
    lo, hi = tie_positions(n, 3)
    xs2[lo] = 0.125
    xs2[hi] = 0.875
    run_edge("edge_loss", "offset4", xs2, t2, 5.0, 0.37, misaligned=True)


# ================================================================================================
# K4: Gaussian grid
# ================================================================================================
GAUSS_SHAPES = [(2, 2, 1), (3, 5, 2), (9, 7, 3), (9, 7, 6), (50, 37, 30), (46, 46, 45), (17, 130, 20), (130, 17, 20), (40, 3, 45),
                (80, 80, 45), (80, 80, 127)]
MODES = {"entry": R.PAD_REPLICATION, "replication": R.PAD_REPLICATION, "reflect": R.PAD_REFLECT, "zero": R.PAD_ZERO}
GAUSS_CASES = [(hs, ws, pad, mode, "softmax") for hs, ws, pad in GAUSS_SHAPES for mode in MODES
               if mode != "reflect" or pad <= min(hs, ws) - 1] + [(80, 80, 45, "replication", "pixel"), (80, 80, 45, "entry", "pixel")]


def gauss_taps(pad):
    return torch.ones(1, dtype=F64) if pad == 0 else torch.from_numpy(O.gaussian_1d(2 * pad + 1, pad))


def gauss_fwd_call(mode, xd, gd, out, B, hs, ws, pad):
    if mode == "entry":
        hip.call("fs_gauss_grid_fwd", hip.ptr(xd), hip.ptr(gd), out.ptr, B, hs, ws, pad)
    else:
        hip.call("fs_gauss_grid_fwd_mode", hip.ptr(xd), hip.ptr(gd), out.ptr, B, hs, ws, pad, MODES[mode])


def gauss_bwd_call(mode, xd, gd, dd, out, B, hs, ws, pad, scr):
    if mode == "entry":
        hip.call("fs_gauss_grid_bwd", hip.ptr(xd), hip.ptr(gd), hip.ptr(dd), out.ptr, B, hs, ws, pad, scr.ptr)
    else:
        hip.call("fs_gauss_grid_bwd_mode", hip.ptr(xd), hip.ptr(gd), hip.ptr(dd), out.ptr, B, hs, ws, pad, MODES[mode], scr.ptr)


@pytest.mark.parametrize("hs,ws,pad,mode,sal", GAUSS_CASES)
def test_gauss_grid(hs, ws, pad, mode, sal):
    """Knife-edge rule: a grid component is left out of the BACKWARD comparison (its cotangent zeroed) only where the fp64 unclamped
    value satisfies | |u| - 1 | <= 1e-4; clearly clamped components keep a non-zero cotangent and must contribute nothing.  The share
    left out is capped on the reference before the device is touched: 0.1 % for replication / zero padding on random softmax
    saliency, 10 % for the uniform map with one bright pixel, exactly the border components under reflect (which sit on the bound
    by symmetry).  The forward compares every component."""
    fam = "gauss_grid"
    what = f"{hs}x{ws}.pad{pad}.{mode}.{sal}"
    gen = torch.Generator().manual_seed(hs * 1000 + ws * 10 + pad)
    B, n = 2, hs * ws
    if sal == "softmax":
        xs = f32(torch.softmax(2 * torch.randn(B, n, generator=gen, dtype=F64), 1)).reshape(B, hs, ws)
    else:          # the realistic background: a flat map and one bright pixel
        xs = torch.full((B, hs, ws), 0.5 / n, dtype=F64)
        xs[0, 20, 50] += 0.5
        xs[1, 70, 3] += 0.5
        xs = f32(xs)
    g1d = gauss_taps(pad)
    m = MODES[mode]
    u, grid_r, fp = R.gauss_grid_fwd(xs, g1d, pad, m)
    knife = ((u.abs() - 1).abs() <= 1e-4)
    share = float(knife.double().mean())
    clamped = float((u.abs() > 1 + 1e-4).double().mean())
    print(f"[knife] {fam} {what} share {share:.6f} clearly-clamped {clamped:.4f}")
    if mode == "reflect":
        border = torch.zeros_like(knife)
        border[:, :, 0, 0] = border[:, :, ws - 1, 0] = True
        border[:, 0, :, 1] = border[:, hs - 1, :, 1] = True
        assert torch.equal(knife, border)
    else:
        assert share <= (0.10 if sal == "pixel" else 0.001), share
    cot = randn(gen, B, hs, ws, 2)
    cot = torch.where(knife, torch.zeros_like(cot), cot)

    xd, gd, cd = dev(xs), dev(g1d, F64), dev(cot)
    grid_o = Out(B * n * 2)
    gauss_fwd_call(mode, xd, gd, grid_o, B, hs, ws, pad)
    # forward.  The row pass rounds R0 = sum g x~ and R1 = sum g x~ c to fp32 (u each on sums accumulated in double); the column pass
    # and the quotient run in double: p carries u p, ax u absax, ay u absay, and u = 2 a / p - 1 moves by 2 u (absa + |a|) / p; the
    # store rounds once more at |grid| <= 1
    p, ax, ay = fp["p"], fp["ax"], fp["ay"]
    b_fwd = torch.stack((2 * U * (fp["absax"] + ax.abs()) / p + U, 2 * U * (fp["absay"] + ay.abs()) / p + U), -1)
    if pad <= 3 * (min(hs, ws) - 1):          # |c| <= 1 + pad / (side - 1) <= 4: the bound stays below what the existing tests assert
        assert float(b_fwd.max()) <= 3e-6
    check(fam, what + ".fwd", grid_o.get().reshape(B, hs, ws, 2), grid_r, b_fwd)

    nscr = hip.query("fs_gauss_grid_bwd_scratch_floats", B, hs, ws)
    assert nscr == 3 * B * n
    dxs_o, scr = Out(B * n), Out(nscr)
    gauss_bwd_call(mode, xd, gd, cd, dxs_o, B, hs, ws, pad, scr)
    scr.get()
    dxs_r, bp = R.gauss_grid_bwd(xs, g1d, cot, pad, m)
    # backward.  dax = 2 dg / p: u from p, u from the fp32 scratch, and the Bf / Cf round of the second launch: 3 u |dax| (day alike).
    # dp = -(dax ax + day ay) / p: |dax| (u absax + u |ax|) + |day| (u absay + u |ay|) from the inputs, u |dp| each from the divisor,
    # the scratch and Bf.  The transposed filter is linear: the errors pass through it with absolute weights; the store rounds once.
    dp, dax, day = bp["dp"].abs(), bp["dax"].abs(), bp["day"].abs()
    e_dp = dax * U * (fp["absax"] + ax.abs()) + day * U * (fp["absay"] + ay.abs()) + 3 * U * dp
    b_bwd = bp["absmap"](e_dp, 3 * U * dax, 3 * U * day) + U * dxs_r.abs()
    check(fam, what + ".bwd", dxs_o.get().reshape(B, hs, ws), dxs_r, b_bwd)


@pytest.mark.parametrize("hs,ws", [(2, 2), (5, 4)])
def test_gauss_grid_identity(hs, ws):
    """pad 0 with the single tap 1.0: the grid is 2 i / (n - 1) - 1 whatever the saliency"""
    gen = torch.Generator().manual_seed(hs)
    B = 2
    xs = f32(torch.softmax(2 * torch.randn(B, hs * ws, generator=gen, dtype=F64), 1)).reshape(B, hs, ws)
    g1d = gauss_taps(0)
    xd, gd = dev(xs), dev(g1d, F64)
    gx = (2 * torch.arange(ws, dtype=F64) / (ws - 1) - 1)[None, :].expand(hs, ws)
    gy = (2 * torch.arange(hs, dtype=F64) / (hs - 1) - 1)[:, None].expand(hs, ws)
    ref = torch.stack((gx, gy), -1).expand(B, hs, ws, 2)
    for mode in MODES:
        o = Out(B * hs * ws * 2)
        gauss_fwd_call(mode, xd, gd, o, B, hs, ws, 0)
        check("gauss_grid", f"identity.{hs}x{ws}.{mode}", o.get().reshape(B, hs, ws, 2), ref, 5 * U)          # 2 u (c + c) + u, c <= 1


def test_gauss_grid_rejects():
    z = torch.zeros(3 * 8192, device=DEV)
    g = torch.zeros(512, dtype=F64, device=DEV)
    p, gp = hip.ptr(z), hip.ptr(g)
    for B, hs, ws, pad, mode in [(1, 9, 7, 7, R.PAD_REFLECT),          # reflect: pad > ws - 1
                                 (1, 7, 9, 7, R.PAD_REFLECT),          # reflect: pad > hs - 1
                                 (1, 9, 7, 128, R.PAD_REPLICATION),    # 2 pad + 1 > 256
                                 (1, 9, 7, 128, R.PAD_ZERO),
                                 (1, 81, 80, 3, R.PAD_REPLICATION),    # hs ws > 6400
                                 (1, 81, 80, 3, R.PAD_ZERO)]:
        o = [Out(2 * B * hs * ws), Out(B * hs * ws), Out(3 * B * hs * ws)]
        rejected(o[:1], "fs_gauss_grid_fwd_mode", p, gp, o[0].ptr, B, hs, ws, pad, mode)
        rejected(o[1:], "fs_gauss_grid_bwd_mode", p, gp, p, o[1].ptr, B, hs, ws, pad, mode, o[2].ptr)
        if mode == R.PAD_REPLICATION:
            rejected(o[:1], "fs_gauss_grid_fwd", p, gp, o[0].ptr, B, hs, ws, pad)
            rejected(o[1:], "fs_gauss_grid_bwd", p, gp, p, o[1].ptr, B, hs, ws, pad, o[2].ptr)


# ================================================================================================
# grid up-sampling
# ================================================================================================
def upsample_werr(a, h, w, H, W, transpose):
    """the weight perturbation of the header run over |a| in both directions (+ the second-order term)"""
    Wy, Wx = R.lerp_matrix(h, H, F64, True), R.lerp_matrix(w, W, F64, True)
    Ey, Ex = lerp_err(h, H, True), lerp_err(w, W, True)
    ap = a.abs().permute(0, 3, 1, 2)
    if transpose:
        r = Ey.T @ ap @ Wx + Wy.T @ ap @ Ex + Ey.T @ ap @ Ex
    else:
        r = Ey @ ap @ Wx.T + Wy @ ap @ Ex.T + Ey @ ap @ Ex.T
    return r.permute(0, 2, 3, 1)


UP_FWD = [(1, 1, 4, 3), (7, 5, 10, 16), (5, 7, 16, 9), (4, 4, 4, 4), (3, 2, 6, 6), (20, 30, 60, 60), (3, 3, 12, 15)]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("h,w,H,W", UP_FWD)
def test_grid_upsample_fwd(h, w, H, W, kind):
    fam = "grid_upsample"
    gen = torch.Generator().manual_seed(h * w + H)
    B = 3
    integer = kind == "int"
    grid = randint(gen, -8, 8, B, h, w, 2) if integer else f32(rand(gen, B, h, w, 2) * 2 - 1)
    out_o = Out(B * H * W * 2)
    gd = dev(grid)
    hip.call("fs_grid_upsample_fwd", hip.ptr(gd), out_o.ptr, B, h, w, H, W)
    got = out_o.get().reshape(B, H, W, 2)
    ref, mag = R.grid_upsample_fwd(grid, H, W)
    if integer and (H, W) in ((h, w), (2 * h, 2 * w)):          # copies; factor 2: weights 0.25 / 0.75 on small integers, every product exact
        exact(fam, f"fwd.{h}x{w}-{H}x{W}.int", got.double(), ref)
    else:          # the lerp of test_gaze_lowres: 8 roundings, and the weights' own error
        check(fam, f"fwd.{h}x{w}-{H}x{W}.{kind}", got, ref, 8 * U * mag + upsample_werr(grid, h, w, H, W, False))


UP_BWD = [(1, 1, 3, 4), (1, 2, 3, 4), (2, 3, 3, 4), (3, 3, 3, 4), (4, 5, 3, 4), (5, 4, 3, 4), (6, 7, 3, 4), (8, 8, 3, 4), (7, 2, 1, 3),
          (2, 9, 3, 1), (2, 2, 17, 19)]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("fy,fx,h,w", UP_BWD)
def test_grid_upsample_bwd(fy, fx, h, w, kind):
    fam = "grid_upsample"
    gen = torch.Generator().manual_seed(fy * 10 + fx)
    B, H, W = 2, fy * h, fx * w
    integer = kind == "int"
    g = randint(gen, -8, 8, B, H, W, 2) * 16 if integer else randn(gen, B, H, W, 2)
    dg_o = Out(B * h * w * 2)
    gd = dev(g)
    hip.call("fs_grid_upsample_bwd", hip.ptr(gd), dg_o.ptr, B, h, w, H, W)
    got = dg_o.get().reshape(B, h, w, 2)
    ref, mag = R.grid_upsample_bwd(g, h, w)
    if integer and fy in (1, 2) and fx in (1, 2):          # weights in {1, 0.25, 0.75}^2 on multiples of 16: every term and sum exact
        exact(fam, f"bwd.f{fy}x{fx}.int", got.double(), ref)
    else:          # the (2 fy)(2 fx) outputs of the footprint in sequence, each wy wx v (two products), the two weights' 1 - l1
        check(fam, f"bwd.f{fy}x{fx}.h{h}w{w}.{kind}", got, ref, (4 * fy * fx + 4) * U * mag + upsample_werr(g, h, w, H, W, True))


def test_grid_upsample_rejects():
    z = torch.zeros(2 * 7 * 8, device=DEV)
    for h, w, H, W in [(3, 4, 7, 8), (3, 4, 6, 9), (3, 4, 2, 8)]:          # non-integer ratios, and a smaller target
        o = [Out(2 * h * w)]
        rejected(o, "fs_grid_upsample_bwd", hip.ptr(z), o[0].ptr, 1, h, w, H, W)


# ================================================================================================
# K5 / K6: grid_sample
# ================================================================================================
def layout(t, nhwc):
    """reference (B,C,h,w) -> the layout the entry point uses"""
    return t.permute(0, 2, 3, 1).contiguous() if nhwc else t.contiguous()


def unlayout(flat, B, C, h, w, nhwc):
    return flat.reshape(B, h, w, C).permute(0, 3, 1, 2) if nhwc else flat.reshape(B, C, h, w)


def sample_grid(gen, B, h, w, H, W, salt):
    """random points of [-1, 1] whose pixel coordinates keep 0.05 away from the integers (where the gradient with respect to the grid
    jumps), and the edge values: exactly -1 and +1, +-(1 + 1/W) (taps half outside: these DO sit on an integer), +-3 and +-1e6"""
    def coord(n, size):
        k = torch.randint(-1, size, (n,), generator=gen).double()
        i = (k + 0.05 + 0.9 * torch.rand(n, generator=gen, dtype=F64)).clamp(-0.45, size - 0.55)
        return (i + 0.5) * 2 / size - 1
    npt = B * h * w
    g = torch.stack((coord(npt, W), coord(npt, H)), -1)
    spx = [-1.0, 1.0, 1 + 1.0 / W, -(1 + 1.0 / W), 3.0, -3.0, 1e6, -1e6]
    spy = [-1.0, 1.0, 1 + 1.0 / H, -(1 + 1.0 / H), 3.0, -3.0, 1e6, -1e6]
    for i in range(min(npt, 16)):
        j = (i + salt) % 16
        if j < 8:
            g[i, 0] = spx[j]
        else:
            g[i, 1] = spy[j - 8]
    if npt >= 20:          # both coordinates on an edge value
        g[16] = torch.tensor([1.0, -1.0], dtype=F64)
        g[17] = torch.tensor([-(1 + 1.0 / W), 1 + 1.0 / H], dtype=F64)
        g[18] = torch.tensor([3.0, 0.1], dtype=F64)
        g[19] = torch.tensor([-1.0, 1e6], dtype=F64)
    return f32(g).reshape(B, h, w, 2)


def coord_err(t, H, W):
    """|d ix|, |d iy| of the header; beyond the image by two pixels every tap is outside in fp32 and fp64 alike"""
    return 2 * U * (t["ix"].abs().clamp(max=W + 2) + 1), 2 * U * (t["iy"].abs().clamp(max=H + 2) + 1)


def neighbourhood_sum(val, t, H, W):
    """val (B,C,h,w) >= 0 added to every pixel of the 4x4 neighbourhood of its grid point: (B,C,H,W)"""
    B, C = val.shape[:2]
    out = torch.zeros(B, C, H * W, dtype=F64)
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            yy, xx = t["y0"] + dy, t["x0"] + dx
            ok = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).double()
            lin = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, -1).expand(B, C, -1)
            out.scatter_add_(2, lin, (val * ok[:, None]).reshape(B, C, -1))
    return out.reshape(B, C, H, W)


@pytest.mark.parametrize("nhwc", [1, 0])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (16, 17)])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 4), (40, 56)])
def test_grid_sample(H, W, h, w, C, B, nhwc):
    fam = "grid_sample"
    what = f"{H}x{W}.{h}x{w}.C{C}.B{B}.{'nhwc' if nhwc else 'nchw'}"
    salt = H + W + h + C + B
    gen = torch.Generator().manual_seed(salt * 7 + nhwc)
    x = randn(gen, B, C, H, W)
    y = randint(gen, 0, 5, B, H, W)
    grid = sample_grid(gen, B, h, w, H, W, salt)
    go = randn(gen, B, C, h, w)
    assert bool(torch.isfinite(grid).all())
    xd, yd, gd, god = dev(x), dev(y), dev(grid), dev(layout(go, nhwc))
    t = R.grid_taps(grid, H, W)
    ex, ey = coord_err(t, H, W)
    xmax = x.abs().amax((2, 3))[:, :, None, None]          # (B,C,1,1)

    # forward and label: bit-equal to F.grid_sample in fp32 on the CPU (include/fovealseg.h), and within the bound of the fp64 reference
    out_o = Out(B * C * h * w)
    hip.call("fs_grid_sample_fwd", hip.ptr(xd), hip.ptr(gd), out_o.ptr, B, C, H, W, h, w, nhwc)
    got = unlayout(out_o.get(), B, C, h, w, nhwc)
    exact(fam, what + ".fwd.aten", got, F.grid_sample(x.float(), grid.float(), mode="bilinear", padding_mode="zeros", align_corners=False))
    ref, mag = R.grid_sample_fwd(x, grid)
    # the four weights: a difference and a product each (2 u), the four products and three additions: 6 u on sum |w v|; a weight
    # moves by |d ix| + |d iy| on taps of at most max|x|
    check(fam, what + ".fwd", got, ref, 6 * U * mag + (ex + ey)[:, None] * 4 * xmax)
    lab_o, ys_o = Out(B * h * w, torch.int64, fill=-9999), Out(B * h * w)
    hip.call("fs_grid_sample_label", hip.ptr(yd), hip.ptr(gd), lab_o.ptr, ys_o.ptr, B, H, W, h, w)
    ys_t = F.grid_sample(y.float()[:, None], grid.float(), mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
    exact(fam, what + ".ysamp.aten", ys_o.get().reshape(B, h, w), ys_t)
    exact(fam, what + ".label.aten", lab_o.get().reshape(B, h, w), ys_t.long())
    lab2 = Out(B * h * w, torch.int64, fill=-9999)          # ysamp is optional
    hip.call("fs_grid_sample_label", hip.ptr(yd), hip.ptr(gd), lab2.ptr, None, B, H, W, h, w)
    exact(fam, what + ".label.noysamp", lab2.get(), lab_o.get())

    # gradient with respect to the grid.  d/dgx is constant in ix inside a pixel cell and jumps at integer ix: the edge values
    # +-(1 + 1/W) sit there, and fp32 and fp64 may floor them to different sides.  At those components (|ix - round(ix)| <= 1e-4 in
    # fp64) the reference is the one-sided derivative nearer to the device's value; everywhere else it is the plain one.
    dg_o = Out(B * h * w * 2)
    hip.call("fs_grid_sample_bwd_grid", hip.ptr(god), hip.ptr(xd), hip.ptr(gd), dg_o.ptr, B, C, H, W, h, w, nhwc)
    dg = dg_o.get().reshape(B, h, w, 2).double()
    dg_r, dmag = R.grid_sample_bwd_grid(go, x, grid)
    on = torch.stack(((t["ix"] - t["ix"].round()).abs() <= 1e-4, (t["iy"] - t["iy"].round()).abs() <= 1e-4), -1)
    sides = []
    for sgn in (-1e-3, 1e-3):
        sides.append(torch.stack((R.grid_sample_bwd_grid(go, x, grid, dix=sgn)[0][..., 0], R.grid_sample_bwd_grid(go, x, grid, diy=sgn)[0][..., 1]), -1))
    nearer = torch.where((dg - sides[0]).abs() <= (dg - sides[1]).abs(), sides[0], sides[1])
    dg_ref = torch.where(on, nearer, dg_r)
    # per channel two differences, two products, an addition, the product with gout and the running sum: 4 C + 6 with the final scale;
    # the weights s, n (e, w) move by |d iy| (|d ix|) on four taps of at most max|x|
    gsum = (go.abs() * 4 * xmax).sum(1)
    b_dg = (4 * C + 6) * U * dmag + torch.stack((W * 0.5 * ey * gsum, H * 0.5 * ex * gsum), -1)
    check(fam, what + ".bwd_grid", dg, dg_ref, b_dg)

    # gradient with respect to the input: fp32 atomics in any order: (taps on the pixel + 2) u sum|terms|; a weight's own error reaches
    # the 4x4 neighbourhood of the grid point
    dx_o = Out(B * C * H * W)
    hip.call("fs_grid_sample_bwd_input", hip.ptr(god), hip.ptr(gd), dx_o.ptr, B, C, H, W, h, w, nhwc)
    dx_r, xmag, cnt = R.grid_sample_bwd_input(go, grid, H, W)
    b_dx = (cnt[:, None] + 2) * U * xmag + neighbourhood_sum(go.abs() * (ex + ey)[:, None], t, H, W)
    check(fam, what + ".bwd_input", dx_o.get().reshape(B, C, H, W), dx_r, b_dx)


@pytest.mark.parametrize("nhwc", [1, 0])
@pytest.mark.parametrize("H,W", [(1, 1), (4, 8), (16, 2)])
def test_grid_sample_lattice(H, W, nhwc):
    """grid points on pixel centres and half-way between them (sides a power of two: the coordinates are exact in fp32), small
    integers everywhere: weights in {0, 0.25, 0.5, 1}, every product and sum exact: all four kernels bit-equal"""
    fam = "grid_sample"
    gen = torch.Generator().manual_seed(H * W + nhwc)
    B, C, h, w = 2, 3, 9, 13
    x = randint(gen, -8, 8, B, C, H, W) * 4
    y = randint(gen, 0, 5, B, H, W) * 4
    go = randint(gen, -8, 8, B, C, h, w) * 4
    ix = torch.randint(-2, 2 * W + 2, (B, h, w), generator=gen).double() / 2 - 0.5          # -1.5 .. W + 0.5 in halves
    iy = torch.randint(-2, 2 * H + 2, (B, h, w), generator=gen).double() / 2 - 0.5
    grid = torch.stack(((ix + 0.5) * 2 / W - 1, (iy + 0.5) * 2 / H - 1), -1)
    assert torch.equal(f32(grid), grid)
    xd, yd, gd, god = dev(x), dev(y), dev(grid), dev(layout(go, nhwc))
    out_o, lab_o, ys_o, dg_o, dx_o = Out(B * C * h * w), Out(B * h * w, torch.int64, fill=-9999), Out(B * h * w), Out(B * h * w * 2), Out(B * C * H * W)
    hip.call("fs_grid_sample_fwd", hip.ptr(xd), hip.ptr(gd), out_o.ptr, B, C, H, W, h, w, nhwc)
    hip.call("fs_grid_sample_label", hip.ptr(yd), hip.ptr(gd), lab_o.ptr, ys_o.ptr, B, H, W, h, w)
    hip.call("fs_grid_sample_bwd_grid", hip.ptr(god), hip.ptr(xd), hip.ptr(gd), dg_o.ptr, B, C, H, W, h, w, nhwc)
    hip.call("fs_grid_sample_bwd_input", hip.ptr(god), hip.ptr(gd), dx_o.ptr, B, C, H, W, h, w, nhwc)
    what = f"lattice.{H}x{W}.{'nhwc' if nhwc else 'nchw'}"
    exact(fam, what + ".fwd", unlayout(out_o.get(), B, C, h, w, nhwc).double(), R.grid_sample_fwd(x, grid)[0])
    lab_r, ys_r = R.grid_sample_label(y, grid)
    exact(fam, what + ".ysamp", ys_o.get().reshape(B, h, w).double(), ys_r)
    exact(fam, what + ".label", lab_o.get().reshape(B, h, w), lab_r)
    exact(fam, what + ".bwd_grid", dg_o.get().reshape(B, h, w, 2).double(), R.grid_sample_bwd_grid(go, x, grid)[0])
    exact(fam, what + ".bwd_input", dx_o.get().reshape(B, C, H, W).double(), R.grid_sample_bwd_input(go, grid, H, W)[0])


@pytest.mark.parametrize("nhwc", [1, 0])
def test_grid_sample_bwd_input_collisions(nhwc):
    """all 1024 grid points of an image on ONE location (half-way between four pixels), integer cotangents: every atomic adds a
    multiple of 0.25 below 2^24 in magnitude: bit-equal in any order"""
    gen = torch.Generator().manual_seed(11 + nhwc)
    B, C, H, W, h, w = 2, 3, 8, 8, 32, 32
    go = randint(gen, -8, 8, B, C, h, w)
    grid = torch.zeros(B, h, w, 2, dtype=F64)
    grid[0, ..., 0], grid[0, ..., 1] = (3.5 + 0.5) * 2 / W - 1, (2.5 + 0.5) * 2 / H - 1          # ix = 3.5, iy = 2.5
    grid[1, ..., 0], grid[1, ..., 1] = (7.5 + 0.5) * 2 / W - 1, (-0.5 + 0.5) * 2 / H - 1          # a corner: one tap inside
    gd, god = dev(grid), dev(layout(go, nhwc))
    dx_o = Out(B * C * H * W)
    hip.call("fs_grid_sample_bwd_input", hip.ptr(god), hip.ptr(gd), dx_o.ptr, B, C, H, W, h, w, nhwc)
    dx_r, _, cnt = R.grid_sample_bwd_input(go, grid, H, W)
    assert float(cnt.max()) == 1024
    exact("grid_sample", f"bwd_input.collisions.{'nhwc' if nhwc else 'nchw'}", dx_o.get().reshape(B, C, H, W).double(), dx_r)


# ================================================================================================
# segmentation loss
# ================================================================================================
def seg_inputs(gen, B, K, HW, kind):
    if kind == "ties":          # small integers: several classes share the maximum
        pred = randint(gen, -2, 2, B, K, HW)
    elif kind == "saturated":
        pred = torch.where(torch.rand(B, K, HW, generator=gen) > 0.5, 60.0, -60.0).double()
    else:
        pred = f32(randn(gen, B, K, HW) * 3)
    gt = torch.randint(0, K, (B, HW), generator=gen)
    if kind == "absent":          # the odd classes never occur
        gt = gt // 2 * 2
    return pred, gt


def seg_errors(pred, logp, K):
    """softmax pieces: z = v - max (u |z|), expf (2 u each), their sum (K u), logf (u |lse| + 3 u), log p = z - lse (u |log p|):
    e_lp; p = expf(log p): relative e_lp + 2 u.  (1 - pt)^gamma by powf: gamma (1 - pt)^(gamma - 1) (e_pt + u (1 - pt)) + 4 u (1 - pt)^gamma."""
    z = pred - pred.max(dim=1, keepdim=True).values
    e_lp = U * (z.abs() + logp.abs()) + (K + 4) * U + U * (z - logp).abs()
    r_p = e_lp + 2 * U
    return e_lp, r_p


def pow_err(pt, r_pt, gamma):
    one = 1.0 - pt
    if gamma == 0:
        return torch.zeros_like(pt)
    return gamma * one ** (gamma - 1) * (pt * r_pt + U * one) + 4 * U * one ** gamma


SEG_CASES = [(1, 2, 1, "random"), (3, 7, 45, "random"), (2, 51, 1517, "random"), (2, 64, 1025, "random"), (3, 51, 6400, "absent"),
             (3, 7, 45, "saturated"), (2, 5, 1030, "ties"), (2, 64, 300, "ties")]


@pytest.mark.parametrize("gamma", [5.0, 0.0])
@pytest.mark.parametrize("B,K,HW,kind", SEG_CASES)
def test_seg_loss(B, K, HW, kind, gamma):
    fam = "seg_loss"
    what = f"B{B}.K{K}.HW{HW}.{kind}.g{gamma:g}"
    gen = torch.Generator().manual_seed(K * 100 + HW)
    pred, gt = seg_inputs(gen, B, K, HW, kind)
    assert int(gt.min()) >= 0 and int(gt.max()) < K
    eps, gout = float(torch.tensor(1e-7).float()), float(torch.tensor(0.37).float())
    bpi = -(-HW // 1024)
    nacc = B * bpi * (3 * K + 7)
    acc_o, out_o, coef_o = Out(nacc, F64), Out(7), Out(2 * K)
    pd, gtd = dev(pred), gt.to(DEV)
    hip.call("fs_seg_loss_fwd", hip.ptr(pd), hip.ptr(gtd), B, K, HW, gamma, eps, acc_o.ptr, out_o.ptr, coef_o.ptr)
    out_r, coef_r, ps = R.seg_loss_fwd(pred, gt, gamma, eps)
    out32, coef32, _ = R.seg_loss_fwd(pred.float(), gt, gamma, eps)
    rec = acc_o.get().reshape(B, bpi, 3 * K + 7)
    # the counters of every workgroup's record: exact
    exact(fam, what + ".counters", rec[:, :, 3 * K + 1:].sum(1), R.seg_counters(pred, gt).double())
    exact(fam, what + ".class_counts", rec[:, :, 2 * K:3 * K].sum((0, 1)), ps["N"])
    if kind == "ties":
        assert float((pred == pred.max(1, keepdim=True).values).sum(1).double().mean()) > 1.2
    if kind == "absent":
        assert int((ps["N"] == 0).sum()) == K // 2

    e_lp, r_p = seg_errors(pred, ps["logp"], K)
    p = ps["p"]
    onehot = (gt[:, None, :] == torch.arange(K)[None, :, None]).double()
    e_lpt, r_pt = (e_lp * onehot).sum(1), (r_p * onehot).sum(1)
    pt, logpt = ps["pt"], ps["logpt"]
    # focal: |log pt| times the error of the power, the power times the error of log pt, the product and the negation; summed in double;
    # the mean and its cast 2 u
    f = (1 - pt) ** gamma * logpt.abs()
    e_f = logpt.abs() * pow_err(pt, r_pt, gamma) + (1 - pt) ** gamma * e_lpt + 2 * U * f
    b_focal = e_f.sum() / (B * HW) + 2 * U * out_r[1].abs()
    # P_k: per thread at most 4 pixels, six shuffle stages, 4 waves in fp32 (14 u), the records in double; I_k: 2^-40 fixed point per
    # pixel, one cast; card = float(P) + float(N): 2 u
    # (a probability below 2^-126 may be flushed to zero: TINY per pixel)
    e_P = (p * r_p).sum((0, 2)) + 14 * U * ps["P"] + B * HW * TINY
    e_I = (p * onehot * r_p).sum((0, 2)) + B * HW * (2.0 ** -40 + TINY) + U * ps["I"]
    e_card = e_P + 2 * U * ps["card"]
    den, I, pres = ps["den"], ps["I"], ps["present"].double()
    # dice_k = 1 - 2 I / den: the quotient, the doubling and the difference (4 u on 2 I / den, u on the result <= 1)
    e_k = pres * (2 * e_I / den + 2 * I * e_card / den ** 2 + 4 * U * 2 * I / den + U)
    b_dice = e_k.sum() / K + 2 * U * out_r[2].abs()
    b_out = torch.stack((b_focal + b_dice + U * out_r[0].abs(), b_focal, b_dice) + (torch.tensor(8 * U, dtype=F64),) * 4)          # acc: exact counters, <= 8 roundings at <= 1
    check(fam, what + ".out", out_o.get(), out_r, b_out, out32)
    # A = 2 I / den^2 / K (6 roundings), B = -2 / den / K (4)
    A, Bc = coef_r[:K], coef_r[K:]
    e_A = pres * (2 * e_I / den ** 2 + 4 * I * e_card / den ** 3) / K + 6 * U * A.abs()
    e_B = pres * (2 * e_card / den ** 2) / K + 4 * U * Bc.abs()
    check(fam, what + ".coef", coef_o.get(), coef_r, torch.cat((e_A, e_B)), coef32)

    # backward from the reference's coefficients rounded to fp32
    coef_in = f32(coef_r)
    cd, god = dev(coef_in), dev(torch.tensor([gout], dtype=F64))
    dp_o = Out(B * K * HW)
    hip.call("fs_seg_loss_bwd", hip.ptr(pd), hip.ptr(gtd), hip.ptr(cd), hip.ptr(god), dp_o.ptr, B, K, HW, gamma)
    dp_r, bp = R.seg_loss_bwd(pred, gt, coef_in, gout, gamma)
    dp32, _ = R.seg_loss_bwd(pred.float(), gt, coef_in.float(), gout, gamma)
    q, dot = bp["q"].abs(), bp["dot"].abs()
    # dot = sum p q: K products in sequence; dd = p (q - dot); fw = pow / (B HW) (2 u); df = -fw ([k = t] - p); gout (dd + df): 2 u
    e_dot = (p * q * r_p).sum(1, keepdim=True) + (K + 2) * U * bp["absdot"]
    e_dd = p * (e_dot + 2 * U * (q + dot)) + p * (q + dot) * r_p
    r_ptk = r_pt[:, None, :]
    e_fw = pow_err(bp["pt"], r_ptk, gamma) / (B * HW) + 2 * U * bp["fw"]
    e_df = e_fw * (onehot - p).abs() + bp["fw"] * (p * r_p + U) + U * bp["df"].abs()
    check(fam, what + ".dpred", dp_o.get().reshape(B, K, HW), dp_r, abs(gout) * (e_dd + e_df) + 2 * U * dp_r.abs() + 4 * TINY, dp32)


def test_seg_loss_rejects():
    z = torch.zeros(1024, device=DEV)
    gt = torch.zeros(16, dtype=torch.int64, device=DEV)
    p = hip.ptr(z)
    for K in (1, 65):
        o = [Out(3 * K + 7, F64), Out(7), Out(2 * K), Out(K * 8)]
        rejected(o[:3], "fs_seg_loss_fwd", p, hip.ptr(gt), 1, K, 8, 5.0, 1e-7, o[0].ptr, o[1].ptr, o[2].ptr)
        rejected(o[3:], "fs_seg_loss_bwd", p, hip.ptr(gt), p, p, o[3].ptr, 1, K, 8, 5.0)
