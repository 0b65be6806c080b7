"""The memory-bound kernels (csrc/elementwise.hip, the head tail of csrc/head_loss.hip, csrc/optim.hip) at the C ABI against the
plain fp64 references of oracle/elementwise_ref.py (which tests/test_elementwise_ref.py holds to torch on the CPU).

Rules of every case
  * every output buffer is allocated with a guard of GUARD floats of sentinel on both sides and pre-filled with NaN (a marker
    value for integer buffers): after the call no fill value is left where an output is due and the guards are untouched
    (class Out); slices a kernel must leave alone hold a sentinel and are compared exactly;
  * two kinds of data: "int" -- small integers and powers of two, every sum below 2^24, so every reduction is exact in fp32
    in any order and must be BIT-EQUAL to the reference; "float" -- random data, held to the forward error bound
    L * 2^-24 * sum|terms| of the expression (L = the longest fp32 chain, derived beside each check) or, for the pointwise
    passes and Adam, to 4x the error of the same formula evaluated in fp32 by torch on the CPU, whichever is larger.
    No bound is taken from what a kernel returns;
  * no element is left out of a comparison.  Activation branches are taken from the device's own output (bit j <=> out > 0,
    and < 6 for ReLU6), which the mask bytes must equal exactly; the backward stages take that mask as input.

Each stage gets clean inputs (reference values rounded to fp32), never the previous stage's device output, except where the
output IS the next stage's defined input (the activation mask, the slab of a producer).
Every check prints `[bound] family what ratio`: the largest error as a fraction of its bound (profiles/r08/README.md).
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fovealseg  # noqa: E402
from fovealseg import ops  # noqa: E402
import fovealseg_oracle as O  # noqa: E402
import elementwise_ref as R  # noqa: E402
from kernel_testing import GUARD, U, Out, check, choice, dev, exact, f32, randint, randn, report  # noqa: E402,F401

hip = fovealseg.hip
DEV = "cuda"
EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.1))          # as the C ABI carries them: float


# ------------------------------------------------------------------------------------------------
# the row walk of the BatchNorm kernels, read off csrc/elementwise.hip (RowWalk, rows_per_block_for)
# ------------------------------------------------------------------------------------------------
def row_walk(M, C):
    """(row lanes, rows per block) of one channel window of C <= 1024 channels"""
    cw = C // 4
    rpi = max(256 // cw, 1)
    rpb = -(-M // 1024)
    return rpi, max(-(-rpb // rpi) * rpi, rpi)


def chain_len(M, C):
    """longest fp32 addition chain of one column sum of a slab: rows per thread, then the row lanes in LDS (the slab rows are
    added in double by the finalize kernels, in fp64 on the host here)"""
    L = 0
    for c0 in range(0, C, 1024):
        rpi, rpb = row_walk(M, min(1024, C - c0))
        L = max(L, rpb // rpi + rpi)
    return L


def slab_sums(slab, nslab, C):
    s = slab.double().reshape(nslab, C, 2).sum(0)
    return s[:, 0], s[:, 1]


# ================================================================================================
# BatchNorm family
# ================================================================================================
#            C     M      act res route  train acc drop running
BN_CASES = [(4, 1, 0, 0, "z", 1, 0, 0.0, 1),
            (4, 4099, 1, 1, "mask", 1, 1, 0.3, 0),
            (20, 2, 2, 0, "mask", 1, 0, 0.0, 1),
            (20, 1025, 1, 1, "z", 0, 1, 0.0, 1),
            (24, 7, 1, 0, "mask", 1, 1, 0.3, 1),
            (24, 12800, 2, 1, "z", 1, 0, 0.0, 0),
            (48, 255, 1, 1, "mask", 1, 0, 0.0, 1),
            (48, 1023, 0, 0, "z", 1, 1, 0.3, 0),
            (64, 1025, 2, 1, "mask", 0, 0, 0.0, 1),
            (64, 12800, 1, 1, "mask", 1, 1, 0.3, 1),
            (64, 409600, 1, 1, "mask", 1, 0, 0.0, 1),
            (132, 7, 0, 1, "z", 1, 1, 0.0, 0),
            (132, 4099, 1, 0, "mask", 1, 0, 0.3, 1),
            (192, 255, 2, 1, "z", 1, 1, 0.0, 1),
            (192, 1023, 1, 0, "mask", 0, 0, 0.0, 1),
            (240, 1, 1, 0, "mask", 1, 1, 0.0, 0),
            (240, 12800, 1, 1, "mask", 1, 0, 0.0, 1),
            (256, 2, 0, 0, "z", 1, 0, 0.3, 1),
            (256, 4099, 2, 1, "mask", 1, 1, 0.0, 0),
            (512, 7, 1, 1, "z", 1, 0, 0.0, 1),
            (512, 1025, 1, 0, "mask", 1, 1, 0.3, 1),
            (1024, 255, 2, 0, "mask", 1, 0, 0.0, 0),
            (1024, 1023, 1, 1, "z", 1, 1, 0.3, 1),
            (1028, 1, 1, 1, "mask", 1, 0, 0.3, 1),
            (1028, 1025, 1, 1, "mask", 1, 1, 0.3, 1),
            (1028, 4099, 2, 0, "z", 1, 0, 0.0, 0),
            (2048, 2, 0, 1, "mask", 0, 1, 0.0, 1),
            (2048, 255, 1, 1, "mask", 1, 0, 0.3, 1),
            (2048, 1023, 1, 0, "z", 1, 1, 0.0, 0)]


def replay_act(pre, out_dev, act):
    """the reference activation on the branch the device took"""
    if act == 1:
        return torch.where(out_dev > 0, pre, torch.zeros_like(pre))
    if act == 2:
        return torch.where((out_dev > 0) & (out_dev < 6), pre, torch.where(out_dev >= 6, torch.full_like(pre, 6.0), torch.zeros_like(pre)))
    return pre


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("C,M,act,use_res,route,training,acc,drop_p,running", BN_CASES)
def test_batchnorm_chain(C, M, act, use_res, route, training, acc, drop_p, running, kind):
    fam = "batchnorm"
    gen = torch.Generator().manual_seed(C * 7 + M + act)
    integer = kind == "int"
    if integer:          # |y| <= 3, |mean| <= 1, invstd in {1, 1/2}, |dz| <= 2: every sum is below 16 * M half-units < 2^24 at M = 409 600
        y = randint(gen, -3, 3, M, C)
        gamma, beta = choice(gen, [0.5, 1.0, 2.0], C), randint(gen, -2, 2, C)
        res = randint(gen, -3, 3, M, C) if use_res else None
        dz = randint(gen, -2, 2, M, C)
        rm, rv = randint(gen, -2, 2, C), choice(gen, [1.0, 2.0, 4.0], C)
        mean_in, invstd_in = randint(gen, -1, 1, C), choice(gen, [1.0, 0.5], C)
    else:
        y = randn(gen, M, C) * f32(0.5 + torch.rand(C, generator=gen, dtype=torch.float64)) + randn(gen, C)
        y = f32(y)
        gamma, beta = f32(0.5 + randn(gen, C).abs()), randn(gen, C)
        res = randn(gen, M, C) if use_res else None
        dz = randn(gen, M, C)
        rm, rv = f32(randn(gen, C) * 0.1), f32(1 + torch.rand(C, generator=gen, dtype=torch.float64))
        if training:
            mean_in, invstd_in, _, _ = R.bn_batch_stats(y, EPS)
        else:
            mean_in, invstd_in = R.bn_eval_prepare(rm, rv, EPS)
        mean_in, invstd_in = f32(mean_in), f32(invstd_in)
    yd = dev(y)

    # ---- statistics -----------------------------------------------------------------------------------------------------------
    if training:
        mean_o, invstd_o = Out(C), Out(C)
        rm_o, rv_o = (Out(C, body=rm), Out(C, body=rv)) if running else (None, None)
        sums = Out(hip.query("fs_bn_stats_scratch_doubles", M, C), torch.float64)
        hip.call("fs_bn_stats", hip.ptr(yd), M, C, MOM, EPS, rm_o.ptr if running else None, rv_o.ptr if running else None,
                 mean_o.ptr, invstd_o.ptr, sums.ptr)
        sums.get(complete=False)
        mean_r, invstd_r, rm_r, rv_r = R.bn_batch_stats(y, EPS, MOM, rm, rv)
        var_r = 1.0 / invstd_r ** 2 - EPS
        if integer:          # exact sums: the results are the roundings of (almost) the exact values, 1 ulp <= 2^-23 |x|
            dmean, dvar = 2 * U * mean_r.abs(), 2 * U * var_r
            check(fam, "stats.mean.int", mean_o.get(), mean_r, dmean)
            check(fam, "stats.invstd.int", invstd_o.get(), invstd_r, 2 * U * invstd_r)
        else:
            # per thread rpb / rpi fp32 additions of y (and of y * y, one more rounding), then double: L = rpb / rpi (+ 1), + 1 for the store
            L = max(row_walk(M, min(1024, C - c0))[1] // row_walk(M, min(1024, C - c0))[0] for c0 in range(0, C, 1024))
            dmean = (L + 1) * U * y.abs().sum(0) / M + U * mean_r.abs()
            dvar = (L + 2) * U * (y * y).sum(0) / M + 2 * mean_r.abs() * dmean          # var = E[y^2] - mean^2
            check(fam, "stats.mean", mean_o.get(), mean_r, dmean)
            check(fam, "stats.invstd", invstd_o.get(), invstd_r, 0.5 * invstd_r ** 3 * dvar + U * invstd_r)       # d(v^-1/2) = v^-3/2 / 2
        if running:          # mom * x + (1 - mom) * r: three roundings on top of the error of x
            unb = M / (M - 1 if M > 1 else 1)
            check(fam, "stats.running_mean", rm_o.get(), rm_r, MOM * dmean + 4 * U * (MOM * mean_r.abs() + (1 - MOM) * rm.abs()))
            check(fam, "stats.running_var", rv_o.get(), rv_r, MOM * unb * dvar + 5 * U * (MOM * unb * var_r + (1 - MOM) * rv.abs()))
    else:
        mean_o, invstd_o, scale_o, shift_o = Out(C), Out(C), Out(C), Out(C)
        rmd, rvd, gd_, bd_ = dev(rm), dev(rv), dev(gamma), dev(beta)
        hip.call("fs_bn_eval_prepare", hip.ptr(rmd), hip.ptr(rvd), C, EPS, mean_o.ptr, invstd_o.ptr)
        hip.call("fs_bn_eval_affine", hip.ptr(rmd), hip.ptr(rvd), hip.ptr(gd_), hip.ptr(bd_), C, EPS, scale_o.ptr, shift_o.ptr)
        m_r, i_r = R.bn_eval_prepare(rm, rv, EPS)
        s_r, h_r = R.bn_eval_affine(rm, rv, gamma, beta, EPS)
        exact(fam, "eval.mean", mean_o.get(), m_r.float())
        m32, i32 = R.bn_eval_prepare(rm.float(), rv.float(), EPS)
        s32, h32 = R.bn_eval_affine(rm.float(), rv.float(), gamma.float(), beta.float(), EPS)
        check(fam, "eval.invstd", invstd_o.get(), i_r, 3 * U * i_r, i32)                       # add, sqrt, divide
        check(fam, "eval.scale", scale_o.get(), s_r, 4 * U * s_r.abs(), s32)                   # ... and the product with gamma
        check(fam, "eval.shift", shift_o.get(), h_r, 6 * U * (beta.abs() + (rm * s_r).abs()), h32)

    # ---- apply + residual + activation ------------------------------------------------------------------------------------------
    md, isd, gd, bd, rd = dev(mean_in), dev(invstd_in), dev(gamma), dev(beta), dev(res)
    out_o = Out(M * C)
    mask_o = Out(M * C // 4, torch.uint8) if route == "mask" else None
    hip.call("fs_bn_act_fwd", hip.ptr(yd), hip.ptr(md), hip.ptr(isd), hip.ptr(gd), hip.ptr(bd), hip.ptr(rd), out_o.ptr,
             mask_o.ptr if mask_o else None, M, C, act)
    out_d = out_o.get().reshape(M, C).double()
    bits = R.act_bits(out_d, act)
    if mask_o:
        exact(fam, "act_fwd.mask", mask_o.get(), R.pack_mask(bits))
    pre = R.bn_pre_act(y, mean_in, invstd_in, gamma, beta, res)
    if integer:
        exact(fam, "act_fwd.out.int", out_d, R.act_fwd(pre, act))
    else:
        # sc = invstd * gamma, sh = beta - mean * sc, v = y * sc + sh [+ res]: six roundings, each at most U times the largest partial sum
        sc = invstd_in * gamma
        bound = 6 * U * ((y * sc).abs() + (mean_in * sc).abs() + beta.abs() + (res.abs() if use_res else 0))
        pre32 = R.bn_pre_act(y.float(), mean_in.float(), invstd_in.float(), gamma.float(), beta.float(), res.float() if use_res else None)
        check(fam, "act_fwd.out", out_d, replay_act(pre, out_d, act), bound, replay_act(pre32, out_d.float(), act))
    del pre

    # ---- backward: column sums ----------------------------------------------------------------------------------------------------
    nslab = hip.query("fs_bn_bwd_slabs", M, C)
    dzd = dev(dz)
    zd = out_o.t if route == "z" else None
    maskd = mask_o.t if mask_o else None
    slab_o = Out(nslab * C * 2)
    hip.call("fs_bn_bwd_partial", hip.ptr(dzd), hip.ptr(zd), hip.ptr(maskd), hip.ptr(yd), hip.ptr(md), hip.ptr(isd), M, C, act, slab_o.ptr)
    S_d, SX_d = slab_sums(slab_o.get(), nslab, C)
    S_r, SX_r = R.bn_bwd_sums(dz, bits, y, mean_in, invstd_in)
    L = chain_len(M, C)
    g_abs = torch.where(bits, dz, torch.zeros_like(dz)).abs()
    xhat_abs = ((y - mean_in) * invstd_in).abs()
    # S: L additions of exact terms; SX: every term g * ((y - mean) * invstd) carries three roundings of its own
    bS, bSX = L * U * g_abs.sum(0), (L + 3) * U * (g_abs * xhat_abs).sum(0)
    if integer:
        exact(fam, "bwd_partial.S.int", S_d, S_r)
        exact(fam, "bwd_partial.SX.int", SX_d, SX_r)
    else:
        check(fam, "bwd_partial.S", S_d, S_r, bS)
        check(fam, "bwd_partial.SX", SX_d, SX_r, bSX)

    # the same sums from the kernel that forms dz as a sum of 2 - 4 gradients (mask route only: it has no z argument)
    if route == "mask" or act == 0:
        nop = 2 + (C // 4 + M) % 3
        parts = [randint(gen, -1, 1, M, C) if integer else randn(gen, M, C) for _ in range(nop)]
        pd = [dev(p) for p in parts] + [None, None]
        sum_o, slab2 = Out(M * C), Out(nslab * C * 2)
        hip.call("fs_add_n_bnsum", hip.ptr(pd[0]), hip.ptr(pd[1]), hip.ptr(pd[2]), hip.ptr(pd[3]), sum_o.ptr, hip.ptr(maskd), hip.ptr(yd),
                 hip.ptr(md), hip.ptr(isd), M, C, act, slab2.ptr)
        tot_d = sum_o.get().reshape(M, C).double()
        tot_r = R.add_n(parts)
        S2, SX2 = slab_sums(slab2.get(), nslab, C)
        bits2 = bits if maskd is not None else torch.ones_like(bits)
        Sr2, SXr2 = R.bn_bwd_sums(tot_d, bits2, y, mean_in, invstd_in)          # the sums of the gradient the kernel itself stored
        if integer:
            exact(fam, f"add_n_bnsum{nop}.out.int", tot_d, tot_r)
            exact(fam, f"add_n_bnsum{nop}.S.int", S2, Sr2)
            exact(fam, f"add_n_bnsum{nop}.SX.int", SX2, SXr2)
        else:
            check(fam, f"add_n_bnsum{nop}.out", tot_d, tot_r, (nop - 1) * U * sum(p.abs() for p in parts), R.add_n([p.float() for p in parts]))
            ga2 = torch.where(bits2, tot_d, torch.zeros_like(tot_d)).abs()
            check(fam, f"add_n_bnsum{nop}.S", S2, Sr2, L * U * ga2.sum(0))
            check(fam, f"add_n_bnsum{nop}.SX", SX2, SXr2, (L + 3) * U * (ga2 * xhat_abs).sum(0))
        del parts, pd, tot_d, tot_r

    # g = dout * (out > 0) of an HRNet fuse node plus the sums of 1 - 3 layers that receive it
    if C <= 1024:
        nterm = 1 + (C // 4 + M) % 3
        fz = (randint(gen, -2, 2, M, C) if integer else randn(gen, M, C)).clamp(min=0)
        ys = [y, f32(y * 0.5), -y][:nterm]
        ysd = [dev(t) for t in ys]
        fzd = dev(fz)
        g_o = Out(M * C)
        slabs = [Out(nslab * C * 2) for _ in range(nterm)]
        arr = lambda ps: (ctypes.c_void_p * len(ps))(*ps)          # noqa: E731
        hip.call("fs_relu_bwd_bnsum", hip.ptr(dzd), hip.ptr(fzd), g_o.ptr, M, C, nterm, arr([hip.ptr(t) for t in ysd]),
                 arr([hip.ptr(md)] * nterm), arr([hip.ptr(isd)] * nterm), arr([s.ptr for s in slabs]))
        exact(fam, "relu_bwd_bnsum.g", g_o.get().double(), R.relu_bwd(dz, fz))
        for k in range(nterm):
            Sk, SXk = slab_sums(slabs[k].get(), nslab, C)
            Sr, SXr = R.bn_bwd_sums(dz, fz > 0, ys[k], mean_in, invstd_in)
            ga = torch.where(fz > 0, dz, torch.zeros_like(dz)).abs()
            if integer:
                exact(fam, f"relu_bwd_bnsum.S{k}.int", Sk, Sr)
                exact(fam, f"relu_bwd_bnsum.SX{k}.int", SXk, SXr)
            else:
                check(fam, f"relu_bwd_bnsum.S{k}", Sk, Sr, L * U * ga.sum(0))
                check(fam, f"relu_bwd_bnsum.SX{k}", SXk, SXr, (L + 3) * U * (ga * ((ys[k] - mean_in) * invstd_in).abs()).sum(0))
        del ys, ysd, fz, fzd

    # ---- backward: finalize (the producer's slab is its input) ---------------------------------------------------------------------
    tg, tb = (randint(gen, -3, 3, C), randint(gen, -3, 3, C)) if integer else (randn(gen, C), randn(gen, C))
    coef_o, dg_o, db_o = Out(4 * C), Out(C, body=tg if acc else None), Out(C, body=tb if acc else None)
    hip.call("fs_bn_bwd_finalize", slab_o.ptr, nslab, hip.ptr(gd), hip.ptr(md), hip.ptr(isd), M, C, training, coef_o.ptr, dg_o.ptr, db_o.ptr, acc)
    dg_r, db_r, coef_r = R.bn_bwd_finalize(S_d, SX_d, gamma, mean_in, invstd_in, M, training)
    if acc:
        dg_r, db_r = dg_r + tg, db_r + tb
    if integer:
        exact(fam, "bwd_finalize.dgamma.int", dg_o.get().double(), dg_r)
        exact(fam, "bwd_finalize.dbeta.int", db_o.get().double(), db_r)
    else:          # the double sum is rounded to fp32 once and added to the target in fp32
        check(fam, "bwd_finalize.dgamma", dg_o.get(), dg_r, 2 * U * (SX_d.abs() + (tg.abs() if acc else 0)))
        check(fam, "bwd_finalize.dbeta", db_o.get(), db_r, 2 * U * (S_d.abs() + (tb.abs() if acc else 0)))
    # ga = gamma * invstd (1 rounding), d = ga * fp32(SX / M) * invstd (3 more), mean copied, bb = ga * fp32(S / M) (2 more)
    cb = torch.stack([U * coef_r[0].abs(), 4 * U * coef_r[1].abs(), torch.zeros(C, dtype=torch.float64), 3 * U * coef_r[3].abs()])
    c32 = R.bn_bwd_finalize(S_d.float(), SX_d.float(), gamma.float(), mean_in.float(), invstd_in.float(), M, training)[2]
    check(fam, "bwd_finalize.coef", coef_o.get().reshape(4, C), coef_r, cb, c32)

    # ---- backward: apply ------------------------------------------------------------------------------------------------------------
    coef_in = f32(R.bn_bwd_finalize(S_r, SX_r, gamma, mean_in, invstd_in, M, training)[2])
    key = ops.layer_key(123, C + M)
    keep = torch.from_numpy(O.dropout_keep_mask_nhwc(M * C, key, drop_p)).reshape(M, C) if drop_p > 0 else None
    dy_o, dres_o = Out(M * C), Out(M * C) if use_res else None
    cd = dev(coef_in)
    hip.call("fs_bn_bwd_apply", hip.ptr(dzd), hip.ptr(zd), hip.ptr(maskd), hip.ptr(yd), hip.ptr(cd), M, C, act, float(drop_p), key,
             dy_o.ptr, dres_o.ptr if use_res else None)
    dy_r, g_r = R.bn_bwd_apply(dz, bits, y, coef_in, keep, drop_p)
    if use_res:
        exact(fam, "bwd_apply.dres", dres_o.get().double(), g_r)
    # ga * g - d * (y - mean) - bb: three products, three differences, then the dropout scale (its own rounding and the product's)
    bound = 8 * U * ((coef_in[0] * g_r).abs() + (coef_in[1] * (y - coef_in[2])).abs() + coef_in[3].abs()) / (1 - drop_p)
    if keep is not None:
        bound = torch.where(keep, bound, torch.zeros_like(bound))          # dropped elements are exact zeros
    dy32 = R.bn_bwd_apply(dz.float(), bits, y.float(), coef_in.float(), keep, drop_p)[0]
    check(fam, f"bwd_apply.dy.{kind}", dy_o.get(), dy_r, bound, dy32)


@pytest.mark.parametrize("nwg,C", [(1, 4), (3, 20), (255, 132), (256, 64), (257, 1028), (1000, 256)])
@pytest.mark.parametrize("kind", ["int", "float"])
def test_batchnorm_finalize_from_host_slabs(nwg, C, kind):
    """fs_bn_finalize_slab and fs_bn_bwd_finalize on slabs made on the host: their reduction apart from the producers."""
    fam = "batchnorm"
    gen = torch.Generator().manual_seed(nwg + C)
    integer = kind == "int"
    rpw = 5
    M = nwg * rpw
    y = randint(gen, -3, 3, M, C) if integer else f32(randn(gen, M, C) + 2.0)
    part = y.reshape(nwg, rpw, C)
    slab = f32(torch.stack([part.sum(1), (part * part).sum(1)], dim=2))          # [nwg][C][2], fp32 as the conv epilogue stores it
    rm, rv = (randint(gen, -2, 2, C), choice(gen, [1.0, 2.0], C)) if integer else (randn(gen, C), f32(1 + torch.rand(C, generator=gen, dtype=torch.float64)))
    mean_o, invstd_o, rm_o, rv_o = Out(C), Out(C), Out(C, body=rm), Out(C, body=rv)
    sd = dev(slab)
    hip.call("fs_bn_finalize_slab", hip.ptr(sd), nwg, M, C, MOM, EPS, rm_o.ptr, rv_o.ptr, mean_o.ptr, invstd_o.ptr)
    s1, s2 = slab[:, :, 0].sum(0), slab[:, :, 1].sum(0)
    mean_r, var_r, invstd_r = R.bn_stats_from_sums(s1, s2, M, EPS)          # the slab is the input: its fp64 sums define the result
    unb = M / (M - 1)
    # the sums are formed in double: what is left is the rounding of the results (and of var = E[y^2] - mean^2 in double)
    dvar = 4 * 2.0 ** -53 * (s2 / M)
    check(fam, f"finalize_slab.mean.{kind}", mean_o.get(), mean_r, U * mean_r.abs())
    check(fam, f"finalize_slab.invstd.{kind}", invstd_o.get(), invstd_r, U * invstd_r + 0.5 * invstd_r ** 3 * dvar)
    check(fam, f"finalize_slab.running_mean.{kind}", rm_o.get(), MOM * mean_r + (1 - MOM) * rm,
          4 * U * (MOM * mean_r.abs() + (1 - MOM) * rm.abs()))
    check(fam, f"finalize_slab.running_var.{kind}", rv_o.get(), MOM * unb * var_r + (1 - MOM) * rv,
          5 * U * (MOM * unb * var_r + (1 - MOM) * rv.abs()) + MOM * unb * dvar)
    if integer:          # exact sums: also the two-pass statistics of the rows themselves, to 1 ulp
        m2, i2, _, _ = R.bn_batch_stats(y, EPS)
        check(fam, "finalize_slab.mean.two_pass", mean_o.get(), m2, 2 * U * m2.abs())
        check(fam, "finalize_slab.invstd.two_pass", invstd_o.get(), i2, 2 * U * i2)
    nullrun = Out(C), Out(C)          # running statistics NULL
    hip.call("fs_bn_finalize_slab", hip.ptr(sd), nwg, M, C, MOM, EPS, None, None, nullrun[0].ptr, nullrun[1].ptr)
    exact(fam, "finalize_slab.mean.norunning", nullrun[0].get(), mean_o.get())
    exact(fam, "finalize_slab.invstd.norunning", nullrun[1].get(), invstd_o.get())

    # backward finalize on a host slab of nwg rows
    bs = torch.stack([randint(gen, -50, 50, nwg, C), randint(gen, -50, 50, nwg, C) * 0.5], dim=2) if integer else randn(gen, nwg, C, 2)
    gamma = choice(gen, [0.5, 1.0, 2.0], C) if integer else f32(0.5 + randn(gen, C).abs())
    mean_in = randint(gen, -1, 1, C) if integer else randn(gen, C)
    invstd_in = choice(gen, [1.0, 0.5], C) if integer else f32(0.5 + torch.rand(C, generator=gen, dtype=torch.float64))
    S, SX = bs[:, :, 0].sum(0), bs[:, :, 1].sum(0)
    bsd, gd, md, isd = dev(bs), dev(gamma), dev(mean_in), dev(invstd_in)
    for acc in (0, 1):
        tg, tb = (randint(gen, -3, 3, C), randint(gen, -3, 3, C)) if integer else (randn(gen, C), randn(gen, C))
        coef_o, dg_o, db_o = Out(4 * C), Out(C, body=tg if acc else None), Out(C, body=tb if acc else None)
        hip.call("fs_bn_bwd_finalize", hip.ptr(bsd), nwg, hip.ptr(gd), hip.ptr(md), hip.ptr(isd), M, C, 1, coef_o.ptr, dg_o.ptr, db_o.ptr, acc)
        dg_r, db_r, coef_r = R.bn_bwd_finalize(S, SX, gamma, mean_in, invstd_in, M, True)
        dg_r, db_r = (dg_r + tg, db_r + tb) if acc else (dg_r, db_r)
        if integer:
            exact(fam, "bwd_finalize.host.dgamma.int", dg_o.get().double(), dg_r)
            exact(fam, "bwd_finalize.host.dbeta.int", db_o.get().double(), db_r)
        else:
            check(fam, "bwd_finalize.host.dgamma", dg_o.get(), dg_r, 2 * U * (SX.abs() + (tg.abs() if acc else 0)))
            check(fam, "bwd_finalize.host.dbeta", db_o.get(), db_r, 2 * U * (S.abs() + (tb.abs() if acc else 0)))
        cb = torch.stack([U * coef_r[0].abs(), 4 * U * coef_r[1].abs(), torch.zeros(C, dtype=torch.float64), 3 * U * coef_r[3].abs()])
        check(fam, f"bwd_finalize.host.coef.{kind}", coef_o.get().reshape(4, C), coef_r, cb)


# ---- statistics with an offset mean ---------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _offset_errors(y_dev_t, M, C, mean_o, invstd_o, rm_o, rv_o, rm, rv):
    """(normalised output, running mean, running var, variance) relative errors of device statistics of the device tensor y"""
    y = y_dev_t.cpu().double().reshape(M, C)
    mean_r, invstd_r, rm_r, rv_r = R.bn_batch_stats(y, EPS, MOM, rm, rv)
    ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    out_o = Out(M * C)
    hip.call("fs_bn_act_fwd", hip.ptr(y_dev_t), mean_o.ptr, invstd_o.ptr, hip.ptr(ones), hip.ptr(zeros), None, out_o.ptr, None, M, C, 0)
    norm = relerr(out_o.get().reshape(M, C), (y - mean_r) * invstd_r)
    var_d, var_r = 1.0 / invstd_o.get().double() ** 2 - EPS, 1.0 / invstd_r ** 2 - EPS
    return norm, relerr(rm_o.get(), rm_r), relerr(rv_o.get(), rv_r), float(((var_d - var_r).abs() / var_r).max())


@pytest.mark.parametrize("ratio", [10, 30, 100])
def test_batchnorm_stats_offset_mean(ratio):
    """|mean| / sigma = ratio in every channel.  The CPU oracle's 315 BatchNorm inputs reach 4.67 at most (median 2.05) on the
    training batch at name-keyed initialisation; 10 is asserted with the project's own bounds (2e-5 on the normalised output,
    1e-5 on the running statistics, as test_conv_bn_act), 30 and 100 are reported (DESIGN.md states the envelope)."""
    gen = torch.Generator().manual_seed(ratio)
    M, C = 12800, 64
    sigma = f32(0.5 + 1.5 * torch.rand(C, generator=gen, dtype=torch.float64))
    sign = choice(gen, [-1.0, 1.0], C)
    y = f32((randn(gen, M, C) + ratio * sign) * sigma)
    rm, rv = f32(randn(gen, C) * 0.1), f32(1 + 0.1 * torch.rand(C, generator=gen, dtype=torch.float64))
    yd = dev(y)
    mean_o, invstd_o, rm_o, rv_o = Out(C), Out(C), Out(C, body=rm), Out(C, body=rv)
    sums = Out(hip.query("fs_bn_stats_scratch_doubles", M, C), torch.float64)
    hip.call("fs_bn_stats", hip.ptr(yd), M, C, MOM, EPS, rm_o.ptr, rv_o.ptr, mean_o.ptr, invstd_o.ptr, sums.ptr)
    e = _offset_errors(yd, M, C, mean_o, invstd_o, rm_o, rv_o, rm, rv)
    print(f"[offset] fs_bn_stats ratio {ratio}: normalised {e[0]:.3e} running_mean {e[1]:.3e} running_var {e[2]:.3e} var {e[3]:.3e}")
    if ratio == 10:
        assert e[0] <= 2e-5 and e[1] <= 1e-5 and e[2] <= 1e-5, e


@pytest.mark.parametrize("ratio", [10, 30, 100])
def test_conv_stats_offset_mean(ratio):
    """the same through the convolution epilogue: fs_conv2d_fwd_stats on a biased convolution -> fs_bn_finalize_slab"""
    gen = torch.Generator().manual_seed(100 + ratio)
    B, H, W, C = 4, 40, 40, 64
    M = B * H * W
    x = torch.randn(B, C, H, W, generator=gen)
    w = torch.randn(C, C, 3, 3, generator=gen) / 24.0
    y0 = F.conv2d(x.double(), w.double(), None, 1, 1)
    sign = choice(gen, [-1.0, 1.0], C)
    bias = (ratio * sign * y0.std(dim=(0, 2, 3)) - y0.mean(dim=(0, 2, 3))).float()
    rm, rv = f32(randn(gen, C) * 0.1), f32(1 + 0.1 * torch.rand(C, generator=gen, dtype=torch.float64))
    wd = ops.new_rsck_weight(C, C, 3, 3, device=DEV)
    wd.copy_(w)
    yd, slab, nwg = ops.conv2d_fwd_stats(x.permute(0, 2, 3, 1).contiguous().to(DEV), wd, bias.to(DEV), 1, 1)
    mean_o, invstd_o, rm_o, rv_o = Out(C), Out(C), Out(C, body=rm), Out(C, body=rv)
    hip.call("fs_bn_finalize_slab", hip.ptr(slab), nwg, M, C, MOM, EPS, rm_o.ptr, rv_o.ptr, mean_o.ptr, invstd_o.ptr)
    e = _offset_errors(yd.reshape(-1), M, C, mean_o, invstd_o, rm_o, rv_o, rm, rv)
    print(f"[offset] conv2d_fwd_stats ratio {ratio}: normalised {e[0]:.3e} running_mean {e[1]:.3e} running_var {e[2]:.3e} var {e[3]:.3e} ({nwg} slab rows)")
    if ratio == 10:
        assert e[0] <= 2e-5 and e[1] <= 1e-5 and e[2] <= 1e-5, e


# ================================================================================================
# Resize family
# ================================================================================================
def pow2(n):
    return n & (n - 1) == 0


def coord_term(th, tw, Ho, Wo, vmax):
    """Error of the fp32 source index s = (in / out) * (d + 0.5) - 0.5 where the factor is no power of two: three roundings at the
    magnitude of s + 0.5 <= in; the weight moves by as much, the output by at most that times |v0 - v1| <= 2 max|v|, per axis."""
    t = 0.0
    if not pow2(Ho // th):
        t += 3 * U * th * 2 * vmax
    if not pow2(Wo // tw):
        t += 3 * U * tw * 2 * vmax
    return t


def up_bound(src, Ho, Wo):
    """forward bound of one up-sampling: Ly.l0 * (Lx.l0 * v00 + Lx.l1 * v01) + Ly.l1 * (...): the weights carry one rounding each (1 - l1),
    then two products and one sum per level: 7 roundings on sum |w| |v|"""
    B, th, tw, C = src.shape
    Wm = R.upsample_matrix(th, tw, Ho, Wo).abs()
    b = 7 * U * torch.einsum("oq,bqc->boc", Wm, src.abs().reshape(B, th * tw, C)).reshape(B, Ho, Wo, C)
    return b + coord_term(th, tw, Ho, Wo, float(src.abs().max()))


#              B  C    th tw Ho  Wo  Cdst coff
SLICE_CASES = [(1, 4, 3, 5, 6, 20, 12, 4),           # factors 2 x 4
               (3, 36, 4, 6, 4, 48, 100, 32),        # 1 x 8
               (1, 132, 2, 3, 32, 3, 200, 68),       # 16 x 1
               (3, 4, 5, 2, 40, 32, 4, 0),           # 8 x 16, the whole buffer
               (1, 36, 7, 3, 14, 12, 36, 0),         # 2 x 4
               (3, 132, 3, 4, 6, 8, 136, 4),         # 2 x 2
               (1, 36, 4, 5, 12, 15, 40, 4),         # 3 x 3: forward only
               (3, 4, 3, 2, 9, 2, 8, 4)]             # 3 x 1: forward only


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("B,C,th,tw,Ho,Wo,Cdst,coff", SLICE_CASES)
def test_upsample_slice(B, C, th, tw, Ho, Wo, Cdst, coff, kind):
    fam = "resize"
    gen = torch.Generator().manual_seed(C + th * 10 + Wo)
    integer = kind == "int"
    fy, fx = Ho // th, Wo // tw
    src = randint(gen, -8, 8, B, th, tw, C) if integer else randn(gen, B, th, tw, C)
    # the destination: a sentinel in the channels that stay, NaN in the slice
    dst0 = torch.full((B, Ho, Wo, Cdst), 321.5, dtype=torch.float64)
    dst0[..., coff:coff + C] = float("nan")
    dst_o = Out(dst0.numel(), body=dst0)
    sd = dev(src)
    hip.call("fs_upsample_slice_fwd", hip.ptr(sd), B, th, tw, C, dst_o.ptr, Ho, Wo, Cdst, coff)
    got = dst_o.get().reshape(B, Ho, Wo, Cdst).double()
    keep = torch.ones(Cdst, dtype=torch.bool)
    keep[coff:coff + C] = False
    assert bool((got[..., keep] == 321.5).all()), "channels outside the slice were written"
    up_r = R.upsample(src, Ho, Wo)
    up_d = got[..., coff:coff + C]
    if integer and pow2(fy) and pow2(fx):          # weights are multiples of 1 / (4 fy fx): products and sums are exact
        exact(fam, "slice_fwd.int", up_d, up_r)
    else:
        check(fam, f"slice_fwd.{kind}", up_d, up_r, up_bound(src, Ho, Wo), R.upsample(src.float(), Ho, Wo))
    if fy == 3 or fx == 3:
        return

    # transpose
    g = randint(gen, -2, 2, B, Ho, Wo, Cdst) if integer else randn(gen, B, Ho, Wo, Cdst)
    gd = dev(g)
    ds_o = Out(B * th * tw * C)
    hip.call("fs_upsample_slice_bwd", hip.ptr(gd), B, Ho, Wo, Cdst, coff, ds_o.ptr, th, tw, C)
    ds_d = ds_o.get().reshape(B, th, tw, C).double()
    ds_r = R.upsample_slice_bwd(g, coff, C, th, tw)
    Wm = R.upsample_matrix(th, tw, Ho, Wo).abs()
    # up to (2 fy)(2 fx) terms added in sequence, each (wy * wx) * g with the roundings of the two weights and two products
    Lb = 4 * fy * fx + 4
    ds_b = Lb * U * torch.einsum("oq,boc->bqc", Wm, g[..., coff:coff + C].abs().reshape(B, Ho * Wo, C)).reshape(B, th, tw, C)
    if integer:
        exact(fam, "slice_bwd.int", ds_d, ds_r)
    else:
        check(fam, "slice_bwd", ds_d, ds_r, ds_b)
        # adjoint identity on the device results, in fp64: <up(x), g> = <x, up^T(g)>
        gs = g[..., coff:coff + C]
        lhs, rhs = float((up_d * gs).sum()), float((src * ds_d).sum())
        tol = float((up_bound(src, Ho, Wo) * gs.abs()).sum() + (ds_b * src.abs()).sum())
        report(fam, "adjoint", abs(lhs - rhs) / tol)
        assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)

    # the same gather plus the BatchNorm-backward sums of the layer whose output gradient it is (even factors only)
    if fy % 2 == 0 and fx % 2 == 0:
        M = B * th * tw
        # int: dsrc is a multiple of 1 / (4 fy fx) >= 2^-9 and a column's sum |dsrc| <= sum |g| <= 2 * 3 * 40 * 32 < 2^13, xhat in {-1, 0, 1}:
        # 22 bits, so the sums are exact
        yl = randint(gen, -1, 1, M, C) if integer else randn(gen, M, C)
        mean_in = torch.zeros(C, dtype=torch.float64) if integer else randn(gen, C)
        invstd_in = torch.ones(C, dtype=torch.float64) if integer else f32(0.5 + torch.rand(C, generator=gen, dtype=torch.float64))
        nslab = hip.query("fs_bn_bwd_slabs", M, C)
        ds2, slab_o = Out(M * C), Out(nslab * C * 2)
        yd, md, isd = dev(yl), dev(mean_in), dev(invstd_in)
        hip.call("fs_upsample_slice_bwd_bnsum", hip.ptr(gd), B, Ho, Wo, Cdst, coff, ds2.ptr, th, tw, C, hip.ptr(yd), hip.ptr(md), hip.ptr(isd), slab_o.ptr)
        if integer:
            exact(fam, "slice_bwd_bnsum.dsrc.int", ds2.get().reshape(B, th, tw, C).double(), ds_r)
        else:
            check(fam, "slice_bwd_bnsum.dsrc", ds2.get().reshape(B, th, tw, C), ds_r, ds_b)
        S_d, SX_d = slab_sums(slab_o.get(), nslab, C)
        ones = torch.ones(M, C, dtype=torch.bool)
        S_r, SX_r = R.bn_bwd_sums(ds_r.reshape(M, C), ones, yl, mean_in, invstd_in)          # the reference's own gradient and sums
        if integer:
            exact(fam, "slice_bwd_bnsum.S.int", S_d, S_r)
            exact(fam, "slice_bwd_bnsum.SX.int", SX_d, SX_r)
        else:
            L = chain_len(M, C)
            xa = ((yl - mean_in) * invstd_in).abs()
            da, db_ = ds_r.reshape(M, C).abs(), ds_b.reshape(M, C)
            check(fam, "slice_bwd_bnsum.S", S_d, S_r, L * U * da.sum(0) + db_.sum(0))
            check(fam, "slice_bwd_bnsum.SX", SX_d, SX_r, (L + 3) * U * (da * xa).sum(0) + (db_ * xa).sum(0))


#             B  C    Ho  Wo  term sizes                               relu
FUSE_CASES = [(1, 4, 8, 12, [(8, 12)], 0),
              (3, 36, 8, 12, [(8, 12), (4, 6)], 1),
              (1, 132, 16, 6, [(16, 6), (8, 6), (1, 3)], 1),                 # factors 2 x 1 and 16 x 2
              (3, 4, 16, 16, [(16, 16), (8, 4), (4, 2), (2, 1)], 1),         # 2 x 4, 4 x 8, 8 x 16
              (1, 36, 12, 6, [(4, 2), (12, 6)], 0),                          # factor 3, up-sampled term first
              (1, 4, 6, 9, [(2, 3)], 1),                                     # one term, factor 3
              (3, 132, 4, 10, [(4, 10), (4, 5), (2, 10), (1, 5)], 0)]        # factor 1 on one axis only


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("B,C,Ho,Wo,sizes,relu", FUSE_CASES)
def test_hr_fuse(B, C, Ho, Wo, sizes, relu, kind):
    fam = "resize"
    gen = torch.Generator().manual_seed(C + Ho + len(sizes))
    integer = kind == "int"
    terms = [randint(gen, -8, 8, B, h, w, C) if integer else randn(gen, B, h, w, C) for h, w in sizes]
    td = [dev(t) for t in terms]
    n = len(terms)
    out_o = Out(B * Ho * Wo * C)
    hip.call("fs_hr_fuse_fwd", (ctypes.c_void_p * n)(*[hip.ptr(t) for t in td]), (ctypes.c_int * n)(*[s[0] for s in sizes]),
             (ctypes.c_int * n)(*[s[1] for s in sizes]), n, out_o.ptr, B, Ho, Wo, C, relu)
    got = out_o.get().reshape(B, Ho, Wo, C).double()
    acc = R.hr_fuse_fwd(terms, Ho, Wo, 0)
    if integer and all(pow2(Ho // h) and pow2(Wo // w) for h, w in sizes):
        exact(fam, "hr_fuse.int", got, R.hr_fuse_fwd(terms, Ho, Wo, relu))
        return
    # each term's own bound, plus one rounding per addition of the terms
    bound = sum(up_bound(t, Ho, Wo) if t.shape[1:3] != (Ho, Wo) else torch.zeros(B, Ho, Wo, C, dtype=torch.float64) for t in terms)
    bound = bound + (n - 1) * U * sum((t if t.shape[1:3] == (Ho, Wo) else R.upsample(t.abs(), Ho, Wo)).abs() for t in terms)
    acc32 = R.hr_fuse_fwd([t.float() for t in terms], Ho, Wo, 0)
    if relu:          # the branch the device took; where it wrote 0 the reference sum may be positive by no more than the bound
        assert bool((got >= 0).all())
        assert bool((acc[got == 0] <= bound[got == 0]).all())
        acc, acc32 = torch.where(got > 0, acc, torch.zeros_like(acc)), torch.where(got > 0, acc32, torch.zeros_like(acc32))
    check(fam, f"hr_fuse.{kind}", got, acc, bound, acc32)


def test_resize_rejects():
    """a non-dividing size, an odd backward factor, a slice past the buffer: HipLibraryError, and nothing is written"""
    src = torch.zeros(1 * 3 * 4 * 4, device=DEV)
    g = torch.zeros(1 * 9 * 12 * 8, device=DEV)
    y = torch.zeros(3 * 4 * 4, device=DEV)
    v = torch.ones(4, device=DEV)
    for name, args in [
            ("fs_upsample_slice_fwd", lambda o: (hip.ptr(src), 1, 3, 4, 4, o.ptr, 7, 8, 8, 0)),            # 7 % 3 != 0
            ("fs_upsample_slice_fwd", lambda o: (hip.ptr(src), 1, 3, 4, 4, o.ptr, 6, 8, 8, 8)),            # coff + C > Cdst
            ("fs_upsample_slice_bwd", lambda o: (hip.ptr(g), 1, 9, 12, 8, 0, o.ptr, 3, 4, 4)),             # factor 3 backward
            ("fs_upsample_slice_bwd", lambda o: (hip.ptr(g), 1, 6, 8, 8, 8, o.ptr, 3, 4, 4)),              # coff + C > Cg
            ("fs_upsample_slice_bwd", lambda o: (hip.ptr(g), 1, 7, 8, 8, 0, o.ptr, 3, 4, 4)),              # 7 % 3 != 0
            ("fs_upsample_slice_bwd_bnsum", lambda o: (hip.ptr(g), 1, 9, 12, 8, 0, o.ptr, 3, 4, 4, hip.ptr(y), hip.ptr(v), hip.ptr(v), o.ptr)),
            ("fs_upsample_slice_bwd_bnsum", lambda o: (hip.ptr(g), 1, 3, 8, 8, 0, o.ptr, 3, 4, 4, hip.ptr(y), hip.ptr(v), hip.ptr(v), o.ptr))]:   # factor 1
        o = Out(1 * 9 * 12 * 8)
        with pytest.raises(hip.HipLibraryError):
            hip.call(name, *args(o))
        assert o.untouched(), name
    o = Out(7 * 8 * 4)
    with pytest.raises(hip.HipLibraryError):
        hip.call("fs_hr_fuse_fwd", (ctypes.c_void_p * 1)(hip.ptr(src)), (ctypes.c_int * 1)(3), (ctypes.c_int * 1)(4), 1, o.ptr, 1, 7, 8, 4, 0)
    assert o.untouched()


# ================================================================================================
# Pooling
# ================================================================================================
MAXPOOL_CFG = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0), (3, 2, 0)]


def maxpool_input(kind, gen, B, H, W, C):
    if kind == "random":
        return randn(gen, B, H, W, C)
    if kind == "tied":          # what follows a ReLU: exact zeros in most windows, few distinct values
        return randint(gen, -3, 2, B, H, W, C).clamp(min=0)
    if kind == "constant":
        return torch.full((B, H, W, C), 1.5, dtype=torch.float64)
    x = randn(gen, B, H, W, C)
    x[:, : H // 2 + 1] = -float("inf")          # whole windows of -inf
    if kind == "nan":
        x[0, H - 1, W - 2, 0] = float("nan")
        x[0, 0, 0, 0] = float("nan")
    return x


@pytest.mark.parametrize("i,ksp", list(enumerate(MAXPOOL_CFG)))
@pytest.mark.parametrize("H,W", [(10, 11), (7, 8)])
@pytest.mark.parametrize("kind", ["random", "tied", "constant", "neginf", "nan"])
def test_maxpool(i, ksp, H, W, kind):
    fam = "pooling"
    k, s, p = ksp
    C = (1, 3, 64)[(i + H) % 3]
    B = 1 + (i + H) % 2
    gen = torch.Generator().manual_seed(i * 10 + H)
    x = maxpool_input(kind, gen, B, H, W, C)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xd = dev(x)
    out_o, arg_o = Out(B * Ho * Wo * C, fill=-4321.5), Out(B * Ho * Wo * C, torch.int32)          # NaN is a legitimate output here
    hip.call("fs_maxpool_fwd", hip.ptr(xd), out_o.ptr, arg_o.ptr, B, H, W, C, Ho, Wo, k, s, p)
    out_r, arg_r = R.maxpool_fwd(x, k, s, p)
    out_d, arg_d = out_o.get().double().reshape(out_r.shape), arg_o.get().reshape(arg_r.shape)
    exact(fam, "maxpool.arg", arg_d, arg_r)
    assert torch.equal(torch.isnan(out_d), torch.isnan(out_r))
    exact(fam, "maxpool.out", torch.nan_to_num(out_d, nan=0.0), torch.nan_to_num(out_r, nan=0.0))
    # backward from the device's arg, integer-valued gradients: exact
    dout = randint(gen, -8, 8, B, Ho, Wo, C)
    dd = dev(dout)
    dx_o = Out(B * H * W * C)
    hip.call("fs_maxpool_bwd", hip.ptr(dd), arg_o.ptr, dx_o.ptr, B, H, W, C, Ho, Wo, k, s, p)
    dx_d = dx_o.get().double().reshape(B, H, W, C)
    exact(fam, "maxpool.dx", dx_d, R.maxpool_bwd(dout, arg_d, H, W))
    assert float(dx_d.sum()) == float(dout.sum())
    if (k, s, p) == (3, 3, 0) and (H, W) == (10, 11):          # row 9 and columns 9, 10 lie in no window
        assert float(dx_d[:, 9].abs().max()) == 0 and float(dx_d[:, :, 9:].abs().max()) == 0


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("B,HW,C", [(1, 1, 1), (5, 37, 51), (1, 100, 512), (5, 100, 1), (1, 37, 512), (5, 1, 51)])
def test_avgpool(B, HW, C, kind):
    fam = "pooling"
    gen = torch.Generator().manual_seed(HW + C)
    integer = kind == "int"
    x = randint(gen, -8, 8, B, HW, C) if integer else randn(gen, B, HW, C)
    d = randint(gen, -8, 8, B, C) if integer else randn(gen, B, C)
    xd, dd = dev(x), dev(d)
    out_o, dx_o = Out(B * C), Out(B * HW * C)
    hip.call("fs_avgpool_fwd", hip.ptr(xd), B, HW, C, out_o.ptr)
    hip.call("fs_avgpool_bwd", hip.ptr(dd), B, HW, C, dx_o.ptr)
    if integer:          # the sum is exact and the one division is correctly rounded
        exact(fam, "avgpool.out.int", out_o.get(), R.avgpool_fwd(x).float())
    else:                # HW - 1 additions in sequence and the division
        check(fam, "avgpool.out", out_o.get(), R.avgpool_fwd(x), HW * U * x.abs().sum(1) / HW)
    exact(fam, f"avgpool.dx.{kind}", dx_o.get().reshape(B, HW, C), R.avgpool_bwd(d, HW).float())          # one correctly rounded division


# ================================================================================================
# Head tail
# ================================================================================================
def mask_head_ppb():
    """pixels per workgroup of the mask-head backward, read through its scratch query: (C + 1) floats per workgroup"""
    n = 1
    while hip.query("fs_mask_head_bwd_scratch_floats", n, 4) == 5:
        n += 1
        assert n < (1 << 16)
    return n - 1


def mask_head_npix(tag):
    return {"one": 1, "three": 3, "ppb-1": mask_head_ppb() - 1, "ppb+1": mask_head_ppb() + 1, "map": 12800}[tag]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("C,tag", [(4, "one"), (4, "ppb+1"), (4, "map"), (240, "three"), (240, "map"), (256, "ppb-1"), (256, "ppb+1"),
                                   (260, "one"), (260, "ppb-1"), (260, "map"), (1024, "three"), (1024, "ppb+1")])
def test_mask_head(C, tag, kind):
    fam = "head"
    npix = mask_head_npix(tag)
    ppb = mask_head_ppb()
    gen = torch.Generator().manual_seed(C + npix)
    integer = kind == "int"
    if integer:          # m = 0: s (1 - s) = 1/4 and dm a multiple of 4, so dlogit is an integer; |dlogit x| <= 18, 12 800 pixels: < 2^24
        x, w, bias = randint(gen, -3, 3, npix, C), randint(gen, -2, 2, C), torch.zeros(1, dtype=torch.float64)
        m_in, dm = torch.zeros(npix, dtype=torch.float64), 4 * randint(gen, -6, 6, npix)
    else:
        x, w, bias = randn(gen, npix, C), f32(randn(gen, C) / C ** 0.5), randn(gen, 1)
        m_in, dm = f32(R.mask_head_fwd(x, w, bias)), randn(gen, npix)
    xd, wd, bd = dev(x), dev(w), dev(bias)
    m_o = Out(npix)
    hip.call("fs_mask_head_fwd", hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), m_o.ptr, npix, C)
    m_r = R.mask_head_fwd(x, w, bias)
    # per lane ceil(C / 256) float4 dot products of 4 products and 4 additions, six shuffle stages, the bias: L roundings on sum |x w| + |b|;
    # sigmoid' <= 1/4; expf (2 ulp), the reciprocal, 1 + e and - 0.5 at magnitude <= 1 add 6 U
    Lf = 8 * -(-C // 256) + 6 + 1
    bl = Lf * U * ((x.abs() * w.abs()).sum(1) + bias.abs())
    check(fam, f"mask_head.fwd.{kind}", m_o.get(), m_r, 0.25 * bl + 6 * U, R.mask_head_fwd(x.float(), w.float(), bias.float()))

    md, dmd = dev(m_in), dev(dm)
    nscr = hip.query("fs_mask_head_bwd_scratch_floats", npix, C)
    dx_o, dw_o, db_o, scr = Out(npix * C), Out(C), Out(1), Out(nscr)
    hip.call("fs_mask_head_bwd", hip.ptr(dmd), hip.ptr(md), hip.ptr(xd), hip.ptr(wd), dx_o.ptr, dw_o.ptr, db_o.ptr, npix, C, scr.ptr)
    scr.get()
    dx_r, dw_r, db_r = R.mask_head_bwd(dm, m_in, x, w)
    if integer:
        exact(fam, "mask_head.dx.int", dx_o.get().double(), dx_r)
        exact(fam, "mask_head.dw.int", dw_o.get().double(), dw_r)
        exact(fam, "mask_head.db.int", db_o.get().double(), db_r)
    else:
        s = m_in + 0.5
        dl = (dm * s * (1 - s)).abs()
        # dlogit = dm * s * (1 - s).  s = m + 0.5 is rounded once (U s); 1 - s inherits that error absolutely, which is NOT small beside 1 - s
        # near saturation: d(s (1 - s)) = |1 - 2 s| ds <= U s.  The subtraction and the two products add 3 U s (1 - s).
        dl_b = dm.abs() * (U * s.abs() + 3 * U * (s * (1 - s)).abs())
        check(fam, "mask_head.dx", dx_o.get().reshape(npix, C), dx_r, (dl_b + U * dl)[:, None] * w.abs()[None, :],
              R.mask_head_bwd(dm.float(), m_in.float(), x.float(), w.float())[0])
        # per wave ppb / 4 pixels in sequence, the 4 waves, then the workgroups' records (in sequence, or 64 lanes + a shuffle tree)
        nblk = -(-npix // ppb)
        L = ppb // 4 + 3 + nblk
        check(fam, "mask_head.dw", dw_o.get(), dw_r, torch.einsum("p,pc->c", dl_b + (L + 1) * U * dl, x.abs()))
        check(fam, "mask_head.db", db_o.get(), db_r, (dl_b + L * U * dl).sum().reshape(1))


def test_mask_head_saturates_and_rejects():
    gen = torch.Generator().manual_seed(1)
    npix, C = 64, 240
    x, w = randn(gen, npix, C), f32(randn(gen, C) / C ** 0.5)
    logit = torch.linspace(-100, 100, npix, dtype=torch.float64)
    x = f32(x * (logit / (x @ w))[:, None])          # logits from -100 to 100
    m_o = Out(npix)
    xd, wd, bd = dev(x), dev(w), dev(torch.zeros(1))
    hip.call("fs_mask_head_fwd", hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), m_o.ptr, npix, C)
    m = m_o.get().double()
    lr = x @ w
    assert bool(torch.isfinite(m).all()) and float(m.abs().max()) <= 0.5
    assert bool((m[lr > 30] == 0.5).all()) and bool((m[lr < -30] == -0.5).all())
    check("head", "mask_head.saturated", m, R.mask_head_fwd(x, w, torch.zeros(1, dtype=torch.float64)),
          0.25 * 15 * U * (x.abs() * w.abs()).sum(1) + 6 * U)
    # 1028 channels: rejected by both entry points, nothing written
    big = torch.zeros(4 * 1028, device=DEV)
    o, o2, o3, scr = Out(4 * 1028), Out(1028), Out(1), Out(4 * 1029)
    with pytest.raises(hip.HipLibraryError):
        hip.call("fs_mask_head_fwd", hip.ptr(big), hip.ptr(big), hip.ptr(big), o.ptr, 4, 1028)
    with pytest.raises(hip.HipLibraryError):
        hip.call("fs_mask_head_bwd", hip.ptr(big), hip.ptr(big), hip.ptr(big), hip.ptr(big), o.ptr, o2.ptr, o3.ptr, 4, 1028, scr.ptr)
    assert o.untouched() and o2.untouched() and o3.untouched() and scr.untouched()


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("B,K,HW", [(1, 2, 1), (3, 2, 6400), (3, 51, 255), (1, 51, 257), (1, 150, 6400), (3, 150, 1), (1, 2, 257),
                                    (3, 150, 255), (3, 51, 6400)])
def test_pred_assemble(B, K, HW, kind):
    fam = "head"
    gen = torch.Generator().manual_seed(K + HW)
    integer = kind == "int"
    cls = randint(gen, -4, 4, B, K) if integer else randn(gen, B, K)
    m = randint(gen, -2, 2, B, HW) if integer else f32(torch.rand(B, HW, generator=gen, dtype=torch.float64) - 0.5)
    dp = randint(gen, -8, 8, B, K, HW) if integer else randn(gen, B, K, HW)
    cd, md, dpd = dev(cls), dev(m), dev(dp)
    pred_o, dcls_o, dm_o = Out(B * K * HW), Out(B * K), Out(B * HW)
    hip.call("fs_pred_assemble_fwd", hip.ptr(cd), hip.ptr(md), pred_o.ptr, B, K, HW)
    hip.call("fs_pred_assemble_bwd", hip.ptr(dpd), hip.ptr(cd), hip.ptr(md), dcls_o.ptr, dm_o.ptr, B, K, HW)
    exact(fam, "pred_assemble.fwd", pred_o.get().reshape(B, K, HW), R.pred_assemble_fwd(cls, m).float())          # copies and one product
    dcls_r, dm_r = R.pred_assemble_bwd(dp, cls, m)
    exact(fam, "pred_assemble.dm", dm_o.get().reshape(B, HW), dm_r.float())                                        # one product
    if integer:          # |dpred m| <= 16, 6400 pixels
        exact(fam, "pred_assemble.dcls.int", dcls_o.get().double(), dcls_r)
    else:                # per thread ceil(HW / 256) terms, six shuffle stages, four waves, one product each
        L = -(-HW // 256) + 6 + 4 + 1
        terms = dp.abs().sum(2)
        terms[:, K - 1] = (dp[:, K - 1].abs() * m.abs()).sum(1)
        check(fam, "pred_assemble.dcls", dcls_o.get().reshape(B, K), dcls_r, L * U * terms)


# ================================================================================================
# Adam
# ================================================================================================
ARENA = 4096 * 256 * 4 + 4096 + 4          # more float4 groups than the 4096 x 256 threads of the grid: the stride loop runs twice


@pytest.mark.parametrize("n,step,gs,wd", [(4, 1, 1.0, 0.0), (4, 100000, 0.5, 1e-4), (1020, 2, 0.5, 0.0), (1020, 1000, 1.0, 1e-4),
                                          (1048580, 1, 0.5, 1e-4), (1048580, 1000, 1.0, 0.0), (ARENA, 2, 1.0, 1e-4),
                                          (ARENA, 100000, 0.5, 0.0)])
def test_adam(n, step, gs, wd):
    fam = "adam"
    gen = torch.Generator().manual_seed(n % 1000 + step)
    lr, b1, b2, eps = 2e-5, 0.9, 0.999, 1e-8
    p = randn(gen, n)
    g = f32(randn(gen, n) * 10.0 ** torch.randint(-4, 2, (n,), generator=gen).double())
    m = f32(randn(gen, n) * 0.1) if step > 1 else torch.zeros(n, dtype=torch.float64)
    v = f32(torch.rand(n, generator=gen, dtype=torch.float64) * 1e-2) if step > 1 else torch.zeros(n, dtype=torch.float64)
    third = n // 3
    g[:third] = f32(g[:third] * 1e-9)          # v ~ 0: eps dominates the denominator
    v[:third] = f32(v[:third] * 1e-18)
    m[:third] = f32(m[:third] * 1e-9)
    v[third:2 * third] = f32(v[third:2 * third] * 1e6)          # large v
    p_o, m_o, v_o = Out(n, body=p), Out(n, body=m), Out(n, body=v)
    gd = dev(g)
    hip.call("fs_adam_step", p_o.ptr, hip.ptr(gd), m_o.ptr, v_o.ptr, n, lr, b1, b2, eps, wd, step, gs)
    p_r, m_r, v_r = R.adam_step(p, g, m, v, lr, b1, b2, eps, wd, step, gs)
    p32, m32, v32 = R.adam_step(p.float(), g.float(), m.float(), v.float(), lr, b1, b2, eps, wd, step, gs)
    # the forward error of every line of the kernel, in its order (the scalars are the fp32 values the ABI carries):
    lr_, b1_, b2_, eps_, wd_, gs_ = (float(np.float32(a)) for a in (lr, b1, b2, eps, wd, gs))
    bc1, bc2s = 1 - b1_ ** step, math.sqrt(1 - b2_ ** step)
    gg = g * gs_ + wd_ * p
    dgg = 3 * U * ((g * gs_).abs() + (wd_ * p).abs())                                   # g * gs, wd * p, their sum
    dm = 3 * U * ((b1_ * m).abs() + ((1 - b1_) * gg).abs()) + (1 - b1_) * dgg           # two products and a sum, plus the error of g'
    dv = 4 * U * ((b2_ * v).abs() + (1 - b2_) * gg * gg) + (1 - b2_) * 2 * gg.abs() * dgg
    check(fam, "m", m_o.get(), m_r, dm, m32)
    check(fam, "v", v_o.get(), v_r, dv, v32)
    sq = torch.sqrt(v_r)
    denom = sq / bc2s + eps_
    # sqrt is infinitely steep at 0 (there its error is at most sqrt(dv)), elsewhere it takes dv / sqrt(v) at most; its own rounding,
    # the division by the fp32 correction (its rounding and the quotient's) and the sum with eps
    dsq = torch.where(v_r > 4 * dv, dv / sq.clamp_min(1e-300), torch.sqrt(dv))          # sqrt(v) - sqrt(v - dv) <= dv / sqrt(v) there
    # The host forms the bias corrections in fp32: 1.f - powf(b, t).  powf is accurate to 1 ulp (2 U relative, the C library's stated
    # bound), the subtraction cancels: a relative error of 2 U b^t / (1 - b^t) + U of 1 - b^t; exact at t = 1 (1.f - b is exact for
    # b in [1/2, 1]), 6e-5 for b2 = 0.999 at t = 2, gone for large t.  The square root halves it and adds its own rounding.
    rel1 = (2 * U * b1_ ** step / bc1 + U) if step > 1 else 0.0
    rel2s = (0.5 * (2 * U * b2_ ** step / bc2s ** 2 + U) if step > 1 else 0.0) + U
    dden = (dsq + 3 * U * sq) / bc2s + rel2s * sq / bc2s + U * denom
    upd = (lr_ / bc1) * (m_r / denom)
    # m / denom, step_size = lr / fp32(bc1) and their product: 4 roundings; then p - update rounds at the magnitude of p
    dupd = upd.abs() * (dm / m_r.abs().clamp_min(1e-300) + dden / denom + 4 * U + rel1) + U * p.abs()
    dupd = torch.where(m_r == 0, (lr_ / bc1) * dm / denom + U * p.abs(), dupd)
    got_upd = p_o.get().double() - p
    check(fam, "update", got_upd, p_r - p, dupd, p32.double() - p)
