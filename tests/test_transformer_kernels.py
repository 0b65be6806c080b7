"""The SegFormer kernels (csrc/transformer.hip, csrc/attention_split.hip) at the C ABI against the plain fp64 references of
oracle/transformer_ref.py (which tests/test_transformer_ref.py holds to torch on the CPU).

The rules are those of tests/test_elementwise_kernels.py (helpers shared through tests/kernel_testing.py):
  * every output, scratch-sized buffer and in-place target is an `Out`: guards of GUARD floats of sentinel on both sides, the
    body pre-filled with NaN (an integer marker / a visible integer pattern for in-place targets); after the call no fill
    value is left where an output is due and the guards are untouched;
  * two kinds of data: "int" -- small integers and powers of two, every sum below 2^24, BIT-EQUAL to the reference wherever the
    expression is exact in fp32; "float" -- random data held to the forward error bound L * 2^-24 * sum|terms| of the
    expression, L = the kernel's longest fp32 chain, derived in the comment beside each check; for the pointwise passes the
    bound or 4x the error of the same formula evaluated in fp32 by torch on the CPU, whichever is larger (`check` with ref32:
    GELU only; every reduction -- LayerNorm, dwconv3, fold, attention -- is held to its derived bound alone).
    No bound is taken from what a kernel returns;
  * no element is left out of a comparison; each stage gets clean inputs (reference values rounded to fp32), never the
    previous stage's device output.  The attention backward entry points get lse, D and o of the fp64 reference rounded to
    fp32; the rounding of those inputs is a term of the bound (u |lse| on P, u |D| on dS);
  * the float constants of the ABI (eps, drop scale, threshold, attention scale 0.125) are formed as transformer.hip forms them
    (transformer_ref.abi_float / drop_scale / drop_thresh).

Split-precision (bf16x3) attention: an operand is x = x1 + x2 + x3 exactly (three bf16 planes, |x2| <= 2^-8 |x|,
|x3| <= 2^-16 |x|; conv_split.h), six of the nine plane products are kept: the dropped x2 y3 + x3 y2 + x3 y3 is at most
(2^-24 + 2^-24 + 2^-32) |x y| < 3 u |x y| per product, and a contraction step accumulates six partial products instead of
one.  Both enter L beside the checks (SPLIT_TERM, chain * 6).  The derived bound holds for these kernels as it stands: no
emulated fallback scale is used.

Every check prints `[bound] family what ratio`: the largest error as a fraction of its bound (profiles/r10/README.md).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fovealseg  # noqa: E402
import fovealseg_oracle as O  # noqa: E402
import transformer_ref as R  # noqa: E402
from kernel_testing import GUARD, U, Out, check, choice, dev, exact, f32, randint, randn, report  # noqa: E402,F401

hip = fovealseg.hip
HipError = fovealseg.hip.HipLibraryError
DEV = "cuda"
EPS = R.abi_float(1e-6)          # nn.LayerNorm(eps=1e-6) of the Mix-Transformer, as the C ABI carries it: float
SCALE = 0.125                    # 1 / sqrt(head_dim 64)
TINY = 2.0 ** -126               # below the normal range fp32 arithmetic promises no relative accuracy (a flush to zero is allowed)
ERF_ULPS, EXP_ULPS, LOG_ULPS = 16, 4, 4      # accuracy of erff / expf (exp2f) / logf the OpenCL C specification grants a device library
GRID_CAP = 4096 * 256 * 4        # floats one sweep of the capped grid covers (4096 blocks x 256 threads x float4)


def cdiv(a, b):
    return -(-a // b)


def pattern(n):
    """a visible integer pattern for in-place targets: an add shows exactly"""
    return ((torch.arange(n) % 7) - 3).double()


def key_with_both(nsamp, p, seed):
    """a layer key under which `nsamp` samples hold kept AND dropped ones (chosen from the hash oracle on the CPU)"""
    for lid in range(1, 200):
        key = O.layer_key(seed, lid)
        m = R.keep_mask(nsamp, key, p)
        if p == 0 or nsamp < 2 or (bool(m.any()) and not bool(m.all())):
            return key
    raise AssertionError("no key found")


def rejected(name, *args):
    with pytest.raises(HipError, match="rejected"):
        hip.call(name, *args)


# ================================================================================================
# LayerNorm
# ================================================================================================
def ln_form(C):
    """(float4s per lane NJ, lanes per row) of the forward / backward kernel that runs C channels"""
    need = cdiv(C, 64)
    return (1, 16) if need <= 1 else (2, 16) if need <= 2 else (5, 16) if need <= 5 else (8, 64)


def ln_bwd_plan(M, C):
    """(rows per workgroup, workgroups) of the backward kernels, read off ln_bwd_plan in csrc/transformer.hip"""
    if cdiv(C, 64) <= 5:
        rpb = max(cdiv(cdiv(M, 2048), 16) * 16, 16)
    else:
        rpb = max(cdiv(M, 1024), 4)
    return rpb, cdiv(M, rpb)


def ln_row_chain(C):
    """fp32 additions behind one row sum: 4 NJ per lane, then log2(lanes per row) shuffle steps"""
    nj, lanes = ln_form(C)
    return 4 * nj + int(math.log2(lanes))


def ln_col_chain(M, C):
    """fp32 additions behind one column sum: rows per lane, the wave's four groups (16-lane form), the four waves, then the
    block records: ceil(nblk / 64) per lane + 6 shuffle steps + the accumulate"""
    rpb, nblk = ln_bwd_plan(M, C)
    per_lane = cdiv(rpb, 16) + 2 if ln_form(C)[1] == 16 else cdiv(rpb, 4)
    return per_lane + 3 + cdiv(nblk, 64) + 6 + 1


LN_C = [4, 64, 68, 128, 132, 320, 324, 512, 2048]
LN_CASES = [(C, M) for C in LN_C for M in (1, 3, 15, 16, 17, 111)]
LN_CASES += [(C, 4099) for C in (4, 64, 132, 324, 512, 2048)] + [(64, 40003), (320, 40003)]
# one M on each side of a rows_per_block step: narrow rows 16 -> 32 at M = 2048 * 16, wide rows 4 -> 5 at M = 4 * 1024
LN_CASES += [(64, 32768), (64, 32769), (512, 4096), (512, 4097)]


def ln_data(gen, M, C, kind, offset=0.0):
    if kind == "int":        # rows of +-a in equal numbers (mean exactly 0), g and the addend small integers: column sums of g < 2^24
        a = choice(gen, [1.0, 2.0, 4.0], M, 1)
        sign = torch.ones(M, C, dtype=torch.float64)
        sign[:, torch.randperm(C, generator=gen)[:C // 2]] = -1.0
        x = a * sign * (1 - 2 * torch.randint(0, 2, (M, 1), generator=gen).double())
        gamma, beta = choice(gen, [0.5, 1.0, 2.0], C), randint(gen, -2, 2, C)
        g, addend = randint(gen, -4, 4, M, C), randint(gen, -4, 4, M, C)
    else:
        sigma = f32(0.5 + torch.rand(M, 1, generator=gen, dtype=torch.float64))
        x = f32(randn(gen, M, C) * sigma + (randn(gen, M, 1) if offset == 0 else offset * sigma))
        gamma, beta = f32(1 + 0.1 * randn(gen, C)), f32(0.1 * randn(gen, C))
        g, addend = randn(gen, M, C), randn(gen, M, C)
    return x, gamma, beta, g, addend


def ln_forward_check(fam, tag, x, gamma, beta, kind):
    M, C = x.shape
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    y_o, mean_o, rstd_o = Out(M * C), Out(M), Out(M)
    hip.call("fs_layernorm_fwd", hip.ptr(xd), hip.ptr(gd), hip.ptr(bd), y_o.ptr, mean_o.ptr, rstd_o.ptr, M, C, EPS)
    y_r, mean_r, rstd_r = R.layernorm_fwd(x, gamma, beta, EPS)
    Ls = ln_row_chain(C)
    d = x - mean_r[:, None]
    var = (d * d).sum(-1) / C
    # mean = (sum of C terms, chain Ls) / C: (Ls + 1) roundings on sum|x| / C, one more for the quotient
    dmean = (Ls + 2) * U * x.abs().sum(-1) / C
    # two-pass variance about the computed mean: sum (d - dmean)^2 = sum d^2 + C dmean^2 exactly (sum d = 0), so the mean's error
    # enters squared; d is rounded (2 u d^2), squared (u), summed (Ls), divided (1): (Ls + 5) u var
    dvar = dmean ** 2 + (Ls + 5) * U * var
    # rstd = rsqrtf(var + eps): d(v^-1/2) = v^-3/2 / 2 on (dvar + the rounding of the sum), rsqrtf to 2 ulp = 4 u
    drstd = 0.5 * rstd_r ** 3 * (dvar + U * (var + EPS)) + 4 * U * rstd_r
    # y = ((x - mu) rs) gamma + beta: the errors of mu and rs through the product, three roundings on |xhat gamma|, one on y
    xh = d * rstd_r[:, None]
    dy = gamma.abs() * (rstd_r[:, None] * (dmean[:, None] + U * d.abs()) + d.abs() * drstd[:, None]) + 3 * U * (xh * gamma).abs() + U * y_r.abs()
    mean_d = mean_o.get()
    check(fam, f"{tag}.mean", mean_d, mean_r, dmean + TINY)
    check(fam, f"{tag}.rstd", rstd_o.get(), rstd_r, drstd)
    check(fam, f"{tag}.y", y_o.get(), y_r, dy + TINY)
    if kind == "int":
        exact(fam, f"{tag}.mean.int", mean_d, torch.zeros(M))          # +-a in equal numbers: the row sum is exactly 0
    return mean_r, rstd_r


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("C,M", LN_CASES)
def test_layernorm(C, M, kind):
    fam = "layernorm"
    gen = torch.Generator().manual_seed(C * 13 + M)
    x, gamma, beta, g, addend = ln_data(gen, M, C, kind)
    mean_r, rstd_r = ln_forward_check(fam, f"fwd.{kind}", x, gamma, beta, kind)

    # ---- backward: clean mean / rstd (the reference's, rounded to fp32) ----------------------------------------------------------
    mean_c, rstd_c = f32(mean_r), f32(rstd_r)
    rpb, nblk = ln_bwd_plan(M, C)
    nscr = hip.query("fs_layernorm_bwd_scratch_floats", M, C)
    assert nscr == 2 * nblk * C, "the test's row plan is not the library's"
    dx_r, dg_r, db_r = R.layernorm_bwd(g, x, gamma, mean_c, rstd_c)
    Ls, Lc = ln_row_chain(C), ln_col_chain(M, C)
    xh = (x - mean_c[:, None]) * rstd_c[:, None]
    gg = g * gamma
    m1, m2 = gg.sum(-1, keepdim=True) / C, (gg * xh).sum(-1, keepdim=True) / C
    # m1 = sum(g gamma) / C: product, chain Ls, quotient; m2 = sum(g gamma xhat) / C: xhat carries 2 roundings, two products
    dm1 = (Ls + 2) * U * gg.abs().sum(-1, keepdim=True) / C
    dm2 = (Ls + 5) * U * (gg * xh).abs().sum(-1, keepdim=True) / C
    # dx = rs (gg - m1 - xhat m2): u on gg, the errors of m1 and m2, 3 u on xhat m2 (xhat's two, the product), the two
    # subtractions (2 u on each term), the product with rs (u |dx|)
    ddx = rstd_c[:, None] * (3 * U * gg.abs() + dm1 + 2 * U * m1.abs() + xh.abs() * dm2 + 5 * U * (xh * m2).abs()) + U * dx_r.abs() + TINY
    # dgamma = column sum of g xhat (3 roundings per term, chain Lc); dbeta = column sum of g (chain Lc)
    ddg = (Lc + 3) * U * (g * xh).abs().sum(0) + TINY
    ddb = Lc * U * g.abs().sum(0) + TINY
    xd, gmd, gd, md, rd, ad = dev(x), dev(gamma), dev(g), dev(mean_c), dev(rstd_c), dev(addend)
    prior_g, prior_b = pattern(C), pattern(C).flip(0)
    plain = None
    for acc, use_add in ((0, False), (1, True), (1, False), (0, True)):
        dx_o, scr = Out(M * C), Out(nscr)
        dg_o = Out(C, body=prior_g) if acc else Out(C)
        db_o = Out(C, body=prior_b) if acc else Out(C)
        if use_add:
            hip.call("fs_layernorm_bwd_add", hip.ptr(gd), hip.ptr(xd), hip.ptr(gmd), hip.ptr(md), hip.ptr(rd), hip.ptr(ad), dx_o.ptr, dg_o.ptr,
                     db_o.ptr, M, C, acc, scr.ptr)
        else:
            hip.call("fs_layernorm_bwd", hip.ptr(gd), hip.ptr(xd), hip.ptr(gmd), hip.ptr(md), hip.ptr(rd), dx_o.ptr, dg_o.ptr, db_o.ptr, M, C,
                     acc, scr.ptr)
        scr.get(complete=True)          # every record of the scratch is written (and nothing beyond it)
        tag = f"bwd.{kind}.acc{acc}.add{int(use_add)}"
        dx_d, dg_d, db_d = dx_o.get(), dg_o.get(), db_o.get()
        if use_add:          # the addend costs one rounding of the sum ...
            check(fam, f"{tag}.dx", dx_d, dx_r + addend, ddx + U * (dx_r + addend).abs())
            # ... and is exactly that: the plain pass's dx plus the addend, rounded once
            assert plain is not None and torch.equal(dx_d, plain + addend.float().reshape(-1)), f"{fam} {tag}: dx != plain dx + addend"
        else:
            check(fam, f"{tag}.dx", dx_d, dx_r, ddx)
            if plain is None:
                plain = dx_d.clone()
            else:
                assert torch.equal(dx_d, plain), f"{fam} {tag}: dx depends on accumulate"
        pg, pb = (prior_g, prior_b) if acc else (0.0, 0.0)          # accumulate: one more rounding of the sum with the prior contents
        check(fam, f"{tag}.dgamma", dg_d, dg_r + pg, ddg + acc * U * (dg_r + pg).abs())
        check(fam, f"{tag}.dbeta", db_d, db_r + pb, ddb + acc * U * (db_r + pb).abs())
        if kind == "int":          # column sums of small integers (+ an integer pattern): exact in any order
            exact(fam, f"{tag}.dbeta.int", db_d, db_r + pb)


@pytest.mark.parametrize("ratio", [10.0, 100.0])
@pytest.mark.parametrize("C,M", [(64, 111), (132, 17), (320, 4099), (512, 15), (2048, 16)])
def test_layernorm_offset_mean(C, M, ratio):
    """|row mean| / sigma = 10 and 100: the two-pass variance keeps the derived bound (the mean's error enters the variance squared;
    y carries rstd * dmean, which grows with the offset -- that term is in the bound, the bound is not widened)"""
    gen = torch.Generator().manual_seed(C + M + int(ratio))
    x, gamma, beta, _, _ = ln_data(gen, M, C, "float", offset=ratio)
    ln_forward_check("layernorm", f"offset{int(ratio)}.C{C}", x, gamma, beta, "float")


def test_layernorm_rejects():
    M, C = 5, 64
    gen = torch.Generator().manual_seed(1)
    x, gamma, beta, g, _ = ln_data(gen, M, 2052, "float")
    xd, gd, bd, gg = dev(x), dev(gamma), dev(beta), dev(g)
    for Cbad in (6, 66, 2052):          # C % 4 != 0, C > 2048
        y_o, mean_o, rstd_o = Out(M * Cbad), Out(M), Out(M)
        rejected("fs_layernorm_fwd", hip.ptr(xd), hip.ptr(gd), hip.ptr(bd), y_o.ptr, mean_o.ptr, rstd_o.ptr, M, Cbad, EPS)
        assert y_o.untouched() and mean_o.untouched() and rstd_o.untouched()
        dx_o, dg_o, db_o, scr = Out(M * Cbad), Out(Cbad), Out(Cbad), Out(2 * Cbad)
        rejected("fs_layernorm_bwd", hip.ptr(gg), hip.ptr(xd), hip.ptr(gd), mean_o.ptr, rstd_o.ptr, dx_o.ptr, dg_o.ptr, db_o.ptr, M, Cbad, 0, scr.ptr)
        assert dx_o.untouched() and dg_o.untouched() and db_o.untouched() and scr.untouched()
    dx_o, dg_o, db_o, m_o, r_o = Out(M * C), Out(C), Out(C), Out(M, body=torch.zeros(M)), Out(M, body=torch.ones(M))
    rejected("fs_layernorm_bwd", hip.ptr(gg), hip.ptr(xd), hip.ptr(gd), m_o.ptr, r_o.ptr, dx_o.ptr, dg_o.ptr, db_o.ptr, M, C, 0, None)      # null scratch
    rejected("fs_layernorm_bwd_add", hip.ptr(gg), hip.ptr(xd), hip.ptr(gd), m_o.ptr, r_o.ptr, hip.ptr(xd), dx_o.ptr, dg_o.ptr, db_o.ptr, M, C, 1, None)
    assert dx_o.untouched() and dg_o.untouched() and db_o.untouched()


# ================================================================================================
# GELU, GELU + dropout
# ================================================================================================
GELU_N = [4, 1028, GRID_CAP, GRID_CAP + 4, 9_000_000]


def gelu_input(gen, n):
    special = torch.tensor([0.0, -0.0, 30.0, -30.0, 2.0 ** -126, -2.0 ** -126, 1.5 * 2.0 ** -126, -12.0], dtype=torch.float64)
    if n == 4:
        return torch.tensor([-0.0, 30.0, -30.0, -2.0 ** -126], dtype=torch.float64)
    grid = f32(torch.linspace(-12.0, 12.0, min(n - 8, 96001) // 4 * 4 - 0, dtype=torch.float64))
    rest = n - 8 - grid.numel()
    x = torch.cat([special[:4], grid, special[4:], 2 * randn(gen, rest)])
    assert x.numel() == n
    return x


@pytest.mark.parametrize("n", GELU_N)
def test_gelu(n):
    fam = "gelu"
    blocks = cdiv(n // 4, 256)
    if n > GRID_CAP:
        assert blocks > 4096, "this case must lie beyond the grid cap (the grid-stride loop runs a second sweep)"
    elif n == GRID_CAP:
        assert blocks == 4096
    gen = torch.Generator().manual_seed(n % 1000 + 7)
    x, g = gelu_input(gen, n), randn(gen, n)
    xd, gd = dev(x), dev(g)
    y_r, dx_r = R.gelu_fwd(x), R.gelu_bwd(g, x)
    y32, dx32 = R.gelu_fwd(x.float()), R.gelu_bwd(g.float(), x.float())
    # y = (0.5 x) (1 + erff(x c)): erff to ERF_ULPS ulp of a value <= 1 (2 u each), the rounding of x c through erf' (max of
    # 2/sqrt(pi) z exp(-z^2) 2 u < u), the sum 1 + erf (u (1 + erf) <= 2 u): |d(1 + erf)| <= (2 ERF_ULPS + 3) u in BOTH tails --
    # an absolute error 0.5 |x| (2 ERF_ULPS + 3) u where the negative tail's value is far below it; the product: u |y|
    cerf = 2 * ERF_ULPS + 3
    by = 0.5 * x.abs() * cerf * U + U * y_r.abs() + TINY
    # gelu'(x) = cdf + x pdf: cdf as above (halved); pdf = c expf(-0.5 x x): the argument carries 2 u |a|, a = x^2 / 2, expf
    # 2 EXP_ULPS u, the constant and the product 2 u: pdf (x^2 + 2 EXP_ULPS + 2) u; the sum and the product with g: 2 u |dx|
    pdf = R.gelu_pdf(x)
    bgrad = 0.5 * cerf * U + x.abs() * pdf * (x * x + 2 * EXP_ULPS + 3) * U + U * R.gelu_grad(x).abs()
    bdx = g.abs() * bgrad + 2 * U * dx_r.abs() + TINY
    y_o, dx_o = Out(n), Out(n)
    hip.call("fs_gelu_fwd", hip.ptr(xd), y_o.ptr, n)
    hip.call("fs_gelu_bwd", hip.ptr(gd), hip.ptr(xd), dx_o.ptr, n)
    y_d = y_o.get()
    neg, pos = x < -4, x > 4
    check(fam, f"fwd.n{n}", y_d, y_r, by, y32)
    if bool(neg.any()):
        check(fam, f"fwd.n{n}.negative_tail", y_d[neg], y_r[neg], by[neg], y32[neg])
        check(fam, f"fwd.n{n}.positive_tail", y_d[pos], y_r[pos], by[pos], y32[pos])
    check(fam, f"bwd.n{n}", dx_o.get(), dx_r, bdx, dx32)
    zero = x == 0
    assert bool((y_d[zero] == 0).all()) and bool((y_d[x == 30.0] == 30.0).all())

    # ---- with the dropout behind it ------------------------------------------------------------------------------------------------
    p, key = 0.2, O.layer_key(11, 5)
    scale = R.drop_scale(p)
    keep = R.keep_mask(n, key, p)
    if n > 4:
        assert bool(keep.any()) and not bool(keep.all())
    yd_o, dxd_o = Out(n), Out(n)
    hip.call("fs_gelu_dropout_fwd", hip.ptr(xd), yd_o.ptr, n, p, key)
    hip.call("fs_gelu_dropout_bwd", hip.ptr(gd), hip.ptr(xd), dxd_o.ptr, n, p, key)
    yd_d, dxd_d = yd_o.get(), dxd_o.get()
    # dropped elements are exactly 0; the zero pattern is the hash's, ANDed with "the device GELU is not 0" (at x ~ -5.5 the last
    # ulp of erff decides between -0 and -1.6e-7: the zero-ness of gelu(x) is the DEVICE's)
    assert bool((yd_d[~keep] == 0).all()) and bool((dxd_d[~keep] == 0).all()), f"{fam}: a dropped element is not 0"
    assert torch.equal(yd_d != 0, keep & (y_d != 0)), f"{fam}: the zero pattern is not the hash's"
    # kept elements: the GELU result times the fp32 drop scale, one rounding
    assert torch.equal(yd_d[keep], (y_d * np.float32(scale))[keep]), f"{fam}: kept != gelu * drop scale"
    check(fam, f"dropout.fwd.n{n}", yd_d, R.gelu_dropout_fwd(x, p, key), scale * by + U * scale * y_r.abs(), R.gelu_dropout_fwd(x.float(), p, key))
    # backward: (g scale) rounded, then the same factor
    check(fam, f"dropout.bwd.n{n}", dxd_d, R.gelu_dropout_bwd(g, x, p, key), scale * bdx + U * scale * dx_r.abs(), R.gelu_dropout_bwd(g.float(), x.float(), p, key))


def test_gelu_rejects():
    x = dev(torch.zeros(8))
    y_o = Out(8)
    rejected("fs_gelu_fwd", hip.ptr(x), y_o.ptr, 6)
    rejected("fs_gelu_dropout_fwd", hip.ptr(x), y_o.ptr, 8, 0.0, 5)
    rejected("fs_gelu_dropout_fwd", hip.ptr(x), y_o.ptr, 8, 1.0, 5)
    assert y_o.untouched()


# ================================================================================================
# depthwise 3x3
# ================================================================================================
DW_RY, DW_SEG = 4, 16          # output rows / columns per thread (csrc/transformer.hip)
_DW_HW = [(H, W) for H in (1, 3, 4, 5, 9) for W in (1, 15, 16, 17, 33)]
_DW_C, _DW_B = (4, 64, 256, 1280), (1, 3)
# every (H, W) pair twice, C and B cycling so that every value meets every H and every W; (accumulate_w, accumulate_b) cycle too
DW_CASES = [(B, H, W, C, (i + j) % 2, ((i + j) // 2) % 2)
            for i, (H, W) in enumerate(_DW_HW)
            for j, (C, B) in enumerate([(_DW_C[i % 4], _DW_B[(i // 4) % 2]), (_DW_C[(i + 2) % 4], _DW_B[(i // 4 + 1) % 2])])]
DW_CASES += [(2, 80, 160, 1024, 1, 0)]          # lanes < items: a lane walks several items


def dw_data(gen, B, H, W, C, kind):
    if kind == "int":          # |x|, |dy| <= 4, |w|, |bias| <= 3: sum |x dy| <= 16 * 25 600 pixels < 2^24
        return (randint(gen, -4, 4, B, H, W, C), randint(gen, -3, 3, C, 9), randint(gen, -3, 3, C), randint(gen, -4, 4, B, H, W, C))
    return randn(gen, B, H, W, C), f32(0.3 * randn(gen, C, 9)), f32(0.1 * randn(gen, C)), randn(gen, B, H, W, C)


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("B,H,W,C,acc_w,acc_b", DW_CASES)
def test_dwconv3(B, H, W, C, acc_w, acc_b, kind):
    fam = "dwconv3"
    gen = torch.Generator().manual_seed(B * 1000 + H * 100 + W + C)
    x, w, bias, dy = dw_data(gen, B, H, W, C, kind)
    xd, wd, bd, dyd = dev(x), dev(w), dev(bias), dev(dy)
    n = B * H * W * C
    tag = f"{kind}.{B}x{H}x{W}x{C}"
    items = B * cdiv(H, DW_RY) * cdiv(W, DW_SEG)
    lanes = hip.query("fs_dwconv3_wgrad_lanes", B, H, W, C)
    assert 1 <= lanes <= items
    if C == 1024:
        assert lanes < items, "this case must give a lane more than one item"

    # ---- forward (bias / no bias) and the input gradient (flip) -------------------------------------------------------------------------
    outs = {}
    for name, src, srcd, b_, bd_, flip in (("fwd.bias", x, xd, bias, bd, 0), ("fwd.nobias", x, xd, None, None, 0), ("flip", dy, dyd, None, None, 1)):
        y_o = Out(n)
        hip.call("fs_dwconv3_fwd", hip.ptr(srcd), hip.ptr(wd), hip.ptr(bd_), y_o.ptr, B, H, W, C, flip)
        ref = R.dwconv3_fwd(src, w, b_, bool(flip))
        got = outs[name] = y_o.get()
        if kind == "int":
            exact(fam, f"{name}.{tag}", got, ref)
        else:
            # acc = bias, then 9 products (u each) added one after the other (9 roundings), two more for the grouping by rows: 11 u
            # on |bias| + sum |w| |x|
            absum = R.dwconv3_fwd(src.abs(), w.abs(), None if b_ is None else b_.abs(), bool(flip))
            check(fam, f"{name}.{tag}", got, ref, 11 * U * absum + TINY)
    if kind == "int":          # <dwconv(x), dy> = <x, dwconv_flip(dy)> on the device results, exactly
        lhs, rhs = float((outs["fwd.nobias"].double() * dy.reshape(-1)).sum()), float((x.reshape(-1) * outs["flip"].double()).sum())
        assert lhs == rhs, f"{fam} {tag}: adjoint identity {lhs} != {rhs}"

    # ---- weight / bias gradients: ten-plane form, nine-plane form -----------------------------------------------------------------------
    dw_r, db_r = R.dwconv3_bwd_weight(x, dy), R.dwconv3_bwd_bias(dy)
    prior_w, prior_b = pattern(9 * C).reshape(C, 9), pattern(C)
    ws10, ws9 = Out(lanes * 10 * C), Out(lanes * 9 * C)
    dw_o = Out(9 * C, body=prior_w) if acc_w else Out(9 * C)
    db_o = Out(C, body=prior_b) if acc_b else Out(C)
    hip.call("fs_dwconv3_bwd_weight_bias", hip.ptr(xd), hip.ptr(dyd), dw_o.ptr, db_o.ptr, ws10.ptr, B, H, W, C, acc_w, acc_b)
    dw9_o = Out(9 * C, body=prior_w) if acc_w else Out(9 * C)
    hip.call("fs_dwconv3_bwd_weight", hip.ptr(xd), hip.ptr(dyd), dw9_o.ptr, ws9.ptr, B, H, W, C, acc_w)
    ws10.get(), ws9.get()          # every slab row written, nothing beyond
    dw_d, db_d, dw9_d = dw_o.get(), db_o.get(), dw9_o.get()
    want_w = dw_r + (prior_w if acc_w else 0)
    want_b = db_r + (prior_b if acc_b else 0)
    assert torch.equal(dw_d, dw9_d), f"{fam} {tag}: the nine- and ten-plane forms differ in dw"
    if kind == "int":
        exact(fam, f"dw.{tag}", dw_d, want_w)
        exact(fam, f"db.{tag}", db_d, want_b)
    else:
        # a lane adds ceil(items / lanes) items of up to DW_RY * DW_SEG = 64 pixels each into one register (one product rounding per
        # term), the reduce kernel adds ceil(lanes / 8) slab rows per thread, the 8 row groups (7) and the prior contents (1)
        L = cdiv(items, lanes) * DW_RY * DW_SEG + 1 + cdiv(lanes, 8) + 8
        check(fam, f"dw.{tag}.acc{acc_w}", dw_d, want_w, L * U * (R.dwconv3_bwd_weight(x.abs(), dy.abs()) + acc_w * prior_w.abs()) + TINY)
        check(fam, f"db.{tag}.acc{acc_b}", db_d, want_b, L * U * (dy.abs().sum((0, 1, 2)) + acc_b * prior_b.abs()) + TINY)


# ================================================================================================
# residual + DropPath, and the one-pass backward of DropPath(Dropout(.))
# ================================================================================================
#            n            per_sample    (sample boundaries: inside every float4 pair of a block / inside one 256-thread block's 1024 floats /
DP_CASES = [(48, 4),      #              at block multiples / inside one grid stride, n on both sides of the grid cap)
            (1200, 100),
            (3840, 640),
            (GRID_CAP, GRID_CAP // 8),
            (GRID_CAP + 96, 100),
            (5_000_000, 1_000_000)]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("with_x", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("n,per_sample", DP_CASES)
def test_residual_droppath(n, per_sample, p, with_x, kind):
    fam = "droppath"
    assert n % per_sample == 0
    if n > GRID_CAP:
        assert cdiv(n // 4, 256) > 4096, "this case must lie beyond the grid cap"
    if per_sample == 100:
        assert 1024 % per_sample != 0          # boundaries fall inside a block's 1024 floats, at changing places
    if per_sample == 1_000_000:
        assert per_sample < GRID_CAP < 5 * per_sample and GRID_CAP % per_sample != 0          # a boundary inside a grid stride
    gen = torch.Generator().manual_seed(n % 977 + per_sample)
    nsamp = n // per_sample
    key = key_with_both(nsamp, p, 2)
    x, y = (randint(gen, -8, 8, n), randint(gen, -8, 8, n)) if kind == "int" else (randn(gen, n), randn(gen, n))
    xd, yd = dev(x), dev(y)
    out_o = Out(n)
    hip.call("fs_residual_droppath", hip.ptr(xd) if with_x else None, hip.ptr(yd), out_o.ptr, n, per_sample, p, key)
    got = out_o.get()
    ref = R.residual_droppath(x if with_x else None, y, per_sample, p, key)
    tag = f"{kind}.n{n}.ps{per_sample}.p{p}.x{int(with_x)}"
    keep = R.droppath_factor(n, per_sample, p, key)
    # dropped samples: exactly x (exactly 0 without x)
    exact(fam, f"dropped.{tag}", got[~keep], (x if with_x else torch.zeros(n, dtype=torch.float64))[~keep])
    if kind == "int" and p == 0:          # scale 1: x + y of small integers
        exact(fam, f"kept.{tag}", got, ref)
    # kept samples: y * scale rounded (exact for p = 0), then the add rounded: u |y scale| + u |out|
    check(fam, f"kept.{tag}", got, ref, U * (y * R.drop_scale(p)).abs() + U * ref.abs() + TINY)

    # ---- the fused backward = fs_residual_droppath(x = NULL) followed by fs_dropout, bit for bit -----------------------------------------------
    if not with_x:
        for drop_p in (0.0, 0.3):
            dkey = O.layer_key(5, 17)
            dz_o, t_o, dz2_o = Out(n), Out(n), Out(n)
            hip.call("fs_droppath_dropout_bwd", hip.ptr(yd), dz_o.ptr, n, per_sample, p, key, drop_p, dkey)
            hip.call("fs_residual_droppath", None, hip.ptr(yd), t_o.ptr, n, per_sample, p, key)
            t_d = t_o.get()
            if drop_p > 0:
                hip.call("fs_dropout", hip.ptr(t_o.t), dz2_o.ptr, n, drop_p, dkey)
                two = dz2_o.get()
            else:
                two = t_d
            dz_d = dz_o.get()
            assert torch.equal(dz_d, two), f"{fam} {tag}: the fused backward differs from the two passes (dropout {drop_p})"
            ref2 = R.droppath_dropout_bwd(y, per_sample, p, key, drop_p, dkey)
            dkeep = R.keep_mask(n, dkey, drop_p) & keep
            exact(fam, f"bwd.dropped.{tag}.d{drop_p}", dz_d[~dkeep], torch.zeros(n, dtype=torch.float64)[~dkeep])
            # two products, each rounded once
            check(fam, f"bwd.{tag}.d{drop_p}", dz_d, ref2, 2 * U * ref2.abs() + TINY)


def test_residual_droppath_rejects():
    y = dev(torch.zeros(16))
    o = Out(16)
    rejected("fs_residual_droppath", None, hip.ptr(y), o.ptr, 16, 6, 0.0, 1)
    rejected("fs_residual_droppath", None, hip.ptr(y), o.ptr, 14, 4, 0.0, 1)
    rejected("fs_droppath_dropout_bwd", hip.ptr(y), o.ptr, 16, 4, 1.0, 1, 0.0, 2)
    assert o.untouched()


# ================================================================================================
# unfold / fold
# ================================================================================================
#               k  stride pad C   Kp      general kernels: C % 4 != 0, padding, overlap, or Kp > k k C
UNFOLD_FORMS = [(7, 4, 3, 3, 148), (7, 1, 3, 3, 148), (3, 2, 1, 5, 48), (8, 8, 0, 6, 384), (2, 2, 0, 64, 260),
                # patch kernels: stride = k, no padding, C % 4 == 0, Kp = k k C
                (8, 8, 0, 64, 4096), (4, 4, 0, 64, 1024), (2, 2, 0, 320, 1280), (1, 1, 0, 4, 4)]
UNFOLD_SIZES = [(2, 23, 17), (1, 22, 18), (3, 9, 33)]          # odd sizes; 22 x 18 leaves rows and columns outside every 4 x 4 / 8 x 8 patch


@pytest.mark.parametrize("B,H,W", UNFOLD_SIZES)
@pytest.mark.parametrize("k,stride,pad,C,Kp", UNFOLD_FORMS)
def test_unfold_fold(k, stride, pad, C, Kp, B, H, W):
    fam = "unfold"
    gen = torch.Generator().manual_seed(k * 100 + stride * 10 + C + H)
    Ho, Wo = R.out_size(H, k, stride, pad), R.out_size(W, k, stride, pad)
    rows = B * Ho * Wo
    patch_form = stride == k and pad == 0 and C % 4 == 0 and Kp == k * k * C
    assert patch_form == (Kp in (4096, 1024, 1280, 4))
    tag = f"k{k}s{stride}p{pad}C{C}.{B}x{H}x{W}"
    uncovered = R.fold(torch.ones(rows, Kp, dtype=torch.float64), B, H, W, C, k, stride, pad) == 0
    if (H, W) == (22, 18) and stride == k and k in (4, 8):
        assert bool(uncovered.any()), "this size must leave pixels outside every patch"
    for kind in ("int", "float"):
        x = randint(gen, -9, 9, B, H, W, C) if kind == "int" else randn(gen, B, H, W, C)
        col = randint(gen, -9, 9, rows, Kp) if kind == "int" else randn(gen, rows, Kp)
        col_o, dx_o = Out(rows * Kp), Out(B * H * W * C)
        hip.call("fs_unfold", hip.ptr(dev(x)), col_o.ptr, B, H, W, C, k, stride, pad, Ho, Wo, Kp)
        hip.call("fs_fold", hip.ptr(dev(col)), dx_o.ptr, B, H, W, C, k, stride, pad, Ho, Wo, Kp)
        # unfold is data movement: bit-equal on any data, the padding columns and the out-of-image taps exactly 0
        col_d = col_o.get()
        exact(fam, f"unfold.{kind}.{tag}", col_d, R.unfold(x, k, stride, pad, Kp))
        assert bool((col_d.reshape(rows, Kp)[:, k * k * C:] == 0).all())
        dx_d, dx_r = dx_o.get(), R.fold(col, B, H, W, C, k, stride, pad)
        assert bool((dx_d.reshape(uncovered.shape)[uncovered] == 0).all()), f"{fam} {tag}: a pixel no patch reaches is not 0"
        if kind == "int" or patch_form:          # sums of small integers; one term per pixel in the patch form
            exact(fam, f"fold.{kind}.{tag}", dx_d, dx_r)
        else:          # at most ceil(k / stride)^2 terms reach a pixel, added one after the other
            check("fold", f"fold.{kind}.{tag}", dx_d, dx_r, cdiv(k, stride) ** 2 * U * R.fold(col.abs(), B, H, W, C, k, stride, pad) + TINY)
        if kind == "int":          # <unfold(x), c> = <x, fold(c)> on the device results, exactly
            assert float((col_d.double() * col.reshape(-1)).sum()) == float((x.reshape(-1) * dx_d.double()).sum())


def test_unfold_fold_reject_wrong_sizes():
    B, H, W, C, k, stride, pad = 1, 9, 11, 3, 7, 4, 3
    Ho, Wo, Kp = R.out_size(H, k, stride, pad), R.out_size(W, k, stride, pad), 148
    x = dev(torch.zeros(B, H, W, C))
    col_o, dx_o = Out(B * (Ho + 1) * (Wo + 1) * (Kp + 4)), Out(B * H * W * C)
    col = dev(torch.zeros(B * (Ho + 1) * (Wo + 1) * (Kp + 4)))
    for ho, wo, kp in ((Ho + 1, Wo, Kp), (Ho, Wo - 1, Kp), (Ho, Wo, 147), (Ho, Wo, 144), (Ho, Wo, 150)):
        rejected("fs_unfold", hip.ptr(x), col_o.ptr, B, H, W, C, k, stride, pad, ho, wo, kp)
        rejected("fs_fold", hip.ptr(col), dx_o.ptr, B, H, W, C, k, stride, pad, ho, wo, kp)
    assert col_o.untouched() and dx_o.untouched()


# ================================================================================================
# attention: the exact-fp32 MFMA family and the bf16x3 family
# ================================================================================================
KC, QS = 64, 32
SPLIT_TERM = 3          # u |x y| per product of the bf16x3 arithmetic: the three dropped plane products (file header)

#              B  heads  N    Nk    p       every N in {1, 31, 32, 33, 127, 128, 129, 1600} and Nk in {1, 7, 31, 32, 33, 63, 64, 65, 100,
ATTN_SHAPES = [(1, 1, 1, 1, 0.0),          # 127, 128, 129, 400} occurs, each shape runs in both families
               (3, 2, 31, 7, 0.2),
               (1, 5, 32, 31, 0.0),
               (1, 8, 33, 32, 0.2),
               (3, 1, 127, 33, 0.2),
               (1, 2, 128, 63, 0.2),
               (1, 1, 129, 64, 0.0),
               (1, 2, 1600, 65, 0.2),
               (3, 5, 33, 100, 0.2),
               (1, 1, 31, 127, 0.0),
               (1, 2, 129, 128, 0.2),
               (1, 1, 127, 129, 0.2),
               (1, 2, 1600, 400, 0.2),
               (2, 2, 33, 1, 0.0)]          # one key: P = 1 exactly, o = v bit for bit
REGIME_SHAPES = [(1, 2, 33, 129, 0.0), (1, 1, 129, 100, 0.2), (3, 2, 127, 65, 0.0)]          # last chunk partly filled in all three
REGIMES = ["rise", "fall", "same_keys", "offset80", "offset100", "dominant"]
ATTN_CASES = [(s, "randn") for s in ATTN_SHAPES] + [(s, r) for r in REGIMES for s in REGIME_SHAPES]


def attn_data(gen, B, heads, N, Nk, regime):
    C = heads * 64
    q, k, v, go = randn(gen, B, N, C), randn(gen, B, Nk, C), randn(gen, B, Nk, C), randn(gen, B, N, C)
    ones = torch.ones(C, dtype=torch.float64)
    if regime in ("rise", "fall"):
        # scores = 0.125 * (3.75 * 8 * 8) t_j = 30 t_j with t from -1 to 1 along the keys (rise) or back (fall): the running maximum
        # moves by ~30 per 64-key chunk, alpha = exp(m - m_new) is far from 1 in every chunk
        t = torch.linspace(-1.0, 1.0, Nk, dtype=torch.float64) * (1 if regime == "rise" else -1)
        q = 3.75 * ones + 0.3 * q
        k = t[None, :, None] * ones + 0.3 * k
    elif regime == "same_keys":          # P = 1 / Nk exactly, o = the mean of v
        k = k[:, :1].expand(B, Nk, C).clone()
    elif regime in ("offset80", "offset100"):          # every score ~ 0.125 * 64 a b = +80 / +100: exp overflows fp32 unless the maximum is subtracted
        q = (5.0 if regime == "offset80" else 6.25) * ones + 0.2 * q
        k = 2.0 * ones + 0.2 * k
    elif regime == "dominant":
        # query 0 picks the LAST key (in the partly filled last chunk), query 1 the first: score 0.125 * 3.75 |k|^2 ~ 30 against N(0, 3.75^2)
        q = q.clone()
        q[:, 0] = 3.75 * k[:, Nk - 1]
        if N > 1:
            q[:, 1] = 3.75 * k[:, 0]
    return f32(q), f32(k), f32(v), go


def heads_of(t, heads):
    return R._heads(t, heads)


class AttnRef:
    """the fp64 reference of one case and the error terms every bound is made of"""

    def __init__(self, q, k, v, go, heads, p, key, split):
        self.B, self.N, _ = q.shape
        self.Nk, self.heads, self.p, self.key, self.split = k.shape[1], heads, p, key, split
        self.S, self.P, self.M, lse = R.attention_parts(q, k, v, heads, SCALE, p, key)
        self.lse = lse.reshape(-1)
        self.o, _ = R.attention_fwd(q, k, v, heads, SCALE, p, key)
        self.dq, self.dk, self.dv = R.attention_bwd(q, k, v, go, heads, SCALE, p, key)
        self.D = R.attention_rowdot(go, self.o, heads)
        qh, kh, vh, gh = (heads_of(t, heads) for t in (q, k, v, go))
        self.qh, self.kh, self.vh, self.gh = qh, kh, vh, gh
        nchunk = cdiv(self.Nk, KC)
        mult = 6 if split else 1          # partial products accumulated per contraction step
        term = SPLIT_TERM if split else 0
        # S = sum over 64 head-dim products, accumulated in fp32 one after the other (q * 0.125 is exact; the split family scales by
        # 0.125 log2 e: the constant and the product, 2 roundings, and works in base-2 units: one more on the way back)
        self.Ld = 64 * mult + term + (3 if split else 1)
        A = torch.einsum("bhnd,bhkd->bhnk", qh.abs(), kh.abs()) * SCALE
        dS = self.Ld * U * A
        m = self.S.amax(-1, keepdim=True)
        rng = m - self.S.amin(-1, keepdim=True)
        # p_j = exp(S_j - m_run) rescaled by alpha = exp(m_old - m_new) once per chunk: the subtraction u |S_j - m|, the exponentials
        # 2 EXP_ULPS u each, the rescales' arguments add up to at most the row's score range, two products per chunk
        self.e = dS + U * ((m - self.S) + rng) + (2 * EXP_ULPS + 2) * (nchunk + 1) * U
        # l = sum of the p_j: their relative errors weighted by P, plus the chain: 32 per chunk per lane (split) or the 5-step tree
        # + 2 (fp32 family), + the cross-half add and the rescale per chunk
        self.E = (self.P * self.e).sum(-1, keepdim=True) + (34 * nchunk + 2) * U
        # o = (sum_j p~_j v_j) / l: chain over the keys of every chunk (64 nchunk steps, six partials each in the split family), the
        # drop scale, the reciprocal and the product with it
        self.Lo = 64 * nchunk * mult + term + 4
        self.Lq = self.Lo          # dq = sum_j dS_j k_j: the same chain over the keys
        # dk, dv: chain over the queries: the fp32 family adds a wave's 32 rows per 128-query block, then 4 waves, then the query
        # splits (<= 64, atomics in any order); the split family adds 32-query slices one after the other, then <= 8 partial tensors
        nq = 128 * cdiv(self.N, 128)
        self.Lk = (nq * 6 + SPLIT_TERM + 8 + 3) if split else (nq // 4 + 3 + 64 + 1)

    def bound_lse(self):
        # lse = m + log l: the relative error of l, logf to LOG_ULPS ulp, the sum (and the split family's two unit conversions)
        return self.E.squeeze(-1).reshape(-1) + (2 * LOG_ULPS + 4) * U * (self.lse.abs() + self.S.amax(-1).reshape(-1).abs() + 1.0)

    def bound_o(self):
        w = (self.P * self.M).abs() * (self.e + self.E + self.Lo * U)
        return R._tokens(torch.einsum("bhnk,bhkd->bhnd", w, self.vh.abs())) + TINY

    def backward_bounds(self, d_on_device):
        """bounds of dq, dk, dv when lse (and D, unless the entry point forms it from o and dO) are the reference's rounded to fp32"""
        P, M = self.P, self.M
        lse = self.lse.reshape(self.B, self.heads, self.N, 1)
        D = self.D.reshape(self.B, self.heads, self.N, 1)
        A = torch.einsum("bhnd,bhkd->bhnk", self.qh.abs(), self.kh.abs()) * SCALE
        # p = exp(S - lse): the chain of S, the subtraction, the exponential, and the fp32 rounding of the lse that is handed in
        # (the split family also converts it to base-2 units: the constant and the product, two more roundings)
        # (the split kernels start the score's accumulator at -lse log2 e: the partial sums, and with them the chain's roundings, are
        # bounded by A + |lse| there)
        ep = self.Ld * U * (A + (lse.abs() if self.split else 0.0)) + U * (self.S - lse).abs() + 2 * EXP_ULPS * U + (3 if self.split else 1) * U * lse.abs() + 2 * U
        G = torch.einsum("bhnd,bhkd->bhnk", self.gh.abs(), self.vh.abs())
        dPt = torch.einsum("bhnd,bhkd->bhnk", self.gh, self.vh)
        # D as handed in: rounded once; formed on the device from o (rounded to fp32: u |o|) and dO: 4 products + adds per lane,
        # 4 shuffle steps: 9 u on sum |dO o|
        dD = U * D.abs()
        if d_on_device:
            dD = dD + 10 * U * (self.gh.abs() * heads_of(self.o, self.heads).abs()).sum(-1, keepdim=True)
        # dS = p (M dP~ - D) scale: the chain of dP~ (same length as S's), dD, the relative error of p on every term, 5 roundings
        T = P * ((M * dPt).abs() + D.abs()) * SCALE
        ds_err = SCALE * P * (M * self.Ld * U * G + dD) + (ep + 5 * U) * T
        dSabs = (P * (M * dPt - D) * SCALE).abs()
        bq = torch.einsum("bhnk,bhkd->bhnd", ds_err + self.Lq * U * dSabs, self.kh.abs())
        bk = torch.einsum("bhnk,bhnd->bhkd", ds_err + self.Lk * U * dSabs, self.qh.abs())
        bv = torch.einsum("bhnk,bhnd->bhkd", (P * M) * (ep + (self.Lk + 2) * U), self.gh.abs())
        return R._tokens(bq) + TINY, R._tokens(bk) + TINY, R._tokens(bv) + TINY


def keep_words(B, heads, N, Nk, key, p):
    """the keep decisions as fs_attention_fwd_split leaves them: row (b heads + h) N + q, word key >> 5, bit key & 31 (bits of keys >= Nk: 0 here)"""
    nword = cdiv(Nk, 32)
    keep = R.keep_mask(B * heads * N * Nk, key, p).reshape(B * heads * N, Nk).numpy()
    bits = np.zeros((B * heads * N, nword * 32), dtype=np.uint64)
    bits[:, :Nk] = keep
    words = (bits.reshape(-1, nword, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32)


def fp32_dkv_splits(B, heads, N, Nk):
    """query ranges per key chunk of the fp32 dK / dV launch outside deterministic mode (attention_bwd_impl, csrc/transformer.hip)"""
    nkc, nqb = cdiv(Nk, KC), cdiv(N, 128)
    nsplit = min(cdiv(512, nkc * B * heads), nqb, 64)
    return cdiv(nqb, cdiv(nqb, nsplit))


def split_kv_splits(B, heads, N, Nk):
    """attn_kv_splits of csrc/attention_split.hip"""
    base, nslice = cdiv(Nk, 128) * B * heads, cdiv(N, QS)
    best, nsplit = 1e30, 1
    for c in range(1, min(8, nslice) + 1):
        cost = cdiv(base * c, 512) * cdiv(nslice, c) + 0.25 * c
        if cost < best:
            best, nsplit = cost, c
    return cdiv(nslice, cdiv(nslice, nsplit))


def attn_id(case):
    (B, heads, N, Nk, p), regime = case
    return f"{regime}-B{B}h{heads}N{N}Nk{Nk}p{p}"


@pytest.mark.parametrize("case", ATTN_CASES, ids=attn_id)
def test_attention_fp32(case):
    (B, heads, N, Nk, p), regime = case
    fam = "attention.f32"
    tag = attn_id(case)
    gen = torch.Generator().manual_seed(N * 131 + Nk * 7 + heads)
    q, k, v, go = attn_data(gen, B, heads, N, Nk, regime)
    key = O.layer_key(7, 70)
    ref = AttnRef(q, k, v, go, heads, p, key, split=False)
    C, rows = heads * 64, B * heads * N
    qd, kd, vd, god = dev(q), dev(k), dev(v), dev(go)
    o_o, lse_o = Out(B * N * C), Out(rows)
    hip.call("fs_attention_fwd", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), o_o.ptr, lse_o.ptr, B, N, Nk, heads, SCALE, p, key)
    check(fam, f"o.{tag}", o_o.get(), ref.o, ref.bound_o())
    check(fam, f"lse.{tag}", lse_o.get(), ref.lse, ref.bound_lse())
    if Nk == 1 and p == 0:          # P = exp(0) / 1 = 1: o = 1 * v, one exact product per element
        exact(fam, f"o.one_key.{tag}", o_o.get(), R._tokens(heads_of(v, heads).expand(B, heads, N, 64)))
    if regime == "same_keys" and p == 0:          # P = 1 / Nk: o is the mean of v, lse = S + log Nk
        mean_v = heads_of(v, heads).mean(2, keepdim=True).expand(B, heads, N, 64)
        check(fam, f"o.mean_of_v.{tag}", o_o.get(), R._tokens(mean_v), ref.bound_o())

    # ---- backward from clean o, lse (the reference's, rounded to fp32); D is formed on the device -------------------------------------
    od, lsed = dev(f32(ref.o)), dev(f32(ref.lse))
    bq, bk, bv = ref.backward_bounds(d_on_device=True)
    if N in (129, 1600) and regime == "randn":
        assert fp32_dkv_splits(B, heads, N, Nk) > 1, "this case must split the query range of the dK / dV launch"
    results = []
    try:
        for det in (0, 1, 1):          # default (atomics where the query range is split), then deterministic mode twice: the nsplit = 1 form
            hip.set_deterministic(bool(det))
            dq_o, dk_o, dv_o, scr = Out(B * N * C), Out(B * Nk * C), Out(B * Nk * C), Out(rows)
            hip.call("fs_attention_bwd", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), hip.ptr(od), hip.ptr(god), hip.ptr(lsed), dq_o.ptr, dk_o.ptr,
                     dv_o.ptr, scr.ptr, B, N, Nk, heads, SCALE, p, key)
            got = (dq_o.get(), dk_o.get(), dv_o.get())
            check(fam, f"D.det{det}.{tag}", scr.get(), ref.D, 10 * U * (ref.gh.abs() * heads_of(f32(ref.o), heads).abs()).sum(-1).reshape(-1) + U * ref.D.abs() + TINY)
            check(fam, f"dq.det{det}.{tag}", got[0], ref.dq, bq)
            check(fam, f"dk.det{det}.{tag}", got[1], ref.dk, bk)
            check(fam, f"dv.det{det}.{tag}", got[2], ref.dv, bv)
            results.append(got)
    finally:
        hip.set_deterministic(False)
    for a, b_ in zip(results[1], results[2]):
        assert torch.equal(a, b_), f"{fam} {tag}: deterministic mode is not bit-reproducible"
    assert torch.equal(results[0][0], results[1][0]), f"{fam} {tag}: dq depends on the mode"
    if N == 1600:
        # 13 query ranges meet in atomics by default, deterministic mode adds all 13 blocks in one chain (nsplit = 1): another
        # association of 1600 terms per element, so the bits of dk / dv must differ somewhere -- if they do not, the default launch
        # no longer splits (or deterministic mode no longer changes it) and this case has lost what it is for
        assert not (torch.equal(results[0][1], results[1][1]) and torch.equal(results[0][2], results[1][2])), \
            f"{fam} {tag}: default and deterministic dk / dv are bit-identical: the query range was not split"


@pytest.mark.parametrize("case", ATTN_CASES, ids=attn_id)
def test_attention_split(case):
    (B, heads, N, Nk, p), regime = case
    fam = "attention.bf16x3"
    tag = attn_id(case)
    gen = torch.Generator().manual_seed(N * 131 + Nk * 7 + heads)
    q, k, v, go = attn_data(gen, B, heads, N, Nk, regime)
    key = O.layer_key(7, 70)
    ref = AttnRef(q, k, v, go, heads, p, key, split=True)
    C, rows = heads * 64, B * heads * N
    qd, kd, vd, god = dev(q), dev(k), dev(v), dev(go)

    # ---- forward, with the keep words --------------------------------------------------------------------------------------------------
    nw = hip.query("fs_attention_mask_words", B, N, Nk, heads)
    assert nw == rows * cdiv(Nk, 32)
    nb = hip.query("fs_attention_split_ws_bytes", B, Nk, heads)
    o_o, lse_o, ws_o = Out(B * N * C), Out(rows), Out(nb, torch.uint8)
    mask_o = Out(nw, torch.int32)
    hip.call("fs_attention_fwd_split", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), o_o.ptr, lse_o.ptr, mask_o.ptr if p > 0 else None, ws_o.ptr, nb,
             B, N, Nk, heads, SCALE, p, key)
    ws_o.get(complete=False)
    check(fam, f"o.{tag}", o_o.get(), ref.o, ref.bound_o())
    check(fam, f"lse.{tag}", lse_o.get(), ref.lse, ref.bound_lse())
    if Nk == 1 and p == 0:
        # P = 1 exactly (planes 1, 0, 0) and v needs all three of its bf16 planes: o = v1 + v2 + v3 = v BIT FOR BIT only if the plane
        # products (P1, v1), (P1, v2), (P1, v3) are all kept -- a dropped lower-plane product shows at the 2^-8 / 2^-16 level here,
        # far inside the worst-case bound above
        exact(fam, f"o.one_key.{tag}", o_o.get(), R._tokens(heads_of(v, heads).expand(B, heads, N, 64)))
    words = keep_words(B, heads, N, Nk, key, p) if p > 0 else None
    if p > 0:          # every word written; the bits of keys < Nk are the hash oracle's, for every Nk (also beyond 96 keys)
        got_w = mask_o.get().numpy().view(np.uint32).reshape(rows, -1)
        valid = keep_words(B, heads, N, Nk, key, 0.0)          # all-ones below Nk
        assert np.array_equal(got_w & valid, words), f"{fam} {tag}: the keep words are not the hash oracle's"
    else:
        assert mask_o.untouched()
    # a short scratch is refused
    if nb > 0:
        o2 = Out(B * N * C)
        rejected("fs_attention_fwd_split", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), o2.ptr, lse_o.ptr, None, ws_o.ptr, nb - 1, B, N, Nk, heads, SCALE, p, key)
        assert o2.untouched()

    # ---- backward: the two parts alone from clean lse and D, then the whole from clean o and lse -----------------------------------------
    lsed, Dd, od = dev(f32(ref.lse)), dev(f32(ref.D)), dev(f32(ref.o))
    maskd = torch.from_numpy(words.view(np.int32).copy()).reshape(-1).to(DEV) if p > 0 else None
    nbb = hip.query("fs_attention_bwd_split_ws_bytes", B, Nk, heads)
    off = hip.query("fs_attention_bwd_split_parts_offset", B, Nk, heads)
    nparts = 2 * 8 * B * Nk * heads * 64
    assert nbb == off + 4 * nparts and off % 16 == 0
    bq, bk, bv = ref.backward_bounds(d_on_device=False)
    dq_o, wsq = Out(B * N * C), Out(off, torch.uint8)
    hip.call("fs_attention_bwd_dq_split", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), hip.ptr(god), hip.ptr(lsed), hip.ptr(Dd), hip.ptr(maskd), dq_o.ptr,
             wsq.ptr, off, B, N, Nk, heads, SCALE, p, key)
    wsq.get(complete=False)
    dq_parts = dq_o.get()
    check(fam, f"dq.dq_split.{tag}", dq_parts, ref.dq, bq)
    nsp = split_kv_splits(B, heads, N, Nk)
    if N >= 127 and regime == "randn":
        assert nsp > 1, "this case must split the query range of the dK / dV sweep"
    for with_parts in (False, True):          # without parts: one query range; with: attn_kv_splits ranges, summed in index order
        dk_o, dv_o, parts = Out(B * Nk * C), Out(B * Nk * C), Out(nparts)
        hip.call("fs_attention_bwd_dkv_split", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), hip.ptr(god), hip.ptr(lsed), hip.ptr(Dd),
                 None if with_parts else hip.ptr(maskd), dk_o.ptr, dv_o.ptr, parts.ptr if with_parts else None, B, N, Nk, heads, SCALE, p, key)
        body = parts.get(complete=False)
        if not with_parts or nsp == 1:
            assert parts.untouched()
        else:          # the library's own split count: exactly nsp partial tensors of dk and of dv were written, nothing else
            elems = B * Nk * C
            written = ~torch.isnan(body)
            assert bool(written[:2 * nsp * elems].all()) and not bool(written[2 * nsp * elems:].any()), \
                f"{fam} {tag}: the dK / dV sweep did not write {nsp} partial tensors"
        check(fam, f"dk.dkv_split.parts{int(with_parts)}.{tag}", dk_o.get(), ref.dk, bk)
        check(fam, f"dv.dkv_split.parts{int(with_parts)}.{tag}", dv_o.get(), ref.dv, bv)
    bq, bk, bv = ref.backward_bounds(d_on_device=True)
    whole = []
    for rep in range(2):
        dq_o, dk_o, dv_o, scr, wsb = Out(B * N * C), Out(B * Nk * C), Out(B * Nk * C), Out(rows), Out(nbb, torch.uint8)
        hip.call("fs_attention_bwd_split", hip.ptr(qd), hip.ptr(kd), hip.ptr(vd), hip.ptr(od), hip.ptr(god), hip.ptr(lsed), hip.ptr(maskd) if rep == 0 else None,
                 dq_o.ptr, dk_o.ptr, dv_o.ptr, scr.ptr, wsb.ptr, nbb, B, N, Nk, heads, SCALE, p, key)
        wsb.get(complete=False)
        scr.get()
        whole.append((dq_o.get(), dk_o.get(), dv_o.get()))
    for name, got, want, bound in zip(("dq", "dk", "dv"), whole[0], (ref.dq, ref.dk, ref.dv), (bq, bk, bv)):
        check(fam, f"{name}.bwd_split.{tag}", got, want, bound)
    # partial tensors are summed in index order, the keep words equal the hash: two calls (words / hashing again) are bit-identical
    for a, b_ in zip(whole[0], whole[1]):
        assert torch.equal(a, b_), f"{fam} {tag}: two calls of the split backward differ"


def test_attention_rejects():
    B, heads, N, Nk = 1, 1, 4, 4
    t = dev(torch.zeros(B, N, 64))
    o_o, lse_o = Out(B * N * 64), Out(N)
    rejected("fs_attention_fwd", hip.ptr(t), hip.ptr(t), hip.ptr(t), o_o.ptr, lse_o.ptr, B, N, 0, heads, SCALE, 0.0, 1)
    rejected("fs_attention_fwd", hip.ptr(t), hip.ptr(t), hip.ptr(t), o_o.ptr, lse_o.ptr, B, N, Nk, heads, SCALE, 1.0, 1)
    rejected("fs_attention_fwd_split", hip.ptr(t), hip.ptr(t), hip.ptr(t), o_o.ptr, lse_o.ptr, None, None, 0, B, N, Nk, heads, SCALE, 0.0, 1)
    assert o_o.untouched() and lse_o.untouched()
