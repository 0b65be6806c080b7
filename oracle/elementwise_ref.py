"""Plain references of the memory-bound kernels (csrc/elementwise.hip, the head tail of csrc/head_loss.hip, csrc/optim.hip),
one function per entry point, written from the formulas in include/fovealseg.h.

Every function works on torch tensors in the kernels' NHWC layout and computes in the dtype of its inputs: fp64 inputs give
the reference, fp32 inputs give "the same formula in fp32", which the GPU tests use as the error scale of a correct fp32
evaluation.  Nothing here calls F.batch_norm, F.interpolate, max_pool2d, avg_pool2d, conv2d or an optimiser: those are what
tests/test_elementwise_ref.py checks these functions against.  Sums over rows are torch.sum / einsum in the working dtype;
window scans are explicit loops.
"""
import math

import numpy as np
import torch

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2


# ------------------------------------------------------------------------------------------------
# BatchNorm
# ------------------------------------------------------------------------------------------------
def bn_batch_stats(y, eps, momentum=None, running_mean=None, running_var=None):
    """fs_bn_stats / fs_bn_finalize_slab: y (M, C) -> mean, invstd = 1 / sqrt(biased var + eps) and, when running statistics
    are given, their update with the UNBIASED variance (M / (M - 1); M = 1 keeps the biased one, as the kernels do)."""
    M = y.shape[0]
    mean = y.sum(0) / M
    var = ((y - mean) ** 2).sum(0) / M
    invstd = 1.0 / torch.sqrt(var + eps)
    if running_mean is None:
        return mean, invstd, None, None
    unbiased = var * (M / (M - 1 if M > 1 else 1))
    return (mean, invstd, momentum * mean + (1.0 - momentum) * running_mean,
            momentum * unbiased + (1.0 - momentum) * running_var)


def bn_stats_from_sums(s1, s2, M, eps):
    """fs_bn_finalize_slab from the column sums of y and y*y (what a slab adds up to): mean, biased var, invstd."""
    mean = s1 / M
    var = torch.clamp(s2 / M - mean * mean, min=0.0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_eval_prepare(running_mean, running_var, eps):
    return running_mean.clone(), 1.0 / torch.sqrt(running_var + eps)


def bn_eval_affine(running_mean, running_var, gamma, beta, eps):
    scale = gamma / torch.sqrt(running_var + eps)
    return scale, beta - running_mean * scale


def act_fwd(v, act):
    if act == ACT_RELU:
        return torch.where(v < 0, torch.zeros_like(v), v)
    if act == ACT_RELU6:
        return torch.clamp(v, 0.0, 6.0)
    return v


def act_bits(out, act):
    """act'(out) != 0 from the activation OUTPUT: ReLU out > 0, ReLU6 0 < out < 6, none: all ones.  bool, shape of out."""
    if act == ACT_RELU:
        return out > 0
    if act == ACT_RELU6:
        return (out > 0) & (out < 6)
    return torch.ones_like(out, dtype=torch.bool)


def pack_mask(bits):
    """The mask layout of fs_bn_act_fwd: bits (M, C) bool -> (M * C / 4) bytes, bit j of byte e / 4 = bits[e + j]."""
    b = bits.reshape(-1, 4).to(torch.uint8)
    return b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)


def unpack_mask(mask, M, C):
    m = mask.reshape(-1, 1).to(torch.int32)
    return ((m >> torch.arange(4, dtype=torch.int32)) & 1).bool().reshape(M, C)


def bn_pre_act(y, mean, invstd, gamma, beta, res=None):
    """(y - mean) * invstd * gamma + beta [+ res]: the argument of the activation in fs_bn_act_fwd."""
    v = (y - mean) * invstd * gamma + beta
    return v if res is None else v + res


def bn_act_fwd(y, mean, invstd, gamma, beta, res, act):
    return act_fwd(bn_pre_act(y, mean, invstd, gamma, beta, res), act)


def bn_bwd_sums(dz, bits, y, mean, invstd):
    """fs_bn_bwd_partial summed over its slab rows: S = sum g, SX = sum g * xhat over the M rows, g = dz where bits else 0."""
    g = torch.where(bits, dz, torch.zeros_like(dz))
    return g.sum(0), (g * ((y - mean) * invstd)).sum(0)


def bn_bwd_finalize(S, SX, gamma, mean, invstd, M, training):
    """fs_bn_bwd_finalize: dgamma = SX, dbeta = S, coef[4][C] = ga, d, mean, bb with ga = gamma * invstd,
    d = ga * invstd * SX / M, bb = ga * S / M (eval mode: d = bb = 0)."""
    ga = gamma * invstd
    z = torch.zeros_like(ga)
    d = ga * (SX / M) * invstd if training else z
    bb = ga * (S / M) if training else z
    return SX.clone(), S.clone(), torch.stack([ga, d, mean.clone(), bb])


def bn_bwd_apply(dz, bits, y, coef, keep=None, drop_p=0.0):
    """fs_bn_bwd_apply: g = dz where bits else 0; dy = (ga * g - d * (y - mean) - bb) [* keep / (1 - p)]; dres = g.
    keep (M, C) bool: the dropout keep mask of the conv output (fovealseg_oracle.dropout_keep_mask_nhwc)."""
    g = torch.where(bits, dz, torch.zeros_like(dz))
    dy = coef[0] * g - coef[1] * (y - coef[2]) - coef[3]
    if keep is not None:
        dy = torch.where(keep, dy / (1.0 - drop_p), torch.zeros_like(dy))
    return dy, g


def add_n(terms):
    out = terms[0] + terms[1]
    for t in terms[2:]:
        out = out + t
    return out


def relu_bwd(dout, out):
    return torch.where(out > 0, dout, torch.zeros_like(dout))


# ------------------------------------------------------------------------------------------------
# bilinear up-sampling (align_corners=False) as an explicit weight matrix
# ------------------------------------------------------------------------------------------------
def lerp_matrix(n_in, n_out, dtype=torch.float64):
    """(n_out, n_in) weights of one axis: source index s = max(0, (d + 0.5) * n_in / n_out - 0.5), i0 = floor(s),
    i1 = min(i0 + 1, n_in - 1), weights 1 - (s - i0) and s - i0 (both land on i0 at the far edge); identity for n_in == n_out."""
    Wm = torch.zeros(n_out, n_in, dtype=dtype)
    for d in range(n_out):
        if n_in == n_out:
            Wm[d, d] = 1.0
            continue
        s = max(0.0, (d + 0.5) * (n_in / n_out) - 0.5)
        i0 = int(math.floor(s))
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = s - i0
        Wm[d, i0] += 1.0 - l1
        Wm[d, i1] += l1
    return Wm


def upsample_matrix(th, tw, Ho, Wo, dtype=torch.float64):
    """(Ho * Wo, th * tw): the 2-D map as the Kronecker product of the two axis matrices."""
    return torch.kron(lerp_matrix(th, Ho, dtype), lerp_matrix(tw, Wo, dtype))


def upsample(src, Ho, Wo):
    """src (B, th, tw, C) -> (B, Ho, Wo, C)."""
    B, th, tw, C = src.shape
    Wm = upsample_matrix(th, tw, Ho, Wo, src.dtype)
    return torch.einsum("oq,bqc->boc", Wm, src.reshape(B, th * tw, C)).reshape(B, Ho, Wo, C)


def upsample_slice_fwd(dst, src, coff):
    """fs_upsample_slice_fwd: dst[..., coff:coff+C] = up(src); every other channel of dst is kept.  Returns the new dst."""
    out = dst.clone()
    out[..., coff:coff + src.shape[-1]] = upsample(src, dst.shape[1], dst.shape[2])
    return out


def upsample_slice_bwd(g, coff, C, th, tw):
    """fs_upsample_slice_bwd: the transpose of the map applied to g[..., coff:coff+C]; g (B, Ho, Wo, Cg) -> (B, th, tw, C)."""
    B, Ho, Wo, _ = g.shape
    Wm = upsample_matrix(th, tw, Ho, Wo, g.dtype)
    gs = g[..., coff:coff + C].reshape(B, Ho * Wo, C)
    return torch.einsum("oq,boc->bqc", Wm, gs).reshape(B, th, tw, C)


def hr_fuse_fwd(terms, Ho, Wo, relu):
    """fs_hr_fuse_fwd: [relu](sum_t up(terms[t])), summed in term order."""
    acc = None
    for t in terms:
        v = t if (t.shape[1] == Ho and t.shape[2] == Wo) else upsample(t, Ho, Wo)
        acc = v if acc is None else acc + v
    return torch.where(acc < 0, torch.zeros_like(acc), acc) if relu else acc


# ------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------
def maxpool_fwd(x, k, stride, pad):
    """fs_maxpool_fwd: x (B, H, W, C) -> out (B, Ho, Wo, C), arg (B, Ho, Wo, C) int32 = iy * W + ix of the maximum.
    The window is scanned row-major over its in-image taps; the first tap is taken, a later tap replaces it when it is
    greater or NaN (so the first of equal maxima stays, and the last NaN wins)."""
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty(B, Ho, Wo, C, dtype=x.dtype)
    arg = torch.empty(B, Ho, Wo, C, dtype=torch.int32)
    for oy in range(Ho):
        for ox in range(Wo):
            best, bi = None, None
            for r in range(k):
                iy = oy * stride - pad + r
                if iy < 0 or iy >= H:
                    continue
                for q in range(k):
                    ix = ox * stride - pad + q
                    if ix < 0 or ix >= W:
                        continue
                    v = x[:, iy, ix, :]
                    if best is None:
                        best, bi = v.clone(), torch.full((B, C), iy * W + ix, dtype=torch.int32)
                    else:
                        take = (v > best) | torch.isnan(v)
                        best = torch.where(take, v, best)
                        bi = torch.where(take, torch.full_like(bi, iy * W + ix), bi)
            out[:, oy, ox, :], arg[:, oy, ox, :] = best, bi
    return out, arg


def maxpool_bwd(dout, arg, H, W):
    """fs_maxpool_bwd: dx (B, H, W, C) = every dout scattered to the pixel arg names; pixels no window names get 0."""
    B, Ho, Wo, C = dout.shape
    dx = torch.zeros(B, H * W, C, dtype=dout.dtype)
    dx.scatter_add_(1, arg.reshape(B, Ho * Wo, C).long(), dout.reshape(B, Ho * Wo, C))
    return dx.reshape(B, H, W, C)


def avgpool_fwd(x):
    """fs_avgpool_fwd: x (B, HW, C) -> (B, C), the mean over HW."""
    return x.sum(1) / x.shape[1]


def avgpool_bwd(dout, HW):
    """fs_avgpool_bwd: dout (B, C) -> (B, HW, C), every pixel gets dout / HW."""
    return (dout / HW)[:, None, :].expand(-1, HW, -1).contiguous()


# ------------------------------------------------------------------------------------------------
# C1 head tail
# ------------------------------------------------------------------------------------------------
def mask_head_fwd(x, w, bias):
    """fs_mask_head_fwd: x (npix, C), w (C), bias (1) -> m (npix) = sigmoid(x . w + bias) - 0.5."""
    logit = torch.einsum("pc,c->p", x, w) + bias[0]
    return 1.0 / (1.0 + torch.exp(-logit)) - 0.5


def mask_head_bwd(dm, m, x, w):
    """fs_mask_head_bwd: dlogit = dm * s * (1 - s), s = m + 0.5; dx = dlogit w^T, dw = x^T dlogit, db = sum dlogit."""
    s = m + 0.5
    dl = dm * s * (1.0 - s)
    return dl[:, None] * w[None, :], torch.einsum("p,pc->c", dl, x), dl.sum().reshape(1)


def pred_assemble_fwd(cls, m):
    """fs_pred_assemble_fwd: cls (B, K), m (B, HW) -> pred (B, K, HW): pred[:, k] = cls[:, k] for k < K - 1,
    pred[:, K - 1] = cls[:, K - 1] * m."""
    B, K = cls.shape
    pred = cls[:, :, None].expand(B, K, m.shape[1]).clone()
    pred[:, K - 1, :] = cls[:, K - 1, None] * m
    return pred


def pred_assemble_bwd(dpred, cls, m):
    """fs_pred_assemble_bwd: dcls[:, k] = sum_p dpred[:, k] (times m for k = K - 1), dm = dpred[:, K - 1] * cls[:, K - 1]."""
    K = cls.shape[1]
    dcls = dpred.sum(2)
    dcls[:, K - 1] = (dpred[:, K - 1, :] * m).sum(1)
    return dcls, dpred[:, K - 1, :] * cls[:, K - 1, None]


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    """fs_adam_step = torch.optim.Adam(weight_decay): g' = grad_scale * g + wd * p; m = b1 m + (1 - b1) g';
    v = b2 v + (1 - b2) g'^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
    The scalars cross the C ABI as float, so they are rounded to fp32 first; the bias corrections 1 - b^t are formed in
    fp64 from the rounded betas in every working dtype.  Returns (p_new, m_new, v_new)."""
    lr, b1, b2, eps, wd, gs = (float(np.float32(a)) for a in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1 = 1.0 - b1 ** step
    bc2_sqrt = math.sqrt(1.0 - b2 ** step)
    gg = g * gs + wd * p
    m2 = b1 * m + (1.0 - b1) * gg
    v2 = b2 * v + (1.0 - b2) * gg * gg
    denom = torch.sqrt(v2) / bc2_sqrt + eps
    return p - (lr / bc1) * (m2 / denom), m2, v2
