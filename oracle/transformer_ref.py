"""Plain references of the SegFormer kernels (csrc/transformer.hip, csrc/attention_split.hip), one function per entry point,
written from the formulas in include/fovealseg.h.

Every function works on torch tensors in the kernels' layouts (tokens (M, C), images NHWC, depthwise weights (C, 9), patch
rows (B*Ho*Wo, Kp), q / o (B, N, heads*64), k / v (B, Nk, heads*64)) and computes in the dtype of its inputs: fp64 inputs give
the reference, fp32 inputs give "the same formula in fp32", which the GPU tests use as the error scale of a correct fp32
evaluation.  Nothing here calls F.layer_norm, F.gelu, F.conv2d, F.unfold / F.fold, torch.softmax, logsumexp or
scaled_dot_product_attention: those are what tests/test_transformer_ref.py checks these functions against.  Row sums are
torch.sum / einsum in the working dtype; taps and patch elements are explicit loops.

Dropout and DropPath decisions come from the hash oracle (fovealseg_oracle.dropout_keep_mask_nhwc); the constants the C ABI
carries as float (eps, the drop scale, the threshold, the attention scale) are formed here exactly as transformer.hip forms them.
"""

import numpy as np
import torch

import fovealseg_oracle as O

HD = 64          # head dim of the attention kernels


# ------------------------------------------------------------------------------------------------
# the ABI's float constants
# ------------------------------------------------------------------------------------------------
def abi_float(v):
    """a Python number as the C ABI carries it: rounded to float"""
    return float(np.float32(v))


def drop_scale(p):
    """1.0f / (float)(1.0 - (double)p) with p a float argument (0 -> 1)"""
    if p == 0:
        return 1.0
    return float(np.float32(1.0) / np.float32(1.0 - float(np.float32(p))))


def drop_thresh(p):
    """(uint32)((double)p * 2^32) with p a float argument; 0 = no dropout"""
    return int(float(np.float32(p)) * 4294967296.0) & 0xFFFFFFFF


def keep_mask(n, key, p):
    """the keep decisions of elements 0 .. n-1 under (key, p) as a bool tensor (all True for p = 0)"""
    if p == 0:
        return torch.ones(n, dtype=torch.bool)
    return torch.from_numpy(O.dropout_keep_mask_nhwc(n, key, abi_float(p))).bool()


# ------------------------------------------------------------------------------------------------
# LayerNorm over the last dim of (M, C)
# ------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps):
    """fs_layernorm_fwd: y, mean (M), rstd (M) = 1 / sqrt(biased var + eps); the variance is that of the centred row (two-pass)"""
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(var + eps)
    return d * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(g, x, gamma, mean, rstd, addend=None):
    """fs_layernorm_bwd / _bwd_add: dx = rstd * (g gamma - mean_c(g gamma) - xhat * mean_c(g gamma xhat)) [+ addend],
    dgamma = sum_rows g * xhat, dbeta = sum_rows g"""
    C = x.shape[-1]
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = g * gamma
    m1 = gg.sum(-1, keepdim=True) / C
    m2 = (gg * xh).sum(-1, keepdim=True) / C
    dx = rstd[:, None] * (gg - m1 - xh * m2)
    if addend is not None:
        dx = dx + addend
    return dx, (g * xh).sum(0), g.sum(0)


# ------------------------------------------------------------------------------------------------
# exact GELU
# ------------------------------------------------------------------------------------------------
INV_SQRT2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


def gelu_cdf(x):
    """Phi(x) = 0.5 (1 + erf(x / sqrt 2)).  In fp32 exactly that expression (the kernel's); in fp64 the same function as
    0.5 erfc(-x / sqrt 2), which keeps its relative accuracy in the negative tail where 1 + erf cancels"""
    if x.dtype == torch.float64:
        return 0.5 * torch.special.erfc(-x * INV_SQRT2)
    return 0.5 * (1.0 + torch.erf(x * x.new_tensor(INV_SQRT2)))


def gelu_pdf(x):
    return INV_SQRT_2PI * torch.exp(-0.5 * x * x)


def gelu_fwd(x):
    """fs_gelu_fwd: x Phi(x)"""
    if x.dtype == torch.float64:
        return x * gelu_cdf(x)
    return 0.5 * x * (1.0 + torch.erf(x * x.new_tensor(INV_SQRT2)))


def gelu_grad(x):
    """d/dx x Phi(x) = Phi(x) + x phi(x)"""
    return gelu_cdf(x) + x * gelu_pdf(x)


def gelu_bwd(g, x):
    return g * gelu_grad(x)


def gelu_dropout_fwd(x, p, key):
    """fs_gelu_dropout_fwd: keep ? gelu(x) * drop_scale : 0, the element hash on the flat index"""
    keep = keep_mask(x.numel(), key, p).reshape(x.shape)
    return torch.where(keep, gelu_fwd(x) * drop_scale(p), torch.zeros_like(x))


def gelu_dropout_bwd(g, x, p, key):
    """fs_gelu_dropout_bwd: (keep ? g * drop_scale : 0) * gelu'(x)"""
    keep = keep_mask(x.numel(), key, p).reshape(x.shape)
    return torch.where(keep, g * drop_scale(p), torch.zeros_like(g)) * gelu_grad(x)


# ------------------------------------------------------------------------------------------------
# depthwise 3x3, stride 1, pad 1; x (B, H, W, C), w (C, 9) = [c][3 ty + tx], bias (C) or None
# ------------------------------------------------------------------------------------------------
def _pad1(x):
    B, H, W, C = x.shape
    xp = x.new_zeros(B, H + 2, W + 2, C)
    xp[:, 1:H + 1, 1:W + 1] = x
    return xp


def dwconv3_fwd(x, w, bias=None, flip=False):
    """fs_dwconv3_fwd: y[p] = bias + sum_t w[c][t] x[p + t - (1, 1)]; flip: tap t reads w[c][8 - t] (the input gradient)"""
    B, H, W, C = x.shape
    xp = _pad1(x)
    y = x.new_zeros(B, H, W, C)
    if bias is not None:
        y = y + bias
    for ty in range(3):
        for tx in range(3):
            t = 3 * ty + tx
            y = y + xp[:, ty:ty + H, tx:tx + W] * w[:, 8 - t if flip else t]
    return y


def dwconv3_bwd_weight(x, dy):
    """fs_dwconv3_bwd_weight: dw[c][t] = sum_pixels x[p + t - (1, 1)][c] * dy[p][c]  -> (C, 9)"""
    B, H, W, C = x.shape
    xp = _pad1(x)
    cols = []
    for ty in range(3):
        for tx in range(3):
            cols.append((xp[:, ty:ty + H, tx:tx + W] * dy).sum((0, 1, 2)))
    return torch.stack(cols, 1)


def dwconv3_bwd_bias(dy):
    return dy.sum((0, 1, 2))


# ------------------------------------------------------------------------------------------------
# residual + DropPath
# ------------------------------------------------------------------------------------------------
def droppath_factor(n, per_sample, p, key):
    """the per-element factor of DropPath: drop_scale where the element's sample (flat index / per_sample) is kept, else 0"""
    nsamp = -(-n // per_sample)
    keep = keep_mask(nsamp, key, p)
    return keep.repeat_interleave(per_sample)[:n]


def residual_droppath(x, y, per_sample, p, key):
    """fs_residual_droppath: out = x + keep_b * y * drop_scale over the flat tensors (x None: no addend)"""
    keep = droppath_factor(y.numel(), per_sample, p, key).reshape(y.shape)
    v = torch.where(keep, y * drop_scale(p), torch.zeros_like(y))
    return v if x is None else x + v


def droppath_dropout_bwd(g, per_sample, droppath_p, droppath_key, p, key):
    """fs_droppath_dropout_bwd: Dropout-mask(DropPath-scale_b * g)"""
    v = residual_droppath(None, g, per_sample, droppath_p, droppath_key)
    keep = keep_mask(g.numel(), key, p).reshape(g.shape)
    return torch.where(keep, v * drop_scale(p), torch.zeros_like(v))


# ------------------------------------------------------------------------------------------------
# unfold / fold: x (B, H, W, C) <-> col (B*Ho*Wo, Kp), column (r k + s) C + c, zeros in columns k k C .. Kp - 1
# ------------------------------------------------------------------------------------------------
def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def unfold(x, k, stride, pad, Kp):
    B, H, W, C = x.shape
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    col = x.new_zeros(B, Ho, Wo, Kp)
    for r in range(k):
        for s in range(k):
            e = (r * k + s) * C
            for oy in range(Ho):
                iy = oy * stride - pad + r
                if iy < 0 or iy >= H:
                    continue
                for ox in range(Wo):
                    ix = ox * stride - pad + s
                    if 0 <= ix < W:
                        col[:, oy, ox, e:e + C] = x[:, iy, ix]
    return col.reshape(B * Ho * Wo, Kp)


def fold(col, B, H, W, C, k, stride, pad):
    """the adjoint of unfold: dx[pixel] = the sum of every patch element that was copied from it"""
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    col = col.reshape(B, Ho, Wo, -1)
    dx = col.new_zeros(B, H, W, C)
    for r in range(k):
        for s in range(k):
            e = (r * k + s) * C
            for oy in range(Ho):
                iy = oy * stride - pad + r
                if iy < 0 or iy >= H:
                    continue
                for ox in range(Wo):
                    ix = ox * stride - pad + s
                    if 0 <= ix < W:
                        dx[:, iy, ix] += col[:, oy, ox, e:e + C]
    return dx


# ------------------------------------------------------------------------------------------------
# attention: per (batch, head)  S = q k^T scale, P = softmax rows, P~ = mask P drop_scale, O = P~ v
# ------------------------------------------------------------------------------------------------
def _heads(t, heads):          # (B, n, heads*64) -> (B, heads, n, 64)
    B, n, _ = t.shape
    return t.reshape(B, n, heads, HD).permute(0, 2, 1, 3)


def _tokens(t):                # (B, heads, n, 64) -> (B, n, heads*64)
    B, h, n, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, h * HD)


def attention_parts(q, k, v, heads, scale, p=0.0, key=0):
    """S, P, M (= keep mask * drop_scale), all (B, heads, N, Nk), and lse (B, heads, N) = log sum_j exp S_j"""
    qh, kh = _heads(q, heads), _heads(k, heads)
    B, _, N, _ = qh.shape
    Nk = kh.shape[2]
    S = torch.einsum("bhnd,bhkd->bhnk", qh, kh) * scale
    m = S.amax(-1, keepdim=True)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    P = E / l
    lse = (m + torch.log(l)).squeeze(-1)
    keep = keep_mask(B * heads * N * Nk, key, p).reshape(B, heads, N, Nk)
    M = keep.to(S.dtype) * drop_scale(p)
    return S, P, M, lse


def attention_fwd(q, k, v, heads, scale, p=0.0, key=0):
    """fs_attention_fwd / _fwd_split: o (B, N, heads*64), lse (B*heads*N)"""
    S, P, M, lse = attention_parts(q, k, v, heads, scale, p, key)
    o = torch.einsum("bhnk,bhkd->bhnd", P * M, _heads(v, heads))
    return _tokens(o), lse.reshape(-1)


def attention_rowdot(go, o, heads):
    """D = rowsum(dO * O) per (batch, head, query): B*heads*N"""
    return (_heads(go, heads) * _heads(o, heads)).sum(-1).reshape(-1)


def attention_bwd(q, k, v, go, heads, scale, p=0.0, key=0):
    """fs_attention_bwd / _bwd_split: dq, dk, dv with dP~ = dO v^T, D = rowsum(dO * O), dS = P * (M dP~ - D) * scale"""
    S, P, M, lse = attention_parts(q, k, v, heads, scale, p, key)
    qh, kh, vh, gh = (_heads(t, heads) for t in (q, k, v, go))
    Pt = P * M
    o = torch.einsum("bhnk,bhkd->bhnd", Pt, vh)
    dPt = torch.einsum("bhnd,bhkd->bhnk", gh, vh)
    D = (gh * o).sum(-1, keepdim=True)
    dS = P * (M * dPt - D) * scale
    dq = torch.einsum("bhnk,bhkd->bhnd", dS, kh)
    dk = torch.einsum("bhnk,bhnd->bhkd", dS, qh)
    dv = torch.einsum("bhnk,bhnd->bhkd", Pt, gh)
    return _tokens(dq), _tokens(dk), _tokens(dv)
