"""Plain references of the convolution engine (csrc/conv*.hip), one function per entry point, written from the formulas in
include/fovealseg.h and the header of csrc/conv.hip.

Activations are NHWC (B, H, W, C), weights RSCK ([R][S][Cin][Cout]), as the C ABI takes them.  Every function computes in the
dtype of its inputs (fp64 inputs give the reference).  Nothing here calls F.conv2d, conv_transpose2d or autograd: those are what
tests/test_conv_ref.py checks these functions against.  A convolution is an explicit loop over the filter taps; the
contraction over channels (forward, bwd-data) or pixels (bwd-weight) inside one tap is an einsum in the working dtype.

    forward   : y[b,oy,ox,k]  = sum_{r,s,c} x[b, oy*stride - pad + r*dil, ox*stride - pad + s*dil, c] * w[r,s,c,k]
    bwd-data  : dx[b,iy,ix,c] = sum_{r,s,k} dy[b,oy,ox,k] * w[r,s,c,k]      over the (oy, r) with oy*stride - pad + r*dil = iy
    bwd-weight: dw[r,s,c,k]   = sum_{b,oy,ox} x[b, oy*stride - pad + r*dil, ox*stride - pad + s*dil, c] * dy[b,oy,ox,k]

Dropout and DropPath decisions come from the hash oracle (fovealseg_oracle.dropout_keep_mask_nhwc through transformer_ref);
the drop scale is the float the C ABI forms.

Bound helpers: the same loops on absolute values give, for every output element, sum|terms| of its contraction; on all-ones
operands they give the contraction length (the number of in-range products).
"""
import torch

import elementwise_ref as E
import transformer_ref as R


def out_size(n, k, stride, pad, dil=1):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _span(n_in, n_out, t, stride, pad, dil):
    """the outputs o in [lo, hi) whose tap t reads an in-range input i = o*stride - pad + t*dil, and the first such input"""
    off = t * dil - pad
    lo = max(0, -(off // stride))                       # smallest o with o*stride + off >= 0
    hi = min(n_out, (n_in - 1 - off) // stride + 1)     # one past the largest o with o*stride + off <= n_in - 1
    return lo, hi, lo * stride + off


def _taps(H, W, Ho, Wo, R_, S_, stride, pad, dil):
    """(r, s, output slices, input slices) of every tap that reaches the image"""
    for r in range(R_):
        ylo, yhi, iy0 = _span(H, Ho, r, stride, pad, dil)
        if yhi <= ylo:
            continue
        for s in range(S_):
            xlo, xhi, ix0 = _span(W, Wo, s, stride, pad, dil)
            if xhi <= xlo:
                continue
            yield (r, s, slice(ylo, yhi), slice(xlo, xhi),
                   slice(iy0, iy0 + (yhi - ylo - 1) * stride + 1, stride), slice(ix0, ix0 + (xhi - xlo - 1) * stride + 1, stride))


# ------------------------------------------------------------------------------------------------
# the three convolutions
# ------------------------------------------------------------------------------------------------
def conv(x, w, stride=1, pad=0, dil=1):
    """the bare forward sum: x (B, H, W, Cin), w (R, S, Cin, Cout) -> (B, Ho, Wo, Cout)"""
    B, H, W, _ = x.shape
    R_, S_, _, Cout = w.shape
    Ho, Wo = out_size(H, R_, stride, pad, dil), out_size(W, S_, stride, pad, dil)
    y = torch.zeros(B, Ho, Wo, Cout, dtype=x.dtype)
    for r, s, oy, ox, iy, ix in _taps(H, W, Ho, Wo, R_, S_, stride, pad, dil):
        y[:, oy, ox] += torch.einsum("bhwc,ck->bhwk", x[:, iy, ix], w[r, s])
    return y


def dropout(v, p, key):
    """nn.Dropout as fs_conv2d_fwd applies it: element e (flat NHWC index of the output) is kept by the hash, kept values are
    multiplied by the float 1 / (1 - p)"""
    if p == 0:
        return v
    keep = R.keep_mask(v.numel(), key, p).reshape(v.shape)
    return torch.where(keep, v * R.drop_scale(p), torch.zeros_like(v))


def conv2d_fwd(x, w, bias=None, stride=1, pad=0, dil=1, drop_p=0.0, drop_key=0):
    """fs_conv2d_fwd: Dropout(conv(x, w) + bias)"""
    y = conv(x, w, stride, pad, dil)
    if bias is not None:
        y = y + bias
    return dropout(y, drop_p, drop_key)


def conv2d_bwd_data(dy, w, H, W, stride=1, pad=0, dil=1):
    """fs_conv2d_bwd_data: dy (B, Ho, Wo, Cout) -> dx (B, H, W, Cin); pixels no tap reaches are zero"""
    B, Ho, Wo, _ = dy.shape
    R_, S_, Cin, _ = w.shape
    dx = torch.zeros(B, H, W, Cin, dtype=dy.dtype)
    for r, s, oy, ox, iy, ix in _taps(H, W, Ho, Wo, R_, S_, stride, pad, dil):
        dx[:, iy, ix] += torch.einsum("bhwk,ck->bhwc", dy[:, oy, ox], w[r, s])
    return dx


def conv2d_bwd_weight(x, dy, R_, S_, stride=1, pad=0, dil=1, dw0=None):
    """fs_conv2d_bwd_weight: dw (R, S, Cin, Cout); dw0 = the accumulating target of accumulate = 1 (added to)"""
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    dw = torch.zeros(R_, S_, Cin, Cout, dtype=x.dtype)
    for r, s, oy, ox, iy, ix in _taps(H, W, Ho, Wo, R_, S_, stride, pad, dil):
        dw[r, s] = torch.einsum("bhwc,bhwk->ck", x[:, iy, ix], dy[:, oy, ox])
    return dw if dw0 is None else dw0 + dw


def linear_wgrad_ref(x, dy):
    """fs_linear_bwd_weight_bias: x (rows, Cin), dy (rows, Cout) -> dw (Cin, Cout) = x^T dy, dbias (Cout) = column sums of dy"""
    return torch.einsum("rc,rk->ck", x, dy), dy.sum(0)


def linear_wgrad_terms(x, dy):
    """sum|terms| of every element of the pair above: |x|^T |dy| and the column sums of |dy|"""
    return linear_wgrad_ref(x.abs(), dy.abs())


# ------------------------------------------------------------------------------------------------
# the fused entry points
# ------------------------------------------------------------------------------------------------
def stats_totals(y):
    """fs_conv2d_fwd_stats: what the [slabs][Cout][2] partial sums add up to -- per channel sum and sum of squares of the
    STORED output (after bias and dropout) -> (Cout, 2)"""
    v = y.reshape(-1, y.shape[-1])
    return torch.stack([v.sum(0), (v * v).sum(0)], dim=1)


def conv2d_fwd_affine_act_pre(x, w, bias, scale, shift, res=None, stride=1, pad=0, dil=1):
    """the argument of the activation in fs_conv2d_fwd_affine_act: (conv(x, w) + bias) * scale[c] + shift[c] [+ res]"""
    v = conv2d_fwd(x, w, bias, stride, pad, dil) * scale + shift
    return v if res is None else v + res


def conv2d_fwd_affine_act(x, w, bias, scale, shift, res, act, stride=1, pad=0, dil=1):
    return E.act_fwd(conv2d_fwd_affine_act_pre(x, w, bias, scale, shift, res, stride, pad, dil), act)


def conv2d_fwd_residual(x, w, bias, res, stride=1, pad=0, dil=1, drop_p=0.0, drop_key=0, droppath_p=0.0, droppath_key=0,
                        rows_per_sample=1):
    """fs_conv2d_fwd_residual: res + DropPath_b(Dropout(conv(x, w) + bias)); sample b = rows_per_sample consecutive output
    pixels, kept by the per-sample hash of fs_residual_droppath (transformer_ref.residual_droppath)"""
    v = conv2d_fwd(x, w, bias, stride, pad, dil, drop_p, drop_key)
    return R.residual_droppath(res, v, rows_per_sample * v.shape[-1], droppath_p, droppath_key)


def conv2d_bwd_data_bnsum(dy, w, H, W, stride=1, pad=0, dil=1, bn_y=None, bn_bits=None, bn_mean=None, bn_invstd=None,
                          add_src=None, add_bits=None):
    """fs_conv2d_bwd_data_bnsum: dx = bwd-data [+ add_src where add_bits (all where None)], and the BatchNorm-backward sums of
    the layer whose output gradient dx is, as fs_bn_bwd_partial's slab adds up (elementwise_ref.bn_bwd_sums): S = sum g,
    SX = sum g * xhat over the pixels, g = dx where bn_bits (all where None).  Returns dx, S, SX (None, None without bn_y)."""
    dx = conv2d_bwd_data(dy, w, H, W, stride, pad, dil)
    if add_src is not None:
        dx = dx + (add_src if add_bits is None else torch.where(add_bits, add_src, torch.zeros_like(add_src)))
    if bn_y is None:
        return dx, None, None
    C = dx.shape[-1]
    bits = torch.ones(dx.shape, dtype=torch.bool) if bn_bits is None else bn_bits
    S, SX = E.bn_bwd_sums(dx.reshape(-1, C), bits.reshape(-1, C), bn_y.reshape(-1, C), bn_mean, bn_invstd)
    return dx, S, SX


# ------------------------------------------------------------------------------------------------
# bound helpers: sum|terms| and the contraction length of every output element
# ------------------------------------------------------------------------------------------------
def fwd_terms(x, w, stride=1, pad=0, dil=1):
    return conv(x.abs(), w.abs(), stride, pad, dil)


def fwd_count(x, w, stride=1, pad=0, dil=1):
    return conv(torch.ones_like(x), torch.ones_like(w), stride, pad, dil)


def bwd_data_terms(dy, w, H, W, stride=1, pad=0, dil=1):
    return conv2d_bwd_data(dy.abs(), w.abs(), H, W, stride, pad, dil)


def bwd_data_count(dy, w, H, W, stride=1, pad=0, dil=1):
    return conv2d_bwd_data(torch.ones_like(dy), torch.ones_like(w), H, W, stride, pad, dil)


def bwd_weight_terms(x, dy, R_, S_, stride=1, pad=0, dil=1):
    return conv2d_bwd_weight(x.abs(), dy.abs(), R_, S_, stride, pad, dil)


def bwd_weight_count(x, dy, R_, S_, stride=1, pad=0, dil=1):
    return conv2d_bwd_weight(torch.ones_like(x), torch.ones_like(dy), R_, S_, stride, pad, dil)


def flip_transpose(w):
    """the weights of the forward convolution that IS the bwd-data of a stride-1 layer: w'[r,s,k,c] = w[R-1-r, S-1-s, c, k]
    (dx = conv(dy, w', pad' = dil * (R - 1) - pad))"""
    return w.flip(0, 1).permute(0, 1, 3, 2).contiguous()


# Minimal filtering along the image row (csrc/conv_wino.hip F(2,3), csrc/conv_wino4.hip F(4,3)): m outputs of a row come from
# m + 2 transform-domain products, out = A^T [(G g) * (B^T d)], d_t = x[m j - 1 + t].  WINO_SIGNED holds the kernels' transform
# constants as their two file headers state them (tests/test_conv_ref.py: with them the identity reproduces the convolution);
# WINO holds their absolute values, with which the products' sum|terms| in the transform domain is
#     W[b, y, m*j + o, k] = sum_c |A^T|[o, c] * sum_{ky, ci} (|B^T| |d|)_c * (|G| |g|)_c .
WINO_SIGNED = {
    2: dict(BT=[[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
            G=[[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]],
            AT=[[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: dict(BT=[[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
            G=[[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
            AT=[[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
}
WINO = {m: {n: [[abs(v) for v in row] for row in t] for n, t in k.items()} for m, k in WINO_SIGNED.items()}


def wino_conv(x, w, m, tables=None):
    """A 3x3 / stride-1 / pad-1 forward as F(m,3) along the row (W a multiple of m) with the given transform tables (default:
    the signed constants -- then this IS the convolution, up to rounding)."""
    k = WINO_SIGNED[m] if tables is None else tables
    BT, G, AT = (torch.tensor(k[n], dtype=x.dtype) for n in ("BT", "G", "AT"))
    B, H, W, Cin = x.shape
    assert W % m == 0 and tuple(w.shape[:2]) == (3, 3)
    nq = W // m
    xp = torch.zeros(B, H + 2, W + m + 2, Cin, dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    win = torch.stack([xp[:, :, t:t + m * nq:m] for t in range(m + 2)], dim=3)          # (B, H+2, nq, m+2, Cin): d_t of tile j
    T = torch.einsum("ct,byjti->byjci", BT, win)                                          # (B, H+2, nq, m+2, Cin)
    Uw = torch.einsum("cs,rsik->rcik", G, w)                                              # (3, m+2, Cin, Cout)
    M = torch.zeros(B, H, nq, m + 2, w.shape[3], dtype=x.dtype)
    for r in range(3):
        M += torch.einsum("byjci,cik->byjck", T[:, r:r + H], Uw[r])
    out = torch.einsum("oc,byjck->byjok", AT, M)                                           # (B, H, nq, m, Cout)
    return out.reshape(B, H, W, -1)


def wino_fwd_terms(x, w, m):
    """sum|terms| of a 3x3 / stride-1 / pad-1 forward run as F(m,3) along the row (W a multiple of m): the transform-domain
    products of every output, weighted by the output transform.  x (B,H,W,Cin) and w (3,3,Cin,Cout) enter by absolute value."""
    return wino_conv(x.abs(), w.abs(), m, WINO[m])


def wino_wgrad_terms(x, dy):
    """sum|terms| of a 3x3 / stride-1 / pad-1 weight gradient formed in the F(2,3) transform domain (csrc/conv_wgrad.hip,
    conv_wgrad_wino_kernel): dU_c = sum over pixel pairs of T_c * dM_c with T = B^T d, dM = (e0, e0 + e1, e0 - e1, -e1),
    dW[ky][0] = dU0 + (dU1 + dU2) / 2, dW[ky][1] = (dU1 - dU2) / 2, dW[ky][2] = (dU1 + dU2) / 2 + dU3, all by absolute value
    (|T1| and |T2|, |dM1| and |dM2| have one bound each, so the halves add up to one dU1')."""
    B, H, W, Cin = x.shape
    assert W % 2 == 0
    nq = W // 2
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x.abs()
    d = [xp[:, :, t:t + 2 * nq:2] for t in range(4)]
    T = [d[0] + d[2], d[1] + d[2], d[1] + d[3]]                       # components 0, 1 (= 2), 3
    e0, e1 = dy.abs()[:, :, 0::2], dy.abs()[:, :, 1::2]
    dM = [e0, e0 + e1, e1]
    dw = torch.zeros(3, 3, Cin, dy.shape[3], dtype=x.dtype)
    for r in range(3):
        dU = [torch.einsum("byjc,byjk->ck", T[c][:, r:r + H], dM[c]) for c in range(3)]
        dw[r, 0], dw[r, 1], dw[r, 2] = dU[0] + dU[1], dU[1], dU[1] + dU[2]
    return dw
