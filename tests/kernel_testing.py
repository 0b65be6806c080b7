"""Helpers shared by the C-ABI kernel tests (tests/test_*_kernels.py): guarded, pre-filled output buffers, the bound /
bit-equality checks, the precision-mode switch and the bound of an MFMA contraction.  Not a test module and not a conftest."""
import math

import torch

import fovealseg

hip = fovealseg.hip
DEV = "cuda"
GUARD = 256                 # floats (1 KiB) of sentinel on both sides of every output
U = 2.0 ** -24              # unit roundoff of fp32

_FILL = {torch.float32: float("nan"), torch.float64: float("nan"), torch.uint8: 0xFF, torch.int32: -9999, torch.int64: -9999}
_SENT = {torch.float32: 777.25, torch.float64: 777.25, torch.uint8: 0xA5, torch.int32: -7777, torch.int64: -7777}


class Out:
    """A device buffer of n elements a kernel writes: guards of GUARD floats' worth of sentinel around it, the body pre-filled
    with `fill` (NaN; a marker for integer types) or with `body` (in-place targets, buffers with slices to be left alone)."""

    def __init__(self, n, dtype=torch.float32, body=None, fill=None):
        self.n, self.dtype = int(n), dtype
        self.g = GUARD * 4 // torch.empty(0, dtype=dtype).element_size()
        self.fill = _FILL[dtype] if fill is None else fill
        self.base = torch.full((self.n + 2 * self.g,), _SENT[dtype], dtype=dtype, device=DEV)
        self.t = self.base[self.g:self.g + self.n]
        if body is None:
            self.t.fill_(self.fill)
        else:
            self.t.copy_(body.reshape(-1).to(dtype))
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return hip.ptr(self.t)

    def _host(self):
        torch.cuda.synchronize()
        b = self.base.cpu()
        s = _SENT[self.dtype]
        assert bool((b[:self.g] == s).all()) and bool((b[self.g + self.n:] == s).all()), "a guard was written"
        return b[self.g:self.g + self.n]

    def get(self, complete=True):
        """the body on the host, after checking the guards and (complete) that no element still holds the fill value"""
        body = self._host()
        if complete:
            left = torch.isnan(body) if isinstance(self.fill, float) and math.isnan(self.fill) else body == self.fill
            assert not bool(left.any()), f"{int(left.sum())} of {self.n} output elements were not written"
        return body

    def untouched(self):
        body = self._host()
        left = torch.isnan(body) if isinstance(self.fill, float) and math.isnan(self.fill) else body == self.fill
        return bool(left.all())

    def rows_left(self, row):
        """For scratch too large to bring to the host (the slab scratch of the bwd-weight kernels): the guards are compared on
        the device, and the body, taken as rows of `row` elements, gives per row how many elements still hold the fill value
        (0 = written completely, row = untouched).  Returns that count per row as a host tensor."""
        torch.cuda.synchronize()
        s = _SENT[self.dtype]
        assert bool((self.base[:self.g] == s).all()) and bool((self.base[self.g + self.n:] == s).all()), "a guard was written"
        assert self.n % row == 0
        body = self.t.reshape(-1, row)
        left = torch.isnan(body) if isinstance(self.fill, float) and math.isnan(self.fill) else body == self.fill
        return left.sum(dim=1).cpu()


def dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).contiguous().to(DEV)


def f32(t):
    """round an fp64 reference value to the fp32 the kernel is given, back in fp64"""
    return t.float().double()


def report(family, what, ratio):
    print(f"[bound] {family} {what} {ratio:.4f}")


def check(family, what, got, ref, bound, ref32=None):
    """|got - ref| <= bound elementwise, or max|got - ref| <= 4 * max|ref32 - ref| (ref32 = the same formula in fp32 on the CPU)"""
    got = got.double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{family} {what}: non-finite output"
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    over = err > bound
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    report(family, what, ratio)
    if bool(over.any()):
        e32 = float((ref32.double().reshape(ref.shape) - ref).abs().max()) if ref32 is not None else 0.0
        assert float(err.max()) <= 4 * e32, (f"{family} {what}: {int(over.sum())} elements over the bound, worst {ratio:.2f}x, "
                                             f"max err {float(err.max()):.3e}, 4 x fp32-CPU error {4 * e32:.3e}")


def exact(family, what, got, ref):
    got, ref = got.reshape(ref.shape), ref.to(got.dtype)
    bad = got != ref
    assert not bool(bad.any()), f"{family} {what}: {int(bad.sum())} of {ref.numel()} elements differ (bit-equal required)"


# ---- the MFMA GEMM kernels: chain constants and the bound of one contraction (derived in the header of tests/test_conv_kernels.py) ----
MODES = ["f32", "bf16x3", "f16x2"]
P_STEPS = {0: 1, 1: 6, 2: 3}              # accumulator additions per product
S_SPLIT = {0: 0, 1: 3, 2: 12}             # the split's own error, in u |x y| per product
F16_FLOOR = 2.0 ** -37                    # the floor of a two-plane fp16 operand per product, times max|x| max|w|


def direct_bound(a, count, terms, amax, bmax, extra):
    """(P n + S + extra) u sum|terms| [+ n * F16_FLOOR max|x| max|w| in f16x2] per element; a = 0 fp32, 1 bf16x3, 2 f16x2"""
    b = (P_STEPS[a] * count + S_SPLIT[a] + extra) * U * terms
    return b + (count * F16_FLOOR * amax * bmax if a == 2 else 0.0)


class precision:
    """the library's precision (and deterministic) mode for the duration of a with-block"""

    def __init__(self, mode, det=False):
        self.mode, self.det = mode, det

    def __enter__(self):
        hip.set_conv_precision(self.mode)
        hip.set_deterministic(self.det)

    def __exit__(self, *exc):
        hip.set_deterministic(False)
        hip.set_conv_precision(hip.default_conv_precision())


def wide(t):
    """fp32 values with the last mantissa bit set: full 24-bit significands"""
    b = t.float().contiguous().view(torch.int32) | 1
    return b.view(torch.float32).double()


def pow2(gen, *shape):
    """+- 2^j, j in -2 .. 2"""
    return (2.0 ** torch.randint(-2, 3, shape, generator=gen).double()) * (torch.randint(0, 2, shape, generator=gen).double() * 2 - 1)


def randint(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def choice(gen, vals, *shape):
    return torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), shape, generator=gen)]


def randn(gen, *shape):
    return f32(torch.randn(*shape, generator=gen, dtype=torch.float64))
