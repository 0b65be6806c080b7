"""Helpers shared by the C-ABI kernel tests (tests/test_elementwise_kernels.py, tests/test_transformer_kernels.py): guarded,
pre-filled output buffers and the bound / bit-equality checks.  Not a test module and not a conftest."""
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


def randint(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def choice(gen, vals, *shape):
    return torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), shape, generator=gen)]


def randn(gen, *shape):
    return f32(torch.randn(*shape, generator=gen, dtype=torch.float64))
