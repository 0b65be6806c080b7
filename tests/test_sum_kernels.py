"""The small sum kernels of csrc/elementwise.hip at the C ABI: fs_colsum (bias gradients), fs_add_n (the gradient sum at a tensor
with several consumers) and fs_relu_bwd.  Rules as in tests/test_elementwise_kernels.py (helpers from tests/kernel_testing.py):
every output and the scratch is an `Out` with guards and fill, the scratch exactly as large as the query says, nothing is
compared against the code under test and no bound is a bare relative tolerance.

fs_colsum     "int" data (every sum below 2^24) BIT-EQUAL to fp64; "float" data: a sum of M terms in any order has at most
              M - 1 additions on the path of a term: |got - ref| <= (M - 1) u sum|x| per column (with the accumulating target as
              one more term: M u (sum|x| + |out0|)).  The cases walk the row plan of the 16-byte kernel (colsum4_kernel over
              RowWalk: 256 / (C / 4) rows per trip, rows_per_block_for) and the scalar kernel (C % 4 != 0 or C > 1024), and the
              one path ops.colsum cannot reach: a base pointer that is not 16-byte aligned with C % 4 == 0, where the scalar
              kernel runs on scratch sized for the 16-byte plan -- the guards and the fill left behind the scalar plan's rows
              (scalar_plan below, a hand copy of colsum_plan: keep it in step) decide whether it stays inside.
fs_add_n      bit-equal to the left-to-right fp32 sum formed on the CPU (IEEE addition, no reassociation), 2, 3 and 4 operands,
              out aliasing a, n = 4 and one trip past the grid cap of 8192 blocks.
fs_relu_bwd   g == dout bit for bit where out > 0 and +0 elsewhere, out over {-1, -0, +0, the smallest denormal, 1, +inf, NaN},
              dout with NaN and both infinities; n = 4 and one trip past the cap of 4096 blocks.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fovealseg  # noqa: E402
from kernel_testing import DEV, U, Out, check, dev, exact, randint, randn, report  # noqa: E402

hip = fovealseg.hip
HipError = fovealseg.hip.HipLibraryError


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================
# fs_colsum
# ================================================================================================
def scalar_plan(M):
    """row blocks of colsum_kernel (colsum_plan with vec = false, csrc/elementwise.hip)"""
    chunks = min(cdiv(M, 256), 512)
    return cdiv(M, cdiv(M, chunks))


#               M     C   misaligned  what
COLSUM_CASES = [(5, 4, 0, "256 rows per trip exceed M"),
                (77, 1024, 0, "one row per trip"),
                (300, 52, 0, "19 rows per trip, ragged"),
                (1031, 64, 0, "two rows per thread, the second block ragged"),
                (300, 51, 0, "scalar kernel"),
                (40, 1028, 0, "scalar kernel, five column blocks"),
                (513, 8, 1, "base one float into an aligned buffer with C % 4 == 0: the scalar kernel on the 16-byte plan's scratch")]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("M,C,mis,what", COLSUM_CASES, ids=[f"{m}x{c}{'-misaligned' if a else ''}" for m, c, a, _ in COLSUM_CASES])
def test_colsum(M, C, mis, what, kind):
    gen = torch.Generator().manual_seed(M * 1031 + C)
    x = randint(gen, -3, 3, M, C) if kind == "int" else randn(gen, M, C)
    assert M * 3 + 4 < 2 ** 24
    buf = torch.zeros(M * C + 4, dtype=torch.float32, device=DEV)
    xd = buf[mis:mis + M * C]
    xd.copy_(x.reshape(-1).float())
    assert xd.data_ptr() % 16 == 4 * mis
    nscr = int(hip.load().fs_colsum_scratch_floats(M, C))
    vec_plan = C % 4 == 0 and C <= 1024
    assert nscr % C == 0 and nscr > 0
    written = scalar_plan(M) * C if (mis or not vec_plan) else nscr      # floats of partial sums the launch leaves
    if not mis:
        assert written == nscr
    ref, terms = x.sum(0), x.abs().sum(0)
    for accumulate in (0, 1):
        out0 = ((torch.arange(C) % 7) - 3).double() if accumulate else None
        out, scratch = Out(C, body=out0), Out(nscr)
        hip.call("fs_colsum", hip.ptr(xd), M, C, out.ptr, accumulate, scratch.ptr)
        part = scratch.get(complete=not mis)
        assert int(torch.isnan(part).sum()) == nscr - written and not bool(torch.isnan(part[:written]).any()), \
            f"{int(torch.isnan(part).sum())} of {nscr} scratch floats unwritten, expected {nscr - written}"
        got = out.get(complete=not accumulate)
        tag = f"{M}x{C}{' misaligned' if mis else ''} {kind}{' accumulate' if accumulate else ''}"
        if kind == "int":
            exact("colsum", tag, got, ref + (out0 if accumulate else 0))
            exact("colsum", tag + " partial sums", part[:written].double().reshape(-1, C).sum(0), ref)
            report("colsum", tag, 0.0)
        elif accumulate:
            check("colsum", tag, got, ref + out0, M * U * (terms + out0.abs()))
        else:
            check("colsum", tag, got, ref, (M - 1) * U * terms)


def test_colsum_rejections():
    x = dev(torch.ones(8, 4, dtype=torch.float64))
    for args in ((None, 8, 4, True, True), (x, 8, 4, False, True), (x, 8, 4, True, False), (x, 0, 4, True, True), (x, 8, 0, True, True)):
        out, scratch = Out(4), Out(16)
        a = list(args)
        a[0], a[3], a[4] = hip.ptr(a[0]), (out.ptr if a[3] else None), (scratch.ptr if a[4] else None)
        with pytest.raises(HipError, match="rejected"):
            hip.call("fs_colsum", a[0], a[1], a[2], a[3], 0, a[4])
        assert out.untouched() and scratch.untouched()
    assert int(hip.load().fs_colsum_scratch_floats(0, 4)) == 0 and int(hip.load().fs_colsum_scratch_floats(8, 0)) == 0


# ================================================================================================
# fs_add_n
# ================================================================================================
ADD_CAP = 8192 * 256 * 4        # floats one trip of the capped grid covers


@pytest.mark.parametrize("n", [4, ADD_CAP + 4], ids=["n4", "past-the-grid-cap"])
def test_add_n(n):
    gen = torch.Generator().manual_seed(n)
    ops_ = [torch.randn(n, generator=gen, dtype=torch.float32) * (10.0 ** k) for k in (0, 3, -2, 1)]      # magnitudes that make the order visible
    devs = [t.to(DEV) for t in ops_]
    for nop in (2, 3, 4):
        want = ops_[0] + ops_[1]
        for t in ops_[2:nop]:
            want = want + t
        ptrs = [hip.ptr(t) for t in devs[:nop]] + [None] * (4 - nop)
        out = Out(n)
        hip.call("fs_add_n", *ptrs, out.ptr, n)
        exact("add_n", f"n {n} operands {nop}", out.get(), want)
        alias = Out(n, body=ops_[0])          # out aliases a
        hip.call("fs_add_n", alias.ptr, *ptrs[1:], alias.ptr, n)
        exact("add_n", f"n {n} operands {nop} out = a", alias.get(complete=False), want)
    if n > 4:          # the data can tell the orders apart
        assert not torch.equal((ops_[0] + ops_[1]) + ops_[2], ops_[0] + (ops_[1] + ops_[2]))


def test_add_n_rejections():
    a, b, d = (dev(torch.ones(8, dtype=torch.float64)) for _ in range(3))
    for args in ((hip.ptr(a), hip.ptr(b), None, hip.ptr(d), 8), (hip.ptr(a), hip.ptr(b), None, None, 6), (hip.ptr(a), hip.ptr(b), None, None, 0),
                 (None, hip.ptr(b), None, None, 8), (hip.ptr(a), None, None, None, 8)):
        out = Out(8)
        with pytest.raises(HipError, match="rejected"):
            hip.call("fs_add_n", *args[:4], out.ptr, args[4])
        assert out.untouched()
    with pytest.raises(HipError, match="rejected"):
        hip.call("fs_add_n", hip.ptr(a), hip.ptr(b), None, None, None, 8)


# ================================================================================================
# fs_relu_bwd
# ================================================================================================
RELU_CAP = 4096 * 256 * 4
OUT_VALS = [-1.0, -0.0, 0.0, 2.0 ** -149, 1.0, float("inf"), float("nan")]
DOUT_VALS = [1.5, -2.25, float("nan"), float("inf"), float("-inf"), -0.0, 2.0 ** -149, 3.0e38]
FILL = -12345.5                 # the output legitimately holds NaN: a fill value no input holds


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n,shift", [(4, 0), (4, 4), (RELU_CAP + 4, 0)], ids=["n4-a", "n4-b", "past-the-grid-cap"])
def test_relu_bwd(n, shift):
    """element i: out = OUT_VALS[(i + shift) mod 7], dout = DOUT_VALS[((i + shift) div 7) mod 8] -- every pair within 56 elements;
    the two n = 4 runs cover the seven values of out between them"""
    i = torch.arange(n) + shift
    out = torch.tensor(OUT_VALS, dtype=torch.float32)[i % 7]
    dout = torch.tensor(DOUT_VALS, dtype=torch.float32)[(i // 7) % 8] if n > 4 else torch.tensor(DOUT_VALS, dtype=torch.float32)[(i + 2) % 8]
    assert float(out[out == out].min()) == -1.0 and float(torch.tensor(2.0 ** -149, dtype=torch.float32)) > 0
    g = Out(n, fill=FILL)
    od, dd = out.to(DEV), dout.to(DEV)
    hip.call("fs_relu_bwd", hip.ptr(dd), hip.ptr(od), g.ptr, n)
    got = g.get()
    want = torch.where(out > 0, dout, torch.zeros_like(dout))          # NaN > 0 is false: +0
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"relu_bwd n {n}: NaN in {int((torch.isnan(got) != nan).sum())} wrong places"
    bad = (bits(got) != bits(want)) & ~nan
    assert not bool(bad.any()), f"relu_bwd n {n}: {int(bad.sum())} elements differ bit for bit; first at {int(bad.nonzero()[0])}"
    if n > 4:
        pairs = {(int(a), int(b)) for a, b in zip((i % 7)[:56].tolist(), ((i // 7) % 8)[:56].tolist())}
        assert len(pairs) == 56
    report("relu_bwd", f"n {n} shift {shift}", 0.0)


def test_relu_bwd_rejections():
    a, b = (dev(torch.ones(8, dtype=torch.float64)) for _ in range(2))
    for args in ((None, hip.ptr(b), 8), (hip.ptr(a), None, 8), (hip.ptr(a), hip.ptr(b), 6), (hip.ptr(a), hip.ptr(b), 0)):
        g = Out(8)
        with pytest.raises(HipError, match="rejected"):
            hip.call("fs_relu_bwd", args[0], args[1], g.ptr, args[2])
        assert g.untouched()
