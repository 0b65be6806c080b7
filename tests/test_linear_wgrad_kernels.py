"""fs_linear_bwd_weight_bias (the host code in csrc/conv.hip, linear_wgrad_kernel in csrc/conv_wgrad.hip) at the C ABI against the
plain fp64 reference oracle/conv_ref.linear_wgrad_ref (which tests/test_conv_ref.py holds to the autograd of F.linear on the CPU).

The rules are those of tests/test_conv_kernels.py (helpers shared through tests/kernel_testing.py):
  * dW, dbias and the deterministic mode's scratch are `Out`s: guards of sentinel on both sides, the body pre-filled with NaN (a
    visible integer pattern for an accumulating target); the scratch is EXACTLY fs_linear_bwd_weight_bias_ws_bytes bytes;
  * ONE case table (CASES).  A row states the tile variant of linear_wgrad_kernel (1 = 64 x 64, 2 = 64 x 128, 3 = 128 x 64,
    4 = 128 x 128, Cin x Cout), the number of row splits, the rows per split and the length of the last split.  What the host
    queries can see of that is asserted before every launch (assert_row), and test_case_table_reaches_every_tile_and_reduce
    (no GPU) proves the coverage from the queries alone.  The plan is read through fs_conv2d_bwd_weight_plan of the same layer
    as a 1x1 convolution over (rows, 1, 1) pixels -- route 6 runs plan_linear with the same slab cap as the fused entry point:
    in deterministic mode out[5] is the split count and workgroups / splits the tile count; in the default mode workgroups /
    tiles is the split count.  The tile COUNT tells the variants apart wherever they differ in it (both rows with wide
    operands: 35 / 117 tiles); for operands of at most 64 channels all variants that cover the operand have the same count,
    and there tile_rule -- a hand copy of the first lines of plan_linear, keep it in step -- is the only witness;
  * three kinds of data per case:
      "int"   small integers, every sum below 2^24: dW and dbias BIT-EQUAL to fp64 with atomics and with slabs, for all four
              (accumulate_w, accumulate_b); a dropped 32-row chunk, a bias slab summed twice or skipped changes an integer;
      "width" one operand with full 24-bit significands (last mantissa bit set), the other one-hot per output with a power of
              two (row co mod rows of column co), both ways round: every dW element is ONE product, a bit-exact scaled copy; a
              lost third bf16 plane is off by 2^-16 relative.  dbias is the power of two itself (exact) where dy is the
              one-hot operand, a sum of wide values (held to its bound) the other way round;
      "float" randn rounded to fp32: |dW - ref| <= L u |x|^T |dy| for EVERY element, L = 6 rows + 3 + splits + 1: six
              accumulator additions per product (the six plane products of bf16x3), 3 u of split error per product (P_STEPS,
              S_SPLIT of kernel_testing.py, derived in the header of tests/test_conv_kernels.py), one addition per split (an
              atomic, or a slab row of the ordered sum) and one for the accumulating target.  An accumulating dW adds, per
              addition that carries the target's value (every split's atomic; the one last addition of the ordered sum),
              u |dW0|.  dbias: any summation of `rows` terms in any order has at most rows - 1 additions on the path of a
              term: |dbias - ref| <= rows u sum|dy| (with the accumulating target as one more term: rows u (sum|dy| + |db0|)).
              L grows with the row count while random errors do not (measured ratios 0.013 at 17 rows, below 0.0001 from 1000
              rows up, profiles/r24/README.md), so on the long cases one dropped chunk hides inside this bound: "int" is what
              catches it.
    No bound comes from the kernel's output;
  * deterministic mode: two calls are bit-identical and stay within the same bounds; after the call the whole scratch is
    written (the memset covers it), the dW slabs behind the plan's splits and the bias slabs behind 4 x splits are still the
    memset's zeros, and on integer data the 4 x splits bias slabs (which the ordered sum leaves in place) add up to dbias.

Operands of 2 GiB and more are out of scope here (the entry point refuses 4 GB; nothing between is tested).
"""
import ctypes

import pytest
import torch

import fovealseg  # noqa: E402
import conv_ref as C  # noqa: E402
from kernel_testing import U, Out, check, dev, direct_bound, exact, pow2, precision, randint, randn, report, wide  # noqa: E402

hip = fovealseg.hip
HipError = fovealseg.hip.HipLibraryError
gpu = pytest.mark.gpu
MODE = "bf16x3"                            # the only mode the fused launch exists in
TILE_CI, TILE_CO = [0, 64, 64, 128, 128], [0, 64, 128, 64, 128]


def cdiv(a, b):
    return -(-a // b)


class Row:
    def __init__(self, rows, Cin, Cout, tile, splits, per, last, why):
        self.rows, self.Cin, self.Cout, self.tile, self.splits, self.per, self.last, self.why = rows, Cin, Cout, tile, splits, per, last, why
        self.n = Cin * Cout
        self.id = f"{rows}x{Cin}x{Cout}"

    @property
    def tiles(self):
        return cdiv(self.Cin, TILE_CI[self.tile]) * cdiv(self.Cout, TILE_CO[self.tile])

    @property
    def two_stage(self):
        """fs_slab_reduce_inplace (csrc/elementwise.hip) first folds the dW slabs into the first eight, in place"""
        return self.splits >= 32 and self.n > 4096 and self.splits * self.n >= 2 ** 22


#        rows  Cin  Cout tile splits per last
CASES = [
    Row(17, 16, 16, 1, 1, 32, 17, "fewer rows than one 32-row chunk, at the channel minimum"),
    Row(100, 20, 36, 1, 4, 32, 4, "last split of 4 rows; channels multiples of 4 but not of 32"),
    Row(75, 48, 132, 2, 3, 32, 11, "two column tiles, the second 4 wide"),
    Row(75, 132, 48, 3, 3, 32, 11, "the mirror of the previous row"),
    Row(1000, 48, 96, 2, 32, 32, 8, "128 bias slabs: the bias sum takes the wave reduce"),
    Row(7168, 516, 772, 4, 10, 736, 544, "35 tiles of 128 x 128, ragged on both sides"),
    Row(7167, 516, 772, 1, 8, 896, 895, "the same layer one row below the tile threshold: 117 tiles of 64 x 64"),
    Row(65536, 256, 256, 4, 86, 768, 256, "the two-stage in-place slab reduce: 86 slabs of 65536 elements"),
]
IDS = [c.id for c in CASES]


# ================================================================================================
# host-side queries (no launch; these run on a machine without a GPU)
# ================================================================================================
def lib():
    return hip.load()


def tile_rule(rows, Cin, Cout):
    """the tile choice of plan_linear (csrc/conv_wgrad.hip) for plain rows.  A hand copy: keep it in step with that function."""
    if Cin <= 64 and Cout <= 64:
        return 1
    if Cin <= 64:
        return 2
    if Cout <= 64:
        return 3
    nsplit = max(512 // (cdiv(Cin, 128) * cdiv(Cout, 128)), 1)
    return 4 if rows // nsplit >= 512 else 1


def conv_plan(c):
    """fs_conv2d_bwd_weight_plan of the layer as a 1x1 convolution, at the scratch that entry point asks for in the current modes
    -> (route, accumulation kind, launches, workgroups, threads, slab rows), the slab cap of the layer"""
    nbytes = int(lib().fs_conv2d_bwd_weight_ws_bytes(c.Cin, c.Cout, 1, 1, 1, 0, 1))
    out = (ctypes.c_int * 6)()
    ok = lib().fs_conv2d_bwd_weight_plan(c.rows, 1, 1, c.Cin, 1, 1, c.Cout, 1, 1, 1, 0, 1, nbytes, out)
    assert ok == 1 and nbytes % (4 * c.n) == 0, (c.id, ok, nbytes)
    return tuple(int(v) for v in out), nbytes // (4 * c.n)


def ws_bytes(c):
    return int(lib().fs_linear_bwd_weight_bias_ws_bytes(c.Cin, c.Cout))


def assert_row(c):
    """what the row states, against the queries in both modes (the tile choice does not depend on the mode); leaves the
    library in its default modes.  Returns the slab cap of the layer."""
    assert c.per % 32 == 0 and cdiv(c.rows, c.per) == c.splits and c.last == c.rows - (c.splits - 1) * c.per and 0 < c.last <= c.per, c.id
    assert c.tile == tile_rule(c.rows, c.Cin, c.Cout), c.id
    with precision(MODE, True):
        (route, accum, launches, wgs, threads, slabs), cap = conv_plan(c)
        assert (route, accum, launches, threads) == (6, 2, 1, 256), (c.id, route, accum, launches, threads)
        assert slabs == c.splits and wgs == c.tiles * c.splits and slabs <= cap, (c.id, wgs, slabs, cap)
        assert ws_bytes(c) == cap * (c.n + 4 * c.Cout) * 4, c.id
        assert int(lib().fs_linear_bwd_weight_bias_ok(c.rows, c.Cin, c.Cout)) == 1
    with precision(MODE, False):
        (route, accum, launches, wgs, threads, slabs), cap0 = conv_plan(c)
        assert (route, accum, launches, threads, slabs, cap0) == (6, 0, 1, 256, 0, 0), (c.id, route, accum, launches, threads, slabs, cap0)
        assert wgs == c.tiles * c.splits, (c.id, wgs)
        assert ws_bytes(c) == 0
        assert int(lib().fs_linear_bwd_weight_bias_ok(c.rows, c.Cin, c.Cout)) == 1
    return cap


def test_case_table_reaches_every_tile_and_reduce():
    """From the host-side queries alone (no launch): every row is on route 6 with the tile count and split count it states, in
    both modes; the table holds every tile variant -- tiles 4 and 1 on a layer whose tile count (35 / 117) no other variant
    gives --, a single split, a last split that is no multiple of 32 rows, both bias reduce kernels (fs_slab_reduce,
    csrc/elementwise.hip: the wave kernel for more than 64 slabs, here 4 x splits, else the plain one) and both forms of the dW
    reduce (two-stage in place, plain).  The fused launch exists in bf16x3 only."""
    for c in CASES:
        assert_row(c)
        for mode in ("f32", "f16x2"):
            with precision(mode):
                assert int(lib().fs_linear_bwd_weight_bias_ok(c.rows, c.Cin, c.Cout)) == 0
    assert {c.tile for c in CASES} == {1, 2, 3, 4}
    for t in (1, 4):      # identified by the tile count alone
        assert any(c.tile == t and all(cdiv(c.Cin, TILE_CI[o]) * cdiv(c.Cout, TILE_CO[o]) != c.tiles for o in (1, 2, 3, 4) if o != t) for c in CASES), t
    assert any(c.splits == 1 for c in CASES)
    assert any(c.last % 32 != 0 and c.splits > 1 for c in CASES)
    assert any(4 * c.splits > 64 for c in CASES) and any(1 < 4 * c.splits <= 64 for c in CASES)
    assert any(c.two_stage for c in CASES) and any(not c.two_stage and c.splits > 1 for c in CASES)
    assert any(c.Cin % 32 and c.Cout % 32 for c in CASES)
    with precision(MODE):
        for rows, Cin, Cout in ((100, 12, 36), (100, 18, 36), (100, 20, 12), (100, 20, 18), (0, 20, 36), (-1, 20, 36)):
            assert int(lib().fs_linear_bwd_weight_bias_ok(rows, Cin, Cout)) == 0, (rows, Cin, Cout)


# ================================================================================================
# data: made once per test, never modified
# ================================================================================================
def gen_for(c, salt):
    return torch.Generator().manual_seed((c.rows * 131 + c.Cin) * 131 + c.Cout + salt)


def one_hot(gen, rows, Ch):
    """column ch holds a single non-zero, a power of two, in row ch mod rows"""
    t = torch.zeros(rows, Ch, dtype=torch.float64)
    ch = torch.arange(Ch)
    t[ch % rows, ch] = pow2(gen, Ch)
    return t


def make(c, kind):
    g = gen_for(c, {"int": 1, "float": 2, "widthA": 3, "widthB": 4}[kind])
    if kind == "int":
        x, dy = randint(g, -2, 2, c.rows, c.Cin), randint(g, -2, 2, c.rows, c.Cout)
        assert c.rows * 4 + 3 < 2 ** 24
    elif kind == "float":
        x, dy = randn(g, c.rows, c.Cin), randn(g, c.rows, c.Cout)
    elif kind == "widthA":
        x, dy = wide(randn(g, c.rows, c.Cin)), one_hot(g, c.rows, c.Cout)
    else:
        x, dy = one_hot(g, c.rows, c.Cin), wide(randn(g, c.rows, c.Cout))
    dw, db = C.linear_wgrad_ref(x, dy)
    tw, tb = C.linear_wgrad_terms(x, dy) if kind in ("float", "widthB") else (None, None)
    return dict(x=x, dy=dy, xd=dev(x), dyd=dev(dy), dw=dw.reshape(-1), db=db, tw=None if tw is None else tw.reshape(-1), tb=tb)


def pattern(n, m):
    return ((torch.arange(n) % m) - m // 2).double()


def check_scratch(c, ws, cap, d, exact_bias):
    """deterministic mode, after the call: guards untouched, no fill value left (the memset covers all of it), the slabs behind
    the plan's still zero; exact_bias: the 4 x splits bias slabs add up to the column sums"""
    left = ws.rows_left(c.Cout)
    assert int(left.sum()) == 0, f"{c.id}: {int((left > 0).sum())} scratch rows hold unwritten elements"
    dws = ws.t[:cap * c.n].reshape(cap, c.n)
    bias = ws.t[cap * c.n:].reshape(4 * cap, c.Cout)
    assert not bool(dws[c.splits:].any()), f"{c.id}: dW slabs behind the plan's {c.splits} were written"
    assert not bool(bias[4 * c.splits:].any()), f"{c.id}: bias slabs behind the plan's {4 * c.splits} were written"
    if exact_bias:
        exact("linear_wgrad", f"{c.id} bias slabs", bias[:4 * c.splits].double().sum(0).cpu(), d["db"])


def run(c, d, acc_w, acc_b, det, cap, exact_bias=False):
    """one call in the current modes -> dW, dbias on the host, the accumulating targets' start values"""
    dw0, db0 = (pattern(c.n, 7) if acc_w else None), (pattern(c.Cout, 5) if acc_b else None)
    dw, db = Out(c.n, body=dw0), Out(c.Cout, body=db0)
    nbytes = ws_bytes(c)
    assert (nbytes > 0) == det and nbytes % 4 == 0
    ws = Out(nbytes // 4) if det else None
    hip.call("fs_linear_bwd_weight_bias", hip.ptr(d["xd"]), hip.ptr(d["dyd"]), dw.ptr, db.ptr, c.rows, c.Cin, c.Cout, acc_w, acc_b,
             ws.ptr if ws else None, nbytes)
    if ws is not None:
        check_scratch(c, ws, cap, d, exact_bias)
    return dw.get(complete=not acc_w), db.get(complete=not acc_b), dw0, db0


def tag(c, kind, acc_w, acc_b, det):
    return f"{c.id} tile {c.tile} splits {c.splits} {kind} acc {acc_w}{acc_b}{' det' if det else ''}"


# ================================================================================================
# the three kinds of data
# ================================================================================================
@gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_linear_wgrad_int(ci):
    c = CASES[ci]
    cap = assert_row(c)
    d = make(c, "int")
    for det in (False, True):
        with precision(MODE, det):
            for acc_w in (0, 1):
                for acc_b in (0, 1):
                    dw, db, dw0, db0 = run(c, d, acc_w, acc_b, det, cap, exact_bias=True)
                    t = tag(c, "int", acc_w, acc_b, det)
                    exact("linear_wgrad", t + " dW", dw, d["dw"] + (dw0 if acc_w else 0))
                    exact("linear_wgrad", t + " dbias", db, d["db"] + (db0 if acc_b else 0))
                    report("linear_wgrad", t, 0.0)


@gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_linear_wgrad_width(ci):
    c = CASES[ci]
    cap = assert_row(c)
    for kind in ("widthA", "widthB"):
        d = make(c, kind)
        assert int((d["dw"] != 0).sum()) == c.n
        for det in (False, True):
            with precision(MODE, det):
                dw, db, _, _ = run(c, d, 0, 0, det, cap, exact_bias=kind == "widthA")
                t = tag(c, kind, 0, 0, det)
                exact("linear_wgrad", t + " dW", dw, d["dw"])
                if kind == "widthA":
                    exact("linear_wgrad", t + " dbias", db, d["db"])
                    report("linear_wgrad", t, 0.0)
                else:
                    check("linear_wgrad", t + " dbias", db, d["db"], c.rows * U * d["tb"])


@gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_linear_wgrad_float(ci):
    c = CASES[ci]
    cap = assert_row(c)
    d = make(c, "float")
    for det in (False, True):
        with precision(MODE, det):
            for acc in (0, 1):
                dw, db, dw0, db0 = run(c, d, acc, acc, det, cap)
                t = tag(c, "float", acc, acc, det)
                bw = direct_bound(1, c.rows, d["tw"], 0.0, 0.0, c.splits + 1)
                bb = c.rows * U * d["tb"]
                if acc:
                    bw = bw + (1 if det else c.splits) * U * dw0.abs()
                    bb = c.rows * U * (d["tb"] + db0.abs())
                check("linear_wgrad", t + " dW", dw, d["dw"] + (dw0 if acc else 0), bw)
                check("linear_wgrad", t + " dbias", db, d["db"] + (db0 if acc else 0), bb)
                if det:
                    dw2, db2, _, _ = run(c, d, acc, acc, det, cap)
                    assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{t}: two deterministic calls differ"


# ================================================================================================
# rejections: FS_ERR_ARG, nothing launched, every output untouched
# ================================================================================================
@gpu
def test_linear_wgrad_rejections():
    c = CASES[1]
    assert_row(c)
    d = make(c, "int")
    x, dy = hip.ptr(d["xd"]), hip.ptr(d["dyd"])

    def refused(what, mode, det, args, ok, ws_floats=0, ws_bytes_=0):
        """args = (x, dy, dw given?, dbias given?, rows, Cin, Cout); ok = what fs_linear_bwd_weight_bias_ok says of the shape"""
        with precision(mode, det):
            dw, db = Out(c.n), Out(c.Cout)
            ws = Out(ws_floats) if ws_floats else None
            a = list(args)
            a[2], a[3] = (dw.ptr if a[2] else None), (db.ptr if a[3] else None)
            assert int(lib().fs_linear_bwd_weight_bias_ok(*a[4:])) == ok, (what, a[4:])
            with pytest.raises(HipError, match="rejected"):
                hip.call("fs_linear_bwd_weight_bias", *a, 0, 0, ws.ptr if ws else None, ws_bytes_)
            assert dw.untouched() and db.untouched() and (ws is None or ws.untouched()), what

    shape = (c.rows, c.Cin, c.Cout)
    refused("precision f32", "f32", False, (x, dy, True, True) + shape, 0)
    refused("precision f16x2", "f16x2", False, (x, dy, True, True) + shape, 0)
    refused("Cin = 12", MODE, False, (x, dy, True, True, c.rows, 12, c.Cout), 0)
    refused("Cin = 18", MODE, False, (x, dy, True, True, c.rows, 18, c.Cout), 0)
    refused("rows = 0", MODE, False, (x, dy, True, True, 0, c.Cin, c.Cout), 0)
    for k in range(4):
        a = [x, dy, True, True]
        a[k] = None if k < 2 else False
        refused(f"null pointer {k}", MODE, False, tuple(a) + shape, 1)
    with precision(MODE, True):
        nbytes = ws_bytes(c)
    assert nbytes > 0 and nbytes % 4 == 0
    refused("deterministic, ws = NULL", MODE, True, (x, dy, True, True) + shape, 1, ws_bytes_=nbytes)
    refused("deterministic, one byte too little", MODE, True, (x, dy, True, True) + shape, 1, ws_floats=nbytes // 4, ws_bytes_=nbytes - 1)
    # ... and the same scratch with every byte is taken
    with precision(MODE, True):
        dw, db, ws = Out(c.n), Out(c.Cout), Out(nbytes // 4)
        hip.call("fs_linear_bwd_weight_bias", x, dy, dw.ptr, db.ptr, *shape, 0, 0, ws.ptr, nbytes)
        exact("linear_wgrad", "full scratch dW", dw.get(), d["dw"])
        exact("linear_wgrad", "full scratch dbias", db.get(), d["db"])
