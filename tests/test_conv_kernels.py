"""The convolution engine (csrc/conv*.hip) at the C ABI against the plain fp64 references of oracle/conv_ref.py (which
tests/test_conv_ref.py holds to torch on the CPU).

The rules are those of tests/test_elementwise_kernels.py and tests/test_transformer_kernels.py (helpers shared through
tests/kernel_testing.py):
  * every output, the weight-pack scratch, the stats / BatchNorm slabs and the bwd-weight slab scratch is an `Out`: guards of
    sentinel on both sides, the body pre-filled with NaN (0xFF bytes for the pack scratch, a visible integer pattern for an
    accumulating dW); after the call no fill value is left where an output is due and the guards are untouched;
  * ONE case table (CASES), one row per launch path of plan_conv (csrc/conv.hip) / route of fs_wgrad_plan (csrc/conv_wgrad.hip).
    A row records what the host-side queries answer for it in each precision mode; every GPU test asserts those answers before
    it launches, so a case cannot drift to another path unnoticed, and test_case_table_reaches_every_path (no GPU) proves the
    coverage from the queries alone.  Paths that share a public id are told apart by the conditions of plan_conv (route_of);
  * three kinds of data per case:
      "int"   small integers (weights even, so that the F(2,3) filter transform (g0 +- g1 + g2) / 2 stays integral), every
              sum below 2^24: BIT-EQUAL to fp64 in all three modes on every direct path and on the F(2,3) paths (ids 5,
              bwd-weight route 5: their transform constants are 1 and 1/2).  F(4,3) (id 8) divides by 6 and 24: its filter
              transform is inexact for every integer filter, so id 8 is held to its bound only;
      "width" the operand-width probe: one operand carries full 24-bit significands (random fp32 with the last mantissa bit
              set), the other is one-hot per output with a power-of-two value, so every output is ONE product, a scaled copy
              of the first operand.  f32 and bf16x3 (x = x1 + x2 + x3 exactly, conv_split.h) must reproduce it BIT FOR BIT on
              the direct paths; a split that lost its third plane is off by 2^-16 relative.  f16x2 is held to the error of its
              two-plane split (F16_WIDTH below).  On ids 5 / 8 the transform mixes neighbours: held to the derived bound;
      "float" randn rounded to fp32: |got - ref| <= L * 2^-24 * sum|terms| for EVERY element, L derived below.
    No bound comes from a kernel's output and none is a bare relative tolerance;
  * split modes run forward and bwd-data twice: with the scratch fs_conv2d_workspace_bytes asks for, and with ws = NULL (the
    PLAIN fallback, conv_igemm_split_kernel splitting the weights in flight).

The chain length L (fp32 roundings behind one output element; u = 2^-24):
  n       = the element's contraction length: in-range (tap, channel) products (forward, bwd-data) or pixels (bwd-weight),
            conv_ref.*_count.  Zero padding adds exact zeros and no rounding;
  P       = accumulator additions per product: 1 in fp32 (v_mfma_f32_32x32x2_f32), 6 in bf16x3 (six plane products), 3 in f16x2
            (PrecX3::NTERM, PrecF16::NTERM).  An MFMA adds 16 plane products at once; counting each as one rounding step is
            the upper bound whatever the adder tree inside does.  K-chunks x taps x plane products per step is P * n;
  S       = the split itself, in units of u |x y| per product: bf16x3 drops x2 y3 + x3 y2 + x3 y3 < 3 u |x y| (SPLIT_TERM of
            tests/test_transformer_kernels.py); f16x2 carries 22-bit operands (|dx| <= 2^-22 |x|, below) and drops h2 g2:
            3 * 2^-22 = 12 u;
  +2      bias add and dropout scale (forward), +3 more for scale / shift / residual of the fused epilogues;
  bwd-weight adds the split-K sum: at most one addition per workgroup of the plan (atomics or slab rows) + 1 for accumulate;
  ids 5 / 8, route 5: sum|terms| is taken in the TRANSFORM domain (conv_ref.wino_fwd_terms / wino_wgrad_terms: the products
  the kernel really adds, weighted by |A^T|, so the transform gains are inside it), n = 3 filter rows x channels x (m + 2)
  components, + WINO_ROUND roundings of forming T (<= 3 adds), U (<= 5) and the output transform (<= 6).

Activations (fs_conv2d_fwd_affine_act): the sibling files take the activation's branch from the device's own output.  Here the
branch is not selected at all: ReLU and ReLU6 are 1-Lipschitz, so |act(v_dev) - act(v_ref)| <= |v_dev - v_ref|, and the output
is held to the bound of the activation's ARGUMENT against act(v_ref) whichever branch the device took -- no looser, and no
element near a kink needs special care.

f16x2 (PrecF16::split, conv_split.h): the operand is scaled by a power of two 2^(14 - e), e = the exponent of the maximum of
its SCALING GROUP (an LDS stage, a halo tile, the whole weight tensor: every kernel's own choice, always a set that contains
the element), so |xs| < 2^15; h1 = fp16(xs) leaves |xs| 2^-11, h2 = fp16(xs - h1) leaves |xs| 2^-22 -- or, where the
remainder falls below fp16's normal range, half the subnormal spacing 2^-25 ABSOLUTE in the scaled domain, i.e.
2^-39 * 2^e <= 2^-39 * (group maximum) in the operand's units: a floor relative to the group's maximum, not to the element.
conv_igemm_split_kernel scales the source by 2^(14 - (E - eb)) with E the running maximum of ea + eb over the stages, so its
floor is 2^-39 * 2^(E - eb); times |w| < 2^(eb + 1) that is 2^-38 * 2^E <= 2^-38 max|x| max|w| per product, and as much for the
weight's floor: F16_FLOOR = 2^-37 max|x| max|w| per product covers every kernel's grouping.
"""
import ctypes
import functools

import pytest
import torch

import fovealseg  # noqa: E402
import conv_ref as C  # noqa: E402
import elementwise_ref as E  # noqa: E402
import fovealseg_oracle as O  # noqa: E402
import transformer_ref as R  # noqa: E402
from kernel_testing import (F16_FLOOR, MODES, P_STEPS, S_SPLIT, U, Out, check, dev, direct_bound, exact, f32, pow2, precision,  # noqa: E402,F401
                            report, wide)

hip = fovealseg.hip
HipError = fovealseg.hip.HipLibraryError
gpu = pytest.mark.gpu
# MODES, P_STEPS, S_SPLIT, F16_FLOOR, direct_bound, precision, wide and pow2 live in tests/kernel_testing.py (shared with
# tests/test_linear_wgrad_kernels.py)
F16_WIDTH = 2.0 ** -22                    # relative error of a two-plane fp16 operand
WINO_ROUND = 14                           # roundings of the row transforms (T, U, output), see the header

ROUTES = ["GENERIC", "PLAIN", "HALO", "WINO_F23", "WINO_F43", "TAPSET_FWD", "TAPSET_BWD1", "POINTWISE", "GATHER", "SCATTER", "S2FWD",
          "S2BWD", "PARITY"]
PERSISTENT = {"HALO", "WINO_F23", "WINO_F43", "TAPSET_FWD", "TAPSET_BWD1", "POINTWISE", "GATHER", "S2FWD", "S2BWD"}


class Case:
    """One row: the problem, the path it is there for, and per precision mode what the host-side queries answer at the scratch
    fs_conv2d_workspace_bytes asks for: forward id, bwd-data id, bwd-weight (route, accumulation kind) in the default mode."""

    def __init__(self, shape, path, f32_, bf16x3, f16x2, wgrad_only=False):
        self.B, self.H, self.W, self.Cin, self.Cout, self.k, self.stride = shape[:7]
        self.dil = shape[7] if len(shape) > 7 else 1
        self.pad = self.dil * (self.k - 1) // 2
        self.Ho = C.out_size(self.H, self.k, self.stride, self.pad, self.dil)
        self.Wo = C.out_size(self.W, self.k, self.stride, self.pad, self.dil)
        self.path, self.wgrad_only = path, wgrad_only
        self.expect = dict(zip(MODES, (f32_, bf16x3, f16x2)))
        self.id = "x".join(str(v) for v in shape)

    @property
    def args(self):          # the 12 integers every conv entry point and query takes
        return (self.B, self.H, self.W, self.Cin, self.Ho, self.Wo, self.Cout, self.k, self.k, self.stride, self.pad, self.dil)

    @property
    def aligned(self):
        return self.Cin % 4 == 0 and self.Cout % 4 == 0


# (forward id, bwd-data id, bwd-weight route, accumulation kind).  SCATTER / PARITY, POINTWISE / GATHER and the two tap-class
# forms are named in the path column and derived by route_of.
CASES = [
    Case((1, 5, 7, 32, 32, 3, 1), "HALO, ragged; PLAIN without scratch", (1, 1, 2, 0), (2, 2, 4, 0), (2, 2, 4, 0)),
    Case((2, 9, 11, 64, 96, 3, 1), "HALO, ragged, two channel tiles", (1, 1, 2, 0), (2, 2, 4, 0), (2, 2, 4, 0)),
    Case((2, 18, 18, 64, 64, 3, 1), "WINO_F23 (bf16x3)", (1, 1, 2, 0), (5, 5, 4, 0), (2, 2, 4, 0)),
    Case((4, 16, 16, 64, 64, 3, 1), "WINO_F43 (bf16x3)", (1, 1, 2, 0), (8, 8, 4, 0), (2, 2, 4, 0)),
    Case((2, 20, 20, 256, 256, 3, 1), "WINO_F43 (bf16x3) / WINO_F23 (f16x2); fp32 bwd-weight with 9 taps", (1, 1, 3, 0), (8, 8, 4, 0), (5, 5, 4, 0)),
    Case((1, 6, 6, 16, 16, 3, 1), "TAPSET_FWD / TAPSET_BWD1 at the kernel's 16-channel minimum", (1, 1, 2, 0), (3, 3, 4, 0), (3, 3, 4, 0)),
    Case((1, 7, 9, 32, 32, 3, 2), "S2FWD / S2BWD, ragged; PLAIN forward / PARITY bwd-data without scratch", (1, 1, 2, 0), (7, 6, 7, 0), (7, 6, 8, 3)),
    Case((3, 21, 19, 48, 64, 3, 2), "S2FWD / S2BWD, channel tail", (1, 1, 2, 0), (7, 6, 7, 0), (7, 6, 8, 3)),
    Case((2, 16, 16, 32, 64, 5, 1), "TAPSET_FWD / TAPSET_BWD1, 5x5", (1, 1, 1, 0), (3, 3, 1, 0), (3, 3, 1, 0)),
    Case((2, 13, 15, 64, 64, 5, 2), "TAPSET_FWD, four tap classes / PARITY on the tap-class kernel", (1, 1, 1, 0), (3, 3, 1, 0), (3, 3, 1, 0)),
    Case((2, 16, 16, 128, 128, 4, 2), "TAPSET_FWD / PARITY on the tap-class kernel, 4x4", (1, 1, 1, 0), (3, 3, 9, 0), (3, 3, 9, 0)),
    Case((4, 16, 16, 64, 256, 1, 1), "POINTWISE forward and bwd-data", (1, 1, 1, 0), (4, 4, 6, 0), (4, 4, 9, 0)),
    Case((1, 5, 5, 32, 20, 1, 1), "POINTWISE forward, PLAIN bwd-data (K = 20 < 32)", (1, 1, 1, 0), (4, 1, 6, 0), (4, 1, 9, 0)),
    Case((2, 20, 20, 128, 96, 3, 4), "GATHER forward, PARITY bwd-data (Cout % 64 != 0)", (1, 1, 2, 0), (4, 1, 7, 0), (4, 1, 9, 0)),
    Case((2, 16, 16, 64, 64, 1, 4), "GATHER forward, SCATTER bwd-data, 1x1 stride 4: 15 of 16 dX classes zero-filled", (1, 1, 1, 0), (4, 1, 7, 0), (4, 1, 9, 0)),
    Case((2, 17, 17, 192, 32, 3, 3), "GATHER forward, PARITY bwd-data (Cout % 64 != 0)", (1, 1, 2, 0), (4, 1, 7, 3), (4, 1, 8, 3)),
    Case((2, 18, 21, 96, 128, 3, 3), "PLAIN forward (Cin % 64 != 0), SCATTER bwd-data", (1, 1, 2, 0), (1, 1, 7, 3), (1, 1, 8, 3)),
    Case((2, 19, 22, 32, 48, 3, 4), "PARITY, stride > reach: the dX classes no tap reaches are zero-filled", (1, 1, 2, 0), (1, 1, 7, 0), (1, 1, 9, 0)),
    Case((3, 17, 13, 3, 64, 3, 1), "GENERIC, unaligned", (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)),
    Case((2, 23, 17, 3, 64, 7, 2), "GENERIC, unaligned, 7x7 stride 2", (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)),
    Case((2, 10, 10, 64, 64, 3, 1, 2), "PLAIN with scratch: dilation 2", (1, 1, 2, 0), (1, 1, 2, 0), (1, 1, 2, 0)),
    Case((1, 10, 10, 128, 64, 3, 1, 12), "PLAIN, dilation 12: only the centre tap is in range", (1, 1, 2, 0), (1, 1, 2, 0), (1, 1, 2, 0)),
    Case((1, 10, 10, 192, 192, 3, 1), "nine channel tiles; WINO_F23 in both split modes", (1, 1, 3, 0), (5, 5, 4, 0), (5, 5, 4, 0)),
    Case((5, 1, 1, 512, 51, 1, 1), "GENERIC: the FC layer as a 1x1 convolution", (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)),
    Case((3, 12, 11, 64, 96, 1, 1), "POINTWISE forward and bwd-data, ragged: M = 396 rows (a partial last 128-row tile), 132 rows per image "
         "(sample boundaries inside tiles), Cout = 96 (a partial 128-column tile)", (1, 1, 1, 0), (4, 4, 6, 0), (4, 4, 9, 0)),
    # bwd-weight only: the smallest problem the transform-domain kernel (route 5) takes in bf16x3
    Case((1, 64, 64, 768, 768, 3, 1), "bwd-weight route 5 (bf16x3)", (1, 1, 3, 0), (8, 8, 5, 0), (5, 5, 4, 0), wgrad_only=True),
]
FB_CASES = [c for c in CASES if not c.wgrad_only]
case_id = lambda c: c.id


# ================================================================================================
# host-side queries (no launch; these run on a machine without a GPU)
# ================================================================================================
def lib():
    return hip.load()


def ws_bytes(c, transposed):
    return int(lib().fs_conv2d_workspace_bytes(*c.args[1:], transposed))


def choice(c, transposed, nbytes):
    return int(lib().fs_conv2d_kernel_choice(*c.args, transposed, nbytes))


def persistent(c, transposed, nbytes):
    return int(lib().fs_conv2d_pack_persistent(*c.args, transposed, nbytes))


def wgrad_ws_bytes(c):
    return int(lib().fs_conv2d_bwd_weight_ws_bytes(c.Cin, c.Cout, c.k, c.k, c.stride, c.pad, c.dil))


def wgrad_plan(c, nbytes):
    out = (ctypes.c_int * 6)()
    ok = lib().fs_conv2d_bwd_weight_plan(*c.args, nbytes, out)
    return (int(ok),) + tuple(int(v) for v in out)


def scatter_eligible(c):
    """fs_pointwise_scatter_eligible (csrc/conv_pointwise.hip) and the residue-class mask width plan_conv asks for
    (`has(F_SCATTER) && c.stride * c.stride <= 32`).  A hand copy: keep it in step with that function and that line."""
    return (c.stride >= c.k and c.stride > 1 and c.dil == 1 and c.Cout % 64 == 0 and c.Cin % 4 == 0 and c.Cin >= 32 and c.k * c.k <= 9
            and c.stride * c.stride <= 32)


def route_of(c, mode, transposed, nbytes):
    """The launch path of plan_conv for this problem: the public id, and for the ids that several paths share the direction and
    shape facts plan_conv decides by.  Asserts that fs_conv2d_pack_persistent agrees with the path.  A hand copy of the
    first-match chain in plan_conv and of ROUTE_INFO (csrc/conv.hip): keep it in step with both.  SCATTER and PARITY both report
    id 1 and no persistent pack, so between those two this copy is the only witness."""
    fam = choice(c, transposed, nbytes)
    fwd = not transposed
    if fam in (0, 2, 5, 8, 7, 6):
        r = {0: "GENERIC", 2: "HALO", 5: "WINO_F23", 8: "WINO_F43", 7: "S2FWD", 6: "S2BWD"}[fam]
    elif fam == 4:      # POINTWISE: 1x1 / stride 1, either direction; GATHER: forward, stride >= filter
        r = "POINTWISE" if (c.k == 1 and c.stride == 1) else "GATHER"
        assert r == "POINTWISE" or (fwd and c.stride >= c.k and c.Cin % 64 == 0)
    elif fam == 3:      # the tap-class kernel: forward at any stride, bwd-data at stride 1, else the multi-tap classes of PARITY
        r = "TAPSET_FWD" if fwd else "TAPSET_BWD1" if c.stride == 1 else "PARITY"
    else:               # 1: PLAIN forward at any stride and bwd-data at stride 1; strided bwd-data: SCATTER where the family fits
        assert fam == 1
        split = mode != "f32" and nbytes > 0
        r = "PLAIN" if (fwd or c.stride == 1) else "SCATTER" if (split and scatter_eligible(c)) else "PARITY"
    assert persistent(c, transposed, nbytes) == (1 if r in PERSISTENT else 0), (c.id, mode, transposed, r)
    assert (fam == 0) == (not c.aligned or c.k * c.k > 32)
    return r


def assert_expected(c, mode):
    """what the table row records, against the queries; returns (forward path, bwd-data path) at the full scratch"""
    ef, eb, er, ea = c.expect[mode]
    nf, nb = ws_bytes(c, 0), ws_bytes(c, 1)
    assert (choice(c, 0, nf), choice(c, 1, nb)) == (ef, eb), (c.id, mode, choice(c, 0, nf), choice(c, 1, nb))
    assert choice(c, 0, 0) == (1 if c.aligned else 0) and choice(c, 1, 0) == (1 if c.aligned else 0), (c.id, mode)
    plan = wgrad_plan(c, wgrad_ws_bytes(c))
    assert plan[0] == 1 and plan[1:3] == (er, ea), (c.id, mode, plan)
    return route_of(c, mode, 0, nf), route_of(c, mode, 1, nb)


def test_case_table_reaches_every_path():
    """From the host-side queries alone (no launch): every row reaches the ids it records, and the table reaches, in each
    precision mode where the path exists, every public id 0-8 forward and every bwd-data id; every launch path of plan_conv --
    so both members of PLAIN with / without scratch, POINTWISE / GATHER, SCATTER / PARITY and the two tap-class forms;
    the PLAIN fallback (ws = NULL) of a 3x3 stride-1, a stride-2 forward and a 1x1 problem; all ten bwd-weight routes and the
    accumulation kinds 0, 2 and 3 (kind 1 is what accumulate = 1 turns kind 0 into)."""
    fwd_ids, bwd_ids, paths, wg = {}, {}, {}, set()
    for mode in MODES:
        with precision(mode):
            for c in CASES:
                pf, pb = assert_expected(c, mode)
                if c.wgrad_only:
                    continue
                fwd_ids.setdefault(mode, set()).add(c.expect[mode][0])
                bwd_ids.setdefault(mode, set()).add(c.expect[mode][1])
                seen = paths.setdefault(mode, set())
                seen.update([(pf, "fwd", True), (pb, "bwd", True)])      # True: the plan's choice at the scratch the query asks for
                if ws_bytes(c, 0) > 0:                                   # False: the fallback with ws = NULL where a family would run
                    seen.add((route_of(c, mode, 0, 0), "fwd", False))
                if ws_bytes(c, 1) > 0:
                    seen.add((route_of(c, mode, 1, 0), "bwd", False))
        for det in (False, True):
            with precision(mode, det):
                for c in CASES:
                    if c.wgrad_only and mode != "bf16x3":
                        continue
                    plan = wgrad_plan(c, wgrad_ws_bytes(c))
                    assert plan[0] == 1 and (plan[2] == 2 if det else plan[2] in (0, 3)), (c.id, mode, det, plan)
                    wg.add((plan[1], plan[2]))
    assert fwd_ids["f32"] == {0, 1} and bwd_ids["f32"] == {0, 1}
    assert fwd_ids["bf16x3"] == {0, 1, 2, 3, 4, 5, 7, 8} and bwd_ids["bf16x3"] == {0, 1, 2, 3, 4, 5, 6, 8}        # 6 is bwd-data only, 7 forward only
    assert fwd_ids["f16x2"] == {0, 1, 2, 3, 4, 5, 7} and bwd_ids["f16x2"] == {0, 1, 2, 3, 4, 5, 6}                # F(4,3) is bf16x3 only
    got = {m: {p for p, _, _ in s} for m, s in paths.items()}
    assert got["f32"] == {"GENERIC", "PLAIN", "PARITY"}
    assert got["bf16x3"] == set(ROUTES) and got["f16x2"] == set(ROUTES) - {"WINO_F43"}
    for mode in ("bf16x3", "f16x2"):
        s = paths[mode]
        assert ("PLAIN", "fwd", True) in s and ("PLAIN", "fwd", False) in s and ("PLAIN", "bwd", True) in s and ("PLAIN", "bwd", False) in s
        assert ("PARITY", "bwd", True) in s and ("PARITY", "bwd", False) in s and ("SCATTER", "bwd", True) in s
        assert ("POINTWISE", "fwd", True) in s and ("POINTWISE", "bwd", True) in s and ("GATHER", "fwd", True) in s
        assert ("TAPSET_FWD", "fwd", True) in s and ("TAPSET_BWD1", "bwd", True) in s
        with precision(mode):       # the fallback is run for 3x3 stride 1, stride-2 forward and 1x1 problems whose scratch route is another
            for want in ((3, 1, ("HALO", "WINO_F23", "WINO_F43")), (3, 2, ("S2FWD",)), (1, 1, ("POINTWISE",))):
                assert any(c.k == want[0] and c.stride == want[1] and route_of(c, mode, 0, ws_bytes(c, 0)) in want[2]
                           and route_of(c, mode, 0, 0) == "PLAIN" for c in FB_CASES), want
    assert {r for r, _ in wg} == set(range(10)), wg
    assert {a for _, a in wg} == {0, 2, 3}, wg
    # the fused epilogues of the 1x1 GEMM kernel are reached on a ragged case in both split modes: a partial last 128-row tile,
    # and for the residual form a sample boundary inside a tile (rows_per_sample no multiple of 128)
    for mode in ("bf16x3", "f16x2"):
        with precision(mode):
            ragged = [c for c in FB_CASES if (c.B * c.Ho * c.Wo) % 128 != 0]
            assert any(residual_expected(c, route_of(c, mode, 0, ws_bytes(c, 0)), rows) == 1 and rows % 128 != 0
                       and int(lib().fs_conv2d_fwd_residual_ok(*c.args, rows, ws_bytes(c, 0))) == 1
                       for c in ragged for rows in residual_rows(c)), mode
            assert any(route_of(c, mode, 1, ws_bytes(c, 1)) == "POINTWISE" and int(lib().fs_conv2d_bwd_data_bnsum_slabs(*c.args, ws_bytes(c, 1))) > 0
                       for c in ragged), mode


def test_conv_problem_record_is_the_abi_argument_block():
    """ops.ConvProblem, the one place the Python side spells the twelve integers of the conv ABI: built from tensor shapes it IS the
    argument block of the case (c.args is written out independently above), and in every precision mode, for both directions, each of
    its host queries answers what the direct library call with *c.args answers at the scratch fs_conv2d_workspace_bytes asks for."""
    P = fovealseg.ops.ConvProblem
    for mode in MODES:
        with precision(mode):
            for c in CASES:
                p = P.of((c.B, c.H, c.W, c.Cin), (c.Cout, c.Cin, c.k, c.k), c.stride, c.pad, c.dil)
                assert tuple(p) == c.args and len(c.args) == 12, (c.id, p)
                assert p.x_shape == (c.B, c.H, c.W, c.Cin) and p.y_shape == (c.B, c.Ho, c.Wo, c.Cout)
                assert p.flops == 2.0 * c.B * c.Ho * c.Wo * c.Cout * c.k * c.k * c.Cin
                assert tuple(p.at_batch(c.B + 3)) == (c.B + 3,) + c.args[1:]
                assert p.wgrad_ws_bytes() == wgrad_ws_bytes(c), (c.id, mode)
                for tr in (0, 1):
                    ws = ws_bytes(c, tr)
                    assert p.ws_bytes(tr) == ws, (c.id, mode, tr)
                    assert p.pack_persistent(tr, ws) == persistent(c, tr, ws), (c.id, mode, tr)
                    assert p.stats_slabs(ws) == int(lib().fs_conv2d_stats_slabs(*c.args, ws)), (c.id, mode, tr)
                    assert p.bnsum_slabs(ws) == int(lib().fs_conv2d_bwd_data_bnsum_slabs(*c.args, ws)), (c.id, mode, tr)
                    assert p.affine_act_ok(ws) == (int(lib().fs_conv2d_fwd_affine_act_ok(*c.args, ws)) == 1), (c.id, mode, tr)
                    for rows in residual_rows(c):
                        assert p.residual_ok(rows, ws) == (int(lib().fs_conv2d_fwd_residual_ok(*c.args, rows, ws)) == 1), (c.id, mode, tr, rows)
    assert tuple(P.linear(396, 64, 96)) == (1, 396, 1, 64, 396, 1, 96, 1, 1, 1, 0, 1)
    assert P.linear(396, 64, 96).flops == 2.0 * 396 * 96 * 64


# ================================================================================================
# data and references: made once per (case, kind), shared by the three modes, never modified
# ================================================================================================
def gen_for(c, salt):
    return torch.Generator().manual_seed(sum(c.args) * 131 + salt)


def lattice(gen, B, H, W, Ch, step):
    """one non-zero (a power of two, in one channel) per step x step block of pixels: any window of `step` pixels a side
    holds at most one"""
    t = torch.zeros(B, H, W, Ch, dtype=torch.float64)
    for b in range(B):
        for y in range(int(torch.randint(0, min(step, H), (1,), generator=gen)), H, step):
            for x in range(int(torch.randint(0, min(step, W), (1,), generator=gen)), W, step):
                t[b, y, x, int(torch.randint(0, Ch, (1,), generator=gen))] = float(pow2(gen, 1))
    return t


def one_tap_per(gen, k, Ci, Co, per_out):
    """w with a single non-zero tap (r, s, other channel) per output channel (forward: per Cout; bwd-data: per Cin)"""
    w = torch.zeros(k, k, Ci, Co, dtype=torch.float64)
    for n in range(Co if per_out else Ci):
        r, s = int(torch.randint(0, k, (1,), generator=gen)), int(torch.randint(0, k, (1,), generator=gen))
        o = int(torch.randint(0, Ci if per_out else Co, (1,), generator=gen))
        if per_out:
            w[r, s, o, n] = float(pow2(gen, 1))
        else:
            w[r, s, n, o] = float(pow2(gen, 1))
    return w


def one_pixel_per(gen, B, H, W, Ch):
    """a single non-zero pixel per channel"""
    t = torch.zeros(B, H, W, Ch, dtype=torch.float64)
    for ch in range(Ch):
        t[int(torch.randint(0, B, (1,), generator=gen)), int(torch.randint(0, H, (1,), generator=gen)),
          int(torch.randint(0, W, (1,), generator=gen)), ch] = float(pow2(gen, 1))
    return t


def rint(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def rnd(gen, *shape):
    return f32(torch.randn(*shape, generator=gen, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def fwd_data(ci, kind):
    """x, w, bias, drop_p, drop_key of a forward case, and its references: y, sum|terms| (bias included, times the drop scale),
    the contraction length"""
    c = CASES[ci]
    g = gen_for(c, {"int": 1, "float": 2, "widthA": 3, "widthB": 4, "sparse": 5}[kind])
    xs, ws_ = (c.B, c.H, c.W, c.Cin), (c.k, c.k, c.Cin, c.Cout)
    bias, p, key = None, 0.0, 0
    if kind == "sparse":
        # integers thinned out until the sum of y^2 over a channel's pixels stays below 2^24: E y^2 = 8 q^2 n per pixel with
        # density q of the non-zeros (x = +-1, w = +-2, drop scale 2 on half the elements), kept below 2^20 / M
        n, M = c.k * c.k * c.Cin, c.B * c.Ho * c.Wo
        q = min(1.0, (2.0 ** 20 / (8.0 * n * M)) ** 0.5)
        x = rint(g, 0, 1, *xs) * 2 - 1
        x = x * (torch.rand(*xs, generator=g) < q)
        w = (rint(g, 0, 1, *ws_) * 4 - 2) * (torch.rand(*ws_, generator=g) < q)
        bias, p, key = rint(g, -1, 1, c.Cout), 0.5, O.layer_key(9, ci + 1)
        y = C.conv2d_fwd(x, w, bias, c.stride, c.pad, c.dil, p, key)
        return dict(x=x, w=w, bias=bias, p=p, key=key, y=y, terms=None, count=None)
    if kind == "int":
        x, w, bias, p = rint(g, -3, 3, *xs), 2 * rint(g, -1, 1, *ws_), rint(g, -4, 4, c.Cout), 0.5      # drop scale 2: exact
        key = O.layer_key(7, ci + 1)
    elif kind == "float":
        x, w, bias = rnd(g, *xs), rnd(g, *ws_), rnd(g, c.Cout)
    elif kind == "widthA":
        x, w = wide(rnd(g, *xs)), one_tap_per(g, c.k, c.Cin, c.Cout, True)
    else:
        x, w = lattice(g, *xs, c.dil * (c.k - 1) + 1), wide(rnd(g, *ws_))
    y = C.conv2d_fwd(x, w, bias, c.stride, c.pad, c.dil, p, key)
    terms = (C.fwd_terms(x, w, c.stride, c.pad, c.dil) + (0 if bias is None else bias.abs())) * R.drop_scale(p)
    count = C.fwd_count(x, w, c.stride, c.pad, c.dil)
    return dict(x=x, w=w, bias=bias, p=p, key=key, y=y, terms=terms, count=count)


@functools.lru_cache(maxsize=None)
def bwd_data(ci, kind):
    c = CASES[ci]
    g = gen_for(c, {"int": 11, "float": 12, "widthA": 13, "widthB": 14}[kind])
    ys, ws_ = (c.B, c.Ho, c.Wo, c.Cout), (c.k, c.k, c.Cin, c.Cout)
    if kind == "int":
        dy, w = rint(g, -3, 3, *ys), 2 * rint(g, -1, 1, *ws_)
    elif kind == "float":
        dy, w = rnd(g, *ys), rnd(g, *ws_)
    elif kind == "widthA":
        dy, w = wide(rnd(g, *ys)), one_tap_per(g, c.k, c.Cin, c.Cout, False)
    else:
        dy, w = lattice(g, *ys, c.dil * (c.k - 1) + 1), wide(rnd(g, *ws_))
    a = (c.H, c.W, c.stride, c.pad, c.dil)
    return dict(dy=dy, w=w, dx=C.conv2d_bwd_data(dy, w, *a), terms=C.bwd_data_terms(dy, w, *a), count=C.bwd_data_count(dy, w, *a))


@functools.lru_cache(maxsize=None)
def wgrad_data(ci, kind):
    c = CASES[ci]
    g = gen_for(c, {"int": 21, "float": 22, "widthA": 23, "widthB": 24}[kind])
    xs, ys = (c.B, c.H, c.W, c.Cin), (c.B, c.Ho, c.Wo, c.Cout)
    if kind == "int":
        x, dy = rint(g, -2, 2, *xs), 2 * rint(g, -1, 1, *ys)        # dy even: (dU1 +- dU2) / 2 of route 5 stays integral
    elif kind == "float":
        x, dy = rnd(g, *xs), rnd(g, *ys)
    elif kind == "widthA":
        x, dy = wide(rnd(g, *xs)), one_pixel_per(g, *ys)
    else:
        x, dy = one_pixel_per(g, *xs), wide(rnd(g, *ys))
    a = (c.k, c.k, c.stride, c.pad, c.dil)
    count = None if c.wgrad_only else C.bwd_weight_count(x, dy, *a)      # route 5 takes its n from the shape
    return dict(x=x, dy=dy, dw=C.conv2d_bwd_weight(x, dy, *a), terms=None if c.wgrad_only else C.bwd_weight_terms(x, dy, *a), count=count)


def arith(mode, fam):
    """the arithmetic a path runs in: the generic kernel is fp32 in every mode"""
    return 0 if (mode == "f32" or fam == 0) else MODES.index(mode)


def wino_bound(a, m, Cs, wterms, amax, bmax, extra, kind="float"):
    """ids 5 / 8: n = 3 filter rows x Cs channels x (m + 2) components; the f16x2 floor takes the largest transformed operands,
    2 max|x| (T = d_a +- d_b) and 1.5 max|w| (U = (g0 +- g1 + g2) / 2), times the output transform's largest row sum 3.
    The width probes have far fewer NON-ZERO products (a zero product adds exactly and rounds nothing), which is what gives the
    probe its grip here: the one-hot filter of "widthA" has one channel and one filter row per output, so m + 2 products; the
    lattice image of "widthB" (one pixel per 3 x 3 block) puts at most two pixels of one row into a tile's m + 2 <= 6 inputs and
    one row into the filter's three, so 2 (m + 2) products.  A third bf16 plane lost is 2^-16 = 256 u of a product against
    (6 * 2 (m + 2) + 3 + WINO_ROUND + 2) u <= 91 u here."""
    n = {"widthA": m + 2, "widthB": 2 * (m + 2)}.get(kind, 3 * Cs * (m + 2))
    b = (P_STEPS[a] * n + S_SPLIT[a] + WINO_ROUND + extra) * U * wterms
    return b + (n * F16_FLOOR * 2 * amax * 1.5 * bmax * 3 if a == 2 else 0.0)


def width_bound(a, ref, amax, bmax):
    """one product per output.  f32 / bf16x3: exact (None).  f16x2: the wide operand's two-plane error 2^-22 |x| (the one-hot
    operand is a power of two: h1 exact, h2 = 0), the additions of h1 s and h2 s (2 u), and the floor of one product"""
    return None if a < 2 else ref.abs() * (F16_WIDTH + 2 * U) + F16_FLOOR * amax * bmax


def verify(fam_name, what, got, ref, bound):
    if bound is None:
        exact(fam_name, what, got, ref)
        report(fam_name, what, 0.0)
    else:
        check(fam_name, what, got, ref, bound)


def pack_scratch(nbytes):
    return Out(nbytes, torch.uint8) if nbytes > 0 else None


def run_fwd(c, d, nbytes, entry="fs_conv2d_fwd", stats=None):
    y = Out(c.B * c.Ho * c.Wo * c.Cout)
    ws = pack_scratch(nbytes)
    head = (dev(d["x"]), dev(d["w"]), dev(d["bias"]))
    ptrs = [hip.ptr(t) for t in head] + [y.ptr] + ([stats.ptr] if stats is not None else [])
    hip.call(entry, *ptrs, *c.args, d["p"], d["key"], ws.ptr if ws else None, nbytes, None)
    if ws is not None:
        ws.get(complete=False)
    return y.get()


def run_bwd(c, d, nbytes):
    dx = Out(c.B * c.H * c.W * c.Cin)
    ws = pack_scratch(nbytes)
    dy, w = dev(d["dy"]), dev(d["w"])
    hip.call("fs_conv2d_bwd_data", hip.ptr(dy), hip.ptr(w), dx.ptr, *c.args, ws.ptr if ws else None, nbytes, None)
    if ws is not None:
        ws.get(complete=False)
    return dx.get()


def scratch_settings(c, mode, transposed):
    """(bytes, path) of the runs of one direction: the scratch the query asks for, and ws = NULL in the split modes"""
    n = ws_bytes(c, transposed)
    runs = [(n, route_of(c, mode, transposed, n))]
    if n > 0:
        runs.append((0, route_of(c, mode, transposed, 0)))
    return runs


KINDS = ["int", "widthA", "widthB", "float"]


def wino_m(path):
    return {"WINO_F23": 2, "WINO_F43": 4}.get(path)


# ================================================================================================
# forward and bwd-data
# ================================================================================================
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ci", range(len(FB_CASES)), ids=[c.id for c in FB_CASES])
def test_conv2d_fwd(ci, mode):
    c = CASES[ci]
    with precision(mode):
        assert_expected(c, mode)
        for nbytes, path in scratch_settings(c, mode, 0):
            a, m = arith(mode, choice(c, 0, nbytes)), wino_m(path)
            tag = f"{c.id} {mode} {path}{'' if nbytes or mode == 'f32' else ' ws=NULL'}"
            for kind in KINDS:
                d = fwd_data(ci, kind)
                got = run_fwd(c, d, nbytes)
                amax, bmax = float(d["x"].abs().max()), float(d["w"].abs().max())
                if m is not None:      # the transform mixes neighbours: the derived bound for every kind -- but F(2,3) on integers is exact
                    if kind == "int" and m == 2:
                        bound = None
                    else:
                        wt = (C.wino_fwd_terms(d["x"], d["w"], m) + (0 if d["bias"] is None else d["bias"].abs())) * R.drop_scale(d["p"])
                        bound = wino_bound(a, m, c.Cin, wt, amax, bmax, 2, kind)
                elif kind == "int":
                    bound = None
                elif kind == "float":
                    bound = direct_bound(a, d["count"], d["terms"], amax, bmax, 2)
                else:
                    bound = width_bound(a, d["y"], amax, bmax)
                verify("conv_fwd", f"{tag} {kind}", got, d["y"], bound)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ci", range(len(FB_CASES)), ids=[c.id for c in FB_CASES])
def test_conv2d_bwd_data(ci, mode):
    """dX pixels no tap reaches (stride > reach, the zero-filled residue classes of SCATTER / PARITY) are zero in the reference
    and must be WRITTEN zeros: the output starts as NaN"""
    c = CASES[ci]
    with precision(mode):
        assert_expected(c, mode)
        for nbytes, path in scratch_settings(c, mode, 1):
            a, m = arith(mode, choice(c, 1, nbytes)), wino_m(path)
            tag = f"{c.id} {mode} {path}{'' if nbytes or mode == 'f32' else ' ws=NULL'}"
            for kind in KINDS:
                d = bwd_data(ci, kind)
                got = run_bwd(c, d, nbytes)
                amax, bmax = float(d["dy"].abs().max()), float(d["w"].abs().max())
                if m is not None:
                    if kind == "int" and m == 2:
                        bound = None
                    else:      # the bwd-data of a 3x3 / stride-1 / pad-1 layer is the forward of dy with the flipped, transposed filter
                        bound = wino_bound(a, m, c.Cout, C.wino_fwd_terms(d["dy"], C.flip_transpose(d["w"]), m), amax, bmax, 0, kind)
                elif kind == "int":
                    bound = None
                elif kind == "float":
                    bound = direct_bound(a, d["count"], d["terms"], amax, bmax, 0)
                else:
                    bound = width_bound(a, d["dx"], amax, bmax)
                verify("conv_bwd_data", f"{tag} {kind}", got, d["dx"], bound)


# ================================================================================================
# bwd-weight: default mode, deterministic mode with the slab scratch in an Out, accumulate = 1 onto a visible pattern
# ================================================================================================
def wgrad_arith(mode, route):
    """routes 0-3 are the fp32 kernels of conv.hip in every mode"""
    return 0 if (mode == "f32" or route <= 3) else MODES.index(mode)


def pattern(n):
    return ((torch.arange(n) % 7) - 3).double()


def run_wgrad(c, d, accumulate, det):
    """-> dW, the plan.  The scratch is what fs_conv2d_bwd_weight_ws_bytes asks for in this mode (none: ws = NULL), in an Out:
    the slab rows the plan says the launches write (out[5]) are written completely -- where the launches store them (kind 3) or
    a memset zeroes the cap first (kind 2) --, and the rows behind them still hold the fill (kind 3) or the memset's zeros."""
    n = c.k * c.k * c.Cin * c.Cout
    nbytes = wgrad_ws_bytes(c)
    plan = wgrad_plan(c, nbytes)
    ok, route, accum, launches, wgs, threads, slabs = plan
    assert ok == 1 and (accum == 2) == det and (slabs > 0) == (accum >= 2) and nbytes % (4 * n) == 0 and slabs <= nbytes // (4 * n)
    dw0 = pattern(n) if accumulate else None
    dw = Out(n, body=dw0)
    ws = Out(nbytes // 4) if nbytes else None
    x, dy = dev(d["x"]), dev(d["dy"])
    hip.call("fs_conv2d_bwd_weight", hip.ptr(x), hip.ptr(dy), dw.ptr, *c.args, accumulate, ws.ptr if ws else None, nbytes)
    if ws is not None:
        left = ws.rows_left(n)
        assert int(left[:slabs].sum()) == 0, f"{c.id}: {int((left[:slabs] > 0).sum())} of the plan's {slabs} slab rows hold unwritten elements"
        if accum == 3:
            assert bool((left[slabs:] == n).all()), f"{c.id}: slab rows behind the plan's {slabs} were written"
        else:
            assert int(left[slabs:].sum()) == 0 and not bool(ws.t.reshape(-1, n)[slabs:].any()), f"{c.id}: rows behind the plan's {slabs} are not the memset's zeros"
    return dw.get(complete=not accumulate), plan, dw0


WGRAD_RUNS = [(ci, mode) for ci, c in enumerate(CASES) for mode in MODES if not c.wgrad_only or mode == "bf16x3"]


@gpu
@pytest.mark.parametrize("ci,mode", WGRAD_RUNS, ids=[f"{CASES[ci].id}-{mode}" for ci, mode in WGRAD_RUNS])
def test_conv2d_bwd_weight(ci, mode):
    c = CASES[ci]
    settings = [(0, False), (1, False), (0, True), (1, True)]
    for accumulate, det in settings:
        with precision(mode, det):
            if not det:
                assert_expected(c, mode)
            route = wgrad_plan(c, wgrad_ws_bytes(c))[1]
            a = wgrad_arith(mode, route)
            # the width probe and the integers in every setting are cheap on the small cases; the large route-5 case runs int + float
            kinds = KINDS if not c.wgrad_only else ["int", "float"]
            for kind in kinds if not accumulate else ["int", "float"]:
                d = wgrad_data(ci, kind)
                got, plan, dw0 = run_wgrad(c, d, accumulate, det)
                wgs = plan[4]
                ref = d["dw"].reshape(-1) + (dw0 if dw0 is not None else 0)
                amax, bmax = float(d["x"].abs().max()), float(d["dy"].abs().max())
                tag = f"{c.id} {mode} route {route} accum {plan[2]}{' accumulate' if accumulate else ''}{' det' if det else ''} {kind}"
                if kind == "int":
                    bound = None
                elif route == 5:      # transform domain: n = pixel pairs x 4 components
                    terms = C.wino_wgrad_terms(d["x"], d["dy"]).reshape(-1)
                    bound = (P_STEPS[a] * (c.B * c.H * c.W // 2) * 4 + S_SPLIT[a] + WINO_ROUND + wgs + 1) * U * terms
                elif kind == "float":
                    terms = d["terms"].reshape(-1)
                    bound = direct_bound(a, d["count"].reshape(-1), terms, amax, bmax, wgs + 1)
                else:
                    bound = width_bound(a, ref, amax, bmax)
                if accumulate and kind == "float":      # the rounding of the sum onto the pattern
                    bound = bound + U * (terms + dw0.abs())
                verify("conv_bwd_weight", tag, got, ref, bound)


def test_bwd_weight_scratch_cases_cover_slab_rows_and_pixel_splits():
    """host only: among the bwd-weight runs above with their scratch in an Out there is, for each of the nine routes that can
    take one, a case; at least one writes two or more slab rows, and at least one has more workgroups than channel-tile x tap
    units (several pixel splits)"""
    routes, multi_rows, multi_split = set(), 0, 0
    for mode in MODES:
        for det in (False, True):
            with precision(mode, det):
                for c in CASES:
                    if c.wgrad_only and mode != "bf16x3":
                        continue
                    nbytes = wgrad_ws_bytes(c)
                    ok, route, accum, launches, wgs, threads, slabs = wgrad_plan(c, nbytes)
                    if nbytes == 0:
                        continue
                    routes.add(route)
                    multi_rows += slabs >= 2
                    multi_split += wgs > -(-c.Cin // 64) * -(-c.Cout // 64) * c.k * c.k
    assert routes == set(range(10)), routes
    assert multi_rows >= 1 and multi_split >= 1


# ================================================================================================
# fused entry points
# ================================================================================================
def rejected(name, *args):
    with pytest.raises(HipError, match="rejected"):
        hip.call(name, *args)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ci", range(len(FB_CASES)), ids=[c.id for c in FB_CASES])
def test_conv2d_fwd_stats(ci, mode):
    """fs_conv2d_fwd_stats on every path: y as fs_conv2d_fwd, and the [slabs][Cout][2] partial sums, added in fp64 on the host,
    against the per-channel sum and sum of squares of the reference output.  "sparse" integers (fwd_data): bit-equal, every total
    below 2^24 (asserted on the reference); float, over the M pixels of a channel: |sum - ref| <= sum of the elements' bounds + (M + slabs) u sum|y|,
    |sumsq - ref| <= sum of 2 |y| bound + (M + slabs + 1) u sum y^2 (one more rounding for the square).  The generic kernel
    has no such epilogue: the call is refused and nothing is written."""
    c = CASES[ci]
    with precision(mode):
        for nbytes, path in scratch_settings(c, mode, 0):
            slabs = int(lib().fs_conv2d_stats_slabs(*c.args, nbytes))
            stats = Out(slabs * c.Cout * 2)
            if path == "GENERIC":
                d = fwd_data(ci, "int")
                y = Out(c.B * c.Ho * c.Wo * c.Cout)
                x, w = dev(d["x"]), dev(d["w"])
                rejected("fs_conv2d_fwd_stats", hip.ptr(x), hip.ptr(w), None, y.ptr, stats.ptr, *c.args, 0.0, 0, None, 0, None)
                assert y.untouched() and stats.untouched()
                continue
            a, m = arith(mode, choice(c, 0, nbytes)), wino_m(path)
            M = c.B * c.Ho * c.Wo
            for kind in ("sparse", "float"):
                d = fwd_data(ci, kind)
                stats = Out(slabs * c.Cout * 2)
                got = run_fwd(c, d, nbytes, "fs_conv2d_fwd_stats", stats)
                tot = stats.get().double().reshape(slabs, c.Cout, 2).sum(0)
                ref_tot = C.stats_totals(d["y"])
                amax, bmax = float(d["x"].abs().max()), float(d["w"].abs().max())
                tag = f"{c.id} {mode} {path}{'' if nbytes or mode == 'f32' else ' ws=NULL'} {kind}"
                if m is not None and not (kind == "sparse" and m == 2):
                    wt = (C.wino_fwd_terms(d["x"], d["w"], m) + d["bias"].abs()) * R.drop_scale(d["p"])
                    eb = wino_bound(a, m, c.Cin, wt, amax, bmax, 2)
                elif kind == "sparse":
                    eb = None
                else:
                    eb = direct_bound(a, d["count"], d["terms"], amax, bmax, 2)
                verify("conv_fwd_stats", f"{tag} y", got, d["y"], eb)
                if eb is None:
                    assert float((d["y"] ** 2).sum((0, 1, 2)).max()) < 2 ** 24
                    exact("conv_fwd_stats", f"{tag} totals", tot, ref_tot)
                else:
                    ya = d["y"].abs().reshape(M, c.Cout)
                    ebm = torch.as_tensor(eb).expand(d["y"].shape).reshape(M, c.Cout)
                    b1 = ebm.sum(0) + (M + slabs) * U * ya.sum(0)
                    b2 = (2 * ya * ebm + ebm * ebm).sum(0) + (M + slabs + 1) * U * (ya * ya).sum(0)
                    check("conv_fwd_stats", f"{tag} totals", tot, ref_tot, torch.stack([b1, b2], dim=1))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ci", range(len(FB_CASES)), ids=[c.id for c in FB_CASES])
def test_conv2d_fwd_affine_act(ci, mode):
    """z = act((conv + bias) * scale + shift [+ res]).  act is 1-Lipschitz, so |z - act(v_ref)| <= the bound of the activation's
    argument v, whichever branch the device took: (L + 3) u of sum|terms| * |scale| + |shift| + |res| (three more roundings).
    int: scale a power of two, shift and res integers: bit-equal.  Where fs_conv2d_fwd_affine_act_ok says 0 the call is
    refused and z is untouched."""
    c = CASES[ci]
    with precision(mode):
        for nbytes, path in scratch_settings(c, mode, 0):
            ok = int(lib().fs_conv2d_fwd_affine_act_ok(*c.args, nbytes))
            assert ok == (1 if wino_m(path) else 0), (c.id, mode, path)
            if not ok:
                if nbytes == 0 and mode != "f32" and ci % 4:
                    continue          # the refusal is checked at the full scratch of every case and without scratch on every fourth
                d = fwd_data(ci, "int")
                ones = dev(torch.ones(c.Cout, dtype=torch.float64))
                x, w, bias = dev(d["x"]), dev(d["w"]), dev(d["bias"])
                z, ws = Out(d["y"].numel()), pack_scratch(nbytes)
                rejected("fs_conv2d_fwd_affine_act", hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(ones), hip.ptr(ones), None, z.ptr, *c.args, 1,
                         ws.ptr if ws else None, nbytes, None)
                assert z.untouched() and (ws is None or ws.untouched())
                continue
            g = gen_for(c, 31)
            m, a = wino_m(path), arith(mode, choice(c, 0, nbytes))
            for kind in ("int", "float"):
                d = fwd_data(ci, kind)
                if kind == "int":
                    scale, shift, res = pow2(g, c.Cout).abs(), rint(g, -3, 3, c.Cout), rint(g, -5, 5, *d["y"].shape)
                else:
                    scale, shift, res = rnd(g, c.Cout), rnd(g, c.Cout), rnd(g, *d["y"].shape)
                x, w, bias, sc, sh, rs = (dev(t) for t in (d["x"], d["w"], d["bias"], scale, shift, res))
                conv = C.conv2d_fwd(d["x"], d["w"], d["bias"], c.stride, c.pad, c.dil)
                wt0 = None if (kind == "int" and m == 2) else C.wino_fwd_terms(d["x"], d["w"], m) + d["bias"].abs()
                for act in (0, 1, 2):
                    for with_res in (False, True):
                        z, ws = Out(d["y"].numel()), pack_scratch(nbytes)
                        hip.call("fs_conv2d_fwd_affine_act", hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(sc), hip.ptr(sh),
                                 hip.ptr(rs) if with_res else None, z.ptr, *c.args, act, ws.ptr, nbytes, None)
                        ws.get(complete=False)
                        v = conv * scale + shift
                        ref = E.act_fwd(v + res if with_res else v, act)
                        tag = f"{c.id} {mode} {path} {kind} act {act}{' res' if with_res else ''}"
                        if wt0 is None:
                            verify("conv_fwd_affine_act", tag, z.get(), ref, None)
                        else:
                            wt = wt0 * scale.abs() + shift.abs() + (res.abs() if with_res else 0)
                            verify("conv_fwd_affine_act", tag, z.get(), ref,
                                   wino_bound(a, m, c.Cin, wt, float(d["x"].abs().max()), float(d["w"].abs().max()), 5))


def key_with_both(nsamp, p, seed):
    """a layer key under which `nsamp` samples hold kept AND dropped ones (chosen from the hash oracle on the CPU)"""
    for lid in range(1, 200):
        key = O.layer_key(seed, lid)
        m = R.keep_mask(nsamp, key, p)
        if p == 0 or nsamp < 2 or (bool(m.any()) and not bool(m.all())):
            return key
    raise AssertionError("no key found")


def residual_rows(c):
    """rows_per_sample values of a case: one image per sample; and, where they divide the M = B Ho Wo rows, half an image and an
    image and a half -- samples smaller than an image and sample boundaries that fall inside the kernel's 128-row tiles"""
    hw, M = c.Ho * c.Wo, c.B * c.Ho * c.Wo
    return [hw] + [r for r in ((hw // 2) if hw % 2 == 0 else 0, (3 * hw // 2) if hw % 2 == 0 else 0) if r > 0 and M % r == 0 and r != hw]


def residual_expected(c, path, rows):
    """fs_conv2d_fwd_residual_ok as include/fovealseg.h states it: the 1x1 GEMM kernel runs the layer, samples of at least one
    128-row tile"""
    return 1 if (path == "POINTWISE" and rows >= 128 and (c.B * c.Ho * c.Wo) % rows == 0) else 0


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ci", range(len(FB_CASES)), ids=[c.id for c in FB_CASES])
def test_conv2d_fwd_residual(ci, mode):
    """y = res + DropPath_b(Dropout(conv + bias)) for every rows_per_sample of residual_rows.  int: both rates 1/2 (scales 2:
    exact), bit-equal; float: rates 0.25 / 0.2, (L + 3) u of sum|terms| * both scales + |res|.  Keys under which kept and dropped
    samples (and elements) both occur.  Where fs_conv2d_fwd_residual_ok says 0 -- another path, samples below 128 rows, and
    ws = NULL in the split modes -- the call is refused and y and the scratch are untouched."""
    c = CASES[ci]
    M = c.B * c.Ho * c.Wo
    with precision(mode):
        for nbytes, path in scratch_settings(c, mode, 0):
            for rows in residual_rows(c):
                ok = int(lib().fs_conv2d_fwd_residual_ok(*c.args, rows, nbytes))
                assert ok == residual_expected(c, path, rows), (c.id, mode, path, rows)
                g = gen_for(c, 41 + rows)
                for kind in ("int", "float"):
                    d = fwd_data(ci, kind)
                    res = rint(g, -5, 5, *d["y"].shape) if kind == "int" else rnd(g, *d["y"].shape)
                    p, dp = (0.5, 0.5) if kind == "int" else (0.25, 0.2)
                    key, dkey = key_with_both(d["y"].numel(), p, 5), key_with_both(M // rows, dp, 6)
                    x, w, bias, rs = (dev(t) for t in (d["x"], d["w"], d["bias"], res))
                    ws, y = pack_scratch(nbytes), Out(d["y"].numel())
                    args = (hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(rs), y.ptr, *c.args, p, key, dp, dkey, rows, ws.ptr if ws else None, nbytes, None)
                    if not ok:
                        rejected("fs_conv2d_fwd_residual", *args)
                        assert y.untouched() and (ws is None or ws.untouched())
                        break
                    hip.call("fs_conv2d_fwd_residual", *args)
                    ws.get(complete=False)
                    ref = C.conv2d_fwd_residual(d["x"], d["w"], d["bias"], res, c.stride, c.pad, c.dil, p, key, dp, dkey, rows)
                    keep = R.droppath_factor(ref.numel(), rows * c.Cout, dp, dkey)
                    assert M // rows < 2 or (bool(keep.any()) and not bool(keep.all()))
                    tag = f"{c.id} {mode} {path} rows {rows} {kind}"
                    if kind == "int":
                        verify("conv_fwd_residual", tag, y.get(), ref, None)
                    else:
                        t0 = C.fwd_terms(d["x"], d["w"], c.stride, c.pad, c.dil) + d["bias"].abs()
                        terms = t0 * R.drop_scale(p) * R.drop_scale(dp) + res.abs()
                        verify("conv_fwd_residual", tag, y.get(), ref, direct_bound(arith(mode, 4), d["count"], terms, float(d["x"].abs().max()),
                                                                                    float(d["w"].abs().max()) * R.drop_scale(p) * R.drop_scale(dp), 5))


BNSUM_VARIANTS = [("y+mask", True, True, False, False), ("y+add+addmask", True, False, True, True), ("y+mask+add", True, True, True, False),
                  ("add only", False, False, True, True)]


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ci", range(len(FB_CASES)), ids=[c.id for c in FB_CASES])
def test_conv2d_bwd_data_bnsum(ci, mode):
    """dx = bwd-data [+ add_src under add_mask] and the BatchNorm-backward sums S = sum g, SX = sum g xhat of g = dx under
    bn_mask (the slab's rows added in fp64 on the host), with and without bn_mask, add_src / add_mask, and with bn_y = NULL.
    int: mean integer, invstd a power of two: bit-equal.  float: dx to (L + 1) u (sum|terms| + |add|); over the M pixels of a
    channel |S - ref| <= sum of dx's bounds + (M + slabs) u sum|g|, |SX - ref| <= sum of bound |xhat| + (M + slabs + 3) u
    sum|g xhat| (xhat = (y - mean) * invstd and the product: three more roundings).  Where
    fs_conv2d_bwd_data_bnsum_slabs says 0 -- another path, and ws = NULL in the split modes -- the call is refused and dx, the slab
    and the scratch are untouched."""
    c = CASES[ci]
    with precision(mode):
        for nbytes, path in scratch_settings(c, mode, 1):
            bnsum_one(ci, c, mode, nbytes, path)


def bnsum_one(ci, c, mode, nbytes, path):
    slabs = int(lib().fs_conv2d_bwd_data_bnsum_slabs(*c.args, nbytes))
    assert (slabs > 0) == (path in ("WINO_F23", "WINO_F43", "POINTWISE", "S2BWD")), (c.id, mode, path, slabs)
    g = gen_for(c, 51)
    M, Ci = c.B * c.H * c.W, c.Cin
    shape = (c.B, c.H, c.W, Ci)
    for kind in ("int", "float"):
        d = bwd_data(ci, kind)
        if kind == "int":
            bn_y, mean, invstd, add = rint(g, -3, 3, *shape), rint(g, -2, 2, Ci), pow2(g, Ci).abs(), rint(g, -4, 4, *shape)
        else:
            bn_y, mean, invstd, add = rnd(g, *shape), rnd(g, Ci), rnd(g, Ci).abs() + 0.5, rnd(g, *shape)
        bits, abits = torch.rand(*shape, generator=g) < 0.6, torch.rand(*shape, generator=g) < 0.6
        dy, w, by, bm, bi, ad = (dev(t) for t in (d["dy"], d["w"], bn_y, mean, invstd, add))
        mk = amk = None
        if slabs > 0:
            mk, amk = dev(E.pack_mask(bits.reshape(M, Ci)), torch.uint8), dev(E.pack_mask(abits.reshape(M, Ci)), torch.uint8)
        for name, with_y, with_mask, with_add, with_amask in BNSUM_VARIANTS:
            dx, slab, ws = Out(M * Ci), Out(max(slabs, 1) * Ci * 2), pack_scratch(nbytes)
            args = (hip.ptr(dy), hip.ptr(w), dx.ptr, *c.args, ws.ptr if ws else None, nbytes, None,
                    hip.ptr(by) if with_y else None, hip.ptr(mk) if (with_mask and slabs) else None, hip.ptr(bm), hip.ptr(bi),
                    slab.ptr if (with_y or slabs == 0) else None,
                    hip.ptr(ad) if with_add else None, hip.ptr(amk) if (with_amask and slabs) else None)
            if slabs == 0:
                rejected("fs_conv2d_bwd_data_bnsum", *args)
                assert dx.untouched() and slab.untouched() and (ws is None or ws.untouched())
                return
            hip.call("fs_conv2d_bwd_data_bnsum", *args)
            ws.get(complete=False)
            rdx, S, SX = C.conv2d_bwd_data_bnsum(d["dy"], d["w"], c.H, c.W, c.stride, c.pad, c.dil, bn_y if with_y else None,
                                                 bits if with_mask else None, mean, invstd, add if with_add else None,
                                                 abits if with_amask else None)
            tag = f"{c.id} {mode} {path} {kind} {name}"
            m, a = wino_m(path), arith(mode, choice(c, 1, nbytes))
            amax, bmax = float(d["dy"].abs().max()), float(d["w"].abs().max())
            addabs = add.abs() if with_add else 0
            if kind == "int" and m != 4:
                eb = None
            elif m is not None:
                eb = wino_bound(a, m, c.Cout, C.wino_fwd_terms(d["dy"], C.flip_transpose(d["w"]), m) + addabs, amax, bmax, 1)
            else:
                eb = direct_bound(a, d["count"], d["terms"] + addabs, amax, bmax, 1)
            verify("conv_bwd_data_bnsum", f"{tag} dx", dx.get(), rdx, eb)
            if not with_y:
                assert slab.untouched()
                continue
            tot = slab.get().double().reshape(slabs, Ci, 2).sum(0)
            ref_tot = torch.stack([S, SX], dim=1)
            if eb is None:
                assert float((rdx.abs() * ((bn_y - mean) * invstd).abs()).sum((0, 1, 2)).max()) * 4 < 2 ** 24      # quarters: invstd >= 1/4
                exact("conv_bwd_data_bnsum", f"{tag} sums", tot, ref_tot)
                continue
            live = (bits if with_mask else torch.ones_like(bits)).double().reshape(M, Ci)
            ga = rdx.abs().reshape(M, Ci) * live
            xh = ((bn_y - mean) * invstd).abs().reshape(M, Ci)
            ebm = torch.as_tensor(eb).expand(shape).reshape(M, Ci) * live
            b1 = ebm.sum(0) + (M + slabs) * U * ga.sum(0)
            b2 = (ebm * xh).sum(0) + (M + slabs + 3) * U * (ga * xh).sum(0)
            check("conv_bwd_data_bnsum", f"{tag} sums", tot, ref_tot, torch.stack([b1, b2], dim=1))
