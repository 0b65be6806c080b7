"""torch.autograd bindings of the HIP kernels (one Function per kernel group).

Activations travel as contiguous NHWC fp32 tensors (B,H,W,C).  Convolution weights keep the
reference's logical (Cout,Cin,R,S) shape with RSCK strides, so `w.permute(2,3,1,0)` is the contiguous
[R][S][Cin][Cout] array the kernels read (DESIGN.md "Data layout").
"""
import ctypes
import math
import operator
import os
import weakref
import zlib
from typing import NamedTuple

import torch
from torch.autograd import Function

from . import hip

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
BN_EPS = 1e-5


# ----------------------------------------------------------------------------------------------
# dropout keys (integer hash shared with csrc/common.h and the oracle replay)
# ----------------------------------------------------------------------------------------------
class DropoutState:
    """Global (seed, step) pair; every conv layer derives its key from it and its own id."""
    seed = 0
    step = 0

    @classmethod
    def key(cls, layer_id: int) -> int:
        return layer_key(cls.seed * 1000003 + cls.step, layer_id)


def layer_key(seed: int, layer_id: int) -> int:
    x = (seed * 0x9E3779B1 + layer_id * 0x85EBCA6B + 0x27D4EB2F) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    x = (x * 0x297A2D39) & 0xFFFFFFFF
    x ^= x >> 15
    return x


def layer_id_from_name(name: str) -> int:
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


# ----------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------
def rsck(w: torch.Tensor) -> torch.Tensor:
    """Contiguous [R][S][Cin][Cout] view of a logical (Cout,Cin,R,S) weight."""
    v = w.permute(2, 3, 1, 0)
    if not v.is_contiguous():
        raise hip.HipLibraryError(f"conv weight {tuple(w.shape)} is not stored RSCK (strides {w.stride()})")
    return v


def new_rsck_weight(cout, cin, r, s, device=None) -> torch.Tensor:
    """Uninitialised logical (Cout,Cin,R,S) tensor with RSCK storage."""
    return torch.empty(r, s, cin, cout, device=device, dtype=torch.float32).permute(3, 2, 0, 1)


def _out_hw(h, w, r, s, stride, pad, dil=1):
    return (h + 2 * pad - dil * (r - 1) - 1) // stride + 1, (w + 2 * pad - dil * (s - 1) - 1) // stride + 1


class KernelTimer:
    """Optional HIP-event timing of individual launches on the current stream (bench.py only).
    `flops` is the algorithmic work of the launch: 2 * B*Ho*Wo * Cout * R*S*Cin for every conv variant, bytes for the
    HBM-bound kinds (bn_fwd, bn_bwd)."""

    def __init__(self):
        self.records = {}          # kind -> list of (start_event, stop_event, flops)
        self.tags = {}             # kind -> list of (entry point, leading integer arguments) per record

    def launch(self, kind, flops, fn, tag=None):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        self.records.setdefault(kind, []).append((s, e, flops))
        self.tags.setdefault(kind, []).append(tag)

    def by_shape(self):
        """{(entry point, int args...): [launches, total_ms, flops]} over all recorded launches."""
        out = {}
        for kind, recs in self.records.items():
            for (s, e, f), tag in zip(recs, self.tags[kind]):
                d = out.setdefault(tag, [0, 0.0, 0.0])
                d[0] += 1; d[1] += s.elapsed_time(e); d[2] += f
        return out

    def summary(self):
        out = {}
        for kind, recs in self.records.items():
            ms = sum(s.elapsed_time(e) for s, e, _ in recs)
            fl = sum(f for _, _, f in recs)
            out[kind] = dict(launches=len(recs), total_ms=ms, flops=fl)
        return out


WGRAD_FIRST = os.environ.get("FS_WGRAD_FIRST", "1") != "0"      # kernel experiments: order of the two conv backward launches
TIMER = None      # set to a KernelTimer by bench.py around the timed region
# Parity-test instrument: when a list, every activation site appends (BatchNorm module | (HighResolutionModule, i), act kind,
# activated output), so a test can replay the branch each activation took in the CPU oracle (oracle ACT_REPLAY).
ACT_TRACE = None
# Flight recorder of the front-end backward (tests / probes): when a dict, DeformSegmentationModule.forward hooks the cotangents that
# reach x_sampled, the sampling grid and xs -- the grid path's and the edge loss's contributions to xs separately, and their sum -- and
# every hook leaves {name: (fp64 norm, int64 sum of the bit patterns)} there as DEVICE scalars (no host read inside backward).  Every
# kernel on that chain is order-fixed, so two passes over the same inputs must agree bit for bit, whichever way the weight gradients
# travel (arena-direct + side stream, or AccumulateGrad under torch DDP): a mismatch names the stage (tests/test_ddp_gloo.py).
GRAD_TRACE = None


def grad_probe(t, name, alias=False):
    """Record the gradient arriving at `t` under `name` in GRAD_TRACE; alias=True returns a view of t so that ONE consumer's
    contribution is seen on its own."""
    if GRAD_TRACE is None or not t.requires_grad:
        return t
    trace = GRAD_TRACE
    if alias:
        t = t.view_as(t)

    def hook(g):
        gd = g.detach()
        trace[name] = (gd.double().norm(), gd.contiguous().view(torch.int32).to(torch.int64).sum())
    t.register_hook(hook)
    return t


def _launch(kind, flops, name, *args):
    if TIMER is None:
        hip.call(name, *args)
    else:
        TIMER.launch(kind, flops, lambda: hip.call(name, *args), tag=(name,) + tuple(a for a in args if type(a) is int and a < (1 << 20)))


class ConvProblem(NamedTuple):
    """One convolution as the C ABI spells it (csrc/conv_kernels.h FsConvProblem): x (B,H,W,Cin) -> y (B,Ho,Wo,Cout) under an R x S filter.
    The field order IS the argument block of every conv entry point and host query, so `*p` passes it and nothing else in this module
    spells that order out.  The queries go through hip.query: cached per argument tuple, dropped when a library mode changes."""
    B: int
    H: int
    W: int
    Cin: int
    Ho: int
    Wo: int
    Cout: int
    R: int
    S: int
    stride: int
    pad: int
    dil: int

    @classmethod
    def of(cls, x_shape, w_shape, stride, pad, dil=1):
        """The problem of a (B,H,W,Cin) input under a logical (Cout,Cin,R,S) weight."""
        B, H, W, Cin = x_shape
        Cout, Cin2, R, S = w_shape
        assert Cin == Cin2, (tuple(x_shape), tuple(w_shape))
        Ho, Wo = _out_hw(H, W, R, S, stride, pad, dil)
        return cls(B, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil)

    @classmethod
    def linear(cls, rows, cin, cout):
        """A linear layer over `rows` rows of `cin` features as the 1x1 convolution of an image one pixel wide and `rows` high."""
        return cls(1, rows, 1, cin, rows, 1, cout, 1, 1, 1, 0, 1)

    @property
    def flops(self):
        """Algorithmic work of any of the three convolutions of this problem (exact: every factor is an integer, the product < 2^53)."""
        B, _, _, Cin, Ho, Wo, Cout, R, S, _, _, _ = self
        return 2.0 * B * Ho * Wo * Cout * R * S * Cin

    @property
    def x_shape(self):
        """Shape of the input and of its gradient, as a plain tuple (compares equal to tuple(t.shape))."""
        return self[0:4]

    @property
    def y_shape(self):
        return (self.B, self.Ho, self.Wo, self.Cout)

    def at_batch(self, B):
        """The same problem over B images (one batch range of it)."""
        return self._replace(B=B)

    def batch_ranges(self):
        """_batch_ranges over this problem's input and output tensors."""
        return _batch_ranges(self.B, self.H * self.W * self.Cin, self.Ho * self.Wo * self.Cout)

    def kind(self, transposed):
        """Timer bucket = the kernel csrc/conv.hip selects: the halo-tiled 3x3 stride-1 kernel, the other aligned kernels, or the generic one
        (transposed = bwd-data: the kernel's source channels are Cout)."""
        if self.Cin % 4 or self.Cout % 4:
            return "conv_generic"
        if self[7:] == (3, 3, 1, 1, 1) and (self.Cout if transposed else self.Cin) >= 32 and hip.get_conv_precision() != "f32":
            return "conv3x3"
        return "conv_affine"

    def ws_bytes(self, transposed):
        """Scratch bytes the conv entry points can use for this shape under the current precision mode."""
        return hip.query("fs_conv2d_workspace_bytes", *self[1:], transposed)

    def pack_persistent(self, transposed, ws):
        """Non-zero where the kernel this problem runs on can keep its weight pack across calls (fs_conv2d_pack / fs_conv2d_ws_mode)."""
        return hip.query("fs_conv2d_pack_persistent", *self, transposed, ws)

    def stats_slabs(self, ws):
        """Slab rows fs_conv2d_fwd_stats writes."""
        return hip.query("fs_conv2d_stats_slabs", *self, ws)

    def bnsum_slabs(self, ws):
        """Slab rows of fs_conv2d_bwd_data_bnsum, 0 = this problem's kernel has no such epilogue."""
        return hip.query("fs_conv2d_bwd_data_bnsum_slabs", *self, ws)

    def affine_act_ok(self, ws):
        """True where fs_conv2d_fwd_affine_act serves this problem."""
        return hip.query("fs_conv2d_fwd_affine_act_ok", *self, ws) == 1

    def residual_ok(self, rows_per_sample, ws):
        """True where fs_conv2d_fwd_residual serves this problem."""
        return hip.query("fs_conv2d_fwd_residual_ok", *self, rows_per_sample, ws) == 1

    def wgrad_ws_bytes(self):
        """Scratch bytes of fs_conv2d_bwd_weight: per-split partial tiles (deterministic mode; strided 3x3 layers in every mode)."""
        return hip.query("fs_conv2d_bwd_weight_ws_bytes", self.Cin, self.Cout, *self[7:])


def weight_amax(w):
    """Device word holding max|w| bits of parameter w if its optimiser keeps one and w has not been modified since
    (train.FlatParams.refresh_amax), else None: the library then reduces over the weights itself."""
    rec = getattr(w, "_fs_amax", None)
    if rec is not None and rec[1] == w._version:
        return rec[0]
    if torch.is_grad_enabled() or not w.is_cuda or w.dim() != 4 or hip.get_conv_precision() != "f16x2":
        return None
    # inference without an optimiser arena: reduce once per weight version instead of once per call (272 memset + reduction
    # launches per HRNet forward otherwise)
    word = torch.empty(1, dtype=torch.int32, device=w.device)
    offs = torch.zeros(1, dtype=torch.int64, device=w.device)
    sizes = torch.full((1,), w.numel(), dtype=torch.int64, device=w.device)
    hip.call("fs_weight_amax_segments", hip.ptr(rsck(w)), hip.ptr(offs), hip.ptr(sizes), 1, hip.ptr(word))
    w._fs_amax = (word, w._version)
    return word


# The conv kernels address a tensor with 32-bit byte offsets: an activation or gradient tensor of 4 GB or more (configs[3] at B = 64: the C1
# head's 1024-channel input at 160 x 160 is 6.7 GB) is processed in batch ranges that fit -- the images of a batch are independent in all
# three convolutions, BatchNorm partial-sum slabs simply concatenate, weight gradients accumulate.  Only the fused extras of the bwd-data
# epilogue (BatchNorm sums, residual addend) are given up on that path.  Dropout masks hash the element index of the FULL tensor, which
# the library cannot reproduce from a sub-range: such calls are not split (and fail loudly in the library, as before).
MAX_TENSOR_BYTES = 4294967000


def _batch_ranges(B, *per_image_elems):
    """[(b0, b1), ...] with every listed per-image element count x (b1 - b0) x 4 bytes under MAX_TENSOR_BYTES; one range = no split."""
    per = max(per_image_elems) * 4
    if B * per < MAX_TENSOR_BYTES or B == 1:
        return [(0, B)]
    step = max(1, int((MAX_TENSOR_BYTES - 1) // per))
    return [(b, min(B, b + step)) for b in range(0, B, step)]


def conv2d_fwd(x, w, bias, stride, pad, drop_p=0.0, drop_key=0, dil=1, w_amax=None):
    p = ConvProblem.of(x.shape, w.shape, stride, pad, dil)
    ranges = p.batch_ranges() if drop_p == 0.0 else [(0, p.B)]
    if len(ranges) > 1:
        return torch.cat([conv2d_fwd(x[b0:b1], w, bias, stride, pad, 0.0, 0, dil, w_amax) for b0, b1 in ranges])
    y = torch.empty(p.y_shape, device=x.device, dtype=torch.float32)
    ws, ws_bytes, packed = _pack_for(w, x.device, p, 0)
    _launch_conv(packed, p.kind(0), p.flops, "fs_conv2d_fwd", hip.ptr(x), hip.ptr(rsck(w)), hip.ptr(bias),
            hip.ptr(y), *p, float(drop_p), int(drop_key), hip.ptr(ws), ws_bytes, hip.ptr(w_amax))
    return y


# ---- weight packs that outlive the call ------------------------------------------------------------------------------------------
# Every split-precision conv kernel starts with a small launch that writes the layer's weights, split into their 16-bit terms in
# consumption order, into its scratch (438 + 186 such launches per HRNet step).  The library can keep a pack across calls
# (fs_conv2d_pack / fs_conv2d_ws_mode): a parameter whose owner says when it changes -- an optimiser arena (train.FlatParams bumps
# its epoch word at FlatAdam.step, a broadcast, load_state_dict) or static_weight_packs(module) for a serving process -- then keeps one
# scratch per (problem, direction, precision mode); with an arena, `train_step` refills the scratches used in the last step on a side
# stream right after the optimiser step (repack_weights) and the conv entry points are told the scratch is already packed.
# Measured on the headline step (profiles/r04/pack_persist_ab.txt): +-0 (374.7 / 372.7 / 372.9 -> 374.6 / 373.5 / 372.7 img/s); with NO
# pack launch at all (stale packs, timing only) 172.0 -> 170.7 ms -- the 4.5 ms the packs take when the kernels are serialised is
# hidden in the real step, and packs on a side stream still need the CUs the persistent conv kernels fill.  configs[4] +1-2 %,
# configs[3] -0.7 % (19 ms more host time per step).  So: OFF for arena parameters unless FS_PACK_PERSIST=1 (read once); always on
# for parameters marked static.  Parameters with neither (bare tensors in tests, derived weights built per call) pack per call.
PACK_PERSIST = os.environ.get("FS_PACK_PERSIST", "0") == "1"
PACK_GROUP = 32           # packs per hand-over event of the prefetch
_PACK_ORDER = []          # weak references to every live pack, in first-use order (= the order the next step needs them)
_PACK_SIDE = {}           # device index -> torch Stream of the prefetch


class _PackGroup:
    __slots__ = ("event", "waited")

    def __init__(self):
        self.event, self.waited = None, set()


class _Pack:
    __slots__ = ("w", "args", "transposed", "ws", "n", "mode", "cell", "epoch", "version", "used", "group", "stream", "ready", "__weakref__")


def _pack_for(w, device, problem, transposed):
    """(scratch | None, bytes, already packed?) for a conv entry point on weight tensor `w`."""
    n = problem.ws_bytes(transposed)
    if n == 0:
        return None, 0, False
    cell = getattr(w, "_fs_epoch", None) if (PACK_PERSIST or getattr(w, "_fs_static", False)) else None
    if cell is None or not problem.pack_persistent(transposed, n):
        return torch.empty(n, device=device, dtype=torch.uint8), n, False
    packs = w.__dict__.get("_fs_packs")
    if packs is None:
        packs = w.__dict__["_fs_packs"] = {}
    mode = hip.get_conv_precision()
    key = (transposed, *problem, mode)
    e = packs.get(key)
    if e is None:
        e = packs[key] = _Pack()
        e.w, e.args, e.transposed, e.n, e.mode = weakref.ref(w), key[1:13], transposed, n, mode
        e.ws = torch.empty(n, device=device, dtype=torch.uint8)
        e.cell, e.epoch, e.version, e.group, e.stream, e.ready = cell, -1, -1, None, None, set()
        _PACK_ORDER.append(weakref.ref(e))
    e.used = True
    so = hip.stream_override()
    cur = so if so is not None else hip._stream()
    if (e.cell is cell and e.epoch == cell[0] and e.version == w._version):
        if cur not in e.ready:          # first use on this stream since the pack was enqueued: order the stream behind it
            g = e.group
            if g is not None:
                if cur not in g.waited:
                    # the wait goes on `cur`, the stream the launch uses (which is the thread's stream override when that is set), not on torch's
                    # current stream
                    (torch.cuda.current_stream() if cur == hip._stream() else torch.cuda.ExternalStream(cur)).wait_event(g.event)
                    g.waited.add(cur)
            elif e.stream is not None and e.stream != cur:
                hip.stream_wait(cur, e.stream)
            e.ready.add(cur)
        return e.ws, n, True
    # stale (or new): this call packs on its own stream, later calls of the same epoch run on the result.  The scratch is rewritten IN
    # PLACE: consumers of the previous pack on other streams (HRNet branch streams, the autograd streams of the bwd-data packs) must
    # have finished reading it first
    for s_prev in e.ready:
        if s_prev != cur:
            hip.stream_wait(cur, s_prev)
    if e.stream is not None and e.stream != cur and e.stream not in e.ready:
        hip.stream_wait(cur, e.stream)
    e.cell, e.epoch, e.version, e.group, e.stream, e.ready = cell, cell[0], w._version, None, cur, {cur}
    return e.ws, n, False


def static_weight_packs(module, on=True):
    """Serving: the parameters of `module` do not change between forwards (no optimiser): keep every conv layer's weight pack after its
    first forward -- no pack launch from the second forward on.  Call again after rewriting the weights through anything that does not
    move torch's version counters; load_state_dict and in-place torch ops are seen without it."""
    for p in module.parameters():
        if on:
            cell = p.__dict__.get("_fs_epoch")
            if cell is None:
                p._fs_epoch = [0]
            else:
                cell[0] += 1
            p._fs_static = True
        else:
            p.__dict__.pop("_fs_static", None)
            p.__dict__.pop("_fs_packs", None)


def repack_weights():
    """Refill, on a side stream, every weight pack that was used since the last call and whose arena has been rewritten since it was
    packed (train.train_step calls this right after the optimiser steps; a frozen optimiser's packs stay valid and are skipped).  The
    consuming streams wait for the event of the pack's group at first use (_pack_for)."""
    if not _PACK_ORDER or TIMER is not None:
        return
    mode = hip.get_conv_precision()
    todo, live = [], []
    for r in _PACK_ORDER:
        e = r()
        if e is None:
            continue
        live.append(r)
        w = e.w()
        if w is None or not e.used or e.mode != mode:
            continue
        e.used = False
        cell = getattr(w, "_fs_epoch", None)
        if cell is None or (e.cell is cell and e.epoch == cell[0] and e.version == w._version):
            continue
        todo.append((e, w, cell))
    _PACK_ORDER[:] = live
    if not todo:
        return
    dev = todo[0][1].device
    side = _PACK_SIDE.get(dev.index)
    if side is None:
        side = _PACK_SIDE[dev.index] = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())          # the optimiser step (and the arena's max|w| refresh) come first
    raw = side.cuda_stream
    hip.set_stream_override(raw)
    try:
        group = _PackGroup()
        for i, (e, w, cell) in enumerate(todo):
            hip.call("fs_conv2d_pack", hip.ptr(rsck(w)), *e.args, e.transposed, hip.ptr(e.ws), e.n, hip.ptr(weight_amax(w)))
            e.cell, e.epoch, e.version, e.group, e.stream, e.ready = cell, cell[0], w._version, group, raw, set()
            if (i + 1) % PACK_GROUP == 0 or i + 1 == len(todo):
                group.event = torch.cuda.Event()
                group.event.record(side)
                group = _PackGroup()
    finally:
        hip.set_stream_override(None)


def _launch_conv(packed, kind, flops, name, *args):
    """_launch for the conv entry points; packed = their scratch already holds the weight pack (fs_conv2d_ws_mode)."""
    if not packed:
        return _launch(kind, flops, name, *args)
    if TIMER is None:
        hip.call_packed(name, *args)
    else:
        TIMER.launch(kind, flops, lambda: hip.call_packed(name, *args), tag=(name,) + tuple(a for a in args if type(a) is int and a < (1 << 20)))


FUSE_BN_STATS = True     # BatchNorm batch statistics come out of the conv epilogue (fs_conv2d_fwd_stats)
FUSE_EVAL_BN = True      # inference: eval-mode BatchNorm + residual + activation in the conv epilogue (fs_conv2d_fwd_affine_act)
# BatchNorm-backward column sums come out of the kernel that produces the gradient, where one does (FanOut's add, the F(2,3) bwd-data
# epilogue); FS_FUSE_BN_BWD=0 (read once, A/B runs) keeps every layer on its own reduction pass
FUSE_BN_BWD_SUMS = os.environ.get("FS_FUSE_BN_BWD", "1") != "0"


def conv2d_fwd_stats(x, w, bias, stride, pad, drop_p=0.0, drop_key=0, dil=1, w_amax=None):
    """Forward conv + per-workgroup BatchNorm partial sums (slab [nwg][Cout][2])."""
    p = ConvProblem.of(x.shape, w.shape, stride, pad, dil)
    ranges = p.batch_ranges() if drop_p == 0.0 else [(0, p.B)]
    if len(ranges) > 1:          # slab rows of the ranges concatenate: the finalize pass sums over all of them
        parts = [conv2d_fwd_stats(x[b0:b1], w, bias, stride, pad, 0.0, 0, dil, w_amax) for b0, b1 in ranges]
        return torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts]), sum(q[2] for q in parts)
    y = torch.empty(p.y_shape, device=x.device, dtype=torch.float32)
    ws, ws_bytes, packed = _pack_for(w, x.device, p, 0)
    nwg = p.stats_slabs(ws_bytes)
    slab = torch.empty(nwg * p.Cout * 2, device=x.device, dtype=torch.float32)
    _launch_conv(packed, p.kind(0), p.flops, "fs_conv2d_fwd_stats", hip.ptr(x), hip.ptr(rsck(w)), hip.ptr(bias), hip.ptr(y), hip.ptr(slab),
            *p, float(drop_p), int(drop_key), hip.ptr(ws), ws_bytes, hip.ptr(w_amax))
    return y, slab, nwg


def _unmask_bits(amask, like):
    """1 byte per 4 channels -> float {0,1} tensor shaped like `like` (fallback path only)."""
    bits = (amask.view(-1, 1) >> torch.arange(4, device=amask.device, dtype=torch.uint8)) & 1
    return bits.reshape(like.shape).to(like.dtype)


def conv2d_bwd_data(dy, w, x_shape, stride, pad, dil=1, w_amax=None, src_bn=None, addend=None):
    """dX of conv2d.  src_bn = the `_fs_bn` record of the layer that PRODUCED x (x = its output z, this conv its consumer): where the
    kernel this shape runs on can, its epilogue also forms that layer's BatchNorm-backward column sums and the slab is left in BN_SLABS
    under dx's address for ConvBnAct.backward to pick up (if autograd adds another consumer's gradient to dx the sum is a new tensor,
    the lookup misses and the layer runs its own reduction pass).  addend = (dz, mask bytes | None): a second gradient of x -- the
    residual branch's -- added in the same epilogue (ConvBnAct.backward stashes it in PENDING_RES only after asking the library that
    this shape's kernel takes it)."""
    p = ConvProblem.of(x_shape, w.shape, stride, pad, dil)
    assert tuple(dy.shape) == p.y_shape, (tuple(dy.shape), p)
    ranges = p.batch_ranges()
    if len(ranges) > 1:          # without the fused extras; the addend joins afterwards
        dx = torch.cat([conv2d_bwd_data(dy[b0:b1], w, p.at_batch(b1 - b0).x_shape, stride, pad, dil, w_amax) for b0, b1 in ranges])
        if addend is not None:
            a_src, a_mask = addend
            dx += a_src if a_mask is None else a_src * _unmask_bits(a_mask, a_src)
        return dx
    dx = torch.empty(p.x_shape, device=dy.device, dtype=torch.float32)
    kind = p.kind(1)
    ws, ws_bytes, packed = _pack_for(w, dy.device, p, 1)
    if src_bn is not None and not (FUSE_BN_BWD_SUMS and FANOUT and tuple(src_bn[0].shape) == p.x_shape):
        src_bn = None
    if src_bn is not None or addend is not None:
        rows = p.bnsum_slabs(ws_bytes)
        if rows > 0:
            y, amask, mean, invstd = src_bn[:4] if src_bn is not None else (None, None, None, None)
            slab = torch.empty(rows * p.Cin * 2, device=dy.device, dtype=torch.float32) if src_bn is not None else None
            a_src, a_mask = addend if addend is not None else (None, None)
            _launch_conv(packed, kind, p.flops, "fs_conv2d_bwd_data_bnsum", hip.ptr(dy), hip.ptr(rsck(w)), hip.ptr(dx), *p,
                    hip.ptr(ws), ws_bytes, hip.ptr(w_amax), hip.ptr(y), hip.ptr(amask), hip.ptr(mean), hip.ptr(invstd),
                    hip.ptr(slab), hip.ptr(a_src), hip.ptr(a_mask))
            if slab is not None:
                BN_SLABS[(dx.data_ptr(), y.data_ptr())] = (slab, rows, dx)
            return dx
    _launch_conv(packed, kind, p.flops, "fs_conv2d_bwd_data", hip.ptr(dy), hip.ptr(rsck(w)), hip.ptr(dx), *p, hip.ptr(ws), ws_bytes, hip.ptr(w_amax))
    if addend is not None:          # the library no longer takes the addend for this shape (precision mode changed since the stash): add here
        a_src, a_mask = addend
        dx = dx + (a_src if a_mask is None else a_src * _unmask_bits(a_mask, a_src))
    return dx


# Weight / affine gradients of a parameter whose `.grad` IS its slice of a flat gradient arena (train.FlatParams registers the
# slice as `p._fs_grad_home`) are ADDED straight into that slice by the kernels (conv weights and BatchNorm affines alike) and
# the autograd function returns None for them: no temporary, no AccumulateGrad add.  The decision is per parameter -- there is
# no process-wide mode: a parameter outside any arena, or whose `.grad` was re-pointed (module.zero_grad() -> None -> a fresh
# tensor), takes the ordinary autograd path.  The arena is zeroed once per step (optimizer.zero_grad), so repeated backwards
# accumulate exactly like `.grad`.  DIRECT_GRAD = False (or FS_DIRECT_GRAD=0) switches the direct path off altogether.
#
# torch's DistributedDataParallel (the reference's call site, train_deform_semantic.py:395) learns that a gradient is ready from a
# hook on the parameter's AccumulateGrad node, which a kernel that adds straight into the arena never fires.  A forward that runs
# inside a DDP wrapper therefore suspends the direct path for itself and its backward (models.DeformSegmentationModule.forward
# -> under_torch_ddp): gradients are returned to autograd, AccumulateGrad adds them into the same arena views in place, the
# reducer sees every one of them.
DIRECT_GRAD = os.environ.get("FS_DIRECT_GRAD", "1") != "0"
DDP_ACTIVE = False       # set per forward by models.DeformSegmentationModule.forward


def under_torch_ddp(module) -> bool:
    """True while `module.forward` is being run by a torch DistributedDataParallel wrapper around `module`."""
    ddp_cls = torch.nn.parallel.DistributedDataParallel
    active = getattr(ddp_cls, "_active_ddp_module", None)
    return active is not None and getattr(active, "module", None) is module


PARAM_VIEW_DIRECT = os.environ.get("FS_PARAM_VIEW_DIRECT", "1") != "0"


def param_view(leaf, fn):
    """fn(leaf): a VIEW of a parameter over the same storage (nn.Linear's (out, in) weight as the (out, in, 1, 1) filter of a 1x1 conv, a
    k x k stride-k filter as the (k*k*Cin, Cout) matrix of its patch rows) that remembers how it was made, so that a kernel writing the
    view's gradient can write it through the same view of the parameter's arena slice (_direct_grad_target) -- without that the gradient
    is a temporary that travels back through ViewBackward to an AccumulateGrad add: 370 small launches per configs[3] step."""
    v = fn(leaf)
    if PARAM_VIEW_DIRECT:
        v._fs_grad_via = (leaf, fn)
    return v


def _direct_grad_target(p):
    via = getattr(p, "_fs_grad_via", None)
    if via is not None:
        g = _direct_grad_target(via[0])
        if g is None:
            return None
        t = via[1](g)
        return t if (t.data_ptr() == g.data_ptr() and t.shape == p.shape and t.stride() == p.stride()) else None
    home = getattr(p, "_fs_grad_home", None)
    if not DIRECT_GRAD or DDP_ACTIVE or home is None or not p.is_leaf:
        return None
    g = p.grad
    if g is not None and g.is_cuda and g.data_ptr() == home[0].data_ptr() + 4 * home[1] and g.shape == p.shape and g.stride() == p.stride():
        return g
    return None


def conv2d_bwd_weight(x, dy, w_shape, stride, pad, out=None, dil=1, accumulate=False, keep=None):
    """dW of conv2d.  out = a gradient buffer in the weight's layout; accumulate=True adds into it (the DIRECT_GRAD arena
    is zeroed once per step by zero_grad, so the per-layer memset is skipped and repeated backwards accumulate like .grad)."""
    p = ConvProblem.of(x.shape, w_shape, stride, pad, dil)
    assert tuple(dy.shape) == p.y_shape, (tuple(dy.shape), p)
    ranges = p.batch_ranges()
    if len(ranges) > 1:          # the ranges' gradients accumulate in one buffer
        buf = out if out is not None else new_rsck_weight(p.Cout, p.Cin, p.R, p.S, device=x.device)
        for i, (b0, b1) in enumerate(ranges):
            conv2d_bwd_weight(x[b0:b1], dy[b0:b1], w_shape, stride, pad, out=buf, dil=dil, accumulate=accumulate or i > 0)
        return buf
    dw = rsck(out) if out is not None else torch.empty(p.R, p.S, p.Cin, p.Cout, device=x.device, dtype=torch.float32)
    k3 = p[7:] == (3, 3, 1, 1, 1) and p.Cin % 4 == 0 and p.Cout % 4 == 0 and p.Cin >= 16 and p.Cout >= 16
    dws_bytes = p.wgrad_ws_bytes()          # deterministic mode; strided 3x3 layers
    dws = torch.empty(dws_bytes, device=x.device, dtype=torch.uint8) if dws_bytes else None
    if keep is not None and dws is not None:
        keep.append(dws)          # the launch runs on a side stream: the scratch must outlive this call (join_wgrad_streams)
    _launch("wgrad3x3" if (k3 and hip.get_conv_precision() != "f32") else "conv_wgrad", p.flops,
            "fs_conv2d_bwd_weight", hip.ptr(x), hip.ptr(dy), hip.ptr(dw), *p, 1 if accumulate else 0, hip.ptr(dws), dws_bytes)
    return out if out is not None else dw.permute(3, 2, 0, 1)


def colsum(x2d_rows, C, into=None):
    """Column sums (bias gradients).  into = a gradient-arena target: the sums are ADDED to it and None is returned."""
    M = x2d_rows.numel() // C
    scratch = torch.empty(hip.query("fs_colsum_scratch_floats", M, C), device=x2d_rows.device, dtype=torch.float32)
    if into is not None:
        hip.call("fs_colsum", hip.ptr(x2d_rows), M, C, hip.ptr(into), 1, hip.ptr(scratch))
        return None
    out = torch.empty(C, device=x2d_rows.device, dtype=torch.float32)
    hip.call("fs_colsum", hip.ptr(x2d_rows), M, C, hip.ptr(out), 0, hip.ptr(scratch))
    return out


# ----------------------------------------------------------------------------------------------
# Layers fed by 3 or 5 input channels (HRNet stem, saliency net) as aligned problems: the generic scalar-channel kernels spend
# 0.4-1.3 ms per launch on them where the aligned ones are bound by the 105-315 MB of activations they move.
# ----------------------------------------------------------------------------------------------
PAD_ODD_CHANNELS = os.environ.get("FS_PAD_ODD_CHANNELS", "1") != "0"


def padded_in_channels(cin):
    """Input-channel count the aligned kernels accept for a layer with `cin` channels (bwd-weight wants >= 16, all want x4)."""
    return 16 if cin < 16 else (cin + 3) // 4 * 4


class PadWeightChannels(Function):
    """(Cout,Cin,R,S) RSCK weight -> (Cout,Cp,R,S) RSCK weight with zero taps for the padding channels; backward slices."""

    @staticmethod
    def forward(ctx, w, cp):
        cout, cin, r, s = w.shape
        wp = new_rsck_weight(cout, cp, r, s, device=w.device)
        v = rsck(wp)
        v.zero_()
        v[:, :, :cin, :].copy_(rsck(w))
        ctx.cin = cin
        return wp

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.cin], None


class CenterTap(Function):
    """(Cout,Cin,3,3) RSCK weight -> its centre tap as a (Cout,Cin,1,1) RSCK weight; backward = zeros with the centre filled in."""

    @staticmethod
    def forward(ctx, w):
        cout, cin, r, s = w.shape
        wc = new_rsck_weight(cout, cin, 1, 1, device=w.device)
        rsck(wc)[0, 0].copy_(rsck(w)[r // 2, s // 2])
        ctx.rs = (r, s)
        return wc

    @staticmethod
    def backward(ctx, g):
        r, s = ctx.rs
        cout, cin = g.shape[:2]
        gw = new_rsck_weight(cout, cin, r, s, device=g.device)
        v = rsck(gw)
        v.zero_()
        v[r // 2, s // 2].copy_(rsck(g)[0, 0])
        return gw


def pad_in_channels(x, w):
    """(x (B,H,W,Cin), w) -> (x padded with zero channels, w padded alike) when Cin is not a multiple of 4 and the split-precision
    kernels are on; exact: the extra products are 0 * 0."""
    cin = w.shape[1]
    if not PAD_ODD_CHANNELS or cin % 4 == 0 or w.shape[2] * w.shape[3] > 32 or hip.get_conv_precision() == "f32":
        return x, w          # aligned already, or a filter beyond the aligned kernels' 32 taps (7x7 ResNet stem): generic kernels
    cp = padded_in_channels(cin)
    xp = torch.nn.functional.pad(x, (0, cp - cin))
    # the padded tensor stands for x in the layer: it keeps x's producer / fan-out records, so ConvBnAct registers itself as the fan-out's
    # conv consumer (FAN_GEOM, FAN_DONE) as it does without padding.  Every reader of these records compares shapes before a kernel takes
    # a tensor of the unpadded width (conv2d_bwd_data: src_bn; StashGrad / ConvBnAct.backward: the addend), so a padded layer keeps its
    # own reduction pass and the fan-out adds the other alias's gradient
    for tag in ("_fs_fan", "_fs_after_fan", "_fs_bn"):
        v = getattr(x, tag, None)
        if v is not None:
            setattr(xp, tag, v)
    return xp, PadWeightChannels.apply(w, cp)


FANOUT = os.environ.get("FS_FANOUT", "1") != "0"

# Launch-latency-bound layers (DeepLab's 10x10 / 20x20 stages at 16 images per GPU: ~1 700 launches of 5-15 us per 30 ms step, the GPU
# mostly waiting on the dependency chain): a weight gradient has no consumer before the optimiser, so below WGRAD_SIDE_FLOPS it is
# launched on a side stream beside the bwd-data chain.  Only where the kernel adds straight into the gradient arena (no autograd consumer);
# FlatAdam.step / zero_grad and train.allreduce_gradients join the side stream first (join_wgrad_streams).  The headline layers are 30 GFLOP
# each and keep the one-stream order: there the GPU is saturated and a side stream was measured at +-0.
WGRAD_SIDE_FLOPS = float(os.environ.get("FS_WGRAD_SIDE_GFLOP", "4")) * 1e9
_WGRAD_SIDE = {}            # device index -> (torch Stream, raw handle)
_WGRAD_SIDE_BUSY = {}       # raw handle of a side stream with launches since the last join -> tensors those launches read or write
                            # (kept alive while the side stream may still use them: they were allocated on the launching stream's pool,
                            # so freeing them earlier would let the allocator hand them out again; cheaper than three record_stream calls)
_WGRAD_RETIRED = []         # (event recorded on the side stream, tensors): kept lists that were joined or rotated out; dropped once the
                            # event has COMPLETED -- a join only enqueues a wait, the side stream may still be reading the tensors
_WGRAD_ROTATE = 64          # side launches per kept list before it is rotated out (bounds what a long backward holds on to)
_WGRAD_JOIN_QUEUED = [False]


def _wgrad_side_stream(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    s = _WGRAD_SIDE.get(key)
    if s is None:
        st = torch.cuda.Stream(device=device)
        s = _WGRAD_SIDE[key] = (st, st.cuda_stream)
    return s[1]


def _wgrad_stream_obj(raw):
    for st, h in _WGRAD_SIDE.values():
        if h == raw:
            return st
    return None


def _wgrad_retire(raw, keep):
    """The kept tensors of side stream `raw` may be dropped once everything enqueued there so far has run: remember them under an event.
    (Under stream capture nothing runs and an event cannot be queried; the caller drops the list at the join instead -- every node
    captured behind the join is ordered behind the side launches, and the graph's private pool keeps the addresses for its replays.)"""
    st = _wgrad_stream_obj(raw)
    if st is None or not keep or torch.cuda.is_current_stream_capturing():
        return
    ev = torch.cuda.Event()
    ev.record(st)
    _WGRAD_RETIRED.append((ev, keep))


def _wgrad_reap():
    if _WGRAD_RETIRED and not torch.cuda.is_current_stream_capturing():
        _WGRAD_RETIRED[:] = [(ev, keep) for ev, keep in _WGRAD_RETIRED if not ev.query()]


def join_wgrad_streams():
    """The current stream waits for every weight-gradient launch that went to a side stream since the last join.  Since round 5 this runs
    as a final callback of the autograd engine at the end of every backward that used the side stream (_queue_wgrad_join), i.e. with the
    CALLER's current stream -- the stream backward() returns on -- so any reader of .grad / the gradient arena after backward() is ordered
    behind the side stream like behind every other gradient.  FlatAdam.step / zero_grad and train.allreduce_gradients still call it as a
    backstop (no-ops then)."""
    if _WGRAD_SIDE_BUSY:
        cur = hip._stream()
        for h, keep in _WGRAD_SIDE_BUSY.items():
            hip.stream_wait(cur, h)
            _wgrad_retire(h, keep)
        _WGRAD_SIDE_BUSY.clear()
    _wgrad_reap()


def _wgrad_join_callback():
    _WGRAD_JOIN_QUEUED[0] = False
    join_wgrad_streams()


def _queue_wgrad_join():
    """First side launch of a backward pass: have the engine run the join when the pass ends (torch runs final callbacks after it has
    ordered the caller's stream behind the leaf streams, with the caller's current streams set)."""
    if _WGRAD_JOIN_QUEUED[0]:
        return
    try:
        torch.autograd.Variable._execution_engine.queue_callback(_wgrad_join_callback)
        _WGRAD_JOIN_QUEUED[0] = True
    except RuntimeError:          # not inside an engine run (a Function.backward called by hand): the explicit joins remain
        pass


def _wgrad_side_or_inline(x, dy, w_shape, stride, pad, dil, tgt):
    """The weight gradient of ConvBnAct.backward: on the side stream where the kernel adds straight into the gradient arena (tgt) and the
    layer is below WGRAD_SIDE_FLOPS, else on the current stream.  Returns what autograd gets: None where the arena took the gradient."""
    # (not under stream capture: forking the side stream into a capture once per layer and joining it once at the end ends in a host
    #  segmentation fault inside hipStreamEndCapture on ROCm 7.2 -- tools/probes/graph_probe.py, profiles/r05/graph_probe.txt)
    if (tgt is not None and ConvProblem.of(x.shape, w_shape, stride, pad, dil).flops < WGRAD_SIDE_FLOPS and TIMER is None
            and not torch.cuda.is_current_stream_capturing()):
        side = _wgrad_side_stream(dy.device)
        _queue_wgrad_join()                       # backward() returns with its stream ordered behind the side stream
        hip.stream_wait(side, hip._stream())      # dy (and x) were produced on the current stream
        keep = _WGRAD_SIDE_BUSY.setdefault(side, [])
        if len(keep) >= _WGRAD_ROTATE and not torch.cuda.is_current_stream_capturing():
            # a long backward (configs[4]: every layer is small) does not hold on to all of its activations and gradients: lists
            # retire under an event and go when it has completed
            _wgrad_retire(side, keep)
            keep = _WGRAD_SIDE_BUSY[side] = []
            _wgrad_reap()
        keep.append((x, dy))
        hip.set_stream_override(side)
        try:
            conv2d_bwd_weight(x, dy, w_shape, stride, pad, out=tgt, dil=dil, accumulate=True, keep=keep)
        finally:
            hip.set_stream_override(None)
        return None
    dw = conv2d_bwd_weight(x, dy, w_shape, stride, pad, out=tgt, dil=dil, accumulate=tgt is not None)
    return None if tgt is not None else dw


# BatchNorm-backward column sums that the PRODUCER of a gradient tensor already formed (FanOut.backward below, the bwd-data epilogue of the
# consumer conv, HrFuse.backward): (dz.data_ptr(), y.data_ptr()) -> (slab, nslab, dz), y = the conv output of the layer the sums are for
# (one fuse gradient is the output gradient of up to three layers).  The entry keeps dz alive, so its address cannot be reused while the
# entry exists; ConvBnAct.backward pops it.  Cleared at the start of every module forward.
BN_SLABS = {}


class FanOut(Function):
    """x -> n aliases of x, one per consumer.  Backward: ONE n-ary HIP add of the consumers' gradients (fs_add_n, up to four at a
    time) instead of the n - 1 binary ATen adds the autograd engine would issue -- the last ATen compute kernel inside the step.
    When x is the output of a conv + BatchNorm + activation layer (ConvBnAct tags it with `_fs_bn`), the last add also forms that
    layer's BatchNorm-backward column sums (fs_add_n_bnsum): the layer's own reduction pass over (dz, y) is then skipped."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.bn = getattr(x, "_fs_bn", None)
        ctx.set_materialize_grads(False)      # a consumer whose gradient was absorbed elsewhere returns None: keep it None, not a zero tensor
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [g if g.is_contiguous() else g.contiguous() for g in grads if g is not None]
        if not gs:
            return None, None
        acc = gs[0]
        rest = gs[1:]
        if rest and (acc.numel() % 4 or not acc.is_cuda):
            for g in rest:
                acc = acc + g
            return acc, None
        bn = ctx.bn if FUSE_BN_BWD_SUMS else None
        while rest:
            take, rest = rest[:3], rest[3:]
            out = torch.empty_like(acc)
            if bn is not None and not rest and acc.dim() == 4 and acc.shape[-1] % 4 == 0 and acc.shape == bn[0].shape:
                y, amask, mean, invstd, act = bn
                C = acc.shape[-1]
                M = acc.numel() // C
                nslab = hip.bn_bwd_slabs(M, C)
                slab = torch.empty(nslab * C * 2, device=acc.device, dtype=torch.float32)
                hip.call("fs_add_n_bnsum", hip.ptr(acc), hip.ptr(take[0]), hip.ptr(take[1]) if len(take) > 1 else None,
                         hip.ptr(take[2]) if len(take) > 2 else None, hip.ptr(out), hip.ptr(amask), hip.ptr(y), hip.ptr(mean),
                         hip.ptr(invstd), M, C, act if amask is not None else ACT_NONE, hip.ptr(slab))
                BN_SLABS[(out.data_ptr(), y.data_ptr())] = (slab, nslab, out)
            else:
                hip.call("fs_add_n", hip.ptr(acc), hip.ptr(take[0]), hip.ptr(take[1]) if len(take) > 1 else None,
                         hip.ptr(take[2]) if len(take) > 2 else None, hip.ptr(out), acc.numel())
            acc = out
        return acc, None


_FAN_IDS = [0]
# A two-way fan-out whose consumers are a convolution and a residual input (BasicBlock, models/hrnetv2_nodownsp.py:46-62): the conv
# consumer's forward leaves its ConvProblem in FAN_GEOM under the fan id, the residual consumer's backward (it always runs first) asks the
# library whether that convolution's bwd-data epilogue takes an addend and, if so, leaves (dz, mask bytes) in PENDING_RES instead of
# materialising the residual gradient; the conv consumer's backward passes it on (conv2d_bwd_data) -- no n-ary add, no dres tensor.
FAN_GEOM = {}
PENDING_RES = {}
FAN_DONE = set()        # fan ids whose conv consumer has run its backward


def reset_step_state():
    """Start of a module forward: drop the per-step records.  A residual gradient still waiting in PENDING_RES was never added to anything
    -- a silently wrong gradient -- so that is an error, not something to clear."""
    if PENDING_RES:
        left = sorted(PENDING_RES)
        PENDING_RES.clear()
        raise hip.HipLibraryError(f"residual gradients of fan-outs {left} were stashed for a convolution's bwd-data epilogue that never ran")
    BN_SLABS.clear()
    FAN_GEOM.clear()
    FAN_DONE.clear()
    _WGRAD_JOIN_QUEUED[0] = False      # (a backward that raised never ran its final callbacks)


def fan_out(x, n):
    """n references to x for n consumers (n >= 2 and FS_FANOUT on: through FanOut, else x itself n times)."""
    if n < 2 or not FANOUT or not x.requires_grad:
        return (x,) * n
    outs = FanOut.apply(x, n)
    if n == 2:
        _FAN_IDS[0] += 1
        tag = (_FAN_IDS[0], getattr(x, "_fs_bn", None))
        for o in outs:
            o._fs_fan = tag
    return outs


class StashGrad(Function):
    """Identity on one alias of a two-way fan-out whose OTHER alias feeds a convolution (C1: `feat` -> the 3x3 conv of the mask branch and ->
    the classification branch).  Backward: the gradient that arrives here is left in PENDING_RES under the fan id and None is returned, so the
    convolution's bwd-data adds it in its epilogue (one read) instead of FanOut.backward adding two 1.57 GB tensors in a pass of its own
    (806 us per configs[1] step).  The branch behind this node must run its backward BEFORE the convolution's: put the node in the forward
    AFTER the convolution branch (the engine runs ready nodes in reverse order of creation); if the convolution's backward came first anyway
    (FAN_DONE), the gradient is returned as usual and the fan-out adds it.  Likewise when no convolution registered itself as the fan-out's
    conv consumer (FAN_GEOM), or when that convolution reads a zero-padded copy of the tensor (pad_in_channels: another channel count than
    this gradient's): a stash nobody pops would be a gradient that is never added."""

    @staticmethod
    def forward(ctx, x, fan_id):
        ctx.fan_id = fan_id
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        if g is None or ctx.fan_id in FAN_DONE or ctx.fan_id in PENDING_RES or not (FUSE_BN_BWD_SUMS and FANOUT):
            return g, None
        geom = FAN_GEOM.get(ctx.fan_id)
        if geom is None or geom.x_shape != tuple(g.shape):
            return g, None
        PENDING_RES[ctx.fan_id] = (g if g.is_contiguous() else g.contiguous(), None)
        return None, None


FANOUT_SUBSAMPLE = os.environ.get("FS_FANOUT_SUBSAMPLE", "1") != "0"


class FanOutSubsample(Function):
    """x (B,H,W,C) -> (x, x[:, ::s, ::s, :] contiguous).  Backward: the subsampled branch's gradient is added in place into the
    full-resolution branch's gradient at the sampled pixels (that tensor is the fresh dX of the branch's first consumer)."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        ctx.shape = x.shape
        return x.view_as(x), x[:, ::s, ::s, :].contiguous()

    @staticmethod
    def backward(ctx, g_full, g_sub):
        s = ctx.s
        if g_full is None:
            g_full = torch.zeros(ctx.shape, device=g_sub.device, dtype=g_sub.dtype)
        elif not g_full.is_contiguous():
            g_full = g_full.contiguous()
        if g_sub is not None:
            g_full[:, ::s, ::s, :].add_(g_sub)
        return g_full, None


def act_has_bwd(act, amask):
    """The activation derivative is available to another kernel: no activation, or the 1-byte masks were written."""
    return act == ACT_NONE or amask is not None


# ----------------------------------------------------------------------------------------------
# conv (+bias) (+dropout) + BatchNorm + residual + activation
# ----------------------------------------------------------------------------------------------
class ConvBnAct(Function):
    """z = act(BN(dropout(conv(x, w) + bias)) + res).
    meta: dict(stride, pad, act, training, momentum, drop_p, drop_key, running_mean, running_var,
    num_batches_tracked)."""

    @staticmethod
    def forward(ctx, x, w, bias, gamma, beta, res, meta):
        training = meta["training"]
        drop_p = meta["drop_p"] if training else 0.0
        Cout, Cin = w.shape[0], w.shape[1]
        fused_stats = training and FUSE_BN_STATS and Cin % 4 == 0 and Cout % 4 == 0
        dil = meta.get("dil", 1)
        wa = weight_amax(w)
        # (ctx.needs_input_grad mirrors requires_grad of the inputs even under no_grad: "no backward will follow" = grad mode was off at
        #  the call site, which modules.conv_bn_act records in meta before Function.apply switches it off)
        if not training and FUSE_EVAL_BN and not meta.get("grad_enabled", True) and Cin % 4 == 0 and Cout % 4 == 0:
            # inference: eval-mode BatchNorm, residual and activation in the conv epilogue where this shape's kernel has one
            p = ConvProblem.of(x.shape, w.shape, meta["stride"], meta["pad"], dil)
            if p.affine_act_ok(p.ws_bytes(0)):
                coef = torch.empty(2, Cout, device=x.device, dtype=torch.float32)
                hip.call("fs_bn_eval_affine", hip.ptr(meta["running_mean"]), hip.ptr(meta["running_var"]), hip.ptr(gamma), hip.ptr(beta), Cout,
                         BN_EPS, hip.ptr(coef[0]), hip.ptr(coef[1]))
                z = torch.empty(p.y_shape, device=x.device, dtype=torch.float32)
                ws, ws_bytes, packed = _pack_for(w, x.device, p, 0)
                _launch_conv(packed, p.kind(0), p.flops, "fs_conv2d_fwd_affine_act", hip.ptr(x), hip.ptr(rsck(w)), hip.ptr(bias), hip.ptr(coef[0]),
                        hip.ptr(coef[1]), hip.ptr(res), hip.ptr(z), *p, meta["act"], hip.ptr(ws), ws_bytes, hip.ptr(wa))
                return z
        if fused_stats:
            y, slab, nwg = conv2d_fwd_stats(x, w, bias, meta["stride"], meta["pad"], drop_p, meta["drop_key"], dil, w_amax=wa)
        else:
            y = conv2d_fwd(x, w, bias, meta["stride"], meta["pad"], drop_p, meta["drop_key"], dil, w_amax=wa)
        B, Ho, Wo, C = y.shape
        M = B * Ho * Wo
        mean = torch.empty(C, device=y.device, dtype=torch.float32)
        invstd = torch.empty(C, device=y.device, dtype=torch.float32)
        if fused_stats:
            hip.call("fs_bn_finalize_slab", hip.ptr(slab), nwg, M, C, float(meta["momentum"]), BN_EPS,
                     hip.ptr(meta["running_mean"]), hip.ptr(meta["running_var"]), hip.ptr(mean), hip.ptr(invstd))
            meta["num_batches_tracked"].add_(1)
        elif training:
            sums = torch.empty(hip.query("fs_bn_stats_scratch_doubles", M, C), device=y.device, dtype=torch.float64)
            hip.call("fs_bn_stats", hip.ptr(y), M, C, float(meta["momentum"]), BN_EPS, hip.ptr(meta["running_mean"]),
                     hip.ptr(meta["running_var"]), hip.ptr(mean), hip.ptr(invstd), hip.ptr(sums))
            meta["num_batches_tracked"].add_(1)
        else:
            hip.call("fs_bn_eval_prepare", hip.ptr(meta["running_mean"]), hip.ptr(meta["running_var"]), C, BN_EPS,
                     hip.ptr(mean), hip.ptr(invstd))
        z = torch.empty_like(y)
        # activation-derivative bits for the backward passes (1 byte per 4 channels instead of re-reading z)
        amask = torch.empty(M * C // 4, device=y.device, dtype=torch.uint8) if (meta["act"] != 0 and any(ctx.needs_input_grad)) else None
        # timer "work" of the HBM-bound kinds = algorithmic bytes: every operand read once, every result written once
        _launch("bn_fwd", 4.0 * M * C * (2 + (res is not None)) + (M * C // 4 if amask is not None else 0),
                "fs_bn_act_fwd", hip.ptr(y), hip.ptr(mean), hip.ptr(invstd), hip.ptr(gamma), hip.ptr(beta), hip.ptr(res),
                hip.ptr(z), hip.ptr(amask), M, C, meta["act"])
        ctx.meta = dict(stride=meta["stride"], pad=meta["pad"], dil=dil, act=meta["act"], training=training, drop_p=drop_p,
                        drop_key=meta["drop_key"], has_bias=bias is not None, has_res=res is not None)
        ctx.save_for_backward(x, w, gamma, y, z if amask is None else None, mean, invstd, amask)
        ctx.beta_ref = beta
        ctx.w_amax = wa          # the weights do not change between this forward and its backward
        ctx.src_bn = getattr(x, "_fs_bn", None)       # x is the output of another conv + BatchNorm layer: its record, for the bwd-data epilogue
        ctx.fan = getattr(x, "_fs_fan", None)         # x is one of the two aliases of a fan-out: this conv may absorb the other alias's gradient
        if ctx.fan is not None:
            FAN_GEOM[ctx.fan[0]] = ConvProblem.of(x.shape, w.shape, meta["stride"], meta["pad"], dil)
            z._fs_after_fan = ctx.fan[0]              # z is computed FROM the fan-out's conv alias: a layer reading z runs its backward before this one
        rfan = getattr(res, "_fs_fan", None) if res is not None else None
        # The residual gradient may only be left for the fan-out's conv consumer when that consumer's backward is certain to run AFTER this
        # layer's: i.e. when this layer's own conv input was produced by it (BasicBlock: conv1 -> bn1 -> relu -> conv2 + x).  A residual
        # consumer that does not depend on the conv consumer is unordered against it and materialises its gradient as usual.
        ordered = rfan is not None and getattr(x, "_fs_after_fan", None) == rfan[0]
        ctx.res_fan = (rfan[0], FAN_GEOM.get(rfan[0])) if ordered else None
        if act_has_bwd(meta["act"], amask) and meta.get("grad_enabled", True) and any(ctx.needs_input_grad):
            # for the producer of dz (FanOut.backward / a consumer's bwd-data epilogue): this layer's BN-backward operands.  Only when a
            # backward will follow: the record keeps the pre-activation conv output alive as long as z lives
            z._fs_bn = (y, amask, mean, invstd, meta["act"])
        return z

    @staticmethod
    def backward(ctx, dz):
        x, w, gamma, y, z, mean, invstd, amask = ctx.saved_tensors
        m = ctx.meta
        dz = dz.contiguous()
        B, Ho, Wo, C = y.shape
        M = B * Ho * Wo
        dy = torch.empty_like(y)
        # residual gradient: absorbed by the bwd-data epilogue of the convolution that shares the fan-out with `res`, where it can be
        absorb = None
        if (m["has_res"] and ctx.res_fan is not None and ctx.res_fan[1] is not None and FUSE_BN_BWD_SUMS and FANOUT
                and (m["act"] == ACT_NONE or amask is not None)):
            fp = ctx.res_fan[1]          # the problem of the fan-out's conv consumer
            if fp.x_shape == tuple(y.shape) and fp.bnsum_slabs(fp.ws_bytes(1)) > 0 and ctx.res_fan[0] not in FAN_DONE:
                absorb = ctx.res_fan[0]
        dres = torch.empty_like(y) if (m["has_res"] and absorb is None) else None
        tg, tb = _direct_grad_target(gamma), _direct_grad_target(ctx.beta_ref)
        direct_affine = tg is not None and tb is not None
        dgamma = tg if direct_affine else torch.empty(C, device=y.device, dtype=torch.float32)
        dbeta = tb if direct_affine else torch.empty(C, device=y.device, dtype=torch.float32)
        # BatchNorm backward = column sums (unless the kernel that produced dz already formed them) -> finalize -> apply
        pre = BN_SLABS.pop((dz.data_ptr(), y.data_ptr()), None)
        if pre is not None and pre[2].shape == dz.shape:
            slab, nslab = pre[0], pre[1]
            slab.record_stream(torch.cuda.current_stream())
        else:
            nslab = hip.bn_bwd_slabs(M, C)
            slab = torch.empty(nslab * C * 2, device=y.device, dtype=torch.float32)
            _launch("bn_bwd", 0.0, "fs_bn_bwd_partial", hip.ptr(dz), hip.ptr(z), hip.ptr(amask), hip.ptr(y), hip.ptr(mean), hip.ptr(invstd),
                    M, C, m["act"], hip.ptr(slab))
        coef = torch.empty(4 * C, device=y.device, dtype=torch.float32)
        _launch("bn_bwd", 0.0, "fs_bn_bwd_finalize", hip.ptr(slab), nslab, hip.ptr(gamma), hip.ptr(mean), hip.ptr(invstd), M, C,
                1 if m["training"] else 0, hip.ptr(coef), hip.ptr(dgamma), hip.ptr(dbeta), 1 if direct_affine else 0)
        # timer "work" of the three launches together = algorithmic bytes: dz, y and the mask read once, dy [and dres] written once
        _launch("bn_bwd", 4.0 * M * C * (3 + m["has_res"]) + (M * C // 4 if amask is not None else 0),
                "fs_bn_bwd_apply", hip.ptr(dz), hip.ptr(z), hip.ptr(amask), hip.ptr(y), hip.ptr(coef), M, C, m["act"], float(m["drop_p"]),
                int(m["drop_key"]), hip.ptr(dy), hip.ptr(dres))
        if absorb is not None:
            PENDING_RES[absorb] = (dz, amask if m["act"] != ACT_NONE else None)
        tgt = _direct_grad_target(w)
        # this conv's own input: the other alias's gradient (if a residual consumer stashed it) joins dx in the epilogue, and then dx is
        # the WHOLE gradient of the fan-out's input, so that tensor's producer record (fan tag) is the one the BatchNorm sums are for
        pend = PENDING_RES.pop(ctx.fan[0], None) if ctx.fan is not None else None
        if ctx.fan is not None:
            FAN_DONE.add(ctx.fan[0])          # from here on a residual consumer of this fan-out must materialise its own gradient
        src_bn = ctx.src_bn if ctx.fan is None else (ctx.fan[1] if pend is not None else None)
        if not WGRAD_FIRST:
            dx = conv2d_bwd_data(dy, w, x.shape, m["stride"], m["pad"], m["dil"], w_amax=ctx.w_amax, src_bn=src_bn, addend=pend) if ctx.needs_input_grad[0] else None
        dw = _wgrad_side_or_inline(x, dy, w.shape, m["stride"], m["pad"], m["dil"], tgt)
        if WGRAD_FIRST:     # dx is what the next backward node reads: produce it last so it is the freshest tensor in the cache
            dx = conv2d_bwd_data(dy, w, x.shape, m["stride"], m["pad"], m["dil"], w_amax=ctx.w_amax, src_bn=src_bn, addend=pend) if ctx.needs_input_grad[0] else None
        dbias = colsum(dy, C) if m["has_bias"] else None
        if direct_affine:
            dgamma = dbeta = None
        return dx, dw, dbias, dgamma, dbeta, dres, None


class ConvBias(Function):
    """y = [dropout_p](conv(x, w) + bias) without normalisation (nn.Linear as a 1x1 conv, patch embeddings, sequence-reduction convs).
    drop_p > 0: the hidden-state Dropout that follows the layer (SegformerSelfOutput / MixFFN) runs in the conv epilogue -- same hash
    of the output's element index as the stand-alone fs_dropout -- and its backward masks dy once before the two gradient launches."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, drop_p=0.0, drop_key=0):
        ctx.save_for_backward(x, w)
        ctx.sp = (stride, pad, bias is not None, float(drop_p), int(drop_key))
        ctx.bias_ref = bias
        ctx.w_via = getattr(w, "_fs_grad_via", None)      # param_view's record, kept here: the saved tensor may come back as a new object
        return conv2d_fwd(x, w, bias, stride, pad, float(drop_p), int(drop_key))

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, has_bias, drop_p, drop_key = ctx.sp
        dy = dy.contiguous()
        if drop_p > 0.0:
            masked = torch.empty_like(dy)
            hip.call("fs_dropout", hip.ptr(dy), hip.ptr(masked), dy.numel(), drop_p, drop_key)
            dy = masked
        dx = conv2d_bwd_data(dy, w, x.shape, stride, pad) if ctx.needs_input_grad[0] else None
        if ctx.w_via is not None and getattr(w, "_fs_grad_via", None) is None:
            w._fs_grad_via = ctx.w_via
        cout, cin, r, s = w.shape
        if has_bias and r == 1 and s == 1 and stride == 1 and pad == 0 and hip.linear_bwd_weight_bias_ok(dy.numel() // cout, cin, cout):
            # a linear layer: the bias gradient (column sums of dy) rides in the weight-gradient launch, which reads dy anyway
            dw, db = _linear_param_grads(x, dy, w, ctx.bias_ref)
            return dx, dw, db, None, None, None, None
        tgt = _direct_grad_target(w)
        dw = conv2d_bwd_weight(x, dy, w.shape, stride, pad, out=tgt, accumulate=tgt is not None)
        if tgt is not None:
            dw = None
        db = colsum(dy, dy.shape[-1], into=_direct_grad_target(ctx.bias_ref)) if has_bias else None
        return dx, dw, db, None, None, None, None


# ----------------------------------------------------------------------------------------------
# HRNet fuse + final concat
# ----------------------------------------------------------------------------------------------
class HrFuse(Function):
    """out = relu(sum_t up(t)) over up to 4 NHWC terms (lower-resolution terms bilinearly up-sampled)."""

    @staticmethod
    def forward(ctx, Ho, Wo, *terms):
        n = len(terms)
        B, _, _, C = terms[0].shape
        out = torch.empty(B, Ho, Wo, C, device=terms[0].device, dtype=torch.float32)
        ptrs = (ctypes.c_void_p * n)(*[hip.ptr(t) for t in terms])
        th = (ctypes.c_int * n)(*[t.shape[1] for t in terms])
        tw = (ctypes.c_int * n)(*[t.shape[2] for t in terms])
        hip.call("fs_hr_fuse_fwd", ptrs, th, tw, n, hip.ptr(out), B, Ho, Wo, C, 1)
        ctx.save_for_backward(out)
        ctx.shapes = [tuple(t.shape) for t in terms]
        # terms that are the output of an activation-free conv + BatchNorm layer (the last ConvBn of every fuse path): their output gradient
        # IS this node's gradient (up-sampled back for the lower-resolution ones), so backward forms their BatchNorm-backward sums as it
        # produces that gradient (round 5; before, each of them ran its own reduction pass over it: 62 of the 91 left in an HRNet step)
        ctx.bns = [(bn if (bn is not None and bn[4] == ACT_NONE and bn[1] is None and tuple(bn[0].shape) == tuple(t.shape) and t.shape[-1] <= 1024) else None)
                   for t, bn in ((t, getattr(t, "_fs_bn", None)) for t in terms)] if FUSE_BN_BWD_SUMS else [None] * n
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        dout = dout.contiguous()
        g = torch.empty_like(out)
        B, Ho, Wo, C = out.shape
        same = [i for i, shp in enumerate(ctx.shapes) if ctx.needs_input_grad[2 + i] and shp[1] == Ho and shp[2] == Wo and ctx.bns[i] is not None][:3]
        if same:
            M = B * Ho * Wo
            nslab = hip.bn_bwd_slabs(M, C)
            slabs = [torch.empty(nslab * C * 2, device=out.device, dtype=torch.float32) for _ in same]
            arr = lambda xs: (ctypes.c_void_p * len(xs))(*[hip.ptr(x) for x in xs])      # noqa: E731
            hip.call("fs_relu_bwd_bnsum", hip.ptr(dout), hip.ptr(out), hip.ptr(g), M, C, len(same), arr([ctx.bns[i][0] for i in same]),
                     arr([ctx.bns[i][2] for i in same]), arr([ctx.bns[i][3] for i in same]), arr(slabs))
            for i, slab in zip(same, slabs):
                BN_SLABS[(g.data_ptr(), ctx.bns[i][0].data_ptr())] = (slab, nslab, g)
        else:
            hip.call("fs_relu_bwd", hip.ptr(dout), hip.ptr(out), hip.ptr(g), out.numel())
        grads = []
        for i, shp in enumerate(ctx.shapes):
            if not ctx.needs_input_grad[2 + i]:
                grads.append(None)
            elif shp[1] == Ho and shp[2] == Wo:
                grads.append(g)
            else:
                d = torch.empty(shp, device=out.device, dtype=torch.float32)
                bn = ctx.bns[i]
                if bn is not None and (Ho // shp[1]) % 2 == 0 and (Wo // shp[2]) % 2 == 0:
                    y, _, mean, invstd, _ = bn
                    nslab = hip.bn_bwd_slabs(B * shp[1] * shp[2], C)
                    slab = torch.empty(nslab * C * 2, device=out.device, dtype=torch.float32)
                    hip.call("fs_upsample_slice_bwd_bnsum", hip.ptr(g), B, Ho, Wo, C, 0, hip.ptr(d), shp[1], shp[2], C, hip.ptr(y), hip.ptr(mean),
                             hip.ptr(invstd), hip.ptr(slab))
                    BN_SLABS[(d.data_ptr(), y.data_ptr())] = (slab, nslab, d)
                else:
                    hip.call("fs_upsample_slice_bwd", hip.ptr(g), B, Ho, Wo, C, 0, hip.ptr(d), shp[1], shp[2], C)
                grads.append(d)
        return (None, None, *grads)


class UpsampleTo(Function):
    """F.interpolate(x, size=(Ho,Wo), mode='bilinear', align_corners=False) on NHWC (integer factors)."""

    @staticmethod
    def forward(ctx, x, Ho, Wo):
        B, h, w, C = x.shape
        out = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.float32)
        hip.call("fs_upsample_slice_fwd", hip.ptr(x), B, h, w, C, hip.ptr(out), Ho, Wo, C, 0)
        ctx.shape = (B, h, w, C, Ho, Wo)
        return out

    @staticmethod
    def backward(ctx, g):
        B, h, w, C, Ho, Wo = ctx.shape
        d = torch.empty(B, h, w, C, device=g.device, dtype=torch.float32)
        hip.call("fs_upsample_slice_bwd", hip.ptr(g.contiguous()), B, Ho, Wo, C, 0, hip.ptr(d), h, w, C)
        return d, None, None


class UpsampleConcat(Function):
    """cat([x0, up(x1), up(x2), up(x3)], channel) written straight into one NHWC buffer."""

    @staticmethod
    def forward(ctx, *xs):
        B, Ho, Wo, _ = xs[0].shape
        Ct = sum(t.shape[3] for t in xs)
        out = torch.empty(B, Ho, Wo, Ct, device=xs[0].device, dtype=torch.float32)
        off = 0
        for t in xs:
            hip.call("fs_upsample_slice_fwd", hip.ptr(t), B, t.shape[1], t.shape[2], t.shape[3], hip.ptr(out), Ho, Wo, Ct, off)
            off += t.shape[3]
        ctx.shapes = [tuple(t.shape) for t in xs]
        ctx.out_shape = (B, Ho, Wo, Ct)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B, Ho, Wo, Ct = ctx.out_shape
        grads, off = [], 0
        for shp in ctx.shapes:
            d = torch.empty(shp, device=g.device, dtype=torch.float32)
            hip.call("fs_upsample_slice_bwd", hip.ptr(g), B, Ho, Wo, Ct, off, hip.ptr(d), shp[1], shp[2], shp[3])
            grads.append(d)
            off += shp[3]
        return tuple(grads)


# ----------------------------------------------------------------------------------------------
# C1 tail
# ----------------------------------------------------------------------------------------------
class MaskHead(Function):
    """m = sigmoid(conv1x1(x) + b) - 0.5; x (B,H,W,C) -> m (B,H,W)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        B, H, W, C = x.shape
        m = torch.empty(B, H, W, device=x.device, dtype=torch.float32)
        hip.call("fs_mask_head_fwd", hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(m), B * H * W, C)
        ctx.save_for_backward(x, w, m)
        return m

    @staticmethod
    def backward(ctx, dm):
        x, w, m = ctx.saved_tensors
        dm = dm.contiguous()
        C = x.shape[-1]
        dx = torch.empty_like(x)
        dw = torch.empty_like(w)
        db = torch.empty(1, device=x.device, dtype=torch.float32)
        scratch = torch.empty(hip.query("fs_mask_head_bwd_scratch_floats", m.numel(), C), device=x.device, dtype=torch.float32)
        hip.call("fs_mask_head_bwd", hip.ptr(dm), hip.ptr(m), hip.ptr(x), hip.ptr(w), hip.ptr(dx), hip.ptr(dw), hip.ptr(db),
                 m.numel(), C, hip.ptr(scratch))
        return dx, dw, db


class MaxPool(Function):
    """nn.MaxPool2d(k, stride, pad) on NHWC."""

    @staticmethod
    def forward(ctx, x, k, stride, pad):
        B, H, W, C = x.shape
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        out = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.float32)
        arg = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.int32)
        hip.call("fs_maxpool_fwd", hip.ptr(x), hip.ptr(out), hip.ptr(arg), B, H, W, C, Ho, Wo, k, stride, pad)
        ctx.save_for_backward(arg)
        ctx.cfg = (B, H, W, C, Ho, Wo, k, stride, pad)
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        B, H, W, C, Ho, Wo, k, stride, pad = ctx.cfg
        dx = torch.empty(B, H, W, C, device=g.device, dtype=torch.float32)
        hip.call("fs_maxpool_bwd", hip.ptr(g.contiguous()), hip.ptr(arg), hip.ptr(dx), B, H, W, C, Ho, Wo, k, stride, pad)
        return dx, None, None, None


class Dropout(Function):
    """Stand-alone nn.Dropout(p) with the replayable hash mask (identity when p == 0)."""

    @staticmethod
    def forward(ctx, x, p, key):
        ctx.pk = (float(p), int(key))
        out = torch.empty_like(x)
        hip.call("fs_dropout", hip.ptr(x), hip.ptr(out), x.numel(), float(p), int(key))
        return out

    @staticmethod
    def backward(ctx, g):
        p, key = ctx.pk
        out = torch.empty_like(g)
        hip.call("fs_dropout", hip.ptr(g.contiguous()), hip.ptr(out), g.numel(), p, key)
        return out, None, None


class AvgPoolHW(Function):
    @staticmethod
    def forward(ctx, x):
        B, H, W, C = x.shape
        out = torch.empty(B, C, device=x.device, dtype=torch.float32)
        hip.call("fs_avgpool_fwd", hip.ptr(x), B, H * W, C, hip.ptr(out))
        ctx.shape = (B, H, W, C)
        return out

    @staticmethod
    def backward(ctx, g):
        B, H, W, C = ctx.shape
        dx = torch.empty(B, H, W, C, device=g.device, dtype=torch.float32)
        hip.call("fs_avgpool_bwd", hip.ptr(g.contiguous()), B, H * W, C, hip.ptr(dx))
        return dx


class PredAssemble(Function):
    """pred (B,K,H,W): channels < K-1 = class logits broadcast, channel K-1 = logit * mask."""

    @staticmethod
    def forward(ctx, cls, m):
        B, K = cls.shape
        _, H, W = m.shape
        pred = torch.empty(B, K, H, W, device=cls.device, dtype=torch.float32)
        hip.call("fs_pred_assemble_fwd", hip.ptr(cls), hip.ptr(m), hip.ptr(pred), B, K, H * W)
        ctx.save_for_backward(cls, m)
        return pred

    @staticmethod
    def backward(ctx, dpred):
        cls, m = ctx.saved_tensors
        B, K = cls.shape
        dcls = torch.empty_like(cls)
        dm = torch.empty_like(m)
        hip.call("fs_pred_assemble_bwd", hip.ptr(dpred.contiguous()), hip.ptr(cls), hip.ptr(m), hip.ptr(dcls), hip.ptr(dm), B, K,
                 m.shape[1] * m.shape[2])
        return dcls, dm


class SegLoss(Function):
    """(pred (B,K,H,W), gt (B,H,W) int64) -> 7 scalars {dice+focal, focal, dice, 4 accuracies};
    only element 0 carries a gradient."""

    @staticmethod
    def forward(ctx, pred, gt, gamma):
        B, K, H, W = pred.shape
        accum = torch.empty(B * ((H * W + 1023) // 1024) * (3 * K + 7), device=pred.device, dtype=torch.float64)
        out = torch.empty(7, device=pred.device, dtype=torch.float32)
        coef = torch.empty(2 * K, device=pred.device, dtype=torch.float32)
        _launch("fe_seg_loss_fwd", 4.0 * B * H * W * (K + 2), "fs_seg_loss_fwd", hip.ptr(pred), hip.ptr(gt), B, K, H * W, float(gamma), 1e-7, hip.ptr(accum), hip.ptr(out),
                hip.ptr(coef))
        ctx.save_for_backward(pred, gt, coef)
        ctx.gamma = float(gamma)
        return out

    @staticmethod
    def backward(ctx, gout):
        pred, gt, coef = ctx.saved_tensors
        B, K, H, W = pred.shape
        g0 = gout[0:1].contiguous()
        dpred = torch.empty_like(pred)
        _launch("fe_seg_loss_bwd", 4.0 * B * H * W * (2 * K + 2), "fs_seg_loss_bwd", hip.ptr(pred), hip.ptr(gt), hip.ptr(coef), hip.ptr(g0), hip.ptr(dpred), B, K, H * W, ctx.gamma)
        return dpred, None, None


# ----------------------------------------------------------------------------------------------
# foveation front-end
# ----------------------------------------------------------------------------------------------
def byte_frame_strides(shape, strides):
    """byte_frame_layout's rule as a pure function of a (B,3,H,W) shape and its element strides (sb, sc, sy, sx); strides of dimensions
    of size 1 are ignored.  ("planar",) for a contiguous tensor; ("hwc", sb, sy, sx) for interleaved bytes -- sc == 1, sx in {3, 4}, sy
    >= W * sx, and sb == 0 (every viewer sees the one frame), sb >= H * sy or B == 1; None for anything else.  In the hwc tuple the
    ignored strides are normalised: sb = 0 for B == 1, sy = W * sx for H == 1, sx = 3 for W == 1."""
    B, C, H, W = (int(v) for v in shape)
    sb, sc, sy, sx = (int(v) for v in strides)
    if C != 3 or min(B, H, W) < 1:
        return None
    if (W == 1 or sx == 1) and (H == 1 or sy == W) and (sc == H * W) and (B == 1 or sb == 3 * H * W):
        return ("planar",)
    if sc != 1:
        return None
    if W == 1:
        sx = 3
    if sx not in (3, 4):
        return None
    if H == 1:
        sy = W * sx
    if sy < W * sx:
        return None
    if B == 1:
        sb = 0
    if sb != 0 and sb < H * sy:
        return None
    return ("hwc", sb, sy, sx)


def byte_frame_layout(img):
    """How a uint8 frame (B,3,H,W) lies in memory, from its strides alone: ("planar",) when it is contiguous (the fs_*_u8 route);
    ("hwc", sb, sy, sx) when it is a view of interleaved bytes, the byte of channel c at (b, y, x) being byte b * sb + y * sy + x * sx + c
    from img.data_ptr() (the fs_*_hwc route: nothing is copied); None for anything else.  An hwc view is what a camera's or a decoder's
    (B,H,W,3) or (B,H,W,4) buffer is after permute(0, 3, 1, 2) (and [:, :3] for RGBA / RGBX, whose fourth byte is never used): tight or
    with padded rows, a crop of a larger buffer, x.contiguous(memory_format=torch.channels_last), or one frame expanded over the batch
    (sb == 0).  The channel order is the tensor's own.  The kernels read whole pixels, so the W * sx bytes of the last row must lie inside
    the tensor's storage (an RGBA view's last alpha byte: true of every view of a real (B,H,W,4) buffer); a view that ends short is None."""
    if not isinstance(img, torch.Tensor) or img.dim() != 4 or img.dtype != torch.uint8 or img.shape[1] != 3 or img.numel() == 0:
        return None
    if img.is_contiguous():
        return ("planar",)
    layout = byte_frame_strides(img.shape, img.stride())
    if layout is not None and layout[0] == "hwc":
        _, sb, sy, sx = layout
        if img.storage_offset() + (img.shape[0] - 1) * sb + (img.shape[2] - 1) * sy + img.shape[3] * sx > img.untyped_storage().nbytes():
            return None
    return layout


def _byte_frame(img, what="img"):
    """("planar",) or ("hwc", ...) of a uint8 frame the *_u8 functions take; ValueError for any other layout, before any launch."""
    layout = byte_frame_layout(img)
    if layout is None:
        raise ValueError(f"{what} must be a contiguous uint8 (B,3,H,W) or a view of interleaved (B,H,W,3) / (B,H,W,4) bytes "
                         f"(ops.byte_frame_layout), got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))} with strides "
                         f"{tuple(img.stride()) if isinstance(img, torch.Tensor) else None}; call .contiguous() on it")
    return layout


NV12_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}          # (Kr, Kb)
NV12_COEF_MAX = 32768


def nv12_csc(matrix, full_range=False):
    """The integer colour table (yo, yg, rv, gu, gv, bu) of an NV12 frame (include/fovealseg.h "frames as NV12"): rint(256 * real
    coefficient) from the matrix's (Kr, Kb); the luma gain is 255 / 219 and the chroma gain 255 / 224 for limited range (yo = 16), both 1
    for full range (yo = 0).  matrix: "bt601" or "bt709"."""
    if matrix not in NV12_MATRICES:
        raise ValueError(f"matrix must be one of {sorted(NV12_MATRICES)}, got {matrix!r}")
    kr, kb = NV12_MATRICES[matrix]
    kg = 1.0 - kr - kb
    ly, lc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    real = (ly, lc * 2 * (1 - kr), -lc * 2 * (1 - kb) * kb / kg, -lc * 2 * (1 - kr) * kr / kg, lc * 2 * (1 - kb))
    return (0 if full_range else 16,) + tuple(int(round(256.0 * v)) for v in real)


def _nv12_table(csc):
    try:
        t = tuple(operator.index(v) for v in csc)
    except TypeError:
        t = ()
    if len(t) != 6 or any(isinstance(v, bool) for v in csc):
        raise ValueError(f"csc must be six integers (yo, yg, rv, gu, gv, bu), got {csc!r}")
    if not 0 <= t[0] <= 255 or any(abs(v) > NV12_COEF_MAX for v in t[1:]):
        raise ValueError(f"csc wants 0 <= yo <= 255 and every coefficient in [-{NV12_COEF_MAX}, {NV12_COEF_MAX}], got {t}")
    return t


def nv12_frame_strides(y_shape, y_strides, uv_shape, uv_strides):
    """(sb, sy, ub, uy) of an NV12 frame from the shapes and strides of its two views alone, or None: y (B,H,W) with unit column stride
    and rows sy >= W apart, uv (B,ceil(H/2),ceil(W/2),2) with strides (ub, uy, 2, 1) and rows uy >= 2 * ceil(W/2) apart; images that do
    not overlap (sb >= H * sy, ub >= ceil(H/2) * uy) or are all one image (sb = ub = 0).  The strides of a dimension of one element are
    normalised: sb = ub = 0 for B == 1, sy = W for H == 1, uy = 2 * ceil(W/2) for one chroma row."""
    if len(y_shape) != 3 or len(uv_shape) != 4:
        return None
    B, H, W = (int(v) for v in y_shape)
    if min(B, H, W) < 1:
        return None
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    if tuple(int(v) for v in uv_shape) != (B, Hc, Wc, 2):
        return None
    sb, sy, sx = (int(v) for v in y_strides)
    ub, uy, ux, uc = (int(v) for v in uv_strides)
    if (W > 1 and sx != 1) or uc != 1 or (Wc > 1 and ux != 2):
        return None
    if H == 1:
        sy = W
    if Hc == 1:
        uy = 2 * Wc
    if B == 1:
        sb = ub = 0
    if sy < W or uy < 2 * Wc or sb < 0 or ub < 0:
        return None
    if not (sb == 0 and ub == 0) and (sb < H * sy or ub < Hc * uy):
        return None
    return sb, sy, ub, uy


class Nv12Frame:
    """An NV12 frame of B images of H x W pixels where a decoder or a camera left it (include/fovealseg.h "frames as NV12"; unpinned):
    y (B,H,W) uint8, the luma plane, a device tensor or view with unit column stride; uv (B,ceil(H/2),ceil(W/2),2) uint8, the interleaved
    chroma plane, a view with strides (ub, uy, 2, 1).  Two allocations, or two views of one surface (nv12_from_surface).  matrix: "bt601"
    or "bt709", with full_range -- it has no default: a silent wrong colour matrix is worse than a required keyword; csc: a table of the
    caller's own (yo, yg, rv, gu, gv, bu) instead (nv12_csc's rule; matrix is then only a label and may be None).

    predict*, evaluate*, GazeSession.step / render and the ops that take a uint8 frame take this object in its place, and give what they
    give on the planar uint8 frame nv12_to_rgb(frame), bit for bit; the frame is read where it lies and never written.  It shows
    shape == (B,3,H,W), dtype == torch.uint8, device and is_cuda as that frame would.  ValueError for any other dtypes, shapes or
    strides, views on different devices, bytes the kernels may read outside the tensors' storage, or a table out of range."""

    def __init__(self, y, uv, *, matrix, full_range=False, csc=None):
        if not isinstance(y, torch.Tensor) or not isinstance(uv, torch.Tensor) or y.dtype != torch.uint8 or uv.dtype != torch.uint8:
            raise ValueError(f"y and uv must be uint8 tensors, got {getattr(y, 'dtype', None)} and {getattr(uv, 'dtype', None)}")
        strides = nv12_frame_strides(y.shape, y.stride(), uv.shape, uv.stride()) if y.dim() == 3 and uv.dim() == 4 else None
        if strides is None:
            raise ValueError(f"y must be a non-empty (B,H,W) with unit column stride and uv (B,ceil(H/2),ceil(W/2),2) with strides (ub, uy, 2, 1), "
                             f"rows and images that do not overlap (or one image expanded over the batch in both), got {tuple(y.shape)} with "
                             f"strides {tuple(y.stride())} and {tuple(uv.shape)} with strides {tuple(uv.stride())}")
        if y.device != uv.device:
            raise ValueError(f"y and uv must be on one device, got {y.device} and {uv.device}")
        B, H, W = (int(v) for v in y.shape)
        sb, sy, ub, uy = strides
        if (y.storage_offset() + (B - 1) * sb + (H - 1) * sy + W > y.untyped_storage().nbytes()
                or uv.storage_offset() + (B - 1) * ub + ((H + 1) // 2 - 1) * uy + 2 * ((W + 1) // 2) > uv.untyped_storage().nbytes()):
            raise ValueError("y or uv ends short of the bytes its shape and strides describe")
        if csc is None:
            csc = nv12_csc(matrix, full_range)
        elif matrix is not None and matrix not in NV12_MATRICES:
            raise ValueError(f"matrix must be one of {sorted(NV12_MATRICES)} or None beside csc, got {matrix!r}")
        self.y, self.uv = y, uv
        self.matrix, self.full_range = matrix, bool(full_range)
        self.csc = _nv12_table(csc)
        self.strides = strides
        # what _frame_route and _frame_args hand to every call, made once: the planes stay where they are while the frame holds them
        self._tail = self.strides + self.csc
        self._args = (y.data_ptr(), uv.data_ptr()) + self._tail
        self.shape = torch.Size((B, 3, H, W))
        self.dtype = torch.uint8
        self.device = y.device
        self.is_cuda = y.is_cuda

    def dim(self):
        return 4

    def numel(self):
        return self.shape.numel()

    def like(self, y, uv):
        """The frame of other planes under this frame's colour table."""
        return Nv12Frame(y, uv, matrix=self.matrix, full_range=self.full_range, csc=self.csc)

    def route(self):
        """fs_nv12_frame_route of the frame: 1 the vector forms, 0 the one-pixel forms."""
        return int(hip.load().fs_nv12_frame_route(self.y.data_ptr(), self.uv.data_ptr(), *self.strides, int(self.shape[3])))


_FRAME_TYPES = (torch.Tensor, Nv12Frame)


def nv12_from_surface(buf, H, W, pitch, uv_offset, batch_stride=None, *, matrix, full_range=False, csc=None):
    """The Nv12Frame of one decoder surface: buf, a uint8 tensor of the surface's bytes (any shape; it is read flat and must be
    contiguous); B = its images.  Luma rows lie pitch apart from byte 0 of an image, chroma rows pitch apart from byte uv_offset (H *
    pitch for a tight surface; decoders that align the plane give their own); images batch_stride apart (None: one image, B = 1)."""
    if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or not buf.is_contiguous():
        raise ValueError(f"buf must be a contiguous uint8 tensor, got {getattr(buf, 'dtype', None)}")
    H, W, pitch, uv_offset = int(H), int(W), int(pitch), int(uv_offset)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    if min(H, W) < 1 or pitch < max(W, 2 * Wc) or uv_offset < H * pitch:
        raise ValueError(f"a surface of {H} x {W} pixels wants pitch >= {max(W, 2 * Wc)} and uv_offset >= H * pitch, got {pitch} and {uv_offset}")
    flat = buf.view(-1)
    per = uv_offset + (Hc - 1) * pitch + 2 * Wc
    if batch_stride is None:
        B, batch_stride = 1, per
    else:
        batch_stride = int(batch_stride)
        if batch_stride < uv_offset + Hc * pitch:
            raise ValueError(f"batch_stride must be at least uv_offset + ceil(H/2) * pitch = {uv_offset + Hc * pitch}, got {batch_stride}")
        B = (flat.numel() - per) // batch_stride + 1 if flat.numel() >= per else 0
    if flat.numel() < per or B < 1:
        raise ValueError(f"buf has {flat.numel()} bytes, one image of this surface needs {per}")
    y = flat.as_strided((B, H, W), (batch_stride, pitch, 1))
    uv = flat.as_strided((B, Hc, Wc, 2), (batch_stride, pitch, 2, 1), flat.storage_offset() + uv_offset)      # as_strided counts from the storage
    return Nv12Frame(y, uv, matrix=matrix, full_range=full_range, csc=csc)


def nv12_to_rgb(frame, out=None):
    """The RGB bytes of an NV12 frame (fs_nv12_to_rgb; no autograd; unpinned): out, a uint8 (B,3,H,W) tensor, contiguous or a view of
    interleaved (B,H,W,3) / (B,H,W,4) bytes (byte_frame_dest; RGBA gets alpha 255); None: a new contiguous one.  The planar result is
    the frame every other entry point is equal on.  Returns out."""
    if not isinstance(frame, Nv12Frame):
        raise ValueError(f"frame must be an ops.Nv12Frame, got {type(frame).__name__}")
    B, _, H, W = (int(v) for v in frame.shape)
    if out is None:
        out = torch.empty(B, 3, H, W, device=frame.device, dtype=torch.uint8)
    dest = byte_frame_dest(out, (B, 3, H, W))
    suffix, strides = _frame_route(frame)
    hip.call("fs_nv12_to_rgb", *_frame_args(frame, strides), *_dest_args(out, dest), B, H, W)
    return out


def _frame_route(img, what="img"):
    """Which of a pass's four entry points reads the frame img, and what follows the frame's pointer in its arguments: ("", ()) for fp32,
    ("_u8", ()) for contiguous bytes, ("_hwc", (sb, sy, sx)) for an hwc view, ("_nv12", (sb, sy, ub, uy, yo, yg, rv, gu, gv, bu)) for an
    Nv12Frame; ValueError for bytes in any other layout (_byte_frame).  A function of type, dtype, shape, strides and storage size
    alone: no device is asked."""
    if isinstance(img, Nv12Frame):
        return "_nv12", img._tail
    if img.dtype != torch.uint8:
        return "", ()
    layout = _byte_frame(img, what)
    return ("_u8", ()) if layout[0] == "planar" else ("_hwc", layout[1:])


def _frame_args(img, strides):
    """The frame's leading arguments of the entry point _frame_route chose: the device pointer and the strides of an hwc view (which is
    not contiguous, as hip.ptr asks of every other tensor), the two plane pointers, the strides and the table of an Nv12Frame."""
    if not strides:
        return (hip.ptr(img),)
    if not img.is_cuda:
        raise hip.HipLibraryError("fovealseg kernels need device tensors (got a CPU tensor); there is no CPU path")
    if isinstance(img, Nv12Frame):
        return img._args
    return (img.data_ptr(),) + strides


def byte_frame_select(img, sel):
    """img.index_select(0, sel) for an hwc view that stays one: the rows of the chosen frames are gathered from the underlying bytes (3 * H *
    W or 4 * H * W bytes a frame, never a planar copy) and viewed as (n,3,H,W) again.  With sb == 0 the n frames are the one frame.  An
    Nv12Frame stays one likewise: the chosen frames' luma and chroma rows are gathered as they lie, 1.5 bytes a pixel, no RGB copy."""
    if isinstance(img, Nv12Frame):
        B, _, H, W = (int(v) for v in img.shape)
        n = int(sel.shape[0])
        sb, sy, ub, uy = img.strides
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        if sb == 0 and ub == 0:
            return img.like(img.y[:1].expand(n, H, W), img.uv[:1].expand(n, Hc, Wc, 2))
        return img.like(img.y.index_select(0, sel), img.uv.index_select(0, sel))
    layout = byte_frame_layout(img)
    if layout is None or layout[0] != "hwc":
        return img.index_select(0, sel)
    _, sb, sy, sx = layout
    B, _, H, W = (int(v) for v in img.shape)
    n = int(sel.shape[0])
    if sb == 0:
        return img[:1].expand(n, 3, H, W)
    rows = img.as_strided((B, H, W * sx), (sb, sy, 1)).index_select(0, sel)
    return rows.view(n, H, W, sx).permute(0, 3, 1, 2)[:, :3]


def gaze_lowres(x, focus, hs, ws):
    B, C, H, W = x.shape
    assert C == 3
    out = torch.empty(B, hs, ws, 5, device=x.device, dtype=torch.float32)
    suffix, strides = _frame_route(x, "x")
    # a frame of bytes, planar or read where it lies interleaved: four one-byte taps a channel, 12 bytes read and 20 written a point
    traffic = (12 + 20) if suffix else 4 * (4 * 3 + 5)
    _launch("fe_gaze_lowres" + suffix, 1.0 * B * hs * ws * traffic, f"fs_gaze_lowres{suffix}_fwd", *_frame_args(x, strides), hip.ptr(focus),
            hip.ptr(out), B, H, W, hs, ws)
    return out


class CompressSoftmax(Function):
    """xs = softmax_HW(conv1x1(relu(s)) + b): s (B,H,W,C) -> xs (B,1,H,W)."""

    @staticmethod
    def forward(ctx, s, w, bias):
        B, H, W, C = s.shape
        xs = torch.empty(B, 1, H, W, device=s.device, dtype=torch.float32)
        hip.call("fs_compress_softmax_fwd", hip.ptr(s), hip.ptr(w), hip.ptr(bias), hip.ptr(xs), B, H * W, C)
        ctx.save_for_backward(s, w, xs)
        return xs

    @staticmethod
    def backward(ctx, g):
        s, w, xs = ctx.saved_tensors
        B, H, W, C = s.shape
        ds = torch.empty_like(s)
        dw = torch.empty_like(w)
        db = torch.empty(1, device=s.device, dtype=torch.float32)
        scratch = torch.empty(hip.query("fs_compress_softmax_bwd_scratch_floats", B, C), device=s.device, dtype=torch.float32)
        hip.call("fs_compress_softmax_bwd", hip.ptr(g.contiguous()), hip.ptr(xs), hip.ptr(s), hip.ptr(w), hip.ptr(ds), hip.ptr(dw),
                 hip.ptr(db), B, H * W, C, hip.ptr(scratch))
        return ds, dw, db


class Compress(Function):
    """CompressNet.forward on its own (models/models.py:360-372): s (B,H,W,C) -> logits (B,1,H,W) = conv1x1(relu(s)) + b."""

    @staticmethod
    def forward(ctx, s, w, bias):
        B, H, W, C = s.shape
        out = torch.empty(B, 1, H, W, device=s.device, dtype=torch.float32)
        hip.call("fs_compress_fwd", hip.ptr(s), hip.ptr(w), hip.ptr(bias), hip.ptr(out), B, H * W, C)
        ctx.save_for_backward(s, w)
        return out

    @staticmethod
    def backward(ctx, g):
        s, w = ctx.saved_tensors
        B, H, W, C = s.shape
        ds = torch.empty_like(s)
        dw = torch.empty_like(w)
        db = torch.empty(1, device=s.device, dtype=torch.float32)
        scratch = torch.empty(B * (C + 1), device=s.device, dtype=torch.float32)
        hip.call("fs_compress_bwd", hip.ptr(g.contiguous()), hip.ptr(s), hip.ptr(w), hip.ptr(ds), hip.ptr(dw), hip.ptr(db), B, H * W, C,
                 hip.ptr(scratch))
        return ds, dw, db


def area_pool(y, hs, ws):
    B, C, H, W = y.shape
    assert C == 1
    out = torch.empty(B, 1, hs, ws, device=y.device, dtype=torch.float32)
    _launch("fe_area_pool", 4.0 * B * (H * W + hs * ws), "fs_area_pool_fwd", hip.ptr(y), hip.ptr(out), B, H, W, hs, ws)
    return out


class EdgeLoss(Function):
    @staticmethod
    def forward(ctx, xs, target, coef):
        loss = torch.empty(1, device=xs.device, dtype=torch.float32)
        # 6 statistics kept for the backward + the per-workgroup partial records of both passes
        stats = torch.empty(hip.query("fs_edge_loss_stats_floats", xs.numel()), device=xs.device, dtype=torch.float32)
        hip.call("fs_edge_loss_fwd", hip.ptr(xs), hip.ptr(target), xs.numel(), float(coef), hip.ptr(loss), hip.ptr(stats))
        ctx.save_for_backward(xs, target, stats)
        ctx.coef = float(coef)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        xs, target, stats = ctx.saved_tensors
        dxs = torch.empty_like(xs)
        hip.call("fs_edge_loss_bwd", hip.ptr(xs), hip.ptr(target), xs.numel(), ctx.coef, hip.ptr(g.reshape(1).contiguous()),
                 hip.ptr(stats), hip.ptr(dxs))
        return dxs, None, None


PAD_MODES = {"replication": 0, "reflect": 1, "zero": 2}      # TRAIN.def_saliency_pad_mode (models/models.py:819-825)


class GaussGrid(Function):
    """xs (B,1,hs,ws) -> grid (B,hs,ws,2); g1d = separable Gaussian taps (float64, device); pad_mode = PAD_MODES[...] (the padded map
    is never written: the kernels read the source pixel a padded position copies)."""

    @staticmethod
    def forward(ctx, xs, g1d, pad, pad_mode=0):
        B, _, hs, ws = xs.shape
        grid = torch.empty(B, hs, ws, 2, device=xs.device, dtype=torch.float32)
        if pad_mode == 0:
            _launch("fe_gauss_grid_fwd", 4.0 * B * hs * ws * 3, "fs_gauss_grid_fwd", hip.ptr(xs), hip.ptr(g1d), hip.ptr(grid), B, hs, ws, pad)
        else:
            _launch("fe_gauss_grid_fwd", 4.0 * B * hs * ws * 3, "fs_gauss_grid_fwd_mode", hip.ptr(xs), hip.ptr(g1d), hip.ptr(grid), B, hs, ws, pad,
                    pad_mode)
        ctx.save_for_backward(xs, g1d)
        ctx.pad, ctx.pad_mode = pad, pad_mode
        return grid

    @staticmethod
    def backward(ctx, dgrid):
        xs, g1d = ctx.saved_tensors
        B, _, hs, ws = xs.shape
        dxs = torch.empty_like(xs)
        scratch = torch.empty(hip.query("fs_gauss_grid_bwd_scratch_floats", B, hs, ws), device=xs.device, dtype=torch.float32)
        if ctx.pad_mode == 0:
            _launch("fe_gauss_grid_bwd", 4.0 * B * hs * ws * 4, "fs_gauss_grid_bwd", hip.ptr(xs), hip.ptr(g1d), hip.ptr(dgrid.contiguous()), hip.ptr(dxs),
                    B, hs, ws, ctx.pad, hip.ptr(scratch))
        else:
            _launch("fe_gauss_grid_bwd", 4.0 * B * hs * ws * 4, "fs_gauss_grid_bwd_mode", hip.ptr(xs), hip.ptr(g1d), hip.ptr(dgrid.contiguous()),
                    hip.ptr(dxs), B, hs, ws, ctx.pad, ctx.pad_mode, hip.ptr(scratch))
        return dxs, None, None, None


class GridUpsample(Function):
    """nn.Upsample(size=(H,W), mode='bilinear') of the grid (B,h,w,2) -> (B,H,W,2) (models/models.py:621-631)."""

    @staticmethod
    def forward(ctx, grid, H, W):
        B, h, w, _ = grid.shape
        out = torch.empty(B, H, W, 2, device=grid.device, dtype=torch.float32)
        hip.call("fs_grid_upsample_fwd", hip.ptr(grid.contiguous()), hip.ptr(out), B, h, w, H, W)
        ctx.cfg = (B, h, w, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        B, h, w, H, W = ctx.cfg
        d = torch.empty(B, h, w, 2, device=g.device, dtype=torch.float32)
        hip.call("fs_grid_upsample_bwd", hip.ptr(g.contiguous()), hip.ptr(d), B, h, w, H, W)
        return d, None, None


class GridSample(Function):
    """x (B,C,H,W) NCHW, grid (B,h,w,2) -> (B,h,w,C) NHWC; gradient w.r.t. the grid (and, when asked,
    w.r.t. x by scatter-add)."""

    @staticmethod
    def forward(ctx, x, grid):
        B, C, H, W = x.shape
        _, h, w, _ = grid.shape
        out = torch.empty(B, h, w, C, device=x.device, dtype=torch.float32)
        _launch("fe_grid_sample_fwd", 4.0 * B * h * w * (4 * C + 2 + C), "fs_grid_sample_fwd", hip.ptr(x), hip.ptr(grid), hip.ptr(out), B, C, H, W, h, w, 1)
        ctx.save_for_backward(x, grid)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, grid = ctx.saved_tensors
        B, C, H, W = x.shape
        _, h, w, _ = grid.shape
        gout = gout.contiguous()
        dx = dgrid = None
        if ctx.needs_input_grad[1]:
            dgrid = torch.empty_like(grid)
            _launch("fe_grid_sample_bwd_grid", 4.0 * B * h * w * (4 * C + C + 2 + 2), "fs_grid_sample_bwd_grid", hip.ptr(gout), hip.ptr(x), hip.ptr(grid), hip.ptr(dgrid), B, C, H, W, h, w, 1)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            hip.call("fs_grid_sample_bwd_input", hip.ptr(gout), hip.ptr(grid), hip.ptr(dx), B, C, H, W, h, w, 1)
        return dx, dgrid


def grid_sample_u8(x, grid):
    """GridSample's forward on a frame of bytes (fs_grid_sample_u8_fwd; no autograd): x (B,C,H,W) uint8 with the pixel value byte / 255,
    grid (B,h,w,2) fp32 -> (B,h,w,C) fp32 NHWC, equal to GridSample.apply(x.float() / 255, grid) bit for bit."""
    if not isinstance(x, _FRAME_TYPES) or x.dim() != 4 or x.numel() == 0 or x.dtype != torch.uint8:
        raise ValueError(f"x must be a non-empty uint8 (B,C,H,W), got {getattr(x, 'dtype', None)} {tuple(getattr(x, 'shape', ()))}")
    B, C, H, W = (int(v) for v in x.shape)
    if grid.dim() != 4 or grid.shape[0] != B or grid.shape[3] != 2 or grid.numel() == 0 or grid.dtype != torch.float32:
        raise ValueError(f"grid must be a non-empty fp32 ({B},h,w,2), got {grid.dtype} {tuple(grid.shape)}")
    h, w = int(grid.shape[1]), int(grid.shape[2])
    out = torch.empty(B, h, w, C, device=x.device, dtype=torch.float32)
    traffic = 1.0 * B * h * w * (4 * C + 8 + 4 * C)
    if isinstance(x, Nv12Frame):                        # three channels, each tap converted as it is read
        _, strides = _frame_route(x, "x")
        _launch("fe_grid_sample_nv12_fwd", traffic, "fs_grid_sample_nv12_fwd", *_frame_args(x, strides), hip.ptr(grid), hip.ptr(out), B, H, W, h, w, 1)
    elif x.is_contiguous():                             # any C
        _launch("fe_grid_sample_u8_fwd", traffic, "fs_grid_sample_u8_fwd", hip.ptr(x), hip.ptr(grid), hip.ptr(out), B, C, H, W, h, w, 1)
    else:                                               # an interleaved frame (three channels), read where it lies: one address a tap
        _, strides = _frame_route(x, "x")
        _launch("fe_grid_sample_hwc_fwd", traffic, "fs_grid_sample_hwc_fwd", *_frame_args(x, strides), hip.ptr(grid), hip.ptr(out), B, H, W, h, w, 1)
    return out


def grid_sample_label(y, grid, return_float=False):
    B, C, H, W = y.shape
    assert C == 1
    _, h, w, _ = grid.shape
    label = torch.empty(B, h, w, device=y.device, dtype=torch.int64)
    ys = torch.empty(B, h, w, device=y.device, dtype=torch.float32) if return_float else None
    _launch("fe_grid_sample_label", 4.0 * B * h * w * (4 + 2 + 2), "fs_grid_sample_label", hip.ptr(y), hip.ptr(grid), hip.ptr(label), hip.ptr(ys), B, H, W, h, w)
    return (label, ys) if return_float else label


def inverse_index_maps(grid, H, W):
    n = grid.numel() // 2
    u = torch.empty(grid.shape[:-1], device=grid.device, dtype=torch.int64)
    v = torch.empty_like(u)
    hip.call("fs_inverse_index_maps", hip.ptr(grid), hip.ptr(u), hip.ptr(v), n, H, W)
    return u, v


def inverse_grid(grid, Hs, Ws):
    """models/models.py:639-655: (owner (B,Hs,Ws) int32 with -1 in holes, grid_inv (B,Hs,Ws,2) with 0 in holes)."""
    B, h, w, _ = grid.shape
    owner = torch.empty(B, Hs, Ws, device=grid.device, dtype=torch.int32)
    inv = torch.empty(B, Hs, Ws, 2, device=grid.device, dtype=torch.float32)
    hip.call("fs_inverse_grid", hip.ptr(grid.contiguous()), hip.ptr(owner), hip.ptr(inv), B, h, w, Hs, Ws)
    return owner, inv


def unwarp_nearest(pred, grid, Hs, Ws):
    """Full-resolution prediction from the foveated one (no autograd): pred (B,C,h,w) is sampled through the inverse grid
    (F.grid_sample(pred, grid_inv), models/models.py:933) and the never-claimed pixels take their nearest claimed
    neighbour (rev_deform_interp='nearest').  Returns (pred_full (B,C,Hs,Ws), hole mask (B,Hs,Ws) bool)."""
    B, C, h, w = pred.shape
    owner, inv = inverse_grid(grid, Hs, Ws)
    out = torch.empty(B, C, Hs, Ws, device=pred.device, dtype=torch.float32)
    hip.call("fs_grid_sample_fwd", hip.ptr(pred.contiguous()), hip.ptr(inv), hip.ptr(out), B, C, h, w, Hs, Ws, 0)
    scratch = torch.empty(2 * B * Hs * Ws, device=pred.device, dtype=torch.int32)
    hip.call("fs_fill_nearest", hip.ptr(out), hip.ptr(owner), hip.ptr(scratch), B, C, Hs, Ws)
    return out, owner < 0


def unwarp_labels(cls, m, grid, Hs, Ws):
    """Full-resolution class map of the C1 head (no autograd): bit for bit
    `unwarp_nearest(PredAssemble.apply(cls, m), grid, Hs, Ws)[0].argmax(1)`, without the (B,K,Hs,Ws) prediction -- the argmax is
    taken once per grid point and gathered through the owner map (fs_unwarp_labels).  cls (B,K), m (B,h,w) at the grid's
    resolution, grid (B,h,w,2).  Returns (labels (B,Hs,Ws) int64, hole mask (B,Hs,Ws) bool)."""
    B, K = cls.shape
    _, h, w, _ = grid.shape
    if tuple(m.shape) != (B, h, w):
        raise ValueError(f"m {tuple(m.shape)} must be (B, h, w) = {(B, h, w)}: the mask at the grid's resolution")
    labels = torch.empty(B, Hs, Ws, device=cls.device, dtype=torch.int64)
    hole = torch.empty(B, Hs, Ws, device=cls.device, dtype=torch.bool)
    scratch = torch.empty(hip.query("fs_unwarp_labels_scratch_ints", B, h, w, Hs, Ws), device=cls.device, dtype=torch.int32)
    hip.call("fs_unwarp_labels", hip.ptr(cls.contiguous()), hip.ptr(m.contiguous()), hip.ptr(grid.contiguous()), hip.ptr(labels),
             hip.ptr(hole), hip.ptr(scratch), B, K, h, w, Hs, Ws)
    return labels, hole


def _max_runs(max_runs, Ws):
    """The capacity of a run-length code: any int >= 1; None = 8 * Ws + 1, which holds every mask whose columns each cross its outline
    at most eight times (a blob entered and left four times by a column) -- 32 KB of int32 per 1024-wide image."""
    if max_runs is None:
        return 8 * int(Ws) + 1
    if isinstance(max_runs, bool) or int(max_runs) != max_runs or int(max_runs) < 1:
        raise ValueError(f"max_runs must be an integer >= 1, got {max_runs!r}")
    return int(max_runs)


def mask_bits(mask):
    """A mask as bit words (fs_mask_bits; no autograd): mask (B,Hs,Ws) or (Hs,Ws), bool or uint8 (non-zero = set), on the device.
    Returns bits (B,Hs,P) int32, P = ceil(Ws / 32): bit j of word i of row y is pixel x = 32 i + j, the bits at x >= Ws are 0."""
    if mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3 or mask.numel() == 0:
        raise ValueError(f"mask {tuple(mask.shape)} must be a non-empty (B, Hs, Ws)")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"the mask must be bool or uint8, got {mask.dtype}")
    B, Hs, Ws = (int(v) for v in mask.shape)
    bits = torch.empty(B, Hs, (Ws + 31) // 32, device=mask.device, dtype=torch.int32)
    hip.call("fs_mask_bits", hip.ptr(mask.contiguous()), hip.ptr(bits), B, Hs, Ws)
    return bits


def _bits_arg(mask_or_bits, Ws):
    """(bits (B,Hs,P) int32, Ws) of a mask argument as mask_rle / mask_component take it; bits is None for a mask still to be packed."""
    if not isinstance(mask_or_bits, torch.Tensor):
        raise ValueError("the mask must be a tensor: bool / uint8 (B,Hs,Ws) or (Hs,Ws), or int32 bit words with Ws")
    if mask_or_bits.dtype == torch.int32:
        bits = mask_or_bits
        if bits.dim() != 3 or bits.numel() == 0 or Ws is None or int(Ws) < 1 or bits.shape[2] != (int(Ws) + 31) // 32:
            raise ValueError(f"bit words {tuple(bits.shape)} must be a non-empty (B, Hs, ceil(Ws / 32)) with Ws given, got Ws = {Ws!r}")
        return bits, int(Ws)
    if mask_or_bits.dtype not in (torch.bool, torch.uint8) or mask_or_bits.dim() not in (2, 3) or mask_or_bits.numel() == 0:
        raise ValueError(f"the mask must be a non-empty bool / uint8 (B,Hs,Ws) or (Hs,Ws), got {mask_or_bits.dtype} {tuple(mask_or_bits.shape)}")
    if Ws is not None and int(Ws) != mask_or_bits.shape[-1]:
        raise ValueError(f"Ws = {Ws!r} differs from the mask's width {mask_or_bits.shape[-1]}")
    return None, int(mask_or_bits.shape[-1])


def _mask_words(mask_or_bits, Ws):
    """_bits_arg with the mask packed: (bits (B,Hs,P) int32, Ws)."""
    bits, Ws = _bits_arg(mask_or_bits, Ws)
    return (mask_bits(mask_or_bits) if bits is None else bits), Ws


def mask_rle(mask_or_bits, Ws=None, max_runs=None):
    """Area, box and uncompressed COCO run-length code of any mask, exact and on the device (fs_mask_rle; no autograd).  The argument
    is a bool / uint8 mask (B,Hs,Ws) or (Hs,Ws), or int32 bit words (B,Hs,ceil(Ws/32)) as mask_bits returns them together with Ws.
    Returns (stats (B,6) int64 = area, x0, y0, bw, bh, n_runs; counts (B,max_runs) int32).  [x0, y0, bw, bh] is the COCO box of the set
    pixels, all 0 for an empty mask.  counts is the code of the mask read column-major (p = x * Hs + y): the run of zeros before the
    first set pixel (0 when pixel (0,0) is set), then alternating run lengths, runs continuing from the bottom of a column into the
    top of the next; an empty mask is [Hs * Ws], a full one [0, Hs * Ws].  n_runs is always the true length of the code; the first
    min(n_runs, max_runs) entries of counts are its, the rest is 0, and n_runs > max_runs tells that the code was cut.  max_runs
    defaults to 8 * Ws + 1 (see _max_runs).  The format is restated from its published definition (pycocotools' uncompressed RLE)."""
    bits, Ws = _mask_words(mask_or_bits, Ws)
    B, Hs = int(bits.shape[0]), int(bits.shape[1])
    cap = _max_runs(max_runs, Ws)
    stats = torch.empty(B, 6, device=bits.device, dtype=torch.int64)
    counts = torch.empty(B, cap, device=bits.device, dtype=torch.int32)
    scratch = torch.empty(hip.query("fs_mask_rle_scratch_ints", B, Hs, Ws), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_rle", hip.ptr(bits.contiguous()), hip.ptr(stats), hip.ptr(counts), hip.ptr(scratch), B, Hs, Ws, cap)
    return stats, counts


COMPONENT_OFF2 = 2 ** 62                            # a squared distance no pixel reaches: snap_px = None


def _component_args(component, snap_px):
    """(conn, snap2) of mask_component / unwarp_instances(component=...): connectivity 4 or 8; snap_px None (no limit) or a finite number
    of pixels >= 0, snap2 = floor(snap_px ** 2)."""
    if isinstance(component, bool) or component not in (4, 8):
        raise ValueError(f"the connectivity must be 4 or 8, got {component!r}")
    if snap_px is None:
        return int(component), COMPONENT_OFF2
    px = float(snap_px)
    if not (px >= 0.0) or math.isinf(px):
        raise ValueError(f"snap_px must be a finite number of pixels >= 0, got {snap_px!r}")
    return int(component), COMPONENT_OFF2 if px >= 2.0 ** 31 else int(math.floor(px * px))     # 2^31 squared is 2^62: no overflow in px * px


def _focus_arg(focus, B, dev):
    if not isinstance(focus, torch.Tensor) or tuple(focus.shape) != (B, 2):
        raise ValueError(f"focus must be (B, 2) = ({B}, 2), got {tuple(getattr(focus, 'shape', ()))}")
    return focus.to(device=dev, dtype=torch.float32).contiguous()


def mask_component(mask_or_bits, focus, Ws=None, connectivity=8, snap_px=None):
    """The connected component of a mask under the gaze, on the device and on bit words (fs_mask_component; no autograd; unpinned:
    the reference has no counterpart).  The mask as mask_rle takes it: bool / uint8 (B,Hs,Ws) or (Hs,Ws), or int32 bit words
    (B,Hs,ceil(Ws/32)) together with Ws.  focus (B,2) normalised (row, col), turned into a gaze pixel as gate_decide does.  The seed is
    the gaze pixel where it is set, else the nearest set pixel (ties: the smaller row-major index), unless it lies more than snap_px
    pixels away (None: any distance; snap2 = floor(snap_px ** 2) against the squared distance).  connectivity 4 or 8.  Returns
    (bits_c (B,Hs,ceil(Ws/32)) int32, the component's words, all 0 where there is none; comp (B,4) int64 = (seed_y, seed_x, d2, area_all),
    (-1, -1, -1, area_all) where there is none; area_all counts the input's set pixels).  mask_rle(bits_c, Ws) gives its record."""
    conn, snap2 = _component_args(connectivity, snap_px)
    bits, Ws = _mask_words(mask_or_bits, Ws)
    B, Hs = int(bits.shape[0]), int(bits.shape[1])
    f = _focus_arg(focus, B, bits.device)
    out = torch.empty_like(bits, memory_format=torch.contiguous_format)
    comp = torch.empty(B, 4, device=bits.device, dtype=torch.int64)
    scratch = torch.empty(hip.query("fs_mask_component_scratch_ints", B, Hs, Ws), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_component", hip.ptr(bits.contiguous()), hip.ptr(f), hip.ptr(out), hip.ptr(comp), hip.ptr(scratch), B, Hs, Ws, conn, snap2)
    return out, comp


def boundary_dilation(Hs, Ws, ratio=0.02):
    """The dilation of Boundary IoU in pixels (Cheng et al., CVPR 2021, restated: unpinned): d = max(1, int(round(ratio *
    math.sqrt(Hs * Hs + Ws * Ws)))) in Python floats, ratio a finite float > 0 -- 0.02 of the image diagonal, 29 at 1024 x 1024."""
    if isinstance(Hs, bool) or isinstance(Ws, bool) or int(Hs) != Hs or int(Ws) != Ws or int(Hs) < 1 or int(Ws) < 1:
        raise ValueError(f"the size must be two integers >= 1, got {(Hs, Ws)!r}")
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not (float(ratio) > 0.0) or math.isinf(float(ratio)):
        raise ValueError(f"the boundary ratio must be a finite number > 0, got {ratio!r}")
    Hs, Ws = int(Hs), int(Ws)
    return max(1, int(round(float(ratio) * math.sqrt(Hs * Hs + Ws * Ws))))


MORPH_MAX_D = 2047                                  # fs_mask_erode's cap: a diagonal of 100 000 pixels at the default ratio


def _morph_d(d):
    if isinstance(d, bool) or not isinstance(d, int) or d < 1 or d > MORPH_MAX_D:
        raise ValueError(f"d must be an int 1 .. {MORPH_MAX_D}, got {d!r}")
    return d


def mask_erode(mask_or_bits, d, Ws=None):
    """Erosion of a mask by a (2d+1) x (2d+1) square, on the device and on bit words (fs_mask_erode; no autograd; unpinned: restated
    from the published definition of Boundary IoU).  The mask as mask_rle takes it: bool / uint8 (B,Hs,Ws) or (Hs,Ws), or int32 bit
    words (B,Hs,ceil(Ws/32)) together with Ws; d an int >= 1 (and <= 2047), not a bool.  Returns bits (B,Hs,ceil(Ws/32)) int32: pixel
    (y,x) is set iff every pixel of the square centred on it is set, every pixel outside the image counting as unset -- scipy's
    binary_erosion(m, ones((3,3)), iterations=d, border_value=0); all 0 where 2d+1 exceeds a side."""
    d = _morph_d(d)
    bits, Ws = _mask_words(mask_or_bits, Ws)
    B, Hs = int(bits.shape[0]), int(bits.shape[1])
    out = torch.empty_like(bits, memory_format=torch.contiguous_format)
    scratch = torch.empty(max(1, hip.query("fs_mask_erode_scratch_ints", B, Hs, Ws, d)), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_erode", hip.ptr(bits.contiguous()), hip.ptr(out), hip.ptr(scratch), B, Hs, Ws, d)
    return out


def mask_boundary(mask_or_bits, d, Ws=None):
    """The boundary band of Boundary IoU as bit words: m & ~mask_erode(m, d), the set pixels within d of an unset pixel or of the
    image's outside (chessboard distance); the mask itself where 2d+1 exceeds a side.  Arguments as mask_erode's; the bits at
    x >= Ws of the result are 0."""
    d = _morph_d(d)
    bits, Ws = _mask_words(mask_or_bits, Ws)
    er = mask_erode(bits, d, Ws)
    band = bits & ~er
    if Ws & 31:
        band[:, :, -1] &= (1 << (Ws & 31)) - 1                      # the input's padding bits are no pixels
    return band


def mask_pair_counts(a, b, d, Ws=None):
    """The counters of mask IoU and Boundary IoU of a prediction a and a label b (fs_mask_pair_counts; no autograd; unpinned).  a and
    b as mask_erode takes a mask, of one shape and kind; d as there.  Returns pair (B,6) int64 = (|a & b|, |a|, |b|, |band(a) &
    band(b)|, |band(a)|, |band(b)|), band = mask_boundary's; both erosions and the counts are taken on the device without a host
    read, on nothing wider than a bit a pixel.  pair_scores makes the two measures."""
    d = _morph_d(d)
    abits, Wa = _bits_arg(a, Ws)
    bbits, Wb = _bits_arg(b, Ws)
    if (abits is None) != (bbits is None) or tuple(a.shape[-2:]) != tuple(b.shape[-2:]) or Wa != Wb or a.device != b.device:
        raise ValueError(f"the two masks must be of one kind, size and device, got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")
    if abits is None:
        if (a.dim() == 3 and b.dim() == 3 and a.shape[0] != b.shape[0]) or a.dim() != b.dim():
            raise ValueError(f"the two masks must have one batch size, got {tuple(a.shape)} and {tuple(b.shape)}")
        abits, bbits = mask_bits(a), mask_bits(b)
    elif a.shape[0] != b.shape[0]:
        raise ValueError(f"the two masks must have one batch size, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, Hs = int(abits.shape[0]), int(abits.shape[1])
    pair = torch.empty(B, 6, device=abits.device, dtype=torch.int64)
    scratch = torch.empty(max(1, hip.query("fs_mask_pair_scratch_ints", B, Hs, Wa, d)), device=abits.device, dtype=torch.int32)
    hip.call("fs_mask_pair_counts", hip.ptr(abits.contiguous()), hip.ptr(bbits.contiguous()), hip.ptr(pair), hip.ptr(scratch), B, Hs, Wa, d)
    return pair


def pair_scores(pair):
    """(iou, biou), two fp64 tensors (B,), from mask_pair_counts' counters: n / (a + b - n) per triple, 0 where the union is 0."""
    if pair.dim() != 2 or pair.shape[1] != 6:
        raise ValueError(f"pair must be (B, 6), got {tuple(pair.shape)}")
    p = pair.to(torch.int64)
    out = []
    for o in (0, 3):
        n, u = p[:, o], p[:, o + 1] + p[:, o + 2] - p[:, o]
        out.append(torch.where(u > 0, n.double() / u.clamp(min=1).double(), torch.zeros_like(n, dtype=torch.float64)))
    return out[0], out[1]


def head_fg_q(cls, m):
    """The C1 head's foreground probability per grid point as an integer table (fs_head_fg_q; no autograd; unpinned: the reference
    has no counterpart).  cls (B,K), m (B,h,w).  Returns q (B, h*w+1) int32 = rint(P * 2^24): P is the softmax mass of the classes
    below K-1 among the K fp32 values `unwarp_nearest(PredAssemble(cls, m), ...)` carries from grid point p (entry h*w: from the sample at
    (0,0), which feeds an image without a claimed pixel), evaluated in fp64 with the maximum subtracted; 0 where P is NaN."""
    B, K = cls.shape
    if m.dim() != 3 or m.shape[0] != B:
        raise ValueError(f"m {tuple(m.shape)} must be (B, h, w) with B = {B}")
    h, w = int(m.shape[1]), int(m.shape[2])
    q = torch.empty(B, h * w + 1, device=cls.device, dtype=torch.int32)
    hip.call("fs_head_fg_q", hip.ptr(cls.contiguous()), hip.ptr(m.contiguous()), hip.ptr(q), B, K, h, w)
    return q


def unwarp_instances(cls, m, grid, Hs, Ws, max_runs=None, return_bits=False, score=False, component=None, focus=None, snap_px=None):
    """The gazed instance of the C1 head as a record instead of a class map (fs_unwarp_instances; no autograd).  Arguments and checks
    are unwarp_labels'.  The mask is `unwarp_labels(cls, m, grid, Hs, Ws)[0] != K - 1` bit for bit; no (B,Hs,Ws) tensor wider than its
    bit words is allocated.  Returns (cat, stats, counts[, bits]): cat (B,) int64 = torch.argmax(cls[:, :K-1], 1), the head's
    classification (first maximum, NaN maximal); stats (B,6) int64 and counts (B,max_runs) int32 are mask_rle's of the mask; bits
    (B,Hs,ceil(Ws/32)) int32 are mask_bits' of it.  cat is the label of every set pixel except where the bilinear sample of the constant
    class planes ties two classes by rounding or has no in-bounds weight (a grid point on the outer border).  max_runs: any int >= 1,
    default 8 * Ws + 1 -- room for a mask every column of which crosses its outline at most eight times, 32 KB per 1024-wide image;
    n_runs = stats[:, 5] > max_runs tells a cut code.  instances_to_coco makes the result records.

    score=True (fs_unwarp_instances_scored; unpinned) appends conf (B,3) fp32 = (score, cls_prob, mask_prob) and qsum (B,) int64 behind
    everything else: qsum is the sum of head_fg_q(cls, m)[b, feeding point] over the set pixels, added in the same gather; mask_prob =
    qsum / (area * 2^24), 0 for an empty mask; cls_prob = softmax(cls[b, :K-1])[cat[b]] in fp64, NaN where that row holds a NaN; score
    = their product, the mean probability of class cat over the mask.  The other results are the unscored call's bit for bit.

    component = 4 or 8 (fs_unwarp_instances_component; unpinned) keeps only the connected component of that mask under the gaze: focus
    (B,2) normalised (row, col) and snap_px as mask_component's.  stats, counts, bits, qsum, mask_prob and score then describe the
    component (the empty mask's record where there is none); cat and cls_prob are unchanged.  comp (B,4) int64 = (seed_y, seed_x, d2,
    area_all) is appended as the last element, behind conf / qsum where present.  Nothing is read on the host in between."""
    B, K = cls.shape
    _, h, w, _ = grid.shape
    if tuple(m.shape) != (B, h, w):
        raise ValueError(f"m {tuple(m.shape)} must be (B, h, w) = {(B, h, w)}: the mask at the grid's resolution")
    if component is None and (focus is not None or snap_px is not None):
        raise ValueError("focus and snap_px go with component = 4 or 8")
    Hs, Ws = int(Hs), int(Ws)
    cap = _max_runs(max_runs, Ws)
    dev = cls.device
    comp = component is not None
    if comp:
        conn, snap2 = _component_args(component, snap_px)
        if focus is None:
            raise ValueError("component needs focus (B, 2): the gaze that picks it")
        f = _focus_arg(focus, B, dev)
    cat = torch.empty(B, device=dev, dtype=torch.int64)
    stats = torch.empty(B, 6, device=dev, dtype=torch.int64)
    counts = torch.empty(B, cap, device=dev, dtype=torch.int32)
    bits = torch.empty(B, Hs, (Ws + 31) // 32, device=dev, dtype=torch.int32) if return_bits else None
    conf = torch.empty(B, 3, device=dev, dtype=torch.float32) if score else None
    qsum = torch.empty(B, device=dev, dtype=torch.int64) if score else None
    cout = torch.empty(B, 4, device=dev, dtype=torch.int64) if comp else None
    # the smallest entry point for what is asked; the component's takes conf and qsum null for no score
    name = "fs_unwarp_instances_component" if comp else "fs_unwarp_instances_scored" if score else "fs_unwarp_instances"
    scratch = torch.empty(hip.query(name + "_scratch_ints", B, h, w, Hs, Ws), device=dev, dtype=torch.int32)
    tensors = ([cls.contiguous(), m.contiguous(), grid.contiguous()] + ([f] if comp else []) + [cat, stats, counts, bits] +
               ([cout] if comp else []) + ([conf, qsum] if comp or score else []) + [scratch])
    hip.call(name, *[hip.ptr(t) for t in tensors], B, K, h, w, Hs, Ws, cap, *((conn, snap2) if comp else ()))
    return (cat, stats, counts) + ((bits,) if return_bits else ()) + ((conf, qsum) if score else ()) + ((cout,) if comp else ())


RLE_STATUS = {0: "valid", 1: "the code was cut: n_runs exceeds the capacity of counts", 2: "n_runs is below 1 or a count is negative",
              3: "the counts do not sum to Hs * Ws"}


def rle_bits(counts, n_runs, size, check=False):
    """mask_rle's inverse: the uncompressed run-length code back into bit words, on the device (fs_rle_bits; no autograd; unpinned, as
    the code itself).  counts (B,cap) int32 on the device, as mask_rle / unwarp_instances / coco_to_instances make them; n_runs the
    codes' lengths, int64 (B,) -- or a stats (B,6) int64 tensor, whose column 5 is read where it lies, without a copy; size = (Hs, Ws).
    Entries of counts at or past n_runs are never read.  Every well-formed code decodes, canonical or not (zero-length runs anywhere).
    Returns (bits (B,Hs,ceil(Ws/32)) int32 in mask_bits' layout, the bits at x >= Ws 0; info (B,4) int64 = (status, area, n_read,
    total)): status 0 valid, 1 cut (n_runs > cap), 2 bad (n_runs < 1 or a negative count), 3 the counts do not sum to Hs * Ws (the
    first that applies); area the set pixels of a valid code, else 0; an image whose status is not 0 gets all-zero words.  No host
    read -- unless check=True, which reads info once and raises ValueError naming the first such image and its status in words."""
    B, cap, Hs, Ws = _rle_args(counts, n_runs, size)
    n_runs = n_runs.contiguous()
    n_ptr, n_stride = (hip.ptr(n_runs) + 5 * 8, 6) if n_runs.dim() == 2 else (hip.ptr(n_runs), 1)
    dev = counts.device
    bits = torch.empty(B, Hs, (Ws + 31) // 32, device=dev, dtype=torch.int32)
    info = torch.empty(B, 4, device=dev, dtype=torch.int64)
    scratch = torch.empty(hip.query("fs_rle_bits_scratch_ints", B, cap), device=dev, dtype=torch.int32)
    hip.call("fs_rle_bits", hip.ptr(counts.contiguous()), n_ptr, n_stride, hip.ptr(bits), hip.ptr(info), hip.ptr(scratch), B, Hs, Ws, cap)
    if check:
        for b, st in enumerate(info[:, 0].cpu().tolist()):
            if st != 0:
                raise ValueError(f"image {b}: {RLE_STATUS[st]} (status {st}; size {(Hs, Ws)}, capacity {cap})")
    return bits, info


def _rle_args(counts, n_runs, size):
    """(B, cap, Hs, Ws) of rle_bits' arguments, or ValueError: the checks of the host, nothing launched."""
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.dim() != 2 or counts.numel() == 0:
        raise ValueError(f"counts must be a non-empty int32 (B, cap) tensor, got {getattr(counts, 'dtype', None)} {tuple(getattr(counts, 'shape', ()))}")
    B, cap = int(counts.shape[0]), int(counts.shape[1])
    if not isinstance(n_runs, torch.Tensor) or n_runs.dtype != torch.int64 or tuple(n_runs.shape) not in ((B,), (B, 6)) \
            or n_runs.device != counts.device:
        raise ValueError(f"n_runs must be an int64 (B,) = ({B},) tensor or a stats ({B}, 6) tensor on counts' device, got "
                         f"{getattr(n_runs, 'dtype', None)} {tuple(getattr(n_runs, 'shape', ()))}")
    if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in size):
        raise ValueError(f"size must be two integers >= 1 (Hs, Ws), got {size!r}")
    return B, cap, int(size[0]), int(size[1])


def rle_to_string(counts):
    """The compressed string form of a run-length code, the one COCO / LVIS files carry (host; unpinned: restated from the published
    definition, pycocotools' rleToString).  counts: a list of Python ints.  Count i is written as x = counts[i], less counts[i - 2]
    for i > 2, in 5-bit groups, low group first: c = x & 31, x >>= 5 (arithmetic); another group follows iff x != -1 where c & 16 is
    set, iff x != 0 otherwise; a group that is followed has bit 32 set; the character is chr(c + 48).  [0, 5] -> "05",
    [10, 20, 30, 5] -> ":d0n0A"."""
    out = []
    counts = list(counts)
    for i, v in enumerate(counts):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"count {i} must be a Python int, got {v!r}")
        x = v - counts[i - 2] if i > 2 else v
        while True:
            c = x & 31
            x >>= 5
            more = x != -1 if c & 16 else x != 0
            out.append(chr((c | 32 if more else c) + 48))
            if not more:
                break
    return "".join(out)


RLE_STRING_GROUPS = 13                              # 65 bits: more than any int64 count or difference needs


def rle_from_string(s):
    """rle_to_string's inverse (host; unpinned: pycocotools' rleFrString restated): s a str or ASCII bytes -> the list of counts.  Per
    count, (c & 31) << 5 k is accumulated over the groups k = 0, 1, ... while bit 32 of c = ord(ch) - 48 is set, the value is
    sign-extended from bit 16 of the last group, and counts[i - 2] is added for i > 2.  ValueError, naming the position, for a character
    outside chr(48) .. chr(111), a string that ends inside a count, or a count of more than 13 groups; an empty string is []."""
    if isinstance(s, (bytes, bytearray)):
        try:
            s = bytes(s).decode("ascii")
        except UnicodeDecodeError:
            raise ValueError("the compressed code holds a byte outside ASCII") from None
    if not isinstance(s, str):
        raise ValueError(f"the compressed code must be a str or bytes, got {type(s).__name__}")
    counts, p, n = [], 0, len(s)
    while p < n:
        x, k = 0, 0
        while True:
            if p >= n:
                raise ValueError(f"the compressed code ends inside count {len(counts)} (position {p})")
            c = ord(s[p]) - 48
            if c < 0 or c > 63:
                raise ValueError(f"character {s[p]!r} at position {p} is outside chr(48) .. chr(111)")
            if k >= RLE_STRING_GROUPS:
                raise ValueError(f"count {len(counts)} has more than {RLE_STRING_GROUPS} groups (position {p})")
            x |= (c & 31) << (5 * k)
            p, k = p + 1, k + 1
            if not c & 32:
                if c & 16:
                    x -= 1 << (5 * k)
                break
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def instances_to_coco(cat, stats, counts, seg_size, image_ids=None, conf=None, compressed=False):
    """unwarp_instances' / predict_instances' tensors (on any device) as a list of COCO / LVIS result records, one per image:
    {"image_id", "category_id", "bbox": [x, y, w, h], "area", "segmentation": {"size": [H, W], "counts": [...]}} with the uncompressed
    run-length code pycocotools.mask.frPyObjects takes -- or, with compressed=True, "counts" as the compressed string result files carry
    (rle_to_string; about a fifth of the list's size in JSON).  One device-to-host copy.  category_id is the class index cat[b]; image_id is
    image_ids[b], or b.  With conf (B,3) -- unwarp_instances(score=True)'s / predict_instances(return_score=True)'s -- every record
    also has "score": conf[b, 0] as a Python float, the key COCOeval and the LVIS evaluator rank by; without it no score is made up.
    OverflowError, naming the image and the max_runs it needs, where a code was cut (n_runs > counts.shape[1]); ValueError, naming the
    image, where a score is NaN.  coco_to_instances is the inverse."""
    B, cap = int(counts.shape[0]), int(counts.shape[1])
    if tuple(cat.shape) != (B,) or tuple(stats.shape) != (B, 6) or counts.dim() != 2:
        raise ValueError(f"cat {tuple(cat.shape)}, stats {tuple(stats.shape)}, counts {tuple(counts.shape)} must be (B,), (B, 6), (B, max_runs)")
    H, W = int(seg_size[0]), int(seg_size[1])
    ids = list(range(B)) if image_ids is None else list(image_ids)
    if len(ids) != B:
        raise ValueError(f"{len(ids)} image ids for {B} images")
    if conf is not None and (conf.dim() != 2 or conf.shape[0] != B or conf.shape[1] < 1):
        raise ValueError(f"conf {tuple(conf.shape)} must be (B, 3) = ({B}, 3): (score, cls_prob, mask_prob) per image")
    head = torch.cat([cat.to(torch.int64).reshape(B, 1), stats.to(torch.int64)], 1).contiguous()
    parts = [head.view(torch.int32)]                                                   # the int64 columns as pairs of words
    if conf is not None:
        parts.append(conf[:, :1].to(torch.float32).contiguous().view(torch.int32))     # the score's fp32 word
    n0 = sum(int(t.shape[1]) for t in parts)
    host = torch.cat(parts + [counts.to(torch.int32)], 1).cpu()
    head, code = host[:, :14].contiguous().view(torch.int64).tolist(), host[:, n0:]
    scores = host[:, 14:15].contiguous().view(torch.float32).reshape(B).tolist() if conf is not None else None
    out = []
    for b in range(B):
        c, area, x0, y0, bw, bh, n = head[b]
        if n > cap:
            raise OverflowError(f"image {ids[b]}: the run-length code has {n} counts and was cut at max_runs = {cap}; it needs max_runs >= {n}")
        runs = code[b, :n].tolist()
        rec = {"image_id": ids[b], "category_id": c, "bbox": [x0, y0, bw, bh], "area": area,
               "segmentation": {"size": [H, W], "counts": rle_to_string(runs) if compressed else runs}}
        if scores is not None:
            if scores[b] != scores[b]:
                raise ValueError(f"image {ids[b]}: the score is NaN (a NaN among the head's class logits)")
            rec["score"] = scores[b]
        out.append(rec)
    return out


INT32_MAX = 2 ** 31 - 1


def coco_to_instances(records, device, max_runs=None):
    """instances_to_coco's inverse: a list of COCO / LVIS result records, or of annotation records, as the tensors the library's own
    operations take.  Every record has "image_id", "category_id" and "segmentation" = {"size": [H, W], "counts": ...}, counts a list of
    ints (the uncompressed code) or the compressed string (rle_from_string); "score" in every record or in none.  Returns (image_ids, a
    list; cat (n,) int64; n_runs (n,) int64; counts (n,cap) int32, zero behind each code; sizes (n,2) int64 = (H, W); scores (n,)
    fp32, or None where no record has one), the tensors on `device`, made by ONE host-to-device copy.  cap defaults to the longest code;
    with max_runs (an int >= 1) a longer code is stored cut while n_runs stays its true length, which rle_bits reports as status 1.
    rle_bits(counts[sel], n_runs[sel], (H, W)) decodes the records of one size.  ValueError, naming the record, for a polygon
    segmentation (rasterising polygons is not built), a missing key, a count outside int32, a malformed string, or scores in only some."""
    records = list(records)
    if not records:
        raise ValueError("no records")
    rows, ids, longest = [], [], 1
    with_score = [isinstance(r, dict) and "score" in r for r in records]
    if any(with_score) and not all(with_score):
        raise ValueError(f"record {with_score.index(False)} has no score while others have: scores go with every record or with none")
    for i, r in enumerate(records):
        if not isinstance(r, dict):
            raise ValueError(f"record {i} is no dict")
        for key in ("image_id", "category_id", "segmentation"):
            if key not in r:
                raise ValueError(f"record {i}: the key {key!r} is missing")
        seg = r["segmentation"]
        if not isinstance(seg, dict):
            raise ValueError(f"record {i} (image {r['image_id']!r}): the segmentation is a polygon list, not an RLE dict; polygons are not rasterised here")
        for key in ("size", "counts"):
            if key not in seg:
                raise ValueError(f"record {i} (image {r['image_id']!r}): the segmentation's key {key!r} is missing")
        size, code = seg["size"], seg["counts"]
        if len(size) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 or v > INT32_MAX for v in size):
            raise ValueError(f"record {i} (image {r['image_id']!r}): the size must be two integers >= 1, got {size!r}")
        if isinstance(code, (str, bytes, bytearray)):
            try:
                code = rle_from_string(code)
            except ValueError as e:
                raise ValueError(f"record {i} (image {r['image_id']!r}): {e}") from None
        code = list(code)
        for j, v in enumerate(code):
            if isinstance(v, bool) or not isinstance(v, int) or v < -INT32_MAX - 1 or v > INT32_MAX:
                raise ValueError(f"record {i} (image {r['image_id']!r}): count {j} = {v!r} is no integer within int32")
        c = r["category_id"]
        if isinstance(c, bool) or not isinstance(c, int):
            raise ValueError(f"record {i} (image {r['image_id']!r}): category_id must be an integer, got {c!r}")
        ids.append(r["image_id"])
        rows.append((c, len(code), int(size[0]), int(size[1]), code))
        longest = max(longest, len(code))
    cap = longest if max_runs is None else _max_runs(max_runs, 1)
    n = len(rows)
    head = torch.tensor([row[:4] for row in rows], dtype=torch.int64).reshape(n, 4)
    score = torch.tensor([float(r["score"]) for r in records] if all(with_score) else [0.0] * n, dtype=torch.float32).reshape(n, 1)
    code = torch.zeros(n, cap, dtype=torch.int32)
    for i, row in enumerate(rows):
        m = min(row[1], cap)
        if m:
            code[i, :m] = torch.tensor(row[4][:m], dtype=torch.int32)
    dev = torch.cat([head.view(torch.int32), score.view(torch.int32), code], 1).to(device)            # the one copy
    head = dev[:, :8].reshape(-1).view(torch.int64).reshape(n, 4)                                     # flat first: a row's stride is odd
    scores = dev[:, 8].contiguous().view(torch.float32) if all(with_score) else None
    return ids, head[:, 0].contiguous(), head[:, 1].contiguous(), dev[:, 9:].contiguous(), head[:, 2:4].contiguous(), scores


POLY_SIDE_MAX = 16384                               # fs_poly_bits' cap on a side: coordinate products stay inside int32
POLY_STATUS = {0: "valid", 1: "the image's ring or vertex offsets are out of range or decreasing"}


def polygon_rings(polys):
    """COCO / LVIS polygon lists as the three tables fs_poly_bits takes (host).  polys: a list with one entry per image, each entry a
    polygon list [[x0, y0, x1, y1, ...], ...] as an annotation's "segmentation" carries it; an empty polygon list is allowed and is
    the empty mask.  Returns CPU tensors (verts (V,2) int32 = (y, x); ring_off (R+1,) int32: ring r owns verts[ring_off[r] :
    ring_off[r+1]]; img_ring (B+1,) int32: image b owns the rings img_ring[b] : img_ring[b+1]).  The coordinates are rounded half to
    even on float64 (np.round, as the reference's b2_preprocess_lvis.py:282-297 does) and NOT clipped: poly_bits clamps them onto
    the frame.  ValueError, naming the image and the ring, for an entry that is not a list of lists, a ring of odd or zero length, a
    coordinate that is no number or not finite, and a rounded value outside int32."""
    import numpy as np
    if not isinstance(polys, (list, tuple)):
        raise ValueError(f"polys must be a list with one polygon list per image, got {type(polys).__name__}")
    rows, ring_off, img_ring = [], [0], [0]
    for b, entry in enumerate(polys):
        if not isinstance(entry, (list, tuple)) or any(not isinstance(ring, (list, tuple)) for ring in entry):
            raise ValueError(f"image {b}: the segmentation must be a polygon list, a list of lists [x0, y0, x1, y1, ...]")
        for j, ring in enumerate(entry):
            if len(ring) == 0 or len(ring) % 2:
                raise ValueError(f"image {b}, ring {j}: a ring is x, y pairs; it has {len(ring)} numbers")
            for k, v in enumerate(ring):
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise ValueError(f"image {b}, ring {j}: coordinate {k} = {v!r} is no number")
            try:
                xy = np.round(np.array([float(v) for v in ring], dtype=np.float64))
            except OverflowError:
                raise ValueError(f"image {b}, ring {j}: a coordinate is outside float64") from None
            if not np.isfinite(xy).all():
                raise ValueError(f"image {b}, ring {j}: coordinate {int(np.flatnonzero(~np.isfinite(xy))[0])} is not finite")
            if (xy < -INT32_MAX - 1).any() or (xy > INT32_MAX).any():
                raise ValueError(f"image {b}, ring {j}: a rounded coordinate is outside int32")
            rows.append(xy.reshape(-1, 2)[:, ::-1].astype(np.int32))                  # (x, y) pairs -> (y, x)
            ring_off.append(ring_off[-1] + len(ring) // 2)
        img_ring.append(len(ring_off) - 1)
    if ring_off[-1] > INT32_MAX:
        raise ValueError(f"{ring_off[-1]} vertices are more than int32 offsets hold")
    verts = np.concatenate(rows, 0) if rows else np.zeros((0, 2), dtype=np.int32)
    return (torch.from_numpy(np.ascontiguousarray(verts)), torch.tensor(ring_off, dtype=torch.int32), torch.tensor(img_ring, dtype=torch.int32))


def _poly_args(verts, ring_off, img_ring, size):
    """(B, R, V, Hs, Ws) of poly_bits' arguments, or ValueError: the checks of the host, nothing launched."""
    for name, t, ok in (("verts", verts, lambda t: t.dim() == 2 and t.shape[1] == 2), ("ring_off", ring_off, lambda t: t.dim() == 1 and t.numel() >= 1),
                        ("img_ring", img_ring, lambda t: t.dim() == 1 and t.numel() >= 2)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not ok(t):
            raise ValueError(f"{name} must be an int32 tensor -- verts (V, 2), ring_off (R + 1,), img_ring (B + 1,), B >= 1 -- got "
                             f"{getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))}")
    if not (verts.device == ring_off.device == img_ring.device):
        raise ValueError("verts, ring_off and img_ring must be on one device")
    if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 or int(v) > POLY_SIDE_MAX for v in size):
        raise ValueError(f"size must be two integers 1 .. {POLY_SIDE_MAX} (Hs, Ws), got {size!r}")
    return int(img_ring.numel()) - 1, int(ring_off.numel()) - 1, int(verts.shape[0]), int(size[0]), int(size[1])


def poly_bits(verts, ring_off, img_ring, size, device=None, check=False):
    """Polygon lists as bit words, on the device (fs_poly_bits; no autograd).  verts, ring_off, img_ring as polygon_rings makes them
    (int32; (y, x) vertices rounded but not clipped), size = (Hs, Ws), each side at most 16384.  Tables on the host go to `device`
    (default "cuda") in ONE host-to-device copy; tables already on a device are used where they lie.  UNPINNED -- the reference makes
    its labels with np.round, a clip onto the frame and skimage.draw.polygon (b2_preprocess_lvis.py:282-297), which is not at hand, so
    the rule is this library's restatement of what that is understood to give for integer vertices, not verified against it: a vertex
    is clamped to the frame; a ring is the closed chain of a polygon's vertices; it sets pixel (y, x) iff the pixel lies on one of its
    edges (end points included) or the even-odd crossing number is odd (edges oriented so that y0 < y1, y0 <= y < y1, counted where
    (x - x0)(y1 - y0) < (y - y0)(x1 - x0)); an image's mask is the OR of its rings, so overlapping polygons do not cancel while a
    self-intersecting ring follows even-odd.  It is not pycocotools' frPoly, which traces a 5x upsampled outline and differs along the
    rim.  Returns (bits (B,Hs,ceil(Ws/32)) int32 in mask_bits' layout, the bits at x >= Ws 0; info (B,4) int64 = (status, area,
    n_rings, n_vertices)): status 0 valid, 1 the image's offsets are out of range or decreasing (all-zero words, area 0); an image
    without rings is the empty mask.  No host read -- unless check=True, which reads info once and raises ValueError naming the first
    image whose status is not 0.  mask_rle(bits, Ws) gives the label evaluate_instances(seg_label=(counts, stats)) takes."""
    B, R, V, Hs, Ws = _poly_args(verts, ring_off, img_ring, size)
    if verts.device.type == "cpu":
        dev = torch.device("cuda" if device is None else device)
        keep = torch.cat([img_ring, ring_off, verts.reshape(-1)]).to(dev)              # the one copy
        p_img = hip.ptr(keep)
        p_ring, p_verts = p_img + 4 * (B + 1), p_img + 4 * (B + 1 + R + 1)             # the buffer's end where V = 0: never read
    else:
        dev = verts.device
        if device is not None and torch.device(device) != dev:
            raise ValueError(f"the tables are on {dev}, not on {device}")
        keep = (verts.contiguous(), ring_off.contiguous(), img_ring.contiguous())
        p_ring, p_img = hip.ptr(keep[1]), hip.ptr(keep[2])
        p_verts = hip.ptr(keep[0]) if V else p_ring
    bits = torch.empty(B, Hs, (Ws + 31) // 32, device=dev, dtype=torch.int32)
    info = torch.empty(B, 4, device=dev, dtype=torch.int64)
    scratch = torch.empty(max(1, hip.query("fs_poly_bits_scratch_ints", B, Hs, Ws)), device=dev, dtype=torch.int32)
    hip.call("fs_poly_bits", p_verts, p_ring, p_img, hip.ptr(bits), hip.ptr(info), hip.ptr(scratch), B, R, V, Hs, Ws)
    del keep                                                                           # the tables, held until the launch is queued
    if check:
        for b, st in enumerate(info[:, 0].cpu().tolist()):
            if st != 0:
                raise ValueError(f"image {b}: {POLY_STATUS[st]} (status {st}; {R} rings, {V} vertices)")
    return bits, info


def coco_masks(records, size, device):
    """COCO / LVIS records of ONE size as bit words, whichever way each carries its mask: "segmentation" an RLE dict (counts a list or
    the compressed string) or a polygon list.  size = (H, W); records as coco_to_instances takes them ("image_id", "category_id",
    "segmentation"; "score" in every record or in none).  Returns (image_ids, a list; cat (n,) int64; bits (n,H,ceil(W/32)) int32;
    info (n,2) int64 = (status, area); scores (n,) fp32 or None), the rows in record order.  RLE rows go through coco_to_instances and
    rle_bits, polygon rows through polygon_rings and poly_bits (unpinned rules both; see there): each kind is handed all n rows, the
    other kind's rows as empty masks, and the two results are ORed, so the order needs no index on the device.  At most two
    host-to-device copies (one a kind) and no host read: a code or offsets that are not valid give an empty mask and a status that is
    not 0 (rle_bits' for an RLE row, poly_bits' for a polygon row).  ValueError as coco_to_instances and polygon_rings raise it (the
    latter's "image i" is record i), and for an RLE record whose size is not `size`."""
    records = list(records)
    if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in size):
        raise ValueError(f"size must be two integers >= 1 (H, W), got {size!r}")
    H, W = int(size[0]), int(size[1])
    empty = {"size": [H, W], "counts": [H * W]}
    as_rle, polys, n_poly = [], [], 0
    for i, r in enumerate(records):
        seg = r.get("segmentation") if isinstance(r, dict) else None
        if isinstance(seg, (list, tuple)):
            as_rle.append(dict(r, segmentation=empty))
            polys.append(seg)
            n_poly += 1
        else:
            if isinstance(seg, dict) and "size" in seg and list(seg["size"]) != [H, W]:
                raise ValueError(f"record {i} (image {r.get('image_id')!r}): the code's size {seg['size']!r} is not {[H, W]}")
            as_rle.append(r)
            polys.append([])
    ids, cat, n_runs, counts, _sizes, scores = coco_to_instances(as_rle, device)
    bits = info = None
    if n_poly < len(records):
        bits, info4 = rle_bits(counts, n_runs, (H, W))
        info = info4[:, :2]
    if n_poly:
        pbits, pinfo = poly_bits(*polygon_rings(polys), (H, W), device=device)
        bits, info = (pbits, pinfo[:, :2]) if bits is None else (bits | pbits, info + pinfo[:, :2])
    return ids, cat, bits, info.contiguous(), scores


def _candidate_args(cbits, cand_off, Ws, cand_cat):
    """(N, Hs, P, B) of mask_candidates' tables, or ValueError: the checks of the host, nothing launched."""
    if not isinstance(cbits, torch.Tensor) or cbits.dtype != torch.int32 or cbits.dim() != 3 or Ws is None or isinstance(Ws, bool) \
            or int(Ws) != Ws or int(Ws) < 1 or cbits.shape[2] != (int(Ws) + 31) // 32 or cbits.shape[1] < 1:
        raise ValueError(f"cbits must be int32 bit words (N, Hs, ceil(Ws / 32)) with Hs >= 1 and Ws given, got "
                         f"{getattr(cbits, 'dtype', None)} {tuple(getattr(cbits, 'shape', ()))} and Ws = {Ws!r}")
    N, Hs, P = (int(v) for v in cbits.shape)
    if not isinstance(cand_off, torch.Tensor) or cand_off.dtype != torch.int32 or cand_off.dim() != 1 or cand_off.numel() < 2:
        raise ValueError(f"cand_off must be an int32 tensor (B + 1,), B >= 1, got {getattr(cand_off, 'dtype', None)} "
                         f"{tuple(getattr(cand_off, 'shape', ()))}")
    if cand_cat is not None and (not isinstance(cand_cat, torch.Tensor) or cand_cat.dtype != torch.int64 or tuple(cand_cat.shape) != (N,)):
        raise ValueError(f"cand_cat must be int64 ({N},), got {getattr(cand_cat, 'dtype', None)} {tuple(getattr(cand_cat, 'shape', ()))}")
    for name, t in (("cand_off", cand_off), ("cand_cat", cand_cat)):
        if t is not None and t.device != cbits.device:
            raise ValueError(f"{name} is on {t.device}, cbits on {cbits.device}")
    if Hs > POLY_SIDE_MAX or int(Ws) > POLY_SIDE_MAX:
        raise ValueError(f"a side of {(Hs, int(Ws))} is above {POLY_SIDE_MAX}")
    return N, Hs, P, int(cand_off.numel()) - 1


def mask_candidates(cbits, cand_off, focus, Ws, pred=None, cand_cat=None, snap_px=None):
    """Of every image's annotated instances, the one under the gaze, on the device and on bit words (fs_mask_candidates; no autograd).
    UNPINNED: the reference builds its labels by choosing an annotation and putting the gaze inside it
    (b2_preprocess_lvis.py:258-333); this is the inverse of that step and a definition of this library's.  cbits (N,Hs,ceil(Ws/32))
    int32, the candidates' masks in mask_bits' layout (N = 0 allowed; the bits at x >= Ws are not read); cand_off (B+1,) int32: image
    b owns the rows cand_off[b] : cand_off[b+1]; focus (B,2) normalised (row, col), turned into a gaze pixel as mask_component does;
    pred (B,Hs,ceil(Ws/32)) int32 or None, a prediction's bit words per image; cand_cat (N,) int64 or None; snap_px None (any
    distance) or a finite number of pixels >= 0, snap2 = floor(snap_px ** 2) (as mask_component).  Returns (gbits, sel, cand):

    cand (N,6) int64 = (b, area, inter, d2, near_y, near_x): the row's image, its set pixels, |c & pred[b]| (0 without pred), and its
    set pixel nearest to the gaze pixel with the squared distance (ties to the smaller row-major index; -1, -1, -1 for an empty row).
    sel (B,8) int64 = (index, cls, d2, area, inter, n_hit, best, status).  index: the SELECTED row -- among the image's rows with area >
    0 and d2 <= snap2 the least (d2, area, row): of several instances that contain the gaze pixel the smallest (a cup on a table gives
    the cup), of none the nearest within the snap distance, ties to the smaller area, then row -- or -1; cls = cand_cat[index] (-1
    for none or without cand_cat); d2, area, inter the selected row's (-1, 0, 0); n_hit how many of the image's rows contain the gaze
    pixel; best: among rows with inter > 0 the one of the greatest IoU with pred[b], compared exactly in integers, ties to the smaller
    area, then row, or -1.  gbits (B,Hs,ceil(Ws/32)) int32 = the selected row's words with the bits at x >= Ws cleared, all 0 where
    none is selected.  status 1 in every image where cand_off is not 0 = cand_off[0] <= ... <= cand_off[B] = N: then nothing is
    selected anywhere and every cand row is (-1, area, 0, -1, -1, -1).  No host read; the same bits in every run."""
    _conn, snap2 = _component_args(8, snap_px)
    N, Hs, P, B = _candidate_args(cbits, cand_off, Ws, cand_cat)
    Ws, dev = int(Ws), cbits.device
    f = _focus_arg(focus, B, dev)
    if pred is not None and (not isinstance(pred, torch.Tensor) or pred.dtype != torch.int32 or tuple(pred.shape) != (B, Hs, P) or pred.device != dev):
        raise ValueError(f"pred must be int32 bit words {(B, Hs, P)} on {dev}, got {getattr(pred, 'dtype', None)} {tuple(getattr(pred, 'shape', ()))}")
    gbits = torch.empty(B, Hs, P, device=dev, dtype=torch.int32)
    sel = torch.empty(B, 8, device=dev, dtype=torch.int64)
    cand = torch.empty(N, 6, device=dev, dtype=torch.int64)
    scratch = torch.empty(max(1, hip.query("fs_mask_candidates_scratch_ints", B, N, Hs, Ws)), device=dev, dtype=torch.int32)
    hip.call("fs_mask_candidates", hip.ptr(cbits.contiguous()) if N else None, hip.ptr(cand_off.contiguous()),
             None if cand_cat is None or N == 0 else hip.ptr(cand_cat.contiguous()), hip.ptr(f),
             None if pred is None else hip.ptr(pred.contiguous()), hip.ptr(cand) if N else None, hip.ptr(sel), hip.ptr(gbits),
             hip.ptr(scratch), B, N, Hs, Ws, snap2)
    return gbits, sel, cand


def coco_candidates(records, size, device, image_ids):
    """COCO / LVIS annotation records of ONE size, several an image, as mask_candidates' arguments.  records as coco_masks takes them
    (RLE dicts or polygon lists, mixed); size = (H, W); image_ids the images in the order the batch has them.  The records are grouped
    stably by "image_id" in the order of image_ids -- an id without records gets an empty range -- and rasterised through coco_masks
    with its copies (at most two) plus one for the offsets.  Returns (cbits (N,H,ceil(W/32)) int32; cand_off (B+1,) int32; cand_cat
    (N,) int64; info (N,2) int64 = coco_masks' (status, area); rows, a list: rows[i] is the index into `records` of candidate row i,
    which maps mask_candidates' sel[:, 0] back to an annotation: records[rows[index]]["id"]).  "iscrowd" is not interpreted: a
    crowd record is a candidate like any other.  ValueError for a record whose image is not in image_ids, an id named twice, and as
    coco_masks."""
    records, image_ids = list(records), list(image_ids)
    if not image_ids:
        raise ValueError("no image_ids")
    place = {}
    for b, image_id in enumerate(image_ids):
        if image_id in place:
            raise ValueError(f"image_ids names {image_id!r} twice")
        place[image_id] = b
    per = [[] for _ in image_ids]
    for i, r in enumerate(records):
        if not isinstance(r, dict) or "image_id" not in r:
            raise ValueError(f"record {i}: the key 'image_id' is missing")
        if r["image_id"] not in place:
            raise ValueError(f"record {i}: image {r['image_id']!r} is not among image_ids")
        per[place[r["image_id"]]].append(i)
    rows = [i for group in per for i in group]
    off = [0]
    for group in per:
        off.append(off[-1] + len(group))
    if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in size):
        raise ValueError(f"size must be two integers >= 1 (H, W), got {size!r}")
    dev = torch.device(device)
    H, W = int(size[0]), int(size[1])
    cand_off = torch.tensor(off, dtype=torch.int32).to(dev)
    if not rows:
        return (torch.empty(0, H, (W + 31) // 32, device=dev, dtype=torch.int32), cand_off, torch.empty(0, device=dev, dtype=torch.int64),
                torch.empty(0, 2, device=dev, dtype=torch.int64), rows)
    _ids, cat, cbits, info, _scores = coco_masks([{k: v for k, v in records[i].items() if k != "score"} for i in rows], size, dev)
    return cbits, cand_off, cat, info, rows


GATE_TILES = (8, 16, 32, 64)
GATE_CODES = {0: "REUSE", 1: "RUN_INIT", 2: "HOLD_SACCADE", 3: "RUN_SCENE", 4: "RUN_ROI", 5: "RUN_GAZE", 6: "RUN_AGE", 7: "RUN_FORCED"}
GATE_RUNS = (1, 3, 4, 5, 6, 7)                      # the codes after which the network runs


def _gate_tile(T):
    if isinstance(T, bool) or int(T) != T or int(T) not in GATE_TILES:
        raise ValueError(f"the tile side must be one of {GATE_TILES}, got {T!r}")
    return int(T)


def _gate_tiles(dtype, img, key, tile, out):
    T = _gate_tile(tile)
    what = "fp32" if dtype == torch.float32 else "uint8"
    if not isinstance(img, _FRAME_TYPES) or img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0 or img.dtype != dtype:
        raise ValueError(f"img must be a non-empty {what} (B,3,H,W), got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))}")
    if key.dtype != torch.uint8 or key.shape != img.shape:
        raise ValueError(f"key must be uint8 {tuple(img.shape)}, got {key.dtype} {tuple(key.shape)}")
    B, _, H, W = (int(v) for v in img.shape)
    suffix, strides = _frame_route(img)
    shape = (B, (H + T - 1) // T, (W + T - 1) // T)
    if out is None:
        out = torch.empty(shape, device=img.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or tuple(out.shape) != shape:
        raise ValueError(f"out must be int32 {shape}, got {out.dtype} {tuple(out.shape)}")
    hip.call("fs_gate_tiles" + suffix, *_frame_args(img, strides), hip.ptr(key), hip.ptr(out), B, H, W, T)
    return out


def gate_tiles(img, key, tile=32, out=None):
    """How much every tile of new frames differs from the 8-bit key frames (fs_gate_tiles; no autograd; unpinned: the reference has
    no counterpart).  img (B,3,H,W) fp32, key (B,3,H,W) uint8 = q of the frames the records were made from, q(v) = rint(clamp(v, 0, 1) *
    255) in fp32, NaN -> 0.  Returns sad (B,th,tw) int32, th = ceil(H / tile), tw = ceil(W / tile): the sum of |q(img) - key| over the
    three channels and the tile's pixels (the last tiles are ragged).  out: a (B,th,tw) int32 tensor to write into."""
    return _gate_tiles(torch.float32, img, key, tile, out)


def gate_tiles_u8(img, key, tile=32, out=None):
    """gate_tiles for frames of bytes (fs_gate_tiles_u8): img (B,3,H,W) uint8, the pixel value byte / 255, whose code q is the byte.  sad
    is the sum of |img - key|, equal to gate_tiles(img.float() / 255, key, tile); 6 bytes read a pixel instead of 15.  img is contiguous,
    or an hwc view of interleaved bytes (byte_frame_layout; fs_gate_tiles_hwc), read where it lies; ValueError for any other layout."""
    return _gate_tiles(torch.uint8, img, key, tile, out)


def gate_decide(sad, gstate, focus, stats, bits, frame_size, tile=32, level=8, scene_tiles=0, roi_tiles=0, margin=16,
                saccade2=2 ** 62, fixation2=0, max_age=0, inside_on=True, force=None, out=None):
    """The gate's decision per viewer (fs_gate_decide; no autograd; unpinned).  sad (B,th,tw) int32 as gate_tiles returns it; gstate
    (B,6) int64 = (valid, gy_key, gx_key, gy_prev, gx_prev, age), gazes in 1/16-pixel units; focus (B,2) fp32 normalised (row, col);
    stats (B,6) int64 and bits (B,H,ceil(W/32)) int32 the records' (mask_rle, mask_bits); force (B,) int32 or None; frame_size = (H, W).
    saccade2 and fixation2 are squared distances in 1/16-pixel units, floor((px * 16) ** 2).  Returns gate (B,8) int64 = (code,
    n_changed, n_roi_changed, sad_total, d2_key, d2_prev, inside_bit, age + 1); the codes are GATE_CODES, the first rule that holds in
    the order 7, 1, 2, 3, 4, 5, 6, 0 (include/fovealseg.h).  Nothing but gate is written."""
    T = _gate_tile(tile)
    H, W = int(frame_size[0]), int(frame_size[1])
    B = int(sad.shape[0])
    if sad.dtype != torch.int32 or tuple(sad.shape) != (B, (H + T - 1) // T, (W + T - 1) // T):
        raise ValueError(f"sad must be int32 (B, ceil(H/T), ceil(W/T)) for H, W, T = {H}, {W}, {T}, got {sad.dtype} {tuple(sad.shape)}")
    if gstate.dtype != torch.int64 or tuple(gstate.shape) != (B, 6) or stats.dtype != torch.int64 or tuple(stats.shape) != (B, 6):
        raise ValueError(f"gstate and stats must be int64 ({B}, 6), got {tuple(gstate.shape)} and {tuple(stats.shape)}")
    if focus.dtype != torch.float32 or tuple(focus.shape) != (B, 2):
        raise ValueError(f"focus must be fp32 ({B}, 2), got {focus.dtype} {tuple(focus.shape)}")
    if bits.dtype != torch.int32 or tuple(bits.shape) != (B, H, (W + 31) // 32):
        raise ValueError(f"bits must be int32 {(B, H, (W + 31) // 32)}, got {bits.dtype} {tuple(bits.shape)}")
    if force is not None and (force.dtype != torch.int32 or tuple(force.shape) != (B,)):
        raise ValueError(f"force must be int32 ({B},), got {force.dtype} {tuple(force.shape)}")
    if isinstance(level, bool) or int(level) != level or not 0 <= int(level) <= 254:
        raise ValueError(f"level must be an integer 0 .. 254, got {level!r}")
    if int(margin) < 0:
        raise ValueError(f"margin must be >= 0, got {margin!r}")
    if out is None:
        out = torch.empty(B, 8, device=sad.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, 8):
        raise ValueError(f"out must be int64 ({B}, 8), got {out.dtype} {tuple(out.shape)}")
    hip.call("fs_gate_decide", hip.ptr(sad), hip.ptr(gstate), hip.ptr(focus), hip.ptr(stats), hip.ptr(bits), hip.ptr(force), hip.ptr(out),
             B, H, W, T, int(level), int(scene_tiles), int(roi_tiles), int(margin), int(saccade2), int(fixation2), int(max_age),
             1 if inside_on else 0)
    return out


def _gate_commit(dtype, img, idx, key, gstate, focus, src, dst):
    what = "fp32" if dtype == torch.float32 else "uint8"
    if (not isinstance(img, _FRAME_TYPES) or img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0 or img.dtype != dtype
            or key.dtype != torch.uint8 or key.shape != img.shape):
        raise ValueError(f"img must be a non-empty {what} (B,3,H,W) and key uint8 of its shape, got {getattr(img, 'dtype', None)} "
                         f"{tuple(getattr(img, 'shape', ()))} and {tuple(key.shape)}")
    B, _, H, W = (int(v) for v in img.shape)
    suffix, strides = _frame_route(img)
    n = 0 if idx is None else int(idx.shape[0])
    if idx is not None and (idx.dtype != torch.int32 or idx.dim() != 1 or n > B):
        raise ValueError(f"idx must be int32 (n,) with n <= {B}, got {idx.dtype} {tuple(idx.shape)}")
    if gstate.dtype != torch.int64 or tuple(gstate.shape) != (B, 6) or focus.dtype != torch.float32 or tuple(focus.shape) != (B, 2):
        raise ValueError(f"gstate must be int64 ({B}, 6) and focus fp32 ({B}, 2), got {tuple(gstate.shape)} and {tuple(focus.shape)}")
    if len(src) != len(dst) or len(dst) not in (4, 5):
        raise ValueError("src and dst must both be (cat, stats, counts, bits) or (cat, stats, counts, bits, conf)")
    cap = int(dst[2].shape[1])
    tails = ((), (6,), (cap,), (H, (W + 31) // 32), (3,))
    dtypes = (torch.int64, torch.int64, torch.int32, torch.int32, torch.float32)
    for s, d, tail, dt in zip(src, dst, tails, dtypes):
        if d.dtype != dt or tuple(d.shape) != (B,) + tail:
            raise ValueError(f"a dst record tensor must be {dt} {(B,) + tail}, got {d.dtype} {tuple(d.shape)}")
        if s is not d and n > 0 and (s.dtype != dt or tuple(s.shape) != (n,) + tail):
            raise ValueError(f"a src record tensor must be {dt} {(n,) + tail}, got {s.dtype} {tuple(s.shape)}")
    sp = [hip.ptr(s) for s in src] + [None] * (5 - len(src))
    dp = [hip.ptr(d) for d in dst] + [None] * (5 - len(dst))
    hip.call("fs_gate_commit" + suffix, *_frame_args(img, strides), hip.ptr(idx), n, hip.ptr(key), hip.ptr(gstate), hip.ptr(focus), *sp, *dp,
             B, H, W, cap)


def gate_commit(img, idx, key, gstate, focus, src, dst):
    """What a step leaves behind (fs_gate_commit; no autograd; unpinned), in place.  idx (n,) int32 ascending, or None for n = 0: the
    viewers whose record was made anew from img (B,3,H,W) fp32.  src = (cat, stats, counts, bits[, conf]) with n rows, dst the same
    with B rows: row j moves to row idx[j]; a pair that is one tensor is already in place.  For the viewers of idx key (B,3,H,W) uint8
    <- q(img), g_key <- g, age <- 0, valid <- 1 in gstate (B,6) int64; for every viewer g_prev <- g; any other viewer's age grows by
    one.  With n = 0 src is not read (pass dst)."""
    _gate_commit(torch.float32, img, idx, key, gstate, focus, src, dst)


def gate_commit_u8(img, idx, key, gstate, focus, src, dst):
    """gate_commit for frames of bytes (fs_gate_commit_u8): img (B,3,H,W) uint8; for the viewers of idx key <- img, a copy.  Everything
    else as gate_commit, and equal to it on img.float() / 255.  img is contiguous, or an hwc view of interleaved bytes (byte_frame_layout;
    fs_gate_commit_hwc: the key takes the de-interleaved frame and stays planar); ValueError for any other layout."""
    _gate_commit(torch.uint8, img, idx, key, gstate, focus, src, dst)


MOTION_MAX_PX = 255                                 # fs_profile_shift's largest search range


def _index_or_none(v):
    """v as an int where it is an integer of any integer type (no bool, no float), else None."""
    if isinstance(v, bool):
        return None
    try:
        return operator.index(v)
    except TypeError:
        return None


def _motion_px(motion_px, H, W):
    """The search range R of the motion estimate: an integer 1 .. 255 with 4 R < min(H, W)."""
    R = _index_or_none(motion_px)
    if R is None or not 1 <= R <= MOTION_MAX_PX or 4 * R >= min(int(H), int(W)):
        raise ValueError(f"motion_px must be an integer 1 .. {MOTION_MAX_PX} with 4 * motion_px < min(H, W) = {min(int(H), int(W))}, got {motion_px!r}")
    if 8 * max(int(H), int(W)) + 8 * (2 * R + 1) > 65536:
        raise ValueError(f"a side of {max(int(H), int(W))} pixels with motion_px = {R} is beyond the estimate's 64 KiB of LDS")
    return R


def _motion_gain(gain):
    g = _index_or_none(gain)
    if g is None or not 0 <= g <= 8:
        raise ValueError(f"motion_gain must be an integer 0 .. 8, got {gain!r}")
    return g


def _profile_sizes(B, H, W):
    if 765 * max(H, W) >= 2 ** 31 or H * W >= 2 ** 31:
        raise ValueError(f"a frame of {H} x {W} pixels is beyond int32 profiles")
    return (B, H + W)


# the profile pass's entry point by _frame_route's suffix: fs_frame_profiles + suffix ("_nv12" among them), but a planar frame of bytes is a key
_PROFILE_ENTRY = {"": "fs_frame_profiles", "_u8": "fs_key_profiles", "_hwc": "fs_frame_profiles_hwc"}


def _profiles(src, dtype, out):
    if not isinstance(src, _FRAME_TYPES) or src.dim() != 4 or src.shape[1] != 3 or src.numel() == 0 or src.dtype != dtype:
        raise ValueError(f"the frames must be a non-empty {dtype} (B,3,H,W), got {getattr(src, 'dtype', None)} {tuple(getattr(src, 'shape', ()))}")
    B, _, H, W = (int(v) for v in src.shape)
    suffix, strides = _frame_route(src, "the frames")
    shape = _profile_sizes(B, H, W)
    if out is None:
        out = torch.empty(shape, device=src.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or tuple(out.shape) != shape:
        raise ValueError(f"out must be int32 {shape}, got {out.dtype} {tuple(out.shape)}")
    hip.call(_PROFILE_ENTRY.get(suffix, "fs_frame_profiles" + suffix), *_frame_args(src, strides), hip.ptr(out), B, H, W)
    return out


def frame_profiles(img, out=None):
    """The integral projections of frames (fs_frame_profiles; no autograd; unpinned: the reference has no counterpart).  img (B,3,H,W)
    fp32.  Returns prof (B, H + W) int32: prof[b, :H] = the row sums and prof[b, H:] = the column sums of the luma code L = q_r + q_g +
    q_b, q the gate's pixel code (gate_tiles).  out: a (B, H + W) int32 tensor to write into."""
    return _profiles(img, torch.float32, out)


def key_profiles(key, out=None):
    """frame_profiles of 8-bit key frames (fs_key_profiles): key (B,3,H,W) uint8.  The profiles of a frame and of the key gate_commit
    made from it are equal.  A frame of bytes may also be an hwc view of interleaved bytes (byte_frame_layout; fs_frame_profiles_hwc), read
    where it lies; ValueError for any other non-contiguous layout."""
    return _profiles(key, torch.uint8, out)


def profile_shift(prof, prof_key, gstate, frame_size, motion_px, motion_gain=6, out=None):
    """The integer translation of every viewer against its key frame (fs_profile_shift; no autograd; unpinned).  prof, prof_key (B, H +
    W) int32 as frame_profiles / key_profiles make them; gstate (B,6) int64 the gate's; frame_size = (H, W); motion_px = R, the search
    range.  Per axis cost(s) = sum_{i=R}^{n-1-R} |P[i] - K[i - s]|; the least cost wins, ties to the smaller |s|, then to the negative s,
    and the shift is taken only if cost(s) * 8 <= cost(0) * motion_gain.  Returns shift (B,4) int64 = (dy, dx, cost_best, cost_zero),
    all 0 for a viewer without a record."""
    H, W = int(frame_size[0]), int(frame_size[1])
    R, gain = _motion_px(motion_px, H, W), _motion_gain(motion_gain)
    if not isinstance(prof, torch.Tensor) or prof.dim() != 2 or prof.dtype != torch.int32 or prof.shape[1] != H + W or prof.shape[0] < 1:
        raise ValueError(f"prof must be int32 (B, H + W) = (B, {H + W}), got {getattr(prof, 'dtype', None)} {tuple(getattr(prof, 'shape', ()))}")
    B = int(prof.shape[0])
    _profile_sizes(B, H, W)
    if prof_key.dtype != torch.int32 or prof_key.shape != prof.shape:
        raise ValueError(f"prof_key must be int32 {tuple(prof.shape)}, got {prof_key.dtype} {tuple(prof_key.shape)}")
    if gstate.dtype != torch.int64 or tuple(gstate.shape) != (B, 6):
        raise ValueError(f"gstate must be int64 ({B}, 6), got {gstate.dtype} {tuple(gstate.shape)}")
    if out is None:
        out = torch.empty(B, 4, device=prof.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, 4):
        raise ValueError(f"out must be int64 ({B}, 4), got {out.dtype} {tuple(out.shape)}")
    hip.call("fs_profile_shift", hip.ptr(prof), hip.ptr(prof_key), hip.ptr(gstate), hip.ptr(out), B, H, W, R, gain)
    return out


def state_shift_scratch(B, H, W, cap, device):
    """The scratch tensor state_shift wants for these sizes (fs_state_shift_scratch_ints ints)."""
    return torch.empty(hip.query("fs_state_shift_scratch_ints", int(B), int(H), int(W), int(cap)), device=device, dtype=torch.int32)


def _state_shift(dtype, img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch):
    if not isinstance(img, _FRAME_TYPES) or img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0 or img.dtype != dtype:
        raise ValueError(f"img must be a non-empty {'fp32' if dtype == torch.float32 else 'uint8'} (B,3,H,W), got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))}")
    B, _, H, W = (int(v) for v in img.shape)
    suffix, strides = _frame_route(img)
    _profile_sizes(B, H, W)
    P = (W + 31) // 32
    for name, k in (("key", key), ("key2", key2)):
        if k.dtype != torch.uint8 or k.shape != img.shape:
            raise ValueError(f"{name} must be uint8 {tuple(img.shape)}, got {k.dtype} {tuple(k.shape)}")
    for name, w in (("bits", bits), ("bits2", bits2)):
        if w.dtype != torch.int32 or tuple(w.shape) != (B, H, P):
            raise ValueError(f"{name} must be int32 {(B, H, P)}, got {w.dtype} {tuple(w.shape)}")
    if key2.data_ptr() == key.data_ptr() or bits2.data_ptr() == bits.data_ptr():
        raise ValueError("key2 and bits2 must be buffers of their own: the move does not read what it writes")
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[0] != B or counts.shape[1] < 1:
        raise ValueError(f"counts must be int32 ({B}, cap), got {counts.dtype} {tuple(counts.shape)}")
    cap = int(counts.shape[1])
    for name, t, tail in (("shift", shift, (4,)), ("gstate", gstate, (6,)), ("stats", stats, (6,)), ("mstate", mstate, (4,))):
        if t.dtype != torch.int64 or tuple(t.shape) != (B,) + tail:
            raise ValueError(f"{name} must be int64 {(B,) + tail}, got {t.dtype} {tuple(t.shape)}")
    if prof_key.dtype != torch.int32 or tuple(prof_key.shape) != (B, H + W):
        raise ValueError(f"prof_key must be int32 {(B, H + W)}, got {prof_key.dtype} {tuple(prof_key.shape)}")
    if motion is None:
        motion = torch.empty(B, 6, device=img.device, dtype=torch.int64)
    elif motion.dtype != torch.int64 or tuple(motion.shape) != (B, 6):
        raise ValueError(f"motion must be int64 ({B}, 6), got {motion.dtype} {tuple(motion.shape)}")
    need = hip.query("fs_state_shift_scratch_ints", B, H, W, cap)
    if scratch is None:
        scratch = torch.empty(need, device=img.device, dtype=torch.int32)
    elif scratch.dtype != torch.int32 or scratch.dim() != 1 or scratch.numel() < need:
        raise ValueError(f"scratch must be int32 with at least {need} entries, got {scratch.dtype} {tuple(scratch.shape)}")
    hip.call("fs_state_shift" + suffix, *_frame_args(img, strides), hip.ptr(shift), hip.ptr(key), hip.ptr(key2), hip.ptr(bits), hip.ptr(bits2), hip.ptr(gstate),
             hip.ptr(stats), hip.ptr(counts), hip.ptr(prof_key), hip.ptr(mstate), hip.ptr(motion), hip.ptr(scratch), B, H, W, cap)
    return motion


def state_shift(img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion=None, scratch=None):
    """Move the state of every viewer whose shift is not (0, 0), in place (fs_state_shift; no autograd; unpinned).  img (B,3,H,W) fp32
    the new frames; shift (B,4) int64 as profile_shift returns it; key (B,3,H,W) uint8 and bits (B,H,ceil(W/32)) int32 are moved by (dy,
    dx) -- the key's uncovered border is filled with q(img), the mask's with 0 -- through the spare buffers key2 and bits2 of the same
    shapes, whose contents afterwards are unspecified; the four gaze coordinates of gstate (B,6) int64 move by 16 * d, clamped; stats
    (B,6) int64 and counts (B,cap) int32 become mask_rle's of the moved bits; prof_key (B, H + W) int32 becomes key_profiles of the
    moved key; mstate (B,4) int64 = (dy_total, dx_total, moves, path) grows.  A still viewer's rows are not written.  Returns motion
    (B,6) int64 = (dy, dx, cost_best, cost_zero, dy_total, dx_total), written for every viewer.  scratch: state_shift_scratch(...)."""
    return _state_shift(torch.float32, img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch)


def state_shift_u8(img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion=None, scratch=None):
    """state_shift for frames of bytes (fs_state_shift_u8): img (B,3,H,W) uint8; the key's uncovered border is filled with the frame's
    byte.  Everything else as state_shift, and equal to it on img.float() / 255; the scratch is the same.  img is contiguous, or an hwc
    view of interleaved bytes (byte_frame_layout; fs_state_shift_hwc); ValueError for any other layout."""
    return _state_shift(torch.uint8, img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch)


def motion_commit(idx, prof, prof_key, mstate, frame_size):
    """What a step leaves behind for the motion estimate (fs_motion_commit; no autograd; unpinned), in place, after gate_commit: for the
    viewers of idx (int32 (n,) ascending, or None) prof_key (B, H + W) int32 <- prof, this step's frame_profiles, and mstate (B,4) int64
    <- 0.  frame_size = (H, W)."""
    H, W = int(frame_size[0]), int(frame_size[1])
    if not isinstance(prof, torch.Tensor) or prof.dim() != 2 or prof.dtype != torch.int32 or prof.shape[1] != H + W or prof.shape[0] < 1:
        raise ValueError(f"prof must be int32 (B, H + W) = (B, {H + W}), got {getattr(prof, 'dtype', None)} {tuple(getattr(prof, 'shape', ()))}")
    B = int(prof.shape[0])
    _profile_sizes(B, H, W)
    n = 0 if idx is None else int(idx.shape[0])
    if idx is not None and (idx.dtype != torch.int32 or idx.dim() != 1 or n > B):
        raise ValueError(f"idx must be int32 (n,) with n <= {B}, got {idx.dtype} {tuple(idx.shape)}")
    if prof_key.dtype != torch.int32 or prof_key.shape != prof.shape:
        raise ValueError(f"prof_key must be int32 {tuple(prof.shape)}, got {prof_key.dtype} {tuple(prof_key.shape)}")
    if mstate.dtype != torch.int64 or tuple(mstate.shape) != (B, 4):
        raise ValueError(f"mstate must be int64 ({B}, 4), got {mstate.dtype} {tuple(mstate.shape)}")
    if n:
        hip.call("fs_motion_commit", hip.ptr(idx), n, hip.ptr(prof), hip.ptr(prof_key), hip.ptr(mstate), B, H, W)


# ---- showing the record: the overlay pass (csrc/frame_overlay.hip) ----------------------------------------------------------------
OVERLAY_STYLE_COLS = 20                             # ints a style row (include/fovealseg.h "showing the record")
OVERLAY_MAX_PX = 16384                              # the kernel's cap on t, r, w and on a side


def _overlay_colour(name, v):
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 3:
        raise ValueError(f"{name} must be three integers (r, g, b) in 0 .. 255, got {v!r}")
    out = []
    for c in v:
        if isinstance(c, bool) or int(c) != c or not 0 <= int(c) <= 255:
            raise ValueError(f"{name} must be three integers (r, g, b) in 0 .. 255, got {v!r}")
        out.append(int(c))
    return out


def _overlay_int(name, v, hi):
    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer 0 .. {hi}, got {v!r}")
    return int(v)


def _int_ge_zero(name, v):
    if isinstance(v, bool) or int(v) != v or int(v) < 0:
        raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
    return int(v)


def overlay_style(tint=(0, 255, 0), alpha=128, outline=None, box=None, box_px=2, marker=None, marker_px=6, marker_width=None, dim=256,
                  cat=None, palette=None, device=None):
    """The style table of draw_instances / fs_frame_overlay: (S, 20) int32 on `device`, columns tint r g b, a, outline r g b, dim, box r g b,
    t, marker r g b, r, w, the outline flag, two reserved.  tint, and outline / box / marker where given, are (r, g, b) integers 0 .. 255;
    None switches the element off (its colour columns stay 0, and t, r or the flag 0).  alpha and dim are integers 0 .. 256: a mask pixel
    becomes (s * (256 - alpha) + tint * alpha + 128) >> 8, any other (s * dim + 128) >> 8.  box_px = t, the box's line width inward;
    marker_px = r, the gaze marker's radius, marker_width = w its ring width (None: a disc); all 0 .. 16384.  One row, for every viewer,
    unless cat (B,) int64 and palette (K,3) uint8 are given: then S = B and viewer b's tint is palette[cat[b]] (the given tint for a class
    outside the palette), looked up on cat's device without a host read.  ValueError for anything else."""
    row = [0] * OVERLAY_STYLE_COLS
    row[0:3] = _overlay_colour("tint", tint)
    row[3] = _overlay_int("alpha", alpha, 256)
    row[7] = _overlay_int("dim", dim, 256)
    if outline is not None:
        row[4:7] = _overlay_colour("outline", outline)
        row[17] = 1
    if box is not None:
        row[8:11] = _overlay_colour("box", box)
        row[11] = _overlay_int("box_px", box_px, OVERLAY_MAX_PX)
    if marker is not None:
        row[12:15] = _overlay_colour("marker", marker)
        row[15] = _overlay_int("marker_px", marker_px, OVERLAY_MAX_PX)
        row[16] = row[15] if marker_width is None else _overlay_int("marker_width", marker_width, OVERLAY_MAX_PX)
    if (cat is None) != (palette is None):
        raise ValueError("cat and palette go together: a tint a viewer by class needs both")
    if cat is None:
        return torch.tensor([row], dtype=torch.int32, device=device)
    if not isinstance(cat, torch.Tensor) or cat.dim() != 1 or cat.dtype != torch.int64 or cat.numel() == 0:
        raise ValueError(f"cat must be a non-empty int64 (B,), got {getattr(cat, 'dtype', None)} {tuple(getattr(cat, 'shape', ()))}")
    pal = torch.as_tensor(palette)
    if pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < 1 or pal.dtype != torch.uint8:
        raise ValueError(f"palette must be uint8 (K, 3), got {pal.dtype} {tuple(pal.shape)}")
    dev = cat.device if device is None else torch.device(device)
    cat, pal = cat.to(dev), pal.to(dev)
    K = int(pal.shape[0])
    style = torch.tensor([row], dtype=torch.int32, device=dev).repeat(int(cat.shape[0]), 1)
    inside = (cat >= 0) & (cat < K)
    looked = pal[cat.clamp(0, K - 1)].to(torch.int32)
    style[:, 0:3] = torch.where(inside[:, None], looked, style[:, 0:3])
    return style


def byte_frame_dest(out, shape=None):
    """(ob, oy, ox) of a uint8 (B,3,H,W) tensor the overlay pass can write, from byte_frame_layout's rule: (3 * H * W, W, 1) for a
    contiguous one; (sb, sy, sx) for a view of interleaved bytes (hwc.permute(0, 3, 1, 2) of a (B,H,W,3) buffer, rgba.permute(0, 3, 1,
    2)[:, :3] of a (B,H,W,4) one whose fourth byte is then written as 255, padded rows, a crop).  ValueError for any other tensor, another
    shape than `shape`, and one image expanded over several viewers (sb == 0 with B > 1: the viewers' pictures would overwrite each other)."""
    layout = byte_frame_layout(out)
    if layout is None or (shape is not None and tuple(out.shape) != tuple(shape)):
        raise ValueError(f"out must be a uint8 {tuple(shape) if shape is not None else '(B,3,H,W)'}, contiguous or a view of interleaved (B,H,W,3) / "
                         f"(B,H,W,4) bytes (ops.byte_frame_layout), got {getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))} with "
                         f"strides {tuple(out.stride()) if isinstance(out, torch.Tensor) else None}")
    B, _, H, W = (int(v) for v in out.shape)
    if layout[0] == "planar":
        return 3 * H * W, W, 1
    _, sb, sy, sx = layout
    if B > 1 and sb == 0:
        raise ValueError("out is one image expanded over several viewers: every viewer needs bytes of its own")
    return sb, sy, sx


def _dest_args(out, dest):
    if not out.is_cuda:
        raise hip.HipLibraryError("fovealseg kernels need device tensors (got a CPU tensor); there is no CPU path")
    return (out.data_ptr(),) + tuple(dest)


def overlay_band(bits, Ws, d, er=None, scratch=None, band=None):
    """The outline band of draw_instances: bits & ~E_d(bits), E_d fs_mask_erode's, with no host read.  er, band (like bits) and scratch
    (fs_mask_erode_scratch_ints int32) are made where not given; the bits at x >= Ws of the band are unspecified (the overlay pass reads
    none of them).  Returns (band, er, scratch)."""
    d = _morph_d(d)
    B, Hs = int(bits.shape[0]), int(bits.shape[1])
    if er is None:
        er = torch.empty_like(bits, memory_format=torch.contiguous_format)
    if band is None:
        band = torch.empty_like(bits, memory_format=torch.contiguous_format)
    if scratch is None:
        scratch = torch.empty(max(1, hip.query("fs_mask_erode_scratch_ints", B, Hs, Ws, d)), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_erode", hip.ptr(bits), hip.ptr(er), hip.ptr(scratch), B, Hs, Ws, d)
    torch.bitwise_not(er, out=er)
    torch.bitwise_and(bits, er, out=band)
    return band, er, scratch


def _live_arg(live, B, dev):
    """(pointer, stride in elements) of the nullable live flags: an int64 (B,) tensor on the device, contiguous or a column of a matrix."""
    if live is None:
        return None, 1
    if not isinstance(live, torch.Tensor) or live.dtype != torch.int64 or tuple(live.shape) != (B,) or live.device != dev:
        raise ValueError(f"live must be int64 ({B},) on {dev}, got {getattr(live, 'dtype', None)} {tuple(getattr(live, 'shape', ()))}")
    stride = int(live.stride(0)) if B > 1 else 1
    if stride < 1:
        raise ValueError(f"live must have a positive stride, got {stride}")
    return live.data_ptr(), stride


def draw_instances(img, bits, stats=None, focus=None, style=None, outline_px=0, out=None, live=None, band=None):
    """The record drawn onto the frame, in one launch (fs_frame_overlay / _u8 / _hwc; no autograd; unpinned: the reference draws on the
    host).  img (B,3,H,W) as the serving entry points take it, on the device: fp32 (its pixel code q(v) = rint(clamp(v, 0, 1) * 255) is what
    is drawn on), contiguous uint8, or a uint8 view of interleaved bytes (byte_frame_layout), read where it lies; any other layout is
    copied.  bits (B,H,ceil(W/32)) int32, the record's mask; stats (B,6) int64, the record's, for the box; focus (B,2), for the gaze
    marker; a None switches its element off.  style: overlay_style's table, (1,20) or (B,20) int32 (None: its defaults).  outline_px = d >
    0 makes the outline band bits & ~E_d(bits) first (fs_mask_erode; no host read) unless `band` brings it; the style's outline colour
    shows it.  live: None, or int64 (B,) flags (a column of a matrix will do): where 0, the viewer's mask, outline and box count as empty.
    out: a uint8 (B,3,H,W) tensor to write, contiguous or an interleaved view (byte_frame_dest: an RGBA view gets alpha 255); None: a new
    contiguous one.  out may be img itself for a frame of bytes.  The rule per pixel, first that holds: marker, box, outline, tint, dim
    (include/fovealseg.h).  Returns out."""
    if not isinstance(img, _FRAME_TYPES) or img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0 or img.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"img must be a non-empty fp32 or uint8 (B,3,H,W), got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))}")
    B, _, H, W = (int(v) for v in img.shape)
    if max(H, W) > OVERLAY_MAX_PX:
        raise ValueError(f"a frame of {H} x {W} pixels has a side above {OVERLAY_MAX_PX}")
    dev = img.device
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or tuple(bits.shape) != (B, H, (W + 31) // 32):
        raise ValueError(f"bits must be int32 {(B, H, (W + 31) // 32)}, got {getattr(bits, 'dtype', None)} {tuple(getattr(bits, 'shape', ()))}")
    if stats is not None and (stats.dtype != torch.int64 or tuple(stats.shape) != (B, 6)):
        raise ValueError(f"stats must be int64 ({B}, 6), got {stats.dtype} {tuple(stats.shape)}")
    if style is None:
        style = overlay_style(device=dev)
    if not isinstance(style, torch.Tensor) or style.dtype != torch.int32 or style.dim() != 2 or style.shape[1] != OVERLAY_STYLE_COLS or \
            int(style.shape[0]) not in (1, B):
        raise ValueError(f"style must be int32 (1, {OVERLAY_STYLE_COLS}) or ({B}, {OVERLAY_STYLE_COLS}) (ops.overlay_style), got "
                         f"{getattr(style, 'dtype', None)} {tuple(getattr(style, 'shape', ()))}")
    f = None if focus is None else _focus_arg(focus, B, dev)
    live_ptr, live_stride = _live_arg(live, B, dev)
    outline_px = _int_ge_zero("outline_px", outline_px)
    if isinstance(img, Nv12Frame):
        pass                                            # read where it lies
    elif img.dtype == torch.uint8 and byte_frame_layout(img) is None or img.dtype == torch.float32 and not img.is_contiguous():
        img = img.contiguous()
    if out is None:
        out = torch.empty(B, 3, H, W, device=dev, dtype=torch.uint8)
    dest = byte_frame_dest(out, (B, 3, H, W))
    bits = bits.contiguous()
    if band is None and int(outline_px) > 0:
        band = overlay_band(bits, W, int(outline_px))[0]
    elif band is not None and (band.dtype != torch.int32 or band.shape != bits.shape):
        raise ValueError(f"band must be int32 {tuple(bits.shape)}, got {band.dtype} {tuple(band.shape)}")
    suffix, strides = _frame_route(img)
    hip.call("fs_frame_overlay" + suffix, *_frame_args(img, strides), hip.ptr(bits), hip.ptr(band), hip.ptr(stats if stats is None else stats.contiguous()),
             hip.ptr(f), live_ptr, live_stride, hip.ptr(style.contiguous()), int(style.shape[0]), *_dest_args(out, dest), B, H, W)
    return out


def color_encode(labels, palette, out=None):
    """A class map as colours (fs_color_encode; utils.py:207-221 colorEncode, mode RGB, on the device): labels (B,H,W) or (H,W) int64,
    predict()'s map; palette (K,3) uint8.  out (B,3,H,W) uint8 as draw_instances takes it (None: a new contiguous one) = palette[label],
    (0, 0, 0) for a label < 0 or >= K -- the reference skips negative labels and would raise on one >= K.  Returns out."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() not in (2, 3) or labels.numel() == 0:
        raise ValueError(f"labels must be a non-empty int64 (B,H,W) or (H,W), got {getattr(labels, 'dtype', None)} {tuple(getattr(labels, 'shape', ()))}")
    if labels.dim() == 2:
        labels = labels[None]
    B, H, W = (int(v) for v in labels.shape)
    if max(H, W) > OVERLAY_MAX_PX:
        raise ValueError(f"a map of {H} x {W} pixels has a side above {OVERLAY_MAX_PX}")
    pal = torch.as_tensor(palette)
    if pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < 1 or pal.dtype != torch.uint8:
        raise ValueError(f"palette must be uint8 (K, 3), got {pal.dtype} {tuple(pal.shape)}")
    pal = pal.to(labels.device).contiguous()
    if out is None:
        out = torch.empty(B, 3, H, W, device=labels.device, dtype=torch.uint8)
    dest = byte_frame_dest(out, (B, 3, H, W))
    hip.call("fs_color_encode", hip.ptr(labels.contiguous()), hip.ptr(pal), *_dest_args(out, dest), B, H, W, int(pal.shape[0]))
    return out


def _hd_q(q):
    if isinstance(q, bool) or int(q) != q or not 1 <= int(q) <= 100:
        raise ValueError(f"the Hausdorff percentile must be an integer 1 .. 100, got {q!r}")
    return int(q)


def unwarp_count(cls, m, grid, y, cls_label, dia_factor=None, frame=True, areas=False, return_labels=False, hd_q=None):
    """The checks, allocations and call that unwarp_accuracy, unwarp_trimap and unwarp_class_areas share; models.py's evaluate() calls
    it directly.  Internal to the package: the documented ops are those three.  dia_factor=None: no trimap.  hd_q (None, or 1 .. 100):
    the surface-distance statistics of surface_hd, prediction foreground (class != K-1) against label foreground.  The entry point is
    the smallest that counts what is asked for: fs_unwarp_hd with hd_q, else fs_unwarp_class_areas with areas, else fs_unwarp_trimap
    with a trimap, else fs_unwarp_accuracy.  Returns the six-tuple (counts, acc, areas, trim, labels, hd) in this order, None where not
    asked for."""
    with_trim = dia_factor is not None
    D, fr = _trimap_args(dia_factor, frame) if with_trim else (0, 0)
    q = _hd_q(hd_q) if hd_q is not None else None
    B, K = cls.shape
    _, h, w, _ = grid.shape
    if tuple(m.shape) != (B, h, w):
        raise ValueError(f"m {tuple(m.shape)} must be (B, h, w) = {(B, h, w)}: the mask at the grid's resolution")
    if y.dim() == 4 and y.shape[1] == 1:
        y = y[:, 0]
    if y.dim() != 3 or y.shape[0] != B:
        raise ValueError(f"y {tuple(y.shape)} must be (B, Hs, Ws) or (B, 1, Hs, Ws) with B = {B}")
    Hs, Ws = int(y.shape[1]), int(y.shape[2])
    if cls_label.dim() == 2 and cls_label.shape[1] == 1:
        cls_label = cls_label[:, 0]
    if tuple(cls_label.shape) != (B,):
        raise ValueError(f"cls_label {tuple(cls_label.shape)} must be (B,) or (B, 1) with B = {B}")
    dev = cls.device
    counts = torch.empty(B, 6, device=dev, dtype=torch.int64)
    acc = torch.empty(4, device=dev, dtype=torch.float32)
    area = torch.empty(B, 3, K, 3, device=dev, dtype=torch.int64) if areas else None
    trim = torch.empty(B, D + 1, 3, device=dev, dtype=torch.int64) if with_trim else None
    labels = torch.empty(B, Hs, Ws, device=dev, dtype=torch.int64) if return_labels else None
    hd = torch.empty(B, 4, device=dev, dtype=torch.int64) if q is not None else None
    # (entry point, the dimensions its scratch query takes, its outputs after acc, its arguments after the dimensions)
    if q is not None:
        name, qdims, outs, tail = "fs_unwarp_hd", (B, K, h, w, Hs, Ws), (area, trim, labels, hd), (D, fr, q)
    elif areas:
        name, qdims, outs, tail = "fs_unwarp_class_areas", (B, K, h, w, Hs, Ws), (area, trim, labels), (D, fr)
    elif with_trim:
        name, qdims, outs, tail = "fs_unwarp_trimap", (B, h, w, Hs, Ws), (trim, labels), (D, fr)
    else:
        name, qdims, outs, tail = "fs_unwarp_accuracy", (B, h, w, Hs, Ws), (labels,), ()
    scratch = torch.empty(hip.query(name + "_scratch_ints", *qdims), device=dev, dtype=torch.int32)
    hip.call(name, hip.ptr(cls.contiguous()), hip.ptr(m.contiguous()), hip.ptr(grid.contiguous()), hip.ptr(y.float().contiguous()),
             hip.ptr(cls_label.long().contiguous()), hip.ptr(counts), hip.ptr(acc), *(hip.ptr(t) for t in outs), hip.ptr(scratch),
             B, K, h, w, Hs, Ws, *tail)
    return counts, acc, area, trim, labels, hd


def unwarp_accuracy(cls, m, grid, y, cls_label, return_labels=False):
    """The four full-resolution accuracies of MODEL.upsample for the C1 head (no autograd), without the (B,K,Hs,Ws) prediction, a class
    map or a ground-truth tensor: the predicted class of a pixel is `unwarp_labels`'s, its ground truth `t = y.long()`,
    `t * cls_label + (1 - t) * (K - 1)`, and the gather pass counts instead of storing (fs_unwarp_accuracy).  cls (B,K), m (B,h,w),
    grid (B,h,w,2) as for unwarp_labels; y (B,Hs,Ws) or (B,1,Hs,Ws) the label mask at the output size; cls_label (B,) or (B,1).
    Returns (counts (B,6) int64 = cls_fg, bin_fg, union_fg, cls_bg, bin_bg, union_bg per image, acc (4,) fp32 = acc, acc_bin_fg,
    acc_cls_fbg, acc_bin_fbg as SegLoss's out[3:7]) and, with return_labels, the (B,Hs,Ws) int64 class map of unwarp_labels."""
    counts, acc, _, _, labels, _ = unwarp_count(cls, m, grid, y, cls_label, return_labels=return_labels)
    return (counts, acc, labels) if return_labels else (counts, acc)


def _trimap_args(dia_factor, frame):
    D = int(dia_factor)
    if not 0 <= D <= 7:
        raise ValueError(f"dia_factor must be 0 .. 7 (band widths 1 .. 2**dia_factor), got {dia_factor}")
    return D, 1 if frame else 0


def trimap_bands(y, dia_factor=5, frame=True):
    """Which trimap band every pixel of the label mask lies in (eval.py:41-67; VAL.trimap_dia_factor): uint8 (B,Hs,Ws), the smallest
    i <= dia_factor such that the pixel is within 2**i city-block steps of the label's boundary, 255 if none, so that band i of the
    reference (FIND_EDGES, then binary_dilation(iterations=2**i)) is `bands <= i` (fs_trimap_bands).  y (B,Hs,Ws) or (B,1,Hs,Ws), read
    as t = y.long().  A boundary seed is a background pixel (t == 0) with a foreground 8-neighbour; frame=True also seeds every
    background pixel of the outer one-pixel ring, as PIL's filter does -- the reference bit for bit -- and frame=False is the
    neighbour rule alone, pixels outside the image being background.  No autograd."""
    D, fr = _trimap_args(dia_factor, frame)
    if y.dim() == 4 and y.shape[1] == 1:
        y = y[:, 0]
    if y.dim() != 3 or y.numel() == 0:
        raise ValueError(f"y {tuple(y.shape)} must be a non-empty (B, Hs, Ws) or (B, 1, Hs, Ws)")
    B, Hs, Ws = (int(v) for v in y.shape)
    band = torch.empty(B, Hs, Ws, device=y.device, dtype=torch.uint8)
    scratch = torch.empty(hip.query("fs_trimap_bands_scratch_ints", B, Hs, Ws), device=y.device, dtype=torch.int32)
    hip.call("fs_trimap_bands", hip.ptr(y.float().contiguous()), hip.ptr(band), hip.ptr(scratch), B, Hs, Ws, D, fr)
    return band


def unwarp_trimap(cls, m, grid, y, cls_label, dia_factor=5, frame=True, return_labels=False):
    """unwarp_accuracy with the trimap boundary accuracies of eval.py:41-67 counted in the same gather pass (fs_unwarp_trimap).
    Arguments and checks are unwarp_accuracy's; dia_factor / frame are trimap_bands'.  Returns (counts, acc, trim[, labels]): counts,
    acc and labels are unwarp_accuracy's bit for bit, trim (B, dia_factor + 1, 3) int64 holds per image and band width 2**i the number of
    pixels in the band, of those whose predicted class equals the ground truth (the reference's acc_sum) and of those that agree with
    it on foreground versus background.  An image without a boundary seed (a constant label with frame=False, an all-foreground one
    with frame=True) has all-zero rows: the reference divides 0 by 0 there, trimap_from_counts and train.TrimapMeter leave it out."""
    if dia_factor is None:
        raise TypeError("unwarp_trimap needs dia_factor (0 .. 7); unwarp_accuracy is the op without a trimap")
    counts, acc, _, trim, labels, _ = unwarp_count(cls, m, grid, y, cls_label, dia_factor, frame, return_labels=return_labels)
    return (counts, acc, trim, labels) if return_labels else (counts, acc, trim)


def trimap_from_counts(trim):
    """(B, D+1, 3) trim counters (unwarp_trimap's, on any device) -> (B, D+1, 2) fp64: per image and band width the class accuracy
    cls_ok / (total + 1e-10) -- the reference's Python-float quotient, eval.py:64 -- and the foreground / background accuracy
    bin_ok / (total + 1e-10).  An empty band gives 0; `trim[..., 0] > 0` tells which images count (see unwarp_trimap)."""
    if trim.dim() != 3 or trim.shape[2] != 3:
        raise ValueError(f"trim must be (B, D+1, 3), got {tuple(trim.shape)}")
    t = trim.to(torch.float64)
    return t[..., 1:] / (t[..., :1] + 1e-10)


def unwarp_class_areas(cls, m, grid, y, cls_label, dia_factor=None, frame=True, return_labels=False):
    """unwarp_accuracy with the per-class areas of the reference's evaluation summary (eval.py:218-257,313-322; utils.intersectionAndUnion,
    utils.py:289-317) counted in the same gather pass (fs_unwarp_class_areas).  Arguments and checks are unwarp_trimap's; dia_factor=None
    leaves the trimap out.  Returns (counts, acc, areas[, trim][, labels]): counts, acc, trim and labels are unwarp_accuracy's /
    unwarp_trimap's bit for bit; areas (B, 3, K, 3) int64 holds per image, space and class (inter, pred, lab), the union being
    pred + lab - inter.  Space 0 is the prediction at full resolution (unwarp_labels against the ground truth), space 1 the sampling
    ceiling -- the label after the sampler and the nearest un-warp against itself (VAL.y_sampled_reverse, models/models_instance.py:909-918):
    every pixel takes grid_sample_label's value of the grid point that feeds it -- and space 2 the prediction in the sampled space
    (PredAssemble(cls, m).argmax(1) against the sampled ground truth).  A cls_label outside 0 .. K-1 has no lab / inter row."""
    counts, acc, areas, trim, labels, _ = unwarp_count(cls, m, grid, y, cls_label, dia_factor, frame, areas=True, return_labels=return_labels)
    return (counts, acc, areas) + ((trim,) if trim is not None else ()) + ((labels,) if return_labels else ())


def class_scores_from_areas(areas):
    """(..., K, 3) class areas (unwarp_class_areas', on any device; summed over a dataset or not) -> (iou, dice), each (..., K) fp64:
    iou = inter / (union + 1e-10) and dice = 2 * inter / (union + inter + 1e-10) with union = pred + lab - inter -- the reference's
    expressions (eval.py:252, 313-315).  A class with an empty union scores 0."""
    if areas.dim() < 2 or areas.shape[-1] != 3:
        raise ValueError(f"areas must be (..., K, 3), got {tuple(areas.shape)}")
    a = areas.to(torch.float64)
    inter, union = a[..., 0], a[..., 1] + a[..., 2] - a[..., 0]
    return inter / (union + 1e-10), 2 * inter / (union + inter + 1e-10)


def surface_hd(a, b, q=95):
    """The q-th percentile of the Hausdorff distances between the borders of two masks (HD95 at q = 95; VAL.hd95), as the integers it is
    made of (fs_surface_hd; no autograd).  a, b (B,H,W) or (H,W), bool or uint8 (non-zero = foreground), on the device; H, W <= 16384.
    The border of a mask is its foreground with a background 4-neighbour, outside the image counting as background; every border pixel
    of either mask takes the squared distance to the nearest border pixel of the other, and the two sets are pooled.  Returns hd (B,4)
    int64 = (n_a, n_b, d2_lo, d2_hi): the border sizes and the pooled squared distances at the two ranks np.percentile interpolates
    between; d2 = -1 where a border is empty.  hd_from_stats makes the distance.  This is the published 2-D definition; the
    reference's utils.hd95 flattens both masks before it erodes them and returns something else."""
    q = _hd_q(q)
    if a.dim() == 2 and b.dim() == 2:
        a, b = a[None], b[None]
    if a.dim() != 3 or a.shape != b.shape or a.numel() == 0:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} must be two non-empty (B, H, W) masks of one shape")
    if a.dtype not in (torch.bool, torch.uint8) or b.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"masks must be bool or uint8, got {a.dtype} and {b.dtype}")
    B, Hs, Ws = (int(v) for v in a.shape)
    fg = ((a != 0).to(torch.uint8) | ((b != 0).to(torch.uint8) << 1)).contiguous()
    hd = torch.empty(B, 4, device=a.device, dtype=torch.int64)
    scratch = torch.empty(hip.query("fs_surface_hd_scratch_ints", B, Hs, Ws), device=a.device, dtype=torch.int32)
    hip.call("fs_surface_hd", hip.ptr(fg), hip.ptr(hd), hip.ptr(scratch), B, Hs, Ws, q)
    return hd


def hd_from_stats(hd, q=95):
    """(B,4) surface statistics (surface_hd's / evaluate(hausdorff=q)'s, on any device) -> (B,) fp64: np.percentile(distances, q) =
    sqrt(d2_lo) + (sqrt(d2_hi) - sqrt(d2_lo)) * frac with frac = (q (n-1) mod 100) / 100, n = n_a + n_b; NaN where a border is empty
    (the reference raises there).  q must be the q the statistics were made with.  Plain torch."""
    q = _hd_q(q)
    if hd.dim() != 2 or hd.shape[1] != 4:
        raise ValueError(f"hd must be (B, 4), got {tuple(hd.shape)}")
    hd = hd.to(torch.int64)
    n = hd[:, 0] + hd[:, 1]
    frac = ((q * (n - 1)) % 100).to(torch.float64) / 100.0
    empty = (hd[:, 0] <= 0) | (hd[:, 1] <= 0) | (hd[:, 2] < 0)
    lo, hi = hd[:, 2].clamp(min=0).to(torch.float64).sqrt(), hd[:, 3].clamp(min=0).to(torch.float64).sqrt()
    out = lo + (hi - lo) * frac
    return torch.where(empty, torch.full_like(out, float("nan")), out)


def image_accuracies_from_counts(counts):
    """(B,6) counts -> (B,4) fp32 per-image acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg (models/models.py:378-474): plain torch, any device."""
    c = counts.to(torch.float32)
    ufg, ubg = c[:, 2] + 1e-10, c[:, 5] + 1e-10
    cls_fg, bin_fg, cls_bg, bin_bg = c[:, 0] / ufg, c[:, 1] / ufg, c[:, 3] / ubg, c[:, 4] / ubg
    return torch.stack([cls_fg, bin_fg, cls_fg * 0.5 + cls_bg * 0.5, bin_fg * 0.5 + bin_bg * 0.5], 1)


def accuracies_from_counts(counts):
    """(B,6) counts (unwarp_accuracy's, on any device) -> (4,) fp32: the batch's four accuracies, the mean over its images of the fp32
    per-image quotients -- fs_unwarp_accuracy's and SegLoss's arithmetic in plain torch."""
    if counts.dim() != 2 or counts.shape[1] != 6:
        raise ValueError(f"counts must be (B, 6), got {tuple(counts.shape)}")
    return (image_accuracies_from_counts(counts).double().sum(0) / counts.shape[0]).float()


# ----------------------------------------------------------------------------------------------
# SegFormer pieces (tokens = NHWC rows)
# ----------------------------------------------------------------------------------------------
class LayerNorm(Function):
    """nn.LayerNorm over the last dimension."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        C = x.shape[-1]
        M = x.numel() // C
        y = torch.empty_like(x)
        mean = torch.empty(M, device=x.device, dtype=torch.float32)
        rstd = torch.empty(M, device=x.device, dtype=torch.float32)
        hip.call("fs_layernorm_fwd", hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), M, C, float(eps))
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.beta_ref = beta
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, mean, rstd = ctx.saved_tensors
        C = x.shape[-1]
        dx = torch.empty_like(x)
        tg, tb = _direct_grad_target(gamma), _direct_grad_target(ctx.beta_ref)
        direct = tg is not None and tb is not None
        dgamma = tg if direct else torch.empty_like(gamma)
        dbeta = tb if direct else torch.empty_like(gamma)
        M = x.numel() // C
        scratch = torch.empty(hip.query("fs_layernorm_bwd_scratch_floats", M, C), device=x.device, dtype=torch.float32)
        hip.call("fs_layernorm_bwd", hip.ptr(g.contiguous()), hip.ptr(x), hip.ptr(gamma), hip.ptr(mean), hip.ptr(rstd), hip.ptr(dx),
                 hip.ptr(dgamma), hip.ptr(dbeta), M, C, 1 if direct else 0, hip.ptr(scratch))
        if direct:
            dgamma = dbeta = None
        return dx, dgamma, dbeta, None


class LayerNormFan(Function):
    """(LayerNorm(x), x): the pre-norm fan-out of a transformer block -- x feeds the normalisation AND the residual add -- as one autograd
    node, so that both gradients of x arrive together and the LayerNorm backward pass adds the residual's while it writes dx
    (fs_layernorm_bwd_add) instead of the autograd engine running an add pass over the activation (104 per configs[3] step)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        C = x.shape[-1]
        M = x.numel() // C
        y = torch.empty_like(x)
        mean = torch.empty(M, device=x.device, dtype=torch.float32)
        rstd = torch.empty(M, device=x.device, dtype=torch.float32)
        hip.call("fs_layernorm_fwd", hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), M, C, float(eps))
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.beta_ref = beta
        ctx.set_materialize_grads(False)          # an unused output's gradient arrives as None, not as a tensor of zeros
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, g, g_skip):
        x, gamma, mean, rstd = ctx.saved_tensors
        if g is None:
            return g_skip, None, None, None
        C = x.shape[-1]
        dx = torch.empty_like(x)
        tg, tb = _direct_grad_target(gamma), _direct_grad_target(ctx.beta_ref)
        direct = tg is not None and tb is not None
        dgamma = tg if direct else torch.empty_like(gamma)
        dbeta = tb if direct else torch.empty_like(gamma)
        M = x.numel() // C
        scratch = torch.empty(hip.query("fs_layernorm_bwd_scratch_floats", M, C), device=x.device, dtype=torch.float32)
        hip.call("fs_layernorm_bwd_add", hip.ptr(g.contiguous()), hip.ptr(x), hip.ptr(gamma), hip.ptr(mean), hip.ptr(rstd),
                 hip.ptr(g_skip.contiguous()) if g_skip is not None else None, hip.ptr(dx), hip.ptr(dgamma), hip.ptr(dbeta), M, C,
                 1 if direct else 0, hip.ptr(scratch))
        if direct:
            dgamma = dbeta = None
        return dx, dgamma, dbeta, None


class Gelu(Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        hip.call("fs_gelu_fwd", hip.ptr(x), hip.ptr(y), x.numel())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        hip.call("fs_gelu_bwd", hip.ptr(g.contiguous()), hip.ptr(x), hip.ptr(dx), x.numel())
        return dx


class Unfold(Function):
    """(B,H,W,C) -> (1, B*Ho*Wo, 1, Kp): k x k patches as rows, element order (r, s, c), zero-padded to Kp columns; backward folds."""

    @staticmethod
    def forward(ctx, x, k, stride, pad, kp):
        B, H, W, C = x.shape
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        col = torch.empty(1, B * Ho * Wo, 1, kp, device=x.device, dtype=torch.float32)
        hip.call("fs_unfold", hip.ptr(x), hip.ptr(col), B, H, W, C, k, stride, pad, Ho, Wo, kp)
        ctx.geom = (B, H, W, C, k, stride, pad, Ho, Wo, kp)
        return col

    @staticmethod
    def backward(ctx, g):
        B, H, W, C, k, stride, pad, Ho, Wo, kp = ctx.geom
        dx = torch.empty(B, H, W, C, device=g.device, dtype=torch.float32)
        hip.call("fs_fold", hip.ptr(g.contiguous()), hip.ptr(dx), B, H, W, C, k, stride, pad, Ho, Wo, kp)
        return dx, None, None, None, None


UNFOLD_BIG_FILTERS = os.environ.get("FS_UNFOLD_CONV", "1") != "0"
PATCHIFY_DIRECT = os.environ.get("FS_PATCHIFY_DIRECT", "0") == "1"


def conv_bias_any(x, w, bias, stride, pad):
    """ConvBias, with filters of more than 32 taps (which the aligned split-precision kernels do not take: they would run on the generic fp32
    kernels) unfolded into patch rows and computed as one linear layer.  The weight's RSCK storage [r][s][c][k] IS the (k*k*C, Cout) matrix
    of that layer: a view, no copy, and its gradient lands in the same storage."""
    cout, cin, r, s = w.shape
    # ... and so are filters whose stride equals their size (the 2x2 / 4x4 sequence-reduction convs of the Mix-Transformer): their patches
    # do not overlap, the unfold is a pure permutation, and the alternative is one single-tap launch per filter tap and pass (configs[3]:
    # 312 conv_igemm_split launches per step, 13.7 ms; round 4)
    patchify = r > 1 and stride == r and pad == 0
    # (FS_PATCHIFY_DIRECT=1: leave the <= 9-tap ones -- the 2x2 reduction of the Mix-Transformer's 40-block stage -- to the library's own
    # stride >= filter route instead: gathered-row GEMM forward, one scattered-row GEMM per tap for bwd-data, bwd-weight on gathered rows;
    # no unfold / fold passes, no patch matrix kept.  Measured on configs[3], B = 16, alternating on one box: 198.9 / 198.4 ms per step
    # unfolded, 200.4 / 200.4 direct (-0.9 %, 1.2 GB less memory): four quarter-size GEMM launches cost more than one GEMM + a 73 us fold.  Off.)
    if patchify and PATCHIFY_DIRECT and r * s <= 9 and cin % 64 == 0 and cout % 64 == 0:
        patchify = False
    if (not UNFOLD_BIG_FILTERS or r != s or (r * s <= 32 and not patchify) or hip.get_conv_precision() != "bf16x3" or cout % 4 or cout < 16):
        return ConvBias.apply(x, w, bias, stride, pad)
    B, H, W, _ = x.shape
    Ho, Wo = _out_hw(H, W, r, s, stride, pad)
    kk = r * s * cin
    kp = max(16, (kk + 3) // 4 * 4)
    as_matrix = lambda t: t.permute(2, 3, 1, 0).reshape(1, 1, kk, cout).permute(3, 2, 0, 1)      # logical (Cout, kk, 1, 1) over the same RSCK storage
    w2 = param_view(w, as_matrix) if kp == kk else as_matrix(w)
    if kp != kk:
        w2 = PadWeightChannels.apply(w2, kp)
    y = ConvBias.apply(Unfold.apply(x, r, stride, pad, kp), w2, bias, 1, 0)
    return y.view(B, Ho, Wo, cout)


class GeluDropout(Function):
    """dropout_p(gelu(x)) in one pass each way (MixFFN's activation + hidden dropout); the mask is Dropout's for the same key."""

    @staticmethod
    def forward(ctx, x, p, key):
        y = torch.empty_like(x)
        hip.call("fs_gelu_dropout_fwd", hip.ptr(x), hip.ptr(y), x.numel(), float(p), int(key))
        ctx.save_for_backward(x)
        ctx.pk = (float(p), int(key))
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        p, key = ctx.pk
        dx = torch.empty_like(x)
        hip.call("fs_gelu_dropout_bwd", hip.ptr(g.contiguous()), hip.ptr(x), hip.ptr(dx), x.numel(), p, key)
        return dx, None, None


DWCONV_BIAS_FUSED = os.environ.get("FS_DWCONV_BIAS_FUSED", "1") != "0"      # A/B switch: 0 = separate column-sum pass


class DwConv3(Function):
    """Depthwise Conv2d(C,C,3,1,1,groups=C) + bias on NHWC; w logical (C,1,3,3)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        B, H, W, C = x.shape
        y = torch.empty_like(x)
        hip.call("fs_dwconv3_fwd", hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(y), B, H, W, C, 0)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        B, H, W, C = x.shape
        g = g.contiguous()
        dx = torch.empty_like(x)
        hip.call("fs_dwconv3_fwd", hip.ptr(g), hip.ptr(w), None, hip.ptr(dx), B, H, W, C, 1)
        tgt = _direct_grad_target(w)
        tgt = tgt if (tgt is not None and tgt.is_contiguous()) else None
        dw = tgt if tgt is not None else torch.empty_like(w)
        lanes = hip.query("fs_dwconv3_wgrad_lanes", B, H, W, C)
        if ctx.has_bias and not DWCONV_BIAS_FUSED:
            ws = torch.empty(lanes * 9 * C, device=x.device, dtype=torch.float32)
            hip.call("fs_dwconv3_bwd_weight", hip.ptr(x), hip.ptr(g), hip.ptr(dw), hip.ptr(ws), B, H, W, C, 1 if tgt is not None else 0)
            return dx, (None if tgt is not None else dw), colsum(g, C, into=_direct_grad_target(ctx.bias_ref))
        if ctx.has_bias:          # the bias gradient rides in the weight-gradient launches, which read dy once anyway
            btgt = _direct_grad_target(ctx.bias_ref)
            db = btgt if btgt is not None else torch.empty(C, device=x.device, dtype=torch.float32)
            ws = torch.empty(lanes * 10 * C, device=x.device, dtype=torch.float32)
            hip.call("fs_dwconv3_bwd_weight_bias", hip.ptr(x), hip.ptr(g), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), B, H, W, C,
                     1 if tgt is not None else 0, 1 if btgt is not None else 0)
            return dx, (None if tgt is not None else dw), (None if btgt is not None else db)
        ws = torch.empty(lanes * 9 * C, device=x.device, dtype=torch.float32)
        hip.call("fs_dwconv3_bwd_weight", hip.ptr(x), hip.ptr(g), hip.ptr(dw), hip.ptr(ws), B, H, W, C, 1 if tgt is not None else 0)
        if tgt is not None:
            dw = None
        return dx, dw, None


LINEAR_RESIDUAL = os.environ.get("FS_LINEAR_RESIDUAL", "1") != "0"      # A/B switch: 0 = linear layer, then a residual + DropPath pass


class LinearResidual(Function):
    """out = res + DropPath_p2(Dropout_p(x W^T + b)): the linear layer that ends a residual branch of a transformer block with the residual add
    in the GEMM epilogue (fs_conv2d_fwd_residual), and ONE mask pass over the gradient in the backward (fs_droppath_dropout_bwd) where the
    separate nodes ran two (DropPath's, then the Dropout's).  x (..., Cin), res (B, ..., Cout); samples = res.shape[0]."""

    @staticmethod
    def forward(ctx, x, w, bias, res, drop_p, drop_key, dp_p, dp_key):
        cout, cin = w.shape[0], w.shape[1]
        rows = x.numel() // cin
        p = ConvProblem.linear(rows, cin, cout)
        x4 = x.reshape(p.x_shape)
        rps = rows // res.shape[0]
        ws, ws_bytes, packed = _pack_for(w, x.device, p, 0)
        out = torch.empty_like(res)
        _launch_conv(packed, "conv_affine", p.flops, "fs_conv2d_fwd_residual", hip.ptr(x4), hip.ptr(rsck(w)), hip.ptr(bias),
                     hip.ptr(res), hip.ptr(out), *p, float(drop_p), int(drop_key), float(dp_p), int(dp_key), rps, hip.ptr(ws), ws_bytes, None)
        ctx.save_for_backward(x4, w)
        ctx.cfg = (float(drop_p), int(drop_key), float(dp_p), int(dp_key), rps, bias is not None, tuple(x.shape))
        ctx.bias_ref = bias
        ctx.w_via = getattr(w, "_fs_grad_via", None)
        return out

    @staticmethod
    def backward(ctx, g):
        x4, w = ctx.saved_tensors
        drop_p, drop_key, dp_p, dp_key, rps, has_bias, x_shape = ctx.cfg
        cout, cin = w.shape[0], w.shape[1]
        g = g.contiguous()
        rows = x4.shape[1]
        if drop_p > 0.0 or dp_p > 0.0:
            dy = torch.empty_like(g)
            hip.call("fs_droppath_dropout_bwd", hip.ptr(g), hip.ptr(dy), g.numel(), rps * cout, dp_p, dp_key, drop_p, drop_key)
        else:
            dy = g
        dy4 = dy.view(1, rows, 1, cout)
        dx = conv2d_bwd_data(dy4, w, x4.shape, 1, 0).view(x_shape) if ctx.needs_input_grad[0] else None
        if ctx.w_via is not None and getattr(w, "_fs_grad_via", None) is None:
            w._fs_grad_via = ctx.w_via
        dw, db = _linear_param_grads(x4, dy4, w, ctx.bias_ref if has_bias else None)
        return dx, dw, db, g, None, None, None, None


def _linear_param_grads(x4, dy4, w, bias):
    """(dw, db) of a 1x1 / linear layer as autograd wants them: None where the kernel added straight into the parameter's arena slice."""
    tgt = _direct_grad_target(w)
    cout, cin = w.shape[0], w.shape[1]
    rows = dy4.numel() // cout
    if bias is not None and hip.linear_bwd_weight_bias_ok(rows, cin, cout):
        btgt = _direct_grad_target(bias)
        dw = rsck(tgt) if tgt is not None else torch.empty(1, 1, cin, cout, device=x4.device, dtype=torch.float32)
        db = btgt if btgt is not None else torch.empty(cout, device=x4.device, dtype=torch.float32)
        lws_bytes = hip.query("fs_linear_bwd_weight_bias_ws_bytes", cin, cout)      # deterministic mode only
        lws = torch.empty(lws_bytes, device=x4.device, dtype=torch.uint8) if lws_bytes else None
        _launch("conv_wgrad", 2.0 * rows * cout * cin, "fs_linear_bwd_weight_bias", hip.ptr(x4), hip.ptr(dy4), hip.ptr(dw), hip.ptr(db),
                rows, cin, cout, 1 if tgt is not None else 0, 1 if btgt is not None else 0, hip.ptr(lws), lws_bytes)
        return (None if tgt is not None else dw.permute(3, 2, 0, 1)), (None if btgt is not None else db)
    dw = conv2d_bwd_weight(x4, dy4, w.shape, 1, 0, out=tgt, accumulate=tgt is not None)
    db = colsum(dy4, cout, into=_direct_grad_target(bias)) if bias is not None else None
    return (None if tgt is not None else dw), db


def linear_residual(x, w, bias, res, drop_p, drop_key, dp_p, dp_key):
    """res + DropPath(Dropout(linear(x))): fused where the 1x1 GEMM kernel runs the layer (bf16x3 / f16x2, >= 128 rows per sample), else None
    (the caller composes ConvBias + ResidualDropPath)."""
    if not (LINEAR_RESIDUAL and x.is_cuda and hip.get_conv_precision() != "f32"):
        return None
    cout, cin = w.shape[0], w.shape[1]
    rows = x.numel() // cin
    if rows % res.shape[0] or rows * max(cin, cout) * 4 >= MAX_TENSOR_BYTES:
        return None
    p = ConvProblem.linear(rows, cin, cout)
    if not p.residual_ok(rows // res.shape[0], p.ws_bytes(0)):
        return None
    return LinearResidual.apply(x, w, bias, res.contiguous(), drop_p, drop_key, dp_p, dp_key)


class ResidualDropPath(Function):
    """out = x + DropPath_p(y): per-sample keep from the hash (p = 0: plain residual add)."""

    @staticmethod
    def forward(ctx, x, y, p, key):
        out = torch.empty_like(x)
        per = x.numel() // x.shape[0]
        hip.call("fs_residual_droppath", hip.ptr(x), hip.ptr(y), hip.ptr(out), x.numel(), per, float(p), int(key))
        ctx.cfg = (float(p), int(key), per)
        return out

    @staticmethod
    def backward(ctx, g):
        p, key, per = ctx.cfg
        g = g.contiguous()
        if p == 0.0:
            return g, g, None, None
        dy = torch.empty_like(g)
        hip.call("fs_residual_droppath", None, hip.ptr(g), hip.ptr(dy), g.numel(), per, p, key)
        return g, dy, None, None


ATTN_SPLIT = os.environ.get("FS_ATTN_SPLIT", "1") != "0"      # kernel A/B: 0 keeps the exact-fp32 MFMA attention kernels in every mode


class Attention(Function):
    """softmax(q k^T / sqrt(64)) (dropout p) v per head on the matrix cores; q (B,N,C), k/v (B,Nk,C), C = heads*64, any Nk."""

    @staticmethod
    def forward(ctx, q, k, v, heads, p, key, grad_enabled=None):
        # grad_enabled: the grad mode of the CALL SITE (ops.attention records it) -- inside Function.forward grad mode is always off, and
        # ctx.needs_input_grad mirrors requires_grad of the inputs even under no_grad; None (a direct .apply) = decide on needs_input_grad
        will_backward = any(ctx.needs_input_grad[:3]) and (grad_enabled is None or grad_enabled)
        B, N, C = q.shape
        Nk = k.shape[1]
        assert C == heads * 64, "head_dim must be 64"
        o = torch.empty_like(q)
        lse = torch.empty(B * heads * N, device=q.device, dtype=torch.float32)
        mask = None
        split = ATTN_SPLIT and hip.get_conv_precision() == "bf16x3"
        if split:
            # the headline arithmetic (24-bit operands as three bf16 planes, fp32 accumulation) on the attention products as well
            nb = hip.attention_split_ws_bytes(B, Nk, heads)
            ws = torch.empty(nb, device=q.device, dtype=torch.uint8)
            if p > 0 and will_backward:
                # one keep bit per (query, key), left by the forward so that the three backward kernels do not hash every element again
                mask = torch.empty(hip.query("fs_attention_mask_words", B, N, Nk, heads), device=q.device, dtype=torch.int32)
            _launch("attn_fwd", 4.0 * B * heads * N * Nk * 64, "fs_attention_fwd_split", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(o),
                    hip.ptr(lse), hip.ptr(mask) if mask is not None else None, hip.ptr(ws), nb, B, N, Nk, heads, 0.125, float(p), int(key))
        else:
            _launch("attn_fwd", 4.0 * B * heads * N * Nk * 64, "fs_attention_fwd", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(o), hip.ptr(lse),
                    B, N, Nk, heads, 0.125, float(p), int(key))
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.cfg = (heads, float(p), int(key))
        ctx.keep_mask = mask
        ctx.split = split          # the backward takes the kernel family (and workspace contract) the forward prepared for, whatever the mode is by then
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, lse = ctx.saved_tensors
        heads, p, key = ctx.cfg
        B, N, C = q.shape
        Nk = k.shape[1]
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        scratch = torch.empty(B * heads * N, device=q.device, dtype=torch.float32)
        if ctx.split:
            nb = hip.attention_split_ws_bytes(B, Nk, heads, backward=True)
            ws = torch.empty(nb, device=q.device, dtype=torch.uint8)
            mask = ctx.keep_mask
            _launch("attn_bwd", 14.0 * B * heads * N * Nk * 64, "fs_attention_bwd_split", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(o),
                    hip.ptr(go.contiguous()), hip.ptr(lse), hip.ptr(mask) if mask is not None else None, hip.ptr(dq), hip.ptr(dk), hip.ptr(dv),
                    hip.ptr(scratch), hip.ptr(ws), nb, B, N, Nk, heads, 0.125, p, key)
        else:
            _launch("attn_bwd", 14.0 * B * heads * N * Nk * 64, "fs_attention_bwd", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(o),
                    hip.ptr(go.contiguous()), hip.ptr(lse), hip.ptr(dq), hip.ptr(dk), hip.ptr(dv), hip.ptr(scratch), B, N, Nk, heads, 0.125, p, key)
        return dq, dk, dv, None, None, None, None


def attention(q, k, v, heads, p, key):
    """Attention.apply with the call site's grad mode (decides whether the forward leaves the dropout keep words for the backward)."""
    return Attention.apply(q, k, v, heads, p, key, torch.is_grad_enabled())
