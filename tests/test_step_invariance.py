"""The DeepLab and SegFormer training steps held to the contract of hip.set_deterministic: in deterministic mode a training step is
bit-reproducible, and neither the stream a gradient is produced on nor the node its sum is formed in changes a bit of it.

What is under test is host code, not a kernel: the weight-gradient side stream of ops.py (fork per layer, rotate / retire / reap of the
kept tensors, the engine's final-callback join), the fan-out / stash records, deeplab.py's block fan-out and segformer.py's pre-norm
fan-out -- the places where a missing dependency or a dropped addend raises nothing and only moves the numbers by less than any oracle
tolerance.  Every comparison of parts 1-3 is torch.equal; part 4 (the C1 head whose conv alias is zero-padded) keeps the bounds of
test_hip_kernels.py::test_c1_classification_gradient_joins_the_mask_branch_epilogue.  Run on the MI355X box:  python -m pytest tests -m gpu"""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import fovealseg  # noqa: E402
from fovealseg import deeplab, hip, modules, ops, segformer, train  # noqa: E402

DEV = "cuda"
CONFIGS = ["deeplab", "segformer"]


def _cfg(name):
    cfg = fovealseg.lvis50_cfg()
    cfg.MODEL.arch_encoder = name
    if name == "segformer":
        cfg.MODEL.fc_dim = 1024
        cfg.TRAIN.task_input_size = (160, 160)
    return cfg


@contextlib.contextmanager
def _deterministic(precision=None):
    """Deterministic mode (and, if named, a conv precision mode) for the block; both restored whatever happens inside."""
    assert not hip.get_deterministic()
    hip.set_deterministic(True)
    if precision is not None:
        hip.set_conv_precision(precision)
    try:
        yield
    finally:
        hip.set_deterministic(False)
        if precision is not None:
            hip.set_conv_precision(hip.default_conv_precision())


@contextlib.contextmanager
def _switched(*settings):
    """settings = (module, attribute name, value) triples: set for the block, restored in `finally`."""
    saved = [(obj, name, getattr(obj, name)) for obj, name, _ in settings]
    try:
        for obj, name, value in settings:
            setattr(obj, name, value)
        yield
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)


@pytest.fixture(scope="module")
def built():
    """built(name) -> (module, optimisers, batch) of a configuration for the forward + backward comparisons (parts 2 and 3): those never
    step an optimiser, so one module per configuration, built at its first use, serves them all (a train-mode forward only moves the
    BatchNorm running statistics, which a train-mode forward does not read)."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg = _cfg(name)
            dev = torch.device("cuda", 0)
            module, nets = train.build_module(cfg, device=dev)
            module.train()
            cache[name] = (module, train.create_optimizers(nets, cfg), train.synthetic_batch(2, 256, 256, seed=11, device=dev))
        return cache[name]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _fwd_bwd(module, optimizers, batch, read_now=False):
    """Zeroed gradient arenas, one forward, one backward.  -> (loss, arenas after a device synchronise, arenas cloned on the current
    stream straight after backward() -- nothing in between, no synchronise, no explicit join -- or None, side streams still busy)."""
    X, Fp, Y, cls = batch
    for opt in optimizers:
        opt.zero_grad()
    ops.DropoutState.seed, ops.DropoutState.step = 77, 1
    feed = {"img_data": X[:, :3], "seg_label": Y, "focus_point": Fp, "cls_label": cls}
    outs = module(feed, epoch=1, cur_iter=0)
    outs[0].mean().backward()
    now = [o.flat.grad.clone() for o in optimizers] if read_now else None
    busy = dict(ops._WGRAD_SIDE_BUSY)
    torch.cuda.synchronize()
    return float(outs[0].detach()), [o.flat.grad.clone() for o in optimizers], now, busy


def _first_difference(optimizers, got, want):
    """Where two sets of arenas differ, parameter by parameter (the message of a failed comparison): arena index, parameter index, shape."""
    out = []
    for k, (opt, a, b) in enumerate(zip(optimizers, got, want)):
        for i, (p, o) in enumerate(zip(opt.flat.params, opt.flat.offsets)):
            sa, sb = a[o:o + p.numel()], b[o:o + p.numel()]
            if not torch.equal(sa, sb):
                out.append((k, i, tuple(p.shape), float((sa - sb).abs().max()), float(sb.abs().max())))
                if len(out) >= 6:
                    return out
    return out


# ----------------------------------------------------------------------------------------------------------------
# 1. the whole step, twice
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("config", CONFIGS)
def test_two_deterministic_train_steps_repeat_bit_for_bit(config, precision):
    """Two train_steps (forward, backward, four Adam steps, then again on the updated weights) on a freshly built module, done twice: the
    losses and the four parameter arenas are bit-identical.  Per conv precision mode, because the three modes take different bwd-weight
    routes.  This is run(group=False) of test_ddp_gloo.py::test_train_step_through_one_rank_rccl_group for the two other encoders."""
    cfg = _cfg(config)
    dev = torch.device("cuda", 0)
    batch = train.synthetic_batch(2, 256, 256, seed=3, device=dev)

    def run():
        module, nets = train.build_module(cfg, device=dev)
        module.train()
        optimizers = train.create_optimizers(nets, cfg)
        ops.DropoutState.seed, ops.DropoutState.step = 9, 0
        losses = [float(train.train_step(module, optimizers, batch, cfg, epoch=1, cur_iter=it)[0].detach()) for it in range(2)]
        torch.cuda.synchronize()
        return losses, [op.flat.data.clone() for op in optimizers], optimizers

    with _deterministic(precision):
        la, pa, opts = run()
        lb, pb, _ = run()
    print(f"\n[step-invariance] {config} {precision}: losses {la} / {lb}")
    assert all(l == l for l in la)                    # (finite: NaN == NaN would be False below anyway, this names the cause)
    assert la == lb, (la, lb)
    for k, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), (f"parameter arena {k} differs between two deterministic runs", _first_difference(opts, pb, pa))


# ----------------------------------------------------------------------------------------------------------------
# 2. stream placement
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIGS)
def test_stream_placement_does_not_change_a_gradient_bit(built, name):
    """One forward + backward in deterministic mode and the library's default precision with (a) the default WGRAD_SIDE_FLOPS, twice,
    (b) WGRAD_SIDE_FLOPS = 0: every weight gradient on the launching stream, (c) the branch / fuse / stage streams of modules.py off:
    the four gradient arenas are bit-identical across all four, in (a) the arenas read on the current stream straight after
    backward() are already the arenas after a device synchronise, and no side stream is left un-joined.
    The side launches are counted (hip.set_stream_override with a stream): in (a) DeepLab sends more than _WGRAD_ROTATE of them, so the
    kept lists rotate, retire and are reaped inside one backward; SegFormer sends those of the C1 head, classification ResNet, saliency
    and compress nets; in (b) there are none."""
    module, optimizers, batch = built(name)
    launches = []
    real = hip.set_stream_override

    def counting(handle):
        if handle is not None:
            launches.append(handle)
        return real(handle)

    def run(read_now):
        del launches[:]
        loss, grads, now, busy = _fwd_bwd(module, optimizers, batch, read_now)
        return loss, grads, now, busy, len(launches)

    off = ((modules, "PARALLEL_BRANCHES", False), (modules, "PARALLEL_FUSE", False), (modules, "STREAM_DEPS", False))
    hip.set_stream_override = counting
    try:
        with _deterministic():
            assert ops.WGRAD_SIDE_FLOPS > 1e9 and ops.TIMER is None
            a1 = run(True)
            a2 = run(True)
            with _switched((ops, "WGRAD_SIDE_FLOPS", 0.0)):
                b = run(False)
            with _switched(*off):
                c = run(False)
    finally:
        hip.set_stream_override = real
    print(f"\n[step-invariance] {name}: side launches (a) {a1[4]} / {a2[4]}, (b) {b[4]}, (c) {c[4]}; rotate at {ops._WGRAD_ROTATE}; loss {a1[0]}")
    # the test is about what it claims
    if name == "deeplab":
        assert a1[4] > ops._WGRAD_ROTATE and a2[4] == a1[4], (a1[4], a2[4])
    else:
        assert a1[4] > 0 and a2[4] == a1[4], (a1[4], a2[4])
    assert b[4] == 0 and c[4] == a1[4], (b[4], c[4])
    for r in (a1, a2, b, c):
        assert not r[3], "a side stream was still un-joined when backward() returned"
    assert a1[0] == a1[0] and a1[0] == a2[0] == b[0] == c[0], (a1[0], a2[0], b[0], c[0])
    for r in (a1, a2):
        for k, (x, y) in enumerate(zip(r[2], r[1])):
            assert torch.equal(x, y), (f"arena {k} read right after backward() differs from the arena after a device synchronise",
                                       _first_difference(optimizers, r[2], r[1]))
    for tag, r in (("(a) repeated", a2), ("(b) one stream", b), ("(c) module streams off", c)):
        for k, (x, y) in enumerate(zip(r[1], a1[1])):
            assert torch.equal(x, y), (f"gradient arena {k}: {tag} differs from (a)", _first_difference(optimizers, r[1], a1[1]))
    assert all(float(g.abs().max()) > 0 for g in a1[1])           # four arenas, all reached


# ----------------------------------------------------------------------------------------------------------------
# 3. switches that move WHERE a sum is formed, not its operands or their order
# ----------------------------------------------------------------------------------------------------------------
# (configuration, switch, settings held on BOTH sides, parameters whose own slice is exempt).  Decided from the code:
#
# ops.WGRAD_FIRST -- the order of a layer's bwd-weight and bwd-data launches.  Same two kernels on the same operands, disjoint outputs.
#
# deeplab.BLOCK_FANOUT -- on: the block input's two gradients (conv1's dx, conv3's dres) are added by FanOut.backward, a + b in one fp32
#   add per element (fs_add_n / fs_add_n_bnsum), and fs_add_n_bnsum forms the BatchNorm-backward sums of the block in front with the
#   row / column walk and slab layout of fs_bn_bwd_partial.  off: the engine adds the same two tensors (one ATen add, fp32 addition
#   commutes) and that layer runs fs_bn_bwd_partial on the sum.  conv1's dx comes from the bwd-data kernel without (on) or with (off) the
#   sum epilogue, which writes the same dX (test_bwd_data_epilogue_sums_on_the_pointwise_and_stride2_kernels: bit for bit without addend).
#   No residual gradient is absorbed by a bwd-data epilogue in a three-conv bottleneck (conv3's input is not the fan-out's conv alias).
#
# ops.FANOUT -- with FUSE_BN_BWD_SUMS off on both sides it decides only whether fs_add_n or the engine's ATen add forms the two-operand
#   sums (DeepLab blocks, C1's `feat`): a + b either way.  With FUSE_BN_BWD_SUMS on (the default) it ALSO decides whether the
#   BatchNorm-backward sums come from a bwd-data epilogue (per conv tile) or from fs_bn_bwd_partial (per row block), and whether C1's
#   classification gradient is added inside the 3x3 bwd-data kernel: other fp32 orders, no bound of its own in the suite -> not compared.
#
# segformer.LN_FAN -- with LINEAR_RESIDUAL off on both sides the forward is the same (LayerNorm, ConvBias, ResidualDropPath) and the switch
#   decides only where the block input's two gradients meet: fs_layernorm_bwd_add rounds the LayerNorm's dx and then adds the residual's
#   gradient (`d = rs * (...); d += addend`, two statements, one fp32 add per element), the engine adds the same two tensors.  dgamma /
#   dbeta come from the same kernel.  With LINEAR_RESIDUAL on, LN_FAN also moves the residual add of the FORWARD into the GEMM epilogue
#   (another rounding: test_linear_with_the_residual_in_its_epilogue allows 2e-6) -> not compared.
#
# ops.DWCONV_BIAS_FUSED -- the depthwise conv's bias gradient as column sums inside the weight-gradient launches (one partial per lane
#   of fs_dwconv3_wgrad_lanes) or by fs_colsum (one partial per row block): other fp32 order for THOSE sums, no bound in the suite, so
#   the dwconv biases' own slices are exempt.  A bias gradient feeds nothing else in a backward pass: the loss and every other element
#   of the four arenas are compared bit for bit.
SWITCHES = [
    ("deeplab", (ops, "WGRAD_FIRST"), (), None),
    ("deeplab", (deeplab, "BLOCK_FANOUT"), (), None),
    ("deeplab", (ops, "FANOUT"), ((ops, "FUSE_BN_BWD_SUMS", False),), None),
    ("segformer", (segformer, "LN_FAN"), ((ops, "LINEAR_RESIDUAL", False),), None),
    ("segformer", (ops, "DWCONV_BIAS_FUSED"), (), "dwconv.dwconv.bias"),
]


@pytest.mark.parametrize("case", SWITCHES, ids=[f"{c[0]}-{c[1][1]}" for c in SWITCHES])
def test_route_switches_that_keep_the_additions_keep_every_bit(built, case):
    """Forward + backward in deterministic mode with the switch on and off: loss and gradient arenas bit-identical (see the table above for
    why each pair performs the same fp32 additions in the same order, and which are left out because they do not)."""
    name, (owner, switch), held, exempt = case
    module, optimizers, batch = built(name)
    assert getattr(owner, switch) is True
    got = {}
    with _deterministic():
        with _switched(*held):
            for value in (True, False):
                with _switched((owner, switch, value)):
                    got[value] = _fwd_bwd(module, optimizers, batch)
    ops.reset_step_state()
    on, off = got[True], got[False]
    print(f"\n[step-invariance] {name} {switch}: loss on {on[0]} off {off[0]}")
    assert on[0] == on[0] and on[0] == off[0], (on[0], off[0])
    named = {id(p): n for n, p in module.named_parameters()}
    exempted = 0
    for k, (opt, a, b) in enumerate(zip(optimizers, on[1], off[1])):
        if exempt is not None:
            a, b = a.clone(), b.clone()
            for p, o in zip(opt.flat.params, opt.flat.offsets):
                if named[id(p)].endswith(exempt):
                    assert float(b[o:o + p.numel()].abs().max()) > 0          # the exempt gradients exist
                    a[o:o + p.numel()] = 0
                    b[o:o + p.numel()] = 0
                    exempted += 1
        assert torch.equal(a, b), (f"gradient arena {k} changes with {switch}", _first_difference(optimizers, on[1], off[1]))
    assert (exempted > 0) == (exempt is not None)


# ----------------------------------------------------------------------------------------------------------------
# 4. the C1 head when its 3x3 conv reads a zero-padded copy of `feat`
# ----------------------------------------------------------------------------------------------------------------
def _relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_c1_gradient_is_complete_when_the_conv_alias_is_padded(precision):
    """MODEL.fc_dim is a user setting.  With fc_dim % 4 != 0 in a split-precision mode modules.conv_bn_act pads the mask branch's input
    (ops.pad_in_channels), so the 3x3 conv no longer reads the fan-out's alias itself.  The classification branch's gradient must still
    reach `feat`: dfeat and every parameter gradient with C1_STASH on equal those with the two readers left to autograd (bounds of
    test_c1_classification_gradient_joins_the_mask_branch_epilogue: 1e-6 / 1e-5; a missing branch is an O(1) error), nothing is left
    in PENDING_RES after backward(), and the next forward's reset_step_state has nothing to raise."""
    fc_dim, B, hw = 66, 2, 20
    hip.set_conv_precision(precision)
    keep = modules.C1_STASH
    try:
        torch.manual_seed(5)
        dec = modules.C1(num_class=51, fc_dim=fc_dim).to(DEV)
        dec.train(True)
        gg = torch.Generator().manual_seed(99)
        feat = (torch.randn(B, hw, hw, fc_dim, generator=gg) * 0.5).to(DEV)
        cot = None
        got = {}
        for stash in (True, False):
            modules.C1_STASH = stash
            ops.reset_step_state()
            fd = (feat * 1.0).requires_grad_(True)
            h = fd * 1.0                                  # a non-leaf, like the encoder's output
            pred = dec.forward_nhwc(h)
            if cot is None:
                cot = (torch.randn(pred.shape, generator=gg) * 0.01).to(DEV)
            dec.zero_grad()
            pred.backward(cot)
            torch.cuda.synchronize()
            left = sorted(ops.PENDING_RES)
            ops.PENDING_RES.clear()                       # (so that a failure here does not fail the next test's first forward instead)
            assert not left, f"C1_STASH={stash}: gradients of fan-outs {left} were stashed and never added"
            ops.reset_step_state()                        # what the next forward runs: must not raise
            got[stash] = (fd.grad.clone(), {k: q.grad.detach().clone() for k, q in dec.named_parameters() if q.grad is not None})
        # the classification branch's share of dfeat is not small: leaving it out could not hide inside the bound
        e_feat = _relerr(got[True][0], got[False][0])
        print(f"\n[step-invariance] C1 fc_dim {fc_dim} {precision}: dfeat relerr {e_feat:.3e}")
        assert e_feat <= 1e-6, e_feat
        assert set(got[True][1]) == set(got[False][1])
        for k, v in got[False][1].items():
            assert _relerr(got[True][1][k], v) <= 1e-5 or float(v.abs().max()) == 0.0, k
    finally:
        modules.C1_STASH = keep
        ops.PENDING_RES.clear()
        hip.set_conv_precision(hip.default_conv_precision())
