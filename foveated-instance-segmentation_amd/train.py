"""Training-step plumbing around DeformSegmentationModule.

Mirrors train_deform_semantic.py: `ddp_setup` (:45-55), the per-step order of `train()` (:74-129:
zero_grad -> adjust_learning_rate -> forward -> loss.mean().backward() -> 4 optimiser steps),
`create_optimizers` (:260-290, Adam x4 over encoder/decoder/saliency/compress) and
`adjust_learning_rate` (:302-350).

MI355X-first differences (DESIGN.md "Multi-GPU"): each optimiser owns ONE flat fp32 arena holding all
its parameters (params are views into it, conv weights keep RSCK strides), one flat gradient arena
and flat Adam moments, so a step is one fused HIP kernel and the data-parallel exchange is one RCCL
all-reduce per arena (4 per step, 522 MB total) instead of DDP's ~20 x 25 MB buckets.
"""
import math
import os

import torch
import torch.distributed as dist

from . import hip

_ALIGN = 4   # elements; keeps every parameter 16-byte aligned for the float4 kernels


class FlatParams:
    """Re-homes a list of parameters into one flat arena (+ a matching gradient arena)."""

    def __init__(self, params):
        self.params = [p for p in params]
        assert self.params, "empty parameter list"
        dev = self.params[0].device
        self._epoch = [0]          # bumped whenever the arena is rewritten behind the parameters' version counters (refresh_amax)
        offs, n = [], 0
        for p in self.params:
            assert p.dtype == torch.float32
            offs.append(n)
            n += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = n
        self.data = torch.zeros(n, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(n, device=dev, dtype=torch.float32)
        for p, o in zip(self.params, offs):
            size, stride = tuple(p.shape), tuple(p.stride())
            dense = self._dense_strides(p)
            view = self.data.as_strided(size, dense, o)
            view.copy_(p.data)
            p.data = view
            p.grad = self.grad.as_strided(size, dense, o)
            p._fs_grad_home = (self.grad, o)          # ops._direct_grad_target: kernels may add into this slice while .grad points at it
            p._fs_epoch = self._epoch                  # ops._pack_for: a weight pack of p is valid while this word has not moved
            del stride
        self.offsets = offs
        # max|w| bits per parameter, kept current by refresh_amax(): the f16x2 conv kernels scale the weights by it
        self.amax = torch.zeros(len(self.params), device=dev, dtype=torch.int32)
        self._offs_dev = torch.tensor(offs, dtype=torch.int64, device=dev)
        self._sizes_dev = torch.tensor([p.numel() for p in self.params], dtype=torch.int64, device=dev)
        self._amax_words = [self.amax[i:i + 1] for i in range(len(self.params))]
        self.refresh_amax()

    def refresh_amax(self):
        """One launch: max|w| of every parameter of the arena.  Parameters remember their word and the torch version counter
        at this moment (ops.weight_amax drops the word if the tensor is modified through torch afterwards)."""
        self._epoch[0] += 1
        if not self.data.is_cuda:
            return
        hip.call("fs_weight_amax_segments", hip.ptr(self.data), hip.ptr(self._offs_dev), hip.ptr(self._sizes_dev), len(self.params),
                 hip.ptr(self.amax))
        for i, p in enumerate(self.params):
            p._fs_amax = (self._amax_words[i], p._version)

    @staticmethod
    def _dense_strides(p):
        """Strides of p if it is non-overlapping and dense (any permutation), else contiguous ones."""
        size, stride = p.shape, p.stride()
        order = sorted(range(p.dim()), key=lambda d: (stride[d], size[d]))
        expect, ok = 1, True
        for d in order:
            if size[d] == 1:
                continue
            if stride[d] != expect:
                ok = False
                break
            expect *= size[d]
        if ok:
            return tuple(stride)
        return tuple(torch.empty(size).stride())

    def zero_grad(self):
        self.grad.zero_()
        for p, o in zip(self.params, self.offsets):     # autograd may have re-pointed .grad
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self.grad.as_strided(tuple(p.shape), tuple(p.stride()), o)

    def adopt_grads(self):
        """Copy gradients that live outside the arena (a caller followed the reference loop's `module.zero_grad()`, so autograd
        allocated fresh `.grad` tensors) into the arena and re-point `.grad` at the views."""
        for p, o in zip(self.params, self.offsets):
            view = self.grad.as_strided(tuple(p.shape), tuple(p.stride()), o)
            if p.grad is None:
                view.zero_()
            elif p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                view.copy_(p.grad)
            p.grad = view


class FlatAdam:
    """torch.optim.Adam(weight_decay) semantics over a FlatParams arena, one fused HIP launch."""

    def __init__(self, params, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, **group_extras):
        self.flat = FlatParams(params)
        self.m = torch.zeros_like(self.flat.data)
        self.v = torch.zeros_like(self.flat.data)
        self.t = 0
        self.grad_scale = 1.0
        g = dict(params=self.flat.params, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)
        g.update(group_extras)
        self.param_groups = [g]

    def zero_grad(self, set_to_none=False):
        from . import ops
        ops.join_wgrad_streams()          # (a backward whose small-layer weight gradients went to the side stream, never stepped)
        self.flat.zero_grad()

    def check_grads_in_arena(self):
        """Every parameter's .grad must BE its slice of the gradient arena: the fused Adam kernel reads the arena only.  A caller
        that dropped the views (module.zero_grad() sets .grad = None, autograd then allocates fresh tensors) would otherwise
        step with zero gradients and weight decay alone, silently."""
        base = self.flat.grad.data_ptr()
        for p, o in zip(self.flat.params, self.flat.offsets):
            if p.grad is None or p.grad.data_ptr() != base + 4 * o:
                raise RuntimeError("FlatAdam: a parameter's .grad is not its gradient-arena view (use optimizer.zero_grad(), not "
                                   "module.zero_grad(); or call flat.adopt_grads() to copy stray gradients in)")

    def step(self):
        g = self.param_groups[0]
        self.check_grads_in_arena()
        self.t += 1
        from .ops import _launch, join_wgrad_streams
        join_wgrad_streams()              # the arena is complete only when the side-stream weight gradients have landed
        _launch("fe_adam", 28.0 * self.flat.numel, "fs_adam_step", hip.ptr(self.flat.data), hip.ptr(self.flat.grad), hip.ptr(self.m), hip.ptr(self.v),
                self.flat.numel, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                float(g["weight_decay"]), self.t, float(self.grad_scale))
        self.flat.refresh_amax()

    def state_dict(self):
        return dict(t=self.t, m=self.m, v=self.v, param_groups=[{k: v for k, v in self.param_groups[0].items() if k != "params"}])

    def load_state_dict(self, sd):
        self.t = sd["t"]
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])


def create_optimizers(nets, cfg):
    """train_deform_semantic.py:260-290 -- returns (encoder, decoder, saliency, compress) optimisers."""
    net_encoder, net_decoder, crit, net_saliency, net_compress = nets
    if cfg.TRAIN.optim.lower() != "adam":
        raise NotImplementedError("only TRAIN.optim='adam' is usable in the reference (the sgd branch returns undefined names)")
    T = cfg.TRAIN
    mk = lambda net, mult, zoom: FlatAdam(list(net.parameters()), lr=T.lr_encoder, weight_decay=T.weight_decay,  # noqa: E731
                                          lr_mult=mult, zoom=zoom)
    return (mk(net_encoder, T.lr_mult_encoder, False), mk(net_decoder, T.lr_mult_decoder, False),
            mk(net_saliency, T.lr_mult_saliency, True), mk(net_compress, T.lr_mult_compress, True))


def adjust_learning_rate(optimizers, cur_iter, cfg, epoch=None):
    """train_deform_semantic.py:302-350 under scale_by_iter=False, fov_scale_lr=''."""
    T = cfg.TRAIN
    scale_running_lr = (1.0 - float(cur_iter) / T.max_iters) ** T.lr_pow
    T.running_lr_encoder = T.lr_encoder * scale_running_lr
    T.running_lr_decoder = T.lr_decoder * scale_running_lr
    T.running_lr_foveater = T.lr_foveater * scale_running_lr
    base_lr = 0.1
    n_pre = T.deform_pretrain
    if T.scale_by_iter:
        raise NotImplementedError("TRAIN.scale_by_iter=True is not on the default path")
    lr_idx = epoch
    if T.deform_pretrain_bol or lr_idx < n_pre:
        lr_class = base_lr * 0.1 ** (lr_idx // n_pre)
        lr_zoom = base_lr * 0.1 ** (lr_idx // n_pre)
    else:
        lr_class = base_lr * 0.1 ** ((lr_idx - n_pre) // n_pre)
        lr_zoom = base_lr * 0.1 ** (lr_idx // n_pre)
    if T.fix_deform_aft_pretrain and T.fix_deform_start_epoch <= epoch <= T.fix_deform_end_epoch:
        lr_zoom = 0.0
    for opt in optimizers:
        for group in opt.param_groups:
            group["lr"] = group["lr_mult"] * (lr_zoom if group["zoom"] else lr_class)


# ----------------------------------------------------------------------------------------------
# data-parallel (one process per GPU, RCCL over xGMI)
# ----------------------------------------------------------------------------------------------
def ddp_setup(backend=None):
    """train_deform_semantic.py:45-55, driven by torchrun's env instead of mp.spawn arguments."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if torch.cuda.is_available():
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
        kw = {}
        if backend == "nccl" and torch.cuda.is_available():      # bind the communicator (and barrier()) to this rank's GPU
            kw["device_id"] = torch.device("cuda", local_rank % torch.cuda.device_count())
        dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)
    elif torch.cuda.is_available():
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
    return rank, local_rank, world


def _collectives_on():
    """A process group is up.  A group of ONE rank still runs its collectives (they are cheap no-op exchanges): the same
    code path -- device binding, RCCL's stream hand-off behind the side-stream backward -- is then exercised on a single GPU."""
    return dist.is_available() and dist.is_initialized()


def _is_torch_ddp(module):
    return module is not None and isinstance(module, torch.nn.parallel.DistributedDataParallel)


def broadcast_parameters(optimizers, module=None, src=0):
    """DDP construction-time broadcast (train_deform_semantic.py:395): one collective per arena."""
    if not _collectives_on():
        return
    for opt in optimizers:
        dist.broadcast(opt.flat.data, src=src)
        opt.flat.refresh_amax()          # the arena was rewritten behind the parameters' version counters
    if module is not None:
        broadcast_buffers(module, src=src)
    # (No device-wide synchronise here.  Round 4 added one on the guess that a gloo broadcast of the last two arenas "had not landed" in one
    # red run of the 2-rank wrapper test; the record of that run refutes it -- the encoder / decoder arenas agreed to 2e-7, so both passes
    # ran the same parameters and the same forward -- and a synchronous collective already orders the CURRENT stream behind the backend's
    # copy-back (gloo: events on its copy streams; RCCL: its own stream), which is the stream refresh_amax and the next forward run on,
    # and every side stream of this package forks from that stream by an event.  DESIGN.md 6 has the launch-by-launch ordering table.)


class FlatBuffers:
    """Every float32 buffer of `module` (BatchNorm running statistics, the reference SyncBN's three extra buffers, the Gaussian
    filter) re-homed into ONE flat tensor; the registered buffers become views, so the kernels that update running statistics
    through their pointers keep working and the per-step buffer broadcast is a single collective."""

    def __init__(self, module):
        bufs = [b for _, b in module.named_buffers() if b.dtype == torch.float32]
        assert bufs, "module has no float buffers"
        offs, n = [], 0
        for b in bufs:
            offs.append(n)
            n += (b.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.data = torch.zeros(n, device=bufs[0].device, dtype=torch.float32)
        for b, o in zip(bufs, offs):
            view = self.data[o:o + b.numel()].view(b.shape)
            view.copy_(b)
            b.data = view
        self.buffers, self.offsets = bufs, offs


def broadcast_buffers(module, src=0):
    """DDP(broadcast_buffers=True) semantics (train_deform_semantic.py:395; torch DDP syncs module buffers from rank 0 at the start of
    every training forward): after this call every rank holds rank 0's BatchNorm running statistics.  One collective over the
    module's flat buffer arena (built on first use)."""
    if not _collectives_on():
        return
    flat = getattr(module, "_fs_flat_buffers", None)
    if flat is None:
        flat = FlatBuffers(module)
        object.__setattr__(module, "_fs_flat_buffers", flat)      # not a submodule / buffer: keep it out of state_dict
    dist.broadcast(flat.data, src=src)


COMM_EVENTS = None      # bench.py: a list that receives one (start, stop) HIP-event pair per gradient exchange (the four arena all-reduces)


def allreduce_gradients(optimizers, module=None):
    """Gradient average across ranks: one SUM all-reduce per arena; the 1/world is folded into Adam.
    `module` wrapped by torch's DistributedDataParallel (the reference's call site, train_deform_semantic.py:395): its reducer has
    already averaged the gradients into the arena views during backward, so nothing is exchanged here."""
    from . import ops
    ops.join_wgrad_streams()          # weight gradients of small layers may still be running on their side stream
    if not _collectives_on() or _is_torch_ddp(module):
        for opt in optimizers:
            opt.grad_scale = 1.0
        return
    world = dist.get_world_size()
    timed = COMM_EVENTS is not None and optimizers[0].flat.grad.is_cuda
    if timed:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    for opt in optimizers:
        dist.all_reduce(opt.flat.grad, op=dist.ReduceOp.SUM)
        opt.grad_scale = 1.0 / world
    if timed:
        ev1.record()          # (the process group's stream is joined to the current stream by the collective's own event hand-off)
        COMM_EVENTS.append((ev0, ev1))


def shard_indices(n_samples, rank, world, epoch_seed=0, shuffle=True):
    """DistributedSampler(num_replicas, rank, shuffle=True) sharding (train_deform_semantic.py:462);
    set_epoch is never called in the reference, so the permutation is the same every epoch (seed 0)."""
    g = torch.Generator().manual_seed(epoch_seed)
    idx = torch.randperm(n_samples, generator=g).tolist() if shuffle else list(range(n_samples))
    total = (n_samples + world - 1) // world * world
    idx += idx[: total - len(idx)]
    return idx[rank:total:world]


# ----------------------------------------------------------------------------------------------
# one optimisation step / one evaluation step
# ----------------------------------------------------------------------------------------------
def train_step(module, optimizers, batch, cfg, epoch=1, cur_iter=0):
    """train_deform_semantic.py:74-129 for one batch (X,F,Y,cls) already on the device."""
    from .ops import DropoutState
    X, Fp, Y, cls = batch
    feed = {"img_data": X[:, :3], "seg_label": Y, "focus_point": Fp, "cls_label": cls}
    for opt in optimizers:
        opt.zero_grad()
    adjust_learning_rate(optimizers, cur_iter, cfg, epoch=epoch)
    DropoutState.step += 1
    ddp = _is_torch_ddp(module)
    inner = module.module if ddp else module
    if not ddp:
        broadcast_buffers(module)      # no-op without a process group; torch DDP syncs buffers from rank 0 itself before every forward
    out = module(feed, epoch=epoch, cur_iter=cur_iter)
    loss = out[0]
    loss.mean().backward()
    # models/models.py:721 asserts on NaN saliency in the middle of the forward, i.e. BEFORE any update; the deferred flag is read
    # here, after backward (the saliency forward finished long ago: no stall) and before the gradient exchange and the optimiser
    # steps, so a caller that catches the AssertionError still holds the parameters and Adam moments of the previous step
    if hasattr(inner, "check_nan"):
        inner.check_nan()
    allreduce_gradients(optimizers, module)
    T = cfg.TRAIN
    for opt in optimizers:          # train_deform_semantic.py:112-120: which optimisers step in this epoch
        zoom = opt.param_groups[0]["zoom"]
        if T.fix_deform_aft_pretrain and T.fix_deform_start_epoch <= epoch <= T.fix_deform_end_epoch:
            if zoom:                # deformation module frozen: its Adam state (t, m, v) must not advance either
                continue
        elif T.opt_deform_LabelEdge and T.fix_seg_start_epoch <= epoch <= T.fix_seg_end_epoch:
            if not zoom:            # segmentation module frozen
                continue
        opt.step()
    from . import ops
    ops.repack_weights()      # the conv layers' weight packs of the next step, on a side stream beside its front end
    return out


@torch.no_grad()
def eval_step(module, batch):
    """eval.py:389-405 -- same forward with is_inference=True under no_grad (module.eval() by caller)."""
    X, Fp, Y, cls = batch
    feed = {"img_data": X[:, :3], "seg_label": Y, "focus_point": Fp, "cls_label": cls}
    out = module(feed, is_inference=True)
    if hasattr(module, "check_nan"):
        module.check_nan()
    return out


@torch.no_grad()
def evaluate_step(module, batch, meter=None, trimap_meter=None, class_meter=None):
    """Full-resolution scoring of one batch without the loss: module.evaluate on (X, Fp, Y, cls) (module.eval() by caller), the way
    eval_step wraps forward.  Returns evaluate's (acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg, counts); a FullResMeter given as `meter`
    takes the counts (no host read).  With a TrimapMeter as `trimap_meter` the call is evaluate(trimap=trimap_meter.dia_factor,
    trimap_frame=trimap_meter.frame): the result ends with the trim counters, which that meter takes.  With a ClassIoUMeter as
    `class_meter` the call has class_areas=True as well: the class areas come last in the result and go to that meter."""
    return evaluate_step_hd(module, batch, meter, trimap_meter, class_meter)


@torch.no_grad()
def evaluate_step_hd(module, batch, meter=None, trimap_meter=None, class_meter=None, hd_meter=None):
    """evaluate_step with one more meter: with a HausdorffMeter as `hd_meter` the call has hausdorff=hd_meter.q as well, the surface
    statistics come last in the result (after the class areas) and go to that meter.  Without it, evaluate_step itself."""
    X, Fp, Y, cls = batch
    extra = {} if class_meter is None else {"class_areas": True}
    if hd_meter is not None:
        extra["hausdorff"] = hd_meter.q
    if trimap_meter is None:
        out = module.evaluate(X[:, :3], Fp, Y, cls, **extra)
    else:
        out = module.evaluate(X[:, :3], Fp, Y, cls, trimap=trimap_meter.dia_factor, trimap_frame=trimap_meter.frame, **extra)
    module.check_nan()
    if meter is not None:
        meter.update(out[4])
    if trimap_meter is not None:
        trimap_meter.update(out[5])
    if class_meter is not None:
        class_meter.update(out[-2 if hd_meter is not None else -1])
    if hd_meter is not None:
        hd_meter.update(out[-1])
    return out


def synthetic_batch(B, H, W, seed=1, device="cuda"):
    """uniform RGB, gaze in [0.1,0.9), disc mask of radius 0.15 H at the gaze."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(B, 3, H, W, generator=g)
    Fp = torch.rand(B, 2, generator=g) * 0.8 + 0.1
    cls = torch.randint(0, 50, (B, 1), generator=g)
    ii = torch.arange(H, dtype=torch.float32)[None, :, None]
    jj = torch.arange(W, dtype=torch.float32)[None, None, :]
    cy = (Fp[:, 0] * (H - 1))[:, None, None]
    cx = (Fp[:, 1] * (W - 1))[:, None, None]
    Y = (((ii - cy) ** 2 + (jj - cx) ** 2) <= (0.15 * H) ** 2).float().unsqueeze(1)
    return X.to(device), Fp.to(device), Y.to(device), cls.to(device)


def build_module(cfg, device="cuda", init="name_keyed"):
    from . import ModelBuilder, DeformSegmentationModule
    from .weights import apply_name_keyed_init
    M = cfg.MODEL
    enc = ModelBuilder.build_encoder(M.arch_encoder, M.fc_dim, M.weights_encoder)
    dec = ModelBuilder.build_decoder(M.arch_decoder, M.fc_dim, cfg.DATASET.num_class, M.weights_decoder)
    sal = ModelBuilder.build_net_saliency(cfg, M.weights_net_saliency)
    comp = ModelBuilder.build_net_compress(cfg, M.weights_net_compress)
    module = DeformSegmentationModule(enc, dec, sal, comp, None, cfg)
    if init == "name_keyed":
        apply_name_keyed_init(module)
    module.to(device)
    nets = (module.encoder, module.decoder, None, module.localization, module.net_compress)
    return module, nets


# ----------------------------------------------------------------------------------------------
# metrics step after the path
# ----------------------------------------------------------------------------------------------
class DeviceMeter:
    """Running averages of the step outputs (loss, acc, edge loss, ...) kept ON the device: `update` is an in-place add of
    0-d tensors (no `.item()` sync per iteration, unlike utils.AverageMeter at train_deform_semantic.py:100-123), and
    `averages(reduce=True)` makes the one host read, after ONE all-reduce of [sums..., count] over the ranks -- the
    reference keeps its meters per rank and never reduces them."""

    def __init__(self, names, device):
        self.names = list(names)
        self.acc = torch.zeros(len(self.names) + 1, device=device, dtype=torch.float64)
        self._sums, self._count = self.acc[:-1], self.acc[-1:]       # views, made once

    def update(self, values, weight=1.0):
        dev = self.acc.device
        if all(torch.is_tensor(x) and x.device == dev and x.dim() == 0 for x in values):
            v = torch.stack([x.detach() for x in values])          # the step's outputs: one stack + two in-place adds per step
        else:
            v = torch.stack([(x.detach().to(device=dev, dtype=torch.float64) if torch.is_tensor(x) else torch.tensor(float(x), dtype=torch.float64, device=dev)).reshape(())
                             for x in values])
        self._sums.add_(v, alpha=weight)
        self._count.add_(weight)

    def averages(self, reduce=True):
        tot = self.acc.clone()
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        tot = tot.cpu()
        n = float(tot[-1])
        return {k: (float(tot[i]) / n if n > 0 else float("nan")) for i, k in enumerate(self.names)}


class FullResMeter:
    """Dataset-level full-resolution scores from the per-image counts of module.evaluate / ops.unwarp_accuracy (SURVEY.md §8(f)-2:
    'a single global IoU').  `update(counts)` adds a batch's (B,6) int64 counts into device-resident sums -- the six counters, the four
    per-image accuracies (fp64) and the number of images -- without a host read; `result(reduce=True)` makes ONE all-reduce over the
    ranks and ONE host read.  It returns the reference's mean-of-images accuracies (acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg: what
    averaging forward's per-batch values weighted by batch size gives) beside the dataset-level iou_fg = sum cls_fg / sum union_fg and
    iou_bin_fg = sum bin_fg / sum union_fg, in which a large instance weighs by its pixels, plus the raw `counts` and `images`."""

    NAMES = ("acc", "acc_bin_fg", "acc_cls_fbg", "acc_bin_fbg")

    def __init__(self, device):
        self.counts = torch.zeros(6, device=device, dtype=torch.int64)
        self.sums = torch.zeros(5, device=device, dtype=torch.float64)           # four accuracy sums, then the image count

    def update(self, counts):
        from . import ops
        if counts.dim() != 2 or counts.shape[1] != 6:
            raise ValueError(f"counts must be (B, 6), got {tuple(counts.shape)}")
        counts = counts.to(device=self.counts.device, dtype=torch.int64)
        self.counts.add_(counts.sum(0))
        self.sums[:4].add_(ops.image_accuracies_from_counts(counts).double().sum(0))
        self.sums[4:].add_(float(counts.shape[0]))

    def result(self, reduce=True):
        # one fp64 vector carries everything: each int64 sum as two 32-bit halves, whose sums over the ranks stay exact in fp64
        tot = torch.cat([(self.counts >> 32).double(), (self.counts & 0xFFFFFFFF).double(), self.sums])
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        tot = tot.cpu().tolist()
        c = [(int(tot[q]) << 32) + int(tot[6 + q]) for q in range(6)]
        n = tot[16]
        res = {k: (tot[12 + i] / n if n > 0 else float("nan")) for i, k in enumerate(self.NAMES)}
        res["iou_fg"] = c[0] / c[2] if c[2] > 0 else 0.0                         # an empty union scores 0, as the per-image quotients do
        res["iou_bin_fg"] = c[1] / c[2] if c[2] > 0 else 0.0
        res["counts"], res["images"] = c, int(n)
        return res


class TrimapMeter:
    """Dataset-level trimap boundary accuracy (eval.py:41-67,258-262,295-310) from the trim counters of module.evaluate(trimap=...) /
    ops.unwarp_trimap.  `update(trim)` adds a batch's (B, dia_factor + 1, 3) int64 counters into device-resident sums -- the counters, the
    per-image accuracies (fp64) and, per band width, the number of images with a non-empty band -- without a host read;
    `result(reduce=True)` makes ONE all-reduce over the ranks and ONE host read.  Per width 2**i it returns `acc` / `acc_bin`, the
    reference's mean over images of cls_ok / (total + 1e-10) and its foreground / background counterpart, over the images whose band is
    not empty (an image without a boundary pixel has none: the reference divides 0 by 0 there); `pooled` / `pooled_bin`, sum cls_ok /
    sum total and sum bin_ok / sum total, in which an image weighs by its band's pixels; the raw `counts` (D+1 rows of total, cls_ok,
    bin_ok); `images` per width and `widths`.  `frame` is evaluate's trimap_frame."""

    def __init__(self, device, dia_factor=5, frame=True):
        self.dia_factor, self.frame = int(dia_factor), bool(frame)
        if not 0 <= self.dia_factor <= 7:
            raise ValueError(f"dia_factor must be 0 .. 7, got {dia_factor}")
        n = self.dia_factor + 1
        self.counts = torch.zeros(n, 3, device=device, dtype=torch.int64)
        self.sums = torch.zeros(n, 3, device=device, dtype=torch.float64)        # per width: sum of cls acc, of bin acc, image count

    def update(self, trim):
        from . import ops
        if trim.dim() != 3 or tuple(trim.shape[1:]) != (self.dia_factor + 1, 3):
            raise ValueError(f"trim must be (B, {self.dia_factor + 1}, 3), got {tuple(trim.shape)}")
        trim = trim.to(device=self.counts.device, dtype=torch.int64)
        self.counts.add_(trim.sum(0))
        seen = (trim[..., 0] > 0).double()
        self.sums[:, :2].add_((ops.trimap_from_counts(trim) * seen[..., None]).sum(0))
        self.sums[:, 2].add_(seen.sum(0))

    def result(self, reduce=True):
        # one fp64 vector, as FullResMeter.result: each int64 sum as two 32-bit halves, whose sums over the ranks stay exact in fp64
        c = self.counts.reshape(-1)
        tot = torch.cat([(c >> 32).double(), (c & 0xFFFFFFFF).double(), self.sums.reshape(-1)])
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        tot = tot.cpu().tolist()
        n = self.dia_factor + 1
        cnt = [[(int(tot[i * 3 + f]) << 32) + int(tot[3 * n + i * 3 + f]) for f in range(3)] for i in range(n)]
        sums = [tot[6 * n + 3 * i: 6 * n + 3 * i + 3] for i in range(n)]
        nan = float("nan")
        return {"widths": [2 ** i for i in range(n)],
                "acc": [s[0] / s[2] if s[2] > 0 else nan for s in sums],
                "acc_bin": [s[1] / s[2] if s[2] > 0 else nan for s in sums],
                "pooled": [c[1] / c[0] if c[0] > 0 else nan for c in cnt],
                "pooled_bin": [c[2] / c[0] if c[0] > 0 else nan for c in cnt],
                "counts": cnt, "images": [int(s[2]) for s in sums]}


class ClassIoUMeter:
    """Dataset-level per-class IoU / Dice (eval.py:218-257,313-331) from the class areas of module.evaluate(class_areas=True) /
    ops.unwarp_class_areas.  `update(areas)` adds a batch's (B, 3, num_class, 3) int64 areas into device-resident sums -- the areas, the
    per-image label shares (fp64) and the number of images -- without a host read; `result(reduce=True)` makes ONE all-reduce over the
    ranks and ONE host read.  For each space of SPACES it returns `iou` / `dice` [K] from the summed areas (the reference's
    intersection_meter.sum / (union_meter.sum + 1e-10) and its Dice), `miou` / `mdice`, their means over all K classes (the reference's
    iou.mean()), `miou_present`, the mean over the classes whose summed union is not empty (nan without one), and the raw `areas`
    (K rows of inter, pred, lab).  Beside them: `label_share_full` / `label_share_sampled` [K], the mean over images of each class's
    share of the labelled pixels before and after sampling, in percent, and `label_share_shift`, sampled minus full (eval.py:326-328);
    `images`."""

    SPACES = ("full", "ceiling", "sampled")

    def __init__(self, device, num_class):
        self.num_class = int(num_class)
        if self.num_class < 2:
            raise ValueError(f"num_class must be at least 2, got {num_class}")
        self.areas = torch.zeros(3, self.num_class, 3, device=device, dtype=torch.int64)
        self.sums = torch.zeros(2 * self.num_class + 1, device=device, dtype=torch.float64)      # label shares full, sampled; image count

    def update(self, areas):
        K = self.num_class
        if areas.dim() != 4 or tuple(areas.shape[1:]) != (3, K, 3):
            raise ValueError(f"areas must be (B, 3, {K}, 3), got {tuple(areas.shape)}")
        areas = areas.to(device=self.areas.device, dtype=torch.int64)
        self.areas.add_(areas.sum(0))
        lab = areas[:, (0, 2), :, 2].double()                                    # (B, 2, K)
        share = lab / lab.sum(2, keepdim=True).clamp_(min=1.0)                   # an image without a labelled pixel in range: all 0
        self.sums[:2 * K].add_(share.sum(0).reshape(-1))
        self.sums[2 * K:].add_(float(areas.shape[0]))

    def result(self, reduce=True):
        # one fp64 vector, as FullResMeter.result: each int64 sum as two 32-bit halves, whose sums over the ranks stay exact in fp64
        K = self.num_class
        c = self.areas.reshape(-1)
        tot = torch.cat([(c >> 32).double(), (c & 0xFFFFFFFF).double(), self.sums])
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        tot = tot.cpu().tolist()
        n9 = 9 * K
        nan = float("nan")
        res = {}
        for s, name in enumerate(self.SPACES):
            rows = [[(int(tot[(s * K + k) * 3 + f]) << 32) + int(tot[n9 + (s * K + k) * 3 + f]) for f in range(3)] for k in range(K)]
            union = [r[1] + r[2] - r[0] for r in rows]
            iou = [r[0] / (u + 1e-10) for r, u in zip(rows, union)]
            dice = [2 * r[0] / (u + r[0] + 1e-10) for r, u in zip(rows, union)]
            present = [v for v, u in zip(iou, union) if u > 0]
            res[name] = {"iou": iou, "dice": dice, "miou": sum(iou) / K, "mdice": sum(dice) / K,
                         "miou_present": sum(present) / len(present) if present else nan, "areas": rows}
        n = tot[2 * n9 + 2 * K]
        full = [100.0 * v / n if n > 0 else nan for v in tot[2 * n9: 2 * n9 + K]]
        samp = [100.0 * v / n if n > 0 else nan for v in tot[2 * n9 + K: 2 * n9 + 2 * K]]
        res["label_share_full"], res["label_share_sampled"] = full, samp
        res["label_share_shift"] = [b - a for a, b in zip(full, samp)]
        res["images"] = int(n)
        return res


class HausdorffMeter:
    """Dataset-level Hausdorff percentile (HD95 at q = 95; VAL.hd95) from the surface statistics of module.evaluate(hausdorff=q) /
    ops.surface_hd.  `update(hd)` adds a batch's (B,4) int64 statistics into device-resident sums -- the per-image distances
    (ops.hd_from_stats, fp64) of the images where both borders exist, their number, and the numbers of images left out -- without a
    host read; `result(reduce=True)` makes ONE all-reduce over the ranks and ONE host read.  It returns `hd`, the mean distance in
    pixels over the images where both borders exist (nan without one), `images`, their number, and `skipped_empty_pred` /
    `skipped_empty_label`, the images whose predicted / label mask has no border (an image with neither counts in both).  The
    reference's function raises RuntimeError on an empty mask; here such an image is left out and counted, as the trimap's
    empty-band images are."""

    def __init__(self, device, q=95):
        from . import unwarp
        self.q = unwarp._hd_q(q)
        self.sums = torch.zeros(4, device=device, dtype=torch.float64)           # distance sum, images, empty pred, empty label

    def update(self, hd):
        from . import ops
        if hd.dim() != 2 or hd.shape[1] != 4:
            raise ValueError(f"hd must be (B, 4), got {tuple(hd.shape)}")
        hd = hd.to(device=self.sums.device, dtype=torch.int64)
        d = ops.hd_from_stats(hd, self.q)
        ok = ~torch.isnan(d)
        self.sums.add_(torch.stack([torch.where(ok, d, torch.zeros_like(d)).sum(), ok.double().sum(),
                                    (hd[:, 0] <= 0).double().sum(), (hd[:, 1] <= 0).double().sum()]))

    def result(self, reduce=True):
        tot = self.sums.clone()
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        tot = tot.cpu().tolist()
        return {"hd": tot[0] / tot[1] if tot[1] > 0 else float("nan"), "images": int(tot[1]), "skipped_empty_pred": int(tot[2]),
                "skipped_empty_label": int(tot[3]), "q": self.q}


class InstanceAPMeter:
    """Dataset-level AP and Boundary AP of the instance records (module.evaluate_instances / ops.mask_pair_counts): what a COCO / LVIS
    evaluator reports, restated from COCOeval's published algorithm for this task's shape -- one label instance and at most one record
    an image (unpinned: the reference has no instance metric; Boundary AP is Cheng et al., CVPR 2021).  `update(cat, conf, stats, pair,
    cls_label)` keeps one row an image ON the device -- ten int64: cat, cls_label, area, the six counters, and the bits of the fp32
    score -- without a host read; `result(reduce=True)` exchanges the row counts over the ranks, runs ONE padded all_gather, puts the
    ranks' rows one behind the other in rank order, makes ONE host read and computes in int64 / fp64 on the host:

    a record exists iff its area > 0, a label instance iff |g| > 0 (its class is cls_label).  Per class k and threshold t = (50 + 5 j)
    / 100, j = 0 .. 9: the records with cat == k in descending score (ties in insertion order, a NaN score last); a record is a TP iff
    its image's label instance exists, has class k and the measure passes t -- in integers, 100 n >= (50 + 5 j) u with u = a + b - n > 0
    -- else an FP; recall cumTP / nGT_k and precision cumTP / (cumTP + cumFP), precision made non-increasing from the right and sampled
    at the 101 recalls q / 100 (the first rank with 100 cumTP >= q nGT_k; 0 past the end); AP_kj is the mean of the samples.  `AP`,
    `AP50`, `AP75` average over the classes with nGT_k > 0 (AP also over j; nan without such a class), the measure being mask IoU;
    `bAP`, `bAP50`, `bAP75` take min(mask IoU, Boundary IoU): both comparisons must hold.  Beside them `mIoU` and `mBIoU`, the means
    of the two measures over the images whose label instance exists (a missing record counts 0), `cls_acc`, the share of images with
    cat == cls_label, `n_images` and `n_records`."""

    ROW = 10

    def __init__(self, device, num_class):
        self.num_class = int(num_class)
        if self.num_class < 2:
            raise ValueError(f"num_class must be at least 2, got {num_class}")
        self.device = torch.device(device)
        self.rows = []                                                           # one (B, ROW) int64 tensor a batch, on the device

    def update(self, cat, conf, stats, pair, cls_label):
        B = int(cat.shape[0])
        if tuple(conf.shape) != (B, 3) or stats.dim() != 2 or stats.shape[0] != B or tuple(pair.shape) != (B, 6) or cls_label.shape[0] != B \
                or cls_label.numel() != B:
            raise ValueError(f"cat (B,), conf (B,3), stats (B,6), pair (B,6) and cls_label (B,) or (B,1) must share B, got {tuple(cat.shape)}, "
                             f"{tuple(conf.shape)}, {tuple(stats.shape)}, {tuple(pair.shape)}, {tuple(cls_label.shape)}")
        dev = self.device
        score = conf[:, 0].to(device=dev, dtype=torch.float32).contiguous().view(torch.int32).to(torch.int64)
        row = torch.cat([cat.to(device=dev, dtype=torch.int64).reshape(B, 1), cls_label.to(device=dev, dtype=torch.int64).reshape(B, 1),
                         stats[:, :1].to(device=dev, dtype=torch.int64), pair.to(device=dev, dtype=torch.int64), score.reshape(B, 1)], 1)
        self.rows.append(row)

    def gathered(self, reduce=True):
        """The rows of every rank, rank after rank, as a host int64 tensor (n, ROW)."""
        mine = torch.cat(self.rows, 0) if self.rows else torch.zeros(0, self.ROW, device=self.device, dtype=torch.int64)
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            world = dist.get_world_size()
            n = torch.tensor([mine.shape[0]], device=self.device, dtype=torch.int64)
            counts = [torch.zeros_like(n) for _ in range(world)]
            dist.all_gather(counts, n)
            counts = [int(c) for c in torch.cat(counts).cpu().tolist()]
            cap = max(max(counts), 1)
            padded = torch.zeros(cap, self.ROW, device=self.device, dtype=torch.int64)
            padded[:mine.shape[0]] = mine
            parts = [torch.zeros_like(padded) for _ in range(world)]
            dist.all_gather(parts, padded)
            mine = torch.cat([p[:c] for p, c in zip(parts, counts)], 0)
        return mine.cpu()

    @staticmethod
    def _passes(n, a, b, t100):
        u = a + b - n
        return (u > 0) & (100 * n >= t100 * u)

    def result(self, reduce=True):
        import numpy as np
        rows = self.gathered(reduce).numpy()
        cat, cls, area, pair = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:9]
        score = rows[:, 9].astype(np.int32).view(np.float32).astype(np.float64)
        key = np.where(np.isnan(score), -np.inf, score)
        has_gt, has_rec = pair[:, 2] > 0, area > 0
        nan = float("nan")
        res = {}
        aps = {(b, t): [] for b in (0, 1) for t in range(10)}
        for k in range(self.num_class):
            n_gt = int((has_gt & (cls == k)).sum())
            if n_gt == 0:
                continue
            sel = np.nonzero(has_rec & (cat == k))[0]
            sel = sel[np.argsort(-key[sel], kind="stable")]                      # descending score, ties in insertion order
            p = pair[sel]
            right = has_gt[sel] & (cls[sel] == k)
            for j in range(10):
                mask_ok = right & self._passes(p[:, 0], p[:, 1], p[:, 2], 50 + 5 * j)
                for b, ok in ((0, mask_ok), (1, mask_ok & self._passes(p[:, 3], p[:, 4], p[:, 5], 50 + 5 * j))):
                    tp = np.cumsum(ok.astype(np.int64))
                    seen = np.arange(1, len(sel) + 1, dtype=np.int64)
                    prec = tp / seen
                    if len(prec):
                        prec = np.maximum.accumulate(prec[::-1])[::-1]
                    at = np.searchsorted(100 * tp, np.arange(101, dtype=np.int64) * n_gt, side="left")
                    samples = [float(prec[i]) if i < len(prec) else 0.0 for i in at.tolist()]
                    aps[(b, j)].append(math.fsum(samples) / 101)
        for b, name in ((0, "AP"), (1, "bAP")):
            every = [v for j in range(10) for v in aps[(b, j)]]
            res[name] = math.fsum(every) / len(every) if every else nan
            for j, tag in ((0, "50"), (5, "75")):
                res[name + tag] = math.fsum(aps[(b, j)]) / len(aps[(b, j)]) if aps[(b, j)] else nan
        g = pair[has_gt]
        for name, o in (("mIoU", 0), ("mBIoU", 3)):
            u = g[:, o + 1] + g[:, o + 2] - g[:, o]
            vals = [int(n) / int(uu) if uu > 0 else 0.0 for n, uu in zip(g[:, o].tolist(), u.tolist())]
            res[name] = math.fsum(vals) / len(vals) if vals else nan
        res["n_images"], res["n_records"] = int(len(rows)), int(has_rec.sum())
        res["cls_acc"] = int((cat == cls).sum()) / len(rows) if len(rows) else nan
        return res


@torch.no_grad()
def evaluate_instances_step(module, batch, meter=None, **kw):
    """evaluate_step's counterpart for the instance record: module.evaluate_instances on (X, Fp, Y, cls) with **kw (component, snap_px,
    boundary, max_runs, seg_size) (module.eval() by caller).  Returns its (cat, stats, counts, conf[, comp], pair); an InstanceAPMeter
    given as `meter` takes (cat, conf, stats, pair, cls) -- no host read.  With candidates=(cbits, cand_off, cand_cat) in **kw (and
    cand_snap_px, seg_size) the batch's Y and cls are not read: the label is the candidate under the gaze, the result ends in (pair,
    sel), and the meter takes sel[:, 1], the selected candidate's class, as cls."""
    X, Fp, Y, cls = batch
    if kw.get("candidates") is not None:
        out = module.evaluate_instances(X[:, :3], Fp, **kw)
        module.check_nan()
        if meter is not None:
            meter.update(out[0], out[3], out[1], out[-2], out[-1][:, 1])
        return out
    out = module.evaluate_instances(X[:, :3], Fp, Y, cls, **kw)
    module.check_nan()
    if meter is not None:
        meter.update(out[0], out[3], out[1], out[-1], cls)
    return out


@torch.no_grad()
def score_coco_records(dt, gt, meter, boundary=0.02, device=None, chunk=64, images=None, gaze=None):
    """Score stored records: dt a COCO / LVIS results list (ops.instances_to_coco's records, with "score"), gt an annotation list,
    both with RLE segmentations (list or compressed string counts; ops.coco_to_instances), into an InstanceAPMeter -- what
    evaluate_instances_step feeds it, from files instead of a network.  The lists are paired by "image_id": one ground-truth instance
    an image, as everywhere in this library, and at most one result; an image with ground truth but no result enters as an empty
    record (area 0, score 0, class -1).  The images are taken in gt's order, grouped by mask size and cut into chunks of `chunk`; per
    chunk ONE host-to-device copy carries both sides, ops.rle_bits decodes them, ops.mask_pair_counts (d = ops.boundary_dilation(H, W,
    boundary)) counts, and meter.update(cat, conf, stats, pair, cls) takes stats[:, 0] = the decoded area, conf[:, 0] = the record's
    score and cls = the annotation's category_id.  No host read beyond the parse: a code that is not valid scores as an empty mask
    (ops.rle_bits(check=True) tells one).  Returns the number of images.  ValueError for two records of one image on either side, a
    result without ground truth, without a score or of another size than its ground truth, and as ops.coco_to_instances.

    images: the annotation file's "images" list (dicts with "id", "height", "width") or a dict image_id -> (H, W).  With it a
    segmentation may on either side be a polygon list, as LVIS v1 and COCO's non-crowd annotations carry it: its size comes from
    `images` (ValueError for an image that is not there), and a chunk's masks come from ops.coco_masks -- RLE rows through
    ops.rle_bits, polygon rows through ops.poly_bits (the reference's rasterisation restated, unpinned: see there), at most two copies
    a chunk.  With images=None every call, result and error is what it was without the argument.

    gaze: a dict image_id -> (row, col), normalised as focus is, for annotation files as they are downloaded: gt may then hold any
    number of records an image (dt still at most one), `images` is required (sizes come from there for polygon files), and an
    image's label is the annotation under its gaze (ops.mask_candidates, unpinned: of the instances that contain the gaze pixel the
    smallest, else the nearest one at any distance).  Per chunk: ops.coco_candidates for the ground truth, ops.coco_masks for the
    results, ONE ops.mask_candidates (pred = the results' words), ONE ops.mask_pair_counts against the selected words, then
    meter.update(cat, conf, stats, pair, sel[:, 1]) -- the selected annotation's category_id as cls.  An image whose gaze selects
    nothing (every annotation empty or not valid) enters with |g| = 0, i.e. without a label instance, by the meter's rule.
    "iscrowd" is not interpreted: a crowd record is a candidate like any other.  No host read beyond the parse.  ValueError for
    gaze without images, an image of gt without a gaze, a gaze that is not two numbers, and records of one image that differ in size.
    With gaze=None every call, result and error is what it is without the argument, the "more than one record" error included."""
    from . import masks, ops
    if isinstance(boundary, bool) or not isinstance(boundary, float) or not (boundary > 0.0) or math.isinf(boundary):
        raise ValueError(f"boundary must be a finite float > 0, got {boundary!r}")
    if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
        raise ValueError(f"chunk must be an integer >= 1, got {chunk!r}")
    device = meter.device if device is None else torch.device(device)

    def by_image(records, what):
        out = {}
        for i, r in enumerate(records):
            if not isinstance(r, dict) or "image_id" not in r:
                raise ValueError(f"{what} record {i}: the key 'image_id' is missing")
            if r["image_id"] in out:
                raise ValueError(f"{what}: image {r['image_id']!r} has more than one record; one instance an image is scored")
            out[r["image_id"]] = r
        return out

    sizes = None
    if images is not None:
        try:
            sizes = {k: (int(v[0]), int(v[1])) for k, v in images.items()} if isinstance(images, dict) else \
                {im["id"]: (int(im["height"]), int(im["width"])) for im in images}
        except (KeyError, TypeError, IndexError, ValueError):
            raise ValueError('images must be a list of dicts with "id", "height" and "width", or a dict image_id -> (H, W)') from None

    def size_of(r, what):
        seg = r.get("segmentation")
        if sizes is not None and isinstance(seg, (list, tuple)):
            if r["image_id"] not in sizes:
                raise ValueError(f"{what} of image {r['image_id']!r} is a polygon list and the image is missing from `images`")
            return sizes[r["image_id"]]
        if not isinstance(seg, dict) or "size" not in seg or len(seg["size"]) != 2:
            raise ValueError(f"{what} of image {r['image_id']!r}: the segmentation must be an RLE dict with a size (polygons are not rasterised here)")
        return int(seg["size"][0]), int(seg["size"][1])

    if gaze is not None:
        if not isinstance(gaze, dict):
            raise ValueError("gaze must be a dict image_id -> (row, col)")
        if sizes is None:
            raise ValueError("gaze needs `images`: the sizes of polygon annotations come from there")
        many = {}
        for i, r in enumerate(gt):
            if not isinstance(r, dict) or "image_id" not in r:
                raise ValueError(f"ground truth record {i}: the key 'image_id' is missing")
            many.setdefault(r["image_id"], []).append(r)
        dts, groups, focus_of = by_image(dt, "results"), {}, {}
        for image_id, recs in many.items():
            if image_id not in gaze:
                raise ValueError(f"ground truth: image {image_id!r} has no gaze")
            try:
                row, col = gaze[image_id]
                focus_of[image_id] = (float(row), float(col))
            except (TypeError, ValueError):
                raise ValueError(f"the gaze of image {image_id!r} must be two numbers (row, col), got {gaze[image_id]!r}") from None
            size = size_of(recs[0], "the ground truth")
            for r in recs[1:]:
                if size_of(r, "the ground truth") != size:
                    raise ValueError(f"image {image_id!r}: its annotations differ in size, {size} and {size_of(r, 'the ground truth')}")
            groups.setdefault(size, []).append(image_id)
        for image_id, r in dts.items():
            if image_id not in many:
                raise ValueError(f"results: image {image_id!r} has no ground truth")
            if "score" not in r:
                raise ValueError(f"results: the record of image {image_id!r} has no score")
            if size_of(r, "the result") != size_of(many[image_id][0], "the ground truth"):
                raise ValueError(f"image {image_id!r}: the result's size {size_of(r, 'the result')} differs from the ground truth's "
                                 f"{size_of(many[image_id][0], 'the ground truth')}")
        for (H, W), ids in groups.items():
            masks.boundary_dilation_capped(H, W, boundary)
        for (H, W), ids in groups.items():
            d = ops.boundary_dilation(H, W, boundary)
            for at in range(0, len(ids), int(chunk)):
                part = ids[at:at + int(chunk)]
                n = len(part)
                missing = {"category_id": -1, "score": 0.0, "segmentation": {"size": [H, W], "counts": [H * W]}}
                cbits, cand_off, cand_cat, _info, _rows = ops.coco_candidates([r for i in part for r in many[i]], (H, W), device, part)
                _ids, cat, bits, info, scores = ops.coco_masks([dict(dts.get(i, missing), image_id=i) for i in part], (H, W), device)
                focus = torch.tensor([focus_of[i] for i in part], dtype=torch.float32).reshape(n, 2).to(device)
                gbits, sel, _cand = ops.mask_candidates(cbits, cand_off, focus, W, pred=bits, cand_cat=cand_cat)
                pair = ops.mask_pair_counts(bits, gbits, d, Ws=W)
                stats = torch.zeros(n, 6, device=device, dtype=torch.int64)
                stats[:, 0] = info[:, 1]
                conf = torch.zeros(n, 3, device=device, dtype=torch.float32)
                conf[:, 0] = scores
                meter.update(cat, conf, stats, pair, sel[:, 1])
        return len(many)
    gts, dts = by_image(gt, "ground truth"), by_image(dt, "results")
    groups = {}
    for image_id, g in gts.items():
        groups.setdefault(size_of(g, "the ground truth"), []).append(image_id)
    for image_id, r in dts.items():
        if image_id not in gts:
            raise ValueError(f"results: image {image_id!r} has no ground truth")
        if "score" not in r:
            raise ValueError(f"results: the record of image {image_id!r} has no score")
        if size_of(r, "the result") != size_of(gts[image_id], "the ground truth"):
            raise ValueError(f"image {image_id!r}: the result's size {size_of(r, 'the result')} differs from the ground truth's "
                             f"{size_of(gts[image_id], 'the ground truth')}")
    for (H, W), ids in groups.items():
        d = masks.boundary_dilation_capped(H, W, boundary)
        for at in range(0, len(ids), int(chunk)):
            part = ids[at:at + int(chunk)]
            n = len(part)
            missing = {"category_id": -1, "score": 0.0, "segmentation": {"size": [H, W], "counts": [H * W]}}
            both = [dict(dts.get(i, missing), image_id=i) for i in part] + [dict(gts[i], score=0.0) for i in part]
            if sizes is None:
                _ids, cat, n_runs, counts, _sizes, scores = ops.coco_to_instances(both, device)
                bits, info = ops.rle_bits(counts, n_runs, (H, W))
            else:
                _ids, cat, bits, info, scores = ops.coco_masks(both, (H, W), device)
            pair = ops.mask_pair_counts(bits[:n], bits[n:], d, Ws=W)
            stats = torch.zeros(n, 6, device=device, dtype=torch.int64)
            stats[:, 0] = info[:n, 1]
            conf = torch.zeros(n, 3, device=device, dtype=torch.float32)
            conf[:, 0] = scores[:n]
            meter.update(cat[:n], conf, stats, pair, cat[n:])
    return len(gts)


# ----------------------------------------------------------------------------------------------
# checkpoint / resume
# ----------------------------------------------------------------------------------------------
_NET_FILES = ("encoder", "decoder", "saliency", "compress")


def save_checkpoint(dirpath, epoch, nets, optimizers=None, extra=None):
    """train_deform_semantic.py:166-184 -- `{encoder,decoder,saliency,compress}_epoch_{N}.pth` hold plain state_dicts with the
    reference's keys and shapes (they load into the reference and vice versa).  In addition (the reference saves neither, so a
    resumed run restarts Adam from zero) `train_state_epoch_{N}.pth` keeps the four Adam states, the dropout step counter and
    the torch RNG state.  epoch may be 'last' (checkpoint_last, :188-208)."""
    from .ops import DropoutState
    net_encoder, net_decoder, _crit, net_saliency, net_compress = nets
    os.makedirs(dirpath, exist_ok=True)
    for name, net in zip(_NET_FILES, (net_encoder, net_decoder, net_saliency, net_compress)):
        torch.save({k: v.detach().cpu().contiguous() for k, v in net.state_dict().items()}, os.path.join(dirpath, f"{name}_epoch_{epoch}.pth"))
    state = {"epoch": epoch, "dropout": {"seed": DropoutState.seed, "step": DropoutState.step}, "rng": torch.get_rng_state(),
             "extra": extra}
    if optimizers is not None:
        state["optimizers"] = [{"t": o.t, "m": o.m.cpu(), "v": o.v.cpu(), "lr": o.param_groups[0]["lr"]} for o in optimizers]
    torch.save(state, os.path.join(dirpath, f"train_state_epoch_{epoch}.pth"))


def load_checkpoint(dirpath, epoch, nets, optimizers=None, strict=True):
    """Inverse of save_checkpoint; also accepts a directory written by the reference (no train_state file: weights only).
    Returns the `extra` object (or None)."""
    from .ops import DropoutState
    net_encoder, net_decoder, _crit, net_saliency, net_compress = nets
    for name, net in zip(_NET_FILES, (net_encoder, net_decoder, net_saliency, net_compress)):
        sd = torch.load(os.path.join(dirpath, f"{name}_epoch_{epoch}.pth"), map_location="cpu", weights_only=True)
        net.load_state_dict(sd, strict=strict)
    path = os.path.join(dirpath, f"train_state_epoch_{epoch}.pth")
    if not os.path.exists(path):
        if optimizers is not None:
            for o in optimizers:
                o.flat.refresh_amax()
        return None
    state = torch.load(path, map_location="cpu", weights_only=True)      # plain tensors / numbers / strings only (see save_checkpoint)
    DropoutState.seed, DropoutState.step = state["dropout"]["seed"], state["dropout"]["step"]
    torch.set_rng_state(state["rng"])
    if optimizers is not None:
        for o, sd in zip(optimizers, state.get("optimizers", [])):
            o.load_state_dict(sd)
            o.param_groups[0]["lr"] = sd["lr"]
            o.flat.refresh_amax()          # the parameters were rewritten through load_state_dict
    return state.get("extra")


def history_path(dirpath, epoch, rank=0, kind="csv"):
    """The reference writes `history_epoch_last_{rank}.csv` / `history_epoch_{N}_{rank}.pth` (train…:230-235) but resumes from
    `history_epoch_{N}.csv` (:416), which never exists.  Writers and readers here share this one function."""
    return os.path.join(dirpath, f"history_epoch_{epoch}_{rank}.{kind}")
