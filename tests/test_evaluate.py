"""Full-resolution evaluation: ops.unwarp_accuracy (fs_unwarp_accuracy), ops.accuracies_from_counts, DeformSegmentationModule.evaluate,
forward's MODEL.upsample branch on top of it, train.FullResMeter and train.evaluate_step.

Every full-resolution pixel carries the decision of one grid point (tests/test_predict.py), and its ground truth is one read of the label
mask, so the six counters behind the four accuracies are summed in the pass that would have written the class map.  CPU: the counters'
arithmetic against the oracle's accuracies, and the meter over two gloo ranks.  GPU: the fused count pass against the unfused route
(unwarp_nearest -> argmax -> compare in torch; SegLoss's accuracies), evaluate against predict, forward(upsample=True) against the
hand-chained branch it replaces, the oracle, and the memory the route needs."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T
from oracle import fovealseg_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("acc", "acc_bin_fg", "acc_cls_fbg", "acc_bin_fbg")


def assemble(cls, m):
    """ops.PredAssemble restated: (B,K) x (B,h,w) -> (B,K,h,w)."""
    B, K = cls.shape
    pred = cls[:, :, None, None].expand(B, K, m.shape[1], m.shape[2]).clone()
    pred[:, -1] = cls[:, -1, None, None] * m
    return pred


def compose_gt(y, cls_label, K):
    """models.py:290-291: t = y.long() (truncation), gt = t * cls_label + (1 - t) * (K - 1).  y (B,H,W) float."""
    t = y.long()
    return t * cls_label.view(-1, 1, 1).long() + (1 - t) * (K - 1)


def counts_ref(labels, gt, K):
    """(B,6) int64 in plain torch: head_loss.hip:160-162's predicates on a class map and a ground truth."""
    bg = K - 1
    vg, vp, bgg, bgp, eq = gt < bg, labels < bg, gt == bg, labels == bg, labels == gt
    cols = [vg & eq, vg & (vg == vp), vg | vp, bgg & eq, bgg & (bgg == bgp), bgg | bgp]
    return torch.stack([c.flatten(1).sum(1) for c in cols], 1)


# ------------------------------------------------------------------------------------------------------------------ CPU ----------
@pytest.mark.parametrize("B,K,h,w,Hs,Ws,seed", [
    (2, 2, 9, 11, 37, 30, 0),          # the four cases of test_predict.py::test_factorisation_holds_on_the_oracle
    (2, 6, 9, 11, 50, 51, 1),
    (3, 51, 8, 8, 5, 6, 2),
    (1, 5, 12, 7, 23, 61, 3),
])
def test_accuracies_from_counts_against_the_oracle(B, K, h, w, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    grid = (torch.rand(B, h, w, 2, generator=g) * 2.4 - 1.2).clamp(-1, 1)
    cls = torch.randn(B, K, generator=g)
    m = torch.rand(B, h, w, generator=g) - 0.5
    cls[0, K - 1] = 4 * cls[0].abs().max()
    y = (torch.rand(B, Hs, Ws, generator=g) < 0.4).float()
    cls_label = torch.randint(0, K - 1, (B,), generator=g)
    pred_full = O.unwarp_nearest_ref(assemble(cls, m), grid, Hs, Ws)[0]
    gt = compose_gt(y, cls_label, K)
    counts = counts_ref(pred_full.argmax(1), gt, K)
    got = ops.accuracies_from_counts(counts)
    want = O.accuracies(pred_full, gt, bg=K - 1)
    assert got.dtype == torch.float32 and got.shape == (4,)
    for j in range(4):
        # a mean of values in [0,1], each built from exact integers with at most four fp32 roundings (<= 2.4e-7)
        assert abs(float(got[j]) - float(want[j])) <= 1e-6, (NAMES[j], float(got[j]), float(want[j]))
    assert int(counts[:, 2].min()) > 0                                                # foreground somewhere in every image here


def test_accuracies_from_counts_without_foreground():
    # image 1: no foreground in label or prediction -> union_fg = 0 and its foreground accuracies are 0, not NaN
    K = 5
    labels = torch.full((2, 6, 7), K - 1, dtype=torch.int64)
    labels[0, :3] = 2
    y = torch.zeros(2, 6, 7)
    y[0, 1:4] = 1.0
    cls_label = torch.tensor([2, 3])
    gt = compose_gt(y, cls_label, K)
    counts = counts_ref(labels, gt, K)
    assert counts[1].tolist() == [0, 0, 0, 42, 42, 42]
    got = ops.accuracies_from_counts(counts)
    assert bool(torch.isfinite(got).all())
    pred = torch.nn.functional.one_hot(labels, K).permute(0, 3, 1, 2).float()
    want = O.accuracies(pred, gt, bg=K - 1)
    for j in range(4):
        assert abs(float(got[j]) - float(want[j])) <= 1e-6
    per_image = ops.image_accuracies_from_counts(counts)
    assert per_image[1].tolist() == [0.0, 0.0, 0.5, 0.5]
    with pytest.raises(ValueError):
        ops.accuracies_from_counts(counts[:, :5])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _meter_batches():
    """Five batches of (B,6) counts; batch 0 holds two images with very different union sizes (a tiny one scored 1, a huge one 0.1)."""
    g = torch.Generator().manual_seed(9)
    batches = [torch.tensor([[10, 10, 10, 5, 5, 8], [100_000, 400_000, 1_000_000, 7, 9, 11]], dtype=torch.int64)]
    for B in (3, 1, 4, 2):
        union = torch.randint(1, 5_000_000_000, (B, 2), generator=g)                  # sums beyond 2^32: the halves must recombine
        part = (torch.rand(B, 4, generator=g) * union[:, [0, 0, 1, 1]]).long()
        batches.append(torch.stack([part[:, 0], part[:, 1], union[:, 0], part[:, 2], part[:, 3], union[:, 1]], 1))
    return batches


def _meter_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    meter = T.FullResMeter("cpu")
    batches = _meter_batches()
    for b in (batches[:3] if rank == 0 else batches[3:]):                             # three batches on rank 0, two on rank 1
        meter.update(b)
    out[rank] = (meter.result(), meter.result(reduce=False))
    dist.barrier()
    dist.destroy_process_group()


def test_full_res_meter_two_gloo_ranks():
    batches = _meter_batches()
    single = T.FullResMeter("cpu")
    for b in batches:
        single.update(b)
    want = single.result()
    total = torch.cat(batches)
    assert want["counts"] == total.sum(0).tolist() and want["images"] == 12
    mean = ops.image_accuracies_from_counts(total).double().mean(0)
    for j, k in enumerate(NAMES):
        assert abs(want[k] - float(mean[j])) <= 1e-12 * abs(float(mean[j]))
    assert want["iou_fg"] == int(total[:, 0].sum()) / int(total[:, 2].sum())
    assert want["iou_bin_fg"] == int(total[:, 1].sum()) / int(total[:, 2].sum())

    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_meter_worker, args=(world, port, out), nprocs=world, join=True)
    for rank in range(world):
        got, own = out[rank]
        assert got["counts"] == want["counts"] and got["images"] == want["images"]   # integer sums: exact
        assert got["iou_fg"] == want["iou_fg"] and got["iou_bin_fg"] == want["iou_bin_fg"]
        for k in NAMES:
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
        assert own["images"] == 6 and own["counts"] != want["counts"]                 # reduce=False: this rank's own six images

    # the dataset-level IoU is not the mean of the images' accuracies: the tiny image scores 1, the huge one 0.1
    two = T.FullResMeter("cpu")
    two.update(batches[0])
    r = two.result(reduce=False)
    assert abs(r["acc"] - 0.55) <= 1e-7
    assert r["iou_fg"] == 100_010 / 1_000_010 and abs(r["iou_fg"] - r["acc"]) > 0.4
    assert r["iou_bin_fg"] == 400_010 / 1_000_010
    assert T.FullResMeter("cpu").result(reduce=False)["iou_fg"] == 0.0               # nothing seen: an empty union scores 0
    with pytest.raises(ValueError):
        two.update(batches[0][:, :4])


def test_symbols_are_declared_everywhere():
    header = open(os.path.join(os.path.dirname(GOLD), os.pardir, "include", "fovealseg.h")).read()
    for name in ("fs_unwarp_accuracy", "fs_unwarp_accuracy_scratch_ints"):
        assert name + "(" in header
    assert "fs_unwarp_accuracy" in hip.SIGNATURES and "fs_unwarp_accuracy_scratch_ints" in hip.HOST_ONLY
    assert len(hip.SIGNATURES["fs_unwarp_accuracy"]) == 15                            # nine pointers and six ints before the stream


# ------------------------------------------------------------------------------------------------------------------ GPU: op -------
def _inputs(B, K, h, w, seed, lo=-1.1, hi=1.1):
    g = torch.Generator().manual_seed(seed)
    grid = (torch.rand(B, h, w, 2, generator=g) * (hi - lo) + lo).clamp(-1, 1)
    cls = torch.randn(B, K, generator=g)
    cls[:, K - 1] = 3 * cls.abs().amax(1)            # the mask plane decides where m is large, a constant class elsewhere
    m = torch.rand(B, h, w, generator=g) - 0.5
    return cls.cuda(), m.cuda(), grid.cuda()


def _labels_for(B, K, Hs, Ws, seed):
    """A blocky random {0,1} mask (B,1,Hs,Ws) and class labels (B,1) below the background class."""
    g = torch.Generator().manual_seed(seed + 77)
    coarse = (torch.rand(B, 1, (Hs + 7) // 8, (Ws + 7) // 8, generator=g) < 0.4).float()
    y = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :Hs, :Ws].contiguous()
    cl = torch.randint(0, K - 1, (B, 1), generator=g)
    return y.cuda(), cl.cuda()


def _check(cls, m, grid, y, cl):
    """Counts and labels bit for bit against the unfused route, acc against SegLoss's own where SegLoss can run (K <= 64)."""
    B, K = cls.shape
    Hs, Ws = int(y.shape[-2]), int(y.shape[-1])
    counts, acc, labels = ops.unwarp_accuracy(cls, m, grid, y, cl, return_labels=True)
    assert counts.dtype == torch.int64 and counts.shape == (B, 6) and acc.dtype == torch.float32 and acc.shape == (4,)
    pred_full, _ = ops.unwarp_nearest(ops.PredAssemble.apply(cls, m), grid, Hs, Ws)
    gt = compose_gt(y.reshape(B, Hs, Ws), cl, K)
    want = counts_ref(pred_full.argmax(1), gt, K)
    assert torch.equal(counts, want), (counts.tolist(), want.tolist())
    assert labels.dtype == torch.int64 and torch.equal(labels, ops.unwarp_labels(cls, m, grid, Hs, Ws)[0])
    plain = ops.unwarp_accuracy(cls, m, grid, y, cl)
    assert len(plain) == 2 and torch.equal(plain[0], counts) and torch.equal(plain[1], acc)
    assert bool((counts[:, 2] + counts[:, 5] >= Hs * Ws).all())                       # every pixel is in one union at least
    err = float((acc.cpu() - ops.accuracies_from_counts(counts.cpu())).abs().max())
    assert err <= 1e-6, err
    if K <= 64:
        ref = ops.SegLoss.apply(pred_full, gt.contiguous(), 5.0)[3:7]
        err = float((acc - ref).abs().max())
        print(f"acc vs SegLoss: {err:.2e}  {[round(float(v), 6) for v in acc]}")
        assert err <= 1e-6, (acc.tolist(), ref.tolist())
    return counts, acc, labels


@pytest.mark.gpu
def test_unwarp_accuracy_g14_grid():
    g = {k: v for k, v in np.load(os.path.join(GOLD, "g14_inverse.npz")).items()}
    Hs, Ws = (int(v) for v in g["seg"])
    grid = torch.from_numpy(g["grid"]).cuda()
    B, h, w, _ = grid.shape
    cls, m, _ = _inputs(B, 51, h, w, 14)
    y, cl = _labels_for(B, 51, Hs, Ws, 14)
    counts, _, labels = _check(cls, m, grid, y, cl)
    assert len(labels.unique()) >= 2 and int(counts[:, 0].sum()) + int(counts[:, 3].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 6), (50, 513, 3), (8, 1500, 2)])
def test_unwarp_accuracy_ragged_widths(Hs, Ws, K):
    cls, m, grid = _inputs(2, K, 9, 11, Hs * 1000 + Ws)
    y, cl = _labels_for(2, K, Hs, Ws, Hs)
    _check(cls, m, grid, y, cl)


@pytest.mark.gpu
def test_unwarp_accuracy_full_size():
    cls, m, grid = _inputs(2, 51, 80, 80, 7, -1.0, 1.0)
    y, cl = _labels_for(2, 51, 1024, 1024, 7)
    counts, _, labels = _check(cls, m, grid, y, cl)
    assert len(labels.unique()) >= 2 and int(counts[:, 2].min()) > 0 and int(counts[:, 5].min()) > 0


@pytest.mark.gpu
def test_unwarp_accuracy_output_smaller_than_grid():
    cls, m, grid = _inputs(2, 51, 80, 80, 8)
    y, cl = _labels_for(2, 51, 24, 20, 8)
    _check(cls, m, grid, y, cl)


@pytest.mark.gpu
def test_unwarp_accuracy_border_grids():
    g = torch.Generator().manual_seed(5)
    grid = torch.rand(2, 16, 20, 2, generator=g) * 2 - 1
    edge = torch.rand(2, 16, 20, 2, generator=g)
    grid = torch.where(edge < 0.3, torch.full_like(grid, -1.0), torch.where(edge > 0.7, torch.ones_like(grid), grid))
    cls = torch.randn(2, 7, generator=g)
    cls[:, 6] = 3 * cls.abs().amax(1)
    m = torch.rand(2, 16, 20, generator=g) - 0.5
    y, cl = _labels_for(2, 7, 45, 70, 5)
    _check(cls.cuda(), m.cuda(), grid.cuda(), y, cl)


@pytest.mark.gpu
def test_unwarp_accuracy_no_claimed_pixel():
    # image 1's grid lies outside [-1, 1]: nothing is claimed there, every pixel keeps the decision at (0, 0)
    cls, m, grid = _inputs(2, 9, 10, 12, 3)
    grid[1] = 1.5
    y, cl = _labels_for(2, 9, 31, 40, 3)
    _, _, labels = _check(cls, m, grid, y, cl)
    assert len(labels[1].unique()) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 51, 150])
def test_unwarp_accuracy_class_counts(K):
    # K = 150 is beyond SegLoss's 64 classes: counts and labels against the torch route only
    cls, m, grid = _inputs(3, K, 40, 40, K)
    y, cl = _labels_for(3, K, 300, 200, K)
    _, _, labels = _check(cls, m, grid, y, cl)
    assert len(labels.unique()) >= 2


@pytest.mark.gpu
def test_unwarp_accuracy_truncates_the_mask():
    # y.long() truncates: 0.5 is background, 1.5 the instance
    cls, m, grid = _inputs(2, 6, 9, 11, 31)
    y, cl = _labels_for(2, 6, 40, 52, 31)
    frac = torch.where(y > 0, torch.full_like(y, 1.5), torch.full_like(y, 0.5))
    frac[:, :, ::2] = y[:, :, ::2]                   # 0 / 1 on the even rows, 0.5 / 1.5 on the odd ones
    got = _check(cls, m, grid, frac, cl)
    want = ops.unwarp_accuracy(cls, m, grid, y, cl)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # (B,Hs,Ws) and (B,) spellings of the same arguments
    again = ops.unwarp_accuracy(cls, m, grid, y[:, 0], cl[:, 0])
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0.0, 1.0])
def test_unwarp_accuracy_constant_labels(fill):
    cls, m, grid = _inputs(2, 51, 12, 12, 41)
    y = torch.full((2, 1, 64, 48), fill, device="cuda")
    cl = torch.tensor([[3], [17]], device="cuda")
    counts, acc, _ = _check(cls, m, grid, y, cl)
    if fill == 0.0:
        assert bool((counts[:, 0] == 0).all()) and bool((counts[:, 5] == 64 * 48).all())       # no foreground in the label
    else:
        assert bool((counts[:, 3] == 0).all()) and bool((counts[:, 2] == 64 * 48).all())       # no background in the label
    assert bool(torch.isfinite(acc).all())


@pytest.mark.gpu
def test_unwarp_accuracy_is_deterministic():
    cls, m, grid = _inputs(4, 51, 80, 80, 12, -1.0, 1.0)
    y, cl = _labels_for(4, 51, 512, 768, 12)
    a = ops.unwarp_accuracy(cls, m, grid, y, cl)
    b = ops.unwarp_accuracy(cls, m, grid, y, cl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_unwarp_accuracy_rejects_bad_arguments():
    cls, m, grid = _inputs(1, 4, 4, 4, 0)
    y, cl = _labels_for(1, 4, 8, 8, 0)
    with pytest.raises(ValueError):                  # m not at the grid's resolution
        ops.unwarp_accuracy(cls, m[:, :3], grid, y, cl)
    with pytest.raises(ValueError):                  # y: another batch size, not a label mask
        ops.unwarp_accuracy(cls, m, grid, y.repeat(2, 1, 1, 1), cl)
    with pytest.raises(ValueError):
        ops.unwarp_accuracy(cls, m, grid, y.repeat(1, 2, 1, 1), cl)
    with pytest.raises(ValueError):                  # one class label per image
        ops.unwarp_accuracy(cls, m, grid, y, cl.repeat(2, 1))
    with pytest.raises(hip.HipLibraryError):         # K < 2
        ops.unwarp_accuracy(cls[:, :1], m, grid, y, cl)
    big = torch.randn(1, 1025, device="cuda")
    with pytest.raises(hip.HipLibraryError):         # K beyond the kernel's 1 024
        ops.unwarp_accuracy(big, m, grid, y, cl)
    ops.unwarp_accuracy(big[:, :1024].contiguous(), m, grid, y, cl)
    with pytest.raises(hip.HipLibraryError):         # a row longer than the row pass's LDS
        ops.unwarp_accuracy(cls, m, grid, torch.zeros(1, 1, 1, 16385, device="cuda"), cl)
    counts = torch.empty(1, 6, device="cuda", dtype=torch.int64)
    acc = torch.empty(4, device="cuda")
    scr = torch.empty(hip.query("fs_unwarp_accuracy_scratch_ints", 1, 4, 4, 8, 8), device="cuda", dtype=torch.int32)
    assert scr.numel() >= hip.query("fs_unwarp_labels_scratch_ints", 1, 4, 4, 8, 8) + 8
    args = (cls.data_ptr(), m.data_ptr(), grid.data_ptr(), y.data_ptr(), cl.data_ptr(), counts.data_ptr(), acc.data_ptr(), None)
    with pytest.raises(hip.HipLibraryError):         # no scratch
        hip.call("fs_unwarp_accuracy", *args, None, 1, 4, 4, 4, 8, 8)
    with pytest.raises(hip.HipLibraryError):         # no label mask
        hip.call("fs_unwarp_accuracy", *args[:3], None, *args[4:], scr.data_ptr(), 1, 4, 4, 4, 8, 8)
    hip.call("fs_unwarp_accuracy", *args, scr.data_ptr(), 1, 4, 4, 4, 8, 8)                     # the class map is optional
    assert torch.equal(counts, ops.unwarp_accuracy(cls, m, grid, y, cl)[0])


# ------------------------------------------------------------------------------------------------------------------ GPU: module ---
def _cfg(kind):
    cfg = fovealseg.lvis50_cfg()
    if kind == "segformer":
        cfg.MODEL.arch_encoder, cfg.MODEL.fc_dim = "segformer", 1024
        cfg.TRAIN.task_input_size = (160, 160)
    elif kind == "deeplab":
        cfg.MODEL.arch_encoder = "deeplab"
    elif kind == "uniform":
        cfg.MODEL.uniform_sample = "Saliency"
    elif kind == "upsample":
        cfg.MODEL.upsample = True
    return cfg


_MODULES = {}


def _module(kind):
    if kind not in _MODULES:
        _MODULES.clear()                             # one module at a time on the device
        torch.cuda.empty_cache()
        _MODULES[kind] = T.build_module(_cfg(kind), device="cuda")
    module, nets = _MODULES[kind]
    module.eval()
    return module, nets


@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,seg", [("hrnet", 256, None), ("segformer", 256, (200, 180)), ("deeplab", 128, None),
                                           ("uniform", 192, None)])
def test_evaluate_equals_predict_and_a_torch_count(kind, size, seg, deterministic):
    module, _ = _module(kind)
    K = module.cfg.DATASET.num_class
    X, Fp, Y, cl = T.synthetic_batch(2, size, size, seed=11, device="cuda")
    if seg is not None:                              # a non-square label at seg_size, the image at its own size
        _, _, Y, _ = T.synthetic_batch(2, seg[0], seg[1], seed=11, device="cuda")
    keep = [t.clone() for t in (X, Fp, Y, cl)]
    state = {k: v.detach().clone() for k, v in module.state_dict().items()}
    step0 = ops.DropoutState.step
    out = module.evaluate(X, Fp, Y, cl, seg, return_labels=True)
    module.check_nan()
    assert len(out) == 6 and all(v.dim() == 0 and v.dtype == torch.float32 for v in out[:4])
    counts, labels = out[4], out[5]
    want = module.predict(X, Fp, seg)
    assert torch.equal(labels, want)
    assert torch.equal(counts, counts_ref(want, compose_gt(Y[:, 0], cl, K), K))
    acc = ops.accuracies_from_counts(counts.cpu())
    assert float((torch.stack(out[:4]).cpu() - acc).abs().max()) <= 1e-6
    short = module.evaluate(X, Fp, Y[:, 0], cl[:, 0])                                 # no class map; (B,H,W) and (B,) spellings
    assert len(short) == 5 and torch.equal(short[4], counts) and all(torch.equal(a, b) for a, b in zip(short[:4], out[:4]))
    for t, k in zip((X, Fp, Y, cl), keep):
        assert torch.equal(t, k)                                                      # nothing written back into an argument
    assert ops.DropoutState.step == step0
    for k, v in module.state_dict().items():
        assert torch.equal(v, state[k]), k
    stepped = T.evaluate_step(module, (X, Fp, Y, cl))
    assert torch.equal(stepped[4], counts)


@pytest.mark.gpu
def test_evaluate_rejects_train_mode_and_bad_arguments():
    module, _ = _module("hrnet")
    X, Fp, Y, cl = T.synthetic_batch(2, 96, 96, seed=3, device="cuda")
    module.train()
    try:
        with pytest.raises(RuntimeError):
            module.evaluate(X, Fp, Y, cl)
    finally:
        module.eval()
    with pytest.raises(ValueError):
        module.evaluate(X, Fp, Y, cl, (96, 80))                                       # seg_size other than the label's
    with pytest.raises(ValueError):
        module.evaluate(X, Fp, Y[:, :, :80], cl, (96, 96))
    with pytest.raises(ValueError):
        module.evaluate(X, Fp[:1], Y, cl)                                             # batch mismatches
    with pytest.raises(ValueError):
        module.evaluate(X, Fp, Y[:1], cl)
    with pytest.raises(ValueError):
        module.evaluate(X, Fp, Y, cl[:1])
    module.evaluate(X, Fp, Y, cl, (96, 96))


@pytest.mark.gpu
def test_evaluate_step_feeds_the_meter():
    module, _ = _module("hrnet")
    meter = T.FullResMeter("cuda")
    rows = []
    for seed, B in ((1, 2), (2, 3)):
        out = T.evaluate_step(module, T.synthetic_batch(B, 128, 128, seed=seed, device="cuda"), meter)
        rows.append(out[4].cpu())
    res = meter.result()
    total = torch.cat(rows)
    assert res["images"] == 5 and res["counts"] == total.sum(0).tolist()
    mean = ops.image_accuracies_from_counts(total).double().mean(0)
    for j, k in enumerate(NAMES):
        assert abs(res[k] - float(mean[j])) <= 1e-12 * max(abs(float(mean[j])), 1e-30)
    assert res["iou_fg"] == int(total[:, 0].sum()) / max(int(total[:, 2].sum()), 1)


def _parent_upsample_branch(module, X, Fp, Y, cl):
    """The branch forward(MODEL.upsample=True) had: unwarp_nearest + SegLoss chained by hand on the same pred and grid."""
    K = module.cfg.DATASET.num_class
    with torch.no_grad():
        xs, _ = module.saliency(X, Fp)
        grid = module.create_grid(xs)
        pred = module.decoder.forward_nhwc(module.encoder.forward_nhwc(ops.GridSample.apply(X, grid)))
        pred_full, _ = ops.unwarp_nearest(pred.contiguous(), grid, int(Y.shape[2]), int(Y.shape[3]))
        y_hs = Y[:, 0].long()
        gt_hs = y_hs * cl[:, :, None] + (1 - y_hs) * (K - 1)
        return ops.SegLoss.apply(pred_full, gt_hs.contiguous(), 5.0)[3:7]


@pytest.mark.gpu
def test_forward_upsample_equals_the_parents_branch(deterministic):
    module, _ = _module("upsample")
    X, Fp, Y, cl = T.synthetic_batch(2, 192, 192, seed=17, device="cuda")

    def feed():
        return {"img_data": X, "seg_label": Y.clone(), "focus_point": Fp, "cls_label": cl}
    with torch.no_grad():
        got = module(feed(), is_inference=True)
        module.cfg.MODEL.upsample = False            # the same forward without the branch: the loss path
        try:
            low = module(feed(), is_inference=True)
        finally:
            module.cfg.MODEL.upsample = True
    module.check_nan()
    assert len(got) == 6
    assert torch.equal(got[0], low[0]) and torch.equal(got[2], low[2])                # loss, edge loss
    want = _parent_upsample_branch(module, X, Fp, Y, cl)
    diff = [abs(float(got[j]) - float(want[i])) for i, j in enumerate((1, 3, 4, 5))]
    print(f"forward(upsample=True) vs unwarp_nearest + SegLoss: {diff}")
    assert max(diff) <= 1e-6
    ev = module.evaluate(X, Fp, Y, cl)
    assert all(torch.equal(ev[i], got[j]) for i, j in enumerate((1, 3, 4, 5)))        # evaluate is that branch without the loss


@pytest.mark.gpu
def test_evaluate_against_the_oracle():
    """tests/test_next_rows.py::test_upsample_branch_full_resolution_accuracies' batch and bound."""
    module, _ = _module("hrnet")
    o = O.OracleDeformSeg()
    fovealseg.weights.apply_name_keyed_init(o)
    o.eval()
    X, Fp, Y, cl = T.synthetic_batch(2, 160, 160, seed=21, device="cpu")
    got = module.evaluate(X.cuda(), Fp.cuda(), Y.cuda(), cl.cuda())
    module.check_nan()
    with torch.no_grad():
        ref = o({"img_data": X, "seg_label": Y.clone(), "focus_point": Fp, "cls_label": cl}, is_inference=True, upsample=True)
    got = np.array([float(v) for v in got[:4]])
    ref = np.array([float(ref[j]) for j in (1, 3, 4, 5)])
    print(f"evaluate vs oracle: {np.abs(got - ref).tolist()}  (evaluate {got.tolist()})")
    assert np.abs(got - ref).max() <= 5e-3, (got, ref)


@pytest.mark.gpu
def test_evaluate_allocates_no_more_than_predict():
    module, _ = _module("hrnet")
    X, Fp, Y, cl = T.synthetic_batch(2, 2048, 2048, seed=9, device="cuda")
    with torch.no_grad():
        def stages():
            xs, _ = module.saliency(X, Fp)
            grid = module.create_grid(xs)
            return module.decoder.forward_parts_nhwc(module.encoder.forward_nhwc(ops.GridSample.apply(X, grid)))

        def peak_of(fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            out = fn()
            torch.cuda.synchronize()
            return out, torch.cuda.max_memory_allocated()
        stages()
        module.predict(X, Fp)                                                         # warm-up: weight packs, workspaces
        module.evaluate(X, Fp, Y, cl)
        parts, base = peak_of(stages)
        del parts
        labels, peak_predict = peak_of(lambda: module.predict(X, Fp))
        del labels
        out, peak_evaluate = peak_of(lambda: module.evaluate(X, Fp, Y, cl))
    module.check_nan()
    extra_predict, extra_evaluate = (peak_predict - base) / 2 ** 30, (peak_evaluate - base) / 2 ** 30
    print(f"peak over the stages' peak: evaluate {extra_evaluate:.3f} GB, predict {extra_predict:.3f} GB")
    assert out[4].shape == (2, 6)
    assert extra_evaluate <= extra_predict           # the same two int32 maps, no int64 class map; the workgroup records are small
    assert extra_evaluate < 0.3                      # the (B, 51, 2048, 2048) fp32 prediction alone would be 1.6 GiB
