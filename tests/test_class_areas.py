"""Per-class IoU / Dice, the sampling ceiling and the sampled-space areas in evaluate() (eval.py:218-257,313-331; utils.py:289-317;
models/models_instance.py:909-918): ops.unwarp_class_areas (fs_unwarp_class_areas), ops.class_scores_from_areas,
DeformSegmentationModule.evaluate(class_areas=True), train.ClassIoUMeter and train.evaluate_step(class_meter=...).

tests/class_area_ref.py restates utils.intersectionAndUnion as counts by equality; tests/golden/g19_class_areas.npz holds what the
reference's function itself returns.  CPU: the restatement against the fixture bit for bit, the quotients, the meter alone and over two
gloo ranks.  GPU: areas against the restatement applied to three class maps made by the unfused ops -- space 0 ops.unwarp_labels' map,
space 1 a gather of ops.grid_sample_label through ops.inverse_grid's owner map with fs_fill_nearest behind it, space 2
PredAssemble(cls, m).argmax(1) -- every check an equality of integers; only the fp64 quotients carry a tolerance (1e-12)."""
import inspect
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

import class_area_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g19():
    g = np.load(os.path.join(GOLD, "g19_class_areas.npz"), allow_pickle=False)
    cases = []
    for n in g["names"]:
        cases.append({"name": str(n), "K": int(g[f"{n}/K"]), "cl": int(g[f"{n}/cls_label"]), "t": g[f"{n}/t"].astype(np.int64),
                      "pred": g[f"{n}/pred"].astype(np.int64), "inter": g[f"{n}/intersection"], "union": g[f"{n}/union"],
                      "lab": g[f"{n}/area_lab"], "img_iou": g[f"{n}/img_iou"]})
    dataset = {K: (g[f"dataset/{K}/iou"], g[f"dataset/{K}/dice"]) for K in sorted({c["K"] for c in cases})}
    return cases, dataset


# ------------------------------------------------------------------------------------------------------------------ CPU ----------
def test_restatement_reproduces_the_reference_exactly():
    cases, _ = _g19()
    assert len(cases) == 10 and {c["K"] for c in cases} == {2, 3, 51, 150, 1024}
    seen = set()
    for c in cases:
        K = c["K"]
        gt = R.compose_gt(c["t"][None], [c["cl"]], K)[0]
        inter, union, lab = R.intersection_and_union(c["pred"], gt, K)
        assert np.array_equal(inter, c["inter"]) and np.array_equal(union, c["union"]) and np.array_equal(lab, c["lab"]), c["name"]
        a = R.areas(c["pred"], gt, K)
        assert a.dtype == np.int64 and a[:, 1].sum() == gt.size and a[:, 2].sum() == gt.size
        assert np.array_equal(R.scores(a)[0], c["img_iou"]), c["name"]
        if c["t"].min() == c["t"].max():
            seen.add("constant")
        if inter.sum() == 0:
            seen.add("never hits")
        if c["cl"] == K - 1:
            seen.add("cl at K-1")
            assert lab[K - 1] == gt.size                                               # one merged row, counted once
    assert seen == {"constant", "never hits", "cl at K-1"}


def _golden_areas(K):
    """(n, 3, K, 3) int64: the fixture's pairs of one K as areas, the same triple in all three spaces."""
    cases, dataset = _g19()
    rows = [R.areas(c["pred"], R.compose_gt(c["t"][None], [c["cl"]], K)[0], K) for c in cases if c["K"] == K]
    return torch.from_numpy(np.stack(rows))[:, None].repeat(1, 3, 1, 1), [c for c in cases if c["K"] == K], dataset[K]


@pytest.mark.parametrize("K", [2, 3, 51, 150, 1024])
def test_scores_and_meter_reproduce_the_golden(K):
    areas, cases, (ds_iou, ds_dice) = _golden_areas(K)
    iou, dice = ops.class_scores_from_areas(areas)
    assert iou.dtype == torch.float64 and iou.shape == (len(cases), 3, K) and dice.shape == iou.shape
    for i, c in enumerate(cases):
        for s in range(3):
            assert np.abs(iou[i, s].numpy() - c["img_iou"]).max() <= 1e-12, c["name"]
    assert np.abs(np.stack(R.scores(areas.numpy())) - np.stack([iou.numpy(), dice.numpy()])).max() <= 1e-12
    meter = T.ClassIoUMeter("cpu", K)
    for i in range(len(cases)):                                                        # one image at a time
        meter.update(areas[i:i + 1])
    r = meter.result(reduce=False)
    assert r["images"] == len(cases)
    total = areas.sum(0)
    union = (total[..., 1] + total[..., 2] - total[..., 0]).numpy()
    for s, name in enumerate(T.ClassIoUMeter.SPACES):
        got = r[name]
        assert got["areas"] == total[s].tolist()
        assert np.abs(np.array(got["iou"]) - ds_iou).max() <= 1e-12 and np.abs(np.array(got["dice"]) - ds_dice).max() <= 1e-12
        assert abs(got["miou"] - ds_iou.mean()) <= 1e-12 and abs(got["mdice"] - ds_dice.mean()) <= 1e-12
        present = union[s] > 0
        assert abs(got["miou_present"] - ds_iou[present].mean()) <= 1e-12
    lab = areas[:, 0, :, 2].double()
    share = (lab / lab.sum(1, keepdim=True)).mean(0) * 100.0
    assert np.abs(np.array(r["label_share_full"]) - share.numpy()).max() <= 1e-12
    assert np.abs(np.array(r["label_share_sampled"]) - share.numpy()).max() <= 1e-12
    assert max(abs(v) for v in r["label_share_shift"]) <= 1e-12 and abs(sum(r["label_share_full"]) - 100.0) <= 1e-9


def test_scores_and_meter_on_hand_made_areas():
    big = 5_000_000_000                                                                # sums beyond 2^32
    a = torch.zeros(2, 3, 4, 3, dtype=torch.int64)
    a[0, 0] = torch.tensor([[3, 5, 4], [0, 0, 0], [0, 2, 0], [10, 13, 16]])
    a[1, 0] = torch.tensor([[big, big + 7, big + 9], [0, 0, 0], [0, 0, 0], [1, 10, 8]])
    a[:, 1] = a[:, 0]
    a[0, 2] = torch.tensor([[1, 2, 1], [0, 0, 0], [0, 0, 0], [3, 3, 4]])
    a[1, 2] = torch.tensor([[0, 0, 5], [0, 0, 0], [0, 0, 0], [0, 5, 0]])
    iou, dice = ops.class_scores_from_areas(a)
    assert iou[0, 0].tolist() == [3 / (6 + 1e-10), 0.0, 0.0, 10 / (19 + 1e-10)] and dice[0, 0, 0].item() == 6 / (9 + 1e-10)
    with pytest.raises(ValueError):
        ops.class_scores_from_areas(a[..., :2])
    meter = T.ClassIoUMeter("cpu", 4)
    meter.update(a[:1])
    meter.update(a[1:])
    r = meter.result(reduce=False)
    assert r["images"] == 2 and r["full"]["areas"] == a[:, 0].sum(0).tolist() and r["sampled"]["areas"] == a[:, 2].sum(0).tolist()
    assert r["full"]["areas"][0][0] == big + 3
    u0 = (big + 12) + (big + 13) - (big + 3)
    assert r["full"]["iou"][0] == (big + 3) / (u0 + 1e-10) and r["full"]["iou"][1] == 0.0
    assert r["full"]["miou"] == sum(r["full"]["iou"]) / 4
    present = [r["full"]["iou"][k] for k in (0, 2, 3)]                                 # class 1 has an empty union
    assert abs(r["full"]["miou_present"] - sum(present) / 3) <= 1e-15
    assert abs(r["label_share_full"][0] - 100.0 * (4 / 20 + (big + 9) / (big + 17)) / 2) <= 1e-12
    assert abs(r["label_share_sampled"][3] - 100.0 * (4 / 5 + 0.0) / 2) <= 1e-12
    assert abs(r["label_share_shift"][3] - (r["label_share_sampled"][3] - r["label_share_full"][3])) == 0.0
    empty = T.ClassIoUMeter("cpu", 4).result(reduce=False)
    assert empty["images"] == 0 and empty["full"]["miou"] == 0.0 and np.isnan(empty["full"]["miou_present"]) and np.isnan(empty["label_share_full"][0])
    with pytest.raises(ValueError):
        meter.update(a[:, :2])
    with pytest.raises(ValueError):
        T.ClassIoUMeter("cpu", 5).update(a)
    with pytest.raises(ValueError):
        T.ClassIoUMeter("cpu", 1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _meter_batches():
    g = torch.Generator().manual_seed(19)
    out = []
    for B in (2, 3, 1, 4, 2):
        inter = torch.randint(0, 3_000_000_000, (B, 3, 7, 1), generator=g)
        more = torch.randint(0, 3_000_000_000, (B, 3, 7, 2), generator=g)
        out.append(torch.cat([inter, inter + more], 3))
    out[1][0, :, 2] = 0                                                                 # a class absent from one image
    return out


def _meter_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    meter = T.ClassIoUMeter("cpu", 7)
    batches = _meter_batches()
    for b in (batches[:3] if rank == 0 else batches[3:]):                               # three batches on rank 0, two on rank 1
        meter.update(b)
    out[rank] = (meter.result(), meter.result(reduce=False))
    dist.barrier()
    dist.destroy_process_group()


def test_class_iou_meter_two_gloo_ranks():
    batches = _meter_batches()
    single = T.ClassIoUMeter("cpu", 7)
    for b in batches:
        single.update(b)
    want = single.result()
    total = torch.cat(batches).sum(0)
    assert want["images"] == 12 and all(want[n]["areas"] == total[s].tolist() for s, n in enumerate(T.ClassIoUMeter.SPACES))
    assert int(total.max()) > 2 ** 32
    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_meter_worker, args=(world, port, out), nprocs=world, join=True)
    for rank in range(world):
        got, own = out[rank]
        assert got["images"] == 12 and own["images"] == 6
        for n in T.ClassIoUMeter.SPACES:                                               # integer sums: exact, and so every quotient of them
            assert got[n]["areas"] == want[n]["areas"] and got[n]["iou"] == want[n]["iou"] and got[n]["dice"] == want[n]["dice"]
            assert got[n]["miou"] == want[n]["miou"] and got[n]["miou_present"] == want[n]["miou_present"]
            assert own[n]["areas"] != want[n]["areas"]
        for k in ("label_share_full", "label_share_sampled", "label_share_shift"):
            for a, b in zip(got[k], want[k]):
                assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (k, a, b)


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(GOLD), os.pardir, "include", "fovealseg.h")).read()
    for name in ("fs_unwarp_class_areas", "fs_unwarp_class_areas_scratch_ints"):
        assert name + "(" in header
    for cite in ("eval.py:218-257,313-322", "utils.py:289-317", "models/models_instance.py:909-918"):
        assert cite in header
    assert hip.SIGNATURES["fs_unwarp_class_areas"] == "p" * 11 + "i" * 8
    assert "fs_unwarp_class_areas_scratch_ints" in hip.HOST_ONLY
    lib = hip.load()
    assert lib.fs_unwarp_class_areas_scratch_ints(0, 51, 4, 4, 64, 64) == 0
    extra = lib.fs_unwarp_class_areas_scratch_ints(2, 51, 4, 4, 64, 64) - lib.fs_unwarp_trimap_scratch_ints(2, 4, 4, 64, 64)
    assert 2 * 4 * 8 + 2 * 51 <= extra <= 2 * 4 * 8 + 2 * 51 + 8                        # a 32-byte record per workgroup, the (B,K) table


def test_signatures():
    sig = inspect.signature(fovealseg.DeformSegmentationModule.evaluate)
    assert sig.parameters["class_areas"].default is False
    sig = inspect.signature(T.evaluate_step)
    assert list(sig.parameters) == ["module", "batch", "meter", "trimap_meter", "class_meter"] and sig.parameters["class_meter"].default is None
    sig = inspect.signature(ops.unwarp_class_areas)
    assert sig.parameters["dia_factor"].default is None and sig.parameters["frame"].default is True and sig.parameters["return_labels"].default is False


class _Recorder:
    """Stands in for the module: records how evaluate is called."""

    def __init__(self):
        self.calls = []

    def evaluate(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return tuple(range(5)) + (("trim",) if "trimap" in kwargs else ()) + ((torch.zeros(2, 3, 4, 3, dtype=torch.int64),) if kwargs.get("class_areas") else ())

    def check_nan(self):
        pass


def test_evaluate_step_without_class_meter_calls_evaluate_as_before():
    X, Fp, Y, cl = torch.zeros(2, 4, 8, 8), torch.zeros(2, 2), torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, dtype=torch.int64)
    rec = _Recorder()
    out = T.evaluate_step(rec, (X, Fp, Y, cl))
    (args, kwargs), = rec.calls
    assert kwargs == {} and len(args) == 4 and args[0].shape == (2, 3, 8, 8) and args[1] is Fp and args[2] is Y and args[3] is cl
    assert out == tuple(range(5))

    class _Trim:
        dia_factor, frame = 3, False

        def update(self, v):
            self.got = v
    tm = _Trim()
    T.evaluate_step(rec, (X, Fp, Y, cl), None, tm)
    assert rec.calls[1][1] == {"trimap": 3, "trimap_frame": False} and tm.got == "trim"
    meter = T.ClassIoUMeter("cpu", 4)
    out = T.evaluate_step(rec, (X, Fp, Y, cl), None, tm, meter)
    assert rec.calls[2][1] == {"trimap": 3, "trimap_frame": False, "class_areas": True} and len(out) == 7
    T.evaluate_step(rec, (X, Fp, Y, cl), class_meter=meter)
    assert rec.calls[3][1] == {"class_areas": True} and meter.result(reduce=False)["images"] == 4


# ------------------------------------------------------------------------------------------------------------------ GPU: op -------
def _inputs(B, K, h, w, seed, lo=-1.1, hi=1.1, dominant=True):
    g = torch.Generator().manual_seed(seed)
    grid = (torch.rand(B, h, w, 2, generator=g) * (hi - lo) + lo).clamp(-1, 1)
    cls = torch.randn(B, K, generator=g)
    if dominant:
        cls[:, K - 1] = 3 * cls.abs().amax(1)        # the mask plane decides where m is large, a constant class elsewhere
    m = torch.rand(B, h, w, generator=g) - 0.5
    return cls.cuda(), m.cuda(), grid.cuda()


def _labels_for(B, K, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed + 77)
    coarse = (torch.rand(B, 1, (Hs + 7) // 8, (Ws + 7) // 8, generator=g) < 0.4).float()
    y = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :Hs, :Ws].contiguous()
    cl = torch.randint(0, K - 1, (B, 1), generator=g)
    return y.cuda(), cl.cuda()


def _three_maps(cls, m, grid, y, cl):
    """The three (class map, ground truth) pairs by the unfused ops, as numpy int64."""
    B, K = cls.shape
    _, h, w, _ = grid.shape
    Hs, Ws = int(y.shape[-2]), int(y.shape[-1])
    y4 = y.reshape(B, 1, Hs, Ws).float().contiguous()
    cln = cl.reshape(B).cpu().numpy()
    gt = R.compose_gt(y4[:, 0].long().cpu().numpy(), cln, K)
    full = ops.unwarp_labels(cls, m, grid, Hs, Ws)[0].cpu().numpy()
    ts = ops.grid_sample_label(y4, grid.contiguous())                                  # (B,h,w) int64: the training label of every point
    owner, _ = ops.inverse_grid(grid, Hs, Ws)
    vals = torch.gather(ts.reshape(B, h * w), 1, owner.reshape(B, -1).long().clamp(min=0))
    vals = (vals * (owner.reshape(B, -1) >= 0)).float().reshape(B, 1, Hs, Ws).contiguous()      # holes 0: an image without a claim stays background
    scratch = torch.empty(2 * B * Hs * Ws, device="cuda", dtype=torch.int32)
    hip.call("fs_fill_nearest", vals.data_ptr(), owner.data_ptr(), scratch.data_ptr(), B, 1, Hs, Ws)
    ceiling = R.compose_gt(vals[:, 0].long().cpu().numpy(), cln, K)
    sampled = ops.PredAssemble.apply(cls, m).argmax(1).cpu().numpy()
    gs = R.compose_gt(ts.cpu().numpy(), cln, K)
    return (full, gt), (ceiling, gt), (sampled, gs)


def _check(cls, m, grid, y, cl, trimap=True):
    B, K = cls.shape
    _, h, w, _ = grid.shape
    Hs, Ws = int(y.shape[-2]), int(y.shape[-1])
    counts, acc, areas, labels = ops.unwarp_class_areas(cls, m, grid, y, cl, return_labels=True)
    base = ops.unwarp_accuracy(cls, m, grid, y, cl, return_labels=True)
    assert torch.equal(counts, base[0]) and torch.equal(acc, base[1]) and torch.equal(labels, base[2])
    assert areas.dtype == torch.int64 and areas.shape == (B, 3, K, 3)
    want = np.stack([R.areas_batch(a, g, K) for a, g in _three_maps(cls, m, grid, y, cl)], 1)
    got = areas.cpu().numpy()
    for s in range(3):
        assert np.array_equal(got[:, s], want[:, s]), (s, np.argwhere(got[:, s] != want[:, s])[:8].tolist())
    # identities with the six counters and the pixel totals
    clv = cl.reshape(B).cpu()
    for b in range(B):
        c = int(clv[b])
        if 0 <= c < K - 1:                           # at K-1 the counters call the instance background
            assert int(areas[b, 0, c, 0]) == int(counts[b, 0])
        assert int(areas[b, 0, K - 1, 0]) == int(counts[b, 3])
        for s, total in ((0, Hs * Ws), (1, Hs * Ws), (2, h * w)):
            if s != 1 or 0 <= c < K:                 # a network's class is always a row; the ceiling's is cls_label where ts
                assert int(areas[b, s, :, 1].sum()) == total
            if 0 <= c < K:
                assert int(areas[b, s, :, 2].sum()) == total
    plain = ops.unwarp_class_areas(cls, m, grid, y, cl)                                 # no class map; the same bits twice
    assert len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(plain, (counts, acc, areas)))
    if trimap:
        with_trim = ops.unwarp_class_areas(cls, m, grid, y, cl, dia_factor=5, return_labels=True)
        tref = ops.unwarp_trimap(cls, m, grid, y, cl, 5, True)
        assert len(with_trim) == 5 and torch.equal(with_trim[3], tref[2]) and torch.equal(with_trim[4], labels)
        assert all(torch.equal(a, b) for a, b in zip(with_trim[:3], (counts, acc, areas)))
    # at the C ABI: areas pre-filled with a sentinel between guards, so that an unwritten row shows
    G = 8
    a_raw = torch.full((G + B * 3 * K * 3 + G,), -7, device="cuda", dtype=torch.int64)
    c2, acc2 = torch.empty_like(counts), torch.empty_like(acc)
    scr = torch.empty(hip.query("fs_unwarp_class_areas_scratch_ints", B, K, h, w, Hs, Ws), device="cuda", dtype=torch.int32)
    yc, clc = y.float().contiguous(), cl.long().contiguous()
    hip.call("fs_unwarp_class_areas", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), yc.data_ptr(), clc.data_ptr(), c2.data_ptr(),
             acc2.data_ptr(), a_raw.data_ptr() + 8 * G, None, None, scr.data_ptr(), B, K, h, w, Hs, Ws, -3, 9)      # D, frame ignored
    assert bool((a_raw[:G] == -7).all()) and bool((a_raw[-G:] == -7).all()), "guard overwritten"
    assert torch.equal(a_raw[G:-G], areas.flatten()) and torch.equal(c2, counts) and torch.equal(acc2, acc)
    return counts, areas, labels


@pytest.mark.gpu
def test_class_areas_g14_grid():
    g = {k: v for k, v in np.load(os.path.join(GOLD, "g14_inverse.npz")).items()}
    Hs, Ws = (int(v) for v in g["seg"])
    grid = torch.from_numpy(g["grid"]).cuda()
    B, h, w, _ = grid.shape
    cls, m, _ = _inputs(B, 51, h, w, 14)
    y, cl = _labels_for(B, 51, Hs, Ws, 14)
    _, areas, labels = _check(cls, m, grid, y, cl)
    assert len(labels.unique()) >= 2 and int(areas[:, 1, :, 0].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 6), (50, 513, 3), (8, 1500, 2)])
def test_class_areas_ragged_widths(Hs, Ws, K):
    cls, m, grid = _inputs(2, K, 9, 11, Hs * 1000 + Ws)
    y, cl = _labels_for(2, K, Hs, Ws, Hs)
    _check(cls, m, grid, y, cl)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 51, 150, 1024])
def test_class_areas_class_counts(K):
    cls, m, grid = _inputs(3, K, 40, 40, K)
    y, cl = _labels_for(3, K, 300, 200, K)
    _check(cls, m, grid, y, cl)                      # the hot regime: a dominant mask plane, one constant class elsewhere


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,h,Hs,Ws", [(48, 51, 12, 70, 52), (3, 150, 40, 300, 200), (2, 1024, 40, 300, 200)])
def test_class_areas_many_classes(B, K, h, Hs, Ws):
    """cls is plain randn: the last plane is not dominant, nearly every pixel takes its image's best constant class, and the LDS bins
    and the atomics carry most pixels.  (The planes below K-1 are constant, so one image predicts two classes at the most: the variety
    comes from the batch, whose images share one (B, K) table -- 48 images, at least 20 classes.)"""
    cls, m, grid = _inputs(B, K, h, h, K + 1, dominant=False)
    y, cl = _labels_for(B, K, Hs, Ws, K + 1)
    _, areas, labels = _check(cls, m, grid, y, cl, trimap=False)
    if B == 48:
        assert len(labels.unique()) >= 20
    cold = areas[:, 0, :, 1].clone()
    cold[:, K - 1] = 0
    cold[torch.arange(B, device="cuda"), cl.reshape(-1)] = 0
    assert int(cold.sum()) > B * Hs * Ws // 2                                           # classes other than cls_label and K-1


@pytest.mark.gpu
def test_class_areas_border_grids():
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
def test_class_areas_no_claimed_pixel():
    cls, m, grid = _inputs(2, 9, 10, 12, 3)
    grid[1] = 1.5                                    # image 1: nothing claimed; the ceiling is background everywhere
    y, cl = _labels_for(2, 9, 31, 40, 3)
    _, areas, _ = _check(cls, m, grid, y, cl)
    assert int(areas[1, 1, 8, 1]) == 31 * 40 and int(areas[1, 1, :8, 1].sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0.0, 1.0])
def test_class_areas_constant_labels(fill):
    cls, m, grid = _inputs(2, 51, 12, 12, 41)
    y = torch.full((2, 1, 64, 48), fill, device="cuda")
    cl = torch.tensor([[3], [17]], device="cuda")
    _, areas, _ = _check(cls, m, grid, y, cl)
    row = 50 if fill == 0.0 else 3
    assert int(areas[0, 0, row, 2]) == 64 * 48


@pytest.mark.gpu
def test_class_areas_truncates_the_mask():
    cls, m, grid = _inputs(2, 6, 9, 11, 31)
    y, cl = _labels_for(2, 6, 40, 52, 31)
    frac = torch.where(y > 0, torch.full_like(y, 1.5), torch.full_like(y, 0.5))
    frac[:, :, ::2] = y[:, :, ::2]                   # 0 / 1 on the even rows, 0.5 / 1.5 on the odd ones
    _check(cls, m, grid, frac, cl)
    got = ops.unwarp_class_areas(cls, m, grid, frac[:, 0], cl[:, 0])                    # (B,Hs,Ws) and (B,) spellings
    want = ops.unwarp_class_areas(cls, m, grid, y, cl)
    assert torch.equal(got[2][:, 0], want[2][:, 0])                                    # the full-resolution truth truncates to the same map


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["K-1", "K+3", "-1"])
def test_class_areas_cls_label_edge_cases(which):
    K = 9
    cls, m, grid = _inputs(3, K, 10, 12, 13)
    y, cl = _labels_for(3, K, 45, 70, 13)
    cl[1] = {"K-1": K - 1, "K+3": K + 3, "-1": -1}[which]
    _, areas, _ = _check(cls, m, grid, y, cl)
    fg = int(y[1].sum())
    assert fg > 0
    if which == "K-1":                                                                 # merged into the background row, counted once
        assert int(areas[1, 0, K - 1, 2]) == 45 * 70 and int(areas[1, 1, K - 1, 0]) == 45 * 70
    else:                                                                              # in no lab / inter row
        assert int(areas[1, 0, :, 2].sum()) == 45 * 70 - fg and int(areas[1, 0, :K - 1, 0].sum()) == 0


@pytest.mark.gpu
def test_class_areas_full_size():
    cls, m, grid = _inputs(2, 51, 80, 80, 7, -1.0, 1.0)
    y, cl = _labels_for(2, 51, 1024, 1024, 7)
    _, areas, _ = _check(cls, m, grid, y, cl)
    assert int(areas[:, 1, :, 0].sum()) > 0 and int(areas[:, 0, 50, 1].min()) > 0


@pytest.mark.gpu
def test_class_areas_output_smaller_than_grid():
    cls, m, grid = _inputs(2, 51, 80, 80, 8)
    y, cl = _labels_for(2, 51, 24, 20, 8)
    _check(cls, m, grid, y, cl)


@pytest.mark.gpu
def test_class_areas_rejects_bad_arguments():
    cls, m, grid = _inputs(1, 4, 4, 4, 0)
    y, cl = _labels_for(1, 4, 8, 8, 0)
    with pytest.raises(ValueError):
        ops.unwarp_class_areas(cls, m[:, :3], grid, y, cl)
    with pytest.raises(ValueError):
        ops.unwarp_class_areas(cls, m, grid, y.repeat(2, 1, 1, 1), cl)
    with pytest.raises(ValueError):
        ops.unwarp_class_areas(cls, m, grid, y, cl.repeat(2, 1))
    with pytest.raises(ValueError):
        ops.unwarp_class_areas(cls, m, grid, y, cl, dia_factor=8)
    with pytest.raises(hip.HipLibraryError):         # K = 1
        ops.unwarp_class_areas(cls[:, :1], m, grid, y, cl)
    big = torch.zeros(1, 1025, device="cuda")
    with pytest.raises(hip.HipLibraryError):         # K = 1025
        ops.unwarp_class_areas(big, m, grid, y, cl)
    counts = torch.empty(1, 6, device="cuda", dtype=torch.int64)
    acc = torch.empty(4, device="cuda")
    areas = torch.empty(1, 3, 4, 3, device="cuda", dtype=torch.int64)
    trim = torch.empty(1, 6, 3, device="cuda", dtype=torch.int64)
    scr = torch.empty(hip.query("fs_unwarp_class_areas_scratch_ints", 1, 4, 4, 4, 8, 8) + 4, device="cuda", dtype=torch.int32)
    head = (cls.data_ptr(), m.data_ptr(), grid.data_ptr(), y.data_ptr(), cl.data_ptr(), counts.data_ptr(), acc.data_ptr())
    dims = (1, 4, 4, 4, 8, 8)
    hip.call("fs_unwarp_class_areas", *head, areas.data_ptr(), trim.data_ptr(), None, scr.data_ptr(), *dims, 5, 1)
    want = ops.unwarp_class_areas(cls, m, grid, y, cl, dia_factor=5)
    assert torch.equal(areas, want[2]) and torch.equal(trim, want[3])
    for bad in ((*head, None, None, None, scr.data_ptr(), *dims, 5, 1),                 # no areas
                (*head, areas.data_ptr(), None, None, scr.data_ptr() + 4, *dims, 5, 1),         # scratch not 16-byte aligned
                (*head, areas.data_ptr(), None, None, None, *dims, 5, 1),               # no scratch
                (*head[:3], None, *head[4:], areas.data_ptr(), None, None, scr.data_ptr(), *dims, 5, 1),        # no label mask
                (*head, areas.data_ptr(), trim.data_ptr(), None, scr.data_ptr(), *dims, 8, 1),                  # D, with trim
                (*head, areas.data_ptr(), trim.data_ptr(), None, scr.data_ptr(), *dims, 5, 2),                  # frame, with trim
                (*head, areas.data_ptr(), None, None, scr.data_ptr(), 1, 1, 4, 4, 8, 8, 5, 1),                  # K = 1
                (*head, areas.data_ptr(), None, None, scr.data_ptr(), 1, 1025, 4, 4, 8, 8, 5, 1)):              # K = 1025
        with pytest.raises(hip.HipLibraryError):
            hip.call("fs_unwarp_class_areas", *bad)


# ------------------------------------------------------------------------------------------------------------------ GPU: module ---
_MODULES = {}


def _module(kind):
    if kind not in _MODULES:
        _MODULES.clear()                             # one module at a time on the device
        torch.cuda.empty_cache()
        cfg = fovealseg.lvis50_cfg()
        if kind == "segformer":
            cfg.MODEL.arch_encoder, cfg.MODEL.fc_dim = "segformer", 1024
            cfg.TRAIN.task_input_size = (160, 160)
        _MODULES[kind] = T.build_module(cfg, device="cuda")
    module, _ = _MODULES[kind]
    module.eval()
    return module


@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,seg", [("hrnet", 256, None), ("segformer", 256, (200, 180))])
def test_evaluate_with_class_areas(kind, size, seg, deterministic):
    module = _module(kind)
    K = module.cfg.DATASET.num_class
    X, Fp, Y, cl = T.synthetic_batch(2, size, size, seed=11, device="cuda")
    if seg is not None:
        _, _, Y, _ = T.synthetic_batch(2, seg[0], seg[1], seed=11, device="cuda")
    base = module.evaluate(X, Fp, Y, cl, seg)
    assert len(base) == 5                                                               # without the keyword: the parent's tuple
    out = module.evaluate(X, Fp, Y, cl, seg, class_areas=True)
    module.check_nan()
    assert len(out) == 6 and all(torch.equal(a, b) for a, b in zip(out[:5], base))
    labels = module.predict(X, Fp, seg)
    gt = R.compose_gt(Y[:, 0].long().cpu().numpy(), cl.reshape(-1).cpu().numpy(), K)
    assert out[5].shape == (2, 3, K, 3) and np.array_equal(out[5][:, 0].cpu().numpy(), R.areas_batch(labels.cpu().numpy(), gt, K))
    assert np.array_equal(out[5][:, 1, :, 2].cpu().numpy(), out[5][:, 0, :, 2].cpu().numpy())
    every = module.evaluate(X, Fp, Y, cl, seg, return_labels=True, class_areas=True, trimap=5)
    assert len(every) == 8 and torch.equal(every[5], labels) and torch.equal(every[7], out[5])   # labels, trim, areas last
    assert torch.equal(every[6], module.evaluate(X, Fp, Y, cl, seg, trimap=5)[5])


@pytest.mark.gpu
def test_evaluate_step_feeds_the_class_meter():
    module = _module("hrnet")
    K = module.cfg.DATASET.num_class
    meter, cmeter = T.FullResMeter("cuda"), T.ClassIoUMeter("cuda", K)
    rows = []
    for seed, B in ((1, 2), (2, 3)):
        batch = T.synthetic_batch(B, 128, 128, seed=seed, device="cuda")
        out = T.evaluate_step(module, batch, meter, class_meter=cmeter)
        assert len(out) == 6 and torch.equal(out[4], T.evaluate_step(module, batch)[4])
        rows.append(out[5].cpu())
    res = cmeter.result()
    total = torch.cat(rows).sum(0)
    assert res["images"] == 5 and meter.result()["images"] == 5
    iou, dice = ops.class_scores_from_areas(total)
    for s, name in enumerate(T.ClassIoUMeter.SPACES):
        assert res[name]["areas"] == total[s].tolist()
        assert np.abs(np.array(res[name]["iou"]) - iou[s].numpy()).max() <= 1e-12
        assert np.abs(np.array(res[name]["dice"]) - dice[s].numpy()).max() <= 1e-12
        assert abs(res[name]["miou"] - float(iou[s].mean())) <= 1e-12


@pytest.mark.gpu
def test_class_areas_stay_below_the_class_map():
    """evaluate(class_areas=True) must peak below predict() plus one (B,H,W) int64 map: the route it replaces."""
    module = _module("hrnet")
    B, H, W = 2, 1024, 1024
    X, Fp, Y, cl = T.synthetic_batch(B, H, W, seed=9, device="cuda")

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated()
    module.predict(X, Fp)                                                               # warm-up: weight packs, workspaces
    module.evaluate(X, Fp, Y, cl, class_areas=True)
    labels, peak_predict = peak_of(lambda: module.predict(X, Fp))
    del labels
    out, peak_areas = peak_of(lambda: module.evaluate(X, Fp, Y, cl, class_areas=True))
    module.check_nan()
    print(f"evaluate(class_areas=True) peak {peak_areas}, predict() peak {peak_predict}, one int64 map {B * H * W * 8}")
    assert out[5].shape == (B, 3, 51, 3)
    assert peak_areas < peak_predict + B * H * W * 8
