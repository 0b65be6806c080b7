"""Scoring the instance records: erosion and the pair counters on bit words (fs_mask_erode, fs_mask_pair_counts, ops.mask_erode,
ops.mask_boundary, ops.mask_pair_counts, ops.pair_scores, ops.boundary_dilation), DeformSegmentationModule.evaluate_instances,
train.InstanceAPMeter and train.evaluate_instances_step.

The definitions are unpinned (the reference has no instance metric): Boundary IoU is restated from Cheng et al., CVPR 2021, AP from
COCOeval's published algorithm.  tests/boundary_ref.py and tests/ap_ref.py restate them in plain numpy / plain loops and are held to
hand-derived answers (and the erosion to scipy) first.  Every comparison with the device is bit for bit."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from scipy import ndimage

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T
from fovealseg.models import DeformSegmentationModule

import ap_ref as AP
import boundary_ref as R


def parse(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


# ------------------------------------------------------------------------------------------- CPU: the erosion reference by hand ----
def test_reference_full_square_shrinks_from_the_image_border():
    full = np.ones((5, 5), dtype=bool)
    assert np.array_equal(R.erode(full, 1), parse([".....", ".###.", ".###.", ".###.", "....."]))      # the outside counts as unset
    assert np.array_equal(R.erode(full, 2), parse([".....", ".....", "..#..", ".....", "....."]))
    assert not R.erode(full, 3).any() and not R.erode(full, 64).any()
    assert np.array_equal(R.band(full, 3), full)                                                       # 2d+1 > side: the band is the mask


def test_reference_rectangle_touching_the_border():
    m = np.zeros((8, 12), dtype=bool)
    m[0:5, 0:7] = True                                   # rows 0 .. 4, columns 0 .. 6, in the image's corner
    want = np.zeros((8, 12), dtype=bool)
    want[1:4, 1:6] = True                                # the border erodes it like any other edge
    assert np.array_equal(R.erode(m, 1), want)
    want2 = np.zeros((8, 12), dtype=bool)
    want2[2, 2:5] = True
    assert np.array_equal(R.erode(m, 2), want2)


def test_reference_one_hole_removes_a_square():
    m = np.ones((7, 40), dtype=bool)
    m[3, 20] = False
    for d in (1, 2, 3):
        want = np.zeros((7, 40), dtype=bool)
        want[d:7 - d, d:40 - d] = True
        want[3 - d:3 + d + 1, 20 - d:20 + d + 1] = False
        got = R.erode(m, d)
        assert np.array_equal(got, want), d
        assert int(got.sum()) == max(0, (7 - 2 * d) * (40 - 2 * d) - min(7 - 2 * d, 2 * d + 1) * (2 * d + 1))


def test_reference_single_pixel_and_a_blob_across_the_word_border():
    m = np.zeros((5, 5), dtype=bool)
    m[2, 2] = True
    assert not R.erode(m, 1).any() and np.array_equal(R.band(m, 1), m)                                 # a pixel is its own boundary
    m = np.zeros((8, 40), dtype=bool)
    m[1:7, 28:36] = True                                 # columns 28 .. 35: four bits of word 0, four of word 1
    want = np.zeros((8, 40), dtype=bool)
    want[2:6, 29:35] = True
    assert np.array_equal(R.erode(m, 1), want)
    assert R.pack(want)[3].tolist() == [0xE0000000, 0x00000007]
    want2 = np.zeros((8, 40), dtype=bool)
    want2[3:5, 30:34] = True
    assert np.array_equal(R.erode(m, 2), want2) and R.pack(want2)[3].tolist() == [0xC0000000, 0x00000003]
    assert not R.erode(m, 3).any()
    assert int(R.band(m, 1).sum()) == 48 - 24


def test_reference_against_scipy():
    rng = np.random.default_rng(24)
    for Hs, Ws in ((1, 1), (3, 70), (17, 33), (40, 64), (64, 95)):
        for d in (1, 2, 5, 33):
            for density in (0.5, 0.9, 0.99, 1.0):
                m = rng.random((Hs, Ws)) < density
                want = ndimage.binary_erosion(m, np.ones((3, 3)), iterations=d, border_value=0)
                assert np.array_equal(R.erode(m, d), want), (Hs, Ws, d, density)


def test_boundary_dilation():
    assert ops.boundary_dilation(1024, 1024) == 29 and ops.boundary_dilation(480, 640) == 16
    assert ops.boundary_dilation(2048, 2048) == 58 and ops.boundary_dilation(10, 10) == 1
    assert ops.boundary_dilation(1, 1) == 1 and ops.boundary_dilation(1024, 1024, 0.01) == 14
    # a .5 tie of round: the diagonal of 3 x 4 is 5 exactly, 0.5 * 5 = 2.5 -> 2 and 0.7 * 5 = 3.5 -> 4 (half to even)
    assert ops.boundary_dilation(3, 4, 0.5) == 2 and ops.boundary_dilation(3, 4, 0.7) == 4 and ops.boundary_dilation(3, 4, 0.3) == 2
    for Hs, Ws in ((1024, 1024), (480, 640), (37, 300)):
        assert ops.boundary_dilation(Hs, Ws) == R.dilation(Hs, Ws)


def test_pair_counts_and_scores_by_hand():
    g = np.zeros((40, 40), dtype=bool)
    g[5:35, 5:35] = True                                 # 30 x 30
    same = R.pair_counts(g, g, 2)
    assert same == [900, 900, 900, 224, 224, 224] and R.scores(same) == (1.0, 1.0)      # the band: 30^2 - 26^2
    p = np.zeros((40, 40), dtype=bool)
    p[6:34, 6:34] = True                                 # 28 x 28, one pixel inside g all round
    # band(g) is rows / columns 5, 6, 33, 34 of g, band(p) rows / columns 6, 7, 32, 33 of p: they share p's outermost ring, 28^2 - 26^2
    pair = R.pair_counts(p, g, 2)
    assert pair == [784, 784, 900, 108, 784 - 576, 224]
    iou, biou = R.scores(pair)
    assert iou == 784 / 900 and biou == 108 / (208 + 224 - 108) == 1 / 3
    t = torch.tensor([same, pair, [0, 0, 0, 0, 0, 0], [0, 5, 0, 0, 5, 0]])
    i, b = ops.pair_scores(t)
    assert i.dtype == torch.float64 and i.tolist() == [1.0, 784 / 900, 0.0, 0.0] and b.tolist() == [1.0, 1 / 3, 0.0, 0.0]
    with pytest.raises(ValueError):
        ops.pair_scores(torch.zeros(3, 5, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ CPU: the AP reference by hand ----
PERFECT = [100, 100, 100, 40, 40, 40]
MISS = [10, 100, 100, 4, 40, 40]                         # IoU 10 / 190
NOGT = [0, 100, 0, 0, 40, 0]


def test_ap_reference_perfect_dataset():
    rows = [(b % 3, 0.9 - 0.1 * b, 100, b % 3, PERFECT) for b in range(6)]
    res = AP.evaluate(rows, 4)
    for k in ("AP", "AP50", "AP75", "bAP", "bAP50", "bAP75", "mIoU", "mBIoU", "cls_acc"):
        assert res[k] == 1.0, k
    assert res["n_images"] == 6 and res["n_records"] == 6


def test_ap_reference_tp_fp_tp():
    rows = [(0, 0.9, 100, 0, PERFECT), (0, 0.8, 100, 0, MISS), (0, 0.7, 100, 0, PERFECT)]
    # nGT = 3; cumTP = 1, 1, 2; precision 1, 1/2, 2/3 -> 1, 2/3, 2/3 from the right.  Recall q/100 is first reached at rank 0 for
    # q <= 33 (34 samples of 1), at rank 2 for 34 <= q <= 66 (33 samples of 2/3), never for q >= 67 (34 samples of 0)
    assert AP.ap_one([(c, s, a, l, list(p)) for c, s, a, l, p in rows], 0, 50, False) == math.fsum([1.0] * 34 + [2 / 3] * 33) / 101
    assert abs(AP.ap_one(rows, 0, 50, False) - 56 / 101) < 1e-15
    assert AP.ap_one(rows, 1, 50, False) is None
    res = AP.evaluate(rows, 2)
    assert abs(res["AP"] - 56 / 101) < 1e-15 and abs(res["bAP75"] - 56 / 101) < 1e-15
    assert res["mIoU"] == math.fsum([1, 10 / 190, 1]) / 3 and res["mBIoU"] == math.fsum([1, 4 / 76, 1]) / 3


def test_ap_reference_wrong_cat_missing_record_and_no_label():
    # image 0: label class 0, the record says 1 -> an FP of class 1 (ranked first) and a missed GT of class 0
    rows = [(1, 0.9, 100, 0, PERFECT), (1, 0.8, 100, 1, PERFECT)]
    assert AP.ap_one(rows, 0, 50, False) == 0.0          # nGT = 1, no record
    assert AP.ap_one(rows, 1, 50, False) == 0.5          # FP, TP: precision 0, 1/2 -> 1/2, 1/2 at every recall
    res = AP.evaluate(rows, 3)
    assert res["AP"] == 0.25 and res["bAP50"] == 0.25 and res["cls_acc"] == 0.5 and res["mIoU"] == 1.0
    # a missing record: nGT = 2, one TP -> precision 1 up to recall 0.50 (51 samples), 0 beyond
    rows = [(0, 0.9, 100, 0, PERFECT), (0, 0.0, 0, 0, [0, 0, 100, 0, 0, 40])]
    res = AP.evaluate(rows, 2)
    assert abs(res["AP"] - 51 / 101) < 1e-15 and res["n_records"] == 1 and res["n_images"] == 2 and res["mIoU"] == 0.5 and res["mBIoU"] == 0.5
    # an image without a label instance: its record is an FP, ranked first -> precision 1/2 everywhere
    rows = [(0, 0.5, 100, 0, PERFECT), (0, 0.9, 100, 0, NOGT)]
    res = AP.evaluate(rows, 2)
    assert res["AP"] == 0.5 and res["mIoU"] == 1.0 and res["n_records"] == 2
    assert math.isnan(AP.evaluate([(0, 0.9, 100, 0, NOGT)], 2)["AP"])


def test_ap_reference_ties_and_the_exact_threshold():
    fp, tp = (0, 0.5, 100, 0, MISS), (0, 0.5, 100, 0, PERFECT)
    # nGT = 2.  FP then TP: precision 1/2 at ranks 0 and 1, recall 0.5 reached at rank 1 -> 51 samples of 1/2
    assert AP.ap_one([fp, tp], 0, 50, False) == 25.5 / 101
    # TP then FP: precision 1 at rank 0 -> 51 samples of 1
    assert AP.ap_one([tp, fp], 0, 50, False) == 51 / 101
    half = (0, 0.5, 1, 0, [1, 1, 2, 1, 1, 2])            # IoU = 1 / 2 exactly, in both measures
    assert AP.ap_one([half], 0, 50, False) == 1.0 and AP.ap_one([half], 0, 55, False) == 0.0
    assert AP.ap_one([half], 0, 50, True) == 1.0
    assert AP.passes(1, 1, 2, 50) and not AP.passes(1, 1, 2, 55) and not AP.passes(0, 0, 0, 50)
    # the mask passes and the boundary does not: a TP of AP, an FP of bAP
    row = (0, 0.5, 100, 0, [90, 100, 100, 10, 40, 40])
    assert AP.ap_one([row], 0, 50, False) == 1.0 and AP.ap_one([row], 0, 50, True) == 0.0
    nan = (0, float("nan"), 100, 0, MISS)                # a NaN score ranks last
    assert AP.ap_one([nan, tp], 0, 50, False) == 51 / 101


# ------------------------------------------------------------------------------------------------------------- CPU: the meter ----
def _meter_batches():
    """A seeded table of 208 rows over 5 classes in batches of unequal size: (cat, conf, stats, pair, cls_label) per batch."""
    g = torch.Generator().manual_seed(24)
    out = []
    for B in (40, 17, 64, 3, 84):
        cat = torch.randint(0, 4, (B,), generator=g)
        cls = torch.where(torch.rand(B, generator=g) < 0.7, cat, torch.randint(0, 4, (B,), generator=g))
        a = torch.randint(1, 4000, (B,), generator=g)
        b = torch.randint(1, 4000, (B,), generator=g)
        n = (torch.minimum(a, b).double() * torch.rand(B, generator=g, dtype=torch.float64) ** 0.3).long()
        ba, bb = (a.double() ** 0.7).long() + 1, (b.double() ** 0.7).long() + 1
        bn = (torch.minimum(ba, bb).double() * torch.rand(B, generator=g, dtype=torch.float64) ** 0.5).long()
        a = torch.where(torch.rand(B, generator=g) < 0.08, torch.zeros_like(a), a)                      # no record
        b = torch.where(torch.rand(B, generator=g) < 0.08, torch.zeros_like(b), b)                      # no label instance
        both = ((a > 0) & (b > 0)).long()
        n, bn, ba, bb = n * both, bn * both, ba * (a > 0).long(), bb * (b > 0).long()
        pair = torch.stack([n, a, b, bn, ba, bb], 1)
        score = (torch.randint(0, 12, (B,), generator=g).float() / 12)                                   # twelve levels: many ties
        conf = torch.stack([score, score, score], 1)
        stats = torch.zeros(B, 6, dtype=torch.int64)
        stats[:, 0] = a
        out.append((cat, conf, stats, pair, cls[:, None]))
    out[2][1][5, 0] = float("nan")
    return out


def _rows_of(batches):
    rows = []
    for cat, conf, stats, pair, cls in batches:
        for b in range(cat.shape[0]):
            rows.append((int(cat[b]), float(conf[b, 0]), int(stats[b, 0]), int(cls[b, 0]), pair[b].tolist()))
    return rows


def _same(got, want):
    assert set(got) == set(want) == {"AP", "AP50", "AP75", "bAP", "bAP50", "bAP75", "mIoU", "mBIoU", "n_images", "n_records", "cls_acc"}
    for k, v in want.items():
        assert got[k] == v or (math.isnan(v) and math.isnan(got[k])), (k, got[k], v)


def test_meter_equals_the_reference():
    batches = _meter_batches()
    meter = T.InstanceAPMeter("cpu", 5)
    for b in batches:
        meter.update(*b)
    rows = _rows_of(batches)
    want = AP.evaluate(rows, 5)
    got = meter.result()
    _same(got, want)
    assert want["n_images"] == 208 and 150 < want["n_records"] < 208 and 0.0 < want["bAP"] < want["AP"] < 1.0 and want["AP75"] < want["AP50"]
    _same(T.InstanceAPMeter("cpu", 5).result(), AP.evaluate([], 5))                                      # empty: nan, 0 images
    with pytest.raises(ValueError):
        meter.update(batches[0][0], batches[0][1][:, :2], *batches[0][2:])
    with pytest.raises(ValueError):
        T.InstanceAPMeter("cpu", 1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _meter_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    meter = T.InstanceAPMeter("cpu", 5)
    batches = _meter_batches()
    for b in (batches[:3] if rank == 0 else batches[3:]):                               # 121 rows on rank 0, 87 on rank 1
        meter.update(*b)
    out[rank] = (meter.result(), meter.result(reduce=False))
    dist.barrier()
    dist.destroy_process_group()


def test_meter_two_gloo_ranks():
    want = AP.evaluate(_rows_of(_meter_batches()), 5)
    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_meter_worker, args=(world, port, out), nprocs=world, join=True)
    for rank in range(world):
        got, own = out[rank]
        _same(got, want)
        assert own["n_images"] == (121, 87)[rank] and own["AP"] != want["AP"]


# ----------------------------------------------------------------------------------------------------------- CPU: host checks ----
class _Stub:
    training = False


def test_argument_checks_on_the_host():
    mask = torch.zeros(1, 4, 4, dtype=torch.bool)
    words = torch.zeros(1, 4, 1, dtype=torch.int32)
    for d in (0, -1, True, 1.0, None, "2", 2048):
        with pytest.raises(ValueError):
            ops.mask_erode(mask, d)
        with pytest.raises(ValueError):
            ops.mask_boundary(mask, d)
        with pytest.raises(ValueError):
            ops.mask_pair_counts(mask, mask, d)
    for fn in (ops.mask_erode, ops.mask_boundary):
        for bad in ((mask.float(), 1, None), (words, 1, None), (words, 1, 33), (mask, 1, 5), (torch.zeros(0, 4, 4, dtype=torch.bool), 1, None)):
            with pytest.raises(ValueError):
                fn(*bad)
    for a, b, ws in ((mask, words, 4), (mask, torch.zeros(1, 4, 5, dtype=torch.bool), None), (mask, torch.zeros(2, 4, 4, dtype=torch.bool), None),
                     (words, torch.zeros(2, 4, 1, dtype=torch.int32), 4), (words, words, None)):
        with pytest.raises(ValueError):
            ops.mask_pair_counts(a, b, 1, Ws=ws)
    for bad in ((0, 4, 0.02), (4, 4, 0.0), (4, 4, -1.0), (4, 4, float("nan")), (4, 4, float("inf")), (4, 4, True), (4.5, 4, 0.02)):
        with pytest.raises(ValueError):
            ops.boundary_dilation(*bad)
    img, focus = torch.zeros(1, 3, 4, 4), torch.zeros(1, 2)
    y, c = torch.zeros(1, 4, 4), torch.zeros(1, 1, dtype=torch.int64)
    for kw in (dict(boundary=0.0), dict(boundary=-0.02), dict(boundary=float("nan")), dict(boundary=float("inf")), dict(boundary=1),
               dict(boundary=True), dict(seg_size=(5, 4)), dict(component=3), dict(snap_px=2.0)):
        with pytest.raises(ValueError):
            DeformSegmentationModule.evaluate_instances(_Stub(), img, focus, y, c, **kw)
    with pytest.raises(ValueError):
        DeformSegmentationModule.evaluate_instances(_Stub(), img, focus, torch.zeros(1, 2, 4, 4), c)
    with pytest.raises(ValueError):
        DeformSegmentationModule.evaluate_instances(_Stub(), img, focus, torch.zeros(2, 4, 4), c)


def test_the_ctypes_table_binds_the_morphology_symbols():
    assert hip.SIGNATURES["fs_mask_erode"] == "ppp" + "iiii" and hip.SIGNATURES["fs_mask_pair_counts"] == "pppp" + "iiii"
    assert hip.HOST_ONLY["fs_mask_erode_scratch_ints"] == ("l", "iiii") and hip.HOST_ONLY["fs_mask_pair_scratch_ints"] == ("l", "iiii")
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "fovealseg.h")).read()
    for name in ("fs_mask_erode", "fs_mask_erode_scratch_ints", "fs_mask_pair_counts", "fs_mask_pair_scratch_ints"):
        assert name + "(" in header
    assert callable(T.evaluate_instances_step) and ops.MORPH_MAX_D == 2047


def test_scratch_queries():
    for Hs, Ws in ((1, 1), (64, 64), (1024, 1024), (5, 16384)):
        P = (Ws + 31) // 32
        for d in (1, 29, 2047):
            assert [hip.query("fs_mask_erode_scratch_ints", B, Hs, Ws, d) for B in (1, 2, 3, 64)] == [B * Hs * P for B in (1, 2, 3, 64)]
            n = [hip.query("fs_mask_pair_scratch_ints", B, Hs, Ws, d) for B in (1, 2, 3, 64)]
            assert n == sorted(n) and len(set(n)) == 4 and n[0] > 4 * Hs * P and n[3] == 64 * n[0]
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 16385, 8, 1), (1, 8, 16385, 1), (1, 65536, 32768, 1), (1, 8, 8, 0), (1, 8, 8, -3),
                (1, 8, 8, 2048)):
        assert hip.query("fs_mask_erode_scratch_ints", *bad) == 0 and hip.query("fs_mask_pair_scratch_ints", *bad) == 0


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ----
FILL = 0x3C3C3C3D


def _kt():
    import kernel_testing as KT
    return KT


def _tp():
    import test_predict as TP
    return TP


def _words(masks, garbage=True):
    """(B,Hs,Ws) bool -> (B,Hs,P) uint32; with garbage, the padding bits are all set."""
    masks = np.asarray(masks)
    Ws = masks.shape[2]
    words = np.stack([R.pack(m) for m in masks])
    if garbage and Ws & 31:
        words[:, :, -1] |= np.uint32((0xFFFFFFFF << (Ws & 31)) & 0xFFFFFFFF)
    return words


def _erode(words, Ws, d, off=0):
    """fs_mask_erode at the C ABI: words (B,Hs,P) uint32 on the host -> out (B,Hs,P) uint32 on the host; every output word written,
    guard bands of output and scratch intact, the input not written.  off: ints the scratch is moved from 16-byte alignment."""
    KT = _kt()
    B, Hs, P = words.shape
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    out = KT.Out(B * Hs * P, torch.int32, fill=FILL)
    n = hip.query("fs_mask_erode_scratch_ints", B, Hs, Ws, d)
    assert n == B * Hs * P
    scr = KT.Out(n + off, torch.int32)
    hip.call("fs_mask_erode", bits.data_ptr(), out.ptr, scr.ptr + 4 * off, B, Hs, Ws, d)
    body = scr.get(complete=False)
    assert bool((body[:off] == scr.fill).all())
    assert torch.equal(bits.cpu(), torch.from_numpy(words.view(np.int32)))
    return out.get().numpy().view(np.uint32).reshape(B, Hs, P)


def _pair(wa, wb, Ws, d, off=0):
    """fs_mask_pair_counts at the C ABI -> pair (B,6) int64 on the host."""
    KT = _kt()
    B, Hs, P = wa.shape
    a = torch.from_numpy(wa.view(np.int32)).cuda()
    b = a if wb is wa else torch.from_numpy(wb.view(np.int32)).cuda()
    pair = KT.Out(B * 6, torch.int64)
    scr = KT.Out(hip.query("fs_mask_pair_scratch_ints", B, Hs, Ws, d) + off, torch.int32)
    hip.call("fs_mask_pair_counts", a.data_ptr(), b.data_ptr(), pair.ptr, scr.ptr + 4 * off, B, Hs, Ws, d)
    body = scr.get(complete=False)
    assert bool((body[:off] == scr.fill).all())
    assert torch.equal(a.cpu(), torch.from_numpy(wa.view(np.int32))) and torch.equal(b.cpu(), torch.from_numpy(wb.view(np.int32)))
    return pair.get().view(B, 6)


def _check_erode(masks, d, off=0):
    """The device against the reference, bit for bit, garbage in the padding bits; returns the reference erosions."""
    masks = np.asarray(masks)
    Ws = masks.shape[2]
    want = np.stack([R.erode(m, d) for m in masks])
    got = _erode(_words(masks), Ws, d, off)
    assert torch.equal(torch.from_numpy(got.view(np.int32)), torch.from_numpy(_words(want, garbage=False).view(np.int32))), (masks.shape, d)
    return want


def _check_pair(A, G, d, off=0, same=False):
    A, G = np.asarray(A), np.asarray(G)
    wa = _words(A)
    wb = wa if same else _words(G, garbage=False)
    want = torch.from_numpy(R.pair_batch(A, G, d))
    got = _pair(wa, wb, A.shape[2], d, off)
    assert torch.equal(got, want), (A.shape, d, got.tolist(), want.tolist())
    return want


def _rects(rng, Hs, Ws, d, n=3, holes=4):
    """A union of n filled rectangles with sides above 2d+1 where the image allows, with a few single-pixel holes."""
    m = np.zeros((Hs, Ws), dtype=bool)
    L = 2 * d + 1
    for _ in range(n):
        h = int(rng.integers(min(L + 1, Hs), Hs + 1)) if Hs > L else int(rng.integers(1, Hs + 1))
        w = int(rng.integers(min(L + 1, Ws), Ws + 1)) if Ws > L else int(rng.integers(1, Ws + 1))
        y, x = int(rng.integers(0, Hs - h + 1)), int(rng.integers(0, Ws - w + 1))
        m[y:y + h, x:x + w] = True
    ys, xs = np.nonzero(m)
    for i in rng.integers(0, len(ys), size=min(holes, len(ys))):
        m[ys[i], xs[i]] = False
    return m


SHAPES = [(1, 1), (1, 40), (40, 1), (7, 33), (33, 31), (40, 64), (40, 65), (64, 95), (130, 200)]
DS = [1, 2, 5, 31, 32, 33, 64]


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", SHAPES)
def test_mask_erode_against_the_reference(Hs, Ws):
    """B = 3, every d: rectangles with holes, a full mask and an empty one; then three more rectangle unions with the scratch one
    int off its alignment.  Where 2d+1 fits the image, some case's erosion is neither empty nor the mask -- asserted on the
    reference, so an all-zero or a pass-through output cannot pass."""
    rng = np.random.default_rng(Hs * 10007 + Ws)
    for d in DS:
        first = np.stack([_rects(rng, Hs, Ws, d), np.ones((Hs, Ws), dtype=bool), np.zeros((Hs, Ws), dtype=bool)])
        second = np.stack([_rects(rng, Hs, Ws, d, n=1, holes=1), _rects(rng, Hs, Ws, d, n=4, holes=8), _rects(rng, Hs, Ws, d, n=2, holes=0)])
        want = np.concatenate([_check_erode(first, d), _check_erode(second, d, off=1)])
        src = np.concatenate([first, second])
        if 2 * d + 1 <= min(Hs, Ws):
            assert any(w.any() and not np.array_equal(w, s) for w, s in zip(want, src)), (Hs, Ws, d)
            assert int(want[1].sum()) == (Hs - 2 * d) * (Ws - 2 * d)
        else:
            assert not want.any()


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,d", [(1024, 1024, 29), (2200, 40, 5), (2200, 40, 19), (5, 16384, 2), (640, 700, 300), (300, 520, 100)])
def test_mask_erode_every_tiling(Hs, Ws, d):
    """The passes' tilings: 1024 x 1024 at d = 29 (32 word columns by 70 rows a workgroup of the columns pass, 15 tiles down the image),
    a tall image of two word columns in two tiles, a row of 512 words (two rows a workgroup of the rows pass), and dilations whose halo
    leaves room for 2 and for 8 word columns only."""
    yy, xx = np.mgrid[:Hs, :Ws]
    rng = np.random.default_rng(Hs + Ws + d)
    disc = (yy - Hs // 2) ** 2 * Ws * Ws + (xx - Ws // 2) ** 2 * Hs * Hs <= (Hs * Ws) ** 2 // 5      # an ellipse filling most of the image
    full = np.ones((Hs, Ws), dtype=bool)
    full[1, 1] = False                                   # the hole's square takes a corner, 2 x 2 where it has the room, off the eroded interior
    masks = np.stack([disc, full, _rects(rng, Hs, Ws, d, n=3, holes=6)])
    want = _check_erode(masks, d)
    assert int(want[0].sum()) < int(disc.sum()) and want[1].any()
    assert int(want[1].sum()) == (Hs - 2 * d) * (Ws - 2 * d) - min(2, Hs - 2 * d) * min(2, Ws - 2 * d)
    # the pair counters of (disc, full) and (full, rects), the reference's from the erosions it has just made
    a, g = masks[:2], masks[1:]
    ba, bg = a & ~want[:2], g & ~want[1:]
    ref = torch.from_numpy(np.array([[(x & y).sum(), x.sum(), y.sum(), (bx & by).sum(), bx.sum(), by.sum()]
                                     for x, y, bx, by in zip(a, g, ba, bg)], dtype=np.int64))
    got = _pair(_words(a), _words(g, garbage=False), Ws, d)
    assert torch.equal(got, ref), (got.tolist(), ref.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", SHAPES)
def test_mask_pair_counts_against_the_reference(Hs, Ws):
    rng = np.random.default_rng(Hs * 7 + Ws * 10007)
    empty, full = np.zeros((Hs, Ws), dtype=bool), np.ones((Hs, Ws), dtype=bool)
    for d in DS:
        a = np.stack([_rects(rng, Hs, Ws, d), full, _rects(rng, Hs, Ws, d, n=2), empty])
        g = np.stack([_rects(rng, Hs, Ws, d), _rects(rng, Hs, Ws, d, n=1), empty, empty])
        want = _check_pair(a, g, d, off=d & 1)
        assert want[3].tolist() == [0] * 6 and want[2, 0] == 0 and want[2, 2] == 0
        same = _check_pair(a, a, d, same=True)                                          # a == b: one pointer
        assert torch.equal(same[:, 0], same[:, 1]) and torch.equal(same[:, 3], same[:, 5])
        if 2 * d + 1 > min(Hs, Ws):                                                     # the bands are the masks
            assert torch.equal(want[:, 3:], want[:, :3])
    left, right = empty.copy(), empty.copy()
    left[:, :Ws // 2], right[:, Ws // 2:] = True, True
    want = _check_pair(np.stack([left]), np.stack([right]), 1)                          # disjoint
    assert want[0, 0] == 0 and want[0, 3] == 0 and want[0, 1] + want[0, 2] == Hs * Ws
    # the ops: a bool mask, bit words, one image without a batch axis
    a, g = torch.from_numpy(np.stack([left, full])).cuda(), torch.from_numpy(np.stack([full, right])).cuda()
    want = torch.from_numpy(R.pair_batch(a.cpu().numpy(), g.cpu().numpy(), 2))
    assert torch.equal(ops.mask_pair_counts(a, g, 2).cpu(), want)
    assert torch.equal(ops.mask_pair_counts(ops.mask_bits(a), ops.mask_bits(g), 2, Ws=Ws).cpu(), want)
    assert torch.equal(ops.mask_pair_counts(a[0].to(torch.uint8), g[0].to(torch.uint8), 2).cpu(), want[:1])
    er = ops.mask_erode(g, 2)
    assert er.dtype == torch.int32 and np.array_equal(er.cpu().numpy().view(np.uint32), _words([R.erode(m, 2) for m in g.cpu().numpy()], False))
    bd = ops.mask_boundary(ops.mask_bits(g), 2, Ws=Ws)
    assert np.array_equal(bd.cpu().numpy().view(np.uint32), _words([R.band(m, 2) for m in g.cpu().numpy()], False))


@pytest.mark.gpu
def test_morphology_rejects_bad_arguments():
    KT = _kt()
    B, Hs, Ws = 1, 8, 40
    bits, other = KT.Out(B * Hs * 2, torch.int32), KT.Out(B * Hs * 2, torch.int32)
    out, pair, scr = KT.Out(B * Hs * 2, torch.int32), KT.Out(B * 6, torch.int64), KT.Out(4096, torch.int32)

    def rejected(name, *args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call(name, *args)

    good = [bits.ptr, out.ptr, scr.ptr]
    for i in range(3):
        a = list(good)
        a[i] = None
        rejected("fs_mask_erode", *a, B, Hs, Ws, 1)
    rejected("fs_mask_erode", bits.ptr, bits.ptr, scr.ptr, B, Hs, Ws, 1)               # out == bits
    goodp = [bits.ptr, other.ptr, pair.ptr, scr.ptr]
    for i in range(4):
        a = list(goodp)
        a[i] = None
        rejected("fs_mask_pair_counts", *a, B, Hs, Ws, 1)
    for dims in ((0, Hs, Ws, 1), (B, 0, Ws, 1), (B, Hs, 0, 1), (-1, Hs, Ws, 1), (B, 16385, 1, 1), (B, 1, 16385, 1), (B, 2 ** 16, 2 ** 15, 1),
                 (B, Hs, Ws, 0), (B, Hs, Ws, -1), (B, Hs, Ws, 2048)):
        rejected("fs_mask_erode", *good, *dims)
        rejected("fs_mask_pair_counts", *goodp, *dims)
    for t in (bits, other, out, pair, scr):
        assert t.untouched()
    hip.call("fs_mask_erode", *good, B, Hs, Ws, 2047)                                   # the cap itself is legal: the empty erosion
    assert not out.untouched() and bool((out.get() == 0).all())
    hip.call("fs_mask_pair_counts", *goodp, B, Hs, Ws, 1024)
    assert not pair.untouched()


# ------------------------------------------------------------------------------------------------- GPU: the composed call ---------
def _i32(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


def _labelled(B, size, seed):
    return T.synthetic_batch(B, size, size, seed=seed, device="cuda")


class _foreground_head:
    """test_component.py's trick: a large background logit lets the mask plane decide, so the head marks a non-trivial foreground."""

    def __init__(self, module):
        self.bias = module.decoder.cls_net.fc.bias
        self.keep = self.bias.detach().clone()

    def __enter__(self):
        with torch.no_grad():
            self.bias[-1] += 1000.0

    def __exit__(self, *exc):
        with torch.no_grad():
            self.bias.copy_(self.keep)


@pytest.mark.gpu
@pytest.mark.parametrize("component", [None, 8])
def test_evaluate_instances_is_predict_instances_and_the_pair_counts(component, deterministic):
    TP = _tp()
    module, _ = TP._module("hrnet")
    X, Fp, Y, cls = _labelled(2, 256, 11)
    H = W = 256
    d = ops.boundary_dilation(H, W)
    assert d == 7
    with _foreground_head(module):
        # the label: the head's own foreground moved by (2, 3) pixels, joined with the synthetic disc -- the counters of the
        # intersections are then no zeros
        seen = module.predict_instances(X, Fp, return_bits=True)[3].cpu().numpy().view(np.uint32)
        moved = np.roll(np.stack([R.unpack(w, W) for w in seen]), (2, 3), (1, 2))
        Y = ((Y != 0) | torch.from_numpy(moved).cuda()[:, None]).float()
        state = {k: v.detach().clone() for k, v in module.state_dict().items()}
        args0 = [t.clone() for t in (X, Fp, Y, cls)]
        want = module.predict_instances(X, Fp, return_bits=True, return_score=True, component=component)
        got = module.evaluate_instances(X, Fp, Y, cls, component=component)
        wide = module.evaluate_instances(X, Fp, Y[:, 0], cls[:, 0], seg_size=(H, W), component=component, boundary=0.05)
        module.check_nan()
        for a, b in zip((X, Fp, Y, cls), args0):
            assert torch.equal(a, b)
        for k, v in module.state_dict().items():
            assert torch.equal(v, state[k]), k
    assert len(got) == (6 if component else 5) and len(want) == len(got)
    bits = want[3]
    for a, b in zip(got[:-1], want[:3] + want[4:]):
        assert torch.equal(_i32(a), _i32(b))
    for a, b in zip(wide[:-1], got[:-1]):
        assert torch.equal(_i32(a), _i32(b))
    pair = got[-1]
    assert pair.dtype == torch.int64 and pair.shape == (2, 6)
    label = Y[:, 0].long() != 0
    assert torch.equal(pair, ops.mask_pair_counts(bits, ops.mask_bits(label), d, Ws=W))
    masks = np.stack([R.unpack(w, W) for w in bits.cpu().numpy().view(np.uint32)])
    assert torch.equal(pair.cpu(), torch.from_numpy(R.pair_batch(masks, label.cpu().numpy(), d)))
    assert torch.equal(wide[-1].cpu(), torch.from_numpy(R.pair_batch(masks, label.cpu().numpy(), ops.boundary_dilation(H, W, 0.05))))
    assert torch.equal(pair[:, 1], got[1][:, 0]) and int(pair[:, 1].min()) > 0 and int(pair[:, 2].min()) > 0
    assert int(pair[:, 0].min()) > 0 and int(pair[:, 3].min()) > 0
    print(f"evaluate_instances(component={component}) 256x256 d {d}: pair {pair.tolist()}, scores {[t.tolist() for t in ops.pair_scores(pair)]}")
    module.train()
    try:
        with pytest.raises(RuntimeError, match="predict_instances"):
            module.evaluate_instances(X, Fp, Y, cls)
    finally:
        module.eval()


@pytest.mark.gpu
def test_evaluate_instances_allocates_nothing_wide():
    """The peak of the call stays within predict_instances' peak plus mask_bits' of the label: no (B,H,W) tensor wider than a byte is
    added (one fp32 plane would be B * H * W * 4 bytes on top of the label's bool planes)."""
    TP = _tp()
    module, _ = TP._module("hrnet")
    X, Fp, Y, cls = _labelled(2, 256, 11)
    label = Y[:, 0] != 0

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del out
        return top

    for fn in (lambda: module.predict_instances(X, Fp, return_bits=True, return_score=True), lambda: module.evaluate_instances(X, Fp, Y, cls)):
        fn()                                             # warm: caches and workspaces exist
    p_pred = peak(lambda: module.predict_instances(X, Fp, return_bits=True, return_score=True))
    p_bits = peak(lambda: ops.mask_bits(label))
    p_eval = peak(lambda: module.evaluate_instances(X, Fp, Y, cls))
    print(f"peak bytes: predict_instances {p_pred}, mask_bits {p_bits}, evaluate_instances {p_eval}")
    assert p_eval <= p_pred + p_bits
    # the tail of the call alone: the label's bool planes, its words, the pair scratch -- under one byte a pixel and plane
    bits = module.predict_instances(X, Fp, return_bits=True)[3]
    p_tail = peak(lambda: ops.mask_pair_counts(bits, ops.mask_bits((Y[:, 0] >= 1) | (Y[:, 0] <= -1)), 7, Ws=256))
    assert p_tail < 2 * 256 * 256 * 4, p_tail


@pytest.mark.gpu
def test_meter_end_to_end(deterministic):
    TP = _tp()
    module, _ = TP._module("hrnet")
    K = module.cfg.DATASET.num_class
    meter = T.InstanceAPMeter("cuda", K)
    rows = []
    with _foreground_head(module):
        for seed in (3, 5, 8):
            X, Fp, _, _ = _labelled(2, 128, seed)
            cat, _, _, bits, _ = module.predict_instances(X, Fp, return_bits=True, component=8)
            blob = np.stack([R.unpack(w, 128) for w in bits.cpu().numpy().view(np.uint32)])
            Y = torch.from_numpy(np.roll(blob, seed % 3, 2)).cuda()[:, None].float()    # the label: the record's blob moved by 0 .. 2 pixels
            cls = cat.clone()[:, None]                                                  # image 0: the head's class is the label's
            cls[1] = (cls[1] + 1) % (K - 1)                                             # image 1: another one
            batch = (X, Fp, Y, cls)
            out = T.evaluate_instances_step(module, batch, meter, component=8)
            assert len(out) == 6
            for b in range(2):
                rows.append((int(out[0][b]), float(out[3][b, 0]), int(out[1][b, 0]), int(batch[3][b, 0]), out[5][b].tolist()))
    assert all(r.is_cuda for r in meter.rows) and len(meter.rows) == 3
    got = meter.result()
    _same(got, AP.evaluate(rows, K))
    assert got["n_images"] == 6 and got["cls_acc"] == 0.5 and got["mIoU"] > 0.2 and got["AP"] > 0.0
    print(f"meter: {got}")
