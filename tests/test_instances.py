"""The gazed instance as a record: ops.mask_bits / mask_rle / unwarp_instances / instances_to_coco (fs_mask_bits, fs_mask_rle,
fs_unwarp_instances) and DeformSegmentationModule.predict_instances.

All of it is integer work and is held bit for bit.  tests/rle_ref.py restates the definitions in numpy; the run-length format is
restated from its published definition and unpinned (no pycocotools at hand), so the CPU tests pin rle_ref to hand-derived answers and
to decode(encode(m)) == m, and the GPU tests hold the kernels to rle_ref and to `ops.unwarp_labels(...)[0] != K - 1`.  At the C ABI
every output and the scratch sit between sentinel guard bands, and counts / bits are pre-filled with garbage."""
import numpy as np
import pytest
import torch

import fovealseg
from fovealseg import hip, ops

import rle_ref as R

K3X2 = np.array([[0, 1], [1, 1], [0, 0]], dtype=bool)


def _checker(Hs, Ws, inverted):
    y, x = np.mgrid[:Hs, :Ws]
    c = ((x + y) & 1).astype(bool)
    return ~c if inverted else c


def _one(Hs, Ws, y, x):
    m = np.zeros((Hs, Ws), dtype=bool)
    m[y, x] = True
    return m


def _column_boundary(Hs=4, Ws=3):
    m = np.zeros((Hs, Ws), dtype=bool)
    m[Hs - 1, 0] = m[0, 1] = True                       # the bottom of column 0 and the top of column 1: one run of 2
    return m


# name -> (mask, counts, [area, x0, y0, bw, bh, n_runs]), every answer derived by hand
KNOWN = {
    "3x2": (K3X2, [1, 1, 1, 2, 1], [3, 0, 0, 2, 2, 5]),
    "empty": (np.zeros((5, 4), dtype=bool), [20], [0, 0, 0, 0, 0, 1]),
    "full": (np.ones((5, 4), dtype=bool), [0, 20], [20, 0, 0, 4, 5, 2]),
    "first_pixel": (_one(5, 4, 0, 0), [0, 1, 19], [1, 0, 0, 1, 1, 3]),
    "last_pixel": (_one(5, 4, 4, 3), [19, 1], [1, 3, 4, 1, 1, 2]),
    "column_boundary": (_column_boundary(), [3, 2, 7], [2, 0, 0, 2, 4, 3]),
    "inverted_checker_5x7": (_checker(5, 7, True), [0] + [1] * 35, [18, 0, 0, 7, 5, 36]),
}


# ------------------------------------------------------------------------------------------------------------------ CPU ----------
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_rle_ref_known_answers(name):
    m, counts, st = KNOWN[name]
    assert R.encode(m) == counts
    assert R.stats(m) == st
    assert np.array_equal(R.decode(counts, *m.shape), m)
    assert np.array_equal(R.unbits(R.bits(m), m.shape[1]), m)


def test_rle_ref_bits_layout():
    m = np.zeros((2, 40), dtype=bool)
    m[0, 0] = m[0, 31] = m[1, 33] = True
    assert R.bits(m).view(np.uint32).tolist() == [[0x80000001, 0], [0, 2]]


@pytest.mark.parametrize("Hs,Ws,density,seed", [(1, 1, 0.5, 0), (1, 50, 0.5, 1), (50, 1, 0.5, 2), (37, 45, 0.02, 3), (37, 45, 0.5, 4),
                                                (64, 33, 0.98, 5), (130, 70, 0.3, 6)])
def test_rle_ref_round_trip(Hs, Ws, density, seed):
    m = np.random.default_rng(seed).random((Hs, Ws)) < density
    c = R.encode(m)
    assert sum(c) == Hs * Ws and all(v > 0 for v in c[1:]) and len(c) == R.stats(m)[5]
    assert np.array_equal(R.decode(c, Hs, Ws), m)
    assert np.array_equal(R.unbits(R.bits(m), Ws), m)
    assert R.counts_row(m, len(c) + 2).tolist() == c + [0, 0] and R.counts_row(m, 1).tolist() == c[:1]


def test_instances_to_coco_on_cpu_tensors():
    masks = [K3X2, np.zeros((3, 2), dtype=bool)]
    cap = 7
    cat = torch.tensor([4, 0])
    stats = torch.tensor([R.stats(m) for m in masks])
    counts = torch.from_numpy(np.stack([R.counts_row(m, cap) for m in masks]))
    recs = ops.instances_to_coco(cat, stats, counts, (3, 2), image_ids=[17, "b"])
    assert recs[0] == {"image_id": 17, "category_id": 4, "bbox": [0, 0, 2, 2], "area": 3,
                       "segmentation": {"size": [3, 2], "counts": [1, 1, 1, 2, 1]}}
    assert recs[1] == {"image_id": "b", "category_id": 0, "bbox": [0, 0, 0, 0], "area": 0, "segmentation": {"size": [3, 2], "counts": [6]}}
    assert all(type(v) is int for r in recs for v in r["bbox"] + r["segmentation"]["counts"] + [r["area"], r["category_id"]])
    assert [r["image_id"] for r in ops.instances_to_coco(cat, stats, counts, (3, 2))] == [0, 1]
    for r, m in zip(recs, masks):
        assert np.array_equal(R.decode(r["segmentation"]["counts"], *r["segmentation"]["size"]), m)
    cut = torch.from_numpy(np.stack([R.counts_row(m, 4) for m in masks]))
    with pytest.raises(OverflowError, match=r"image 17.*max_runs >= 5"):
        ops.instances_to_coco(cat, stats, cut, (3, 2), image_ids=[17, "b"])
    with pytest.raises(ValueError):
        ops.instances_to_coco(cat, stats, counts, (3, 2), image_ids=[1])


def test_scratch_queries():
    for name, dims in (("fs_mask_rle_scratch_ints", (0, 9, 7)), ("fs_unwarp_instances_scratch_ints", (0, 4, 4, 9, 7))):
        assert hip.query(name, *dims) == 0
    for Hs, Ws in ((1, 1), (9, 7), (64, 32), (65, 33), (1024, 1024)):
        rle = hip.query("fs_mask_rle_scratch_ints", 2, Hs, Ws)
        assert rle == 2 * 3 * Ws * ((Hs + 63) // 64)                                   # three ints per (column, 64-row segment)
        lab = hip.query("fs_unwarp_labels_scratch_ints", 2, 4, 5, Hs, Ws)
        inst = hip.query("fs_unwarp_instances_scratch_ints", 2, 4, 5, Hs, Ws)
        words = 2 * Hs * ((Ws + 31) // 32)
        # everything of fs_unwarp_labels' layout is shared; the bit words and the run-length scratch come behind it, 16-byte aligned
        assert lab > 0 and lab + words + rle <= inst <= lab + words + rle + 6


def test_the_ctypes_table_binds_the_new_symbols():
    assert hip.SIGNATURES["fs_mask_bits"] == "pp" + "iii" and hip.SIGNATURES["fs_mask_rle"] == "pppp" + "iiii"
    assert hip.SIGNATURES["fs_unwarp_instances"] == "p" * 8 + "i" * 7
    assert "fs_mask_rle_scratch_ints" in hip.HOST_ONLY and "fs_unwarp_instances_scratch_ints" in hip.HOST_ONLY


def test_max_runs_argument():
    assert fovealseg.masks._max_runs(None, 1024) == 8 * 1024 + 1 and fovealseg.masks._max_runs(1, 1024) == 1 and fovealseg.masks._max_runs(77, 5) == 77
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            fovealseg.masks._max_runs(bad, 8)


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ----
GUARD = 64
SENTINEL = -0x5A5A5A5B
GARBAGE = 0x3C3C3C3D
RLE_SEG = 64                                             # csrc/mask_rle.hip: rows per (column, segment) item of the run-length passes


class Guarded:
    """n elements pre-filled with garbage between two bands of GUARD sentinels; 16-byte aligned body."""

    def __init__(self, n, dtype=torch.int32):
        self.n = n
        self.whole = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda", dtype=dtype)
        self.body = self.whole[GUARD:GUARD + n]
        self.body.fill_(GARBAGE)
        assert self.body.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.body.data_ptr()

    def intact(self):
        return bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return self.intact() and bool((self.body == GARBAGE).all())


def _bits_dev(masks):
    """(B,Hs,Ws) numpy masks -> their bit words on the device, packed on the host by rle_ref."""
    return torch.from_numpy(np.stack([R.bits(m) for m in masks])).cuda()


def _mask_rle(masks, cap):
    """fs_mask_rle at the C ABI on host-packed bit words -> (stats (B,6), counts (B,cap)) on the host; guards checked."""
    masks = np.asarray(masks)
    B, Hs, Ws = masks.shape
    bits = _bits_dev(masks)
    stats, counts = Guarded(B * 6, torch.int64), Guarded(B * cap)
    scr = Guarded(hip.query("fs_mask_rle_scratch_ints", B, Hs, Ws))
    hip.call("fs_mask_rle", bits.data_ptr(), stats.ptr, counts.ptr, scr.ptr, B, Hs, Ws, cap)
    torch.cuda.synchronize()
    assert stats.intact() and counts.intact() and scr.intact()
    return stats.body.view(B, 6).cpu(), counts.body.view(B, cap).cpu()


def _check_rle(masks, cap=None):
    masks = np.asarray(masks)
    want = [R.stats(m) for m in masks]
    if cap is None:
        cap = max(w[5] for w in want) + 3
    stats, counts = _mask_rle(masks, cap)
    assert stats.tolist() == want
    assert torch.equal(counts, torch.from_numpy(np.stack([R.counts_row(m, cap) for m in masks])))


@pytest.mark.gpu
@pytest.mark.parametrize("Hs", [1, 9])
@pytest.mark.parametrize("Ws", [1, 31, 32, 33, 100])
def test_mask_bits(Hs, Ws):
    B = 2
    g = torch.Generator().manual_seed(Hs * 1000 + Ws)
    vals = torch.tensor([0, 1, 2, 255, 0, 0], dtype=torch.uint8)[torch.randint(0, 6, (B, Hs, Ws), generator=g)]
    vals[0, 0, 0], vals[1, Hs - 1, Ws - 1] = 2, 255
    buf = torch.zeros(B * Hs * Ws + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = vals.reshape(-1).cuda()                    # the mask starts one byte off any alignment
    P = (Ws + 31) // 32
    bits = Guarded(B * Hs * P)
    hip.call("fs_mask_bits", buf.data_ptr() + 1, bits.ptr, B, Hs, Ws)
    torch.cuda.synchronize()
    assert bits.intact()
    got = bits.body.view(B, Hs, P).cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], R.bits(vals[b].numpy()))
        assert np.array_equal(R.unbits(got[b], Ws), vals[b].numpy() != 0)         # and the bits past Ws are clear
    assert torch.equal(ops.mask_bits(vals.cuda()), bits.body.view(B, Hs, P))
    assert torch.equal(ops.mask_bits(vals.cuda() != 0), bits.body.view(B, Hs, P))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_mask_rle_known_answers(name):
    m, counts, st = KNOWN[name]
    cap = len(counts) + 2
    stats, got = _mask_rle(m[None], cap)
    assert stats.tolist() == [st] and got.tolist() == [counts + [0, 0]]


@pytest.mark.gpu
@pytest.mark.parametrize("inverted", [False, True])
def test_mask_rle_checkerboards(inverted):
    m = _checker(5, 7, inverted)
    _check_rle(m[None], cap=5 * 7 + 1)


def _disc_and_ring(Hs, Ws):
    y, x = np.mgrid[:Hs, :Ws]
    r2 = (y - Hs * 0.45) ** 2 + (x - Ws * 0.55) ** 2
    r = min(Hs, Ws) * 0.4
    return np.stack([r2 <= r * r, (r2 <= r * r) & (r2 >= (0.6 * r) ** 2)])


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", [(1, 77), (77, 1), (1, 1), (300, 70), (257, 1025), (1030, 33)])
def test_mask_rle_shapes(Hs, Ws):
    """(257, 1025): more than 1 024 columns and a ragged last word; (1030, 33): columns of 17 row segments (RLE_SEG = 64 rows each), the
    last one ragged, and a second word with one column."""
    assert Hs != 1030 or Hs > RLE_SEG
    rng = np.random.default_rng(Hs * 10000 + Ws)
    masks = np.stack([rng.random((Hs, Ws)) < 0.5, rng.random((Hs, Ws)) < 0.03])
    _check_rle(masks)


@pytest.mark.gpu
def test_mask_rle_images_are_independent():
    rng = np.random.default_rng(8)
    Hs, Ws = 70, 45
    _check_rle(np.stack([np.zeros((Hs, Ws), dtype=bool), np.ones((Hs, Ws), dtype=bool), rng.random((Hs, Ws)) < 0.4]))
    _check_rle(np.stack([rng.random((Hs, Ws)) < 0.4, np.ones((Hs, Ws), dtype=bool), np.zeros((Hs, Ws), dtype=bool)]))


@pytest.mark.gpu
@pytest.mark.parametrize("density", [0.02, 0.5, 0.98])
def test_mask_rle_densities(density):
    rng = np.random.default_rng(int(density * 100))
    _check_rle(rng.random((2, 130, 97)) < density)


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", [(64, 64), (150, 201)])
def test_mask_rle_blobs(Hs, Ws):
    masks = _disc_and_ring(Hs, Ws)
    assert all(R.stats(m)[5] <= 4 * Ws + 1 for m in masks)                        # a column crosses a ring at most four times
    _check_rle(masks, cap=4 * Ws + 1)
    stats, counts = ops.mask_rle(torch.from_numpy(masks).cuda())                    # the op, at its default capacity
    assert counts.shape == (2, 8 * Ws + 1) and stats.tolist() == [R.stats(m) for m in masks]
    assert torch.equal(counts.cpu(), torch.from_numpy(np.stack([R.counts_row(m, 8 * Ws + 1) for m in masks])))
    s2, c2 = ops.mask_rle(ops.mask_bits(torch.from_numpy(masks).cuda()), Ws=Ws, max_runs=9)
    assert torch.equal(s2, stats) and torch.equal(c2, counts[:, :9])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["exact", "one_short", "one"])
def test_mask_rle_overflow(which):
    rng = np.random.default_rng(21)
    masks = np.stack([rng.random((37, 45)) < 0.3, K3X2.repeat(13, 0)[:37].repeat(23, 1)[:, :45]])
    runs = [R.stats(m)[5] for m in masks]
    cap = {"exact": runs[0], "one_short": runs[0] - 1, "one": 1}[which]
    assert 1 <= cap <= runs[0] and runs[1] < runs[0] - 1                            # image 1 fits unless cap = 1
    stats, counts = _mask_rle(masks, cap)                                           # the guards behind counts are checked there
    assert stats.tolist() == [R.stats(m) for m in masks]                            # n_runs stays the true number
    assert torch.equal(counts, torch.from_numpy(np.stack([R.counts_row(m, cap) for m in masks])))   # true prefix, zero tail


def _instances(cls, m, grid, Hs, Ws, cap, with_bits):
    """fs_unwarp_instances at the C ABI -> dict of host tensors; guards checked."""
    B, K = cls.shape
    _, h, w, _ = grid.shape
    P = (Ws + 31) // 32
    cat, stats, counts = Guarded(B, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * cap)
    bits = Guarded(B * Hs * P) if with_bits else None
    scr = Guarded(hip.query("fs_unwarp_instances_scratch_ints", B, h, w, Hs, Ws))
    hip.call("fs_unwarp_instances", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), cat.ptr, stats.ptr, counts.ptr,
             bits.ptr if with_bits else None, scr.ptr, B, K, h, w, Hs, Ws, cap)
    torch.cuda.synchronize()
    assert cat.intact() and stats.intact() and counts.intact() and scr.intact() and (bits is None or bits.intact())
    out = {"cat": cat.body.cpu(), "stats": stats.body.view(B, 6).cpu(), "counts": counts.body.view(B, cap).cpu()}
    if with_bits:
        out["bits"] = bits.body.view(B, Hs, P).cpu()
    return out


def _check_instances(cls, m, grid, Hs, Ws, tie_free=True):
    B, K = cls.shape
    labels = ops.unwarp_labels(cls, m, grid, Hs, Ws)[0].cpu()
    mask = (labels != K - 1).numpy()
    cap = max(R.stats(mk)[5] for mk in mask) + 2
    got = _instances(cls, m, grid, Hs, Ws, cap, True)
    assert np.array_equal(got["bits"].numpy(), np.stack([R.bits(mk) for mk in mask]))
    assert got["stats"].tolist() == [R.stats(mk) for mk in mask]
    assert torch.equal(got["counts"], torch.from_numpy(np.stack([R.counts_row(mk, cap) for mk in mask])))
    assert torch.equal(got["cat"], torch.argmax(cls[:, :K - 1], 1).cpu())
    if tie_free:
        for b in range(B):
            assert bool((labels[b][torch.from_numpy(mask[b])] == got["cat"][b]).all())
    without = _instances(cls, m, grid, Hs, Ws, cap, False)                           # bits = NULL: the words stay in scratch
    for k in without:
        assert torch.equal(without[k], got[k]), k
    return mask


def _tp():
    import test_predict as TP
    return TP


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 6), (50, 513, 3), (8, 1500, 2), (9, 7, 4), (8, 8, 4), (300, 200, 51)])
def test_unwarp_instances_shapes(Hs, Ws, K):
    cls, m, grid = _tp()._inputs(2, K, 9, 11, Hs * 1000 + Ws)
    mask = _check_instances(cls, m, grid, Hs, Ws)
    assert mask.any() and not mask.all()


@pytest.mark.gpu
def test_unwarp_instances_border_grids():
    g = torch.Generator().manual_seed(5)
    grid = torch.rand(2, 16, 20, 2, generator=g) * 2 - 1
    edge = torch.rand(2, 16, 20, 2, generator=g)
    grid = torch.where(edge < 0.3, torch.full_like(grid, -1.0), torch.where(edge > 0.7, torch.ones_like(grid), grid))
    cls = torch.randn(2, 7, generator=g)
    cls[:, 6] = 3 * cls.abs().amax(1)
    m = torch.rand(2, 16, 20, generator=g) - 0.5
    for Hs, Ws in ((45, 70), (45, 72)):                                              # the one-pixel and the four-pixel gather
        _check_instances(cls.cuda(), m.cuda(), grid.cuda(), Hs, Ws)


@pytest.mark.gpu
def test_unwarp_instances_no_claimed_pixel():
    cls, m, grid = _tp()._inputs(2, 9, 10, 12, 3)
    grid[1] = 1.5                                                                    # image 1: nothing claimed, every pixel = the sample at (0,0)
    for Hs, Ws in ((31, 41), (31, 40)):
        _check_instances(cls, m, grid, Hs, Ws)


@pytest.mark.gpu
def test_unwarp_instances_nan():
    cls, m, grid = _tp()._inputs(2, 6, 8, 8, 6)
    cls[0, 3] = float("nan")                                                         # NaN is the maximum: class 3 everywhere, and cat = 3
    m[1, 2:5, 1:6] = float("nan")
    mask = _check_instances(cls, m, grid, 20, 30, tie_free=False)
    assert mask[0].all()
    cls[0, 3], cls[0, 5] = 0.0, float("nan")                                        # the mask plane's factor: background everywhere
    mask = _check_instances(cls, m, grid, 20, 32, tie_free=False)
    assert not mask[0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", [(9, 7), (8, 8)])
def test_new_entry_points_stay_inside_their_scratch(Hs, Ws):
    """test_unwarp_scratch.py's pattern: the queried ints plus 64 sentinels, two calls on fresh scratch, equal outputs."""
    B, K, h, w, cap = 2, 4, 4, 4, 40
    g = torch.Generator().manual_seed(11)
    cls = torch.randn(B, K, generator=g)
    cls[:, K - 1] = 3 * cls.abs().amax(1)                # the mask plane decides where m is large
    cls = cls.cuda()
    m = (torch.rand(B, h, w, generator=g) - 0.5).cuda()
    grid = (torch.rand(B, h, w, 2, generator=g) * 2 - 1).cuda()
    bits = _bits_dev(np.random.default_rng(3).random((B, Hs, Ws)) < 0.4)

    def run_instances(scr):
        o = {"cat": torch.zeros(B, device="cuda", dtype=torch.int64), "stats": torch.zeros(B, 6, device="cuda", dtype=torch.int64),
             "counts": torch.full((B, cap), GARBAGE, device="cuda", dtype=torch.int32)}
        hip.call("fs_unwarp_instances", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), o["cat"].data_ptr(), o["stats"].data_ptr(),
                 o["counts"].data_ptr(), None, scr, B, K, h, w, Hs, Ws, cap)
        return o

    def run_rle(scr):
        o = {"stats": torch.zeros(B, 6, device="cuda", dtype=torch.int64), "counts": torch.full((B, cap), GARBAGE, device="cuda", dtype=torch.int32)}
        hip.call("fs_mask_rle", bits.data_ptr(), o["stats"].data_ptr(), o["counts"].data_ptr(), scr, B, Hs, Ws, cap)
        return o

    for name, qargs, run in (("fs_unwarp_instances", (B, h, w, Hs, Ws), run_instances), ("fs_mask_rle", (B, Hs, Ws), run_rle)):
        ints = hip.query(name + "_scratch_ints", *qargs)
        assert ints > 0
        results = []
        for _ in range(2):
            t = torch.full((ints + GUARD,), SENTINEL, device="cuda", dtype=torch.int32)
            assert t.data_ptr() % 16 == 0
            results.append(run(t.data_ptr()))
            assert bool((t[ints:] == SENTINEL).all()), f"{name}: wrote past the {ints} ints it asked for"
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), (name, k)
    cat, stats, counts = ops.unwarp_instances(cls, m, grid, Hs, Ws, max_runs=cap)
    scr = torch.empty(hip.query("fs_unwarp_instances_scratch_ints", B, h, w, Hs, Ws), device="cuda", dtype=torch.int32)
    ref = run_instances(scr.data_ptr())
    assert torch.equal(cat, ref["cat"]) and torch.equal(stats, ref["stats"]) and torch.equal(counts, ref["counts"])


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(8, 8, 4), (37, 300, 6), (9, 7, 4)])
def test_instances_scratch_off_16_bytes(Hs, Ws, K):
    """A scratch that is only 4-byte aligned takes the one-pixel gather at every width, also where Ws % 4 == 0 and an aligned one takes
    four pixels a thread (test_instance_score.py has the scored entry point's case).  The results are the aligned call's."""
    import kernel_testing as KT
    cls, m, grid = _tp()._inputs(2, K, 9, 11, Hs * 1000 + Ws)
    B, cap, P = 2, 8 * Ws + 1, (Ws + 31) // 32
    want = ops.unwarp_instances(cls, m, grid, Hs, Ws, return_bits=True)
    ints = hip.query("fs_unwarp_instances_scratch_ints", B, 9, 11, Hs, Ws)
    scr = KT.Out(ints + 4, torch.int32)
    assert scr.ptr % 16 == 0
    o = [KT.Out(B, torch.int64), KT.Out(B * 6, torch.int64), KT.Out(B * cap, torch.int32), KT.Out(B * Hs * P, torch.int32, fill=0x3C3C3C3D)]
    hip.call("fs_unwarp_instances", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), *[t.ptr for t in o], scr.ptr + 4, B, K, 9, 11, Hs, Ws, cap)
    body = scr.get(complete=False)
    assert int(body[0]) == -9999 and bool((body[ints + 1:] == -9999).all())             # the ints before and behind the shifted scratch
    assert len(want) == 4
    for t, w in zip(o, want):
        assert torch.equal(t.get().view(w.shape), w.cpu())


@pytest.mark.gpu
def test_new_entry_points_reject_bad_arguments():
    B, K, h, w, Hs, Ws, cap = 1, 4, 4, 4, 8, 8, 20
    cls, m, grid = _tp()._inputs(B, K, h, w, 0)
    cat, stats, counts, bits = Guarded(B, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * cap), Guarded(B * Hs)
    wide = Guarded(B * 513)                              # a row of 16 385 columns
    scr = Guarded(max(hip.query("fs_unwarp_instances_scratch_ints", B, h, w, Hs, Ws), hip.query("fs_unwarp_instances_scratch_ints", B, h, w, 1, 16385)))
    mask = torch.ones(B, Hs, Ws, device="cuda", dtype=torch.uint8)
    head = (cls.data_ptr(), m.data_ptr(), grid.data_ptr())
    outs = (cat.ptr, stats.ptr, counts.ptr, bits.ptr, scr.ptr)

    def rejected(name, *args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call(name, *args)

    rejected("fs_unwarp_instances", *head, *outs, B, K, h, w, Hs, Ws, 0)                                          # cap = 0
    rejected("fs_unwarp_instances", *head, *outs, B, 1, h, w, Hs, Ws, cap)                                        # K = 1
    rejected("fs_unwarp_instances", *head, cat.ptr, stats.ptr, counts.ptr, wide.ptr, scr.ptr, B, K, h, w, 1, 16385, cap)     # Ws = 16 385
    for i in (0, 1, 2):
        a = list(head)
        a[i] = None
        rejected("fs_unwarp_instances", *a, *outs, B, K, h, w, Hs, Ws, cap)
    for i in (0, 1, 2, 4):                                                                                         # bits alone may be null
        a = list(outs)
        a[i] = None
        rejected("fs_unwarp_instances", *head, *a, B, K, h, w, Hs, Ws, cap)
    rejected("fs_mask_rle", bits.ptr, stats.ptr, counts.ptr, scr.ptr, B, Hs, Ws, 0)
    rejected("fs_mask_rle", bits.ptr, stats.ptr, counts.ptr, scr.ptr, B, 0, Ws, cap)
    for i in range(4):
        a = [bits.ptr, stats.ptr, counts.ptr, scr.ptr]
        a[i] = None
        rejected("fs_mask_rle", *a, B, Hs, Ws, cap)
    rejected("fs_mask_bits", None, bits.ptr, B, Hs, Ws)
    rejected("fs_mask_bits", mask.data_ptr(), None, B, Hs, Ws)
    rejected("fs_mask_bits", mask.data_ptr(), bits.ptr, B, Hs, 0)
    torch.cuda.synchronize()
    for t in (cat, stats, counts, bits, wide, scr):                                                                # nothing was launched
        assert t.untouched()
    with pytest.raises(ValueError):
        ops.unwarp_instances(cls, m[:, :3], grid, Hs, Ws)
    with pytest.raises(ValueError):
        ops.unwarp_instances(cls, m, grid, Hs, Ws, max_runs=0)
    with pytest.raises(ValueError):
        ops.mask_rle(mask.float())
    with pytest.raises(ValueError):
        ops.mask_rle(ops.mask_bits(mask))                                                                          # bit words without Ws


# ------------------------------------------------------------------------------------------------------------------ GPU: module ---
@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [None, (200, 180)])
def test_predict_instances_equals_predict(seg, deterministic):
    TP = _tp()
    module, _ = TP._module("hrnet")
    K = module.cfg.DATASET.num_class
    X, Fp = TP._batch(2, 256, 11)
    # with the name-keyed weights one constant class wins everywhere: a large background logit lets the mask plane decide where m > 0
    bias = module.decoder.cls_net.fc.bias
    keep = bias.detach().clone()
    with torch.no_grad():
        bias[-1] += 1000.0
    try:
        state = {k: v.detach().clone() for k, v in module.state_dict().items()}
        step0 = ops.DropoutState.step
        X0, F0 = X.clone(), Fp.clone()
        cat, stats, counts, bits = module.predict_instances(X, Fp, seg, return_bits=True)
        module.check_nan()
        assert ops.DropoutState.step == step0 and torch.equal(X, X0) and torch.equal(Fp, F0)
        for k, v in module.state_dict().items():
            assert torch.equal(v, state[k]), k
        labels = module.predict(X, Fp, seg).cpu()
        with torch.no_grad():
            cls, _m, _grid, size = module._head_parts(X, Fp, seg, "test")
        three = module.predict_instances(X, Fp, seg, max_runs=5)
    finally:
        with torch.no_grad():
            bias.copy_(keep)
    H, W = seg or (256, 256)
    assert size == (H, W) and labels.shape == (2, H, W)
    mask = (labels != K - 1).numpy()
    cap = 8 * W + 1
    assert cat.dtype == torch.int64 and stats.dtype == torch.int64 and counts.dtype == torch.int32 and bits.dtype == torch.int32
    assert counts.shape == (2, cap) and bits.shape == (2, H, (W + 31) // 32)
    assert np.array_equal(bits.cpu().numpy(), np.stack([R.bits(mk) for mk in mask]))
    assert stats.tolist() == [R.stats(mk) for mk in mask]
    assert torch.equal(counts.cpu(), torch.from_numpy(np.stack([R.counts_row(mk, cap) for mk in mask])))
    assert torch.equal(cat, torch.argmax(cls[:, :K - 1], 1))
    print(f"predict_instances {H}x{W}: areas {stats[:, 0].tolist()}, runs {stats[:, 5].tolist()}, classes {cat.tolist()}")
    assert len(three) == 3 and torch.equal(three[1], stats) and torch.equal(three[2], counts[:, :5])
    if int(stats[:, 5].max()) <= cap:
        recs = ops.instances_to_coco(cat, stats, counts, (H, W), image_ids=[7, 9])
        for b, r in enumerate(recs):
            assert r["image_id"] == (7, 9)[b] and r["area"] == int(mask[b].sum()) and r["segmentation"]["size"] == [H, W]
            assert np.array_equal(R.decode(r["segmentation"]["counts"], H, W), mask[b])
    if int(stats[:, 5].max()) > 5:
        with pytest.raises(OverflowError):
            ops.instances_to_coco(*three, (H, W))


@pytest.mark.gpu
def test_predict_instances_rejects_train_mode():
    TP = _tp()
    module, _ = TP._module("hrnet")
    X, Fp = TP._batch(2, 96, 3)
    module.train()
    try:
        with pytest.raises(RuntimeError, match="predict_instances"):
            module.predict_instances(X, Fp)
    finally:
        module.eval()
    with pytest.raises(ValueError):
        module.predict_instances(X, Fp, (96, 0))
    with pytest.raises(ValueError):
        module.predict_instances(X, Fp, max_runs=0)


@pytest.mark.gpu
def test_predict_instances_allocates_no_full_resolution_map():
    """Behind the stages the call allocates its queried scratch and its outputs and nothing else -- less than a byte per pixel beside
    them -- and stays below what predict's un-warp allocates by more than half of the (B,H,W) int64 class map."""
    TP = _tp()
    module, _ = TP._module("hrnet")
    B, S = 2, 1024
    X, Fp = TP._batch(B, S, 9)
    with torch.no_grad():
        module.predict_instances(X, Fp)                                               # warm-up: weight packs, workspaces
        module.predict(X, Fp)
        parts = module._head_parts(X, Fp, None, "test")
        h, w = int(parts[2].shape[1]), int(parts[2].shape[2])
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = ops.unwarp_instances(*parts[:3], S, S, return_bits=True)
        torch.cuda.synchronize()
        inst = torch.cuda.max_memory_allocated() - base
        del out
        torch.cuda.reset_peak_memory_stats()
        out = ops.unwarp_labels(*parts[:3], S, S)
        torch.cuda.synchronize()
        lab = torch.cuda.max_memory_allocated() - base
        del out, parts
    module.check_nan()
    scratch = 4 * hip.query("fs_unwarp_instances_scratch_ints", B, h, w, S, S)
    outputs = B * (8 + 48 + 4 * (8 * S + 1) + 4 * S * (S // 32))
    map_bytes = 8 * B * S * S
    print(f"unwarp_instances adds {inst / 2 ** 20:.1f} MiB (scratch {scratch / 2 ** 20:.1f}, outputs {outputs / 2 ** 20:.2f}), "
          f"unwarp_labels {lab / 2 ** 20:.1f} MiB (class map {map_bytes / 2 ** 20:.1f})")
    assert inst <= scratch + outputs + 64 * 1024                                      # the allocator rounds each tensor up to 512 bytes
    assert scratch + outputs + 64 * 1024 < scratch + B * S * S                        # ... which is less than a byte map beside the scratch
    assert inst < lab - map_bytes // 2
