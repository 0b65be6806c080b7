"""Of an image's annotated instances, the one under the gaze: fs_mask_candidates, fs_mask_candidates_scratch_ints, ops.mask_candidates,
ops.coco_candidates, module.evaluate_instances(candidates=...) and train.score_coco_records(gaze=...).

The definition is UNPINNED: the reference chooses an annotation and puts the gaze inside it (b2_preprocess_lvis.py:258-333) and has
nothing that goes the other way, so tests/candidates_ref.py restates the library's rule -- of the instances that contain the gaze
pixel the smallest, else the nearest within the snap distance; the best-overlapping one by exact IoU -- as a double loop over dense
masks, and is held here to hand-derived answers before anything on the device is held to it.  Every comparison is == / torch.equal."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fovealseg import hip, ops
from fovealseg import train as T

import candidates_ref as CR
import component_ref as CP
import poly_ref as PR
import rle_ref as R


def parse(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


def rect(H, W, y0, y1, x0, x1):
    """rows y0 .. y1 and columns x0 .. x1, both ends included"""
    m = np.zeros((H, W), dtype=bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def dots(H, W, *yx):
    m = np.zeros((H, W), dtype=bool)
    for y, x in yx:
        m[y, x] = True
    return m


def foc(py, px, H, W):
    """the normalised focus whose gaze pixel is (py, px): rint(py / (H - 1) * (H - 1) * 16) = 16 py, (16 py + 8) >> 4 = py"""
    return [py / (H - 1) if H > 1 else 0.0, px / (W - 1) if W > 1 else 0.0]


NONE = [-1, -1, -1, 0, 0, 0, -1, 0]                      # an image that selects nothing, contains nothing, overlaps nothing


# ------------------------------------------------------------------------------------------------ the hand-derived answers --------
def test_reference_nested_instances_the_smaller_one_wins():
    H, W = 6, 10
    outer, inner = rect(H, W, 0, 5, 0, 7), rect(H, W, 1, 3, 2, 4)                # 48 and 9 pixels, both hold (2, 3)
    for order, want in (([outer, inner], 1), ([inner, outer], 0)):
        g, sel, cand = CR.candidates(np.stack(order), [0, 2], [foc(2, 3, H, W)], cand_cat=[7, 8])
        assert sel.tolist() == [[want, 7 + want, 0, 9, 0, 2, -1, 0]]
        assert np.array_equal(g[0], inner)
        assert cand.tolist() == [[0, int(m.sum()), 0, 0, 2, 3] for m in order]


def test_reference_equal_areas_the_smaller_row_wins():
    H, W = 6, 10
    a, b = rect(H, W, 0, 2, 0, 2), rect(H, W, 2, 4, 2, 4)                        # 9 pixels each, (2, 2) in both
    g, sel, _ = CR.candidates(np.stack([a, b]), [0, 2], [foc(2, 2, H, W)])
    assert sel.tolist() == [[0, -1, 0, 9, 0, 2, -1, 0]] and np.array_equal(g[0], a)
    g, sel, _ = CR.candidates(np.stack([b, a]), [0, 2], [foc(2, 2, H, W)])
    assert sel.tolist() == [[0, -1, 0, 9, 0, 2, -1, 0]] and np.array_equal(g[0], b)


def test_reference_equal_distance_the_smaller_area_wins_and_the_snap_distance():
    H, W = 5, 12
    a, b = dots(H, W, (2, 0), (2, 1), (2, 2)), dots(H, W, (2, 8))                # gaze (2, 5): (2, 2) and (2, 8) are both 3 away
    masks, f = np.stack([a, b]), [foc(2, 5, H, W)]
    g, sel, cand = CR.candidates(masks, [0, 2], f, cand_cat=[4, 5])
    assert cand.tolist() == [[0, 3, 0, 9, 2, 2], [0, 1, 0, 9, 2, 8]]
    assert sel.tolist() == [[1, 5, 9, 1, 0, 0, -1, 0]] and np.array_equal(g[0], b)
    assert CR.snap2_of(3) == 9 and CR.snap2_of(2.999) == 8 and CR.snap2_of(None) == CR.OFF2 and CR.snap2_of(0) == 0
    g, sel, cand9 = CR.candidates(masks, [0, 2], f, cand_cat=[4, 5], snap2=9)    # exactly at the nearest pixel
    assert sel.tolist() == [[1, 5, 9, 1, 0, 0, -1, 0]] and np.array_equal(cand9, cand)
    g, sel, cand8 = CR.candidates(masks, [0, 2], f, cand_cat=[4, 5], snap2=8)    # one below: nothing, and the cand rows do not change
    assert sel.tolist() == [NONE] and not g.any() and np.array_equal(cand8, cand)


def test_reference_empty_candidates_and_images_without_candidates():
    H, W = 3, 4
    masks = np.stack([np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool), np.zeros((H, W), dtype=bool)])
    g, sel, cand = CR.candidates(masks, [0, 0, 2, 2, 3], [foc(1, 1, H, W)] * 4, cand_cat=[1, 2, 3])
    assert cand.tolist() == [[1, 0, 0, -1, -1, -1], [1, 12, 0, 0, 1, 1], [3, 0, 0, -1, -1, -1]]
    assert sel.tolist() == [NONE, [1, 2, 0, 12, 0, 1, -1, 0], NONE, NONE]
    assert g[1].all() and not g[0].any() and not g[2].any() and not g[3].any()
    assert [CR.outcome(sel[b], lo, hi, cand) for b, (lo, hi) in enumerate([(0, 0), (0, 2), (2, 2), (2, 3)])] == ["none", "one", "none", "empty"]
    g, sel, cand = CR.candidates(masks[:0], [0, 0], [foc(1, 1, H, W)])           # N = 0
    assert sel.tolist() == [NONE] and cand.shape == (0, 6) and not g.any()


def test_reference_across_the_word_border_and_ties_inside_a_candidate():
    H, W = 2, 40
    a, b, c = dots(H, W, (0, 32)), dots(H, W, (0, 29)), dots(H, W, (0, 30), (0, 32))
    g, sel, cand = CR.candidates(np.stack([b, c, a]), [0, 3], [foc(0, 31, H, W)])
    # (0, 30) and (0, 32) are both 1 away: the smaller row-major index is the nearest pixel; a and c tie at d2 = 1, a is smaller
    assert cand.tolist() == [[0, 1, 0, 4, 0, 29], [0, 2, 0, 1, 0, 30], [0, 1, 0, 1, 0, 32]]
    assert sel.tolist() == [[2, -1, 1, 1, 0, 0, -1, 0]] and np.array_equal(g[0], a)
    # garbage in the padding bits is no pixel: the words of a 40-wide row carry 24 of them
    words = R.bits(a).copy()
    words[:, -1] |= np.int32(-1) << 8
    assert np.array_equal(_unwords(words, W), a) and not np.array_equal(words, R.bits(a))


def test_reference_nan_and_out_of_range_focus():
    H, W = 4, 6
    masks = np.stack([dots(H, W, (0, 0)), dots(H, W, (3, 5))])
    assert CR.gaze_pixel([float("nan"), float("nan")], H, W) == (0, 0)
    assert CR.gaze_pixel([2.0, 7.5], H, W) == (3, 5) and CR.gaze_pixel([-1.0, 2.0], H, W) == (0, 5)
    assert CR.gaze_pixel([float("inf"), float("-inf")], H, W) == (3, 0)
    focus = [[float("nan"), float("nan")], [2.0, 7.5], [-1.0, 2.0]]
    g, sel, cand = CR.candidates(np.concatenate([masks] * 3), [0, 2, 4, 6], focus)
    # image 2 looks at (0, 5): (0, 0) is 25 away, (3, 5) is 9 away
    assert sel.tolist() == [[0, -1, 0, 1, 0, 1, -1, 0], [3, -1, 0, 1, 0, 1, -1, 0], [5, -1, 9, 1, 0, 0, -1, 0]]
    assert cand[4].tolist() == [2, 1, 0, 25, 0, 0] and cand[5].tolist() == [2, 1, 0, 9, 3, 5]


def test_reference_best_overlap_and_its_ties():
    H, W = 4, 8
    pred = rect(H, W, 0, 1, 0, 3)                                                # 8 pixels
    a, b = rect(H, W, 0, 1, 0, 1), rect(H, W, 0, 1, 2, 3)                        # 4 / (4 + 8 - 4) = 1 / 2 each
    c = rect(H, W, 0, 3, 0, 3)                                                   # 8 / (16 + 8 - 8) = 1 / 2 with four times the area
    e = rect(H, W, 1, 3, 3, 7)                                                   # 1 / (15 + 8 - 1)
    g, sel, cand = CR.candidates(np.stack([c, e, b, a]), [0, 4], [foc(3, 7, H, W)], pred=[pred])
    assert cand[:, 1:3].tolist() == [[16, 8], [15, 1], [4, 4], [4, 4]]
    assert sel.tolist() == [[1, -1, 0, 15, 1, 1, 2, 0]]                          # the gaze is on e; b before a by the row, both before c by area
    g, sel, _ = CR.candidates(np.stack([c, e]), [0, 2], [foc(3, 7, H, W)], pred=[pred])
    assert sel[0, 6] == 0
    g, sel, _ = CR.candidates(np.stack([a, e]), [0, 2], [foc(3, 7, H, W)], pred=[np.zeros_like(pred)])
    assert sel[0, 6] == -1 and sel[0, 4] == 0                                    # nothing overlaps an empty prediction


def test_reference_compares_overlaps_exactly_where_float_division_ties():
    i1, u1, i2, u2 = 100000001, 200000003, 100000000, 200000001                 # sides <= 16384: below 2^28, the products below 2^57
    assert i1 / u1 == i2 / u2 and i1 * u2 != i2 * u1 and max(i1, u1, i2, u2) < 2 ** 28 and i1 * u2 < 2 ** 57
    assert i1 * u2 == 20000000300000001 and i2 * u1 == 20000000300000000        # the first is greater, by one part in 2 * 10^16
    assert CR.overlap_before((i1, u1, 5, 9), (i2, u2, 1, 0)) and not CR.overlap_before((i2, u2, 1, 0), (i1, u1, 5, 9))
    assert CR.overlap_before((1, 2, 3, 1), (2, 4, 3, 2)) and CR.overlap_before((2, 4, 2, 5), (1, 2, 3, 1))      # equal: area, then row


def test_reference_malformed_offsets():
    H, W = 3, 4
    masks = np.stack([rect(H, W, 0, 1, 0, 1), np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool)])
    for off in ([1, 2, 3], [0, 2, 1, 3], [0, 1, 2], [0, 1, 4]):
        assert not CR.offsets_valid(off, 3)
        g, sel, cand = CR.candidates(masks, off, [foc(0, 0, H, W)] * (len(off) - 1), cand_cat=[1, 2, 3])
        assert cand.tolist() == [[-1, 4, 0, -1, -1, -1], [-1, 0, 0, -1, -1, -1], [-1, 12, 0, -1, -1, -1]]
        assert sel.tolist() == [[-1, -1, -1, 0, 0, 0, -1, 1]] * (len(off) - 1) and not g.any()
    assert CR.offsets_valid([0, 0, 3, 3], 3) and CR.offsets_valid([0], 0)


# ------------------------------------------------------------------------------------------------------- CPU: the host side --------
def _bands(Hs, Ws):
    P = (Ws + 31) // 32
    return math.ceil(Hs / min(Hs, 256, max(1, 8192 // P)))


def test_the_ctypes_table_binds_the_selection():
    assert hip.SIGNATURES["fs_mask_candidates"] == "p" * 9 + "iiii" + "l"       # nine pointers, B, N, Hs, Ws, snap2
    assert hip.HOST_ONLY["fs_mask_candidates_scratch_ints"] == ("l", "iiii")
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "fovealseg.h")).read()
    assert "long fs_mask_candidates_scratch_ints(int B, int N, int Hs, int Ws);" in header
    assert "int fs_mask_candidates(const unsigned int* cbits, const int* cand_off, const long long* cand_cat, const float* focus," in header
    doc = header.split("fs_mask_candidates_scratch_ints(int B")[0].split("fs_mask_pair_counts(")[-1]
    assert "UNPINNED" in doc and "b2_preprocess_lvis.py:258-333" in doc and "the inverse of" in doc
    # a header of four ints, then five a (candidate, band of min(Hs, 256, 8192 / P) rows)
    for B, N, Hs, Ws in ((1, 0, 1, 1), (1, 1, 1, 1), (3, 20, 130, 200), (3, 40, 1300, 1024), (64, 512, 640, 640), (2, 7, 100, 16384)):
        assert hip.query("fs_mask_candidates_scratch_ints", B, N, Hs, Ws) == 4 + N * _bands(Hs, Ws) * 5
    assert (_bands(130, 200), _bands(600, 40), _bands(1300, 1024), _bands(257, 33), _bands(100, 16384)) == (1, 3, 6, 2, 7)
    for B, N, Hs, Ws in ((0, 1, 5, 5), (-1, 1, 5, 5), (1, -1, 5, 5), (1, 1, 0, 5), (1, 1, 5, 0), (1, 1, 16385, 4), (1, 1, 4, 16385)):
        assert hip.query("fs_mask_candidates_scratch_ints", B, N, Hs, Ws) == 0


def test_mask_candidates_refuses_on_the_host():
    cb, off, f = torch.zeros(3, 5, 2, dtype=torch.int32), torch.tensor([0, 1, 3], dtype=torch.int32), torch.zeros(2, 2)
    for args, kw in (((cb.long(), off, f, 40), {}), ((cb, off, f, 70), {}), ((cb, off, f, None), {}), ((cb[0], off, f, 40), {}),
                     ((cb, off.long(), f, 40), {}), ((cb, off[:1], f, 40), {}), ((cb, off, f[:1], 40), {}), ((cb, off, f, True), {}),
                     ((cb, off, f, 40), {"pred": cb}), ((cb, off, f, 40), {"pred": cb[:2].long()}), ((cb, off, f, 40), {"cand_cat": torch.zeros(2, dtype=torch.int64)}),
                     ((cb, off, f, 40), {"cand_cat": torch.zeros(3, dtype=torch.int32)}), ((cb, off, f, 40), {"snap_px": -1.0}),
                     ((cb, off, f, 40), {"snap_px": float("nan")}), ((cb, off, f, 40), {"snap_px": float("inf")})):
        with pytest.raises(ValueError):
            ops.mask_candidates(*args, **kw)


def _rec(image_id, seg, cat=1, score=None, ann=None):
    r = {"image_id": image_id, "category_id": cat, "segmentation": seg}
    if score is not None:
        r["score"] = score
    if ann is not None:
        r["id"] = ann
    return r


def test_coco_candidates_refuses_on_the_host():
    rle = {"size": [3, 4], "counts": [12]}
    with pytest.raises(ValueError, match="not among image_ids"):
        ops.coco_candidates([_rec(1, rle), _rec(9, rle)], (3, 4), "cpu", [1, 2])
    with pytest.raises(ValueError, match="twice"):
        ops.coco_candidates([_rec(1, rle)], (3, 4), "cpu", [1, 2, 1])
    with pytest.raises(ValueError, match="image_id"):
        ops.coco_candidates([{"category_id": 1, "segmentation": rle}], (3, 4), "cpu", [1])
    with pytest.raises(ValueError, match="no image_ids"):
        ops.coco_candidates([], (3, 4), "cpu", [])
    with pytest.raises(ValueError, match="size"):
        ops.coco_candidates([], (3,), "cpu", [1])
    # no record at all: empty tables, nothing launched
    cbits, off, cat, info, rows = ops.coco_candidates([], (3, 40), "cpu", ["a", "b"])
    assert tuple(cbits.shape) == (0, 3, 2) and off.tolist() == [0, 0, 0] and cat.numel() == 0 and tuple(info.shape) == (0, 2) and rows == []


def test_score_coco_records_gaze_refusals():
    rle = {"size": [3, 4], "counts": [12]}
    poly = [[0.0, 0.0, 3.0, 0.0, 3.0, 2.0]]
    meter = T.InstanceAPMeter("cpu", 4)
    gt = [_rec(1, rle), _rec(1, poly), _rec(2, rle)]
    dt = [_rec(1, rle, score=0.5)]
    images = {1: (3, 4), 2: (3, 4)}
    gaze = {1: (0.5, 0.5), 2: (0.0, 1.0)}
    with pytest.raises(ValueError, match="more than one record; one instance an image is scored"):
        T.score_coco_records(dt, gt, meter, images=images)                      # as on the parent
    with pytest.raises(ValueError, match="more than one record; one instance an image is scored"):
        T.score_coco_records(dt, [_rec(1, rle), _rec(1, rle)], meter)
    with pytest.raises(ValueError, match="gaze needs `images`"):
        T.score_coco_records(dt, gt, meter, gaze=gaze)
    with pytest.raises(ValueError, match="gaze must be a dict"):
        T.score_coco_records(dt, gt, meter, images=images, gaze=[(0.5, 0.5)])
    with pytest.raises(ValueError, match="image 2 has no gaze"):
        T.score_coco_records(dt, gt, meter, images=images, gaze={1: (0.5, 0.5)})
    for bad in ((0.5,), "ab", 0.5, (0.5, None)):
        with pytest.raises(ValueError, match="two numbers"):
            T.score_coco_records(dt, gt, meter, images=images, gaze={1: bad, 2: (0.0, 0.0)})
    with pytest.raises(ValueError, match="differ in size"):
        T.score_coco_records(dt, gt + [_rec(2, {"size": [4, 3], "counts": [12]})], meter, images=images, gaze=gaze)
    with pytest.raises(ValueError, match="missing from `images`"):
        T.score_coco_records(dt, gt + [_rec(3, poly)], meter, images=images, gaze={**gaze, 3: (0.0, 0.0)})
    with pytest.raises(ValueError, match="results: image 1 has more than one record"):
        T.score_coco_records(dt + dt, gt, meter, images=images, gaze=gaze)      # dt is still at most one an image
    with pytest.raises(ValueError, match="has no ground truth"):
        T.score_coco_records([_rec(5, rle, score=0.5)], gt, meter, images=images, gaze=gaze)
    with pytest.raises(ValueError, match="has no score"):
        T.score_coco_records([_rec(1, rle)], gt, meter, images=images, gaze=gaze)
    with pytest.raises(ValueError, match="differs from the ground truth's"):
        T.score_coco_records([_rec(1, {"size": [4, 3], "counts": [12]}, score=0.5)], gt, meter, images=images, gaze=gaze)
    with pytest.raises(ValueError, match="'image_id' is missing"):
        T.score_coco_records(dt, [{"category_id": 1, "segmentation": rle}], meter, images=images, gaze=gaze)
    assert meter.rows == []


# ------------------------------------------------------------------------------------------------------- the seeded inputs ---------
SIZES = [(1, 1), (5, 31), (7, 32), (9, 33), (64, 64), (65, 95), (130, 200), (257, 33), (600, 40)]      # the last two: two and three row bands
DENSITIES = (0.08, 0.5, 0.97)
RANGES = {1: ((1,), (2,), (17,)), 3: ((2, 0, 17), (17, 1, 0), (0, 17, 2)), 4: ((0, 1, 2, 17), (17, 2, 1, 0), (1, 0, 17, 2))}
SNAPS = (None, 0, 1, 2.5, 6)
OUTCOMES = ("one", "several", "snapped", "beyond", "none", "empty")


def _unwords(words, Ws):
    """(.., Hs, P) int32 -> (.., Hs, Ws) bool; the bits at x >= Ws are whatever they are and are no pixels"""
    w = np.ascontiguousarray(words).view(np.uint32)
    return ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(*w.shape[:-1], -1).astype(bool)[..., :Ws]


def _garbage(words, Ws, rng):
    """the words with random bits at x >= Ws"""
    out = words.copy()
    if Ws & 31:
        noise = rng.integers(0, 2 ** 32, size=out[..., -1].shape, dtype=np.uint64).astype(np.uint32) & np.uint32((0xFFFFFFFF << (Ws & 31)) & 0xFFFFFFFF)
        out[..., -1] = (out[..., -1].view(np.uint32) | noise).view(np.int32)
    return out


def _blob(rng, Hs, Ws, density):
    """a rectangle of random extent thinned to `density`; now and then the whole frame, a single pixel or nothing"""
    kind = rng.integers(0, 12)
    if kind == 0:
        return np.zeros((Hs, Ws), dtype=bool)
    if kind == 1:
        return dots(Hs, Ws, (int(rng.integers(0, Hs)), int(rng.integers(0, Ws))))
    y0, x0 = int(rng.integers(0, Hs)), int(rng.integers(0, Ws))
    y1, x1 = (Hs - 1, Ws - 1) if kind == 2 else (int(rng.integers(y0, Hs)), int(rng.integers(x0, Ws)))
    if kind == 2:
        y0 = x0 = 0
    return rect(Hs, Ws, y0, y1, x0, x1) & (rng.random((Hs, Ws)) < density)


def _case(seed, Hs, Ws, ranges, density, variant):
    rng = np.random.default_rng(seed)
    B, N = len(ranges), sum(ranges)
    masks = np.stack([_blob(rng, Hs, Ws, density) for _ in range(N)]) if N else np.zeros((0, Hs, Ws), dtype=bool)
    off = np.concatenate([[0], np.cumsum(ranges)]).astype(np.int32)
    for b in range(B):                                                           # one image in six has empty candidates only
        if rng.integers(0, 6) == 0:
            masks[off[b]:off[b + 1]] = False
    focus = rng.random((B, 2)).astype(np.float32)
    odd = rng.integers(0, 10, size=B)
    focus[odd == 0] = np.float32("nan")
    focus[odd == 1] *= 3.0
    focus[odd == 2] -= 1.0
    pred = np.stack([_blob(rng, Hs, Ws, max(density, 0.5)) for _ in range(B)]) if variant & 1 else None
    cat = rng.integers(-5, 2 ** 40, size=N).astype(np.int64) if variant & 2 else None
    snap2 = CR.snap2_of(SNAPS[int(rng.integers(0, len(SNAPS)))])
    want = CR.candidates(masks, off, focus, pred, cat, snap2)
    return {"Hs": Hs, "Ws": Ws, "masks": masks, "off": off, "focus": focus, "pred": pred, "cat": cat, "snap2": snap2, "want": want,
            "scratch_off": (variant >> 2) & 1, "seed": seed}


_CASES = {}


def _cases(Hs, Ws):
    """the seeded inputs of one size with their reference results, made once"""
    if (Hs, Ws) not in _CASES:
        out, k = [], 0
        for B in (1, 3, 4):
            for ranges, density in zip(RANGES[B], DENSITIES):
                for rep in range(2):
                    out.append(_case(1000 * Hs + Ws + 7919 * k, Hs, Ws, ranges, density, k % 8))
                    k += 1
        _CASES[(Hs, Ws)] = out
    return _CASES[(Hs, Ws)]


def test_the_seeded_inputs_reach_every_outcome():
    """On the reference alone, before any kernel runs: every outcome at least five times, with and without pred and cand_cat, both
    scratch alignments, every range length, and cuts of several row bands."""
    seen = dict.fromkeys(OUTCOMES, 0)
    variants, lengths = set(), set()
    for Hs, Ws in SIZES:
        for c in _cases(Hs, Ws):
            _g, sel, cand = c["want"]
            for b in range(len(c["off"]) - 1):
                seen[CR.outcome(sel[b], int(c["off"][b]), int(c["off"][b + 1]), cand)] += 1
                lengths.add(int(c["off"][b + 1] - c["off"][b]))
            variants.add((c["pred"] is not None, c["cat"] is not None, c["scratch_off"]))
    assert all(seen[k] >= 5 for k in OUTCOMES), seen
    assert len(variants) == 8 and lengths == {0, 1, 2, 17}
    assert _bands(257, 33) == 2 and _bands(600, 40) == 3                         # 17 candidates in a cut of several row bands
    best = [int(c["want"][1][b, 6]) for Hs, Ws in SIZES for c in _cases(Hs, Ws) for b in range(len(c["off"]) - 1) if c["pred"] is not None]
    assert sum(v >= 0 for v in best) >= 20 and sum(v < 0 for v in best) >= 5


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ----
POISON = -0x3C3C3C3D


def _kt():
    import kernel_testing as KT
    return KT


class Buf:
    """An output between kernel_testing's guard bands, pre-filled with its marker; off = 1 (int32) starts the body 4 bytes past the
    16-byte aligned address, and the element in front of it has to keep the marker."""

    def __init__(self, n, dtype=torch.int32, off=0):
        assert off == 0 or dtype == torch.int32
        self.out, self.off = _kt().Out(n + off, dtype), off

    @property
    def ptr(self):
        return self.out.ptr + 4 * self.off

    def get(self, complete=False):
        body = self.out.get(complete=False)
        assert bool((body[:self.off] == self.out.fill).all()), "the word in front of a misaligned body was written"
        assert not complete or not bool((body[self.off:] == self.out.fill).any()), "an element was not written"
        return body[self.off:]

    def untouched(self):
        return self.out.untouched()


def _abi(words, off, focus, Ws, pwords=None, cat=None, snap2=CR.OFF2, scratch_off=0, null_empty=True, words_off=0):
    """fs_mask_candidates at the C ABI; returns (gbits (B,Hs,P) int32, sel (B,8), cand (N,6)) as numpy, having checked the guard bands,
    that every element of the three outputs was written, and that the inputs are what they were."""
    N, Hs, P = words.shape
    B = len(off) - 1
    lead = np.full(words_off, POISON, dtype=np.int32)                            # words_off = 1: the candidates' words start 4 bytes past alignment
    ins = [torch.from_numpy(np.concatenate([lead, (words if N else np.full((1, Hs, P), POISON, dtype=np.int32)).reshape(-1)])).cuda(),
           torch.from_numpy(np.asarray(off, dtype=np.int32)).cuda(), torch.from_numpy(np.asarray(focus, dtype=np.float32).reshape(B, 2)).cuda()]
    if pwords is not None:
        ins.append(torch.from_numpy(np.ascontiguousarray(pwords)).cuda())
    if cat is not None:
        ins.append(torch.from_numpy(np.asarray(cat if N else [POISON], dtype=np.int64)).cuda())
    before = [t.clone() for t in ins]
    need = hip.query("fs_mask_candidates_scratch_ints", B, N, Hs, Ws)
    assert need == 4 + N * _bands(Hs, Ws) * 5
    cand, sel, gb, scr = Buf(N * 6, torch.int64), Buf(B * 8, torch.int64), Buf(B * Hs * P), Buf(need, off=scratch_off)
    hip.call("fs_mask_candidates", None if (N == 0 and null_empty) else ins[0].data_ptr() + 4 * words_off, ins[1].data_ptr(),
             None if cat is None else ins[-1].data_ptr(), ins[2].data_ptr(), None if pwords is None else ins[3].data_ptr(),
             None if (N == 0 and null_empty) else cand.ptr, sel.ptr, gb.ptr, scr.ptr, B, N, Hs, Ws, snap2)
    torch.cuda.synchronize()
    scr.get()
    for t, was in zip(ins, before):
        assert torch.equal(t.reshape(-1).view(torch.uint8), was.reshape(-1).view(torch.uint8))           # inputs are inputs, a NaN focus included
    return gb.get(True).numpy().reshape(B, Hs, P), sel.get(True).numpy().reshape(B, 8), cand.get(True).numpy().reshape(N, 6)


def _hold(c, words_off=0):
    """one seeded case through the C ABI, with garbage in the padding bits, against its reference"""
    rng = np.random.default_rng(c["seed"] + 1)
    Hs, Ws = c["Hs"], c["Ws"]
    P = (Ws + 31) // 32
    words = _garbage(np.stack([R.bits(m) for m in c["masks"]]) if len(c["masks"]) else np.zeros((0, Hs, P), dtype=np.int32), Ws, rng)
    pwords = None if c["pred"] is None else _garbage(np.stack([R.bits(m) for m in c["pred"]]), Ws, rng)
    gb, sel, cand = _abi(words, c["off"], c["focus"], Ws, pwords, c["cat"], c["snap2"], c["scratch_off"], words_off=words_off)
    g, wsel, wcand = c["want"]
    assert np.array_equal(cand, wcand), (c["seed"], cand.tolist(), wcand.tolist())
    assert np.array_equal(sel, wsel), (c["seed"], sel.tolist(), wsel.tolist())
    assert np.array_equal(gb, np.stack([R.bits(m) for m in g]))                  # the padding bits too: R.bits leaves them 0
    return gb, sel, cand


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", SIZES)
def test_mask_candidates_shapes(Hs, Ws):
    for c in _cases(Hs, Ws):
        _hold(c)


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", [(70, 128), (9, 225)])
def test_mask_candidates_four_words_a_load(Hs, Ws):
    """Rows of whole groups of four words (P = 4; P = 8 with a tail of one pixel) take the count pass's 16-byte loads where the planes
    are 16-byte aligned, and its one-word loads where the candidates' words are not: the same results on either path."""
    assert ((Ws + 31) // 32) % 4 == 0
    for k, c in enumerate(_cases(Hs, Ws)):
        _hold(c, words_off=k % 2)


@pytest.mark.gpu
def test_mask_candidates_hand_cases_on_the_device():
    H, W = 6, 10
    outer, inner = rect(H, W, 0, 5, 0, 7), rect(H, W, 1, 3, 2, 4)
    gb, sel, cand = _abi(np.stack([R.bits(outer), R.bits(inner)]), [0, 2], [foc(2, 3, H, W)], W, cat=[7, 8])
    assert sel.tolist() == [[1, 8, 0, 9, 0, 2, -1, 0]] and np.array_equal(gb[0], R.bits(inner))
    H, W = 5, 12
    two = np.stack([R.bits(dots(H, W, (2, 0), (2, 1), (2, 2))), R.bits(dots(H, W, (2, 8)))])
    for snap2, want in ((CR.OFF2, [1, 5, 9, 1, 0, 0, -1, 0]), (9, [1, 5, 9, 1, 0, 0, -1, 0]), (8, NONE), (0, NONE)):
        gb, sel, cand = _abi(two, [0, 2], [foc(2, 5, H, W)], W, cat=[4, 5], snap2=snap2)
        assert sel.tolist() == [want] and cand.tolist() == [[0, 3, 0, 9, 2, 2], [0, 1, 0, 9, 2, 8]]
    H, W = 2, 40
    a, b, c = dots(H, W, (0, 32)), dots(H, W, (0, 29)), dots(H, W, (0, 30), (0, 32))
    gb, sel, cand = _abi(np.stack([R.bits(m) for m in (b, c, a)]), [0, 3], [foc(0, 31, H, W)], W)
    assert cand.tolist() == [[0, 1, 0, 4, 0, 29], [0, 2, 0, 1, 0, 30], [0, 1, 0, 1, 0, 32]] and sel.tolist() == [[2, -1, 1, 1, 0, 0, -1, 0]]
    H, W = 4, 8
    pred = rect(H, W, 0, 1, 0, 3)
    four = [rect(H, W, 0, 3, 0, 3), rect(H, W, 1, 3, 3, 7), rect(H, W, 0, 1, 2, 3), rect(H, W, 0, 1, 0, 1)]
    gb, sel, cand = _abi(np.stack([R.bits(m) for m in four]), [0, 4], [foc(3, 7, H, W)], W, pwords=R.bits(pred)[None])
    assert sel.tolist() == [[1, -1, 0, 15, 1, 1, 2, 0]] and cand[:, 1:3].tolist() == [[16, 8], [15, 1], [4, 4], [4, 4]]
    H, W = 4, 6
    masks = np.stack([R.bits(dots(H, W, (0, 0))), R.bits(dots(H, W, (3, 5)))] * 3)
    focus = [[float("nan"), float("nan")], [2.0, 7.5], [-1.0, 2.0]]
    gb, sel, cand = _abi(masks, [0, 2, 4, 6], focus, W)
    assert sel.tolist() == [[0, -1, 0, 1, 0, 1, -1, 0], [3, -1, 0, 1, 0, 1, -1, 0], [5, -1, 9, 1, 0, 0, -1, 0]]


@pytest.mark.gpu
def test_mask_candidates_large():
    """1300 x 1024 with 40 candidates over three images: 6 bands a candidate (21 in the copy pass), a bisection over four offsets"""
    Hs, Ws = 1300, 1024
    c = _case(32, Hs, Ws, (23, 0, 17), 0.6, 7)                                   # contained by four; no candidate; snapped over one pixel
    assert _bands(Hs, Ws) == 6 and len(c["masks"]) == 40
    gb, sel, cand = _hold(c)
    assert sel[:, 0].tolist() == [2, -1, 33] and sel[:, 2].tolist() == [0, -1, 1] and sel[:, 5].tolist() == [4, 0, 0]
    assert sel[:, 6].tolist() == [18, -1, 27] and int(cand[:, 1].max()) > 100000


def _small():
    Hs, Ws = 9, 33
    rng = np.random.default_rng(5)
    masks = np.stack([_blob(rng, Hs, Ws, 0.7) for _ in range(5)])
    masks[0, 4, 16] = masks[3, 4, 16] = True
    return Hs, Ws, masks, _garbage(np.stack([R.bits(m) for m in masks]), Ws, rng), [foc(4, 16, Hs, Ws)] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("off", [[1, 2, 4, 5], [0, 3, 2, 5], [0, 2, 4, 4], [0, 2, 4, 6], [POISON, 2, 4, 5], [0, 2 ** 31 - 1, -(2 ** 31), 5]])
def test_mask_candidates_malformed_offsets(off):
    """First not 0, a decrease, last != N (below and above), and values far outside: status 1 everywhere, zero gbits, the areas alone in
    cand, and untouched guard bands (checked in _abi)."""
    Hs, Ws, masks, words, focus = _small()
    good = _abi(words, [0, 2, 4, 5], focus, Ws, cat=[1, 2, 3, 4, 5])
    assert good[1][:, 7].tolist() == [0, 0, 0] and good[1][0, 0] >= 0
    pred = np.stack([R.bits(masks[1])] * 3)
    for pw, cat in ((None, None), (pred, [1, 2, 3, 4, 5])):
        gb, sel, cand = _abi(words, off, focus, Ws, pwords=pw, cat=cat, scratch_off=1)
        assert sel.tolist() == [[-1, -1, -1, 0, 0, 0, -1, 1]] * 3 and not gb.any()
        assert cand.tolist() == [[-1, int(m.sum()), 0, -1, -1, -1] for m in masks]
        g, wsel, wcand = CR.candidates(masks, off, focus, None if pw is None else [masks[1]] * 3, cat)
        assert np.array_equal(sel, wsel) and np.array_equal(cand, wcand)


@pytest.mark.gpu
def test_mask_candidates_without_candidates():
    Hs, Ws = 9, 33
    focus = [foc(4, 16, Hs, Ws)] * 2
    for null_empty in (True, False):
        gb, sel, cand = _abi(np.zeros((0, Hs, 2), dtype=np.int32), [0, 0, 0], focus, Ws, pwords=np.full((2, Hs, 2), -1, dtype=np.int32), cat=[],
                             null_empty=null_empty)
        assert sel.tolist() == [NONE, NONE] and not gb.any() and cand.shape == (0, 6)
    gb, sel, cand = _abi(np.zeros((0, Hs, 2), dtype=np.int32), [0, 0, 1], focus, Ws)          # the last offset is not N = 0
    assert sel[:, 7].tolist() == [1, 1] and not gb.any()


@pytest.mark.gpu
def test_rejected_arguments_leave_the_outputs_alone():
    Hs, Ws, masks, words, focus = _small()
    B, N, P = 3, 5, 2
    cd, od, fd = torch.from_numpy(words).cuda(), torch.tensor([0, 2, 4, 5], dtype=torch.int32).cuda(), torch.tensor(focus, dtype=torch.float32).cuda()
    pd, kd = torch.from_numpy(words[:3].copy()).cuda(), torch.arange(5, dtype=torch.int64).cuda()
    cand, sel, gb = Buf(N * 6, torch.int64), Buf(B * 8, torch.int64), Buf(B * Hs * P)
    scr = Buf(hip.query("fs_mask_candidates_scratch_ints", B, N, Hs, Ws))

    def rejected(*args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call("fs_mask_candidates", *args)

    good = [cd.data_ptr(), od.data_ptr(), kd.data_ptr(), fd.data_ptr(), pd.data_ptr(), cand.ptr, sel.ptr, gb.ptr, scr.ptr]
    for i in (0, 1, 3, 5, 6, 7, 8):                                              # cand_cat and pbits may be null
        a = list(good)
        a[i] = None
        rejected(*a, B, N, Hs, Ws, 4)
    a = list(good)
    a[7] = a[0]
    rejected(*a, B, N, Hs, Ws, 4)                                                # gbits == cbits
    for dims in ((0, N, Hs, Ws, 4), (-1, N, Hs, Ws, 4), (B, -1, Hs, Ws, 4), (B, N, 0, Ws, 4), (B, N, Hs, 0, 4), (B, N, -9, Ws, 4), (B, N, Hs, -1, 4),
                 (B, N, 16385, Ws, 4), (B, N, Hs, 16385, 4),                     # a side above 16384
                 (B, 2 ** 31 - 1, 16384, Ws, 4),                                 # N times 64 bands is beyond int range
                 (B, N, Hs, Ws, -1)):                                            # snap2 < 0
        rejected(*good, *dims)
    torch.cuda.synchronize()
    assert cand.untouched() and sel.untouched() and gb.untouched() and scr.untouched()
    hip.call("fs_mask_candidates", *good, B, N, Hs, Ws, 4)                       # and the same pointers are taken with the sizes they were made for
    torch.cuda.synchronize()
    g, wsel, wcand = CR.candidates(masks, [0, 2, 4, 5], focus, masks[:3], [0, 1, 2, 3, 4], 4)
    assert np.array_equal(sel.get(True).numpy().reshape(B, 8), wsel) and np.array_equal(cand.get(True).numpy().reshape(N, 6), wcand)
    assert np.array_equal(gb.get(True).numpy().reshape(B, Hs, P), np.stack([R.bits(m) for m in g]))


# ------------------------------------------------------------------------------------------------- GPU: the composed calls ---------
@pytest.mark.gpu
def test_ops_mask_candidates_is_the_c_abi_call():
    for c in _cases(65, 95)[4:10] + _cases(9, 33)[:4]:
        Ws = c["Ws"]
        rng = np.random.default_rng(c["seed"] + 1)
        words = _garbage(np.stack([R.bits(m) for m in c["masks"]]), Ws, rng)
        pwords = None if c["pred"] is None else np.stack([R.bits(m) for m in c["pred"]])
        snap_px = None if c["snap2"] == CR.OFF2 else math.sqrt(c["snap2"]) + 1e-9
        assert CR.snap2_of(snap_px) == c["snap2"]
        want = _abi(words, c["off"], c["focus"], Ws, pwords, c["cat"], c["snap2"])
        got = ops.mask_candidates(torch.from_numpy(words).cuda(), torch.from_numpy(c["off"]).cuda(), torch.from_numpy(c["focus"]).cuda(), Ws,
                                  pred=None if pwords is None else torch.from_numpy(pwords).cuda(),
                                  cand_cat=None if c["cat"] is None else torch.from_numpy(c["cat"]).cuda(), snap_px=snap_px)
        assert [t.dtype for t in got] == [torch.int32, torch.int64, torch.int64]
        for a, b in zip(got, want):
            assert torch.equal(a.cpu(), torch.from_numpy(b))
        again = ops.mask_candidates(torch.from_numpy(words).cuda(), torch.from_numpy(c["off"]).cuda(), torch.from_numpy(c["focus"]).cuda(), Ws,
                                    pred=None if pwords is None else torch.from_numpy(pwords).cuda(),
                                    cand_cat=None if c["cat"] is None else torch.from_numpy(c["cat"]).cuda(), snap_px=snap_px)
        assert all(torch.equal(a, b) for a, b in zip(got, again))                # the same bits in every run
    # one candidate an image: gbits is that candidate with the tail masked, wherever the gaze is
    Hs, Ws = 9, 33
    rng = np.random.default_rng(6)
    masks = np.stack([_blob(rng, Hs, Ws, 0.5) | dots(Hs, Ws, (8, 32)) for _ in range(4)])
    words = _garbage(np.stack([R.bits(m) for m in masks]), Ws, rng)
    gbits, sel, cand = ops.mask_candidates(torch.from_numpy(words).cuda(), torch.arange(5, dtype=torch.int32).cuda(), torch.rand(4, 2).cuda(), Ws)
    clean = torch.from_numpy(np.stack([R.bits(m) for m in masks])).cuda()
    assert torch.equal(gbits, clean) and not torch.equal(gbits, torch.from_numpy(words).cuda()) and sel[:, 0].tolist() == [0, 1, 2, 3]
    assert torch.equal(gbits[:, :, -1], torch.from_numpy(words).cuda()[:, :, -1] & 1)
    # N = 0 through ops
    gbits, sel, cand = ops.mask_candidates(torch.zeros(0, Hs, 2, dtype=torch.int32).cuda(), torch.zeros(3, dtype=torch.int32).cuda(),
                                           torch.rand(2, 2).cuda(), Ws, cand_cat=torch.zeros(0, dtype=torch.int64).cuda())
    assert sel.tolist() == [NONE, NONE] and not gbits.any() and tuple(cand.shape) == (0, 6)


HS, WS = 37, 70


def _annotations(rng, H, W, n, image_id, first_ann, empty=False):
    """n annotation records of one image, polygons (rectangles and triangles) and run-length codes mixed, with their dense masks"""
    recs, masks = [], []
    for j in range(n):
        kind = ("poly", "rle", "str")[int(rng.integers(0, 3))]
        if empty:
            m, seg = np.zeros((H, W), dtype=bool), {"size": [H, W], "counts": [H * W]}
        elif kind == "poly":
            pts = [(float(rng.integers(0, 2 * W)) / 2, float(rng.integers(0, 2 * H)) / 2) for _ in range(int(rng.integers(3, 6)))]
            seg = [[v for xy in pts for v in xy]]
            m = PR.poly_mask_rows(PR.coco_rings(seg), H, W)
        else:
            y0, x0 = int(rng.integers(0, H - 2)), int(rng.integers(0, W - 2))
            m = rect(H, W, y0, int(rng.integers(y0, H)), x0, int(rng.integers(x0, W))) & (rng.random((H, W)) < 0.8)
            seg = {"size": [H, W], "counts": ops.rle_to_string(R.encode(m)) if kind == "str" else R.encode(m)}
        recs.append(_rec(image_id, seg, cat=int(rng.integers(0, 5)), ann=first_ann + j))
        masks.append(m)
    return recs, masks


@pytest.mark.gpu
def test_coco_candidates_groups_by_image():
    rng = np.random.default_rng(21)
    per = {}
    for k, (image_id, n) in enumerate((("a", 3), (7, 1), ("c", 4))):
        per[image_id] = _annotations(rng, HS, WS, n, image_id, 100 * k)
    # the file's order interleaves the images; "b" has no record at all
    order = [("a", 0), ("c", 0), (7, 0), ("c", 1), ("a", 1), ("c", 2), ("a", 2), ("c", 3)]
    records = json.loads(json.dumps([per[i][0][j] for i, j in order]))
    image_ids = ["c", "b", "a", 7]
    cbits, off, cat, info, rows = ops.coco_candidates(records, (HS, WS), "cuda", image_ids)
    assert off.dtype == torch.int32 and off.tolist() == [0, 4, 4, 7, 8] and rows == [1, 3, 5, 7, 0, 4, 6, 2]
    want = [per[i][1][j] for i, j in (order[r] for r in rows)]
    assert torch.equal(cbits, torch.from_numpy(np.stack([R.bits(m) for m in want])).cuda())
    assert cat.tolist() == [records[r]["category_id"] for r in rows] and info.tolist() == [[0, int(m.sum())] for m in want]
    assert [records[r]["id"] for r in rows] == [200, 201, 202, 203, 0, 1, 2, 100]
    # through the selection and back to the annotation's id
    focus = torch.tensor([foc(*np.argwhere(per[i][1][0])[0], HS, WS) if i != "b" else [0.5, 0.5] for i in image_ids]).cuda()
    gbits, sel, _ = ops.mask_candidates(cbits, off, focus, WS, cand_cat=cat)
    g, wsel, _ = CR.candidates(np.stack(want), off.tolist(), focus.cpu().numpy(), None, cat.tolist())
    assert np.array_equal(sel.cpu().numpy(), wsel) and sel[1].tolist() == NONE and int(sel[3, 0]) == 7 and records[rows[int(sel[3, 0])]]["id"] == 100
    # records with a score are annotations all the same
    again = ops.coco_candidates([dict(r, score=0.5) if i % 2 else r for i, r in enumerate(records)], (HS, WS), "cuda", image_ids)
    assert torch.equal(again[0], cbits) and again[4] == rows


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.gpu
def test_evaluate_instances_with_candidates():
    import test_predict as TP
    module, _ = TP._module("hrnet")
    size = 128
    X, Fp, Y, cls = T.synthetic_batch(2, size, size, seed=11, device="cuda")
    rng = np.random.default_rng(22)
    masks = np.stack([_blob(rng, size, size, 0.9) for _ in range(7)])
    py, px = CR.gaze_pixel(Fp[0].cpu().numpy(), size, size)
    masks[1] = rect(size, size, max(py - 20, 0), min(py + 20, size - 1), max(px - 30, 0), min(px + 30, size - 1))
    masks[2] = rect(size, size, max(py - 5, 0), min(py + 5, size - 1), max(px - 5, 0), min(px + 5, size - 1))
    off, cat = [0, 4, 7], [3, 1, 4, 1, 5, 9, 2]
    cbits = ops.mask_bits(torch.from_numpy(masks).cuda())
    cand = (cbits, torch.tensor(off, dtype=torch.int32).cuda(), torch.tensor(cat, dtype=torch.int64).cuda())
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        for kw, snap in (({}, None), ({"component": 8, "snap_px": 40.0}, 3.0)):
            rec = module.predict_instances(X, Fp, (size, size), return_bits=True, return_score=True, **kw)
            got = module.evaluate_instances(X, Fp, seg_size=(size, size), candidates=cand, cand_snap_px=snap, **kw)
            step = T.evaluate_instances_step(module, (X, Fp, Y, cls), meter := T.InstanceAPMeter("cuda", 12), seg_size=(size, size), candidates=cand,
                                             cand_snap_px=snap, **kw)
            assert len(got) == len(rec) + 1 == len(step)                         # the bits leave, pair and sel come
            for a, b in zip(got[:-2], rec[:3] + rec[4:]):
                assert _same(a, b)
            pred = _unwords(rec[3].cpu().numpy(), size)
            g, wsel, _ = CR.candidates(masks, off, Fp.cpu().numpy(), pred, cat, CR.snap2_of(snap))
            assert np.array_equal(got[-1].cpu().numpy(), wsel) and int(wsel[0, 0]) == 2 and int(wsel[0, 5]) >= 2
            d = ops.boundary_dilation(size, size, 0.02)
            assert torch.equal(got[-2], ops.mask_pair_counts(rec[3], ops.mask_bits(torch.from_numpy(g).cuda()), d, Ws=size))
            assert all(_same(a, b) for a, b in zip(got, step))
            row = torch.cat(meter.rows)
            assert row[:, 1].tolist() == wsel[:, 1].tolist() and torch.equal(row[:, 3:9], got[-2])
        # without the keyword: the positional call, the keyword call and the step are one call, results and peak memory
        module.evaluate_instances(X, Fp, Y, cls)                                 # caches are warm before anything is measured
        outs, peaks = [], []
        for call in (lambda: module.evaluate_instances(X, Fp, Y, cls), lambda: module.evaluate_instances(X, Fp, seg_label=Y, cls_label=cls),
                     lambda: T.evaluate_instances_step(module, (X, Fp, Y, cls))):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            held = torch.cuda.memory_allocated()                                 # the earlier calls' results are still alive
            outs.append(call())
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated() - held)
        assert len(outs[0]) == 5 and all(len(o) == 5 and all(_same(a, b) for a, b in zip(o, outs[0])) for o in outs[1:])
        assert peaks[0] == peaks[1] == peaks[2]
    finally:
        hip.set_deterministic(was)
    for args, kw in (((X, Fp, Y, cls), {"candidates": cand, "seg_size": (size, size)}), ((X, Fp, None, cls), {"candidates": cand, "seg_size": (size, size)}),
                     ((X, Fp), {"candidates": cand}), ((X, Fp), {"candidates": cand[:2], "seg_size": (size, size)}),
                     ((X, Fp), {"candidates": cand, "seg_size": (size, size), "cand_snap_px": -1}),
                     ((X, Fp), {"candidates": cand, "seg_size": (64, size)}), ((X, Fp), {"candidates": (cbits, cand[1][:2], None), "seg_size": (size, size)}),
                     ((X, Fp, Y, cls), {"cand_snap_px": 3.0})):
        with pytest.raises(ValueError):
            module.evaluate_instances(*args, **kw)
    with pytest.raises(TypeError):
        module.evaluate_instances(X, Fp)


@pytest.mark.gpu
def test_score_coco_records_with_a_gaze():
    """~12 images of two sizes with 1 - 6 annotations each: the meter's rows are those of the reference-selected annotation per image
    fed through the one-instance path."""
    rng = np.random.default_rng(23)
    sizes = [(HS, WS), (20, 33)]
    gt, single, dt, gaze, images = [], [], [], {}, []
    chosen = []
    for k in range(12):
        H, W = sizes[k % 3 == 1]
        image_id = f"im{k}" if k % 2 else k
        recs, masks = _annotations(rng, H, W, 1 + k % 6, image_id, 10 * k, empty=(k == 9))
        gaze[image_id] = (float(rng.random()), float(rng.random())) if k % 4 else foc(*np.argwhere(masks[-1])[0], H, W)
        found = np.roll(masks[int(rng.integers(0, len(masks)))], 1, 1)
        if k != 5:                                                               # image 5 has no result
            dt.append(_rec(image_id, {"size": [H, W], "counts": R.encode(found)}, cat=recs[0]["category_id"], score=0.25 + k / 16))
        g, sel, _ = CR.candidates(np.stack(masks), [0, len(masks)], [gaze[image_id]], [found], [r["category_id"] for r in recs])
        chosen.append(int(sel[0, 0]))
        single.append(recs[chosen[-1]] if chosen[-1] >= 0 else _rec(image_id, {"size": [H, W], "counts": [H * W]}, cat=-1))
        gt.extend(recs)
        images.append({"id": image_id, "height": H, "width": W})
    assert chosen[9] == -1 and sum(c > 0 for c in chosen) >= 3 and len(gt) > 30
    gt, single, dt = (json.loads(json.dumps(v)) for v in (gt, single, dt))
    old, new, whole = (T.InstanceAPMeter("cuda", 5) for _ in range(3))
    with pytest.raises(ValueError, match="more than one record"):
        T.score_coco_records(dt, gt, old, images=images)
    assert old.rows == []
    assert T.score_coco_records(dt, single, old, chunk=4, images=images) == 12
    assert T.score_coco_records(dt, gt, new, chunk=4, images=images, gaze=gaze) == 12
    assert T.score_coco_records(dt, gt, whole, images=images, gaze=gaze) == 12
    assert len(new.rows) == 3 and len(whole.rows) == 2
    assert torch.equal(torch.cat(new.rows), torch.cat(old.rows)) and torch.equal(torch.cat(whole.rows), torch.cat(old.rows))
    res = new.result()
    assert res["n_images"] == 12 and 8 <= res["n_records"] <= 11 and res["mIoU"] > 0.0


# ------------------------------------------------------------- the component's seed and the candidate choice: one gaze pixel, one key ----
AGREE_SIZES = [(1, 1), (1, 70), (8, 32), (8, 33), (9, 7), (37, 300)]   # one word; a tail word; a word boundary; a row beyond a wave's words


def _exact_gazes(side):
    """The fp32 focus values whose 1/16-pixel product is exact: (k + 0.5 for an even k, for an odd k, 16 j + 8), or None for side 1,
    where every product is 0.  side - 1 = odd * 2^e: i / 2^(e+5) gives odd * i / 2, i / 2^(e+1) gives 8 * odd * i -- dyadic, so exact."""
    if side == 1:
        return None
    odd, e = side - 1, 0
    while odd % 2 == 0:
        odd, e = odd // 2, e + 1
    a, b, c = 1.0 / 2 ** (e + 5), 3.0 / 2 ** (e + 5), 1.0 / 2 ** (e + 1)
    top = float((side - 1) * 16)
    ka, kb = (odd - 1) // 2, (3 * odd - 1) // 2
    assert all(float(np.float32(v)) == v and v <= 1.0 for v in (a, b, c)) and (ka + kb) % 2 == 1
    assert a * top == ka + 0.5 and b * top == kb + 0.5 and c * top == 8 * odd and (8 * odd) % 16 == 8
    even, other = (a, b) if ka % 2 == 0 else (b, a)
    return even, other, c


def _agree_gazes(Hs, Ws):
    """(row, col) focus pairs: the corners, rint's ties to an even and to an odd k on either axis, the pixel-rounding tie, NaN and values
    outside [0, 1]"""
    ey, ex = _exact_gazes(Hs) or (0.5, 0.5, 0.5), _exact_gazes(Ws) or (0.5, 0.5, 0.5)
    nan = float("nan")
    return [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (ey[0], ex[1]), (ey[1], ex[0]), (ey[2], ex[2]), (nan, nan), (nan, 0.5),
            (-0.25, 1.5), (1.5, -0.25)]


def test_the_tie_gazes_are_ties():
    """rint goes to the even neighbour on both kinds of tie, and the pixel tie 16 j + 8 goes up to pixel j + 1: on the references, whose
    two restatements of the gaze must be one function"""
    for side in sorted({v for hw in AGREE_SIZES for v in hw} - {1}):
        even, other, c = _exact_gazes(side)
        top = (side - 1) * 16
        for f in (even, other):
            k = int(math.floor(f * top))
            assert CP.gaze(f, side) == CR.gaze(f, side) == (k if k % 2 == 0 else k + 1)
        assert int(math.floor(even * top)) % 2 == 0 and int(math.floor(other * top)) % 2 == 1
        g = CP.gaze(c, side)
        assert g == CR.gaze(c, side) and g % 16 == 8 and CP.gaze_pixel((c, c), side, side) == ((g >> 4) + 1,) * 2
    for f in (float("nan"), -0.25, 1.5, 0.0, 1.0):
        assert all(CP.gaze(f, side) == CR.gaze(f, side) for side in (1, 7, 300))


_AGREE = {}


def _agree_case(Hs, Ws):
    """B = 3 seeded masks of a size (density 0.02, 0.5 and an empty one), and for every gaze the two references' answers, made once:
    (focus (3,2), snap2, comp (3,4) of component_ref, (sel, cand) of candidates_ref with one candidate an image equal to the mask)"""
    if (Hs, Ws) not in _AGREE:
        rng = np.random.default_rng(4000 * Hs + Ws)
        masks = np.stack([rng.random((Hs, Ws)) < 0.02, rng.random((Hs, Ws)) < 0.5, np.zeros((Hs, Ws), dtype=bool)])
        rows = []
        for k, fo in enumerate(_agree_gazes(Hs, Ws)):
            focus = np.array([fo] * 3, dtype=np.float32)
            snap2 = CR.OFF2 if k % 2 == 0 else 2                                 # every other gaze with a snap distance of sqrt(2)
            _c, comp = CP.component_batch(masks, focus, 8, snap2)
            _g, sel, cand = CR.candidates(masks, [0, 1, 2, 3], focus, snap2=snap2)
            rows.append((focus, snap2, comp, sel, cand))
        _AGREE[(Hs, Ws)] = (masks, rows)
    return _AGREE[(Hs, Ws)]


def _agree(comp, sel, cand, snap2):
    """fs_mask_component's comp rows and fs_mask_candidates' rows of one candidate an image say the same: the nearest pixel and its
    squared distance (none for an empty mask), the area, and the seed is taken where the selection is"""
    for b in range(3):
        sy, sx, d2, area = (int(v) for v in comp[b])
        assert cand[b].tolist()[:2] == [b, area] and area == int(sel[b, 3] if sel[b, 0] >= 0 else cand[b, 1])
        assert (sel[b, 0] >= 0) == (sy >= 0) == (area > 0 and int(cand[b, 3]) <= snap2)
        if sy >= 0:
            assert [d2, sy, sx] == cand[b].tolist()[3:] and int(sel[b, 0]) == b and int(sel[b, 2]) == d2
        else:
            assert [sy, sx, d2] == [-1, -1, -1] and sel[b].tolist()[:3] == [-1, -1, -1]
            assert (area == 0) == (cand[b].tolist()[3:] == [-1, -1, -1])


@pytest.mark.parametrize("Hs,Ws", AGREE_SIZES)
def test_reference_seed_and_candidate_choice_agree(Hs, Ws):
    """component_ref and candidates_ref, written apart, on the inputs of the device test below"""
    masks, rows = _agree_case(Hs, Ws)
    seen = set()
    for focus, snap2, comp, sel, cand in rows:
        _agree(comp, sel, cand, snap2)
        assert CP.gaze_pixel(focus[0], Hs, Ws) == CR.gaze_pixel(focus[0], Hs, Ws)
        seen |= {(int(comp[b, 0]) >= 0, int(comp[b, 3]) > 0) for b in range(3)}
    assert (False, False) in seen and ((True, True) in seen or Hs * Ws == 1)


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", AGREE_SIZES)
def test_component_seed_and_candidate_choice_agree(Hs, Ws):
    """One candidate an image equal to the mask: fs_mask_component's seed and fs_mask_candidates' nearest pixel are the same pixel at
    the same squared distance with the same area, for gazes on the corners, on both kinds of rounding tie, NaN and outside [0, 1] --
    and each is its own reference's."""
    masks, rows = _agree_case(Hs, Ws)
    rng = np.random.default_rng(Hs + Ws)
    words = _garbage(np.stack([R.bits(m) for m in masks]), Ws, rng)
    bits = torch.from_numpy(words).cuda()
    need = hip.query("fs_mask_component_scratch_ints", 3, Hs, Ws)
    for focus, snap2, wcomp, wsel, wcand in rows:
        out, comp, scr = Buf(words.size), Buf(12, torch.int64), Buf(need)
        f = torch.from_numpy(focus).cuda()
        hip.call("fs_mask_component", bits.data_ptr(), f.data_ptr(), out.ptr, comp.ptr, scr.ptr, 3, Hs, Ws, 8, snap2)
        torch.cuda.synchronize()
        comp = comp.get(True).numpy().reshape(3, 4)
        _gb, sel, cand = _abi(words, [0, 1, 2, 3], focus, Ws, snap2=snap2)
        assert np.array_equal(comp, wcomp) and np.array_equal(sel, wsel) and np.array_equal(cand, wcand), (focus[0].tolist(), snap2)
        _agree(comp, sel, cand, snap2)
