"""COCO / LVIS polygon lists into bit words: fs_poly_bits, fs_poly_bits_scratch_ints, fs_poly_bits_band_rows, ops.polygon_rings,
ops.poly_bits, ops.coco_masks and train.score_coco_records(images=...).

The rule is UNPINNED: the reference rasterises with skimage.draw.polygon (b2_preprocess_lvis.py:282-297), which is not at hand, so
tests/poly_ref.py restates the library's definition -- clamped rounded vertices, the outline's lattice points, the even-odd crossing
number inside, the OR of the rings -- and is held here to hand-derived answers and, away from the outline, to matplotlib's
point-in-path test before anything on the device is held to it.  Every comparison is == / torch.equal: nothing here has a tolerance."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fovealseg import hip, ops
from fovealseg import train as T

import poly_ref as PR
import rle_ref as R


def parse(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


# ------------------------------------------------------------------------------------------------ the hand-derived answers --------
# Rings are (y, x) vertices.  Each picture was drawn from the definition by hand (the derivations are beside the cases).
HAND = {
    # right angle at (0,0); the hypotenuse (4,0)-(0,6) has gcd(4, 6) + 1 = 3 lattice points: (4,0), (2,3), (0,6).  Inside: 2x + 3y < 12.
    # row 1: 2x < 9 -> x <= 4; row 2: 2x < 6 -> x <= 2, and (2,3) lies on the hypotenuse; row 3: x <= 1; row 4: the vertex alone.
    "triangle": ([[(0, 0), (4, 0), (0, 6)]], 6, 8,
                 ["#######.", "#####...", "####....", "##......", "#.......", "........"]),
    # the diagonal (0,0)-(4,4) carries a lattice point on every row
    "triangle45": ([[(0, 0), (4, 0), (4, 4)]], 6, 8,
                   ["#.......", "##......", "###.....", "####....", "#####...", "........"]),
    # closed: [1,1]-[3,4] sets 3 x 4 pixels
    "rectangle": ([[(1, 1), (1, 4), (3, 4), (3, 1)]], 5, 7,
                  [".......", ".####..", ".####..", ".####..", "......."]),
    "one_vertex": ([[(2, 5)]], 4, 8, ["........", "........", ".....#..", "........"]),
    # the segment (0,0)-(2,4): lattice points (0,0), (1,2), (2,4); its two edges cancel in the crossing number
    "two_vertices": ([[(0, 0), (2, 4)]], 4, 8, ["#.......", "..#.....", "....#...", "........"]),
    "repeated_vertex": ([[(1, 1), (1, 1), (1, 4), (3, 4), (3, 1)]], 5, 7,
                        [".......", ".####..", ".####..", ".####..", "......."]),
    "collinear": ([[(1, 1), (1, 2), (1, 4), (3, 4), (2, 4), (3, 1)]], 5, 7,          # (2,4) lies on the right side: then the ring cuts back
                  None),
    # (0,0) -> (4,4) -> (0,4) -> (4,0): two triangles that meet in (2,2); the wedges above and below the crossing are outside
    "bow_tie": ([[(0, 0), (4, 4), (0, 4), (4, 0)]], 5, 6,
                ["#...#.", "##.##.", "#####.", "##.##.", "#...#."]),
    # A = rows 0-4 x columns 0-5, B = rows 2-6 x columns 3-9, as two rings: the union, 30 + 35 - 9 = 56 pixels
    "two_rectangles": ([[(0, 0), (0, 5), (4, 5), (4, 0)], [(2, 3), (2, 9), (6, 9), (6, 3)]], 8, 11,
                       ["######.....", "######.....", "##########.", "##########.", "##########.", "...#######.", "...#######.", "..........."]),
    # the same outline as ONE ring through the common point (2,5): A, then B.  The overlap rows 2-4 x columns 3-5 is crossed twice,
    # so only its outline stays -- row 2 (B's top), row 4 (A's bottom), column 3 (B's left), column 5 (A's right): (3,4) alone is unset
    "self_overlap": ([[(2, 5), (4, 5), (4, 0), (0, 0), (0, 5), (2, 5), (2, 9), (6, 9), (6, 3), (2, 3)]], 8, 11,
                     ["######.....", "######.....", "##########.", "####.#####.", "##########.", "...#######.", "...#######.", "..........."]),
    # vertices (3,0) and (3,6) lie on the row between two edges each: row 3 is there once, and whole
    "diamond": ([[(0, 3), (3, 6), (6, 3), (3, 0)]], 7, 8,
                ["...#....", "..###...", ".#####..", "#######.", ".#####..", "..###...", "...#...."]),
    # the apex (2,2) parts the edges (0,0)-(2,2), rows 0-1, and (2,2)-(4,0), rows 2-3
    "apex": ([[(0, 0), (2, 2), (4, 0)]], 5, 4, ["#...", "##..", "###.", "##..", "#..."]),
    # clipped onto the border, not wrapped: (-5,-3), (-5,100), (2,100), (2,-3) -> (0,0), (0,9), (2,9), (2,0)
    "clipped": ([[(-5, -3), (-5, 100), (2, 100), (2, -3)]], 4, 10,
                ["##########", "##########", "##########", ".........."]),
    "wide": ([[(1, 2), (1, 38), (6, 38), (6, 2)]], 8, 40,
             ["." * 40] + [".." + "#" * 37 + "."] * 6 + ["." * 40]),                   # columns 2 - 38 across a word border
}
# "collinear": the ring (1,1) (1,2) (1,4) (3,4) (2,4) (3,1).  (1,2) lies on the top side and changes nothing.  The outline then runs
# down the right side to (3,4), back up it to (2,4) and from there to (3,1): the triangle (2,4), (3,4), (3,1) is cut away, and of the
# bottom row only what the edge (2,4)-(3,1) -- lattice points its two ends, gcd(1, 3) = 1 -- and the edge (3,1)-(1,1) touch.  Row 2: the
# slanted edge sits at x = 4 there, so columns 1-4.  Row 3: x < 1 + 0 inside -> nothing; the vertices (3,1) and (3,4) on the outline.
HAND["collinear"] = (HAND["collinear"][0], 5, 7, [".......", ".####..", ".####..", ".#..#..", "......."])


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_by_hand(name):
    rings, H, W, rows = HAND[name]
    assert H <= 8 and W <= 40
    want = parse(rows)
    assert want.shape == (H, W)
    assert np.array_equal(PR.poly_mask(rings, H, W), want), name
    assert np.array_equal(PR.poly_mask_rows(rings, H, W), want), name


def test_reference_counts_by_hand():
    assert int(parse(HAND["rectangle"][3]).sum()) == 12
    assert int(parse(HAND["two_rectangles"][3]).sum()) == 56 and int(parse(HAND["self_overlap"][3]).sum()) == 55
    two, one = parse(HAND["two_rectangles"][3]), parse(HAND["self_overlap"][3])
    assert np.argwhere(two != one).tolist() == [[3, 4]]                      # 0 pixels cancelled in the union; one in the single ring


def test_reference_rounds_half_to_even():
    assert [PR.rne(v) for v in (0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 0.49999, 2.50001, 7.0, -7.0)] == [0, 2, 2, 4, 0, -2, -2, 0, 3, 7, -7]
    # x: 0.5 -> 0, 2.5 -> 2; y: 0.5 -> 0, 1.5 -> 2: the closed rectangle rows 0-2 x columns 0-2
    rings = PR.coco_rings([[0.5, 0.5, 2.5, 0.5, 2.5, 1.5, 0.5, 1.5]])
    assert rings == [[(0, 0), (0, 2), (2, 2), (2, 0)]]
    assert np.array_equal(PR.poly_mask(rings, 4, 5), parse(["###..", "###..", "###..", "....."]))


def test_row_form_of_the_reference_is_the_double_loop():
    rng = np.random.default_rng(30)
    for _ in range(150):
        H, W = int(rng.integers(1, 14)), int(rng.integers(1, 40))
        rings = [[(int(rng.integers(-3, H + 3)), int(rng.integers(-3, W + 3))) for _ in range(int(rng.integers(1, 10)))]
                 for _ in range(int(rng.integers(0, 4)))]
        assert np.array_equal(PR.poly_mask_rows(rings, H, W), PR.poly_mask(rings, H, W))


# ------------------------------------------------------------------------------------- CPU: the yardstick away from the outline ----
def _hull(points):
    """Andrew's monotone chain on (x, y) integer points -> the hull's vertices in order, collinear points dropped."""
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0]) <= 0:
                out.pop()
            out.append(p)
        return out
    lower, upper = half(pts), half(pts[::-1])
    return lower[:-1] + upper[:-1]


def _against_matplotlib(rings_of, n_cases, seed):
    from matplotlib.path import Path
    rng = np.random.default_rng(seed)
    least = 1.0
    for case in range(n_cases):
        H, W = int(rng.integers(8, 25)), int(rng.integers(20, 70))
        xy = rings_of(rng, H, W)
        ring = [(y, x) for x, y in xy]
        mask = PR.poly_mask([ring], H, W)
        rim = PR.boundary_mask([ring], H, W)
        yy, xx = np.mgrid[0:H, 0:W]
        inside = Path(np.array(xy + [xy[0]], dtype=np.float64)).contains_points(np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64))
        inside = inside.reshape(H, W)
        share = 1.0 - rim.sum() / (H * W)
        least = min(least, share)
        assert share >= 0.75, (case, share)                                  # a case may leave out at most a quarter of its pixels
        assert np.array_equal(mask[~rim], inside[~rim]), case
    return least


def test_matplotlib_agrees_off_the_outline_convex():
    def hulls(rng, H, W):
        while True:
            hull = _hull([(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(8)])
            if len(hull) >= 3:
                return hull
    least = _against_matplotlib(hulls, 200, 301)
    print(f"least compared share, convex: {least:.3f}")


def test_matplotlib_agrees_off_the_outline_self_intersecting():
    least = _against_matplotlib(lambda rng, H, W: [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(6)], 200, 302)
    print(f"least compared share, self-intersecting: {least:.3f}")


# ------------------------------------------------------------------------------------------------------ CPU: the host side ---------
def test_polygon_rings_packs_a_mixed_batch():
    polys = [[],                                                             # no ring: the empty mask
             [[1.0, 2.0, 5.0, 2.0, 5.0, 7.0]],
             [[0, 0, 3, 0, 3, 3], [10.5, 11.5, 12.5, 13.5], [7.25, -8.75]]]
    verts, ring_off, img_ring = ops.polygon_rings(polys)
    assert verts.dtype == ring_off.dtype == img_ring.dtype == torch.int32 and not verts.is_cuda
    assert img_ring.tolist() == [0, 0, 1, 4] and ring_off.tolist() == [0, 3, 6, 8, 9]
    # (y, x), rounded half to even and not clipped: 10.5 -> 10, 11.5 -> 12, 12.5 -> 12, 13.5 -> 14, 7.25 -> 7, -8.75 -> -9
    assert verts.tolist() == [[2, 1], [2, 5], [7, 5], [0, 0], [0, 3], [3, 3], [12, 10], [14, 12], [-9, 7]]
    want = PR.pack([PR.coco_rings(entry) for entry in polys])                # the reference's own rounding and packing
    assert all(np.array_equal(got.numpy(), w) for got, w in zip((verts, ring_off, img_ring), want))
    v, ro, ir = ops.polygon_rings([[], []])
    assert tuple(v.shape) == (0, 2) and ro.tolist() == [0] and ir.tolist() == [0, 0, 0]
    v, _, _ = ops.polygon_rings([[[0.5, 1.5, 2.5, 3.5, -0.5, -1.5, 2 ** 31 - 1, -2 ** 31]]])
    assert v.tolist() == [[2, 0], [4, 2], [-2, 0], [-2 ** 31, 2 ** 31 - 1]]


def test_polygon_rings_refusals():
    good = [[0.0, 0.0, 3.0, 0.0, 3.0, 2.0]]
    ops.polygon_rings([good])
    for bad, what in (([good, [[0.0, 1.0, 2.0]]], "image 1, ring 0"), ([[good[0], []]], "image 0, ring 1"),
                      ([[[0.0, "1"]]], "no number"), ([[[0.0, None]]], "no number"), ([[[True, 1.0]]], "no number"),
                      ([[[0.0, float("nan")]]], "not finite"), ([[[float("inf"), 1.0]]], "not finite"),
                      ([[[2.0 ** 31, 1.0]]], "int32"), ([[[0.0, -2.0 ** 31 - 1]]], "int32"), ([[[10 ** 400, 1]]], "float64"),
                      ([[0.0, 1.0]], "image 0"), ([good, {"size": [3, 4], "counts": [12]}], "image 1"), ([good, None], "image 1"),
                      ([good, "polygon"], "image 1")):
        with pytest.raises(ValueError, match=what):
            ops.polygon_rings(bad)
    for bad in (None, 5, {"a": 1}):
        with pytest.raises(ValueError):
            ops.polygon_rings(bad)


def test_poly_bits_argument_checks_on_the_host():
    v, ro, ir = ops.polygon_rings([[[0, 0, 3, 0, 3, 3]]])
    for bad in ((v.long(), ro, ir), (v.reshape(-1), ro, ir), (v, ro.long(), ir), (v, ro[None], ir), (v, ro, ir.float()), (v, ro, ir[:1]),
                (None, ro, ir), (v.tolist(), ro, ir)):
        with pytest.raises(ValueError):
            ops.poly_bits(*bad, (4, 4))
    for size in ((4,), (4, 0), (0, 4), (4, 4, 4), (4.5, 4), (True, 4), (16385, 4), (4, 16385)):
        with pytest.raises(ValueError, match="size"):
            ops.poly_bits(v, ro, ir, size)


def _rec(i, seg, score=None, cat=1):
    r = {"image_id": i, "category_id": cat, "segmentation": seg}
    if score is not None:
        r["score"] = score
    return r


def test_records_with_polygons_refusals():
    poly = [[0.0, 0.0, 3.0, 0.0, 3.0, 2.0]]
    rle = {"size": [3, 4], "counts": [12]}
    meter = T.InstanceAPMeter("cpu", 4)
    gt = [_rec(1, poly), _rec(2, rle)]
    images = [{"id": 1, "height": 3, "width": 4}, {"id": 2, "height": 3, "width": 4}]
    with pytest.raises(ValueError, match="RLE"):
        T.score_coco_records([_rec(2, rle, 0.5)], gt, meter)                  # images=None: as it was
    with pytest.raises(ValueError, match="RLE"):
        T.score_coco_records([_rec(1, poly, 0.5)], [_rec(1, rle)], meter)
    with pytest.raises(ValueError, match="image 1.*missing from `images`"):
        T.score_coco_records([_rec(2, rle, 0.5)], gt, meter, images=images[1:])
    with pytest.raises(ValueError, match="missing from `images`"):
        T.score_coco_records([_rec(2, poly, 0.5)], [_rec(2, rle)], meter, images={1: (3, 4)})
    with pytest.raises(ValueError, match="differs"):
        T.score_coco_records([_rec(1, {"size": [4, 3], "counts": [12]}, 0.5)], gt, meter, images=images)
    for bad in ([{"id": 1}], [5], 7, {1: 3}):
        with pytest.raises(ValueError, match="images"):
            T.score_coco_records([_rec(2, rle, 0.5)], gt, meter, images=bad)
    assert meter.rows == []
    # coco_to_instances keeps its refusal; coco_masks refuses a code of another size before anything is copied
    with pytest.raises(ValueError, match="polygon"):
        ops.coco_to_instances([_rec(1, poly)], "cpu")
    with pytest.raises(ValueError, match="record 1.*size"):
        ops.coco_masks([_rec(1, poly), _rec(2, {"size": [4, 3], "counts": [12]})], (3, 4), "cpu")
    with pytest.raises(ValueError, match="size"):
        ops.coco_masks([_rec(1, poly)], (3,), "cpu")
    with pytest.raises(ValueError, match="image 0, ring 0"):
        ops.coco_masks([_rec(1, [[0.0, 1.0, 2.0]])], (3, 4), "cpu")


def test_the_ctypes_table_binds_the_rasteriser():
    assert hip.SIGNATURES["fs_poly_bits"] == "pppppp" + "iiiii"              # six pointers, B, R, V, Hs, Ws
    assert hip.HOST_ONLY["fs_poly_bits_scratch_ints"] == ("l", "iii") and hip.HOST_ONLY["fs_poly_bits_band_rows"] == ("i", "ii")
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "fovealseg.h")).read()
    assert "long fs_poly_bits_scratch_ints(int B, int Hs, int Ws);" in header and "int fs_poly_bits_band_rows(int Hs, int Ws);" in header
    assert "int fs_poly_bits(const int* verts, const int* ring_off, const int* img_ring, unsigned int* bits, long long* info, int* scratch, " \
           "int B, int R,\n                 int V, int Hs, int Ws, fs_stream_t stream);" in header
    assert "UNPINNED" in header.split("fs_poly_bits_scratch_ints")[0].split("fs_rle_bits(")[-1]
    # rows a band = min(Hs, 64, 4096 / P); scratch = one int per image and band
    assert [hip.query("fs_poly_bits_band_rows", H, W) for H, W in ((1, 1), (5, 31), (1024, 1024), (1000, 96), (100, 16384), (3, 4097), (40, 4097))] \
        == [1, 5, 64, 64, 8, 3, 31]
    assert [hip.query("fs_poly_bits_scratch_ints", B, H, W) for B, H, W in ((1, 1, 1), (3, 130, 97), (64, 1024, 1024), (2, 100, 16384))] \
        == [1, 9, 1024, 26]
    assert [hip.query("fs_poly_bits_scratch_ints", B, H, W) for B, H, W in ((0, 5, 5), (-1, 5, 5), (2, 0, 5), (2, 5, 0), (1, 16385, 4), (1, 4, 16385))] \
        == [0] * 6


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ----
POISON = -0x3C3C3C3D                                    # as a word it is no mask of these tests; as an offset or a vertex it is far outside


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

    def get(self):
        body = self.out.get(complete=False)
        assert bool((body[:self.off] == self.out.fill).all()), "the word in front of a misaligned body was written"
        return body[self.off:]

    def untouched(self):
        return self.out.untouched()


def _inputs(arr, off):
    """An int32 input on the device, `off` words past an aligned address; the tensor is kept whole for the comparison afterwards."""
    flat = np.concatenate([np.full(off, POISON, dtype=np.int32), np.asarray(arr, dtype=np.int32).reshape(-1)])
    whole = torch.from_numpy(flat).cuda()
    return whole, whole.data_ptr() + 4 * off, flat


def _call(tables, B, Hs, Ws, off=0):
    """fs_poly_bits at the C ABI on packed tables; returns (words (B,Hs,P) int32 numpy, info rows) having checked guards and inputs."""
    verts, ring_off, img_ring = tables
    R_, V = len(ring_off) - 1, len(verts)
    P = (Ws + 31) // 32
    vd, vp, vflat = _inputs(verts if V else np.zeros((1, 2), dtype=np.int32), off)
    rd, rp, rflat = _inputs(ring_off, off)
    gd, gp, gflat = _inputs(img_ring, 0)
    bits, info = Buf(B * Hs * P, off=off), Buf(B * 4, torch.int64)
    need = hip.query("fs_poly_bits_scratch_ints", B, Hs, Ws)
    assert need == B * math.ceil(Hs / hip.query("fs_poly_bits_band_rows", Hs, Ws))
    scr = Buf(need, off=off)
    hip.call("fs_poly_bits", vp, rp, gp, bits.ptr, info.ptr, scr.ptr, B, R_, V, Hs, Ws)
    torch.cuda.synchronize()
    scr.get()
    for d, flat in ((vd, vflat), (rd, rflat), (gd, gflat)):
        assert np.array_equal(d.cpu().numpy(), flat)                         # inputs are inputs
    return bits.get().numpy().reshape(B, Hs, P), info.get().reshape(B, 4).tolist()


def _poly(batch, Hs, Ws, off=0, tables=None, tail=3):
    """A batch (images of rings of (y, x)) through fs_poly_bits, held to poly_ref image by image; `tail` vertices of poison lie behind
    the last ring and belong to V.  tables overrides the packed tables (malformed offsets)."""
    verts, ring_off, img_ring = PR.pack(batch) if tables is None else tables
    if tables is None and tail:
        verts = np.concatenate([verts, np.full((tail, 2), POISON, dtype=np.int32)])
    B = len(img_ring) - 1
    words, info = _call((verts, ring_off, img_ring), B, Hs, Ws, off=off)
    for b in range(B):
        mask, want = PR.poly_info(verts, ring_off, img_ring, b, Hs, Ws, fast=Hs * Ws > 1500)
        assert info[b] == want, (b, info[b], want)
        assert np.array_equal(words[b], R.bits(mask)), b                     # the padding bits too: R.bits leaves them 0
        assert np.array_equal(R.unbits(words[b], Ws), mask)
        assert int(np.unpackbits(words[b].view(np.uint8)).sum()) == info[b][1]
    return words, info


def _random_batch(rng, B, Hs, Ws):
    return [[[(int(rng.integers(-2, Hs + 2)), int(rng.integers(-2, Ws + 2))) for _ in range(int(rng.integers(1, 10)))]
             for _ in range(int(rng.integers(0, 5)))] for _ in range(B)]


SHAPES = [(1, 1), (5, 31), (7, 32), (9, 33), (3, 64), (4, 65), (70, 40), (130, 97), (63, 96), (65, 96)]


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("Hs,Ws", SHAPES)
def test_poly_bits_shapes(Hs, Ws, off):
    assert hip.query("fs_poly_bits_band_rows", 1000, 96) == 64               # (63, 96) and (65, 96) sit on either side of a band
    rng = np.random.default_rng(Hs * 1000 + Ws)
    for B in (1, 3):
        batch = _random_batch(rng, B, Hs, Ws)
        if B == 3:
            batch[1] = []                                                    # an image without rings between two with
        _poly(batch, Hs, Ws, off=off)


@pytest.mark.gpu
def test_poly_bits_hand_cases_on_the_device():
    for name in sorted(HAND):
        rings, H, W, rows = HAND[name]
        words, info = _poly([rings], H, W)
        assert np.array_equal(R.unbits(words[0], W), parse(rows)), name
        assert info[0] == [0, int(parse(rows).sum()), len(rings), sum(len(r) for r in rings)], name
    # all of one frame size as one batch, and the ties of the rounding through ops.polygon_rings
    same = [HAND[k][0] for k in ("triangle", "triangle45")]
    words, _ = _poly(same, 6, 8)
    assert np.array_equal(R.unbits(words[1], 8), parse(HAND["triangle45"][3]))
    bits, info = ops.poly_bits(*ops.polygon_rings([[[0.5, 0.5, 2.5, 0.5, 2.5, 1.5, 0.5, 1.5]]]), (4, 5), check=True)
    assert np.array_equal(R.unbits(bits[0].cpu().numpy(), 5), parse(["###..", "###..", "###..", "....."])) and info.tolist() == [[0, 9, 1, 4]]


@pytest.mark.gpu
def test_poly_bits_borders():
    # bands of 64 rows: vertices on the rows 63, 64, 127 and 128, edges across both borders
    _poly([[[(10, 5), (63, 30), (64, 8), (128, 35), (127, 2), (129, 20)]], [[(0, 0), (129, 39)], [(63, 0), (63, 39), (64, 39), (64, 0)]]], 130, 40)
    # horizontal edges across word borders; vertical edges in the columns 31, 32 and Ws - 1
    _poly([[[(2, 20), (2, 75)]], [[(1, 30), (1, 70), (3, 70), (3, 30)]], [[(0, 0), (0, 79)], [(3, 31), (3, 32)], [(1, 63), (1, 64)]]], 4, 80)
    words, _ = _poly([[[(0, 31), (5, 31)]], [[(0, 32), (5, 32)]], [[(0, 64), (5, 64)]], [[(0, 31), (5, 31), (5, 32), (0, 32)]]], 6, 65)
    assert [sorted(set(np.argwhere(R.unbits(w, 65))[:, 1].tolist())) for w in words] == [[31], [32], [64], [31, 32]]
    # the clamp: INT32_MIN and INT32_MAX are vertices like any other -> the triangle (0,0), (8,32), (0,32)
    lo, hi = PR.INT32_MIN, PR.INT32_MAX
    words, _ = _poly([[[(lo, lo), (hi, hi), (lo, hi)]]], 9, 33)
    assert np.array_equal(R.unbits(words[0], 33), PR.poly_mask([[(0, 0), (8, 32), (0, 32)]], 9, 33))


@pytest.mark.gpu
def test_poly_bits_many_edges():
    # more edges than threads: a 1500-vertex zigzag between the top and the bottom row
    zig = [(0 if i % 2 == 0 else 39, i * 199 // 1499) for i in range(1500)]
    _poly([[zig]], 40, 200)
    # one 1024 x 1024 image, a star of 2048 vertices: 16 bands, 8 edges a thread
    star = [(int(round(512 + r * math.sin(2 * math.pi * i / 2048))), int(round(512 + r * math.cos(2 * math.pi * i / 2048))))
            for i in range(2048) for r in ((500, 440)[i % 2],)]
    words, info = _poly([[star]], 1024, 1024)
    assert 440 * 440 * 3 < info[0][1] < 500 * 500 * 4


def _base_tables():
    batch = [[[(1, 1), (1, 20), (7, 20), (7, 1)], [(3, 30), (8, 39), (3, 39)]] for _ in range(5)]
    verts, ring_off, img_ring = PR.pack(batch)
    assert ring_off.tolist() == [0, 4, 7, 11, 14, 18, 21, 25, 28, 32, 35] and img_ring.tolist() == [0, 2, 4, 6, 8, 10]
    return verts, ring_off, img_ring


@pytest.mark.gpu
@pytest.mark.parametrize("which,index,value,statuses", [
    ("ring", 3, 2, [0, 1, 0, 0, 0]),                     # decreasing: ring 2 = [7, 2)
    ("ring", 3, -1, [0, 1, 0, 0, 0]),                    # negative
    ("ring", 3, 40, [0, 1, 0, 0, 0]),                    # beyond V = 35
    ("ring", 10, 36, [0, 0, 0, 0, 1]),                   # the last offset one beyond V
    ("ring", 0, -3, [1, 0, 0, 0, 0]),
    ("img", 2, 13, [0, 1, 1, 0, 0]),                     # beyond R = 10: the image that ends there and the one that begins there
    ("img", 2, -2, [0, 1, 1, 0, 0]),
    ("img", 2, 1, [0, 1, 0, 0, 0]),                      # decreasing: image 1 = rings [2, 1); image 2 = rings [1, 6) is valid
    ("img", 5, POISON, [0, 0, 0, 0, 1]),
    ("img", 0, PR.INT32_MIN, [1, 0, 0, 0, 0]),
])
def test_poly_bits_malformed_offsets(which, index, value, statuses):
    """Malformed offsets are ordinary inputs with defined results: zeros and status 1; the images beside them are what they were, and
    nothing outside the tensors is written (the guard bands, checked in _call)."""
    verts, ring_off, img_ring = _base_tables()
    good, _ = _poly(None, 10, 40, tables=(verts, ring_off, img_ring))
    (ring_off if which == "ring" else img_ring)[index] = value
    words, info = _poly(None, 10, 40, tables=(verts, ring_off, img_ring))
    assert [r[0] for r in info] == statuses
    for b, st in enumerate(statuses):
        if st:
            assert not words[b].any() and info[b] == [1, 0, 0, 0]
        elif not (which, index, value) == ("img", 2, 1) or b != 2:
            assert np.array_equal(words[b], good[b])


@pytest.mark.gpu
def test_rejected_arguments_leave_the_outputs_alone():
    B, Hs, Ws = 2, 9, 65
    verts, ring_off, img_ring = PR.pack([[[(1, 1), (1, 60), (7, 30)]], []])
    vd, rd, gd = (torch.from_numpy(a.reshape(-1)).cuda() for a in (verts, ring_off, img_ring))
    bits, info, scr = Buf(B * Hs * 3), Buf(B * 4, torch.int64), Buf(hip.query("fs_poly_bits_scratch_ints", B, Hs, Ws))

    def rejected(*args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call("fs_poly_bits", *args)

    good = [vd.data_ptr(), rd.data_ptr(), gd.data_ptr(), bits.ptr, info.ptr, scr.ptr]
    for i in range(6):
        a = list(good)
        a[i] = None
        rejected(*a, B, 1, 3, Hs, Ws)
    for dims in ((0, 1, 3, Hs, Ws), (-1, 1, 3, Hs, Ws), (B, -1, 3, Hs, Ws), (B, 1, -1, Hs, Ws), (B, 1, 3, 0, Ws), (B, 1, 3, Hs, 0),
                 (B, 1, 3, -9, Ws), (B, 1, 3, Hs, -1),
                 (B, 1, 3, 16385, Ws), (B, 1, 3, Hs, 16385),               # a side above 16384
                 (B, 1, 3, 65536, 32768),                                    # Hs * Ws = 2^31
                 (16, 1, 3, 16384, 16384)):                                  # 2^32 bit slots
        rejected(*good, *dims)
    torch.cuda.synchronize()
    assert bits.untouched() and info.untouched() and scr.untouched()
    hip.call("fs_poly_bits", *good, B, 1, 3, Hs, Ws)                         # and the same pointers are taken with the sizes they were made for
    torch.cuda.synchronize()
    want = PR.poly_mask([[(1, 1), (1, 60), (7, 30)]], Hs, Ws)
    assert np.array_equal(bits.get().numpy().reshape(B, Hs, 3), np.stack([R.bits(want), R.bits(np.zeros_like(want))]))
    assert info.get().reshape(B, 4).tolist() == [[0, int(want.sum()), 1, 3], [0, 0, 0, 0]]


# ------------------------------------------------------------------------------------------------- GPU: the composed calls ---------
HS, WS = 37, 70


def _coco_polys(rng, n):
    """n images' polygon lists in COCO's form (x, y floats, halves among them), 1 - 3 rings each."""
    out = []
    for _ in range(n):
        out.append([[float(v) for xy in [(rng.integers(-4, 2 * WS + 8) / 2, rng.integers(-4, 2 * HS + 8) / 2) for _ in range(int(rng.integers(3, 9)))]
                     for v in xy] for _ in range(int(rng.integers(1, 4)))])
    return out


def _ref_masks(polys, H, W):
    return np.stack([PR.poly_mask_rows(PR.coco_rings(p), H, W) for p in polys])


@pytest.mark.gpu
def test_ops_poly_bits_and_the_round_trip():
    rng = np.random.default_rng(11)
    polys = _coco_polys(rng, 4) + [[]]
    masks = _ref_masks(polys, HS, WS)
    assert np.array_equal(masks[:2], np.stack([PR.poly_mask(PR.coco_rings(p), HS, WS) for p in polys[:2]]))
    tables = ops.polygon_rings(polys)
    bits, info = ops.poly_bits(*tables, (HS, WS), check=True)
    want = torch.from_numpy(np.stack([R.bits(m) for m in masks])).cuda()
    assert bits.dtype == torch.int32 and torch.equal(bits, want) and torch.equal(bits, ops.mask_bits(torch.from_numpy(masks).cuda()))
    assert info[:, 0].tolist() == [0] * 5 and info[:, 1].tolist() == [int(m.sum()) for m in masks] and info[4].tolist() == [0, 0, 0, 0]
    again, info2 = ops.poly_bits(*(t.cuda() for t in tables), (HS, WS))      # tables on the device are used where they lie
    assert torch.equal(again, bits) and torch.equal(info2, info)             # and two calls give the same bits
    # the record goes through the library's own operations: encode, decode, the same words; the three areas agree
    stats, counts = ops.mask_rle(bits, WS, max_runs=HS * WS + 1)
    back, rinfo = ops.rle_bits(counts, stats, (HS, WS), check=True)
    assert torch.equal(back, bits) and torch.equal(stats[:, 0], info[:, 1]) and torch.equal(rinfo[:, 1], info[:, 1])
    # images without vertices at all
    bits0, info0 = ops.poly_bits(*ops.polygon_rings([[], []]), (HS, WS), check=True)
    assert not bits0.any() and info0.tolist() == [[0, 0, 0, 0]] * 2
    # check=True names the image
    v, ro, ir = tables
    ro = ro.clone()
    ro[1] = 10 ** 6                                                          # image 0's first ring ends far beyond V
    with pytest.raises(ValueError, match="image 0: the image's ring or vertex offsets"):
        ops.poly_bits(v, ro, ir, (HS, WS), check=True)


def _records(polys, masks, kinds, scores=True):
    recs = []
    for i, (p, m, kind) in enumerate(zip(polys, masks, kinds)):
        code = R.encode(m)
        seg = p if kind == "poly" else {"size": [HS, WS], "counts": ops.rle_to_string(code) if kind == "str" else code}
        recs.append(_rec(f"im{i}" if i % 2 else i, seg, score=0.25 + i / 16 if scores else None, cat=i % 5))
    return json.loads(json.dumps(recs))


@pytest.mark.gpu
def test_coco_masks_mixes_the_two_kinds():
    rng = np.random.default_rng(12)
    polys = _coco_polys(rng, 7)
    masks = _ref_masks(polys, HS, WS)
    want = torch.from_numpy(np.stack([R.bits(m) for m in masks])).cuda()
    order = rng.permutation(7).tolist()
    outs = []
    for kinds in (["poly"] * 7, ["rle"] * 7, ["poly", "rle", "str", "poly", "poly", "str", "rle"]):
        recs = _records(polys, masks, kinds)
        recs = [recs[i] for i in order]
        ids, cat, bits, info, scores = ops.coco_masks(recs, (HS, WS), "cuda")
        assert ids == [r["image_id"] for r in recs] and cat.tolist() == [i % 5 for i in order]
        assert torch.equal(bits, want[order]) and info.tolist() == [[0, int(masks[i].sum())] for i in order]
        assert scores.tolist() == [0.25 + i / 16 for i in order]
        outs.append(bits)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert ops.coco_masks(_records(polys, masks, ["poly"] * 7, scores=False), (HS, WS), "cuda")[4] is None


@pytest.mark.gpu
def test_score_coco_records_with_polygon_ground_truth():
    rng = np.random.default_rng(13)
    polys = _coco_polys(rng, 6)
    masks = _ref_masks(polys, HS, WS)
    found = np.roll(masks, 1, 2)                                             # the results: the ground truth moved by a pixel
    found[:, :, 0] = False
    dt = _records(polys, found, ["str", "rle", "str", "rle", "str", "rle"])[:5]          # the last image has no result
    gt_rle = _records(polys, masks, ["rle"] * 6, scores=False)
    gt_poly = _records(polys, masks, ["poly", "poly", "rle", "poly", "str", "poly"], scores=False)
    images = [{"id": r["image_id"], "height": HS, "width": WS, "file_name": "x.jpg"} for r in gt_rle]
    meters = [T.InstanceAPMeter("cuda", 5) for _ in range(4)]
    assert T.score_coco_records(dt, gt_rle, meters[0], chunk=4) == 6         # as before: no images
    assert T.score_coco_records(dt, gt_poly, meters[1], chunk=4, images=images) == 6
    assert T.score_coco_records(dt, gt_poly, meters[2], chunk=4, images={r["image_id"]: (HS, WS) for r in gt_rle}) == 6
    assert T.score_coco_records(dt, gt_rle, meters[3], chunk=4, images=images) == 6
    rows = [torch.cat(m.rows) for m in meters]
    assert all(torch.equal(r, rows[0]) for r in rows[1:]) and len(meters[1].rows) == 2
    res = meters[1].result()
    assert res == meters[0].result() or all(v == res[k] or v != v for k, v in meters[0].result().items())
    assert res["n_images"] == 6 and res["n_records"] == 5 and res["mIoU"] > 0.0
    # polygons on the results' side too
    both = T.InstanceAPMeter("cuda", 5)
    dt_poly = [dict(r, score=0.5) for r in gt_poly]
    assert T.score_coco_records(dt_poly, gt_poly, both, images=images) == 6
    pair = torch.cat(both.rows)[:, 3:9]
    assert torch.equal(pair[:, 0], pair[:, 1]) and torch.equal(pair[:, 0], pair[:, 2]) and pair[:, 0].tolist() == [int(m.sum()) for m in masks]


@pytest.mark.gpu
def test_evaluate_instances_with_a_polygon_label():
    import test_predict as TP
    module, _ = TP._module("hrnet")
    size = 128
    X, Fp, _Y, cls = T.synthetic_batch(2, size, size, seed=11, device="cuda")
    polys = [[[20.5, 30.0, 90.0, 25.5, 100.0, 80.0, 60.5, 110.5, 15.0, 70.0]],
             [[64.0, 10.0, 120.0, 64.0, 64.0, 118.0, 8.0, 64.0], [5.0, 5.0, 30.0, 5.0, 5.0, 30.0]]]
    dense = torch.from_numpy(np.stack([PR.poly_mask_rows(PR.coco_rings(p), size, size) for p in polys])).cuda()
    bits, info = ops.poly_bits(*ops.polygon_rings(polys), (size, size), check=True)
    assert torch.equal(bits, ops.mask_bits(dense)) and int(info[:, 1].min()) > 1000
    stats, counts = ops.mask_rle(bits, size)
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        want = module.evaluate_instances(X, Fp, dense[:, None].float(), cls)
        got = module.evaluate_instances(X, Fp, (counts, stats), cls, seg_size=(size, size))
    finally:
        hip.set_deterministic(was)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert int(want[-1][:, 2].min()) > 1000                                  # the label is not empty
