"""The connected component under the gaze (fs_mask_component, fs_unwarp_instances_component, predict_instances(component=...),
GazeSession(component=...)).  The definition is this library's (unpinned: the reference has no counterpart); it is the textbook one,
so tests/component_ref.py takes the component from scipy.ndimage.label and is itself held to hand-derived answers first.  Every
comparison with the device is bit for bit."""
import numpy as np
import pytest
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg.models import DeformSegmentationModule
from fovealseg.session import GazeSession

import component_ref as C
import rle_ref as RLE
import score_ref as S


def parse(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


def at(py, px, Hs, Ws):
    """The focus whose gaze pixel is (py, px)."""
    return np.array([py / (Hs - 1) if Hs > 1 else 0.0, px / (Ws - 1) if Ws > 1 else 0.0], dtype=np.float32)


def expect(rows, focus, conn, want_rows, want_comp, snap2=C.OFF2):
    got, comp = C.component(parse(rows), focus, conn, snap2)
    assert np.array_equal(got, parse(want_rows)), (rows, focus, conn)
    assert comp == want_comp, (comp, want_comp)


# --------------------------------------------------------------------------------------------------- CPU: the reference by hand ----
def test_reference_two_blobs_and_the_gaze_on_each():
    rows = ["##......",
            "##......",
            "......##",
            "......##"]
    for conn in (4, 8):
        expect(rows, at(0, 0, 4, 8), conn, ["##......", "##......", "........", "........"], [0, 0, 0, 8])
        expect(rows, at(3, 7, 4, 8), conn, ["........", "........", "......##", "......##"], [3, 7, 0, 8])
        # from the background between them: (1, 3) is 2 columns from (1, 1) and 3 from (2, 6) -> the first blob, seed (1, 1), d2 = 4
        expect(rows, at(1, 3, 4, 8), conn, ["##......", "##......", "........", "........"], [1, 1, 4, 8])


def test_reference_blobs_touching_at_a_corner():
    rows = ["##..",
            "##..",
            "..##",
            "..##"]
    expect(rows, at(0, 0, 4, 4), 8, rows, [0, 0, 0, 8])
    expect(rows, at(0, 0, 4, 4), 4, ["##..", "##..", "....", "...."], [0, 0, 0, 8])
    expect(rows, at(3, 3, 4, 4), 4, ["....", "....", "..##", "..##"], [3, 3, 0, 8])


def test_reference_ties_go_to_the_smaller_row_major_index():
    rows = ["..#..",
            ".....",
            "..#.."]
    expect(rows, at(1, 2, 3, 5), 8, ["..#..", ".....", "....."], [0, 2, 1, 2])              # above and below at d2 = 1: the upper one
    rows = [".....",
            ".#.#.",
            "....."]
    expect(rows, at(1, 2, 3, 5), 8, [".....", ".#...", "....."], [1, 1, 1, 2])              # left and right at d2 = 1: the left one
    rows = ["....#",
            ".....",
            "#...."]
    expect(rows, at(1, 2, 3, 5), 4, ["....#", ".....", "....."], [0, 4, 5, 2])              # two diagonals at d2 = 5


def test_reference_a_blob_across_the_word_border():
    row = "." * 28 + "#" * 8 + "..#."                                                       # columns 28 .. 35, and a speck at 38
    assert len(row) == 40
    rows = [row, "." * 40]
    want = ["." * 28 + "#" * 8 + "....", "." * 40]
    for conn in (4, 8):
        expect(rows, at(0, 30, 2, 40), conn, want, [0, 30, 0, 9])
        expect(rows, at(0, 33, 2, 40), conn, want, [0, 33, 0, 9])
        expect(rows, at(1, 39, 2, 40), conn, ["." * 38 + "#.", "." * 40], [0, 38, 2, 9])
    words = C.pack(parse(rows))
    assert words.tolist() == [[0xF0000000, 0x0000004F], [0, 0]]
    out, comp = C.component_words(words, 40, at(0, 30, 2, 40), 4)
    assert out.tolist() == [[0xF0000000, 0x0000000F], [0, 0]] and comp == [0, 30, 0, 9]


def test_reference_garbage_in_the_padding_bits():
    # Ws = 33: word 1 holds pixel 32 in bit 0, the other 31 bits are no pixels.  Row 0 is all set, row 1 has only garbage in word 1.
    words = np.array([[0xFFFFFFFF, 0xFFFFFFFF], [0x00000000, 0xFFFFFFFE]], dtype=np.uint32)
    for conn in (4, 8):
        out, comp = C.component_words(words, 33, at(0, 0, 2, 33), conn)
        assert out.tolist() == [[0xFFFFFFFF, 0x00000001], [0, 0]] and comp == [0, 0, 0, 33]
        out, comp = C.component_words(words, 33, at(1, 32, 2, 33), conn)                    # the gaze on the clear pixel (1, 32) below (0, 32)
        assert out.tolist() == [[0xFFFFFFFF, 0x00000001], [0, 0]] and comp == [0, 32, 1, 33]


def test_reference_single_row_single_column_empty_and_full():
    expect(["#"], np.array([0.3, 0.7], dtype=np.float32), 8, ["#"], [0, 0, 0, 1])
    expect(["."], np.array([0.3, 0.7], dtype=np.float32), 8, ["."], [-1, -1, -1, 0])
    expect(["#.##."], at(0, 4, 1, 5), 4, ["..##."], [0, 3, 1, 3])
    expect(["#.##."], at(0, 1, 1, 5), 8, ["#...."], [0, 0, 1, 3])                           # columns 0 and 2 at d2 = 1: the left one
    col = ["#", ".", "#", "#"]
    expect(col, at(1, 0, 4, 1), 8, ["#", ".", ".", "."], [0, 0, 1, 3])
    expect(col, at(3, 0, 4, 1), 4, [".", ".", "#", "#"], [3, 0, 0, 3])
    empty, full = ["....."] * 3, ["#####"] * 3
    for conn in (4, 8):
        expect(empty, at(1, 1, 3, 5), conn, empty, [-1, -1, -1, 0])
        expect(full, at(1, 1, 3, 5), conn, full, [1, 1, 0, 15])


def test_reference_snap_distance():
    rows = ["...#", "...."]
    f = at(0, 0, 2, 4)                                                                      # the nearest set pixel is 3 columns away
    assert C.snap2_of(3) == 9 and C.snap2_of(2) == 4 and C.snap2_of(2.999) == 8 and C.snap2_of(0) == 0 and C.snap2_of(None) == 2 ** 62
    expect(rows, f, 8, rows, [0, 3, 9, 1], snap2=C.snap2_of(3))                             # exactly at the distance: kept
    expect(rows, f, 8, ["....", "...."], [-1, -1, -1, 1], snap2=C.snap2_of(2))              # one below: rejected
    expect(rows, f, 8, ["....", "...."], [-1, -1, -1, 1], snap2=C.snap2_of(2.999))
    expect(rows, at(0, 3, 2, 4), 8, rows, [0, 3, 0, 1], snap2=0)                            # on the pixel itself any snap holds


def test_reference_focus_nan_and_out_of_range():
    rows = ["#...#",
            ".....",
            "#...#"]
    nan = float("nan")
    for f, corner in (((nan, nan), (0, 0)), ((-0.5, -3.0), (0, 0)), ((1.5, 7.0), (2, 4)), ((nan, 2.0), (0, 4)), ((1.0001, -0.0), (2, 0)),
                      ((float("inf"), float("-inf")), (2, 0))):
        want = np.zeros((3, 5), dtype=bool)
        want[corner] = True
        got, comp = C.component(parse(rows), np.array(f, dtype=np.float32), 8)
        assert np.array_equal(got, want) and comp == [corner[0], corner[1], 0, 4], f
    # the gaze pixel rounds to the nearest pixel: 1/16-pixel units, then (g + 8) >> 4
    assert C.gaze_pixel(np.array([0.5, 0.5], dtype=np.float32), 4, 6) == (2, 3)             # 1.5 -> 24/16 -> (24 + 8) >> 4 = 2; 2.5 -> 40 -> 3
    assert C.gaze_pixel(np.array([0.47, 0.47], dtype=np.float32), 4, 6) == (1, 2)           # 22.56 -> 23 -> 31 >> 4 = 1; 37.6 -> 38 -> 46 >> 4 = 2
    assert C.gaze_pixel(np.array([0.49, 0.49], dtype=np.float32), 4, 6) == (2, 2)           # 23.52 -> 24 -> 2: half a sixteenth below 1.5 rounds up


# ----------------------------------------------------------------------------------------------------------- CPU: host checks ----
class _Stub:
    training = False


def test_argument_checks_on_the_host():
    mask = torch.zeros(1, 4, 4, dtype=torch.bool)
    focus = torch.zeros(1, 2)
    for kw in (dict(connectivity=3), dict(connectivity=True), dict(connectivity=None), dict(snap_px=-1), dict(snap_px=float("nan")),
               dict(snap_px=float("inf"))):
        with pytest.raises(ValueError):
            ops.mask_component(mask, focus, **kw)
    assert fovealseg.masks._component_args(8, 1e200) == (8, 2 ** 62) and fovealseg.masks._component_args(8, 2.0 ** 31) == (8, 2 ** 62)      # finite, however large: no limit
    assert fovealseg.masks._component_args(8, None) == (8, 2 ** 62) and fovealseg.masks._component_args(4, 2.999) == (4, 8) and fovealseg.masks._component_args(4, 0) == (4, 0)
    cls, m, grid = torch.zeros(1, 3), torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, 2)
    for kw in (dict(component=3, focus=focus), dict(component=8, focus=focus, snap_px=-1), dict(snap_px=2.0), dict(focus=focus),
               dict(component=8), dict(component=8, focus=torch.zeros(2, 2))):
        with pytest.raises(ValueError):
            ops.unwarp_instances(cls, m, grid, 4, 4, **kw)
    img = torch.zeros(1, 3, 4, 4)
    for kw in (dict(component=3), dict(component=8, snap_px=-1), dict(snap_px=2.0)):
        with pytest.raises(ValueError):
            DeformSegmentationModule.predict_instances(_Stub(), img, focus, **kw)
        with pytest.raises(ValueError):
            GazeSession(_Stub(), 1, (64, 64), **kw)
    s = GazeSession(_Stub(), 1, (64, 64), component=4, snap_px=2.5)
    assert (s.component, s.snap_px) == (4, 2.5) and GazeSession(_Stub(), 1, (64, 64)).component is None


def test_the_ctypes_table_binds_the_component_symbols():
    assert hip.SIGNATURES["fs_mask_component"] == "p" * 5 + "iiii" + "l"
    assert hip.SIGNATURES["fs_unwarp_instances_component"] == "p" * 12 + "i" * 8 + "l"
    for name in ("fs_mask_component_scratch_ints", "fs_mask_component_route", "fs_unwarp_instances_component_scratch_ints"):
        assert name in hip.HOST_ONLY
    assert callable(ops.mask_component)


def test_scratch_queries_are_positive_and_monotone():
    for Hs, Ws in ((1, 1), (64, 64), (1024, 1024), (1300, 1024)):
        n = [hip.query("fs_mask_component_scratch_ints", B, Hs, Ws) for B in (1, 2, 3, 64)]
        assert n[0] > 0 and n == sorted(n) and len(set(n)) == 4
        n = [hip.query("fs_unwarp_instances_component_scratch_ints", B, 8, 8, Hs, Ws) for B in (1, 2, 3, 64)]
        assert n[0] > 0 and n == sorted(n) and len(set(n)) == 4
        assert n[0] >= hip.query("fs_unwarp_instances_scored_scratch_ints", 1, 8, 8, Hs, Ws) + hip.query("fs_mask_component_scratch_ints", 1, Hs, Ws)
    assert hip.query("fs_mask_component_scratch_ints", 0, 8, 8) == 0 and hip.query("fs_mask_component_scratch_ints", 1, 16385, 8) == 0
    assert hip.query("fs_mask_component_route", 1, 64, 64) == 1 and hip.query("fs_mask_component_route", 64, 1024, 1024) == 1
    assert hip.query("fs_mask_component_route", 1, 1300, 1024) == 2 and hip.query("fs_mask_component_route", 1, 8, 16385) == 0
    assert hip.query("fs_mask_component_route", 1, 65536, 32768) == 0 and hip.query("fs_mask_component_route", 1, 0, 8) == 0


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ----
FILL = 0x3C3C3C3D


def _kt():
    import kernel_testing as KT
    return KT


def _tp():
    import test_predict as TP
    return TP


def _component(words, focus, Ws, conn, snap2=C.OFF2, off=0):
    """fs_mask_component at the C ABI.  words (B,Hs,P) uint32 and focus (B,2) fp32 on the host -> (out (B,Hs,P) uint32, comp (B,4)) on
    the host; every output written, guard bands of outputs and scratch intact.  off: ints the scratch is moved from 16-byte alignment."""
    KT = _kt()
    B, Hs, P = words.shape
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    f = torch.from_numpy(np.asarray(focus, dtype=np.float32)).cuda()
    out, comp = KT.Out(B * Hs * P, torch.int32, fill=FILL), KT.Out(B * 4, torch.int64)
    n = hip.query("fs_mask_component_scratch_ints", B, Hs, Ws)
    scr = KT.Out(n + off, torch.int32)
    hip.call("fs_mask_component", bits.data_ptr(), f.data_ptr(), out.ptr, comp.ptr, scr.ptr + 4 * off, B, Hs, Ws, conn, snap2)
    body = scr.get(complete=False)
    assert bool((body[:off] == scr.fill).all())
    assert torch.equal(bits.cpu(), torch.from_numpy(words.view(np.int32)))                  # the input is not written
    return out.get().numpy().view(np.uint32).reshape(B, Hs, P), comp.get().view(B, 4)


def _check(masks, focus, conn, snap2=C.OFF2, off=0, garbage=True):
    """The device against the reference, bit for bit; with garbage, the padding bits of the input are all set."""
    masks = np.asarray(masks)
    B, Hs, Ws = masks.shape
    words = np.stack([C.pack(m) for m in masks])
    if garbage and Ws & 31:
        words[:, :, -1] |= np.uint32((0xFFFFFFFF << (Ws & 31)) & 0xFFFFFFFF)
    want, wcomp = C.component_batch(masks, focus, conn, snap2)
    out, comp = _component(words, focus, Ws, conn, snap2, off)
    assert torch.equal(comp, torch.from_numpy(wcomp)), (comp.tolist(), wcomp.tolist())
    assert torch.equal(torch.from_numpy(out.view(np.int32)), torch.from_numpy(np.stack([C.pack(w) for w in want]).view(np.int32)))
    return want, wcomp


def _blobs(rng, Hs, Ws, density):
    return rng.random((Hs, Ws)) < density


def _pick(mask, want, rng):
    """The focus of a pixel of `mask` whose value is `want`, a seeded choice; the middle pixel where there is none."""
    ys, xs = np.nonzero(mask == want)
    Hs, Ws = mask.shape
    if len(ys) == 0:
        return at(Hs // 2, Ws // 2, Hs, Ws)
    i = int(rng.integers(len(ys)))
    return at(int(ys[i]), int(xs[i]), Hs, Ws)


SHAPES = [(1, 1), (1, 70), (9, 7), (8, 32), (8, 33), (37, 300), (64, 64), (50, 513), (96, 1500)]


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("Hs,Ws", SHAPES)
def test_mask_component_seeded_blobs(Hs, Ws, conn):
    """B = 3, a density per image: 0.3 (many small components), 0.5, 0.6 (one that percolates at 8); two calls, the gazes on a blob,
    on background and on the four corners, the densities rotated between the calls."""
    rng = np.random.default_rng(Hs * 10007 + Ws * 13 + conn)
    dens = (0.3, 0.5, 0.6)
    for call in range(2):
        masks = np.stack([_blobs(rng, Hs, Ws, dens[(b + call) % 3]) for b in range(3)])
        if call == 0:
            focus = np.stack([_pick(masks[0], True, rng), _pick(masks[1], False, rng), at(0, 0, Hs, Ws)])
        else:
            focus = np.stack([at(0, Ws - 1, Hs, Ws), at(Hs - 1, 0, Hs, Ws), at(Hs - 1, Ws - 1, Hs, Ws)])
        want, comp = _check(masks, focus, conn)
        print(f"{Hs}x{Ws} conn {conn} call {call}: comp {comp.tolist()}, component areas {[int(w.sum()) for w in want]}")


def spiral(Hs, Ws):
    """A one-pixel-wide rectangular spiral with 2-pixel pitch from (0, 0) inwards; returns (mask, its inner end)."""
    m = np.zeros((Hs, Ws), dtype=bool)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = d = 0
    m[0, 0] = True

    def free(yy, xx):
        return not (0 <= yy < Hs and 0 <= xx < Ws) or not m[yy, xx]

    while True:
        for _ in range(2):
            dy, dx = dirs[d]
            ny, nx = y + dy, x + dx
            if 0 <= ny < Hs and 0 <= nx < Ws and not m[ny, nx] and free(ny + dy, nx + dx):
                break
            d = (d + 1) % 4
        else:
            return m, (y, x)
        y, x = ny, nx
        m[y, x] = True


def test_the_spiral_is_one_thin_path():
    m, end = spiral(64, 96)
    for structure in (C.CROSS, C.FULL):
        assert C.ndimage.label(m, structure=structure)[1] == 1
    assert m[0].all() and m[:, 95].all() and m[63].all() and m[2:, 0].all() and not m[1, :95].any() and m[2, 1] and not m[3:63, 1].any()
    assert 1000 < int(m.sum()) < 64 * 96 // 2 + 200 and m[end] and 20 < end[0] < 44 and 20 < end[1] < 76


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [4, 8])
def test_mask_component_structured_masks(conn):
    Hs, Ws = 64, 96
    sp, end = spiral(Hs, Ws)
    comb = np.zeros((Hs, Ws), dtype=bool)
    comb[:, ::2] = True                                                                     # teeth in every other column ...
    comb[-1, :] = True                                                                      # ... joined by the last row alone
    yy, xx = np.mgrid[:Hs, :Ws]
    checker = (yy + xx) % 2 == 0
    frame = np.zeros((Hs, Ws), dtype=bool)
    frame[0], frame[-1], frame[:, 0], frame[:, -1] = True, True, True, True
    frame[20:30, 40:50] = True                                                              # a blob inside that the ring does not touch
    masks = np.stack([sp, comb, checker, frame])
    focus = np.stack([at(*end, Hs, Ws), at(0, 0, Hs, Ws), at(0, 0, Hs, Ws), at(0, 0, Hs, Ws)])
    want, comp = _check(masks, focus, conn)
    assert np.array_equal(want[0], sp) and np.array_equal(want[1], comb) and comp[0].tolist() == [end[0], end[1], 0, int(sp.sum())]
    assert int(want[2].sum()) == (Hs * Ws // 2 if conn == 8 else 1)                         # the checkerboard: one component at 8, single pixels at 4
    assert int(want[3].sum()) == 2 * Hs + 2 * Ws - 4
    # the gaze on the spiral's outer end, and between the comb's teeth (the nearest tooth is the one to the left)
    focus = np.stack([at(0, 0, Hs, Ws), at(10, 5, Hs, Ws), at(5, 5, Hs, Ws), at(25, 45, Hs, Ws)])
    want, comp = _check(masks, focus, conn)
    assert comp[1].tolist() == [10, 4, 1, int(comb.sum())] and int(want[3].sum()) == 100


@pytest.mark.gpu
def test_mask_component_beyond_the_lds_budget():
    """1300 x 1024: the reached set lives in the output words in global memory; three discs and a spiral arm."""
    Hs, Ws = 1300, 1024
    assert hip.query("fs_mask_component_route", 1, Hs, Ws) == 2 and hip.query("fs_mask_component_route", 1, 64, 64) == 1
    yy, xx = np.mgrid[:Hs, :Ws]
    mask = np.zeros((Hs, Ws), dtype=bool)
    for cy, cx, r in ((200, 200, 150), (650, 700, 250), (1150, 300, 120)):
        mask |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    t = np.linspace(0, 5 * np.pi, 4000)                                                     # an arm winding out of the middle disc, 5 pixels wide
    ay, ax = 650 + (250 + 18 * t) * np.sin(t) * 0.9, 700 + (250 + 18 * t) * np.cos(t) * 0.55
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ok = (ay + dy >= 0) & (ay + dy < Hs) & (ax + dx >= 0) & (ax + dx < Ws)
            mask[(ay + dy).astype(int)[ok], (ax + dx).astype(int)[ok]] = True
    for conn, focus in ((8, at(650, 700, Hs, Ws)), (4, at(200, 200, Hs, Ws))):
        want, comp = _check(mask[None], focus[None], conn)
        print(f"1300x1024 conn {conn}: comp {comp.tolist()}, component area {int(want.sum())}")
        assert 0 < int(want.sum()) < int(mask.sum())


@pytest.mark.gpu
def test_mask_component_lds_route_above_the_default_in_growing_sizes():
    """The LDS route beyond what a kernel may use without opting in, smaller sizes first: 512 x 1024 (66 KiB), 1024 x 1024 (132 KiB),
    then 1024 x 1216, whose 1024 x 39 words are the 156 KiB budget exactly; one row more takes the global route.  The opt-in is a
    per-process attribute of the kernel, so a later, larger image must not depend on what came before it.  Both connectivities."""
    assert hip.query("fs_mask_component_route", 1, 1024, 1216) == 1 and hip.query("fs_mask_component_route", 1, 1025, 1216) == 2
    for Hs, Ws in ((512, 1024), (1024, 1024), (1024, 1216)):
        assert hip.query("fs_mask_component_route", 2, Hs, Ws) == 1
        assert Hs * (((Ws + 31) // 32) | 1) * 4 > 64 * 1024
        yy, xx = np.mgrid[:Hs, :Ws]
        disc = (yy - Hs // 2) ** 2 + (xx - Ws // 2) ** 2 <= (Hs // 3) ** 2
        ring = np.zeros((Hs, Ws), dtype=bool)
        ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True                 # the last row and column of R in LDS
        ring[Hs - 2, ::2] = True
        masks = np.stack([disc | ring, disc | ring])
        focus = np.stack([at(Hs // 2, Ws // 2, Hs, Ws), at(Hs - 1, Ws - 1, Hs, Ws)])
        for conn in (8, 4):
            want, comp = _check(masks, focus, conn)
            assert np.array_equal(want[0], disc) and np.array_equal(want[1], ring) and comp[0, 2] == 0 and comp[1, 2] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("off", [1, 2])
def test_mask_component_scratch_off_16_bytes(off):
    rng = np.random.default_rng(77 + off)
    for Hs, Ws in ((37, 300), (9, 7)):
        masks = np.stack([_blobs(rng, Hs, Ws, d) for d in (0.3, 0.5, 0.6)])
        focus = rng.random((3, 2)).astype(np.float32)
        for conn in (4, 8):
            _check(masks, focus, conn, off=off)


@pytest.mark.gpu
def test_mask_component_snap_empty_and_odd_gazes():
    rng = np.random.default_rng(5)
    Hs, Ws = 37, 300
    lone = np.zeros((Hs, Ws), dtype=bool)
    lone[10, 100:104] = True
    masks = np.stack([lone, lone, np.zeros((Hs, Ws), dtype=bool), np.ones((Hs, Ws), dtype=bool)])
    focus = np.stack([at(10, 97, Hs, Ws)] * 2 + [at(3, 3, Hs, Ws)] * 2)                     # 3 columns left of the run
    want, comp = _check(masks, focus, 8, snap2=C.snap2_of(3))
    assert comp.tolist() == [[10, 100, 9, 4], [10, 100, 9, 4], [-1, -1, -1, 0], [3, 3, 0, Hs * Ws]]
    want, comp = _check(masks, focus, 8, snap2=C.snap2_of(2))
    assert comp.tolist() == [[-1, -1, -1, 4], [-1, -1, -1, 4], [-1, -1, -1, 0], [3, 3, 0, Hs * Ws]] and not want[:3].any()
    nan = float("nan")
    blobs = np.stack([_blobs(rng, Hs, Ws, 0.5) for _ in range(4)])
    _check(blobs, np.array([[nan, nan], [-0.5, 2.0], [1.5, -1.0], [nan, 0.5]], dtype=np.float32), 4)
    # the op: a bool mask, bit words, one image without a batch axis
    t = torch.from_numpy(blobs).cuda()
    f = torch.from_numpy(rng.random((4, 2)).astype(np.float32)).cuda()
    want, wcomp = C.component_batch(blobs, f.cpu().numpy(), 8, C.snap2_of(1.5))
    bc, comp = ops.mask_component(t, f, snap_px=1.5)
    assert bc.dtype == torch.int32 and torch.equal(comp.cpu(), torch.from_numpy(wcomp))
    assert np.array_equal(bc.cpu().numpy().view(np.uint32), np.stack([C.pack(w) for w in want]))
    b2, c2 = ops.mask_component(ops.mask_bits(t), f, Ws=Ws, connectivity=8, snap_px=1.5)
    assert torch.equal(b2, bc) and torch.equal(c2, comp)
    b1, c1 = ops.mask_component(t[0].to(torch.uint8), f[:1], connectivity=4)
    w1, r1 = C.component(blobs[0], f[0].cpu().numpy(), 4)
    assert np.array_equal(b1[0].cpu().numpy().view(np.uint32), C.pack(w1)) and c1[0].tolist() == r1
    stats, counts = ops.mask_rle(bc, Ws)
    assert stats[:, 0].tolist() == [int(w.sum()) for w in want]


@pytest.mark.gpu
def test_mask_component_rejects_bad_arguments():
    KT = _kt()
    B, Hs, Ws = 1, 8, 40
    bits = KT.Out(B * Hs * 2, torch.int32)
    out, comp, scr = KT.Out(B * Hs * 2, torch.int32), KT.Out(B * 4, torch.int64), KT.Out(64, torch.int32)
    f = torch.zeros(B, 2, device="cuda")
    good = [bits.ptr, f.data_ptr(), out.ptr, comp.ptr, scr.ptr]

    def rejected(*args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call("fs_mask_component", *args)

    for i in range(5):
        a = list(good)
        a[i] = None
        rejected(*a, B, Hs, Ws, 8, 0)
    rejected(bits.ptr, f.data_ptr(), bits.ptr, comp.ptr, scr.ptr, B, Hs, Ws, 8, 0)          # out == bits
    for conn in (0, 3, 6, 9, -4):
        rejected(*good, B, Hs, Ws, conn, 0)
    rejected(*good, B, Hs, Ws, 8, -1)
    for dims in ((0, Hs, Ws), (B, 0, Ws), (B, Hs, 0), (-1, Hs, Ws), (B, 16385, 1), (B, 1, 16385), (B, 2 ** 16, 2 ** 15)):
        rejected(*good, *dims, 8, 0)
    for t in (bits, out, comp, scr):
        assert t.untouched()


# ------------------------------------------------------------------------------------------------- GPU: the composed call ---------
def _i32(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _restricted_qsum(cls, m, grid, Hs, Ws, comp_masks):
    """score_ref.pixel_reference's unfused route with the sum restricted to the given pixels: (mask (B,Hs,Ws) bool of the whole
    foreground, qsum (B,) int64 over comp_masks, points inside the rounding band among the foreground's)."""
    B, K = cls.shape
    masks, qsum, close = [], [], 0
    for b in range(B):
        full = ops.unwarp_nearest(ops.PredAssemble.apply(cls[b:b + 1], m[b:b + 1]), grid[b:b + 1], Hs, Ws)[0][0]      # (K,Hs,Ws)
        mask = full.argmax(0) != K - 1
        q, x = S.q_from_v(full.permute(1, 2, 0)[mask])
        close += S.in_band(torch.unique(x[~torch.isnan(x)]), K)
        qmap = torch.zeros(Hs, Ws, dtype=torch.int64, device=full.device)
        qmap[mask] = q.to(torch.int64)
        sel = torch.from_numpy(comp_masks[b]).to(full.device)
        assert bool((mask | ~sel).all())                                                   # the component lies inside the foreground
        masks.append(mask)
        qsum.append(qmap[sel].sum())
    return torch.stack(masks), torch.stack(qsum), close


def _check_composed(cls, m, grid, focus, Hs, Ws, conn, snap_px=None):
    """ops.unwarp_instances(component=conn) against the unfiltered call, the reference component of its bits, ops.mask_rle of that,
    the restricted q sum of the unfused route and the fp64 confidence."""
    plain = ops.unwarp_instances(cls, m, grid, Hs, Ws, return_bits=True, score=True)
    got = ops.unwarp_instances(cls, m, grid, Hs, Ws, return_bits=True, score=True, component=conn, focus=focus, snap_px=snap_px)
    assert len(plain) == 6 and len(got) == 7
    cat, stats, counts, bits, conf, qsum, comp = got
    raw = plain[3].cpu().numpy().view(np.uint32)
    B = raw.shape[0]
    whole = np.stack([C.unpack(w, Ws) for w in raw])
    want, wcomp = C.component_batch(whole, focus.cpu().numpy(), conn, C.snap2_of(snap_px))
    assert torch.equal(comp.cpu(), torch.from_numpy(wcomp))
    wbits = torch.from_numpy(np.stack([C.pack(w) for w in want]).view(np.int32)).cuda()
    assert torch.equal(bits, wbits)
    rs, rc = ops.mask_rle(wbits, Ws)
    assert torch.equal(stats, rs) and torch.equal(counts, rc)
    assert torch.equal(cat, plain[0]) and torch.equal(_i32(conf[:, 1].contiguous()), _i32(plain[4][:, 1].contiguous()))
    mask, wq, close = _restricted_qsum(cls, m, grid, Hs, Ws, want)
    assert close == 0, "the seeded input has a point inside the rounding band: pick another seed"
    assert np.array_equal(mask.cpu().numpy(), whole)
    assert torch.equal(qsum, wq)
    ref = S.conf_ref(cls.cpu(), cat.cpu(), qsum.cpu(), stats[:, 0].cpu())
    u = S.ulps32(conf.cpu(), ref)
    print(f"{Hs}x{Ws} conn {conn}: comp {comp.tolist()}, areas {stats[:, 0].tolist()} of {plain[1][:, 0].tolist()}, worst {float(u.max()):.3f} fp32 ulp")
    assert bool((u <= 1.0).all())
    none = torch.from_numpy(wcomp[:, 0] < 0)
    if bool(none.any()):                                                                    # no component: the empty mask's record
        assert stats[none.cuda()].tolist() == [[0, 0, 0, 0, 0, 1]] * int(none.sum())
        assert bool((counts[none.cuda(), 0] == Hs * Ws).all()) and bool((conf[none.cuda()][:, [0, 2]] == 0).all()) and bool((qsum[none.cuda()] == 0).all())
    # the narrower results are the same tensors
    three = ops.unwarp_instances(cls, m, grid, Hs, Ws, component=conn, focus=focus, snap_px=snap_px)
    assert len(three) == 4 and all(torch.equal(a, b) for a, b in zip(three, (cat, stats, counts, comp)))
    five = ops.unwarp_instances(cls, m, grid, Hs, Ws, score=True, component=conn, focus=focus, snap_px=snap_px)
    assert len(five) == 6 and all(torch.equal(_i32(a), _i32(b)) for a, b in zip(five, (cat, stats, counts, conf, qsum, comp)))
    return got, plain, want


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("Hs,Ws,K", [(200, 180, 6), (37, 300, 4), (9, 7, 3)])
def test_unwarp_instances_component(Hs, Ws, K, conn):
    cls, m, grid = _tp()._inputs(3, K, 9, 11, Hs * 1000 + Ws)
    rng = np.random.default_rng(Hs + Ws)
    focus = torch.from_numpy(rng.random((3, 2)).astype(np.float32)).cuda()
    m[2] = 1.0                                                                              # image 2: the background plane wins everywhere
    got, plain, want = _check_composed(cls, m, grid, focus, Hs, Ws, conn)
    assert int(plain[1][2, 0]) == 0 and got[6][2].tolist() == [-1, -1, -1, 0]
    assert bool((got[1][:2, 0] > 0).all()) and bool((got[1][:2, 0] <= plain[1][:2, 0]).all())
    _check_composed(cls, m, grid, focus, Hs, Ws, conn, snap_px=0)                           # a snap that rejects unless the gaze is on the mask


def _composed_abi(cls, m, grid, focus, Hs, Ws, cap, conn, snap2, score=True, with_bits=True):
    """fs_unwarp_instances_component at the C ABI -> dict of host tensors; outputs complete, guard bands of outputs and scratch intact."""
    KT = _kt()
    B, K = cls.shape
    _, h, w, _ = grid.shape
    P = (Ws + 31) // 32
    o = {"cat": KT.Out(B, torch.int64), "stats": KT.Out(B * 6, torch.int64), "counts": KT.Out(B * cap, torch.int32), "comp": KT.Out(B * 4, torch.int64)}
    if with_bits:
        o["bits"] = KT.Out(B * Hs * P, torch.int32, fill=FILL)
    if score:
        o["conf"], o["qsum"] = KT.Out(B * 3, torch.float32, fill=777.5), KT.Out(B, torch.int64)
    scr = KT.Out(hip.query("fs_unwarp_instances_component_scratch_ints", B, h, w, Hs, Ws), torch.int32)
    hip.call("fs_unwarp_instances_component", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), focus.data_ptr(), o["cat"].ptr, o["stats"].ptr,
             o["counts"].ptr, o["bits"].ptr if with_bits else None, o["comp"].ptr, o["conf"].ptr if score else None,
             o["qsum"].ptr if score else None, scr.ptr, B, K, h, w, Hs, Ws, cap, conn, snap2)
    scr.get(complete=False)                              # the bands around the queried ints
    out = {k: t.get() for k, t in o.items()}
    shapes = {"stats": (B, 6), "counts": (B, cap), "comp": (B, 4), "bits": (B, Hs, P), "conf": (B, 3)}
    return {k: v.view(*shapes[k]) if k in shapes else v for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 4), (9, 7, 3), (200, 180, 6)])
def test_unwarp_instances_component_at_the_c_abi(Hs, Ws, K, conn):
    """The composed entry point between guard bands -- its scratch regions are the last of the plan -- with and without the score
    and the caller's bit words, against the op (itself held to the references above)."""
    cls, m, grid = _tp()._inputs(3, K, 9, 11, Hs * 1000 + Ws)
    focus = torch.from_numpy(np.random.default_rng(Hs + Ws).random((3, 2)).astype(np.float32)).cuda()
    m[2] = 1.0
    for snap_px in (None, 0):
        want = ops.unwarp_instances(cls, m, grid, Hs, Ws, return_bits=True, score=True, component=conn, focus=focus, snap_px=snap_px)
        want = dict(zip(("cat", "stats", "counts", "bits", "conf", "qsum", "comp"), (t.cpu() for t in want)))
        cap = want["counts"].shape[1]
        for score in (True, False):
            for with_bits in (True, False):
                got = _composed_abi(cls, m, grid, focus, Hs, Ws, cap, conn, C.snap2_of(snap_px), score, with_bits)
                assert set(got) == {"cat", "stats", "counts", "comp"} | ({"bits"} if with_bits else set()) | ({"conf", "qsum"} if score else set())
                for k, v in got.items():
                    assert torch.equal(_i32(v), _i32(want[k])), (k, score, with_bits)


@pytest.mark.gpu
def test_unwarp_instances_component_rejects_bad_arguments():
    KT = _kt()
    B, K, h, w, Hs, Ws, cap = 1, 4, 4, 4, 8, 8, 20
    cls, m, grid = _tp()._inputs(B, K, h, w, 0)
    focus = torch.zeros(B, 2, device="cuda")
    n = max(hip.query("fs_unwarp_instances_component_scratch_ints", B, h, w, Hs, Ws),
            hip.query("fs_unwarp_instances_component_scratch_ints", B, h, w, 1, 16384))
    # cat, stats, counts, bits, comp, conf, qsum, scratch
    outs = [KT.Out(B, torch.int64), KT.Out(B * 6, torch.int64), KT.Out(B * cap, torch.int32), KT.Out(B * 513, torch.int32), KT.Out(B * 4, torch.int64),
            KT.Out(B * 3), KT.Out(B, torch.int64), KT.Out(n, torch.int32)]
    head = [cls.data_ptr(), m.data_ptr(), grid.data_ptr(), focus.data_ptr()]
    ptrs = [t.ptr for t in outs]
    dims = (B, K, h, w, Hs, Ws, cap)

    def rejected(*args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call("fs_unwarp_instances_component", *args)

    for i in range(4):                                                                      # cls, m, grid, focus
        a = list(head)
        a[i] = None
        rejected(*a, *ptrs, *dims, 8, 0)
    for i in (0, 1, 2, 4, 5, 6, 7):                                                         # bits (3) alone may be null; conf without qsum and qsum without conf
        a = list(ptrs)
        a[i] = None
        rejected(*head, *a, *dims, 8, 0)
    for conn in (0, 3, 6, 9, -8):
        rejected(*head, *ptrs, *dims, conn, 0)
    rejected(*head, *ptrs, *dims, 8, -1)
    rejected(*head, *ptrs, B, K, h, w, Hs, Ws, 0, 8, 0)                                     # cap
    rejected(*head, *ptrs, B, 1, h, w, Hs, Ws, cap, 8, 0)                                   # K
    for hs, ws in ((0, Ws), (Hs, 0), (1, 16385), (16385, 1)):
        rejected(*head, *ptrs, B, K, h, w, hs, ws, cap, 8, 0)
    rejected(*head, *ptrs, 0, K, h, w, Hs, Ws, cap, 8, 0)
    for t in outs:                                                                          # nothing was launched
        assert t.untouched()
    hip.call("fs_unwarp_instances_component", *head, *ptrs, *dims, 8, 0)                    # the same buffers are accepted as they are
    assert not outs[0].untouched() and not outs[4].untouched()


@pytest.mark.gpu
def test_unwarp_instances_component_repeats_bit_for_bit_in_every_mode():
    cls, m, grid = _tp()._inputs(2, 6, 9, 11, 37300)
    focus = torch.tensor([[0.3, 0.6], [0.8, 0.1]], device="cuda")
    mode0, det0 = hip.get_conv_precision(), hip.get_deterministic()
    runs = []
    try:
        for mode in ("f32", "bf16x3", "f16x2"):
            for det in (True, False):
                hip.set_conv_precision(mode)
                hip.set_deterministic(det)
                for _ in range(2):
                    runs.append(ops.unwarp_instances(cls, m, grid, 37, 300, return_bits=True, score=True, component=8, focus=focus))
    finally:
        hip.set_conv_precision(mode0)
        hip.set_deterministic(det0)
    assert len(runs) == 12
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(_i32(a), _i32(b))


@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [None, (200, 180)])
def test_predict_instances_component(seg, deterministic):
    TP = _tp()
    module, _ = TP._module("hrnet")
    X, Fp = TP._batch(2, 256, 11)
    bias = module.decoder.cls_net.fc.bias            # test_instances.py: a large background logit lets the mask plane decide where m > 0
    keep = bias.detach().clone()
    with torch.no_grad():
        bias[-1] += 1000.0
    try:
        state = {k: v.detach().clone() for k, v in module.state_dict().items()}
        X0, F0 = X.clone(), Fp.clone()
        before = module.predict_instances(X, Fp, seg, return_bits=True, return_score=True)
        got = module.predict_instances(X, Fp, seg, return_bits=True, return_score=True, component=8)
        again = module.predict_instances(X, Fp, seg, return_bits=True, return_score=True, component=8)
        four = module.predict_instances(X, Fp, seg, component=4, snap_px=3)
        H, W = seg or (256, 256)
        wide = module.predict_instances(X, Fp, seg, return_score=True, component=8, max_runs=H * W + 1)    # no code is longer than that
        after = module.predict_instances(X, Fp, seg, return_bits=True, return_score=True, component=None)
        module.check_nan()
        assert torch.equal(X, X0) and torch.equal(Fp, F0)
        for k, v in module.state_dict().items():
            assert torch.equal(v, state[k]), k
        with torch.no_grad():
            cls, mm, grid, _ = module._head_parts(X, Fp, (H, W), "test")
            (cat, stats, counts, bits, conf, qsum, comp), plain, want = _check_composed(cls, mm, grid, Fp, H, W, 8)
            by4 = ops.unwarp_instances(cls, mm, grid, H, W, component=4, focus=Fp, snap_px=3)
    finally:
        with torch.no_grad():
            bias.copy_(keep)
    assert len(got) == 6 and len(before) == 5 and len(after) == 5 and len(four) == 4
    for a, b in zip(before, after):                                                        # component=None: the parent's tuple
        assert torch.equal(_i32(a), _i32(b))
    for a, b in zip(before, plain[:5]):
        assert torch.equal(_i32(a), _i32(b))
    for a, b in zip(got, (cat, stats, counts, bits, conf, comp)):
        assert torch.equal(_i32(a), _i32(b))
    for a, b in zip(got, again):
        assert torch.equal(_i32(a), _i32(b))
    for a, b in zip(four, by4):
        assert torch.equal(a, b)
    assert got[5].dtype == torch.int64 and got[5].shape == (2, 4)
    print(f"predict_instances(component=8) {H}x{W}: comp {got[5].tolist()}, areas {got[1][:, 0].tolist()} of {before[1][:, 0].tolist()}")
    assert len(wide) == 5 and wide[2].shape == (2, H * W + 1) and torch.equal(wide[1], got[1]) and torch.equal(wide[4], got[5])
    assert torch.equal(_i32(wide[3]), _i32(got[4])) and int(wide[1][:, 5].max()) <= wide[2].shape[1]
    recs = ops.instances_to_coco(*wide[:3], (H, W), image_ids=[7, 9], conf=wide[3])
    masks = np.stack([C.unpack(w, W) for w in got[3].cpu().numpy().view(np.uint32)])
    for b, r in enumerate(recs):
        assert r["image_id"] == (7, 9)[b] and r["area"] == int(masks[b].sum()) == int(got[1][b, 0]) and r["score"] == float(got[4][b, 0])
        assert r["segmentation"]["size"] == [H, W] and np.array_equal(RLE.decode(r["segmentation"]["counts"], H, W), masks[b])
        assert r["bbox"] == RLE.stats(masks[b])[1:5]


@pytest.mark.gpu
def test_predict_instances_component_repeats_within_every_precision_mode(deterministic):
    """The network in front of the component runs in the precision mode: the whole call, twice in each of the three modes, gives
    the same bits within the mode (the masks of two modes may differ)."""
    TP = _tp()
    module, _ = TP._module("hrnet")
    X, Fp = TP._batch(2, 256, 11)
    bias = module.decoder.cls_net.fc.bias
    keep = bias.detach().clone()
    mode0 = hip.get_conv_precision()
    with torch.no_grad():
        bias[-1] += 1000.0
    try:
        for mode in ("f32", "bf16x3", "f16x2"):
            hip.set_conv_precision(mode)
            a = module.predict_instances(X, Fp, return_bits=True, return_score=True, component=8)
            b = module.predict_instances(X, Fp, return_bits=True, return_score=True, component=8)
            module.check_nan()
            assert len(a) == len(b) == 6 and int(a[1][:, 0].min()) > 0, mode
            for s, t in zip(a, b):
                assert torch.equal(_i32(s), _i32(t)), mode
    finally:
        hip.set_conv_precision(mode0)
        with torch.no_grad():
            bias.copy_(keep)


@pytest.mark.gpu
def test_predict_instances_component_rejects_train_mode():
    TP = _tp()
    module, _ = TP._module("hrnet")
    X, Fp = TP._batch(2, 96, 3)
    module.train()
    try:
        with pytest.raises(RuntimeError, match="predict_instances"):
            module.predict_instances(X, Fp, component=8)
    finally:
        module.eval()


# ------------------------------------------------------------------------------------------------------- GPU: the session ---------
@pytest.mark.gpu
def test_session_follows_the_component():
    """A head with two blobs (fixed head parts behind the real predict_instances): the session's record is the blob under the gaze,
    and a gaze moved onto the other blob is outside that record's mask and re-makes it."""
    TP = _tp()
    module, _ = TP._module("hrnet")
    H = W = 64
    h = w = 16
    K = 4
    cls = torch.tensor([[0.5, 1.0, -0.3, 3.0]], device="cuda")
    m = torch.ones(1, h, w, device="cuda")
    m[0, 2:6, 2:6] = -1.0                                                                   # the head's foreground: the mask plane below the class planes
    m[0, 9:13, 9:14] = -1.0
    c = (torch.arange(w, device="cuda", dtype=torch.float32) + 0.5) / w * 2 - 1
    grid = torch.stack([c[None, :].expand(h, w), c[:, None].expand(h, w)], -1)[None].contiguous()       # (x, y) of a regular grid
    X = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    calls = []

    def parts(img, focus, seg_size, who):
        calls.append(int(img.shape[0]))
        return cls, m, grid, (H, W)
    module._head_parts = parts
    try:
        whole = module.predict_instances(X, torch.zeros(1, 2, device="cuda"), return_bits=True)
        mask = C.unpack(whole[3][0].cpu().numpy().view(np.uint32), W)
        lab, n = C.ndimage.label(mask, structure=C.FULL)
        assert n == 2, "the stub head must make two blobs"
        (ya, xa), (yb, xb) = [tuple(int(v) for v in np.argwhere(lab == i).mean(0).round()) for i in (1, 2)]
        assert lab[ya, xa] == 1 and lab[yb, xb] == 2 and np.hypot(ya - yb, xa - xb) > 20
        Fa = torch.from_numpy(at(ya, xa, H, W))[None].cuda()
        Fb = torch.from_numpy(at(yb, xb, H, W))[None].cuda()
        want_a = module.predict_instances(X, Fa, return_bits=True, component=8)
        want_b = module.predict_instances(X, Fb, return_bits=True, component=8)
        assert np.array_equal(C.unpack(want_a[3][0].cpu().numpy().view(np.uint32), W), lab == 1)
        assert np.array_equal(C.unpack(want_b[3][0].cpu().numpy().view(np.uint32), W), lab == 2)
        assert int(want_a[1][0, 0]) == int((lab == 1).sum()) and int(whole[1][0, 0]) == int(mask.sum())
        calls.clear()
        s = GazeSession(module, 1, (H, W), component=8, saccade_px=None, fixation_px=2)
        *rec, gate = s.step(X, Fa)                                                          # 1: made
        assert gate[0, 0] == 1 and calls == [1] and len(rec) == 4
        for a, b in zip(rec, want_a[:4]):
            assert torch.equal(a, b)
        held = [t.clone() for t in rec]
        *rec, gate = s.step(X, Fa)                                                          # 2: reused
        assert gate[0, 0] == 0 and calls == [1]
        for a, b in zip(rec, held):
            assert torch.equal(a, b)
        *rec, gate = s.step(X, Fb)                                                          # 3: the gaze on the other blob
        assert gate[0, 0] == 5 and gate[0, 6] == 0 and calls == [1, 1], gate.tolist()      # RUN_GAZE: outside the record's mask
        for a, b in zip(rec, want_b[:4]):
            assert torch.equal(a, b)
        # without the component the same move stays on the head's mask and reuses the record of both blobs
        calls.clear()
        s0 = GazeSession(module, 1, (H, W), saccade_px=None, fixation_px=2)
        s0.step(X, Fa)
        *rec0, gate0 = s0.step(X, Fb)
        assert gate0[0, 0] == 0 and gate0[0, 6] == 1 and calls == [1] and torch.equal(rec0[3], whole[3])
        sc = GazeSession(module, 1, (H, W), component=4, snap_px=1, score=True, saccade_px=None)
        *rec, gate = sc.step(X, Fa)
        want = module.predict_instances(X, Fa, return_bits=True, return_score=True, component=4, snap_px=1)
        assert len(rec) == 5 and all(torch.equal(_i32(a), _i32(b)) for a, b in zip(rec, want[:5]))
    finally:
        del module._head_parts
