"""Showing the record: fs_frame_overlay / fs_frame_overlay_u8 / fs_frame_overlay_hwc, fs_color_encode, ops.overlay_style, ops.draw_instances,
ops.color_encode and GazeSession.render against tests/overlay_ref.py, the rule of include/fovealseg.h as a double loop over pixels.

The rule is all integers, so every comparison is np.array_equal / torch.equal.  The reference is held to hand-derived answers first
(CPU).  On the GPU every destination sits between guard bands in a buffer of random bytes and the WHOLE buffer is compared with the
reference placed into a copy of it: pitch padding, gaps and guard bands must come back untouched, an RGBA pixel's fourth byte 255.  Bits
and band are random words, padding bits included; alpha bytes, pitch padding and gaps of the sources are random too."""
import os

import numpy as np
import pytest
import torch

from fovealseg import hip, ops
from fovealseg.session import GazeSession

import boundary_ref as BR
import gate_ref as R
import motion_ref as M
import overlay_ref as O
import rle_ref as RLE
import kernel_testing                                                                                  # noqa: F401  (the suite's shared helpers import)
from test_gaze_session import Guarded, _GARB, served                                                   # noqa: F401  (served is a fixture)
from test_frames_hwc import Frame
from test_frames_u8 import _bytes_of, SIZE

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY_POINTS = ("fs_frame_overlay", "fs_frame_overlay_u8", "fs_frame_overlay_hwc", "fs_color_encode")
OFF = O.style_row()                                       # nothing switched on: a = 0, dim = 256, t = r = 0, no outline


def words_of(mask):
    """(B,H,W) bool -> (B,H,P) int32 bit words."""
    return np.stack([RLE.bits(m) for m in mask])


def grey(B, H, W, v):
    return np.full((B, 3, H, W), v, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------ CPU: the reference ----
def test_the_ctypes_table_binds_the_overlay_entry_points():
    tail = "ppppp" + "l" + "pi" + "plli" + "iii"
    assert hip.SIGNATURES["fs_frame_overlay"] == hip.SIGNATURES["fs_frame_overlay_u8"] == "p" + tail
    assert hip.SIGNATURES["fs_frame_overlay_hwc"] == "plli" + tail
    assert hip.SIGNATURES["fs_color_encode"] == "pp" + "plli" + "iiii"
    assert all(name in hip.SIGNATURES for name in ENTRY_POINTS)


def test_reference_one_set_bit_at_the_word_and_half_word_borders():
    H, W = 2, 40
    src = grey(1, H, W, 9)
    style = [O.style_row(tint=(200, 100, 50), a=256)]                   # a = 256: a mask pixel is the tint itself
    for x in (15, 16, 31, 32, W - 1):
        mask = np.zeros((1, H, W), dtype=bool)
        mask[0, 1, x] = True
        got = O.draw(src, words_of(mask), style=style)
        want = src.copy()
        want[0, :, 1, x] = (200, 100, 50)
        assert np.array_equal(got, want), x
        # the padding bits of the last word are no pixels
        w = words_of(mask).copy()
        w[0, :, 1] |= np.int32(-1) << np.int32(W - 32)
        assert np.array_equal(O.draw(src, w, style=style), want), x


def test_reference_blend_and_dim_rounding():
    s = np.array([0, 1, 127, 255], dtype=np.uint8)
    src = np.broadcast_to(s[None, None, None, :], (1, 3, 1, 4)).copy()
    full, none = words_of(np.ones((1, 1, 4), dtype=bool)), words_of(np.zeros((1, 1, 4), dtype=bool))
    # (s * (256 - a) + 200 * a + 128) >> 8: a = 0 -> (256 s + 128) >> 8 = s; a = 128 -> 128 (s + 201) >> 8 = (s + 201) >> 1; a = 256 -> 200
    for a, want in ((0, [0, 1, 127, 255]), (128, [100, 101, 164, 228]), (256, [200, 200, 200, 200])):
        got = O.draw(src, full, style=[O.style_row(tint=(200, 200, 200), a=a, dim=0)])
        assert got[0, 0, 0].tolist() == got[0, 1, 0].tolist() == got[0, 2, 0].tolist() == want, a
    # (s * dim + 128) >> 8: dim = 0 -> 128 >> 8 = 0; dim = 255 -> (128, 383, 32513, 65153) >> 8 = (0, 1, 127, 254); dim = 256 -> s
    for dim, want in ((0, [0, 0, 0, 0]), (255, [0, 1, 127, 254]), (256, [0, 1, 127, 255])):
        got = O.draw(src, none, style=[O.style_row(tint=(200, 200, 200), a=77, dim=dim)])
        assert got[0, 0, 0].tolist() == got[0, 2, 0].tolist() == want, dim


def _stats(x0, y0, bw, bh, area=1):
    return np.array([[area, x0, y0, bw, bh, 1]], dtype=np.int64)


def test_reference_boxes():
    H, W = 6, 8
    src, none = grey(1, H, W, 40), words_of(np.zeros((1, H, W), dtype=bool))
    style = lambda t: [O.style_row(box=(1, 2, 3), t=t)]
    hit = lambda got: {(y, x) for y in range(H) for x in range(W) if got[0, :, y, x].tolist() == [1, 2, 3]}
    rest = lambda got: all(got[0, :, y, x].tolist() == [40, 40, 40] for y in range(H) for x in range(W) if (y, x) not in hit(got))
    got = O.draw(src, none, stats=_stats(2, 1, 1, 1), style=style(1))                      # a 1 x 1 box is its one pixel
    assert hit(got) == {(1, 2)} and rest(got)
    got = O.draw(src, none, stats=_stats(1, 1, 4, 3), style=style(5))                      # t above half a side: the box is filled
    assert hit(got) == {(y, x) for y in (1, 2, 3) for x in (1, 2, 3, 4)} and rest(got)
    got = O.draw(src, none, stats=_stats(1, 0, 5, 4), style=style(1))                      # a frame one pixel thick, its inside untouched
    assert hit(got) == {(y, x) for y in range(4) for x in range(1, 6)} - {(y, x) for y in (1, 2) for x in (2, 3, 4)} and rest(got)
    for st in (_stats(1, 1, 0, 3), _stats(1, 1, 4, 0), _stats(1, 1, -4, 3)):              # bw = 0, bh = 0, a negative width: no box
        assert np.array_equal(O.draw(src, none, stats=st, style=style(2)), src)
    assert np.array_equal(O.draw(src, none, stats=_stats(1, 1, 4, 3), style=style(0)), src)            # t = 0 switches it off
    assert np.array_equal(O.draw(src, none, stats=None, style=style(2)), src)
    got = O.draw(src, none, stats=_stats(-2 ** 62, -2 ** 62, 2 ** 62 + 3, 2 ** 62 + 2), style=style(1))     # the box ends at x = 2, y = 1
    assert hit(got) == {(y, x) for y in (0, 1) for x in (0, 1, 2)} - {(0, 0), (0, 1)} and rest(got)


def test_reference_markers():
    H, W = 5, 6
    src, none = grey(1, H, W, 40), words_of(np.zeros((1, H, W), dtype=bool))
    hit = lambda got: {(y, x) for y in range(H) for x in range(W) if got[0, :, y, x].tolist() == [9, 8, 7]}
    disc = {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)}                               # y^2 + x^2 <= 4, clipped by the frame's corner
    f0 = np.zeros((1, 2), dtype=np.float32)
    assert hit(O.draw(src, none, focus=f0, style=[O.style_row(marker=(9, 8, 7), r=2, w=2)])) == disc
    assert hit(O.draw(src, none, focus=f0, style=[O.style_row(marker=(9, 8, 7), r=2, w=99)])) == disc
    assert hit(O.draw(src, none, focus=f0, style=[O.style_row(marker=(9, 8, 7), r=2, w=1)])) == disc - {(0, 0)}       # a ring: d2 >= 1
    assert hit(O.draw(src, none, focus=f0, style=[O.style_row(marker=(9, 8, 7), r=2, w=0)])) == {(0, 2), (2, 0)}      # d2 == 4 alone
    nan = np.full((1, 2), np.nan, dtype=np.float32)
    assert hit(O.draw(src, none, focus=nan, style=[O.style_row(marker=(9, 8, 7), r=2, w=2)])) == disc                 # NaN -> 0
    far = np.array([[1.0, 1.0]], dtype=np.float32)                                       # (4, 5), the opposite corner; r = 1: a plus sign, clipped
    assert hit(O.draw(src, none, focus=far, style=[O.style_row(marker=(9, 8, 7), r=1, w=1)])) == {(4, 5), (3, 5), (4, 4)}
    assert np.array_equal(O.draw(src, none, focus=f0, style=[O.style_row(marker=(9, 8, 7), r=0, w=3)]), src)          # r = 0 switches it off
    assert np.array_equal(O.draw(src, none, focus=None, style=[O.style_row(marker=(9, 8, 7), r=2, w=2)]), src)


def test_reference_priority_and_live():
    H, W = 3, 4
    src = grey(1, H, W, 100)
    mask = np.zeros((1, H, W), dtype=bool)
    mask[0, 1, 1] = True
    w = words_of(mask)
    f = np.array([[0.5, 1.0 / 3.0]], dtype=np.float32)                                    # the gaze pixel (1, 1)
    assert (O.gaze_pixel(f[0, 0], H), O.gaze_pixel(f[0, 1], W)) == (1, 1)
    every = dict(tint=(10, 10, 10), a=256, outline=(20, 20, 20), flag=1, dim=128, box=(30, 30, 30), t=1, marker=(40, 40, 40), r=1, w=1)
    st = _stats(1, 1, 1, 1)
    at = lambda **kw: O.draw(src, w, band=kw.pop("band", w), stats=kw.pop("stats", st), focus=kw.pop("focus", f), live=kw.pop("live", None),
                             style=[O.style_row(**{**every, **kw})])[0, :, 1, 1].tolist()
    assert at() == [40] * 3                                                               # all five meet on (1, 1): the marker
    assert at(r=0) == [30] * 3 and at(focus=None) == [30] * 3                             # then the box
    assert at(r=0, t=0) == [20] * 3 and at(r=0, stats=None) == [20] * 3                   # then the outline
    assert at(r=0, t=0, flag=0) == [10] * 3 and at(r=0, t=0, band=None) == [10] * 3       # then the tint
    zero = words_of(np.zeros((1, H, W), dtype=bool))
    assert O.draw(src, zero, style=[O.style_row(**{**every, "r": 0, "t": 0})])[0, :, 1, 1].tolist() == [50] * 3       # (100 * 128 + 128) >> 8
    # live = 0: mask, band and box count as empty; the marker and dim still apply
    dead = np.zeros(1, dtype=np.int64)
    assert at(live=dead) == [40] * 3 and at(live=dead, r=0) == [50] * 3
    got = O.draw(src, w, band=w, stats=st, focus=f, live=dead, style=[O.style_row(**every)])
    assert got[0, :, 0, 0].tolist() == [50] * 3 and got[0, :, 0, 1].tolist() == [40] * 3
    assert at(live=np.array([7], dtype=np.int64)) == [40] * 3 and at(live=np.array([-1], dtype=np.int64), r=0) == [30] * 3


def _random_case(seed, B, H, W, S, hostile=False):
    """A record with every element on: random words (padding bits included), a box, a gaze, live flags, a style row a viewer."""
    rng = np.random.default_rng(seed)
    P = (W + 31) // 32
    c = {"bits": rng.integers(-2 ** 31, 2 ** 31, (B, H, P)).astype(np.int32), "band": rng.integers(-2 ** 31, 2 ** 31, (B, H, P)).astype(np.int32)}
    c["band"] &= rng.integers(-2 ** 31, 2 ** 31, (B, H, P)).astype(np.int32)
    stats = np.zeros((B, 6), dtype=np.int64)
    for b in range(B):
        x0, y0 = int(rng.integers(-2, W)), int(rng.integers(-2, H))
        stats[b] = (5, x0, y0, int(rng.integers(1, W + 3)), int(rng.integers(1, H + 3)), 1)
    c["stats"] = stats
    c["focus"] = rng.random((B, 2)).astype(np.float32) * 1.2 - 0.1
    gstate = rng.integers(0, 3, (B, 6)).astype(np.int64)
    gstate[0, 0] = 1
    c["gstate"] = gstate
    rows = []
    for _ in range(S):
        col = lambda: tuple(int(v) for v in rng.integers(0, 256, 3))
        rows.append(O.style_row(tint=col(), a=int(rng.integers(0, 257)), outline=col(), dim=int(rng.integers(0, 257)), box=col(), t=int(rng.integers(1, 3)),
                                marker=col(), r=int(rng.integers(1, 4)), w=int(rng.integers(0, 3)), flag=1))
    if hostile:
        big = [2 ** 31 - 1, -2 ** 31, 70000, -70000, 257, -1, 16385, 2 ** 30]
        rows = [[int(rng.choice(big)) if rng.random() < 0.6 else v for v in row] for row in rows]
        for b in range(B):
            stats[b, 1:5] = [int(rng.choice([2 ** 62, -2 ** 62, 1, 0])) for _ in range(4)]
        stats[0, 1:5] = (-2 ** 62, -2 ** 62, 2 ** 62 + 2, 2 ** 62 + 1)
        c["focus"][0] = (np.nan, np.inf)
    c["style"] = np.array(rows, dtype=np.int32)
    return c


def _ref(c, src, draw=O.draw, **nulls):
    get = lambda k: None if nulls.get(k) else c[k]
    return draw(src, c["bits"], band=get("band"), stats=get("stats"), focus=get("focus"), live=None if nulls.get("live") else c["gstate"][:, 0],
                style=c["style"])


def test_reference_whole_planes_equal_the_double_loop():
    for seed, (B, H, W, S, hostile) in enumerate([(2, 5, 33, 2, False), (1, 6, 40, 1, False), (3, 4, 64, 1, True), (2, 7, 9, 2, True)]):
        c = _random_case(100 + seed, B, H, W, S, hostile)
        rng = np.random.default_rng(seed)
        for src in (rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8), (rng.random((B, 3, H, W)) * 1.4 - 0.2).astype(np.float32)):
            for nulls in ({}, {"band": 1}, {"stats": 1}, {"focus": 1}, {"live": 1}):
                assert np.array_equal(_ref(c, src, **nulls), _ref(c, src, draw=O.draw_planes, **nulls))


# ------------------------------------------------------------------------------------------------------------------ CPU: the Python surface ----
def test_overlay_style_packing_and_refusals():
    s = ops.overlay_style()
    assert s.dtype == torch.int32 and tuple(s.shape) == (1, 20) and s.device.type == "cpu"
    assert s[0].tolist() == O.style_row(tint=(0, 255, 0), a=128, dim=256)
    s = ops.overlay_style(tint=(1, 2, 3), alpha=256, outline=(4, 5, 6), box=(7, 8, 9), box_px=3, marker=(10, 11, 12), marker_px=5, marker_width=2, dim=90)
    assert s[0].tolist() == O.style_row(tint=(1, 2, 3), a=256, outline=(4, 5, 6), dim=90, box=(7, 8, 9), t=3, marker=(10, 11, 12), r=5, w=2, flag=1)
    assert ops.overlay_style(marker=(1, 1, 1), marker_px=7)[0, 15:17].tolist() == [7, 7]              # no width: a disc
    assert ops.overlay_style(box_px=9, marker_px=9)[0, 8:17].tolist() == [0] * 9                     # no colour: the element is off
    pal = torch.tensor([[10, 20, 30], [40, 50, 60]], dtype=torch.uint8)
    s = ops.overlay_style(tint=(9, 9, 9), alpha=64, cat=torch.tensor([1, 0, 2, -1]), palette=pal)
    assert tuple(s.shape) == (4, 20) and s[:, 0:3].tolist() == [[40, 50, 60], [10, 20, 30], [9, 9, 9], [9, 9, 9]] and s[:, 3].tolist() == [64] * 4
    for bad in (dict(tint=(1, 2)), dict(tint=(1, 2, 256)), dict(tint=(1, 2, -1)), dict(tint="abc"), dict(tint=(1.5, 2, 3)), dict(alpha=257), dict(alpha=-1),
                dict(dim=300), dict(dim=True), dict(outline=(0, 0)), dict(box=(1, 1, 1), box_px=-1), dict(box=(1, 1, 1), box_px=16385),
                dict(marker=(1, 1, 1), marker_px=-2), dict(marker=(1, 1, 1), marker_width=-1), dict(cat=torch.tensor([0])), dict(palette=pal),
                dict(cat=torch.tensor([0.5]), palette=pal), dict(cat=torch.tensor([[0]]), palette=pal), dict(cat=torch.tensor([0]), palette=pal.float()),
                dict(cat=torch.tensor([0]), palette=pal[:, :2])):
        with pytest.raises(ValueError):
            ops.overlay_style(**bad)


def test_byte_frame_dest_classifies_out_tensors():
    B, H, W = 3, 6, 8
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    assert ops.byte_frame_dest(u8(B, 3, H, W)) == (3 * H * W, W, 1)
    assert ops.byte_frame_dest(u8(B, H, W, 3).permute(0, 3, 1, 2)) == (H * W * 3, W * 3, 3)
    assert ops.byte_frame_dest(u8(B, H, W, 4).permute(0, 3, 1, 2)[:, :3]) == (H * W * 4, W * 4, 4)
    crop = u8(B, H + 5, W + 7, 4)[:, 2:2 + H, 3:3 + W, :3].permute(0, 3, 1, 2)
    assert ops.byte_frame_dest(crop, (B, 3, H, W)) == ((H + 5) * (W + 7) * 4, (W + 7) * 4, 4)
    assert ops.byte_frame_dest(u8(1, H, W, 3).permute(0, 3, 1, 2)) == (0, W * 3, 3)                   # one image: no image step
    for bad in (u8(1, H, W, 3).permute(0, 3, 1, 2).expand(B, 3, H, W),                               # every viewer would write the one image
                u8(B, 3, H, 2 * W)[:, :, :, ::2], u8(B, W, H, 3).permute(0, 3, 2, 1), u8(B, 3, H, W).float(), u8(3, H, W), None):
        with pytest.raises(ValueError):
            ops.byte_frame_dest(bad)
    with pytest.raises(ValueError):
        ops.byte_frame_dest(u8(B, 3, H, W), (B, 3, H, W + 1))
    # draw_instances and color_encode refuse before any launch (CPU tensors: a launch would raise another error)
    bits = torch.zeros(B, H, 1, dtype=torch.int32)
    for bad in (dict(img=u8(B, 3, H, W).double()), dict(bits=bits.long()), dict(bits=bits[:, :, :0]), dict(stats=torch.zeros(B, 5, dtype=torch.int64)),
                dict(style=torch.zeros(2, 20, dtype=torch.int32)), dict(style=torch.zeros(1, 19, dtype=torch.int32)), dict(outline_px=-1),
                dict(live=torch.zeros(B, dtype=torch.int32)), dict(focus=torch.zeros(B, 3)), dict(out=u8(B, 3, H, W + 1))):
        kw = {"img": u8(B, 3, H, W), "bits": bits, **bad}
        with pytest.raises(ValueError):
            ops.draw_instances(kw.pop("img"), kw.pop("bits"), **kw)
    pal = torch.zeros(4, 3, dtype=torch.uint8)
    for labels, p in ((torch.zeros(H, W), pal), (torch.zeros(H, dtype=torch.int64), pal), (torch.zeros(H, W, dtype=torch.int64), pal.int()),
                      (torch.zeros(H, W, dtype=torch.int64), pal[:, :2])):
        with pytest.raises(ValueError):
            ops.color_encode(labels, p)


def test_color_encode_restatement_against_the_reference():
    """tests/golden/g_color_encode.npz (make_color_encode_golden.py): utils.colorEncode with data/color150.mat on a seeded 8 x 12 map that
    includes -1 -- pinned where the fixture covers it; a label >= K raises in the reference and is black here (unpinned)."""
    g = np.load(os.path.join(HERE, "golden", "g_color_encode.npz"))
    labels, colors, rgb = g["labels"], g["colors"], g["rgb"]
    assert labels.shape == (8, 12) and (labels == -1).sum() >= 2 and labels.max() == 149 and colors.shape == (150, 3) and colors.dtype == np.uint8
    got = O.color_encode(labels[None], colors)
    assert np.array_equal(got[0].transpose(1, 2, 0), rgb)
    assert (rgb[labels == -1] == 0).all()
    over = labels.copy()
    over[1, 1] = 150
    assert O.color_encode(over[None], colors)[0, :, 1, 1].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ GPU: the C ABI ----
SIZES = [(2, 1), (5, 33), (4, 40), (3, 16), (9, 48), (7, 64), (6, 80)]
# interleaved sources (tests/test_frames_hwc.py LAYOUTS): tight RGB, RGBA with garbage alpha, pitched rows with garbage padding on the
# vector and on the one-pixel route, one frame for all viewers, a pointer moved one byte
HWC_SOURCES = [("tight", 3), ("tight", 4), ("pitch16", 4), ("pitch5", 3), ("sb0", 3), ("off1", 3), ("off1", 4)]


class Dest:
    """A destination in a buffer of random bytes between guard bands: planar, tight RGB, or RGBA with padded rows and a gap between images."""

    def __init__(self, kind, B, H, W, off=0, seed=0):
        self.B, self.H, self.W = B, H, W
        if kind == "planar":
            self.ob, self.oy, self.ox = 3 * H * W, W, 1
        elif kind == "rgb":
            self.ob, self.oy, self.ox = H * W * 3, W * 3, 3
        else:
            self.oy, self.ox = W * 4 + 16, 4
            self.ob = H * self.oy + 32
        self.buf = np.random.default_rng(seed).integers(0, 256, B * self.ob).astype(np.uint8)
        self.g = Guarded(self.buf.size, torch.uint8, body=torch.from_numpy(self.buf), off=off)

    @property
    def args(self):
        return (self.g.ptr, self.ob, self.oy, self.ox)

    def check(self, want_planar, what):
        got = self.g.host(-1).numpy()                                                  # asserts the guard bands
        want = O.place(want_planar, self.ob, self.oy, self.ox, self.buf)
        assert np.array_equal(got, want), what


DESTS = ("planar", "rgb", "rgba_pitch")


def _planar_bytes(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, 3, H, W)).astype(np.uint8)


def _floats(B, H, W, seed):
    """An fp32 frame with NaN, infinities and values outside 0 .. 1."""
    rng = np.random.default_rng(seed)
    x = (rng.random((B, 3, H, W)) * 1.6 - 0.3).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] = np.nan
    flat[3::11] = np.inf
    flat[5::13] = -np.inf
    flat[1::17] = 0.5
    return x


class Record:
    """A case's record on the device, and the arguments that follow the frame."""

    def __init__(self, c):
        self.c = c
        self.t = {k: torch.from_numpy(c[k]).cuda() for k in ("bits", "band", "stats", "focus", "gstate", "style")}

    def args(self, **nulls):
        p = lambda k: None if nulls.get(k) else self.t[k].data_ptr()
        return (p("bits"), p("band"), p("stats"), p("focus"), None if nulls.get("live") else self.t["gstate"].data_ptr(), 6, p("style"),
                int(self.c["style"].shape[0]))


def _sources(B, H, W, seed, offs):
    """(name, entry point, guarded source, frame arguments, the planar frame the reference reads, unchanged()) for every source kind."""
    U, X = _planar_bytes(B, H, W, seed), _floats(B, H, W, seed + 1)
    out = []
    for off in offs:
        gf = Guarded(X.size, torch.float32, body=torch.from_numpy(X), off=off)
        out.append((f"fp32 off {off}", "fs_frame_overlay", gf, (gf.ptr,), X, lambda g=gf: g.intact() and torch.equal(g.body.cpu().view(torch.int32), torch.from_numpy(X).reshape(-1).view(torch.int32))))
        gu = Guarded(U.size, torch.uint8, body=torch.from_numpy(U), off=off)
        out.append((f"bytes off {off}", "fs_frame_overlay_u8", gu, (gu.ptr,), U, lambda g=gu: g.intact() and torch.equal(g.body.cpu(), torch.from_numpy(U).reshape(-1))))
    for name, sx in HWC_SOURCES:
        if name == "off1" and 1 not in offs:
            continue
        f = Frame(U, name, sx, seed=seed + 2)
        g = f.guarded()
        out.append((f"{name} sx {sx}", "fs_frame_overlay_hwc", g, f.args(g), f.planar, lambda f=f, g=g: f.unchanged(g)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_entry_points_against_the_reference(H, W):
    """Every source x destination x (B, S), on the vector route and (widths that are multiples of 16) on the one-pixel route, forced by
    a source or a destination pointer moved one byte: both equal the reference, so each other."""
    offs = (0, 1) if W % 16 == 0 else (0,)
    for B, S in ((1, 1), (3, 1), (3, 3)):
        c = _random_case(1000 * H + 10 * W + B + S, B, H, W, S)
        rec = Record(c)
        refs = {}
        for name, entry, g, fargs, planar, unchanged in _sources(B, H, W, H * W + B, offs):
            key = (planar.dtype.str, planar.tobytes())
            if key not in refs:
                refs[key] = _ref(c, planar)
            for kind in DESTS:
                for doff in offs:
                    d = Dest(kind, B, H, W, off=doff, seed=H + W + doff)
                    hip.call(entry, *fargs, *rec.args(), *d.args, B, H, W)
                    d.check(refs[key], (name, kind, doff, B, S))
            assert unchanged(), name
        assert all(np.array_equal(t.cpu().numpy(), c[k]) for k, t in rec.t.items())


@pytest.mark.gpu
def test_transcode_with_nothing_switched_on():
    """a = 0, dim = 256 and every element off: out is the source's codes for every source x destination pair, alpha 255."""
    for H, W in ((4, 40), (3, 16)):
        B = 2
        c = _random_case(7, B, H, W, 1)
        c["style"] = np.array([OFF], dtype=np.int32)
        rec = Record(c)
        for name, entry, g, fargs, planar, unchanged in _sources(B, H, W, 77, (0,)):
            for kind in DESTS:
                d = Dest(kind, B, H, W, seed=3)
                hip.call(entry, *fargs, *rec.args(), *d.args, B, H, W)
                d.check(O.codes(planar).astype(np.uint8), (name, kind))


@pytest.mark.gpu
def test_hostile_records_and_null_elements():
    """Bits at x >= W set (always: random words), style entries far out of range, stats of +-2^62, NaN and infinite gaze; then a null
    band, stats, focus or live, each alone."""
    for H, W in ((5, 33), (7, 64)):
        B = 3
        for hostile in (True, False):
            c = _random_case(31 + H, B, H, W, B, hostile=hostile)
            rec = Record(c)
            for name, entry, g, fargs, planar, unchanged in _sources(B, H, W, 5, (0,))[:4]:
                for nulls in ({},) if hostile else ({"band": 1}, {"stats": 1}, {"focus": 1}, {"live": 1}):
                    want = _ref(c, planar, **nulls)
                    for kind in ("planar", "rgba_pitch"):
                        d = Dest(kind, B, H, W, seed=9)
                        hip.call(entry, *fargs, *rec.args(**nulls), *d.args, B, H, W)
                        d.check(want, (name, kind, hostile, nulls))


@pytest.mark.gpu
def test_in_place_equals_out_of_place():
    for H, W in ((7, 64), (5, 33)):
        B = 2
        c = _random_case(50 + W, B, H, W, B)
        rec = Record(c)
        U = _planar_bytes(B, H, W, 8)
        want = _ref(c, U)
        g = Guarded(U.size, torch.uint8, body=torch.from_numpy(U))
        hip.call("fs_frame_overlay_u8", g.ptr, *rec.args(), g.ptr, 3 * H * W, W, 1, B, H, W)
        assert np.array_equal(g.host(B, 3, H, W).numpy(), want)
        for name in ("tight", "pitch16"):
            f = Frame(U, name, 4, seed=4)
            g = f.guarded()
            hip.call("fs_frame_overlay_hwc", *f.args(g), *rec.args(), g.ptr, f.sb, f.sy, 4, B, H, W)
            assert np.array_equal(g.host(-1).numpy(), O.place(want, f.sb, f.sy, 4, f.buf)), name


@pytest.mark.gpu
def test_refusals_launch_nothing():
    B, H, W = 3, 4, 16
    c = _random_case(1, B, H, W, B)
    rec = Record(c)
    U, X = _planar_bytes(B, H, W, 2), _floats(B, H, W, 3)
    gu = Guarded(U.size, torch.uint8, body=torch.from_numpy(U))
    gf = Guarded(X.size, torch.float32, body=torch.from_numpy(X))
    f = Frame(U, "tight", 4, seed=1)
    gh = f.guarded()
    out = Guarded(B * H * W * 4 + 64, torch.uint8)

    def rejected(name, args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call(name, *args)
        torch.cuda.synchronize()
        assert out.intact() and bool((out.body == _GARB[torch.uint8]).all()), f"a rejected {name} launched something"
        assert torch.equal(gu.body.cpu(), torch.from_numpy(U).reshape(-1)) and f.unchanged(gh)

    def each(name, good, bads):
        for i, bad in bads:
            a = list(good)
            a[i] = bad
            rejected(name, a)

    planar, rgb, rgba = (out.ptr, 3 * H * W, W, 1), (out.ptr, 3 * H * W, 3 * W, 3), (out.ptr, 4 * H * W, 4 * W, 4)
    tail = (B, H, W)
    good = [gu.ptr, *rec.args(), *planar, *tail]
    hip.call("fs_frame_overlay_u8", *good)                                              # the good call is good
    out.body.fill_(_GARB[torch.uint8])
    common = ((1, None), (7, None), (9, None), (8, 2), (8, 0), (8, B + 1), (13, 0), (13, -1), (14, 0), (15, 0), (15, -3), (14, 16385), (15, 16385),
              (12, 0), (12, 2), (12, 5), (12, -1), (6, 0), (6, -6), (10, 0), (10, 3 * H * W - 1), (10, -3 * H * W), (11, W - 1), (11, W + 1))
    each("fs_frame_overlay_u8", good, ((0, None),) + common)
    each("fs_frame_overlay", [gf.ptr, *rec.args(), *planar, *tail], ((0, None),) + common)
    goodh = [*f.args(gh), *rec.args(), *planar, *tail]
    each("fs_frame_overlay_hwc", goodh, ((0, None), (3, 5), (3, 1), (2, 4 * W - 1), (1, -1), (1, H * 4 * W - 1)) + tuple((i + 3, bad) for i, bad in common))
    for dest in (rgb, rgba):
        good = [gu.ptr, *rec.args(), *dest, *tail]
        each("fs_frame_overlay_u8", good, ((11, dest[2] - 1), (10, H * dest[2] - 1), (10, 0)))
    # out == img with differing descriptions
    rejected("fs_frame_overlay", [gf.ptr, *rec.args(), gf.ptr, 3 * H * W, W, 1, *tail])
    rejected("fs_frame_overlay_u8", [gu.ptr, *rec.args(), gu.ptr, 3 * H * W, 3 * W, 3, *tail])
    rejected("fs_frame_overlay_u8", [gu.ptr, *rec.args(), gu.ptr, 3 * H * W + 16, W, 1, *tail])
    rejected("fs_frame_overlay_hwc", [*f.args(gh), *rec.args(), gh.ptr, f.sb, f.sy, 3, *tail])
    rejected("fs_frame_overlay_hwc", [*f.args(gh), *rec.args(), gh.ptr, f.sb, f.sy + 4, 4, *tail])
    rejected("fs_frame_overlay_hwc", [*f.args(gh), *rec.args(), gh.ptr, 3 * H * W, W, 1, *tail])
    assert gf.intact() and torch.equal(gf.body.cpu().view(torch.int32), torch.from_numpy(X).reshape(-1).view(torch.int32))
    # fs_color_encode
    labels = torch.zeros(B, H, W, dtype=torch.int64, device="cuda")
    pal = torch.zeros(5, 3, dtype=torch.uint8, device="cuda")
    each("fs_color_encode", [labels.data_ptr(), pal.data_ptr(), *planar, *tail, 5],
         ((0, None), (1, None), (2, None), (9, 0), (9, -1), (6, 0), (7, 0), (8, -1), (7, 16385), (5, 2), (5, 0), (4, W + 1), (3, 0), (3, 3 * H * W - 1)))


@pytest.mark.gpu
def test_color_encode_entry_point():
    g = np.load(os.path.join(HERE, "golden", "g_color_encode.npz"))
    colors = g["colors"]
    K = colors.shape[0]
    assert colors.flags.c_contiguous                                                      # its pointer goes to the entry point as it is
    pal = torch.from_numpy(colors).cuda()
    for H, W in ((5, 33), (4, 64)):
        B = 2
        rng = np.random.default_rng(H)
        labels = rng.integers(-1, K + 1, (B, H, W)).astype(np.int64)
        labels[0, 0, 0], labels[1, H - 1, W - 1], labels[0, 1, 1], labels[1, 0, 2] = -1, K, 2 ** 62, -2 ** 62
        want = O.color_encode(labels, colors)
        ld = torch.from_numpy(labels).cuda()
        for kind in DESTS:
            d = Dest(kind, B, H, W, seed=H)
            hip.call("fs_color_encode", ld.data_ptr(), pal.data_ptr(), *d.args, B, H, W, K)
            d.check(want, (H, W, kind))
        assert torch.equal(ld.cpu(), torch.from_numpy(labels))
        assert np.array_equal(ops.color_encode(ld, pal).cpu().numpy(), want)
        rgba = torch.zeros(B, H, W, 4, dtype=torch.uint8, device="cuda")
        assert ops.color_encode(ld, colors, out=rgba.permute(0, 3, 1, 2)[:, :3]).data_ptr() == rgba.data_ptr()
        assert np.array_equal(rgba[..., :3].permute(0, 3, 1, 2).cpu().numpy(), want) and bool((rgba[..., 3] == 255).all())
    # the pinned map through the kernel
    got = ops.color_encode(torch.from_numpy(g["labels"]).cuda(), pal)
    assert np.array_equal(got[0].permute(1, 2, 0).cpu().numpy(), g["rgb"])


# ------------------------------------------------------------------------------------------------------------------ GPU: composed calls ----
def _band_words(bits, W, d):
    m = O.unbits(bits, W)
    return words_of(np.stack([BR.band(x, d) for x in m]))


@pytest.mark.gpu
def test_draw_instances_on_a_predicted_record(served):
    module, calls, TP = served
    X, Fp = TP._batch(2, SIZE, 11)
    U = _bytes_of(X)
    U0 = U.clone()
    cat, stats, counts, bits = module.predict_instances(U, Fp, return_bits=True)
    assert 0 < int(stats[0, 0]) < SIZE * SIZE
    pal = torch.from_numpy(np.load(os.path.join(HERE, "golden", "g_color_encode.npz"))["colors"])
    style = ops.overlay_style(tint=(255, 0, 0), alpha=96, outline=(255, 255, 0), box=(0, 0, 255), box_px=2, marker=(255, 255, 255), marker_px=5,
                              marker_width=2, dim=160, cat=cat, palette=pal)
    assert style.is_cuda and tuple(style.shape) == (2, 20)
    b, s, f, st = bits.cpu().numpy(), stats.cpu().numpy(), Fp.cpu().numpy(), style.cpu().numpy()
    rgba = torch.randint(0, 256, (2, SIZE, SIZE, 4), dtype=torch.uint8, device="cuda")
    rgba[..., :3] = U.permute(0, 2, 3, 1)
    for d in (0, 1, 3):
        band = _band_words(b, SIZE, d) if d else None
        for src in (U, U.float() / 255, rgba.permute(0, 3, 1, 2)[:, :3]):
            want = O.draw_planes(src.cpu().numpy() if src.dtype == torch.float32 else U.cpu().numpy(), b, band=band, stats=s, focus=f, style=st)
            got = ops.draw_instances(src, bits, stats=stats, focus=Fp, style=style, outline_px=d)
            assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), d
    # camera RGBA in, display RGBA out, in place
    out = ops.draw_instances(rgba.permute(0, 3, 1, 2)[:, :3], bits, stats=stats, focus=Fp, style=style, outline_px=3, out=rgba.permute(0, 3, 1, 2)[:, :3])
    assert out.data_ptr() == rgba.data_ptr() and np.array_equal(rgba[..., :3].permute(0, 3, 1, 2).cpu().numpy(), want) and bool((rgba[..., 3] == 255).all())
    assert torch.equal(U, U0)


@pytest.mark.gpu
def test_session_render_follows_the_record(served):
    module, calls, TP = served
    PAD = 16

    def frames(windows):
        out = [M.window(M.canvas(seed, SIZE + 2 * PAD, SIZE + 2 * PAD, 4), y, x, SIZE, SIZE) for seed, y, x in windows]
        return _bytes_of(torch.from_numpy(np.stack(out)).cuda())

    focus = lambda pixels: torch.tensor([[py / (SIZE - 1), px / (SIZE - 1)] for py, px in pixels], dtype=torch.float32, device="cuda")
    U1, F1 = frames([(25, PAD, PAD), (31, PAD, PAD)]), focus([(128, 128), (100, 140)])
    U2, F2 = frames([(25, PAD - 3, PAD + 5), (31, PAD, PAD)]), focus([(131, 123), (100, 140)])       # the content moves by (3, -5)
    s = GazeSession(module, 2, (SIZE, SIZE), motion_px=5)
    with pytest.raises(RuntimeError):
        s.render(U1)
    style = ops.overlay_style(tint=(0, 200, 255), alpha=100, outline=(255, 0, 0), box=(0, 255, 0), box_px=1, marker=(255, 255, 255), marker_px=4,
                              marker_width=1, dim=128, device="cuda")

    def want(U, Fp, d, live=(1, 1)):
        b = s._rec[3].cpu().numpy()
        return O.draw_planes(U.cpu().numpy(), b, band=_band_words(b, SIZE, d) if d else None, stats=s._rec[1].cpu().numpy(), focus=Fp.cpu().numpy(),
                             live=np.array(live, dtype=np.int64), style=style.cpu().numpy())

    *rec, gate, motion = s.step(U1, F1)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2
    assert np.array_equal(s.render(U1, focus=F1, style=style, outline_px=2).cpu().numpy(), want(U1, F1, 2))
    *rec, gate, motion = s.step(U1, F1)
    assert gate[:, 0].tolist() == [R.REUSE] * 2
    out = torch.empty_like(U1)
    assert s.render(U1, focus=F1, style=style, out=out) is out and np.array_equal(out.cpu().numpy(), want(U1, F1, 0))
    held = s._rec[3].clone()
    *rec, gate, motion = s.step(U2, F2)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and motion[:, :2].tolist() == [[3, -5], [0, 0]] and not torch.equal(held[0], s._rec[3][0])
    assert np.array_equal(s.render(U2, focus=F2, style=style, out=out, outline_px=2).cpu().numpy(), want(U2, F2, 2))      # the moved record
    # the second call allocates nothing: without an outline, and with the kept band buffers
    for d in (0, 2):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        s.render(U2, focus=F2, style=style, out=out, outline_px=d)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - base
        print(f"a second render with outline_px = {d} raised the peak by {grew} bytes")
        assert grew == 0
    s.render(U2, out=out)                                                                 # the default style is made once
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    s.render(U2, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base == 0
    s.reset([1])
    got = s.render(U2, focus=F2, style=style, outline_px=2).cpu().numpy()
    assert np.array_equal(got, want(U2, F2, 2, live=(1, 0)))
    empty = np.zeros_like(s._rec[3][1:].cpu().numpy())                                    # the reset viewer is drawn empty: marker and dim alone
    assert np.array_equal(got[1:], O.draw_planes(U2[1:].cpu().numpy(), empty, focus=F2[1:].cpu().numpy(), style=style.cpu().numpy()))
    # an interleaved frame, rendered in place
    rgba = torch.full((2, SIZE, SIZE, 4), 7, dtype=torch.uint8, device="cuda")
    rgba[..., :3] = U2.permute(0, 2, 3, 1)
    view = rgba.permute(0, 3, 1, 2)[:, :3]
    s.render(view, focus=F2, style=style, outline_px=2, out=view)
    assert np.array_equal(view.cpu().numpy(), got) and bool((rgba[..., 3] == 255).all())
