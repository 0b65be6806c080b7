"""The connected component under the gaze in plain numpy, restated from the definition of include/fovealseg.h (fs_mask_component;
unpinned: the reference has no counterpart).  The seed is chosen by the definition's key; the component itself is the textbook one
and comes from scipy.ndimage.label.  tests/test_component.py holds this file to hand-derived answers first.  Not a test module."""
import math

import numpy as np
from scipy import ndimage

OFF2 = 2 ** 62                                           # snap_px = None: no distance rejects
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
FULL = np.ones((3, 3), dtype=int)


def gaze(f, side):
    """The gaze coordinate in 1/16-pixel units: clamp(rint((double)f * ((side - 1) * 16)), 0, (side - 1) * 16), NaN -> 0, f an fp32."""
    f = float(np.float32(f))
    top = (side - 1) * 16
    if math.isnan(f):
        return 0
    v = f * float(top)                                   # one fp64 product, as the kernel's
    if math.isinf(v):
        return top if v > 0 else 0
    return int(min(max(np.rint(v), 0.0), float(top)))    # np.rint: half to even


def gaze_pixel(focus, Hs, Ws):
    return (gaze(focus[0], Hs) + 8) >> 4, (gaze(focus[1], Ws) + 8) >> 4


def snap2_of(snap_px):
    return OFF2 if snap_px is None else int(math.floor(float(snap_px) ** 2))


def seed(mask, py, px, snap2=OFF2):
    """(seed_y, seed_x, d2) of the set pixel minimising key = d2 * 2^31 + (y * Ws + x), or None (empty mask, or d2 > snap2)."""
    m = np.asarray(mask) != 0
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return None
    d2 = (ys.astype(np.int64) - py) ** 2 + (xs.astype(np.int64) - px) ** 2
    key = d2 * 2 ** 31 + (ys.astype(np.int64) * m.shape[1] + xs)
    i = int(np.argmin(key))
    if int(d2[i]) > snap2:
        return None
    return int(ys[i]), int(xs[i]), int(d2[i])


def component(mask, focus, conn=8, snap2=OFF2):
    """mask (Hs, Ws), non-zero = set; focus = (row, col) normalised.  Returns (component (Hs, Ws) bool, comp = [seed_y, seed_x, d2,
    area_all]); all False and [-1, -1, -1, area_all] where there is no component."""
    assert conn in (4, 8)
    m = np.asarray(mask) != 0
    Hs, Ws = m.shape
    py, px = gaze_pixel(focus, Hs, Ws)
    area = int(m.sum())
    s = seed(m, py, px, snap2)
    if s is None:
        return np.zeros_like(m), [-1, -1, -1, area]
    lab, _ = ndimage.label(m, structure=FULL if conn == 8 else CROSS)
    return lab == lab[s[0], s[1]], [s[0], s[1], s[2], area]


def component_batch(masks, focus, conn=8, snap2=OFF2):
    """(B, Hs, Ws), (B, 2) -> ((B, Hs, Ws) bool, (B, 4) int64)."""
    out = [component(m, f, conn, snap2) for m, f in zip(np.asarray(masks), np.asarray(focus))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int64)


def unpack(words, Ws):
    """(Hs, P) bit words -> (Hs, Ws) bool; the bits at x >= Ws are whatever they are and are not pixels."""
    w = np.asarray(words).view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], -1).astype(bool)[:, :Ws]


def pack(mask):
    """(Hs, Ws) -> (Hs, ceil(Ws / 32)) uint32, bit j of word i = pixel 32 i + j, the padding bits 0."""
    m = np.asarray(mask) != 0
    Hs, Ws = m.shape
    P = (Ws + 31) // 32
    pad = np.zeros((Hs, P * 32), dtype=np.uint64)
    pad[:, :Ws] = m
    return (pad.reshape(Hs, P, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def component_words(words, Ws, focus, conn=8, snap2=OFF2):
    """fs_mask_component on one image's bit words: (out (Hs, P) uint32, comp)."""
    c, rec = component(unpack(words, Ws), focus, conn, snap2)
    return pack(c), rec
