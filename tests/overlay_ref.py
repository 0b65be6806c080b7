"""The overlay pass by its definition (include/fovealseg.h "showing the record"; unpinned: the reference draws on the host), as a plain
double loop over pixels in numpy and Python integers, which cannot overflow: what tests/test_frame_overlay.py holds fs_frame_overlay /
_u8 / _hwc, fs_color_encode, ops.draw_instances and GazeSession.render to.  It is itself held to hand-derived answers first."""
import numpy as np

import gate_ref as R

STYLE_COLS = 20
MAX_PX = 16384


def style_row(tint=(0, 0, 0), a=0, outline=(0, 0, 0), dim=256, box=(0, 0, 0), t=0, marker=(0, 0, 0), r=0, w=0, flag=0):
    """One row of the style table, in the header's column order."""
    return [*tint, a, *outline, dim, *box, t, *marker, r, w, flag, 0, 0]


def clamp(v, hi):
    return min(max(int(v), 0), hi)


def codes(img):
    """(B,3,H,W) integer pixel codes of a planar source: q of fp32 values, the bytes themselves."""
    img = np.asarray(img)
    return R.q(img) if img.dtype == np.float32 else img.astype(np.int64)


def gaze_pixel(f, side):
    return (R.gaze(f, side) + 8) >> 4


def draw(src, bits, band=None, stats=None, focus=None, live=None, style=None):
    """src (B,3,H,W) fp32 or uint8, planar; bits, band (B,H,P) bit words (any integer dtype of 32 bits); stats (B,6) int64; focus (B,2);
    live (B,) ; style (S,20) -> out (B,3,H,W) uint8.  A None is the kernel's null pointer."""
    s = codes(src)
    B, _, H, W = s.shape
    style = np.asarray(style, dtype=np.int64)
    S = style.shape[0]
    assert S in (1, B) and style.shape[1] == STYLE_COLS
    words = np.asarray(bits).view(np.uint32).reshape(B, H, -1)
    bwords = None if band is None else np.asarray(band).view(np.uint32).reshape(B, H, -1)
    out = np.zeros((B, 3, H, W), dtype=np.uint8)
    for b in range(B):
        st = [int(v) for v in style[0 if S == 1 else b]]
        tint = [clamp(v, 255) for v in st[0:3]]
        a = clamp(st[3], 256)
        line = [clamp(v, 255) for v in st[4:7]]
        dim = clamp(st[7], 256)
        boxc = [clamp(v, 255) for v in st[8:11]]
        t = clamp(st[11], MAX_PX)
        mark = [clamp(v, 255) for v in st[12:15]]
        r, w = clamp(st[15], MAX_PX), clamp(st[16], MAX_PX)
        flag = st[17] != 0
        alive = live is None or int(live[b]) != 0
        if focus is not None:
            py, px = gaze_pixel(focus[b][0], H), gaze_pixel(focus[b][1], W)
        if stats is not None:
            x0, y0, bw, bh = (int(v) for v in np.asarray(stats)[b][1:5])
        for y in range(H):
            for x in range(W):
                bit = alive and (int(words[b, y, x >> 5]) >> (x & 31)) & 1
                bnd = alive and flag and bwords is not None and (int(bwords[b, y, x >> 5]) >> (x & 31)) & 1
                c = None
                if focus is not None and r > 0:
                    d2 = (y - py) ** 2 + (x - px) ** 2
                    if d2 <= r * r and d2 >= max(r - w, 0) ** 2:
                        c = mark
                if c is None and stats is not None and alive and t > 0 and bw > 0 and bh > 0 and x0 <= x < x0 + bw and y0 <= y < y0 + bh:
                    if x - x0 < t or x0 + bw - 1 - x < t or y - y0 < t or y0 + bh - 1 - y < t:
                        c = boxc
                if c is None and bnd:
                    c = line
                if c is None and bit:
                    c = [(int(s[b, ch, y, x]) * (256 - a) + tint[ch] * a + 128) >> 8 for ch in range(3)]
                if c is None:
                    c = [(int(s[b, ch, y, x]) * dim + 128) >> 8 for ch in range(3)]
                out[b, :, y, x] = c
    return out


def unbits(words, W):
    """(..., H, P) bit words -> (..., H, W) bool."""
    w = np.asarray(words).view(np.uint32)
    x = np.arange(W)
    return ((w[..., x >> 5] >> (x & 31).astype(np.uint32)) & 1).astype(bool)


def draw_planes(src, bits, band=None, stats=None, focus=None, live=None, style=None):
    """draw() with whole planes instead of the double loop, for the frames of the composed tests (256 x 256), where the loop takes
    seconds.  Held equal to draw() on random small cases by the CPU tests; int64 planes, and the box in Python integers a viewer."""
    s = codes(src)
    B, _, H, W = s.shape
    style = np.asarray(style, dtype=np.int64)
    S = style.shape[0]
    out = np.zeros((B, 3, H, W), dtype=np.uint8)
    y, x = np.mgrid[:H, :W]
    for b in range(B):
        st = [int(v) for v in style[0 if S == 1 else b]]
        col = lambda i: np.array([clamp(v, 255) for v in st[i:i + 3]], dtype=np.int64)[:, None, None]
        a, dim, t = clamp(st[3], 256), clamp(st[7], 256), clamp(st[11], MAX_PX)
        r, w = clamp(st[15], MAX_PX), clamp(st[16], MAX_PX)
        alive = live is None or int(live[b]) != 0
        bit = unbits(bits[b], W) & alive
        o = np.where(bit[None], (s[b] * (256 - a) + col(0) * a + 128) >> 8, (s[b] * dim + 128) >> 8)
        if band is not None and alive and st[17] != 0:
            o = np.where(unbits(band[b], W)[None], col(4), o)
        if stats is not None and alive and t > 0:
            x0, y0, bw, bh = (int(v) for v in np.asarray(stats)[b][1:5])
            if bw > 0 and bh > 0:
                xin = np.array([x0 <= v < x0 + bw for v in range(W)])[None, :]
                yin = np.array([y0 <= v < y0 + bh for v in range(H)])[:, None]
                xe = np.array([v - x0 < t or x0 + bw - 1 - v < t for v in range(W)])[None, :]
                ye = np.array([v - y0 < t or y0 + bh - 1 - v < t for v in range(H)])[:, None]
                o = np.where((xin & yin & (xe | ye))[None], col(8), o)
        if focus is not None and r > 0:
            d2 = (y - gaze_pixel(focus[b][0], H)) ** 2 + (x - gaze_pixel(focus[b][1], W)) ** 2
            o = np.where(((d2 <= r * r) & (d2 >= max(r - w, 0) ** 2))[None], col(12), o)
        out[b] = o
    return out


def color_encode(labels, palette):
    """labels (B,H,W) integers, palette (K,3) uint8 -> (B,3,H,W) uint8: palette[label], black for a label outside 0 .. K-1."""
    labels = np.asarray(labels)
    palette = np.asarray(palette, dtype=np.uint8)
    B, H, W = labels.shape
    out = np.zeros((B, 3, H, W), dtype=np.uint8)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                l = int(labels[b, y, x])
                if 0 <= l < palette.shape[0]:
                    out[b, :, y, x] = palette[l]
    return out


def place(planar, ob, oy, ox, buf):
    """planar (B,3,H,W) bytes written into the flat byte buffer buf (a copy is returned) as the destination (ob, oy, ox) lays them out."""
    B, _, H, W = planar.shape
    buf = np.array(buf, dtype=np.uint8, copy=True)
    b, c, y, x = np.meshgrid(np.arange(B), np.arange(3), np.arange(H), np.arange(W), indexing="ij")
    at = b * ob + c * H * W + y * W + x if ox == 1 else b * ob + y * oy + x * ox + c
    assert len(np.unique(at)) == at.size                # every byte has one writer
    buf[at] = planar
    if ox == 4:
        buf[(b * ob + y * oy + x * ox + 3)[:, 0]] = 255
    return buf
