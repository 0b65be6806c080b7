"""Of an image's annotated instances, the one under the gaze, in plain numpy on dense masks: a double loop, images outside, candidates
inside, restated from the definition of include/fovealseg.h (fs_mask_candidates; UNPINNED: the reference chooses an annotation and
puts the gaze inside it, b2_preprocess_lvis.py:258-333, and has nothing that goes the other way).  Python integers throughout, so
the comparison of two IoUs is exact.  tests/test_mask_candidates.py holds this file to hand-derived answers first.  Not a test module."""
import math

import numpy as np

OFF2 = 2 ** 62                                           # snap_px = None: no distance rejects


def gaze(f, side):
    """The gaze coordinate in 1/16-pixel units: clamp(rint((double)f * ((side - 1) * 16)), 0, (side - 1) * 16), NaN -> 0, f an fp32."""
    f = float(np.float32(f))
    top = (side - 1) * 16
    if math.isnan(f):
        return 0
    v = f * float(top)                                   # one fp64 product
    if math.isinf(v):
        return top if v > 0 else 0
    return int(min(max(np.rint(v), 0.0), float(top)))    # half to even


def gaze_pixel(focus, Hs, Ws):
    return (gaze(focus[0], Hs) + 8) >> 4, (gaze(focus[1], Ws) + 8) >> 4


def snap2_of(snap_px):
    return OFF2 if snap_px is None else int(math.floor(float(snap_px) ** 2))


def nearest(mask, py, px):
    """(d2, y, x) of the set pixel minimising key = d2 * 2^31 + (y * Ws + x), or (-1, -1, -1) for an empty mask."""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return -1, -1, -1
    d2 = (ys.astype(np.int64) - py) ** 2 + (xs.astype(np.int64) - px) ** 2
    i = int(np.argmin(d2 * 2 ** 31 + (ys.astype(np.int64) * mask.shape[1] + xs)))
    return int(d2[i]), int(ys[i]), int(xs[i])


def offsets_valid(cand_off, N):
    off = [int(v) for v in cand_off]
    return off[0] == 0 and off[-1] == N and all(a <= b for a, b in zip(off, off[1:]))


def overlap_before(a, b):
    """a = (inter, union, area, n) goes before b: the greater inter / union, compared exactly by cross-multiplication in Python
    integers, then the smaller area, then the smaller row."""
    l, r = a[0] * b[1], b[0] * a[1]
    return l > r if l != r else (a[2], a[3]) < (b[2], b[3])


def candidates(masks, cand_off, focus, pred=None, cand_cat=None, snap2=OFF2):
    """masks (N, Hs, Ws), non-zero = set; cand_off (B + 1,); focus (B, 2); pred (B, Hs, Ws) or None; cand_cat (N,) or None.
    Returns (gmask (B, Hs, Ws) bool, sel (B, 8) int64, cand (N, 6) int64) as fs_mask_candidates defines them."""
    m = np.asarray(masks) != 0
    N, Hs, Ws = m.shape
    B = len(cand_off) - 1
    gmask = np.zeros((B, Hs, Ws), dtype=bool)
    sel = np.zeros((B, 8), dtype=np.int64)
    cand = np.zeros((N, 6), dtype=np.int64)
    if not offsets_valid(cand_off, N):
        for n in range(N):
            cand[n] = [-1, int(m[n].sum()), 0, -1, -1, -1]
        sel[:] = [-1, -1, -1, 0, 0, 0, -1, 1]
        return gmask, sel, cand
    for b in range(B):
        py, px = gaze_pixel(focus[b], Hs, Ws)
        p = None if pred is None else np.asarray(pred[b]) != 0
        parea = 0 if p is None else int(p.sum())
        pick, best, hits = None, None, 0                 # pick = (d2, area, n); best = (inter, union, area, n)
        for n in range(int(cand_off[b]), int(cand_off[b + 1])):
            area = int(m[n].sum())
            inter = 0 if p is None else int((m[n] & p).sum())
            d2, ny, nx = nearest(m[n], py, px)
            cand[n] = [b, area, inter, d2, ny, nx]
            if area == 0:
                continue
            hits += bool(m[n, py, px])
            assert bool(m[n, py, px]) == (d2 == 0)
            if d2 <= snap2 and (pick is None or (d2, area, n) < pick[:3]):
                pick = (d2, area, n, inter)
            if inter > 0:
                mine = (inter, area + parea - inter, area, n)
                if best is None or overlap_before(mine, best):
                    best = mine
        if pick is None:
            sel[b] = [-1, -1, -1, 0, 0, hits, -1 if best is None else best[3], 0]
        else:
            d2, area, n, inter = pick
            sel[b] = [n, -1 if cand_cat is None else int(cand_cat[n]), d2, area, inter, hits, -1 if best is None else best[3], 0]
            gmask[b] = m[n]
    return gmask, sel, cand


def outcome(row, lo, hi, cand):
    """What an image's sel row shows, as one of the six outcomes the tests must reach: 'none' (no candidate), 'empty' (candidates,
    all empty), 'one' / 'several' (contained by one / by several), 'snapped' (selected at d2 > 0), 'beyond' (non-empty candidates,
    none within snap2)."""
    if lo == hi:
        return "none"
    if all(int(cand[n][1]) == 0 for n in range(lo, hi)):
        return "empty"
    if row[0] < 0:
        return "beyond"
    if row[2] > 0:
        return "snapped"
    return "one" if row[5] == 1 else "several"
