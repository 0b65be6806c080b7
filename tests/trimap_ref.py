"""The trimap boundary accuracy of eval.py:41-67 restated in numpy, for tests/test_trimap.py.

The reference normalises the label to 0..255, takes PIL's FIND_EDGES of it and dilates the result 2**i times with scipy's default cross
element.  Restated without either library:
  seeds   FIND_EDGES is the kernel 8*centre - sum(8 neighbours), clipped to 0..255, so a pixel is marked where it holds the LARGER label
          value and a neighbour the smaller one.  On this path the larger value is the background class K - 1: a seed is a background
          pixel (t = trunc(y) == 0) with a foreground 8-neighbour.  PIL copies the outer one-pixel ring through unfiltered, where every
          non-zero (= background) pixel then counts (`frame=True`); `frame=False` applies the neighbour rule on the ring too, pixels
          outside the image being background.
  bands   n dilations by the cross element reach exactly the pixels within city-block distance n of a seed.  The L1 distance separates
          into a pass of prefix / suffix minima along the columns and one along the rows.  Band i = {d <= 2**i}; the band index of a
          pixel is the smallest such i <= D, 255 if there is none.
  counts  per band: the pixels in it, those with pred == gt, those with (pred == K-1) == (gt == K-1).
tests/golden/g18_trimap.npz holds what PIL and scipy themselves give (tests/golden/make_trimap_golden.py)."""
import numpy as np

INF = 1 << 20


def seeds(t, frame=True):
    """t (H,W) integer mask, non-zero = foreground -> bool (H,W) boundary seeds."""
    fg = np.asarray(t) != 0
    H, W = fg.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = fg
    nb = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            nb |= p[dy:dy + H, dx:dx + W]
    s = ~fg & nb
    if frame:
        ring = np.zeros((H, W), bool)
        ring[0] = ring[-1] = True
        ring[:, 0] = ring[:, -1] = True
        s = np.where(ring, ~fg, s)
    return s


def _pass(a, axis):
    a = np.moveaxis(a, axis, -1)
    j = np.arange(a.shape[-1])
    fwd = np.minimum.accumulate(a - j, axis=-1) + j
    bwd = np.minimum.accumulate((a + j)[..., ::-1], axis=-1)[..., ::-1] - j
    return np.moveaxis(np.minimum(fwd, bwd), -1, axis)


def l1_distance(seed):
    """bool (H,W) -> int64 (H,W) city-block distance to the nearest seed, >= INF without one."""
    g = np.where(seed, 0, INF).astype(np.int64)
    return _pass(_pass(g, 0), 1)


def band_index(t, D, frame=True):
    """uint8 (H,W): the smallest i <= D with d <= 2**i, 255 if none (fs_trimap_bands for one image)."""
    d = l1_distance(seeds(t, frame))
    out = np.full(d.shape, 255, np.uint8)
    for i in range(D, -1, -1):
        out[d <= 2 ** i] = i
    return out


def band_index_batch(y, D, frame=True):
    """y (B,H,W) float label masks, t = trunc(y) -> uint8 (B,H,W)."""
    y = np.asarray(y)
    return np.stack([band_index(np.trunc(y[b]).astype(np.int64), D, frame) for b in range(y.shape[0])])


def counters(pred, gt, bands, D, K):
    """pred, gt (B,H,W) integer class maps, bands (B,H,W) uint8 -> int64 (B, D+1, 3): total, cls_ok, bin_ok of every band."""
    pred, gt, bands = np.asarray(pred), np.asarray(gt), np.asarray(bands)
    out = np.zeros((pred.shape[0], D + 1, 3), np.int64)
    eq, same_side = pred == gt, (pred == K - 1) == (gt == K - 1)
    for i in range(D + 1):
        inb = bands <= i
        out[:, i, 0] = inb.sum((1, 2))
        out[:, i, 1] = (inb & eq).sum((1, 2))
        out[:, i, 2] = (inb & same_side).sum((1, 2))
    return out


def accuracies(trim):
    """(..., 3) counters -> (..., 2) float64: cls_ok / (total + 1e-10), bin_ok / (total + 1e-10) (eval.py:56)."""
    trim = np.asarray(trim).astype(np.float64)
    return trim[..., 1:] / (trim[..., :1] + 1e-10)
