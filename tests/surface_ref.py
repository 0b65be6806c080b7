"""The Hausdorff percentile (HD95) between two 2-D masks, restated in integers with numpy: border, brute-force squared distances,
ranks, interpolation.  What fs_surface_hd / ops.surface_hd / evaluate(hausdorff=q) are tested against; tests/golden/g20_hd95.npz holds
what scipy's binary_erosion + distance_transform_edt and np.percentile give on the same pairs.  Not a test module."""
import numpy as np


def border(mask):
    """Foreground pixels with a background 4-neighbour; everything outside the image is background."""
    f = np.asarray(mask) != 0
    p = np.pad(f, 1, constant_values=False)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return f & ~inner


def nearest_d2(src, dst, chunk=2048):
    """For every pixel of the border map src, in row-major order, the squared distance to the nearest pixel of dst (int64)."""
    s, d = np.argwhere(src).astype(np.int64), np.argwhere(dst).astype(np.int64)
    if len(s) == 0 or len(d) == 0:
        return np.zeros(0, np.int64)
    out = np.empty(len(s), np.int64)
    for i in range(0, len(s), chunk):
        diff = s[i:i + chunk, None, :] - d[None, :, :]
        out[i:i + chunk] = (diff * diff).sum(2).min(1)
    return out


def ranks(n, q):
    """np.percentile's two ranks and the interpolation weight, in integers: (lo, hi, numerator of frac over 100)."""
    t = q * (n - 1)
    return t // 100, t // 100 + (t % 100 != 0), t % 100


def stats(a, b, q):
    """(n_a, n_b, d2_lo, d2_hi) as fs_surface_hd defines them; d2 = -1 where a border is empty."""
    ba, bb = border(a), border(b)
    na, nb = int(ba.sum()), int(bb.sum())
    if na == 0 or nb == 0:
        return np.array([na, nb, -1, -1], np.int64)
    pooled = np.sort(np.concatenate([nearest_d2(ba, bb), nearest_d2(bb, ba)]))
    lo, hi, _ = ranks(na + nb, q)
    return np.array([na, nb, pooled[lo], pooled[hi]], np.int64)


def stats_batch(a, b, q):
    return np.stack([stats(x, y, q) for x, y in zip(a, b)])


def percentile(st, q):
    """The distance from one row of stats: sqrt and linear interpolation, the only floating-point steps; nan for an empty border."""
    na, nb, lo, hi = (int(v) for v in st)
    if na == 0 or nb == 0:
        return float("nan")
    frac = ranks(na + nb, q)[2] / 100.0
    return float(np.sqrt(np.float64(lo)) + (np.sqrt(np.float64(hi)) - np.sqrt(np.float64(lo))) * frac)
