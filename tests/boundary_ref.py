"""Erosion by a square, the boundary band and the pair counters of mask IoU / Boundary IoU in plain numpy, restated from the
definitions of include/fovealseg.h (fs_mask_erode, fs_mask_pair_counts; unpinned: the reference has no counterpart; Boundary IoU is
Cheng et al., CVPR 2021).  tests/test_instance_eval.py holds this file to hand-derived answers and to scipy first.  Not a test module."""
import math

import numpy as np

from component_ref import pack, unpack  # noqa: F401  (the bit-word layout is fs_mask_bits', restated once)


def dilation(Hs, Ws, ratio=0.02):
    """d = max(1, int(round(ratio * sqrt(Hs^2 + Ws^2)))) in Python floats (round: half to even)."""
    return max(1, int(round(ratio * math.sqrt(Hs * Hs + Ws * Ws))))


def erode(mask, d):
    """E_d(m)[y,x] = 1 iff every pixel of the (2d+1) x (2d+1) square centred on (y,x) is set; outside the image counts as unset.
    A window AND over a zero-padded copy, along x then along y (the square is the product of the two runs)."""
    m = np.asarray(mask) != 0
    Hs, Ws = m.shape
    pad = np.zeros((Hs + 2 * d, Ws + 2 * d), dtype=bool)
    pad[d:d + Hs, d:d + Ws] = m
    rows = np.ones((Hs + 2 * d, Ws), dtype=bool)
    for s in range(2 * d + 1):
        rows &= pad[:, s:s + Ws]
    out = np.ones((Hs, Ws), dtype=bool)
    for s in range(2 * d + 1):
        out &= rows[s:s + Hs]
    return out


def band(mask, d):
    """The boundary band m & ~E_d(m): the set pixels within d (chessboard) of an unset pixel or of the image's outside."""
    m = np.asarray(mask) != 0
    return m & ~erode(m, d)


def pair_counts(p, g, d):
    """[|p & g|, |p|, |g|, |band(p) & band(g)|, |band(p)|, |band(g)|] as Python ints."""
    p, g = np.asarray(p) != 0, np.asarray(g) != 0
    bp, bg = band(p, d), band(g, d)
    return [int((p & g).sum()), int(p.sum()), int(g.sum()), int((bp & bg).sum()), int(bp.sum()), int(bg.sum())]


def pair_batch(P, G, d):
    return np.array([pair_counts(p, g, d) for p, g in zip(P, G)], dtype=np.int64)


def scores(pair):
    """(iou, biou) of one row of counters as Python floats; a measure whose union is 0 is 0."""
    n, a, b, bn, ba, bb = (int(v) for v in pair)
    u, bu = a + b - n, ba + bb - bn
    return (n / u if u > 0 else 0.0), (bn / bu if bu > 0 else 0.0)
