"""The instance record of a mask in plain numpy: bit words, statistics and the uncompressed COCO run-length code, restated from the
definitions of include/fovealseg.h (fs_mask_bits, fs_mask_rle).  The format itself is restated from its published definition
(pycocotools' uncompressed RLE) and is unpinned: no copy of that library is at hand, so tests/test_instances.py holds this file to
hand-derived answers and to decode(encode(mask)) == mask."""
import numpy as np


def encode(mask):
    """(Hs, Ws) mask, non-zero = set -> the list of counts: v[p] = mask[y, x] at p = x * Hs + y, v[-1] = 0, the boundaries T = {p :
    v[p] != v[p-1]} ascending, counts = T[0], T[i] - T[i-1], N - T[last]."""
    m = np.asarray(mask) != 0
    Hs, Ws = m.shape
    v = m.T.reshape(-1).astype(np.int8)                  # column-major
    T = np.flatnonzero(np.diff(np.concatenate([[0], v])) != 0)
    edges = np.concatenate([[0], T, [Hs * Ws]])
    return np.diff(edges).tolist()


def decode(counts, Hs, Ws):
    """the inverse: runs of 0, 1, 0, ... laid out column-major -> (Hs, Ws) bool."""
    assert sum(counts) == Hs * Ws and all(c >= 0 for c in counts)
    v = np.zeros(Hs * Ws, dtype=bool)
    p, val = 0, False
    for c in counts:
        v[p:p + c] = val
        p, val = p + c, not val
    return v.reshape(Ws, Hs).T.copy()


def bits(mask):
    """(Hs, Ws) -> (Hs, ceil(Ws / 32)) int32: bit j of word i of row y is pixel x = 32 i + j, the bits at x >= Ws are 0."""
    m = np.asarray(mask) != 0
    Hs, Ws = m.shape
    P = (Ws + 31) // 32
    pad = np.zeros((Hs, P * 32), dtype=np.uint64)
    pad[:, :Ws] = m
    words = (pad.reshape(Hs, P, 32) << np.arange(32, dtype=np.uint64)).sum(2)
    return words.astype(np.uint32).view(np.int32)


def unbits(words, Ws):
    """bits' inverse: (Hs, P) int32 -> (Hs, Ws) bool; asserts the padding bits are clear."""
    w = np.asarray(words).view(np.uint32)
    m = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], -1).astype(bool)
    assert not m[:, Ws:].any()
    return m[:, :Ws]


def stats(mask):
    """[area, x0, y0, bw, bh, n_runs]: the set pixels, their COCO box (zeros for an empty mask), the length of the code."""
    m = np.asarray(mask) != 0
    n = len(encode(m))
    if not m.any():
        return [0, 0, 0, 0, 0, n]
    ys, xs = np.nonzero(m)
    return [int(m.sum()), int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1), n]


def counts_row(mask, cap):
    """fs_mask_rle's counts row: the first min(n_runs, cap) counts, zeros behind."""
    c = encode(mask)[:cap]
    return np.array(c + [0] * (cap - len(c)), dtype=np.int32)
