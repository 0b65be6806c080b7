"""Global motion compensation in front of the gaze gate, restated in numpy (tests/test_gaze_motion.py).  Not a test module.

The definitions are those of include/fovealseg.h (fs_frame_profiles, fs_key_profiles, fs_profile_shift, fs_state_shift,
fs_motion_commit), written the slow and obvious way: Python loops over viewers, shifts and pixels, Python integers for everything that
is an integer.  The reference has no counterpart (unpinned), so the CPU tests hold this file to hand-derived answers and the GPU tests
hold the kernels to this file."""
import numpy as np

import gate_ref as G
import rle_ref as RLE


def luma(img):
    """L (B,H,W) int64 = q_r + q_g + q_b of fp32 frames (B,3,H,W)."""
    return G.q(img).sum(axis=1)


def profiles(L):
    """prof (B, H + W) int64 of luma codes (B,H,W): the row sums, then the column sums."""
    L = np.asarray(L).astype(np.int64)
    return np.concatenate([L.sum(axis=2), L.sum(axis=1)], axis=1)


def frame_profiles(img):
    return profiles(luma(img))


def key_profiles(key):
    return profiles(np.asarray(key).astype(np.int64).sum(axis=1))


def cost(P, K, s, R):
    """sum_{i=R}^{n-1-R} |P[i] - K[i - s]| as a Python integer."""
    n = len(P)
    return sum(abs(int(P[i]) - int(K[i - s])) for i in range(R, n - R))


def axis_shift(P, K, R, gain):
    """(shift taken, least cost, cost(0)) of one axis: ties go to the smaller |s|, then to the negative s; the best shift is taken only
    if cost * 8 <= cost(0) * gain."""
    zero = cost(P, K, 0, R)
    best, s_best = zero, 0
    for a in range(1, R + 1):
        for s in (-a, a):
            c = cost(P, K, s, R)
            if c < best:
                best, s_best = c, s
    return (s_best if best * 8 <= zero * gain else 0), best, zero


def profile_shift(prof, prof_key, gstate, H, W, R, gain):
    """shift (B,4) int64 = (dy, dx, cost_best, cost_zero); zeros for a viewer with valid == 0."""
    assert 1 <= R <= 255 and 4 * R < min(H, W) and 0 <= gain <= 8
    B = prof.shape[0]
    out = np.zeros((B, 4), dtype=np.int64)
    for b in range(B):
        if int(gstate[b, 0]) == 0:
            continue
        dy, by, zy = axis_shift(prof[b, :H], prof_key[b, :H], R, gain)
        dx, bx, zx = axis_shift(prof[b, H:], prof_key[b, H:], R, gain)
        out[b] = (dy, dx, by + bx, zy + zx)
    return out


def move_key(key_b, img_b, dy, dx):
    """key'[c,y,x] = key[c,y-dy,x-dx] where that lies in the frame, else q(img[c,y,x]); one viewer, (3,H,W)."""
    _, H, W = key_b.shape
    fill = G.q(img_b).astype(np.uint8)
    out = np.empty_like(key_b)
    for y in range(H):
        for x in range(W):
            sy, sx = y - dy, x - dx
            out[:, y, x] = key_b[:, sy, sx] if 0 <= sy < H and 0 <= sx < W else fill[:, y, x]
    return out


def move_mask(mask, dy, dx):
    """mask'[y,x] = mask[y-dy,x-dx], else False; one viewer, (H,W) bool."""
    H, W = mask.shape
    out = np.zeros_like(mask)
    for y in range(H):
        for x in range(W):
            sy, sx = y - dy, x - dx
            if 0 <= sy < H and 0 <= sx < W:
                out[y, x] = mask[sy, sx]
    return out


def move_gaze(g, d, side):
    return min(max(int(g) + 16 * int(d), 0), (side - 1) * 16)


def state_shift(img, shift, key, bits, gstate, stats, counts, prof_key, mstate):
    """The state after the move, as new arrays: (key, bits, gstate, stats, counts, prof_key, mstate, motion).  bits (B,H,P) int32 as
    fs_mask_bits lays them out; a still viewer's rows are the old ones."""
    B, _, H, W = img.shape
    cap = counts.shape[1]
    key, bits, gstate, stats, counts = key.copy(), bits.copy(), gstate.copy(), stats.copy(), counts.copy()
    prof_key, mstate = prof_key.copy(), mstate.copy()
    motion = np.zeros((B, 6), dtype=np.int64)
    for b in range(B):
        dy, dx = int(shift[b, 0]), int(shift[b, 1])
        if (dy, dx) != (0, 0):
            key[b] = move_key(key[b], img[b], dy, dx)
            mask = move_mask(RLE.unbits(bits[b], W), dy, dx)
            bits[b] = RLE.bits(mask)
            gstate[b, 1], gstate[b, 3] = move_gaze(gstate[b, 1], dy, H), move_gaze(gstate[b, 3], dy, H)
            gstate[b, 2], gstate[b, 4] = move_gaze(gstate[b, 2], dx, W), move_gaze(gstate[b, 4], dx, W)
            stats[b] = RLE.stats(mask)
            counts[b] = RLE.counts_row(mask, cap)
            prof_key[b] = key_profiles(key[b:b + 1])[0]
            mstate[b] += (dy, dx, 1, abs(dy) + abs(dx))
        motion[b] = (dy, dx, shift[b, 2], shift[b, 3], mstate[b, 0], mstate[b, 1])
    return key, bits, gstate, stats, counts, prof_key, mstate, motion


def motion_commit(idx, prof, prof_key, mstate):
    prof_key, mstate = prof_key.copy(), mstate.copy()
    for b in idx:
        prof_key[b] = prof[b]
        mstate[b] = 0
    return prof_key, mstate


def canvas(seed, H, W, scale):
    """A seeded texture (3,H,W) fp32 in [0, 1]: uniform noise box-filtered over scale x scale pixels, stretched to the full range."""
    rng = np.random.default_rng(seed)
    n = rng.random((3, H + scale, W + scale))
    c = np.cumsum(np.cumsum(np.pad(n, ((0, 0), (1, 0), (1, 0))), axis=1), axis=2)
    box = c[:, scale:scale + H, scale:scale + W] - c[:, :H, scale:scale + W] - c[:, scale:scale + H, :W] + c[:, :H, :W]
    box = (box - box.min()) / (box.max() - box.min())
    return box.astype(np.float32)


def window(canv, y, x, H, W):
    """The frame a camera at (y, x) sees.  A camera that moves by (+cy, +cx) moves the content by (-cy, -cx): the window at (y - dy,
    x - dx) shows the content of the window at (y, x) shifted by (dy, dx)."""
    return canv[:, y:y + H, x:x + W].copy()
