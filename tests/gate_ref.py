"""The gaze gate restated in numpy (tests/test_gaze_session.py).  Not a test module.

The definitions are those of include/fovealseg.h (fs_gate_tiles, fs_gate_decide, fs_gate_commit), written the slow and obvious way:
Python loops over viewers and tiles, Python integers for everything that is an integer.  The reference has no counterpart (unpinned),
so the CPU tests hold this file to hand-derived answers and the GPU tests hold the kernels to this file."""
import numpy as np

REUSE, RUN_INIT, HOLD_SACCADE, RUN_SCENE, RUN_ROI, RUN_GAZE, RUN_AGE, RUN_FORCED = range(8)
RUNS = (RUN_INIT, RUN_SCENE, RUN_ROI, RUN_GAZE, RUN_AGE, RUN_FORCED)


def q(v):
    """The pixel code: (int) rintf(fminf(fmaxf(v, 0), 1) * 255.0f) -- one fp32 multiply, round to nearest even, NaN -> 0."""
    v = np.asarray(v, dtype=np.float32)
    c = np.where(np.isnan(v), np.float32(0), np.minimum(np.maximum(v, np.float32(0)), np.float32(1))).astype(np.float32)
    return np.rint(c * np.float32(255.0)).astype(np.int64)


def tiles(img, key, T):
    """sad (B,th,tw) int64: the sum of |q(img) - key| over 3 channels and the tile's pixels, the last tiles ragged."""
    d = np.abs(q(img) - np.asarray(key).astype(np.int64))
    B, _, H, W = d.shape
    th, tw = -(-H // T), -(-W // T)
    sad = np.zeros((B, th, tw), dtype=np.int64)
    for ty in range(th):
        for tx in range(tw):
            sad[:, ty, tx] = d[:, :, ty * T:(ty + 1) * T, tx * T:(tx + 1) * T].sum(axis=(1, 2, 3))
    return sad


def gaze(f, side):
    """One gaze coordinate in 1/16-pixel units: clamp(rint((double)f * ((side-1)*16)), 0, (side-1)*16), NaN -> 0."""
    top = (side - 1) * 16
    with np.errstate(invalid="ignore"):
        v = np.rint(np.float64(np.float32(f)) * np.float64(top))
    if np.isnan(v):
        return 0
    return int(min(max(v, 0.0), float(top)))


def d2(ay, ax, by, bx):
    return (ay - by) ** 2 + (ax - bx) ** 2


def thr2(px):
    """A distance in pixels as a squared threshold in 1/16-pixel units, computed on the host."""
    return int(np.floor((float(px) * 16.0) ** 2))


def bit(bits_row, py, px):
    """Bit (py, px) of one viewer's bit words (H,P) as fs_mask_bits lays them out."""
    return int((int(np.asarray(bits_row).view(np.uint32)[py, px >> 5]) >> (px & 31)) & 1)


def roi_tiles(stat, py, px, H, W, T, margin):
    """The set of (ty, tx) in the region of interest: tiles meeting the box grown by margin and clipped, plus the gaze pixel's tile."""
    out = {(py // T, px // T)}
    area, x0, y0, bw, bh = (int(v) for v in stat[:5])
    if area != 0:
        bx0, bx1 = max(x0 - margin, 0), min(x0 + bw + margin, W)
        by0, by1 = max(y0 - margin, 0), min(y0 + bh + margin, H)
        if bx0 < bx1 and by0 < by1:
            out |= {(ty, tx) for ty in range(by0 // T, (by1 - 1) // T + 1) for tx in range(bx0 // T, (bx1 - 1) // T + 1)}
    return out


def decide(sad, gstate, focus, stats, bits, force, H, W, T, level, scene_tiles, roi_tiles_tol, margin, saccade2, fixation2, max_age, inside_on):
    """gate (B,8) int64 = (code, n_changed, n_roi_changed, sad_total, d2_key, d2_prev, inside_bit, age + 1)."""
    B, th, tw = sad.shape
    gate = np.zeros((B, 8), dtype=np.int64)
    for b in range(B):
        gy, gx = gaze(focus[b, 0], H), gaze(focus[b, 1], W)
        py, px = (gy + 8) >> 4, (gx + 8) >> 4
        roi = roi_tiles(stats[b], py, px, H, W, T, margin)
        nc = nr = tot = 0
        for ty in range(th):
            for tx in range(tw):
                n_el = 3 * min(T, H - ty * T) * min(T, W - tx * T)
                s = int(sad[b, ty, tx])
                tot += s
                if s > level * n_el:
                    nc += 1
                    nr += (ty, tx) in roi
        valid, gyk, gxk, gyp, gxp, age = (int(v) for v in gstate[b])
        dk, dp = d2(gy, gx, gyk, gxk), d2(gy, gx, gyp, gxp)
        inside = bit(bits[b], py, px)
        if force is not None and int(force[b]) != 0:
            code = RUN_FORCED
        elif valid == 0:
            code = RUN_INIT
        elif dp > saccade2:
            code = HOLD_SACCADE
        elif nc > scene_tiles:
            code = RUN_SCENE
        elif nr > roi_tiles_tol:
            code = RUN_ROI
        elif not (inside_on and inside) and dk > fixation2:
            code = RUN_GAZE
        elif max_age > 0 and age + 1 > max_age:
            code = RUN_AGE
        else:
            code = REUSE
        gate[b] = (code, nc, nr, tot, dk, dp, inside, age + 1)
    return gate


def commit(img, idx, key, gstate, focus, src, dst):
    """The state after a step, as new arrays: (key, gstate, dst).  idx ascending; row j of every src array goes to row idx[j]."""
    key, gstate, dst = key.copy(), gstate.copy(), [d.copy() for d in dst]
    _, _, H, W = img.shape
    ran = {int(b): j for j, b in enumerate(idx)}
    for b in range(img.shape[0]):
        gy, gx = gaze(focus[b, 0], H), gaze(focus[b, 1], W)
        if b in ran:
            key[b] = q(img[b]).astype(np.uint8)
            gstate[b, 0], gstate[b, 1], gstate[b, 2], gstate[b, 5] = 1, gy, gx, 0
            for s, d in zip(src, dst):
                d[b] = s[ran[b]]
        else:
            gstate[b, 5] += 1
        gstate[b, 3], gstate[b, 4] = gy, gx
    return key, gstate, dst
