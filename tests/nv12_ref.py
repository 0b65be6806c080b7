"""NV12 frames in plain numpy, restated from the definition of include/fovealseg.h ("frames as NV12"; UNPINNED: the reference reads image
files only, so tests/test_frames_nv12.py holds this file to hand-derived answers before it holds the kernels to this file).

Layout: the luma byte of (b, y, x) is yp[b * sb + y * sy + x]; its chroma is (U, V) = uvp[b * ub + (y >> 1) * uy + 2 * (x >> 1) + (0, 1)], the
sample of the pixel's 2 x 2 block, replicated.  Colour: with C = Y - yo, D = U - 128, E = V - 128 and >> the floor shift,
    R = clamp((yg * C + rv * E + 128) >> 8), G = clamp((yg * C + gu * D + gv * E + 128) >> 8), B = clamp((yg * C + bu * D + 128) >> 8).
Written the slow and obvious way, in int64."""
import numpy as np

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}                      # (Kr, Kb)
# (yo, yg, rv, gu, gv, bu), as the definition lists them
TABLES = {("bt601", False): (16, 298, 409, -100, -208, 516), ("bt601", True): (0, 256, 359, -88, -183, 454),
          ("bt709", False): (16, 298, 459, -55, -136, 541), ("bt709", True): (0, 256, 403, -48, -120, 475)}


def real_coefficients(matrix, full_range):
    """(yo, luma gain, V -> R, U -> G, V -> G, U -> B) of the real conversion."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    ly, lc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    return (0 if full_range else 16, ly, lc * 2 * (1 - kr), -lc * 2 * (1 - kb) * kb / kg, -lc * 2 * (1 - kr) * kr / kg, lc * 2 * (1 - kb))


def csc(matrix, full_range):
    yo, *co = real_coefficients(matrix, full_range)
    return (yo,) + tuple(int(np.rint(256.0 * c)) for c in co)


def rgb_of(Y, U, V, table):
    """The RGB bytes of (Y, U, V), arrays of one shape -> three uint8 arrays."""
    yo, yg, rv, gu, gv, bu = (int(v) for v in table)
    C, D, E = np.asarray(Y, dtype=np.int64) - yo, np.asarray(U, dtype=np.int64) - 128, np.asarray(V, dtype=np.int64) - 128
    clamp = lambda v: np.clip(v >> 8, 0, 255).astype(np.uint8)                       # >> of a negative int64 floors
    return clamp(yg * C + rv * E + 128), clamp(yg * C + gu * D + gv * E + 128), clamp(yg * C + bu * D + 128)


def real_rgb_of(Y, U, V, matrix, full_range):
    """clip(rint(real formula)), what the integer tables approximate."""
    yo, ly, rv, gu, gv, bu = real_coefficients(matrix, full_range)
    C, D, E = np.asarray(Y, dtype=np.float64) - yo, np.asarray(U, dtype=np.float64) - 128, np.asarray(V, dtype=np.float64) - 128
    clip = lambda v: np.clip(np.rint(v), 0, 255).astype(np.int64)
    return clip(ly * C + rv * E), clip(ly * C + gu * D + gv * E), clip(ly * C + bu * D)


def to_rgb(y, uv, table):
    """y (B,H,W) and uv (B,ceil(H/2),ceil(W/2),2) uint8 arrays -> the planar frame (B,3,H,W) uint8."""
    B, H, W = y.shape
    assert uv.shape == (B, (H + 1) // 2, (W + 1) // 2, 2), (y.shape, uv.shape)
    j, i = np.arange(H) >> 1, np.arange(W) >> 1
    U, V = uv[:, j][:, :, i, 0], uv[:, j][:, :, i, 1]
    return np.stack(rgb_of(y, U, V, table), axis=1)


def frame_rgb(ybuf, uvbuf, sb, sy, ub, uy, B, H, W, table):
    """The planar frame of two flat byte buffers, pixel by pixel from the addresses of the definition."""
    out = np.empty((B, 3, H, W), dtype=np.uint8)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                Y = ybuf[b * sb + y * sy + x]
                at = b * ub + (y >> 1) * uy + 2 * (x >> 1)
                r, g, bl = rgb_of(Y, uvbuf[at], uvbuf[at + 1], table)
                out[b, :, y, x] = (r, g, bl)
    return out


def route(y_ptr, uv_ptr, sb, sy, ub, uy, W):
    """fs_nv12_frame_route: 1 the vector forms, 0 the one-pixel forms, -1 a description refused (the table aside)."""
    if not y_ptr or not uv_ptr or W < 1 or sy < W or uy < 2 * ((W + 1) // 2) or sb < 0 or ub < 0:
        return -1
    return 1 if W % 16 == 0 and all(v % 16 == 0 for v in (y_ptr, uv_ptr, sb, sy, ub, uy)) else 0
