"""NV12 frames read in place: ops.Nv12Frame, ops.nv12_csc, ops.nv12_from_surface, ops.nv12_to_rgb, fs_nv12_frame_route, fs_nv12_to_rgb,
fs_gaze_lowres_nv12_fwd, fs_grid_sample_nv12_fwd, fs_gate_tiles_nv12, fs_gate_commit_nv12, fs_frame_profiles_nv12, fs_state_shift_nv12,
fs_frame_overlay_nv12, and the frames that predict* / evaluate* / GazeSession.step / render take in a uint8 frame's place.

The RGB byte of every pixel of an NV12 frame is a fixed integer function of (Y, U, V) (include/fovealseg.h "frames as NV12"; unpinned: the
reference reads image files), that byte is the pixel's code and byte / 255 its value.  So every NV12 entry point must equal its planar
uint8 twin (tests/test_frames_u8.py holds those to the fp32 route, tests/gate_ref.py and tests/motion_ref.py) fed the converted frame,
bit for bit: every comparison is torch.equal / np.array_equal.  tests/nv12_ref.py restates the layout and the rule in numpy and is held to
hand-derived answers first.  The pitch padding and the gaps between planes and images hold random bytes; on the GPU the frame's buffers sit
between guard bands and are compared with their contents after the calls."""
import numpy as np
import pytest
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T
from fovealseg.session import GazeSession

import gate_ref as R
import motion_ref as M
import nv12_ref as N
import rle_ref as RLE
import session_ref as S
from test_gaze_session import Guarded, _GARB, _same, served                                                # noqa: F401  (served is a fixture)
from test_frames_u8 import floats, _bits32, _bytes_of, _peak_of, _state_of, SIZE, SEED

NV12_ENTRY_POINTS = ("fs_nv12_to_rgb", "fs_gaze_lowres_nv12_fwd", "fs_grid_sample_nv12_fwd", "fs_gate_tiles_nv12", "fs_gate_commit_nv12",
                     "fs_frame_profiles_nv12", "fs_state_shift_nv12", "fs_frame_overlay_nv12")
BT601 = N.TABLES[("bt601", False)]


# ------------------------------------------------------------------------------------------------------------------ the reference ---
def test_nv12_ref_gives_the_hand_derived_colours():
    """bt601 limited: black, white, mid grey, the three primaries as a limited-range encoder makes them, and the two corners of the
    (Y, U, V) cube, where the clamps and the floor shift of a negative sum act.  Worked out with pencil from the definition."""
    hand = {(16, 128, 128): (0, 0, 0), (235, 128, 128): (255, 255, 255), (126, 128, 128): (128, 128, 128), (81, 90, 240): (255, 0, 0),
            (145, 54, 34): (0, 255, 1), (41, 240, 110): (0, 0, 255), (0, 0, 0): (0, 135, 0), (255, 255, 255): (255, 125, 255)}
    for (Y, U, V), want in hand.items():
        assert tuple(int(c) for c in N.rgb_of(Y, U, V, BT601)) == want, (Y, U, V)
    # (145, 54, 34) by its sums: yg * C = 298 * 129 = 38442; R = (38442 - 38446 + 128) >> 8 = 0; G = (38442 + 7400 + 19552 + 128) >> 8 = 255;
    # B = (38442 - 38184 + 128) >> 8 = 386 >> 8 = 1.  (81, 90, 240): B = (19370 - 19608 + 128) >> 8 = -110 >> 8 = -1 -> 0: the shift floors.
    assert (-110 >> 8) == -1


def test_the_four_standard_tables_entry_for_entry():
    hand = {("bt601", False): (16, 298, 409, -100, -208, 516), ("bt601", True): (0, 256, 359, -88, -183, 454),
            ("bt709", False): (16, 298, 459, -55, -136, 541), ("bt709", True): (0, 256, 403, -48, -120, 475)}
    assert N.TABLES == hand
    for (matrix, full), want in hand.items():
        assert N.csc(matrix, full) == want and ops.nv12_csc(matrix, full) == want, (matrix, full)
        assert all(type(v) is int for v in ops.nv12_csc(matrix, full))
    assert ops.nv12_csc("bt709") == hand[("bt709", False)]                                # limited range is the default
    for bad in ("bt2020", None, 601):
        with pytest.raises(ValueError):
            ops.nv12_csc(bad)


def test_a_3_by_5_frame_shares_its_chroma_by_2_by_2_blocks():
    """H = 3, W = 5: two chroma rows of three pairs.  The table (0, 256, 256, 0, 0, 256) makes R = Y + (V - 128), G = Y, B = Y + (U - 128), so
    with chroma sample n = 1 .. 6 stored as (U, V) = (128 + n, 128 - n) the pixel reads R = Y - n, B = Y + n: the block it belongs to.  The
    last column and the last row have a sample to themselves."""
    table = (0, 256, 256, 0, 0, 256)
    y = np.array([[[100, 101, 102, 103, 104], [110, 111, 112, 113, 114], [120, 121, 122, 123, 124]]], dtype=np.uint8)
    uv = np.array([[[[129, 127], [130, 126], [131, 125]], [[132, 124], [133, 123], [134, 122]]]], dtype=np.uint8)
    want_r = [[99, 100, 100, 101, 101], [109, 110, 110, 111, 111], [116, 117, 117, 118, 118]]
    want_b = [[101, 102, 104, 105, 107], [111, 112, 114, 115, 117], [124, 125, 127, 128, 130]]
    got = N.to_rgb(y, uv, table)
    assert got.shape == (1, 3, 3, 5) and got[0, 0].tolist() == want_r and got[0, 1].tolist() == y[0].tolist() and got[0, 2].tolist() == want_b
    # the same frame from flat buffers with pitches of their own, by the addresses of the definition
    ybuf, uvbuf = np.full(3 * 7, 0xEE, dtype=np.uint8), np.full(2 * 9, 0xEE, dtype=np.uint8)
    for r in range(3):
        ybuf[r * 7:r * 7 + 5] = y[0, r]
    for j in range(2):
        uvbuf[j * 9:j * 9 + 6] = uv[0, j].reshape(-1)
    assert np.array_equal(N.frame_rgb(ybuf, uvbuf, 0, 7, 0, 9, 1, 3, 5, table), got)


def test_every_standard_table_stays_within_one_grey_level_of_the_real_formula():
    """Over all 2^24 (Y, U, V): |integer rule - clip(rint(real formula))| <= 1 in every channel (the definition's claim)."""
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for (matrix, full), table in N.TABLES.items():
        worst, differ = 0, np.zeros(3, dtype=np.int64)
        for Y in range(256):
            got, want = N.rgb_of(np.full_like(U, Y), U, V, table), N.real_rgb_of(np.full_like(U, Y), U, V, matrix, full)
            for c in range(3):
                d = np.abs(got[c].astype(np.int64) - want[c])
                worst = max(worst, int(d.max()))
                differ[c] += int((d != 0).sum())
        share = differ / float(1 << 24)
        print(f"{matrix} {'full' if full else 'limited'}: worst {worst}, share of triplets that differ R G B = {share.round(4).tolist()}")
        assert worst <= 1, (matrix, full, worst)
        assert share.max() <= 0.113, (matrix, full, share)


# ------------------------------------------------------------------------------------------------------------------ layouts --------
# name -> (luma pitch padding, chroma pitch padding, gap between images, one image for all viewers, luma pointer one byte off, one surface,
#          stays on the vector route)
LAYOUTS = {"tight": (0, 0, 0, False, False, False, True), "pitched": (16, 32, 48, False, False, False, True),
           "pitch5": (5, 3, 7, False, False, False, False), "off1": (0, 0, 0, False, True, False, False),
           "surface": (16, 16, 32, False, False, True, True), "sb0": (0, 0, 0, True, False, False, True)}


def random_planes(rng, B, H, W):
    return rng.integers(0, 256, (B, H, W)).astype(np.uint8), rng.integers(0, 256, (B, (H + 1) // 2, (W + 1) // 2, 2)).astype(np.uint8)


class Nv12:
    """Planes y (B,H,W) and uv (B,Hc,Wc,2) laid out in buffers of random bytes; .planar is what the planar twin is fed."""

    def __init__(self, y, uv, name, table=BT601, seed=0):
        ypad, cpad, gap, one, self.off, self.surface, vec = LAYOUTS[name]
        B, H, W = y.shape
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        self.B, self.H, self.W, self.table = B, H, W, tuple(table)
        nb = 1 if one else B
        rng = np.random.default_rng(1000 + seed)
        if self.surface:                                                    # luma rows, then chroma rows, one pitch, image after image
            pitch = -(-max(W, 2 * Wc) // 16) * 16 + ypad
            self.sy = self.uy = pitch
            self.uv_offset = H * pitch
            self.sb = self.ub = (H + Hc) * pitch + gap
            self.buf = rng.integers(0, 256, nb * self.sb).astype(np.uint8)
            self.ybuf, self.uvbuf = self.buf, self.buf[self.uv_offset:]
        else:
            self.sy, self.uy = W + ypad, 2 * Wc + cpad
            self.sb, self.ub = H * self.sy + gap, Hc * self.uy + 2 * gap
            self.ybuf = rng.integers(0, 256, nb * self.sb).astype(np.uint8)
            self.uvbuf = rng.integers(0, 256, nb * self.ub).astype(np.uint8)
        as_strided = np.lib.stride_tricks.as_strided
        as_strided(self.ybuf, shape=(nb, H, W), strides=(self.sb, self.sy, 1))[...] = y[:nb]
        as_strided(self.uvbuf, shape=(nb, Hc, Wc, 2), strides=(self.ub, self.uy, 2, 1))[...] = uv[:nb]
        self.y, self.uv = (np.repeat(y[:1], B, axis=0), np.repeat(uv[:1], B, axis=0)) if one else (y, uv)
        self.planar = N.to_rgb(self.y, self.uv, self.table)
        if one or B == 1:
            self.sb = self.ub = 0
        self.vec = vec and W % 16 == 0

    def guarded(self):
        """The buffers on the device between guard bands -> (luma, chroma) Guarded (one object twice for a surface)."""
        if self.surface:
            g = Guarded(self.buf.size, torch.uint8, body=torch.from_numpy(self.buf))
            return g, g
        return (Guarded(self.ybuf.size, torch.uint8, body=torch.from_numpy(self.ybuf), off=1 if self.off else 0),
                Guarded(self.uvbuf.size, torch.uint8, body=torch.from_numpy(self.uvbuf)))

    def pointers(self, g):
        return g[0].ptr, g[1].ptr + (self.uv_offset if self.surface else 0)

    def args(self, g):
        yp, up = self.pointers(g)
        want = N.route(yp, up, self.sb, self.sy, self.ub, self.uy, self.W)
        assert want == (1 if self.vec else 0), (want, self.vec)                           # the case runs the route it is there for
        assert hip.load().fs_nv12_frame_route(yp, up, self.sb, self.sy, self.ub, self.uy, self.W) == want
        return (yp, up, self.sb, self.sy, self.ub, self.uy) + self.table

    def frame(self, g):
        """The ops.Nv12Frame of the guarded buffers."""
        B, H, W = self.B, self.H, self.W
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        if self.surface:
            f = ops.nv12_from_surface(g[0].body, H, W, self.sy, self.uv_offset, None if B == 1 else self.sb, matrix=None, csc=self.table)
        else:
            y = g[0].body.as_strided((B, H, W), (self.sb, self.sy, 1))
            uv = g[1].body.as_strided((B, Hc, Wc, 2), (self.ub, self.uy, 2, 1))
            f = ops.Nv12Frame(y, uv, matrix=None, csc=self.table)
        # the pitch of a plane of one row is not looked at: the frame shows the tight one
        want = (self.sb, W if H == 1 else self.sy, self.ub, 2 * Wc if Hc == 1 else self.uy)
        assert f.strides == want and f.route() == (1 if self.vec else 0), (f.strides, want, f.route())
        return f

    def unchanged(self, g):
        ok = g[0].intact() and g[1].intact()
        if self.surface:
            return ok and torch.equal(g[0].body.cpu(), torch.from_numpy(self.buf))
        return ok and torch.equal(g[0].body.cpu(), torch.from_numpy(self.ybuf)) and torch.equal(g[1].body.cpu(), torch.from_numpy(self.uvbuf))


# ------------------------------------------------------------------------------------------------------------------ CPU ------------
def test_the_ctypes_table_binds_the_nv12_entry_points():
    frame = "ppllll" + "iiiiii"
    assert hip.SIGNATURES["fs_gaze_lowres_nv12_fwd"] == frame + hip.SIGNATURES["fs_gaze_lowres_u8_fwd"][1:]
    assert hip.SIGNATURES["fs_grid_sample_nv12_fwd"] == frame + hip.SIGNATURES["fs_grid_sample_hwc_fwd"][4:]
    assert hip.SIGNATURES["fs_gate_tiles_nv12"] == frame + hip.SIGNATURES["fs_gate_tiles_u8"][1:]
    assert hip.SIGNATURES["fs_gate_commit_nv12"] == frame + hip.SIGNATURES["fs_gate_commit_u8"][1:]
    assert hip.SIGNATURES["fs_frame_profiles_nv12"] == frame + hip.SIGNATURES["fs_key_profiles"][1:]
    assert hip.SIGNATURES["fs_state_shift_nv12"] == frame + hip.SIGNATURES["fs_state_shift_u8"][1:]
    assert hip.SIGNATURES["fs_frame_overlay_nv12"] == frame + hip.SIGNATURES["fs_frame_overlay_u8"][1:]
    assert hip.SIGNATURES["fs_nv12_to_rgb"] == frame + "plli" + "iii"
    assert hip.HOST_ONLY["fs_nv12_frame_route"] == ("l", "ppllll" + "i")
    assert all(name in hip.SIGNATURES for name in NV12_ENTRY_POINTS)


def _planes(B, H, W, ypitch=None, cpitch=None):
    """CPU views of a luma and a chroma buffer with the pitches asked for (tight by default)."""
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    sy, uy = ypitch or W, cpitch or 2 * Wc
    y = torch.zeros(B * H * sy, dtype=torch.uint8).as_strided((B, H, W), (H * sy, sy, 1))
    uv = torch.zeros(B * Hc * uy, dtype=torch.uint8).as_strided((B, Hc, Wc, 2), (Hc * uy, uy, 2, 1))
    return y, uv


def _route_cases(H=6, W=32):
    """((yp, uvp, sb, sy, ub, uy, W), route) by hand, on addresses that are only numbers: the function reads no memory."""
    Y, C = 4096, 8192
    ones = [((Y, C, H * W, W, 3 * W, W, W), 1),                                            # tight, aligned
            ((Y, C, H * 48, 48, 3 * 64, 64, W), 1),                                        # pitched, uy != sy
            ((Y, C, 0, W, 0, W, W), 1)]                                                    # one image for every viewer
    zeros = [((Y + 1, C, H * W, W, 3 * W, W, W), 0), ((Y, C + 2, H * W, W, 3 * W, W, W), 0),      # a pointer off
             ((Y, C, H * 37, 37, 3 * W, W, W), 0), ((Y, C, H * W, W, 3 * 40, 40, W), 0),          # a pitch off
             ((Y, C, H * W + 8, W, 3 * W, W, W), 0), ((Y, C, H * W, W, 3 * W + 8, W, W), 0),      # a gap of 8 between images
             ((Y, C, H * 24, 24, 3 * 24, 24, 24), 0),                                             # W % 16 != 0
             ((Y, C, 0, 7, 0, 8, 7), 0)]                                                          # odd W: the chroma row is 2 * ceil(W / 2) bytes
    bad = [((0, C, 0, W, 0, W, W), -1), ((Y, 0, 0, W, 0, W, W), -1), ((Y, C, 0, W - 1, 0, W, W), -1), ((Y, C, 0, W, 0, W - 1, W), -1),
           ((Y, C, -16, W, 0, W, W), -1), ((Y, C, 0, W, -16, W, W), -1), ((Y, C, 0, W, 0, W, 0), -1), ((Y, C, 0, 7, 0, 7, 7), -1)]
    return ones + zeros + bad


ROUTE_CASES = _route_cases()


def test_nv12_strides_of_stride_patterns_and_the_route_rule_of_nv12_ref():
    B, H, W = 3, 6, 32
    kw = dict(matrix="bt601")
    y, uv = _planes(B, H, W)
    f = ops.Nv12Frame(y, uv, **kw)
    assert f.strides == (H * W, W, 3 * W, W) and f.csc == BT601
    assert tuple(f.shape) == (B, 3, H, W) and f.dtype == torch.uint8 and f.device == y.device and f.is_cuda is False and f.dim() == 4
    assert f.numel() == B * 3 * H * W
    assert ops.Nv12Frame(*_planes(B, H, W, 48, 64), **kw).strides == (H * 48, 48, 3 * 64, 64)          # luma and chroma pitched differently
    assert ops.Nv12Frame(*_planes(B, 5, 7), **kw).strides == (35, 7, 3 * 8, 8)                       # odd sides: 3 chroma rows of 4 pairs
    # one image expanded over the batch in both planes
    one = ops.Nv12Frame(y[:1].expand(B, H, W), uv[:1].expand(B, 3, 16, 2), **kw)
    assert one.strides == (0, W, 0, W)
    # B = 1: the image steps are not looked at
    assert ops.nv12_frame_strides((1, H, W), (12345, W, 1), (1, 3, 16, 2), (777, W, 2, 1)) == (0, W, 0, W)
    assert ops.nv12_frame_strides((B, 1, W), (W, 999, 1), (B, 1, 16, 2), (W, 555, 2, 1)) == (W, W, W, W)      # one row: no pitch
    # the route rule as nv12_ref restates it; test_nv12_entry_points_reject_bad_arguments holds fs_nv12_frame_route to the same cases
    for args, want in ROUTE_CASES:
        assert N.route(*args) == want, args
    # overlapping images, sb = 0 with ub != 0, and the other way round
    assert ops.nv12_frame_strides((B, H, W), (H * W - 1, W, 1), (B, 3, 16, 2), (3 * W, W, 2, 1)) is None
    assert ops.nv12_frame_strides((B, H, W), (H * W, W, 1), (B, 3, 16, 2), (3 * W - 1, W, 2, 1)) is None
    assert ops.nv12_frame_strides((B, H, W), (0, W, 1), (B, 3, 16, 2), (3 * W, W, 2, 1)) is None
    assert ops.nv12_frame_strides((B, H, W), (H * W, W, 1), (B, 3, 16, 2), (0, W, 2, 1)) is None
    assert ops.nv12_frame_strides((B, H, W), (H * W, W - 1, 1), (B, 3, 16, 2), (3 * W, W, 2, 1)) is None        # rows that overlap
    assert ops.nv12_frame_strides((B, H, W), (H * W, W, 1), (B, 3, 16, 2), (3 * W, W - 2, 2, 1)) is None


def test_nv12_from_surface_builds_the_two_views():
    H, W, pitch = 5, 7, 16
    Hc = 3
    per = (H + Hc) * pitch
    buf = torch.arange(2 * per, dtype=torch.int64).to(torch.uint8)
    f = ops.nv12_from_surface(buf, H, W, pitch, H * pitch, per, matrix="bt709", full_range=True)
    assert tuple(f.shape) == (2, 3, H, W) and f.strides == (per, pitch, per, pitch) and f.csc == N.TABLES[("bt709", True)]
    assert f.y.data_ptr() == buf.data_ptr() and f.uv.data_ptr() == buf.data_ptr() + H * pitch
    assert int(f.y[1, 2, 3]) == (per + 2 * pitch + 3) % 256 and f.uv[1, 2, 3].tolist() == [(per + (H + 2) * pitch + 6) % 256, (per + (H + 2) * pitch + 7) % 256]
    # a surface that begins inside a larger allocation: the planes are counted from the surface's first byte
    part = ops.nv12_from_surface(buf[48:48 + per], H, W, pitch, H * pitch, matrix="bt601")
    assert part.y.data_ptr() == buf.data_ptr() + 48 and part.uv.data_ptr() == buf.data_ptr() + 48 + H * pitch
    assert int(part.uv[0, 1, 2, 1]) == (48 + (H + 1) * pitch + 5) % 256
    one = ops.nv12_from_surface(buf[:per], H, W, pitch, H * pitch, matrix="bt601")
    assert tuple(one.shape) == (1, 3, H, W) and one.strides == (0, pitch, 0, pitch)
    for bad in (dict(pitch=6), dict(uv_offset=H * pitch - 1), dict(batch_stride=per - 1)):
        a = dict(pitch=pitch, uv_offset=H * pitch, batch_stride=per)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.nv12_from_surface(buf, H, W, a["pitch"], a["uv_offset"], a["batch_stride"], matrix="bt601")
    with pytest.raises(ValueError):
        ops.nv12_from_surface(buf[:per - 10], H, W, pitch, H * pitch, matrix="bt601")                    # ends short of its last chroma pair
    with pytest.raises(ValueError):
        ops.nv12_from_surface(buf.float(), H, W, pitch, H * pitch, matrix="bt601")
    with pytest.raises(TypeError):
        ops.nv12_from_surface(buf, H, W, pitch, H * pitch)                                               # matrix has no default


def test_nv12_frame_refuses_before_any_launch():
    B, H, W = 2, 6, 10
    y, uv = _planes(B, H, W)
    kw = dict(matrix="bt601")
    with pytest.raises(TypeError):
        ops.Nv12Frame(y, uv)                                                              # a missing matrix
    with pytest.raises(ValueError):
        ops.Nv12Frame(y, uv, matrix="rec709")
    bad_pairs = ((y.float(), uv), (y, uv.to(torch.int8)), (y[0], uv), (y, uv[..., 0]), (y, uv[:, :, :4]), (y, uv[:, :2]), (y[:1], uv),
                 (y.numpy(), uv), (y[:0], uv[:0]),
                 (torch.zeros(B, H, 2 * W, dtype=torch.uint8)[:, :, ::2], uv),              # a column stride of 2
                 (y, torch.zeros(B, 3, 5, 4, dtype=torch.uint8)[..., ::2]),                 # U and V two bytes apart
                 (y, torch.zeros(B, 3, 2, 5, dtype=torch.uint8).transpose(2, 3)),           # planar chroma (I420): not NV12
                 (y[:1].expand(B, H, W), uv),                                               # sb = 0 with ub != 0
                 (y, uv[:1].expand(B, 3, 5, 2)))
    for a, b in bad_pairs:
        with pytest.raises(ValueError):
            ops.Nv12Frame(a, b, **kw)
    # a chroma view one pair short for an odd width: W = 11 needs 6 pairs a row
    y11, uv11 = _planes(B, H, 11)
    with pytest.raises(ValueError):
        ops.Nv12Frame(y11, uv11[:, :, :5], **kw)
    # the table: yo outside 0 .. 255, a coefficient outside [-32768, 32768], not six integers
    for bad in ((256, 256, 0, 0, 0, 0), (-1, 256, 0, 0, 0, 0), (0, 32769, 0, 0, 0, 0), (0, 256, 0, -32769, 0, 0), (0, 256, 0, 0, 0), (0, 256.5, 0, 0, 0, 0),
                (0, 256, 0, 0, 0, True)):
        with pytest.raises(ValueError):
            ops.Nv12Frame(y, uv, matrix=None, csc=bad)
    edge = ops.Nv12Frame(y, uv, matrix=None, csc=(255, 32768, -32768, 32768, -32768, 32768))
    assert edge.csc == (255, 32768, -32768, 32768, -32768, 32768)
    # the ops that take a frame refuse what is no frame, and an NV12 frame on the CPU reaches no kernel
    f = ops.Nv12Frame(y, uv, **kw)
    key = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.gate_tiles(f, key)                                                            # the fp32 op
    with pytest.raises(ValueError):
        ops.gate_tiles_u8(f, key[:, :, :4])
    with pytest.raises(ValueError):
        ops.nv12_to_rgb(key)
    with pytest.raises(hip.HipLibraryError):
        ops.gate_tiles_u8(f, key, out=torch.zeros(B, 1, 1, dtype=torch.int32))


def test_frame_route_of_an_nv12_frame():
    B, H, W = 2, 6, 32
    f = ops.Nv12Frame(*_planes(B, H, W, 48, 64), matrix="bt709")
    suffix, tail = fovealseg.frames._frame_route(f)
    assert suffix == "_nv12" and tail == (H * 48, 48, 3 * 64, 64) + N.TABLES[("bt709", False)]
    with pytest.raises(hip.HipLibraryError):                                               # the device check stays at the call
        fovealseg.frames._frame_args(f, tail)
    for stem in ("fs_gate_tiles", "fs_gate_commit", "fs_state_shift", "fs_frame_overlay", "fs_frame_profiles"):
        assert stem + suffix in hip.SIGNATURES
    for stem in ("fs_gaze_lowres", "fs_grid_sample"):
        assert f"{stem}{suffix}_fwd" in hip.SIGNATURES
    # tensors go where they went
    assert fovealseg.frames._frame_route(torch.zeros(B, 3, H, W)) == ("", ()) and fovealseg.frames._frame_route(torch.zeros(B, 3, H, W, dtype=torch.uint8)) == ("_u8", ())


def test_byte_frame_select_of_an_nv12_frame_gathers_the_planes():
    B, H, W = 4, 5, 7
    y, uv = _planes(B, H, W, 16, 16)
    y.copy_(torch.randint(0, 256, (B, H, W), dtype=torch.uint8))
    uv.copy_(torch.randint(0, 256, (B, 3, 4, 2), dtype=torch.uint8))
    f = ops.Nv12Frame(y, uv, matrix="bt709", full_range=True)
    sel = torch.tensor([3, 1])
    g = ops.byte_frame_select(f, sel)
    assert isinstance(g, ops.Nv12Frame) and tuple(g.shape) == (2, 3, H, W) and g.csc == f.csc
    assert torch.equal(g.y, y[sel]) and torch.equal(g.uv, uv[sel])
    assert g.y.numel() + g.uv.numel() == 2 * (H * W + 3 * 4 * 2)                           # 1.5 bytes a pixel (odd sides rounded up), no RGB
    one = ops.Nv12Frame(y[:1].expand(B, H, W), uv[:1].expand(B, 3, 4, 2), matrix="bt601")
    g = ops.byte_frame_select(one, sel)
    assert g.strides == (0, 16, 0, 16) and g.y.data_ptr() == y.data_ptr() and tuple(g.shape) == (2, 3, H, W)


# ------------------------------------------------------------------------------------------------------------------ GPU: the conversion
def _to_rgb_abi(f, ox, pad=0, off=0):
    """fs_nv12_to_rgb at the C ABI into a guarded destination -> the planar (B,3,H,W) frame it holds (and the fourth bytes for ox = 4)."""
    B, H, W = f.B, f.H, f.W
    g = f.guarded()
    if ox == 1:
        ob, oy = 3 * H * W, W
    else:
        oy = W * ox + pad
        ob = H * oy
    out = Guarded(B * ob, torch.uint8, off=off)
    hip.call("fs_nv12_to_rgb", *f.args(g), out.ptr, ob, oy, ox, B, H, W)
    got = out.host(B * ob).numpy()
    assert f.unchanged(g)
    if ox == 1:
        return got.reshape(B, 3, H, W), None
    px = np.lib.stride_tricks.as_strided(got, shape=(B, H, W, ox), strides=(ob, oy, ox, 1))
    assert pad == 0 or bool((got.reshape(B, H, oy)[:, :, W * ox:] == _GARB[torch.uint8]).all())            # the padding stays garbage
    return np.ascontiguousarray(px[..., :3].transpose(0, 3, 1, 2)), (px[..., 3] if ox == 4 else None)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [("bt601", False), ("bt709", True)])
def test_nv12_to_rgb_over_all_triplets(which):
    """One 4096 x 4096 frame that holds every (Y, U, V): chroma sample s = j * 2048 + i carries the pair s & 0xFFFF, and its block the four
    lumas 4 * (s >> 16) + (0 .. 3): 65 536 pairs x 64 blocks x 4 lumas = 2^24 triplets, each once.  Against nv12_ref, planar destination."""
    table = N.TABLES[which]
    side = 4096
    s = np.arange(side // 2 * side // 2, dtype=np.int64).reshape(side // 2, side // 2)
    uv = np.stack([(s & 0xFF), (s >> 8) & 0xFF], axis=-1).astype(np.uint8)[None]
    y = np.empty((1, side, side), dtype=np.uint8)
    for dy in range(2):
        for dx in range(2):
            y[0, dy::2, dx::2] = 4 * (s >> 16) + 2 * dy + dx
    seen = np.zeros(1 << 24, dtype=bool)
    seen[(y[0].astype(np.int64) << 16) | (np.repeat(np.repeat(s & 0xFFFF, 2, axis=0), 2, axis=1))] = True
    assert seen.all()                                                                     # the frame is what it is said to be
    want = torch.from_numpy(N.to_rgb(y, uv, table))
    yd, uvd = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    f = ops.Nv12Frame(yd, uvd, matrix=which[0], full_range=which[1])
    assert f.csc == table and f.route() == 1
    out = Guarded(3 * side * side, torch.uint8)
    got = ops.nv12_to_rgb(f, out=out.body.view(1, 3, side, side))
    assert torch.equal(out.host(1, 3, side, side), want)
    assert torch.equal(yd.cpu(), torch.from_numpy(y)) and torch.equal(uvd.cpu(), torch.from_numpy(uv))
    # the one-pixel form on the same triplets: a luma view one byte off its alignment (the first 4095 columns, moved by one)
    y1 = torch.empty(side * side + 16, dtype=torch.uint8, device="cuda")[1:1 + side * side].view(1, side, side)
    y1.copy_(yd)
    f1 = ops.Nv12Frame(y1, uvd, matrix=which[0], full_range=which[1])
    assert f1.route() == 0 and torch.equal(ops.nv12_to_rgb(f1).cpu(), want)
    del got


@pytest.mark.gpu
def test_nv12_to_rgb_with_a_table_at_its_limits_into_every_destination():
    """A seeded table with coefficients at +-32768 and yo = 255, on 64 x 64 (and on an odd 5 x 7): planar, RGB and RGBA destinations, tight and
    pitched, aligned and one byte off -- the vector and the one-pixel form of both sides."""
    rng = np.random.default_rng(77)
    tables = [(255, 32768, -32768, 32768, -32768, 32768), (255, -32768, 32768, -32768, 32768, -32768), (0, 32768, 32768, 32768, 32768, 32768),
              tuple(int(v) for v in [rng.integers(0, 256)] + list(rng.integers(-32768, 32769, 5)))]
    for table in tables:
        for (B, H, W) in ((2, 64, 64), (3, 5, 7)):
            y, uv = random_planes(rng, B, H, W)
            y[0, 0, :4], uv[0, 0, 0] = (0, 255, 1, 254), (0, 255)                            # the corners of the cube are there
            for name in LAYOUTS:
                f = Nv12(y, uv, name, table, seed=B)
                want = N.to_rgb(f.y, f.uv, table)
                if (H, W) == (5, 7):                                                        # the buffers hold that frame, address by address
                    assert np.array_equal(want, N.frame_rgb(f.ybuf, f.uvbuf, f.sb, f.sy, f.ub, f.uy, B, H, W, table))
                for ox, pad, off in ((1, 0, 0), (3, 0, 0), (4, 0, 0), (3, 16, 0), (4, 5, 0), (1, 0, 1), (4, 0, 1)):
                    got, alpha = _to_rgb_abi(f, ox, pad, off)
                    assert np.array_equal(got, want), (table, name, ox, pad, off)
                    assert alpha is None or bool((alpha == 255).all())
                assert {0, 255} <= set(np.unique(want).tolist())                           # both clamps act in every frame


# ------------------------------------------------------------------------------------------------------------------ GPU: every pass --
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 16, 48), (1, 33, 80), (3, 20, 40), (2, 64, 272)]


def _tiles_abi(name, frame_args, key, B, H, W, T_):
    th, tw = -(-H // T_), -(-W // T_)
    gk, sad = Guarded(key.size, torch.uint8, body=torch.from_numpy(key)), Guarded(B * th * tw)
    hip.call(name, *frame_args, gk.ptr, sad.ptr, B, H, W, T_)
    got = sad.host(B, th, tw)
    assert gk.intact() and torch.equal(gk.body.cpu(), torch.from_numpy(key).reshape(-1))
    return got


def _every_pass(x, key, focus, bits, gstate, mstate, stats, counts, shift, grid, idx, T_, hs, ws, Rs):
    """Every op that reads a frame, on x (a planar uint8 tensor or an Nv12Frame) -> name -> result."""
    B, _, H, W = (int(v) for v in x.shape)
    out = {f"tiles {t}": ops.gate_tiles_u8(x, key, t) for t in T_}
    k, g = key.clone(), gstate.clone()
    rec = (torch.zeros(B, dtype=torch.int64, device="cuda"), stats.clone(), counts.clone(), bits.clone())
    ops.gate_commit_u8(x, idx, k, g, focus, rec, rec)
    out["commit key"], out["commit gstate"] = k, g
    out["profiles"] = ops.key_profiles(x)
    for r in Rs:                                                                          # motion: the estimate against the key, then the move
        out[f"estimate {r}"] = ops.profile_shift(out["profiles"], ops.key_profiles(key), gstate.clamp(min=1), (H, W), r)
    st = dict(key=key.clone(), bits=bits.clone(), gstate=gstate.clone(), stats=stats.clone(), counts=counts.clone(),
              prof_key=ops.key_profiles(key), mstate=mstate.clone())
    out["motion"] = ops.state_shift_u8(x, shift, st["key"], torch.zeros_like(key), st["bits"], torch.zeros_like(bits), st["gstate"], st["stats"],
                                       st["counts"], st["prof_key"], st["mstate"])
    out.update({"shift " + k_: v for k_, v in st.items()})
    out["lowres"] = ops.gaze_lowres(x, focus, hs, ws)
    out["sample"] = ops.grid_sample_u8(x, grid)
    out["overlay"] = ops.draw_instances(x, bits, stats=stats.clamp(0, min(H, W)), focus=focus)
    rgba = torch.full((B, H, W, 4), 0x3C, dtype=torch.uint8, device="cuda")
    ops.draw_instances(x, bits, focus=focus, outline_px=1, out=rgba.permute(0, 3, 1, 2)[:, :3])
    out["overlay rgba"] = rgba
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_every_nv12_pass_equals_its_planar_twin(B, H, W):
    """Tiles (T = 8 and 32), commit, profiles, the motion estimate and move, the two gathers of the front and the overlay, through the ops, on
    one random NV12 frame in six layouts -- tight, luma and chroma pitched differently, odd pitches, a pointer one byte off, one surface,
    one image for every viewer -- against the planar uint8 twin fed nv12_ref's RGB.  The one-pixel and the 16-pixel forms meet here: at W
    % 16 == 0 "tight", "pitched", "surface" and "sb0" take the vector forms, "pitch5" and "off1" the one-pixel forms of the same frame."""
    rng = np.random.default_rng(B * 100003 + H * 1009 + W)
    gen = torch.Generator().manual_seed(H * 1009 + W * 7 + B)
    y, uv = random_planes(rng, B, H, W)
    cap, hs, ws = 16, 5, 7
    key = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)).cuda()
    focus = torch.rand(B, 2, generator=gen).cuda()
    bits = torch.from_numpy(np.stack([RLE.bits(rng.random((H, W)) < 0.5) for _ in range(B)])).cuda()
    i64 = lambda *s: torch.randint(0, 16 * max(min(H, W) - 1, 1), s, generator=gen, dtype=torch.int64).cuda()
    gstate, mstate, stats = i64(B, 6), i64(B, 4), i64(B, 6)
    counts = torch.zeros(B, cap, dtype=torch.int32, device="cuda")
    shift = torch.tensor([[min(1, H - 1) * (-1) ** b, -min(2, W - 1) * (b != 1), 11, 22] for b in range(B)], dtype=torch.int64, device="cuda")
    grid = (torch.rand(B, 6, 5, 2, generator=gen) * 2.2 - 1.1).cuda()
    idx = torch.tensor([B - 1], dtype=torch.int32, device="cuda")
    Rs = [r for r in (1, 2) if 4 * r < min(H, W)]
    common = (key, focus, bits, gstate, mstate, stats, counts, shift, grid, idx, (8, 32), hs, ws, Rs)
    twins, routes = {}, set()
    for n, name in enumerate(LAYOUTS):
        f = Nv12(y, uv, name, seed=n)
        one = LAYOUTS[name][3]
        if one not in twins:
            planar = torch.from_numpy(f.planar).cuda()
            twins[one] = _every_pass(planar, *common)
            # the twin of the tile pass is itself what gate_ref says of the converted frame
            assert torch.equal(twins[one]["tiles 8"].cpu().long(), torch.from_numpy(R.tiles(f.planar.astype(np.float32) / np.float32(255), key.cpu().numpy(), 8)))
            assert torch.equal(ops.nv12_to_rgb(f.frame(f.guarded())), planar)
        g = f.guarded()
        got = _every_pass(f.frame(g), *common)
        torch.cuda.synchronize()
        assert f.unchanged(g), name
        routes.add(1 if f.vec else 0)
        for what, want in twins[one].items():
            assert got[what].dtype == want.dtype and torch.equal(_bits32(got[what]), _bits32(want)), (name, what)
        # the hot pass at the C ABI as well, between guard bands
        for T_ in (8, 32):
            g = f.guarded()
            sad = _tiles_abi("fs_gate_tiles_nv12", f.args(g), key.cpu().numpy(), B, H, W, T_)
            assert f.unchanged(g) and torch.equal(sad, twins[one][f"tiles {T_}"].cpu()), (name, T_)
    assert routes == ({0, 1} if W % 16 == 0 else {0})
    want = twins[False]
    assert B * H * W < 64 or (bool(want["tiles 8"].any()) and not torch.equal(want["shift key"], key))


@pytest.mark.gpu
def test_one_changed_byte_moves_the_sums_it_should():
    """The key is the converted frame, so every tile reads 0.  One luma byte changed: exactly that pixel's tile reads the |change| of its
    three channels.  One chroma byte changed: the tiles of its 2 x 2 block read the four pixels' changes.  In both forms of the pass."""
    B, H, W, T_ = 2, 33, 80, 8
    rng = np.random.default_rng(5)
    y, uv = random_planes(rng, B, H, W)
    y[:] = rng.integers(60, 200, y.shape)
    uv[:] = rng.integers(100, 156, uv.shape)                                              # away from the clamps: every change shows
    key = N.to_rgb(y, uv, BT601)
    th, tw = -(-H // T_), -(-W // T_)
    # the first and the last pixel of a lane's sixteen, both sides of a tile border, the last row (odd H: a chroma row of its own)
    spots = [(0, 0, 0), (1, 3, 15), (0, 8, 16), (1, 7, 31), (0, H - 1, W - 1), (1, 32, 0), (0, 15, 47)]
    for n, (b, py, px) in enumerate(spots):
        for what in ("luma", "u", "v"):
            y2, uv2 = y.copy(), uv.copy()
            if what == "luma":
                y2[b, py, px] += 9
            else:
                uv2[b, py >> 1, px >> 1, 0 if what == "u" else 1] += 7
            changed = np.abs(N.to_rgb(y2, uv2, BT601).astype(np.int64) - key).sum(1)          # (B,H,W): |dR| + |dG| + |dB|
            block = np.zeros((B, H, W), dtype=bool)
            if what == "luma":
                block[b, py, px] = True
            else:
                block[b, (py >> 1) * 2:(py >> 1) * 2 + 2, (px >> 1) * 2:(px >> 1) * 2 + 2] = True
            assert changed[block].all() and not changed[~block].any()                     # by hand: who moves
            want = np.zeros((B, th, tw), dtype=np.int64)
            for (bb, yy, xx) in zip(*np.nonzero(block)):
                want[bb, yy // T_, xx // T_] += changed[bb, yy, xx]
            for name in ("tight", "off1"):
                f = Nv12(y2, uv2, name, seed=n)
                g = f.guarded()
                got = _tiles_abi("fs_gate_tiles_nv12", f.args(g), key, B, H, W, T_)
                assert torch.equal(got.long(), torch.from_numpy(want)), (b, py, px, what, name)


@pytest.mark.gpu
def test_nv12_entry_points_reject_bad_arguments():
    B, H, W, T_ = 2, 16, 24, 8
    sy, uy = 32, 40
    sb, ub = H * sy, (H // 2) * uy
    yb, ub_, key, sad, rgb = Guarded(B * sb, torch.uint8), Guarded(B * ub, torch.uint8), Guarded(B * 3 * H * W, torch.uint8), Guarded(B * 6), Guarded(B * 3 * H * W, torch.uint8)
    prof, key2, cap = Guarded(B * (H + W)), Guarded(B * 3 * H * W, torch.uint8), 5
    low, samp = Guarded(B * 4 * 4 * 5, torch.float32), Guarded(B * 4 * 4 * 3, torch.float32)
    gstate, stats, mstate = Guarded(B * 6, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * 4, torch.int64)
    focus, grid = Guarded(B * 2, torch.float32), Guarded(B * 4 * 4 * 2, torch.float32)
    bits, bits2, prof_key = Guarded(B * H), Guarded(B * H), Guarded(B * (H + W))
    shift, motion, counts = Guarded(B * 4, torch.int64, body=torch.ones(B * 4)), Guarded(B * 6, torch.int64), Guarded(B * cap)
    scratch = Guarded(hip.query("fs_state_shift_scratch_ints", B, H, W, cap))
    rec = [Guarded(B, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * cap), Guarded(B * H), Guarded(B * 3, torch.float32)]
    style, drawn = Guarded(20), Guarded(B * 3 * H * W, torch.uint8)
    idx = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    outs = [yb, ub_, key, key2, sad, rgb, prof, low, samp, gstate, stats, mstate, bits, bits2, prof_key, motion, counts, scratch, drawn] + rec
    fr = [yb.ptr, ub_.ptr, sb, sy, ub, uy, *BT601]
    # the description: a null plane, rows that overlap, negative steps, images that overlap, sb = 0 with ub != 0; the table
    frame_bads = ((0, None), (1, None), (3, W - 1), (5, W - 1), (2, -sb), (4, -ub), (2, sb - 1), (4, ub - 1), (2, 0), (4, 0), (6, -1), (6, 256),
                  (7, 32769), (8, -32769), (9, 40000), (10, -40000), (11, 1 << 20))

    def each(name, good, bads):
        for i, bad in frame_bads + tuple(bads):
            a = list(good)
            a[i] = bad
            with pytest.raises(hip.HipLibraryError, match="argument rejected"):
                hip.call(name, *a)
            torch.cuda.synchronize()
            assert all(o.intact() and bool((o.body == o.body[0]).all()) for o in outs), f"a rejected {name} launched something"

    each("fs_gate_tiles_nv12", fr + [key.ptr, sad.ptr, B, H, W, T_], ((12, None), (13, None), (14, 0), (15, 0), (16, -1), (17, 12)))
    # the conversion and the overlay also refuse a destination that is one of the frame's planes
    each("fs_nv12_to_rgb", fr + [rgb.ptr, 3 * H * W, W, 1, B, H, W],
         ((12, None), (12, yb.ptr), (12, ub_.ptr), (13, 3 * H * W - 1), (14, W + 1), (15, 2), (16, 0), (17, 0), (18, 0)))
    each("fs_frame_profiles_nv12", fr + [prof.ptr, B, H, W], ((12, None), (13, 0), (14, 0), (15, -1)))
    each("fs_gaze_lowres_nv12_fwd", fr + [focus.ptr, low.ptr, B, H, W, 4, 4], ((12, None), (13, None), (14, 0), (15, 0), (16, -1), (17, 1), (18, 0)))
    each("fs_grid_sample_nv12_fwd", fr + [grid.ptr, samp.ptr, B, H, W, 4, 4, 1], ((12, None), (13, None), (14, 0), (15, 0), (16, -1), (17, 0), (18, 0)))
    ptrs = [g.ptr for g in rec]
    each("fs_gate_commit_nv12", fr + [idx.data_ptr(), 2, key.ptr, gstate.ptr, focus.ptr, *ptrs, *ptrs, B, H, W, cap],
         ((12, None), (13, 3), (13, -1), (14, None), (15, None), (16, None), (17, None), (20, None), (22, None), (25, None), (26, None),
          (27, 0), (28, 0), (29, 0), (30, 0)))
    good = fr + [shift.ptr, key.ptr, key2.ptr, bits.ptr, bits2.ptr, gstate.ptr, stats.ptr, counts.ptr, prof_key.ptr, mstate.ptr, motion.ptr,
                 scratch.ptr, B, H, W, cap]
    each("fs_state_shift_nv12", good, [(i, None) for i in range(12, 24)] + [(14, key.ptr), (16, bits.ptr), (23, scratch.ptr + 4), (24, 0), (25, 0), (26, 0), (27, 0)])
    good = fr + [bits.ptr, None, None, None, None, 1, style.ptr, 1, drawn.ptr, 3 * H * W, W, 1, B, H, W]
    each("fs_frame_overlay_nv12", good, ((12, None), (18, None), (19, 3), (20, None), (20, yb.ptr), (20, ub_.ptr), (23, 2), (24, 0), (25, 0), (26, 0)))
    route = hip.load().fs_nv12_frame_route
    for args, want in ROUTE_CASES:                                                         # the C function against the cases held by hand
        assert route(args[0] or None, args[1] or None, *args[2:]) == want, args
    assert route(yb.ptr, ub_.ptr, sb, sy, ub, uy, W) == 0 and route(yb.ptr, ub_.ptr, sb, sy, ub, uy, 16) == 0          # uy = 40
    assert route(yb.ptr, ub_.ptr, sb, sy, 16 * 48, 48, 16) == 1 and route(yb.ptr + 1, ub_.ptr, sb, sy, 16 * 48, 48, 16) == 0
    assert route(None, ub_.ptr, sb, sy, ub, uy, W) == -1 and route(yb.ptr, ub_.ptr, sb, W - 1, ub, uy, W) == -1
    # B == 1: the image steps are not looked at beyond their sign
    hip.call("fs_gate_tiles_nv12", yb.ptr, ub_.ptr, 1, sy, 3, uy, *BT601, key.ptr, sad.ptr, 1, H, W, T_)
    torch.cuda.synchronize()
    assert sad.intact()


# ------------------------------------------------------------------------------------------------------------------ GPU: module -----
def nv12_of_rgb(U):
    """NV12 planes (bt601 limited, the chroma of a block's top-left pixel) whose picture resembles the uint8 frame U (B,3,H,W): the tests'
    way to an NV12 frame with something to segment.  What the frame then *is* is nv12_ref's conversion of it, not U."""
    r, g, b = (U[:, c].float() for c in range(3))
    y = (16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255).round().clamp(0, 255).to(torch.uint8)
    u = (128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255).round().clamp(0, 255).to(torch.uint8)
    v = (128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255).round().clamp(0, 255).to(torch.uint8)
    return y.contiguous(), torch.stack([u[:, ::2, ::2], v[:, ::2, ::2]], dim=-1).contiguous()


def _nv12_views(y, uv, seed=0):
    """The same planes as two tight allocations, as views pitched differently, and as one surface per batch."""
    B, H, W = y.shape
    Hc, Wc = uv.shape[1:3]
    gen = torch.Generator(device="cuda").manual_seed(200 + seed)
    rnd = lambda n: torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    kw = dict(matrix="bt601")
    yp = rnd(B * H * (W + 16)).as_strided((B, H, W), (H * (W + 16), W + 16, 1))
    up = rnd(B * Hc * (2 * Wc + 48)).as_strided((B, Hc, Wc, 2), (Hc * (2 * Wc + 48), 2 * Wc + 48, 2, 1))
    yp.copy_(y), up.copy_(uv)
    pitch = W + 5
    per = (H + Hc) * pitch + 3
    surf = rnd(B * per)
    fs = ops.nv12_from_surface(surf, H, W, pitch, H * pitch, per, **kw)
    fs.y.copy_(y), fs.uv.copy_(uv)
    frames = dict(tight=ops.Nv12Frame(y, uv, **kw), pitched=ops.Nv12Frame(yp, up, **kw), surface=fs)
    assert [f.route() for f in frames.values()] == [1, 1, 0]
    return frames


@pytest.mark.gpu
def test_module_reads_nv12_frames(served):
    module, calls, TP = served
    X, Fp, Y, cl = T.synthetic_batch(2, SIZE, SIZE, seed=SEED, device="cuda")
    y, uv = nv12_of_rgb(_bytes_of(X))
    frames = _nv12_views(y, uv)
    U = ops.nv12_to_rgb(frames["tight"])
    assert torch.equal(U.cpu(), torch.from_numpy(N.to_rgb(y.cpu().numpy(), uv.cpu().numpy(), BT601))) and len(torch.unique(U)) > 100
    kw = dict(return_bits=True, return_score=True)
    want = (module.predict(U, Fp), module.predict_instances(U, Fp, **kw), module.evaluate(U, Fp, Y, cl, class_areas=True),
            module.evaluate_instances(U, Fp, Y, cl, component=8))
    assert 0 < int(want[1][1][0, 0]) < SIZE * SIZE
    for name, f in frames.items():
        y0, uv0 = f.y.clone(), f.uv.clone()
        assert torch.equal(module.predict(f, Fp), want[0]), name
        assert _same(module.predict_instances(f, Fp, **kw), want[1])
        assert _same(module.evaluate(f, Fp, Y, cl, class_areas=True), want[2])
        assert _same(module.evaluate_instances(f, Fp, Y, cl, component=8), want[3])
        assert torch.equal(f.y, y0) and torch.equal(f.uv, uv0)
    module.check_nan()
    # nothing of the frame's size is made in front of the call: the NV12 call's peak is not above the planar call's
    pn, pp = _peak_of(lambda: module.predict_instances(frames["pitched"], Fp)), _peak_of(lambda: module.predict_instances(U, Fp))
    print(f"predict_instances raised the peak by {pn} bytes fed NV12 and by {pp} fed planar uint8")
    assert pn <= pp


# ------------------------------------------------------------------------------------------------------------------ GPU: session ----
def _grew(call):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = call()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def _feed(kind, y, uv, seed=0):
    if kind in ("tight", "pitched", "surface"):
        return _nv12_views(y, uv, seed)[kind]
    U = ops.nv12_to_rgb(ops.Nv12Frame(y, uv, matrix="bt601"))
    return {"u8": U, "f32": floats(U), "hwc": U.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)}[kind]


def _step_all(sessions, feeds, y, uv, Fp, force=None, seed=0):
    """One step of every session on the same picture, each fed its own layout; all results and states must agree.  Returns the first result."""
    outs = [s.step(_feed(kind, y, uv, seed), Fp, force=force) for s, kind in zip(sessions, feeds)]
    for s, o in zip(sessions[1:], outs[1:]):
        assert _same(tuple(outs[0]), tuple(o)) and s.counts == sessions[0].counts
        for a, b in zip(_state_of(sessions[0]), _state_of(s)):
            assert torch.equal(_bits32(a), _bits32(b))
    return outs[0]


def _cycle(*kinds):
    n = 0
    while True:
        yield kinds[n % len(kinds)]
        n += 1


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(score=True), dict(component=8)], ids=["score", "component"])
def test_session_on_nv12_equals_the_session_on_planar_bytes(served, kw):
    module, calls, TP = served
    H = W = SIZE
    X, Fp = TP._batch(2, SIZE, SEED)
    y, uv = nv12_of_rgb(_bytes_of(X))
    y0, uv0 = y.clone(), uv.clone()
    U = _feed("u8", y, uv)
    sessions = [GazeSession(module, 2, (H, W), **kw) for _ in range(3)]
    alt = _cycle("surface", "u8", "tight", "f32", "pitched", "hwc")                        # the layout may change from step to step
    feed = lambda: ("u8", "pitched", next(alt))
    *rec, gate = _step_all(sessions, feed(), y, uv, Fp)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and all(torch.equal(s._key, U) for s in sessions)       # the key is planar RGB bytes
    held = [t.clone() for t in rec]
    *rec, gate = _step_all(sessions, feed(), y, uv, Fp, seed=1)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and gate[:, 1:6].tolist() == [[0] * 5] * 2 and _same(rec, held)
    # a REUSE step fed NV12 allocates nothing
    views = _nv12_views(y, uv, 2)
    for s, name in zip(sessions[1:], ("tight", "surface")):
        grew, out = _grew(lambda: s.step(views[name], Fp))
        print(f"a REUSE step fed the {name} NV12 frame raised the peak by {grew} bytes")
        assert grew == 0 and out[-1][:, 0].tolist() == [R.REUSE] * 2
    sessions[0].step(U, Fp)
    # the luma of a tile inside viewer 1's box inverted: RUN_ROI, a partial run
    ty, tx = int(held[1][1, 2]) // 32, int(held[1][1, 1]) // 32
    y4 = y.clone()
    y4[1, 32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32] = 255 - y4[1, 32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32]
    *rec, gate = _step_all(sessions, feed(), y4, uv, Fp, seed=3)
    assert gate[:, 0].tolist() == [R.REUSE, R.RUN_ROI]
    U4 = _feed("u8", y4, uv)
    want = module.predict_instances(U4[1:2], Fp[1:2], return_bits=True, return_score=bool(kw.get("score")), **({"component": 8} if "component" in kw else {}))
    assert _same(tuple(t[1:2] for t in rec), tuple(want)[:len(rec)])
    # a partial run fed NV12 gathers the running viewer's 1.5 bytes a pixel: its peak is not above the planar step's, which selects 3
    V4 = _nv12_views(y4, uv, 4)
    g_planar, out_p = _grew(lambda: sessions[0].step(U4, Fp, force=[0, 1]))
    g_nv12, out_v = _grew(lambda: sessions[1].step(V4["pitched"], Fp, force=[0, 1]))
    print(f"a partial run raised the peak by {g_nv12} bytes fed NV12 and by {g_planar} fed planar bytes")
    assert g_nv12 <= g_planar and out_v[-1][:, 0].tolist() == [R.REUSE, R.RUN_FORCED] and _same(tuple(out_p), tuple(out_v))
    assert _same(tuple(sessions[2].step(V4["surface"], Fp, force=[0, 1])), tuple(out_p))
    for a, b, c in zip(*(_state_of(s) for s in sessions)):
        assert torch.equal(_bits32(a), _bits32(b)) and torch.equal(_bits32(a), _bits32(c))
    # render: the records drawn onto the NV12 frame are those drawn onto its planar twin
    for s in sessions[:2]:
        assert torch.equal(s.render(V4["tight"], focus=Fp, outline_px=2), s.render(U4, focus=Fp, outline_px=2))
    assert torch.equal(y, y0) and torch.equal(uv, uv0) and all(s.counts == sessions[0].counts for s in sessions)


@pytest.mark.gpu
def test_moving_session_on_nv12_equals_the_session_on_planar_bytes(served):
    module, calls, TP = served
    PAD = 16

    def planes(windows):
        out = [M.window(M.canvas(seed, SIZE + 2 * PAD, SIZE + 2 * PAD, 4), yy, xx, SIZE, SIZE) for seed, yy, xx in windows]
        return nv12_of_rgb(_bytes_of(torch.from_numpy(np.stack(out)).cuda()))

    focus = lambda pixels: torch.tensor([[py / (SIZE - 1), px / (SIZE - 1)] for py, px in pixels], dtype=torch.float32, device="cuda")
    # the content moves by even amounts, so that the chroma blocks move with it
    P1, F1 = planes([(25, PAD, PAD), (31, PAD, PAD)]), focus([(128, 128), (100, 140)])
    P2, F2 = planes([(25, PAD - 2, PAD + 4), (31, PAD, PAD)]), focus([(130, 124), (100, 140)])
    P3, F3 = planes([(25, PAD, PAD + 2), (31, PAD, PAD)]), focus([(128, 126), (100, 140)])
    sessions = [GazeSession(module, 2, (SIZE, SIZE), motion_px=5) for _ in range(3)]
    alt = _cycle("tight", "u8", "surface", "f32")
    feed = lambda: ("u8", "pitched", next(alt))
    *rec, gate, motion = _step_all(sessions, feed(), *P1, F1)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and motion.tolist() == [[0] * 6] * 2
    assert torch.equal(sessions[1]._prof_key, ops.key_profiles(_feed("u8", *P1)))
    *rec, gate, motion = _step_all(sessions, feed(), *P2, F2, seed=1)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and motion[:, :2].tolist() == [[2, -4], [0, 0]]
    f3 = _nv12_views(*P3, 2)["tight"]
    grew, out = _grew(lambda: sessions[1].step(f3, F3))
    print(f"a moved REUSE step fed NV12 raised the peak by {grew} bytes")
    assert grew == 0 and out[-2][:, 0].tolist() == [R.REUSE] * 2 and out[-1][:, :2].tolist() == [[-2, 2], [0, 0]]
    for s, kind in ((sessions[0], "u8"), (sessions[2], "surface")):
        assert _same(tuple(out), tuple(s.step(_feed(kind, *P3, 3), F3)))
    for a, b, c in zip(*(_state_of(s) for s in sessions)):
        assert torch.equal(_bits32(a), _bits32(b)) and torch.equal(_bits32(a), _bits32(c))


# ------------------------------------------------------------------------------------------------------------------ GPU: a stream ---
class _Nv12Stub(S.StubModule):
    """session_ref's stub head, which reads tensors: an Nv12Frame reaches it as the frame it is, and is noted as such."""

    def predict_instances(self, img, focus, **kw):
        if isinstance(img, ops.Nv12Frame):
            out = super().predict_instances(ops.nv12_to_rgb(img), focus, **kw)
            self.seen[-1] = "nv12"
            return out
        return super().predict_instances(img, focus, **kw)


STREAM = dict(B=2, H=50, W=80, steps=40, seed=4, kw=dict(tile=16, motion_px=3, score=True))
STREAM_LAYOUTS = ("nv12", "u8", "nv12 pitched", "hwc", "nv12 surface", "f32")


@pytest.mark.gpu
def test_session_equals_the_model_over_a_stream_with_nv12_among_the_layouts():
    """A seeded stream of tests/session_ref.py's kind -- cameras on textures, gazes that follow, drift and jump, forces and resets -- whose
    every frame is NV12 content: the step's bytes are turned into planes, and the picture is nv12_ref's conversion of them.  The numpy
    model of the session sees that picture; the device session is fed it as NV12 (tight, pitched, one surface), planar bytes, interleaved
    bytes and fp32 in turn, so every change of layout between NV12 and the others occurs.  Every step's outputs are the model's."""
    from test_session_streams import _np, _bits_equal
    B, H, W, kw = STREAM["B"], STREAM["H"], STREAM["W"], STREAM["kw"]
    model = S.RefSession(S.stub_predict(H, W, 8 * W + 1, True), B, (H, W), **kw)
    stub = _Nv12Stub()
    s = GazeSession(stub, B, (H, W), **kw)
    seen, subsets, moved = set(), 0, 0
    for t, (rgba, focus, force, reset, _layout) in enumerate(S.stream(STREAM["seed"], B, H, W, STREAM["steps"], kw["motion_px"], tile=kw["tile"], model=model)):
        if reset is not None:
            model.reset(reset)
            s.reset(reset)
        y, uv = nv12_of_rgb(torch.from_numpy(np.ascontiguousarray(rgba[..., :3].transpose(0, 3, 1, 2))))
        picture = N.to_rgb(y.numpy(), uv.numpy(), BT601)
        layout = STREAM_LAYOUTS[(t * 5 + t // 6) % len(STREAM_LAYOUTS)]
        yd, uvd = y.cuda(), uv.cuda()
        if layout.startswith("nv12"):
            x = _nv12_views(yd, uvd, t)[{"nv12": "tight", "nv12 pitched": "pitched", "nv12 surface": "surface"}[layout]]
            before = (x.y.clone(), x.uv.clone())
        else:
            U = torch.from_numpy(picture).cuda()
            x = {"u8": U, "f32": floats(U), "hwc": U.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)}[layout]
        want = model.step(picture.astype(np.float32) / np.float32(255), focus, force)
        got = s.step(x, torch.from_numpy(focus).cuda(), force)
        assert len(got) == len(want) == 7
        for k, (g, w) in enumerate(zip(got, want)):
            assert _bits_equal(_np(g), np.asarray(w)), f"step {t} ({layout}): element {k}"
        assert s.counts == model.counts and np.array_equal(s._key.cpu().numpy(), model.key), f"step {t} ({layout})"
        if layout.startswith("nv12"):
            assert torch.equal(x.y, before[0]) and torch.equal(x.uv, before[1])
            if model.ran:
                assert stub.seen[-1] == "nv12", f"step {t}: the head was handed {stub.seen[-1]} frames"
            subsets += 0 < len(model.ran) < B
            moved += bool(np.asarray(want[-1])[:, :2].any())
        seen.add(layout)
    print(f"counts {s.counts}; on NV12 steps: {subsets} ran a strict subset, {moved} moved a record")
    assert seen == set(STREAM_LAYOUTS) and s.counts[R.REUSE] > 0
