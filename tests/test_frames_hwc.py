"""Interleaved (HWC / RGBA) uint8 frames read in place: ops.byte_frame_layout, fs_byte_frame_route, fs_gaze_lowres_hwc_fwd,
fs_grid_sample_hwc_fwd, fs_gate_tiles_hwc, fs_gate_commit_hwc, fs_frame_profiles_hwc, fs_state_shift_hwc, and the views that predict* /
evaluate* / GazeSession.step take without a copy.

The byte of channel c at (b, y, x) of such a frame is buf[b * sb + y * sy + x * sx + c].  Every hwc entry point must equal its planar twin
(tests/test_frames_u8.py holds those to the fp32 route and to tests/gate_ref.py / tests/motion_ref.py) fed the de-interleaved bytes, bit
for bit: every comparison is torch.equal / np.array_equal.  The alpha bytes, the pitch padding and the gaps between images hold random
bytes, differently filled from call to call, so a result that equals the twin's -- which never sees them -- is influenced by none of
them.  At the C ABI every buffer sits between guard bands and the frame buffer is compared with its contents before the call."""
import numpy as np
import pytest
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T
from fovealseg.session import GazeSession

import gate_ref as R
import motion_ref as M
import rle_ref as RLE
import kernel_testing                                                                                  # noqa: F401  (the suite's shared helpers import)
from test_gaze_session import Guarded, _GARB, _same, _flip_tile, served                               # noqa: F401  (served is a fixture)
from test_frames_u8 import (as_float, floats, _bits32, _records, _REC_TYPES, _STATE_ORDER, _STATE_TYPES, _all_bytes_frame, _bytes_of, _peak_of,
                            _state_of, SIZE, SEED)

HWC_ENTRY_POINTS = ("fs_gaze_lowres_hwc_fwd", "fs_grid_sample_hwc_fwd", "fs_gate_tiles_hwc", "fs_gate_commit_hwc", "fs_frame_profiles_hwc",
                    "fs_state_shift_hwc")


# ------------------------------------------------------------------------------------------------------------------ layouts --------
# name -> (pitch padding in bytes, gap between images in bytes, one image for all viewers, base pointer one byte off, stays on the vector route)
LAYOUTS = {"tight": (0, 0, False, False, True), "pitch16": (16, 0, False, False, True), "pitch5": (5, 0, False, False, False),
           "off1": (0, 0, False, True, False), "gap": (0, 32, False, False, True), "sb0": (0, 0, True, False, True)}
CASES = [(name, sx) for name in LAYOUTS for sx in (3, 4)]


class Frame:
    """A planar (B,3,H,W) byte frame laid out interleaved in a buffer of random bytes; .planar is what the planar twin is fed."""

    def __init__(self, planar, name, sx, seed=0):
        pad, gap, one, self.off, vec = LAYOUTS[name]
        B, _, H, W = planar.shape
        self.B, self.H, self.W, self.sx = B, H, W, sx
        self.sy = W * sx + pad
        nb = 1 if one else B
        stride = H * self.sy + gap
        self.sb = 0 if one else stride
        self.planar = np.repeat(planar[:1], B, axis=0) if one else planar
        self.buf = np.random.default_rng(seed).integers(0, 256, nb * stride).astype(np.uint8)       # alpha, padding and gaps: garbage
        view = np.lib.stride_tricks.as_strided(self.buf, shape=(nb, H, W, 3), strides=(stride, self.sy, sx, 1))
        view[...] = planar[:nb].transpose(0, 2, 3, 1)
        self.route = 1 if (vec and W % 16 == 0) else 0

    def guarded(self):
        g = Guarded(self.buf.size, torch.uint8, body=torch.from_numpy(self.buf), off=1 if self.off else 0)
        want = hip.load().fs_byte_frame_route(g.ptr, self.sb, self.sy, self.sx, self.W)
        assert want == self.route, (want, self.route)                       # the case runs the route it is there for
        return g

    def args(self, g):
        return (g.ptr, self.sb, self.sy, self.sx)

    def unchanged(self, g):
        return g.intact() and torch.equal(g.body.cpu(), torch.from_numpy(self.buf))


def deinterleave(buf, sb, sy, sx, B, H, W):
    """The planar frame of an interleaved buffer, by the definition."""
    out = np.empty((B, 3, H, W), dtype=np.uint8)
    for b in range(B):
        for c in range(3):
            for y in range(H):
                out[b, c, y] = buf[b * sb + y * sy + c + sx * np.arange(W)]
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU ------------
def test_the_ctypes_table_binds_the_interleaved_entry_points():
    frame = "plli"
    assert hip.SIGNATURES["fs_gaze_lowres_hwc_fwd"] == frame + hip.SIGNATURES["fs_gaze_lowres_u8_fwd"][1:]
    assert hip.SIGNATURES["fs_grid_sample_hwc_fwd"] == frame + "pp" + "iiiiii"                         # no C: three channels
    assert hip.SIGNATURES["fs_gate_tiles_hwc"] == frame + hip.SIGNATURES["fs_gate_tiles_u8"][1:]
    assert hip.SIGNATURES["fs_gate_commit_hwc"] == frame + hip.SIGNATURES["fs_gate_commit_u8"][1:]
    assert hip.SIGNATURES["fs_frame_profiles_hwc"] == frame + hip.SIGNATURES["fs_key_profiles"][1:]
    assert hip.SIGNATURES["fs_state_shift_hwc"] == frame + hip.SIGNATURES["fs_state_shift_u8"][1:]
    assert hip.HOST_ONLY["fs_byte_frame_route"] == ("l", "plli" + "i")
    assert all(name in hip.SIGNATURES for name in HWC_ENTRY_POINTS)


def _layout(t):
    return ops.byte_frame_strides(tuple(t.shape), tuple(t.stride()))


def test_byte_frame_layout_of_stride_patterns():
    B, H, W = 3, 6, 8
    planar = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    assert _layout(planar) == ("planar",) and ops.byte_frame_layout(planar) == ("planar",)
    hwc = torch.zeros(B, H, W, 3, dtype=torch.uint8).permute(0, 3, 1, 2)
    assert _layout(hwc) == ("hwc", H * W * 3, W * 3, 3) == ops.byte_frame_layout(hwc)
    rgba = torch.zeros(B, H, W, 4, dtype=torch.uint8).permute(0, 3, 1, 2)[:, :3]
    assert _layout(rgba) == ("hwc", H * W * 4, W * 4, 4) == ops.byte_frame_layout(rgba)
    big = torch.zeros(B, H + 5, W + 7, 4, dtype=torch.uint8)
    crop = big[:, 2:2 + H, 3:3 + W, :3].permute(0, 3, 1, 2)
    assert _layout(crop) == ("hwc", (H + 5) * (W + 7) * 4, (W + 7) * 4, 4) == ops.byte_frame_layout(crop)
    one = torch.zeros(1, H, W, 3, dtype=torch.uint8).permute(0, 3, 1, 2).expand(B, 3, H, W)
    assert _layout(one) == ("hwc", 0, W * 3, 3) == ops.byte_frame_layout(one)
    cl = planar.contiguous(memory_format=torch.channels_last)
    assert _layout(cl) == ("hwc", H * W * 3, W * 3, 3) == ops.byte_frame_layout(cl)
    # strides of dimensions of size 1 are ignored
    assert ops.byte_frame_strides((1, 3, H, W), (12345, 1, W * 3, 3)) == ("hwc", 0, W * 3, 3)
    assert ops.byte_frame_strides((B, 3, H, 1), (H * 7, 1, 7, 999)) == ("hwc", H * 7, 7, 3)
    assert ops.byte_frame_strides((B, 3, 1, W), (W * 4, 1, 1, 4)) == ("hwc", W * 4, W * 4, 4)
    assert ops.byte_frame_strides((1, 3, H, 1), (77, H, 1, 55)) == ("planar",)
    assert ops.byte_frame_strides((1, 3, H, W), (1, H * W, W, 1)) == ("planar",)
    # anything else is no byte frame view
    assert ops.byte_frame_strides((B, 3, H, W), (H * W * 5, 1, W * 5, 5)) is None                      # sx = 5
    assert _layout(torch.zeros(B, W, H, 3, dtype=torch.uint8).permute(0, 3, 2, 1)) is None             # H and W transposed
    assert _layout(torch.zeros(B, 3, H, 2 * W, dtype=torch.uint8)[:, :, :, ::2]) is None               # a planar slice
    assert _layout(torch.zeros(B, 3, 2 * H, W, dtype=torch.uint8)[:, :, ::2]) is None
    assert ops.byte_frame_strides((B, 3, H, W), (W * 3, 1, W * 3, 3)) is None                          # images that overlap: 0 < sb < H * sy
    assert ops.byte_frame_strides((B, 3, H, W), (H * W * 3, 1, W * 3 - 1, 3)) is None                  # rows that overlap
    assert ops.byte_frame_strides((B, 2, H, W), (H * W * 2, 1, W * 2, 2)) is None
    for other in (planar.float(), planar[0], planar[:0], planar.numpy(), None):
        assert ops.byte_frame_layout(other) is None


def test_frame_route_of_dtypes_and_stride_patterns():
    """ops._frame_route: the entry-point suffix and the arguments after the frame's pointer that gate_tiles*, gate_commit*, frame_profiles /
    key_profiles, state_shift*, gaze_lowres and grid_sample_u8 all take from it -- byte_frame_layout's rule, on CPU tensors: no device is
    asked before the call."""
    B, H, W = 3, 6, 8
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    hwc = lambda t: t.permute(0, 3, 1, 2)[:, :3]
    pitch = W * 3 + 5
    table = [
        ("planar fp32", torch.zeros(B, 3, H, W), ("", ())),
        ("planar uint8", u8(B, 3, H, W), ("_u8", ())),
        ("tight RGB", hwc(u8(B, H, W, 3)), ("_hwc", (H * W * 3, W * 3, 3))),
        ("RGBA [:, :3]", hwc(u8(B, H, W, 4)), ("_hwc", (H * W * 4, W * 4, 4))),
        ("channels_last", u8(B, 3, H, W).contiguous(memory_format=torch.channels_last), ("_hwc", (H * W * 3, W * 3, 3))),
        ("padded pitch", u8(B * H * pitch).as_strided((B, 3, H, W), (H * pitch, 1, pitch, 3)), ("_hwc", (H * pitch, pitch, 3))),
        ("padded pitch, base one byte off", u8(1 + B * H * pitch).as_strided((B, 3, H, W), (H * pitch, 1, pitch, 3), 1), ("_hwc", (H * pitch, pitch, 3))),
        ("a crop", hwc(u8(B, H + 5, W + 7, 4)[:, 2:2 + H, 3:3 + W]), ("_hwc", ((H + 5) * (W + 7) * 4, (W + 7) * 4, 4))),
        ("sb == 0, expanded", hwc(u8(1, H, W, 3)).expand(B, 3, H, W), ("_hwc", (0, W * 3, 3))),
        ("B == 1", hwc(u8(1, H, W, 3)), ("_hwc", (0, W * 3, 3))),
        ("H == 1", hwc(u8(B, 1, W, 4)), ("_hwc", (W * 4, W * 4, 4))),
        ("W == 1", hwc(u8(B, H, 1, 3)), ("_hwc", (H * 3, 3, 3))),
        ("B == H == W == 1: contiguous", hwc(u8(1, 1, 1, 4)), ("_u8", ())),
        # fp32 has one entry point: a view of it is refused at the call, by hip.ptr, as every non-contiguous tensor is
        ("non-contiguous fp32", torch.zeros(B, 3, H, 2 * W)[:, :, :, ::2], ("", ())),
        ("uint8 with sc != 1", u8(B, 3, H, 2 * W)[:, :, :, ::2], ValueError),
        ("uint8, H and W transposed", u8(B, 3, W, H).transpose(2, 3), ValueError),
        ("sx == 5", hwc(u8(B, H, W, 5)), ValueError),
        ("images that overlap", u8(B * H * W * 3).as_strided((B, 3, H, W), (W * 3, 1, W * 3, 3)), ValueError),
        ("ends short of its storage", u8(B * H * W * 4 - 1).as_strided((B, 3, H, W), (H * W * 4, 1, W * 4, 4)), ValueError),
    ]
    for name, t, want in table:
        if want is ValueError:
            with pytest.raises(ValueError):
                fovealseg.frames._frame_route(t)
            continue
        assert fovealseg.frames._frame_route(t) == want, name
        if t.dtype == torch.uint8:                                                         # the rule is byte_frame_layout's
            assert ops.byte_frame_layout(t) == (("planar",) if want[0] == "_u8" else ("hwc",) + want[1]), name
        with pytest.raises(hip.HipLibraryError):                                           # the device check stays at the call
            fovealseg.frames._frame_args(t, want[1])
    assert fovealseg.gaze._PROFILE_ENTRY == {"": "fs_frame_profiles", "_u8": "fs_key_profiles", "_hwc": "fs_frame_profiles_hwc"}
    for stem in ("fs_gate_tiles", "fs_gate_commit", "fs_state_shift"):
        assert all(stem + suffix in hip.SIGNATURES for suffix in ("", "_u8", "_hwc"))
    for stem in ("fs_gaze_lowres", "fs_grid_sample"):
        assert all(f"{stem}{suffix}_fwd" in hip.SIGNATURES for suffix in ("", "_u8", "_hwc"))


def test_deinterleaving_commutes_with_the_reference_passes():
    """The premise on the reference code: tiles, profiles and the border fill of an interleaved frame, computed on the bytes where they
    lie, are those of its de-interleaved copy -- whatever the alpha bytes and the pitch padding hold."""
    B, H, W, T_ = 2, 16, 24, 8
    rng = np.random.default_rng(5)
    planar = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    key = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    for name, sx in (("tight", 3), ("tight", 4), ("pitch5", 3), ("pitch16", 4), ("gap", 4), ("sb0", 3)):
        results = []
        for seed in (1, 2):                                                             # two fills of everything that is not a pixel
            f = Frame(planar, name, sx, seed)
            at = lambda b, c, y, x: int(f.buf[b * f.sb + y * f.sy + x * f.sx + c])
            assert np.array_equal(deinterleave(f.buf, f.sb, f.sy, f.sx, B, H, W), f.planar)
            sad = np.zeros((B, H // T_, W // T_), dtype=np.int64)
            prof = np.zeros((B, H + W), dtype=np.int64)
            for b in range(B):
                for y in range(H):
                    for x in range(W):
                        luma = 0
                        for c in range(3):
                            sad[b, y // T_, x // T_] += abs(at(b, c, y, x) - int(key[b, c, y, x]))
                            luma += at(b, c, y, x)
                        prof[b, y] += luma
                        prof[b, H + x] += luma
            moved = np.stack([M.move_key(key[b], as_float(f.planar[b]), 2, -3) for b in range(B)])
            direct = moved.copy()
            for b in range(B):
                for y in range(H):
                    for x in range(W):
                        if not (0 <= y - 2 < H and 0 <= x + 3 < W):
                            direct[b, :, y, x] = [at(b, c, y, x) for c in range(3)]
            assert np.array_equal(sad, R.tiles(as_float(f.planar), key, T_))
            assert np.array_equal(prof, M.key_profiles(f.planar))
            assert np.array_equal(direct, moved)
            results.append((sad, prof, direct))
        assert all(np.array_equal(a, b) for a, b in zip(*results))


def test_byte_ops_refuse_other_layouts_before_any_launch():
    B, H, W = 2, 16, 24
    key = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    bits = torch.zeros(B, H, 1, dtype=torch.int32)
    bad_views = (torch.zeros(B, 3, H, 2 * W, dtype=torch.uint8)[:, :, :, ::2], torch.zeros(B, 3, W, H, dtype=torch.uint8).transpose(2, 3),
                 torch.zeros(B, H, W, 5, dtype=torch.uint8).permute(0, 3, 1, 2)[:, :3])
    rec = [i64(B), i64(B, 6), torch.zeros(B, 5, dtype=torch.int32), bits]
    for bad in bad_views:
        assert tuple(bad.shape) == (B, 3, H, W) and ops.byte_frame_layout(bad) is None
        with pytest.raises(ValueError):
            ops.gate_tiles_u8(bad, key)
        with pytest.raises(ValueError):
            ops.gate_commit_u8(bad, None, key, i64(B, 6), torch.zeros(B, 2), rec, rec)
        with pytest.raises(ValueError):
            ops.key_profiles(bad)
        with pytest.raises(ValueError):
            ops.state_shift_u8(bad, i64(B, 4), key, key.clone(), bits, bits.clone(), i64(B, 6), i64(B, 6), torch.zeros(B, 5, dtype=torch.int32),
                               torch.zeros(B, H + W, dtype=torch.int32), i64(B, 4))
        with pytest.raises(ValueError):
            ops.grid_sample_u8(bad, torch.zeros(B, 4, 4, 2))
        with pytest.raises(ValueError):
            ops.gaze_lowres(bad, torch.zeros(B, 2), 4, 4)
    # pixels of four bytes whose last one lies outside the storage: refused, not read
    short = torch.zeros(B * H * W * 4 - 1, dtype=torch.uint8).as_strided((B, 3, H, W), (H * W * 4, 1, W * 4, 4))
    assert _layout(short) == ("hwc", H * W * 4, W * 4, 4) and ops.byte_frame_layout(short) is None
    with pytest.raises(ValueError):
        ops.gate_tiles_u8(short, key)


# ------------------------------------------------------------------------------------------------------------------ GPU: tiles ------
FRAME_HW = [(5, 16), (16, 24), (7, 33), (37, 48), (64, 64), (33, 1040)]


def _tiles_u8(planar, key, T_):
    B, _, H, W = planar.shape
    th, tw = -(-H // T_), -(-W // T_)
    gi, gk, sad = Guarded(planar.size, torch.uint8, body=torch.from_numpy(planar)), Guarded(key.size, torch.uint8, body=torch.from_numpy(key)), Guarded(B * th * tw)
    hip.call("fs_gate_tiles_u8", gi.ptr, gk.ptr, sad.ptr, B, H, W, T_)
    return sad.host(B, th, tw)


def _tiles_hwc(f, key, T_):
    th, tw = -(-f.H // T_), -(-f.W // T_)
    gi, gk, sad = f.guarded(), Guarded(key.size, torch.uint8, body=torch.from_numpy(key)), Guarded(f.B * th * tw)
    hip.call("fs_gate_tiles_hwc", *f.args(gi), gk.ptr, sad.ptr, f.B, f.H, f.W, T_)
    got = sad.host(f.B, th, tw)
    assert f.unchanged(gi) and gk.intact() and torch.equal(gk.body.cpu(), torch.from_numpy(key).reshape(-1))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", FRAME_HW)
def test_gate_tiles_hwc(H, W, B):
    rng = np.random.default_rng(H * 1009 + W * 7 + B)
    planar = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    key = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    routes = set()
    for n, T_ in enumerate((8, 16, 32, 64)):
        twins = {}
        for name, sx in CASES:
            f = Frame(planar, name, sx, seed=n)                                         # another fill of the garbage for every tile side
            one = LAYOUTS[name][2]
            if one not in twins:
                twins[one] = _tiles_u8(f.planar, key, T_)
                assert torch.equal(twins[one].long(), torch.from_numpy(R.tiles(as_float(f.planar), key, T_)))
            assert torch.equal(_tiles_hwc(f, key, T_), twins[one]), (name, sx, T_)
            routes.add((f.route, sx))
        # a frame equal to the key: nothing differs, whatever lies between the pixels
        for name, sx in (("tight", 3), ("pitch16", 4), ("pitch5", 4)):
            assert not bool(_tiles_hwc(Frame(key, name, sx, seed=9), key, T_).any())
    assert routes == ({(0, 3), (0, 4), (1, 3), (1, 4)} if W % 16 == 0 else {(0, 3), (0, 4)})
    # the op on a view of device bytes
    x = torch.from_numpy(planar).cuda()
    k = torch.from_numpy(key).cuda()
    rgba = torch.randint(0, 256, (B, H, W, 4), dtype=torch.uint8, device="cuda")
    rgba[..., :3] = x.permute(0, 2, 3, 1)
    for view in (x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), rgba.permute(0, 3, 1, 2)[:, :3]):
        assert not view.is_contiguous() and torch.equal(ops.gate_tiles_u8(view, k, 16), ops.gate_tiles_u8(x, k, 16))


@pytest.mark.gpu
def test_gate_tiles_hwc_one_byte_off_by_one():
    """The answer known by hand: one byte of one channel differs by one -> the tile that holds the pixel reads 1, every other 0."""
    B, H, W = 2, 37, 48
    rng = np.random.default_rng(41)
    key = rng.integers(1, 255, (B, 3, H, W)).astype(np.uint8)
    # the first and the last pixel of a lane's sixteen, both sides of a tile border of every T, the last pixel of the last ragged tile
    spots = [(0, 0, 0, 0), (1, 1, 3, 15), (0, 2, 8, 16), (1, 0, 7, 31), (0, 1, 31, 32), (1, 2, H - 1, W - 1), (0, 0, 36, 47), (1, 1, 32, 7)]
    for T_ in (8, 16, 32, 64):
        th, tw = -(-H // T_), -(-W // T_)
        for n, (b, c, y, x) in enumerate(spots):
            planar = key.copy()
            planar[b, c, y, x] = int(key[b, c, y, x]) + (1 if n % 2 else -1)
            want = torch.zeros(B, th, tw, dtype=torch.int32)
            want[b, y // T_, x // T_] = 1
            for name, sx in (("tight", 3), ("tight", 4), ("pitch5", 3), ("off1", 4)):
                assert torch.equal(_tiles_hwc(Frame(planar, name, sx, seed=n), key, T_), want), (T_, b, c, y, x, name, sx)
            assert torch.equal(_tiles_u8(planar, key, T_), want)


# ------------------------------------------------------------------------------------------------------------------ GPU: commit -----
def _commit(name, frame_args, gi, idx, key, gstate, focus, src, dst, B, H, W):
    n = len(idx)
    gk = Guarded(key.size, torch.uint8, body=torch.from_numpy(key))
    gs = Guarded(gstate.size, torch.int64, body=torch.from_numpy(gstate))
    gf = Guarded(focus.size, torch.float32, body=torch.from_numpy(focus))
    gd = [Guarded(d.size, dt, body=torch.from_numpy(d)) for d, dt in zip(dst, _REC_TYPES)]
    sd = [Guarded(max(s.size, 1), dt, body=torch.from_numpy(s) if s.size else None) for s, dt in zip(src, _REC_TYPES)]
    ix = torch.tensor(idx, dtype=torch.int32, device="cuda") if n else None
    sp = [g.ptr for g in sd] + [None] * (5 - len(sd))
    dp = [g.ptr for g in gd] + [None] * (5 - len(gd))
    hip.call(name, *frame_args, None if ix is None else ix.data_ptr(), n, gk.ptr, gs.ptr, gf.ptr, *sp, *dp, B, H, W, dst[2].shape[1])
    torch.cuda.synchronize()
    assert gi.intact() and gf.intact() and all(g.intact() for g in sd)
    return [gk.host(*key.shape), gs.host(B, 6)] + [g.host(*d.shape) for g, d in zip(gd, dst)]


def _profiles_hwc(f):
    gi, prof = f.guarded(), Guarded(f.B * (f.H + f.W))
    hip.call("fs_frame_profiles_hwc", *f.args(gi), prof.ptr, f.B, f.H, f.W)
    got = prof.host(f.B, f.H + f.W)
    assert f.unchanged(gi)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("W", [48, 37])
@pytest.mark.parametrize("conf", [False, True])
def test_gate_commit_hwc(W, conf):
    B, H, cap = 5, 9, 6
    rng = np.random.default_rng(300 + W + conf)
    planar = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    focus = rng.random((B, 2), dtype=np.float32)
    for n, idx in enumerate(([], list(range(B)), [1, 3], [0, 2, B + 3], [-1, 4])):     # the last two: an entry outside 0 .. B-1 writes nothing
        key = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)                      # what an untouched viewer must keep
        gstate = rng.integers(0, 1000, (B, 6))
        dst, src = _records(rng, B, H, W, cap, conf), _records(rng, len(idx), H, W, cap, conf)
        twins = {}
        for name, sx in CASES:
            f = Frame(planar, name, sx, seed=n)
            one = LAYOUTS[name][2]
            if one not in twins:
                gp = Guarded(f.planar.size, torch.uint8, body=torch.from_numpy(f.planar))
                twins[one] = _commit("fs_gate_commit_u8", (gp.ptr,), gp, idx, key, gstate, focus, src, dst, B, H, W)
            gi = f.guarded()
            got = _commit("fs_gate_commit_hwc", f.args(gi), gi, idx, key, gstate, focus, src, dst, B, H, W)
            assert f.unchanged(gi)
            for a, b in zip(got, twins[one]):
                assert torch.equal(_bits32(a), _bits32(b)), (name, sx, idx)
            for b in range(B):
                assert np.array_equal(got[0][b].numpy(), f.planar[b] if b in idx else key[b])      # a viewer outside idx keeps its key
            # the profile invariant after the commit: the frame's profiles are those of the key made from it
            ran = [b for b in idx if 0 <= b < B]
            assert np.array_equal(_profiles_hwc(f).numpy()[ran], M.key_profiles(got[0].numpy())[ran])
    # the op on views: a subset of viewers, and the key the tile pass then finds equal to the frame
    x = torch.from_numpy(planar).cuda()
    rgba = torch.randint(0, 256, (B, H, W, 4), dtype=torch.uint8, device="cuda")
    rgba[..., :3] = x.permute(0, 2, 3, 1)
    view = rgba.permute(0, 3, 1, 2)[:, :3]
    key = torch.full((B, 3, H, W), 0x3D, dtype=torch.uint8, device="cuda")
    gstate = torch.zeros(B, 6, dtype=torch.int64, device="cuda")
    rec = [torch.from_numpy(a).cuda() for a in _records(rng, B, H, W, cap, conf)]
    ops.gate_commit_u8(view, torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda"), key, gstate, torch.from_numpy(focus).cuda(),
                       [t[:3].contiguous() for t in rec], rec)
    assert torch.equal(key[[0, 2, 4]], x[[0, 2, 4]]) and bool((key[[1, 3]] == 0x3D).all()) and gstate[:, 0].tolist() == [1, 0, 1, 0, 1]
    assert ops.gate_tiles_u8(view, key, 8)[[0, 2, 4]].sum().item() == 0
    assert torch.equal(ops.key_profiles(view), ops.key_profiles(x))


# ------------------------------------------------------------------------------------------------------------------ GPU: profiles ---
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", FRAME_HW + [(70, 272)])                                  # the last: two bands and two 256-column segments
def test_frame_profiles_hwc(H, W, B):
    rng = np.random.default_rng(H * 31 + W + B)
    planar = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    planar[0, :, 0, :] = 255                                                             # a row of the largest luma
    twins = {}
    for name, sx in CASES:
        f = Frame(planar, name, sx, seed=sx)
        one = LAYOUTS[name][2]
        if one not in twins:
            gp, prof = Guarded(f.planar.size, torch.uint8, body=torch.from_numpy(f.planar)), Guarded(B * (H + W))
            hip.call("fs_key_profiles", gp.ptr, prof.ptr, B, H, W)
            twins[one] = prof.host(B, H + W)
            assert np.array_equal(twins[one].numpy(), M.key_profiles(f.planar))
        assert torch.equal(_profiles_hwc(f), twins[one]), (name, sx)


# ------------------------------------------------------------------------------------------------------------------ GPU: shift ------
def _shift(name, frame_args, gi, st, B, H, W):
    cap, P = st["counts"].shape[1], (W + 31) // 32
    gs = Guarded(B * 4, torch.int64, body=torch.from_numpy(st["shift"]))
    g = {k: Guarded(st[k].size, _STATE_TYPES[k], body=torch.from_numpy(np.ascontiguousarray(st[k]))) for k in _STATE_ORDER}
    key2, bits2 = Guarded(st["key"].size, torch.uint8), Guarded(B * H * P)
    motion = Guarded(B * 6, torch.int64)
    scratch = Guarded(hip.query("fs_state_shift_scratch_ints", B, H, W, cap))
    hip.call(name, *frame_args, gs.ptr, g["key"].ptr, key2.ptr, g["bits"].ptr, bits2.ptr, g["gstate"].ptr, g["stats"].ptr, g["counts"].ptr,
             g["prof_key"].ptr, g["mstate"].ptr, motion.ptr, scratch.ptr, B, H, W, cap)
    torch.cuda.synchronize()
    assert gi.intact() and gs.intact() and key2.intact() and bits2.intact() and scratch.intact()
    out = {k: g[k].host(*st[k].shape).numpy() for k in _STATE_ORDER}
    out["motion"] = motion.host(B, 6).numpy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(12, 40), (24, 64), (9, 37)])
def test_state_shift_hwc(H, W):
    B, cap, Rg = 3, 8 * W + 1, (min(H, W) - 1) // 4
    for n, (dy, dx) in enumerate(((1, 0), (0, -1), (Rg, -Rg), (0, 33), (-2, 3))):
        rng = np.random.default_rng(H * 1009 + W * 7 + n)
        shifts = [(dy, dx), (0, 0), (-dy, dx if dy else -dx)]                             # viewer 1 stands still beside two that move
        shape = (B, 3, H, W)
        masks = [rng.random((H, W)) < 0.5 for _ in range(B)]
        planar = rng.integers(0, 256, shape).astype(np.uint8)
        st = dict(key=rng.integers(0, 256, shape).astype(np.uint8), bits=np.stack([RLE.bits(m) for m in masks]),
                  gstate=rng.integers(0, 16 * min(H, W), (B, 6)), mstate=rng.integers(-50, 50, (B, 4)),
                  shift=np.array([[a, b, int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 40))] for a, b in shifts], dtype=np.int64),
                  stats=rng.integers(0, 99, (B, 6)), counts=rng.integers(0, 99, (B, cap)).astype(np.int32),
                  prof_key=rng.integers(0, 99, (B, H + W)).astype(np.int32))
        twins = {}
        for name, sx in (CASES if n == 0 else [("tight", 3), ("pitch5", 4), ("sb0", 4), ("pitch16", 3)]):
            f = Frame(planar, name, sx, seed=n)
            one = LAYOUTS[name][2]
            if one not in twins:
                gp = Guarded(f.planar.size, torch.uint8, body=torch.from_numpy(f.planar))
                twins[one] = _shift("fs_state_shift_u8", (gp.ptr,), gp, st, B, H, W)
            gi = f.guarded()
            got = _shift("fs_state_shift_hwc", f.args(gi), gi, st, B, H, W)
            assert f.unchanged(gi)
            for k in twins[one]:
                assert np.array_equal(got[k], twins[one][k]), (k, name, sx, shifts)
            for k in _STATE_ORDER:
                assert np.array_equal(got[k][1], st[k][1]), k                               # the still viewer: untouched, garbage included
            for b in (0, 2):                                                              # the profile invariant after the move
                assert np.array_equal(got["prof_key"][b], M.key_profiles(got["key"][b:b + 1])[0])
        want = dict(zip(_STATE_ORDER + ("motion",), M.state_shift(as_float(planar), st["shift"], *(st[k] for k in _STATE_ORDER))))
        for k in want:
            assert np.array_equal(twins[False][k], want[k]), k
    # the op on a view of device bytes
    x = torch.from_numpy(planar).cuda()
    dev = {k: torch.from_numpy(np.ascontiguousarray(st[k])).cuda() for k in _STATE_ORDER + ("shift",)}
    motion = ops.state_shift_u8(x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), dev["shift"], dev["key"], torch.zeros_like(dev["key"]),
                                dev["bits"], torch.zeros_like(dev["bits"]), dev["gstate"], dev["stats"], dev["counts"], dev["prof_key"], dev["mstate"])
    assert np.array_equal(motion.cpu().numpy(), want["motion"]) and all(np.array_equal(dev[k].cpu().numpy(), want[k]) for k in _STATE_ORDER)


# ------------------------------------------------------------------------------------------------------------------ GPU: front ------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W,hs,ws", [(37, 53, 8, 6), (64, 64, 16, 16), (5, 7, 8, 9)])
def test_gaze_lowres_hwc(H, W, hs, ws):
    B = 2
    rng = np.random.default_rng(H * 1009 + W)
    planar = _all_bytes_frame(rng, B, 3, H, W)
    for f0 in (0.0, 1.0, 0.37):
        focus = np.full((B, 2), f0, dtype=np.float32)
        twins = {}
        for name, sx in CASES:
            f = Frame(planar, name, sx, seed=sx)
            one = LAYOUTS[name][2]
            if one not in twins:
                gp, gf, out = Guarded(f.planar.size, torch.uint8, body=torch.from_numpy(f.planar)), Guarded(focus.size, torch.float32, body=torch.from_numpy(focus)), Guarded(B * hs * ws * 5, torch.float32)
                hip.call("fs_gaze_lowres_u8_fwd", gp.ptr, gf.ptr, out.ptr, B, H, W, hs, ws)
                twins[one] = out.host(B, hs, ws, 5)
            gi, gf, out = f.guarded(), Guarded(focus.size, torch.float32, body=torch.from_numpy(focus)), Guarded(B * hs * ws * 5, torch.float32)
            hip.call("fs_gaze_lowres_hwc_fwd", *f.args(gi), gf.ptr, out.ptr, B, H, W, hs, ws)
            got = out.host(B, hs, ws, 5)
            assert f.unchanged(gi) and gf.intact()
            assert torch.equal(got.view(torch.int32), twins[one].view(torch.int32)), (name, sx, f0)
    x, fo = torch.from_numpy(planar).cuda(), torch.tensor([[0.2, 0.9], [0.5, 0.5]], device="cuda")
    view = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert torch.equal(ops.gaze_lowres(view, fo, hs, ws).view(torch.int32), ops.gaze_lowres(x, fo, hs, ws).view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("nhwc", [0, 1])
def test_grid_sample_hwc(nhwc):
    B, H, W, h, w = 2, 11, 13, 6, 5
    rng = np.random.default_rng(70 + nhwc)
    planar = _all_bytes_frame(rng, B, 3, H, W)
    grid = (rng.random((B, h, w, 2), dtype=np.float32) * 2.2 - 1.1)
    g = grid.reshape(-1, 2)
    g[0], g[1], g[2], g[3] = (-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0)                     # the corners of the grid's range, exactly
    g[4], g[5] = (-1.0 - 1.0 / W, 0.3), (0.2, 1.0 + 1.0 / H)                                         # half a pixel outside
    g[6], g[7], g[8] = (1e30, 0.0), (0.0, -1e30), (np.float32("nan"), np.float32("nan"))             # far outside, and no point at all
    twins = {}
    for name, sx in CASES:
        f = Frame(planar, name, sx, seed=sx)
        one = LAYOUTS[name][2]
        if one not in twins:
            gp, gg, out = Guarded(f.planar.size, torch.uint8, body=torch.from_numpy(f.planar)), Guarded(grid.size, torch.float32, body=torch.from_numpy(grid)), Guarded(B * h * w * 3, torch.float32)
            hip.call("fs_grid_sample_u8_fwd", gp.ptr, gg.ptr, out.ptr, B, 3, H, W, h, w, nhwc)
            twins[one] = out.host(B * h * w * 3)
            assert bool(twins[one].isnan().any()) and bool((twins[one] > 0).any())                   # the NaN point and real samples are both there
        gi, gg, out = f.guarded(), Guarded(grid.size, torch.float32, body=torch.from_numpy(grid)), Guarded(B * h * w * 3, torch.float32)
        hip.call("fs_grid_sample_hwc_fwd", *f.args(gi), gg.ptr, out.ptr, B, H, W, h, w, nhwc)
        got = out.host(B * h * w * 3)
        assert f.unchanged(gi) and gg.intact()
        assert torch.equal(got.view(torch.int32), twins[one].view(torch.int32)), (name, sx)
    if nhwc:
        x, gd = torch.from_numpy(planar).cuda(), torch.from_numpy(grid).cuda()
        view = x.contiguous(memory_format=torch.channels_last)
        assert not view.is_contiguous() and torch.equal(ops.grid_sample_u8(view, gd).view(torch.int32), ops.grid_sample_u8(x, gd).view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ GPU: one frame, five layouts
@pytest.mark.gpu
@pytest.mark.parametrize("T_", [8, 16])
@pytest.mark.parametrize("H,W", [(24, 64), (9, 37)])      # vector routes, a 16-pixel piece over two tiles at T = 8 | one-pixel routes, ragged tiles, a partial bit word
def test_every_pass_agrees_across_the_five_layouts(H, W, T_):
    """One random byte frame as fp32 (byte / 255), planar bytes, tight RGB, RGBA and RGB with a pitch of W * 3 + 5 from a base one byte off
    (the one-pixel route at any W), through every op that reads a frame: all results torch.equal, the interleaved buffers unchanged."""
    B, cap, hs, ws = 2, 16, 5, 7
    gen = torch.Generator().manual_seed(H * 1009 + W * 7 + T_)
    rnd = lambda *s: torch.randint(0, 256, s, generator=gen, dtype=torch.uint8)
    planar = rnd(B, 3, H, W).cuda()
    hwc_of = planar.permute(0, 2, 3, 1)
    rgb_buf = hwc_of.contiguous()
    rgba_buf = rnd(B, H, W, 4).cuda()
    rgba_buf[..., :3] = hwc_of
    pitch = W * 3 + 5
    off_buf = rnd(1 + B * H * pitch).cuda()
    off_view = off_buf.as_strided((B, 3, H, W), (H * pitch, 1, pitch, 3), 1)
    off_view.copy_(planar)
    frames = {"fp32": floats(planar), "planar": planar, "rgb": rgb_buf.permute(0, 3, 1, 2), "rgba": rgba_buf.permute(0, 3, 1, 2)[:, :3],
              "pitch5 off1": off_view}
    bufs = {"rgb": rgb_buf, "rgba": rgba_buf, "pitch5 off1": off_buf}
    before = {k: v.clone() for k, v in bufs.items()}
    want_route = 1 if W % 16 == 0 else 0
    for name, want in (("rgb", want_route), ("rgba", want_route), ("pitch5 off1", 0)):     # each view runs the route it is there for
        suffix, (sb, sy, sx) = fovealseg.frames._frame_route(frames[name])
        assert suffix == "_hwc" and hip.load().fs_byte_frame_route(frames[name].data_ptr(), sb, sy, sx, W) == want, name
    by_dtype = lambda f32_op, u8_op, x: f32_op if x.dtype == torch.float32 else u8_op

    key = rnd(B, 3, H, W).cuda()
    focus = torch.tensor([[0.2, 0.9], [0.5, 0.5]], device="cuda")
    mask = np.zeros((H, W), dtype=bool)
    mask[2:H - 2, W - 9:W - 1] = True                                                      # reaches the partial bit word at W = 37
    bits = torch.from_numpy(np.stack([RLE.bits(mask), RLE.bits(mask[::-1].copy())])).cuda()
    i64 = lambda *s: torch.randint(0, 16 * (min(H, W) - 1), s, generator=gen, dtype=torch.int64).cuda()
    gstate, mstate, stats = i64(B, 6), i64(B, 4), i64(B, 6)
    counts = torch.zeros(B, cap, dtype=torch.int32, device="cuda")
    shift = torch.tensor([[1, -2, 11, 22], [-2, 1, 33, 44]], dtype=torch.int64, device="cuda")          # within motion_px = 2: 4 R < min(H, W) at H = 9
    grid = (torch.rand(B, 6, 5, 2, generator=gen) * 2.2 - 1.1).cuda()
    idx = torch.tensor([1], dtype=torch.int32, device="cuda")

    results = {}
    for name, x in frames.items():
        out = {"tiles": by_dtype(ops.gate_tiles, ops.gate_tiles_u8, x)(x, key, T_)}
        k, g = key.clone(), gstate.clone()
        rec = (torch.zeros(B, dtype=torch.int64, device="cuda"), stats.clone(), counts.clone(), bits.clone())
        by_dtype(ops.gate_commit, ops.gate_commit_u8, x)(x, idx, k, g, focus, rec, rec)
        out["commit key"], out["commit gstate"] = k, g
        out["profiles"] = by_dtype(ops.frame_profiles, ops.key_profiles, x)(x)
        st = dict(key=key.clone(), bits=bits.clone(), gstate=gstate.clone(), stats=stats.clone(), counts=counts.clone(),
                  prof_key=ops.key_profiles(key), mstate=mstate.clone())
        out["motion"] = by_dtype(ops.state_shift, ops.state_shift_u8, x)(x, shift, st["key"], torch.zeros_like(key), st["bits"], torch.zeros_like(bits),
                                                                         st["gstate"], st["stats"], st["counts"], st["prof_key"], st["mstate"])
        out.update({"shift " + k_: v for k_, v in st.items()})
        out["lowres"] = ops.gaze_lowres(x, focus, hs, ws)
        out["sample"] = ops.GridSample.apply(x, grid) if x.dtype == torch.float32 else ops.grid_sample_u8(x, grid)
        results[name] = out
    torch.cuda.synchronize()
    want = results["planar"]
    assert bool(want["tiles"].any()) and not torch.equal(want["shift key"], key) and torch.equal(want["commit key"][1], planar[1])
    assert torch.equal(want["commit key"][0], key[0]) and want["motion"][:, :2].tolist() == [[1, -2], [-2, 1]]
    for name, got in results.items():
        for what in want:
            assert got[what].dtype == want[what].dtype and torch.equal(got[what], want[what]), (name, what)
    for name, buf in bufs.items():
        assert torch.equal(buf, before[name]), name


# ------------------------------------------------------------------------------------------------------------------ GPU: refusals ---
@pytest.mark.gpu
def test_interleaved_entry_points_reject_bad_arguments():
    B, H, W, T_, cap = 2, 16, 24, 8, 5
    sx, sy = 4, 24 * 4 + 8
    sb = H * sy
    img, key, key2 = Guarded(B * sb, torch.uint8), Guarded(B * 3 * H * W, torch.uint8), Guarded(B * 3 * H * W, torch.uint8)
    sad, low, samp = Guarded(B * 6), Guarded(B * 4 * 4 * 5, torch.float32), Guarded(B * 4 * 4 * 3, torch.float32)
    gstate, stats, mstate = Guarded(B * 6, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * 4, torch.int64)
    focus, grid = Guarded(B * 2, torch.float32), Guarded(B * 4 * 4 * 2, torch.float32)
    bits, bits2, prof_key, prof = Guarded(B * H), Guarded(B * H), Guarded(B * (H + W)), Guarded(B * (H + W))
    shift, motion, counts = Guarded(B * 4, torch.int64, body=torch.ones(B * 4)), Guarded(B * 6, torch.int64), Guarded(B * cap)
    scratch = Guarded(hip.query("fs_state_shift_scratch_ints", B, H, W, cap))
    rec = [Guarded(B, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * cap), Guarded(B * H), Guarded(B * 3, torch.float32)]
    idx = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    outs = [img, key, key2, sad, low, samp, gstate, stats, mstate, bits, bits2, prof_key, prof, motion, counts, scratch] + rec
    # the description itself: no frame, sx outside {3, 4}, rows that overlap, a negative batch stride, images that overlap
    frame_bads = ((0, None), (3, 5), (3, 2), (3, 0), (2, W * sx - 1), (2, 0), (1, -sb), (1, sb - 1), (1, 1))

    def each(name, good, bads):
        for i, bad in frame_bads + tuple(bads):
            a = list(good)
            a[i] = bad
            with pytest.raises(hip.HipLibraryError, match="argument rejected"):
                hip.call(name, *a)
            torch.cuda.synchronize()
            assert all(g.intact() and bool((g.body == _GARB[g.dtype]).all()) for g in outs), f"a rejected {name} launched something"

    fr = [img.ptr, sb, sy, sx]
    each("fs_gate_tiles_hwc", fr + [key.ptr, sad.ptr, B, H, W, T_], ((4, None), (5, None), (6, 0), (7, 0), (8, -1), (9, 12), (9, 0), (9, 128)))
    each("fs_gaze_lowres_hwc_fwd", fr + [focus.ptr, low.ptr, B, H, W, 4, 4], ((4, None), (5, None), (6, 0), (7, 0), (8, -1), (9, 1), (10, 0)))
    each("fs_grid_sample_hwc_fwd", fr + [grid.ptr, samp.ptr, B, H, W, 4, 4, 1], ((4, None), (5, None), (6, 0), (7, 0), (8, -1), (9, 0), (10, 0)))
    each("fs_frame_profiles_hwc", fr + [prof.ptr, B, H, W], ((4, None), (5, 0), (6, 0), (7, -1)))
    ptrs = [g.ptr for g in rec]
    each("fs_gate_commit_hwc", fr + [idx.data_ptr(), 2, key.ptr, gstate.ptr, focus.ptr, *ptrs, *ptrs, B, H, W, cap],
         ((4, None), (5, 3), (5, -1), (6, None), (7, None), (8, None), (9, None), (12, None), (14, None), (17, None), (18, None),
          (19, 0), (20, 0), (21, 0), (22, 0)))
    good = fr + [shift.ptr, key.ptr, key2.ptr, bits.ptr, bits2.ptr, gstate.ptr, stats.ptr, counts.ptr, prof_key.ptr, mstate.ptr, motion.ptr,
                 scratch.ptr, B, H, W, cap]
    each("fs_state_shift_hwc", good, [(i, None) for i in range(4, 16)] + [(6, key.ptr), (8, bits.ptr), (15, scratch.ptr + 4), (16, 0), (17, 0), (18, 0), (19, 0)])
    route = hip.load().fs_byte_frame_route
    assert route(img.ptr, sb, sy, sx, W) == 0 and route(img.ptr, sb, sy, sx, 16) == 0               # the width; a pitch of 104 bytes
    assert route(img.ptr, 16 * 112, 112, 4, 16) == 1 and route(img.ptr + 1, 16 * 112, 112, 4, 16) == 0
    assert route(img.ptr, 0, 48, 3, 16) == 1 and route(img.ptr, 0, 53, 3, 16) == 0 and route(img.ptr, 8, 48, 3, 16) == 0
    for bad in ((None, sb, sy, sx, W), (img.ptr, -16, sy, sx, W), (img.ptr, sb, W * sx - 1, sx, W), (img.ptr, sb, sy, 5, W), (img.ptr, sb, sy, sx, 0)):
        assert route(*bad) == -1
    # B == 1: the batch stride is not looked at beyond its sign
    hip.call("fs_gate_tiles_hwc", img.ptr, 1, sy, sx, key.ptr, sad.ptr, 1, H, W, T_)
    torch.cuda.synchronize()
    assert sad.intact()


# ------------------------------------------------------------------------------------------------------------------ GPU: module -----
def _views(U, seed=0):
    """The same bytes as views of interleaved buffers whose other bytes are random: RGB, RGBA and a pitched crop of a larger RGBA buffer."""
    B, _, H, W = U.shape
    gen = torch.Generator(device="cuda").manual_seed(100 + seed)
    hwc = U.permute(0, 2, 3, 1)
    rgb = hwc.contiguous().permute(0, 3, 1, 2)
    buf = torch.randint(0, 256, (B, H, W, 4), dtype=torch.uint8, device="cuda", generator=gen)
    buf[..., :3] = hwc
    big = torch.randint(0, 256, (B, H + 5, W + 16, 4), dtype=torch.uint8, device="cuda", generator=gen)
    big[:, 3:3 + H, 8:8 + W, :3] = hwc
    views = dict(rgb=rgb, rgba=buf.permute(0, 3, 1, 2)[:, :3], crop=big[:, 3:3 + H, 8:8 + W, :3].permute(0, 3, 1, 2))
    for v in views.values():
        assert not v.is_contiguous() and ops.byte_frame_layout(v)[0] == "hwc" and torch.equal(v, U)
    return views


@pytest.mark.gpu
def test_module_reads_interleaved_frames(served):
    module, calls, TP = served
    X, Fp, Y, cl = T.synthetic_batch(2, SIZE, SIZE, seed=SEED, device="cuda")
    U = _bytes_of(X)
    kw = dict(return_bits=True, return_score=True)
    want = (module.predict(U, Fp), module.predict_instances(U, Fp, **kw), module.evaluate(U, Fp, Y, cl, class_areas=True),
            module.evaluate_instances(U, Fp, Y, cl, component=8))
    assert 0 < int(want[1][1][0, 0]) < SIZE * SIZE
    views = _views(U)
    for name, V in views.items():
        V0 = V.clone()
        assert torch.equal(module.predict(V, Fp), want[0]), name
        assert _same(module.predict_instances(V, Fp, **kw), want[1])
        assert _same(module.evaluate(V, Fp, Y, cl, class_areas=True), want[2])
        assert _same(module.evaluate_instances(V, Fp, Y, cl, component=8), want[3])
        assert torch.equal(V, V0)
    module.check_nan()
    # nothing of the frame's size is made in front of the call: the view's peak is not above the planar call's
    ph, pp = _peak_of(lambda: module.predict_instances(views["rgba"], Fp)), _peak_of(lambda: module.predict_instances(U, Fp))
    print(f"predict_instances raised the peak by {ph} bytes fed an RGBA view and by {pp} fed planar uint8")
    assert ph <= pp


# ------------------------------------------------------------------------------------------------------------------ GPU: session ----
def _grew(call):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = call()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def _step_all(sessions, feeds, U, Fp, force=None, seed=0):
    """One step of every session on the same bytes, each fed its own layout; all results and states must agree.  Returns the first result."""
    views = dict(_views(U, seed), u8=U)
    outs = [s.step(views[feed] if feed != "f32" else floats(U), Fp, force=force) for s, feed in zip(sessions, feeds)]
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
def test_session_on_interleaved_bytes_equals_the_session_on_planar_bytes(served):
    module, calls, TP = served
    H = W = SIZE
    X, Fp = TP._batch(2, SIZE, SEED)
    U = _bytes_of(X)
    U0 = U.clone()
    sessions = [GazeSession(module, 2, (H, W), score=True) for _ in range(3)]
    alt = _cycle("crop", "u8", "rgb", "f32", "rgba")                                     # the layout may change from step to step
    feed = lambda: ("u8", "rgba", next(alt))
    *rec, gate = _step_all(sessions, feed(), U, Fp)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and all(torch.equal(s._key, U) for s in sessions)       # the key stays planar
    held = [t.clone() for t in rec]
    *rec, gate = _step_all(sessions, feed(), U, Fp, seed=1)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and gate[:, 1:6].tolist() == [[0] * 5] * 2 and _same(rec, held)
    # a REUSE step fed a view allocates nothing (the parent copies the view: 3 * B * H * W bytes)
    views = _views(U, 2)
    for s, name in zip(sessions[1:], ("rgb", "crop")):
        grew, out = _grew(lambda: s.step(views[name], Fp))
        print(f"a REUSE step fed the {name} view raised the peak by {grew} bytes")
        assert grew == 0 and out[-1][:, 0].tolist() == [R.REUSE] * 2
    sessions[0].step(U, Fp)
    # a flipped tile inside viewer 1's box: RUN_ROI, a partial run
    box_tile = (int(held[1][1, 2]) // 32, int(held[1][1, 1]) // 32)
    U4 = _bytes_of(_flip_tile(floats(U), 1, *box_tile))
    *rec, gate = _step_all(sessions, feed(), U4, Fp, seed=3)
    assert gate[:, 0].tolist() == [R.REUSE, R.RUN_ROI]
    assert _same(tuple(t[1:2] for t in rec), module.predict_instances(U4[1:2], Fp[1:2], return_bits=True, return_score=True))
    # a partial run fed a view gathers the running viewers' bytes as they lie: its peak is not above the planar step's, which selects
    # 3 * H * W bytes a running viewer (a planar copy on top of the gathered rows would add as much again)
    V4 = _views(U4, 4)
    g_planar, out_p = _grew(lambda: sessions[0].step(U4, Fp, force=[0, 1]))
    g_view, out_v = _grew(lambda: sessions[1].step(V4["rgb"], Fp, force=[0, 1]))
    print(f"a partial run raised the peak by {g_view} bytes fed the rgb view and by {g_planar} fed planar bytes")
    assert g_view <= g_planar and out_v[-1][:, 0].tolist() == [R.REUSE, R.RUN_FORCED] and _same(tuple(out_p), tuple(out_v))
    assert _same(tuple(sessions[2].step(V4["crop"], Fp, force=[0, 1])), tuple(out_p))
    for a, b, c in zip(*(_state_of(s) for s in sessions)):
        assert torch.equal(_bits32(a), _bits32(b)) and torch.equal(_bits32(a), _bits32(c))
    assert torch.equal(U, U0) and sessions[0].counts[R.REUSE] >= 5 and all(s.counts == sessions[0].counts for s in sessions)


@pytest.mark.gpu
def test_session_on_one_frame_for_every_viewer(served):
    """sb == 0: one camera frame expanded over the viewers, against its planar copy; a partial run selects the same view with a smaller B."""
    module, calls, TP = served
    X, Fp = TP._batch(2, SIZE, SEED)
    U1 = _bytes_of(X)[:1]
    one = _views(U1)["rgba"].expand(2, 3, SIZE, SIZE)
    assert ops.byte_frame_layout(one) == ("hwc", 0, SIZE * 4, 4)
    planar = U1.expand(2, 3, SIZE, SIZE).contiguous()
    pair = [GazeSession(module, 2, (SIZE, SIZE)) for _ in range(2)]
    for force, codes in ((None, [R.RUN_INIT] * 2), (None, None), ([0, 1], None), ([1, 0], None)):
        a, b = pair[0].step(planar, Fp, force=force), pair[1].step(one, Fp, force=force)
        assert _same(tuple(a), tuple(b)) and pair[0].counts == pair[1].counts
        assert codes is None or a[-1][:, 0].tolist() == codes
        for s, t in zip(_state_of(pair[0]), _state_of(pair[1])):
            assert torch.equal(_bits32(s), _bits32(t))
    assert pair[0].counts[R.RUN_FORCED] == 2
    grew, out = _grew(lambda: pair[1].step(one, Fp))
    assert grew == 0 and all(c not in R.RUNS for c in out[-1][:, 0].tolist())


@pytest.mark.gpu
def test_moving_session_on_interleaved_bytes_equals_the_session_on_planar_bytes(served):
    module, calls, TP = served
    PAD = 16

    def frames(windows):
        out = [M.window(M.canvas(seed, SIZE + 2 * PAD, SIZE + 2 * PAD, 4), y, x, SIZE, SIZE) for seed, y, x in windows]
        return _bytes_of(torch.from_numpy(np.stack(out)).cuda())

    focus = lambda pixels: torch.tensor([[py / (SIZE - 1), px / (SIZE - 1)] for py, px in pixels], dtype=torch.float32, device="cuda")
    U1, F1 = frames([(25, PAD, PAD), (31, PAD, PAD)]), focus([(128, 128), (100, 140)])
    U2, F2 = frames([(25, PAD - 3, PAD + 5), (31, PAD, PAD)]), focus([(131, 123), (100, 140)])       # the content moves by (3, -5)
    U3, F3 = frames([(25, PAD - 1, PAD + 4), (31, PAD, PAD)]), focus([(129, 124), (100, 140)])       # and by a further (-2, 1)
    sessions = [GazeSession(module, 2, (SIZE, SIZE), motion_px=5) for _ in range(3)]
    alt = _cycle("rgb", "u8", "crop")
    feed = lambda: ("u8", "rgba", next(alt))
    *rec, gate, motion = _step_all(sessions, feed(), U1, F1)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and motion.tolist() == [[0] * 6] * 2
    assert torch.equal(sessions[1]._prof_key, ops.key_profiles(U1))
    *rec, gate, motion = _step_all(sessions, feed(), U2, F2, seed=1)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and motion[:, :2].tolist() == [[3, -5], [0, 0]]
    assert torch.equal(sessions[1]._prof_key, ops.key_profiles(sessions[1]._key))
    # a moved REUSE step fed a view allocates nothing
    V3 = _views(U3, 2)
    out = sessions[0].step(U3, F3)
    for s, name in zip(sessions[1:], ("rgba", "crop")):
        grew, o = _grew(lambda: s.step(V3[name], F3))
        print(f"a moved REUSE step fed the {name} view raised the peak by {grew} bytes")
        assert grew == 0 and _same(tuple(out), tuple(o))
    assert out[-2][:, 0].tolist() == [R.REUSE] * 2 and out[-1][:, :2].tolist() == [[-2, 1], [0, 0]] and out[-1][:, 4:].tolist() == [[1, -4], [0, 0]]
    for a, b, c in zip(*(_state_of(s) for s in sessions)):
        assert torch.equal(_bits32(a), _bits32(b)) and torch.equal(_bits32(a), _bits32(c))
