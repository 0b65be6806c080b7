"""Frames as bytes: fs_gaze_lowres_u8_fwd, fs_grid_sample_u8_fwd, fs_gate_tiles_u8, fs_gate_commit_u8, fs_state_shift_u8, their ops, and
the dtype dispatch of predict* / evaluate* / GazeSession.step.

A uint8 frame's pixel value is byte / 255 and its pixel code is the byte, so the uint8 route must equal the fp32 route fed byte / 255
in fp32, correctly rounded (`floats` below), bit for bit.  Every comparison is torch.equal (float tensors as int32 views) against code
that its own tests already hold to fp64, to the goldens, or to tests/gate_ref.py and tests/motion_ref.py.  The CPU tests check the premise on the reference code
first.  At the C ABI every output sits between sentinel guard bands and is pre-filled with garbage."""
import numpy as np
import pytest
import torch

from fovealseg import hip, ops
from fovealseg import train as T
from fovealseg.session import GazeSession

import gate_ref as R
import motion_ref as M
import rle_ref as RLE
from test_gaze_session import Guarded, _GARB, _same, _flip_tile, _focus_at, _pixel, served       # noqa: F401  (served is a fixture)

F255 = np.float32(255)


def as_float(u8):
    """The fp32 frame of a byte frame, as numpy computes byte / 255 in fp32 (correctly rounded, as torch and the kernels do)."""
    return u8.astype(np.float32) / F255


def floats(U):
    """The fp32 frame of a byte tensor on the device: byte / 255 correctly rounded, computed on the host.  On the device torch divides by
    a Python scalar by multiplying with its reciprocal, which is one ulp off the quotient for some bytes."""
    return (U.cpu().float() / 255).to(U.device)


def _bits32(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------------------------ CPU ------------
def test_the_ctypes_table_binds_the_byte_entry_points():
    assert hip.SIGNATURES["fs_gaze_lowres_u8_fwd"] == hip.SIGNATURES["fs_gaze_lowres_fwd"] == "ppp" + "iiiii"
    assert hip.SIGNATURES["fs_grid_sample_u8_fwd"] == hip.SIGNATURES["fs_grid_sample_fwd"] == "ppp" + "iiiiiii"
    assert hip.SIGNATURES["fs_gate_tiles_u8"] == hip.SIGNATURES["fs_gate_tiles"] == "ppp" + "iiii"
    assert hip.SIGNATURES["fs_gate_commit_u8"] == hip.SIGNATURES["fs_gate_commit"] == "pp" + "i" + "p" * 13 + "iiii"
    assert hip.SIGNATURES["fs_state_shift_u8"] == hip.SIGNATURES["fs_state_shift"] == "p" * 13 + "iiii"
    for name in ("gate_tiles_u8", "gate_commit_u8", "state_shift_u8", "grid_sample_u8"):
        assert callable(getattr(ops, name))


def test_the_pixel_code_of_a_byte_is_the_byte():
    k = np.arange(256)
    assert R.q(k.astype(np.float32) / F255).tolist() == k.tolist()
    # the 16 x 24 hand frame of tests/test_gaze_session.py in bytes: the sad table of byte / 255 is the plain integer sum over the bytes
    rng = np.random.default_rng(3)
    key = np.full((1, 3, 16, 24), 10, dtype=np.uint8)
    img = key.copy()
    img[0, 0, 0, 0], img[0, 2, 7, 23], img[0, 2, 15, 23], img[0, 0, 15, 23] = 13, 0, 0, 255
    img[0, 1, 8:16, 8:16] = 12
    assert R.tiles(as_float(img), key, 8).tolist() == [[[3, 0, 10], [0, 128, 255]]]
    for a, b in ((img, key), (rng.integers(0, 256, img.shape).astype(np.uint8), rng.integers(0, 256, img.shape).astype(np.uint8))):
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        for T_ in (8, 16):
            th, tw = -(-16 // T_), -(-24 // T_)
            plain = [[[int(d[0, :, ty * T_:(ty + 1) * T_, tx * T_:(tx + 1) * T_].sum()) for tx in range(tw)] for ty in range(th)]]
            assert R.tiles(as_float(a), b, T_).tolist() == plain
    # and the profiles of such a frame are the key's
    assert np.array_equal(M.frame_profiles(as_float(img)), M.key_profiles(img))


def test_byte_ops_refuse_before_any_launch():
    B, H, W = 2, 16, 24
    u8 = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    key = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    bits = torch.zeros(B, H, 1, dtype=torch.int32)
    prof = torch.zeros(B, H + W, dtype=torch.int32)
    bad_imgs = (u8.float(), u8.int(), u8[:, :2], u8[:0], u8.numpy())
    for bad in bad_imgs:
        with pytest.raises(ValueError):
            ops.gate_tiles_u8(bad, key)
    for bad_key in (key[:1], key[:, :, :8], key.int()):
        with pytest.raises(ValueError):
            ops.gate_tiles_u8(u8, bad_key)
    with pytest.raises(ValueError):
        ops.gate_tiles_u8(u8, key, tile=12)
    rec = [i64(B), i64(B, 6), torch.zeros(B, 5, dtype=torch.int32), bits]
    commit = dict(img=u8, idx=None, key=key, gstate=i64(B, 6), focus=torch.zeros(B, 2), src=rec, dst=rec)
    for k, v in [("img", b) for b in bad_imgs] + [("key", key[:1]), ("key", key.int()), ("gstate", i64(B, 5)), ("idx", torch.zeros(1, dtype=torch.int64))]:
        with pytest.raises(ValueError):
            ops.gate_commit_u8(**dict(commit, **{k: v}))
    shift = dict(img=u8, shift=i64(B, 4), key=key, key2=key.clone(), bits=bits, bits2=bits.clone(), gstate=i64(B, 6), stats=i64(B, 6),
                 counts=torch.zeros(B, 5, dtype=torch.int32), prof_key=prof, mstate=i64(B, 4))
    for k, v in [("img", b) for b in bad_imgs] + [("key", key[:1]), ("key2", key), ("key2", key[:, :, :8]), ("bits2", bits), ("shift", i64(B, 2))]:
        with pytest.raises(ValueError):
            ops.state_shift_u8(**dict(shift, **{k: v}))
    grid = torch.zeros(B, 4, 4, 2)
    for bad in (u8.float(), u8.int(), u8[:0], u8[0]):
        with pytest.raises(ValueError):
            ops.grid_sample_u8(bad, grid)
    for bad_grid in (grid[:1], grid[..., :1], grid.double()):
        with pytest.raises(ValueError):
            ops.grid_sample_u8(u8, bad_grid)
    # the fp32 names keep refusing bytes
    for call in (lambda: ops.gate_tiles(u8, key), lambda: ops.gate_commit(**commit), lambda: ops.state_shift(**shift), lambda: ops.frame_profiles(u8)):
        with pytest.raises(ValueError):
            call()


class _Stub:
    training = False


def test_session_refuses_byte_frames_of_the_wrong_shape_or_device():
    s = GazeSession(_Stub(), 2, (64, 48))
    X, Fp = torch.zeros(2, 3, 64, 48, dtype=torch.uint8), torch.zeros(2, 2)
    for img in (X[:1], X[:, :, :32], X[:, :2], X.transpose(2, 3), X.int(), X.double(), X):          # the last: the right shape, on the CPU
        with pytest.raises(ValueError):
            s.step(img, Fp if img.shape[0] == 2 else Fp[:1])
    assert s.counts == {c: 0 for c in range(8)}


# ------------------------------------------------------------------------------------------------------------------ GPU: tiles ------
def _tiles_abi(name, img, key, T_, off=False):
    B, _, H, W = img.shape
    th, tw = -(-H // T_), -(-W // T_)
    dt = torch.uint8 if img.dtype == np.uint8 else torch.float32
    gi = Guarded(img.size, dt, body=torch.from_numpy(img), off=1 if off else 0)
    gk = Guarded(key.size, torch.uint8, body=torch.from_numpy(key), off=1 if off else 0)
    sad = Guarded(B * th * tw)
    hip.call(name, gi.ptr, gk.ptr, sad.ptr, B, H, W, T_)
    got = sad.host(B, th, tw)
    assert gi.intact() and gk.intact()
    assert torch.equal(gi.body.cpu(), torch.from_numpy(img).reshape(-1)) and torch.equal(gk.body.cpu(), torch.from_numpy(key).reshape(-1))
    return got


TILE_HW = [(9, 16), (33, 48), (40, 1040), (7, 2064), (16, 20), (13, 37)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T_", [8, 16, 32, 64])
@pytest.mark.parametrize("H,W", TILE_HW)
def test_gate_tiles_u8(H, W, T_, B):
    rng = np.random.default_rng(H * 1009 + W * 7 + T_ * 3 + B)
    shape = (B, 3, H, W)
    rand = (rng.integers(0, 256, shape).astype(np.uint8), rng.integers(0, 256, shape).astype(np.uint8))
    cases = [rand, (np.zeros(shape, dtype=np.uint8), np.full(shape, 255, dtype=np.uint8)), (rand[1], rand[1].copy())]
    for n, (img, key) in enumerate(cases):
        want = torch.from_numpy(R.tiles(as_float(img), key, T_))
        for off in ((False, True) if (n == 0 and W % 16 == 0) else (False,)):       # off: both pointers one byte on, the one-pixel form on a 16-pixel width
            got = _tiles_abi("fs_gate_tiles_u8", img, key, T_, off)
            assert got.dtype == torch.int32 and torch.equal(got.long(), want), (n, off)
        if n == 0:
            assert torch.equal(got, _tiles_abi("fs_gate_tiles", as_float(img), key, T_))
        if n == 1:
            assert int(got[0, 0, 0]) == 3 * 255 * min(T_, H) * min(T_, W)           # the largest entry: 64 * 64 * 3 * 255 for a full tile of 64
        if n == 2:
            assert not bool(got.any())
    img_d, key_d = torch.from_numpy(rand[0]).cuda(), torch.from_numpy(rand[1]).cuda()
    want = torch.from_numpy(R.tiles(as_float(rand[0]), rand[1], T_)).int()
    out = torch.full_like(want, 7).cuda()
    assert ops.gate_tiles_u8(img_d, key_d, T_, out=out) is out and torch.equal(out.cpu(), want)
    assert torch.equal(ops.gate_tiles_u8(img_d, key_d, tile=T_), ops.gate_tiles(floats(img_d), key_d, tile=T_))


# ------------------------------------------------------------------------------------------------------------------ GPU: commit -----
_REC_TYPES = (torch.int64, torch.int64, torch.int32, torch.int32, torch.float32)


def _records(rng, rows, H, W, cap, conf):
    P = (W + 31) // 32
    rec = [rng.integers(-2 ** 40, 2 ** 40, (rows,)), rng.integers(-2 ** 40, 2 ** 40, (rows, 6)),
           rng.integers(-2 ** 31, 2 ** 31, (rows, cap)).astype(np.int32), rng.integers(-2 ** 31, 2 ** 31, (rows, H, P)).astype(np.int32)]
    if conf:
        rec.append(rng.random((rows, 3), dtype=np.float32))
    return rec


def _commit_abi(name, img, idx, key, gstate, focus, src, dst):
    """fs_gate_commit / fs_gate_commit_u8 on guarded buffers -> [key, gstate, *dst] on the host."""
    B, _, H, W = img.shape
    n = len(idx)
    gi = Guarded(img.size, torch.uint8 if img.dtype == np.uint8 else torch.float32, body=torch.from_numpy(img))
    gk = Guarded(key.size, torch.uint8, body=torch.from_numpy(key))
    gs = Guarded(gstate.size, torch.int64, body=torch.from_numpy(gstate))
    gf = Guarded(focus.size, torch.float32, body=torch.from_numpy(focus))
    gd = [Guarded(d.size, dt, body=torch.from_numpy(d)) for d, dt in zip(dst, _REC_TYPES)]
    sd = [Guarded(max(s.size, 1), dt, body=torch.from_numpy(s) if s.size else None) for s, dt in zip(src, _REC_TYPES)]
    ix = torch.tensor(idx, dtype=torch.int32, device="cuda") if n else None
    sp = [g.ptr for g in sd] + [None] * (5 - len(sd))
    dp = [g.ptr for g in gd] + [None] * (5 - len(gd))
    hip.call(name, gi.ptr, None if ix is None else ix.data_ptr(), n, gk.ptr, gs.ptr, gf.ptr, *sp, *dp, B, H, W, dst[2].shape[1])
    torch.cuda.synchronize()
    assert gi.intact() and gf.intact() and all(g.intact() for g in sd)
    assert torch.equal(gi.body.cpu(), torch.from_numpy(img).reshape(-1))
    return [gk.host(*key.shape), gs.host(B, 6)] + [g.host(*d.shape) for g, d in zip(gd, dst)]


@pytest.mark.gpu
@pytest.mark.parametrize("W", [48, 37])
@pytest.mark.parametrize("conf", [False, True])
def test_gate_commit_u8(W, conf):
    B, H, cap = 5, 9, 6
    rng = np.random.default_rng(200 + W + conf)
    img = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    focus = rng.random((B, 2), dtype=np.float32)
    for idx in ([], list(range(B)), [1, 3], [0, 2, B + 3], [-1, 4]):          # the last two: an entry outside 0 .. B-1 writes nothing
        key = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)             # what an untouched viewer must keep
        gstate = rng.integers(0, 1000, (B, 6))
        dst, src = _records(rng, B, H, W, cap, conf), _records(rng, len(idx), H, W, cap, conf)
        got = _commit_abi("fs_gate_commit_u8", img, idx, key, gstate, focus, src, dst)
        want = _commit_abi("fs_gate_commit", as_float(img), idx, key, gstate, focus, src, dst)
        for a, b in zip(got, want):
            assert torch.equal(_bits32(a), _bits32(b))
        for b in range(B):
            assert np.array_equal(got[0][b].numpy(), img[b] if b in idx else key[b])
    # the op, and the pair of kernels: a byte frame against the key commit made from it differs nowhere
    x = torch.from_numpy(img).cuda()
    key = torch.full((B, 3, H, W), 0x3D, dtype=torch.uint8, device="cuda")
    gstate = torch.zeros(B, 6, dtype=torch.int64, device="cuda")
    rec = [torch.from_numpy(a).cuda() for a in _records(rng, B, H, W, cap, conf)]
    ops.gate_commit_u8(x, torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda"), key, gstate, torch.from_numpy(focus).cuda(),
                       [t[:3].contiguous() for t in rec], rec)
    assert torch.equal(key[[0, 2, 4]], x[[0, 2, 4]]) and bool((key[[1, 3]] == 0x3D).all()) and gstate[:, 0].tolist() == [1, 0, 1, 0, 1]
    assert ops.gate_tiles_u8(x, key, 8)[[0, 2, 4]].sum().item() == 0


# ------------------------------------------------------------------------------------------------------------------ GPU: shift ------
_STATE_ORDER = ("key", "bits", "gstate", "stats", "counts", "prof_key", "mstate")
_STATE_TYPES = dict(key=torch.uint8, bits=torch.int32, gstate=torch.int64, stats=torch.int64, counts=torch.int32, prof_key=torch.int32,
                    mstate=torch.int64)


def _shift_abi(name, img, st):
    B, _, H, W = img.shape
    cap, P = st["counts"].shape[1], (W + 31) // 32
    gi = Guarded(img.size, torch.uint8 if img.dtype == np.uint8 else torch.float32, body=torch.from_numpy(img))
    gs = Guarded(B * 4, torch.int64, body=torch.from_numpy(st["shift"]))
    g = {k: Guarded(st[k].size, _STATE_TYPES[k], body=torch.from_numpy(np.ascontiguousarray(st[k]))) for k in _STATE_ORDER}
    key2, bits2 = Guarded(st["key"].size, torch.uint8), Guarded(B * H * P)
    motion = Guarded(B * 6, torch.int64)
    scratch = Guarded(hip.query("fs_state_shift_scratch_ints", B, H, W, cap))
    hip.call(name, gi.ptr, gs.ptr, g["key"].ptr, key2.ptr, g["bits"].ptr, bits2.ptr, g["gstate"].ptr, g["stats"].ptr, g["counts"].ptr,
             g["prof_key"].ptr, g["mstate"].ptr, motion.ptr, scratch.ptr, B, H, W, cap)
    torch.cuda.synchronize()
    assert gi.intact() and gs.intact() and key2.intact() and bits2.intact() and scratch.intact()
    assert torch.equal(gi.body.cpu(), torch.from_numpy(img).reshape(-1))
    out = {k: g[k].host(*st[k].shape).numpy() for k in _STATE_ORDER}
    out["motion"] = motion.host(B, 6).numpy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(12, 40), (24, 64)])
def test_state_shift_u8(H, W):
    B, cap, Rg = 3, 8 * W + 1, (min(H, W) - 1) // 4
    for n, (dy, dx) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1), (Rg, -Rg), (0, 33), (0, -31))):          # the last two: across the 32-bit word border
        rng = np.random.default_rng(H * 1009 + W * 7 + n)
        shifts = [(dy, dx), (0, 0), (-dy, dx if dy else -dx)]                                               # viewer 1 stands still
        shape = (B, 3, H, W)
        masks = [rng.random((H, W)) < 0.5 for _ in range(B)]
        img = rng.integers(0, 256, shape).astype(np.uint8)
        st = dict(key=rng.integers(0, 256, shape).astype(np.uint8), bits=np.stack([RLE.bits(m) for m in masks]),
                  gstate=rng.integers(0, 16 * min(H, W), (B, 6)), mstate=rng.integers(-50, 50, (B, 4)),
                  shift=np.array([[a, b, int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 40))] for a, b in shifts], dtype=np.int64),
                  stats=rng.integers(0, 99, (B, 6)), counts=rng.integers(0, 99, (B, cap)).astype(np.int32),
                  prof_key=rng.integers(0, 99, (B, H + W)).astype(np.int32))
        got = _shift_abi("fs_state_shift_u8", img, st)
        twin = _shift_abi("fs_state_shift", as_float(img), st)
        want = dict(zip(_STATE_ORDER + ("motion",), M.state_shift(as_float(img), st["shift"], *(st[k] for k in _STATE_ORDER))))
        for k in want:
            assert np.array_equal(got[k], twin[k]) and np.array_equal(got[k], want[k]), (k, shifts)
        for k in _STATE_ORDER:
            assert np.array_equal(got[k][1], st[k][1]), k                                                    # untouched, garbage included
    # the op on device tensors
    dev = {k: torch.from_numpy(np.ascontiguousarray(st[k])).cuda() for k in _STATE_ORDER + ("shift",)}
    motion = ops.state_shift_u8(torch.from_numpy(img).cuda(), dev["shift"], dev["key"], torch.zeros_like(dev["key"]), dev["bits"],
                                torch.zeros_like(dev["bits"]), dev["gstate"], dev["stats"], dev["counts"], dev["prof_key"], dev["mstate"])
    assert np.array_equal(motion.cpu().numpy(), want["motion"]) and all(np.array_equal(dev[k].cpu().numpy(), want[k]) for k in _STATE_ORDER)


# ------------------------------------------------------------------------------------------------------------------ GPU: front ------
def _all_bytes_frame(rng, B, C, H, W):
    """Random bytes in which every value 0 .. 255 occurs (where the frame has room for them)."""
    img = rng.integers(0, 256, (B, C, H, W)).astype(np.uint8)
    flat = img.reshape(-1)
    n = min(256, flat.size)
    flat[rng.choice(flat.size, n, replace=False)] = np.arange(n, dtype=np.uint8)
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,hs,ws", [(37, 53, 8, 6), (64, 64, 16, 16), (5, 7, 8, 9)])
def test_gaze_lowres_u8(H, W, hs, ws):
    B = 2
    rng = np.random.default_rng(H * 1009 + W)
    img = _all_bytes_frame(rng, B, 3, H, W)
    assert len(np.unique(img)) == min(256, img.size)
    for f in (0.0, 1.0, 0.37):
        focus = np.full((B, 2), f, dtype=np.float32)
        outs = []
        for name, frame, dt in (("fs_gaze_lowres_u8_fwd", img, torch.uint8), ("fs_gaze_lowres_fwd", as_float(img), torch.float32)):
            gx = Guarded(frame.size, dt, body=torch.from_numpy(frame))
            gf = Guarded(focus.size, torch.float32, body=torch.from_numpy(focus))
            out = Guarded(B * hs * ws * 5, torch.float32)
            hip.call(name, gx.ptr, gf.ptr, out.ptr, B, H, W, hs, ws)
            outs.append(out.host(B, hs, ws, 5))
            assert gx.intact() and gf.intact() and torch.equal(gx.body.cpu(), torch.from_numpy(frame).reshape(-1))
        diff = (outs[0].view(torch.int32) != outs[1].view(torch.int32))
        print(f"focus {f}: entries that differ per channel {diff.sum(dim=(0, 1, 2)).tolist()}")
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    x, fo = torch.from_numpy(img).cuda(), torch.tensor([[0.2, 0.9], [0.5, 0.5]], device="cuda")
    assert torch.equal(ops.gaze_lowres(x, fo, hs, ws).view(torch.int32), ops.gaze_lowres(floats(x), fo, hs, ws).view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("nhwc", [0, 1])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_grid_sample_u8(C, nhwc):
    B, H, W, h, w = 2, 11, 13, 6, 5
    rng = np.random.default_rng(C * 10 + nhwc)
    img = _all_bytes_frame(rng, B, C, H, W)
    grid = (rng.random((B, h, w, 2), dtype=np.float32) * 2.2 - 1.1)
    g = grid.reshape(-1, 2)
    g[0], g[1], g[2], g[3] = (-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0)                     # the corners of the grid's range, exactly
    g[4], g[5] = (-1.0 - 1.0 / W, 0.3), (0.2, 1.0 + 1.0 / H)                                         # half a pixel outside
    g[6], g[7], g[8] = (1e30, 0.0), (0.0, -1e30), (np.float32("nan"), np.float32("nan"))             # far outside, and no point at all
    outs = []
    for name, frame, dt in (("fs_grid_sample_u8_fwd", img, torch.uint8), ("fs_grid_sample_fwd", as_float(img), torch.float32)):
        gx = Guarded(frame.size, dt, body=torch.from_numpy(frame))
        gg = Guarded(grid.size, torch.float32, body=torch.from_numpy(grid))
        out = Guarded(B * h * w * C, torch.float32)
        hip.call(name, gx.ptr, gg.ptr, out.ptr, B, C, H, W, h, w, nhwc)
        outs.append(out.host(B * h * w * C))
        assert gx.intact() and gg.intact() and torch.equal(gx.body.cpu(), torch.from_numpy(frame).reshape(-1))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert bool(outs[0].isnan().any()) and bool((outs[0] > 0).any())                                 # the NaN point and real samples are both there
    if nhwc:
        x, gd = torch.from_numpy(img).cuda(), torch.from_numpy(grid).cuda()
        got = ops.grid_sample_u8(x, gd)
        assert got.shape == (B, h, w, C) and torch.equal(got.view(torch.int32), ops.GridSample.apply(floats(x), gd).view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ GPU: refusals ---
@pytest.mark.gpu
def test_byte_entry_points_reject_bad_arguments():
    B, H, W, T_, cap = 2, 16, 24, 8, 5
    img, key, key2 = Guarded(B * 3 * H * W, torch.uint8), Guarded(B * 3 * H * W, torch.uint8), Guarded(B * 3 * H * W, torch.uint8)
    sad, low, samp = Guarded(B * 6), Guarded(B * 4 * 4 * 5, torch.float32), Guarded(B * 4 * 4 * 3, torch.float32)
    gstate, stats, mstate = Guarded(B * 6, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * 4, torch.int64)
    focus, grid = Guarded(B * 2, torch.float32), Guarded(B * 4 * 4 * 2, torch.float32)
    bits, bits2, prof_key = Guarded(B * H), Guarded(B * H), Guarded(B * (H + W))
    shift, motion, counts = Guarded(B * 4, torch.int64, body=torch.ones(B * 4)), Guarded(B * 6, torch.int64), Guarded(B * cap)
    scratch = Guarded(hip.query("fs_state_shift_scratch_ints", B, H, W, cap))
    rec = [Guarded(B, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * cap), Guarded(B * H), Guarded(B * 3, torch.float32)]
    idx = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    outs = [key, key2, sad, low, samp, gstate, stats, mstate, bits, bits2, prof_key, motion, counts, scratch] + rec

    def each(name, good, bads):
        for i, bad in bads:
            a = list(good)
            a[i] = bad
            with pytest.raises(hip.HipLibraryError, match="argument rejected"):
                hip.call(name, *a)
            torch.cuda.synchronize()
            assert all(g.intact() and bool((g.body == _GARB[g.dtype]).all()) for g in outs), f"a rejected {name} launched something"

    each("fs_gate_tiles_u8", [img.ptr, key.ptr, sad.ptr, B, H, W, T_],
         ((0, None), (1, None), (2, None), (3, 0), (4, 0), (5, -1), (6, 12), (6, 0), (6, 128)))
    each("fs_gaze_lowres_u8_fwd", [img.ptr, focus.ptr, low.ptr, B, H, W, 4, 4], ((0, None), (1, None), (2, None), (3, 0), (4, 0), (5, -1), (6, 1), (7, 0)))
    each("fs_grid_sample_u8_fwd", [img.ptr, grid.ptr, samp.ptr, B, 3, H, W, 4, 4, 1], ((0, None), (1, None), (2, None), (3, 0), (4, 0), (5, 0), (6, -1), (7, 0), (8, 0)))
    ptrs = [g.ptr for g in rec]
    each("fs_gate_commit_u8", [img.ptr, idx.data_ptr(), 2, key.ptr, gstate.ptr, focus.ptr, *ptrs, *ptrs, B, H, W, cap],
         ((0, None), (1, None), (2, 3), (2, -1), (3, None), (4, None), (5, None), (6, None), (9, None), (11, None), (14, None), (15, None),
          (16, 0), (17, 0), (18, 0), (19, 0)))
    good = [img.ptr, shift.ptr, key.ptr, key2.ptr, bits.ptr, bits2.ptr, gstate.ptr, stats.ptr, counts.ptr, prof_key.ptr, mstate.ptr, motion.ptr,
            scratch.ptr, B, H, W, cap]
    each("fs_state_shift_u8", good, [(i, None) for i in range(13)] + [(3, key.ptr), (5, bits.ptr), (12, scratch.ptr + 4), (13, 0), (14, 0), (15, 0), (16, 0)])


# ------------------------------------------------------------------------------------------------------------------ GPU: module -----
SIZE, SEED = 256, 11


def _bytes_of(X):
    """A synthetic fp32 batch quantised to bytes."""
    return (X.clamp(0, 1) * 255).round().to(torch.uint8)


def _peak_of(call):
    """The rise of the allocator's peak over one call, after a warm-up call."""
    call()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = call()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


@pytest.mark.gpu
def test_module_reads_byte_frames(served):
    module, calls, TP = served
    X, Fp, Y, cl = T.synthetic_batch(2, SIZE, SIZE, seed=SEED, device="cuda")
    U = _bytes_of(X)
    U0 = U.clone()
    Xf = floats(U)
    assert len(torch.unique(U)) > 100
    assert torch.equal(module.predict(U, Fp), module.predict(Xf, Fp))
    kw = dict(return_bits=True, return_score=True, component=8)
    want = module.predict_instances(Xf, Fp, **kw)
    assert 0 < int(want[1][0, 0]) < SIZE * SIZE
    assert _same(module.predict_instances(U, Fp, **kw), want)
    assert _same(module.predict_instances(U, Fp, (200, 180), max_runs=50), module.predict_instances(Xf, Fp, (200, 180), max_runs=50))
    for kwe in (dict(class_areas=True), dict(return_labels=True, trimap=5, hausdorff=95)):
        assert _same(module.evaluate(U, Fp, Y, cl, **kwe), module.evaluate(Xf, Fp, Y, cl, **kwe))
    assert _same(module.evaluate_instances(U, Fp, Y, cl, component=8), module.evaluate_instances(Xf, Fp, Y, cl, component=8))
    module.check_nan()
    assert torch.equal(U, U0)
    # the float detour is gone: the byte call's peak is not above the fp32 call's (an internal U.float() would add 1.5 MB)
    p8, p32 = _peak_of(lambda: module.predict_instances(U, Fp)), _peak_of(lambda: module.predict_instances(Xf, Fp))
    print(f"predict_instances raised the peak by {p8} bytes fed uint8 and by {p32} fed fp32")
    assert p8 <= p32


# ------------------------------------------------------------------------------------------------------------------ GPU: session ----
def _state_of(s):
    out = [s._key, s._gstate] + list(s._rec)
    if s.motion_px is not None:
        out += [s._prof_key, s._mstate]
    return out


def _step_all(sessions, feeds, U, Fp, force=None):
    """One step of every session on the same bytes, each fed its own dtype; all results and states must agree.  Returns the first result."""
    outs = []
    for s, feed in zip(sessions, feeds):
        outs.append(s.step(U if feed == "u8" else floats(U), Fp, force=force))
    for s, o in zip(sessions[1:], outs[1:]):
        assert _same(tuple(outs[0]), tuple(o)) and s.counts == sessions[0].counts
        for a, b in zip(_state_of(sessions[0]), _state_of(s)):
            assert torch.equal(_bits32(a), _bits32(b))
    return outs[0]


def _alternating(n):
    while True:
        n += 1
        yield "u8" if n % 2 else "f32"


@pytest.mark.gpu
def test_session_on_bytes_equals_the_session_on_floats(served):
    module, calls, TP = served
    H = W = SIZE
    X, Fp = TP._batch(2, SIZE, SEED)
    U = _bytes_of(X)
    U0 = U.clone()
    sessions = [GazeSession(module, 2, (H, W), score=True) for _ in range(3)]
    alt = _alternating(0)
    feed = lambda: ("u8", "f32", next(alt))
    *rec, gate = _step_all(sessions, feed(), U, Fp)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and _same(tuple(rec), module.predict_instances(floats(U), Fp, return_bits=True, return_score=True))
    assert torch.equal(sessions[0]._key, U)                                            # the key frame is the frame
    held = [t.clone() for t in rec]
    *rec, gate = _step_all(sessions, feed(), U, Fp)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and gate[:, 1:6].tolist() == [[0] * 5] * 2 and _same(rec, held)
    # a REUSE step on bytes allocates nothing
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = sessions[0].step(U, Fp)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"a REUSE step on bytes raised the peak by {grew} bytes")
    assert grew == 0 and out[-1][:, 0].tolist() == [R.REUSE] * 2
    for s in sessions[1:]:
        s.step(floats(U), Fp)
    # a flipped tile inside viewer 1's box: RUN_ROI
    box_tile = (int(held[1][1, 2]) // 32, int(held[1][1, 1]) // 32)
    U4 = _bytes_of(_flip_tile(floats(U), 1, *box_tile))
    *rec, gate = _step_all(sessions, feed(), U4, Fp)
    assert gate[:, 0].tolist() == [R.REUSE, R.RUN_ROI]
    assert _same(tuple(t[1:2] for t in rec), module.predict_instances(floats(U4[1:2]), Fp[1:2], return_bits=True, return_score=True))
    # a gaze drift of 12 pixels to a clear pixel: RUN_GAZE
    mask0 = RLE.unbits(rec[3][0].cpu().numpy(), W)
    py, px = _pixel(Fp, 0)
    y, x = np.mgrid[:H, :W]
    d = np.hypot(y - py, x - px)
    ok = (~mask0) & (d > 9) & (d < 24)
    assert ok.any()
    i = int(np.argmin(np.where(ok, np.abs(d - 16), np.inf)))
    F5 = _focus_at(Fp, 0, i // W, i % W)
    *rec, gate = _step_all(sessions, feed(), U4, F5)
    assert gate[:, 0].tolist() == [R.RUN_GAZE, R.REUSE]
    *rec, gate = _step_all(sessions, feed(), U4, F5, force=[0, 1])
    assert gate[:, 0].tolist() == [R.REUSE, R.RUN_FORCED]
    assert torch.equal(U, U0) and sessions[0].counts[R.REUSE] >= 5


@pytest.mark.gpu
def test_moving_session_on_bytes_equals_the_session_on_floats(served):
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
    alt = _alternating(1)
    feed = lambda: ("u8", "f32", next(alt))
    *rec, gate, motion = _step_all(sessions, feed(), U1, F1)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and motion.tolist() == [[0] * 6] * 2
    assert torch.equal(sessions[0]._prof_key, ops.key_profiles(U1))
    *rec, gate, motion = _step_all(sessions, feed(), U2, F2)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and motion[:, :2].tolist() == [[3, -5], [0, 0]]
    assert torch.equal(sessions[0]._prof_key, ops.key_profiles(sessions[0]._key))
    # a moved REUSE step on bytes allocates nothing
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = sessions[0].step(U3, F3)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"a moved REUSE step on bytes raised the peak by {grew} bytes")
    assert grew == 0 and out[-2][:, 0].tolist() == [R.REUSE] * 2 and out[-1][:, :2].tolist() == [[-2, 1], [0, 0]] and out[-1][:, 4:].tolist() == [[1, -4], [0, 0]]
    for s, f in zip(sessions[1:], ("f32", "u8")):
        o = s.step(floats(U3) if f == "f32" else U3, F3)
        assert _same(tuple(out), tuple(o))
    for a, b, c in zip(*(_state_of(s) for s in sessions)):
        assert torch.equal(_bits32(a), _bits32(b)) and torch.equal(_bits32(a), _bits32(c))
