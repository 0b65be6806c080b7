"""Global motion compensation in front of the gaze gate: ops.frame_profiles / key_profiles / profile_shift / state_shift /
motion_commit (fs_frame_profiles, fs_key_profiles, fs_profile_shift, fs_state_shift + fs_state_shift_scratch_ints, fs_motion_commit)
and GazeSession(motion_px=...).

All of it is integer work and is held bit for bit.  tests/motion_ref.py restates the definitions in numpy; the reference has no
counterpart (unpinned), so the CPU tests pin motion_ref to hand-derived answers on frames of at most 12 x 40, and the GPU tests hold the
kernels to motion_ref and the session to the reference move of its own records.  At the C ABI every output sits between sentinel guard
bands and is pre-filled with garbage."""
import numpy as np
import pytest
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg.session import GazeSession

import gate_ref as R
import motion_ref as M
import rle_ref as RLE
from test_gaze_session import Guarded, _GARB, _same, _row, served       # noqa: F401  (served is a fixture)

NAN = np.float32("nan")


# ------------------------------------------------------------------------------------------------------------------ CPU: hand-built --
def test_ref_profiles_of_a_bright_row_and_column():
    img = np.zeros((1, 3, 6, 8), dtype=np.float32)
    img[0, :, 2, :] = 1.0                                # a bright row: L = 765 on its 8 pixels
    img[0, :, :, 5] = 1.0                                # and a bright column, which shares pixel (2, 5) with it
    prof = M.frame_profiles(img)
    assert prof.shape == (1, 14)
    assert prof[0, :6].tolist() == [765, 765, 765 * 8, 765, 765, 765]
    assert prof[0, 6:].tolist() == [765, 765, 765, 765, 765, 765 * 6, 765, 765]
    key = R.q(img).astype(np.uint8)
    assert np.array_equal(M.key_profiles(key), prof)                                  # the invariant the session rests on


def test_ref_luma_at_the_ties_and_nan():
    img = np.zeros((1, 3, 1, 4), dtype=np.float32)
    img[0, :, 0, 0] = (0.5 / 255, 1.5 / 255, NAN)        # ties to even: 0 and 2; NaN: 0
    img[0, :, 0, 1] = (-3.0, 7.0, 1.0)                   # clamped: 0, 255, 255
    img[0, :, 0, 2] = (np.float32("inf"), np.float32("-inf"), 0.5)                    # 255, 0, rint(127.5) = 128
    assert M.luma(img)[0, 0].tolist() == [2, 510, 383, 0]


HH, HW, HR = 12, 40, 2                                   # the hand frame: R = 2 is the largest range with 4 R < 12


def _row_frame(y):
    img = np.zeros((1, 3, HH, HW), dtype=np.float32)
    img[0, :, y, :] = 1.0
    return img


@pytest.mark.parametrize("d", [-2, -1, 1, 2])
def test_ref_a_moved_row_gives_that_dy(d):
    valid = np.ones((1, 6), dtype=np.int64)
    got = M.profile_shift(M.frame_profiles(_row_frame(5 + d)), M.frame_profiles(_row_frame(5)), valid, HH, HW, HR, 6)
    # rows 5 and 5 + d lie inside the window 2 .. 9: standing still costs both rows, 2 * 765 * 40; every column profile is 765 flat
    assert got.tolist() == [[d, 0, 0, 2 * 765 * 40]]


def test_ref_a_flat_frame_and_an_invalid_viewer():
    flat = np.full((2, 3, HH, HW), 0.25, dtype=np.float32)
    p = M.frame_profiles(flat)
    assert M.profile_shift(p, p, np.ones((2, 6), dtype=np.int64), HH, HW, HR, 6).tolist() == [[0, 0, 0, 0]] * 2      # every cost ties: |s| = 0
    g = np.ones((2, 6), dtype=np.int64)
    g[1, 0] = 0
    got = M.profile_shift(M.frame_profiles(np.concatenate([_row_frame(6), _row_frame(6)])), M.frame_profiles(np.concatenate([_row_frame(5)] * 2)), g, HH, HW, HR, 6)
    assert got.tolist() == [[1, 0, 0, 61200], [0, 0, 0, 0]]


def _gain_profiles(r):
    """n = 12, R = 2, window 2 .. 9.  K has one peak of 80 at 5; P has it at 6 and a residual r at 3.  cost(1) = r, cost(0) = 160 + r,
    cost(-1) = cost(2) = 160 + r, cost(-2) = |r - 80| + 80."""
    K, P = np.zeros(12, dtype=np.int64), np.zeros(12, dtype=np.int64)
    K[5], P[6], P[3] = 80, 80, r
    return P, K


def test_ref_costs_and_the_tie_rule():
    P, K = _gain_profiles(480)
    assert [M.cost(P, K, s, 2) for s in (-2, -1, 0, 1, 2)] == [480, 640, 640, 480, 640]
    assert M.axis_shift(P, K, 2, 8) == (1, 480, 640)     # -2 and +1 tie: the smaller |s|
    P2, K2 = np.zeros(12, dtype=np.int64), np.zeros(12, dtype=np.int64)
    P2[5], K2[4], K2[6] = 9, 9, 9                        # -1 and +1 tie at 9, cost(0) = 27: the negative s
    assert [M.cost(P2, K2, s, 2) for s in (-1, 0, 1)] == [9, 27, 9] and M.axis_shift(P2, K2, 2, 8) == (-1, 9, 27)


def test_ref_the_gain_rule_at_its_edge():
    P, K = _gain_profiles(480)                           # 480 * 8 == 640 * 6: taken
    assert M.axis_shift(P, K, 2, 6) == (1, 480, 640)
    P, K = _gain_profiles(481)                           # 481 * 8 = 3848 > 641 * 6 = 3846: refused; the costs are reported all the same
    assert M.axis_shift(P, K, 2, 6) == (0, 481, 641)
    assert M.axis_shift(P, K, 2, 8) == (1, 481, 641) and M.axis_shift(P, K, 2, 0) == (0, 481, 641)
    P, K = _gain_profiles(0)                             # an exact shift costs 0 and passes gain = 0
    assert M.axis_shift(P, K, 2, 0) == (1, 0, 160)
    P, K = _gain_profiles(10 ** 6)                       # gain = 8 takes whatever is no worse than standing still
    assert M.axis_shift(P, K, 2, 8) == (1, 10 ** 6, 10 ** 6 + 160) and M.axis_shift(P, K, 2, 7)[0] == 0


def _one_viewer_state(mask, H, W, gaze=(0, 0, 0, 0), cap=9):
    img = np.full((1, 3, H, W), 0.5, dtype=np.float32)                                # q = 128
    key = (np.arange(3 * H * W, dtype=np.int64) % 251).astype(np.uint8).reshape(1, 3, H, W)
    gstate = np.array([[1, *gaze, 4]], dtype=np.int64)
    return dict(img=img, key=key, bits=RLE.bits(mask)[None], gstate=gstate, stats=np.array([RLE.stats(mask)], dtype=np.int64),
                counts=np.array([RLE.counts_row(mask, cap)], dtype=np.int32), prof_key=M.key_profiles(key), mstate=np.array([[2, -3, 1, 5]], dtype=np.int64))


def _ref_move(st, dy, dx):
    shift = np.array([[dy, dx, 11, 22]], dtype=np.int64)
    return M.state_shift(st["img"], shift, st["key"], st["bits"], st["gstate"], st["stats"], st["counts"], st["prof_key"], st["mstate"])


@pytest.mark.parametrize("x,dx,want", [(31, 1, [0, 1]), (31, -1, [1 << 30, 0]), (32, 1, [0, 2]), (32, -1, [-2 ** 31, 0]),
                                       (31, 7, [0, 1 << 6]), (32, 7, [0, 1 << 7]), (31, -7, [1 << 24, 0]), (32, -7, [1 << 25, 0]),
                                       (32, 8, [0, 0]), (39, 1, [0, 0]), (0, -1, [0, 0])])
def test_ref_bits_move_across_the_word_border(x, dx, want):
    mask = np.zeros((3, 40), dtype=bool)
    mask[1, x] = True
    key, bits, gstate, stats, counts, prof_key, mstate, motion = _ref_move(_one_viewer_state(mask, 3, 40), 0, dx)
    assert bits[0].tolist() == [[0, 0], want, [0, 0]]
    assert int(stats[0, 0]) == (1 if any(want) else 0)
    if any(want):
        assert stats[0].tolist() == [1, x + dx, 1, 1, 1, 3] and counts[0, :3].tolist() == [(x + dx) * 3 + 1, 1, 120 - (x + dx) * 3 - 2]
    else:
        assert stats[0].tolist() == [0, 0, 0, 0, 0, 1] and counts[0, :2].tolist() == [120, 0]           # the bit left the frame
    assert motion.tolist() == [[0, dx, 11, 22, 2, -3 + dx]] and mstate.tolist() == [[2, -3 + dx, 2, 5 + abs(dx)]]


def test_ref_rows_leave_the_frame_and_the_gaze_clamps():
    mask = np.zeros((4, 8), dtype=bool)
    mask[0, 2], mask[3, 2] = True, True
    top_y, top_x = 3 * 16, 7 * 16
    st = _one_viewer_state(mask, 4, 8, gaze=(8, top_x - 8, top_y - 8, 40))
    key, bits, gstate, stats, counts, prof_key, mstate, motion = _ref_move(st, -1, 1)
    assert bits[0, :, 0].tolist() == [0, 0, 1 << 3, 0]                                 # row 0 left, row 3 went to row 2
    assert gstate.tolist() == [[1, 0, top_x, top_y - 24, 56, 4]]                       # 8 - 16 clamps to 0, top_x - 8 + 16 to top_x
    key, bits, gstate, *_ = _ref_move(st, 1, -1)
    assert bits[0, :, 0].tolist() == [0, 1 << 1, 0, 0]
    assert gstate.tolist() == [[1, 24, top_x - 24, top_y, 24, 4]]                      # top_y - 8 + 16 clamps to top_y


def test_ref_the_key_moves_and_its_border_is_the_new_frame():
    H, W = 4, 8
    st = _one_viewer_state(np.zeros((H, W), dtype=bool), H, W)
    key, bits, gstate, stats, counts, prof_key, mstate, motion = _ref_move(st, 1, -2)
    old = st["key"][0]
    for c in range(3):
        assert key[0, c, 0].tolist() == [128] * W                                      # the uncovered row
        for y in range(1, H):
            assert key[0, c, y].tolist() == old[c, y - 1, 2:].tolist() + [128, 128]    # the uncovered columns
    assert np.array_equal(prof_key, M.key_profiles(key))
    # a still viewer: nothing moves, the motion row reports the totals
    key0, bits0, g0, s0, c0, p0, m0, mo0 = _ref_move(st, 0, 0)
    assert np.array_equal(key0, st["key"]) and np.array_equal(g0, st["gstate"]) and np.array_equal(m0, st["mstate"])
    assert mo0.tolist() == [[0, 0, 11, 22, 2, -3]]
    pk, ms = M.motion_commit([0], np.full_like(p0, 7), p0, m0)
    assert bool((pk == 7).all()) and ms.tolist() == [[0, 0, 0, 0]]


class _Stub:
    training = False


@pytest.mark.parametrize("kw", [dict(motion_px=0), dict(motion_px=16), dict(motion_px=256), dict(motion_px=-1), dict(motion_px=True),
                                dict(motion_px=2.0), dict(motion_px="4"), dict(motion_px=4, motion_gain=9), dict(motion_px=4, motion_gain=-1),
                                dict(motion_px=4, motion_gain=True), dict(motion_px=4, motion_gain=6.0), dict(motion_gain=9)])
def test_session_rejects_bad_motion_parameters(kw):
    with pytest.raises(ValueError):
        GazeSession(_Stub(), 2, (64, 80), **kw)          # 4 * 16 = 64 is not below min(H, W) = 64


def test_session_takes_the_motion_parameters():
    s = GazeSession(_Stub(), 2, (64, 80), motion_px=15)
    assert (s.motion_px, s.motion_gain) == (15, 6) and s.counts == {c: 0 for c in range(8)}
    s = GazeSession(_Stub(), 2, (64, 80), motion_px=np.int64(3), motion_gain=0)
    assert (s.motion_px, s.motion_gain) == (3, 0)
    assert GazeSession(_Stub(), 2, (64, 80)).motion_px is None
    assert fovealseg.gaze._motion_px(255, 1024, 1100) == 255
    with pytest.raises(ValueError):
        fovealseg.gaze._motion_px(255, 1024, 8000)                  # 8 * 8000 + 8 * 511 bytes of LDS


def test_the_ctypes_table_binds_the_motion_entry_points():
    assert hip.SIGNATURES["fs_frame_profiles"] == hip.SIGNATURES["fs_key_profiles"] == "pp" + "iii"
    assert hip.SIGNATURES["fs_profile_shift"] == "pppp" + "iiiii"
    assert hip.SIGNATURES["fs_state_shift"] == "p" * 13 + "iiii"
    assert hip.SIGNATURES["fs_motion_commit"] == "p" + "i" + "ppp" + "iii"
    assert hip.HOST_ONLY["fs_state_shift_scratch_ints"] == ("l", "iiii")
    assert sorted(ops.GATE_CODES) == list(range(8))      # the motion stage adds no decision code


def test_ops_reject_wrong_dtypes_and_shapes():
    B, H, W = 2, 16, 24
    P = 1
    img, key = torch.zeros(B, 3, H, W), torch.zeros(B, 3, H, W, dtype=torch.uint8)
    prof = torch.zeros(B, H + W, dtype=torch.int32)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    for bad in (img.double(), img[:, :2], img[0], key, img.numpy()):
        with pytest.raises(ValueError):
            ops.frame_profiles(bad)
    for bad in (img, key[:, :2], key.int()):
        with pytest.raises(ValueError):
            ops.key_profiles(bad)
    with pytest.raises(ValueError):
        ops.frame_profiles(img, out=prof[:, :-1])
    with pytest.raises(ValueError):
        ops.key_profiles(key, out=prof.long())
    good = dict(prof=prof, prof_key=prof.clone(), gstate=i64(B, 6), frame_size=(H, W), motion_px=3)
    for k, v in (("prof", prof.long()), ("prof", prof[:, :-1]), ("prof_key", prof[:1]), ("gstate", i64(B, 5)), ("gstate", i64(B, 6).int()),
                 ("motion_px", 0), ("motion_px", 4), ("motion_px", 256), ("motion_px", True), ("motion_px", 1.0), ("frame_size", (H, W + 1)),
                 ("motion_gain", 9), ("motion_gain", True), ("out", i64(B, 3))):
        with pytest.raises(ValueError):
            ops.profile_shift(**dict(good, **{k: v}))
    bits = torch.zeros(B, H, P, dtype=torch.int32)
    good = dict(img=img, shift=i64(B, 4), key=key, key2=key.clone(), bits=bits, bits2=bits.clone(), gstate=i64(B, 6), stats=i64(B, 6),
                counts=torch.zeros(B, 5, dtype=torch.int32), prof_key=prof, mstate=i64(B, 4))
    for k, v in (("img", img.double()), ("shift", i64(B, 2)), ("key", key.int()), ("key2", key[:1]), ("key2", key), ("bits", bits.long()),
                 ("bits2", bits), ("bits2", bits[:, :-1]), ("gstate", i64(B, 8)), ("stats", i64(B, 6).int()), ("counts", i64(B, 5)),
                 ("prof_key", prof[:, 1:]), ("mstate", i64(B, 6)), ("motion", i64(B, 8)), ("scratch", torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.state_shift(**dict(good, **{k: v}))
    for k, v in (("prof", prof.long()), ("prof_key", prof[:1]), ("mstate", i64(B, 6)), ("idx", torch.zeros(1, dtype=torch.int64)),
                 ("idx", torch.zeros(B + 1, dtype=torch.int32)), ("frame_size", (H + 1, W))):
        with pytest.raises(ValueError):
            ops.motion_commit(**dict(dict(idx=None, prof=prof, prof_key=prof.clone(), mstate=i64(B, 4), frame_size=(H, W)), **{k: v}))


# ---- estimator inputs: crops of a seeded, box-filtered noise canvas ----------------------------------------------------------------
EH, EW, ER, EPAD, ESCALE = 96, 128, 16, 12, 4
ESHIFTS = [(dy, dx) for dy in range(-12, 13, 3) for dx in range(-12, 13, 3)]           # 81 viewers, one launch


def _estimator_profiles(noise):
    """(prof (81, H + W), prof_key (81, H + W)): viewer j sees the key window's content moved by ESHIFTS[j], plus Gaussian noise."""
    canv = M.canvas(25, EH + 2 * EPAD, EW + 2 * EPAD, ESCALE)
    rng = np.random.default_rng(7)
    key = M.window(canv, EPAD, EPAD, EH, EW)
    frames = np.stack([M.window(canv, EPAD - dy, EPAD - dx, EH, EW) for dy, dx in ESHIFTS])
    if noise:
        frames = frames + rng.normal(0, noise, frames.shape).astype(np.float32)
    return frames, M.frame_profiles(frames), np.repeat(M.frame_profiles(key[None]), len(ESHIFTS), axis=0)


_EST = {}


def estimator_case(noise):
    if noise not in _EST:
        frames, prof, prof_key = _estimator_profiles(noise)
        want = M.profile_shift(prof, prof_key, np.ones((len(ESHIFTS), 6), dtype=np.int64), EH, EW, ER, 6)
        _EST[noise] = (frames, prof, prof_key, want)
    return _EST[noise]


@pytest.mark.parametrize("noise", [0.0, 0.02])
def test_ref_finds_every_true_shift_on_the_textured_crops(noise):
    """A condition on the inputs, not a measurement: texture scale 4 at 96 x 128, every shift of a grid of step 3 in [-12, 12]^2."""
    frames, prof, prof_key, want = estimator_case(noise)
    assert want[:, :2].tolist() == [list(s) for s in ESHIFTS]


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ------
SHAPES = [(12, 20), (33, 40), (64, 96), (70, 130), (128, 257),
          (130, 264)]                                    # the four-pixel form with three bands of rows and a second segment of columns
RANGES = (1, 2, 5, 16)


def _wild(rng, shape):
    """Frames with a tenth of the pixels NaN, a tenth below 0, a tenth above 1, some infinite."""
    img = rng.random(shape, dtype=np.float32)
    pick = rng.random(shape)
    img[pick < 0.1] = NAN
    img[(pick >= 0.1) & (pick < 0.2)] = -3.5
    img[(pick >= 0.2) & (pick < 0.3)] = 1.0 + 2.0 ** -20
    img[(pick >= 0.3) & (pick < 0.33)] = np.float32("inf")
    img[(pick >= 0.33) & (pick < 0.36)] = np.float32("-inf")
    return img


def _profiles_abi(name, src, off):
    B, _, H, W = src.shape
    dt = torch.float32 if src.dtype == np.float32 else torch.uint8
    gs = Guarded(src.size, dt, body=torch.from_numpy(src), off=1 if off else 0)
    prof = Guarded(B * (H + W))
    hip.call(name, gs.ptr, prof.ptr, B, H, W)
    got = prof.host(B, H + W)
    assert gs.intact()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_profiles(H, W, B):
    rng = np.random.default_rng(H * 1009 + W * 7 + B)
    shape = (B, 3, H, W)
    key = rng.integers(0, 256, shape).astype(np.uint8)
    frames = [_wild(rng, shape), np.ones(shape, dtype=np.float32), key.astype(np.float32) / np.float32(255)]
    for off in (False, True):
        for img in frames:
            got = _profiles_abi("fs_frame_profiles", img, off)
            assert got.dtype == torch.int32 and torch.equal(got.long(), torch.from_numpy(M.frame_profiles(img)))
        got = _profiles_abi("fs_key_profiles", key, off)
        assert torch.equal(got.long(), torch.from_numpy(M.key_profiles(key)))
        assert torch.equal(got, _profiles_abi("fs_frame_profiles", frames[2], off))     # a frame and the key made from it
    x, k = torch.from_numpy(frames[0]).cuda(), torch.from_numpy(key).cuda()
    out = torch.full((B, H + W), 7, dtype=torch.int32, device="cuda")
    assert ops.frame_profiles(x, out=out) is out and torch.equal(out.cpu().long(), torch.from_numpy(M.frame_profiles(frames[0])))
    assert torch.equal(ops.key_profiles(k).cpu().long(), torch.from_numpy(M.key_profiles(key)))


def _shift_abi(prof, prof_key, gstate, H, W, Rg, gain):
    B = prof.shape[0]
    gp = Guarded(prof.size, body=torch.from_numpy(prof))
    gk = Guarded(prof_key.size, body=torch.from_numpy(prof_key))
    gg = Guarded(gstate.size, torch.int64, body=torch.from_numpy(gstate))
    out = Guarded(B * 4, torch.int64)
    hip.call("fs_profile_shift", gp.ptr, gk.ptr, gg.ptr, out.ptr, B, H, W, Rg, gain)
    got = out.host(B, 4)
    for g, a in ((gp, prof), (gk, prof_key), (gg, gstate)):                            # pure: nothing but shift is written
        assert g.intact() and np.array_equal(g.body.cpu().numpy(), a.reshape(-1))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_profile_shift(H, W, B):
    for Rg in RANGES:
        if 4 * Rg >= min(H, W):
            continue
        rng = np.random.default_rng(H * 1009 + W * 7 + B * 31 + Rg)
        canv = M.canvas(H + W + Rg, H + 2 * Rg, W + 2 * Rg, 4)
        key = M.window(canv, Rg, Rg, H, W)
        true = rng.integers(-Rg, Rg + 1, (B, 2))
        frames = np.stack([M.window(canv, Rg - int(dy), Rg - int(dx), H, W) for dy, dx in true])
        frames[0] += rng.normal(0, 0.02, frames[0].shape).astype(np.float32)
        gstate = rng.integers(0, 1000, (B, 6))
        gstate[:, 0] = 1
        if B > 1:
            gstate[1, 0] = 0                             # a viewer without a record, between two that have one
        cases = [(M.frame_profiles(frames).astype(np.int32), np.repeat(M.frame_profiles(key[None]), B, axis=0).astype(np.int32)),
                 # profiles of small integers: ties everywhere, the order decides
                 (rng.integers(0, 3, (B, H + W)).astype(np.int32), rng.integers(0, 3, (B, H + W)).astype(np.int32)),
                 # the largest entries a profile can hold: the costs need 64 bits
                 (rng.integers(0, 2, (B, H + W)).astype(np.int32) * (2 ** 31 - 1), rng.integers(0, 2, (B, H + W)).astype(np.int32) * (2 ** 31 - 1))]
        for prof, prof_key in cases:
            for gain in (0, 6, 8):
                want = M.profile_shift(prof, prof_key, gstate, H, W, Rg, gain)
                got = _shift_abi(prof, prof_key, gstate, H, W, Rg, gain)
                assert torch.equal(got, torch.from_numpy(want)), (Rg, gain)
        prof, prof_key = cases[0]
        out = ops.profile_shift(torch.from_numpy(prof).cuda(), torch.from_numpy(prof_key).cuda(), torch.from_numpy(gstate).cuda(), (H, W), Rg)
        assert torch.equal(out.cpu(), torch.from_numpy(M.profile_shift(prof, prof_key, gstate, H, W, Rg, 6)))


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [0.0, 0.02])
def test_profile_shift_finds_the_true_shifts(noise):
    frames, prof, prof_key, want = estimator_case(noise)
    assert want[:, :2].tolist() == [list(s) for s in ESHIFTS]                           # the condition on the inputs comes first
    n = len(ESHIFTS)
    got_prof = _profiles_abi("fs_frame_profiles", frames, False)
    assert torch.equal(got_prof.long(), torch.from_numpy(prof))
    got = _shift_abi(prof.astype(np.int32), prof_key.astype(np.int32), np.ones((n, 6), dtype=np.int64), EH, EW, ER, 6)
    assert torch.equal(got, torch.from_numpy(want))


def _blob(rng, H, W):
    m = np.zeros((H, W), dtype=bool)
    y0, x0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 4))
    y1, x1 = int(rng.integers(y0 + 1, H + 1)), int(rng.integers(x0 + 1, W + 1))
    m[y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < 0.8
    return m


def _state(rng, B, H, W, cap, shifts):
    """Seeded viewers; a still viewer (shift (0, 0)) holds garbage in stats, counts and prof_key, which must stay."""
    shape = (B, 3, H, W)
    masks = [_blob(rng, H, W) for _ in range(B)]
    masks[0][:, W - 1] = True                            # set pixels in the last column, beside the padding bits
    masks[0][H - 1, :] = True
    st = dict(img=_wild(rng, shape), key=rng.integers(0, 256, shape).astype(np.uint8), bits=np.stack([RLE.bits(m) for m in masks]),
              gstate=rng.integers(0, 16 * min(H, W), (B, 6)), mstate=rng.integers(-50, 50, (B, 4)),
              shift=np.array([[dy, dx, int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 40))] for dy, dx in shifts], dtype=np.int64))
    st["gstate"][:, 0] = 1
    st["gstate"][0, 1:5] = (0, (W - 1) * 16, (H - 1) * 16, 8)                           # gazes at the clamps
    st["stats"] = np.array([RLE.stats(m) if any(s) else rng.integers(0, 99, 6).tolist() for m, s in zip(masks, shifts)], dtype=np.int64)
    st["counts"] = np.array([RLE.counts_row(m, cap) if any(s) else rng.integers(0, 99, cap) for m, s in zip(masks, shifts)], dtype=np.int32)
    pk = M.key_profiles(st["key"])
    st["prof_key"] = np.array([pk[b] if any(s) else rng.integers(0, 99, H + W) for b, s in enumerate(shifts)], dtype=np.int32)
    return st


_STATE_ORDER = ("key", "bits", "gstate", "stats", "counts", "prof_key", "mstate")
_STATE_TYPES = dict(key=torch.uint8, bits=torch.int32, gstate=torch.int64, stats=torch.int64, counts=torch.int32, prof_key=torch.int32,
                    mstate=torch.int64)


def _state_shift_abi(st, off):
    """fs_state_shift at the C ABI on guarded buffers -> the seven state arrays and motion on the host, and the moved bits on the device."""
    B, _, H, W = st["img"].shape
    cap = st["counts"].shape[1]
    P = (W + 31) // 32
    o = 1 if off else 0
    gi = Guarded(st["img"].size, torch.float32, body=torch.from_numpy(st["img"]), off=o)
    gs = Guarded(B * 4, torch.int64, body=torch.from_numpy(st["shift"]))
    g = {k: Guarded(st[k].size, _STATE_TYPES[k], body=torch.from_numpy(np.ascontiguousarray(st[k])), off=o if k == "key" else 0) for k in _STATE_ORDER}
    key2, bits2 = Guarded(st["key"].size, torch.uint8, off=o), Guarded(B * H * P)
    motion = Guarded(B * 6, torch.int64)
    need = hip.query("fs_state_shift_scratch_ints", B, H, W, cap)
    assert need == 12 * B + ((B * cap + 1) & ~1) + hip.query("fs_mask_rle_scratch_ints", B, H, W)
    scratch = Guarded(need)
    hip.call("fs_state_shift", gi.ptr, gs.ptr, g["key"].ptr, key2.ptr, g["bits"].ptr, bits2.ptr, g["gstate"].ptr, g["stats"].ptr, g["counts"].ptr,
             g["prof_key"].ptr, g["mstate"].ptr, motion.ptr, scratch.ptr, B, H, W, cap)
    torch.cuda.synchronize()
    assert gi.intact() and gs.intact() and key2.intact() and bits2.intact() and scratch.intact()
    assert np.array_equal(gs.body.cpu().numpy(), st["shift"].reshape(-1))
    still = [b for b in range(B) if not st["shift"][b, :2].any()]
    if len(still) == B:                                  # nobody moves: the spare buffers are not written at all
        assert bool((key2.body == _GARB[torch.uint8]).all()) and bool((bits2.body == _GARB[torch.int32]).all())
    out = {k: g[k].host(*st[k].shape).numpy() for k in _STATE_ORDER}
    out["motion"] = motion.host(B, 6).numpy()
    return out, g["bits"].body.view(B, H, P)


STATE_SHIFTS = {1: [[(1, 0)], [(0, -1)], [(-2, 7)], [(2, -2)], [(0, 0)]],
                3: [[(1, -1), (0, 0), (-2, 2)], [(0, 0), (0, 33), (0, 0)], [(0, 0), (0, 0), (0, 0)]]}


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_state_shift_and_motion_commit(H, W, B):
    cap = 7 if B == 1 else 8 * W + 1                     # a code that is cut, and the default capacity
    for n, shifts in enumerate(STATE_SHIFTS[B]):
        shifts = [(dy, dx) if abs(dx) < W else (dy, W - 1) for dy, dx in shifts]
        rng = np.random.default_rng(H * 1009 + W * 7 + B * 31 + n)
        st = _state(rng, B, H, W, cap, shifts)
        want = dict(zip(_STATE_ORDER + ("motion",), M.state_shift(st["img"], st["shift"], *(st[k] for k in _STATE_ORDER))))
        for off in ((False, True) if n < 2 else (False,)):
            got, bits_dev = _state_shift_abi(st, off)
            for k in want:
                assert np.array_equal(got[k], want[k]), (k, shifts, off)
            for b, s in enumerate(shifts):
                if not any(s):                           # a still viewer's tensors are untouched, garbage included
                    for k in _STATE_ORDER:
                        assert np.array_equal(got[k][b], st[k][b]), (k, b)
                else:                                    # the profile invariant, and the record is mask_rle's of the moved words
                    assert np.array_equal(got["prof_key"][b], M.key_profiles(got["key"][b:b + 1])[0])
            stats, counts = ops.mask_rle(bits_dev.clone(), W, max_runs=cap)
            for b, s in enumerate(shifts):
                if any(s):
                    assert np.array_equal(stats[b].cpu().numpy(), got["stats"][b]) and np.array_equal(counts[b].cpu().numpy(), got["counts"][b])
        # the motion commit on what the move left: the frame's profiles become the key's, the totals 0
        prof = rng.integers(0, 2 ** 20, (B, H + W)).astype(np.int32)
        for idx in ([], [B - 1], list(range(B))):
            gp = Guarded(prof.size, body=torch.from_numpy(prof))
            gk = Guarded(prof.size, body=torch.from_numpy(want["prof_key"]))
            gm = Guarded(B * 4, torch.int64, body=torch.from_numpy(want["mstate"]))
            ix = torch.tensor(idx, dtype=torch.int32, device="cuda") if idx else None
            hip.call("fs_motion_commit", None if ix is None else ix.data_ptr(), len(idx), gp.ptr, gk.ptr, gm.ptr, B, H, W)
            wk, wm = M.motion_commit(idx, prof, want["prof_key"], want["mstate"])
            assert np.array_equal(gk.host(B, H + W).numpy(), wk) and np.array_equal(gm.host(B, 4).numpy(), wm) and gp.intact()
            assert np.array_equal(gp.body.cpu().numpy(), prof.reshape(-1))


@pytest.mark.gpu
def test_state_shift_op_keeps_the_profile_invariant():
    """The ops on device tensors, chained as the session chains them: after the move and after the commit the key profiles are the
    profiles of the key frame."""
    B, H, W, cap = 3, 70, 96, 8 * 96 + 1
    rng = np.random.default_rng(5)
    canv = M.canvas(3, H + 16, W + 16, 4)
    first = np.stack([M.window(canv, 8, 8, H, W)] * B)
    then = np.stack([M.window(canv, 8 - 2, 8 + 3, H, W), M.window(canv, 8, 8, H, W), M.window(canv, 8 + 1, 8, H, W)])
    masks = np.stack([_blob(rng, H, W) for _ in range(B)])
    x0, x1 = torch.from_numpy(first).cuda(), torch.from_numpy(then).cuda()
    key, gstate = torch.zeros(B, 3, H, W, dtype=torch.uint8, device="cuda"), torch.zeros(B, 6, dtype=torch.int64, device="cuda")
    focus = torch.full((B, 2), 0.5, device="cuda")
    bits = ops.mask_bits(torch.from_numpy(masks).cuda())
    stats, counts = ops.mask_rle(bits, W)
    cat = torch.zeros(B, dtype=torch.int64, device="cuda")
    rec = [cat, stats, counts, bits]
    ops.gate_commit(x0, torch.arange(B, dtype=torch.int32, device="cuda"), key, gstate, focus, rec, rec)
    prof_key, mstate = torch.zeros(B, H + W, dtype=torch.int32, device="cuda"), torch.ones(B, 4, dtype=torch.int64, device="cuda")
    ops.motion_commit(torch.arange(B, dtype=torch.int32, device="cuda"), ops.frame_profiles(x0), prof_key, mstate, (H, W))
    assert torch.equal(prof_key, ops.key_profiles(key)) and not bool(mstate.any())
    prof = ops.frame_profiles(x1)
    shift = ops.profile_shift(prof, prof_key, gstate, (H, W), 5)
    assert shift[:, :2].tolist() == [[2, -3], [0, 0], [-1, 0]]
    g0 = gstate.clone()
    motion = ops.state_shift(x1, shift, key, torch.zeros_like(key), bits, torch.zeros_like(bits), gstate, stats, counts, prof_key, mstate)
    assert motion[:, [0, 1, 4, 5]].tolist() == [[2, -3, 2, -3], [0, 0, 0, 0], [-1, 0, -1, 0]] and torch.equal(motion[:, 2:4], shift[:, 2:])
    assert torch.equal(prof_key, ops.key_profiles(key))
    assert torch.equal(key, torch.from_numpy(R.q(then).astype(np.uint8)).cuda())       # the moved key is the new frame: nothing for the gate to see
    assert not bool(ops.gate_tiles(x1, key, 8).any())
    assert torch.equal(gstate[:, 1:5] - g0[:, 1:5], torch.tensor([[32, -48, 32, -48], [0, 0, 0, 0], [-16, 0, -16, 0]], device="cuda"))
    for b, (dy, dx) in enumerate(((2, -3), (0, 0), (-1, 0))):
        assert np.array_equal(RLE.unbits(bits[b].cpu().numpy(), W), M.move_mask(masks[b], dy, dx))
    s2, c2 = ops.mask_rle(bits, W)
    assert torch.equal(s2, stats) and torch.equal(c2, counts)
    ops.motion_commit(torch.tensor([0, 2], dtype=torch.int32, device="cuda"), prof, prof_key, mstate, (H, W))
    assert torch.equal(prof_key, ops.key_profiles(key)) and mstate[:, :2].tolist() == [[0, 0], [0, 0], [0, 0]]


@pytest.mark.gpu
def test_motion_entry_points_reject_bad_arguments():
    B, H, W, cap = 2, 16, 24, 5
    img, key, key2 = Guarded(B * 3 * H * W, torch.float32), Guarded(B * 3 * H * W, torch.uint8), Guarded(B * 3 * H * W, torch.uint8)
    prof, prof_key = Guarded(B * (H + W)), Guarded(B * (H + W))
    bits, bits2 = Guarded(B * H), Guarded(B * H)
    gstate, stats, mstate = Guarded(B * 6, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * 4, torch.int64)
    shift, motion, counts = Guarded(B * 4, torch.int64, body=torch.ones(B * 4)), Guarded(B * 6, torch.int64), Guarded(B * cap)
    scratch = Guarded(hip.query("fs_state_shift_scratch_ints", B, H, W, cap))
    idx = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    outs = [key, key2, prof, prof_key, bits, bits2, gstate, stats, mstate, motion, counts, scratch]

    def rejected(name, *args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call(name, *args)
        torch.cuda.synchronize()
        assert all(g.intact() and bool((g.body == _GARB[g.dtype]).all()) for g in outs), "a rejected call launched something"

    def each(name, good, bads):
        for i, bad in bads:
            a = list(good)
            a[i] = bad
            rejected(name, *a)

    each("fs_frame_profiles", [img.ptr, prof.ptr, B, H, W], ((0, None), (1, None), (2, 0), (3, 0), (4, -1)))
    each("fs_key_profiles", [key.ptr, prof.ptr, B, H, W], ((0, None), (1, None), (2, 0), (3, -2), (4, 0)))
    rejected("fs_frame_profiles", img.ptr, prof.ptr, 1, 65536, 32768)                  # H * W = 2^31
    rejected("fs_key_profiles", key.ptr, prof.ptr, 1, 1, 2807208)                      # 765 * W >= 2^31
    each("fs_profile_shift", [prof.ptr, prof_key.ptr, gstate.ptr, shift.ptr, B, H, W, 3, 6],
         ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (6, 0), (7, 0), (7, 4), (7, 256), (7, -1), (8, 9), (8, -1)))
    rejected("fs_profile_shift", prof.ptr, prof_key.ptr, gstate.ptr, shift.ptr, 1, 1024, 8000, 255, 6)      # beyond 64 KiB of LDS
    good = [img.ptr, shift.ptr, key.ptr, key2.ptr, bits.ptr, bits2.ptr, gstate.ptr, stats.ptr, counts.ptr, prof_key.ptr, mstate.ptr, motion.ptr,
            scratch.ptr, B, H, W, cap]
    each("fs_state_shift", good, [(i, None) for i in range(13)] + [(3, key.ptr), (5, bits.ptr), (12, scratch.ptr + 4), (13, 0), (14, 0), (15, 0), (16, 0)])
    each("fs_motion_commit", [idx.data_ptr(), 2, prof.ptr, prof_key.ptr, mstate.ptr, B, H, W],
         ((0, None), (1, 3), (1, -1), (2, None), (3, None), (4, None), (5, 0), (6, 0), (7, 0)))
    assert hip.query("fs_state_shift_scratch_ints", 0, H, W, cap) == 0 and hip.query("fs_state_shift_scratch_ints", B, H, W, 0) == 0


# ------------------------------------------------------------------------------------------------------------------ GPU: session ----
SIZE, PAD = 256, 16


def _frames(windows):
    """One frame per viewer: windows = [(canvas seed, y, x)], crops of seeded textured canvases of scale 4."""
    out = []
    for seed, y, x in windows:
        out.append(M.window(M.canvas(seed, SIZE + 2 * PAD, SIZE + 2 * PAD, 4), y, x, SIZE, SIZE))
    return torch.from_numpy(np.stack(out)).cuda()


def _focus(pixels):
    return torch.tensor([[py / (SIZE - 1), px / (SIZE - 1)] for py, px in pixels], dtype=torch.float32, device="cuda")


def _moved(rec, b, dy, dx, cap):
    """The reference move of viewer b's record: (cat, stats, counts, bits[, conf]) rows with cat and conf as they are."""
    mask = M.move_mask(RLE.unbits(rec[3][b].cpu().numpy(), SIZE), dy, dx)
    row = [rec[0][b:b + 1].clone(), torch.tensor([RLE.stats(mask)], dtype=torch.int64, device="cuda"),
           torch.tensor(np.array([RLE.counts_row(mask, cap)]), dtype=torch.int32, device="cuda"), torch.from_numpy(RLE.bits(mask)[None]).cuda()]
    return tuple(row + [t[b:b + 1].clone() for t in rec[4:]])


@pytest.mark.gpu
@pytest.mark.parametrize("component", [None, 8])
def test_session_carries_the_record_along_a_moving_window(served, component):
    """Viewer 0's camera translates over a textured canvas and its gaze goes with it; viewer 1 stands still."""
    module, calls, TP = served
    kw = dict(score=True) if component is None else dict(score=True, component=8)
    cap = 8 * SIZE + 1
    X1, F1 = _frames([(25, PAD, PAD), (31, PAD, PAD)]), _focus([(128, 128), (100, 140)])
    X2, F2 = _frames([(25, PAD - 3, PAD + 5), (31, PAD, PAD)]), _focus([(131, 123), (100, 140)])       # the content moves by (3, -5)
    X3, F3 = _frames([(25, PAD - 1, PAD + 4), (31, PAD, PAD)]), _focus([(129, 124), (100, 140)])       # and by a further (-2, 1)
    X4 = _frames([(26, PAD, PAD), (31, PAD, PAD)])                                                    # a cut to other content

    # without motion compensation the moved window re-makes the record: the defect
    off = GazeSession(module, 2, (SIZE, SIZE), **kw)
    out = off.step(X1, F1)
    assert len(out) == 6 and out[-1].shape == (2, 8) and out[-1][:, 0].tolist() == [R.RUN_INIT] * 2           # the parent's tuple
    assert not hasattr(off, "_key2")
    assert off.step(X2, F2)[-1][:, 0].tolist() == [R.RUN_SCENE, R.REUSE]

    calls.clear()
    s = GazeSession(module, 2, (SIZE, SIZE), motion_px=8, **kw)
    *rec, gate, motion = s.step(X1, F1)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and calls == [2]
    assert motion.dtype == torch.int64 and motion.shape == (2, 6) and not motion.is_cuda and motion.tolist() == [[0] * 6] * 2
    first = [t.clone() for t in rec]
    area = first[1][:, 0].tolist()
    print(f"areas {area}, boxes {first[1][:, 1:5].tolist()}")
    assert all(0 < a < SIZE * SIZE for a in area), "the seeds must give masks that are neither empty nor full"
    assert torch.equal(s._prof_key, ops.key_profiles(s._key))

    # 2: the window moves by (3, -5): the record moves with it, nothing runs
    *rec, gate, motion = s.step(X2, F2)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and calls == [2]
    assert motion[:, :2].tolist() == [[3, -5], [0, 0]] and motion[:, 4:].tolist() == [[3, -5], [0, 0]]
    assert gate[0, 1:6].tolist() == [0] * 5              # the moved key is the new frame, the moved key gaze the new gaze
    assert _same(_row(rec, 0), _moved(first, 0, 3, -5, cap)) and _same(_row(rec, 1), _row(first, 1))
    # (this module's mask is a strip on the frame's left edge whatever it is shown: five columns to the left it has left the frame, and
    # the moved record is the empty mask's; test_session_moves_the_record_inside_the_frame goes the other way)
    assert torch.equal(s._prof_key, ops.key_profiles(s._key))
    second = [t.clone() for t in rec]

    # 3: a further (-2, 1); a step in which nobody runs allocates nothing
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    *rec, gate, motion = s.step(X3, F3)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"a moved REUSE step raised the peak by {grew} bytes")
    assert grew == 0
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and calls == [2]
    assert motion[:, :2].tolist() == [[-2, 1], [0, 0]] and motion[:, 4:].tolist() == [[1, -4], [0, 0]]
    assert _same(_row(rec, 0), _moved(second, 0, -2, 1, cap)) and _same(_row(rec, 1), _row(first, 1))
    assert torch.equal(rec[0], first[0]) and torch.equal(rec[4].view(torch.int32), first[4].view(torch.int32))   # cat and conf as they were made

    # 4: a cut for viewer 0: a fresh record, totals 0; viewer 1 keeps its record
    *rec, gate, motion = s.step(X4, F3)
    assert gate[:, 0].tolist() == [R.RUN_SCENE, R.REUSE] and calls == [2, 1]
    assert motion[:, 4:].tolist() == [[0, 0], [0, 0]] and s._mstate.cpu().tolist() == [[0] * 4] * 2
    fresh = module.predict_instances(X4[:1], F3[:1], return_bits=True, return_score=True, **({} if component is None else dict(component=8)))
    assert _same(_row(rec, 0), tuple(fresh[:5])) and _same(_row(rec, 1), _row(first, 1))
    assert torch.equal(s._prof_key, ops.key_profiles(s._key))
    *rec, gate, motion = s.step(X4, F3)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and motion[:, [0, 1, 4, 5]].tolist() == [[0] * 4] * 2
    assert s.counts == {0: 7, 1: 2, 2: 0, 3: 1, 4: 0, 5: 0, 6: 0, 7: 0}


@pytest.mark.gpu
def test_session_moves_the_record_inside_the_frame(served):
    """One viewer, the content moving by (-3, 5) and back: the moved mask stays in the frame, and moving back loses only what left it."""
    module, calls, TP = served
    cap = 8 * SIZE + 1
    X1, F1 = _frames([(25, PAD, PAD)]), _focus([(128, 128)])
    X2, F2 = _frames([(25, PAD + 3, PAD - 5)]), _focus([(125, 133)])
    calls.clear()
    s = GazeSession(module, 1, (SIZE, SIZE), motion_px=8)
    cat, stats, counts, bits, gate, motion = s.step(X1, F1)
    first = [t.clone() for t in (cat, stats, counts, bits)]
    mask = RLE.unbits(bits[0].cpu().numpy(), SIZE)
    want = M.move_mask(mask, -3, 5)
    assert int(want.sum()) > 0, "the move must keep set pixels in the frame"
    *rec, gate, motion = s.step(X2, F2)
    assert gate[:, 0].tolist() == [R.REUSE] and calls == [1] and motion.tolist()[0][:2] == [-3, 5] and motion.tolist()[0][4:] == [-3, 5]
    assert _same(tuple(rec), _moved(first, 0, -3, 5, cap)) and int(rec[1][0, 0]) == int(want.sum())
    assert np.array_equal(RLE.unbits(rec[3][0].cpu().numpy(), SIZE), want)
    *rec, gate, motion = s.step(X1, F1)                  # and back: the rows that left the frame do not return
    assert gate[:, 0].tolist() == [R.REUSE] and calls == [1] and motion.tolist()[0][:2] == [3, -5] and motion.tolist()[0][4:] == [0, 0]
    assert np.array_equal(RLE.unbits(rec[3][0].cpu().numpy(), SIZE), M.move_mask(want, 3, -5))
    assert s.counts[R.REUSE] == 2 and s.counts[R.RUN_INIT] == 1
