"""The gaze gate and GazeSession: ops.gate_tiles / gate_decide / gate_commit (fs_gate_tiles, fs_gate_decide, fs_gate_commit) and
fovealseg.GazeSession.

All of it is integer work and is held bit for bit.  tests/gate_ref.py restates the definitions in numpy; the reference has no
counterpart (unpinned), so the CPU tests pin gate_ref to hand-derived answers on a 16 x 24 frame with 8 x 8 tiles, and the GPU tests
hold the kernels to gate_ref and the session to module.predict_instances.  At the C ABI every output sits between sentinel guard
bands and is pre-filled with garbage."""
import numpy as np
import pytest
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg.session import GazeSession, px_to_thr2, OFF2

import gate_ref as R
import rle_ref as RLE

# ------------------------------------------------------------------------------------------------------------------ hand-built -----
HH, HW, HT = 16, 24, 8                                   # the hand frame: 2 x 3 tiles of 8 x 8, n_el = 192 each
TOP_Y, TOP_X = (HH - 1) * 16, (HW - 1) * 16              # 240, 368: the gaze range in 1/16-pixel units


def fo(gy, gx):
    """The focus that lands on (gy, gx) in 1/16-pixel units on the hand frame."""
    return np.array([gy / TOP_Y, gx / TOP_X], dtype=np.float32)


def hand_mask():
    m = np.zeros((HH, HW), dtype=bool)
    m[8:12, 8:10] = True                                 # rows 8 .. 11, columns 8 .. 9: area 8, box [8, 8, 2, 4], inside tile (1, 1)
    return m


HAND_RULE = dict(level=1, scene_tiles=2, roi_tiles=0, margin=0, saccade2=4096, fixation2=256, max_age=3, inside_on=1)
KEY = (128, 128)                                         # the key gaze: pixel (8, 8), a set pixel


def _sad(**tiles):
    s = np.zeros((2, 3), dtype=np.int64)
    for k, v in tiles.items():
        s[int(k[1]), int(k[2])] = v
    return s


# name -> (sad, gstate, g = (gy, gx), force, rule overrides, expected gate row); every expected row derived by hand:
# gate = (code, n_changed, n_roi_changed, sad_total, d2_key, d2_prev, inside_bit, age + 1); a tile is changed iff sad > 1 * 192
HAND = {
    "reuse": (_sad(), [1, *KEY, *KEY, 0], KEY, None, {}, [0, 0, 0, 0, 0, 0, 1, 1]),
    "at_the_level_is_not_changed": (_sad(t11=192), [1, *KEY, *KEY, 0], KEY, None, {}, [0, 0, 0, 192, 0, 0, 1, 1]),
    "forced": (_sad(), [1, *KEY, *KEY, 0], KEY, 1, {}, [7, 0, 0, 0, 0, 0, 1, 1]),
    "forced_over_init": (_sad(), [0, *KEY, *KEY, 0], KEY, 1, {}, [7, 0, 0, 0, 0, 0, 1, 1]),
    "force_zero_is_no_force": (_sad(), [1, *KEY, *KEY, 0], KEY, 0, {}, [0, 0, 0, 0, 0, 0, 1, 1]),
    "init": (_sad(), [0, *KEY, *KEY, 5], KEY, None, {}, [1, 0, 0, 0, 0, 0, 1, 6]),
    # the previous gaze 80 units to the right: d2_prev = 6400 > 4096
    "saccade": (_sad(), [1, *KEY, 128, 208, 0], KEY, None, {}, [2, 0, 0, 0, 0, 6400, 1, 1]),
    "saccade_at_the_threshold_is_none": (_sad(), [1, *KEY, 128, 192, 0], KEY, None, {}, [0, 0, 0, 0, 0, 4096, 1, 1]),
    "saccade_over_scene": (_sad(t00=193, t01=193, t02=193), [1, *KEY, 128, 208, 0], KEY, None, {}, [2, 3, 0, 579, 0, 6400, 1, 1]),
    "scene": (_sad(t00=193, t01=193, t02=193), [1, *KEY, *KEY, 0], KEY, None, {}, [3, 3, 0, 579, 0, 0, 1, 1]),
    "scene_over_roi": (_sad(t00=193, t01=193, t02=193, t11=200), [1, *KEY, *KEY, 0], KEY, None, {}, [3, 4, 1, 779, 0, 0, 1, 1]),
    "two_changed_tiles_are_no_scene": (_sad(t00=193, t02=500), [1, *KEY, *KEY, 0], KEY, None, {}, [0, 2, 0, 693, 0, 0, 1, 1]),
    "roi_box_tile": (_sad(t11=193), [1, *KEY, *KEY, 0], KEY, None, {}, [4, 1, 1, 193, 0, 0, 1, 1]),
    # margin 1 grows the box to columns 7 .. 10 and rows 7 .. 12: tiles (0..1, 0..1)
    "roi_margin": (_sad(t00=193), [1, *KEY, *KEY, 0], KEY, None, dict(margin=1), [4, 1, 1, 193, 0, 0, 1, 1]),
    "roi_tolerated": (_sad(t11=193), [1, *KEY, *KEY, 0], KEY, None, dict(roi_tiles=1), [0, 1, 1, 193, 0, 0, 1, 1]),
    # the gaze rests on pixel (2, 20), tile (0, 2), far from the box: that tile is of interest too
    "roi_gaze_tile": (_sad(t02=193), [1, 32, 320, 32, 320, 0], (32, 320), None, {}, [4, 1, 1, 193, 0, 0, 0, 1]),
    # pixel (13, 8) is clear and 80 units from the key gaze; the previous gaze was there already
    "gaze": (_sad(), [1, *KEY, 208, 128, 0], (208, 128), None, {}, [5, 0, 0, 0, 6400, 0, 0, 1]),
    "gaze_at_the_threshold_is_none": (_sad(), [1, *KEY, 128, 144, 0], (128, 144), None, dict(inside_on=0), [0, 0, 0, 0, 256, 0, 1, 1]),
    # pixel (11, 8) is set and 48 units away: the mask keeps the record, unless the rule is off
    "inside_over_distance": (_sad(), [1, *KEY, 176, 128, 0], (176, 128), None, {}, [0, 0, 0, 0, 2304, 0, 1, 1]),
    "inside_off": (_sad(), [1, *KEY, 176, 128, 0], (176, 128), None, dict(inside_on=0), [5, 0, 0, 0, 2304, 0, 1, 1]),
    # rounding to the gaze pixel: gy = 184 is pixel (184 + 8) >> 4 = 12, below the mask
    "gaze_pixel_rounds_half_up": (_sad(), [1, *KEY, 184, 128, 0], (184, 128), None, {}, [5, 0, 0, 0, 3136, 0, 0, 1]),
    "age": (_sad(), [1, *KEY, *KEY, 3], KEY, None, {}, [6, 0, 0, 0, 0, 0, 1, 4]),
    "age_not_yet": (_sad(), [1, *KEY, *KEY, 2], KEY, None, {}, [0, 0, 0, 0, 0, 0, 1, 3]),
    "age_off": (_sad(), [1, *KEY, *KEY, 99], KEY, None, dict(max_age=0), [0, 0, 0, 0, 0, 0, 1, 100]),
    "age_last": (_sad(), [1, *KEY, 208, 128, 3], (208, 128), None, {}, [5, 0, 0, 0, 6400, 0, 0, 4]),
    # the last row and column: pixel (15, 23), tile (1, 2)
    "last_row_and_column": (_sad(t12=193), [1, TOP_Y, TOP_X, TOP_Y, TOP_X, 0], (TOP_Y, TOP_X), None, {}, [4, 1, 1, 193, 0, 0, 0, 1]),
}


# T = 16 on the same frame: one row of two tiles, the second 16 x 8 with n_el = 384 against 768
RAGGED = {
    "ragged_tile_changed": ([[768, 385]], [0, 1, 0, 1153, 0, 0, 1, 1]),
    "ragged_tile_at_its_level": ([[769, 384]], [4, 1, 1, 1153, 0, 0, 1, 1]),
}


def _ragged_inputs(name):
    inp, rule, g, _ = _hand_inputs("reuse")
    inp["sad"] = np.array([RAGGED[name][0]], dtype=np.int32)
    return inp, rule, RAGGED[name][1]


def _hand_inputs(name):
    sad, gstate, g, force, over, want = HAND[name]
    rule = dict(HAND_RULE, **over)
    m = hand_mask()
    return dict(sad=sad[None].astype(np.int32), gstate=np.array([gstate], dtype=np.int64), focus=fo(*g)[None],
                stats=np.array([RLE.stats(m)], dtype=np.int64), bits=RLE.bits(m)[None],
                force=None if force is None else np.array([force], dtype=np.int32)), rule, g, want


def _ref_decide(inp, rule, H=HH, W=HW, T=HT):
    return R.decide(inp["sad"], inp["gstate"], inp["focus"], inp["stats"], inp["bits"], inp["force"], H, W, T, rule["level"],
                    rule["scene_tiles"], rule["roi_tiles"], rule["margin"], rule["saccade2"], rule["fixation2"], rule["max_age"], rule["inside_on"])


# ------------------------------------------------------------------------------------------------------------------ CPU ------------
def test_gate_ref_pixel_code():
    # fl32(0.5/255) * 255 and fl32(1.5/255) * 255 round to exactly 0.5 and 1.5 in fp32: ties, which go to the even neighbour
    assert R.q([0.5 / 255, 1.5 / 255, -0.1, 1.2, float("nan")]).tolist() == [0, 2, 0, 255, 0]
    assert R.q([float("inf"), float("-inf"), -0.0, 1.0, 0.0]).tolist() == [255, 0, 0, 255, 0]
    assert R.q(np.arange(256, dtype=np.float32) / np.float32(255)).tolist() == list(range(256))       # k/255 gives k


def hand_frame():
    """A 16 x 24 frame against the key frame "10 everywhere", with a handful of differences placed by hand."""
    key = np.full((1, 3, HH, HW), 10, dtype=np.uint8)
    img = np.full((1, 3, HH, HW), 10 / 255, dtype=np.float32)
    img[0, 0, 0, 0] = 13 / 255                           # tile (0,0): one pixel 3 levels up
    img[0, 2, 7, 23] = 0.0                               # tile (0,2), its last pixel: 10 levels down
    img[0, 1, 8:16, 8:16] = 12 / 255                     # tile (1,1): a whole channel 2 levels up, 64 * 2
    img[0, 2, 15, 23] = float("nan")                     # tile (1,2): NaN codes as 0, 10 levels
    img[0, 0, 15, 23] = 1.2                              #             and 1.2 as 255, 245 levels
    return img, key, [[3, 0, 10], [0, 128, 255]]


def test_gate_ref_hand_sad_table():
    img, key, want = hand_frame()
    assert R.tiles(img, key, HT).tolist() == [want]
    assert R.tiles(img, R.q(img).astype(np.uint8), HT).tolist() == [[[0] * 3] * 2]
    # T = 16: one row of tiles, the second 16 x 8 (ragged)
    assert R.tiles(img, key, 16).tolist() == [[[3 + 128, 10 + 255]]]


def test_hand_mask_stats():
    m = hand_mask()
    assert RLE.stats(m)[:5] == [8, 8, 8, 2, 4]
    assert R.bit(RLE.bits(m), 8, 8) == 1 and R.bit(RLE.bits(m), 11, 9) == 1 and R.bit(RLE.bits(m), 12, 8) == 0 and R.bit(RLE.bits(m), 8, 10) == 0
    assert R.roi_tiles(RLE.stats(m), 8, 8, HH, HW, HT, 0) == {(1, 1)}
    assert R.roi_tiles(RLE.stats(m), 2, 20, HH, HW, HT, 0) == {(1, 1), (0, 2)}
    assert R.roi_tiles(RLE.stats(m), 8, 8, HH, HW, HT, 1) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert R.roi_tiles(RLE.stats(m), 8, 8, HH, HW, HT, 100) == {(ty, tx) for ty in range(2) for tx in range(3)}        # clipped
    assert R.roi_tiles([0, 0, 0, 0, 0, 1], 15, 23, HH, HW, HT, 100) == {(1, 2)}                                        # an empty mask has no box


def test_gate_ref_gaze_units():
    assert R.gaze(0.0, 16) == 0 and R.gaze(1.0, 16) == 240 and R.gaze(0.5, 16) == 120
    assert R.gaze(-3.0, 16) == 0 and R.gaze(7.0, 16) == 240 and R.gaze(float("nan"), 16) == 0 and R.gaze(float("inf"), 1) == 0
    assert R.gaze(0.5, 2) == 8 and R.gaze(np.float32(1.5 / 16), 2) == 2                      # ties go to the even neighbour
    for gy, gx in ((128, 128), (208, 128), (184, 128), (32, 320), (TOP_Y, TOP_X)):
        f = fo(gy, gx)
        assert (R.gaze(f[0], HH), R.gaze(f[1], HW)) == (gy, gx)
    assert R.d2(3, -4, 0, 0) == 25 and R.d2(2 ** 30, 0, 0, 2 ** 30) == 2 ** 61


@pytest.mark.parametrize("name", sorted(HAND))
def test_gate_ref_hand_decisions(name):
    inp, rule, g, want = _hand_inputs(name)
    assert _ref_decide(inp, rule).tolist() == [want]


@pytest.mark.parametrize("name", sorted(RAGGED))
def test_gate_ref_ragged_tiles(name):
    inp, rule, want = _ragged_inputs(name)
    assert _ref_decide(inp, rule, T=16).tolist() == [want]


def test_hand_cases_cover_every_code_and_precedence():
    assert {HAND[k][5][0] for k in HAND} == set(range(8))
    for k in ("saccade_over_scene", "scene_over_roi", "inside_over_distance", "age_last", "forced_over_init"):
        assert k in HAND


def test_gate_ref_commit():
    img, key, _ = hand_frame()
    img = np.concatenate([img, np.full_like(img, 0.5)])
    key = np.concatenate([key, key])
    gstate = np.array([[0, 1, 2, 3, 4, 5], [1, 6, 7, 8, 9, 10]], dtype=np.int64)
    focus = np.stack([fo(128, 144), fo(32, 320)])
    src, dst = [np.array([77])], [np.array([5, 6])]
    k2, g2, d2 = R.commit(img, [1], key, gstate, focus, src, dst)
    assert g2.tolist() == [[0, 1, 2, 128, 144, 6], [1, 32, 320, 32, 320, 0]]
    assert d2[0].tolist() == [5, 77] and np.array_equal(k2[0], key[0]) and bool((k2[1] == 128).all())       # 0.5 * 255 = 127.5 -> 128
    k3, g3, d3 = R.commit(img, [], key, gstate, focus, src, dst)
    assert np.array_equal(k3, key) and d3[0].tolist() == [5, 6] and g3.tolist() == [[0, 1, 2, 128, 144, 6], [1, 6, 7, 32, 320, 11]]


class _Stub:
    """What GazeSession asks of a module before it touches the device."""
    training = False


def test_host_conversion_of_the_thresholds():
    assert px_to_thr2(0) == 0 and px_to_thr2(1) == 256 and px_to_thr2(0.5) == 64 and px_to_thr2(4) == 4096
    assert px_to_thr2(7.68) == 15099                    # 122.88 ** 2 = 15099.49
    assert px_to_thr2(1e30) == OFF2 == 2 ** 62
    assert R.thr2(7.68) == 15099 and R.thr2(25.6) == 167772
    s = GazeSession(_Stub(), 2, (256, 256))
    assert (s.tile, s.level, s.th, s.tw, s.scene_tiles, s.roi_tiles, s.roi_margin, s.max_age, s.inside_on, s.score) == (32, 8, 8, 8, 16, 0, 16, 0, True, False)
    assert s.fixation2 == 15099 and s.saccade2 == 167772 and s.cap == 8 * 256 + 1           # 0.03 * 256 and 0.10 * 256 pixels
    assert s.counts == {c: 0 for c in range(8)}
    s = GazeSession(_Stub(), 1, (70, 45), tile=16, scene_frac=0.5, saccade_px=None, fixation_px=2, max_runs=9, max_age=3, reuse_inside_mask=False, score=True)
    assert (s.th, s.tw, s.scene_tiles, s.saccade2, s.fixation2, s.cap, s.max_age, s.inside_on, s.score) == (5, 3, 7, 2 ** 62, 1024, 9, 3, False, True)
    assert GazeSession(_Stub(), 1, (100, 300)).fixation2 == 2304                                       # 0.03 * min(H, W) = 3 pixels
    s.reset()                                           # before the first step: nothing to forget
    s.reset([0])


@pytest.mark.parametrize("kw", [dict(tile=12), dict(tile=128), dict(tile=True), dict(level=255), dict(level=-1), dict(level=2.5), dict(roi_tiles=-1),
                                dict(roi_margin=-1), dict(max_age=-1), dict(fixation_px=-1.0), dict(saccade_px=-2), dict(saccade_px=float("nan")),
                                dict(scene_frac=-0.1), dict(max_runs=0)])
def test_session_rejects_bad_parameters(kw):
    with pytest.raises(ValueError):
        GazeSession(_Stub(), 2, (64, 64), **kw)


def test_session_rejects_bad_sizes_shapes_and_train_mode():
    for batch, size in ((0, (64, 64)), (2, (0, 64)), (2, (64,)), (2, (64, 64, 3)), (1, (2 ** 16, 2 ** 15)), (1.5, (64, 64))):
        with pytest.raises(ValueError):
            GazeSession(_Stub(), batch, size)
    mod = _Stub()
    s = GazeSession(mod, 2, (64, 48))
    X, Fp = torch.zeros(2, 3, 64, 48), torch.zeros(2, 2)
    for img, focus in ((X[:1], Fp[:1]), (X[:, :, :32], Fp), (X[:, :2], Fp), (X.transpose(2, 3), Fp), (X, Fp[:1]), (X, torch.zeros(2, 3)),
                       (X.double(), Fp), (X.numpy(), Fp), (X, Fp)):                            # the last: the right shapes, but no GPU tensors
        with pytest.raises(ValueError):
            s.step(img, focus)
    with pytest.raises(ValueError):
        s.reset([2])
    mod.training = True
    with pytest.raises(RuntimeError):
        s.step(X, Fp)
    assert s.counts == {c: 0 for c in range(8)}


def test_the_ctypes_table_binds_the_gate():
    assert hip.SIGNATURES["fs_gate_tiles"] == "ppp" + "iiii"
    assert hip.SIGNATURES["fs_gate_decide"] == "p" * 7 + "i" * 8 + "ll" + "ii"
    assert hip.SIGNATURES["fs_gate_commit"] == "pp" + "i" + "p" * 13 + "iiii"
    assert fovealseg.GazeSession is GazeSession and "GazeSession" in fovealseg.__all__
    assert sorted(ops.GATE_CODES) == list(range(8)) and ops.GATE_RUNS == R.RUNS and ops.GATE_CODES[2] == "HOLD_SACCADE"
    for bad in (12, 0, True, 7.5):
        with pytest.raises(ValueError):
            fovealseg.gaze._gate_tile(bad)


# ---- the seeded viewers of the decide test -----------------------------------------------------------------------------------------
SH, SW, ST, SB, SEED = 40, 56, 8, 257, 22
SEEDED_RULE = dict(level=2, scene_tiles=8, roi_tiles=0, margin=4, saccade2=R.thr2(10), fixation2=R.thr2(3), max_age=4)


def seeded_viewers(seed=SEED):
    """257 viewers on a 40 x 56 frame, 5 x 7 tiles of 8 x 8: masks, states, gazes, tile sums and force flags drawn from one seed."""
    rng = np.random.default_rng(seed)
    th, tw = SH // ST, SW // ST
    top_y, top_x = (SH - 1) * 16, (SW - 1) * 16
    masks = np.zeros((SB, SH, SW), dtype=bool)
    gstate = np.zeros((SB, 6), dtype=np.int64)
    focus = np.zeros((SB, 2), dtype=np.float32)
    sad = np.zeros((SB, th, tw), dtype=np.int32)
    for b in range(SB):
        if rng.random() < 0.9:                           # a blob: a rectangle with holes; one viewer in ten has an empty mask
            y0, x0 = int(rng.integers(0, SH - 4)), int(rng.integers(0, SW - 4))
            y1, x1 = int(rng.integers(y0 + 1, min(SH, y0 + 20) + 1)), int(rng.integers(x0 + 1, min(SW, x0 + 24) + 1))
            masks[b, y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < 0.8
        gk = np.array([rng.integers(0, top_y + 1), rng.integers(0, top_x + 1)])
        jump = (0, 0, 0, 40, 40, 100, 400)[int(rng.integers(0, 7))]          # the gaze against the key gaze, in 1/16 pixels
        g = np.clip(gk + rng.integers(-jump, jump + 1, 2), 0, (top_y, top_x))
        step = (0, 0, 0, 0, 60, 300)[int(rng.integers(0, 6))]                 # the previous gaze against this one
        gp = np.clip(g + rng.integers(-step, step + 1, 2), 0, (top_y, top_x))
        gstate[b] = (rng.random() < 0.9, gk[0], gk[1], gp[0], gp[1], rng.integers(0, 6))
        focus[b] = (g[0] / top_y, g[1] / top_x)
        n = (0, 0, 0, 1, 2, 5, 12, 35)[int(rng.integers(0, 8))]              # changed tiles
        sad[b] = rng.integers(0, 2 * 3 * ST * ST + 1, (th, tw))               # at or below the level of 2
        for t in rng.choice(th * tw, n, replace=False):
            sad[b, t // tw, t % tw] = rng.integers(2 * 3 * ST * ST + 1, 255 * 3 * ST * ST + 1)
    focus[0], focus[1], focus[2], focus[3] = (1.0, 1.0), (float("nan"), float("nan")), (-0.5, 2.0), (1.0, 0.0)   # the last row and column; no gaze; out of range
    force = (rng.random(SB) < 0.08).astype(np.int32) * rng.integers(1, 1000, SB).astype(np.int32)
    return dict(masks=masks, gstate=gstate, focus=focus, sad=sad, force=force)


def seeded_reference(v, with_force, inside_on):
    stats = np.array([RLE.stats(m) for m in v["masks"]], dtype=np.int64)
    bits = np.stack([RLE.bits(m) for m in v["masks"]])
    inp = dict(sad=v["sad"], gstate=v["gstate"], focus=v["focus"], stats=stats, bits=bits, force=v["force"] if with_force else None)
    return _ref_decide(inp, dict(SEEDED_RULE, inside_on=inside_on), SH, SW, ST)


def test_seeded_viewers_reach_every_code():
    v = seeded_viewers()
    gate = seeded_reference(v, True, 1)
    hist = np.bincount(gate[:, 0], minlength=8)
    print("codes of the seeded viewers:", hist.tolist())
    assert hist.sum() == SB and int(hist.min()) >= 5
    assert int(np.bincount(seeded_reference(v, False, 0)[:, 0], minlength=8)[1:7].min()) >= 5
    assert seeded_reference(v, True, 1)[0, 6] == R.bit(RLE.bits(v["masks"][0]), SH - 1, SW - 1)        # viewer 0 looks at the last pixel


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ------
GUARD = 64
_SENT = {torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5B5A5A5A5B, torch.uint8: 0xA5, torch.float32: 777.25}
_GARB = {torch.int32: 0x3C3C3C3D, torch.int64: 0x3C3C3C3D3C3C3C3D, torch.uint8: 0x3D, torch.float32: -12345.5}


class Guarded:
    """n elements pre-filled with garbage (or `body`) between two bands of GUARD sentinels; `off` elements off a 16-byte boundary."""

    def __init__(self, n, dtype=torch.int32, body=None, off=0):
        self.n, self.dtype = n, dtype
        lead = 2 * GUARD + off                           # GUARD elements of any of these types are a multiple of 16 bytes
        self.whole = torch.full((lead + n + GUARD,), _SENT[dtype], device="cuda", dtype=dtype)
        self.body = self.whole[lead:lead + n]
        self.lead = lead
        if body is None:
            self.body.fill_(_GARB[dtype])
        else:
            self.body.copy_(torch.as_tensor(body).reshape(-1).to(dtype))
        assert self.body.data_ptr() % 16 == (off * self.body.element_size()) % 16

    @property
    def ptr(self):
        return self.body.data_ptr()

    def intact(self):
        s = _SENT[self.dtype]
        return bool((self.whole[:self.lead] == s).all()) and bool((self.whole[self.lead + self.n:] == s).all())

    def host(self, *shape):
        torch.cuda.synchronize()
        assert self.intact(), "a guard band was written"
        return self.body.cpu().view(*shape)


def _tiles(img, key, T, off=False):
    """fs_gate_tiles at the C ABI -> sad (B,th,tw) on the host; off: img one float and key one byte off their alignment."""
    B, _, H, W = img.shape
    th, tw = -(-H // T), -(-W // T)
    gi = Guarded(img.size, torch.float32, body=torch.from_numpy(img), off=1 if off else 0)
    gk = Guarded(key.size, torch.uint8, body=torch.from_numpy(key), off=1 if off else 0)
    sad = Guarded(B * th * tw)
    hip.call("fs_gate_tiles", gi.ptr, gk.ptr, sad.ptr, B, H, W, T)
    got = sad.host(B, th, tw)
    assert gi.intact() and gk.intact()
    assert torch.equal(gi.body.cpu(), torch.from_numpy(img).reshape(-1)) or np.isnan(img).any()
    assert torch.equal(gk.body.cpu(), torch.from_numpy(key).reshape(-1))
    return got


def _check_tiles(img, key, T, off=False):
    got = _tiles(img, key, T, off)
    assert got.dtype == torch.int32
    assert torch.equal(got.long(), torch.from_numpy(R.tiles(img, key, T)))
    return got


TILE_SHAPES = [(1, 1, 1, 8), (2, 8, 8, 8), (3, 70, 45, 32), (2, 64, 72, 16), (2, 65, 128, 64), (1, 130, 260, 32),
               (1, 9, 264, 8)]                          # the four-pixel form with 32 tiles a 256-column segment, and a second segment


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,T", TILE_SHAPES)
def test_gate_tiles(B, H, W, T):
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W * 7 + T)
    shape = (B, 3, H, W)
    key = rng.integers(0, 256, shape).astype(np.uint8)
    img = (rng.integers(0, 256, shape).astype(np.float32) / np.float32(255))                          # seeded k/255 frames
    offs = (False, True) if (H, W) == (64, 72) else (False,)
    for off in offs:
        _check_tiles(img, key, T, off)
        same = key.astype(np.float32) / np.float32(255)
        assert not bool(_check_tiles(same, key, T, off).any())                                       # an identical pair: all zero
        # one grey level of difference at the last pixel of the last (ragged) tile, in channel 2
        one = same.copy()
        one[B - 1, 2, H - 1, W - 1] = (int(key[B - 1, 2, H - 1, W - 1]) ^ 1) / np.float32(255)
        got = _check_tiles(one, key, T, off)
        assert int(got.sum()) == 1 and int(got[B - 1, -1, -1]) == 1
        # out-of-range and NaN pixels
        wild = img.copy()
        pick = rng.random(shape)
        wild[pick < 0.1] = np.float32("nan")
        wild[(pick >= 0.1) & (pick < 0.2)] = -3.5
        wild[(pick >= 0.2) & (pick < 0.3)] = 1.0 + 2.0 ** -20
        wild[(pick >= 0.3) & (pick < 0.35)] = np.float32("inf")
        wild[(pick >= 0.35) & (pick < 0.4)] = np.float32("-inf")
        wild[(pick >= 0.4) & (pick < 0.5)] = rng.random(int(((pick >= 0.4) & (pick < 0.5)).sum()), dtype=np.float32)
        _check_tiles(wild, key, T, off)
    if T == 64:
        got = _check_tiles(np.ones(shape, dtype=np.float32), np.zeros(shape, dtype=np.uint8), T)
        assert int(got[0, 0, 0]) == 3133440 and int(got[0, 1, 0]) == 3 * 255 * 64 * (H - 64)          # a full tile, a ragged one
    img_d, key_d = torch.from_numpy(img).cuda(), torch.from_numpy(key).cuda()
    want = torch.from_numpy(R.tiles(img, key, T)).int()
    out = torch.full_like(want, 7).cuda()
    assert ops.gate_tiles(img_d, key_d, T, out=out) is out and torch.equal(out.cpu(), want)           # the op, into a given tensor
    assert torch.equal(ops.gate_tiles(img_d, key_d, tile=T).cpu(), want)


def _decide(inp, rule, H, W, T):
    """fs_gate_decide at the C ABI -> gate (B,8) on the host; the inputs sit in guarded buffers and are compared afterwards."""
    B = inp["sad"].shape[0]
    bufs = {k: Guarded(inp[k].size, dt, body=torch.from_numpy(np.ascontiguousarray(inp[k])))
            for k, dt in (("sad", torch.int32), ("gstate", torch.int64), ("focus", torch.float32), ("stats", torch.int64), ("bits", torch.int32))}
    force = None if inp["force"] is None else torch.from_numpy(inp["force"]).cuda()
    gate = Guarded(B * 8, torch.int64)
    hip.call("fs_gate_decide", bufs["sad"].ptr, bufs["gstate"].ptr, bufs["focus"].ptr, bufs["stats"].ptr, bufs["bits"].ptr,
             None if force is None else force.data_ptr(), gate.ptr, B, H, W, T, rule["level"], rule["scene_tiles"], rule["roi_tiles"],
             rule["margin"], rule["saccade2"], rule["fixation2"], rule["max_age"], rule["inside_on"])
    got = gate.host(B, 8)
    for k, g in bufs.items():                            # pure: nothing but gate is written
        assert g.intact()
        a, b = g.body.cpu().numpy(), np.ascontiguousarray(inp[k]).reshape(-1)
        assert np.array_equal(a.view(np.int32) if k == "focus" else a, b.view(np.int32) if k == "focus" else b), k
    return got


@pytest.mark.gpu
def test_gate_decide_hand_cases():
    for name in sorted(HAND):
        inp, rule, g, want = _hand_inputs(name)
        assert _decide(inp, rule, HH, HW, HT).tolist() == [want], name
    for name in sorted(RAGGED):
        inp, rule, want = _ragged_inputs(name)
        assert _decide(inp, rule, HH, HW, 16).tolist() == [want], name


@pytest.mark.gpu
@pytest.mark.parametrize("with_force", [False, True])
@pytest.mark.parametrize("inside_on", [0, 1])
def test_gate_decide_seeded_viewers(with_force, inside_on):
    v = seeded_viewers()
    masks = torch.from_numpy(v["masks"]).cuda()
    stats, _counts = ops.mask_rle(masks)                                                              # the records come from the library itself
    bits = ops.mask_bits(masks)
    assert stats.cpu().tolist() == [RLE.stats(m) for m in v["masks"]]
    assert np.array_equal(bits.cpu().numpy(), np.stack([RLE.bits(m) for m in v["masks"]]))
    inp = dict(sad=v["sad"], gstate=v["gstate"], focus=v["focus"], stats=stats.cpu().numpy(), bits=bits.cpu().numpy(),
               force=v["force"] if with_force else None)
    rule = dict(SEEDED_RULE, inside_on=inside_on)
    want = seeded_reference(v, with_force, inside_on)
    got = _decide(inp, rule, SH, SW, ST)
    assert torch.equal(got, torch.from_numpy(want))
    # the op on the same tensors
    dev = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).cuda() for k in ("sad", "gstate", "focus")}
    out = ops.gate_decide(dev["sad"], dev["gstate"], dev["focus"], stats, bits, (SH, SW), tile=ST,
                          force=torch.from_numpy(v["force"]).cuda() if with_force else None, **rule)
    assert torch.equal(out.cpu(), torch.from_numpy(want))


def _records(rng, rows, H, W, cap, conf):
    P = (W + 31) // 32
    rec = [rng.integers(-2 ** 40, 2 ** 40, (rows,)), rng.integers(-2 ** 40, 2 ** 40, (rows, 6)),
           rng.integers(-2 ** 31, 2 ** 31, (rows, cap)).astype(np.int32), rng.integers(-2 ** 31, 2 ** 31, (rows, H, P)).astype(np.int32)]
    if conf:
        rec.append(rng.random((rows, 3), dtype=np.float32))
    return rec


_REC_TYPES = (torch.int64, torch.int64, torch.int32, torch.int32, torch.float32)


def _commit(img, idx, key, gstate, focus, src, dst, in_place=False, off=False):
    """fs_gate_commit at the C ABI on guarded buffers -> (key, gstate, dst) on the host."""
    B, _, H, W = img.shape
    n = len(idx)
    gi = Guarded(img.size, torch.float32, body=torch.from_numpy(img), off=1 if off else 0)
    gk = Guarded(key.size, torch.uint8, body=torch.from_numpy(key), off=1 if off else 0)
    gs = Guarded(gstate.size, torch.int64, body=torch.from_numpy(gstate))
    gf = Guarded(focus.size, torch.float32, body=torch.from_numpy(focus))
    gd = [Guarded(d.size, dt, body=torch.from_numpy(d)) for d, dt in zip(dst, _REC_TYPES)]
    sd = gd if in_place else [Guarded(max(s.size, 1), dt, body=torch.from_numpy(s) if s.size else None) for s, dt in zip(src, _REC_TYPES)]
    ix = torch.tensor(idx, dtype=torch.int32, device="cuda") if n else None
    sp = [g.ptr for g in sd] + [None] * (5 - len(sd))
    dp = [g.ptr for g in gd] + [None] * (5 - len(gd))
    hip.call("fs_gate_commit", gi.ptr, None if ix is None else ix.data_ptr(), n, gk.ptr, gs.ptr, gf.ptr, *sp, *dp, B, H, W, dst[2].shape[1])
    torch.cuda.synchronize()
    assert gi.intact() and gf.intact() and all(g.intact() for g in sd)
    return (gk.host(*key.shape).numpy(), gs.host(B, 6).numpy(), [g.host(*d.shape).numpy() for g, d in zip(gd, dst)])


@pytest.mark.gpu
@pytest.mark.parametrize("W", [12, 7])
@pytest.mark.parametrize("conf", [False, True])
def test_gate_commit(W, conf):
    B, H, cap = 5, 9, 6
    rng = np.random.default_rng(100 + W + conf)
    img = rng.random((B, 3, H, W), dtype=np.float32) * 1.4 - 0.2
    img[0, 0, 0, 0], img[B - 1, 2, H - 1, W - 1] = np.float32("nan"), np.float32("nan")
    focus = rng.random((B, 2), dtype=np.float32)
    focus[2] = (1.0, 1.0)
    for idx in ([], list(range(B)), [1, 3], [0], [B - 1]):
        key = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)                     # what an untouched viewer must keep
        gstate = rng.integers(0, 1000, (B, 6))
        dst = _records(rng, B, H, W, cap, conf)
        src = _records(rng, len(idx), H, W, cap, conf)
        for off in ((False, True) if W == 12 else (False,)):
            wk, wg, wd = R.commit(img, idx, key, gstate, focus, src, dst)
            gk, gg, gd = _commit(img, idx, key, gstate, focus, src, dst, off=off)
            assert np.array_equal(gk, wk) and np.array_equal(gg, wg)
            for a, b in zip(gd, wd):
                assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)
        if len(idx) == B:                                # src == dst: the records are in place already, the state and the key still move
            wk, wg, _ = R.commit(img, idx, key, gstate, focus, dst, dst)
            gk, gg, gd = _commit(img, idx, key, gstate, focus, dst, dst, in_place=True)
            assert np.array_equal(gk, wk) and np.array_equal(gg, wg)
            for a, b in zip(gd, dst):
                assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)


@pytest.mark.gpu
def test_gate_commit_op_and_the_key_it_makes():
    """ops.gate_commit, and the two kernels together: a frame against the key that commit made from it differs nowhere."""
    B, H, cap = 3, 70, 5
    for W in (45, 72):
        rng = np.random.default_rng(W)
        img = rng.random((B, 3, H, W), dtype=np.float32) * 1.4 - 0.2
        img[rng.random(img.shape) < 0.05] = np.float32("nan")
        img[rng.random(img.shape) < 0.02] = np.float32("inf")
        x = torch.from_numpy(img).cuda()
        key = torch.full((B, 3, H, W), 0x3D, dtype=torch.uint8, device="cuda")
        gstate = torch.zeros(B, 6, dtype=torch.int64, device="cuda")
        focus = torch.from_numpy(rng.random((B, 2), dtype=np.float32)).cuda()
        dst = [torch.from_numpy(a).cuda() for a in _records(rng, B, H, W, cap, True)]
        src = [torch.from_numpy(a).cuda() for a in _records(rng, B, H, W, cap, True)]
        ops.gate_commit(x, torch.arange(B, dtype=torch.int32, device="cuda"), key, gstate, focus, src, dst)
        assert np.array_equal(key.cpu().numpy(), R.q(img).astype(np.uint8))
        for s, d in zip(src, dst):
            assert torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, d.view(torch.int32) if d.dtype == torch.float32 else d)
        assert gstate[:, 0].tolist() == [1] * B and gstate[:, 5].tolist() == [0] * B
        for T in (8, 32):
            assert not bool(ops.gate_tiles(x, key, T).any())
        keep = key.clone()
        ops.gate_commit(x * 0, None, key, gstate, focus, dst, dst)                     # n = 0: only the ages and previous gazes move
        assert torch.equal(key, keep) and gstate[:, 5].tolist() == [1] * B


@pytest.mark.gpu
def test_gate_entry_points_reject_bad_arguments():
    B, H, W, T = 2, 16, 24, 8
    img, key = Guarded(B * 3 * H * W, torch.float32), Guarded(B * 3 * H * W, torch.uint8)
    sad, gate = Guarded(B * 6), Guarded(B * 8, torch.int64)
    gstate, stats = Guarded(B * 6, torch.int64), Guarded(B * 6, torch.int64)
    focus, bits = Guarded(B * 2, torch.float32), Guarded(B * H)
    rec = [Guarded(B, torch.int64), Guarded(B * 6, torch.int64), Guarded(B * 4), Guarded(B * H), Guarded(B * 3, torch.float32)]
    idx = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    outs = [sad, gate, key, gstate] + rec

    def rejected(name, *args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call(name, *args)
        torch.cuda.synchronize()
        s = _GARB
        assert all(g.intact() and bool((g.body == s[g.dtype]).all()) for g in outs), "a rejected call launched something"

    tiles = [img.ptr, key.ptr, sad.ptr, B, H, W, T]
    for i, bad in ((0, None), (1, None), (2, None), (3, 0), (4, 0), (5, -1), (6, 12), (6, 0), (6, 128)):
        a = list(tiles)
        a[i] = bad
        rejected("fs_gate_tiles", *a)
    rejected("fs_gate_tiles", img.ptr, key.ptr, sad.ptr, 1, 65536, 32768, 64)                        # H * W = 2^31
    decide = [sad.ptr, gstate.ptr, focus.ptr, stats.ptr, bits.ptr, None, gate.ptr, B, H, W, T, 1, 2, 0, 0, 4096, 256, 0, 1]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (6, None), (7, 0), (8, 0), (9, 0), (10, 24), (11, 255), (11, -1), (14, -1)):
        a = list(decide)
        a[i] = bad
        rejected("fs_gate_decide", *a)
    ptrs = [g.ptr for g in rec]
    commit = [img.ptr, idx.data_ptr(), 2, key.ptr, gstate.ptr, focus.ptr, *ptrs, *ptrs, B, H, W, 4]
    for i, bad in ((0, None), (1, None), (2, 3), (2, -1), (3, None), (4, None), (5, None), (6, None), (9, None), (11, None), (14, None), (15, None),
                   (16, 0), (17, 0), (18, 0), (19, 0)):
        a = list(commit)
        a[i] = bad
        rejected("fs_gate_commit", *a)


# ------------------------------------------------------------------------------------------------------------------ GPU: session ----
E2E_SEED, SIZE = 11, 256


@pytest.fixture
def served():
    """The hrnet module of tests/test_predict.py in deterministic mode, with the background bias of
    test_predict_instances_equals_predict (the mask plane decides where m > 0), and a counter around _head_parts."""
    import test_predict as TP
    module, _ = TP._module("hrnet")
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    bias = module.decoder.cls_net.fc.bias
    keep = bias.detach().clone()
    with torch.no_grad():
        bias[-1] += 1000.0
    calls = []
    inner = module._head_parts

    def counted(img, focus, seg_size, who):
        calls.append(int(img.shape[0]))
        return inner(img, focus, seg_size, who)
    module._head_parts = counted
    try:
        yield module, calls, TP
    finally:
        del module._head_parts
        with torch.no_grad():
            bias.copy_(keep)
        hip.set_deterministic(was)


def _same(a, b):
    """Two records (tuples of tensors), bit for bit."""
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert s.dtype == t.dtype and s.shape == t.shape
        assert torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)
    return True


def _row(rec, b):
    return tuple(t[b:b + 1].clone() for t in rec)


def _mask_of(bits_row, W):
    return RLE.unbits(bits_row.cpu().numpy(), W)


def _focus_at(Fp, b, py, px):
    f = Fp.clone()
    f[b, 0], f[b, 1] = py / (SIZE - 1), px / (SIZE - 1)
    return f


def _pixel(Fp, b):
    return (R.gaze(float(Fp[b, 0]), SIZE) + 8) >> 4, (R.gaze(float(Fp[b, 1]), SIZE) + 8) >> 4


def _find(mask, want, py, px, lo, hi):
    """A pixel of `mask` with value `want` whose distance from (py, px) lies in (lo, hi) pixels; the nearest to the middle of the ring."""
    y, x = np.mgrid[:mask.shape[0], :mask.shape[1]]
    d = np.hypot(y - py, x - px)
    ok = (mask == want) & (d > lo) & (d < hi)
    assert ok.any(), f"no {'set' if want else 'clear'} pixel between {lo} and {hi} pixels from ({py}, {px})"
    i = int(np.argmin(np.where(ok, np.abs(d - (lo + hi) / 2), np.inf)))
    return i // mask.shape[1], i % mask.shape[1]


def _beside(mask, gap, py, px, far):
    """A clear pixel `gap` pixels beside a set pixel of `mask` (left, right, above or below it), more than `far` pixels from (py, px)."""
    ys, xs = np.nonzero(mask)
    for i in np.argsort(np.abs(ys - mask.shape[0] // 2), kind="stable"):                 # set pixels near the middle rows first
        for dy, dx in ((0, gap), (0, -gap), (gap, 0), (-gap, 0)):
            y, x = int(ys[i]) + dy, int(xs[i]) + dx
            if 0 <= y < mask.shape[0] and 0 <= x < mask.shape[1] and not mask[y, x] and np.hypot(y - py, x - px) > far:
                return y, x
    raise AssertionError("no clear pixel beside the mask")


def _flip_tile(X, b, ty, tx, T=32):
    X = X.clone()
    t = X[b, :, ty * T:(ty + 1) * T, tx * T:(tx + 1) * T]
    t.copy_((t < 0.5).float())                           # every pixel moves by half the range or more
    return X


@pytest.mark.gpu
def test_session_runs_only_when_the_frame_or_the_gaze_asks(served):
    module, calls, TP = served
    H = W = SIZE
    X, Fp = TP._batch(2, SIZE, E2E_SEED)
    X0, F0 = X.clone(), Fp.clone()
    state = {k: v.detach().clone() for k, v in module.state_dict().items()}
    want = module.predict_instances(X, Fp, return_bits=True)
    area = want[1][:, 0].tolist()
    print(f"areas {area}, boxes {want[1][:, 1:5].tolist()}, gaze pixels {[_pixel(Fp, b) for b in range(2)]}")
    assert all(0 < a < H * W for a in area)
    calls.clear()
    s = GazeSession(module, 2, (H, W))

    # 1: the first step makes every record
    *rec, gate = s.step(X, Fp)
    assert gate.dtype == torch.int64 and gate.shape == (2, 8) and not gate.is_cuda
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and calls == [2] and _same(rec, want)
    held = [t.clone() for t in rec]
    # 2: the same frame and gaze again
    *rec, gate = s.step(X, Fp)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and calls == [2] and _same(rec, held)
    assert gate[:, 1:6].tolist() == [[0] * 5] * 2 and gate[:, 7].tolist() == [1, 1]
    # 3: one tile changes outside viewer 1's grown box (and away from its gaze)
    py, px = _pixel(Fp, 1)
    roi = R.roi_tiles(held[1][1].tolist(), py, px, H, W, 32, 16)
    outside = [(ty, tx) for ty in range(8) for tx in range(8) if (ty, tx) not in roi]
    assert outside and len(roi) > 1, "the seed must leave a tile outside the grown box"
    X3 = _flip_tile(X, 1, *outside[0])
    *rec, gate = s.step(X3, Fp)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and gate[1, 1:3].tolist() == [1, 0] and calls == [2] and _same(rec, held)
    # 4: one tile changes inside it
    box_tile = (int(held[1][1, 2]) // 32, int(held[1][1, 1]) // 32)
    assert box_tile in roi
    X4 = _flip_tile(X, 1, *box_tile)
    *rec, gate = s.step(X4, Fp)
    assert gate[:, 0].tolist() == [R.REUSE, R.RUN_ROI] and gate[1, 1:3].tolist() == [1, 1] and calls == [2, 1]
    assert _same(_row(rec, 0), _row(held, 0))
    again = module.predict_instances(X4[1:2], Fp[1:2], return_bits=True)
    assert _same(_row(rec, 1), again)
    calls.clear()
    held = [t.clone() for t in rec]
    # 5: a jump beyond saccade_px, to a clear pixel beside viewer 0's mask: the old record, nothing runs
    py0, px0 = _pixel(Fp, 0)
    P0 = _beside(_mask_of(held[3][0], W), 12, py0, px0, 40)
    F5 = _focus_at(Fp, 0, *P0)
    *rec, gate = s.step(X4, F5)
    assert gate[:, 0].tolist() == [R.HOLD_SACCADE, R.REUSE] and int(gate[0, 5]) > s.saccade2 and calls == [] and _same(rec, held)
    # 6: the gaze has landed there
    *rec, gate = s.step(X4, F5)
    assert gate[:, 0].tolist() == [R.RUN_GAZE, R.REUSE] and int(gate[0, 5]) == 0 and int(gate[0, 6]) == 0 and calls == [1]
    assert _same(_row(rec, 0), module.predict_instances(X4[:1], F5[:1], return_bits=True)) and _same(_row(rec, 1), _row(held, 1))
    calls.clear()
    held = [t.clone() for t in rec]
    # 7: it drifts onto a set pixel of the new mask, further than fixation_px (7.68) and nearer than saccade_px (25.6): the mask keeps the record
    mask0 = _mask_of(held[3][0], W)
    F7 = _focus_at(F5, 0, *_find(mask0, True, *P0, 9, 24))
    *rec, gate = s.step(X4, F7)
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and int(gate[0, 4]) > s.fixation2 and int(gate[0, 6]) == 1 and calls == [] and _same(rec, held)
    *rec, gate = s.step(X4, F5)                          # and back
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and int(gate[0, 4]) == 0
    # 8: to a clear pixel that far away
    F8 = _focus_at(F5, 0, *_find(mask0, False, *P0, 9, 24))
    *rec, gate = s.step(X4, F8)
    assert gate[:, 0].tolist() == [R.RUN_GAZE, R.REUSE] and int(gate[0, 4]) > s.fixation2 and int(gate[0, 6]) == 0 and calls == [1]
    assert _same(_row(rec, 0), module.predict_instances(X4[:1], F8[:1], return_bits=True)) and _same(_row(rec, 1), _row(held, 1))
    calls.clear()
    held = [t.clone() for t in rec]
    Fg = F8                                              # where the gaze rests for the remaining steps
    # 9: force and reset
    *rec, gate = s.step(X4, Fg, force=[0, 1])
    assert gate[:, 0].tolist() == [R.REUSE, R.RUN_FORCED] and calls == [1] and _same(rec, held)        # the same frame: the same record
    *rec, gate = s.step(X4, Fg, force=torch.tensor([False, False]))
    assert gate[:, 0].tolist() == [R.REUSE] * 2 and calls == [1]
    s.reset([0])
    *rec, gate = s.step(X4, Fg)
    assert gate[:, 0].tolist() == [R.RUN_INIT, R.REUSE] and calls == [1, 1] and _same(rec, held)
    s.reset()
    *rec, gate = s.step(X4, Fg)
    assert gate[:, 0].tolist() == [R.RUN_INIT] * 2 and calls == [1, 1, 2]
    assert _same(rec, module.predict_instances(X4, Fg, return_bits=True))
    assert s.counts == {0: 16, 1: 5, 2: 1, 3: 0, 4: 1, 5: 2, 6: 0, 7: 1} and sum(s.counts.values()) == 2 * 13
    # 10: nothing written into an argument or the module
    module.check_nan()
    assert torch.equal(X, X0) and torch.equal(Fp, F0)
    for k, v in module.state_dict().items():
        assert torch.equal(v, state[k]), k


@pytest.mark.gpu
def test_session_single_viewer_score_age_and_memory(served):
    module, calls, TP = served
    H = W = SIZE
    X, Fp = TP._batch(1, SIZE, E2E_SEED)
    want = module.predict_instances(X, Fp, return_bits=True, return_score=True)
    assert 0 < int(want[1][0, 0]) < H * W
    calls.clear()
    s = GazeSession(module, 1, (H, W), score=True, max_age=2)
    out = s.step(X, Fp)
    assert len(out) == 6 and out[5][:, 0].tolist() == [R.RUN_INIT] and _same(out[:5], want) and out[4].shape == (1, 3)
    held = [t.clone() for t in out[:5]]
    *rec, gate = s.step(X, Fp)
    assert gate[:, 0].tolist() == [R.REUSE] and int(gate[0, 7]) == 1 and _same(rec, held)
    # a REUSE step allocates nothing of the frame's size
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    *rec, gate = s.step(X, Fp)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"a REUSE step raised the peak by {grew} bytes")
    assert gate[:, 0].tolist() == [R.REUSE] and int(gate[0, 7]) == 2 and grew < H * W and calls == [1] and _same(rec, held)
    *rec, gate = s.step(X, Fp)                           # the third step after the record was made: age + 1 = 3 > max_age = 2
    assert gate[:, 0].tolist() == [R.RUN_AGE] and int(gate[0, 7]) == 3 and calls == [1, 1] and _same(rec, held)
    *rec, gate = s.step(X, Fp)
    assert gate[:, 0].tolist() == [R.REUSE] and int(gate[0, 7]) == 1
    # max_runs reaches predict_instances
    s2 = GazeSession(module, 1, (H, W), max_runs=5)
    cat, stats, counts, bits, gate = s2.step(X, Fp)
    assert counts.shape == (1, 5) and torch.equal(counts, want[2][:, :5]) and torch.equal(stats, want[1])
    module.train()
    try:
        with pytest.raises(RuntimeError):
            s2.step(X, Fp)
    finally:
        module.eval()
