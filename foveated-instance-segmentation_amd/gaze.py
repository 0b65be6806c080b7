"""The passes of GazeSession (csrc/gaze_gate.hip, csrc/gaze_motion.hip): gate tiles / decide / commit, frame profiles, the motion
estimate and the state shift, with their argument checks.  Stateless, no autograd.
"""
import operator

import torch

from . import hip
from .frames import _FRAME_TYPES, _frame_args, _frame_route

__all__ = [
    "GATE_TILES", "GATE_CODES", "GATE_RUNS", "gate_tiles", "gate_tiles_u8", "gate_decide", "gate_commit", "gate_commit_u8",
    "MOTION_MAX_PX", "frame_profiles", "key_profiles", "profile_shift", "state_shift_scratch", "state_shift", "state_shift_u8",
    "motion_commit",
]


GATE_TILES = (8, 16, 32, 64)
GATE_CODES = {0: "REUSE", 1: "RUN_INIT", 2: "HOLD_SACCADE", 3: "RUN_SCENE", 4: "RUN_ROI", 5: "RUN_GAZE", 6: "RUN_AGE", 7: "RUN_FORCED"}
GATE_RUNS = (1, 3, 4, 5, 6, 7)                      # the codes after which the network runs


def _gate_tile(T):
    if isinstance(T, bool) or int(T) != T or int(T) not in GATE_TILES:
        raise ValueError(f"the tile side must be one of {GATE_TILES}, got {T!r}")
    return int(T)


def _gate_tiles(dtype, img, key, tile, out):
    T = _gate_tile(tile)
    what = "fp32" if dtype == torch.float32 else "uint8"
    if not isinstance(img, _FRAME_TYPES) or img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0 or img.dtype != dtype:
        raise ValueError(f"img must be a non-empty {what} (B,3,H,W), got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))}")
    if key.dtype != torch.uint8 or key.shape != img.shape:
        raise ValueError(f"key must be uint8 {tuple(img.shape)}, got {key.dtype} {tuple(key.shape)}")
    B, _, H, W = (int(v) for v in img.shape)
    suffix, strides = _frame_route(img)
    shape = (B, (H + T - 1) // T, (W + T - 1) // T)
    if out is None:
        out = torch.empty(shape, device=img.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or tuple(out.shape) != shape:
        raise ValueError(f"out must be int32 {shape}, got {out.dtype} {tuple(out.shape)}")
    hip.call("fs_gate_tiles" + suffix, *_frame_args(img, strides), hip.ptr(key), hip.ptr(out), B, H, W, T)
    return out


def gate_tiles(img, key, tile=32, out=None):
    """How much every tile of new frames differs from the 8-bit key frames (fs_gate_tiles; no autograd; unpinned: the reference has
    no counterpart).  img (B,3,H,W) fp32, key (B,3,H,W) uint8 = q of the frames the records were made from, q(v) = rint(clamp(v, 0, 1) *
    255) in fp32, NaN -> 0.  Returns sad (B,th,tw) int32, th = ceil(H / tile), tw = ceil(W / tile): the sum of |q(img) - key| over the
    three channels and the tile's pixels (the last tiles are ragged).  out: a (B,th,tw) int32 tensor to write into."""
    return _gate_tiles(torch.float32, img, key, tile, out)


def gate_tiles_u8(img, key, tile=32, out=None):
    """gate_tiles for frames of bytes (fs_gate_tiles_u8): img (B,3,H,W) uint8, the pixel value byte / 255, whose code q is the byte.  sad
    is the sum of |img - key|, equal to gate_tiles(img.float() / 255, key, tile); 6 bytes read a pixel instead of 15.  img is contiguous,
    or an hwc view of interleaved bytes (byte_frame_layout; fs_gate_tiles_hwc), read where it lies; ValueError for any other layout."""
    return _gate_tiles(torch.uint8, img, key, tile, out)


def gate_decide(sad, gstate, focus, stats, bits, frame_size, tile=32, level=8, scene_tiles=0, roi_tiles=0, margin=16,
                saccade2=2 ** 62, fixation2=0, max_age=0, inside_on=True, force=None, out=None):
    """The gate's decision per viewer (fs_gate_decide; no autograd; unpinned).  sad (B,th,tw) int32 as gate_tiles returns it; gstate
    (B,6) int64 = (valid, gy_key, gx_key, gy_prev, gx_prev, age), gazes in 1/16-pixel units; focus (B,2) fp32 normalised (row, col);
    stats (B,6) int64 and bits (B,H,ceil(W/32)) int32 the records' (mask_rle, mask_bits); force (B,) int32 or None; frame_size = (H, W).
    saccade2 and fixation2 are squared distances in 1/16-pixel units, floor((px * 16) ** 2).  Returns gate (B,8) int64 = (code,
    n_changed, n_roi_changed, sad_total, d2_key, d2_prev, inside_bit, age + 1); the codes are GATE_CODES, the first rule that holds in
    the order 7, 1, 2, 3, 4, 5, 6, 0 (include/fovealseg.h).  Nothing but gate is written."""
    T = _gate_tile(tile)
    H, W = int(frame_size[0]), int(frame_size[1])
    B = int(sad.shape[0])
    if sad.dtype != torch.int32 or tuple(sad.shape) != (B, (H + T - 1) // T, (W + T - 1) // T):
        raise ValueError(f"sad must be int32 (B, ceil(H/T), ceil(W/T)) for H, W, T = {H}, {W}, {T}, got {sad.dtype} {tuple(sad.shape)}")
    if gstate.dtype != torch.int64 or tuple(gstate.shape) != (B, 6) or stats.dtype != torch.int64 or tuple(stats.shape) != (B, 6):
        raise ValueError(f"gstate and stats must be int64 ({B}, 6), got {tuple(gstate.shape)} and {tuple(stats.shape)}")
    if focus.dtype != torch.float32 or tuple(focus.shape) != (B, 2):
        raise ValueError(f"focus must be fp32 ({B}, 2), got {focus.dtype} {tuple(focus.shape)}")
    if bits.dtype != torch.int32 or tuple(bits.shape) != (B, H, (W + 31) // 32):
        raise ValueError(f"bits must be int32 {(B, H, (W + 31) // 32)}, got {bits.dtype} {tuple(bits.shape)}")
    if force is not None and (force.dtype != torch.int32 or tuple(force.shape) != (B,)):
        raise ValueError(f"force must be int32 ({B},), got {force.dtype} {tuple(force.shape)}")
    if isinstance(level, bool) or int(level) != level or not 0 <= int(level) <= 254:
        raise ValueError(f"level must be an integer 0 .. 254, got {level!r}")
    if int(margin) < 0:
        raise ValueError(f"margin must be >= 0, got {margin!r}")
    if out is None:
        out = torch.empty(B, 8, device=sad.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, 8):
        raise ValueError(f"out must be int64 ({B}, 8), got {out.dtype} {tuple(out.shape)}")
    hip.call("fs_gate_decide", hip.ptr(sad), hip.ptr(gstate), hip.ptr(focus), hip.ptr(stats), hip.ptr(bits), hip.ptr(force), hip.ptr(out),
             B, H, W, T, int(level), int(scene_tiles), int(roi_tiles), int(margin), int(saccade2), int(fixation2), int(max_age),
             1 if inside_on else 0)
    return out


def _gate_commit(dtype, img, idx, key, gstate, focus, src, dst):
    what = "fp32" if dtype == torch.float32 else "uint8"
    if (not isinstance(img, _FRAME_TYPES) or img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0 or img.dtype != dtype
            or key.dtype != torch.uint8 or key.shape != img.shape):
        raise ValueError(f"img must be a non-empty {what} (B,3,H,W) and key uint8 of its shape, got {getattr(img, 'dtype', None)} "
                         f"{tuple(getattr(img, 'shape', ()))} and {tuple(key.shape)}")
    B, _, H, W = (int(v) for v in img.shape)
    suffix, strides = _frame_route(img)
    n = 0 if idx is None else int(idx.shape[0])
    if idx is not None and (idx.dtype != torch.int32 or idx.dim() != 1 or n > B):
        raise ValueError(f"idx must be int32 (n,) with n <= {B}, got {idx.dtype} {tuple(idx.shape)}")
    if gstate.dtype != torch.int64 or tuple(gstate.shape) != (B, 6) or focus.dtype != torch.float32 or tuple(focus.shape) != (B, 2):
        raise ValueError(f"gstate must be int64 ({B}, 6) and focus fp32 ({B}, 2), got {tuple(gstate.shape)} and {tuple(focus.shape)}")
    if len(src) != len(dst) or len(dst) not in (4, 5):
        raise ValueError("src and dst must both be (cat, stats, counts, bits) or (cat, stats, counts, bits, conf)")
    cap = int(dst[2].shape[1])
    tails = ((), (6,), (cap,), (H, (W + 31) // 32), (3,))
    dtypes = (torch.int64, torch.int64, torch.int32, torch.int32, torch.float32)
    for s, d, tail, dt in zip(src, dst, tails, dtypes):
        if d.dtype != dt or tuple(d.shape) != (B,) + tail:
            raise ValueError(f"a dst record tensor must be {dt} {(B,) + tail}, got {d.dtype} {tuple(d.shape)}")
        if s is not d and n > 0 and (s.dtype != dt or tuple(s.shape) != (n,) + tail):
            raise ValueError(f"a src record tensor must be {dt} {(n,) + tail}, got {s.dtype} {tuple(s.shape)}")
    sp = [hip.ptr(s) for s in src] + [None] * (5 - len(src))
    dp = [hip.ptr(d) for d in dst] + [None] * (5 - len(dst))
    hip.call("fs_gate_commit" + suffix, *_frame_args(img, strides), hip.ptr(idx), n, hip.ptr(key), hip.ptr(gstate), hip.ptr(focus), *sp, *dp,
             B, H, W, cap)


def gate_commit(img, idx, key, gstate, focus, src, dst):
    """What a step leaves behind (fs_gate_commit; no autograd; unpinned), in place.  idx (n,) int32 ascending, or None for n = 0: the
    viewers whose record was made anew from img (B,3,H,W) fp32.  src = (cat, stats, counts, bits[, conf]) with n rows, dst the same
    with B rows: row j moves to row idx[j]; a pair that is one tensor is already in place.  For the viewers of idx key (B,3,H,W) uint8
    <- q(img), g_key <- g, age <- 0, valid <- 1 in gstate (B,6) int64; for every viewer g_prev <- g; any other viewer's age grows by
    one.  With n = 0 src is not read (pass dst)."""
    _gate_commit(torch.float32, img, idx, key, gstate, focus, src, dst)


def gate_commit_u8(img, idx, key, gstate, focus, src, dst):
    """gate_commit for frames of bytes (fs_gate_commit_u8): img (B,3,H,W) uint8; for the viewers of idx key <- img, a copy.  Everything
    else as gate_commit, and equal to it on img.float() / 255.  img is contiguous, or an hwc view of interleaved bytes (byte_frame_layout;
    fs_gate_commit_hwc: the key takes the de-interleaved frame and stays planar); ValueError for any other layout."""
    _gate_commit(torch.uint8, img, idx, key, gstate, focus, src, dst)


MOTION_MAX_PX = 255                                 # fs_profile_shift's largest search range


def _index_or_none(v):
    """v as an int where it is an integer of any integer type (no bool, no float), else None."""
    if isinstance(v, bool):
        return None
    try:
        return operator.index(v)
    except TypeError:
        return None


def _motion_px(motion_px, H, W):
    """The search range R of the motion estimate: an integer 1 .. 255 with 4 R < min(H, W)."""
    R = _index_or_none(motion_px)
    if R is None or not 1 <= R <= MOTION_MAX_PX or 4 * R >= min(int(H), int(W)):
        raise ValueError(f"motion_px must be an integer 1 .. {MOTION_MAX_PX} with 4 * motion_px < min(H, W) = {min(int(H), int(W))}, got {motion_px!r}")
    if 8 * max(int(H), int(W)) + 8 * (2 * R + 1) > 65536:
        raise ValueError(f"a side of {max(int(H), int(W))} pixels with motion_px = {R} is beyond the estimate's 64 KiB of LDS")
    return R


def _motion_gain(gain):
    g = _index_or_none(gain)
    if g is None or not 0 <= g <= 8:
        raise ValueError(f"motion_gain must be an integer 0 .. 8, got {gain!r}")
    return g


def _profile_sizes(B, H, W):
    if 765 * max(H, W) >= 2 ** 31 or H * W >= 2 ** 31:
        raise ValueError(f"a frame of {H} x {W} pixels is beyond int32 profiles")
    return (B, H + W)


# the profile pass's entry point by _frame_route's suffix: fs_frame_profiles + suffix ("_nv12" among them), but a planar frame of bytes is a key
_PROFILE_ENTRY = {"": "fs_frame_profiles", "_u8": "fs_key_profiles", "_hwc": "fs_frame_profiles_hwc"}


def _profiles(src, dtype, out):
    if not isinstance(src, _FRAME_TYPES) or src.dim() != 4 or src.shape[1] != 3 or src.numel() == 0 or src.dtype != dtype:
        raise ValueError(f"the frames must be a non-empty {dtype} (B,3,H,W), got {getattr(src, 'dtype', None)} {tuple(getattr(src, 'shape', ()))}")
    B, _, H, W = (int(v) for v in src.shape)
    suffix, strides = _frame_route(src, "the frames")
    shape = _profile_sizes(B, H, W)
    if out is None:
        out = torch.empty(shape, device=src.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or tuple(out.shape) != shape:
        raise ValueError(f"out must be int32 {shape}, got {out.dtype} {tuple(out.shape)}")
    hip.call(_PROFILE_ENTRY.get(suffix, "fs_frame_profiles" + suffix), *_frame_args(src, strides), hip.ptr(out), B, H, W)
    return out


def frame_profiles(img, out=None):
    """The integral projections of frames (fs_frame_profiles; no autograd; unpinned: the reference has no counterpart).  img (B,3,H,W)
    fp32.  Returns prof (B, H + W) int32: prof[b, :H] = the row sums and prof[b, H:] = the column sums of the luma code L = q_r + q_g +
    q_b, q the gate's pixel code (gate_tiles).  out: a (B, H + W) int32 tensor to write into."""
    return _profiles(img, torch.float32, out)


def key_profiles(key, out=None):
    """frame_profiles of 8-bit key frames (fs_key_profiles): key (B,3,H,W) uint8.  The profiles of a frame and of the key gate_commit
    made from it are equal.  A frame of bytes may also be an hwc view of interleaved bytes (byte_frame_layout; fs_frame_profiles_hwc), read
    where it lies; ValueError for any other non-contiguous layout."""
    return _profiles(key, torch.uint8, out)


def profile_shift(prof, prof_key, gstate, frame_size, motion_px, motion_gain=6, out=None):
    """The integer translation of every viewer against its key frame (fs_profile_shift; no autograd; unpinned).  prof, prof_key (B, H +
    W) int32 as frame_profiles / key_profiles make them; gstate (B,6) int64 the gate's; frame_size = (H, W); motion_px = R, the search
    range.  Per axis cost(s) = sum_{i=R}^{n-1-R} |P[i] - K[i - s]|; the least cost wins, ties to the smaller |s|, then to the negative s,
    and the shift is taken only if cost(s) * 8 <= cost(0) * motion_gain.  Returns shift (B,4) int64 = (dy, dx, cost_best, cost_zero),
    all 0 for a viewer without a record."""
    H, W = int(frame_size[0]), int(frame_size[1])
    R, gain = _motion_px(motion_px, H, W), _motion_gain(motion_gain)
    if not isinstance(prof, torch.Tensor) or prof.dim() != 2 or prof.dtype != torch.int32 or prof.shape[1] != H + W or prof.shape[0] < 1:
        raise ValueError(f"prof must be int32 (B, H + W) = (B, {H + W}), got {getattr(prof, 'dtype', None)} {tuple(getattr(prof, 'shape', ()))}")
    B = int(prof.shape[0])
    _profile_sizes(B, H, W)
    if prof_key.dtype != torch.int32 or prof_key.shape != prof.shape:
        raise ValueError(f"prof_key must be int32 {tuple(prof.shape)}, got {prof_key.dtype} {tuple(prof_key.shape)}")
    if gstate.dtype != torch.int64 or tuple(gstate.shape) != (B, 6):
        raise ValueError(f"gstate must be int64 ({B}, 6), got {gstate.dtype} {tuple(gstate.shape)}")
    if out is None:
        out = torch.empty(B, 4, device=prof.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (B, 4):
        raise ValueError(f"out must be int64 ({B}, 4), got {out.dtype} {tuple(out.shape)}")
    hip.call("fs_profile_shift", hip.ptr(prof), hip.ptr(prof_key), hip.ptr(gstate), hip.ptr(out), B, H, W, R, gain)
    return out


def state_shift_scratch(B, H, W, cap, device):
    """The scratch tensor state_shift wants for these sizes (fs_state_shift_scratch_ints ints)."""
    return torch.empty(hip.query("fs_state_shift_scratch_ints", int(B), int(H), int(W), int(cap)), device=device, dtype=torch.int32)


def _state_shift(dtype, img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch):
    if not isinstance(img, _FRAME_TYPES) or img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0 or img.dtype != dtype:
        raise ValueError(f"img must be a non-empty {'fp32' if dtype == torch.float32 else 'uint8'} (B,3,H,W), got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))}")
    B, _, H, W = (int(v) for v in img.shape)
    suffix, strides = _frame_route(img)
    _profile_sizes(B, H, W)
    P = (W + 31) // 32
    for name, k in (("key", key), ("key2", key2)):
        if k.dtype != torch.uint8 or k.shape != img.shape:
            raise ValueError(f"{name} must be uint8 {tuple(img.shape)}, got {k.dtype} {tuple(k.shape)}")
    for name, w in (("bits", bits), ("bits2", bits2)):
        if w.dtype != torch.int32 or tuple(w.shape) != (B, H, P):
            raise ValueError(f"{name} must be int32 {(B, H, P)}, got {w.dtype} {tuple(w.shape)}")
    if key2.data_ptr() == key.data_ptr() or bits2.data_ptr() == bits.data_ptr():
        raise ValueError("key2 and bits2 must be buffers of their own: the move does not read what it writes")
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[0] != B or counts.shape[1] < 1:
        raise ValueError(f"counts must be int32 ({B}, cap), got {counts.dtype} {tuple(counts.shape)}")
    cap = int(counts.shape[1])
    for name, t, tail in (("shift", shift, (4,)), ("gstate", gstate, (6,)), ("stats", stats, (6,)), ("mstate", mstate, (4,))):
        if t.dtype != torch.int64 or tuple(t.shape) != (B,) + tail:
            raise ValueError(f"{name} must be int64 {(B,) + tail}, got {t.dtype} {tuple(t.shape)}")
    if prof_key.dtype != torch.int32 or tuple(prof_key.shape) != (B, H + W):
        raise ValueError(f"prof_key must be int32 {(B, H + W)}, got {prof_key.dtype} {tuple(prof_key.shape)}")
    if motion is None:
        motion = torch.empty(B, 6, device=img.device, dtype=torch.int64)
    elif motion.dtype != torch.int64 or tuple(motion.shape) != (B, 6):
        raise ValueError(f"motion must be int64 ({B}, 6), got {motion.dtype} {tuple(motion.shape)}")
    need = hip.query("fs_state_shift_scratch_ints", B, H, W, cap)
    if scratch is None:
        scratch = torch.empty(need, device=img.device, dtype=torch.int32)
    elif scratch.dtype != torch.int32 or scratch.dim() != 1 or scratch.numel() < need:
        raise ValueError(f"scratch must be int32 with at least {need} entries, got {scratch.dtype} {tuple(scratch.shape)}")
    hip.call("fs_state_shift" + suffix, *_frame_args(img, strides), hip.ptr(shift), hip.ptr(key), hip.ptr(key2), hip.ptr(bits), hip.ptr(bits2), hip.ptr(gstate),
             hip.ptr(stats), hip.ptr(counts), hip.ptr(prof_key), hip.ptr(mstate), hip.ptr(motion), hip.ptr(scratch), B, H, W, cap)
    return motion


def state_shift(img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion=None, scratch=None):
    """Move the state of every viewer whose shift is not (0, 0), in place (fs_state_shift; no autograd; unpinned).  img (B,3,H,W) fp32
    the new frames; shift (B,4) int64 as profile_shift returns it; key (B,3,H,W) uint8 and bits (B,H,ceil(W/32)) int32 are moved by (dy,
    dx) -- the key's uncovered border is filled with q(img), the mask's with 0 -- through the spare buffers key2 and bits2 of the same
    shapes, whose contents afterwards are unspecified; the four gaze coordinates of gstate (B,6) int64 move by 16 * d, clamped; stats
    (B,6) int64 and counts (B,cap) int32 become mask_rle's of the moved bits; prof_key (B, H + W) int32 becomes key_profiles of the
    moved key; mstate (B,4) int64 = (dy_total, dx_total, moves, path) grows.  A still viewer's rows are not written.  Returns motion
    (B,6) int64 = (dy, dx, cost_best, cost_zero, dy_total, dx_total), written for every viewer.  scratch: state_shift_scratch(...)."""
    return _state_shift(torch.float32, img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch)


def state_shift_u8(img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion=None, scratch=None):
    """state_shift for frames of bytes (fs_state_shift_u8): img (B,3,H,W) uint8; the key's uncovered border is filled with the frame's
    byte.  Everything else as state_shift, and equal to it on img.float() / 255; the scratch is the same.  img is contiguous, or an hwc
    view of interleaved bytes (byte_frame_layout; fs_state_shift_hwc); ValueError for any other layout."""
    return _state_shift(torch.uint8, img, shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch)


def motion_commit(idx, prof, prof_key, mstate, frame_size):
    """What a step leaves behind for the motion estimate (fs_motion_commit; no autograd; unpinned), in place, after gate_commit: for the
    viewers of idx (int32 (n,) ascending, or None) prof_key (B, H + W) int32 <- prof, this step's frame_profiles, and mstate (B,4) int64
    <- 0.  frame_size = (H, W)."""
    H, W = int(frame_size[0]), int(frame_size[1])
    if not isinstance(prof, torch.Tensor) or prof.dim() != 2 or prof.dtype != torch.int32 or prof.shape[1] != H + W or prof.shape[0] < 1:
        raise ValueError(f"prof must be int32 (B, H + W) = (B, {H + W}), got {getattr(prof, 'dtype', None)} {tuple(getattr(prof, 'shape', ()))}")
    B = int(prof.shape[0])
    _profile_sizes(B, H, W)
    n = 0 if idx is None else int(idx.shape[0])
    if idx is not None and (idx.dtype != torch.int32 or idx.dim() != 1 or n > B):
        raise ValueError(f"idx must be int32 (n,) with n <= {B}, got {idx.dtype} {tuple(idx.shape)}")
    if prof_key.dtype != torch.int32 or prof_key.shape != prof.shape:
        raise ValueError(f"prof_key must be int32 {tuple(prof.shape)}, got {prof_key.dtype} {tuple(prof_key.shape)}")
    if mstate.dtype != torch.int64 or tuple(mstate.shape) != (B, 4):
        raise ValueError(f"mstate must be int64 ({B}, 4), got {mstate.dtype} {tuple(mstate.shape)}")
    if n:
        hip.call("fs_motion_commit", hip.ptr(idx), n, hip.ptr(prof), hip.ptr(prof_key), hip.ptr(mstate), B, H, W)
