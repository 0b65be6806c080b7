"""GazeSession: the gazed instance for a stream of frames, re-made only when the frame or the gaze asks for it.

`predict_instances` answers "which instance is the viewer looking at" for one frame.  On a stream most consecutive frames show the
same instance under the same fixation, and the record the caller holds is still right.  A session keeps, per viewer, the last record
and an 8-bit copy of the frame it was made from; every step it measures on the device how much the new frame differs from that key
frame per tile, looks at where the gaze went, and runs the network only for the viewers whose record no longer holds (ops.gate_tiles,
gate_decide, gate_commit: csrc/gaze_gate.hip).  The definition is this library's own -- the reference has no temporal logic -- and is
all integers (include/fovealseg.h).
"""
import math

import torch

from . import frames, gaze, masks, ops, overlay

OFF2 = 2 ** 62                                      # a squared distance no gaze reaches: the saccade rule switched off
_DEFAULT = object()                                 # saccade_px not given (None means "off")


def px_to_thr2(px):
    """A distance in pixels as the squared threshold the gate compares with, in 1/16-pixel units: floor((px * 16) ** 2)."""
    px = float(px)
    if not (px >= 0.0) or math.isinf(px):
        raise ValueError(f"a gaze distance must be a finite number of pixels >= 0, got {px!r}")
    return OFF2 if px >= 2.0 ** 27 else int(math.floor((px * 16.0) ** 2))


def _int_ge(name, v, lo):
    if isinstance(v, bool) or int(v) != v or int(v) < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


class GazeSession:
    """A per-viewer stream state around `module.predict_instances`.

    module: a DeformSegmentationModule in eval mode; batch: the number of viewers B; frame_size = (H, W) of every frame.  The record
    is always at the frame's size.

    tile (32): tile side T, one of 8, 16, 32, 64.  level (8): a tile is changed when its mean absolute difference to the key frame
    exceeds `level` grey levels of 255 (sad > level * 3 * pixels).  scene_frac (0.25): more than floor(scene_frac * tiles) changed
    tiles re-make the record (a cut, a head turn).  roi_tiles (0): changed tiles tolerated inside the region of interest -- the
    record's box grown by roi_margin (16) pixels, plus the tile under the gaze.  fixation_px (0.03 * min(H, W)): gaze drift tolerated
    around the gaze the record was made for.  saccade_px (0.10 * min(H, W)): a jump this long since the last step counts as a saccade
    in flight: the old record is kept and nothing runs; None switches the rule off.  max_age (0): steps after which a record is
    re-made whatever else holds; 0 = never.  reuse_inside_mask (True): a gaze that still lies on the record's mask keeps the record
    however far it has drifted.  max_runs (None): as predict_instances.  score (False): also keep conf.  component (None, 4 or 8)
    and snap_px (None): as predict_instances -- the record is the connected component under the gaze.  The gate needs no change for
    it: its box, the region of interest grown from it and the inside bit are read from the record's stats and bits, so they follow the
    component; a gaze that lands on another blob the head also marked is then outside the record's mask and re-makes it (RUN_GAZE).

    motion_px (None): an integer R >= 1 switches global motion compensation on, for a camera that translates (a head-mounted one):
    before the gate looks, every step estimates an integer shift (dy, dx) in [-R, R]^2 per viewer from the integral projections of the
    new frame against the key frame's (ops.frame_profiles, profile_shift) and moves the viewer's state by it -- key frame, mask, key
    and previous gaze, stats / counts re-encoded (ops.state_shift).  The unchanged gate then verifies the move: a wrong estimate shows
    as changed tiles and the record is re-made as before.  cat and conf are not touched: mask_prob keeps describing the pixels the
    record was made from.  motion_gain (6), an integer 0 .. 8: a shift is taken only if its cost is at most motion_gain / 8 of the
    cost of standing still.  Needs 4 * R < min(H, W), R <= 255, and a second key buffer: 3 * H * W bytes a viewer more (201 MB at B =
    64, 1024 x 1024).  With motion_px the step returns one more element, motion.

    These defaults are this library's choices.  They have not been validated on real gaze data: tune them on recordings of the
    headset and scenes you serve.

    step(img, focus, force=None) returns (cat, stats, counts, bits[, conf], gate[, motion]).  `counts` (the attribute) is a dict,
    decision code -> number of viewer-steps so far (ops.GATE_CODES names the codes)."""

    def __init__(self, module, batch, frame_size, *, tile=32, level=8, scene_frac=0.25, roi_tiles=0, roi_margin=16, fixation_px=None,
                 saccade_px=_DEFAULT, max_age=0, reuse_inside_mask=True, max_runs=None, score=False, component=None, snap_px=None,
                 motion_px=None, motion_gain=6):
        self.module = module
        self.batch = _int_ge("batch", batch, 1)
        if len(frame_size) != 2:
            raise ValueError(f"frame_size must be (H, W), got {frame_size!r}")
        self.H, self.W = _int_ge("frame height", frame_size[0], 1), _int_ge("frame width", frame_size[1], 1)
        if self.H * self.W >= 2 ** 31 or max(self.H, self.W) > 2 ** 26:
            raise ValueError(f"a frame of {self.H} x {self.W} pixels is beyond 32-bit pixel indices")
        self.tile = gaze._gate_tile(tile)
        self.level = _int_ge("level", level, 0)
        if self.level > 254:
            raise ValueError(f"level must be an integer 0 .. 254, got {level!r}")
        self.th, self.tw = (self.H + self.tile - 1) // self.tile, (self.W + self.tile - 1) // self.tile
        frac = float(scene_frac)
        if not (frac >= 0.0) or math.isinf(frac):
            raise ValueError(f"scene_frac must be a finite number >= 0, got {scene_frac!r}")
        self.scene_tiles = min(int(math.floor(frac * self.th * self.tw)), 2 ** 31 - 1)
        self.roi_tiles = _int_ge("roi_tiles", roi_tiles, 0)
        self.roi_margin = _int_ge("roi_margin", roi_margin, 0)
        side = min(self.H, self.W)
        self.fixation2 = px_to_thr2(0.03 * side if fixation_px is None else fixation_px)
        if saccade_px is None:
            self.saccade2 = OFF2
        else:
            self.saccade2 = px_to_thr2(0.10 * side if saccade_px is _DEFAULT else saccade_px)
        self.max_age = _int_ge("max_age", max_age, 0)
        self.inside_on = bool(reuse_inside_mask)
        self.cap = masks._max_runs(max_runs, self.W)
        self.max_runs = max_runs
        self.score = bool(score)
        if component is None:
            if snap_px is not None:
                raise ValueError("snap_px goes with component = 4 or 8")
        else:
            masks._component_args(component, snap_px)
        self.component, self.snap_px = component, snap_px
        self.motion_gain = gaze._motion_gain(motion_gain)
        self.motion_px = None if motion_px is None else gaze._motion_px(motion_px, self.H, self.W)
        self.counts = {code: 0 for code in sorted(ops.GATE_CODES)}
        self._dev = None

    # ---- state on the device, made at the first step ---------------------------------------------------------------------------
    def _allocate(self, dev):
        B, H, W = self.batch, self.H, self.W
        self._dev = dev
        self._key = torch.zeros(B, 3, H, W, device=dev, dtype=torch.uint8)
        self._sad = torch.zeros(B, self.th, self.tw, device=dev, dtype=torch.int32)
        self._gstate = torch.zeros(B, 6, device=dev, dtype=torch.int64)
        self._gate = torch.zeros(B, 8, device=dev, dtype=torch.int64)
        self._gate_host = torch.zeros(B, 8, dtype=torch.int64).pin_memory()
        rec = [torch.zeros(B, device=dev, dtype=torch.int64), torch.zeros(B, 6, device=dev, dtype=torch.int64),
               torch.zeros(B, self.cap, device=dev, dtype=torch.int32), torch.zeros(B, H, (W + 31) // 32, device=dev, dtype=torch.int32)]
        if self.score:
            rec.append(torch.zeros(B, 3, device=dev, dtype=torch.float32))
        self._rec = rec
        if self.motion_px is not None:
            self._key2 = torch.zeros_like(self._key)
            self._bits2 = torch.zeros_like(rec[3])
            self._prof = torch.zeros(B, H + W, device=dev, dtype=torch.int32)
            self._prof_key = torch.zeros(B, H + W, device=dev, dtype=torch.int32)       # the profiles of the all-zero key
            self._shift = torch.zeros(B, 4, device=dev, dtype=torch.int64)
            self._mstate = torch.zeros(B, 4, device=dev, dtype=torch.int64)
            self._motion = torch.zeros(B, 6, device=dev, dtype=torch.int64)
            self._motion_host = torch.zeros(B, 6, dtype=torch.int64).pin_memory()
            self._scratch = ops.state_shift_scratch(B, H, W, self.cap, dev)

    def reset(self, viewers=None):
        """Forget the records of `viewers` (a sequence of viewer indices; None = all): their next step is RUN_INIT."""
        if viewers is not None:
            viewers = [int(v) for v in viewers]
            if any(not 0 <= v < self.batch for v in viewers):
                raise ValueError(f"viewers must lie in 0 .. {self.batch - 1}, got {viewers!r}")
        if self._dev is None:
            return
        if viewers is None:
            self._gstate[:, 0].zero_()
        elif viewers:
            self._gstate[torch.tensor(viewers, device=self._dev), 0] = 0

    @torch.no_grad()
    def render(self, img, focus=None, style=None, outline_px=0, out=None):
        """Every viewer's current record drawn onto img, in one launch (ops.draw_instances; unpinned).  img (B,3,H,W) as step() takes it --
        fp32, uint8, or a uint8 view of interleaved bytes, read where it lies -- usually the frame just stepped.  The session's bits and
        stats are drawn as they stand after the last step, any motion_px move included; a viewer without a record (before its first step,
        after reset()) is drawn empty: column 0 of the gate's state is the kernel's live flag, read on the device.  focus (B,2) adds the
        gaze marker of the style; style is ops.overlay_style's table (None: its defaults); outline_px = d > 0 outlines the mask with the
        band bits & ~E_d(bits).  out: a uint8 (B,3,H,W) tensor, contiguous or an interleaved view (ops.byte_frame_dest), img itself for a
        frame of bytes; None: a new contiguous one.  With out given and outline_px = 0 nothing is allocated (after the first call, which
        makes the default style); with an outline the band and its scratch are made at the first call and kept.  No host read; step() is
        untouched.  Returns out.  RuntimeError before the first step."""
        B, H, W = self.batch, self.H, self.W
        if self._dev is None:
            raise RuntimeError("GazeSession.render() draws the records step() made: call step() first")
        if not isinstance(img, (torch.Tensor, ops.Nv12Frame)) or tuple(img.shape) != (B, 3, H, W) or img.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"img must be fp32 or uint8 {(B, 3, H, W)}, got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))}")
        if img.device != self._dev:
            raise ValueError(f"the session lives on {self._dev}, img is on {img.device}")
        if style is None:
            style = getattr(self, "_style", None)
            if style is None:
                style = self._style = ops.overlay_style(device=self._dev)
        bits, band = self._rec[3], None
        d = overlay._int_ge_zero("outline_px", outline_px)
        if d > 0:
            kept = getattr(self, "_band", None)
            if kept is None or kept[0] != d:
                scratch = torch.empty(max(1, ops.hip.query("fs_mask_erode_scratch_ints", B, H, W, masks._morph_d(d))), device=self._dev, dtype=torch.int32)
                kept = self._band = (d, torch.empty_like(bits), torch.empty_like(bits), scratch)
            band = ops.overlay_band(bits, W, d, er=kept[2], scratch=kept[3], band=kept[1])[0]
        return ops.draw_instances(img, bits, stats=self._rec[1], focus=focus, style=style, out=out, live=self._gstate[:, 0], band=band)

    def _force(self, force, dev):
        if force is None:
            return None
        f = torch.as_tensor(force)
        if tuple(f.shape) != (self.batch,):
            raise ValueError(f"force must have one entry per viewer, ({self.batch},), got {tuple(f.shape)}")
        return (f != 0).to(device=dev, dtype=torch.int32)

    @torch.no_grad()
    def step(self, img, focus, force=None):
        """One frame per viewer.  img (B,3,H,W) fp32, or uint8 with the pixel value byte / 255, and focus (B,2) as predict_instances takes
        them, on the device; force: None, or B flags (any sequence or tensor), non-zero = re-make this viewer's record now.  A uint8 frame
        gives what img.float() / 255 gives bit for bit and is never converted: gate, commit, motion, the selection of the viewers that run
        and the network's front all read the bytes.  The state is the same tensors either way, so the dtype may change from step to step.
        A uint8 frame may also be a view of interleaved bytes, as a camera or a decoder makes them -- hwc.permute(0, 3, 1, 2) of a (B,H,W,3)
        buffer, rgba.permute(0, 3, 1, 2)[:, :3] of a (B,H,W,4) one, with padded rows, as a crop, or one frame expanded over the viewers
        (ops.byte_frame_layout) --: it is read where it lies, gives what its planar copy gives bit for bit, and a step in which nobody
        runs allocates nothing.  Any other non-contiguous frame is copied, as before.  An ops.Nv12Frame -- a video decoder's luma and
        chroma planes, 1.5 bytes a pixel -- is taken in a uint8 frame's place: every pass reads it where it lies and gives what it gives on
        ops.nv12_to_rgb(img) bit for bit, a step in which nobody runs allocates nothing, and a partial run gathers the running viewers'
        luma and chroma rows alone.

        Returns (cat, stats, counts, bits[, conf], gate[, motion]): the record of every viewer as predict_instances(img, focus, return_bits=True)
        makes it -- made now for the viewers that ran, the held one for the others -- and gate (B,8) int64 on the host = (code,
        n_changed, n_roi_changed, sad_total, d2_key, d2_prev, inside_bit, age + 1) per viewer (ops.gate_decide).  The record tensors are
        the session's own: the next step overwrites them.  The step reads gate once, 64 * B bytes, its only synchronisation; the
        network runs on the viewers with a RUN code alone (img itself when that is everyone, img[idx] otherwise).  img and focus are
        never written.  With motion_px the state is moved to the new frame first (the class docstring), and motion (B,6) int64 on the host =
        (dy, dx, cost_best, cost_zero, dy_total, dx_total) per viewer comes last, read in the same synchronisation: the shift applied in
        this step, the estimate's costs, and the shift summed since the record was made (0 for a viewer whose record this step made).
        RuntimeError in train mode, ValueError for other shapes than the constructor's."""
        if self.module.training:
            raise RuntimeError("GazeSession.step() needs eval mode (module.eval()): in train mode the encoder would update its BatchNorm running statistics")
        B, H, W = self.batch, self.H, self.W
        if not isinstance(img, (torch.Tensor, ops.Nv12Frame)) or tuple(img.shape) != (B, 3, H, W) or img.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"img must be fp32 or uint8 {(B, 3, H, W)}, got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))}")
        if not isinstance(focus, torch.Tensor) or tuple(focus.shape) != (B, 2):
            raise ValueError(f"focus must be ({B}, 2), got {tuple(getattr(focus, 'shape', ()))}")
        if not img.is_cuda or focus.device != img.device:
            raise ValueError("img and focus must be on the same GPU: the session has no CPU path")
        if self._dev is None:
            self._allocate(img.device)
        elif img.device != self._dev:
            raise ValueError(f"the session lives on {self._dev}, img is on {img.device}")
        fdev = self._force(force, img.device)
        # a view of interleaved bytes (ops.byte_frame_layout: a camera's HWC / RGBA buffer, permuted) is read where it lies
        # and so is an NV12 frame (ops.Nv12Frame: a decoder's surface): the state stays planar RGB bytes
        x, hwc = frames.frame_in_place(img)
        f = focus.float().contiguous()
        moving = self.motion_px is not None
        # a frame of bytes stays bytes: its pixel code is the byte, so its profiles are key_profiles of it and the gate compares bytes
        if x.dtype == torch.uint8:
            profiles, state_shift, gate_tiles, gate_commit = ops.key_profiles, ops.state_shift_u8, ops.gate_tiles_u8, ops.gate_commit_u8
        else:
            profiles, state_shift, gate_tiles, gate_commit = ops.frame_profiles, ops.state_shift, ops.gate_tiles, ops.gate_commit
        if moving:
            profiles(x, out=self._prof)
            ops.profile_shift(self._prof, self._prof_key, self._gstate, (H, W), self.motion_px, self.motion_gain, out=self._shift)
            state_shift(x, self._shift, self._key, self._key2, self._rec[3], self._bits2, self._gstate, self._rec[1], self._rec[2],
                        self._prof_key, self._mstate, motion=self._motion, scratch=self._scratch)
        gate_tiles(x, self._key, self.tile, out=self._sad)
        ops.gate_decide(self._sad, self._gstate, f, self._rec[1], self._rec[3], (H, W), tile=self.tile, level=self.level,
                        scene_tiles=self.scene_tiles, roi_tiles=self.roi_tiles, margin=self.roi_margin, saccade2=self.saccade2,
                        fixation2=self.fixation2, max_age=self.max_age, inside_on=self.inside_on, force=fdev, out=self._gate)
        self._gate_host.copy_(self._gate, non_blocking=True)
        if moving:
            self._motion_host.copy_(self._motion, non_blocking=True)
        torch.cuda.current_stream(img.device).synchronize()
        gate = self._gate_host.clone()
        codes = gate[:, 0].tolist()
        for c in codes:
            self.counts[c] += 1
        run = [b for b, c in enumerate(codes) if c in ops.GATE_RUNS]
        if not run:
            gate_commit(x, None, self._key, self._gstate, f, self._rec, self._rec)
        else:
            idx = torch.tensor(run, dtype=torch.int32, device=img.device)
            if len(run) == B:
                xi, fi = x, focus
            else:
                sel = idx.long()
                # the running viewers of an interleaved frame stay interleaved: their bytes are gathered as they lie, no planar copy
                xi, fi = (ops.byte_frame_select(x, sel) if hwc else x.index_select(0, sel)), focus.index_select(0, sel)
            if self.component is None:
                new = list(self.module.predict_instances(xi, fi, max_runs=self.max_runs, return_bits=True, return_score=self.score))
            else:                                                          # comp, the last element, is not part of the record
                new = list(self.module.predict_instances(xi, fi, max_runs=self.max_runs, return_bits=True, return_score=self.score,
                                                         component=self.component, snap_px=self.snap_px))[:-1]
            if len(run) == B:
                # every record is new: the tensors predict_instances made become the session's, nothing is copied
                self._rec = new
            gate_commit(x, idx, self._key, self._gstate, f, new, self._rec)
            if moving:
                ops.motion_commit(idx, self._prof, self._prof_key, self._mstate, (H, W))
        if moving:
            motion = self._motion_host.clone()
            if run:
                motion[run, 4:] = 0                                        # motion_commit's totals, known without a second read
            return (*self._rec, gate, motion)
        return (*self._rec, gate)
