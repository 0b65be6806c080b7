"""GazeSession restated in numpy, a stub head with a numpy twin, and a seeded stream generator (tests/test_session_streams.py).  Not a
test module.

RefSession is the class docstring of fovealseg.session.GazeSession written out step by step over the pieces the kernels are already
held to: gate_ref (tiles, decide, commit), motion_ref (frame_profiles, profile_shift, state_shift, motion_commit) and rle_ref.  It holds
numpy copies of the state and knows nothing of layouts: a frame reaches it as fp32 (B,3,H,W), a byte frame u as u.astype(float32) / 255.
Everything is integers, so a device session is held to it bit for bit.

The head is a stub: a record that is a pure integer function of one viewer's own frame and gaze (stub_record in numpy, StubModule with
torch and ops.mask_bits / ops.mask_rle on the device), so that a wrong row in the subset that runs shows in the record."""
import functools

import numpy as np

import gate_ref as R
import motion_ref as M
import rle_ref as RLE

OFF2 = 2 ** 62
_DEFAULT = object()


# --------------------------------------------------------------------------------------------------- the moves of motion_ref, sliced --
def _overlap(n, d):
    """(destination slice, source slice) of an axis of n entries moved by d: out[i] = in[i - d] where both lie in 0 .. n - 1."""
    if abs(d) >= n:
        return slice(0, 0), slice(0, 0)
    return (slice(d, n), slice(0, n - d)) if d >= 0 else (slice(0, n + d), slice(-d, n))


def move_key(key_b, img_b, dy, dx):
    """motion_ref.move_key without the loop over pixels."""
    out = R.q(img_b).astype(np.uint8)
    (yd, ys), (xd, xs) = _overlap(key_b.shape[1], dy), _overlap(key_b.shape[2], dx)
    out[:, yd, xd] = key_b[:, ys, xs]
    return out


def move_mask(mask, dy, dx):
    """motion_ref.move_mask without the loop over pixels."""
    out = np.zeros_like(mask)
    (yd, ys), (xd, xs) = _overlap(mask.shape[0], dy), _overlap(mask.shape[1], dx)
    out[yd, xd] = mask[ys, xs]
    return out


def state_shift(img, shift, key, bits, gstate, stats, counts, prof_key, mstate):
    """motion_ref.state_shift with the sliced moves; also returns, per moved viewer, what the coverage conditions ask about:
    diag[b] = (area before, area after, n_runs before, a key gaze coordinate clamped)."""
    B, _, H, W = img.shape
    cap = counts.shape[1]
    key, bits, gstate, stats, counts = key.copy(), bits.copy(), gstate.copy(), stats.copy(), counts.copy()
    prof_key, mstate = prof_key.copy(), mstate.copy()
    motion = np.zeros((B, 6), dtype=np.int64)
    diag = {}
    for b in range(B):
        dy, dx = int(shift[b, 0]), int(shift[b, 1])
        if (dy, dx) != (0, 0):
            before = RLE.unbits(bits[b], W)
            mask = move_mask(before, dy, dx)
            clamped = not (0 <= int(gstate[b, 1]) + 16 * dy <= (H - 1) * 16 and 0 <= int(gstate[b, 2]) + 16 * dx <= (W - 1) * 16)
            diag[b] = (int(before.sum()), int(mask.sum()), int(stats[b, 5]), clamped)
            key[b] = move_key(key[b], img[b], dy, dx)
            bits[b] = RLE.bits(mask)
            gstate[b, 1], gstate[b, 3] = M.move_gaze(gstate[b, 1], dy, H), M.move_gaze(gstate[b, 3], dy, H)
            gstate[b, 2], gstate[b, 4] = M.move_gaze(gstate[b, 2], dx, W), M.move_gaze(gstate[b, 4], dx, W)
            stats[b] = RLE.stats(mask)
            counts[b] = RLE.counts_row(mask, cap)
            prof_key[b] = M.key_profiles(key[b:b + 1])[0]
            mstate[b] += (dy, dx, 1, abs(dy) + abs(dx))
        motion[b] = (dy, dx, shift[b, 2], shift[b, 3], mstate[b, 0], mstate[b, 1])
    return key, bits, gstate, stats, counts, prof_key, mstate, motion, diag


# ------------------------------------------------------------------------------------------------------------------ the session ------
class RefSession:
    """GazeSession in numpy.  predict(img (n,3,H,W) fp32, focus (n,2) fp32) -> [cat (n,), stats (n,6), counts (n,cap), bits (n,H,P)[,
    conf (n,3)]] stands for module.predict_instances on the viewers that run, in ascending order; the other arguments are
    GazeSession's, converted on the host as it converts them."""

    def __init__(self, predict, batch, frame_size, *, tile=32, level=8, scene_frac=0.25, roi_tiles=0, roi_margin=16, fixation_px=None,
                 saccade_px=_DEFAULT, max_age=0, reuse_inside_mask=True, max_runs=None, score=False, component=None, snap_px=None,
                 motion_px=None, motion_gain=6):
        self.predict, self.B = predict, int(batch)
        self.H, self.W = H, W = int(frame_size[0]), int(frame_size[1])
        self.tile, self.level = int(tile), int(level)
        self.th, self.tw = -(-H // self.tile), -(-W // self.tile)
        self.scene_tiles = int(np.floor(float(scene_frac) * self.th * self.tw))
        self.roi_tiles, self.roi_margin = int(roi_tiles), int(roi_margin)
        side = min(H, W)
        self.fixation2 = R.thr2(0.03 * side if fixation_px is None else fixation_px)
        self.saccade2 = OFF2 if saccade_px is None else R.thr2(0.10 * side if saccade_px is _DEFAULT else saccade_px)
        self.max_age, self.inside_on = int(max_age), bool(reuse_inside_mask)
        self.cap = 8 * W + 1 if max_runs is None else int(max_runs)
        self.score = bool(score)
        self.motion_px, self.motion_gain = (None if motion_px is None else int(motion_px)), int(motion_gain)
        B, P = self.B, (W + 31) // 32
        self.key = np.zeros((B, 3, H, W), dtype=np.uint8)
        self.gstate = np.zeros((B, 6), dtype=np.int64)
        self.sad = np.zeros((B, self.th, self.tw), dtype=np.int64)
        self.rec = [np.zeros(B, dtype=np.int64), np.zeros((B, 6), dtype=np.int64), np.zeros((B, self.cap), dtype=np.int32),
                    np.zeros((B, H, P), dtype=np.int32)]
        if self.score:
            self.rec.append(np.zeros((B, 3), dtype=np.float32))
        self.prof = np.zeros((B, H + W), dtype=np.int64)
        self.prof_key = np.zeros((B, H + W), dtype=np.int64)
        self.mstate = np.zeros((B, 4), dtype=np.int64)
        self.counts = {code: 0 for code in range(8)}
        self.diag = {}

    def reset(self, viewers=None):
        for v in (range(self.B) if viewers is None else viewers):
            self.gstate[int(v), 0] = 0

    def mask(self, b):
        return RLE.unbits(self.rec[3][b], self.W)

    def step(self, img, focus, force=None):
        """-> (cat, stats, counts, bits[, conf], gate[, motion]); self.ran lists the viewers that ran, self.diag what the move did."""
        img, focus = np.asarray(img, dtype=np.float32), np.asarray(focus, dtype=np.float32)
        H, W = self.H, self.W
        assert img.shape == (self.B, 3, H, W) and focus.shape == (self.B, 2)
        moving = self.motion_px is not None
        self.diag = {}
        if moving:
            self.prof = M.frame_profiles(img)
            shift = M.profile_shift(self.prof, self.prof_key, self.gstate, H, W, self.motion_px, self.motion_gain)
            (self.key, self.rec[3], self.gstate, self.rec[1], self.rec[2], self.prof_key, self.mstate, motion, self.diag) = state_shift(
                img, shift, self.key, self.rec[3], self.gstate, self.rec[1], self.rec[2], self.prof_key, self.mstate)
        self.sad = R.tiles(img, self.key, self.tile)
        gate = R.decide(self.sad, self.gstate, focus, self.rec[1], self.rec[3], force, H, W, self.tile, self.level, self.scene_tiles,
                        self.roi_tiles, self.roi_margin, self.saccade2, self.fixation2, self.max_age, self.inside_on)
        for c in gate[:, 0].tolist():
            self.counts[c] += 1
        run = [b for b in range(self.B) if int(gate[b, 0]) in R.RUNS]
        new = [np.asarray(a) for a in self.predict(img[run], focus[run])] if run else self.rec
        self.key, self.gstate, self.rec = R.commit(img, run, self.key, self.gstate, focus, new, self.rec)
        self.ran = run
        if not moving:
            return (*self.rec, gate)
        if run:
            self.prof_key, self.mstate = M.motion_commit(run, self.prof, self.prof_key, self.mstate)
            motion[run, 4:] = 0
        return (*self.rec, gate, motion)


# ------------------------------------------------------------------------------------------------------------------ the stub head ----
STUB_LUMA, STUB_CATS = 383, 50


def stub_record(img, focus, H, W, cap, score):
    """The stub's record of one viewer: img (3,H,W) fp32, focus (2,) -> (cat, stats (6,), counts (cap,), bits (H,P)[, conf (3,)])."""
    L = R.q(img).sum(0)
    py, px = (R.gaze(focus[0], H) + 8) >> 4, (R.gaze(focus[1], W) + 8) >> 4
    r = min(H, W) // 4
    y, x = np.mgrid[:H, :W]
    mask = (L >= STUB_LUMA) & (np.maximum(np.abs(y - py), np.abs(x - px)) <= r)
    cat = (31 * py + 17 * px) % STUB_CATS
    rec = [np.int64(cat), np.array(RLE.stats(mask), dtype=np.int64), RLE.counts_row(mask, cap), RLE.bits(mask)]
    if score:
        rec.append(np.array([L[py, px], int(mask.sum()) % 1024, cat], dtype=np.float32))
    return tuple(rec)


def stub_predict(H, W, cap, score):
    """RefSession's predict made of stub_record."""
    def predict(img, focus):
        rows = [stub_record(img[j], focus[j], H, W, cap, score) for j in range(img.shape[0])]
        return [np.stack([r[k] for r in rows]) for k in range(len(rows[0]))]
    return predict


class StubModule:
    """stub_record on the device, with predict_instances' signature: what GazeSession needs of a module and nothing else."""
    training = False

    def __init__(self):
        self.calls = []                                  # the batch size of every call
        self.seen = []                                   # and how its frames lay: "f32", or "planar" / "hwc" (ops.byte_frame_layout)

    def predict_instances(self, img, focus, seg_size=None, max_runs=None, return_bits=False, return_score=False, component=None, snap_px=None):
        import torch
        from fovealseg import ops
        n, _, H, W = (int(v) for v in img.shape)
        self.calls.append(n)
        if img.dtype == torch.uint8:
            layout = ops.byte_frame_layout(img)
            self.seen.append(None if layout is None else layout[0])
            c = img.long()
        else:
            self.seen.append("f32")
            v = torch.where(torch.isnan(img), torch.zeros_like(img), img).clamp(0.0, 1.0)
            c = torch.round(v * 255.0).long()
        L = c.sum(1)
        g = []
        for k, side in ((0, H), (1, W)):
            top = (side - 1) * 16
            t = torch.round(focus[:, k].double() * float(top))
            g.append((torch.where(torch.isnan(t), torch.zeros_like(t), t).clamp(0.0, float(top)).long() + 8) >> 4)
        py, px = g
        r = min(H, W) // 4
        y = torch.arange(H, device=img.device).view(1, H, 1)
        x = torch.arange(W, device=img.device).view(1, 1, W)
        mask = (L >= STUB_LUMA) & (torch.maximum((y - py.view(n, 1, 1)).abs(), (x - px.view(n, 1, 1)).abs()) <= r)
        bits = ops.mask_bits(mask)
        stats, counts = ops.mask_rle(bits, W, max_runs=max_runs)
        cat = (31 * py + 17 * px) % STUB_CATS
        out = [cat, stats, counts]
        if return_bits:
            out.append(bits)
        if return_score:
            rows = torch.arange(n, device=img.device)
            out.append(torch.stack([L[rows, py, px], stats[:, 0] % 1024, cat], dim=1).float())
        if component is not None:
            out.append(torch.zeros(n, 4, dtype=torch.int64, device=img.device))       # comp: not part of the record
        return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ frames -----------
LAYOUTS = ("f32", "wild", "u8", "hwc", "rgba", "crop")
BYTE_LAYOUTS = ("u8", "hwc", "rgba", "crop")
HEAD_SEES = dict(f32="f32", wild="f32", u8="planar", hwc="hwc", rgba="hwc", crop="hwc", expand="hwc")     # a frame is never converted
CROP_PAD = (2, 3, 3, 4)                                  # rows above, columns left, rows below, columns right of a "crop" frame


def model_frame(rgba, layout):
    """What the model sees of a step's bytes (B,H,W,4) in a layout: fp32 (B,3,H,W).  "wild" is fp32 only -- the pixels whose fourth
    byte is below 5 take values no byte stands for (NaN, below 0, above 1, infinite), so that q clamps; every other layout is bytes / 255."""
    img = np.ascontiguousarray(rgba[..., :3].transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)
    if layout == "wild":
        a = rgba[..., 3]
        img[:, 0][a == 0] = np.float32("nan")
        img[:, 1][a == 1] = np.float32(-3.5)
        img[:, 2][a == 2] = np.float32(1.0 + 2.0 ** -20)
        img[:, 0][a == 3] = np.float32("inf")
        img[:, 1][a == 4] = np.float32("-inf")
    return img


def device_frame(rgba, layout, device="cuda"):
    """The same step as the tensor a caller would hand to GazeSession.step in that layout."""
    import torch
    B, H, W, _ = rgba.shape
    if layout in ("f32", "wild"):
        return torch.from_numpy(model_frame(rgba, layout)).to(device)
    buf = torch.from_numpy(rgba).to(device)
    if layout == "u8":
        return buf[..., :3].permute(0, 3, 1, 2).contiguous()
    if layout == "hwc":
        return buf[..., :3].contiguous().permute(0, 3, 1, 2)
    if layout == "rgba":
        return buf.permute(0, 3, 1, 2)[:, :3]
    if layout == "crop":
        t, l, b, r = CROP_PAD
        big = torch.full((B, H + t + b, W + l + r, 4), 0x5B, dtype=torch.uint8, device=device)
        big[:, t:t + H, l:l + W] = buf
        return big[:, t:t + H, l:l + W].permute(0, 3, 1, 2)[:, :3]
    if layout == "expand":
        assert B == 1
        return buf[0].permute(2, 0, 1)[:3].unsqueeze(0).expand(B, 3, H, W)
    raise ValueError(layout)


# ------------------------------------------------------------------------------------------------------------------ the stream -------
PAD = 24                                                 # the canvas is the frame and PAD pixels around it
PROBS = dict(run=0.10, jump=0.02, cut=0.02, flip=0.04, noise=0.04, jitter=0.06, on_set=0.03, on_clear=0.04, saccade=0.03, edge=0.03,
             force=0.03, reset=0.04, reset_beside_run=0.12, reset_all=0.2)


@functools.lru_cache(maxsize=None)
def _canvas_bytes(seed, H, W):
    return np.rint(M.canvas(seed, H + 2 * PAD, W + 2 * PAD, 4) * np.float32(255)).astype(np.uint8)


def _ring(rng, mask, want, py, px, lo, hi):
    """A pixel of the frame between lo and hi pixels from (py, px); with a mask, one whose bit is `want`.  None if there is none."""
    H, W = mask.shape
    y, x = np.mgrid[:H, :W]
    d = np.hypot(y - py, x - px)
    ok = (d > lo) & (d < hi)
    if want is not None:
        ok &= mask == want
    cand = np.flatnonzero(ok)
    if cand.size == 0:
        return None
    i = int(cand[rng.integers(cand.size)])
    return i // W, i % W


def stream(seed, B, H, W, steps, R_motion, *, tile=32, fixation_px=None, saccade_px=_DEFAULT, model=None, layouts=None, probs=None):
    """A seeded stream: yields per step (frame bytes (B,H,W,4) uint8, focus (B,2) fp32, force or None, viewers to reset or None,
    layout).  The reset comes before the step.  Per viewer a camera sits on an M.canvas texture of scale 4 and M.window cuts the frame;
    the fourth byte is noise no reader may use.  `model` is a RefSession the consumer steps with every item before it asks for the
    next: the generator reads the viewers' current masks from it to aim the gaze at set and at clear pixels.  Without it those draws
    aim at any pixel of the ring."""
    rng = np.random.default_rng(seed)
    p = dict(PROBS, **(probs or {}))
    layouts = tuple(layouts or (LAYOUTS + (("expand",) if B == 1 else ())))
    Rt = R_motion if R_motion is not None else 2
    side = min(H, W)
    fix = 0.03 * side if fixation_px is None else float(fixation_px)
    sacc = 9.0 if saccade_px is None else (0.10 * side if saccade_px is _DEFAULT else float(saccade_px))
    lo, hi = fix + 0.6, sacc - 0.6
    seeds = [1000 * seed + b for b in range(B)]
    next_seed = 1000 * seed + 100
    cam = [[PAD + int(rng.integers(-4, 5)), PAD + int(rng.integers(-4, 5))] for _ in range(B)]
    gaze = [[int(rng.integers(H // 4, 3 * H // 4)), int(rng.integers(W // 4, 3 * W // 4))] for _ in range(B)]
    anchor = [list(g) for g in gaze]
    plans = [[] for _ in range(B)]
    if R_motion is not None:                             # a move within three steps of the first step, in which everybody runs
        plans[0] = [dict(), dict(shift=(1, -Rt)), dict(shift=(1, -Rt))]
    todo = {(a, b) for a in layouts for b in layouts if a != b}
    layout = None

    def clampg(g):
        return [min(max(int(g[0]), 0), H - 1), min(max(int(g[1]), 0), W - 1)]

    def run_plan(d=None, n=None):
        if d is None:
            while True:
                d = (int(rng.integers(-Rt, Rt + 1)), int(rng.integers(-Rt, Rt + 1)))
                if d != (0, 0):
                    break
            kind = rng.random()
            if kind < 0.3:                               # both components
                d = (d[0] or 1, d[1] or -1)
            elif kind < 0.55:                            # the full range
                d = (Rt if d[0] >= 0 else -Rt, d[1])
        n = int(rng.integers(3, 7)) if n is None else n
        return [dict(shift=d) for _ in range(n)]

    for t in range(steps):
        force = [0] * B
        reset = None
        u = rng.random()
        running = [b for b in range(B) if sum("shift" in a for a in plans[b]) >= 2]
        if t > 0 and B > 1 and running and u < p["reset_beside_run"]:
            w = running[int(rng.integers(len(running)))]
            reset = [w + 1 if w + 1 < B else w - 1]
        elif t > 0 and u < p["reset"] + (p["reset_beside_run"] if running else 0.0):
            reset = list(range(B)) if rng.random() < p["reset_all"] or B == 1 else sorted(rng.choice(B, size=int(rng.integers(1, B)), replace=False).tolist())
            if len(reset) == B and R_motion is not None and not plans[0]:
                plans[0] = [dict()] + run_plan(n=3)      # everybody runs, and a move follows
        frames = np.empty((B, H, W, 4), dtype=np.uint8)
        for b in range(B):
            if not plans[b] and t > 0:
                u, acc = rng.random(), 0.0
                for what in ("run", "jump", "cut", "flip", "noise", "jitter", "on_set", "on_clear", "saccade", "edge", "force"):
                    acc += p[what]
                    if u < acc:
                        break
                else:
                    what = "still"
                if what == "run":
                    plans[b] = run_plan()
                    k = int(rng.integers(len(plans[b])))
                    extra = rng.random()
                    if extra < 0.2:
                        plans[b][k]["force"] = True      # a move and a run in one step
                    elif extra < 0.4:
                        plans[b][k]["gaze"] = "on_clear"
                elif what == "jump":
                    far = Rt + int(rng.integers(2, 7))
                    plans[b] = [dict(shift=(far, 0) if rng.random() < 0.5 else (int(rng.integers(-Rt, Rt + 1)), -far))]
                elif what == "edge" and R_motion is not None:
                    e = int(rng.integers(4))
                    spot = [int(rng.integers(0, 3)), int(rng.integers(W // 4, 3 * W // 4))] if e < 2 else [int(rng.integers(H // 4, 3 * H // 4)), int(rng.integers(0, 3))]
                    out = [-int(rng.integers(2, Rt + 1)), int(rng.integers(-1, 2))] if e < 2 else [int(rng.integers(-1, 2)), -int(rng.integers(2, Rt + 1))]
                    if e % 2:                            # the far edge
                        k = 0 if e < 2 else 1
                        spot[k], out[k] = (H, W)[k] - 1 - spot[k], -out[k]
                    plans[b] = [dict(gaze="goto", spot=spot), dict(force=True)] + run_plan(d=tuple(out), n=int(rng.integers(3, 5)))
                elif what == "saccade":
                    plans[b] = [dict(gaze="saccade"), dict()]
                elif what in ("edge", "still"):
                    plans[b] = [dict()]
                elif what == "force":
                    plans[b] = [dict(force=True)]
                elif what in ("jitter", "on_set", "on_clear"):
                    plans[b] = [dict(gaze=what)]
                else:
                    plans[b] = [{what: True}]
            act = plans[b].pop(0) if plans[b] else {}
            d = act.get("shift", (0, 0))
            ny, nx = cam[b][0] - d[0], cam[b][1] - d[1]
            if not (0 <= ny <= 2 * PAD and 0 <= nx <= 2 * PAD):                         # the canvas ends: the camera turns round
                d = (-d[0], -d[1])
                for a in plans[b]:
                    if "shift" in a:
                        a["shift"] = (-a["shift"][0], -a["shift"][1])
                ny, nx = cam[b][0] - d[0], cam[b][1] - d[1]
                if not (0 <= ny <= 2 * PAD and 0 <= nx <= 2 * PAD):
                    d, (ny, nx) = (0, 0), cam[b]
            cam[b] = [ny, nx]
            if act.get("cut"):
                seeds[b], next_seed = next_seed, next_seed + 1
            canv = _canvas_bytes(seeds[b], H, W)
            f = canv[:, cam[b][0]:cam[b][0] + H, cam[b][1]:cam[b][1] + W].transpose(1, 2, 0).copy()
            # the gaze: it goes with the content unless the step says otherwise
            g = act.get("gaze", "follow")
            gaze[b], anchor[b] = clampg([gaze[b][0] + d[0], gaze[b][1] + d[1]]), clampg([anchor[b][0] + d[0], anchor[b][1] + d[1]])
            if g == "jitter":
                gaze[b] = clampg([anchor[b][0] + int(rng.integers(-1, 2)), anchor[b][1] + int(rng.integers(-1, 2))])
            elif g in ("on_set", "on_clear"):
                mask = move_mask(model.mask(b), d[0], d[1]) if model is not None else np.zeros((H, W), dtype=bool)
                hit = _ring(rng, mask, (g == "on_set") if model is not None else None, gaze[b][0], gaze[b][1], lo, hi)
                if hit is not None:
                    gaze[b] = anchor[b] = list(hit)
            elif g == "saccade":
                hit = _ring(rng, np.zeros((H, W), dtype=bool), None, gaze[b][0], gaze[b][1], sacc + 2.0, float(H + W))
                gaze[b] = anchor[b] = list(hit)
            elif g == "goto":
                gaze[b] = anchor[b] = list(act["spot"])
            if act.get("flip"):                          # a few tiles change, at the gaze (the region of interest) or anywhere
                for _ in range(int(rng.integers(1, 4))):
                    ty, tx = (gaze[b][0] // tile, gaze[b][1] // tile) if rng.random() < 0.7 else (int(rng.integers(-(-H // tile))), int(rng.integers(-(-W // tile))))
                    ty, tx = min(max(ty + int(rng.integers(-1, 2)), 0), -(-H // tile) - 1), min(max(tx + int(rng.integers(-1, 2)), 0), -(-W // tile) - 1)
                    f[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile] = 255 - f[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile]
            if act.get("noise"):
                f = np.clip(f.astype(np.int64) + rng.integers(-5, 6, f.shape), 0, 255).astype(np.uint8)
            force[b] = int(bool(act.get("force")))
            frames[b, :, :, :3] = f
            frames[b, :, :, 3] = rng.integers(0, 256, (H, W))
        # the layout: a pair of consecutive layouts not yet seen where there is one, any layout otherwise
        fresh = [n for n in layouts if (layout, n) in todo]
        pick = fresh if fresh else list(layouts)
        nxt = pick[int(rng.integers(len(pick)))]
        todo.discard((layout, nxt))
        layout = nxt
        focus = np.array([[g[0] / (H - 1), g[1] / (W - 1)] for g in gaze], dtype=np.float32)
        yield frames, focus, (force if any(force) else None), reset, layout


# ------------------------------------------------------------------------------------------------------------------ configurations ---
CONFIGS = {
    "A": dict(B=3, H=72, W=100, steps=120, seed=1, kw=dict(tile=16, max_age=5, score=True, roi_tiles=1)),
    "B": dict(B=3, H=72, W=100, steps=120, seed=2, kw=dict(tile=32, motion_px=4, component=8)),
    "C": dict(B=2, H=67, W=93, steps=120, seed=2, kw=dict(tile=8, motion_px=3, reuse_inside_mask=False, saccade_px=None, max_runs=6, motion_gain=8)),
    "D": dict(B=1, H=64, W=64, steps=120, seed=1, kw=dict(tile=64, motion_px=5, score=True, scene_frac=0)),
}


def make_model(name, predict=None):
    c = CONFIGS[name]
    kw = c["kw"]
    cap = 8 * c["W"] + 1 if kw.get("max_runs") is None else kw["max_runs"]
    return RefSession(predict or stub_predict(c["H"], c["W"], cap, bool(kw.get("score"))), c["B"], (c["H"], c["W"]), **kw)


def config_stream(name, model):
    c = CONFIGS[name]
    kw = c["kw"]
    extra = {k: kw[k] for k in ("saccade_px", "fixation_px") if k in kw}
    return stream(c["seed"], c["B"], c["H"], c["W"], c["steps"], kw.get("motion_px"), tile=kw["tile"], model=model, probs=c.get("probs"), **extra)


@functools.lru_cache(maxsize=None)
def trace(name):
    """The stream of a configuration run through the model, once: a list of per-step dicts -- the inputs (rgba, focus, force, reset,
    layout), the model's frame, its outputs (out), the viewers that ran, what the move did (diag), the counts dict and the state after
    the step.  Read-only: the tests share it."""
    model = make_model(name)
    steps = []
    for rgba, focus, force, reset, layout in config_stream(name, model):
        if reset is not None:
            model.reset(None if len(reset) == model.B else reset)
        img = model_frame(rgba, layout)
        out = model.step(img, focus, force)
        steps.append(dict(rgba=rgba, focus=focus, force=force, reset=reset, layout=layout, img=img, out=[np.array(a) for a in out],
                          ran=list(model.ran), diag=dict(model.diag), counts=dict(model.counts),
                          state=dict(key=model.key.copy(), gstate=model.gstate.copy(), sad=model.sad.copy(), prof=model.prof.copy(),
                                     prof_key=model.prof_key.copy(), mstate=model.mstate.copy())))
    return steps
