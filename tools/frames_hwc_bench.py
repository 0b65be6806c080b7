"""What reading interleaved (HWC / RGBA) uint8 frames in place costs and saves on one MI355X.  Eval mode, ops.static_weight_packs
(serving), HRNetV2 + C1 (LVIS-50, K = 51), input side^2 -> 80^2 grid -> side^2.  All routes run in ONE process, three rounds, the order
changing every iteration:

    step_planar               session().step on an unchanged frame and gaze (REUSE), fed a planar uint8 frame
    step_rgb / step_rgba      the same bytes as hwc.permute(0, 3, 1, 2) / rgba.permute(0, 3, 1, 2)[:, :3], read where they lie
    step_copy                 what a caller with such a buffer paid before: view.contiguous(), then the planar step
    step_copy_parent          (--parent-lib) the same through a library built from the parent commit
    *_motion                  the same with motion_px=16
    instances_planar / _rgb   module.predict_instances(frame, Fp, return_bits=True)

    python tools/frames_hwc_bench.py [--sizes 1:1024,64:1024] [--warmup 3] [--iters 10] [--parent-lib FILE.so] [--out FILE.json]
    python tools/frames_hwc_bench.py --pass-ab --parent-lib FILE.so [--out FILE.json]      # every frame pass against the parent's, below

Route figures are host wall time in ms, median (min - max) per round; a step ends with its own read-back, the other routes with a device
synchronise.  "tiles" are device-event times over 20 back-to-back calls of the tile pass, alternated over three rounds, in microseconds a
call, with the bytes each must read (planar and RGB 6 B a pixel, RGBA 7 B; the copy route reads 3 and writes 3 more) and the rate in
TB/s on those bytes: (a) fs_gate_tiles_u8 on a planar frame, (b) permute().contiguous() followed by fs_gate_tiles_u8, and
fs_gate_tiles_hwc on the RGB and the RGBA view (the vector route).

--pass-ab (for a change that must leave every pass as fast as it was; no network is built): every pass that reads a frame -- tiles,
commit, profiles, state shift with every viewer moving, gaze_lowres, grid_sample_u8 -- on an fp32, a planar uint8, an RGB and an RGBA
frame, B = 64, H = 1024, at W = 1024 (every vector route) and W = 1021 (every one-pixel route), through this tree's library and through
--parent-lib: device-event time over 100 back-to-back calls in microseconds a call, one round of both libraries that is not kept, then
three rounds in which the two alternate and the one that goes first changes; a row's ranges overlap or they do not."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

from gaze_session_bench import wall
from motion_bench import event_us

NEW = ("fs_gaze_lowres_hwc_fwd", "fs_grid_sample_hwc_fwd", "fs_gate_tiles_hwc", "fs_gate_commit_hwc", "fs_frame_profiles_hwc", "fs_state_shift_hwc")
NEW_HOST = ("fs_byte_frame_route",)


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


class ParentLibrary:
    """A library built from the parent commit, bound like this one's without those of the interleaved entry points it does not have;
    inside a `with` every hip.call goes to it."""

    def __init__(self, path):
        own_lib, own_path, own_env = hip._lib, hip.LIB_PATH, os.environ.get("FS_HIP_LIB")
        has = ctypes.CDLL(path)
        new = {k: hip.SIGNATURES.pop(k) for k in NEW if not hasattr(has, k)}
        new_host = {k: hip.HOST_ONLY.pop(k) for k in NEW_HOST if not hasattr(has, k)}
        os.environ["FS_HIP_LIB"], hip.LIB_PATH, hip._lib = path, path, None
        try:
            self.lib = hip.load()
        finally:
            hip.SIGNATURES.update(new)
            hip.HOST_ONLY.update(new_host)
            hip._lib, hip.LIB_PATH = own_lib, own_path
            if own_env is None:
                del os.environ["FS_HIP_LIB"]
            else:
                os.environ["FS_HIP_LIB"] = own_env
        self.cache = {}

    def __enter__(self):
        self.keep = (hip._lib, hip._fn_cache)
        hip._lib, hip._fn_cache = self.lib, self.cache

    def __exit__(self, *exc):
        hip._lib, hip._fn_cache = self.keep


def views(U):
    """The bytes of a planar frame as an RGB and an RGBA view of interleaved buffers (the alpha bytes random)."""
    hwc = U.permute(0, 2, 3, 1)
    rgb = hwc.contiguous().permute(0, 3, 1, 2)
    buf = torch.randint(0, 256, (*hwc.shape[:3], 4), device=U.device, dtype=torch.uint8)
    buf[..., :3] = hwc
    rgba = buf.permute(0, 3, 1, 2)[:, :3]
    assert ops.byte_frame_layout(rgb)[0] == "hwc" and ops.byte_frame_layout(rgba)[0] == "hwc"
    return rgb, rgba


def tile_pass(B, side, tile=32, rounds=3):
    """fs_gate_tiles_hwc on the RGB and the RGBA view against (a) fs_gate_tiles_u8 on the planar bytes and (b) the copy a caller made
    before, permute().contiguous(), followed by fs_gate_tiles_u8; alternated."""
    g = torch.Generator(device="cuda").manual_seed(B * 7 + side)
    U = torch.randint(0, 256, (B, 3, side, side), device="cuda", dtype=torch.uint8, generator=g)
    key = torch.randint(0, 256, (B, 3, side, side), device="cuda", dtype=torch.uint8, generator=g)
    rgb, rgba = views(U)
    route = [int(hip.load().fs_byte_frame_route(v.data_ptr(), *ops.byte_frame_layout(v)[1:], side)) for v in (rgb, rgba)]
    T_ = (side + tile - 1) // tile
    sad = {k: torch.empty(B, T_, T_, device="cuda", dtype=torch.int32) for k in ("planar", "copy", "rgb", "rgba")}
    px = B * side * side
    calls = {"planar": (lambda: ops.gate_tiles_u8(U, key, tile, out=sad["planar"]), 6),
             "copy": (lambda: ops.gate_tiles_u8(rgb.contiguous(), key, tile, out=sad["copy"]), 12),
             "rgb": (lambda: ops.gate_tiles_u8(rgb, key, tile, out=sad["rgb"]), 6),
             "rgba": (lambda: ops.gate_tiles_u8(rgba, key, tile, out=sad["rgba"]), 7)}
    out = []
    for _ in range(rounds):
        row = {}
        for k, (fn, bpp) in calls.items():
            us = event_us(fn)
            row[k + "_us"], row[k + "_TBps"] = round(us, 2), round(bpp * px / us / 1e6, 3)
        out.append(row)
    spread = lambda k: (min(r[k + "_us"] for r in out), max(r[k + "_us"] for r in out))
    return {"batch": B, "side": side, "tile": tile, "routes": route, "bytes_per_pixel": {k: v[1] for k, v in calls.items()},
            "equal": all(bool(torch.equal(sad["planar"], v)) for v in sad.values()), "rounds": out,
            "rgb_beats_copy_outside_the_spread": spread("rgb")[1] < spread("copy")[0],
            "rgba_beats_copy_outside_the_spread": spread("rgba")[1] < spread("copy")[0]}


def frame_passes(B, H, W):
    """layout -> pass -> a call of the op on tensors of its own."""
    g = torch.Generator(device="cuda").manual_seed(B * 7 + W)
    rnd = lambda *s: torch.randint(0, 256, s, device="cuda", dtype=torch.uint8, generator=g)
    U, key = rnd(B, 3, H, W), rnd(B, 3, H, W)
    rgb, rgba = views(U)
    P, cap = (W + 31) // 32, 64
    focus = torch.rand(B, 2, device="cuda")
    idx = torch.arange(B, dtype=torch.int32, device="cuda")
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    shift = i64(B, 4)
    shift[:, 0], shift[:, 1] = 3, -5
    grid = torch.rand(B, 256, 256, 2, device="cuda") * 2 - 1
    calls = {}
    for name, x in {"fp32": (U.cpu().float() / 255).cuda(), "planar": U, "rgb": rgb, "rgba": rgba}.items():
        f32 = x.dtype == torch.float32
        tiles, commit, profiles, move = ((ops.gate_tiles, ops.gate_commit, ops.frame_profiles, ops.state_shift) if f32 else
                                         (ops.gate_tiles_u8, ops.gate_commit_u8, ops.key_profiles, ops.state_shift_u8))
        sad, prof = i32(B, (H + 31) // 32, (W + 31) // 32), i32(B, H + W)
        k, k2, bits, bits2 = key.clone(), key.clone(), i32(B, H, P), i32(B, H, P)
        bits[:, H // 4:H // 2, 1:P - 1] = -1
        rec = (i64(B), i64(B, 6), i32(B, cap), bits.clone())
        st = (i64(B, 6), i64(B, 6), i32(B, cap), ops.key_profiles(key), i64(B, 4), i64(B, 6), ops.state_shift_scratch(B, H, W, cap, "cuda"))
        gstate = i64(B, 6)
        calls[name] = {"tiles": lambda x=x, sad=sad, tiles=tiles: tiles(x, key, 32, out=sad),
                       "commit": lambda x=x, k=k, gstate=gstate, rec=rec, commit=commit: commit(x, idx, k, gstate, focus, rec, rec),
                       "profiles": lambda x=x, prof=prof, profiles=profiles: profiles(x, out=prof),
                       "shift": lambda x=x, k=k, k2=k2, bits=bits, bits2=bits2, st=st, move=move: move(x, shift, k, k2, bits, bits2, *st),
                       "lowres": lambda x=x: ops.gaze_lowres(x, focus, 256, 256)}
        if not f32:
            calls[name]["sample"] = lambda x=x: ops.grid_sample_u8(x, grid)
    return calls


def pass_ab(parent, out):
    def timed(who, fn):
        if who == "new":
            return round(event_us(fn, 100), 2)
        with parent:
            return round(event_us(fn, 100), 2)
    res = []
    for B, H, W in ((64, 1024, 1024), (64, 1024, 1021)):
        calls, rows = frame_passes(B, H, W), {}
        for rnd in range(-1, 3):                         # round -1 is not kept
            for name, of_layout in calls.items():
                for what, fn in of_layout.items():
                    order = ("new", "parent") if rnd % 2 == 0 else ("parent", "new")
                    timed(order[1], fn)                  # not kept: whoever goes first follows the other library's run of the same pass
                    for who in order:
                        t = timed(who, fn)
                        if rnd >= 0:
                            rows.setdefault((name, what), {"new": [], "parent": []})[who].append(t)
        for (name, what), r in rows.items():
            res.append({"B": B, "H": H, "W": W, "layout": name, "pass": what, "new_us": r["new"], "parent_us": r["parent"],
                        "ranges_overlap": min(r["new"]) <= max(r["parent"]) and min(r["parent"]) <= max(r["new"])})
            print(json.dumps(res[-1]), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1:1024,64:1024", help="batch:side pairs")
    ap.add_argument("--tile-sizes", default="", help="batch:side pairs for the tile pass alone")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--motion-px", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pass-ab", action="store_true", help="every frame pass, this library against --parent-lib, and nothing else")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frames_hwc_bench measures on the GPU"
    hip.load()
    if args.pass_ab:
        assert args.parent_lib, "--pass-ab compares with --parent-lib"
        return pass_ab(ParentLibrary(args.parent_lib), args.out)
    module, _ = T.build_module(fovealseg.lvis50_cfg(), device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    with torch.no_grad():                                # as gaze_session_bench: a large background logit lets the mask plane draw a blob
        module.decoder.cls_net.fc.bias[-1] += 1000.0
    parent = ParentLibrary(args.parent_lib) if args.parent_lib else None
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(), "motion_px": args.motion_px, "sizes": [], "tiles": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            X0, Fp, _Y, _cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            U = (X0.clamp(0, 1) * 255).round().to(torch.uint8)
            del X0, _Y
            rgb, rgba = views(U)
            frames = {"planar": U, "rgb": rgb, "rgba": rgba}
            mk = lambda **kw: fovealseg.GazeSession(module, B, (side, side), **kw)
            mo = dict(motion_px=args.motion_px)
            sess, routes = {}, {}

            def through_parent(fn):
                def run():
                    with parent:
                        return fn()
                return run
            for tail, kw in (("", {}), ("_motion", mo)):
                for name, frame in frames.items():
                    k = "step_" + name + tail
                    sess[k] = mk(**kw)
                    routes[k] = ((lambda k=k, frame=frame: sess[k].step(frame, Fp)), False)
                k = "step_copy" + tail                   # the parent's step on a view: img.contiguous(), then the planar passes
                sess[k] = mk(**kw)
                routes[k] = ((lambda k=k: sess[k].step(rgb.contiguous(), Fp)), False)
                if parent is not None:
                    k = "step_copy_parent" + tail
                    sess[k] = mk(**kw)
                    routes[k] = (through_parent(lambda k=k: sess[k].step(rgb.contiguous(), Fp)), False)
            routes["instances_planar"] = (lambda: module.predict_instances(U, Fp, return_bits=True), True)
            routes["instances_rgb"] = (lambda: module.predict_instances(rgb, Fp, return_bits=True), True)
            for k, s in sess.items():                    # every record is made from the one frame
                assert routes[k][0]()[len(s._rec)][:, 0].tolist() == [1] * B
            for _ in range(args.warmup):
                for fn, _sync in routes.values():
                    fn()
            keys, rng = list(routes), random.Random(B * 1009 + side)
            rounds, codes_ok, equal = [], True, True
            for _ in range(3):
                ms = {k: [] for k in routes}
                for it in range(args.iters):
                    order = list(keys)
                    rng.shuffle(order)                   # a seeded shuffle: no route keeps the same predecessor
                    outs = {}
                    for k in order:
                        t, outs[k] = wall(*routes[k])
                        ms[k].append(t)
                    torch.cuda.synchronize()
                    for k, s in sess.items():
                        codes_ok &= outs[k][len(s._rec)][:, 0].tolist() == [0] * B
                        equal &= all(bool(torch.equal(a, b)) for a, b in zip(outs[k][:4], outs["step_planar"][:4]))
                    equal &= all(bool(torch.equal(a, b)) for a, b in zip(outs["instances_rgb"], outs["instances_planar"]))
                    del outs
                rounds.append({k: stats(v) for k, v in ms.items()})
            row = {"batch": B, "side": side, "iters": args.iters, "rounds": rounds, "every_step_reuse": codes_ok, "records_equal": equal,
                   "copy_minus_rgb_ms": [round(r["step_copy"]["ms_median"] - r["step_rgb"]["ms_median"], 4) for r in rounds],
                   "copy_minus_rgb_motion_ms": [round(r["step_copy_motion"]["ms_median"] - r["step_rgb_motion"]["ms_median"], 4) for r in rounds],
                   "rgb_minus_planar_ms": [round(r["step_rgb"]["ms_median"] - r["step_planar"]["ms_median"], 4) for r in rounds],
                   "rgb_minus_planar_motion_ms": [round(r["step_rgb_motion"]["ms_median"] - r["step_planar_motion"]["ms_median"], 4) for r in rounds]}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del U, rgb, rgba, frames, Fp, sess, routes
            torch.cuda.empty_cache()
            res["tiles"].append(tile_pass(B, side))
            print(json.dumps(res["tiles"][-1]), flush=True)
        for spec in filter(None, args.tile_sizes.split(",")):
            B, side = (int(v) for v in spec.split(":"))
            res["tiles"].append(tile_pass(B, side))
            print(json.dumps(res["tiles"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
