"""What feeding frames as bytes costs and saves on one MI355X.  Eval mode, ops.static_weight_packs (serving), HRNetV2 + C1 (LVIS-50,
K = 51), input side^2 -> 80^2 grid -> side^2.  All routes run in ONE process, three rounds, the order changing every iteration:

    step_u8 / step_f32        session().step on an unchanged frame and gaze (REUSE), fed uint8 / fed the same frame as fp32
    step_convert              the route a caller with bytes had before: u8.float().div_(255), then step
    *_motion                  the same three with motion_px=16
    instances_u8 / _f32       module.predict_instances(frame, Fp, return_bits=True)
    *_parent                  (--parent-lib) step_f32 and instances_f32 through a library built from the parent commit

    python tools/frames_u8_bench.py [--sizes 1:1024,64:1024] [--warmup 3] [--iters 10] [--parent-lib FILE.so] [--out FILE.json]

Route figures are host wall time in ms, median (min - max) per round; a step ends with its own read-back, the other routes with a device
synchronise.  "tiles" are device-event times over 20 back-to-back calls of the tile pass, alternated over three rounds, in microseconds a
call, with the bytes each must read (fs_gate_tiles 15 B a pixel, fs_gate_tiles_u8 6 B) and the rate in TB/s; --tile-sizes adds frames
the session routes are not run on (256^2: the lane cut of a narrow frame)."""
import argparse
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

NEW = ("fs_gaze_lowres_u8_fwd", "fs_grid_sample_u8_fwd", "fs_gate_tiles_u8", "fs_gate_commit_u8", "fs_state_shift_u8")


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


class ParentLibrary:
    """A library built from the parent commit, bound like this one's without the byte entry points; inside a `with` every hip.call goes
    to it."""

    def __init__(self, path):
        own_lib, own_path, own_env = hip._lib, hip.LIB_PATH, os.environ.get("FS_HIP_LIB")
        new = {k: hip.SIGNATURES.pop(k) for k in NEW}
        os.environ["FS_HIP_LIB"], hip.LIB_PATH, hip._lib = path, path, None
        try:
            self.lib = hip.load()
        finally:
            hip.SIGNATURES.update(new)
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


def tile_pass(B, side, tile=32, rounds=3):
    """fs_gate_tiles against fs_gate_tiles_u8 on the same bytes, alternated."""
    g = torch.Generator(device="cuda").manual_seed(B * 7 + side)
    U = torch.randint(0, 256, (B, 3, side, side), device="cuda", dtype=torch.uint8, generator=g)
    key = torch.randint(0, 256, (B, 3, side, side), device="cuda", dtype=torch.uint8, generator=g)
    X = (U.cpu().float() / 255).cuda()
    T_ = (side + tile - 1) // tile
    sad_f, sad_u = (torch.empty(B, T_, T_, device="cuda", dtype=torch.int32) for _ in range(2))
    px = B * side * side
    out = []
    for _ in range(rounds):
        us_f = event_us(lambda: ops.gate_tiles(X, key, tile, out=sad_f))
        us_u = event_us(lambda: ops.gate_tiles_u8(U, key, tile, out=sad_u))
        out.append({"fp32_us": round(us_f, 2), "u8_us": round(us_u, 2), "fp32_bytes": 15 * px, "u8_bytes": 6 * px,
                    "fp32_TBps": round(15 * px / us_f / 1e6, 3), "u8_TBps": round(6 * px / us_u / 1e6, 3)})
    return {"batch": B, "side": side, "tile": tile, "equal": bool(torch.equal(sad_f, sad_u)), "rounds": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1:1024,64:1024", help="batch:side pairs")
    ap.add_argument("--tile-sizes", default="1:256,64:256", help="batch:side pairs for the tile pass alone")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--motion-px", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frames_u8_bench measures on the GPU"
    hip.load()
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
            X = (U.cpu().float() / 255).cuda()           # the fp32 frame of the same bytes: byte / 255 correctly rounded, as the kernels convert
            mk = lambda **kw: fovealseg.GazeSession(module, B, (side, side), **kw)
            mo = dict(motion_px=args.motion_px)
            sess = {"step_u8": mk(), "step_f32": mk(), "step_convert": mk(), "step_u8_motion": mk(**mo), "step_f32_motion": mk(**mo),
                    "step_convert_motion": mk(**mo)}
            feed = lambda k: U if "_u8" in k else (U.float().div_(255) if "_convert" in k else X)

            def through_parent(fn):
                def run():
                    with parent:
                        return fn()
                return run
            routes = {k: ((lambda k=k: sess[k].step(feed(k), Fp)), False) for k in sess}
            routes["instances_u8"] = (lambda: module.predict_instances(U, Fp, return_bits=True), True)
            routes["instances_f32"] = (lambda: module.predict_instances(X, Fp, return_bits=True), True)
            if parent is not None:
                sess["step_f32_parent"] = mk()
                routes["step_f32_parent"] = (through_parent(lambda: sess["step_f32_parent"].step(X, Fp)), False)
                routes["instances_parent"] = (through_parent(lambda: module.predict_instances(X, Fp, return_bits=True)), True)
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
                        equal &= all(bool(torch.equal(a, b)) for a, b in zip(outs[k][:4], outs["step_f32"][:4]))
                    equal &= all(bool(torch.equal(a, b)) for a, b in zip(outs["instances_u8"], outs["instances_f32"]))
                    if parent is not None:
                        equal &= all(bool(torch.equal(a, b)) for a, b in zip(outs["instances_f32"], outs["instances_parent"]))
                    del outs
                rounds.append({k: stats(v) for k, v in ms.items()})
            inside = lambda r, a, b: r[a]["ms_median"] <= r[b]["ms_max"]
            row = {"batch": B, "side": side, "iters": args.iters, "rounds": rounds, "every_step_reuse": codes_ok, "records_equal": equal,
                   "step_u8_inside_or_below_f32": [inside(r, "step_u8", "step_f32") for r in rounds],
                   "step_u8_motion_inside_or_below_f32": [inside(r, "step_u8_motion", "step_f32_motion") for r in rounds],
                   "convert_minus_u8_ms": [round(r["step_convert"]["ms_median"] - r["step_u8"]["ms_median"], 4) for r in rounds],
                   "convert_minus_u8_motion_ms": [round(r["step_convert_motion"]["ms_median"] - r["step_u8_motion"]["ms_median"], 4) for r in rounds]}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del U, X, Fp, sess, routes
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
