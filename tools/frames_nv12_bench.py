"""What reading NV12 decoder frames in place costs and saves on one MI355X.  Eval mode, ops.static_weight_packs (serving), HRNetV2 + C1
(LVIS-50, K = 51), input side^2 -> 80^2 grid -> side^2.  All routes run in ONE process, three rounds, the order changing every iteration:

    step_planar               session().step on an unchanged frame and gaze (REUSE), fed the planar uint8 frame ops.nv12_to_rgb makes
    step_nv12                 the same picture as an ops.Nv12Frame, read where it lies
    step_convert              what a caller with such a surface paid before: ops.nv12_to_rgb, then the planar step
    *_motion                  the same with motion_px=16
    instances_planar / _nv12  module.predict_instances(frame, Fp, return_bits=True)

    python tools/frames_nv12_bench.py [--sizes 1:1024,64:1024] [--warmup 3] [--iters 10] [--out FILE.json]
    python tools/frames_nv12_bench.py --tiles-only [--tile-sizes 64:1024]

Route figures are host wall time in ms, median (min - max) per round; a step ends with its own read-back, the other routes with a device
synchronise.  "tiles" are device-event times over 20 back-to-back calls of the tile pass, alternated over three rounds, in microseconds a
call, with the bytes each must read and write a pixel and the rate in TB/s on those bytes: fs_gate_tiles_u8 on the planar frame (6 B);
fs_gate_tiles_nv12 in its 16-pixel form and, on a luma view one byte off its alignment, in its one-pixel form (4.5 B); fs_nv12_to_rgb
followed by fs_gate_tiles_u8 (1.5 + 3 + 6 B); a torch expression of the same integer rule followed by fs_gate_tiles_u8."""
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


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def planes_of(U):
    """NV12 planes (bt601 limited, a block's top-left chroma) whose picture resembles the uint8 frame U."""
    r, g, b = (U[:, c].float() for c in range(3))
    to8 = lambda v: v.round().clamp(0, 255).to(torch.uint8)
    y = to8(16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255)
    u = to8(128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255)
    v = to8(128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255)
    return y.contiguous(), torch.stack([u[:, ::2, ::2], v[:, ::2, ::2]], dim=-1).contiguous()


def torch_rgb(y, uv, csc):
    """The definition's integer rule in torch: what a caller without fs_nv12_to_rgb writes."""
    yo, yg, rv, gu, gv, bu = csc
    H, W = y.shape[1:]
    up = lambda c: c.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W].int() - 128
    D, E = up(uv[..., 0]), up(uv[..., 1])
    l = yg * (y.int() - yo) + 128
    return torch.stack([((l + rv * E) >> 8), ((l + gu * D + gv * E) >> 8), ((l + bu * D) >> 8)], dim=1).clamp_(0, 255).to(torch.uint8)


def tile_pass(B, side, tile=32, rounds=3):
    g = torch.Generator(device="cuda").manual_seed(B * 7 + side)
    rnd = lambda *s: torch.randint(0, 256, s, device="cuda", dtype=torch.uint8, generator=g)
    y, uv, key = rnd(B, side, side), rnd(B, (side + 1) // 2, (side + 1) // 2, 2), rnd(B, 3, side, side)
    f = ops.Nv12Frame(y, uv, matrix="bt601")
    y1 = torch.empty(y.numel() + 16, device="cuda", dtype=torch.uint8)[1:1 + y.numel()].view_as(y)
    y1.copy_(y)
    f1 = ops.Nv12Frame(y1, uv, matrix="bt601")
    U = ops.nv12_to_rgb(f)
    assert torch.equal(U, torch_rgb(y, uv, f.csc))
    T_ = (side + tile - 1) // tile
    names = ("planar", "nv12", "nv12_px", "convert", "torch")
    sad = {k: torch.empty(B, T_, T_, device="cuda", dtype=torch.int32) for k in names}
    tmp = torch.empty_like(U)
    px = B * side * side
    calls = {"planar": (lambda: ops.gate_tiles_u8(U, key, tile, out=sad["planar"]), 6),
             "nv12": (lambda: ops.gate_tiles_u8(f, key, tile, out=sad["nv12"]), 4.5),
             "nv12_px": (lambda: ops.gate_tiles_u8(f1, key, tile, out=sad["nv12_px"]), 4.5),
             "convert": (lambda: ops.gate_tiles_u8(ops.nv12_to_rgb(f, out=tmp), key, tile, out=sad["convert"]), 10.5),
             "torch": (lambda: ops.gate_tiles_u8(torch_rgb(y, uv, f.csc), key, tile, out=sad["torch"]), 10.5)}
    out = []
    for _ in range(rounds):
        row = {}
        for k, (fn, bpp) in calls.items():
            us = event_us(fn)
            row[k + "_us"], row[k + "_TBps"] = round(us, 2), round(bpp * px / us / 1e6, 3)
        out.append(row)
    spread = lambda k: (min(r[k + "_us"] for r in out), max(r[k + "_us"] for r in out))
    return {"batch": B, "side": side, "tile": tile, "routes": [f.route(), f1.route()], "bytes_per_pixel": {k: v[1] for k, v in calls.items()},
            "equal": all(bool(torch.equal(sad["planar"], v)) for v in sad.values()), "rounds": out,
            "nv12_beats_nv12_px_outside_the_spread": spread("nv12")[1] < spread("nv12_px")[0],
            "nv12_beats_convert_outside_the_spread": spread("nv12")[1] < spread("convert")[0],
            "nv12_beats_planar_outside_the_spread": spread("nv12")[1] < spread("planar")[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1:1024,64:1024", help="batch:side pairs")
    ap.add_argument("--tile-sizes", default="", help="batch:side pairs for the tile pass alone")
    ap.add_argument("--tiles-only", action="store_true", help="no network: the tile pass of --tile-sizes (default 64:1024) and nothing else")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--motion-px", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frames_nv12_bench measures on the GPU"
    hip.load()
    res = {"device": torch.cuda.get_device_name(0), "motion_px": args.motion_px, "sizes": [], "tiles": []}
    if not args.tiles_only:
        module, _ = T.build_module(fovealseg.lvis50_cfg(), device="cuda")
        module.eval()
        ops.static_weight_packs(module)
        with torch.no_grad():                            # as gaze_session_bench: a large background logit lets the mask plane draw a blob
            module.decoder.cls_net.fc.bias[-1] += 1000.0
        res["conv_precision"] = hip.get_conv_precision()
    with torch.no_grad():
        for spec in ([] if args.tiles_only else args.sizes.split(",")):
            B, side = (int(v) for v in spec.split(":"))
            X0, Fp, _Y, _cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            y, uv = planes_of((X0.clamp(0, 1) * 255).round().to(torch.uint8))
            del X0, _Y
            f = ops.Nv12Frame(y, uv, matrix="bt601")
            U = ops.nv12_to_rgb(f)
            tmp = torch.empty_like(U)
            mk = lambda **kw: fovealseg.GazeSession(module, B, (side, side), **kw)
            sess, routes = {}, {}
            for tail, kw in (("", {}), ("_motion", dict(motion_px=args.motion_px))):
                for name, frame in (("planar", lambda: U), ("nv12", lambda: f), ("convert", lambda: ops.nv12_to_rgb(f, out=tmp))):
                    k = "step_" + name + tail
                    sess[k] = mk(**kw)
                    routes[k] = ((lambda k=k, frame=frame: sess[k].step(frame(), Fp)), False)
            routes["instances_planar"] = (lambda: module.predict_instances(U, Fp, return_bits=True), True)
            routes["instances_nv12"] = (lambda: module.predict_instances(f, Fp, return_bits=True), True)
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
                    equal &= all(bool(torch.equal(a, b)) for a, b in zip(outs["instances_nv12"], outs["instances_planar"]))
                    del outs
                rounds.append({k: stats(v) for k, v in ms.items()})
            diff = lambda a, b: [round(r[a]["ms_median"] - r[b]["ms_median"], 4) for r in rounds]
            row = {"batch": B, "side": side, "iters": args.iters, "rounds": rounds, "every_step_reuse": codes_ok, "records_equal": equal,
                   "convert_minus_nv12_ms": diff("step_convert", "step_nv12"), "convert_minus_nv12_motion_ms": diff("step_convert_motion", "step_nv12_motion"),
                   "nv12_minus_planar_ms": diff("step_nv12", "step_planar"), "nv12_minus_planar_motion_ms": diff("step_nv12_motion", "step_planar_motion"),
                   "instances_nv12_minus_planar_ms": diff("instances_nv12", "instances_planar")}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del U, y, uv, f, tmp, Fp, sess, routes
            torch.cuda.empty_cache()
            res["tiles"].append(tile_pass(B, side))
            print(json.dumps(res["tiles"][-1]), flush=True)
        for spec in filter(None, (args.tile_sizes or ("64:1024" if args.tiles_only else "")).split(",")):
            B, side = (int(v) for v in spec.split(":"))
            res["tiles"].append(tile_pass(B, side))
            print(json.dumps(res["tiles"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f_:
            json.dump(res, f_, indent=1)


if __name__ == "__main__":
    main()
