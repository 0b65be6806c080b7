"""What GazeSession(motion_px=...) costs and saves on one MI355X.  Eval mode, ops.static_weight_packs (serving), HRNetV2 + C1 (LVIS-50,
K = 51), input side^2 -> 80^2 grid -> side^2.  All routes run in ONE process, three rounds, the order changing every iteration:

    still_motion      session(motion_px=16).step on an unchanged frame and gaze
    still_plain       session().step on the same: the REUSE step without the keyword
    moved_reuse       session(motion_px=16).step on a stream whose window moves by +-(3, 5) every frame, the gaze with it
    run_scene         session().step on that stream: RUN_SCENE every frame, the step that moved_reuse replaces
    instances         module.predict_instances(X, Fp, return_bits=True)
    *_parent          (--parent-lib) still_plain and instances through a library built from the parent commit

    python tools/motion_bench.py [--sizes 1:1024,64:1024] [--warmup 3] [--iters 10] [--parent-lib FILE.so] [--out FILE.json]

Route figures are host wall time in ms, median (min - max) per round; a step ends with its own read-back, the other routes with a device
synchronise.  "launches" are device-event times over 20 back-to-back calls of one op, in microseconds a call, and the two hot passes'
rates in TB/s from the bytes they must read (frame_profiles 12 B a pixel, gate_tiles 15 B a pixel)."""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import torch.nn.functional as F

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

from gaze_session_bench import wall
from instances_bench import stats

NEW = ("fs_frame_profiles", "fs_key_profiles", "fs_profile_shift", "fs_state_shift", "fs_motion_commit")
PAD, SCALE, MOVE = 8, 4, (3, 5)


class ParentLibrary:
    """A library built from the parent commit, bound like this one's without the motion entry points; inside a `with` every hip.call
    goes to it."""

    def __init__(self, path):
        own_lib, own_path, own_env = hip._lib, hip.LIB_PATH, os.environ.get("FS_HIP_LIB")
        new = {k: hip.SIGNATURES.pop(k) for k in NEW}
        host = hip.HOST_ONLY.pop("fs_state_shift_scratch_ints")
        os.environ["FS_HIP_LIB"], hip.LIB_PATH, hip._lib = path, path, None
        try:
            self.lib = hip.load()
        finally:
            hip.SIGNATURES.update(new)
            hip.HOST_ONLY["fs_state_shift_scratch_ints"] = host
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


def textured_stream(B, side, seed):
    """Two frames per viewer, windows of a box-filtered noise canvas MOVE apart, and the gazes that go with them."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    big = side + 2 * PAD
    frames = torch.empty(2, B, 3, side, side, device="cuda")
    for b in range(B):                                   # a viewer at a time: the canvas of a whole batch would not fit beside the frames
        c = F.avg_pool2d(torch.rand(1, 3, big + SCALE - 1, big + SCALE - 1, device="cuda", generator=g), SCALE, 1)[0]
        c = (c - c.min()) / (c.max() - c.min())
        frames[0, b] = c[:, PAD:PAD + side, PAD:PAD + side]
        frames[1, b] = c[:, PAD - MOVE[0]:PAD - MOVE[0] + side, PAD - MOVE[1]:PAD - MOVE[1] + side]
    py, px = side // 2, side // 2
    focus = torch.tensor([[[py / (side - 1), px / (side - 1)]] * B, [[(py + MOVE[0]) / (side - 1), (px + MOVE[1]) / (side - 1)]] * B], device="cuda")
    return frames, focus


def event_us(fn, n=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def launches(s, X, B, side):
    """Device time of each new launch group on a still stream, on the session's own tensors."""
    sad = torch.empty(B, s.th, s.tw, device="cuda", dtype=torch.int32)
    us = {"frame_profiles": event_us(lambda: ops.frame_profiles(X, out=s._prof)),
          "gate_tiles": event_us(lambda: ops.gate_tiles(X, s._key, s.tile, out=sad)),
          "profile_shift": event_us(lambda: ops.profile_shift(s._prof, s._prof_key, s._gstate, (side, side), s.motion_px, s.motion_gain, out=s._shift)),
          "state_shift_still": event_us(lambda: ops.state_shift(X, s._shift, s._key, s._key2, s._rec[3], s._bits2, s._gstate, s._rec[1], s._rec[2],
                                                                s._prof_key, s._mstate, motion=s._motion, scratch=s._scratch)),
          "mask_rle_alone": event_us(lambda: ops.mask_rle(s._rec[3], side))}
    px = B * side * side
    return {"us": {k: round(v, 2) for k, v in us.items()},
            "frame_profiles_TBps": round(12 * px / us["frame_profiles"] / 1e6, 3), "gate_tiles_TBps": round(15 * px / us["gate_tiles"] / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1:1024,64:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--motion-px", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "motion_bench measures on the GPU"
    hip.load()
    module, _ = T.build_module(fovealseg.lvis50_cfg(), device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    with torch.no_grad():                                # as gaze_session_bench: a large background logit lets the mask plane draw a blob
        module.decoder.cls_net.fc.bias[-1] += 1000.0
    parent = ParentLibrary(args.parent_lib) if args.parent_lib else None
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(), "motion_px": args.motion_px, "sizes": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            frames, focus = textured_stream(B, side, seed=1)
            X, Fp = frames[0], focus[0]
            mk = lambda **kw: fovealseg.GazeSession(module, B, (side, side), **kw)
            sess = {"still_motion": mk(motion_px=args.motion_px), "still_plain": mk(), "moved_reuse": mk(motion_px=args.motion_px), "run_scene": mk()}
            turn = {"moved_reuse": 0, "run_scene": 0}

            def moving(k):
                turn[k] ^= 1
                return sess[k].step(frames[turn[k]], focus[turn[k]])

            def through_parent(fn):
                def run():
                    with parent:
                        return fn()
                return run
            routes = {"still_motion": (lambda: sess["still_motion"].step(X, Fp), False), "still_plain": (lambda: sess["still_plain"].step(X, Fp), False),
                      "moved_reuse": (lambda: moving("moved_reuse"), False), "run_scene": (lambda: moving("run_scene"), True),
                      "instances": (lambda: module.predict_instances(X, Fp, return_bits=True), True)}
            if parent is not None:
                sess["still_plain_parent"] = mk()
                routes["still_plain_parent"] = (through_parent(lambda: sess["still_plain_parent"].step(X, Fp)), False)
                routes["instances_parent"] = (through_parent(lambda: module.predict_instances(X, Fp, return_bits=True)), True)
            for k, s in sess.items():                    # every record is made from frame 0
                fn = through_parent(lambda: s.step(X, Fp)) if k.endswith("_parent") else (lambda: s.step(X, Fp))
                assert fn()[len(s._rec)][:, 0].tolist() == [1] * B
            for _ in range(args.warmup):
                for fn, _sync in routes.values():
                    fn()
            perms = list(itertools.permutations(routes))
            rounds, codes_ok, shifts_ok, equal = [], True, True, True
            for _ in range(3):
                ms = {k: [] for k in routes}
                for it in range(args.iters):
                    outs = {}
                    for k in perms[(997 * it + 131) % len(perms)]:     # a stride that changes the head of the order too
                        t, outs[k] = wall(*routes[k])
                        ms[k].append(t)
                    torch.cuda.synchronize()
                    sign = 1 if turn["moved_reuse"] else -1
                    codes_ok &= all(outs[k][-2][:, 0].tolist() == [0] * B for k in ("still_motion", "moved_reuse"))
                    codes_ok &= outs["still_plain"][-1][:, 0].tolist() == [0] * B and outs["run_scene"][-1][:, 0].tolist() == [3] * B
                    shifts_ok &= outs["moved_reuse"][-1][:, :2].tolist() == [[sign * MOVE[0], sign * MOVE[1]]] * B
                    shifts_ok &= outs["still_motion"][-1][:, :2].tolist() == [[0, 0]] * B
                    if parent is not None:
                        equal &= all(bool(torch.equal(a, b)) for a, b in zip(outs["instances"][:4], outs["instances_parent"][:4]))
                        equal &= all(bool(torch.equal(a, b)) for a, b in zip(outs["still_plain"][:4], outs["still_plain_parent"][:4]))
                    del outs
                rounds.append({k: stats(v) for k, v in ms.items()})
            med = lambda r, k: r[k]["ms_median"]
            row = {"batch": B, "side": side, "iters": args.iters, "rounds": rounds, "codes_as_expected": codes_ok, "shifts_as_expected": shifts_ok,
                   "parent_records_equal": equal if parent is not None else None,
                   "still_motion_minus_plain_ms": [round(med(r, "still_motion") - med(r, "still_plain"), 4) for r in rounds],
                   "run_scene_over_moved_reuse": [round(med(r, "run_scene") / med(r, "moved_reuse"), 2) for r in rounds],
                   "launches": launches(sess["still_motion"], X, B, side)}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del frames, focus, X, Fp, sess, routes
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
