"""What keeping the connected component under the gaze costs on one MI355X.  Eval mode, ops.static_weight_packs (serving), HRNetV2 + C1
(LVIS-50, K = 51), input side^2 -> 80^2 grid -> side^2.  The routes run in ONE process, three rounds, the order changing every iteration:

    instances         module.predict_instances(X, Fp, return_bits=True, return_score=True)
    component         the same with component=8
    instances_parent  (--parent-lib) `instances` through a library built from the parent commit

and ops.mask_component alone on synthetic side^2 masks (a disc, two discs, the head's own mask, the 2-pixel-pitch spiral: the stated
worst case), with the sweeps its grow pass took, against the same selection by a device -> host copy, scipy.ndimage.label and a
re-encode to bit words on the device.

    python tools/component_bench.py [--sizes 1:1024,64:1024] [--warmup 3] [--iters 10] [--parent-lib FILE.so] [--out FILE.json] [--profile]

Every figure is host wall time in ms around a device synchronise.  Per size and round: median (min - max).
--profile: a short run for `rocprofv3 --kernel-trace --stats` (a few predict_instances(component=8) calls per size, no timing).
--summarize DIR: the component kernels of such a run's kernel trace, per kernel and launch size."""
import argparse
import ctypes
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

import instances_bench as IB
from instances_bench import stats

NEW = ("fs_mask_component", "fs_unwarp_instances_component")


class ParentLibrary:
    """A library built from the parent commit (it has none of the component symbols), bound as hip.load() binds this one's; inside a
    `with` every hip.call and every host-side query goes to it."""

    def __init__(self, path):
        own = hip.load()
        lib = ctypes.CDLL(path)
        for name, sig in hip.SIGNATURES.items():
            if name in NEW:
                continue
            fn = getattr(lib, name)
            fn.restype = hip._I
            fn.argtypes = [hip._CT[c] for c in sig] + [hip._P]
        for name in hip.HOST_ONLY:
            if hasattr(lib, name):
                getattr(lib, name).restype = getattr(own, name).restype
                getattr(lib, name).argtypes = getattr(own, name).argtypes
        self.lib, self.cache, self.ws = lib, {}, {}

    def __enter__(self):
        self.keep = (hip._lib, hip._fn_cache, hip._ws_cache)
        hip._lib, hip._fn_cache, hip._ws_cache = self.lib, self.cache, self.ws

    def __exit__(self, *exc):
        hip._lib, hip._fn_cache, hip._ws_cache = self.keep


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spiral(Hs, Ws):
    """A one-pixel-wide rectangular spiral with 2-pixel pitch from (0, 0) inwards, by legs; returns (mask, inner end)."""
    m = np.zeros((Hs, Ws), dtype=bool)
    top, left, bottom, right = 0, 0, Hs - 1, Ws - 1
    y = x = 0
    while True:
        if right < left:
            break
        m[top, left:right + 1] = True; y, x = top, right
        if bottom - top < 2:
            break
        m[top:bottom + 1, right] = True; y, x = bottom, right
        if right - left < 2:
            break
        m[bottom, left:right + 1] = True; y, x = bottom, left
        if bottom - top < 4:
            break
        m[top + 2:bottom + 1, left] = True; y, x = top + 2, left
        if right - left < 4:
            break
        top, bottom, right = top + 2, bottom - 2, right - 2
        m[top, left:left + 3] = True
        left += 2
    return m, (y, x)


def focus_at(py, px, Hs, Ws):
    return [py / (Hs - 1), px / (Ws - 1)]


def component_with_sweeps(bits, focus, Ws, conn=8):
    """fs_mask_component with the scratch in hand: (bits_c, comp, sweeps (B,)).  The sweep count is a diagnostic the grow kernel
    leaves in the third int of an image's seed record (csrc/mask_component.hip: COMP_REC); it is no part of the C ABI."""
    B, Hs, P = bits.shape
    out = torch.empty_like(bits)
    comp = torch.empty(B, 4, device=bits.device, dtype=torch.int64)
    scratch = torch.zeros(hip.query("fs_mask_component_scratch_ints", B, Hs, Ws), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_component", hip.ptr(bits), hip.ptr(focus), hip.ptr(out), hip.ptr(comp), hip.ptr(scratch), B, Hs, Ws, conn, 2 ** 62)
    return out, comp, scratch.view(B, -1)[:, 2]


def host_route(bits, focus_px, Ws):
    """The same selection off the device: copy the words, unpack, scipy.ndimage.label (8-connected), keep the label under the gaze
    pixel (the synthetic gazes lie on the mask), pack, copy back."""
    from scipy import ndimage
    w = bits.cpu().numpy().view(np.uint32)
    out = np.zeros_like(w)
    for b in range(w.shape[0]):
        m = ((w[b][:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[1], -1).astype(bool)[:, :Ws]
        lab, _ = ndimage.label(m, structure=np.ones((3, 3), dtype=int))
        py, px = focus_px[b]
        c = (lab == lab[py, px]) & m
        pad = np.zeros((c.shape[0], w.shape[2] * 32), dtype=np.uint64)
        pad[:, :Ws] = c
        out[b] = (pad.reshape(c.shape[0], -1, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
    return torch.from_numpy(out.view(np.int32)).to(bits.device)


def synthetic(side):
    yy, xx = np.mgrid[:side, :side]
    r = side // 5
    disc = (yy - side // 2) ** 2 + (xx - side // 2) ** 2 <= r * r
    two = ((yy - side // 3) ** 2 + (xx - side // 3) ** 2 <= (r // 2) ** 2) | ((yy - 2 * side // 3) ** 2 + (xx - 2 * side // 3) ** 2 <= r * r)
    sp, end = spiral(side, side)
    return {"disc": (disc, (side // 2, side // 2)), "two_discs": (two, (side // 3, side // 3)), "spiral": (sp, end)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1:1024,64:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--skip-host", action="store_true", help="leave the scipy route out")
    args = ap.parse_args()
    if args.summarize:
        IB.KERNELS = ("component_seed", "component_grow", "component_qsum", "unwarp_bits", "rle_walk", "rle_scan", "instance_conf", "head_fg_q")
        return IB.summarize(args.summarize)
    assert torch.cuda.is_available(), "component_bench measures on the GPU"
    hip.load()
    cfg = fovealseg.lvis50_cfg()
    module, _ = T.build_module(cfg, device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    with torch.no_grad():
        module.decoder.cls_net.fc.bias[-1] += 1000.0                                   # the mask plane draws the blob (gaze_session_bench)
    parent = ParentLibrary(args.parent_lib) if args.parent_lib else None
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(),
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> side^2", "sizes": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            X, Fp, _, _ = T.synthetic_batch(B, side, side, seed=1, device="cuda")

            def instances_parent():
                with parent:
                    return module.predict_instances(X, Fp, return_bits=True, return_score=True)
            routes = {"instances": lambda: module.predict_instances(X, Fp, return_bits=True, return_score=True),
                      "component": lambda: module.predict_instances(X, Fp, return_bits=True, return_score=True, component=8)}
            if parent is not None:
                routes["instances_parent"] = instances_parent
            head = routes["instances"]()
            masks = {k: (torch.from_numpy(np.broadcast_to(m, (B,) + m.shape).copy()).cuda(), px) for k, (m, px) in synthetic(side).items()}
            bitsets = {k: (ops.mask_bits(m), torch.tensor([focus_at(*px, side, side)] * B, device="cuda", dtype=torch.float32), [px] * B)
                       for k, (m, px) in masks.items()}
            first = routes["component"]()
            seeds = first[-1][:, :2].tolist()
            bitsets["head"] = (head[3], Fp.float().contiguous(), None)
            if args.profile:
                for _ in range(3):                                                     # the head's own mask: the kernels of the served path
                    routes["component"]()
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            perms = list(itertools.permutations(routes))
            rounds, equal = [], True
            for _ in range(3):
                ms = {k: [] for k in routes}
                for it in range(args.iters):
                    outs = {}
                    for k in perms[(7 * it) % len(perms)]:                             # another order every iteration
                        t, outs[k] = wall(routes[k])
                        ms[k].append(t)
                    if parent is not None:
                        equal &= all(bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                      b.view(torch.int32) if b.dtype == torch.float32 else b))
                                     for a, b in zip(outs["instances"], outs["instances_parent"]))
                    del outs
                rounds.append({k: stats(v) for k, v in ms.items()})
            module.check_nan()
            alone = {}
            for k, (bits, f, px) in bitsets.items():
                out, comp, sweeps = component_with_sweeps(bits, f, side)
                for _ in range(args.warmup):
                    ops.mask_component(bits, f, Ws=side)
                t = [wall(lambda: ops.mask_component(bits, f, Ws=side))[0] for _ in range(args.iters)]
                alone[k] = {"device": stats(t), "sweeps_min_max": [int(sweeps.min()), int(sweeps.max())], "area_in": int(comp[0, 3]),
                            "area_component": int(ops.mask_rle(out, side)[0][0, 0])}
                if not args.skip_host and px is not None and (B == 1 or k == "disc"):
                    th = [wall(lambda: host_route(bits, px, side)) for _ in range(3)]
                    alone[k]["host_scipy"] = stats([v[0] for v in th])
                    alone[k]["host_equals_device"] = bool(torch.equal(th[0][1], out))
            row = {"batch": B, "side": side, "iters": args.iters, "rounds": rounds, "instances_equal_parent_bit_for_bit": equal if parent else None,
                   "component_minus_instances_ms": [round(r["component"]["ms_median"] - r["instances"]["ms_median"], 3) for r in rounds],
                   "areas_first_images": {"head": head[1][:4, 0].tolist(), "component": first[1][:4, 0].tolist(), "seeds": seeds[:4]},
                   "mask_component_alone": alone}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp, head, first, masks, bitsets
            torch.cuda.empty_cache()
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
