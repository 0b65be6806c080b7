"""What the trimap boundary accuracy costs on one MI355X: DeformSegmentationModule.evaluate() against evaluate(trimap=5), against
evaluate() through the parent commit's fs_unwarp_accuracy, and against predict() followed by the same bands made in torch (a cross
dilation by max-pooling, iterated 2**D times) and a torch count -- in ONE process, alternating the routes per iteration (in another order every
iteration) after a warm-up of each.  Eval mode, ops.static_weight_packs, HRNetV2 + C1 (LVIS-50, K = 51).

    python tools/trimap_bench.py [--sizes 64:1024,1:1024] [--warmup 3] [--iters 10] [--parent-lib FILE.so] [--out FILE.json] [--profile]

--parent-lib: a libfovealseg_hip.so built from the parent commit; the `evaluate_parent` route then runs evaluate() with that library's
fs_unwarp_accuracy in place of this one's (every other kernel of the call is the same code in both), so that the default path can be
held against the parent's own run-to-run spread in the same run.
Per size: median / min / max ms per call of each route; trim of the fused and the torch route compared with torch.equal; and the band
kernels alone (ops.trimap_bands, device events around `--band-reps` calls) against the bytes they must move -- y read once, one byte
written, the row pass's byte written and read -- beside a device-to-device copy of y on the same box.
--profile: a short run for `rocprofv3 --kernel-trace --stats` (two calls of evaluate(trimap=5), no timing)."""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

K, D = 51, 5


def torch_bands(Y, frame=True):
    """ops.trimap_bands in torch: seeds by a 3x3 max-pool, then 2**D cross dilations (max of a 3x1 and a 1x3 max-pool)."""
    fg = (Y.long() != 0).float()
    seed = (1 - fg) * F.max_pool2d(fg, 3, 1, 1)
    if frame:
        ring = torch.zeros_like(fg)
        ring[..., 0, :] = ring[..., -1, :] = 1
        ring[..., :, 0] = ring[..., :, -1] = 1
        seed = torch.where(ring > 0, 1 - fg, seed)
    band = torch.full(fg.shape, 255, device=Y.device, dtype=torch.uint8)
    cur, nxt = seed, 0
    for n in range(1, 2 ** D + 1):
        cur = torch.maximum(F.max_pool2d(cur, (3, 1), 1, (1, 0)), F.max_pool2d(cur, (1, 3), 1, (0, 1)))
        if n == 2 ** nxt:
            band = torch.where((band == 255) & (cur > 0), torch.full_like(band, nxt), band)
            nxt += 1
    return band[:, 0]


def predict_torch(module, X, Fp, Y, cl):
    a = module.predict(X, Fp)
    band = torch_bands(Y)
    t = Y[:, 0].long()
    g = t * cl[:, :, None] + (1 - t) * (K - 1)
    eq, side = a == g, (a == K - 1) == (g == K - 1)
    rows = []
    for i in range(D + 1):
        inb = band <= i
        rows.append(torch.stack([inb.flatten(1).sum(1), (inb & eq).flatten(1).sum(1), (inb & side).flatten(1).sum(1)], 1))
    return torch.stack(rows, 1)


class ParentAccuracy:
    """Swaps the parent library's fs_unwarp_accuracy into hip.call for the duration of a `with`."""

    def __init__(self, path):
        self.fn = ctypes.CDLL(path).fs_unwarp_accuracy
        self.fn.restype = ctypes.c_int
        self.fn.argtypes = [hip._CT[c] for c in hip.SIGNATURES["fs_unwarp_accuracy"]] + [hip._P]
        self.own = hip.load().fs_unwarp_accuracy

    def __enter__(self):
        hip._fn_cache["fs_unwarp_accuracy"] = self.fn

    def __exit__(self, *exc):
        hip._fn_cache["fs_unwarp_accuracy"] = self.own


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64:1024,1:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--band-reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "trimap_bench measures on the GPU"
    hip.load()
    module, _ = T.build_module(fovealseg.lvis50_cfg(), device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    parent = ParentAccuracy(args.parent_lib) if args.parent_lib else None

    def evaluate_parent():
        with parent:
            return module.evaluate(X, Fp, Y, cl)
    routes = {"evaluate": lambda: module.evaluate(X, Fp, Y, cl)}
    if parent is not None:
        routes["evaluate_parent"] = evaluate_parent
    routes["evaluate_trimap"] = lambda: module.evaluate(X, Fp, Y, cl, trimap=D)
    routes["predict_torch_bands"] = lambda: predict_torch(module, X, Fp, Y, cl)
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(), "dia_factor": D,
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> scores at side^2", "sizes": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            X, Fp, Y, cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            if args.profile:
                for _ in range(2):
                    routes["evaluate_trimap"]()
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            ms = {k: [] for k in routes}
            equal = True
            perms = list(itertools.permutations(routes))
            for it in range(args.iters):
                outs = {}
                for k in perms[(7 * it) % len(perms)]:                                 # another order every iteration
                    t, outs[k] = timed(routes[k])
                    ms[k].append(t)
                equal &= bool(torch.equal(outs["evaluate_trimap"][5], outs["predict_torch_bands"]))
                equal &= all(torch.equal(a, b) for a, b in zip(outs["evaluate"], outs["evaluate_trimap"][:5]))
                if parent is not None:
                    equal &= all(torch.equal(a, b) for a, b in zip(outs["evaluate"], outs["evaluate_parent"]))
                del outs
            module.check_nan()
            row = {"batch": B, "side": side, "iters": args.iters, "results_equal": equal}
            for k in routes:
                row[k] = {"ms_median": round(statistics.median(ms[k]), 3), "ms_min": round(min(ms[k]), 3), "ms_max": round(max(ms[k]), 3)}
            if parent is not None:
                # the default path against the parent's, the two alone: A B B A ..., so that neither always follows the other
                ab = {"evaluate": [], "evaluate_parent": []}
                for it in range(2 * args.iters):
                    for k in (("evaluate", "evaluate_parent") if it % 2 == 0 else ("evaluate_parent", "evaluate")):
                        ab[k].append(timed(routes[k])[0])
                row["default_vs_parent_abba"] = {k: {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3),
                                                     "ms_max": round(max(v), 3)} for k, v in ab.items()}
            row["trimap_adds_ms"] = round(row["evaluate_trimap"]["ms_median"] - row["evaluate"]["ms_median"], 3)
            row["torch_route_adds_ms"] = round(row["predict_torch_bands"]["ms_median"] - row["evaluate"]["ms_median"], 3)
            # the band kernels alone, and a copy of y for the box's copy rate
            y3 = Y[:, 0].contiguous()
            dst = torch.empty_like(y3)
            for _ in range(3):
                ops.trimap_bands(y3, D)
                dst.copy_(y3)

            def reps(fn):
                def run():
                    for _ in range(args.band_reps):
                        fn()
                return timed(run)[0] / args.band_reps
            band_ms = [reps(lambda: ops.trimap_bands(y3, D)) for _ in range(3)]
            copy_ms = [reps(lambda: dst.copy_(y3)) for _ in range(3)]
            n = B * side * side
            band_bytes, copy_bytes = n * (4 + 1 + 1 + 1), n * 8
            row["band_kernels"] = {"ms": [round(v, 4) for v in band_ms], "bytes": band_bytes,
                                   "GB_per_s": round(band_bytes / (min(band_ms) * 1e-3) / 1e9, 1)}
            row["copy_of_y"] = {"ms": [round(v, 4) for v in copy_ms], "bytes": copy_bytes,
                                "GB_per_s": round(copy_bytes / (min(copy_ms) * 1e-3) / 1e9, 1)}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp, Y, cl, y3, dst
            torch.cuda.empty_cache()
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
