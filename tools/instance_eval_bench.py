"""What scoring an instance record costs on one MI355X: fs_mask_erode and fs_mask_pair_counts alone on three kinds of mask, against
the same six counters made by torch on zero-padded float masks (`-max_pool2d(-m)` with a 2d+1 window) -- a cross check as well: the
two routes must give the same integers -- then DeformSegmentationModule.evaluate_instances() against predict_instances(return_bits=True,
return_score=True), and predict_instances() through the parent commit's library against this one's.  Everything runs in ONE process,
the routes alternating, in three rounds.

    python tools/instance_eval_bench.py [--sizes 1:1024,64:1024] [--warmup 3] [--iters 10] [--op-reps 20] [--parent-lib FILE.so] [--out FILE.json]

--parent-lib: a libfovealseg_hip.so built from the parent commit (build.py on a checkout of it).  The bench binds every entry point
the parent has from that file and puts it under hip.call and hip.query for the duration of a call, so that predict_instances() runs
once through each library inside one process (no existing kernel or launch changes in this commit: the two are expected inside each
other's spread)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T


NEW = ("fs_mask_erode", "fs_mask_pair_counts")           # what the parent's library does not have


class ParentLibrary:
    """A library built from the parent commit, bound as hip.load() binds this one's; inside a `with` every hip.call and every
    host-side query goes to it (tools/component_bench.py)."""

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


def timed(fn, reps=1):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def peak_over_start(fn):
    """Bytes the call's peak allocation lies above what was allocated when it began."""
    torch.cuda.synchronize()
    start = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - start


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def torch_pair(a, b, d):
    """The six counters from float masks: erosion as -max_pool2d(-m) over a zero-padded copy, eight images at a time (the padded
    fp32 copy and the pooled one are 8 bytes a pixel and mask)."""
    out = []
    for lo in range(0, a.shape[0], 8):
        m = torch.stack([a[lo:lo + 8], b[lo:lo + 8]], 1).float()                         # (b, 2, H, W)
        er = -F.max_pool2d(-F.pad(m, (d, d, d, d)), 2 * d + 1, stride=1)
        band = m * (1 - er)
        out.append(torch.stack([(m[:, 0] * m[:, 1]).sum((1, 2)), m[:, 0].sum((1, 2)), m[:, 1].sum((1, 2)),
                                (band[:, 0] * band[:, 1]).sum((1, 2)), band[:, 0].sum((1, 2)), band[:, 1].sum((1, 2))], 1).double())
    return torch.cat(out).long()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1:1024,64:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--op-reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "instance_eval_bench measures on the GPU"
    hip.load()
    module, _ = T.build_module(fovealseg.lvis50_cfg(), device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    with torch.no_grad():
        module.decoder.cls_net.fc.bias[-1] += 1000.0     # a large background logit lets the mask plane draw a blob (tools/component_bench.py)
    parent = ParentLibrary(args.parent_lib) if args.parent_lib else None
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(),
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> record at side^2", "sizes": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            d = ops.boundary_dilation(side, side)
            X, Fp, Y, cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            label = Y[:, 0] != 0                                                          # the disc at the gaze
            head = module.predict_instances(X, Fp, return_bits=True)[3]
            P = head.shape[2]
            shift = torch.roll(label, (side // 50, side // 70), (1, 2))
            kinds = {"disc": (ops.mask_bits(shift), ops.mask_bits(label)), "head": (head, ops.mask_bits(label)),
                     "full": (torch.full_like(head, -1), torch.full_like(head, -1))}
            row = {"batch": B, "side": side, "d": d, "op_alone": {}}
            out = torch.empty(B, side, P, device="cuda", dtype=torch.int32)
            pair = torch.empty(B, 6, device="cuda", dtype=torch.int64)
            scr_e = torch.empty(hip.query("fs_mask_erode_scratch_ints", B, side, side, d), device="cuda", dtype=torch.int32)
            scr_p = torch.empty(hip.query("fs_mask_pair_scratch_ints", B, side, side, d), device="cuda", dtype=torch.int32)
            for name, (a, b) in kinds.items():
                def erode():
                    hip.call("fs_mask_erode", a.data_ptr(), out.data_ptr(), scr_e.data_ptr(), B, side, side, d)

                def counts():
                    hip.call("fs_mask_pair_counts", a.data_ptr(), b.data_ptr(), pair.data_ptr(), scr_p.data_ptr(), B, side, side, d)
                am, bm = (torch.from_numpy(np.unpackbits(t.cpu().numpy().view(np.uint8), axis=-1, bitorder="little")).bool()[:, :, :side].cuda()
                          for t in (a, b))
                erode(), counts(), torch_pair(am[:1], bm[:1], d)
                entry = {"fs_mask_erode_ms": [round(timed(erode, args.op_reps)[0], 4) for _ in range(3)],
                         "fs_mask_pair_counts_ms": [round(timed(counts, args.op_reps)[0], 4) for _ in range(3)],
                         "torch_float_ms": [round(timed(lambda: torch_pair(am, bm, d))[0], 3) for _ in range(2)],
                         "pair_first_image": pair[0].tolist(), "scratch_bytes": scr_p.numel() * 4,
                         "peak_bytes_over_start": {"mask_pair_counts": peak_over_start(lambda: ops.mask_pair_counts(a, b, d, Ws=side)),
                                                   "torch_float": peak_over_start(lambda: torch_pair(am, bm, d))}}
                entry["torch_agrees"] = bool(torch.equal(torch_pair(am, bm, d), pair))
                row["op_alone"][name] = entry
                del am, bm
            del out, scr_e, scr_p, kinds
            routes = {"predict_instances": lambda: module.predict_instances(X, Fp, return_bits=True, return_score=True),
                      "evaluate_instances": lambda: module.evaluate_instances(X, Fp, Y, cl)}
            if parent is not None:
                def through_parent():
                    with parent:
                        return module.predict_instances(X, Fp, return_bits=True, return_score=True)
                routes["predict_instances_parent"] = through_parent
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            names = list(routes)
            rounds = []
            for _ in range(3):
                ms = {k: [] for k in names}
                for it in range(args.iters):
                    for k in (names if it % 2 == 0 else names[::-1]):                      # neither always follows the other
                        ms[k].append(timed(routes[k])[0])
                rounds.append({k: stats(v) for k, v in ms.items()})
            module.check_nan()
            row["rounds"] = rounds
            a, b = routes["predict_instances"](), routes["evaluate_instances"]()
            row["results_equal"] = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                   y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a[:3] + a[4:], b[:-1]))
            if parent is not None:
                c = routes["predict_instances_parent"]()
                row["parent_equal"] = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                      y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, c))
            row["pair_first_image"] = b[-1][0].tolist()
            row["peak_bytes_over_start"] = {k: peak_over_start(routes[k]) for k in ("predict_instances", "evaluate_instances")}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp, Y, cl, label, head, shift
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
