"""What the per-class areas cost on one MI355X: DeformSegmentationModule.evaluate() against evaluate(class_areas=True), against
evaluate() through the parent commit's fs_unwarp_accuracy, and against predict() followed by the same full-resolution areas made with
torch.bincount on the (B,H,W) int64 class map (a cross check as well: the two must agree).  All routes run in ONE process, the order
changing every iteration.

    python tools/class_area_bench.py [--sizes 64:1024] [--warmup 3] [--iters 10] [--parent-lib FILE.so] [--out FILE.json] [--profile]

--parent-lib: a libfovealseg_hip.so built from the parent commit (build.py on a checkout of it); the bench calls that library's
fs_unwarp_accuracy in place of this one's (every other kernel of the call is the same code in both), so that the default path can be
compared across the two commits inside one process.
After the module routes, the op alone (ops.unwarp_class_areas against ops.unwarp_accuracy, device events around `--op-reps` calls) in
the hot regime (a dominant mask plane, K = 51) and in the cold one (K = 150, cls plain randn: nearly every pixel goes through the LDS
bins and the atomics), at the first size of --sizes.
--profile: a short run for `rocprofv3 --kernel-trace --stats` (two calls of evaluate(class_areas=True), two of the cold op; no timing)."""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

K = 51


def bincount_areas(labels, Y, cl, K):
    """(B, K, 3) int64 (inter, pred, lab) of a class map against the composed ground truth: three torch.bincount calls."""
    B = labels.shape[0]
    t = Y[:, 0].long()
    g = t * cl[:, :, None] + (1 - t) * (K - 1)
    off = torch.arange(B, device=labels.device)[:, None, None] * K
    pred = torch.bincount((labels + off).flatten(), minlength=B * K)
    lab = torch.bincount((g + off).flatten(), minlength=B * K)
    inter = torch.bincount((labels + off)[labels == g], minlength=B * K)
    return torch.stack([inter, pred, lab]).reshape(3, B, K).permute(1, 2, 0).contiguous()


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
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def op_inputs(B, Kc, side, dominant, seed=5):
    g = torch.Generator().manual_seed(seed)
    grid = (torch.rand(B, 80, 80, 2, generator=g) * 2 - 1)
    cls = torch.randn(B, Kc, generator=g)
    if dominant:
        cls[:, Kc - 1] = 3 * cls.abs().amax(1)
    m = torch.rand(B, 80, 80, generator=g) - 0.5
    _, _, Y, _ = T.synthetic_batch(B, side, side, seed=seed, device="cuda")
    cl = torch.randint(0, Kc - 1, (B, 1), generator=g)
    return cls.cuda(), m.cuda(), grid.cuda(), Y, cl.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--op-reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "class_area_bench measures on the GPU"
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
    routes["evaluate_areas"] = lambda: module.evaluate(X, Fp, Y, cl, class_areas=True)
    routes["predict_bincount"] = lambda: bincount_areas(module.predict(X, Fp), Y, cl, K)
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(),
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> scores at side^2", "sizes": []}
    with torch.no_grad():
        for n_spec, spec in enumerate(args.sizes.split(",")):
            B, side = (int(v) for v in spec.split(":"))
            X, Fp, Y, cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            cold = op_inputs(B, 150, side, dominant=False) if n_spec == 0 else None
            if args.profile:
                for _ in range(2):
                    routes["evaluate_areas"]()
                if cold is not None:
                    for _ in range(2):
                        ops.unwarp_class_areas(*cold)
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
                equal &= bool(torch.equal(outs["evaluate_areas"][5][:, 0], outs["predict_bincount"]))
                equal &= all(torch.equal(a, b) for a, b in zip(outs["evaluate"], outs["evaluate_areas"][:5]))
                if parent is not None:
                    equal &= all(torch.equal(a, b) for a, b in zip(outs["evaluate"], outs["evaluate_parent"]))
                del outs
            module.check_nan()
            row = {"batch": B, "side": side, "iters": args.iters, "results_equal": equal}
            for k in routes:
                row[k] = stats(ms[k])
            if parent is not None:
                # the default path against the parent's, the two alone: A B B A ..., so that neither always follows the other
                ab = {"evaluate": [], "evaluate_parent": []}
                for it in range(2 * args.iters):
                    for k in (("evaluate", "evaluate_parent") if it % 2 == 0 else ("evaluate_parent", "evaluate")):
                        ab[k].append(timed(routes[k])[0])
                row["default_vs_parent_abba"] = {k: stats(v) for k, v in ab.items()}
            row["areas_add_ms"] = round(row["evaluate_areas"]["ms_median"] - row["evaluate"]["ms_median"], 3)
            row["bincount_route_adds_ms"] = round(row["predict_bincount"]["ms_median"] - row["evaluate"]["ms_median"], 3)
            row["peak_bytes_over_start"] = {k: peak_over_start(routes[k]) for k in ("evaluate", "evaluate_areas", "predict_bincount")}
            if n_spec == 0:
                # the op alone: hot regime at K = 51, cold regime at K = 150
                hot = op_inputs(B, K, side, dominant=True)

                def reps(fn):
                    def run():
                        for _ in range(args.op_reps):
                            fn()
                    return timed(run)[0] / args.op_reps
                op = {}
                for name, inp in (("hot_K51", hot), ("cold_K150", cold)):
                    for _ in range(2):
                        ops.unwarp_accuracy(*inp)
                        areas = ops.unwarp_class_areas(*inp)[2]
                    hotpix = areas[:, 0, -1, 1] + areas[torch.arange(B, device=areas.device), 0, inp[4].reshape(-1), 1]
                    a_ms, c_ms = [], []
                    for _ in range(3):                                                 # alternating
                        a_ms.append(reps(lambda: ops.unwarp_accuracy(*inp)))
                        c_ms.append(reps(lambda: ops.unwarp_class_areas(*inp)))
                    op[name] = {"unwarp_accuracy_ms": [round(v, 4) for v in a_ms], "unwarp_class_areas_ms": [round(v, 4) for v in c_ms],
                                "share_of_pixels_in_lds_bins": round(1.0 - float(hotpix.sum()) / (B * side * side), 4),
                                "classes_predicted": int((areas[:, 0, :, 1].sum(0) > 0).sum())}
                row["op_alone"] = op
                del hot
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp, Y, cl, cold
            torch.cuda.empty_cache()
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
