"""What the Hausdorff percentile costs on one MI355X: DeformSegmentationModule.evaluate() against evaluate(hausdorff=95), against
evaluate() through the parent commit's fs_unwarp_accuracy, and against evaluate(return_labels=True) followed by the same metric made
per image on the host with scipy (binary_erosion, distance_transform_edt) and np.percentile -- a cross check as well: the device's
integers must give the host's distances.  The device routes run in ONE process, the order changing every iteration; the host route
runs `--host-iters` times (it takes seconds).

    python tools/hd_bench.py [--sizes 64:1024] [--warmup 3] [--iters 10] [--host-iters 1] [--parent-lib FILE.so] [--out FILE.json] [--profile]

--parent-lib: a libfovealseg_hip.so built from the parent commit (build.py on a checkout of it); the bench calls that library's
fs_unwarp_accuracy in place of this one's (every other kernel of the call is the same code in both), so that the default path can be
compared across the two commits inside one process, in three rounds of alternating calls.
After the module routes, the op alone at the first size of --sizes: ops.surface_hd on the byte map of the module's own class map and
label (the column pass, twice the row pass and the selections), and the same on a noisy prediction (5 % of the pixels flipped: two
million border pixels an image), device events around `--op-reps` calls.
--profile: a short run for `rocprofv3 --kernel-trace --stats` (two calls of evaluate(hausdorff=95), two of the noisy op; no timing)."""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

K = 51
Q = 95


def host_hd(labels, Y, q=Q):
    """(B,) fp64: the metric per image with scipy on the host, from the (B,H,W) int64 class map and the label mask."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    cross = generate_binary_structure(2, 1)
    pred = (labels != K - 1).cpu().numpy()
    lab = (Y[:, 0].long() != 0).cpu().numpy()
    out = np.full(len(pred), np.nan)
    for i, (a, b) in enumerate(zip(pred, lab)):
        ab, bb = a ^ binary_erosion(a, structure=cross), b ^ binary_erosion(b, structure=cross)
        if not ab.any() or not bb.any():
            continue
        out[i] = np.percentile(np.hstack([distance_transform_edt(~bb)[ab], distance_transform_edt(~ab)[bb]]), q)
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--op-reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hd_bench measures on the GPU"
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
    routes["evaluate_hd"] = lambda: module.evaluate(X, Fp, Y, cl, hausdorff=Q)
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(), "q": Q,
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> scores at side^2", "sizes": []}
    with torch.no_grad():
        for n_spec, spec in enumerate(args.sizes.split(",")):
            B, side = (int(v) for v in spec.split(":"))
            X, Fp, Y, cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            g = torch.Generator().manual_seed(5)
            noisy_a = torch.rand(B, side, side, generator=g) < 0.5
            noisy = (noisy_a.cuda(), (noisy_a ^ (torch.rand(B, side, side, generator=g) < 0.05)).cuda()) if n_spec == 0 else None
            del noisy_a
            if args.profile:
                for _ in range(2):
                    routes["evaluate_hd"]()
                if noisy is not None:
                    for _ in range(2):
                        ops.surface_hd(*noisy, q=Q)
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
                equal &= all(torch.equal(a, b) for a, b in zip(outs["evaluate"], outs["evaluate_hd"][:5]))
                if parent is not None:
                    equal &= all(torch.equal(a, b) for a, b in zip(outs["evaluate"], outs["evaluate_parent"]))
                hd = outs["evaluate_hd"][5]
                del outs
            module.check_nan()
            row = {"batch": B, "side": side, "iters": args.iters, "results_equal": equal, "hd_stats_first_images": hd[:4].tolist()}
            for k in routes:
                row[k] = stats(ms[k])
            if parent is not None:
                # the default path against the parent's, the two alone, in three rounds: A B B A ..., so that neither always follows the other
                rounds = []
                for _ in range(3):
                    ab = {"evaluate": [], "evaluate_parent": []}
                    for it in range(args.iters):
                        for k in (("evaluate", "evaluate_parent") if it % 2 == 0 else ("evaluate_parent", "evaluate")):
                            ab[k].append(timed(routes[k])[0])
                    rounds.append({k: stats(v) for k, v in ab.items()})
                row["default_vs_parent_rounds"] = rounds
            row["hd_add_ms"] = round(row["evaluate_hd"]["ms_median"] - row["evaluate"]["ms_median"], 3)
            # the host route: the class map to the host, scipy per image
            host_s, dist_host = [], None
            for _ in range(args.host_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = module.evaluate(X, Fp, Y, cl, return_labels=True)
                dist_host = host_hd(out[5], Y)
                host_s.append(time.perf_counter() - t0)
                del out
            if dist_host is not None:
                dist_dev = ops.hd_from_stats(hd, Q).cpu().numpy()
                both = ~np.isnan(dist_host)
                row["host_scipy_route_s"] = [round(v, 3) for v in host_s]
                row["host_agrees"] = bool(np.array_equal(np.isnan(dist_dev), np.isnan(dist_host)) and
                                          (not both.any() or np.abs(dist_dev[both] - dist_host[both]).max() <= 1e-12 * max(1.0, dist_host[both].max())))
                row["hd_pixels_first_images"] = [None if np.isnan(v) else round(float(v), 4) for v in dist_dev[:4]]
                row["images_with_both_borders"] = int(both.sum())
            row["peak_bytes_over_start"] = {k: peak_over_start(routes[k]) for k in ("evaluate", "evaluate_hd")}
            row["peak_bytes_over_start"]["evaluate_labels"] = peak_over_start(lambda: module.evaluate(X, Fp, Y, cl, return_labels=True))
            if n_spec == 0:
                labels = module.evaluate(X, Fp, Y, cl, return_labels=True)[5]
                own = (labels != K - 1, Y[:, 0].long() != 0)
                del labels

                def reps(fn):
                    def run():
                        for _ in range(args.op_reps):
                            fn()
                    return timed(run)[0] / args.op_reps
                op = {}
                for name, pair in (("module_masks", own), ("noisy_masks", noisy)):
                    fg = ((pair[0] != 0).to(torch.uint8) | ((pair[1] != 0).to(torch.uint8) << 1)).contiguous()
                    out = torch.empty(B, 4, device="cuda", dtype=torch.int64)
                    scr = torch.empty(hip.query("fs_surface_hd_scratch_ints", B, side, side), device="cuda", dtype=torch.int32)

                    def call():
                        hip.call("fs_surface_hd", fg.data_ptr(), out.data_ptr(), scr.data_ptr(), B, side, side, Q)
                    call()
                    op[name] = {"fs_surface_hd_ms": [round(reps(call), 4) for _ in range(3)],
                                "border_pixels_per_image": round(float((out[:, 0] + out[:, 1]).double().mean()), 1),
                                "scratch_bytes": scr.numel() * 4}
                    del fg, scr
                row["op_alone"] = op
                del own
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp, Y, cl, noisy
            torch.cuda.empty_cache()
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
