"""What the instance record costs on one MI355X: DeformSegmentationModule.predict_instances() against predict(), and against the
route a user writes without it -- predict(), `!= K - 1`, the mask to the host, the run-length code per image in numpy
(tests/rle_ref.py) -- a cross check as well: the device's records must be the host's.  Eval mode, ops.static_weight_packs (serving),
HRNetV2 + C1 (LVIS-50, K = 51).  The routes run in ONE process, three rounds, the order changing every iteration; the host route runs
`--host-iters` times a round (it takes seconds at B = 64).

    python tools/instances_bench.py [--sizes 64:1024,1:1024] [--warmup 3] [--iters 10] [--host-iters 1] [--parent-lib FILE.so] [--out FILE.json] [--profile]

Per size and round: median (min - max) ms per call of each route; per size the peak-memory increase of each device route over the
memory allocated before its call, the bytes a consumer copies to the host on either route, and whether the records agree.
--parent-lib: a libfovealseg_hip.so built from the parent commit; predict() through that library's fs_unwarp_labels is alternated with
this one's (A B B A ...) in the same three rounds, every other kernel of the call being the same code in both.
--profile: a short run for `rocprofv3 --kernel-trace --stats` (two calls of each device route, no timing).
--summarize DIR: the un-warp kernels of such a run's kernel trace, per kernel and launch size (average us, calls)."""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

import rle_ref as R

KERNELS = ("unwarp_", "inverse_owner", "fill_row", "rle_", "instance_cat", "mask_bits", "fillBuffer")


class ParentLabels:
    """Swaps the parent library's fs_unwarp_labels into hip.call for the duration of a `with`."""

    def __init__(self, path):
        self.fn = ctypes.CDLL(path).fs_unwarp_labels
        self.fn.restype = ctypes.c_int
        self.fn.argtypes = [hip._CT[c] for c in hip.SIGNATURES["fs_unwarp_labels"]] + [hip._P]
        self.own = hip.load().fs_unwarp_labels

    def __enter__(self):
        hip._fn_cache["fs_unwarp_labels"] = self.fn

    def __exit__(self, *exc):
        hip._fn_cache["fs_unwarp_labels"] = self.own


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


def summarize(trace_dir):
    """Per (kernel, launch size): calls and average duration from rocprofv3's kernel_trace.csv or its results database."""
    import csv
    import glob
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if not any(k in r["Kernel_Name"] for k in KERNELS):
                continue
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            rows.setdefault((name[:70], int(r["Grid_Size_X"])), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for path in glob.glob(os.path.join(trace_dir, "**", "*_results.db"), recursive=True):      # rocprofv3's default output: its `kernels` view
        import sqlite3
        for kname, grid, dur in sqlite3.connect(path).execute("select name, grid_x, duration from kernels"):
            if not any(k in kname for k in KERNELS):
                continue
            name = kname.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            rows.setdefault((name[:70], int(grid)), []).append(dur / 1e3)
    print(f"{'kernel':72s} {'work-items':>12s} {'calls':>6s} {'avg us':>9s}")
    for (name, grid), ts in sorted(rows.items(), key=lambda kv: (-kv[0][1], kv[0][0])):
        print(f"{name:72s} {grid:12d} {len(ts):6d} {sum(ts) / len(ts):9.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64:1024,1:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    assert torch.cuda.is_available(), "instances_bench measures on the GPU"
    hip.load()
    cfg = fovealseg.lvis50_cfg()
    K = cfg.DATASET.num_class
    module, _ = T.build_module(cfg, device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    # with the name-keyed weights one constant class wins everywhere: a large background logit lets the mask plane draw a blob
    with torch.no_grad():
        module.decoder.cls_net.fc.bias[-1] += 1000.0
    parent = ParentLabels(args.parent_lib) if args.parent_lib else None

    def predict_parent():
        with parent:
            return module.predict(X, Fp)
    routes = {"predict_instances": lambda: module.predict_instances(X, Fp), "predict": lambda: module.predict(X, Fp)}
    if parent is not None:
        routes["predict_parent"] = predict_parent
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(),
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> side^2", "sizes": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            X, Fp, _, _ = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            if args.profile:
                for _ in range(2):
                    module.predict_instances(X, Fp)
                    module.predict(X, Fp)
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            perms = list(itertools.permutations(routes))
            rounds, equal = [], True
            host_s, host_agrees = [], True
            for _ in range(3):
                ms = {k: [] for k in routes}
                for it in range(args.iters):
                    outs = {}
                    for k in perms[(7 * it) % len(perms)]:                             # another order every iteration
                        t, outs[k] = timed(routes[k])
                        ms[k].append(t)
                    if parent is not None:
                        equal &= bool(torch.equal(outs["predict"], outs["predict_parent"]))
                    cat, st, counts = outs["predict_instances"]
                    del outs
                rnd = {k: stats(v) for k, v in ms.items()}
                # the route without the op: the class map, the comparison, the mask to the host, numpy per image
                for _ in range(args.host_iters):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    mask = (module.predict(X, Fp) != K - 1).cpu().numpy()
                    want = [(R.stats(m), R.encode(m)) for m in mask]
                    host_s.append(time.perf_counter() - t0)
                    cap = counts.shape[1]
                    sth, ch = st.cpu().tolist(), counts.cpu().numpy()
                    host_agrees &= all(sth[b] == want[b][0] and ch[b, :min(cap, len(want[b][1]))].tolist() == want[b][1][:cap] for b in range(B))
                rounds.append(rnd)
            module.check_nan()
            row = {"batch": B, "side": side, "iters": args.iters, "rounds": rounds, "predict_equals_parent": equal if parent is not None else None,
                   "host_route_s": [round(v, 3) for v in host_s], "records_equal_host": host_agrees,
                   "areas_first_images": st[:4, 0].tolist(), "runs_first_images": st[:4, 5].tolist(), "runs_max": int(st[:, 5].max()),
                   "max_runs": int(counts.shape[1])}
            row["peak_mem_increase_mib"] = {k: round(peak_over_start(routes[k]) / 2 ** 20, 1) for k in ("predict_instances", "predict")}
            row["bytes_to_host"] = {"predict_instances": cat.numel() * 8 + st.numel() * 8 + counts.numel() * 4,
                                    "predict_instances_used_counts": cat.numel() * 8 + st.numel() * 8 + int(st[:, 5].clamp(max=counts.shape[1]).sum()) * 4,
                                    "predict_labels": B * side * side * 8, "predict_bool_mask": B * side * side}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp
            torch.cuda.empty_cache()
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
