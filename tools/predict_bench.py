"""Label-free full-resolution prediction on one MI355X: DeformSegmentationModule.predict against the route a user chains by hand
(stages -> PredAssemble -> ops.unwarp_nearest -> argmax), and the shared stages alone, in ONE process, alternating the three per
iteration after a warm-up of each.  Eval mode, ops.static_weight_packs (serving), HRNetV2 + C1 (LVIS-50, K = 51).

    python tools/predict_bench.py [--sizes 64:1024,1:1024] [--warmup 3] [--iters 10] [--out FILE.json] [--profile]

Per size: median / min ms per call of each route, img/s, the unwarp share (route - stages), and the peak-memory increase of each
route over the memory allocated before its call.  Both routes' outputs are compared with torch.equal at every timed size.
--profile: a short run for `rocprofv3 --kernel-trace --stats` (two calls of each route, no timing).
--summarize DIR: the un-warp kernels of such a run's kernel trace, per kernel and launch size (average us, calls)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fovealseg
from fovealseg import ops
from fovealseg import train as T


def stages(module, X, Fp):
    xs, _ = module.saliency(X, Fp)
    grid = module.create_grid(xs)
    cls, m = module.decoder.forward_parts_nhwc(module.encoder.forward_nhwc(ops.GridSample.apply(X, grid)))
    return cls, m, grid


def chained(module, X, Fp):
    cls, m, grid = stages(module, X, Fp)
    full, _ = ops.unwarp_nearest(ops.PredAssemble.apply(cls, m), grid, X.shape[2], X.shape[3])
    return full.argmax(1)


def timed(fn):
    """(ms, peak-memory increase in GB, result) of one call."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (torch.cuda.max_memory_allocated() - before) / 2 ** 30, out


UNWARP_KERNELS = ("unwarp_", "inverse_owner", "inverse_grid", "fill_row", "fill_col", "fill_copy", "grid_sample_fwd", "pred_assemble",
                  "ArgMax", "compare_scalar", "fillBuffer")


def summarize(trace_dir):
    """Per (kernel, launch size): calls and average duration from rocprofv3's kernel_trace.csv."""
    import csv
    import glob
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            if not any(k in r["Kernel_Name"] for k in UNWARP_KERNELS):
                continue
            key = (name[:70], int(r["Grid_Size_X"]))
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':72s} {'work-items':>12s} {'calls':>6s} {'avg us':>9s}")
    for (name, grid), ts in sorted(rows.items(), key=lambda kv: (-kv[0][1], kv[0][0])):
        print(f"{name:72s} {grid:12d} {len(ts):6d} {sum(ts) / len(ts):9.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64:1024,1:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    assert torch.cuda.is_available(), "predict_bench measures on the GPU"
    fovealseg.hip.load()
    cfg = fovealseg.lvis50_cfg()
    module, _ = T.build_module(cfg, device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": fovealseg.hip.get_conv_precision(),
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> side^2 class map", "sizes": []}
    routes = {"predict": lambda: module.predict(X, Fp), "chained": lambda: chained(module, X, Fp), "stages": lambda: stages(module, X, Fp)}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            X, Fp, _, _ = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            if args.profile:
                for _ in range(2):
                    for fn in routes.values():
                        fn()
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                for fn in routes.values():
                    fn()
            ms = {k: [] for k in routes}
            mem = {k: 0.0 for k in routes}
            equal = True
            for _ in range(args.iters):
                outs = {}
                for k, fn in routes.items():
                    t, gb, outs[k] = timed(fn)
                    ms[k].append(t)
                    mem[k] = max(mem[k], gb)
                equal &= bool(torch.equal(outs["predict"], outs["chained"]))
                del outs
            module.check_nan()
            row = {"batch": B, "input": side, "seg_size": side, "iters": args.iters, "outputs_equal": equal}
            for k in routes:
                med = statistics.median(ms[k])
                row[k] = {"ms_median": round(med, 3), "ms_min": round(min(ms[k]), 3), "img_per_s": round(1e3 * B / med, 1),
                          "peak_mem_increase_gb": round(mem[k], 3)}
            row["unwarp_ms"] = {k: round(row[k]["ms_median"] - row["stages"]["ms_median"], 3) for k in ("predict", "chained")}
            row["speedup_chained_over_predict"] = round(row["chained"]["ms_median"] / row["predict"]["ms_median"], 3)
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp
            torch.cuda.empty_cache()
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
