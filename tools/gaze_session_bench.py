"""What a GazeSession step costs on one MI355X against DeformSegmentationModule.predict_instances() on every frame.  Eval mode,
ops.static_weight_packs (serving), HRNetV2 + C1 (LVIS-50, K = 51), input side^2 -> 80^2 grid -> side^2.  The routes run in ONE process,
three rounds, the order changing every iteration:

    instances         module.predict_instances(X, Fp, return_bits=True), what a caller without a session runs per frame
    reuse             session.step(X, Fp) on an unchanged frame and gaze: tiles, decide, the 64 * B byte read-back, commit
    run_all           session.step(X, Fp, force=all): the same, then the network for every viewer and the commit of frame and records
    instances_parent  (--parent-lib) `instances` through a library built from the parent commit

    python tools/gaze_session_bench.py [--sizes 1:1024,64:1024] [--warmup 3] [--iters 10] [--parent-lib FILE.so] [--out FILE.json] [--profile]

Every figure is host wall time in ms.  `reuse` ends with the step's own read-back (its commit launch is enqueued, not waited for: the
next step's read-back waits for it, so back-to-back steps pay it); the other routes end with a device synchronise.  Per size and
round: median (min - max).  run_all - instances is the added cost of a step in which every viewer runs.
--profile: a short run for `rocprofv3 --kernel-trace --stats` (reuse steps and one forced step per size, no timing).
--summarize DIR: the gate kernels of such a run's kernel trace, per kernel and launch size."""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

import instances_bench as IB
from instances_bench import stats


class ParentLibrary:
    """A library built from the parent commit, bound like this one's (it has no fs_gate_* symbols); inside a `with` every hip.call
    and every host-side switch goes to it."""

    def __init__(self, path):
        own_lib, own_path, own_env = hip._lib, hip.LIB_PATH, os.environ.get("FS_HIP_LIB")
        gate = {k: hip.SIGNATURES.pop(k) for k in list(hip.SIGNATURES) if k.startswith("fs_gate_")}
        os.environ["FS_HIP_LIB"], hip.LIB_PATH, hip._lib = path, path, None
        try:
            self.lib = hip.load()
        finally:
            hip.SIGNATURES.update(gate)
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


def wall(fn, sync):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1:1024,64:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tile", type=int, default=32)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize:
        IB.KERNELS = ("gate_tiles", "gate_decide", "gate_commit")
        return IB.summarize(args.summarize)
    assert torch.cuda.is_available(), "gaze_session_bench measures on the GPU"
    hip.load()
    cfg = fovealseg.lvis50_cfg()
    module, _ = T.build_module(cfg, device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    # with the name-keyed weights one constant class wins everywhere: a large background logit lets the mask plane draw a blob
    with torch.no_grad():
        module.decoder.cls_net.fc.bias[-1] += 1000.0
    parent = ParentLibrary(args.parent_lib) if args.parent_lib else None
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(), "tile": args.tile,
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> side^2", "sizes": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            X, Fp, _, _ = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            reuse_s = fovealseg.GazeSession(module, B, (side, side), tile=args.tile)
            run_s = fovealseg.GazeSession(module, B, (side, side), tile=args.tile)
            force = torch.ones(B, dtype=torch.int32, device="cuda")

            def instances_parent():
                with parent:
                    return module.predict_instances(X, Fp, return_bits=True)
            routes = {"instances": (lambda: module.predict_instances(X, Fp, return_bits=True), True),
                      "reuse": (lambda: reuse_s.step(X, Fp), False),
                      "run_all": (lambda: run_s.step(X, Fp, force=force), True)}
            if parent is not None:
                routes["instances_parent"] = (instances_parent, True)
            first = reuse_s.step(X, Fp)
            assert first[-1][:, 0].tolist() == [1] * B                                  # RUN_INIT
            if args.profile:
                for _ in range(4):
                    reuse_s.step(X, Fp)
                run_s.step(X, Fp, force=force)
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                for fn, _sync in routes.values():
                    fn()
            perms = list(itertools.permutations(routes))
            rounds, equal, codes_ok = [], True, True
            for _ in range(3):
                ms = {k: [] for k in routes}
                for it in range(args.iters):
                    outs = {}
                    for k in perms[(7 * it) % len(perms)]:                             # another order every iteration
                        t, outs[k] = wall(*routes[k])
                        ms[k].append(t)
                    torch.cuda.synchronize()
                    codes_ok &= outs["reuse"][-1][:, 0].tolist() == [0] * B and outs["run_all"][-1][:, 0].tolist() == [7] * B
                    for i in range(4):                                                  # cat, stats, counts, bits: one record on every route
                        equal &= all(bool(torch.equal(outs[k][i], outs["instances"][i])) for k in routes)
                    del outs
                rounds.append({k: stats(v) for k, v in ms.items()})
            module.check_nan()
            row = {"batch": B, "side": side, "iters": args.iters, "rounds": rounds, "records_equal_on_every_route": equal,
                   "reuse_steps_all_REUSE_and_forced_steps_all_RUN_FORCED": codes_ok, "areas_first_images": first[1][:4, 0].tolist(),
                   "reuse_over_instances": [round(r["reuse"]["ms_median"] / r["instances"]["ms_median"], 5) for r in rounds],
                   "run_all_minus_instances_ms": [round(r["run_all"]["ms_median"] - r["instances"]["ms_median"], 3) for r in rounds],
                   "session_counts": {"reuse": reuse_s.counts, "run_all": run_s.counts}}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp, reuse_s, run_s, first
            torch.cuda.empty_cache()
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
