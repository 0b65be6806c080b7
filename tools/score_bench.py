"""What the instance score costs on one MI355X: DeformSegmentationModule.predict_instances(return_score=True) against
predict_instances(), the un-warp alone with and without the score on fixed head outputs (the model's mask, and an all-foreground one), the table kernel alone (fs_head_fg_q), and --
for the record, and as a cross check -- the same score by the route without the op: ops.unwarp_nearest on the (B,K,H,W) prediction, a
softmax in fp64 per image, the mean over the mask.  Eval mode, ops.static_weight_packs (serving), HRNetV2 + C1 (LVIS-50, K = 51).  The
routes run in ONE process, three rounds, the order changing every iteration.

    python tools/score_bench.py [--sizes 64:1024,1:1024] [--warmup 3] [--iters 10] [--op-reps 20] [--route-iters 1] [--parent-lib FILE.so] [--out FILE.json] [--profile]

Per size and round: median (min - max) ms per call of each route.  The un-warp rows time --op-reps back-to-back calls between two
device events and divide.
--parent-lib: a libfovealseg_hip.so built from the parent commit; predict_instances() through that library's fs_unwarp_instances is
alternated with this one's in the same three rounds, every other kernel of the call being the same code in both.
--profile: a short run for `rocprofv3 --kernel-trace --stats` (two calls of each route, no timing).
--summarize DIR: the un-warp kernels of such a run's kernel trace, per kernel and launch size (tools/instances_bench.py's table)."""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

import instances_bench as IB
from instances_bench import stats, timed


class ParentInstances:
    """Swaps the parent library's fs_unwarp_instances into hip.call for the duration of a `with`."""

    def __init__(self, path):
        self.fn = ctypes.CDLL(path).fs_unwarp_instances
        self.fn.restype = ctypes.c_int
        self.fn.argtypes = [hip._CT[c] for c in hip.SIGNATURES["fs_unwarp_instances"]] + [hip._P]
        self.own = hip.load().fs_unwarp_instances

    def __enter__(self):
        hip._fn_cache["fs_unwarp_instances"] = self.fn

    def __exit__(self, *exc):
        hip._fn_cache["fs_unwarp_instances"] = self.own


def timed_reps(fn, reps):
    ms, out = timed(lambda: [fn() for _ in range(reps)][-1])
    return ms / reps, out


def score_by_softmax(module, X, Fp, K):
    """The score without the op: the full-resolution prediction, its argmax, an fp64 softmax per image."""
    xs, _ = module.saliency(X, Fp)
    grid = module.create_grid(xs)
    feat = module.encoder.forward_nhwc(ops.GridSample.apply(X, grid))
    cls, _m = module.decoder.forward_parts_nhwc(feat)
    full, _ = ops.unwarp_nearest(module.decoder.forward_nhwc(feat), grid, X.shape[2], X.shape[3])
    out = []
    for b in range(X.shape[0]):
        mask = full[b].argmax(0) != K - 1
        fg = 1.0 - torch.softmax(full[b].permute(1, 2, 0)[mask].double(), 1)[:, K - 1]
        cp = torch.softmax(cls[b, :K - 1].double(), 0).max()
        out.append((cp * fg.mean()) if fg.numel() else cp * 0)
    return torch.stack(out), int(full.numel()) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64:1024,1:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--op-reps", type=int, default=20)
    ap.add_argument("--route-iters", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize:
        IB.KERNELS = IB.KERNELS + ("head_fg_q", "instance_conf")
        return IB.summarize(args.summarize)
    assert torch.cuda.is_available(), "score_bench measures on the GPU"
    hip.load()
    cfg = fovealseg.lvis50_cfg()
    K = cfg.DATASET.num_class
    module, _ = T.build_module(cfg, device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    # with the name-keyed weights one constant class wins everywhere: a large background logit lets the mask plane draw a blob
    with torch.no_grad():
        module.decoder.cls_net.fc.bias[-1] += 1000.0
    parent = ParentInstances(args.parent_lib) if args.parent_lib else None

    def instances_parent():
        with parent:
            return module.predict_instances(X, Fp)
    routes = {"scored": lambda: module.predict_instances(X, Fp, return_score=True), "unscored": lambda: module.predict_instances(X, Fp)}
    if parent is not None:
        routes["unscored_parent"] = instances_parent
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(),
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> side^2", "sizes": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            X, Fp, _, _ = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            cls, m, grid, _size = module._head_parts(X, Fp, None, "score_bench")
            dense = -m.abs() - 0.01
            ops_routes = {"unwarp_scored": lambda: ops.unwarp_instances(cls, m, grid, side, side, score=True),
                          "unwarp_unscored": lambda: ops.unwarp_instances(cls, m, grid, side, side),
                          "head_fg_q": lambda: ops.head_fg_q(cls, m),
                          # every pixel foreground: every wave of the scored gather reduces and adds
                          "unwarp_scored_dense": lambda: ops.unwarp_instances(cls, dense, grid, side, side, score=True),
                          "unwarp_unscored_dense": lambda: ops.unwarp_instances(cls, dense, grid, side, side)}
            if args.profile:
                for _ in range(2):
                    for fn in list(routes.values())[:2] + [ops_routes["head_fg_q"]]:
                        fn()
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                for fn in list(routes.values()) + list(ops_routes.values()):
                    fn()
            perms, operms = list(itertools.permutations(routes)), list(itertools.permutations(ops_routes))
            rounds, equal = [], True
            for _ in range(3):
                ms = {k: [] for k in list(routes) + list(ops_routes)}
                for it in range(args.iters):
                    outs = {}
                    for k in perms[(7 * it) % len(perms)]:                             # another order every iteration
                        t, outs[k] = timed(routes[k])
                        ms[k].append(t)
                    for k in operms[(5 * it) % len(operms)]:
                        t, outs[k] = timed_reps(ops_routes[k], args.op_reps)
                        ms[k].append(t)
                    for i in range(3):                                                  # cat, stats, counts: one record on every route
                        equal &= all(bool(torch.equal(outs[k][i], outs["scored"][i])) for k in routes)
                        equal &= all(bool(torch.equal(outs[k][i], outs["scored"][i])) for k in ("unwarp_scored", "unwarp_unscored"))
                    equal &= all(bool(torch.equal(outs["unwarp_scored_dense"][i], outs["unwarp_unscored_dense"][i])) for i in range(3))
                    dense_area = outs["unwarp_scored_dense"][1][:, 0]
                    equal &= bool(torch.equal(outs["unwarp_scored"][3], outs["scored"][3]))
                    st, conf = outs["scored"][1], outs["scored"][3]
                    del outs
                rounds.append({k: stats(v) for k, v in ms.items()})
            soft_ms, soft = [], None
            for _ in range(args.route_iters):
                t, (soft, full_bytes) = timed(lambda: score_by_softmax(module, X, Fp, K))
                soft_ms.append(round(t, 1))
            torch.cuda.empty_cache()
            module.check_nan()
            row = {"batch": B, "side": side, "iters": args.iters, "op_reps": args.op_reps, "rounds": rounds, "records_equal_on_every_route": equal,
                   "areas_first_images": st[:4, 0].tolist(), "dense_areas_first_images": dense_area[:4].tolist(), "conf_first_images": conf[:4].tolist(),
                   "softmax_route_ms": soft_ms, "softmax_route_prediction_bytes": full_bytes if soft is not None else None,
                   "softmax_route_max_abs_score_diff": float((soft - conf[:, 0].double()).abs().max()) if soft is not None else None}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
            del X, Fp, cls, m, grid, dense
            torch.cuda.empty_cache()
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
