"""What choosing the annotated instance under the gaze costs on one MI355X: fs_mask_candidates at B = 64 on 640^2 and 1024^2 with 8 and 64
candidates an image, against the composition a caller had before it -- a torch gather of the image's prediction per candidate, the
counters through ops.mask_pair_counts (d = 1), the gaze pixel's bit of every candidate by indexing, ONE host read and the choice
(smallest area among those that contain the gaze pixel) on the host; that composition does not snap to the nearest instance.  Then
train.score_coco_records(gaze=...) on 256 images with several polygon annotations each against the host pre-filter (PIL draws every
annotation, the gaze pixel is looked up, the smallest containing annotation is kept) followed by the one-instance call.  Everything
runs in ONE process, the routes alternating, in three rounds.

    python tools/candidates_bench.py [--batch 64] [--op-reps 10] [--images 256] [--parent-lib FILE.so] [--kernel-only] [--out FILE.json]

Device passes are event times over --op-reps back-to-back calls on preallocated buffers, in microseconds a call; routes are host wall
time in ms ending with a device synchronise.  The shares of the passes come from torch.profiler's kernel times of one call.
--parent-lib (a library built from the parent commit) adds predict_instances and evaluate_instances through either library.
--kernel-only prints the fs_mask_candidates times and passes alone: under a kernel A/B build (FS_BUILD_EXPERIMENTS=1 python build.py;
FS_HIP_LIB=ab/libfovealseg_experiments.so) FS_CAND_VEC=1 turns the 16-byte loads of the count pass off, FS_CAND_ROWS / FS_CAND_WORDS
change the band plan."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from fovealseg import hip, ops
from fovealseg import train as T

from instance_eval_bench import timed
from poly_bench import blob, wall


def rect_words(gen, n, side):
    """n random rectangles of a tenth to six tenths of the side, as bit words, made in chunks on the device"""
    out = []
    yy = torch.arange(side, device="cuda")[None, :, None]
    xx = torch.arange(side, device="cuda")[None, None, :]
    for at in range(0, n, 128):
        k = min(128, n - at)
        ext = (torch.rand(k, 2, generator=gen, device="cuda") * 0.5 + 0.1) * side
        org = torch.rand(k, 2, generator=gen, device="cuda") * (side - ext)
        y0, x0, y1, x1 = org[:, 0], org[:, 1], org[:, 0] + ext[:, 0], org[:, 1] + ext[:, 1]
        m = (yy >= y0[:, None, None]) & (yy < y1[:, None, None]) & (xx >= x0[:, None, None]) & (xx < x1[:, None, None])
        out.append(ops.mask_bits(m))
    return torch.cat(out)


def composition(cbits, img_of, off, pred, py, px, side):
    """The parent's route: gather, counters, the gaze bit, one host read, the choice on the host."""
    pair = ops.mask_pair_counts(cbits, pred[img_of], 1, Ws=side)
    hit = (cbits[torch.arange(cbits.shape[0], device="cuda"), py[img_of], px[img_of] >> 5] >> (px[img_of] & 31)) & 1
    host = torch.cat([pair[:, :3], hit[:, None].long()], 1).cpu().numpy()
    sel = []
    for b in range(len(off) - 1):
        rows = host[off[b]:off[b + 1]]
        inside = np.flatnonzero(rows[:, 3] == 1)
        sel.append(off[b] + int(inside[np.argmin(rows[inside, 1])]) if len(inside) else -1)
    return sel


def pass_times(fn):
    """{kernel name: microseconds} of one call, from torch.profiler; None where the profiler gives no kernel rows"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
            name = re.search(r"cand_[a-z]+_kernel", e.key)
            if name and t:
                out[name.group(0)] = round(out.get(name.group(0), 0.0) + float(t), 2)
        return out or None
    except Exception as e:                               # a measurement aid: the times above do not depend on it
        return {"error": repr(e)[:200]}


def module_routes(parent_lib, B, side=1024, per=8, iters=6):
    """predict_instances and evaluate_instances without the keyword through this library and through one built from the parent commit
    (tools/instance_eval_bench.py's ParentLibrary), and evaluate_instances(candidates=...), alternating in three rounds."""
    import fovealseg
    import instance_eval_bench as IE
    IE.NEW = ("fs_mask_candidates",)                     # what the parent's library does not have
    parent = IE.ParentLibrary(parent_lib)
    module, _ = T.build_module(fovealseg.lvis50_cfg(), device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(32)
    with torch.no_grad():
        X, Fp, Y, cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
        cand = (rect_words(gen, B * per, side), torch.arange(0, B * per + 1, per, dtype=torch.int32, device="cuda"),
                torch.arange(B * per, device="cuda") % 50)

        def through(fn):
            def run():
                with parent:
                    return fn()
            return run
        predict = lambda: module.predict_instances(X, Fp, return_bits=True, return_score=True)
        evaluate = lambda: module.evaluate_instances(X, Fp, Y, cl)
        routes = {"predict_instances": predict, "predict_instances_parent": through(predict), "evaluate_instances": evaluate,
                  "evaluate_instances_parent": through(evaluate),
                  "evaluate_instances_candidates": lambda: module.evaluate_instances(X, Fp, seg_size=(side, side), candidates=cand)}
        for _ in range(2):
            for fn in routes.values():
                fn()
        names, rounds = list(routes), []
        for _ in range(3):
            ms = {k: [] for k in names}
            for it in range(iters):
                for k in (names if it % 2 == 0 else names[::-1]):
                    ms[k].append(timed(routes[k])[0])
            rounds.append({k: IE.stats(v) for k, v in ms.items()})
        module.check_nan()
        same = lambda a, b: all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                            y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
        return {"batch": B, "side": side, "candidates_per_image": per, "rounds": rounds,
                "parent_equal": same(routes["evaluate_instances"](), routes["evaluate_instances_parent"]())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--op-reps", type=int, default=10)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "candidates_bench measures on the GPU"
    hip.load()
    B = args.batch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "lib": os.environ.get("FS_HIP_LIB", "shipped"),
           "env": {k: v for k, v in os.environ.items() if k.startswith("FS_CAND_")}, "cases": []}
    for side in (640, 1024):
        for per in (8, 64):
            N, P = B * per, (side + 31) // 32
            cbits = rect_words(gen, N, side)
            pred = rect_words(gen, B, side)
            off = list(range(0, N + 1, per))
            cand_off = torch.tensor(off, dtype=torch.int32, device="cuda")
            cat = torch.arange(N, device="cuda") % 50
            focus = torch.rand(B, 2, generator=gen, device="cuda") * 0.5 + 0.25
            py = (focus[:, 0].double() * (side - 1)).round().long()
            px = (focus[:, 1].double() * (side - 1)).round().long()
            img_of = torch.arange(N, device="cuda") // per
            gbits = torch.empty(B, side, P, device="cuda", dtype=torch.int32)
            sel = torch.empty(B, 8, device="cuda", dtype=torch.int64)
            cand = torch.empty(N, 6, device="cuda", dtype=torch.int64)
            scr = torch.empty(hip.query("fs_mask_candidates_scratch_ints", B, N, side, side), device="cuda", dtype=torch.int32)

            def kernel():
                hip.call("fs_mask_candidates", cbits.data_ptr(), cand_off.data_ptr(), cat.data_ptr(), focus.data_ptr(), pred.data_ptr(),
                         cand.data_ptr(), sel.data_ptr(), gbits.data_ptr(), scr.data_ptr(), B, N, side, side, ops.COMPONENT_OFF2)
            kernel()
            entry = {"side": side, "candidates_per_image": per, "N": N, "candidate_bytes": N * side * P * 4, "rounds": []}
            for _ in range(3):                            # the routes take turns within a round
                row = {"fs_mask_candidates_us": round(timed(kernel, args.op_reps)[0] * 1e3, 2)}
                if args.kernel_only:
                    entry["rounds"].append(row)
                    continue
                row = {"fs_mask_candidates_us": row["fs_mask_candidates_us"],
                       "ops_mask_candidates_us": round(timed(lambda: ops.mask_candidates(cbits, cand_off, focus, side, pred=pred, cand_cat=cat),
                                                             args.op_reps)[0] * 1e3, 2),
                       "composition_ms": round(wall(lambda: composition(cbits, img_of, off, pred, py, px, side))[0], 2)}
                entry["rounds"].append(row)
            entry["passes_us"] = pass_times(kernel)
            count = next((v for k, v in (entry["passes_us"] or {}).items() if "count" in k), None)
            if count:
                entry["count_pass_GBps"] = round(entry["candidate_bytes"] / count / 1e3, 1)
                entry["small_passes_share"] = round(1.0 - count / sum(entry["passes_us"].values()), 4)
            if not args.kernel_only:
                theirs = composition(cbits, img_of, off, pred, py, px, side)
                ours = sel[:, 0].tolist()
                entry["selected"] = sum(v >= 0 for v in ours)
                entry["agree_where_contained"] = sum(a == b for a, b in zip(ours, theirs) if b >= 0)
                entry["contained"] = sum(b >= 0 for b in theirs)
            res["cases"].append(entry)
            print(json.dumps(entry), flush=True)
            del cbits, pred, gbits, cand, scr
            torch.cuda.empty_cache()
    if args.kernel_only:
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    # stored records: several polygon annotations an image
    side, n, per = 640, args.images, 8
    rng = np.random.default_rng(31)
    polys = [[blob(rng, side, 48, side * rng.uniform(0.05, 0.25)) for _ in range(per)] for _ in range(n)]
    gt = [{"image_id": i, "category_id": int(rng.integers(0, 50)), "segmentation": [ring], "id": i * per + j}
          for i, rings in enumerate(polys) for j, ring in enumerate(rings)]
    gaze = {i: (float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.3, 0.7))) for i in range(n)}
    images = [{"id": i, "height": side, "width": side} for i in range(n)]
    first, _ = ops.poly_bits(*ops.polygon_rings([[rings[0]] for rings in polys]), (side, side))
    st, cn = ops.mask_rle(first, side)
    dt = [dict(r, score=0.5) for r in ops.instances_to_coco(torch.zeros(n, dtype=torch.int64, device="cuda"), st, cn, (side, side), compressed=True)]
    for r, i in zip(dt, range(n)):
        r["image_id"] = i

    def prefilter():
        from PIL import Image, ImageDraw
        keep = []
        for i in range(n):
            py, px = int(round(gaze[i][0] * (side - 1))), int(round(gaze[i][1] * (side - 1)))
            best = None
            for r in gt[i * per:(i + 1) * per]:
                im = Image.new("L", (side, side), 0)
                ring = r["segmentation"][0]
                ImageDraw.Draw(im).polygon([(round(ring[2 * k]), round(ring[2 * k + 1])) for k in range(len(ring) // 2)], fill=1, outline=1)
                m = np.asarray(im)
                if m[py, px] and (best is None or int(m.sum()) < best[0]):
                    best = (int(m.sum()), r)
            keep.append(best[1] if best else {"image_id": i, "category_id": -1, "segmentation": {"size": [side, side], "counts": [side * side]}})
        return T.score_coco_records(dt, keep, T.InstanceAPMeter("cuda", 51), images=images)

    routes = {"gaze_ms": lambda: T.score_coco_records(dt, gt, T.InstanceAPMeter("cuda", 51), images=images, gaze=gaze),
              "host_prefilter_ms": prefilter}
    routes["gaze_ms"]()
    rounds = [{k: round(wall(fn)[0], 2) for k, fn in routes.items()} for _ in range(3)]
    res["score_coco_records"] = {"images": n, "side": side, "annotations_per_image": per, "rounds": rounds}
    print(json.dumps(res["score_coco_records"]), flush=True)
    if args.parent_lib:
        res["module"] = module_routes(args.parent_lib, B)
        print(json.dumps(res["module"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
