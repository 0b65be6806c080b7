"""What rasterising polygon lists on the device costs on one MI355X: fs_poly_bits / ops.poly_bits at B = 64 on five cases -- one ring of
64 vertices and five rings of 400 at 640^2 and 1024^2, and one 4096-vertex zigzag at 1024^2 -- against the route a caller had before:
PIL.ImageDraw.polygon per image on the host, an upload, ops.mask_bits.  PIL's rule differs from this library's along the outline, so
that comparison is of time only.  Then train.score_coco_records with polygon ground truth (images=...) against the same ground truth
as run-length codes.  Everything runs in ONE process, the routes alternating, in three rounds.

    python tools/poly_bench.py [--batch 64] [--op-reps 20] [--host-reps 2] [--kernel-only] [--out FILE.json]

Device passes are event times over --op-reps back-to-back calls on preallocated buffers and tables already on the device, in
microseconds a call; ops.poly_bits includes polygon_rings' tables going up (one copy) and the allocations.  Routes are host wall
time in ms ending with a device synchronise.  --kernel-only prints the fs_poly_bits times alone: run under a kernel A/B build
(FS_BUILD_EXPERIMENTS=1 python build.py; FS_HIP_LIB=ab/libfovealseg_experiments.so) with FS_POLY_SKIP=1 / 3 it leaves out the scan /
the scan and the edge pass, which splits the kernel's time; FS_POLY_BAND / FS_POLY_WORDS change the band plan."""
import argparse
import json
import math
import os
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


def blob(rng, side, n, radius):
    """A wobbling closed outline of n vertices around a random centre, as a COCO polygon [x0, y0, ...]."""
    cy, cx = rng.uniform(0.3, 0.7, 2) * side
    r = radius * (1.0 + 0.25 * np.sin(np.arange(n) * (2 * math.pi * 5 / n) + rng.uniform(0, 6)) + rng.uniform(-0.05, 0.05, n))
    t = np.arange(n) * (2 * math.pi / n)
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1).round(2).reshape(-1).tolist()


def zigzag(side, n):
    x = np.arange(n) * ((side - 1) / (n - 1))
    y = np.where(np.arange(n) % 2 == 0, 0.0, side - 1.0)
    return np.stack([x, y], 1).round(2).reshape(-1).tolist()


def cases(B, rng):
    out = []
    for side in (640, 1024):
        out.append((f"{side}^2, 1 ring of 64", side, [[blob(rng, side, 64, side * 0.2)] for _ in range(B)]))
        out.append((f"{side}^2, 5 rings of 400", side, [[blob(rng, side, 400, side * rng.uniform(0.05, 0.25)) for _ in range(5)] for _ in range(B)]))
    out.append(("1024^2, one 4096-vertex zigzag", 1024, [[zigzag(1024, 4096)] for _ in range(B)]))
    return out


def host_route(polys, side):
    """What a caller did before: PIL draws every image's polygons on the host, the masks go up, ops.mask_bits packs them."""
    from PIL import Image, ImageDraw
    masks = np.empty((len(polys), side, side), dtype=np.uint8)
    for b, rings in enumerate(polys):
        im = Image.new("L", (side, side), 0)
        draw = ImageDraw.Draw(im)
        for ring in rings:
            draw.polygon([(round(ring[2 * i]), round(ring[2 * i + 1])) for i in range(len(ring) // 2)], fill=1, outline=1)
        masks[b] = np.asarray(im)
    return ops.mask_bits(torch.from_numpy(masks).cuda())


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--op-reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "poly_bench measures on the GPU"
    hip.load()
    B = args.batch
    rng = np.random.default_rng(30)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "lib": os.environ.get("FS_HIP_LIB", "shipped"),
           "env": {k: v for k, v in os.environ.items() if k.startswith("FS_POLY_")}, "cases": []}
    for name, side, polys in cases(B, rng):
        P = (side + 31) // 32
        tables = ops.polygon_rings(polys)
        verts, ring_off, img_ring = (t.cuda() for t in tables)
        V, R = int(verts.shape[0]), int(ring_off.numel()) - 1
        bits = torch.empty(B, side, P, device="cuda", dtype=torch.int32)
        info = torch.empty(B, 4, device="cuda", dtype=torch.int64)
        scr = torch.empty(hip.query("fs_poly_bits_scratch_ints", B, side, side), device="cuda", dtype=torch.int32)

        def kernel():
            hip.call("fs_poly_bits", verts.data_ptr(), ring_off.data_ptr(), img_ring.data_ptr(), bits.data_ptr(), info.data_ptr(), scr.data_ptr(),
                     B, R, V, side, side)
        kernel()
        entry = {"case": name, "side": side, "rings": R, "vertices": V, "band_rows": hip.query("fs_poly_bits_band_rows", side, side),
                 "words_bytes": B * side * P * 4, "rounds": []}
        for _ in range(3):                                # the routes take turns within a round
            row = {"fs_poly_bits_us": round(timed(kernel, args.op_reps)[0] * 1e3, 2)}
            if not args.kernel_only:
                row["ops_poly_bits_us"] = round(timed(lambda: ops.poly_bits(*tables, (side, side)), args.op_reps)[0] * 1e3, 2)
                row["polygon_rings_ms"] = round(min(_time_host(lambda: ops.polygon_rings(polys)) for _ in range(args.host_reps)), 2)
                row["host_route_ms"] = [round(wall(lambda: host_route(polys, side))[0], 2) for _ in range(args.host_reps)]
            entry["rounds"].append(row)
        entry["area_mean"] = float(info[:, 1].double().mean())
        if not args.kernel_only:
            pil = host_route(polys, side)
            diff = (pil ^ bits).view(torch.uint8)
            entry["pixels_differing_from_PIL_mean"] = float(sum(int(((diff >> k) & 1).sum()) for k in range(8))) / B
        res["cases"].append(entry)
        print(json.dumps(entry), flush=True)
        del bits, info, scr
    if not args.kernel_only:
        side, n = 1024, 256
        polys = [[blob(rng, side, 64, side * 0.2)] for _ in range(n)]
        gbits, _ = ops.poly_bits(*ops.polygon_rings(polys), (side, side))
        gstats, gcounts = ops.mask_rle(gbits, side)
        cat = torch.arange(n, device="cuda") % 50
        gt_rle = ops.instances_to_coco(cat, gstats, gcounts, (side, side), compressed=True)
        gt_poly = [dict(r, segmentation=p) for r, p in zip(gt_rle, polys)]
        dt = [dict(r, score=0.5) for r in gt_rle]
        images = [{"id": i, "height": side, "width": side} for i in range(n)]
        routes = {"rle_ground_truth": lambda: T.score_coco_records(dt, gt_rle, T.InstanceAPMeter("cuda", 51)),
                  "polygon_ground_truth": lambda: T.score_coco_records(dt, gt_poly, T.InstanceAPMeter("cuda", 51), images=images)}
        for fn in routes.values():
            fn()
        rounds = []
        for _ in range(3):
            rounds.append({k: round(wall(fn)[0], 2) for k, fn in routes.items()})
        a, b = T.InstanceAPMeter("cuda", 51), T.InstanceAPMeter("cuda", 51)
        T.score_coco_records(dt, gt_rle, a), T.score_coco_records(dt, gt_poly, b, images=images)
        res["score_coco_records"] = {"images": n, "side": side, "ms_rounds": rounds, "rows_equal": bool(torch.equal(torch.cat(a.rows), torch.cat(b.rows)))}
        print(json.dumps(res["score_coco_records"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def _time_host(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


if __name__ == "__main__":
    main()
