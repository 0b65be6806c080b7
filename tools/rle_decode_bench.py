"""What decoding run-length codes on the device costs on one MI355X: ops.rle_bits (fs_rle_bits) on (a) the head's own records and (b) a
worst-case code of 8 W + 1 runs, against the route a caller had before -- counts.cpu(), a numpy decode, an upload, ops.mask_bits --
with fs_mask_rle's time on the same masks beside it; then DeformSegmentationModule.evaluate_instances() fed the run-length label
against the dense label, with the peak allocation of each, and predict_instances() through the parent commit's library against this
one's.  Everything runs in ONE process, the routes alternating, in three rounds.

    python tools/rle_decode_bench.py [--sizes 64:1024] [--warmup 3] [--iters 10] [--op-reps 20] [--host-reps 2] [--parent-lib FILE.so] [--out FILE.json]

Device passes are event times over --op-reps back-to-back calls on preallocated buffers, in microseconds a call; "bytes" is what the
decoder must move at the least -- the counts read (4 B a run), the ends written and read back once (8 B a run), the words written
(Hs * P * 4 B an image) and the info rows -- and the rate is taken on those bytes.  Routes are host wall time in ms ending with a device
synchronise, median (min - max) per round.  --parent-lib as tools/instance_eval_bench.py takes it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

import instance_eval_bench as IE
from instance_eval_bench import peak_over_start, stats, timed

NEW = ("fs_rle_bits",)                                   # what the parent's library does not have


def host_route(counts, n_runs, side):
    """What a caller did before: the codes to the host, a numpy decode (np.repeat of 0, 1, 0, ... by the counts, column-major), the
    bool masks back to the device, ops.mask_bits."""
    c, n = counts.cpu().numpy(), n_runs.cpu().tolist()
    masks = np.empty((len(n), side, side), dtype=bool)
    for b, k in enumerate(n):
        v = np.repeat(np.arange(k) & 1, c[b, :k]).astype(bool)
        masks[b] = v.reshape(side, side).T
    return ops.mask_bits(torch.from_numpy(masks).cuda())


def worst_case(B, side):
    """8 W + 1 runs: every column is entered and left four times (nine bands of rows, the second, fourth, sixth and eighth set; a
    column begins and ends unset, so no run continues into the next)."""
    m = torch.zeros(B, side, side, dtype=torch.bool, device="cuda")
    band = torch.clamp(torch.arange(side, device="cuda") // (side // 9), max=8)
    m[:, band % 2 == 1, :] = True
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64:1024", help="batch:side pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--op-reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rle_decode_bench measures on the GPU"
    hip.load()
    module, _ = T.build_module(fovealseg.lvis50_cfg(), device="cuda")
    module.eval()
    ops.static_weight_packs(module)
    with torch.no_grad():
        module.decoder.cls_net.fc.bias[-1] += 1000.0     # a large background logit lets the mask plane draw a blob (tools/component_bench.py)
    IE.NEW = NEW
    parent = IE.ParentLibrary(args.parent_lib) if args.parent_lib else None
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": hip.get_conv_precision(),
           "workload": "HRNetV2-nodownsp + C1, K = 51, eval, static weight packs; input side^2 -> 80^2 grid -> record at side^2", "sizes": []}
    with torch.no_grad():
        for spec in args.sizes.split(","):
            B, side = (int(v) for v in spec.split(":"))
            P = (side + 31) // 32
            X, Fp, Y, cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
            _cat, hstats, hcounts, hbits = module.predict_instances(X, Fp, return_bits=True)
            wbits = ops.mask_bits(worst_case(B, side))
            wstats, wcounts = ops.mask_rle(wbits, side)
            assert wstats[:, 5].tolist() == [8 * side + 1] * B
            row = {"batch": B, "side": side, "decode": {}}
            for name, (st, counts, bits) in {"head": (hstats, hcounts, hbits), "worst": (wstats, wcounts, wbits)}.items():
                cap = int(counts.shape[1])
                runs = int(st[:, 5].sum())
                out = torch.empty(B, side, P, device="cuda", dtype=torch.int32)
                info = torch.empty(B, 4, device="cuda", dtype=torch.int64)
                scr = torch.empty(hip.query("fs_rle_bits_scratch_ints", B, cap), device="cuda", dtype=torch.int32)
                st2, c2 = torch.empty_like(st), torch.empty_like(counts)
                scr_e = torch.empty(hip.query("fs_mask_rle_scratch_ints", B, side, side), device="cuda", dtype=torch.int32)

                def decode():
                    hip.call("fs_rle_bits", counts.data_ptr(), st.data_ptr() + 40, 6, out.data_ptr(), info.data_ptr(), scr.data_ptr(), B, side, side, cap)

                def encode():
                    hip.call("fs_mask_rle", bits.data_ptr(), st2.data_ptr(), c2.data_ptr(), scr_e.data_ptr(), B, side, side, cap)
                decode(), encode()
                moved = 12 * runs + B * side * P * 4 + B * 32
                entry = {"runs_total": runs, "runs_max": int(st[:, 5].max()), "cap": cap, "bytes_moved": moved, "rounds": []}
                for _ in range(3):                        # the routes take turns within a round
                    us_d = timed(decode, args.op_reps)[0] * 1e3
                    us_e = timed(encode, args.op_reps)[0] * 1e3
                    us_o = timed(lambda: ops.rle_bits(counts, st, (side, side)), args.op_reps)[0] * 1e3
                    ms_h = [timed(lambda: host_route(counts, st[:, 5], side))[0] for _ in range(args.host_reps)]
                    entry["rounds"].append({"fs_rle_bits_us": round(us_d, 2), "GBps": round(moved / us_d / 1e3, 1), "ops_rle_bits_us": round(us_o, 2),
                                            "fs_mask_rle_us": round(us_e, 2), "host_route_ms": [round(v, 2) for v in ms_h]})
                entry["equal"] = bool(torch.equal(out, bits)) and bool(torch.equal(host_route(counts, st[:, 5], side), bits)) \
                    and bool(torch.equal(c2, counts)) and info[:, 0].tolist() == [0] * B
                entry["scratch_bytes"] = scr.numel() * 4
                row["decode"][name] = entry
                print(json.dumps({name: entry}), flush=True)
                del out, info, scr, st2, c2, scr_e
            lstats, lcounts = ops.mask_rle(Y[:, 0] != 0)
            lcounts = lcounts[:, :int(lstats[:, 5].max())].contiguous()
            routes = {"predict_instances": lambda: module.predict_instances(X, Fp, return_bits=True, return_score=True),
                      "evaluate_dense": lambda: module.evaluate_instances(X, Fp, Y, cl),
                      "evaluate_rle": lambda: module.evaluate_instances(X, Fp, (lcounts, lstats), cl, seg_size=(side, side))}
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
            same = lambda a, b: all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,                      # noqa: E731
                                                y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
            row["evaluate_equal"] = same(routes["evaluate_dense"](), routes["evaluate_rle"]())
            if parent is not None:
                row["parent_equal"] = same(routes["predict_instances"](), routes["predict_instances_parent"]())
            row["label_bytes"] = {"dense_fp32": Y.numel() * 4, "dense_int64": Y.numel() * 8, "rle": lcounts.numel() * 4 + lstats.numel() * 8}
            row["peak_bytes_over_start"] = {k: peak_over_start(routes[k]) for k in ("predict_instances", "evaluate_dense", "evaluate_rle")}
            res["sizes"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "decode"}), flush=True)
            del X, Fp, Y, cl, hbits, wbits
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
