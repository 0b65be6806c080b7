"""What drawing the record onto the frame costs on one MI355X (fs_frame_overlay / _u8 / _hwc, ops.draw_instances, GazeSession.render).
Everything runs in ONE process, the sizes alternated over three rounds:

    (a) entry points   the three entry points (fp32, planar bytes, an RGBA view read where it lies) into a planar and into an RGBA
                       destination, every element of the style on (tint, outline band, box, marker, dim): device-event time over 20
                       back-to-back calls in microseconds a call, the bytes the rule says are moved a pixel (12, 3 or 4 read, 3 or 4
                       written, a bit of the mask and a bit of the band) and the rate in TB/s on those bytes, next to fs_gate_tiles_u8's
                       rate on its 6 bytes a pixel in the same round.  expected_us = the pass's bytes over that rate.
    (b) composition    what a caller had before: torch shifts unpack the bit words to a (B,H,W) mask, torch.where and an fp32 blend tint
                       it, permute().contiguous() makes the display's HWC bytes (no outline, box or marker: less than (a) draws); its time and
                       the rise of the allocator's peak, beside the pass's.
    (c) session        GazeSession.render (RGBA in, RGBA out, outline_px 0 and 3) beside a REUSE step on the same frame, host wall time
                       in ms ending in a device synchronise (the step ends in its own read-back).  --no-session leaves it out (no network is built).

    python tools/overlay_bench.py [--sizes 64:1024,1:1024] [--rounds 3] [--no-session] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

from gaze_session_bench import wall
from motion_bench import event_us


def peak_of(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def record(B, side, g):
    """A blob a viewer as bit words, its stats, a gaze inside it, live flags, and the band of an outline three pixels wide."""
    y, x = torch.meshgrid(torch.arange(side, device="cuda"), torch.arange(side, device="cuda"), indexing="ij")
    cy = torch.randint(side // 4, 3 * side // 4, (B, 1, 1), device="cuda", generator=g)
    cx = torch.randint(side // 4, 3 * side // 4, (B, 1, 1), device="cuda", generator=g)
    mask = ((y[None] - cy) ** 2 + ((x[None] - cx) * 2 // 3) ** 2) < (side // 5) ** 2
    bits = ops.mask_bits(mask)
    stats, _ = ops.mask_rle(bits, side, max_runs=8)
    focus = torch.cat([cy.view(B, 1), cx.view(B, 1)], 1).float() / (side - 1)
    band = ops.overlay_band(bits, side, 3)[0]
    live = torch.ones(B, 6, dtype=torch.int64, device="cuda")
    return mask, bits, band, stats, focus, live


def composition(U, bits, tint, alpha):
    """The caller's route before this pass: unpack, blend in fp32, permute to the display's layout."""
    B, _, H, W = U.shape
    sh = torch.arange(32, device=U.device, dtype=torch.int32)
    mask = ((bits[..., None] >> sh) & 1).view(B, H, -1)[:, :, :W].bool()
    x = U.float()
    t = torch.tensor(tint, device=U.device, dtype=torch.float32).view(1, 3, 1, 1)
    out = torch.where(mask[:, None], x * (1 - alpha / 256) + t * (alpha / 256), x)
    return out.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def entry_points(B, side, rounds):
    g = torch.Generator(device="cuda").manual_seed(B * 7 + side)
    U = torch.randint(0, 256, (B, 3, side, side), device="cuda", dtype=torch.uint8, generator=g)
    key = torch.randint(0, 256, (B, 3, side, side), device="cuda", dtype=torch.uint8, generator=g)
    X = (U.cpu().float() / 255).cuda()
    cam = torch.randint(0, 256, (B, side, side, 4), device="cuda", dtype=torch.uint8, generator=g)
    cam[..., :3] = U.permute(0, 2, 3, 1)
    rgba = cam.permute(0, 3, 1, 2)[:, :3]
    mask, bits, band, stats, focus, live = record(B, side, g)
    del mask
    style = ops.overlay_style(tint=(255, 64, 0), alpha=96, outline=(255, 255, 0), box=(0, 128, 255), box_px=2, marker=(255, 255, 255), marker_px=9,
                              marker_width=3, dim=176, device="cuda")
    planar = torch.empty(B, 3, side, side, device="cuda", dtype=torch.uint8)
    disp = torch.empty(B, side, side, 4, device="cuda", dtype=torch.uint8)
    dests = {"planar": (planar, 3), "rgba": (disp.permute(0, 3, 1, 2)[:, :3], 4)}
    sad = torch.empty(B, side // 32, side // 32, device="cuda", dtype=torch.int32)
    px = B * side * side
    calls = {"gate_tiles_u8": (lambda: ops.gate_tiles_u8(U, key, 32, out=sad), 6.0)}
    for sname, src, rd in (("fp32", X, 12), ("u8", U, 3), ("hwc_rgba", rgba, 4)):
        for dname, (out, wr) in dests.items():
            calls[f"{sname}->{dname}"] = (lambda src=src, out=out: ops.draw_instances(src, bits, stats=stats, focus=focus, style=style, out=out,
                                                                                       live=live[:, 0], band=band), rd + wr + 0.25)
    calls["hwc_rgba in place"] = (lambda: ops.draw_instances(rgba, bits, stats=stats, focus=focus, style=style, out=rgba, live=live[:, 0], band=band), 8.25)
    calls["torch composition -> hwc"] = (lambda: composition(U, bits, (255, 64, 0), 96), None)
    # the three routes give one picture
    a = ops.draw_instances(U, bits, stats=stats, focus=focus, style=style, live=live[:, 0], band=band)
    equal = all(bool(torch.equal(a, ops.draw_instances(s, bits, stats=stats, focus=focus, style=style, live=live[:, 0], band=band))) for s in (X, rgba))
    ops.draw_instances(rgba, bits, stats=stats, focus=focus, style=style, out=dests["rgba"][0], live=live[:, 0], band=band)
    equal &= bool(torch.equal(disp[..., :3].permute(0, 3, 1, 2), a)) and bool((disp[..., 3] == 255).all())
    del a
    out = []
    for _ in range(rounds):
        row = {}
        for k, (fn, bpp) in calls.items():
            us = event_us(fn)
            row[k] = {"us": round(us, 2)}
            if bpp is not None:
                row[k]["TBps"] = round(bpp * px / us / 1e6, 3)
        rate = row["gate_tiles_u8"]["TBps"]
        for k, (fn, bpp) in calls.items():
            if bpp is not None and k != "gate_tiles_u8":
                row[k]["expected_us"] = round(bpp * px / rate / 1e6, 2)
        out.append(row)
    peaks = {"u8->rgba": peak_of(calls["u8->rgba"][0]), "torch composition -> hwc": peak_of(calls["torch composition -> hwc"][0])}
    return {"batch": B, "side": side, "bytes_per_pixel": {k: v[1] for k, v in calls.items()}, "routes_equal": equal, "rounds": out, "peak_rise_bytes": peaks}


def session(module, B, side, rounds, iters=10):
    X0, Fp, _Y, _cl = T.synthetic_batch(B, side, side, seed=1, device="cuda")
    U = (X0.clamp(0, 1) * 255).round().to(torch.uint8)
    del X0, _Y
    cam = torch.full((B, side, side, 4), 255, device="cuda", dtype=torch.uint8)
    cam[..., :3] = U.permute(0, 2, 3, 1)
    view = cam.permute(0, 3, 1, 2)[:, :3]
    disp = torch.empty_like(cam)
    out = disp.permute(0, 3, 1, 2)[:, :3]
    s = fovealseg.GazeSession(module, B, (side, side))
    style = ops.overlay_style(outline=(255, 255, 0), box=(0, 128, 255), marker=(255, 255, 255), dim=176, device="cuda")
    assert s.step(view, Fp)[4][:, 0].tolist() == [1] * B
    routes = {"step_reuse": (lambda: s.step(view, Fp), False), "render": (lambda: s.render(view, focus=Fp, style=style, out=out), True),
              "render_outline3": (lambda: s.render(view, focus=Fp, style=style, outline_px=3, out=out), True)}
    for fn, _ in routes.values():
        fn()
    res = []
    for _ in range(rounds):
        ms = {k: [] for k in routes}
        for _it in range(iters):
            for k, r in routes.items():
                ms[k].append(wall(*r)[0])
        res.append({k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()})
    us = {k: round(event_us(routes[k][0]), 2) for k in ("render", "render_outline3")}
    return {"batch": B, "side": side, "iters": iters, "rounds": res, "render_device_us": us, "render_peak_rise_bytes": peak_of(routes["render"][0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64:1024,1:1024", help="batch:side pairs")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-session", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "overlay_bench measures on the GPU"
    hip.load()
    sizes = [tuple(int(v) for v in spec.split(":")) for spec in args.sizes.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "entry_points": [], "session": []}
    with torch.no_grad():
        for rnd in range(args.rounds):                      # the sizes alternate: a round of each, three times
            for B, side in sizes:
                row = entry_points(B, side, 1)
                row["round"] = rnd
                res["entry_points"].append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
        if not args.no_session:
            module, _ = T.build_module(fovealseg.lvis50_cfg(), device="cuda")
            module.eval()
            ops.static_weight_packs(module)
            module.decoder.cls_net.fc.bias[-1] += 1000.0  # as gaze_session_bench: a large background logit lets the mask plane draw a blob
            for B, side in sizes:
                row = session(module, B, side, args.rounds)
                res["session"].append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
