#!/usr/bin/env python3
"""Record the SHA-256 of every persistent weight pack fs_conv2d_pack writes for PACK_CASES, in bf16x3 and f16x2, forward and bwd-data
(needs the GPU: the pack is a kernel launch).

Usage: python tools/record_conv_pack_hashes.py OUT.json      (the library of this tree, or the one FS_HIP_LIB names)
       python tools/record_conv_pack_hashes.py --choices     (CPU: print the fs_conv2d_kernel_choice ids of PACK_CASES)

tests/test_hip_kernels.py imports PACK_CASES, PACK_CHOICE and pack_hashes() from here: test_persistent_weight_pack runs the cases and
asserts the ids, test_weight_pack_bytes_match_recorded_hashes compares pack_hashes() of the library beside it with
tests/golden/conv_pack_hashes.json.  The fixture was recorded from the library as it stood before the families' pack-then-run steps moved
into fs_pack_then_run (csrc/conv_run.h), so a differing hash is a pack whose bytes changed.  The weights come from numpy's PCG64 with a
fixed seed per case and the scratch is pre-filled with 0xA5, so the hashes depend on the library alone."""
import hashlib
import json
import os
import sys

# B, H, W, Cin, Cout, k, stride
PACK_CASES = [
    (4, 16, 16, 64, 64, 3, 1),       # W % 4 == 0: F(4,3) kernel in bf16x3, halo-tiled kernel in f16x2 (K < 128)
    (2, 15, 15, 64, 64, 3, 1),       # halo-tiled kernel (odd width)
    (2, 20, 20, 256, 256, 3, 1),     # W % 4 == 0, K >= 128: F(4,3) in bf16x3, F(2,3) in f16x2
    (4, 16, 16, 64, 128, 3, 2),      # stride 2: parity-plane forward, four-parity bwd-data
    (4, 16, 16, 64, 256, 1, 1),      # 1x1 GEMM kernel
    (2, 16, 16, 32, 64, 5, 1),       # tap-class kernel (5x5)
    (2, 16, 16, 64, 64, 3, 3),       # stride 3: bwd-data re-packs per parity class -> no persistent pack
    (2, 18, 18, 64, 64, 3, 1),       # even width, no multiple of 4: four-wave F(2,3) form in bf16x3
    (2, 18, 18, 256, 128, 3, 1),     # the same width with Cs >= 256, Cd > 64: eight-wave F(2,3) form in bf16x3; F(2,3) in f16x2
    (2, 16, 16, 64, 64, 3, 4),       # stride >= filter: forward = gather GEMM (persistent pack), bwd-data = scatter route (none)
]
# What each case is there for: the fs_conv2d_kernel_choice id (include/fovealseg.h) with the scratch fs_conv2d_workspace_bytes asks for,
# as {precision mode: (forward, bwd-data)}.  Derived on the CPU (the query launches nothing) from the library as it stood before
# fs_pack_then_run; test_persistent_weight_pack asserts them, so a case cannot drift to another route unnoticed.
PACK_CHOICE = dict(zip(PACK_CASES, [
    {"bf16x3": (8, 8), "f16x2": (2, 2)},
    {"bf16x3": (2, 2), "f16x2": (2, 2)},
    {"bf16x3": (8, 8), "f16x2": (5, 5)},
    {"bf16x3": (7, 6), "f16x2": (7, 6)},
    {"bf16x3": (4, 4), "f16x2": (4, 4)},
    {"bf16x3": (3, 3), "f16x2": (3, 3)},
    {"bf16x3": (4, 1), "f16x2": (4, 1)},      # forward: gather GEMM; bwd-data: one sub-problem per parity class
    {"bf16x3": (5, 5), "f16x2": (2, 2)},
    {"bf16x3": (5, 5), "f16x2": (5, 5)},
    {"bf16x3": (4, 1), "f16x2": (4, 1)},      # bwd-data: one GEMM per tap, scattered
]))
PRECISIONS = ("bf16x3", "f16x2")


def geometry(case):
    """The 12 shape arguments of the C ABI (B, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil) of a PACK_CASES entry."""
    B, H, W, Ci, Co, k, s = case
    pad = k // 2
    return (B, H, W, Ci, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1, Co, k, k, s, pad, 1)


def case_key(case, prec, transposed):
    return "%s|%s|%s" % (",".join(map(str, case)), prec, "bwd_data" if transposed else "fwd")


def choices(hip):
    """{case: {prec: (forward id, bwd-data id)}} from the library's host-side query.  Leaves the precision mode as it found it."""
    lib = hip.load()
    saved = lib.fs_get_conv_precision()
    out = {}
    try:
        for case in PACK_CASES:
            shape = geometry(case)
            out[case] = {}
            for prec in PRECISIONS:
                hip.set_conv_precision(prec)
                out[case][prec] = tuple(int(lib.fs_conv2d_kernel_choice(*shape, tr, hip.conv_workspace_bytes(*shape[1:], tr)))
                                        for tr in (0, 1))
    finally:
        lib.fs_set_conv_precision(saved)
    return out


def pack_hashes(hip):
    """{case_key: sha256 hex} of the scratch after fs_conv2d_pack, for every case x precision x direction whose pack is persistent."""
    import numpy as np
    import torch
    lib = hip.load()
    saved = lib.fs_get_conv_precision()
    out = {}
    try:
        for i, case in enumerate(PACK_CASES):
            B, H, W, Ci, Co, k, s = case
            shape = geometry(case)
            w = np.random.Generator(np.random.PCG64(1000 + i)).standard_normal((k, k, Ci, Co)).astype(np.float32) / np.float32(k * Ci ** 0.5)
            wd = torch.from_numpy(w).to("cuda")
            for prec in PRECISIONS:
                hip.set_conv_precision(prec)
                for tr in (0, 1):
                    n = hip.conv_workspace_bytes(*shape[1:], tr)
                    if n == 0 or not int(lib.fs_conv2d_pack_persistent(*shape, tr, n)):
                        continue
                    ws = torch.full((n,), 0xA5, device="cuda", dtype=torch.uint8)
                    hip.call("fs_conv2d_pack", hip.ptr(wd), *shape, tr, hip.ptr(ws), n, None)
                    out[case_key(case, prec, tr)] = hashlib.sha256(ws.cpu().numpy().tobytes()).hexdigest()
    finally:
        lib.fs_set_conv_precision(saved)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fovealseg import hip
    if sys.argv[1] == "--choices":
        for case, ids in choices(hip).items():
            print(case, ids)
    else:
        hashes = pack_hashes(hip)
        with open(sys.argv[1], "w") as f:
            json.dump(hashes, f, indent=1, sort_keys=True)
            f.write("\n")
        print(len(hashes), "packs")
