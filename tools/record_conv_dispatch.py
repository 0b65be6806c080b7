#!/usr/bin/env python3
"""Record every host-side answer of the forward / bwd-data conv dispatch over a grid of problems, in all three precision modes
(CPU only: the queries launch nothing and the library loads without a GPU).

Usage: python tools/record_conv_dispatch.py OUT.npz      (the library of this tree; built with the shipped flags, no A/B switches)

tests/test_conv_dispatch_table.py imports the grid and table() from here and compares the library beside it with
tests/golden/conv_dispatch_table.npz, row by row.  The fixture holds answers only: one int64 row per (mode, problem, ws_bytes) in the
order table() walks them, columns COLUMNS.  It is written with fixed zip timestamps, so that recording twice from the same library
gives the same bytes."""
import itertools
import os
import sys
import zipfile

import numpy as np

# (R = S, stride, pad, dil)
FILT = [(1, 1, 0, 1), (1, 2, 0, 1), (1, 4, 0, 1), (3, 1, 1, 1), (3, 2, 1, 1), (3, 4, 1, 1), (3, 3, 1, 1), (3, 1, 2, 2), (3, 1, 4, 4),
        (3, 1, 0, 1), (5, 1, 2, 1), (7, 2, 3, 1), (2, 2, 0, 1), (4, 4, 0, 1)]
CH = [(3, 64), (64, 64), (64, 256), (256, 64), (16, 16), (18, 36), (48, 96), (128, 128), (256, 256), (960, 512), (720, 720), (64, 51),
      (12, 20), (32, 32), (2048, 512), (28, 32)]
# the last two: an even width that is no multiple of 4 (F(2,3), not F(4,3)) and a small multiple of 4
HW = [(80, 80), (81, 81), (10, 10), (20, 20), (40, 40), (7, 9), (160, 160), (256, 256), (2, 2), (128, 6), (22, 22), (12, 12)]
BS = [1, 2, 64, 2800]
COLUMNS = ("ws_full", "ws_bytes", "kernel_choice", "pack_persistent", "stats_slabs", "bwd_data_bnsum_slabs", "fwd_affine_act_ok",
           "fwd_residual_ok")


def problems():
    """(B, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil, transposed) of every grid point with a positive output size."""
    for (R, st, pad, dil), (ci, co), (H, W), B, tr in itertools.product(FILT, CH, HW, BS, (0, 1)):
        Ho = (H + 2 * pad - dil * (R - 1) - 1) // st + 1
        Wo = (W + 2 * pad - dil * (R - 1) - 1) // st + 1
        if Ho > 0 and Wo > 0:
            yield B, H, W, ci, Ho, Wo, co, R, R, st, pad, dil, tr


def table(lib):
    """The answers of `lib` (fovealseg.hip.load()) as an int64 array [rows][len(COLUMNS)].  Leaves the precision mode as it found it."""
    out = []
    saved = lib.fs_get_conv_precision()
    try:
        for mode in (0, 1, 2):
            assert lib.fs_set_conv_precision(mode) == 0
            for p in problems():
                B, H, W = p[:3]
                shape, tr = p[:12], p[12]
                full = int(lib.fs_conv2d_workspace_bytes(*shape[1:], tr))
                rows_per_sample = H * W if H * W >= 128 else B * H * W
                for ws in sorted({0, full // 2, max(full - 1, 0), full, 1 << 30}):
                    out.append((full, ws,
                                lib.fs_conv2d_kernel_choice(*shape, tr, ws), lib.fs_conv2d_pack_persistent(*shape, tr, ws),
                                lib.fs_conv2d_stats_slabs(*shape, ws), lib.fs_conv2d_bwd_data_bnsum_slabs(*shape, ws),
                                lib.fs_conv2d_fwd_affine_act_ok(*shape, ws), lib.fs_conv2d_fwd_residual_ok(*shape, rows_per_sample, ws)))
    finally:
        lib.fs_set_conv_precision(saved)
    return np.asarray(out, dtype=np.int64)


def save(path, tab):
    with zipfile.ZipFile(path, "w") as z:
        info = zipfile.ZipInfo("table.npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        with z.open(info, "w", force_zip64=True) as f:
            np.lib.format.write_array(f, tab, allow_pickle=False)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fovealseg import hip
    tab = table(hip.load())
    save(sys.argv[1], tab)
    print(tab.shape, os.path.getsize(sys.argv[1]), "bytes")
    for col, name in enumerate(COLUMNS):
        v, c = np.unique(tab[:, col], return_counts=True)
        print(name, len(v), "distinct", dict(zip(v.tolist(), c.tolist())) if len(v) <= 12 else "")
