#!/usr/bin/env python3
"""Record the bwd-weight plan (fs_conv2d_bwd_weight_plan) over the grid of tools/record_conv_dispatch.py, in all three precision modes,
with deterministic mode off and on, without scratch, with the scratch fs_conv2d_bwd_weight_ws_bytes asks for, and with 1 GiB
(CPU only: the query launches nothing and the library loads without a GPU).

Usage: python tools/record_wgrad_dispatch.py OUT.npz      (the library of this tree; built with the shipped flags, no A/B switches)

tests/test_wgrad_dispatch_table.py imports the grid and table() from here and compares the library beside it with
tests/golden/wgrad_dispatch_table.npz, row by row.  One int64 row per (mode, deterministic, problem, ws_bytes) in the order table() walks
them, columns COLUMNS; the problem itself is not stored (problems() regenerates it).  Written as record_conv_dispatch.save does."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import record_conv_dispatch as fwd      # noqa: E402  (FILT x CH x HW x BS is defined once, there)

NOUT = 6
COLUMNS = ("ws_full", "ws_bytes", "ok", "route", "accum", "launches", "workgroups", "threads", "slabs")
ROUTES = ("generic", "generic_vec", "taps3", "taps9", "class33", "wino", "linear", "gather", "planes", "classes")
ACCUMS = ("atomic_zeroed", "atomic_add", "slabs_zeroed", "slabs_stored")


def problems():
    """(B, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil) of every grid point with a positive output size."""
    seen = set()
    for p in fwd.problems():
        if p[:12] not in seen:      # fwd.problems() has every problem once per direction
            seen.add(p[:12])
            yield p[:12]


def plan(lib, shape, ws_bytes):
    """(ok, route, accum, launches, workgroups, threads, slabs) of one problem under the library's current modes."""
    out = (ctypes.c_int * NOUT)()
    ok = lib.fs_conv2d_bwd_weight_plan(*shape, ws_bytes, out)
    return (ok,) + tuple(out)


def walk(lib):
    """(mode, deterministic, shape, ws_full, ws_bytes, plan) of every row, in table order.  Leaves both modes as it found them."""
    saved = lib.fs_get_conv_precision(), lib.fs_get_deterministic()
    probs = list(problems())
    try:
        for mode in (0, 1, 2):
            assert lib.fs_set_conv_precision(mode) == 0
            for det in (0, 1):
                assert lib.fs_set_deterministic(det) == 0
                for shape in probs:
                    Cin, Cout, R, S, stride, pad, dil = shape[3], shape[6], shape[7], shape[8], shape[9], shape[10], shape[11]
                    full = int(lib.fs_conv2d_bwd_weight_ws_bytes(Cin, Cout, R, S, stride, pad, dil))
                    for ws in sorted({0, full, 1 << 30}):
                        yield mode, det, shape, full, ws, plan(lib, shape, ws)
    finally:
        lib.fs_set_conv_precision(saved[0])
        lib.fs_set_deterministic(saved[1])


def table(lib):
    """The answers of `lib` (fovealseg.hip.load()) as an int64 array [rows][len(COLUMNS)]."""
    return np.asarray([(full, ws) + ans for _, _, _, full, ws, ans in walk(lib)], dtype=np.int64)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fovealseg import hip
    tab = table(hip.load())
    fwd.save(sys.argv[1], tab)
    print(tab.shape, os.path.getsize(sys.argv[1]), "bytes")
    for col, name in enumerate(COLUMNS):
        v, c = np.unique(tab[:, col], return_counts=True)
        print(name, len(v), "distinct", dict(zip(v.tolist(), c.tolist())) if len(v) <= 12 else "")
