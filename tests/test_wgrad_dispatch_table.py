"""CPU tests of the bwd-weight plan (csrc/conv_wgrad.hip fs_wgrad_plan) through its query fs_conv2d_bwd_weight_plan: the slab cap, a
recorded table over the grid of tools/record_wgrad_dispatch.py, and the launches the library made before the plan existed
(no launch, no GPU)."""
import json
import os
import re
import sys

import numpy as np
import pytest

from fovealseg import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_wgrad_dispatch as rec      # noqa: E402  (the grid is defined once, beside the recorder)

ROUTE = {name: i for i, name in enumerate(rec.ROUTES)}
ACCUM = {name: i for i, name in enumerate(rec.ACCUMS)}


@pytest.fixture(scope="module")
def rows():
    """Every (mode, deterministic, shape, ws_full, ws_bytes, plan) of the grid, asked once for the tests below."""
    lib = hip.load()
    saved = lib.fs_get_conv_precision(), lib.fs_get_deterministic()
    out = list(rec.walk(lib))
    assert (lib.fs_get_conv_precision(), lib.fs_get_deterministic()) == saved
    return out


def _slab_bytes(shape):
    B, H, W, Cin, Ho, Wo, Cout, R, S = shape[:9]
    return R * S * Cin * Cout * 4


def test_plan_slabs_fit_the_scratch_the_library_asks_for(rows):
    """fs_wgrad_slab_cap is a bound of the split counts the plan chooses: wherever the plan claims slab rows, that many slabs fit in
    fs_conv2d_bwd_weight_ws_bytes of the same mode.  Until the plan existed only a comment said so.

    The linear kernel's gathered-row target (1024 / taps workgroups, whatever the tile) exceeds the cap on 128 x 128 tiles -- bf16x3,
    1x1 / stride 2 or 4, more than 64 channels on both sides: 730 splits against a cap of 514 for 128 -> 128 at B = 2800, 40x40 -- so
    the plan bounds that kernel's split count by the cap wherever the splits go to slabs (46 problems of this grid)."""
    claims = [r for r in rows if r[5][6] > 0]
    assert len(claims) >= 10000
    bad = [r for r in claims if r[5][6] * _slab_bytes(r[2]) > r[3]]
    assert not bad, f"{len(bad)} of {len(claims)} rows claim more slabs than the scratch holds; first (mode, det, shape, ws_full, ws, plan): {bad[0]}"


def test_plan_accepts_the_scratch_the_library_asks_for(rows):
    """Wherever the claimed slabs fit fs_conv2d_bwd_weight_ws_bytes and exactly that much scratch is given, the launch is accepted."""
    asked = [r for r in rows if r[5][6] > 0 and r[4] == r[3] and r[5][6] * _slab_bytes(r[2]) <= r[3]]
    assert len(asked) >= 10000
    bad = [r for r in asked if r[5][0] != 1]
    assert not bad, f"{len(bad)} rows refused; first (mode, det, shape, ws_full, ws, plan): {bad[0]}"


def test_wgrad_dispatch_matches_recorded_table(golden, rows):
    """fs_conv2d_bwd_weight_ws_bytes and every int of fs_conv2d_bwd_weight_plan over the grid of tools/record_wgrad_dispatch.py -- three
    precision modes, deterministic mode off and on, no / the asked-for / ample scratch -- reproduce tests/golden/wgrad_dispatch_table.npz
    exactly.  The table was recorded when the plan was introduced, after its routes, launch counts and workgroups had been compared with
    the launches of the library before it (test below): any difference is a problem whose kernel, split count, accumulation or slab
    count changed.  (Shipped library only: a -DFS_EXPERIMENTS build with a kernel switched off answers differently.)"""
    want = golden("wgrad_dispatch_table")["table"]
    assert want.dtype == np.int64 and want.shape[1] == len(rec.COLUMNS)

    # the stored table is not hollow: every route and every accumulation kind the query can report occurs often
    # (kind 1, atomics into an accumulating dW, belongs to calls with accumulate != 0; the query has no such argument)
    col = {name: want[:, i] for i, name in enumerate(rec.COLUMNS)}
    ids, counts = np.unique(col["route"], return_counts=True)
    assert ids.tolist() == list(range(len(rec.ROUTES))) and counts.min() >= 100, dict(zip(ids.tolist(), counts.tolist()))
    ids, counts = np.unique(col["accum"], return_counts=True)
    assert ids.tolist() == [ACCUM["atomic_zeroed"], ACCUM["slabs_zeroed"], ACCUM["slabs_stored"]] and counts.min() >= 100
    assert set(np.unique(col["ok"]).tolist()) == {0, 1} and int(col["ok"].sum()) >= 1000 and int((col["ok"] == 0).sum()) >= 1000
    assert int((col["launches"] > 1).sum()) >= 1000 and int((col["slabs"] > 0).sum()) >= 1000

    got = np.asarray([(full, ws) + ans for _, _, _, full, ws, ans in rows], dtype=np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (f"{bad.size} rows differ; first: row {bad[0]}, columns {rec.COLUMNS}, "
                           f"got {got[bad[0]].tolist()}, recorded {want[bad[0]].tolist()}")


# kernel of a recorded launch -> the routes that launch it (the linear kernel serves plain and gathered rows)
KERNEL_ROUTES = [
    (r"^conv_wgrad_kernel<false>$", {ROUTE["generic"]}),
    (r"^conv_wgrad_kernel<true>$", {ROUTE["generic_vec"]}),
    (r"^conv_wgrad_taps_kernel<3>$", {ROUTE["taps3"]}),
    (r"^conv_wgrad_taps_kernel<9>$", {ROUTE["taps9"]}),
    (r"^conv_wgrad_class_kernel<fs_split::Prec\w+, 3, 3>$", {ROUTE["class33"]}),
    (r"^conv_wgrad_wino_kernel<fs_split::PrecX3>$", {ROUTE["wino"]}),
    (r"^linear_wgrad_kernel<fs_split::PrecX3, \d, \d, \d, \d>$", {ROUTE["linear"], ROUTE["gather"]}),
    (r"^conv_wgrad_planes_kernel<fs_split::Prec\w+>$", {ROUTE["planes"]}),
    (r"^conv_wgrad_class_kernel<fs_split::Prec\w+, [12], [12]>$", {ROUTE["classes"]}),
]


def test_plan_reproduces_the_launches_before_it():
    """tests/golden/wgrad_parent_launches.json: the ordered (kernel, workgroups, threads) list of every fs_conv2d_bwd_weight call over a
    subgrid that reaches every route, precision mode and accumulation kind, recorded from a kernel trace of the library as it stood
    BEFORE kernel selection moved into fs_wgrad_plan.  The query names the same route, the same number of launches, the same workgroup
    sum and workgroup size for every problem in it."""
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_parent_launches.json")) as f:
        problems = json.load(f)["problems"]
    assert len(problems) >= 200
    lib = hip.load()
    saved = lib.fs_get_conv_precision(), lib.fs_get_deterministic()
    seen = set()
    try:
        for p in problems:
            assert lib.fs_set_conv_precision(p["mode"]) == 0 and lib.fs_set_deterministic(p["deterministic"]) == 0
            ok, route, accum, launches, workgroups, threads, slabs = rec.plan(lib, p["shape"], p["ws_bytes"])
            where = (p["shape"], p["mode"], p["deterministic"], p["ws_bytes"])
            assert ok == 1, where
            routes = []
            for name, wgs, thr in p["launches"]:
                hit = [r for pat, r in KERNEL_ROUTES if re.match(pat, name)]
                assert len(hit) == 1, (name, where)
                routes.append(hit[0])
                assert thr == threads, (where, name, thr, threads)
            assert all(route in r for r in routes), (where, route, p["launches"])
            assert len(p["launches"]) == launches, (where, launches, p["launches"])
            assert sum(wgs for _, wgs, _ in p["launches"]) == workgroups, (where, workgroups, p["launches"])
            seen.add((route, p["mode"] > 0, accum))
    finally:
        lib.fs_set_conv_precision(saved[0])
        lib.fs_set_deterministic(saved[1])
    assert {r for r, _, _ in seen} == set(range(len(rec.ROUTES)))
    assert {a for _, _, a in seen} == {ACCUM["atomic_zeroed"], ACCUM["slabs_zeroed"], ACCUM["slabs_stored"]}
