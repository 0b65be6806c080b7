"""The scratch sizes of the un-warp / evaluation entry points (csrc/unwarp.hip: unwarp_plan) against the values recorded before the
layout had one owner, and the layout itself under sentinels on the GPU."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_unwarp_scratch as rec  # noqa: E402

from fovealseg import hip, ops  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unwarp_scratch_ints.json")


def test_scratch_sizes_equal_the_recorded_ones():
    with open(GOLD) as f:
        want = json.load(f)
    shapes = list(rec.shapes())
    assert len(shapes) == 4 * 3 * 3 * 6 and sorted(want) == sorted(rec.QUERIES)
    got = rec.answers(hip.load())
    for q in rec.QUERIES:
        assert len(want[q]) == len(shapes)
        bad = [(s, w, g) for s, w, g in zip(shapes, want[q], got[q]) if w != g]
        assert not bad, (q, len(bad), bad[:5])
        assert all(v == 0 for s, v in zip(shapes, got[q]) if s[0] == 0) and all(v > 0 for s, v in zip(shapes, got[q]) if s[0] > 0)


# ------------------------------------------------------------------------------------------------------------------ GPU: bounds ---
GUARD = 64
SENTINEL = -0x5A5A5A5B


def _guarded(ints):
    """(whole tensor, 16-byte aligned pointer of its first `ints` ints): the queried size plus GUARD sentinel ints."""
    t = torch.full((ints + GUARD,), SENTINEL, device="cuda", dtype=torch.int32)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", [(9, 7), (8, 8)])            # the scalar and the four-pixel count pass
def test_entry_points_stay_inside_the_scratch_they_ask_for(Hs, Ws):
    """Every entry point with the scratch its query asks for plus 64 sentinel ints: the sentinels survive, and a second call with
    fresh scratch writes the same outputs (nothing is read from beyond a region that was written)."""
    B, K, h, w, D = 2, 4, 4, 4, 2
    g = torch.Generator().manual_seed(11)
    cls = torch.randn(B, K, generator=g).cuda()
    m = (torch.rand(B, h, w, generator=g) - 0.5).cuda()
    grid = (torch.rand(B, h, w, 2, generator=g) * 2 - 1).cuda()
    y = (torch.rand(B, Hs, Ws, generator=g) < 0.4).float().cuda()
    cl = torch.randint(0, K - 1, (B,), generator=g).cuda()
    head = (cls.data_ptr(), m.data_ptr(), grid.data_ptr())
    dims = (B, K, h, w, Hs, Ws)

    def outputs(with_trim, with_labels, with_areas=False):
        o = {"counts": torch.zeros(B, 6, device="cuda", dtype=torch.int64), "acc": torch.zeros(4, device="cuda")}
        if with_trim:
            o["trim"] = torch.zeros(B, D + 1, 3, device="cuda", dtype=torch.int64)
        if with_labels:
            o["labels"] = torch.zeros(B, Hs, Ws, device="cuda", dtype=torch.int64)
        if with_areas:
            o["areas"] = torch.zeros(B, 3, K, 3, device="cuda", dtype=torch.int64)
        return o

    def p(o, k):
        return o[k].data_ptr() if k in o else None

    def run_labels(scr):
        o = {"labels": torch.zeros(B, Hs, Ws, device="cuda", dtype=torch.int64), "hole": torch.zeros(B, Hs, Ws, device="cuda", dtype=torch.bool)}
        hip.call("fs_unwarp_labels", *head, o["labels"].data_ptr(), o["hole"].data_ptr(), scr, *dims)
        return o

    def run_bands(scr):
        o = {"band": torch.zeros(B, Hs, Ws, device="cuda", dtype=torch.uint8)}
        hip.call("fs_trimap_bands", y.data_ptr(), o["band"].data_ptr(), scr, B, Hs, Ws, D, 1)
        return o

    def run_accuracy(with_labels):
        def run(scr):
            o = outputs(False, with_labels)
            hip.call("fs_unwarp_accuracy", *head, y.data_ptr(), cl.data_ptr(), p(o, "counts"), p(o, "acc"), p(o, "labels"), scr, *dims)
            return o
        return run

    def run_trimap(with_labels):
        def run(scr):
            o = outputs(True, with_labels)
            hip.call("fs_unwarp_trimap", *head, y.data_ptr(), cl.data_ptr(), p(o, "counts"), p(o, "acc"), p(o, "trim"), p(o, "labels"), scr, *dims, D, 1)
            return o
        return run

    def run_areas(with_trim, with_labels):
        def run(scr):
            o = outputs(with_trim, with_labels, True)
            hip.call("fs_unwarp_class_areas", *head, y.data_ptr(), cl.data_ptr(), p(o, "counts"), p(o, "acc"), p(o, "areas"), p(o, "trim"),
                     p(o, "labels"), scr, *dims, D, 1)
            return o
        return run

    cases = [("fs_unwarp_labels", (B, h, w, Hs, Ws), run_labels), ("fs_trimap_bands", (B, Hs, Ws), run_bands)]
    for lab in (False, True):
        cases.append(("fs_unwarp_accuracy", (B, h, w, Hs, Ws), run_accuracy(lab)))
        cases.append(("fs_unwarp_trimap", (B, h, w, Hs, Ws), run_trimap(lab)))
        for trim in (False, True):
            cases.append(("fs_unwarp_class_areas", dims, run_areas(trim, lab)))
    for name, qargs, run in cases:
        ints = hip.query(name + "_scratch_ints", *qargs)
        assert ints > 0
        results = []
        for _ in range(2):
            t, scr = _guarded(ints)
            results.append(run(scr))
            assert bool((t[ints:] == SENTINEL).all()), f"{name}: wrote past the {ints} ints it asked for"
        assert results[0].keys() == results[1].keys()
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), (name, k)
    # the library agrees with itself across entry points: the class map and the counters are the same whoever makes them
    ref = ops.unwarp_class_areas(cls, m, grid, y, cl, dia_factor=D, return_labels=True)
    assert torch.equal(ref[4], ops.unwarp_labels(cls, m, grid, Hs, Ws)[0]) and torch.equal(ref[0], ops.unwarp_accuracy(cls, m, grid, y, cl)[0])
    assert torch.equal(ref[3], ops.unwarp_trimap(cls, m, grid, y, cl, D)[2]) and torch.equal(ref[2], ops.unwarp_class_areas(cls, m, grid, y, cl)[2])
