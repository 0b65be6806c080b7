"""The Hausdorff percentile (HD95; VAL.hd95) at full resolution: fs_surface_hd / ops.surface_hd, ops.hd_from_stats,
DeformSegmentationModule.evaluate(hausdorff=q), train.HausdorffMeter and train.evaluate_step_hd.

What is computed is the published 2-D definition (border = foreground with a background 4-neighbour, nearest border pixel of the other
mask in both directions, pooled, np.percentile), not what the reference's utils.hd95 returns: that function flattens both masks before
it erodes them (tests/golden/g20_hd95.npz records both).  tests/surface_ref.py restates the definition in integers; the golden holds
what scipy + numpy give.  CPU: the restatement against the golden (integers exactly, percentiles within 1e-12 relative: the square
root and the interpolation are the only floating-point steps, and a brute-force integer restatement differed from scipy + numpy by at
most 1.9e-14 over 200 random pairs), hd_from_stats, the meter alone and over two gloo ranks, the C ABI's declarations.  GPU: every
check an equality of integers.

train.evaluate_step keeps its five parameters (tests/test_class_areas.py pins the list); the meter goes through
train.evaluate_step_hd, which evaluate_step now calls."""
import inspect
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T

import surface_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("row_1x9", "col_9x1", "dot_3x3", "two_dots", "rect_16x20", "blocky_37x61", "blocky_130x97", "touching_40x33", "thin_2x300",
         "disc_64x64", "full_12x15", "empty_pred", "empty_label", "both_empty")
EMPTY = ("empty_pred", "empty_label", "both_empty")
RTOL = 1e-12
_G20 = {}


def _g20():
    if not _G20:
        g = np.load(os.path.join(GOLD, "g20_hd95.npz"), allow_pickle=False)
        _G20["qs"] = [int(q) for q in g["qs"]]
        _G20["cases"] = {str(n): {k: g[f"{n}/{k}"] for k in ("a", "b", "d2_pred_to_label", "d2_label_to_pred", "n_pred", "n_label",
                                                             "percentile", "utils_hd95")} for n in g["names"]}
    return _G20["qs"], _G20["cases"]


def _golden_stats(c, q):
    """(n_pred, n_label, d2_lo, d2_hi) from the golden's sorted multisets."""
    na, nb = int(c["n_pred"]), int(c["n_label"])
    if na == 0 or nb == 0:
        return np.array([na, nb, -1, -1], np.int64)
    pooled = np.sort(np.concatenate([c["d2_pred_to_label"], c["d2_label_to_pred"]]))
    lo, hi, _ = R.ranks(na + nb, q)
    return np.array([na, nb, pooled[lo], pooled[hi]], np.int64)


# ------------------------------------------------------------------------------------------------------------------ CPU ----------
def test_golden_has_the_cases():
    qs, cases = _g20()
    assert qs == [1, 50, 95, 100] and tuple(cases) == NAMES
    mult = {(95 * (int(c["n_pred"]) + int(c["n_label"]) - 1)) % 100 == 0 for n, c in cases.items() if n not in EMPTY}
    assert mult == {True, False}                                                       # both an exact rank and an interpolated one
    t = cases["touching_40x33"]
    assert abs(float(t["utils_hd95"]) - float(t["percentile"][2])) > 100               # the recorded divergence of utils.hd95


def test_restatement_reproduces_the_golden_integers_exactly():
    _, cases = _g20()
    for name, c in cases.items():
        ba, bb = R.border(c["a"]), R.border(c["b"])
        assert int(ba.sum()) == int(c["n_pred"]) and int(bb.sum()) == int(c["n_label"]), name
        assert np.array_equal(np.sort(R.nearest_d2(ba, bb)), c["d2_pred_to_label"]), name
        assert np.array_equal(np.sort(R.nearest_d2(bb, ba)), c["d2_label_to_pred"]), name
    assert np.array_equal(np.sort(R.nearest_d2(R.border(cases["two_dots"]["a"]), R.border(cases["two_dots"]["b"]))), [19 * 19 + 30 * 30])


def test_restatement_reproduces_the_golden_percentiles():
    qs, cases = _g20()
    for name, c in cases.items():
        for i, q in enumerate(qs):
            st = R.stats(c["a"], c["b"], q)
            assert np.array_equal(st, _golden_stats(c, q)), (name, q)
            got, want = R.percentile(st, q), float(c["percentile"][i])
            if name in EMPTY:
                assert math.isnan(got) and math.isnan(want) and st[2] == -1 and st[3] == -1
            else:
                assert abs(got - want) <= RTOL * abs(want), (name, q, got, want)


def test_hd_from_stats_reproduces_the_golden():
    qs, cases = _g20()
    for i, q in enumerate(qs):
        hd = torch.from_numpy(np.stack([_golden_stats(c, q) for c in cases.values()]))
        got = ops.hd_from_stats(hd, q)
        assert got.dtype == torch.float64 and got.shape == (len(cases),)
        for j, (name, c) in enumerate(cases.items()):
            want = float(c["percentile"][i])
            if name in EMPTY:
                assert math.isnan(float(got[j])), name
            else:
                assert abs(float(got[j]) - want) <= RTOL * abs(want), (name, q, float(got[j]), want)
    with pytest.raises(ValueError):
        ops.hd_from_stats(torch.zeros(2, 3, dtype=torch.int64))
    for bad in (0, 101, 2.5, True):
        with pytest.raises(ValueError):
            ops.hd_from_stats(torch.zeros(2, 4, dtype=torch.int64), bad)


def test_hausdorff_meter_on_hand_made_input():
    meter = T.HausdorffMeter("cpu")
    assert meter.q == 95 and math.isnan(meter.result(reduce=False)["hd"])
    # n = 21: 95 * 20 = 1900, rank 19 exactly; n = 2: ranks 0 and 1, frac 0.95
    a = torch.tensor([[11, 10, 49, 999], [1, 1, 9, 25], [0, 8, -1, -1]])
    b = torch.tensor([[5, 0, -1, -1], [0, 0, -1, -1]])
    meter.update(a)
    meter.update(b)
    r = meter.result(reduce=False)
    assert r["images"] == 2 and r["skipped_empty_pred"] == 2 and r["skipped_empty_label"] == 2 and r["q"] == 95
    assert abs(r["hd"] - (7.0 + (3.0 + 2.0 * 0.95)) / 2) <= 1e-14
    m50 = T.HausdorffMeter("cpu", q=50)
    m50.update(a[1:2])
    assert m50.result(reduce=False)["hd"] == 4.0
    with pytest.raises(ValueError):
        meter.update(torch.zeros(2, 3, dtype=torch.int64))
    for bad in (0, 101):
        with pytest.raises(ValueError):
            T.HausdorffMeter("cpu", q=bad)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _meter_batches():
    g = torch.Generator().manual_seed(20)
    out = []
    for B in (2, 3, 1, 4, 2):
        n = torch.randint(1, 5000, (B, 2), generator=g)
        lo = torch.randint(0, 1 << 28, (B, 1), generator=g)
        out.append(torch.cat([n, lo, lo + torch.randint(0, 1000, (B, 1), generator=g)], 1))
    out[1][1] = torch.tensor([0, 7, -1, -1])
    out[3][2] = torch.tensor([9, 0, -1, -1])
    return out


def _meter_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    meter = T.HausdorffMeter("cpu")
    batches = _meter_batches()
    for b in (batches[:3] if rank == 0 else batches[3:]):                               # three batches on rank 0, two on rank 1
        meter.update(b)
    out[rank] = (meter.result(), meter.result(reduce=False))
    dist.barrier()
    dist.destroy_process_group()


def test_hausdorff_meter_two_gloo_ranks():
    batches = _meter_batches()
    single = T.HausdorffMeter("cpu")
    for b in batches:
        single.update(b)
    want = single.result()
    every = torch.cat(batches)
    d = ops.hd_from_stats(every, 95)
    assert want["images"] == 10 and want["skipped_empty_pred"] == 1 and want["skipped_empty_label"] == 1
    assert abs(want["hd"] - float(d[~torch.isnan(d)].mean())) <= 1e-12 * want["hd"]
    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_meter_worker, args=(world, port, out), nprocs=world, join=True)
    for rank in range(world):
        got, own = out[rank]
        assert got["images"] == 10 and got["skipped_empty_pred"] == 1 and got["skipped_empty_label"] == 1
        assert abs(got["hd"] - want["hd"]) <= 1e-12 * want["hd"]
        assert own["images"] == 5 and own["hd"] != want["hd"]          # six images a rank, one of them empty


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(GOLD), os.pardir, "include", "fovealseg.h")).read()
    for name in ("fs_surface_hd", "fs_surface_hd_scratch_ints", "fs_unwarp_hd", "fs_unwarp_hd_scratch_ints"):
        assert name + "(" in header
    assert "utils.py:25-101" in header and "VAL.hd95" in header
    assert hip.SIGNATURES["fs_surface_hd"] == "ppp" + "iiii"
    assert hip.SIGNATURES["fs_unwarp_hd"] == hip.SIGNATURES["fs_unwarp_class_areas"][:11] + "p" + "i" * 9
    assert "fs_surface_hd_scratch_ints" in hip.HOST_ONLY and "fs_unwarp_hd_scratch_ints" in hip.HOST_ONLY


def test_scratch_queries():
    lib = hip.load()
    assert lib.fs_unwarp_hd_scratch_ints(0, 51, 4, 4, 64, 64) == 0 and lib.fs_surface_hd_scratch_ints(0, 64, 64) == 0
    assert lib.fs_surface_hd_scratch_ints(2, 0, 64) == 0
    for dims in ((2, 51, 4, 4, 64, 64), (3, 6, 9, 11, 37, 300), (1, 2, 80, 80, 1024, 1024)):
        B, _, _, _, Hs, Ws = dims
        areas, hd, surf = lib.fs_unwarp_class_areas_scratch_ints(*dims), lib.fs_unwarp_hd_scratch_ints(*dims), lib.fs_surface_hd_scratch_ints(B, Hs, Ws)
        assert hd >= areas
        assert hd - areas >= surf + B * Hs * Ws // 4 and surf >= B * Hs * Ws                # the byte map, then fs_surface_hd's own
    # no (B, Hs, Ws) list of distances: at most one int per pixel (two 16-bit column distances) plus histograms that do not grow with B * Hs * Ws
    assert lib.fs_surface_hd_scratch_ints(4, 1024, 1024) - 4 * 1024 * 1024 <= 4 * (6 + 64 + 2 * 32768)


def test_signatures():
    sig = inspect.signature(fovealseg.DeformSegmentationModule.evaluate)
    assert sig.parameters["hausdorff"].default is None
    sig = inspect.signature(T.evaluate_step_hd)
    assert list(sig.parameters) == ["module", "batch", "meter", "trimap_meter", "class_meter", "hd_meter"] and sig.parameters["hd_meter"].default is None
    assert inspect.signature(ops.surface_hd).parameters["q"].default == 95 and inspect.signature(ops.hd_from_stats).parameters["q"].default == 95
    assert inspect.signature(ops.unwarp_count).parameters["hd_q"].default is None
    assert inspect.signature(T.HausdorffMeter.__init__).parameters["q"].default == 95


class _Recorder:
    """Stands in for the module: records how evaluate is called."""

    def __init__(self):
        self.calls = []

    def evaluate(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return (tuple(range(5)) + (("trim",) if "trimap" in kwargs else ()) + ((torch.zeros(2, 3, 4, 3, dtype=torch.int64),) if kwargs.get("class_areas") else ())
                + ((torch.tensor([[1, 1, 9, 25], [0, 3, -1, -1]]),) if kwargs.get("hausdorff") else ()))

    def check_nan(self):
        pass


def test_evaluate_step_without_hd_meter_calls_evaluate_as_before():
    X, Fp, Y, cl = torch.zeros(2, 4, 8, 8), torch.zeros(2, 2), torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, dtype=torch.int64)
    rec = _Recorder()
    for step in (T.evaluate_step, T.evaluate_step_hd):
        rec.calls.clear()
        out = step(rec, (X, Fp, Y, cl))
        (args, kwargs), = rec.calls
        assert kwargs == {} and len(args) == 4 and args[0].shape == (2, 3, 8, 8) and args[1] is Fp and args[2] is Y and args[3] is cl
        assert out == tuple(range(5))
        cm = T.ClassIoUMeter("cpu", 4)
        out = step(rec, (X, Fp, Y, cl), None, None, cm)
        assert rec.calls[1][1] == {"class_areas": True} and len(out) == 6 and cm.result(reduce=False)["images"] == 2
    hm, cm = T.HausdorffMeter("cpu", q=50), T.ClassIoUMeter("cpu", 4)
    out = T.evaluate_step_hd(rec, (X, Fp, Y, cl), class_meter=cm, hd_meter=hm)
    assert rec.calls[-1][1] == {"class_areas": True, "hausdorff": 50} and len(out) == 7
    r = hm.result(reduce=False)
    assert r["images"] == 1 and r["skipped_empty_pred"] == 1 and r["hd"] == 4.0 and cm.result(reduce=False)["images"] == 2
    out = T.evaluate_step_hd(rec, (X, Fp, Y, cl), hd_meter=hm)
    assert rec.calls[-1][1] == {"hausdorff": 50} and len(out) == 6 and hm.result(reduce=False)["images"] == 2


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ----
def _surface(a, b, q=95, offset=0, garbage=-9999):
    """fs_surface_hd under tests/kernel_testing.py's rules: the byte map and hd between guards, hd pre-filled with a marker, the
    scratch between guards and pre-filled with garbage.  a, b (B,H,W) numpy; returns hd (B,4) as numpy."""
    import kernel_testing as KT
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    B, Hs, Ws = a.shape
    fg = torch.from_numpy(a.astype(np.uint8) | (b.astype(np.uint8) << 1))
    body = torch.cat([torch.full((offset,), 0xFF, dtype=torch.uint8), fg.reshape(-1)])
    fgb = KT.Out(body.numel(), torch.uint8, body=body)
    hd = KT.Out(B * 4, torch.int64)
    scratch = KT.Out(hip.query("fs_surface_hd_scratch_ints", B, Hs, Ws), torch.int32, fill=garbage)
    hip.call("fs_surface_hd", fgb.ptr + offset, hd.ptr, scratch.ptr, B, Hs, Ws, q)
    out = hd.get().reshape(B, 4).numpy()
    assert torch.equal(fgb.get(complete=False), body)                                  # the input is only read
    scratch.rows_left(1)                                                                # its guards
    return out


def _expect(a, b, q=95, **kw):
    got, want = _surface(a, b, q, **kw), R.stats_batch(a, b, q)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_surface_hd_golden(name):
    qs, cases = _g20()
    c = cases[name]
    for q in qs:
        got = _surface(c["a"][None], c["b"][None], q)
        assert np.array_equal(got[0], _golden_stats(c, q)), (name, q, got.tolist())


def _sparse(rng, H, W, p):
    return rng.random((1, H, W)) < p


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(3, 255), (3, 256), (3, 257), (3, 1025), (1, 3), (2, 3), (257, 3), (1025, 3)])
def test_surface_hd_seams(H, W):
    """Widths across the lane and workgroup seams of the row pass, heights across the column pass's sweeps."""
    rng = np.random.default_rng(H * 10000 + W)
    a, b = _sparse(rng, H, W, 0.3), _sparse(rng, H, W, 0.02)
    a[0, H - 1, W - 1], b[0, 0, 0] = True, True                                         # a distance across the whole image
    _expect(a, b, 95)
    _expect(b, a, 100)
    dense = rng.random((1, H, W)) < 0.9
    _expect(dense, a, 50)


@pytest.mark.gpu
def test_surface_hd_widest_row_and_refusals():
    import kernel_testing as KT
    W = 16384
    a, b = np.zeros((1, 2, W), bool), np.zeros((1, 2, W), bool)
    a[0, 0, [0, 5000, W - 1]], b[0, 1, [3, 16000]] = True, True
    got = _expect(a, b, 100)
    assert got[0, 3] == 1 + (5000 - 3) ** 2                                           # column 5000's nearest is column 3, a row away
    hd = KT.Out(4, torch.int64)
    fg = torch.zeros(2 * (W + 1), dtype=torch.uint8, device="cuda")
    scratch = KT.Out(hip.query("fs_surface_hd_scratch_ints", 1, 2, W + 1) + 4, torch.int32)
    for args in ((fg.data_ptr(), hd.ptr, scratch.ptr, 1, 2, W + 1, 95), (fg.data_ptr(), hd.ptr, scratch.ptr, 1, W + 1, 2, 95),
                 (fg.data_ptr(), hd.ptr, scratch.ptr, 1, 2, W, 0), (fg.data_ptr(), hd.ptr, scratch.ptr, 1, 2, W, 101),
                 (None, hd.ptr, scratch.ptr, 1, 2, W, 95), (fg.data_ptr(), None, scratch.ptr, 1, 2, W, 95),
                 (fg.data_ptr(), hd.ptr, None, 1, 2, W, 95), (fg.data_ptr(), hd.ptr, scratch.ptr + 4, 1, 2, W, 95),
                 (fg.data_ptr(), hd.ptr, scratch.ptr, 0, 2, W, 95)):
        with pytest.raises(hip.HipLibraryError):
            hip.call("fs_surface_hd", *args)
    assert hd.untouched() and scratch.untouched()                                       # a refused call launches nothing
    with pytest.raises(ValueError):
        ops.surface_hd(fg.reshape(1, 2, W + 1), fg.reshape(1, 2, W + 1), q=0)
    with pytest.raises(ValueError):
        ops.surface_hd(fg.reshape(1, 2, W + 1), fg.reshape(1, W + 1, 2))
    with pytest.raises(ValueError):
        ops.surface_hd(fg.reshape(1, 2, W + 1).float(), fg.reshape(1, 2, W + 1).float())


@pytest.mark.gpu
def test_surface_hd_pruning_adversary():
    """The label's border is the single pixel (0,0); the nearest-in-row scan of the prediction's far pixel must not stop early."""
    a, b = np.zeros((1, 97, 130), bool), np.zeros((1, 97, 130), bool)
    b[0, 0, 0] = True
    a[0, 96, 129] = a[0, 50, 3] = a[0, 0, 1] = a[0, 96, 0] = True
    got = _expect(a, b, 100)
    assert got[0, 3] == 96 * 96 + 129 * 129
    _expect(a, b, 50)


@pytest.mark.gpu
def test_surface_hd_batch_does_not_leak():
    rng = np.random.default_rng(3)
    a, b = rng.random((3, 40, 52)) < 0.2, rng.random((3, 40, 52)) < 0.05
    a[1] = False                                                                        # an empty image in the middle
    b[2, 20:] = False
    got = _expect(a, b, 95)
    assert got[1].tolist() == [0, int(R.border(b[1]).sum()), -1, -1] and len({int(v) for v in got[:, 0] + got[:, 1]}) == 3
    for i in range(3):                                                                  # every image alone gives its row
        assert np.array_equal(_surface(a[i:i + 1], b[i:i + 1], 95)[0], got[i])


@pytest.mark.gpu
def test_surface_hd_percentiles_offset_and_repeat():
    rng = np.random.default_rng(4)
    a = rng.random((2, 61, 45)) < 0.5
    b = a ^ (rng.random((2, 61, 45)) < 0.03)
    b[:, 40:] = False                                                                   # far pixels: the upper ranks are large
    rows = [_expect(a, b, q) for q in (1, 50, 95, 100)]
    assert all((r[:, 2] <= r[:, 3]).all() for r in rows) and (rows[0][:, 2] <= rows[3][:, 3]).all()
    assert np.array_equal(_surface(a, b, 95, offset=1), rows[2])                        # a byte map that is not even 2-byte aligned
    assert np.array_equal(_surface(a, b, 95, garbage=0x7F7F7F7F), rows[2])              # the same bits twice, whatever the scratch held
    op = ops.surface_hd(torch.from_numpy(a).cuda(), torch.from_numpy(b.astype(np.uint8) * 7).cuda(), q=95)
    assert op.dtype == torch.int64 and np.array_equal(op.cpu().numpy(), rows[2])
    assert np.array_equal(ops.surface_hd(torch.from_numpy(a[0]).cuda(), torch.from_numpy(b[0]).cuda()).cpu().numpy(), rows[2][:1])
    want = [R.percentile(r, 95) for r in rows[2]]
    assert np.abs(ops.hd_from_stats(op, 95).cpu().numpy() - want).max() <= RTOL * max(want)


@pytest.mark.gpu
def test_surface_hd_every_pixel_a_border_pixel():
    """A checkerboard against its complement: every pixel is a border pixel of one of the two masks, n = Hs * Ws, every d^2 = 1.  (No
    mask has more border pixels than a checkerboard's half, so n = Hs * Ws is the most two masks of this kind give.)  Then a
    checkerboard against a noisy mask: most pixels are border pixels and the distances differ."""
    ii, jj = np.mgrid[:64, :64]
    a = ((ii + jj) % 2 == 0)[None]
    got = _expect(a, ~a, 95)
    assert got[0].tolist() == [2048, 2048, 1, 1]
    assert _expect(a, a, 100)[0].tolist() == [2048, 2048, 0, 0]
    rng = np.random.default_rng(6)
    b = rng.random((1, 64, 64)) < 0.5
    b[0, :, 40:] = False
    got = _expect(a, b, 95)
    assert got[0, 0] + got[0, 1] > 64 * 64 // 2 + 500


# ------------------------------------------------------------------------------------------------------------------ GPU: op -------
def _inputs(B, K, h, w, seed, lo=-1.1, hi=1.1):
    g = torch.Generator().manual_seed(seed)
    grid = (torch.rand(B, h, w, 2, generator=g) * (hi - lo) + lo).clamp(-1, 1)
    cls = torch.randn(B, K, generator=g)
    cls[:, K - 1] = 3 * cls.abs().amax(1)            # the mask plane decides where m is large, a constant class elsewhere
    m = torch.rand(B, h, w, generator=g) - 0.5
    return cls.cuda(), m.cuda(), grid.cuda()


def _labels_for(B, K, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed + 77)
    coarse = (torch.rand(B, 1, (Hs + 7) // 8, (Ws + 7) // 8, generator=g) < 0.4).float()
    y = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :Hs, :Ws].contiguous()
    cl = torch.randint(0, K - 1, (B, 1), generator=g)
    return y.cuda(), cl.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 6), (8, 1500, 2)])
def test_unwarp_count_with_hd_ragged_widths(Hs, Ws, K):
    cls, m, grid = _inputs(2, K, 9, 11, Hs * 1000 + Ws)
    y, cl = _labels_for(2, K, Hs, Ws, Hs)
    base = ops.unwarp_count(cls, m, grid, y, cl, return_labels=True)
    assert len(base) == 6 and base[5] is None
    for kw in ({}, {"areas": True}, {"dia_factor": 5}, {"areas": True, "dia_factor": 5}):
        ref = ops.unwarp_count(cls, m, grid, y, cl, return_labels=True, **kw)
        got = ops.unwarp_count(cls, m, grid, y, cl, return_labels=True, hd_q=95, **kw)
        for i in range(5):                                                              # everything else: the bits of the call without it
            assert (got[i] is None and ref[i] is None) or torch.equal(got[i], ref[i]), (kw, i)
        labels = got[4].cpu().numpy()
        want = R.stats_batch(labels != K - 1, y[:, 0].long().cpu().numpy() != 0, 95)
        assert got[5].dtype == torch.int64 and np.array_equal(got[5].cpu().numpy(), want), (kw, got[5].tolist(), want.tolist())
    plain = ops.unwarp_count(cls, m, grid, y, cl, hd_q=50)                              # no class map
    want = R.stats_batch(base[4].cpu().numpy() != K - 1, y[:, 0].long().cpu().numpy() != 0, 50)
    assert plain[4] is None and np.array_equal(plain[5].cpu().numpy(), want)
    with pytest.raises(ValueError):
        ops.unwarp_count(cls, m, grid, y, cl, hd_q=0)


# ------------------------------------------------------------------------------------------------------------------ GPU: module ---
_MODULES = {}


def _module(kind):
    if kind not in _MODULES:
        _MODULES.clear()                             # one module at a time on the device
        torch.cuda.empty_cache()
        cfg = fovealseg.lvis50_cfg()
        if kind == "segformer":
            cfg.MODEL.arch_encoder, cfg.MODEL.fc_dim = "segformer", 1024
            cfg.TRAIN.task_input_size = (160, 160)
        _MODULES[kind] = T.build_module(cfg, device="cuda")
    module, _ = _MODULES[kind]
    module.eval()
    return module


@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,seg", [("hrnet", 256, None), ("segformer", 256, (200, 180))])
def test_evaluate_with_hausdorff(kind, size, seg, deterministic):
    module = _module(kind)
    K = module.cfg.DATASET.num_class
    X, Fp, Y, cl = T.synthetic_batch(2, size, size, seed=11, device="cuda")
    if seg is not None:
        _, _, Y, _ = T.synthetic_batch(2, seg[0], seg[1], seed=11, device="cuda")
    base = module.evaluate(X, Fp, Y, cl, seg, return_labels=True)
    assert len(base) == 6                                                               # without the keyword: the parent's tuple
    out = module.evaluate(X, Fp, Y, cl, seg, hausdorff=95, return_labels=True)
    module.check_nan()
    assert len(out) == 7 and all(torch.equal(a, b) for a, b in zip(out[:6], base))
    want = R.stats_batch(out[5].cpu().numpy() != K - 1, Y[:, 0].long().cpu().numpy() != 0, 95)
    assert out[6].dtype == torch.int64 and out[6].shape == (2, 4) and np.array_equal(out[6].cpu().numpy(), want)
    every = module.evaluate(X, Fp, Y, cl, seg, return_labels=True, class_areas=True, trimap=5, hausdorff=95)
    ref = module.evaluate(X, Fp, Y, cl, seg, return_labels=True, class_areas=True, trimap=5)
    assert len(every) == 9 and len(ref) == 8 and all(torch.equal(a, b) for a, b in zip(every[:8], ref))      # (.., labels, trim, areas, hd)
    assert torch.equal(every[8], out[6]) and every[7].shape == (2, 3, K, 3) and every[6].shape == (2, 6, 3)
    with pytest.raises(ValueError):
        module.evaluate(X, Fp, Y, cl, seg, hausdorff=101)


@pytest.mark.gpu
def test_evaluate_step_feeds_the_hausdorff_meter():
    module = _module("hrnet")
    meter, hmeter = T.FullResMeter("cuda"), T.HausdorffMeter("cuda")
    rows = []
    for seed, B in ((1, 2), (2, 3)):
        batch = T.synthetic_batch(B, 128, 128, seed=seed, device="cuda")
        out = T.evaluate_step_hd(module, batch, meter, hd_meter=hmeter)
        assert len(out) == 6 and torch.equal(out[4], T.evaluate_step(module, batch)[4])
        rows.append(out[5].cpu())
    # a prediction without foreground: the class plane of K-1 far above the others
    X, Fp, Y, cl = T.synthetic_batch(2, 128, 128, seed=3, device="cuda")
    K = module.cfg.DATASET.num_class
    with torch.no_grad():
        cls, m, grid, _ = module._head_parts(X, Fp, (128, 128), "evaluate")
    cls = cls.clone()
    cls[:, :K - 1] = -1e30
    hd = ops.unwarp_count(cls, m, grid, Y, cl, return_labels=True, hd_q=95)
    assert bool((hd[4] == K - 1).all()) and hd[5][:, 0].tolist() == [0, 0] and hd[5][:, 2:].tolist() == [[-1, -1], [-1, -1]]
    assert bool((hd[5][:, 1] > 0).all())
    hmeter.update(hd[5])
    rows.append(hd[5].cpu())
    res = hmeter.result()
    every = torch.cat(rows)
    d = ops.hd_from_stats(every, 95)
    ok = ~torch.isnan(d)
    assert res["images"] == int(ok.sum()) and res["skipped_empty_pred"] == int((every[:, 0] == 0).sum()) >= 2
    assert res["images"] + int((~ok).sum()) == 7 and meter.result()["images"] == 5
    if res["images"]:
        assert abs(res["hd"] - float(d[ok].mean())) <= 1e-12 * max(1.0, float(d[ok].mean()))
