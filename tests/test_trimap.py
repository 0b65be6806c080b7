"""Trimap boundary accuracy at full resolution (eval.py:41-67): ops.trimap_bands (fs_trimap_bands), ops.unwarp_trimap (fs_unwarp_trimap),
ops.trimap_from_counts, DeformSegmentationModule.evaluate(trimap=...), train.TrimapMeter and train.evaluate_step(trimap_meter=...).

The reference dilates PIL's FIND_EDGES of the label 2**i times with scipy's cross element and scores the prediction inside each band.
tests/trimap_ref.py restates that as a seed rule and an L1 distance; tests/golden/g18_trimap.npz holds what PIL and scipy themselves give.
CPU: the restatement against the fixture bit for bit, the counters' arithmetic, the meter over two gloo ranks.  GPU: the band kernel bit
for bit against the restatement on the shapes that can break a tile, a halo or a doubling step; the fused count against a torch count of
the class map; evaluate(trimap=5) against evaluate() and predict(); the memory the feature adds."""
import inspect
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

import trimap_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g18():
    g = np.load(os.path.join(GOLD, "g18_trimap.npz"), allow_pickle=False)
    D, K = int(g["D"]), int(g["K"])
    out = []
    for n in g["names"]:
        t = g[f"{n}/t"].astype(np.int64)
        bands = np.unpackbits(g[f"{n}/bands"], axis=-1)[..., :t.shape[1]].astype(bool)
        out.append((str(n), t, int(g[f"{n}/cls_label"]), g[f"{n}/pred"].astype(np.int64), bands, g[f"{n}/acc"], bool(g[f"{n}/constant"])))
    return D, K, out


# ------------------------------------------------------------------------------------------------------------------ CPU ----------
def test_restatement_reproduces_the_reference_bit_for_bit():
    D, K, cases = _g18()
    assert D == 5 and len(cases) == 10
    shapes = {c[1].shape for c in cases}
    assert {(1, 9), (2, 50), (3, 3), (16, 20), (37, 61), (130, 97)} <= shapes
    for name, t, cl, pred, bands, acc, constant in cases:
        idx = R.band_index(t, D, frame=True)
        for i in range(D + 1):
            assert np.array_equal(idx <= i, bands[i]), (name, i)
        gt = t * cl + (1 - t) * (K - 1)
        trim = R.counters(pred[None], gt[None], idx[None], D, K)[0]
        got = R.accuracies(trim)[:, 0]
        assert np.abs(got - acc).max() <= 1e-15, (name, got, acc)
        assert bool((trim[:, 0] > 0).all()) != (name.startswith("all_foreground")), name
        if name.startswith("all_background"):                                          # the ring alone: PIL on a constant 255 image
            ring = np.ones(t.shape, bool)
            ring[1:-1, 1:-1] = False
            assert np.array_equal(idx == 0, R.l1_distance(ring) <= 1)
        if name.startswith("all_"):
            assert constant and not R.seeds(t, frame=False).any() and (R.band_index(t, D, frame=False) == 255).all()


def test_restatement_without_the_frame_is_scipys_dilation_of_the_neighbour_rule():
    from scipy import ndimage
    D, _, cases = _g18()
    for name, t, *_ in cases:
        H, W = t.shape
        seed = np.zeros((H, W), bool)
        for v in range(H):
            for u in range(W):
                if t[v, u] == 0:
                    seed[v, u] = t[max(v - 1, 0):v + 2, max(u - 1, 0):u + 2].any()
        assert np.array_equal(R.seeds(t, frame=False), seed), name
        idx = R.band_index(t, D, frame=False)
        for i in range(D + 1):
            want = ndimage.binary_dilation(seed, iterations=2 ** i) if seed.any() else np.zeros((H, W), bool)
            assert np.array_equal(idx <= i, want), (name, i)


def _hand_made():
    """Three images, D = 2: a plain one, one with empty bands (no boundary pixel), one whose sums pass 2^32."""
    a = [[10, 7, 9], [40, 20, 30], [100, 90, 95]]
    b = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    c = [[5_000_000_000, 2_500_000_000, 4_000_000_000], [6_000_000_000, 3_000_000_000, 4_500_000_000], [7_000_000_000, 7_000_000_000, 7_000_000_000]]
    return torch.tensor([a, b, c], dtype=torch.int64)


def test_trimap_from_counts_and_meter_on_hand_made_counters():
    trim = _hand_made()
    acc = ops.trimap_from_counts(trim)
    assert acc.dtype == torch.float64 and acc.shape == (3, 3, 2)
    assert acc[0, 0].tolist() == [7 / (10 + 1e-10), 9 / (10 + 1e-10)] and acc[1].abs().sum() == 0 and acc[2, 2].tolist() == [7e9 / (7e9 + 1e-10)] * 2
    assert np.array_equal(acc.numpy(), R.accuracies(trim.numpy()))
    with pytest.raises(ValueError):
        ops.trimap_from_counts(trim[..., :2])
    meter = T.TrimapMeter("cpu", 2)
    meter.update(trim[:2])
    meter.update(trim[2:])
    r = meter.result(reduce=False)
    assert r["widths"] == [1, 2, 4] and r["images"] == [2, 2, 2]                        # the image with empty bands is left out
    assert r["counts"] == trim.sum(0).tolist()
    for i in range(3):
        assert abs(r["acc"][i] - float(acc[[0, 2], i, 0].mean())) <= 1e-15
        assert abs(r["acc_bin"][i] - float(acc[[0, 2], i, 1].mean())) <= 1e-15
        tot = trim[:, i].sum(0).tolist()
        assert r["pooled"][i] == tot[1] / tot[0] and r["pooled_bin"][i] == tot[2] / tot[0]
    empty = T.TrimapMeter("cpu", 2)
    empty.update(trim[1:2])
    r = empty.result(reduce=False)
    assert r["images"] == [0, 0, 0] and all(np.isnan(v) for v in r["acc"] + r["pooled"])
    assert T.TrimapMeter("cpu").dia_factor == 5 and T.TrimapMeter("cpu").frame is True
    with pytest.raises(ValueError):
        meter.update(_hand_made()[:, :2])
    with pytest.raises(ValueError):
        T.TrimapMeter("cpu", 8)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _meter_batches():
    g = torch.Generator().manual_seed(18)
    batches = [_hand_made()]
    for B in (3, 1, 4, 2):
        total = torch.randint(1, 5_000_000_000, (B, 3, 1), generator=g).cumsum(1)      # bands grow with the width
        part = (torch.rand(B, 3, 2, generator=g) * total).long()
        batches.append(torch.cat([total, part.amin(2, keepdim=True), part.amax(2, keepdim=True)], 2))
    batches[3][1] = 0                                                                   # one more image without a boundary
    return batches


def _meter_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    meter = T.TrimapMeter("cpu", 2)
    batches = _meter_batches()
    for b in (batches[:3] if rank == 0 else batches[3:]):                               # three batches on rank 0, two on rank 1
        meter.update(b)
    out[rank] = (meter.result(), meter.result(reduce=False))
    dist.barrier()
    dist.destroy_process_group()


def test_trimap_meter_two_gloo_ranks():
    batches = _meter_batches()
    single = T.TrimapMeter("cpu", 2)
    for b in batches:
        single.update(b)
    want = single.result()
    total = torch.cat(batches)
    assert want["counts"] == total.sum(0).tolist() and want["images"] == [11, 11, 11]
    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_meter_worker, args=(world, port, out), nprocs=world, join=True)
    for rank in range(world):
        got, own = out[rank]
        assert got["counts"] == want["counts"] and got["images"] == want["images"]     # integer sums: exact
        assert got["pooled"] == want["pooled"] and got["pooled_bin"] == want["pooled_bin"]
        for k in ("acc", "acc_bin"):
            for a, b in zip(got[k], want[k]):
                assert abs(a - b) <= 1e-12 * abs(b), (k, a, b)
        assert own["counts"] != want["counts"] and own["images"] == ([6, 6, 6] if rank == 0 else [5, 5, 5])


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(GOLD), os.pardir, "include", "fovealseg.h")).read()
    for name in ("fs_trimap_bands", "fs_trimap_bands_scratch_ints", "fs_unwarp_trimap", "fs_unwarp_trimap_scratch_ints"):
        assert name + "(" in header
    assert header.count("eval.py:41-67") >= 2
    assert hip.SIGNATURES["fs_trimap_bands"] == "ppp" + "iiiii" and hip.SIGNATURES["fs_unwarp_trimap"] == "p" * 10 + "i" * 8
    assert "fs_trimap_bands_scratch_ints" in hip.HOST_ONLY and "fs_unwarp_trimap_scratch_ints" in hip.HOST_ONLY
    lib = hip.load()
    assert lib.fs_trimap_bands_scratch_ints(3, 5, 7) == 3 * 5 * 8 // 4 and lib.fs_trimap_bands_scratch_ints(0, 5, 7) == 0
    extra = lib.fs_unwarp_trimap_scratch_ints(2, 4, 4, 64, 64) - lib.fs_unwarp_accuracy_scratch_ints(2, 4, 4, 64, 64)
    assert 2 * 2 * 64 * 64 // 4 <= extra <= 2 * 2 * 64 * 64 // 4 + 2 * 4 * 24 + 16       # band bytes + row-pass bytes + bucket records


def test_evaluate_signature_and_configuration():
    sig = inspect.signature(fovealseg.DeformSegmentationModule.evaluate)
    assert sig.parameters["trimap"].default is None and sig.parameters["trimap_frame"].default is True
    assert list(sig.parameters)[-2:] == ["trimap", "trimap_frame"]
    sig = inspect.signature(T.evaluate_step)
    assert sig.parameters["meter"].default is None and sig.parameters["trimap_meter"].default is None
    V = fovealseg.lvis50_cfg().VAL
    assert V.trimap is False and V.trimap_dia_factor == 5 and V.trimap_visual_check is False


# ------------------------------------------------------------------------------------------------------------------ GPU: bands ----
GUARD = 64


def _bands_guarded(y, D, frame):
    """fs_trimap_bands at the C ABI into a 0xAB-filled buffer between guard bytes."""
    B, Hs, Ws = y.shape
    n = B * Hs * Ws
    raw = torch.full((GUARD + n + GUARD,), 0xAB, device="cuda", dtype=torch.uint8)
    scratch = torch.empty(hip.query("fs_trimap_bands_scratch_ints", B, Hs, Ws), device="cuda", dtype=torch.int32)
    hip.call("fs_trimap_bands", y.data_ptr(), raw.data_ptr() + GUARD, scratch.data_ptr(), B, Hs, Ws, D, int(frame))
    raw = raw.cpu().numpy()
    assert (raw[:GUARD] == 0xAB).all() and (raw[GUARD + n:] == 0xAB).all(), "guard bytes overwritten"
    return raw[GUARD:GUARD + n].reshape(B, Hs, Ws)


def _index_from_distance(d, D):
    out = np.full(d.shape, 255, np.uint8)
    for i in range(D, -1, -1):
        out[d <= 2 ** i] = i
    return out


def _contents(Hs, Ws, seed):
    """Label masks (Hs,Ws) float32 that stress the passes: lone pixels whose diamond crosses every tile edge, constants, blocky masks,
    fractional values around the truncation."""
    rng = np.random.default_rng(seed)
    out = []
    for v, u in ((0, 0), (0, Ws // 2), (Hs - 1, Ws - 1), (Hs // 2, Ws // 2), (Hs // 2, min(Ws - 1, 511)), (min(Hs - 1, 127), Ws // 3)):
        y = np.zeros((Hs, Ws), np.float32)
        y[v, u] = 1.0
        out.append(y)
    out += [np.zeros((Hs, Ws), np.float32), np.ones((Hs, Ws), np.float32)]
    for p in (0.4, 0.1):
        c = rng.random(((Hs + 7) // 8, (Ws + 7) // 8)) < p
        out.append(np.repeat(np.repeat(c, 8, 0), 8, 1)[:Hs, :Ws].astype(np.float32))
    out.append(np.where(out[-2] > 0, 1.7, 0.9).astype(np.float32))                      # truncation: 0.9 is background, 1.7 foreground
    while len(out) % 3:
        out.append(out[len(out) - 9])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", [(1, 1), (1, 65), (2, 3), (2, 1500), (8, 63), (8, 513), (37, 64), (37, 300), (130, 1), (130, 65), (130, 513),
                                   (8, 1500), (37, 3), (1, 300), (130, 300)])
def test_trimap_bands_equal_the_restatement(Hs, Ws):
    contents = _contents(Hs, Ws, Hs * 10000 + Ws)
    dist_of = {fr: [R.l1_distance(R.seeds(np.trunc(y).astype(np.int64), fr)) for y in contents] for fr in (True, False)}
    seen = set()
    for k in range(0, len(contents), 3):                                                # B = 3, another content in every image
        y = torch.from_numpy(np.stack(contents[k:k + 3])).cuda()
        for D in (0, 5, 7):
            for fr in (True, False):
                got = _bands_guarded(y, D, fr)
                want = np.stack([_index_from_distance(d, D) for d in dist_of[fr][k:k + 3]])
                bad = np.argwhere(got != want)
                assert len(bad) == 0, (Hs, Ws, k, D, fr, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
                seen |= set(np.unique(got).tolist())
    assert seen <= set(range(8)) | {255}
    # the op's spelling: (B,1,Hs,Ws), defaults D = 5 / frame = True
    y4 = torch.from_numpy(np.stack(contents[:3]))[:, None].cuda()
    assert np.array_equal(ops.trimap_bands(y4).cpu().numpy(), np.stack([_index_from_distance(d, 5) for d in dist_of[True][:3]]))


@pytest.mark.gpu
def test_trimap_bands_probes_around_a_single_seed():
    """One foreground pixel, frame=False: its eight neighbours are the only seeds, so along its row the pixel 2**i past the neighbour is
    the last of band i and the next one the first of band i + 1 (or of none) -- across the row pass's 512-column segments and the column
    pass's 128-row tiles."""
    Hs, Ws, D = 300, 700, 7
    r, c = 140, 505
    y = torch.zeros(1, Hs, Ws, device="cuda")
    y[0, r, c] = 1.0
    got = _bands_guarded(y, D, False)[0]
    assert got[r, c] == 0                                                               # the pixel itself: foreground, one step from a seed
    for i in range(D + 1):
        nxt = i + 1 if i < D else 255
        for dv, du in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            at = lambda k: got[r + dv * (1 + k), c + du * (1 + k)]                      # noqa: E731
            assert at(2 ** i) == i and at(2 ** i + 1) == nxt, (i, dv, du)
    assert np.array_equal(got, R.band_index(y[0].cpu().numpy().astype(np.int64), D, False))
    assert (_bands_guarded(y, D, True)[0][0] == 0).all()                                # with the frame the ring seeds itself


@pytest.mark.gpu
def test_trimap_bands_rejects_bad_arguments():
    y = torch.zeros(1, 4, 4, device="cuda")
    band = torch.empty(1, 4, 4, device="cuda", dtype=torch.uint8)
    scr = torch.empty(hip.query("fs_trimap_bands_scratch_ints", 1, 4, 4), device="cuda", dtype=torch.int32)
    ok = (y.data_ptr(), band.data_ptr(), scr.data_ptr(), 1, 4, 4, 5, 1)
    hip.call("fs_trimap_bands", *ok)
    for bad in ((None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:2] + (None,) + ok[3:], ok[:3] + (0, 4, 4, 5, 1), ok[:3] + (1, 0, 4, 5, 1),
                ok[:3] + (1, 4, -1, 5, 1), ok[:6] + (-1, 1), ok[:6] + (8, 1), ok[:6] + (5, 2), ok[:6] + (5, -1)):
        with pytest.raises(hip.HipLibraryError):
            hip.call("fs_trimap_bands", *bad)
    with pytest.raises(ValueError):
        ops.trimap_bands(y, dia_factor=8)
    with pytest.raises(ValueError):
        ops.trimap_bands(y[0, 0])


# ------------------------------------------------------------------------------------------------------------------ GPU: count ----
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


def _trim_ref(labels, y, cl, K, D, frame):
    """(B, D+1, 3) int64 on the device: a torch count of a class map against the restated bands."""
    B = labels.shape[0]
    y = y.reshape(B, labels.shape[1], labels.shape[2])
    bands = torch.from_numpy(R.band_index_batch(y.cpu().numpy(), D, frame)).to(labels.device)
    t = y.long()
    gt = t * cl.view(-1, 1, 1).long() + (1 - t) * (K - 1)
    eq, side = labels == gt, (labels == K - 1) == (gt == K - 1)
    rows = []
    for i in range(D + 1):
        inb = bands <= i
        rows.append(torch.stack([inb.flatten(1).sum(1), (inb & eq).flatten(1).sum(1), (inb & side).flatten(1).sum(1)], 1))
    return torch.stack(rows, 1)


def _check(cls, m, grid, y, cl, D=5, frame=True):
    B, K = cls.shape
    _, h, w, _ = grid.shape
    Hs, Ws = int(y.shape[-2]), int(y.shape[-1])
    counts, acc, trim, labels = ops.unwarp_trimap(cls, m, grid, y, cl, D, frame, return_labels=True)
    base = ops.unwarp_accuracy(cls, m, grid, y, cl, return_labels=True)
    assert torch.equal(counts, base[0]) and torch.equal(acc, base[1]) and torch.equal(labels, base[2])
    assert trim.dtype == torch.int64 and trim.shape == (B, D + 1, 3)
    want = _trim_ref(ops.unwarp_labels(cls, m, grid, Hs, Ws)[0], y, cl, K, D, frame)
    assert torch.equal(trim, want), (trim.tolist(), want.tolist())
    plain = ops.unwarp_trimap(cls, m, grid, y, cl, D, frame)                            # no class map; the same bits twice
    assert len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(plain, (counts, acc, trim)))
    # at the C ABI: pre-filled outputs between guards
    G = 8
    c_raw = torch.full((G + B * 6 + G,), -7, device="cuda", dtype=torch.int64)
    t_raw = torch.full((G + B * (D + 1) * 3 + G,), -7, device="cuda", dtype=torch.int64)
    a_raw = torch.full((G + 4 + G,), -7.0, device="cuda")
    scr = torch.empty(hip.query("fs_unwarp_trimap_scratch_ints", B, h, w, Hs, Ws), device="cuda", dtype=torch.int32)
    yc, clc = y.float().contiguous(), cl.long().contiguous()
    hip.call("fs_unwarp_trimap", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), yc.data_ptr(), clc.data_ptr(), c_raw.data_ptr() + 8 * G,
             a_raw.data_ptr() + 4 * G, t_raw.data_ptr() + 8 * G, None, scr.data_ptr(), B, K, h, w, Hs, Ws, D, int(frame))
    for raw, val in ((c_raw, counts), (t_raw, trim), (a_raw, acc)):
        assert bool((raw[:G] == -7).all()) and bool((raw[-G:] == -7).all()), "guard overwritten"
        assert torch.equal(raw[G:-G], val.flatten())
    return counts, acc, trim, labels


@pytest.mark.gpu
def test_unwarp_trimap_g14_grid():
    g = {k: v for k, v in np.load(os.path.join(GOLD, "g14_inverse.npz")).items()}
    Hs, Ws = (int(v) for v in g["seg"])
    grid = torch.from_numpy(g["grid"]).cuda()
    B, h, w, _ = grid.shape
    cls, m, _ = _inputs(B, 51, h, w, 14)
    y, cl = _labels_for(B, 51, Hs, Ws, 14)
    _, _, trim, _ = _check(cls, m, grid, y, cl)
    assert int(trim[:, 0, 0].min()) > 0 and bool((trim[:, 1:, 0] >= trim[:, :-1, 0]).all())   # bands nest
    assert bool((trim[..., 1] <= trim[..., 2]).all()) and bool((trim[..., 2] <= trim[..., 0]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 6), (50, 513, 3), (8, 1500, 2)])
def test_unwarp_trimap_ragged_widths(Hs, Ws, K):
    cls, m, grid = _inputs(2, K, 9, 11, Hs * 1000 + Ws)
    y, cl = _labels_for(2, K, Hs, Ws, Hs)
    _check(cls, m, grid, y, cl)
    _check(cls, m, grid, y, cl, D=7, frame=False)
    _check(cls, m, grid, y, cl, D=0)


@pytest.mark.gpu
def test_unwarp_trimap_no_claimed_pixel_and_many_classes():
    cls, m, grid = _inputs(2, 150, 10, 12, 3)
    grid[1] = 1.5                                    # image 1: nothing claimed, every pixel keeps the decision at (0, 0)
    y, cl = _labels_for(2, 150, 31, 40, 3)
    _, _, _, labels = _check(cls, m, grid, y, cl)
    assert len(labels[1].unique()) == 1


@pytest.mark.gpu
def test_unwarp_trimap_full_size():
    cls, m, grid = _inputs(2, 51, 80, 80, 7, -1.0, 1.0)
    y, cl = _labels_for(2, 51, 1024, 1024, 7)
    _, _, trim, _ = _check(cls, m, grid, y, cl)
    assert int(trim[:, 0, 0].min()) > 0 and int(trim[:, 0, 0].max()) < 1024 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("fill,frame", [(0.0, True), (0.0, False), (1.0, True)])
def test_unwarp_trimap_constant_labels(fill, frame):
    """The constant-label rule: without a boundary pixel every counter is 0; all background with the frame has the ring for seeds."""
    cls, m, grid = _inputs(2, 51, 12, 12, 41)
    y = torch.full((2, 1, 64, 48), fill, device="cuda")
    cl = torch.tensor([[3], [17]], device="cuda")
    _, _, trim, _ = _check(cls, m, grid, y, cl, frame=frame)
    if fill == 0.0 and frame:
        assert trim[:, 0, 0].tolist() == [64 * 48 - 60 * 44] * 2                        # the ring and the pixels one step inside it
    else:
        assert int(trim.abs().sum()) == 0
        assert float(ops.trimap_from_counts(trim).abs().sum()) == 0.0


@pytest.mark.gpu
def test_unwarp_trimap_rejects_bad_arguments():
    cls, m, grid = _inputs(1, 4, 4, 4, 0)
    y, cl = _labels_for(1, 4, 8, 8, 0)
    with pytest.raises(ValueError):
        ops.unwarp_trimap(cls, m[:, :3], grid, y, cl)
    with pytest.raises(ValueError):
        ops.unwarp_trimap(cls, m, grid, y.repeat(2, 1, 1, 1), cl)
    with pytest.raises(ValueError):
        ops.unwarp_trimap(cls, m, grid, y, cl.repeat(2, 1))
    with pytest.raises(ValueError):
        ops.unwarp_trimap(cls, m, grid, y, cl, dia_factor=8)
    with pytest.raises(ValueError):
        ops.unwarp_trimap(cls, m, grid, y, cl, dia_factor=-1)
    with pytest.raises(hip.HipLibraryError):         # K < 2
        ops.unwarp_trimap(cls[:, :1], m, grid, y, cl)
    counts = torch.empty(1, 6, device="cuda", dtype=torch.int64)
    acc = torch.empty(4, device="cuda")
    trim = torch.empty(1, 6, 3, device="cuda", dtype=torch.int64)
    scr = torch.empty(hip.query("fs_unwarp_trimap_scratch_ints", 1, 4, 4, 8, 8), device="cuda", dtype=torch.int32)
    head = (cls.data_ptr(), m.data_ptr(), grid.data_ptr(), y.data_ptr(), cl.data_ptr(), counts.data_ptr(), acc.data_ptr())
    dims = (1, 4, 4, 4, 8, 8)
    hip.call("fs_unwarp_trimap", *head, trim.data_ptr(), None, scr.data_ptr(), *dims, 5, 1)
    assert torch.equal(trim, ops.unwarp_trimap(cls, m, grid, y, cl)[2])
    for bad in ((*head, None, None, scr.data_ptr(), *dims, 5, 1),                       # no trim
                (*head[:3], None, *head[4:], trim.data_ptr(), None, scr.data_ptr(), *dims, 5, 1),       # no label mask
                (*head, trim.data_ptr(), None, None, *dims, 5, 1),                      # no scratch
                (*head, trim.data_ptr(), None, scr.data_ptr(), *dims, 8, 1),            # D
                (*head, trim.data_ptr(), None, scr.data_ptr(), *dims, -1, 1),
                (*head, trim.data_ptr(), None, scr.data_ptr(), *dims, 5, 2),            # frame
                (*head, trim.data_ptr(), None, scr.data_ptr(), 1, 4, 4, 4, 0, 8, 5, 1)):
        with pytest.raises(hip.HipLibraryError):
            hip.call("fs_unwarp_trimap", *bad)


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
def test_evaluate_with_trimap(kind, size, seg, deterministic):
    module = _module(kind)
    K = module.cfg.DATASET.num_class
    X, Fp, Y, cl = T.synthetic_batch(2, size, size, seed=11, device="cuda")
    if seg is not None:
        _, _, Y, _ = T.synthetic_batch(2, seg[0], seg[1], seed=11, device="cuda")
    base = module.evaluate(X, Fp, Y, cl, seg)
    assert len(base) == 5                                                               # without the keyword: today's tuple
    out = module.evaluate(X, Fp, Y, cl, seg, trimap=5)
    module.check_nan()
    assert len(out) == 6 and all(torch.equal(a, b) for a, b in zip(out[:5], base))
    want = _trim_ref(module.predict(X, Fp, seg), Y, cl, K, 5, True)
    assert torch.equal(out[5], want) and int(want[:, 0, 0].min()) > 0
    both = module.evaluate(X, Fp, Y, cl, seg, return_labels=True, trimap=5, trimap_frame=False)
    assert len(both) == 7 and torch.equal(both[5], module.predict(X, Fp, seg))          # the class map, then trim last
    assert torch.equal(both[6], _trim_ref(both[5], Y, cl, K, 5, False))
    with pytest.raises(ValueError):
        module.evaluate(X, Fp, Y, cl, seg, trimap=9)


@pytest.mark.gpu
def test_evaluate_step_feeds_both_meters():
    module = _module("hrnet")
    meter, tmeter = T.FullResMeter("cuda"), T.TrimapMeter("cuda", 5)
    rows, trims = [], []
    for seed, B in ((1, 2), (2, 3)):
        batch = T.synthetic_batch(B, 128, 128, seed=seed, device="cuda")
        out = T.evaluate_step(module, batch, meter, tmeter)
        assert len(out) == 6 and torch.equal(out[4], T.evaluate_step(module, batch)[4])
        rows.append(out[4].cpu())
        trims.append(out[5].cpu())
    res, tres = meter.result(), tmeter.result()
    assert res["images"] == 5 and res["counts"] == torch.cat(rows).sum(0).tolist()
    trim = torch.cat(trims)
    assert tres["counts"] == trim.sum(0).tolist() and tres["images"] == [5] * 6 and tres["widths"] == [1, 2, 4, 8, 16, 32]
    mean = ops.trimap_from_counts(trim).mean(0)
    for i in range(6):
        assert abs(tres["acc"][i] - float(mean[i, 0])) <= 1e-12 and abs(tres["acc_bin"][i] - float(mean[i, 1])) <= 1e-12


@pytest.mark.gpu
def test_trimap_adds_the_byte_map_and_its_scratch():
    """evaluate(trimap=5) may hold, beyond evaluate(): the band byte per pixel, the row pass's byte per pixel (rows pitched to 4), one
    96-byte bucket record per 1 024 pixels and the (B,6,3) int64 result; 4 KiB for the allocator's 512-byte rounding of those blocks."""
    module = _module("hrnet")
    B, H, W, D = 2, 1024, 1024, 5
    X, Fp, Y, cl = T.synthetic_batch(B, H, W, seed=9, device="cuda")

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated()
    module.evaluate(X, Fp, Y, cl)                                                       # warm-up: weight packs, workspaces
    module.evaluate(X, Fp, Y, cl, trimap=D)
    _, plain = peak_of(lambda: module.evaluate(X, Fp, Y, cl))
    out, with_trim = peak_of(lambda: module.evaluate(X, Fp, Y, cl, trimap=D))
    module.check_nan()
    allowed = B * H * W + B * H * ((W + 3) // 4 * 4) + B * ((H * W + 1023) // 1024) * 96 + B * (D + 1) * 3 * 8 + 4096
    print(f"evaluate(trimap=5) peak over evaluate(): {with_trim - plain} bytes, allowed {allowed}")
    assert out[5].shape == (B, D + 1, 3)
    assert with_trim - plain <= allowed
