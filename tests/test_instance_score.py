"""The confidence score of the gazed instance: ops.head_fg_q (fs_head_fg_q), ops.unwarp_instances(score=True)
(fs_unwarp_instances_scored), ops.instances_to_coco(conf=...) and DeformSegmentationModule.predict_instances(return_score=True).

The score is unpinned (the reference has none); tests/score_ref.py restates its definition in fp64 torch.  The CPU tests pin that
restatement to hand-derived answers.  Every GPU reference takes its fp32 values v from the device's own sampler -- per pixel
ops.unwarp_nearest(ops.PredAssemble(cls, m), ...), per grid point fs_grid_sample_fwd at the inverse coordinates -- so only the fp64
exponentials and their summation order differ between reference and device.  A q may then differ by 1 only where the reference's
P * 2^24 lies within score_ref.band(K) of a half-integer; the tests assert that their seeded inputs have no such point and compare
with torch.equal.  At the C ABI every output sits NaN- or marker-filled between guard bands (kernel_testing.Out), the scratch too."""
import math

import numpy as np
import pytest
import torch

from fovealseg import hip, ops

import rle_ref as R
import score_ref as S

ONE = 2 ** 24
FAKE = 4096                                              # a non-null pointer for calls that must be refused before anything reads it


# ------------------------------------------------------------------------------------------------------------------ CPU ----------
def _interior(h, w):
    return 1 * w + 1                                     # grid point (1,1): all four taps in bounds


def test_reference_hand_derived_answers():
    h = w = 4
    p = _interior(h, w)
    m = torch.rand(1, h, w, generator=torch.Generator().manual_seed(0))
    # exp(ln 3) / (exp(ln 3) + exp(0 * m)) = 3/4, and 0.75 * 2^24 = 12 582 912; fp32(ln 3) moves P by 6e-9, x by 0.1
    q, _ = S.q_from_v(S.point_values_cpu(torch.tensor([[math.log(3.0), 0.0]]), m))
    assert int(q[0, p]) == 12582912 and int(q[0, h * w]) == 12582912
    # 4 * 0.25 = 1 = the constant plane: a tie, P = 1/2 exactly; the argmax is the first maximum, class 0: foreground
    v = S.point_values_cpu(torch.tensor([[1.0, 4.0]]), torch.full((1, h, w), 0.25))
    q, x = S.q_from_v(v)
    assert int(q[0, p]) == 2 ** 23 and float(x[0, p]) == 2.0 ** 23 and int(v[0, p].argmax()) == 0
    # 200 * +-0.4 = +-80: 1 / (1 + e^80) = 1.8e-35 -> 0, 1 / (1 + e^-80) -> 2^24
    for sign, want in ((1.0, 0), (-1.0, ONE)):
        q, _ = S.q_from_v(S.point_values_cpu(torch.tensor([[0.0, 200.0]]), torch.full((1, h, w), 0.4 * sign)))
        assert int(q[0, p]) == want


def test_reference_nan_and_range():
    v = torch.tensor([[0.0, float("nan"), 1.0], [float("inf"), 0.0, 0.0], [-float("inf")] * 3, [1.0, 2.0, 3.0]])
    q, x = S.q_from_v(v)
    assert q[:3].tolist() == [0, 0, 0] and bool(torch.isnan(x[:3]).all())
    assert 0 < int(q[3]) < ONE and S.in_band(x, 3) == 0
    assert S.in_band(torch.tensor([5.5, 7.5 + S.band(51) / 2, 7.5 + 2 * S.band(51), float("nan")], dtype=torch.float64), 51) == 2
    assert S.band(51) == 2.0 * 53 * 2.0 ** -28 and S.band(1024) < 1e-2       # far below the half unit it guards
    ref = S.conf_ref(torch.tensor([[0.0, math.log(3.0), 9.0]]), torch.tensor([1]), torch.tensor([3 * ONE // 2]), torch.tensor([2]))
    assert torch.allclose(ref, torch.tensor([[0.75 * 0.75, 0.75, 0.75]], dtype=torch.float64), atol=1e-7)
    assert S.conf_ref(torch.zeros(1, 3), torch.tensor([0]), torch.tensor([0]), torch.tensor([0])).tolist() == [[0.0, 0.5, 0.0]]


def _cpu_records():
    masks = [np.array([[0, 1], [1, 1], [0, 0]], dtype=bool), np.zeros((3, 2), dtype=bool)]
    cat = torch.tensor([4, 0])
    stats = torch.tensor([R.stats(m) for m in masks])
    counts = torch.from_numpy(np.stack([R.counts_row(m, 7) for m in masks]))
    return cat, stats, counts


def test_instances_to_coco_with_conf_on_cpu_tensors():
    cat, stats, counts = _cpu_records()
    conf = torch.tensor([[0.8125, 0.9, 0.9], [0.0, 0.25, 0.0]])
    plain = ops.instances_to_coco(cat, stats, counts, (3, 2), image_ids=[17, "b"])
    recs = ops.instances_to_coco(cat, stats, counts, (3, 2), image_ids=[17, "b"], conf=conf)
    assert plain[0] == {"image_id": 17, "category_id": 4, "bbox": [0, 0, 2, 2], "area": 3,
                        "segmentation": {"size": [3, 2], "counts": [1, 1, 1, 2, 1]}}      # without conf: the record as it was
    assert all("score" not in r for r in plain)
    assert [r["score"] for r in recs] == [0.8125, 0.0] and all(type(r["score"]) is float for r in recs)
    for r, p in zip(recs, plain):
        assert {k: v for k, v in r.items() if k != "score"} == p
    assert ops.instances_to_coco(cat, stats, counts, (3, 2), conf=conf.double())[0]["score"] == 0.8125
    third = float(torch.tensor(1 / 3, dtype=torch.float32))
    assert ops.instances_to_coco(cat, stats, counts, (3, 2), conf=torch.tensor([[1 / 3, 1, 1], [0, 0, 0]]))[0]["score"] == third
    bad = conf.clone()
    bad[1, 0] = float("nan")
    with pytest.raises(ValueError, match="image b"):
        ops.instances_to_coco(cat, stats, counts, (3, 2), image_ids=[17, "b"], conf=bad)
    bad[1, 0], bad[1, 1] = 0.0, float("nan")            # only the score is looked at
    assert len(ops.instances_to_coco(cat, stats, counts, (3, 2), conf=bad)) == 2
    with pytest.raises(ValueError):
        ops.instances_to_coco(cat, stats, counts, (3, 2), conf=conf[:1])
    with pytest.raises(OverflowError, match=r"image 17.*max_runs >= 5"):
        ops.instances_to_coco(cat, stats, counts[:, :4], (3, 2), image_ids=[17, "b"], conf=conf)


def test_the_ctypes_table_binds_the_score_symbols():
    assert hip.SIGNATURES["fs_head_fg_q"] == "ppp" + "iiii"
    assert hip.SIGNATURES["fs_unwarp_instances_scored"] == "p" * 10 + "i" * 7
    assert hip.SIGNATURES["fs_unwarp_instances"] == "p" * 8 + "i" * 7                  # the unscored entry point is what it was
    assert "fs_unwarp_instances_scored_scratch_ints" in hip.HOST_ONLY
    lib = hip.load()
    for name in ("fs_head_fg_q", "fs_unwarp_instances_scored", "fs_unwarp_instances_scored_scratch_ints"):
        assert getattr(lib, name) is not None


def test_scored_scratch_query():
    assert hip.query("fs_unwarp_instances_scored_scratch_ints", 0, 4, 4, 9, 7) == 0
    for B, h, w, Hs, Ws in ((2, 4, 5, 1, 1), (2, 4, 5, 9, 7), (2, 9, 11, 8, 8), (3, 9, 11, 65, 33), (2, 80, 80, 1024, 1024)):
        plain = hip.query("fs_unwarp_instances_scratch_ints", B, h, w, Hs, Ws)
        scored = hip.query("fs_unwarp_instances_scored_scratch_ints", B, h, w, Hs, Ws)
        # two more regions behind the unscored layout, 16-byte aligned: a word per grid point (and the no-claim entry), and the records
        # of the gather's waves -- two ints for every 8 bit words where Ws % 4 == 0, one for every 2 otherwise
        words = B * Hs * ((Ws + 31) // 32)
        more = B * (h * w + 1) + (8 * ((words + 31) // 32) if Ws % 4 == 0 else 4 * ((words + 7) // 8))
        assert plain + more <= scored <= plain + more + 6
    B, h, w, Hs, Ws = 2, 80, 80, 1024, 1024
    more = hip.query("fs_unwarp_instances_scored_scratch_ints", B, h, w, Hs, Ws) - hip.query("fs_unwarp_instances_scratch_ints", B, h, w, Hs, Ws)
    assert 0 <= more < B * Hs * Ws // 8                                                # ints: less than a bit a pixel


def _refused(name, *args):
    """The call is refused at the C ABI; with a null stream, so that it can be made where there is no device: a refusal comes before
    the first launch and reads no argument."""
    old = hip.set_stream_override(0)
    try:
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call(name, *args)
    finally:
        hip.set_stream_override(old)


def test_argument_checks_on_the_host():
    B, K, h, w, Hs, Ws, cap = 1, 4, 4, 4, 8, 8, 20
    ptrs = [FAKE] * 10                                   # cls m grid cat stats counts bits conf qsum scratch
    _refused("fs_unwarp_instances_scored", *ptrs, B, K, h, w, Hs, Ws, 0)                 # cap = 0
    _refused("fs_unwarp_instances_scored", *ptrs, B, 1, h, w, Hs, Ws, cap)               # K = 1
    _refused("fs_unwarp_instances_scored", *ptrs, B, 1025, h, w, Hs, Ws, cap)            # K beyond the kernels' 1 024
    _refused("fs_unwarp_instances_scored", *ptrs, B, K, h, w, 1, 16385, cap)             # a row longer than the row pass's LDS
    _refused("fs_unwarp_instances_scored", *ptrs, 0, K, h, w, Hs, Ws, cap)
    _refused("fs_unwarp_instances_scored", *ptrs, B, K, h, w, 65536, 32768, cap)         # Hs * Ws = 2^31
    for i in (0, 1, 2, 3, 4, 5, 7, 8, 9):                                                # bits (6) alone may be null
        a = list(ptrs)
        a[i] = None
        _refused("fs_unwarp_instances_scored", *a, B, K, h, w, Hs, Ws, cap)
    for i in range(3):
        a = [FAKE] * 3
        a[i] = None
        _refused("fs_head_fg_q", *a, B, K, h, w)
    for dims in ((0, K, h, w), (B, 1, h, w), (B, 1025, h, w), (B, K, 0, w), (B, K, h, 0)):
        _refused("fs_head_fg_q", FAKE, FAKE, FAKE, *dims)


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ----
def _kt():
    import kernel_testing as KT
    return KT


def _tp():
    import test_predict as TP
    return TP


def _table(cls, m):
    """fs_head_fg_q at the C ABI -> (B, h*w+1) int32 on the host; every entry written, guards intact."""
    B, K = cls.shape
    h, w = int(m.shape[1]), int(m.shape[2])
    q = _kt().Out(B * (h * w + 1), torch.int32)
    hip.call("fs_head_fg_q", cls.data_ptr(), m.data_ptr(), q.ptr, B, K, h, w)
    return q.get().view(B, h * w + 1)


def _table_inputs(B, K, h, w, variant):
    g = torch.Generator().manual_seed(B * 1000 + K * 10 + h + {"plain": 0, "saturated": 1, "nan_m": 2, "nan_cls": 3}[variant] * 7919)
    cls = torch.randn(B, K, generator=g)
    cls[:, K - 1] = 3 * cls.abs().amax(1)
    m = torch.rand(B, h, w, generator=g) - 0.5
    if variant == "saturated":
        m = torch.where(torch.rand(B, h, w, generator=g) < 0.5, -torch.ones(B, h, w), torch.ones(B, h, w)) * (80.0 / cls[:, K - 1, None, None])
    elif variant == "nan_m":
        m[B - 1, h // 2, w // 2] = float("nan")
        m[0, 0, 0] = float("nan")                        # a corner: the only in-bounds tap of point (0,0)
    elif variant == "nan_cls":
        cls[B - 1, 0] = float("nan")                     # a constant plane: every point of that image
    return cls.cuda(), m.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "saturated", "nan_m", "nan_cls"])
@pytest.mark.parametrize("B,K,h,w", [(2, 2, 3, 5), (3, 51, 8, 8), (1, 1024, 4, 4), (2, 6, 9, 11)])
def test_head_fg_q_table(B, K, h, w, variant):
    """The border points (row 0 / column 0: two or three of the four taps out of bounds, weight 1/2 or 1/4 left) are part of every
    case; with the inverse coordinates fixed by (h, w) no point loses all four taps."""
    cls, m = _table_inputs(B, K, h, w, variant)
    v = S.point_values_dev(cls, m)
    want, x = S.q_from_v(v)
    assert S.in_band(x, K) == 0, "the seeded input has a point inside the rounding band: pick another seed"
    got = _table(cls, m)
    assert torch.equal(got, want.cpu())
    assert torch.equal(ops.head_fg_q(cls, m).cpu(), got)
    assert int(got.min()) >= 0 and int(got.max()) <= ONE
    nan_rows = torch.isnan(x).cpu()
    assert bool((got[nan_rows] == 0).all())
    if variant == "saturated":
        assert bool((got == 0).any()) and bool((got == ONE).any())       # e^-80 against the constant planes, and e^80
        assert 79.0 < float(v[..., K - 1].abs().max()) < 81.0               # |cls_bg * m| = 80 at every tap; bilinear means of +-80 between
    if variant == "nan_m":
        assert bool(nan_rows[B - 1].any()) and not bool(nan_rows[B - 1].all()) and bool(nan_rows[0, 0])
    if variant == "nan_cls":
        assert bool(nan_rows[B - 1].all()) and (B == 1 or not bool(nan_rows[0].any()))
    # the border points really are partial samples: a constant plane reads below its value there
    if variant == "plain":
        c0 = cls[:, 0].cpu()
        assert torch.allclose(v[:, 0, 0].cpu(), c0 * 0.25, rtol=1e-5, atol=1e-6) and torch.allclose(v[:, w + 1, 0].cpu(), c0, rtol=1e-5, atol=1e-6)


def _scored(cls, m, grid, Hs, Ws, cap, with_bits=True):
    """fs_unwarp_instances_scored at the C ABI -> dict of host tensors; outputs complete, guards and scratch bands intact."""
    KT = _kt()
    B, K = cls.shape
    _, h, w, _ = grid.shape
    P = (Ws + 31) // 32
    o = {"cat": KT.Out(B, torch.int64), "stats": KT.Out(B * 6, torch.int64), "counts": KT.Out(B * cap, torch.int32),
         "conf": KT.Out(B * 3, torch.float32, fill=777.5), "qsum": KT.Out(B, torch.int64)}
    if with_bits:
        o["bits"] = KT.Out(B * Hs * P, torch.int32, fill=0x3C3C3C3D)
    scr = KT.Out(hip.query("fs_unwarp_instances_scored_scratch_ints", B, h, w, Hs, Ws), torch.int32)
    hip.call("fs_unwarp_instances_scored", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), o["cat"].ptr, o["stats"].ptr, o["counts"].ptr,
             o["bits"].ptr if with_bits else None, o["conf"].ptr, o["qsum"].ptr, scr.ptr, B, K, h, w, Hs, Ws, cap)
    scr.get(complete=False)                              # the bands around the queried ints
    out = {k: t.get() for k, t in o.items()}             # conf's fill is a number: a NaN result counts as written
    return {"cat": out["cat"], "stats": out["stats"].view(B, 6), "counts": out["counts"].view(B, cap), "conf": out["conf"].view(B, 3),
            "qsum": out["qsum"], **({"bits": out["bits"].view(B, Hs, P)} if with_bits else {})}


def _unscored(cls, m, grid, Hs, Ws, cap):
    KT = _kt()
    B, K = cls.shape
    _, h, w, _ = grid.shape
    P = (Ws + 31) // 32
    o = {"cat": KT.Out(B, torch.int64), "stats": KT.Out(B * 6, torch.int64), "counts": KT.Out(B * cap, torch.int32),
         "bits": KT.Out(B * Hs * P, torch.int32, fill=0x3C3C3C3D)}
    scr = KT.Out(hip.query("fs_unwarp_instances_scratch_ints", B, h, w, Hs, Ws), torch.int32)
    hip.call("fs_unwarp_instances", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), o["cat"].ptr, o["stats"].ptr, o["counts"].ptr,
             o["bits"].ptr, scr.ptr, B, K, h, w, Hs, Ws, cap)
    scr.get(complete=False)
    out = {k: t.get() for k, t in o.items()}
    return {"cat": out["cat"], "stats": out["stats"].view(B, 6), "counts": out["counts"].view(B, cap), "bits": out["bits"].view(B, Hs, P)}


def _check_conf(got, cls):
    """conf against the fp64 reference made from the call's own integers: mask_prob bit for bit (one correctly rounded fp64 division
    and one rounding to fp32 on both sides), cls_prob and score within one fp32 ulp, NaN exactly where the reference is."""
    area = got["stats"][:, 0]
    ref = S.conf_ref(cls.cpu(), got["cat"], got["qsum"], area)
    conf = got["conf"]
    assert torch.equal(conf[:, 2], torch.where(area > 0, got["qsum"].double() / (area.double().clamp_min(1) * ONE),
                                               torch.zeros(len(area), dtype=torch.float64)).float())
    for col, name in ((0, "score"), (1, "cls_prob")):
        nan = torch.isnan(ref[:, col])
        assert torch.equal(torch.isnan(conf[:, col]), nan), name
        u = S.ulps32(conf[~nan, col], ref[~nan, col])
        print(f"{name}: worst {float(u.max()) if u.numel() else 0.0:.3f} fp32 ulp")
        assert bool((u <= 1.0).all()), name
    assert torch.equal(torch.isnan(conf[:, 0]), torch.isnan(conf[:, 1]))
    ok = ~torch.isnan(conf[:, 0])
    assert bool(((0 <= conf[ok, 0]) & (conf[ok, 0] <= conf[ok, 1]) & (conf[ok, 1] <= 1)).all()) and bool(((0 <= conf[:, 2]) & (conf[:, 2] <= 1)).all())
    assert bool((conf[area == 0][:, [0, 2]].nan_to_num(0.0) == 0).all())
    return ref


def _check_scored(cls, m, grid, Hs, Ws):
    """The scored call against the unscored one (bit for bit) and the unfused route (qsum), then conf; without bits the same."""
    B, K = cls.shape
    mask, qsum, close = S.pixel_reference(cls, m, grid, Hs, Ws)
    assert close == 0, "the seeded input has a point inside the rounding band: pick another seed"
    cap = max(R.stats(mk)[5] for mk in mask.cpu().numpy()) + 2
    got, plain = _scored(cls, m, grid, Hs, Ws, cap), _unscored(cls, m, grid, Hs, Ws, cap)
    for k in plain:
        assert torch.equal(got[k], plain[k]), k
    assert np.array_equal(got["bits"].numpy(), np.stack([R.bits(mk) for mk in mask.cpu().numpy()]))
    assert torch.equal(got["qsum"], qsum.cpu())
    _check_conf(got, cls)
    without = _scored(cls, m, grid, Hs, Ws, cap, with_bits=False)                      # bits = NULL: the words stay in scratch
    for k in without:                                                                  # conf by its words: a NaN equals itself
        assert torch.equal(without[k].view(torch.int32) if k == "conf" else without[k], got[k].view(torch.int32) if k == "conf" else got[k]), k
    return got, mask


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 6), (50, 513, 3), (8, 1500, 2), (9, 7, 4), (8, 8, 4), (300, 200, 51)])
def test_scored_instances_against_the_unfused_route(Hs, Ws, K):
    """Both gathers (Ws % 4 == 0 and not), ragged word tails (300, 513, 1500, 7, 200 columns), and workgroups spanning two images:
    (9, 7) has 9 words an image against 8 a workgroup, (8, 8) 8 against 32, (37, 300) 370 against 32."""
    cls, m, grid = _tp()._inputs(2, K, 9, 11, Hs * 1000 + Ws)
    got, mask = _check_scored(cls, m, grid, Hs, Ws)
    assert bool(mask.any()) and not bool(mask.all())
    assert bool((got["conf"][:, 0] > 0).all())
    c2, s2, n2, conf, qsum = ops.unwarp_instances(cls, m, grid, Hs, Ws, max_runs=got["counts"].shape[1], score=True)     # the op
    assert torch.equal(conf.cpu().view(torch.int32), got["conf"].view(torch.int32)) and torch.equal(qsum.cpu(), got["qsum"])
    assert torch.equal(c2.cpu(), got["cat"]) and torch.equal(s2.cpu(), got["stats"]) and torch.equal(n2.cpu(), got["counts"])
    six = ops.unwarp_instances(cls, m, grid, Hs, Ws, return_bits=True, score=True)
    assert len(six) == 6 and torch.equal(six[3].cpu(), got["bits"]) and torch.equal(six[5].cpu(), got["qsum"])
    assert len(ops.unwarp_instances(cls, m, grid, Hs, Ws)) == 3                        # the default call is what it was


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 6), (8, 8, 4), (9, 7, 4)])
def test_scored_instances_scratch_off_16_bytes(Hs, Ws, K):
    """A scratch that is only 4-byte aligned takes the one-pixel gather at every width; where Ws % 4 == 0 the records were sized for
    the other one and every sum goes through the atomics.  The results are the aligned call's."""
    KT = _kt()
    cls, m, grid = _tp()._inputs(2, K, 9, 11, Hs * 1000 + Ws)
    B, cap, P = 2, 8 * Ws + 1, (Ws + 31) // 32
    want = ops.unwarp_instances(cls, m, grid, Hs, Ws, return_bits=True, score=True)
    ints = hip.query("fs_unwarp_instances_scored_scratch_ints", B, 9, 11, Hs, Ws)
    scr = KT.Out(ints + 4, torch.int32)
    o = [KT.Out(B, torch.int64), KT.Out(B * 6, torch.int64), KT.Out(B * cap, torch.int32), KT.Out(B * Hs * P, torch.int32, fill=0x3C3C3C3D),
         KT.Out(B * 3, torch.float32, fill=777.5), KT.Out(B, torch.int64)]
    hip.call("fs_unwarp_instances_scored", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), *[t.ptr for t in o], scr.ptr + 4, B, K, 9, 11, Hs, Ws, cap)
    body = scr.get(complete=False)
    assert int(body[0]) == -9999 and bool((body[ints + 1:] == -9999).all())             # the ints before and behind the shifted scratch
    for t, w in zip(o, want):
        got = t.get().view(w.shape)
        assert torch.equal(got.view(torch.int32) if w.dtype == torch.float32 else got, w.cpu().view(torch.int32) if w.dtype == torch.float32 else w.cpu())


@pytest.mark.gpu
def test_scored_instances_border_grids():
    g = torch.Generator().manual_seed(5)                                             # test_instances.py's border grids
    grid = torch.rand(2, 16, 20, 2, generator=g) * 2 - 1
    edge = torch.rand(2, 16, 20, 2, generator=g)
    grid = torch.where(edge < 0.3, torch.full_like(grid, -1.0), torch.where(edge > 0.7, torch.ones_like(grid), grid))
    cls = torch.randn(2, 7, generator=g)
    cls[:, 6] = 3 * cls.abs().amax(1)
    m = torch.rand(2, 16, 20, generator=g) - 0.5
    for Hs, Ws in ((45, 70), (45, 72)):
        _check_scored(cls.cuda(), m.cuda(), grid.cuda(), Hs, Ws)


@pytest.mark.gpu
def test_scored_instances_no_claimed_pixel():
    TP = _tp()
    for seed, fg in ((3, None), (4, True)):
        cls, m, grid = TP._inputs(2, 9, 10, 12, seed)
        grid[1] = 1.5                                                                # image 1: every pixel feeds from entry h*w, the sample at (0,0)
        if fg:
            m[1] = -1.0                                                              # ... and is foreground
        for Hs, Ws in ((31, 41), (31, 40)):
            got, mask = _check_scored(cls, m, grid, Hs, Ws)
            table = ops.head_fg_q(cls, m).cpu()
            if bool(mask[1].all()):
                assert int(got["qsum"][1]) == Hs * Ws * int(table[1, 10 * 12])
            else:
                assert not bool(mask[1].any()) and int(got["qsum"][1]) == 0
    assert fg and bool(mask[1].all())                                                # the second seed's image 1 was all foreground


@pytest.mark.gpu
def test_scored_instances_all_foreground_sum_exceeds_32_bits():
    cls, m, grid = _tp()._inputs(2, 5, 9, 11, 12)
    cls[:, 4] = 400.0
    m[:] = -1.0                                                                      # background logit -400 (-100 at a corner point): P = 1 in fp64
    Hs, Ws = 300, 200
    got, mask = _check_scored(cls, m, grid, Hs, Ws)
    assert bool(mask.all())
    assert got["qsum"].tolist() == [Hs * Ws * ONE] * 2 and Hs * Ws * ONE > 2 ** 32
    assert got["conf"][:, 2].tolist() == [1.0, 1.0] and torch.equal(got["conf"][:, 0], got["conf"][:, 1])


@pytest.mark.gpu
def test_scored_instances_empty_mask():
    cls, m, grid = _tp()._inputs(2, 5, 9, 11, 13)
    m[0] = 1.0                                                                       # image 0: the mask plane wins everywhere
    got, mask = _check_scored(cls, m, grid, 40, 52)
    assert not bool(mask[0].any()) and bool(mask[1].any())
    cp = torch.softmax(cls[0, :4].double(), 0).max().float().cpu()
    assert got["conf"][0, 0] == 0 and got["conf"][0, 2] == 0 and abs(float(got["conf"][0, 1]) - float(cp)) <= 1.2e-7 * float(cp)
    assert int(got["qsum"][0]) == 0 and got["stats"][0].tolist() == [0, 0, 0, 0, 0, 1]


@pytest.mark.gpu
def test_scored_instances_nan():
    cls, m, grid = _tp()._inputs(2, 6, 8, 8, 6)
    cls[0, 3] = float("nan")                                                         # class 3 everywhere, every q = 0: cls_prob and score NaN
    m[1, 2:5, 1:6] = float("nan")                                                    # image 1: NaN points are background, its score is defined
    got, mask = _check_scored(cls, m, grid, 20, 30)
    assert bool(mask[0].all()) and int(got["qsum"][0]) == 0 and int(got["cat"][0]) == 3
    assert math.isnan(float(got["conf"][0, 0])) and math.isnan(float(got["conf"][0, 1])) and float(got["conf"][0, 2]) == 0.0
    assert not bool(torch.isnan(got["conf"][1]).any()) and float(got["conf"][1, 0]) > 0
    cls[0, 3], cls[0, 5] = 0.0, float("nan")                                        # the mask plane's factor: background everywhere
    got, mask = _check_scored(cls, m, grid, 20, 32)
    assert not bool(mask[0].any()) and got["conf"][0, [0, 2]].tolist() == [0.0, 0.0] and not math.isnan(float(got["conf"][0, 1]))


@pytest.mark.gpu
def test_scored_instances_full_size():
    cls, m, grid = _tp()._inputs(2, 51, 80, 80, 7, -1.0, 1.0)
    got, mask = _check_scored(cls, m, grid, 1024, 1024)
    assert bool(mask.any()) and not bool(mask.all())
    print(f"full size: areas {got['stats'][:, 0].tolist()}, qsum {got['qsum'].tolist()}, conf {got['conf'].tolist()}")


@pytest.mark.gpu
def test_scored_instances_repeat_bit_for_bit_in_every_mode():
    cls, m, grid = _tp()._inputs(2, 6, 9, 11, 37300)
    mode0, det0 = hip.get_conv_precision(), hip.get_deterministic()
    runs = []
    try:
        for mode in ("f32", "bf16x3", "f16x2"):
            for det in (True, False):
                hip.set_conv_precision(mode)
                hip.set_deterministic(det)
                for _ in range(2):
                    runs.append(ops.unwarp_instances(cls, m, grid, 37, 300, return_bits=True, score=True))
    finally:
        hip.set_conv_precision(mode0)
        hip.set_deterministic(det0)
    assert len(runs) == 12
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.gpu
def test_scored_entry_points_reject_bad_arguments():
    KT = _kt()
    B, K, h, w, Hs, Ws, cap = 1, 4, 4, 4, 8, 8, 20
    cls, m, grid = _tp()._inputs(B, K, h, w, 0)
    outs = [KT.Out(B, torch.int64), KT.Out(B * 6, torch.int64), KT.Out(B * cap, torch.int32), KT.Out(B * 513, torch.int32), KT.Out(B * 3),
            KT.Out(B, torch.int64),
            KT.Out(max(hip.query("fs_unwarp_instances_scored_scratch_ints", B, h, w, Hs, Ws),
                       hip.query("fs_unwarp_instances_scored_scratch_ints", B, h, w, 1, 16385)), torch.int32)]
    table = KT.Out(B * (h * w + 1), torch.int32)
    head = (cls.data_ptr(), m.data_ptr(), grid.data_ptr())
    ptrs = [t.ptr for t in outs]

    def rejected(name, *args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call(name, *args)

    rejected("fs_unwarp_instances_scored", *head, *ptrs, B, K, h, w, Hs, Ws, 0)
    rejected("fs_unwarp_instances_scored", *head, *ptrs, B, 1, h, w, Hs, Ws, cap)
    rejected("fs_unwarp_instances_scored", *head, *ptrs, B, K, h, w, 1, 16385, cap)
    for i in (0, 1, 2):
        a = list(head)
        a[i] = None
        rejected("fs_unwarp_instances_scored", *a, *ptrs, B, K, h, w, Hs, Ws, cap)
    for i in (0, 1, 2, 4, 5, 6):                                                       # bits (3) alone may be null
        a = list(ptrs)
        a[i] = None
        rejected("fs_unwarp_instances_scored", *head, *a, B, K, h, w, Hs, Ws, cap)
    rejected("fs_head_fg_q", cls.data_ptr(), m.data_ptr(), None, B, K, h, w)
    rejected("fs_head_fg_q", cls.data_ptr(), m.data_ptr(), table.ptr, B, 1, h, w)
    for t in outs + [table]:                                                           # nothing was launched
        assert t.untouched()
    with pytest.raises(ValueError):
        ops.unwarp_instances(cls, m[:, :3], grid, Hs, Ws, score=True)
    with pytest.raises(ValueError):
        ops.head_fg_q(cls, m[0])


# ------------------------------------------------------------------------------------------------------------------ GPU: module ---
@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [None, (200, 180)])
def test_predict_instances_with_score(seg, deterministic):
    TP = _tp()
    module, _ = TP._module("hrnet")
    K = module.cfg.DATASET.num_class
    X, Fp = TP._batch(2, 256, 11)
    bias = module.decoder.cls_net.fc.bias            # test_instances.py: a large background logit lets the mask plane decide where m > 0
    keep = bias.detach().clone()
    with torch.no_grad():
        bias[-1] += 1000.0
    try:
        state = {k: v.detach().clone() for k, v in module.state_dict().items()}
        step0 = ops.DropoutState.step
        X0, F0 = X.clone(), Fp.clone()
        scored = module.predict_instances(X, Fp, seg, return_bits=True, return_score=True)
        module.check_nan()
        assert ops.DropoutState.step == step0 and torch.equal(X, X0) and torch.equal(Fp, F0)
        for k, v in module.state_dict().items():
            assert torch.equal(v, state[k]), k
        plain = module.predict_instances(X, Fp, seg, return_bits=True)
        four = module.predict_instances(X, Fp, seg, return_score=True)
        H, W = seg or (256, 256)
        labels, grid = TP._chained(module, X, Fp, (H, W))
        with torch.no_grad():                                                         # the hand-chained stages up to the head's two factors
            feat = module.encoder.forward_nhwc(ops.GridSample.apply(X, grid))
            cls, m = module.decoder.forward_parts_nhwc(feat)
            by_hand = ops.unwarp_instances(cls, m, grid, H, W, return_bits=True, score=True)
    finally:
        with torch.no_grad():
            bias.copy_(keep)
    assert len(scored) == 5 and len(plain) == 4 and len(four) == 4
    for a, b in zip(scored[:4], plain):
        assert torch.equal(a, b)
    conf = scored[4]
    assert conf.dtype == torch.float32 and conf.shape == (2, 3)
    assert torch.equal(four[3], conf) and torch.equal(four[0], plain[0]) and torch.equal(four[2], plain[2])
    assert torch.equal(conf, by_hand[4]) and torch.equal(scored[3], by_hand[3])
    mask = (labels != K - 1).cpu().numpy()
    assert np.array_equal(scored[3].cpu().numpy(), np.stack([R.bits(mk) for mk in mask]))
    c = conf.cpu()
    print(f"predict_instances {H}x{W}: conf {c.tolist()}, areas {scored[1][:, 0].tolist()}")
    assert bool(((0 <= c[:, 0]) & (c[:, 0] <= c[:, 1]) & (c[:, 1] <= 1)).all())
    ref = S.conf_ref(cls.cpu(), scored[0].cpu(), by_hand[5].cpu(), scored[1][:, 0].cpu())
    assert bool((S.ulps32(c, ref) <= 1.0).all())
    if int(scored[1][:, 5].max()) <= scored[2].shape[1]:
        recs = ops.instances_to_coco(*scored[:3], (H, W), image_ids=[7, 9], conf=conf)
        assert [r["score"] for r in recs] == c[:, 0].tolist() and all(type(r["score"]) is float for r in recs)
        assert [{k: v for k, v in r.items() if k != "score"} for r in recs] == ops.instances_to_coco(*plain[:3], (H, W), image_ids=[7, 9])


@pytest.mark.gpu
def test_predict_instances_with_score_rejects_train_mode():
    TP = _tp()
    module, _ = TP._module("hrnet")
    X, Fp = TP._batch(2, 96, 3)
    module.train()
    try:
        with pytest.raises(RuntimeError, match="predict_instances"):
            module.predict_instances(X, Fp, return_score=True)
    finally:
        module.eval()


@pytest.mark.gpu
def test_the_score_allocates_less_than_a_bit_per_pixel():
    TP = _tp()
    module, _ = TP._module("hrnet")
    B, Sz = 2, 1024
    X, Fp = TP._batch(B, Sz, 9)
    with torch.no_grad():
        module.predict_instances(X, Fp, return_score=True)                            # warm-up: weight packs, workspaces
        parts = module._head_parts(X, Fp, None, "test")
        peaks = []
        for score in (False, True, False, True):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = ops.unwarp_instances(*parts[:3], Sz, Sz, score=score)
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated() - base)
            del out
        del parts
    module.check_nan()
    print(f"unwarp_instances peak: unscored {peaks[0]} B, scored {peaks[1]} B, a bit per pixel {B * Sz * Sz // 8} B")
    assert peaks[0] == peaks[2] and peaks[1] == peaks[3]
    assert 0 < peaks[1] - peaks[0] < B * Sz * Sz // 8
