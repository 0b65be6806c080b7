"""Records in, records out: the run-length code back into bit words (fs_rle_bits, fs_rle_bits_scratch_ints, ops.rle_bits), the
compressed string form (ops.rle_to_string / rle_from_string), ops.instances_to_coco(compressed=True), ops.coco_to_instances,
DeformSegmentationModule.evaluate_instances with a run-length label and train.score_coco_records.

The format is unpinned (restated from its published definition, like tests/rle_ref.py): tests/rle_codec_ref.py restates the decoder
and the string form and is held to hand-derived answers first.  Every comparison is == / torch.equal: nothing here has a tolerance."""
import json
import os

import numpy as np
import pytest
import torch

from fovealseg import hip, ops
from fovealseg import train as T
from fovealseg.models import DeformSegmentationModule

import rle_codec_ref as C
import rle_ref as R


def parse(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


# ------------------------------------------------------------------------------------------ CPU: the decoder's reference by hand ----
def test_reference_empty_and_full():
    m, info = C.decode_info([200], 1, 5, 40)
    assert not m.any() and info == [0, 0, 1, 200]
    m, info = C.decode_info([0, 200], 2, 5, 40)
    assert m.all() and info == [0, 200, 2, 200]
    m, info = C.decode_info([1], 1, 1, 1)
    assert m.shape == (1, 1) and not m.any() and info == [0, 0, 1, 1]


def test_reference_run_crossing_the_bottom_of_a_column():
    # 3 rows, 4 columns, p = 3 x + y: two zeros, then five set pixels p = 2 .. 6 = (2,0), (0,1), (1,1), (2,1), (0,2), then five zeros
    m, info = C.decode_info([2, 5, 5], 3, 3, 4)
    assert np.array_equal(m, parse([".##.", ".#..", "##.."])) and info == [0, 5, 3, 12]
    assert R.encode(m) == [2, 5, 5]


def test_reference_zero_length_run_is_the_merged_code():
    # [2, 3, 0, 2, 5]: three set pixels, a run of zeros of length 0, two more set pixels = [2, 5, 5]
    merged, info_m = C.decode_info([2, 5, 5], 3, 3, 4)
    m, info = C.decode_info([2, 3, 0, 2, 5], 5, 3, 4)
    assert np.array_equal(m, merged) and info == [0, 5, 5, 12] and info_m[1] == 5
    # zero-length runs in front: no zeros, no ones, no zeros, then all twelve set
    m, info = C.decode_info([0, 0, 0, 12], 4, 3, 4)
    assert m.all() and info == [0, 12, 4, 12]
    # and behind: the closing runs are empty
    m, info = C.decode_info([12, 0, 0], 3, 3, 4)
    assert not m.any() and info == [0, 0, 3, 12]


def test_reference_statuses_and_their_precedence():
    # cap = 3 and a code of 4 counts: cut, whatever else is wrong with what was read
    m, info = C.decode_info([2, 5, 4], 4, 3, 4)
    assert not m.any() and info == [1, 0, 3, 11]                             # CUT before SUM
    m, info = C.decode_info([2, -5, 4], 4, 3, 4)
    assert not m.any() and info == [1, 0, 3, 1]                              # CUT before BAD (and before SUM)
    m, info = C.decode_info([2, -5, 4], 3, 3, 4)
    assert not m.any() and info == [2, 0, 3, 1]                              # BAD before SUM: the sum is 1, not 12
    m, info = C.decode_info([14, -2], 2, 3, 4)
    assert not m.any() and info == [2, 0, 2, 12]                             # a negative count with the right sum is still bad
    m, info = C.decode_info([2, 5, 4], 3, 3, 4)
    assert not m.any() and info == [3, 0, 3, 11]                             # short
    m, info = C.decode_info([2, 5, 6], 3, 3, 4)
    assert not m.any() and info == [3, 0, 3, 13]                             # long
    for n in (0, -1, -2 ** 40):
        m, info = C.decode_info([12, 0, 0], n, 3, 4)
        assert not m.any() and info == [2, 0, 0, 0]                          # no code at all: nothing read
    m, info = C.decode_info([2, 5, 5], 2 ** 40, 3, 4)
    assert info == [1, 0, 3, 12]


def test_reference_ignores_what_lies_past_n_runs():
    want, info_w = C.decode_info([2, 5, 5], 3, 3, 4)
    m, info = C.decode_info([2, 5, 5, -7, 99, -(2 ** 31)], 3, 3, 4)
    assert np.array_equal(m, want) and info == info_w == [0, 5, 3, 12]
    m, info = C.decode_info([12, -7], 1, 3, 4)
    assert not m.any() and info == [0, 0, 1, 12]


def test_reference_inverts_rle_ref():
    rng = np.random.default_rng(29)
    for Hs, Ws in ((1, 1), (1, 40), (5, 1), (5, 40), (3, 33)):
        for density in (0.0, 0.1, 0.5, 0.9, 1.0):
            mask = rng.random((Hs, Ws)) < density
            code = R.encode(mask)
            m, info = C.decode_info(code + [-1, -1], len(code), Hs, Ws)
            assert np.array_equal(m, mask) and np.array_equal(R.decode(code, Hs, Ws), mask)
            assert info == [0, int(mask.sum()), len(code), Hs * Ws]
            loose = C.with_zero_runs(code, rng)
            assert len(loose) == len(code) + 10
            m, info = C.decode_info(loose, len(loose), Hs, Ws)
            assert np.array_equal(m, mask) and info == [0, int(mask.sum()), len(loose), Hs * Ws]


# ------------------------------------------------------------------------------------------------------ CPU: the string form ----
# By hand, from the definition (5-bit groups, low first; a group that is followed carries 32; chr(group + 48)):
#   [0, 5]            0 -> group 0 -> '0' (48); 5 -> '5' (53)
#   [3, 2, 4, 2]      '3', '2', '4'; the fourth count is written as 2 - counts[1] = 0 -> '0'
#   [10, 20, 30, 5]   10 -> chr(58) = ':'; 20 = 10100b: bit 16 is set and what is left (0) is not -1, so a second group follows:
#                     20 + 32 = 52 -> chr(100) = 'd', then 0 -> '0'; 30 likewise: 62 -> chr(110) = 'n', then '0'; the fourth is 5 - 20 =
#                     -15 = ...10001b: group 17, what is left is -1 and bit 16 is set: the last group -> chr(65) = 'A'
#   [1000]            1000 = 31 * 32 + 8: group 8 + 32 = 40 -> chr(88) = 'X'; then 31: bit 16 set, left 0 != -1 -> 63 -> chr(111) = 'o';
#                     then 0 -> '0'
#   [5, 1, 2, 40]     the fourth is 40 - 1 = 39 = 32 + 7: group 7 + 32 -> chr(87) = 'W', then 1 -> '1'
HAND = (([0, 5], "05"), ([3, 2, 4, 2], "3240"), ([10, 20, 30, 5], ":d0n0A"), ([1000], "Xo0"), ([5, 1, 2, 40], "512W1"), ([], ""))


def test_string_form_by_hand():
    for counts, s in HAND:
        assert ops.rle_to_string(counts) == s and C.to_string(counts) == s, counts
        assert ops.rle_from_string(s) == counts and ops.rle_from_string(s.encode()) == counts


def test_string_form_round_trip():
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 40))
        top = (8, 40, 2 ** 10, 2 ** 15, 2 ** 16 + 3, 2 ** 20, 2 ** 31 - 1)[trial % 7]
        counts = [int(v) for v in rng.integers(0, top + 1, n)]
        if trial % 5 == 0:
            counts[n // 2] = top                                              # counts of 2^15 and more, differences of both signs
            counts[0] = 2 ** 15
        s = ops.rle_to_string(counts)
        assert s == C.to_string(counts) and all(48 <= ord(ch) < 112 for ch in s)
        assert ops.rle_from_string(s) == counts
    updown = [0, 2 ** 31 - 1, 2 ** 20, 0, 0, 2 ** 31 - 1, 1, 2 ** 15, 2 ** 15 - 1, 2 ** 15 + 1, 16, 15, 17, 31, 32, 33]
    assert ops.rle_from_string(ops.rle_to_string(updown)) == updown
    mask = np.random.default_rng(3).random((37, 50)) < 0.4
    code = R.encode(mask)
    assert ops.rle_from_string(ops.rle_to_string(code)) == code


def test_string_form_refusals():
    for bad in ("d", "05d", ":d0n", "o" * 14 + "0", "05 ", "0\x7f", "/", "p", "0é"):
        with pytest.raises(ValueError):
            ops.rle_from_string(bad)
    with pytest.raises(ValueError, match="ends inside count 2"):
        ops.rle_from_string("05d")
    with pytest.raises(ValueError, match="position 1"):
        ops.rle_from_string("0 5")
    for bad in (None, 5, [48, 53], b"\xff0"):
        with pytest.raises(ValueError):
            ops.rle_from_string(bad)
    for bad in ([1.0], [True], ["3"], [None]):
        with pytest.raises(ValueError):
            ops.rle_to_string(bad)


# ------------------------------------------------------------------------------------------------------ CPU: the records ----------
def _fixed_records_input():
    masks = [parse([".##.", ".#..", "##.."]), parse(["....", "....", "...."]), parse(["####", "####", "####"])]
    cap = 6
    stats = torch.tensor([R.stats(m) for m in masks], dtype=torch.int64)
    counts = torch.from_numpy(np.stack([R.counts_row(m, cap) for m in masks]))
    cat = torch.tensor([4, 0, 2], dtype=torch.int64)
    conf = torch.tensor([[0.75, 1.0, 0.75], [0.0, 0.5, 0.0], [0.5, 0.5, 1.0]], dtype=torch.float32)
    return masks, cat, stats, counts, conf


def test_default_records_are_what_they_were():
    _masks, cat, stats, counts, conf = _fixed_records_input()
    want = [{"image_id": 0, "category_id": 4, "bbox": [0, 0, 3, 3], "area": 5, "segmentation": {"size": [3, 4], "counts": [2, 5, 5]}},
            {"image_id": 1, "category_id": 0, "bbox": [0, 0, 0, 0], "area": 0, "segmentation": {"size": [3, 4], "counts": [12]}},
            {"image_id": 2, "category_id": 2, "bbox": [0, 0, 4, 3], "area": 12, "segmentation": {"size": [3, 4], "counts": [0, 12]}}]
    got = ops.instances_to_coco(cat, stats, counts, (3, 4))
    assert got == want and json.dumps(got) == json.dumps(want)
    assert ops.instances_to_coco(cat, stats, counts, (3, 4), compressed=False) == want
    scored = ops.instances_to_coco(cat, stats, counts, (3, 4), image_ids=["a", "b", "c"], conf=conf)
    assert [r["score"] for r in scored] == [0.75, 0.0, 0.5] and [r["image_id"] for r in scored] == ["a", "b", "c"]
    assert [{k: v for k, v in r.items() if k not in ("score", "image_id")} for r in scored] == \
        [{k: v for k, v in r.items() if k != "image_id"} for r in want]
    packed = ops.instances_to_coco(cat, stats, counts, (3, 4), compressed=True)
    assert [r["segmentation"]["counts"] for r in packed] == ["255", "<", "0<"]           # 12 -> chr(60)
    for a, b in zip(packed, want):
        assert {k: v for k, v in a.items() if k != "segmentation"} == {k: v for k, v in b.items() if k != "segmentation"}
        assert a["segmentation"]["size"] == [3, 4]


@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("scored", [False, True])
def test_records_round_trip(compressed, scored):
    _masks, cat, stats, counts, conf = _fixed_records_input()
    recs = ops.instances_to_coco(cat, stats, counts, (3, 4), image_ids=[7, "x", 9], conf=conf if scored else None, compressed=compressed)
    recs = json.loads(json.dumps(recs))
    ids, cat2, n_runs, counts2, sizes, scores = ops.coco_to_instances(recs, "cpu")
    assert ids == [7, "x", 9] and torch.equal(cat2, cat) and torch.equal(n_runs, stats[:, 5])
    assert counts2.dtype == torch.int32 and torch.equal(counts2, counts[:, :3])          # cap = the longest code
    assert sizes.tolist() == [[3, 4]] * 3 and sizes.dtype == torch.int64
    if scored:
        assert scores.dtype == torch.float32 and torch.equal(scores, conf[:, 0])
    else:
        assert scores is None
    wide = ops.coco_to_instances(recs, "cpu", max_runs=6)
    assert torch.equal(wide[3], counts) and torch.equal(wide[2], stats[:, 5])
    cut = ops.coco_to_instances(recs, "cpu", max_runs=2)
    assert cut[3].tolist() == [[2, 5], [12, 0], [0, 12]] and cut[2].tolist() == [3, 1, 2]      # the true lengths stay


def test_annotation_records_and_mixed_codes():
    gt = [{"id": 1, "image_id": 5, "category_id": 3, "iscrowd": 0, "bbox": [0, 0, 3, 3], "area": 5,
           "segmentation": {"size": [3, 4], "counts": "255"}},
          {"id": 2, "image_id": 6, "category_id": 1, "segmentation": {"size": [2, 2], "counts": [0, 0, 1, 3]}}]
    ids, cat, n_runs, counts, sizes, scores = ops.coco_to_instances(gt, "cpu")
    assert ids == [5, 6] and cat.tolist() == [3, 1] and n_runs.tolist() == [3, 4] and scores is None
    assert counts.tolist() == [[2, 5, 5, 0], [0, 0, 1, 3]] and sizes.tolist() == [[3, 4], [2, 2]]


def test_coco_to_instances_refusals():
    good = {"image_id": 1, "category_id": 2, "segmentation": {"size": [3, 4], "counts": [12]}}

    def but(**kw):
        r = json.loads(json.dumps(good))
        for k, v in kw.items():
            if v is None:
                del r[k]
            else:
                r[k] = v
        return r

    ops.coco_to_instances([good], "cpu")
    with pytest.raises(ValueError, match="polygon"):
        ops.coco_to_instances([good, but(segmentation=[[0.0, 0.0, 3.0, 0.0, 3.0, 2.0]])], "cpu")
    for key in ("image_id", "category_id", "segmentation"):
        with pytest.raises(ValueError, match=key):
            ops.coco_to_instances([but(**{key: None})], "cpu")
    with pytest.raises(ValueError, match="record 1.*'counts'"):
        ops.coco_to_instances([good, but(segmentation={"size": [3, 4]})], "cpu")
    with pytest.raises(ValueError, match="'size'"):
        ops.coco_to_instances([but(segmentation={"counts": [12]})], "cpu")
    for bad in ([2 ** 31], [-2 ** 31 - 1], [1.5], [True], ["3"]):
        with pytest.raises(ValueError, match="record 0.*count 0"):
            ops.coco_to_instances([but(segmentation={"size": [3, 4], "counts": bad})], "cpu")
    with pytest.raises(ValueError, match="record 1 .*image 1.*ends inside"):
        ops.coco_to_instances([good, but(segmentation={"size": [3, 4], "counts": "05d"})], "cpu")
    with pytest.raises(ValueError, match="score"):
        ops.coco_to_instances([but(score=0.5), good], "cpu")
    for bad in ([3], [3, 0], [3, 4.0], [True, 4], [3, 4, 1]):
        with pytest.raises(ValueError, match="size"):
            ops.coco_to_instances([but(segmentation={"size": bad, "counts": [12]})], "cpu")
    with pytest.raises(ValueError):
        ops.coco_to_instances([], "cpu")
    with pytest.raises(ValueError):
        ops.coco_to_instances([7], "cpu")
    with pytest.raises(ValueError):
        ops.coco_to_instances([but(category_id="cat")], "cpu")
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError):
            ops.coco_to_instances([good], "cpu", max_runs=bad)
    # a negative count is a count within int32: it is carried, and the decoder reports it (status 2)
    assert ops.coco_to_instances([but(segmentation={"size": [3, 4], "counts": [14, -2]})], "cpu")[3].tolist() == [[14, -2]]


class _Stub:
    training = False


def test_argument_checks_on_the_host():
    counts = torch.zeros(2, 5, dtype=torch.int32)
    n = torch.ones(2, dtype=torch.int64)
    for bad_counts in (counts.long(), counts.float(), counts[0], torch.zeros(0, 5, dtype=torch.int32), [[1]], None):
        with pytest.raises(ValueError):
            ops.rle_bits(bad_counts, n, (3, 4))
    for bad_n in (n.int(), n.float(), torch.ones(3, dtype=torch.int64), torch.ones(2, 1, dtype=torch.int64), torch.ones(2, 5, dtype=torch.int64),
                  [1, 1], None):
        with pytest.raises(ValueError):
            ops.rle_bits(counts, bad_n, (3, 4))
    for bad_size in ((3,), (3, 0), (0, 4), (3, 4, 5), (3.5, 4), (True, 4)):
        with pytest.raises(ValueError):
            ops.rle_bits(counts, n, bad_size)
    img, focus, c = torch.zeros(2, 3, 4, 4), torch.zeros(2, 2), torch.zeros(2, 1, dtype=torch.int64)
    ev = DeformSegmentationModule.evaluate_instances
    with pytest.raises(ValueError, match="seg_size"):
        ev(_Stub(), img, focus, (counts, n), c)                               # a code does not carry its size
    for label in ((counts,), (counts, n, n), (counts[:1], n[:1]), (counts.long(), n), (counts, n.int()), (counts[0], n)):
        with pytest.raises(ValueError):
            ev(_Stub(), img, focus, label, c, seg_size=(4, 4))
    for kw in (dict(boundary=0.0), dict(boundary=1), dict(component=3), dict(snap_px=2.0), dict(seg_size=(4,))):
        with pytest.raises(ValueError):
            ev(_Stub(), img, focus, (counts, n), c, **{"seg_size": (4, 4), **kw})


def test_score_coco_records_refusals():
    def rec(i, score=None, size=(3, 4), counts=(12,)):
        r = {"image_id": i, "category_id": 1, "segmentation": {"size": list(size), "counts": list(counts)}}
        if score is not None:
            r["score"] = score
        return r

    meter = T.InstanceAPMeter("cpu", 4)
    gt = [rec(1), rec(2)]
    for dt, g, what in (([rec(1, 0.5), rec(1, 0.4)], gt, "more than one"), ([rec(1, 0.5)], gt + [rec(2)], "more than one"),
                        ([rec(3, 0.5)], gt, "no ground truth"), ([rec(1)], gt, "no score"), ([rec(1, 0.5, size=(4, 3))], gt, "differs"),
                        ([{"category_id": 1}], gt, "image_id"), ([rec(1, 0.5)], [{"image_id": 1, "category_id": 1, "segmentation": [[0.0, 1.0]]}], "RLE")):
        with pytest.raises(ValueError, match=what):
            T.score_coco_records(dt, g, meter)
    for kw in (dict(boundary=0.0), dict(boundary=1), dict(boundary=True), dict(chunk=0), dict(chunk=1.5)):
        with pytest.raises(ValueError):
            T.score_coco_records([rec(1, 0.5)], gt, meter, **kw)
    assert meter.rows == []


def test_the_ctypes_table_binds_the_decoder():
    assert hip.SIGNATURES["fs_rle_bits"] == "pp" + "i" + "ppp" + "iiii" and hip.HOST_ONLY["fs_rle_bits_scratch_ints"] == ("l", "ii")
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "fovealseg.h")).read()
    assert "fs_rle_bits(" in header and "fs_rle_bits_scratch_ints(" in header
    assert [hip.query("fs_rle_bits_scratch_ints", B, cap) for B, cap in ((1, 1), (3, 7), (64, 8193))] == [3, 27, 64 * 8195]
    assert [hip.query("fs_rle_bits_scratch_ints", B, cap) for B, cap in ((0, 5), (-1, 5), (2, 0), (2, -3))] == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ GPU: C ABI ----
GUARD = 64
SENTINEL = -0x5A5A5A5B
POISON = -0x3C3C3C3D                                    # negative: read as a count it would make the code BAD; as a word it is no mask


class Guarded:
    """n elements (int32, or int64 = pairs of them) pre-filled with poison between two bands of GUARD sentinels.  The body is 16-byte
    aligned, or with off = 1 (int32 only) 4 bytes past that: aligned to 4 bytes and no more."""

    def __init__(self, n, dtype=torch.int32, off=0):
        words = n * (2 if dtype == torch.int64 else 1)
        assert off == 0 or dtype == torch.int32
        self.words = words
        self.whole = torch.full((words + 2 * GUARD + 4,), SENTINEL, device="cuda", dtype=torch.int32)
        self.lo = GUARD + off
        self.raw = self.whole[self.lo:self.lo + words]
        self.raw.fill_(POISON)
        self.body = self.raw.view(dtype) if dtype == torch.int64 else self.raw
        assert self.raw.data_ptr() % 16 == 4 * off

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def intact(self):
        return bool((self.whole[:self.lo] == SENTINEL).all()) and bool((self.whole[self.lo + self.words:] == SENTINEL).all())

    def untouched(self):
        return self.intact() and bool((self.raw == POISON).all())


def _rows(codes, cap):
    """The counts rows of a call: each code's first cap counts, poison behind them -- what lies at or past n_runs is never read."""
    rows = np.full((len(codes), cap), POISON, dtype=np.int64)
    for b, code in enumerate(codes):
        rows[b, :min(len(code), cap)] = code[:cap]
    return rows.astype(np.int32)


def _decode(codes, Hs, Ws, cap=None, n_runs=None, form="vec", off=0):
    """fs_rle_bits at the C ABI between guard bands, every output pre-filled with poison.  codes: one list of counts an image; n_runs
    defaults to their lengths.  form 'vec': n_runs as a (B,) vector, n_stride 1; 'stats': column 5 of a (B,6) tensor whose other columns
    hold poison, n_stride 6.  off = 1 puts counts, bits and scratch on addresses aligned to 4 bytes only.  Returns (words (B,Hs,P) uint32,
    info (B,4)) on the host, having checked them against rle_codec_ref.decode_info."""
    B = len(codes)
    cap = max(len(c) for c in codes) + 2 if cap is None else cap
    n_runs = [len(c) for c in codes] if n_runs is None else list(n_runs)
    rows = _rows(codes, cap)
    P = (Ws + 31) // 32
    counts = Guarded(B * cap, off=off)
    counts.raw.copy_(torch.from_numpy(rows.reshape(-1)).cuda())
    if form == "vec":
        n_dev = Guarded(B, torch.int64)
        n_dev.body.copy_(torch.tensor(n_runs, dtype=torch.int64).cuda())
        n_ptr, n_stride = n_dev.ptr, 1
    else:
        n_dev = Guarded(B * 6, torch.int64)
        n_dev.body.view(B, 6)[:, 5] = torch.tensor(n_runs, dtype=torch.int64).cuda()
        n_ptr, n_stride = n_dev.ptr + 5 * 8, 6
    n_before = n_dev.raw.clone()
    bits, info = Guarded(B * Hs * P, off=off), Guarded(B * 4, torch.int64)
    need = hip.query("fs_rle_bits_scratch_ints", B, cap)
    assert need == B * cap + 2 * B
    scr = Guarded(need, off=off)
    hip.call("fs_rle_bits", counts.ptr, n_ptr, n_stride, bits.ptr, info.ptr, scr.ptr, B, Hs, Ws, cap)
    torch.cuda.synchronize()
    assert counts.intact() and n_dev.intact() and bits.intact() and info.intact() and scr.intact()
    assert torch.equal(counts.raw.cpu(), torch.from_numpy(rows.reshape(-1))) and torch.equal(n_dev.raw, n_before)      # inputs are inputs
    words = bits.body.view(B, Hs, P).cpu().numpy()
    got_info = info.body.view(B, 4).cpu().tolist()
    for b in range(B):
        mask, want = C.decode_info(rows[b].tolist(), n_runs[b], Hs, Ws)
        assert got_info[b] == want, (b, got_info[b], want)
        assert np.array_equal(words[b], R.bits(mask)), b                     # the padding bits too: R.bits leaves them 0
        assert np.array_equal(R.unbits(words[b], Ws), mask)
    return words.view(np.uint32), got_info


SHAPES = [(1, 1), (1, 40), (40, 1), (5, 33), (7, 64), (9, 65), (70, 70), (65, 96), (130, 129)]


def _masks(Hs, Ws, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    lead = np.zeros((Hs, Ws), dtype=bool)
    lead[0, 0] = True                                    # a leading count of 0
    lead[Hs - 1, Ws - 1] = True
    named = {"empty": np.zeros((Hs, Ws), dtype=bool), "full": np.ones((Hs, Ws), dtype=bool), "lead": lead,
             "checker": (yy + xx) % 2 == 1, "checker_inv": (yy + xx) % 2 == 0}
    for density in (0.03, 0.5, 0.97):
        named[f"random{density}"] = rng.random((Hs, Ws)) < density
    return named, rng


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("Hs,Ws", SHAPES)
def test_rle_bits_shapes(Hs, Ws, off):
    named, rng = _masks(Hs, Ws, Hs * 1000 + Ws)
    codes = {k: R.encode(m) for k, m in named.items()}
    assert codes["empty"] == [Hs * Ws] and codes["full"] == [0, Hs * Ws] and codes["lead"][0] == 0
    if Hs % 2 == 1 or Ws == 1:                           # with an even Hs the runs join across the column ends
        assert len(codes["checker_inv"]) == Hs * Ws + 1  # the most runs a mask has: every pixel a run, behind a leading 0
    keys = list(codes)
    assert len(keys) == 8
    # three images a call, each with its own n_runs; the vector form and the stats form take turns
    for group, form in ((keys[0:3], "vec"), (keys[3:6], "stats"), (keys[5:8], "vec")):
        _decode([codes[k] for k in group], Hs, Ws, form=form, off=off)
    _decode([codes["checker_inv"]], Hs, Ws, cap=len(codes["checker_inv"]), form="stats", off=off)     # B = 1, the row exactly full
    loose = [C.with_zero_runs(codes[k], rng) for k in ("random0.03", "random0.5", "random0.97")]
    words, _ = _decode(loose, Hs, Ws, form="stats", off=off)
    for w, k in zip(words, ("random0.03", "random0.5", "random0.97")):
        assert np.array_equal(w.view(np.int32), R.bits(named[k]))
    _decode([C.with_zero_runs(codes[k], rng, k=9) for k in ("empty", "full", "checker")], Hs, Ws, off=off)


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", [(9, 65), (70, 70), (130, 129)])
def test_rle_bits_faulty_codes_beside_a_valid_image(Hs, Ws):
    """Malformed codes are ordinary inputs with defined results: zeros and a status; the valid images beside them are untouched by it."""
    N = Hs * Ws
    rng = np.random.default_rng(N)
    mask = rng.random((Hs, Ws)) < 0.4
    good = R.encode(mask)
    cap = len(good)
    neg = list(good)
    neg[3], neg[4] = -neg[3], neg[4] + 2 * neg[3]        # a negative count, the sum still N: BAD
    short, long_ = list(good), list(good)
    short[-1] -= 1
    long_[5] += N
    codes = [good, good + [0, 0, 0], neg, short, long_, good, [2 ** 31 - 1] * cap, good]
    n_runs = [cap, cap + 3, cap, cap, cap, 0, cap, -5]
    for form in ("vec", "stats"):
        words, info = _decode(codes, Hs, Ws, cap=cap, n_runs=n_runs, form=form)
        assert [r[0] for r in info] == [0, 1, 2, 3, 3, 2, 3, 2]
        assert np.array_equal(words[0].view(np.int32), R.bits(mask)) and not words[1:].any()
        assert info[6][3] == cap * (2 ** 31 - 1) and info[0][1] == int(mask.sum())                   # the total is an int64 sum
    # precedence: cut and negative -> CUT; negative and a wrong sum -> BAD
    bad = list(short)
    bad[2] = -7
    _w, info = _decode([bad, bad, good], Hs, Ws, cap=cap, n_runs=[cap + 1, cap, cap])
    assert [r[0] for r in info] == [1, 2, 0]
    # a valid image between two faulty ones, and the last image of the batch valid
    words, info = _decode([short, good, neg, good], Hs, Ws, cap=cap + 5)
    assert [r[0] for r in info] == [3, 0, 2, 0] and np.array_equal(words[1], words[3]) and words[1].any()


def _encode_dev(bits_dev, Hs, Ws, cap):
    B = bits_dev.shape[0]
    stats = torch.empty(B, 6, device="cuda", dtype=torch.int64)
    counts = torch.empty(B, cap, device="cuda", dtype=torch.int32)
    scr = torch.empty(hip.query("fs_mask_rle_scratch_ints", B, Hs, Ws), device="cuda", dtype=torch.int32)
    hip.call("fs_mask_rle", bits_dev.data_ptr(), stats.data_ptr(), counts.data_ptr(), scr.data_ptr(), B, Hs, Ws, cap)
    return stats, counts


def _decode_dev(counts, n_ptr, n_stride, B, Hs, Ws):
    cap = counts.shape[1]
    bits = torch.full((B, Hs, (Ws + 31) // 32), POISON, device="cuda", dtype=torch.int32)
    info = torch.full((B, 4), POISON, device="cuda", dtype=torch.int64)
    scr = torch.full((hip.query("fs_rle_bits_scratch_ints", B, cap),), POISON, device="cuda", dtype=torch.int32)
    hip.call("fs_rle_bits", counts.data_ptr(), n_ptr, n_stride, bits.data_ptr(), info.data_ptr(), scr.data_ptr(), B, Hs, Ws, cap)
    return bits, info


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws", [(1, 40), (9, 65), (65, 96), (130, 129)])
def test_device_round_trips(Hs, Ws):
    named, _rng = _masks(Hs, Ws, Hs + Ws)
    masks = np.stack(list(named.values()))
    B = len(masks)
    bits = torch.from_numpy(np.stack([R.bits(m) for m in masks])).cuda()
    cap = Hs * Ws + 1
    # bits -> code -> bits, the stats tensor handed over as it lies
    stats, counts = _encode_dev(bits, Hs, Ws, cap)
    back, info = _decode_dev(counts, stats.data_ptr() + 5 * 8, 6, B, Hs, Ws)
    assert torch.equal(back, bits) and torch.equal(info[:, 1], stats[:, 0]) and not info[:, 0].any()
    assert torch.equal(info[:, 2], stats[:, 5]) and (info[:, 3] == Hs * Ws).all()
    # code -> bits -> code, for canonical codes (the encoder writes zeros behind a code; so does this row)
    rows = torch.from_numpy(np.stack([R.counts_row(m, cap) for m in masks])).cuda()
    n = torch.tensor([len(R.encode(m)) for m in masks], dtype=torch.int64).cuda()
    words, _ = _decode_dev(rows, n.data_ptr(), 1, B, Hs, Ws)
    stats2, counts2 = _encode_dev(words, Hs, Ws, cap)
    assert torch.equal(counts2, rows) and torch.equal(stats2[:, 5], n) and torch.equal(stats2, stats)


@pytest.mark.gpu
def test_rejected_arguments_leave_the_outputs_alone():
    B, Hs, Ws, cap = 2, 9, 65, 12
    P = 3
    counts, n = Guarded(B * cap), Guarded(B, torch.int64)
    counts.raw.copy_(torch.tensor([Hs * Ws] + [0] * (cap - 1), dtype=torch.int32).repeat(B).cuda())
    n.body.fill_(1)
    bits, info, scr = Guarded(B * Hs * P), Guarded(B * 4, torch.int64), Guarded(hip.query("fs_rle_bits_scratch_ints", B, cap))

    def rejected(*args):
        with pytest.raises(hip.HipLibraryError, match="argument rejected"):
            hip.call("fs_rle_bits", *args)

    good = [counts.ptr, n.ptr, 1, bits.ptr, info.ptr, scr.ptr]
    for i in (0, 1, 3, 4, 5):
        a = list(good)
        a[i] = None
        rejected(*a, B, Hs, Ws, cap)
    for stride in (0, -1):
        a = list(good)
        a[2] = stride
        rejected(*a, B, Hs, Ws, cap)
    for dims in ((B, Hs, Ws, 0), (B, Hs, Ws, -1), (0, Hs, Ws, cap), (-1, Hs, Ws, cap), (B, 0, Ws, cap), (B, Hs, 0, cap), (B, -9, Ws, cap),
                 (B, 65536, 32768, cap),                 # Hs * Ws = 2^31
                 (B, 46341, 46341, cap),                 # just above 2^31
                 (4, 32768, 32768, cap)):                # 2^32 bit slots
        rejected(*good, *dims)
    torch.cuda.synchronize()
    assert bits.untouched() and info.untouched() and scr.untouched()
    hip.call("fs_rle_bits", *good, B, Hs, Ws, cap)       # and the same pointers are taken with the sizes they were made for
    torch.cuda.synchronize()
    assert bits.intact() and info.intact() and scr.intact() and not bits.body.any()
    assert info.body.view(B, 4).tolist() == [[0, 0, 1, Hs * Ws]] * B


@pytest.mark.gpu
def test_ops_rle_bits():
    Hs, Ws = 9, 65
    rng = np.random.default_rng(5)
    masks = rng.random((3, Hs, Ws)) < 0.3
    dev = torch.from_numpy(masks).cuda()
    stats, counts = ops.mask_rle(dev, max_runs=Hs * Ws + 1)
    bits = ops.mask_bits(dev)
    for n_runs in (stats, stats[:, 5].contiguous(), stats[:, 5]):
        got, info = ops.rle_bits(counts, n_runs, (Hs, Ws), check=True)
        assert torch.equal(got, bits) and got.dtype == torch.int32 and info.tolist() == [[0, int(m.sum()), int(s[5]), Hs * Ws]
                                                                                        for m, s in zip(masks, stats.tolist())]
    # the record goes back into the library's own operations
    assert torch.equal(ops.mask_rle(got, Ws, max_runs=Hs * Ws + 1)[1], counts)
    short = counts.clone()
    short[1, 0] += 1
    got, info = ops.rle_bits(short, stats, (Hs, Ws))
    assert info[:, 0].tolist() == [0, 3, 0] and not got[1].any() and torch.equal(got[0], bits[0]) and torch.equal(got[2], bits[2])
    with pytest.raises(ValueError, match="image 1: the counts do not sum"):
        ops.rle_bits(short, stats, (Hs, Ws), check=True)
    with pytest.raises(ValueError, match="image 0: the code was cut"):
        ops.rle_bits(counts[:, :4].contiguous(), stats, (Hs, Ws), check=True)
    neg = counts.clone()
    neg[2, 1] = -1
    with pytest.raises(ValueError, match="image 2: n_runs is below 1 or a count is negative"):
        ops.rle_bits(neg, stats, (Hs, Ws), check=True)
    with pytest.raises(ValueError):
        ops.rle_bits(counts, stats.cpu(), (Hs, Ws))       # n_runs on another device


# ------------------------------------------------------------------------------------------------- GPU: the composed calls ---------
def _tp():
    import test_predict as TP
    return TP


class _foreground_head:
    """test_component.py's trick: a large background logit lets the mask plane decide, so the head marks a non-trivial foreground."""

    def __init__(self, module):
        self.bias = module.decoder.cls_net.fc.bias
        self.keep = self.bias.detach().clone()

    def __enter__(self):
        with torch.no_grad():
            self.bias[-1] += 1000.0

    def __exit__(self, *exc):
        with torch.no_grad():
            self.bias.copy_(self.keep)


@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


SIZE = 128


def _unpack(bits):
    return np.stack([R.unbits(w, SIZE) for w in bits.cpu().numpy()])


@pytest.mark.gpu
@pytest.mark.parametrize("component", [None, 8])
def test_the_record_decodes_to_its_bits(component):
    module, _ = _tp()._module("hrnet")
    X, Fp, _Y, _cls = T.synthetic_batch(2, SIZE, SIZE, seed=11, device="cuda")
    with _foreground_head(module):
        out = module.predict_instances(X, Fp, return_bits=True, component=component)
    _cat, stats, counts, bits = out[:4]
    got, info = ops.rle_bits(counts, stats, (SIZE, SIZE), check=True)
    assert torch.equal(got, bits) and torch.equal(info[:, 1], stats[:, 0]) and torch.equal(info[:, 2], stats[:, 5])
    print(f"areas {stats[:, 0].tolist()}, runs {stats[:, 5].tolist()}")
    assert 0 < int(stats[:, 0].max()) < SIZE * SIZE and int(stats[:, 5].max()) > 3


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    top = torch.cuda.max_memory_allocated() - base
    del out
    return top


@pytest.mark.gpu
@pytest.mark.parametrize("component", [None, 8])
def test_evaluate_instances_with_a_run_length_label(component, deterministic):
    module, _ = _tp()._module("hrnet")
    X, Fp, Y, cls = T.synthetic_batch(2, SIZE, SIZE, seed=11, device="cuda")
    with _foreground_head(module):
        seen = _unpack(module.predict_instances(X, Fp, return_bits=True)[3])
        # the label: the synthetic disc joined with the head's own foreground moved by (2, 1) pixels (at this size a blob three pixels wide)
        Y = ((Y != 0) | torch.from_numpy(np.roll(seen, (2, 1), (1, 2))).cuda()[:, None]).float()
        stats, counts = ops.mask_rle(Y[:, 0] != 0, max_runs=SIZE * SIZE + 1)
        counts = counts[:, :int(stats[:, 5].max())].contiguous()             # a row as long as the longest code, as coco_to_instances makes it
        dense = module.evaluate_instances(X, Fp, Y, cls, component=component)
        for label in ((counts, stats), (counts, stats[:, 5].contiguous()), [counts, stats]):
            got = module.evaluate_instances(X, Fp, label, cls, seg_size=(SIZE, SIZE), component=component)
            assert len(got) == len(dense) == (6 if component else 5)
            for a, b in zip(got, dense):
                assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                          b.view(torch.int32) if b.dtype == torch.float32 else b)
        print(f"pair {dense[-1].tolist()}, label runs {stats[:, 5].tolist()}")
        assert int(dense[-1][:, 1].min()) > 0 and int(dense[-1][:, 2].min()) > 0      # neither the record nor the label is empty
        # a label whose code is not valid scores as an empty label, without a host read
        broken = counts.clone()
        broken[1, 0] += 1
        got = module.evaluate_instances(X, Fp, (broken, stats), cls, seg_size=(SIZE, SIZE), component=component)
        assert torch.equal(got[-1][0], dense[-1][0]) and got[-1][1].tolist() == [0, int(dense[-1][1, 1]), 0, 0, int(dense[-1][1, 4]), 0]
        # memory: the call's peak is predict_instances' plus the decoder's, and the decoder's is below a byte a pixel -- the dense
        # label alone is four (fp32), or eight as the data pipeline makes it
        run = lambda: module.evaluate_instances(X, Fp, (counts, stats), cls, seg_size=(SIZE, SIZE), component=component)    # noqa: E731
        pred = lambda: module.predict_instances(X, Fp, return_bits=True, return_score=True, component=component)             # noqa: E731
        run(), pred()
        p_pred, p_dec, p_eval = _peak(pred), _peak(lambda: ops.rle_bits(counts, stats, (SIZE, SIZE))), _peak(run)
    print(f"peak bytes: predict_instances {p_pred}, rle_bits {p_dec}, evaluate_instances(rle) {p_eval}; a uint8 label {2 * SIZE * SIZE}")
    assert p_dec < 2 * SIZE * SIZE and p_eval <= p_pred + p_dec


@pytest.mark.gpu
def test_score_coco_records_is_the_meter_of_the_evaluated_batches(deterministic):
    module, _ = _tp()._module("hrnet")
    K = module.cfg.DATASET.num_class
    live, stored = T.InstanceAPMeter("cuda", K), T.InstanceAPMeter("cuda", K)
    dt, gt = [], []
    with _foreground_head(module):
        for i, seed in enumerate((3, 5, 8)):
            X, Fp, _, _ = T.synthetic_batch(2, SIZE, SIZE, seed=seed, device="cuda")
            cat, _, _, bits, _ = module.predict_instances(X, Fp, return_bits=True, component=8)
            label = torch.from_numpy(np.roll(_unpack(bits), seed % 3, 2)).cuda()          # the record's blob moved by 0 .. 2 pixels
            cls = cat.clone()[:, None]
            cls[1] = (cls[1] + 1) % (K - 1)
            out = T.evaluate_instances_step(module, (X, Fp, label[:, None].float(), cls), live, component=8)
            ids = [f"img{2 * i}", 2 * i + 1]
            dt += ops.instances_to_coco(out[0], out[1], out[2], (SIZE, SIZE), image_ids=ids, conf=out[3], compressed=True)
            lstats, lcounts = ops.mask_rle(label, max_runs=SIZE * SIZE + 1)
            gt += ops.instances_to_coco(cls[:, 0], lstats, lcounts, (SIZE, SIZE), image_ids=ids, compressed=True)
    assert all(isinstance(r["segmentation"]["counts"], str) for r in dt + gt)
    dt, gt = json.loads(json.dumps(dt)), json.loads(json.dumps(gt))
    assert T.score_coco_records(dt, gt, stored, chunk=4) == 6
    assert len(stored.rows) == 2 and all(r.is_cuda for r in stored.rows)                  # chunks of 4 and 2
    want = live.result()
    got = stored.result()
    assert set(got) == set(want) and all(got[k] == v or (v != v and got[k] != got[k]) for k, v in want.items()), (got, want)
    assert got["n_images"] == 6 and got["mIoU"] > 0.2 and got["AP"] > 0.0
    assert torch.equal(torch.cat(stored.rows), torch.cat(live.rows))
    # an image with ground truth and no result enters as an empty record
    fewer = T.InstanceAPMeter("cuda", K)
    assert T.score_coco_records(dt[:2] + dt[3:], gt, fewer) == 6
    rows = torch.cat(fewer.rows).cpu()
    assert rows[2].tolist() == [-1, gt[2]["category_id"], 0, 0, 0, int(torch.cat(live.rows)[2, 5]), 0, 0, int(torch.cat(live.rows)[2, 8]), 0]
    assert torch.equal(rows[[0, 1, 3, 4, 5]], torch.cat(live.rows).cpu()[[0, 1, 3, 4, 5]])
    res = fewer.result()
    assert res["n_images"] == 6 and res["n_records"] == got["n_records"] - int(torch.cat(live.rows)[2, 2] > 0)
    print(f"stored records: {got}")
