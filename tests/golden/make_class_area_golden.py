"""Writes tests/golden/g19_class_areas.npz: what the reference's utils.intersectionAndUnion(pred, gt, K, ignore_index=-2)
(utils.py:289-317; -2 is DATASET.ignore_index's "none") returns on ten small (prediction, ground truth) pairs, with the per-image IoU
(VAL.report_per_img_iou, eval.py:252) and the dataset IoU / Dice of each K by the reference's expressions (eval.py:313-315).

The pairs cover K = 2, 3, 51, 150 and 1024, constant labels, a prediction that never hits and a foreground class at K - 1 (which
merges into the background row).  Every map is made from a seed here; nothing is read but the reference's function.

Run in the build container only:  python tests/golden/make_class_area_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402


def reference_function():
    sys.dont_write_bytecode = True
    if rh.REF not in sys.path:
        sys.path.insert(0, rh.REF)
    import utils as ref_utils
    return ref_utils.intersectionAndUnion


def blocky(rng, H, W, p=0.4, cell=4):
    c = rng.random(((H + cell - 1) // cell, (W + cell - 1) // cell)) < p
    return np.repeat(np.repeat(c, cell, 0), cell, 1)[:H, :W].astype(np.int64)


def cases():
    """(name, K, cls_label, t (H,W) 0/1, pred (H,W))."""
    rng = np.random.default_rng(19)
    out = []

    def noisy(t, cl, K, keep=0.8):
        shift = np.roll(t, (1, 2), (0, 1))
        return np.where(rng.random(t.shape) < keep, shift * cl + (1 - shift) * (K - 1), rng.integers(0, K, t.shape))
    for name, K, cl, shape in (("k2_9x14", 2, 0, (9, 14)), ("k3_16x20", 3, 1, (16, 20)), ("k51_37x61", 51, 17, (37, 61)),
                               ("k51_40x33", 51, 49, (40, 33)), ("k150_31x40", 150, 88, (31, 40)), ("k1024_64x48", 1024, 511, (64, 48))):
        t = blocky(rng, *shape)
        out.append((name, K, cl, t, noisy(t, cl, K)))
    t = np.zeros((12, 15), np.int64)
    out.append(("k51_all_background", 51, 3, t, noisy(t, 3, 51)))
    t = np.ones((12, 15), np.int64)
    out.append(("k51_all_foreground", 51, 3, t, noisy(t, 3, 51)))
    t = blocky(rng, 20, 24)
    gt = t * 7 + (1 - t) * 50
    out.append(("k51_never_hits", 51, 7, t, np.where(gt == 7, 50, np.where(rng.random(t.shape) < 0.5, 7, 23))))
    t = blocky(rng, 18, 22)
    out.append(("k51_label_is_background", 51, 50, t, noisy(t, 50, 51)))
    return out


def main():
    fn = reference_function()
    cs = cases()
    data = {"names": np.array([c[0] for c in cs]), "source": np.array("utils.intersectionAndUnion(pred, gt, K, ignore_index=-2)")}
    sums = {}
    for name, K, cl, t, pred in cs:
        gt = t * cl + (1 - t) * (K - 1)
        inter, union, lab = fn(pred, gt, K, ignore_index=-2)
        assert inter.shape == (K,) and union.shape == (K,) and lab.shape == (K,)
        data[f"{name}/K"] = np.int64(K)
        data[f"{name}/cls_label"] = np.int64(cl)
        data[f"{name}/t"] = t.astype(np.uint8)
        data[f"{name}/pred"] = pred.astype(np.int16)
        data[f"{name}/intersection"] = inter.astype(np.int64)
        data[f"{name}/union"] = union.astype(np.int64)
        data[f"{name}/area_lab"] = lab.astype(np.int64)
        data[f"{name}/img_iou"] = inter / (union + 1e-10)                       # eval.py:252
        s = sums.setdefault(K, [np.zeros(K), np.zeros(K)])                      # AverageMeter.sum: float sums of the arrays
        s[0] = s[0] + inter
        s[1] = s[1] + union
    for K, (si, su) in sums.items():
        data[f"dataset/{K}/iou"] = si / (su + 1e-10)                            # eval.py:313
        data[f"dataset/{K}/dice"] = (2 * si) / (su + si + 1e-10)                # eval.py:315
    path = os.path.join(HERE, "g19_class_areas.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
