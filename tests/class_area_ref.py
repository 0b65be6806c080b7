"""The per-class areas of the reference's evaluation summary (utils.intersectionAndUnion, utils.py:289-317; eval.py:218-257,313-322)
restated in numpy, for tests/test_class_areas.py.

The reference shifts both maps by one, zeroes the prediction where the label is unlabelled, and takes three np.histogram(bins=K,
range=(1, K)) -- of prediction * (prediction == label), of the prediction and of the label.  On integer classes that binning is the
identity on 1 .. K and drops everything else, so with ignore_index = -2 ("none") the three histograms are counts by equality:

    inter[k] = #(pred == k and gt == k)     pred[k] = #(pred == k)     lab[k] = #(gt == k)         k = 0 .. K-1

for labels >= 0.  (A negative label becomes <= 0 after the shift and is the reference's "unlabelled": it also takes its pixel out of
pred.  The data path makes none -- only a cls_label below 0 would -- and fs_unwarp_class_areas defines every row by equality alone,
so the restatement does too; the fixture has no negative label.)  The reference returns (inter, union = pred + lab - inter, lab); fs_unwarp_class_areas stores (inter, pred, lab).
tests/golden/g19_class_areas.npz holds what utils.intersectionAndUnion itself gives (tests/golden/make_class_area_golden.py)."""
import numpy as np


def _hist(v, K):
    v = np.asarray(v).reshape(-1)
    v = v[(v >= 0) & (v < K)]
    return np.bincount(v, minlength=K).astype(np.int64)


def areas(pred, gt, K):
    """(K, 3) int64 = (inter, pred, lab) per class for one pair of integer maps of any (equal) shape."""
    pred, gt = np.asarray(pred).astype(np.int64).reshape(-1), np.asarray(gt).astype(np.int64).reshape(-1)
    assert pred.shape == gt.shape
    return np.stack([_hist(pred[pred == gt], K), _hist(pred, K), _hist(gt, K)], 1)


def areas_batch(pred, gt, K):
    """(B, K, 3) for (B, ...) maps."""
    return np.stack([areas(p, g, K) for p, g in zip(pred, gt)])


def intersection_and_union(pred, gt, K):
    """The reference's return value: (area_intersection, area_union, area_lab)."""
    a = areas(pred, gt, K)
    return a[:, 0], a[:, 1] + a[:, 2] - a[:, 0], a[:, 2]


def compose_gt(t, cl, K):
    """models/models.py:968: t * cls_label + (1 - t) * (K - 1) for an integer 0 / 1 map t (B, ...) and cls_label (B,)."""
    t = np.asarray(t).astype(np.int64)
    cl = np.asarray(cl).astype(np.int64).reshape((-1,) + (1,) * (t.ndim - 1))
    return t * cl + (1 - t) * (K - 1)


def scores(a):
    """(..., K, 3) areas -> (iou, dice) fp64, the reference's expressions (eval.py:252, 313-315)."""
    a = np.asarray(a).astype(np.float64)
    inter, union = a[..., 0], a[..., 1] + a[..., 2] - a[..., 0]
    return inter / (union + 1e-10), 2 * inter / (union + inter + 1e-10)
