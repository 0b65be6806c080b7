"""Writes tests/golden/g20_hd95.npz: the Hausdorff percentile between two 2-D masks by the published definition the reference's
utils.hd95 (utils.py:25-101) was copied from, made with scipy's binary_erosion and distance_transform_edt and np.percentile called
directly on the 2-D arrays.  Per case: the two masks, the sorted integer d^2 of either direction (round(dt^2), exact), the border
sizes, and the percentile at q = 1, 50, 95, 100 (nan where a border is empty).

utils.hd95 itself passes both masks through preprocessing_accuracy, which flattens them, so that its erosion and distance transform
run along a 1-D array; what it returns on the same pair is stored as `utils_hd95` where it runs (nan where it raises), to record the
divergence.  It is not a target of any test.

Run in the build container only:  python tests/golden/make_hd95_golden.py"""
import os
import sys
import warnings

import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

QS = (1, 50, 95, 100)


def reference_function():
    sys.dont_write_bytecode = True
    if not hasattr(np, "bool"):
        np.bool = np.bool_                           # the reference was written for a numpy that still had the alias
    if rh.REF not in sys.path:
        sys.path.insert(0, rh.REF)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import utils as ref_utils
    return ref_utils.hd95


def blocky(rng, H, W, p=0.4, cell=8):
    c = rng.random(((H + cell - 1) // cell, (W + cell - 1) // cell)) < p
    return np.repeat(np.repeat(c, cell, 0), cell, 1)[:H, :W]


def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    return m


def disc(H, W, cy, cx, r):
    ii, jj = np.mgrid[:H, :W]
    return (ii - cy) ** 2 + (jj - cx) ** 2 <= r * r


def cases():
    """(name, a (H,W) bool: the prediction, b (H,W) bool: the label)."""
    rng = np.random.default_rng(20)
    out = []
    a, b = np.zeros((1, 9), bool), np.zeros((1, 9), bool)
    a[0, 1:4], b[0, [5, 6, 8]] = True, True
    out.append(("row_1x9", a, b))
    out.append(("col_9x1", a.T.copy(), b.T.copy()))
    a = rect(3, 3, 1, 2, 1, 2)
    out.append(("dot_3x3", a, a.copy()))
    out.append(("two_dots", rect(20, 31, 0, 1, 0, 1), rect(20, 31, 19, 20, 30, 31)))
    out.append(("rect_16x20", rect(16, 20, 3, 10, 4, 13), rect(16, 20, 5, 12, 7, 16)))
    for H, W in ((37, 61), (130, 97)):
        a = blocky(rng, H, W)
        out.append((f"blocky_{H}x{W}", a, a ^ (rng.random((H, W)) < 0.05)))
    out.append(("touching_40x33", rect(40, 33, 0, 15, 0, 14), rect(40, 33, 5, 20, 4, 18) | rect(40, 33, 36, 40, 28, 33)))
    a, b = np.zeros((2, 300), bool), np.zeros((2, 300), bool)
    a[0, 2:13], b[1, 288:298] = True, True            # 11 + 10 border pixels: 95 * (n - 1) is a multiple of 100
    out.append(("thin_2x300", a, b))
    out.append(("disc_64x64", disc(64, 64, 30, 28, 17), disc(64, 64, 34, 35, 15)))
    out.append(("full_12x15", np.ones((12, 15), bool), rect(12, 15, 3, 8, 4, 11)))
    out.append(("empty_pred", np.zeros((6, 7), bool), rect(6, 7, 1, 4, 2, 5)))
    out.append(("empty_label", rect(6, 7, 1, 4, 2, 5), np.zeros((6, 7), bool)))
    out.append(("both_empty", np.zeros((6, 7), bool), np.zeros((6, 7), bool)))
    return out


def surface_d2(src, dst):
    """The two scipy calls of the definition on 2-D arrays: d^2 from every border pixel of src to the nearest one of dst, sorted."""
    cross = generate_binary_structure(2, 1)
    sb = src ^ binary_erosion(src, structure=cross, iterations=1)
    db = dst ^ binary_erosion(dst, structure=cross, iterations=1)
    if not db.any():
        return np.zeros(0, np.int64), int(sb.sum())
    dt = distance_transform_edt(~db)
    d2 = np.rint(dt[sb] ** 2).astype(np.int64)
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), dt[sb])                  # the integers are exact
    return np.sort(d2), int(sb.sum())


def main():
    ref = reference_function()
    cs = cases()
    data = {"names": np.array([c[0] for c in cs]), "qs": np.array(QS, np.int64),
            "source": np.array("scipy binary_erosion(cross) + distance_transform_edt on 2-D arrays, np.percentile")}
    mult = {True: 0, False: 0}
    for name, a, b in cs:
        d_ab, na = surface_d2(a, b)
        d_ba, nb = surface_d2(b, a)
        data[f"{name}/a"], data[f"{name}/b"] = a.astype(np.uint8), b.astype(np.uint8)
        data[f"{name}/d2_pred_to_label"], data[f"{name}/d2_label_to_pred"] = d_ab, d_ba
        data[f"{name}/n_pred"], data[f"{name}/n_label"] = np.int64(na), np.int64(nb)
        if na and nb:
            pooled = np.sqrt(np.concatenate([d_ab, d_ba]).astype(np.float64))
            pct = np.array([np.percentile(pooled, q) for q in QS])
            mult[(95 * (na + nb - 1)) % 100 == 0] += 1
        else:
            pct = np.full(len(QS), np.nan)
        data[f"{name}/percentile"] = pct
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                theirs = float(ref(a.astype(np.float64), b.astype(np.float64)))
        except Exception:                             # an empty mask raises RuntimeError; other shapes may not run at all
            theirs = float("nan")
        data[f"{name}/utils_hd95"] = np.float64(theirs)
        print(f"{name:16s} n_pred {na:5d} n_label {nb:5d} hd95 {pct[2]:10.4f}  utils.hd95 {theirs:10.4f}")
    assert mult[True] >= 1 and mult[False] >= 1, mult  # q (n - 1) both a multiple of 100 and not
    path = os.path.join(HERE, "g20_hd95.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
