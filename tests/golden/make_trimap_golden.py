"""Writes tests/golden/g18_trimap.npz: what the reference's trimap boundary accuracy (eval.py:41-67) gives on ten small label /
prediction pairs -- its per-width accuracies and the band masks of the very PIL / scipy calls it makes (ImageFilter.FIND_EDGES on the
min/max-normalised label, ndimage.binary_dilation(iterations=2**i)).

eval.trim_accuracy itself is tried first, through ref_harness's stubs with the working directory in the reference; its module pulls in
the whole evaluation script (a .mat file, datasets, pandas ...) and may not import, in which case the same two library calls are made
here.  The fixture's `source` field says which of the two produced the accuracies.  The band masks always come from the direct calls
(trim_accuracy does not return them).  Two cases have a constant label, where the reference divides 0 by 0 before the filter: they are
stored as PIL sees a constant image (255 for all background: the ring; 0 for all foreground: nothing) and flagged `constant`.

Needs PIL and scipy; run in the build container only:  python tests/golden/make_trimap_golden.py"""
import os
import sys
import warnings

import numpy as np
from PIL import Image, ImageFilter
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_harness as rh  # noqa: E402

D = 5


def library_bands(label, constant_grey=0):
    """The reference's edge image and its D + 1 dilations for one (H,W) int label; a constant label is the grey level given."""
    lo, hi = int(label.min()), int(label.max())
    if lo == hi:
        grey = np.full(label.shape, constant_grey, np.uint8)
    else:
        grey = np.array((label - lo) / (hi - lo) * 255).astype(np.uint8)
    edges = np.array(Image.fromarray(grey, "L").filter(ImageFilter.FIND_EDGES).convert("L"))
    edges[edges > 0] = 1
    return np.stack([ndimage.binary_dilation(edges, iterations=2 ** i) for i in range(D + 1)])


def library_acc(pred, label, bands):
    return np.array([float((b * (pred == label)).sum()) / (b.sum() + 1e-10) for b in bands])


def reference_trim_accuracy():
    """eval.trim_accuracy, or None with the reason it could not be imported."""
    try:
        rh.load_reference()
        os.chdir(rh.REF)
        for name in ("pandas", "tqdm"):
            try:
                __import__(name)
            except ImportError:
                rh._stub(name, tqdm=None, trange=None)
        import eval as ref_eval
        return ref_eval.trim_accuracy, "eval.trim_accuracy"
    except BaseException as e:          # the script's import chain: anything from ImportError to a missing data file
        return None, f"direct PIL FIND_EDGES + scipy binary_dilation calls (import eval failed: {type(e).__name__}: {e})"


def blocky(rng, H, W, p=0.4, cell=8):
    c = rng.random(((H + cell - 1) // cell, (W + cell - 1) // cell)) < p
    t = np.repeat(np.repeat(c, cell, 0), cell, 1)[:H, :W].astype(np.int64)
    if t.min() == t.max():
        t[0, 0] = 1 - t[0, 0]
    return t


def cases():
    rng = np.random.default_rng(18)
    out = []
    t = np.zeros((1, 9), np.int64); t[0, 3:5] = 1
    out.append(("row_1x9", t))
    out.append(("rows_2x50", blocky(rng, 2, 50, cell=5)))
    t = np.zeros((3, 3), np.int64); t[1, 1] = 1
    out.append(("dot_3x3", t))
    t = np.zeros((16, 20), np.int64); t[5:11, 4:15] = 1
    out.append(("rect_16x20", t))
    out.append(("blocky_37x61", blocky(rng, 37, 61)))
    out.append(("blocky_130x97", blocky(rng, 130, 97)))
    import torch  # noqa: F401
    from fovealseg import train as T
    _, _, Y, _ = T.synthetic_batch(1, 64, 64, seed=5, device="cpu")
    out.append(("disc_64x64", Y[0, 0].numpy().astype(np.int64)))
    out.append(("all_background_12x15", np.zeros((12, 15), np.int64)))
    out.append(("all_foreground_12x15", np.ones((12, 15), np.int64)))
    t = np.zeros((40, 33), np.int64); t[0:14, 20:33] = 1; t[30:40, 0:6] = 1
    out.append(("touching_40x33", t))
    return out, rng


def main():
    trim_accuracy, source = reference_trim_accuracy()
    os.chdir(ROOT)
    cs, rng = cases()
    K = 51
    data = {"names": np.array([n for n, _ in cs]), "D": np.int64(D), "K": np.int64(K), "source": np.array(source)}
    for n, t in cs:
        cl = int(rng.integers(0, K - 1))
        gt = t * cl + (1 - t) * (K - 1)
        # a prediction that is right in most places, smeared near the boundary and wrong in class here and there
        shift = np.roll(t, (1, 2), (0, 1))
        pred = np.where(rng.random(t.shape) < 0.8, shift * cl + (1 - shift) * (K - 1), rng.integers(0, K, t.shape))
        constant = gt.min() == gt.max()
        bands = library_bands(gt, constant_grey=255 if t.flat[0] == 0 else 0)
        acc = library_acc(pred, gt, bands)
        if trim_accuracy is not None and not constant:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                cfg = rh._CfgNode(VAL=rh._CfgNode(trimap_visual_check=False))
                got = trim_accuracy(pred, gt, D, cfg)
            acc = np.array([got[f"trim_width_{2 ** i}_acc"] for i in range(D + 1)])
        data[f"{n}/t"] = t.astype(np.uint8)
        data[f"{n}/cls_label"] = np.int64(cl)
        data[f"{n}/pred"] = pred.astype(np.int16)
        data[f"{n}/bands"] = np.packbits(bands, axis=-1)
        data[f"{n}/acc"] = acc
        data[f"{n}/constant"] = np.bool_(constant)
    path = os.path.join(HERE, "g18_trimap.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", source)


if __name__ == "__main__":
    main()
