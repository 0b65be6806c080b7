"""Writes tests/golden/g_color_encode.npz: what the reference's utils.colorEncode(labelmap, colors, mode='RGB') (utils.py:207-221) returns
for a seeded 8 x 12 label map that includes -1, with the 150 colours of data/color150.mat (the palette eval.py:26 loads), which is
stored beside it.  The map is made from a seed here; nothing is read but the reference's function and its palette.

Run in the build container only:  python tests/golden/make_color_encode_golden.py"""
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
    return ref_utils.colorEncode


def main():
    from scipy.io import loadmat
    colors = np.ascontiguousarray(loadmat(os.path.join(rh.REF, "data", "color150.mat"))["colors"])       # loadmat gives column-major
    assert colors.shape == (150, 3) and colors.dtype == np.uint8
    rng = np.random.default_rng(34)
    labels = rng.integers(-1, 150, (8, 12)).astype(np.int64)
    labels[0, 0], labels[3, 5], labels[7, 11], labels[2, 2] = -1, -1, 149, 0
    rgb = reference_function()(labels, colors)
    assert rgb.shape == (8, 12, 3) and rgb.dtype == np.uint8
    path = os.path.join(HERE, "g_color_encode.npz")
    np.savez_compressed(path, labels=labels, colors=colors, rgb=rgb, source=np.array("utils.colorEncode(labels, colors, mode='RGB')"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
