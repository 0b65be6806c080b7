#!/usr/bin/env python3
"""Record what the five scratch-size queries of the un-warp / evaluation entry points answer over a grid of shapes (CPU only: the
queries launch nothing and the library loads without a GPU).

Usage: python tools/record_unwarp_scratch.py OUT.json      (FS_HIP_LIB chooses the library: the fixture holds the answers of the
                                                            commit BEFORE the scratch layout moved into unwarp_plan, csrc/unwarp.hip)

tests/test_unwarp_scratch.py imports shapes() and answers() from here and compares the library beside it with
tests/golden/unwarp_scratch_ints.json, value by value.  The file maps each query to the list of its answers in shapes() order."""
import itertools
import json
import os
import sys

QUERIES = ("fs_unwarp_labels_scratch_ints", "fs_unwarp_accuracy_scratch_ints", "fs_trimap_bands_scratch_ints", "fs_unwarp_trimap_scratch_ints",
           "fs_unwarp_class_areas_scratch_ints")
BATCHES = (0, 1, 2, 64)
CLASSES = (2, 51, 150)
GRIDS = (1, 4, 80)                                   # h = w
OUTPUTS = ((1, 1), (8, 8), (9, 7), (64, 64), (1024, 1024), (1023, 1021))


def shapes():
    """(B, K, h, w, Hs, Ws) of every grid point."""
    for B, K, g, (Hs, Ws) in itertools.product(BATCHES, CLASSES, GRIDS, OUTPUTS):
        yield B, K, g, g, Hs, Ws


def arguments(query, shape):
    B, K, h, w, Hs, Ws = shape
    if query == "fs_trimap_bands_scratch_ints":
        return B, Hs, Ws
    return (B, K, h, w, Hs, Ws) if query == "fs_unwarp_class_areas_scratch_ints" else (B, h, w, Hs, Ws)


def answers(lib):
    """query -> [its answer for every shape of shapes(), in order] from `lib` (fovealseg.hip.load())."""
    return {q: [int(getattr(lib, q)(*arguments(q, s))) for s in shapes()] for q in QUERIES}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fovealseg import hip
    got = answers(hip.load())
    with open(sys.argv[1], "w") as f:
        json.dump(got, f, separators=(",", ":"))
        f.write("\n")
    print({q: (len(v), max(v)) for q, v in got.items()}, os.path.getsize(sys.argv[1]), "bytes")
