"""CPU test: the host-side answers of the forward / bwd-data conv dispatch against a recorded table (no launch, no GPU)."""
import os
import sys

import numpy as np

from fovealseg import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_conv_dispatch as rec      # noqa: E402  (the grid is defined once, beside the recorder)


def test_conv_dispatch_matches_recorded_table(golden):
    """fs_conv2d_workspace_bytes, _kernel_choice, _pack_persistent, _stats_slabs, _bwd_data_bnsum_slabs, _fwd_affine_act_ok and
    _fwd_residual_ok over the grid of tools/record_conv_dispatch.py, in all three precision modes, reproduce
    tests/golden/conv_dispatch_table.npz exactly: every row, every column.  The table was recorded from the library as it stood before
    kernel selection moved into plan_conv (csrc/conv.hip), so any difference is a problem whose route, slab layout or "fused extra
    available" answer changed.  (Shipped library only: a -DFS_EXPERIMENTS build with a kernel switched off answers differently.)"""
    want = golden("conv_dispatch_table")["table"]
    assert want.dtype == np.int64 and want.shape[1] == len(rec.COLUMNS)

    # the stored table is not hollow: every family and every fused extra occurs often
    col = {name: want[:, i] for i, name in enumerate(rec.COLUMNS)}
    ids, counts = np.unique(col["kernel_choice"], return_counts=True)
    assert ids.tolist() == list(range(9)) and counts.min() >= 500, dict(zip(ids.tolist(), counts.tolist()))
    for name in ("pack_persistent", "fwd_affine_act_ok", "fwd_residual_ok"):
        assert set(np.unique(col[name]).tolist()) == {0, 1} and int(col[name].sum()) >= 1000, name
    assert int((col["bwd_data_bnsum_slabs"] > 0).sum()) >= 1000

    lib = hip.load()
    saved = lib.fs_get_conv_precision()
    got = rec.table(lib)
    assert lib.fs_get_conv_precision() == saved
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (f"{bad.size} rows differ; first: row {bad[0]}, columns {rec.COLUMNS}, "
                           f"got {got[bad[0]].tolist()}, recorded {want[bad[0]].tolist()}")
