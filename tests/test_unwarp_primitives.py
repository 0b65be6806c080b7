"""The un-warp primitives of csrc/unwarp.hip at the C ABI, on hand-built inputs: the corner rules include/fovealseg.h promises for
fs_inverse_grid (the largest index wins a pixel claimed twice; a point outside the frame claims nothing; an image nobody claims
is all holes), fs_fill_nearest (ties go to the smallest row, then column; an image without a claim is left alone) and the
index maps of fs_inverse_index_maps.  Every output and scratch is an `Out` of tests/kernel_testing.py (guards, fill); everything
is exact.  Expected values: a sequential restatement in the test (claims_ref, nearest_ref: brute force over all claimed pixels),
and oracle/fovealseg_oracle.inverse_grid_ref wherever every point lies inside the frame (that function indexes with numpy and
cannot take a point outside).  Finite coordinates only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fovealseg  # noqa: E402
import fovealseg_oracle as O  # noqa: E402
from kernel_testing import Out, dev, exact  # noqa: E402

hip = fovealseg.hip
HipError = fovealseg.hip.HipLibraryError


# ================================================================================================
# fs_inverse_grid, fs_inverse_index_maps
# ================================================================================================
def index_maps(grid, Hs, Ws):
    """models/models.py:644-645 in fp32: u = int((gx + 1) / 2 * (Ws - 1)), truncated toward zero"""
    g = grid.float()
    return (((g[..., 0] + 1) / 2) * (Ws - 1)).int(), (((g[..., 1] + 1) / 2) * (Hs - 1)).int()


def claims_ref(grid, Hs, Ws):
    """owner (B, Hs, Ws) and grid_inv (B, Hs, Ws, 2) of a sequential pass over the grid points in index order: a later point
    overwrites an earlier one, a point outside the frame is skipped"""
    B, h, w, _ = grid.shape
    u, v = index_maps(grid, Hs, Ws)
    u, v = u.reshape(B, -1).tolist(), v.reshape(B, -1).tolist()
    owner = torch.full((B, Hs, Ws), -1, dtype=torch.int32)
    for b in range(B):
        for i in range(h * w):
            if 0 <= u[b][i] < Ws and 0 <= v[b][i] < Hs:
                owner[b, v[b][i], u[b][i]] = i
    xi, yi = (owner % w).float(), torch.div(owner, w, rounding_mode="floor").float()
    inv = torch.stack([xi / w * 2 - 1, yi / h * 2 - 1], dim=-1)
    return owner, torch.where((owner >= 0)[..., None], inv, torch.zeros_like(inv))


def run_inverse_grid(grid, Hs, Ws):
    B, h, w, _ = grid.shape
    owner, inv = Out(B * Hs * Ws, torch.int32), Out(B * Hs * Ws * 2)
    gd = dev(grid)
    hip.call("fs_inverse_grid", hip.ptr(gd), owner.ptr, inv.ptr, B, h, w, Hs, Ws)
    return owner.get(complete=False).reshape(B, Hs, Ws), inv.get().reshape(B, Hs, Ws, 2)      # -9999, the int fill, is no owner value


def check_inverse_grid(grid, Hs, Ws, inside):
    grid = grid.float().double()
    owner, inv = run_inverse_grid(grid, Hs, Ws)
    want_owner, want_inv = claims_ref(grid, Hs, Ws)
    assert not bool((owner == -9999).any())
    exact("inverse_grid", "owner", owner, want_owner)
    exact("inverse_grid", "grid_inv", inv, want_inv)
    assert not bool(torch.signbit(inv[want_owner < 0]).any())          # holes are +0
    if inside:
        ref = O.inverse_grid_ref(grid.float(), Hs, Ws)
        assert torch.equal(torch.isnan(ref[..., 0]), owner < 0)
        exact("inverse_grid", "grid_inv against the oracle", inv, torch.nan_to_num(ref, nan=0.0))
    return owner


def coord(p, n):
    """the coordinate whose index map is pixel p of n (the pixel's centre in index space, so truncation cannot flip it)"""
    return (p + 0.5) / (n - 1) * 2 - 1 if n > 1 else 0.0


def test_inverse_grid_largest_index_wins():
    Hs, Ws, h, w = 6, 9, 3, 4
    grid = torch.zeros(1, h, w, 2, dtype=torch.float64)
    target = [(2, 3)] * 5 + [(0, 0)] + [(2, 3)] * 2 + [(4, 7), (4, 7), (5, 8), (1, 1)]      # (row, column) of point i; both channels equal claims
    for i, (y, x) in enumerate(target):
        grid[0, i // w, i % w] = torch.tensor([coord(x, Ws) if x < Ws - 1 else 1.0, coord(y, Hs) if y < Hs - 1 else 1.0])
    owner = check_inverse_grid(grid, Hs, Ws, inside=True)
    assert int(owner[0, 2, 3]) == 7 and int(owner[0, 4, 7]) == 9 and int(owner[0, 0, 0]) == 5 and int(owner[0, 5, 8]) == 10 and int(owner[0, 1, 1]) == 11
    assert int((owner >= 0).sum()) == 5


def test_inverse_grid_edges_of_the_frame():
    """exactly +-1 are the first and last pixel; truncation toward zero keeps a coordinate a little below -1 on pixel 0 and one a
    little above 1 on the last pixel (as the reference's .int()); from a whole pixel outside on nothing is claimed"""
    Hs, Ws = 9, 9
    nxt = float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)))
    xs = [-1.0, 1.0, -nxt, nxt, -1.1, 1.1, -1.25, 1.25, -1.5, 3.0, 0.0, -0.999]
    grid = torch.zeros(1, 2, len(xs), 2, dtype=torch.float64)
    for i, gx in enumerate(xs):
        grid[0, 0, i] = torch.tensor([gx, coord(4, Hs)])          # x on the edge, y inside: row 4
        grid[0, 1, i] = torch.tensor([coord(6, Ws), gx])          # y on the edge, x inside: column 6
    owner = check_inverse_grid(grid, Hs, Ws, inside=False)
    u, _ = index_maps(grid, Hs, Ws)
    assert u[0, 0].tolist() == [0, 8, 0, 8, 0, 8, -1, 9, -2, 16, 4, 0]
    n = len(xs)
    assert int(owner[0, 4, 0]) == 11 and int(owner[0, 4, 8]) == 5 and int(owner[0, 4, 4]) == 10      # the last claimant of each
    assert int(owner[0, 0, 6]) == n + 11 and int(owner[0, 8, 6]) == n + 5 and int(owner[0, 4, 6]) == n + 10
    assert int((owner >= 0).sum()) == 6
    check_inverse_grid(grid[:, :, :6], Hs, Ws, inside=True)      # the in-range part against the oracle as well


@pytest.mark.parametrize("Hs,Ws", [(1, 1), (1, 5), (5, 1)])
def test_inverse_grid_single_row_or_column(Hs, Ws):
    gen = torch.Generator().manual_seed(Hs * 10 + Ws)
    grid = torch.rand(2, 3, 3, 2, generator=gen, dtype=torch.float64) * 2 - 1
    owner = check_inverse_grid(grid, Hs, Ws, inside=True)
    if Hs == Ws == 1:
        assert owner.reshape(-1).tolist() == [8, 8]


def test_inverse_grid_image_without_a_claim():
    Hs, Ws = 7, 9
    gen = torch.Generator().manual_seed(5)
    grid = torch.rand(2, 4, 5, 2, generator=gen, dtype=torch.float64) * 2 - 1
    grid[1] = 1.5 + torch.rand(4, 5, 2, generator=gen, dtype=torch.float64)          # every point of image 1 lies outside
    owner, inv = run_inverse_grid(grid.float().double(), Hs, Ws)
    assert bool((owner[1] == -1).all()) and bool((inv[1] == 0).all()) and not bool(torch.signbit(inv[1]).any())
    assert bool((owner[0] >= 0).any())
    check_inverse_grid(grid, Hs, Ws, inside=False)


def test_inverse_grid_rejections():
    grid = dev(torch.zeros(1, 2, 2, 2, dtype=torch.float64))
    for args in ((None, True, True, 1, 2, 2, 4, 4), (grid, False, True, 1, 2, 2, 4, 4), (grid, True, False, 1, 2, 2, 4, 4),
                 (grid, True, True, 0, 2, 2, 4, 4), (grid, True, True, 1, 0, 2, 4, 4), (grid, True, True, 1, 2, 2, 0, 4), (grid, True, True, 1, 2, 2, 4, 0)):
        owner, inv = Out(16, torch.int32), Out(32)
        with pytest.raises(HipError, match="rejected"):
            hip.call("fs_inverse_grid", hip.ptr(args[0]), owner.ptr if args[1] else None, inv.ptr if args[2] else None, *args[3:])
        assert owner.untouched() and inv.untouched()


def test_inverse_index_maps_truncate_toward_zero():
    H, W = 9, 17
    nxt = float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)))
    vals = [-1.0, 1.0, -nxt, nxt, -1.1, 1.1, -1.25, 1.25, -1.5, 3.0, 0.0, -0.999, 0.999, 0.5, -0.5]
    gen = torch.Generator().manual_seed(3)
    grid = torch.tensor([[a, b] for a in vals for b in vals], dtype=torch.float64)
    grid = torch.cat([grid, torch.rand(37, 2, generator=gen, dtype=torch.float64) * 2.4 - 1.2]).float().double()
    n = grid.shape[0]
    u, v = Out(n, torch.int64), Out(n, torch.int64)
    gd = dev(grid)
    hip.call("fs_inverse_index_maps", hip.ptr(gd), u.ptr, v.ptr, n, H, W)
    wu, wv = index_maps(grid, H, W)
    exact("inverse_index_maps", "u", u.get(complete=False), wu.long())
    exact("inverse_index_maps", "v", v.get(complete=False), wv.long())
    assert int(wu.min()) < 0 and int(wu.max()) >= W and int(wv.min()) < 0 and int(wv.max()) >= H
    for args in ((None, True, True, n), (gd, False, True, n), (gd, True, False, n), (gd, True, True, 0)):
        u, v = Out(n, torch.int64), Out(n, torch.int64)
        with pytest.raises(HipError, match="rejected"):
            hip.call("fs_inverse_index_maps", hip.ptr(args[0]), u.ptr if args[1] else None, v.ptr if args[2] else None, args[3], H, W)
        assert u.untouched() and v.untouched()


# ================================================================================================
# fs_fill_nearest
# ================================================================================================
def nearest_ref(vals, owner):
    """every hole takes the values of the claimed pixel that minimises (squared distance, row, column); an image without a
    claim is returned as given.  Brute force over all claimed pixels."""
    B, C, Hs, Ws = vals.shape
    out = vals.clone()
    for b in range(B):
        ys, xs = torch.where(owner[b] >= 0)                # row-major: ascending (row, column)
        hy, hx = torch.where(owner[b] < 0)
        if len(ys) == 0 or len(hy) == 0:
            continue
        key = ((hy[:, None] - ys[None, :]) ** 2 + (hx[:, None] - xs[None, :]) ** 2) * (Hs * Ws) + (ys * Ws + xs)[None, :]
        j = key.argmin(dim=1)
        out[b][:, hy, hx] = vals[b][:, ys[j], xs[j]]
    return out


def run_fill(vals, owner):
    B, C, Hs, Ws = vals.shape
    v, scratch = Out(vals.numel(), body=vals), Out(2 * B * Hs * Ws, torch.int32)
    od = owner.to(torch.int32).contiguous().to("cuda")
    hip.call("fs_fill_nearest", v.ptr, hip.ptr(od), scratch.ptr, B, C, Hs, Ws)
    scratch.get()                                          # guards; both index maps are written for every pixel
    return v.get(complete=False).reshape(vals.shape)


def marked(B, C, Hs, Ws):
    """distinct values everywhere: a hole that is not filled, or filled from the wrong pixel, shows"""
    return (torch.arange(B * C * Hs * Ws, dtype=torch.float32).reshape(B, C, Hs, Ws) + 0.5).double()


def check_fill(owner, C):
    B, Hs, Ws = owner.shape
    vals = marked(B, C, Hs, Ws)
    got = run_fill(vals, owner)
    exact("fill_nearest", f"{B}x{C}x{Hs}x{Ws}", got, nearest_ref(vals, owner))
    return got, vals


def test_fill_nearest_image_without_a_claim_and_single_claim():
    owner = torch.full((3, 5, 7), -1)
    owner[1, 3, 2] = 4                                     # image 0 and 2: no claim at all; image 1: one claimed pixel
    got, vals = check_fill(owner, 3)
    assert torch.equal(got[0], vals[0].float()) and torch.equal(got[2], vals[2].float())
    assert bool((got[1] == vals[1, :, 3, 2].float()[:, None, None]).all())


TIES = {
    "left-right": [(3, 1), (3, 5)],
    "up-down": [(1, 3), (5, 3)],
    "diagonal": [(1, 1), (1, 5), (5, 1), (5, 5)],
    "cross": [(3, 1), (3, 5), (1, 3), (5, 3)],
    "knight": [(2, 5), (4, 5), (5, 2), (5, 4), (1, 2), (2, 1)],          # distance^2 5 from the centre in different rows and columns
    "ring": [(0, 3), (3, 0), (3, 6), (6, 3), (1, 1), (5, 5)],
}


@pytest.mark.parametrize("name", list(TIES))
def test_fill_nearest_ties_go_to_the_smallest_row_then_column(name):
    """7 x 7 images, the claimed pixels symmetric about the centre (3, 3): the centre (and every other pixel on an axis of
    symmetry) is equidistant from several claimed pixels"""
    pts = TIES[name]
    owner = torch.full((1, 7, 7), -1)
    for k, (y, x) in enumerate(pts):
        owner[0, y, x] = k
    got, vals = check_fill(owner, 2)
    d2 = [(y - 3) ** 2 + (x - 3) ** 2 for y, x in pts]
    tied = sorted(p for p, d in zip(pts, d2) if d == min(d2))
    assert len(tied) >= 2
    assert torch.equal(got[0, :, 3, 3], vals[0, :, tied[0][0], tied[0][1]].float())


@pytest.mark.parametrize("Hs,Ws,C", [(5, 1, 1), (4, 255, 4), (3, 257, 5), (3, 513, 6), (6, 256, 2)])
def test_fill_nearest_widths_and_channel_counts(Hs, Ws, C):
    """around the 256 segments of the row pass (one column per thread up to 256, then two, then three) and the 4-way unrolled
    copy; sparse claims, one row and one image without any, the first and last column claimed somewhere"""
    gen = torch.Generator().manual_seed(Hs * 1000 + Ws + C)
    B = 3
    owner = torch.where(torch.rand(B, Hs, Ws, generator=gen) < 0.04, torch.randint(0, 99, (B, Hs, Ws), generator=gen), torch.full((B, Hs, Ws), -1))
    owner[0, 0, 0], owner[0, Hs - 1, Ws - 1] = 0, 5
    owner[0, Hs // 2] = -1
    owner[2] = -1
    got, vals = check_fill(owner, C)
    assert torch.equal(got[2], vals[2].float())


def test_fill_nearest_rejections():
    owner = torch.zeros(1, 4, 4, dtype=torch.int32, device="cuda")
    for args in ((False, owner, True, 1, 2, 4, 4), (True, None, True, 1, 2, 4, 4), (True, owner, False, 1, 2, 4, 4), (True, owner, True, 0, 2, 4, 4),
                 (True, owner, True, 1, 0, 4, 4), (True, owner, True, 1, 2, 0, 4), (True, owner, True, 1, 2, 4, 0), (True, owner, True, 1, 2, 4, 16385)):
        v, scratch = Out(32), Out(32, torch.int32)
        with pytest.raises(HipError, match="rejected"):
            hip.call("fs_fill_nearest", v.ptr if args[0] else None, hip.ptr(args[1]), scratch.ptr if args[2] else None, *args[3:])
        assert v.untouched() and scratch.untouched()
