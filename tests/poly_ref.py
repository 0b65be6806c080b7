"""fs_poly_bits' definition in plain Python (include/fovealseg.h): COCO / LVIS polygon lists as a mask.  UNPINNED: the reference makes
its labels with np.round, a clip onto the frame and skimage.draw.polygon (b2_preprocess_lvis.py:282-297); skimage is not at hand, so
the rule below is this library's restatement -- interior by the even-odd crossing number plus every lattice point of the outline -- and
tests/test_poly_bits.py holds this file to hand-derived answers and to matplotlib's point-in-path test away from the outline first.
It is not pycocotools' frPoly.

    vertex   (clip(rne(y), 0, H-1), clip(rne(x), 0, W-1)); rne = round half to even
    ring     the closed chain of n >= 1 vertices, edges (v_i, v_(i+1) mod n)
    pixel    set by a ring iff (a) it lies on an edge, end points included, or (b) the number of edges, oriented so that y0 < y1, with
             y0 <= y < y1 and (x - x0)(y1 - y0) < (y - y0)(x1 - x0) is odd
    mask     the OR of the rings
"""
import numpy as np

OK, BAD_OFFSETS = 0, 1
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def clip(v, top):
    return 0 if v < 0 else (top if v > top else v)


def clamped(ring, H, W):
    """ring: (y, x) integer vertices, any values -> the vertices on the frame."""
    return [(clip(int(y), H - 1), clip(int(x), W - 1)) for y, x in ring]


def on_edge(y, x, a, b):
    (y0, x0), (y1, x1) = a, b
    return (x - x0) * (y1 - y0) == (y - y0) * (x1 - x0) and min(y0, y1) <= y <= max(y0, y1) and min(x0, x1) <= x <= max(x0, x1)


def crosses(y, x, a, b):
    (y0, x0), (y1, x1) = (a, b) if a[0] < b[0] else (b, a)
    return y0 <= y < y1 and (x - x0) * (y1 - y0) < (y - y0) * (x1 - x0)


def ring_mask(ring, H, W):
    """One ring, (a) and (b) as written, pixel by pixel and edge by edge."""
    v = clamped(ring, H, W)
    n = len(v)
    assert n >= 1
    edges = [(v[i], v[(i + 1) % n]) for i in range(n)]
    m = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            m[y, x] = any(on_edge(y, x, a, b) for a, b in edges) or sum(crosses(y, x, a, b) for a, b in edges) % 2 == 1
    return m


def poly_mask(rings, H, W):
    """rings: a list of rings, each a list of (y, x) integer vertices (rounded, not clipped) -> (H, W) bool, the OR of the rings."""
    m = np.zeros((H, W), dtype=bool)
    for ring in rings:
        m |= ring_mask(ring, H, W)
    return m


def boundary_mask(rings, H, W):
    """The pixels rule (a) alone sets: the lattice points of the outlines."""
    m = np.zeros((H, W), dtype=bool)
    for ring in rings:
        v = clamped(ring, H, W)
        edges = [(v[i], v[(i + 1) % len(v)]) for i in range(len(v))]
        for y in range(H):
            for x in range(W):
                m[y, x] |= any(on_edge(y, x, a, b) for a, b in edges)
    return m


def ring_mask_rows(ring, H, W):
    """ring_mask for frames too large for the double loop: the same two rules, an edge at a time over the rows it spans, numpy along the
    row.  test_poly_bits.py holds it to ring_mask on every small case before it uses it on a large one."""
    v = clamped(ring, H, W)
    n = len(v)
    xs = np.arange(W, dtype=np.int64)
    odd = np.zeros((H, W), dtype=bool)
    edge = np.zeros((H, W), dtype=bool)
    for i in range(n):
        a, b = v[i], v[(i + 1) % n]
        (y0, x0), (y1, x1) = (a, b) if a[0] <= b[0] else (b, a)
        if y0 == y1:
            edge[y0, min(x0, x1):max(x0, x1) + 1] = True
            continue
        ys = np.arange(y0, y1 + 1, dtype=np.int64)[:, None]
        lhs, rhs = (xs[None, :] - x0) * (y1 - y0), (ys - y0) * (x1 - x0)
        edge[y0:y1 + 1] |= (lhs == rhs) & (xs[None, :] >= min(x0, x1)) & (xs[None, :] <= max(x0, x1))
        odd[y0:y1] ^= (lhs < rhs)[:-1]
    return odd | edge


def poly_mask_rows(rings, H, W):
    m = np.zeros((H, W), dtype=bool)
    for ring in rings:
        m |= ring_mask_rows(ring, H, W)
    return m


def rne(v):
    """Round half to even on a double, by its definition (not numpy's): the nearer integer, the even one of two equally near."""
    lo = int(np.floor(v))
    d = v - lo                                            # exact for |v| < 2^52
    if d < 0.5:
        return lo
    if d > 0.5:
        return lo + 1
    return lo if lo % 2 == 0 else lo + 1


def coco_rings(polygons):
    """One image's COCO polygon list [[x0, y0, x1, y1, ...], ...] -> rings of rounded (y, x) vertices."""
    return [[(rne(float(p[2 * i + 1])), rne(float(p[2 * i]))) for i in range(len(p) // 2)] for p in polygons]


def pack(batch):
    """batch: a list of images, each a list of rings of (y, x) -> (verts (V,2), ring_off (R+1), img_ring (B+1)) int32 arrays."""
    verts, ring_off, img_ring = [], [0], [0]
    for rings in batch:
        for ring in rings:
            verts += [[int(y), int(x)] for y, x in ring]
            ring_off.append(len(verts))
        img_ring.append(len(ring_off) - 1)
    return (np.array(verts, dtype=np.int32).reshape(-1, 2), np.array(ring_off, dtype=np.int32), np.array(img_ring, dtype=np.int32))


def poly_info(verts, ring_off, img_ring, b, H, W, fast=False):
    """Image b of a packed batch as fs_poly_bits defines it, malformed offsets included -> (mask, [status, area, n_rings, n_vertices]).
    Offsets outside their tables' ranges or decreasing over the image's rings give status 1, an empty mask and zeros."""
    R, V = len(ring_off) - 1, len(verts)
    ra, rb = int(img_ring[b]), int(img_ring[b + 1])
    bad = not (0 <= ra <= rb <= R)
    if not bad:
        for r in range(ra, rb):
            a, c = int(ring_off[r]), int(ring_off[r + 1])
            bad = bad or not (0 <= a <= c <= V)
    if bad:
        return np.zeros((H, W), dtype=bool), [BAD_OFFSETS, 0, 0, 0]
    rings = [[(int(y), int(x)) for y, x in verts[int(ring_off[r]):int(ring_off[r + 1])]] for r in range(ra, rb)]
    rings = [r for r in rings if r]
    m = (poly_mask_rows if fast else poly_mask)(rings, H, W)
    return m, [OK, int(m.sum()), rb - ra, int(ring_off[rb]) - int(ring_off[ra]) if rb > ra else 0]
