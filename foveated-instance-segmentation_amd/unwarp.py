"""The full-resolution un-warp (csrc/unwarp.hip) and what is counted in it: class maps, the instance record, the accuracies, trimap
bands, class areas and the Hausdorff distance, with the plain-torch scores made from their counters.  Stateless, no autograd.
"""
import torch

from . import hip
from .masks import _component_args, _focus_arg, _max_runs

__all__ = [
    "inverse_index_maps", "inverse_grid", "unwarp_nearest", "unwarp_labels", "head_fg_q", "unwarp_instances", "unwarp_count",
    "unwarp_accuracy", "trimap_bands", "unwarp_trimap", "trimap_from_counts", "unwarp_class_areas", "class_scores_from_areas",
    "surface_hd", "hd_from_stats", "image_accuracies_from_counts", "accuracies_from_counts",
]


def inverse_index_maps(grid, H, W):
    n = grid.numel() // 2
    u = torch.empty(grid.shape[:-1], device=grid.device, dtype=torch.int64)
    v = torch.empty_like(u)
    hip.call("fs_inverse_index_maps", hip.ptr(grid), hip.ptr(u), hip.ptr(v), n, H, W)
    return u, v


def inverse_grid(grid, Hs, Ws):
    """models/models.py:639-655: (owner (B,Hs,Ws) int32 with -1 in holes, grid_inv (B,Hs,Ws,2) with 0 in holes)."""
    B, h, w, _ = grid.shape
    owner = torch.empty(B, Hs, Ws, device=grid.device, dtype=torch.int32)
    inv = torch.empty(B, Hs, Ws, 2, device=grid.device, dtype=torch.float32)
    hip.call("fs_inverse_grid", hip.ptr(grid.contiguous()), hip.ptr(owner), hip.ptr(inv), B, h, w, Hs, Ws)
    return owner, inv


def unwarp_nearest(pred, grid, Hs, Ws):
    """Full-resolution prediction from the foveated one (no autograd): pred (B,C,h,w) is sampled through the inverse grid
    (F.grid_sample(pred, grid_inv), models/models.py:933) and the never-claimed pixels take their nearest claimed
    neighbour (rev_deform_interp='nearest').  Returns (pred_full (B,C,Hs,Ws), hole mask (B,Hs,Ws) bool)."""
    B, C, h, w = pred.shape
    owner, inv = inverse_grid(grid, Hs, Ws)
    out = torch.empty(B, C, Hs, Ws, device=pred.device, dtype=torch.float32)
    hip.call("fs_grid_sample_fwd", hip.ptr(pred.contiguous()), hip.ptr(inv), hip.ptr(out), B, C, h, w, Hs, Ws, 0)
    scratch = torch.empty(2 * B * Hs * Ws, device=pred.device, dtype=torch.int32)
    hip.call("fs_fill_nearest", hip.ptr(out), hip.ptr(owner), hip.ptr(scratch), B, C, Hs, Ws)
    return out, owner < 0


def unwarp_labels(cls, m, grid, Hs, Ws):
    """Full-resolution class map of the C1 head (no autograd): bit for bit
    `unwarp_nearest(PredAssemble.apply(cls, m), grid, Hs, Ws)[0].argmax(1)`, without the (B,K,Hs,Ws) prediction -- the argmax is
    taken once per grid point and gathered through the owner map (fs_unwarp_labels).  cls (B,K), m (B,h,w) at the grid's
    resolution, grid (B,h,w,2).  Returns (labels (B,Hs,Ws) int64, hole mask (B,Hs,Ws) bool)."""
    B, K = cls.shape
    _, h, w, _ = grid.shape
    if tuple(m.shape) != (B, h, w):
        raise ValueError(f"m {tuple(m.shape)} must be (B, h, w) = {(B, h, w)}: the mask at the grid's resolution")
    labels = torch.empty(B, Hs, Ws, device=cls.device, dtype=torch.int64)
    hole = torch.empty(B, Hs, Ws, device=cls.device, dtype=torch.bool)
    scratch = torch.empty(hip.query("fs_unwarp_labels_scratch_ints", B, h, w, Hs, Ws), device=cls.device, dtype=torch.int32)
    hip.call("fs_unwarp_labels", hip.ptr(cls.contiguous()), hip.ptr(m.contiguous()), hip.ptr(grid.contiguous()), hip.ptr(labels),
             hip.ptr(hole), hip.ptr(scratch), B, K, h, w, Hs, Ws)
    return labels, hole


def head_fg_q(cls, m):
    """The C1 head's foreground probability per grid point as an integer table (fs_head_fg_q; no autograd; unpinned: the reference
    has no counterpart).  cls (B,K), m (B,h,w).  Returns q (B, h*w+1) int32 = rint(P * 2^24): P is the softmax mass of the classes
    below K-1 among the K fp32 values `unwarp_nearest(PredAssemble(cls, m), ...)` carries from grid point p (entry h*w: from the sample at
    (0,0), which feeds an image without a claimed pixel), evaluated in fp64 with the maximum subtracted; 0 where P is NaN."""
    B, K = cls.shape
    if m.dim() != 3 or m.shape[0] != B:
        raise ValueError(f"m {tuple(m.shape)} must be (B, h, w) with B = {B}")
    h, w = int(m.shape[1]), int(m.shape[2])
    q = torch.empty(B, h * w + 1, device=cls.device, dtype=torch.int32)
    hip.call("fs_head_fg_q", hip.ptr(cls.contiguous()), hip.ptr(m.contiguous()), hip.ptr(q), B, K, h, w)
    return q


def unwarp_instances(cls, m, grid, Hs, Ws, max_runs=None, return_bits=False, score=False, component=None, focus=None, snap_px=None):
    """The gazed instance of the C1 head as a record instead of a class map (fs_unwarp_instances; no autograd).  Arguments and checks
    are unwarp_labels'.  The mask is `unwarp_labels(cls, m, grid, Hs, Ws)[0] != K - 1` bit for bit; no (B,Hs,Ws) tensor wider than its
    bit words is allocated.  Returns (cat, stats, counts[, bits]): cat (B,) int64 = torch.argmax(cls[:, :K-1], 1), the head's
    classification (first maximum, NaN maximal); stats (B,6) int64 and counts (B,max_runs) int32 are mask_rle's of the mask; bits
    (B,Hs,ceil(Ws/32)) int32 are mask_bits' of it.  cat is the label of every set pixel except where the bilinear sample of the constant
    class planes ties two classes by rounding or has no in-bounds weight (a grid point on the outer border).  max_runs: any int >= 1,
    default 8 * Ws + 1 -- room for a mask every column of which crosses its outline at most eight times, 32 KB per 1024-wide image;
    n_runs = stats[:, 5] > max_runs tells a cut code.  instances_to_coco makes the result records.

    score=True (fs_unwarp_instances_scored; unpinned) appends conf (B,3) fp32 = (score, cls_prob, mask_prob) and qsum (B,) int64 behind
    everything else: qsum is the sum of head_fg_q(cls, m)[b, feeding point] over the set pixels, added in the same gather; mask_prob =
    qsum / (area * 2^24), 0 for an empty mask; cls_prob = softmax(cls[b, :K-1])[cat[b]] in fp64, NaN where that row holds a NaN; score
    = their product, the mean probability of class cat over the mask.  The other results are the unscored call's bit for bit.

    component = 4 or 8 (fs_unwarp_instances_component; unpinned) keeps only the connected component of that mask under the gaze: focus
    (B,2) normalised (row, col) and snap_px as mask_component's.  stats, counts, bits, qsum, mask_prob and score then describe the
    component (the empty mask's record where there is none); cat and cls_prob are unchanged.  comp (B,4) int64 = (seed_y, seed_x, d2,
    area_all) is appended as the last element, behind conf / qsum where present.  Nothing is read on the host in between."""
    B, K = cls.shape
    _, h, w, _ = grid.shape
    if tuple(m.shape) != (B, h, w):
        raise ValueError(f"m {tuple(m.shape)} must be (B, h, w) = {(B, h, w)}: the mask at the grid's resolution")
    if component is None and (focus is not None or snap_px is not None):
        raise ValueError("focus and snap_px go with component = 4 or 8")
    Hs, Ws = int(Hs), int(Ws)
    cap = _max_runs(max_runs, Ws)
    dev = cls.device
    comp = component is not None
    if comp:
        conn, snap2 = _component_args(component, snap_px)
        if focus is None:
            raise ValueError("component needs focus (B, 2): the gaze that picks it")
        f = _focus_arg(focus, B, dev)
    cat = torch.empty(B, device=dev, dtype=torch.int64)
    stats = torch.empty(B, 6, device=dev, dtype=torch.int64)
    counts = torch.empty(B, cap, device=dev, dtype=torch.int32)
    bits = torch.empty(B, Hs, (Ws + 31) // 32, device=dev, dtype=torch.int32) if return_bits else None
    conf = torch.empty(B, 3, device=dev, dtype=torch.float32) if score else None
    qsum = torch.empty(B, device=dev, dtype=torch.int64) if score else None
    cout = torch.empty(B, 4, device=dev, dtype=torch.int64) if comp else None
    # the smallest entry point for what is asked; the component's takes conf and qsum null for no score
    name = "fs_unwarp_instances_component" if comp else "fs_unwarp_instances_scored" if score else "fs_unwarp_instances"
    scratch = torch.empty(hip.query(name + "_scratch_ints", B, h, w, Hs, Ws), device=dev, dtype=torch.int32)
    tensors = ([cls.contiguous(), m.contiguous(), grid.contiguous()] + ([f] if comp else []) + [cat, stats, counts, bits] +
               ([cout] if comp else []) + ([conf, qsum] if comp or score else []) + [scratch])
    hip.call(name, *[hip.ptr(t) for t in tensors], B, K, h, w, Hs, Ws, cap, *((conn, snap2) if comp else ()))
    return (cat, stats, counts) + ((bits,) if return_bits else ()) + ((conf, qsum) if score else ()) + ((cout,) if comp else ())


def _hd_q(q):
    if isinstance(q, bool) or int(q) != q or not 1 <= int(q) <= 100:
        raise ValueError(f"the Hausdorff percentile must be an integer 1 .. 100, got {q!r}")
    return int(q)


def unwarp_count(cls, m, grid, y, cls_label, dia_factor=None, frame=True, areas=False, return_labels=False, hd_q=None):
    """The checks, allocations and call that unwarp_accuracy, unwarp_trimap and unwarp_class_areas share; models.py's evaluate() calls
    it directly.  Internal to the package: the documented ops are those three.  dia_factor=None: no trimap.  hd_q (None, or 1 .. 100):
    the surface-distance statistics of surface_hd, prediction foreground (class != K-1) against label foreground.  The entry point is
    the smallest that counts what is asked for: fs_unwarp_hd with hd_q, else fs_unwarp_class_areas with areas, else fs_unwarp_trimap
    with a trimap, else fs_unwarp_accuracy.  Returns the six-tuple (counts, acc, areas, trim, labels, hd) in this order, None where not
    asked for."""
    with_trim = dia_factor is not None
    D, fr = _trimap_args(dia_factor, frame) if with_trim else (0, 0)
    q = _hd_q(hd_q) if hd_q is not None else None
    B, K = cls.shape
    _, h, w, _ = grid.shape
    if tuple(m.shape) != (B, h, w):
        raise ValueError(f"m {tuple(m.shape)} must be (B, h, w) = {(B, h, w)}: the mask at the grid's resolution")
    if y.dim() == 4 and y.shape[1] == 1:
        y = y[:, 0]
    if y.dim() != 3 or y.shape[0] != B:
        raise ValueError(f"y {tuple(y.shape)} must be (B, Hs, Ws) or (B, 1, Hs, Ws) with B = {B}")
    Hs, Ws = int(y.shape[1]), int(y.shape[2])
    if cls_label.dim() == 2 and cls_label.shape[1] == 1:
        cls_label = cls_label[:, 0]
    if tuple(cls_label.shape) != (B,):
        raise ValueError(f"cls_label {tuple(cls_label.shape)} must be (B,) or (B, 1) with B = {B}")
    dev = cls.device
    counts = torch.empty(B, 6, device=dev, dtype=torch.int64)
    acc = torch.empty(4, device=dev, dtype=torch.float32)
    area = torch.empty(B, 3, K, 3, device=dev, dtype=torch.int64) if areas else None
    trim = torch.empty(B, D + 1, 3, device=dev, dtype=torch.int64) if with_trim else None
    labels = torch.empty(B, Hs, Ws, device=dev, dtype=torch.int64) if return_labels else None
    hd = torch.empty(B, 4, device=dev, dtype=torch.int64) if q is not None else None
    # (entry point, the dimensions its scratch query takes, its outputs after acc, its arguments after the dimensions)
    if q is not None:
        name, qdims, outs, tail = "fs_unwarp_hd", (B, K, h, w, Hs, Ws), (area, trim, labels, hd), (D, fr, q)
    elif areas:
        name, qdims, outs, tail = "fs_unwarp_class_areas", (B, K, h, w, Hs, Ws), (area, trim, labels), (D, fr)
    elif with_trim:
        name, qdims, outs, tail = "fs_unwarp_trimap", (B, h, w, Hs, Ws), (trim, labels), (D, fr)
    else:
        name, qdims, outs, tail = "fs_unwarp_accuracy", (B, h, w, Hs, Ws), (labels,), ()
    scratch = torch.empty(hip.query(name + "_scratch_ints", *qdims), device=dev, dtype=torch.int32)
    hip.call(name, hip.ptr(cls.contiguous()), hip.ptr(m.contiguous()), hip.ptr(grid.contiguous()), hip.ptr(y.float().contiguous()),
             hip.ptr(cls_label.long().contiguous()), hip.ptr(counts), hip.ptr(acc), *(hip.ptr(t) for t in outs), hip.ptr(scratch),
             B, K, h, w, Hs, Ws, *tail)
    return counts, acc, area, trim, labels, hd


def unwarp_accuracy(cls, m, grid, y, cls_label, return_labels=False):
    """The four full-resolution accuracies of MODEL.upsample for the C1 head (no autograd), without the (B,K,Hs,Ws) prediction, a class
    map or a ground-truth tensor: the predicted class of a pixel is `unwarp_labels`'s, its ground truth `t = y.long()`,
    `t * cls_label + (1 - t) * (K - 1)`, and the gather pass counts instead of storing (fs_unwarp_accuracy).  cls (B,K), m (B,h,w),
    grid (B,h,w,2) as for unwarp_labels; y (B,Hs,Ws) or (B,1,Hs,Ws) the label mask at the output size; cls_label (B,) or (B,1).
    Returns (counts (B,6) int64 = cls_fg, bin_fg, union_fg, cls_bg, bin_bg, union_bg per image, acc (4,) fp32 = acc, acc_bin_fg,
    acc_cls_fbg, acc_bin_fbg as SegLoss's out[3:7]) and, with return_labels, the (B,Hs,Ws) int64 class map of unwarp_labels."""
    counts, acc, _, _, labels, _ = unwarp_count(cls, m, grid, y, cls_label, return_labels=return_labels)
    return (counts, acc, labels) if return_labels else (counts, acc)


def _trimap_args(dia_factor, frame):
    D = int(dia_factor)
    if not 0 <= D <= 7:
        raise ValueError(f"dia_factor must be 0 .. 7 (band widths 1 .. 2**dia_factor), got {dia_factor}")
    return D, 1 if frame else 0


def trimap_bands(y, dia_factor=5, frame=True):
    """Which trimap band every pixel of the label mask lies in (eval.py:41-67; VAL.trimap_dia_factor): uint8 (B,Hs,Ws), the smallest
    i <= dia_factor such that the pixel is within 2**i city-block steps of the label's boundary, 255 if none, so that band i of the
    reference (FIND_EDGES, then binary_dilation(iterations=2**i)) is `bands <= i` (fs_trimap_bands).  y (B,Hs,Ws) or (B,1,Hs,Ws), read
    as t = y.long().  A boundary seed is a background pixel (t == 0) with a foreground 8-neighbour; frame=True also seeds every
    background pixel of the outer one-pixel ring, as PIL's filter does -- the reference bit for bit -- and frame=False is the
    neighbour rule alone, pixels outside the image being background.  No autograd."""
    D, fr = _trimap_args(dia_factor, frame)
    if y.dim() == 4 and y.shape[1] == 1:
        y = y[:, 0]
    if y.dim() != 3 or y.numel() == 0:
        raise ValueError(f"y {tuple(y.shape)} must be a non-empty (B, Hs, Ws) or (B, 1, Hs, Ws)")
    B, Hs, Ws = (int(v) for v in y.shape)
    band = torch.empty(B, Hs, Ws, device=y.device, dtype=torch.uint8)
    scratch = torch.empty(hip.query("fs_trimap_bands_scratch_ints", B, Hs, Ws), device=y.device, dtype=torch.int32)
    hip.call("fs_trimap_bands", hip.ptr(y.float().contiguous()), hip.ptr(band), hip.ptr(scratch), B, Hs, Ws, D, fr)
    return band


def unwarp_trimap(cls, m, grid, y, cls_label, dia_factor=5, frame=True, return_labels=False):
    """unwarp_accuracy with the trimap boundary accuracies of eval.py:41-67 counted in the same gather pass (fs_unwarp_trimap).
    Arguments and checks are unwarp_accuracy's; dia_factor / frame are trimap_bands'.  Returns (counts, acc, trim[, labels]): counts,
    acc and labels are unwarp_accuracy's bit for bit, trim (B, dia_factor + 1, 3) int64 holds per image and band width 2**i the number of
    pixels in the band, of those whose predicted class equals the ground truth (the reference's acc_sum) and of those that agree with
    it on foreground versus background.  An image without a boundary seed (a constant label with frame=False, an all-foreground one
    with frame=True) has all-zero rows: the reference divides 0 by 0 there, trimap_from_counts and train.TrimapMeter leave it out."""
    if dia_factor is None:
        raise TypeError("unwarp_trimap needs dia_factor (0 .. 7); unwarp_accuracy is the op without a trimap")
    counts, acc, _, trim, labels, _ = unwarp_count(cls, m, grid, y, cls_label, dia_factor, frame, return_labels=return_labels)
    return (counts, acc, trim, labels) if return_labels else (counts, acc, trim)


def trimap_from_counts(trim):
    """(B, D+1, 3) trim counters (unwarp_trimap's, on any device) -> (B, D+1, 2) fp64: per image and band width the class accuracy
    cls_ok / (total + 1e-10) -- the reference's Python-float quotient, eval.py:64 -- and the foreground / background accuracy
    bin_ok / (total + 1e-10).  An empty band gives 0; `trim[..., 0] > 0` tells which images count (see unwarp_trimap)."""
    if trim.dim() != 3 or trim.shape[2] != 3:
        raise ValueError(f"trim must be (B, D+1, 3), got {tuple(trim.shape)}")
    t = trim.to(torch.float64)
    return t[..., 1:] / (t[..., :1] + 1e-10)


def unwarp_class_areas(cls, m, grid, y, cls_label, dia_factor=None, frame=True, return_labels=False):
    """unwarp_accuracy with the per-class areas of the reference's evaluation summary (eval.py:218-257,313-322; utils.intersectionAndUnion,
    utils.py:289-317) counted in the same gather pass (fs_unwarp_class_areas).  Arguments and checks are unwarp_trimap's; dia_factor=None
    leaves the trimap out.  Returns (counts, acc, areas[, trim][, labels]): counts, acc, trim and labels are unwarp_accuracy's /
    unwarp_trimap's bit for bit; areas (B, 3, K, 3) int64 holds per image, space and class (inter, pred, lab), the union being
    pred + lab - inter.  Space 0 is the prediction at full resolution (unwarp_labels against the ground truth), space 1 the sampling
    ceiling -- the label after the sampler and the nearest un-warp against itself (VAL.y_sampled_reverse, models/models_instance.py:909-918):
    every pixel takes grid_sample_label's value of the grid point that feeds it -- and space 2 the prediction in the sampled space
    (PredAssemble(cls, m).argmax(1) against the sampled ground truth).  A cls_label outside 0 .. K-1 has no lab / inter row."""
    counts, acc, areas, trim, labels, _ = unwarp_count(cls, m, grid, y, cls_label, dia_factor, frame, areas=True, return_labels=return_labels)
    return (counts, acc, areas) + ((trim,) if trim is not None else ()) + ((labels,) if return_labels else ())


def class_scores_from_areas(areas):
    """(..., K, 3) class areas (unwarp_class_areas', on any device; summed over a dataset or not) -> (iou, dice), each (..., K) fp64:
    iou = inter / (union + 1e-10) and dice = 2 * inter / (union + inter + 1e-10) with union = pred + lab - inter -- the reference's
    expressions (eval.py:252, 313-315).  A class with an empty union scores 0."""
    if areas.dim() < 2 or areas.shape[-1] != 3:
        raise ValueError(f"areas must be (..., K, 3), got {tuple(areas.shape)}")
    a = areas.to(torch.float64)
    inter, union = a[..., 0], a[..., 1] + a[..., 2] - a[..., 0]
    return inter / (union + 1e-10), 2 * inter / (union + inter + 1e-10)


def surface_hd(a, b, q=95):
    """The q-th percentile of the Hausdorff distances between the borders of two masks (HD95 at q = 95; VAL.hd95), as the integers it is
    made of (fs_surface_hd; no autograd).  a, b (B,H,W) or (H,W), bool or uint8 (non-zero = foreground), on the device; H, W <= 16384.
    The border of a mask is its foreground with a background 4-neighbour, outside the image counting as background; every border pixel
    of either mask takes the squared distance to the nearest border pixel of the other, and the two sets are pooled.  Returns hd (B,4)
    int64 = (n_a, n_b, d2_lo, d2_hi): the border sizes and the pooled squared distances at the two ranks np.percentile interpolates
    between; d2 = -1 where a border is empty.  hd_from_stats makes the distance.  This is the published 2-D definition; the
    reference's utils.hd95 flattens both masks before it erodes them and returns something else."""
    q = _hd_q(q)
    if a.dim() == 2 and b.dim() == 2:
        a, b = a[None], b[None]
    if a.dim() != 3 or a.shape != b.shape or a.numel() == 0:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} must be two non-empty (B, H, W) masks of one shape")
    if a.dtype not in (torch.bool, torch.uint8) or b.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"masks must be bool or uint8, got {a.dtype} and {b.dtype}")
    B, Hs, Ws = (int(v) for v in a.shape)
    fg = ((a != 0).to(torch.uint8) | ((b != 0).to(torch.uint8) << 1)).contiguous()
    hd = torch.empty(B, 4, device=a.device, dtype=torch.int64)
    scratch = torch.empty(hip.query("fs_surface_hd_scratch_ints", B, Hs, Ws), device=a.device, dtype=torch.int32)
    hip.call("fs_surface_hd", hip.ptr(fg), hip.ptr(hd), hip.ptr(scratch), B, Hs, Ws, q)
    return hd


def hd_from_stats(hd, q=95):
    """(B,4) surface statistics (surface_hd's / evaluate(hausdorff=q)'s, on any device) -> (B,) fp64: np.percentile(distances, q) =
    sqrt(d2_lo) + (sqrt(d2_hi) - sqrt(d2_lo)) * frac with frac = (q (n-1) mod 100) / 100, n = n_a + n_b; NaN where a border is empty
    (the reference raises there).  q must be the q the statistics were made with.  Plain torch."""
    q = _hd_q(q)
    if hd.dim() != 2 or hd.shape[1] != 4:
        raise ValueError(f"hd must be (B, 4), got {tuple(hd.shape)}")
    hd = hd.to(torch.int64)
    n = hd[:, 0] + hd[:, 1]
    frac = ((q * (n - 1)) % 100).to(torch.float64) / 100.0
    empty = (hd[:, 0] <= 0) | (hd[:, 1] <= 0) | (hd[:, 2] < 0)
    lo, hi = hd[:, 2].clamp(min=0).to(torch.float64).sqrt(), hd[:, 3].clamp(min=0).to(torch.float64).sqrt()
    out = lo + (hi - lo) * frac
    return torch.where(empty, torch.full_like(out, float("nan")), out)


def image_accuracies_from_counts(counts):
    """(B,6) counts -> (B,4) fp32 per-image acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg (models/models.py:378-474): plain torch, any device."""
    c = counts.to(torch.float32)
    ufg, ubg = c[:, 2] + 1e-10, c[:, 5] + 1e-10
    cls_fg, bin_fg, cls_bg, bin_bg = c[:, 0] / ufg, c[:, 1] / ufg, c[:, 3] / ubg, c[:, 4] / ubg
    return torch.stack([cls_fg, bin_fg, cls_fg * 0.5 + cls_bg * 0.5, bin_fg * 0.5 + bin_bg * 0.5], 1)


def accuracies_from_counts(counts):
    """(B,6) counts (unwarp_accuracy's, on any device) -> (4,) fp32: the batch's four accuracies, the mean over its images of the fp32
    per-image quotients -- fs_unwarp_accuracy's and SegLoss's arithmetic in plain torch."""
    if counts.dim() != 2 or counts.shape[1] != 6:
        raise ValueError(f"counts must be (B, 6), got {tuple(counts.shape)}")
    return (image_accuracies_from_counts(counts).double().sum(0) / counts.shape[0]).float()
