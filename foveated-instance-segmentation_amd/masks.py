"""Masks as bit words (csrc/mask_words.h): packing, COCO run-length codes and strings, the component under the gaze, erosion /
boundary / pair counters, polygons, candidates, and the COCO record converters.

Every function checks its arguments, allocates and makes one `hip.call`; stateless, no autograd.  Imports none of the package's other
op modules.
"""
import math

import torch

from . import hip

__all__ = [
    "mask_bits", "mask_rle", "COMPONENT_OFF2", "mask_component", "boundary_dilation", "MORPH_MAX_D", "boundary_dilation_capped", "mask_erode",
    "mask_boundary", "mask_pair_counts", "pair_scores", "RLE_STATUS", "rle_bits", "rle_to_string", "RLE_STRING_GROUPS", "rle_from_string",
    "instances_to_coco", "INT32_MAX", "coco_to_instances", "POLY_SIDE_MAX", "POLY_STATUS", "polygon_rings", "poly_bits",
    "coco_masks", "mask_candidates", "coco_candidates",
]


def _max_runs(max_runs, Ws):
    """The capacity of a run-length code: any int >= 1; None = 8 * Ws + 1, which holds every mask whose columns each cross its outline
    at most eight times (a blob entered and left four times by a column) -- 32 KB of int32 per 1024-wide image."""
    if max_runs is None:
        return 8 * int(Ws) + 1
    if isinstance(max_runs, bool) or int(max_runs) != max_runs or int(max_runs) < 1:
        raise ValueError(f"max_runs must be an integer >= 1, got {max_runs!r}")
    return int(max_runs)


def mask_bits(mask):
    """A mask as bit words (fs_mask_bits; no autograd): mask (B,Hs,Ws) or (Hs,Ws), bool or uint8 (non-zero = set), on the device.
    Returns bits (B,Hs,P) int32, P = ceil(Ws / 32): bit j of word i of row y is pixel x = 32 i + j, the bits at x >= Ws are 0."""
    if mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3 or mask.numel() == 0:
        raise ValueError(f"mask {tuple(mask.shape)} must be a non-empty (B, Hs, Ws)")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"the mask must be bool or uint8, got {mask.dtype}")
    B, Hs, Ws = (int(v) for v in mask.shape)
    bits = torch.empty(B, Hs, (Ws + 31) // 32, device=mask.device, dtype=torch.int32)
    hip.call("fs_mask_bits", hip.ptr(mask.contiguous()), hip.ptr(bits), B, Hs, Ws)
    return bits


def _bits_arg(mask_or_bits, Ws):
    """(bits (B,Hs,P) int32, Ws) of a mask argument as mask_rle / mask_component take it; bits is None for a mask still to be packed."""
    if not isinstance(mask_or_bits, torch.Tensor):
        raise ValueError("the mask must be a tensor: bool / uint8 (B,Hs,Ws) or (Hs,Ws), or int32 bit words with Ws")
    if mask_or_bits.dtype == torch.int32:
        bits = mask_or_bits
        if bits.dim() != 3 or bits.numel() == 0 or Ws is None or int(Ws) < 1 or bits.shape[2] != (int(Ws) + 31) // 32:
            raise ValueError(f"bit words {tuple(bits.shape)} must be a non-empty (B, Hs, ceil(Ws / 32)) with Ws given, got Ws = {Ws!r}")
        return bits, int(Ws)
    if mask_or_bits.dtype not in (torch.bool, torch.uint8) or mask_or_bits.dim() not in (2, 3) or mask_or_bits.numel() == 0:
        raise ValueError(f"the mask must be a non-empty bool / uint8 (B,Hs,Ws) or (Hs,Ws), got {mask_or_bits.dtype} {tuple(mask_or_bits.shape)}")
    if Ws is not None and int(Ws) != mask_or_bits.shape[-1]:
        raise ValueError(f"Ws = {Ws!r} differs from the mask's width {mask_or_bits.shape[-1]}")
    return None, int(mask_or_bits.shape[-1])


def _mask_words(mask_or_bits, Ws):
    """_bits_arg with the mask packed: (bits (B,Hs,P) int32, Ws)."""
    bits, Ws = _bits_arg(mask_or_bits, Ws)
    return (mask_bits(mask_or_bits) if bits is None else bits), Ws


def mask_rle(mask_or_bits, Ws=None, max_runs=None):
    """Area, box and uncompressed COCO run-length code of any mask, exact and on the device (fs_mask_rle; no autograd).  The argument
    is a bool / uint8 mask (B,Hs,Ws) or (Hs,Ws), or int32 bit words (B,Hs,ceil(Ws/32)) as mask_bits returns them together with Ws.
    Returns (stats (B,6) int64 = area, x0, y0, bw, bh, n_runs; counts (B,max_runs) int32).  [x0, y0, bw, bh] is the COCO box of the set
    pixels, all 0 for an empty mask.  counts is the code of the mask read column-major (p = x * Hs + y): the run of zeros before the
    first set pixel (0 when pixel (0,0) is set), then alternating run lengths, runs continuing from the bottom of a column into the
    top of the next; an empty mask is [Hs * Ws], a full one [0, Hs * Ws].  n_runs is always the true length of the code; the first
    min(n_runs, max_runs) entries of counts are its, the rest is 0, and n_runs > max_runs tells that the code was cut.  max_runs
    defaults to 8 * Ws + 1 (see _max_runs).  The format is restated from its published definition (pycocotools' uncompressed RLE)."""
    bits, Ws = _mask_words(mask_or_bits, Ws)
    B, Hs = int(bits.shape[0]), int(bits.shape[1])
    cap = _max_runs(max_runs, Ws)
    stats = torch.empty(B, 6, device=bits.device, dtype=torch.int64)
    counts = torch.empty(B, cap, device=bits.device, dtype=torch.int32)
    scratch = torch.empty(hip.query("fs_mask_rle_scratch_ints", B, Hs, Ws), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_rle", hip.ptr(bits.contiguous()), hip.ptr(stats), hip.ptr(counts), hip.ptr(scratch), B, Hs, Ws, cap)
    return stats, counts


COMPONENT_OFF2 = 2 ** 62                            # a squared distance no pixel reaches: snap_px = None


def _component_args(component, snap_px):
    """(conn, snap2) of mask_component / unwarp_instances(component=...): connectivity 4 or 8; snap_px None (no limit) or a finite number
    of pixels >= 0, snap2 = floor(snap_px ** 2)."""
    if isinstance(component, bool) or component not in (4, 8):
        raise ValueError(f"the connectivity must be 4 or 8, got {component!r}")
    if snap_px is None:
        return int(component), COMPONENT_OFF2
    px = float(snap_px)
    if not (px >= 0.0) or math.isinf(px):
        raise ValueError(f"snap_px must be a finite number of pixels >= 0, got {snap_px!r}")
    return int(component), COMPONENT_OFF2 if px >= 2.0 ** 31 else int(math.floor(px * px))     # 2^31 squared is 2^62: no overflow in px * px


def _focus_arg(focus, B, dev):
    if not isinstance(focus, torch.Tensor) or tuple(focus.shape) != (B, 2):
        raise ValueError(f"focus must be (B, 2) = ({B}, 2), got {tuple(getattr(focus, 'shape', ()))}")
    return focus.to(device=dev, dtype=torch.float32).contiguous()


def mask_component(mask_or_bits, focus, Ws=None, connectivity=8, snap_px=None):
    """The connected component of a mask under the gaze, on the device and on bit words (fs_mask_component; no autograd; unpinned:
    the reference has no counterpart).  The mask as mask_rle takes it: bool / uint8 (B,Hs,Ws) or (Hs,Ws), or int32 bit words
    (B,Hs,ceil(Ws/32)) together with Ws.  focus (B,2) normalised (row, col), turned into a gaze pixel as gate_decide does.  The seed is
    the gaze pixel where it is set, else the nearest set pixel (ties: the smaller row-major index), unless it lies more than snap_px
    pixels away (None: any distance; snap2 = floor(snap_px ** 2) against the squared distance).  connectivity 4 or 8.  Returns
    (bits_c (B,Hs,ceil(Ws/32)) int32, the component's words, all 0 where there is none; comp (B,4) int64 = (seed_y, seed_x, d2, area_all),
    (-1, -1, -1, area_all) where there is none; area_all counts the input's set pixels).  mask_rle(bits_c, Ws) gives its record."""
    conn, snap2 = _component_args(connectivity, snap_px)
    bits, Ws = _mask_words(mask_or_bits, Ws)
    B, Hs = int(bits.shape[0]), int(bits.shape[1])
    f = _focus_arg(focus, B, bits.device)
    out = torch.empty_like(bits, memory_format=torch.contiguous_format)
    comp = torch.empty(B, 4, device=bits.device, dtype=torch.int64)
    scratch = torch.empty(hip.query("fs_mask_component_scratch_ints", B, Hs, Ws), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_component", hip.ptr(bits.contiguous()), hip.ptr(f), hip.ptr(out), hip.ptr(comp), hip.ptr(scratch), B, Hs, Ws, conn, snap2)
    return out, comp


def boundary_dilation(Hs, Ws, ratio=0.02):
    """The dilation of Boundary IoU in pixels (Cheng et al., CVPR 2021, restated: unpinned): d = max(1, int(round(ratio *
    math.sqrt(Hs * Hs + Ws * Ws)))) in Python floats, ratio a finite float > 0 -- 0.02 of the image diagonal, 29 at 1024 x 1024."""
    if isinstance(Hs, bool) or isinstance(Ws, bool) or int(Hs) != Hs or int(Ws) != Ws or int(Hs) < 1 or int(Ws) < 1:
        raise ValueError(f"the size must be two integers >= 1, got {(Hs, Ws)!r}")
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not (float(ratio) > 0.0) or math.isinf(float(ratio)):
        raise ValueError(f"the boundary ratio must be a finite number > 0, got {ratio!r}")
    Hs, Ws = int(Hs), int(Ws)
    return max(1, int(round(float(ratio) * math.sqrt(Hs * Hs + Ws * Ws))))


MORPH_MAX_D = 2047                                  # fs_mask_erode's cap: a diagonal of 100 000 pixels at the default ratio


def _morph_d(d):
    if isinstance(d, bool) or not isinstance(d, int) or d < 1 or d > MORPH_MAX_D:
        raise ValueError(f"d must be an int 1 .. {MORPH_MAX_D}, got {d!r}")
    return d


def boundary_dilation_capped(Hs, Ws, ratio):
    """boundary_dilation(Hs, Ws, ratio) where fs_mask_erode can take it; ValueError above MORPH_MAX_D, before anything is launched."""
    d = boundary_dilation(Hs, Ws, ratio)
    if d > MORPH_MAX_D:
        raise ValueError(f"boundary {ratio!r} gives a dilation of {d} pixels at {(Hs, Ws)}, above ops.MORPH_MAX_D = {MORPH_MAX_D}")
    return d


def mask_erode(mask_or_bits, d, Ws=None):
    """Erosion of a mask by a (2d+1) x (2d+1) square, on the device and on bit words (fs_mask_erode; no autograd; unpinned: restated
    from the published definition of Boundary IoU).  The mask as mask_rle takes it: bool / uint8 (B,Hs,Ws) or (Hs,Ws), or int32 bit
    words (B,Hs,ceil(Ws/32)) together with Ws; d an int >= 1 (and <= 2047), not a bool.  Returns bits (B,Hs,ceil(Ws/32)) int32: pixel
    (y,x) is set iff every pixel of the square centred on it is set, every pixel outside the image counting as unset -- scipy's
    binary_erosion(m, ones((3,3)), iterations=d, border_value=0); all 0 where 2d+1 exceeds a side."""
    d = _morph_d(d)
    bits, Ws = _mask_words(mask_or_bits, Ws)
    B, Hs = int(bits.shape[0]), int(bits.shape[1])
    out = torch.empty_like(bits, memory_format=torch.contiguous_format)
    scratch = torch.empty(max(1, hip.query("fs_mask_erode_scratch_ints", B, Hs, Ws, d)), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_erode", hip.ptr(bits.contiguous()), hip.ptr(out), hip.ptr(scratch), B, Hs, Ws, d)
    return out


def mask_boundary(mask_or_bits, d, Ws=None):
    """The boundary band of Boundary IoU as bit words: m & ~mask_erode(m, d), the set pixels within d of an unset pixel or of the
    image's outside (chessboard distance); the mask itself where 2d+1 exceeds a side.  Arguments as mask_erode's; the bits at
    x >= Ws of the result are 0."""
    d = _morph_d(d)
    bits, Ws = _mask_words(mask_or_bits, Ws)
    er = mask_erode(bits, d, Ws)
    band = bits & ~er
    if Ws & 31:
        band[:, :, -1] &= (1 << (Ws & 31)) - 1                      # the input's padding bits are no pixels
    return band


def mask_pair_counts(a, b, d, Ws=None):
    """The counters of mask IoU and Boundary IoU of a prediction a and a label b (fs_mask_pair_counts; no autograd; unpinned).  a and
    b as mask_erode takes a mask, of one shape and kind; d as there.  Returns pair (B,6) int64 = (|a & b|, |a|, |b|, |band(a) &
    band(b)|, |band(a)|, |band(b)|), band = mask_boundary's; both erosions and the counts are taken on the device without a host
    read, on nothing wider than a bit a pixel.  pair_scores makes the two measures."""
    d = _morph_d(d)
    abits, Wa = _bits_arg(a, Ws)
    bbits, Wb = _bits_arg(b, Ws)
    if (abits is None) != (bbits is None) or tuple(a.shape[-2:]) != tuple(b.shape[-2:]) or Wa != Wb or a.device != b.device:
        raise ValueError(f"the two masks must be of one kind, size and device, got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")
    if abits is None:
        if (a.dim() == 3 and b.dim() == 3 and a.shape[0] != b.shape[0]) or a.dim() != b.dim():
            raise ValueError(f"the two masks must have one batch size, got {tuple(a.shape)} and {tuple(b.shape)}")
        abits, bbits = mask_bits(a), mask_bits(b)
    elif a.shape[0] != b.shape[0]:
        raise ValueError(f"the two masks must have one batch size, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, Hs = int(abits.shape[0]), int(abits.shape[1])
    pair = torch.empty(B, 6, device=abits.device, dtype=torch.int64)
    scratch = torch.empty(max(1, hip.query("fs_mask_pair_scratch_ints", B, Hs, Wa, d)), device=abits.device, dtype=torch.int32)
    hip.call("fs_mask_pair_counts", hip.ptr(abits.contiguous()), hip.ptr(bbits.contiguous()), hip.ptr(pair), hip.ptr(scratch), B, Hs, Wa, d)
    return pair


def pair_scores(pair):
    """(iou, biou), two fp64 tensors (B,), from mask_pair_counts' counters: n / (a + b - n) per triple, 0 where the union is 0."""
    if pair.dim() != 2 or pair.shape[1] != 6:
        raise ValueError(f"pair must be (B, 6), got {tuple(pair.shape)}")
    p = pair.to(torch.int64)
    out = []
    for o in (0, 3):
        n, u = p[:, o], p[:, o + 1] + p[:, o + 2] - p[:, o]
        out.append(torch.where(u > 0, n.double() / u.clamp(min=1).double(), torch.zeros_like(n, dtype=torch.float64)))
    return out[0], out[1]


RLE_STATUS = {0: "valid", 1: "the code was cut: n_runs exceeds the capacity of counts", 2: "n_runs is below 1 or a count is negative",
              3: "the counts do not sum to Hs * Ws"}


def rle_bits(counts, n_runs, size, check=False):
    """mask_rle's inverse: the uncompressed run-length code back into bit words, on the device (fs_rle_bits; no autograd; unpinned, as
    the code itself).  counts (B,cap) int32 on the device, as mask_rle / unwarp_instances / coco_to_instances make them; n_runs the
    codes' lengths, int64 (B,) -- or a stats (B,6) int64 tensor, whose column 5 is read where it lies, without a copy; size = (Hs, Ws).
    Entries of counts at or past n_runs are never read.  Every well-formed code decodes, canonical or not (zero-length runs anywhere).
    Returns (bits (B,Hs,ceil(Ws/32)) int32 in mask_bits' layout, the bits at x >= Ws 0; info (B,4) int64 = (status, area, n_read,
    total)): status 0 valid, 1 cut (n_runs > cap), 2 bad (n_runs < 1 or a negative count), 3 the counts do not sum to Hs * Ws (the
    first that applies); area the set pixels of a valid code, else 0; an image whose status is not 0 gets all-zero words.  No host
    read -- unless check=True, which reads info once and raises ValueError naming the first such image and its status in words."""
    B, cap, Hs, Ws = _rle_args(counts, n_runs, size)
    n_runs = n_runs.contiguous()
    n_ptr, n_stride = (hip.ptr(n_runs) + 5 * 8, 6) if n_runs.dim() == 2 else (hip.ptr(n_runs), 1)
    dev = counts.device
    bits = torch.empty(B, Hs, (Ws + 31) // 32, device=dev, dtype=torch.int32)
    info = torch.empty(B, 4, device=dev, dtype=torch.int64)
    scratch = torch.empty(hip.query("fs_rle_bits_scratch_ints", B, cap), device=dev, dtype=torch.int32)
    hip.call("fs_rle_bits", hip.ptr(counts.contiguous()), n_ptr, n_stride, hip.ptr(bits), hip.ptr(info), hip.ptr(scratch), B, Hs, Ws, cap)
    if check:
        for b, st in enumerate(info[:, 0].cpu().tolist()):
            if st != 0:
                raise ValueError(f"image {b}: {RLE_STATUS[st]} (status {st}; size {(Hs, Ws)}, capacity {cap})")
    return bits, info


def _rle_args(counts, n_runs, size):
    """(B, cap, Hs, Ws) of rle_bits' arguments, or ValueError: the checks of the host, nothing launched."""
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.dim() != 2 or counts.numel() == 0:
        raise ValueError(f"counts must be a non-empty int32 (B, cap) tensor, got {getattr(counts, 'dtype', None)} {tuple(getattr(counts, 'shape', ()))}")
    B, cap = int(counts.shape[0]), int(counts.shape[1])
    if not isinstance(n_runs, torch.Tensor) or n_runs.dtype != torch.int64 or tuple(n_runs.shape) not in ((B,), (B, 6)) \
            or n_runs.device != counts.device:
        raise ValueError(f"n_runs must be an int64 (B,) = ({B},) tensor or a stats ({B}, 6) tensor on counts' device, got "
                         f"{getattr(n_runs, 'dtype', None)} {tuple(getattr(n_runs, 'shape', ()))}")
    if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in size):
        raise ValueError(f"size must be two integers >= 1 (Hs, Ws), got {size!r}")
    return B, cap, int(size[0]), int(size[1])


def rle_to_string(counts):
    """The compressed string form of a run-length code, the one COCO / LVIS files carry (host; unpinned: restated from the published
    definition, pycocotools' rleToString).  counts: a list of Python ints.  Count i is written as x = counts[i], less counts[i - 2]
    for i > 2, in 5-bit groups, low group first: c = x & 31, x >>= 5 (arithmetic); another group follows iff x != -1 where c & 16 is
    set, iff x != 0 otherwise; a group that is followed has bit 32 set; the character is chr(c + 48).  [0, 5] -> "05",
    [10, 20, 30, 5] -> ":d0n0A"."""
    out = []
    counts = list(counts)
    for i, v in enumerate(counts):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"count {i} must be a Python int, got {v!r}")
        x = v - counts[i - 2] if i > 2 else v
        while True:
            c = x & 31
            x >>= 5
            more = x != -1 if c & 16 else x != 0
            out.append(chr((c | 32 if more else c) + 48))
            if not more:
                break
    return "".join(out)


RLE_STRING_GROUPS = 13                              # 65 bits: more than any int64 count or difference needs


def rle_from_string(s):
    """rle_to_string's inverse (host; unpinned: pycocotools' rleFrString restated): s a str or ASCII bytes -> the list of counts.  Per
    count, (c & 31) << 5 k is accumulated over the groups k = 0, 1, ... while bit 32 of c = ord(ch) - 48 is set, the value is
    sign-extended from bit 16 of the last group, and counts[i - 2] is added for i > 2.  ValueError, naming the position, for a character
    outside chr(48) .. chr(111), a string that ends inside a count, or a count of more than 13 groups; an empty string is []."""
    if isinstance(s, (bytes, bytearray)):
        try:
            s = bytes(s).decode("ascii")
        except UnicodeDecodeError:
            raise ValueError("the compressed code holds a byte outside ASCII") from None
    if not isinstance(s, str):
        raise ValueError(f"the compressed code must be a str or bytes, got {type(s).__name__}")
    counts, p, n = [], 0, len(s)
    while p < n:
        x, k = 0, 0
        while True:
            if p >= n:
                raise ValueError(f"the compressed code ends inside count {len(counts)} (position {p})")
            c = ord(s[p]) - 48
            if c < 0 or c > 63:
                raise ValueError(f"character {s[p]!r} at position {p} is outside chr(48) .. chr(111)")
            if k >= RLE_STRING_GROUPS:
                raise ValueError(f"count {len(counts)} has more than {RLE_STRING_GROUPS} groups (position {p})")
            x |= (c & 31) << (5 * k)
            p, k = p + 1, k + 1
            if not c & 32:
                if c & 16:
                    x -= 1 << (5 * k)
                break
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def instances_to_coco(cat, stats, counts, seg_size, image_ids=None, conf=None, compressed=False):
    """unwarp_instances' / predict_instances' tensors (on any device) as a list of COCO / LVIS result records, one per image:
    {"image_id", "category_id", "bbox": [x, y, w, h], "area", "segmentation": {"size": [H, W], "counts": [...]}} with the uncompressed
    run-length code pycocotools.mask.frPyObjects takes -- or, with compressed=True, "counts" as the compressed string result files carry
    (rle_to_string; about a fifth of the list's size in JSON).  One device-to-host copy.  category_id is the class index cat[b]; image_id is
    image_ids[b], or b.  With conf (B,3) -- unwarp_instances(score=True)'s / predict_instances(return_score=True)'s -- every record
    also has "score": conf[b, 0] as a Python float, the key COCOeval and the LVIS evaluator rank by; without it no score is made up.
    OverflowError, naming the image and the max_runs it needs, where a code was cut (n_runs > counts.shape[1]); ValueError, naming the
    image, where a score is NaN.  coco_to_instances is the inverse."""
    B, cap = int(counts.shape[0]), int(counts.shape[1])
    if tuple(cat.shape) != (B,) or tuple(stats.shape) != (B, 6) or counts.dim() != 2:
        raise ValueError(f"cat {tuple(cat.shape)}, stats {tuple(stats.shape)}, counts {tuple(counts.shape)} must be (B,), (B, 6), (B, max_runs)")
    H, W = int(seg_size[0]), int(seg_size[1])
    ids = list(range(B)) if image_ids is None else list(image_ids)
    if len(ids) != B:
        raise ValueError(f"{len(ids)} image ids for {B} images")
    if conf is not None and (conf.dim() != 2 or conf.shape[0] != B or conf.shape[1] < 1):
        raise ValueError(f"conf {tuple(conf.shape)} must be (B, 3) = ({B}, 3): (score, cls_prob, mask_prob) per image")
    head = torch.cat([cat.to(torch.int64).reshape(B, 1), stats.to(torch.int64)], 1).contiguous()
    parts = [head.view(torch.int32)]                                                   # the int64 columns as pairs of words
    if conf is not None:
        parts.append(conf[:, :1].to(torch.float32).contiguous().view(torch.int32))     # the score's fp32 word
    n0 = sum(int(t.shape[1]) for t in parts)
    host = torch.cat(parts + [counts.to(torch.int32)], 1).cpu()
    head, code = host[:, :14].contiguous().view(torch.int64).tolist(), host[:, n0:]
    scores = host[:, 14:15].contiguous().view(torch.float32).reshape(B).tolist() if conf is not None else None
    out = []
    for b in range(B):
        c, area, x0, y0, bw, bh, n = head[b]
        if n > cap:
            raise OverflowError(f"image {ids[b]}: the run-length code has {n} counts and was cut at max_runs = {cap}; it needs max_runs >= {n}")
        runs = code[b, :n].tolist()
        rec = {"image_id": ids[b], "category_id": c, "bbox": [x0, y0, bw, bh], "area": area,
               "segmentation": {"size": [H, W], "counts": rle_to_string(runs) if compressed else runs}}
        if scores is not None:
            if scores[b] != scores[b]:
                raise ValueError(f"image {ids[b]}: the score is NaN (a NaN among the head's class logits)")
            rec["score"] = scores[b]
        out.append(rec)
    return out


INT32_MAX = 2 ** 31 - 1


def coco_to_instances(records, device, max_runs=None):
    """instances_to_coco's inverse: a list of COCO / LVIS result records, or of annotation records, as the tensors the library's own
    operations take.  Every record has "image_id", "category_id" and "segmentation" = {"size": [H, W], "counts": ...}, counts a list of
    ints (the uncompressed code) or the compressed string (rle_from_string); "score" in every record or in none.  Returns (image_ids, a
    list; cat (n,) int64; n_runs (n,) int64; counts (n,cap) int32, zero behind each code; sizes (n,2) int64 = (H, W); scores (n,)
    fp32, or None where no record has one), the tensors on `device`, made by ONE host-to-device copy.  cap defaults to the longest code;
    with max_runs (an int >= 1) a longer code is stored cut while n_runs stays its true length, which rle_bits reports as status 1.
    rle_bits(counts[sel], n_runs[sel], (H, W)) decodes the records of one size.  ValueError, naming the record, for a polygon
    segmentation (rasterising polygons is not built), a missing key, a count outside int32, a malformed string, or scores in only some."""
    records = list(records)
    if not records:
        raise ValueError("no records")
    rows, ids, longest = [], [], 1
    with_score = [isinstance(r, dict) and "score" in r for r in records]
    if any(with_score) and not all(with_score):
        raise ValueError(f"record {with_score.index(False)} has no score while others have: scores go with every record or with none")
    for i, r in enumerate(records):
        if not isinstance(r, dict):
            raise ValueError(f"record {i} is no dict")
        for key in ("image_id", "category_id", "segmentation"):
            if key not in r:
                raise ValueError(f"record {i}: the key {key!r} is missing")
        seg = r["segmentation"]
        if not isinstance(seg, dict):
            raise ValueError(f"record {i} (image {r['image_id']!r}): the segmentation is a polygon list, not an RLE dict; polygons are not rasterised here")
        for key in ("size", "counts"):
            if key not in seg:
                raise ValueError(f"record {i} (image {r['image_id']!r}): the segmentation's key {key!r} is missing")
        size, code = seg["size"], seg["counts"]
        if len(size) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 or v > INT32_MAX for v in size):
            raise ValueError(f"record {i} (image {r['image_id']!r}): the size must be two integers >= 1, got {size!r}")
        if isinstance(code, (str, bytes, bytearray)):
            try:
                code = rle_from_string(code)
            except ValueError as e:
                raise ValueError(f"record {i} (image {r['image_id']!r}): {e}") from None
        code = list(code)
        for j, v in enumerate(code):
            if isinstance(v, bool) or not isinstance(v, int) or v < -INT32_MAX - 1 or v > INT32_MAX:
                raise ValueError(f"record {i} (image {r['image_id']!r}): count {j} = {v!r} is no integer within int32")
        c = r["category_id"]
        if isinstance(c, bool) or not isinstance(c, int):
            raise ValueError(f"record {i} (image {r['image_id']!r}): category_id must be an integer, got {c!r}")
        ids.append(r["image_id"])
        rows.append((c, len(code), int(size[0]), int(size[1]), code))
        longest = max(longest, len(code))
    cap = longest if max_runs is None else _max_runs(max_runs, 1)
    n = len(rows)
    head = torch.tensor([row[:4] for row in rows], dtype=torch.int64).reshape(n, 4)
    score = torch.tensor([float(r["score"]) for r in records] if all(with_score) else [0.0] * n, dtype=torch.float32).reshape(n, 1)
    code = torch.zeros(n, cap, dtype=torch.int32)
    for i, row in enumerate(rows):
        m = min(row[1], cap)
        if m:
            code[i, :m] = torch.tensor(row[4][:m], dtype=torch.int32)
    dev = torch.cat([head.view(torch.int32), score.view(torch.int32), code], 1).to(device)            # the one copy
    head = dev[:, :8].reshape(-1).view(torch.int64).reshape(n, 4)                                     # flat first: a row's stride is odd
    scores = dev[:, 8].contiguous().view(torch.float32) if all(with_score) else None
    return ids, head[:, 0].contiguous(), head[:, 1].contiguous(), dev[:, 9:].contiguous(), head[:, 2:4].contiguous(), scores


POLY_SIDE_MAX = 16384                               # fs_poly_bits' cap on a side: coordinate products stay inside int32
POLY_STATUS = {0: "valid", 1: "the image's ring or vertex offsets are out of range or decreasing"}


def polygon_rings(polys):
    """COCO / LVIS polygon lists as the three tables fs_poly_bits takes (host).  polys: a list with one entry per image, each entry a
    polygon list [[x0, y0, x1, y1, ...], ...] as an annotation's "segmentation" carries it; an empty polygon list is allowed and is
    the empty mask.  Returns CPU tensors (verts (V,2) int32 = (y, x); ring_off (R+1,) int32: ring r owns verts[ring_off[r] :
    ring_off[r+1]]; img_ring (B+1,) int32: image b owns the rings img_ring[b] : img_ring[b+1]).  The coordinates are rounded half to
    even on float64 (np.round, as the reference's b2_preprocess_lvis.py:282-297 does) and NOT clipped: poly_bits clamps them onto
    the frame.  ValueError, naming the image and the ring, for an entry that is not a list of lists, a ring of odd or zero length, a
    coordinate that is no number or not finite, and a rounded value outside int32."""
    import numpy as np
    if not isinstance(polys, (list, tuple)):
        raise ValueError(f"polys must be a list with one polygon list per image, got {type(polys).__name__}")
    rows, ring_off, img_ring = [], [0], [0]
    for b, entry in enumerate(polys):
        if not isinstance(entry, (list, tuple)) or any(not isinstance(ring, (list, tuple)) for ring in entry):
            raise ValueError(f"image {b}: the segmentation must be a polygon list, a list of lists [x0, y0, x1, y1, ...]")
        for j, ring in enumerate(entry):
            if len(ring) == 0 or len(ring) % 2:
                raise ValueError(f"image {b}, ring {j}: a ring is x, y pairs; it has {len(ring)} numbers")
            for k, v in enumerate(ring):
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise ValueError(f"image {b}, ring {j}: coordinate {k} = {v!r} is no number")
            try:
                xy = np.round(np.array([float(v) for v in ring], dtype=np.float64))
            except OverflowError:
                raise ValueError(f"image {b}, ring {j}: a coordinate is outside float64") from None
            if not np.isfinite(xy).all():
                raise ValueError(f"image {b}, ring {j}: coordinate {int(np.flatnonzero(~np.isfinite(xy))[0])} is not finite")
            if (xy < -INT32_MAX - 1).any() or (xy > INT32_MAX).any():
                raise ValueError(f"image {b}, ring {j}: a rounded coordinate is outside int32")
            rows.append(xy.reshape(-1, 2)[:, ::-1].astype(np.int32))                  # (x, y) pairs -> (y, x)
            ring_off.append(ring_off[-1] + len(ring) // 2)
        img_ring.append(len(ring_off) - 1)
    if ring_off[-1] > INT32_MAX:
        raise ValueError(f"{ring_off[-1]} vertices are more than int32 offsets hold")
    verts = np.concatenate(rows, 0) if rows else np.zeros((0, 2), dtype=np.int32)
    return (torch.from_numpy(np.ascontiguousarray(verts)), torch.tensor(ring_off, dtype=torch.int32), torch.tensor(img_ring, dtype=torch.int32))


def _poly_args(verts, ring_off, img_ring, size):
    """(B, R, V, Hs, Ws) of poly_bits' arguments, or ValueError: the checks of the host, nothing launched."""
    for name, t, ok in (("verts", verts, lambda t: t.dim() == 2 and t.shape[1] == 2), ("ring_off", ring_off, lambda t: t.dim() == 1 and t.numel() >= 1),
                        ("img_ring", img_ring, lambda t: t.dim() == 1 and t.numel() >= 2)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not ok(t):
            raise ValueError(f"{name} must be an int32 tensor -- verts (V, 2), ring_off (R + 1,), img_ring (B + 1,), B >= 1 -- got "
                             f"{getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))}")
    if not (verts.device == ring_off.device == img_ring.device):
        raise ValueError("verts, ring_off and img_ring must be on one device")
    if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 or int(v) > POLY_SIDE_MAX for v in size):
        raise ValueError(f"size must be two integers 1 .. {POLY_SIDE_MAX} (Hs, Ws), got {size!r}")
    return int(img_ring.numel()) - 1, int(ring_off.numel()) - 1, int(verts.shape[0]), int(size[0]), int(size[1])


def poly_bits(verts, ring_off, img_ring, size, device=None, check=False):
    """Polygon lists as bit words, on the device (fs_poly_bits; no autograd).  verts, ring_off, img_ring as polygon_rings makes them
    (int32; (y, x) vertices rounded but not clipped), size = (Hs, Ws), each side at most 16384.  Tables on the host go to `device`
    (default "cuda") in ONE host-to-device copy; tables already on a device are used where they lie.  UNPINNED -- the reference makes
    its labels with np.round, a clip onto the frame and skimage.draw.polygon (b2_preprocess_lvis.py:282-297), which is not at hand, so
    the rule is this library's restatement of what that is understood to give for integer vertices, not verified against it: a vertex
    is clamped to the frame; a ring is the closed chain of a polygon's vertices; it sets pixel (y, x) iff the pixel lies on one of its
    edges (end points included) or the even-odd crossing number is odd (edges oriented so that y0 < y1, y0 <= y < y1, counted where
    (x - x0)(y1 - y0) < (y - y0)(x1 - x0)); an image's mask is the OR of its rings, so overlapping polygons do not cancel while a
    self-intersecting ring follows even-odd.  It is not pycocotools' frPoly, which traces a 5x upsampled outline and differs along the
    rim.  Returns (bits (B,Hs,ceil(Ws/32)) int32 in mask_bits' layout, the bits at x >= Ws 0; info (B,4) int64 = (status, area,
    n_rings, n_vertices)): status 0 valid, 1 the image's offsets are out of range or decreasing (all-zero words, area 0); an image
    without rings is the empty mask.  No host read -- unless check=True, which reads info once and raises ValueError naming the first
    image whose status is not 0.  mask_rle(bits, Ws) gives the label evaluate_instances(seg_label=(counts, stats)) takes."""
    B, R, V, Hs, Ws = _poly_args(verts, ring_off, img_ring, size)
    if verts.device.type == "cpu":
        dev = torch.device("cuda" if device is None else device)
        keep = torch.cat([img_ring, ring_off, verts.reshape(-1)]).to(dev)              # the one copy
        p_img = hip.ptr(keep)
        p_ring, p_verts = p_img + 4 * (B + 1), p_img + 4 * (B + 1 + R + 1)             # the buffer's end where V = 0: never read
    else:
        dev = verts.device
        if device is not None and torch.device(device) != dev:
            raise ValueError(f"the tables are on {dev}, not on {device}")
        keep = (verts.contiguous(), ring_off.contiguous(), img_ring.contiguous())
        p_ring, p_img = hip.ptr(keep[1]), hip.ptr(keep[2])
        p_verts = hip.ptr(keep[0]) if V else p_ring
    bits = torch.empty(B, Hs, (Ws + 31) // 32, device=dev, dtype=torch.int32)
    info = torch.empty(B, 4, device=dev, dtype=torch.int64)
    scratch = torch.empty(max(1, hip.query("fs_poly_bits_scratch_ints", B, Hs, Ws)), device=dev, dtype=torch.int32)
    hip.call("fs_poly_bits", p_verts, p_ring, p_img, hip.ptr(bits), hip.ptr(info), hip.ptr(scratch), B, R, V, Hs, Ws)
    del keep                                                                           # the tables, held until the launch is queued
    if check:
        for b, st in enumerate(info[:, 0].cpu().tolist()):
            if st != 0:
                raise ValueError(f"image {b}: {POLY_STATUS[st]} (status {st}; {R} rings, {V} vertices)")
    return bits, info


def coco_masks(records, size, device):
    """COCO / LVIS records of ONE size as bit words, whichever way each carries its mask: "segmentation" an RLE dict (counts a list or
    the compressed string) or a polygon list.  size = (H, W); records as coco_to_instances takes them ("image_id", "category_id",
    "segmentation"; "score" in every record or in none).  Returns (image_ids, a list; cat (n,) int64; bits (n,H,ceil(W/32)) int32;
    info (n,2) int64 = (status, area); scores (n,) fp32 or None), the rows in record order.  RLE rows go through coco_to_instances and
    rle_bits, polygon rows through polygon_rings and poly_bits (unpinned rules both; see there): each kind is handed all n rows, the
    other kind's rows as empty masks, and the two results are ORed, so the order needs no index on the device.  At most two
    host-to-device copies (one a kind) and no host read: a code or offsets that are not valid give an empty mask and a status that is
    not 0 (rle_bits' for an RLE row, poly_bits' for a polygon row).  ValueError as coco_to_instances and polygon_rings raise it (the
    latter's "image i" is record i), and for an RLE record whose size is not `size`."""
    records = list(records)
    if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in size):
        raise ValueError(f"size must be two integers >= 1 (H, W), got {size!r}")
    H, W = int(size[0]), int(size[1])
    empty = {"size": [H, W], "counts": [H * W]}
    as_rle, polys, n_poly = [], [], 0
    for i, r in enumerate(records):
        seg = r.get("segmentation") if isinstance(r, dict) else None
        if isinstance(seg, (list, tuple)):
            as_rle.append(dict(r, segmentation=empty))
            polys.append(seg)
            n_poly += 1
        else:
            if isinstance(seg, dict) and "size" in seg and list(seg["size"]) != [H, W]:
                raise ValueError(f"record {i} (image {r.get('image_id')!r}): the code's size {seg['size']!r} is not {[H, W]}")
            as_rle.append(r)
            polys.append([])
    ids, cat, n_runs, counts, _sizes, scores = coco_to_instances(as_rle, device)
    bits = info = None
    if n_poly < len(records):
        bits, info4 = rle_bits(counts, n_runs, (H, W))
        info = info4[:, :2]
    if n_poly:
        pbits, pinfo = poly_bits(*polygon_rings(polys), (H, W), device=device)
        bits, info = (pbits, pinfo[:, :2]) if bits is None else (bits | pbits, info + pinfo[:, :2])
    return ids, cat, bits, info.contiguous(), scores


def _candidate_args(cbits, cand_off, Ws, cand_cat):
    """(N, Hs, P, B) of mask_candidates' tables, or ValueError: the checks of the host, nothing launched."""
    if not isinstance(cbits, torch.Tensor) or cbits.dtype != torch.int32 or cbits.dim() != 3 or Ws is None or isinstance(Ws, bool) \
            or int(Ws) != Ws or int(Ws) < 1 or cbits.shape[2] != (int(Ws) + 31) // 32 or cbits.shape[1] < 1:
        raise ValueError(f"cbits must be int32 bit words (N, Hs, ceil(Ws / 32)) with Hs >= 1 and Ws given, got "
                         f"{getattr(cbits, 'dtype', None)} {tuple(getattr(cbits, 'shape', ()))} and Ws = {Ws!r}")
    N, Hs, P = (int(v) for v in cbits.shape)
    if not isinstance(cand_off, torch.Tensor) or cand_off.dtype != torch.int32 or cand_off.dim() != 1 or cand_off.numel() < 2:
        raise ValueError(f"cand_off must be an int32 tensor (B + 1,), B >= 1, got {getattr(cand_off, 'dtype', None)} "
                         f"{tuple(getattr(cand_off, 'shape', ()))}")
    if cand_cat is not None and (not isinstance(cand_cat, torch.Tensor) or cand_cat.dtype != torch.int64 or tuple(cand_cat.shape) != (N,)):
        raise ValueError(f"cand_cat must be int64 ({N},), got {getattr(cand_cat, 'dtype', None)} {tuple(getattr(cand_cat, 'shape', ()))}")
    for name, t in (("cand_off", cand_off), ("cand_cat", cand_cat)):
        if t is not None and t.device != cbits.device:
            raise ValueError(f"{name} is on {t.device}, cbits on {cbits.device}")
    if Hs > POLY_SIDE_MAX or int(Ws) > POLY_SIDE_MAX:
        raise ValueError(f"a side of {(Hs, int(Ws))} is above {POLY_SIDE_MAX}")
    return N, Hs, P, int(cand_off.numel()) - 1


def mask_candidates(cbits, cand_off, focus, Ws, pred=None, cand_cat=None, snap_px=None):
    """Of every image's annotated instances, the one under the gaze, on the device and on bit words (fs_mask_candidates; no autograd).
    UNPINNED: the reference builds its labels by choosing an annotation and putting the gaze inside it
    (b2_preprocess_lvis.py:258-333); this is the inverse of that step and a definition of this library's.  cbits (N,Hs,ceil(Ws/32))
    int32, the candidates' masks in mask_bits' layout (N = 0 allowed; the bits at x >= Ws are not read); cand_off (B+1,) int32: image
    b owns the rows cand_off[b] : cand_off[b+1]; focus (B,2) normalised (row, col), turned into a gaze pixel as mask_component does;
    pred (B,Hs,ceil(Ws/32)) int32 or None, a prediction's bit words per image; cand_cat (N,) int64 or None; snap_px None (any
    distance) or a finite number of pixels >= 0, snap2 = floor(snap_px ** 2) (as mask_component).  Returns (gbits, sel, cand):

    cand (N,6) int64 = (b, area, inter, d2, near_y, near_x): the row's image, its set pixels, |c & pred[b]| (0 without pred), and its
    set pixel nearest to the gaze pixel with the squared distance (ties to the smaller row-major index; -1, -1, -1 for an empty row).
    sel (B,8) int64 = (index, cls, d2, area, inter, n_hit, best, status).  index: the SELECTED row -- among the image's rows with area >
    0 and d2 <= snap2 the least (d2, area, row): of several instances that contain the gaze pixel the smallest (a cup on a table gives
    the cup), of none the nearest within the snap distance, ties to the smaller area, then row -- or -1; cls = cand_cat[index] (-1
    for none or without cand_cat); d2, area, inter the selected row's (-1, 0, 0); n_hit how many of the image's rows contain the gaze
    pixel; best: among rows with inter > 0 the one of the greatest IoU with pred[b], compared exactly in integers, ties to the smaller
    area, then row, or -1.  gbits (B,Hs,ceil(Ws/32)) int32 = the selected row's words with the bits at x >= Ws cleared, all 0 where
    none is selected.  status 1 in every image where cand_off is not 0 = cand_off[0] <= ... <= cand_off[B] = N: then nothing is
    selected anywhere and every cand row is (-1, area, 0, -1, -1, -1).  No host read; the same bits in every run."""
    _conn, snap2 = _component_args(8, snap_px)
    N, Hs, P, B = _candidate_args(cbits, cand_off, Ws, cand_cat)
    Ws, dev = int(Ws), cbits.device
    f = _focus_arg(focus, B, dev)
    if pred is not None and (not isinstance(pred, torch.Tensor) or pred.dtype != torch.int32 or tuple(pred.shape) != (B, Hs, P) or pred.device != dev):
        raise ValueError(f"pred must be int32 bit words {(B, Hs, P)} on {dev}, got {getattr(pred, 'dtype', None)} {tuple(getattr(pred, 'shape', ()))}")
    gbits = torch.empty(B, Hs, P, device=dev, dtype=torch.int32)
    sel = torch.empty(B, 8, device=dev, dtype=torch.int64)
    cand = torch.empty(N, 6, device=dev, dtype=torch.int64)
    scratch = torch.empty(max(1, hip.query("fs_mask_candidates_scratch_ints", B, N, Hs, Ws)), device=dev, dtype=torch.int32)
    hip.call("fs_mask_candidates", hip.ptr(cbits.contiguous()) if N else None, hip.ptr(cand_off.contiguous()),
             None if cand_cat is None or N == 0 else hip.ptr(cand_cat.contiguous()), hip.ptr(f),
             None if pred is None else hip.ptr(pred.contiguous()), hip.ptr(cand) if N else None, hip.ptr(sel), hip.ptr(gbits),
             hip.ptr(scratch), B, N, Hs, Ws, snap2)
    return gbits, sel, cand


def coco_candidates(records, size, device, image_ids):
    """COCO / LVIS annotation records of ONE size, several an image, as mask_candidates' arguments.  records as coco_masks takes them
    (RLE dicts or polygon lists, mixed); size = (H, W); image_ids the images in the order the batch has them.  The records are grouped
    stably by "image_id" in the order of image_ids -- an id without records gets an empty range -- and rasterised through coco_masks
    with its copies (at most two) plus one for the offsets.  Returns (cbits (N,H,ceil(W/32)) int32; cand_off (B+1,) int32; cand_cat
    (N,) int64; info (N,2) int64 = coco_masks' (status, area); rows, a list: rows[i] is the index into `records` of candidate row i,
    which maps mask_candidates' sel[:, 0] back to an annotation: records[rows[index]]["id"]).  "iscrowd" is not interpreted: a
    crowd record is a candidate like any other.  ValueError for a record whose image is not in image_ids, an id named twice, and as
    coco_masks."""
    records, image_ids = list(records), list(image_ids)
    if not image_ids:
        raise ValueError("no image_ids")
    place = {}
    for b, image_id in enumerate(image_ids):
        if image_id in place:
            raise ValueError(f"image_ids names {image_id!r} twice")
        place[image_id] = b
    per = [[] for _ in image_ids]
    for i, r in enumerate(records):
        if not isinstance(r, dict) or "image_id" not in r:
            raise ValueError(f"record {i}: the key 'image_id' is missing")
        if r["image_id"] not in place:
            raise ValueError(f"record {i}: image {r['image_id']!r} is not among image_ids")
        per[place[r["image_id"]]].append(i)
    rows = [i for group in per for i in group]
    off = [0]
    for group in per:
        off.append(off[-1] + len(group))
    if len(size) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in size):
        raise ValueError(f"size must be two integers >= 1 (H, W), got {size!r}")
    dev = torch.device(device)
    H, W = int(size[0]), int(size[1])
    cand_off = torch.tensor(off, dtype=torch.int32).to(dev)
    if not rows:
        return (torch.empty(0, H, (W + 31) // 32, device=dev, dtype=torch.int32), cand_off, torch.empty(0, device=dev, dtype=torch.int64),
                torch.empty(0, 2, device=dev, dtype=torch.int64), rows)
    _ids, cat, cbits, info, _scores = coco_masks([{k: v for k, v in records[i].items() if k != "score"} for i in rows], size, dev)
    return cbits, cand_off, cat, info, rows
