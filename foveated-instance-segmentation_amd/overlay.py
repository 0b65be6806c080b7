"""Showing the record: the overlay pass (csrc/frame_overlay.hip), its style table and outline band, and the class map as colours.
Stateless, no autograd.
"""
import torch

from . import hip
from .frames import _FRAME_TYPES, Nv12Frame, _dest_args, _frame_args, _frame_route, byte_frame_dest, byte_frame_layout
from .masks import _focus_arg, _morph_d

__all__ = [
    "OVERLAY_STYLE_COLS", "OVERLAY_MAX_PX", "overlay_style", "overlay_band", "draw_instances", "color_encode",
]


OVERLAY_STYLE_COLS = 20                             # ints a style row (include/fovealseg.h "showing the record")
OVERLAY_MAX_PX = 16384                              # the kernel's cap on t, r, w and on a side


def _overlay_colour(name, v):
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 3:
        raise ValueError(f"{name} must be three integers (r, g, b) in 0 .. 255, got {v!r}")
    out = []
    for c in v:
        if isinstance(c, bool) or int(c) != c or not 0 <= int(c) <= 255:
            raise ValueError(f"{name} must be three integers (r, g, b) in 0 .. 255, got {v!r}")
        out.append(int(c))
    return out


def _overlay_int(name, v, hi):
    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer 0 .. {hi}, got {v!r}")
    return int(v)


def _int_ge_zero(name, v):
    if isinstance(v, bool) or int(v) != v or int(v) < 0:
        raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
    return int(v)


def overlay_style(tint=(0, 255, 0), alpha=128, outline=None, box=None, box_px=2, marker=None, marker_px=6, marker_width=None, dim=256,
                  cat=None, palette=None, device=None):
    """The style table of draw_instances / fs_frame_overlay: (S, 20) int32 on `device`, columns tint r g b, a, outline r g b, dim, box r g b,
    t, marker r g b, r, w, the outline flag, two reserved.  tint, and outline / box / marker where given, are (r, g, b) integers 0 .. 255;
    None switches the element off (its colour columns stay 0, and t, r or the flag 0).  alpha and dim are integers 0 .. 256: a mask pixel
    becomes (s * (256 - alpha) + tint * alpha + 128) >> 8, any other (s * dim + 128) >> 8.  box_px = t, the box's line width inward;
    marker_px = r, the gaze marker's radius, marker_width = w its ring width (None: a disc); all 0 .. 16384.  One row, for every viewer,
    unless cat (B,) int64 and palette (K,3) uint8 are given: then S = B and viewer b's tint is palette[cat[b]] (the given tint for a class
    outside the palette), looked up on cat's device without a host read.  ValueError for anything else."""
    row = [0] * OVERLAY_STYLE_COLS
    row[0:3] = _overlay_colour("tint", tint)
    row[3] = _overlay_int("alpha", alpha, 256)
    row[7] = _overlay_int("dim", dim, 256)
    if outline is not None:
        row[4:7] = _overlay_colour("outline", outline)
        row[17] = 1
    if box is not None:
        row[8:11] = _overlay_colour("box", box)
        row[11] = _overlay_int("box_px", box_px, OVERLAY_MAX_PX)
    if marker is not None:
        row[12:15] = _overlay_colour("marker", marker)
        row[15] = _overlay_int("marker_px", marker_px, OVERLAY_MAX_PX)
        row[16] = row[15] if marker_width is None else _overlay_int("marker_width", marker_width, OVERLAY_MAX_PX)
    if (cat is None) != (palette is None):
        raise ValueError("cat and palette go together: a tint a viewer by class needs both")
    if cat is None:
        return torch.tensor([row], dtype=torch.int32, device=device)
    if not isinstance(cat, torch.Tensor) or cat.dim() != 1 or cat.dtype != torch.int64 or cat.numel() == 0:
        raise ValueError(f"cat must be a non-empty int64 (B,), got {getattr(cat, 'dtype', None)} {tuple(getattr(cat, 'shape', ()))}")
    pal = torch.as_tensor(palette)
    if pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < 1 or pal.dtype != torch.uint8:
        raise ValueError(f"palette must be uint8 (K, 3), got {pal.dtype} {tuple(pal.shape)}")
    dev = cat.device if device is None else torch.device(device)
    cat, pal = cat.to(dev), pal.to(dev)
    K = int(pal.shape[0])
    style = torch.tensor([row], dtype=torch.int32, device=dev).repeat(int(cat.shape[0]), 1)
    inside = (cat >= 0) & (cat < K)
    looked = pal[cat.clamp(0, K - 1)].to(torch.int32)
    style[:, 0:3] = torch.where(inside[:, None], looked, style[:, 0:3])
    return style


def overlay_band(bits, Ws, d, er=None, scratch=None, band=None):
    """The outline band of draw_instances: bits & ~E_d(bits), E_d fs_mask_erode's, with no host read.  er, band (like bits) and scratch
    (fs_mask_erode_scratch_ints int32) are made where not given; the bits at x >= Ws of the band are unspecified (the overlay pass reads
    none of them).  Returns (band, er, scratch)."""
    d = _morph_d(d)
    B, Hs = int(bits.shape[0]), int(bits.shape[1])
    if er is None:
        er = torch.empty_like(bits, memory_format=torch.contiguous_format)
    if band is None:
        band = torch.empty_like(bits, memory_format=torch.contiguous_format)
    if scratch is None:
        scratch = torch.empty(max(1, hip.query("fs_mask_erode_scratch_ints", B, Hs, Ws, d)), device=bits.device, dtype=torch.int32)
    hip.call("fs_mask_erode", hip.ptr(bits), hip.ptr(er), hip.ptr(scratch), B, Hs, Ws, d)
    torch.bitwise_not(er, out=er)
    torch.bitwise_and(bits, er, out=band)
    return band, er, scratch


def _live_arg(live, B, dev):
    """(pointer, stride in elements) of the nullable live flags: an int64 (B,) tensor on the device, contiguous or a column of a matrix."""
    if live is None:
        return None, 1
    if not isinstance(live, torch.Tensor) or live.dtype != torch.int64 or tuple(live.shape) != (B,) or live.device != dev:
        raise ValueError(f"live must be int64 ({B},) on {dev}, got {getattr(live, 'dtype', None)} {tuple(getattr(live, 'shape', ()))}")
    stride = int(live.stride(0)) if B > 1 else 1
    if stride < 1:
        raise ValueError(f"live must have a positive stride, got {stride}")
    return live.data_ptr(), stride


def draw_instances(img, bits, stats=None, focus=None, style=None, outline_px=0, out=None, live=None, band=None):
    """The record drawn onto the frame, in one launch (fs_frame_overlay / _u8 / _hwc; no autograd; unpinned: the reference draws on the
    host).  img (B,3,H,W) as the serving entry points take it, on the device: fp32 (its pixel code q(v) = rint(clamp(v, 0, 1) * 255) is what
    is drawn on), contiguous uint8, or a uint8 view of interleaved bytes (byte_frame_layout), read where it lies; any other layout is
    copied.  bits (B,H,ceil(W/32)) int32, the record's mask; stats (B,6) int64, the record's, for the box; focus (B,2), for the gaze
    marker; a None switches its element off.  style: overlay_style's table, (1,20) or (B,20) int32 (None: its defaults).  outline_px = d >
    0 makes the outline band bits & ~E_d(bits) first (fs_mask_erode; no host read) unless `band` brings it; the style's outline colour
    shows it.  live: None, or int64 (B,) flags (a column of a matrix will do): where 0, the viewer's mask, outline and box count as empty.
    out: a uint8 (B,3,H,W) tensor to write, contiguous or an interleaved view (byte_frame_dest: an RGBA view gets alpha 255); None: a new
    contiguous one.  out may be img itself for a frame of bytes.  The rule per pixel, first that holds: marker, box, outline, tint, dim
    (include/fovealseg.h).  Returns out."""
    if not isinstance(img, _FRAME_TYPES) or img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0 or img.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"img must be a non-empty fp32 or uint8 (B,3,H,W), got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))}")
    B, _, H, W = (int(v) for v in img.shape)
    if max(H, W) > OVERLAY_MAX_PX:
        raise ValueError(f"a frame of {H} x {W} pixels has a side above {OVERLAY_MAX_PX}")
    dev = img.device
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or tuple(bits.shape) != (B, H, (W + 31) // 32):
        raise ValueError(f"bits must be int32 {(B, H, (W + 31) // 32)}, got {getattr(bits, 'dtype', None)} {tuple(getattr(bits, 'shape', ()))}")
    if stats is not None and (stats.dtype != torch.int64 or tuple(stats.shape) != (B, 6)):
        raise ValueError(f"stats must be int64 ({B}, 6), got {stats.dtype} {tuple(stats.shape)}")
    if style is None:
        style = overlay_style(device=dev)
    if not isinstance(style, torch.Tensor) or style.dtype != torch.int32 or style.dim() != 2 or style.shape[1] != OVERLAY_STYLE_COLS or \
            int(style.shape[0]) not in (1, B):
        raise ValueError(f"style must be int32 (1, {OVERLAY_STYLE_COLS}) or ({B}, {OVERLAY_STYLE_COLS}) (ops.overlay_style), got "
                         f"{getattr(style, 'dtype', None)} {tuple(getattr(style, 'shape', ()))}")
    f = None if focus is None else _focus_arg(focus, B, dev)
    live_ptr, live_stride = _live_arg(live, B, dev)
    outline_px = _int_ge_zero("outline_px", outline_px)
    if isinstance(img, Nv12Frame):
        pass                                            # read where it lies
    elif img.dtype == torch.uint8 and byte_frame_layout(img) is None or img.dtype == torch.float32 and not img.is_contiguous():
        img = img.contiguous()
    if out is None:
        out = torch.empty(B, 3, H, W, device=dev, dtype=torch.uint8)
    dest = byte_frame_dest(out, (B, 3, H, W))
    bits = bits.contiguous()
    if band is None and int(outline_px) > 0:
        band = overlay_band(bits, W, int(outline_px))[0]
    elif band is not None and (band.dtype != torch.int32 or band.shape != bits.shape):
        raise ValueError(f"band must be int32 {tuple(bits.shape)}, got {band.dtype} {tuple(band.shape)}")
    suffix, strides = _frame_route(img)
    hip.call("fs_frame_overlay" + suffix, *_frame_args(img, strides), hip.ptr(bits), hip.ptr(band), hip.ptr(stats if stats is None else stats.contiguous()),
             hip.ptr(f), live_ptr, live_stride, hip.ptr(style.contiguous()), int(style.shape[0]), *_dest_args(out, dest), B, H, W)
    return out


def color_encode(labels, palette, out=None):
    """A class map as colours (fs_color_encode; utils.py:207-221 colorEncode, mode RGB, on the device): labels (B,H,W) or (H,W) int64,
    predict()'s map; palette (K,3) uint8.  out (B,3,H,W) uint8 as draw_instances takes it (None: a new contiguous one) = palette[label],
    (0, 0, 0) for a label < 0 or >= K -- the reference skips negative labels and would raise on one >= K.  Returns out."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() not in (2, 3) or labels.numel() == 0:
        raise ValueError(f"labels must be a non-empty int64 (B,H,W) or (H,W), got {getattr(labels, 'dtype', None)} {tuple(getattr(labels, 'shape', ()))}")
    if labels.dim() == 2:
        labels = labels[None]
    B, H, W = (int(v) for v in labels.shape)
    if max(H, W) > OVERLAY_MAX_PX:
        raise ValueError(f"a map of {H} x {W} pixels has a side above {OVERLAY_MAX_PX}")
    pal = torch.as_tensor(palette)
    if pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < 1 or pal.dtype != torch.uint8:
        raise ValueError(f"palette must be uint8 (K, 3), got {pal.dtype} {tuple(pal.shape)}")
    pal = pal.to(labels.device).contiguous()
    if out is None:
        out = torch.empty(B, 3, H, W, device=labels.device, dtype=torch.uint8)
    dest = byte_frame_dest(out, (B, 3, H, W))
    hip.call("fs_color_encode", hip.ptr(labels.contiguous()), hip.ptr(pal), *_dest_args(out, dest), B, H, W, int(pal.shape[0]))
    return out
