"""Frames as the serving entry points take them: fp32, planar or interleaved bytes, NV12 planes (csrc/frame_view.h).

Describes how a frame lies in memory and hands the kernels its leading arguments (`_frame_route`, `_frame_args`); stateless, no
autograd.  Imports none of the package's other op modules.
"""
import operator

import torch

from . import hip

__all__ = [
    "byte_frame_strides", "byte_frame_layout", "NV12_MATRICES", "NV12_COEF_MAX", "nv12_csc", "nv12_frame_strides", "Nv12Frame",
    "nv12_from_surface", "nv12_to_rgb", "byte_frame_select", "frame_in_place", "byte_frame_dest",
]


def byte_frame_strides(shape, strides):
    """byte_frame_layout's rule as a pure function of a (B,3,H,W) shape and its element strides (sb, sc, sy, sx); strides of dimensions
    of size 1 are ignored.  ("planar",) for a contiguous tensor; ("hwc", sb, sy, sx) for interleaved bytes -- sc == 1, sx in {3, 4}, sy
    >= W * sx, and sb == 0 (every viewer sees the one frame), sb >= H * sy or B == 1; None for anything else.  In the hwc tuple the
    ignored strides are normalised: sb = 0 for B == 1, sy = W * sx for H == 1, sx = 3 for W == 1."""
    B, C, H, W = (int(v) for v in shape)
    sb, sc, sy, sx = (int(v) for v in strides)
    if C != 3 or min(B, H, W) < 1:
        return None
    if (W == 1 or sx == 1) and (H == 1 or sy == W) and (sc == H * W) and (B == 1 or sb == 3 * H * W):
        return ("planar",)
    if sc != 1:
        return None
    if W == 1:
        sx = 3
    if sx not in (3, 4):
        return None
    if H == 1:
        sy = W * sx
    if sy < W * sx:
        return None
    if B == 1:
        sb = 0
    if sb != 0 and sb < H * sy:
        return None
    return ("hwc", sb, sy, sx)


def byte_frame_layout(img):
    """How a uint8 frame (B,3,H,W) lies in memory, from its strides alone: ("planar",) when it is contiguous (the fs_*_u8 route);
    ("hwc", sb, sy, sx) when it is a view of interleaved bytes, the byte of channel c at (b, y, x) being byte b * sb + y * sy + x * sx + c
    from img.data_ptr() (the fs_*_hwc route: nothing is copied); None for anything else.  An hwc view is what a camera's or a decoder's
    (B,H,W,3) or (B,H,W,4) buffer is after permute(0, 3, 1, 2) (and [:, :3] for RGBA / RGBX, whose fourth byte is never used): tight or
    with padded rows, a crop of a larger buffer, x.contiguous(memory_format=torch.channels_last), or one frame expanded over the batch
    (sb == 0).  The channel order is the tensor's own.  The kernels read whole pixels, so the W * sx bytes of the last row must lie inside
    the tensor's storage (an RGBA view's last alpha byte: true of every view of a real (B,H,W,4) buffer); a view that ends short is None."""
    if not isinstance(img, torch.Tensor) or img.dim() != 4 or img.dtype != torch.uint8 or img.shape[1] != 3 or img.numel() == 0:
        return None
    if img.is_contiguous():
        return ("planar",)
    layout = byte_frame_strides(img.shape, img.stride())
    if layout is not None and layout[0] == "hwc":
        _, sb, sy, sx = layout
        if img.storage_offset() + (img.shape[0] - 1) * sb + (img.shape[2] - 1) * sy + img.shape[3] * sx > img.untyped_storage().nbytes():
            return None
    return layout


def _byte_frame(img, what="img"):
    """("planar",) or ("hwc", ...) of a uint8 frame the *_u8 functions take; ValueError for any other layout, before any launch."""
    layout = byte_frame_layout(img)
    if layout is None:
        raise ValueError(f"{what} must be a contiguous uint8 (B,3,H,W) or a view of interleaved (B,H,W,3) / (B,H,W,4) bytes "
                         f"(ops.byte_frame_layout), got {getattr(img, 'dtype', None)} {tuple(getattr(img, 'shape', ()))} with strides "
                         f"{tuple(img.stride()) if isinstance(img, torch.Tensor) else None}; call .contiguous() on it")
    return layout


NV12_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}          # (Kr, Kb)
NV12_COEF_MAX = 32768


def nv12_csc(matrix, full_range=False):
    """The integer colour table (yo, yg, rv, gu, gv, bu) of an NV12 frame (include/fovealseg.h "frames as NV12"): rint(256 * real
    coefficient) from the matrix's (Kr, Kb); the luma gain is 255 / 219 and the chroma gain 255 / 224 for limited range (yo = 16), both 1
    for full range (yo = 0).  matrix: "bt601" or "bt709"."""
    if matrix not in NV12_MATRICES:
        raise ValueError(f"matrix must be one of {sorted(NV12_MATRICES)}, got {matrix!r}")
    kr, kb = NV12_MATRICES[matrix]
    kg = 1.0 - kr - kb
    ly, lc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    real = (ly, lc * 2 * (1 - kr), -lc * 2 * (1 - kb) * kb / kg, -lc * 2 * (1 - kr) * kr / kg, lc * 2 * (1 - kb))
    return (0 if full_range else 16,) + tuple(int(round(256.0 * v)) for v in real)


def _nv12_table(csc):
    try:
        t = tuple(operator.index(v) for v in csc)
    except TypeError:
        t = ()
    if len(t) != 6 or any(isinstance(v, bool) for v in csc):
        raise ValueError(f"csc must be six integers (yo, yg, rv, gu, gv, bu), got {csc!r}")
    if not 0 <= t[0] <= 255 or any(abs(v) > NV12_COEF_MAX for v in t[1:]):
        raise ValueError(f"csc wants 0 <= yo <= 255 and every coefficient in [-{NV12_COEF_MAX}, {NV12_COEF_MAX}], got {t}")
    return t


def nv12_frame_strides(y_shape, y_strides, uv_shape, uv_strides):
    """(sb, sy, ub, uy) of an NV12 frame from the shapes and strides of its two views alone, or None: y (B,H,W) with unit column stride
    and rows sy >= W apart, uv (B,ceil(H/2),ceil(W/2),2) with strides (ub, uy, 2, 1) and rows uy >= 2 * ceil(W/2) apart; images that do
    not overlap (sb >= H * sy, ub >= ceil(H/2) * uy) or are all one image (sb = ub = 0).  The strides of a dimension of one element are
    normalised: sb = ub = 0 for B == 1, sy = W for H == 1, uy = 2 * ceil(W/2) for one chroma row."""
    if len(y_shape) != 3 or len(uv_shape) != 4:
        return None
    B, H, W = (int(v) for v in y_shape)
    if min(B, H, W) < 1:
        return None
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    if tuple(int(v) for v in uv_shape) != (B, Hc, Wc, 2):
        return None
    sb, sy, sx = (int(v) for v in y_strides)
    ub, uy, ux, uc = (int(v) for v in uv_strides)
    if (W > 1 and sx != 1) or uc != 1 or (Wc > 1 and ux != 2):
        return None
    if H == 1:
        sy = W
    if Hc == 1:
        uy = 2 * Wc
    if B == 1:
        sb = ub = 0
    if sy < W or uy < 2 * Wc or sb < 0 or ub < 0:
        return None
    if not (sb == 0 and ub == 0) and (sb < H * sy or ub < Hc * uy):
        return None
    return sb, sy, ub, uy


class Nv12Frame:
    """An NV12 frame of B images of H x W pixels where a decoder or a camera left it (include/fovealseg.h "frames as NV12"; unpinned):
    y (B,H,W) uint8, the luma plane, a device tensor or view with unit column stride; uv (B,ceil(H/2),ceil(W/2),2) uint8, the interleaved
    chroma plane, a view with strides (ub, uy, 2, 1).  Two allocations, or two views of one surface (nv12_from_surface).  matrix: "bt601"
    or "bt709", with full_range -- it has no default: a silent wrong colour matrix is worse than a required keyword; csc: a table of the
    caller's own (yo, yg, rv, gu, gv, bu) instead (nv12_csc's rule; matrix is then only a label and may be None).

    predict*, evaluate*, GazeSession.step / render and the ops that take a uint8 frame take this object in its place, and give what they
    give on the planar uint8 frame nv12_to_rgb(frame), bit for bit; the frame is read where it lies and never written.  It shows
    shape == (B,3,H,W), dtype == torch.uint8, device and is_cuda as that frame would.  ValueError for any other dtypes, shapes or
    strides, views on different devices, bytes the kernels may read outside the tensors' storage, or a table out of range."""

    def __init__(self, y, uv, *, matrix, full_range=False, csc=None):
        if not isinstance(y, torch.Tensor) or not isinstance(uv, torch.Tensor) or y.dtype != torch.uint8 or uv.dtype != torch.uint8:
            raise ValueError(f"y and uv must be uint8 tensors, got {getattr(y, 'dtype', None)} and {getattr(uv, 'dtype', None)}")
        strides = nv12_frame_strides(y.shape, y.stride(), uv.shape, uv.stride()) if y.dim() == 3 and uv.dim() == 4 else None
        if strides is None:
            raise ValueError(f"y must be a non-empty (B,H,W) with unit column stride and uv (B,ceil(H/2),ceil(W/2),2) with strides (ub, uy, 2, 1), "
                             f"rows and images that do not overlap (or one image expanded over the batch in both), got {tuple(y.shape)} with "
                             f"strides {tuple(y.stride())} and {tuple(uv.shape)} with strides {tuple(uv.stride())}")
        if y.device != uv.device:
            raise ValueError(f"y and uv must be on one device, got {y.device} and {uv.device}")
        B, H, W = (int(v) for v in y.shape)
        sb, sy, ub, uy = strides
        if (y.storage_offset() + (B - 1) * sb + (H - 1) * sy + W > y.untyped_storage().nbytes()
                or uv.storage_offset() + (B - 1) * ub + ((H + 1) // 2 - 1) * uy + 2 * ((W + 1) // 2) > uv.untyped_storage().nbytes()):
            raise ValueError("y or uv ends short of the bytes its shape and strides describe")
        if csc is None:
            csc = nv12_csc(matrix, full_range)
        elif matrix is not None and matrix not in NV12_MATRICES:
            raise ValueError(f"matrix must be one of {sorted(NV12_MATRICES)} or None beside csc, got {matrix!r}")
        self.y, self.uv = y, uv
        self.matrix, self.full_range = matrix, bool(full_range)
        self.csc = _nv12_table(csc)
        self.strides = strides
        # what _frame_route and _frame_args hand to every call, made once: the planes stay where they are while the frame holds them
        self._tail = self.strides + self.csc
        self._args = (y.data_ptr(), uv.data_ptr()) + self._tail
        self.shape = torch.Size((B, 3, H, W))
        self.dtype = torch.uint8
        self.device = y.device
        self.is_cuda = y.is_cuda

    def dim(self):
        return 4

    def numel(self):
        return self.shape.numel()

    def like(self, y, uv):
        """The frame of other planes under this frame's colour table."""
        return Nv12Frame(y, uv, matrix=self.matrix, full_range=self.full_range, csc=self.csc)

    def route(self):
        """fs_nv12_frame_route of the frame: 1 the vector forms, 0 the one-pixel forms."""
        return int(hip.load().fs_nv12_frame_route(self.y.data_ptr(), self.uv.data_ptr(), *self.strides, int(self.shape[3])))


_FRAME_TYPES = (torch.Tensor, Nv12Frame)


def nv12_from_surface(buf, H, W, pitch, uv_offset, batch_stride=None, *, matrix, full_range=False, csc=None):
    """The Nv12Frame of one decoder surface: buf, a uint8 tensor of the surface's bytes (any shape; it is read flat and must be
    contiguous); B = its images.  Luma rows lie pitch apart from byte 0 of an image, chroma rows pitch apart from byte uv_offset (H *
    pitch for a tight surface; decoders that align the plane give their own); images batch_stride apart (None: one image, B = 1)."""
    if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or not buf.is_contiguous():
        raise ValueError(f"buf must be a contiguous uint8 tensor, got {getattr(buf, 'dtype', None)}")
    H, W, pitch, uv_offset = int(H), int(W), int(pitch), int(uv_offset)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    if min(H, W) < 1 or pitch < max(W, 2 * Wc) or uv_offset < H * pitch:
        raise ValueError(f"a surface of {H} x {W} pixels wants pitch >= {max(W, 2 * Wc)} and uv_offset >= H * pitch, got {pitch} and {uv_offset}")
    flat = buf.view(-1)
    per = uv_offset + (Hc - 1) * pitch + 2 * Wc
    if batch_stride is None:
        B, batch_stride = 1, per
    else:
        batch_stride = int(batch_stride)
        if batch_stride < uv_offset + Hc * pitch:
            raise ValueError(f"batch_stride must be at least uv_offset + ceil(H/2) * pitch = {uv_offset + Hc * pitch}, got {batch_stride}")
        B = (flat.numel() - per) // batch_stride + 1 if flat.numel() >= per else 0
    if flat.numel() < per or B < 1:
        raise ValueError(f"buf has {flat.numel()} bytes, one image of this surface needs {per}")
    y = flat.as_strided((B, H, W), (batch_stride, pitch, 1))
    uv = flat.as_strided((B, Hc, Wc, 2), (batch_stride, pitch, 2, 1), flat.storage_offset() + uv_offset)      # as_strided counts from the storage
    return Nv12Frame(y, uv, matrix=matrix, full_range=full_range, csc=csc)


def nv12_to_rgb(frame, out=None):
    """The RGB bytes of an NV12 frame (fs_nv12_to_rgb; no autograd; unpinned): out, a uint8 (B,3,H,W) tensor, contiguous or a view of
    interleaved (B,H,W,3) / (B,H,W,4) bytes (byte_frame_dest; RGBA gets alpha 255); None: a new contiguous one.  The planar result is
    the frame every other entry point is equal on.  Returns out."""
    if not isinstance(frame, Nv12Frame):
        raise ValueError(f"frame must be an ops.Nv12Frame, got {type(frame).__name__}")
    B, _, H, W = (int(v) for v in frame.shape)
    if out is None:
        out = torch.empty(B, 3, H, W, device=frame.device, dtype=torch.uint8)
    dest = byte_frame_dest(out, (B, 3, H, W))
    suffix, strides = _frame_route(frame)
    hip.call("fs_nv12_to_rgb", *_frame_args(frame, strides), *_dest_args(out, dest), B, H, W)
    return out


def _frame_route(img, what="img"):
    """Which of a pass's four entry points reads the frame img, and what follows the frame's pointer in its arguments: ("", ()) for fp32,
    ("_u8", ()) for contiguous bytes, ("_hwc", (sb, sy, sx)) for an hwc view, ("_nv12", (sb, sy, ub, uy, yo, yg, rv, gu, gv, bu)) for an
    Nv12Frame; ValueError for bytes in any other layout (_byte_frame).  A function of type, dtype, shape, strides and storage size
    alone: no device is asked."""
    if isinstance(img, Nv12Frame):
        return "_nv12", img._tail
    if img.dtype != torch.uint8:
        return "", ()
    layout = _byte_frame(img, what)
    return ("_u8", ()) if layout[0] == "planar" else ("_hwc", layout[1:])


def _frame_args(img, strides):
    """The frame's leading arguments of the entry point _frame_route chose: the device pointer and the strides of an hwc view (which is
    not contiguous, as hip.ptr asks of every other tensor), the two plane pointers, the strides and the table of an Nv12Frame."""
    if not strides:
        return (hip.ptr(img),)
    if not img.is_cuda:
        raise hip.HipLibraryError("fovealseg kernels need device tensors (got a CPU tensor); there is no CPU path")
    if isinstance(img, Nv12Frame):
        return img._args
    return (img.data_ptr(),) + strides


def byte_frame_select(img, sel):
    """img.index_select(0, sel) for an hwc view that stays one: the rows of the chosen frames are gathered from the underlying bytes (3 * H *
    W or 4 * H * W bytes a frame, never a planar copy) and viewed as (n,3,H,W) again.  With sb == 0 the n frames are the one frame.  An
    Nv12Frame stays one likewise: the chosen frames' luma and chroma rows are gathered as they lie, 1.5 bytes a pixel, no RGB copy."""
    if isinstance(img, Nv12Frame):
        B, _, H, W = (int(v) for v in img.shape)
        n = int(sel.shape[0])
        sb, sy, ub, uy = img.strides
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        if sb == 0 and ub == 0:
            return img.like(img.y[:1].expand(n, H, W), img.uv[:1].expand(n, Hc, Wc, 2))
        return img.like(img.y.index_select(0, sel), img.uv.index_select(0, sel))
    layout = byte_frame_layout(img)
    if layout is None or layout[0] != "hwc":
        return img.index_select(0, sel)
    _, sb, sy, sx = layout
    B, _, H, W = (int(v) for v in img.shape)
    n = int(sel.shape[0])
    if sb == 0:
        return img[:1].expand(n, 3, H, W)
    rows = img.as_strided((B, H, W * sx), (sb, sy, 1)).index_select(0, sel)
    return rows.view(n, H, W, sx).permute(0, 3, 1, 2)[:, :3]


def frame_in_place(img):
    """(the frame to hand to the kernels, whether it is read where it lies): an Nv12Frame (a decoder's surface) and a uint8 view of
    interleaved bytes (byte_frame_layout: a camera's HWC / RGBA buffer, permuted) stay as they are, flag True -- a part of such a frame is
    taken with byte_frame_select; anything else is img.contiguous(), img itself where it is contiguous already, flag False."""
    if isinstance(img, Nv12Frame) or (img.dtype == torch.uint8 and not img.is_contiguous() and byte_frame_layout(img) is not None):
        return img, True
    return img.contiguous(), False


def byte_frame_dest(out, shape=None):
    """(ob, oy, ox) of a uint8 (B,3,H,W) tensor the overlay pass can write, from byte_frame_layout's rule: (3 * H * W, W, 1) for a
    contiguous one; (sb, sy, sx) for a view of interleaved bytes (hwc.permute(0, 3, 1, 2) of a (B,H,W,3) buffer, rgba.permute(0, 3, 1,
    2)[:, :3] of a (B,H,W,4) one whose fourth byte is then written as 255, padded rows, a crop).  ValueError for any other tensor, another
    shape than `shape`, and one image expanded over several viewers (sb == 0 with B > 1: the viewers' pictures would overwrite each other)."""
    layout = byte_frame_layout(out)
    if layout is None or (shape is not None and tuple(out.shape) != tuple(shape)):
        raise ValueError(f"out must be a uint8 {tuple(shape) if shape is not None else '(B,3,H,W)'}, contiguous or a view of interleaved (B,H,W,3) / "
                         f"(B,H,W,4) bytes (ops.byte_frame_layout), got {getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))} with "
                         f"strides {tuple(out.stride()) if isinstance(out, torch.Tensor) else None}")
    B, _, H, W = (int(v) for v in out.shape)
    if layout[0] == "planar":
        return 3 * H * W, W, 1
    _, sb, sy, sx = layout
    if B > 1 and sb == 0:
        raise ValueError("out is one image expanded over several viewers: every viewer needs bytes of its own")
    return sb, sy, sx


def _dest_args(out, dest):
    if not out.is_cuda:
        raise hip.HipLibraryError("fovealseg kernels need device tensors (got a CPU tensor); there is no CPU path")
    return (out.data_ptr(),) + tuple(dest)
