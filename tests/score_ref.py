"""The instance score restated in torch (tests/test_instance_score.py).  Not a test module.

Definition (include/fovealseg.h, fs_head_fg_q / fs_unwarp_instances_scored; unpinned, the reference has no score): at a pixel the K
fp32 values v that unwarp_nearest(PredAssemble(cls, m)) holds give the foreground probability P = sum_{k<K-1} exp(v_k - max v) /
sum_k exp(v_k - max v) in fp64, quantised to q = rint(P * 2^24), 0 for a NaN P.  qsum = the sum of q over the mask's pixels,
mask_prob = qsum / (area * 2^24), cls_prob = softmax(cls[:K-1])[cat], score = mask_prob * cls_prob, all three in fp64.

Every reference here takes the fp32 v from a sampler and does only the softmax itself, in fp64 torch: on the CPU the v come from
F.grid_sample (the oracle's sampler), on the GPU from the library's own, so that device and reference differ by their fp64
exponentials and summation order alone."""
import torch
import torch.nn.functional as F

ONE = 2.0 ** 24


def band(K):
    """How far from a half-integer the reference's x = P * 2^24 must lie for rint(x) to be the same integer on both sides.  Per side:
    the arguments v_k - max v are the same doubles (IEEE subtraction); each of the K exponentials is within one ulp, a relative 2^-52;
    a sum of up to K positive terms adds (K-1) roundings of 2^-53 in any order; the division one more.  Numerator and denominator
    together: a relative error of P below 2 * (2^-52 + (K-1) * 2^-53) + 2^-53 < (K + 2) * 2^-52 per side, twice that between two
    sides, and P <= 1, so |x_device - x_reference| < 2 * (K + 2) * 2^-52 * 2^24 (the scaling by 2^24 is exact)."""
    return 2.0 * (K + 2) * 2.0 ** -52 * ONE


def q_from_v(v):
    """v (..., K) fp32 -> (q (...) int32, x (...) fp64 = P * 2^24, NaN where P is)."""
    assert v.dtype == torch.float32
    d = v.double()
    e = torch.exp(d - d.amax(-1, keepdim=True))
    x = e[..., :-1].sum(-1) / e.sum(-1) * ONE
    q = torch.where(torch.isnan(x), torch.zeros_like(x), torch.round(x)).to(torch.int32)          # torch.round: half to even, as rint
    return q, x


def in_band(x, K):
    """How many of the reference's x lie within band(K) of a half-integer: there the device may round to the other neighbour."""
    f = x[~torch.isnan(x)]
    return int(((f - torch.floor(f) - 0.5).abs() <= band(K)).sum())


def assemble(cls, m):
    """ops.PredAssemble restated: (B,K) x (B,h,w) -> (B,K,h,w)."""
    B, K = cls.shape
    pred = cls[:, :, None, None].expand(B, K, m.shape[1], m.shape[2]).clone()
    pred[:, -1] = cls[:, -1, None, None] * m
    return pred


def point_coords(h, w):
    """(h*w+1, 2) fp32: the inverse coordinate of every grid point (xi / w * 2 - 1, yi / h * 2 - 1), then (0,0) for an image without a
    claimed pixel; tests/test_predict.py factored_labels_ref's."""
    xi = torch.arange(w, dtype=torch.float32).repeat(h)
    yi = torch.arange(h, dtype=torch.float32).repeat_interleave(w)
    pts = torch.stack([xi / w * 2 - 1, yi / h * 2 - 1], -1)
    return torch.cat([pts, torch.zeros(1, 2)])


def point_values_cpu(cls, m):
    """(B, h*w+1, K) fp32 on the CPU: the prediction sampled by F.grid_sample at the points' inverse coordinates."""
    B, K = cls.shape
    h, w = m.shape[1:]
    pts = point_coords(h, w)[None, None].expand(B, 1, h * w + 1, 2).contiguous()
    return F.grid_sample(assemble(cls, m), pts, align_corners=False)[:, :, 0].permute(0, 2, 1).contiguous()


def point_values_dev(cls, m):
    """The same on the device, through the library's sampler (fs_grid_sample_fwd on ops.PredAssemble's prediction)."""
    from fovealseg import hip, ops
    B, K = cls.shape
    h, w = int(m.shape[1]), int(m.shape[2])
    n = h * w + 1
    pts = point_coords(h, w)[None, None].expand(B, 1, n, 2).contiguous().cuda()
    pred = ops.PredAssemble.apply(cls, m).contiguous()
    out = torch.empty(B, K, 1, n, device="cuda", dtype=torch.float32)
    hip.call("fs_grid_sample_fwd", hip.ptr(pred), hip.ptr(pts), hip.ptr(out), B, K, h, w, 1, n, 0)
    return out[:, :, 0].permute(0, 2, 1).contiguous()


def pixel_reference(cls, m, grid, Hs, Ws):
    """The unfused route on the device, one image at a time: (mask (B,Hs,Ws) bool = argmax != K-1, qsum (B,) int64, points inside the
    band).  v per pixel is ops.unwarp_nearest(ops.PredAssemble(cls, m), grid, Hs, Ws)[0]."""
    from fovealseg import ops
    B, K = cls.shape
    masks, qsum, close = [], [], 0
    for b in range(B):
        full = ops.unwarp_nearest(ops.PredAssemble.apply(cls[b:b + 1], m[b:b + 1]), grid[b:b + 1], Hs, Ws)[0][0]      # (K,Hs,Ws)
        mask = full.argmax(0) != K - 1
        sel = full.permute(1, 2, 0)[mask]                                              # (area, K): only the set pixels count
        q, x = q_from_v(sel)
        # every set pixel repeats one of at most h*w+1 points: the band is asked of the distinct values
        close += in_band(torch.unique(x[~torch.isnan(x)]), K)
        masks.append(mask)
        qsum.append(q.to(torch.int64).sum())
    return torch.stack(masks), torch.stack(qsum), close


def conf_ref(cls, cat, qsum, area):
    """(score, cls_prob, mask_prob) (B,3) in fp64 from fp32 cls (B,K), cat (B,), qsum (B,) int64, area (B,) int64."""
    cp = torch.softmax(cls[:, :-1].double(), 1).gather(1, cat.view(-1, 1))[:, 0]
    a = area.double()
    mp = torch.where(area > 0, qsum.double() / (a.clamp_min(1) * ONE), torch.zeros_like(a))
    return torch.stack([cp * mp, cp, mp], 1)


def ulps32(got, ref64):
    """|got - ref| in units of the fp32 spacing at ref (ref64 fp64, got fp32); NaN where either is NaN."""
    r32 = ref64.float()
    spacing = (torch.nextafter(r32.abs(), torch.full_like(r32, float("inf"))) - r32.abs()).double()
    return (got.double() - ref64).abs() / spacing
