"""Label-free full-resolution prediction: ops.unwarp_labels (fs_unwarp_labels) and DeformSegmentationModule.predict.

The C1 prediction is pred[b,k] = cls[b,k] for k < K-1 and cls[b,K-1] * m[b] for k = K-1.  Through the inverse warp every
full-resolution pixel carries the bilinear sample of pred at ONE grid point's inverse coordinate (its owner's; its nearest claimed
pixel's owner's; (0,0) in an image without any claim), so argmax_k of unwarp_nearest(pred) is a per-grid-point decision gathered
through the nearest-filled owner map.  CPU: that factorisation against the oracle.  GPU: the fused kernels against the unfused route
bit for bit, and predict against the hand-chained stages, the oracle and its contract (eval only, nothing written back)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fovealseg
from fovealseg import hip, ops
from fovealseg import train as T
from oracle import fovealseg_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------------------ CPU ----------
def assemble(cls, m):
    """ops.PredAssemble restated: (B,K) x (B,h,w) -> (B,K,h,w)."""
    B, K = cls.shape
    pred = cls[:, :, None, None].expand(B, K, m.shape[1], m.shape[2]).clone()
    pred[:, -1] = cls[:, -1, None, None] * m
    return pred


def owner_ref(grid, Hs, Ws):
    """(B, Hs*Ws) int64: index of the grid point claiming each pixel (the last claimant wins, as in O.inverse_grid_ref), -1 = hole."""
    B, h, w, _ = grid.shape
    u = (((grid[..., 0] + 1) / 2) * (Ws - 1)).int().long().view(B, -1).numpy()
    v = (((grid[..., 1] + 1) / 2) * (Hs - 1)).int().long().view(B, -1).numpy()
    own = np.full((B, Hs * Ws), -1, dtype=np.int64)
    for b in range(B):
        own[b][v[b] * Ws + u[b]] = np.arange(h * w)
    return torch.from_numpy(own)


def factored_labels_ref(cls, m, grid, Hs, Ws):
    """The factorisation in torch: argmax per grid point (and for the no-claim coordinate (0,0)), then a gather through the owner
    map, holes through the owner of their nearest claimed pixel (smallest (row, col) among equidistant ones)."""
    B, K = cls.shape
    _, h, w, _ = grid.shape
    xi = torch.arange(w, dtype=torch.float32).repeat(h)
    yi = torch.arange(h, dtype=torch.float32).repeat_interleave(w)
    pts = torch.stack([xi / w * 2 - 1, yi / h * 2 - 1], -1)                          # O.inverse_grid_ref's coordinates
    pts = torch.cat([pts, torch.zeros(1, 2)])                                         # + (0,0): the hole value of grid_inv
    pts = pts[None, None].expand(B, 1, h * w + 1, 2).contiguous()
    dec = F.grid_sample(assemble(cls, m), pts, align_corners=False)[:, :, 0].argmax(1)     # (B, h*w+1)
    own = owner_ref(grid, Hs, Ws)
    out = torch.empty(B, Hs * Ws, dtype=torch.int64)
    for b in range(B):
        claimed = torch.nonzero(own[b] >= 0).view(-1)                                 # row-major order
        feed = own[b].clone()
        holes = torch.nonzero(own[b] < 0).view(-1)
        if len(claimed) == 0:
            feed[:] = h * w
        elif len(holes):
            d = (holes[:, None] // Ws - claimed[None] // Ws) ** 2 + (holes[:, None] % Ws - claimed[None] % Ws) ** 2
            feed[holes] = own[b][claimed[d.argmin(1)]]
        out[b] = dec[b][feed]
    return out.view(B, Hs, Ws)


@pytest.mark.parametrize("B,K,h,w,Hs,Ws,seed", [
    (2, 2, 9, 11, 37, 30, 0),          # K = 2: one constant plane against the mask plane
    (2, 6, 9, 11, 50, 51, 1),
    (3, 51, 8, 8, 5, 6, 2),            # output smaller than the grid: duplicate claims everywhere, no holes
    (1, 5, 12, 7, 23, 61, 3),
])
def test_factorisation_holds_on_the_oracle(B, K, h, w, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    grid = (torch.rand(B, h, w, 2, generator=g) * 2.4 - 1.2).clamp(-1, 1)           # some points on the border
    cls = torch.randn(B, K, generator=g)
    m = torch.rand(B, h, w, generator=g) - 0.5
    cls[0, K - 1] = 4 * cls[0].abs().max()          # make the mask plane win somewhere and lose elsewhere in image 0
    want = O.unwarp_nearest_ref(assemble(cls, m), grid, Hs, Ws)[0].argmax(1)
    got = factored_labels_ref(cls, m, grid, Hs, Ws)
    assert torch.equal(got, want)
    assert len(want[0].unique()) >= 2
    claims = owner_ref(grid, Hs, Ws)
    assert int((claims >= 0).sum()) < B * h * w                                       # duplicate claims in every case


# ------------------------------------------------------------------------------------------------------------------ GPU: op -------
def _route(cls, m, grid, Hs, Ws):
    """The unfused route: (B,K,h,w) prediction -> (B,K,Hs,Ws) through the inverse warp and nearest fill -> argmax."""
    full, hole = ops.unwarp_nearest(ops.PredAssemble.apply(cls, m), grid, Hs, Ws)
    return full.argmax(1), hole


def _check(cls, m, grid, Hs, Ws):
    labels, hole = ops.unwarp_labels(cls, m, grid, Hs, Ws)
    want, whole = _route(cls, m, grid, Hs, Ws)
    assert labels.dtype == torch.int64 and labels.shape == (cls.shape[0], Hs, Ws) and hole.dtype == torch.bool
    assert torch.equal(hole, whole)
    assert torch.equal(labels, want)
    return labels, hole


def _inputs(B, K, h, w, seed, lo=-1.1, hi=1.1):
    g = torch.Generator().manual_seed(seed)
    grid = (torch.rand(B, h, w, 2, generator=g) * (hi - lo) + lo).clamp(-1, 1)
    cls = torch.randn(B, K, generator=g)
    cls[:, K - 1] = 3 * cls.abs().amax(1)            # the mask plane decides where m is large, a constant class elsewhere
    m = torch.rand(B, h, w, generator=g) - 0.5
    return cls.cuda(), m.cuda(), grid.cuda()


@pytest.mark.gpu
def test_unwarp_labels_g14_grid():
    g = {k: v for k, v in np.load(os.path.join(GOLD, "g14_inverse.npz")).items()}
    Hs, Ws = (int(v) for v in g["seg"])
    grid = torch.from_numpy(g["grid"]).cuda()
    B, h, w, _ = grid.shape
    cls, m, _ = _inputs(B, 51, h, w, 14)
    labels, hole = _check(cls, m, grid, Hs, Ws)
    assert torch.equal(hole.cpu(), torch.from_numpy(g["unfilled"]))
    assert len(labels.unique()) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("Hs,Ws,K", [(37, 300, 6), (50, 513, 3), (8, 1500, 2)])
def test_unwarp_labels_ragged_widths(Hs, Ws, K):
    cls, m, grid = _inputs(2, K, 9, 11, Hs * 1000 + Ws)
    _check(cls, m, grid, Hs, Ws)


@pytest.mark.gpu
def test_unwarp_labels_full_size():
    cls, m, grid = _inputs(2, 51, 80, 80, 7, -1.0, 1.0)
    labels, hole = _check(cls, m, grid, 1024, 1024)
    assert float(hole.float().mean()) > 0.99 and len(labels.unique()) >= 2


@pytest.mark.gpu
def test_unwarp_labels_output_smaller_than_grid():
    cls, m, grid = _inputs(2, 51, 80, 80, 8)
    labels, hole = _check(cls, m, grid, 24, 20)
    assert not bool(hole.any())                      # 6 400 points on 480 pixels: every pixel claimed, most of them many times


@pytest.mark.gpu
def test_unwarp_labels_border_grids():
    # grid points pushed onto +-1 claim the corner rows / columns; the border points' inverse coordinates take half-weight taps
    g = torch.Generator().manual_seed(5)
    grid = torch.rand(2, 16, 20, 2, generator=g) * 2 - 1
    edge = torch.rand(2, 16, 20, 2, generator=g)
    grid = torch.where(edge < 0.3, torch.full_like(grid, -1.0), torch.where(edge > 0.7, torch.ones_like(grid), grid))
    cls = torch.randn(2, 7, generator=g)
    cls[:, 6] = 3 * cls.abs().amax(1)
    m = torch.rand(2, 16, 20, generator=g) - 0.5
    _check(cls.cuda(), m.cuda(), grid.cuda(), 45, 70)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 51, 150])
def test_unwarp_labels_class_counts(K):
    cls, m, grid = _inputs(3, K, 40, 40, K)
    labels, _ = _check(cls, m, grid, 300, 200)
    assert len(labels.unique()) >= 2


@pytest.mark.gpu
def test_unwarp_labels_no_claimed_pixel():
    # image 1's grid lies outside [-1, 1]: nothing is claimed there, every pixel keeps the sample at (0, 0)
    cls, m, grid = _inputs(2, 9, 10, 12, 3)
    grid[1] = 1.5
    labels, hole = _check(cls, m, grid, 31, 40)
    assert bool(hole[1].all()) and not bool(hole[0].all())


@pytest.mark.gpu
def test_unwarp_labels_ties_go_to_the_lower_class():
    cls, m, grid = _inputs(2, 8, 12, 12, 4)
    cls[0] = torch.arange(8, device="cuda", dtype=torch.float32) * 0.1
    cls[0, 2] = cls[0, 5] = 9.0                      # two constant classes tie everywhere
    cls[1] = -1.0
    cls[1, 4] = cls[1, 7] = 2.0                      # a constant class ties with the mask plane where m == 1
    m[1] = 1.0
    labels, _ = _check(cls, m, grid, 40, 50)
    assert bool((labels[0] == 2).all()) and bool((labels[1] == 4).all())


@pytest.mark.gpu
def test_unwarp_labels_nan_is_maximal():
    cls, m, grid = _inputs(2, 6, 8, 8, 6)
    cls[0, 3] = float("nan")                         # torch.argmax: a NaN is the maximum
    labels, _ = _check(cls, m, grid, 20, 30)
    assert bool((labels[0] == 3).all())


@pytest.mark.gpu
def test_unwarp_labels_rejects_bad_arguments():
    cls, m, grid = _inputs(1, 4, 4, 4, 0)
    with pytest.raises(ValueError):                  # m not at the grid's resolution
        ops.unwarp_labels(cls, m[:, :3], grid, 8, 8)
    with pytest.raises(hip.HipLibraryError):         # K < 2
        ops.unwarp_labels(cls[:, :1], m, grid, 8, 8)
    big = torch.randn(1, 1025, device="cuda")
    with pytest.raises(hip.HipLibraryError):         # K beyond the kernel's 1 024
        ops.unwarp_labels(big, m, grid, 8, 8)
    ops.unwarp_labels(big[:, :1024].contiguous(), m, grid, 8, 8)
    with pytest.raises(hip.HipLibraryError):         # a row longer than the row pass's LDS
        ops.unwarp_labels(cls, m, grid, 1, 16385)
    lab = torch.empty(1, 8, 8, device="cuda", dtype=torch.int64)
    scr = torch.empty(hip.query("fs_unwarp_labels_scratch_ints", 1, 4, 4, 8, 8), device="cuda", dtype=torch.int32)
    with pytest.raises(hip.HipLibraryError):         # no scratch
        hip.call("fs_unwarp_labels", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), lab.data_ptr(), None, None, 1, 4, 4, 4, 8, 8)
    hip.call("fs_unwarp_labels", cls.data_ptr(), m.data_ptr(), grid.data_ptr(), lab.data_ptr(), None, scr.data_ptr(), 1, 4, 4, 4, 8, 8)
    assert torch.equal(lab, _route(cls, m, grid, 8, 8)[0])           # the hole mask is optional


# ------------------------------------------------------------------------------------------------------------------ GPU: module ---
def _cfg(kind):
    cfg = fovealseg.lvis50_cfg()
    if kind == "segformer":
        cfg.MODEL.arch_encoder, cfg.MODEL.fc_dim = "segformer", 1024
        cfg.TRAIN.task_input_size = (160, 160)
    elif kind == "deeplab":
        cfg.MODEL.arch_encoder = "deeplab"
    elif kind == "uniform":
        cfg.MODEL.uniform_sample = "Saliency"
    return cfg


_MODULES = {}


def _module(kind):
    if kind not in _MODULES:
        _MODULES.clear()                             # one module at a time on the device
        torch.cuda.empty_cache()
        _MODULES[kind] = T.build_module(_cfg(kind), device="cuda")
    module, nets = _MODULES[kind]
    module.eval()
    return module, nets


def _chained(module, img, focus, seg_size):
    """The route a user chains by hand today: stages -> PredAssemble -> unwarp_nearest -> argmax."""
    with torch.no_grad():
        xs, _ = module.saliency(img, focus)
        if module.cfg.MODEL.uniform_sample != "":
            xs = xs * 0 + 1.0 / (module.grid_size_x * module.grid_size_y)
        grid = module.create_grid(xs)
        feat = module.encoder.forward_nhwc(ops.GridSample.apply(img, grid))
        pred = module.decoder.forward_nhwc(feat)
        full, _ = ops.unwarp_nearest(pred, grid, int(seg_size[0]), int(seg_size[1]))
        return full.argmax(1), grid


def _batch(B, size, seed):
    X, Fp, _Y, _cls = T.synthetic_batch(B, size, size, seed=seed, device="cuda")
    return X, Fp


@pytest.fixture
def deterministic():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,seg", [("hrnet", 256, None), ("segformer", 256, (200, 180)), ("deeplab", 128, None),
                                           ("uniform", 192, None)])
def test_predict_equals_the_hand_chained_route(kind, size, seg, deterministic):
    module, _ = _module(kind)
    X, Fp = _batch(2, size, 11)
    X0, F0 = X.clone(), Fp.clone()
    got = module.predict(X, Fp, seg)
    module.check_nan()
    seg = seg or (size, size)
    want, grid = _chained(module, X, Fp, seg)
    assert got.dtype == torch.int64 and got.shape == (2, *seg)
    assert torch.equal(got, want)
    assert torch.equal(X, X0) and torch.equal(Fp, F0)                                 # nothing written back into an argument
    assert 0 <= int(got.min()) and int(got.max()) < module.cfg.DATASET.num_class
    if kind == "segformer":
        assert grid.shape[1:3] == (160, 160)                                          # the task-size up-sampled grid
    if kind == "hrnet":
        ops.static_weight_packs(module)                                               # serving: weight packs kept across calls
        try:
            assert torch.equal(module.predict(X, Fp), module.predict(X, Fp))
            assert torch.equal(module.predict(X, Fp, seg), want)
        finally:
            ops.static_weight_packs(module, on=False)


@pytest.mark.gpu
def test_predict_against_the_oracle():
    module, _ = _module("hrnet")
    o = O.OracleDeformSeg()
    fovealseg.weights.apply_name_keyed_init(o)
    o.eval()
    # with the name-keyed weights one constant class wins everywhere; a large background logit on both sides lets the mask
    # plane (cls[K-1] * m) decide wherever m > 0
    bias = module.decoder.cls_net.fc.bias
    keep = bias.detach().clone()
    with torch.no_grad():
        bias[-1] += 1000.0
        o.decoder.cls_net.fc.bias[-1] += 1000.0
    X, Fp = _batch(2, 128, 21)
    try:
        got = module.predict(X, Fp).cpu()
        _, grid = _chained(module, X, Fp, (128, 128))
    finally:
        with torch.no_grad():
            bias.copy_(keep)
    Xc, Fc = X.cpu(), Fp.cpu()
    with torch.no_grad():
        # the device's grid injected into the oracle's stages
        g = grid.cpu()
        pred = o.decoder(o.encoder(F.grid_sample(Xc, g, align_corners=False), return_feature_maps=True))
        want = O.unwarp_nearest_ref(pred, g, 128, 128)[0].argmax(1)
        # free running: the oracle's own grid
        og = o.grid_from_saliency(o.saliency(Xc, Fc)[0])
        fpred = o.decoder(o.encoder(F.grid_sample(Xc, og, align_corners=False), return_feature_maps=True))
        free = O.unwarp_nearest_ref(fpred, og, 128, 128)[0].argmax(1)
    differ = float((got != want).float().mean())
    print(f"predict vs oracle: {differ:.2e} of pixels differ with the device grid injected, "
          f"{float((got != free).float().mean()):.2e} free running (grid err {float((g - og).abs().max()):.2e})")
    print(f"  classes in the oracle's map: {want.unique().tolist()}, background share {float((want == 50).float().mean()):.3f}")
    assert differ <= 1e-3


@pytest.mark.gpu
def test_predict_rejects_train_mode_and_bad_arguments():
    module, _ = _module("hrnet")
    X, Fp = _batch(2, 96, 3)
    module.train()
    try:
        with pytest.raises(RuntimeError):
            module.predict(X, Fp)
    finally:
        module.eval()
    with pytest.raises(ValueError):
        module.predict(X, Fp[:1])                                                     # batch mismatch
    with pytest.raises(ValueError):
        module.predict(X, Fp, (96, 0))
    with pytest.raises(ValueError):
        module.predict(X, Fp, (96, 96, 1))


@pytest.mark.gpu
def test_predict_leaves_the_module_untouched(deterministic):
    module, nets = _module("hrnet")
    cfg = module.cfg
    X, Fp, Y, cls = T.synthetic_batch(2, 160, 160, seed=5, device="cuda")
    state = {k: v.detach().clone() for k, v in module.state_dict().items()}
    step0 = ops.DropoutState.step
    module.predict(X, Fp)
    module.check_nan()
    assert ops.DropoutState.step == step0
    for k, v in module.state_dict().items():
        assert torch.equal(v, state[k]), k

    # a training step after predict is the training step without it, bit for bit
    opts = T.create_optimizers(nets, cfg)

    def step():
        module.load_state_dict(state)
        for opt in opts:
            opt.t = 0
            opt.m.zero_()
            opt.v.zero_()
            opt.flat.refresh_amax()
        ops.DropoutState.step = step0
        module.train()
        out = T.train_step(module, opts, (X, Fp, Y, cls), cfg)
        res = [out[0].detach().clone()] + [opt.flat.grad.clone() for opt in opts]
        module.eval()
        return res

    try:
        plain = step()
        module.predict(X, Fp)
        after = step()
    finally:
        module.load_state_dict(state)
        ops.DropoutState.step = step0
        _MODULES.clear()                             # the optimisers re-homed the parameters into their arenas
    for a, b in zip(plain, after):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_predict_allocates_no_full_resolution_class_tensor():
    module, _ = _module("hrnet")
    X, Fp = _batch(2, 2048, 9)
    with torch.no_grad():
        def stages():
            xs, _ = module.saliency(X, Fp)
            grid = module.create_grid(xs)
            return module.decoder.forward_parts_nhwc(module.encoder.forward_nhwc(ops.GridSample.apply(X, grid)))
        stages()
        module.predict(X, Fp)                                                         # warm-up: weight packs, workspaces
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        parts = stages()
        torch.cuda.synchronize()
        base = torch.cuda.max_memory_allocated()
        del parts
        torch.cuda.reset_peak_memory_stats()
        labels = module.predict(X, Fp)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
    module.check_nan()
    extra = (peak - base) / 2 ** 30
    print(f"predict peak over the stages' peak: {extra:.3f} GB (labels {labels.numel() * 8 / 2 ** 30:.3f} GB)")
    assert labels.shape == (2, 2048, 2048)
    assert extra < 0.3                               # the (B, 51, 2048, 2048) fp32 prediction alone would be 1.6 GiB
