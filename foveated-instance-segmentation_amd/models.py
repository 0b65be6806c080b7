"""Plugin surface of the reference, backed by the HIP path.

`ModelBuilder` (models/models.py:1146-1230) and `DeformSegmentationModule` (models/models.py:476-1094)
with the same constructor/forward signatures, attribute names, return tuples, state_dict keys and the
`feed_dict['seg_label']` side effect (:951), under the effective LVIS-50 configuration
(SURVEY.md Appendix A).  Branches the default run never takes raise NotImplementedError.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import frames, masks
from . import modules as M
from . import ops
from .weights import apply_name_keyed_init  # noqa: F401  (re-export for callers)


def make_gaussian_1d(size: int, fwhm: float) -> np.ndarray:
    """1-D factor of makeGaussian (models/models.py:140-157): G[i,j] = g[i]*g[j], float64."""
    ax = np.arange(0, size, 1, float)
    return np.exp(-4 * np.log(2) * (ax - size // 2) ** 2 / fwhm ** 2)


class ModelBuilder:
    @staticmethod
    def weights_init(m):
        """models/models.py:1149-1155 (by class name: Conv -> kaiming normal, BatchNorm -> w=1, b=1e-4)."""
        classname = m.__class__.__name__
        if classname.find("Conv2d") != -1 and hasattr(m, "weight"):
            nn.init.kaiming_normal_(m.weight.data)
        elif classname.find("BatchNorm") != -1:
            m.weight.data.fill_(1.0)
            m.bias.data.fill_(1e-4)

    @staticmethod
    def _load(net, weights):
        if len(weights) > 0:
            net.load_state_dict(torch.load(weights, map_location=lambda storage, loc: storage), strict=False)
        return net

    @staticmethod
    def build_encoder(arch="resnet50", fc_dim=2048, weights="", dilate_rate=4):
        arch = arch.lower()
        if arch == "hrnetv2_nodownsp":
            net = M.hrnetv2_nodownsp(pretrained=False)
        elif arch == "deeplab":
            from . import deeplab as _dl
            net = _dl.deeplab(pretrained=False)
        elif arch == "segformer":
            from . import segformer as _sf
            net = _sf.segformer(pretrained=False)
        else:
            raise Exception("Architecture undefined!")
        return ModelBuilder._load(net, weights)

    @staticmethod
    def build_decoder(arch="upernet", fc_dim=2048, num_class=150, weights="", use_softmax=False):
        arch = arch.lower()
        if arch == "c1":
            net = M.C1(num_class=num_class, fc_dim=fc_dim, use_softmax=use_softmax)
        else:
            raise Exception("Architecture undefined!")
        net.apply(ModelBuilder.weights_init)
        return ModelBuilder._load(net, weights)

    @staticmethod
    def build_net_saliency(cfg=None, weights=""):
        if not (cfg.MODEL.track_running_stats and cfg.MODEL.saliency_net == "fovsimple"):
            raise Exception("Architecture undefined!")
        net = M.fov_simple(cfg)
        if len(weights) == 0:
            net.apply(ModelBuilder.weights_init)
        return ModelBuilder._load(net, weights)

    @staticmethod
    def build_net_compress(cfg=None, weights=""):
        net = M.CompressNet(cfg)
        if len(weights) == 0:
            net.apply(ModelBuilder.weights_init)
        return ModelBuilder._load(net, weights)


class _FilterHolder(nn.Module):
    """Keeps the `filter.weight` state_dict key of the reference (a fixed 91x91 Gaussian, Q6)."""

    def __init__(self, k, fwhm):
        super().__init__()
        g = make_gaussian_1d(k, fwhm)
        self.register_buffer("weight", torch.from_numpy(np.outer(g, g)).float().view(1, 1, k, k))


class DeformSegmentationModule(nn.Module):
    def __init__(self, net_encoder, net_decoder, net_saliency, net_compress, crit, cfg, deep_sup_scale=None):
        super().__init__()
        self.encoder = net_encoder
        self.decoder = net_decoder
        self.localization = net_saliency
        self.net_compress = net_compress
        self.cfg = cfg
        self.deep_sup_scale = deep_sup_scale
        T = cfg.TRAIN
        if cfg.MODEL.saliency_output_size_short != 0 or cfg.MODEL.gaussian_ap != 0.0:
            raise NotImplementedError("only saliency_output_size_short=0, gaussian_ap=0.0 (defaults) are built")
        self.grid_size_x, self.grid_size_y = int(T.saliency_input_size[0]), int(T.saliency_input_size[1])
        self.padding_size_x = self.padding_size_y = int(cfg.MODEL.gaussian_radius)
        self.input_size = tuple(T.saliency_input_size)
        self.input_size_net = tuple(T.task_input_size)
        ti, si = tuple(int(v) for v in self.input_size_net), tuple(int(v) for v in self.input_size)
        if ti != si and (ti[0] % si[0] or ti[1] % si[1]):
            raise NotImplementedError("task_input_size must be an integer multiple of saliency_input_size (grid up-sampling, models/models.py:621-631)")
        if cfg.DATASET.segm_downsampling_rate != 1:
            raise NotImplementedError("DATASET.segm_downsampling_rate must be 1 (grid_y == grid, models/models.py:627): with any other rate the "
                                      "reference samples the label at task_input_size // rate and multiplies it with cls_label.repeat(1, HS, WS) at the "
                                      "saliency size (:968) against a prediction at the task size -- a shape error with every encoder of this path")
        k = 2 * self.padding_size_x + 1
        self.filter = _FilterHolder(k, cfg.MODEL.gaussian_radius)
        self.register_buffer("g1d", torch.from_numpy(make_gaussian_1d(k, cfg.MODEL.gaussian_radius)), persistent=False)
        self._check_cfg()

    def _check_cfg(self):
        c = self.cfg
        off = [("MODEL.loss_at_high_res", c.MODEL.loss_at_high_res),
               ("MODEL.gt_gradient", c.MODEL.gt_gradient), ("TRAIN.opt_deform_LabelEdge", c.TRAIN.opt_deform_LabelEdge)]
        for name, val in off:
            if val:
                raise NotImplementedError(f"{name}=True is outside the built hot path (SURVEY.md Appendix A)")
        if c.MODEL.upsample and c.MODEL.rev_deform_interp != "nearest":
            raise NotImplementedError("MODEL.upsample needs rev_deform_interp='nearest' (the reference's 'tri' default calls an undefined name)")
        if c.MODEL.uniform_sample == "BI":
            raise NotImplementedError("MODEL.uniform_sample='BI' is unreachable in the reference with this fork's (B,1,H,W) labels: "
                                      "nn.Upsample(mode='bilinear') of y.float().unsqueeze(1) is handed a 5-D tensor (models/models.py:877); "
                                      "'' (learned sampling) and any other value (uniform saliency, config/defaults.py:69) are built")
        if c.TRAIN.def_saliency_pad_mode not in ops.PAD_MODES:
            # models/models.py:819-825 has no else branch: xs_hm stays unbound and line 845 raises the NameError subclass below
            raise UnboundLocalError("local variable 'xs_hm' referenced before assignment (TRAIN.def_saliency_pad_mode must be "
                                    "'replication', 'reflect' or 'zero', models/models.py:819-825)")
        if c.TRAIN.def_saliency_pad_mode == "reflect" and self.padding_size_x > min(self.grid_size_x, self.grid_size_y) - 1:
            raise NotImplementedError("def_saliency_pad_mode='reflect' needs gaussian_radius <= saliency side - 1 (F.pad refuses it too)")
        if not c.TRAIN.opt_deform_LabelEdge_norm:
            raise NotImplementedError("only the min/max-normalised edge loss is built")
        if self.deep_sup_scale is not None:
            raise NotImplementedError("deep supervision is not used on this path")

    # ---- stages (exposed for stage-wise parity tests) -------------------------------------------
    def saliency(self, x, focus):
        """x (B,3,H,W), focus (B,2) -> xs (B,1,hs,ws), x_low (B,hs,ws,5) NHWC."""
        x_low = ops.gaze_lowres(x, focus, self.grid_size_x, self.grid_size_y)
        s = self.localization.forward_nhwc(x_low)
        return self.net_compress.softmax_nhwc(s), x_low

    def create_grid(self, xs):
        """xs (B,1,hs,ws) -> grid (B,ht,wt,2) at the task network's input size; the padding of TRAIN.def_saliency_pad_mode
        ('replication' nn.ReplicationPad2d, 'reflect' / 'zero' F.pad) folded in (models/models.py:594-637,819-825).  When task_input_size != saliency_input_size the (hs,ws) grid is bilinearly up-sampled
        (nn.Upsample(size=input_size_net, mode='bilinear'), :621-631); grid_y is the same tensor (segm_downsampling_rate 1)."""
        grid = ops.GaussGrid.apply(xs, self.g1d, self.padding_size_x, ops.PAD_MODES[self.cfg.TRAIN.def_saliency_pad_mode])
        ht, wt = int(self.input_size_net[0]), int(self.input_size_net[1])
        if (ht, wt) != (grid.shape[1], grid.shape[2]):
            grid = ops.GridUpsample.apply(grid, ht, wt)
        return grid

    @torch.no_grad()
    def unwarp(self, pred, grid, seg_size):
        """Full-resolution prediction from the foveated one: the inverse grid of `create_grid(..., segSize, x_inv)`
        (models/models.py:639-655), `F.grid_sample(pred, grid_inv)` (:933) and the nearest-neighbour hole filling of
        `fillMissingValues_tensor(..., interp_mode='nearest')` (:159-286), all on the device (the
        'tri' default of the reference calls an undefined name).  pred (B,C,h,w) logical NCHW, grid (B,h,w,2) as returned by
        create_grid; returns (pred_full (B,C,H,W), hole mask (B,H,W))."""
        return ops.unwarp_nearest(pred.contiguous(), grid, int(seg_size[0]), int(seg_size[1]))

    # models/models.py:721 asserts `not torch.isnan(xs).any()` in the middle of the forward: a device->host read that drains the
    # stream once per step (2-3 % of the training step on MI355X, profiles/r02/nan_check_ab.txt).  The same flag is taken on the
    # device, copied to pinned host memory without blocking, and the AssertionError (same message) is raised when the flag is
    # next looked at: at the end of train.train_step / train.eval_step, at the next forward, or by check_nan().
    # FS_NAN_CHECK=sync restores the reference's in-place assert, FS_NAN_CHECK=0 drops the check.
    _nan_mode = os.environ.get("FS_NAN_CHECK", "defer")

    def _note_nan(self, xs):
        if self._nan_mode == "0":
            return
        if self._nan_mode == "sync" or not xs.is_cuda:
            assert not torch.isnan(xs).any(), "xs contains NaN values!"
            return
        st = self.__dict__.setdefault("_nan_state", {"host": torch.zeros(1, dtype=torch.bool).pin_memory(), "event": None})
        st["host"].copy_(torch.isnan(xs).any().reshape(1), non_blocking=True)
        st["event"] = torch.cuda.Event()
        st["event"].record()

    def check_nan(self):
        """Raise the pending `xs contains NaN values!` assertion of the last forward, if any (see _note_nan)."""
        st = self.__dict__.get("_nan_state")
        if st is None or st["event"] is None:
            return
        st["event"].synchronize()
        st["event"] = None
        assert not bool(st["host"][0]), "xs contains NaN values!"

    def _head_parts(self, img, focus, seg_size, who):
        """predict's / evaluate's shared front: argument checks, then forward's stages up to the C1 head's two factors.
        Returns (cls (B,K), m (B,h,w), grid (B,h,w,2), seg_size as two ints).  img is fp32, or a planar torch.uint8 frame whose pixel
        value is byte / 255 correctly rounded: the results equal those of the fp32 frame of that quotient bit for bit, and the frame is
        read as bytes by the two gathers of the front (ops.gaze_lowres, ops.grid_sample_u8).  A uint8 frame may also be a view of
        interleaved bytes (hwc.permute(0, 3, 1, 2), rgba.permute(0, 3, 1, 2)[:, :3], padded rows, a crop: ops.byte_frame_layout): the
        gathers read it where it lies, nothing is copied, and the results equal those of its planar copy bit for bit.  An ops.Nv12Frame (a
        decoder's luma and chroma planes) is taken in a uint8 frame's place and read where it lies too: the results equal those of
        ops.nv12_to_rgb(img) bit for bit."""
        if self.training:
            raise RuntimeError(f"{who}() needs eval mode (module.eval()): in train mode the encoder would update its BatchNorm running statistics")
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"img must be (B,3,H,W), got {tuple(img.shape)}")
        B = img.shape[0]
        if tuple(focus.shape) != (B, 2):
            raise ValueError(f"focus must be (B,2) = ({B},2), got {tuple(focus.shape)}")
        if seg_size is None:
            seg_size = (img.shape[2], img.shape[3])
        if len(seg_size) != 2 or int(seg_size[0]) <= 0 or int(seg_size[1]) <= 0:
            raise ValueError(f"seg_size must be (H, W) with positive sides, got {tuple(seg_size)}")
        self.check_nan()
        ops.reset_step_state()
        # a uint8 view of interleaved bytes (ops.byte_frame_layout: a permuted HWC / RGBA buffer) is read where it lies
        # so is an NV12 frame (ops.Nv12Frame: a decoder's surface), each tap converted to its RGB byte as it is read
        x, _in_place = frames.frame_in_place(img)
        xs, _ = self.saliency(x, focus.float().contiguous())
        self._note_nan(xs)
        if self.cfg.MODEL.uniform_sample != "":
            xs = xs * 0 + 1.0 / (self.grid_size_x * self.grid_size_y)       # as forward, models/models.py:816-818
        grid = self.create_grid(xs)
        # a frame of bytes (pixel value byte / 255) is read by the two gathers of the front alone: no fp32 frame is made
        sampled = ops.grid_sample_u8(x, grid) if x.dtype == torch.uint8 else ops.GridSample.apply(x, grid)
        feat = self.encoder.forward_nhwc(sampled)
        cls, m = self.decoder.forward_parts_nhwc(feat)
        return cls, m, grid, (int(seg_size[0]), int(seg_size[1]))

    @torch.no_grad()
    def predict(self, img, focus, seg_size=None):
        """Label-free inference: which class every full-resolution pixel of `img` belongs to, given the gaze point `focus`.

        img (B,3,H,W) as forward's img_data -- or the same frame as torch.uint8, pixel value byte / 255, which gives the same result bit
        for bit without an fp32 frame (predict_instances, evaluate and evaluate_instances likewise) --, focus (B,2) as its focus_point; returns the int64 class map (B, *seg_size), seg_size
        defaulting to (H, W).  The stages are forward's -- saliency, the sampling grid (uniform_sample and the task-size up-sampling
        included), GridSample, encoder, C1 head -- then the inverse warp with nearest hole filling and the argmax over classes
        (models/models.py:639-655,930-940; eval.py:195), fused in ops.unwarp_labels so that no (B,K,*seg_size) prediction exists.
        The result equals `unwarp_nearest(decoder.forward_nhwc(feat), grid, *seg_size)[0].argmax(1)` bit for bit.

        Class num_class - 1 is background: the gazed instance's mask is `labels != num_class - 1`.  Eval mode only (module.eval()):
        a train-mode forward would update the BatchNorm running statistics.  No label is read, no loss is computed and no argument is
        written to.  A NaN saliency map raises forward's `xs contains NaN values!` assertion at the next forward / predict or at
        check_nan(), as in forward (_note_nan)."""
        cls, m, grid, seg_size = self._head_parts(img, focus, seg_size, "predict")
        labels, _hole = ops.unwarp_labels(cls, m, grid, *seg_size)
        return labels

    @torch.no_grad()
    def predict_instances(self, img, focus, seg_size=None, max_runs=None, return_bits=False, return_score=False, component=None, snap_px=None):
        """Label-free inference as an instance record: the gazed instance's class, area, box and mask, without the class map.

        img, focus and seg_size as predict's; the stages are predict's up to the gather, which stores the mask `predict(...) !=
        num_class - 1` as bit words (ops.unwarp_instances / fs_unwarp_instances) so that nothing of (B, *seg_size) wider than a bit
        per pixel exists.  Returns (cat, stats, counts[, bits]): cat (B,) int64 the head's classification among the classes below
        num_class - 1 (torch.argmax of their logits); stats (B,6) int64 = (area, x0, y0, bw, bh, n_runs) with [x0, y0, bw, bh] the
        COCO box, all 0 for an empty mask; counts (B,max_runs) int32 the uncompressed COCO run-length code (column-major), zero past
        its n_runs entries; with return_bits the mask itself, (B,H,ceil(W/32)) int32, bit j of word i = pixel x = 32 i + j.  All of it
        equals what `predict` gives bit for bit, except that cat is the head's decision and not a pixel's label: a foreground pixel's
        label differs from it only where the bilinear sample of the constant class planes ties two classes by rounding or has no
        in-bounds weight.  max_runs (any int >= 1) defaults to 8 * W + 1, room for a mask whose every column crosses its outline at
        most eight times; stats[:, 5] > max_runs tells a cut code.  ops.instances_to_coco turns the result into COCO / LVIS records.

        return_score=True appends conf (B,3) fp32 = (score, cls_prob, mask_prob) as the last element (ops.unwarp_instances(score=True);
        unpinned, the reference has no score): cls_prob the softmax probability of cat among the classes below num_class - 1, mask_prob
        the mean over the mask's pixels of the softmax mass of those classes against background, score their product -- the mean
        probability of class cat over the mask, what COCOeval / the LVIS evaluator rank records by (instances_to_coco(..., conf=conf)).
        mask_prob and score are 0 for an empty mask, cls_prob and score NaN where the class logits hold a NaN.  The other results are
        the unscored call's bit for bit; the call allocates a few bytes per grid point more and no full-resolution tensor.

        component = 4 or 8 (ops.unwarp_instances(component=...); unpinned) keeps only the connected component of the mask under the
        gaze -- the set pixel at the gaze point `focus`, or the nearest one within snap_px pixels (None: any distance) -- with 4- or
        8-connectivity, taken on the device from the bit words: stats, counts, bits, mask_prob and score then describe that one blob,
        not a second object or specks the head also marked, and are the empty mask's where there is none; cat and cls_prob are
        unchanged.  comp (B,4) int64 = (seed_y, seed_x, d2, area_all) is appended as the last element, behind conf.  ValueError for
        any other component, or for snap_px without component.  With component=None the call is what it was.

        Eval mode only, no label read, no argument written to, and a NaN saliency map is reported as in predict."""
        if component is None:
            if snap_px is not None:
                raise ValueError("snap_px goes with component = 4 or 8")
        else:
            masks._component_args(component, snap_px)
        cls, m, grid, seg_size = self._head_parts(img, focus, seg_size, "predict_instances")
        if component is not None:
            out = ops.unwarp_instances(cls, m, grid, *seg_size, max_runs=max_runs, return_bits=return_bits, score=return_score,
                                       component=component, focus=focus, snap_px=snap_px)
            return out[:-2] + out[-1:] if return_score else out              # qsum stays inside
        if return_score:
            return ops.unwarp_instances(cls, m, grid, *seg_size, max_runs=max_runs, return_bits=return_bits, score=True)[:-1]
        return ops.unwarp_instances(cls, m, grid, *seg_size, max_runs=max_runs, return_bits=return_bits)

    @torch.no_grad()
    def evaluate_instances(self, img, focus, seg_label=None, cls_label=None, seg_size=None, max_runs=None, component=None, snap_px=None, boundary=0.02,
                           candidates=None, cand_snap_px=None):
        """The instance record scored against the label: predict_instances(..., return_bits=True, return_score=True, component=...),
        then the counters of mask IoU and Boundary IoU (Cheng et al., CVPR 2021, restated: unpinned) of the record's mask against the
        label's foreground `seg_label.long() != 0` (evaluate's hausdorff rule), taken on bit words (ops.mask_bits, ops.mask_pair_counts).

        img, focus, max_runs, component and snap_px as predict_instances'; seg_label (B,H,W) or (B,1,H,W) and cls_label (B,) or (B,1)
        as evaluate's, seg_size defaulting to the label's size and not differing from it.  boundary is the dilation ratio, a finite
        float > 0: d = ops.boundary_dilation(H, W, boundary), 0.02 of the diagonal.  Returns (cat, stats, counts, conf[, comp], pair):
        every element but the last is predict_instances' for the same arguments bit for bit (comp exactly when component is given);
        pair (B,6) int64 = (|p & g|, |p|, |g|, |band(p) & band(g)|, |band(p)|, |band(g)|) of the record's mask p -- the component,
        with component -- and the label g.  ops.pair_scores makes IoU and Boundary IoU, train.InstanceAPMeter AP and Boundary AP over
        a dataset (cls_label is that meter's; here only its batch size is checked).  Nothing of (B,H,W) wider than a bit a pixel is
        allocated beyond the label's bool mask.  Eval mode only, no host read, no argument written to, nothing in the module changes.

        seg_label may also be a tuple (counts, n_runs): the label's uncompressed run-length code as ops.rle_bits takes it -- counts
        (B,cap) int32, n_runs int64 (B,) or a stats (B,6) tensor --, at seg_size, which is then required (ops.coco_to_instances makes
        both from COCO / LVIS annotations).  The label's bit words then come from ops.rle_bits instead of ops.mask_bits and no dense
        label exists at all.  An image whose code is not valid (cut, a negative count, a wrong sum) scores as an empty label, |g| = 0:
        the call still reads nothing on the host; ops.rle_bits(counts, n_runs, seg_size, check=True) tells such a code beforehand.

        candidates = (cbits, cand_off, cand_cat) gives the images' annotated instances instead of one label (ops.coco_candidates makes
        the three from an annotation file's records): cbits (N,H,ceil(W/32)) int32 bit words at seg_size, which is then required,
        cand_off (B+1,) int32, cand_cat (N,) int64 or None.  seg_label and cls_label must then be None.  The label is the candidate
        selected by the call's own focus (ops.mask_candidates, unpinned: of the instances that contain the gaze pixel the smallest,
        else the nearest within cand_snap_px pixels, None meaning any distance): after predict_instances one
        ops.mask_candidates(..., pred=the record's bits) and one ops.mask_pair_counts(the record's bits, the selected words, d)
        follow, without a host read.  Returns (cat, stats, counts, conf[, comp], pair, sel): sel (B,8) int64 as ops.mask_candidates'
        -- sel[:, 1] is the class train.InstanceAPMeter needs, sel[:, 0] the selected row, sel[:, 6] the row that overlaps the
        record best; an image whose gaze selects nothing has |g| = 0.  Without the keyword every call and result is what it was."""
        if candidates is None:
            if cand_snap_px is not None:
                raise ValueError("cand_snap_px goes with candidates")
            if seg_label is None or cls_label is None:
                raise TypeError("evaluate_instances() needs seg_label and cls_label, or candidates=(cbits, cand_off, cand_cat)")
        if isinstance(boundary, bool) or not isinstance(boundary, float) or not (boundary > 0.0) or math.isinf(boundary):
            raise ValueError(f"boundary must be a finite float > 0, got {boundary!r}")
        if component is None:
            if snap_px is not None:
                raise ValueError("snap_px goes with component = 4 or 8")
        else:
            masks._component_args(component, snap_px)
        # each kind of label checks its own arguments and says how its bit words are made once the record's are there; nothing runs before
        if candidates is not None:
            if seg_label is not None or cls_label is not None:
                raise ValueError("with candidates the label is the selected candidate: seg_label and cls_label must be None")
            if not isinstance(candidates, (tuple, list)) or len(candidates) != 3:
                raise ValueError("candidates is a tuple (cbits, cand_off, cand_cat)")
            if seg_size is None or len(seg_size) != 2:
                raise ValueError("candidates need seg_size = (H, W): bit words do not carry their width")
            cbits, cand_off, cand_cat = candidates
            label_size = (int(seg_size[0]), int(seg_size[1]))
            masks._component_args(8, cand_snap_px)
            _N, Hc, _P, Bc = masks._candidate_args(cbits, cand_off, label_size[1], cand_cat)        # before the network runs
            if Hc != label_size[0] or Bc != img.shape[0]:
                raise ValueError(f"candidates of height {Hc} for {Bc} images do not go with seg_size {label_size} and img's batch size {img.shape[0]}")
            d = masks.boundary_dilation_capped(*label_size, boundary)

            def label_words(bits):                      # the candidate the gaze selects, and sel behind the pair
                gbits, sel, _cand = ops.mask_candidates(cbits, cand_off, focus, label_size[1], pred=bits, cand_cat=cand_cat, snap_px=cand_snap_px)
                return gbits, (sel,)
        elif isinstance(seg_label, (tuple, list)):
            if len(seg_label) != 2:
                raise ValueError(f"a run-length label is a tuple (counts, n_runs), got {len(seg_label)} elements")
            if seg_size is None or len(seg_size) != 2:
                raise ValueError("a run-length label needs seg_size = (H, W): the code does not carry its size")
            counts, n_runs = seg_label
            label_size = (int(seg_size[0]), int(seg_size[1]))
            if not isinstance(counts, torch.Tensor) or counts.dim() != 2 or counts.shape[0] != img.shape[0] or cls_label.shape[0] != img.shape[0]:
                raise ValueError(f"counts {tuple(getattr(counts, 'shape', ()))} and cls_label {tuple(cls_label.shape)} must have img's batch size "
                                 f"{img.shape[0]}")
            d = masks.boundary_dilation_capped(*label_size, boundary)
            masks._rle_args(counts, n_runs, label_size)                             # other dtypes and shapes raise before the network runs

            def label_words(bits):
                return ops.rle_bits(counts, n_runs, label_size)[0], ()
        else:
            if seg_label.dim() not in (3, 4) or (seg_label.dim() == 4 and seg_label.shape[1] != 1):
                raise ValueError(f"seg_label must be (B,H,W) or (B,1,H,W), got {tuple(seg_label.shape)}")
            label_size = (int(seg_label.shape[-2]), int(seg_label.shape[-1]))
            if seg_size is not None and (len(seg_size) != 2 or (int(seg_size[0]), int(seg_size[1])) != label_size):
                raise ValueError(f"seg_size {tuple(seg_size)} differs from the label's size {label_size}: the counters are taken pixel against pixel")
            if seg_label.shape[0] != img.shape[0] or cls_label.shape[0] != img.shape[0]:
                raise ValueError(f"seg_label {tuple(seg_label.shape)} and cls_label {tuple(cls_label.shape)} must have img's batch size {img.shape[0]}")
            d = masks.boundary_dilation_capped(*label_size, boundary)

            def label_words(bits):
                y = seg_label.reshape(seg_label.shape[0], *label_size)
                # seg_label.long() != 0 without the int64 copy: truncation towards 0 keeps what is at least 1 in magnitude (NaN: unset)
                return ops.mask_bits((y >= 1) | (y <= -1) if y.is_floating_point() else y != 0), ()
        out = self.predict_instances(img, focus, label_size, max_runs=max_runs, return_bits=True, return_score=True, component=component,
                                     snap_px=snap_px)
        label, extra = label_words(out[3])                                          # behind the network's peak
        pair = ops.mask_pair_counts(out[3], label, d, Ws=label_size[1])
        return out[:3] + out[4:] + (pair,) + extra

    @torch.no_grad()
    def evaluate(self, img, focus, seg_label, cls_label, seg_size=None, return_labels=False, class_areas=False, hausdorff=None, trimap=None, trimap_frame=True):
        """Full-resolution scoring without the loss: predict's stages, then the four accuracies of forward's MODEL.upsample branch
        (models/models.py:378-474,869-873,1074-1083) taken against the label in the pass that would have written the class map
        (ops.unwarp_accuracy / fs_unwarp_accuracy): no (B,K,H,W) prediction, no class map and no ground-truth tensor exist.

        img (B,3,H,W), focus (B,2) as predict's; seg_label (B,H,W) or (B,1,H,W) the label mask as fed to forward, cls_label (B,) or
        (B,1) the gazed instance's class.  Returns (acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg, counts): four 0-d fp32 tensors, the
        batch means forward(is_inference=True) reports, and counts (B,6) int64 = cls_fg, bin_fg, union_fg, cls_bg, bin_bg, union_bg per
        image (train.FullResMeter accumulates them into dataset-level scores); with return_labels, predict's class map as a sixth
        element.  seg_size defaults to the label's size and may not differ from it.  Eval mode only; no argument is written to,
        nothing in the module changes, and a NaN saliency map is reported as in predict.

        trimap (None, or VAL.trimap_dia_factor: an int 0 .. 7) adds the reference's trimap boundary accuracy (eval.py:41-67), counted
        in the same pass (ops.unwarp_trimap): the last element of the result is then trim (B, trimap + 1, 3) int64 = per image and band
        the pixels in the band, those with the right class, those right on foreground versus background.  Band i is every pixel within
        2**i city-block steps of the label's boundary -- the background pixels that touch the foreground and, with trimap_frame (the
        reference's PIL filter, bit for bit), the background pixels of the image's outer ring; trimap_frame=False reads the boundary
        alone.  Constant-label rule: an image without any boundary pixel (a constant label with trimap_frame=False, an all-foreground
        one with it) has empty bands and all-zero counters -- the reference divides 0 by 0 there -- and ops.trimap_from_counts /
        train.TrimapMeter leave it out of the mean.  With trimap=None the call is unchanged.

        class_areas=True adds the per-class areas of the reference's evaluation summary (eval.py:218-257,313-322; utils.py:289-317),
        counted in the same pass (ops.unwarp_class_areas): the LAST element of the result, after labels and trim where those are
        present, is then areas (B, 3, num_class, 3) int64 = per image, space and class (inter, pred, lab), union = pred + lab - inter.
        Space 0 scores the full-resolution prediction (the paper's IoU / Dice, VAL.report_per_img_iou per image), space 1 the sampling
        ceiling (VAL.y_sampled_reverse, IoU(Y', Y): every pixel takes the sampled label of the grid point that feeds it -- what a
        perfect network behind this sampler would score), space 2 the prediction in the sampled space (Mean IoU_deformed); the lab
        rows of spaces 0 and 2 are the label distribution before and after sampling.  ops.class_scores_from_areas makes IoU and Dice,
        train.ClassIoUMeter the dataset-level summary.  With the default the call, its result and its launches are unchanged.

        hausdorff (None, or the percentile: an int 1 .. 100, 95 for VAL.hd95) adds the surface-distance statistics of ops.surface_hd
        for the predicted foreground (class != num_class - 1) against the label's (seg_label.long() != 0): the LAST element of the
        result, after labels, trim and areas where those are present, is then hd (B,4) int64 = (n_pred, n_label, d2_lo, d2_hi) -- the
        two borders' sizes and the two pooled squared distances np.percentile interpolates between, -1 where a border is empty.
        ops.hd_from_stats makes the distance in pixels, train.HausdorffMeter the dataset mean.  It is the published 2-D definition,
        not what the reference's uncalled utils.hd95 returns.  With the default the call is unchanged."""
        if seg_label.dim() not in (3, 4) or (seg_label.dim() == 4 and seg_label.shape[1] != 1):
            raise ValueError(f"seg_label must be (B,H,W) or (B,1,H,W), got {tuple(seg_label.shape)}")
        label_size = (int(seg_label.shape[-2]), int(seg_label.shape[-1]))
        if seg_size is not None and (len(seg_size) != 2 or (int(seg_size[0]), int(seg_size[1])) != label_size):
            raise ValueError(f"seg_size {tuple(seg_size)} differs from the label's size {label_size}: the accuracies are taken pixel against pixel")
        if seg_label.shape[0] != img.shape[0] or cls_label.shape[0] != img.shape[0]:
            raise ValueError(f"seg_label {tuple(seg_label.shape)} and cls_label {tuple(cls_label.shape)} must have img's batch size {img.shape[0]}")
        cls, m, grid, _ = self._head_parts(img, focus, label_size, "evaluate")
        counts, acc, areas, trim, labels, hd = ops.unwarp_count(cls, m, grid, seg_label, cls_label, dia_factor=trimap, frame=trimap_frame,
                                                                areas=class_areas, return_labels=return_labels, hd_q=hausdorff)
        return (acc[0], acc[1], acc[2], acc[3], counts) + tuple(t for t in (labels, trim, areas, hd) if t is not None)

    def forward(self, feed_dict, *, writer=None, segSize=None, F_Xlr_acc_map=False, count=None, epoch=None,
                feed_dict_info=None, feed_batch_count=None, cur_iter=None, is_inference=False, rank=None):
        self.check_nan()
        ops.reset_step_state()
        ops.DDP_ACTIVE = ops.under_torch_ddp(self)      # wrapped by torch DDP: weight gradients go through AccumulateGrad (ops.py)
        if segSize is not None:
            raise NotImplementedError("forward(segSize=...): the reference has no inference branch left either -- its forward body is one "
                                      "`if segSize is None:` block (models/models.py:828-1094) and falls off the end, returning None, which its only "
                                      "caller (eval.py:178-180) cannot unpack; use is_inference=True (train.eval_step) for evaluation")
        cfg = self.cfg
        x = feed_dict["img_data"].contiguous()
        y = feed_dict["seg_label"]
        if y.dim() == 3:
            y = y.unsqueeze(1)
        y = y.float().contiguous()
        focus = feed_dict["focus_point"].float().contiguous()
        hs, ws = self.grid_size_x, self.grid_size_y

        xs, _ = self.saliency(x, focus)
        self._note_nan(xs)
        xs = ops.grad_probe(xs, "dxs_sum")                              # (ops.GRAD_TRACE: no-ops unless a test switched the recorder on)
        xs_grid = xs
        if cfg.MODEL.uniform_sample != "":
            # models/models.py:816-818 ('Saliency', config/defaults.py:69): the sampler runs on a uniform map; the edge loss keeps the learned
            # one (xs_our is cloned at :726, before this line) and the grid path hands the saliency net a zero gradient (d(xs*0)/dxs)
            xs_grid = xs * 0 + 1.0 / (self.grid_size_x * self.grid_size_y)
        grid = ops.grad_probe(self.create_grid(ops.grad_probe(xs_grid, "dxs_grid", alias=True)), "dgrid")

        joint = cfg.TRAIN.deform_joint_loss
        if joint:
            target = ops.area_pool(y, hs, ws)
            edge_loss = ops.EdgeLoss.apply(ops.grad_probe(xs, "dxs_edge", alias=True), target, 0.05 * float(cfg.TRAIN.edge_loss_scale))

        label = ops.grid_sample_label(y, grid.detach())
        x_sampled = ops.grad_probe(ops.GridSample.apply(x, grid), "dx_sampled")      # (B,hs,ws,3) NHWC
        feat = self.encoder.forward_nhwc(x_sampled)
        if cfg.MODEL.upsample:
            # the head's two factors feed the full-resolution accuracies below; the prediction is decoder.forward_nhwc's
            head_cls, head_m = self.decoder.forward_parts_nhwc(feat)
            pred = ops.PredAssemble.apply(head_cls, head_m)
        else:
            pred = self.decoder.forward_nhwc(feat)                     # (B,K,hs,ws)
        feed_dict["seg_label"] = label                                  # models/models.py:951

        cls = feed_dict["cls_label"].to(label.dtype)
        gt = label * cls[:, :, None] + (1 - label) * (cfg.DATASET.num_class - 1)
        out = ops.SegLoss.apply(pred, gt.contiguous(), 5.0)
        loss = out[0]
        if joint:
            loss = loss + edge_loss
        acc = out[3].detach()
        accs = (out[4].detach(), out[5].detach(), out[6].detach())
        if cfg.MODEL.upsample:
            # models/models.py:869-873,933-940,1074-1083: the loss stays at the sampled resolution, the four accuracies are taken at
            # FULL resolution on the prediction warped back through the inverse grid (never-claimed pixels filled from their
            # nearest claimed neighbour) against the original label map.  No gradient flows through this branch.  The class of a
            # pixel is one grid point's decision and its ground truth one read of y, so the counters are taken in one gather pass
            # (ops.unwarp_accuracy) instead of unwarp_nearest + SegLoss on a (B,K,H,W) prediction.
            with torch.no_grad():
                _counts, full = ops.unwarp_accuracy(head_cls.detach(), head_m.detach(), grid.detach(), y, cls)
                acc, accs = full[0], (full[1], full[2], full[3])
        if joint:
            if not is_inference:
                return loss, acc, edge_loss
            return loss, acc, edge_loss, accs[0], accs[1], accs[2]
        if not is_inference:
            return loss, acc
        return loss, acc, accs[0], accs[1], accs[2]
