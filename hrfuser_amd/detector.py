"""Detector-level caller of the hot path: what `TwoStageDetector` does around backbone + neck.

Mirrors mmdet/models/detectors/two_stage.py: `combine_mod_imgs` (:9-19), `extract_feat` (:76-84), the sensor-keyword
entry of `forward_train` (:156-160) and the test-time list unwrapping of `simple_test` (:211-220).  Under a real
mmdet installation nothing here is needed - `TwoStageDetector` builds `backbone` / `neck` through the registries that
`import hrfuser_amd` re-populates and calls them exactly like this class does; stand-alone (this image
has no mmcv) `FeatureExtractor` is that caller, and `ExtractTrainer` is the data-parallel training step over BOTH
engines in one hipGraph: backbone tape -> neck tape -> neck backward -> backbone backward -> gradient exchange ->
fused AdamW on the two flat parameter arenas.
"""
import torch
import torch.nn as nn

from . import _lib
from . import runtime as R
from .registry import BACKBONES, HEADS, NECKS, ROI_EXTRACTORS
from .trainer import Trainer


def combine_mod_imgs(lidar_img=None, radar_img=None, gated_img=None):
    """two_stage.py:9-19 - fixed sensor order lidar, radar, gated; None when no modality is given."""
    mod_imgs = [m for m in (lidar_img, radar_img, gated_img) if m is not None]
    return mod_imgs if mod_imgs else None


class FeatureExtractor(nn.Module):
    """backbone (+ neck) of a `TwoStageDetector` config: `FeatureExtractor(cfg.model.backbone, cfg.model.neck)`;
    `bbox_roi_extractor` (optional): the `roi_head.bbox_roi_extractor` dict of the config (hrfuser_amd.roi); `rpn_head`
    (optional): the `rpn_head` dict of the config plus `test_cfg=cfg.model.test_cfg.rpn` (hrfuser_amd.rpn); `roi_head`
    (optional): the `roi_head` dict of the config plus `test_cfg=cfg.model.test_cfg.rcnn` (hrfuser_amd.roi_head) - with it and
    an rpn_head, `detect` / `simple_test` go from the images to detections."""

    def __init__(self, backbone, neck=None, bbox_roi_extractor=None, rpn_head=None, roi_head=None):
        super().__init__()
        self.backbone = BACKBONES.build(backbone) if isinstance(backbone, dict) else backbone      # two_stage.py:41
        if neck is not None:
            self.neck = NECKS.build(neck) if isinstance(neck, dict) else neck                       # two_stage.py:43-44
        if bbox_roi_extractor is not None:                                                          # standard_roi_head.py:25
            self.bbox_roi_extractor = (ROI_EXTRACTORS.build(bbox_roi_extractor) if isinstance(bbox_roi_extractor, dict)
                                       else bbox_roi_extractor)
        if rpn_head is not None:                                                                    # two_stage.py:46-50
            self.rpn_head = HEADS.build(rpn_head) if isinstance(rpn_head, dict) else rpn_head
        if roi_head is not None:                                                                    # two_stage.py:52-58
            self.roi_head = HEADS.build(roi_head) if isinstance(roi_head, dict) else roi_head

    @property
    def with_neck(self):
        return hasattr(self, 'neck') and self.neck is not None                                      # base.py:27-29

    @property
    def matrix_mode(self):
        """The neck's matrix mode (HRFPN.matrix_mode); 'fp32' without a neck."""
        return self.neck.matrix_mode if self.with_neck else 'fp32'

    def set_matrix_mode(self, mode):
        """HRFPN.set_matrix_mode of the neck (the backbone's engines are fp32 in either mode)."""
        if not self.with_neck:
            raise ValueError('FeatureExtractor.set_matrix_mode: no neck - the matrix mode belongs to HRFPN')
        self.neck.set_matrix_mode(mode)

    def extract_feat(self, img, mod_imgs=None):
        """two_stage.py:76-84."""
        if mod_imgs is not None:
            x = self.backbone(img, mod_imgs)
        else:
            x = self.backbone(img)             # camera-only backbones (HRFormer); HRFuser raises TypeError like the reference
        if self.with_neck:
            x = self.neck(x)
        return x

    def _proposals(self, x, img, img_shapes, cfg):
        if getattr(self, 'rpn_head', None) is None:
            raise ValueError('FeatureExtractor: built without an rpn_head')
        if img_shapes is None:
            img_shapes = [tuple(img.shape[-2:])] * img.shape[0]
        return self.rpn_head.proposals(*self.rpn_head(x), img_shapes, cfg)

    def extract_proposals(self, img, img_shapes=None, lidar_img=None, radar_img=None, gated_img=None, cfg=None):
        """extract_feat followed by the RPN head (two_stage.py:178-181 `rpn_head.simple_test_rpn(x, img_metas)`, with fixed
        shapes): -> (dets (B,max_per_img,5), count (B,) int32, rois (B*max_per_img,5)), no synchronisation.  img_shapes: (B,2)
        device tensor or list of (h, w[, c]); None: the padded input size."""
        x = self.extract_feat(img, mod_imgs=combine_mod_imgs(lidar_img, radar_img, gated_img))
        return self._proposals(x, img, img_shapes, cfg)

    def rpn_loss(self, img, gt_bboxes, img_metas=None, lidar_img=None, radar_img=None, gated_img=None):
        """extract_feat -> rpn_head -> loss (two_stage.py:163-172 `rpn_head.forward_train` without the proposals): mmdet's dict of
        per-level lists.  gt_bboxes / img_metas as RPNHead.loss takes them; img_metas None: every image has the padded input size.
        The head's forward is eval only, so the losses carry no gradient into the pyramid: the gradient maps on the head's outputs
        are what RPNHead.loss keeps."""
        if getattr(self, 'rpn_head', None) is None:
            raise ValueError('FeatureExtractor.rpn_loss: built without an rpn_head')
        x = self.extract_feat(img, mod_imgs=combine_mod_imgs(lidar_img, radar_img, gated_img))
        if img_metas is None:
            img_metas = [dict(img_shape=tuple(img.shape[-2:]), pad_shape=tuple(img.shape[-2:]))] * img.shape[0]
        return self.rpn_head.loss(*self.rpn_head(x), gt_bboxes, img_metas)

    def _roi_losses(self, x, outs, img, gt_bboxes, gt_labels, img_metas, proposal_cfg):
        if getattr(self, 'roi_head', None) is None or getattr(self, 'rpn_head', None) is None:
            raise ValueError('FeatureExtractor.roi_loss: built without an rpn_head / roi_head')
        from .rpn import _shapes
        shp = _shapes([m['img_shape'] for m in img_metas], img.shape[0], x[0].device)
        _, count, rois = self.rpn_head.proposals(*outs, shp, proposal_cfg)
        return self.roi_head.forward_train(x, img_metas, (rois, count), gt_bboxes, gt_labels)

    def roi_loss(self, img, gt_bboxes, gt_labels, img_metas=None, lidar_img=None, radar_img=None, gated_img=None, proposal_cfg=None):
        """extract_feat -> RPNHead.proposals -> CascadeRoIHead.forward_train (two_stage.py:163-177 without the RPN's own loss): mmdet's
        dict s{i}.loss_cls / s{i}.acc / s{i}.loss_bbox.  The proposals stay in their fixed shape (rois, count): nothing synchronises.
        gt_bboxes / gt_labels: lists per image; img_metas None: every image has the padded input size; proposal_cfg: train_cfg.rpn_proposal
        (None: the RPN head's test_cfg)."""
        x = self.extract_feat(img, mod_imgs=combine_mod_imgs(lidar_img, radar_img, gated_img))
        if img_metas is None:
            img_metas = [dict(img_shape=tuple(img.shape[-2:]), pad_shape=tuple(img.shape[-2:]))] * img.shape[0]
        if getattr(self, 'rpn_head', None) is None:
            raise ValueError('FeatureExtractor.roi_loss: built without an rpn_head')
        return self._roi_losses(x, self.rpn_head(x), img, gt_bboxes, gt_labels, img_metas, proposal_cfg)

    def roi_loss_backward(self, img, gt_bboxes, gt_labels, img_metas=None, lidar_img=None, radar_img=None, gated_img=None, proposal_cfg=None,
                          pyramid_grads=None):
        """`roi_loss` with its backward, on the explicit tapes: backbone tape -> neck tape -> rpn_head + proposals (no_grad) ->
        CascadeRoIHead.losses_nhwc on the neck's ctx -> neck backward -> backbone backward - the tape calls of
        ExtractTrainer._step_impl with the RoI losses in place of the synthetic cotangents.  Returns roi_loss's dict (the same
        values) and leaves d (sum of the s{i}.loss_cls / s{i}.loss_bbox) in the two flat gradient arenas (added to their
        contents, like .backward()) and in .grad of the head parameters.  No optimizer step, no gradient through the RPN head.
        pyramid_grads: a list that receives a copy of the gradient on every pyramid level (NHWC; None for an unused level)."""
        if getattr(self, 'roi_head', None) is None or getattr(self, 'rpn_head', None) is None or not self.with_neck:
            raise ValueError('FeatureExtractor.roi_loss_backward: built without a neck / rpn_head / roi_head')
        from .roi_head import pack_gt_labels
        from .rpn import _shapes, pack_gts
        mods = combine_mod_imgs(lidar_img, radar_img, gated_img) or []
        if img_metas is None:
            img_metas = [dict(img_shape=tuple(img.shape[-2:]), pad_shape=tuple(img.shape[-2:]))] * img.shape[0]
        dev = img.device
        gt, gt_count = pack_gts(gt_bboxes, dev)
        shp = _shapes([m['img_shape'] for m in img_metas], img.shape[0], dev)
        vals = self._roi_loss_backward(img, mods, gt, pack_gt_labels(gt_labels, dev, gt.shape[1]), gt_count, shp, proposal_cfg, pyramid_grads)
        out = {}
        for i in range(self.roi_head.num_stages):
            out[f's{i}.loss_cls'], out[f's{i}.acc'], out[f's{i}.loss_bbox'] = vals[i, 0], vals[i, 2], vals[i, 1]
        return out

    def _roi_loss_backward(self, img, mods, gt, gt_labels, gt_count, shp, proposal_cfg=None, pyramid_grads=None):
        """the device part of roi_loss_backward on packed ground truths (rpn.pack_gts, roi_head.pack_gt_labels) and the (B,2) shape
        tensor: fixed shapes, nothing read on the host - capturable -> the (num_stages, 3) values of CascadeRoIHead.losses"""
        net, neck = self.backbone, self.neck
        cb, outs, _ = net._execute((img,) + tuple(mods), True)
        en = neck._engine()
        en.ready(img.device)
        en.begin_forward(neck.training)
        cn = R.Ctx(neck, neck.training, True)
        with torch.no_grad():
            srcs = [R.Act(o.t, True) for o in outs]              # the backbone's NHWC maps, in place
            pyr = neck._run(cn, srcs)
            x = [p.t.permute(0, 3, 1, 2) for p in pyr]
            _, count, rois = self.rpn_head.proposals(*self.rpn_head(x), shp, proposal_cfg)
            vals, _ = self.roi_head.losses_nhwc(cn, pyr, rois, count, gt, gt_labels, gt_count, shp)
        cn.run_backward()
        if pyramid_grads is not None:
            pyramid_grads.extend(None if p.grad is None else p.grad.clone() for p in pyr)
        for o, s_ in zip(outs, srcs):
            o.grad = s_.grad
        cb.run_backward()
        return vals

    def losses(self, img, gt_bboxes, gt_labels, img_metas=None, lidar_img=None, radar_img=None, gated_img=None, proposal_cfg=None):
        """two_stage.py:163-177: the RPN's dict (loss_rpn_cls / loss_rpn_bbox per level) and the RoI head's (s{i}.*) merged, from
        ONE pass through the backbone, the neck and the RPN head."""
        if getattr(self, 'rpn_head', None) is None:
            raise ValueError('FeatureExtractor.losses: built without an rpn_head')
        x = self.extract_feat(img, mod_imgs=combine_mod_imgs(lidar_img, radar_img, gated_img))
        if img_metas is None:
            img_metas = [dict(img_shape=tuple(img.shape[-2:]), pad_shape=tuple(img.shape[-2:]))] * img.shape[0]
        outs = self.rpn_head(x)
        out = dict(self.rpn_head.loss(*outs, gt_bboxes, img_metas))
        out.update(self._roi_losses(x, outs, img, gt_bboxes, gt_labels, img_metas, proposal_cfg))
        return out

    def extract_roi_feats(self, img, rois=None, lidar_img=None, radar_img=None, gated_img=None, img_shapes=None):
        """extract_feat followed by the RoI extractor (standard_roi_head.py:116-118: `bbox_roi_extractor(x[:num_inputs],
        rois)`): rois (K,5) = (batch index, x1, y1, x2, y2) -> (K, out_channels, 7, 7).  rois None: the `rois` of the RPN head
        (B * max_per_img rows, the padded ones give rows of zeros)."""
        if getattr(self, 'bbox_roi_extractor', None) is None:
            raise ValueError('FeatureExtractor.extract_roi_feats: built without a bbox_roi_extractor')
        x = self.extract_feat(img, mod_imgs=combine_mod_imgs(lidar_img, radar_img, gated_img))
        if rois is None:
            rois = self._proposals(x, img, img_shapes, None)[2]
        return self.bbox_roi_extractor(x, rois)

    def detect(self, img, img_shapes=None, scale_factors=None, lidar_img=None, radar_img=None, gated_img=None):
        """The whole test-time forward with fixed shapes (two_stage.py:178-186 `rpn_head.simple_test_rpn` + `roi_head.simple_test`):
        extract_feat -> RPNHead.proposals -> CascadeRoIHead.detect -> (dets (B,max_per_img,5), labels (B,max_per_img) int32,
        count (B,) int32).  No synchronisation.  img_shapes: (B,2) device tensor or list of (h, w[, c]), None: the padded input
        size; scale_factors: (B,4) device tensor or list (boxes are divided by it), None: no rescale."""
        if getattr(self, 'roi_head', None) is None:
            raise ValueError('FeatureExtractor.detect: built without a roi_head')
        from .rpn import _shapes
        x = self.extract_feat(img, mod_imgs=combine_mod_imgs(lidar_img, radar_img, gated_img))
        if img_shapes is None:
            img_shapes = [tuple(img.shape[-2:])] * img.shape[0]
        shp = _shapes(img_shapes, img.shape[0], x[0].device)
        _, count, rois = self._proposals(x, img, shp, None)
        return self.roi_head.detect(x, rois, count, shp, scale_factors)

    def simple_test(self, img, img_metas, rescale=False, lidar_img=None, radar_img=None, gated_img=None):
        """two_stage.py:205-226 without precomputed proposals: per image a list of num_classes (n, 5) numpy arrays.  The
        modalities come wrapped in one-entry lists, as test pipelines deliver them.  SYNCHRONISES."""
        if getattr(self, 'roi_head', None) is None or getattr(self, 'rpn_head', None) is None:
            raise ValueError('FeatureExtractor.simple_test: built without an rpn_head / roi_head')
        x = self.simple_test_feats(img, lidar_img, radar_img, gated_img)
        proposal_list = self.rpn_head.simple_test_rpn(x, img_metas)
        return self.roi_head.simple_test(x, proposal_list, img_metas, rescale=rescale)

    def forward(self, img, lidar_img=None, radar_img=None, gated_img=None):
        """The feature part of forward_train (two_stage.py:156-160): sensors by keyword."""
        return self.extract_feat(img, mod_imgs=combine_mod_imgs(lidar_img, radar_img, gated_img))

    def simple_test_feats(self, img, lidar_img=None, radar_img=None, gated_img=None):
        """The feature part of simple_test (two_stage.py:211-220): test pipelines wrap every modality in a list
        (one entry per augmentation); `mod_imgs[i] = mod_imgs[i][0]` unwraps the single-scale case."""
        mod_imgs = combine_mod_imgs(lidar_img, radar_img, gated_img)
        if mod_imgs:
            mod_imgs = [m[0] for m in mod_imgs]
        return self.extract_feat(img, mod_imgs=mod_imgs)


class ExtractTrainer:
    """Training step over backbone + neck on the explicit tapes (no torch.autograd), capturable into one hipGraph.

    Same contract as `Trainer` (synthetic loss L = sum_i <pyramid_i, cot_i>, flat-arena gradient all-reduce, fused
    AdamW with the reference's `paramwise_cfg` decay mask), with the neck's arena exchanged and stepped beside the
    backbone's.  max_norm / norm_type / skip_nonfinite as for `Trainer`, with ONE norm over both arenas (mmcv clips the whole
    model at once): the two hrf_grad_sumsq launches fill one partials buffer, one hrf_adamw_tick_clip finalises it and both
    hrf_adamw_clipped launches read the same `clip`."""

    def __init__(self, feats, group=None, world_size=1, **opt):
        assert feats.with_neck
        self.feats = feats
        self.tb = Trainer(feats.backbone, group=group, world_size=world_size, **opt)
        self.tn = Trainer(feats.neck, group=group, world_size=world_size, **opt)
        self.clipping = self.tb.clipping
        self.clip = None                     # the device float[8] both arenas share (Trainer.clip)
        self.group, self.world = group, world_size
        self.graph = None
        self._graph_mm = None                # the neck's matrix mode the graph was captured in

    def _step_impl(self, x, mods, cots):
        net, neck = self.feats.backbone, self.feats.neck
        eb, en = net._engine(), neck._engine()
        if not self.tb._ready:
            self.tb._setup(x.device)
            self.tn._setup(x.device)
            if self.clipping:
                self.clip = self.tn.clip = self.tb.clip
                self._partials = torch.zeros(self.tb._nparts + self.tn._nparts, device=x.device, dtype=torch.float64)
        R.gpu_zero_(eb.flat_g)
        R.gpu_zero_(en.flat_g)
        cb, outs, _ = net._execute((x,) + tuple(mods), True)
        en.ready(x.device)
        en.begin_forward(True)
        cn = R.Ctx(neck, True, True)
        with torch.no_grad():
            srcs = [R.Act(o.t, True) for o in outs]              # the backbone's NHWC maps, in place
            pyr = neck._run(cn, srcs)
        for o, c in zip(pyr, cots):
            o.grad = R.gpu_clone(c)
        cn.run_backward()
        for o, s_ in zip(outs, srcs):
            o.grad = s_.grad
        cb.run_backward()
        L = _lib.lib()
        pairs = ((self.tb, eb), (self.tn, en))

        def exchange(tr, eng):
            if self.world > 1 or tr.force:
                import torch.distributed as dist
                for a, b in tr.buckets(eng.flat_g.numel()):
                    dist.all_reduce(eng.flat_g[a:b], group=self.group)
        if not self.clipping:
            for tr, eng in pairs:
                exchange(tr, eng)
                s = _lib.stream_ptr()
                L.hrf_adamw_tick(tr.state, tr.betas[0], tr.betas[1], s)
                L.hrf_adamw(eng.flat_p, eng.flat_g, tr.m, tr.v, tr.wd_mask, eng.flat_p.numel(), tr.lr, tr.betas[0],
                            tr.betas[1], tr.eps, tr.wd, tr.state, 1.0 / self.world, s)
        else:
            # one norm over both arenas: both exchanges first, the partial sums back to back, ONE finalize; the neck's step count
            # advances behind it under the same skip flag (nparts = 0)
            for tr, eng in pairs:
                exchange(tr, eng)
            s = _lib.stream_ptr()
            tb, tn = self.tb, self.tn
            L.hrf_grad_sumsq(eb.flat_g, tb.wd_mask, eb.flat_g.numel(), self._partials, s)
            L.hrf_grad_sumsq(en.flat_g, tn.wd_mask, en.flat_g.numel(), self._partials[tb._nparts:], s)
            L.hrf_adamw_tick_clip(tb.state, self.clip, self._partials, tb._nparts + tn._nparts, 1.0 / self.world,
                                  int(tb.skip_nonfinite), tb.betas[0], tb.betas[1], s)
            L.hrf_adamw_tick_clip(tn.state, self.clip, None, 0, 1.0 / self.world, int(tn.skip_nonfinite), tn.betas[0], tn.betas[1], s)
            for tr, eng in pairs:
                L.hrf_adamw_clipped(eng.flat_p, eng.flat_g, tr.m, tr.v, tr.wd_mask, eng.flat_p.numel(), tr.lr, tr.betas[0],
                                    tr.betas[1], tr.eps, tr.wd, tr.state, 1.0 / self.world, self.clip, s)
        net.params_updated()
        neck.params_updated()
        return pyr

    def step(self, x, mods, cots):
        return self._step_impl(x, mods, cots)

    def set_max_norm(self, max_norm):
        """Trainer.set_max_norm for the norm both arenas share (a captured graph follows it)."""
        self.tb.set_max_norm(max_norm)
        self.tn.max_norm = self.tb.max_norm

    def grad_norm(self):
        """Global L2 norm of the last step's averaged gradient over backbone AND neck, before clipping.  Synchronises."""
        return self.tb.grad_norm()

    def clip_coef(self):
        """Trainer.clip_coef of the shared norm.  Synchronises."""
        return self.tb.clip_coef()

    def skipped_steps(self):
        """Trainer.skipped_steps (both arenas skip together).  Synchronises."""
        return self.tb.skipped_steps()

    def capture(self, x, mods, cots, warmup=2):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._step_impl(x, mods, cots)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if self.world > 1 or self.tb.force:
            import os
            import time
            time.sleep(float(os.environ.get('HRF_CAPTURE_SETTLE', '1.0')))       # see Trainer.capture
        g = torch.cuda.CUDAGraph()
        with R.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
            self._graph_outs = self._step_impl(x, mods, cots)
        self.graph = g
        self._graph_mm = self.feats.neck.matrix_mode
        return g

    def replay(self):
        if self._graph_mm != self.feats.neck.matrix_mode:
            # (a graph replays the launches it recorded: the other mode's kernels are never reached through it)
            raise _lib.HRFuserHipError(f'ExtractTrainer.replay: this graph was captured in matrix mode {self._graph_mm!r}, the '
                                       f'neck is in {self.feats.neck.matrix_mode!r} now (set_matrix_mode) - capture again')
        self.graph.replay()


def make_pyramid_cotangents(feats, x, mods, seed=5):
    """Fixed random cotangents (NHWC) for the pyramid outputs, shaped by a dry eval forward."""
    was_b, was_n = feats.backbone.training, feats.neck.training
    feats.eval()
    with torch.no_grad():
        ys = feats.extract_feat(x, list(mods))
    feats.backbone.train(was_b)
    feats.neck.train(was_n)
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(tuple(y.permute(0, 2, 3, 1).shape), generator=g).to(x.device) / y.numel() for y in ys]
