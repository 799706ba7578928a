"""RPNHead on the HIP engine - the producer of the `rois` that `SingleRoIExtractor` consumes, in every reference config
(configs/_base_/models/cascade_rcnn_hrfuser_fpn_*_fusion.py:132-147; two_stage.py: extract_feat -> rpn_head -> roi_head).

Drop-in for mmdet's `RPNHead` (mmdet/models/dense_heads/rpn_head.py) at test time: same registry name, constructor keywords
and state-dict keys (`rpn_conv.*`, `rpn_cls.*`, `rpn_reg.*`).  Eval / forward only: there is no tape, `loss` raises.

  forward      3x3 conv 256 -> 256 on the wide packed engine (hrf_conv3_pack + hrf_conv3_packed, the launches of
               neck._conv3_wide), one ReLU launch (hrf_affine_act_res), and BOTH 1x1 convolutions as ONE padded row GEMM
               (hrf_rowgemm over a packed copy of rpn_cls / rpn_reg weights, A + 4A -> 16 columns): cls and reg are column
               slices of one [B][H][W][16] buffer, which the proposal kernels read in place (row pitch 16).
  proposals    csrc/hrf_rpn.h in four launches: per-level top-k + decode, per-level NMS (bit matrix + one wave per level),
               merge.  Fixed-shape outputs (dets, count, rois), no host read, no synchronisation: capturable in a hipGraph.
  get_bboxes   mmdet's return type - a list of (n_i, 5) - which slices by `count` and therefore SYNCHRONISES.

Three functional entries underneath (`select_decode`, `nms_segments`, `rpn_proposals`) take NHWC maps / candidate rows
directly.  There is no CPU fallback.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from .registry import HEADS

MAX_PRE = _lib._header_int('HRF_RPN_MAX_PRE', 2048)
MAX_LEVELS = _lib._header_int('HRF_RPN_MAX_LEVELS', 5)
MAX_ANCHORS = _lib._header_int('HRF_RPN_MAX_ANCHORS', 3)


def _rows(t, C, what):
    """logical NCHW fp32 (B,C,H,W) -> (B,H,W,C) view whose [B][H][W] rows share one pitch: channels-last storage (also a
    channel slice of a wider NHWC buffer) in place, anything else through ONE copy."""
    if t.dtype != torch.float32:
        raise TypeError(f'{what}: fp32 maps only, got {t.dtype}')
    if t.dim() != 4 or t.shape[1] != C:
        raise ValueError(f'{what}: expected (B, {C}, H, W), got {tuple(t.shape)}')
    v = t.detach().permute(0, 2, 3, 1)
    H, W = v.shape[1], v.shape[2]
    ld = v.stride(2)
    if not (v.stride(3) == 1 and ld >= C and v.stride(1) == W * ld and v.stride(0) == H * W * ld):
        v = v.contiguous()
    return v


def _levels(cls_maps, reg_maps, strides, bases):
    """hrf_rpn_levels_t over NHWC views (B,H,W,A) / (B,H,W,4A) (see _rows)."""
    lv = _lib.RpnLevels()
    B, A = cls_maps[0].shape[0], cls_maps[0].shape[3]
    lv.num_levels, lv.A, lv.B = len(cls_maps), A, B
    for l, (c, r) in enumerate(zip(cls_maps, reg_maps)):
        if c.shape[:3] != r.shape[:3] or c.shape[0] != B or c.shape[3] != A or r.shape[3] != 4 * A:
            raise ValueError(f'rpn: level {l} has cls {tuple(c.shape)} / reg {tuple(r.shape)} (NHWC), expected B = {B}, A = {A}')
        lv.cls[l], lv.reg[l] = c.data_ptr(), r.data_ptr()
        lv.H[l], lv.W[l] = c.shape[1], c.shape[2]
        lv.ld_cls[l], lv.ld_reg[l] = c.stride(2), r.stride(2)
        lv.stride[l] = int(strides[l])
        for a in range(A):
            for k in range(4):
                lv.base_anchors[(l * MAX_ANCHORS + a) * 4 + k] = float(bases[l][a][k])
    return lv


def _cfg(nms_pre, max_per_img, iou_thr, min_bbox_size):
    c = _lib.RpnCfg()
    c.nms_pre, c.max_per_img, c.iou_thr, c.min_bbox_size = int(nms_pre), int(max_per_img), float(iou_thr), float(min_bbox_size)
    return c


def _check(cls_maps, reg_maps, strides, bases):
    L = _lib.lib()
    if not 1 <= len(cls_maps) <= MAX_LEVELS or len(reg_maps) != len(cls_maps) or len(strides) != len(cls_maps) or len(bases) != len(cls_maps):
        raise ValueError(f'rpn: 1..{MAX_LEVELS} levels with cls, reg, stride and base anchors each, got {len(cls_maps)} / '
                         f'{len(reg_maps)} / {len(strides)} / {len(bases)}')
    A = cls_maps[0].shape[3]
    if not 1 <= A <= MAX_ANCHORS:
        raise NotImplementedError(f'rpn on the HIP engine: {A} base anchors per position are not built (1..{MAX_ANCHORS})')
    for t in tuple(cls_maps) + tuple(reg_maps):
        if L.require_cuda and not t.is_cuda:
            raise _lib.HRFuserHipError(f'rpn: tensor on {t.device}; the HIP path has no CPU fallback')
    return L


def _shapes(img_shapes, B, dev):
    """(B,2) fp32 device tensor of (h, w): given as one, or a list of (h, w[, c])"""
    if isinstance(img_shapes, torch.Tensor):
        t = img_shapes
        if t.shape != (B, 2) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f'rpn: img_shapes tensor must be contiguous fp32 ({B}, 2) on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}')
        return t
    if len(img_shapes) != B:
        raise ValueError(f'rpn: {len(img_shapes)} image shapes for a batch of {B}')
    return torch.tensor([[float(s[0]), float(s[1])] for s in img_shapes], dtype=torch.float32).to(dev)


def candidate_rows(cls_maps, nms_pre):
    """k_l = min(nms_pre, H W A) per level"""
    return [min(int(nms_pre), m.shape[1] * m.shape[2] * m.shape[3]) for m in cls_maps]


def select_decode(cls_maps, reg_maps, img_shapes, strides, bases, nms_pre, min_bbox_size=0.0, want_idx=False, stream=None):
    """Stage 1 alone (hrf_rpn_select_decode) on NHWC views -> cand (B,K,5), valid (B,K) int32[, idx (B,K) int32]; K = sum k_l."""
    L = _check(cls_maps, reg_maps, strides, bases)
    dev, B = cls_maps[0].device, cls_maps[0].shape[0]
    K = sum(candidate_rows(cls_maps, nms_pre))
    cand = torch.empty((B, K, 5), device=dev, dtype=torch.float32)
    valid = torch.empty((B, K), device=dev, dtype=torch.int32)
    idx = torch.empty((B, K), device=dev, dtype=torch.int32) if want_idx else None
    L.hrf_rpn_select_decode(_levels(cls_maps, reg_maps, strides, bases), _cfg(nms_pre, 1, 0.5, min_bbox_size), _shapes(img_shapes, B, dev),
                            cand, valid, idx, _lib.stream_ptr() if stream is None else stream)
    return (cand, valid, idx) if want_idx else (cand, valid)


def _outputs(B, max_per_img, dev):
    return (torch.empty((B, max_per_img, 5), device=dev, dtype=torch.float32), torch.empty((B,), device=dev, dtype=torch.int32),
            torch.empty((B * max_per_img, 5), device=dev, dtype=torch.float32))


def nms_segments(cand, valid, seg_len, max_per_img, iou_thr, apply_sigmoid=False, workspace=None, stream=None):
    """Stages 2 + 3 on explicit rows (hrf_nms_segments): cand (B,K,5) = (x1, y1, x2, y2, score), K = sum(seg_len), every segment
    in descending score order; valid (B,K) int32 or None -> dets (B,max_per_img,5), count (B,) int32, rois (B*max_per_img,5)."""
    L = _lib.lib()
    if cand.dim() != 3 or cand.shape[2] != 5 or cand.shape[1] != sum(seg_len) or cand.dtype != torch.float32 or not cand.is_contiguous():
        raise ValueError(f'nms_segments: cand must be contiguous fp32 (B, {sum(seg_len)}, 5), got {tuple(cand.shape)} {cand.dtype}')
    if valid is not None and (valid.shape != cand.shape[:2] or valid.dtype != torch.int32 or not valid.is_contiguous()):
        raise ValueError(f'nms_segments: valid must be contiguous int32 {tuple(cand.shape[:2])}, got {tuple(valid.shape)} {valid.dtype}')
    B, dev = cand.shape[0], cand.device
    lens = (ctypes.c_int * len(seg_len))(*[int(n) for n in seg_len])
    need = L.hrf_nms_workspace_bytes(lens, len(seg_len), B)
    if workspace is None:
        workspace = torch.empty((max(need, 256),), device=dev, dtype=torch.uint8)
    dets, count, rois = _outputs(B, max_per_img, dev)
    L.hrf_nms_segments(cand, valid, lens, len(seg_len), B, int(max_per_img), float(iou_thr), int(bool(apply_sigmoid)), workspace,
                       workspace.numel(), dets, count, rois, _lib.stream_ptr() if stream is None else stream)
    return dets, count, rois


def rpn_proposals(cls_maps, reg_maps, img_shapes, strides, bases, nms_pre, max_per_img, iou_thr=0.7, min_bbox_size=0.0, workspace=None,
                  stream=None):
    """All three stages (hrf_rpn_proposals) on NHWC views -> dets (B,max_per_img,5), count (B,) int32, rois (B*max_per_img,5)."""
    L = _check(cls_maps, reg_maps, strides, bases)
    dev, B = cls_maps[0].device, cls_maps[0].shape[0]
    lv, cfg = _levels(cls_maps, reg_maps, strides, bases), _cfg(nms_pre, max_per_img, iou_thr, min_bbox_size)
    if not L.hrf_rpn_supported(lv, cfg):
        raise NotImplementedError(f'rpn_proposals on the HIP engine: nms_pre {nms_pre} (1..{MAX_PRE}), max_per_img {max_per_img} (>= 1), '
                                  f'iou_threshold {iou_thr} (0 < t <= 1), min_bbox_size {min_bbox_size} (>= 0) or the maps are not supported')
    need = L.hrf_rpn_workspace_bytes(lv, cfg)
    if workspace is None:
        workspace = torch.empty((need,), device=dev, dtype=torch.uint8)
    dets, count, rois = _outputs(B, int(max_per_img), dev)
    L.hrf_rpn_proposals(lv, cfg, _shapes(img_shapes, B, dev), workspace, workspace.numel(), dets, count, rois,
                        _lib.stream_ptr() if stream is None else stream)
    return dets, count, rois


def _not_built(key, value, why):
    return NotImplementedError(f'RPNHead on the HIP engine: {key}={value!r} is not built ({why})')


@HEADS.register_module()
class RPNHead(nn.Module):
    """rpn_head.py:13-235 / anchor_head.py:43-107 at test time.  `feats`: the pyramid (logical NCHW, finest first)."""

    def __init__(self, in_channels, feat_channels=256, anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0],
                                                                              strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=(.0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0)),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0), loss_bbox=None, train_cfg=None, test_cfg=None,
                 init_cfg=dict(type='Normal', layer='Conv2d', std=0.01), num_convs=1, reg_decoded_bbox=False):
        super().__init__()
        ag, bc = dict(anchor_generator), dict(bbox_coder)
        if ag.pop('type', None) != 'AnchorGenerator':
            raise _not_built('anchor_generator.type', anchor_generator.get('type'), 'AnchorGenerator in every HRFuser config')
        if bc.pop('type', None) != 'DeltaXYWHBBoxCoder':
            raise _not_built('bbox_coder.type', bbox_coder.get('type'), 'DeltaXYWHBBoxCoder in every HRFuser config')
        means, stds = bc.pop('target_means', (0., 0., 0., 0.)), bc.pop('target_stds', (1., 1., 1., 1.))
        if any(float(m) != 0.0 for m in means):
            raise _not_built('bbox_coder.target_means', means, 'the kernel decodes with means 0')
        if any(float(s) != 1.0 for s in stds):
            raise _not_built('bbox_coder.target_stds', stds, 'the kernel decodes with stds 1')
        for k, dflt in (('clip_border', True), ('add_ctr_clamp', False), ('ctr_clamp', 32)):
            if bc.pop(k, dflt) != dflt:
                raise _not_built('bbox_coder.' + k, bbox_coder[k], f'{dflt!r}, the default')
        if bc:
            raise _not_built('bbox_coder keys', sorted(bc), 'unknown to the kernel')
        strides, ratios, scales = ag.pop('strides'), ag.pop('ratios'), ag.pop('scales', None)
        if ag.pop('center_offset', 0.0) != 0:
            raise _not_built('anchor_generator.center_offset', anchor_generator['center_offset'], '0 in every HRFuser config')
        if scales is None or ag.pop('scale_major', True) is not True or ag.pop('base_sizes', None) is not None or ag.pop('centers', None) is not None \
                or ag.pop('octave_base_scale', None) is not None or ag.pop('scales_per_octave', None) is not None or ag:
            raise _not_built('anchor_generator', anchor_generator, 'only strides / ratios / scales / center_offset=0 are')
        if any(not isinstance(s, int) or s < 1 for s in strides) or len(strides) > MAX_LEVELS:
            raise _not_built('anchor_generator.strides', strides, f'1..{MAX_LEVELS} square integer strides')
        if len(ratios) * len(scales) > MAX_ANCHORS:
            raise _not_built('anchor_generator ratios x scales', (ratios, scales), f'more than {MAX_ANCHORS} base anchors')
        if not dict(loss_cls or {}).get('use_sigmoid', False):
            raise _not_built('loss_cls.use_sigmoid', False, 'one sigmoid logit per anchor in every HRFuser config')
        if num_convs != 1:
            raise _not_built('num_convs', num_convs, '1 in every HRFuser config')
        if reg_decoded_bbox:
            raise _not_built('reg_decoded_bbox', reg_decoded_bbox, 'a training-only switch')
        if test_cfg is not None:
            self._proposal_cfg(test_cfg)                       # an unsupported nms type raises at build time
        from .testing import rpn_base_anchors
        self.in_channels, self.feat_channels, self.num_convs = in_channels, feat_channels, num_convs
        self.anchor_generator, self.bbox_coder = dict(anchor_generator), dict(bbox_coder)
        self.loss_cls, self.loss_bbox, self.train_cfg, self.test_cfg, self.init_cfg = loss_cls, loss_bbox, train_cfg, test_cfg, init_cfg
        self.strides = list(strides)
        self.base_anchors = [rpn_base_anchors(s, scales, ratios) for s in strides]     # base_sizes = strides (anchor_generator.py:85-86)
        self.num_base_priors = self.num_anchors = len(ratios) * len(scales)
        self.use_sigmoid_cls, self.cls_out_channels, self.num_classes = True, 1, 1
        self.fp16_enabled = False
        self.rpn_conv = nn.Conv2d(in_channels, feat_channels, 3, padding=1)
        self.rpn_cls = nn.Conv2d(feat_channels, self.num_base_priors, 1)
        self.rpn_reg = nn.Conv2d(feat_channels, self.num_base_priors * 4, 1)
        self.init_weights()
        self.__dict__['_packs'] = {}

    def init_weights(self):
        """init_cfg Normal(layer Conv2d, std 0.01), bias 0 (rpn_head.py:26)."""
        std = float(dict(self.init_cfg or {}).get('std', 0.01))
        for m in (self.rpn_conv, self.rpn_cls, self.rpn_reg):
            nn.init.normal_(m.weight, mean=0.0, std=std)
            nn.init.constant_(m.bias, 0)

    @staticmethod
    def _proposal_cfg(cfg):
        """-> (nms_pre, max_per_img, iou_threshold, min_bbox_size) of a test_cfg / proposal cfg dict"""
        nms = dict(cfg.get('nms', {}))
        if nms.get('type', 'nms') != 'nms':
            raise _not_built('nms.type', nms.get('type'), "'nms' in every HRFuser config; soft_nms and nms_match are not")
        if nms.get('split_thr') is not None or nms.get('class_agnostic', False):
            raise _not_built('nms', nms, 'levels are always separate NMS problems')
        return int(cfg.get('nms_pre', -1)), int(cfg.get('max_per_img', -1)), float(nms.get('iou_threshold', 0.7)), float(cfg.get('min_bbox_size', 0))

    # -- execution ----------------------------------------------------------------------------------
    def _packed(self, dev):
        """packed weights of the three convolutions, refreshed when a parameter changed (its version counter or storage)"""
        ps = (self.rpn_conv.weight, self.rpn_conv.bias, self.rpn_cls.weight, self.rpn_cls.bias, self.rpn_reg.weight, self.rpn_reg.bias)
        tag = tuple((p.data_ptr(), p._version) for p in ps) + (str(dev),)
        pk = self.__dict__['_packs']
        if pk.get('tag') != tag:
            L, s = _lib.lib(), _lib.stream_ptr()
            F, C, A = self.feat_channels, self.in_channels, self.num_base_priors
            w3 = torch.empty((9 * F * C,), device=dev, dtype=torch.float32)
            L.hrf_conv3_pack(self.rpn_conv.weight.detach(), F, C, 0, w3, s)
            both = torch.cat([self.rpn_cls.weight.detach().reshape(A, F), self.rpn_reg.weight.detach().reshape(4 * A, F)]).contiguous()
            w1 = torch.empty((16 * F,), device=dev, dtype=torch.float32)
            L.hrf_rowgemm_pack(both, 5 * A, F, 0, 16, F, w1, s)
            b1 = torch.zeros(16, device=dev, dtype=torch.float32)
            b1[:5 * A] = torch.cat([self.rpn_cls.bias.detach(), self.rpn_reg.bias.detach()])
            pk.update(tag=tag, w3=w3, w1=w1, b1=b1, b3=self.rpn_conv.bias.detach().contiguous(),
                      one=torch.ones(F, device=dev), zero=torch.zeros(F, device=dev))
        return pk

    def forward_single(self, x):
        """rpn_head.py:62-68 on one level -> (cls (B,A,H,W), reg (B,4A,H,W)): column slices of ONE NHWC buffer of pitch 16."""
        L, s = _lib.lib(), _lib.stream_ptr()
        F, C, A = self.feat_channels, self.in_channels, self.num_base_priors
        if C % 64 != 0 or F % 64 != 0 or F % 16 != 0:
            raise _not_built('in_channels / feat_channels', (C, F), 'the wide 3x3 engine takes multiples of 64; 256 in every HRFuser config')
        if L.require_cuda and not x.is_cuda:
            raise _lib.HRFuserHipError(f'RPNHead: tensor on {x.device}; the HIP path has no CPU fallback')
        xr = _rows(x, C, 'RPNHead.forward')
        if xr.stride(2) != C:
            xr = xr.contiguous()
        B, H, W, _ = xr.shape
        pk = self._packed(x.device)
        y = torch.empty((B, H, W, F), device=x.device, dtype=torch.float32)
        L.hrf_conv3_packed(xr, C, pk['w3'], pk['b3'], y, F, 0, B, H, W, C, F, s)
        z = torch.empty_like(y)
        L.hrf_affine_act_res(y, pk['one'], pk['zero'], None, None, None, None, None, H * W, 1, 0, z, B * H * W, F, None, 0.0, None, None, s)
        out = torch.empty((B, H, W, 16), device=x.device, dtype=torch.float32)
        L.hrf_rowgemm(z, F, pk['w1'], pk['b1'], out, 16, 0, B * H * W, F, 16, s)
        return out[..., :A].permute(0, 3, 1, 2), out[..., A:5 * A].permute(0, 3, 1, 2)

    def forward(self, feats):
        """anchor_head.py:136-157 -> (cls_scores, bbox_preds): two lists, one entry per level.  Eval only, no autograd."""
        if len(feats) > len(self.strides):
            raise ValueError(f'RPNHead: {len(feats)} maps, {len(self.strides)} anchor strides')
        with torch.no_grad():
            outs = [self.forward_single(x) for x in feats]
        return [o[0] for o in outs], [o[1] for o in outs]

    def proposals(self, cls_scores, bbox_preds, img_shapes, cfg=None):
        """-> (dets (B,max_per_img,5), count (B,) int32, rois (B*max_per_img,5)): fixed shapes, no synchronisation, capturable.
        img_shapes: a device fp32 tensor (B,2) of (h, w) - read by the kernel, a captured graph follows its contents - or a
        list of (h, w[, c]).  The maps are read in place when channels-last (what `forward` returns)."""
        cfg = self.test_cfg if cfg is None else cfg
        if cfg is None:
            raise ValueError('RPNHead.proposals: no cfg and the head was built without test_cfg')
        nms_pre, max_per_img, thr, min_size = self._proposal_cfg(cfg)
        if not 0 < nms_pre <= MAX_PRE:
            raise _not_built('nms_pre', nms_pre, f'1..{MAX_PRE}; 2000 / 1000 in every HRFuser config')
        if max_per_img < 1:
            raise _not_built('max_per_img', max_per_img, 'a fixed output shape needs a bound')
        if min_size < 0:
            raise _not_built('min_bbox_size', min_size, 'the filter is always applied; 0 in every HRFuser config')
        A, n = self.num_base_priors, len(cls_scores)
        cm = [_rows(t, A, 'RPNHead.proposals cls_scores') for t in cls_scores]
        rm = [_rows(t, 4 * A, 'RPNHead.proposals bbox_preds') for t in bbox_preds]
        bases = [b.tolist() for b in self.base_anchors[:n]]
        return rpn_proposals(cm, rm, img_shapes, self.strides[:n], bases, nms_pre, max_per_img, thr, min_size)

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False, with_nms=True):
        """base_dense_head.py:32-108 -> [(n_i, 5)] as mmdet returns.  Slices by `count`: this one SYNCHRONISES (use `proposals`
        inside a captured graph)."""
        if rescale or not with_nms:
            raise _not_built('rescale / with_nms', (rescale, with_nms), 'RPN proposals are never rescaled and always go through NMS')
        dets, count, _ = self.proposals(cls_scores, bbox_preds, [m['img_shape'] for m in img_metas], cfg)
        return [dets[b, :n] for b, n in enumerate(count.tolist())]

    def simple_test_rpn(self, x, img_metas):
        """dense_test_mixins.py:116-131."""
        return self.get_bboxes(*self.forward(x), img_metas=img_metas)

    def loss(self, *args, **kwargs):
        raise NotImplementedError('RPNHead on the HIP engine: loss is not built - the anchor assigner and sampler (train_cfg.assigner / '
                                  'sampler) are out of scope; the head is forward / proposals only')

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError('RPNHead on the HIP engine: forward_train is not built - the anchor assigner and sampler (train_cfg.'
                                  'assigner / sampler) are out of scope; the head is forward / proposals only')


def build_head(cfg):
    """mmdet.models.builder.build_head (builder.py:33-35)."""
    return HEADS.build(cfg)
