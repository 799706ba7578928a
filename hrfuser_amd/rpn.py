"""RPNHead on the HIP engine - the producer of the `rois` that `SingleRoIExtractor` consumes, in every reference config
(configs/_base_/models/cascade_rcnn_hrfuser_fpn_*_fusion.py:132-147; two_stage.py: extract_feat -> rpn_head -> roi_head).

Drop-in for mmdet's `RPNHead` (mmdet/models/dense_heads/rpn_head.py) at test time: same registry name, constructor keywords
and state-dict keys (`rpn_conv.*`, `rpn_cls.*`, `rpn_reg.*`).  The forward is eval only (no tape for the head's own three
convolutions); with a `train_cfg` the head computes mmdet's RPN losses and their gradients on its output maps.

  forward      3x3 conv 256 -> 256 on the wide packed engine (hrf_conv3_pack + hrf_conv3_packed, the launches of
               neck._conv3_wide), one ReLU launch (hrf_affine_act_res), and BOTH 1x1 convolutions as ONE padded row GEMM
               (hrf_rowgemm over a packed copy of rpn_cls / rpn_reg weights, A + 4A -> 16 columns): cls and reg are column
               slices of one [B][H][W][16] buffer, which the proposal kernels read in place (row pitch 16).
  proposals    csrc/hrf_rpn.h in four launches: per-level top-k + decode, per-level NMS (bit matrix + one wave per level),
               merge.  Fixed-shape outputs (dets, count, rois), no host read, no synchronisation: capturable in a hipGraph.
  get_bboxes   mmdet's return type - a list of (n_i, 5) - which slices by `count` and therefore SYNCHRONISES.
  loss         csrc/hrf_rpn_train.h in six launches: IoU + argmax per anchor, the best IoU per gt, MaxIoUAssigner, the sampler's
               radix select, BCE-with-logits + SmoothL1 with their gradient maps, the per-level sums.  Fixed shapes, no host
               read: capturable.  The values reach torch.autograd through `_RpnLossFn`.

Five functional entries underneath (`select_decode`, `nms_segments`, `rpn_proposals`, `rpn_assign`, `rpn_loss`) take NHWC maps /
candidate rows directly.  There is no CPU fallback.
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


# ----------------------------------------------------------------------------- training targets and loss (csrc/hrf_rpn_train.h)
MAX_GT = _lib._header_int('HRF_RPN_MAX_GT', 256)
GRAD_PITCH = 16                                 # floats per position of a gradient buffer: cls in [:A], reg in [A:5A] - the dY of the head's row GEMM


def train_cfg_struct(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, allowed_border=0, num=256, num_pos=128,
                     beta=1.0 / 9.0, loss_weight_cls=1.0, loss_weight_bbox=1.0):
    """hrf_rpn_train_cfg_t; num_pos = int(num * pos_fraction)"""
    c = _lib.RpnTrainCfg()
    c.pos_iou_thr, c.neg_iou_thr, c.min_pos_iou = float(pos_iou_thr), float(neg_iou_thr), float(min_pos_iou)
    c.match_low_quality, c.allowed_border, c.num, c.num_pos = int(bool(match_low_quality)), int(allowed_border), int(num), int(num_pos)
    c.beta, c.loss_weight_cls, c.loss_weight_bbox = float(beta), float(loss_weight_cls), float(loss_weight_bbox)
    return c


def pack_gts(gt_bboxes, dev, gmax=None):
    """list of (n_i, 4) boxes -> (gt (B,Gmax,4) fp32, gt_count (B,) int32) on `dev`.  The counts are the shapes: no device value
    is read, nothing synchronises.  gmax: the fixed Gmax (a captured graph needs one), default max(n_i, 1)."""
    ns = [int(t.shape[0]) for t in gt_bboxes]
    gmax = max(ns + [1]) if gmax is None else int(gmax)
    if max(ns + [0]) > gmax or not 1 <= gmax <= MAX_GT:
        raise NotImplementedError(f'rpn on the HIP engine: {max(ns + [0])} ground-truth boxes in an image with Gmax {gmax} are not built (1..{MAX_GT})')
    gt = torch.zeros((len(ns), gmax, 4), device=dev, dtype=torch.float32)
    for b, t in enumerate(gt_bboxes):
        if ns[b]:
            gt[b, :ns[b]] = t.detach().reshape(-1, 4).to(device=dev, dtype=torch.float32)
    return gt, torch.tensor(ns, dtype=torch.int32).to(dev)


def rng_state(seed, counter=0, device='cpu'):
    """the (seed, counter) pair the kernels draw sampling keys from: int32 (2,) holding two uint32 values"""
    v = [int(x) & 0xffffffff for x in (seed, counter)]
    return torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in v], dtype=torch.int32).to(device)


def _train_args(cls_maps, reg_maps, img_shapes, pad_shapes, gt, gt_count, strides, bases, cfg, keys, rng, workspace):
    L = _check(cls_maps, reg_maps, strides, bases)
    dev, B = cls_maps[0].device, cls_maps[0].shape[0]
    N = sum(m.shape[1] * m.shape[2] * m.shape[3] for m in cls_maps)
    if gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != 4 or gt.dtype != torch.float32 or not gt.is_contiguous() or gt.device != dev:
        raise ValueError(f'rpn: gt must be contiguous fp32 ({B}, Gmax, 4) on {dev}, got {tuple(gt.shape)} {gt.dtype} on {gt.device}')
    if gt_count.shape != (B,) or gt_count.dtype != torch.int32 or gt_count.device != dev:
        raise ValueError(f'rpn: gt_count must be int32 ({B},) on {dev}, got {tuple(gt_count.shape)} {gt_count.dtype} on {gt_count.device}')
    if keys is not None and (keys.shape != (B, N) or keys.dtype != torch.int32 or not keys.is_contiguous() or keys.device != dev):
        raise ValueError(f'rpn: keys must be contiguous int32 ({B}, {N}) holding uint32 values on {dev}, got {tuple(keys.shape)} {keys.dtype}')
    if keys is None and (rng is None or rng.shape != (2,) or rng.dtype != torch.int32 or rng.device != dev):
        raise ValueError(f'rpn: without keys an int32 (2,) rng_state (seed, counter) on {dev} is needed (rpn.rng_state)')
    lv = _levels(cls_maps, reg_maps, strides, bases)
    gmax = gt.shape[1]
    if not L.hrf_rpn_train_supported(lv, cfg, gmax):
        raise NotImplementedError(f'rpn targets on the HIP engine: Gmax {gmax} (1..{MAX_GT}), thresholds ({cfg.pos_iou_thr}, {cfg.neg_iou_thr}, '
                                  f'{cfg.min_pos_iou}) in [0, 1], num {cfg.num} >= 1, num_pos {cfg.num_pos} in [0, num], beta {cfg.beta} > 0 or '
                                  'the maps are not supported')
    need = L.hrf_rpn_train_workspace_bytes(lv, cfg, gmax)
    if workspace is None:
        workspace = torch.empty((need,), device=dev, dtype=torch.uint8)
    outs = (torch.empty((B, N), device=dev, dtype=torch.int32), torch.empty((B, N), device=dev, dtype=torch.float32),
            torch.empty((B, N), device=dev, dtype=torch.int32), torch.empty((B, 4), device=dev, dtype=torch.int32))
    return L, lv, _shapes(img_shapes, B, dev), _shapes(pad_shapes, B, dev), gmax, workspace, outs


def rpn_assign(cls_maps, reg_maps, img_shapes, pad_shapes, gt, gt_count, strides, bases, cfg, keys=None, rng=None, workspace=None, stream=None):
    """hrf_rpn_assign on NHWC views: inside flags, MaxIoUAssigner, sampler -> (assigned (B,N) int32, max_iou (B,N) fp32,
    sampled (B,N) int32, counts (B,4) int32); N = the anchors of all levels, level after level.  cfg: train_cfg_struct(...);
    gt / gt_count: pack_gts(...); keys (B,N) int32 (uint32 values) or rng = rng_state(seed, counter) (not advanced here)."""
    L, lv, shp, pad, gmax, ws, outs = _train_args(cls_maps, reg_maps, img_shapes, pad_shapes, gt, gt_count, strides, bases, cfg, keys, rng, workspace)
    L.hrf_rpn_assign(lv, cfg, shp, pad, gt, gt_count, gmax, keys, rng, ws, ws.numel(), *outs, _lib.stream_ptr() if stream is None else stream)
    return outs


def rpn_loss(cls_maps, reg_maps, img_shapes, pad_shapes, gt, gt_count, strides, bases, cfg, keys=None, rng=None, workspace=None, stream=None,
             grads=None):
    """hrf_rpn_loss on NHWC views -> (losses (2,L) fp32: loss_cls per level, loss_bbox per level; grads: per level ONE zero-padded
    (B,H,W,16) buffer with d loss_cls_l / d cls in [..., :A] and d loss_bbox_l / d reg in [..., A:5A]; assigned, max_iou, sampled,
    counts as rpn_assign).  With rng (no keys) the counter is advanced on the device by the call.  grads: buffers of an earlier
    call to write into again (their padding columns are zero already) instead of new ones."""
    L, lv, shp, pad, gmax, ws, outs = _train_args(cls_maps, reg_maps, img_shapes, pad_shapes, gt, gt_count, strides, bases, cfg, keys, rng, workspace)
    dev, A = cls_maps[0].device, cls_maps[0].shape[3]
    if grads is None:
        grads = [torch.zeros(tuple(m.shape[:3]) + (GRAD_PITCH,), device=dev, dtype=torch.float32) for m in cls_maps]
    if any(g.shape != tuple(m.shape[:3]) + (GRAD_PITCH,) or g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev
           for g, m in zip(grads, cls_maps)) or len(grads) != len(cls_maps):
        raise ValueError(f'rpn_loss: grads must be contiguous fp32 (B, H, W, {GRAD_PITCH}) buffers on {dev}, one per level')
    gr = _lib.RpnGrads()
    for l, g in enumerate(grads):
        gr.d_cls[l], gr.d_reg[l] = g.data_ptr(), g.data_ptr() + 4 * A
        gr.ld_cls[l] = gr.ld_reg[l] = GRAD_PITCH
    losses = torch.empty((2, len(cls_maps)), device=dev, dtype=torch.float32)
    L.hrf_rpn_loss(lv, cfg, shp, pad, gt, gt_count, gmax, keys, rng, ws, ws.numel(), *outs, gr, losses, _lib.stream_ptr() if stream is None else stream)
    return (losses, grads) + outs


class _RpnLossFn(torch.autograd.Function):
    """torch.autograd bridge: any producer of cls_scores / bbox_preds trains against the HIP loss.  Forward runs hrf_rpn_loss and
    keeps the gradient maps; backward scales them by the incoming per-loss gradients."""

    @staticmethod
    def forward(fctx, call, A, *maps):
        n = len(maps) // 2
        losses, grads = call([_rows(t, A, 'RPNHead.loss cls_scores') for t in maps[:n]], [_rows(t, 4 * A, 'RPNHead.loss bbox_preds') for t in maps[n:]])[:2]
        fctx.hrf = (grads, A)
        return losses

    @staticmethod
    def backward(fctx, gl):
        grads, A = fctx.hrf
        gl = gl.float()
        dc = [(g[..., :A] * gl[0, l]).permute(0, 3, 1, 2) for l, g in enumerate(grads)]
        dr = [(g[..., A:5 * A] * gl[1, l]).permute(0, 3, 1, 2) for l, g in enumerate(grads)]
        return (None, None) + tuple(dc) + tuple(dr)


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
        if train_cfg is not None:
            self._train_cfg(train_cfg, loss_cls, loss_bbox)    # an unsupported assigner / sampler / loss raises at build time
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

    @staticmethod
    def _train_cfg(train_cfg, loss_cls, loss_bbox):
        """-> the keywords of train_cfg_struct for a train_cfg.rpn dict + the two loss dicts; anything the kernels do not build raises"""
        tc = dict(train_cfg)
        asg, smp = dict(tc.pop('assigner', {})), dict(tc.pop('sampler', {}))
        if asg.pop('type', None) != 'MaxIoUAssigner':
            raise _not_built('train_cfg.assigner.type', train_cfg.get('assigner', {}).get('type'), 'MaxIoUAssigner in every HRFuser config')
        pos, neg = asg.pop('pos_iou_thr', None), asg.pop('neg_iou_thr', None)
        if not isinstance(neg, float) or not isinstance(pos, (int, float)):
            raise _not_built('train_cfg.assigner.pos_iou_thr / neg_iou_thr', (pos, neg), 'two numbers; a (low, high) tuple for neg_iou_thr is not')
        min_pos, mlq = float(asg.pop('min_pos_iou', 0.0)), bool(asg.pop('match_low_quality', True))
        if asg.pop('ignore_iof_thr', -1) > 0:
            raise _not_built('train_cfg.assigner.ignore_iof_thr', train_cfg['assigner']['ignore_iof_thr'], 'gt_bboxes_ignore is out of scope; -1 in every HRFuser config')
        asg.pop('ignore_wrt_candidates', True)                      # (only read with ignore_iof_thr > 0)
        if asg.pop('gt_max_assign_all', True) is not True:
            raise _not_built('train_cfg.assigner.gt_max_assign_all', False, 'True, the default')
        if asg.pop('gpu_assign_thr', -1) != -1:
            raise _not_built('train_cfg.assigner.gpu_assign_thr', train_cfg['assigner']['gpu_assign_thr'], 'the assignment never leaves the device; -1')
        if dict(asg.pop('iou_calculator', dict(type='BboxOverlaps2D'))) != dict(type='BboxOverlaps2D') or asg:
            raise _not_built('train_cfg.assigner keys', sorted(asg) or 'iou_calculator', 'unknown to the kernel')
        if smp.pop('type', None) != 'RandomSampler':
            raise _not_built('train_cfg.sampler.type', train_cfg.get('sampler', {}).get('type'), 'RandomSampler in every HRFuser config')
        num, frac = smp.pop('num', None), smp.pop('pos_fraction', None)
        if not isinstance(num, int) or num < 1 or frac is None or not 0.0 <= float(frac) <= 1.0:
            raise _not_built('train_cfg.sampler.num / pos_fraction', (num, frac), 'num >= 1 and 0 <= pos_fraction <= 1')
        if smp.pop('neg_pos_ub', -1) != -1:
            raise _not_built('train_cfg.sampler.neg_pos_ub', train_cfg['sampler']['neg_pos_ub'], '-1 in every HRFuser config')
        if smp.pop('add_gt_as_proposals', True) is not False:
            raise _not_built('train_cfg.sampler.add_gt_as_proposals', train_cfg['sampler'].get('add_gt_as_proposals', True),
                             'False for an RPN: ground truths are not anchors')
        if smp:
            raise _not_built('train_cfg.sampler keys', sorted(smp), 'unknown to the kernel')
        if tc.get('pos_weight', -1) > 0:
            raise _not_built('train_cfg.pos_weight', tc['pos_weight'], '-1 in every HRFuser config')
        if tc.get('debug', False):
            raise _not_built('train_cfg.debug', True, 'False')
        lc, lb = dict(loss_cls or {}), dict(loss_bbox or {})
        if lc.get('type') != 'CrossEntropyLoss' or not lc.get('use_sigmoid', False) or lc.get('use_mask', False) or lc.get('class_weight') is not None \
                or lc.get('reduction', 'mean') != 'mean':
            raise _not_built('loss_cls', loss_cls, 'a sigmoid CrossEntropyLoss with mean reduction')
        if lb.get('type') != 'SmoothL1Loss' or lb.get('reduction', 'mean') != 'mean' or not float(lb.get('beta', 1.0)) > 0:
            raise _not_built('loss_bbox', loss_bbox, 'a SmoothL1Loss with beta > 0 and mean reduction')
        return dict(pos_iou_thr=float(pos), neg_iou_thr=neg, min_pos_iou=min_pos, match_low_quality=mlq, allowed_border=int(tc.get('allowed_border', 0)),
                    num=num, num_pos=int(num * float(frac)), beta=float(lb.get('beta', 1.0)), loss_weight_cls=float(lc.get('loss_weight', 1.0)),
                    loss_weight_bbox=float(lb.get('loss_weight', 1.0)))

    def _no_train_cfg(self, what):
        return NotImplementedError(f'RPNHead on the HIP engine: {what} is not built without train_cfg - the anchor assigner and sampler (train_cfg.'
                                   'assigner / sampler) are named there; the head is forward / proposals only')

    def rng(self, device):
        """the device (seed, counter) pair the sampler draws from (rpn.rng_state); hrf_rpn_loss advances the counter"""
        st = self.__dict__.get('_rng')
        if st is None or st.device != torch.device(device):
            st = self.__dict__['_rng'] = rng_state(int(torch.initial_seed()), 0, device)
        return st

    def _loss_call(self, cls_scores, gt_bboxes, img_metas, keys=None):
        """-> f(cls_maps, reg_maps) = rpn_loss(...) with everything but the maps bound; gt_bboxes: a list of (n_i, 4) tensors or the
        fixed-shape pair (gt (B,Gmax,4), gt_count (B,) int32) on the device"""
        dev, n = cls_scores[0].device, len(cls_scores)
        if isinstance(gt_bboxes, tuple) and len(gt_bboxes) == 2 and isinstance(gt_bboxes[0], torch.Tensor) and gt_bboxes[0].dim() == 3:
            gt, gt_count = gt_bboxes
        else:
            gt, gt_count = pack_gts(gt_bboxes, dev)
        cfg = train_cfg_struct(**self._train_cfg(self.train_cfg, self.loss_cls, self.loss_bbox))
        shp = [m['img_shape'] for m in img_metas] if not isinstance(img_metas, tuple) else img_metas[0]
        pad = [m.get('pad_shape', m['img_shape']) for m in img_metas] if not isinstance(img_metas, tuple) else img_metas[1]
        bases, strides = [b.tolist() for b in self.base_anchors[:n]], self.strides[:n]
        rng = None if keys is not None else self.rng(dev)
        return lambda cm, rm: rpn_loss(cm, rm, shp, pad, gt, gt_count, strides, bases, cfg, keys=keys, rng=rng)

    def get_targets(self, cls_scores, bbox_preds, gt_bboxes, img_metas, keys=None):
        """The fixed-shape form of anchor_head.py:299-400: -> (assigned (B,N) int32: -2 not inside / -1 / 0 / i + 1, max_iou (B,N),
        sampled (B,N) int32: +1 / -1 / 0, counts (B,4) int32) over the anchors of all levels, level after level.  Draws with the
        head's current counter and does not advance it."""
        if self.train_cfg is None:
            raise self._no_train_cfg('get_targets')
        A, dev = self.num_base_priors, cls_scores[0].device
        cm = [_rows(t, A, 'RPNHead.get_targets cls_scores') for t in cls_scores]
        rm = [_rows(t, 4 * A, 'RPNHead.get_targets bbox_preds') for t in bbox_preds]
        gt, gt_count = gt_bboxes if isinstance(gt_bboxes, tuple) else pack_gts(gt_bboxes, dev)
        n = len(cm)
        return rpn_assign(cm, rm, [m['img_shape'] for m in img_metas], [m.get('pad_shape', m['img_shape']) for m in img_metas], gt, gt_count,
                          self.strides[:n], [b.tolist() for b in self.base_anchors[:n]],
                          train_cfg_struct(**self._train_cfg(self.train_cfg, self.loss_cls, self.loss_bbox)), keys=keys,
                          rng=None if keys is not None else self.rng(dev))

    def loss(self, *args, **kwargs):
        """rpn_head.py:70-101 -> dict(loss_rpn_cls=[per level], loss_rpn_bbox=[per level]).  Signature (cls_scores, bbox_preds,
        gt_bboxes, img_metas, gt_bboxes_ignore=None); gt_bboxes: a list of (n_i, 4) tensors (packed without a synchronisation) or the
        fixed-shape pair (gt (B,Gmax,4) fp32, gt_count (B,) int32) for a captured graph; img_metas: dicts with img_shape / pad_shape,
        or the pair of (B,2) device tensors (img_shape, pad_shape).  The values carry a grad_fn: backward delivers the kernel's
        gradient maps, scaled by the incoming gradients, to cls_scores / bbox_preds."""
        if self.train_cfg is None:
            raise self._no_train_cfg('loss')
        return self._loss(*args, **kwargs)

    def _loss(self, cls_scores, bbox_preds, gt_bboxes, img_metas, gt_bboxes_ignore=None, keys=None):
        if gt_bboxes_ignore is not None:
            raise _not_built('gt_bboxes_ignore', 'given', 'ignore regions are out of scope')
        if len(cls_scores) != len(bbox_preds) or len(cls_scores) > len(self.strides):
            raise ValueError(f'RPNHead.loss: {len(cls_scores)} / {len(bbox_preds)} maps, {len(self.strides)} anchor strides')
        call = self._loss_call(cls_scores, gt_bboxes, img_metas, keys)
        losses = _RpnLossFn.apply(call, self.num_base_priors, *cls_scores, *bbox_preds)
        n = len(cls_scores)
        return dict(loss_rpn_cls=[losses[0, l] for l in range(n)], loss_rpn_bbox=[losses[1, l] for l in range(n)])

    def forward_train(self, *args, **kwargs):
        """base_dense_head.py:303-346 -> losses, or (losses, proposal_list) with a proposal_cfg.  Signature (x, img_metas, gt_bboxes,
        gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None); the proposal list slices by count and SYNCHRONISES."""
        if self.train_cfg is None:
            raise self._no_train_cfg('forward_train')
        return self._forward_train(*args, **kwargs)

    def _forward_train(self, x, img_metas, gt_bboxes, gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None, **kwargs):
        outs = self(x)
        losses = self.loss(*outs, gt_bboxes, img_metas, gt_bboxes_ignore=gt_bboxes_ignore)
        if proposal_cfg is None:
            return losses
        return losses, self.get_bboxes(*outs, img_metas=img_metas, cfg=proposal_cfg)


def build_head(cfg):
    """mmdet.models.builder.build_head (builder.py:33-35)."""
    return HEADS.build(cfg)
