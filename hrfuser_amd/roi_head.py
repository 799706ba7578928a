"""CascadeRoIHead + Shared2FCBBoxHead on the HIP engine at test time - from the pyramid and the RPN's rois to detections, in every
reference config (configs/_base_/models/cascade_rcnn_hrfuser_fpn_*_fusion.py:148-208 with test_cfg.rcnn :289-292).

Drop-ins for mmdet's `Shared2FCBBoxHead` (mmdet/models/roi_heads/bbox_heads/convfc_bbox_head.py, bbox_head.py) and
`CascadeRoIHead` (cascade_roi_head.py:288-400): same registry names, constructor keywords and state-dict keys
(`bbox_head.{i}.shared_fcs.{0,1}.*`, `fc_cls.*`, `fc_reg.*`).  Eval / forward only, fp32, no tape: `loss` / `forward_train` raise.

  Shared2FCBBoxHead.forward   fc1 and fc2 through hrf_fc (bias and ReLU in the launch, csrc/hrf_fc.h); fc_cls and fc_reg as ONE
               padded GEMM (the same entry, no activation) into a buffer of ceil16(num_classes + 5) columns - cls and reg are
               column slices of it, which the post-processing kernels read in place.  HRF_FC_ROUTE=rowgemm runs the layers as
               hrf_rowgemm (+ hrf_affine_act_res for fc1 / fc2): the launches the library had before hrf_fc, the A/B baseline of
               tools/roi_head_cost.py and the route `fc_route` keeps from 256 workgroups on, where hrf_fc measured no faster;
               HRF_FC_ROUTE=fc forces hrf_fc.
  CascadeRoIHead.detect       per stage hrf_roi_align_fwd ([K][7][7][C], fc1's columns permuted to match at pack time) -> head ->
               hrf_bbox_refine, then hrf_bbox_detect (csrc/hrf_bbox.h).  Fixed-shape outputs (dets, labels, count), no host
               read, no synchronisation: capturable in a hipGraph.
  CascadeRoIHead.simple_test  mmdet's return type - bbox2result lists - which slices by `count` and therefore SYNCHRONISES.

Functional entries underneath: `fc`, `bbox_refine`, `bbox_detect`.  There is no CPU fallback.
"""
import os

import torch
import torch.nn as nn

from . import _lib
from .registry import HEADS, ROI_EXTRACTORS
from .roi import POOLED, _nhwc, roi_forward
from .rpn import MAX_PRE, _shapes

MAX_CLASSES = _lib._header_int('HRF_BBOX_MAX_CLASSES', 16)
MAX_STAGES = _lib._header_int('HRF_BBOX_MAX_STAGES', 4)

FC_ROUTES = ('fc', 'rowgemm')
FC_FILL_BLOCKS = 256            # workgroups of an hrf_rowgemm launch (128 rows x 128 columns each) from which it fills the chip


def fc_route(M, N):
    """The route of an activated FC layer of M rows and N columns: HRF_FC_ROUTE when set, otherwise hrf_fc while the hrf_rowgemm
    launch of the shape would have fewer than FC_FILL_BLOCKS workgroups.  Measured at K = 12544, N = 1024 (DESIGN.md section 19,
    profiles/roi_head_cost.txt): at M = 200, 1000, 2000 (16 / 64 / 128 workgroups) the range of hrf_fc's times lies below that of
    hrf_rowgemm + hrf_affine_act_res; at M = 4000 (256 workgroups) the ranges overlap and the old route stays."""
    r = os.environ.get('HRF_FC_ROUTE')
    if r is None:
        return 'fc' if ((M + 127) // 128) * ((N + 127) // 128) < FC_FILL_BLOCKS else 'rowgemm'
    if r not in FC_ROUTES:
        raise ValueError(f'HRF_FC_ROUTE={r!r}: one of {FC_ROUTES}')
    return r


def _ceil16(n):
    return (n + 15) // 16 * 16


def _stream(stream):
    return _lib.stream_ptr() if stream is None else stream


def fc(x, wp, bias, N, relu=False, out=None, route=None, stream=None, consts=None):
    """y (M, N) = act(bias + x @ wp.T): x (M, K) fp32 rows of one pitch (a column slice is read in place), wp the packed (N, K)
    weight (hrf_fc_pack), bias (N,) or None.  route None: fc_route(M, N).  consts: (ones (N,), zeros (N,)) of the rowgemm route."""
    L = _lib.lib()
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise ValueError(f'fc: x must be fp32 (M, K) rows, got {tuple(x.shape)} {x.dtype} strides {tuple(x.stride())}')
    M, K = x.shape
    ldX = x.stride(0) if M > 1 else max(x.stride(0), K)
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    ldY = out.stride(0) if M > 1 else max(out.stride(0), N)
    s = _stream(stream)
    if (fc_route(M, N) if route is None else route) == 'rowgemm':
        if not relu:
            L.hrf_rowgemm(x, ldX, wp, bias, out, ldY, 0, M, K, N, s)
            return out
        if ldY != N:
            raise ValueError('fc (rowgemm route): the ReLU launch takes dense rows')
        y = torch.empty((M, N), device=x.device, dtype=torch.float32)
        L.hrf_rowgemm(x, ldX, wp, bias, y, N, 0, M, K, N, s)
        one, zero = consts if consts is not None else (torch.ones(N, device=x.device), torch.zeros(N, device=x.device))
        if M > 0:
            L.hrf_affine_act_res(y, one, zero, None, None, None, None, None, max(M, 1), 1, 0, out, M, N, None, 0.0, None, None, s)
        return out
    need = L.hrf_fc_workspace_bytes(M, K, N)
    ws = torch.empty((need,), device=x.device, dtype=torch.uint8) if need > 0 else None
    L.hrf_fc(x, ldX, wp, bias, out, ldY, int(bool(relu)), M, K, N, ws, need, s)
    return out


def bbox_refine(rois, deltas, stds, img_shapes, B, out=None, stream=None):
    """hrf_bbox_refine: rois (K,5), deltas (K,4) rows of one pitch (a column slice of the head output), stds (4), img_shapes the
    device (B,2) fp32 tensor of (h, w) -> rois_out (K,5)"""
    L = _lib.lib()
    if rois.dim() != 2 or rois.shape[1] != 5 or rois.dtype != torch.float32 or not rois.is_contiguous():
        raise ValueError(f'bbox_refine: rois must be contiguous fp32 (K, 5), got {tuple(rois.shape)} {rois.dtype}')
    K = rois.shape[0]
    if deltas.shape != (K, 4) or deltas.dtype != torch.float32 or deltas.stride(1) != 1:
        raise ValueError(f'bbox_refine: deltas must be fp32 ({K}, 4) rows, got {tuple(deltas.shape)} {deltas.dtype}')
    if out is None:
        out = torch.empty_like(rois)
    ldd = deltas.stride(0) if K > 1 else max(deltas.stride(0), 4)
    L.hrf_bbox_refine(rois, deltas, ldd, float(stds[0]), float(stds[1]), float(stds[2]), float(stds[3]), _shapes(img_shapes, B, rois.device), B, K,
                      out, _stream(stream))
    return out


def _scales_t(scale_factors, B, dev):
    if scale_factors is None:
        return None
    if isinstance(scale_factors, torch.Tensor):
        t = scale_factors
        if t.shape != (B, 4) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f'bbox_detect: scale_factors tensor must be contiguous fp32 ({B}, 4) on {dev}')
        return t
    if len(scale_factors) != B:
        raise ValueError(f'bbox_detect: {len(scale_factors)} scale factors for a batch of {B}')
    return torch.tensor([[float(v) for v in s] for s in scale_factors], dtype=torch.float32).reshape(B, 4).to(dev)


def bbox_detect(rois, count, logits, deltas, stds, img_shapes, B, num_classes, score_thr, iou_thr, max_per_img, scale_factors=None,
                workspace=None, stream=None):
    """hrf_bbox_detect: rois (B*R,5), count (B,) int32 or None, logits = [(B*R, num_classes+1)] per stage and deltas (B*R,4) as
    rows of one pitch each (all stages the same) -> dets (B,max_per_img,5), labels (B,max_per_img) int32, count (B,) int32"""
    L = _lib.lib()
    K, dev = rois.shape[0], rois.device
    if rois.dim() != 2 or rois.shape[1] != 5 or rois.dtype != torch.float32 or not rois.is_contiguous() or K % B != 0:
        raise ValueError(f'bbox_detect: rois must be contiguous fp32 (B * R, 5), got {tuple(rois.shape)} {rois.dtype} for B = {B}')
    R = K // B
    if not 1 <= R <= MAX_PRE or not 1 <= num_classes <= MAX_CLASSES or not 1 <= len(logits) <= MAX_STAGES:
        raise NotImplementedError(f'bbox_detect on the HIP engine: {R} rois per image (1..{MAX_PRE}), {num_classes} classes (1..{MAX_CLASSES}) or '
                                  f'{len(logits)} stages (1..{MAX_STAGES}) are not built')
    if count is not None and (count.shape != (B,) or count.dtype != torch.int32 or not count.is_contiguous()):
        raise ValueError(f'bbox_detect: count must be contiguous int32 ({B},), got {tuple(count.shape)} {count.dtype}')
    d = _lib.BboxDet()
    d.B, d.R, d.num_classes, d.num_stages = B, R, num_classes, len(logits)
    d.rois, d.count = rois.data_ptr(), (None if count is None else count.data_ptr())
    ldl = None
    for s, t in enumerate(logits):
        if t.shape != (K, num_classes + 1) or t.dtype != torch.float32 or t.stride(1) != 1:
            raise ValueError(f'bbox_detect: logits[{s}] must be fp32 ({K}, {num_classes + 1}) rows, got {tuple(t.shape)} {t.dtype}')
        ld = t.stride(0) if K > 1 else max(t.stride(0), num_classes + 1)
        if ldl is not None and ld != ldl:
            raise ValueError('bbox_detect: the stages\' logits must share one row pitch')
        ldl = ld
        if L.require_cuda and not t.is_cuda:
            raise _lib.HRFuserHipError(f'bbox_detect: tensor on {t.device}; the HIP path has no CPU fallback')
        d.logits[s] = t.data_ptr()
    if deltas.shape != (K, 4) or deltas.dtype != torch.float32 or deltas.stride(1) != 1:
        raise ValueError(f'bbox_detect: deltas must be fp32 ({K}, 4) rows, got {tuple(deltas.shape)} {deltas.dtype}')
    d.ld_logits, d.deltas, d.ld_deltas = ldl, deltas.data_ptr(), (deltas.stride(0) if K > 1 else max(deltas.stride(0), 4))
    for k in range(4):
        d.stds[k] = float(stds[k])
    shp, sf = _shapes(img_shapes, B, dev), _scales_t(scale_factors, B, dev)
    d.img_shape, d.scale_factor = shp.data_ptr(), (None if sf is None else sf.data_ptr())
    d.score_thr, d.iou_thr, d.max_per_img = float(score_thr), float(iou_thr), int(max_per_img)
    for t in (rois, deltas, shp):
        if L.require_cuda and not t.is_cuda:
            raise _lib.HRFuserHipError(f'bbox_detect: tensor on {t.device}; the HIP path has no CPU fallback')
    need = L.hrf_bbox_detect_workspace_bytes(B, R, num_classes)
    if workspace is None:
        workspace = torch.empty((max(need, 256),), device=dev, dtype=torch.uint8)
    mp = max(int(max_per_img), 1)
    dets = torch.empty((B, mp, 5), device=dev, dtype=torch.float32)
    labels = torch.empty((B, mp), device=dev, dtype=torch.int32)
    cnt = torch.empty((B,), device=dev, dtype=torch.int32)
    L.hrf_bbox_detect(d, workspace, workspace.numel(), dets, labels, cnt, _stream(stream))
    return dets, labels, cnt


def _not_built(who, key, value, why):
    return NotImplementedError(f'{who} on the HIP engine: {key}={value!r} is not built ({why})')


@HEADS.register_module()
class Shared2FCBBoxHead(nn.Module):
    """convfc_bbox_head.py:206-220 (ConvFCBBoxHead with two shared FCs) / bbox_head.py:15-100 at test time."""

    def __init__(self, fc_out_channels=1024, with_avg_pool=False, with_cls=True, with_reg=True, roi_feat_size=7, in_channels=256, num_classes=80,
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', clip_border=True, target_means=[0., 0., 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2]),
                 reg_class_agnostic=False, reg_decoded_bbox=False, reg_predictor_cfg=dict(type='Linear'), cls_predictor_cfg=dict(type='Linear'),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0), init_cfg=None, num_shared_convs=0, num_shared_fcs=2,
                 num_cls_convs=0, num_cls_fcs=0, num_reg_convs=0, num_reg_fcs=0, conv_out_channels=256, conv_cfg=None, norm_cfg=None):
        super().__init__()
        who = 'Shared2FCBBoxHead'
        if not reg_class_agnostic:
            raise _not_built(who, 'reg_class_agnostic', reg_class_agnostic, 'True in every HRFuser config; class-specific regression is out of scope')
        for k, v in (('num_shared_convs', num_shared_convs), ('num_cls_convs', num_cls_convs), ('num_reg_convs', num_reg_convs),
                     ('num_cls_fcs', num_cls_fcs), ('num_reg_fcs', num_reg_fcs)):
            if v != 0:
                raise _not_built(who, k, v, 'convolution / separate branches are not; Shared2FCBBoxHead has none')
        if num_shared_fcs != 2:
            raise _not_built(who, 'num_shared_fcs', num_shared_fcs, 'two shared FCs')
        if with_avg_pool:
            raise _not_built(who, 'with_avg_pool', with_avg_pool, 'False in every HRFuser config')
        if not (with_cls and with_reg):
            raise _not_built(who, 'with_cls / with_reg', (with_cls, with_reg), 'both outputs come from one GEMM')
        if roi_feat_size not in (POOLED, (POOLED, POOLED), [POOLED, POOLED]):
            raise _not_built(who, 'roi_feat_size', roi_feat_size, '7, the RoIAlign output size')
        bc = dict(bbox_coder)
        if bc.pop('type', None) != 'DeltaXYWHBBoxCoder':
            raise _not_built(who, 'bbox_coder.type', bbox_coder.get('type'), 'DeltaXYWHBBoxCoder in every HRFuser config')
        means, stds = bc.pop('target_means', (0., 0., 0., 0.)), bc.pop('target_stds', (1., 1., 1., 1.))
        if any(float(m) != 0.0 for m in means):
            raise _not_built(who, 'bbox_coder.target_means', means, 'the kernels decode with means 0')
        if len(stds) != 4 or any(not float(s) > 0.0 for s in stds):
            raise _not_built(who, 'bbox_coder.target_stds', stds, 'four positive values')
        for k, dflt in (('clip_border', True), ('add_ctr_clamp', False), ('ctr_clamp', 32)):
            if bc.pop(k, dflt) != dflt:
                raise _not_built(who, 'bbox_coder.' + k, bbox_coder[k], f'{dflt!r}, the default')
        if bc:
            raise _not_built(who, 'bbox_coder keys', sorted(bc), 'unknown to the kernels')
        lc = dict(loss_cls or {})
        if lc.get('use_sigmoid', False):
            raise _not_built(who, 'loss_cls.use_sigmoid', True, 'softmax over num_classes + 1 logits in every HRFuser config')
        if lc.get('type', 'CrossEntropyLoss') != 'CrossEntropyLoss' or lc.get('use_mask', False):
            raise _not_built(who, 'loss_cls', loss_cls, 'custom activations / class channels (Seesaw loss ...) are not')
        for k, v in (('reg_predictor_cfg', reg_predictor_cfg), ('cls_predictor_cfg', cls_predictor_cfg)):
            if dict(v) != dict(type='Linear'):
                raise _not_built(who, k, v, "dict(type='Linear')")
        if reg_decoded_bbox:
            raise _not_built(who, 'reg_decoded_bbox', reg_decoded_bbox, 'a training-only switch')
        if conv_cfg is not None or norm_cfg is not None:
            raise _not_built(who, 'conv_cfg / norm_cfg', (conv_cfg, norm_cfg), 'there are no convolutions')
        if not 1 <= num_classes <= MAX_CLASSES:
            raise _not_built(who, 'num_classes', num_classes, f'1..{MAX_CLASSES}; 10 and 3 in the HRFuser configs')
        if in_channels % 16 != 0 or fc_out_channels % 16 != 0 or in_channels < 16 or fc_out_channels < 16:
            raise _not_built(who, 'in_channels / fc_out_channels', (in_channels, fc_out_channels), 'multiples of 16; 256 / 1024 in every HRFuser config')
        self.in_channels, self.fc_out_channels, self.num_classes = in_channels, fc_out_channels, num_classes
        self.roi_feat_size, self.roi_feat_area = (POOLED, POOLED), POOLED * POOLED
        self.with_avg_pool, self.with_cls, self.with_reg = False, True, True
        self.reg_class_agnostic, self.reg_decoded_bbox = True, False
        self.num_shared_convs, self.num_shared_fcs = 0, 2
        self.bbox_coder, self.loss_cls, self.loss_bbox, self.init_cfg = dict(bbox_coder), loss_cls, loss_bbox, init_cfg
        self.target_stds = tuple(float(s) for s in stds)
        self.custom_cls_channels = self.custom_activation = self.custom_accuracy = False
        self.fp16_enabled = False
        self.shared_fcs = nn.ModuleList([nn.Linear(in_channels * self.roi_feat_area, fc_out_channels), nn.Linear(fc_out_channels, fc_out_channels)])
        self.fc_cls = nn.Linear(fc_out_channels, num_classes + 1)
        self.fc_reg = nn.Linear(fc_out_channels, 4)
        self.relu = nn.ReLU(inplace=True)
        self.init_weights()
        self.__dict__['_packs'] = {}

    @property
    def out_pitch(self):
        """columns of the padded fc_cls / fc_reg output: (num_classes + 1) logits, 4 deltas, zeros"""
        return _ceil16(self.num_classes + 5)

    def init_weights(self):
        """bbox_head.py:89-96 + convfc_bbox_head.py:100-115: Xavier uniform shared_fcs, Normal 0.01 fc_cls, Normal 0.001 fc_reg, bias 0"""
        for m in self.shared_fcs:
            nn.init.xavier_uniform_(m.weight, gain=1)
            nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.fc_cls.weight, 0, 0.01)
        nn.init.normal_(self.fc_reg.weight, 0, 0.001)
        nn.init.constant_(self.fc_cls.bias, 0)
        nn.init.constant_(self.fc_reg.bias, 0)

    def _packed(self, dev):
        """packed weights, refreshed when a parameter changed (its version counter or storage).  w1: fc1 for (K,C,7,7) features;
        w1n: the same with its columns permuted for [K][7][7][C] features (made on first use)"""
        ps = tuple(p for m in (self.shared_fcs[0], self.shared_fcs[1], self.fc_cls, self.fc_reg) for p in (m.weight, m.bias))
        tag = tuple((p.data_ptr(), p._version) for p in ps) + (str(dev),)
        pk = self.__dict__['_packs']
        if pk.get('tag') != tag:
            pk.clear()
            L, s = _lib.lib(), _lib.stream_ptr()
            F, Kin, P, nc = self.fc_out_channels, self.in_channels * self.roi_feat_area, self.out_pitch, self.num_classes
            w2 = torch.empty((F * F,), device=dev, dtype=torch.float32)
            L.hrf_fc_pack(self.shared_fcs[1].weight.detach().contiguous(), F, F, F, F, w2, s)
            both = torch.cat([self.fc_cls.weight.detach(), self.fc_reg.weight.detach()]).contiguous()
            w3 = torch.empty((P * F,), device=dev, dtype=torch.float32)
            L.hrf_fc_pack(both, nc + 5, F, P, F, w3, s)
            b3 = torch.zeros(P, device=dev, dtype=torch.float32)
            b3[:nc + 5] = torch.cat([self.fc_cls.bias.detach(), self.fc_reg.bias.detach()])
            pk.update(tag=tag, w2=w2, w3=w3, b3=b3, b1=self.shared_fcs[0].bias.detach().contiguous(), b2=self.shared_fcs[1].bias.detach().contiguous(),
                      consts=(torch.ones(F, device=dev), torch.zeros(F, device=dev)), Kin=Kin)
        return pk

    def _w1(self, pk, dev, nhwc):
        key = 'w1n' if nhwc else 'w1'
        if key not in pk:
            L, s = _lib.lib(), _lib.stream_ptr()
            F, C, A = self.fc_out_channels, self.in_channels, self.roi_feat_area
            w = self.shared_fcs[0].weight.detach()
            if nhwc:                                               # column (c, y, x) -> (y, x, c)
                w = w.reshape(F, C, A).permute(0, 2, 1)
            w = w.reshape(F, C * A).contiguous()
            wp = torch.empty((F * C * A,), device=dev, dtype=torch.float32)
            L.hrf_fc_pack(w, F, C * A, F, C * A, wp, s)
            pk[key] = wp
        return pk[key]

    def run(self, x2d, nhwc=False, route=None, stream=None):
        """x2d (K, 49 * C) fp32 dense rows, flattened (C,7,7) (nhwc False) or (7,7,C) -> the padded output (K, out_pitch):
        columns [0, num_classes] the logits, the next four the deltas"""
        L = _lib.lib()
        if L.require_cuda and not x2d.is_cuda:
            raise _lib.HRFuserHipError(f'Shared2FCBBoxHead: tensor on {x2d.device}; the HIP path has no CPU fallback')
        dev = x2d.device
        pk = self._packed(dev)
        if x2d.dim() != 2 or x2d.shape[1] != pk['Kin'] or x2d.dtype != torch.float32 or not x2d.is_contiguous():
            raise ValueError(f'Shared2FCBBoxHead: features must be contiguous fp32 (K, {pk["Kin"]}), got {tuple(x2d.shape)} {x2d.dtype}')
        F = self.fc_out_channels
        h = fc(x2d, self._w1(pk, dev, nhwc), pk['b1'], F, True, route=route, stream=stream, consts=pk['consts'])
        h = fc(h, pk['w2'], pk['b2'], F, True, route=route, stream=stream, consts=pk['consts'])
        return fc(h, pk['w3'], pk['b3'], self.out_pitch, False, route=route, stream=stream)

    def forward(self, x, layout=None):
        """convfc_bbox_head.py:155-191: x (K, C, 7, 7), or the extractor's (K, 7, 7, C) with layout='nhwc' (layout None: by the
        shape; (K, 7, 7, 7) is taken as NCHW) -> (cls_score (K, num_classes + 1), bbox_pred (K, 4)): column slices of ONE buffer"""
        C, nc = self.in_channels, self.num_classes
        if layout is None:
            layout = 'nchw' if tuple(x.shape[1:]) == (C, POOLED, POOLED) else 'nhwc'
        want = (C, POOLED, POOLED) if layout == 'nchw' else (POOLED, POOLED, C)
        if x.dim() != 4 or tuple(x.shape[1:]) != want:
            raise ValueError(f'Shared2FCBBoxHead.forward: expected (K, {want[0]}, {want[1]}, {want[2]}) ({layout}), got {tuple(x.shape)}')
        with torch.no_grad():
            out = self.run(x.detach().contiguous().reshape(x.shape[0], -1), nhwc=layout == 'nhwc')
        return out[:, :nc + 1], out[:, nc + 1:nc + 5]

    def loss(self, *args, **kwargs):
        raise NotImplementedError('Shared2FCBBoxHead on the HIP engine: loss is not built - assigners, samplers and losses are out of scope; '
                                  'the head is forward only')

    def get_targets(self, *args, **kwargs):
        raise NotImplementedError('Shared2FCBBoxHead on the HIP engine: get_targets is not built - training is out of scope')


def _rcnn_cfg(cfg):
    """-> (score_thr, iou_threshold, max_per_img) of a test_cfg.rcnn dict"""
    nms = dict(cfg.get('nms', {}))
    if nms.get('type', 'nms') != 'nms':
        raise _not_built('CascadeRoIHead', 'nms.type', nms.get('type'), "'nms' in every HRFuser config; soft_nms is not")
    if nms.get('split_thr') is not None or nms.get('class_agnostic', False):
        raise _not_built('CascadeRoIHead', 'nms', nms, 'classes are always separate NMS problems')
    mp = int(cfg.get('max_per_img', -1))
    if mp < 1:
        raise _not_built('CascadeRoIHead', 'max_per_img', mp, 'a fixed output shape needs a bound; 100 in every HRFuser config')
    return float(cfg.get('score_thr', 0.05)), float(nms.get('iou_threshold', 0.5)), mp


@HEADS.register_module()
class CascadeRoIHead(nn.Module):
    """cascade_roi_head.py:18-400 at test time, bbox branch only.  `x`: the pyramid (logical NCHW, finest first)."""

    def __init__(self, num_stages, stage_loss_weights, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None,
                 shared_head=None, train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None):
        super().__init__()
        who = 'CascadeRoIHead'
        if bbox_roi_extractor is None or bbox_head is None:
            raise ValueError('CascadeRoIHead: bbox_roi_extractor and bbox_head are required')
        if mask_roi_extractor is not None or mask_head is not None:
            raise _not_built(who, 'mask_head', mask_head, 'mask heads are out of scope; no HRFuser config has one')
        if shared_head is not None:
            raise _not_built(who, 'shared_head', shared_head, 'not supported by Cascade R-CNN')
        if not 1 <= num_stages <= MAX_STAGES:
            raise _not_built(who, 'num_stages', num_stages, f'1..{MAX_STAGES}; 3 in every HRFuser config')
        if len(stage_loss_weights) != num_stages:
            raise ValueError(f'CascadeRoIHead: {len(stage_loss_weights)} stage_loss_weights for {num_stages} stages')
        ext = bbox_roi_extractor if isinstance(bbox_roi_extractor, (list, tuple)) else [bbox_roi_extractor] * num_stages
        hd = bbox_head if isinstance(bbox_head, (list, tuple)) else [bbox_head] * num_stages
        if len(ext) != num_stages or len(hd) != num_stages:
            raise ValueError(f'CascadeRoIHead: {len(ext)} extractors / {len(hd)} heads for {num_stages} stages')
        self.num_stages, self.stage_loss_weights = num_stages, list(stage_loss_weights)
        self.train_cfg, self.test_cfg, self.init_cfg = train_cfg, test_cfg, init_cfg
        self.bbox_roi_extractor = nn.ModuleList([ROI_EXTRACTORS.build(dict(e)) if isinstance(e, dict) else e for e in ext])
        self.bbox_head = nn.ModuleList([HEADS.build(dict(h)) if isinstance(h, dict) else h for h in hd])
        for h in self.bbox_head:
            if not isinstance(h, Shared2FCBBoxHead):
                raise _not_built(who, 'bbox_head.type', type(h).__name__, 'Shared2FCBBoxHead in every HRFuser config')
            if h.num_classes != self.bbox_head[0].num_classes:
                raise _not_built(who, 'bbox_head num_classes', [b.num_classes for b in self.bbox_head], 'one class count for all stages')
        if test_cfg is not None:
            _rcnn_cfg(test_cfg)                                    # an unsupported nms raises at build time
        self.fp16_enabled = False

    with_bbox, with_mask, with_shared_head = True, False, False

    def init_weights(self):
        for h in self.bbox_head:
            h.init_weights()

    def detect(self, x, rois, count, img_shapes, scale_factors=None, cfg=None, stages=None):
        """x: the pyramid; rois (B*R,5) = (b, x1, y1, x2, y2), image b at rows b*R.. (RPNHead.proposals' `rois`); count (B,) int32
        valid rows per image or None; img_shapes / scale_factors: device fp32 tensors (B,2) of (h, w) / (B,4) - read by the
        kernels, a captured graph follows their contents - or lists -> (dets (B,max_per_img,5), labels (B,max_per_img) int32,
        count (B,) int32).  Fixed shapes, no synchronisation, capturable.  stages: a list that receives (rois, padded head output)
        of every stage (tests compare them one by one)."""
        cfg = self.test_cfg if cfg is None else cfg
        if cfg is None:
            raise ValueError('CascadeRoIHead.detect: no cfg and the head was built without test_cfg')
        score_thr, iou_thr, max_per_img = _rcnn_cfg(cfg)
        x = tuple(x)
        B, dev = x[0].shape[0], x[0].device
        rois = rois.detach().float().contiguous()
        if rois.dim() != 2 or rois.shape[1] != 5 or rois.shape[0] % B != 0 or rois.shape[0] == 0:
            raise ValueError(f'CascadeRoIHead.detect: rois must be (B * R, 5) with R >= 1, got {tuple(rois.shape)} for B = {B}')
        shp = _shapes(img_shapes, B, dev)
        nc = self.bbox_head[0].num_classes
        maps = {}
        logits, out = [], None
        with torch.no_grad():
            for i in range(self.num_stages):
                ex, hd = self.bbox_roi_extractor[i], self.bbox_head[i]
                n = ex.num_inputs
                if n not in maps:
                    if len(x) < n:
                        raise ValueError(f'CascadeRoIHead: {n} strides, {len(x)} maps')
                    maps[n] = [_nhwc(t) for t in x[:n]]
                feat = roi_forward(maps[n], rois, ex._scales(), float(ex.finest_scale), 1)           # (K,7,7,C)
                out = hd.run(feat.reshape(feat.shape[0], -1), nhwc=True)
                logits.append(out[:, :nc + 1])
                if stages is not None:
                    stages.append((rois, out))
                if i < self.num_stages - 1:
                    rois = bbox_refine(rois, out[:, nc + 1:nc + 5], hd.target_stds, shp, B)
            return bbox_detect(rois, count, logits, out[:, nc + 1:nc + 5], self.bbox_head[-1].target_stds, shp, B, nc, score_thr, iou_thr,
                               max_per_img, scale_factors)

    def simple_test(self, x, proposal_list, img_metas, rescale=False):
        """cascade_roi_head.py:288-400 -> per image a list of num_classes numpy arrays (n, 5) fp32 (bbox2result).  Slices by
        `count`: this one SYNCHRONISES (use `detect` inside a captured graph)."""
        import numpy as np
        nc, B = self.bbox_head[-1].num_classes, len(proposal_list)
        dev = tuple(x)[0].device
        R = max([int(p.shape[0]) for p in proposal_list] + [1])
        rois = torch.zeros((B, R, 5), device=dev, dtype=torch.float32)
        for b, p in enumerate(proposal_list):
            rois[b, :, 0] = float(b)
            rois[b, :p.shape[0], 1:] = p[:, :4].to(dev).float()
        count = torch.tensor([int(p.shape[0]) for p in proposal_list], dtype=torch.int32).to(dev)
        sf = [m['scale_factor'] for m in img_metas] if rescale else None
        dets, labels, cnt = self.detect(x, rois.reshape(B * R, 5), count, [m['img_shape'] for m in img_metas], sf)
        dets, labels = dets.cpu().numpy(), labels.cpu().numpy()
        res = []
        for b, n in enumerate(cnt.tolist()):
            d, l = dets[b, :n], labels[b, :n]
            res.append([d[l == c].astype(np.float32) for c in range(nc)])
        return res

    def aug_test(self, *args, **kwargs):
        raise NotImplementedError('CascadeRoIHead on the HIP engine: aug_test is not built (out of scope)')

    def loss(self, *args, **kwargs):
        raise NotImplementedError('CascadeRoIHead on the HIP engine: loss is not built - assigners, samplers and losses (train_cfg) are out '
                                  'of scope; the head is detect / simple_test only')

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError('CascadeRoIHead on the HIP engine: forward_train is not built - assigners, samplers and losses (train_cfg) '
                                  'are out of scope; the head is detect / simple_test only')
