"""CascadeRoIHead + Shared2FCBBoxHead on the HIP engine at test time - from the pyramid and the RPN's rois to detections, in every
reference config (configs/_base_/models/cascade_rcnn_hrfuser_fpn_*_fusion.py:148-208 with test_cfg.rcnn :289-292).

Drop-ins for mmdet's `Shared2FCBBoxHead` (mmdet/models/roi_heads/bbox_heads/convfc_bbox_head.py, bbox_head.py) and
`CascadeRoIHead` (cascade_roi_head.py:288-400): same registry names, constructor keywords and state-dict keys
(`bbox_head.{i}.shared_fcs.{0,1}.*`, `fc_cls.*`, `fc_reg.*`).  `forward` / `detect` / `losses` are fp32 without a tape; with a `train_cfg` (a list of
one train_cfg.rcnn dict per stage) the RoI head computes mmdet's per-stage losses and their gradient on each stage's head output,
without one `loss` / `get_targets` / `forward_train` raise.

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

  CascadeRoIHead.losses       per stage hrf_bbox_targets (MaxIoUAssigner without low-quality matching, the gts added as proposals,
               RandomSampler, bbox2delta / stds; two launches, csrc/hrf_bbox_train.h) -> hrf_roi_align_fwd -> the head ->
               hrf_bbox_loss (softmax CE, SmoothL1, top-1 accuracy and the gradient rows; two launches) -> hrf_bbox_refine.  The
               sampled rows of an image are its sampled gts, then its other positives, then its negatives, then padding, so the next
               stage's proposals - the refined rows without the gts - are a row range read from the device `counts`.  Fixed shapes, no
               host read: capturable.  `forward_train` wraps it into mmdet's dict; `Shared2FCBBoxHead.loss` gives the values a grad_fn.

  Shared2FCBBoxHead.run_train / run_backward / forward_autograd   the same forward with the activations kept, and its backward
               (csrc/hrf_fc_bwd.h): per layer hrf_fc_bwd_weight (dw += dy^T x, db += sum dy) and hrf_fc_bwd_data (dx = dy w with the
               ReLU mask of the layer below in the epilogue), exact fp32 MFMA, no atomics; .grad lands on the eight parameters.
  CascadeRoIHead.losses_nhwc  `losses` on the explicit tape (runtime.Ctx): the same values, and per stage the closures that carry the
               loss gradient through the head and the RoIAlign adjoint into the pyramid's act.grad.

Functional entries underneath: `fc`, `fc_backward_data`, `fc_backward_weight`, `bbox_refine`, `bbox_detect`, `bbox_targets`, `bbox_loss`.
There is no CPU fallback.
"""
import os

import torch
import torch.nn as nn

from . import _lib
from . import runtime as R
from .registry import HEADS, ROI_EXTRACTORS
from .roi import POOLED, _nhwc, roi_forward
from .rpn import MAX_GT, MAX_PRE, _shapes, pack_gts, rng_state

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


def _rows(t, cols, what):
    if t.dim() != 2 or t.shape[1] < cols or t.dtype != torch.float32 or t.stride(1) != 1:
        raise ValueError(f'{what} must be fp32 (M, >= {cols}) rows, got {tuple(t.shape)} {t.dtype} strides {tuple(t.stride())}')
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def fc_bwd_workspace(M, K, N, dev):
    """the workspace one layer's two backward launches share (hrf_fc_bwd_workspace_bytes), or None"""
    need = _lib.lib().hrf_fc_bwd_workspace_bytes(M, K, N)
    return torch.empty((need,), device=dev, dtype=torch.uint8) if need > 0 else None


def fc_backward_data(dy, wp, K, mask=None, out=None, workspace=None, stream=None):
    """hrf_fc_bwd_data: dy (M, >= N) rows (the N leading columns are read), wp the packed (N, K) weight, mask (M, K) the forward
    output of the ReLU layer below or None -> dx (M, K) = where(mask <= 0, 0, dy @ w): the dy of the layer below"""
    L = _lib.lib()
    M, N = dy.shape[0], wp.numel() // K
    ldDY = _rows(dy, N, 'fc_backward_data: dy')
    if out is None:
        out = torch.empty((M, K), device=dy.device, dtype=torch.float32)
    ldDX = _rows(out, K, 'fc_backward_data: out')
    ldM = 0 if mask is None else _rows(mask, K, 'fc_backward_data: mask')
    if workspace is None:
        workspace = fc_bwd_workspace(M, K, N, dy.device)
    L.hrf_fc_bwd_data(dy, ldDY, wp, K, mask, ldM, out, ldDX, M, K, N, workspace, 0 if workspace is None else workspace.numel(), _stream(stream))
    return out


def fc_backward_weight(x, dy, N, dw, db=None, accumulate=False, workspace=None, stream=None):
    """hrf_fc_bwd_weight: x (M, K) rows, dy (M, >= N) rows -> dw (N, K) (+)= dy[:, :N].T @ x, db (N,) (+)= dy[:, :N].sum(0)"""
    L = _lib.lib()
    M, K = x.shape
    ldX, ldDY, ldDW = _rows(x, K, 'fc_backward_weight: x'), _rows(dy, N, 'fc_backward_weight: dy'), _rows(dw, K, 'fc_backward_weight: dw')
    if dw.shape[0] != N or (db is not None and (db.shape != (N,) or db.dtype != torch.float32 or not db.is_contiguous())):
        raise ValueError(f'fc_backward_weight: dw ({N}, {K}) and db ({N},) fp32 are needed, got {tuple(dw.shape)}')
    if workspace is None:
        workspace = fc_bwd_workspace(M, K, N, x.device)
    L.hrf_fc_bwd_weight(x, ldX, dy, ldDY, dw, ldDW, db, int(bool(accumulate)), M, K, N, workspace, 0 if workspace is None else workspace.numel(),
                        _stream(stream))
    return dw, db


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


# ----------------------------------------------------------------------------- training targets and loss (csrc/hrf_bbox_train.h)
def rcnn_train_cfg_struct(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, add_gt_as_proposals=True, num=512, num_pos=128, num_classes=80,
                          stds=(0.1, 0.1, 0.2, 0.2), beta=1.0, loss_weight_cls=1.0, loss_weight_bbox=1.0):
    """hrf_bbox_train_cfg_t of one stage; num_pos = int(num * pos_fraction); the loss weights include the stage's loss weight"""
    c = _lib.BboxTrainCfg()
    c.pos_iou_thr, c.neg_iou_thr, c.min_pos_iou = float(pos_iou_thr), float(neg_iou_thr), float(min_pos_iou)
    c.add_gt_as_proposals, c.num, c.num_pos, c.num_classes = int(bool(add_gt_as_proposals)), int(num), int(num_pos), int(num_classes)
    for k in range(4):
        c.stds[k] = float(stds[k])
    c.beta, c.loss_weight_cls, c.loss_weight_bbox = float(beta), float(loss_weight_cls), float(loss_weight_bbox)
    return c


def pack_gt_labels(gt_labels, dev, gmax):
    """list of (n_i,) labels -> (B, gmax) int32 on `dev`, the companion of rpn.pack_gts (zeros past n_i; nothing synchronises)"""
    out = torch.zeros((len(gt_labels), int(gmax)), device=dev, dtype=torch.int32)
    for b, t in enumerate(gt_labels):
        if t.shape[0]:
            out[b, :t.shape[0]] = t.detach().reshape(-1).to(device=dev, dtype=torch.int32)
    return out


def _i32(t, shape, dev, what):
    if t.shape != shape or t.dtype != torch.int32 or t.device != dev:
        raise ValueError(f'{what} must be int32 {tuple(shape)} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}')
    return t


def _refused(cfg, B, R, gmax):
    return NotImplementedError(f'bbox targets on the HIP engine: R {R} (1..{MAX_PRE}), Gmax {gmax} (1..{MAX_GT}), num {cfg.num} (1..{MAX_PRE}), num_pos '
                               f'{cfg.num_pos} in [0, num], num_classes {cfg.num_classes} (1..{MAX_CLASSES}), thresholds ({cfg.pos_iou_thr}, '
                               f'{cfg.neg_iou_thr}, {cfg.min_pos_iou}) in [0, 1], stds {list(cfg.stds)} > 0, beta {cfg.beta} > 0, finite loss '
                               f'weights or B {B} are not supported')


def bbox_targets(rois, gt, gt_labels, gt_count, cfg, first=None, count=None, keys=None, rng=None, stage=0, stream=None):
    """hrf_bbox_targets: rois (B*R,5) fp32, image b at rows b*R..; gt (B,Gmax,4) / gt_count (B,) from rpn.pack_gts, gt_labels (B,Gmax)
    int32 (pack_gt_labels); cfg: rcnn_train_cfg_struct(...); first / count: int32 (B,) views of ONE stride (two columns of an earlier
    stage's `counts` are read in place) or None; keys (B,Gmax+R) int32 (uint32 values) or rng = rpn.rng_state(seed, counter) (never
    advanced here) -> (rois_s (B*num,5), labels (B*num,) int32, bbox_targets (B*num,4), src (B*num,) int32, counts (B,6) int32,
    assigned (B,Gmax+R) int32, max_iou (B,Gmax+R) fp32)"""
    L = _lib.lib()
    dev = rois.device
    if gt.dim() != 3 or gt.shape[2] != 4 or gt.dtype != torch.float32 or not gt.is_contiguous() or gt.device != dev:
        raise ValueError(f'bbox_targets: gt must be contiguous fp32 (B, Gmax, 4) on {dev}, got {tuple(gt.shape)} {gt.dtype} on {gt.device}')
    B, gmax = gt.shape[0], gt.shape[1]
    if rois.dim() != 2 or rois.shape[1] != 5 or rois.dtype != torch.float32 or not rois.is_contiguous() or rois.shape[0] % B != 0:
        raise ValueError(f'bbox_targets: rois must be contiguous fp32 (B * R, 5), got {tuple(rois.shape)} {rois.dtype} for B = {B}')
    R = rois.shape[0] // B
    _i32(gt_count, (B,), dev, 'bbox_targets: gt_count')
    if not _i32(gt_labels, (B, gmax), dev, 'bbox_targets: gt_labels').is_contiguous():
        raise ValueError('bbox_targets: gt_labels must be contiguous')
    rs = 1
    for t, what in ((first, 'first'), (count, 'count')):
        if t is not None:
            _i32(t, (B,), dev, 'bbox_targets: ' + what)
    strides = {max(int(t.stride(0)), 1) for t in (first, count) if t is not None and B > 1}
    if len(strides) > 1:
        raise ValueError('bbox_targets: first and count must share one stride')
    if strides:
        rs = strides.pop()
    if keys is not None and (keys.shape != (B, gmax + R) or keys.dtype != torch.int32 or not keys.is_contiguous() or keys.device != dev):
        raise ValueError(f'bbox_targets: keys must be contiguous int32 ({B}, {gmax + R}) holding uint32 values on {dev}, got {tuple(keys.shape)} {keys.dtype}')
    if keys is None and (rng is None or rng.shape != (2,) or rng.dtype != torch.int32 or rng.device != dev):
        raise ValueError(f'bbox_targets: without keys an int32 (2,) rng_state (seed, counter) on {dev} is needed (rpn.rng_state)')
    if L.require_cuda and not rois.is_cuda:
        raise _lib.HRFuserHipError(f'bbox_targets: tensor on {dev}; the HIP path has no CPU fallback')
    if not L.hrf_bbox_train_supported(cfg, B, R, gmax):
        raise _refused(cfg, B, R, gmax)
    n = B * cfg.num
    outs = (torch.empty((n, 5), device=dev, dtype=torch.float32), torch.empty((n,), device=dev, dtype=torch.int32),
            torch.empty((n, 4), device=dev, dtype=torch.float32), torch.empty((n,), device=dev, dtype=torch.int32),
            torch.empty((B, 6), device=dev, dtype=torch.int32), torch.empty((B, gmax + R), device=dev, dtype=torch.int32),
            torch.empty((B, gmax + R), device=dev, dtype=torch.float32))
    L.hrf_bbox_targets(cfg, B, R, rois, first, count, rs, gt, gt_labels, gt_count, gmax, keys, rng, int(stage), *outs, _stream(stream))
    return outs


def bbox_loss(out, labels, targets, counts, cfg, rng=None, d_out=None, losses=None, workspace=None, stream=None):
    """hrf_bbox_loss: out (B*num, >= num_classes + 5) fp32 rows of one pitch (the padded head output), labels / targets / counts of
    bbox_targets -> (losses (3,) fp32 = loss_cls, loss_bbox, acc; d_out (B*num, ceil16(num_classes + 5)): d (loss_cls + loss_bbox) /
    d out - the dY of the fused fc_cls / fc_reg GEMM).  rng: the rng_state whose counter this call advances (the last stage of a
    step), or None.  d_out / losses: buffers to write into instead of new ones."""
    L = _lib.lib()
    dev, B = out.device, counts.shape[0]
    n, P = B * cfg.num, _ceil16(cfg.num_classes + 5)
    if out.dim() != 2 or out.shape[0] != n or out.shape[1] < cfg.num_classes + 5 or out.dtype != torch.float32 or out.stride(1) != 1:
        raise ValueError(f'bbox_loss: out must be fp32 ({n}, >= {cfg.num_classes + 5}) rows, got {tuple(out.shape)} {out.dtype}')
    _i32(labels, (n,), dev, 'bbox_loss: labels')
    _i32(counts, (B, 6), dev, 'bbox_loss: counts')
    if targets.shape != (n, 4) or targets.dtype != torch.float32 or not targets.is_contiguous() or not labels.is_contiguous() or not counts.is_contiguous():
        raise ValueError(f'bbox_loss: contiguous labels ({n},), targets fp32 ({n}, 4) and counts ({B}, 6) are needed')
    if L.require_cuda and not out.is_cuda:
        raise _lib.HRFuserHipError(f'bbox_loss: tensor on {dev}; the HIP path has no CPU fallback')
    need = L.hrf_bbox_train_workspace_bytes(cfg, B, 1, 1)
    if need == 0:
        raise _refused(cfg, B, 1, 1)
    if workspace is None:
        workspace = torch.empty((need,), device=dev, dtype=torch.uint8)
    if d_out is None:
        d_out = torch.empty((n, P), device=dev, dtype=torch.float32)
    if d_out.shape[0] != n or d_out.shape[1] < P or d_out.dtype != torch.float32 or d_out.stride(1) != 1 or d_out.device != dev:
        raise ValueError(f'bbox_loss: d_out must be fp32 ({n}, >= {P}) rows on {dev}, got {tuple(d_out.shape)} {d_out.dtype}')
    if losses is None:
        losses = torch.empty((3,), device=dev, dtype=torch.float32)
    ld = out.stride(0) if n > 1 else max(out.stride(0), out.shape[1])
    ldd = d_out.stride(0) if n > 1 else max(d_out.stride(0), d_out.shape[1])
    L.hrf_bbox_loss(cfg, B, out, ld, labels, targets, counts, workspace, workspace.numel(), d_out, ldd, losses, rng, _stream(stream))
    return losses, d_out


class _BboxLossFn(torch.autograd.Function):
    """torch.autograd bridge of Shared2FCBBoxHead.loss: forward runs hrf_bbox_loss on a packed copy of (cls_score, bbox_pred) and
    keeps the gradient rows; backward scales them by the incoming per-loss gradients.  The gradient of loss_cls lives in the logit
    columns alone and that of loss_bbox in the delta columns alone, so one buffer serves both."""

    @staticmethod
    def forward(fctx, cfg, labels, targets, counts, cls_score, bbox_pred):
        nc = cfg.num_classes
        out = torch.zeros((cls_score.shape[0], _ceil16(nc + 5)), device=cls_score.device, dtype=torch.float32)
        out[:, :nc + 1], out[:, nc + 1:nc + 5] = cls_score.detach().float(), bbox_pred.detach().float()
        losses, d = bbox_loss(out, labels, targets, counts, cfg)
        fctx.hrf = (d, nc)
        return losses

    @staticmethod
    def backward(fctx, gl):
        d, nc = fctx.hrf
        gl = gl.float()
        return None, None, None, None, d[:, :nc + 1] * gl[0], d[:, nc + 1:nc + 5] * gl[1]


class _HeadFn(torch.autograd.Function):
    """torch.autograd bridge of Shared2FCBBoxHead.forward_autograd over run_train / run_backward.  The parameters are not autograd
    inputs: run_backward adds their gradients into .grad itself."""

    @staticmethod
    def forward(fctx, head, nhwc, x):
        out, saved = head.run_train(x.detach().float().contiguous().reshape(x.shape[0], -1), nhwc=nhwc)
        fctx.hrf = (head, saved, tuple(x.shape))
        return out

    @staticmethod
    def backward(fctx, gout):
        head, saved, shape = fctx.hrf
        g = gout.float()
        if g.stride(1) != 1:
            g = g.contiguous()
        dx = head.run_backward(saved, g, need_dx=fctx.needs_input_grad[2])
        return None, None, (None if dx is None else dx.reshape(shape))


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

    # -- training: the same forward with what the backward needs kept, and the backward (csrc/hrf_fc_bwd.h) -----------------
    def run_train(self, x2d, nhwc=False, stream=None):
        """`run` (the same launches, the same bits) -> (out, saved): saved keeps x2d, the two hidden activations and the packed
        weights the forward used, for `run_backward`"""
        L = _lib.lib()
        if L.require_cuda and not x2d.is_cuda:
            raise _lib.HRFuserHipError(f'Shared2FCBBoxHead: tensor on {x2d.device}; the HIP path has no CPU fallback')
        dev = x2d.device
        pk = self._packed(dev)
        if x2d.dim() != 2 or x2d.shape[1] != pk['Kin'] or x2d.dtype != torch.float32 or not x2d.is_contiguous():
            raise ValueError(f'Shared2FCBBoxHead: features must be contiguous fp32 (K, {pk["Kin"]}), got {tuple(x2d.shape)} {x2d.dtype}')
        F = self.fc_out_channels
        w1 = self._w1(pk, dev, nhwc)
        h1 = fc(x2d, w1, pk['b1'], F, True, stream=stream, consts=pk['consts'])
        h2 = fc(h1, pk['w2'], pk['b2'], F, True, stream=stream, consts=pk['consts'])
        out = fc(h2, pk['w3'], pk['b3'], self.out_pitch, False, stream=stream)
        return out, dict(x=x2d, h1=h1, h2=h2, w1=w1, w2=pk['w2'], w3=pk['w3'], nhwc=bool(nhwc))

    def _grad_pair(self, lin, dev):
        """(weight.grad, bias.grad, accumulate) of a Linear: existing gradients are added to, missing ones created"""
        w, b = lin.weight, lin.bias
        fresh = w.grad is None and b.grad is None
        for p in (w, b):
            if p.grad is None:
                p.grad = torch.empty_like(p, memory_format=torch.contiguous_format) if fresh else torch.zeros_like(p, memory_format=torch.contiguous_format)
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != dev:
                raise _not_built('Shared2FCBBoxHead', 'parameter .grad', (p.grad.dtype, str(p.grad.device)), f'contiguous fp32 on {dev}')
        return w.grad, b.grad, not fresh

    def run_backward(self, saved, d_out, need_dx=True, stream=None):
        """The backward of `run_train`: d_out (K, >= out_pitch) rows, the gradient on the padded output (hrf_bbox_loss's d_out) ->
        the gradient on x2d (K, 49 * C) in x2d's column order, or None (need_dx False).  Six launches of the two backward kernels -
        w3 weight / data, w2 weight / data, w1 weight / (data) - plus the bias sums; each data gradient carries the ReLU mask of the
        layer below.  Adds into .grad of the eight parameters, in the parameters' own shape and order (created when None): rows
        [0, num_classes] of the padded last layer are fc_cls, the next four fc_reg, the padding rows go nowhere; fc1's gradient
        taken on (y, x, c) feature columns is brought back to (c, y, x) by hrf_fc_bwd_cols."""
        L = _lib.lib()
        x, h1, h2 = saved['x'], saved['h1'], saved['h2']
        dev, M = x.device, x.shape[0]
        F, Kin, P, nc = self.fc_out_channels, self.in_channels * self.roi_feat_area, self.out_pitch, self.num_classes
        if d_out.dim() != 2 or d_out.shape[0] != M or d_out.shape[1] < P or d_out.dtype != torch.float32 or d_out.stride(1) != 1 or d_out.device != dev:
            raise ValueError(f'Shared2FCBBoxHead.run_backward: d_out must be fp32 ({M}, >= {P}) rows on {dev}, got {tuple(d_out.shape)} {d_out.dtype}')
        s = _stream(stream)
        # last layer: one padded gradient, its rows handed to the two parameters
        ws = fc_bwd_workspace(M, F, P, dev)
        dw3, db3 = torch.empty((P, F), device=dev), torch.empty((P,), device=dev)
        fc_backward_weight(h2, d_out, P, dw3, db3, False, ws, s)
        for lin, lo, hi in ((self.fc_cls, 0, nc + 1), (self.fc_reg, nc + 1, nc + 5)):
            gw, gb, acc = self._grad_pair(lin, dev)
            n = gw.numel()
            L.hrf_scale_add(dw3[lo:hi], None, 1.0, None, 1, gw if acc else None, None, gw, n, 1, s)
            L.hrf_scale_add(db3[lo:hi], None, 1.0, None, 1, gb if acc else None, None, gb, hi - lo, 1, s)
        d2 = fc_backward_data(d_out, saved['w3'], F, h2, None, ws, s)
        # fc2
        ws = fc_bwd_workspace(M, F, F, dev)
        gw, gb, acc = self._grad_pair(self.shared_fcs[1], dev)
        fc_backward_weight(h1, d2, F, gw, gb, acc, ws, s)
        d1 = fc_backward_data(d2, saved['w2'], F, h1, None, ws, s)
        # fc1
        ws = fc_bwd_workspace(M, Kin, F, dev)
        gw, gb, acc = self._grad_pair(self.shared_fcs[0], dev)
        if saved['nhwc']:
            tmp, tmpb = torch.empty((F, Kin), device=dev), torch.empty((F,), device=dev)
            fc_backward_weight(x, d1, F, tmp, tmpb, False, ws, s)
            L.hrf_fc_bwd_cols(tmp, Kin, gw, Kin, int(acc), F, self.in_channels, self.roi_feat_area, s)
            L.hrf_scale_add(tmpb, None, 1.0, None, 1, gb if acc else None, None, gb, F, 1, s)
        else:
            fc_backward_weight(x, d1, F, gw, gb, acc, ws, s)
        if not need_dx:
            return None
        return fc_backward_data(d1, saved['w1'], Kin, None, None, ws, s)

    def forward_autograd(self, x, layout=None):
        """`forward` with a grad_fn on (cls_score, bbox_pred): backward runs `run_backward`, which leaves the parameter gradients
        in .grad and delivers x.grad in x's layout.  With `loss` and SingleRoIExtractor.forward a .backward() on s{i}.loss_*
        reaches the pyramid."""
        C, nc = self.in_channels, self.num_classes
        if layout is None:
            layout = 'nchw' if tuple(x.shape[1:]) == (C, POOLED, POOLED) else 'nhwc'
        want = (C, POOLED, POOLED) if layout == 'nchw' else (POOLED, POOLED, C)
        if x.dim() != 4 or tuple(x.shape[1:]) != want:
            raise ValueError(f'Shared2FCBBoxHead.forward_autograd: expected (K, {want[0]}, {want[1]}, {want[2]}) ({layout}), got {tuple(x.shape)}')
        out = _HeadFn.apply(self, layout == 'nhwc', x)
        return out[:, :nc + 1], out[:, nc + 1:nc + 5]

    def _no_train_cfg(self, what):
        return NotImplementedError(f'Shared2FCBBoxHead on the HIP engine: {what} is not built without a train_cfg - assigners, samplers and losses are '
                                   'named by the train_cfg of the CascadeRoIHead that owns the head; this head is forward only')

    def _stage_cfg(self, n=None):
        """the hrf_bbox_train_cfg_t of the owning stage; n: one `image` of n rows (the rows of a whole batch, mmdet's loss signature)"""
        kw = dict(self.__dict__['_rcnn_train'])
        if n is not None:
            kw.update(num=n, num_pos=min(kw['num_pos'], n))
        return rcnn_train_cfg_struct(**kw)

    def get_targets(self, *args, **kwargs):
        """bbox_head.py:187-255 on the fixed-shape sampling results of this engine.  Signature (sampling_results, gt_bboxes, gt_labels,
        rcnn_train_cfg=None, concat=True); sampling_results: what `bbox_targets` returned for the stage (the kernel has encoded the
        targets already; gt_bboxes / gt_labels are not read again) -> (labels (B*num,) int64 with num_classes on the padding, as a
        zero label weight makes it irrelevant, label_weights, bbox_targets (B*num,4), bbox_weights (B*num,4))"""
        if '_rcnn_train' not in self.__dict__:
            raise self._no_train_cfg('get_targets')
        return self._get_targets(*args, **kwargs)

    def _get_targets(self, sampling_results, gt_bboxes=None, gt_labels=None, rcnn_train_cfg=None, concat=True):
        if not concat:
            raise _not_built('Shared2FCBBoxHead', 'get_targets concat', concat, 'the kernels keep the rows of a batch in one buffer')
        if not isinstance(sampling_results, (tuple, list)) or len(sampling_results) != 7 or not isinstance(sampling_results[1], torch.Tensor):
            raise _not_built('Shared2FCBBoxHead', 'get_targets sampling_results', type(sampling_results).__name__,
                             'the tuple roi_head.bbox_targets returns; mmdet SamplingResult objects are not')
        _, labels, targets = sampling_results[:3]
        nc = self.num_classes
        lw = (labels >= 0).float()
        bw = ((labels >= 0) & (labels < nc)).float()[:, None].expand(-1, 4)
        return torch.where(labels >= 0, labels, torch.full_like(labels, nc)).long(), lw, targets, bw

    def loss(self, *args, **kwargs):
        """bbox_head.py:257-313 -> dict(loss_cls, acc, loss_bbox) with a grad_fn: backward delivers the kernel's gradient, scaled by
        the incoming gradients, to cls_score / bbox_pred.  Signature (cls_score (n, num_classes + 1), bbox_pred (n, 4), rois, labels,
        label_weights, bbox_targets, bbox_weights, reduction_override=None); n <= HRF_RPN_MAX_PRE rows.  A zero label weight marks
        a padding row; the other weights are what get_targets gives (1 / positives), they are not read again."""
        if '_rcnn_train' not in self.__dict__:
            raise self._no_train_cfg('loss')
        return self._loss(*args, **kwargs)

    def _loss(self, cls_score, bbox_pred, rois, labels, label_weights, bbox_targets, bbox_weights, reduction_override=None):
        if reduction_override is not None:
            raise _not_built('Shared2FCBBoxHead', 'loss reduction_override', reduction_override, 'mean, the default')
        n, nc, dev = int(cls_score.shape[0]), self.num_classes, cls_score.device
        if not 1 <= n <= MAX_PRE or tuple(cls_score.shape) != (n, nc + 1) or tuple(bbox_pred.shape) != (n, 4):
            raise _not_built('Shared2FCBBoxHead', 'loss rows', (tuple(cls_score.shape), tuple(bbox_pred.shape)),
                             f'(n, {nc + 1}) logits and (n, 4) class-agnostic deltas with 1 <= n <= {MAX_PRE}')
        lab = torch.where(label_weights > 0, labels, torch.full_like(labels, -1)).to(device=dev, dtype=torch.int32).contiguous()
        counts = torch.zeros((1, 6), device=dev, dtype=torch.int32)
        counts[0, 5:6] = (lab >= 0).sum().to(torch.int32)           # the average factor, counted on the device: nothing synchronises
        losses = _BboxLossFn.apply(self._stage_cfg(n), lab, bbox_targets.detach().float().contiguous().to(dev), counts, cls_score, bbox_pred)
        return dict(loss_cls=losses[0], acc=losses[2], loss_bbox=losses[1])


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
        if train_cfg is not None:                                  # an unsupported assigner / sampler / loss raises at build time
            self.__dict__['_stage_train'] = self._rcnn_train_cfg(train_cfg, self.bbox_head, self.stage_loss_weights)
            for h, kw in zip(self.bbox_head, self._stage_train):
                h.__dict__['_rcnn_train'] = kw
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

    # -- training: targets and losses (csrc/hrf_bbox_train.h) ---------------------------------------------
    @staticmethod
    def _rcnn_train_cfg(train_cfg, heads, stage_loss_weights):
        """-> per stage the keywords of rcnn_train_cfg_struct for train_cfg.rcnn (a list of dicts, one per stage) + the stage's head
        and loss weight; anything the kernels do not build raises NotImplementedError naming the key"""
        who = 'CascadeRoIHead'
        if not isinstance(train_cfg, (list, tuple)) or len(train_cfg) != len(heads):
            raise _not_built(who, 'train_cfg', train_cfg if not isinstance(train_cfg, (list, tuple)) else f'{len(train_cfg)} entries',
                             f'a list of one dict per stage ({len(heads)} stages)')
        out = []
        for i, (tc_, hd, sw) in enumerate(zip(train_cfg, heads, stage_loss_weights)):
            tc, pre = dict(tc_), f'train_cfg[{i}].'
            asg, smp = dict(tc.pop('assigner', {})), dict(tc.pop('sampler', {}))
            if asg.pop('type', None) != 'MaxIoUAssigner':
                raise _not_built(who, pre + 'assigner.type', tc_.get('assigner', {}).get('type'), 'MaxIoUAssigner in every HRFuser config')
            pos, neg = asg.pop('pos_iou_thr', None), asg.pop('neg_iou_thr', None)
            if isinstance(neg, (tuple, list)) or not isinstance(neg, (int, float)) or not isinstance(pos, (int, float)):
                raise _not_built(who, pre + 'assigner.pos_iou_thr / neg_iou_thr', (pos, neg), 'two numbers; a (low, high) tuple for neg_iou_thr is not')
            min_pos = float(asg.pop('min_pos_iou', 0.0))
            if asg.pop('match_low_quality', True):
                raise _not_built(who, pre + 'assigner.match_low_quality', True, 'False in every HRFuser config; the RPN kernels have the low-quality pass')
            if asg.pop('ignore_iof_thr', -1) >= 0:
                raise _not_built(who, pre + 'assigner.ignore_iof_thr', tc_['assigner']['ignore_iof_thr'], 'gt_bboxes_ignore is out of scope; -1 in every HRFuser config')
            asg.pop('ignore_wrt_candidates', True)                      # (only read with ignore_iof_thr >= 0)
            asg.pop('gt_max_assign_all', True)                          # (only read with match_low_quality)
            if asg.pop('gpu_assign_thr', -1) != -1:
                raise _not_built(who, pre + 'assigner.gpu_assign_thr', tc_['assigner']['gpu_assign_thr'], 'the assignment never leaves the device; -1')
            if dict(asg.pop('iou_calculator', dict(type='BboxOverlaps2D'))) != dict(type='BboxOverlaps2D') or asg:
                raise _not_built(who, pre + 'assigner keys', sorted(asg) or 'iou_calculator', 'unknown to the kernel')
            if smp.pop('type', None) != 'RandomSampler':
                raise _not_built(who, pre + 'sampler.type', tc_.get('sampler', {}).get('type'), 'RandomSampler in every HRFuser config; OHEM is out of scope')
            num, frac = smp.pop('num', None), smp.pop('pos_fraction', None)
            if not isinstance(num, int) or not 1 <= num <= MAX_PRE or frac is None or not 0.0 <= float(frac) <= 1.0:
                raise _not_built(who, pre + 'sampler.num / pos_fraction', (num, frac), f'1 <= num <= {MAX_PRE} and 0 <= pos_fraction <= 1')
            if smp.pop('neg_pos_ub', -1) >= 0:
                raise _not_built(who, pre + 'sampler.neg_pos_ub', tc_['sampler']['neg_pos_ub'], '-1 in every HRFuser config')
            add_gt = bool(smp.pop('add_gt_as_proposals', True))
            if smp:
                raise _not_built(who, pre + 'sampler keys', sorted(smp), 'unknown to the kernel')
            if tc.get('pos_weight', -1) > 0:
                raise _not_built(who, pre + 'pos_weight', tc['pos_weight'], '-1 in every HRFuser config')
            if tc.get('debug', False):
                raise _not_built(who, pre + 'debug', True, 'False')
            lc, lb = dict(hd.loss_cls or {}), dict(hd.loss_bbox or {})
            if lc.get('class_weight') is not None or lc.get('reduction', 'mean') != 'mean':
                raise _not_built(who, f'bbox_head[{i}].loss_cls', hd.loss_cls, 'a softmax CrossEntropyLoss with mean reduction and no class_weight')
            if lb.get('type') != 'SmoothL1Loss' or lb.get('reduction', 'mean') != 'mean' or not float(lb.get('beta', 1.0)) > 0:
                raise _not_built(who, f'bbox_head[{i}].loss_bbox', hd.loss_bbox, 'a SmoothL1Loss with beta > 0 and mean reduction')
            out.append(dict(pos_iou_thr=float(pos), neg_iou_thr=float(neg), min_pos_iou=min_pos, add_gt_as_proposals=add_gt, num=num,
                            num_pos=int(num * float(frac)), num_classes=hd.num_classes, stds=hd.target_stds, beta=float(lb.get('beta', 1.0)),
                            loss_weight_cls=float(lc.get('loss_weight', 1.0)) * float(sw), loss_weight_bbox=float(lb.get('loss_weight', 1.0)) * float(sw)))
        return out

    def _no_train_cfg(self, what):
        return NotImplementedError(f'CascadeRoIHead on the HIP engine: {what} is not built without train_cfg - the assigners and samplers of the '
                                   'stages are named there (train_cfg.rcnn); the head is detect / simple_test only')

    def rng(self, device):
        """the device (seed, counter) pair the samplers draw from (rpn.rng_state); `losses` advances the counter once per call"""
        st = self.__dict__.get('_rng')
        if st is None or st.device != torch.device(device):
            st = self.__dict__['_rng'] = rng_state(int(torch.initial_seed()), 0, device)
        return st

    def losses(self, *args, **kwargs):
        """All stages of cascade_roi_head.py:191-286 with fixed shapes.  Signature (x, rois, count, gt, gt_labels, gt_count, img_shapes,
        stages=None, keys=None): x the pyramid; rois (B*R,5) / count (B,) int32 or None as `detect` takes them (RPNHead.proposals);
        gt (B,Gmax,4) fp32, gt_labels (B,Gmax) int32, gt_count (B,) int32 on the device (rpn.pack_gts, pack_gt_labels); img_shapes a
        device (B,2) tensor or a list -> (losses (num_stages, 3) fp32: loss_cls, loss_bbox (both with the stage weight), acc per
        stage; [d_out (B*num, ceil16(num_classes + 5))] per stage: the gradient of the stage's two losses on its padded head output,
        the dY of its fc_cls / fc_reg GEMM).  Per stage hrf_bbox_targets -> hrf_roi_align_fwd -> Shared2FCBBoxHead.run ->
        hrf_bbox_loss -> hrf_bbox_refine; the next stage reads rows [sampled gts, n_b) of the refined rows in place.  No host read,
        no synchronisation: capturable; a captured graph follows changed gt / gt_labels / gt_count / rois contents and the last
        launch advances the counter of `rng`.  stages: a list that receives a dict per stage (rois, first, count, targets, out,
        d_out, cfg); keys: per stage explicit sampling keys (B, Gmax + R_stage) int32 instead of the generated ones."""
        if self.train_cfg is None:
            raise self._no_train_cfg('losses')
        return self._losses(*args, **kwargs)

    loss = losses

    def _losses(self, x, rois, count, gt, gt_labels, gt_count, img_shapes, stages=None, keys=None):
        x = tuple(x)
        B, dev = x[0].shape[0], x[0].device
        rois = rois.detach().float().contiguous()
        if rois.dim() != 2 or rois.shape[1] != 5 or rois.shape[0] % B != 0 or rois.shape[0] == 0:
            raise ValueError(f'CascadeRoIHead.losses: rois must be (B * R, 5) with R >= 1, got {tuple(rois.shape)} for B = {B}')
        shp = _shapes(img_shapes, B, dev)
        nc, S = self.bbox_head[0].num_classes, self.num_stages
        rng = None if keys is not None else self.rng(dev)
        out_losses = torch.empty((S, 3), device=dev, dtype=torch.float32)
        maps, grads, first = {}, [], None
        with torch.no_grad():
            for i in range(S):
                ex, hd = self.bbox_roi_extractor[i], self.bbox_head[i]
                n = ex.num_inputs
                if n not in maps:
                    if len(x) < n:
                        raise ValueError(f'CascadeRoIHead: {n} strides, {len(x)} maps')
                    maps[n] = [_nhwc(t) for t in x[:n]]
                cfg = rcnn_train_cfg_struct(**self._stage_train[i])
                t = bbox_targets(rois, gt, gt_labels, gt_count, cfg, first, count, keys=None if keys is None else keys[i], rng=rng, stage=i)
                rois_s, labels, targets, _, counts = t[:5]
                feat = roi_forward(maps[n], rois_s, ex._scales(), float(ex.finest_scale), 1)         # (B*num,7,7,C)
                out = hd.run(feat.reshape(feat.shape[0], -1), nhwc=True)
                _, d = bbox_loss(out, labels, targets, counts, cfg, rng=rng if i == S - 1 else None, losses=out_losses[i])
                grads.append(d)
                if stages is not None:
                    stages.append(dict(rois=rois, first=first, count=count, targets=t, out=out, d_out=d, cfg=cfg))
                if i < S - 1:
                    rois = bbox_refine(rois_s, out[:, nc + 1:nc + 5], hd.target_stds, shp, B)
                    first, count = counts[:, 4], counts[:, 5]      # the sampled gts lead every image: the pos_is_gt filter is a row range
        return out_losses, grads

    def losses_nhwc(self, *args, **kwargs):
        """`losses` on the tape.  Signature (ctx, acts, rois, count, gt, gt_labels, gt_count, img_shapes, stages=None, keys=None): acts
        the runtime.Act's of the pyramid (HRFPN._run's outputs, NHWC, read in place), the rest as `losses` -> what `losses`
        returns, the same bits for the same inputs and keys (the same launches in the same order).  With a recording ctx every
        stage pushes its backward: the features come through SingleRoIExtractor.extract_nhwc (whose closure is the RoIAlign
        adjoint) and the head's closure runs Shared2FCBBoxHead.run_backward on the stage's d_out, which fills the features'
        gradient.  ctx.run_backward() then adds into act.grad of the used levels and into .grad of the head parameters.  No
        gradient flows through the boxes between the stages (cascade_roi_head.py:269 refines them under no_grad).  Fixed
        shapes, no host read, no synchronisation: forward and backward are capturable.  The FC backward is free of atomics;
        hrf_roi_align_bwd is not, and stays refused in deterministic mode."""
        if self.train_cfg is None:
            raise self._no_train_cfg('losses_nhwc')
        return self._losses_nhwc(*args, **kwargs)

    def _losses_nhwc(self, ctx, acts, rois, count, gt, gt_labels, gt_count, img_shapes, stages=None, keys=None, out_layout=1):
        acts = list(acts)
        B, dev = acts[0].t.shape[0], acts[0].t.device
        rois = rois.detach().float().contiguous()
        if rois.dim() != 2 or rois.shape[1] != 5 or rois.shape[0] % B != 0 or rois.shape[0] == 0:
            raise ValueError(f'CascadeRoIHead.losses_nhwc: rois must be (B * R, 5) with R >= 1, got {tuple(rois.shape)} for B = {B}')
        shp = _shapes(img_shapes, B, dev)
        nc, S = self.bbox_head[0].num_classes, self.num_stages
        rng = None if keys is not None else self.rng(dev)
        out_losses = torch.empty((S, 3), device=dev, dtype=torch.float32)
        grads, first, s = [], None, ctx.stream
        with torch.no_grad():
            for i in range(S):
                ex, hd = self.bbox_roi_extractor[i], self.bbox_head[i]
                if len(acts) < ex.num_inputs:
                    raise ValueError(f'CascadeRoIHead: {ex.num_inputs} strides, {len(acts)} maps')
                cfg = rcnn_train_cfg_struct(**self._stage_train[i])
                t = bbox_targets(rois, gt, gt_labels, gt_count, cfg, first, count, keys=None if keys is None else keys[i], rng=rng, stage=i, stream=s)
                rois_s, labels, targets, _, counts = t[:5]
                # (y, x, c) feature columns, as `losses` runs them: the values are the same bits; out_layout 0 is the A/B of
                # tools/fc_bwd_cost.py (fc1's gradient then needs no hrf_fc_bwd_cols)
                feat = ex.extract_nhwc(ctx, acts, rois_s, out_layout=out_layout)
                out, saved = hd.run_train(feat.t.reshape(feat.t.shape[0], -1), nhwc=out_layout == 1, stream=s)
                _, d = bbox_loss(out, labels, targets, counts, cfg, rng=rng if i == S - 1 else None, losses=out_losses[i], stream=s)
                grads.append(d)

                def bwd(hd=hd, saved=saved, d=d, feat=feat, used=acts[:ex.num_inputs]):
                    dx = hd.run_backward(saved, d, need_dx=any(a.needs_grad for a in used), stream=ctx.stream)
                    if dx is not None:
                        feat.grad = dx.reshape(feat.t.shape)
                ctx.push(bwd)
                if stages is not None:
                    stages.append(dict(rois=rois, first=first, count=count, targets=t, out=out, d_out=d, cfg=cfg, feat=feat))
                if i < S - 1:
                    rois = bbox_refine(rois_s, out[:, nc + 1:nc + 5], hd.target_stds, shp, B, stream=s)
                    first, count = counts[:, 4], counts[:, 5]
        nmax = max(ex.num_inputs for ex in self.bbox_roi_extractor)

        def bwd_first():                                            # pushed last: the first closure of this part of the tape
            for a in acts[:nmax]:                                   # the RoIAlign adjoint adds into act.grad: zeroed maps where there is none yet
                if a.needs_grad and a.grad is None:
                    a.grad = R._keep(torch.zeros_like(a.t))
        ctx.push(bwd_first)
        return out_losses, grads

    def forward_train(self, *args, **kwargs):
        """cascade_roi_head.py:191-286 -> mmdet's dict: s{i}.loss_cls, s{i}.acc, s{i}.loss_bbox (the stage weight on the two losses
        only).  Signature (x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None); proposal_list: a
        list of (n_i, >= 4) boxes per image, or the fixed-shape pair (rois (B*R,5), count (B,) int32) of RPNHead.proposals;
        gt_bboxes / gt_labels: lists per image (packed without a synchronisation).  The head's forward is no_grad: the values carry
        no grad_fn; `losses` returns the gradient buffers."""
        if self.train_cfg is None:
            raise self._no_train_cfg('forward_train')
        return self._forward_train(*args, **kwargs)

    def _forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None, stages=None):
        if gt_bboxes_ignore is not None:
            raise _not_built('CascadeRoIHead', 'gt_bboxes_ignore', 'given', 'ignore regions are out of scope')
        if gt_masks is not None:
            raise _not_built('CascadeRoIHead', 'gt_masks', 'given', 'mask heads are out of scope')
        x = tuple(x)
        dev = x[0].device
        if isinstance(proposal_list, tuple) and len(proposal_list) == 2 and isinstance(proposal_list[0], torch.Tensor) and proposal_list[0].dim() == 2 \
                and proposal_list[0].shape[1] == 5 and proposal_list[1].dim() == 1:
            rois, count = proposal_list
        else:
            B = len(proposal_list)
            R = max([int(p.shape[0]) for p in proposal_list] + [1])
            rois = torch.zeros((B, R, 5), device=dev, dtype=torch.float32)
            for b, p in enumerate(proposal_list):
                rois[b, :, 0] = float(b)
                rois[b, :p.shape[0], 1:] = p[:, :4].to(dev).float()
            rois = rois.reshape(B * R, 5)
            count = torch.tensor([int(p.shape[0]) for p in proposal_list], dtype=torch.int32).to(dev)
        gt, gt_count = pack_gts(gt_bboxes, dev)
        vals, _ = self.losses(x, rois, count, gt, pack_gt_labels(gt_labels, dev, gt.shape[1]), gt_count, [m['img_shape'] for m in img_metas], stages=stages)
        out = {}
        for i in range(self.num_stages):
            out[f's{i}.loss_cls'], out[f's{i}.acc'], out[f's{i}.loss_bbox'] = vals[i, 0], vals[i, 2], vals[i, 1]
        return out
