"""Harness that runs a SUB-BLOCK of the backbone (Bottleneck, HRFormerBlock, fusion block, HR
module ...) on the HIP engine with NCHW torch tensors in/out, so block-level parity tests can
compare each piece against the oracle exactly like the reference's own module boundaries."""
import torch

from . import runtime as R
from .backbone import HipModule


class BlockHarness(HipModule):
    """`runner(ctx, block, acts) -> list[Act]`; inputs/outputs are logical NCHW tensors."""

    def __init__(self, block, runner):
        super().__init__()
        self.block = block
        self._runner = runner

    def forward(self, *inputs):
        return self._call_engine(tuple(inputs))

    def _wrap_inputs(self, inputs):
        return [R.Act(t.permute(0, 2, 3, 1).contiguous(), bool(t.requires_grad)) for t in inputs]

    def _run(self, ctx, srcs):
        outs = self._runner(ctx, self.block, srcs)
        return list(outs) if isinstance(outs, (list, tuple)) else [outs]


# ----------------------------------------------------------------------------- SingleRoIExtractor / RoIAlign restatement
# The oracle of hrfuser_amd.roi (mmcv is not installed here: parity against real mmcv is unpinned).  A literal fp64
# restatement of mmcv 1.3.17 RoIAlign(aligned=True, pool_mode='avg', sampling_ratio=0): the per-sample loop, four corners per
# sample.  Only the sample positions and the integer decisions are plain Python; the feature values pass through differentiable
# torch ops, so torch.autograd.grad of the result IS the backward reference.  tests/test_roi_align.py pins it against
# F.grid_sample + avg_pool2d on boxes that stay inside the map.
def roi_level_ref(rois, num_levels, finest_scale=56):
    """map_roi_levels (single_level_roi_extractor.py:36-55) in fp32, as the reference evaluates it -> (K,) int64.  A box whose
    scale is NaN (a negative area) matches no level there and keeps its row of zeros: level -1 here."""
    r = rois.detach().float().cpu()
    s = torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
    lv = torch.floor(torch.log2(s / finest_scale + 1e-6)).clamp(min=0, max=num_levels - 1)
    return torch.where(torch.isnan(lv), torch.full_like(lv, -1), lv).long()


def roi_samples(box, spatial_scale, H, W, P=7):
    """Sample positions of one box (x1, y1, x2, y2 as Python floats) -> (ys [P][grid_h], xs [P][grid_w], count)."""
    import math
    x1, y1, x2, y2 = (float(v) * spatial_scale - 0.5 for v in box)
    rw, rh = x2 - x1, y2 - y1
    bin_h, bin_w = rh / P, rw / P
    grid_h, grid_w = math.ceil(rh / P), math.ceil(rw / P)
    ys = [[y1 + ph * bin_h + (iy + 0.5) * bin_h / grid_h for iy in range(grid_h)] for ph in range(P)]
    xs = [[x1 + pw * bin_w + (ix + 0.5) * bin_w / grid_w for ix in range(grid_w)] for pw in range(P)]
    return ys, xs, max(grid_h * grid_w, 1)


def _roi_corner(v, n):
    """bilinear_interpolate of one axis: v already inside [-1, n] -> (low, high, weight of low, weight of high)"""
    v = max(v, 0.0)
    lo = int(v)
    if lo >= n - 1:
        lo = hi = n - 1
        v = float(lo)
    else:
        hi = lo + 1
    l = v - lo
    return lo, hi, 1.0 - l, l


def roi_align_ref(feat, rois, spatial_scale, P=7):
    """feat (B,C,H,W) fp64 (may require grad), rois (K,5) -> (K,C,P,P) fp64: the literal per-sample loop."""
    B, C, H, W = feat.shape
    flat = feat.permute(0, 2, 3, 1).reshape(B * H * W, C)
    rows = []
    for r in rois.detach().double().cpu().tolist():
        idx, wts, dst = [], [], []
        b = int(r[0])
        ys, xs, count = roi_samples(r[1:], spatial_scale, H, W, P)
        for ph in range(P):
            for pw in range(P):
                for y in ys[ph]:
                    for x in xs[pw]:
                        if y < -1.0 or y > H or x < -1.0 or x > W:
                            continue
                        yl, yh, hy, ly = _roi_corner(y, H)
                        xl, xh, hx, lx = _roi_corner(x, W)
                        for yy, xx, w in ((yl, xl, hy * hx), (yl, xh, hy * lx), (yh, xl, ly * hx), (yh, xh, ly * lx)):
                            idx.append((b * H + yy) * W + xx)
                            wts.append(w / count)
                            dst.append(ph * P + pw)
        row = torch.zeros(P * P, C, dtype=feat.dtype)
        if idx:
            vals = flat[torch.tensor(idx)] * torch.tensor(wts, dtype=feat.dtype)[:, None]
            row = row.index_add(0, torch.tensor(dst), vals)
        rows.append(row.t().reshape(C, P, P))
    return torch.stack(rows) if rows else feat.new_zeros(0, C, P, P)


def roi_extract_ref(feats, rois, strides, finest_scale=56, levels=None, P=7):
    """SingleRoIExtractor.forward on fp64 NCHW maps -> (K,C,P,P) fp64; `levels`: the level of every box instead of
    roi_level_ref's (tests force a wrong one)."""
    L = len(strides)
    lv = roi_level_ref(rois, L, finest_scale) if levels is None else levels
    if L == 1 and levels is None:
        lv = torch.zeros_like(lv)
    K, C = rois.shape[0], feats[0].shape[1]
    out = feats[0].new_zeros(K, C, P, P)
    for l in range(L):
        sel = torch.nonzero(lv == l)[:, 0]
        if sel.numel():
            ss = float(torch.tensor(1.0 / strides[l], dtype=torch.float32))
            out = out.index_add(0, sel, roi_align_ref(feats[l], rois[sel], ss, P))
    return out


# ----------------------------------------------------------------------------- RPNHead.get_bboxes restatement
# The oracle of hrfuser_amd.rpn / csrc/hrf_rpn.h (no mmcv here: parity against real mmcv nms is unpinned): a
# literal fp32 torch restatement of rpn_head.py:103-235 with anchor_generator.py:151-194 / 241-281, delta_xywh_bbox_coder.py:
# 164-260 and mmcv 1.3.17 nms (offset 0), every stage callable on its own.  Where the reference leaves the result open or
# non-finite the restatement fixes it as the header states: equal scores go to the lower index (a stable sort), a NaN logit
# ranks last and its candidate is invalid, levels are separate NMS problems (no coordinate offset).
def rpn_base_anchors(base_size, scales, ratios, center_offset=0.0):
    """gen_single_level_base_anchors (anchor_generator.py:151-194, scale_major) -> (len(ratios) * len(scales), 4) fp32"""
    scales, ratios = torch.tensor(scales, dtype=torch.float32), torch.tensor(ratios, dtype=torch.float32)
    w = h = base_size
    xc, yc = center_offset * w, center_offset * h
    h_ratios = torch.sqrt(ratios)
    w_ratios = 1 / h_ratios
    ws = (w * w_ratios[:, None] * scales[None, :]).view(-1)
    hs = (h * h_ratios[:, None] * scales[None, :]).view(-1)
    return torch.stack([xc - 0.5 * ws, yc - 0.5 * hs, xc + 0.5 * ws, yc + 0.5 * hs], dim=-1)


def rpn_grid_anchors(base, H, W, stride):
    """single_level_grid_priors (anchor_generator.py:241-281) -> (H * W * A, 4) fp32, row (y * W + x) * A + a"""
    sx = torch.arange(0, W).to(torch.float32) * stride
    sy = torch.arange(0, H).to(torch.float32) * stride
    xx, yy = sx.repeat(H), sy.view(-1, 1).repeat(1, W).view(-1)
    shifts = torch.stack([xx, yy, xx, yy], dim=-1)
    return (base[None, :, :] + shifts[:, None, :]).view(-1, 4)


def rpn_delta2bbox(rois, deltas, max_shape=None, wh_ratio_clip=16 / 1000):
    """delta2bbox (delta_xywh_bbox_coder.py:224-260) with means 0, stds 1, clip_border -> (N, 4), the dtype of the inputs"""
    import math
    dxy, dwh = deltas[:, :2], deltas[:, 2:]
    pxy = (rois[:, :2] + rois[:, 2:]) * 0.5
    pwh = rois[:, 2:] - rois[:, :2]
    dxy_wh = pwh * dxy
    max_ratio = abs(math.log(wh_ratio_clip))
    dwh = dwh.clamp(min=-max_ratio, max=max_ratio)
    gxy = pxy + dxy_wh
    gwh = pwh * dwh.exp()
    boxes = torch.cat([gxy - gwh * 0.5, gxy + gwh * 0.5], dim=-1)
    if max_shape is not None:
        boxes[:, 0::2].clamp_(min=0, max=float(max_shape[1]))
        boxes[:, 1::2].clamp_(min=0, max=float(max_shape[0]))
    return boxes


def rpn_rank(logits, k, by='logit'):
    """the k first indices of a stable descending sort of the flat logits (by='sigmoid': of their fp32 sigmoid, what the
    reference sorts); NaN last"""
    v = logits if by == 'logit' else logits.sigmoid()
    nan = torch.isnan(v)
    order = torch.argsort(torch.where(nan, torch.full_like(v, float('-inf')), v), descending=True, stable=True)
    order = torch.cat([order[~nan[order]], order[nan[order]]])
    return order[:k]


def rpn_stage1_ref(cls_scores, bbox_preds, img_shapes, strides, bases, nms_pre, min_bbox_size=0.0, by='logit'):
    """cls_scores[l] (B,A,H,W), bbox_preds[l] (B,4A,H,W) fp32 CPU, img_shapes [(h, w)], bases[l] (A,4) ->
    out[b][l] = dict(idx (k,) int64, cand (k,5) = box + logit, valid (k,) bool): rpn_head.py:150-187 + :217-228"""
    out = []
    for b in range(cls_scores[0].shape[0]):
        levels = []
        for l, (cs, bp) in enumerate(zip(cls_scores, bbox_preds)):
            H, W = cs.shape[-2:]
            logit = cs[b].float().permute(1, 2, 0).reshape(-1)
            deltas = bp[b].float().permute(1, 2, 0).reshape(-1, 4)
            idx = rpn_rank(logit, min(nms_pre, logit.numel()), by)
            anchors = rpn_grid_anchors(bases[l], H, W, strides[l])[idx]
            boxes = rpn_delta2bbox(anchors, deltas[idx], max_shape=img_shapes[b])
            w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
            valid = (w > min_bbox_size) & (h > min_bbox_size) & ~torch.isnan(logit[idx])
            levels.append(dict(idx=idx, cand=torch.cat([boxes, logit[idx, None]], dim=1), valid=valid))
        out.append(levels)
    return out


def nms_iou(boxes):
    """pairwise IoU (n, n) in the dtype of `boxes`, in the order mmcv's kernel writes it (offset 0)"""
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    area = (x2 - x1) * (y2 - y1)
    iw = (torch.min(x2[:, None], x2[None, :]) - torch.max(x1[:, None], x1[None, :])).clamp(min=0)
    ih = (torch.min(y2[:, None], y2[None, :]) - torch.max(y1[:, None], y1[None, :])).clamp(min=0)
    inter = iw * ih
    return inter / (area[:, None] + area[None, :] - inter)


def nms_greedy_ref(boxes, valid, thr):
    """greedy NMS in row order on fp32 boxes -> keep (n,) bool; invalid rows are never kept and suppress nothing"""
    n = boxes.shape[0]
    keep = torch.zeros(n, dtype=torch.bool)
    if n == 0:
        return keep
    over = nms_iou(boxes.float()) > thr
    dead = ~valid.clone() if valid is not None else torch.zeros(n, dtype=torch.bool)
    for i in range(n):
        if dead[i]:
            continue
        keep[i] = True
        dead[i + 1:] |= over[i, i + 1:]
    return keep


def nms_segments_ref(segs, thr, max_per_img, sigmoid=True):
    """segs = [dict(cand (n,5), valid (n,) or None)] of ONE image, each in descending score order -> (dets (m,5) fp32,
    src (m,2) int64 = (segment, row) of every output row): per-segment greedy NMS, then a stable descending sort of the kept
    scores over the concatenation (ties: lower segment, lower row), [:max_per_img]"""
    rows, src = [], []
    for s, sg in enumerate(segs):
        keep = nms_greedy_ref(sg['cand'][:, :4], sg.get('valid'), thr)
        sel = torch.nonzero(keep)[:, 0]
        rows.append(sg['cand'][sel])
        src.append(torch.stack([torch.full_like(sel, s), sel], dim=1))
    rows, src = torch.cat(rows), torch.cat(src)
    order = torch.argsort(rows[:, 4], descending=True, stable=True)[:max_per_img]
    dets = rows[order].clone()
    if sigmoid:
        dets[:, 4] = dets[:, 4].sigmoid()
    return dets, src[order]


def rpn_proposals_ref(cls_scores, bbox_preds, img_shapes, strides, bases, nms_pre, max_per_img, iou_thr=0.7, min_bbox_size=0.0):
    """RPNHead.get_bboxes -> [(n_b, 5)] per image: (x1, y1, x2, y2, score)"""
    st1 = rpn_stage1_ref(cls_scores, bbox_preds, img_shapes, strides, bases, nms_pre, min_bbox_size)
    return [nms_segments_ref(levels, iou_thr, max_per_img)[0] for levels in st1]


# ----------------------------------------------------------------------------- CascadeRoIHead.simple_test restatement
# The oracle of hrfuser_amd.roi_head / csrc/hrf_bbox.h / csrc/hrf_fc.h: a literal torch restatement of cascade_roi_head.py:288-400,
# bbox_head.py:316-378 / :460-497, convfc_bbox_head.py (Shared2FCBBoxHead.forward), bbox_nms.py:8-95 and delta_xywh_bbox_coder.py:
# 224-260 with mmcv 1.3.17 nms (offset 0) per class.  Where the reference leaves the result open the header's rule is taken: equal
# scores go to the lower class, then the lower roi row; a NaN score is invalid; classes are separate NMS problems.
def bbox_delta2bbox(rois, deltas, stds=(1., 1., 1., 1.), max_shape=None, wh_ratio_clip=16 / 1000):
    """delta2bbox (delta_xywh_bbox_coder.py:224-260) with means 0: `deltas * stds` first, then rpn_delta2bbox's order"""
    return rpn_delta2bbox(rois, deltas * deltas.new_tensor(stds).view(1, -1), max_shape=max_shape, wh_ratio_clip=wh_ratio_clip)


def bbox_head_ref(x, sd, prefix=''):
    """Shared2FCBBoxHead.forward (convfc_bbox_head.py:155-191) in the dtype of `x` (K,C,7,7) with mmdet's state-dict keys ->
    (cls_score (K, num_classes + 1), bbox_pred (K, 4))"""
    import torch.nn.functional as F
    p = lambda k: sd[prefix + k].to(x.dtype)                            # noqa: E731
    h = x.flatten(1)
    for i in (0, 1):
        h = F.relu(F.linear(h, p(f'shared_fcs.{i}.weight'), p(f'shared_fcs.{i}.bias')))
    return F.linear(h, p('fc_cls.weight'), p('fc_cls.bias')), F.linear(h, p('fc_reg.weight'), p('fc_reg.bias'))


def multiclass_nms_ref(boxes, scores, score_thr, iou_thr, max_per_img, row_valid=None):
    """multiclass_nms (bbox_nms.py:8-95) of ONE image with class-agnostic boxes (n,4) and scores (n, num_classes + 1) fp32 ->
    (dets (m,5), labels (m,) int64, src (m,) int64 = the roi row of every output row).  Per class: candidates in descending score
    order (stable: lower row first), valid = score > score_thr (NaN fails) and row_valid, greedy NMS on nms_greedy_ref; the kept
    rows of all classes in a stable descending sort by score (ties: lower class, then lower row), [:max_per_img]"""
    n, C = scores.shape[0], scores.shape[1] - 1
    rows, labels, src = [], [], []
    for c in range(C):
        s = scores[:, c]
        nan = torch.isnan(s)
        order = torch.argsort(torch.where(nan, torch.full_like(s, float('-inf')), s), descending=True, stable=True)
        order = torch.cat([order[~nan[order]], order[nan[order]]])
        valid = s[order] > score_thr
        if row_valid is not None:
            valid = valid & row_valid[order]
        keep = nms_greedy_ref(boxes[order], valid, iou_thr)
        sel = order[keep]
        rows.append(torch.cat([boxes[sel], s[sel, None]], dim=1))
        labels.append(torch.full_like(sel, c))
        src.append(sel)
    rows, labels, src = torch.cat(rows), torch.cat(labels), torch.cat(src)
    order = torch.argsort(rows[:, 4], descending=True, stable=True)[:max_per_img]
    return rows[order], labels[order], src[order]


def bbox_detect_ref(rois, logits, deltas, stds, img_shapes, counts, score_thr, iou_thr, max_per_img, scale_factors=None):
    """the last stage's get_bboxes (bbox_head.py:316-378) on fixed-shape inputs: rois (B*R,5), logits = [(B*R, C+1)] per stage,
    deltas (B*R,4), counts [n_b] (rows >= n_b of image b are invalid) -> [(dets, labels, src)] per image"""
    B = len(img_shapes)
    R = rois.shape[0] // B
    mean = sum(logits) / float(len(logits))
    out = []
    for b in range(B):
        sl = slice(b * R, (b + 1) * R)
        scores = torch.softmax(mean[sl], dim=-1)
        boxes = bbox_delta2bbox(rois[sl, 1:], deltas[sl], stds, max_shape=img_shapes[b])
        if scale_factors is not None:
            boxes = boxes / boxes.new_tensor(scale_factors[b])
        out.append(multiclass_nms_ref(boxes, scores, score_thr, iou_thr, max_per_img, torch.arange(R) < int(counts[b])))
    return out


def cascade_simple_test_ref(feats, rois, counts, img_shapes, sds, stds_per_stage, strides, score_thr, iou_thr, max_per_img,
                            scale_factors=None, finest_scale=56, dtype=torch.float32):
    """CascadeRoIHead.simple_test (cascade_roi_head.py:288-400) on fixed-shape rois (B*R,5) with counts [n_b]: per stage
    roi_extract_ref -> bbox_head_ref -> regress_by_class (class-agnostic), then bbox_detect_ref on the stage-averaged logits.
    feats: NCHW maps; sds: one mmdet state dict per stage.  RoI features and the head run in `dtype`, the box arithmetic in fp32.
    -> ([(dets, labels, src)] per image, per-stage list of the rois that entered the stage)"""
    B = len(img_shapes)
    R = rois.shape[0] // B
    rois = rois.float().clone()
    logits, stage_rois, deltas = [], [], None
    for i, sd in enumerate(sds):
        stage_rois.append(rois.clone())
        x = roi_extract_ref([f.to(dtype) for f in feats], rois.to(dtype), strides, finest_scale)
        cls, deltas = bbox_head_ref(x, sd)
        cls, deltas = cls.float(), deltas.float()
        logits.append(cls)
        if i < len(sds) - 1:
            new = [torch.cat([rois[b * R:(b + 1) * R, :1],
                              bbox_delta2bbox(rois[b * R:(b + 1) * R, 1:], deltas[b * R:(b + 1) * R], stds_per_stage[i], max_shape=img_shapes[b])], dim=1)
                   for b in range(B)]
            rois = torch.cat(new)
    return bbox_detect_ref(rois, logits, deltas, stds_per_stage[-1], img_shapes, counts, score_thr, iou_thr, max_per_img, scale_factors), stage_rois


# ----------------------------------------------------------------------------- RPNHead.loss restatement
# The oracle of hrfuser_amd.rpn.rpn_assign / rpn_loss (csrc/hrf_rpn_train.h; no mmcv / mmdet here: parity against an installed
# mmdet is unpinned): literal torch restatements of anchor_generator.py:392-451 (valid_flags), core/anchor/
# utils.py:21-47 (anchor_inside_flags), iou2d_calculator.py:213-253 (bbox_overlaps), max_iou_assigner.py:128-213
# (assign_wrt_overlaps), base_sampler.py:83-98 / random_sampler.py:64-82 with the random choice replaced by "the k smallest
# (key, index)", anchor_head.py:253-283 / :383-384 / :402-450 and delta_xywh_bbox_coder.py:118-160 (bbox2delta).  Everything runs
# in the dtype of its inputs: fp32 is the reference's arithmetic, fp64 (rpn_loss_ref(dtype=torch.float64)) the yardstick of it.
def rpn_inside_flags_ref(anchors, H, W, A, stride, img_shape, pad_shape, allowed_border=0):
    """valid_flags (valid_h = min(ceil(pad_h / stride), H)) and anchor_inside_flags of ONE level -> (H * W * A,) bool"""
    import math
    vh, vw = min(int(math.ceil(pad_shape[0] / stride)), H), min(int(math.ceil(pad_shape[1] / stride)), W)
    vy, vx = torch.arange(H) < vh, torch.arange(W) < vw
    valid = (vy[:, None] & vx[None, :]).reshape(-1)[:, None].expand(H * W, A).reshape(-1)
    if allowed_border >= 0:
        img_h, img_w = img_shape[:2]
        return valid & (anchors[:, 0] >= -allowed_border) & (anchors[:, 1] >= -allowed_border) & \
            (anchors[:, 2] < img_w + allowed_border) & (anchors[:, 3] < img_h + allowed_border)
    return valid


def bbox_overlaps_ref(gts, anchors, eps=1e-6):
    """bbox_overlaps(gts (G,4), anchors (N,4), mode='iou') -> (G, N) in the dtype of the inputs, in the written order"""
    area1 = (gts[:, 2] - gts[:, 0]) * (gts[:, 3] - gts[:, 1])
    area2 = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    lt = torch.max(gts[:, None, :2], anchors[None, :, :2])
    rb = torch.min(gts[:, None, 2:], anchors[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2[None, :] - overlap
    union = torch.max(union, union.new_tensor([eps]))
    return overlap / union


def max_iou_assign_ref(overlaps, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True):
    """MaxIoUAssigner.assign_wrt_overlaps (gt_max_assign_all) on overlaps (G, N) -> (assigned (N,) int64: -1 / 0 / i + 1,
    max_overlaps (N,))"""
    G, N = overlaps.shape
    assigned = torch.full((N,), -1, dtype=torch.long, device=overlaps.device)
    if G == 0 or N == 0:
        if G == 0:
            assigned[:] = 0
        return assigned, overlaps.new_zeros((N,))
    max_overlaps, argmax_overlaps = overlaps.max(dim=0)
    gt_max_overlaps, _ = overlaps.max(dim=1)
    assigned[(max_overlaps >= 0) & (max_overlaps < neg_iou_thr)] = 0
    pos = max_overlaps >= pos_iou_thr
    assigned[pos] = argmax_overlaps[pos] + 1
    if match_low_quality:
        for i in range(G):
            if gt_max_overlaps[i] >= min_pos_iou:
                assigned[overlaps[i, :] == gt_max_overlaps[i]] = i + 1
    return assigned, max_overlaps


def rpn_assign_ref(sizes, strides, bases, img_shape, pad_shape, gts, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True,
                   allowed_border=0):
    """ONE image: the anchors of all levels (sizes [(H, W)], bases[l] (A,4)), the inside flags, the assignment of the inside
    anchors -> (assigned (N,) int64 with -2 where not inside, max_iou (N,) fp32 with 0 there, anchors (N,4), inside (N,) bool)"""
    anchors = torch.cat([rpn_grid_anchors(bases[l], H, W, strides[l]) for l, (H, W) in enumerate(sizes)])
    inside = torch.cat([rpn_inside_flags_ref(rpn_grid_anchors(bases[l], H, W, strides[l]), H, W, bases[l].shape[0], strides[l], img_shape,
                                             pad_shape, allowed_border) for l, (H, W) in enumerate(sizes)])
    a, m = max_iou_assign_ref(bbox_overlaps_ref(gts.float().reshape(-1, 4), anchors[inside]), pos_iou_thr, neg_iou_thr, min_pos_iou,
                              match_low_quality)
    assigned = torch.full((anchors.shape[0],), -2, dtype=torch.long)
    max_iou = torch.zeros(anchors.shape[0], dtype=torch.float32)
    assigned[inside], max_iou[inside] = a, m
    return assigned, max_iou, anchors, inside


def rpn_key_ref(seed, counter, b, N):
    """the generated sampling keys of image b (csrc/hrf_rpn_train.h: rpnt_hash) -> (N,) int64 holding uint32 values:
    mix(h) = h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16 (mod 2^32);
    key = mix(mix(mix(mix(seed + 0x9e3779b9) ^ counter) + b) ^ n)"""
    M = 0xffffffff

    def mix(h):
        h = h ^ (h >> 16)
        h = (h * 0x7feb352d) & M
        h = h ^ (h >> 15)
        h = (h * 0x846ca68b) & M                                    # (an int64 product may wrap: its low 32 bits do not change)
        return h ^ (h >> 16)
    h = torch.tensor([(int(seed) + 0x9e3779b9) & M], dtype=torch.long)
    h = mix(h) ^ (int(counter) & M)
    h = (mix(h) + int(b)) & M
    return mix(mix(h) ^ torch.arange(N, dtype=torch.long))


def rpn_sample_ref(assigned, keys, num, num_pos):
    """RandomSampler on ONE image with the random choice spelled out: assigned (N,) int64, keys (N,) int64 (uint32 values),
    num_pos = int(num * pos_fraction) -> sampled (N,) int64: +1 / -1 / 0.  num_pos' = min(P, num_pos) positives and
    min(Q, num - num_pos') negatives, each the members of smallest (key, index)"""
    sampled = torch.zeros_like(assigned)
    pos, neg = torch.nonzero(assigned > 0)[:, 0], torch.nonzero(assigned == 0)[:, 0]
    npos = min(pos.numel(), int(num_pos))
    nneg = min(neg.numel(), int(num) - npos)
    for members, k, tag in ((pos, npos, 1), (neg, nneg, -1)):
        order = torch.argsort(keys[members], stable=True)           # (members ascend: equal keys go to the lower index)
        sampled[members[order[:k]]] = tag
    return sampled


def rpn_bbox2delta_ref(proposals, gt):
    """bbox2delta (delta_xywh_bbox_coder.py:118-160), means 0, stds 1, in the dtype of the inputs"""
    px, py = (proposals[..., 0] + proposals[..., 2]) * 0.5, (proposals[..., 1] + proposals[..., 3]) * 0.5
    pw, ph = proposals[..., 2] - proposals[..., 0], proposals[..., 3] - proposals[..., 1]
    gx, gy = (gt[..., 0] + gt[..., 2]) * 0.5, (gt[..., 1] + gt[..., 3]) * 0.5
    gw, gh = gt[..., 2] - gt[..., 0], gt[..., 3] - gt[..., 1]
    return torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph)], dim=-1)


def rpn_loss_ref(cls_scores, bbox_preds, anchors, assigned, sampled, gts, beta=1.0 / 9.0, loss_weight_cls=1.0, loss_weight_bbox=1.0,
                 dtype=torch.float32):
    """anchor_head.py:253-283 (targets) + :383-384 (avg) + :402-450 (loss_single) per level, rpn_head.py:70-101.
    cls_scores[l] (B,A,H,W), bbox_preds[l] (B,4A,H,W); anchors (N,4) fp32; assigned / sampled: per image (N,) int64 over the
    concatenated levels; gts: per image (G_b,4).  Computed in `dtype` from the fp32 inputs ->
    (loss_cls [L], loss_bbox [L], d loss_cls_l / d cls_scores[l] [L], d loss_bbox_l / d bbox_preds[l] [L], smooth-L1 arm counts
    (quadratic, linear))"""
    import torch.nn.functional as F
    B = cls_scores[0].shape[0]
    avg = float(sum(max(int((s > 0).sum()), 1) + max(int((s < 0).sum()), 1) for s in sampled))
    an = anchors.to(dtype)
    labels_t, weights, targets, bweights = [], [], [], []
    for b in range(B):
        pos = sampled[b] > 0
        tg = torch.zeros(an.shape, dtype=dtype, device=an.device)
        if bool(pos.any()):
            tg[pos] = rpn_bbox2delta_ref(an[pos], gts[b].to(dtype)[assigned[b][pos] - 1])
        labels_t.append(pos.to(dtype))                              # label 0 (foreground) -> one-hot 1, background -> 0
        weights.append((sampled[b] != 0).to(dtype))
        targets.append(tg)
        bweights.append(pos.to(dtype)[:, None].expand(-1, 4))
    labels_t, weights, targets, bweights = (torch.stack(t) for t in (labels_t, weights, targets, bweights))
    out_c, out_b, g_c, g_b, arms, off = [], [], [], [], [0, 0], 0
    for cs, bp in zip(cls_scores, bbox_preds):
        cs, bp = cs.detach().to(dtype).requires_grad_(True), bp.detach().to(dtype).requires_grad_(True)
        n = cs.shape[1] * cs.shape[2] * cs.shape[3]
        sl = slice(off, off + n)
        x = cs.permute(0, 2, 3, 1).reshape(B, n)
        loss_cls = (F.binary_cross_entropy_with_logits(x, labels_t[:, sl], reduction='none') * weights[:, sl]).sum() / avg * loss_weight_cls
        d = bp.permute(0, 2, 3, 1).reshape(B, n, 4)
        diff = (d - targets[:, sl]).abs()
        l1 = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
        loss_bbox = (l1 * bweights[:, sl]).sum() / avg * loss_weight_bbox
        on = bweights[:, sl] > 0
        arms[0] += int(((diff < beta) & on).sum())
        arms[1] += int((~(diff < beta) & on).sum())
        g_c.append(torch.autograd.grad(loss_cls, cs)[0])
        g_b.append(torch.autograd.grad(loss_bbox, bp)[0])
        out_c.append(loss_cls.detach())
        out_b.append(loss_bbox.detach())
        off += n
    return out_c, out_b, g_c, g_b, tuple(arms)


# ----------------------------------------------------------------------------- CascadeRoIHead.forward_train restatement
# The oracle of hrfuser_amd.roi_head.bbox_targets / bbox_loss / CascadeRoIHead.losses (csrc/hrf_bbox_train.h; no mmcv / mmdet here:
# parity against an installed mmdet is unpinned): literal torch restatements of max_iou_assigner.py:84-213 with
# match_low_quality False, assign_result.py:196-206 (add_gt_), base_sampler.py:68-102 (the gts in FRONT of the proposals) +
# random_sampler.py:64-82 with the random choice replaced by "the k smallest (key, index)", sampling_result.py (bboxes = cat(pos,
# neg), positives and negatives each in ascending index), bbox_head.py:122-255 (get_targets) / :257-313 (loss) and
# cascade_roi_head.py:191-286.  Candidates are in mmdet's compact order: the G gts (when added), then the proposals.  Everything
# runs in `dtype` from fp32 inputs: fp32 is the reference's arithmetic, fp64 the yardstick of it.
def _mix32(h):
    M = 0xffffffff
    h &= M
    h ^= h >> 16
    h = (h * 0x7feb352d) & M
    h ^= h >> 15
    h = (h * 0x846ca68b) & M
    return h ^ (h >> 16)


def rcnn_key_ref(seed, counter, stage, b, N):
    """the generated sampling keys of image b in stage `stage` over the N = Gmax + R candidate slots (csrc/hrf_bbox_train.h):
    the RPN's hash with the stage folded into the seed, rpn_key_ref(seed ^ mix(0x5bd1e995 + stage), counter, b, N)"""
    return rpn_key_ref((int(seed) & 0xffffffff) ^ _mix32(0x5bd1e995 + int(stage)), counter, b, N)


def rcnn_assign_ref(proposals, gts, pos_iou_thr, neg_iou_thr, add_gt_as_proposals=True, dtype=torch.float32):
    """MaxIoUAssigner(match_low_quality=False).assign on ONE image's proposals (n,4) and gts (G,4), then add_gt_ ->
    (assigned (G + n,) int64: -1 / 0 / i + 1, max_iou (G + n,), boxes (G + n, 4)); without add_gt_as_proposals the G leading
    entries are absent.  A NaN IoU makes the column's maximum NaN (torch.max), which fails every comparison: -1."""
    p, g = proposals.reshape(-1, 4).to(dtype), gts.reshape(-1, 4).to(dtype)
    assigned, mx = max_iou_assign_ref(bbox_overlaps_ref(g, p), pos_iou_thr, neg_iou_thr, 0.0, False)
    if not add_gt_as_proposals:
        return assigned, mx, p
    G = g.shape[0]
    return torch.cat([torch.arange(1, G + 1, dtype=torch.long, device=assigned.device), assigned]), torch.cat([mx.new_ones(G), mx]), torch.cat([g, p])


def rcnn_sample_ref(assigned, keys, num, num_pos):
    """RandomSampler (neg_pos_ub -1) on ONE image given keys (one per candidate, uint32 values in int64) -> (pos_inds, neg_inds),
    each ascending: the min(P, num_pos) positives and the min(Q, num - that) negatives of smallest (key, index)"""
    s = rpn_sample_ref(assigned, keys, num, num_pos)
    return torch.nonzero(s > 0)[:, 0], torch.nonzero(s < 0)[:, 0]


def bbox_targets_ref(boxes, assigned, pos_inds, neg_inds, gts, gt_labels, num_classes, stds, dtype=torch.float32):
    """bbox_head.py:122-185 (_get_target_single, pos_weight <= 0) on ONE image -> (rows (n,4) = cat(pos boxes, neg boxes),
    labels (n,) int64, bbox_targets (n,4)): bbox2delta(pos box, its gt) / stds on the positives, zero on the negatives"""
    bx, g = boxes.to(dtype), gts.reshape(-1, 4).to(dtype)
    rows = torch.cat([bx[pos_inds], bx[neg_inds]])
    labels = torch.full((rows.shape[0],), int(num_classes), dtype=torch.long, device=rows.device)
    targets = torch.zeros((rows.shape[0], 4), dtype=dtype, device=rows.device)
    npos = pos_inds.numel()
    if npos:
        m = assigned[pos_inds] - 1
        labels[:npos] = gt_labels.long()[m]
        targets[:npos] = rpn_bbox2delta_ref(bx[pos_inds], g[m]) / targets.new_tensor([float(s) for s in stds])
    return rows, labels, targets


def bbox_loss_ref(logits, deltas, labels, targets, num_classes, beta=1.0, loss_weight_cls=1.0, loss_weight_bbox=1.0, dtype=torch.float32):
    """bbox_head.py:257-313 on the rows of the whole batch (labels in [0, num_classes]; label weights 1): F.cross_entropy summed /
    max(n, 1), SmoothL1 on the positives summed / n (avg_factor = bbox_targets.size(0)), accuracy top-1 ->
    dict(loss_cls, loss_bbox, acc, correct, d_logits, d_deltas, arms = SmoothL1 (quadratic, linear) counts)"""
    import torch.nn.functional as F
    x, d = logits.detach().to(dtype).requires_grad_(True), deltas.detach().to(dtype).requires_grad_(True)
    n = int(labels.numel())
    t = targets.to(dtype)
    if n == 0:
        z = torch.zeros((), dtype=dtype)
        return dict(loss_cls=z, loss_bbox=z, acc=z, correct=0, d_logits=torch.zeros_like(x), d_deltas=torch.zeros_like(d), arms=(0, 0))
    loss_cls = F.cross_entropy(x, labels.long(), reduction='none').sum() / float(max(n, 1)) * loss_weight_cls
    pos = (labels >= 0) & (labels < num_classes)
    diff = (d[pos] - t[pos]).abs()
    l1 = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
    loss_bbox = l1.sum() / float(n) * loss_weight_bbox
    correct = int((x.detach().argmax(dim=1) == labels).sum())
    g_x = torch.autograd.grad(loss_cls, x)[0]
    g_d = torch.autograd.grad(loss_bbox, d)[0] if bool(pos.any()) else torch.zeros_like(d)
    return dict(loss_cls=loss_cls.detach(), loss_bbox=loss_bbox.detach(), acc=torch.tensor(100.0 * correct / n, dtype=dtype), correct=correct,
                d_logits=g_x, d_deltas=g_d, arms=(int((diff < beta).sum()), int((~(diff < beta)).sum())))


def cascade_forward_train_ref(feats, proposals, gts, gt_labels, img_shapes, sds, stage_cfgs, stds_per_stage, num_classes, strides, key_fn,
                              finest_scale=56, dtype=torch.float32):
    """CascadeRoIHead.forward_train (cascade_roi_head.py:191-286), bbox branch, class-agnostic regression.  feats: NCHW maps;
    proposals [(n_b,4)], gts [(G_b,4)], gt_labels [(G_b,)] per image; sds: one mmdet state dict per stage; stage_cfgs: per stage
    dict(pos_iou_thr, neg_iou_thr, num, num_pos, add_gt_as_proposals, beta, loss_weight_cls, loss_weight_bbox, stage_weight);
    key_fn(stage, b, is_gt (m,) bool, index (m,) int64) -> (m,) int64 keys of the candidates (index: the gt number or the
    proposal's position in the stage's list).  RoI features and the head run in `dtype`, the box arithmetic in fp32 ->
    (losses: mmdet's dict s{i}.loss_cls / s{i}.acc / s{i}.loss_bbox, per-stage records dict(proposals, rois, labels, targets,
    pos_is_gt, logits, deltas))"""
    B = len(proposals)
    props = [p.float().reshape(-1, 4) for p in proposals]
    losses, records = {}, []
    for i, (sd, sc) in enumerate(zip(sds, stage_cfgs)):
        rows, labels, targets, is_gt = [], [], [], []
        for b in range(B):
            add = bool(sc.get('add_gt_as_proposals', True))
            assigned, _, boxes = rcnn_assign_ref(props[b], gts[b], sc['pos_iou_thr'], sc['neg_iou_thr'], add)
            G = gts[b].reshape(-1, 4).shape[0] if add else 0
            m = boxes.shape[0]
            gt_flag = torch.arange(m) < G
            keys = key_fn(i, b, gt_flag, torch.where(gt_flag, torch.arange(m), torch.arange(m) - G))
            pos, neg = rcnn_sample_ref(assigned, keys, sc['num'], sc['num_pos'])
            r, l, t = bbox_targets_ref(boxes, assigned, pos, neg, gts[b], gt_labels[b], num_classes, stds_per_stage[i])
            rows.append(torch.cat([torch.full((r.shape[0], 1), float(b)), r], dim=1))
            labels.append(l)
            targets.append(t)
            is_gt.append(torch.cat([gt_flag[pos], torch.zeros(neg.numel(), dtype=torch.bool)]))
        rois = torch.cat(rows)
        x = roi_extract_ref([f.to(dtype) for f in feats], rois.to(dtype), strides, finest_scale)
        cls, deltas = bbox_head_ref(x, sd)
        w = float(sc.get('stage_weight', 1.0))
        lr = bbox_loss_ref(cls.float(), deltas.float(), torch.cat(labels), torch.cat(targets), num_classes, sc.get('beta', 1.0),
                           sc.get('loss_weight_cls', 1.0) * w, sc.get('loss_weight_bbox', 1.0) * w, dtype)
        losses[f's{i}.loss_cls'], losses[f's{i}.acc'], losses[f's{i}.loss_bbox'] = lr['loss_cls'], lr['acc'], lr['loss_bbox']
        records.append(dict(proposals=[p.clone() for p in props], rois=rois, labels=torch.cat(labels), targets=torch.cat(targets),
                            pos_is_gt=is_gt, logits=cls.float(), deltas=deltas.float()))
        if i < len(sds) - 1:                                        # refine_bboxes: regress every sampled row, drop the sampled gts
            off, new = 0, []
            for b in range(B):
                n = rows[b].shape[0]
                bx = bbox_delta2bbox(rois[off:off + n, 1:], deltas.float()[off:off + n], stds_per_stage[i], max_shape=img_shapes[b])
                keep = torch.ones(n, dtype=torch.bool)
                keep[:n] = ~is_gt[b]
                new.append(bx[keep])
                off += n
            props = new
    return losses, records
