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
