"""RPN proposal generation (csrc/hrf_rpn.h: hrf_rpn_select_decode / hrf_nms_segments / hrf_rpn_proposals; hrfuser_amd/rpn.py:
RPNHead) against the literal fp32 torch restatement of RPNHead.get_bboxes (hrfuser_amd.testing.rpn_proposals_ref and its
stages), through the C ABI on the CPU emulator and on the GPU.  mmcv is not installed: parity against real mmcv nms is unpinned
(INTEGRATION.md); the restatement's anchors and decode are pinned against the reference's docstring examples here.

Small case: B = 2, images 64 x 96 and 60 x 90 (both on the 64 x 96 pyramid 16x24, 8x12, 4x6, 2x3, 1x2, A = 3: 1152 / 288 / 72 /
18 / 6 anchors), nms_pre 200 (two levels select, three take all), max_per_img 300; once more with row pitches larger than the
rows and NaN in the padding.  Full-width case: 128 x 192 / 120 x 180, level 0 = 32 x 48 (4608 anchors), nms_pre 2000: the radix
select, the 2048-entry sort and a full suppression matrix.  Logits ~ N(0, 1), deltas ~ N(0, 0.1): neighbouring anchors overlap
above 0.7, suppression is the common case.  The seeds are the first of 0, 1, 2, ... whose restatement candidates are unambiguous
(distinct fp32 sigmoids of the selected logits per image, no fp64 IoU within 1e-5 of the threshold): test_inputs_unambiguous.

Bounds.  Stage 1: indices, order and valid flags identical; max|box - want| / max(img_h, img_w) < 2e-5, the bound of the sibling
kernel tests - the only operation that is not bit-defined is one expf per side, a wrong anchor / clamp / axis is a pixel or more.
NMS + merge: everything is bit-defined (-ffp-contract=off), so keep set, order, count and the copied box / score bits are
compared EXACTLY; the one exception is the score column of hrf_rpn_proposals, 1 / (1 + expf(-logit)) on the device against
torch.sigmoid: within 1e-6 (the issue's bound for scores), with the source candidate of every output row identical."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import load_cfgs, relmax, use_backend
from hrfuser_amd import _lib
from hrfuser_amd.testing import (nms_greedy_ref, nms_iou, nms_segments_ref, rpn_base_anchors, rpn_delta2bbox, rpn_grid_anchors,
                                 rpn_proposals_ref, rpn_rank, rpn_stage1_ref)

STRIDES = [4, 8, 16, 32, 64]
A, B, THR = 3, 2, 0.7
BASES = [rpn_base_anchors(s, [8], [0.5, 1.0, 2.0]) for s in STRIDES]
BOUND = 2e-5
CASES = {
    # name: (map sizes, image shapes (h, w), nms_pre, max_per_img, committed seed)
    'small': ([(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)], [(64, 96), (60, 90)], 200, 300, 0),
    'full': ([(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)], [(128, 192), (120, 180)], 2000, 1000, 106),
    'hostile': ([(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)], [(64, 96), (60, 90)], 200, 300, 0),
    # stage 1 only: logits rounded to halves (and -0.0 among the zeros) - hundreds of equal logits at every level's cut
    'ties': ([(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)], [(128, 192), (120, 180)], 2000, 1000, 0),
}
RPN_CFG = dict(type='RPNHead', in_channels=256, feat_channels=256,
               anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
               bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0]),
               loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
               loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0))
TEST_CFG = dict(nms_pre=200, max_per_img=300, nms=dict(type='nms', iou_threshold=0.7), min_bbox_size=0)


def _draw(case, seed):
    """-> (cls_scores, bbox_preds): lists of NCHW fp32 maps.  'hostile': 4 % of the logits and of the deltas replaced by NaN / +-Inf"""
    sizes = CASES[case][0]
    g = torch.Generator().manual_seed(seed)
    cs = [torch.randn(B, A, h, w, generator=g) for h, w in sizes]
    bp = [0.1 * torch.randn(B, 4 * A, h, w, generator=g) for h, w in sizes]
    if case == 'ties':
        cs = [torch.round(2 * c) / 2 for c in cs]
        assert any(bool(((c == 0) & torch.signbit(c)).any()) for c in cs)
    if case == 'hostile':
        special = torch.tensor([float('nan'), float('inf'), float('-inf'), float('nan')])
        for t in cs + bp:
            hit = torch.rand(t.shape, generator=g) < 0.04
            pick = special[torch.randint(0, 4, t.shape, generator=g)]
            t[hit] = pick[hit]
    return cs, bp


def _stage1_of(case, seed):
    sizes, shapes, nms_pre, _, _ = CASES[case]
    cs, bp = _draw(case, seed)
    return rpn_stage1_ref(cs, bp, shapes, STRIDES, BASES, nms_pre)


def _pair_iou(a, b):
    """elementwise IoU of box rows a, b (n,4) in their dtype, the order of nms_iou"""
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = (torch.min(a[:, 2], b[:, 2]) - torch.max(a[:, 0], b[:, 0])).clamp(min=0)
    ih = (torch.min(a[:, 3], b[:, 3]) - torch.max(a[:, 1], b[:, 1])).clamp(min=0)
    return iw * ih / (area_a + area_b - iw * ih)


def _scores_distinct(case, seed):
    """the selected logits of an image, within and across levels, have distinct fp32 SIGMOIDS (so distinct logits too): the
    reference's sort by score has no ties, the order by logit is its order (+-Inf and NaN excepted: the header puts them by index)"""
    cs, nms_pre = _draw(case, seed)[0], CASES[case][2]
    for b in range(B):
        sel = []
        for m in cs:
            logit = m[b].permute(1, 2, 0).reshape(-1)
            sel.append(logit[rpn_rank(logit, min(nms_pre, logit.numel()))])
        sg = torch.cat(sel)
        sg = sg[torch.isfinite(sg)].sigmoid()
        if sg.unique().numel() != sg.numel():
            return False
    return True


def _unambiguous(case, seed):
    """_scores_distinct, and no pair of valid candidates of one level with an fp64 IoU within 1e-5 of the threshold (pairs
    pre-selected within 1e-3 in fp32)"""
    if not _scores_distinct(case, seed):
        return False
    for levels in _stage1_of(case, seed):
        for lv in levels:
            boxes = lv['cand'][lv['valid'], :4]
            near = torch.nonzero((nms_iou(boxes) - THR).abs() < 1e-3)
            iou = _pair_iou(boxes[near[:, 0]].double(), boxes[near[:, 1]].double())
            if bool(((iou - THR).abs() < 1e-5).any()):
                return False
    return True


@functools.lru_cache(None)
def _ref(case):
    """-> (cls_scores, bbox_preds, stage 1 of the restatement, [(dets, src)] per image): computed once, never modified"""
    sizes, shapes, nms_pre, max_per, seed = CASES[case]
    cs, bp = _draw(case, seed)
    st1 = rpn_stage1_ref(cs, bp, shapes, STRIDES, BASES, nms_pre)
    return cs, bp, st1, [nms_segments_ref(levels, THR, max_per) for levels in st1]


def _nhwc(case, dev, pitch=False):
    """the maps as the kernels take them: (B,H,W,C) views; pitch: rows of C + 5 / C + 3 floats, NaN in the padding"""
    cs, bp = _ref(case)[:2]
    out = []
    for maps, extra in ((cs, 5), (bp, 3)):
        lst = []
        for m in maps:
            t = m.permute(0, 2, 3, 1).contiguous()
            if pitch:
                big = torch.full(t.shape[:3] + (t.shape[3] + extra,), float('nan'))
                big[..., :t.shape[3]] = t
                t = big.to(dev)[..., :t.shape[3]]
            lst.append(t.to(dev))
        out.append(lst)
    return out


def _shapes_list(case):
    return [tuple(s) for s in CASES[case][1]]


# ----------------------------------------------------------------------------- 1. the restatement, pinned on the CPU
def test_restatement_anchor_docstring():
    """anchor_generator.py:45-56: AnchorGenerator([16], [1.], [1.], [9]).grid_priors([(2, 2)]) (base size 9, stride 16)"""
    base = rpn_base_anchors(9, [1.], [1.])
    want = torch.tensor([[-4.5, -4.5, 4.5, 4.5], [11.5, -4.5, 20.5, 4.5], [-4.5, 11.5, 4.5, 20.5], [11.5, 11.5, 20.5, 20.5]])
    assert torch.equal(rpn_grid_anchors(base, 2, 2, 16), want)
    assert torch.equal(rpn_grid_anchors(rpn_base_anchors(18, [1.], [1.]), 1, 1, 32), torch.tensor([[-9., -9., 9., 9.]]))
    # A = 3: row (y * W + x) * A + a
    g = rpn_grid_anchors(BASES[0], 2, 3, 4)
    assert torch.equal(g[(1 * 3 + 2) * 3 + 1], BASES[0][1] + torch.tensor([8., 4., 8., 4.]))


def test_restatement_delta2bbox_docstring():
    """delta_xywh_bbox_coder.py:210-222"""
    rois = torch.tensor([[0., 0., 1., 1.], [0., 0., 1., 1.], [0., 0., 1., 1.], [5., 5., 5., 5.]])
    deltas = torch.tensor([[0., 0., 0., 0.], [1., 1., 1., 1.], [0., 0., 2., -1.], [0.7, -1.9, -0.5, 0.3]])
    want = torch.tensor([[0.0000, 0.0000, 1.0000, 1.0000], [0.1409, 0.1409, 2.8591, 2.8591], [0.0000, 0.3161, 4.1945, 0.6839],
                         [5.0000, 5.0000, 5.0000, 5.0000]])
    got = rpn_delta2bbox(rois, deltas, max_shape=(32, 32, 3))
    assert float((got - want).abs().max()) < 5e-5                   # (the docstring prints four decimals)


@pytest.mark.parametrize('case', ['small', 'full'])
def test_restatement_sigmoid_order(case):
    """ranking by the fp32 sigmoid (what the reference sorts) = ranking by the logit on the test inputs: the literal reference
    and the restatement agree there"""
    cs = _ref(case)[0]
    nms_pre = CASES[case][2]
    for b in range(B):
        for m in cs:
            logit = m[b].permute(1, 2, 0).reshape(-1)
            k = min(nms_pre, logit.numel())
            a, s = rpn_rank(logit, k, 'logit'), rpn_rank(logit, k, 'sigmoid')
            assert torch.equal(a, s)
            sg = logit[a].sigmoid()
            assert bool((sg[1:] < sg[:-1]).all())                  # strictly: torch.sort's unspecified tie order never matters


# ----------------------------------------------------------------------------- 2. the inputs are unambiguous (CPU)
@pytest.mark.parametrize('case', ['small', 'full', 'hostile'])
def test_inputs_unambiguous(case):
    """the committed seed is the first of 0, 1, 2, ... for which the restatement's own candidates are unambiguous"""
    seed = CASES[case][4]
    first = next(s for s in range(seed + 1) if _unambiguous(case, s))
    assert first == seed, (case, first)


@pytest.mark.parametrize('case', ['small', 'full'])
def test_suppression_is_common(case):
    """the restatement keeps between 10 % and 90 % of the candidates"""
    st1 = _ref(case)[2]
    for levels in st1:
        n = sum(int(lv['valid'].sum()) for lv in levels)
        kept = sum(int(nms_greedy_ref(lv['cand'][:, :4], lv['valid'], THR).sum()) for lv in levels)
        print(f'{case}: {kept} of {n} candidates kept')
        assert 0.1 * n < kept < 0.9 * n, (kept, n)


# ----------------------------------------------------------------------------- 3. stage 1 against the restatement
def _stage1(backend, case, pitch):
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    cm, rm = _nhwc(case, dev, pitch)
    shapes, nms_pre = _shapes_list(case), CASES[case][2]
    cand, valid, idx = rpn.select_decode(cm, rm, shapes, STRIDES, [b.tolist() for b in BASES], nms_pre, 0.0, want_idx=True)
    cand, valid, idx = cand.cpu(), valid.cpu(), idx.cpu()
    st1 = _ref(case)[2]
    worst = 0.0
    for b in range(B):
        off = 0
        for l, lv in enumerate(st1[b]):
            k = lv['idx'].numel()
            assert torch.equal(idx[b, off:off + k].long(), lv['idx']), (b, l)
            assert torch.equal(valid[b, off:off + k].bool(), lv['valid']), (b, l)
            got, want = cand[b, off:off + k], lv['cand']
            assert torch.equal(got[:, 4].isnan(), want[:, 4].isnan()) and torch.equal(got[:, 4].nan_to_num(7.0), want[:, 4].nan_to_num(7.0))
            ok = lv['valid']
            if ok.any():
                worst = max(worst, float((got[ok, :4] - want[ok, :4]).abs().max()) / max(shapes[b]))
            off += k
        assert off == cand.shape[1]
    print(f'rpn stage 1 {backend} {case} pitch={pitch}: box err {worst:.3e}')
    assert worst < BOUND, worst
    return cand, valid


@pytest.mark.parametrize('case,pitch', [('small', False), ('small', True), ('full', False), ('ties', False)])
def test_stage1_emul(case, pitch):
    _stage1('emul', case, pitch)


@pytest.mark.gpu
@pytest.mark.parametrize('case,pitch', [('small', False), ('small', True), ('full', False), ('ties', False)])
def test_stage1_gpu(case, pitch):
    _stage1('hip', case, pitch)


# ----------------------------------------------------------------------------- 4. hrf_nms_segments on explicit boxes
IMG_W, IMG_H = 640.0, 384.0


@functools.lru_cache(None)
def _clustered():
    """400 cluster centres in a 640 x 384 image, sides log-uniform 8..128, aspect e^+-0.7, five copies each jittered by 6 % of the
    side and clipped: 2000 boxes; a draw that would put a pair within 1e-3 of the threshold is rejected.
    -> (cand (2000,5) fp32 in descending score order, draws, rejected)"""
    g = torch.Generator().manual_seed(11)
    boxes = torch.zeros(0, 4, dtype=torch.float32)
    draws = rejected = 0
    for _ in range(400):
        u = torch.rand(4, generator=g, dtype=torch.float64).tolist()
        s = math.exp(math.log(8.0) + u[0] * (math.log(128.0) - math.log(8.0)))
        a = math.exp(-0.7 + 1.4 * u[1])
        w, h = s * math.sqrt(a), s / math.sqrt(a)
        cx, cy = u[2] * IMG_W, u[3] * IMG_H
        n = 0
        while n < 5:
            draws += 1
            j = (torch.rand(4, generator=g, dtype=torch.float64) * 2 - 1).tolist()
            box = torch.tensor([[cx - w / 2 + 0.06 * w * j[0], cy - h / 2 + 0.06 * h * j[1], cx + w / 2 + 0.06 * w * j[2],
                                 cy + h / 2 + 0.06 * h * j[3]]], dtype=torch.float32)
            box[:, 0::2].clamp_(0, IMG_W)
            box[:, 1::2].clamp_(0, IMG_H)
            if not (float(box[0, 2] - box[0, 0]) > 0 and float(box[0, 3] - box[0, 1]) > 0) \
                    or bool(((_pair_iou(boxes.double(), box.double().expand(boxes.shape[0], 4)) - THR).abs() < 1e-3).any()):
                rejected += 1
                continue
            boxes = torch.cat([boxes, box])
            n += 1
    score = torch.randperm(2000, generator=g).float() / 100.0 - 10.0              # distinct, in (-10, 10)
    order = torch.argsort(score, descending=True)
    return torch.cat([boxes[order], score[order, None]], dim=1), draws, rejected


def test_clustered_set():
    cand, draws, rejected = _clustered()
    iou = nms_iou(cand[:, :4].double())
    pairs = int((torch.triu(iou, 1) > THR).sum())
    kept = int(nms_greedy_ref(cand[:, :4], None, THR).sum())
    print(f'clustered set: {draws} draws, {rejected} rejected, {pairs} pairs above {THR}, {kept} kept')
    assert rejected < 0.02 * draws, (draws, rejected)
    assert pairs > 2000 and 0.1 * 2000 < kept < 0.9 * 2000
    assert not bool(((iou - THR).abs() < 1e-3).any())


def _check_segments(dets, count, rois, want, max_per, b=0):
    """one image of the outputs against the restatement's dets (m,5): exact"""
    m = want.shape[0]
    assert int(count[b]) == m, (int(count[b]), m)
    assert torch.equal(dets[b, :m], want), float((dets[b, :m] - want).abs().max())
    assert not bool(dets[b, m:].any())
    r = rois[b * max_per:(b + 1) * max_per]
    assert bool((r[:, 0] == b).all()) and torch.equal(r[:m, 1:], want[:, :4]) and not bool(r[m:, 1:].any())


@functools.lru_cache(None)
def _segment_problems():
    """-> {name: (cand (2,K,5), valid (2,K) int32, seg_len, max_per, [want dets per image])}: image 0 all valid, image 1 the same
    rows with every tenth-or-so marked invalid"""
    cand = _clustered()[0]
    g = torch.Generator().manual_seed(12)
    valid = torch.ones(2, 2000, dtype=torch.int32)
    valid[1] = (torch.rand(2000, generator=g) > 0.1).int()
    out = {}
    label = torch.cat([torch.full((n,), s) for s, n in enumerate([700, 0, 1, 999, 300])])[torch.randperm(2000, generator=g)]
    for name, lab, lens in (('one', torch.zeros(2000, dtype=torch.long), [2000]), ('five', label, [700, 0, 1, 999, 300])):
        perm = torch.cat([torch.nonzero(lab == s)[:, 0] for s in range(len(lens))])      # every segment keeps the descending order
        c = cand[perm]
        v = valid[:, perm].contiguous()
        want = []
        for b in range(2):
            segs, off = [], 0
            for n in lens:
                segs.append(dict(cand=c[off:off + n], valid=v[b, off:off + n].bool()))
                off += n
            want.append(nms_segments_ref(segs, THR, 1000, sigmoid=False)[0])
        out[name] = (torch.stack([c, c]).contiguous(), v, lens, 1000, want)
    return out


def _segments(backend, name):
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    cand, valid, lens, max_per, want = _segment_problems()[name]
    dets, count, rois = (t.cpu() for t in rpn.nms_segments(cand.to(dev), valid.to(dev), lens, max_per, THR))
    for b in range(2):
        print(f'nms_segments {backend} {name} image {b}: {int(count[b])} kept')
        _check_segments(dets, count, rois, want[b], max_per, b)


@pytest.mark.parametrize('name', ['one', 'five'])
def test_nms_segments_emul(name):
    _segments('emul', name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['one', 'five'])
def test_nms_segments_gpu(name):
    _segments('hip', name)


def _box(x1, y1, x2, y2, s):
    return [float(x1), float(y1), float(x2), float(y2), float(s)]


FIXED = {
    # name: (rows in descending score order, valid or None, max_per_img, expected kept rows)
    'identical': ([_box(10, 10, 50, 40, 3), _box(10, 10, 50, 40, 2), _box(10, 10, 50, 40, 1)], None, 4, [0]),
    # 100 x 100 holds 90 x 90 (iou 0.81 > 0.7: suppressed) and 50 x 50 (iou 0.25: kept)
    'nested': ([_box(0, 0, 100, 100, 3), _box(5, 5, 95, 95, 2), _box(20, 20, 70, 70, 1)], None, 4, [0, 2]),
    # iou(A, B) = iou(B, C) = 85 / 115 = 0.74, iou(A, C) = 70 / 130 = 0.54: A suppresses B, B would have suppressed C, C is kept
    'chain': ([_box(0, 0, 100, 10, 3), _box(15, 0, 115, 10, 2), _box(30, 0, 130, 10, 1)], None, 4, [0, 2]),
    'all_invalid': ([_box(0, 0, 50, 10, 3), _box(100, 0, 160, 10, 2)], [0, 0], 4, []),
    'invalid_suppresses_nothing': ([_box(0, 0, 100, 100, 3), _box(5, 5, 95, 95, 2)], [0, 1], 4, [1]),
    'max_smaller': ([_box(0, 0, 10, 10, 5), _box(20, 0, 30, 10, 4), _box(40, 0, 50, 10, 3), _box(60, 0, 70, 10, 2)], None, 2, [0, 1]),
    'max_larger': ([_box(0, 0, 10, 10, 5), _box(20, 0, 30, 10, 4)], None, 7, [0, 1]),
}


def _fixed(backend, name):
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    rows, valid, max_per, kept = FIXED[name]
    cand = torch.tensor(rows, dtype=torch.float32)
    v = None if valid is None else torch.tensor(valid, dtype=torch.int32)
    want = nms_segments_ref([dict(cand=cand, valid=None if v is None else v.bool())], THR, max_per, sigmoid=False)[0]
    assert torch.equal(want, cand[kept][:max_per])                  # the restatement gives the expected rows
    dets, count, rois = (t.cpu() for t in rpn.nms_segments(cand[None].to(dev), None if v is None else v[None].to(dev), [len(rows)],
                                                            max_per, THR))
    _check_segments(dets, count, rois, want, max_per)


@pytest.mark.parametrize('name', sorted(FIXED))
def test_nms_fixed_emul(name):
    _fixed('emul', name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(FIXED))
def test_nms_fixed_gpu(name):
    _fixed('hip', name)


# ----------------------------------------------------------------------------- 5. / 6. end to end, hostile inputs
def _split(cand, valid, case, b):
    """device stage-1 rows of image b -> the restatement's segment list"""
    segs, off = [], 0
    for lv in _ref(case)[2][b]:
        k = lv['idx'].numel()
        segs.append(dict(cand=cand[b, off:off + k], valid=valid[b, off:off + k].bool()))
        off += k
    return segs


def _end_to_end(backend, case, pitch=False):
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    cm, rm = _nhwc(case, dev, pitch)
    shapes, nms_pre, max_per = _shapes_list(case), CASES[case][2], CASES[case][3]
    bases = [b.tolist() for b in BASES]
    cand, valid = (t.cpu() for t in rpn.select_decode(cm, rm, shapes, STRIDES, bases, nms_pre))
    dets, count, rois = (t.cpu() for t in rpn.rpn_proposals(cm, rm, shapes, STRIDES, bases, nms_pre, max_per, THR))
    assert bool(torch.isfinite(dets).all()) and bool(torch.isfinite(rois).all())
    full = _ref(case)[3]
    for b in range(B):
        # (a) stages 2 + 3 of the restatement on the device's own stage-1 rows: same candidates in the same order, box bits
        # equal, count equal; the score is the device's sigmoid against torch's
        want, src = nms_segments_ref(_split(cand, valid, case, b), THR, max_per)
        m = want.shape[0]
        assert int(count[b]) == m, (b, int(count[b]), m)
        assert torch.equal(dets[b, :m, :4], want[:, :4]), b
        se = float((dets[b, :m, 4] - want[:, 4]).abs().max()) if m else 0.0
        assert se < 1e-6, se
        assert not bool(dets[b, m:].any())
        r = rois[b * max_per:(b + 1) * max_per]
        assert bool((r[:, 0] == b).all()) and torch.equal(r[:m, 1:], want[:, :4]) and not bool(r[m:, 1:].any())
        # (b) the full restatement: same count, same source candidates, boxes within the stage-1 bound, scores within 1e-6
        fw, fsrc = full[b]
        assert m == fw.shape[0], (b, m, fw.shape[0])
        assert torch.equal(src, fsrc), b
        be = float((dets[b, :m, :4] - fw[:, :4]).abs().max()) / max(shapes[b]) if m else 0.0
        fe = float((dets[b, :m, 4] - fw[:, 4]).abs().max()) if m else 0.0
        print(f'rpn proposals {backend} {case} pitch={pitch} image {b}: {m} proposals, box err {be:.3e}, score err {se:.3e} / {fe:.3e}')
        assert be < BOUND and fe < 1e-6, (be, fe)
    return cand, valid


@pytest.mark.parametrize('case,pitch', [('small', False), ('small', True), ('full', False)])
def test_end_to_end_emul(case, pitch):
    _end_to_end('emul', case, pitch)


@pytest.mark.gpu
@pytest.mark.parametrize('case,pitch', [('small', False), ('small', True), ('full', False)])
def test_end_to_end_gpu(case, pitch):
    _end_to_end('hip', case, pitch)


def _hostile(backend):
    """NaN and +-Inf among logits and deltas: the call returns, NaN logits are never selected ahead of numbers, every output
    row is finite, count (and everything else) matches the restatement"""
    cs = _ref('hostile')[0]
    assert any(bool(m.isnan().any()) for m in cs) and any(bool(m.isinf().any()) for m in cs)
    cand, valid = _end_to_end(backend, 'hostile')
    _stage1(backend, 'hostile', False)
    off = 0
    for lv in _ref('hostile')[2][0]:
        k = lv['idx'].numel()
        for b in range(B):
            nan = cand[b, off:off + k, 4].isnan()
            assert not bool((nan[:-1] & ~nan[1:]).any())            # no number after a NaN
            assert not bool((nan & valid[b, off:off + k].bool()).any())
        off += k


def test_hostile_emul():
    _hostile('emul')


@pytest.mark.gpu
def test_hostile_gpu():
    _hostile('hip')


# ----------------------------------------------------------------------------- 7. ABI refusals (emulator)
def test_abi_refusals_emul():
    from hrfuser_amd import rpn
    dev = use_backend('emul')
    L = _lib.lib()
    cm, rm = _nhwc('small', dev)
    bases = [b.tolist() for b in BASES]
    shp = torch.tensor(_shapes_list('small'), dtype=torch.float32)
    ws = torch.empty(1 << 22, dtype=torch.uint8)
    dets, count, rois = torch.empty(B, 300, 5), torch.empty(B, dtype=torch.int32), torch.empty(B * 300, 5)

    def refused(edit_lv=None, edit_cfg=None, n=5):
        lv, cfg = rpn._levels(cm[:n], rm[:n], STRIDES[:n], bases[:n]), rpn._cfg(200, 300, THR, 0.0)
        if edit_lv:
            edit_lv(lv)
        if edit_cfg:
            edit_cfg(cfg)
        if L.hrf_rpn_supported(lv, cfg) != 0 or L.hrf_rpn_workspace_bytes(lv, cfg) != 0:
            return False
        for call in (lambda: L.hrf_rpn_proposals(lv, cfg, shp, ws, ws.numel(), dets, count, rois, 0),
                     lambda: L.hrf_rpn_select_decode(lv, cfg, shp, None, None, None, 0)):       # (null outputs: a launch would fault)
            with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
                call()
        return True

    assert not refused()                                            # the unedited call is accepted
    assert L.hrf_rpn_workspace_bytes(rpn._levels(cm, rm, STRIDES, bases), rpn._cfg(200, 300, THR, 0.0)) <= ws.numel()
    assert refused(edit_cfg=lambda c: setattr(c, 'nms_pre', 2049))
    assert refused(edit_cfg=lambda c: setattr(c, 'nms_pre', 0))
    assert refused(edit_cfg=lambda c: setattr(c, 'max_per_img', 0))
    for t in (0.0, -0.1, 1.5, float('nan')):
        assert refused(edit_cfg=lambda c, t=t: setattr(c, 'iou_thr', t)), t
    assert not refused(edit_cfg=lambda c: setattr(c, 'iou_thr', 1.0))
    assert refused(edit_cfg=lambda c: setattr(c, 'min_bbox_size', -1.0))
    assert refused(edit_lv=lambda v: setattr(v, 'A', 4))
    assert refused(edit_lv=lambda v: setattr(v, 'num_levels', 6))
    assert refused(edit_lv=lambda v: setattr(v, 'num_levels', 0))
    assert refused(edit_lv=lambda v: v.cls.__setitem__(2, None))
    assert refused(edit_lv=lambda v: v.reg.__setitem__(0, None))
    assert refused(edit_lv=lambda v: v.ld_cls.__setitem__(1, A - 1))
    assert refused(edit_lv=lambda v: v.ld_reg.__setitem__(4, 4 * A - 1))
    assert refused(edit_lv=lambda v: v.H.__setitem__(3, 0))
    # a workspace that is too small, null outputs
    lv, cfg = rpn._levels(cm, rm, STRIDES, bases), rpn._cfg(200, 300, THR, 0.0)
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
        L.hrf_rpn_proposals(lv, cfg, shp, ws, 1024, dets, count, rois, 0)
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
        L.hrf_rpn_proposals(lv, cfg, shp, ws, ws.numel(), dets, None, rois, 0)
    # hrf_nms_segments: six segments, a segment of 2049 rows, a threshold of 0, max_per_img 0
    cand = torch.zeros(1, 4, 5)
    for lens, max_per, thr in (([1, 1, 1, 1, 0, 0], 4, THR), ([2049], 4, THR), ([4], 4, 0.0), ([4], 0, THR)):
        arr = (ctypes.c_int * len(lens))(*lens)
        if max_per > 0 and thr > 0:
            assert L.hrf_nms_workspace_bytes(arr, len(lens), 1) == 0
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_nms_segments(cand, None, arr, len(lens), 1, max_per, thr, 0, ws, ws.numel(), dets, count, rois, 0)
    # the Python layer names what it refuses
    with pytest.raises(NotImplementedError, match='nms_pre'):
        rpn.rpn_proposals(cm, rm, _shapes_list('small'), STRIDES, bases, 4096, 300)


def test_module_refusals():
    """anything the kernels do not build raises NotImplementedError naming the key (no GPU needed: raised at build time)"""
    import copy
    from hrfuser_amd import HEADS

    def build(**edit):
        cfg = copy.deepcopy(dict(RPN_CFG, test_cfg=copy.deepcopy(TEST_CFG)))
        for path, v in edit.items():
            d, keys = cfg, path.split('__')
            for k in keys[:-1]:
                d = d[k]
            d[keys[-1]] = v
        return HEADS.build(cfg)

    head = build()
    assert sorted((k, tuple(v.shape)) for k, v in head.state_dict().items()) == sorted([
        ('rpn_conv.weight', (256, 256, 3, 3)), ('rpn_conv.bias', (256,)), ('rpn_cls.weight', (3, 256, 1, 1)), ('rpn_cls.bias', (3,)),
        ('rpn_reg.weight', (12, 256, 1, 1)), ('rpn_reg.bias', (12,))])
    assert float(head.rpn_conv.bias.detach().abs().max()) == 0.0 and 0.005 < float(head.rpn_conv.weight.detach().std()) < 0.02
    for edit, key in ((dict(bbox_coder__type='TBLRBBoxCoder'), 'bbox_coder.type'), (dict(anchor_generator__type='SSDAnchorGenerator'), 'anchor_generator.type'),
                      (dict(bbox_coder__target_means=[0., 0., 0.1, 0.]), 'target_means'), (dict(bbox_coder__target_stds=[1., 1., 2., 2.]), 'target_stds'),
                      (dict(anchor_generator__center_offset=0.5), 'center_offset'), (dict(anchor_generator__scales=[8, 16]), 'base anchors'),
                      (dict(loss_cls__use_sigmoid=False), 'use_sigmoid'), (dict(num_convs=2), 'num_convs'),
                      (dict(test_cfg__nms__type='soft_nms'), 'nms.type')):
        with pytest.raises(NotImplementedError, match=key):
            build(**edit)
    for fn in (head.loss, head.forward_train):
        with pytest.raises(NotImplementedError, match='assigner and sampler'):
            fn()


# ----------------------------------------------------------------------------- 8. the module, on the GPU
@functools.lru_cache(None)
def _head_cpu():
    import copy
    from hrfuser_amd import HEADS
    torch.manual_seed(3)
    head = HEADS.build(copy.deepcopy(dict(RPN_CFG, test_cfg=copy.deepcopy(TEST_CFG))))
    with torch.no_grad():
        for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
            m.bias.normal_(0.0, 0.01)
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn(B, 256, h, w, generator=g) for h, w in CASES['small'][0]]
    return head, feats


@pytest.mark.gpu
def test_module_forward_and_bboxes_gpu():
    import copy
    dev = use_backend('hip')
    head_cpu, feats = _head_cpu()
    head = copy.deepcopy(head_cpu).to(dev).eval()
    cls, reg = head([f.to(dev) for f in feats])
    assert len(cls) == len(reg) == 5
    with torch.no_grad():
        for l, f in enumerate(feats):
            y = F.relu(F.conv2d(f.double(), head_cpu.rpn_conv.weight.double(), head_cpu.rpn_conv.bias.double(), padding=1))
            wc = F.conv2d(y, head_cpu.rpn_cls.weight.double(), head_cpu.rpn_cls.bias.double())
            wr = F.conv2d(y, head_cpu.rpn_reg.weight.double(), head_cpu.rpn_reg.bias.double())
            assert cls[l].shape == wc.shape and reg[l].shape == wr.shape
            ec, er = relmax(cls[l], wc), relmax(reg[l], wr)
            print(f'RPNHead.forward level {l}: cls err {ec:.3e}, reg err {er:.3e}')
            assert ec < 1e-3 and er < 1e-3, (l, ec, er)
    metas = [dict(img_shape=(64, 96, 3)), dict(img_shape=(60, 90, 3))]
    dets, count, rois = head.proposals(cls, reg, [m['img_shape'] for m in metas])
    out = head.get_bboxes(cls, reg, metas)
    assert [o.shape[0] for o in out] == count.tolist() and all(o.shape[1] == 5 for o in out)
    assert all(torch.equal(o, dets[b, :o.shape[0]]) for b, o in enumerate(out))
    want = rpn_proposals_ref([c.cpu() for c in cls], [r.cpu() for r in reg], [(64, 96), (60, 90)], STRIDES, BASES, 200, 300)
    assert [w.shape[0] for w in want] == count.tolist()
    out2 = head.simple_test_rpn([f.to(dev) for f in feats], metas)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))


@pytest.mark.gpu
def test_module_proposals_graph_gpu():
    """proposals captured in a graph, replayed after the logits and img_shapes changed in place = a fresh eager call"""
    import copy
    from hrfuser_amd import runtime as R
    dev = use_backend('hip')
    head = copy.deepcopy(_head_cpu()[0]).to(dev).eval()
    cs, bp = _ref('small')[:2]
    cs2 = _draw('small', 101)[0]
    cls = [c.to(dev).contiguous(memory_format=torch.channels_last) for c in cs]
    reg = [r.to(dev).contiguous(memory_format=torch.channels_last) for r in bp]
    shp = torch.tensor([[64., 96.], [60., 90.]], device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        head.proposals(cls, reg, shp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with R.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
        cap = head.proposals(cls, reg, shp)
    g.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in cap]
    assert all(torch.equal(a, b) for a, b in zip(first, head.proposals(cls, reg, shp)))
    for c, c2 in zip(cls, cs2):
        c.copy_(c2.to(dev))
    shp.copy_(torch.tensor([[50., 96.], [64., 70.]], device=dev))
    g.replay()
    torch.cuda.synchronize()
    fresh = head.proposals(cls, reg, shp)
    assert all(torch.equal(a, b) for a, b in zip(cap, fresh))
    assert not torch.equal(first[0], cap[0])
    assert float(cap[0][0, :, 3].max()) <= 50.0 and float(cap[0][1, :, 2].max()) <= 70.0


@pytest.mark.gpu
def test_feature_extractor_gpu():
    import copy
    import hrfuser_oracle as O
    from hrfuser_amd.detector import FeatureExtractor
    dev = use_backend('hip')
    cfg = load_cfgs()['t_nus']
    torch.manual_seed(0)
    roi_cfg = dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                   featmap_strides=[4, 8, 16, 32])
    fx = FeatureExtractor(copy.deepcopy(cfg), dict(type='HRFPN', in_channels=[18, 36, 72, 144], out_channels=256), roi_cfg,
                          copy.deepcopy(dict(RPN_CFG, test_cfg=copy.deepcopy(TEST_CFG))))
    O.seeded_fill_(fx.backbone, 0)
    fx.neck.init_weights()
    fx.to(dev).eval()
    x, mods = O.seeded_inputs(B, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    kw = dict(zip(('lidar_img', 'radar_img', 'gated_img'), mods))
    with torch.no_grad():
        # a randomly initialised head on a seeded-filled backbone: scale rpn_reg so that the deltas are of order 0.1, as a
        # trained head's are (deltas of tens of anchor sizes push every box out of the image: all invalid, zero proposals)
        feats = fx.extract_feat(x, mods)
        cls, reg = fx.rpn_head(feats)
        mag = float(torch.cat([r.reshape(-1) for r in reg]).std())
        print(f'pyramid std {float(feats[0].std()):.3e}, logit std {float(cls[0].std()):.3e}, delta std {mag:.3e}')
        assert math.isfinite(mag) and mag > 0
        fx.rpn_head.rpn_reg.weight.mul_(0.1 / mag)
        dets, count, rois = fx.extract_proposals(x, [(64, 96), (60, 90)], **kw)
        print('proposals per image', count.tolist())
        assert dets.shape == (B, 300, 5) and rois.shape == (B * 300, 5) and bool((count > 0).all())
        out = fx.extract_roi_feats(x, **kw)
    assert out.shape == (B * 300, 256, 7, 7) and bool(torch.isfinite(out).all())
    n0 = int(count[0])
    assert bool(out[:n0].abs().sum() > 0) and not bool(out[n0:300].any())       # padded rois give rows of zeros
