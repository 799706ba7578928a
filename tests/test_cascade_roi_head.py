"""Shared2FCBBoxHead / CascadeRoIHead / FeatureExtractor.detect (hrfuser_amd/roi_head.py, detector.py) on the CPU emulator and on
the GPU against the literal torch restatements of hrfuser_amd.testing (bbox_head_ref, cascade_simple_test_ref, bbox_detect_ref).

The roi_head dict is the one of configs/_base_/models/cascade_rcnn_hrfuser_fpn_nus_clr_fusion.py:148-208 with test_cfg.rcnn
(:289-292), built unmodified.  The head's initial weights (fc_cls Normal 0.01) give eleven equal scores per roi, so the tests scale
fc_cls / fc_reg of the seeded head until the logits are ~ N(0, 2) and deltas * stds ~ N(0, 0.1), as a trained head's are.

Bounds.  forward: relmax <= 2e-5 against the fp64 restatement, the bound of hrf_fc (tests/test_bbox_head.py).  detect, stage by
stage against the fp64 restatement run on the SAME first-stage rois: the rois that enter stage i within i * 2e-5 * max(h, w) (one
decode per stage, each held to 2e-5 in test_bbox_head), the logits of stage i within (i + 1) * 2e-5 relmax.  The final step is
bit-defined given its inputs, so dets / labels / count are compared EXACTLY against bbox_detect_ref on the device's own last-stage
rois, logits and deltas (boxes: those hrf_bbox_refine decodes), scores within 1e-6; and against the all-CPU restatement the keep
set and labels are the same on the committed seed, the first of 0, 1, 2, ... for which the fp32 and the fp64 restatement agree on
them (the reference's own rounding does not move a decision), boxes within 3 * 2e-5 * max(h, w).
The emulator runs the same comparisons on a 64-channel pyramid with 64 / 64 heads and 16 random rois per image (the 256-channel
RPN and 12544 x 1024 layers take minutes on the fiber emulator); the GPU case is the issue's: 256 channels, 128 x 192, B = 2,
64 rois per image from RPNHead.proposals."""
import copy
import functools

import pytest
import torch

from helpers import load_cfgs, relmax, use_backend
from hrfuser_amd import _lib
from hrfuser_amd.testing import bbox_detect_ref, bbox_head_ref, cascade_simple_test_ref, multiclass_nms_ref

BOUND = 2e-5
STDS = [[0.1, 0.1, 0.2, 0.2], [0.05, 0.05, 0.1, 0.1], [0.033, 0.033, 0.067, 0.067]]


def _bbox_head_cfg(stds, in_channels=256, fc_out=1024, num_classes=10):
    return dict(type='Shared2FCBBoxHead', in_channels=in_channels, fc_out_channels=fc_out, roi_feat_size=7, num_classes=num_classes,
                bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.], target_stds=stds), reg_class_agnostic=True,
                loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))


def _roi_head_cfg(in_channels=256, fc_out=1024):
    return dict(type='CascadeRoIHead', num_stages=3, stage_loss_weights=[1, 0.5, 0.25],
                bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
                                        out_channels=in_channels, featmap_strides=[4, 8, 16, 32]),
                bbox_head=[_bbox_head_cfg(s, in_channels, fc_out) for s in STDS])


RCNN = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
SHAPES = [(128, 192), (120, 180)]
SIZES = [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]
STRIDES = [4, 8, 16, 32]


# ----------------------------------------------------------------------------- 1. build, keys, init, refusals (CPU)
def test_build_and_state_dict():
    from hrfuser_amd import HEADS, CascadeRoIHead, Shared2FCBBoxHead
    h = HEADS.build(_bbox_head_cfg(STDS[0]))
    assert isinstance(h, Shared2FCBBoxHead)
    assert {k: tuple(v.shape) for k, v in h.state_dict().items()} == {
        'shared_fcs.0.weight': (1024, 12544), 'shared_fcs.0.bias': (1024,), 'shared_fcs.1.weight': (1024, 1024), 'shared_fcs.1.bias': (1024,),
        'fc_cls.weight': (11, 1024), 'fc_cls.bias': (11,), 'fc_reg.weight': (4, 1024), 'fc_reg.bias': (4,)}
    rh = HEADS.build(dict(_roi_head_cfg(), test_cfg=copy.deepcopy(RCNN)))
    assert isinstance(rh, CascadeRoIHead) and rh.num_stages == 3 and len(rh.bbox_head) == 3 and len(rh.bbox_roi_extractor) == 3
    assert [tuple(b.target_stds) for b in rh.bbox_head] == [tuple(s) for s in STDS]
    g = torch.Generator().manual_seed(0)
    sd = {f'bbox_head.{i}.{k}': torch.randn(v.shape, generator=g) for i in range(3) for k, v in h.state_dict().items()}
    assert rh.load_state_dict(sd, strict=True) is not None
    assert torch.equal(rh.bbox_head[2].fc_reg.weight, sd['bbox_head.2.fc_reg.weight'])
    one = HEADS.build(dict(type='CascadeRoIHead', num_stages=2, stage_loss_weights=[1, 0.5], bbox_roi_extractor=_roi_head_cfg()['bbox_roi_extractor'],
                           bbox_head=_bbox_head_cfg(STDS[0])))
    assert len(one.bbox_head) == 2 and one.bbox_head[0] is not one.bbox_head[1]
    with pytest.raises(NotImplementedError):
        rh.forward_train()
    with pytest.raises(NotImplementedError):
        rh.loss()
    with pytest.raises(NotImplementedError):
        h.loss()


def test_init_weights():
    from hrfuser_amd import HEADS
    torch.manual_seed(0)
    h = HEADS.build(_bbox_head_cfg(STDS[0]))
    for fc_ in h.shared_fcs:
        lim = (6.0 / (fc_.weight.shape[0] + fc_.weight.shape[1])) ** 0.5                 # Xavier uniform
        assert 0.99 * lim < float(fc_.weight.detach().abs().max()) <= lim
    assert abs(float(h.fc_cls.weight.detach().std()) - 0.01) < 1e-3 and abs(float(h.fc_reg.weight.detach().std()) - 0.001) < 1e-4
    assert all(not bool(m.bias.any()) for m in (h.shared_fcs[0], h.shared_fcs[1], h.fc_cls, h.fc_reg))


@pytest.mark.parametrize('change', [
    dict(reg_class_agnostic=False), dict(num_shared_convs=1), dict(num_cls_convs=1), dict(num_reg_convs=2), dict(with_avg_pool=True),
    dict(bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0.1, 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2])),
    dict(bbox_coder=dict(type='TBLRBBoxCoder', normalizer=4.0)),
    dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)), dict(loss_cls=dict(type='SeesawLoss', num_classes=10)),
    dict(num_classes=17), dict(roi_feat_size=14), dict(in_channels=100), dict(reg_predictor_cfg=dict(type='NormedLinear')),
])
def test_build_refusals(change):
    from hrfuser_amd import HEADS
    with pytest.raises(NotImplementedError, match='not built'):
        HEADS.build(dict(_bbox_head_cfg(STDS[0]), **change))


def test_cascade_build_refusals():
    from hrfuser_amd import HEADS
    for change in (dict(mask_head=dict(type='FCNMaskHead')), dict(mask_roi_extractor=dict(type='SingleRoIExtractor')), dict(num_stages=5, stage_loss_weights=[1] * 5),
                   dict(test_cfg=dict(score_thr=0.05, nms=dict(type='soft_nms', iou_threshold=0.5), max_per_img=100)),
                   dict(test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=-1))):
        with pytest.raises(NotImplementedError, match='not built'):
            HEADS.build(dict(_roi_head_cfg(), **change))


# ----------------------------------------------------------------------------- 2. Shared2FCBBoxHead.forward
@functools.lru_cache(None)
def _head_problem(C, F, K):
    from hrfuser_amd import HEADS
    torch.manual_seed(5)
    h = HEADS.build(_bbox_head_cfg(STDS[0], C, F))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for m in (h.shared_fcs[0], h.shared_fcs[1], h.fc_cls, h.fc_reg):
            m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
        h.fc_cls.weight.mul_(100.0)
        h.fc_reg.weight.mul_(1000.0)
    x = torch.randn(K, C, 7, 7, generator=g)
    sd = {k: v.detach().clone() for k, v in h.state_dict().items()}
    return h, x, bbox_head_ref(x.double(), sd)


def _forward(backend, C, F, K, route, monkeypatch):
    dev = use_backend(backend)
    monkeypatch.setenv('HRF_FC_ROUTE', route)
    h, x, (wc, wr) = _head_problem(C, F, K)
    hd = copy.deepcopy(h).to(dev).eval()
    cls, reg = hd(x.to(dev))
    assert cls.shape == (K, 11) and reg.shape == (K, 4) and cls.data_ptr() + 44 == reg.data_ptr()      # column slices of one buffer
    ec, er = relmax(cls, wc), relmax(reg, wr)
    cls2, reg2 = hd(x.to(dev).permute(0, 2, 3, 1).contiguous(), layout='nhwc')
    assert torch.equal(cls2.isnan(), cls.isnan())
    en = max(relmax(cls2, wc), relmax(reg2, wr))
    print(f'Shared2FCBBoxHead.forward {backend} {route} C={C} F={F} K={K}: cls {ec:.3e} reg {er:.3e} nhwc {en:.3e}')
    assert max(ec, er, en) <= BOUND
    # the packed weights follow a parameter change
    with torch.no_grad():
        hd.fc_cls.bias.add_(1.0)
    assert relmax(hd(x.to(dev))[0], wc + 1.0) <= BOUND


@pytest.mark.parametrize('route', ['fc', 'rowgemm'])
def test_forward_emul(route, monkeypatch):
    _forward('emul', 64, 64, 20, route, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['fc', 'rowgemm'])
def test_forward_gpu(route, monkeypatch):
    _forward('hip', 256, 1024, 130, route, monkeypatch)


# ----------------------------------------------------------------------------- 3. CascadeRoIHead.detect
def _scaled_head(C, F, feats, rois, seed):
    """the seeded CascadeRoIHead (CPU) with fc_cls / fc_reg scaled so that logits ~ N(0, 2) and deltas * stds ~ N(0, 0.1)"""
    from hrfuser_amd import HEADS
    from hrfuser_amd.testing import roi_extract_ref
    torch.manual_seed(seed)
    rh = HEADS.build(dict(_roi_head_cfg(C, F), test_cfg=copy.deepcopy(RCNN)))
    x = roi_extract_ref([f.double() for f in feats[:4]], rois.double(), STRIDES)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i, h in enumerate(rh.bbox_head):
            cls, reg = bbox_head_ref(x, {k: v.detach() for k, v in h.state_dict().items()})
            h.fc_cls.weight.mul_(2.0 / float(cls.std()))
            h.fc_reg.weight.mul_(0.1 / STDS[i][0] / float(reg.std()))
            h.fc_cls.bias.copy_(0.5 * torch.randn(11, generator=g))
    return rh


def _random_rois(R, seed):
    g = torch.Generator().manual_seed(seed)
    rois = torch.zeros(2 * R, 5)
    for b, (h, w) in enumerate(SHAPES):
        c = torch.rand(6, 2, generator=g) * torch.tensor([w, h])
        wh = 10 + torch.rand(6, 2, generator=g) * 70
        base = torch.cat([c - wh / 2, c + wh / 2], dim=1)[torch.randint(0, 6, (R,), generator=g)]
        box = base + 0.1 * (base[:, 2:] - base[:, :2]).repeat(1, 2) * (torch.rand(R, 4, generator=g) * 2 - 1)
        box[:, 0::2].clamp_(0, w)
        box[:, 1::2].clamp_(0, h)
        rois[b * R:(b + 1) * R, 0] = b
        rois[b * R:(b + 1) * R, 1:] = box
    return rois


@functools.lru_cache(None)
def _emul_problem(seed):
    g = torch.Generator().manual_seed(100 + seed)
    feats = [torch.randn(2, 64, h, w, generator=g) for h, w in SIZES[:4]]
    rois = _random_rois(16, 200 + seed)
    return feats, rois, (16, 11), _scaled_head(64, 64, feats, rois, seed)


def _refs(rh, feats, rois, counts):
    sds = [{k: v.detach().clone() for k, v in h.state_dict().items()} for h in rh.bbox_head]
    return {dt: cascade_simple_test_ref(feats[:4], rois, counts, SHAPES, sds, STDS, STRIDES, 0.05, 0.5, 100, dtype=dt)
            for dt in (torch.float64, torch.float32)}


def _agree(refs):
    """the fp32 and the fp64 restatement take the same decisions"""
    a, b = refs[torch.float64][0], refs[torch.float32][0]
    return all(torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) for x, y in zip(a, b))


def _check_detect(backend, rh_cpu, feats, rois, counts, dev, strict_vs_cpu):
    refs = _refs(rh_cpu, feats, rois.cpu(), counts)
    want, stage_rois = refs[torch.float64]
    rh = copy.deepcopy(rh_cpu).to(dev).eval()
    R = rois.shape[0] // 2
    cnt = torch.tensor(counts, dtype=torch.int32).to(dev)
    stages = []
    dets, labels, n = rh.detect([f.to(dev) for f in feats], rois.to(dev), cnt, SHAPES, stages=stages)
    assert dets.shape == (2, 100, 5) and labels.shape == (2, 100) and labels.dtype == torch.int32 and n.dtype == torch.int32
    dets, labels, n = dets.cpu(), labels.cpu(), n.cpu()
    sds = [{k: v.detach() for k, v in h.state_dict().items()} for h in rh_cpu.bbox_head]
    from hrfuser_amd.testing import roi_extract_ref
    for i, (r_dev, out) in enumerate(stages):
        r_dev, out = r_dev.cpu(), out.cpu()
        err = max(float((r_dev[b * R:(b + 1) * R, 1:] - stage_rois[i][b * R:(b + 1) * R, 1:]).abs().max()) / max(SHAPES[b]) for b in range(2))
        assert torch.equal(r_dev[:, 0], stage_rois[i][:, 0])
        cls, _ = bbox_head_ref(roi_extract_ref([f.double() for f in feats[:4]], stage_rois[i].double(), STRIDES), sds[i])
        el = relmax(out[:, :11], cls)
        print(f'detect {backend} stage {i}: rois err {err:.3e} (bound {i * BOUND:.1e}), logits relmax {el:.3e} (bound {(i + 1) * BOUND:.1e})')
        assert err <= i * BOUND and el <= (i + 1) * BOUND
    # the final step on the device's own inputs: exact
    from hrfuser_amd import roi_head
    r_last, o_last = stages[-1]
    boxes = roi_head.bbox_refine(r_last, o_last[:, 11:15], STDS[2], SHAPES, 2).cpu()[:, 1:]
    mean = sum(o.cpu()[:, :11] for _, o in stages) / 3.0
    for b in range(2):
        sl = slice(b * R, (b + 1) * R)
        wd, wl, _ = multiclass_nms_ref(boxes[sl], torch.softmax(mean[sl], dim=-1), 0.05, 0.5, 100, torch.arange(R) < counts[b])
        m = wd.shape[0]
        assert int(n[b]) == m and torch.equal(labels[b, :m].long(), wl) and torch.equal(dets[b, :m, :4], wd[:, :4])
        assert m == 0 or float((dets[b, :m, 4] - wd[:, 4]).abs().max()) <= 1e-6
        assert bool((labels[b, m:] == -1).all()) and not bool(dets[b, m:].any())
        print(f'detect {backend} image {b}: {m} detections')
        if strict_vs_cpu:                                           # the all-CPU restatement: same keep set and labels, boxes within the bound
            cd, cl, _ = want[b]
            assert cd.shape[0] == m and torch.equal(cl, wl)
            assert float((dets[b, :m, :4] - cd[:, :4]).abs().max()) / max(SHAPES[b]) <= 3 * BOUND
            assert float((dets[b, :m, 4] - cd[:, 4]).abs().max()) <= 1e-4
    return rh, refs


EMUL_SEED = 0


def test_inputs_unambiguous_emul():
    first = next(s for s in range(EMUL_SEED + 1) if _agree(_refs(_emul_problem(s)[3], _emul_problem(s)[0], _emul_problem(s)[1], _emul_problem(s)[2])))
    assert first == EMUL_SEED


def test_detect_emul():
    dev = use_backend('emul')
    feats, rois, counts, rh = _emul_problem(EMUL_SEED)
    _check_detect('emul', rh, feats, rois, counts, dev, True)


def test_simple_test_emul():
    import numpy as np
    dev = use_backend('emul')
    feats, rois, counts, rh = _emul_problem(EMUL_SEED)
    rh = copy.deepcopy(rh).eval()
    props = [torch.cat([rois[b * 16:b * 16 + c, 1:], torch.ones(c, 1)], dim=1) for b, c in enumerate(counts)]
    metas = [dict(img_shape=s + (3,), scale_factor=np.array([2., 2., 2., 2.], dtype=np.float32)) for s in SHAPES]
    res = rh.simple_test(feats, props, metas, rescale=True)
    assert len(res) == 2 and all(len(r) == 10 for r in res)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 5 for r in res for a in r)
    plain = rh.simple_test(feats, props, metas, rescale=False)
    assert sum(a.shape[0] for a in plain[0]) > 0
    for r, p in zip(res, plain):
        for a, q in zip(r, p):
            assert a.shape == q.shape and np.array_equal(a[:, :4], q[:, :4] / 2.0) and np.array_equal(a[:, 4], q[:, 4])
    empty = rh.simple_test(feats, [torch.zeros(0, 5), torch.zeros(0, 5)], metas)
    assert all(a.shape == (0, 5) and a.dtype == np.float32 for r in empty for a in r)


# ----------------------------------------------------------------------------- 4. the GPU case: RPN rois, 256 channels
GPU_SEED = 0


@functools.lru_cache(None)
def _gpu_pyramid(seed):
    g = torch.Generator().manual_seed(300 + seed)
    return [torch.randn(2, 256, h, w, generator=g) for h, w in SIZES]


def _rpn_head(dev):
    from hrfuser_amd import HEADS
    from test_rpn_proposals import RPN_CFG
    torch.manual_seed(7)
    head = HEADS.build(dict(copy.deepcopy(RPN_CFG), test_cfg=dict(nms_pre=200, max_per_img=64, nms=dict(type='nms', iou_threshold=0.7), min_bbox_size=0)))
    with torch.no_grad():
        head.rpn_reg.weight.mul_(0.5)
    return head.to(dev).eval()


@pytest.mark.gpu
def test_detect_gpu():
    dev = use_backend('hip')
    feats = _gpu_pyramid(GPU_SEED)
    rpn = _rpn_head(dev)
    fd = [f.to(dev) for f in feats]
    _, count, rois = rpn.proposals(*rpn(fd), SHAPES)
    counts = tuple(count.tolist())
    print('proposals per image', counts)
    assert rois.shape == (128, 5) and min(counts) > 8
    rh = _scaled_head(256, 1024, feats, rois.cpu(), GPU_SEED)
    _, refs = _check_detect('hip', rh, feats, rois.cpu(), counts, dev, True)
    assert _agree(refs)                                             # the committed seed is unambiguous for the restatement itself


@pytest.mark.gpu
def test_detect_graph_and_deterministic_gpu():
    """detect captured in a graph, replayed after the pyramid, img_shapes and count changed in place = a fresh eager call, bit for
    bit; the same bits in deterministic mode"""
    from hrfuser_amd import runtime as R
    dev = use_backend('hip')
    L = _lib.lib()
    feats = [f.to(dev) for f in _gpu_pyramid(GPU_SEED)]
    other = [f.to(dev) for f in _gpu_pyramid(GPU_SEED + 1)]
    rois = _random_rois(64, 9).to(dev)
    rh = _scaled_head(256, 1024, _gpu_pyramid(GPU_SEED), rois.cpu(), GPU_SEED).to(dev).eval()
    shp = torch.tensor([[128., 192.], [120., 180.]], device=dev)
    cnt = torch.tensor([64, 40], dtype=torch.int32, device=dev)
    eager = rh.detect(feats, rois, cnt, shp)
    L.hrf_set_deterministic(1)
    try:
        det = rh.detect(feats, rois, cnt, shp)
    finally:
        L.hrf_set_deterministic(0)
    assert all(torch.equal(a, b) for a, b in zip(eager, det))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rh.detect(feats, rois, cnt, shp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with R.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
        cap = rh.detect(feats, rois, cnt, shp)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(cap, eager))
    first = [t.clone() for t in cap]
    for f, o in zip(feats, other):
        f.copy_(o)
    shp.copy_(torch.tensor([[100., 192.], [120., 150.]], device=dev))
    cnt.copy_(torch.tensor([30, 64], dtype=torch.int32, device=dev))
    g.replay()
    torch.cuda.synchronize()
    fresh = rh.detect(feats, rois, cnt, shp)
    assert all(torch.equal(a, b) for a, b in zip(cap, fresh))
    assert not torch.equal(first[0], cap[0])
    assert float(cap[0][0, :, 3].max()) <= 100.0 and float(cap[0][1, :, 2].max()) <= 150.0


@pytest.mark.gpu
def test_simple_test_gpu():
    import numpy as np
    dev = use_backend('hip')
    feats = [f.to(dev) for f in _gpu_pyramid(GPU_SEED)]
    rois = _random_rois(64, 9)
    rh = _scaled_head(256, 1024, _gpu_pyramid(GPU_SEED), rois, GPU_SEED).to(dev).eval()
    props = [torch.cat([rois[b * 64:b * 64 + c, 1:], torch.ones(c, 1)], dim=1).to(dev) for b, c in enumerate((64, 33))]
    metas = [dict(img_shape=s + (3,), scale_factor=np.array([1., 1., 1., 1.], dtype=np.float32)) for s in SHAPES]
    res = rh.simple_test(feats, props, metas)
    assert len(res) == 2 and all(len(r) == 10 for r in res)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 5 for r in res for a in r)
    assert all(0 < sum(a.shape[0] for a in r) <= 100 for r in res)


@pytest.mark.gpu
def test_feature_extractor_detect_gpu():
    """HRFuser-T at 2 x 128 x 192: images -> detections; a FeatureExtractor without roi_head is what it was"""
    import hrfuser_oracle as O
    from hrfuser_amd.detector import FeatureExtractor
    from test_rpn_proposals import RPN_CFG
    dev = use_backend('hip')
    cfg = load_cfgs()['t_nus']
    torch.manual_seed(0)
    rpn_cfg = dict(copy.deepcopy(RPN_CFG), test_cfg=dict(nms_pre=200, max_per_img=64, nms=dict(type='nms', iou_threshold=0.7), min_bbox_size=0))
    neck = dict(type='HRFPN', in_channels=[18, 36, 72, 144], out_channels=256)
    fx = FeatureExtractor(copy.deepcopy(cfg), neck, None, rpn_cfg, dict(_roi_head_cfg(), test_cfg=copy.deepcopy(RCNN)))
    O.seeded_fill_(fx.backbone, 0)
    fx.neck.init_weights()
    fx.to(dev).eval()
    x, mods = O.seeded_inputs(2, 128, 192, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    kw = dict(zip(('lidar_img', 'radar_img', 'gated_img'), mods))
    with torch.no_grad():
        feats = fx.extract_feat(x, mods)
        cls, reg = fx.rpn_head(feats)
        fx.rpn_head.rpn_reg.weight.mul_(0.1 / float(torch.cat([r.reshape(-1) for r in reg]).std()))
        dets, labels, count = fx.detect(x, SHAPES, **kw)
    assert dets.shape == (2, 100, 5) and labels.shape == (2, 100) and count.shape == (2,)
    assert bool(torch.isfinite(dets).all()) and bool((count >= 0).all()) and bool((count <= 100).all())
    c = count.tolist()
    print('detections per image', c)
    for b in range(2):
        assert bool((labels[b, :c[b]] >= 0).all()) and bool((labels[b, :c[b]] < 10).all()) and bool((labels[b, c[b]:] == -1).all())
        assert float(dets[b, :, 2].max()) <= SHAPES[b][1] and float(dets[b, :, 3].max()) <= SHAPES[b][0]
    import numpy as np
    metas = [dict(img_shape=s + (3,), scale_factor=np.ones(4, dtype=np.float32)) for s in SHAPES]
    res = fx.simple_test(x, metas, **{k: [v] for k, v in kw.items()})
    assert len(res) == 2 and all(len(r) == 10 for r in res) and [sum(a.shape[0] for a in r) for r in res] == c
    plain = FeatureExtractor(fx.backbone, fx.neck, None, fx.rpn_head)
    assert not hasattr(plain, 'roi_head')
    with pytest.raises(ValueError, match='roi_head'):
        plain.detect(x, SHAPES, **kw)
    d2, c2, r2 = plain.extract_proposals(x, SHAPES, **kw)
    assert d2.shape == (2, 64, 5) and r2.shape == (128, 5)
