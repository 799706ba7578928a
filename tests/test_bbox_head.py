"""The kernels of the cascade bbox head at test time (csrc/hrf_fc.h: hrf_fc; csrc/hrf_bbox.h: hrf_bbox_refine / hrf_bbox_detect)
through the C ABI on the CPU emulator and on the GPU, against fp64 F.linear and the literal torch restatements of
hrfuser_amd.testing (bbox_delta2bbox, multiclass_nms_ref / bbox_detect_ref).

Bounds.  hrf_fc: relmax <= 2e-5, the bound of the sibling kernel tests (test_rpn_proposals.BOUND, test_roi_align), valid because
torch's own fp32 CPU F.linear on the same inputs stays under a quarter of it (test_fc_bound_holds: measured 3.3e-7 at
K = 12544).  hrf_bbox_refine: batch column identical, max|box - want| / max(h, w) < 2e-5 (one expf per side).  hrf_bbox_detect:
everything after the box decode and the softmax is bit-defined, so keep set, order, labels, count and the copied box bits are
compared EXACTLY against the restatement run on identical input boxes - the boxes hrf_bbox_refine decodes on the same backend
(the same device function; itself held to the restatement above) - and the scores within 1e-6 (device expf softmax against
torch.softmax).

Unambiguous seeds.  The issue asks for "no two valid scores of an image within 4e-6 of each other".  With logits ~ N(0, 2) an
image of the first case has ~1300 valid scores between 0.05 and 1: about thirty such pairs are EXPECTED per draw and no seed
passes (nor does one with the condition taken per class: seven pairs expected).  What makes the restatement ambiguous is a
near-tie where the ORDER decides something, so the condition is taken there: no two valid scores of one (image, class) within
4e-6 whose boxes overlap above iou_thr - 1e-5 (greedy NMS depends on the order of two candidates only when one can suppress the
other; four scores within 4e-6 in a row are rejected outright) and no two KEPT scores of an image within 4e-6 (the merge and the
cut at max_per_img).  The other two conditions are as stated: no valid row's score within 1e-6 of score_thr, no fp64 IoU of two
candidate boxes of an image within 1e-5 of iou_thr.  The full-width case (R = 2048: the whole sort and a 32 x 32 block
suppression matrix) has `count` = (400, 250): the valid rows are spread over all 2048 sorted positions."""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import relmax, use_backend
from hrfuser_amd import _lib
from hrfuser_amd.testing import bbox_delta2bbox, bbox_detect_ref, nms_iou

BOUND = 2e-5


# ----------------------------------------------------------------------------- 1. hrf_fc
@functools.lru_cache(None)
def _fc_problem(M, K, N, pitch=0):
    """-> (x (M,K) fp32, w (N,K), bias (N,), rows checked, fp64 reference of those rows WITHOUT ReLU)"""
    g = torch.Generator().manual_seed(1000 + M + K + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    if M > 512:                                                    # first and last row of every 128-row tile + 64 random rows
        rows = sorted(set([r for t in range(0, M, 128) for r in (t, min(t + 127, M - 1))] + torch.randint(0, M, (64,), generator=g).tolist()))
    else:
        rows = list(range(M))
    rows = torch.tensor(rows)
    ref = F.linear(x[rows].double(), w.double(), bias.double())
    return x, w, bias, rows, ref


def _fc_run(backend, M, K, N, relu, route, pitch=0):
    from hrfuser_amd import roi_head
    dev = use_backend(backend)
    L = _lib.lib()
    x, w, bias, rows, ref = _fc_problem(M, K, N)
    wp = torch.empty((N * K,), device=dev)
    L.hrf_fc_pack(w.to(dev), N, K, N, K, wp, _lib.stream_ptr())
    if pitch:
        big = torch.full((M, K + pitch), float('nan'))
        big[:, :K] = x
        xd = big.to(dev)[:, :K]
    else:
        xd = x.to(dev)
    out = [roi_head.fc(xd, wp, bias.to(dev), N, relu, route=route).cpu() for _ in range(2)]
    assert torch.equal(out[0], out[1])                             # bit-reproducible from run to run
    want = ref.clamp(min=0) if relu else ref
    err = relmax(out[0][rows], want)
    print(f'hrf_fc {backend} route={route} M={M} K={K} N={N} relu={relu} pitch={pitch}: relmax {err:.3e}')
    assert err <= BOUND, err
    if relu:
        assert bool((out[0] >= 0).all())
    return out[0]


@pytest.mark.parametrize('route', ['fc', 'rowgemm'])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('M,K,N', [(1, 784, 64), (127, 3136, 80), (130, 784, 80), (130, 3136, 64)])
def test_fc_emul(M, K, N, relu, route):
    _fc_run('emul', M, K, N, relu, route)


def test_fc_pitch_emul():
    _fc_run('emul', 130, 784, 80, True, 'fc', pitch=8)


def test_fc_splits_agree_emul():
    """K = 3136 at M = 130 is split (the workspace query says so) and K = 16 is not: both paths ran above / run here"""
    L = (use_backend('emul'), _lib.lib())[1]
    assert L.hrf_fc_workspace_bytes(130, 3136, 80) > 0 and L.hrf_fc_workspace_bytes(130, 16, 80) == 0
    _fc_run('emul', 130, 16, 80, True, 'fc')


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['fc', 'rowgemm'])
@pytest.mark.parametrize('M,relu', [(1, True), (130, False), (130, True), (2000, True), (2000, False)])
def test_fc_gpu(M, relu, route):
    _fc_run('hip', M, 12544, 1024, relu, route)


@pytest.mark.gpu
def test_fc_pitch_gpu():
    _fc_run('hip', 130, 12544, 1024, True, 'fc', pitch=16)


def test_fc_bound_holds():
    """the bound 2e-5 stands if torch's own fp32 CPU F.linear stays under a quarter of it on the GPU test's inputs"""
    for M in (130, 2000):
        x, w, bias, rows, ref = _fc_problem(M, 12544, 1024)
        err = relmax(F.linear(x[rows], w, bias), ref)
        print(f'fp32 CPU F.linear M={M} K=12544 N=1024: relmax {err:.3e}')
        assert err < BOUND / 4, err


def _fc_refusals(backend):
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    x, wp, b, y = torch.zeros(4, 32, device=dev), torch.zeros(16 * 32, device=dev), torch.zeros(16, device=dev), torch.zeros(4, 16, device=dev)
    ws = torch.zeros(1 << 16, device=dev, dtype=torch.uint8)
    ok = (x, 32, wp, b, y, 16, 1, 4, 32, 16, ws, ws.numel(), s)
    L.hrf_fc(*ok)
    L.hrf_fc(x, 32, wp, b, y, 16, 1, 0, 32, 16, None, 0, s)        # M = 0: nothing to do
    bad = {'K % 16': dict(i8=24), 'N % 16': dict(i9=8), 'null x': dict(i0=None), 'null wp': dict(i2=None), 'null y': dict(i4=None),
           'ldX < K': dict(i1=16), 'ldY < N': dict(i5=8), 'relu': dict(i6=2), 'M < 0': dict(i7=-1)}
    for name, ch in bad.items():
        a = list(ok)
        for k, v in ch.items():
            a[int(k[1:])] = v
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_fc(*a)
    need = L.hrf_fc_workspace_bytes(130, 3136, 80)
    assert need > 0
    xx, ww, yy = torch.zeros(130, 3136, device=dev), torch.zeros(80 * 3136, device=dev), torch.zeros(130, 80, device=dev)
    for w_, n_ in ((None, 0), (ws, need - 1)):
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_fc(xx, 3136, ww, None, yy, 80, 0, 130, 3136, 80, w_, n_, s)
    assert L.hrf_fc_workspace_bytes(130, 3128, 80) == 0
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
        L.hrf_fc_pack(x, 16, 32, 16, 24, wp, s)


def test_fc_refusals_emul():
    _fc_refusals('emul')


@pytest.mark.gpu
def test_fc_refusals_gpu():
    _fc_refusals('hip')


# ----------------------------------------------------------------------------- 2. hrf_bbox_refine
SHAPES = [(128, 192), (120, 180)]
STDS = (0.1, 0.1, 0.2, 0.2)


@functools.lru_cache(None)
def _refine_problem(hostile):
    g = torch.Generator().manual_seed(3)
    R = 70
    rois = torch.zeros(2 * R, 5)
    for b, (h, w) in enumerate(SHAPES):
        c = torch.rand(R, 2, generator=g) * torch.tensor([w, h])
        wh = 4 + torch.rand(R, 2, generator=g) * 60
        box = torch.cat([c - wh / 2, c + wh / 2], dim=1)
        box[:, 0::2].clamp_(0, w)
        box[:, 1::2].clamp_(0, h)
        rois[b * R:(b + 1) * R, 0] = b
        rois[b * R:(b + 1) * R, 1:] = box
        rois[(b + 1) * R - 6:(b + 1) * R, 1:] = 0                    # padded rows (b, 0, 0, 0, 0)
    deltas = 0.5 * torch.randn(2 * R, 4, generator=g) / torch.tensor(STDS)       # deltas * stds ~ N(0, 0.5): the clamp and the clip are hit
    if hostile:
        special = torch.tensor([float('nan'), float('inf'), float('-inf'), float('nan')])
        hit = torch.rand(deltas.shape, generator=g) < 0.1
        deltas[hit] = special[torch.randint(0, 4, deltas.shape, generator=g)][hit]
        rois[3, 0], rois[4, 0], rois[5, 0], rois[6, 0] = 2.0, -1.0, 0.5, float('nan')
    return rois, deltas


def _refine(backend, hostile):
    from hrfuser_amd import roi_head
    dev = use_backend(backend)
    rois, deltas = _refine_problem(hostile)
    R = rois.shape[0] // 2
    pad = torch.full((2 * R, 16), float('nan'))
    pad[:, 11:15] = deltas                                          # a column slice of a padded head output
    got = roi_head.bbox_refine(rois.to(dev), pad.to(dev)[:, 11:15], STDS, SHAPES, 2).cpu()
    bidx = rois[:, 0]
    good = (bidx == bidx.floor()) & (bidx >= 0) & (bidx < 2)
    assert torch.equal(got[:, 0].nan_to_num(-7.0), bidx.nan_to_num(-7.0))
    assert not bool(got[~good, 1:].any())                           # a bad batch index: the box (0, 0, 0, 0)
    worst = 0.0
    for b, shp in enumerate(SHAPES):
        sel = good & (bidx == b)
        want = bbox_delta2bbox(rois[sel, 1:], deltas[sel], STDS, max_shape=shp)
        g = got[sel, 1:]
        assert torch.equal(g.isnan(), want.isnan())
        worst = max(worst, float((g - want).nan_to_num(0.0).abs().max()) / max(shp))
        if not hostile:
            assert not bool(g[-6:].any())                           # padded rows stay zero
            assert int((want == 0).sum() + (want[:, 0::2] == shp[1]).sum() + (want[:, 1::2] == shp[0]).sum()) > 10      # the clip is hit
    print(f'hrf_bbox_refine {backend} hostile={hostile}: box err {worst:.3e}')
    assert worst < BOUND, worst


@pytest.mark.parametrize('hostile', [False, True])
def test_refine_emul(hostile):
    _refine('emul', hostile)


@pytest.mark.gpu
@pytest.mark.parametrize('hostile', [False, True])
def test_refine_gpu(hostile):
    _refine('hip', hostile)


def test_refine_refusals_emul():
    dev = use_backend('emul')
    L, s = _lib.lib(), _lib.stream_ptr()
    r, d, shp = torch.zeros(4, 5), torch.zeros(4, 4), torch.ones(1, 2)
    L.hrf_bbox_refine(r, d, 4, .1, .1, .2, .2, shp, 1, 4, r.clone(), s)
    for a in ((None, d, 4, .1, .1, .2, .2, shp, 1, 4, r, s), (r, d, 3, .1, .1, .2, .2, shp, 1, 4, r, s), (r, d, 4, 0., .1, .2, .2, shp, 1, 4, r, s),
              (r, d, 4, .1, .1, .2, float('nan'), shp, 1, 4, r, s), (r, d, 4, .1, .1, .2, .2, None, 1, 4, r, s), (r, d, 4, .1, .1, .2, .2, shp, 0, 4, r, s),
              (r, d, 4, .1, .1, .2, .2, shp, 1, -1, r, s), (r, d, 4, .1, .1, .2, .2, shp, 1, 4, None, s)):
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_bbox_refine(*a)


# ----------------------------------------------------------------------------- 3. hrf_bbox_detect
SCORE_THR, IOU_THR = 0.05, 0.5
DET_CASES = {
    # name: (R, num_classes, count, max_per_img, rescale, committed seed)
    'cfg': (300, 10, (300, 170), 100, False, 8),
    'cfg_rescale': (300, 10, (300, 170), 100, True, 8),
    'full': (2048, 3, (400, 250), 100, False, 1),
    'hostile': (300, 10, (300, 170), 100, False, 4),
    'empty': (300, 10, (0, 170), 100, False, 0),
}
SCALE = [(1.5, 1.25, 1.5, 1.25), (0.75, 0.5, 0.75, 0.5)]


def _det_draw(case, seed):
    """-> (rois (2R,5), [logits (2R, C+1)] * 3, deltas (2R,4)).  rois: jittered copies of 30 cluster boxes per image"""
    R, C = DET_CASES[case][:2]
    g = torch.Generator().manual_seed(seed)
    rois = torch.zeros(2 * R, 5)
    for b, (h, w) in enumerate(SHAPES):
        c = torch.rand(30, 2, generator=g) * torch.tensor([w, h])
        wh = 8 + torch.rand(30, 2, generator=g) * 56
        base = torch.cat([c - wh / 2, c + wh / 2], dim=1)[torch.randint(0, 30, (R,), generator=g)]
        side = (base[:, 2:] - base[:, :2]).repeat(1, 2)
        box = base + 0.08 * side * (torch.rand(R, 4, generator=g) * 2 - 1)
        box[:, 0::2].clamp_(0, w)
        box[:, 1::2].clamp_(0, h)
        rois[b * R:(b + 1) * R, 0] = b
        rois[b * R:(b + 1) * R, 1:] = box
    logits = [2.0 * torch.randn(2 * R, C + 1, generator=g) for _ in range(3)]
    deltas = 0.3 * torch.randn(2 * R, 4, generator=g)
    if case == 'hostile':
        special = torch.tensor([float('nan'), float('inf'), float('-inf'), float('nan')])
        for t in logits + [deltas]:
            hit = torch.rand(t.shape, generator=g) < 0.02
            t[hit] = special[torch.randint(0, 4, t.shape, generator=g)][hit]
    return rois, logits, deltas


def _unambiguous(case, seed):
    """the restatement on the CPU-decoded boxes is unambiguous for this draw (module docstring)"""
    R, C, count, max_per, rescale, _ = DET_CASES[case]
    rois, logits, deltas = _det_draw(case, seed)
    mean = sum(logits) / 3.0
    sf = SCALE if rescale else None
    for b in range(2):
        sl = slice(b * R, b * R + count[b])
        sc = torch.softmax(mean[sl], dim=-1)[:, :C]
        sc = torch.where(torch.isnan(sc), torch.zeros_like(sc), sc)
        if bool(((sc - SCORE_THR).abs() < 1e-6).any()):
            return False
        boxes = bbox_delta2bbox(rois[sl, 1:], deltas[sl], STDS, max_shape=SHAPES[b])
        if sf is not None:
            boxes = boxes / boxes.new_tensor(sf[b])
        iou = nms_iou(boxes.double()).nan_to_num(1.0)               # (a NaN box: treated as overlapping everything)
        any_valid = (sc > SCORE_THR).any(dim=1)
        pair = any_valid[:, None] & any_valid[None, :]
        if bool(((torch.triu(iou, 1) - IOU_THR).abs() < 1e-5)[pair].any()):
            return False
        for c in range(C):
            idx = torch.nonzero(sc[:, c] > SCORE_THR)[:, 0]
            v, o = sc[idx, c].sort()
            idx = idx[o]
            for d in (1, 2, 3):                                      # near-ties up to three sorted places apart
                if v.numel() > d:
                    close = torch.nonzero((v[d:] - v[:-d]) < 4e-6)[:, 0]
                    if d == 3 and close.numel():
                        return False
                    if bool((iou[idx[close], idx[close + d]] > IOU_THR - 1e-5).any()):
                        return False
    res = bbox_detect_ref(rois, logits, deltas, STDS, SHAPES, count, SCORE_THR, IOU_THR, 1 << 20, sf)
    for b in range(2):
        kept = res[b][0][:, 4].sort().values
        if kept.numel() > 1 and float((kept[1:] - kept[:-1]).min()) < 4e-6:
            return False
    return True


@pytest.mark.parametrize('case', sorted(DET_CASES))
def test_inputs_unambiguous(case):
    """the committed seed is the first of 0, 1, 2, ... whose restatement is unambiguous"""
    seed = DET_CASES[case][5]
    first = next(s for s in range(seed + 1) if _unambiguous(case, s))
    assert first == seed, (case, first)


def test_suppression_is_common():
    R, C, count, max_per, rescale, seed = DET_CASES['cfg']
    rois, logits, deltas = _det_draw('cfg', seed)
    res = bbox_detect_ref(rois, logits, deltas, STDS, SHAPES, count, SCORE_THR, IOU_THR, 1 << 20)
    for b in range(2):
        sc = torch.softmax((sum(logits) / 3.0)[b * R:b * R + count[b]], dim=-1)[:, :C]
        n, kept = int((sc > SCORE_THR).sum()), res[b][0].shape[0]
        print(f'image {b}: {kept} of {n} candidates kept')
        assert 0.05 * n < kept < 0.9 * n and kept > max_per


def _detect(backend, case):
    from hrfuser_amd import roi_head
    dev = use_backend(backend)
    R, C, count, max_per, rescale, seed = DET_CASES[case]
    rois, logits, deltas = _det_draw(case, seed)
    sf = SCALE if rescale else None
    pad = [torch.full((2 * R, 16), float('nan')) for _ in range(3)]                # the padded head outputs: logits, deltas, NaN
    for p, l in zip(pad, logits):
        p[:, :C + 1] = l
    pad[2][:, C + 1:C + 5] = deltas
    pd = [p.to(dev) for p in pad]
    cnt = torch.tensor(count, dtype=torch.int32).to(dev)
    dets, labels, n = (t.cpu() for t in roi_head.bbox_detect(rois.to(dev), cnt, [p[:, :C + 1] for p in pd], pd[2][:, C + 1:C + 5], STDS, SHAPES, 2, C,
                                                              SCORE_THR, IOU_THR, max_per, sf))
    # the restatement on identical input boxes: the rows hrf_bbox_refine decodes on this backend (held to bbox_delta2bbox above)
    boxes = roi_head.bbox_refine(rois.to(dev), pd[2][:, C + 1:C + 5], STDS, SHAPES, 2).cpu()[:, 1:]
    mean = sum(logits) / 3.0
    from hrfuser_amd.testing import multiclass_nms_ref
    for b in range(2):
        sl = slice(b * R, (b + 1) * R)
        bx = boxes[sl] / boxes.new_tensor(sf[b]) if sf is not None else boxes[sl]
        want, wl, src = multiclass_nms_ref(bx, torch.softmax(mean[sl], dim=-1), SCORE_THR, IOU_THR, max_per, torch.arange(R) < count[b])
        m = want.shape[0]
        print(f'hrf_bbox_detect {backend} {case} image {b}: {m} detections')
        assert int(n[b]) == m, (int(n[b]), m)
        assert torch.equal(labels[b, :m].long(), wl) and bool((labels[b, m:] == -1).all())
        got = dets[b, :m, :4]                                       # (hostile: a NaN box is kept like any other)
        assert torch.equal(got.isnan(), want[:, :4].isnan()) and torch.equal(got.nan_to_num(-1.0), want[:, :4].nan_to_num(-1.0))
        assert float((dets[b, :m, 4] - want[:, 4]).abs().max()) <= 1e-6 if m else True
        assert not bool((dets[b, m:] != 0).any())
        if case == 'empty' and count[b] == 0:
            assert m == 0
        elif case in ('cfg', 'cfg_rescale'):
            assert m == max_per


@pytest.mark.parametrize('case', sorted(DET_CASES))
def test_detect_emul(case):
    _detect('emul', case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(DET_CASES))
def test_detect_gpu(case):
    _detect('hip', case)


def _detect_refusals(backend):
    from hrfuser_amd import roi_head
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    R, C = 8, 3
    rois, lg, dl = torch.zeros(2 * R, 5, device=dev), torch.zeros(2 * R, C + 1, device=dev), torch.zeros(2 * R, 4, device=dev)
    shp = torch.ones(2, 2, device=dev)
    ws = torch.zeros(L.hrf_bbox_detect_workspace_bytes(2, R, C), device=dev, dtype=torch.uint8)
    dets, lab, cnt = torch.zeros(2, 5, 5, device=dev), torch.zeros(2, 5, device=dev, dtype=torch.int32), torch.zeros(2, device=dev, dtype=torch.int32)

    def make(**kw):
        d = _lib.BboxDet()
        d.B, d.R, d.num_classes, d.num_stages = 2, R, C, 1
        d.rois, d.logits[0], d.ld_logits, d.deltas, d.ld_deltas, d.img_shape = rois.data_ptr(), lg.data_ptr(), C + 1, dl.data_ptr(), 4, shp.data_ptr()
        for k in range(4):
            d.stds[k] = 0.1
        d.score_thr, d.iou_thr, d.max_per_img = 0.05, 0.5, 5
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    L.hrf_bbox_detect(make(), ws, ws.numel(), dets, lab, cnt, s)
    for kw in (dict(R=2049), dict(R=0), dict(num_classes=17), dict(num_classes=0), dict(num_stages=5), dict(max_per_img=0), dict(score_thr=-0.1),
               dict(score_thr=1.5), dict(iou_thr=0.0), dict(iou_thr=1.5), dict(iou_thr=float('nan')), dict(ld_logits=C), dict(ld_deltas=3),
               dict(rois=None), dict(deltas=None), dict(img_shape=None), dict(B=0)):
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_bbox_detect(make(**kw), ws, ws.numel(), dets, lab, cnt, s)
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
        L.hrf_bbox_detect(make(), ws, ws.numel() - 1, dets, lab, cnt, s)
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
        L.hrf_bbox_detect(make(), ws, ws.numel(), dets, None, cnt, s)
    assert L.hrf_bbox_detect_workspace_bytes(2, 2049, 3) == 0 and L.hrf_bbox_detect_workspace_bytes(2, 8, 17) == 0
    with pytest.raises(NotImplementedError):
        roi_head.bbox_detect(torch.zeros(2 * 2049, 5, device=dev), None, [torch.zeros(2 * 2049, 4, device=dev)], torch.zeros(2 * 2049, 4, device=dev),
                             STDS, SHAPES, 2, 3, 0.05, 0.5, 10)


def test_detect_refusals_emul():
    _detect_refusals('emul')


@pytest.mark.gpu
def test_detect_refusals_gpu():
    _detect_refusals('hip')


def test_fc_route_rule(monkeypatch):
    """the default route: hrf_fc below 256 workgroups of the hrf_rowgemm launch (where it measured faster), HRF_FC_ROUTE overrides"""
    from hrfuser_amd import roi_head
    monkeypatch.delenv('HRF_FC_ROUTE', raising=False)
    assert [roi_head.fc_route(M, 1024) for M in (1, 200, 1000, 2000, 3968, 3969, 4000)] == ['fc'] * 5 + ['rowgemm'] * 2
    monkeypatch.setenv('HRF_FC_ROUTE', 'rowgemm')
    assert roi_head.fc_route(200, 1024) == 'rowgemm'
    monkeypatch.setenv('HRF_FC_ROUTE', 'fc')
    assert roi_head.fc_route(4000, 1024) == 'fc'
    monkeypatch.setenv('HRF_FC_ROUTE', 'eager')
    with pytest.raises(ValueError):
        roi_head.fc_route(200, 1024)
