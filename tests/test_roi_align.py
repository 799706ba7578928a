"""Multi-level RoIAlign (csrc/hrf_roi.h: hrf_roi_align_fwd / _bwd; hrfuser_amd/roi.py: SingleRoIExtractor, roi_align) against a
literal fp64 restatement of mmcv 1.3.17 RoIAlign(aligned=True, avg, sampling_ratio=0) + map_roi_levels
(hrfuser_amd.testing.roi_extract_ref; its backward = torch.autograd of it), through the C ABI on the CPU emulator and on the GPU.
mmcv is not installed: parity against real mmcv is unpinned; the restatement itself is pinned against
F.grid_sample + avg_pool2d here (test_restatement_against_grid_sample).

Pyramid of a 64 x 96 image (16x24, 8x12, 4x6, 2x3 at strides 4..32, B = 2), 256 channels and a narrow 12, one case with a row
pitch ld > C.  Boxes: 64 seeded draws (none within 1e-3 relative of a level boundary, so a last-bit difference of sqrt / log2
cannot move one) plus fixed ones: the exact boundaries 56 / 112 / 224 / 448, zero area, thinner than a pixel, over each border,
the whole image and twice it, outside the image within a pixel of the border and beyond.

Bound of the kernel tests: max|out - want| / max|want| < 2e-5, the bound of the sibling kernel tests (test_ffn_eval.py,
test_bottleneck_eval.py): a bin averages at most a few hundred fp32 products; a wrong corner, a dropped sample, a missing -0.5, a
wrong count or a wrong level is an error of order 0.1 .. 1.  The backward is held to the same bound per level."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import load_cfgs, relmax, use_backend
from hrfuser_amd import _lib
from hrfuser_amd.testing import roi_align_ref, roi_extract_ref, roi_level_ref, roi_samples

STRIDES = [4, 8, 16, 32]
SCALES = tuple(1.0 / s for s in STRIDES)
SIZES = [(16, 24), (8, 12), (4, 6), (2, 3)]
B, IMG_H, IMG_W = 2, 64, 96
SEED = 7
BOUND = 2e-5
ROI_CFG = dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
               out_channels=256, featmap_strides=[4, 8, 16, 32])

FIXED = [
    [0, 3, 2, 59, 58], [1, 3, 2, 115, 114], [0, 3, 2, 227, 226], [1, 3, 2, 451, 450],       # sides 56, 112, 224, 448: levels 0..3
    [0, 10, 10, 10, 10],                                                                      # zero area
    [1, 30, 12, 31.5, 52],                                                                    # thinner than a feature pixel in x only
    [0, -6, 10, 30, 40], [1, 70, 10, 102, 40], [0, 20, -5, 50, 20], [1, 20, 45, 50, 70],      # over the four borders
    [0, 0, 0, 96, 64], [1, -48, -32, 144, 96],                                                # the whole image, twice its size
    [0, 97, 10, 99.5, 40], [1, -5, 10, -2, 40], [0, 20, 65, 50, 67.5],                        # outside, within a feature pixel of the border
    [1, 104, 10, 110, 40], [0, -12, 10, -7, 40], [1, 20, -20, 50, -8],                        # outside, beyond it
]


@functools.lru_cache(None)
def _boxes():
    """-> (rois (K,5) fp32, draws, rejected)"""
    g = torch.Generator().manual_seed(SEED)
    rows, draws, rejected = [], 0, 0
    while len(rows) < 64:
        draws += 1
        u = torch.rand(5, generator=g).tolist()
        s = math.exp(math.log(10.0) + u[0] * (math.log(600.0) - math.log(10.0)))
        a = math.exp(-0.7 + 1.4 * u[1])
        w, h = s * math.sqrt(a), s / math.sqrt(a)
        cx, cy = -10 + u[2] * (IMG_W + 20), -10 + u[3] * (IMG_H + 20)
        box = torch.tensor([float(len(rows) % B), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dtype=torch.float32)
        sc = float(torch.sqrt((box[3] - box[1]) * (box[4] - box[2]))) / 56.0
        if any(abs(sc / t - 1.0) < 1e-3 for t in (2.0, 4.0, 8.0)):
            rejected += 1
            continue
        rows.append(box)
    rois = torch.cat([torch.stack(rows), torch.tensor(FIXED, dtype=torch.float32)])
    return rois, draws, rejected


@functools.lru_cache(None)
def _maps(C):
    """the pyramid: NCHW fp32 maps (contiguous)"""
    g = torch.Generator().manual_seed(1000 + C)
    return tuple(torch.randn(B, C, h, w, generator=g) for h, w in SIZES)


def _nhwc(C, dev, ld=None):
    out = []
    for m in _maps(C):
        t = m.permute(0, 2, 3, 1).contiguous()
        if ld is not None:
            big = torch.full(t.shape[:3] + (ld,), float('nan'))
            big[..., :C] = t
            t = big.to(dev)[..., :C]
        out.append(t.to(dev))
    return out


@functools.lru_cache(None)
def _ref(C):
    """-> (want (K,C,7,7) fp64, dout (K,C,7,7) fp32, gradients per level NCHW fp64)"""
    rois = _boxes()[0]
    feats = [m.double().requires_grad_(True) for m in _maps(C)]
    want = roi_extract_ref(feats, rois, STRIDES)
    dout = torch.randn(want.shape, generator=torch.Generator().manual_seed(2000 + C))
    grads = torch.autograd.grad(want, feats, dout.double(), allow_unused=True)
    grads = tuple(torch.zeros_like(f) if g is None else g for f, g in zip(feats, grads))
    return want.detach(), dout, grads


def _lay(t, layout):
    """(K,C,7,7) <-> the kernel's out_layout"""
    return t if layout == 0 else t.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------- the box set and the restatement (CPU)
def test_box_set():
    rois, draws, rejected = _boxes()
    assert rejected < 0.02 * draws, (draws, rejected)
    lv = roi_level_ref(rois, 4)
    for l in range(4):
        assert int((lv == l).sum()) >= 4, (l, lv.tolist())
    assert set(rois[:, 0].tolist()) == {0.0, 1.0}
    k = 64
    assert lv[k:k + 4].tolist() == [0, 1, 2, 3]                     # the exact boundaries 56, 112, 224, 448
    assert int(lv[k + 4]) == 0                                      # zero area


def test_restatement_against_grid_sample():
    """the literal loop against F.grid_sample(bilinear, border, align_corners=True) at the same sample positions + avg_pool2d,
    on boxes whose samples all lie inside [0, H-1] x [0, W-1]; fp64, 2e-15 measured."""
    g = torch.Generator().manual_seed(3)
    H, W, C = 16, 24, 5
    feat = torch.randn(2, C, H, W, generator=g, dtype=torch.float64)
    n = 0
    for _ in range(200):
        u = torch.rand(5, generator=g).tolist()
        w, h = 4 + u[0] * 60, 4 + u[1] * 40
        x1, y1 = 2 + u[2] * (4 * W - 8 - w), 2 + u[3] * (4 * H - 8 - h)
        box = [x1, y1, x1 + w, y1 + h]
        ys, xs, count = roi_samples(box, 0.25, H, W)
        fy, fx = [v for r in ys for v in r], [v for r in xs for v in r]
        if min(fy) < 0 or max(fy) > H - 1 or min(fx) < 0 or max(fx) > W - 1:
            continue
        n += 1
        b = int(u[4] * 2)
        gy = torch.tensor(fy, dtype=torch.float64) * 2 / (H - 1) - 1
        gx = torch.tensor(fx, dtype=torch.float64) * 2 / (W - 1) - 1
        grid = torch.stack(torch.meshgrid(gx, gy, indexing='xy'), -1)[None]
        smp = F.grid_sample(feat[b:b + 1], grid, mode='bilinear', padding_mode='border', align_corners=True)
        want = F.avg_pool2d(smp, (len(ys[0]), len(xs[0])))[0]
        got = roi_align_ref(feat, torch.tensor([[float(b)] + box], dtype=torch.float64), 0.25)[0]
        assert float((got - want).abs().max()) < 1e-13, box
    assert n >= 50, n


def test_level_mapping():
    from hrfuser_amd.roi import SingleRoIExtractor
    ex = SingleRoIExtractor(**{k: v for k, v in ROI_CFG.items() if k != 'type'})
    rois = _boxes()[0]
    lv = roi_level_ref(rois, 4)
    s = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
    ok = ~torch.isnan(s)
    assert torch.equal(ex.map_roi_levels(rois, 4)[ok], lv[ok])
    sides = torch.tensor([[0, 0, 0, s_, s_] for s_ in (56.0, 112.0, 224.0, 448.0, 0.0)])
    assert ex.map_roi_levels(sides, 4).tolist() == [0, 1, 2, 3, 0]
    assert ex.map_roi_levels(sides, 2).tolist() == [0, 1, 1, 1, 0]


# ----------------------------------------------------------------------------- 1. forward parity
def _forward(backend, C, layout, ld):
    from hrfuser_amd import roi
    dev = use_backend(backend)
    rois = _boxes()[0]
    want = _ref(C)[0]
    out = roi.roi_forward(_nhwc(C, dev, ld), rois.to(dev), SCALES, 56.0, layout).cpu()
    out = out if layout == 0 else out.permute(0, 3, 1, 2)
    err = relmax(out, want)
    print(f'roi_align fwd {backend} C={C} layout={layout} ld={ld}: err {err:.3e} (max|want| {float(want.abs().max()):.2f})')
    assert err < BOUND, err
    # every row belongs to ITS level: the restatement with the level forced wrong does not match
    lv = roi_level_ref(rois, 4)
    wrong = roi_extract_ref([m.double() for m in _maps(C)], rois, STRIDES, levels=(lv + 1) % 4)
    big = float(want.abs().max())
    for k in range(rois.shape[0]):
        if float(want[k].abs().max()) == 0.0 and float(wrong[k].abs().max()) == 0.0:
            continue
        assert float((out[k].double() - wrong[k]).abs().max()) > 1e-3 * big, k
        assert float((out[k].double() - want[k]).abs().max()) < BOUND * big, k


FWD_CASES = [(256, 0, None), (256, 1, None), (12, 0, None), (12, 1, None), (12, 0, 20)]


@pytest.mark.parametrize('C,layout,ld', FWD_CASES)
def test_forward_emul(C, layout, ld):
    _forward('emul', C, layout, ld)


@pytest.mark.gpu
@pytest.mark.parametrize('C,layout,ld', FWD_CASES)
def test_forward_gpu(C, layout, ld):
    _forward('hip', C, layout, ld)


# ----------------------------------------------------------------------------- 3. backward parity per level
def _backward(backend, C, layout, ld):
    from hrfuser_amd import roi
    dev = use_backend(backend)
    rois = _boxes()[0]
    _, dout, grads = _ref(C)
    maps = _nhwc(C, dev, ld)
    g = torch.Generator().manual_seed(77)

    def targets(fill):
        out = []
        for m in maps:
            t = torch.zeros(m.shape[:3] + (m.stride(2),))
            if fill:
                t.normal_(generator=g)
            out.append(t.to(dev)[..., :C])
        return out
    d = _lay(dout, layout).to(dev)
    dz = targets(False)
    roi.roi_backward(maps, dz, rois.to(dev), SCALES, d, 56.0, layout)
    for l in range(4):
        err = relmax(dz[l].cpu().permute(0, 3, 1, 2), grads[l])
        print(f'roi_align bwd {backend} C={C} layout={layout} ld={ld} level {l}: err {err:.3e} (max|want| {float(grads[l].abs().max()):.2f})')
        assert err < BOUND, (l, err)
    # accumulation: a pre-filled target ends up as pre-fill + gradient
    dp = targets(True)
    pre = [t.cpu().clone() for t in dp]
    roi.roi_backward(maps, dp, rois.to(dev), SCALES, d, 56.0, layout)
    for l in range(4):
        err = relmax(dp[l].cpu().permute(0, 3, 1, 2), pre[l].double().permute(0, 3, 1, 2) + grads[l])
        assert err < BOUND, (l, err)
    # a level no box maps to keeps its pre-fill, bit for bit (and the others their full gradient: a box adds into ITS level only)
    lv = roi_level_ref(rois, 4)
    keep = lv != 2
    dq = targets(True)
    pre = [t.cpu().clone() for t in dq]
    roi.roi_backward(maps, dq, rois[keep].to(dev), SCALES, d[keep.to(dev)].contiguous(), 56.0, layout)
    assert torch.equal(dq[2].cpu(), pre[2])
    for l in (0, 1, 3):
        assert relmax(dq[l].cpu().permute(0, 3, 1, 2), pre[l].double().permute(0, 3, 1, 2) + grads[l]) < BOUND, l


BWD_CASES = [(256, 0, None), (12, 1, None), (12, 0, 20)]


@pytest.mark.parametrize('C,layout,ld', BWD_CASES)
def test_backward_emul(C, layout, ld):
    _backward('emul', C, layout, ld)


@pytest.mark.gpu
@pytest.mark.parametrize('C,layout,ld', BWD_CASES + [(256, 1, None)])
def test_backward_gpu(C, layout, ld):
    _backward('hip', C, layout, ld)


# ----------------------------------------------------------------------------- 4. hostile boxes (emulator only: a wrong guard would be a hang on a GPU)
def test_hostile_boxes_emul():
    from hrfuser_amd import roi
    dev = use_backend('emul')
    L = _lib.lib()
    C = 12
    rois = _boxes()[0]
    K = rois.shape[0]
    inf, nan = float('inf'), float('nan')
    hostile = []
    for v in (1e9, -1e9, 1e30, -1e30, inf, -inf, nan):
        for pos in range(1, 5):
            r = [0.0, 10.0, 10.0, 40.0, 40.0]
            r[pos] = v
            hostile.append(r)
    hostile += [[0.0, -1e9, -1e9, 1e9, 1e9], [1.0, -inf, -inf, inf, inf], [1.0, nan, nan, nan, nan]]
    hostile += [[bi, 10.0, 10.0, 40.0, 40.0] for bi in (-1.0, float(B), 1e9, nan, -inf)]
    hostile = torch.tensor(hostile, dtype=torch.float32)
    nh = hostile.shape[0]
    # interleave: hostile rows in front, in the middle and behind
    mixed = torch.cat([hostile[:nh // 3], rois[:K // 2], hostile[nh // 3:2 * nh // 3], rois[K // 2:], hostile[2 * nh // 3:]])
    is_h = torch.cat([torch.ones(nh // 3), torch.zeros(K // 2), torch.ones(2 * nh // 3 - nh // 3), torch.zeros(K - K // 2),
                      torch.ones(nh - 2 * nh // 3)]).bool()
    maps = _nhwc(C, dev)
    clean = roi.roi_forward(maps, rois, SCALES, 56.0, 0)
    out = roi.roi_forward(maps, mixed, SCALES, 56.0, 0, out=torch.full((mixed.shape[0], C, 7, 7), nan))
    assert bool((out[is_h] == 0).all())
    assert torch.equal(out[~is_h], clean)
    dout = torch.randn(mixed.shape[0], C, 7, 7, generator=torch.Generator().manual_seed(5))
    da = [torch.zeros_like(m) for m in maps]
    db = [torch.zeros_like(m) for m in maps]
    roi.roi_backward(maps, da, mixed, SCALES, dout, 56.0, 0)
    roi.roi_backward(maps, db, rois, SCALES, dout[~is_h].contiguous(), 56.0, 0)
    for l in range(4):
        assert bool(torch.isfinite(da[l]).all())
        assert relmax(da[l], db[l]) < 1e-6, l                      # (the emulator's blocks run on several threads: the order of the adds)
    # trip counts are bounded by the MAP: boxes far larger than the map that pass the coordinate bound (|coord / stride| <= 2^20)
    huge = torch.tensor([[0, -1e5, -1e5, 1e5, 1e5], [1, -3e7, -3e7, 3e7, 3e7], [0, -3e7, 10, 3e7, 11], [1, 40, -3e7, 41, 3e7],
                         [0, 1e5, 1e5, 3e7, 3e7], [1, -3e7, -3e7, -1e5, -1e5]], dtype=torch.float32)
    slack = _lib._header_int('HRF_ROI_AXIS_SLACK', -1)
    assert slack > 0
    fn = L._dll.hrf_roi_debug_iters
    fn.restype, fn.argtypes = None, [ctypes.c_void_p, ctypes.c_int]
    cnt = (ctypes.c_long * 2)()
    for which in ('fwd', 'bwd'):
        for rs in (huge, mixed):
            fn(None, 1)
            if which == 'fwd':
                o = roi.roi_forward(maps, rs, SCALES, 56.0, 0)
                assert bool(torch.isfinite(o).all())
            else:
                dd = [torch.zeros_like(m) for m in maps]
                roi.roi_backward(maps, dd, rs, SCALES, torch.ones(rs.shape[0], C, 7, 7), 56.0, 0)
                assert all(bool(torch.isfinite(t).all()) for t in dd)
            fn(ctypes.addressof(cnt), 0)
            # documented constant (include/hrfuser_hip.h): per box and axis of n pixels at most 2 n + HRF_ROI_AXIS_SLACK sample
            # iterations, i.e. K * c * (H + W) with c = 2 + 2 * HRF_ROI_AXIS_SLACK / (H + W) of the largest level
            Hm, Wm = SIZES[0]
            assert 0 < cnt[0] <= rs.shape[0] * (2 * (Hm + Wm) + 2 * slack), (which, cnt[0])
            assert cnt[1] <= rs.shape[0] * (Hm + 14) * (Wm + 14), (which, cnt[1])
    lv = roi_level_ref(huge, 4)
    assert lv.tolist() == [3] * 6


# ----------------------------------------------------------------------------- 5. ABI refusals
def _abi(backend):
    from hrfuser_amd import roi
    dev = use_backend(backend)
    L = _lib.lib()
    s = _lib.stream_ptr() if backend == 'hip' else 0
    C = 12
    rois = _boxes()[0][:8].contiguous().to(dev)
    maps = _nhwc(C, dev)
    nan = float('nan')
    out = torch.full((8, C, 7, 7), nan, device=dev)
    dmaps = [torch.full_like(m, nan) for m in maps]
    dout = torch.ones(8, C, 7, 7, device=dev)

    def untouched():
        if backend == 'hip':
            torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and all(bool(torch.isnan(d).all()) for d in dmaps)

    def refused(lv, sup):
        assert L.hrf_roi_align_supported(*sup) == 0, sup
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_roi_align_fwd(lv, rois, 8, out, 0, s)
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_roi_align_bwd(lv, rois, 8, dout, 0, s)
        untouched()
    assert L.hrf_roi_align_supported(256, 7, 4) == 1 and L.hrf_roi_align_supported(12, 7, 1) == 1
    for nl in (0, 5):
        lv = roi._levels(maps, dmaps, SCALES, 56.0)
        lv.num_levels = nl
        refused(lv, (C, 7, nl))
    lv = roi._levels(maps, dmaps, SCALES, 56.0)
    lv.C = 6
    refused(lv, (6, 7, 4))
    lv = roi._levels(maps, dmaps, SCALES, 56.0)
    lv.C = 260                                                      # wider than the kernel's staging
    refused(lv, (260, 7, 4))
    lv = roi._levels(maps, dmaps, SCALES, 56.0)
    lv.pooled = 14
    refused(lv, (C, 14, 4))
    # K = 0: HRF_OK, nothing touched
    lv = roi._levels(maps, dmaps, SCALES, 56.0)
    L.hrf_roi_align_fwd(lv, rois, 0, out, 0, s)
    L.hrf_roi_align_bwd(lv, rois, 0, dout, 0, s)
    untouched()
    # deterministic mode: the backward is refused, the forward is the same bits
    plain = roi.roi_forward(maps, rois, SCALES, 56.0, 0)
    L.hrf_set_deterministic(1)
    try:
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_roi_align_bwd(lv, rois, 8, dout, 0, s)
        untouched()
        det = roi.roi_forward(maps, rois, SCALES, 56.0, 0)
    finally:
        L.hrf_set_deterministic(0)
    assert torch.equal(det.cpu(), plain.cpu())


def test_abi_emul():
    _abi('emul')


@pytest.mark.gpu
def test_abi_gpu():
    _abi('hip')


# ----------------------------------------------------------------------------- 6. the module
def test_module_builds_and_refuses():
    from hrfuser_amd.registry import ROI_EXTRACTORS
    from hrfuser_amd.roi import SingleRoIExtractor, roi_align
    ex = ROI_EXTRACTORS.build(dict(ROI_CFG))
    assert isinstance(ex, SingleRoIExtractor) and ex.num_inputs == 4
    assert len(ex.state_dict()) == 0 and len(list(ex.parameters())) == 0
    ROI_EXTRACTORS.build(dict(ROI_CFG, roi_layer=dict(type='RoIAlign', output_size=(7, 7), sampling_ratio=0, pool_mode='avg', aligned=True)))
    for bad in (dict(type='RoIPool', output_size=7), dict(type='RoIAlign', output_size=14, sampling_ratio=0),
                dict(type='RoIAlign', output_size=7, sampling_ratio=2), dict(type='RoIAlign', output_size=7, sampling_ratio=0, pool_mode='max'),
                dict(type='RoIAlign', output_size=7, sampling_ratio=0, aligned=False)):
        with pytest.raises(NotImplementedError):
            ROI_EXTRACTORS.build(dict(ROI_CFG, roi_layer=bad))
    use_backend('emul')
    feats = [m[:, :12] for m in _maps(12)]
    rois = _boxes()[0][:4]
    with pytest.raises(NotImplementedError, match='roi_scale_factor'):
        ex(feats, rois, roi_scale_factor=1.2)
    for kw in (dict(output_size=14), dict(output_size=7, sampling_ratio=2), dict(output_size=7, pool_mode='max'), dict(output_size=7, aligned=False)):
        with pytest.raises(NotImplementedError):
            roi_align(feats[0], rois, spatial_scale=0.25, **kw)
    use_backend('hip')                                              # the product library, whatever ran before
    try:
        with pytest.raises(_lib.HRFuserHipError):                   # a CPU tensor on the product library: refused, no fallback
            roi_align(feats[0].cpu(), rois.cpu(), 7, 0.25)
    finally:
        use_backend('emul')


def _module(backend, C):
    from hrfuser_amd.registry import ROI_EXTRACTORS
    from hrfuser_amd.roi import roi_align
    dev = use_backend(backend)
    ex = ROI_EXTRACTORS.build(dict(ROI_CFG, out_channels=C))
    rois = _boxes()[0].to(dev)
    want, dout, grads = _ref(C)
    plain = [m.to(dev).requires_grad_(True) for m in _maps(C)]                                  # contiguous NCHW: copied once
    cl = [m.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for m in _maps(C)]     # used in place
    fifth = torch.full((B, C, 1, 2), float('nan'), device=dev)
    o_plain = ex(plain, rois)
    o_cl = ex(tuple(cl) + (fifth,), rois)                           # five maps given: the fifth is ignored
    assert tuple(o_cl.shape) == (rois.shape[0], C, 7, 7)
    assert torch.equal(o_plain, o_cl)
    assert relmax(o_cl, want) < BOUND
    got = torch.autograd.grad(o_cl, cl, dout.to(dev))
    for l in range(4):
        assert relmax(got[l], grads[l]) < BOUND, l
    # the single-level call shape of mmcv.ops.roi_align: every box on the one map
    lv1 = roi_level_ref(_boxes()[0], 4) == 1
    o1 = roi_align(cl[1], rois[lv1.to(dev)], 7, 1.0 / 8)
    assert relmax(o1, want[lv1]) < BOUND


def test_module_emul():
    _module('emul', 12)


@pytest.mark.gpu
def test_module_gpu():
    _module('hip', 256)


def test_extract_nhwc_tape_emul():
    """the tape-level entry on runtime.Act's: forward in place, backward closure adds into act.grad (created zeroed)"""
    from hrfuser_amd import runtime as R
    from hrfuser_amd.registry import ROI_EXTRACTORS
    from hrfuser_amd.testing import BlockHarness
    dev = use_backend('emul')
    C = 12
    ex = ROI_EXTRACTORS.build(dict(ROI_CFG, out_channels=C))
    want, dout, grads = _ref(C)
    rois = _boxes()[0]
    h = BlockHarness(torch.nn.Identity(), lambda ctx, blk, acts: ex.extract_nhwc(ctx, acts, rois, out_layout=1))
    ins = [m.clone().requires_grad_(True) for m in _maps(C)]
    out = h(*ins)[0]                                                # harness outputs: NHWC Act -> permute(0, 3, 1, 2) view
    got_out = out.permute(0, 2, 3, 1).reshape(rois.shape[0], 7, 7, C).permute(0, 3, 1, 2)
    assert relmax(got_out, want) < BOUND
    gin = torch.autograd.grad(out, ins, _lay(dout, 1).permute(0, 3, 1, 2))
    for l in range(4):
        assert relmax(gin[l], grads[l]) < BOUND, l


def test_profile_rows_emul():
    """profiling.work_model names both launches and prices them by traffic (no unnamed kernel in a profile)"""
    from hrfuser_amd import profiling, roi
    dev = use_backend('emul')
    C = 12
    maps, rois = _nhwc(C, dev), _boxes()[0]
    K = rois.shape[0]
    real = _lib.lib
    prof = profiling.ProfLib(real(), timing=False)
    _lib.lib = lambda: prof
    try:
        out = roi.roi_forward(maps, rois, SCALES, 56.0, 0)
        roi.roi_backward(maps, [torch.zeros_like(m) for m in maps], rois, SCALES, torch.ones_like(out), 56.0, 0)
    finally:
        _lib.lib = real
    names = [r[0] for r in prof.records]
    assert names == ['hrf_roi_align_fwd', 'hrf_roi_align_bwd']
    for (name, desc, _), key in zip(prof.records, ('roi_align_fwd_kernel', 'roi_align_bwd_kernel')):
        k, fl, by = profiling.work_model(name, desc)
        assert k == key and fl > 0 and by > 4.0 * K * 49 * C


# ----------------------------------------------------------------------------- 7. forward repeatability on the GPU
@pytest.mark.gpu
def test_forward_repeatable_gpu():
    from hrfuser_amd import roi
    dev = use_backend('hip')
    maps, rois = _nhwc(256, dev), _boxes()[0].to(dev)
    a = roi.roi_forward(maps, rois, SCALES, 56.0, 0)
    b = roi.roi_forward(maps, rois, SCALES, 56.0, 0)
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 9. end to end on the GPU
@pytest.mark.gpu
def test_end_to_end_gpu(monkeypatch):
    import copy
    import hrfuser_oracle as O
    from hrfuser_amd import runtime as R
    from hrfuser_amd.detector import FeatureExtractor
    monkeypatch.setenv('HRF_MODULE_GRAPH', '0')                     # eager launches: the whole chain is captured below
    dev = use_backend('hip')
    cfg = load_cfgs()['t_nus']
    torch.manual_seed(0)
    fx = FeatureExtractor(copy.deepcopy(cfg), dict(type='HRFPN', in_channels=[18, 36, 72, 144], out_channels=256), dict(ROI_CFG))
    O.seeded_fill_(fx.backbone, 0)
    fx.neck.init_weights()
    fx.to(dev).eval()
    x, mods = O.seeded_inputs(1, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    rois = _boxes()[0].clone()
    rois[:, 0] = 0
    rois = rois.to(dev)
    kw = dict(zip(('lidar_img', 'radar_img', 'gated_img'), mods))
    with torch.no_grad():
        feats = fx.extract_feat(x, mods)
        assert len(feats) == 5
        eager = fx.extract_roi_feats(x, rois, **kw)
        want = roi_extract_ref([f.double().cpu() for f in feats[:4]], rois.cpu(), STRIDES)
        err = relmax(eager, want)
        print(f'end to end: err {err:.3e}')
        assert err < BOUND, err
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fx.extract_roi_feats(x, rois, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with R.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
            cap = fx.extract_roi_feats(x, rois, **kw)
        cap.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap, eager)
