"""The backward of the cascade bbox head from the public interface down: Shared2FCBBoxHead.run_train / run_backward /
forward_autograd, CascadeRoIHead.losses_nhwc on the tape, a captured forward + backward, FeatureExtractor.roi_loss_backward.

Reference: fp64 torch.autograd through the literal restatements of hrfuser_amd.testing (roi_extract_ref -> bbox_head_ref ->
bbox_loss_ref).  Rule (test_roi_loss.py's): per tensor, relmax(HIP, fp64) <= 4 x relmax(the same restatement in fp32, fp64) on the
same inputs; both figures are printed.  The cascade comparison feeds the restatement every stage's OWN kernel inputs (the sampled
rows, labels and targets the stage produced, as test_roi_loss._chain does): the later stages of cascade_forward_train_ref sample
from boxes its fp32 torch decode refined, which are not bit-equal to hrf_bbox_refine's, so its later records name other rows;
its first-stage record (identical inputs) must name the same rows and is asserted to."""
import copy
import functools

import pytest
import torch

from helpers import relmax, use_backend
from hrfuser_amd import _lib
from hrfuser_amd.testing import BlockHarness, bbox_head_ref, bbox_loss_ref, cascade_forward_train_ref, roi_extract_ref
from test_roi_loss import B, CASES, NC, SHAPES, SIZES, STDS, STRIDES, _as_i32, _build, _draw_gts, _inputs

NUM = 48                                                            # test_roi_loss.TRAIN: 48 rows per image, 12 positives
WEIGHTS = [1.0, 0.5, 0.25]
PARAMS = ('shared_fcs.0.weight', 'shared_fcs.0.bias', 'shared_fcs.1.weight', 'shared_fcs.1.bias', 'fc_cls.weight', 'fc_cls.bias', 'fc_reg.weight',
          'fc_reg.bias')


def _gate(tag, got, r32, r64):
    e, e_ref = relmax(got, r64), relmax(r32, r64)
    print(f'{tag}: {got.numel()} values, HIP vs fp64 {e:.3e}, fp32 restatement vs fp64 {e_ref:.3e}')
    assert e <= 4.0 * e_ref, (tag, e, e_ref)


# ----------------------------------------------------------------------------- 1. the head alone
@functools.lru_cache(None)
def _head_problem(C, F, M):
    """-> (head, x (M,C,7,7), d (M, out_pitch) with junk in the pad columns, {dtype: (cls, reg, dx, {param: grad})})"""
    from hrfuser_amd import HEADS
    torch.manual_seed(31)
    hd = HEADS.build(dict(type='Shared2FCBBoxHead', in_channels=C, fc_out_channels=F, num_classes=NC, reg_class_agnostic=True))
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for p in hd.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.randn(M, C, 7, 7, generator=g).clamp_(min=0)
    d = torch.randn(M, hd.out_pitch, generator=g)
    d[M - M // 4:, :NC + 5] = 0                                      # padding rows of a loss gradient
    ref = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in hd.state_dict().items()}
        xr = x.detach().clone().to(dt).requires_grad_(True)
        cls, reg = bbox_head_ref(xr, sd)
        torch.autograd.backward([cls, reg], [d[:, :NC + 1].to(dt), d[:, NC + 1:NC + 5].to(dt)])
        ref[dt] = (cls.detach(), reg.detach(), xr.grad, {k: sd[k].grad for k in PARAMS})
    return hd, x, d, ref


def _head(backend, C, F, M, nhwc):
    dev = use_backend(backend)
    hd0, x, d, ref = _head_problem(C, F, M)
    hd = copy.deepcopy(hd0).to(dev)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    x2d = (x.permute(0, 2, 3, 1) if nhwc else x).contiguous().reshape(M, -1).to(dev)
    tag = f'head {backend} C={C} F={F} M={M} nhwc={nhwc}'
    with torch.no_grad():
        want = hd.run(x2d, nhwc=nhwc)
        out, saved = hd.run_train(x2d, nhwc=nhwc)
    assert torch.equal(out, want)                                   # the same launches: the same bits
    assert saved['x'] is x2d and saved['h1'].shape == (M, F) and saved['h2'].shape == (M, F)
    _gate(tag + ' cls', out[:, :NC + 1].cpu(), r32[0], r64[0])
    dd = d.to(dev)
    with torch.no_grad():
        dx = hd.run_backward(saved, dd)
    sd = dict(hd.named_parameters())
    once = {k: sd[k].grad.clone().cpu() for k in PARAMS}
    for k in PARAMS:                                                # in the parameter's own shape and order (fc1: (c, y, x) columns)
        assert once[k].shape == r64[3][k].shape
        _gate(f'{tag} {k}.grad', once[k], r32[3][k], r64[3][k])
    dx = dx.cpu().reshape(M, 7, 7, C).permute(0, 3, 1, 2) if nhwc else dx.cpu().reshape(M, C, 7, 7)
    _gate(tag + ' dx', dx, r32[2], r64[2])
    # the wrong column order of fc1's gradient would not pass: the (y, x, c) arrangement of the reference is far outside the gate
    wrong = r64[3]['shared_fcs.0.weight'].reshape(F, C, 49).permute(0, 2, 1).reshape(F, -1)
    assert relmax(once['shared_fcs.0.weight'], wrong) > 0.1
    # a second backward adds: .grad doubles (2 g is exact), and need_dx = False returns nothing
    with torch.no_grad():
        assert hd.run_backward(saved, dd, need_dx=False) is None
    for k in PARAMS:
        assert torch.equal(sd[k].grad.cpu(), 2.0 * once[k]), k
    # forward_autograd: the same gradients through torch.autograd, x.grad in x's layout
    hd2 = copy.deepcopy(hd0).to(dev)
    xin = (x.permute(0, 2, 3, 1).contiguous() if nhwc else x.clone()).to(dev).requires_grad_(True)
    cls, reg = hd2.forward_autograd(xin, layout='nhwc' if nhwc else 'nchw')
    assert cls.grad_fn is not None and reg.grad_fn is not None and torch.equal(cls, out[:, :NC + 1]) and torch.equal(reg, out[:, NC + 1:NC + 5])
    ((cls * dd[:, :NC + 1]).sum() + (reg * dd[:, NC + 1:NC + 5]).sum()).backward()
    gx = xin.grad.cpu().permute(0, 3, 1, 2) if nhwc else xin.grad.cpu()
    assert xin.grad.shape == xin.shape
    _gate(tag + ' autograd x.grad', gx, r32[2], r64[2])
    for k, p in hd2.named_parameters():
        _gate(f'{tag} autograd {k}.grad', p.grad.cpu(), r32[3][k], r64[3][k])


@pytest.mark.parametrize('nhwc', [False, True])
def test_head_emul(nhwc):
    _head('emul', 16, 64, 70, nhwc)


@pytest.mark.gpu
@pytest.mark.parametrize('nhwc', [False, True])
def test_head_gpu(nhwc):
    _head('hip', 256, 1024, 130, nhwc)


# ----------------------------------------------------------------------------- 2. the cascade on the tape
FS = 16                                                             # finest_scale: boxes of 12 .. 120 px spread over three levels
CASE = 'few'                                                        # 40 / 25 proposals + 3 / 2 gts per image: fewer candidates than 48 rows


@functools.lru_cache(None)
def _cascade_problem(C, F, sizes):
    torch.manual_seed(41)
    rh = _build(edit=lambda cf: cf['bbox_roi_extractor'].update(finest_scale=FS), in_channels=C, fc_out=F)
    g = torch.Generator().manual_seed(42)
    with torch.no_grad():
        for i, h in enumerate(rh.bbox_head):                         # logits ~ N(0, 1), deltas * stds ~ 0.05: as a trained head's
            h.fc_cls.weight.mul_(40.0)
            h.fc_reg.weight.mul_(40.0 / STDS[i][0] * 0.1)
            h.fc_cls.bias.copy_(0.5 * torch.randn(NC + 1, generator=g))
    feats = [torch.randn(B, C, h, w, generator=g) for h, w in sizes]
    inp = _inputs(CASE)
    c = CASES[CASE]
    keys = [_as_i32(torch.randint(0, 1 << 32, (B, c['gmax'] + r), generator=g, dtype=torch.long)) for r in (c['R'], NUM, NUM)]
    return rh, feats, inp, keys


def _run_tape(rh, feats_dev, args, keys, out_layout=1):
    """forward on a recording ctx, then the tape -> (values, d_out list, stages, pyramid gradients NHWC)"""
    box = {}

    def runner(ctx, blk, acts):
        box['stages'] = []
        box['vals'], box['d'] = rh._losses_nhwc(ctx, acts, *args, stages=box['stages'], keys=keys, out_layout=out_layout)
        return acts
    h = BlockHarness(torch.nn.Identity(), runner)
    ctx, _, srcs = h._execute(tuple(feats_dev), True, needs=[True] * len(feats_dev))
    ctx.run_backward()
    return box['vals'], box['d'], box['stages'], [s.grad for s in srcs]


def _cascade_ref(rh0, feats, stages, dt):
    """the restatement with autograd in `dt` on the stages' own sampled rows -> ([pyramid grads NCHW], [{param: grad}] per stage)"""
    fs = [f.detach().clone().to(dt).requires_grad_(True) for f in feats]
    pg = []
    for i, sg in enumerate(stages):
        rois_s, labels, targets = (t.cpu() for t in sg['targets'][:3])
        valid = labels >= 0
        assert int(valid.sum()) < labels.numel()                    # padding rows exist
        sd = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in rh0.bbox_head[i].state_dict().items()}
        x = roi_extract_ref(fs, rois_s[valid].to(dt), STRIDES, FS)
        cls, reg = bbox_head_ref(x, sd)
        lr = bbox_loss_ref(cls, reg, labels[valid].long(), targets[valid], NC, 1.0, WEIGHTS[i], WEIGHTS[i], dt)
        torch.autograd.backward([cls, reg], [lr['d_logits'], lr['d_deltas']])
        pg.append({k: sd[k].grad for k in PARAMS})
    return [f.grad if f.grad is not None else torch.zeros_like(f) for f in fs], pg


def _cascade(backend, C, F, sizes):
    from hrfuser_amd import roi_head, rpn
    dev = use_backend(backend)
    rh0, feats, inp, keys = _cascade_problem(C, F, sizes)
    c = CASES[CASE]
    rh = copy.deepcopy(rh0).to(dev).eval()
    gt, cnt = rpn.pack_gts(inp['gts'], dev, c['gmax'])
    gl = roi_head.pack_gt_labels(inp['labels'], dev, c['gmax'])
    count = torch.tensor(inp['count'], dtype=torch.int32).to(dev)
    args = (inp['rois'].to(dev), count, gt, gl, cnt, SHAPES)
    kd = [k.to(dev) for k in keys]
    x = [f.to(dev) for f in feats]
    want_vals, want_d = rh.losses(x, *args, keys=kd)
    vals, d, stages, pgrads = _run_tape(rh, x, args, kd)
    assert torch.equal(vals, want_vals) and all(torch.equal(a, b) for a, b in zip(d, want_d))          # the same bits as `losses`
    assert all(g is not None for g in pgrads)
    # stage 0 of the literal chain samples the same rows (identical inputs)
    props = [inp['rois'].reshape(B, c['R'], 5)[b, :inp['count'][b], 1:] for b in range(B)]
    k64 = [torch.where(k < 0, k.long() + (1 << 32), k.long()) for k in keys]
    key_fn = lambda i, b, is_gt, idx: k64[i][b][torch.where(is_gt, idx, c['gmax'] + idx)]              # noqa: E731
    sds = [{k: v.detach().clone() for k, v in h.state_dict().items()} for h in rh0.bbox_head]
    cfgs = [dict(pos_iou_thr=t, neg_iou_thr=t, num=NUM, num_pos=12, stage_weight=w) for t, w in zip((0.5, 0.6, 0.7), WEIGHTS)]
    _, rec = cascade_forward_train_ref(feats, props, inp['gts'], inp['labels'], SHAPES, sds[:1], cfgs[:1], STDS, NC, STRIDES, key_fn, FS)
    t0 = [t.cpu() for t in stages[0]['targets'][:3]]
    v0 = t0[1] >= 0
    assert torch.equal(t0[0][v0], rec[0]['rois']) and torch.equal(t0[1][v0].long(), rec[0]['labels'])
    # gradients: head parameters per stage, pyramid per level
    g64, p64 = _cascade_ref(rh0, feats, stages, torch.float64)
    g32, p32 = _cascade_ref(rh0, feats, stages, torch.float32)
    for i in range(3):
        sd = dict(rh.bbox_head[i].named_parameters())
        for k in PARAMS:
            _gate(f'cascade {backend} stage {i} {k}.grad', sd[k].grad.cpu(), p32[i][k], p64[i][k])
    assert all(float(g64[l].abs().max()) > 0 for l in range(3))
    for l, g in enumerate(pgrads):                                  # (a level no box maps to: exactly zero on both sides)
        _gate(f'cascade {backend} pyramid level {l}', g.cpu().permute(0, 3, 1, 2), g32[l], g64[l])


def test_cascade_emul():
    _cascade('emul', 16, 32, tuple(SIZES))


@pytest.mark.gpu
def test_cascade_gpu():
    _cascade('hip', 16, 32, ((96, 160), (48, 80), (24, 40), (12, 20)))


def test_cascade_feature_layout_emul():
    """the (c, y, x) feature layout (no hrf_fc_bwd_cols) gives the same gradients up to the summation order of fc1"""
    from hrfuser_amd import roi_head, rpn
    dev = use_backend('emul')
    rh0, feats, inp, keys = _cascade_problem(16, 32, tuple(SIZES))
    c = CASES[CASE]
    gt, cnt = rpn.pack_gts(inp['gts'], dev, c['gmax'])
    args = (inp['rois'], torch.tensor(inp['count'], dtype=torch.int32), gt, roi_head.pack_gt_labels(inp['labels'], dev, c['gmax']), cnt, SHAPES)
    res = []
    for lay in (1, 0):
        rh = copy.deepcopy(rh0).eval()
        vals, _, _, pg = _run_tape(rh, feats, args, keys, out_layout=lay)
        res.append((vals, pg, [dict(h.named_parameters()) for h in rh.bbox_head]))
    assert relmax(res[1][0], res[0][0]) < 1e-5
    for l in range(4):
        assert relmax(res[1][1][l], res[0][1][l]) < 1e-4
    for i in range(3):
        for k in PARAMS:
            assert relmax(res[1][2][i][k].grad, res[0][2][i][k].grad) < 1e-4, (i, k)


def test_losses_nhwc_needs_train_cfg():
    bare = _build(train=False)
    with pytest.raises(NotImplementedError, match='train_cfg'):
        bare.losses_nhwc()


# ----------------------------------------------------------------------------- 3. forward + backward in one captured graph
@pytest.mark.gpu
def test_graph_gpu():
    """forward + backward captured once; after the gt contents are rewritten a replay leaves the head gradients of an eager run on
    the new contents, bit for bit (the FC backward has no atomics), and the pyramid gradient within RoIAlign's atomic spread"""
    from hrfuser_amd import roi_head, rpn
    from hrfuser_amd import runtime as R
    dev = use_backend('hip')
    rh0, feats, inp, keys = _cascade_problem(16, 32, tuple(SIZES))
    rh = copy.deepcopy(rh0).to(dev).eval()
    x = [f.to(dev) for f in feats]
    gt, cnt = rpn.pack_gts(inp['gts'], dev, 8)
    gl = roi_head.pack_gt_labels(inp['labels'], dev, 8)
    args = (inp['rois'].to(dev), torch.tensor(inp['count'], dtype=torch.int32).to(dev), gt, gl, cnt, torch.tensor(SHAPES, dtype=torch.float32).to(dev))
    kd = [k.to(dev) for k in keys]
    params = [p for h in rh.bbox_head for p in h.parameters()]

    def run():
        vals, _, _, pg = _run_tape(rh, x, args, kd)
        return vals, pg
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                       # creates every .grad: the graph adds into these tensors
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with R.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
        cap = run()
    c = CASES[CASE]
    seen = []
    for k, gts in enumerate((inp['gts'], _draw_gts(c['G'], 1))):
        g2, c2 = rpn.pack_gts(gts, dev, 8)
        gt.copy_(g2)
        cnt.copy_(c2)
        for p in params:
            p.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = [cap[0].clone()] + [p.grad.clone() for p in params]
        got_pg = [t.clone() for t in cap[1]]
        for p in params:
            p.grad.zero_()
        fresh = run()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, [fresh[0]] + [p.grad for p in params])), k
        for a, b in zip(got_pg, fresh[1]):
            assert relmax(a, b) < 1e-5
        assert bool(torch.isfinite(got[0]).all()) and float(got[1].abs().max()) > 0
        seen.append(got)
    assert not torch.equal(seen[0][1], seen[1][1])                   # the graph followed the rewritten gts


# ----------------------------------------------------------------------------- 4. from the image
@pytest.mark.gpu
def test_roi_loss_backward_gpu():
    """FeatureExtractor.roi_loss_backward: the dict of roi_loss, and in the two flat arenas what the existing tapes produce when the
    recorded pyramid gradient is fed to them as cotangents (ExtractTrainer's step with lr = 0), under test_detector's gate"""
    import helpers as T
    import hrfuser_oracle as O
    from hrfuser_amd.detector import ExtractTrainer, FeatureExtractor
    from test_roi_loss import TRAIN, _roi_head_cfg
    from test_rpn_loss import RPN_CFG, TEST_CFG, TRAIN_CFG
    dev = use_backend('hip')
    cfg = T.load_cfgs()['t_nus']
    torch.manual_seed(0)
    train = copy.deepcopy(TRAIN)
    for t in train:
        t['sampler'].update(num=64)
    fx = FeatureExtractor(copy.deepcopy(cfg), dict(type='HRFPN', in_channels=[18, 36, 72, 144], out_channels=256), None,
                          copy.deepcopy(dict(RPN_CFG, train_cfg=copy.deepcopy(TRAIN_CFG), test_cfg=copy.deepcopy(TEST_CFG))),
                          dict(_roi_head_cfg(train=False, in_channels=256, fc_out=64), train_cfg=train))
    O.seeded_fill_(fx.backbone, 0)
    fx.neck.init_weights()
    fx.to(dev).train()
    T.disable_stochastic(fx.backbone)
    x, mods = O.seeded_inputs(B, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    kw = dict(zip(('lidar_img', 'radar_img', 'gated_img'), mods))
    gts = [torch.tensor([[4., 6., 40., 50.], [30., 10., 90., 60.]]).to(dev), torch.tensor([[10., 10., 50., 40.]]).to(dev)]
    labs = [torch.tensor([1, 4]).to(dev), torch.tensor([9]).to(dev)]
    metas = [dict(img_shape=(64, 96, 3), pad_shape=(64, 96, 3)), dict(img_shape=(60, 90, 3), pad_shape=(64, 96, 3))]
    rng = fx.roi_head.rng(dev)
    state = rng.clone()
    want = fx.roi_loss(x, gts, labs, metas, **kw)                    # (grad enabled: the recording forward, the launches roi_loss_backward issues)
    want = {k: v.detach().clone() for k, v in want.items()}
    rng.copy_(state)
    eb, en = fx.backbone._engine(), fx.neck._engine()
    eb.ready(dev); en.ready(dev)
    eb.flat_g.zero_(); en.flat_g.zero_()
    pg = []
    got = fx.roi_loss_backward(x, gts, labs, metas, pyramid_grads=pg, **kw)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want), ({k: float(v) for k, v in got.items()}, {k: float(v) for k, v in want.items()})
    gb, gn = eb.flat_g.clone(), en.flat_g.clone()
    assert float(gb.abs().max()) > 0 and float(gn.abs().max()) > 0 and bool(torch.isfinite(gb).all()) and bool(torch.isfinite(gn).all())
    for h in fx.roi_head.bbox_head:
        for k, p in h.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    assert len(pg) == 5 and all(t is not None for t in pg[:4])
    cots = [t if t is not None else torch.zeros((B, 64 // (4 << i), 96 // (4 << i), 256), device=dev) for i, t in enumerate(pg)]
    tr = ExtractTrainer(fx, lr=0.0, weight_decay=0.0)
    tr.step(x, mods, cots)
    torch.cuda.synchronize()
    e_n, e_b = T.rel_l2(gn, en.flat_g), T.rel_l2(gb, eb.flat_g)
    print(f'roi_loss_backward arenas vs the cotangent route: neck rel-L2 {e_n:.3e}, backbone rel-L2 {e_b:.3e}')
    assert e_n < 1e-4 and e_b < 1e-3
