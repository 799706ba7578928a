"""Cost of the backward of the cascade bbox head (csrc/hrf_fc_bwd.h, hrfuser_amd/roi_head.py, FeatureExtractor.roi_loss_backward;
DESIGN.md section 24): every route of a comparison in the SAME process, interleaved, graph-timed (profiling._graph_time: launches
captured in a hipGraph, device events).  The parent has no such path; the outside yardstick is torch.matmul on the same GPU in the
same run (dy.t() @ x, dy @ w), and the fraction of the 157 TFLOP/s fp32-MFMA peak is reported beside it.

    python tools/fc_bwd_cost.py [--out profiles/fc_bwd_cost.txt] [--rounds 5] [--legs kernels,stage,cascade,step]

  kernels  hrf_fc_bwd_weight (with db) and hrf_fc_bwd_data (with the ReLU mask) at the three layer shapes (K, N) = (12544, 1024),
           (1024, 1024), (1024, 16) for M in {200, 1024, 2048} against torch.matmul; us per call, TFLOP/s on 2 M K N
  stage    one stage's Shared2FCBBoxHead.run_backward at M = 1024, features in (y, x, c) column order (hrf_fc_bwd_cols brings fc1's
           gradient back) against (c, y, x) order (no such launch), and hrf_fc_bwd_cols alone: the fc1 layout decision
  cascade  CascadeRoIHead.losses_nhwc + its tape (three stages, RoIAlign forward and adjoint) at B * num = 2 * 512 rows on the
           pyramid of 2 x 384 x 640, beside CascadeRoIHead.losses (the forward alone), in both feature layouts
  step     FeatureExtractor.roi_loss_backward (HRFuser-T + HRFPN + RPN head + cascade head, 2 x 384 x 640) beside ExtractTrainer's
           synthetic-loss step of the same backbone and neck, each captured in one hipGraph
Median [min - max] over --rounds interleaved rounds.  There is no CPU path: without a GPU the tool fails."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [(96, 160), (48, 80), (24, 40), (12, 20), (6, 10)]
STDS = [[0.1, 0.1, 0.2, 0.2], [0.05, 0.05, 0.1, 0.1], [0.033, 0.033, 0.067, 0.067]]
PEAK = 157.0                                                        # TFLOP/s, fp32 MFMA (MI355X)


def stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def sp(s):
    return f"{s['median']:9.2f} [{s['min']:.2f} - {s['max']:.2f}]"


def interleave(jobs, rounds, reps):
    from hrfuser_amd import profiling
    us = {n: [] for n, _ in jobs}
    for _ in range(rounds):
        for n, fn in jobs:
            us[n].append(profiling._graph_time(fn, reps=reps) * 1e6)
    return us


def train_cfg(num=512):
    return [dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=t, neg_iou_thr=t, min_pos_iou=t, match_low_quality=False, ignore_iof_thr=-1),
                 sampler=dict(type='RandomSampler', num=num, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1, debug=False)
            for t in (0.5, 0.6, 0.7)]


def roi_head_cfg():
    head = lambda s: dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=10,   # noqa: E731
                          bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.], target_stds=s), reg_class_agnostic=True,
                          loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    return dict(type='CascadeRoIHead', num_stages=3, stage_loss_weights=[1, 0.5, 0.25],
                bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                                        featmap_strides=[4, 8, 16, 32]),
                bbox_head=[head(s) for s in STDS], train_cfg=train_cfg(), test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100))


def rpn_cfg():
    return dict(type='RPNHead', in_channels=256, feat_channels=256,
                anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0]),
                loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                test_cfg=dict(nms_pre=1000, max_per_img=1000, nms=dict(type='nms', iou_threshold=0.7), min_bbox_size=0))


def leg_kernels(a, emit, torch, dev):
    from hrfuser_amd import _lib, roi_head
    emit(f'\n== 1. the two kernels against torch.matmul; us per call, median [min - max] of {a.rounds} interleaved rounds; TFLOP/s on 2 M K N '
         f'(fraction of the {PEAK:.0f} TFLOP/s fp32-MFMA peak) ==')
    g = torch.Generator().manual_seed(0)
    for K, N in ((12544, 1024), (1024, 1024), (1024, 16)):
        w = (torch.randn(N, K, generator=g) / N ** 0.5).to(dev)
        for M in (200, 1024, 2048):
            x = torch.randn(M, K, generator=g).clamp_(min=0).to(dev)
            dy = torch.randn(M, N, generator=g).to(dev)
            mask = torch.randn(M, K, generator=g).clamp_(min=0).to(dev)
            ws = roi_head.fc_bwd_workspace(M, K, N, dev)
            dw, db, dx = torch.empty(N, K, device=dev), torch.empty(N, device=dev), torch.empty(M, K, device=dev)
            tw, tx = torch.empty(N, K, device=dev), torch.empty(M, K, device=dev)
            jobs = [('weight', lambda: roi_head.fc_backward_weight(x, dy, N, dw, db, False, ws)),
                    ('torch dy.t() @ x', lambda: torch.matmul(dy.t(), x, out=tw)),
                    ('data', lambda: roi_head.fc_backward_data(dy, w, K, mask, dx, ws)),
                    ('torch dy @ w', lambda: torch.matmul(dy, w, out=tx))]
            us = interleave(jobs, a.rounds, 5)
            st = {k: stats(v) for k, v in us.items()}
            fl = 2.0 * M * K * N
            tf = lambda k: fl / st[k]['median'] / 1e6                # noqa: E731
            rw = float((dw - tw).abs().max() / tw.abs().max())
            rx = float((dx - torch.where(mask <= 0, torch.zeros_like(tx), tx)).abs().max() / tx.abs().max())
            emit(f"M = {M:5d} K = {K:5d} N = {N:4d}  weight {sp(st['weight'])} ({tf('weight'):6.1f} TFLOP/s, {tf('weight') / PEAK:5.1%})   torch {sp(st['torch dy.t() @ x'])} "
                 f"({tf('torch dy.t() @ x'):6.1f})   hip / torch = {st['weight']['median'] / st['torch dy.t() @ x']['median']:.2f}   relmax {rw:.1e}")
            emit(f"{'':34s}data   {sp(st['data'])} ({tf('data'):6.1f} TFLOP/s, {tf('data') / PEAK:5.1%})   torch {sp(st['torch dy @ w'])} "
                 f"({tf('torch dy @ w'):6.1f})   hip / torch = {st['data']['median'] / st['torch dy @ w']['median']:.2f}   relmax {rx:.1e}"
                 f"   workspace {_lib.lib().hrf_fc_bwd_workspace_bytes(M, K, N) / 2 ** 20:.1f} MiB")
            emit('  json: ' + json.dumps(dict(what='kernels', M=M, K=K, N=N, **{k.replace(' ', '_') + '_us': v for k, v in st.items()})))


def leg_stage(a, emit, torch, dev):
    from hrfuser_amd import HEADS, _lib
    torch.manual_seed(0)
    hd = HEADS.build(roi_head_cfg()['bbox_head'][0]).to(dev)
    M, F, Kin = 1024, 1024, 12544
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, Kin, generator=g).clamp_(min=0).to(dev)
    d = (torch.randn(M, 16, generator=g) / M).to(dev)
    saved = {}
    with torch.no_grad():
        for nhwc in (True, False):
            saved[nhwc] = hd.run_train(x, nhwc=nhwc)[1]
        hd.run_backward(saved[True], d)                             # creates every .grad: the timed calls add into them
        tmp, gw = torch.empty(F, Kin, device=dev), hd.shared_fcs[0].weight.grad
        jobs = [('(y, x, c) + hrf_fc_bwd_cols', lambda: hd.run_backward(saved[True], d)), ('(c, y, x)', lambda: hd.run_backward(saved[False], d)),
                ('hrf_fc_bwd_cols alone', lambda: _lib.lib().hrf_fc_bwd_cols(tmp, Kin, gw, Kin, 1, F, 256, 49, _lib.stream_ptr()))]
        us = interleave(jobs, a.rounds, 3)
    st = {k: stats(v) for k, v in us.items()}
    fl = 2.0 * M * (2 * Kin * F + 2 * F * F + 2 * F * 16)
    emit(f'\n== 2. one stage: Shared2FCBBoxHead.run_backward, M = {M} rows, 12544 -> 1024 -> 1024 -> 16; us per call ({fl / 1e9:.1f} GFLOP) ==')
    for k, v in st.items():
        emit(f"{k:30s} {sp(v)}" + (f"   {fl / v['median'] / 1e6:6.1f} TFLOP/s ({fl / v['median'] / 1e6 / PEAK:5.1%} of peak)" if 'alone' not in k else ''))
    emit('  json: ' + json.dumps(dict(what='stage', M=M, **{k: v for k, v in st.items()})))


def _pyramid_and_heads(torch, dev):
    from hrfuser_amd import HEADS
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(2, 256, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    rpn = HEADS.build(rpn_cfg()).to(dev).eval()
    rh = HEADS.build(roi_head_cfg()).to(dev).eval()
    with torch.no_grad():
        rpn.rpn_reg.weight.mul_(0.5)
        for h in rh.bbox_head:
            h.fc_cls.weight.mul_(400.0)
            h.fc_reg.weight.mul_(2000.0)
    return feats, rpn, rh


def _gts(torch, dev):
    from hrfuser_amd import roi_head, rpn
    g = torch.Generator().manual_seed(3)
    gts, labs = [], []
    for n in (9, 6):
        c = torch.rand(n, 2, generator=g) * torch.tensor([640., 384.])
        wh = 24 + torch.rand(n, 2, generator=g) * 200
        b = torch.cat([c - wh / 2, c + wh / 2], dim=1)
        b[:, 0::2].clamp_(0, 640)
        b[:, 1::2].clamp_(0, 384)
        gts.append(b.to(dev))
        labs.append(torch.randint(0, 10, (n,), generator=g).to(dev))
    gt, cnt = rpn.pack_gts(gts, dev, 16)
    return gt, roi_head.pack_gt_labels(labs, dev, 16), cnt


def leg_cascade(a, emit, torch, dev):
    from hrfuser_amd import runtime as R
    from hrfuser_amd.testing import BlockHarness
    feats, rpn, rh = _pyramid_and_heads(torch, dev)
    shp = torch.tensor([[384., 640.], [384., 640.]], device=dev)
    with torch.no_grad():
        _, count, rois = rpn.proposals(*rpn(feats), shp)
    gt, gl, cnt = _gts(torch, dev)
    args = (rois, count, gt, gl, cnt, shp)

    def tape(layout):
        def runner(ctx, blk, acts):
            rh._losses_nhwc(ctx, acts, *args, out_layout=layout)
            return acts
        ctx, _, _ = BlockHarness(torch.nn.Identity(), runner)._execute(tuple(feats[:4]), True, needs=[True] * 4)
        ctx.run_backward()
    with torch.no_grad():
        tape(1)
        jobs = [('losses (forward alone)', lambda: rh.losses(feats, *args)), ('losses_nhwc + tape, (y, x, c)', lambda: tape(1)),
                ('losses_nhwc + tape, (c, y, x)', lambda: tape(0))]
        us = interleave(jobs, a.rounds, 1)
    st = {k: stats(v) for k, v in us.items()}
    emit(f'\n== 3. three stages at B * num = 2 * 512 rows ({rois.shape[0]} proposals, {cnt.tolist()} gts) on the pyramid of 2 x 384 x 640; us per call ==')
    for k, v in st.items():
        emit(f'{k:32s} {sp(v)}')
    b = st['losses_nhwc + tape, (y, x, c)']['median'] - st['losses (forward alone)']['median']
    emit(f'the backward of the three stages with RoIAlign\'s adjoint (difference of the medians; the tape call also copies the four maps in) ~ {b:.0f} us')
    emit('  json: ' + json.dumps(dict(what='cascade', **st)))
    R.release_step_buffers()


def leg_step(a, emit, torch, dev):
    import time
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import hrfuser_oracle as O
    from hrfuser_amd import HRFPN
    from hrfuser_amd import runtime as R
    from hrfuser_amd.configs import backbone_cfg
    from hrfuser_amd.detector import ExtractTrainer, FeatureExtractor, make_pyramid_cotangents
    cfg = backbone_cfg('t_nus_bn')
    torch.manual_seed(0)
    fx = FeatureExtractor(copy.deepcopy(cfg), dict(type='HRFPN', in_channels=list(cfg['extra']['stage4']['num_channels']), out_channels=256), None,
                          rpn_cfg(), roi_head_cfg())
    O.seeded_fill_(fx.backbone, 0)
    fx.neck.init_weights()
    fx.to(dev).train()
    x, mods = O.seeded_inputs(2, 384, 640, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    gt, gl, cnt = _gts(torch, dev)
    shp = torch.tensor([[384., 640.], [384., 640.]], device=dev)

    def timed(g, n=10):
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            g.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fx._roi_loss_backward(x, mods, gt, gl, cnt, shp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g1 = torch.cuda.CUDAGraph()
    with R.gc_paused(), torch.cuda.graph(g1, capture_error_mode='thread_local'):
        vals = fx._roi_loss_backward(x, mods, gt, gl, cnt, shp)
    et = ExtractTrainer(fx, lr=0.0, weight_decay=0.0)
    et.capture(x, mods, make_pyramid_cotangents(fx, x, mods))
    ms = {'roi_loss_backward': [], 'ExtractTrainer step': []}
    for _ in range(a.rounds):                                       # the two graphs alternate
        ms['roi_loss_backward'].append(timed(g1))
        ms['ExtractTrainer step'].append(timed(et.graph))
    st = {k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in ms.items()}
    emit('\n== 4. from the images: HRFuser-T (t_nus_bn) + HRFPN at 2 x 384 x 640, one hipGraph each; ms per replay (wall clock over 10 replays) ==')
    emit(f"FeatureExtractor.roi_loss_backward (backbone + neck tapes, RPN head + proposals, 3 stages forward + backward; no optimizer) "
         f"{st['roi_loss_backward']['median']:.3f} [{st['roi_loss_backward']['min']:.3f} - {st['roi_loss_backward']['max']:.3f}]")
    emit(f"ExtractTrainer step (backbone + neck tapes, synthetic loss, AdamW on both arenas)                                      "
         f"{st['ExtractTrainer step']['median']:.3f} [{st['ExtractTrainer step']['min']:.3f} - {st['ExtractTrainer step']['max']:.3f}]")
    emit(f'losses of the captured pass: {[round(float(v), 4) for v in vals.flatten().tolist()]}')
    emit('  json: ' + json.dumps(dict(what='step', **st)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fc_bwd_cost.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--legs', default='kernels,stage,cascade,step')
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit('fc_bwd_cost: --rounds must be at least 5 (the spread is part of the result)')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fc_bwd_cost: no GPU - this tool measures on the device and has no CPU path')
    dev = torch.device('cuda:0')
    rows = []

    def emit(text):
        print(text, flush=True)
        rows.append(text)
        if a.out:                                                     # rewritten after every line: a leg that fails keeps what came before
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                fh.write('\n'.join(rows) + '\n')
    emit('tools/fc_bwd_cost.py: backward of the cascade bbox head - hrf_fc_bwd_weight / hrf_fc_bwd_data against torch.matmul, the stage, the cascade, the step '
         '(same build, same process, interleaved)')
    legs = dict(kernels=leg_kernels, stage=leg_stage, cascade=leg_cascade, step=leg_step)
    for name in a.legs.split(','):
        legs[name](a, emit, torch, dev)


if __name__ == '__main__':
    main()
