"""Cost of the cascade bbox head at test time (csrc/hrf_fc.h, csrc/hrf_bbox.h, hrfuser_amd/roi_head.py): the
hrf_fc route against the HRF_FC_ROUTE=rowgemm route (hrf_rowgemm + hrf_affine_act_res, the launches the library had before) of the
SAME build in the SAME process, interleaved, graph-timed (profiling._graph_time: back-to-back launches in a hipGraph, device events).

    python tools/roi_head_cost.py [--out profiles/roi_head_cost.txt] [--rounds 5] [--legs fc,stage,detect,whole]

  fc       fc1 alone (bias + ReLU): M in {200, 1000, 2000, 4000}, K = 12544, N = 1024; us per call, TFLOP/s on 2 M K N
  stage    one whole cascade stage at 2000 rois on the pyramid of 2 x 384 x 640: hrf_roi_align_fwd + the three FCs + hrf_bbox_refine
  detect   hrf_bbox_detect alone at B = 2, R = 1000, 10 classes, 3 stages (score_thr 0.05, iou_thr 0.5, max_per_img 100)
  whole    CascadeRoIHead.detect (3 stages + post-processing) on the same pyramid with the 2 x 1000 rois of RPNHead.proposals
           (test_cfg.rpn of the configs), and RPNHead forward + proposals beside it (the eval forward of the backbones at this
           size: profiles/bneck_eval_cost.txt, section 2)
Median [min - max] over --rounds interleaved rounds.  There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [(96, 160), (48, 80), (24, 40), (12, 20), (6, 10)]
STDS = [[0.1, 0.1, 0.2, 0.2], [0.05, 0.05, 0.1, 0.1], [0.033, 0.033, 0.067, 0.067]]
ROUTES = ('fc', 'rowgemm')


def stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def sp(s):
    return f"{s['median']:9.2f} [{s['min']:.2f} - {s['max']:.2f}]"


def interleave(jobs, rounds, reps):
    """jobs: [(name, fn)] -> {name: [us per call] per round}, the jobs interleaved within every round"""
    from hrfuser_amd import profiling
    us = {n: [] for n, _ in jobs}
    for _ in range(rounds):
        for n, fn in jobs:
            us[n].append(profiling._graph_time(fn, reps=reps) * 1e6)
    return us


def roi_head_cfg():
    head = lambda s: dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=10,
                          bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.], target_stds=s), reg_class_agnostic=True)
    return dict(type='CascadeRoIHead', num_stages=3, stage_loss_weights=[1, 0.5, 0.25],
                bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                                        featmap_strides=[4, 8, 16, 32]),
                bbox_head=[head(s) for s in STDS], test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100))


def rpn_cfg():
    return dict(type='RPNHead', in_channels=256, feat_channels=256,
                anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0]),
                loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                test_cfg=dict(nms_pre=1000, max_per_img=1000, nms=dict(type='nms', iou_threshold=0.7), min_bbox_size=0))


def leg_fc(a, emit, torch, dev):
    from hrfuser_amd import _lib, roi_head
    L = _lib.lib()
    K, N = 12544, 1024
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    wp = torch.empty(N * K, device=dev)
    L.hrf_fc_pack(w, N, K, N, K, wp, _lib.stream_ptr())
    bias = torch.randn(N, generator=g).to(dev)
    consts = (torch.ones(N, device=dev), torch.zeros(N, device=dev))
    emit(f'\n== 1. fc1 alone: y = relu(bias + x W^T), K = {K}, N = {N}; us per call, median [min - max] of {a.rounds} interleaved rounds ==')
    for M in (200, 1000, 2000, 4000):
        x = torch.randn(M, K, generator=g).to(dev)
        outs = {r: torch.empty(M, N, device=dev) for r in ROUTES}
        jobs = [(r, lambda r=r: roi_head.fc(x, wp, bias, N, True, out=outs[r], route=r, consts=consts)) for r in ROUTES]
        us = interleave(jobs, a.rounds, 5)
        st = {r: stats(us[r]) for r in ROUTES}
        rel = float((outs['fc'] - outs['rowgemm']).abs().max() / outs['rowgemm'].abs().max())
        below = st['fc']['max'] < st['rowgemm']['min']
        fl = 2.0 * M * K * N
        emit(f"M = {M:5d}  hrf_fc {sp(st['fc'])} ({fl / st['fc']['median'] / 1e6:6.1f} TFLOP/s)   rowgemm + act {sp(st['rowgemm'])} "
             f"({fl / st['rowgemm']['median'] / 1e6:6.1f} TFLOP/s)   fc / rowgemm = {st['fc']['median'] / st['rowgemm']['median']:.3f}"
             f"   ranges {'disjoint, hrf_fc below' if below else 'NOT separated'}   routes relmax {rel:.1e}"
             f"   workspace {L.hrf_fc_workspace_bytes(M, K, N) / 2 ** 20:.1f} MiB")
        emit('  json: ' + json.dumps(dict(what='fc', M=M, K=K, N=N, fc_us=st['fc'], rowgemm_us=st['rowgemm'], fc_rounds=us['fc'], rowgemm_rounds=us['rowgemm'])))


def _pyramid_and_heads(torch, dev):
    from hrfuser_amd import HEADS
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(2, 256, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    rpn = HEADS.build(rpn_cfg()).to(dev).eval()
    rh = HEADS.build(roi_head_cfg()).to(dev).eval()
    with torch.no_grad():
        rpn.rpn_reg.weight.mul_(0.5)
        for h in rh.bbox_head:                                     # logits ~ N(0, 2), deltas * stds ~ N(0, 0.1): a trained head's ranges
            h.fc_cls.weight.mul_(400.0)
            h.fc_reg.weight.mul_(2000.0)
    return feats, rpn, rh


def leg_stage(a, emit, torch, dev):
    from hrfuser_amd import roi_head
    from hrfuser_amd.roi import _nhwc, roi_forward
    feats, rpn, rh = _pyramid_and_heads(torch, dev)
    shp = torch.tensor([[384., 640.], [384., 640.]], device=dev)
    _, count, rois = rpn.proposals(*rpn(feats), shp)
    maps = [_nhwc(t) for t in feats[:4]]
    ex, hd = rh.bbox_roi_extractor[0], rh.bbox_head[0]

    def stage(route):
        f = roi_forward(maps, rois, ex._scales(), float(ex.finest_scale), 1)
        out = hd.run(f.reshape(f.shape[0], -1), nhwc=True, route=route)
        return roi_head.bbox_refine(rois, out[:, 11:15], hd.target_stds, shp, 2)
    us = interleave([(r, lambda r=r: stage(r)) for r in ROUTES] + [('roi_align', lambda: roi_forward(maps, rois, ex._scales(), float(ex.finest_scale), 1))],
                    a.rounds, 3)
    st = {k: stats(v) for k, v in us.items()}
    emit(f'\n== 2. one cascade stage at {rois.shape[0]} rois (proposals per image {count.tolist()}), pyramid of 2 x 384 x 640; us ==')
    emit(f"hrf_fc route   {sp(st['fc'])}\nrowgemm route  {sp(st['rowgemm'])}\n  of which hrf_roi_align_fwd {sp(st['roi_align'])}")
    emit('  json: ' + json.dumps(dict(what='stage', rois=rois.shape[0], **{k + '_us': v for k, v in st.items()})))


def leg_detect(a, emit, torch, dev):
    from hrfuser_amd import roi_head
    B, R, C = 2, 1000, 10
    g = torch.Generator().manual_seed(2)
    c = torch.rand(40, 2, generator=g) * torch.tensor([640., 384.])
    wh = 16 + torch.rand(40, 2, generator=g) * 200
    base = torch.cat([c - wh / 2, c + wh / 2], dim=1)[torch.randint(0, 40, (B * R,), generator=g)]
    box = base + 0.08 * (base[:, 2:] - base[:, :2]).repeat(1, 2) * (torch.rand(B * R, 4, generator=g) * 2 - 1)
    box[:, 0::2].clamp_(0, 640)
    box[:, 1::2].clamp_(0, 384)
    rois = torch.cat([torch.arange(B).repeat_interleave(R)[:, None].float(), box], dim=1).to(dev)
    pads = [torch.zeros(B * R, 16) for _ in range(3)]
    for p in pads:
        p[:, :C + 1] = 2.0 * torch.randn(B * R, C + 1, generator=g)
    pads[2][:, C + 1:C + 5] = 0.3 * torch.randn(B * R, 4, generator=g)
    pads = [p.to(dev) for p in pads]
    shp = torch.tensor([[384., 640.], [384., 640.]], device=dev)
    cnt = torch.tensor([R, R], dtype=torch.int32, device=dev)
    ws = torch.empty(roi_head._lib.lib().hrf_bbox_detect_workspace_bytes(B, R, C), device=dev, dtype=torch.uint8)
    fn = lambda: roi_head.bbox_detect(rois, cnt, [p[:, :C + 1] for p in pads], pads[2][:, C + 1:C + 5], STDS[2], shp, B, C, 0.05, 0.5, 100, workspace=ws)
    us = interleave([('detect', fn)], a.rounds, 5)
    st = stats(us['detect'])
    n = roi_head.bbox_detect(rois, cnt, [p[:, :C + 1] for p in pads], pads[2][:, C + 1:C + 5], STDS[2], shp, B, C, 0.05, 0.5, 100)[2].tolist()
    emit(f'\n== 3. hrf_bbox_detect alone: B = {B}, R = {R}, {C} classes, 3 stages of logits; us per call (4 launches) ==')
    emit(f"hrf_bbox_detect {sp(st)}   detections per image {n}, workspace {ws.numel() / 2 ** 20:.1f} MiB")
    emit('  json: ' + json.dumps(dict(what='detect', B=B, R=R, classes=C, us=st)))


def leg_whole(a, emit, torch, dev):
    feats, rpn, rh = _pyramid_and_heads(torch, dev)
    shp = torch.tensor([[384., 640.], [384., 640.]], device=dev)
    _, count, rois = rpn.proposals(*rpn(feats), shp)

    def det(route):
        os.environ['HRF_FC_ROUTE'] = route
        try:
            return rh.detect(feats, rois, count, shp)
        finally:
            os.environ.pop('HRF_FC_ROUTE', None)
    us = interleave([(r, lambda r=r: det(r)) for r in ROUTES] + [('rpn', lambda: rpn.proposals(*rpn(feats), shp))], a.rounds, 2)
    st = {k: stats(v) for k, v in us.items()}
    same = all(torch.equal(x, y) for x, y in zip(det('fc'), det('fc')))
    emit(f'\n== 4. CascadeRoIHead.detect, 3 stages + post-processing, {rois.shape[0]} rois on the pyramid of 2 x 384 x 640; us per call ==')
    emit(f"hrf_fc route   {sp(st['fc'])}   = {st['fc']['median'] / 2e3:.3f} ms per image\nrowgemm route  {sp(st['rowgemm'])}   = "
         f"{st['rowgemm']['median'] / 2e3:.3f} ms per image\nRPNHead forward + proposals {sp(st['rpn'])}   two calls bit-equal: {same}")
    emit('  json: ' + json.dumps(dict(what='whole', rois=rois.shape[0], **{k + '_us': v for k, v in st.items()})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'roi_head_cost.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--legs', default='fc,stage,detect,whole')
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit('roi_head_cost: --rounds must be at least 5 (the spread is part of the result)')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('roi_head_cost: no GPU - this tool measures on the device and has no CPU path')
    dev = torch.device('cuda:0')
    rows = []

    def emit(text):
        print(text, flush=True)
        rows.append(text)
        if a.out:                                                     # rewritten after every line: a leg that fails keeps what came before
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                fh.write('\n'.join(rows) + '\n')
    emit('tools/roi_head_cost.py: cascade bbox head at test time, hrf_fc route against the rowgemm route (same build, same process, interleaved)')
    legs = dict(fc=leg_fc, stage=leg_stage, detect=leg_detect, whole=leg_whole)
    with torch.no_grad():
        for name in a.legs.split(','):
            legs[name](a, emit, torch, dev)


if __name__ == '__main__':
    main()
