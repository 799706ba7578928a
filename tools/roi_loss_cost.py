"""Cost of the cascade RoI head's training targets + losses (csrc/hrf_bbox_train.h: hrf_bbox_targets / hrf_bbox_loss;
hrfuser_amd/roi_head.py: CascadeRoIHead.losses).

    python tools/roi_loss_cost.py [--out profiles/roi_loss_cost.txt] [--rounds 5]

One process.  The roi_head of the configs (three Shared2FCBBoxHead stages, 256 channels, 1024-wide FCs, 10 classes, train_cfg.rcnn:
MaxIoUAssigner 0.5 / 0.6 / 0.7 without low-quality matching, RandomSampler 512 x 0.25 with the gts added, SmoothL1 beta 1, stage
weights 1 / 0.5 / 0.25) on the pyramid of 2 x 384 x 640 (96x160 ... 12x20), B = 2, 30 ground truths per image (sides log-uniform
16..256 px), R = 1000 and R = 2000 proposals per image: half of them ground truths jittered by up to 30 % of their size, half
uniformly random boxes; generated sampling keys.  Everything is timed graph-batched (profiling._graph_time: the call captured several
times into one hipGraph, replayed, device events) after a warm-up call, --rounds rounds, interleaved: median [min - max].
  per stage   hrf_bbox_targets (two launches; the prefix of one launch through hrf_debug_knob 48), hrf_bbox_loss (two launches),
              hrf_bbox_refine, each on the stage's own inputs taken from a `losses(..., stages=[])` call
  chain       the three stages' targets -> loss -> refine alone, on the stored head outputs (no RoIAlign, no FC layers)
  losses      CascadeRoIHead.losses: the same with hrf_roi_align_fwd and the three FC layers of every stage
Beside it: the torch restatement of hrfuser_amd.testing (rcnn_assign_ref -> rcnn_sample_ref -> bbox_targets_ref -> bbox_loss_ref
with autograd, per stage on the stage's own inputs) on the SAME GPU, wall clock around a synchronised call - what the reference's
host-driven code costs today (nonzero / argsort per image, `.item()` per stage; it cannot be captured).  No threshold is attached:
the parent of this path has no RoI loss at all; the times stand beside the 10.3 ms training step they add to.  There is no CPU
path: without a GPU the tool fails."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, G, NC, C = 2, 30, 10, 256
IMG = (384, 640)
STRIDES = [4, 8, 16, 32]
STDS = [[0.1, 0.1, 0.2, 0.2], [0.05, 0.05, 0.1, 0.1], [0.033, 0.033, 0.067, 0.067]]
THR = (0.5, 0.6, 0.7)
STEP_MS = 10.3


def stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def roi_head_cfg():
    head = lambda s: dict(type='Shared2FCBBoxHead', in_channels=C, fc_out_channels=1024, roi_feat_size=7, num_classes=NC,       # noqa: E731
                          bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.], target_stds=s), reg_class_agnostic=True,
                          loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                          loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    train = [dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=t, neg_iou_thr=t, min_pos_iou=t, match_low_quality=False, ignore_iof_thr=-1),
                  sampler=dict(type='RandomSampler', num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1, debug=False)
             for t in THR]
    return dict(type='CascadeRoIHead', num_stages=3, stage_loss_weights=[1, 0.5, 0.25],
                bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=C,
                                        featmap_strides=STRIDES),
                bbox_head=[head(s) for s in STDS], train_cfg=train)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'roi_loss_cost.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=11)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('roi_loss_cost: no GPU - this tool measures on the device and has no CPU path')
    from hrfuser_amd import HEADS, _lib, profiling, roi_head, rpn
    from hrfuser_amd import testing as T
    dev = torch.device('cuda:0')
    L = _lib.lib()
    torch.manual_seed(a.seed)
    rh = HEADS.build(roi_head_cfg())
    with torch.no_grad():
        for h in rh.bbox_head:                                       # logits of a few units, as a trained head's
            h.fc_cls.weight.mul_(30.0)
            h.fc_reg.weight.mul_(100.0)
    rh = rh.to(dev).eval()
    img_h, img_w = IMG
    g = torch.Generator().manual_seed(a.seed)
    feats = [torch.randn(B, C, img_h // s, img_w // s, generator=g).to(dev).contiguous(memory_format=torch.channels_last) for s in STRIDES]
    gts = []
    for _ in range(B):
        u = torch.rand(G, 4, generator=g, dtype=torch.float64)
        bw = torch.exp(math.log(16.0) + u[:, 0] * (math.log(256.0) - math.log(16.0))).clamp(max=img_w)
        bh = torch.exp(math.log(16.0) + u[:, 1] * (math.log(256.0) - math.log(16.0))).clamp(max=img_h)
        x1, y1 = u[:, 2] * (img_w - bw), u[:, 3] * (img_h - bh)
        gts.append(torch.stack([x1, y1, x1 + bw, y1 + bh], dim=1).float())
    labels = [torch.randint(0, NC, (G,), generator=g) for _ in range(B)]
    gt, cnt = rpn.pack_gts(gts, dev)
    gl = roi_head.pack_gt_labels(labels, dev, gt.shape[1])
    shp = torch.tensor([[float(img_h), float(img_w)]] * B, device=dev)
    sp = lambda s: f"{s['median']:8.2f} [{s['min']:.2f} - {s['max']:.2f}]"                    # noqa: E731
    rows = [f'tools/roi_loss_cost.py: CascadeRoIHead.losses, B = {B}, {G} ground truths per image, {NC} classes, train_cfg.rcnn of the configs (num 512, '
            f'thresholds {THR}), pyramid of {B} x {img_h} x {img_w}; us per call, median [min - max] of {a.rounds} interleaved rounds; the training '
            f'step they add to: {STEP_MS} ms']
    for R in (1000, 2000):
        rois = torch.zeros(B, R, 5)
        for b in range(B):
            base = gts[b][torch.randint(0, G, (R // 2,), generator=g)]
            wh = (base[:, 2:] - base[:, :2]).repeat(1, 2)
            jit = base + 0.3 * wh * (torch.rand(R // 2, 4, generator=g) * 2 - 1)
            c = torch.rand(R - R // 2, 2, generator=g) * torch.tensor([float(img_w), float(img_h)])
            s = 8 + torch.rand(R - R // 2, 2, generator=g) * 200
            rois[b, :, 0] = b
            rois[b, :, 1:] = torch.cat([jit, torch.cat([c - s / 2, c + s / 2], dim=1)])
        rois = rois.reshape(B * R, 5).to(dev)
        count = torch.full((B,), R, dtype=torch.int32, device=dev)
        st = rh.rng(dev)
        st.copy_(rpn.rng_state(a.seed, 0, dev))
        stages = []
        vals, _ = rh.losses(feats, rois, count, gt, gl, cnt, shp, stages=stages)
        torch.cuda.synchronize()
        counts = [sg['targets'][4].tolist() for sg in stages]

        def targets(i):
            sg = stages[i]
            return roi_head.bbox_targets(sg['rois'], gt, gl, cnt, sg['cfg'], sg['first'], sg['count'], rng=st, stage=i)

        def loss(i):
            sg = stages[i]
            return roi_head.bbox_loss(sg['out'], sg['targets'][1], sg['targets'][2], sg['targets'][4], sg['cfg'], d_out=sg['d_out'])

        def refine(i):
            sg = stages[i]
            return roi_head.bbox_refine(sg['targets'][0], sg['out'][:, NC + 1:NC + 5], STDS[i], shp, B)

        def chain():
            cur, first, cn = rois, None, count
            for i, sg in enumerate(stages):
                t = roi_head.bbox_targets(cur, gt, gl, cnt, sg['cfg'], first, cn, rng=st, stage=i)
                roi_head.bbox_loss(sg['out'], t[1], t[2], t[4], sg['cfg'], rng=st if i == 2 else None, d_out=sg['d_out'])
                cur, first, cn = roi_head.bbox_refine(t[0], sg['out'][:, NC + 1:NC + 5], STDS[i], shp, B), t[4][:, 4], t[4][:, 5]

        whole = lambda: rh.losses(feats, rois, count, gt, gl, cnt, shp)                              # noqa: E731
        jobs = {}
        for i in range(3):
            jobs[f's{i}.targets.launch1'] = (lambda i=i: targets(i), 1)
            jobs[f's{i}.targets'] = (lambda i=i: targets(i), 0)
            jobs[f's{i}.loss'] = (lambda i=i: loss(i), 0)
            jobs[f's{i}.refine'] = (lambda i=i: refine(i), 0)
        jobs['chain'] = (chain, 0)
        jobs['losses'] = (whole, 0)
        us = {k: [] for k in jobs}
        try:
            for _ in range(a.rounds):
                for k, (fn, knob) in jobs.items():
                    L.hrf_debug_knob(48, knob)
                    us[k].append(profiling._graph_time(fn, reps=4 if k == 'losses' else 20) * 1e6)
        finally:
            L.hrf_debug_knob(48, 0)
        stt = {k: stats(v) for k, v in us.items()}

        # the restatement with torch on the same GPU (fp32, the reference's arithmetic), per stage on the stage's own inputs
        gts_d, labels_d = [t.to(dev) for t in gts], [t.to(dev) for t in labels]
        Gm = gt.shape[1]

        def restatement():
            out = []
            for i, sg in enumerate(stages):
                Rs = sg['rois'].shape[0] // B
                first = [0] * B if sg['first'] is None else sg['first'].tolist()          # (the host reads the reference makes too)
                cn = sg['count'].tolist()
                lab, tg = [], []
                for b in range(B):
                    props = sg['rois'].reshape(B, Rs, 5)[b, first[b]:cn[b], 1:]
                    asg, _, boxes = T.rcnn_assign_ref(props, gts_d[b], THR[i], THR[i])
                    slots = torch.cat([torch.arange(G), Gm + first[b] + torch.arange(cn[b] - first[b])]).to(dev)
                    keys = T.rcnn_key_ref(a.seed, 0, i, b, Gm + Rs).to(dev)
                    pos, neg = T.rcnn_sample_ref(asg, keys[slots], 512, 128)
                    _, l, t = T.bbox_targets_ref(boxes, asg, pos, neg, gts_d[b], labels_d[b], NC, STDS[i])
                    pad = 512 - l.numel()
                    lab.append(torch.cat([l, l.new_full((pad,), -1)]))
                    tg.append(torch.cat([t, t.new_zeros((pad, 4))]))
                lab, tg = torch.cat(lab), torch.cat(tg)
                v = lab >= 0
                w = (1.0, 0.5, 0.25)[i]
                out.append(T.bbox_loss_ref(sg['out'][v][:, :NC + 1], sg['out'][v][:, NC + 1:NC + 5], lab[v], tg[v], NC, 1.0, w, w))
            return out
        ref = restatement()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            restatement()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        rs = stats(ms)
        dl = max(abs(float(ref[i][k]) - float(vals[i, j])) for i in range(3) for j, k in ((0, 'loss_cls'), (1, 'loss_bbox'), (2, 'acc')))
        res = dict(R=R, counts=counts, us=stt, restatement_ms=rs, max_result_diff=dl, losses=[[round(float(x), 6) for x in r] for r in vals.tolist()],
                   share_of_step=dict(chain=round(stt['chain']['median'] / (STEP_MS * 1e3), 4), losses=round(stt['losses']['median'] / (STEP_MS * 1e3), 4)))
        rows.append(f'\nR = {R} proposals per image; counts per stage (P, N, sampled pos, sampled neg, sampled gts, rows) {counts}')
        for i in range(3):
            t1, tt = stt[f's{i}.targets.launch1'], stt[f's{i}.targets']
            rows.append(f"  stage {i}: targets {sp(tt)} (bbt_assign_kernel {t1['median']:.2f}, bbt_sample_kernel {tt['median'] - t1['median']:.2f})   loss "
                        f"{sp(stt[f's{i}.loss'])}   refine {sp(stt[f's{i}.refine'])}")
        rows.append(f"  three stages, targets + loss + refine alone  {sp(stt['chain'])}   = {100 * res['share_of_step']['chain']:.2f} % of the {STEP_MS} ms step")
        rows.append(f"  CascadeRoIHead.losses (with RoIAlign + FCs)  {sp(stt['losses'])}   = {100 * res['share_of_step']['losses']:.2f} % of the {STEP_MS} ms step; "
                    'captured in a hipGraph')
        rows.append(f"  torch restatement of targets + loss on the same GPU, ms per call {sp(rs)}   = {rs['median'] * 1e3 / stt['chain']['median']:.0f} x the "
                    f'HIP chain; largest difference of a result {dl:.2e}')
        rows.append('  json: ' + json.dumps(res))
    text = '\n'.join(rows) + '\n'
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
