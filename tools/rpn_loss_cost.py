"""Cost of the RPN training targets + loss (csrc/hrf_rpn_train.h: hrf_rpn_assign / hrf_rpn_loss; hrfuser_amd/rpn.py; DESIGN.md
section 20).

    python tools/rpn_loss_cost.py [--out profiles/rpn_loss_cost.txt] [--rounds 5]

One process.  The head's maps on the pyramid of 2 x 384 x 640 (96x160 ... 6x10, A = 3: 61 380 anchors per image) and of
2 x 384 x 1248 (96x312 ... 6x19), 30 ground truths per image (sides log-uniform 16..256 px, inside the image), the config's
train_cfg.rpn (MaxIoUAssigner 0.7 / 0.3 / 0.3 with low-quality matching, RandomSampler 256 x 0.5, allowed_border 0, SmoothL1
beta 1 / 9), generated sampling keys; logits ~ N(0, 2^2), deltas ~ N(0, 0.3^2) from a seed.  The whole call (six launches) and its
prefixes of 1 .. 5 launches (hrf_debug_knob 44) are timed graph-batched (profiling._graph_time: 20 calls per hipGraph, 5
replays, device events) after a warm-up call, --rounds rounds: median [min - max]; a launch's time is the difference of two
consecutive prefixes' medians.  That the call can be captured at all is what the graph timing shows (tests/test_rpn_loss.py::
test_loss_graph_gpu pins that a replay follows changed contents).

Beside it: the torch restatement of hrfuser_amd.testing (rpn bbox_overlaps_ref -> max_iou_assign_ref -> rpn_sample_ref ->
rpn_loss_ref with autograd) on the SAME GPU, wall clock around a synchronised call - what a user of the reference's host-driven
code has today (it reads device values on the host once per ground truth and cannot be captured).  No threshold is attached: the
parent of this path has no loss at all; the times stand beside the 10.3 ms training step they add to.  There is no CPU path:
without a GPU the tool fails."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, A, G = 2, 3, 30
STRIDES = [4, 8, 16, 32, 64]
STEP_MS = 10.3
LAUNCHES = ['rpnt_iou_kernel', 'rpnt_gtmax_kernel', 'rpnt_assign_kernel', 'rpnt_select_kernel', 'rpnt_loss_kernel<true>', 'rpnt_finalize_kernel']


def stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rpn_loss_cost.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=11)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('rpn_loss_cost: no GPU - this tool measures on the device and has no CPU path')
    from hrfuser_amd import _lib, profiling, rpn
    from hrfuser_amd import testing as T
    dev = torch.device('cuda:0')
    L = _lib.lib()
    bases_t = [T.rpn_base_anchors(s, [8], [0.5, 1.0, 2.0]) for s in STRIDES]
    bases = [b.tolist() for b in bases_t]
    cfg = rpn.train_cfg_struct(0.7, 0.3, 0.3, True, 0, 256, 128, 1.0 / 9.0, 1.0, 1.0)
    rows = [f'tools/rpn_loss_cost.py: hrf_rpn_loss (six launches), B = {B}, A = {A}, {G} ground truths per image, train_cfg.rpn of the configs, us per '
            f'call, median [min - max] of {a.rounds} rounds; the training step they add to: {STEP_MS} ms']
    sp = lambda s: f"{s['median']:8.2f} [{s['min']:.2f} - {s['max']:.2f}]"                    # noqa: E731
    for img_h, img_w in ((384, 640), (384, 1248)):
        g = torch.Generator().manual_seed(a.seed)
        sizes = [(img_h // s, img_w // s) for s in STRIDES]
        cm = [(2.0 * torch.randn(B, h, w, A, generator=g)).to(dev) for h, w in sizes]
        rm = [(0.3 * torch.randn(B, h, w, 4 * A, generator=g)).to(dev) for h, w in sizes]
        gts = []
        for _ in range(B):
            u = torch.rand(G, 4, generator=g, dtype=torch.float64)
            bw = torch.exp(math.log(16.0) + u[:, 0] * (math.log(256.0) - math.log(16.0))).clamp(max=img_w)
            bh = torch.exp(math.log(16.0) + u[:, 1] * (math.log(256.0) - math.log(16.0))).clamp(max=img_h)
            x1, y1 = u[:, 2] * (img_w - bw), u[:, 3] * (img_h - bh)
            gts.append(torch.stack([x1, y1, x1 + bw, y1 + bh], dim=1).float())
        shp = torch.tensor([[float(img_h), float(img_w)]] * B, device=dev)
        gt, cnt = rpn.pack_gts(gts, dev)
        st = rpn.rng_state(a.seed, 0, dev)
        out = rpn.rpn_loss(cm, rm, shp, shp, gt, cnt, STRIDES, bases, cfg, rng=st)
        grads, counts = out[1], out[5].tolist()
        N = out[2].shape[1]
        inside = int((out[2][0] > -2).sum())
        ws = torch.empty((L.hrf_rpn_train_workspace_bytes(rpn._levels(cm, rm, STRIDES, bases), cfg, gt.shape[1]),), device=dev, dtype=torch.uint8)
        call = lambda: rpn.rpn_loss(cm, rm, shp, shp, gt, cnt, STRIDES, bases, cfg, rng=st, workspace=ws, grads=grads)       # noqa: E731
        us = {k: [] for k in range(7)}
        try:
            for _ in range(a.rounds):
                for k in (1, 2, 3, 4, 5, 6, 0):                     # prefixes of k launches; 0 = the whole call
                    L.hrf_debug_knob(44, k)
                    us[k].append(profiling._graph_time(call) * 1e6)
        finally:
            L.hrf_debug_knob(44, 0)
        stt = {k: stats(v) for k, v in us.items()}
        # the restatement with torch on the same GPU (fp32, the reference's arithmetic): wall clock around a synchronised call
        anchors = torch.cat([T.rpn_grid_anchors(bases_t[l], h, w, STRIDES[l]) for l, (h, w) in enumerate(sizes)])
        ins = torch.cat([T.rpn_inside_flags_ref(T.rpn_grid_anchors(bases_t[l], h, w, STRIDES[l]), h, w, A, STRIDES[l], (img_h, img_w), (img_h, img_w), 0)
                         for l, (h, w) in enumerate(sizes)]).to(dev)
        anchors_d = anchors.to(dev)
        keys = [T.rpn_key_ref(a.seed, 0, b, N).to(dev) for b in range(B)]
        gts_d = [t.to(dev) for t in gts]
        cs = [m.permute(0, 3, 1, 2) for m in cm]
        bp = [m.permute(0, 3, 1, 2) for m in rm]

        def restatement():
            asg, smp = [], []
            for b in range(B):
                av, _ = T.max_iou_assign_ref(T.bbox_overlaps_ref(gts_d[b], anchors_d[ins]), 0.7, 0.3, 0.3, True)
                full = torch.full((N,), -2, dtype=torch.long, device=dev)
                full[ins] = av
                asg.append(full)
                smp.append(T.rpn_sample_ref(full, keys[b], 256, 128))
            return T.rpn_loss_ref(cs, bp, anchors_d, asg, smp, gts_d, 1.0 / 9.0, 1.0, 1.0)
        ref = restatement()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            restatement()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        rs = stats(ms)
        dl = float((torch.stack(ref[0] + ref[1]).cpu() - rpn.rpn_loss(cm, rm, shp, shp, gt, cnt, STRIDES, bases, cfg,
                                                                        rng=rpn.rng_state(a.seed, 0, dev))[0].reshape(-1).cpu()).abs().max())
        per = {LAUNCHES[k - 1]: round(stt[k]['median'] - (stt[k - 1]['median'] if k > 1 else 0.0), 2) for k in range(1, 7)}
        res = dict(img=[img_h, img_w], maps=sizes, anchors=N, inside=inside, counts=counts, whole_us=stt[0],
                   prefix_us={str(k): stt[k] for k in range(1, 7)}, launch_us=per, restatement_ms=rs, max_loss_diff=dl,
                   share_of_step=round(stt[0]['median'] / (STEP_MS * 1e3), 4))
        rows.append(f'\n{B} x {img_h} x {img_w}, maps ' + ', '.join(f'{h}x{w}' for h, w in sizes) + f': {N} anchors per image, {inside} inside, '
                    f'counts (assigned pos, assigned neg, sampled pos, sampled neg) {counts}')
        for k in range(1, 7):
            rows.append(f'  launches 1..{k}  {sp(stt[k])}   {LAUNCHES[k - 1]:24s} {per[LAUNCHES[k - 1]]:8.2f}')
        rows.append(f"  whole call     {sp(stt[0])}   = {100 * res['share_of_step']:.2f} % of the {STEP_MS} ms training step; captured in a hipGraph")
        rows.append(f"  torch restatement on the same GPU, ms per call {sp(rs)}   = {rs['median'] * 1e3 / stt[0]['median']:.0f} x the HIP call; "
                    f'largest loss difference {dl:.2e}')
        rows.append('  json: ' + json.dumps(res))
    text = '\n'.join(rows) + '\n'
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
