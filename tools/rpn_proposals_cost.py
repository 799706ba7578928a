"""Cost of the RPN proposal launches (csrc/hrf_rpn.h: hrf_rpn_select_decode / hrf_nms_segments / hrf_rpn_proposals;
hrfuser_amd/rpn.py).

    python tools/rpn_proposals_cost.py [--out profiles/rpn_proposals_cost.txt] [--rounds 5]

One process.  The head's maps on the pyramid of 2 x 384 x 640 (96x160 ... 6x10, A = 3) and of 2 x 384 x 1248 (96x312 ... 6x19),
nms_pre = max_per_img = 2000 and 1000, iou_threshold 0.7; logits ~ N(0, 1), deltas ~ N(0, 0.1) from a seed (neighbouring anchors
overlap above 0.7: suppression is the common case, as on a trained head).  Stage 1 (one launch), stages 2 + 3 (three launches,
on the rows stage 1 produced) and the whole call (four launches) are timed graph-batched (profiling._graph_time: 20 calls per
hipGraph, 5 replays, device events) after a warm-up call, --rounds rounds: median [min - max].  No threshold is attached: the
parent of this path has no proposals at all; the times stand beside the 1.78 ms / image eval forward they add to.  There is no
CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, A = 2, 3
STRIDES = [4, 8, 16, 32, 64]
EVAL_MS_PER_IMG = 1.78


def stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rpn_proposals_cost.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=11)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('rpn_proposals_cost: no GPU - this tool measures on the device and has no CPU path')
    from hrfuser_amd import profiling, rpn
    from hrfuser_amd.testing import rpn_base_anchors
    dev = torch.device('cuda:0')
    bases = [rpn_base_anchors(s, [8], [0.5, 1.0, 2.0]).tolist() for s in STRIDES]
    rows = [f'tools/rpn_proposals_cost.py: hrf_rpn_select_decode (stage 1), hrf_nms_segments (stages 2 + 3), hrf_rpn_proposals (all), B = {B}, '
            f'A = {A}, us per call, median [min - max] of {a.rounds} rounds; the eval forward they add to: {EVAL_MS_PER_IMG} ms / image']
    sp = lambda s: f"{s['median']:8.2f} [{s['min']:.2f} - {s['max']:.2f}]"
    for img_h, img_w in ((384, 640), (384, 1248)):
        g = torch.Generator().manual_seed(a.seed)
        sizes = [(img_h // s, img_w // s) for s in STRIDES]
        cm = [torch.randn(B, h, w, A, generator=g).to(dev) for h, w in sizes]
        rm = [(0.1 * torch.randn(B, h, w, 4 * A, generator=g)).to(dev) for h, w in sizes]
        shp = torch.tensor([[float(img_h), float(img_w)]] * B, device=dev)
        for nms_pre in (2000, 1000):
            lens = rpn.candidate_rows(cm, nms_pre)
            cand, valid = rpn.select_decode(cm, rm, shp, STRIDES, bases, nms_pre)
            dets, count, _ = rpn.rpn_proposals(cm, rm, shp, STRIDES, bases, nms_pre, nms_pre)
            kept = count.tolist()
            jobs = [('stage1', lambda: rpn.select_decode(cm, rm, shp, STRIDES, bases, nms_pre)),
                    ('nms_merge', lambda: rpn.nms_segments(cand, valid, lens, nms_pre, 0.7, True)),
                    ('all', lambda: rpn.rpn_proposals(cm, rm, shp, STRIDES, bases, nms_pre, nms_pre))]
            us = {n: [] for n, _ in jobs}
            for _ in range(a.rounds):
                for n, fn in jobs:
                    us[n].append(profiling._graph_time(fn) * 1e6)
            st = {n: stats(v) for n, v in us.items()}
            res = dict(img=[img_h, img_w], maps=sizes, nms_pre=nms_pre, candidates_per_level=lens, proposals=kept, **{n + '_us': s for n, s in st.items()},
                       share_of_eval_forward=round(st['all']['median'] / (EVAL_MS_PER_IMG * 1e3 * B), 3))
            rows.append(f'\n{B} x {img_h} x {img_w}, maps ' + ', '.join(f'{h}x{w}' for h, w in sizes) + f', nms_pre = max_per_img = {nms_pre}: '
                        f'candidates per level {lens}, proposals {kept}')
            rows.append(f"  stage 1 (select + decode) {sp(st['stage1'])}")
            rows.append(f"  stages 2 + 3 (NMS, merge)  {sp(st['nms_merge'])}")
            rows.append(f"  whole call                {sp(st['all'])}   = {st['all']['median'] / B:.1f} us / image, "
                        f"{100 * res['share_of_eval_forward']:.1f} % of the {EVAL_MS_PER_IMG} ms / image eval forward")
            rows.append('  json: ' + json.dumps(res))
    text = '\n'.join(rows) + '\n'
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
