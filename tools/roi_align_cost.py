"""Cost of the multi-level RoIAlign launches (csrc/hrf_roi.h: hrf_roi_align_fwd / hrf_roi_align_bwd; hrfuser_amd/roi.py; DESIGN.md
section 16) against their own traffic floors.

    python tools/roi_align_cost.py [--out profiles/roi_align_cost.txt] [--rounds 5]

One process.  Pyramid of HRFuser-T nus at 2 x 384 x 640 (maps 96x160 ... 12x20, 256 channels, strides 4 ... 32), K = 1024 boxes
(the training sampler's 512 per image) and K = 2000 (1000 test proposals per image); box sides log-uniform in 16 ... 512 px from a
seed, centres uniform in the image.  Every launch is timed graph-batched (profiling._graph_time: 20 launches per hipGraph, 5
replays, device events) after a warm-up launch, --rounds rounds: median [min - max].

Bytes a launch must move at least (computed on the host from the same boxes):
  forward   the clipped footprint of every box read once + K * 49 * C * 4 written;
  backward  dout read + the footprint bytes added with fp32 atomics.
and what the measured time makes of them: GB/s and the fraction of the measured HBM copy rate (6.29 TB/s) resp., for the
backward's atomic bytes, of the chip-wide float-atomic rate (1.3 TB/s of added bytes).  The backward's floor is its atomic bytes
over that rate.  There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS, ATOMIC_TBS = 6.29, 1.3
B, IMG_H, IMG_W, C = 2, 384, 640, 256
STRIDES = [4, 8, 16, 32]


def make_boxes(K, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(K, 4, generator=g)
    w = torch.exp(math.log(16.0) + u[:, 0] * math.log(512.0 / 16.0))
    h = torch.exp(math.log(16.0) + u[:, 1] * math.log(512.0 / 16.0))
    cx, cy = u[:, 2] * IMG_W, u[:, 3] * IMG_H
    b = (torch.arange(K) % B).float()
    return torch.stack([b, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)


def footprint_pixels(rois):
    """Sum over the boxes of the pixels their valid samples touch (rows x columns of the clipped footprint), and per level."""
    from hrfuser_amd.testing import roi_level_ref, roi_samples
    lv = roi_level_ref(rois, len(STRIDES)).tolist()
    tot, per = 0, [0] * len(STRIDES)

    def span(vals, n):
        ok = [min(max(v, 0.0), n - 1.0) for r in vals for v in r if -1.0 <= v <= n]
        if not ok:
            return 0
        lo, hi = int(min(ok)), int(max(ok))
        return min(hi + 1, n - 1) - lo + 1
    for r, l in zip(rois.tolist(), lv):
        H, W = IMG_H // STRIDES[l], IMG_W // STRIDES[l]
        ys, xs, _ = roi_samples(r[1:], 1.0 / STRIDES[l], H, W)
        p = span(ys, H) * span(xs, W)
        tot += p
        per[l] += 1
    return tot, per


def stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'roi_align_cost.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=11)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('roi_align_cost: no GPU - this tool measures on the device and has no CPU path')
    from hrfuser_amd import profiling, roi
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(a.seed)
    maps = [torch.randn(B, IMG_H // s, IMG_W // s, C, generator=g).to(dev) for s in STRIDES]
    scales = tuple(1.0 / s for s in STRIDES)
    rows = ['tools/roi_align_cost.py: hrf_roi_align_fwd / hrf_roi_align_bwd, pyramid '
            + ', '.join(f'{IMG_H // s}x{IMG_W // s}' for s in STRIDES) + f' x {C} (B = {B}), us per launch, median [min - max] of {a.rounds} rounds']
    sp = lambda s: f"{s['median']:8.2f} [{s['min']:.2f} - {s['max']:.2f}]"
    for K in (1024, 2000):
        rois_h = make_boxes(K, a.seed + K)
        pix, per = footprint_pixels(rois_h)
        rois = rois_h.to(dev)
        fp_bytes, out_bytes = pix * C * 4.0, K * 49 * C * 4.0
        rows.append(f'\nK = {K}: boxes per level {per}, clipped footprints {pix} pixels = {fp_bytes / 1e6:.1f} MB, output {out_bytes / 1e6:.1f} MB')
        for layout in (0, 1):
            out = roi.roi_forward(maps, rois, scales, 56.0, layout)
            dout = torch.randn(out.shape, device=dev)
            dmaps = [torch.zeros_like(m) for m in maps]
            jobs = [('fwd', lambda: roi.roi_forward(maps, rois, scales, 56.0, layout, out=out)),
                    ('bwd', lambda: roi.roi_backward(maps, dmaps, rois, scales, dout, 56.0, layout))]
            us = {n: [] for n, _ in jobs}
            for _ in range(a.rounds):
                for n, fn in jobs:
                    us[n].append(profiling._graph_time(fn) * 1e6)
            f, b = stats(us['fwd']), stats(us['bwd'])
            fby, bby = fp_bytes + out_bytes, out_bytes + fp_bytes
            floor = fp_bytes / (ATOMIC_TBS * 1e6)                     # us
            res = dict(K=K, out_layout=layout, fwd_us=f, bwd_us=b, fwd_mbytes=round(fby / 1e6, 1), bwd_atomic_mbytes=round(fp_bytes / 1e6, 1),
                       fwd_gbs=round(fby / f['median'] / 1e3, 1), bwd_atomic_gbs=round(fp_bytes / b['median'] / 1e3, 1),
                       bwd_atomic_floor_us=round(floor, 2))
            rows.append(f"  out_layout {layout}: forward  {sp(f)}   {fby / 1e6:.1f} MB -> {res['fwd_gbs']:.0f} GB/s = "
                        f"{res['fwd_gbs'] / (HBM_TBS * 1e3):.2f} of the measured HBM copy rate")
            rows.append(f"                backward {sp(b)}   {fp_bytes / 1e6:.1f} MB added (+ {out_bytes / 1e6:.1f} MB dout read) -> {res['bwd_atomic_gbs']:.0f} GB/s "
                        f"of atomic bytes = {res['bwd_atomic_gbs'] / (ATOMIC_TBS * 1e3):.2f} of the float-atomic rate; floor {floor:.1f} us, "
                        f"measured / floor = {b['median'] / floor:.2f}")
            rows.append('  json: ' + json.dumps(res))
    text = '\n'.join(rows) + '\n'
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
