"""Cost and effect of the bf16x3 matrix mode: the wide 3x3 kernel and the HRFPN neck, 'fp32' against
'bf16x3', same process, same box, the two modes alternating.

    python tools/matrix_mode_cost.py [--batch 2 --height 96 --width 160 --channels 256] [--iters 200] [--rounds 5]
                                     [--only fp32|bf16x3] [--no-neck]

Prints JSON lines:
  kernel   per direction (forward: bias; data gradient: the dir = 1 pack): us per launch of hrf_conv3_packed and of
           hrf_conv3_packed_bf16x3 from device events around --iters launches after a warm-up, --rounds alternating rounds;
           median and min-max per mode, relmax between the two modes' outputs, and the speed criterion: the bf16x3 median is below
           the fp32 median by more than the fp32 min-max spread of this run.
  neck     ms per eager forward + backward of the HRFuser-T neck (in_channels 18/36/72/144 -> 256, five levels) in both modes,
           and relmax between the two modes' outputs.
--only times ONE mode (kernels only): the form to put under `rocprofv3 --kernel-trace --stats -- python tools/matrix_mode_cost.py
--only ...`, one run per mode, no other tracing beside it.  There is no CPU path: without a GPU the tool fails.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MODES = ('fp32', 'bf16x3')


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), rounds=[round(t, 3) for t in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--height', type=int, default=96)
    ap.add_argument('--width', type=int, default=160)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', choices=MODES, default=None)
    ap.add_argument('--no-neck', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('matrix_mode_cost: no GPU - this tool measures on the device and has no CPU path')
    if a.rounds < 5 and a.only is None:
        raise SystemExit('matrix_mode_cost: --rounds must be at least 5 (the spread is part of the result)')
    from hrfuser_amd import _lib
    L, s = _lib.lib(), _lib.stream_ptr()
    dev = torch.device('cuda:0')
    B, H, W, C = a.batch, a.height, a.width, a.channels
    modes = MODES if a.only is None else (a.only,)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, C, generator=g).to(dev)
    w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    dy = torch.randn(B, H, W, C, generator=g).to(dev)
    fns = {'fp32': (L.hrf_conv3_pack, L.hrf_conv3_packed), 'bf16x3': (L.hrf_conv3_pack_bf16x3, L.hrf_conv3_packed_bf16x3)}

    for direction, src, b_, d in (('forward', x, bias, 0), ('data_gradient', dy, None, 1)):
        packs, outs = {}, {}
        for m in modes:
            packs[m] = torch.empty(9 * C * C, device=dev)
            fns[m][0](w, C, C, d, packs[m], s)
            outs[m] = torch.empty(B, H, W, C, device=dev)

        def timed(m, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fns[m][1](src, C, packs[m], b_, outs[m], C, 0, B, H, W, C, C, s)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n
        for m in modes:
            timed(m, 5)                                  # warm-up: code object, LDS attribute
        us = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                us[m].append(timed(m, a.iters))
        res = dict(what='kernel', direction=direction, shape=[B, H, W, C, C], iters=a.iters, flop=2.0 * 9 * B * H * W * C * C)
        for m in modes:
            res[m + '_us'] = stats(us[m])
            res[m + '_tflops'] = round(res['flop'] / (res[m + '_us']['median'] * 1e-6) / 1e12, 1)
        if a.only is None:
            f, h = res['fp32_us'], res['bf16x3_us']
            res['relmax_bf16x3_vs_fp32'] = relmax(outs['bf16x3'], outs['fp32'])
            res['fp32_spread_us'] = round(f['max'] - f['min'], 3)
            res['speedup'] = round(f['median'] / h['median'], 3)
            res['speed_criterion_met'] = bool(f['median'] - h['median'] > f['max'] - f['min'])
        print(json.dumps(res), flush=True)

    if a.no_neck or a.only is not None:
        return
    from hrfuser_amd import HRFPN
    chans = [18, 36, 72, 144]
    torch.manual_seed(0)
    net = HRFPN(in_channels=chans, out_channels=C).to(dev)
    net.init_weights()
    net.train()
    xs = [torch.randn(B, ch, H >> i, W >> i, generator=g).to(dev).requires_grad_(True) for i, ch in enumerate(chans)]
    cots = None

    def step(m):
        nonlocal cots
        net.set_matrix_mode(m)
        ys = net(xs)
        if cots is None:
            cots = [torch.randn(y.shape, generator=g).to(dev) for y in ys]
        sum((y * c).sum() for y, c in zip(ys, cots)).backward()
        return ys

    def timed_steps(m, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step(m)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n
    ys = {}
    for m in MODES:
        for _ in range(3):
            ys[m] = [y.detach().clone() for y in step(m)]
    n = max(5, a.iters // 5)
    ms = {m: [] for m in MODES}
    for _ in range(a.rounds):
        for m in MODES:
            ms[m].append(timed_steps(m, n))
    res = dict(what='neck', config='T', shape=[B, H, W], steps=n, mode_of='eager forward + backward (autograd boundary included)')
    for m in MODES:
        res[m + '_ms'] = stats(ms[m])
    res['relmax_bf16x3_vs_fp32'] = [relmax(p, q) for p, q in zip(ys['bf16x3'], ys['fp32'])]
    res['speedup'] = round(res['fp32_ms']['median'] / res['bf16x3_ms']['median'], 3)
    net.set_matrix_mode('fp32')
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
