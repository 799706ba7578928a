"""Cost of the deterministic mode: captured-graph Trainer step, default mode versus deterministic mode, same
process, same box.

    python tools/det_cost.py --model t_nus_bn [--height 384 --width 640] [--steps 50] [--rounds 3] [--only default|deterministic]

Prints one JSON line: ms/step of both modes (median over --rounds alternating rounds of --steps replays), the device memory
each mode's net + captured Trainer allocates (torch allocator) beside the computed size of the shadow bins, and whether the
gradient arena of two deterministic replays is bit-identical.  --only builds and replays ONE mode: the form to put under
`rocprofv3 --kernel-trace --stats`, one run per mode, to see which kernels carry the difference.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='t_nus_bn')
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--width', type=int, default=0)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', choices=['default', 'deterministic'], default=None)
    a = ap.parse_args()
    import hrfuser_oracle as O
    from hrfuser_amd import build_backbone
    from hrfuser_amd.configs import backbone_cfg
    from hrfuser_amd.trainer import Trainer
    W = a.width or (1248 if 'stf' in a.model else 640)
    dev = torch.device('cuda:0')
    from hrfuser_amd import _lib
    L = _lib.lib()
    cfg = backbone_cfg(a.model)
    x, mods = O.seeded_inputs(a.batch, a.height, W, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    # one net (engine, step tables) per mode: the two modes lay the engine's step tables out differently, so their graphs must
    # not share an engine; the mode is process-wide but only read when launches are ISSUED, i.e. while capturing
    nets, trainers, mem = {}, {}, {}
    modes = (False, True) if a.only is None else (a.only == 'deterministic',)
    for det in modes:
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        torch.manual_seed(0)
        net = nets[det] = build_backbone(backbone_cfg(a.model)).to(dev)
        net.train()
        net.set_deterministic(det)
        with torch.no_grad():
            shapes = [t.shape for t in net(x, list(mods))]
        g = torch.Generator().manual_seed(5)
        cots = [torch.randn(s, generator=g).to(dev) for s in shapes]
        tr = trainers[det] = Trainer(net, lr=0.0)      # lr = 0: every replay starts from the same parameters (as bench.py)
        tr.capture(x, mods, cots)
        torch.cuda.synchronize()
        mem[det] = round((torch.cuda.memory_allocated() - m0) / 2 ** 20, 1)
    eng = nets[modes[-1]]._engine()

    def timed(det):
        L.hrf_set_deterministic(1 if det else 0)       # (what Trainer.replay checks; a replay issues nothing)
        tr = trainers[det]
        tr.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps
    ms = {det: [] for det in modes}
    for _ in range(a.rounds):
        for det in modes:
            ms[det].append(timed(det))
    res = dict(model=a.model, batch=a.batch, height=a.height, width=W)
    for det in modes:
        name = 'deterministic' if det else 'default'
        res[name + '_ms'] = [round(v, 3) for v in ms[det]]
        res[name + '_ms_median'] = round(statistics.median(ms[det]), 3)
        res[name + '_allocated_mb'] = mem[det]
    if a.only is None:                                 # (not under a profiler: both runs then hold the same number of steps)
        L.hrf_set_deterministic(1)
        trainers[True].replay()
        torch.cuda.synchronize()
        g0 = eng.flat_g.clone()
        trainers[True].replay()
        torch.cuda.synchronize()
        res['deterministic_replays_bitwise_equal'] = bool(torch.equal(g0.view(torch.int32), eng.flat_g.view(torch.int32)))
        res['shadow_bins_mb'] = round(32.0 * (eng.flat_g.numel() + eng.ps_n) / 2 ** 20, 1)
    L.hrf_set_deterministic(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
