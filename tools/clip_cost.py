"""Cost of gradient-norm clipping and of gradient accumulation: captured-graph Trainer step, same process, same box.

    python tools/clip_cost.py --model t_nus_bn [--height 384 --width 640] [--steps 50] [--rounds 3]

Prints one JSON line: ms per optimizer step (median over --rounds alternating rounds of --steps replays) of
  default    Trainer(net)                        - hrf_adamw_tick + hrf_adamw
  clip       Trainer(net, max_norm=1e30)         - hrf_grad_sumsq + hrf_adamw_tick_clip + hrf_adamw_clipped, coef = 1: the same
                                                   arithmetic as the default step
  accum2     capture_accumulated of k = 2 micro-batches, clipping on - one optimizer step = two forward / backward passes
and the gradient norm the clipping step reports.  lr = 0 throughout (every replay starts from the same parameters, as bench.py).
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
    a = ap.parse_args()
    import hrfuser_oracle as O
    from hrfuser_amd import build_backbone
    from hrfuser_amd.configs import backbone_cfg
    from hrfuser_amd.trainer import Trainer
    W = a.width or (1248 if 'stf' in a.model else 640)
    dev = torch.device('cuda:0')
    cfg = backbone_cfg(a.model)
    x, mods = O.seeded_inputs(a.batch, a.height, W, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    # one net (engine) per variant: a captured graph carries the addresses of its engine's buffers
    variants = dict(default=dict(), clip=dict(max_norm=1e30), accum2=dict(max_norm=1e30))
    trainers = {}
    for name, kw in variants.items():
        torch.manual_seed(0)
        net = build_backbone(backbone_cfg(a.model)).to(dev)
        net.train()
        with torch.no_grad():
            shapes = [t.shape for t in net(x, list(mods))]
        g = torch.Generator().manual_seed(5)
        cots = [torch.randn(s, generator=g).to(dev) for s in shapes]
        tr = trainers[name] = Trainer(net, lr=0.0, **kw)
        if name == 'accum2':
            tr.capture_accumulated([(x, mods, cots), (x.clone(), [m.clone() for m in mods], cots)])
        else:
            tr.capture(x, mods, cots)
        torch.cuda.synchronize()

    def timed(tr):
        tr.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps
    ms = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name in variants:
            ms[name].append(timed(trainers[name]))
    res = dict(model=a.model, batch=a.batch, height=a.height, width=W, steps=a.steps,
               arena_mb=round(4.0 * trainers['clip'].net._engine().flat_g.numel() / 2 ** 20, 1))
    for name in variants:
        res[name + '_ms'] = [round(v, 3) for v in ms[name]]
        res[name + '_ms_median'] = round(statistics.median(ms[name]), 3)
    res['clip_minus_default_us'] = round(1e3 * (res['clip_ms_median'] - res['default_ms_median']), 1)
    res['grad_norm'] = trainers['clip'].grad_norm()
    res['grad_norm_accum2'] = trainers['accum2'].grad_norm()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
