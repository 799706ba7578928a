"""Cost of the eval-mode Bottleneck in one launch (csrc/hrf_bneck_eval.h, hrf_bottleneck_eval; runtime.bottleneck_eval, switch
net.set_bottleneck_eval / HRF_BNECK_EVAL) against the per-op route of the SAME build in the SAME process.

    python tools/bneck_eval_cost.py [--out profiles/bneck_eval_cost.txt] [--rounds 5] [--legs kernel,net] [--timeout 420]

The driver starts ONE PROCESS PER LEG, each under its own time limit, and stops at the first leg that fails.
  kernel   per shape (B, H, W, Cin; Cin = 64: the first block of a stream, with the downsample; 256: the second): a Bottleneck is
           run once on each route through the block harness with every C-ABI call recorded; the recorded launches are then
           re-issued graph-batched (profiling._graph_time: 20 launches per hipGraph, 5 replays, device events), the routes and the
           single launches of the per-op route interleaved, --rounds rounds.  Median and min-max per launch, the per-op SUM
           (the three hrf_conv_fwd / hrf_conv_fwd_packed calls + affine_act_res + the downsample convolution) beside the fused
           launch, achieved TFLOP/s and GB/s of the fused launch on profiling.work_model's algorithmic FLOPs / compulsory bytes,
           and whether the two routes agree (relmax of the outputs).
  net      per model: eval forward ms per image (profiling.time_eval_forward: hipGraph replay of the whole forward) with the
           route off and on in one process, alternating, --rounds rounds each; the C-ABI launches per forward on both routes.
There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 96, 160, 64), (2, 96, 160, 256), (2, 96, 312, 64), (2, 96, 312, 256)]
NETS = ['t_nus_bn', 'b_nus_bn', 't_stf_bn']
PER_OP = ('hrf_conv_fwd', 'hrf_conv_fwd_packed', 'hrf_affine_act_res')


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bneck_eval_cost: no GPU - this tool measures on the device and has no CPU path')
    return torch


def _record(fn):
    """-> the C-ABI calls `fn` issues: [(entry point, described arguments, raw arguments)]"""
    from hrfuser_amd import _lib, profiling
    real = _lib.lib
    prof = profiling.ProfLib(real(), timing=False)
    _lib.lib = lambda: prof
    try:
        fn()
    finally:
        _lib.lib = real
    return prof.records


def kernel_leg(a):
    sys.path.insert(0, ROOT)
    torch = _need_gpu()
    import torch.nn as nn
    os.environ['HRF_LANES'] = '0'
    from hrfuser_amd import _lib, profiling
    import hrfuser_amd.backbone as Bk
    from hrfuser_amd.testing import BlockHarness
    B, H, W, Cin = (int(v) for v in a.shape.split(','))
    dev = torch.device('cuda:0')
    norm = dict(type='BN', requires_grad=True, momentum=0.1)
    torch.manual_seed(3)
    ds = nn.Sequential(nn.Conv2d(Cin, 256, 1, bias=False), nn.BatchNorm2d(256)) if Cin == 64 else None
    blk = Bk.Bottleneck(Cin, 64, norm, ds)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.3); m.bias.normal_(0.0, 0.2)
                m.running_mean.normal_(0.0, 0.3); m.running_var.uniform_(0.5, 1.5)
    # channels-last on the device and held for the whole leg: the harness reads it in place, so the raw pointer in the recorded
    # argument struct stays valid (a temporary NHWC copy would be returned to the allocator after the forward and unmapped by the
    # empty_cache() every graph capture starts with)
    xd = torch.randn(B, Cin, H, W).to(dev).contiguous(memory_format=torch.channels_last)
    # one harness per route: the buffers of a forward live until the next forward of the same engine
    hs, recs, outs = {}, {}, {}
    for route in ('per_op', 'fused'):
        import copy
        h = hs[route] = BlockHarness(copy.deepcopy(blk), lambda k, b, xs: b.run(k, xs[0])).to(dev).eval()
        h.set_bottleneck_eval(route == 'fused')
        with torch.no_grad():
            h(xd)                                                 # warm-up: code objects, LDS attribute
            torch.cuda.synchronize()
            box = []
            recs[route] = _record(lambda: box.append(h(xd)[0]))
            torch.cuda.synchronize()
            outs[route] = box[0]
    L = _lib.lib()
    per_op = [(n, d, c) for n, d, c in recs['per_op'] if n in PER_OP]
    fused = [(n, d, c) for n, d, c in recs['fused'] if n == 'hrf_bottleneck_eval']
    assert len(fused) == 1 and len(per_op) == (5 if Cin == 64 else 4), ([r[0] for r in recs['fused']], [r[0] for r in recs['per_op']])
    assert not any(n in PER_OP for n, _, _ in recs['fused'])
    assert fused[0][2][0].x == xd.data_ptr()                      # the replayed launches read the tensor held above, not a dead copy
    issue = lambda n, c: getattr(L, n)(*c[:-1], _lib.stream_ptr())
    jobs = [('fused', lambda: issue(*fused[0][::2]))]
    jobs.append(('per_op_chain', lambda: [issue(n, c) for n, _, c in per_op]))
    for k, (n, d, c) in enumerate(per_op):
        jobs.append((f'{k}:{profiling.shape_tag(n, d)}', lambda n=n, c=c: issue(n, c)))
    us = {name: [] for name, _ in jobs}
    for _ in range(a.rounds):
        for name, fn in jobs:
            reps = 20 if name != 'per_op_chain' else 4            # (the chain: 4 x its 4 / 5 launches per graph)
            us[name].append(profiling._graph_time(fn, reps=reps) * 1e6)
    key, fl, by = profiling.work_model('hrf_bottleneck_eval', fused[0][1])
    med = statistics.median(us['fused'])
    singles = [name for name, _ in jobs[2:]]
    ssum = [sum(us[n][r] for n in singles) for r in range(a.rounds)]
    res = dict(what='kernel', shape=[B, H, W, Cin], kernel=key, rounds=a.rounds, fused_us=stats(us['fused']),
               per_op_sum_us=stats(ssum), per_op_chain_us=stats(us['per_op_chain']),
               per_op_launches={n: stats(us[n]) for n in singles},
               fused_tflops=round(fl / med / 1e6, 2), fused_gbs=round(by / med / 1e3, 1), gflop=round(fl / 1e9, 3), mbytes=round(by / 1e6, 2),
               routes_relmax=float((outs['fused'] - outs['per_op']).abs().max() / outs['per_op'].abs().max()))
    print(json.dumps(res), flush=True)


def net_leg(a):
    sys.path.insert(0, ROOT)
    os.chdir(ROOT)
    os.environ['HRF_MODULE_GRAPH'] = '0'                          # the timed graph is time_eval_forward's own
    torch = _need_gpu()
    import bench
    from hrfuser_amd import profiling
    args = bench.parse(['--model', a.model])
    dev = torch.device('cuda:0')
    _, cfg, stf, H, W, mc, net, B, x, mods, cots, trainer = bench.build_workload(args, 0, 1, dev, None, False)
    net.eval()
    census, outs = {}, {}
    for on in (False, True):
        net.set_bottleneck_eval(on)
        with torch.no_grad():
            net(x, list(mods))
            torch.cuda.synchronize()
            box = []
            recs = _record(lambda: box.append(net(x, list(mods))))
            torch.cuda.synchronize()
        outs[on] = [t.clone() for t in box[0]]
        census[on] = dict(launches=len(recs), bottleneck_eval=sum(1 for n, _, _ in recs if n == 'hrf_bottleneck_eval'),
                          conv_fwd=sum(1 for n, _, _ in recs if n in ('hrf_conv_fwd', 'hrf_conv_fwd_packed')),
                          affine_act_res=sum(1 for n, _, _ in recs if n == 'hrf_affine_act_res'))
    ms = {False: [], True: []}
    for _ in range(a.rounds):
        for on in (False, True):
            net.set_bottleneck_eval(on)
            ms[on].append(profiling.time_eval_forward(net, x, mods, iters=a.net_iters))
    rel = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(outs[True], outs[False]))
    print(json.dumps(dict(what='net', model=a.model, shape=[B, H, W], unit='eval forward, hipGraph replay, ms per image', iters=a.net_iters,
                          rounds=a.rounds, off_ms=stats(ms[False]), on_ms=stats(ms[True]), off_rounds=ms[False], on_rounds=ms[True],
                          launches_off=census[False], launches_on=census[True], outputs_relmax_on_vs_off=rel)), flush=True)


def child(a, leg, extra):
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--rounds', str(a.rounds), '--net-iters', str(a.net_iters)] + extra
    p = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f'bneck_eval_cost: leg {leg} {extra} failed (exit {p.returncode}); nothing further is started')
    return [json.loads(ln) for ln in lines]


def fmt(r):
    sp = lambda s: f"{s['median']:8.2f} [{s['min']:.2f} - {s['max']:.2f}]"
    if r['what'] == 'kernel':
        B, H, W, Cin = r['shape']
        out = [f"{B} x {H} x {W}, Cin {Cin} ({'with downsample' if Cin == 64 else 'identity'}), {r['kernel']}, us per launch, median [min - max] of {r['rounds']} rounds",
               f"  fused launch          {sp(r['fused_us'])}   {r['fused_tflops']:.2f} TFLOP/s, {r['fused_gbs']:.1f} GB/s ({r['gflop']} GFLOP, {r['mbytes']} MB compulsory)",
               f"  per-op launches, sum  {sp(r['per_op_sum_us'])}   ({len(r['per_op_launches'])} launches timed one by one)",
               f"  per-op chain          {sp(r['per_op_chain_us'])}   (the same launches back to back in one graph, per pass)"]
        out += [f"    {sp(s)}  {n}" for n, s in r['per_op_launches'].items()]
        out.append(f"  fused / per-op sum = {r['fused_us']['median'] / r['per_op_sum_us']['median']:.3f}, fused / chain = "
                   f"{r['fused_us']['median'] / r['per_op_chain_us']['median']:.3f}; outputs of the two routes: relmax {r['routes_relmax']:.2e}")
        return '\n'.join(out)
    B, H, W = r['shape']
    lo, ln = r['launches_off'], r['launches_on']
    sp = lambda s: f"{s['median']:7.3f} [{s['min']:.3f} - {s['max']:.3f}]"
    return '\n'.join([
        f"{r['model']} {B} x {H} x {W}: eval forward ms per image (hipGraph replay, {r['iters']} replays per round), median [min - max] of {r['rounds']} alternating rounds",
        f"  route off {sp(r['off_ms'])}   {lo['launches']} C-ABI launches per forward ({lo['conv_fwd']} conv_fwd, {lo['affine_act_res']} affine_act_res, {lo['bottleneck_eval']} bottleneck_eval)",
        f"  route on  {sp(r['on_ms'])}   {ln['launches']} C-ABI launches per forward ({ln['conv_fwd']} conv_fwd, {ln['affine_act_res']} affine_act_res, {ln['bottleneck_eval']} bottleneck_eval)",
        f"  on / off = {r['on_ms']['median'] / r['off_ms']['median']:.4f}; outputs on vs off: relmax {r['outputs_relmax_on_vs_off']:.2e}"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bneck_eval_cost.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--legs', default='kernel,net')
    ap.add_argument('--nets', default=','.join(NETS))
    ap.add_argument('--timeout', type=float, default=420.0, help='seconds per leg process')
    ap.add_argument('--net-iters', type=int, default=30)
    ap.add_argument('--leg', default='', help=argparse.SUPPRESS)       # internal: one leg in this process
    ap.add_argument('--shape', default='', help=argparse.SUPPRESS)
    ap.add_argument('--model', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == 'kernel':
        return kernel_leg(a)
    if a.leg == 'net':
        return net_leg(a)
    if a.rounds < 5:
        raise SystemExit('bneck_eval_cost: --rounds must be at least 5 (the spread is part of the result)')
    rows = []

    def emit(text):
        print(text, flush=True)
        rows.append(text)
        if a.out:                                                     # rewritten after every leg: a leg that fails keeps what came before
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                fh.write('\n'.join(rows) + '\n')
    emit('tools/bneck_eval_cost.py: eval-mode Bottleneck in one launch (hrf_bottleneck_eval) against the per-op route, same build, same process')
    legs = a.legs.split(',')
    if 'kernel' in legs:
        emit('\n== 1. isolated launches (graph-batched, device events) ==')
        for sh in SHAPES:
            for r in child(a, 'kernel', ['--shape', ','.join(str(v) for v in sh)]):
                emit(fmt(r))
                emit('  json: ' + json.dumps(r))
    if 'net' in legs:
        emit('\n== 2. eval forward, route off / on alternating in one process ==')
        for model in a.nets.split(','):
            for r in child(a, 'net', ['--model', model]):
                emit(fmt(r))
                emit('  json: ' + json.dumps(r))


if __name__ == '__main__':
    main()
