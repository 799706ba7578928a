"""Cost of the per-head attention forward with LayerNorm and the q / k / v projections in the kernel (csrc/attention.hip
attn_proj_fwd_kernel; runtime.window_attention_proj, width gate HRF_ATTN_PROJ) against the two routes an
attention site has today, same box, the variants alternating.

    python tools/attn_proj_cost.py [--tree DIR] [--iters 200] [--rounds 5] [--legs kernel,net] [--timeout 300]

The driver starts ONE PROCESS PER LEG, each under its own time limit, and stops at the first leg that fails.  JSON lines:
  kernel   per shape (B, H, W, C, heads; self-attention, row statistics of the input given): us per pass over the attention half of a
           block up to the CrossFFN 1x1 expansion, from device events around --iters passes after a warm-up, --rounds alternating
           rounds; median and min-max per route:
             block  hrf_attn_block_fwd without its fc1 head (it emits the row statistics) + fc1 on the row engine          2 launches
             chain  hrf_conv_fwd(LayerNorm on load) -> q | k | v + hrf_window_attn_fwd + out_proj + fc1                    4 launches
             proj   hrf_window_attn_proj_fwd + out_proj + fc1                                                              3 launches
           (out_proj = hrf_conv_fwd with the residual and the row statistics of its output; fc1 = hrf_conv_fwd(LayerNorm on load)
           into the 4C-wide hidden rows: the same two launches in chain and proj), `proj_store` = proj with the q | k | v store of a
           training forward, whether proj reproduces the chain's `out` rows, and the verdict per incumbent: proj "wins" where its
           median is below the incumbent's median by more than the incumbent's min-max spread in this run.
  net      per model and mode (eval: forward ms per image, hipGraph replay, profiling.time_eval_forward; train: ms per captured
           training step, Trainer.capture / replay) at --net-size: gate off against HRF_ATTN_PROJ=<widths>, one process per arm (and
           one per pass of the library of --tree, a checkout of the parent commit with its library built), the arms alternating,
           --net-passes of each; median and min-max per arm and the same verdict against the gate-off arm.
There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 24, 40, 72, 4), (2, 12, 20, 144, 8), (2, 96, 160, 78, 2), (2, 48, 80, 156, 4)]
NETS = [('t_nus', 'eval', '72,144'), ('t_nus', 'train', '72,144'), ('b_nus', 'train', '78,156')]
TF_LN = 4


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), rounds=[round(t, 3) for t in v])


def verdict(ref, new):
    return dict(speedup=round(ref['median'] / new['median'], 3), incumbent_spread=round(ref['max'] - ref['min'], 3),
                wins=bool(ref['median'] - new['median'] > ref['max'] - ref['min']),
                loses=bool(new['median'] - ref['median'] > ref['max'] - ref['min']))


def kernel_leg(a):
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('attn_proj_cost: no GPU - this tool measures on the device and has no CPU path')
    from hrfuser_amd import _lib
    B, H, W, C, heads = (int(v) for v in a.shape.split(','))
    L, s = _lib.lib(), _lib.stream_ptr()
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *sh, k=1.0: (torch.randn(*sh, generator=gen) * k).to(dev)
    rows, N1 = B * H * W, 4 * C
    t = dict(x=rnd(rows, C), lnq_g=rnd(C) + 1, lnq_b=rnd(C, k=0.1), wqkv=rnd(3 * C, C, k=C ** -0.5), bqkv=rnd(3 * C, k=0.1),
             rpb=rnd(169, heads, k=0.5), wo=rnd(C, C, k=C ** -0.5), bo=rnd(C, k=0.1), ln2_g=rnd(C) + 1, ln2_b=rnd(C, k=0.1),
             w1=rnd(N1, C, k=C ** -0.5), b1=rnd(N1, k=0.1))
    stat = torch.empty(rows, 2, device=dev)
    L.hrf_ln_stats(t['x'], rows, C, 1e-6, stat, s)
    strides = (H * W * C, W * C, C, 1)
    P = _lib._ptr
    w, bias = t['wqkv'], t['bqkv']
    wrows = [(w.data_ptr() + 4 * k * C * C, bias.data_ptr() + 4 * k * C) for k in range(3)]
    bufs = {r: dict(qkv=torch.empty(rows, 3 * C, device=dev), o=torch.empty(rows, C, device=dev), out=torch.empty(rows, C, device=dev),
                    rowstat=torch.empty(rows, 2, device=dev), h1=torch.empty(rows, N1, device=dev))
            for r in ('block', 'chain', 'proj', 'proj_store')}

    def tail(b, with_out_proj=True):
        if with_out_proj:
            L.hrf_conv_fwd(b['o'], *strides, B, H, W, C, t['wo'], t['bo'], 1, 1, C, b['out'], C, 0, t['x'], None, C,
                           0, None, None, None, None, None, b['rowstat'], 1e-6, s)
        L.hrf_conv_fwd(b['out'], *strides, B, H, W, C, t['w1'], t['b1'], 1, 1, N1, b['h1'], N1, 0, None, None, 0,
                       TF_LN, t['ln2_g'], t['ln2_b'], b['rowstat'], None, None, None, 0.0, s)

    pb = _lib.AttnBlock()
    pb.B, pb.H, pb.W, pb.C, pb.heads = B, H, W, C, heads
    pb.xq = pb.xkv = pb.res = P(t['x'])
    pb.lnq_g, pb.lnq_b, pb.lnkv_g, pb.lnkv_b, pb.ln_eps = P(t['lnq_g']), P(t['lnq_b']), P(t['lnq_g']), P(t['lnq_b']), 1e-6
    (pb.wq, pb.bq), (pb.wk, pb.bk), (pb.wv, pb.bv) = wrows
    pb.rpb, pb.wo, pb.bo = P(t['rpb']), P(t['wo']), P(t['bo'])
    pb.mscale, pb.rows_per_sample = 1.0, H * W
    pb.out, pb.out_rowstat, pb.out_eps = P(bufs['block']['out']), P(bufs['block']['rowstat']), 1e-6

    def proj_args(b, store):
        p = _lib.AttnProj()
        p.B, p.H, p.W, p.C, p.heads = B, H, W, C, heads
        p.xq = p.xkv = P(t['x'])
        p.lnq_g, p.lnq_b, p.rowstat_q = P(t['lnq_g']), P(t['lnq_b']), P(stat)
        (p.wq, p.bq), (p.wk, p.bk), (p.wv, p.bv) = wrows
        p.rpb, p.o, p.ldo = P(t['rpb']), P(b['o']), C
        if store:
            p.q_out, p.ldq, p.qoff = P(b['qkv']), 3 * C, 0
            p.k_out, p.ldk, p.koff = P(b['qkv']), 3 * C, C
            p.v_out, p.ldv, p.voff = P(b['qkv']), 3 * C, 2 * C
        return p
    pp = {r: proj_args(bufs[r], r == 'proj_store') for r in ('proj', 'proj_store')}

    def run_block():
        L.hrf_attn_block_fwd(pb, s)
        tail(bufs['block'], with_out_proj=False)

    def run_chain():
        b = bufs['chain']
        L.hrf_conv_fwd(t['x'], *strides, B, H, W, C, w, bias, 1, 1, 3 * C, b['qkv'], 3 * C, 0, None, None, 0,
                       TF_LN, t['lnq_g'], t['lnq_b'], stat, None, None, None, 0.0, s)
        L.hrf_window_attn_fwd(b['qkv'], 3 * C, 0, b['qkv'], 3 * C, C, b['qkv'], 3 * C, 2 * C, bias[C:2 * C], bias[2 * C:], t['rpb'],
                              b['o'], C, B, H, W, C, heads, s)
        tail(b)

    def run_proj(r):
        L.hrf_window_attn_proj_fwd(pp[r], s)
        tail(bufs[r])
    routes = [('chain', run_chain), ('proj', lambda: run_proj('proj')), ('proj_store', lambda: run_proj('proj_store'))]
    if L.hrf_attn_block_supported(C, heads):
        routes.insert(0, ('block', run_block))

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n
    for _, fn in routes:
        timed(fn, 5)                                                 # warm-up: code objects, LDS attributes
    us = {name: [] for name, _ in routes}
    for _ in range(a.rounds):
        for name, fn in routes:
            us[name].append(timed(fn, a.iters))
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
    res = dict(what='kernel', shape=[B, H, W, C, heads], windows=B * ((H + 6) // 7) * ((W + 6) // 7), iters=a.iters,
               attn_block_form=_lib.attn_fwd_form(C) if 'block' in us else None)
    for name, _ in routes:
        res[name + '_us'] = stats(us[name])
    res['proj_vs_chain'] = dict(out_bit_equal=bool(torch.equal(bufs['proj']['out'], bufs['chain']['out'])),
                                out_relmax=rel(bufs['proj']['out'], bufs['chain']['out']),
                                h1_relmax=rel(bufs['proj']['h1'], bufs['chain']['h1']),
                                qkv_relmax=rel(bufs['proj_store']['qkv'], bufs['chain']['qkv']))
    res['verdict'] = {inc: verdict(res[inc + '_us'], res['proj_us']) for inc in ('block', 'chain') if inc in us}
    res['verdict_store'] = {'chain': verdict(res['chain_us'], res['proj_store_us'])}
    print(json.dumps(res), flush=True)


def net_leg(a):
    tree = os.path.abspath(a.tree) if a.tree else ROOT               # the package, its library and bench.py of THAT tree
    sys.path.insert(0, tree)
    os.chdir(tree)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('attn_proj_cost: no GPU - this tool measures on the device and has no CPU path')
    import bench
    from hrfuser_amd import profiling
    h, w = (int(v) for v in a.net_size.split('x'))
    args = bench.parse(['--model', a.model, '--height', str(h), '--width', str(w)])
    dev = torch.device('cuda:0')
    _, cfg, stf, H, W, mc, net, B, x, mods, cots, trainer = bench.build_workload(args, 0, 1, dev, None, False)
    if a.mode == 'eval':
        ms = [profiling.time_eval_forward(net, x, mods, iters=a.net_iters) for _ in range(a.rounds)]
    else:
        for _ in range(2):
            trainer.step(x, mods, cots)
        trainer.check()
        trainer.capture(x, mods, cots)
        for _ in range(3):
            trainer.replay()
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.net_iters):
                trainer.replay()
            e1.record()
            e1.synchronize()
            ms.append(round(e0.elapsed_time(e1) / a.net_iters, 4))
        trainer.check()
    print(json.dumps(dict(what='net_rounds', model=a.model, mode=a.mode, gate=os.environ.get('HRF_ATTN_PROJ', ''),
                          tree='parent' if a.tree else 'this', shape=[B, H, W], iters=a.net_iters, ms=ms)), flush=True)


def child(a, leg, extra, tree, gate=''):
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--iters', str(a.iters), '--rounds', str(a.rounds),
           '--net-iters', str(a.net_iters), '--net-size', a.net_size] + extra + (['--tree', tree] if tree else [])
    env = dict(os.environ)
    env['HRF_ATTN_PROJ'] = gate                                      # the arm's width gate, whatever the caller's environment
    p = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f'attn_proj_cost: leg {leg} {extra} failed (exit {p.returncode}); nothing further is started')
    return [json.loads(ln) for ln in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default='', help='another checkout (the parent commit) with its library built: a third arm of the net legs')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--legs', default='kernel,net')
    ap.add_argument('--nets', default='', help='restrict the net legs: comma list of model:mode, e.g. t_nus:eval,b_nus:train')
    ap.add_argument('--timeout', type=float, default=300.0, help='seconds per leg process')
    ap.add_argument('--net-size', default='384x640')
    ap.add_argument('--net-iters', type=int, default=30)
    ap.add_argument('--net-passes', type=int, default=2, help='processes per arm, the arms alternating')
    ap.add_argument('--leg', default='', help=argparse.SUPPRESS)       # internal: one leg in this process
    ap.add_argument('--shape', default='', help=argparse.SUPPRESS)
    ap.add_argument('--model', default='', help=argparse.SUPPRESS)
    ap.add_argument('--mode', default='eval', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == 'kernel':
        return kernel_leg(a)
    if a.leg == 'net':
        return net_leg(a)
    if a.rounds < 5:
        raise SystemExit('attn_proj_cost: --rounds must be at least 5 (the spread is part of the result)')
    legs = a.legs.split(',')
    if 'kernel' in legs:
        for sh in SHAPES:
            for row in child(a, 'kernel', ['--shape', ','.join(str(v) for v in sh)], ''):
                print(json.dumps(row), flush=True)
    if 'net' in legs:
        only = [tuple(v.split(':')) for v in a.nets.split(',') if v]
        for model, mode, gate in NETS:
            if only and (model, mode) not in only:
                continue
            arms = ([('parent', a.tree, '')] if a.tree else []) + [('off', '', ''), ('on', '', gate)]
            ms = {name: [] for name, _, _ in arms}
            for _ in range(a.net_passes):
                for name, tree, g in arms:
                    for row in child(a, 'net', ['--model', model, '--mode', mode], tree, g):
                        ms[name] += row['ms']
                        shape = row['shape']
            unit = 'eval forward, hipGraph replay, ms per image' if mode == 'eval' else 'captured training step, hipGraph replay, ms per step'
            res = dict(what='net', model=model, mode=mode, unit=unit, shape=shape, gate=gate, iters=a.net_iters)
            for name, _, _ in arms:
                res[name + '_ms'] = stats(ms[name])
            res['verdict'] = verdict(res['off_ms'], res['on_ms'])
            if a.tree:
                res['off_vs_parent'] = verdict(res['parent_ms'], res['off_ms'])
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
