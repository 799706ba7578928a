"""Cost of the wave-group forms of the fused attention forward (csrc/attn_block.hip) and of the fused route
at the head_dim 39 widths: every built form of a width against each other and against the library of ANOTHER tree (--tree DIR:
a checkout of the parent commit with its library built), same box, the variants alternating.

    python tools/attn_fwd_groups_cost.py [--tree DIR] [--iters 200] [--rounds 5] [--legs kernel,net] [--timeout 300]

The driver starts ONE PROCESS PER LEG, each under its own time limit, and stops at the first leg that fails.  JSON lines:
  kernel   per shape (B, H, W, C, heads; self-attention with the CrossFFN head and its moments): us per launch of
           hrf_attn_block_fwd from device events around --iters launches after a warm-up, --rounds alternating rounds; median and
           min-max per variant ('parent' = the library of --tree where it has the width, 'G1' / 'G2' / 'G4' = hrf_debug_knob(36, G)
           on this tree's library), whether every form reproduces G1 bit for bit, and per G > 1 the criterion of the dispatcher's
           default: its median is below the parent's median (this tree's G1 where the parent lacks the width) by more than that
           reference's min-max spread in this run.
  net      eval forward ms per image (hipGraph replay, profiling.time_eval_forward) of a model at --net-size, --rounds rounds per
           process, the processes of the two trees alternating (--net-passes of each); this tree runs with HRF_ATTN_FUSED_D39=1 (the
           head_dim 39 widths on the fused launch, whatever the default of the gate); median and min-max per tree and the
           criterion: this tree's median is below the parent's by more than the parent's spread.
There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 24, 40, 72, 4), (2, 12, 20, 144, 8), (2, 96, 160, 78, 2), (2, 48, 80, 156, 4)]
MODELS = ['t_nus', 'b_nus']


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), rounds=[round(t, 3) for t in v])


def kernel_leg(a):
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('attn_fwd_groups_cost: no GPU - this tool measures on the device and has no CPU path')
    from hrfuser_amd import _lib
    B, H, W, C, heads = (int(v) for v in a.shape.split(','))
    L, s = _lib.lib(), _lib.stream_ptr()
    dev = torch.device('cuda:0')
    variants = []                                                    # (name, library, forced form)
    if a.tree:
        Lp = _lib.Lib(os.path.join(os.path.abspath(a.tree), 'hrfuser_amd', 'libhrfuser_hip.so'))
        if Lp.hrf_attn_block_supported(C, heads):
            variants.append(('parent', Lp, None))
    for g in (1, 2, 4):
        L.hrf_debug_knob(36, g)
        if _lib.attn_fwd_form(C) == g:
            variants.append((f'G{g}', L, g))
    L.hrf_debug_knob(36, 0)
    default_form = _lib.attn_fwd_form(C)
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *sh, k=1.0: (torch.randn(*sh, generator=gen) * k).to(dev)
    rows, N1 = B * H * W, 4 * C
    t = dict(x=rnd(rows, C), lnq_g=rnd(C) + 1, lnq_b=rnd(C, k=0.1), wqkv=rnd(3 * C, C, k=C ** -0.5), bqkv=rnd(3 * C, k=0.1),
             rpb=rnd(169, heads, k=0.5), wo=rnd(C, C, k=C ** -0.5), bo=rnd(C, k=0.1), ln2_g=rnd(C) + 1, ln2_b=rnd(C, k=0.1),
             w1=rnd(N1, C, k=C ** -0.5), b1=rnd(N1, k=0.1))
    outs = {}
    P = _lib._ptr

    def block(name):
        o = outs[name] = dict(out=torch.empty(rows, C, device=dev), h1=torch.empty(rows, N1, device=dev),
                              rowstat=torch.empty(rows, 2, device=dev),
                              stats=torch.zeros(_lib.STAT_COPIES * 2 * N1, dtype=torch.float64, device=dev))
        p = _lib.AttnBlock()
        p.B, p.H, p.W, p.C, p.heads = B, H, W, C, heads
        p.xq = p.xkv = p.res = P(t['x'])
        p.lnq_g, p.lnq_b, p.lnkv_g, p.lnkv_b, p.ln_eps = P(t['lnq_g']), P(t['lnq_b']), P(t['lnq_g']), P(t['lnq_b']), 1e-6
        w, bias = t['wqkv'], t['bqkv']
        p.wq, p.bq = w.data_ptr(), bias.data_ptr()
        p.wk, p.bk = w.data_ptr() + 4 * C * C, bias.data_ptr() + 4 * C
        p.wv, p.bv = w.data_ptr() + 8 * C * C, bias.data_ptr() + 8 * C
        p.rpb, p.wo, p.bo = P(t['rpb']), P(t['wo']), P(t['bo'])
        p.mscale, p.rows_per_sample = 1.0, H * W
        p.out, p.out_rowstat, p.out_eps = P(o['out']), P(o['rowstat']), 1e-6
        p.ln2_g, p.ln2_b, p.w1, p.b1, p.h1, p.stats1, p.hidden = P(t['ln2_g']), P(t['ln2_b']), P(t['w1']), P(t['b1']), P(o['h1']), P(o['stats']), N1
        return p
    blocks = {name: block(name) for name, _, _ in variants}

    def timed(name, lib, g, n):
        if g is not None:
            L.hrf_debug_knob(36, g)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            lib.hrf_attn_block_fwd(blocks[name], s)
        e1.record()
        e1.synchronize()
        L.hrf_debug_knob(36, 0)
        return e0.elapsed_time(e1) * 1e3 / n
    try:
        for v in variants:
            timed(*v, 5)                                             # warm-up: code object, LDS attribute
        us = {name: [] for name, _, _ in variants}
        for _ in range(a.rounds):
            for v in variants:
                us[v[0]].append(timed(*v, a.iters))
    finally:
        L.hrf_debug_knob(36, 0)
    res = dict(what='kernel', shape=[B, H, W, C, heads], windows=B * ((H + 6) // 7) * ((W + 6) // 7), iters=a.iters,
               default_form=default_form)
    for name, _, _ in variants:
        res[name + '_us'] = stats(us[name])
    res['bit_equal_to_G1'] = {name: all(bool(torch.equal(outs[name][k], outs['G1'][k])) for k in ('out', 'h1', 'rowstat'))
                              for name, _, _ in variants if name != 'G1'}
    ref = 'parent' if 'parent_us' in res else 'G1'
    r = res[ref + '_us']
    res['reference'] = ref
    res['reference_spread_us'] = round(r['max'] - r['min'], 3)
    res['criterion'] = {name: dict(speedup=round(r['median'] / res[name + '_us']['median'], 3),
                                   met=bool(r['median'] - res[name + '_us']['median'] > r['max'] - r['min']))
                        for name, _, g in variants if g is not None and g > 1}
    print(json.dumps(res), flush=True)


def net_leg(a):
    tree = os.path.abspath(a.tree) if a.tree else ROOT               # the package, its library and bench.py of THAT tree
    sys.path.insert(0, tree)
    os.chdir(tree)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('attn_fwd_groups_cost: no GPU - this tool measures on the device and has no CPU path')
    import bench
    from hrfuser_amd import profiling
    h, w = (int(v) for v in a.net_size.split('x'))
    args = bench.parse(['--model', a.model, '--height', str(h), '--width', str(w)])
    dev = torch.device('cuda:0')
    _, cfg, stf, H, W, mc, net, B, x, mods, cots, trainer = bench.build_workload(args, 0, 1, dev, None, False)
    ms = [profiling.time_eval_forward(net, x, mods, iters=a.net_iters) for _ in range(a.rounds)]
    print(json.dumps(dict(what='net_rounds', model=a.model, tree='parent' if a.tree else 'this', shape=[B, H, W], iters=a.net_iters,
                          ms_per_img=ms)), flush=True)


def child(a, leg, extra, tree):
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg, '--iters', str(a.iters), '--rounds', str(a.rounds),
           '--net-iters', str(a.net_iters), '--net-size', a.net_size] + extra + (['--tree', tree] if tree else [])
    env = dict(os.environ)
    if leg == 'net' and not tree:
        env['HRF_ATTN_FUSED_D39'] = '1'                # the route this leg is about, whatever its default (runtime._ATTN_FUSED_D39)
    p = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f'attn_fwd_groups_cost: leg {leg} {extra} failed (exit {p.returncode}); nothing further is started')
    return [json.loads(ln) for ln in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default='', help='another checkout (the parent commit) with its library built')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--legs', default='kernel,net')
    ap.add_argument('--timeout', type=float, default=300.0, help='seconds per leg process')
    ap.add_argument('--net-size', default='384x640')
    ap.add_argument('--net-iters', type=int, default=30)
    ap.add_argument('--net-passes', type=int, default=2, help='processes per tree and model, the trees alternating')
    ap.add_argument('--leg', default='', help=argparse.SUPPRESS)       # internal: one leg in this process
    ap.add_argument('--shape', default='', help=argparse.SUPPRESS)
    ap.add_argument('--model', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == 'kernel':
        return kernel_leg(a)
    if a.leg == 'net':
        return net_leg(a)
    if a.rounds < 5:
        raise SystemExit('attn_fwd_groups_cost: --rounds must be at least 5 (the spread is part of the result)')
    legs = a.legs.split(',')
    if 'kernel' in legs:
        for sh in SHAPES:
            for row in child(a, 'kernel', ['--shape', ','.join(str(v) for v in sh)], a.tree):
                print(json.dumps(row), flush=True)
    if 'net' in legs:
        for model in MODELS:
            ms = {'this': [], 'parent': []}
            for _ in range(a.net_passes):
                for tree in ([('parent', a.tree)] if a.tree else []) + [('this', '')]:
                    for row in child(a, 'net', ['--model', model], tree[1]):
                        ms[tree[0]] += row['ms_per_img']
                        shape = row['shape']
            res = dict(what='net', model=model, shape=shape, mode='eval forward, hipGraph replay, ms per image', iters=a.net_iters,
                       this_ms=stats(ms['this']))
            if ms['parent']:
                p, t = stats(ms['parent']), res['this_ms']
                res.update(parent_ms=p, parent_spread_ms=round(p['max'] - p['min'], 4), speedup=round(p['median'] / t['median'], 4),
                           faster_beyond_spread=bool(p['median'] - t['median'] > p['max'] - p['min']),
                           slower_beyond_spread=bool(t['median'] - p['median'] > p['max'] - p['min']))
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
