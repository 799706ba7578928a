"""Cost of the one-launch backward of the exchange sums (hrf_fuse_sum_bwd, HRF_FUSE_BWD) and of the vector forward kernel
(hrf_fuse_sum), at the row shapes of HRFuser-T at 2 x 384 x 640 and at the training step.  The sections of
profiles/fuse_bwd_cost.txt are this tool's output.

python tools/fuse_bwd_cost.py kernels [rounds]
    Per row shape of the stages 1 x 2, 3 x 3 and 2 x 4 (modules x branches): hrf_fuse_sum_bwd against the launches it replaces
    for the same row (hrf_act_bwd mode 0 + the identity's hrf_scale_add + one hrf_bilinear_up_bwd per up-sampled term), and the
    vector forward kernel against the per-element one (hrf_debug_knob 19 = 1), graph-timed as bench.py times launches, the
    sides ALTERNATING in one process, `rounds` (7) times each; median [min - max] per side.
python tools/fuse_bwd_cost.py step [--parent DIR] [--rounds N] [--model M] [--steps K] [--warmup W]
    bench.py --gpus 1 --steps K --warmup W of the arms `parent` (bench.py and library of the tree exported into DIR, when
    given), `default` (this tree), `0` (this tree, HRF_FUSE_BWD=0) and `off` (HRF_FUSE_BWD=0 and HRF_KNOBS=19=1: the forward
    sums through the per-element kernel too, i.e. the parent's launches from this library), interleaved, N rounds, every run a
    fresh process; then per arm the median of ms_per_step with min - max and the verdict of the criterion: the default arm's
    median below the parent's by more than the parent's min - max spread, the `0` / `off` arms inside it.  The first run that
    fails ends the job."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (H, W, C) of the row, same-resolution terms, low-resolution sizes of the up-sampled terms, exchange sums of this form per step
ROWS = [
    ((96, 160, 18), 0, ((48, 80),), 1),
    ((96, 160, 18), 0, ((48, 80), (24, 40)), 3),
    ((96, 160, 18), 0, ((48, 80), (24, 40), (12, 20)), 2),
    ((48, 80, 36), 1, ((24, 40),), 3),
    ((48, 80, 36), 1, ((24, 40), (12, 20)), 2),
    ((24, 40, 72), 2, ((12, 20),), 2),
    ((48, 80, 36), 1, (), 1),
    ((24, 40, 72), 2, (), 3),
    ((12, 20, 144), 3, (), 2),
]


def _fmt(v):
    return f'{statistics.median(v):6.2f} us [{min(v):6.2f} - {max(v):6.2f}]'


def kernels(rounds):
    import torch
    from hrfuser_amd import _lib
    from hrfuser_amd.profiling import _graph_time
    L = _lib.lib()
    dev = torch.device('cuda:0')
    R = lambda *sh: torch.randn(*sh, device=dev)
    sp, P, KC, B = _lib.stream_ptr, _lib._ptr, _lib.STAT_COPIES, 2
    zst = lambda C: torch.zeros(KC * 2 * C, dtype=torch.float64, device=dev)
    tot = {'fused': 0.0, 'sep': 0.0, 'vec': 0.0, 'elem': 0.0}
    for (H, W, C), nsame, lows, per_step in ROWS:
        dout, out = R(B, H, W, C), R(B, H, W, C)
        ys, sts = [R(B, H, W, C) for _ in range(nsame)], [zst(C) for _ in range(nsame)]
        ylo, du, ust = [R(B, h, w, C) for h, w in lows], [R(B, h, w, C) for h, w in lows], [zst(C) for _ in lows]
        g, idg = torch.empty(B, H, W, C, device=dev), torch.empty(B, H, W, C, device=dev)
        # the identity gradient as the runtime forms it: g itself without a same-resolution term, a fresh tensor next to one
        a = _lib.FuseBwd()
        a.dout, a.out, a.B, a.H, a.W, a.C, a.g = P(dout), P(out), B, H, W, C, P(g)
        if nsame:
            a.id_dst = P(idg)
        for k in range(nsame):
            a.y[k], a.st[k] = P(ys[k]), P(sts[k])
        for k, (h, w) in enumerate(lows):
            a.up_kind[k], a.up_ylow[k], a.up_Hs[k], a.up_Ws[k], a.up_du[k], a.up_stats[k] = 1, P(ylo[k]), h, w, P(du[k]), P(ust[k])
        yy, ss = ys + [None] * 3, sts + [None] * 3

        def fused():
            L.hrf_fuse_sum_bwd(a, sp())

        def sep():
            L.hrf_act_bwd(dout, out, yy[0], None, None, None, 1, 0, g, yy[1], yy[2], ss[0], ss[1], ss[2], B * H * W, C, sp())
            if nsame:
                L.hrf_scale_add(g, None, 1.0, None, 1, None, None, idg, g.numel(), 1, sp())
            for k, (h, w) in enumerate(lows):
                L.hrf_bilinear_up_bwd(g, C, 0, B, H, W, C, ylo[k], h, w, du[k], ust[k], sp())
        # forward: identity + BN-affine same-resolution terms + BN-affine up-sampled terms (at most four)
        sc, sh, x0, o = R(C), R(C), R(B, H, W, C), torch.empty(B, H, W, C, device=dev)
        fa = [1, x0, None, None, 0, 0]
        for k in range(min(nsame, 3 - len(lows))):
            fa += [2, ys[k], sc, sh, 0, 0]
        for k, (h, w) in enumerate(lows):
            fa += [3, ylo[k], sc, sh, h, w]
        fa += [0, None, None, None, 0, 0] * (4 - len(fa) // 6)

        def fwd():
            L.hrf_fuse_sum(*fa, o, B, H, W, C, None, sp())
        t = {'fused': [], 'sep': [], 'vec': [], 'elem': []}
        for _ in range(rounds):
            t['fused'].append(_graph_time(fused) * 1e6)
            t['sep'].append(_graph_time(sep) * 1e6)
            t['vec'].append(_graph_time(fwd) * 1e6)
            L.hrf_debug_knob(19, 1)
            try:
                t['elem'].append(_graph_time(fwd) * 1e6)
            finally:
                L.hrf_debug_knob(19, 0)
        for k in tot:
            tot[k] += statistics.median(t[k]) * per_step
        ok = lambda new, old: 'below the spread' if statistics.median(t[new]) < statistics.median(t[old]) - (max(t[old]) - min(t[old])) \
            else 'NOT below the spread'
        name = f'2x{H}x{W}x{C} same {nsame} ups {"+".join(f"{h}x{w}" for h, w in lows) or "-"} (x{per_step})'
        print(f'{name:52s} bwd fused {_fmt(t["fused"])}   separate ({1 + bool(nsame) + len(lows)} launches) {_fmt(t["sep"])}   {ok("fused", "sep")}',
              flush=True)
        print(f'{"":52s} fwd vector {_fmt(t["vec"])}   per-element {_fmt(t["elem"])}   {ok("vec", "elem")}', flush=True)
    print(f'# per step (19 exchange sums, medians): backward fused {tot["fused"]:.1f} us, separate {tot["sep"]:.1f} us; '
          f'forward vector {tot["vec"]:.1f} us, per-element {tot["elem"]:.1f} us')


def step(args):
    arms = ([('parent', args.parent, {})] if args.parent else []) + [('default', ROOT, {}), ('0', ROOT, {'HRF_FUSE_BWD': '0'}),
                                                                 ('off', ROOT, {'HRF_FUSE_BWD': '0', 'HRF_KNOBS': '19=1'})]
    ms = {name: [] for name, _, _ in arms}
    for rnd in range(1, args.rounds + 1):
        for name, tree, env in arms:
            e = dict(os.environ)
            e.pop('HRF_FUSE_BWD', None)
            e.pop('HRF_KNOBS', None)
            e.update(env)
            cmd = [sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(args.steps), '--warmup', str(args.warmup),
                   '--model', args.model, '--no-cpu-baseline', '--no-neck', '--no-eager', '--no-roofline']
            p = subprocess.run(cmd, cwd=tree, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.timeout)
            if p.returncode != 0:
                print(f'round {rnd} {name}: bench.py exited with {p.returncode}\n{p.stderr[-2000:]}', flush=True)
                return 1
            d = json.loads(p.stdout.strip().splitlines()[-1])
            ms[name].append(d['ms_per_step'])
            s = d['step_ms']
            print(f'round {rnd}  {name:8s} ms_per_step {d["ms_per_step"]:.4f}  step_ms.median {s["median"]:.4f}  p10 {s["p10"]:.4f}  '
                  f'p90 {s["p90"]:.4f}', flush=True)
    for name, v in ms.items():
        print(f'# {name:8s} median {statistics.median(v):.4f} ms [{min(v):.4f} - {max(v):.4f}]')
    if args.parent:
        par = ms['parent']
        spread, med = max(par) - min(par), statistics.median(par)
        gain = med - statistics.median(ms['default'])
        inside = lambda arm: 'inside' if min(par) <= statistics.median(ms[arm]) <= max(par) else 'OUTSIDE'
        print(f'# parent spread {spread:.4f} ms; default below the parent by {gain:.4f} ms ({100 * gain / med:.2f} %): '
              f'{"gain counts" if gain > spread else "NO gain by the criterion"}; HRF_FUSE_BWD=0 {inside("0")} the parent\'s spread, '
              f'with the per-element forward kernel as well {inside("off")}')
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='what', required=True)
    k = sub.add_parser('kernels')
    k.add_argument('rounds', nargs='?', type=int, default=7)
    s = sub.add_parser('step')
    s.add_argument('--parent', default='', help='directory holding the parent commit\'s tree with its library built')
    s.add_argument('--rounds', type=int, default=6)
    s.add_argument('--model', default='t_nus_bn')
    s.add_argument('--steps', type=int, default=50)
    s.add_argument('--warmup', type=int, default=10)
    s.add_argument('--timeout', type=float, default=300.0, help='seconds per bench.py run')
    a = ap.parse_args()
    if a.what == 'kernels':
        kernels(a.rounds)
        return 0
    return step(a)


if __name__ == '__main__':
    sys.exit(main())
