"""What the fused weight-gradient tail adds to a lin_bwd_data launch, against the pair of launches it replaces: for each call-site
shape hrf_conv_bwd_data_weight and (hrf_conv_bwd_weight + hrf_conv_bwd_data) are graph-timed as bench.py times launches,
ALTERNATING in one process, `rounds` times each; median and min - max per side, and the data gradient alone for scale.
out_proj shapes add straight into dw, the fc3 shapes into HRF_STAT_COPIES replicated accumulators (as the engine hands them out).
python tools/bench_lin_fused_wg.py [out.json] [rounds]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hrfuser_amd import _lib                                   # noqa: E402
from hrfuser_amd.profiling import _graph_time                  # noqa: E402

L = _lib.lib()
dev = torch.device('cuda:0')
R = lambda *sh: torch.randn(*sh, device=dev)
sp = _lib.stream_ptr
KC = _lib.STAT_COPIES
# B, H, W, Cin, Cout, site
SHAPES = [(2, 24, 40, 72, 72, 'proj'), (2, 12, 20, 144, 144, 'proj'), (2, 96, 160, 72, 18, 'ffn'), (2, 48, 80, 144, 36, 'ffn'),
          (2, 24, 40, 288, 72, 'ffn')]


def problem(B, H, W, Cin, Cout, site):
    """-> (fused, pair, data) launch closures, or fused = None where the entry point does not take the shape"""
    st = (H * W * Cin, W * Cin, Cin, 1)
    ffn = site == 'ffn'
    dy, yraw, x, w = R(B, H, W, Cout), R(B, H, W, Cout), R(B, H, W, Cin), R(Cout, Cin, 1, 1) * 0.1
    co = [R(Cout) for _ in range(3)] if ffn else [None] * 3
    sc, sh = R(Cin), R(Cin)
    stats = torch.zeros(KC * 2 * Cin, dtype=torch.float64, device=dev)
    dx = torch.zeros(B, H, W, Cin, device=dev)
    n = Cout * Cin + Cout
    acc = torch.zeros(KC * n, device=dev)
    dw, db = torch.zeros(Cout, Cin, device=dev), torch.zeros(Cout, device=dev)
    tail = (0, 1, x, Cin, sc, sh, 2, stats) if ffn else (0, 0, None, 0, None, None, 0, None)
    head = (dy, Cout, 0, yraw if ffn else None, *co, None, w, 1, 1, Cout, B, H, W, Cin, dx, *st, *tail)
    tf = (3, sc, sh) if ffn else (0, None, None)

    def data():
        L.hrf_conv_bwd_data(*head, sp())

    def pair():
        L.hrf_conv_bwd_weight(dy, Cout, 0, yraw if ffn else None, *co, x, *st, B, H, W, Cin, 1, 1, Cout, *tf, None, dw, db, sp())
        L.hrf_conv_bwd_data(*head, sp())
    fused = None
    if L.hrf_conv_bwd_data_weight_supported(Cin, Cout, B * H * W, 1 if ffn else 0, 1 if ffn else 0):
        if ffn:
            fused = lambda: L.hrf_conv_bwd_data_weight(*head, None, 0, acc[:Cout * Cin], acc[Cout * Cin:n], n, sp())
        else:
            fused = lambda: L.hrf_conv_bwd_data_weight(*head, x, Cin, dw, db, 0, sp())
    return fused, pair, data


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else ''
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    rows = {}
    for shp in SHAPES:
        fused, pair, data = problem(*shp)
        t = {'fused': [], 'pair': [], 'data': []}
        for _ in range(rounds):
            for name, fn in (('fused', fused), ('pair', pair), ('data', data)):
                if fn is not None:
                    t[name].append(_graph_time(fn) * 1e6)
        name = 'x'.join(map(str, shp[:3])) + f' {shp[3]}->{shp[4]} {shp[5]}'
        rows[name] = {k: ({'median': statistics.median(v), 'min': min(v), 'max': max(v)} if v else None) for k, v in t.items()}
        f = lambda k: 'not taken' if not t[k] else f'{statistics.median(t[k]):6.2f} us [{min(t[k]):6.2f} - {max(t[k]):6.2f}]'
        print(f'{name:28s} fused {f("fused")}   wgrad + data {f("pair")}   data alone {f("data")}', flush=True)
    if out:
        json.dump(rows, open(out, 'w'), indent=1)


if __name__ == '__main__':
    main()
