"""bf16x3 matrix mode of the wide 3x3 engine (include/hrfuser_hip.h: hrf_conv3_pack_bf16x3 / hrf_conv3_packed_bf16x3,
HRFPN.set_matrix_mode).

Kernel level - every case on the CPU emulator and on the GPU, forward (bias, pad columns) and data gradient (accumulate):
  G1  relmax(kernel, fp64 convolution) <= 5e-5: 9x the worst simulated bf16x3 error (5.7e-6), 40x below the error of one
      bf16 product (1.9e-3 .. 2.6e-3) - a missing cross term fails it;
  G2  relmax(kernel, fp64 sum of the three products hi*hi + hi*lo + lo*hi of the split operands) <= max(2e-6, 8 * e32), e32 =
      the error of the fp32 entry point against the fp64 convolution on the same inputs: the kernel computes exactly that
      model up to fp32 accumulation;
  G3  the two planes of hrf_conv3_pack_bf16x3 are bit-equal to p.bfloat16() and (p - p.bfloat16().float()).bfloat16() of the
      fp32 pack p, both directions.
Module level - HRFPN in 'bf16x3' under the unchanged gates of tests/test_neck.run_case, the route is taken (output bits
differ from 'fp32') and the weight-gradient route is not (bit-equal weight gradients); the mode's interface.
Graph level - an ExtractTrainer step captured in 'bf16x3' replays the eager step and is refused after a switch to 'fp32'.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import helpers as T
import test_neck as TN
from hrfuser_amd import _lib

G1 = 5e-5
CASES = [  # B, H, W, Cin, Cout, forced channel groups per block (0 = dispatcher's choice)
    (2, 9, 17, 64, 64, 0),       # two K slabs (the halo is replaced mid-loop), partial tiles in both axes
    (1, 9, 17, 64, 256, 4),      # four-group form
    (1, 10, 9, 64, 128, 2),      # two-group form
    (1, 5, 7, 96, 64, 1),        # three slabs, a single partial tile
    (1, 3, 40, 64, 320, 0)]      # a block column past N: switched-off waves
GPU_ONLY = (1, 16, 24, 256, 256, 0)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def split(t):
    """fp32 -> (hi, lo) as fp64 tensors holding bf16 values: hi = rne(v), lo = rne(v - hi)."""
    hi = t.bfloat16()
    lo = (t - hi.float()).bfloat16()
    return hi.double(), lo.double()


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs by run_conv3w's law (tests/test_kernels.py: seed 7, x ~ N(0,1), w ~ N(0,1)/(3 sqrt(Cin))) and the fp64
    references, computed once per case and shared by the emulator and the GPU test (never modified)."""
    B, H, W, Cin, Cout, _ = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    prev = torch.randn(B, H, W, Cin, generator=g)
    xd, wd, dyd = x.double(), w.double(), dy.double()
    (xh, xl), (wh, wl), (dh, dl) = split(x), split(w), split(dy)
    conv = lambda a, b: F.conv2d(a, b, None, padding=1)
    dconv = lambda a, b: F.conv_transpose2d(a, b, None, padding=1)       # grad_input of conv2d(., b, padding=1)
    return dict(
        x=x, w=w, bias=bias, dy=dy, prev=prev,
        y64=nhwc(conv(xd, wd) + bias.double().view(1, -1, 1, 1)),
        y3=nhwc(conv(xh, wh) + conv(xh, wl) + conv(xl, wh) + bias.double().view(1, -1, 1, 1)),
        dx64=nhwc(dconv(dyd, wd)),
        dx3=nhwc(dconv(dh, wh) + dconv(dh, wl) + dconv(dl, wh)))


def planes(wp, N, K):
    """The (hi, lo) planes [9][N][K] of a bf16x3 pack: bf16 view [9][N][K/32][2][32] (include/hrfuser_hip.h)."""
    v = wp.cpu().view(torch.bfloat16).view(9, N, K // 32, 2, 32)
    return v[:, :, :, 0, :].reshape(9, N, K), v[:, :, :, 1, :].reshape(9, N, K)


def bits(t):
    return t.contiguous().view(torch.int16)


def run_kernel(case, backend):
    B, H, W, Cin, Cout, wn = case
    ref = reference(case)
    dev = T.use_backend(backend)
    try:
        L, s = _lib.lib(), _lib.stream_ptr()
        D = lambda t: t.detach().to(dev).contiguous()
        L.hrf_debug_knob(24, wn)
        xk, wk, dyk, bk = D(nhwc(ref['x'])), D(ref['w']), D(nhwc(ref['dy'])), D(ref['bias'])
        ld = Cout + 4
        # the data gradient has N = Cin output channels: 96 -> 64 has none on this engine (N % 64 != 0, in either mode;
        # tests/test_kernels.run_conv3w skips it the same way) - the refusal is checked instead
        has_bwd = Cin % 64 == 0
        assert L.hrf_conv3_bf16x3_supported(Cout, Cin) == int(has_bwd)
        res = {}
        for mode, pack, conv in (('fp32', L.hrf_conv3_pack, L.hrf_conv3_packed),
                                 ('bf16x3', L.hrf_conv3_pack_bf16x3, L.hrf_conv3_packed_bf16x3)):
            wp = torch.empty(9 * Cout * Cin, device=dev)
            yk = torch.full((B, H, W, ld), 7.0, device=dev)              # ldY > N: the pad columns must stay untouched
            pack(wk, Cout, Cin, 0, wp, s)
            p0 = wp.clone()
            conv(xk, Cin, wp, bk, yk, ld, 0, B, H, W, Cin, Cout, s)
            dx = D(ref['prev']).clone()
            pack(wk, Cout, Cin, 1, wp, s)
            if has_bwd:
                conv(dyk, Cout, wp, None, dx, Cin, 1, B, H, W, Cout, Cin, s)
            else:
                with pytest.raises(_lib.HRFuserHipError):
                    conv(dyk, Cout, wp, None, dx, Cin, 1, B, H, W, Cout, Cin, s)
                assert torch.equal(dx.cpu(), ref['prev'])
            res[mode] = (p0, wp.clone(), yk.cpu(), dx.cpu())
        # G3: the planes against the split of the fp32 pack, bit for bit, both directions
        for d, (N, K) in enumerate(((Cout, Cin), (Cin, Cout))):
            p = res['fp32'][d].cpu().view(9, N, K)
            hi, lo = planes(res['bf16x3'][d], N, K)
            assert torch.equal(bits(hi), bits(p.bfloat16())), ('G3 hi', d)
            assert torch.equal(bits(lo), bits((p - p.bfloat16().float()).bfloat16())), ('G3 lo', d)
        prev = ref['prev'].double()
        for what, k, r64, r3 in (('fwd', 2, ref['y64'], ref['y3']), ('bwd-data', 3, ref['dx64'], ref['dx3']))[:1 + has_bwd]:
            a32, abf = res['fp32'][k].double(), res['bf16x3'][k].double()
            if what == 'fwd':
                assert float((res['bf16x3'][k][..., Cout:] - 7.0).abs().max()) == 0.0, 'pad columns written'
                a32, abf = a32[..., :Cout], abf[..., :Cout]
            else:
                a32, abf = a32 - prev, abf - prev                         # (exact in fp64: what the kernel added)
            e32, e1, e2 = T.relmax(a32, r64), T.relmax(abf, r64), T.relmax(abf, r3)
            print(f'matrix_mode {backend} {case} {what}: e32 {e32:.2e}  G1 {e1:.2e}  G2 {e2:.2e}  G2/e32 {e2 / e32:.2f}')
            assert e1 <= G1, ('G1', what, e1)
            assert e2 <= max(2e-6, 8 * e32), ('G2', what, e2, e32)
        # refusals: an unsupported K returns HRF_ERR_ARG before any launch, and the query agrees
        assert L.hrf_conv3_bf16x3_supported(Cin, Cout) == 1
        assert L.hrf_conv3_bf16x3_supported(Cin - 1, Cout) == 0 and L.hrf_conv3_bf16x3_supported(Cin, Cout - 1) == 0
        yk = torch.full((B, H, W, ld), 7.0, device=dev)
        with pytest.raises(_lib.HRFuserHipError):
            L.hrf_conv3_packed_bf16x3(xk, Cin, wp, None, yk, ld, 0, B, H, W, Cin - 1, Cout, s)
        assert float((yk - 7.0).abs().max()) == 0.0
    finally:
        _lib.lib().hrf_debug_knob(24, 0)
        T.use_backend('hip')


@pytest.mark.parametrize('case', CASES, ids=str)
def test_kernel_emul(case):
    run_kernel(case, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES + [GPU_ONLY], ids=str)
def test_kernel_gpu(case):
    run_kernel(case, 'hip')


# ---------------------------------------------------------------------------------------------------------------- module
def run_module(name, backend):
    """tests/test_neck.run_case's gates with the neck in 'bf16x3', beside the same neck in 'fp32'."""
    from hrfuser_amd import HRFPN
    dev = T.use_backend(backend)
    try:
        c = TN.CASES[name]
        xs = TN._inputs(c)
        orc, xo, ys, cots = TN._oracle_run(c, xs)
        o64, x64, _, _ = TN._oracle_run(c, xs, dtype=torch.float64)
        got = {}
        for mode in ('fp32', 'bf16x3'):
            net = HRFPN(**TN._ctor(c))
            net.load_state_dict(orc.state_dict())
            net.to(dev).train()
            net.set_matrix_mode(mode)
            assert net.matrix_mode == mode
            xp = [t.detach().clone().to(dev).requires_grad_(True) for t in xs]
            yp = net(xp)
            sum((y * ct.to(dev)).sum() for y, ct in zip(yp, cots)).backward()
            if dev.type == 'cuda':
                torch.cuda.synchronize()
            got[mode] = (net, xp, yp)
        net, xp, yp = got['bf16x3']
        for i, (a, b) in enumerate(zip(yp, ys)):
            assert a.shape == b.shape
            assert T.relmax(a, b) <= 1e-3, (name, 'out', i, T.relmax(a, b))
        for i, (a, b, b32) in enumerate(zip(xp, x64, xo)):
            e, e_ref = T.rel_l2(a.grad, b.grad), T.rel_l2(b32.grad, b.grad)
            assert e <= max(1e-3, 3 * e_ref), (name, 'din', i, e, e_ref)
        T.tight_grad_gate(net.named_parameters(), o64.named_parameters(), orc.named_parameters(), 1e-3,
                          f'neck {name} bf16x3 ({backend})')
        # the route was taken: some output differs in its bits from the fp32 mode's ...
        assert any(not torch.equal(a, b) for a, b in zip(yp, got['fp32'][2])), 'bf16x3 outputs are bit-equal to fp32: route not taken'
        # ... and the weight-gradient route was not: same launches on the same inputs
        p32 = dict(got['fp32'][0].named_parameters())
        n = 0
        for k, p in net.named_parameters():
            if k.startswith('fpn_convs.') and k.endswith('.conv.weight'):
                assert torch.equal(p.grad, p32[k].grad), k
                n += 1
        assert n == net.num_outs
    finally:
        T.use_backend('hip')


def test_module_emul():
    run_module('wide128', 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['t_small', 'b_small'])
def test_module_gpu(name):
    run_module(name, 'hip')


def test_mode_interface():
    from hrfuser_amd import HRFPN
    from hrfuser_amd.detector import FeatureExtractor
    net = HRFPN(in_channels=[18, 36], out_channels=64)
    assert net.matrix_mode == os.environ.get('HRF_MATRIX_MODE', 'fp32')
    net.set_matrix_mode('bf16x3')
    assert net.matrix_mode == 'bf16x3'
    with pytest.raises(ValueError):
        net.set_matrix_mode('tf32')
    assert net.matrix_mode == 'bf16x3'                      # a refused value changes nothing
    with pytest.raises(AttributeError):
        net.matrix_mode = 'fp32'                            # read-only: set_matrix_mode is the switch
    net.set_matrix_mode('fp32')
    assert net.matrix_mode == 'fp32'
    fx = FeatureExtractor(torch.nn.Identity(), net)         # the callers follow their neck
    fx.set_matrix_mode('bf16x3')
    assert fx.matrix_mode == 'bf16x3' and net.matrix_mode == 'bf16x3'
    with pytest.raises(ValueError):
        fx.set_matrix_mode('fp16')


def test_mode_from_environment():
    """HRF_MATRIX_MODE is the initial value of a new HRFPN (a fresh child process: nothing is re-executed here)."""
    code = ('import sys; sys.path.insert(0, %r)\n'
            'from hrfuser_amd import HRFPN\n'
            'print("mode", HRFPN(in_channels=[18, 36], out_channels=64).matrix_mode)\n' % T.ROOT)
    for val, want in (('bf16x3', 'mode bf16x3'),):
        out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, HRF_MATRIX_MODE=val), capture_output=True,
                             text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        assert want in out.stdout, out.stdout
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, HRF_MATRIX_MODE='tf32'), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode != 0 and 'ValueError' in out.stderr


# ----------------------------------------------------------------------------------------------------------------- graph
@pytest.mark.gpu
def test_extract_trainer_graph_gpu():
    """A step captured in 'bf16x3' replays the eager step of that mode (the gates of tests/test_detector.py for eager against
    replay: rel-L2 1e-4 on the neck's arena, 1e-3 on the backbone's) and is refused - not silently replayed - after the
    neck went back to 'fp32', as Trainer.replay refuses a graph of the other deterministic mode."""
    import hrfuser_oracle as O
    import hrfpn_oracle as N
    from hrfuser_amd import HRFPN
    from hrfuser_amd.detector import ExtractTrainer, FeatureExtractor, make_pyramid_cotangents
    dev = T.use_backend('hip')
    bb, orc, cfg = T.build_pair('t_nus', dev)
    norc = N.HRFPNOracle(in_channels=[18, 36, 72, 144], out_channels=256)
    O.seeded_fill_(norc, 11)
    neck = HRFPN(in_channels=[18, 36, 72, 144], out_channels=256)
    neck.load_state_dict(norc.state_dict())
    neck.to(dev)
    fx = FeatureExtractor(bb, neck)
    x, mods = O.seeded_inputs(2, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    fx.train()
    cots = make_pyramid_cotangents(fx, x, mods)
    eb, en = bb._engine(), neck._engine()
    tr = ExtractTrainer(fx, lr=0.0, weight_decay=0.0)        # lr = 0: the parameters stay put, the arenas hold a step's gradients
    outs32 = [o.t.clone() for o in tr.step(x, mods, cots)]
    fx.set_matrix_mode('bf16x3')
    outs = [o.t.clone() for o in tr.step(x, mods, cots)]
    torch.cuda.synchronize()
    gb, gn = eb.flat_g.clone(), en.flat_g.clone()
    assert any(not torch.equal(a, b) for a, b in zip(outs, outs32))      # the eager step took the bf16x3 route
    tr.capture(x, mods, cots)
    eb.flat_g.zero_(); en.flat_g.zero_()
    tr.replay()
    torch.cuda.synchronize()
    assert T.rel_l2(en.flat_g, gn) < 1e-4 and T.rel_l2(eb.flat_g, gb) < 1e-3
    for o, e in zip(tr._graph_outs, outs):
        assert T.rel_l2(o.t, e) < 1e-4
    assert any(not torch.equal(o.t, b) for o, b in zip(tr._graph_outs, outs32))
    fx.set_matrix_mode('fp32')
    keep = en.flat_g.clone()
    with pytest.raises(_lib.HRFuserHipError, match='matrix mode'):
        tr.replay()
    torch.cuda.synchronize()
    assert torch.equal(en.flat_g, keep)                      # nothing was launched
    fx.set_matrix_mode('bf16x3')
    tr.replay()                                              # its own mode again: the graph is still good
    torch.cuda.synchronize()
    assert T.rel_l2(en.flat_g, gn) < 1e-4
