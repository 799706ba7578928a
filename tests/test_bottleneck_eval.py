"""Eval-mode Bottleneck in one launch (csrc/hrf_bneck_eval.h, hrf_bottleneck_eval): resnet.py:263-302 with frozen BatchNorm
statistics against the same block in torch fp64 - through the C ABI on the CPU emulator and on the GPU (ragged grids, maps
smaller than the 4 x 16 tile, a tile whose whole halo lies outside the image, interior tiles, the model's own grid); the block
through Bottleneck.run on the emulator (route on / off / unsupported width); and the whole backbone in eval mode with the
route switched on against the reference-derived goldens.

Bound of the kernel tests: max|out - want| / max|want| < 2e-5, the bound of the sibling kernel (test_ffn_eval.py) - torch's own
fp32 evaluation of the block is at 2.6e-7 ... 5.1e-7 of fp64 on these shapes; a wrong halo value (ReLU(t1) instead of 0), a
dropped tap or a wrong ragged edge is an error of order 0.1."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import hrfuser_oracle as O
from helpers import NORM, ROOT, build_pair, relmax, use_backend
from hrfuser_amd import _lib

GOLD = os.path.join(ROOT, 'tests', 'golden')
# (B, H, W, Cin): Cin = 64 -> with the downsample, Cin = 256 -> identity
CASES = [(1, 5, 7, 64), (1, 5, 7, 256), (1, 3, 5, 64), (1, 4, 16, 256), (2, 9, 21, 256)]
GPU_CASES = CASES + [(2, 17, 33, 64), (1, 96, 160, 256)]


def _block(case):
    """-> (x NHWC fp32, modules in fp32, want NHWC fp64)"""
    B, H, W, Cin = case
    ds = Cin == 64
    g = torch.Generator().manual_seed(B * 100000 + H * 1000 + W * 10 + (1 if ds else 0))
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(B, H, W, Cin)
    convs = [nn.Conv2d(Cin, 64, 1, bias=False), nn.Conv2d(64, 64, 3, 1, 1, bias=False), nn.Conv2d(64, 256, 1, bias=False)]
    bns = [nn.BatchNorm2d(64), nn.BatchNorm2d(64), nn.BatchNorm2d(256)]
    if ds:
        convs.append(nn.Conv2d(Cin, 256, 1, bias=False))
        bns.append(nn.BatchNorm2d(256))
    with torch.no_grad():
        for m in convs:
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.copy_(rn(*m.weight.shape) * math.sqrt(2.0 / fan_in))
        for bn in bns:
            n = bn.num_features
            bn.weight.copy_(1 + 0.3 * rn(n)); bn.bias.copy_(0.2 * rn(n))
            bn.running_mean.copy_(0.3 * rn(n)); bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
    mods = nn.ModuleList(convs + bns).double().eval()
    with torch.no_grad():
        xd = x.double().permute(0, 3, 1, 2)
        y = F.relu(bns[0](convs[0](xd)))
        y = F.relu(bns[1](convs[1](y)))
        y = bns[2](convs[2](y))
        idt = bns[3](convs[3](xd)) if ds else xd
        want = F.relu(y + idt).permute(0, 2, 3, 1).contiguous()
    return x, convs, bns, want


def _args(case, dev, L, keep):
    B, H, W, Cin = case
    ds = Cin == 64
    x, convs, bns, want = _block(case)

    def P(t):
        t = t.detach().float().contiguous().to(dev)
        keep.append(t)
        return t.data_ptr()
    aff = []
    for bn in bns:                                   # the frozen-statistics affine in fp64, cast
        sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        aff.append((sc.float(), (bn.bias.double() - bn.running_mean.double() * sc).float()))
    w2 = convs[1].weight.detach().float().contiguous().to(dev)
    wp = torch.zeros(L.hrf_conv3x_pack_size(64, 64, 0), device=dev)
    keep += [w2, wp]
    jobs = (_lib.Conv3xPackJob * 1)()
    jobs[0] = _lib.Conv3xPackJob(w2.data_ptr(), wp.data_ptr(), 64, 64, 0)
    L.hrf_conv3x_pack(jobs, 1, _lib.stream_ptr() if dev.type == 'cuda' else 0)
    a = _lib.BottleneckEval()
    a.B, a.H, a.W, a.Cin, a.planes, a.has_downsample = B, H, W, Cin, 64, 1 if ds else 0
    a.x = P(x)
    a.w1, a.s1, a.t1 = P(convs[0].weight), P(aff[0][0]), P(aff[0][1])
    a.w2, a.s2, a.t2 = wp.data_ptr(), P(aff[1][0]), P(aff[1][1])
    a.w3, a.s3, a.t3 = P(convs[2].weight), P(aff[2][0]), P(aff[2][1])
    if ds:
        a.wd, a.sd, a.td = P(convs[3].weight), P(aff[3][0]), P(aff[3][1])
    out = torch.full((B, H, W, 256), float('nan'), device=dev)
    a.out = out.data_ptr()
    return a, out, want


def _run(case, backend):
    dev = use_backend(backend)
    L = _lib.lib()
    keep = []
    a, out, want = _args(case, dev, L, keep)
    L.hrf_bottleneck_eval(a, _lib.stream_ptr() if backend == 'hip' else 0)
    if backend == 'hip':
        torch.cuda.synchronize()
    err = float((out.double().cpu() - want).abs().max() / want.abs().max())
    print(f'bottleneck_eval {backend} {case}: err {err:.3e} (max|want| {float(want.abs().max()):.2f})')
    assert err < 2e-5, (case, err)


def _abi(backend):
    dev = use_backend(backend)
    L = _lib.lib()
    assert L.hrf_bottleneck_eval_supported(64, 64, 1) == 1 and L.hrf_bottleneck_eval_supported(256, 64, 0) == 1
    for bad in ((64, 64, 0), (256, 64, 1), (64, 16, 0), (128, 64, 1)):
        assert L.hrf_bottleneck_eval_supported(*bad) == 0, bad
    keep = []
    a, out, _ = _args((1, 5, 7, 64), dev, L, keep)
    s = _lib.stream_ptr() if backend == 'hip' else 0

    def refused():
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_bottleneck_eval(a, s)
        if backend == 'hip':
            torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())          # nothing was launched
    a.has_downsample = 0                             # (64, 64, 0): unsupported
    refused()
    a.has_downsample, a.planes = 1, 16
    refused()
    a.planes, a.H = 64, 0
    refused()
    a.H, a.sd = 5, None                              # a required pointer of the downsample
    refused()


@pytest.mark.parametrize('case', CASES, ids=str)
def test_bottleneck_eval_emul(case):
    _run(case, 'emul')


def test_bottleneck_eval_abi_emul():
    _abi('emul')


@pytest.mark.gpu
@pytest.mark.parametrize('case', GPU_CASES, ids=str)
def test_bottleneck_eval_gpu(case):
    _run(case, 'hip')


@pytest.mark.gpu
def test_bottleneck_eval_abi_gpu():
    _abi('hip')


# ----------------------------------------------------------------------------- the block through Bottleneck.run (emulator)
def _count(monkeypatch, L):
    calls = [0]
    real = L._fns['hrf_bottleneck_eval']

    def counted(*a):
        calls[0] += 1
        return real(*a)
    monkeypatch.setitem(L._fns, 'hrf_bottleneck_eval', counted)
    return calls


def _block_pair(inpl, planes, with_ds):
    import hrfuser_amd.backbone as Bk
    from hrfuser_amd.testing import BlockHarness
    ds = (lambda: nn.Sequential(nn.Conv2d(inpl, 4 * planes, 1, bias=False), nn.BatchNorm2d(4 * planes))) if with_ds else (lambda: None)
    orc = O.Bottleneck(inpl, planes, NORM, ds())
    O.seeded_fill_(orc, 3)
    h = BlockHarness(Bk.Bottleneck(inpl, planes, NORM, ds()), lambda k, b, x: b.run(k, x[0]))
    h.block.load_state_dict(orc.state_dict(), strict=True)
    return h, orc


@pytest.mark.parametrize('inpl,with_ds', [(64, True), (256, False)])
def test_block_route_emul(monkeypatch, inpl, with_ds):
    dev = use_backend('emul')
    calls = _count(monkeypatch, _lib.lib())
    h, orc = _block_pair(inpl, 64, with_ds)
    h.to(dev).eval()
    o64 = copy.deepcopy(orc).double().eval()
    x = torch.randn(2, inpl, 9, 10, generator=torch.Generator().manual_seed(40))
    with torch.no_grad():
        want = o64(x.double())
        h.set_bottleneck_eval(False)
        off = h(x.clone())[0]
        assert calls[0] == 0
        h.set_bottleneck_eval(True)
        on = h(x.clone())[0]
        assert calls[0] == 1
    e_on, e_off = relmax(on, want), relmax(off, want)
    print(f'Bottleneck({inpl}, 64) route on {e_on:.3e}, off {e_off:.3e}')
    assert e_on < 2e-5, e_on
    # a forward with a tape keeps the per-op chain
    h(x.clone().requires_grad_(True))
    assert calls[0] == 1


def test_block_route_unsupported_width_emul(monkeypatch):
    dev = use_backend('emul')
    calls = _count(monkeypatch, _lib.lib())
    h, _ = _block_pair(64, 16, False)
    h.to(dev).eval()
    x = torch.randn(2, 64, 9, 10, generator=torch.Generator().manual_seed(41))
    with torch.no_grad():
        h.set_bottleneck_eval(False)
        off = h(x.clone())[0].clone()
        h.set_bottleneck_eval(True)
        on = h(x.clone())[0].clone()
    assert calls[0] == 0
    assert torch.equal(on, off)


def test_set_bottleneck_eval_drops_graphs():
    import hrfuser_amd.backbone as Bk
    for cls in (Bk.HRFuserHRFormerBased, Bk.HipModule):
        assert callable(getattr(cls, 'set_bottleneck_eval', None)), cls
    h, _ = _block_pair(64, 64, True)
    h.__dict__['_hrf_graphs'] = {}
    h.set_bottleneck_eval(True)
    assert '_hrf_graphs' not in h.__dict__ and h.__dict__['_hrf_bneck_eval'] is True


# ----------------------------------------------------------------------------- whole net on the GPU
def _wholenet(tag, monkeypatch, both):
    dev = use_backend('hip')
    calls = _count(monkeypatch, _lib.lib())
    net, _, cfg = build_pair(tag, dev)
    net.eval()
    x, mods = O.seeded_inputs(2, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    gold = np.load(os.path.join(GOLD, f'wholenet_{tag}.npz'))
    nstreams = 1 + len(mods)

    def fwd():
        with torch.no_grad():
            ys = net(x.to(dev), [m.to(dev) for m in mods])
        assert len(ys) == 4
        for i, y in enumerate(ys):
            e = relmax(y, torch.as_tensor(gold[f'B2_64x96/eval/out{i}']))
            assert e < 1e-3, (tag, i, e)             # the north-star gate
    net.set_bottleneck_eval(True)
    fwd()
    assert calls[0] == 2 * nstreams, calls[0]        # two blocks per sensor stream
    if not both:
        return
    net.set_bottleneck_eval(False)
    fwd()
    assert calls[0] == 2 * nstreams
    # a forward that records a tape keeps the per-op chain (the backward path is untouched)
    net.set_bottleneck_eval(True)
    ys = net(x.to(dev).requires_grad_(True), [m.to(dev) for m in mods])
    assert calls[0] == 2 * nstreams and ys[0].requires_grad


@pytest.mark.gpu
def test_wholenet_route_t_nus_gpu(monkeypatch):
    _wholenet('t_nus', monkeypatch, True)


@pytest.mark.gpu
def test_wholenet_route_b_nus_gpu(monkeypatch):
    _wholenet('b_nus', monkeypatch, False)
