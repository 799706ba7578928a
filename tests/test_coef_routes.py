"""Width envelope of the per-channel coefficient routes (include/hrfuser_hip.h).

Every dense kernel applies the preceding BatchNorm on load; its coefficients arrive either finalised in the kernel prologue
(hrf_bn_fin_t / hrf_bn_bfin_t: 'fin') or as plain arrays ('array').  Each kernel stages them in a fixed-size LDS array whose
size differs per file (HRF_C3X_MAXC = 256 in the packed 3x3 engine, HRF_FIN_MAXC = 576 in the other convolution engines and
the pointwise kernels, half of that per term in hrf_fuse_sum, 32-channel blocks in the depthwise kernels).  A write past a
__shared__ array is silent on the GPU, so each entry point is run AT its bound and PAST it, on both routes: taken calls
against a float64 reference at test_kernels.TOL, calls the contract does not take refused with HRF_ERR_ARG before anything
is launched (test_kernels.refused: the NaN-filled output stays NaN).  Few pixels (one ragged tile), so the emulator affords
the widths."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from helpers import use_backend
from hrfuser_amd import _lib
from test_kernels import (TOL, _pack3x, check_bfin, check_fin, make_bfin, make_fin, nhwc, r, refused, run_conv, run_dw, run_lin2)

C3X, FIN = _lib.C3X_MAXC, _lib.FIN_MAXC
ROUTES = ('fin', 'array')


def test_bounds_come_from_the_header():
    """one definition each; the staging arrays of the kernels are sized by these names"""
    assert (C3X, FIN) == (256, 576)
    src = open(_lib.HEADER).read()
    assert src.count('#define HRF_C3X_MAXC') == 1 and src.count('#define HRF_FIN_MAXC') == 1


# ------------------------------------------------------------------ packed 3x3 engine (csrc/conv3x_engine.hip)
# B,H,W,Cin,Cout,KH,stride,tf,bnb,epi - both directions of every case run packed (hrf_conv3x_supported takes them)
PACKED_CASES = (
    # forward, stride 1: Cin at the bound, one slab past it not a multiple of 32, 4.5 and 5 slabs of 64
    [(1, 6, 5, cin, 40, 3, 1, 2, True, True) for cin in (256, 272, 288, 320)] +
    [(1, 5, 6, 288, 64, 3, 1, 1, True, False)] +
    # forward, stride 2 (parity planes); its backward is the parity-class walk (Cout <= 64: never past the bound)
    [(1, 6, 5, cin, 64, 3, 2, 3, True, True) for cin in (256, 288, 320)] +
    [(1, 5, 6, 320, 40, 3, 2, 1, True, False)] +
    # backward data, stride 1: Cout = dY channels at the bound and past it, BatchNorm backward on load, with / without the act' epilogue
    [(1, 6, 5, 40, cout, 3, 1, 1, True, epi) for cout in (256, 288, 320) for epi in (True, False)] +
    [(1, 5, 6, 64, 272, 3, 1, 2, True, True)] +
    # past the bound WITHOUT coefficients on that side: taken (tf 0 forward / no BatchNorm behind the convolution)
    [(1, 6, 5, 320, 40, 3, 1, 0, True, False), (1, 6, 5, 40, 320, 3, 1, 2, False, True)]
)


@pytest.mark.parametrize('coef', ROUTES)
@pytest.mark.parametrize('case', PACKED_CASES, ids=str)
def test_packed_envelope_emul(case, coef):
    run_conv(case, 'emul', packed=True, coef=coef, ref64=True)


@pytest.mark.gpu
@pytest.mark.parametrize('coef', ROUTES)
@pytest.mark.parametrize('case', PACKED_CASES, ids=str)
def test_packed_envelope_gpu(case, coef):
    run_conv(case, 'hip', packed=True, coef=coef, ref64=True)


# ------------------------------------------------------------------ hrf_conv_fwd / hrf_conv_bwd_data
WIDE_CASES = (
    # 3x3 stride 1 (halo engine, csrc/conv3_engine.hip): coefficient channels on the forward side, then on the backward side
    [(1, 6, 5, c, 40, 3, 1, 2, True, True) for c in (576, 624)] + [(1, 5, 6, 40, c, 3, 1, 1, True, False) for c in (576, 624)] +
    # 3x3 stride 2 (conv_fwd_kernel / parity-class backward)
    [(1, 6, 5, c, 36, 3, 2, 3, True, True) for c in (576, 624)] + [(1, 5, 6, 40, c, 3, 2, 2, True, True) for c in (576, 624)] +
    # 1x1 row GEMM (csrc/lin_engine.hip)
    [(1, 6, 5, c, 48, 1, 1, 3, True, True) for c in (576, 624)] + [(1, 5, 6, 48, c, 1, 1, 1, True, False) for c in (576, 624)]
)
WIDE_LIN2_CASES = [c for c in WIDE_CASES if c[5] == 1]


@pytest.mark.parametrize('coef', ROUTES)
@pytest.mark.parametrize('case', WIDE_CASES, ids=str)
def test_conv_envelope_emul(case, coef):
    run_conv(case, 'emul', coef=coef, ref64=True)


@pytest.mark.parametrize('coef', ROUTES)
@pytest.mark.parametrize('case', WIDE_LIN2_CASES, ids=str)
def test_lin2_envelope_emul(case, coef):
    run_lin2(case, 0, 'emul', coef=coef, ref64=True)


@pytest.mark.gpu
@pytest.mark.parametrize('coef', ROUTES)
@pytest.mark.parametrize('case', WIDE_CASES, ids=str)
def test_conv_envelope_gpu(case, coef):
    run_conv(case, 'hip', coef=coef, ref64=True)


@pytest.mark.gpu
@pytest.mark.parametrize('coef', ROUTES)
@pytest.mark.parametrize('case', WIDE_LIN2_CASES, ids=str)
def test_lin2_envelope_gpu(case, coef):
    run_lin2(case, 0, 'hip', coef=coef, ref64=True)


# ------------------------------------------------------------------ depthwise (32-channel blocks: no bound on either route)
DW_WIDE_CASES = [(1, 6, 5, 624, 1, 3, True, True, True), (1, 5, 6, 624, 2, 2, False, True, True)]


@pytest.mark.parametrize('coef', ROUTES)
@pytest.mark.parametrize('case', DW_WIDE_CASES, ids=str)
def test_dwconv_envelope_emul(case, coef):
    run_dw(case, 'emul', coef=coef, ref64=True)


@pytest.mark.gpu
@pytest.mark.parametrize('coef', ROUTES)
@pytest.mark.parametrize('case', DW_WIDE_CASES, ids=str)
def test_dwconv_envelope_gpu(case, coef):
    run_dw(case, 'hip', coef=coef, ref64=True)


# ------------------------------------------------------------------ the contract of the packed entry points
def packed_taken(Cin, Cout, stride, direction, has_coef):
    """The rule of include/hrfuser_hip.h, restated: the SHAPE (hrf_conv3x_supported) and the coefficient bound."""
    if direction == 0:
        shape = Cout > 32
        return shape and not (has_coef and Cin > C3X)
    shape = Cin > 32 and (stride == 1 or Cout <= 64)
    return shape and not (has_coef and Cout > C3X)


def _contract_fwd(L, dev, g, Cin, Cout, stride, tf, route):
    B, H, W = 1, 5, 4
    rn = lambda *s: torch.randn(*s, generator=g)
    D = lambda t: None if t is None else t.float().to(dev)
    x, w, b = rn(B, Cin, H, W), rn(Cout, Cin, 3, 3) * 0.2, rn(Cout)
    sc, sh = torch.rand(Cin, generator=g) + 0.5, rn(Cin) * 0.3
    fin = ft = None
    if tf and route == 'fin':
        fin, ft = make_fin(L, Cin, 977.0, dev, g)
        sc, sh = ft['ref_scale'].cpu(), ft['ref_shift'].cpu()
    u = x.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    xt = {0: x.double(), 1: u, 2: F.relu(u), 3: F.gelu(u)}[tf]
    ref = nhwc(F.conv2d(xt, w.double(), b.double(), stride, 1))
    xr = nhwc(x)
    st = (H * W * Cin, W * Cin, Cin, 1)
    arr = (D(sc), D(sh)) if (tf and fin is None) else (None, None)
    yk = torch.zeros(ref.shape, device=dev)
    args = lambda: (D(xr), *st, B, H, W, Cin, D(w), D(b), 3, stride, Cout, yk, Cout, 0, None, None, 0, tf, *arr, None, None, fin, None, 0.0)
    wp = _pack3x(L, D(w), dev, 0)
    packed = lambda: L.hrf_conv_fwd_packed(*args(), wp, _lib.stream_ptr())
    assert bool(L.hrf_conv3x_supported(Cin, Cout, 3, stride, 0)) == (Cout > 32)
    if not packed_taken(Cin, Cout, stride, 0, tf != 0):
        refused(packed, yk)
        return
    packed()
    e_packed = r(yk, ref)
    yk.fill_(float('nan'))
    L.hrf_conv_fwd(*args(), _lib.stream_ptr())          # (taken widths are <= HRF_C3X_MAXC < HRF_FIN_MAXC: the same fin is legal here)
    e_plain = r(yk, ref)
    print(f'fwd Cin={Cin} Cout={Cout} s={stride} tf={tf} {route}: packed {e_packed:.2e} plain {e_plain:.2e}')
    assert e_packed < TOL and e_plain < TOL, (e_packed, e_plain)


def _contract_bwd(L, dev, g, Cin, Cout, stride, bn, route):
    B, H, W = 1, 5, 4
    rn = lambda *s: torch.randn(*s, generator=g)
    D = lambda t: None if t is None else t.float().to(dev)
    w = rn(Cout, Cin, 3, 3) * 0.2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    du, yraw = rn(B, Ho, Wo, Cout), rn(B, Ho, Wo, Cout)
    co, bfin = (None, None, None), None
    dy = du.double()
    if bn:
        if route == 'fin':
            bfin, bt = make_bfin(L, Cout, 811.0, dev, g)
            co = (bt['cA'], bt['cB'], bt['cC'])
            cr = [bt['ref_' + k].cpu().double() for k in ('cA', 'cB', 'cC')]
        else:
            cr = [rn(Cout).double(), rn(Cout).double() * 0.3, rn(Cout).double() * 0.1]
            co = tuple(D(c) for c in cr)
        dy = cr[0] * du.double() + cr[1] * yraw.double() + cr[2]
    xz = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(F.conv2d(xz, w.double(), None, stride, 1), xz, dy.permute(0, 3, 1, 2))
    ref = nhwc(ref)
    st = (H * W * Cin, W * Cin, Cin, 1)
    dx = torch.zeros(B, H, W, Cin, device=dev)
    args = lambda: (D(du), Cout, 0, D(yraw), *co, bfin, D(w), 3, stride, Cout, B, H, W, Cin, dx, *st, 0, 0, None, 0, None, None, 0, None)
    wp = _pack3x(L, D(w), dev, 1)
    packed = lambda: L.hrf_conv_bwd_data_packed(*args(), wp, _lib.stream_ptr())
    if not packed_taken(Cin, Cout, stride, 1, bn):
        refused(packed, dx)
        return
    packed()
    e_packed = r(dx, ref)
    dx.fill_(float('nan'))
    L.hrf_conv_bwd_data(*args(), _lib.stream_ptr())
    e_plain = r(dx, ref)
    print(f'bwd Cin={Cin} Cout={Cout} s={stride} bn={bn} {route}: packed {e_packed:.2e} plain {e_plain:.2e}')
    assert e_packed < TOL and e_plain < TOL, (e_packed, e_plain)


# (Cin, Cout): shapes the engine does not take (<= 32 channels on the N side), narrow ones, and 256 / 288 channels on either side
CONTRACT_GRID = [(24, 40), (40, 24), (40, 64), (256, 40), (288, 40), (40, 256), (40, 288), (24, 288), (288, 24)]


def run_packed_contract(backend):
    """Whenever the documented predicate says "taken", hrf_conv_fwd_packed / hrf_conv_bwd_data_packed return HRF_OK and both they
    and hrf_conv_fwd / hrf_conv_bwd_data on the same arguments are within TOL of the float64 reference (the two engines sum in
    different orders: they are not compared with each other more tightly than that); whenever it says "not taken" the call is
    refused before a launch.  No third outcome.  (Cin, Cout) x stride x direction x transform x route."""
    dev = use_backend(backend)
    L = _lib.lib()
    g = torch.Generator().manual_seed(41)
    n = [0, 0]
    for (Cin, Cout), stride in itertools.product(CONTRACT_GRID, (1, 2)):
        for tf, route in ((0, 'array'), (2, 'array'), (3, 'fin')):
            _contract_fwd(L, dev, g, Cin, Cout, stride, tf, route)
            n[packed_taken(Cin, Cout, stride, 0, tf != 0)] += 1
        for bn, route in ((False, 'array'), (True, 'array'), (True, 'fin')):
            _contract_bwd(L, dev, g, Cin, Cout, stride, bn, route)
            n[packed_taken(Cin, Cout, stride, 1, bn)] += 1
    assert n[0] >= 30 and n[1] >= 50, n                                   # both outcomes are really walked


def test_packed_contract_emul():
    run_packed_contract('emul')


@pytest.mark.gpu
def test_packed_contract_gpu():
    run_packed_contract('hip')


# ------------------------------------------------------------------ hrf_affine_act_res
def run_affine_act_res(C, backend):
    """C = HRF_FIN_MAXC: fin1 / fin2 finalised on load and arrays staged in LDS; C past it: fins refused, arrays read from global
    memory (the kernel's lds_coef == false branch).  One- and two-operand ReLU forms (Bottleneck / BasicBlock tails), the GELU
    tail with its fused LayerNorm row statistics (CrossFFN), vector and dword paths."""
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    g = torch.Generator().manual_seed(C)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    D = lambda t: None if t is None else t.float().to(dev)
    B, HW = 2, 23                                        # 46 rows: ragged against the 16-row blocks of the GELU-tail kernel
    rows = B * HW
    y1, y2, res = rn(rows, C) * 2 + 1, rn(rows, C), rn(rows, C)
    rs = torch.tensor([0.75, 1.25])
    rsr = rs.double().repeat_interleave(HW)[:, None]
    d = lambda t: t.double()

    def forms(c1, c2, f1, f2, knob18):
        """-> [(name, output, reference)] of the three forms with coefficients c1 = (sc, sh) of y1, c2 of y2 (arrays unless fin)"""
        a1 = (None, None) if f1 is not None else (D(c1[0]), D(c1[1]))
        a2 = (None, None) if f2 is not None else (D(c2[0]), D(c2[1]))
        L.hrf_debug_knob(18, knob18)
        try:
            o1, o2, o3 = (torch.full((rows, C), float('nan'), device=dev) for _ in range(3))
            lnr = torch.zeros(rows, 2, device=dev)
            L.hrf_affine_act_res(D(y1), *a1, None, None, None, D(res), None, 1, 1, 0, o1, rows, C, None, 0.0, f1, None, s)
            L.hrf_affine_act_res(D(y1), *a1, D(y2), *a2, None, None, 1, 1, 0, o2, rows, C, None, 0.0, f1, f2, s)
            L.hrf_affine_act_res(D(y1), *a1, None, None, None, D(res), D(rs), HW, 2, 1, o3, rows, C, lnr, 1e-6, f1, None, s)
        finally:
            L.hrf_debug_knob(18, 0)
        u1, u2 = d(y1) * d(c1[0]) + d(c1[1]), d(y2) * d(c2[0]) + d(c2[1])
        r3 = d(res) + rsr * F.gelu(u1)
        return [('relu1', o1, F.relu(u1 + d(res))), ('relu2', o2, F.relu(u1 + u2)), ('gelu_tail', o3, r3),
                ('ln_mean', lnr[:, 0], r3.mean(-1)), ('ln_rstd', lnr[:, 1], (r3.var(-1, unbiased=False) + 1e-6).rsqrt())]

    arr1 = (torch.rand(C, generator=g) + 0.5, rn(C) * 0.3)
    arr2 = (torch.rand(C, generator=g) + 0.5, rn(C) * 0.3)
    for knob18 in (0, 1):                                # float4 lanes; dword path
        for name, o, ref in forms(arr1, arr2, None, None, knob18):
            assert r(o, ref) < (1e-4 if name == 'ln_rstd' else TOL), (C, 'array', knob18, name, r(o, ref))
    f1, t1 = make_fin(L, C, 733.0, dev, g, write=0)
    f2, t2 = make_fin(L, C, 733.0, dev, g)
    if C <= FIN:
        f1w, t1w = make_fin(L, C, 733.0, dev, g)
        c1, c2 = (t1w['ref_scale'].cpu(), t1w['ref_shift'].cpu()), (t2['ref_scale'].cpu(), t2['ref_shift'].cpu())
        o = torch.full((rows, C), float('nan'), device=dev)
        L.hrf_affine_act_res(D(y1), None, None, D(y2), None, None, None, None, 1, 1, 0, o, rows, C, None, 0.0, f1w, f2, s)
        check_fin(t1w)
        check_fin(t2)
        assert r(o, F.relu(d(y1) * d(c1[0]) + d(c1[1]) + d(y2) * d(c2[0]) + d(c2[1]))) < TOL
        # the three forms with non-writing fins (running statistics were updated once above)
        f2n = _lib.BnFin.from_buffer_copy(f2)
        f2n.write = 0
        c1 = (t1['ref_scale'].cpu(), t1['ref_shift'].cpu())
        for name, o, ref in forms(c1, c2, f1, f2n, 0):
            assert r(o, ref) < (1e-4 if name == 'ln_rstd' else TOL), (C, 'fin', name, r(o, ref))
    else:
        o = torch.empty(rows, C, device=dev)
        refused(lambda: L.hrf_affine_act_res(D(y1), None, None, None, None, None, D(res), None, 1, 1, 0, o, rows, C, None, 0.0, f1, None, s), o)
        refused(lambda: L.hrf_affine_act_res(D(y1), *map(D, arr1), D(y2), None, None, None, None, 1, 1, 0, o, rows, C, None, 0.0, None, f2, s), o)
        refused(lambda: L.hrf_affine_act_res(D(y1), None, None, None, None, None, D(res), D(rs), HW, 2, 1, o, rows, C,
                                             torch.zeros(rows, 2, device=dev), 1e-6, f1, None, s), o)


@pytest.mark.parametrize('C', [FIN, 624, 626])
def test_affine_act_res_envelope_emul(C):
    run_affine_act_res(C, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('C', [FIN, 624, 626])
def test_affine_act_res_envelope_gpu(C):
    run_affine_act_res(C, 'hip')


# ------------------------------------------------------------------ hrf_fuse_sum
def run_fuse_sum(C, backend):
    """four terms (identity, same-resolution BatchNorm, bilinear x2, nearest x2): every conv-produced term's BatchNorm finalised
    on load up to HRF_FIN_MAXC / 2 channels, refused past it; scale / shift arrays at any width"""
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    g = torch.Generator().manual_seed(C)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    D = lambda t: None if t is None else t.float().to(dev)
    B, H, W = 1, 4, 6
    x0, ysame, ylo, ynr = rn(B, H, W, C), rn(B, H, W, C), rn(B, 2, 3, C), rn(B, 2, 3, C)

    def ref(cs):
        aff = lambda t, c: t.double() * c[0].double() + c[1].double()
        up = lambda t, mode: F.interpolate(t.permute(0, 3, 1, 2), size=(H, W), mode=mode,
                                           **({'align_corners': False} if mode == 'bilinear' else {})).permute(0, 2, 3, 1)
        return F.relu(x0.double() + aff(ysame, cs[0]) + aff(up(ylo.double(), 'bilinear'), cs[1]) + aff(up(ynr.double(), 'nearest'), cs[2]))

    def call(cs, fins, o):
        a = [(None, None) if (fins is not None and fins[k + 1].stats) else (D(cs[k][0]), D(cs[k][1])) for k in range(3)]
        L.hrf_fuse_sum(1, D(x0), None, None, 0, 0, 2, D(ysame), *a[0], 0, 0, 3, D(ylo), *a[1], 2, 3, 4, D(ynr), *a[2], 2, 3,
                       o, B, H, W, C, fins, s)
    cs = [(torch.rand(C, generator=g) + 0.5, rn(C) * 0.3) for _ in range(3)]
    o = torch.full((B, H, W, C), float('nan'), device=dev)
    call(cs, None, o)
    assert r(o, ref(cs)) < TOL, (C, 'array', r(o, ref(cs)))
    made = [make_fin(L, C, 611.0, dev, g) for _ in range(3)]
    fins = (_lib.BnFin * 4)()
    for k in range(3):
        fins[k + 1] = made[k][0]
    csf = [(t['ref_scale'].cpu(), t['ref_shift'].cpu()) for _, t in made]
    if C <= FIN // 2:
        o.fill_(float('nan'))
        call(csf, fins, o)
        for _, t in made:
            check_fin(t)
        assert r(o, ref(csf)) < TOL, (C, 'fin', r(o, ref(csf)))
        one = (_lib.BnFin * 4)()                         # a single fin among array terms
        m1 = make_fin(L, C, 611.0, dev, g)
        one[2] = m1[0]
        mix = [cs[0], (m1[1]['ref_scale'].cpu(), m1[1]['ref_shift'].cpu()), cs[2]]
        o.fill_(float('nan'))
        call(mix, one, o)
        check_fin(m1[1])
        assert r(o, ref(mix)) < TOL
    else:
        refused(lambda: call(csf, fins, o), o)
        one = (_lib.BnFin * 4)()
        one[3] = made[2][0]
        refused(lambda: call(cs, one, o), o)


@pytest.mark.parametrize('C', [FIN // 2, FIN // 2 + 2, 624])
def test_fuse_sum_envelope_emul(C):
    run_fuse_sum(C, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('C', [FIN // 2, FIN // 2 + 2, 624])
def test_fuse_sum_envelope_gpu(C):
    run_fuse_sum(C, 'hip')
