"""Direct C-ABI tests of the resampling and pooling kernels of csrc/pointwise.hip at the shapes where index math goes wrong:
hrf_bilinear_up_into, hrf_bilinear_up_bwd (narrow and wide gather, > 256-channel rows, strided input, grouped launch),
hrf_nearest_up_bwd (ky != kx, idle threads), hrf_avg_pool / hrf_avg_pool_bwd (floor-cropped sizes), hrf_slice_cols, hrf_fuse_sum on
its per-element and vector kernels with bilinear and non-square nearest terms, and the second pass of the grid-stride loops of the
elementwise kernels (ew_grid caps the grid at 2048 blocks; the gather adjoints cap theirs at 1024).

Every output buffer is `guarded`: 256 sentinel floats on either side that must stay bit-unchanged; outputs the kernel must
overwrite start as NaN, columns it must leave alone start as a sentinel and are compared with torch.equal.

Reference: the torch operator in float64 on the CPU (fp64 autograd for adjoints).  Gate, for a kernel output a:
    r(a, ref64) <= min(TOL, 4 * r(ref32, ref64) + 2**-23)
with ref32 the same torch operator in float32 on the CPU, TOL = test_kernels.TOL, the factor 4 the margin tests/test_rpn_loss.py
gives a kernel over the restatement's own fp32 error, and one fp32 ulp so that an exact reference does not give a zero bound.
Each forward / adjoint pair is also tied to itself by <fwd(x), g> == <x, bwd(g)> on the kernels' own outputs.

Out of scope: the 64-bit index path of the elementwise kernels (it needs 2^31 elements)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_kernels as TK
from helpers import use_backend
from hrfuser_amd import _lib

TOL, KC, r, zstat, fold, refused = TK.TOL, TK.KC, TK.r, TK.zstat, TK.fold, TK.refused
GUARD = 256                 # floats on either side of every output buffer
SENT = -1234.5              # guard bands and the columns / regions a kernel must leave alone
NAN = float('nan')
PASS = 2048 * 256           # work items of one pass of an ew_grid launch
WORST = {}                  # (backend, kernel) -> (r, bound, case): what the gate measured in the running test, printed at its end


def guarded(shape, fill, dev, offset=0, dtype=torch.float32):
    """A buffer of numel + 2 * GUARD (+ offset) elements of SENT; returns (the inner view filled with `fill` - a number or a
    tensor -, check) where check() asserts that both bands are bit-unchanged.  offset = 1: the view starts on a base that is
    aligned to one element only (test_kernels.run_pointwise's `unal`)."""
    n = int(math.prod(shape))
    buf = torch.full((n + 2 * GUARD + offset,), SENT, dtype=dtype, device=dev)
    lo = GUARD + offset
    inner = buf[lo:lo + n].view(shape)
    if isinstance(fill, torch.Tensor):
        inner.copy_(fill.to(dev))
    else:
        inner.fill_(fill)
    if offset:
        assert inner.data_ptr() % 16 != 0

    def check(tag=''):
        assert bool((buf[:lo] == SENT).all()), (tag, 'write below the buffer')
        assert bool((buf[lo + n:] == SENT).all()), (tag, 'write above the buffer')
    return inner, check


def gate(backend, kernel, a, ref64, ref32, case):
    e, e32 = r(a, ref64), r(ref32, ref64)
    bound = min(TOL, 4 * e32 + 2.0 ** -23)
    w = WORST.get((backend, kernel))
    if w is None or not e / bound <= w[0] / w[1]:
        WORST[(backend, kernel)] = (e, bound, case)
    assert e <= bound, (kernel, case, f'r {e:.3e} bound {bound:.3e} (ref32 {e32:.3e})')


def report(backend):
    for (b, k), (e, bound, case) in sorted(WORST.items()):
        if b == backend:
            print(f'[resample {b}] {k}: worst r {e:.2e} at bound {bound:.2e} ({case})')


def setup(backend, seed):
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    D = lambda t: None if t is None else t.detach().float().contiguous().to(dev)
    return dev, _lib.lib(), _lib.stream_ptr(), rn, D


def run(body, backend, *a):
    WORST.clear()
    try:
        body(backend, *a)
    finally:
        use_backend('hip')
        report(backend)


# ------------------------------------------------------------------ references (torch, CPU)
def up_ref(x, size, mode, dt):
    """NHWC x -> F.interpolate(size) in dtype dt, NHWC"""
    kw = dict(align_corners=False) if mode == 'bilinear' else {}
    return F.interpolate(x.detach().to(dt).permute(0, 3, 1, 2), size=size, mode=mode, **kw).permute(0, 2, 3, 1).contiguous()


def up_adj(g, lo, mode, dt):
    """autograd adjoint of up_ref at cotangent g (NHWC, B x H x W x C) for a source of lo = (Hs, Ws)"""
    B, H, W, C = g.shape
    x = torch.zeros(B, lo[0], lo[1], C, dtype=dt, requires_grad=True)
    kw = dict(align_corners=False) if mode == 'bilinear' else {}
    y = F.interpolate(x.permute(0, 3, 1, 2), size=(H, W), mode=mode, **kw)
    gx, = torch.autograd.grad(y, x, g.detach().to(dt).permute(0, 3, 1, 2))
    return gx.contiguous()


def pool_ref(x, k, dt):
    return F.avg_pool2d(x.detach().to(dt).permute(0, 3, 1, 2), k, k).permute(0, 2, 3, 1).contiguous()


def pool_adj(g, H, W, k, dt):
    B, _, _, C = g.shape
    x = torch.zeros(B, H, W, C, dtype=dt, requires_grad=True)
    gx, = torch.autograd.grad(F.avg_pool2d(x.permute(0, 3, 1, 2), k, k), x, g.detach().to(dt).permute(0, 3, 1, 2))
    return gx.contiguous()


def moments_gate(backend, kernel, st, du, ylow, C, case):
    """fold(st) against the fp64 sums of the kernel's OWN fp32 du (du itself is gated against autograd separately); ref32 = the
    same sums in fp32.  ylow None: the second-moment half must be exactly zero."""
    f = fold(st).cpu()
    d = du.detach().cpu().reshape(-1, C)
    gate(backend, kernel + '.stats', f[:C], d.double().sum(0), d.sum(0), case + ' sum du')
    if ylow is None:
        assert bool((f[C:] == 0).all()), (kernel, case, 'second moments without ylow')
    else:
        y = ylow.detach().cpu().reshape(-1, C)
        gate(backend, kernel + '.stats', f[C:], (d.double() * y.double()).sum(0), (d * y.float()).sum(0), case + ' sum du*ylow')


def bwd_window(q, n_hi, n_lo):
    """the candidate window of bilinear_up_bwd_kernel along one axis, restated: (lo, hi) inclusive, in the kernel's fp32"""
    f = np.float32
    ratio = f(n_hi) / f(n_lo)
    lo = int(np.floor((f(q) - f(1) + f(0.5)) * ratio - f(0.5))) - 1
    hi = int(np.ceil((f(q) + f(1) + f(0.5)) * ratio - f(0.5))) + 1
    return max(lo, 0), min(hi, n_hi - 1)


def is_wide(q, n_hi, n_lo):
    lo, hi = bwd_window(q, n_hi, n_lo)
    return hi - lo >= 24           # (the kernel: narrow = xhi - xlo < 24)


# ------------------------------------------------------------------ 1. hrf_bilinear_up_into
UP_SIZES = [((5, 7), (5, 7)), ((3, 5), (6, 10)), ((2, 3), (16, 24)), ((2, 3), (32, 48)), ((8, 4), (15, 7)), ((1, 1), (5, 7))]


def run_up_into(backend, lo, hi):
    dev, L, s, rn, D = setup(backend, 101 + lo[0] + 7 * hi[0])
    B, (Hs, Ws), (H, W) = 2, lo, hi
    for C in (1, 15, 18, 300, 624):
        x = rn(B, Hs, Ws, C)
        assert not torch.equal(x[0], x[1])
        ref64, ref32 = up_ref(x, hi, 'bilinear', torch.float64), up_ref(x, hi, 'bilinear', torch.float32)
        layouts = [(C, 0, 0), (C + 9, 0, 0), (C + 9, 4, 0), (C + 9, 9, 0)] + ([(C + 9, 4, 1)] if C == 18 else [])
        for ld, off, unal in layouts:
            case = f'{lo}->{hi} C{C} ld{ld} off{off} unal{unal}'
            out, chk = guarded((B, H, W, ld), SENT, dev, unal)
            out[..., off:off + C] = NAN
            L.hrf_bilinear_up_into(D(x), Hs, Ws, C, out, ld, off, B, H, W, s)
            o = out.cpu()
            chk(case)
            assert torch.equal(o[..., :off], torch.full_like(o[..., :off], SENT)), (case, 'columns left of the slice')
            assert torch.equal(o[..., off + C:], torch.full_like(o[..., off + C:], SENT)), (case, 'columns right of the slice')
            gate(backend, 'hrf_bilinear_up_into', o[..., off:off + C], ref64, ref32, case)


def run_up_into_adjacent(backend):
    """the neck's concat: an identity-size branch, an up-sampled branch and the zeroed pad columns (a 1 x 1 source of zeros) as
    three launches into adjacent slices of one row buffer; no launch disturbs what another wrote"""
    dev, L, s, rn, D = setup(backend, 102)
    B, H, W, C1, C2, pad = 2, 6, 10, 15, 18, 3
    ld = C1 + C2 + pad
    x1, x2 = rn(B, H, W, C1), rn(B, 3, 5, C2)
    out, chk = guarded((B, H, W, ld), NAN, dev)
    L.hrf_bilinear_up_into(D(x1), H, W, C1, out, ld, 0, B, H, W, s)
    first = out[..., :C1].clone()
    assert bool(torch.isnan(out[..., C1:]).all())
    L.hrf_bilinear_up_into(D(x2), 3, 5, C2, out, ld, C1, B, H, W, s)
    second = out[..., C1:C1 + C2].clone()
    assert torch.equal(out[..., :C1], first) and bool(torch.isnan(out[..., C1 + C2:]).all())
    L.hrf_bilinear_up_into(torch.zeros(B, 1, 1, pad, device=dev), 1, 1, pad, out, ld, C1 + C2, B, H, W, s)
    chk('adjacent')
    assert torch.equal(out[..., :C1], first) and torch.equal(out[..., C1:C1 + C2], second)
    assert torch.equal(out[..., C1 + C2:], torch.zeros(B, H, W, pad, device=dev))
    assert torch.equal(first.cpu(), x1)                                      # Hs == H: an identity copy
    gate(backend, 'hrf_bilinear_up_into', second, up_ref(x2, (H, W), 'bilinear', torch.float64),
         up_ref(x2, (H, W), 'bilinear', torch.float32), 'adjacent slices')


@pytest.mark.parametrize('lo,hi', UP_SIZES, ids=str)
def test_bilinear_up_into_emul(lo, hi):
    run(run_up_into, 'emul', lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize('lo,hi', UP_SIZES, ids=str)
def test_bilinear_up_into_gpu(lo, hi):
    run(run_up_into, 'hip', lo, hi)


def test_bilinear_up_into_adjacent_emul():
    run(run_up_into_adjacent, 'emul')


@pytest.mark.gpu
def test_bilinear_up_into_adjacent_gpu():
    run(run_up_into_adjacent, 'hip')


# ------------------------------------------------------------------ 2. hrf_bilinear_up_bwd
UPB_SIZES = UP_SIZES + [((2, 3), (24, 39))]      # factors 12 and 13: wide interior windows and narrow border windows in one launch


def test_bwd_window_cases_reach_both_branches():
    """by the kernel's own window formula: 2x3 -> 24x39 has a low-resolution column with a window of >= 24 columns (the general
    loop) and one with less (the unrolled gather); x16 is wide everywhere; every factor up to 8 and 15/8 is narrow everywhere"""
    wide = [is_wide(q, 39, 3) for q in range(3)]
    assert any(wide) and not all(wide), wide
    assert all(is_wide(q, 48, 3) for q in range(3))
    for (hs, ws), (h, w) in UP_SIZES[:3] + UP_SIZES[4:5]:
        assert not any(is_wide(q, w, ws) for q in range(ws))


def run_up_bwd(backend, lo, hi):
    dev, L, s, rn, D = setup(backend, 201 + lo[0] + 7 * hi[0])
    B, (Hs, Ws), (H, W) = 2, lo, hi
    for C in (10, 18, 100, 256, 300, 624, 768):
        case = f'{lo}->{hi} C{C}'
        g, ylow = rn(B, H, W, C), rn(B, Hs, Ws, C)
        ref64, ref32 = up_adj(g, lo, 'bilinear', torch.float64), up_adj(g, lo, 'bilinear', torch.float32)
        # contiguous g, moments with ylow (one width on a 4-byte aligned du)
        du, chk = guarded((B, Hs, Ws, C), NAN, dev, 1 if C == 18 else 0)
        st, chks = guarded((KC * 2 * C,), 0.0, dev, dtype=torch.float64)
        L.hrf_bilinear_up_bwd(D(g), C, 0, B, H, W, C, D(ylow), Hs, Ws, du, st, s)
        chk(case), chks(case)
        gate(backend, 'hrf_bilinear_up_bwd', du, ref64, ref32, case)
        moments_gate(backend, 'hrf_bilinear_up_bwd', st, du, ylow, C, case)
        # the slice [3, 3 + C) of rows of C + 7 floats, NaN in every other column: a read outside the slice poisons du; no ylow
        gs = torch.full((B, H, W, C + 7), NAN)
        gs[..., 3:3 + C] = g
        du2, chk2 = guarded((B, Hs, Ws, C), NAN, dev)
        st2, chks2 = guarded((KC * 2 * C,), 0.0, dev, dtype=torch.float64)
        L.hrf_bilinear_up_bwd(D(gs), C + 7, 3, B, H, W, C, None, Hs, Ws, du2, st2, s)
        chk2(case), chks2(case)
        gate(backend, 'hrf_bilinear_up_bwd', du2, ref64, ref32, case + ' strided')
        assert torch.equal(du2.cpu(), du.cpu()), (case, 'the same arithmetic through (ldG, goff)')
        moments_gate(backend, 'hrf_bilinear_up_bwd', st2, du2, None, C, case + ' strided')
        # no moments
        du3, chk3 = guarded((B, Hs, Ws, C), NAN, dev)
        L.hrf_bilinear_up_bwd(D(g), C, 0, B, H, W, C, None, Hs, Ws, du3, None, s)
        chk3(case)
        assert torch.equal(du3.cpu(), du.cpu()), (case, 'du without moments')


def run_up_bwd_misc(backend):
    dev, L, s, rn, D = setup(backend, 202)
    # ---- C = 769 is refused, nothing written
    B, H, W, Hs, Ws, C = 1, 6, 10, 3, 5, 769
    du, chk = guarded((B, Hs, Ws, C), NAN, dev)
    st, chks = guarded((KC * 2 * C,), 0.0, dev, dtype=torch.float64)
    g = D(rn(B, H, W, C))
    refused(lambda: L.hrf_bilinear_up_bwd(g, C, 0, B, H, W, C, None, Hs, Ws, du, st, s), du)
    chk('C769'), chks('C769')
    assert bool((st == 0).all())
    # ---- queued between hrf_group_begin / hrf_group_end next to a problem of another size: the plain calls' results
    probs = [(2, (2, 3), (24, 39), 18, 25, 4), (1, (8, 4), (15, 7), 300, 300, 0)]        # B, lo, hi, C, ldG, goff
    data = []
    for B, (Hs, Ws), (H, W), C, ld, off in probs:
        gs = torch.full((B, H, W, ld), NAN)
        gs[..., off:off + C] = rn(B, H, W, C)
        data.append((D(gs), D(rn(B, Hs, Ws, C))))

    def issue():
        outs = []
        for (B, (Hs, Ws), (H, W), C, ld, off), (gs, yl) in zip(probs, data):
            du, chk = guarded((B, Hs, Ws, C), NAN, dev)
            st, chks = guarded((KC * 2 * C,), 0.0, dev, dtype=torch.float64)
            L.hrf_bilinear_up_bwd(gs, ld, off, B, H, W, C, yl, Hs, Ws, du, st, s)
            outs.append((du, st, chk, chks))
        return outs
    plain = issue()
    L.hrf_group_begin()
    try:
        grouped = issue()
    finally:
        L.hrf_group_end(s)
    for k, ((du, st, chk, chks), (dug, stg, chkg, chksg)) in enumerate(zip(plain, grouped)):
        chk(k), chks(k), chkg(k), chksg(k)
        (B, lo, hi, C, ld, off), gs = probs[k], data[k][0].cpu()
        gate(backend, 'hrf_bilinear_up_bwd', dug, up_adj(gs[..., off:off + C], lo, 'bilinear', torch.float64),
             up_adj(gs[..., off:off + C], lo, 'bilinear', torch.float32), f'grouped {k}')
        assert torch.equal(dug.cpu(), du.cpu()), (k, 'du of the queued call')
        # (the moments are fp64 atomic sums over blocks: the order of the additions is free, their value is not)
        assert r(fold(stg), fold(st)) <= 1e-12, (k, 'moments of the queued call')


@pytest.mark.parametrize('lo,hi', UPB_SIZES, ids=str)
def test_bilinear_up_bwd_emul(lo, hi):
    run(run_up_bwd, 'emul', lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize('lo,hi', UPB_SIZES, ids=str)
def test_bilinear_up_bwd_gpu(lo, hi):
    run(run_up_bwd, 'hip', lo, hi)


def test_bilinear_up_bwd_refusal_and_group_emul():
    run(run_up_bwd_misc, 'emul')


@pytest.mark.gpu
def test_bilinear_up_bwd_refusal_and_group_gpu():
    run(run_up_bwd_misc, 'hip')


# ------------------------------------------------------------------ 3. hrf_nearest_up_bwd
NEAREST_FACTORS = [(1, 1), (2, 2), (2, 4), (3, 1), (8, 8)]


def run_nearest_bwd(backend, ky, kx):
    dev, L, s, rn, D = setup(backend, 301 + 10 * ky + kx)
    B, Hs, Ws = 2, 3, 2
    H, W = Hs * ky, Ws * kx
    for C in (6, 18, 100, 256, 300, 768):
        case = f'k{ky}x{kx} C{C}'
        g, ylow = rn(B, H, W, C), rn(B, Hs, Ws, C)
        ref64, ref32 = up_adj(g, (Hs, Ws), 'nearest', torch.float64), up_adj(g, (Hs, Ws), 'nearest', torch.float32)
        # (the reference checked against the definition: every low-resolution pixel owns its ky x kx block)
        assert r(ref64, g.double().view(B, Hs, ky, Ws, kx, C).sum((2, 4))) <= 1e-14
        du, chk = guarded((B, Hs, Ws, C), NAN, dev, 1 if C == 18 else 0)
        st, chks = guarded((KC * 2 * C,), 0.0, dev, dtype=torch.float64)
        L.hrf_nearest_up_bwd(D(g), C, 0, B, H, W, C, D(ylow), Hs, Ws, du, st, s)
        chk(case), chks(case)
        gate(backend, 'hrf_nearest_up_bwd', du, ref64, ref32, case)
        moments_gate(backend, 'hrf_nearest_up_bwd', st, du, ylow, C, case)
        gs = torch.full((B, H, W, C + 7), NAN)
        gs[..., 3:3 + C] = g
        du2, chk2 = guarded((B, Hs, Ws, C), NAN, dev)
        L.hrf_nearest_up_bwd(D(gs), C + 7, 3, B, H, W, C, None, Hs, Ws, du2, None, s)
        chk2(case)
        gate(backend, 'hrf_nearest_up_bwd', du2, ref64, ref32, case + ' strided')
        assert torch.equal(du2.cpu(), du.cpu()), (case, 'the same arithmetic through (ldG, goff)')


def run_nearest_bwd_refusals(backend):
    dev, L, s, rn, D = setup(backend, 302)
    for B, H, W, Hs, Ws, C in ((1, 7, 4, 3, 2, 6), (1, 6, 5, 3, 2, 6), (1, 6, 4, 3, 2, 769)):
        du, chk = guarded((B, Hs, Ws, C), NAN, dev)
        st, chks = guarded((KC * 2 * C,), 0.0, dev, dtype=torch.float64)
        g = D(rn(B, H, W, C))
        refused(lambda: L.hrf_nearest_up_bwd(g, C, 0, B, H, W, C, None, Hs, Ws, du, st, s), du)
        chk((H, W, C)), chks((H, W, C))
        assert bool((st == 0).all())


@pytest.mark.parametrize('ky,kx', NEAREST_FACTORS, ids=str)
def test_nearest_up_bwd_emul(ky, kx):
    run(run_nearest_bwd, 'emul', ky, kx)


@pytest.mark.gpu
@pytest.mark.parametrize('ky,kx', NEAREST_FACTORS, ids=str)
def test_nearest_up_bwd_gpu(ky, kx):
    run(run_nearest_bwd, 'hip', ky, kx)


def test_nearest_up_bwd_refusals_emul():
    run(run_nearest_bwd_refusals, 'emul')


@pytest.mark.gpu
def test_nearest_up_bwd_refusals_gpu():
    run(run_nearest_bwd_refusals, 'hip')


# ------------------------------------------------------------------ 4. hrf_avg_pool / hrf_avg_pool_bwd
POOL_CASES = [(1, 5, 7), (2, 6, 8), (2, 7, 9), (3, 7, 10), (3, 3, 3), (4, 10, 13), (8, 8, 8), (8, 17, 9)]      # k, H, W


def run_pool(backend, k, H, W):
    dev, L, s, rn, D = setup(backend, 401 + 100 * k + H)
    B, Ho, Wo = 2, H // k, W // k
    for C in (1, 15, 256, 624):
        case = f'k{k} {H}x{W} C{C}'
        x = rn(B, H, W, C)
        out, chk = guarded((B, Ho, Wo, C), NAN, dev, 1 if C == 15 else 0)
        L.hrf_avg_pool(D(x), B, H, W, C, k, out, s)
        chk(case)
        gate(backend, 'hrf_avg_pool', out, pool_ref(x, k, torch.float64), pool_ref(x, k, torch.float32), case)
        g = rn(B, Ho, Wo, C)
        ref64, ref32 = pool_adj(g, H, W, k, torch.float64), pool_adj(g, H, W, k, torch.float32)
        # accumulate = 0 onto NaN: everything finite, the rows / columns cut off by floor(H / k) exactly 0.0
        dx, chkd = guarded((B, H, W, C), NAN, dev, 1 if C == 15 else 0)
        L.hrf_avg_pool_bwd(D(g), B, H, W, C, k, dx, 0, s)
        chkd(case)
        d = dx.cpu()
        assert bool(torch.isfinite(d).all()), case
        assert bool((d[:, Ho * k:] == 0).all()) and bool((d[:, :, Wo * k:] == 0).all()), (case, 'cropped region')
        gate(backend, 'hrf_avg_pool_bwd', d, ref64, ref32, case)
        # accumulate = 1 onto a random base: the cropped region bit-equal to the base, the rest base + gradient
        base = rn(B, H, W, C)
        dx1, chk1 = guarded((B, H, W, C), base, dev)
        L.hrf_avg_pool_bwd(D(g), B, H, W, C, k, dx1, 1, s)
        chk1(case)
        d1 = dx1.cpu()
        assert torch.equal(d1[:, Ho * k:], base[:, Ho * k:]) and torch.equal(d1[:, :, Wo * k:], base[:, :, Wo * k:]), (case, 'cropped region')
        gate(backend, 'hrf_avg_pool_bwd', d1, base.double() + ref64, base + ref32, case + ' accumulate')


def run_pool_refusals(backend):
    dev, L, s, rn, D = setup(backend, 402)
    B, H, W, C = 1, 4, 6, 5
    x = D(rn(B, H, W, C))
    for k in (0, 5, 7):                 # k = 0, k > H, k > W (k = 5: H / k = 0; k = 7: both)
        out, chk = guarded((B, 1, 1, C), NAN, dev)
        refused(lambda: L.hrf_avg_pool(x, B, H, W, C, k, out, s), out)
        dx, chkd = guarded((B, H, W, C), NAN, dev)
        refused(lambda: L.hrf_avg_pool_bwd(out, B, H, W, C, k, dx, 0, s), dx)
        chk(k), chkd(k)
    out, chk = guarded((B, 1, 1, C), NAN, dev)                 # k > W alone
    refused(lambda: L.hrf_avg_pool(x, B, 6, 4, C, 5, out, s), out)
    dx, chkd = guarded((B, 6, 4, C), NAN, dev)
    refused(lambda: L.hrf_avg_pool_bwd(out, B, 6, 4, C, 5, dx, 1, s), dx)
    chk('k>W'), chkd('k>W')


@pytest.mark.parametrize('k,H,W', POOL_CASES, ids=str)
def test_avg_pool_emul(k, H, W):
    run(run_pool, 'emul', k, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize('k,H,W', POOL_CASES, ids=str)
def test_avg_pool_gpu(k, H, W):
    run(run_pool, 'hip', k, H, W)


def test_avg_pool_refusals_emul():
    run(run_pool_refusals, 'emul')


@pytest.mark.gpu
def test_avg_pool_refusals_gpu():
    run(run_pool_refusals, 'hip')


# ------------------------------------------------------------------ 5. hrf_slice_cols
def run_slice_cols(backend):
    dev, L, s, rn, D = setup(backend, 501)
    rows = 37
    for C in (1, 15, 18, 624):
        ld = C + 11
        src = rn(rows, ld)
        for off in (0, 5, 11):
            case = f'C{C} off{off}'
            want = src[:, off:off + C]
            dst, chk = guarded((rows, C), NAN, dev, 1 if off == 5 else 0)
            L.hrf_slice_cols(D(src), ld, off, rows, C, dst, 0, s)
            chk(case)
            assert torch.equal(dst.cpu(), want), case
            base = rn(rows, C)
            dst1, chk1 = guarded((rows, C), base, dev)
            L.hrf_slice_cols(D(src), ld, off, rows, C, dst1, 1, s)
            chk1(case)
            assert torch.equal(dst1.cpu(), base + want), (case, 'accumulate: one fp32 add per element')
    dst, chk = guarded((4, 6), NAN, dev)
    L.hrf_slice_cols(D(rn(4, 17)), 17, 5, 0, 6, dst, 0, s)               # rows = 0: nothing is launched
    chk('rows 0')
    assert bool(torch.isnan(dst).all())


def test_slice_cols_emul():
    run(run_slice_cols, 'emul')


@pytest.mark.gpu
def test_slice_cols_gpu():
    run(run_slice_cols, 'hip')


# ------------------------------------------------------------------ 6. hrf_fuse_sum: per-element and vector kernels
# out size, bilinear source, nearest source.  15 x 7 has no divisor pair (2, 4): its nearest term takes (3, 7), the second problem
# carries (2, 4) with H a multiple of 4 - both have H / Hs != W / Ws.
FUSE_PROBLEMS = [((15, 7), (8, 4), (5, 1)), ((8, 16), (2, 4), (4, 4))]


def fuse_ref(x0, ysame, ylo, ynr, cs, size, dt):
    """the restatement of tests/test_coef_routes.py::run_fuse_sum in dtype dt"""
    aff = lambda t, c: t.to(dt) * c[0].to(dt) + c[1].to(dt)
    return F.relu(x0.to(dt) + aff(ysame, cs[0]) + aff(up_ref(ylo, size, 'bilinear', dt), cs[1]) + aff(up_ref(ynr, size, 'nearest', dt), cs[2]))


def fuse_call(L, s, D, x0, ysame, ylo, ynr, cs, out, C):
    B, H, W = x0.shape[:3]
    L.hrf_fuse_sum(1, D(x0), None, None, 0, 0, 2, D(ysame), D(cs[0][0]), D(cs[0][1]), 0, 0,
                   3, D(ylo), D(cs[1][0]), D(cs[1][1]), ylo.shape[1], ylo.shape[2],
                   4, D(ynr), D(cs[2][0]), D(cs[2][1]), ynr.shape[1], ynr.shape[2], out, B, H, W, C, None, s)


def run_fuse(backend, prob):
    dev, L, s, rn, D = setup(backend, 601 + prob)
    (H, W), blo, nlo = FUSE_PROBLEMS[prob]
    B = 2
    for C in (15, 10, 20):                  # per-element, two-wide, four-wide
        case = f'{H}x{W} C{C}'
        x0, ysame, ylo, ynr = rn(B, H, W, C), rn(B, H, W, C), rn(B, *blo, C), rn(B, *nlo, C)
        # (the nearest reference against the definition: repeat every source pixel ky x kx times)
        ky, kx = H // nlo[0], W // nlo[1]
        assert torch.equal(up_ref(ynr, (H, W), 'nearest', torch.float32), ynr.repeat_interleave(ky, 1).repeat_interleave(kx, 2))
        cs = [(torch.rand(C, generator=torch.Generator().manual_seed(C + k)) + 0.5, rn(C) * 0.3) for k in range(3)]
        ref64, ref32 = (fuse_ref(x0, ysame, ylo, ynr, cs, (H, W), dt) for dt in (torch.float64, torch.float32))
        out, chk = guarded((B, H, W, C), NAN, dev, 1 if C == 20 else 0)
        fuse_call(L, s, D, x0, ysame, ylo, ynr, cs, out, C)
        chk(case)
        gate(backend, 'hrf_fuse_sum', out, ref64, ref32, case)
        if C == 20:                         # the same problem forced onto the per-element kernel
            outk, chkk = guarded((B, H, W, C), NAN, dev)
            L.hrf_debug_knob(18, 1)
            try:
                fuse_call(L, s, D, x0, ysame, ylo, ynr, cs, outk, C)
            finally:
                L.hrf_debug_knob(18, 0)
            chkk(case)
            gate(backend, 'hrf_fuse_sum', outk, ref64, ref32, case + ' knob 18')
            assert r(outk, out) <= 1e-6, (case, 'per-element kernel against the vector kernel')
    # a nearest term whose Hs does not divide H
    C = 10
    out, chk = guarded((B, H, W, C), NAN, dev)
    z = D(rn(B, H, W, C))
    refused(lambda: L.hrf_fuse_sum(1, z, None, None, 0, 0, 4, z, z, z, H - 1, W, 0, None, None, None, 0, 0, 0, None, None, None, 0, 0,
                                   out, B, H, W, C, None, s), out)
    chk('refused')


@pytest.mark.parametrize('prob', [0, 1])
def test_fuse_sum_terms_emul(prob):
    run(run_fuse, 'emul', prob)


@pytest.mark.gpu
@pytest.mark.parametrize('prob', [0, 1])
def test_fuse_sum_terms_gpu(prob):
    run(run_fuse, 'hip', prob)


# ------------------------------------------------------------------ adjoint identities on the kernels' own outputs
def run_adjoints(backend):
    """<fwd(x), g> == <x, bwd(g)> in float64 to 1e-5 relative.  x and g are positive (rand + 0.5): the inner products have no
    cancellation, so `relative` is relative to their own size; a positive input also keeps the ReLU of hrf_fuse_sum inactive."""
    dev, L, s, rn, D = setup(backend, 701)
    gen = torch.Generator().manual_seed(702)
    pos = lambda *sh: torch.rand(*sh, generator=gen) + 0.5
    dot = lambda a, b: float((a.detach().cpu().double() * b.detach().cpu().double()).sum())

    def same(lhs, rhs, tag):
        assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (tag, lhs, rhs)
    B = 2
    for (Hs, Ws), (H, W) in UPB_SIZES:
        for C in (18, 300):
            x, g = pos(B, Hs, Ws, C), pos(B, H, W, C)
            y, chk = guarded((B, H, W, C), NAN, dev)
            L.hrf_bilinear_up_into(D(x), Hs, Ws, C, y, C, 0, B, H, W, s)
            du, chkd = guarded((B, Hs, Ws, C), NAN, dev)
            L.hrf_bilinear_up_bwd(D(g), C, 0, B, H, W, C, None, Hs, Ws, du, None, s)
            chk(), chkd()
            same(dot(y, g), dot(x, du), ('bilinear', Hs, Ws, H, W, C))
    for k, H, W in POOL_CASES:
        for C in (15, 256):
            x, g = pos(B, H, W, C), pos(B, H // k, W // k, C)
            y, chk = guarded((B, H // k, W // k, C), NAN, dev)
            L.hrf_avg_pool(D(x), B, H, W, C, k, y, s)
            dx, chkd = guarded((B, H, W, C), NAN, dev)
            L.hrf_avg_pool_bwd(D(g), B, H, W, C, k, dx, 0, s)
            chk(), chkd()
            same(dot(y, g), dot(x, dx), ('avg_pool', k, H, W, C))
    Hs, Ws = 3, 2
    for ky, kx in NEAREST_FACTORS:
        for C in (15, 18, 300):
            H, W = Hs * ky, Ws * kx
            x, g = pos(B, Hs, Ws, C), pos(B, H, W, C)
            y, chk = guarded((B, H, W, C), NAN, dev)
            one, zero = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            L.hrf_fuse_sum(4, D(x), one, zero, Hs, Ws, 0, None, None, None, 0, 0, 0, None, None, None, 0, 0, 0, None, None, None, 0, 0,
                           y, B, H, W, C, None, s)
            du, chkd = guarded((B, Hs, Ws, C), NAN, dev)
            L.hrf_nearest_up_bwd(D(g), C, 0, B, H, W, C, None, Hs, Ws, du, None, s)
            chk(), chkd()
            assert float(y.min()) > 0
            same(dot(y, g), dot(x, du), ('nearest', ky, kx, C))


def test_adjoint_identities_emul():
    run(run_adjoints, 'emul')


@pytest.mark.gpu
def test_adjoint_identities_gpu():
    run(run_adjoints, 'hip')


# ------------------------------------------------------------------ 7. more than one grid pass
def second_pass(out, ref64, vw, what, rel=TOL):
    """the first work item of the second pass of an ew_grid launch (VW floats from flat element 2048 * 256 * VW), by name"""
    i = PASS * vw
    a, b = out.detach().cpu().reshape(-1)[i:i + vw].double(), ref64.reshape(-1)[i:i + vw].double()
    assert a.numel() == vw, (what, 'the case has no second pass')
    assert bool(((a - b).abs() <= rel * ref64.abs().max()).all()), \
        f'{what}: flat element {i} = 2048 * 256 * {vw}, the first work item of the SECOND grid pass, is {a.tolist()}, expected {b.tolist()}'


def run_pass_scale_add(backend):
    dev, L, s, rn, D = setup(backend, 801)
    rows, C, rps = 35001, 15, 5001                      # 525 015 items: 2 050 blocks of work plus a tail of 215
    assert rows * C > PASS and (rows * C) % 256
    y, res, res2 = rn(rows, C), rn(rows, C), rn(rows, C)
    mask = torch.empty(rows, C).bernoulli_(0.9, generator=torch.Generator().manual_seed(3))
    rs = torch.rand(rows // rps + 1, generator=torch.Generator().manual_seed(4)) + 0.5
    rsr = rs[torch.arange(rows) // rps][:, None]
    msc = torch.tensor(1 / 0.9, dtype=torch.float32)                           # (the kernel receives mscale as a float)
    ref = lambda dt: res.to(dt) + res2.to(dt) + y.to(dt) * msc.to(dt) * mask.to(dt) * rsr.to(dt)
    out, chk = guarded((rows, C), NAN, dev)
    L.hrf_scale_add(D(y), D(mask), 1 / 0.9, D(rs), rps, D(res), D(res2), out, rows, C, s)
    chk()
    second_pass(out, ref(torch.float64), 1, 'hrf_scale_add')
    gate(backend, 'hrf_scale_add', out, ref(torch.float64), ref(torch.float32), 'two passes')


def run_pass_affine(backend, C):
    dev, L, s, rn, D = setup(backend, 802 + C)
    vw = 4 if C % 4 == 0 else (2 if C % 2 == 0 else 1)
    rows = -(-(PASS * vw + 8000) // C)
    assert rows * C // vw > PASS and (rows * C // vw) % 256, (rows, C)
    y1, y2, res = rn(rows, C), rn(rows, C), rn(rows, C)
    sc1, sh1, sc2, sh2 = torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.5, rn(C), rn(C), rn(C)
    ref = lambda dt: F.relu(y1.to(dt) * sc1.to(dt) + sh1.to(dt) + res.to(dt) + y2.to(dt) * sc2.to(dt) + sh2.to(dt))
    out, chk = guarded((rows, C), NAN, dev)
    L.hrf_affine_act_res(D(y1), D(sc1), D(sh1), D(y2), D(sc2), D(sh2), D(res), None, 1, 1, 0, out, rows, C, None, 0.0, None, None, s)
    chk()
    second_pass(out, ref(torch.float64), vw, f'hrf_affine_act_res C{C}')
    gate(backend, 'hrf_affine_act_res', out, ref(torch.float64), ref(torch.float32), f'two passes C{C}')


BIG = dict(hi=(330, 318), blo=(83, 80), nlo=(165, 106))       # 104 940 pixels: x 5 = 524 700 items, a tail of 156


def run_pass_fuse(backend):
    dev, L, s, rn, D = setup(backend, 803)
    (H, W), C, B = BIG['hi'], 20, 1
    assert B * H * W * C // 4 > PASS and (B * H * W * C // 4) % 256
    x0, ysame, ylo, ynr = rn(B, H, W, C), rn(B, H, W, C), rn(B, *BIG['blo'], C), rn(B, *BIG['nlo'], C)
    cs = [(torch.rand(C, generator=torch.Generator().manual_seed(k)) + 0.5, rn(C) * 0.3) for k in range(3)]
    ref64, ref32 = (fuse_ref(x0, ysame, ylo, ynr, cs, (H, W), dt) for dt in (torch.float64, torch.float32))
    out, chk = guarded((B, H, W, C), NAN, dev)
    fuse_call(L, s, D, x0, ysame, ylo, ynr, cs, out, C)
    chk()
    second_pass(out, ref64, 4, 'hrf_fuse_sum C20')
    gate(backend, 'hrf_fuse_sum', out, ref64, ref32, 'two passes C20')


def run_pass_up_into(backend):
    dev, L, s, rn, D = setup(backend, 804)
    (H, W), (Hs, Ws), C, B, ld, off = BIG['hi'], BIG['blo'], 5, 1, 8, 2
    assert B * H * W * C > PASS and (B * H * W * C) % 256
    x = rn(B, Hs, Ws, C)
    ref64, ref32 = up_ref(x, (H, W), 'bilinear', torch.float64), up_ref(x, (H, W), 'bilinear', torch.float32)
    out, chk = guarded((B, H, W, ld), SENT, dev)
    out[..., off:off + C] = NAN
    L.hrf_bilinear_up_into(D(x), Hs, Ws, C, out, ld, off, B, H, W, s)
    chk()
    o = out.cpu()
    assert bool((o[..., :off] == SENT).all()) and bool((o[..., off + C:] == SENT).all())
    second_pass(o[..., off:off + C].contiguous(), ref64, 1, 'hrf_bilinear_up_into')
    gate(backend, 'hrf_bilinear_up_into', o[..., off:off + C], ref64, ref32, 'two passes')


def run_pass_pool_bwd(backend):
    dev, L, s, rn, D = setup(backend, 805)
    (H, W), C, B, k = BIG['hi'], 5, 1, 4                # 330 = 4 * 82 + 2, 318 = 4 * 79 + 2: cropped rows and columns
    assert B * H * W * C > PASS and (B * H * W * C) % 256
    g = rn(B, H // k, W // k, C)
    ref64, ref32 = pool_adj(g, H, W, k, torch.float64), pool_adj(g, H, W, k, torch.float32)
    dx, chk = guarded((B, H, W, C), NAN, dev)
    L.hrf_avg_pool_bwd(D(g), B, H, W, C, k, dx, 0, s)
    chk()
    second_pass(dx, ref64, 1, 'hrf_avg_pool_bwd')
    d = dx.cpu()
    assert bool((d[:, (H // k) * k:] == 0).all()) and bool((d[:, :, (W // k) * k:] == 0).all())
    gate(backend, 'hrf_avg_pool_bwd', d, ref64, ref32, 'two passes')


def run_pass_slice(backend):
    dev, L, s, rn, D = setup(backend, 806)
    rows, C, ld, off = 35001, 15, 26, 5
    assert rows * C > PASS and (rows * C) % 256
    src, base = rn(rows, ld), rn(rows, C)
    for acc in (0, 1):
        dst, chk = guarded((rows, C), base if acc else NAN, dev)
        L.hrf_slice_cols(D(src), ld, off, rows, C, dst, acc, s)
        chk()
        want = base + src[:, off:off + C] if acc else src[:, off:off + C]
        second_pass(dst, want, 1, f'hrf_slice_cols accumulate {acc}', rel=0.0)
        assert torch.equal(dst.cpu(), want)


def run_pass_gather_bwd(backend):
    """the gather adjoints cap their grid at 1024 blocks of 256 / C low-resolution pixels: at C = 256 (one pixel per block) 1058
    pixels need a second pass; pixel 1024 is its first"""
    dev, L, s, rn, D = setup(backend, 807)
    B, Hs, Ws, C = 2, 23, 23, 256
    assert B * Hs * Ws > 1024
    for name, mode, k in (('hrf_bilinear_up_bwd', 'bilinear', 2), ('hrf_nearest_up_bwd', 'nearest', 2)):
        H, W = Hs * k, Ws * k
        g, ylow = rn(B, H, W, C), rn(B, Hs, Ws, C)
        ref64, ref32 = up_adj(g, (Hs, Ws), mode, torch.float64), up_adj(g, (Hs, Ws), mode, torch.float32)
        du, chk = guarded((B, Hs, Ws, C), NAN, dev)
        st, chks = guarded((KC * 2 * C,), 0.0, dev, dtype=torch.float64)
        getattr(L, name)(D(g), C, 0, B, H, W, C, D(ylow), Hs, Ws, du, st, s)
        chk(), chks()
        a, b = du.cpu().reshape(-1, C)[1024].double(), ref64.reshape(-1, C)[1024]
        assert bool(((a - b).abs() <= TOL * ref64.abs().max()).all()), \
            f'{name}: low-resolution pixel 1024, the first of the SECOND grid pass, is wrong by {float((a - b).abs().max()):.3e}'
        gate(backend, name, du, ref64, ref32, 'two passes')
        moments_gate(backend, name, st, du, ylow, C, 'two passes')


PASS_RUNS = [(run_pass_scale_add,), (run_pass_affine, 260), (run_pass_affine, 15), (run_pass_fuse,), (run_pass_up_into,),
             (run_pass_pool_bwd,), (run_pass_slice,), (run_pass_gather_bwd,)]
PASS_IDS = ['scale_add', 'affine_act_res_C260', 'affine_act_res_C15', 'fuse_sum_C20', 'bilinear_up_into', 'avg_pool_bwd', 'slice_cols',
            'gather_bwd']


@pytest.mark.parametrize('case', PASS_RUNS, ids=PASS_IDS)
def test_second_grid_pass_emul(case):
    run(case[0], 'emul', *case[1:])


@pytest.mark.gpu
@pytest.mark.parametrize('case', PASS_RUNS, ids=PASS_IDS)
def test_second_grid_pass_gpu(case):
    run(case[0], 'hip', *case[1:])
