"""hrf_fuse_sum_bwd (include/hrfuser_hip.h): the backward of one HRModule exchange sum out = ReLU(sum of terms) in ONE launch -
the ReLU mask, the identity gradient, the moments of the same-resolution terms and every bilinear adjoint as sections of one grid
(csrc/pointwise.hip) - against the launches it replaces and against float64 autograd.

Per case, on the emulator and on the GPU:
  * g and the identity gradient are bit-equal to what hrf_act_bwd (+ hrf_scale_add) write for the same arguments;
  * du of a term whose gather order is unchanged (every ratio but the integer factors 2, 4 and 8: case c, and the factor 3 of
    case f) is bit-equal to hrf_bilinear_up_bwd fed with that g; du of a term on the integer-factor gather (rows of the window
    in rounds, spread over several threads from factor 4) is within test_kernels.TOL (the `r` metric) of the float64 autograd
    gradient of F.interpolate(..., align_corners=False);
  * every folded moment is within TOL of the float64 sums;
  * deterministic mode: two calls leave identical bits in g, du, the identity gradient and the moments;
  * widths the kernel does not take (an odd one, one beyond the vector layout) are refused before any launch and
    runtime.fuse_sum issues the separate launches instead;
  * an HRFomerModule with 3 and with 4 branches at 16 x 24 gives the same input and parameter gradients (TOL) with
    HRF_FUSE_BWD at 0 and at 1."""
import os

import pytest
import torch
import torch.nn.functional as F

import hrfuser_oracle as O
import hrfuser_amd.backbone as BB
import hrfuser_amd.runtime as R
from helpers import LN, NORM, disable_stochastic, use_backend
from hrfuser_amd import _lib
from hrfuser_amd.testing import BlockHarness
from test_kernels import TOL, fold, r, refused, zstat

# name: (B, H, W, C), identity form (None | 'fresh' | 'alias' | 'acc'), same-resolution terms, low-resolution sizes
CASES = {
    'a': ((2, 12, 20, 18), 'fresh', 1, ((6, 10), (3, 5))),            # factors 2 and 4 (row split), the 2-channel vector layout
    'b': ((2, 16, 24, 36), 'alias', 0, ((8, 12), (4, 6), (2, 3))),    # x2, x4 and x8; no same-resolution term: the identity IS g
    'c': ((1, 15, 7, 72), None, 0, ((8, 4),)),                        # non-integer ratio, up-sampling sections only
    'd': ((2, 6, 10, 144), 'acc', 3, ()),                             # coarsest row: three moment sets, identity accumulated
    # beyond the issue's list: factor 3 (an integer ratio on the generic gather), x2 / x4 at 78 channels where a block holds
    # only 3 row groups (x4 shared by 2 threads instead of 4), one image
    'f': ((1, 12, 24, 78), 'fresh', 2, ((4, 8), (6, 12), (3, 6))),
}


def _split(dims, low, C):
    """does this term take the kernel's integer-factor gather (csrc/pointwise.hip: factor 2, 4 or 8 - the 2F x 2F window in
    rounds of 32 loads, its rows spread over up to F threads and added in lane order), whose order of additions is not the one
    of hrf_bilinear_up_bwd?  Every other ratio keeps that order and must be bit-equal."""
    _, H, W, _ = dims
    return H % low[0] == 0 and W % low[1] == 0 and H // low[0] == W // low[1] and H // low[0] in (2, 4, 8)


def _problem(name, dev):
    dims, ident, nsame, lows = CASES[name]
    B, H, W, C = dims
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g)
    p = dict(dims=dims, ident=ident, lows=lows, dev=dev)
    p['dout'], p['out'] = rn(B, H, W, C), rn(B, H, W, C)
    p['ys'] = [rn(B, H, W, C) for _ in range(nsame)]
    p['ylows'] = [rn(B, hs, ws, C) for hs, ws in lows]
    p['base'] = rn(B, H, W, C)                              # what the identity gradient holds before an accumulating call
    return p


_REF = {}


def _reference(name, p):
    """float64, computed once per case: v = dout [out > 0], its moments, and per up-sampled term the autograd gradient of
    F.interpolate(bilinear, align_corners=False) under v with its moments"""
    if name in _REF:
        return _REF[name]
    B, H, W, C = p['dims']
    v = p['dout'].double() * (p['out'] > 0)
    ref = dict(v=v, same=[(v.reshape(-1, C).sum(0), (v * y.double()).reshape(-1, C).sum(0)) for y in p['ys']], up=[])
    for yl in p['ylows']:
        q = yl.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        F.interpolate(q, size=(H, W), mode='bilinear', align_corners=False).backward(v.permute(0, 3, 1, 2))
        du = q.grad.permute(0, 2, 3, 1)
        ref['up'].append((du, du.reshape(-1, C).sum(0), (du * yl.double()).reshape(-1, C).sum(0)))
    _REF[name] = ref
    return ref


def _fused(L, p):
    """one hrf_fuse_sum_bwd call on fresh outputs -> dict of everything it wrote"""
    B, H, W, C = p['dims']
    dev = p['dev']
    D = lambda t: t.to(dev)
    P = _lib._ptr
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    o = dict(g=None, idg=None, st=[zstat(C, dev) for _ in p['ys']], du=[nan(*yl.shape) for yl in p['ylows']],
             ust=[zstat(C, dev) for _ in p['ylows']])
    keep = [D(p['dout']), D(p['out'])] + [D(y) for y in p['ys']] + [D(y) for y in p['ylows']]
    a = _lib.FuseBwd()
    a.dout, a.out, a.B, a.H, a.W, a.C = P(keep[0]), P(keep[1]), B, H, W, C
    if p['ys'] or p['ident'] == 'alias':
        o['g'] = nan(B, H, W, C)
        a.g = P(o['g'])
    if p['ident'] == 'fresh':
        o['idg'] = nan(B, H, W, C)
        a.id_dst = P(o['idg'])
    elif p['ident'] == 'acc':
        o['idg'] = D(p['base']).clone()
        a.id_dst, a.id_accumulate = P(o['idg']), 1
    for k in range(len(p['ys'])):
        a.y[k], a.st[k] = P(keep[2 + k]), P(o['st'][k])
    for k, (hs, ws) in enumerate(p['lows']):
        a.up_kind[k], a.up_ylow[k], a.up_Hs[k], a.up_Ws[k] = 1, P(keep[2 + len(p['ys']) + k]), hs, ws
        a.up_du[k], a.up_stats[k] = P(o['du'][k]), P(o['ust'][k])
    L.hrf_fuse_sum_bwd(a, _lib.stream_ptr())
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return o


def _separate(L, p):
    """the launches the fused call replaces, on the same arguments"""
    B, H, W, C = p['dims']
    dev = p['dev']
    D = lambda t: t.to(dev)
    s = _lib.stream_ptr()
    ys = [D(y) for y in p['ys']] + [None] * (3 - len(p['ys']))
    o = dict(g=torch.zeros(B, H, W, C, device=dev), idg=None, st=[zstat(C, dev) for _ in p['ys']], du=[], ust=[])
    sts = o['st'] + [None] * (3 - len(p['ys']))
    L.hrf_act_bwd(D(p['dout']), D(p['out']), ys[0], None, None, None, 1, 0, o['g'], ys[1], ys[2], sts[0], sts[1], sts[2],
                  B * H * W, C, s)
    if p['ident'] == 'fresh':
        o['idg'] = torch.zeros(B, H, W, C, device=dev)
        L.hrf_scale_add(o['g'], None, 1.0, None, 1, None, None, o['idg'], o['g'].numel(), 1, s)
    elif p['ident'] == 'acc':
        o['idg'] = D(p['base']).clone()
        L.hrf_scale_add(o['g'], None, 1.0, None, 1, o['idg'], None, o['idg'], o['g'].numel(), 1, s)
    for yl, (hs, ws) in zip(p['ylows'], p['lows']):
        du, st = torch.zeros(B, hs, ws, C, device=dev), zstat(C, dev)
        L.hrf_bilinear_up_bwd(o['g'], C, 0, B, H, W, C, D(yl), hs, ws, du, st, s)
        o['du'].append(du)
        o['ust'].append(st)
    return o


def run_case(name, backend):
    dev = use_backend(backend)
    L = _lib.lib()
    p = _problem(name, dev)
    dims, C = p['dims'], p['dims'][3]
    assert L.hrf_fuse_sum_bwd_supported(C) == 1
    ref = _reference(name, p)
    f, o = _fused(L, p), _separate(L, p)
    if f['g'] is not None:
        assert torch.equal(f['g'], o['g']), 'g differs from hrf_act_bwd'
    if p['ident'] in ('fresh', 'acc'):
        assert torch.equal(f['idg'], o['idg']), 'identity gradient differs from hrf_scale_add'
    for k in range(len(p['ys'])):
        e = (r(fold(f['st'][k])[:C], ref['same'][k][0]), r(fold(f['st'][k])[C:], ref['same'][k][1]))
        print(f'case {name} same term {k}: moments vs fp64 {e[0]:.2e} {e[1]:.2e}')
        assert max(e) < TOL, (name, k, e)
    for k, low in enumerate(p['lows']):
        du64, s1, s2 = ref['up'][k]
        split = _split(dims, low, C)
        e = (r(f['du'][k], du64), r(fold(f['ust'][k])[:C], s1), r(fold(f['ust'][k])[C:], s2))
        print(f'case {name} up term {low} ({"integer-factor gather" if split else "gather order kept"}): du vs fp64 {e[0]:.2e}, '
              f'moments {e[1]:.2e} {e[2]:.2e}')
        if not split:
            assert torch.equal(f['du'][k], o['du'][k]), (name, low, 'du differs from hrf_bilinear_up_bwd')
        assert max(e) < TOL, (name, low, e)


@pytest.mark.parametrize('name', sorted(CASES))
def test_fuse_bwd_emul(name):
    run_case(name, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_fuse_bwd_gpu(name):
    run_case(name, 'hip')


# ------------------------------------------------------------------ deterministic mode
def _det_fold(st, C):
    """value of the 2*C accumulators of a deterministic moment slot: four bins of 2^40 per accumulator, lowest unit 2^-96"""
    b = st.cpu().view(torch.int64)[:8 * C].view(4, 2 * C).tolist()
    return torch.tensor([float(sum(b[k][i] << (40 * k) for k in range(4))) * 2.0 ** -96 for i in range(2 * C)],
                        dtype=torch.float64)


def run_deterministic(backend):
    dev = use_backend(backend)
    L = _lib.lib()
    old = os.environ.get('HRF_EMUL_THREADS')
    L.hrf_set_deterministic(1)
    try:
        for name in ('a', 'b'):
            p = _problem(name, dev)
            C = p['dims'][3]
            ref = _reference(name, p)
            runs = []
            for workers in ('1', '8'):                        # (emulator: the blocks of a launch over 1 / 8 OS threads)
                os.environ['HRF_EMUL_THREADS'] = workers
                runs.append(_fused(L, p))
            x, y = runs
            for key in ('g', 'idg'):
                assert (x[key] is None) == (y[key] is None) and (x[key] is None or torch.equal(x[key], y[key])), key
            for key in ('du', 'st', 'ust'):
                for u, w in zip(x[key], y[key]):
                    assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u,
                                       w.view(torch.int64) if w.dtype == torch.float64 else w), (name, key)
            for k in range(len(p['ys'])):
                m = _det_fold(x['st'][k], C)
                assert r(m[:C], ref['same'][k][0]) < TOL and r(m[C:], ref['same'][k][1]) < TOL
            for k in range(len(p['lows'])):
                m = _det_fold(x['ust'][k], C)
                assert r(m[:C], ref['up'][k][1]) < TOL and r(m[C:], ref['up'][k][2]) < TOL
    finally:
        L.hrf_set_deterministic(0)
        if old is None:
            os.environ.pop('HRF_EMUL_THREADS', None)
        else:
            os.environ['HRF_EMUL_THREADS'] = old


def test_fuse_bwd_deterministic_emul():
    run_deterministic('emul')


@pytest.mark.gpu
def test_fuse_bwd_deterministic_gpu():
    run_deterministic('hip')


# ------------------------------------------------------------------ refusals and the runtime's routes
class _Ctx:
    """what runtime.fuse_sum needs of a backward context: the library, the stream, and the pushed backward closures"""

    def __init__(self, L):
        self.L, self.stream, self.probe, self.cbs = L, _lib.stream_ptr(), None, []

    def push(self, bwd, sync=None):
        self.cbs.append(bwd)


class _Counting:
    """the library with its hrf_fuse_sum_bwd calls counted"""

    def __init__(self, lib):
        self.__dict__.update(_lib_=lib, n=0)

    def __getattr__(self, name):
        fn = getattr(self._lib_, name)
        if name != 'hrf_fuse_sum_bwd':
            return fn

        def call(*a):
            self.__dict__['n'] += 1
            return fn(*a)
        return call


def _bn_state(raw, g):
    C = raw.shape[-1]
    st = R.BNState()
    st.pending, st.raw, st.C, st.du = None, raw, C, None
    st.scale = (torch.rand(C, generator=g) + 0.5).to(raw.device)
    st.shift = (torch.randn(C, generator=g) * 0.3).to(raw.device)
    st.gstats = zstat(C, raw.device)
    return st


def _runtime_sum(L, dev, C, mode, prior_grad):
    """runtime.fuse_sum forward + backward of ReLU(identity + same-resolution term + x2 and x4 up-sampled terms) at 2 x 8 x 12 x C
    under HRF_FUSE_BWD = mode -> (fused calls issued, gradients and moments, float64 references)"""
    B, H, W = 2, 8, 12
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g)
    x0, ys, yl2, yl4, cot, base = rn(B, H, W, C), rn(B, H, W, C), rn(B, 4, 6, C), rn(B, 2, 3, C), rn(B, H, W, C), rn(B, H, W, C)
    ident = R.Act(x0.to(dev))
    if prior_grad:
        ident.grad = base.to(dev).clone()
    sts = [_bn_state(t.to(dev), g) for t in (ys, yl2, yl4)]
    terms = [('id', ident), ('same', R.Lazy(sts[0], R.TF_AFFINE)), ('up', R.Lazy(sts[1], R.TF_AFFINE)),
             ('up', R.Lazy(sts[2], R.TF_AFFINE))]
    lib = _Counting(L)
    ctx = _Ctx(lib)
    old = os.environ.get('HRF_FUSE_BWD')
    os.environ['HRF_FUSE_BWD'] = mode
    try:
        out = R.fuse_sum(ctx, (B, H, W, C), terms)
        out.grad = cot.to(dev)
        for cb in reversed(ctx.cbs):
            cb()
    finally:
        if old is None:
            os.environ.pop('HRF_FUSE_BWD', None)
        else:
            os.environ['HRF_FUSE_BWD'] = old
    # float64: the same sum through autograd (the BatchNorm affines are constants here: du is the gradient at the affine's output)
    q = [t.double().requires_grad_(True) for t in (x0, ys, yl2, yl4)]
    aff = [q[k + 1] * sts[k].scale.cpu().double() + sts[k].shift.cpu().double() for k in range(3)]
    for t in aff:
        t.retain_grad()
    up = lambda t: F.interpolate(t.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    ref = F.relu(q[0] + aff[0] + up(aff[1]) + up(aff[2]))
    assert r(out.t, ref) < TOL
    mask = (out.t.cpu() > 0).double()                      # (the product's own ReLU decisions)
    (q[0] + aff[0] + up(aff[1]) + up(aff[2])).backward(cot.double() * mask)
    got = dict(idg=ident.grad, du=[st.du for st in sts], mom=[fold(st.gstats) for st in sts])
    want = dict(idg=q[0].grad + (base.double() if prior_grad else 0), du=[t.grad for t in aff],
                mom=[torch.cat([t.grad.reshape(-1, C).sum(0), (t.grad * raw.double()).reshape(-1, C).sum(0)])
                     for t, raw in zip(aff, (ys, yl2, yl4))])
    return lib.n, got, want


def run_routes(backend):
    dev = use_backend(backend)
    L = _lib.lib()
    # the two widths of case e: refused before any launch ...
    assert (L.hrf_fuse_sum_bwd_supported(15), L.hrf_fuse_sum_bwd_supported(258), L.hrf_fuse_sum_bwd_supported(18)) == (0, 0, 1)
    for C in (15, 258):
        a = _lib.FuseBwd()
        dd, oo, gk = torch.randn(1, 4, 6, C).to(dev), torch.randn(1, 4, 6, C).to(dev), torch.empty(1, 4, 6, C, device=dev)
        a.dout, a.out, a.g, a.B, a.H, a.W, a.C = dd.data_ptr(), oo.data_ptr(), gk.data_ptr(), 1, 4, 6, C
        refused(lambda: L.hrf_fuse_sum_bwd(a, _lib.stream_ptr()), gk)
    # ... as is a nearest term (kind 2) at a width the kernel takes
    a = _lib.FuseBwd()
    dd, oo, du = torch.randn(1, 4, 6, 18).to(dev), torch.randn(1, 4, 6, 18).to(dev), torch.empty(1, 2, 3, 18, device=dev)
    a.dout, a.out, a.B, a.H, a.W, a.C = dd.data_ptr(), oo.data_ptr(), 1, 4, 6, 18
    a.up_kind[0], a.up_Hs[0], a.up_Ws[0], a.up_du[0] = 2, 2, 3, du.data_ptr()
    refused(lambda: L.hrf_fuse_sum_bwd(a, _lib.stream_ptr()), du)
    # ... and runtime.fuse_sum issues the separate launches for them, the fused one otherwise (and never with HRF_FUSE_BWD=0)
    for C, mode, prior, calls in ((15, '1', False, 0), (258, '1', True, 0), (18, '1', False, 1), (18, '1', True, 1), (18, '0', False, 0)):
        n, got, want = _runtime_sum(L, dev, C, mode, prior)
        assert n == calls, (C, mode, n)
        e = [r(got['idg'], want['idg'])] + [r(a_, b_) for a_, b_ in zip(got['du'], want['du'])] + \
            [r(a_, b_) for a_, b_ in zip(got['mom'], want['mom'])]
        print(f'runtime.fuse_sum C={C} HRF_FUSE_BWD={mode} prior gradient={prior}: fused calls {n}, worst error {max(e):.2e}')
        assert max(e) < TOL, (C, mode, e)


def test_fuse_bwd_routes_emul():
    run_routes('emul')


@pytest.mark.gpu
def test_fuse_bwd_routes_gpu():
    run_routes('hip')


# ------------------------------------------------------------------ the forward kernel with 2 / 4 channels per thread
def run_forward(name, backend):
    """hrf_fuse_sum on the terms of cases a - c: the vector kernel's output is bit-equal to the per-element kernel's (the
    parent's formula, still the route of odd widths; hrf_debug_knob 19 = 1 selects it), with scale / shift arrays and with the
    BatchNorms of two terms finalised on load (test_kernels.make_fin), and within TOL of float64"""
    from test_kernels import check_fin, make_fin
    dev = use_backend(backend)
    L = _lib.lib()
    s = _lib.stream_ptr()
    p = _problem(name, dev)
    B, H, W, C = p['dims']
    g = torch.Generator().manual_seed(5)
    D = lambda t: t.to(dev)
    raws = ([p['base']] if p['ident'] else []) + p['ys'] + p['ylows']
    types = ([1] if p['ident'] else []) + [2] * len(p['ys']) + [3] * len(p['ylows'])
    assert len(raws) <= 4
    scs = [torch.rand(C, generator=g) + 0.5 for _ in raws]
    shs = [torch.randn(C, generator=g) * 0.3 for _ in raws]
    keep = [D(t) for t in raws] + [D(t) for t in scs] + [D(t) for t in shs]
    n = len(raws)

    def call(fin_terms, knob):
        fins, fts = (_lib.BnFin * 4)(), {}
        gf = torch.Generator().manual_seed(9)                 # (the same synthetic moments for both kernels)
        for k in fin_terms:
            fins[k], fts[k] = make_fin(L, C, 611.0, dev, gf)
        args = []
        for k in range(4):
            if k >= n:
                args += [0, None, None, None, 0, 0]
            else:
                aff = types[k] != 1 and k not in fin_terms
                hs, ws = raws[k].shape[1:3] if types[k] == 3 else (0, 0)
                args += [types[k], keep[k], keep[n + k] if aff else None, keep[2 * n + k] if aff else None, hs, ws]
        out = torch.full((B, H, W, C), float('nan'), device=dev)
        L.hrf_debug_knob(19, knob)
        try:
            L.hrf_fuse_sum(*args, out, B, H, W, C, fins if fin_terms else None, s)
        finally:
            L.hrf_debug_knob(19, 0)
        for ft in fts.values():
            check_fin(ft)
        return out, fts
    fin_terms = [k for k in range(n) if types[k] != 1][:2]
    for ft_ in ([], fin_terms):
        (new, fts), (old, _) = call(ft_, 0), call(ft_, 1)
        assert torch.equal(new, old), (name, ft_, 'differs from the per-element kernel')
        acc = 0
        for k in range(n):
            t = raws[k].double()
            if types[k] != 1:
                sc = fts[k]['ref_scale'].cpu().double() if k in ft_ else scs[k].double()
                sh = fts[k]['ref_shift'].cpu().double() if k in ft_ else shs[k].double()
                t = t * sc + sh
            if types[k] == 3:
                t = F.interpolate(t.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
            acc = acc + t
        e = r(new, F.relu(acc))
        print(f'forward case {name} fins {ft_}: vs fp64 {e:.2e}')
        assert e < TOL, (name, ft_, e)


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_fuse_fwd_vec_emul(name):
    run_forward(name, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_fuse_fwd_vec_gpu(name):
    run_forward(name, 'hip')


# ------------------------------------------------------------------ module level
CH, HD = (8, 16, 32, 64), (1, 2, 4, 8)


def run_module(nb, backend):
    """HRFomerModule with nb branches, finest map 16 x 24, one training forward + backward per setting of HRF_FUSE_BWD from the
    same parameters and inputs: every input gradient and every parameter gradient agrees within TOL"""
    dev = use_backend(backend)
    orc = O.HRFormerModule(list(CH[:nb]), (1,) * nb, HD[:nb], (4,) * nb, NORM, LN)
    O.seeded_fill_(orc, 3)
    h = BlockHarness(BB.HRFomerModule(nb, BB.HRFormerBlock, (1,) * nb, list(CH[:nb]), CH[:nb], HD[:nb], (7,) * nb, (4,) * nb,
                                      norm_cfg=NORM, transformer_norm_cfg=LN), lambda k, b, x: b.run(k, x))
    h.block.load_state_dict(orc.state_dict(), strict=True)
    h.to(dev)
    disable_stochastic(h)
    h.train(True)
    state0 = {k: v.detach().clone() for k, v in h.state_dict().items()}
    ins = [torch.randn((2, CH[i], 16 >> i, 24 >> i), generator=torch.Generator().manual_seed(40 + i)) for i in range(nb)]
    L = _lib.lib()
    count = [0]
    real = L._fns['hrf_fuse_sum_bwd']

    def counted(*a):
        count[0] += 1
        return real(*a)
    L._fns['hrf_fuse_sum_bwd'] = counted
    res = {}
    old = os.environ.get('HRF_FUSE_BWD')
    try:
        for mode in ('0', '1'):
            os.environ['HRF_FUSE_BWD'] = mode
            h.load_state_dict(state0)
            h.zero_grad(set_to_none=True)
            a = [t.clone().to(dev).requires_grad_(True) for t in ins]
            ya = h(*a)
            g = torch.Generator().manual_seed(7)
            cots = [torch.randn(y.shape, generator=g) for y in ya]
            sum((y * k.to(dev)).sum() for y, k in zip(ya, cots)).backward()
            res[mode] = ([t.grad.detach().clone() for t in a],
                         {k: q.grad.detach().clone() for k, q in h.block.named_parameters() if q.grad is not None}, count[0])
    finally:
        L._fns['hrf_fuse_sum_bwd'] = real
        if old is None:
            os.environ.pop('HRF_FUSE_BWD', None)
        else:
            os.environ['HRF_FUSE_BWD'] = old
    (gi0, gp0, n0), (gi1, gp1, n1) = res['0'], res['1']
    assert n0 == 0 and n1 - n0 == nb, f'one fused launch per exchange sum expected: {n0}, {n1}'
    assert gp0.keys() == gp1.keys()
    errs = [(r(p, q), f'input{i}') for i, (p, q) in enumerate(zip(gi1, gi0))]
    gmax = max(float(q.abs().max()) for q in gp0.values())
    for k in gp0:
        if float(gp0[k].abs().max()) < 1e-6 * gmax:         # analytically zero (a bias in front of a train-mode BatchNorm): no scale
            assert float(gp1[k].abs().max()) < 1e-4 * gmax, k
            continue
        errs.append((r(gp1[k], gp0[k]), k))
    print(f'{nb} branches: {len(errs)} gradients, worst {max(errs)[0]:.2e} ({max(errs)[1]})')
    assert max(errs)[0] < TOL, max(errs)


@pytest.mark.parametrize('nb', [3, 4])
def test_fuse_bwd_module_emul(nb):
    run_module(nb, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('nb', [3, 4])
def test_fuse_bwd_module_gpu(nb):
    run_module(nb, 'hip')
