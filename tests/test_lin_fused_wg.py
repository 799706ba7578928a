"""hrf_conv_bwd_data_weight (include/hrfuser_hip.h): the data gradient of a 1x1 convolution and its weight / bias gradient from
ONE launch of the register-only row GEMM (csrc/lin_engine.hip, WG instantiations).

Per shape, on the emulator and on the GPU: dx and the folded moments are bit-equal to what hrf_conv_bwd_data writes for the same
arguments; dw / dbias are within test_kernels.TOL of the float64 autograd reference (built as test_kernels.run_conv builds it)
and of hrf_conv_bwd_weight; on the hrf_bn_bfin_t route the published coefficients are those of hrf_bn_bwd_finalize.  Calls the
contract does not take are refused before anything is launched; in deterministic mode dw / dbias are bit-reproducible."""
import os

import pytest
import torch
import torch.nn.functional as F

import hrfuser_oracle as O
from helpers import build_pair, rel_l2, use_backend
from hrfuser_amd import _lib
from test_kernels import KC, TOL, check_bfin, fold, make_bfin, nhwc, r, refused, zstat

# (B, H, W, Cin, Cout), what runs: 'plain' = out_proj (x rows, bias, accumulate = 1), 'ffn' = CrossFFN fc3 (BatchNorm backward on
# load, act' epilogue with GELU, moments; cA / cB / cC arrays, then hrf_bn_bfin_t)
CASES = [
    ((2, 9, 11, 72, 72), 'plain'),       # 198 rows: 3 full row blocks and a ragged one; 5 channel groups of one tile
    ((2, 6, 5, 144, 144), 'plain'),      # out_proj at 144: the split-K form (9 slabs over the four waves), 9 channel tiles
    ((2, 9, 11, 72, 18), 'ffn'),         # fc3 at 18: one batch of two slabs (the second ragged), 5 tiles per wave
    ((2, 9, 11, 144, 36), 'ffn'),        # fc3 at 36: one batch of three slabs, two channel groups (5 + 4 tiles)
    ((1, 5, 3, 78, 78), 'plain'),        # fewer rows than one block, ragged K and N (dword path)
]
COPIES_CASE = (1, 40, 52, 72, 18)        # 2 080 rows = 33 row blocks into replicated accumulators, then hrf_fold_copies


def _problem(case, kind, dev):
    """operands, and the float64 reference gradients of y = conv1x1(x, w) + bias under dy (autograd, as run_conv)"""
    B, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(sum(case))
    rn = lambda *s: torch.randn(*s, generator=g)
    D = lambda t: None if t is None else t.float().to(dev)
    p = dict(case=case, kind=kind, dev=dev, g=g)
    xraw, w, bias = rn(B, H, W, Cin), rn(Cout, Cin, 1, 1) * 0.2, rn(Cout)
    sc, sh = torch.rand(Cin, generator=g) + 0.5, rn(Cin) * 0.3
    du, yraw = rn(B, H, W, Cout), rn(B, H, W, Cout)
    p.update(xraw=D(xraw), w=D(w), sc=D(sc), sh=D(sh), du=D(du), yraw=D(yraw), base=D(rn(B, H, W, Cin)))
    p['cpu'] = dict(xraw=xraw, w=w, bias=bias, sc=sc, sh=sh, du=du, yraw=yraw)
    return p


def _reference(p, coefs):
    """-> (dw, dbias) in float64 for BatchNorm-backward coefficients `coefs` = (cA, cB, cC) or None"""
    c = p['cpu']
    d = lambda t: t.double()
    x = d(c['xraw'])
    if p['kind'] == 'ffn':
        x = F.gelu(x * d(c['sc']) + d(c['sh']))
    dy = d(c['du'])
    if coefs is not None:
        dy = d(coefs[0]) * dy + d(coefs[1]) * d(c['yraw']) + d(coefs[2])
    wq, bq = d(c['w']).clone().requires_grad_(True), d(c['bias']).clone().requires_grad_(True)
    y = F.conv2d(x.permute(0, 3, 1, 2), wq, bq)
    y.backward(dy.permute(0, 3, 1, 2))
    return wq.grad, bq.grad


def _calls(p, L, coefs, bfin):
    """-> (separate(dx, stats, dw, db), fused(dx, stats, dw, db, copy_stride)) issuing the two routes on the same arguments"""
    B, H, W, Cin, Cout = p['case']
    st = (H * W * Cin, W * Cin, Cin, 1)
    s = _lib.stream_ptr()
    co = coefs if coefs is not None else (None, None, None)
    ffn = p['kind'] == 'ffn'

    def head(dx, stats):
        tail = (0, 1, p['xraw'], Cin, p['sc'], p['sh'], 2, stats) if ffn else (1, 0, None, 0, None, None, 0, None)
        return (p['du'], Cout, 0, p['yraw'] if coefs is not None else None, *co, bfin, p['w'], 1, 1, Cout, B, H, W, Cin, dx, *st, *tail)

    def separate(dx, stats, dw, db):
        L.hrf_conv_bwd_data(*head(dx, stats), s)
        tf = (3, p['sc'], p['sh']) if ffn else (0, None, None)
        # (after the data gradient: on the bfin route that launch has published cA / cB / cC)
        L.hrf_conv_bwd_weight(p['du'], Cout, 0, p['yraw'] if coefs is not None else None, *co, p['xraw'], *st, B, H, W, Cin, 1, 1, Cout,
                              *tf, None, dw, db, s)

    def fused(dx, stats, dw, db, cs=0):
        L.hrf_conv_bwd_data_weight(*head(dx, stats), None if ffn else p['xraw'], 0 if ffn else Cin, dw, db, cs, s)
    return separate, fused


def _outputs(p):
    B, H, W, Cin, Cout = p['case']
    dev = p['dev']
    dx = p['base'].clone() if p['kind'] == 'plain' else torch.zeros(B, H, W, Cin, device=dev)
    return dx, (zstat(Cin, dev) if p['kind'] == 'ffn' else None), torch.zeros(Cout, Cin, device=dev), torch.zeros(Cout, device=dev)


def _compare(p, L, coefs, bfin_pair=None, tag=''):
    """both routes on fresh outputs; the assertions of the module docstring"""
    B, H, W, Cin, Cout = p['case']
    ffn = p['kind'] == 'ffn'
    assert L.hrf_conv_bwd_data_weight_supported(Cin, Cout, B * H * W, 1 if ffn else 0, 1 if coefs is not None else 0) == 1
    outs = []
    for which in (0, 1):
        bfin = None
        if bfin_pair is not None:
            bfin, bt = bfin_pair()
            coefs_dev = (bt['cA'], bt['cB'], bt['cC'])
        else:
            coefs_dev = None if coefs is None else tuple(c.float().to(p['dev']) for c in coefs)
        dx, stats, dw, db = _outputs(p)
        _calls(p, L, coefs_dev, bfin)[which](dx, stats, dw, db)
        if bfin_pair is not None:
            check_bfin(bt)
        outs.append((dx, stats, dw, db))
    (dx0, st0, dw0, db0), (dx1, st1, dw1, db1) = outs
    assert torch.equal(dx0, dx1), (tag, 'dx differs from hrf_conv_bwd_data')
    if ffn:
        assert torch.equal(fold(st0), fold(st1)), (tag, 'moments differ from hrf_conv_bwd_data')
    rw, rb = _reference(p, coefs)
    rw = rw.reshape(Cout, Cin)
    e = (r(dw1, rw), r(db1, rb), r(dw1, dw0), r(db1, db0))
    print(f'{p["case"]} {p["kind"]} {tag}: dw vs fp64 {e[0]:.2e}, db vs fp64 {e[1]:.2e}, dw vs hrf_conv_bwd_weight {e[2]:.2e}, db {e[3]:.2e}')
    assert max(e) < TOL, (tag, e)


def run_case(case, kind, backend):
    dev = use_backend(backend)
    L = _lib.lib()
    p = _problem(case, kind, dev)
    Cout = case[4]
    if kind == 'plain':
        _compare(p, L, None)
        return
    g = p['g']
    cr = (torch.randn(Cout, generator=g), torch.randn(Cout, generator=g) * 0.3, torch.randn(Cout, generator=g) * 0.1)
    _compare(p, L, cr, tag='arrays')
    # hrf_bn_bfin_t: the same synthetic moments for both routes (the writer block adds dgamma / dbeta: fresh buffers per call)
    seeds = iter((7, 7))

    def bfin_pair():
        return make_bfin(L, Cout, 811.0, dev, torch.Generator().manual_seed(next(seeds)))
    _, bt = make_bfin(L, Cout, 811.0, dev, torch.Generator().manual_seed(7))
    cref = tuple(bt['ref_' + k].cpu() for k in ('cA', 'cB', 'cC'))
    _compare(p, L, cref, bfin_pair=bfin_pair, tag='bfin')


@pytest.mark.parametrize('case,kind', CASES, ids=str)
def test_fused_wg_emul(case, kind):
    run_case(case, kind, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('case,kind', CASES, ids=str)
def test_fused_wg_gpu(case, kind):
    run_case(case, kind, 'hip')


def run_copies(backend):
    """33 row blocks add into the HRF_STAT_COPIES replicated accumulators (block index % copies); hrf_fold_copies sums them into
    the gradients"""
    dev = use_backend(backend)
    L = _lib.lib()
    p = _problem(COPIES_CASE, 'ffn', dev)
    B, H, W, Cin, Cout = COPIES_CASE
    g = p['g']
    cr = (torch.randn(Cout, generator=g), torch.randn(Cout, generator=g) * 0.3, torch.randn(Cout, generator=g) * 0.1)
    cd = tuple(c.float().to(dev) for c in cr)
    separate, fused = _calls(p, L, cd, None)
    dx0, st0, dw0, db0 = _outputs(p)
    separate(dx0, st0, dw0, db0)
    n = Cout * Cin + Cout
    acc = torch.zeros(KC * n, device=dev)
    dx1, st1, _, _ = _outputs(p)
    fused(dx1, st1, acc[:Cout * Cin], acc[Cout * Cin:n], n)
    assert torch.equal(dx0, dx1) and torch.equal(fold(st0), fold(st1))
    used = acc.view(KC, n).abs().sum(1)
    assert bool((used > 0).all()), 'every copy receives row blocks'
    grads = torch.zeros(n, device=dev)
    L.hrf_fold_copies(acc, n, torch.arange(n, dtype=torch.int32, device=dev), grads, n, _lib.stream_ptr())
    rw, rb = _reference(p, cr)
    dw1, db1 = grads[:Cout * Cin].view(Cout, Cin), grads[Cout * Cin:]
    e = (r(dw1, rw.reshape(Cout, Cin)), r(db1, rb), r(dw1, dw0), r(db1, db0))
    print(f'{COPIES_CASE} copies: {e}')
    assert max(e) < TOL, e


def test_fused_wg_copies_emul():
    run_copies('emul')


@pytest.mark.gpu
def test_fused_wg_copies_gpu():
    run_copies('hip')


def run_refusals(backend):
    dev = use_backend(backend)
    L = _lib.lib()
    s = _lib.stream_ptr()
    B, H, W = 1, 6, 5
    rn = lambda *sh: torch.randn(*sh, device=dev)

    def call(Cin, Cout, KH=1, stride=1, bnb=False, sX=None):
        sX = Cin if sX is None else sX
        st = (H * W * sX, W * sX, sX, 1)
        dx, dw, db = torch.empty(B, H, W, sX, device=dev), torch.zeros(Cout, Cin, KH, KH, device=dev), torch.zeros(Cout, device=dev)
        co = (rn(Cout), rn(Cout), rn(Cout)) if bnb else (None, None, None)
        fn = lambda: L.hrf_conv_bwd_data_weight(rn(B, H, W, Cout), Cout, 0, rn(B, H, W, Cout) if bnb else None, *co, None,
                                                rn(Cout, Cin, KH, KH), KH, stride, Cout, B, H, W, Cin, dx, *st, 0,
                                                0, None, 0, None, None, 0, None, rn(B, H, W, Cin), Cin, dw, db, 0, s)
        return fn, dx, dw
    for kw in (dict(Cin=72, Cout=72, KH=3), dict(Cin=72, Cout=72, stride=2), dict(Cin=72, Cout=72, sX=80),
               dict(Cin=72, Cout=18), dict(Cin=72, Cout=72, bnb=True)):
        fn, dx, dw = call(**kw)
        refused(fn, dx)
        assert float(dw.abs().max()) == 0.0, kw
    # the query says what the entry point does: narrow contractions only behind a BatchNorm backward, wide ones only without;
    # nothing the LDS-tiled route of hrf_conv_bwd_data claims (72 -> 72 at 2 x 96 x 160 rows)
    Q = L.hrf_conv_bwd_data_weight_supported
    assert (Q(72, 18, 30, 1, 1), Q(72, 18, 30, 1, 0), Q(72, 72, 30, 0, 0), Q(72, 72, 30, 0, 1)) == (1, 0, 1, 0)
    assert Q(72, 72, 30720, 0, 0) == 0 and Q(72, 72, 1920, 0, 0) == 1 and Q(144, 144, 480, 0, 0) == 1
    assert Q(72, 18, 30720, 1, 1) == 1 and Q(144, 36, 7680, 1, 1) == 1
    assert Q(312, 312, 1920, 0, 0) == 0 and Q(156, 156, 480, 0, 0) == 1          # the fused form is built up to 160 channels


def test_fused_wg_refusals_emul():
    run_refusals('emul')


@pytest.mark.gpu
def test_fused_wg_refusals_gpu():
    run_refusals('hip')


def run_deterministic(backend):
    """deterministic mode: dw / dbias go through the registered shadow bins (bit-equal over two runs, within TOL of the
    reference); unregistered accumulators are refused"""
    dev = use_backend(backend)
    L = _lib.lib()
    case = CASES[0][0]
    p = _problem(case, 'plain', dev)
    B, H, W, Cin, Cout = case
    _, fused = _calls(p, L, None, None)
    n = Cout * Cin + Cout
    L.hrf_set_deterministic(1)
    try:
        dx, _, dw, db = _outputs(p)
        refused(lambda: fused(dx, None, dw, db), dx)
        runs = []
        for _ in range(2):
            gbuf = torch.zeros(n, device=dev)
            bins = torch.zeros(L.hrf_det_bins_bytes(n) // 8, dtype=torch.int64, device=dev)
            L.hrf_det_register(gbuf, n, bins)
            try:
                dx, _, _, _ = _outputs(p)
                fused(dx, None, gbuf[:Cout * Cin], gbuf[Cout * Cin:])
                L.hrf_det_resolve(gbuf, n, _lib.stream_ptr())
            finally:
                L.hrf_det_register(gbuf, n, None)
            runs.append(gbuf.clone())
        assert torch.equal(runs[0], runs[1])
        rw, rb = _reference(p, None)
        assert r(runs[0][:Cout * Cin], rw.reshape(-1)) < TOL and r(runs[0][Cout * Cin:], rb) < TOL
    finally:
        L.hrf_set_deterministic(0)


def test_fused_wg_deterministic_emul():
    run_deterministic('emul')


@pytest.mark.gpu
def test_fused_wg_deterministic_gpu():
    run_deterministic('hip')


# ------------------------------------------------------------------ net level
def _step(net, x, mods, dev, mode):
    old = os.environ.get('HRF_LIN_FUSED_WG')
    os.environ['HRF_LIN_FUSED_WG'] = mode
    try:
        net.zero_grad(set_to_none=False)
        xa = x.clone().to(dev).requires_grad_(True)
        ma = [m.clone().to(dev).requires_grad_(True) for m in mods]
        ya = net(xa, list(ma))
        g = torch.Generator().manual_seed(5)
        cots = [torch.randn(t.shape, generator=g).to(dev) for t in ya]
        sum((t * c).sum() for t, c in zip(ya, cots)).backward()
        return ([t.detach().clone() for t in ya], [xa.grad.clone()] + [m.grad.clone() for m in ma],
                {k: (None if q.grad is None else q.grad.detach().clone()) for k, q in net.named_parameters()})
    finally:
        if old is None:
            os.environ.pop('HRF_LIN_FUSED_WG', None)
        else:
            os.environ['HRF_LIN_FUSED_WG'] = old


def _one_per_stage(cfg):
    """one module / one block per stage (the reduction of test_deterministic's emulator steps): every branch width and both
    call sites stay, the emulator step takes a fraction of the time"""
    for st in cfg['extra'].values():
        if isinstance(st, dict) and 'num_modules' in st:
            st['num_modules'] = 1
            if 'num_blocks' in st:
                st['num_blocks'] = [1] * len(st['num_blocks'])


def run_net(backend):
    """t_nus, one training step at 2 x 64 x 96 with HRF_LIN_FUSED_WG=all and one with 0 from the same state: equal outputs, every
    gradient within rel-L2 1e-5 (ten times the gradient noise floor of BASELINE.md 2), zero gradients stay zero.  The fused
    launches are counted: both sites are really taken.  (Emulator: one module / block per stage, see _one_per_stage.)"""
    dev = use_backend(backend)
    net, _, cfg = build_pair('t_nus', dev, edit=_one_per_stage if backend == 'emul' else None)
    net.train(True)
    x, mods = O.seeded_inputs(2, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    state0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    L = _lib.lib()
    count = [0]
    real = L._fns['hrf_conv_bwd_data_weight']

    def counted(*a):
        count[0] += 1
        return real(*a)
    L._fns['hrf_conv_bwd_data_weight'] = counted
    try:
        y1, gi1, gp1 = _step(net, x, mods, dev, 'all')
        n_all = count[0]
        net.load_state_dict(state0)
        y0, gi0, gp0 = _step(net, x, mods, dev, '0')
        assert count[0] == n_all, 'HRF_LIN_FUSED_WG=0 still takes the fused call'
    finally:
        L._fns['hrf_conv_bwd_data_weight'] = real
    print(f'fused launches per step: {n_all}')
    assert n_all > 0
    for a, b in zip(y1, y0):
        assert torch.equal(a, b)
    pairs = [(f'input{i}', ab) for i, ab in enumerate(zip(gi1, gi0))] + [(k, (gp1[k], gp0[k])) for k in gp0]
    nmax = max(float(b.double().norm()) for _, (_, b) in pairs if b is not None)
    gmax = max(float(b.abs().max()) for _, (_, b) in pairs if b is not None)
    worst, zeros = (0.0, ''), 0
    for k, (a, b) in pairs:
        if b is None or float(b.abs().max()) == 0.0:
            assert a is None or float(a.abs().max()) == 0.0, (k, 'a zero gradient became non-zero')
            continue
        if float(b.double().norm()) < 1e-9 * nmax:
            # analytically zero (the bias of a convolution in front of a train-mode BatchNorm, fc3's among them: SURVEY App. E):
            # both routes hold rounding residue of a cancelling sum, which has no rel-L2; gated as helpers.tight_grad_gate gates
            # such tensors, absolutely against the largest gradient of the net.  (Measured on MI355X: these tensors sit at
            # 1e-11 of the largest norm, every other tensor agrees to 2e-7.)
            zeros += 1
            assert float(a.abs().max()) <= 1e-4 * gmax, (k, 'analytically zero', float(a.abs().max()), gmax)
            continue
        e = rel_l2(a, b)
        worst = max(worst, (e, k))
        assert e <= 1e-5, (k, e)
    print(f'{len(pairs)} tensors, {zeros} analytically zero; worst rel-L2 between the routes {worst[0]:.2e} ({worst[1]})')


def test_fused_wg_net_emul():
    run_net('emul')


@pytest.mark.gpu
def test_fused_wg_net_gpu():
    run_net('hip')
