"""Per-head window attention forward with LayerNorm and the q / k / v projections in the kernel (csrc/attention.hip
attn_proj_fwd_kernel, hrf_window_attn_proj_fwd) and its route (runtime.window_attention_proj, width gate HRF_ATTN_PROJ).

  1. C ABI against fp64: LayerNorm -> projections -> O._window_attention_core, pad tokens carrying the projection bias (as
     tests/test_kernels.py::run_attn), `o` and the stored q | k | v by relmax at TOL = 2e-5 - the gate of the incumbent chain
     (hrf_ln_stats + hrf_conv_fwd(LayerNorm on load) + hrf_window_attn_fwd), which runs on the same inputs under the same gate.
  2. the stored q | k | v feed hrf_window_attn_bwd unchanged (run_attn's gates against fp64 autograd).
  3. interface: the _supported truth table, every refusal returns HRF_ERR_ARG and leaves the outputs untouched.
  4. route, module level: a 72-wide HRFormerBlock and a 72-wide fusion block (M = 2) with the gate on and off.
  5. whole net: t_nus_bn with the gate "72,144" under the gates of tests/test_parity_wholenet.py, and twice in deterministic
     mode from the same state, bit-equal.
Every case runs on the CPU emulator (unmarked) and on the GPU (marked gpu); the emulator's whole-net leg is the one module /
one block per stage reduction of t_nus_bn."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import hrfuser_oracle as O
import test_parity_blocks as PB
from helpers import LN, NORM, build_pair, disable_stochastic, relmax, use_backend
from hrfuser_amd import _lib
from hrfuser_amd.profiling import ProfLib
from hrfuser_amd.testing import BlockHarness
import hrfuser_amd.backbone as B
import hrfuser_amd.runtime as R

TOL = 2e-5                  # tests/test_kernels.py TOL; the `out` gate of tests/test_attn_block_abi.py
EPS = 1e-6
TF_LN = 4
CASES = [(18, 1, 1, 7, 7),          # exactly one window
         (36, 2, 2, 6, 15),         # H < 7
         (72, 4, 2, 8, 9),
         (144, 8, 3, 5, 10),        # B = 3, one padded window row
         (78, 2, 2, 10, 13),        # asymmetric centre pad
         (156, 4, 1, 3, 20)]        # C, heads, B, H, W
NAN = float('nan')


@functools.lru_cache(maxsize=None)
def _reference(case, cross):
    """Seeded fp32 inputs and the fp64 reference of one case (computed once, shared by the tests, never modified): q / k / v rows,
    `o`, and the gradients of a seeded dout with respect to q, k, v, the bias table and the pad key / value."""
    C, heads, Bn, H, W = case
    P = Bn * H * W
    g = torch.Generator().manual_seed(1000 * cross + sum(case))
    rn = lambda *s: torch.randn(*s, generator=g)
    t = dict(xq=rn(P, C), lnq_g=1 + 0.1 * rn(C), lnq_b=0.1 * rn(C), w=rn(3 * C, C) / C ** 0.5, b=0.1 * rn(3 * C), rpb=0.5 * rn(169, heads),
             dout=rn(P, C))
    if cross:
        t.update(xkv=rn(P, C), lnkv_g=1 + 0.1 * rn(C), lnkv_b=0.1 * rn(C))
    d = {k: v.double() for k, v in t.items()}
    xnq = F.layer_norm(d['xq'], (C,), d['lnq_g'], d['lnq_b'], EPS)
    xnkv = F.layer_norm(d['xkv'], (C,), d['lnkv_g'], d['lnkv_b'], EPS) if cross else xnq
    w, b = d['w'], d['b']
    q = (xnq @ w[:C].T + b[:C]).requires_grad_(True)
    k = (xnkv @ w[C:2 * C].T + b[C:2 * C]).requires_grad_(True)
    v = (xnkv @ w[2 * C:].T + b[2 * C:]).requires_grad_(True)
    kpad, vpad = b[C:2 * C].clone().requires_grad_(True), b[2 * C:].clone().requires_grad_(True)
    T = d['rpb'].clone().requires_grad_(True)

    def part(x, padval):     # padded tokens carry the projection bias (zero input after LayerNorm)
        return O.window_partition(x.view(Bn, H * W, -1) - padval, H, W) + padval
    ow = O._window_attention_core(O.window_partition(q.view(Bn, H * W, C), H, W), part(k, kpad), part(v, vpad), heads, T,
                                  O.rel_pos_index())
    o = O.window_merge(ow, Bn, H, W).reshape(P, C)
    o.backward(d['dout'])
    ref = dict(q=q.detach(), k=k.detach(), v=v.detach(), o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dT=T.grad, dkpad=kpad.grad,
               dvpad=vpad.grad)
    return t, ref


def _guarded(P, ld, dev):
    """a NaN-filled (P, ld) buffer with one guard row on either side -> (whole allocation, the P rows)"""
    full = torch.full((P + 2, ld), NAN, device=dev)
    return full, full[1:-1]


def _launch(case, cross, store, backend, edit=None, raw=False):
    """One hrf_window_attn_proj_fwd launch on the inputs of _reference -> dict of outputs.  The store buffers have the layout of
    the chain (self: one packed (rows, 3C) buffer; cross: q and a (rows, 2C) k | v buffer) widened by NaN guard columns; without the
    store they are allocated, NaN-filled and NOT handed to the launch.  edit(a): changes the argument struct before the launch;
    raw: call the unchecked symbol and return its status as 'rc'."""
    dev = use_backend(backend)
    L = _lib.lib()
    s = _lib.stream_ptr() if backend == 'hip' else 0
    C, heads, Bn, H, W = case
    P = Bn * H * W
    t, _ = _reference(case, cross)
    D = {k: v.to(dev).contiguous() for k, v in t.items()}
    statq = torch.zeros(P, 2, device=dev)
    L.hrf_ln_stats(D['xq'], P, C, EPS, statq, s)
    ofull, o = _guarded(P, C + 1, dev)
    if cross:
        statkv = torch.zeros(P, 2, device=dev)
        L.hrf_ln_stats(D['xkv'], P, C, EPS, statkv, s)
        qfull, qb = _guarded(P, C + 1, dev)
        kvfull, kvb = _guarded(P, 2 * C + 1, dev)
        dst = ((qb, 1), (kvb, 0), (kvb, C + 1))
        fulls = (qfull, kvfull)
    else:
        qkvfull, qkvb = _guarded(P, 3 * C + 2, dev)
        dst = ((qkvb, 1), (qkvb, C + 1), (qkvb, 2 * C + 1))
        fulls = (qkvfull,)
    Pt = _lib._ptr
    a = _lib.AttnProj()
    a.B, a.H, a.W, a.C, a.heads = Bn, H, W, C, heads
    a.xq, a.xkv = Pt(D['xq']), Pt(D['xkv'] if cross else D['xq'])
    a.lnq_g, a.lnq_b, a.rowstat_q = Pt(D['lnq_g']), Pt(D['lnq_b']), Pt(statq)
    if cross:
        a.lnkv_g, a.lnkv_b, a.rowstat_kv = Pt(D['lnkv_g']), Pt(D['lnkv_b']), Pt(statkv)
    w, b = D['w'], D['b']
    a.wq, a.wk, a.wv = w.data_ptr(), w.data_ptr() + 4 * C * C, w.data_ptr() + 8 * C * C        # rows of one packed Linear
    a.bq, a.bk, a.bv = b.data_ptr(), b.data_ptr() + 4 * C, b.data_ptr() + 8 * C
    a.rpb, a.o, a.ldo = Pt(D['rpb']), Pt(o), C + 1
    if store:
        (qd, qo), (kd, ko), (vd, vo) = dst
        a.q_out, a.ldq, a.qoff = Pt(qd), qd.shape[-1], qo
        a.k_out, a.ldk, a.koff = Pt(kd), kd.shape[-1], ko
        a.v_out, a.ldv, a.voff = Pt(vd), vd.shape[-1], vo
    if edit is not None:
        edit(a)
    res = dict(ofull=ofull, o=o, fulls=fulls, dst=dst, dev=D, statq=statq, statkv=statkv if cross else None)
    if raw:
        res['rc'] = L._dll.hrf_window_attn_proj_fwd(ctypes.addressof(a), ctypes.c_void_p(s))
    else:
        L.hrf_window_attn_proj_fwd(a, s)
    if backend == 'hip':
        torch.cuda.synchronize()
    return res


def _chain(case, cross, backend):
    """the incumbent chain on the same inputs: hrf_ln_stats + hrf_conv_fwd(LayerNorm on load) + hrf_window_attn_fwd -> (q, k, v, o)"""
    dev = use_backend(backend)
    L = _lib.lib()
    s = _lib.stream_ptr() if backend == 'hip' else 0
    C, heads, Bn, H, W = case
    P = Bn * H * W
    t, _ = _reference(case, cross)
    D = {k: v.to(dev).contiguous() for k, v in t.items()}
    strides = (H * W * C, W * C, C, 1)

    def proj(x, g, bt, w, b, out, off):
        stat = torch.zeros(P, 2, device=dev)
        L.hrf_ln_stats(x, P, C, EPS, stat, s)
        L.hrf_conv_fwd(x, *strides, Bn, H, W, C, w, b, 1, 1, w.shape[0], out, out.shape[-1], off, None, None, 0,
                       TF_LN, g, bt, stat, None, None, None, 0.0, s)
    w, b = D['w'], D['b']
    o = torch.zeros(P, C, device=dev)
    if cross:
        q, kv = torch.zeros(P, C, device=dev), torch.zeros(P, 2 * C, device=dev)
        proj(D['xq'], D['lnq_g'], D['lnq_b'], w[:C], b[:C], q, 0)
        proj(D['xkv'], D['lnkv_g'], D['lnkv_b'], w[C:2 * C], b[C:2 * C], kv, 0)
        proj(D['xkv'], D['lnkv_g'], D['lnkv_b'], w[2 * C:], b[2 * C:], kv, C)
        L.hrf_window_attn_fwd(q, C, 0, kv, 2 * C, 0, kv, 2 * C, C, b[C:2 * C], b[2 * C:], D['rpb'], o, C, Bn, H, W, C, heads, s)
        return q, kv[:, :C], kv[:, C:], o
    qkv = torch.zeros(P, 3 * C, device=dev)
    proj(D['xq'], D['lnq_g'], D['lnq_b'], w, b, qkv, 0)
    L.hrf_window_attn_fwd(qkv, 3 * C, 0, qkv, 3 * C, C, qkv, 3 * C, 2 * C, b[C:2 * C], b[2 * C:], D['rpb'], o, C, Bn, H, W, C, heads, s)
    return qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o


def _only_nan_outside(full, cols):
    """every element of the allocation outside rows 1 .. -2 x the given column ranges is still NaN; inside, all finite"""
    inside = torch.zeros_like(full, dtype=torch.bool)
    for c0, c1 in cols:
        inside[1:-1, c0:c1] = True
    return bool(torch.isnan(full[~inside]).all()) and bool(torch.isfinite(full[inside]).all())


def _abi(case, cross, store, backend):
    C = case[0]
    _, ref = _reference(case, cross)
    res = _launch(case, cross, store, backend)
    errs = {'o': relmax(res['o'][:, :C], ref['o'])}
    # pad tokens have no rows in the outputs: exactly the rows x C payload is written, the guard rows / columns stay NaN
    assert _only_nan_outside(res['ofull'], [(0, C)])
    if store:
        for nm, (buf, off) in zip('qkv', res['dst']):
            errs[nm] = relmax(buf[:, off:off + C], ref[nm])
        if cross:
            assert _only_nan_outside(res['fulls'][0], [(1, C + 1)]) and _only_nan_outside(res['fulls'][1], [(0, C), (C + 1, 2 * C + 1)])
        else:
            assert _only_nan_outside(res['fulls'][0], [(1, 3 * C + 1)])
    else:
        assert all(bool(torch.isnan(f).all()) for f in res['fulls'])          # a run without the store leaves them untouched
    # the incumbent chain on the same inputs, same gate
    cq, ck, cv, co = _chain(case, cross, backend)
    cerr = {'o': relmax(co, ref['o']), 'q': relmax(cq, ref['q']), 'k': relmax(ck, ref['k']), 'v': relmax(cv, ref['v'])}
    print(f'[attn_proj {case} cross={cross} store={store} {backend}] new', {k: f'{v:.2e}' for k, v in errs.items()},
          'chain', {k: f'{v:.2e}' for k, v in cerr.items()})
    assert all(v < TOL for v in cerr.values()), ('chain', cerr)
    assert all(v < TOL for v in errs.values()), errs


@pytest.mark.parametrize('store', [False, True])
@pytest.mark.parametrize('cross', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_abi_emul(case, cross, store):
    _abi(case, cross, store, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('store', [False, True])
@pytest.mark.parametrize('cross', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_abi_gpu(case, cross, store):
    _abi(case, cross, store, 'hip')


# ------------------------------------------------------------------------------------------ the store feeds the chain's backward
def _store_bwd(case, cross, backend):
    """hrf_window_attn_bwd on the q | k | v the launch stored, seeded dout, against fp64 autograd of the same reference at the gates
    of tests/test_kernels.py::run_attn"""
    C, heads, Bn, H, W = case
    P = Bn * H * W
    _, ref = _reference(case, cross)
    res = _launch(case, cross, True, backend)
    dev = res['o'].device
    L = _lib.lib()
    s = _lib.stream_ptr() if backend == 'hip' else 0
    (qb, qo), (kb, ko), (vb, vo) = res['dst']
    b = res['dev']['b']
    dq, dk, dv = (torch.zeros_like(x) for x in (qb, kb, vb))
    if kb is vb:
        dv = dk
    if qb is kb:
        dq = dk
    dkb, dvb, dT = torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(169, heads, device=dev)
    L.hrf_window_attn_bwd(qb, qb.shape[-1], qo, kb, kb.shape[-1], ko, vb, vb.shape[-1], vo, b[C:2 * C], b[2 * C:], res['dev']['rpb'],
                          res['dev']['dout'], C, dq, dq.shape[-1], qo, dk, dk.shape[-1], ko, dv, dv.shape[-1], vo, dkb, dvb, dT, 0,
                          Bn, H, W, C, heads, s)
    r = relmax
    assert r(dq[:, qo:qo + C], ref['dq']) < TOL and r(dk[:, ko:ko + C], ref['dk']) < TOL and r(dv[:, vo:vo + C], ref['dv']) < TOL
    assert r(dT, ref['dT']) < TOL
    if (H % 7) or (W % 7):
        assert r(dkb, ref['dkpad']) < 1e-4 and r(dvb, ref['dvpad']) < TOL


BWD_CASES = [((72, 4, 2, 8, 9), False), ((78, 2, 2, 10, 13), True)]


@pytest.mark.parametrize('case,cross', BWD_CASES)
def test_store_feeds_backward_emul(case, cross):
    _store_bwd(case, cross, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('case,cross', BWD_CASES)
def test_store_feeds_backward_gpu(case, cross):
    _store_bwd(case, cross, 'hip')


# ------------------------------------------------------------------------------------------------------------- interface
def _untouched(res):
    return bool(torch.isnan(res['ofull']).all()) and all(bool(torch.isnan(f).all()) for f in res['fulls'])


def _interface(backend):
    use_backend(backend)
    L = _lib.lib()
    for heads in (1, 2, 4, 8):
        assert L.hrf_window_attn_proj_supported(18 * heads, heads) == 1
    for heads in (2, 4):
        assert L.hrf_window_attn_proj_supported(39 * heads, heads) == 1
    for C, heads in ((312, 8), (20, 1), (64, 8)):
        assert L.hrf_window_attn_proj_supported(C, heads) == 0
    case = (36, 2, 1, 7, 9)

    def width(a):
        a.C, a.heads = 64, 8
    refusals = [('unsupported width', False, width)]
    for f in ('xq', 'xkv', 'lnq_g', 'lnq_b', 'rowstat_q', 'wq', 'wk', 'wv', 'rpb', 'o'):
        refusals.append((f'null {f}', False, lambda a, f=f: setattr(a, f, None)))
    for f in ('rowstat_kv', 'lnkv_g', 'lnkv_b'):
        refusals.append((f'cross without {f}', True, lambda a, f=f: setattr(a, f, None)))
    for what, cross, edit in refusals:
        res = _launch(case, cross, True, backend, edit=edit, raw=True)
        assert res['rc'] == 1, what                                   # HRF_ERR_ARG
        assert _untouched(res), what
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):    # ... and through the checked binding
        _launch(case, False, True, backend, edit=width)
    res = _launch(case, True, True, backend, raw=True)
    assert res['rc'] == 0 and not _untouched(res)


def test_interface_emul():
    _interface('emul')


@pytest.mark.gpu
def test_interface_gpu():
    _interface('hip')


# ---------------------------------------------------------------------------------------------------------- module level
FUSION72 = (lambda: B.HRFuserFusionBlock(72, 72, 4, norm_cfg=NORM, transformer_norm_cfg=LN, num_fused_modalities=2,
                                         drop_path=0.2, proj_drop_rate=0.1),
            lambda k, b, x: b.run(k, x[0], x[1:]), lambda: O.HRFuserFusionBlock(72, 4, 4, NORM, LN, 0.2, 2, 0.1),
            lambda m, i: m(i[0], list(i[1:])), [(2, 72, 8, 9)] * 3)
BLOCKS = [('block_c72_h4', 1), ('fusion_c72_M2', 2)]          # case, attention sites per forward


@pytest.fixture
def cases72(monkeypatch):
    monkeypatch.setitem(PB.CASES, 'fusion_c72_M2', FUSION72)


def _module_eval(name, gate, backend):
    """names and shape records of the C-ABI calls of one tape-free eval forward of PB.CASES[name] with the width gate set to `gate`;
    the outputs are checked against the fp64 oracle at the gate of tests/test_parity_blocks.py"""
    dev = use_backend(backend)
    mk_prod, runner, mk_orc, orc_call, shapes = PB.CASES[name]
    orc = mk_orc()
    O.seeded_fill_(orc, 3)
    h = BlockHarness(mk_prod(), runner)
    h.block.load_state_dict(orc.state_dict(), strict=True)
    h.to(dev)
    o64 = orc.double()
    disable_stochastic(h, o64)
    h.train(False)
    o64.train(False)
    ins = [torch.randn(s, generator=torch.Generator().manual_seed(40 + i)) for i, s in enumerate(shapes)]
    real, default = _lib.lib, R._ATTN_PROJ
    prof = ProfLib(real(), timing=False)
    _lib.lib = lambda: prof
    R._ATTN_PROJ = frozenset(gate)
    try:
        with torch.no_grad():
            ya = h(*[t.to(dev) for t in ins])
        if backend == 'hip':
            torch.cuda.synchronize()
    finally:
        _lib.lib = real
        R._ATTN_PROJ = default
    with torch.no_grad():
        yb = orc_call(o64, [t.double() for t in ins])
    yb = list(yb) if isinstance(yb, (list, tuple)) else [yb]
    for p, q in zip(ya, yb):
        assert relmax(p, q) < 1e-4, (name, relmax(p, q))
    return [rec[0] for rec in prof.records], [(rec[0], rec[1]) for rec in prof.records]


def _route_eval(name, sites, backend):
    names, recs = _module_eval(name, (72,), backend)
    mine = [d for n, d in recs if n == 'hrf_window_attn_proj_fwd']
    assert len(mine) == sites and all(d['C'] == 72 and d['heads'] == 4 and d['store'] == 0 for d in mine), names
    assert all(d['cross'] == int(name.startswith('fusion')) for d in mine)
    assert 'hrf_window_attn_fwd' not in names
    assert not any(n == 'hrf_attn_block_fwd' and d['C'] == 72 for n, d in recs), names
    names_off, _ = _module_eval(name, (), backend)
    assert 'hrf_window_attn_proj_fwd' not in names_off and 'hrf_attn_block_fwd' in names_off, names_off


def _route_train(name, sites, backend, monkeypatch):
    """forward + backward with a tape through the output and gradient gates of tests/test_parity_blocks.py::run_case, gate on
    (the launch stores q | k | v, the chain's backward runs on them) and gate off"""
    calls = []
    real = R.window_attention_proj

    def counted(ctx, *a, **kw):
        calls.append(bool(ctx.record))
        return real(ctx, *a, **kw)
    monkeypatch.setattr(R, 'window_attention_proj', counted)
    monkeypatch.setattr(R, '_ATTN_PROJ', frozenset((72,)))
    PB.run_case(name, True, backend)
    assert calls == [True] * sites, calls
    monkeypatch.setattr(R, '_ATTN_PROJ', frozenset())
    PB.run_case(name, True, backend)
    assert len(calls) == sites


@pytest.mark.parametrize('name,sites', BLOCKS)
def test_module_eval_route_emul(cases72, name, sites):
    _route_eval(name, sites, 'emul')


@pytest.mark.parametrize('name,sites', BLOCKS)
def test_module_train_route_emul(cases72, monkeypatch, name, sites):
    _route_train(name, sites, 'emul', monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize('name,sites', BLOCKS)
def test_module_eval_route_gpu(cases72, name, sites):
    _route_eval(name, sites, 'hip')


@pytest.mark.gpu
@pytest.mark.parametrize('name,sites', BLOCKS)
def test_module_train_route_gpu(cases72, monkeypatch, name, sites):
    _route_train(name, sites, 'hip', monkeypatch)


def test_gate_names_an_unbuilt_width(monkeypatch):
    """a listed width the kernel is not built for is an error at the first attention site, not a silent change of route"""
    use_backend('emul')

    class Ctx:
        L = _lib.lib()
    monkeypatch.setattr(R, '_ATTN_PROJ', frozenset((312,)))
    with pytest.raises(_lib.HRFuserHipError, match='312'):
        R.attn_proj_ok(Ctx, 312, 8)
    assert R.attn_proj_ok(Ctx, 72, 4) is False


# ------------------------------------------------------------------------------------------------------------- whole net
def _one_per_stage(cfg):
    """one module / one block per stage: every branch width and both kinds of attention site stay"""
    for st in cfg['extra'].values():
        if isinstance(st, dict) and 'num_modules' in st:
            st['num_modules'] = 1
            if 'num_blocks' in st:
                st['num_blocks'] = [1] * len(st['num_blocks'])


def _train_step(net, x, mods, dev):
    """one train step with fixed cotangents -> the outputs and the concatenated gradients"""
    net.zero_grad(set_to_none=False)
    xa = x.clone().to(dev).requires_grad_(True)
    ma = [m.clone().to(dev).requires_grad_(True) for m in mods]
    ya = net(xa, list(ma))
    g = torch.Generator().manual_seed(5)
    cots = [torch.randn(t.shape, generator=g).to(dev) for t in ya]
    sum((t * c).sum() for t, c in zip(ya, cots)).backward()
    grads = torch.cat([xa.grad.reshape(-1)] + [m.grad.reshape(-1) for m in ma] + [p.grad.reshape(-1) for p in net.parameters()])
    return [t.detach().clone() for t in ya] + [grads.clone()]


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _wholenet(backend, monkeypatch, edit):
    import test_parity_wholenet as TP
    dev = use_backend(backend)
    calls = []
    real = R.window_attention_proj

    def counted(ctx, q_in, *a, **kw):
        calls.append(q_in.shape[-1])
        return real(ctx, q_in, *a, **kw)
    monkeypatch.setattr(R, 'window_attention_proj', counted)
    monkeypatch.setattr(R, '_ATTN_PROJ', frozenset((72, 144)))
    pair = build_pair('t_nus_bn', dev, edit=edit)
    net, _, cfg = pair
    state0 = copy.deepcopy(net.state_dict())
    TP._fwd_bwd('t_nus_bn', 2, 64, 96, True, backend, pair=lambda d: pair)
    assert 72 in calls and 144 in calls and set(calls) <= {72, 144}, calls
    # deterministic mode, twice from the same state: the launch has no cross-block sum and the backward is the chain's
    x, mods = O.seeded_inputs(2, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    L = _lib.lib()
    L.hrf_set_deterministic(1)
    try:
        steps = []
        for _ in range(2):
            net.load_state_dict(state0)
            steps.append(_train_step(net, x, mods, dev))
    finally:
        L.hrf_set_deterministic(0)
    assert float(steps[0][-1].abs().max()) > 0
    for i, (p, q) in enumerate(zip(*steps)):
        assert bits_equal(p, q), f'result {i} differs between two deterministic steps'


def test_wholenet_emul(monkeypatch):
    _wholenet('emul', monkeypatch, _one_per_stage)


@pytest.mark.gpu
def test_wholenet_gpu(monkeypatch):
    _wholenet('hip', monkeypatch, None)
