"""Fused attention forward at head_dim 39 (widths 78 / 156, HRFuser-B / HRFormer-B) and the wave-group forms of the wide widths
(csrc/attn_block.hip: G groups of four waves per window, hrf_debug_knob(36, G)).

  * the new widths against the fp64 block of tests/test_attn_block_abi.py (its runner and its gates, unchanged: out 2e-5, h1 2e-5,
    moments 1e-4, formed tail rows 1e-5), forward only, at the dispatcher's form and at every forced G;
  * every built G against G = 1 on the same inputs, BIT for bit (out, h1, out_rowstat, x_out; the moments at the moment gate, and
    bit for bit in deterministic mode) - with res2, a dropout mask, row scale, and both coefficient routes of the lazy tail;
  * the interface: supported widths, a forced form that is not built is refused before any launch;
  * module level: eval forwards of 78-wide blocks take the launch, training forwards do not."""
import contextlib

import pytest
import torch

import hrfuser_oracle as O
import test_attn_block_abi as ABI
import test_parity_blocks as PB
from helpers import disable_stochastic, relmax, use_backend
from hrfuser_amd import _lib
from hrfuser_amd import runtime as R
from hrfuser_amd.profiling import ProfLib
from hrfuser_amd.testing import BlockHarness

KC = _lib.STAT_COPIES
FORMS = {18: (1,), 36: (1,), 72: (1, 4), 144: (1, 4), 78: (1, 2), 156: (1, 2, 4)}     # wave-group forms built per width

NEW = [  # C, heads, B, H, W
    (78, 2, 1, 7, 7),       # exactly one window
    (78, 2, 2, 10, 13),     # 2 x 2 windows, asymmetric centre pad
    (156, 4, 3, 5, 6),      # H and W < 7: one padded window per sample
    (156, 4, 1, 3, 20),     # H < 7, three windows in a row
]
EQ = [(72, 4, 2, 8, 9), (144, 8, 3, 5, 10), (78, 2, 2, 10, 13), (156, 4, 1, 3, 20)]
# (cross, with_ffn, tail)
VARIANTS = [(False, False, False), (False, True, False), (True, False, False), (True, True, False), (False, True, True)]


@contextlib.contextmanager
def forced(backend, g):
    """hrf_debug_knob(36, g) on the library of `backend`, back to the dispatcher's choice afterwards"""
    use_backend(backend)
    L = _lib.lib()
    L.hrf_debug_knob(36, g)
    try:
        yield L
    finally:
        L.hrf_debug_knob(36, 0)


def _parity(case, g, variant, backend):
    cross, with_ffn, tail = variant
    with forced(backend, g):
        ABI._run(*case, cross, with_ffn, False, backend, tail=tail)


def _case_forms(cases):
    return [(c, g) for c in cases for g in (0,) + FORMS[c[0]]]


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('case,g', _case_forms([NEW[1], NEW[3]]))
def test_new_widths_emul(case, g, variant):
    _parity(case, g, variant, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('case,g', _case_forms(NEW))
def test_new_widths_gpu(case, g, variant):
    _parity(case, g, variant, 'hip')


# ------------------------------------------------------------------------------------------------ bit-equality of the forms
def _launch(case, mode, backend, with_stats=True):
    """One forward on seeded random operands -> {out, h1, rowstat, x_out, stats}.  mode: 'self' | 'cross' (res2, dropout mask,
    mask scale, per-sample row scale) | 'tail' (rows formed on load from coefficient arrays) | 'tail_fin' (... from moments
    finalised on load)."""
    C, heads, B, H, W = case
    dev = use_backend(backend)
    L = _lib.lib()
    g = torch.Generator().manual_seed(17)
    rnd = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev)
    P = _lib._ptr
    rows, N1 = B * H * W, 4 * C
    cross, tail = mode == 'cross', mode.startswith('tail')
    keep = dict(lnq_g=rnd(C) + 1, lnq_b=rnd(C, k=0.1), lnkv_g=rnd(C) + 1, lnkv_b=rnd(C, k=0.1), wqkv=rnd(3 * C, C, k=C ** -0.5),
                bqkv=rnd(3 * C, k=0.1), rpb=rnd(169, heads, k=0.5), wo=rnd(C, C, k=C ** -0.5), bo=rnd(C, k=0.1),
                ln2_g=rnd(C) + 1, ln2_b=rnd(C, k=0.1), w1=rnd(N1, C, k=C ** -0.5), b1=rnd(N1, k=0.1))
    a = _lib.AttnBlock()
    a.B, a.H, a.W, a.C, a.heads = B, H, W, C, heads
    xq = rnd(rows, C) if not tail else torch.full((rows, C), float('nan'), device=dev)
    xkv = rnd(rows, C) if cross else xq
    a.xq, a.xkv, a.res = P(xq), P(xkv), P(xq)
    a.lnq_g, a.lnq_b, a.lnkv_g, a.lnkv_b, a.ln_eps = P(keep['lnq_g']), P(keep['lnq_b']), P(keep['lnkv_g']), P(keep['lnkv_b']), 1e-6
    w, bias = keep['wqkv'], keep['bqkv']
    a.wq, a.bq = w.data_ptr(), bias.data_ptr()
    a.wk, a.bk = w.data_ptr() + 4 * C * C, bias.data_ptr() + 4 * C
    a.wv, a.bv = w.data_ptr() + 8 * C * C, bias.data_ptr() + 8 * C
    a.rpb, a.wo, a.bo = P(keep['rpb']), P(keep['wo']), P(keep['bo'])
    a.mask, a.mscale, a.rowscale, a.rows_per_sample = None, 1.0, None, H * W
    if cross:
        keep['mask'] = (torch.rand(rows, C, generator=g) > 0.1).float().to(dev)
        keep['rs'] = torch.tensor([1.25, 0.0, 1.25][:B] + [1.25] * max(0, B - 3)).to(dev)
        a.res2, a.mask, a.mscale, a.rowscale = P(xkv), P(keep['mask']), 1.0 / 0.9, P(keep['rs'])
    if tail:
        keep.update(t_res=rnd(rows, C), t_raw=rnd(rows, C), t_rs=torch.tensor([1.25, 0.0, 1.25][:B] + [1.25] * max(0, B - 3)).to(dev))
        a.tail_res, a.tail_raw, a.tail_rowscale, a.x_out = P(keep['t_res']), P(keep['t_raw']), P(keep['t_rs']), P(xq)
        if mode == 'tail':
            keep.update(t_sc=(torch.rand(C, generator=g) + 0.5).to(dev), t_sh=rnd(C))
            a.tail_scale, a.tail_shift = P(keep['t_sc']), P(keep['t_sh'])
        else:                                           # folded moments (copies = 1) of the tail's BatchNorm, finalised on load
            cnt = float(rows)
            mean, var = torch.randn(C, generator=g).double() * 0.3, torch.rand(C, generator=g).double() + 0.5
            keep['t_st'] = torch.cat([mean * cnt, (var + mean * mean) * cnt]).to(dev)
            keep.update(t_g=rnd(C) + 1, t_b=rnd(C, k=0.1), t_rm=torch.zeros(C, device=dev), t_rv=torch.ones(C, device=dev),
                        **{k: torch.full((C,), float('nan'), device=dev) for k in ('t_sc', 't_sh', 't_mean', 't_is')})
            keep['fin'] = _lib.BnFin(P(keep['t_st']), P(keep['t_g']), P(keep['t_b']), P(keep['t_rm']), P(keep['t_rv']), P(keep['t_sc']),
                                     P(keep['t_sh']), P(keep['t_mean']), P(keep['t_is']), cnt, 1e-5, 0.1, 1, 1, C, 1, None)
            import ctypes
            a.tail_fin = ctypes.addressof(keep['fin'])
    out = torch.full((rows, C), float('nan'), device=dev)
    rowstat = torch.full((rows, 2), float('nan'), device=dev)
    h1 = torch.full((rows, N1), float('nan'), device=dev)
    stats = torch.zeros(KC * 2 * N1, dtype=torch.float64, device=dev)
    a.out, a.out_rowstat, a.out_eps = P(out), P(rowstat), 1e-6
    a.ln2_g, a.ln2_b, a.w1, a.b1, a.h1, a.hidden = P(keep['ln2_g']), P(keep['ln2_b']), P(keep['w1']), P(keep['b1']), P(h1), N1
    a.stats1 = P(stats) if with_stats else None
    L.hrf_attn_block_fwd(a, _lib.stream_ptr())
    res = dict(out=out, h1=h1, rowstat=rowstat, x_out=xq, stats=stats)
    if mode == 'tail_fin':
        res.update(t_sc=keep['t_sc'], t_sh=keep['t_sh'], t_rm=keep['t_rm'])
    return {k: v.cpu() for k, v in res.items()}


def _forms_equal(case, mode, backend):
    with forced(backend, 1):
        ref = _launch(case, mode, backend)
    assert torch.isfinite(ref['out']).all() and torch.isfinite(ref['h1']).all() and torch.isfinite(ref['rowstat']).all()
    assert not mode.startswith('tail') or torch.isfinite(ref['x_out']).all()
    N1 = 4 * case[0]
    for g in FORMS[case[0]][1:]:
        with forced(backend, g):
            got = _launch(case, mode, backend)
        for k in ref:
            if k != 'stats':
                assert torch.equal(got[k], ref[k]), (case, mode, g, k, float((got[k] - ref[k]).abs().max()))
        sa, sb = got['stats'].view(KC, 2, N1).sum(0), ref['stats'].view(KC, 2, N1).sum(0)
        assert ABI.r(sa[0], sb[0]) < 1e-4 and ABI.r(sa[1], sb[1]) < 1e-4, (case, mode, g)
    return ref


MODES = ['self', 'cross', 'tail', 'tail_fin']


@pytest.mark.parametrize('mode', ['self', 'cross', 'tail'])
@pytest.mark.parametrize('case', EQ)
def test_forms_bit_equal_emul(case, mode):
    _forms_equal(case, mode, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', EQ)
def test_forms_bit_equal_gpu(case, mode):
    _forms_equal(case, mode, 'hip')


def _forms_equal_det(case, backend):
    """deterministic mode: stats1 is tagged, the moments are exact integer sums - the same BINS in every form"""
    use_backend(backend)
    L = _lib.lib()
    L.hrf_set_deterministic(1)
    try:
        with forced(backend, 1):
            ref = _launch(case, 'self', backend)
        for g in FORMS[case[0]][1:]:
            with forced(backend, g):
                got = _launch(case, 'self', backend)
            for k in ref:
                a, b = (got[k].view(torch.int64), ref[k].view(torch.int64)) if k == 'stats' else (got[k], ref[k])
                assert torch.equal(a, b), (case, g, k)
        assert bool((ref['stats'].view(torch.int64) != 0).any())
    finally:
        L.hrf_set_deterministic(0)


@pytest.mark.parametrize('case', [EQ[0], EQ[3]])
def test_forms_bit_equal_deterministic_emul(case):
    _forms_equal_det(case, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('case', EQ)
def test_forms_bit_equal_deterministic_gpu(case):
    _forms_equal_det(case, 'hip')


# ------------------------------------------------------------------------------------------------------------- interface
def _interface(backend):
    use_backend(backend)
    L = _lib.lib()
    for C, heads in ((78, 2), (156, 4)):
        assert L.hrf_attn_block_supported(C, heads) == 1
        assert L.hrf_attn_block_bwd_supported(C, heads) == 0
    for C, heads in ((312, 8), (624, 16), (78, 1), (156, 2)):
        assert L.hrf_attn_block_supported(C, heads) == 0
    for C, heads in ((18, 1), (36, 2), (72, 4), (144, 8)):
        assert L.hrf_attn_block_supported(C, heads) == 1
    assert L.hrf_attn_block_bwd_supported(18, 1) == 1 and L.hrf_attn_block_bwd_supported(72, 4) == 0
    # the query (knob 37) answers with a built form; a forced form that is not built is refused BEFORE any launch
    for C, forms in FORMS.items():
        assert _lib.attn_fwd_form(C) in forms
        for g in (1, 2, 4):
            with forced(backend, g):
                assert _lib.attn_fwd_form(C) == (g if g in forms else 0)
    with pytest.raises(_lib.HRFuserHipError):
        L.hrf_debug_knob(36, 3)
    assert _lib.attn_fwd_form(72) in FORMS[72]
    for case, g in (((78, 2, 1, 7, 7), 4), ((72, 4, 1, 7, 7), 2), ((18, 1, 1, 7, 7), 2)):
        with forced(backend, g):
            with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
                _launch(case, 'self', backend)
    # ... and leaves the outputs as they were: the same call through the raw status
    with forced(backend, 4):
        got = _launch_raw((78, 2, 1, 7, 7), backend)
    assert got['rc'] == 1 and all(bool(torch.isnan(v).all()) for k, v in got.items() if k != 'rc')
    assert _launch_raw((78, 2, 1, 7, 7), backend)['rc'] == 0


def _launch_raw(case, backend):
    """the forward through the unchecked symbol -> status and the (NaN-prefilled) outputs"""
    dev = use_backend(backend)
    L = _lib.lib()
    checked = L._fns['hrf_attn_block_fwd']
    got = {}

    def raw(a, stream):
        import ctypes
        got['rc'] = L._dll.hrf_attn_block_fwd(ctypes.addressof(a), stream)
    L._fns['hrf_attn_block_fwd'] = raw
    try:
        res = _launch(case, 'self', backend, with_stats=False)
    finally:
        L._fns['hrf_attn_block_fwd'] = checked
    got.update({k: res[k] for k in ('out', 'h1', 'rowstat')})
    return got


def test_interface_emul():
    _interface('emul')


@pytest.mark.gpu
def test_interface_gpu():
    _interface('hip')


# ---------------------------------------------------------------------------------------------------------- module level
def _module(name, train, gate=None):
    """-> names of the C-ABI calls of one forward of PB.CASES[name] and the shapes of its fused attention launches; the outputs
    are checked against the fp64 oracle at the tolerance of tests/test_parity_blocks.py.  eval: tape-free; train: with a
    tape.  gate: the width gate of the head_dim 39 widths for this forward (None: its default)."""
    dev = use_backend('hip')
    mk_prod, runner, mk_orc, orc_call, shapes = PB.CASES[name]
    orc = mk_orc()
    O.seeded_fill_(orc, 3)
    h = BlockHarness(mk_prod(), runner)
    h.block.load_state_dict(orc.state_dict(), strict=True)
    h.to(dev)
    o64 = orc.double()
    disable_stochastic(h, o64)
    h.train(train)
    o64.train(train)
    ins = [torch.randn(s, generator=torch.Generator().manual_seed(40 + i)) for i, s in enumerate(shapes)]
    real, default = _lib.lib, R._ATTN_FUSED_D39
    prof = ProfLib(real(), timing=False)
    _lib.lib = lambda: prof
    if gate is not None:
        R._ATTN_FUSED_D39 = gate
    try:
        if train:
            ya = h(*[t.clone().to(dev).requires_grad_(True) for t in ins])
        else:
            with torch.no_grad():
                ya = h(*[t.to(dev) for t in ins])
        torch.cuda.synchronize()
    finally:
        _lib.lib = real
        R._ATTN_FUSED_D39 = default
    with torch.no_grad():
        yb = orc_call(o64, [t.double() for t in ins])
    yb = list(yb) if isinstance(yb, (list, tuple)) else [yb]
    for p, q in zip(ya, yb):
        assert relmax(p, q) < 1e-4, (name, relmax(p, q))
    return [rec[0] for rec in prof.records], [rec[1] for rec in prof.records if rec[0] == 'hrf_attn_block_fwd']


BLOCKS = [('block_c78_h2', 1), ('wide_fusion_c78_M2', 2)]       # case of tests/test_parity_blocks.py, attention launches per forward


@pytest.mark.gpu
@pytest.mark.parametrize('name,launches', BLOCKS)
def test_module_eval_takes_the_fused_forward_gpu(name, launches):
    """with the width gate on (runtime._ATTN_FUSED_D39 / HRF_ATTN_FUSED_D39=1) an eval forward matches its oracle THROUGH the launch"""
    names, recs = _module(name, train=False, gate=True)
    assert len(recs) == launches and all(d['C'] == 78 and d['heads'] == 2 for d in recs), names
    assert 'hrf_window_attn_fwd' not in names


@pytest.mark.gpu
@pytest.mark.parametrize('name,launches', BLOCKS)
def test_module_eval_default_route_gpu(name, launches):
    """the default of the width gate decides the route of an eval forward - the launch, or the per-op chain and no launch"""
    names, recs = _module(name, train=False)
    if R._ATTN_FUSED_D39:
        assert len(recs) == launches and 'hrf_window_attn_fwd' not in names, names
    else:
        assert not recs and 'hrf_window_attn_fwd' in names, names


@pytest.mark.gpu
@pytest.mark.parametrize('gate', [False, True])
@pytest.mark.parametrize('name,launches', BLOCKS)
def test_module_train_keeps_the_per_op_route_gpu(name, launches, gate):
    """the fused backward is not built for 78 / 156: a forward with a tape issues no fused launch, whatever the gate"""
    names, recs = _module(name, train=True, gate=gate)
    assert not recs and 'hrf_window_attn_fwd' in names, names
