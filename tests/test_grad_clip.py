"""Global gradient-norm clipping in front of the fused AdamW (include/hrfuser_hip.h: hrf_grad_sumsq, hrf_adamw_tick_clip,
hrf_adamw_clipped) and its use by Trainer / ExtractTrainer (max_norm, skip_nonfinite).

Kernel level: synthetic arenas against torch on the CPU (float64 norm, clip_grad_norm_ + torch.optim.AdamW).  Trainer level:
t_nus_bn with one module per stage (tests/test_dp_gloo.py::_short) on 2 images of 64x64 - the smallest size at which the
stride-32 BatchNorms still see 8 samples - in deterministic mode, so the gradients under comparison are stable bits.  Every
case runs on the kernel emulator and, marked gpu, on the device.

Bound of the norm, derived: a float's square is exact in fp64 and the fp64 summation error is <= n * 2^-53 relative, far
below half an fp32 ulp for every n here; so is the one of sqrt and of the product with grad_scale.  total_norm is therefore the
exact value rounded to fp32, give or take the double rounding: within 1 fp32 ulp of the float64 reference rounded to fp32.
"""
import math

import pytest
import torch

import helpers
import hrfuser_oracle as O
import test_kernels as TK
from helpers import build_pair, use_backend
from hrfuser_amd import _lib

TOL = TK.TOL
r = TK.r


@pytest.fixture
def backend():
    """use_backend for the test, the product library selected again afterwards"""
    try:
        yield use_backend
    finally:
        _lib.lib = helpers._REAL_LIB_FN


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.contiguous().reshape(-1).view(torch.uint8).cpu(), b.contiguous().reshape(-1).view(torch.uint8).cpu())


def ulps(a, b):
    """distance of two finite, non-negative floats in fp32 units in the last place"""
    ia = int(torch.tensor(float(a), dtype=torch.float32).view(torch.int32))
    ib = int(torch.tensor(float(b), dtype=torch.float32).view(torch.int32))
    return abs(ia - ib)


def f32(x):
    return float(torch.tensor(x, dtype=torch.float64).float())


def offset_view(t, dev):
    """a copy of `t` on `dev` whose base address is one float off a 16-byte boundary (the arena guarantees 4 bytes only)"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()]
    v.copy_(t)
    return v


def norm_of(L, g, mask, n, gscale, max_norm=0.0, skip=0, state=None, clip=None):
    """hrf_grad_sumsq + hrf_adamw_tick_clip on one arena -> (partials, clip, state)"""
    s = _lib.stream_ptr()
    P = int(L.hrf_grad_sumsq_parts(n))
    partials = torch.full((P,), float('nan'), dtype=torch.float64, device=g.device)
    state = torch.zeros(4, device=g.device) if state is None else state
    if clip is None:
        clip = torch.zeros(8, device=g.device)
        clip[4] = max_norm
    L.hrf_grad_sumsq(g, mask, n, partials, s)
    L.hrf_adamw_tick_clip(state, clip, partials, P, gscale, skip, 0.9, 0.999, s)
    return partials, clip, state


def run_norm(use, name):
    dev = use(name)
    L = _lib.lib()
    pmax = int(L.hrf_grad_sumsq_parts(1 << 40))
    assert 1 <= pmax <= 1024 and L.hrf_grad_sumsq_parts(0) == 1 and L.hrf_grad_sumsq_parts(1) == 1
    gen = torch.Generator().manual_seed(3)
    # 4 * 256 * P_max + 5: a second grid-stride pass of the first thread; 16 * 256 * P_max + 9: a second trip of the unrolled loop
    sizes = [0, 1, 3, 255, 1025, 4 * 256 * pmax + 5, 16 * 256 * pmax + 9]
    gscale = 0.5
    for n in sizes:
        assert 1 <= L.hrf_grad_sumsq_parts(n) <= pmax and L.hrf_grad_sumsq_parts(n) == L.hrf_grad_sumsq_parts(n)
        g = torch.randn(n, generator=gen)
        mask = (torch.rand(n, generator=gen) * 2).floor()                    # decay multipliers 0 / 1 ...
        off = torch.rand(n, generator=gen) < 0.1
        mask[off] = -1.0                                                     # ... and ~10 % without a gradient
        ref = f32(gscale * math.sqrt(float((g.double()[~off] ** 2).sum())))
        ref_all = f32(gscale * math.sqrt(float((g.double() ** 2).sum())))
        gp = g.clone()
        idx = off.nonzero().reshape(-1)
        gp[idx[0::2]] = float('nan')                                         # must not show
        gp[idx[1::2]] = 1e30
        gd, md = offset_view(gp, dev), offset_view(mask, dev)
        assert n == 0 or gd.data_ptr() % 16 == 4
        part, clip, state = norm_of(L, gd, md, n, gscale)
        assert bool(torch.isfinite(part).all()), n                           # every partial was written
        got = float(clip[1])
        print(f'[norm {name}] n = {n}: {got!r} vs {ref!r} ({ulps(got, ref)} ulp), {part.numel()} partials')
        assert ulps(got, ref) <= 1, (n, got, ref)
        assert clip.tolist()[2:] == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and float(clip[0]) == 1.0 and float(state[2]) == 1.0
        part2, clip2, _ = norm_of(L, gd, md, n, gscale)
        assert bits_equal(part, part2) and bits_equal(clip, clip2), n        # no atomics: the same bits every time
        _, clip3, _ = norm_of(L, offset_view(g, dev), None, n, gscale)       # NULL mask: every element counts
        assert ulps(float(clip3[1]), ref_all) <= 1, (n, float(clip3[1]), ref_all)
    # elements of 1e25: torch's fp32 norm overflows, the fp64 partial sums do not (documented divergence)
    n = 1025
    g = torch.randn(n, generator=gen).sign() * 1e25
    assert math.isinf(float(torch.linalg.vector_norm(g)))
    _, clip, _ = norm_of(L, offset_view(g, dev), None, n, 1.0)
    ref = f32(math.sqrt(float((g.double() ** 2).sum())))
    assert math.isfinite(ref) and ulps(float(clip[1]), ref) <= 1 and float(clip[2]) == 1.0


def run_clip_adamw(use, name):
    """three steps against clip_grad_norm_ + torch.optim.AdamW, a decay and a no-decay group, another gradient each step"""
    dev = use(name)
    L, s = _lib.lib(), _lib.stream_ptr()
    gen = torch.Generator().manual_seed(11)
    n, nd = 1000, 600
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (1.0 + k) for k in range(3)]
    mask = torch.cat([torch.ones(nd), torch.zeros(n - nd)])
    norm0 = float(grads[0].double().norm())
    for max_norm in (0.5 * norm0, 10.0 * 3.0 * norm0):
        pd, pn = torch.nn.Parameter(p0[:nd].clone()), torch.nn.Parameter(p0[nd:].clone())
        opt = torch.optim.AdamW([dict(params=[pd], weight_decay=0.01), dict(params=[pn], weight_decay=0.0)], lr=3e-4)
        pk, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        state, clip = torch.zeros(4, device=dev), torch.zeros(8, device=dev)
        clip[4] = max_norm
        pk2, m2, v2, state2 = pk.clone(), m.clone(), v.clone(), state.clone()          # plain hrf_adamw beside it
        md = mask.to(dev)
        P = int(L.hrf_grad_sumsq_parts(n))
        part = torch.zeros(P, dtype=torch.float64, device=dev)
        for k, gr in enumerate(grads):
            pd.grad, pn.grad = gr[:nd].clone(), gr[nd:].clone()
            tn = torch.nn.utils.clip_grad_norm_([pd, pn], max_norm)
            coef = min(1.0, float(torch.tensor(max_norm, dtype=torch.float32) / (tn + 1e-6)))
            opt.step()
            gd = gr.to(dev)
            L.hrf_grad_sumsq(gd, md, n, part, s)
            L.hrf_adamw_tick_clip(state, clip, part, P, 1.0, 0, 0.9, 0.999, s)
            L.hrf_adamw_clipped(pk, gd, m, v, md, n, 3e-4, 0.9, 0.999, 1e-8, 0.01, state, 1.0, clip, s)
            L.hrf_adamw_tick(state2, 0.9, 0.999, s)
            L.hrf_adamw(pk2, gd, m2, v2, md, n, 3e-4, 0.9, 0.999, 1e-8, 0.01, state2, 1.0, s)
            st = [opt.state[q] for q in (pd, pn)]
            em = torch.cat([q['exp_avg'] for q in st])
            ev = torch.cat([q['exp_avg_sq'] for q in st])
            assert abs(float(clip[1]) - float(tn)) <= TOL * float(tn), (k, float(clip[1]), float(tn))
            assert abs(float(clip[0]) - coef) <= TOL * coef, (k, float(clip[0]), coef)
            # Adam's first update is g / (|g| + eps): p alone cannot tell whether the clip was applied - m and v can
            assert r(m, em) < TOL and r(v, ev) < TOL, (k, r(m, em), r(v, ev))
            assert r(pk, torch.cat([pd.data, pn.data])) < TOL
            if max_norm > norm0:
                assert float(clip[0]) == 1.0
                assert bits_equal(pk, pk2) and bits_equal(m, m2) and bits_equal(v, v2) and bits_equal(state, state2)
            else:
                assert float(clip[0]) < 0.6 and not bits_equal(m, m2)
        assert float(state[2]) == 3.0


def run_nonfinite(use, name):
    dev = use(name)
    L, s = _lib.lib(), _lib.stream_ptr()
    gen = torch.Generator().manual_seed(13)
    n = 1000
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    gbad = g.clone()
    gbad[417] = float('inf')
    P = int(L.hrf_grad_sumsq_parts(n))

    def step(skip, gr, pk, m, v, state, clip):
        part = torch.zeros(P, dtype=torch.float64, device=dev)
        L.hrf_grad_sumsq(gr, None, n, part, s)
        L.hrf_adamw_tick_clip(state, clip, part, P, 1.0, skip, 0.9, 0.999, s)
        L.hrf_adamw_clipped(pk, gr, m, v, None, n, 3e-4, 0.9, 0.999, 1e-8, 0.01, state, 1.0, clip, s)
    for max_norm in (0.0, 1.0):
        # skip_nonfinite = 0: torch / mmcv behaviour - the parameter of the Inf gradient becomes NaN (with clipping on, coef = 0
        # and 0 * Inf = NaN as in clip_grad_norm_)
        pk, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        state, clip = torch.zeros(4, device=dev), torch.zeros(8, device=dev)
        clip[4] = max_norm
        step(0, gbad.to(dev), pk, m, v, state, clip)
        pt = torch.nn.Parameter(p0.clone())
        pt.grad = gbad.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
        torch.optim.AdamW([pt], lr=3e-4, weight_decay=0.01).step()
        assert math.isnan(float(pt.data[417])) and math.isnan(float(pk[417]))
        assert bool(torch.equal(torch.isnan(pk.cpu()), torch.isnan(pt.data)))
        assert float(clip[2]) == 0.0 and float(clip[5]) == 0.0 and float(clip[3]) == 0.0 and float(state[2]) == 1.0
        # skip_nonfinite = 1: nothing moves, the step is counted; the finite step behind it is step 1, not 2
        pk, m, v = p0.clone().to(dev), torch.rand(n, generator=gen).to(dev), torch.rand(n, generator=gen).to(dev)
        state, clip = torch.zeros(4, device=dev), torch.zeros(8, device=dev)
        clip[4] = max_norm
        state[3] = 3e-4
        keep = [t.clone() for t in (pk, m, v, state)]
        step(1, gbad.to(dev), pk, m, v, state, clip)
        for a, b in zip((pk, m, v, state), keep):
            assert bits_equal(a, b)
        assert float(clip[3]) == 1.0 and float(clip[2]) == 0.0 and float(clip[5]) == 1.0
        step(1, g.to(dev), pk, m, v, state, clip)
        assert float(state[2]) == 1.0 and float(clip[3]) == 1.0 and float(clip[2]) == 1.0 and float(clip[5]) == 0.0
        assert not bits_equal(pk, keep[0]) and bool(torch.isfinite(pk).all())


def run_nparts0(use, name):
    """nparts == 0: clip is final for this step - clip[0..2] stay, the step count follows clip[5]"""
    dev = use(name)
    L, s = _lib.lib(), _lib.stream_ptr()
    for flag in (0.0, 1.0):
        clip = torch.tensor([0.25, 3.0, 1.0 - flag, 2.0, 7.0, flag, 0.0, 0.0], device=dev)
        before = clip.clone()
        state = torch.zeros(4, device=dev)
        L.hrf_adamw_tick_clip(state, clip, None, 0, 1.0, 1, 0.9, 0.999, s)
        assert bits_equal(clip, before)
        assert float(state[2]) == (0.0 if flag else 1.0)
        if not flag:
            assert abs(float(state[0]) - 0.1) < 1e-6 and abs(float(state[1]) - 0.001) < 1e-6
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
        L.hrf_adamw_tick_clip(torch.zeros(4, device=dev), torch.zeros(8, device=dev), None, 3, 1.0, 0, 0.9, 0.999, s)


KERNEL_RUNS = dict(norm=run_norm, clip_adamw=run_clip_adamw, nonfinite=run_nonfinite, nparts0=run_nparts0)


@pytest.mark.parametrize('case', sorted(KERNEL_RUNS))
def test_clip_kernels_emul(backend, case):
    KERNEL_RUNS[case](backend, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(KERNEL_RUNS))
def test_clip_kernels_gpu(backend, case):
    KERNEL_RUNS[case](backend, 'hip')
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- Trainer level
NEW_ENTRY_POINTS = ('hrf_grad_sumsq', 'hrf_grad_sumsq_parts', 'hrf_adamw_tick_clip', 'hrf_adamw_clipped')


def short(cfg):
    """tests/test_dp_gloo.py::_short"""
    for k in ('stage3', 'stage4', 'LidarStageC'):
        cfg['extra'][k]['num_modules'] = 1


def fresh_net(dev, tag='t_nus_bn'):
    net, _, cfg = build_pair(tag, dev, edit=short)
    net.train()
    return net, cfg


def batch(dev, cfg, seed, B=2, H=64, W=64):
    x, mods = O.seeded_inputs(B, H, W, cfg.get('mod_in_channels', [3, 3]), seed=seed)
    g = torch.Generator().manual_seed(100 + seed)
    cots = [torch.randn((B, H // 4 >> i, W // 4 >> i, c), generator=g).to(dev)
            for i, c in enumerate(cfg['extra']['stage4']['num_channels'])]
    return x.to(dev), [m.to(dev) for m in mods], cots


class CountCalls:
    """counts the calls of every entry point of the loaded library (as tests/test_dp_gloo.py wraps L._fns)"""

    def __init__(self, L):
        self.L, self.n = L, {}

    def __enter__(self):
        self.saved = dict(self.L._fns)
        for name, fn in self.saved.items():
            self.L._fns[name] = (lambda name, fn: (lambda *a: (self.n.__setitem__(name, self.n.get(name, 0) + 1), fn(*a))[1]))(name, fn)
        return self

    def __exit__(self, *exc):
        self.L._fns.update(self.saved)
        return False


def host_norm(g, mask):
    """the norm torch computes from a read-back arena: float64 over the elements that receive a gradient"""
    g, mask = g.detach().double().cpu(), mask.cpu()
    return math.sqrt(float((g[mask >= 0] ** 2).sum()))


def run_trainer_clip(use, name):
    """defaults unchanged (no new entry point, one hrf_adamw_tick + one hrf_adamw), the clip inside Trainer.step, and a huge
    max_norm == the default step bit for bit"""
    from hrfuser_amd.trainer import Trainer
    dev = use(name)
    L = _lib.lib()
    sync = torch.cuda.synchronize if dev.type == 'cuda' else (lambda: None)
    lr = 1e-3
    try:
        with pytest.raises(ValueError):
            Trainer(fresh_net(dev)[0], norm_type=1, max_norm=1.0)
        # ---- default Trainer: the launches of today
        net, cfg = fresh_net(dev)
        x, mods, cots = batch(dev, cfg, 1)
        td = Trainer(net, lr=lr, deterministic=True)
        with CountCalls(L) as cc:
            td.step(x, mods, cots)
        sync()
        assert all(cc.n.get(k, 0) == 0 for k in NEW_ENTRY_POINTS), {k: cc.n.get(k, 0) for k in NEW_ENTRY_POINTS}
        assert cc.n.get('hrf_adamw_tick') == 1 and cc.n.get('hrf_adamw') == 1
        assert td.clip is None and not hasattr(td, '_partials')
        p_default = net._engine().flat_p.clone()
        # ---- A: the gradient of the step, read back
        net, cfg = fresh_net(dev)
        ta = Trainer(net, lr=lr, deterministic=True)
        ta.step(x, mods, cots, grads_only=True)
        sync()
        g_a, mask = net._engine().flat_g.detach().cpu().clone(), ta.wd_mask.cpu().clone()
        ref = host_norm(g_a, mask)
        assert ref > 0 and bool((mask < 0).any())
        # ---- B: the same step clipped to half its norm
        net, cfg = fresh_net(dev)
        tb = Trainer(net, lr=lr, deterministic=True, max_norm=0.5 * ref)
        with CountCalls(L) as cc:
            tb.step(x, mods, cots)
        sync()
        assert [cc.n.get(k, 0) for k in ('hrf_grad_sumsq', 'hrf_adamw_tick_clip', 'hrf_adamw_clipped', 'hrf_adamw_tick', 'hrf_adamw')] == [1, 1, 1, 0, 0]
        got, coef = tb.grad_norm(), tb.clip_coef()
        print(f'[trainer clip {name}] grad_norm {got!r} vs {f32(ref)!r} ({ulps(got, f32(ref))} ulp), coef {coef!r}')
        assert ulps(got, f32(ref)) <= 1, (got, ref)
        c32 = torch.tensor(0.5 * ref, dtype=torch.float32) / (torch.tensor(got, dtype=torch.float32) + 1e-6)
        assert coef == float(c32) and 0.49 < coef < 0.51 and tb.skipped_steps() == 0
        assert bits_equal(tb.clip, torch.tensor([coef, got, 1.0, 0.0, f32(0.5 * ref), 0.0, 0.0, 0.0]))
        assert bits_equal(net._engine().flat_g.cpu(), g_a)                  # (deterministic mode: the same gradient bits as A)
        gr = (g_a * 1.0) * c32                                              # fl(fl(g * grad_scale) * coef)
        one = torch.tensor(1.0, dtype=torch.float32)
        b1, b2 = torch.tensor(0.9, dtype=torch.float32), torch.tensor(0.999, dtype=torch.float32)
        m_ref = b1 * 0.0 + (one - b1) * gr
        v_ref = b2 * 0.0 + (one - b2) * gr * gr
        live = mask >= 0
        m, v = tb.m.cpu(), tb.v.cpu()
        assert bits_equal(m[live], m_ref[live]) and bits_equal(v[live], v_ref[live])
        assert float(m[~live].abs().max()) == 0.0 and float(v[~live].abs().max()) == 0.0       # spans without a gradient stay 0
        assert float(tb.state[2]) == 1.0
        # ---- a huge max_norm: coef = 1, the parameters of the default step bit for bit
        net, cfg = fresh_net(dev)
        th = Trainer(net, lr=lr, deterministic=True, max_norm=1e30)
        th.step(x, mods, cots)
        sync()
        assert th.clip_coef() == 1.0 and ulps(th.grad_norm(), f32(ref)) <= 1
        assert bits_equal(net._engine().flat_p, p_default)
        th.set_max_norm(0.25 * ref)
        assert float(th.clip[4]) == f32(0.25 * ref)
    finally:
        L.hrf_set_deterministic(0)


def test_trainer_clip_emul(backend):
    run_trainer_clip(backend, 'emul')


@pytest.mark.gpu
def test_trainer_clip_gpu(backend):
    run_trainer_clip(backend, 'hip')


def run_extract_clip(use, name):
    """ExtractTrainer, default mode, at the shapes of tests/test_detector.py: ONE norm over the backbone's and the neck's arena.
    With lr = 0 the two arenas still hold the step's gradients afterwards, so the norm is checked twice: against the arenas of
    the SAME step (no noise at all: 1 fp32 ulp), and against the arenas of a max_norm=None twin, whose gradients differ from
    this step's by the order of the floating-point atomics - tests/test_detector.py gates that noise at rel-L2 < 1e-3 per arena
    (1e-4 for the neck's), and | ||a|| - ||b|| | <= ||a - b||, so the two norms agree within 1e-3 relative + 1 ulp."""
    import test_detector as TD
    from hrfuser_amd.detector import ExtractTrainer, make_pyramid_cotangents
    dev = use(name)
    sync = torch.cuda.synchronize if dev.type == 'cuda' else (lambda: None)
    fx, _, _, cfg = TD._pair(dev)
    x, mods = O.seeded_inputs(2, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    x, mods = x.to(dev), [m.to(dev) for m in mods]
    fx.train()
    cots = make_pyramid_cotangents(fx, x, mods)
    eb, en = fx.backbone._engine(), fx.neck._engine()

    def both_norm(tr):
        sq = sum(host_norm(e.flat_g, t.wd_mask) ** 2 for e, t in ((eb, tr.tb), (en, tr.tn)))
        return math.sqrt(sq)
    max_norm = 1e-3
    tr = ExtractTrainer(fx, lr=0.0, weight_decay=0.0, max_norm=max_norm)
    tr.step(x, mods, cots)
    sync()
    got, same = tr.grad_norm(), both_norm(tr)
    assert ulps(got, f32(same)) <= 1, (got, same)
    assert host_norm(en.flat_g, tr.tn.wd_mask) > 1e-3 * same                # the neck's arena is a visible part of it
    c32 = torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(got, dtype=torch.float32) + 1e-6)
    assert tr.clip_coef() == float(torch.clamp(c32, max=1.0)) and tr.clip is tr.tn.clip
    assert float(tr.tb.state[2]) == 1.0 and float(tr.tn.state[2]) == 1.0   # both step counts advanced, the neck's with nparts = 0
    twin = ExtractTrainer(fx, lr=0.0, weight_decay=0.0)
    twin.step(x, mods, cots)
    sync()
    ref = both_norm(twin)
    print(f'[extract clip {name}] grad_norm {got!r}; same step {f32(same)!r}; twin {f32(ref)!r} (rel {abs(got - ref) / ref:.2e})')
    assert abs(got - ref) <= 1e-3 * ref + 2.0 ** -23 * ref, (got, ref)
    assert twin.clip is None


def test_extract_trainer_clip_emul(backend):
    run_extract_clip(backend, 'emul')


@pytest.mark.gpu
def test_extract_trainer_clip_gpu(backend):
    run_extract_clip(backend, 'hip')
