"""Deterministic mode (include/hrfuser_hip.h: hrf_set_deterministic): bit-reproducible results under any block schedule.

CPU legs run the kernel sources on the fiber emulator, whose launcher spreads the blocks of a launch over
HRF_EMUL_THREADS worker threads (read at every launch): 1 worker = one fixed order, 8 workers = atomics land in whatever
order the threads reach them.  Every leg runs its case with 1, 8 and 8 workers and compares EVERY tensor argument of every
library call bit for bit; the case's own fp64 comparisons (the runners of test_kernels.py, same TOL) run inside each repeat.

The runners of test_kernels.py are reused unchanged through a proxy library (DetLib) that does what a caller of the C ABI
does in deterministic mode: it owns shadow bins for the fp32 gradient accumulators a call names (dw, dbias, dgamma, dbeta,
dkpad, dvpad, drpb), registers them (hrf_det_register) and resolves them after the call (hrf_det_resolve).  The moments
helpers of that module (`fold`, `_rep_moments`) are swapped for versions that speak the bin format of a deterministic
moment slot.  A replicated slot cannot be finalised ON LOAD in deterministic mode (the entry points refuse it - see
test_refusals_emul - and the runtime issues the stand-alone finalize launches instead), so the runners take their
coefficients as arrays (coef='array') and `make_bfin` hands out the array route: coefficients from hrf_bn_bwd_finalize on the
same deterministic moments.

hrf_attn_block_fwd / _bwd have a runner of their own here (run_attn_block_det): the one of test_attn_block_abi.py sums the
moment copies inline and calls hrf_rpb_grad_all, which the mode refuses; this one folds bins and gathers dRPB per layer with
hrf_rpb_grad, as the engine does in the mode, against the same fp64 block at the same tolerances.
"""
import math
import os
import subprocess
import sys
import time

import pytest
import torch

import helpers
import hrfuser_oracle as O
import test_kernels as TK
from helpers import ROOT, build_pair, use_backend
from hrfuser_amd import _lib

GRAD_ARGS = ('dw', 'dbias', 'dgamma', 'dbeta', 'dkpad', 'dvpad', 'drpb')


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _storage_view(t):
    """the whole storage of `t` as a 1-d float32 tensor (tests pass slices of one scratch buffer as separate accumulators)"""
    return torch.empty(0, dtype=torch.float32, device=t.device).set_(t.untyped_storage())


class DetLib:
    """The library as a deterministic-mode caller uses it (see the module docstring); logs every call's tensor arguments."""

    def __init__(self, lib):
        self.__dict__.update(_lib_=lib, protos=lib.protos, ranges={}, collecting=False, log=[])

    def _register(self, t):
        full = _storage_view(t)
        key = (full.data_ptr(), full.numel())
        ent = self.ranges.get(key)
        if ent is None:
            bins = torch.zeros(self._lib_.hrf_det_bins_bytes(full.numel()) // 8, dtype=torch.int64, device=t.device)
            self._lib_.hrf_det_register(full, full.numel(), bins)
            ent = self.ranges[key] = (full, bins)
        return ent

    def _resolve(self, ents):
        for full, _ in ents:
            self._lib_.hrf_det_resolve(full, full.numel(), _lib.stream_ptr())

    def close(self):
        for full, _ in self.ranges.values():
            self._lib_.hrf_det_register(full, full.numel(), None)
        self.ranges.clear()

    def __getattr__(self, name):
        fn = getattr(self._lib_, name)
        args = self.protos.get(name, [])

        def call(*a):
            touched = [self._register(v) for v, (_, an) in zip(a, args) if an in GRAD_ARGS and isinstance(v, torch.Tensor)]
            rc = fn(*a)
            if name == 'hrf_wgrad_group_begin':
                self.__dict__['collecting'] = True
            elif name == 'hrf_wgrad_group_end':
                self.__dict__['collecting'] = False
                self._resolve(self.ranges.values())
                self.log.append((name, [full.clone() for full, _ in self.ranges.values()]))
            elif not self.collecting:
                self._resolve(touched)
            self.log.append((name, [v.detach().clone() for v in a if isinstance(v, torch.Tensor)]))
            return rc
        return call


def det_fold(st):
    """value of every accumulator of a deterministic moment slot [4 bins][n] (exact integer sum, one rounding)"""
    b = st.cpu().view(torch.int64).view(4, -1).tolist()
    tot = [b[0][i] + (b[1][i] << 40) + (b[2][i] << 80) + (b[3][i] << 120) for i in range(len(b[0]))]
    return torch.tensor([math.ldexp(float(x), -96) for x in tot], dtype=torch.float64)


def det_rep_moments(rows, count, g, dev):
    """a deterministic moment slot holding rows * count: the bins hrf_det_add would leave for one addend per element"""
    torch.rand(TK.KC, 1, 1, generator=g)                       # (same draws as the default-mode helper)
    vals = (rows.double() * count).reshape(-1).tolist()
    bins = [[0] * len(vals) for _ in range(4)]
    for i, v in enumerate(vals):
        x = int(math.ldexp(v, 96))                             # exact; truncates below 2^-96 like the kernel
        sgn, x = (-1 if x < 0 else 1), abs(x)
        for k in range(4):
            bins[k][i] = sgn * ((x >> (40 * k)) & ((1 << 40) - 1))
    return torch.tensor(bins, dtype=torch.int64).view(torch.float64).reshape(-1).contiguous().to(dev)


def det_make_bfin(L, C, count, dev, g, train=1):
    """TK.make_bfin for deterministic mode: no descriptor (finalize on load is refused) - the coefficient arrays ARE what
    hrf_bn_bwd_finalize computed from the deterministic moments"""
    _, t = _REAL_MAKE_BFIN(L, C, count, dev, g, train)
    for k in ('cA', 'cB', 'cC', 'dgamma', 'dbeta'):
        t[k] = t['ref_' + k]
    return None, t


_REAL_MAKE_BFIN = TK.make_bfin


@pytest.fixture
def det_emul(monkeypatch):
    """deterministic mode on the emulator backend, the test_kernels helpers speaking bins; restores everything"""
    use_backend('emul')
    real = helpers._EMUL
    assert TK.KC == 4
    proxy = DetLib(real)
    monkeypatch.setattr(helpers, '_EMUL', proxy)
    monkeypatch.setattr(TK, 'fold', det_fold)
    monkeypatch.setattr(TK, '_rep_moments', det_rep_moments)
    monkeypatch.setattr(TK, 'make_bfin', det_make_bfin)
    old_threads = os.environ.get('HRF_EMUL_THREADS')
    real.hrf_set_deterministic(1)
    try:
        yield proxy
    finally:
        real.hrf_set_deterministic(0)
        proxy.close()
        if old_threads is None:
            os.environ.pop('HRF_EMUL_THREADS', None)
        else:
            os.environ['HRF_EMUL_THREADS'] = old_threads
        _lib.lib = helpers._REAL_LIB_FN


def _repeat_bitwise(proxy, run, workers=(1, 8, 8)):
    """run() under each worker count; every tensor argument of every library call must be the same bits in all repeats"""
    logs = []
    for n in workers:
        os.environ['HRF_EMUL_THREADS'] = str(n)
        del proxy.log[:]
        proxy.close()                                          # (every repeat starts without registered ranges)
        run()
        logs.append(list(proxy.log))
    ref = logs[0]
    assert len(ref) > 0
    for lg in logs[1:]:
        assert [n for n, _ in lg] == [n for n, _ in ref]
        for (name, ta), (_, tb) in zip(ref, lg):
            assert len(ta) == len(tb)
            for i, (p, q) in enumerate(zip(ta, tb)):
                assert bits_equal(p, q), f'{name}: tensor argument {i} differs between worker counts'
    return ref


def run_pointwise_det(backend):
    """The pointwise reductions against plain fp64 math at TK.TOL (TK.run_pointwise writes synthetic moments as raw doubles
    into the copies of a slot, which a deterministic slot does not hold: this is its reduction part, moments through bins)."""
    import torch.nn.functional as F
    dev = use_backend(backend)
    L, s, r, TOL = _lib.lib(), _lib.stream_ptr(), TK.r, TK.TOL
    g = torch.Generator().manual_seed(11)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    D = lambda t: t.float().to(dev)
    # ---- hrf_ln_bwd: both lane layouts, straight into a gradient and through the replicated accumulators
    for rows, C in ((301, 18), (77, 156)):
        x, da = rn(rows, C), rn(rows, C)
        ln = torch.nn.LayerNorm(C, eps=1e-6).double()
        with torch.no_grad():
            ln.weight.copy_(torch.rand(C, generator=g) + 0.5); ln.bias.copy_(rn(C))
        xq = x.double().requires_grad_(True)
        ln(xq).backward(da.double())
        mean = x.double().mean(-1, keepdim=True)
        rstd = (x.double().var(-1, unbiased=False, keepdim=True) + 1e-6).rsqrt()
        rsb = D(torch.cat([mean, rstd], -1))
        dx, dg, db = torch.zeros(rows, C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        L.hrf_ln_bwd(D(da), D(x), rsb, D(ln.weight), rows, C, dx, 0, dg, db, 0, s)
        assert r(dx, xq.grad) < TOL and r(dg, ln.weight.grad) < TOL and r(db, ln.bias.grad) < TOL
        scr = torch.zeros(TK.KC * 2 * C, device=dev)
        L.hrf_ln_bwd(D(da), D(x), rsb, D(ln.weight), rows, C, dx, 0, scr, scr[C:], 2 * C, s)
        tot = scr.view(TK.KC, 2 * C).sum(0)
        assert r(tot[:C], ln.weight.grad) < TOL and r(tot[C:], ln.bias.grad) < TOL
    # ---- hrf_act_bwd, ReLU mode with two moment sets: the vector kernel (C = 20) and the scalar one (C = 21, 300 > 256)
    for rows, C in ((301, 20), (45, 21), (7, 300)):
        dd, oo, ya, yb = rn(rows, C), rn(rows, C), rn(rows, C), rn(rows, C)
        gk = torch.zeros(rows, C, device=dev)
        s1, s2 = TK.zstat(C, dev), TK.zstat(C, dev)
        L.hrf_act_bwd(D(dd), D(oo), D(ya), None, None, None, 1, 0, gk, D(yb), None, s1, s2, None, rows, C, s)
        gr = dd.double() * (oo.double() > 0)
        assert r(gk, gr) < TOL
        for st, y in ((s1, ya), (s2, yb)):
            f = TK.fold(st)
            assert r(f[:C], gr.sum(0)) < TOL and r(f[C:], (gr * y.double()).sum(0)) < TOL
    # ---- deterministic moments -> hrf_bn_finalize -> hrf_affine_act_res: the normalisation torch computes from the same sums
    rows, C = 64, 24
    _, ft = TK.make_fin(L, C, float(rows), dev, g)
    m = TK.fold(ft['stats']) / rows
    mean, var = m[:C], m[C:] - m[:C] ** 2
    sc = ft['gamma'].double().cpu() / (var + 1e-5).sqrt()
    sh = ft['beta'].double().cpu() - mean * sc
    assert r(ft['ref_scale'], sc) < TOL and r(ft['ref_shift'], sh) < TOL and r(ft['ref_mean'], mean) < TOL
    y = rn(rows, C)
    o1 = torch.zeros(rows, C, device=dev)
    L.hrf_affine_act_res(D(y), ft['ref_scale'], ft['ref_shift'], None, None, None, None, None, 1, 1, 0, o1, rows, C, None, 0.0,
                         None, None, s)
    assert r(o1, F.relu(y.double() * sc + sh)) < TOL
    # ---- hrf_nearest_up_bwd / hrf_bilinear_up_bwd: the adjoint of the up-sampling + the moments of the low-resolution BatchNorm
    B, Hs, Ws, f, C = 2, 3, 5, 2, 18
    H, W = Hs * f, Ws * f
    gr, ylow = rn(B, H, W, C), rn(B, Hs, Ws, C)
    du, st = torch.full((B, Hs, Ws, C), float('nan'), device=dev), TK.zstat(C, dev)
    L.hrf_nearest_up_bwd(D(gr), C, 0, B, H, W, C, D(ylow), Hs, Ws, du, st, s)
    ref = gr.double().view(B, Hs, f, Ws, f, C).sum((2, 4))
    fs = TK.fold(st)
    assert r(du, ref) < TOL and r(fs[:C], ref.sum((0, 1, 2))) < TOL and r(fs[C:], (ref * ylow.double()).sum((0, 1, 2))) < TOL
    ylo = rn(B, Hs, Ws, C).double().requires_grad_(True)
    F.interpolate(ylo.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=False).backward(gr.double().permute(0, 3, 1, 2))
    du, st = torch.full((B, Hs, Ws, C), float('nan'), device=dev), TK.zstat(C, dev)
    L.hrf_bilinear_up_bwd(D(gr), C, 0, B, H, W, C, D(ylo.detach()), Hs, Ws, du, st, s)
    fs = TK.fold(st)
    assert r(du, ylo.grad) < TOL and r(fs[:C], ylo.grad.sum((0, 1, 2))) < TOL
    assert r(fs[C:], (ylo.grad * ylo.detach()).sum((0, 1, 2))) < TOL



def run_attn_block_det(C, heads, B, H, W, cross, tail, backend='emul'):
    """hrf_attn_block_fwd / _bwd + hrf_fold_slots + hrf_rpb_grad as test_attn_block_abi._run drives them (with the CrossFFN
    head; `tail`: the preceding block's CrossFFN tail formed on load, its du and BatchNorm moments emitted by the backward),
    against the same fp64 block at the same tolerances - the moments (stats1, tail_gstats) folded from their bins, dRPB
    gathered by the per-layer hrf_rpb_grad.  Every buffer the launches write goes into the proxy's log for the bitwise
    comparison (the argument struct carries pointers, which the proxy cannot log by itself)."""
    import test_attn_block_abi as TA
    r = TA.r
    dev = use_backend(backend)
    L, s, P = _lib.lib(), _lib.stream_ptr(), _lib._ptr
    if cross:
        blk = O.HRFuserFusionBlock(C, heads, 4, helpers.NORM, helpers.LN, 0.0, 1, 0.0)
        msa, lnq, lnkv, ln2 = blk.attn[0].attn, blk.norm1[0], blk.norm2[0], blk.norm3
    else:
        blk = O.HRFormerBlock(C, heads, 4, helpers.NORM, helpers.LN)
        msa, lnq, lnkv, ln2 = blk.attn.attn, blk.norm1, blk.norm1, blk.norm2
    O.seeded_fill_(blk, 5)
    blk = blk.double()
    g = torch.Generator().manual_seed(3)
    if tail:
        assert not cross
        t_res = torch.randn(B, C, H, W, generator=g).double().requires_grad_(True)
        t_raw = torch.randn(B, C, H, W, generator=g).double()
        t_sc, t_sh = (torch.rand(C, generator=g) + 0.5).double(), torch.randn(C, generator=g).double()
        t_rs = torch.tensor([1.25, 0.0, 1.25][:B] + [1.25] * max(0, B - 3)).double()
        t_u = (t_raw * t_sc.view(1, C, 1, 1) + t_sh.view(1, C, 1, 1)).requires_grad_(True)
        x = t_res + t_rs.view(B, 1, 1, 1) * torch.nn.functional.gelu(t_u)
    else:
        x = torch.randn(B, C, H, W, generator=g).double().requires_grad_(True)
    xkv = torch.randn(B, C, H, W, generator=g).double().requires_grad_(True) if cross else x
    out_ref, h1_ref = TA._reference(blk, x, xkv, True, cross, True)

    f32 = lambda t: t.detach().float().contiguous().to(dev)
    rows = lambda t: f32(t.permute(0, 2, 3, 1).reshape(B * H * W, C))
    nan = lambda *sh: torch.full(sh, float('nan'), device=dev)
    M, N1 = B * H * W, 4 * C
    xq_d = rows(x) if not tail else nan(M, C)                   # tail: written by the launch
    xkv_d = rows(xkv) if cross else xq_d
    keep = []

    def dp(t):
        keep.append(f32(t))
        return keep[-1]
    a = _lib.AttnBlock()
    a.B, a.H, a.W, a.C, a.heads = B, H, W, C, heads
    a.xq, a.xkv = P(xq_d), P(xkv_d)
    a.lnq_g, a.lnq_b, a.lnkv_g, a.lnkv_b, a.ln_eps = P(dp(lnq.weight)), P(dp(lnq.bias)), P(dp(lnkv.weight)), P(dp(lnkv.bias)), 1e-6
    if cross:
        a.wq, a.bq, a.wk, a.bk, a.wv, a.bv = (P(dp(t)) for t in (msa.q_proj.weight, msa.q_proj.bias, msa.k_proj.weight,
                                                                 msa.k_proj.bias, msa.v_proj.weight, msa.v_proj.bias))
    else:
        wqkv, bqkv = dp(msa.qkv.weight), dp(msa.qkv.bias)
        a.wq, a.bq = wqkv.data_ptr(), bqkv.data_ptr()
        a.wk, a.bk = wqkv.data_ptr() + 4 * C * C, bqkv.data_ptr() + 4 * C
        a.wv, a.bv = wqkv.data_ptr() + 8 * C * C, bqkv.data_ptr() + 8 * C
    a.rpb, a.wo, a.bo = P(dp(msa.relative_position_bias_table)), P(dp(msa.out_proj.weight)), P(dp(msa.out_proj.bias))
    a.res, a.res2 = P(xq_d), (P(xkv_d) if cross else None)
    a.mask, a.mscale, a.rowscale, a.rows_per_sample = None, 1.0, None, H * W
    if tail:
        tres_d, traw_d = rows(t_res), rows(t_raw)
        a.tail_res, a.tail_raw, a.tail_scale, a.tail_shift, a.tail_rowscale, a.x_out = \
            P(tres_d), P(traw_d), P(dp(t_sc)), P(dp(t_sh)), P(dp(t_rs)), P(xq_d)
    out, h1 = nan(M, C), nan(M, N1)
    stats = torch.zeros(TK.KC * 2 * N1, dtype=torch.float64, device=dev)
    conv1 = blk.ffn.layers[0]
    a.out = P(out)
    a.ln2_g, a.ln2_b, a.out_eps = P(dp(ln2.weight)), P(dp(ln2.bias)), 1e-6
    a.w1, a.b1, a.h1, a.stats1, a.hidden = P(dp(conv1.weight.reshape(N1, C))), P(dp(conv1.bias)), P(h1), P(stats), N1
    L.hrf_attn_block_fwd(a, s)
    assert r(out.reshape(B, H * W, C), out_ref) < 2e-5
    if tail:
        assert r(xq_d.reshape(B, H, W, C).permute(0, 3, 1, 2), x) < 1e-5
    assert r(h1.reshape(B, H * W, N1), h1_ref) < 2e-5
    st = det_fold(stats).view(2, N1)
    assert r(st[0], h1_ref.sum((0, 1))) < 1e-4 and r(st[1], (h1_ref ** 2).sum((0, 1))) < 1e-4

    # ---- backward: loss = <out, gout> + <h1, du1>
    gout = torch.randn(B, H * W, C, generator=g).double()
    du1 = torch.randn(B, H * W, N1, generator=g).double()
    ((out_ref * gout).sum() + (h1_ref * du1).sum()).backward()
    nwin = B * ((H + 6) // 7) * ((W + 6) // 7)
    names = ['w1', 'b1', 'g2', 'bt2', 'wo', 'bo', 'wq', 'bq', 'wk', 'bk', 'wv', 'bv', 'gq', 'btq'] + (['gkv', 'btkv'] if cross else [])
    size = dict(w1=N1 * C, b1=N1, g2=C, bt2=C, wo=C * C, bo=C, wq=C * C, bq=C, wk=C * C, bk=C, wv=C * C, bv=C, gq=C, btq=C, gkv=C, btkv=C)
    offs, slot = {}, 0
    for n in names:
        offs[n] = slot
        slot += size[n]
    pslot, dsp = nan(nwin * slot), nan(nwin * heads * 49 * 49)
    gout_d, du1_d = f32(gout.reshape(-1, C)), f32(du1.reshape(-1, N1))
    cA, cB, cC = torch.ones(N1, device=dev), torch.zeros(N1, device=dev), torch.zeros(N1, device=dev)
    a.gout, a.du1, a.cA1, a.cB1, a.cC1 = P(gout_d), P(du1_d), P(cA), P(cB), P(cC)
    dq, dkv, tdu = nan(M, C), nan(M, C), nan(M, C)
    tgs = torch.zeros(TK.KC * 2 * C, dtype=torch.float64, device=dev)
    a.dq, a.dq_acc, a.dq_add_res = P(dq), 0, 1
    if tail:
        a.tail_du, a.tail_gstats = P(tdu), P(tgs)
    if cross:
        a.dkv, a.dkv_acc, a.dkv_add_res = P(dkv), 0, 1
    park = nan(nwin * 64 * 32)                                  # scratch of the 8-wave 18-channel backward
    a.pslot, a.slot_stride, a.ds_plane, a.gx_park = P(pslot), slot, P(dsp), P(park)
    for n in ('w1', 'b1', 'g2', 'bt2', 'wo', 'bo', 'wq', 'bq', 'wk', 'bk', 'wv', 'bv', 'gq', 'btq', 'gkv', 'btkv', 'rpb'):
        setattr(a, 'off_' + n, offs.get(n, -1))
    L.hrf_attn_block_bwd(a, s)
    if tail:
        assert r(dq.reshape(B, H, W, C).permute(0, 3, 1, 2), t_res.grad) < 5e-5
        du_ref = t_u.grad.permute(0, 2, 3, 1).reshape(-1, C)
        assert r(tdu, du_ref) < 5e-5
        gs = det_fold(tgs).view(2, C)
        raw_rows = t_raw.permute(0, 2, 3, 1).reshape(-1, C)
        assert r(gs[0], du_ref.sum(0)) < 1e-4 and r(gs[1], (du_ref * raw_rows).sum(0)) < 1e-4
    else:
        assert r(dq.reshape(B, H, W, C).permute(0, 3, 1, 2), x.grad) < 5e-5
    if cross:
        assert r(dkv.reshape(B, H, W, C).permute(0, 3, 1, 2), xkv.grad) < 5e-5
    # ---- hrf_fold_slots: the per-window slots into a flat "gradient arena"
    dst = torch.zeros(slot, device=dev)
    seg = torch.tensor([[0, nwin, slot, slot, 0]], dtype=torch.long, device=dev)
    mp = torch.arange(slot, dtype=torch.int32, device=dev)
    L.hrf_fold_slots(pslot, seg, 1, mp, dst, slot, s)
    if cross:
        ref = dict(wo=msa.out_proj.weight, bo=msa.out_proj.bias, wq=msa.q_proj.weight, bq=msa.q_proj.bias, wk=msa.k_proj.weight,
                   wv=msa.v_proj.weight, bv=msa.v_proj.bias, gq=lnq.weight, btq=lnq.bias, gkv=lnkv.weight, btkv=lnkv.bias)
        ref = {k: v.grad.reshape(-1) for k, v in ref.items()}
    else:
        gw, gb = msa.qkv.weight.grad, msa.qkv.bias.grad
        ref = dict(wo=msa.out_proj.weight.grad.reshape(-1), bo=msa.out_proj.bias.grad, wq=gw[:C].reshape(-1), bq=gb[:C],
                   wk=gw[C:2 * C].reshape(-1), wv=gw[2 * C:].reshape(-1), bv=gb[2 * C:], gq=lnq.weight.grad, btq=lnq.bias.grad)
    ref.update(w1=conv1.weight.grad.reshape(-1), b1=conv1.bias.grad, g2=ln2.weight.grad, bt2=ln2.bias.grad)
    gmax = max(float(v.abs().max()) for v in ref.values())
    for n, q in ref.items():
        err = float((dst[offs[n]:offs[n] + size[n]].double().cpu() - q).abs().max()) / max(float(q.abs().max()), 1e-3 * gmax)
        assert err < 1e-4, (n, err)
    # ---- hrf_rpb_grad, one layer: the form the engine issues in deterministic mode (the proxy registers and resolves drpb's bins)
    drpb = torch.zeros(TK.KC * 169 * heads, device=dev)
    L.hrf_rpb_grad(dsp, nwin, heads, drpb, 169 * heads, s)
    assert r(drpb.view(TK.KC, 169, heads).sum(0), msa.relative_position_bias_table.grad) < 1e-4
    L.log.append(('attn_block', [t.clone() for t in (out, h1, stats, xq_d, dq, dkv if cross else dq, tdu if tail else dq, tgs,
                                                      pslot, dsp, dst, drpb)]))



def run_packed_det(C_list, backend='emul'):
    """The one-rank SyncBN forms on deterministic moments (test_attn_block_abi._packed with slots that hold bins): hrf_bn_pack
    resolves the bins into the packed doubles, hrf_bn_finalize_packed / hrf_bn_bwd_finalize_packed on the packed slice equal
    the stand-alone finalize launches on the bins (same tolerances as _packed)."""
    import ctypes
    import test_attn_block_abi as TA
    r = TA.r
    dev = use_backend(backend)
    L, s, P = _lib.lib(), _lib.stream_ptr(), _lib._ptr
    g = torch.Generator().manual_seed(9)
    n, count = len(C_list), 240.0
    stats, ref = [], []
    for C in C_list:
        v = torch.rand(2 * C, generator=g).double()
        v[C:] += 2.0                                         # sum of squares > (sum)^2 / count
        ref.append(v * count)
        stats.append(det_rep_moments(v, count, g, dev))
        assert r(det_fold(stats[-1]), ref[-1]) < 1e-12
    tail = sum(2 * C for C in C_list)
    packed = torch.full((tail + n,), float('nan'), dtype=torch.float64, device=dev)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in stats])
    cs = (ctypes.c_int * n)(*C_list)
    rows = (ctypes.c_double * n)(*[count + 7.0 * i for i in range(n)])
    L.hrf_bn_pack(ptrs, cs, n, rows, packed, s)
    assert r(packed[:tail], torch.cat(ref)) < 1e-12
    assert packed[tail:].tolist() == [count + 7.0 * i for i in range(n)]
    packed[tail:] = count
    off, made = 0, [packed.clone()]
    for li, (C, st) in enumerate(zip(C_list, stats)):
        bufs = {k: torch.zeros(C, device=dev) for k in ('scale', 'shift', 'mean', 'invstd', 'rscale', 'rshift', 'rmean', 'rinvstd')}
        gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
        rm, rv = torch.randn(C, generator=g).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
        rm2, rv2 = rm.clone(), rv.clone()
        L.hrf_bn_finalize(st, gamma, beta, rm2, rv2, count, 1e-5, 0.1, 1, bufs['rscale'], bufs['rshift'], bufs['rmean'],
                          bufs['rinvstd'], C, s)
        fin = _lib.BnFin(None, P(gamma), P(beta), P(rm), P(rv), P(bufs['scale']), P(bufs['shift']), P(bufs['mean']),
                         P(bufs['invstd']), 3.0, 1e-5, 0.1, 1, 1, C, 1, packed.data_ptr() + 8 * (tail + li))
        L.hrf_bn_finalize_packed(fin, 1, packed.data_ptr() + 8 * off, s)
        for k in ('scale', 'shift', 'mean', 'invstd'):
            assert r(bufs[k], bufs['r' + k]) < 1e-6, (C, k)
        assert r(rm, rm2) < 1e-6 and r(rv, rv2) < 1e-6
        mean, invstd = bufs['rmean'], bufs['rinvstd']
        c = {k: torch.zeros(C, device=dev) for k in ('cA', 'cB', 'cC', 'rA', 'rB', 'rC')}
        dg, db, dg2, db2 = (torch.zeros(C, device=dev) for _ in range(4))
        L.hrf_bn_bwd_finalize(st, None, gamma, mean, invstd, count, 1, dg2, db2, c['rA'], c['rB'], c['rC'], C, s)
        bf = _lib.BnBFin(None, P(gamma), P(mean), P(invstd), P(dg), P(db), P(c['cA']), P(c['cB']), P(c['cC']), 3.0, 1, 1, C, 1, None, 0.5,
                         packed.data_ptr() + 8 * (tail + li))
        L.hrf_bn_bwd_finalize_packed(bf, 1, packed.data_ptr() + 8 * off, None, s)
        for k in 'ABC':
            assert r(c['c' + k], c['r' + k]) < 1e-6, (C, k)
        assert r(dg, 0.5 * dg2) < 1e-6 and r(db, 0.5 * db2) < 1e-6
        off += 2 * C
        made += [t.clone() for t in list(bufs.values()) + list(c.values()) + [rm, rv, dg, db]]
    L.log.append(('packed', made))


def _wgrad_tiled_array(case):
    """TK.run_wgrad_tiled with the array route"""
    L = _lib.lib()
    L.hrf_debug_knob(8, 2)
    try:
        TK.run_conv(case, 'emul', coef='array')
    finally:
        L.hrf_debug_knob(8, 0)


KERNEL_LEGS = {
    # hrf_conv_fwd moments (lin engine), hrf_conv_bwd_data gstats, hrf_conv_bwd_weight (pixel-major kernel), coefficient arrays
    'conv_1x1': lambda: TK.run_conv(TK.CONV_CASES[1], 'emul', coef='array'),
    # 3x3: conv3 engine moments, tap-blocked weight gradient + bias gradient, the wgrad3x slab route
    'conv_3x3': lambda: TK.run_conv(TK.CONV_CASES[2], 'emul', coef='array'),
    # generic conv_fwd_kernel / conv_bwd_data_kernel / conv_bwd_wgt_kernel (stride 2, strided input)
    'conv_3x3_s2': lambda: TK.run_conv(TK.CONV_CASES[4], 'emul', coef='array'),
    # hrf_conv_fwd_packed / hrf_conv_bwd_data_packed moments (conv3x engine)
    'conv_packed': lambda: TK.run_conv(TK.C3X_CASES[0], 'emul', packed=True, coef='array'),
    # the LDS-tiled row GEMM (lin2 engine) moments
    'lin2': lambda: TK.run_lin2(TK.LIN2_CASES[1], 1, 'emul', coef='array'),
    # the wgrad_tiled route of hrf_conv_bwd_weight
    'wgrad_tiled': lambda: _wgrad_tiled_array(TK.WT_CASES[5]),
    # hrf_dwconv_fwd moments, hrf_dwconv_bwd_data gstats, hrf_dwconv_bwd_weight (direct, queued, replicated), _bwd_data_weight
    'dwconv': lambda: TK.run_dw(TK.DW_CASES[0], 'emul', coef='array'),
    # hrf_window_attn_bwd: dkpad / dvpad / drpb, direct and replicated
    'attention': lambda: TK.run_attn(TK.ATTN_CASES[0], 'emul'),
    # hrf_ln_bwd, hrf_act_bwd (both kernels), hrf_bn_finalize / hrf_affine_act_res on deterministic moments, the up-sampling adjoints
    'pointwise': lambda: run_pointwise_det('emul'),
    # hrf_attn_block_fwd / _bwd (stats1, per-window slots, dS planes) + hrf_fold_slots + hrf_rpb_grad: self-attention block,
    # the same with the CrossFFN tail on load (tail_gstats), and one modality of a fusion block; edge grids of
    # test_attn_block_abi.EDGE (2 x 2 windows with padding; 36 channels / 2 heads; B = 3 with H, W < 7)
    # the one-rank SyncBN forms: hrf_bn_pack / hrf_bn_finalize_packed / hrf_bn_bwd_finalize_packed on moment bins (one layer
    # wider than HRF_FIN_MAXC)
    'bn_packed': lambda: run_packed_det([18, 624, 72]),
    'attn_block': lambda: run_attn_block_det(18, 1, 2, 10, 13, False, False),
    'attn_block_tail': lambda: run_attn_block_det(36, 2, 1, 3, 20, False, True),
    'attn_block_cross': lambda: run_attn_block_det(18, 1, 3, 5, 6, True, False),
}


@pytest.mark.parametrize('leg', sorted(KERNEL_LEGS))
def test_kernel_bitwise_emul(det_emul, leg):
    """One representative case per reduction entry point: passes its own fp64 comparison at TOL in deterministic mode, and
    every buffer is bit-identical with 1, 8 and 8 emulator workers."""
    _repeat_bitwise(det_emul, KERNEL_LEGS[leg])


def test_rpb_grad_bitwise_emul(det_emul):
    """hrf_rpb_grad with more windows than window chunks (blocks of one head add into the same 169 bins)"""
    import test_attn_block_abi as TA
    _repeat_bitwise(det_emul, lambda: TA._rpb_many_windows('emul'))


def test_det_value_roundtrip_emul(det_emul):
    """The bin arithmetic itself: addends of mixed sign and magnitude 2^-90 ... 2^60 through hrf_ln_bwd-free plumbing -
    hrf_det_resolve of hand-made bins equals the exact sum rounded once to double, then to float; a poisoned accumulator
    (bin 3 at 2^62) resolves to NaN."""
    L = det_emul._lib_
    vals = [1.0, -1.0, 3.5e-20, -7.25e15, 2.0 ** -90, -(2.0 ** -90), 1e-3, 123456.789, -0.3333333, 2.0 ** 40 + 2.0 ** -40]
    g = torch.zeros(4)
    bins = torch.zeros(16, dtype=torch.int64)
    acc = [0, 0, 0, 0]
    for v in vals:                                              # element 0: all addends; element 1: cancels to a tiny negative
        x = int(math.ldexp(v, 96))
        sgn, x = (-1 if x < 0 else 1), abs(x)
        for k in range(4):
            acc[k] += sgn * ((x >> (40 * k)) & ((1 << 40) - 1))
    bins[0:4] = torch.tensor(acc)
    bins[4:8] = torch.tensor([-1, 0, 0, 0]) + torch.tensor([0, 0, 1, -1]) + torch.tensor([0, 0, (1 << 40) - 1, 0])
    bins[8:12] = torch.tensor([5, 0, 0, 1 << 62])               # poisoned
    L.hrf_det_register(g, 4, bins)
    try:
        L.hrf_det_resolve(g, 4, _lib.stream_ptr())
    finally:
        L.hrf_det_register(g, 4, None)
    exact0 = sum(int(math.ldexp(v, 96)) for v in vals)
    assert g[0].item() == torch.tensor(math.ldexp(float(exact0), -96), dtype=torch.float64).float().item()
    exact1 = -1 + ((1 << 40) << 80) - (1 << 120)                # bins [-1, 0, 2^40, -1]  =  -2^-96
    assert exact1 == -1
    assert g[1].item() == torch.tensor(-(2.0 ** -96), dtype=torch.float64).float().item()
    assert math.isnan(g[2].item())
    assert g[3].item() == 0.0
    assert int(bins.abs().sum()) == 0                           # the bins are back at zero


def test_refusals_emul(det_emul):
    """What the mode cannot honour returns HRF_ERR_ARG before any launch (outputs untouched) and succeeds with the mode off."""
    L = det_emul._lib_                                          # (the bare library: nothing registers bins here)
    s = _lib.stream_ptr()
    g = torch.Generator().manual_seed(0)
    # hrf_conv3_wgrad_wide with a bias gradient
    B, H, W, Cin, Cout = 1, 6, 8, 64, 128
    dy, x = torch.randn(B, H, W, Cout, generator=g), torch.randn(B, H, W, Cin, generator=g)
    dw, db = torch.zeros(Cout, Cin, 3, 3), torch.zeros(Cout)
    scr = torch.empty(L.hrf_conv3_wgrad_wide_scratch(B, H, W, Cin, Cout))
    wide = lambda: L.hrf_conv3_wgrad_wide(dy, Cout, x, Cin, B, H, W, Cin, Cout, dw, db, scr, s)
    TK.refused(wide, db)
    # an fp32 gradient accumulator without registered shadow bins
    dwl, dbl = torch.zeros(16, 8, 1, 1), torch.zeros(16)
    xs, dys = torch.randn(1, 4, 5, 8, generator=g), torch.randn(1, 4, 5, 16, generator=g)
    plain = lambda: L.hrf_conv_bwd_weight(dys, 16, 0, None, None, None, None, xs, 160, 40, 8, 1, 1, 4, 5, 8, 1, 1, 16, 0,
                                          None, None, None, dwl, dbl, s)
    TK.refused(plain, dwl)
    # a replicated moment slot finalised on load
    fin, ft = TK.make_fin(L, 8, 20.0, torch.device('cpu'), g)
    o = torch.zeros(20, 8)
    onload = lambda: L.hrf_affine_act_res(xs.reshape(20, 8), None, None, None, None, None, None, None, 1, 1, 0, o, 20, 8, None, 0.0,
                                          fin, None, s)
    TK.refused(onload, o)
    # GroupNorm moments
    mom = torch.zeros(1 * 2 * 8, dtype=torch.float64)
    TK.refused(lambda: L.hrf_gn_moments(xs, None, 1, 20, 8, mom, s), mom)
    # hrf_rpb_grad_all (device-side accumulator table)
    seg = torch.zeros(5, dtype=torch.long)
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
        L.hrf_rpb_grad_all(torch.zeros(49 * 49), seg, 1, 1, 1, s)
    L.hrf_set_deterministic(0)
    dw.zero_(), db.zero_(), dwl.zero_(), dbl.zero_(), mom.zero_()
    wide()
    plain()
    onload()
    L.hrf_gn_moments(xs, None, 1, 20, 8, mom, s)
    assert float(db.abs().max()) > 0 and float(dwl.abs().max()) > 0 and float(mom.abs().max()) > 0


def _one_per_stage(cfg):
    for st in cfg['extra'].values():
        if isinstance(st, dict) and 'num_modules' in st:
            st['num_modules'] = 1
            if 'num_blocks' in st:
                st['num_blocks'] = [1] * len(st['num_blocks'])


def _train_step(net, x, mods, dev):
    """one autograd train step with fixed cotangents -> every result of the step as a flat list of tensors"""
    net.zero_grad(set_to_none=False)
    xa = x.clone().to(dev).requires_grad_(True)
    ma = [m.clone().to(dev).requires_grad_(True) for m in mods]
    ya = net(xa, list(ma))
    g = torch.Generator().manual_seed(5)
    cots = [torch.randn(t.shape, generator=g).to(dev) for t in ya]
    sum((t * c).sum() for t, c in zip(ya, cots)).backward()
    res = [t.detach().clone() for t in ya] + [xa.grad.clone()] + [m.grad.clone() for m in ma]
    res.append(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone())
    res += [b.detach().clone() for b in net.buffers()]
    return res


def test_wholenet_bitwise_emul(det_emul):
    """t_nus_bn reduced to one module (one block) per stage, one train step at 2x64x96 with 1 emulator worker, then 8, from
    the same parameters and running statistics: outputs, input gradients, the concatenated parameter gradients and every
    BatchNorm buffer bit-identical.  The 8-worker step IS the run of test_parity_wholenet._fwd_bwd, i.e. the deterministic
    results themselves pass the oracle gates (relmax < 1e-3, tight_grad_gate 1e-3).  Measured on an 8-thread CPU box: 495 - 530 s
    for the one-worker step (the issue fixes that leg; it is two thirds of the test), 100 s for the eight-worker step, the rest the
    fp32 / fp64 oracle runs of the gate: 650 s alone, 763 s with other tests running beside it; the full config costs ~150 s per
    8-worker step."""
    import copy
    import test_parity_wholenet as TP
    dev = torch.device('cpu')
    helpers._EMUL = det_emul._lib_                              # (the bare library: the net's engine owns its shadow bins)
    net, orc, cfg = build_pair('t_nus_bn', dev, edit=_one_per_stage)
    x, mods = O.seeded_inputs(2, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    net.train(True)
    helpers.enable_relu_probe(net)                              # (as _fwd_bwd does: both steps issue the same launches)
    state0 = copy.deepcopy(net.state_dict())
    nbuf = len(list(net.buffers()))
    os.environ['HRF_EMUL_THREADS'] = '1'
    t0 = time.time()
    one = _train_step(net, x, mods, dev)
    print(f'[deterministic whole net] 1 worker: {time.time() - t0:.1f} s')
    # 8 workers: the same step as issued by the parity gate (same inputs, same cotangents: seed 5 over the outputs in order)
    os.environ['HRF_EMUL_THREADS'] = '8'
    net.load_state_dict(state0)
    net.zero_grad(set_to_none=False)
    seen = {}
    hook = net.register_forward_hook(lambda m, inp, out: seen.update(inp=inp, out=out))
    t0 = time.time()
    try:
        TP._fwd_bwd('t_nus_bn', 2, 64, 96, True, 'emul', pair=lambda d: (net, orc, cfg))
    finally:
        hook.remove()
    print(f'[deterministic whole net] 8 workers + oracle gates: {time.time() - t0:.1f} s')
    xa, ma = seen['inp'][0], list(seen['inp'][1])
    eight = [t.detach().clone() for t in seen['out']] + [xa.grad.clone()] + [m.grad.clone() for m in ma]
    eight.append(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone())
    eight += [b.detach().clone() for b in net.buffers()]
    assert len(one) == len(eight) and float(one[-1 - nbuf].abs().max()) > 0
    for i, (p, q) in enumerate(zip(one, eight)):
        assert bits_equal(p, q), f'result {i} of the step differs between 1 and 8 workers'


def test_other_backbones_emul(det_emul, monkeypatch):
    """Contract point 3: HRFuserHRNetBased and HRFormer RUN in deterministic mode (no refusal) and pass their own oracle gates
    there - one train step each through the runners of test_hrnet_based.py / test_hrformer.py (relmax < 1e-3 on the outputs,
    tight_grad_gate 1e-3); both reduced to one module / one block per stage."""
    import copy
    import test_hrformer as TH
    import test_hrnet_based as TN
    helpers._EMUL = det_emul._lib_                              # (the bare library: each net's engine owns its shadow bins)
    L = det_emul._lib_
    meta = copy.deepcopy(TN._cfg())
    _one_per_stage(meta['cfg'])
    monkeypatch.setattr(TN, '_cfg', lambda: copy.deepcopy(meta))
    TN._run(True, 'emul')
    assert L.hrf_get_deterministic() == 1
    cfgs = copy.deepcopy(TH._cfgs())
    _one_per_stage(cfgs['hrformer_t_bn'])
    monkeypatch.setattr(TH, '_cfgs', lambda: cfgs)
    TH._run('hrformer_t_bn', 2, 64, 64, True, 'emul')           # (its `finally` selects the hip backend again: as every test ends)
    assert L.hrf_get_deterministic() == 1


def test_trainer_and_exchange_refusals_emul(det_emul):
    """The two refusals above the kernels: hrf_p2p_exchange returns HRF_ERR_ARG before it reads its context, and a Trainer
    with more than one rank raises before the step issues anything (the gradient arena keeps its contents); the same Trainer
    runs the check again with the mode off and gets past it."""
    import ctypes
    L = det_emul._lib_
    helpers._EMUL = L
    one = (ctypes.c_int * 1)(8)
    with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
        L.hrf_p2p_exchange(_lib.P2p(), (ctypes.c_void_p * 1)(0), one, 1, (ctypes.c_double * 1)(1.0), (ctypes.c_long * 1)(0), one,
                           None, 0, _lib.stream_ptr())
    from hrfuser_amd.trainer import Trainer
    dev = torch.device('cpu')
    net, _, cfg = build_pair('t_nus_bn', dev, edit=_one_per_stage)
    net.train(True)
    tr = Trainer(net, world_size=2, deterministic=True)
    assert L.hrf_get_deterministic() == 1
    eng = net._engine()
    eng.ready(dev)
    eng.flat_g.fill_(3.0)
    x, mods = O.seeded_inputs(2, 32, 32, cfg.get('mod_in_channels', [3, 3]), seed=1)
    with pytest.raises(_lib.HRFuserHipError, match='deterministic mode'):
        tr._step_impl(x, mods, [])
    assert float(eng.flat_g.min()) == 3.0 and float(eng.flat_g.max()) == 3.0
    net.set_sync_group(None, 1)


def test_stale_bins_and_mode_switch_emul(det_emul):
    """Residue in the shadow bins (a backward pass that died between a producer and the fold) is not added to the next
    step's gradients, and a backward pass refuses to run in the other mode than its forward."""
    dev = torch.device('cpu')
    helpers._EMUL = det_emul._lib_
    os.environ['HRF_EMUL_THREADS'] = '8'
    net, _, cfg = build_pair('t_nus_bn', dev, edit=_one_per_stage)
    net.train(True)
    x, mods = O.seeded_inputs(2, 32, 32, cfg.get('mod_in_channels', [3, 3]), seed=1)
    clean = _train_step(net, x, mods, dev)
    eng = net._engine()
    nbuf = len(list(net.buffers()))
    assert eng._det_bins is not None and not eng.det_dirty
    assert int(eng._det_bins[1].abs().sum()) == 0 and int(eng._det_bins[2].abs().sum()) == 0       # resolve returned them to zero
    eng._det_bins[1].fill_(1 << 30)                             # what an aborted pass leaves: bins not resolved ...
    eng.det_dirty = True                                        # ... and the flag run_backward set still up
    eng._det_bins[2].fill_(1 << 30)
    again = _train_step(net, x, mods, dev)
    # (the running statistics moved on; train-mode results do not read them: everything in front of the buffers must agree)
    for i, (p, q) in enumerate(zip(clean[:len(clean) - nbuf], again[:len(clean) - nbuf])):
        assert bits_equal(p, q), i
    # forward in deterministic mode, backward after the mode was switched off: refused, not misread
    xa = x.clone().requires_grad_(True)
    ya = net(xa, [m.clone() for m in mods])
    det_emul._lib_.hrf_set_deterministic(0)
    try:
        with pytest.raises(Exception, match='other deterministic mode'):
            sum(t.sum() for t in ya).backward()
    finally:
        det_emul._lib_.hrf_set_deterministic(1)


def test_mode_bookkeeping_emul():
    """set_deterministic on the three backbone classes flips hrf_get_deterministic() and clears captured module graphs;
    HRF_DETERMINISTIC=1 sets the initial state of a freshly loaded library."""
    from hrfuser_amd import backbone as BB
    use_backend('emul')
    L = _lib.lib()
    try:
        for cls in (BB.HRFuserHRFormerBased, BB.HRFormer, BB.HRFuserHRNetBased):
            assert callable(getattr(cls, 'set_deterministic', None)), cls
        net, _, _ = build_pair('t_nus_bn', torch.device('cpu'), edit=_one_per_stage)
        assert L.hrf_get_deterministic() == 0
        k0 = net._graph_key((torch.zeros(1, 3, 8, 8),), True)
        net.__dict__['_hrf_graphs'] = {'stale': object()}
        net.set_deterministic(True)
        assert L.hrf_get_deterministic() == 1
        assert '_hrf_graphs' not in net.__dict__               # reset_graphs ran
        assert net._graph_key((torch.zeros(1, 3, 8, 8),), True) != k0   # the mode is part of the module-graph signature
        net.set_deterministic(False)
        assert L.hrf_get_deterministic() == 0
        assert net._graph_key((torch.zeros(1, 3, 8, 8),), True) == k0
    finally:
        L.hrf_set_deterministic(0)
        _lib.lib = helpers._REAL_LIB_FN
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import build_emul\n'
            'from hrfuser_amd import _lib\n'
            'print("state", _lib.Lib(build_emul.build(), require_cuda=False).hrf_get_deterministic())\n'
            % (ROOT, os.path.join(ROOT, 'tests', 'emul')))
    for val, want in (('1', 'state 1'), ('0', 'state 0')):
        out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, HRF_DETERMINISTIC=val), capture_output=True,
                             text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        assert want in out.stdout, out.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU
_GPU_CHILD = r'''
import json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, 'tests')); sys.path.insert(0, os.path.join({root!r}, 'oracle'))
import torch
import hrfuser_oracle as O
from helpers import build_pair
from hrfuser_amd.trainer import Trainer
mode, tag, H, W, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
dev = torch.device('cuda:0')
net, _, cfg = build_pair(tag, dev)
net.train(True)
x, mods = O.seeded_inputs(2, H, W, cfg.get('mod_in_channels', [3, 3]), seed=1)
x, mods = x.to(dev), [m.to(dev) for m in mods]
with torch.no_grad():
    shapes = [t.shape for t in net(x, list(mods))]
g = torch.Generator().manual_seed(5)
cots = [torch.randn(s, generator=g).to(dev) for s in shapes]
eng = net._engine()
def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()
if mode == 'repro':
    # three eager steps, capture, three replays - all from the same parameters and running statistics
    tr = Trainer(net, lr=0.0, deterministic=True)
    tr.step(x, mods, cots, grads_only=True)                   # (allocations, engine setup)
    torch.cuda.synchronize()
    p0, rs0, nbt0 = eng.flat_p.clone(), eng.rstat.clone(), eng.nbt_flat.clone()
    def restore():
        eng.flat_p.copy_(p0); eng.rstat.copy_(rs0); eng.nbt_flat.copy_(nbt0)
    def snap(outs):
        torch.cuda.synchronize()
        return [bits(eng.flat_g), bits(eng.rstat)] + [bits(o.t) for o in outs]
    runs = []
    for _ in range(3):
        restore()
        runs.append(snap(tr.step(x, mods, cots, grads_only=True)))
    restore()
    tr.optimizer_step = lambda: None                          # the captured step = the same grads-only step
    tr.capture(x, mods, cots, warmup=1)
    for _ in range(3):
        restore()
        tr.replay()
        runs.append(snap(tr._graph_outs))
    same = all(all(torch.equal(a, b) for a, b in zip(runs[0], r)) for r in runs[1:])
    nz = int((eng.flat_g != 0).sum())
    json.dump(dict(same=bool(same), nonzero=nz, runs=len(runs)), open(out, 'w'))
elif mode == 'train':
    tr = Trainer(net, lr=3e-4, deterministic=True)
    for _ in range(6):
        tr.step(x, mods, cots)
    torch.cuda.synchronize()
    open(out, 'wb').write(bits(eng.flat_p).numpy().tobytes())
elif mode == 'stale':
    # module-boundary graphs: warm up + capture in default mode, toggle, the next call must not replay that graph
    xa = x.clone().requires_grad_(True)
    for _ in range(4):
        net(xa, list(mods))
    keys0 = set(k for k in net.__dict__.get('_hrf_graphs', {{}}) if k != '_setup')
    captured0 = [k for k in keys0 if net.__dict__['_hrf_graphs'][k].fwd is not None]
    net.set_deterministic(True)
    cleared = '_hrf_graphs' not in net.__dict__
    net(xa, list(mods))
    ents = {{k: e for k, e in net.__dict__.get('_hrf_graphs', {{}}).items() if k != '_setup'}}
    json.dump(dict(captured_before=len(captured0), cleared=bool(cleared), keys_after=len(ents),
                   calls_after=[e.calls for e in ents.values()], replayed=[e.fwd is not None for e in ents.values()],
                   det_in_key=[k[-1] for k in ents]), open(out, 'w'))
'''


def _gpu_child(tmp_path, mode, tag, H, W, timeout, name='out'):
    out = tmp_path / name
    script = tmp_path / 'child.py'
    script.write_text(_GPU_CHILD.format(root=ROOT))
    r = subprocess.run([sys.executable, str(script), mode, tag, str(H), str(W), str(out)], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (mode, tag, r.returncode, r.stderr[-3000:])       # nothing more runs on the GPU after a failure
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('tag,H,W', [('t_nus', 384, 640), ('b_nus', 64, 96), ('t_stf', 64, 96)])
def test_step_reproducible_gpu(tmp_path, tag, H, W):
    """Three eager Trainer.step(grads_only=True), capture, three replays from the same state: flat_g, the running statistics
    and the four outputs bitwise equal across all six runs."""
    import json
    res = json.load(open(_gpu_child(tmp_path, 'repro', tag, H, W, timeout=600)))
    assert res['runs'] == 6 and res['nonzero'] > 0
    assert res['same'], res


@pytest.mark.gpu
def test_training_reproducible_gpu(tmp_path):
    """Two fresh processes, 6 AdamW steps of t_nus at 2x64x96 with lr = 3e-4 on one seeded batch: byte-identical parameters."""
    a = _gpu_child(tmp_path, 'train', 't_nus', 64, 96, timeout=600, name='p_a').read_bytes()
    b = _gpu_child(tmp_path, 'train', 't_nus', 64, 96, timeout=600, name='p_b').read_bytes()
    assert len(a) > 0 and a == b


@pytest.mark.gpu
def test_parity_deterministic_gpu():
    """One deterministic-mode train step of t_nus at 2x64x96 through the output and gradient gates of
    test_parity_wholenet.py::test_wholenet_gpu_train_small."""
    import test_parity_wholenet as TP
    use_backend('hip')
    L = _lib.lib()
    L.hrf_set_deterministic(1)
    try:
        TP._fwd_bwd('t_nus', 2, 64, 96, True, 'hip', gold_key='B2_64x96')
    finally:
        L.hrf_set_deterministic(0)


@pytest.mark.gpu
def test_other_backbones_gpu():
    """HRFormer-T and HRFuserHRNetBased, one deterministic-mode train step each at 2x64x96 through the oracle gates of their own
    test files (outputs against the reference goldens / the fp64 oracle at 1e-3, tight_grad_gate 1e-3)."""
    import test_hrformer as TH
    import test_hrnet_based as TN
    use_backend('hip')
    L = _lib.lib()
    L.hrf_set_deterministic(1)
    try:
        TH._run('hrformer_t_bn', 2, 64, 96, True, 'hip')
        assert L.hrf_get_deterministic() == 1
        TN._run(True, 'hip')
    finally:
        L.hrf_set_deterministic(0)


@pytest.mark.gpu
def test_no_stale_graph_gpu(tmp_path):
    """Toggling the mode between calls of one input signature: the captured module graphs are dropped and the call after the
    toggle is an eager one under a new signature."""
    import json
    res = json.load(open(_gpu_child(tmp_path, 'stale', 't_nus', 64, 96, timeout=600)))
    assert res['cleared'], res
    assert res['keys_after'] >= 1 and all(c == 1 for c in res['calls_after']) and not any(res['replayed']), res
    assert all(d == 1 for d in res['det_in_key']), res
