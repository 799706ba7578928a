"""Gradient accumulation in the Trainer (step_accumulated / capture_accumulated): k micro-batches, one optimizer step.

t_nus_bn with one module per stage on 2 images of 64x64 (see tests/test_grad_clip.py), deterministic mode: the gradients under
comparison are stable bits, so "equal" below means bit for bit.

Bound of the accumulated arena against the host sum of the two separately computed arenas, per tensor, derived: every leaf adds
its micro-batch's partial to what the arena holds, so an element of the cycle's arena is fl(fl(a) + b) where the two separate
steps give fl(a) and fl(b) - at most two extra fp32 roundings (2^-24 relative each) at the magnitude of the partials; with a
factor 2 of margin  || acc - (g1 + g2) ||_2  <=  4 * 2^-24 * (|| g1 ||_2 + || g2 ||_2).
"""
import os
import subprocess
import sys

import pytest
import torch

from hrfuser_amd import _lib
from test_grad_clip import backend, batch, bits_equal, f32, fresh_net, host_norm, ulps      # noqa: F401  (backend: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_RESULTS = {}


def accumulation(use, name):
    """Everything the accumulation tests compare, computed once per backend (8 forward / backward passes; host copies):
    g1, g2: the arenas of two separate step(grads_only=True) calls on b1 and b2, one after the other; acc: the arena of
    step_accumulated([b1, b2], grads_only=True) on a fresh net of the same seed (the same BatchNorm running state to start
    from); then two step_accumulated([b1, b2]) with lr > 0, each from that start state."""
    if name in _RESULTS:
        return _RESULTS[name]
    from hrfuser_amd.trainer import Trainer
    dev = use(name)
    L = _lib.lib()
    sync = torch.cuda.synchronize if dev.type == 'cuda' else (lambda: None)
    H = lambda t: t.detach().cpu().clone()
    res = {}
    try:
        net, cfg = fresh_net(dev)
        b1, b2 = batch(dev, cfg, 1), batch(dev, cfg, 2)
        eng = net._engine()
        tr = Trainer(net, lr=0.0, deterministic=True)
        tr.step(*b1, grads_only=True)
        sync()
        res['g1'] = H(eng.flat_g)
        tr.step(*b2, grads_only=True)
        sync()
        res['g2'] = H(eng.flat_g)
        res['stats_ref'] = (H(eng.rstat), H(eng.nbt_flat))
        net, cfg = fresh_net(dev)
        eng = net._engine()
        tr = Trainer(net, lr=1e-3, deterministic=True)
        with pytest.raises(ValueError):
            tr.step_accumulated([])
        tr._setup(dev)
        state = (eng.flat_p, eng.rstat, eng.nbt_flat, tr.m, tr.v, tr.state)
        keep = [t.clone() for t in state]

        def restore():
            for t, k in zip(state, keep):
                t.copy_(k)
        outs = tr.step_accumulated([b1, b2], grads_only=True)
        sync()
        res['outs'] = (len(outs), len(outs[0]))
        res['acc'] = H(eng.flat_g)
        res['stats'] = (H(eng.rstat), H(eng.nbt_flat))
        res['grads_only'] = (H(eng.flat_p), H(keep[0]), float(tr.state[2]))
        res['names'] = [n for n, _ in net.named_parameters()]
        res['spans'] = list(eng._spans)
        res['live'] = H(tr.wd_mask) >= 0
        for k in ('first', 'repeat'):
            restore()
            tr.step_accumulated([b1, b2])
            sync()
            res[k] = dict(g=H(eng.flat_g), m=H(tr.m), p=H(eng.flat_p), t=float(tr.state[2]))
    finally:
        L.hrf_set_deterministic(0)
    _RESULTS[name] = res
    return res


def check_gradient_bound(use, name):
    """|| acc - (g1 + g2) ||_2 <= 4 * 2^-24 * (|| g1 ||_2 + || g2 ||_2) for every parameter tensor.

    The tensors that decide this are the analytically-zero ones: the key biases of the cross-attention blocks on the 4x4 / 2x2
    maps receive two leaves of magnitude 1 ... 30 that cancel (the k_proj bias gradient over the real tokens and the pad-key
    gradient of the mostly padded 7x7 windows), and what remains is 1e-5 where other tensors have 5e1 ... 1.8e5.  In
    deterministic mode both leaves meet in the same shadow bins (runtime._conv_backward), so a pass adds ONE exactly summed,
    once rounded value per element to the arena; two separately rounded adds miss this bound by 7e4 ... 2e5 on those six
    tensors (measured before that change: errors of 5e-7 ... 4.6e-6).  Measured now, MI355X: 0 of 1185 tensors above the bound,
    the largest at 0.14 of it."""
    res = accumulation(use, name)
    acc, g1, g2 = res['acc'], res['g1'], res['g2']
    assert not bits_equal(g1, g2)
    assert float((acc.double() - g1.double()).norm()) > 0.1 * float(g2.double().norm())            # the second micro-batch is in there
    rows = []
    for pname, (off, cnt) in zip(res['names'], res['spans']):
        a, p, q = (t[off:off + cnt].double() for t in (acc, g1, g2))
        err, lim = float((a - (p + q)).norm()), 4 * 2.0 ** -24 * (float(p.norm()) + float(q.norm()))
        rows.append((err / lim if lim > 0 else (0.0 if err == 0 else float('inf')), err, lim, pname))
    rows.sort(reverse=True)
    bad = [r for r in rows if r[1] > r[2]]
    print(f'[accumulation {name}] {len(rows)} tensors, {len(bad)} above the bound; largest err / bound:')
    for q, err, lim, pname in rows[:max(8, len(bad) + 2)]:
        print(f'    {q:10.3g}  err {err:.3e}  bound {lim:.3e}  {pname}')
    assert not bad, [(pname, err, lim) for _, err, lim, pname in bad]


def check_cycle_state(use, name):
    """grads_only runs no optimizer step; the running statistics after the cycle are those of the two sequential steps"""
    res = accumulation(use, name)
    assert res['outs'] == (2, 4)
    p_after, p_before, t = res['grads_only']
    assert bits_equal(p_after, p_before) and t == 0.0
    for a, b in zip(res['stats'], res['stats_ref']):
        assert bits_equal(a, b)


def check_mean_and_repeat(use, name):
    """with lr > 0 AdamW sees the MEAN of the two micro-batches: m == (1 - beta1) * fl(acc * 0.5) bit for bit; a repeat from
    the same state gives the same parameter bits"""
    res = accumulation(use, name)
    first, repeat, acc, live = res['first'], res['repeat'], res['acc'], res['live']
    assert bits_equal(first['g'], acc) and bits_equal(repeat['g'], acc)
    one, b1f = torch.tensor(1.0, dtype=torch.float32), torch.tensor(0.9, dtype=torch.float32)
    m_ref = b1f * 0.0 + (one - b1f) * (acc * 0.5)
    assert bits_equal(first['m'][live], m_ref[live]) and float(first['m'][~live].abs().max()) == 0.0
    assert first['t'] == 1.0 and not bits_equal(first['p'], res['grads_only'][1])
    assert bits_equal(first['p'], repeat['p']) and bits_equal(first['m'], repeat['m'])


CHECKS = dict(gradient_bound=check_gradient_bound, cycle_state=check_cycle_state, mean_and_repeat=check_mean_and_repeat)


@pytest.mark.parametrize('check', list(CHECKS))
def test_accumulation_emul(backend, check):
    CHECKS[check](backend, 'emul')


@pytest.mark.gpu
@pytest.mark.parametrize('check', list(CHECKS))
def test_accumulation_gpu(backend, check):
    CHECKS[check](backend, 'hip')


@pytest.mark.gpu
def test_capture_accumulated_gpu(backend):
    """capture_accumulated, k = 2, clipping on: two replays == two eager step_accumulated calls from the same state, bit for bit
    (parameters, m, v, step count, clip, running statistics); later replays follow set_max_norm and set_lr."""
    from hrfuser_amd.trainer import Trainer
    dev = backend('hip')
    L = _lib.lib()
    try:
        net, cfg = fresh_net(dev)
        b1, b2 = batch(dev, cfg, 1), batch(dev, cfg, 2)
        eng = net._engine()
        tr = Trainer(net, lr=1e-3, deterministic=True, max_norm=1.0)
        tr.step_accumulated([b1, b2], grads_only=True)               # (allocations, engine setup)
        torch.cuda.synchronize()
        norm = host_norm(eng.flat_g, tr.wd_mask) * 0.5
        tr.set_max_norm(0.5 * norm)
        tensors = lambda: (eng.flat_p, eng.rstat, eng.nbt_flat, tr.m, tr.v, tr.state, tr.clip)
        keep = [t.clone() for t in tensors()]

        def restore():
            for t, k in zip(tensors(), keep):
                t.copy_(k)

        def snap():
            torch.cuda.synchronize()
            return [t.clone() for t in tensors()]
        for _ in range(2):
            tr.step_accumulated([b1, b2])
        eager = snap()
        assert ulps(tr.grad_norm(), f32(host_norm(eng.flat_g, tr.wd_mask) * 0.5)) <= 1 and float(tr.state[2]) == 2.0
        assert not bits_equal(eager[0], keep[0])
        restore()
        tr.capture_accumulated([b1, b2], warmup=1)
        restore()
        for _ in range(2):
            tr.replay()
        replayed = snap()
        for i, (a, b) in enumerate(zip(eager, replayed)):
            assert bits_equal(a, b), f'tensor {i} differs between two eager cycles and two replays'
        assert len(tr._graph_outs) == 2 and 0.3 < tr.clip_coef() < 1.0
        # the captured graph reads max_norm and the learning rate from the device
        tr.set_max_norm(0.01 * norm)
        tr.replay()
        torch.cuda.synchronize()
        assert tr.clip_coef() < 0.02
        tr.set_max_norm(None)
        tr.set_lr(0.0)
        before = eng.flat_p.clone()
        tr.replay()
        torch.cuda.synchronize()
        assert tr.clip_coef() == 1.0 and bits_equal(eng.flat_p, before) and float(tr.state[2]) == 4.0
    finally:
        L.hrf_set_deterministic(0)


WORKER = r'''
import os, sys, torch
ROOT = %r
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29661', RANK='0', WORLD_SIZE='1', HRF_FORCE_COLLECTIVES='1')
import torch.distributed as dist
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)
dist.init_process_group('nccl', device_id=dev)                 # 'nccl' is RCCL on ROCm
from helpers import use_backend
from test_grad_clip import batch, fresh_net
from hrfuser_amd.trainer import Trainer
use_backend('hip')
net, cfg = fresh_net(dev, 't_nus')                              # norm_cfg type SyncBN
assert cfg['norm_cfg']['type'] == 'SyncBN'
b1, b2 = batch(dev, cfg, 1), batch(dev, cfg, 2)
tr = Trainer(net, lr=0.0, weight_decay=0.0, group=dist.group.WORLD, world_size=1, max_norm=1.0)
assert tr.force
tr.step(*b1)
torch.cuda.synchronize()
nb = len(tr.buckets(net._engine().flat_g.numel()))
one_grad, one_all = tr.grad_collectives_per_step, tr.collectives_per_step
tr.step_accumulated([b1, b2])
torch.cuda.synchronize()
two_grad, two_all = tr.grad_collectives_per_step, tr.collectives_per_step
assert one_grad == nb and two_grad == nb, (one_grad, two_grad, nb)             # the gradient exchange: once per cycle, not k times
assert one_all > one_grad and two_all - two_grad == 2 * (one_all - one_grad), (one_all, two_all)   # SyncBN: in every micro-batch
assert bool(torch.isfinite(net._engine().flat_g).all()) and tr.grad_norm() > 0
print('ACCUM_COLLECTIVES_OK', one_grad, one_all, two_grad, two_all)
sys.stdout.flush()
dist.barrier()
os._exit(0)
'''


@pytest.mark.gpu
def test_accumulation_exchanges_once_per_cycle_gpu():
    """A forced one-rank group (HRF_FORCE_COLLECTIVES=1, default mode; modelled on tests/test_syncbn_gpu.py): step_accumulated
    issues the gradient-bucket collectives once per cycle, the SyncBN exchanges in every micro-batch."""
    r = subprocess.run([sys.executable, '-c', WORKER % ROOT], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout[-2000:])
    assert 'ACCUM_COLLECTIVES_OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
