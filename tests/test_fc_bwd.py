"""The backward kernels of the bbox head's linear layers (csrc/hrf_fc_bwd.h: hrf_fc_bwd_data / hrf_fc_bwd_weight) through the C ABI
on the CPU emulator and on the GPU, against fp64 torch.

Bound.  relmax <= 2e-5 for dX, dW and db - test_bbox_head.BOUND, the bound of hrf_fc - valid because torch's own fp32 CPU matmul on
the same inputs stays under a quarter of it (test_bound_holds; measured: dW ~3e-7, dX ~5e-7, db ~1.4e-7 at K = 12544, N = 1024).

Inputs.  x >= 0 (a post-ReLU activation), the last quarter of the dy rows zero (as padding rows are), the mask a post-ReLU map
(about half of it zero).  Every input is pitched with NaN in its pad columns, every output sits in a larger buffer whose other
elements (a row before, a row after, the pad columns) must keep their fill, and each case runs twice: the two results are
torch.equal.  At the large shapes the fp64 reference is taken on the first and last row / column of every 128-wide tile plus 48
random ones."""
import functools

import pytest
import torch

from helpers import relmax, use_backend
from hrfuser_amd import _lib

BOUND = 2e-5
EMUL_SHAPES = [(1, 784, 64), (127, 3136, 80), (130, 784, 80), (130, 784, 16), (300, 16, 80)]
GPU_SHAPES = [(1, 12544, 1024), (130, 12544, 1024), (1024, 12544, 1024), (1024, 1024, 16)]
FILL = 777.0


def _subset(n, g):
    if n <= 512:
        return torch.arange(n)
    idx = [r for t in range(0, n, 128) for r in (t, min(t + 127, n - 1))] + torch.randint(0, n, (48,), generator=g).tolist()
    return torch.tensor(sorted(set(idx)))


@functools.lru_cache(None)
def _problem(M, K, N):
    """-> dict: x (M,K) >= 0, dy (M,N), w (N,K), mask (M,K) >= 0, the checked index sets and the fp64 references on them"""
    g = torch.Generator().manual_seed(2000 + M + K + N)
    x = torch.randn(M, K, generator=g).clamp_(min=0)
    dy = torch.randn(M, N, generator=g)
    dy[M - M // 4:] = 0
    w = torch.randn(N, K, generator=g) / N ** 0.5
    mask = torch.randn(M, K, generator=g).clamp_(min=0)
    rm, rk, rn = _subset(M, g), _subset(K, g), _subset(N, g)
    p = dict(x=x, dy=dy, w=w, mask=mask, rm=rm, rk=rk, rn=rn)
    for dt, tag in ((torch.float64, 'ref'), (torch.float32, 'f32')):
        xd, dd, wd = x.to(dt), dy.to(dt), w.to(dt)
        p[tag] = dict(dx_rows=dd[rm] @ wd, dx_cols=dd @ wd[:, rk], dw_rows=dd[:, rn].t() @ xd, dw_cols=dd.t() @ xd[:, rk], db=dd.sum(0))
    return p


def _pitched(t, pad, dev):
    """t (R, C) -> a (R, C) view of a (R, C + pad) device buffer with NaN in the pad columns"""
    big = torch.full((t.shape[0], t.shape[1] + pad), float('nan'))
    big[:, :t.shape[1]] = t
    return big.to(dev)[:, :t.shape[1]]


def _guarded(R, C, pad, dev, fill=FILL):
    """-> (buffer (R + 2, C + pad) of `fill`, its (R, C) view one row in)"""
    big = torch.full((R + 2, C + pad), fill, device=dev)
    return big, big[1:R + 1, :C]


def _guards_ok(big, R, C, fill=FILL):
    b = big.cpu()
    return bool((b[0] == fill).all() and (b[R + 1] == fill).all() and (b[:, C:] == fill).all())


def _ld(t):
    return t.stride(0)


def _ws(L, M, K, N, dev):
    need = L.hrf_fc_bwd_workspace_bytes(M, K, N)
    return (torch.empty((need,), device=dev, dtype=torch.uint8) if need > 0 else None), need


def _run_data(backend, M, K, N, masked):
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    p = _problem(M, K, N)
    dy, w = _pitched(p['dy'], 8, dev), _pitched(p['w'], 4, dev)
    mask = _pitched(p['mask'], 12, dev) if masked else None
    ws, need = _ws(L, M, K, N, dev)
    outs = []
    for _ in range(2):
        big, dx = _guarded(M, K, 4, dev)
        L.hrf_fc_bwd_data(dy, _ld(dy), w, _ld(w), mask, _ld(mask) if masked else 0, dx, _ld(dx), M, K, N, ws, need, s)
        assert _guards_ok(big, M, K)
        outs.append(dx.cpu())
    assert torch.equal(outs[0], outs[1])                           # bit-reproducible from run to run
    got = outs[0]
    rows, cols = p['ref']['dx_rows'], p['ref']['dx_cols']
    if masked:
        rows = torch.where(p['mask'][p['rm']] <= 0, torch.zeros_like(rows), rows)
        cols = torch.where(p['mask'][:, p['rk']] <= 0, torch.zeros_like(cols), cols)
        assert not bool(got[p['mask'] <= 0].any())                 # exactly zero where masked
    e1, e2 = relmax(got[p['rm']], rows), relmax(got[:, p['rk']], cols)
    print(f'hrf_fc_bwd_data {backend} M={M} K={K} N={N} mask={masked}: relmax rows {e1:.3e} cols {e2:.3e}')
    assert max(e1, e2) <= BOUND, (e1, e2)


def _run_weight(backend, M, K, N, accumulate, with_db=True):
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    p = _problem(M, K, N)
    dy, x = _pitched(p['dy'], 8, dev), _pitched(p['x'], 4, dev)
    ws, need = _ws(L, M, K, N, dev)
    fill = 0.25 if accumulate else FILL                            # the prefilled value the gradient is added to
    outs = []
    for _ in range(2):
        big, dw = _guarded(N, K, 4, dev, fill)
        bigb = torch.full((3, N), fill, device=dev)
        L.hrf_fc_bwd_weight(x, _ld(x), dy, _ld(dy), dw, _ld(dw), bigb[1] if with_db else None, accumulate, M, K, N, ws, need, s)
        assert _guards_ok(big, N, K, fill)
        bb = bigb.cpu()
        assert bool((bb[0] == fill).all() and (bb[2] == fill).all())
        if not with_db:
            assert bool((bb[1] == fill).all())
        outs.append((dw.cpu(), bb[1]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dw, db = outs[0]
    base = fill if accumulate else 0.0
    e1, e2 = relmax(dw[p['rn']], p['ref']['dw_rows'] + base), relmax(dw[:, p['rk']], p['ref']['dw_cols'] + base)
    e3 = relmax(db, p['ref']['db'] + base) if with_db else 0.0
    print(f'hrf_fc_bwd_weight {backend} M={M} K={K} N={N} accumulate={accumulate}: relmax dw rows {e1:.3e} cols {e2:.3e} db {e3:.3e}')
    assert max(e1, e2, e3) <= BOUND, (e1, e2, e3)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('M,K,N', EMUL_SHAPES)
def test_data_emul(M, K, N, masked):
    _run_data('emul', M, K, N, masked)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('M,K,N', EMUL_SHAPES)
def test_weight_emul(M, K, N, accumulate):
    _run_weight('emul', M, K, N, accumulate)


def test_weight_no_bias_emul():
    _run_weight('emul', 130, 784, 80, 0, with_db=False)


def test_splits_emul():
    """the workspace query tells a split weight gradient (slots of N x K floats) from an unsplit one; both ran above.  A split DATA
    gradient needs a reduction of 512: (1, 16, 512) runs here"""
    L = (use_backend('emul'), _lib.lib())[1]
    assert L.hrf_fc_bwd_workspace_bytes(1, 784, 64) == 0                          # one 16-row step: nothing to split
    for M, K, N in EMUL_SHAPES[1:]:
        need = L.hrf_fc_bwd_workspace_bytes(M, K, N)
        assert need >= 2 * N * K * 4 and need % (N * K * 4) == 0, (M, K, N, need)
    assert L.hrf_fc_bwd_workspace_bytes(300, 16, 80) == 4 * 80 * 16 * 4
    assert L.hrf_fc_bwd_workspace_bytes(1, 16, 512) == 2 * 1 * 16 * 4             # the data gradient's two slots of M x K
    assert L.hrf_fc_bwd_workspace_bytes(130, 780, 80) == 0 and L.hrf_fc_bwd_workspace_bytes(0, 784, 80) == 0
    _run_data('emul', 1, 16, 512, True)
    # the split is a function of the shape alone: the same query twice
    assert L.hrf_fc_bwd_workspace_bytes(130, 784, 80) == L.hrf_fc_bwd_workspace_bytes(130, 784, 80)


def _mask_semantics(backend):
    """a select, not a multiply: Inf / NaN sums are +0 where masked and non-finite elsewhere; a NaN in the mask lets the gradient through"""
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    M, K, N = 5, 32, 16
    g = torch.Generator().manual_seed(5)
    dy, w = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g)
    dy[1, 3] = float('inf')                                         # row 1: every sum is +-Inf
    dy[2, 0], dy[2, 1] = float('inf'), float('-inf')                # row 2: every sum is NaN or +-Inf
    mask = torch.ones(M, K)
    mask[:, ::2] = 0.0
    mask[:, 1] = -1.0
    mask[3, 4] = float('nan')                                       # (an even column: masked in the other rows)
    mask[4, 5] = -0.0
    dx = torch.full((M, K), FILL, device=dev)
    L.hrf_fc_bwd_data(dy.to(dev), N, w.to(dev), K, mask.to(dev), K, dx, K, M, K, N, None, 0, s)
    dx = dx.cpu()
    off = mask <= 0
    assert bool((dx[off] == 0).all()) and not bool(torch.signbit(dx[off]).any())
    assert not bool(dx[1:3][~off[1:3]].isfinite().any())
    want = dy.double() @ w.double()
    assert abs(float(dx[3, 4]) - float(want[3, 4])) <= BOUND * float(want[3].abs().max())
    fin = ~off
    fin[1:3] = False
    assert relmax(dx[fin], want[fin]) <= BOUND


def test_mask_semantics_emul():
    _mask_semantics('emul')


@pytest.mark.gpu
def test_mask_semantics_gpu():
    _mask_semantics('hip')


def _zero_rows(backend):
    """M = 0: a no-op, except that accumulate = 0 defines dw / db: zeros"""
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    K, N = 32, 16
    x, dy = torch.zeros(1, K, device=dev), torch.zeros(1, N, device=dev)
    for acc in (0, 1):
        big, dw = _guarded(N, K, 4, dev)
        db = torch.full((N,), FILL, device=dev)
        L.hrf_fc_bwd_weight(x, K, dy, N, dw, _ld(dw), db, acc, 0, K, N, None, 0, s)
        assert _guards_ok(big, N, K)
        want = FILL if acc else 0.0
        assert bool((dw.cpu() == want).all()) and bool((db.cpu() == want).all())
    dx = torch.full((1, K), FILL, device=dev)
    L.hrf_fc_bwd_data(dy, N, torch.zeros(N, K, device=dev), K, None, 0, dx, K, 0, K, N, None, 0, s)
    assert bool((dx.cpu() == FILL).all())


def test_zero_rows_emul():
    _zero_rows('emul')


@pytest.mark.gpu
def test_zero_rows_gpu():
    _zero_rows('hip')


@pytest.mark.gpu
@pytest.mark.parametrize('M,K,N', EMUL_SHAPES + GPU_SHAPES)
def test_data_gpu(M, K, N):
    _run_data('hip', M, K, N, True)


@pytest.mark.gpu
@pytest.mark.parametrize('M,K,N', EMUL_SHAPES + GPU_SHAPES)
def test_weight_gpu(M, K, N):
    _run_weight('hip', M, K, N, 1 if M == 130 else 0)


@pytest.mark.gpu
def test_data_unmasked_gpu():
    _run_data('hip', 130, 12544, 1024, False)


def test_bound_holds():
    """the bound 2e-5 stands if torch's own fp32 CPU result stays under a quarter of it on the GPU tests' inputs"""
    for M, K, N in GPU_SHAPES:
        p = _problem(M, K, N)
        for k, ref in p['ref'].items():
            err = relmax(p['f32'][k], ref)
            print(f'fp32 CPU torch M={M} K={K} N={N} {k}: relmax {err:.3e}')
            assert err < BOUND / 4, (M, K, N, k, err)


def _refusals(backend):
    dev = use_backend(backend)
    L, s = _lib.lib(), _lib.stream_ptr()
    M, K, N = 4, 32, 16
    dy, w, mk, dx, x, dw, db = (torch.zeros(sh, device=dev) for sh in ((M, N), (N, K), (M, K), (M, K), (M, K), (N, K), (N,)))
    ws = torch.zeros(1 << 16, device=dev, dtype=torch.uint8)
    okd = (dy, N, w, K, mk, K, dx, K, M, K, N, ws, ws.numel(), s)
    okw = (x, K, dy, N, dw, K, db, 0, M, K, N, ws, ws.numel(), s)
    L.hrf_fc_bwd_data(*okd)
    L.hrf_fc_bwd_weight(*okw)
    L.hrf_fc_bwd_data(dy, N, w, K, None, 0, dx, K, M, K, N, None, 0, s)           # no mask, no workspace needed
    L.hrf_fc_bwd_weight(x, K, dy, N, dw, K, None, 1, M, K, N, None, 0, s)         # no db
    badd = {'K % 16': dict(i9=24), 'N % 16': dict(i10=8), 'null dy': dict(i0=None), 'null w': dict(i2=None), 'null dx': dict(i6=None),
            'ldDY < N': dict(i1=8), 'ldW < K': dict(i3=16), 'ldMask < K': dict(i5=16), 'ldDX < K': dict(i7=31), 'M < 0': dict(i8=-1)}
    badw = {'K % 16': dict(i9=24), 'N % 16': dict(i10=8), 'null x': dict(i0=None), 'null dy': dict(i2=None), 'null dw': dict(i4=None),
            'ldX < K': dict(i1=16), 'ldDY < N': dict(i3=8), 'ldDW < K': dict(i5=31), 'accumulate': dict(i7=2), 'accumulate < 0': dict(i7=-1),
            'M < 0': dict(i8=-1)}
    for fn, ok, bad in ((L.hrf_fc_bwd_data, okd, badd), (L.hrf_fc_bwd_weight, okw, badw)):
        for name, ch in bad.items():
            a = list(ok)
            for k, v in ch.items():
                a[int(k[1:])] = v
            with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
                fn(*a)
    # a split shape of each entry with a null / short workspace
    need = L.hrf_fc_bwd_workspace_bytes(300, 16, 80)
    assert need == 4 * 80 * 16 * 4
    xx, dd, ww = torch.zeros(300, 16, device=dev), torch.zeros(300, 80, device=dev), torch.zeros(80, 16, device=dev)
    for w_, n_ in ((None, 0), (None, need), (ws, need - 1)):
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_fc_bwd_weight(xx, 16, dd, 80, ww, 16, None, 0, 300, 16, 80, w_, n_, s)
    need = L.hrf_fc_bwd_workspace_bytes(1, 16, 512)
    assert need == 2 * 16 * 4
    d1, w1, x1 = torch.zeros(1, 512, device=dev), torch.zeros(512, 16, device=dev), torch.zeros(1, 16, device=dev)
    for w_, n_ in ((None, 0), (ws, need - 1)):
        with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
            L.hrf_fc_bwd_data(d1, 512, w1, 16, None, 0, x1, 16, 1, 16, 512, w_, n_, s)


def test_refusals_emul():
    _refusals('emul')


@pytest.mark.gpu
def test_refusals_gpu():
    _refusals('hip')
