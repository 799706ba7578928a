"""RPN training targets and loss (csrc/hrf_rpn_train.h: hrf_rpn_assign / hrf_rpn_loss; hrfuser_amd/rpn.py: rpn_assign, rpn_loss,
RPNHead.loss) against the literal torch restatement of anchor_inside_flags, bbox_overlaps, MaxIoUAssigner, the sampler given keys
and the two losses (hrfuser_amd.testing), through the C ABI on the CPU emulator and on the GPU.  mmdet is not installed: parity
against an installed mmdet is unpinned; the restatement is pinned against the reference's docstring example here.

Pyramid 128 x 192: (32,48), (16,24), (8,12), (4,6), (2,3), A = 3, B = 2: N = 6138 anchors per image (24 blocks of 256: level 0
alone spans 18, the coarse levels end in partial blocks).  Ground truths: sides log-uniform in 12..120 px, placed uniformly inside
the image.  Logits ~ N(0, 2^2), deltas ~ N(0, 0.3^2).  The committed seeds are the first of 0, 1, 2, ... whose inputs are
unambiguous (test_inputs_unambiguous): no inside-anchor / gt pair with an fp64 IoU within 1e-5 of a threshold, no anchor with two
gts at an equal positive maximum.

Bounds.  Assignment, max_iou and sampling are bit-defined (-ffp-contract=off, IEEE division): compared EXACTLY.  Losses and
gradients: the sample sets are identical and the gradients exactly zero off-sample; for the values the bound is measured per
group (the 2 L losses / the on-sample d_cls / the on-sample d_reg): 4 x max|fp32 restatement - fp64 restatement| (a different
summation order, a different expf / log1pf / logf) + one fp32 ulp of the group's largest fp64 magnitude.  A sign error, a wrong
avg, a wrong beta arm or a wrong level offset is orders of magnitude above it.  Measured max |x - fp64 restatement| (printed by
test_loss_*; the emulator and the MI355X gave the same figures to the digits shown):
  case              group    kernel     fp32 restatement   bound
  ref               losses   2.565e-08  2.565e-08          2.218e-07   (10 values, largest 1.057)
  ref               d_cls    1.486e-10  1.486e-10          7.106e-10   (512 values, largest 1.947e-03)
  ref               d_reg    3.018e-09  3.018e-09          1.230e-08   (316 values, largest 1.953e-03)
  crowded, pitched  losses   5.638e-08  6.283e-08          3.705e-07   (10 values, largest 1.078)
  crowded, pitched  d_cls    1.486e-10  1.486e-10          7.106e-10   (512 values)
  crowded, pitched  d_reg    5.935e-09  5.935e-09          2.397e-08   (612 values)"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from helpers import load_cfgs, use_backend
from hrfuser_amd import _lib
from hrfuser_amd.testing import (bbox_overlaps_ref, max_iou_assign_ref, rpn_assign_ref, rpn_base_anchors, rpn_bbox2delta_ref, rpn_delta2bbox,
                                 rpn_grid_anchors, rpn_inside_flags_ref, rpn_key_ref, rpn_loss_ref, rpn_sample_ref)

STRIDES = [4, 8, 16, 32, 64]
A, B = 3, 2
BASES = [rpn_base_anchors(s, [8], [0.5, 1.0, 2.0]) for s in STRIDES]
FULL = [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]
TINY = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
BETA = 1.0 / 9.0
CONFIG = dict(thr=(0.7, 0.3, 0.3), mlq=True, border=0)               # train_cfg.rpn of every reference config
CASES = {
    # name: sizes, image shapes (h, w), pad shapes, gts per image, thresholds (pos, neg, min_pos), match_low_quality, allowed_border, seed
    'ref': dict(sizes=FULL, shapes=[(128, 192), (120, 180)], pads=[(128, 192), (128, 192)], G=[6, 6], seed=0, **CONFIG),
    'padded': dict(sizes=FULL, shapes=[(128, 192), (90, 150)], pads=[(128, 192), (96, 160)], G=[6, 6], seed=0, **CONFIG),
    'crowded': dict(sizes=FULL, shapes=[(128, 192), (120, 180)], pads=[(128, 192), (128, 192)], G=[40, 6], seed=0, **CONFIG),
    'empty': dict(sizes=FULL, shapes=[(128, 192), (120, 180)], pads=[(128, 192), (128, 192)], G=[0, 3], seed=0, **CONFIG),
    'rcnn-like': dict(sizes=FULL, shapes=[(128, 192), (120, 180)], pads=[(128, 192), (128, 192)], G=[6, 6], seed=0, thr=(0.5, 0.5, 0.5),
                      mlq=False, border=0),
    'border': dict(sizes=FULL, shapes=[(128, 192), (120, 180)], pads=[(128, 192), (128, 192)], G=[6, 6], seed=0, thr=(0.7, 0.3, 0.3),
                   mlq=True, border=-1),
    'tiny': dict(sizes=TINY, shapes=[(64, 96), (60, 90)], pads=[(64, 96), (64, 96)], G=[6, 6], seed=0, **CONFIG),
}
NUM, NUM_POS = 256, 128                                               # sampler num, int(num * pos_fraction)


def _draw_gts(case, seed):
    """-> [gts (G_b, 4) fp32] per image: sides log-uniform 12..120 (at most the image), uniformly placed inside the image"""
    c = CASES[case]
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for (h, w), n in zip(c['shapes'], c['G']):
        u = torch.rand(n, 4, generator=g, dtype=torch.float64)
        bw = torch.exp(math.log(12.0) + u[:, 0] * (math.log(120.0) - math.log(12.0))).clamp(max=w)
        bh = torch.exp(math.log(12.0) + u[:, 1] * (math.log(120.0) - math.log(12.0))).clamp(max=h)
        x1, y1 = u[:, 2] * (w - bw), u[:, 3] * (h - bh)
        out.append(torch.stack([x1, y1, x1 + bw, y1 + bh], dim=1).float())
    return out


def _assign_of(case, seed):
    """the restatement's assignment of every image: [(assigned, max_iou, anchors, inside)]"""
    c = CASES[case]
    gts = _draw_gts(case, seed)
    return gts, [rpn_assign_ref(c['sizes'], STRIDES, BASES, c['shapes'][b], c['pads'][b], gts[b], *c['thr'], c['mlq'], c['border']) for b in range(B)]


def _unambiguous(case, seed):
    c = CASES[case]
    gts, asg = _assign_of(case, seed)
    for b in range(B):
        if gts[b].shape[0] == 0:
            continue
        _, _, anchors, inside = asg[b]
        o32 = bbox_overlaps_ref(gts[b], anchors[inside])
        o64 = bbox_overlaps_ref(gts[b].double(), anchors[inside].double())
        for t in set(c['thr']):
            if bool(((o64 - t).abs() < 1e-5).any()):
                return False
        mx = o32.max(dim=0)[0]
        if bool((((o32 == mx[None, :]).sum(dim=0) > 1) & (mx > 0)).any()):
            return False
    return True


@functools.lru_cache(None)
def _ref(case):
    """-> dict(gts, assigned [b], max_iou [b], anchors, inside [b], cs, bp): computed once, never modified"""
    c = CASES[case]
    gts, asg = _assign_of(case, c['seed'])
    g = torch.Generator().manual_seed(77)
    cs = [2.0 * torch.randn(B, A, h, w, generator=g) for h, w in c['sizes']]
    bp = [0.3 * torch.randn(B, 4 * A, h, w, generator=g) for h, w in c['sizes']]
    return dict(gts=gts, assigned=[a[0] for a in asg], max_iou=[a[1] for a in asg], anchors=asg[0][2], inside=[a[3] for a in asg], cs=cs, bp=bp)


def _n_anchors(case):
    return sum(h * w * A for h, w in CASES[case]['sizes'])


def _keys(case, kind):
    """(B, N) int64 uint32 values: 'random' or 'equal'"""
    N = _n_anchors(case)
    if kind == 'equal':
        return torch.full((B, N), 12345, dtype=torch.long)
    return torch.randint(0, 1 << 32, (B, N), generator=torch.Generator().manual_seed(5), dtype=torch.long)


def _as_i32(k):
    """uint32 values in int64 -> the same bits as int32"""
    return torch.where(k >= (1 << 31), k - (1 << 32), k).to(torch.int32)


def _nhwc(case, dev, pitch=False):
    """the maps as the kernels take them: (B,H,W,C) views; pitch: rows of C + 5 / C + 3 floats, NaN in the padding"""
    r = _ref(case)
    out = []
    for maps, extra in ((r['cs'], 5), (r['bp'], 3)):
        lst = []
        for m in maps:
            t = m.permute(0, 2, 3, 1).contiguous()
            if pitch:
                big = torch.full(t.shape[:3] + (t.shape[3] + extra,), float('nan'))
                big[..., :t.shape[3]] = t
                t = big.to(dev)[..., :t.shape[3]]
            lst.append(t.to(dev))
        out.append(lst)
    return out


def _cfg(case, num=NUM, num_pos=NUM_POS):
    from hrfuser_amd import rpn
    c = CASES[case]
    return rpn.train_cfg_struct(*c['thr'], c['mlq'], c['border'], num, num_pos, BETA, 1.0, 1.0)


def _call(fn, case, dev, pitch=False, keys=None, rng=None, num=NUM, num_pos=NUM_POS, gts=None, gmax=None, maps=None):
    from hrfuser_amd import rpn
    c = CASES[case]
    cm, rm = _nhwc(case, dev, pitch) if maps is None else maps
    gt, cnt = rpn.pack_gts(_ref(case)['gts'] if gts is None else gts, dev, gmax)
    return fn(cm, rm, c['shapes'], c['pads'], gt, cnt, STRIDES, [b.tolist() for b in BASES], _cfg(case, num, num_pos),
              keys=None if keys is None else _as_i32(keys).to(dev), rng=rng)


# ----------------------------------------------------------------------------- 1. the restatement, pinned on the CPU
def test_restatement_assigner_docstring():
    """max_iou_assigner.py:87-92: MaxIoUAssigner(0.5, 0.5) on two boxes and one gt -> gt_inds [1, 0]"""
    bboxes = torch.tensor([[0., 0., 10., 10.], [10., 10., 20., 20.]])
    gt = torch.tensor([[0., 0., 10., 9.]])
    o = bbox_overlaps_ref(gt, bboxes)
    assert o.shape == (1, 2) and abs(float(o[0, 0]) - 0.9) < 1e-6 and float(o[0, 1]) == 0.0
    assigned, mx = max_iou_assign_ref(o, 0.5, 0.5)
    assert assigned.tolist() == [1, 0] and torch.equal(mx, o[0])
    # no gts: everything background; low-quality matching: later gts overwrite earlier ones, equality takes every best anchor
    assert max_iou_assign_ref(torch.zeros(0, 3), 0.5, 0.5)[0].tolist() == [0, 0, 0]
    o = torch.tensor([[0.4, 0.4, 0.1, 0.0], [0.4, 0.2, 0.1, 0.6]])
    assert max_iou_assign_ref(o, 0.7, 0.3, 0.3, True)[0].tolist() == [1, 1, 0, 2]
    assert max_iou_assign_ref(o, 0.7, 0.3, 0.3, False)[0].tolist() == [-1, -1, 0, -1]
    assert max_iou_assign_ref(o, 0.5, 0.3, 0.5, True)[0].tolist() == [-1, -1, 0, 2]       # gt 0's best (0.4) is below min_pos_iou


def test_restatement_bbox2delta_round_trip():
    """bbox2delta through the already pinned rpn_delta2bbox gives the gt back"""
    g = torch.Generator().manual_seed(2)
    p = torch.rand(64, 2, generator=g) * 100
    anchors = torch.cat([p, p + 8 + torch.rand(64, 2, generator=g) * 60], dim=1)
    q = torch.rand(64, 2, generator=g) * 100
    gts = torch.cat([q, q + 8 + torch.rand(64, 2, generator=g) * 60], dim=1)
    back = rpn_delta2bbox(anchors, rpn_bbox2delta_ref(anchors, gts))
    assert float((back - gts).abs().max()) < 1e-3
    d = rpn_bbox2delta_ref(torch.tensor([[0., 0., 10., 20.]]), torch.tensor([[5., 0., 15., 20.]]))
    assert torch.equal(d, torch.tensor([[0.5, 0., 0., 0.]]))


def test_restatement_inside_flags():
    """anchor_inside_flags: x1 == -border is inside, x2 == img_w + border is outside; border < 0: the valid flags alone; the valid
    flags cut at ceil(pad / stride)"""
    H, W, s = 2, 3, 16
    base = torch.tensor([[0., 0., 16., 16.]])                        # anchors (16 x, 16 y, 16 x + 16, 16 y + 16)
    an = rpn_grid_anchors(base, H, W, s)
    f = rpn_inside_flags_ref(an, H, W, 1, s, (32, 48), (32, 48), 0)
    assert f.tolist() == [True, True, False, False, False, False]   # x2 == 48 == img_w and y2 == 32 == img_h are outside
    assert rpn_inside_flags_ref(an, H, W, 1, s, (33, 49), (32, 48), 0).all()
    assert rpn_inside_flags_ref(an, H, W, 1, s, (32, 48), (32, 48), 1).all()            # x2 < 48 + 1
    assert rpn_inside_flags_ref(an, H, W, 1, s, (1, 1), (32, 48), -1).all()             # border < 0: valid alone
    assert rpn_inside_flags_ref(an, H, W, 1, s, (99, 99), (17, 33), -1).all()           # ceil(17 / 16) = 2 rows, ceil(33 / 16) = 3 columns
    assert rpn_inside_flags_ref(an, H, W, 1, s, (99, 99), (16, 32), -1).tolist() == [True, True, False, False, False, False]
    shifted = rpn_grid_anchors(torch.tensor([[-4., -4., 12., 12.]]), 1, 1, s)
    assert not rpn_inside_flags_ref(shifted, 1, 1, 1, s, (32, 48), (32, 48), 3).any()   # x1 = -4 < -3
    assert rpn_inside_flags_ref(shifted, 1, 1, 1, s, (32, 48), (32, 48), 4).all()       # x1 = -4 >= -4


def test_restatement_key_hash():
    """rpn_key_ref against the hash computed with Python integers"""
    M = 0xffffffff

    def mix(h):
        h ^= h >> 16
        h = (h * 0x7feb352d) & M
        h ^= h >> 15
        h = (h * 0x846ca68b) & M
        return h ^ (h >> 16)
    for seed, counter, b in ((0, 0, 0), (7, 1, 1), (0xfffffff0, 0xffffffff, 3)):
        got = rpn_key_ref(seed, counter, b, 300)
        want = [mix(mix(((mix(mix((seed + 0x9e3779b9) & M) ^ counter)) + b) & M) ^ n) for n in range(300)]
        assert got.tolist() == want
    assert rpn_key_ref(7, 0, 0, 4096).unique().numel() > 4090


# ----------------------------------------------------------------------------- 2. / 3. the inputs: unambiguous, every arm reached
@pytest.mark.parametrize('case', sorted(CASES))
def test_inputs_unambiguous(case):
    """the committed seed is the first of 0, 1, 2, ... whose inputs are unambiguous"""
    seed = CASES[case]['seed']
    first = next(s for s in range(seed + 1) if _unambiguous(case, s))
    assert first == seed, (case, first)


def test_arms_are_reached():
    """the restatement alone: bit-equal best anchors, low-quality reassignment away from the argmax, both sides of the positive
    cap, more negatives than wanted everywhere but in `tiny`"""
    ties = moved = 0
    for case in ('ref', 'crowded'):
        r = _ref(case)
        for b in range(B):
            inside = r['inside'][b]
            o = bbox_overlaps_ref(r['gts'][b], r['anchors'][inside])
            ties += int(((o == o.max(dim=1, keepdim=True)[0]).sum(dim=1) > 1).sum())
            arg = o.max(dim=0)[1] + 1
            a = r['assigned'][b][inside]
            moved += int(((a > 0) & (a != arg)).sum())               # matched to a gt that is not its argmax: only the low-quality loop does that
    print(f'gts with more than one bit-equal best anchor: {ties}; anchors reassigned away from their argmax: {moved}')
    assert ties >= 1 and moved >= 1
    pos = [int((a > 0).sum()) for a in _ref('crowded')['assigned']]
    print('crowded: assigned positives per image', pos)
    assert max(pos) > NUM_POS > min(pos)
    for case in CASES:
        for b, a in enumerate(_ref(case)['assigned']):
            P, Q = int((a > 0).sum()), int((a == 0).sum())
            want = NUM - min(P, NUM_POS)
            print(f'{case} image {b}: {int((a > -2).sum())} inside, {P} positives, {Q} negatives')
            assert (Q < want) if case == 'tiny' else (Q > want), (case, b, P, Q)
    assert int(_ref('tiny')['inside'][0].sum()) == 369


# ----------------------------------------------------------------------------- 4. the assignment is exact
def _assign(backend, case, pitch=False):
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    r = _ref(case)
    assigned, max_iou, sampled, counts = (t.cpu() for t in _call(rpn.rpn_assign, case, dev, pitch, keys=_keys(case, 'random')))
    for b in range(B):
        assert torch.equal(assigned[b].long(), r['assigned'][b]), (b, int((assigned[b].long() != r['assigned'][b]).sum()))
        assert torch.equal(max_iou[b].view(torch.int32), r['max_iou'][b].view(torch.int32)), b
        assert counts[b, :2].tolist() == [int((r['assigned'][b] > 0).sum()), int((r['assigned'][b] == 0).sum())], b
    print(f'rpn assign {backend} {case} pitch={pitch}: counts {counts.tolist()}')


ASSIGN_CASES = [('ref', False), ('ref', True), ('padded', False), ('crowded', False), ('empty', False), ('rcnn-like', False), ('border', False)]


@pytest.mark.parametrize('case,pitch', ASSIGN_CASES)
def test_assign_emul(case, pitch):
    _assign('emul', case, pitch)


@pytest.mark.gpu
@pytest.mark.parametrize('case,pitch', ASSIGN_CASES)
def test_assign_gpu(case, pitch):
    _assign('hip', case, pitch)


# ----------------------------------------------------------------------------- 5. the sampling is exact given keys
def _check_sampling(case, sampled, counts, keys, num, num_pos):
    r = _ref(case)
    for b in range(B):
        want = rpn_sample_ref(r['assigned'][b], keys[b], num, num_pos)
        assert torch.equal(sampled[b].long(), want), (case, b, int((sampled[b].long() != want).sum()))
        a = r['assigned'][b]
        assert counts[b].tolist() == [int((a > 0).sum()), int((a == 0).sum()), int((want > 0).sum()), int((want < 0).sum())], (case, b)


def _sampling(backend, variant):
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    case, kind, num, num_pos = {'random': ('ref', 'random', NUM, NUM_POS), 'equal': ('ref', 'equal', NUM, NUM_POS),
                                'crowded': ('crowded', 'random', NUM, NUM_POS), 'tiny': ('tiny', 'random', NUM, NUM_POS),
                                'num32': ('crowded', 'random', 32, 16), 'generated': ('ref', None, NUM, NUM_POS)}[variant]
    N = _n_anchors(case)
    if kind is not None:
        keys = _keys(case, kind)
        _, _, sampled, counts = (t.cpu() for t in _call(rpn.rpn_assign, case, dev, keys=keys, num=num, num_pos=num_pos))
        _check_sampling(case, sampled, counts, keys, num, num_pos)
        if variant == 'equal':                                       # all keys equal: the lowest indices win
            for b in range(B):
                pos = torch.nonzero(_ref(case)['assigned'][b] > 0)[:, 0]
                assert torch.equal(torch.nonzero(sampled[b] > 0)[:, 0], pos[:min(pos.numel(), num_pos)])
        if variant == 'tiny':                                        # fewer negatives than wanted: all are taken
            for b in range(B):
                assert torch.equal(sampled[b] < 0, _ref(case)['assigned'][b] == 0)
        print(f'rpn sampling {backend} {variant}: counts {counts.tolist()}')
        return
    sets = []
    for counter in (41, 42):                                         # generated keys, two consecutive counters
        st = rpn.rng_state(0x9abcdef0, counter, dev)
        _, _, sampled, counts = (t.cpu() for t in _call(rpn.rpn_assign, case, dev, rng=st))
        assert st.cpu().tolist() == rpn.rng_state(0x9abcdef0, counter).tolist()      # hrf_rpn_assign does not advance the counter
        keys = torch.stack([rpn_key_ref(0x9abcdef0, counter, b, N) for b in range(B)])
        _check_sampling(case, sampled, counts, keys, num, num_pos)
        sets.append(sampled)
    assert not torch.equal(sets[0], sets[1])


SAMPLING = ['random', 'equal', 'crowded', 'tiny', 'num32', 'generated']


@pytest.mark.parametrize('variant', SAMPLING)
def test_sampling_emul(variant):
    _sampling('emul', variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', SAMPLING)
def test_sampling_gpu(variant):
    _sampling('hip', variant)


# ----------------------------------------------------------------------------- 6. loss and gradients
def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@functools.lru_cache(None)
def _loss_ref(case):
    """-> (sampled [b], fp32 restatement, fp64 restatement) with the 'random' keys: computed once"""
    r = _ref(case)
    keys = _keys(case, 'random')
    sampled = [rpn_sample_ref(r['assigned'][b], keys[b], NUM, NUM_POS) for b in range(B)]
    args = (r['cs'], r['bp'], r['anchors'], r['assigned'], sampled, r['gts'], BETA, 1.0, 1.0)
    return sampled, rpn_loss_ref(*args, dtype=torch.float32), rpn_loss_ref(*args, dtype=torch.float64)


def _loss(backend, case, pitch):
    """Measured (emulator and MI355X alike), max |kernel - fp64 restatement| / max |fp32 restatement - fp64 restatement| / bound:
    ref: losses 2.565e-08 / 2.565e-08 / 2.218e-07, d_cls 1.486e-10 / 1.486e-10 / 7.106e-10, d_reg 3.018e-09 / 3.018e-09 / 1.230e-08;
    crowded, pitched: losses 5.638e-08 / 6.283e-08 / 3.705e-07, d_cls 1.486e-10 / 1.486e-10 / 7.106e-10, d_reg 5.935e-09 / 5.935e-09 /
    2.397e-08."""
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    sampled_ref, r32, r64 = _loss_ref(case)
    assert r64[4][0] > 0 and r64[4][1] > 0, r64[4]                   # both SmoothL1 arms occur on the sampled positives
    keys = _keys(case, 'random')
    losses, grads, assigned, _, sampled, counts = (t if isinstance(t, list) else t.cpu() for t in _call(rpn.rpn_loss, case, dev, pitch, keys=keys))
    grads = [g.cpu() for g in grads]
    _check_sampling(case, sampled, counts, keys, NUM, NUM_POS)
    L = len(grads)
    # the three groups: (kernel values, fp32 restatement, fp64 restatement) as flat tensors
    off, on_c, on_r = 0, [], []
    groups = {'losses': (losses.reshape(-1).double(), torch.stack(r32[0] + r32[1]).double(), torch.stack(r64[0] + r64[1]))}
    kc, kr, c32, c64, b32, b64 = [], [], [], [], [], []
    for l, g in enumerate(grads):
        n = g.shape[1] * g.shape[2] * A
        smp = torch.stack([s[off:off + n] for s in sampled_ref])    # (B, n)
        dc, dr = g[..., :A].reshape(B, n), g[..., A:5 * A].reshape(B, n, 4)
        assert not bool(g[..., 5 * A:].any())
        assert not bool(dc[smp == 0].any()) and not bool(dr[smp <= 0].any()), l                    # exactly zero off-sample
        kc.append(dc[smp != 0].double())
        kr.append(dr[smp > 0].reshape(-1).double())
        for src, dst_c, dst_b in ((r32, c32, b32), (r64, c64, b64)):
            gc = src[2][l].permute(0, 2, 3, 1).reshape(B, n)
            gb = src[3][l].permute(0, 2, 3, 1).reshape(B, n, 4)
            assert not bool(gc[smp == 0].any()) and not bool(gb[smp <= 0].any())
            dst_c.append(gc[smp != 0].double())
            dst_b.append(gb[smp > 0].reshape(-1).double())
        off += n
    groups['d_cls'] = (torch.cat(kc), torch.cat(c32), torch.cat(c64))
    groups['d_reg'] = (torch.cat(kr), torch.cat(b32), torch.cat(b64))
    for name, (k, a32, a64) in groups.items():
        e_ref, e = float((a32 - a64).abs().max()), float((k - a64).abs().max())
        bound = 4.0 * e_ref + _ulp32(float(a64.abs().max()))
        print(f'rpn loss {backend} {case} pitch={pitch} {name}: {k.numel()} values, max |value| {float(a64.abs().max()):.3e}, restatement fp32 vs '
              f'fp64 {e_ref:.3e}, kernel vs fp64 {e:.3e}, bound {bound:.3e}')
        assert k.numel() > 0 and e <= bound, (name, e, bound)
    assert float(groups['losses'][2].min()) >= 0 and float(groups['losses'][2][:2].min()) > 0       # the two finest levels hold samples


@pytest.mark.parametrize('case,pitch', [('ref', False), ('crowded', True)])
def test_loss_emul(case, pitch):
    _loss('emul', case, pitch)


@pytest.mark.gpu
@pytest.mark.parametrize('case,pitch', [('ref', False), ('crowded', True)])
def test_loss_gpu(case, pitch):
    _loss('hip', case, pitch)


# ----------------------------------------------------------------------------- 7. bit-reproducibility
def _flat(outs):
    return [t for o in outs for t in (o if isinstance(o, list) else [o])]


def _reproducible(backend):
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    runs = []
    for _ in range(2):
        st = rpn.rng_state(3, 9, dev)
        runs.append([t.cpu() for t in _flat(_call(rpn.rpn_loss, 'crowded', dev, rng=st))])
        assert st.cpu().tolist() == [3, 10]                          # hrf_rpn_loss advanced the counter
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    st = rpn.rng_state(3, 10, dev)
    other = _call(rpn.rpn_loss, 'crowded', dev, rng=st)
    assert not torch.equal(other[4].cpu(), runs[0][-2])              # the next counter draws another sample


def test_reproducible_emul():
    _reproducible('emul')


@pytest.mark.gpu
def test_reproducible_gpu():
    _reproducible('hip')


# ----------------------------------------------------------------------------- 8. hostile inputs
def _hostile(backend, count1):
    """image 1 is hostile (a gt_count outside [0, Gmax], NaN / Inf / inverted boxes, NaN logits), image 0 is the `ref` image: the
    call returns, counts stay in range, image 0's targets are those of the restatement"""
    from hrfuser_amd import rpn
    dev = use_backend(backend)
    r, c = _ref('ref'), CASES['ref']
    nan, inf = float('nan'), float('inf')
    bad = torch.tensor([[10., 10., 60., 50.], [nan, 5., 40., 40.], [0., 0., inf, inf], [80., 70., 30., 20.], [-inf, nan, inf, 3.],
                        [20., 30., 20., 30.]])
    cm, rm = _nhwc('ref', dev)
    cm = [m.clone() for m in cm]
    for m in cm:
        m[1].view(-1)[::7] = nan
    gt, cnt = rpn.pack_gts([r['gts'][0], bad], dev)
    cnt = torch.tensor([int(cnt[0]), count1], dtype=torch.int32).to(dev)
    keys = _keys('ref', 'random')
    losses, grads, assigned, max_iou, sampled, counts = rpn.rpn_loss(cm, rm, c['shapes'], c['pads'], gt, cnt, STRIDES, [b.tolist() for b in BASES],
                                                                     _cfg('ref'), keys=_as_i32(keys).to(dev))
    assigned, max_iou, sampled, counts = assigned.cpu(), max_iou.cpu(), sampled.cpu(), counts.cpu()
    N = _n_anchors('ref')
    assert bool((counts >= 0).all()) and bool((counts[:, :2].sum(dim=1) <= N).all())
    assert bool((counts[:, 2] <= NUM_POS).all()) and bool((counts[:, 2:].sum(dim=1) <= NUM).all())
    assert bool((assigned >= -2).all()) and bool((assigned <= gt.shape[1]).all())
    assert counts[1, 2:].tolist() == [int((sampled[1] > 0).sum()), int((sampled[1] < 0).sum())]
    want = rpn_sample_ref(r['assigned'][0], keys[0], NUM, NUM_POS)
    assert torch.equal(assigned[0].long(), r['assigned'][0]) and torch.equal(max_iou[0].view(torch.int32), r['max_iou'][0].view(torch.int32))
    assert torch.equal(sampled[0].long(), want)
    assert counts[0].tolist() == [int((r['assigned'][0] > 0).sum()), int((r['assigned'][0] == 0).sum()), int((want > 0).sum()), int((want < 0).sum())]
    off = 0
    for g in grads:                                                  # image 0: finite gradients, zero off-sample
        n = g.shape[1] * g.shape[2] * A
        g0, smp = g[0].cpu(), want[off:off + n]
        assert bool(torch.isfinite(g0).all()) and not bool(g0[..., :A].reshape(n)[smp == 0].any())
        off += n
    print(f'rpn hostile {backend} gt_count[1]={count1}: counts {counts.tolist()}, losses {losses.cpu().tolist()}')


@pytest.mark.parametrize('count1', [6, 1000, -5])
def test_hostile_emul(count1):
    _hostile('emul', count1)


@pytest.mark.gpu
@pytest.mark.parametrize('count1', [6, 1000, -5])
def test_hostile_gpu(count1):
    _hostile('hip', count1)


# ----------------------------------------------------------------------------- 9. ABI refusals (emulator)
def test_abi_refusals_emul():
    from hrfuser_amd import rpn
    dev = use_backend('emul')
    L = _lib.lib()
    c = CASES['ref']
    cm, rm = _nhwc('ref', dev)
    bases = [b.tolist() for b in BASES]
    N = _n_anchors('ref')
    gt, cnt = rpn.pack_gts(_ref('ref')['gts'], dev)
    G = gt.shape[1]
    shp, pad = torch.tensor(c['shapes'], dtype=torch.float32), torch.tensor(c['pads'], dtype=torch.float32)
    keys, st = _as_i32(_keys('ref', 'random')), rpn.rng_state(1, 2)
    ws = torch.empty(1 << 20, dtype=torch.uint8)
    outs = [torch.full((B, N), 77, dtype=torch.int32), torch.full((B, N), 77.0), torch.full((B, N), 77, dtype=torch.int32),
            torch.full((B, 4), 77, dtype=torch.int32)]
    gbuf = [torch.full(tuple(m.shape[:3]) + (16,), 77.0) for m in cm]
    losses = torch.full((2, 5), 77.0)

    def grads(edit=None):
        gr = _lib.RpnGrads()
        for l, g in enumerate(gbuf):
            gr.d_cls[l], gr.d_reg[l], gr.ld_cls[l], gr.ld_reg[l] = g.data_ptr(), g.data_ptr() + 4 * A, 16, 16
        if edit:
            edit(gr)
        return gr

    def untouched():
        return all(bool((t == 77).all()) for t in outs + gbuf + [losses]) and st.tolist() == [1, 2]

    def refused(edit_lv=None, edit_cfg=None, gmax=G, n=5, support=True, **kw):
        lv, cfg = rpn._levels(cm[:n], rm[:n], STRIDES[:n], bases[:n]), _cfg('ref')
        if edit_lv:
            edit_lv(lv)
        if edit_cfg:
            edit_cfg(cfg)
        if support and (L.hrf_rpn_train_supported(lv, cfg, gmax) != 0 or L.hrf_rpn_train_workspace_bytes(lv, cfg, gmax) != 0):
            return False
        a = dict(img_shape=shp, pad_shape=pad, gt=gt, gt_count=cnt, keys=keys, rng=st, ws=ws, wsb=ws.numel(), o0=outs[0], o1=outs[1], o2=outs[2],
                 o3=outs[3], gr=grads(), losses=losses)
        a.update(kw)
        head = (lv, cfg, a['img_shape'], a['pad_shape'], a['gt'], a['gt_count'], gmax, a['keys'], a['rng'], a['ws'], a['wsb'], a['o0'], a['o1'],
                a['o2'], a['o3'])
        calls = [lambda: L.hrf_rpn_loss(*head, a['gr'], a['losses'], 0)]
        if 'gr' not in kw and 'losses' not in kw:                    # (hrf_rpn_assign takes neither)
            calls.append(lambda: L.hrf_rpn_assign(*head, 0))
        for call in calls:
            with pytest.raises(_lib.HRFuserHipError, match='HRF_ERR_ARG'):
                call()
        return untouched()

    lv, cfg = rpn._levels(cm, rm, STRIDES, bases), _cfg('ref')
    assert L.hrf_rpn_train_supported(lv, cfg, G) == 1 and 0 < L.hrf_rpn_train_workspace_bytes(lv, cfg, G) <= ws.numel()
    assert untouched()
    for name, v in (('pos_iou_thr', 1.5), ('pos_iou_thr', float('nan')), ('neg_iou_thr', -0.1), ('min_pos_iou', 2.0), ('num', 0), ('num_pos', -1),
                    ('num_pos', NUM + 1), ('beta', 0.0), ('beta', float('nan')), ('loss_weight_cls', float('inf')), ('loss_weight_bbox', float('nan')),
                    ('allowed_border', 1 << 25)):
        assert refused(edit_cfg=lambda c_, name=name, v=v: setattr(c_, name, v)), (name, v)
    assert refused(gmax=0) and refused(gmax=_lib._header_int('HRF_RPN_MAX_GT', 0) + 1)
    assert refused(edit_lv=lambda v: setattr(v, 'A', 4))
    assert refused(edit_lv=lambda v: setattr(v, 'num_levels', 6))
    assert refused(edit_lv=lambda v: setattr(v, 'num_levels', 0))
    assert refused(edit_lv=lambda v: setattr(v, 'B', 0))
    assert refused(edit_lv=lambda v: v.cls.__setitem__(2, None))
    assert refused(edit_lv=lambda v: v.reg.__setitem__(0, None))
    assert refused(edit_lv=lambda v: v.ld_cls.__setitem__(1, A - 1))
    assert refused(edit_lv=lambda v: v.ld_reg.__setitem__(4, 4 * A - 1))
    assert refused(edit_lv=lambda v: v.H.__setitem__(3, 0))
    assert refused(edit_lv=lambda v: v.stride.__setitem__(0, 0))
    for k in ('img_shape', 'pad_shape', 'gt', 'gt_count', 'ws', 'o0', 'o1', 'o2', 'o3'):
        assert refused(support=False, **{k: None}), k
    assert refused(support=False, keys=None, rng=None)
    assert refused(support=False, wsb=1024)
    assert refused(support=False, gr=None) and refused(support=False, losses=None)
    assert refused(support=False, gr=grads(lambda g: g.d_cls.__setitem__(1, None)))
    assert refused(support=False, gr=grads(lambda g: g.ld_reg.__setitem__(0, 4 * A - 1)))
    # the Python layer names what it refuses
    with pytest.raises(NotImplementedError, match='Gmax'):
        rpn.pack_gts([torch.zeros(300, 4)], dev)
    with pytest.raises(NotImplementedError, match='num_pos'):
        _call(rpn.rpn_assign, 'ref', dev, keys=_keys('ref', 'random'), num=8, num_pos=9)
    with pytest.raises(ValueError, match='rng_state'):
        _call(rpn.rpn_assign, 'ref', dev)
    # ... and the unedited call is accepted
    L.hrf_rpn_loss(lv, cfg, shp, pad, gt, cnt, G, keys, st, ws, ws.numel(), *outs, grads(), losses, 0)
    assert not untouched()


# ----------------------------------------------------------------------------- 10. the module
RPN_CFG = dict(type='RPNHead', in_channels=256, feat_channels=256,
               anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
               bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0]),
               loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
               loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0))
TRAIN_CFG = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1),
                 sampler=dict(type='RandomSampler', num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False),
                 allowed_border=0, pos_weight=-1, debug=False)
TEST_CFG = dict(nms_pre=200, max_per_img=300, nms=dict(type='nms', iou_threshold=0.7), min_bbox_size=0)


def _build(**edit):
    from hrfuser_amd import HEADS
    cfg = copy.deepcopy(dict(RPN_CFG, train_cfg=copy.deepcopy(TRAIN_CFG), test_cfg=copy.deepcopy(TEST_CFG)))
    for path, v in edit.items():
        d, keys = cfg, path.split('__')
        for k in keys[:-1]:
            d = d[k]
        d[keys[-1]] = v
    return HEADS.build(cfg)


def test_module_train_refusals():
    """what the kernels do not build raises NotImplementedError naming the key, at build time (no GPU needed)"""
    head = _build()
    assert head._train_cfg(head.train_cfg, head.loss_cls, head.loss_bbox) == dict(
        pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, allowed_border=0, num=256, num_pos=128, beta=1.0 / 9.0,
        loss_weight_cls=1.0, loss_weight_bbox=1.0)
    for edit, key in ((dict(train_cfg__assigner__type='ATSSAssigner'), 'assigner.type'), (dict(train_cfg__assigner__neg_iou_thr=(0.1, 0.3)), 'neg_iou_thr'),
                      (dict(train_cfg__assigner__ignore_iof_thr=0.5), 'ignore_iof_thr'), (dict(train_cfg__assigner__gt_max_assign_all=False), 'gt_max_assign_all'),
                      (dict(train_cfg__assigner__gpu_assign_thr=100), 'gpu_assign_thr'), (dict(train_cfg__sampler__type='OHEMSampler'), 'sampler.type'),
                      (dict(train_cfg__sampler__neg_pos_ub=3), 'neg_pos_ub'), (dict(train_cfg__sampler__add_gt_as_proposals=True), 'add_gt_as_proposals'),
                      (dict(train_cfg__pos_weight=2.0), 'pos_weight'), (dict(loss_bbox__type='L1Loss'), 'loss_bbox'),
                      (dict(loss_bbox=None), 'loss_bbox'), (dict(loss_cls__type='FocalLoss'), 'loss_cls')):
        with pytest.raises(NotImplementedError, match=key):
            _build(**edit)
    with pytest.raises(NotImplementedError, match='gt_bboxes_ignore'):
        head.loss([torch.zeros(1, 3, 2, 2)], [torch.zeros(1, 12, 2, 2)], [torch.zeros(0, 4)], [dict(img_shape=(8, 8, 3))], gt_bboxes_ignore=[torch.zeros(1, 4)])


@pytest.mark.gpu
def test_module_loss_gpu():
    from hrfuser_amd import rpn
    dev = use_backend('hip')
    head = _build().to(dev)
    r, c = _ref('ref'), CASES['ref']
    cls = [t.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in r['cs']]
    reg = [t.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in r['bp']]
    metas = [dict(img_shape=s + (3,), pad_shape=p + (3,)) for s, p in zip(c['shapes'], c['pads'])]
    gts = [g.to(dev) for g in r['gts']]
    st = head.rng(dev)
    st0 = st.clone()
    out = head.loss(cls, reg, gts, metas)
    assert sorted(out) == ['loss_rpn_bbox', 'loss_rpn_cls'] and len(out['loss_rpn_cls']) == len(out['loss_rpn_bbox']) == 5
    assert st.tolist() == [st0.tolist()[0], st0.tolist()[1] + 1]
    cm, rm = [t.detach().permute(0, 2, 3, 1) for t in cls], [t.detach().permute(0, 2, 3, 1) for t in reg]
    gt, cnt = rpn.pack_gts(gts, dev)
    fn = rpn.rpn_loss(cm, rm, c['shapes'], c['pads'], gt, cnt, STRIDES, [b.tolist() for b in BASES], _cfg('ref'), rng=st0.clone())
    assert torch.equal(torch.stack(out['loss_rpn_cls']), fn[0][0]) and torch.equal(torch.stack(out['loss_rpn_bbox']), fn[0][1])
    assert bool(torch.isfinite(fn[0]).all()) and float(fn[0][0, 0]) > 0 and float(fn[0][1, 0]) > 0
    # the targets of the head at the same counter: the functional call's
    head.rng(dev).copy_(st0)
    tg = head.get_targets(cls, reg, gts, metas)
    assert all(torch.equal(a, b) for a, b in zip(tg, fn[2:]))
    # backward: the stored maps scaled by the incoming gradients
    out['loss_rpn_cls'][0].backward(retain_graph=True)
    assert torch.equal(cls[0].grad, fn[1][0][..., :A].permute(0, 3, 1, 2)) and float(cls[0].grad.abs().max()) > 0
    assert not bool(reg[0].grad.any()) and not bool(cls[1].grad.any())
    (3.0 * out['loss_rpn_bbox'][1]).backward()
    assert torch.equal(reg[1].grad, 3.0 * fn[1][1][..., A:5 * A].permute(0, 3, 1, 2)) and float(reg[1].grad.abs().max()) > 0
    assert torch.equal(cls[0].grad, fn[1][0][..., :A].permute(0, 3, 1, 2))               # unchanged by the second backward
    # forward_train on a pyramid: mmdet's return types
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn(B, 256, h, w, generator=g).to(dev) for h, w in c['sizes']]
    losses = head.forward_train(feats, metas, gts)
    assert sorted(losses) == ['loss_rpn_bbox', 'loss_rpn_cls'] and all(bool(torch.isfinite(v)) for k in losses for v in losses[k])
    losses, props = head.forward_train(feats, metas, gts, proposal_cfg=TEST_CFG)
    assert len(props) == B and all(p.shape[1] == 5 for p in props)


@pytest.mark.gpu
def test_feature_extractor_rpn_loss_gpu():
    import hrfuser_oracle as O
    from hrfuser_amd.detector import FeatureExtractor
    dev = use_backend('hip')
    cfg = load_cfgs()['t_nus']
    torch.manual_seed(0)
    fx = FeatureExtractor(copy.deepcopy(cfg), dict(type='HRFPN', in_channels=[18, 36, 72, 144], out_channels=256), None,
                          copy.deepcopy(dict(RPN_CFG, train_cfg=copy.deepcopy(TRAIN_CFG), test_cfg=copy.deepcopy(TEST_CFG))))
    O.seeded_fill_(fx.backbone, 0)
    fx.neck.init_weights()
    fx.to(dev).eval()
    x, mods = O.seeded_inputs(B, 64, 96, cfg.get('mod_in_channels', [3, 3]), seed=1)
    kw = dict(zip(('lidar_img', 'radar_img', 'gated_img'), [m.to(dev) for m in mods]))
    with torch.no_grad():
        out = fx.rpn_loss(x.to(dev), [g.to(dev) for g in _ref('tiny')['gts']], [dict(img_shape=(64, 96, 3), pad_shape=(64, 96, 3)),
                                                                                  dict(img_shape=(60, 90, 3), pad_shape=(64, 96, 3))], **kw)
    vals = torch.stack(out['loss_rpn_cls'] + out['loss_rpn_bbox']).cpu()
    print('FeatureExtractor.rpn_loss', vals.tolist())
    assert vals.shape == (10,) and bool(torch.isfinite(vals).all()) and float(vals[:5].sum()) > 0


# ----------------------------------------------------------------------------- 11. capture
@pytest.mark.gpu
def test_loss_graph_gpu():
    """hrf_rpn_loss captured in a graph: after each replay the gt contents are overwritten in place; the replay equals an eager
    call on the new contents at the advanced counter"""
    from hrfuser_amd import rpn
    from hrfuser_amd import runtime as R
    dev = use_backend('hip')
    c = CASES['ref']
    cm, rm = _nhwc('ref', dev)
    bases = [b.tolist() for b in BASES]
    shp, pad = torch.tensor(c['shapes'], dtype=torch.float32).to(dev), torch.tensor(c['pads'], dtype=torch.float32).to(dev)
    gt, cnt = rpn.pack_gts(_ref('ref')['gts'], dev, gmax=8)
    st, cfg = rpn.rng_state(7, 0, dev), _cfg('ref')
    run = lambda rng: rpn.rpn_loss(cm, rm, shp, pad, gt, cnt, STRIDES, bases, cfg, rng=rng)          # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with R.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
        cap = run(st)
    st.copy_(rpn.rng_state(7, 0, dev))
    seen = []
    new_gts = [_ref('ref')['gts'], _draw_gts('ref', 1), [_draw_gts('crowded', 2)[0][:8], torch.zeros(0, 4)]]
    for k, gts in enumerate(new_gts):
        g2, c2 = rpn.pack_gts(gts, dev, gmax=8)
        gt.copy_(g2)
        cnt.copy_(c2)
        g.replay()
        torch.cuda.synchronize()
        assert st.tolist() == [7, k + 1]
        got = [t.clone() for t in _flat(cap)]
        fresh = _flat(run(rpn.rng_state(7, k, dev)))
        assert all(torch.equal(a, b) for a, b in zip(got, fresh)), k
        assert bool(torch.isfinite(got[0]).all())
        seen.append(got)
    assert not torch.equal(seen[0][-2], seen[1][-2]) and not torch.equal(seen[0][0], seen[2][0])
