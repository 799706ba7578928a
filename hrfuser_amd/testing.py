"""Harness that runs a SUB-BLOCK of the backbone (Bottleneck, HRFormerBlock, fusion block, HR
module ...) on the HIP engine with NCHW torch tensors in/out, so block-level parity tests can
compare each piece against the oracle exactly like the reference's own module boundaries."""
import torch

from . import runtime as R
from .backbone import HipModule


class BlockHarness(HipModule):
    """`runner(ctx, block, acts) -> list[Act]`; inputs/outputs are logical NCHW tensors."""

    def __init__(self, block, runner):
        super().__init__()
        self.block = block
        self._runner = runner

    def forward(self, *inputs):
        return self._call_engine(tuple(inputs))

    def _wrap_inputs(self, inputs):
        return [R.Act(t.permute(0, 2, 3, 1).contiguous(), bool(t.requires_grad)) for t in inputs]

    def _run(self, ctx, srcs):
        outs = self._runner(ctx, self.block, srcs)
        return list(outs) if isinstance(outs, (list, tuple)) else [outs]


# ----------------------------------------------------------------------------- SingleRoIExtractor / RoIAlign restatement
# The oracle of hrfuser_amd.roi (mmcv is not installed here: parity against real mmcv is unpinned).  A literal fp64
# restatement of mmcv 1.3.17 RoIAlign(aligned=True, pool_mode='avg', sampling_ratio=0): the per-sample loop, four corners per
# sample.  Only the sample positions and the integer decisions are plain Python; the feature values pass through differentiable
# torch ops, so torch.autograd.grad of the result IS the backward reference.  tests/test_roi_align.py pins it against
# F.grid_sample + avg_pool2d on boxes that stay inside the map.
def roi_level_ref(rois, num_levels, finest_scale=56):
    """map_roi_levels (single_level_roi_extractor.py:36-55) in fp32, as the reference evaluates it -> (K,) int64.  A box whose
    scale is NaN (a negative area) matches no level there and keeps its row of zeros: level -1 here."""
    r = rois.detach().float().cpu()
    s = torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
    lv = torch.floor(torch.log2(s / finest_scale + 1e-6)).clamp(min=0, max=num_levels - 1)
    return torch.where(torch.isnan(lv), torch.full_like(lv, -1), lv).long()


def roi_samples(box, spatial_scale, H, W, P=7):
    """Sample positions of one box (x1, y1, x2, y2 as Python floats) -> (ys [P][grid_h], xs [P][grid_w], count)."""
    import math
    x1, y1, x2, y2 = (float(v) * spatial_scale - 0.5 for v in box)
    rw, rh = x2 - x1, y2 - y1
    bin_h, bin_w = rh / P, rw / P
    grid_h, grid_w = math.ceil(rh / P), math.ceil(rw / P)
    ys = [[y1 + ph * bin_h + (iy + 0.5) * bin_h / grid_h for iy in range(grid_h)] for ph in range(P)]
    xs = [[x1 + pw * bin_w + (ix + 0.5) * bin_w / grid_w for ix in range(grid_w)] for pw in range(P)]
    return ys, xs, max(grid_h * grid_w, 1)


def _roi_corner(v, n):
    """bilinear_interpolate of one axis: v already inside [-1, n] -> (low, high, weight of low, weight of high)"""
    v = max(v, 0.0)
    lo = int(v)
    if lo >= n - 1:
        lo = hi = n - 1
        v = float(lo)
    else:
        hi = lo + 1
    l = v - lo
    return lo, hi, 1.0 - l, l


def roi_align_ref(feat, rois, spatial_scale, P=7):
    """feat (B,C,H,W) fp64 (may require grad), rois (K,5) -> (K,C,P,P) fp64: the literal per-sample loop."""
    B, C, H, W = feat.shape
    flat = feat.permute(0, 2, 3, 1).reshape(B * H * W, C)
    rows = []
    for r in rois.detach().double().cpu().tolist():
        idx, wts, dst = [], [], []
        b = int(r[0])
        ys, xs, count = roi_samples(r[1:], spatial_scale, H, W, P)
        for ph in range(P):
            for pw in range(P):
                for y in ys[ph]:
                    for x in xs[pw]:
                        if y < -1.0 or y > H or x < -1.0 or x > W:
                            continue
                        yl, yh, hy, ly = _roi_corner(y, H)
                        xl, xh, hx, lx = _roi_corner(x, W)
                        for yy, xx, w in ((yl, xl, hy * hx), (yl, xh, hy * lx), (yh, xl, ly * hx), (yh, xh, ly * lx)):
                            idx.append((b * H + yy) * W + xx)
                            wts.append(w / count)
                            dst.append(ph * P + pw)
        row = torch.zeros(P * P, C, dtype=feat.dtype)
        if idx:
            vals = flat[torch.tensor(idx)] * torch.tensor(wts, dtype=feat.dtype)[:, None]
            row = row.index_add(0, torch.tensor(dst), vals)
        rows.append(row.t().reshape(C, P, P))
    return torch.stack(rows) if rows else feat.new_zeros(0, C, P, P)


def roi_extract_ref(feats, rois, strides, finest_scale=56, levels=None, P=7):
    """SingleRoIExtractor.forward on fp64 NCHW maps -> (K,C,P,P) fp64; `levels`: the level of every box instead of
    roi_level_ref's (tests force a wrong one)."""
    L = len(strides)
    lv = roi_level_ref(rois, L, finest_scale) if levels is None else levels
    if L == 1 and levels is None:
        lv = torch.zeros_like(lv)
    K, C = rois.shape[0], feats[0].shape[1]
    out = feats[0].new_zeros(K, C, P, P)
    for l in range(L):
        sel = torch.nonzero(lv == l)[:, 0]
        if sel.numel():
            ss = float(torch.tensor(1.0 / strides[l], dtype=torch.float32))
            out = out.index_add(0, sel, roi_align_ref(feats[l], rois[sel], ss, P))
    return out
