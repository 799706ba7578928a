"""SingleRoIExtractor / RoIAlign on the HIP engine - the consumer of the HRFPN pyramid in every reference config
(configs/_base_/models/cascade_rcnn_hrfuser_fpn_*_fusion.py:152-156, once per cascade stage).

Drop-in for mmdet's `SingleRoIExtractor` (mmdet/models/roi_heads/roi_extractors/single_level_roi_extractor.py) with mmcv's
`RoIAlign(output_size=7, sampling_ratio=0)` as its roi layer: same registry name, constructor keywords and
`forward(feats, rois) -> (K, out_channels, 7, 7)` contract, no parameters.  ONE launch serves all levels forward
(hrf_roi_align_fwd) and one backward (hrf_roi_align_bwd): the kernel derives each box's level itself, so nothing here reads
`rois` on the host, sorts, or synchronises - the calls can be captured in a hipGraph.  The maps are read in place when they are
channels-last storage (what `HRFPN.forward` returns).

Three entries: the module / `roi_align` on torch tensors (torch.autograd bridge `_RoiFn`), and `extract_nhwc` on the explicit
tape of `runtime.Ctx` for callers that consume the neck's `Act`s directly.  There is no CPU fallback.
"""
import torch
import torch.nn as nn

from . import _lib
from . import runtime as R
from .registry import ROI_EXTRACTORS

POOLED = 7


def _nhwc(t):
    """logical NCHW fp32 -> (B,H,W,C) contiguous: a view of channels-last storage, otherwise ONE copy."""
    if t.dtype != torch.float32:
        raise TypeError(f'roi_align: fp32 maps only, got {t.dtype}')
    return t.permute(0, 2, 3, 1).contiguous()


def _levels(maps, dmaps, scales, finest_scale):
    """hrf_roi_levels_t over NHWC tensors `maps` (and their gradient targets `dmaps`, or None)."""
    lv = _lib.RoiLevels()
    B, _, _, C = maps[0].shape
    lv.num_levels, lv.C, lv.B, lv.pooled = len(maps), C, B, POOLED
    lv.finest_scale = float(finest_scale)
    for l, m in enumerate(maps):
        if m.shape[0] != B or m.shape[3] != C:
            raise ValueError(f'roi_align: level {l} is {tuple(m.shape)} (NHWC), level 0 has B = {B}, C = {C}')
        H, W, ld = m.shape[1], m.shape[2], m.stride(2)
        if m.stride(3) != 1 or ld < C or m.stride(1) != W * ld or m.stride(0) != H * W * ld:
            raise ValueError(f'roi_align: level {l} is not [B][H][W] rows of one pitch (strides {tuple(m.stride())})')
        lv.feat[l] = m.data_ptr()
        lv.dfeat[l] = dmaps[l].data_ptr() if dmaps is not None else None
        lv.H[l], lv.W[l], lv.ld[l] = m.shape[1], m.shape[2], m.stride(2)
        lv.spatial_scale[l] = float(scales[l])
    return lv


def _check(maps, rois, scales):
    L = _lib.lib()
    if not 1 <= len(maps) <= 4 or len(scales) != len(maps):
        raise ValueError(f'roi_align: 1..4 levels with one scale each, got {len(maps)} maps / {len(scales)} scales')
    for t in tuple(maps) + (rois,):
        if L.require_cuda and not t.is_cuda:
            raise _lib.HRFuserHipError(f'roi_align: tensor on {t.device}; the HIP path has no CPU fallback')
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise ValueError(f'roi_align: rois must be (K, 5) = (batch index, x1, y1, x2, y2), got {tuple(rois.shape)}')
    C = maps[0].shape[3]
    if not L.hrf_roi_align_supported(C, POOLED, len(maps)):
        raise NotImplementedError(f'roi_align on the HIP engine: {C} channels is not supported (C % 4 == 0, C <= 256)')
    return L


def roi_forward(maps, rois, scales, finest_scale=56.0, out_layout=0, out=None, stream=None):
    """maps: NHWC fp32 tensors (one per level), rois (K,5) -> (K,C,7,7) (out_layout 0) or (K,7,7,C) (1).  One launch."""
    L = _check(maps, rois, scales)
    rois = rois.detach().float().contiguous()
    K, C = rois.shape[0], maps[0].shape[3]
    if out is None:
        out = torch.empty((K, C, POOLED, POOLED) if out_layout == 0 else (K, POOLED, POOLED, C), device=rois.device, dtype=torch.float32)
    L.hrf_roi_align_fwd(_levels(maps, None, scales, finest_scale), rois, K, out, out_layout, _lib.stream_ptr() if stream is None else stream)
    return out


def roi_backward(maps, dmaps, rois, scales, dout, finest_scale=56.0, out_layout=0, stream=None):
    """dmaps[l] += the adjoint of roi_forward applied to dout.  One launch; refused in deterministic mode."""
    L = _check(maps, rois, scales)
    rois = rois.detach().float().contiguous()
    L.hrf_roi_align_bwd(_levels(maps, dmaps, scales, finest_scale), rois, rois.shape[0], dout, out_layout,
                        _lib.stream_ptr() if stream is None else stream)


class _RoiFn(torch.autograd.Function):
    """torch.autograd bridge: a PyTorch RoI head trains on top of the pyramid.  rois get no gradient (as in mmcv)."""

    @staticmethod
    def forward(fctx, rois, scales, finest_scale, *feats):
        maps = [_nhwc(t) for t in feats]
        out = roi_forward(maps, rois, scales, finest_scale, 0)
        fctx.hrf = (maps, rois.detach().float().contiguous(), scales, finest_scale)
        return out

    @staticmethod
    def backward(fctx, gout):
        maps, rois, scales, finest_scale = fctx.hrf
        dmaps = [torch.zeros_like(m) for m in maps]             # channels-last gradients of the used maps
        roi_backward(maps, dmaps, rois, scales, gout.float().contiguous(), finest_scale, 0)
        return (None, None, None) + tuple(d.permute(0, 3, 1, 2) for d in dmaps)


def _roi_layer_check(roi_layer, who):
    cfg = dict(roi_layer)
    kind = cfg.pop('type', None)
    if kind != 'RoIAlign':
        raise NotImplementedError(f'{who} on the HIP engine: roi_layer type {kind!r} is not built (every HRFuser config uses RoIAlign)')
    osz = cfg.pop('output_size', None)
    if osz not in (POOLED, (POOLED, POOLED), [POOLED, POOLED]):
        raise NotImplementedError(f'{who} on the HIP engine: output_size {osz!r} is not built (7 in every HRFuser config)')
    _knob_check(who, sampling_ratio=cfg.pop('sampling_ratio', 0), pool_mode=cfg.pop('pool_mode', 'avg'), aligned=cfg.pop('aligned', True))
    if cfg:
        raise NotImplementedError(f'{who} on the HIP engine: roi_layer keys {sorted(cfg)} are not built')


def _knob_check(who, sampling_ratio, pool_mode, aligned):
    if sampling_ratio != 0:
        raise NotImplementedError(f'{who} on the HIP engine: sampling_ratio {sampling_ratio!r} is not built (0 = adaptive in every HRFuser config)')
    if pool_mode != 'avg':
        raise NotImplementedError(f'{who} on the HIP engine: pool_mode {pool_mode!r} is not built (avg)')
    if aligned is not True:
        raise NotImplementedError(f'{who} on the HIP engine: aligned={aligned!r} is not built (True, the mmcv default)')


def roi_align(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True):
    """mmcv.ops.roi_align's call shape for one map: input (B,C,H,W), rois (K,5) -> (K,C,7,7)."""
    if output_size not in (POOLED, (POOLED, POOLED), [POOLED, POOLED]):
        raise NotImplementedError(f'roi_align on the HIP engine: output_size {output_size!r} is not built (7)')
    _knob_check('roi_align', sampling_ratio, pool_mode, aligned)
    return _RoiFn.apply(rois, (float(spatial_scale),), 56.0, input)


@ROI_EXTRACTORS.register_module()
class SingleRoIExtractor(nn.Module):
    """single_level_roi_extractor.py:10-108.  `feats`: the pyramid (logical NCHW, finest first; the first
    len(featmap_strides) maps are used, like mmdet's heads do); `rois` (K,5) = (batch index, x1, y1, x2, y2)."""

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56, init_cfg=None):
        super().__init__()
        _roi_layer_check(roi_layer, 'SingleRoIExtractor')
        if not 1 <= len(featmap_strides) <= 4:
            raise NotImplementedError(f'SingleRoIExtractor on the HIP engine: {len(featmap_strides)} levels (1..4 are built)')
        self.roi_layer = dict(roi_layer)
        self.out_channels = out_channels
        self.featmap_strides = list(featmap_strides)
        self.finest_scale = finest_scale
        self.init_cfg = init_cfg
        self.fp16_enabled = False

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def init_weights(self):
        pass

    def map_roi_levels(self, rois, num_levels):
        """single_level_roi_extractor.py:36-55 in torch (the kernel evaluates the same mapping itself; kept for users and tests)."""
        scale = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
        lvls = torch.floor(torch.log2(scale / self.finest_scale + 1e-6))
        return lvls.clamp(min=0, max=num_levels - 1).long()

    def _scales(self):
        return tuple(1.0 / s for s in self.featmap_strides)

    def forward(self, feats, rois, roi_scale_factor=None):
        if roi_scale_factor is not None:
            raise NotImplementedError(f'SingleRoIExtractor on the HIP engine: roi_scale_factor {roi_scale_factor!r} is not built '
                                      '(CascadeRoIHead never passes it)')
        feats = tuple(feats)[:self.num_inputs]
        if len(feats) != self.num_inputs:
            raise ValueError(f'SingleRoIExtractor: {self.num_inputs} strides, {len(feats)} maps')
        if feats[0].shape[1] != self.out_channels:
            raise ValueError(f'SingleRoIExtractor: maps of {feats[0].shape[1]} channels, out_channels = {self.out_channels}')
        return _RoiFn.apply(rois, self._scales(), float(self.finest_scale), *feats)

    def extract_nhwc(self, ctx, acts, rois, out_layout=0):
        """Tape-level entry: `acts` = runtime.Act's of the pyramid (NHWC, e.g. HRFPN._run's outputs, in place) -> Act of
        (K,C,7,7) (out_layout 0) or (K,7,7,C) (1).  With a recording ctx the backward closure goes on the tape: it adds into
        act.grad of every used level, creating it zeroed when it is None."""
        acts = list(acts)[:self.num_inputs]
        maps = [a.t for a in acts]
        scales, fs = self._scales(), float(self.finest_scale)
        rois = rois.detach().float().contiguous()
        K, C = rois.shape[0], maps[0].shape[3]
        shape = (K, C, POOLED, POOLED) if out_layout == 0 else (K, POOLED, POOLED, C)
        out = R.Act(roi_forward(maps, rois, scales, fs, out_layout, out=R._new(shape, rois.device), stream=ctx.stream))

        def bwd():
            if out.grad is None or not any(a.needs_grad for a in acts):
                return
            for a in acts:
                if a.grad is None:
                    a.grad = R.gpu_zero_(R._new_like(a.t))
            roi_backward(maps, [a.grad for a in acts], rois, scales, out.grad, fs, out_layout, stream=ctx.stream)
        ctx.push(bwd)
        return out


def build_roi_extractor(cfg):
    """mmdet.models.builder.build_roi_extractor (builder.py:28-30)."""
    return ROI_EXTRACTORS.build(cfg)
