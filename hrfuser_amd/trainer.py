"""Data-parallel training step for the HIP backbone (one process per GPU, RCCL over xGMI).

Mirrors what the reference gets from mmdet/apis/train.py:113-121 (MMDistributedDataParallel,
find_unused_parameters=True), nn.SyncBatchNorm and the AdamW `paramwise_cfg` of
configs/hrfuser/*_fusion.py:37-48 - restricted to the backbone hot path:

  * forward + backward run on the explicit tape (no torch.autograd graph);
  * every parameter gradient already lives in ONE flat fp32 arena, so the gradient exchange is a
    handful of large RCCL all-reduces on slices of that arena (no per-parameter bucketing copies,
    unused parameters such as transition1.0.1.* are simply zeros in the arena);
  * SyncBN = all-reduce of the per-channel fp64 (sum, sumsq) slots between the producing conv and
    the BN-finalize kernel (runtime.bn_forward / bn_backward_coef);
  * the optimizer is one fused AdamW launch over the flat arena with a per-element decay mask
    (decay_mult=0 for `relative_position_bias_table` and `norm` keys) and a device-side step count;
  * the whole step is captured into a hipGraph when possible (launch-bound regime at batch 2);
  * optional, all on the device so the captured step stays one graph: global gradient-norm clipping (mmcv's
    OptimizerHook(grad_clip=dict(max_norm=..., norm_type=2)) = torch.nn.utils.clip_grad_norm_ over the arena), skipping a
    step whose gradient norm is not finite, and gradient accumulation over k micro-batches (mmcv's
    GradientCumulativeOptimizerHook; DDP no_sync for all but the last micro-batch).
"""
import os

import torch

from . import _lib
from . import runtime as R

NO_DECAY_KEYS = ('absolute_pos_embed', 'relative_position_bias_table', 'norm')


class Trainer:
    def __init__(self, net, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, group=None,
                 world_size=1, n_buckets=4, deterministic=None, max_norm=None, norm_type=2, skip_nonfinite=False):
        """max_norm: clip the global L2 norm of the (averaged) gradient arena to it before AdamW, as clip_grad_norm_ does
        (None: no clipping; the norm covers the parameters of this arena that receive a gradient).  skip_nonfinite: a step
        whose gradient norm is NaN / Inf leaves the parameters, m, v and the step count untouched and is counted
        (skipped_steps()) - the BatchNorm running statistics of that step's forward HAVE moved by then; False is torch /
        mmcv behaviour: the NaN propagates into the parameters.  With neither, the step issues exactly the two optimizer
        launches it always did and allocates nothing more."""
        if norm_type != 2:
            raise ValueError(f'Trainer: norm_type {norm_type!r} is not supported (only the L2 norm, norm_type=2)')
        self.net = net
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.clipping = max_norm is not None or self.skip_nonfinite
        self.clip = None                     # device float[8] of hrf_adamw_tick_clip (include/hrfuser_hip.h), for asynchronous logging
        self._accum = 1                      # micro-batches behind the optimizer step being issued
        if deterministic is not None:        # None: follow the net (net.set_deterministic / HRF_DETERMINISTIC)
            net.set_deterministic(bool(deterministic))
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.group, self.world = group, world_size
        self.n_buckets = n_buckets
        self.force = R.force_collectives() and group is not None
        if world_size > 1 or self.force:
            net.set_sync_group(group, world_size)
        self._ready = False
        self.graph = None
        self._graph_det = None               # (deterministic mode, engine's det_epoch) the graph was captured in
        self._graph_mm = None                # matrix mode of the net (HRFPN.set_matrix_mode) the graph was captured in
        self.collectives_per_step = 0

    # -------------------------------------------------------------------------------------------
    def _setup(self, device):
        eng = self.net._engine()
        eng.ready(device)
        n = eng.flat_p.numel()
        self.m = torch.zeros(n, device=device)
        self.v = torch.zeros(n, device=device)
        self.state = torch.zeros(4, device=device)
        mask = torch.ones(n, device=device)
        unused = set(getattr(self.net, 'unused_parameter_names', lambda: ())())
        for (name, p), (off, cnt) in zip(self.net.named_parameters(), eng._spans):
            # mmcv DefaultOptimizerConstructor custom_keys: substring match on the parameter name
            if any(k in name for k in NO_DECAY_KEYS):
                mask[off:off + cnt] = 0.0
            if name in unused or not p.requires_grad:
                mask[off:off + cnt] = -1.0            # no gradient ever: torch.optim leaves such parameters untouched
        self.wd_mask = mask
        self.state[3] = self.lr
        if self.clipping:
            self.clip = torch.zeros(8, device=device)
            self.clip[4] = 0.0 if self.max_norm is None else self.max_norm
            self._nparts = int(self.net._lib_handle().hrf_grad_sumsq_parts(n))
            self._partials = torch.zeros(self._nparts, device=device, dtype=torch.float64)
        self._ready = True

    def set_lr(self, lr):
        """Learning rate of the NEXT steps, also for an already captured hipGraph (the kernel reads it from the device)."""
        self.lr = float(lr)
        if self._ready:
            self.state[3:4].fill_(self.lr)

    def set_max_norm(self, max_norm):
        """max_norm of the NEXT steps, also for an already captured hipGraph (the kernel reads it from the device, like the
        learning rate); None, <= 0 or inf: report the norm, do not clip."""
        if not self.clipping:
            raise ValueError('Trainer.set_max_norm: this Trainer was built without max_norm / skip_nonfinite (no norm is computed)')
        self.max_norm = None if max_norm is None else float(max_norm)
        if self._ready:
            self.clip[4:5].fill_(0.0 if self.max_norm is None else self.max_norm)

    def _clip_slot(self, i):
        if self.clip is None:
            raise ValueError('Trainer: built without max_norm / skip_nonfinite, or no step has run yet (no norm is computed)')
        return float(self.clip[i].item())

    def grad_norm(self):
        """Global L2 norm of the averaged gradient of the last step, before clipping (mmcv logs it as grad_norm).
        Synchronises (a device-to-host read of `clip`); log from `tr.clip` to stay asynchronous."""
        return self._clip_slot(1)

    def clip_coef(self):
        """The factor the last step's gradient was multiplied with, min(1, max_norm / (norm + 1e-6)).  Synchronises."""
        return self._clip_slot(0)

    def skipped_steps(self):
        """Steps skipped so far because their gradient norm was not finite (skip_nonfinite=True).  Synchronises."""
        return int(self._clip_slot(3))

    def optimizer_step(self):
        """Fused AdamW over the flat arenas (device-side step count and learning rate); with clipping / skip_nonfinite the
        norm of the arena first: hrf_grad_sumsq, hrf_adamw_tick_clip, hrf_adamw_clipped."""
        net = self.net
        eng = net._engine()
        L = net._lib_handle()
        s = _lib.stream_ptr()
        n = eng.flat_p.numel()
        gscale = 1.0 / (self.world * self._accum)
        if not self.clipping:
            L.hrf_adamw_tick(self.state, self.betas[0], self.betas[1], s)
            L.hrf_adamw(eng.flat_p, eng.flat_g, self.m, self.v, self.wd_mask, n, -1.0,
                        self.betas[0], self.betas[1], self.eps, self.wd, self.state, gscale, s)
            return
        L.hrf_grad_sumsq(eng.flat_g, self.wd_mask, n, self._partials, s)
        L.hrf_adamw_tick_clip(self.state, self.clip, self._partials, self._nparts, gscale, int(self.skip_nonfinite),
                              self.betas[0], self.betas[1], s)
        L.hrf_adamw_clipped(eng.flat_p, eng.flat_g, self.m, self.v, self.wd_mask, n, -1.0,
                            self.betas[0], self.betas[1], self.eps, self.wd, self.state, gscale, self.clip, s)

    def buckets(self, n):
        """Contiguous slices of the flat gradient arena for the RCCL all-reduce (>= 1 MiB each)."""
        nb = max(1, min(self.n_buckets, n // (256 * 1024)))
        step = (n + nb - 1) // nb
        return [(i, min(n, i + step)) for i in range(0, n, step)]

    def overlap_rounds(self, n):
        """Groups of buckets whose all-reduce overlaps the weight-gradient leaves of the next group.  HRF_GRAD_OVERLAP: a number,
        or auto = one group per bucket from 64 MB of gradients (HRFuser-B: 243 MB, ~5 ms on xGMI beside a > 10 ms
        weight-gradient phase), a single group below (HRFuser-T: 16 MB = 0.3 ms - every extra fork / join of the leaf lanes
        costs more than it hides)."""
        v = os.environ.get('HRF_GRAD_OVERLAP', 'auto').strip().lower()
        if v not in ('', 'auto'):
            return max(1, int(v))
        return self.n_buckets if 4 * n >= (64 << 20) else 1

    def _step_impl(self, x, mods, cots, grads_only=False):
        return self._cycle_impl([(x, mods, cots)], grads_only)[0]

    def _cycle_impl(self, batches, grads_only=False):
        """One optimizer step over the micro-batches [(x, mods, cots), ...]: the arena is zeroed once, every weight-gradient
        leaf adds into it, only the last backward carries the gradient exchange (DDP no_sync; SyncBN exchanges in every
        micro-batch), AdamW / the clip divide by world * k."""
        net = self.net
        eng = net._engine()
        L = net._lib_handle()
        if L.hrf_get_deterministic() and (self.world > 1 or self.force):
            raise _lib.HRFuserHipError('deterministic mode: a gradient / SyncBN exchange over a process group is not supported '
                                       '(the cross-rank summation order is outside the mode; a forced one-rank group takes the '
                                       'same exchange path and is refused with it): Trainer with a process group')
        R.gpu_zero_(eng.flat_g)
        ncoll = n_p2p = n_grad = 0
        hist, all_outs = {}, []
        for j, (x, mods, cots) in enumerate(batches):
            ctx, outs, _ = net._execute((x,) + tuple(mods), True)
            for o, c in zip(outs, cots):
                o.grad = R.gpu_clone(c)         # synthetic loss  L = sum_i <out_i, cot_i>   
            if (self.world > 1 or self.force) and j == len(batches) - 1:
                import torch.distributed as dist
                # the gradient exchange is part of the backward pass: the weight-gradient leaves are issued bucket group by bucket
                # group and a group's all-reduce runs on a communication lane beside the next group's leaves (runtime.Ctx.
                # _exchange_rounds; the reference: DDP's bucketed overlap, mmdet/apis/train.py:113-121)
                ctx.exchange = (self.buckets(eng.flat_g.numel()),
                                lambda a, b: dist.all_reduce(eng.flat_g[a:b], group=self.group), self.overlap_rounds(eng.flat_g.numel()))
            ctx.run_backward()
            ncoll += ctx.n_collectives + ctx.n_grad_collectives
            n_p2p += ctx.n_p2p
            n_grad += ctx.n_grad_collectives
            for key, cnt in ctx.xhist.items():
                hist[key] = hist.get(key, 0) + cnt
            all_outs.append(outs)
        self.p2p_exchanges_per_step = n_p2p
        self.grad_collectives_per_step = n_grad
        self.collectives_per_step = ncoll
        self.exchange_hist = hist
        self.sync_schedule = ctx.schedule_desc()
        if not grads_only:
            self._accum = len(batches)
            self.optimizer_step()
        st = net.__dict__.get('_stage_stamps')
        if st is not None:
            st.take(ctx, 'step', 'step_end')
        return all_outs

    def step(self, x, mods, cots, grads_only=False):
        """One eager training step (forward, backward, gradient exchange, AdamW; grads_only: no optimizer step - the
        all-reduced gradient arena of the step stays in net._engine().flat_g)."""
        if not self._ready:
            self._setup(x.device)
        outs = self._step_impl(x, mods, cots, grads_only)
        self._poll_exchange()
        return outs

    def step_accumulated(self, batches, grads_only=False):
        """One eager optimizer step over k >= 1 micro-batches [(x, mods, cots), ...] (gradient accumulation): one forward and
        backward each, the gradients summed in the arena, ONE gradient exchange (with the last backward), AdamW and the clip
        on the mean over world * k.  With plain BatchNorm this is a k-rank data-parallel run without SyncBN, its per-micro-
        batch BatchNorm statistics included.  Returns the list of the k outputs."""
        batches = list(batches)
        if not batches:
            raise ValueError('Trainer.step_accumulated: at least one micro-batch')
        if not self._ready:
            self._setup(batches[0][0].device)
        outs = self._cycle_impl(batches, grads_only)
        self._poll_exchange()
        return outs

    def _exchange(self):
        """The peer-to-peer SyncBN exchange context of the engine, or None (plain BatchNorm, the collective schedules, or the
        agreed fallback of the auto mode: Engine.p2p_context stores (group, world, None, mode) then)."""
        px = self.net._engine().__dict__.get('_p2p')
        return px[2] if (px is not None and px[2] is not None) else None

    def _poll_exchange(self):
        """Step boundary: a lost SyncBN exchange (a peer that did not arrive within HRF_P2P_TIMEOUT_S) raises here, one step
        late at the latest, without a host synchronisation (P2PExchange.poll)."""
        px = self._exchange()
        if px is not None:
            px.poll()

    # -------------------------------------------------------------------------------------------
    def capture(self, x, mods, cots, warmup=2):
        """Capture the full step into a hipGraph (static input buffers x/mods/cots)."""
        g = self._capture([(x, mods, cots)], warmup)
        self._graph_outs = self._graph_outs[0]
        return g

    def capture_accumulated(self, batches, warmup=2):
        """Capture one accumulated optimizer step (step_accumulated) into ONE hipGraph with k sets of static input buffers;
        replay() then runs one optimizer step.  _graph_outs: the list of the k outputs."""
        batches = list(batches)
        if not batches:
            raise ValueError('Trainer.capture_accumulated: at least one micro-batch')
        return self._capture(batches, warmup)

    def _capture(self, batches, warmup):
        if not self._ready:
            self._setup(batches[0][0].device)
        side = torch.cuda.Stream(priority=int(os.environ.get('HRF_LANE_PRIORITY', '0')))
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._cycle_impl(batches)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        old = self.__dict__.pop('_graph_px', None)
        if old is not None:
            old.unpin()                  # the graph this capture replaces goes away with its pin
        px = self._exchange()
        if px is not None:
            # the per-lane exchange-order digest of the first eager step is compared across ranks HERE, outside the capture: with
            # warmup = 0 after one eager step the second forward would be the captured one and skip it
            px.verify_order()
        if self.world > 1 or self.force:
            # The RCCL watchdog thread is still polling the end events of the warm-up collectives (one
            # sweep per 100 ms); an event query that lands on the communicator stream after it joined the
            # capture invalidates the capture ("capturing stream has unjoined work": 3 of 6 runs).  Give
            # the watchdog time to retire the eager work first (6 of 6 runs pass with the pause).
            import time
            time.sleep(float(os.environ.get('HRF_CAPTURE_SETTLE', '1.0')))
        g = torch.cuda.CUDAGraph()
        # thread_local: the RCCL watchdog thread polls events of earlier (eager) collectives while we
        # capture; in the default "global" mode such a call from another thread invalidates the capture
        # ("capturing stream has unjoined work", seen in ~3 of 4 runs with collectives in the graph)
        with R.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
            self._graph_outs = self._cycle_impl(batches)
        self.graph = g
        self._graph_det = (int(self.net._lib_handle().hrf_get_deterministic()), self.net._engine().det_epoch)
        self._graph_mm = getattr(self.net, 'matrix_mode', 'fp32')
        px = self._exchange()
        if px is not None:
            px.pin()                     # the graph's exchange launches carry the context's inbox / flag / counter pointers
            self._graph_px = px          # (Engine.p2p_context never closes a pinned context)
        return g

    def replay(self):
        if self._graph_det != (int(self.net._lib_handle().hrf_get_deterministic()), self.net._engine().det_epoch):
            raise _lib.HRFuserHipError('Trainer.replay: the deterministic mode was switched since this graph was captured '
                                       '(net.set_deterministic) - capture again')
        if self._graph_mm != getattr(self.net, 'matrix_mode', 'fp32'):
            raise _lib.HRFuserHipError(f'Trainer.replay: this graph was captured in matrix mode {self._graph_mm!r}, the net is in '
                                       f'{self.net.matrix_mode!r} now (set_matrix_mode) - capture again')
        self.graph.replay()
        self._poll_exchange()

    def check(self):
        """Raise if a peer-to-peer SyncBN exchange timed out (synchronises: call where the caller synchronises anyway - the
        end of a timed loop, an evaluation interval)."""
        px = self._exchange()
        if px is not None:
            if px.err.device.type == 'cuda':
                torch.cuda.synchronize()
            px.check()


def make_cotangents(net, x, mods, seed=5):
    """Fixed random output cotangents (NHWC) for the synthetic loss, shaped by a dry eval forward."""
    was = net.training
    net.eval()
    with torch.no_grad():
        ys = net(x, list(mods))
    net.train(was)
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(tuple(y.permute(0, 2, 3, 1).shape), generator=g).to(x.device) / y.numel() for y in ys]
