/* hrfuser_hip.h — C ABI of libhrfuser_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the HRFuser backbone hot path.  The reference has no
 * native layer: its backbone calls PyTorch ATen ops (cuDNN/cuBLAS underneath).  Every entry
 * point below names the ATen call sites in /root/reference it replaces; a host binding
 * (ctypes here, cgo/JNI elsewhere) passes raw device pointers, sizes and a hipStream_t.
 *
 * Conventions
 *   - all activations fp32, NHWC ("NLC" in the reference) unless explicit element strides
 *     (sB,sY,sX,sC) are taken, which also admit NCHW views (network inputs / input grads);
 *   - weights keep the reference's parameter layouts (Conv2d OIHW, Linear (out,in)) so
 *     state-dicts load unchanged;
 *   - every function enqueues on `stream` and returns immediately: 0 = HRF_OK, 1 = bad argument,
 *     2 = launch failure.  Nothing throws, allocates, or synchronises.  Re-entrant per device.
 *   - "stats" buffers are double[2*C] = (sum, sum of squares | sum, sum*x) accumulated with
 *     atomics: zero them (hipMemsetAsync) before the producing launch.
 *   - transform-on-load modes (tf_mode): 0 none, 1 affine, 2 affine+ReLU, 3 affine+GELU(erf),
 *     4 LayerNorm (rowstat = (rows,2) mean,rstd).  They replace materialised BatchNorm /
 *     LayerNorm / activation tensors of the reference graph.
 */
#ifndef HRFUSER_HIP_H_
#define HRFUSER_HIP_H_

/* Cross-block reductions (BatchNorm moments, LayerNorm / depthwise parameter gradients).
 * Same-address global atomics serialise at ~25 ns each on MI355X (measured: 512 blocks -> 13.5 us),
 * so every accumulator that many blocks add into is REPLICATED: a block adds into copy
 * (block index % HRF_STAT_COPIES) and the (tiny) consumer kernel sums the copies.
 *   - every `stats` / `gstats` argument points to [HRF_STAT_COPIES][2*C] doubles (zeroed by the caller);
 *   - hrf_ln_bwd / hrf_dwconv_bwd_weight take `copy_stride`: element distance between the copies of
 *     their fp32 parameter-gradient accumulators (0 = one copy, plain accumulation into the grads);
 *     hrf_fold_copies adds the summed copies into the gradient arena.
 * 4 copies: every block of a CONSUMER launch re-reads all copies in its finalize-on-load prologue (below), and the request
 * count on those hot cache lines is what that prologue costs (tools/bench_fin.py: +0.5 us per consumer launch at 4 copies, +1.0 at
 * 8, +2.0 at 16, +4.5 ... 11 at 32).  Same-box A/B of the captured training steps (tools/ab_copies.sh, ab_copies_models.sh):
 * round 2: 16 copies 17.20 ms, 8: 16.70, 4: 16.64, 2: 17.1, 1: 18.3; round 5 (kernels 30 % shorter, the prologue a larger share):
 * HRFuser-T 32 copies 16.14 ms, 16: 12.58, 8: 11.61, 4: **11.47**, 2: 11.54; STF 8: 23.63, 4: 23.39; HRFuser-B 8: 42.98, 4: 42.98. */
#ifndef HRF_STAT_COPIES      /* (a build may override it: tools/ab_copies.sh) */
#define HRF_STAT_COPIES 4
#endif

/* BatchNorm finalize ON LOAD (consumer side).  A train-mode BatchNorm needs its batch moments complete before anything
 * can be normalised, i.e. a grid-wide dependency between the producing convolution and its consumer; the kernel boundary
 * between the two already is that dependency.  A consumer kernel that is handed one of these for an input tensor derives
 * the scale/shift of that BatchNorm itself, in its prologue, from the producer's replicated moments `stats`
 * ([HRF_STAT_COPIES][2*C] doubles) - the arithmetic of hrf_bn_finalize, evaluated redundantly by every block (C <=
 * HRF_FIN_MAXC) - so the ~330 separate hrf_bn_finalize launches of a training step (and their launch boundaries on the
 * dependency chain) disappear.  `write` != 0: block 0 of the launch also stores scale/shift/mean/invstd (read by the
 * backward kernels) and updates the running statistics; exactly one consumer launch per BatchNorm and step sets it.
 * hrf_bn_bfin_t is the backward counterpart: the data-gradient kernel of the PRODUCING convolution derives the
 * BatchNorm-backward coefficients (dy = cA*du + cB*y + cC) from `gstats` = replicated (sum du, sum du*y); `write` != 0:
 * block 0 stores cA/cB/cC (read by the weight-gradient kernel) and adds dgamma / dbeta. */
#define HRF_FIN_MAXC 576
/* The packed-weight 3x3 engine (csrc/conv3x_engine.hip) stages per-channel coefficients - finalised on load OR handed in as
 * arrays - in a smaller LDS array: hrf_conv_fwd_packed / hrf_conv_bwd_data_packed take a transform on load (tf_mode != 0) /
 * a BatchNorm backward on load (cA != NULL) only up to this many coefficient channels (Cin forward, Cout backward). */
#define HRF_C3X_MAXC 256
typedef struct hrf_bn_fin {
  const double* stats;
  const float* gamma; const float* beta; float* running_mean; float* running_var;
  float* scale; float* shift; float* mean; float* invstd;
  double count; float eps; float momentum; int update_running; int write; int C;
  int copies;                    /* replication of `stats`: 0 = HRF_STAT_COPIES; 1 = already folded (SyncBN: the packed,
                                    all-reduced moments of hrf_bn_pack) */
  const double* count_ptr;       /* nullable: the sample count read from the DEVICE instead of `count` - SyncBN all-reduces
                                    the ranks' row counts with the moments (hrf_bn_pack `rows`), so ranks with unequal
                                    batches normalise by the true global count, as torch.nn.SyncBatchNorm does */
} hrf_bn_fin_t;
typedef struct hrf_bn_bfin {
  const double* gstats;
  const float* gamma; const float* mean; const float* invstd;
  float* dgamma; float* dbeta; float* cA; float* cB; float* cC;
  double count; int train; int write; int C;
  int copies;                    /* as in hrf_bn_fin_t */
  const double* gstats_local;    /* SyncBN: this rank's folded moments (parameter gradients); NULL = gstats */
  float pgrad_scale;             /* gstats_local == NULL: dgamma / dbeta += pgrad_scale * (value from gstats); 0 means 1.
                                    SyncBN without a rank-local copy: the all-reduced sums give the GLOBAL dgamma / dbeta,
                                    every rank adds 1/world of it and the gradient all-reduce restores the sum */
  const double* count_ptr;       /* as in hrf_bn_fin_t */
} hrf_bn_bfin_t;

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense convolution / Linear engine (fp32 MFMA implicit GEMM) -------------------------
 * Replaces F.conv2d(k=1|3, groups=1) and F.linear:
 *   stems hrnet.py:341-358, hrfuser_hrformer_based.py:380-396; Bottleneck resnet.py:166-205;
 *   transitions hrnet.py:430-459; CrossFFN 1x1 hrformer.py:268,280; fuse 1x1
 *   hrformer.py:511-517,544-551; qkv/out_proj hrformer.py:84,86; q/k/v/out_proj
 *   hrfuser_hrformer_based.py:92-96.  Linear = 1x1 conv over a (1,1,rows,C) view.            */
int hrf_conv_fwd(const float* x, int sB, int sY, int sX, int sC, int B, int H, int W, int Cin,
                 const float* w, const float* bias, int KH, int stride, int Cout,
                 float* y, int ldY, int yoff, const float* res, const float* res2, int ldR,
                 int tf_mode, const float* tf_scale, const float* tf_shift,
                 const float* tf_rowstat, double* stats, const hrf_bn_fin_t* tf_fin, float* ln_rowstat, float ln_eps, void* stream);
/* The same forward with a SPLIT OVER K for deep contractions that leave the chip empty (3x3, K = 9*Cin >= 1024, <= 128 row blocks:
 * the 256 -> 36 stride-2 transition, hrnet.py:430-459): four K slices write partial tiles (slice 0 into y, the others into
 * `scratch`), a second launch adds them in a fixed order (bit-reproducible) and takes the moments.
 * hrf_conv_fwd_split_scratch -> floats of scratch this problem wants (0: it would not be split - call hrf_conv_fwd);
 * hrf_conv_fwd_split with scratch == NULL is hrf_conv_fwd. */
long hrf_conv_fwd_split_scratch(int sB, int sY, int sX, int sC, int B, int H, int W, int Cin, int KH, int stride, int Cout,
                                int ldY, int yoff);
int hrf_conv_fwd_split(const float* x, int sB, int sY, int sX, int sC, int B, int H, int W, int Cin,
                       const float* w, const float* bias, int KH, int stride, int Cout,
                       float* y, int ldY, int yoff, const float* res, const float* res2, int ldR,
                       int tf_mode, const float* tf_scale, const float* tf_shift,
                       const float* tf_rowstat, double* stats, const hrf_bn_fin_t* tf_fin, float* ln_rowstat, float ln_eps,
                       float* scratch, void* stream);
/* dX (or, epi=1, dU = dX*act'(scale*xraw+shift) plus (sum dU, sum dU*xraw) for the producer BN).
 * (cA,cB,cC) != NULL applies the BatchNorm backward on load: dy = cA*du + cB*yraw + cC; with `bfin` (nullable, Cout <=
 * HRF_FIN_MAXC) the coefficients are derived in the kernel prologue from bfin->gstats instead of being read (see
 * hrf_bn_bfin_t).  `tf_fin` of hrf_conv_fwd (nullable, tf_mode 1..3, Cin <= HRF_FIN_MAXC) is the forward analogue.    */
int hrf_conv_bwd_data(const float* dy, int ldD, int doff, const float* yraw,
                      const float* cA, const float* cB, const float* cC, const hrf_bn_bfin_t* bfin,
                      const float* w, int KH, int stride, int Cout,
                      int B, int H, int W, int Cin,
                      float* dx, int sB, int sY, int sX, int sC, int accumulate,
                      int epi, const float* xraw, int ldXr, const float* tf_scale,
                      const float* tf_shift, int act, double* stats, void* stream);
/* hrf_conv_bwd_data (same arguments, the same dx / `stats` moments / bfin publication, bit for bit) that ALSO accumulates the
 * weight / bias gradient of the same convolution - dw[Cout][Cin] +=, dbias[Cout] += (nullable), what hrf_conv_bwd_weight adds
 * for these operands - from the rows the data-gradient kernel holds in registers anyway: no second pass over dy, no leaf launch.
 * The forward input of the convolution is `x` rows ([B*H*W][ldX], read when epi == 0) or, with epi == 1,
 * act(tf_scale * xraw + tf_shift) of the rows the epilogue reads.  dw / dbias: fp32 atomics (zero or pre-load the targets);
 * copy_stride > 0: [HRF_STAT_COPIES] replicated accumulators that far apart (see above; for launches of many row blocks),
 * folded by hrf_fold_copies; 0: plain accumulation.  Deterministic mode: registered accumulators, as hrf_conv_bwd_weight.
 * Taken for KH = 1, stride 1, dense NHWC rows (sC = 1, sX = Cin, sY = W*sX, sB = H*sY) on the register-only row-GEMM route when
 * hrf_conv_bwd_data_weight_supported(Cin, Cout, rows = B*H*W, epi, bnb = (cA != NULL)) says 1 (a query: launches nothing) -
 * Cout <= 48 with a BatchNorm backward on load (CrossFFN fc3 of narrow branches), 48 < Cout <= 160 without one (out_proj),
 * and a shape the LDS-tiled route of hrf_conv_bwd_data does not claim.  Every other call returns HRF_ERR_ARG before anything is
 * launched or written: the caller issues hrf_conv_bwd_data and hrf_conv_bwd_weight. */
int hrf_conv_bwd_data_weight_supported(int Cin, int Cout, long rows, int epi, int bnb);
int hrf_conv_bwd_data_weight(const float* dy, int ldD, int doff, const float* yraw,
                             const float* cA, const float* cB, const float* cC, const hrf_bn_bfin_t* bfin,
                             const float* w, int KH, int stride, int Cout,
                             int B, int H, int W, int Cin,
                             float* dx, int sB, int sY, int sX, int sC, int accumulate,
                             int epi, const float* xraw, int ldXr, const float* tf_scale,
                             const float* tf_shift, int act, double* stats,
                             const float* x, int ldX, float* dw, float* dbias, long copy_stride, void* stream);
/* dW += , dbias += (split-K over pixels, fp32 atomics: zero or pre-load the targets).          */
int hrf_conv_bwd_weight(const float* dy, int ldD, int doff, const float* yraw,
                        const float* cA, const float* cB, const float* cC,
                        const float* x, int sB, int sY, int sX, int sC,
                        int B, int H, int W, int Cin, int KH, int stride, int Cout,
                        int tf_mode, const float* tf_scale, const float* tf_shift,
                        const float* tf_rowstat, float* dw, float* dbias, void* stream);

/* ---- the front-end 3x3 convolutions on tap-major PACKED weights (csrc/conv3x_engine.hip) ----------------------------------
 * The stems' second convolution, the Bottleneck conv2 of layer1 and transition1 (hrnet.py:341-358,417-459;
 * resnet.py:263-302; hrfuser_hrformer_based.py:380-396) are the FLOP carriers of the backbone.  Their kernels want the weights
 * as wp[tap][n][k] (a K step = one contiguous run per output channel; backward-data = the same kernel on the transposed pack):
 *   hrf_conv3x_pack_size  floats of one pack: 9 * Np * Kp, N rounded up to 64, K to 32 (zero rows / columns past the tensor);
 *   hrf_conv3x_pack       ONE launch (per 16 jobs) packs any number of OIHW tensors w = [Cout][Cin][3][3]:
 *                         dir 0 (forward operand, N = Cout, K = Cin):        wp[tap][n][k] = w[n][k][tap]
 *                         dir 1 (backward-data operand, N = Cin, K = Cout):  wp[tap][n][k] = w[k][n][tap]
 *                         `jobs` is a HOST array; the packs are caller-owned scratch, refreshed whenever w changes (once per step);
 *   hrf_conv3x_supported  1 when hrf_conv_fwd_packed (dir 0) / hrf_conv_bwd_data_packed (dir 1) take the SHAPE:
 *                         KH = 3; dir 0: stride 1 or 2, Cout > 32; dir 1: stride 1, Cin > 32, or stride 2, Cin > 32 and
 *                         Cout <= 64.  (The shape only: the coefficient bound below depends on the call's other arguments.)
 *   hrf_conv_fwd_packed / hrf_conv_bwd_data_packed: hrf_conv_fwd / hrf_conv_bwd_data (same arguments, same results) with
 *                         `wp` = the pack of `w` in the matching direction, on dense NHWC rows.  A call is TAKEN when
 *                         hrf_conv3x_supported says 1 AND its per-channel coefficients fit the kernel's staging array:
 *                           forward:  tf_mode == HRF_TF_NONE or Cin  <= HRF_C3X_MAXC (tf_fin and tf_scale / tf_shift alike;
 *                                     HRF_TF_LN is never taken),
 *                           backward: cA == NULL             or Cout <= HRF_C3X_MAXC (bfin and cA / cB / cC arrays alike).
 *                         Every other call returns HRF_ERR_ARG before anything is launched - the caller goes through
 *                         hrf_conv_fwd / hrf_conv_bwd_data, which take any width on the array route and up to HRF_FIN_MAXC
 *                         channels on the finalise-on-load route. */
typedef struct hrf_conv3x_pack_job {
  const float* w; float* wp;
  int Cout, Cin, dir;
} hrf_conv3x_pack_job_t;
long hrf_conv3x_pack_size(int Cout, int Cin, int dir);
int hrf_conv3x_pack(const hrf_conv3x_pack_job_t* jobs, int n, void* stream);
int hrf_conv3x_supported(int Cin, int Cout, int KH, int stride, int dir);
int hrf_conv_fwd_packed(const float* x, int sB, int sY, int sX, int sC, int B, int H, int W, int Cin,
                        const float* w, const float* bias, int KH, int stride, int Cout,
                        float* y, int ldY, int yoff, const float* res, const float* res2, int ldR,
                        int tf_mode, const float* tf_scale, const float* tf_shift,
                        const float* tf_rowstat, double* stats, const hrf_bn_fin_t* tf_fin, float* ln_rowstat, float ln_eps,
                        const float* wp, void* stream);
int hrf_conv_bwd_data_packed(const float* dy, int ldD, int doff, const float* yraw,
                             const float* cA, const float* cB, const float* cC, const hrf_bn_bfin_t* bfin,
                             const float* w, int KH, int stride, int Cout,
                             int B, int H, int W, int Cin,
                             float* dx, int sB, int sY, int sX, int sC, int accumulate,
                             int epi, const float* xraw, int ldXr, const float* tf_scale,
                             const float* tf_shift, int act, double* stats, const float* wp, void* stream);

/* The weight gradient of the LARGE 3x3 problems (the stems' 64 -> 64 convolutions, transition1: >= 16 384 output pixels, >= 32 input
 * channels, NHWC rows, no bias gradient) on the LDS-staged 32x32x2 kernel of csrc/wgrad3x_engine.hip: the pixel splits leave their
 * sums as plain stores in caller-owned scratch, a second small launch of the same call folds them into dw (no atomics: bit-
 * reproducible).  hrf_conv_bwd_weight_scratch -> floats of scratch the problem wants (0: it would not use any - call
 * hrf_conv_bwd_weight); hrf_conv_bwd_weight_s = hrf_conv_bwd_weight with that scratch (contents irrelevant; NULL, or a problem
 * that wants none: plain hrf_conv_bwd_weight).  Launches at once, also between hrf_wgrad_group_begin / _end. */
long hrf_conv_bwd_weight_scratch(int sB, int sY, int sX, int sC, int B, int H, int W, int Cin, int KH, int stride, int Cout,
                                 int tf_mode, int has_bias);
int hrf_conv_bwd_weight_s(const float* dy, int ldD, int doff, const float* yraw,
                          const float* cA, const float* cB, const float* cC,
                          const float* x, int sB, int sY, int sX, int sC,
                          int B, int H, int W, int Cin, int KH, int stride, int Cout,
                          int tf_mode, const float* tf_scale, const float* tf_shift,
                          const float* tf_rowstat, float* dw, float* dbias, float* scratch, void* stream);

/* ---- depthwise 3x3 convolution, pad 1, stride 1|2, NHWC (F.conv2d groups=C) -----------------
 * CrossFFN hrformer.py:271-277 (bias, stride 1, input = GELU(BN(h1)) applied on load) and the
 * fuse-down chains hrformer.py:532-541 (stride 2, no bias).  w is (C,1,3,3).                    */
int hrf_dwconv_fwd(const float* x, int B, int H, int W, int C, const float* w, const float* bias,
                   int stride, int tf_mode, const float* tf_scale, const float* tf_shift, float* y,
                   double* stats, const hrf_bn_fin_t* tf_fin, void* stream);
int hrf_dwconv_bwd_data(const float* dy, const float* yraw, const float* cA, const float* cB,
                        const float* cC, const hrf_bn_bfin_t* bfin, const float* w, int stride, int B, int H, int W, int C,
                        float* dx, int accumulate, int epi, const float* xraw, const float* tf_scale,
                        const float* tf_shift, int act, double* stats, void* stream);
/* hrf_dwconv_bwd_data (stride 1, epi = 1: the input was act(tf_scale*xraw+tf_shift)) that ALSO accumulates the weight /
 * bias gradient of the same convolution (what hrf_dwconv_bwd_weight computes from dy, yraw, x = act(.)): dW[ky][kx] =
 * sum_p x[p]*dy'[p-(ky-1,kx-1)] uses the staged dy' element dx[p] needs anyway, and x[p] is a by-product of act'.
 * dw / dbias (nullable bias): [HRF_STAT_COPIES] replicated fp32 accumulators, `copy_stride` apart (see above). */
int hrf_dwconv_bwd_data_weight(const float* dy, const float* yraw, const float* cA, const float* cB,
                               const float* cC, const hrf_bn_bfin_t* bfin, const float* w, int B, int H, int W, int C,
                               float* dx, const float* xraw, const float* tf_scale, const float* tf_shift, int act,
                               double* stats, float* dw, float* dbias, long copy_stride, void* stream);
int hrf_dwconv_bwd_weight(const float* dy, const float* yraw, const float* cA, const float* cB,
                          const float* cC, const float* x, int B, int H, int W, int C, int stride,
                          int tf_mode, const float* tf_scale, const float* tf_shift, float* dw,
                          float* dbias, long copy_stride, void* stream);

/* ---- 7x7 windowed attention core (per window x head: q k^T*d^-1/2 + RPB, softmax, @v) --------
 * WindowMSA hrformer.py:103-128 / WindowMCA hrfuser_hrformer_based.py:115-148 incl. the centre
 * zero-pad, window partition/merge and de-pad of hrformer.py:196-236 / hrfuser...:202-248 as
 * index math.  q/k/v/o are (B*H*W, ld) NHWC projections with column offsets (packed qkv = one
 * buffer, three offsets).  kpad/vpad (C) = key/value of a padded token (the projection biases);
 * padded keys are attended, not masked (with_pad_mask=False).  head_dim in {8,16,18,32,39}.
 * bwd: dq/dk/dv written for every real token; dkpad/dvpad/drpb accumulate (+=, atomics).        */
int hrf_window_attn_fwd(const float* q, int ldq, int qoff, const float* k, int ldk, int koff,
                        const float* v, int ldv, int voff, const float* kpad, const float* vpad,
                        const float* rpb, float* o, int ldo, int B, int H, int W, int C, int heads,
                        void* stream);
int hrf_window_attn_bwd(const float* q, int ldq, int qoff, const float* k, int ldk, int koff,
                        const float* v, int ldv, int voff, const float* kpad, const float* vpad,
                        const float* rpb, const float* dout, int lddo,
                        float* dq, int lddq, int dqoff, float* dk, int lddk, int dkoff,
                        float* dv, int lddv, int dvoff, float* dkpad, float* dvpad, float* drpb, long copy_stride,
                        int B, int H, int W, int C, int heads, void* stream);

/* ---- per-head window attention forward with LayerNorm and the q / k / v projections in the kernel ----------------------
 * o = attention core of hrf_window_attn_fwd applied to q = LN_q(xq) wq^T + bq, k = LN_kv(xkv) wk^T + bk, v = LN_kv(xkv) wv^T +
 * bv in ONE launch of windows x heads workgroups: what the per-op chain runs as hrf_conv_fwd(tf_mode = LayerNorm on load) into
 * a projection buffer + hrf_window_attn_fwd.  xq / xkv: (B*H*W, C) NHWC rows; xkv == xq: self-attention (LN_kv / rowstat_kv
 * unused).  rowstat_*: the [rows][2] (mean, rstd) LayerNorm statistics of the rows (hrf_ln_stats or a producer's epilogue).
 * wq / wk / wv: [C][C] row-major Linear weights (possibly rows of one packed Linear), biases nullable.  A padded token is an
 * exact zero AFTER LayerNorm, so its key / value is the projection bias, attended and not masked.  o: (B*H*W, ldo).
 * q_out / k_out / v_out (each nullable; (rows, ld) with a column offset as in hrf_window_attn_fwd): the UNscaled q and the k /
 * v rows of the real tokens, exactly what hrf_window_attn_bwd and the projections' backward read - a training forward.
 * hrf_window_attn_proj_supported: C == head_dim * heads, head_dim in {18, 39}, C <= 160.  Never allocates or synchronises;
 * an unsupported width, a NULL required pointer or cross-attention without rowstat_kv / LN_kv: HRF_ERR_ARG before any launch. */
typedef struct hrf_attn_proj {
  int B, H, W, C, heads;
  const float* xq; const float* xkv;
  const float* lnq_g; const float* lnq_b; const float* lnkv_g; const float* lnkv_b;
  const float* rowstat_q; const float* rowstat_kv;
  const float* wq; const float* bq; const float* wk; const float* bk; const float* wv; const float* bv;
  const float* rpb;
  float* o; int ldo;
  float* q_out; int ldq, qoff;
  float* k_out; int ldk, koff;
  float* v_out; int ldv, voff;
} hrf_attn_proj_t;
int hrf_window_attn_proj_supported(int C, int heads);
int hrf_window_attn_proj_fwd(const hrf_attn_proj_t* p, void* stream);

/* ---- fused window-attention block (csrc/attn_block.hip): the whole token-local half of an HRFormerBlock
 * (hrformer.py:365-373: norm1 -> LocalWindowSelfAttention :184-236 / WindowMSA :96-131 -> residual -> norm2 -> CrossFFN
 * layers[0] :268) or of one modality of a fusion block (hrfuser_hrformer_based.py:305-317: norm1[k] / norm2[k] ->
 * MultiWindowCrossAttention :189-248 / WindowMCA :106-151 incl. Dropout -> DropPath + residuals; after the last modality
 * norm3 + the CrossFFN head) in ONE launch per direction, one workgroup per 7x7 window; head_dim 18 (HRFuser-T / STF
 * widths 18 / 36 / 72 / 144) and, forward only, head_dim 39 (HRFuser-B / HRFormer-B widths 78 / 156; their 312 / 624 do
 * not fit the LDS): hrf_attn_block_supported.  Rows are NHWC (B*H*W, C); weights keep the reference layouts
 * (Linear (out, in); for the packed qkv Linear pass three pointers into the same tensor).
 *   forward : out = res (+ res2) + mask*mscale*rowscale[b] * out_proj(attn(LN_q(xq), LN_kv(xkv)));  xkv == xq: self-
 *             attention (LN_kv unused).  mask / rowscale / res2 nullable; mscale = 1 when unused.
 *             out_rowstat (nullable): LayerNorm (mean, rstd) of the out rows with out_eps.
 *             w1 != NULL: h1 = LN_2(out) w1^T + b1 (hidden = 4*C rows, pre-BatchNorm) and, stats1 != NULL, its
 *             replicated moments [HRF_STAT_COPIES][2*hidden] (+=).
 *   backward: gout = dL/d out rows; du1 (+ cA1/cB1/cC1, or bfin1 to derive them on load like hrf_conv_bwd_data) = the
 *             gradient reaching h1 through its BatchNorm (dy1 = cA*du1 + cB*h1 + cC).  With gx = gout + (gradient through
 *             LN_2 / w1):  dres (+)= gx;  dq (+)= gradient through LN_q (+ gx when dq_add_res: self-attention, where the
 *             residual row IS the query row);  dkv (+)= gradient through LN_kv (+ gx when dkv_add_res: the modality row
 *             is both residual and key/value source).  Each *_acc flag selects += over =; NULL outputs are skipped.
 *             Parameter gradients are NOT accumulated with atomics: every workgroup writes the complete partial sums of
 *             its window to its own slot pslot[blockIdx * slot_stride + off_*] (plain stores, deterministic);
 *             hrf_fold_slots adds the slots into the gradient arena.  Slot layout (floats; off_* < 0: not produced):
 *             w1 [4C][C], b1 [4C], ln2 gamma / beta [C]; wo [C][C], bo [C]; wq / wk / wv [C][C], bq / bk / bv [C];
 *             LN_q gamma / beta, LN_kv gamma / beta [C].  The relative-position-bias gradient is a leaf: the kernel leaves
 *             dS[key][query] of every (window, head) in ds_plane [windows][heads][49][49]; hrf_rpb_grad (any time later)
 *             gathers it into the replicated accumulator drpb [HRF_STAT_COPIES][169][heads] (copy_stride apart).
 *             hrf_attn_block_bwd_supported: widths 18 / 36 (72 / 144 / 78 / 156 are forward-only: a training step keeps
 *             the per-op kernels there).
 * The last five fields are derived by the library.                                                                     */
typedef struct hrf_attn_block {
  int B, H, W, C, heads;
  const float* xq; const float* xkv;
  const float* lnq_g; const float* lnq_b; const float* lnkv_g; const float* lnkv_b; float ln_eps;
  const float* wq; const float* bq; const float* wk; const float* bk; const float* wv; const float* bv;
  const float* rpb; const float* wo; const float* bo;
  const float* res; const float* res2;
  const float* mask; float mscale; const float* rowscale; int rows_per_sample;
  float* out; float* out_rowstat; float out_eps;
  const float* ln2_g; const float* ln2_b; const float* w1; const float* b1; float* h1; double* stats1; int hidden;
  const float* gout; const float* du1; const float* cA1; const float* cB1; const float* cC1; const hrf_bn_bfin_t* bfin1;
  float* dres; int dres_acc; float* dq; int dq_acc; int dq_add_res; float* dkv; int dkv_acc; int dkv_add_res;
  float* pslot; long slot_stride; float* ds_plane;
  float* gx_park;      /* [windows][64][ceil(C/16)*16] floats of step-lifetime scratch (18-channel backward, 8-wave form; else unused) */
  /* CrossFFN tail of the PRECEDING block formed on load (hrformer.py:371-372 x = x' + DropPath(GELU(BN3(fc3(.)))), self-
   * attention only, tail_raw != NULL): the block input rows are x = tail_res + tail_rowscale[b] * GELU(tail_scale *
   * tail_raw + tail_shift) (tail_fin: scale / shift derived on load from the producer's moments, as hrf_conv_fwd's fin).
   * forward : every workgroup forms the rows of its window and WRITES them to x_out (== xq == xkv == res: the block's
   *           residual and, in the backward, its recomputation source).
   * backward: with dx = the block-input gradient (what dq receives; dq_add_res = 1): tail_du = dx * rowscale * GELU'(u),
   *           tail_gstats [HRF_STAT_COPIES][2*C] += (sum tail_du, sum tail_du * tail_raw): the hrf_act_bwd launch of the
   *           preceding block's BatchNorm is gone; tail_scale / tail_shift must be in memory (published by the forward). */
  const float* tail_res; const float* tail_raw; const float* tail_scale; const float* tail_shift; const float* tail_rowscale;
  const hrf_bn_fin_t* tail_fin; float* x_out; float* tail_du; double* tail_gstats;
  int off_w1, off_b1, off_g2, off_bt2, off_wo, off_bo, off_wq, off_bq, off_wk, off_bk, off_wv, off_bv;
  int off_gq, off_btq, off_gkv, off_btkv, off_rpb;
  int nWh, nWw, pt, pl; float scale;
} hrf_attn_block_t;
int hrf_attn_block_supported(int C, int heads);
int hrf_attn_block_bwd_supported(int C, int heads);
int hrf_attn_block_fwd(const hrf_attn_block_t* p, void* stream);
int hrf_attn_block_bwd(const hrf_attn_block_t* p, void* stream);
int hrf_rpb_grad(const float* ds_plane, int nwin, int heads, float* drpb, long copy_stride, void* stream);

/* ---- eval-mode CrossFFN in one launch (csrc/ffn_eval.hip) ---------------------------------------------------------------
 * out = x + GELU(BN3(fc3( GELU(BN2(dw3x3( GELU(BN1(fc1( LN(x) ))) ))) ))) with FROZEN BatchNorm statistics: the second half
 * of an HRFormerBlock / HRFuserFusionBlock in eval mode - hrformer.py:351 (norm2), :267-295 (CrossFFN.forward), :371-372
 * (residual; DropPath is the identity) resp. hrfuser_hrformer_based.py:291,315-316.  x, out: (B,H,W,C) NHWC fp32; w1 [hidden][C]
 * + b1, wd [hidden][3][3] + bd, w3 [C][hidden] + b3 in their Conv2d layouts; (s_k, t_k) = the frozen-statistics affine of
 * BatchNorm k (scale = gamma * rsqrt(running_var + eps), shift = beta - running_mean * scale).  hidden = 4 C;
 * hrf_ffn_eval_supported: C in {18, 36} (the two finest branches of HRFuser-T / STF, where a launch has hundreds of tiles);
 * other widths keep the per-op kernels.  The 4C-wide hidden tensor never leaves the chip.                                   */
typedef struct hrf_ffn_eval {
  int B, H, W, C, hidden;
  const float* x;
  const float* ln_g; const float* ln_b; float ln_eps;
  const float* w1; const float* b1; const float* s1; const float* t1;
  const float* wd; const float* bd; const float* s2; const float* t2;
  const float* w3; const float* b3; const float* s3; const float* t3;
  float* out;
} hrf_ffn_eval_t;
int hrf_ffn_eval_supported(int C, int hidden);
int hrf_ffn_eval(const hrf_ffn_eval_t* p, void* stream);

/* ---- eval-mode Bottleneck in one launch (csrc/hrf_bneck_eval.h, part of csrc/conv3x_engine.hip) --------------------------
 * resnet.py:263-302 with every BatchNorm FROZEN (eval mode / norm_eval: running statistics as a per-channel affine):
 *   y1  = ReLU(s1 * conv1x1(x;  w1 [planes][Cin])        + t1)
 *   y2  = ReLU(s2 * conv3x3(y1; w2, pad 1, stride 1)     + t2)
 *   idt = has_downsample ? sd * conv1x1(x; wd [4 planes][Cin]) + td : x
 *   out = ReLU(s3 * conv1x1(y2; w3 [4 planes][planes])   + t3 + idt)
 * x: (B,H,W,Cin), out: (B,H,W,4 planes), dense NHWC fp32.  No convolution has a bias; w1, w3, wd in their Conv2d layouts, w2 =
 * the direction-0 tap-major pack of hrf_conv3x_pack (wp[tap][n][k]); (s_k, t_k) = the frozen-statistics affine of BatchNorm k
 * (scale = gamma * rsqrt(running_var + eps), shift = beta - running_mean * scale), applied in the epilogues - nothing derived
 * from the weights is cached.  y1 at a halo position outside the image is zero (the padding of conv2).  Neither 64-channel
 * intermediate leaves the chip.  hrf_bottleneck_eval_supported: planes == 64 and (Cin == 256 without, Cin == 64 with the
 * downsample) - the two blocks of layer1 of every reference config; anything else, a null required pointer (wd / sd / td are
 * required with the downsample only) or B / H / W < 1: HRF_ERR_ARG before anything is launched.                          */
typedef struct hrf_bottleneck_eval {
  int B, H, W, Cin, planes, has_downsample;
  const float* x;
  const float* w1; const float* s1; const float* t1;
  const float* w2; const float* s2; const float* t2;
  const float* w3; const float* s3; const float* t3;
  const float* wd; const float* sd; const float* td;
  float* out;
} hrf_bottleneck_eval_t;
int hrf_bottleneck_eval_supported(int Cin, int planes, int has_downsample);
int hrf_bottleneck_eval(const hrf_bottleneck_eval_t* p, void* stream);

/* ---- multi-level RoIAlign: SingleRoIExtractor forward / backward (csrc/hrf_roi.h, part of csrc/pointwise.hip) --------------
 * What every reference config does with the pyramid (configs/_base_/models/cascade_rcnn_hrfuser_fpn_*_fusion.py:152-156,
 * once per cascade stage): SingleRoIExtractor.forward (mmdet/models/roi_heads/roi_extractors/single_level_roi_extractor.py:
 * 57-108) = map_roi_levels (:36-55) + mmcv.ops.RoIAlign(output_size 7, sampling_ratio 0, pool_mode 'avg', aligned True) per
 * level, and their autograd backward.  ONE launch serves all levels: the kernel derives each box's level itself -
 *   scale = sqrt((x2 - x1) * (y2 - y1)),  lvl = clamp(floor(log2(scale / finest_scale + 1e-6)), 0, num_levels - 1)
 * in fp32 (the log2 as comparisons against 2, 4, 8), num_levels == 1: level 0 for every box (:76-79) - so there is no host read
 * of `rois`, no sort, no nonzero, no allocation, no synchronisation: the calls can be captured in a hipGraph.
 *   feat[l]   the maps of one pyramid, NHWC fp32 [B][H_l][W_l] rows of pitch ld_l >= C floats (the HRFPN outputs in place);
 *   rois      [K][5] fp32 on the device: (batch index, x1, y1, x2, y2) in image pixels, unscaled;
 *   out       out_layout 0: [K][C][7][7] (the reference's order), 1: [K][7][7][C]; every row is written;
 *   dfeat[l]  backward only, same shape and pitch as feat[l]: "+=" with fp32 atomics - the caller zeroes it, or it already
 *             holds another consumer's gradient; a level no box maps to is not touched.  The box coordinates get no gradient
 *             (as in mmcv).  The reference's `feats[i].sum() * 0.` term (DDP graph completeness) has no counterpart.
 * Per level: x1' = x1 * spatial_scale - 0.5 (likewise y1', x2', y2'), rw = x2' - x1' (no clamp to 1), bin = rw / 7,
 * grid = ceil(rw / 7), sample (ix) of bin pw at x1' + pw * bin + (ix + 0.5) * bin / grid; a sample outside [-1, W] (or
 * [-1, H]) contributes 0, otherwise it is clamped to >= 0 and read bilinearly with the last row / column repeated; a bin is
 * the sum of its samples / max(grid_h * grid_w, 1); a box with grid_h <= 0 or grid_w <= 0 produces zeros.  The sample
 * positions are evaluated in fp64 (mmcv: fp32), the sums in fp32.
 * DELIBERATE DEVIATION (the coordinates are unvalidated device data; trip counts are bounded by the map, never by the box): a
 * box with a coordinate that is not finite, with |coordinate * spatial_scale| > HRF_ROI_COORD_MAX, or with a batch index outside
 * [0, B) gives a row of zeros forward and contributes nothing backward (the reference reads out of bounds or returns garbage).
 * For every other box the sample loops are clipped to the samples that can fall inside the map: at most
 * 2 n + HRF_ROI_AXIS_SLACK sample iterations per axis of n pixels and box, whatever the box is.
 * hrf_roi_align_supported(C, pooled, num_levels): C % 4 == 0, 4 <= C <= HRF_ROI_MAX_C, pooled == 7, 1 <= num_levels <=
 * HRF_ROI_MAX_LEVELS.  Anything else - also `pooled` of the struct != 7, B / H_l / W_l < 1, ld_l < C, a null map, an out_layout
 * other than 0 / 1, maps whose weight tables do not fit the LDS (H_l + W_l beyond ~3 700 at C = 256) - is HRF_ERR_ARG before
 * any launch.  K == 0: HRF_OK, no launch.
 * hrf_roi_align_fwd has no atomics: bit-reproducible in any mode.  hrf_roi_align_bwd is REFUSED in deterministic mode (below).   */
#define HRF_ROI_MAX_LEVELS 4
#define HRF_ROI_MAX_C 256
#define HRF_ROI_COORD_MAX 1048576.0f
#define HRF_ROI_AXIS_SLACK 40
typedef struct hrf_roi_levels {
  int num_levels, C, B;
  const float* feat[HRF_ROI_MAX_LEVELS];
  float* dfeat[HRF_ROI_MAX_LEVELS];
  int H[HRF_ROI_MAX_LEVELS];
  int W[HRF_ROI_MAX_LEVELS];
  int ld[HRF_ROI_MAX_LEVELS];
  float spatial_scale[HRF_ROI_MAX_LEVELS];
  float finest_scale;
  int pooled;                    /* output_size: 7 */
} hrf_roi_levels_t;
int hrf_roi_align_supported(int C, int pooled, int num_levels);
int hrf_roi_align_fwd(const hrf_roi_levels_t* lv, const float* rois, int K, float* out, int out_layout, void* stream);
int hrf_roi_align_bwd(const hrf_roi_levels_t* lv, const float* rois, int K, const float* dout, int out_layout, void* stream);

/* ---- RPN proposal generation: top-k + decode, per-level NMS, merge (csrc/hrf_rpn.h, part of csrc/pointwise.hip) ------------
 * The producer of the `rois` above: what RPNHead.get_bboxes does at test time with the head's two maps per level
 * (mmdet/models/dense_heads/base_dense_head.py:32-108, rpn_head.py:103-235, anchor_generator.py:241-281,
 * delta_xywh_bbox_coder.py:164-260 with means 0 / stds 1, mmcv 1.3.17 batched_nms with the level as the class id), as FOUR
 * launches with fixed-shape outputs: no host read of an input, no allocation, no synchronisation, no float atomics (the same
 * bits in deterministic mode), every loop bounded by a map size or HRF_RPN_MAX_PRE - capturable in a hipGraph.  Logits and
 * deltas are unvalidated device data and may be NaN / Inf.
 *   cls[l]     objectness logits (use_sigmoid: one per anchor), NHWC fp32 [B][H_l][W_l] rows of pitch ld_cls_l >= A floats;
 *   reg[l]     deltas (dx, dy, dw, dh) per anchor, NHWC fp32 [B][H_l][W_l] rows of pitch ld_reg_l >= 4 A floats;
 *              the flat anchor index of a level is (y * W + x) * A + a, the order of permute(1, 2, 0).reshape(-1);
 *   stride[l]  anchor stride of the level; base_anchors[(l * HRF_RPN_MAX_ANCHORS + a) * 4 ..] = (x1, y1, x2, y2) of base anchor a
 *              (AnchorGenerator.gen_single_level_base_anchors, computed by the caller); anchor = base + (x, y, x, y) * stride;
 *   img_shape  [B][2] fp32 on the device: (height, width) every box of image b is clipped to; read at run time - a captured
 *              graph follows a changed array;
 *   cfg        nms_pre (1 .. HRF_RPN_MAX_PRE), max_per_img (>= 1), iou_thr in (0, 1], min_bbox_size >= 0.
 * Stage 1 (hrf_rpn_select_decode), per (image, level): the k_l = min(nms_pre, H_l W_l A) anchors of largest RAW logit in
 * descending order - sigmoid is monotone; equal logits: lower flat index first; -0 == +0; a NaN logit ranks below every number -
 * are decoded (delta2bbox in its written fp32 order, dw / dh clamped to +-|log(16 / 1000)|, clipped to the image) into
 *   cand       [B][K][5] fp32, K = sum_l k_l, level l of image b at rows b * K + sum_{j<l} k_j ..: (x1, y1, x2, y2, logit);
 *   valid      [B][K] int32: 1 when w > min_bbox_size && h > min_bbox_size (a NaN box fails) and the logit is not NaN
 *              (DEVIATION: the reference keeps a NaN score); idx (nullable) [B][K] int32: the flat anchor index of each row.
 * Stages 2 + 3 (hrf_nms_segments, usable for any per-segment NMS): `cand` / `valid` (nullable: all valid) as above for nseg
 * segments per image of seg_len[s] rows (a HOST array, 0 <= seg_len[s] <= HRF_RPN_MAX_PRE, nseg <= HRF_RPN_MAX_LEVELS), every
 * segment in descending score order (the merge relies on it).  Greedy NMS in row order within a segment: row j is dropped when an
 * earlier KEPT row i has iou > iou_thr, with area = (x2-x1)*(y2-y1), iw = max(min(x2i,x2j) - max(x1i,x1j), 0), ih likewise,
 * inter = iw*ih, iou = inter / (area_i + area_j - inter) in fp32 in exactly this order; invalid rows are never kept and
 * suppress nothing; segments are independent (mmcv's coordinate-offset form of that is not reproduced).  The kept rows of an
 * image are ordered by score descending - ties: lower segment, then lower row - and the first max_per_img become
 *   dets       [B][max_per_img][5] fp32 (x1, y1, x2, y2, apply_sigmoid ? 1 / (1 + exp(-score)) : score), rows past count[b] zero;
 *   count      [B] int32;
 *   rois       [B * max_per_img][5] fp32 (b, x1, y1, x2, y2) - bbox2roi's layout, hrf_roi_align_fwd's input - padded rows
 *              (b, 0, 0, 0, 0) (RoIAlign gives them a row of zeros).
 *   workspace  caller-owned device memory of hrf_nms_workspace_bytes / hrf_rpn_workspace_bytes bytes, 256-byte aligned, contents
 *              irrelevant (suppression bit matrices, keep words, counts; for hrf_rpn_proposals also cand / valid).
 * hrf_rpn_proposals = all three on the sigmoid of the logit.  hrf_rpn_supported -> 1 / 0; the *_workspace_bytes return 0 for
 * what is refused.  REFUSED with HRF_ERR_ARG before any launch: nms_pre outside [1, HRF_RPN_MAX_PRE], A outside
 * [1, HRF_RPN_MAX_ANCHORS], num_levels outside [1, HRF_RPN_MAX_LEVELS], a null map or output, H / W / stride / B < 1, a pitch
 * smaller than the row, max_per_img < 1, iou_thr outside (0, 1], a negative min_bbox_size, a workspace that is too small.    */
#define HRF_RPN_MAX_LEVELS 5
#define HRF_RPN_MAX_ANCHORS 3
#define HRF_RPN_MAX_PRE 2048
#define HRF_RPN_ANCHOR_FLOATS 60               /* HRF_RPN_MAX_LEVELS * HRF_RPN_MAX_ANCHORS * 4 */
typedef struct hrf_rpn_levels {
  int num_levels, A, B;
  const float* cls[HRF_RPN_MAX_LEVELS];
  const float* reg[HRF_RPN_MAX_LEVELS];
  int H[HRF_RPN_MAX_LEVELS];
  int W[HRF_RPN_MAX_LEVELS];
  int ld_cls[HRF_RPN_MAX_LEVELS];
  int ld_reg[HRF_RPN_MAX_LEVELS];
  int stride[HRF_RPN_MAX_LEVELS];
  float base_anchors[HRF_RPN_ANCHOR_FLOATS];
} hrf_rpn_levels_t;
typedef struct hrf_rpn_cfg {
  int nms_pre, max_per_img;
  float iou_thr, min_bbox_size;
} hrf_rpn_cfg_t;
int hrf_rpn_supported(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg);
long hrf_rpn_workspace_bytes(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg);
long hrf_nms_workspace_bytes(const int* seg_len, int nseg, int B);
int hrf_rpn_select_decode(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg, const float* img_shape, float* cand, int* valid,
                          int* idx, void* stream);
int hrf_nms_segments(const float* cand, const int* valid, const int* seg_len, int nseg, int B, int max_per_img, float iou_thr,
                     int apply_sigmoid, void* workspace, long workspace_bytes, float* dets, int* count, float* rois, void* stream);
int hrf_rpn_proposals(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg, const float* img_shape, void* workspace,
                      long workspace_bytes, float* dets, int* count, float* rois, void* stream);

/* ---- RPN training targets and loss (csrc/hrf_rpn_train.h, part of csrc/pointwise.hip) --------------------------------------------
 * What RPNHead.loss does with the head's two maps per level and the ground-truth boxes (mmdet/core/anchor/anchor_generator.py:
 * 392-451, core/anchor/utils.py:21-47, core/bbox/iou_calculators/iou2d_calculator.py:213-253, core/bbox/assigners/
 * max_iou_assigner.py:128-213, core/bbox/samplers/base_sampler.py:83-98 + random_sampler.py:64-82, models/dense_heads/
 * anchor_head.py:239-283 / :383-384 / :402-450 / :498-520, core/bbox/coder/delta_xywh_bbox_coder.py:118-160, rpn_head.py:70-101):
 * inside flags, MaxIoUAssigner (gt_max_assign_all), a random sampler, BCE-with-logits + SmoothL1 and their gradients on the maps.
 * Fixed-shape outputs, no host read of an input, no allocation, no synchronisation, no float atomics (the same bits in
 * deterministic mode and from run to run), every loop bounded by a map size, Gmax or eight radix passes - capturable in a
 * hipGraph.  Boxes, logits and deltas are unvalidated device data and may be NaN / Inf.
 *   lv         the maps and anchors of the proposal entries above, read in place at their pitch.  The anchors of an image form
 *              ONE list of N = sum_l H_l W_l A entries: level l at sum_{j<l} N_j, then (y * W + x) * A + a;
 *   img_shape  [B][2] fp32 (h, w) for the inside flags; pad_shape [B][2] fp32 (h, w) for the valid flags
 *              (valid_h = min(ceil(pad_h / stride), H)); both read at run time;
 *   gt         [B][Gmax][4] fp32 (x1, y1, x2, y2); gt_count [B] int32, clamped to [0, Gmax] in the kernel; both read at run time:
 *              a captured graph follows changed contents.  1 <= Gmax <= HRF_RPN_MAX_GT;
 *   cfg        pos_iou_thr, neg_iou_thr, min_pos_iou in [0, 1]; match_low_quality 0 / 1; allowed_border (< 0: valid flags alone);
 *              num >= 1 samples per image of which at most num_pos (0 .. num) positives; SmoothL1 beta > 0; the two loss weights;
 *   keys       [B][N] uint32 sampling keys, or null: key = hash(rng_state[0] = seed, rng_state[1] = counter, image, n), the
 *              32-bit integer hash written out in csrc/hrf_rpn_train.h.  The sampled positives (negatives) of an image are the
 *              num_pos' = min(P, num_pos) (min(Q, num - num_pos')) assigned positives (negatives) of smallest (key, n): a uniform
 *              subset - the reference's distribution, not its randperm stream.  With null keys hrf_rpn_loss advances the
 *              counter in its last launch (a replayed graph draws fresh samples); hrf_rpn_assign never does;
 *   assigned   [B][N] int32: -2 not inside, -1 ignored, 0 negative, i + 1 matched to gt i;  max_iou [B][N] fp32 (0 when not inside);
 *   sampled    [B][N] int32: +1 sampled positive, -1 sampled negative, 0 neither;
 *   counts     [B][4] int32: assigned positives, assigned negatives, sampled positives, sampled negatives;
 *   grads      d_cls[l] / d_reg[l]: NHWC fp32 [B][H_l][W_l] rows of pitch ld_cls_l >= A / ld_reg_l >= 4 A; the A resp. 4 A leading
 *              floats of EVERY row are written (zero off-sample, no memset needed): d loss_cls_l / d cls and d loss_bbox_l / d reg
 *              with both loss weights and 1 / avg applied, avg = sum_b max(sampled pos_b, 1) + max(sampled neg_b, 1);
 *   losses     [2][num_levels] fp32: loss_cls per level, then loss_bbox per level (sum of the weighted terms / avg * loss weight);
 *   workspace  caller-owned device memory of hrf_rpn_train_workspace_bytes bytes, 256-byte aligned, contents irrelevant.
 * hrf_rpn_assign = everything up to `sampled` (five launches); hrf_rpn_loss = everything (six).  hrf_rpn_train_supported -> 1 / 0,
 * hrf_rpn_train_workspace_bytes -> 0 for what is refused.  REFUSED with HRF_ERR_ARG before any launch: A, num_levels, B, H, W,
 * stride, the map pointers and pitches as for the proposal entries; N >= 2^30; Gmax outside [1, HRF_RPN_MAX_GT]; a threshold
 * outside [0, 1] or NaN; num < 1; num_pos outside [0, num]; |allowed_border| > 2^24; beta <= 0 or not finite; a loss weight that is
 * not finite; a null img_shape / pad_shape / gt / gt_count / output; keys and rng_state both null; a null gradient map or a
 * gradient pitch smaller than the row (hrf_rpn_loss); a workspace that is null or too small.                                   */
#define HRF_RPN_MAX_GT 256
typedef struct hrf_rpn_train_cfg {
  float pos_iou_thr, neg_iou_thr, min_pos_iou;
  int match_low_quality, allowed_border, num, num_pos;
  float beta, loss_weight_cls, loss_weight_bbox;
} hrf_rpn_train_cfg_t;
typedef struct hrf_rpn_grads {
  float* d_cls[HRF_RPN_MAX_LEVELS];
  float* d_reg[HRF_RPN_MAX_LEVELS];
  int ld_cls[HRF_RPN_MAX_LEVELS];
  int ld_reg[HRF_RPN_MAX_LEVELS];
} hrf_rpn_grads_t;
int hrf_rpn_train_supported(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, int Gmax);
long hrf_rpn_train_workspace_bytes(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, int Gmax);
int hrf_rpn_assign(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, const float* img_shape, const float* pad_shape,
                   const float* gt, const int* gt_count, int Gmax, const unsigned* keys, unsigned* rng_state, void* workspace,
                   long workspace_bytes, int* assigned, float* max_iou, int* sampled, int* counts, void* stream);
int hrf_rpn_loss(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, const float* img_shape, const float* pad_shape,
                 const float* gt, const int* gt_count, int Gmax, const unsigned* keys, unsigned* rng_state, void* workspace,
                 long workspace_bytes, int* assigned, float* max_iou, int* sampled, int* counts, const hrf_rpn_grads_t* grads,
                 float* losses, void* stream);

/* ---- Cascade bbox head at test time (csrc/hrf_fc.h in csrc/conv3w_engine.hip; csrc/hrf_bbox.h in csrc/pointwise.hip) ----------
 * What CascadeRoIHead.simple_test does after RoIAlign (mmdet/models/roi_heads/cascade_roi_head.py:288-400, bbox_heads/
 * bbox_head.py:316-378 / :460-497, convfc_bbox_head.py, core/post_processing/bbox_nms.py:8-95, delta_xywh_bbox_coder.py:224-260):
 * the fully connected layers, the box refinement between stages and the final softmax / per-class NMS / top-k.  fp32, test time
 * only.  Every entry validates its arguments (HRF_ERR_ARG before any launch), reads no device data on the host, allocates
 * nothing, never synchronises, uses no float atomics (the same bits in deterministic mode and from run to run), bounds every
 * loop by a size known at launch and can be captured in a hipGraph.
 *
 * hrf_fc  y[m][n] = act(bias[n] + sum_k x[m][k] * wp[n][k]), act = ReLU when relu == 1 (a NaN stays a NaN): a few rows, a deep K.
 *   x [M] rows of pitch ldX >= K (the pad columns are never read), wp [N][K] from hrf_fc_pack (= hrf_rowgemm_pack, dir 0), bias [N]
 *   or null, y [M] rows of pitch ldY >= N.  K % 16 == 0, N % 16 == 0, N <= 65536, 0 <= M <= 2^24; M == 0: HRF_OK, no launch.
 *   fp32 MFMA with hrf_rowgemm's operand precision and tile; the K steps are split over blocks (a function of (M, K, N) alone) so
 *   that M ~ 2000, K = 12544, N = 1024 is 512 blocks, the partial sums go through slots of `workspace`
 *   (hrf_fc_workspace_bytes(M, K, N) bytes, 0 when the shape is not split or refused; caller-owned, contents irrelevant, 16-byte
 *   aligned) and are folded in slot order by a second launch that also applies bias / ReLU.  No atomics, no arrival counters.
 *   REFUSED: K % 16 != 0, N % 16 != 0, K / N < 1, M < 0, a null x / wp / y, ldX < K, ldY < N, relu not 0 / 1, a workspace that
 *   is null or too small when one is needed.
 * hrf_bbox_refine  regress_by_class with reg_class_agnostic: rois_out[r] = (rois_in[r][0], delta2bbox(rois_in[r][1:5],
 *   deltas[r][0:4] * stds, clipped to img_shape[b])), b = rois_in[r][0], in the written fp32 order: deltas * stds first, dw / dh
 *   clamped to +-|log(16 / 1000)|, one expf per side, the clip to [0, w] / [0, h].  deltas: rows of pitch ld_deltas >= 4 (a
 *   column slice of the padded head output); img_shape: the device [B][2] (h, w) array of the RPN entries.  A row whose batch
 *   index is not an integer in [0, B) (also NaN) keeps its first column and gets the box (0, 0, 0, 0) - hrf_roi_align_fwd gives
 *   such a row zeros - and img_shape is never indexed with it.  A padded row (b, 0, 0, 0, 0) stays (b, 0, 0, 0, 0) for finite
 *   deltas.  rois_out may be rois_in.  REFUSED: a null pointer, ld_deltas < 4, B < 1, K < 0, a std that is not positive and finite.
 * hrf_bbox_detect  the last stage's get_bboxes: for row r of image b (rows b * R ..) score = softmax((sum_s logits_s) / S) over
 *   the num_classes + 1 columns (background last; the sum in stage order), box = delta2bbox(rois[r][1:5], deltas[r] * stds)
 *   clipped to img_shape[b] and then, when scale_factor ([B][4], nullable: no rescale) is given, divided by it.  Candidate (r, c),
 *   c < num_classes, is valid iff score > score_thr (a NaN score fails) and r < count[b] (count nullable: all R rows).  Each
 *   (image, class) is put in descending score order (equal scores: lower row) and goes through the greedy NMS of
 *   hrf_nms_segments (same IoU formula and fp32 order; classes are independent, mmcv's coordinate offsets are not reproduced);
 *   the kept rows of an image are merged by score descending - ties: lower class, then lower row - and the first max_per_img are
 *     dets   [B][max_per_img][5] (x1, y1, x2, y2, score), rows past count_out[b] zero;
 *     labels [B][max_per_img] int32, -1 past count_out[b];   count_out [B] int32.
 *   logits / deltas: rows of pitch ld_logits >= num_classes + 1 / ld_deltas >= 4.  workspace: hrf_bbox_detect_workspace_bytes(B, R,
 *   num_classes) bytes (0 for what is refused), 256-byte aligned, caller-owned, contents irrelevant.  REFUSED: R outside
 *   [1, HRF_RPN_MAX_PRE], num_classes outside [1, HRF_BBOX_MAX_CLASSES], num_stages outside [1, HRF_BBOX_MAX_STAGES], B < 1 or
 *   B * HRF_BBOX_MAX_CLASSES > 65535, a pitch smaller than the row, a null pointer (count / scale_factor excepted), a std that is
 *   not positive and finite, max_per_img < 1, score_thr outside [0, 1], iou_thr outside (0, 1], a workspace that is too small. */
#define HRF_BBOX_MAX_CLASSES 16
#define HRF_BBOX_MAX_STAGES 4
typedef struct hrf_bbox_det {
  int B, R, num_classes, num_stages;
  const float* rois;                     /* [B * R][5] (b, x1, y1, x2, y2): the last stage's input rois */
  const int* count;                      /* [B] valid rows per image, nullable */
  const float* logits[HRF_BBOX_MAX_STAGES];
  int ld_logits;
  const float* deltas;                   /* the last stage's */
  int ld_deltas;
  float stds[4];
  const float* img_shape;                /* [B][2] (h, w) */
  const float* scale_factor;             /* [B][4], nullable */
  float score_thr, iou_thr;
  int max_per_img;
} hrf_bbox_det_t;
long hrf_fc_workspace_bytes(long M, int K, int N);
int hrf_fc_pack(const float* w, int N, int K, int Np, int Kp, float* wp, void* stream);
int hrf_fc(const float* x, int ldX, const float* wp, const float* bias, float* y, int ldY, int relu, long M, int K, int N,
           void* workspace, long workspace_bytes, void* stream);
int hrf_bbox_refine(const float* rois_in, const float* deltas, int ld_deltas, float std_x, float std_y, float std_w, float std_h,
                    const float* img_shape, int B, long K, float* rois_out, void* stream);
long hrf_bbox_detect_workspace_bytes(int B, int R, int num_classes);
int hrf_bbox_detect(const hrf_bbox_det_t* d, void* workspace, long workspace_bytes, float* dets, int* labels, int* count_out,
                    void* stream);

/* ---- Backward of hrf_fc's layer (csrc/hrf_fc_bwd.h, part of csrc/conv3w_engine.hip) ------------------------------------------------
 * The gradients of y = act(bias + x w^T) for the three linear layers of Shared2FCBBoxHead in training.  Exact fp32 MFMA, hrf_fc's
 * block tile; no atomics, no arrival counters (the same bits from run to run and in deterministic mode), nothing read on the host,
 * no allocation, no synchronisation: capturable.  All pointers fp32; K % 16 == 0, N % 16 == 0, N <= 65536, 0 <= M <= 2^24.
 *
 * hrf_fc_bwd_data  dx[m][k] = (mask != null && mask[m][k] <= 0) ? +0 : sum_n dy[m][n] * w[n][k].
 *   dy [M] rows of pitch ldDY >= N, w [N] rows of pitch ldW >= K (what hrf_fc_pack writes, pitch K), mask [M] rows of pitch ldMask
 *   >= K or null: the FORWARD OUTPUT of the layer below when that layer ran with relu == 1, so that dx is already that layer's dy.
 *   The mask is a select (torch's threshold_backward): a masked element is +0 even where the sum is NaN / Inf, and a NaN in the
 *   mask lets the gradient through.  dx [M] rows of pitch ldDX >= K.  Pad columns are never read or written.
 * hrf_fc_bwd_weight  dw[n][k] (+)= sum_m dy[m][n] * x[m][k];  db[n] (+)= sum_m dy[m][n]  (db nullable; one more small launch).
 *   x [M] rows of pitch ldX >= K, dw [N] rows of pitch ldDW >= K, accumulate 0 (overwrite) or 1 (add to the contents).
 * Where the output has too few 128 x 128 tiles the reduction (N resp. M) is split over blocks - a function of (M, K, N) alone - and
 * the partial tiles go through slots of `workspace`, folded in slot order by a second launch.  hrf_fc_bwd_workspace_bytes(M, K, N):
 * the larger of the two entries' needs (0 when neither splits or the shape is refused); caller-owned, contents irrelevant, 16-byte
 * aligned; one buffer serves both calls of a layer.
 * M == 0: HRF_OK; hrf_fc_bwd_weight with accumulate == 0 still writes zeros to dw / db.
 * REFUSED (HRF_ERR_ARG before any launch): K % 16 != 0, N % 16 != 0, K / N < 1, M < 0, a null dy / w / dx / x / dw, a pitch below its
 * row length, accumulate not 0 / 1, a workspace that is null or too small when one is needed.
 * hrf_fc_bwd_cols  dst[n][c * A + a] (+)= src[n][a * C + c], n < N: a weight gradient taken on (y, x, c)-ordered feature columns
 *   ([K][7][7][C] RoI features, A = 49) into the parameter's (c, y, x) order.  Rows of pitch ldSrc / ldDst >= A * C; one launch.
 *   REFUSED: null pointers, N < 0, C / A < 1, a pitch below A * C, accumulate not 0 / 1, A * (C + 1) floats above 64 KB of LDS. */
long hrf_fc_bwd_workspace_bytes(long M, int K, int N);
int hrf_fc_bwd_data(const float* dy, int ldDY, const float* w, int ldW, const float* mask, int ldMask, float* dx, int ldDX, long M, int K,
                    int N, void* workspace, long workspace_bytes, void* stream);
int hrf_fc_bwd_weight(const float* x, int ldX, const float* dy, int ldDY, float* dw, int ldDW, float* db, int accumulate, long M, int K, int N,
                      void* workspace, long workspace_bytes, void* stream);
int hrf_fc_bwd_cols(const float* src, int ldSrc, float* dst, int ldDst, int accumulate, int N, int C, int A, void* stream);

/* ---- Cascade RoI head training targets and loss (csrc/hrf_bbox_train.h, part of csrc/pointwise.hip) -----------------------------
 * One stage of train_cfg.rcnn[i]: what CascadeRoIHead.forward_train does per stage between the proposals and the loss values
 * (mmdet/models/roi_heads/cascade_roi_head.py:191-286, bbox_heads/bbox_head.py:122-313, core/bbox/assigners/max_iou_assigner.py
 * with match_low_quality False, assign_result.py add_gt_, samplers/base_sampler.py:68-102 + random_sampler.py with neg_pos_ub -1,
 * iou2d_calculator.py:213-253, delta_xywh_bbox_coder.py:118-160, CrossEntropyLoss (softmax), SmoothL1Loss, accuracy top-1).
 * Fixed-shape outputs, no host read of an input, no allocation, no synchronisation, no float atomics (the same bits in
 * deterministic mode and from run to run), every loop bounded by Gmax, Gmax + R, num, num_classes or six radix passes - never by
 * data: capturable in a hipGraph.  Boxes, labels, logits and deltas are unvalidated device data.
 *
 * hrf_bbox_targets (two launches): assignment, sampling, target encoding.
 *   rois_in    [B * R][5] fp32 (b, x1, y1, x2, y2), image b at rows b * R ..; 1 <= R <= HRF_RPN_MAX_PRE;
 *   first / count  row range [first_b, count_b) of image b: int32 read at first[b * range_stride] / count[b * range_stride] on the
 *              device and clamped into [0, R]; either may be null (0 / R).  Rows outside the range are never read.  range_stride
 *              >= 1 lets two columns of an earlier stage's `counts` serve (counts + 4, counts + 5, stride 6);
 *   gt         [B][Gmax][4] fp32, gt_labels [B][Gmax] int32, gt_count [B] int32 clamped to [0, Gmax] in the kernel; read at run
 *              time: a captured graph follows changed contents.  1 <= Gmax <= HRF_RPN_MAX_GT;
 *   keys       [B][Gmax + R] uint32 sampling keys, or null: key = the hash of hrf_rpn_loss over (rng_state[0] ^ mix(0x5bd1e995 +
 *              stage), rng_state[1], image, slot) - `stage` (0 .. 255) decorrelates the stages of a step from each other and
 *              from the RPN.  hrf_bbox_targets never advances the counter.
 * The candidates of image b are the slots c of ONE index space of Gmax + R: c < Gmax is ground truth c, valid iff
 * add_gt_as_proposals != 0 and c < G_b; c = Gmax + r is row r, valid iff first_b <= r < count_b.  A ground-truth slot is assigned
 * c + 1 with max_iou 1 (add_gt_).  A row takes the maximum of bbox_overlaps over the G_b ground truths in its fp32 order (ties:
 * the first ground truth): max >= pos_iou_thr -> argmax + 1; 0 <= max < neg_iou_thr -> 0; otherwise -1.  G_b == 0: every row 0
 * with max_iou 0.  NaN propagates as in torch.max / torch.min: a row with any NaN IoU has max_iou NaN, is assigned -1 and is never
 * sampled.  The sampler keeps the min(P_b, num_pos) positives of smallest (key, c), then the min(N_b, num - sampled pos_b)
 * negatives of smallest (key, c): a uniform subset - RandomSampler's distribution, not its randperm stream.  Outputs (every
 * element of every output is written, no memset needed), image b at rows b * num ..:
 *   rois_s     [B * num][5]: the sampled positives in ascending c, then the sampled negatives in ascending c, then padding rows
 *              (b, 0, 0, 0, 0).  Sampled ground truths are therefore the first rows of an image, and rows [counts[b][4], counts[b][5])
 *              are the sampled proposals: the next stage's range after hrf_bbox_refine (the reference's pos_is_gt filter);
 *   labels     [B * num] int32: gt_labels of the matched ground truth / num_classes (negative) / -1 (padding);
 *   bbox_targets [B * num][4]: bbox2delta(box, matched gt) / stds on the positives, zero elsewhere;
 *   src        [B * num] int32: the candidate slot of the row, -1 for padding;
 *   counts     [B][6] int32: P_b, N_b, sampled positives, sampled negatives, sampled ground truths, rows n_b;
 *   assigned   [B][Gmax + R] int32 (-2: the slot is no candidate), max_iou [B][Gmax + R] fp32 (0 there).
 *
 * hrf_bbox_loss (two launches): the losses of those rows on the padded head output, and their gradient.
 *   out        [B * num] rows of pitch ld >= num_classes + 5: num_classes + 1 logits (background last), then four deltas;
 *   losses     [3] fp32, n = sum_b n_b (read on the device):
 *              [0] loss_weight_cls * sum_rows CE(softmax, stable log-sum-exp) / max(n, 1)   (label weights 1),
 *              [1] loss_weight_bbox * sum_{positive rows, 4} SmoothL1_beta(delta - target) / n   (0 when n == 0 or no positive),
 *              [2] 100 * #(argmax of the logits == label, the lowest index wins a tie) / n   (0 when n == 0; no loss weight);
 *   d_out      [B * num] rows of pitch ld_d: the ceil16(num_classes + 5) leading floats of EVERY row are written: d (losses[0] +
 *              losses[1]) / d out, zero on padding rows, on rows whose label is outside [0, num_classes] and in the pad columns;
 *   rng_state  nullable: when given, the last launch advances rng_state[1] (the caller passes it with the last stage of a step);
 *   workspace  hrf_bbox_train_workspace_bytes bytes (one fp64 slot triple per 256 rows, folded in slot order), 256-byte aligned,
 *              caller-owned, contents irrelevant.
 * cfg: the loss weights already include the stage's loss weight; min_pos_iou is validated but unused (match_low_quality False).
 * hrf_bbox_train_supported -> 1 / 0; hrf_bbox_train_workspace_bytes -> 0 for what is refused.  REFUSED with HRF_ERR_ARG before
 * any launch: B outside [1, 65535]; R outside [1, HRF_RPN_MAX_PRE]; Gmax outside [1, HRF_RPN_MAX_GT]; num outside
 * [1, HRF_RPN_MAX_PRE]; num_pos outside [0, num]; num_classes outside [1, HRF_BBOX_MAX_CLASSES]; a threshold outside [0, 1] or NaN;
 * a std or beta that is not positive and finite; a loss weight that is not finite; range_stride < 1; stage outside [0, 255];
 * ld < num_classes + 5; ld_d < ceil16(num_classes + 5); a null cfg / input / output (first, count, keys and the rng_state of
 * hrf_bbox_loss excepted); keys and rng_state both null (hrf_bbox_targets); a workspace that is null or too small (hrf_bbox_loss). */
typedef struct hrf_bbox_train_cfg {
  float pos_iou_thr, neg_iou_thr, min_pos_iou;
  int add_gt_as_proposals, num, num_pos, num_classes;
  float stds[4];
  float beta, loss_weight_cls, loss_weight_bbox;
} hrf_bbox_train_cfg_t;
int hrf_bbox_train_supported(const hrf_bbox_train_cfg_t* cfg, int B, int R, int Gmax);
long hrf_bbox_train_workspace_bytes(const hrf_bbox_train_cfg_t* cfg, int B, int R, int Gmax);
int hrf_bbox_targets(const hrf_bbox_train_cfg_t* cfg, int B, int R, const float* rois_in, const int* first, const int* count,
                     int range_stride, const float* gt, const int* gt_labels, const int* gt_count, int Gmax, const unsigned* keys,
                     const unsigned* rng_state, int stage, float* rois_s, int* labels, float* bbox_targets, int* src, int* counts,
                     int* assigned, float* max_iou, void* stream);
int hrf_bbox_loss(const hrf_bbox_train_cfg_t* cfg, int B, const float* out, int ld, const int* labels, const float* bbox_targets,
                  const int* counts, void* workspace, long workspace_bytes, float* d_out, int ld_d, float* losses,
                  unsigned* rng_state, void* stream);
/* the same gather for EVERY fused layer of a step in one launch: seg = nseg rows of 5 longs on the device {offset (floats) of the
 * layer's ds_plane in `planes`, windows, heads, address of its drpb accumulator, copy_stride}; max_nwin / max_heads = the
 * largest of the rows (launch geometry).                                                                               */
int hrf_rpb_grad_all(const float* planes, const long* seg, int nseg, int max_nwin, int max_heads, void* stream);
/* dst[map[i]] += sum_{s < nslots} slots[s*slot_stride + i]  (i < n; map[i] < 0: skipped).  One launch folds the slots of
 * every fused layer of a step: seg = nseg rows of 5 longs {slot offset (floats) into `slots`, nslots, slot_stride, n,
 * offset into `map`} on the device.                                                                                  */
int hrf_fold_slots(const float* slots, const long* seg, int nseg, const int* map, float* dst, long max_n, void* stream);

/* ---- BatchNorm bookkeeping (F.batch_norm, 329 call sites: every build_norm_layer(norm_cfg)) ---
 * stats = (sum y, sum y^2) from the producing conv -> scale/shift used by consumers' loaders,
 * saved mean/invstd, running-stat update (momentum, unbiased var).  With SyncBN the host
 * all-reduces `stats` (RCCL) between the producer and this call.                               */
int hrf_bn_finalize(const double* stats, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, double count, float eps, float momentum, int update_running,
                    float* scale, float* shift, float* mean_out, float* invstd_out, int C, void* stream);
/* gstats = (sum du, sum du*yraw): dgamma += , dbeta += , and the on-load backward coefficients
 * dy = cA*du + cB*yraw + cC.  train=0: frozen statistics (eval / norm_eval).  gstats_local
 * (nullable) = this rank's moments for the parameter grads when gstats was all-reduced (SyncBN). */
int hrf_bn_bwd_finalize(const double* gstats, const double* gstats_local, const float* gamma,
                        const float* mean, const float* invstd, double count, int train, float* dgamma, float* dbeta, float* cA, float* cB,
                        float* cC, int C, void* stream);

/* SyncBN over RCCL, several mutually independent BatchNorms per collective (the three sensor streams at equal depth, the
 * branches of one HRModule, the fuse layers of one exchange): hrf_bn_pack folds the replicated moments of n layers into
 * `packed` (2*C doubles per layer, back to back) -> ONE all-reduce of `packed` by the host -> hrf_bn_finalize_packed /
 * hrf_bn_bwd_finalize_packed finalise all n layers from the packed sums (the `stats` / `gstats` / `write` fields of the
 * structs are ignored; packed_local = this rank's copy of `packed` taken before the all-reduce: parameter gradients use the
 * rank-local moments).  stats / C / fins / bfins are HOST arrays of n entries.  `rows` (nullable HOST array of n doubles):
 * this rank's sample count of every layer, stored behind the sums at packed[sum_i 2*C_i + i] so that the SAME all-reduce
 * yields the global counts (hrf_bn_fin_t.count_ptr points there): `packed` then holds sum_i 2*C_i + n doubles.            */
int hrf_bn_pack(const double* const* stats, const int* C, int n, const double* rows, double* packed, void* stream);
int hrf_bn_finalize_packed(const hrf_bn_fin_t* fins, int n, const double* packed, void* stream);
int hrf_bn_bwd_finalize_packed(const hrf_bn_bfin_t* bfins, int n, const double* packed, const double* packed_local /* nullable: see pgrad_scale */, void* stream);

/* ---- peer-to-peer SyncBN exchange over xGMI (csrc/p2p_exchange.hip): what torch.nn.SyncBatchNorm's all-gather / all-reduce
 * of the per-layer moments does in the reference (norm_cfg type SyncBN, configs/_base_/models/cascade_rcnn_hrfuser_fpn_nus_clr_
 * fusion.py:2), without a communicator: every rank exposes an INBOX (fine-grained device memory, mapped by its peers through
 * IPC handles) of `world` source regions x 2 generation parities x slot_doubles doubles plus world x 2 x nslots flags; every
 * BatchNorm layer and direction owns a static slot (slot_off doubles into a region, flag index slot_id; 2*C + 1 doubles).
 * hrf_p2p_exchange = ONE launch on the lane that needs the result: fold this rank's replicated moments of n layers (the job of
 * hrf_bn_pack; rows as there), store them into the slot of every PEER's inbox, release flag = *gen at system scope, spin until
 * all peers show *gen (time-out: *err = ((source+1) << 32) | (slot_id+1), the launch completes with garbage and the
 * host raises), add the contributions in rank order into `packed` (layout of hrf_bn_pack: sums back to back, then n counts).
 * phase: 0 / 3 = all of it (the product); 1 = fold + push only, 2 = wait + reduce only (single-thread emulator tests).
 * hrf_p2p_tick: *gen += 1, once per training step before the first exchange (inside the captured graph).
 * hrf_p2p_alloc / open / close / free: inbox memory and its 64-byte IPC handle (hipExtMallocWithFlags fine-grained,
 * hipIpcGetMemHandle / hipIpcOpenMemHandle).  inbox[p] / flags[p]: rank p's data / flag area AS MAPPED INTO THIS PROCESS.     */
#define HRF_P2P_MAX_RANKS 8
typedef struct hrf_p2p {
  int world, rank;
  double* inbox[HRF_P2P_MAX_RANKS];
  long* flags[HRF_P2P_MAX_RANKS];
  long slot_doubles, nslots;
  const long* gen;
  long* err;
  long timeout_ticks;            /* 100 MHz ticks; <= 0: wait for ever */
} hrf_p2p_t;
int hrf_p2p_exchange(const hrf_p2p_t* ctx, const double* const* stats, const int* C, int n, const double* rows,
                     const long* slot_off, const int* slot_id, double* packed, int phase, void* stream);
int hrf_p2p_tick(long* gen, void* stream);
int hrf_p2p_alloc(long bytes, void** ptr, void* handle64);
int hrf_p2p_open(const void* handle64, void** ptr);
int hrf_p2p_close(void* ptr);
int hrf_p2p_free(void* ptr);

/* ---- GroupNorm (norm_cfg = dict(type='GN', num_groups=G): build_norm_layer at hrnet.py:338-339,438,459,476,
 * resnet.py:34-35,161-164, hrformer.py:269,278,281,518,542,552 -> nn.GroupNorm / F.group_norm).  Per-(sample, group)
 * statistics, no exchange between samples or ranks.  Three launches per direction:
 *   hrf_gn_moments  out[b][0][c] += sum_p v, out[b][1][c] += sum_p v*w (w NULL: v*v) over the rows_per_sample pixels of
 *                   sample b; `out` ([B][2][C] doubles) must be zero.  Forward: v = raw conv output; backward: v = du, w = raw.
 *   hrf_gn_apply    y = gamma*(raw - mean)*rstd + beta with (mean, rstd) of every (sample, group) folded from `mom`,
 *                   also stored in stat[b][g][2] for the backward.
 *   hrf_gn_bwd      draw = rstd*(du*gamma - mean_group(du*gamma) - xhat*mean_group(du*gamma*xhat)); dgamma += , dbeta += . */
int hrf_gn_moments(const float* v, const float* w, int B, long rows_per_sample, int C, double* out, void* stream);
int hrf_gn_apply(const float* raw, const double* mom, const float* gamma, const float* beta, float eps, int B,
                 long rows_per_sample, int C, int G, float* y, float* stat, void* stream);
int hrf_gn_bwd(const float* du, const float* raw, const float* stat, const double* gmom, const float* gamma, int B,
               long rows_per_sample, int C, int G, float* draw, float* dgamma, float* dbeta, void* stream);

/* ---- LayerNorm over channels (F.layer_norm: hrformer.py:343,351; hrfuser_hrformer_based.py:279-291) */
int hrf_ln_stats(const float* x, int rows, int C, float eps, float* rowstat, void* stream);
int hrf_ln_bwd(const float* da, const float* x, const float* rowstat, const float* gamma, int rows, int C,
               float* dx, int accumulate, float* dgamma, float* dbeta, long copy_stride, void* stream);

/* `ln_rowstat` (hrf_conv_fwd, hrf_affine_act_res; nullable): also emit the LayerNorm row statistics
 * (mean, rstd with ln_eps) of the OUTPUT rows - the consumer's LayerNorm needs no hrf_ln_stats launch. */
/* ---- BN-apply + activation + residual materialisation and its adjoint ---------------------
 * act: 0 none, 1 ReLU, 2 GELU.  act_first=1: out = res + rowscale[b]*act(sc1*y1+sh1)
 * (CrossFFN tail hrformer.py:371 / DropPath); act_first=0: out = act(sc1*y1+sh1 + res + sc2*y2+sh2)
 * (Bottleneck tail resnet.py:282-300, transition ReLU hrnet.py:438-440).                        */
int hrf_affine_act_res(const float* y1, const float* sc1, const float* sh1, const float* y2,
                       const float* sc2, const float* sh2, const float* res, const float* rowscale,
                       int rows_per_sample, int act, int act_first, float* out, long rows, int C, float* ln_rowstat, float ln_eps,
                       const hrf_bn_fin_t* fin1, const hrf_bn_fin_t* fin2, void* stream);
/* out = res + res2 + y*mask*mscale*rowscale[b]: nn.Dropout(proj_drop) hrfuser_hrformer_based.py:97
 * and mmcv DropPath hrfuser_hrformer_based.py:301-315 arithmetic (mask / rowscale nullable).    */
int hrf_scale_add(const float* y, const float* mask, float mscale, const float* rowscale,
                  int rows_per_sample, const float* res, const float* res2, float* out, long rows, int C,
                  void* stream);
/* mode 0: g = dout*(out>0); 1: g = dout*rowscale*gelu'(sc*y1+sh); 2: g = dout.  st_k (nullable)
 * accumulate (sum g, sum g*y_k) for the BatchNorms whose output fed the activation.            */
int hrf_act_bwd(const float* dout, const float* out, const float* y1, const float* sc, const float* sh,
                const float* rowscale, int rows_per_sample, int mode, float* g, const float* y2,
                const float* y3, double* st1, double* st2, double* st3, long rows, int C, void* stream);

/* ---- HRModule cross-resolution exchange (hrnet.py:184-207; fuse layers hrformer.py:498-561) ---
 * out = ReLU(sum of up to four terms); term type 0 unused, 1 identity, 2 BN-affine of a same-
 * resolution raw conv output, 3 BN-affine of a bilinearly up-sampled (align_corners=False)
 * low-resolution raw conv output (Hs x Ws), 4 the same through nn.Upsample(mode='nearest') by the integer factor
 * H / Hs (the convolutional HRModule, hrnet.py:135-146; H % Hs == 0 and W % Ws == 0).              */
int hrf_fuse_sum(int type0, const float* p0, const float* sc0, const float* sh0, int Hs0, int Ws0,
                 int type1, const float* p1, const float* sc1, const float* sh1, int Hs1, int Ws1,
                 int type2, const float* p2, const float* sc2, const float* sh2, int Hs2, int Ws2,
                 int type3, const float* p3, const float* sc3, const float* sh3, int Hs3, int Ws3,
                 float* out, int B, int H, int W, int C, const hrf_bn_fin_t* fins, void* stream);
/* `fin1` / `fin2` of hrf_affine_act_res and `fins` of hrf_fuse_sum (an array of FOUR hrf_bn_fin_t, one per term; entries
 * with stats == NULL are unused; C <= HRF_FIN_MAXC / 2) finalise the BatchNorm of the respective operand on load.  */
/* adjoint of the bilinear up-sampling (gather form) + (sum du, sum du*ylow) moments              */
int hrf_bilinear_up_bwd(const float* g, int ldG, int goff, int B, int H, int W, int C, const float* ylow, int Hs, int Ws,
                        float* du, double* stats, void* stream);
/* adjoint of the nearest up-sampling of term type 4 (block sums) + the same moments                       */
int hrf_nearest_up_bwd(const float* g, int ldG, int goff, int B, int H, int W, int C, const float* ylow, int Hs, int Ws,
                       float* du, double* stats, void* stream);
/* The whole backward of ONE exchange sum out = ReLU(sum of terms) in ONE launch: what hrf_act_bwd (mode 0), hrf_scale_add
 * (the identity term) and one hrf_bilinear_up_bwd per up-sampled term do in series, as block-uniform sections of one grid.
 * With v = dout * [out > 0] ([B, H, W, C] rows):
 *   elementwise section: g = v (g nullable: written when a same-resolution term or an aliasing identity needs it);
 *     id_dst (nullable) = v, or id_dst += v with id_accumulate = 1 (the identity term's gradient);
 *     same-resolution term k (st[k] != NULL; y[k] its raw conv output): st[k] [HRF_STAT_COPIES][2*C] += (sum v, sum v*y[k]).
 *   one section per up-sampled term j (up_kind[j] = 1: bilinear, align_corners=False; 0: unused): up_du[j] [B, up_Hs, up_Ws, C]
 *     = the adjoint of the up-sampling applied to v (read from dout / out with the mask applied on load - no section waits
 *     for g), up_stats[j] (nullable) += (sum du, sum du*up_ylow[j]) (up_ylow nullable).  For the integer factors 2, 4 and 8
 *     (H = F up_Hs and W = F up_Ws) the 2F x 2F taps of a (low-resolution pixel, channel) are loaded 32 at a time, their rows
 *     spread over up to F threads from factor 4 and added in a fixed order; for every other ratio the gather order is the one
 *     of hrf_bilinear_up_bwd (bit-equal du).
 * g and id_dst are bit-equal to hrf_act_bwd + hrf_scale_add on the same arguments.  No float atomics on LDS or on the
 * tensors; the moments go through the replicated / deterministic accumulators like every other entry point.
 * Taken: C even, 8 <= C <= 256 (hrf_fuse_sum_bwd_supported(C) == 1), up_kind in {0, 1}, every tensor below 2^30 elements.
 * Everything else - a nearest term included - is HRF_ERR_ARG before any launch: the caller issues the three entry points
 * above. */
typedef struct hrf_fuse_bwd {
  const float* dout; const float* out;
  int B, H, W, C;
  float* g;
  float* id_dst; int id_accumulate;
  const float* y[3]; double* st[3];
  int up_kind[3]; const float* up_ylow[3]; int up_Hs[3]; int up_Ws[3]; float* up_du[3]; double* up_stats[3];
} hrf_fuse_bwd_t;
int hrf_fuse_sum_bwd_supported(int C);
int hrf_fuse_sum_bwd(const hrf_fuse_bwd_t* p, void* stream);

/* ---- HRFPN neck pieces (mmdet/models/necks/hrfpn.py:77-100) --------------------
 * hrf_bilinear_up_into: out[pix][off + c] = F.interpolate(x, size=(H,W), mode='bilinear')[pix][c]
 *   (align_corners=False; a plain copy when Hs == H): the up-sample + channel concat in one pass;
 *   its adjoint is hrf_bilinear_up_bwd reading the concat gradient through (ldG, goff).
 * hrf_avg_pool / hrf_avg_pool_bwd: F.avg_pool2d(kernel_size = stride = k) on NHWC rows.
 * hrf_slice_cols: dst[row][c] (+)= src[row][off + c] - the concat adjoint of the branch that is not up-sampled. */
int hrf_bilinear_up_into(const float* x, int Hs, int Ws, int C, float* out, int ldOut, int off, int B, int H, int W,
                         void* stream);
int hrf_avg_pool(const float* x, int B, int H, int W, int C, int k, float* out, void* stream);
/* The 3x3 / pad-1 patches of a FEW-channel input as rows (the stem's first convolution, 3 -> 64 stride 2 on the NCHW network input:
 * hrnet.py:341-347, hrfuser_hrformer_based.py:380-386):  cols[(b, yo, xo)][ci * 9 + tap] = x(b, ci, yo * stride - 1 + tap / 3,
 * xo * stride - 1 + tap % 3), zero outside the image; x through element strides (NCHW or channels-last), rows `ld` >= 9 Cin floats apart.
 * The column order is the OIHW weight's memory order: F.conv2d(x, w, stride, 1) = cols . w.view(Cout, 9 Cin)^T (hrf_conv_fwd with KH = 1
 * on the rows) and grad_weight = dY^T . cols (hrf_conv_bwd_weight with KH = 1) - both on the channel-contiguous row kernels
 * instead of 27 strided gathers per output pixel, and the patches are formed once per step for both. */
int hrf_im2col3x3(const float* x, int sB, int sY, int sX, int sC, int B, int H, int W, int Cin, int stride,
                  float* cols, int ld, void* stream);
int hrf_slice_cols(const float* src, int ld, int off, long rows, int C, float* dst, int accumulate, void* stream);
int hrf_avg_pool_bwd(const float* g, int B, int H, int W, int C, int k, float* dx, int accumulate, void* stream);

/* Wide 3x3 / stride-1 / pad-1 convolution on tap-major packed weights (the HRFPN 256->256 output convolutions,
 * hrfpn.py:60-70,92-100, and their backward-data): K % 32 == 0 input channels, N % 64 == 0 output channels.
 *   hrf_conv3_pack   wp[tap][n][k] = w[n][k][tap]        (dir 0: forward operand, N = Cout, K = Cin)
 *                    wp[tap][n][k] = w[k][n][8 - tap]    (dir 1: backward-data operand, N = Cin, K = Cout)
 *                    w is the OIHW tensor [Cout][Cin][3][3]; wp holds 9*Cout*Cin floats (caller-owned scratch,
 *                    refreshed whenever w changes - once per step).
 *   hrf_conv3_packed y[pix][n] (+)= bias[n] + sum_{tap,k} x[pix + tap][k] * wp[tap][n][k]   (zero padding);
 *                    forward: x = input rows, wp = pack(dir 0); backward-data (aten convolution_backward's
 *                    grad_input): x = dY rows, wp = pack(dir 1), bias = null, accumulate = 1 to add into a gradient. */
int hrf_conv3_pack(const float* w, int Cout, int Cin, int dir, float* wp, void* stream);
int hrf_conv3_packed(const float* x, int ldX, const float* wp, const float* bias, float* y, int ldY, int accumulate,
                     int B, int H, int W, int K, int N, void* stream);
/* bf16x3 matrix mode of the same convolution: the bf16 matrix cores with fp32-level accuracy.  Every fp32 operand v is split
 * into two bf16 values, hi = rne(v) and lo = rne(v - hi) (round to nearest even), and every product is computed as
 * lo*hi + hi*lo + hi*hi on v_mfma_f32_16x16x32_bf16, accumulated in fp32; bias and accumulate are applied in the fp32 epilogue.
 * Accuracy: relmax against an fp64 convolution 4e-6 .. 6e-6 on unit-variance data (fp32 kernel: 2e-7 .. 5e-7; one bf16 product
 * alone: 2e-3) - the dropped lo*lo term and the rounding of lo, 2^-16 .. 2^-17 per product; DESIGN section 13.
 *   hrf_conv3_pack_bf16x3    same `dir` semantics and the same 9*Cout*Cin*4 bytes as hrf_conv3_pack, holding bf16 planes: with
 *                    p = the fp32 pack [tap][n][k], the 32-channel slab s of row (tap, n) is 64 bf16 at the byte offset of
 *                    p[tap][n][32 s]: bf16 [0, 32) = hi(p[tap][n][32 s + j]), bf16 [32, 64) = lo(p[tap][n][32 s + j]), i.e. the
 *                    buffer viewed as bf16 is [9][N][K/32][2 (hi, lo)][32].  K (Cin for dir 0, Cout for dir 1) % 32 == 0.
 *   hrf_conv3_packed_bf16x3  the contract of hrf_conv3_packed (fp32 rows in, fp32 rows out, K % 32 == 0, N % 64 == 0, columns
 *                    of y beyond N untouched) on a pack of hrf_conv3_pack_bf16x3; an unsupported shape returns HRF_ERR_ARG
 *                    before any launch.  No atomics: bit-reproducible, independent of hrf_set_deterministic.
 *   hrf_conv3_bf16x3_supported  1 when (K, N) is a shape hrf_conv3_packed_bf16x3 accepts, else 0; no launch. */
int hrf_conv3_pack_bf16x3(const float* w, int Cout, int Cin, int dir, float* wp, void* stream);
int hrf_conv3_packed_bf16x3(const float* x, int ldX, const float* wp, const float* bias, float* y, int ldY, int accumulate,
                            int B, int H, int W, int K, int N, void* stream);
int hrf_conv3_bf16x3_supported(int K, int N);
/*   hrf_conv3_wgrad_wide  dW[co][ci][3][3] += sum_pix dY[pix][co] * x[pix + tap][ci],  dbias[co] += sum_pix dY[pix][co]
 *                    (aten convolution_backward's grad_weight / grad_bias of the same convolution; OIHW dW;
 *                    Cout % 128 == 0, Cin % 64 == 0; dbias nullable).  The pixel-split partial sums pass through
 *                    `scratch`: hrf_conv3_wgrad_wide_scratch(...) floats, caller-owned, contents irrelevant. */
long hrf_conv3_wgrad_wide_scratch(int B, int H, int W, int Cin, int Cout);
int hrf_conv3_wgrad_wide(const float* dy, int ldD, const float* x, int ldX, int B, int H, int W, int Cin, int Cout,
                         float* dw, float* dbias, float* scratch, void* stream);

/* Wide 1x1 convolution / Linear as an LDS-tiled MFMA row GEMM (the HRFPN reduction convolution, hrfpn.py:53-58,85):
 *   hrf_rowgemm_pack  wp[n][k] (n < Np, k < Kp) = w[n][k] (dir 0: forward operand, w = [Cout][Cin]) or w[k][n]
 *                     (dir 1: backward-data operand), zero outside the tensor: Np / Kp are the padded sizes.
 *   hrf_rowgemm       y[m][n] (+)= bias[n] + sum_k x[m][k] * wp[n][k];  K % 16 == 0, N % 16 == 0 (pad columns of x must
 *                     hold zeros or finite values matched by zero weights; bias, if given, has N entries). */
int hrf_rowgemm_pack(const float* w, int Cout, int Cin, int dir, int Np, int Kp, float* wp, void* stream);
int hrf_rowgemm(const float* x, int ldX, const float* wp, const float* bias, float* y, int ldY, int accumulate,
                long M, int K, int N, void* stream);

/* Grouped weight gradients.  Weight gradients are leaves of the backward graph; between hrf_wgrad_group_begin() and
 * hrf_wgrad_group_end(stream) every hrf_conv_bwd_weight call that maps to the pixel-major kernel is queued instead of
 * launched (its `stream` argument is ignored), and _end issues the queue on `stream`, up to 16 problems of one kernel
 * variant per launch (results identical to separate launches).  Calls that use other kernels launch immediately. */
int hrf_wgrad_group_begin(void);
int hrf_wgrad_group_end(void* stream);

/* Multi-problem launches for the EQUAL-SHAPE layers of sibling sensor streams.  The reference runs the camera stream's
 * finest branch and the M modality streams through layers of identical shape with different weights
 * (hrfuser_hrformer_based.py:536-544 stems, :564-565 stage 2 || LidarStageB, :585-586 stage 3 || LidarStageC), each as its own
 * sequence of ATen launches.  Here the hot kernels take their arguments as an array of up to 4 problems (blockIdx.z selects
 * the problem; csrc/hrf_group.h): between hrf_group_begin() and hrf_group_end(stream) the launches of the calls to
 *   hrf_conv_fwd, hrf_conv_bwd_data, hrf_dwconv_fwd, hrf_dwconv_bwd_data(_weight), hrf_attn_block_fwd / _bwd,
 *   hrf_window_attn_fwd / _bwd, hrf_window_attn_proj_fwd, hrf_affine_act_res, hrf_act_bwd, hrf_scale_add, hrf_ln_stats, hrf_ln_bwd,
 *   hrf_fuse_sum,
 *   hrf_bilinear_up_bwd
 * are queued (their `stream` argument is ignored) and hrf_group_end issues them on `stream`: launches of the same kernel
 * instantiation and launch geometry that sit at the same position of DIFFERENT calls become ONE launch; everything else is
 * issued as it would have been, the launches of one call in their order.  The caller brackets MUTUALLY INDEPENDENT calls
 * only.  Results are identical to separate launches.  Per-thread state; begin / end must pair on one thread.
 * hrf_group_count(what): process-wide totals since load - 0 launches issued by hrf_group_end, 1 calls' launches they
 * carried, 2 hrf_group_end calls (measurement aid); 3: the number of problems per launch the library was COMPILED for
 * (HRF_GROUP_MAX).  The shipped build uses 1 - begin / end then only queue and re-issue - because on MI355X the merged
 * launches measured slower than one HIP stream per sensor (csrc/hrf_group.h); -DHRF_GROUP_MAX=4 builds the
 * multi-problem kernels (the CPU-emulator test build does). */
int hrf_group_begin(void);
int hrf_group_end(void* stream);
long hrf_group_count(int what);

/* Device-side input pipeline: the image side of Normalize -> RandomFlip -> Pad(size_divisor) -> RandomDrop ->
 * DefaultFormatBundle (mmdet/datasets/pipelines/transforms.py:706-753,440-466,649-664,487-514; formating.py:212-227) for ONE
 * sensor of a batch in one pass: in = [B][H0][W0][C] HWC images (float32, or uint8 when is_u8), out = [B][Hp][Wp][C]
 * float32 (channels-last storage of the logical (B,C,Hp,Wp) tensor the backbone takes);
 *   out = drop[b] ? 0 : inside ? (in(b, y, flip[b] ? W0-1-x : x, to_rgb ? C-1-c : c) - mean[c]) * stdinv[c] : 0.
 * mean / stdinv: C floats on the device (stdinv = float32(1 / float64(std)), as mmcv.imnormalize computes it);
 * flip / drop: B bytes each (nullable): the random decisions stay with the host's RNG. */
int hrf_pack_input(const void* in, int is_u8, int B, int H0, int W0, int C, const float* mean, const float* stdinv,
                   int to_rgb, const unsigned char* flip, const unsigned char* drop, float* out, int Hp, int Wp,
                   void* stream);

/* ---- fused flat-buffer AdamW (configs/hrfuser: AdamW lr 3e-4, wd 0.01, decay_mult 0 masks) ---
 * state = float[4] on device: {1-b1^t, 1-b2^t, t, lr}; hrf_adamw_tick advances t on device so a
 * captured hipGraph replays correct bias corrections; lr < 0 in the call = take the learning rate from state[3]
 * (the host updates that one float between replays: warm-up / step schedules work under hipGraph replay).
 * wd_mask[i]: weight-decay multiplier of element i (0 for `norm` / `relative_position_bias_table` keys); < 0 =
 * the element belongs to a parameter that never receives a gradient: skipped entirely, as torch.optim skips
 * parameters whose .grad is None (mmdet runs DDP with find_unused_parameters=True for transition1.0.1.*).        */
int hrf_adamw_tick(float* state, float beta1, float beta2, void* stream);
/* dst[map[i]] += sum_k scratch[k*copy_stride + i], k < HRF_STAT_COPIES (see top of file)          */
int hrf_fold_copies(const float* scratch, long copy_stride, const int* map, float* dst, long n,
                    void* stream);
int hrf_adamw(float* p, const float* g, float* m, float* v, const float* wd_mask, long n, float lr,
              float beta1, float beta2, float eps, float weight_decay, const float* state,
              float grad_scale, void* stream);

/* ---- global gradient-norm clipping in front of the fused AdamW (torch.nn.utils.clip_grad_norm_, norm_type 2; mmcv's
 * OptimizerHook(grad_clip=dict(max_norm=...))) - three launches, everything on the device, no atomics in any mode:
 *   hrf_grad_sumsq: partials[b] = sum of (double)g[i]^2 over block b's fixed share of the n floats, b < hrf_grad_sumsq_parts(n)
 *     (a pure function of n, 1 ... 1024: the caller sizes `partials` with it).  wd_mask as in hrf_adamw: elements with
 *     wd_mask[i] < 0 are skipped (torch skips `grad is None`), NULL = all count.  g / wd_mask need 4-byte alignment only;
 *     any n >= 0.  fp64 sums in a fixed order (a float's square is exact in fp64): a partial is a bit-exact function of the
 *     arena, so the deterministic mode has no second code path and every rank computes the same norm after the all-reduce.
 *   hrf_adamw_tick_clip: one single-block launch that sums partials[0 .. nparts) in a fixed order (the partials of several
 *     arenas may lie back to back), fills clip and advances the step count.  clip = float[8] on the device:
 *       [0] coef  [1] total_norm  [2] finite (1 / 0)  [3] count of skipped steps  [4] max_norm  [5] skip this step  [6..7] 0
 *     clip[4] is written by the HOST (a device value, so a captured hipGraph follows it); <= 0 or +inf = report the norm, do
 *     not clip (coef = 1).  total_norm = float(grad_scale * sqrt(sum)) in fp64 - the norm of the AVERAGED gradient, finite
 *     wherever the fp64 sum is (torch's fp32 norm overflows from elements of ~1e19 on); coef = min(1, max_norm /
 *     (total_norm + 1e-6f)) in fp32 as torch computes it (a NaN norm gives a NaN coef, an Inf norm coef 0).  finite =
 *     isfinite(total_norm).  skip_nonfinite != 0 and finite == 0: clip[5] = 1, clip[3] += 1 and `state` is NOT advanced;
 *     otherwise clip[5] = 0 and state advances as in hrf_adamw_tick.  nparts == 0: clip is already final for this step -
 *     clip[0..5] stay, state advances unless clip[5] is set (the tick of a second arena that shares the norm).
 *   hrf_adamw_clipped: hrf_adamw with the gradient fl(fl(g[i] * grad_scale) * clip[0]) - two fp32 roundings in that order:
 *     DDP averages, then clip_grad_norm_ multiplies (coef == 1: bit-equal to hrf_adamw); returns without touching p, m, v
 *     when clip[5] != 0.                                                                                              */
long hrf_grad_sumsq_parts(long n);
int hrf_grad_sumsq(const float* g, const float* wd_mask, long n, double* partials, void* stream);
int hrf_adamw_tick_clip(float* state, float* clip, const double* partials, int nparts, float grad_scale,
                        int skip_nonfinite, float beta1, float beta2, void* stream);
int hrf_adamw_clipped(float* p, const float* g, float* m, float* v, const float* wd_mask, long n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, const float* state,
                      float grad_scale, const float* clip, void* stream);

/* The digest (sha256, 64 hex characters) of the sources, headers, flags and target this library was built from
 * (hrfuser_amd/build_ext.py compares it with the tree on every build(): a source change is never paired with an old binary). */
const char* hrf_build_digest(void);

/* Measurement and tuning entry points (GPU time stamps inside a captured graph, the critical-lane probe, kernel tuning knobs,
 * the in-situ timing report of the grouped weight gradients) are NOT part of this interface: include/hrfuser_hip_debug.h. */

/* ---- deterministic mode (opt-in, off by default; csrc/hrf_rt.h has the arithmetic) ---------------------------------------
 * hrf_set_deterministic(1): every later call of this library accumulates its cross-block sums - the replicated BatchNorm
 * moments and the fp32 parameter gradients that are otherwise added with floating-point atomics - as EXACT 64-bit integer
 * sums (four bins of 40 bits per accumulator, 2^-96 ... 2^64; integer atomics), so every result is a bit-exact function of
 * the call's inputs: independent of the order in which blocks or waves run, across repeats, processes and graph replays.
 * With the mode off nothing changes.  The mode is process-wide host state, read when a call ISSUES its launches: a captured
 * hipGraph keeps the mode it was captured in; producer and consumer of one buffer must be issued in the same mode.
 *   - moments: the four fp64 copies of a [HRF_STAT_COPIES][2*C] slot are the four bins of each element - same buffers, same
 *     zeroing; hrf_bn_finalize, hrf_bn_bwd_finalize and hrf_bn_pack read the bins instead of summing copies.  The finalize-
 *     on-load prologues of the consumer kernels do not (the integer chains would cost the default-mode kernels registers):
 *     in deterministic mode a BatchNorm is finalised by its own launch, as with HRF_FIN_ONLOAD=0.  A build with
 *     HRF_STAT_COPIES < 4 cannot be switched on (HRF_ERR_ARG).
 *   - fp32 gradient accumulators (dw / dbias / dgamma / dbeta / dkpad / dvpad / drpb arguments that are "+=" with atomics):
 *     the caller owns SHADOW BINS, hrf_det_bins_bytes(n) bytes (32 per element, 8-byte aligned, zeroed once) for a range of n
 *     floats, announced with hrf_det_register(base, n, bins) (bins == NULL: forget the range; a new range replaces the ones it
 *     overlaps; at most 64 ranges).  In deterministic mode the kernels add into the bins of the target element - of copy 0
 *     where the accumulator is replicated (`copy_stride`) - and leave the floats alone; hrf_det_resolve(g, n, stream) then
 *     does g[i] += value(bins[i]) and returns the bins to zero (any mode; before hrf_fold_copies, a gradient exchange or the
 *     optimizer read g).  Plain "+=" / stores of other kernels into the same floats are ordered by the stream as always.
 *   - limits: at most 2^20 addends per accumulator and launch sequence; bits of an addend below 2^-96 are dropped (per addend,
 *     so still order-independent); an addend that is not finite, or not below 2^64, makes the accumulator NaN.
 *   - REFUSED in deterministic mode (HRF_ERR_ARG before any launch, outputs untouched) - never a silent unordered atomic:
 *       a gradient accumulator outside every registered range;
 *       an hrf_bn_fin_t / hrf_bn_bfin_t over REPLICATED moments (copies 0 / HRF_STAT_COPIES) handed to any consumer - hrf_conv_fwd
 *       (_split, _packed), hrf_conv_bwd_data (_packed), hrf_dwconv_fwd / _bwd_data (_weight), hrf_attn_block_fwd / _bwd,
 *       hrf_affine_act_res, hrf_fuse_sum; folded moments (copies 1) are plain doubles and are taken;
 *       hrf_rpb_grad_all (its accumulator addresses sit in a device table: use hrf_rpb_grad per layer);
 *       hrf_conv3_wgrad_wide with a bias gradient (the HRFPN neck's output convolutions);
 *       hrf_gn_moments (GroupNorm);
 *       hrf_p2p_exchange (SyncBN over more than one rank: the cross-rank order is out of scope; the one-rank path through
 *       hrf_bn_pack / hrf_bn_finalize_packed works);
 *       hrf_roi_align_bwd (fp32 atomics into whole activation maps: shadow bins of 32 bytes per element are out of proportion,
 *       an order-independent backward is not built; hrf_roi_align_fwd has no atomics and is the same bits in either mode). */
int hrf_set_deterministic(int on);
int hrf_get_deterministic(void);
long hrf_det_bins_bytes(long n);
int hrf_det_register(float* base, long n, void* bins);
int hrf_det_resolve(float* g, long n, void* stream);

/* hipMemsetAsync on `stream` (the per-step zeroing of the replicated accumulators). */
int hrf_memset(void* ptr, int value, long bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HRFUSER_HIP_H_ */
