// Cascade RoI head training targets and loss, one stage of train_cfg.rcnn[i] per call: MaxIoUAssigner (match_low_quality False),
// add_gt_as_proposals, RandomSampler, bbox2delta targets, softmax cross-entropy + SmoothL1 + accuracy and their gradient on the
// padded fc_cls / fc_reg output (gfx950, fp32).
//
//   mmdet/models/roi_heads/cascade_roi_head.py:191-286 (forward_train: per stage assign + sample per image, _bbox_forward_train,
//   refine_bboxes with the pos_is_gt filter), bbox_heads/bbox_head.py:122-255 (get_targets), :257-313 (loss; avg_factor of loss_cls =
//   the rows, of loss_bbox = bbox_targets.size(0)), core/bbox/assigners/max_iou_assigner.py:84-213, assign_result.py:196-206 (add_gt_),
//   core/bbox/samplers/base_sampler.py:68-102 (gts in front of the proposals), random_sampler.py:64-82, sampling_result.py (bboxes =
//   cat(pos, neg)), core/bbox/iou_calculators/iou2d_calculator.py:213-253, coder/delta_xywh_bbox_coder.py:118-160, losses/
//   cross_entropy_loss.py, smooth_l1_loss.py, accuracy.py.
//
// Part of the translation unit pointwise.hip (included after hrf_rpn_train.h, whose hash, gt staging, gt_count clamp and 64-bit
// sampling codes it uses).  Fixed-shape outputs, no host read of any input, no allocation, no synchronisation, no float atomics (the
// only atomics are integer adds in LDS: the same bits in deterministic mode and from run to run).  Every loop is bounded by Gmax,
// Gmax + R, num, num_classes or the six radix passes, never by data; boxes, labels, logits and deltas may be anything.
//
// The candidates of image b live in ONE index space of N = Gmax + R slots: slot c < Gmax is ground truth c (valid iff
// add_gt_as_proposals and c < G_b), slot Gmax + r is row r of the image (valid iff first_b <= r < count_b).
//
//   hrf_bbox_targets
//   1  bbt_assign_kernel    per candidate (256 per block, grid (ceil(N / 256), B)): the image's gts staged in LDS; a gt slot gets
//                           (c + 1, 1.0f) as add_gt_ does; a row gets the maximum over the gts of bbox_overlaps in its fp32 order
//                           (NaN propagates as torch.max does: any NaN IoU makes the maximum NaN, which fails every comparison -> -1;
//                           ties: the lowest gt), then -1 / 0 (0 <= max < neg_iou_thr) / argmax + 1 (max >= pos_iou_thr); no gts: 0.
//                           Slots that are no candidates get (-2, 0): every element of assigned / max_iou is written.
//   2  bbt_sample_kernel    one workgroup of 1024 per image: assigned + the 64-bit codes (key << 32 | c) of all N <= 2304 slots in
//                           LDS, P and Q counted, the k-th smallest code of the positives / negatives by the radix select of
//                           rpnt_select_kernel (8 bits per pass, at most 6 passes: 4 key bytes + 2 index bytes), an exclusive scan of
//                           the two sampled flags over the slots (each thread owns BBT_PER consecutive slots; Hillis-Steele over the
//                           1024 thread totals, positives and negatives packed into one word) = the output row of every sampled
//                           slot: positives in ascending c, then negatives in ascending c, then padding.  The thread of a sampled
//                           slot writes its row of rois_s / labels / bbox_targets / src; the padding rows and counts follow.
//   hrf_bbox_loss
//   3  bbt_loss_kernel      per row (256 per block): stable log-sum-exp cross-entropy over num_classes + 1 logits, top-1 (lowest index
//                           wins a tie), SmoothL1(beta) on the four deltas of a positive row, the gradient row (EVERY one of the
//                           ceil16(num_classes + 5) leading floats), three fp64 block sums (LDS tree) into the block's own slot.
//                           n = sum_b n_b is read from the device counts.
//   4  bbt_finalize_kernel  one wave folds the slots in slot order (lane j: slots j, j + 64, ...; then the 64 lane sums in lane
//                           order), writes the three results and (rng_state given) advances the counter.
//
// SAMPLING as in hrf_rpn_train.h with the stage folded into the seed: key = keys[b][c], or
//   rpnt_hash(seed ^ rpnt_mix(0x5bd1e995 + stage), counter, b, c)      (hrfuser_amd.testing.rcnn_key_ref restates it)
// so that the stages of one step and the RPN (which hashes the bare seed) draw decorrelated samples.
#pragma once

namespace {

constexpr int BBT_NT = 256;                    // per-candidate and per-row kernels
constexpr int BBT_SEL_NT = 1024;               // the sampling workgroup
constexpr int BBT_MAXN = HRF_RPN_MAX_GT + HRF_RPN_MAX_PRE;            // candidate slots of an image
constexpr int BBT_PER = (BBT_MAXN + BBT_SEL_NT - 1) / BBT_SEL_NT;     // consecutive slots a thread of the sampling workgroup owns

__device__ __forceinline__ float bbt_nan() { return __builtin_nanf(""); }
// torch.max / torch.min / clamp(min=) of two values: a NaN operand gives NaN (fmaxf / fminf would drop it)
__device__ __forceinline__ float bbt_pmax(float a, float b) { return (a != a || b != b) ? bbt_nan() : fmaxf(a, b); }
__device__ __forceinline__ float bbt_pmin(float a, float b) { return (a != a || b != b) ? bbt_nan() : fminf(a, b); }

// bbox_overlaps(gt, box) in its fp32 order (rpnt_iou's instructions on NaN-free inputs), NaN-propagating like the torch ops
__device__ __forceinline__ float bbt_iou(float gx1, float gy1, float gx2, float gy2, float garea, const RpntBox& an, float aarea) {
  const float w = bbt_pmax(bbt_pmin(gx2, an.x2) - bbt_pmax(gx1, an.x1), 0.f);
  const float h = bbt_pmax(bbt_pmin(gy2, an.y2) - bbt_pmax(gy1, an.y1), 0.f);
  const float overlap = w * h;
  const float uni = bbt_pmax(garea + aarea - overlap, 1e-6f);
  return overlap / uni;
}

// the row range [lo, hi) of image b, clamped into [0, R]
__device__ __forceinline__ void bbt_range(const int* first, const int* count, int stride, int b, int R, int& lo, int& hi) {
  lo = first != nullptr ? first[(long)b * stride] : 0;
  hi = count != nullptr ? count[(long)b * stride] : R;
  lo = lo < 0 ? 0 : (lo > R ? R : lo);
  hi = hi < 0 ? 0 : (hi > R ? R : hi);
}

__device__ __forceinline__ unsigned bbt_seed(unsigned seed, int stage) { return seed ^ rpnt_mix(0x5bd1e995u + (unsigned)stage); }

__global__ __launch_bounds__(BBT_NT) void bbt_assign_kernel(hrf_bbox_train_cfg_t cfg, int R, const float* rois_in, const int* first,
                                                            const int* count, int rstride, const float* gt, const int* gt_count, int Gmax,
                                                            int* assigned, float* max_iou) {
  __shared__ float s_gt[HRF_RPN_MAX_GT][5];
  const int b = blockIdx.y, N = Gmax + R;
  const int G = rpnt_count(gt_count, b, Gmax);
  rpnt_stage(gt, b, Gmax, G, s_gt);
  __syncthreads();
  const int c = blockIdx.x * BBT_NT + (int)threadIdx.x;
  if (c >= N) return;
  const long o = (long)b * N + c;
  if (c < Gmax) {                              // a ground truth as a proposal (AssignResult.add_gt_)
    const bool v = cfg.add_gt_as_proposals != 0 && c < G;
    assigned[o] = v ? c + 1 : -2; max_iou[o] = v ? 1.f : 0.f;
    return;
  }
  int lo, hi;
  bbt_range(first, count, rstride, b, R, lo, hi);
  const int r = c - Gmax;
  if (r < lo || r >= hi) { assigned[o] = -2; max_iou[o] = 0.f; return; }             // (the row is never read)
  if (G == 0) { assigned[o] = 0; max_iou[o] = 0.f; return; }
  const float* p = rois_in + ((long)b * R + r) * 5;
  RpntBox an;
  an.x1 = p[1]; an.y1 = p[2]; an.x2 = p[3]; an.y2 = p[4];
  const float aarea = (an.x2 - an.x1) * (an.y2 - an.y1);
  float best = -1.f;
  int arg = 0;
  bool nan = false;
  for (int g = 0; g < G; ++g) {
    const float v = bbt_iou(s_gt[g][0], s_gt[g][1], s_gt[g][2], s_gt[g][3], s_gt[g][4], an, aarea);
    nan = nan || v != v;
    if (v > best) { best = v; arg = g; }
  }
  int a = -1;
  if (nan) best = bbt_nan();
  else {
    if (best >= 0.f && best < cfg.neg_iou_thr) a = 0;
    if (best >= cfg.pos_iou_thr) a = arg + 1;
  }
  assigned[o] = a; max_iou[o] = best;
}

// the exclusive bound T of the k smallest codes among the slots of one class (kind 0: assigned > 0, 1: assigned == 0), cnt members:
// a member is sampled iff its code < T.  rpnt_select_kernel's radix select on codes held in LDS.  Block-uniform; every thread calls it.
__device__ __forceinline__ rpn_u64 bbt_select(const int* s_a, const rpn_u64* s_code, int N, int kind, int k, int cnt, unsigned* s_hist,
                                              unsigned* s_ctl) {
  if (k <= 0) return 0ull;
  if (k >= cnt) return ~0ull;                  // (every code is below: its low word is a slot index)
  const int tid = threadIdx.x;
  rpn_u64 Pf = 0ull, M = 0ull;
  unsigned want = (unsigned)k;
  int sh = 0;
  for (int pass = 0; pass < 6; ++pass) {       // key bytes 7..4, then the two index bytes that can differ (N <= BBT_MAXN < 2^16)
    const int byte = pass < 4 ? 7 - pass : 5 - pass;
    sh = 8 * byte;
    if (tid < 256) s_hist[tid] = 0u;
    if (tid == 0) { s_ctl[0] = 0u; s_ctl[1] = 1u; s_ctl[2] = 1u; }
    __syncthreads();
    for (int i = tid; i < N; i += BBT_SEL_NT) {
      const int a = s_a[i];
      const rpn_u64 c = s_code[i];
      if ((kind ? a == 0 : a > 0) && ((c ^ Pf) & M) == 0ull) atomicAdd(&s_hist[(unsigned)(c >> sh) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 256) {                           // bin `tid` holds the wanted code when  below < want <= below + its count  (one bin does)
      unsigned below = 0u;
      for (int d = 0; d < 255; ++d) below += d < tid ? s_hist[d] : 0u;
      const unsigned mine = s_hist[tid];
      if (below < want && want <= below + mine) { s_ctl[0] = (unsigned)tid; s_ctl[1] = want - below; s_ctl[2] = (mine == want - below) ? 1u : 0u; }
    }
    __syncthreads();
    Pf |= (rpn_u64)s_ctl[0] << sh; M |= 0xffull << sh;
    want = s_ctl[1];
    const bool done = s_ctl[2] != 0u;
    if (pass == 3) M |= 0xffff0000ull;         // those index bytes are 0 in every code
    __syncthreads();
    if (done) break;                           // (block-uniform) every code under this prefix is taken; the last pass always ends here
  }
  rpn_u64 T = (Pf | ((1ull << sh) - 1ull)) + 1ull;                    // every code under the prefix found so far, and nothing above it
  if (T == 0ull) T = ~0ull;
  return T;
}

__global__ __launch_bounds__(BBT_SEL_NT) void bbt_sample_kernel(hrf_bbox_train_cfg_t cfg, int R, const float* rois_in, const float* gt,
                                                                const int* gt_labels, int Gmax, const unsigned* keys, const unsigned* rng_state,
                                                                int stage, const int* assigned, float* rois_s, int* labels, float* bbox_targets,
                                                                int* src, int* counts) {
  __shared__ rpn_u64 s_code[BBT_MAXN];
  __shared__ int s_a[BBT_MAXN];
  __shared__ unsigned s_scan[2][BBT_SEL_NT];
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_ctl[4];
  const int b = blockIdx.x, tid = threadIdx.x, N = Gmax + R, num = cfg.num;
  const unsigned seed = keys == nullptr ? bbt_seed(rng_state[0], stage) : 0u, counter = keys == nullptr ? rng_state[1] : 0u;
  if (tid < 3) s_ctl[tid] = 0u;
  __syncthreads();
  {
    unsigned p = 0u, q = 0u;
    for (int i = tid; i < N; i += BBT_SEL_NT) {
      const int a = assigned[(long)b * N + i];
      s_a[i] = a;
      s_code[i] = rpnt_code(keys, seed, counter, b, N, i);
      p += a > 0 ? 1u : 0u; q += a == 0 ? 1u : 0u;
    }
    if (p) atomicAdd(&s_ctl[0], p);
    if (q) atomicAdd(&s_ctl[1], q);
  }
  __syncthreads();
  const int P = (int)s_ctl[0], Q = (int)s_ctl[1];
  __syncthreads();
  const int npos = min(P, cfg.num_pos), nneg = min(Q, num - npos);
  const rpn_u64 Tp = bbt_select(s_a, s_code, N, 0, npos, P, s_hist, s_ctl);
  __syncthreads();
  const rpn_u64 Tn = bbt_select(s_a, s_code, N, 1, nneg, Q, s_hist, s_ctl);
  // the sampled flags of this thread's slots c0 .. c0 + BBT_PER - 1 and their exclusive scan (positives low half, negatives high half)
  const int c0 = tid * BBT_PER;
  int flag[BBT_PER];
  unsigned mine = 0u, gts = 0u;
#pragma unroll
  for (int u = 0; u < BBT_PER; ++u) {
    const int c = c0 + u;
    flag[u] = 0;
    if (c < N) {
      const int a = s_a[c];
      if (a > 0 && s_code[c] < Tp) { flag[u] = 1; mine += 1u; gts += c < Gmax ? 1u : 0u; }
      else if (a == 0 && s_code[c] < Tn) { flag[u] = -1; mine += 1u << 16; }
    }
  }
  if (tid == 0) s_ctl[3] = 0u;
  s_scan[0][tid] = mine;
  __syncthreads();
  if (gts) atomicAdd(&s_ctl[3], gts);
  int cur = 0;
  for (int d = 1; d < BBT_SEL_NT; d <<= 1) {
    const unsigned v = s_scan[cur][tid] + (tid >= d ? s_scan[cur][tid - d] : 0u);
    s_scan[cur ^ 1][tid] = v;
    cur ^= 1;
    __syncthreads();
  }
  const unsigned before = s_scan[cur][tid] - mine;                    // (npos, nneg <= num <= 2048: the halves never carry)
  const int ngts = (int)s_ctl[3];
  int ip = (int)(before & 0xffffu), in = (int)(before >> 16);
#pragma unroll
  for (int u = 0; u < BBT_PER; ++u) {
    if (flag[u] == 0) continue;
    const int c = c0 + u, a = s_a[c];
    const int row = flag[u] > 0 ? ip++ : npos + in++;
    if (row >= num) continue;                  // (never: exactly npos + nneg <= num codes lie below the two bounds)
    const long o = (long)b * num + row;
    float bx[4];
    if (c < Gmax) { const float* g = gt + ((long)b * Gmax + c) * 4; bx[0] = g[0]; bx[1] = g[1]; bx[2] = g[2]; bx[3] = g[3]; }
    else { const float* p = rois_in + ((long)b * R + (c - Gmax)) * 5; bx[0] = p[1]; bx[1] = p[2]; bx[2] = p[3]; bx[3] = p[4]; }
    float* ro = rois_s + o * 5;
    ro[0] = (float)b; ro[1] = bx[0]; ro[2] = bx[1]; ro[3] = bx[2]; ro[4] = bx[3];
    float t4[4] = {0.f, 0.f, 0.f, 0.f};
    int lab = cfg.num_classes;
    if (flag[u] > 0) {                         // bbox2delta(box, gt[a - 1]) / stds (means 0)
      const float* g = gt + ((long)b * Gmax + (a - 1)) * 4;
      lab = gt_labels[(long)b * Gmax + (a - 1)];
      const float px = (bx[0] + bx[2]) * 0.5f, py = (bx[1] + bx[3]) * 0.5f, pw = bx[2] - bx[0], ph = bx[3] - bx[1];
      const float gx = (g[0] + g[2]) * 0.5f, gy = (g[1] + g[3]) * 0.5f, gw = g[2] - g[0], gh = g[3] - g[1];
      t4[0] = (gx - px) / pw / cfg.stds[0]; t4[1] = (gy - py) / ph / cfg.stds[1];
      t4[2] = logf(gw / pw) / cfg.stds[2]; t4[3] = logf(gh / ph) / cfg.stds[3];
    }
    labels[o] = lab; src[o] = c;
    float* to = bbox_targets + o * 4;
    to[0] = t4[0]; to[1] = t4[1]; to[2] = t4[2]; to[3] = t4[3];
  }
  const int n = npos + nneg;
  for (int row = n + tid; row < num; row += BBT_SEL_NT) {             // padding: (b, 0, 0, 0, 0), label -1, no target, no source
    const long o = (long)b * num + row;
    float* ro = rois_s + o * 5;
    ro[0] = (float)b; ro[1] = 0.f; ro[2] = 0.f; ro[3] = 0.f; ro[4] = 0.f;
    labels[o] = -1; src[o] = -1;
    float* to = bbox_targets + o * 4;
    to[0] = 0.f; to[1] = 0.f; to[2] = 0.f; to[3] = 0.f;
  }
  if (tid == 0) {
    int* cn = counts + 6 * b;
    cn[0] = P; cn[1] = Q; cn[2] = npos; cn[3] = nneg; cn[4] = ngts; cn[5] = n;
  }
}

// n = sum_b n_b, every n_b clamped into [0, num]
__device__ __forceinline__ int bbt_rows(const int* counts, int B, int num) {
  int n = 0;
  for (int b = 0; b < B; ++b) { const int v = counts[6 * b + 5]; n += v < 0 ? 0 : (v > num ? num : v); }
  return n;
}

__global__ __launch_bounds__(BBT_NT) void bbt_loss_kernel(hrf_bbox_train_cfg_t cfg, int B, const float* out, int ld, const int* labels,
                                                          const float* bbox_targets, const int* counts, float* d_out, int ld_d, double* slots) {
  __shared__ double s_sum[3][BBT_NT];
  const int tid = threadIdx.x, nc = cfg.num_classes, ncol = nc + 1, width = (nc + 5 + 15) / 16 * 16;
  const long rows = (long)B * cfg.num, row = (long)blockIdx.x * BBT_NT + tid;
  double lc = 0.0, lb = 0.0, ok = 0.0;
  if (row < rows) {
    const int n = bbt_rows(counts, B, cfg.num);
    const int lab = labels[row];
    float* d = d_out + row * ld_d;
    if (lab < 0 || lab > nc) {                 // padding (or a label no class has): no loss, a zero gradient row
      for (int j = 0; j < width; ++j) d[j] = 0.f;
    } else {
      const float* x = out + row * ld;
      const float sc = cfg.loss_weight_cls / (float)max(n, 1), sb = cfg.loss_weight_bbox / (float)max(n, 1);
      float m = x[0];
      int top = 0;
      for (int j = 1; j < ncol; ++j) { const float v = x[j]; if (v > m) { m = v; top = j; } }
      float sum = 0.f;
      for (int j = 0; j < ncol; ++j) sum += expf(x[j] - m);
      lc = (double)((m + logf(sum)) - x[lab]);
      ok = top == lab ? 1.0 : 0.0;
      for (int j = 0; j < ncol; ++j) d[j] = (expf(x[j] - m) / sum - (j == lab ? 1.f : 0.f)) * sc;
      float g4[4] = {0.f, 0.f, 0.f, 0.f};
      if (lab < nc) {
        const float* t = bbox_targets + row * 4;
        for (int c = 0; c < 4; ++c) {
          const float df = x[ncol + c] - t[c], ad = fabsf(df);
          if (ad < cfg.beta) { lb += (double)(0.5f * ad * ad / cfg.beta); g4[c] = df / cfg.beta * sb; }
          else { lb += (double)(ad - 0.5f * cfg.beta); g4[c] = (df > 0.f ? 1.f : df < 0.f ? -1.f : df) * sb; }
        }
      }
      for (int c = 0; c < 4; ++c) d[ncol + c] = g4[c];
      for (int j = nc + 5; j < width; ++j) d[j] = 0.f;
    }
  }
  s_sum[0][tid] = lc; s_sum[1][tid] = lb; s_sum[2][tid] = ok;
  __syncthreads();
  for (int s = BBT_NT / 2; s > 0; s >>= 1) {
    if (tid < s) { s_sum[0][tid] += s_sum[0][tid + s]; s_sum[1][tid] += s_sum[1][tid + s]; s_sum[2][tid] += s_sum[2][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = slots + (long)blockIdx.x * 3;
    o[0] = s_sum[0][0]; o[1] = s_sum[1][0]; o[2] = s_sum[2][0];
  }
}

__global__ __launch_bounds__(64) void bbt_finalize_kernel(hrf_bbox_train_cfg_t cfg, int B, int nblk, const double* slots, const int* counts,
                                                          float* losses, unsigned* rng_state) {
  __shared__ double s_p[3][64];
  const int lane = threadIdx.x;
  double c = 0.0, r = 0.0, k = 0.0;
  for (int q = lane; q < nblk; q += 64) { const double* p = slots + (long)q * 3; c += p[0]; r += p[1]; k += p[2]; }
  s_p[0][lane] = c; s_p[1][lane] = r; s_p[2][lane] = k;
  __syncthreads();
  if (lane == 0) {
    const int n = bbt_rows(counts, B, cfg.num);
    double sc = 0.0, sr = 0.0, sk = 0.0;
    for (int j = 0; j < 64; ++j) { sc += s_p[0][j]; sr += s_p[1][j]; sk += s_p[2][j]; }
    losses[0] = (float)(sc / (double)max(n, 1) * (double)cfg.loss_weight_cls);
    losses[1] = n > 0 ? (float)(sr / (double)n * (double)cfg.loss_weight_bbox) : 0.f;
    losses[2] = n > 0 ? (float)(100.0 * sk / (double)n) : 0.f;
    if (rng_state != nullptr) rng_state[1] += 1u;
  }
}

// measurement aid (hrf_debug_knob 48, tools/roi_loss_cost.py): k > 0 = return after launch k of the stage (1, 2: hrf_bbox_targets;
// 3, 4: hrf_bbox_loss), incomplete outputs
static int g_bbt_stop = 0;
#define BBT_STEP(k) { if (hrf_check_launch() != HRF_OK) return HRF_ERR_LAUNCH; if (g_bbt_stop == (k)) return HRF_OK; }

bool bbt_finite_pos(float v) { return v > 0.f && v < 3.0e38f; }       // (NaN fails)

bool bbt_check(const hrf_bbox_train_cfg_t* c, int B, int R, int Gmax) {
  if (c == nullptr || B < 1 || B > 65535 || R < 1 || R > HRF_RPN_MAX_PRE || Gmax < 1 || Gmax > HRF_RPN_MAX_GT) return false;
  if (!(c->pos_iou_thr >= 0.f && c->pos_iou_thr <= 1.f) || !(c->neg_iou_thr >= 0.f && c->neg_iou_thr <= 1.f) ||
      !(c->min_pos_iou >= 0.f && c->min_pos_iou <= 1.f)) return false;                               // (NaN fails)
  if (c->num < 1 || c->num > HRF_RPN_MAX_PRE || c->num_pos < 0 || c->num_pos > c->num) return false;
  if (c->num_classes < 1 || c->num_classes > HRF_BBOX_MAX_CLASSES) return false;
  for (int k = 0; k < 4; ++k)
    if (!bbt_finite_pos(c->stds[k])) return false;
  if (!bbt_finite_pos(c->beta)) return false;
  if (!(fabsf(c->loss_weight_cls) < 3.0e38f) || !(fabsf(c->loss_weight_bbox) < 3.0e38f)) return false;
  return true;
}

long bbt_blocks(const hrf_bbox_train_cfg_t* c, int B) { return ((long)B * c->num + BBT_NT - 1) / BBT_NT; }
long bbt_bytes(const hrf_bbox_train_cfg_t* c, int B) { return rpn_align(bbt_blocks(c, B) * 3 * 8); }

}  // namespace

// (reached through hrf_debug_knob only: not exported)
extern "C" __attribute__((visibility("hidden"))) int hrf_bbt_knob(int key, int value) {
  if (key != 0 || value < 0 || value > 4) return HRF_ERR_ARG;
  g_bbt_stop = value;
  return HRF_OK;
}

extern "C" int hrf_bbox_train_supported(const hrf_bbox_train_cfg_t* cfg, int B, int R, int Gmax) { return bbt_check(cfg, B, R, Gmax) ? 1 : 0; }

extern "C" long hrf_bbox_train_workspace_bytes(const hrf_bbox_train_cfg_t* cfg, int B, int R, int Gmax) {
  return bbt_check(cfg, B, R, Gmax) ? bbt_bytes(cfg, B) : 0;
}

extern "C" int hrf_bbox_targets(const hrf_bbox_train_cfg_t* cfg, int B, int R, const float* rois_in, const int* first, const int* count,
                                int range_stride, const float* gt, const int* gt_labels, const int* gt_count, int Gmax, const unsigned* keys,
                                const unsigned* rng_state, int stage, float* rois_s, int* labels, float* bbox_targets, int* src, int* counts,
                                int* assigned, float* max_iou, void* stream) {
  if (!bbt_check(cfg, B, R, Gmax) || range_stride < 1 || stage < 0 || stage > 255) return HRF_ERR_ARG;
  if (rois_in == nullptr || gt == nullptr || gt_labels == nullptr || gt_count == nullptr || (keys == nullptr && rng_state == nullptr)) return HRF_ERR_ARG;
  if (rois_s == nullptr || labels == nullptr || bbox_targets == nullptr || src == nullptr || counts == nullptr || assigned == nullptr ||
      max_iou == nullptr) return HRF_ERR_ARG;
  const int N = Gmax + R;
  HRF_LAUNCH(bbt_assign_kernel, dim3((N + BBT_NT - 1) / BBT_NT, B), dim3(BBT_NT), 0, stream, *cfg, R, rois_in, first, count, range_stride, gt,
             gt_count, Gmax, assigned, max_iou);
  BBT_STEP(1)
  HRF_LAUNCH(bbt_sample_kernel, dim3(B), dim3(BBT_SEL_NT), 0, stream, *cfg, R, rois_in, gt, gt_labels, Gmax, keys, rng_state, stage,
             (const int*)assigned, rois_s, labels, bbox_targets, src, counts);
  return hrf_check_launch();
}

extern "C" int hrf_bbox_loss(const hrf_bbox_train_cfg_t* cfg, int B, const float* out, int ld, const int* labels, const float* bbox_targets,
                             const int* counts, void* workspace, long workspace_bytes, float* d_out, int ld_d, float* losses,
                             unsigned* rng_state, void* stream) {
  if (!bbt_check(cfg, B, 1, 1)) return HRF_ERR_ARG;
  const int width = (cfg->num_classes + 5 + 15) / 16 * 16;
  if (ld < cfg->num_classes + 5 || ld_d < width) return HRF_ERR_ARG;
  if (out == nullptr || labels == nullptr || bbox_targets == nullptr || counts == nullptr || d_out == nullptr || losses == nullptr) return HRF_ERR_ARG;
  if (workspace == nullptr || workspace_bytes < bbt_bytes(cfg, B)) return HRF_ERR_ARG;
  double* slots = static_cast<double*>(workspace);
  const int nblk = (int)bbt_blocks(cfg, B);
  HRF_LAUNCH(bbt_loss_kernel, dim3(nblk), dim3(BBT_NT), 0, stream, *cfg, B, out, ld, labels, bbox_targets, counts, d_out, ld_d, slots);
  BBT_STEP(3)
  HRF_LAUNCH(bbt_finalize_kernel, dim3(1), dim3(64), 0, stream, *cfg, B, nblk, (const double*)slots, counts, losses, rng_state);
  return hrf_check_launch();
}
