// RPN training targets and loss: anchor inside flags, MaxIoUAssigner, RandomSampler, BCE-with-logits + SmoothL1 and their
// gradients on the head's output maps (gfx950, NHWC fp32).
//
//   mmdet/core/anchor/anchor_generator.py:392-451 (valid_flags: valid_h = min(ceil(pad_h / stride), H), likewise the width),
//   mmdet/core/anchor/utils.py:21-47 (anchor_inside_flags: valid & x1 >= -border & y1 >= -border & x2 < img_w + border &
//   y2 < img_h + border; allowed_border < 0: valid alone), mmdet/models/dense_heads/anchor_head.py:239-245 (only inside anchors
//   take part), mmdet/core/bbox/iou_calculators/iou2d_calculator.py:213-253 (bbox_overlaps), mmdet/core/bbox/assigners/
//   max_iou_assigner.py:128-213 (assign_wrt_overlaps, gt_max_assign_all), mmdet/core/bbox/samplers/base_sampler.py:83-98 and
//   random_sampler.py:64-82 (num_pos = min(P, int(num * pos_fraction)), num_neg = min(Nneg, num - num_pos), uniform subsets),
//   mmdet/models/dense_heads/anchor_head.py:253-283 (targets), :383-384 (avg), :402-450 (loss_single), :498-520 (loss),
//   mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:118-160 (bbox2delta, means 0, stds 1), mmdet/models/dense_heads/rpn_head.py:70-101.
//
// Part of the translation unit pointwise.hip (included at its end, after hrf_rpn.h whose anchor convention, level table and
// RPN_SEL it uses).  Fixed-shape outputs, no host read of any input, no allocation, no synchronisation, no float atomics (the
// only atomics are integer adds in LDS: the same bits in deterministic mode and from run to run).  Every loop is bounded by a
// map size, Gmax or the eight radix passes, never by data; boxes, logits and deltas may be NaN / Inf.
//
// The anchors of all levels of an image form ONE list of N = sum_l H_l W_l A entries, level l at off_l = sum_{j<l} N_j, within
// a level the flat index (y W + x) A + a of hrf_rpn.h.  The per-anchor kernels run on a grid whose 256-thread blocks never
// straddle a level (RpntGrid).
//
//   1  rpnt_iou_kernel      per anchor: the image's gts staged in LDS, the anchor from (level, y, x, a), the inside flag, the loop
//                           over the gts in the fp32 order of bbox_overlaps (-ffp-contract=off: bit-defined):
//                             area = (x2-x1)*(y2-y1), wh = max(min(rb) - max(lt), 0), overlap = w*h,
//                             union = max(area_gt + area_anchor - overlap, 1e-6), iou = overlap / union;
//                           max_iou and the argmax (ties: the lowest gt) are written; argmax = -2 marks "not inside".
//   2  rpnt_gtmax_kernel    per (image, gt, slice): a workgroup strides over its slice of the inside anchors, recomputes the IoU with
//                           the same inline function and block-reduces the maximum (LDS tree: no atomics) into its own slot;
//                           32 slices per gt (one workgroup per gt left 60 workgroups on 256 CUs: 117 us of a 209 us call).  The
//                           maximum of the 32 slots - exact in any order - is taken where launch 3 stages gt_max[b][i].
//   3  rpnt_assign_kernel   per anchor: -1, then 0 where 0 <= max < neg_iou_thr, argmax + 1 where max >= pos_iou_thr, then with
//                           match_low_quality for i ascending: gt_max[i] >= min_pos_iou and iou(i, anchor) == gt_max[i] (fp32
//                           equality on the recomputed value - the same instructions on the same inputs) -> i + 1.
//                           No gts: 0.  Not inside: -2.
//   4  rpnt_select_kernel   per (image, {pos, neg}): one workgroup of 1024 counts the assigned positives P and negatives Q,
//                           k = min(P, num_pos) resp. min(Q, num - min(P, num_pos)), and finds by a radix select (8 bits per pass
//                           from the top, LDS histogram, at most 8 passes) the k-th SMALLEST 64-bit code key << 32 | index among
//                           its class.  Only an exclusive bound T is kept: an anchor is sampled iff its code < T.
//   5  rpnt_loss_kernel     per anchor: sampled = +1 / -1 / 0; with LOSS: w = sampled != 0, t = sampled > 0,
//                           bce = max(x,0) - x t + log1p(exp(-|x|)), d_cls = w (sigmoid(x) - t) lw_cls / avg; for a sampled positive
//                           the target bbox2delta(anchor, gt[assigned - 1]) is computed on the fly, SmoothL1(beta) per coordinate,
//                           d_reg = (|d| < beta ? d / beta : sign(d)) lw_bbox / avg, zero elsewhere: EVERY element of the gradient
//                           maps is written.  avg = sum_b max(npos_b, 1) + max(nneg_b, 1) is read from the device counts.  The
//                           block's two sums (fp64, LDS tree) go into its own slot.
//   6  rpnt_finalize_kernel one wave per level folds the level's slots in slot order (lane j: slots j, j + 64, ...; then the 64 lane
//                           sums in lane order), writes losses[0][l] = lw_cls sum / avg, losses[1][l] = lw_bbox sum / avg and
//                           advances the counter of rng_state.
//
// SAMPLING.  A uniform subset of size k = the k members with the smallest (key, index).  key = keys[b][n] when an explicit array
// is given, otherwise rpnt_hash(seed, counter, b, n) with (seed, counter) = rng_state[0], rng_state[1] read on the device:
//   mix(h) = h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16     (all mod 2^32)
//   key = mix(mix(mix(mix(seed + 0x9e3779b9) ^ counter) + b) ^ n)
// (hrfuser_amd.testing.rpn_key_ref restates it).  This reproduces the reference's distribution, not its randperm stream.
#pragma once

namespace {

constexpr int RPNT_NT = 256;                   // per-anchor kernels
constexpr int RPNT_SEL_NT = 1024;              // the select workgroup
constexpr int RPNT_SLICES = 32;                // workgroups per (image, gt) of the per-gt maximum: slice s takes anchors s 256 + t, + 32 * 256, ...
constexpr int RPNT_UNROLL = 8;                 // loads a thread of the select workgroup issues before it uses the first

// the per-anchor grid: blocks boff[l] .. boff[l + 1] - 1 cover level l, anchors noff[l] .. of the image's list
struct RpntGrid {
  int nlev, N, nblk;
  int n[HRF_RPN_MAX_LEVELS];
  int noff[HRF_RPN_MAX_LEVELS];
  int boff[HRF_RPN_MAX_LEVELS];
};

struct RpntBox { float x1, y1, x2, y2; };

__device__ __forceinline__ RpntBox rpnt_anchor(const hrf_rpn_levels_t& lv, int l, int i) {
  const int A = lv.A, W = RPN_SEL(lv.W, l);
  const int pix = i / A, a = i - pix * A, y = pix / W, x = pix - y * W;
  const float stride = (float)RPN_SEL(lv.stride, l);
  const float* ba = lv.base_anchors + (l * HRF_RPN_MAX_ANCHORS + a) * 4;
  const float sx = (float)x * stride, sy = (float)y * stride;
  RpntBox r;
  r.x1 = ba[0] + sx; r.y1 = ba[1] + sy; r.x2 = ba[2] + sx; r.y2 = ba[3] + sy;
  return r;
}

// valid flag (anchor_generator.py:392-451) and inside flag (utils.py:21-47) of anchor i of level l
__device__ __forceinline__ bool rpnt_inside(int A, int H, int W, int s, int i, const RpntBox& an, float img_h, float img_w, float pad_h,
                                            float pad_w, int border) {
  const int pix = i / A, y = pix / W, x = pix - y * W;
  // pad_h / pad_w are whole numbers of pixels; anything else (NaN, negative, huge) is clamped into [0, H s] first
  const float ph = pad_h > 0.f ? fminf(pad_h, (float)H * (float)s) : 0.f, pw = pad_w > 0.f ? fminf(pad_w, (float)W * (float)s) : 0.f;
  const int vh = min(((int)ceilf(ph) + s - 1) / s, H), vw = min(((int)ceilf(pw) + s - 1) / s, W);
  const bool valid = y < vh && x < vw;
  if (border < 0) return valid;
  const float bd = (float)border;
  return valid && an.x1 >= -bd && an.y1 >= -bd && an.x2 < img_w + bd && an.y2 < img_h + bd;
}

// bbox_overlaps(gt, anchor) in its fp32 order; garea / aarea = (x2-x1)*(y2-y1) of either
__device__ __forceinline__ float rpnt_iou(float gx1, float gy1, float gx2, float gy2, float garea, const RpntBox& an, float aarea) {
  const float w = fmaxf(fminf(gx2, an.x2) - fmaxf(gx1, an.x1), 0.f);
  const float h = fmaxf(fminf(gy2, an.y2) - fmaxf(gy1, an.y1), 0.f);
  const float overlap = w * h;
  const float uni = fmaxf(garea + aarea - overlap, 1e-6f);
  return overlap / uni;
}

__device__ __forceinline__ unsigned rpnt_mix(unsigned h) {
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  return h;
}

__device__ __forceinline__ unsigned rpnt_hash(unsigned seed, unsigned counter, unsigned b, unsigned n) {
  return rpnt_mix(rpnt_mix(rpnt_mix(rpnt_mix(seed + 0x9e3779b9u) ^ counter) + b) ^ n);
}

__device__ __forceinline__ rpn_u64 rpnt_code(const unsigned* keys, unsigned seed, unsigned counter, int b, int N, int n) {
  const unsigned key = keys != nullptr ? keys[(long)b * N + n] : rpnt_hash(seed, counter, (unsigned)b, (unsigned)n);
  return ((rpn_u64)key << 32) | (rpn_u64)(unsigned)n;
}

__device__ __forceinline__ int rpnt_count(const int* gt_count, int b, int Gmax) {
  const int g = gt_count[b];
  return g < 0 ? 0 : (g > Gmax ? Gmax : g);
}

// stage the G gts of image b and their areas (blockDim-strided; the caller synchronises)
__device__ __forceinline__ void rpnt_stage(const float* gt, int b, int Gmax, int G, float (*s_gt)[5]) {
  for (int i = threadIdx.x; i < G; i += blockDim.x) {
    const float* g = gt + ((long)b * Gmax + i) * 4;
    const float x1 = g[0], y1 = g[1], x2 = g[2], y2 = g[3];
    s_gt[i][0] = x1; s_gt[i][1] = y1; s_gt[i][2] = x2; s_gt[i][3] = y2;
    s_gt[i][4] = (x2 - x1) * (y2 - y1);
  }
}

// -> false: no anchor for this thread; otherwise its level l, index i in the level and n in the image's list
__device__ __forceinline__ bool rpnt_locate(const RpntGrid& tg, int& l, int& i, int& n) {
  const int blk = blockIdx.x;
  l = 0;
  while (l + 1 < tg.nlev && blk >= RPN_SEL(tg.boff, l + 1)) ++l;
  i = (blk - RPN_SEL(tg.boff, l)) * RPNT_NT + (int)threadIdx.x;
  n = RPN_SEL(tg.noff, l) + i;
  return i < RPN_SEL(tg.n, l);
}

__global__ __launch_bounds__(RPNT_NT) void rpnt_iou_kernel(hrf_rpn_levels_t lv, RpntGrid tg, hrf_rpn_train_cfg_t cfg, const float* img_shape,
                                                           const float* pad_shape, const float* gt, const int* gt_count, int Gmax,
                                                           float* max_iou, int* argmax) {
  __shared__ float s_gt[HRF_RPN_MAX_GT][5];
  const int b = blockIdx.y;
  const int G = rpnt_count(gt_count, b, Gmax);
  rpnt_stage(gt, b, Gmax, G, s_gt);
  __syncthreads();
  int l, i, n;
  if (!rpnt_locate(tg, l, i, n)) return;
  const RpntBox an = rpnt_anchor(lv, l, i);
  const long o = (long)b * tg.N + n;
  if (!rpnt_inside(lv.A, RPN_SEL(lv.H, l), RPN_SEL(lv.W, l), RPN_SEL(lv.stride, l), i, an, img_shape[2 * b], img_shape[2 * b + 1], pad_shape[2 * b], pad_shape[2 * b + 1], cfg.allowed_border)) {
    max_iou[o] = 0.f; argmax[o] = -2;
    return;
  }
  const float aarea = (an.x2 - an.x1) * (an.y2 - an.y1);
  float best = G > 0 ? -1.f : 0.f;             // (no gts: max_overlaps = 0; all-NaN IoUs: -1, which no threshold arm takes)
  int arg = 0;
  for (int g = 0; g < G; ++g) {
    const float v = rpnt_iou(s_gt[g][0], s_gt[g][1], s_gt[g][2], s_gt[g][3], s_gt[g][4], an, aarea);
    if (v > best) { best = v; arg = g; }
  }
  max_iou[o] = best; argmax[o] = arg;
}

__global__ __launch_bounds__(RPNT_NT) void rpnt_gtmax_kernel(hrf_rpn_levels_t lv, RpntGrid tg, const float* gt, const int* gt_count, int Gmax,
                                                             const int* argmax, float* gt_part) {
  __shared__ float s_m[RPNT_NT];
  const int g = blockIdx.x, b = blockIdx.y, sl = blockIdx.z, tid = threadIdx.x;
  const int G = rpnt_count(gt_count, b, Gmax);
  if (g >= G) return;                          // (block-uniform; the partials of gts past the count are never read)
  const float* p = gt + ((long)b * Gmax + g) * 4;
  const float gx1 = p[0], gy1 = p[1], gx2 = p[2], gy2 = p[3];
  const float garea = (gx2 - gx1) * (gy2 - gy1);
  float m = -1.f;
  for (int l = 0; l < tg.nlev; ++l) {
    const int nl = RPN_SEL(tg.n, l);
    const int* am = argmax + (long)b * tg.N + RPN_SEL(tg.noff, l);
    for (int i = sl * RPNT_NT + tid; i < nl; i += RPNT_SLICES * RPNT_NT) {
      if (am[i] == -2) continue;
      const RpntBox an = rpnt_anchor(lv, l, i);
      const float v = rpnt_iou(gx1, gy1, gx2, gy2, garea, an, (an.x2 - an.x1) * (an.y2 - an.y1));
      if (v > m) m = v;
    }
  }
  s_m[tid] = m;
  __syncthreads();
  for (int s = RPNT_NT / 2; s > 0; s >>= 1) {
    if (tid < s && s_m[tid + s] > s_m[tid]) s_m[tid] = s_m[tid + s];
    __syncthreads();
  }
  if (tid == 0) gt_part[((long)b * Gmax + g) * RPNT_SLICES + sl] = s_m[0];
}

__global__ __launch_bounds__(RPNT_NT) void rpnt_assign_kernel(hrf_rpn_levels_t lv, RpntGrid tg, hrf_rpn_train_cfg_t cfg, const float* gt,
                                                              const int* gt_count, int Gmax, const float* max_iou, const int* argmax,
                                                              const float* gt_part, int* assigned) {
  __shared__ float s_gt[HRF_RPN_MAX_GT][5];
  __shared__ float s_gm[HRF_RPN_MAX_GT];
  const int b = blockIdx.y;
  const int G = rpnt_count(gt_count, b, Gmax);
  rpnt_stage(gt, b, Gmax, G, s_gt);
  for (int g = threadIdx.x; g < G; g += RPNT_NT) {             // the maximum of the slices' maxima: exact, whatever the order
    const float* pp = gt_part + ((long)b * Gmax + g) * RPNT_SLICES;
    float m = -1.f;
    for (int sl = 0; sl < RPNT_SLICES; ++sl) m = pp[sl] > m ? pp[sl] : m;
    s_gm[g] = m;
  }
  __syncthreads();
  int l, i, n;
  if (!rpnt_locate(tg, l, i, n)) return;
  const long o = (long)b * tg.N + n;
  const int arg = argmax[o];
  if (arg == -2) { assigned[o] = -2; return; }
  if (G == 0) { assigned[o] = 0; return; }
  const float mx = max_iou[o];
  int a = -1;
  if (mx >= 0.f && mx < cfg.neg_iou_thr) a = 0;
  if (mx >= cfg.pos_iou_thr) a = arg + 1;
  if (cfg.match_low_quality) {
    const RpntBox an = rpnt_anchor(lv, l, i);
    const float aarea = (an.x2 - an.x1) * (an.y2 - an.y1);
    for (int g = 0; g < G; ++g) {
      const float gm = s_gm[g];
      if (!(gm >= cfg.min_pos_iou)) continue;
      if (rpnt_iou(s_gt[g][0], s_gt[g][1], s_gt[g][2], s_gt[g][3], s_gt[g][4], an, aarea) == gm) a = g + 1;
    }
  }
  assigned[o] = a;
}

// thr[b][kind]: the exclusive bound of the sampled codes of the class; counts[b] = (P, Q, sampled pos, sampled neg)
__global__ __launch_bounds__(RPNT_SEL_NT) void rpnt_select_kernel(int N, hrf_rpn_train_cfg_t cfg, const int* assigned, const unsigned* keys,
                                                                  const unsigned* rng_state, rpn_u64* thr, int* counts) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_ctl[4];                // (P, Q) first; then digit, still wanted, done
  const int kind = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int* asg = assigned + (long)b * N;
  const unsigned seed = keys == nullptr ? rng_state[0] : 0u, counter = keys == nullptr ? rng_state[1] : 0u;
  if (tid < 2) s_ctl[tid] = 0u;
  __syncthreads();
  {
    unsigned p = 0u, q = 0u;
    for (int i0 = tid; i0 < N; i0 += RPNT_SEL_NT * RPNT_UNROLL) {
      int a[RPNT_UNROLL];
#pragma unroll
      for (int u = 0; u < RPNT_UNROLL; ++u) a[u] = asg[min(i0 + u * RPNT_SEL_NT, N - 1)];
#pragma unroll
      for (int u = 0; u < RPNT_UNROLL; ++u)
        if (i0 + u * RPNT_SEL_NT < N) { p += a[u] > 0 ? 1u : 0u; q += a[u] == 0 ? 1u : 0u; }
    }
    if (p) atomicAdd(&s_ctl[0], p);
    if (q) atomicAdd(&s_ctl[1], q);
  }
  __syncthreads();
  const int P = (int)s_ctl[0], Q = (int)s_ctl[1];
  __syncthreads();
  const int npos = min(P, cfg.num_pos), nneg = min(Q, cfg.num - npos);
  const int cnt = kind ? Q : P, k = kind ? nneg : npos;
  if (tid == 0) { counts[4 * b + kind] = cnt; counts[4 * b + 2 + kind] = k; }
  rpn_u64 T;
  if (k <= 0) T = 0ull;
  else if (k >= cnt) T = ~0ull;                // (every code is below: its low word is an index < 2^31)
  else {
    const int nbytes = N <= (1 << 8) ? 1 : N <= (1 << 16) ? 2 : N <= (1 << 24) ? 3 : 4;              // index bytes that can differ
    rpn_u64 Pf = 0ull, M = 0ull;
    unsigned want = (unsigned)k;
    int sh = 0;
    for (int pass = 0; pass < 4 + nbytes; ++pass) {
      const int byte = pass < 4 ? 7 - pass : nbytes - 1 - (pass - 4);
      sh = 8 * byte;
      if (tid < 256) s_hist[tid] = 0u;
      if (tid == 0) { s_ctl[0] = 0u; s_ctl[1] = 1u; s_ctl[2] = 1u; }
      __syncthreads();
      for (int i0 = tid; i0 < N; i0 += RPNT_SEL_NT * RPNT_UNROLL) {     // RPNT_UNROLL independent loads in flight per thread
        int a[RPNT_UNROLL];
        rpn_u64 c[RPNT_UNROLL];
#pragma unroll
        for (int u = 0; u < RPNT_UNROLL; ++u) {
          const int i = min(i0 + u * RPNT_SEL_NT, N - 1);
          a[u] = asg[i];
          c[u] = rpnt_code(keys, seed, counter, b, N, i);
        }
#pragma unroll
        for (int u = 0; u < RPNT_UNROLL; ++u)
          if (i0 + u * RPNT_SEL_NT < N && (kind ? a[u] == 0 : a[u] > 0) && ((c[u] ^ Pf) & M) == 0ull)
            atomicAdd(&s_hist[(unsigned)(c[u] >> sh) & 255u], 1u);
      }
      __syncthreads();
      if (tid < 256) {                         // bin `tid` holds the wanted code when  below < want <= below + its count  (one bin does)
        unsigned below = 0u;
        for (int d = 0; d < 255; ++d) below += d < tid ? s_hist[d] : 0u;
        const unsigned mine = s_hist[tid];
        if (below < want && want <= below + mine) { s_ctl[0] = (unsigned)tid; s_ctl[1] = want - below; s_ctl[2] = (mine == want - below) ? 1u : 0u; }
      }
      __syncthreads();
      Pf |= (rpn_u64)s_ctl[0] << sh; M |= 0xffull << sh;
      want = s_ctl[1];
      const bool done = s_ctl[2] != 0u;
      if (pass == 3 && nbytes < 4) M |= (0xffffffffull >> (8 * nbytes)) << (8 * nbytes);             // those index bytes are 0 in every code
      __syncthreads();
      if (done) break;                         // (block-uniform) every code under this prefix is taken; the last pass always ends here
    }
    T = (Pf | ((1ull << sh) - 1ull)) + 1ull;   // every code under the prefix found so far, and nothing above it
    if (T == 0ull) T = ~0ull;                  // (the prefix was all ones: no code reaches ~0, its low word is an index)
  }
  if (tid == 0) thr[2 * b + kind] = T;
}

template <bool LOSS>
__global__ __launch_bounds__(RPNT_NT) void rpnt_loss_kernel(hrf_rpn_levels_t lv, RpntGrid tg, hrf_rpn_train_cfg_t cfg, hrf_rpn_grads_t gr,
                                                            const float* gt, int Gmax, const unsigned* keys, const unsigned* rng_state,
                                                            const int* assigned, const rpn_u64* thr, const int* counts, int* sampled,
                                                            double* slots) {
  __shared__ double s_sum[2][RPNT_NT];
  const int b = blockIdx.y, tid = threadIdx.x;
  int l, i, n;
  const bool have = rpnt_locate(tg, l, i, n);
  double lc = 0.0, lb = 0.0;
  if (have) {
    const long o = (long)b * tg.N + n;
    const int a = assigned[o];
    int s = 0;
    if (a >= 0) {
      const unsigned seed = keys == nullptr ? rng_state[0] : 0u, counter = keys == nullptr ? rng_state[1] : 0u;
      const rpn_u64 c = rpnt_code(keys, seed, counter, b, tg.N, n);
      if (c < thr[2 * b + (a > 0 ? 0 : 1)]) s = a > 0 ? 1 : -1;
    }
    sampled[o] = s;
    if (LOSS) {
      int tot = 0;
      for (int bb = 0; bb < lv.B; ++bb) tot += max(counts[4 * bb + 2], 1) + max(counts[4 * bb + 3], 1);
      const float avg = (float)tot;
      const int A = lv.A, pix = i / A, an_i = i - pix * A;
      const long HW = (long)RPN_SEL(lv.H, l) * RPN_SEL(lv.W, l);
      const long row = (long)b * HW + pix;
      float* dc = RPN_SEL(gr.d_cls, l) + row * RPN_SEL(gr.ld_cls, l) + an_i;
      float* dr = RPN_SEL(gr.d_reg, l) + row * RPN_SEL(gr.ld_reg, l) + 4 * an_i;
      float gc = 0.f, g4[4] = {0.f, 0.f, 0.f, 0.f};
      if (s != 0) {
        const float x = RPN_SEL(lv.cls, l)[row * RPN_SEL(lv.ld_cls, l) + an_i];
        const float t = s > 0 ? 1.f : 0.f;
        const float e = expf(-fabsf(x));
        lc = (double)(fmaxf(x, 0.f) - x * t + log1pf(e));
        const float sg = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        gc = (sg - t) * (cfg.loss_weight_cls / avg);
      }
      if (s > 0) {
        const RpntBox an = rpnt_anchor(lv, l, i);
        const float* g = gt + ((long)b * Gmax + (a - 1)) * 4;
        const float px = (an.x1 + an.x2) * 0.5f, py = (an.y1 + an.y2) * 0.5f, pw = an.x2 - an.x1, ph = an.y2 - an.y1;
        const float gx = (g[0] + g[2]) * 0.5f, gy = (g[1] + g[3]) * 0.5f, gw = g[2] - g[0], gh = g[3] - g[1];
        const float tg4[4] = {(gx - px) / pw, (gy - py) / ph, logf(gw / pw), logf(gh / ph)};
        const float* pr = RPN_SEL(lv.reg, l) + row * RPN_SEL(lv.ld_reg, l) + 4 * an_i;
        const float scale = cfg.loss_weight_bbox / avg;
        for (int c = 0; c < 4; ++c) {
          const float d = pr[c] - tg4[c], ad = fabsf(d);
          if (ad < cfg.beta) { lb += (double)(0.5f * ad * ad / cfg.beta); g4[c] = d / cfg.beta * scale; }
          else { lb += (double)(ad - 0.5f * cfg.beta); g4[c] = (d > 0.f ? 1.f : d < 0.f ? -1.f : d) * scale; }
        }
      }
      dc[0] = gc;
      for (int c = 0; c < 4; ++c) dr[c] = g4[c];
    }
  }
  if (LOSS) {
    s_sum[0][tid] = lc; s_sum[1][tid] = lb;
    __syncthreads();
    for (int s = RPNT_NT / 2; s > 0; s >>= 1) {
      if (tid < s) { s_sum[0][tid] += s_sum[0][tid + s]; s_sum[1][tid] += s_sum[1][tid + s]; }
      __syncthreads();
    }
    if (tid == 0) {
      double* o = slots + ((long)b * tg.nblk + blockIdx.x) * 2;
      o[0] = s_sum[0][0]; o[1] = s_sum[1][0];
    }
  }
}

// one wave per level: slot q of the level = (image q / nb, block q % nb)
__global__ __launch_bounds__(64) void rpnt_finalize_kernel(RpntGrid tg, hrf_rpn_train_cfg_t cfg, int B, const double* slots, const int* counts,
                                                           float* losses, unsigned* rng_state) {
  __shared__ double s_p[2][64];
  const int l = blockIdx.x, lane = threadIdx.x;
  const int b0 = RPN_SEL(tg.boff, l), nb = (RPN_SEL(tg.n, l) + RPNT_NT - 1) / RPNT_NT;
  double c = 0.0, r = 0.0;
  for (int q = lane; q < B * nb; q += 64) {
    const int b = q / nb, k = q - b * nb;
    const double* p = slots + ((long)b * tg.nblk + b0 + k) * 2;
    c += p[0]; r += p[1];
  }
  s_p[0][lane] = c; s_p[1][lane] = r;
  __syncthreads();
  if (lane == 0) {
    int tot = 0;
    for (int b = 0; b < B; ++b) tot += max(counts[4 * b + 2], 1) + max(counts[4 * b + 3], 1);
    double sc = 0.0, sr = 0.0;
    for (int j = 0; j < 64; ++j) { sc += s_p[0][j]; sr += s_p[1][j]; }
    losses[l] = (float)(sc / (double)tot * (double)cfg.loss_weight_cls);
    losses[tg.nlev + l] = (float)(sr / (double)tot * (double)cfg.loss_weight_bbox);
    if (l == 0 && rng_state != nullptr) rng_state[1] += 1u;
  }
}

// measurement aid (hrf_debug_knob 44, tools/rpn_loss_cost.py): k > 0 = return after the first k launches (incomplete outputs)
static int g_rpnt_stop = 0;
#define RPNT_STEP(k) { if (hrf_check_launch() != HRF_OK) return HRF_ERR_LAUNCH; if (g_rpnt_stop == (k)) return HRF_OK; }

bool rpnt_cfg_ok(const hrf_rpn_train_cfg_t* c) {
  if (c == nullptr) return false;
  if (!(c->pos_iou_thr >= 0.f && c->pos_iou_thr <= 1.f) || !(c->neg_iou_thr >= 0.f && c->neg_iou_thr <= 1.f) ||
      !(c->min_pos_iou >= 0.f && c->min_pos_iou <= 1.f)) return false;                               // (NaN fails)
  if (c->num < 1 || c->num_pos < 0 || c->num_pos > c->num) return false;
  if (c->allowed_border > (1 << 24) || c->allowed_border < -(1 << 24)) return false;
  if (!(c->beta > 0.f && c->beta < 3.0e38f)) return false;
  if (!(fabsf(c->loss_weight_cls) < 3.0e38f) || !(fabsf(c->loss_weight_bbox) < 3.0e38f)) return false;
  return true;
}

// -> false: the pyramid / settings are outside the contract; otherwise the grid table
bool rpnt_check(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, int Gmax, RpntGrid& tg) {
  if (lv == nullptr || !rpnt_cfg_ok(cfg) || Gmax < 1 || Gmax > HRF_RPN_MAX_GT) return false;
  if (lv->num_levels < 1 || lv->num_levels > HRF_RPN_MAX_LEVELS || lv->A < 1 || lv->A > HRF_RPN_MAX_ANCHORS || lv->B < 1 || lv->B > 65535) return false;
  long N = 0, nblk = 0;
  for (int l = 0; l < HRF_RPN_MAX_LEVELS; ++l) {
    tg.n[l] = 0; tg.noff[l] = (int)N; tg.boff[l] = (int)nblk;
    if (l >= lv->num_levels) continue;
    if (lv->cls[l] == nullptr || lv->reg[l] == nullptr || lv->H[l] < 1 || lv->W[l] < 1 || lv->stride[l] < 1) return false;
    if (lv->ld_cls[l] < lv->A || lv->ld_reg[l] < 4 * lv->A) return false;
    const long nl = (long)lv->H[l] * lv->W[l] * lv->A;
    if (N + nl > 0x3fffffffL) return false;
    tg.n[l] = (int)nl;
    N += nl; nblk += (nl + RPNT_NT - 1) / RPNT_NT;
  }
  tg.nlev = lv->num_levels; tg.N = (int)N; tg.nblk = (int)nblk;
  return true;
}

long rpnt_bytes(const RpntGrid& tg, int B, int Gmax) {
  return rpn_align((long)B * tg.N * 4) + rpn_align((long)B * Gmax * RPNT_SLICES * 4) + rpn_align((long)B * 2 * 8) + rpn_align((long)B * tg.nblk * 2 * 8);
}

bool rpnt_grads_ok(const hrf_rpn_levels_t* lv, const hrf_rpn_grads_t* gr) {
  if (gr == nullptr) return false;
  for (int l = 0; l < lv->num_levels; ++l)
    if (gr->d_cls[l] == nullptr || gr->d_reg[l] == nullptr || gr->ld_cls[l] < lv->A || gr->ld_reg[l] < 4 * lv->A) return false;
  return true;
}

int rpnt_run(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, const float* img_shape, const float* pad_shape, const float* gt,
             const int* gt_count, int Gmax, const unsigned* keys, unsigned* rng_state, void* workspace, long workspace_bytes, int* assigned,
             float* max_iou, int* sampled, int* counts, const hrf_rpn_grads_t* grads, float* losses, bool loss, void* stream) {
  RpntGrid tg;
  if (!rpnt_check(lv, cfg, Gmax, tg)) return HRF_ERR_ARG;
  if (img_shape == nullptr || pad_shape == nullptr || gt == nullptr || gt_count == nullptr || (keys == nullptr && rng_state == nullptr)) return HRF_ERR_ARG;
  if (assigned == nullptr || max_iou == nullptr || sampled == nullptr || counts == nullptr) return HRF_ERR_ARG;
  if (workspace == nullptr || workspace_bytes < rpnt_bytes(tg, lv->B, Gmax)) return HRF_ERR_ARG;
  if (loss && (!rpnt_grads_ok(lv, grads) || losses == nullptr)) return HRF_ERR_ARG;
  const int B = lv->B;
  char* ws = static_cast<char*>(workspace);
  int* argmax = reinterpret_cast<int*>(ws);
  float* gt_max = reinterpret_cast<float*>(ws + rpn_align((long)B * tg.N * 4));     // [B][Gmax][RPNT_SLICES]
  rpn_u64* thr = reinterpret_cast<rpn_u64*>(reinterpret_cast<char*>(gt_max) + rpn_align((long)B * Gmax * RPNT_SLICES * 4));
  double* slots = reinterpret_cast<double*>(reinterpret_cast<char*>(thr) + rpn_align((long)B * 2 * 8));
  const dim3 grid(tg.nblk, B);
  HRF_LAUNCH(rpnt_iou_kernel, grid, dim3(RPNT_NT), 0, stream, *lv, tg, *cfg, img_shape, pad_shape, gt, gt_count, Gmax, max_iou, argmax);
  RPNT_STEP(1)
  HRF_LAUNCH(rpnt_gtmax_kernel, dim3(Gmax, B, RPNT_SLICES), dim3(RPNT_NT), 0, stream, *lv, tg, gt, gt_count, Gmax, (const int*)argmax, gt_max);
  RPNT_STEP(2)
  HRF_LAUNCH(rpnt_assign_kernel, grid, dim3(RPNT_NT), 0, stream, *lv, tg, *cfg, gt, gt_count, Gmax, (const float*)max_iou, (const int*)argmax,
             (const float*)gt_max, assigned);
  RPNT_STEP(3)
  HRF_LAUNCH(rpnt_select_kernel, dim3(2, B), dim3(RPNT_SEL_NT), 0, stream, tg.N, *cfg, (const int*)assigned, keys, (const unsigned*)rng_state, thr,
             counts);
  RPNT_STEP(4)
  if (!loss) {
    hrf_rpn_grads_t none = {};
    HRF_LAUNCH(rpnt_loss_kernel<false>, grid, dim3(RPNT_NT), 0, stream, *lv, tg, *cfg, none, gt, Gmax, keys, (const unsigned*)rng_state,
               (const int*)assigned, (const rpn_u64*)thr, (const int*)counts, sampled, slots);
    return hrf_check_launch();
  }
  HRF_LAUNCH(rpnt_loss_kernel<true>, grid, dim3(RPNT_NT), 0, stream, *lv, tg, *cfg, *grads, gt, Gmax, keys, (const unsigned*)rng_state,
             (const int*)assigned, (const rpn_u64*)thr, (const int*)counts, sampled, slots);
  RPNT_STEP(5)
  HRF_LAUNCH(rpnt_finalize_kernel, dim3(tg.nlev), dim3(64), 0, stream, tg, *cfg, B, (const double*)slots, (const int*)counts, losses,
             keys == nullptr ? rng_state : (unsigned*)nullptr);
  return hrf_check_launch();
}

}  // namespace

// (reached through hrf_debug_knob only: not exported)
extern "C" __attribute__((visibility("hidden"))) int hrf_rpnt_knob(int key, int value) {
  if (key != 0 || value < 0 || value > 6) return HRF_ERR_ARG;
  g_rpnt_stop = value;
  return HRF_OK;
}

extern "C" int hrf_rpn_train_supported(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, int Gmax) {
  RpntGrid tg;
  return rpnt_check(lv, cfg, Gmax, tg) ? 1 : 0;
}

extern "C" long hrf_rpn_train_workspace_bytes(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, int Gmax) {
  RpntGrid tg;
  return rpnt_check(lv, cfg, Gmax, tg) ? rpnt_bytes(tg, lv->B, Gmax) : 0;
}

extern "C" int hrf_rpn_assign(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, const float* img_shape, const float* pad_shape,
                              const float* gt, const int* gt_count, int Gmax, const unsigned* keys, unsigned* rng_state, void* workspace,
                              long workspace_bytes, int* assigned, float* max_iou, int* sampled, int* counts, void* stream) {
  return rpnt_run(lv, cfg, img_shape, pad_shape, gt, gt_count, Gmax, keys, rng_state, workspace, workspace_bytes, assigned, max_iou, sampled,
                  counts, nullptr, nullptr, false, stream);
}

extern "C" int hrf_rpn_loss(const hrf_rpn_levels_t* lv, const hrf_rpn_train_cfg_t* cfg, const float* img_shape, const float* pad_shape,
                            const float* gt, const int* gt_count, int Gmax, const unsigned* keys, unsigned* rng_state, void* workspace,
                            long workspace_bytes, int* assigned, float* max_iou, int* sampled, int* counts, const hrf_rpn_grads_t* grads,
                            float* losses, void* stream) {
  return rpnt_run(lv, cfg, img_shape, pad_shape, gt, gt_count, Gmax, keys, rng_state, workspace, workspace_bytes, assigned, max_iou, sampled,
                  counts, grads, losses, true, stream);
}
