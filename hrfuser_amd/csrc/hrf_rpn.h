// RPN proposal generation: per-level top-k + anchor decode, per-level greedy NMS, cross-level merge (gfx950, NHWC fp32).
//
//   mmdet/models/dense_heads/base_dense_head.py:32-108 (get_bboxes: per image, the level lists, the anchors of grid_priors),
//   mmdet/models/dense_heads/rpn_head.py:103-235 (_get_bboxes_single: sigmoid, per-level sort + nms_pre; _bbox_post_process:
//   decode, min_bbox_size filter, batched_nms with the level as the class id, [:max_per_img]),
//   mmdet/core/anchor/anchor_generator.py:151-194 (base anchors - computed by the CALLER, handed over in the argument struct)
//   and :241-281 (anchor (y, x, a) = base[a] + (x * stride, y * stride, x * stride, y * stride), flat index (y * W + x) * A + a),
//   mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:164-260 (delta2bbox, means 0, stds 1, wh_ratio_clip 16 / 1000, clip_border),
//   mmcv 1.3.17 ops/nms.py batched_nms / nms (csrc/pytorch/cuda/nms_cuda_kernel.cuh: offset 0, iou > threshold suppresses).
//
// Part of the translation unit pointwise.hip (included at its end).  Four launches, fixed-shape outputs, no host read of any
// input, no allocation, no synchronisation, no float atomics (the same bits in deterministic mode).  Every loop is bounded by a
// map size or by HRF_RPN_MAX_PRE, never by data; logits and deltas may be NaN / Inf.
//
// RANKING.  The reference sorts sigmoid(logit) descending with torch.sort, whose order among equal scores is unspecified.  Here the
// rank is taken on the RAW logit: sigmoid is monotone, so on inputs whose selected logits have distinct fp32 sigmoids any
// reference output is reproduced; equal logits (and logits merged by the fp32 sigmoid) go to the lower flat index, -0 == +0,
// a NaN logit ranks below everything and its candidate is marked invalid (the reference would emit a NaN score).
// The order is carried by ONE 64-bit integer per anchor, (order-preserving image of the logit) << 32 | (2^32 - 1 - flat index):
// all distinct, larger = earlier.
//
//   1  rpn_select_decode_kernel   one workgroup of 1024 per (image, level).  N = H * W * A > 2048: radix select of the k-th
//      largest 64-bit code, 8 bits per pass from the top (LDS histogram of the codes that match the prefix so far; the passes
//      stop as soon as the bin that holds the k-th code is taken entirely - 4 passes on tie-free logits; index bytes that
//      cannot differ are never visited), then the k winners are compacted into LDS in any order.  N <= 2048: all codes are
//      loaded.  A bitonic sort of <= 2048 codes in LDS orders them; thread r decodes rank r: anchor from base[a] + shifts,
//      delta2bbox in the written fp32 order (one expf per side is the only operation that is not bit-defined), clip to the
//      image of img_shape[b], valid = w > min_bbox_size && h > min_bbox_size (a NaN box fails both).
//   2  rpn_nms_tile_kernel        one 64-thread block per 64 x 64 tile (row block <= column block) of a segment's suppression
//      matrix: bit (i, j), j > i, = iou(i, j) > thr with  area = (x2-x1)*(y2-y1), iw = max(min(x2i,x2j) - max(x1i,x1j), 0),
//      inter = iw*ih, iou = inter / (area_i + area_j - inter)  in fp32, in this order (-ffp-contract=off: bit-defined).
//   3  rpn_nms_reduce_kernel      one wave per segment; lane w owns the "removed" word of column block w (initially: the invalid
//      candidates and the bits past n).  Per 64-row block: the diagonal tile goes through LDS and every lane resolves it
//      (64 steps on registers, broadcast LDS reads whose addresses do not depend on the outcome), then the rows of the block's
//      kept boxes are ORed into the lanes' words - ALL their loads issued before the first OR (their addresses are known from the
//      kept word: one memory latency per block, not one per box), the next diagonal tile already in flight.  Writes the keep words and their prefix counts.
//   4  rpn_merge_kernel           one thread per candidate: its rank in the image = kept candidates before it in its own
//      segment (prefix count + popcount) + for every other segment the kept candidates before the insertion point of its logit
//      (binary search in that segment's descending list; ties: lower segment, then lower row).  rank < max_per_img: the row
//      of `dets` (box, sigmoid(logit)) and of `rois` (image, box) is written; rows past the count are zeroed / (b, 0, 0, 0, 0).
//
// Levels are independent in the NMS: that is what batched_nms does with the level as the class id.  mmcv's way of getting there
// below 10 000 boxes - adding level * (max coordinate + 1) to the boxes of a joint NMS - only adds fp32 rounding to the same
// decisions and is NOT reproduced.
#pragma once

namespace {

constexpr int RPN_NT = 1024;                   // select + decode workgroup
constexpr int RPN_UNROLL = 8;                  // logits a thread of it loads before it uses the first
constexpr int RPN_WORDS = HRF_RPN_MAX_PRE / 64;        // 64-candidate blocks of a segment
constexpr int RPN_PREF = RPN_WORDS + 1;        // prefix counts per segment (the last one: the segment's total)
typedef unsigned long long rpn_u64;

#define RPN_SEL(arr, l) ((l) == 0 ? (arr)[0] : (l) == 1 ? (arr)[1] : (l) == 2 ? (arr)[2] : (l) == 3 ? (arr)[3] : (arr)[4])

// SEG_SEL: entry l of a segment table's member.  The NMS kernels are templates over the table SG: RpnSegs (below: arrays of
// HRF_RPN_MAX_LEVELS entries, picked with selects so that the by-value kernel argument stays in registers) or a `uniform` table
// whose members are indexable objects (hrf_bbox.h: up to HRF_BBOX_MAX_CLASSES segments of one length).  SG::uniform is a
// constant: the other arm folds away.
#define SEG_SEL(SG, sg, arr, l) (SG::uniform ? (sg).arr[l] : RPN_SEL((sg).arr, l))

// the segments of ONE image (every image has the same): rows of `cand`, words of the suppression matrices
struct RpnSegs {
  static constexpr bool uniform = false;
  int nseg, ktot;
  int n[HRF_RPN_MAX_LEVELS];                   // candidates
  int off[HRF_RPN_MAX_LEVELS];                 // first row within the image
  long moff[HRF_RPN_MAX_LEVELS];               // first matrix word within the image
  long mtot;                                   // matrix words of one image
};

// order-preserving integer image of a logit: a > b  <=>  key(a) > key(b); -0 == +0; NaN -> 0, below every number
__device__ __forceinline__ unsigned rpn_key(float f) {
  if (f != f) return 0u;
  if (f == 0.f) f = 0.f;
  unsigned u;
  __builtin_memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ rpn_u64 rpn_code(const float* cls, int ldc, int A, int i) {
  const int pix = i / A, a = i - pix * A;
  return ((rpn_u64)rpn_key(cls[(long)pix * ldc + a]) << 32) | (rpn_u64)(0xffffffffu - (unsigned)i);
}

__device__ __forceinline__ float rpn_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // (keeps a NaN, as torch.clamp)

__device__ __forceinline__ int rpn_popc(rpn_u64 v) { return __builtin_popcountll(v); }

__global__ __launch_bounds__(RPN_NT) void rpn_select_decode_kernel(hrf_rpn_levels_t lv, RpnSegs sg, float min_size, const float* img_shape,
                                                                   float* cand, int* valid, int* idx_out) {
  __shared__ rpn_u64 s_c[HRF_RPN_MAX_PRE];
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_ctl[4];                // digit, still wanted, done, compaction cursor
  const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int H = RPN_SEL(lv.H, l), W = RPN_SEL(lv.W, l), A = lv.A, ldc = RPN_SEL(lv.ld_cls, l), ldr = RPN_SEL(lv.ld_reg, l);
  const int N = H * W * A, k = RPN_SEL(sg.n, l);
  const float* cls = RPN_SEL(lv.cls, l) + (long)b * H * W * ldc;
  const float* reg = RPN_SEL(lv.reg, l) + (long)b * H * W * ldr;
  int nsort = 2;
  if (N <= HRF_RPN_MAX_PRE) {
    while (nsort < N) nsort <<= 1;
    for (int i = tid; i < nsort; i += RPN_NT) s_c[i] = i < N ? rpn_code(cls, ldc, A, i) : 0ull;      // (0 sorts behind every code)
  } else {
    while (nsort < k) nsort <<= 1;
    // radix select: P / M = the bytes of the k-th largest code found so far and their mask
    const int nbytes = N <= (1 << 8) ? 1 : N <= (1 << 16) ? 2 : N <= (1 << 24) ? 3 : 4;              // index bytes that can differ
    rpn_u64 P = 0ull, M = 0ull;
    unsigned want = (unsigned)k;
    for (int pass = 0; pass < 4 + nbytes; ++pass) {
      const int byte = pass < 4 ? 7 - pass : nbytes - 1 - (pass - 4);
      const int sh = 8 * byte;
      if (tid < 256) s_hist[tid] = 0u;
      __syncthreads();
      for (int i0 = tid; i0 < N; i0 += RPN_NT * RPN_UNROLL) {           // RPN_UNROLL independent loads in flight per thread
        rpn_u64 c[RPN_UNROLL];
#pragma unroll
        for (int u = 0; u < RPN_UNROLL; ++u) c[u] = rpn_code(cls, ldc, A, min(i0 + u * RPN_NT, N - 1));
#pragma unroll
        for (int u = 0; u < RPN_UNROLL; ++u)
          if (i0 + u * RPN_NT < N && ((c[u] ^ P) & M) == 0ull) atomicAdd(&s_hist[(unsigned)(c[u] >> sh) & 255u], 1u);
      }
      __syncthreads();
      if (tid < 256) {                         // bin `tid` holds the wanted code when  above < want <= above + its count  (one bin does)
        unsigned above = 0u;
        for (int d = 255; d > 0; --d) above += d > tid ? s_hist[d] : 0u;      // (independent broadcast reads, fixed trip count)
        const unsigned mine = s_hist[tid];
        if (above < want && want <= above + mine) { s_ctl[0] = (unsigned)tid; s_ctl[1] = want - above; s_ctl[2] = (mine == want - above) ? 1u : 0u; }
      }
      __syncthreads();
      P |= (rpn_u64)s_ctl[0] << sh; M |= 0xffull << sh;
      want = s_ctl[1];
      if (pass == 3 && nbytes < 4) {           // the index bytes above `nbytes` are 0xff in every code
        const rpn_u64 hi = (0xffffffffull >> (8 * nbytes)) << (8 * nbytes);
        P |= hi; M |= hi;
      }
      if (s_ctl[2]) break;                     // (block-uniform) every code under this prefix is taken
    }
    if (tid == 0) s_ctl[3] = 0u;
    __syncthreads();
    for (int i0 = tid; i0 < N; i0 += RPN_NT * RPN_UNROLL) {             // exactly k codes pass
      rpn_u64 c[RPN_UNROLL];
#pragma unroll
      for (int u = 0; u < RPN_UNROLL; ++u) c[u] = rpn_code(cls, ldc, A, min(i0 + u * RPN_NT, N - 1));
#pragma unroll
      for (int u = 0; u < RPN_UNROLL; ++u)
        if (i0 + u * RPN_NT < N && (c[u] & M) >= P) {
          const unsigned pos = atomicAdd(&s_ctl[3], 1u);
          if (pos < (unsigned)HRF_RPN_MAX_PRE) s_c[pos] = c[u];
        }
    }
    for (int i = k + tid; i < nsort; i += RPN_NT) s_c[i] = 0ull;
  }
  __syncthreads();
  for (int size = 2; size <= nsort; size <<= 1) {                      // bitonic sort, descending
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (nsort >> 1); t += RPN_NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i + j;        // (j is a power of two)
        const rpn_u64 a = s_c[i], c = s_c[p];
        const bool down = (i & size) == 0;
        if ((a < c) == down && a != c) { s_c[i] = c; s_c[p] = a; }
      }
      __syncthreads();
    }
  }
  const float img_h = img_shape[2 * b], img_w = img_shape[2 * b + 1];
  const float stride = (float)RPN_SEL(lv.stride, l);
  const float max_ratio = 4.135166556742356f;                          // |log(16 / 1000)|
  for (int r = tid; r < k; r += RPN_NT) {
    const unsigned idx = 0xffffffffu - (unsigned)s_c[r];               // < N: the k <= N real codes sort before the padding
    const int pix = (int)idx / A, a = (int)idx - pix * A, y = pix / W, x = pix - y * W;
    const float logit = cls[(long)pix * ldc + a];
    const float* d = reg + (long)pix * ldr + 4 * a;
    const float* ba = lv.base_anchors + (l * HRF_RPN_MAX_ANCHORS + a) * 4;
    const float sx = (float)x * stride, sy = (float)y * stride;
    const float ax1 = ba[0] + sx, ay1 = ba[1] + sy, ax2 = ba[2] + sx, ay2 = ba[3] + sy;
    const float px = (ax1 + ax2) * 0.5f, py = (ay1 + ay2) * 0.5f, pw = ax2 - ax1, ph = ay2 - ay1;
    const float dw = rpn_clamp(d[2], -max_ratio, max_ratio), dh = rpn_clamp(d[3], -max_ratio, max_ratio);
    const float gx = px + pw * d[0], gy = py + ph * d[1];
    const float gw = pw * expf(dw), gh = ph * expf(dh);
    const float hw = gw * 0.5f, hh = gh * 0.5f;
    const float x1 = rpn_clamp(gx - hw, 0.f, img_w), y1 = rpn_clamp(gy - hh, 0.f, img_h);
    const float x2 = rpn_clamp(gx + hw, 0.f, img_w), y2 = rpn_clamp(gy + hh, 0.f, img_h);
    const long row = (long)b * sg.ktot + RPN_SEL(sg.off, l) + r;
    float* o = cand + 5 * row;
    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; o[4] = logit;
    valid[row] = ((x2 - x1) > min_size && (y2 - y1) > min_size && logit == logit) ? 1 : 0;
    if (idx_out != nullptr) idx_out[row] = (int)idx;
  }
}

template <class SG>
__global__ __launch_bounds__(64) void rpn_nms_tile_kernel(const float* cand, SG sg, float thr, rpn_u64* mask) {
  __shared__ float s_box[64][5];
  const int b = blockIdx.z / sg.nseg, s = blockIdx.z - b * sg.nseg, t = threadIdx.x;
  const int n = SEG_SEL(SG, sg, n, s), nb = (n + 63) >> 6;
  const int ib = blockIdx.y, jb = blockIdx.x;
  if (ib > jb || jb >= nb) return;             // (block-uniform)
  const float* base = cand + ((long)b * sg.ktot + SEG_SEL(SG, sg, off, s)) * 5;
  const int j0 = jb * 64;
  {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (j0 + t < n)
      for (int c = 0; c < 4; ++c) v[c] = base[(long)(j0 + t) * 5 + c];
    for (int c = 0; c < 4; ++c) s_box[t][c] = v[c];
    s_box[t][4] = (v[2] - v[0]) * (v[3] - v[1]);
  }
  __syncthreads();
  const int i = ib * 64 + t;
  if (i >= n) return;
  const float x1 = base[(long)i * 5], y1 = base[(long)i * 5 + 1], x2 = base[(long)i * 5 + 2], y2 = base[(long)i * 5 + 3];
  const float area = (x2 - x1) * (y2 - y1);
  rpn_u64 bits = 0ull;
  const int jn = min(64, n - j0);
  for (int jj = 0; jj < jn; ++jj) {
    if (j0 + jj <= i) continue;
    const float iw = fmaxf(fminf(x2, s_box[jj][2]) - fmaxf(x1, s_box[jj][0]), 0.f);
    const float ih = fmaxf(fminf(y2, s_box[jj][3]) - fmaxf(y1, s_box[jj][1]), 0.f);
    const float inter = iw * ih;
    const float iou = inter / (area + s_box[jj][4] - inter);
    if (iou > thr) bits |= 1ull << jj;
  }
  mask[(long)b * sg.mtot + SEG_SEL(SG, sg, moff, s) + (long)i * nb + jb] = bits;
}

template <class SG>
__global__ __launch_bounds__(64) void rpn_nms_reduce_kernel(const int* valid, SG sg, const rpn_u64* mask, rpn_u64* keepw, int* pref) {
  __shared__ rpn_u64 s_d[64];
  __shared__ int s_pc[64];
  const int b = blockIdx.x / sg.nseg, s = blockIdx.x - b * sg.nseg, lane = threadIdx.x;
  const int n = SEG_SEL(SG, sg, n, s), nb = (n + 63) >> 6;
  const long row0 = (long)b * sg.ktot + SEG_SEL(SG, sg, off, s);
  const rpn_u64* M = mask + (long)b * sg.mtot + SEG_SEL(SG, sg, moff, s);
  rpn_u64 removed = ~0ull;
  if (lane < nb) {
    removed = 0ull;
    for (int bit = 0; bit < 64; ++bit) {
      const int i = lane * 64 + bit;
      if (i >= n || (valid != nullptr && valid[row0 + i] == 0)) removed |= 1ull << bit;
    }
  }
  rpn_u64 diag = (nb > 0 && lane < n) ? M[(long)lane * nb] : 0ull;
  for (int ib = 0; ib < nb; ++ib) {
    rpn_u64 cur = __shfl(removed, ib);
    s_d[lane] = diag;
    const int inext = (ib + 1) * 64 + lane;                            // the next block's diagonal tile: in flight during this block
    diag = (ib + 1 < nb && inext < n) ? M[(long)inext * nb + ib + 1] : 0ull;
    HRF_WAVE_SYNC();
    for (int t = 0; t < 64; ++t)
      if (!((cur >> t) & 1ull)) cur |= s_d[t];
    HRF_WAVE_SYNC();
    if (lane == ib) removed = cur;
    const rpn_u64 kept = ~cur;                 // (wave-uniform) rows >= n and invalid rows are never kept
    if (kept == 0ull || ib + 1 >= nb) continue;
    const bool mine = lane > ib && lane < nb;
    const rpn_u64* Mr = M + (long)ib * 64 * nb + lane;
    rpn_u64 v[64];
#pragma unroll
    for (int t = 0; t < 64; ++t) v[t] = (mine && ((kept >> t) & 1ull)) ? Mr[(long)t * nb] : 0ull;
#pragma unroll
    for (int t = 0; t < 64; ++t) removed |= v[t];
  }
  const rpn_u64 keep = ~removed;               // lanes >= nb: 0
  s_pc[lane] = rpn_popc(keep);
  HRF_WAVE_SYNC();
  if (lane < RPN_WORDS) keepw[(long)blockIdx.x * RPN_WORDS + lane] = keep;
  if (lane < RPN_PREF) {
    int p = 0;
    for (int w = 0; w < lane; ++w) p += s_pc[w];
    pref[(long)blockIdx.x * RPN_PREF + lane] = p;
  }
}

// kept candidates among the first p rows of a segment
__device__ __forceinline__ int rpn_kept_before(const rpn_u64* keepw, const int* pref, int p) {
  const int w = p >> 6, bit = p & 63;
  return pref[w] + (bit ? rpn_popc(keepw[w] & ((1ull << bit) - 1ull)) : 0);
}

// rois / labels are nullable; labels[b][rank] = the segment of the row, -1 past the count
template <class SG>
__global__ __launch_bounds__(256) void rpn_merge_kernel(const float* cand, SG sg, const rpn_u64* keepw, const int* pref, int maxp,
                                                        int sigmoid, float* dets, int* count, float* rois, int* labels) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  const rpn_u64* kw = keepw + (long)b * sg.nseg * RPN_WORDS;
  const int* pf = pref + (long)b * sg.nseg * RPN_PREF;
  int total = 0;
  for (int s = 0; s < sg.nseg; ++s) total += pf[s * RPN_PREF + RPN_WORDS];
  const int cnt = min(total, maxp);
  if (j == 0) count[b] = cnt;
  if (j < maxp && j >= cnt) {
    float* d = dets + ((long)b * maxp + j) * 5;
    for (int c = 0; c < 5; ++c) d[c] = 0.f;
    if (rois != nullptr) {
      float* r = rois + ((long)b * maxp + j) * 5;
      for (int c = 0; c < 5; ++c) r[c] = c == 0 ? (float)b : 0.f;
    }
    if (labels != nullptr) labels[(long)b * maxp + j] = -1;
  }
  if (j >= sg.ktot) return;
  int s = 0;
  while (s + 1 < sg.nseg && j >= SEG_SEL(SG, sg, off, s) + SEG_SEL(SG, sg, n, s)) ++s;
  const int r = j - SEG_SEL(SG, sg, off, s);
  if (r >= SEG_SEL(SG, sg, n, s)) return;
  if (!((kw[s * RPN_WORDS + (r >> 6)] >> (r & 63)) & 1ull)) return;
  const float* img = cand + (long)b * sg.ktot * 5;
  const float* me = img + (long)j * 5;
  const unsigned key = rpn_key(me[4]);
  int rank = rpn_kept_before(kw + s * RPN_WORDS, pf + s * RPN_PREF, r);
  for (int s2 = 0; s2 < sg.nseg; ++s2) {
    if (s2 == s) continue;
    const float* other = img + (long)SEG_SEL(SG, sg, off, s2) * 5 + 4;
    int lo = 0, hi = SEG_SEL(SG, sg, n, s2);
    while (lo < hi) {                          // rows of s2 that come before (key, s, r): <= 12 steps
      const int mid = (lo + hi) >> 1;
      const unsigned k2 = rpn_key(other[(long)mid * 5]);
      if (s2 < s ? k2 >= key : k2 > key) lo = mid + 1;
      else hi = mid;
    }
    rank += rpn_kept_before(kw + s2 * RPN_WORDS, pf + s2 * RPN_PREF, lo);
  }
  if (rank >= maxp) return;
  float* d = dets + ((long)b * maxp + rank) * 5;
  d[0] = me[0]; d[1] = me[1]; d[2] = me[2]; d[3] = me[3];
  d[4] = sigmoid ? 1.f / (1.f + expf(-me[4])) : me[4];
  if (rois != nullptr) {
    float* ro = rois + ((long)b * maxp + rank) * 5;
    ro[0] = (float)b; ro[1] = me[0]; ro[2] = me[1]; ro[3] = me[2]; ro[4] = me[3];
  }
  if (labels != nullptr) labels[(long)b * maxp + rank] = s;
}

// the segment table of one image -> false: a length outside [0, HRF_RPN_MAX_PRE] or a count outside [1, HRF_RPN_MAX_LEVELS]
bool rpn_segs(const int* seg_len, int nseg, RpnSegs& sg) {
  if (seg_len == nullptr || nseg < 1 || nseg > HRF_RPN_MAX_LEVELS) return false;
  sg.nseg = nseg; sg.ktot = 0; sg.mtot = 0;
  for (int s = 0; s < HRF_RPN_MAX_LEVELS; ++s) {
    const int n = s < nseg ? seg_len[s] : 0;
    if (n < 0 || n > HRF_RPN_MAX_PRE) return false;
    sg.n[s] = n; sg.off[s] = sg.ktot; sg.moff[s] = sg.mtot;
    sg.ktot += n;
    sg.mtot += (long)n * ((n + 63) / 64);
  }
  return true;
}

inline long rpn_align(long v) { return (v + 255) / 256 * 256; }

// bytes of the NMS part of a workspace: matrices, keep words, prefix counts
template <class SG>
long rpn_nms_bytes(const SG& sg, int B) {
  return rpn_align((long)B * sg.mtot * 8) + rpn_align((long)B * sg.nseg * RPN_WORDS * 8) + rpn_align((long)B * sg.nseg * RPN_PREF * 4);
}

bool rpn_cfg_ok(const hrf_rpn_cfg_t* cfg) {
  if (cfg == nullptr) return false;
  if (cfg->nms_pre < 1 || cfg->nms_pre > HRF_RPN_MAX_PRE || cfg->max_per_img < 1) return false;
  if (!(cfg->iou_thr > 0.f && cfg->iou_thr <= 1.f)) return false;     // (NaN fails)
  if (!(cfg->min_bbox_size >= 0.f && cfg->min_bbox_size < 3.0e38f)) return false;
  return true;
}

// -> false: the pyramid / settings are outside the contract; otherwise the segment table (k_l = min(nms_pre, H_l * W_l * A))
bool rpn_check(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg, RpnSegs& sg) {
  if (lv == nullptr || !rpn_cfg_ok(cfg)) return false;
  if (lv->num_levels < 1 || lv->num_levels > HRF_RPN_MAX_LEVELS || lv->A < 1 || lv->A > HRF_RPN_MAX_ANCHORS || lv->B < 1 || lv->B > 65535) return false;
  int len[HRF_RPN_MAX_LEVELS];
  for (int l = 0; l < lv->num_levels; ++l) {
    if (lv->cls[l] == nullptr || lv->reg[l] == nullptr || lv->H[l] < 1 || lv->W[l] < 1 || lv->stride[l] < 1) return false;
    if (lv->ld_cls[l] < lv->A || lv->ld_reg[l] < 4 * lv->A) return false;
    if ((long)lv->H[l] * lv->W[l] * lv->A > 0x7fffffffL) return false;
    const long N = (long)lv->H[l] * lv->W[l] * lv->A;
    len[l] = N < (long)cfg->nms_pre ? (int)N : cfg->nms_pre;
  }
  return rpn_segs(len, lv->num_levels, sg);
}

template <class SG>
int rpn_launch_nms(const float* cand, const int* valid, const SG& sg, int B, int maxp, float thr, int sigmoid, char* ws,
                   float* dets, int* count, float* rois, int* labels, void* stream) {
  rpn_u64* mask = reinterpret_cast<rpn_u64*>(ws);
  rpn_u64* keepw = reinterpret_cast<rpn_u64*>(ws + rpn_align((long)B * sg.mtot * 8));
  int* pref = reinterpret_cast<int*>(reinterpret_cast<char*>(keepw) + rpn_align((long)B * sg.nseg * RPN_WORDS * 8));
  int nbmax = 0;
  for (int s = 0; s < sg.nseg; ++s) nbmax = max(nbmax, (sg.n[s] + 63) / 64);
  if (nbmax > 0) {
    HRF_LAUNCH((rpn_nms_tile_kernel<SG>), dim3(nbmax, nbmax, B * sg.nseg), dim3(64), 0, stream, cand, sg, thr, mask);
    if (hrf_check_launch() != HRF_OK) return HRF_ERR_LAUNCH;
  }
  HRF_LAUNCH((rpn_nms_reduce_kernel<SG>), dim3(B * sg.nseg), dim3(64), 0, stream, valid, sg, (const rpn_u64*)mask, keepw, pref);
  if (hrf_check_launch() != HRF_OK) return HRF_ERR_LAUNCH;
  HRF_LAUNCH((rpn_merge_kernel<SG>), dim3(hrf_cdiv(max(sg.ktot, maxp), 256), B), dim3(256), 0, stream, cand, sg, (const rpn_u64*)keepw,
             (const int*)pref, maxp, sigmoid, dets, count, rois, labels);
  return hrf_check_launch();
}

}  // namespace

extern "C" int hrf_rpn_supported(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg) {
  RpnSegs sg;
  return rpn_check(lv, cfg, sg) ? 1 : 0;
}

extern "C" long hrf_nms_workspace_bytes(const int* seg_len, int nseg, int B) {
  RpnSegs sg;
  if (B < 1 || B > 65535 / HRF_RPN_MAX_LEVELS || !rpn_segs(seg_len, nseg, sg)) return 0;
  return rpn_nms_bytes(sg, B);
}

extern "C" long hrf_rpn_workspace_bytes(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg) {
  RpnSegs sg;
  if (!rpn_check(lv, cfg, sg) || lv->B > 65535 / HRF_RPN_MAX_LEVELS) return 0;
  return rpn_align((long)lv->B * sg.ktot * 20) + rpn_align((long)lv->B * sg.ktot * 4) + rpn_nms_bytes(sg, lv->B);
}

extern "C" int hrf_rpn_select_decode(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg, const float* img_shape, float* cand, int* valid,
                                     int* idx, void* stream) {
  RpnSegs sg;
  if (!rpn_check(lv, cfg, sg) || img_shape == nullptr || cand == nullptr || valid == nullptr) return HRF_ERR_ARG;
  HRF_LAUNCH(rpn_select_decode_kernel, dim3(lv->num_levels, lv->B), dim3(RPN_NT), 0, stream, *lv, sg, cfg->min_bbox_size, img_shape, cand,
             valid, idx);
  return hrf_check_launch();
}

extern "C" int hrf_nms_segments(const float* cand, const int* valid, const int* seg_len, int nseg, int B, int max_per_img, float iou_thr,
                                int apply_sigmoid, void* workspace, long workspace_bytes, float* dets, int* count, float* rois, void* stream) {
  RpnSegs sg;
  if (B < 1 || B > 65535 / HRF_RPN_MAX_LEVELS || !rpn_segs(seg_len, nseg, sg)) return HRF_ERR_ARG;
  if (max_per_img < 1 || !(iou_thr > 0.f && iou_thr <= 1.f)) return HRF_ERR_ARG;
  if (workspace == nullptr || workspace_bytes < rpn_nms_bytes(sg, B) || dets == nullptr || count == nullptr || rois == nullptr) return HRF_ERR_ARG;
  if (sg.ktot > 0 && cand == nullptr) return HRF_ERR_ARG;
  return rpn_launch_nms(cand, valid, sg, B, max_per_img, iou_thr, apply_sigmoid ? 1 : 0, static_cast<char*>(workspace), dets, count, rois, nullptr, stream);
}

extern "C" int hrf_rpn_proposals(const hrf_rpn_levels_t* lv, const hrf_rpn_cfg_t* cfg, const float* img_shape, void* workspace,
                                 long workspace_bytes, float* dets, int* count, float* rois, void* stream) {
  RpnSegs sg;
  if (!rpn_check(lv, cfg, sg) || lv->B > 65535 / HRF_RPN_MAX_LEVELS || img_shape == nullptr) return HRF_ERR_ARG;
  if (workspace == nullptr || workspace_bytes < hrf_rpn_workspace_bytes(lv, cfg) || dets == nullptr || count == nullptr || rois == nullptr) return HRF_ERR_ARG;
  char* ws = static_cast<char*>(workspace);
  float* cand = reinterpret_cast<float*>(ws);
  int* valid = reinterpret_cast<int*>(ws + rpn_align((long)lv->B * sg.ktot * 20));
  char* nms = reinterpret_cast<char*>(valid) + rpn_align((long)lv->B * sg.ktot * 4);
  HRF_LAUNCH(rpn_select_decode_kernel, dim3(lv->num_levels, lv->B), dim3(RPN_NT), 0, stream, *lv, sg, cfg->min_bbox_size, img_shape, cand,
             valid, (int*)nullptr);
  if (hrf_check_launch() != HRF_OK) return HRF_ERR_LAUNCH;
  return rpn_launch_nms(cand, valid, sg, lv->B, cfg->max_per_img, cfg->iou_thr, 1, nms, dets, count, rois, nullptr, stream);
}
