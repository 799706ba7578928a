// Multi-level RoIAlign (SingleRoIExtractor) forward and backward, one launch each for all pyramid levels (gfx950, NHWC fp32).
//
//   mmdet/models/roi_heads/roi_extractors/single_level_roi_extractor.py:36-55 (map_roi_levels) and mmcv 1.3.17 RoIAlign with
//   aligned=True, pool_mode='avg', sampling_ratio=0, output_size 7 (csrc/pytorch/cuda/roi_align_cuda_kernel.cuh).
//
// Part of the translation unit pointwise.hip (included at its end).  ONE workgroup of four waves per box; the kernel derives the
// box's level itself (no host read of `rois`, no sort, no allocation).
//
// The operator is separable: the bilinear weights and the "sample outside [-1, n]" zeroing both factor per axis, so for one box
//
//   out[c][ph][pw] = (1 / count) * sum_y sum_x Ay[ph][y] * Ax[pw][x] * F[y][x][c]
//
// with Ay (7 x rows of the footprint) a function of (y1', rh, H) only and Ax of (x1', rw, W) only.  Threads 0..13 build the two
// weight tables in LDS (one thread per axis and bin, positions in fp64 - the integer decisions then are those of an fp64
// evaluation of the reference's formula), as per-bin ranges [lo, hi) of non-zero weights; the waves then walk footprint pixels:
//   forward   wave w takes bins w, w + 4, ...: lanes run along channels (float4 per lane: one pixel of a 256-channel map is ONE
//             1 KB wave load), four loads of a row in flight, the bin accumulates in registers; out_layout 1 stores the bin's row directly, out_layout 0
//             stages the 49 x C tile in LDS (pitch C + 1) and writes the box's [C][49] block contiguously;
//   backward  dout of the box is staged in LDS (pitch C + 4, pre-scaled by 1 / count); wave w takes footprint pixels w, w + 4,
//             ...: lane l owns channels l, l + 64, ...: the <= 2 x 2 bins that reach the pixel are summed on chip and every wave
//             instruction adds 256 contiguous bytes with global_atomic_add_f32.
//
// TRIP COUNTS ARE BOUNDED BY THE MAP, NEVER BY THE BOX (the coordinates come from device memory, unvalidated):
//   - a box with a coordinate that is not finite or with |coord * spatial_scale| > HRF_ROI_COORD_MAX, or a batch index outside
//     [0, B), takes the early exit BEFORE any float -> int conversion: forward row of zeros, backward nothing;
//   - the samples of one axis are evenly spaced, by more than 0.5 pixel whenever a bin has more than one, and a sample outside
//     [-1, n] contributes nothing: each bin's sample loop is clipped (in fp64, clamped to [0, grid] before the conversion) to
//     the samples that can fall inside, widened by one / two against rounding, the per-sample test is kept.  Per axis at most
//     2 n + HRF_ROI_AXIS_SLACK iterations whatever the box is; `count` still uses the full grid;
//   - the pixel loops run over the [lo, hi) ranges of the tables, which are ranges of map indices.
#pragma once

namespace {

constexpr int ROI_P = 7, ROI_NB = ROI_P * ROI_P, ROI_NT = 256;
constexpr int ROI_ALLOC_SLACK = 40;            // floats a weight table holds beyond the n of its axis (7 generous ranges overlap by <= 5)
constexpr int ROI_SMEM_MAX = 65536 - 512;      // dynamic LDS a launch may ask for (no attribute needed below 64 KB)

#ifdef HRF_EMUL
long g_roi_iters[2];                           // [0] sample-loop iterations of the table builds, [1] footprint pixels visited
#define ROI_COUNT(i, n) __atomic_fetch_add(&g_roi_iters[i], (long)(n), __ATOMIC_RELAXED)
#else
#define ROI_COUNT(i, n)
#endif

#define ROI_SEL(arr, l) ((l) == 0 ? (arr)[0] : (l) == 1 ? (arr)[1] : (l) == 2 ? (arr)[2] : (arr)[3])

struct RoiBox {
  int b, lvl, H, W, ld, gh, gw;
  float inv_count;
  double y1, x1, rh, rw;
};

// -> false: the box produces zeros (hostile coordinates / batch index, or a non-positive extent)
__device__ __forceinline__ bool roi_box(const hrf_roi_levels_t& lv, const float* r, RoiBox& bx) {
  const float bf = r[0], x1 = r[1], y1 = r[2], x2 = r[3], y2 = r[4];
  if (!(bf >= 0.f && bf < (float)lv.B)) return false;                 // (NaN fails both)
  // single_level_roi_extractor.py:36-55 in fp32, the log2 as a comparison chain; num_levels == 1: level 0 (:76-79)
  const float t = sqrtf((x2 - x1) * (y2 - y1)) / lv.finest_scale + 1e-6f;
  int lvl = t >= 8.f ? 3 : t >= 4.f ? 2 : t >= 2.f ? 1 : 0;           // (a NaN scale: level 0, and a non-positive extent below)
  lvl = min(lvl, lv.num_levels - 1);
  const double ss = (double)ROI_SEL(lv.spatial_scale, lvl);
  const double ax1 = x1 * ss, ay1 = y1 * ss, ax2 = x2 * ss, ay2 = y2 * ss;
  const double lim = (double)HRF_ROI_COORD_MAX;
  if (!(fabs(ax1) <= lim && fabs(ay1) <= lim && fabs(ax2) <= lim && fabs(ay2) <= lim)) return false;   // (not finite fails too)
  bx.b = (int)bf;
  bx.lvl = lvl;
  bx.H = ROI_SEL(lv.H, lvl); bx.W = ROI_SEL(lv.W, lvl); bx.ld = ROI_SEL(lv.ld, lvl);
  bx.x1 = ax1 - 0.5; bx.y1 = ay1 - 0.5;                               // aligned=True
  bx.rw = (ax2 - 0.5) - bx.x1; bx.rh = (ay2 - 0.5) - bx.y1;
  bx.gh = (int)ceil(bx.rh / ROI_P); bx.gw = (int)ceil(bx.rw / ROI_P); // |r| <= 2^21 + 1: the conversion is safe
  if (bx.gh <= 0 || bx.gw <= 0) return false;
  bx.inv_count = (float)(1.0 / ((double)bx.gh * (double)bx.gw));
  return true;
}

// Weight table of bin p of one axis (start s, extent r > 0, `grid` samples per bin, map size n): wts[base + j] = the summed
// bilinear weight of pixel j over the bin's samples, non-zero for j in [lo, hi) only.  rng = lo[7], hi[7], base[7].
__device__ __forceinline__ void roi_axis_build(double s, double r, int grid, int n, int p, float* wts, int cap, int* rng) {
  const double bin = r / ROI_P;
  int off = 0, glo = 0, ghi = 0;
  for (int q = 0; q <= p; ++q) {               // generous pixel range of bin q: every valid sample of it lands inside
    off += ghi - glo;
    const double st = s + q * bin, en = s + (q + 1) * bin;
    const double a = fmin(fmax(floor(st) - 1.0, 0.0), (double)n), b = fmin(fmax(floor(en) + 3.0, 0.0), (double)n);
    glo = (int)a; ghi = max((int)b, glo);
  }
  const int width = max(min(ghi - glo, cap - off), 0);
  float* w = wts + off;
  for (int j = 0; j < width; ++j) w[j] = 0.f;
  int ilo = 0, ihi = grid;
  if (grid > 1) {                              // spacing bin / grid in (0.5, 1]: the samples that can lie in [-1, n]
    const double step = bin / grid, base = s + p * bin;
    const double a = floor((-1.0 - base) / step - 0.5) - 1.0, b = ceil(((double)n - base) / step - 0.5) + 2.0;
    ilo = (int)fmin(fmax(a, 0.0), (double)grid);
    ihi = (int)fmin(fmax(b, 0.0), (double)grid);
  }
  ROI_COUNT(0, max(ihi - ilo, 0));
  for (int i = ilo; i < ihi; ++i) {
    double y = s + p * bin + (i + 0.5) * bin / grid;
    if (y < -1.0 || y > (double)n) continue;
    if (y < 0.0) y = 0.0;
    int lo = (int)y, hi;
    if (lo >= n - 1) { lo = hi = n - 1; y = (double)lo; }
    else hi = lo + 1;
    const double l = y - lo, h = 1.0 - l;
    const int jl = lo - glo, jh = hi - glo;
    if ((unsigned)jl < (unsigned)width) w[jl] += (float)h;
    if ((unsigned)jh < (unsigned)width) w[jh] += (float)l;
  }
  int tl = 0, th = width;
  while (th > tl && w[th - 1] == 0.f) --th;
  while (tl < th && w[tl] == 0.f) ++tl;
  rng[p] = glo + tl; rng[ROI_P + p] = glo + th; rng[2 * ROI_P + p] = off - glo;
}

__global__ __launch_bounds__(ROI_NT) void roi_align_fwd_kernel(hrf_roi_levels_t lv, const float* rois, float* out, int layout,
                                                               int capY, int capX) {
  HRF_DYN_SMEM(float, smem);
  __shared__ int s_rng[2][3 * ROI_P];
  const int C = lv.C, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int TP = C + 1;
  float* sT = smem;                            // layout 0: [49][C + 1]
  float* sWy = smem + (layout == 0 ? ROI_NB * TP : 0);
  float* sWx = sWy + capY;
  float* o = out + (long)blockIdx.x * ROI_NB * C;
  RoiBox bx;
  if (!roi_box(lv, rois + 5L * blockIdx.x, bx)) {                     // (block-uniform)
    for (int e = tid; e < ROI_NB * C; e += ROI_NT) o[e] = 0.f;
    return;
  }
  if (tid < ROI_P) roi_axis_build(bx.y1, bx.rh, bx.gh, bx.H, tid, sWy, capY, s_rng[0]);
  else if (tid < 2 * ROI_P) roi_axis_build(bx.x1, bx.rw, bx.gw, bx.W, tid - ROI_P, sWx, capX, s_rng[1]);
  __syncthreads();
  const float* F = ROI_SEL(lv.feat, bx.lvl) + (long)bx.b * bx.H * bx.W * bx.ld + 4 * lane;
  const bool act = 4 * lane < C;
  for (int bin = wave; bin < ROI_NB; bin += ROI_NT / 64) {
    const int ph = bin / ROI_P, pw = bin - ph * ROI_P;
    const int ylo = s_rng[0][ph], yhi = s_rng[0][ROI_P + ph], xlo = s_rng[1][pw], xhi = s_rng[1][ROI_P + pw];
    const float* wy = sWy + s_rng[0][2 * ROI_P + ph];
    const float* wx = sWx + s_rng[1][2 * ROI_P + pw];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (lane == 0) ROI_COUNT(1, max(yhi - ylo, 0) * max(xhi - xlo, 0));
    for (int y = ylo; y < yhi; ++y) {
      const float vy = wy[y];
      const float* row = F + (long)y * bx.W * bx.ld;
      for (int x = xlo; x < xhi; x += 4) {      // four pixel loads in flight (a short last group repeats its last pixel at weight 0)
        float w[4];
        hrf_f4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int xu = min(x + u, xhi - 1);
          w[u] = x + u < xhi ? vy * wx[xu] : 0.f;
          if (act) v[u] = hrf_ld4(row + (long)xu * bx.ld);
        }
        if (act) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += w[u] * v[u][j];
        }
      }
    }
    if (act) {
      if (layout == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sT[bin * TP + 4 * lane + j] = acc[j] * bx.inv_count;
      } else {
        hrf_f4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = acc[j] * bx.inv_count;
        hrf_st4(o + bin * C + 4 * lane, r);
      }
    }
  }
  if (layout == 0) {                           // the box's [C][49] block, contiguous
    __syncthreads();
    for (int e = tid; e < ROI_NB * C; e += ROI_NT) {
      const int c = e / ROI_NB, bin = e - c * ROI_NB;
      o[e] = sT[bin * TP + c];
    }
  }
}

__global__ __launch_bounds__(ROI_NT) void roi_align_bwd_kernel(hrf_roi_levels_t lv, const float* rois, const float* dout, int layout,
                                                               int capY, int capX) {
  HRF_DYN_SMEM(float, smem);
  __shared__ int s_rng[2][3 * ROI_P];
  const int C = lv.C, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int TP = C + 4;
  float* sT = smem;                            // [49][C + 4]: dout / count
  float* sWy = smem + ROI_NB * TP;
  float* sWx = sWy + capY;
  RoiBox bx;
  if (!roi_box(lv, rois + 5L * blockIdx.x, bx)) return;               // (block-uniform)
  if (tid < ROI_P) roi_axis_build(bx.y1, bx.rh, bx.gh, bx.H, tid, sWy, capY, s_rng[0]);
  else if (tid < 2 * ROI_P) roi_axis_build(bx.x1, bx.rw, bx.gw, bx.W, tid - ROI_P, sWx, capX, s_rng[1]);
  const float* d = dout + (long)blockIdx.x * ROI_NB * C;
  for (int e = tid; e < ROI_NB * C; e += ROI_NT) {
    int c, bin;
    if (layout == 0) { c = e / ROI_NB; bin = e - c * ROI_NB; }
    else { bin = e / C; c = e - bin * C; }
    sT[bin * TP + c] = d[e] * bx.inv_count;
  }
  __syncthreads();
  int Y0 = bx.H, Y1 = 0, X0 = bx.W, X1 = 0;                           // the footprint: the union of the non-empty bin ranges
  for (int p = 0; p < ROI_P; ++p) {
    if (s_rng[0][p] < s_rng[0][ROI_P + p]) { Y0 = min(Y0, s_rng[0][p]); Y1 = max(Y1, s_rng[0][ROI_P + p]); }
    if (s_rng[1][p] < s_rng[1][ROI_P + p]) { X0 = min(X0, s_rng[1][p]); X1 = max(X1, s_rng[1][ROI_P + p]); }
  }
  const int nY = Y1 - Y0, nX = X1 - X0;
  if (nY <= 0 || nX <= 0) return;
  float* dF = ROI_SEL(lv.dfeat, bx.lvl) + (long)bx.b * bx.H * bx.W * bx.ld + lane;
  const int npix = nY * nX;                    // <= H * W of the level
  for (int q = wave; q < npix; q += ROI_NT / 64) {
    const int yy = q / nX, y = Y0 + yy, x = X0 + (q - yy * nX);
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    bool any = false;
    for (int ph = 0; ph < ROI_P; ++ph) {
      if (y < s_rng[0][ph] || y >= s_rng[0][ROI_P + ph]) continue;
      const float vy = sWy[s_rng[0][2 * ROI_P + ph] + y];
      for (int pw = 0; pw < ROI_P; ++pw) {
        if (x < s_rng[1][pw] || x >= s_rng[1][ROI_P + pw]) continue;
        const float w = vy * sWx[s_rng[1][2 * ROI_P + pw] + x];
        const float* t = sT + (ph * ROI_P + pw) * TP + lane;
        any = true;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (lane + 64 * j < C) g[j] += w * t[64 * j];
      }
    }
    if (!any) continue;
    if (lane == 0) ROI_COUNT(1, 1);
    float* p = dF + ((long)y * bx.W + x) * bx.ld;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane + 64 * j < C) hrf_atomic_add(p + 64 * j, g[j]);      // 256 contiguous bytes per wave instruction
  }
}

// the argument checks both entry points share -> HRF_OK with the weight tables' capacities (floats) and the dynamic LDS bytes of the launch
int roi_check(const hrf_roi_levels_t* lv, const float* rois, int K, const void* io, int layout, bool bwd, int& capY, int& capX, size_t& smem) {
  if (lv == nullptr || !hrf_roi_align_supported(lv->C, lv->pooled, lv->num_levels)) return HRF_ERR_ARG;
  if (K < 0 || lv->B < 1 || (layout != 0 && layout != 1)) return HRF_ERR_ARG;
  if (!(lv->finest_scale > 0.f) || !(lv->finest_scale < 3.0e38f)) return HRF_ERR_ARG;
  int mh = 0, mw = 0;
  for (int l = 0; l < lv->num_levels; ++l) {
    if (lv->H[l] < 1 || lv->W[l] < 1 || lv->ld[l] < lv->C || lv->feat[l] == nullptr) return HRF_ERR_ARG;
    if (bwd && lv->dfeat[l] == nullptr) return HRF_ERR_ARG;
    if (!(lv->spatial_scale[l] > 0.f) || !(lv->spatial_scale[l] < 3.0e38f)) return HRF_ERR_ARG;
    if ((long)lv->H[l] * lv->W[l] > 0x7fffffffL || lv->H[l] > (1 << 20) || lv->W[l] > (1 << 20)) return HRF_ERR_ARG;
    mh = max(mh, lv->H[l]); mw = max(mw, lv->W[l]);
  }
  if (K > 0 && (rois == nullptr || io == nullptr)) return HRF_ERR_ARG;
  capY = mh + ROI_ALLOC_SLACK; capX = mw + ROI_ALLOC_SLACK;
  const long tile = bwd ? (long)ROI_NB * (lv->C + 4) : (layout == 0 ? (long)ROI_NB * (lv->C + 1) : 0L);
  const long bytes = (tile + capY + capX) * (long)sizeof(float);
  if (bytes > ROI_SMEM_MAX) return HRF_ERR_ARG;                       // maps too large for the weight tables (H + W of ~3 700 at C = 256)
  smem = (size_t)bytes;
  return HRF_OK;
}

}  // namespace

extern "C" int hrf_roi_align_supported(int C, int pooled, int num_levels) {
  return (C >= 4 && C <= HRF_ROI_MAX_C && C % 4 == 0 && pooled == ROI_P && num_levels >= 1 && num_levels <= HRF_ROI_MAX_LEVELS) ? 1 : 0;
}

extern "C" int hrf_roi_align_fwd(const hrf_roi_levels_t* lv, const float* rois, int K, float* out, int out_layout, void* stream) {
  int capY = 0, capX = 0;
  size_t smem = 0;
  if (roi_check(lv, rois, K, out, out_layout, false, capY, capX, smem) != HRF_OK) return HRF_ERR_ARG;
  if (K == 0) return HRF_OK;
  HRF_LAUNCH(roi_align_fwd_kernel, dim3(K), dim3(ROI_NT), (unsigned)smem, stream, *lv, rois, out, out_layout, capY, capX);
  return hrf_check_launch();
}

extern "C" int hrf_roi_align_bwd(const hrf_roi_levels_t* lv, const float* rois, int K, const float* dout, int out_layout, void* stream) {
  int capY = 0, capX = 0;
  size_t smem = 0;
  if (hrf_det_on()) return HRF_ERR_ARG;        // fp32 atomics into whole activation maps: refused in deterministic mode (header)
  if (roi_check(lv, rois, K, dout, out_layout, true, capY, capX, smem) != HRF_OK) return HRF_ERR_ARG;
  if (K == 0) return HRF_OK;
  HRF_LAUNCH(roi_align_bwd_kernel, dim3(K), dim3(ROI_NT), (unsigned)smem, stream, *lv, rois, dout, out_layout, capY, capX);
  return hrf_check_launch();
}

#ifdef HRF_EMUL
extern "C" void hrf_roi_debug_iters(long* out2, int reset) {
  if (out2 != nullptr) { out2[0] = __atomic_load_n(&g_roi_iters[0], __ATOMIC_RELAXED); out2[1] = __atomic_load_n(&g_roi_iters[1], __ATOMIC_RELAXED); }
  if (reset) { __atomic_store_n(&g_roi_iters[0], 0L, __ATOMIC_RELAXED); __atomic_store_n(&g_roi_iters[1], 0L, __ATOMIC_RELAXED); }
}
#endif
