// Cascade bbox head at test time: box refinement between stages and the final softmax / per-class NMS / top-k (gfx950, fp32).
//
//   mmdet/models/roi_heads/cascade_roi_head.py:288-400 (simple_test: per stage bbox_head -> regress_by_class, the stage logits
//   averaged, the last stage's get_bboxes), bbox_heads/bbox_head.py:316-378 (get_bboxes: softmax, decode with max_shape, / scale
//   factor, multiclass_nms) and :460-497 (regress_by_class; reg_class_agnostic: the label is unused), core/post_processing/
//   bbox_nms.py:8-95 (multiclass_nms: score > score_thr, batched_nms with the class as the id, [:max_num]),
//   core/bbox/coder/delta_xywh_bbox_coder.py:224-260 (delta2bbox: deltas * stds + means first, dw / dh clamped, clip_border).
//
// Part of the translation unit pointwise.hip (included after hrf_rpn.h, whose NMS kernels it launches on its own segment table:
// one segment per class, all of the same length R).  Fixed-shape outputs, no host read of device data, no allocation, no
// synchronisation, no float atomics; every loop is bounded by R <= HRF_RPN_MAX_PRE, num_classes + 1 or the stage count.
//
//   bbox_refine_kernel      one thread per roi: (b, box) -> (b, delta2bbox(box, deltas * stds) clipped to img_shape[b]).
//   bbox_score_sort_kernel  one workgroup of 1024 per (image, class): every row's softmax score of the class over the averaged
//      stage logits, the 64-bit code (rpn_key(score) << 32 | 2^32 - 1 - row), hrf_rpn.h's bitonic sort in LDS; thread r decodes
//      the row of rank r (the same box for every class) and writes the candidate (box, score) and its valid flag.
//   rpn_nms_tile / _reduce / _merge kernels on BboxSegs: greedy NMS per (image, class), merge by score (ties: lower class, then
//      lower row - the order of the codes), dets + labels + count.
#pragma once

namespace {

// a `uniform` segment table (hrf_rpn.h, SEG_SEL): every class is one segment of n rows
struct BboxSame { int v; __host__ __device__ __forceinline__ int operator[](int) const { return v; } };
struct BboxMul { int v; __host__ __device__ __forceinline__ int operator[](int s) const { return s * v; } };
struct BboxMulL { long v; __host__ __device__ __forceinline__ long operator[](int s) const { return (long)s * v; } };
struct BboxSegs {
  static constexpr bool uniform = true;
  int nseg, ktot;                              // classes, rows of one image (nseg * n)
  BboxSame n;                                  // rows of a segment
  BboxMul off;                                 // first row within the image: s * n
  BboxMulL moff;                               // first matrix word within the image: s * words of one segment
  long mtot;                                   // matrix words of one image
};

struct BboxBox { float x1, y1, x2, y2; };

// delta2bbox of one box in the written fp32 order: d * std, dw / dh clamped to +-|log(16 / 1000)|, clipped to (img_h, img_w)
__device__ __forceinline__ BboxBox bbox_decode(const float* roi4, const float* d, float s0, float s1, float s2, float s3, float img_h, float img_w) {
  const float max_ratio = 4.135166556742356f;
  const float dx = d[0] * s0, dy = d[1] * s1;
  const float dw = rpn_clamp(d[2] * s2, -max_ratio, max_ratio), dh = rpn_clamp(d[3] * s3, -max_ratio, max_ratio);
  const float px = (roi4[0] + roi4[2]) * 0.5f, py = (roi4[1] + roi4[3]) * 0.5f, pw = roi4[2] - roi4[0], ph = roi4[3] - roi4[1];
  const float gx = px + pw * dx, gy = py + ph * dy;
  const float gw = pw * expf(dw), gh = ph * expf(dh);
  const float hw = gw * 0.5f, hh = gh * 0.5f;
  BboxBox o;
  o.x1 = rpn_clamp(gx - hw, 0.f, img_w); o.y1 = rpn_clamp(gy - hh, 0.f, img_h);
  o.x2 = rpn_clamp(gx + hw, 0.f, img_w); o.y2 = rpn_clamp(gy + hh, 0.f, img_h);
  return o;
}

__global__ __launch_bounds__(256) void bbox_refine_kernel(const float* rois_in, const float* deltas, int ldd, float s0, float s1, float s2, float s3,
                                                          const float* img_shape, int B, long K, float* rois_out) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= K) return;
  const float* ri = rois_in + r * 5;
  float* ro = rois_out + r * 5;
  const float bf = ri[0];
  ro[0] = bf;
  if (!(bf >= 0.f && bf < (float)B) || bf != floorf(bf)) {            // (NaN fails the first test) never indexes img_shape
    ro[1] = 0.f; ro[2] = 0.f; ro[3] = 0.f; ro[4] = 0.f;
    return;
  }
  const int b = (int)bf;
  const BboxBox o = bbox_decode(ri + 1, deltas + r * ldd, s0, s1, s2, s3, img_shape[2 * b], img_shape[2 * b + 1]);
  ro[1] = o.x1; ro[2] = o.y1; ro[3] = o.x2; ro[4] = o.y2;
}

__device__ __forceinline__ float bbox_unkey(unsigned k) {             // the inverse of rpn_key (0 -> a NaN)
  const unsigned u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

struct BboxDetArgs {
  const float* rois; const int* count;
  const float* logit[HRF_BBOX_MAX_STAGES]; int ldl, S;
  const float* deltas; int ldd;
  float s0, s1, s2, s3;
  const float* img_shape; const float* scale;
  float score_thr;
  int R, C;
};

__global__ __launch_bounds__(RPN_NT) void bbox_score_sort_kernel(BboxDetArgs a, float* cand, int* valid) {
  __shared__ rpn_u64 s_c[HRF_RPN_MAX_PRE];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int R = a.R, ncol = a.C + 1;
  int nsort = 2;
  while (nsort < R) nsort <<= 1;
  const float fs = (float)a.S;
  for (int r = tid; r < nsort; r += RPN_NT) {
    rpn_u64 code = 0ull;                       // (sorts behind every real code)
    if (r < R) {
      const long row = (long)b * R + r;
      // mean logit of column j: ((l_0 + l_1) + ...) / S, as sum(cls_scores) / num_stages
      auto col = [&](int j) {
        float v = a.logit[0][row * a.ldl + j];
        for (int s = 1; s < a.S; ++s) v += (s == 1 ? a.logit[1] : s == 2 ? a.logit[2] : a.logit[3])[row * a.ldl + j];
        return v / fs;
      };
      float m = col(0);
      for (int j = 1; j < ncol; ++j) { const float v = col(j); m = v > m ? v : m; }
      float sum = 0.f;
      for (int j = 0; j < ncol; ++j) sum += expf(col(j) - m);
      const float score = expf(col(c) - m) / sum;
      code = ((rpn_u64)rpn_key(score) << 32) | (rpn_u64)(0xffffffffu - (unsigned)r);
    }
    s_c[r] = code;
  }
  __syncthreads();
  for (int size = 2; size <= nsort; size <<= 1) {                      // bitonic sort, descending
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (nsort >> 1); t += RPN_NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i + j;
        const rpn_u64 x = s_c[i], y = s_c[p];
        const bool down = (i & size) == 0;
        if ((x < y) == down && x != y) { s_c[i] = y; s_c[p] = x; }
      }
      __syncthreads();
    }
  }
  const float img_h = a.img_shape[2 * b], img_w = a.img_shape[2 * b + 1];
  const int cnt = a.count != nullptr ? a.count[b] : R;
  for (int r = tid; r < R; r += RPN_NT) {
    const rpn_u64 code = s_c[r];
    const int src = (int)(0xffffffffu - (unsigned)code);               // < R: the R real codes sort before the padding
    const float score = bbox_unkey((unsigned)(code >> 32));
    const long row = (long)b * R + src;
    BboxBox o = bbox_decode(a.rois + row * 5 + 1, a.deltas + row * a.ldd, a.s0, a.s1, a.s2, a.s3, img_h, img_w);
    if (a.scale != nullptr) {
      const float* sf = a.scale + 4 * b;
      o.x1 = o.x1 / sf[0]; o.y1 = o.y1 / sf[1]; o.x2 = o.x2 / sf[2]; o.y2 = o.y2 / sf[3];
    }
    const long orow = ((long)b * a.C + c) * R + r;
    float* out = cand + 5 * orow;
    out[0] = o.x1; out[1] = o.y1; out[2] = o.x2; out[3] = o.y2; out[4] = score;
    valid[orow] = (score > a.score_thr && src < cnt) ? 1 : 0;          // (a NaN score fails)
  }
}

bool bbox_segs(int B, int R, int C, BboxSegs& sg) {
  if (B < 1 || R < 1 || R > HRF_RPN_MAX_PRE || C < 1 || C > HRF_BBOX_MAX_CLASSES || B > 65535 / HRF_BBOX_MAX_CLASSES) return false;
  sg.nseg = C; sg.n.v = R; sg.off.v = R; sg.ktot = C * R;
  sg.moff.v = (long)R * ((R + 63) / 64);
  sg.mtot = sg.moff.v * C;
  return true;
}

long bbox_det_bytes(const BboxSegs& sg, int B) {
  return rpn_align((long)B * sg.ktot * 20) + rpn_align((long)B * sg.ktot * 4) + rpn_nms_bytes(sg, B);
}

}  // namespace

extern "C" int hrf_bbox_refine(const float* rois_in, const float* deltas, int ld_deltas, float std_x, float std_y, float std_w, float std_h,
                               const float* img_shape, int B, long K, float* rois_out, void* stream) {
  if (rois_in == nullptr || deltas == nullptr || img_shape == nullptr || rois_out == nullptr || ld_deltas < 4 || B < 1 || K < 0 ||
      K > (1L << 30))
    return HRF_ERR_ARG;
  const float st[4] = {std_x, std_y, std_w, std_h};
  for (int k = 0; k < 4; ++k)
    if (!(st[k] > 0.f && st[k] < 3.0e38f)) return HRF_ERR_ARG;       // (NaN fails)
  if (K == 0) return HRF_OK;
  HRF_LAUNCH(bbox_refine_kernel, dim3(hrf_cdiv(K, 256)), dim3(256), 0, stream, rois_in, deltas, ld_deltas, std_x, std_y, std_w, std_h, img_shape,
             B, K, rois_out);
  return hrf_check_launch();
}

extern "C" long hrf_bbox_detect_workspace_bytes(int B, int R, int num_classes) {
  BboxSegs sg;
  return bbox_segs(B, R, num_classes, sg) ? bbox_det_bytes(sg, B) : 0;
}

extern "C" int hrf_bbox_detect(const hrf_bbox_det_t* d, void* workspace, long workspace_bytes, float* dets, int* labels, int* count_out,
                               void* stream) {
  BboxSegs sg;
  if (d == nullptr || !bbox_segs(d->B, d->R, d->num_classes, sg)) return HRF_ERR_ARG;
  if (d->num_stages < 1 || d->num_stages > HRF_BBOX_MAX_STAGES || d->ld_logits < d->num_classes + 1 || d->ld_deltas < 4) return HRF_ERR_ARG;
  if (d->rois == nullptr || d->deltas == nullptr || d->img_shape == nullptr || dets == nullptr || labels == nullptr || count_out == nullptr)
    return HRF_ERR_ARG;
  for (int s = 0; s < d->num_stages; ++s)
    if (d->logits[s] == nullptr) return HRF_ERR_ARG;
  for (int k = 0; k < 4; ++k)
    if (!(d->stds[k] > 0.f && d->stds[k] < 3.0e38f)) return HRF_ERR_ARG;
  if (d->max_per_img < 1 || !(d->iou_thr > 0.f && d->iou_thr <= 1.f) || !(d->score_thr >= 0.f && d->score_thr <= 1.f)) return HRF_ERR_ARG;
  if (workspace == nullptr || workspace_bytes < bbox_det_bytes(sg, d->B)) return HRF_ERR_ARG;
  char* ws = static_cast<char*>(workspace);
  float* cand = reinterpret_cast<float*>(ws);
  int* valid = reinterpret_cast<int*>(ws + rpn_align((long)d->B * sg.ktot * 20));
  char* nms = reinterpret_cast<char*>(valid) + rpn_align((long)d->B * sg.ktot * 4);
  BboxDetArgs a;
  a.rois = d->rois; a.count = d->count;
  for (int s = 0; s < HRF_BBOX_MAX_STAGES; ++s) a.logit[s] = d->logits[s < d->num_stages ? s : 0];
  a.ldl = d->ld_logits; a.S = d->num_stages;
  a.deltas = d->deltas; a.ldd = d->ld_deltas;
  a.s0 = d->stds[0]; a.s1 = d->stds[1]; a.s2 = d->stds[2]; a.s3 = d->stds[3];
  a.img_shape = d->img_shape; a.scale = d->scale_factor;
  a.score_thr = d->score_thr;
  a.R = d->R; a.C = d->num_classes;
  HRF_LAUNCH(bbox_score_sort_kernel, dim3(d->num_classes, d->B), dim3(RPN_NT), 0, stream, a, cand, valid);
  if (hrf_check_launch() != HRF_OK) return HRF_ERR_LAUNCH;
  return rpn_launch_nms(cand, valid, sg, d->B, d->max_per_img, d->iou_thr, 0, nms, dets, count_out, (float*)nullptr, labels, stream);
}
