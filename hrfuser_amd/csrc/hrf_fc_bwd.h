// Backward of hrf_fc's linear layer y = act(bias + x wp^T) (gfx950, exact fp32 MFMA): the data gradient with the ReLU mask of the
// layer below in its epilogue, and the weight / bias gradient.
//
//   hrf_fc_bwd_data    dx[m][k] = (mask && mask[m][k] <= 0) ? +0 : sum_n dy[m][n] * w[n][k]         output M x K, reduction N
//   hrf_fc_bwd_weight  dw[n][k] (+)= sum_m dy[m][n] * x[m][k],  db[n] (+)= sum_m dy[m][n]            output N x K, reduction M
//
// Part of the translation unit conv3w_engine.hip (included at its end, after hrf_fc.h).  Both run fcb_kernel: hrf_fc's block (128
// output rows x 128 output columns, 8 waves of 32 x 64, 16-deep reduction steps through a 2-slot LDS ring, global loads three steps
// ahead, v_mfma_f32_16x16x4_f32 with the same operand order) - what differs is how the operands arrive.  In both gradients the
// B operand (w resp. x) is stored with the REDUCTION index as its row, in the weight gradient the A operand (dy) too, while an
// MFMA lane (i, q) wants one element (output index i, reduction index).  Such a tile is staged as it lies in memory -
// [16 reduction rows][128 outputs], one coalesced float4 per thread, pitch 144 floats - and the fragments are read as four
// ds_read_b32 per 16 x 16 tile instead of one ds_read_b128: lanes (i, q) of MFMA j read row 4 j + q, bank (16 q + i) mod 32 in each
// 32-lane half, conflict-free.  That is wgrad3w_kernel's way; LDS has the cycles (24 such reads per 32 MFMAs of a wave and step).
// In the data gradient the A operand (dy, reduction index innermost) keeps hrf_fc's [128][20] tile and its ds_read_b128, which
// hands MFMA j the reduction index 4 q + j; the rows of the B tile are therefore stored transposed within the 4 x 4 index (global
// row 4 a + b at LDS row 4 b + a), so that row 4 j + q holds the same index.
//
// Too few output tiles (fc2: 64; the 16-row last layer): the reduction steps are split over blockIdx.z, the raw partial tiles go to
// slot z of the workspace and fcb_fold_kernel adds them in slot order and applies the epilogue (mask resp. accumulate).  No atomics:
// bit-reproducible, and the split count is a function of (M, K, N) alone.  db is one small launch of its own (fcb_bias_kernel).
#pragma once

namespace {

constexpr int FCB_PB = 128 + 16;               // pitch of a reduction-major tile: = 16 mod 32
constexpr int FCB_TARGET_BLOCKS = 512, FCB_MAX_SPLITS = 32;
constexpr int FCB_MIN_STEPS_DATA = 16, FCB_MIN_STEPS_WEIGHT = 4;

struct FcbArgs {
  const float* a; long ldA;                    // data: dy [rows][red];  weight: dy [red][rows]
  const float* b; long ldB;                    // data: w [red][cols];   weight: x [red][cols]
  float* out; long ldOut;                      // [rows][cols]
  const float* mask; long ldMask;              // data only, nullable
  int accumulate;                              // weight only
  float* part;                                 // [splits][rows][cols] when splits > 1
  long rows; int cols; long red;
  int splits, chunk;                           // chunk: reduction steps per split
};

// WG false: the data gradient (A rows hold the reduction index innermost); true: the weight gradient (A is reduction-major too)
template <bool WG>
__global__ __launch_bounds__(NTHR) void fcb_kernel(FcbArgs a) {
  constexpr int ASZ = WG ? GK * FCB_PB : GROWS * GLP, SLOT = ASZ + GK * FCB_PB;
  HRF_DYN_SMEM(float, smem);                            // [2][SLOT]: the A tile, then the B tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int chg = wave & 1, rg = wave >> 1;
  const long r0 = (long)blockIdx.x * GROWS;
  const int c0 = blockIdx.y * 128;
  const int z = blockIdx.z;
  const long s0 = (long)z * a.chunk;
  const int S = (int)min((a.red + GK - 1) / GK - s0, (long)a.chunk);          // >= 1: the launcher makes every split non-empty
  bool col_on[4], row_on[2];
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) col_on[tt] = c0 + chg * 64 + tt * 16 < a.cols;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) row_on[rr] = r0 + rg * 32 + rr * 16 < a.rows;

  hrf_f4 acc[2][4];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) acc[rr][tt] = hrf_f4{0.f, 0.f, 0.f, 0.f};

  // staging, one float4 per thread and tile.  Reduction-major tile: thread -> (reduction row tr, outputs 4 tj ..); rows past the
  // reduction length and outputs past the edge are read as zeros (both operands, so nothing non-finite meets a zero)
  const int tr = tid >> 5, tj = tid & 31;
  const float* asrc; int adst; bool aok = true;
  if (WG) {
    aok = r0 + 4 * tj < a.rows;
    asrc = a.a + r0 + 4 * tj;
    adst = tr * FCB_PB + 4 * tj;
  } else {
    const long xr = r0 + (tid >> 2) < a.rows ? r0 + (tid >> 2) : a.rows - 1;  // tail rows re-read the last row, never stored
    asrc = a.a + xr * a.ldA + 4 * (tid & 3);
    adst = (tid >> 2) * GLP + 4 * (tid & 3);
  }
  const bool bok = c0 + 4 * tj < a.cols;
  const float* bsrc = a.b + c0 + 4 * tj;
  const int bdst = ASZ + (WG ? tr : 4 * (tr & 3) + (tr >> 2)) * FCB_PB + 4 * tj;
  hrf_f4 apre, bpre;
  auto load_tile = [&](int s) {
    const long r = (s0 + s) * GK + tr;                  // the reduction row of this thread
    const bool rok = r < a.red;
    if (WG) apre = hrf_ld4(aok && rok ? asrc + r * a.ldA : g_zero4w);
    else apre = hrf_ld4(asrc + (s0 + s) * GK);
    bpre = hrf_ld4(bok && rok ? bsrc + r * a.ldB : g_zero4w);
  };
  auto store_tile = [&](int slot) {
    float* d = smem + slot * SLOT;
    lds_st4(d + adst, apre);
    lds_st4(d + bdst, bpre);
  };
  hrf_f4 fa[2][2], fb[2][4];
  const float* abase = WG ? smem + q * FCB_PB + rg * 32 + i : smem + (rg * 32 + i) * GLP + 4 * q;
  const float* bbase = smem + ASZ + q * FCB_PB + chg * 64 + i;
  auto read_frags = [&](int slot, int set) {
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      if (WG) {
#pragma unroll
        for (int m = 0; m < 4; ++m) fa[set][rr][m] = abase[slot * SLOT + 4 * m * FCB_PB + rr * 16];
      } else {
        fa[set][rr] = lds_ld4(abase + slot * SLOT + rr * 16 * GLP);
      }
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int m = 0; m < 4; ++m) fb[set][tt][m] = bbase[slot * SLOT + 4 * m * FCB_PB + tt * 16];
  };
  auto mma = [&](int set, int half) {
#pragma unroll
    for (int m = 2 * half; m < 2 * half + 2; ++m)
#pragma unroll
      for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
          if (col_on[tt] && row_on[rr]) acc[rr][tt] = hrf_mfma16(fb[set][tt][m], fa[set][rr][m], acc[rr][tt]);
  };

  load_tile(0);
  store_tile(0);
  if (S > 1) { load_tile(1); store_tile(1); }
  if (S > 2) load_tile(2);
  __syncthreads();
  read_frags(0, 0);
  HRF_WAIT_LDS();
  __syncthreads();                                      // slot 0 is rewritten in step 0: every wave holds its fragments first
  // (fc_kernel's step)
  auto step = [&](int s, int set) {
    HRF_SCHED_FENCE();
    mma(set, 0);
    HRF_SCHED_FENCE();
    if (s + 2 < S) store_tile(s & 1);
    if (s + 3 < S) load_tile(s + 3);
    read_frags((s + 1) & 1, set ^ 1);          // complete since the previous barrier (stale but valid after the last step)
    HRF_SCHED_FENCE();
    mma(set, 1);
    HRF_SCHED_FENCE();
    __syncthreads();
  };
  for (int s = 0; s < S; s += 2) {
    step(s, 0);
    if (s + 1 < S) step(s + 1, 1);
  }

  // ---- epilogue: acc[rr][tt][r] = (row r0 + rg*32 + rr*16 + i, column c0 + chg*64 + tt*16 + 4q + r)
  const bool whole = a.splits == 1;            // (uniform)
  float* obase = whole ? a.out : a.part + (long)z * a.rows * a.cols;
  const long ldo = whole ? a.ldOut : a.cols;
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) {
    if (!col_on[tt]) continue;
    const int ch = c0 + chg * 64 + tt * 16 + 4 * q;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const long m = r0 + rg * 32 + rr * 16 + i;
      if (m < a.rows) {
        hrf_f4 v = acc[rr][tt];
        if (whole) {
          if (!WG && a.mask != nullptr) {
            const hrf_f4 mk = hrf_ld4(a.mask + m * a.ldMask + ch);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = mk[r] <= 0.f ? 0.f : v[r];       // a select: a NaN mask lets the gradient through
          }
          if (WG && a.accumulate) {
            const hrf_f4 p = hrf_ld4(obase + m * ldo + ch);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += p[r];
          }
        }
        hrf_st4(obase + m * ldo + ch, v);
      }
    }
  }
}

// out[m][c .. c+3] = select(mask, (old +) (((p_0 + p_1) + p_2) + ...)) in slot order; one thread per 4 columns (cols % 16 == 0);
// splits == 0 writes zeros (old + 0 with accumulate)
__global__ __launch_bounds__(256) void fcb_fold_kernel(const float* part, int splits, long rows, int cols, float* out, long ldOut,
                                                        const float* mask, long ldMask, int accumulate) {
  const int c4 = cols >> 2;
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= rows * c4) return;
  const long m = f / c4;
  const int c = (int)(f - m * c4) * 4;
  const long slab = rows * (long)cols;
  const float* p = part + m * cols + c;
  hrf_f4 v = hrf_f4{0.f, 0.f, 0.f, 0.f};
  if (splits > 0) v = hrf_ld4(p);
  int s = 1;
  for (; s + 4 <= splits; s += 4) {            // four independent loads in flight, added in slot order
    const hrf_f4 a0 = hrf_ld4(p + s * slab), a1 = hrf_ld4(p + (s + 1) * slab), a2 = hrf_ld4(p + (s + 2) * slab), a3 = hrf_ld4(p + (s + 3) * slab);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (((v[r] + a0[r]) + a1[r]) + a2[r]) + a3[r];
  }
  for (; s < splits; ++s) {
    const hrf_f4 a0 = hrf_ld4(p + s * slab);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += a0[r];
  }
  float* o = out + m * ldOut + c;
  if (mask != nullptr) {
    const hrf_f4 mk = hrf_ld4(mask + m * ldMask + c);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = mk[r] <= 0.f ? 0.f : v[r];
  }
  if (accumulate) {
    const hrf_f4 old = hrf_ld4(o);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += old[r];
  }
  hrf_st4(o, v);
}

// db[n] (+)= sum_m dy[m][n]: block = 16 columns; 64 row groups of 4 threads sum rows g, g + 64, ..., then 16 threads add the
// groups in order.  A fixed order: the same bits every run.  The sums are kept in fp64 (M adds per column, nothing beside the
// GEMMs): db is the correctly rounded sum of the fp32 gradient rows.
__global__ __launch_bounds__(256) void fcb_bias_kernel(const float* dy, long ldDY, float* db, int accumulate, long M) {
  __shared__ double sh[64 * 16];
  const int tid = threadIdx.x, j = tid & 3, g = tid >> 2;
  const float* p = dy + blockIdx.x * 16 + 4 * j;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (long m = g; m < M; m += 64) {
    const hrf_f4 d = hrf_ld4(p + m * ldDY);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += (double)d[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) sh[g * 16 + 4 * j + r] = v[r];
  __syncthreads();
  if (tid < 16) {
    double t = 0.0;
    for (int gg = 0; gg < 64; ++gg) t += sh[gg * 16 + tid];
    float* o = db + blockIdx.x * 16 + tid;
    *o = accumulate ? *o + (float)t : (float)t;
  }
}

// dst[n][c][a] (+)= src[n][a][c]: fc1's weight gradient from the (y, x, c) column order of [K][7][7][C] features back to the
// parameter's (c, y, x).  One block per row n: the row (A * C floats, contiguous) through an LDS tile of pitch C + 1.
__global__ __launch_bounds__(256) void fcb_cols_kernel(const float* src, long ldSrc, float* dst, long ldDst, int accumulate, int C, int A) {
  HRF_DYN_SMEM(float, sm);                              // [A][C + 1]
  const float* s = src + (long)blockIdx.x * ldSrc;
  float* d = dst + (long)blockIdx.x * ldDst;
  const int total = A * C;
  for (int e = threadIdx.x; e < total; e += 256) sm[(e / C) * (C + 1) + e % C] = s[e];
  __syncthreads();
  for (int e = threadIdx.x; e < total; e += 256) {
    const float v = sm[(e % A) * (C + 1) + e / A];
    d[e] = accumulate ? d[e] + v : v;
  }
}

// splits and steps per split of `S` reduction steps over `tiles` output tiles
void fcb_plan(long tiles, long S, int min_steps, int& splits, int& chunk) {
  long want = (FCB_TARGET_BLOCKS + tiles - 1) / tiles;
  if (want > S / min_steps) want = S / min_steps;
  if (want > FCB_MAX_SPLITS) want = FCB_MAX_SPLITS;
  if (want < 1) want = 1;
  chunk = (int)((S + want - 1) / want);
  splits = (int)((S + chunk - 1) / chunk);     // every split holds at least one step
}

void fcb_plan_data(long M, int K, int N, int& splits, int& chunk) {
  fcb_plan(hrf_cdiv(M, GROWS) * hrf_cdiv(K, 128), N / GK, FCB_MIN_STEPS_DATA, splits, chunk);
}

void fcb_plan_weight(long M, int K, int N, int& splits, int& chunk) {
  fcb_plan((long)hrf_cdiv(N, GROWS) * hrf_cdiv(K, 128), (M + GK - 1) / GK, FCB_MIN_STEPS_WEIGHT, splits, chunk);
}

template <bool WG>
int launch_fcb(const FcbArgs& a, void* stream) {
  constexpr size_t smem = (size_t)2 * ((WG ? GK * FCB_PB : GROWS * GLP) + GK * FCB_PB) * sizeof(float);
#ifndef HRF_EMUL
  static std::atomic<unsigned> lds_set{0u};
  if (hrf_dyn_lds_once(lds_set, reinterpret_cast<const void*>(&fcb_kernel<WG>), (int)smem) != HRF_OK) return HRF_ERR_LAUNCH;
#endif
  const dim3 grid(hrf_cdiv(a.rows, GROWS), hrf_cdiv(a.cols, 128), a.splits);
  HRF_LAUNCH((fcb_kernel<WG>), grid, dim3(NTHR), smem, stream, a);
  return hrf_check_launch();
}

int fcb_fold(const FcbArgs& a, void* stream) {
  HRF_LAUNCH(fcb_fold_kernel, dim3(hrf_cdiv(a.rows * (a.cols / 4), 256)), dim3(256), 0, stream, (const float*)a.part, a.splits, a.rows, a.cols, a.out,
             a.ldOut, a.mask, a.ldMask, a.accumulate);
  return hrf_check_launch();
}

}  // namespace

extern "C" long hrf_fc_bwd_workspace_bytes(long M, int K, int N) {
  if (!fc_shape_ok(M, K, N) || M == 0) return 0;
  int sd, sw, chunk;
  fcb_plan_data(M, K, N, sd, chunk);
  fcb_plan_weight(M, K, N, sw, chunk);
  const long nd = sd > 1 ? (long)sd * M * K * (long)sizeof(float) : 0, nw = sw > 1 ? (long)sw * N * K * (long)sizeof(float) : 0;
  return nd > nw ? nd : nw;
}

extern "C" int hrf_fc_bwd_data(const float* dy, int ldDY, const float* w, int ldW, const float* mask, int ldMask, float* dx, int ldDX, long M, int K,
                               int N, void* workspace, long workspace_bytes, void* stream) {
  if (!fc_shape_ok(M, K, N) || dy == nullptr || w == nullptr || dx == nullptr || ldDY < N || ldW < K || ldDX < K || (mask != nullptr && ldMask < K))
    return HRF_ERR_ARG;
  int splits, chunk;
  if (M > 0) fcb_plan_data(M, K, N, splits, chunk);
  const long need = (M > 0 && splits > 1) ? (long)splits * M * K * (long)sizeof(float) : 0;
  if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return HRF_ERR_ARG;
  if (M == 0) return HRF_OK;
  FcbArgs a{dy, ldDY, w, ldW, dx, ldDX, mask, ldMask, 0, static_cast<float*>(workspace), M, K, (long)N, splits, chunk};
  const int rc = launch_fcb<false>(a, stream);
  if (rc != HRF_OK || splits == 1) return rc;
  return fcb_fold(a, stream);
}

extern "C" int hrf_fc_bwd_weight(const float* x, int ldX, const float* dy, int ldDY, float* dw, int ldDW, float* db, int accumulate, long M, int K, int N,
                                 void* workspace, long workspace_bytes, void* stream) {
  if (!fc_shape_ok(M, K, N) || x == nullptr || dy == nullptr || dw == nullptr || ldX < K || ldDY < N || ldDW < K || (accumulate != 0 && accumulate != 1))
    return HRF_ERR_ARG;
  int splits = 0, chunk = 1;
  if (M > 0) fcb_plan_weight(M, K, N, splits, chunk);
  const long need = splits > 1 ? (long)splits * N * K * (long)sizeof(float) : 0;
  if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return HRF_ERR_ARG;
  FcbArgs a{dy, ldDY, x, ldX, dw, ldDW, nullptr, 0, accumulate, static_cast<float*>(workspace), (long)N, K, M, splits, chunk};
  if (M == 0) {                                // nothing to add; accumulate == 0 still defines the outputs: zeros
    if (accumulate) return HRF_OK;
    if (fcb_fold(a, stream) != HRF_OK) return HRF_ERR_LAUNCH;
  } else {
    const int rc = launch_fcb<true>(a, stream);
    if (rc != HRF_OK) return rc;
    if (splits > 1 && fcb_fold(a, stream) != HRF_OK) return HRF_ERR_LAUNCH;
  }
  if (db != nullptr) {
    HRF_LAUNCH(fcb_bias_kernel, dim3(N / 16), dim3(256), 0, stream, dy, (long)ldDY, db, accumulate, M);
    return hrf_check_launch();
  }
  return HRF_OK;
}

extern "C" int hrf_fc_bwd_cols(const float* src, int ldSrc, float* dst, int ldDst, int accumulate, int N, int C, int A, void* stream) {
  if (src == nullptr || dst == nullptr || N < 0 || C < 1 || A < 1 || (long)A * C > (1 << 20) || ldSrc < A * C || ldDst < A * C ||
      (accumulate != 0 && accumulate != 1) || (size_t)A * (C + 1) * sizeof(float) > 64 * 1024)
    return HRF_ERR_ARG;
  if (N == 0) return HRF_OK;
  HRF_LAUNCH(fcb_cols_kernel, dim3(N), dim3(256), (size_t)A * (C + 1) * sizeof(float), stream, src, (long)ldSrc, dst, (long)ldDst, accumulate, C, A);
  return hrf_check_launch();
}
