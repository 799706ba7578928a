// Few-rows, deep-K linear layer with bias and optional ReLU: y[m][n] = act(bias[n] + sum_k x[m][k] * wp[n][k])  (gfx950, fp32 MFMA).
//
// The fully connected layers of Shared2FCBBoxHead (mmdet/models/roi_heads/bbox_heads/convfc_bbox_head.py: shared_fcs 12544 ->
// 1024 -> 1024, fc_cls / fc_reg) at test time: M = rois (a few hundred to a few thousand), K up to 12544.  Part of the
// translation unit conv3w_engine.hip (included at its end): the tile machinery is rowgemm_kernel's - 128 rows x WN * 64 columns
// per block, 16-deep K steps through a 2-slot LDS ring, global loads three steps ahead, exact fp32 v_mfma_f32_16x16x4_f32 with
// the same operand order - so one (row, column, K range) is the same fmaf chain as hrf_rowgemm's.  What hrf_rowgemm lacks at this
// shape is blocks: 16 x 8 of them at M = 2000, N = 1024, each 784 steps deep.  Here the K steps are SPLIT over blockIdx.z:
//   1  fc_kernel       block (m tile, n tile, split z) runs steps [z * chunk, min(S, (z + 1) * chunk)) and stores its raw partial
//                      tile into slot z of the workspace, [splits][M][N]; with one split it applies bias / ReLU and stores y.
//   2  fc_fold_kernel  y = act(bias + (((p_0 + p_1) + p_2) + ...)): the slots folded in slot order by one thread per 4 columns.
// No atomics, no arrival counters: the result does not depend on the order in which blocks run (bit-reproducible), and the
// split count is a function of (M, K, N) alone.  splits = ceil(FC_TARGET_BLOCKS / (m tiles * n tiles)), at least FC_MIN_STEPS
// steps per split, at most FC_MAX_SPLITS: 512 blocks at M = 2000, K = 12544, N = 1024 (4 splits of 196 steps) on 256 CUs.
#pragma once

namespace {

constexpr int FC_TARGET_BLOCKS = 512, FC_MIN_STEPS = 16, FC_MAX_SPLITS = 32;

struct FcArgs {
  const float* x; int ldX; const float* wp; const float* bias;
  float* y; int ldY; int relu;
  float* part;                                 // [splits][M][N] when splits > 1
  long M; int K, N, splits, chunk;             // chunk: K steps per split
};

__device__ __forceinline__ float fc_act(float v, int relu) { return (relu && v < 0.f) ? 0.f : v; }      // (keeps a NaN, as torch.relu)

template <int WN>
__global__ __launch_bounds__(NTHR) void fc_kernel(FcArgs a) {
  constexpr int NB = WN * 64, SLOT = (GROWS + NB) * GLP;
  constexpr int NWV = (NB * 4 + NTHR - 1) / NTHR;      // weight float4 per thread
  HRF_DYN_SMEM(float, smem);                            // [2][SLOT]: x tile rows first, then the weight rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int chg = wave % WN, rg = wave / WN;
  const long m0 = (long)blockIdx.x * GROWS;
  const int n0 = blockIdx.y * NB;
  const int z = blockIdx.z;
  const int s0 = z * a.chunk;
  const int S = min(a.K / GK - s0, a.chunk);            // >= 1: the launcher makes every split non-empty
  bool tile_on[4];
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) tile_on[tt] = n0 + chg * 64 + tt * 16 < a.N;

  hrf_f4 acc[WN][4];
#pragma unroll
  for (int rr = 0; rr < WN; ++rr)
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) acc[rr][tt] = hrf_f4{0.f, 0.f, 0.f, 0.f};

  // staging: x tile = 128 rows x 4 float4 (one per thread); weight tile = NB rows x 4 float4
  const long xr = m0 + (tid >> 2) < a.M ? m0 + (tid >> 2) : a.M - 1;          // tail rows re-read the last row, never stored
  const float* xsrc = a.x + xr * a.ldX + (long)s0 * GK + 4 * (tid & 3);
  const int xdst = (tid >> 2) * GLP + 4 * (tid & 3);
  const float* wsrc[NWV]; int wdst[NWV];
#pragma unroll
  for (int e = 0; e < NWV; ++e) {
    const int f = tid + e * NTHR, n = min(f >> 2, NB - 1);
    wsrc[e] = a.wp + (long)min(n0 + n, a.N - 1) * a.K + (long)s0 * GK + 4 * (f & 3);
    wdst[e] = f < NB * 4 ? (GROWS + n) * GLP + 4 * (f & 3) : -1;
  }
  hrf_f4 xpre, wpre[NWV];
  auto load_tile = [&](int s) {
    xpre = hrf_ld4(xsrc + s * GK);
#pragma unroll
    for (int e = 0; e < NWV; ++e) wpre[e] = hrf_ld4(wsrc[e] + s * GK);
  };
  auto store_tile = [&](int slot) {
    float* d = smem + slot * SLOT;
    lds_st4(d + xdst, xpre);
#pragma unroll
    for (int e = 0; e < NWV; ++e)
      if (wdst[e] >= 0) lds_st4(d + wdst[e], wpre[e]);
  };
  hrf_f4 fa[2][WN], fb[2][4];
  const float* abase = smem + (rg * 16 * WN + i) * GLP + 4 * q;
  const float* bbase = smem + (GROWS + chg * 64 + i) * GLP + 4 * q;
  auto read_frags = [&](int slot, int set) {
#pragma unroll
    for (int rr = 0; rr < WN; ++rr) fa[set][rr] = lds_ld4(abase + slot * SLOT + rr * 16 * GLP);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) fb[set][tt] = lds_ld4(bbase + slot * SLOT + tt * 16 * GLP);
  };
  auto mma = [&](int set, int half) {
#pragma unroll
    for (int m = 2 * half; m < 2 * half + 2; ++m)
#pragma unroll
      for (int rr = 0; rr < WN; ++rr)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
          if (tile_on[tt]) acc[rr][tt] = hrf_mfma16(fb[set][tt][m], fa[set][rr][m], acc[rr][tt]);
  };

  load_tile(0);
  store_tile(0);
  if (S > 1) { load_tile(1); store_tile(1); }
  if (S > 2) load_tile(2);
  __syncthreads();
  read_frags(0, 0);
  HRF_WAIT_LDS();
  __syncthreads();                                      // slot 0 is rewritten in step 0: every wave holds its fragments first
  // (rowgemm_kernel's step) MFMAs of step s on fragment set `set`, the tile of step s+2 written into slot s%2, the fragments of
  // step s+1 fetched from the other slot half-way
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

  // ---- epilogue: acc[rr][tt][r] = (row m0 + rg*16*WN + rr*16 + i, column n0 + chg*64 + tt*16 + 4q + r)
  const bool whole = a.splits == 1;            // (uniform)
  float* obase = whole ? a.y : a.part + (long)z * a.M * a.N;
  const long ldo = whole ? a.ldY : a.N;
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) {
    if (!tile_on[tt]) continue;
    const int ch = n0 + chg * 64 + tt * 16 + 4 * q;
    hrf_f4 bv = hrf_f4{0.f, 0.f, 0.f, 0.f};
    if (whole && a.bias != nullptr) bv = hrf_ld4(a.bias + ch);
#pragma unroll
    for (int rr = 0; rr < WN; ++rr) {
      const long m = m0 + rg * 16 * WN + rr * 16 + i;
      if (m < a.M) {
        hrf_f4 v = acc[rr][tt];
        if (whole) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fc_act(bv[r] + v[r], a.relu);
        }
        hrf_st4(obase + m * ldo + ch, v);
      }
    }
  }
}

// y[m][n .. n+3] = act(bias + p_0 + p_1 + ... ) in slot order; one thread per 4 columns (N % 16 == 0)
__global__ __launch_bounds__(256) void fc_fold_kernel(const float* part, const float* bias, float* y, int ldY, int relu, long M, int N, int splits) {
  const int n4 = N >> 2;
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= M * n4) return;
  const long m = f / n4;
  const int n = (int)(f - m * n4) * 4;
  const long slab = M * (long)N;
  const float* p = part + m * N + n;
  hrf_f4 v = hrf_ld4(p);
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
  hrf_f4 bv = hrf_f4{0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr) bv = hrf_ld4(bias + n);
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = fc_act(bv[r] + v[r], relu);
  hrf_st4(y + m * ldY + n, v);
}

// the decomposition of a shape: 64-column groups per block, K splits and steps per split
void fc_plan(long M, int K, int N, int& wn, int& splits, int& chunk) {
  wn = N > 64 ? 2 : 1;
  const long blocks = ((M + GROWS - 1) / GROWS) * ((N + wn * 64 - 1) / (wn * 64));
  const int S = K / GK;
  long want = (FC_TARGET_BLOCKS + blocks - 1) / blocks;
  if (want > S / FC_MIN_STEPS) want = S / FC_MIN_STEPS;
  if (want > FC_MAX_SPLITS) want = FC_MAX_SPLITS;
  if (want > S) want = S;
  if (want < 1) want = 1;
  chunk = (S + (int)want - 1) / (int)want;
  splits = (S + chunk - 1) / chunk;            // every split holds at least one step
}

bool fc_shape_ok(long M, int K, int N) {
  return K > 0 && N > 0 && K % GK == 0 && N % 16 == 0 && M >= 0 && M <= (1L << 24) && N <= (1 << 16);      // (grid extents and the slot offsets stay in range)
}

template <int WN>
int launch_fc(const FcArgs& a, void* stream) {
  constexpr size_t smem = (size_t)2 * (GROWS + WN * 64) * GLP * sizeof(float);
#ifndef HRF_EMUL
  static std::atomic<unsigned> lds_set{0u};
  if (hrf_dyn_lds_once(lds_set, reinterpret_cast<const void*>(&fc_kernel<WN>), (int)smem) != HRF_OK) return HRF_ERR_LAUNCH;
#endif
  const dim3 grid(hrf_cdiv(a.M, GROWS), hrf_cdiv(a.N, WN * 64), a.splits);
  HRF_LAUNCH((fc_kernel<WN>), grid, dim3(NTHR), smem, stream, a);
  return hrf_check_launch();
}

}  // namespace

extern "C" long hrf_fc_workspace_bytes(long M, int K, int N) {
  if (!fc_shape_ok(M, K, N) || M == 0) return 0;
  int wn, splits, chunk;
  fc_plan(M, K, N, wn, splits, chunk);
  return splits > 1 ? (long)splits * M * N * (long)sizeof(float) : 0;
}

extern "C" int hrf_fc_pack(const float* w, int N, int K, int Np, int Kp, float* wp, void* stream) {
  if (w == nullptr || wp == nullptr || N < 1 || K < 1 || Np < N || Kp < K || Np % 16 != 0 || Kp % GK != 0) return HRF_ERR_ARG;
  return hrf_rowgemm_pack(w, N, K, 0, Np, Kp, wp, stream);
}

extern "C" int hrf_fc(const float* x, int ldX, const float* wp, const float* bias, float* y, int ldY, int relu, long M, int K, int N,
                      void* workspace, long workspace_bytes, void* stream) {
  if (!fc_shape_ok(M, K, N) || x == nullptr || wp == nullptr || y == nullptr || ldX < K || ldY < N || (relu != 0 && relu != 1)) return HRF_ERR_ARG;
  if (M == 0) return HRF_OK;
  int wn, splits, chunk;
  fc_plan(M, K, N, wn, splits, chunk);
  const long need = splits > 1 ? (long)splits * M * N * (long)sizeof(float) : 0;
  if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return HRF_ERR_ARG;
  FcArgs a{x, ldX, wp, bias, y, ldY, relu, static_cast<float*>(workspace), M, K, N, splits, chunk};
  const int rc = wn == 2 ? launch_fc<2>(a, stream) : launch_fc<1>(a, stream);
  if (rc != HRF_OK || splits == 1) return rc;
  HRF_LAUNCH(fc_fold_kernel, dim3(hrf_cdiv(M * (N / 4), 256)), dim3(256), 0, stream, (const float*)a.part, bias, y, ldY, relu, M, N, splits);
  return hrf_check_launch();
}
