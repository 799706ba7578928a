// Eval-mode Bottleneck in ONE launch (gfx950, fp32 MFMA 32x32x2): resnet.py:263-302 with every BatchNorm frozen,
//
//   y1  = ReLU(s1 * conv1x1(x;  w1 [64][Cin]) + t1)
//   y2  = ReLU(s2 * conv3x3(y1; w2, pad 1)    + t2)
//   out = ReLU(s3 * conv1x1(y2; w3 [256][64]) + t3 + (downsample ? sd * conv1x1(x; wd [256][Cin]) + td : x))
//
// Part of the translation unit conv3x_engine.hip (included at its end): it is the packed 3x3 engine's block - 4 waves on a
// 4 x 16 pixel tile, the 6 x 18 halo at pixel pitch 68 / row pitch 1280 floats, 32 x 64 weight tiles through the 3-slot LDS
// ring with one barrier per step, every operand fetch a ds_read_b128 on the k-permuted fragments of hrf_mfma32 - with a 1x1
// GEMM in front of the 3x3 (conv1 recomputed on the halo, 108 / 64 of its useful work) and one behind it (conv3, and the
// downsample GEMM of the first block of a stream).  With frozen statistics a BatchNorm is a per-channel affine, so nothing
// crosses a tile but the 1-pixel halo of conv2 and neither 64-channel intermediate goes to memory.
//
// ONE weight-tile sequence runs through the ring from the first step to the last:
//   conv1: Cin / 32 tiles of w1 (rows = the 64 planes, 32 input channels each)           wave w: halo pixels 32 w .. 32 w + 31,
//                                                                                         both 32-channel groups (two chains)
//   conv2: 9 taps x 2 tiles of the direction-0 pack of hrf_conv3x_pack                    wave (rp, cg): 2 x 16 pixels x 32 channels
//   conv3: per 64-channel column group of the 256 outputs: [2 tiles of wd,] 2 tiles of w3 wave (rp, cg) as conv2, epilogue per group
// The A operand of conv1 comes straight from global memory (each x row is used by exactly one wave: LDS would add a copy and no
// re-use), one step ahead; y1 lives in the halo buffer, y2 in its own 64 x 68 tile, and the x tile of the downsample GEMM
// takes the halo buffer's place once conv2 is through with it.  LDS 72 704 bytes: two blocks per CU.
//
// y1 at a halo position OUTSIDE the image is ZERO (conv2 pads its input with zeros), not ReLU(t1).
#pragma once

namespace {

constexpr int BE_TH = 4;                       // tile height (XW = 16 wide)
constexpr int BE_HW = XW + 2, BE_NPH = (BE_TH + 2) * BE_HW;      // 18 x 6 = 108 halo pixels
constexpr int BE_HALO = (BE_TH + 2) * XRP;     // floats of the halo buffer
constexpr int BE_WT = 64 * 32;                 // floats of a weight tile
constexpr int BE_Y2 = BE_TH * XW * XPP;        // floats of the y2 (and the x) tile: pixel p = 16 row + column at pitch XPP
constexpr size_t BE_SMEM = (size_t)(BE_HALO + 3 * BE_WT + BE_Y2) * sizeof(float);
static_assert(BE_Y2 <= BE_HALO, "the x tile of the downsample GEMM lives in the halo buffer");

template <bool DS>
__global__ __launch_bounds__(XNT, 2) void bneck_eval_kernel(hrf_bottleneck_eval_t a, int tilesX, int tilesY, int ntiles, int per_xcd) {
  constexpr int CIN = DS ? 64 : 256;
  constexpr int N1 = CIN / 32, N2 = 18, PER = DS ? 4 : 2, N3 = 4 * PER, NT = N1 + N2 + N3;    // ring tiles per phase / block
  HRF_DYN_SMEM(float, smem);
  float* sY1 = smem;                           // [6][XRP]: y1 on the halo (0 outside the image); phase 3, DS: the x tile
  float* sW = sY1 + BE_HALO;                   // [3][BE_WT] weight ring
  float* sY2 = sW + 3 * BE_WT;                 // [64][XPP]
  float* sX = sY1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int rp = wave & 1, cg = wave >> 1;
  // XCD-aware tile order (as conv3x_kernel): XCD x walks the contiguous tile range [x per, (x + 1) per)
  int t = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (t >= ntiles) return;
  const int tx = t % tilesX; t /= tilesX;
  const int ty = t % tilesY; const int b = t / tilesY;
  const int y0 = ty * BE_TH, x0 = tx * XW;

  // ---- the weight ring: thread -> rows (tid >> 3) + 32 e of a tile, 16-byte chunk tid & 7
  const int wn = tid >> 3, wc = tid & 7;
  const int wdst = ((((wn & 15) << 1) | (wn >> 4)) << 5) + 4 * (wc ^ (wn & 7));
  hrf_f4 wreg[2];
  auto load_w = [&](int ti) X_INLINE {
    const float* p;
    int ld = 64;
    if (ti < N1) { p = a.w1 + 32 * ti; ld = CIN; }
    else if (ti < N1 + N2) { const int u = ti - N1; p = a.w2 + (u >> 1) * 4096 + 32 * (u & 1); }
    else {
      const int u = ti - N1 - N2, col = u / PER, v = u - col * PER;
      p = ((DS && v < 2) ? a.wd : a.w3) + col * 4096 + 32 * (v & 1);
    }
    p += wn * ld + 4 * wc;
#pragma unroll
    for (int e = 0; e < 2; ++e) wreg[e] = hrf_ld4(p + e * 32 * ld);
  };
  auto store_w = [&](int slot) X_INLINE {
#pragma unroll
    for (int e = 0; e < 2; ++e) xlds_st4(sW + slot * BE_WT + e * 1024 + wdst, wreg[e]);
  };
  int lt = 0;                                  // next tile to fetch
  bool have = false;
  auto ring_advance = [&](int slot) X_INLINE {  // in front of the MFMAs of the step that consumes `slot`
    if (have) { store_w(slot >= 1 ? slot - 1 : 2); have = false; }
    if (lt < NT) { load_w(lt); ++lt; have = true; }
  };

  // ---- conv1 operands: A = x of halo pixel 32 wave + j (k half h), straight from memory
  const int hp = 32 * wave + j;
  const int hpy = hp / BE_HW, hpx = hp - hpy * BE_HW;
  const int hgy = y0 - 1 + hpy, hgx = x0 - 1 + hpx;
  const bool hin = hp < BE_NPH && (unsigned)hgy < (unsigned)a.H && (unsigned)hgx < (unsigned)a.W;
  const float* xrow = hin ? a.x + ((long)(b * a.H + hgy) * a.W + hgx) * CIN + 4 * h : g_zero4x;
  const int brow = (((j & 15) << 1) | (j >> 4)) << 5;
  int bsw[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bsw[g] = 4 * ((2 * g + h) ^ (j & 7));
  hrf_f4 fa[2][4], fb[2][2][4];
  auto read1 = [&](int s, int slot, int set) X_INLINE {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      fa[set][g] = hrf_ld4(hin ? xrow + 32 * s + 8 * g : g_zero4x);
#pragma unroll
      for (int c = 0; c < 2; ++c) fb[set][c][g] = xlds_ld4(sW + slot * BE_WT + c * 1024 + brow + bsw[g]);
    }
  };

  // ---- prologue: tiles 0 and 1 into the ring, tile 2 in registers
  load_w(0); store_w(0);
  load_w(1); store_w(1);
  load_w(2); lt = 3; have = true;
  __syncthreads();

  int slot = 0;
  hrf_f16 acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc2[r] = 0.f; }

  // ---- phase 1: y1 = ReLU(s1 conv1(x) + t1) on the halo; acc / acc2 = channel groups 0 / 1 of the wave's 32 halo pixels
  read1(0, slot, 0);
#pragma unroll
  for (int s = 0; s < N1; ++s) {
    const int set = s & 1, nslot = slot == 2 ? 0 : slot + 1;
    ring_advance(slot);
    X_SCHED_FENCE();
    if (s + 1 < N1) read1(s + 1, nslot, set ^ 1);
    X_SCHED_FENCE();
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc = hrf_mfma32(fa[set][g][m], fb[set][0][g][m], acc);
        acc2 = hrf_mfma32(fa[set][g][m], fb[set][1][g][m], acc2);
      }
    X_SCHED_FENCE();
    slot = nslot;
    __syncthreads();
  }
  {
    const float sc0 = a.s1[j], sh0 = a.t1[j], sc1 = a.s1[32 + j], sh1 = a.t1[32 + j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
      const int py = p / BE_HW, px = p - py * BE_HW;
      const bool in = (unsigned)(y0 - 1 + py) < (unsigned)a.H && (unsigned)(x0 - 1 + px) < (unsigned)a.W;
      if (p < BE_NPH) {                        // zero padding of conv2's input applies AFTER BN1 + ReLU
        float* d = sY1 + py * XRP + px * XPP + j;
        d[0] = in ? fmaxf(fmaf(acc[r], sc0, sh0), 0.f) : 0.f;
        d[32] = in ? fmaxf(fmaf(acc2[r], sc1, sh1), 0.f) : 0.f;
      }
    }
  }
  // the x tile of the downsample GEMM: fetched here, stored behind conv2 (thread -> pixel (tid >> 4) + 16 e, channels 4 (tid & 15))
  hrf_f4 xt[4];
  if (DS) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int gy = y0 + e, gx = x0 + (tid >> 4);
      const bool in = gy < a.H && gx < a.W;
      xt[e] = hrf_ld4(in ? a.x + ((long)(b * a.H + gy) * a.W + gx) * CIN + 4 * (tid & 15) : g_zero4x);
    }
  }
  __syncthreads();                             // y1 complete

  // ---- phase 2: y2 = ReLU(s2 conv2(y1) + t2): the K loop of conv3x_kernel<0, 2>
  const float* abase = sY1 + (2 * rp + (j >> 4)) * XRP + (j & 15) * XPP + 4 * h;
  const float* bbase = sW + cg * 1024 + brow;
  auto read2 = [&](int u, int sl, int set) X_INLINE {
    const int tap = u >> 1, dy = tap / 3, dx = tap - 3 * dy;
    const float* ap = abase + dy * XRP + dx * XPP + 32 * (u & 1);
#pragma unroll
    for (int g = 0; g < 4; ++g) { fa[set][g] = xlds_ld4(ap + 8 * g); fb[set][0][g] = xlds_ld4(bbase + sl * BE_WT + bsw[g]); }
  };
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  read2(0, slot, 0);
  X_WAIT_LDS();
#pragma unroll
  for (int u = 0; u < N2; ++u) {
    const int set = u & 1, nslot = slot == 2 ? 0 : slot + 1;
    ring_advance(slot);
    X_SCHED_FENCE();
    if (u + 1 < N2) read2(u + 1, nslot, set ^ 1);
    X_SCHED_FENCE();
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int m = 0; m < 4; ++m) acc = hrf_mfma32(fa[set][g][m], fb[set][0][g][m], acc);
    X_SCHED_FENCE();
    slot = nslot;
    __syncthreads();
  }
  // every wave is behind the barrier of conv2's last step: the halo buffer is free
  {
    const int ch = 32 * cg + j;
    const float sc = a.s2[ch], sh = a.t2[ch];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = (2 * rp + (r >> 3)) * XW + (r & 3) + 8 * ((r >> 2) & 1) + 4 * h;
      sY2[p * XPP + ch] = fmaxf(fmaf(acc[r], sc, sh), 0.f);
    }
    if (DS) {
#pragma unroll
      for (int e = 0; e < 4; ++e) xlds_st4(sX + (e * XW + (tid >> 4)) * XPP + 4 * (tid & 15), xt[e]);
    }
  }
  __syncthreads();

  // ---- phase 3: out = ReLU(s3 conv3(y2) + t3 + identity), one 64-channel column group of the 256 outputs at a time
  // acc = conv3, acc2 = the downsample GEMM; acc[r] = pixel (row 2 rp + (r >> 3), column (r & 3) + 8 ((r >> 2) & 1) + 4 h), channel j
  const int poff = ((2 * rp + (j >> 4)) * XW + (j & 15)) * XPP + 4 * h;
  auto read3 = [&](int u, int sl, int set) X_INLINE {
    const int v = u % PER;
    const float* ap = ((DS && v < 2) ? sX : sY2) + poff + 32 * (v & 1);
#pragma unroll
    for (int g = 0; g < 4; ++g) { fa[set][g] = xlds_ld4(ap + 8 * g); fb[set][0][g] = xlds_ld4(bbase + sl * BE_WT + bsw[g]); }
  };
  read3(0, slot, 0);
  X_WAIT_LDS();
#pragma unroll
  for (int u = 0; u < N3; ++u) {
    const int set = u & 1, nslot = slot == 2 ? 0 : slot + 1;
    const int col = u / PER, v = u - col * PER;
    if (v == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc2[r] = 0.f; }
    }
    ring_advance(slot);
    X_SCHED_FENCE();
    if (u + 1 < N3) read3(u + 1, nslot, set ^ 1);
    X_SCHED_FENCE();
    if (DS && v < 2) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc2 = hrf_mfma32(fa[set][g][m], fb[set][0][g][m], acc2);
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc = hrf_mfma32(fa[set][g][m], fb[set][0][g][m], acc);
    }
    X_SCHED_FENCE();
    slot = nslot;
    __syncthreads();
    if (v == PER - 1) {
      const int ch = 64 * col + 32 * cg + j;
      const float sc = a.s3[ch], sh = a.t3[ch];
      const float dsc = DS ? a.sd[ch] : 0.f, dsh = DS ? a.td[ch] : 0.f;
      long off[16]; bool ok[16]; float idt[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int y = y0 + 2 * rp + (r >> 3), x = x0 + (r & 3) + 8 * ((r >> 2) & 1) + 4 * h;
        ok[r] = y < a.H && x < a.W;
        off[r] = ((long)(b * a.H + y) * a.W + x) * 256 + ch;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) idt[r] = DS ? fmaf(acc2[r], dsc, dsh) : *(ok[r] ? a.x + off[r] : g_zero4x);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (ok[r]) a.out[off[r]] = fmaxf(fmaf(acc[r], sc, sh) + idt[r], 0.f);
    }
  }
}

template <bool DS>
int bneck_eval_launch(const hrf_bottleneck_eval_t& a, void* stream) {
#ifndef HRF_EMUL
  static std::atomic<unsigned> lds_set{0u};
  if (hrf_dyn_lds_once(lds_set, reinterpret_cast<const void*>(&bneck_eval_kernel<DS>), (int)BE_SMEM) != HRF_OK) return HRF_ERR_LAUNCH;
#endif
  const int tilesX = hrf_cdiv(a.W, XW), tilesY = hrf_cdiv(a.H, BE_TH);
  const long nt = (long)tilesX * tilesY * a.B;
  if (nt > 0x7fffff00L) return HRF_ERR_ARG;
  const int ntiles = (int)nt, per_xcd = hrf_cdiv(ntiles, 8);
  HRF_LAUNCH((bneck_eval_kernel<DS>), dim3(per_xcd * 8), dim3(XNT), (unsigned)BE_SMEM, stream, a, tilesX, tilesY, ntiles, per_xcd);
  return hrf_check_launch();
}

}  // namespace

extern "C" int hrf_bottleneck_eval_supported(int Cin, int planes, int has_downsample) {
  if (planes != 64) return 0;
  return ((Cin == 256 && !has_downsample) || (Cin == 64 && has_downsample == 1)) ? 1 : 0;
}

extern "C" int hrf_bottleneck_eval(const hrf_bottleneck_eval_t* p, void* stream) {
  if (p == nullptr || !hrf_bottleneck_eval_supported(p->Cin, p->planes, p->has_downsample)) return HRF_ERR_ARG;
  const hrf_bottleneck_eval_t& a = *p;
  if (a.B < 1 || a.H < 1 || a.W < 1) return HRF_ERR_ARG;
  if (a.x == nullptr || a.out == nullptr || a.w1 == nullptr || a.s1 == nullptr || a.t1 == nullptr || a.w2 == nullptr || a.s2 == nullptr ||
      a.t2 == nullptr || a.w3 == nullptr || a.s3 == nullptr || a.t3 == nullptr) return HRF_ERR_ARG;
  if (a.has_downsample && (a.wd == nullptr || a.sd == nullptr || a.td == nullptr)) return HRF_ERR_ARG;
  return a.has_downsample ? bneck_eval_launch<true>(a, stream) : bneck_eval_launch<false>(a, stream);
}
