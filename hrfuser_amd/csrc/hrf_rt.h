// Runtime shim for the HRFuser gfx950 kernels.
//
// Product build (hipcc --offload-arch=gfx950): plain HIP, nothing else.
// Test build (-DHRF_EMUL, g++): the SAME kernel sources run on a CPU fiber emulator
// (tests/emul/emul_rt.h) so kernel index math / barriers / shuffles / MFMA fragment layouts can
// be debugged and sanitised (ASan/UBSan) without a GPU.  The emulator is test infrastructure:
// the product package never loads the emulation library.
#pragma once

#ifdef HRF_EMUL
#include "emul_rt.h"
#else
#include <hip/hip_runtime.h>
#define HRF_DYN_SMEM(T, name)                                                   \
  extern __shared__ __attribute__((aligned(16))) unsigned char hrf_dyn_smem_[]; \
  T* name = reinterpret_cast<T*>(hrf_dyn_smem_)
// every launch of the library goes through here
#define HRF_LAUNCH(kern, grid, block, smem, stream, ...) \
  hipLaunchKernelGGL(kern, grid, block, smem, (hipStream_t)(stream), __VA_ARGS__)
// LDS hand-off between lanes of ONE wave (a lane reads what another lane of its wave stored): the hardware executes a
// wave's LDS operations in program order, so only the compiler must be kept from moving code across the point
#define HRF_WAVE_SYNC() __builtin_amdgcn_wave_barrier()
typedef float hrf_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ hrf_f4 hrf_mfma16(float a, float b, hrf_f4 c) {
  // v_mfma_f32_16x16x4_f32: exact fp32 (fmaf chain), A[l&15][l>>4], B[l>>4][l&15],
  // C/D: col = lane&15, row = (lane>>4)*4 + reg.
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// 16-byte global access on 4-byte aligned addresses (gfx950 global_load/store_dwordx4 do not need
// natural alignment; NHWC rows of C = 18, 54, 78 ... floats are only 8-byte aligned)
typedef float hrf_f4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ hrf_f4 hrf_ld4(const float* p) { return *reinterpret_cast<const hrf_f4u*>(p); }
__device__ __forceinline__ void hrf_st4(float* p, hrf_f4 v) { *reinterpret_cast<hrf_f4u*>(p) = v; }
// sum over each 16-lane row (lanes sharing lane>>4) with four DPP adds - no LDS, no ds_bpermute
__device__ __forceinline__ float hrf_row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
  return v;
}
__device__ __forceinline__ void hrf_atomic_add(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void hrf_atomic_add(double* p, double v) { unsafeAtomicAdd(p, v); }
#endif

// ------------------------------------------------------------------ deterministic accumulation (hrf_set_deterministic)
// An exact, order-independent replacement of a floating-point atomic add.  An accumulator is HRF_DET_BINS signed 64-bit
// integers `stride` words apart; bin k counts units of 2^(HRF_DET_E0 + 40 k), so the four bins cover 2^-96 ... 2^64.  An addend
// is split EXACTLY into one integer of < 2^40 per bin (bits below 2^-96 are dropped per addend - still independent of the order)
// and the integers are added with 64-bit integer atomics: integer addition is associative, the bins are the same bits under
// every block / wave schedule.  Up to 2^20 addends per accumulator keep every bin below 2^60.  An addend that is not finite or
// not below 2^64 in magnitude raises bin 3 to HRF_DET_POISON with an atomic max; whatever else is added, bin 3 then stays
// above 2^60 and hrf_det_value returns NaN - the bins of a poisoned accumulator may depend on the order, its value does not.
#define HRF_DET_BINS 4
#define HRF_DET_E0 (-96)
#define HRF_DET_POISON (1LL << 62)
#define HRF_DET_LIMIT (1LL << 60)
#ifdef HRF_EMUL
inline void hrf_det_atomic_add(long long* p, long long v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline void hrf_det_atomic_max(long long* p, long long v) {
  long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
#else
__device__ __forceinline__ void hrf_det_atomic_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);       // global_atomic_add_x2
}
__device__ __forceinline__ void hrf_det_atomic_max(long long* p, long long v) { atomicMax(p, v); }
#endif
__device__ __forceinline__ void hrf_det_add(long long* bins, long stride, double v) {
  if (!(fabs(v) < 0x1p64)) { hrf_det_atomic_max(bins + 3 * stride, HRF_DET_POISON); return; }   // (NaN fails the comparison too)
  double r = v;
  // every product is a scaling by a power of two and every difference removes the leading bits of r: all exact
  double q = trunc(r * 0x1p-24);
  if (q != 0.0) { hrf_det_atomic_add(bins + 3 * stride, (long long)q); r -= q * 0x1p24; }
  q = trunc(r * 0x1p16);
  if (q != 0.0) { hrf_det_atomic_add(bins + 2 * stride, (long long)q); r -= q * 0x1p-16; }
  q = trunc(r * 0x1p56);
  if (q != 0.0) { hrf_det_atomic_add(bins + stride, (long long)q); r -= q * 0x1p-56; }
  q = trunc(r * 0x1p96);
  if (q != 0.0) hrf_det_atomic_add(bins, (long long)q);
}
// the value of an accumulator, one fixed rounding sequence: carries are propagated in integers (in place), a negative total is negated limb by limb, and the magnitude is
// summed from the top bin down (all terms of one sign: no cancellation) - relative error <= 2^-51, the same bits for the same bins
#define HRF_DET_CARRY(lo, hi) { const long long c_ = (lo) >> 40; (lo) &= (1LL << 40) - 1; (hi) += c_; }
__device__ __forceinline__ double hrf_det_value(long long b0, long long b1, long long b2, long long b3) {
  if (b3 >= HRF_DET_LIMIT || b3 <= -HRF_DET_LIMIT) return __builtin_nan("");
  HRF_DET_CARRY(b0, b1) HRF_DET_CARRY(b1, b2) HRF_DET_CARRY(b2, b3)      // lower limbs in [0, 2^40): the top one carries the sign
  const bool neg = b3 < 0;
  if (neg) {
    b0 = -b0; b1 = -b1; b2 = -b2; b3 = -b3;
    HRF_DET_CARRY(b0, b1) HRF_DET_CARRY(b1, b2) HRF_DET_CARRY(b2, b3)
  }
  const double m = (((double)b3 * 0x1p24 + (double)b2 * 0x1p-16) + (double)b1 * 0x1p-56) + (double)b0 * 0x1p-96;
  return neg ? -m : m;
}
// The mode travels IN the pointer of an accumulator argument: the entry points set bit 0 of a `stats` / gradient pointer when
// they are called in deterministic mode (the targets are 8- resp. 4-byte aligned: the bit is free), the kernels test it - a
// wave-uniform scalar test per block epilogue, no kernel signature or argument struct grows, and a captured graph keeps the
// mode its launches were issued in.
template <class T> __device__ __forceinline__ bool hrf_det_tagged(const T* p) { return ((unsigned long long)p & 1ull) != 0; }
template <class T> __device__ __forceinline__ T* hrf_det_untag(T* p) { return (T*)((unsigned long long)p & ~1ull); }

#define HRF_OK 0
#define HRF_ERR_ARG 1
#define HRF_ERR_LAUNCH 2

static inline int hrf_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

#ifndef HRF_EMUL
static inline int hrf_check_launch() {
  return hipGetLastError() == hipSuccess ? HRF_OK : HRF_ERR_LAUNCH;
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) of a kernel, once per DEVICE and safe under concurrent callers (forwards from two
// Python threads, the autograd thread): `mask` = one bit per device ordinal; racing threads both set the attribute (idempotent)
// before either publishes its bit.  (a plain `static bool once` was neither.)
#include <atomic>
static inline int hrf_dyn_lds_once(std::atomic<unsigned>& mask, const void* fn, int bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return HRF_ERR_LAUNCH;
  const unsigned bit = 1u << (dev & 31);
  if (mask.load(std::memory_order_acquire) & bit) return HRF_OK;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return HRF_ERR_LAUNCH;
  mask.fetch_or(bit, std::memory_order_release);
  return HRF_OK;
}
#else
static inline int hrf_check_launch() { return HRF_OK; }
#endif
