// Shared device/host helpers for libcreid_hip (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "../../include/creid.h"

#define CREID_CHECK_ARG(cond) do { if (!(cond)) return CREID_E_ARG; } while (0)
#define CREID_LAUNCH_RET() do { hipError_t e_ = hipGetLastError(); return (int)e_; } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Timing-only ablation switches (CREID_*_DRY, CREID_STREAM_NOEPI, CREID_STREAM1X1_DBG: they SKIP work, results are wrong).
// Reading one through this helper announces it on stderr, so a stray environment variable cannot silently corrupt a run.
#include <stdio.h>
#include <stdlib.h>
static inline int creid_ablation_env(const char* name) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  if (v) fprintf(stderr, "[libcreid_hip] WARNING: %s=%d is a timing-only ablation switch -- results of this process are WRONG\n", name, v);
  return v;
}

// Knobs that tests, the tuner and the probes flip INSIDE one process (kernel-variant forcing, grid caps, ablation bits).  They
// are re-read from the environment on every call only when CREID_DEBUG_KNOBS=1 was set before the library's first launch
// (tests/conftest.py and the tools under tools/ do that); otherwise every call site reads its knob ONCE: no environ scan per
// convolution launch on eager paths, and no getenv racing a setenv from another Python thread in production.
static inline bool creid_knobs_live() {
  static const bool v = [] { const char* e = getenv("CREID_DEBUG_KNOBS"); return e && atoi(e) != 0; }();
  return v;
}
// (the once-read value is an OWNED copy: a later putenv() with a caller-owned buffer or another libc may free or rewrite the
// string getenv() pointed into)
#include <string.h>
static inline const char* creid_env_copy(const char* name) { const char* e = getenv(name); return e ? strdup(e) : nullptr; }
#define CREID_KNOB_ENV(NAME) ([]() -> const char* { static const char* once_ = creid_env_copy(NAME); return creid_knobs_live() ? getenv(NAME) : once_; }())

typedef float  f32x4  __attribute__((ext_vector_type(4)));
typedef float  f32x16 __attribute__((ext_vector_type(16)));
typedef short  s16x8  __attribute__((ext_vector_type(8)));
typedef short  s16x4  __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
// lanes strictly below this lane
__device__ __forceinline__ unsigned long long lanemask_lt() {
  const int lane = threadIdx.x & 63;
  return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// bf16 <-> f32 (round-to-nearest-even), bit-level so they work in any context
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
  return __uint_as_float(((unsigned)b) << 16);
}
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
  return __builtin_bit_cast(unsigned short, (__bf16)f);   // gfx950: one v_cvt_pk_bf16_f32 (round to nearest even, quiet NaN)
}
// two floats -> packed bf16 pair (lo in bits 0..15): a single v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned f32x2_to_bf16x2_bits(float lo, float hi) {
  typedef float cvt_f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 cvt_bf16x2 __attribute__((ext_vector_type(2)));
  const cvt_f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, cvt_bf16x2));
}

// 16-bit element types of the MFMA convolution path (storage = 2 bytes per element; a "word" holds two elements, the lower
// column in bits 0..15).  bf16: the throughput mode of configs[1]; f16: the reference's own mixed precision
// (utils/misc.py:111 `precision=16`), same MFMA rate, three more mantissa bits.
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
struct Bf16T {
  static constexpr int DT = CREID_BF16;
  static constexpr unsigned ONE2 = 0x3f803f80u;                        // (1.0, 1.0)
  static __device__ __forceinline__ unsigned pack2(float lo, float hi) { return f32x2_to_bf16x2_bits(lo, hi); }
  static __device__ __forceinline__ float lo(unsigned w) { return __uint_as_float(w << 16); }
  static __device__ __forceinline__ float hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
  static __device__ __forceinline__ f32x16 mfma(s16x8 a, s16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
struct F16T {
  static constexpr int DT = CREID_F16;
  static constexpr unsigned ONE2 = 0x3c003c00u;
  static __device__ __forceinline__ unsigned pack2(float lo, float hi) {   // round to nearest even (v_cvt_f16_f32 x2 + v_pack_b32_f16)
    const h16x2 v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(unsigned, v);
  }
  static __device__ __forceinline__ float lo(unsigned w) { return (float)__builtin_bit_cast(h16x2, w)[0]; }
  static __device__ __forceinline__ float hi(unsigned w) { return (float)__builtin_bit_cast(h16x2, w)[1]; }
  static __device__ __forceinline__ f32x16 mfma(s16x8 a, s16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
  }
};
static inline bool creid_is16(int dtype) { return dtype == CREID_BF16 || dtype == CREID_F16; }
// the storage types: CREID_BF16X3 is a convolution mode (fp32 activations, split bf16 weights), accepted only by the forward
// convolutions and the weight preparation
static inline bool creid_is_storage(int dtype) { return dtype == CREID_F32 || creid_is16(dtype); }
