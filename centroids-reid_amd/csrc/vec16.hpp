// One 16-byte channel vector of an NHWC activation, as fp32 values in registers: 4 floats, 8 bf16 or 8 f16.  Shared by the
// element-wise layers (elementwise.hip) and the generalized-mean pool (gem_pool.hip).
#pragma once
#include "common.hpp"

template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
  static __device__ __forceinline__ float rnd(float v) { return v; }
};
template <> struct Vec16<unsigned short> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const unsigned short* p, float (&v)[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
  static __device__ __forceinline__ void store(unsigned short* p, const float (&v)[8]) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = f32x2_to_bf16x2_bits(v[2 * i], v[2 * i + 1]);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  static __device__ __forceinline__ float rnd(float v) { return bf16_bits_to_f32(f32_to_bf16_bits(v)); }   // value as stored
};

// An f32 -> f16 conversion whose operand the compiler sees coming out of an fma may be folded into v_fma_mixlo/hi_f16, which rounds
// the exact fma ONCE, to f16; the same expression converted with v_cvt_pk_f16_f32 rounds twice (fp32, then f16).  Which lanes of
// which kernel get the folded form is the compiler's choice (gfx950, ROCm 7: elements 6 and 7 of the second chunk of
// bn2d_bwd_apply_kernel's two-chunk loop and nowhere else), and the two differ by one f16 ulp where the fp32 value falls on an f16
// tie -- a few elements in a million, enough to break "bit-identical to the separate launches" between kernels of elementwise.hip.
// Every f16 value stored through Vec16 therefore converts from an fp32 value that is opaque to that fold: fp32 first, then f16,
// everywhere.
static __device__ __forceinline__ float f16_src(float v) { asm("" : "+v"(v)); return v; }

template <> struct Vec16<_Float16> {                            // f16 storage (the reference's own mixed precision)
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const _Float16* p, float (&v)[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = F16T::lo(w[i]); v[2 * i + 1] = F16T::hi(w[i]); }
  }
  static __device__ __forceinline__ void store(_Float16* p, const float (&v)[8]) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = F16T::pack2(f16_src(v[2 * i]), f16_src(v[2 * i + 1]));
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  static __device__ __forceinline__ float rnd(float v) { return (float)(_Float16)f16_src(v); }
};
