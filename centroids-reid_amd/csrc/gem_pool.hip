// Generalized-mean pooling (GeM, Radenovic et al., TPAMI 2019) over the final NHWC feature map, with a trainable exponent:
//   u = max(x, eps),  m = mean_hw u^p,  y = m^(1/p)                                    (feat fp32 [B, C])
// The opt-in replacement of the global average pool (elementwise.hip: gap_fwd_kernel / gap_bwd_kernel); same access pattern:
// 32 channel vectors x 8 row lanes per workgroup, grid (C/V/32, B), lane partials meeting in LDS in a fixed order.
//
// Scaled form.  eps^p leaves the fp32 normal range near p = 6.3 and 65504^8 is far above it, so no u^p is ever formed.  With
// U = max_hw u (one extra pass over the workgroup's slice of the map, which the first pass has just pulled into the cache),
//   r = u / U in (0, 1],  r^p = exp2(p * log2 r),  S = sum_hw r^p in [1, HW],  T = sum_hw r^p * log2 r <= 0
//   y = U * (S / HW)^(1/p)
// r is an IEEE division, so the largest element gives r = 1 and r^p = 1 exactly: a channel that is constant over the map (all
// zeros after the ReLU, or everything below eps) gives S = HW and y = U with no rounding at all.  The (S / HW)^(1/p) of the B * C
// outputs is evaluated in fp64; per element everything is fp32 (v_log_f32 / v_exp_f32).
//
// What the forward saves per (b, c) for the backward (stats [3][B][C] fp32), so that the backward never re-reduces the map:
//   U   the maximum
//   k   (1 / HW) * (S / HW)^(1/p - 1)              dx_i = dy * k * r_i^(p - 1)   where x_i >= eps, else a true zero
//   q   y * (T ln2 / (S p) - ln(S / HW) / p^2)     dp   = sum_{b, c} dy * q
// q is the definition's  y * ((sum u^p ln u) / (HW m p) - ln(m) / p^2)  with  ln u = ln U + ln r  and  ln m = p ln U + ln(S / HW)
// put in: the two ln U terms cancel exactly, in algebra instead of in floating point.
//
// dp is deterministic: one partial per workgroup (a fixed-order wave butterfly over its 32 V channels), then a one-workgroup
// kernel adds the partials in a fixed order to *p_grad.  No floating-point atomics, no tickets.
// p is read from device memory: the training step is a captured graph and the optimiser rewrites p on the device.
#include "vec16.hpp"

template <typename T, bool SAVE>
__global__ __launch_bounds__(256) void gem_fwd_kernel(const T* __restrict__ x, int HW, int C, const float* __restrict__ p_ptr,
                                                      float eps, float* __restrict__ out, float* __restrict__ stats,
                                                      int64_t BC, int64_t* __restrict__ counter) {
  constexpr int V = Vec16<T>::N;
  __shared__ float red_s[8][32][V + 1];
  __shared__ float red_t[8][32][V + 1];
  __shared__ float umax[32][V + 1];
  if (counter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *counter += 1;   // the training forward's step count
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int b = blockIdx.y, cc = blockIdx.x * 32 + cl;
  const bool live = cc * V < C;
  const float p = *p_ptr;
  const T* px = x + (int64_t)b * HW * C + cc * V;
  // pass 1: the maximum of max(x, eps) over this lane's rows, then over the eight row lanes
  float U[V];
#pragma unroll
  for (int k = 0; k < V; ++k) U[k] = eps;
  if (live) {
    for (int i = rl; i < HW; i += 8) {
      float v[V];
      Vec16<T>::load(px + (int64_t)i * C, v);
#pragma unroll
      for (int k = 0; k < V; ++k) U[k] = fmaxf(U[k], v[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) red_s[rl][cl][k] = U[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < V; ++k) {
    float a = red_s[0][cl][k];
#pragma unroll
    for (int q = 1; q < 8; ++q) a = fmaxf(a, red_s[q][cl][k]);
    U[k] = a;
  }
  if (rl == 0) {
#pragma unroll
    for (int k = 0; k < V; ++k) umax[cl][k] = U[k];
  }
  __syncthreads();                                       // red_s is written again below
  // pass 2: S = sum r^p and (training) T = sum r^p log2 r.  A quotient that flushes to zero (u / U below the normal range) has
  // log2 = -inf; the floor keeps 0 * inf out of T, its r^p is 0 either way.
  float S[V], Tn[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { S[k] = 0.f; Tn[k] = 0.f; }
  if (live) {
    for (int i = rl; i < HW; i += 8) {
      float v[V];
      Vec16<T>::load(px + (int64_t)i * C, v);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float r = fmaxf(v[k], eps) / U[k];
        const float lr = fmaxf(__builtin_amdgcn_logf(r), -256.f);
        const float t = __builtin_amdgcn_exp2f(p * lr);
        S[k] += t;
        if constexpr (SAVE) Tn[k] += t * lr;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    red_s[rl][cl][k] = S[k];
    if constexpr (SAVE) red_t[rl][cl][k] = Tn[k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 32 * V; e += 256) {
    const int c2 = e / V, k = e - c2 * V;
    const int ch = (blockIdx.x * 32 + c2) * V + k;
    if (ch < C) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) s += red_s[q][c2][k];
      const double ip = 1.0 / (double)p;
      const double lz = log2((double)s / (double)HW);                    // in [-log2 HW, 0]
      const double um = (double)umax[c2][k];
      const double y = um * exp2(lz * ip);
      const int64_t o = (int64_t)b * C + ch;
      out[o] = (float)y;
      if constexpr (SAVE) {
        float tt = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) tt += red_t[q][c2][k];
        constexpr double LN2 = 0.69314718055994530942;
        stats[o] = (float)um;
        stats[BC + o] = (float)(exp2(lz * (ip - 1.0)) / (double)HW);
        stats[2 * BC + o] = (float)(y * LN2 * ip * ((double)tt / (double)s - lz * ip));
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gem_bwd_kernel(const T* __restrict__ x, const float* __restrict__ dy,
                                                      const float* __restrict__ stats, int64_t BC, int HW, int C,
                                                      const float* __restrict__ p_ptr, float eps, T* __restrict__ dx,
                                                      float* __restrict__ partial) {
  constexpr int V = Vec16<T>::N;
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int b = blockIdx.y, cc = blockIdx.x * 32 + cl;
  const bool live = cc * V < C;
  const float pm1 = *p_ptr - 1.f;
  float dpl = 0.f;
  if (live) {
    const int64_t o = (int64_t)b * C + cc * V;
    float U[V], g[V];
#pragma unroll
    for (int k = 0; k < V; k += 4) {
      const float4 u4 = *reinterpret_cast<const float4*>(stats + o + k);
      const float4 k4 = *reinterpret_cast<const float4*>(stats + BC + o + k);
      const float4 d4 = *reinterpret_cast<const float4*>(dy + o + k);
      U[k] = u4.x; U[k + 1] = u4.y; U[k + 2] = u4.z; U[k + 3] = u4.w;
      g[k] = d4.x * k4.x; g[k + 1] = d4.y * k4.y; g[k + 2] = d4.z * k4.z; g[k + 3] = d4.w * k4.w;
      if (partial && rl == 0) {                          // this workgroup's share of dp = sum dy * q, channels in order
        const float4 q4 = *reinterpret_cast<const float4*>(stats + 2 * BC + o + k);
        dpl += d4.x * q4.x; dpl += d4.y * q4.y; dpl += d4.z * q4.z; dpl += d4.w * q4.w;
      }
    }
    const int64_t base = (int64_t)b * HW * C + cc * V;
    for (int i = rl; i < HW; i += 8) {
      float v[V], w[V];
      Vec16<T>::load(x + base + (int64_t)i * C, v);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float r = fmaxf(v[k], eps) / U[k];
        const float f = __builtin_amdgcn_exp2f(pm1 * fmaxf(__builtin_amdgcn_logf(r), -256.f));
        w[k] = v[k] >= eps ? g[k] * f : 0.f;             // the gradient of clamp(min = eps): a true zero below eps
      }
      Vec16<T>::store(dx + base + (int64_t)i * C, w);
    }
  }
  if (partial && threadIdx.x < 64) {                     // wave 0: lanes 0..31 are row lane 0, lanes 32..63 carry zeros
    const float s = wave_sum(dpl);
    if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// *p_grad += the sum of the n workgroup partials, in an order that depends on n alone
__global__ __launch_bounds__(256) void gem_dp_sum_kernel(const float* __restrict__ partial, int64_t n, float* __restrict__ p_grad) {
  __shared__ float red[256];
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) a += partial[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) p_grad[0] += red[0];
}

static inline int64_t gem_vec(int dtype) { return dtype == CREID_F32 ? 4 : 8; }

#define GEM_FWD(T, SAVE)                                                                                              \
  hipLaunchKernelGGL((gem_fwd_kernel<T, SAVE>), grid, dim3(256), 0, s, (const T*)x, (int)HW, (int)C, p, eps, feat, stats, \
                     B * C, forward_counter)
#define GEM_BWD(T)                                                                                                    \
  hipLaunchKernelGGL(gem_bwd_kernel<T>, grid, dim3(256), 0, s, (const T*)x, dfeat, stats, B * C, (int)HW, (int)C, p, eps, \
                     (T*)dx, p_grad ? partials : nullptr)

extern "C" {

int64_t creid_gem_bwd_partials(int64_t B, int64_t C, int dtype) {
  if (!creid_is_storage(dtype) || B <= 0 || C <= 0) return 0;
  const int64_t v = gem_vec(dtype);
  return B * ((C / v + 31) / 32);
}

int creid_gem_fwd(const void* x, int64_t B, int64_t HW, int64_t C, int dtype, const float* p, float eps, float* feat,
                  float* stats, int64_t* forward_counter, void* stream) {
  if (!creid_is_storage(dtype)) return CREID_E_DTYPE;
  CREID_CHECK_ARG(x && p && feat && B > 0 && B <= 65535 && HW > 0 && HW < ((int64_t)1 << 31) && C > 0 && C < ((int64_t)1 << 31) &&
                  C % gem_vec(dtype) == 0 && eps > 0.f);
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)((C / gem_vec(dtype) + 31) / 32), (unsigned)B);
  if (stats) {
    if (dtype == CREID_F32) GEM_FWD(float, true);
    else if (dtype == CREID_BF16) GEM_FWD(unsigned short, true);
    else GEM_FWD(_Float16, true);
  } else {
    if (dtype == CREID_F32) GEM_FWD(float, false);
    else if (dtype == CREID_BF16) GEM_FWD(unsigned short, false);
    else GEM_FWD(_Float16, false);
  }
  CREID_LAUNCH_RET();
}

int creid_gem_bwd(const void* x, const float* dfeat, const float* stats, int64_t B, int64_t HW, int64_t C, int dtype,
                  const float* p, float eps, void* dx, float* p_grad, float* partials, void* stream) {
  if (!creid_is_storage(dtype)) return CREID_E_DTYPE;
  CREID_CHECK_ARG(x && dfeat && stats && p && dx && (!p_grad || partials) && B > 0 && B <= 65535 && HW > 0 &&
                  HW < ((int64_t)1 << 31) && C > 0 && C < ((int64_t)1 << 31) && C % gem_vec(dtype) == 0 && eps > 0.f);
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)((C / gem_vec(dtype) + 31) / 32), (unsigned)B);
  if (dtype == CREID_F32) GEM_BWD(float);
  else if (dtype == CREID_BF16) GEM_BWD(unsigned short);
  else GEM_BWD(_Float16);
  if (p_grad)
    hipLaunchKernelGGL(gem_dp_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)partials, (int64_t)grid.x * grid.y, p_grad);
  CREID_LAUNCH_RET();
}

}  // extern "C"
