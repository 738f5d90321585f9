// Neighbour expansion (AQE / alpha-QE / DBA): out[i] = [self_rows[i] +] sum_t w[i][t] * x[idx[i][t]], the weighted gather behind
// reid_metric.query_expansion.  The neighbour search (topk_stream) is the expensive half; this pass is HBM-bound: (m k + m) D 4
// bytes, 1.8 GB at 17 661 + 2 228 rows, k = 10, D = 2048.
//
// One wave per destination row, four waves per workgroup.  A lane owns the 16-byte column chunks lane, lane + 64, ... of a
// 2048-column block and keeps their sums in registers (NJ float4, 32 VGPRs at D = 2048); wider rows take one block after
// another.  The row's k indices and weights are read once, one per lane (64 per batch), and handed to the whole wave by
// v_readlane, so a neighbour row's base address is scalar.  Four neighbour rows are loaded before the first of their fmafs is
// issued: 4 NJ independent 16-byte loads per lane in flight (at NJ = 8: 198 VGPRs, two waves per SIMD, 256 KiB in flight per
// CU; no scratch).  Each column's chain runs in the order of t whatever the batching, so the bits depend on neither the layout
// nor the split of m.  No LDS, no atomics, nothing between workgroups.  Measured (profiles/query_expansion.md): 5.7 TB/s at
// 206 250 rows of 8 KiB, 4.8-5.8 times the torch composition.
#include "common.hpp"
#include <math.h>

namespace {
constexpr int NX_INFLIGHT = 4;          // neighbour rows loaded ahead of their fmafs
enum { NX_ONE = 0, NX_SIM = 1, NX_POW = 2 };

template <int MODE>
__device__ __forceinline__ float nx_weight(const float* __restrict__ dist, int64_t at, float alpha) {
  if constexpr (MODE == NX_ONE) return 1.0f;
  const float sim = fminf(fmaxf(fmaf(-0.5f, dist[at], 1.0f), 0.0f), 1.0f);      // the cosine of unit rows; a NaN distance gives 0
  if constexpr (MODE == NX_SIM) return sim;
  return (float)pow((double)sim, (double)alpha);
}

__device__ __forceinline__ void nx_fma(float4& a, float w, const float4 v) {
  a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
}

__device__ __forceinline__ const float* nx_row(const float* __restrict__ x, int64_t my_idx, int t, int64_t D) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(my_idx & 0xffffffff), t);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((uint64_t)my_idx >> 32), t);
  return x + (int64_t)(((uint64_t)hi << 32) | lo) * D;
}

template <int MODE, int NJ>
__global__ __launch_bounds__(256) void neighbour_expand_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx,
                                                               const float* __restrict__ dist,
                                                               const float* __restrict__ self_rows, int64_t m, int k, int64_t D,
                                                               float alpha, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;                                     // (wave-uniform)
  constexpr int BLOCK = 64 * 4 * NJ;                        // columns of one block: 2048 at NJ = 8
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t c0 = 0; c0 < D; c0 += BLOCK) {
    const int nv = (int)((D - c0 < BLOCK ? D - c0 : BLOCK) >> 2);           // 16-byte chunks of this block
    // a lane's chunk indices, clamped into the block: every load below is unconditional (one 16-byte load each; a branch around
    // it makes the compiler split and serialise it), lanes beyond the row re-read its last chunk and store nothing
    int ch[NJ];
    float4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      ch[j] = lane + 64 * j < nv ? lane + 64 * j : nv - 1;
      acc[j] = zero;
    }
    if (self_rows) {
      const float4* sr = reinterpret_cast<const float4*>(self_rows + row * D + c0);
      float4 v[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) v[j] = sr[ch[j]];
#pragma unroll
      for (int j = 0; j < NJ; ++j) nx_fma(acc[j], 1.0f, v[j]);
    }
    for (int t0 = 0; t0 < k; t0 += 64) {
      const int kb = k - t0 < 64 ? k - t0 : 64;
      int64_t my_idx = 0;
      float my_w = 0.f;
      if (lane < kb) {
        my_idx = idx[row * k + t0 + lane];
        my_w = nx_weight<MODE>(dist, row * k + t0 + lane, alpha);
      }
      int t = 0;
      for (; t + NX_INFLIGHT <= kb; t += NX_INFLIGHT) {
        float4 v[NX_INFLIGHT][NJ];
#pragma unroll
        for (int u = 0; u < NX_INFLIGHT; ++u) {
          const float4* src = reinterpret_cast<const float4*>(nx_row(x, my_idx, t + u, D) + c0);
#pragma unroll
          for (int j = 0; j < NJ; ++j) v[u][j] = src[ch[j]];
        }
        // every load of the four rows is issued before the first fmaf: without the two fences the scheduler interleaves them
        // to save registers and a wave waits on a load two instructions after issuing it
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < NX_INFLIGHT; ++u) {
          const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_w), t + u));
#pragma unroll
          for (int j = 0; j < NJ; ++j) nx_fma(acc[j], w, v[u][j]);
        }
      }
      for (; t < kb; ++t) {                                 // the last k % 4 rows of the batch
        const float4* src = reinterpret_cast<const float4*>(nx_row(x, my_idx, t, D) + c0);
        float4 v[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[j] = src[ch[j]];
        const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_w), t));
#pragma unroll
        for (int j = 0; j < NJ; ++j) nx_fma(acc[j], w, v[j]);
      }
    }
    float4* dst = reinterpret_cast<float4*>(out + row * D + c0);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (lane + 64 * j < nv) dst[lane + 64 * j] = acc[j];
  }
}

template <int MODE>
void nx_launch(int nj, dim3 grid, hipStream_t s, const float* x, const int64_t* idx, const float* dist, const float* self_rows,
               int64_t m, int k, int64_t D, float alpha, float* out) {
  switch (nj) {
    case 1: hipLaunchKernelGGL((neighbour_expand_kernel<MODE, 1>), grid, dim3(256), 0, s, x, idx, dist, self_rows, m, k, D, alpha, out); break;
    case 2: hipLaunchKernelGGL((neighbour_expand_kernel<MODE, 2>), grid, dim3(256), 0, s, x, idx, dist, self_rows, m, k, D, alpha, out); break;
    case 4: hipLaunchKernelGGL((neighbour_expand_kernel<MODE, 4>), grid, dim3(256), 0, s, x, idx, dist, self_rows, m, k, D, alpha, out); break;
    default: hipLaunchKernelGGL((neighbour_expand_kernel<MODE, 8>), grid, dim3(256), 0, s, x, idx, dist, self_rows, m, k, D, alpha, out); break;
  }
}
}  // namespace

extern "C" {

int creid_neighbour_expand(const float* x, int64_t n_src, const int64_t* idx, const float* dist, const float* self_rows,
                           int64_t m, int32_t k, int64_t D, float alpha, float* out, void* stream) {
  if (m == 0) return 0;
  CREID_CHECK_ARG(m > 0 && k >= 0 && out && out != x && out != self_rows);
  CREID_CHECK_ARG(alpha >= 0.f && alpha <= 3.402823466e38f);                // (false for NaN)
  const int mode = alpha == 0.f ? NX_ONE : alpha == 1.f ? NX_SIM : NX_POW;  // compared once per launch
  if (k > 0) CREID_CHECK_ARG(x && idx && n_src >= 1 && (mode == NX_ONE || dist));
  if (D < 4 || D % 4 != 0 || (m + 3) / 4 > 0x7fffffffLL) return CREID_E_SHAPE;
  // the narrowest register block that covers the row in one pass; rows beyond 2048 columns loop over blocks of 2048
  const int nj = D <= 256 ? 1 : D <= 512 ? 2 : D <= 1024 ? 4 : 8;
  const dim3 grid((unsigned)((m + 3) / 4));
  hipStream_t s = as_stream(stream);
  if (mode == NX_ONE) nx_launch<NX_ONE>(nj, grid, s, x, idx, dist, self_rows, m, k, D, alpha, out);
  else if (mode == NX_SIM) nx_launch<NX_SIM>(nj, grid, s, x, idx, dist, self_rows, m, k, D, alpha, out);
  else nx_launch<NX_POW>(nj, grid, s, x, idx, dist, self_rows, m, k, D, alpha, out);
  CREID_LAUNCH_RET();
}

}  // extern "C"
