// Tail shared by the top-k kernels (rank.hip topk_rows_kernel: candidates of one materialised row; stream_eval.hip
// stream_topk_select_kernel: candidates the streamed contraction collected; stream_prefilter.hip stream_topk_rescore_kernel: the
// same, re-scored in fp32): a row's candidates sit in LDS as
// (order-preserving key of the fp32 distance) << 32 | gallery index, so the 64-bit order IS the (distance, index) order and
// ties resolve by gallery index like the stable rank kernel.
#pragma once
#include "common.hpp"

namespace {
__device__ __forceinline__ float tk_unkey(unsigned k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// cand[0 .. total) -> padded to the next power of two (cand must hold that many words) and bitonic-sorted ascending.  Every thread
// of the T-thread workgroup calls it, after a barrier behind the last write of cand; it ends with a barrier.
template <int T>
__device__ __forceinline__ void tk_sort(unsigned long long* cand, int total) {
  const int tid = threadIdx.x;
  int S = 1;
  while (S < total) S <<= 1;
  for (int i = total + tid; i < S; i += T) cand[i] = ~0ull;
  __syncthreads();
  for (int sz = 2; sz <= S; sz <<= 1) {
    for (int st = sz >> 1; st > 0; st >>= 1) {
      for (int i = tid; i < (S >> 1); i += T) {
        const int a = ((i / st) * st * 2) + (i % st), b = a + st;
        const bool up = ((a & sz) == 0);
        const unsigned long long x = cand[a], y = cand[b];
        if ((x > y) == up) { cand[a] = y; cand[b] = x; }
      }
      __syncthreads();
    }
  }
}

// The first k entries of the sorted list leave as out_idx[row][0 .. k) / out_dist[row][0 .. k) (out_dist nullable).
template <int T>
__device__ __forceinline__ void tk_emit(const unsigned long long* cand, int k, int64_t row, int64_t* __restrict__ out_idx,
                                        float* __restrict__ out_dist) {
  for (int t = threadIdx.x; t < k; t += T) {
    const unsigned long long c = cand[t];
    out_idx[row * k + t] = (int64_t)(c & 0xffffffffull);
    if (out_dist) out_dist[row * k + t] = tk_unkey((unsigned)(c >> 32));
  }
}

template <int T>
__device__ __forceinline__ void tk_sort_emit(unsigned long long* cand, int total, int k, int64_t row,
                                             int64_t* __restrict__ out_idx, float* __restrict__ out_dist) {
  tk_sort<T>(cand, total);
  tk_emit<T>(cand, k, row, out_idx, out_dist);
}
}  // namespace
