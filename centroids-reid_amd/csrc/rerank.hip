// k-reciprocal re-ranking (Zhong et al., CVPR 2017), the sparse middle: reciprocal-neighbour sets and their expansion,
// the weight rows, local query expansion and the Jaccard blend, all on CSR rows -- no N x N matrix anywhere.  The neighbour
// table comes from the streamed top-k, the row maxima and the [nq, ng] distance matrix from creid_sqdist_matrix; the
// definition every kernel follows is spelled out at the entry points in include/creid.h.
//
// Every kernel owns one row per workgroup and keeps the row's working set in LDS; results never depend on the order in which
// lanes or workgroups run: compaction is by ballot rank, sums run in a fixed order, and the blend claims each (query, gallery)
// pair once in an LDS bitmap and computes it from sorted lists.  No floating-point atomics.
#include "common.hpp"
#include <limits.h>

namespace {

constexpr int RR_T = 256;                       // threads of the weight / expand / blend kernels (the set kernel runs one wave)
constexpr size_t RR_LDS_MAX = 64u << 10;        // dynamic LDS every kernel stays inside
constexpr int RR_TILE_BITS = 128 << 10;         // gallery entries one bitmap tile of the blend covers (16 KiB of LDS)

// in-place ascending bitonic sort of a[0 .. P) in LDS, P a power of two; ends with a barrier
template <class T>
__device__ __forceinline__ void bitonic_lds(T* a, int P, int tid, int nt) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < P; e += nt) {
        const int p = e ^ j;
        if (p > e) {
          const T x = a[e], y = a[p];
          const bool up = (e & k) == 0;
          if ((x > y) == up) { a[e] = y; a[p] = x; }
        }
      }
      __syncthreads();
    }
  }
}

// rank of this thread's flag among the set flags of an RR_T-thread workgroup (threads in order), and their number
__device__ __forceinline__ int block_rank(bool f, int* wsum, int& total) {
  const unsigned long long m = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int x = 0; x < RR_T / 64; ++x) { const int c = wsum[x]; off += x < w ? c : 0; tot += c; }
  __syncthreads();
  total = tot;
  return off + __popcll(m & lanemask_lt());
}

// ---------------------------------------------------------------------------------------------- reciprocal sets
// One wave per row i.  nb int64 [N][K]: row i's K = k1 + 1 nearest columns in (distance, index) order.
//   R(i, k1) = { j in nb[i, :K]  : i in nb[j, :K] }                      -> r1 (and the head of `list`)
//   each c in R(i, k1): R(c, kh) = { j in nb[c, :KH] : c in nb[j, :KH] }, KH = kh + 1; appended to `list` when
//   3 |R(c, kh) & R(i, k1)| > 2 |R(c, kh)|
// then `list` (at most K (KH + 1) entries) is sorted and its distinct values are the row of R*.  cols == nullptr: only the
// row length is written (count pass); else the row goes to cols[rowptr[i] ..].
__global__ __launch_bounds__(64) void rerank_recip_kernel(const int64_t* __restrict__ nb, int N, int K, int KH,
                                                           const int64_t* __restrict__ rowptr, int32_t* __restrict__ count,
                                                           int32_t* __restrict__ cols) {
  extern __shared__ __attribute__((aligned(16))) int rr_recip_smem[];
  int* r1 = rr_recip_smem;            // [K]
  int* fl = r1 + K;                   // [KH]
  int* list = fl + KH;                // [pow2 >= K (KH + 1)]
  const int i = blockIdx.x, lane = threadIdx.x;
  const unsigned long long lt = lanemask_lt();
  const int64_t* row = nb + (int64_t)i * K;
  int n1 = 0;
  for (int base = 0; base < K; base += 64) {
    const int t = base + lane;
    bool f = false;
    int j = 0;
    if (t < K) {
      const int64_t jj = row[t];
      if (jj >= 0 && jj < N) {
        j = (int)jj;
        const int64_t* rj = nb + jj * K;
        for (int u = 0; u < K; ++u) f |= rj[u] == i;
      }
    }
    const unsigned long long m = __ballot(f);
    if (f) { const int p = n1 + __popcll(m & lt); r1[p] = j; list[p] = j; }
    n1 += __popcll(m);
  }
  __syncthreads();
  int nl = n1;
  for (int ci = 0; ci < n1; ++ci) {
    const int c = r1[ci];
    const int64_t* rc = nb + (int64_t)c * K;
    int size = 0, inter = 0;
    for (int base = 0; base < KH; base += 64) {
      const int t = base + lane;
      bool f = false, in = false;
      if (t < KH) {
        const int64_t jj = rc[t];
        if (jj >= 0 && jj < N) {
          const int64_t* rj = nb + jj * K;
          for (int u = 0; u < KH; ++u) f |= rj[u] == c;
          if (f) for (int x = 0; x < n1; ++x) in |= r1[x] == (int)jj;
        }
        fl[t] = f ? (int)jj : -1;
      }
      size += __popcll(__ballot(f));
      inter += __popcll(__ballot(f && in));
    }
    __syncthreads();
    if (3 * inter > 2 * size) {
      for (int base = 0; base < KH; base += 64) {
        const int t = base + lane;
        const int j = t < KH ? fl[t] : -1;
        const unsigned long long m = __ballot(j >= 0);
        if (j >= 0) list[nl + __popcll(m & lt)] = j;
        nl += __popcll(m);
      }
    }
    __syncthreads();
  }
  int P = 1;
  while (P < nl) P <<= 1;
  for (int e = nl + lane; e < P; e += 64) list[e] = INT_MAX;
  __syncthreads();
  bitonic_lds(list, P, lane, 64);
  const int64_t o = cols ? rowptr[i] : 0;
  int run = 0;
  for (int base = 0; base < P; base += 64) {
    const int e = base + lane;
    const int v = e < P ? list[e] : INT_MAX;
    const bool f = v != INT_MAX && (e == 0 || list[e - 1] != v);
    const unsigned long long m = __ballot(f);
    if (f && cols) cols[o + run + __popcll(m & lt)] = v;
    run += __popcll(m);
  }
  if (!cols && lane == 0) count[i] = run;
}

// ---------------------------------------------------------------------------------------------- weight rows
// One workgroup per row i: x_i staged once in LDS; each wave takes listed columns j in turn, reads x_j in 16-byte loads and
// reduces the dot product over a fixed lane / butterfly order; w = exp(-d(i, j) / M_i), then the row is divided by its sum
// (wave 0, fixed order).
__global__ __launch_bounds__(RR_T) void rerank_weights_kernel(const float* __restrict__ X, const float* __restrict__ qq,
                                                               const float* __restrict__ rowmax, int D,
                                                               const int64_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ cols, float* vals) {
  extern __shared__ __attribute__((aligned(16))) float rr_w_smem[];
  float* xi = rr_w_smem;              // [D]
  float* red = xi + D;                // [1]
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = rowptr[i];
  const int len = (int)(rowptr[i + 1] - b);
  if (len == 0) return;
  const int D4 = D >> 2;
  const f32x4* xg = reinterpret_cast<const f32x4*>(X + (int64_t)i * D);
  f32x4* xi4 = reinterpret_cast<f32x4*>(xi);
  for (int k = tid; k < D4; k += RR_T) xi4[k] = xg[k];
  __syncthreads();
  const float qi = qq[i], Mi = rowmax[i];
  for (int x = w; x < len; x += RR_T / 64) {
    const int j = cols[b + x];
    const f32x4* xj = reinterpret_cast<const f32x4*>(X + (int64_t)j * D);
    float acc = 0.f;
    for (int k = lane; k < D4; k += 64) {
      const f32x4 a = xj[k], c = xi4[k];
      acc = fmaf(a.x, c.x, acc); acc = fmaf(a.y, c.y, acc); acc = fmaf(a.z, c.z, acc); acc = fmaf(a.w, c.w, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      const float d = fmaf(-2.f, acc, qi + qq[j]);
      const float od = Mi == 0.f ? 0.f : d / Mi;
      vals[b + x] = expf(-od);
    }
  }
  __syncthreads();
  if (w == 0) {
    float p = 0.f;
    for (int x = lane; x < len; x += 64) p += vals[b + x];
    p = wave_sum(p);
    if (lane == 0) red[0] = p;
  }
  __syncthreads();
  const float tot = red[0];
  for (int x = tid; x < len; x += RR_T) vals[b + x] = vals[b + x] / tot;
}

// ---------------------------------------------------------------------------------------------- local query expansion
// One workgroup per row i: the rows V(nb[i, t]), t < k2, are concatenated into LDS as (column << 32 | position) keys --
// positions ascend with t -- sorted, and every run of one column is summed in position order (= N_k2(i) order) and divided
// by k2.  cols2 == nullptr: count pass.
__global__ __launch_bounds__(RR_T) void rerank_expand_kernel(const int64_t* __restrict__ nb, int N, int K, int k2,
                                                              const int64_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ cols, const float* __restrict__ vals,
                                                              int cap, const int64_t* __restrict__ rowptr2,
                                                              int32_t* __restrict__ count2, int32_t* __restrict__ cols2,
                                                              float* __restrict__ vals2) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long rr_e_smem[];
  unsigned long long* keys = rr_e_smem;                       // [cap]
  float* sv = reinterpret_cast<float*>(keys + cap);           // [cap]
  int* off = reinterpret_cast<int*>(sv + cap);                // [k2 + 1]
  int* wsum = off + k2 + 1;                                   // [RR_T / 64]
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t* row = nb + (int64_t)i * K;
  if (tid == 0) {
    int64_t o = 0;
    for (int t = 0; t < k2; ++t) {
      const int64_t r = row[t];
      off[t] = (int)(o < cap ? o : cap);
      if (r >= 0 && r < N) o += rowptr[r + 1] - rowptr[r];
    }
    off[k2] = (int)(o <= cap ? o : -1);
  }
  __syncthreads();
  const int total = off[k2];
  if (total < 0) {                                            // the caller sized `cap` from these very lengths: not reached
    if (!cols2 && tid == 0) count2[i] = 0;
    return;
  }
  for (int t = w; t < k2; t += RR_T / 64) {
    const int64_t r = row[t];
    const int len = off[t + 1] - off[t];
    if (len <= 0) continue;
    const int64_t rb = rowptr[r];
    for (int u = lane; u < len; u += 64) {
      const int e = off[t] + u;
      keys[e] = ((unsigned long long)(unsigned)cols[rb + u] << 32) | (unsigned)e;
      sv[e] = vals[rb + u];
    }
  }
  int P = 1;
  while (P < total) P <<= 1;
  for (int e = total + tid; e < P; e += RR_T) keys[e] = ~0ull;
  __syncthreads();
  bitonic_lds(keys, P, tid, RR_T);
  const int64_t o = cols2 ? rowptr2[i] : 0;
  const float fk = (float)k2;
  int run = 0;
  for (int base = 0; base < P; base += RR_T) {
    const int e = base + tid;
    const unsigned long long key = e < P ? keys[e] : ~0ull;
    const unsigned c = (unsigned)(key >> 32);
    const bool f = key != ~0ull && (e == 0 || (unsigned)(keys[e - 1] >> 32) != c);
    int tot;
    const int rk = block_rank(f, wsum, tot);
    if (f && cols2) {
      float acc = 0.f;
      for (int x = e; x < total && (unsigned)(keys[x] >> 32) == c; ++x) acc += sv[(unsigned)keys[x]];
      cols2[o + run + rk] = (int)c;
      vals2[o + run + rk] = acc / fk;
    }
    run += tot;
  }
  if (!cols2 && tid == 0) count2[i] = run;
}

// ---------------------------------------------------------------------------------------------- blend
// dense pass: a pair whose rows share no column has Jaccard distance exactly 1
__global__ __launch_bounds__(RR_T) void rerank_blend_dense_kernel(const float* __restrict__ dist,
                                                                   const float* __restrict__ rowmax, int64_t nq, int64_t ng,
                                                                   float lambda, float* __restrict__ out) {
  const float om = 1.f - lambda;
  const int64_t total = nq * ng;
  for (int64_t e = (int64_t)blockIdx.x * RR_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * RR_T) {
    const float Mi = rowmax[e / ng];
    const float od = Mi == 0.f ? 0.f : dist[e] / Mi;
    out[e] = om + lambda * od;
  }
}

// sparse fix-up, one workgroup per query i with V'(i) in LDS.  colptr / colrows: the gallery rows of V' column-major (gallery
// indices ascending inside a column).  Per gallery tile: every gallery row listed under a column of V'(i) sets its bit
// (atomicOr on LDS words: a pair is claimed once however many columns it shares), then the set bits are walked and each
// pair's s = sum_c min(V'(i, c), V'(j, c)) is accumulated in ascending column order from row j's sorted list.
__global__ __launch_bounds__(RR_T) void rerank_blend_sparse_kernel(const float* __restrict__ dist,
                                                                    const float* __restrict__ rowmax, int nq, int ng,
                                                                    float lambda, const int64_t* __restrict__ rowptr,
                                                                    const int32_t* __restrict__ cols,
                                                                    const float* __restrict__ vals,
                                                                    const int64_t* __restrict__ colptr,
                                                                    const int32_t* __restrict__ colrows, int cap, int tile,
                                                                    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) int rr_b_smem[];
  int* ci = rr_b_smem;                                        // [cap]
  float* vi = reinterpret_cast<float*>(ci + cap);             // [cap]
  unsigned* bm = reinterpret_cast<unsigned*>(vi + cap);       // [tile / 32]
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = rowptr[i];
  int len = (int)(rowptr[i + 1] - b);
  if (len == 0) return;
  if (len > cap) len = cap;                                   // (cap is the longest query row: not reached)
  for (int x = tid; x < len; x += RR_T) { ci[x] = cols[b + x]; vi[x] = vals[b + x]; }
  const float Mi = rowmax[i], om = 1.f - lambda;
  const int words = tile >> 5;
  for (int t0 = 0; t0 < ng; t0 += tile) {
    const int t1 = min(ng, t0 + tile);
    for (int x = tid; x < words; x += RR_T) bm[x] = 0u;
    __syncthreads();
    for (int x = w; x < len; x += RR_T / 64) {
      const int c = ci[x];
      int64_t lo = colptr[c];
      const int64_t hi = colptr[c + 1];
      if (t0 > 0) {                                           // first listed gallery row >= t0
        int64_t h = hi;
        while (lo < h) { const int64_t mid = (lo + h) >> 1; if (colrows[mid] < t0) lo = mid + 1; else h = mid; }
      }
      for (int64_t p = lo + lane; p < hi; p += 64) {
        const int j = colrows[p];
        if (j >= t1) break;
        atomicOr(&bm[(j - t0) >> 5], 1u << ((j - t0) & 31));
      }
    }
    __syncthreads();
    for (int x = tid; x < words; x += RR_T) {
      unsigned bits = bm[x];
      while (bits) {
        const int bit = __ffs(bits) - 1;
        bits &= bits - 1;
        const int j = t0 + (x << 5) + bit;
        const int64_t pe = rowptr[nq + j + 1];
        float s = 0.f;
        int a = 0;
        for (int64_t p = rowptr[nq + j]; p < pe; ++p) {
          const int c = cols[p];
          while (a < len && ci[a] < c) ++a;
          if (a == len) break;
          if (ci[a] == c) s += fminf(vi[a], vals[p]);
        }
        const float J = 1.f - s / (2.f - s);
        const int64_t e = (int64_t)i * ng + j;
        const float od = Mi == 0.f ? 0.f : dist[e] / Mi;
        out[e] = om * J + lambda * od;
      }
    }
    __syncthreads();
  }
}

inline int pow2_at_least(int64_t v) { int p = 1; while (p < v) p <<= 1; return p; }

}  // namespace

extern "C" int creid_rerank_recip(const int64_t* nb, int64_t N, int32_t K, int32_t kh, const int64_t* rowptr,
                                  int32_t* count, int32_t* cols, void* stream) {
  CREID_CHECK_ARG(N >= 0 && K >= 1 && kh >= 0);
  if (N == 0) return 0;
  CREID_CHECK_ARG(nb && (cols ? rowptr != nullptr : count != nullptr));
  if (N > INT_MAX || K > 1024 || K > N || kh + 1 > K) return CREID_E_SHAPE;
  const int KH = kh + 1;
  const size_t lds = sizeof(int) * ((size_t)K + KH + pow2_at_least((int64_t)K * (KH + 1)));
  if (lds > RR_LDS_MAX) return CREID_E_SHAPE;
  hipLaunchKernelGGL(rerank_recip_kernel, dim3((unsigned)N), dim3(64), lds, as_stream(stream), nb, (int)N, (int)K, KH, rowptr,
                     count, cols);
  CREID_LAUNCH_RET();
}

extern "C" int creid_rerank_weights(const float* X, const float* qq, const float* rowmax, int64_t N, int64_t D,
                                    const int64_t* rowptr, const int32_t* cols, float* vals, void* stream) {
  CREID_CHECK_ARG(N >= 0 && D >= 1);
  if (N == 0) return 0;
  CREID_CHECK_ARG(X && qq && rowmax && rowptr);
  if (N > INT_MAX || D % 4 != 0) return CREID_E_SHAPE;
  const size_t lds = sizeof(float) * ((size_t)D + 4);
  if (lds > RR_LDS_MAX) return CREID_E_SHAPE;
  hipLaunchKernelGGL(rerank_weights_kernel, dim3((unsigned)N), dim3(RR_T), lds, as_stream(stream), X, qq, rowmax, (int)D, rowptr,
                     cols, vals);
  CREID_LAUNCH_RET();
}

extern "C" int creid_rerank_expand(const int64_t* nb, int64_t N, int32_t K, int32_t k2, const int64_t* rowptr,
                                   const int32_t* cols, const float* vals, int32_t cap, const int64_t* rowptr2,
                                   int32_t* count2, int32_t* cols2, float* vals2, void* stream) {
  CREID_CHECK_ARG(N >= 0 && K >= 1 && k2 >= 1 && cap >= 1);
  if (N == 0) return 0;
  CREID_CHECK_ARG(nb && rowptr && (cols2 ? (rowptr2 != nullptr && vals2 != nullptr) : count2 != nullptr));
  if (N > INT_MAX || K > 1024 || k2 > K || (cap & (cap - 1)) != 0) return CREID_E_SHAPE;
  const size_t lds = (size_t)cap * 12 + sizeof(int) * ((size_t)k2 + 1 + RR_T / 64);
  if (lds > RR_LDS_MAX) return CREID_E_SHAPE;
  hipLaunchKernelGGL(rerank_expand_kernel, dim3((unsigned)N), dim3(RR_T), lds, as_stream(stream), nb, (int)N, (int)K, (int)k2,
                     rowptr, cols, vals, (int)cap, rowptr2, count2, cols2, vals2);
  CREID_LAUNCH_RET();
}

extern "C" int creid_rerank_blend(const float* dist, const float* rowmax, int64_t nq, int64_t ng, float lambda,
                                  const int64_t* rowptr, const int32_t* cols, const float* vals, const int64_t* colptr,
                                  const int32_t* colrows, int32_t max_row, float* out, void* stream) {
  CREID_CHECK_ARG(nq >= 0 && ng >= 0 && max_row >= 0 && lambda >= 0.f && lambda <= 1.f);
  if (nq == 0 || ng == 0) return 0;
  CREID_CHECK_ARG(dist && rowmax && rowptr && colptr && out);
  if (nq + ng > INT_MAX) return CREID_E_SHAPE;
  const int tile = (int)(ng < RR_TILE_BITS ? (ng + 31) / 32 * 32 : RR_TILE_BITS);
  const size_t lds = (size_t)max_row * 8 + (size_t)tile / 8;
  if (lds > RR_LDS_MAX) return CREID_E_SHAPE;
  const int64_t total = nq * ng;
  const int64_t blocks = (total + RR_T - 1) / RR_T;
  hipLaunchKernelGGL(rerank_blend_dense_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(RR_T), 0,
                     as_stream(stream), dist, rowmax, nq, ng, lambda, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (max_row == 0) return 0;
  hipLaunchKernelGGL(rerank_blend_sparse_kernel, dim3((unsigned)nq), dim3(RR_T), lds, as_stream(stream), dist, rowmax, (int)nq,
                     (int)ng, lambda, rowptr, cols, vals, colptr, colrows, (int)max_row, tile, out);
  CREID_LAUNCH_RET();
}
