// Camera-aware centroid index (modelling/bases.py:205-236 of the reference) built ON THE DEVICE from the raw label vectors.
//
// For every gallery pid and every distinct camera `cur` of its QUERIES the reference forms one centroid of the pid's gallery
// rows from the other cameras, de-duplicated by the tuple of cameras it was built from.  In closed form, per gallery pid
// (ascending) with gmask = OR of its rows' cameras, qmask = OR of its queries' cameras, for cur over the bits of qmask
// (ascending):
//   cur in gmask    : used = gmask & ~(1 << cur); used == 0 -> nothing; else one centroid of the rows with camera != cur;
//   cur not in gmask: the FIRST such cur gives one centroid of all the pid's rows with set gmask, later ones nothing.
// The reference looks a gallery row's camera up with the gallery-relative index on the FULL vector (:214): row j of the gallery
// has camera camids[j], not camids[num_query + j].  That is kept: `cams` below is the full vector from its start.
//
// Counting sort over the dense pid range [pmin, pmin + R), slot = pid - pmin:
//   ci_count    per slot: #gallery rows, gmask, qmask                                        (integer atomics)
//   ci_scan     csr = exclusive scan of the counts (int64)
//   ci_scatter  gallery rows grouped by slot, in the order the atomics give
//   ci_rank     every row to its place in ascending gallery index inside its group (rank by counting): the list order is
//               the order creid_gather_mean_rows sums in, so it decides the centroids' bits
//   ci_sizes    per slot: #centroids, #listed rows
//   ci_scan2    exclusive scans of both (int64) + the totals {n_cent, rows} -- the one read-back, which sizes the outputs
//   ci_fill     order / offsets / labels / masks, one wave per slot, ordered ballot compaction per centroid
// Only integer atomics whose result does not depend on their order: two runs give the same arrays.
#include "common.hpp"

namespace {

constexpr int CI_T = 256;

__global__ __launch_bounds__(CI_T) void ci_count_kernel(const int64_t* __restrict__ pids, const int64_t* __restrict__ cams,
                                                        int nq, int ng, int64_t pmin, int R, int32_t* __restrict__ count,
                                                        unsigned long long* __restrict__ gmask,
                                                        unsigned long long* __restrict__ qmask) {
  const int top = nq > ng ? nq : ng;
  for (int i = blockIdx.x * CI_T + threadIdx.x; i < top; i += gridDim.x * CI_T) {
    const unsigned long long bit = 1ull << (cams[i] & 63);      // (the caller checked 0..62 for every index below max(nq, ng))
    if (i < ng) {
      const int64_t s = pids[(int64_t)nq + i] - pmin;
      if (s >= 0 && s < R) { atomicAdd(&count[s], 1); atomicOr(&gmask[s], bit); }
    }
    if (i < nq) {
      const int64_t s = pids[i] - pmin;
      if (s >= 0 && s < R) atomicOr(&qmask[s], bit);
    }
  }
}

// one workgroup of 1024: out[0 .. R] = exclusive scan of in[0 .. R) (int64 sums); may run in place when IN is long long
template <typename IN>
__device__ __forceinline__ long long ci_block_scan(const IN* in, int R, long long* out, long long* wsum, long long* carry_s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) *carry_s = 0;
  __syncthreads();
  for (int base = 0; base < R; base += 1024) {
    const int i = base + tid;
    const long long v = i < R ? (long long)in[i] : 0;
    long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    long long off = *carry_s;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (i < R) out[i] = off + x - v;
    __syncthreads();
    if (tid == 1023) *carry_s = off + x;
    __syncthreads();
  }
  const long long total = *carry_s;
  if (tid == 0) out[R] = total;
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(1024) void ci_scan_kernel(const int32_t* __restrict__ count, int R, long long* __restrict__ csr,
                                                       int32_t* __restrict__ cursor) {
  __shared__ long long wsum[16];
  __shared__ long long carry_s;
  for (int i = threadIdx.x; i < R; i += 1024) cursor[i] = 0;
  ci_block_scan(count, R, csr, wsum, &carry_s);
}

__global__ __launch_bounds__(CI_T) void ci_scatter_kernel(const int64_t* __restrict__ pids, int nq, int ng, int64_t pmin, int R,
                                                          const long long* __restrict__ csr, int32_t* __restrict__ cursor,
                                                          int32_t* __restrict__ g_tmp) {
  for (int i = blockIdx.x * CI_T + threadIdx.x; i < ng; i += gridDim.x * CI_T) {
    const int64_t s = pids[(int64_t)nq + i] - pmin;
    if (s >= 0 && s < R) {
      const long long at = csr[s] + atomicAdd(&cursor[s], 1);
      if (at < ng) g_tmp[at] = i;
    }
  }
}

// gallery row i goes to csr[slot] + #(rows of its group with a smaller index): ascending gallery index inside every group
__global__ __launch_bounds__(CI_T) void ci_rank_kernel(const int64_t* __restrict__ pids, int nq, int ng, int64_t pmin, int R,
                                                       const long long* __restrict__ csr, const int32_t* __restrict__ g_tmp,
                                                       int32_t* __restrict__ g_order) {
  for (int i = blockIdx.x * CI_T + threadIdx.x; i < ng; i += gridDim.x * CI_T) {
    const int64_t s = pids[(int64_t)nq + i] - pmin;
    if (s < 0 || s >= R) continue;
    const long long c0 = csr[s], c1 = csr[s + 1];
    long long r = 0;
    for (long long e = c0; e < c1; ++e) r += g_tmp[e] < i ? 1 : 0;
    if (c0 + r < ng) g_order[c0 + r] = i;
  }
}

// Walks the centroids of one slot in the reference's order; f(cur, used, all): cur = the query camera, used = the centroid's
// camera set, all = it lists every row of the pid (cur is not a gallery camera)
template <typename F>
__device__ __forceinline__ void ci_for_each_centroid(unsigned long long gm, unsigned long long qm, F f) {
  bool collapsed = false;
  for (unsigned long long rest = qm; rest; rest &= rest - 1) {
    const int cur = __ffsll((long long)rest) - 1;
    const unsigned long long bit = 1ull << cur;
    if (gm & bit) {
      const unsigned long long used = gm & ~bit;
      if (used) f(cur, used, false);
    } else if (!collapsed) {
      collapsed = true;
      f(cur, gm, true);
    }
  }
}

// one wave per slot (grid-stride): n_cent[s], n_rows[s] written into the arrays the second scan turns into offsets
__global__ __launch_bounds__(CI_T) void ci_sizes_kernel(const int64_t* __restrict__ cams, int R, const long long* __restrict__ csr,
                                                        const int32_t* __restrict__ g_order,
                                                        const unsigned long long* __restrict__ gmask,
                                                        const unsigned long long* __restrict__ qmask,
                                                        long long* __restrict__ cent_off, long long* __restrict__ rows_off) {
  const int lane = threadIdx.x & 63;
  const int wave0 = blockIdx.x * (CI_T / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (CI_T / 64);
  for (int s = wave0; s < R; s += nwaves) {                     // (wave-uniform)
    const long long c0 = csr[s], c1 = csr[s + 1];
    const unsigned long long gm = gmask[s], qm = qmask[s];
    long long ncent = 0, nrows = 0;
    if (c1 > c0 && qm) {
      ci_for_each_centroid(gm, qm, [&](int cur, unsigned long long, bool all) {
        int kept = 0;
        if (all) kept = lane == 0 ? (int)(c1 - c0) : 0;
        else
          for (long long e = c0 + lane; e < c1; e += 64) kept += cams[g_order[e]] != cur ? 1 : 0;
        nrows += kept;
        ++ncent;
      });
      long long t = nrows;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
      nrows = t;
    }
    if (lane == 0) { cent_off[s] = ncent; rows_off[s] = nrows; }
  }
}

// two workgroups: exclusive scan (in place) of the per-slot centroid counts / row counts; totals[0] = n_cent, totals[1] = rows
__global__ __launch_bounds__(1024) void ci_scan2_kernel(int R, long long* __restrict__ cent_off, long long* __restrict__ rows_off,
                                                        long long* __restrict__ totals) {
  __shared__ long long wsum[16];
  __shared__ long long carry_s;
  long long* a = blockIdx.x == 0 ? cent_off : rows_off;
  const long long t = ci_block_scan(a, R, a, wsum, &carry_s);
  if (threadIdx.x == 0) totals[blockIdx.x] = t;
}

// one wave per slot: its centroids' headers and member lists (full-vector row numbers = gallery index + nq), members in the
// group's order (ascending gallery index), compacted with a ballot per 64 rows
__global__ __launch_bounds__(CI_T) void ci_fill_kernel(const int64_t* __restrict__ cams, int nq, int64_t pmin, int R,
                                                       const long long* __restrict__ csr, const int32_t* __restrict__ g_order,
                                                       const unsigned long long* __restrict__ gmask,
                                                       const unsigned long long* __restrict__ qmask,
                                                       const long long* __restrict__ cent_off,
                                                       const long long* __restrict__ rows_off, long long n_cent, long long rows,
                                                       int64_t* __restrict__ order, int64_t* __restrict__ offsets,
                                                       int64_t* __restrict__ cent_labels, int64_t* __restrict__ cent_masks) {
  const int lane = threadIdx.x & 63;
  const int wave0 = blockIdx.x * (CI_T / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (CI_T / 64);
  if (wave0 == 0 && lane == 0) offsets[n_cent] = rows;
  for (int s = wave0; s < R; s += nwaves) {                     // (wave-uniform)
    long long k = cent_off[s];
    if (cent_off[s + 1] == k) continue;
    const long long c0 = csr[s], c1 = csr[s + 1];
    long long o = rows_off[s];
    ci_for_each_centroid(gmask[s], qmask[s], [&](int cur, unsigned long long used, bool all) {
      if (lane == 0 && k < n_cent) { offsets[k] = o; cent_labels[k] = pmin + s; cent_masks[k] = (int64_t)used; }
      ++k;
      for (long long b = c0; b < c1; b += 64) {
        const long long e = b + lane;
        int gi = -1;
        if (e < c1) { gi = g_order[e]; if (!all && cams[gi] == cur) gi = -1; }
        const unsigned long long bal = __ballot(gi >= 0);
        const long long at = o + __popcll(bal & lanemask_lt());
        if (gi >= 0 && at < rows) order[at] = (int64_t)gi + nq;
        o += __popcll(bal);
      }
    });
  }
}

// workspace: [csr | cent_off | rows_off] int64 (R + 1 each), totals int64[2], gmask / qmask uint64 [R], count / cursor int32 [R],
// g_tmp / g_order int32 [ng]
struct CiWs {
  long long *csr, *cent_off, *rows_off, *totals;
  unsigned long long *gmask, *qmask;
  int32_t *count, *cursor, *g_tmp, *g_order;
};
inline CiWs ci_ws(void* ws, int64_t ng, int64_t R) {
  CiWs w;
  long long* p = static_cast<long long*>(ws);
  w.csr = p; p += R + 1;
  w.cent_off = p; p += R + 1;
  w.rows_off = p; p += R + 1;
  w.totals = p; p += 2;
  w.gmask = reinterpret_cast<unsigned long long*>(p); p += R;
  w.qmask = reinterpret_cast<unsigned long long*>(p); p += R;
  int32_t* q = reinterpret_cast<int32_t*>(p);
  w.count = q; q += R;
  w.cursor = q; q += R;
  w.g_tmp = q; q += ng;
  w.g_order = q;
  return w;
}
inline unsigned ci_grid(int64_t items, int per_block) {
  const int64_t b = (items + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

}  // namespace

extern "C" {

size_t creid_centroid_index_ws_bytes(int64_t num_gallery, int64_t R) {
  if (num_gallery <= 0 || R <= 0) return 0;
  return (size_t)(3 * (R + 1) + 2 + 2 * R) * 8 + (size_t)(2 * R + 2 * num_gallery) * 4;
}

int creid_centroid_index_plan(const int64_t* labels, int64_t num_query, int64_t num_gallery, int64_t pmin, int64_t R, void* ws,
                              int64_t* totals, void* stream) {
  CREID_CHECK_ARG(labels && ws && totals && num_query >= 0 && num_gallery > 0 && R > 0);
  if (num_query + num_gallery > 0x7ffffff0LL || R > (1LL << 26)) return CREID_E_SHAPE;
  const int nq = (int)num_query, ng = (int)num_gallery;
  const int64_t* pids = labels;
  const int64_t* cams = labels + (num_query + num_gallery);
  hipStream_t s = as_stream(stream);
  const CiWs w = ci_ws(ws, num_gallery, R);
  // gmask | qmask | count are adjacent: one clear
  hipError_t e = hipMemsetAsync(w.gmask, 0, (size_t)R * (8 + 8 + 4), s);
  if (e != hipSuccess) return (int)e;
  const unsigned gb = ci_grid(nq > ng ? nq : ng, CI_T), gg = ci_grid(ng, CI_T), gs = ci_grid(R, CI_T / 64);
  hipLaunchKernelGGL(ci_count_kernel, dim3(gb), dim3(CI_T), 0, s, pids, cams, nq, ng, pmin, (int)R, w.count, w.gmask, w.qmask);
  hipLaunchKernelGGL(ci_scan_kernel, dim3(1), dim3(1024), 0, s, w.count, (int)R, w.csr, w.cursor);
  hipLaunchKernelGGL(ci_scatter_kernel, dim3(gg), dim3(CI_T), 0, s, pids, nq, ng, pmin, (int)R, w.csr, w.cursor, w.g_tmp);
  hipLaunchKernelGGL(ci_rank_kernel, dim3(gg), dim3(CI_T), 0, s, pids, nq, ng, pmin, (int)R, w.csr, w.g_tmp, w.g_order);
  hipLaunchKernelGGL(ci_sizes_kernel, dim3(gs), dim3(CI_T), 0, s, cams, (int)R, w.csr, w.g_order, w.gmask, w.qmask, w.cent_off,
                     w.rows_off);
  hipLaunchKernelGGL(ci_scan2_kernel, dim3(2), dim3(1024), 0, s, (int)R, w.cent_off, w.rows_off, w.totals);
  e = hipMemcpyAsync(totals, w.totals, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return (int)e;
  CREID_LAUNCH_RET();
}

int creid_centroid_index_fill(const int64_t* labels, int64_t num_query, int64_t num_gallery, int64_t pmin, int64_t R,
                              const void* ws, int64_t n_cent, int64_t rows, int64_t* order, int64_t* offsets,
                              int64_t* cent_labels, int64_t* cent_masks, void* stream) {
  CREID_CHECK_ARG(labels && ws && offsets && num_query >= 0 && num_gallery > 0 && R > 0 && n_cent >= 0 && rows >= 0);
  CREID_CHECK_ARG((order || rows == 0) && ((cent_labels && cent_masks) || n_cent == 0));
  if (num_query + num_gallery > 0x7ffffff0LL || R > (1LL << 26)) return CREID_E_SHAPE;
  const int64_t* cams = labels + (num_query + num_gallery);
  const CiWs w = ci_ws(const_cast<void*>(ws), num_gallery, R);
  hipLaunchKernelGGL(ci_fill_kernel, dim3(ci_grid(R, CI_T / 64)), dim3(CI_T), 0, as_stream(stream), cams, (int)num_query, pmin,
                     (int)R, w.csr, w.g_order, w.gmask, w.qmask, w.cent_off, w.rows_off, (long long)n_cent, (long long)rows, order,
                     offsets, cent_labels, cent_masks);
  CREID_LAUNCH_RET();
}

}  // extern "C"
