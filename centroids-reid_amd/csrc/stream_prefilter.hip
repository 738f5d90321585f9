// Exact fp32 top-k retrieval with the contraction on the 16-bit MFMA (reid_metric.topk_stream(prefilter=...)): the streamed
// 16-bit contraction of stream_h16.hip only decides which few (query, gallery) pairs can be in the answer, with a proven margin;
// those few are re-scored with the fp32 kernels' own arithmetic.  The result has the indices and the distance bits of the fp32
// creid_stream_topk_collect + creid_stream_topk_select, i.e. of creid_sqdist_matrix + creid_topk_rows.
//
// Per query i and gallery row j: d the fp32 kernels' distance, dh the 16-bit streamed kernel's distance on the rows rounded once
// to bf16 / f16 WITH THE FP32 ROWS' OWN NORMS (so only the dot product differs), m_i >= |dh - d| for every j.  With dh_(k) the
// k-th smallest dh of the row: the k pairs of smallest dh have d <= dh_(k) + m_i, so the true k-th distance d_(k) <= dh_(k) + m_i;
// every pair of the true top-k, ties at d_(k) included, has d <= d_(k), hence dh <= dh_(k) + 2 m_i.  The pairs within that cut
// are a superset of the answer; re-scored and sorted by (d, j) they give exactly the fp32 result.
//
//   prefilter_pack_kernel<T>      fp32 rows -> the bf16 / f16 copy (round to nearest even) and per row |x - xh|^2, |xh|^2, |x|^2 in
//                                 double: what the margin m_i is computed from (reid_metric.prefilter_margin).
//   (creid_stream_topk_collect_h16, unchanged, collects every dh <= tau_i + 2 m_i, tau_i >= dh_(k) from a gallery sample.)
//   stream_topk_rescore_kernel    per query: sorts the list by dh, keeps the prefix within dh_(k) + 2 m_i, replaces each kept key
//                                 with the fp32 distance (STREAM_FMAF_CHAIN + the sqdist epilogue) and sorts again.
//
// The exact fp32 evaluation (reid_metric.R1_mAP(streamed=True, prefilter=...)) is built the same way: the banded count of
// stream_h16.hip (EPI_BAND, stream_consume.hpp) places every negative whose 16-bit distance, widened by m_i on both sides, falls
// between two positives' fp32 keys, and lists the others;
//   stream_count_rescore_kernel   per query: each listed pair receives the fp32 distance and goes through the fp32 count
//                                 epilogue's own search.  The histogram is then creid_stream_count's, element for element.
#include "stream_chain.hpp"
#include "stream_common.hpp"
#include "topk_tail.hpp"

namespace {
constexpr int RS_T = 1024;                       // threads of a re-score workgroup: one fmaf chain each
constexpr int RS_CAP = RS_T;                     // entries a row may keep (reid_metric.STREAM_RESCORE_CAPACITY)
constexpr int64_t PF_MAX_D = 1 << 20;            // as the 16-bit streamed kernels
constexpr int CR_T = 256;                        // threads of a count re-score workgroup
}  // namespace

// ----------------------------------------------------------------------------------------
// 1. pack.  One wave per row, four rows per workgroup; a lane converts 8 consecutive elements per pass (two 16-byte loads, one
//    16-byte store: D % 8 == 0).  x - xh is exact in fp32 (xh is x rounded to fewer bits, or 0 / a 16-bit subnormal), its square
//    and the squares of x and xh are exact in double; the sums are double: D + 6 roundings of 2^-53 each, relative.
//    A row with an Inf / NaN element, or one that overflows f16, gets non-finite statistics: the caller deals with it.
// ----------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void prefilter_pack_kernel(const float* __restrict__ x, int64_t rows, int D,
                                                             unsigned short* __restrict__ y, double* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* __restrict__ xr = x + row * D;
  unsigned short* __restrict__ yr = y + row * D;
  double e2 = 0.0, h2 = 0.0, x2 = 0.0;
  auto acc = [&](float v, float vh) {
    const double d = (double)(v - vh), a = (double)v, b = (double)vh;
    e2 = fma(d, d, e2); h2 = fma(b, b, h2); x2 = fma(a, a, x2);
  };
  for (int k = lane * 8; k < D; k += 512) {
    const float4 a = *reinterpret_cast<const float4*>(xr + k), b = *reinterpret_cast<const float4*>(xr + k + 4);
    const uint4 w = make_uint4(T::pack2(a.x, a.y), T::pack2(a.z, a.w), T::pack2(b.x, b.y), T::pack2(b.z, b.w));
    *reinterpret_cast<uint4*>(yr + k) = w;
    acc(a.x, T::lo(w.x)); acc(a.y, T::hi(w.x)); acc(a.z, T::lo(w.y)); acc(a.w, T::hi(w.y));
    acc(b.x, T::lo(w.z)); acc(b.y, T::hi(w.z)); acc(b.z, T::lo(w.w)); acc(b.w, T::hi(w.w));
  }
  e2 = wave_sum_d(e2); h2 = wave_sum_d(h2); x2 = wave_sum_d(x2);
  if (lane == 0) { stats[row * 3 + 0] = e2; stats[row * 3 + 1] = h2; stats[row * 3 + 2] = x2; }
}

// ----------------------------------------------------------------------------------------
// 2. re-score.  One workgroup per query; the list (count <= cap words of key(dh) << 32 | column) goes to LDS and is sorted, so
//    dh_(k) is entry k - 1 and the kept entries are a prefix: those with key <= key(cut), cut = add_up(dh_(k), margin2[row]) --
//    margin2 >= 2 m_i comes rounded up from the caller, add_up never rounds below the real sum, so the cut is never below the
//    real one.  Thread t re-scores kept entry t with the fmaf chain of stream_poslist_kernel (the query row is wave-uniform:
//    scalar loads) and the sqdist epilogue; the shared sort tail writes the first k by (d, column).
//    Flagged, nothing written: the list overflowed or holds fewer than k entries (as stream_topk_select_kernel), the margin is not
//    a finite number >= 0, the cut is NaN, more than RS_CAP entries are kept, or a column lies outside the gallery.
//    No static LDS (and no barrier-with-vote, which takes some): at capacity 8192 the list alone is the 64 KiB a workgroup gets
//    by default.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_T) void stream_topk_rescore_kernel(
    const unsigned long long* __restrict__ cand, const int32_t* __restrict__ count, int cap, int k, const float* __restrict__ q,
    const float* __restrict__ g, const float* __restrict__ qq, const float* __restrict__ gg, int n, int D,
    const float* __restrict__ margin2, int64_t* __restrict__ out_idx, float* __restrict__ out_dist, uint8_t* __restrict__ flags,
    int32_t* __restrict__ kept) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_cand[];      // [cap]
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int c = count[row];                                                        // (everything up to the chains is uniform)
  const float mg = margin2[row];
  if (c > cap || c < k || !(mg >= 0.f && mg <= 3.402823466e+38f)) {
    if (tid == 0) { flags[row] = 1; kept[row] = 0; }
    return;
  }
  for (int i = tid; i < c; i += RS_T) s_cand[i] = cand[row * cap + i];
  __syncthreads();
  tk_sort<RS_T>(s_cand, c);
  const float cut = add_up(tk_unkey((unsigned)(s_cand[k - 1] >> 32)), mg);
  const unsigned kcut = mono_key(cut);
  int lo = k, hi = c;                              // entries [0, k) are within the cut; nk = the first index beyond it
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)(s_cand[mid] >> 32) <= kcut) lo = mid + 1; else hi = mid;
  }
  const int nk = lo;
  if (!(cut == cut) || nk > RS_CAP) {
    if (tid == 0) { flags[row] = 1; kept[row] = nk; }
    return;
  }
  __syncthreads();                                 // the search has read the list: now its entries are replaced
  const float* __restrict__ qrow = q + row * D;
  if (tid < nk) {
    const unsigned col = (unsigned)(s_cand[tid] & 0xffffffffull);
    unsigned long long e = ~0ull;                  // a column outside the gallery: no entry with a column < n has this value
    if (col < (unsigned)n) {
      const float* __restrict__ grow = g + (int64_t)col * D;
      STREAM_FMAF_CHAIN(acc, qrow, grow, D);
      e = ((unsigned long long)mono_key(fmaf(-2.0f, acc, qq[row] + gg[col])) << 32) | col;             // sqdist epilogue, same bits
    }
    s_cand[tid] = e;
  }
  __syncthreads();
  tk_sort<RS_T>(s_cand, nk);
  if (s_cand[nk - 1] == ~0ull) {                   // (sorted: such an entry is the last one)
    if (tid == 0) { flags[row] = 1; kept[row] = nk; }
    return;
  }
  tk_emit<RS_T>(s_cand, k, row, out_idx, out_dist);
  if (tid == 0) { flags[row] = 0; kept[row] = nk; }
}

// ----------------------------------------------------------------------------------------
// 3. count re-score.  One workgroup per query; the row's positive keys and gallery indices are staged once in LDS.  Thread t takes
//    listed pairs t, t + 256, ..: the fmaf chain and the sqdist epilogue give the fp32 key, then the fp32 count epilogue
//    (stream_tile_consume<EPI_COUNT>): nothing beyond the last positive's key, l = #positives with a smaller key by binary search
//    over the padded list, ties walked by gallery index, one integer atomic on hist[row][l].  (Same-pid columns never reach a
//    list: the banded count skips them.)
//    Flagged, nothing written: the list overflowed or names a column outside the gallery.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(CR_T) void stream_count_rescore_kernel(
    const unsigned* __restrict__ amb, const int32_t* __restrict__ amb_count, int acap, const float* __restrict__ q,
    const float* __restrict__ g, const float* __restrict__ qq, const float* __restrict__ gg, int n, int D, int cap,
    const unsigned* __restrict__ pos_key, const int32_t* __restrict__ pos_idx, const int32_t* __restrict__ npos,
    unsigned* __restrict__ hist, uint8_t* __restrict__ flags) {
  __shared__ unsigned s_key[PL_MAXC];
  __shared__ int s_idx[PL_MAXC];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int c = amb_count[row];                                                    // (uniform)
  const int np = min(max(npos[row], 0), cap);
  if (c > acap) { if (tid == 0) flags[row] = 1; return; }
  if (c <= 0 || np == 0) { if (tid == 0) flags[row] = 0; return; }
  const unsigned* __restrict__ list = amb + row * acap;
  if (tid == 0) s_bad = 0;
  for (int i = tid; i < cap; i += CR_T) { s_key[i] = pos_key[row * cap + i]; s_idx[i] = pos_idx[row * cap + i]; }
  __syncthreads();
  bool bad = false;
  for (int i = tid; i < c; i += CR_T) bad |= list[i] >= (unsigned)n;
  if (bad) s_bad = 1;
  __syncthreads();
  if (s_bad) { if (tid == 0) flags[row] = 1; return; }
  if (tid == 0) flags[row] = 0;
  const float* __restrict__ qrow = q + row * D;
  const unsigned kmax = s_key[np - 1];
  const float qv = qq[row];
  for (int i = tid; i < c; i += CR_T) {
    const int col = (int)list[i];
    const float* __restrict__ grow = g + (int64_t)col * D;
    STREAM_FMAF_CHAIN(acc, qrow, grow, D);
    const unsigned key = mono_key(fmaf(-2.0f, acc, qv + gg[col]));                 // sqdist epilogue, same bits
    if (key > kmax) continue;                                                      // behind every positive
    int l = 0;
    for (int step = cap >> 1; step > 0; step >>= 1) l += (s_key[l + step - 1] < key) ? step : 0;
    l += (s_key[l] < key) ? 1 : 0;
    while (l < np && s_key[l] == key && s_idx[l] < col) ++l;                       // ties: by gallery index
    if (l < np) atomicAdd(&hist[row * cap + l], 1u);
  }
}

extern "C" {

int creid_prefilter_pack(const float* x, int64_t rows, int64_t D, int dtype, void* y, double* stats, void* stream) {
  CREID_CHECK_ARG(rows >= 0 && D > 0);
  if (D % 8 != 0 || D > PF_MAX_D || rows > 0x7ffffff0LL) return CREID_E_SHAPE;
  if (!creid_is16(dtype)) return CREID_E_DTYPE;
  if (rows == 0) return 0;
  CREID_CHECK_ARG(x && y && stats);
  const dim3 grid((unsigned)((rows + 3) / 4));
  unsigned short* yh = static_cast<unsigned short*>(y);
  if (dtype == CREID_BF16)
    hipLaunchKernelGGL(prefilter_pack_kernel<Bf16T>, grid, dim3(256), 0, as_stream(stream), x, rows, (int)D, yh, stats);
  else
    hipLaunchKernelGGL(prefilter_pack_kernel<F16T>, grid, dim3(256), 0, as_stream(stream), x, rows, (int)D, yh, stats);
  CREID_LAUNCH_RET();
}

int creid_stream_topk_rescore(const uint64_t* cand, const int32_t* count, int64_t m, int32_t cap, int32_t k, const float* q,
                              const float* g, const float* qq, const float* gg, int64_t n, int64_t D, const float* margin2,
                              int64_t* out_idx, float* out_dist, uint8_t* flags, int32_t* kept, void* stream) {
  CREID_CHECK_ARG(m >= 0 && n > 0 && D > 0 && k >= 1);
  if (!stream_topk_cap_ok(cap) || k > 1024 || k > cap || D % 4 != 0 || D > PF_MAX_D) return CREID_E_SHAPE;
  if (!stream_mn_ok(m, n)) return CREID_E_SHAPE;
  if (m == 0) return 0;
  CREID_CHECK_ARG(cand && count && q && g && qq && gg && margin2 && out_idx && flags && kept);
  hipLaunchKernelGGL(stream_topk_rescore_kernel, dim3((unsigned)m), dim3(RS_T), (size_t)cap * sizeof(unsigned long long),
                     as_stream(stream), reinterpret_cast<const unsigned long long*>(cand), count, (int)cap, (int)k, q, g, qq, gg,
                     (int)n, (int)D, margin2, out_idx, out_dist, flags, kept);
  CREID_LAUNCH_RET();
}

int creid_stream_count_rescore(const uint32_t* amb, const int32_t* amb_count, int64_t m, int32_t amb_cap, const float* q,
                               const float* g, const float* qq, const float* gg, int64_t n, int64_t D, int32_t cap,
                               const uint32_t* pos_key, const int32_t* pos_idx, const int32_t* npos, uint32_t* hist,
                               uint8_t* flags, void* stream) {
  CREID_CHECK_ARG(m >= 0 && n > 0 && D > 0);
  if (!stream_topk_cap_ok(amb_cap) || !stream_count_cap_ok(cap) || D % 4 != 0 || D > PF_MAX_D) return CREID_E_SHAPE;
  if (!stream_mn_ok(m, n)) return CREID_E_SHAPE;
  if (m == 0) return 0;
  CREID_CHECK_ARG(amb && amb_count && q && g && qq && gg && pos_key && pos_idx && npos && hist && flags);
  hipLaunchKernelGGL(stream_count_rescore_kernel, dim3((unsigned)m), dim3(CR_T), 0, as_stream(stream), amb, amb_count, (int)amb_cap,
                     q, g, qq, gg, (int)n, (int)D, (int)cap, pos_key, pos_idx, npos, hist, flags);
  CREID_LAUNCH_RET();
}

}  // extern "C"
