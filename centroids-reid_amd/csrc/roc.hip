// Open-set operating points (TAR @ FAR): what sits beside the histogram epilogue of the streamed contractions (EPI_HIST in
// stream_consume.hpp).  The impostor key of a given rank is found by a radix select over the 32-bit order-preserving keys of the
// distances: a pass counts, per class, the keys that share a prefix by their next digit; the select step walks the impostor
// counts to the digit that holds the rank, and the digit extends the prefix.  Three passes (11 + 11 + 10 bits) give the key
// exactly, with the numbers of impostor and genuine keys strictly below it, and nothing of size m x n is ever sorted.
//   dist_hist_matrix_kernel   a pass over an EXISTING fp32 distance matrix (the materialised routes; the cross-check of EPI_HIST)
//   roc_descend_kernel        the select step, one workgroup per target rate
#include "stream_consume.hpp"

// One workgroup per (row, 256 columns) in a grid-stride loop; the table [nsel][2][2^bits] lives in dynamic LDS for the whole
// kernel and leaves once, with 64-bit integer atomics.  Class and bin of an element: EPI_HIST's, word for word.
__global__ __launch_bounds__(256) void dist_hist_matrix_kernel(const float* __restrict__ dist, int m, int n,
                                                               const int64_t* __restrict__ q_pids, const int64_t* __restrict__ g_pids,
                                                               const int64_t* __restrict__ q_cams, const int64_t* __restrict__ g_cams,
                                                               int camsets, const unsigned* __restrict__ prefix, int nsel, int pb,
                                                               int bits, unsigned long long* __restrict__ hist_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned tab[];     // [nsel][2][2^bits]
  const int tid = threadIdx.x, lane = tid & 63;
  const int words = (2 * nsel) << bits;
  for (int i = tid; i < words; i += 256) tab[i] = 0u;
  __syncthreads();
  const int dshift = 32 - pb - bits;
  const unsigned dmask = (1u << bits) - 1u;
  const long long chunks = (n + 255) / 256, total = (long long)m * chunks;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const int row = (int)(w / chunks), col = (int)(w - (long long)row * chunks) * 256 + tid;
    const long long qp = q_pids[row], qc = q_cams[row];
    bool live = col < n;
    unsigned key = 0u, cls = 1u;
    if (live) {
      key = mono_key(dist[(int64_t)row * n + col]);
      if ((long long)g_pids[col] == qp) {
        cls = 0u;
        const int64_t gc = g_cams[col];
        if (camsets ? cam_removed<true>(gc, qc) : cam_removed<false>(gc, qc)) live = false;
      }
    }
    const unsigned pfx = (unsigned)((unsigned long long)key >> (32 - pb));
    const unsigned bin = (key >> dshift) & dmask;
    for (int s = 0; s < nsel; ++s) {
      const unsigned want = pb ? prefix[s] : 0u;
      wave_hist_add(tab, live && pfx == want, ((2u * s + cls) << bits) | bin, lane, pb != 0);
    }
  }
  __syncthreads();
  for (int i = tid; i < words; i += 256) {
    const unsigned v = tab[i];
    if (v) atomicAdd(&hist_out[i], (unsigned long long)v);
  }
}

// state int64 [T][8] per target: the rank still to walk inside the current prefix, the prefix, the impostor and genuine keys
// known to lie below it, the class totals, the lowest key of the prefix (after the last pass: THE key), flags.
enum { RS_K = 0, RS_PREFIX, RS_FA, RS_TA, RS_NIMP, RS_NGEN, RS_KEY, RS_FLAGS };
constexpr long long RF_NO_IMPOSTOR = 1, RF_INCONSISTENT = 2;         // flags bits 0 / 1; bits 8..15: the key bits fixed so far

__global__ __launch_bounds__(256) void roc_descend_kernel(const unsigned long long* __restrict__ hist, int bits, int level,
                                                          const double* __restrict__ far, long long* __restrict__ state,
                                                          unsigned* __restrict__ prefix_out) {
  __shared__ unsigned long long s_imp[256], s_gen[256];
  __shared__ long long s_k, s_flags;                                 // the state as thread 0 found it: one thread rewrites it below
  const int t = blockIdx.x, tid = threadIdx.x, nb = 1 << bits;
  const unsigned long long* gen = hist + ((size_t)(level == 0 ? 0 : t) * 2) * nb;      // the first pass has ONE selector
  const unsigned long long* imp = gen + nb;
  long long* st = state + (size_t)t * 8;
  const int per = (nb + 255) / 256, b0 = tid * per, b1 = min(nb, b0 + per);
  unsigned long long ti = 0, tg = 0;
  for (int b = b0; b < b1; ++b) { ti += imp[b]; tg += gen[b]; }
  s_imp[tid] = ti; s_gen[tid] = tg;
  __syncthreads();
  if (tid == 0) {                                                    // exclusive scans of the 256 partial sums (in place)
    unsigned long long ai = 0, ag = 0;
    for (int i = 0; i < 256; ++i) {
      const unsigned long long vi = s_imp[i], vg = s_gen[i];
      s_imp[i] = ai; s_gen[i] = ag;
      ai += vi; ag += vg;
    }
    if (level == 0) {
      long long k = 0, flags = 0;
      if (ai == 0) flags = RF_NO_IMPOSTOR;
      else {
        k = (long long)floor(far[t] * (double)ai);                   // the one floating-point product
        if (k > (long long)ai - 1) k = (long long)ai - 1;
        if (k < 0) k = 0;
      }
      st[RS_K] = k; st[RS_PREFIX] = 0; st[RS_FA] = 0; st[RS_TA] = 0;
      st[RS_NIMP] = (long long)ai; st[RS_NGEN] = (long long)ag; st[RS_KEY] = 0; st[RS_FLAGS] = flags;
    }
    if (!(st[RS_FLAGS] & (RF_NO_IMPOSTOR | RF_INCONSISTENT)) && (unsigned long long)st[RS_K] >= ai)
      st[RS_FLAGS] |= RF_INCONSISTENT;                               // the counts do not hold the rank: not this state's pass
    if (st[RS_FLAGS] & (RF_NO_IMPOSTOR | RF_INCONSISTENT)) prefix_out[t] = 0u;
    s_k = st[RS_K]; s_flags = st[RS_FLAGS];
  }
  __syncthreads();                                                   // (block-wide: thread 0's state writes are visible below)
  const long long flags = s_flags;
  if (flags & (RF_NO_IMPOSTOR | RF_INCONSISTENT)) return;
  const unsigned long long k = (unsigned long long)s_k;
  unsigned long long ci = s_imp[tid], cg = s_gen[tid];
  if (!(ci <= k && k < ci + ti)) return;                             // exactly one thread's bins hold the rank
  int d = b0;
  for (; d + 1 < b1; ++d) {                                          // (the last bin is the answer when no earlier one is)
    const unsigned long long v = imp[d];
    if (k < ci + v) break;
    ci += v; cg += gen[d];
  }
  long long done = ((flags >> 8) & 0xff) + bits;
  if (done > 32) done = 32;                                          // (more passes than the key has bits: the caller's error)
  const unsigned long long p = ((unsigned long long)st[RS_PREFIX] << bits) | (unsigned)d;
  st[RS_K] = (long long)(k - ci);
  st[RS_PREFIX] = (long long)p;
  st[RS_FA] += (long long)ci;
  st[RS_TA] += (long long)cg;
  st[RS_KEY] = (long long)((p << (32 - done)) & 0xffffffffull);
  st[RS_FLAGS] = (flags & 0xff) | (done << 8);
  prefix_out[t] = (unsigned)p;
}

extern "C" {

int creid_dist_hist_matrix(const float* dist, int64_t m, int64_t n, const int64_t* q_pids, const int64_t* g_pids,
                           const int64_t* q_cams, const int64_t* g_cams, int32_t camsets, const uint32_t* prefix, int32_t nsel,
                           int32_t prefix_bits, int32_t bits, uint64_t* hist, void* stream) {
  CREID_CHECK_ARG(m >= 0 && n > 0);
  if (!stream_hist_ok(nsel, prefix_bits, bits) || !stream_mn_ok(m, n)) return CREID_E_SHAPE;
  if (m == 0) return 0;
  CREID_CHECK_ARG(dist && q_pids && g_pids && q_cams && g_cams && hist && (prefix || prefix_bits == 0));
  static const hipError_t attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(dist_hist_matrix_kernel),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, 2 * HS_MAX_BINS * (int)sizeof(unsigned));
  if (attr_rc != hipSuccess) return (int)attr_rc;
  const long long work = m * ((n + 255) / 256);
  const unsigned grid = (unsigned)(work < 2048 ? work : 2048);
  hipLaunchKernelGGL(dist_hist_matrix_kernel, dim3(grid), dim3(256), (size_t)((2 * nsel) << bits) * sizeof(unsigned), as_stream(stream),
                     dist, (int)m, (int)n, q_pids, g_pids, q_cams, g_cams, camsets != 0 ? 1 : 0, prefix, (int)nsel, (int)prefix_bits,
                     (int)bits, reinterpret_cast<unsigned long long*>(hist));
  CREID_LAUNCH_RET();
}

int creid_roc_descend(const uint64_t* hist, int32_t nsel, int32_t bits, int32_t level, const double* far, int64_t* state,
                      uint32_t* prefix, void* stream) {
  if (bits < 1 || bits > HS_MAX_BITS || nsel < 1 || nsel > (HS_MAX_BINS >> bits) || level < 0 || level > 31) return CREID_E_SHAPE;
  CREID_CHECK_ARG(hist && far && state && prefix);
  hipLaunchKernelGGL(roc_descend_kernel, dim3((unsigned)nsel), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long*>(hist), (int)bits, (int)level, far,
                     reinterpret_cast<long long*>(state), prefix);
  CREID_LAUNCH_RET();
}

}  // extern "C"
