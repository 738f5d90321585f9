// What the two streamed contractions (stream_eval.hip: fp32 features on the f32 MFMA; stream_h16.hip: bf16 / f16 features on the
// 16-bit MFMA) share on both sides of a launch: the tile geometry the work split is expressed in, the epilogue selector, the list
// capacities and the argument tests of the entry points, the order-preserving key of a distance, the work split (stream_split)
// and a workgroup's share of it (stream_run).  What the kernels do with a finished tile is in stream_consume.hpp.
#pragma once
#include "common.hpp"
#include <stdlib.h>
#include <type_traits>

constexpr int SQ_TM = 64, SQ_TN = 256;           // a tile: 64 query rows x 256 gallery columns (four units of 64 columns)
constexpr int EPI_COUNT = 0, EPI_TOPK = 1;       // what a streamed contraction does with a finished tile
constexpr int EPI_BAND = 2;                      // the count with a per-row error band (16-bit kernel only: stream_consume.hpp)
constexpr int EPI_TOPK_KEEP = 3;                 // the top-k that lists only the entries the evaluation protocol keeps (no junk)
constexpr int EPI_HIST = 4;                      // the radix histogram of the non-junk distance keys, by class (open-set ROC)
constexpr bool epi_is_topk(int epi) { return epi == EPI_TOPK || epi == EPI_TOPK_KEEP; }
constexpr int PL_MAXC = 128;                     // positive-list capacity of the count epilogue (LDS: [64][cap] keys + histogram)
constexpr int TS_MIN_CAP = 64, TS_MAX_CAP = 8192;   // candidate-list capacity of the top-k epilogue
constexpr int HS_MAX_BITS = 11, HS_MAX_BINS = 8192; // histogram epilogue: digit width, and nsel << bits (the LDS table
                                                    // [nsel][2][2^bits] words fits the count's 64 KiB of dynamic LDS)

// Argument tests of the entry points.  A list capacity is a power of two inside its epilogue's range (the kernels index with
// shifts and masks: stream_log2cap); m and n leave room for the 32-bit tile arithmetic.
static bool stream_cap_ok(int64_t cap, int lo, int hi) { return cap >= lo && cap <= hi && (cap & (cap - 1)) == 0; }
static bool stream_count_cap_ok(int64_t cap) { return stream_cap_ok(cap, 2, PL_MAXC); }
static bool stream_topk_cap_ok(int64_t cap) { return stream_cap_ok(cap, TS_MIN_CAP, TS_MAX_CAP); }
static bool stream_mn_ok(int64_t m, int64_t n) { return m <= 0x7ffffff0LL && n <= 0x7ffffff0LL; }
// A radix pass: nsel selectors of prefix_bits leading key bits each, a digit of `bits` bits behind them.  Without a prefix there
// is nothing to tell selectors apart, so there is one.
static bool stream_hist_ok(int64_t nsel, int64_t prefix_bits, int64_t bits) {
  return bits >= 1 && bits <= HS_MAX_BITS && prefix_bits >= 0 && prefix_bits + bits <= 32 && nsel >= 1 &&
         nsel <= (HS_MAX_BINS >> bits) && (prefix_bits != 0 || nsel == 1);
}
static int stream_log2cap(int cap) {
  int l = 0;
  while ((1 << l) < cap) ++l;
  return l;
}

// float -> unsigned with the same order (negatives included; squared distances may be slightly negative)
__device__ __forceinline__ unsigned mono_key(float d) {
  const unsigned u = __float_as_uint(d);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// Is a same-pid gallery entry removed for a query on camera qc (utils/eval_reid.py:51-57)?  Plain: the entry's camera is qc.
// CAMSETS: the entry carries a bitmask of cameras (bit c = camera c) and is removed when qc (0..62, checked by the entry
// points' callers) is in it -- the test of creid_cmc_ap_ranked_camsets.
template <bool CAMSETS>
__device__ __forceinline__ bool cam_removed(int64_t g_cam, int64_t qc) {
  if constexpr (CAMSETS) return (((unsigned long long)g_cam >> (qc & 63)) & 1ull) != 0;
  else return g_cam == qc;
}

// a + b rounded towards +inf or beyond: never below the real sum (round to nearest, then one step up; a zero sum steps to the
// smallest positive number, past +0)
__device__ __forceinline__ float add_up(float a, float b) {
  const float s = a + b;
  if (!(fabsf(s) <= 3.402823466e+38f)) return s;  // inf / NaN stay
  const unsigned u = __float_as_uint(s);
  if ((u << 1) == 0u) return __uint_as_float(1u);
  return __uint_as_float((u >> 31) ? u - 1u : u + 1u);
}

// a - b rounded towards -inf or beyond: never above the real difference (the mirror of add_up; a zero difference steps to the
// smallest negative number, past -0, so that its key is below the key of either zero)
__device__ __forceinline__ float sub_down(float a, float b) {
  const float s = a - b;
  if (!(fabsf(s) <= 3.402823466e+38f)) return s;  // inf / NaN stay
  const unsigned u = __float_as_uint(s);
  if ((u << 1) == 0u) return __uint_as_float(0x80000001u);
  return __uint_as_float((u >> 31) ? u + 1u : u - 1u);
}

/* The work split of a streamed contraction (both kernels, both epilogues).  elem_bytes: the size of a feature element (the
 * gallery's footprint decides between the two modes). */
struct StreamSplit { int tiles_m, U, upw, mode; unsigned grid; };
static StreamSplit stream_split(int64_t m, int64_t n, int64_t D, int64_t elem_bytes = 4) {
  const int tiles_m = (int)((m + SQ_TM - 1) / SQ_TM), tiles_n = (int)((n + SQ_TN - 1) / SQ_TN);
  const int U = (int)((n + 63) / 64);                           // units of 64 gallery columns per row of query tiles
  // enough workgroups for two per CU, but never fewer than ~4 gallery tiles per workgroup (per-tile restart cost)
  static const int target = [] { const char* e = getenv("CREID_STREAM_WGS"); int v = e ? atoi(e) : 0; return v > 0 ? v : 512; }();
  // mode 0: never MORE than `tper_max` gallery tiles per workgroup: the grid overshoots the 512 slots by up to tiles_m - 1
  // workgroups, which start when the first ones finish -- harmless when a workgroup is 5 tiles long, a whole second round on an
  // idle chip when it is 131 (6250 x 200 000: 588 workgroups, 66.0 ms; with <= 8 tiles per workgroup 46.1 ms; HBM-side traffic by
  // the counters the same under both rules -- profiles/r05_stream_grid.md)
  static const int tper_max = [] { const char* e = getenv("CREID_STREAM_TPER"); int v = e ? atoi(e) : 0; return v > 0 ? v : 8; }();
  int nsplit = (target + tiles_m - 1) / tiles_m;
  if (nsplit < (tiles_n + tper_max - 1) / tper_max) nsplit = (tiles_n + tper_max - 1) / tper_max;
  if (nsplit > tiles_n) nsplit = tiles_n;
  if (nsplit < 1) nsplit = 1;
  const int t_per = (tiles_n + nsplit - 1) / nsplit;
  nsplit = (tiles_n + t_per - 1) / t_per;                       // drop empty slices
  // mode 1 (equal runs of units over the resident slots): only while the gallery fits the Infinity Cache beside the queries, the
  // grid of mode 0 is a single round, and the equal run is shorter than mode 0's longest workgroup by more than the narrow tile
  // and the second segment cost (~a quarter tile: 2228 x 17661 -- 4.75 tiles against 5 -- measured EQUAL in both modes,
  // 3000 x 15000 -- 5.5 against 6 -- 5.6 % faster in mode 1; profiles/r06_eval_kloop.md).  CREID_STREAM_BALANCE=0 / 1 forces a
  // mode (the tests run both).
  const long long T = (long long)tiles_m * U;
  const long long wg1 = T / 4 < target ? (T / 4 > 0 ? T / 4 : 1) : target;
  const char* bal_e = CREID_KNOB_ENV("CREID_STREAM_BALANCE");
  const int bal = (bal_e && *bal_e) ? atoi(bal_e) : -1;
  const double run1 = (double)((T + wg1 - 1) / wg1) / 4.0 + 0.3;
  const int mode = bal >= 0 ? (bal != 0)
                            : ((double)n * (double)D * (double)elem_bytes <= 192e6 && (long long)tiles_m * nsplit <= target &&
                               run1 < (double)t_per);
  const int upw = 4 * t_per;
  const unsigned grid = mode == 0 ? (unsigned)(tiles_m * nsplit) : (unsigned)wg1;
  return StreamSplit{tiles_m, U, upw, mode, grid};
}

/* Launch of a count contraction (Kernel: an instantiation of either file's kernel, 256 threads): its dynamic LDS is the query
 * tile's positive keys and histogram, [64][cap] words each -- beyond the default limit at capacity 128, so every instantiation
 * raises its own limit once.  EXTRA: words behind them (the banded count's row margins). */
template <auto Kernel, int EXTRA = 0, class... Args>
static int stream_count_launch(const StreamSplit& sp, int cap, void* stream, Args... args) {
  static const hipError_t attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        (2 * SQ_TM * PL_MAXC + EXTRA) * (int)sizeof(unsigned));
  if (attr_rc != hipSuccess) return (int)attr_rc;
  hipLaunchKernelGGL(Kernel, dim3(sp.grid), dim3(256), (size_t)(2 * SQ_TM * cap + EXTRA) * sizeof(unsigned), as_stream(stream), args...);
  return (int)hipGetLastError();
}

/* The arguments of a streamed contraction, in the groups its epilogues read.  An entry point fills the groups of its epilogue
 * and leaves the others empty ({}); stream_args_pass tests exactly the groups the epilogue uses, and the kernels receive the
 * empty ones as null pointers and zeros. */
struct StreamRows { const void *q, *g; const float *qq, *gg; int64_t m, n, D; };       // the operands and their square norms
struct StreamPids { const int64_t *q_pids = nullptr, *g_pids = nullptr; };             // EPI_COUNT, EPI_BAND, EPI_TOPK_KEEP
struct StreamPos {                                                                     // EPI_COUNT, EPI_BAND: the positive lists
  int32_t cap = 0;
  const uint32_t* key = nullptr;
  const int32_t *idx = nullptr, *npos = nullptr;
  uint32_t* hist = nullptr;
};
struct StreamList {       // EPI_TOPK[_KEEP]: thresholds and candidate lists; EPI_BAND: row margins and the lists of ambiguous pairs
  const float* thr = nullptr;
  unsigned long long* list = nullptr;
  int32_t* count = nullptr;
  int32_t cap = 0;
};
struct StreamCams { const int64_t *q_cams = nullptr, *g_cams = nullptr; int camsets = 0; };   // EPI_TOPK_KEEP, EPI_HIST
struct StreamHist {       // EPI_HIST: the pass's selectors (prefix may be null without prefix bits) and the counts it adds into
  const uint32_t* prefix = nullptr;
  int32_t nsel = 0, prefix_bits = 0, bits = 0;
  unsigned long long* out = nullptr;
};

/* The argument tests of every streamed contraction; false: return *rc (0: nothing to do).  d_mult / d_max: the widths the
 * kernel loads; dtype_ok: the 16-bit kernels' dtype test.  An empty query set is a no-op -- for the count epilogues whatever
 * the capacities and widths are, for the top-k epilogues once they have passed: the precedence each family of entry points
 * has always had (tests/test_stream_h16_cpu.py and the *_abi_argument_checks GPU tests pin both); the histogram epilogue follows
 * the top-k family (every refusal of a shape or dtype, then m == 0, then the pointers). */
template <int EPI>
static bool stream_args_pass(const StreamRows& x, const StreamPids& pids, const StreamPos& pos, const StreamList& list,
                             const StreamCams& cams, int64_t d_mult, int64_t d_max, bool dtype_ok, int* rc,
                             const StreamHist& hs = {}) {
  constexpr bool topk = epi_is_topk(EPI), hist = EPI == EPI_HIST;
  constexpr bool use_pids = EPI != EPI_TOPK, use_pos = !topk && !hist, use_list = EPI != EPI_COUNT && !hist;
  constexpr bool use_cams = EPI == EPI_TOPK_KEEP || hist;
  const bool ptrs = x.q && x.g && x.qq && x.gg && (!use_pids || (pids.q_pids && pids.g_pids)) &&
                    (!use_pos || (pos.key && pos.idx && pos.npos && pos.hist)) &&
                    (!use_list || (list.thr && list.list && list.count)) && (!use_cams || (cams.q_cams && cams.g_cams)) &&
                    (!hist || (hs.out && (hs.prefix || hs.prefix_bits == 0)));
  const auto stop = [rc](int code) { *rc = code; return false; };
  if (!(x.m >= 0 && x.n > 0 && x.D > 0)) return stop(CREID_E_ARG);
  if (!topk && !hist && x.m == 0) return stop(0);
  if (!topk && !hist && !ptrs) return stop(CREID_E_ARG);
  if ((use_pos && !stream_count_cap_ok(pos.cap)) || (use_list && !stream_topk_cap_ok(list.cap)) || x.D % d_mult != 0 || x.D > d_max ||
      (hist && !stream_hist_ok(hs.nsel, hs.prefix_bits, hs.bits)))
    return stop(CREID_E_SHAPE);
  if (!stream_mn_ok(x.m, x.n)) return stop(CREID_E_SHAPE);
  if (!dtype_ok) return stop(CREID_E_DTYPE);
  if (x.m == 0) return stop(0);
  if (!ptrs) return stop(CREID_E_ARG);
  return true;
}

/* Launch of either file's kernel for the epilogue EPI: the count epilogues through stream_count_launch (dynamic LDS; the banded
 * count with its row margins behind the lists), the top-k epilogues with static LDS only.  The histogram epilogue's table,
 * 2 * (nsel << bits) words, takes the place of the count's lists: pos_cap = stream_hist_lds_cap(nsel, bits). */
static int stream_hist_lds_cap(int nsel, int bits) { return ((nsel << bits) + SQ_TM - 1) / SQ_TM; }
template <auto Kernel, int EPI, class... Args>
static int stream_launch(const StreamSplit& sp, int pos_cap, void* stream, Args... args) {
  if constexpr (epi_is_topk(EPI)) {
    hipLaunchKernelGGL(Kernel, dim3(sp.grid), dim3(256), 0, as_stream(stream), args...);
    CREID_LAUNCH_RET();
  } else {
    return stream_count_launch<Kernel, EPI == EPI_BAND ? SQ_TM : 0>(sp, pos_cap, stream, args...);
  }
}

// Device side of the split: the run [g0, g1) of workgroup blockIdx.x, in units of the rows laid end to end.
__device__ __forceinline__ void stream_run(int tiles_m, int U, int upw, int mode, long long& g0, long long& g1) {
  // XCD-aware order: consecutive ids land on different XCDs; every XCD gets a contiguous run of ids
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int base = (xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    bid = base + (bid >> 3);
  }
  if (mode == 0) {
    const int split = bid / tiles_m, tile_m = bid - split * tiles_m;
    const int u0 = split * upw;
    g0 = (long long)tile_m * U + u0;
    g1 = (long long)tile_m * U + min(U, u0 + upw);
  } else {
    const long long T = (long long)tiles_m * U;
    g0 = bid * T / gridDim.x;
    g1 = (bid + 1) * T / gridDim.x;
  }
}
