// The streamed contraction of stream_eval.hip for bf16 / f16 features: the same two consumers -- the evaluation's count
// (CMC / mAP with no m x n matrix) and the retrieval's candidate collection (top-k with no matrix) -- and a third, the banded
// count (the exact fp32 evaluation's pre-filter: the count where the 16-bit distance decides, a list of the pairs where not), on
// v_mfma_f32_32x32x16_{bf16,f16}, the instruction of the materialised 16-bit distance kernel (sqdist_h16_kernel, dist.hip).
//
// Bit contract with sqdist_h16_kernel.  Every accumulator element starts at 0 and receives ONE MFMA per 16-deep k-step, steps
// in ascending k; lane (l31 = lane & 31, kh = lane >> 5) supplies k = 16 step + 8 kh + 0..7 in fragment elements 0..7 (the
// materialised kernel's chunk ch = 2 kk + kh of a 64-deep k-tile); k beyond D is zero-filled in 16-byte chunks (D % 8 == 0),
// and like there every k-tile runs its four steps, zero ones included; the distance is fmaf(-2, acc, qq[row] + gg[col]) and
// the key mono_key of it.  The query is the A operand and the gallery the B operand in both.  So a streamed distance has the
// bits of the materialised one, the exact-threshold argument of topk_stream and the tie rule of the count carry over, and the
// streamed results equal the materialised ones bit for bit.
//
//   sqdist_stream_h16_kernel<DT, EPI>   persistent: a workgroup walks a run of gallery tiles for one query tile and hands every
//                                       finished 64 x 256 tile, in registers, to the count, top-k or banded-count epilogue.
//   stream_poslist_h16_kernel<DT>       the distances of a query to its <= 128 positives on the same MFMA (a 16-bit MFMA's
//                                       internal summation cannot be reproduced with an fmaf chain).
// This file keeps what is 16-bit: the operand staging and LDS image, the k-loop, and the positives' distances.  The epilogues, the
// LDS state they read, the histogram flush and the positives' tail are stream_consume.hpp's, the work split (stream_split,
// stream_run) and the argument tests stream_common.hpp's -- one copy each, shared with the fp32 kernels of stream_eval.hip.  The
// plan, finalize and top-k select launches of stream_eval.hip do not depend on the feature type and serve both.
#include "stream_consume.hpp"

namespace {
constexpr int H_BK = 64;                         // k-tile: 64 elements = one 128-byte LDS row = 8 chunks of 16 bytes

template <int DT>
__device__ __forceinline__ f32x16 mfma_h16(const uint4& a, const uint4& b, f32x16 c) {
  if constexpr (DT == CREID_BF16) return Bf16T::mfma(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), c);
  else return F16T::mfma(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), c);
}
}  // namespace

// ----------------------------------------------------------------------------------------
// 1. positives.  One wave per query.  Candidates as in stream_poslist_kernel (the query's CSR slice, kept when the camera
//    differs), compacted in gallery-index order, 64 CSR entries per pass.  The distances: block b = candidates 32 b .. 32 b + 31
//    is one 32 x 32 MFMA tile whose A fragment is the query row in all 32 rows (every lane loads q[16 step + 8 kh ..]) and whose
//    B fragment is 16 bytes of the gathered gallery row cand[32 b + l31], straight from global memory; the distance of
//    candidate 32 b + l31 is accumulator register 0 of lane l31 (row 0).  A k-tile (four steps: one 128-byte line per gallery
//    row) is in flight while the previous one is multiplied.  CAMSETS: as in stream_poslist_kernel (cam_removed).
// ----------------------------------------------------------------------------------------
template <int DT, bool CAMSETS>
__global__ __launch_bounds__(64) void stream_poslist_h16_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ g, const float* __restrict__ qq,
    const float* __restrict__ gg, int D, const int32_t* __restrict__ q_slot, const int64_t* __restrict__ csr_off,
    const int32_t* __restrict__ g_order, const int64_t* __restrict__ q_cams, const int64_t* __restrict__ g_cams, int cap,
    unsigned* __restrict__ pos_key, int32_t* __restrict__ pos_idx, int32_t* __restrict__ npos) {
  __shared__ int cand[PL_MAXC];
  __shared__ unsigned skey[PL_MAXC];
  const int qi = blockIdx.x, lane = threadIdx.x;
  unsigned* okey = pos_key + (int64_t)qi * cap;
  int32_t* oidx = pos_idx + (int64_t)qi * cap;
  poslist_pad<64>(okey, oidx, cap);
  const int slot = q_slot[qi];
  if (slot < 0) { if (lane == 0) npos[qi] = 0; return; }
  const int64_t c0 = csr_off[slot], c1 = csr_off[slot + 1];
  const int64_t qc = q_cams[qi];
  int nc = 0;                                          // (wave-uniform)
  for (int64_t b = c0; b < c1; b += 64) {
    const int64_t e = b + lane;
    int gi = -1;
    if (e < c1) { gi = g_order[e]; if (cam_removed<CAMSETS>(g_cams[gi], qc)) gi = -1; }
    const unsigned long long bal = __ballot(gi >= 0);
    if (gi >= 0) {
      const int p = nc + __popcll(bal & lanemask_lt());
      if (p < PL_MAXC) cand[p] = gi;
    }
    nc += __popcll(bal);
  }
  __syncthreads();
  if (nc > cap || nc > PL_MAXC) { if (lane == 0) npos[qi] = -1; return; }   // the caller sends such queries to the general path
  if (nc == 0) { if (lane == 0) npos[qi] = 0; return; }
  const int l31 = lane & 31, kh = lane >> 5;
  const char* __restrict__ qrow = reinterpret_cast<const char*>(q + (int64_t)qi * D) + 16 * kh;
  const int nk = (D + H_BK - 1) / H_BK;
  const float qv = qq[qi];
  auto dist = [&](auto NB_) {                          // NB blocks of 32 candidates
    constexpr int NB = decltype(NB_)::value;
    const char* grow[NB];
    int gi[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      gi[b] = cand[min(32 * b + l31, nc - 1)];         // lanes beyond the list multiply a copy of its last row
      grow[b] = reinterpret_cast<const char*>(g + (int64_t)gi[b] * D) + 16 * kh;
    }
    f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    uint4 fa[2][4], fb[2][4][NB];
    auto load = [&](auto S_, int t) {                  // k-tile t: steps 4 t .. 4 t + 3, chunk 2 kk + kh of each row
      constexpr int S = decltype(S_)::value;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int k = t * H_BK + 16 * kk;              // + 8 kh: inside the row pointers
        const bool in = k + 8 * kh < D;                // branch-free: a chunk beyond D reads the row's first chunk, times a zero A
        const int ko = in ? 2 * k : -16 * kh;
        const unsigned mk = in ? 0xffffffffu : 0u;
        const uint4 av = *reinterpret_cast<const uint4*>(qrow + ko);
        fa[S][kk] = make_uint4(av.x & mk, av.y & mk, av.z & mk, av.w & mk);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const uint4 bv = *reinterpret_cast<const uint4*>(grow[b] + ko);
          fb[S][kk][b] = make_uint4(bv.x & mk, bv.y & mk, bv.z & mk, bv.w & mk);
        }
      }
    };
    auto mma = [&](auto S_) {
      constexpr int S = decltype(S_)::value;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = mfma_h16<DT>(fa[S][kk], fb[S][kk][b], acc[b]);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    load(I0{}, 0);
    int t = 0;
    for (; t + 2 <= nk; t += 2) {
      load(I1{}, t + 1);
      mma(I0{});
      if (t + 2 < nk) load(I0{}, t + 2);
      mma(I1{});
    }
    if (t < nk) mma(I0{});
    if (kh == 0) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (32 * b + l31 < nc) skey[32 * b + l31] = mono_key(fmaf(-2.0f, acc[b][0], qv + gg[gi[b]]));   // sqdist epilogue, same bits
    }
  };
  const int nblk = (nc + 31) >> 5;
  if (nblk == 1) dist(std::integral_constant<int, 1>{});
  else if (nblk == 2) dist(std::integral_constant<int, 2>{});
  else if (nblk == 3) dist(std::integral_constant<int, 3>{});
  else dist(std::integral_constant<int, 4>{});
  __syncthreads();
  poslist_rank_emit<64>(skey, cand, nc, okey, oidx, &npos[qi]);
}

// ----------------------------------------------------------------------------------------
// 2. streamed contraction.  Workgroup = (query tile of 64 rows, run of gallery units); 4 waves as 2 x 2, each 32 rows x 128
//    columns (1 x 4 MFMA 32 x 32 blocks, dealt to the two column waves alternately) of a 64 x 256 tile, k-tiles of 64.
//    LDS operand image: sqdist_h16_kernel's -- row-major [row][64] (128-byte rows), the eight 16-byte chunks of a row
//    XOR-swizzled with (row >> 1) & 7, so the 16 lanes a ds_read_b128 serves together touch 16 distinct 16-byte slots of the
//    256-byte bank row.  One image of 8 + 32 KiB; with the count's lists ([64][cap] keys + histogram, dynamic) 57 KiB at
//    capacity 32 -- two workgroups per CU up to capacity 64 -- and 105 KiB at capacity 128.  Per 16-deep step a wave reads
//    1 + NJ fragments for NJ MFMAs.  A k-tile is fetched into registers while the previous one is multiplied and replaces it
//    in LDS between two barriers; the second workgroup of the CU covers those waits.  The kernel is bound by operand traffic
//    (51 FLOP per operand byte) and its epilogue, not by the MFMA (profiles/stream_h16.md).
//    The work split (both modes), the clamped rows / columns and the narrow last tile (NJ < 4) are described at
//    sqdist_count_f32_kernel in stream_eval.hip.
// ----------------------------------------------------------------------------------------
template <int DT, int EPI>
__global__ __launch_bounds__(256, 2) void sqdist_stream_h16_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ g, const float* __restrict__ qq,
    const float* __restrict__ gg, int m, int n, int D, const int64_t* __restrict__ q_pids, const int64_t* __restrict__ g_pids,
    int cap, int log2cap, const unsigned* __restrict__ pos_key, const int32_t* __restrict__ pos_idx,
    const int32_t* __restrict__ npos, unsigned* __restrict__ hist_out, int tiles_m, int U, int upw, int mode,
    const float* __restrict__ tau, unsigned long long* __restrict__ cand, int32_t* __restrict__ cand_count, int acap,
    const int64_t* __restrict__ q_cams, const int64_t* __restrict__ g_cams, int camsets) {
  __shared__ __attribute__((aligned(16))) unsigned short As[SQ_TM * H_BK];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[SQ_TN * H_BK];
  __shared__ float s_qq[SQ_TM];
  __shared__ long long s_qpid[SQ_TM];
  __shared__ long long s_qcam[SQ_TM];            // EPI_TOPK_KEEP / EPI_HIST only (no other instantiation names it: no LDS there)
  __shared__ int s_np[SQ_TM];
  __shared__ unsigned s_kmax[SQ_TM];             // count: key of the row's last positive; top-k: key of the row's threshold
  extern __shared__ __attribute__((aligned(16))) unsigned dyn[];
  unsigned* s_keys = dyn;                        // [64][cap]
  unsigned* s_hist = dyn + SQ_TM * cap;          // [64][cap]
  float* s_mg = reinterpret_cast<float*>(dyn + 2 * SQ_TM * cap);     // [64], banded count only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const StreamLds L{s_qq, s_qpid, s_np, s_kmax, s_keys, s_hist, s_mg, s_qcam};
  const StreamProblem P{m, n, cap, log2cap, qq, gg, q_pids, g_pids, pos_key, pos_idx, npos, hist_out, tau, cand, cand_count, acap,
                        q_cams, g_cams, camsets};
  long long g0, g1;                              // this workgroup's run, in units of the rows laid end to end
  stream_run(tiles_m, U, upw, mode, g0, g1);

  // Staging: a pass of the 256 threads covers 32 rows x 8 chunks; the query tile is 2 passes, the gallery tile 8 (2 per unit).
  // Row lrow + 32 i has the swizzle of row lrow, so one LDS offset serves every pass.
  const int lrow = tid >> 3, lch = tid & 7;
  const int so = lrow * H_BK + ((lch ^ ((lrow >> 1) & 7)) << 3);
  // one wave-uniform base per operand + a 32-bit byte offset per lane and row (clamped rows: at most 256 rows x D elements)
  const char* abase = nullptr;
  const char* bbase = nullptr;
  unsigned aoff[2], boff[8];
  uint4 ra[2], rb[8];                              // the staged k-tile: fetched while the previous one is multiplied
  auto set_tile = [&](int col0) {
    const int c0 = min(col0, n - 1);
    bbase = reinterpret_cast<const char*>(g + (int64_t)c0 * D);
#pragma unroll
    for (int i = 0; i < 8; ++i) boff[i] = (unsigned)(min(col0 + lrow + 32 * i, n - 1) - c0) * (unsigned)D * 2u + 16u * lch;
  };
  // k-tile at k0 into the staging registers: the query tile and the first ni passes of the gallery tile.  Branch-free: a lane
  // whose chunk lies beyond D reads its row's first 16 bytes instead and lstore writes zeros for it (D % 8 == 0: a chunk is
  // inside or outside).  (With a branch per load the loads of a k-tile were issued one after the other's arrival.)
  unsigned rmask = 0u;
  auto gload = [&](int k0, int ni) {
    const bool in = k0 + 8 * lch < D;
    rmask = in ? 0xffffffffu : 0u;
    const unsigned ko = in ? (unsigned)k0 * 2u : 0u - 16u * lch;     // added to aoff / boff (which hold + 16 lch): no wrap below 0
#pragma unroll
    for (int i = 0; i < 2; ++i) ra[i] = *reinterpret_cast<const uint4*>(abase + (aoff[i] + ko));
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < ni) rb[i] = *reinterpret_cast<const uint4*>(bbase + (boff[i] + ko));
  };
  auto masked = [](const uint4& v, unsigned mk) { return make_uint4(v.x & mk, v.y & mk, v.z & mk, v.w & mk); };
  auto lstore = [&](int ni) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(&As[so + 32 * H_BK * i]) = masked(ra[i], rmask);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < ni) *reinterpret_cast<uint4*>(&Bs[so + 32 * H_BK * i]) = masked(rb[i], rmask);
  };
  // fragments: row wm * 32 + l31 of the query tile; wave wn multiplies the 32-column blocks wn, wn + 2, wn + 4, wn + 6
  // (block b = gallery rows 32 b .. 32 b + 31); every one of these rows has the swizzle (l31 >> 1) & 7
  const int fsw = (l31 >> 1) & 7;
  const int fa = (wm * 32 + l31) * H_BK, fb = (wn * 32 + l31) * H_BK;
  const int nk = (D + H_BK - 1) / H_BK;
  int row0 = 0;

  // ---- one tile of NJ units at column col0; `next` >= 0: the following tile's column.  On entry the staging registers hold
  //      k-tile 0.
  auto tile = [&](auto NJ_, int col0, int next) {
    constexpr int NJ = decltype(NJ_)::value;
    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    __syncthreads();                               // previous tile's readers are done with the LDS image
    lstore(2 * NJ);
    __syncthreads();
    // k-tile t is multiplied while k-tile t + 1 is fetched into the staging registers; then, between two barriers, it replaces
    // k-tile t in LDS.  The LDS image is single-buffered on purpose: 40 KiB instead of 80 lets TWO workgroups share a CU, and
    // the second one multiplies while this one waits for its loads, at its barriers or in its epilogue (measured with the
    // count epilogue at 2228 x 17661 x 2048: 0.36 ms against 0.99 ms for the double-buffered image with one workgroup per CU;
    // profiles/stream_h16.md).
    for (int t = 0; t < nk; ++t) {
      if (t + 1 < nk) gload((t + 1) * H_BK, 2 * NJ);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {             // four 16-deep steps in k order; this lane's chunk of step kk is 2 kk + kh
        const int co = ((2 * kk + kh) ^ fsw) << 3;
        const uint4 a = *reinterpret_cast<const uint4*>(&As[fa + co]);
        uint4 b[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = *reinterpret_cast<const uint4*>(&Bs[fb + 64 * H_BK * j + co]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = mfma_h16<DT>(a, b[j], acc[j]);
      }
      if (t + 1 < nk) {
        __syncthreads();
        lstore(2 * NJ);
        __syncthreads();
      }
    }
    // the next tile's k-tile 0: under the (light) top-k epilogue; behind the count epilogue, whose searches need the registers,
    // and behind the junk-free top-k's, whose label test needs one register more than the 256 leave under the staged tile
    if constexpr (EPI == EPI_TOPK) { if (next >= 0) { set_tile(next); gload(0, 8); } }
    // One accumulator row at a time in the count (the fp32 kernel runs two): one row's NJ search chains keep this kernel inside
    // the 256 registers of two workgroups per CU, and the second workgroup fills the gaps of the chains.
    stream_tile_consume<EPI, 1, NJ>(acc, wm, wn, l31, kh, row0, col0, 0, L, P);
    if constexpr (EPI != EPI_TOPK) { if (next >= 0) { set_tile(next); gload(0, 8); } }
  };

  while (g0 < g1) {                               // the run's segments: one per row it touches
    const int row = (int)(g0 / U), u0 = (int)(g0 - (long long)row * U);
    const int u1 = (int)min((long long)U, u0 + (g1 - g0));
    g0 += u1 - u0;
    row0 = row * SQ_TM;
    __syncthreads();                               // the previous segment's histogram has been flushed
    stream_segment_begin<EPI>(L, P, row0);
    const int r0c = min(row0, m - 1);
    abase = reinterpret_cast<const char*>(q + (int64_t)r0c * D);
#pragma unroll
    for (int i = 0; i < 2; ++i) aoff[i] = (unsigned)(min(row0 + lrow + 32 * i, m - 1) - r0c) * (unsigned)D * 2u + 16u * lch;
    const int cend = u1 * 64;
    int col = u0 * 64;
    set_tile(col);
    gload(0, 8);
    while (col < cend) {
      const int nj = min(4, (cend - col) >> 6), next = col + 256 < cend ? col + 256 : -1;
      STREAM_DISPATCH_NJ(nj, tile, col, next);
      col += 256;
    }
    if constexpr (!epi_is_topk(EPI)) stream_segment_end<EPI>(L, P, row0);
  }
}

namespace {
constexpr int64_t H_MAX_D = 1 << 20;             // the staging offsets are 32-bit byte offsets over 256 rows of D elements
}

template <bool CAMSETS>
static int stream_poslist_h16_launch(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n, int64_t D,
                                     int dtype, const int32_t* q_slot, const int64_t* csr_off, const int32_t* g_order,
                                     const int64_t* q_cams, const int64_t* g_cams, int32_t cap, uint32_t* pos_key,
                                     int32_t* pos_idx, int32_t* npos, void* stream) {
  CREID_CHECK_ARG(m >= 0 && n > 0 && D > 0);
  if (m == 0) return 0;
  CREID_CHECK_ARG(q && g && qq && gg && q_slot && csr_off && g_order && q_cams && g_cams && pos_key && pos_idx && npos);
  if (!stream_count_cap_ok(cap) || D % 8 != 0 || D > H_MAX_D) return CREID_E_SHAPE;
  if (!stream_mn_ok(m, n)) return CREID_E_SHAPE;
  if (!creid_is16(dtype)) return CREID_E_DTYPE;
  const unsigned short* qh = static_cast<const unsigned short*>(q);
  const unsigned short* gh = static_cast<const unsigned short*>(g);
  if (dtype == CREID_BF16)
    hipLaunchKernelGGL((stream_poslist_h16_kernel<CREID_BF16, CAMSETS>), dim3((unsigned)m), dim3(64), 0, as_stream(stream), qh, gh,
                       qq, gg, (int)D, q_slot, csr_off, g_order, q_cams, g_cams, (int)cap, pos_key, pos_idx, npos);
  else
    hipLaunchKernelGGL((stream_poslist_h16_kernel<CREID_F16, CAMSETS>), dim3((unsigned)m), dim3(64), 0, as_stream(stream), qh, gh,
                       qq, gg, (int)D, q_slot, csr_off, g_order, q_cams, g_cams, (int)cap, pos_key, pos_idx, npos);
  CREID_LAUNCH_RET();
}

/* The one host side of the streamed 16-bit contraction: the argument tests, the work split, and the launch of the kernel for
 * the dtype and the epilogue EPI with the groups it does not use left empty. */
template <int EPI>
static int stream_h16_launch(const StreamRows& x, int dtype, const StreamPids& pids, const StreamPos& pos, const StreamList& list,
                             const StreamCams& cams, void* stream, const StreamHist& hs = {}) {
  int rc;
  if (!stream_args_pass<EPI>(x, pids, pos, list, cams, 8, H_MAX_D, creid_is16(dtype), &rc, hs)) return rc;
  constexpr bool topk = epi_is_topk(EPI), hist = EPI == EPI_HIST;
  const StreamSplit sp = stream_split(x.m, x.n, x.D, 2);
  // the histogram epilogue: cap = the selectors, log2cap = the digit's width, acap = the prefix bits (stream_consume.hpp)
  const int cap = hist ? hs.nsel : topk ? list.cap : pos.cap, log2cap = hist ? hs.bits : topk ? 0 : stream_log2cap(pos.cap);
  const int acap = hist ? hs.prefix_bits : EPI == EPI_BAND ? list.cap : 0;
  const int lds_cap = hist ? stream_hist_lds_cap(hs.nsel, hs.bits) : pos.cap;
  const auto launch = [&](auto dt) {
    return stream_launch<sqdist_stream_h16_kernel<decltype(dt)::value, EPI>, EPI>(
        sp, lds_cap, stream, static_cast<const unsigned short*>(x.q), static_cast<const unsigned short*>(x.g), x.qq, x.gg, (int)x.m,
        (int)x.n, (int)x.D, pids.q_pids, pids.g_pids, cap, log2cap, hist ? hs.prefix : pos.key, pos.idx, pos.npos, pos.hist,
        sp.tiles_m, sp.U, sp.upw, sp.mode, list.thr, hist ? hs.out : list.list, list.count, acap, cams.q_cams, cams.g_cams,
        cams.camsets);
  };
  return dtype == CREID_BF16 ? launch(std::integral_constant<int, CREID_BF16>{}) : launch(std::integral_constant<int, CREID_F16>{});
}

extern "C" {

int creid_stream_poslist_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n, int64_t D,
                             int dtype, const int32_t* q_slot, const int64_t* csr_off, const int32_t* g_order,
                             const int64_t* q_cams, const int64_t* g_cams, int32_t cap, uint32_t* pos_key, int32_t* pos_idx,
                             int32_t* npos, void* stream) {
  return stream_poslist_h16_launch<false>(q, g, qq, gg, m, n, D, dtype, q_slot, csr_off, g_order, q_cams, g_cams, cap, pos_key,
                                          pos_idx, npos, stream);
}

/* creid_stream_poslist_h16 for gallery entries that carry camera sets (see creid_stream_poslist_camsets) */
int creid_stream_poslist_h16_camsets(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                     int64_t D, int dtype, const int32_t* q_slot, const int64_t* csr_off, const int32_t* g_order,
                                     const int64_t* q_cams, const int64_t* g_cam_masks, int32_t cap, uint32_t* pos_key,
                                     int32_t* pos_idx, int32_t* npos, void* stream) {
  return stream_poslist_h16_launch<true>(q, g, qq, gg, m, n, D, dtype, q_slot, csr_off, g_order, q_cams, g_cam_masks, cap, pos_key,
                                         pos_idx, npos, stream);
}

int creid_stream_count_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n, int64_t D,
                           int dtype, const int64_t* q_pids, const int64_t* g_pids, int32_t cap, const uint32_t* pos_key,
                           const int32_t* pos_idx, const int32_t* npos, uint32_t* hist, void* stream) {
  return stream_h16_launch<EPI_COUNT>({q, g, qq, gg, m, n, D}, dtype, {q_pids, g_pids}, {cap, pos_key, pos_idx, npos, hist}, {}, {},
                                      stream);
}

int creid_stream_topk_collect_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                  int64_t D, int dtype, const float* tau, int32_t cap, uint64_t* cand, int32_t* count,
                                  void* stream) {
  return stream_h16_launch<EPI_TOPK>({q, g, qq, gg, m, n, D}, dtype, {}, {},
                                     {tau, reinterpret_cast<unsigned long long*>(cand), count, cap}, {}, stream);
}

int creid_stream_topk_collect_keep_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                       int64_t D, int dtype, const float* tau, const int64_t* q_pids, const int64_t* g_pids,
                                       const int64_t* q_cams, const int64_t* g_cams, int32_t camsets, int32_t cap,
                                       uint64_t* cand, int32_t* count, void* stream) {
  return stream_h16_launch<EPI_TOPK_KEEP>({q, g, qq, gg, m, n, D}, dtype, {q_pids, g_pids}, {},
                                          {tau, reinterpret_cast<unsigned long long*>(cand), count, cap},
                                          {q_cams, g_cams, camsets != 0 ? 1 : 0}, stream);
}

int creid_stream_dist_hist_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n, int64_t D,
                               int dtype, const int64_t* q_pids, const int64_t* g_pids, const int64_t* q_cams, const int64_t* g_cams,
                               int32_t camsets, const uint32_t* prefix, int32_t nsel, int32_t prefix_bits, int32_t bits,
                               uint64_t* hist, void* stream) {
  return stream_h16_launch<EPI_HIST>({q, g, qq, gg, m, n, D}, dtype, {q_pids, g_pids}, {}, {}, {q_cams, g_cams, camsets != 0 ? 1 : 0},
                                     stream, {prefix, nsel, prefix_bits, bits, reinterpret_cast<unsigned long long*>(hist)});
}

int creid_stream_count_band_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n, int64_t D,
                                int dtype, const int64_t* q_pids, const int64_t* g_pids, int32_t cap, const uint32_t* pos_key,
                                const int32_t* pos_idx, const int32_t* npos, const float* margin, int32_t amb_cap, uint32_t* amb,
                                int32_t* amb_count, uint32_t* hist, void* stream) {
  return stream_h16_launch<EPI_BAND>({q, g, qq, gg, m, n, D}, dtype, {q_pids, g_pids}, {cap, pos_key, pos_idx, npos, hist},
                                     {margin, reinterpret_cast<unsigned long long*>(amb), amb_count, amb_cap}, {}, stream);
}

}  // extern "C"
