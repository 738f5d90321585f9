// The streamed contraction of stream_eval.hip for bf16 / f16 features: the same two consumers -- the evaluation's count
// (CMC / mAP with no m x n matrix) and the retrieval's candidate collection (top-k with no matrix) -- on
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
//   sqdist_stream_h16_kernel<DT, EPI>   persistent: a workgroup walks a run of gallery tiles for one query tile (the work
//                                       split of the fp32 kernel: stream_split(), both modes) and consumes every finished
//                                       64 x 256 tile in registers with the count or the top-k epilogue.  The epilogues are
//                                       this file's own copies of sqdist_count_f32_kernel's: that kernel's register
//                                       allocation is tuned to the last VGPR and was left alone.
//   stream_poslist_h16_kernel<DT>       the distances of a query to its <= 128 positives on the same MFMA (a 16-bit MFMA's
//                                       internal summation cannot be reproduced with an fmaf chain).
// The plan, finalize and top-k select launches of stream_eval.hip do not depend on the feature type and serve both.
#include "stream_common.hpp"
#include <type_traits>

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
//    row) is in flight while the previous one is multiplied.
// ----------------------------------------------------------------------------------------
template <int DT>
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
  for (int i = lane; i < cap; i += 64) { okey[i] = 0xffffffffu; oidx[i] = 0x7fffffff; }   // padding for the search
  const int slot = q_slot[qi];
  if (slot < 0) { if (lane == 0) npos[qi] = 0; return; }
  const int64_t c0 = csr_off[slot], c1 = csr_off[slot + 1];
  const int64_t qc = q_cams[qi];
  int nc = 0;                                          // (wave-uniform)
  for (int64_t b = c0; b < c1; b += 64) {
    const int64_t e = b + lane;
    int gi = -1;
    if (e < c1) { gi = g_order[e]; if (g_cams[gi] == qc) gi = -1; }
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
  for (int c = lane; c < nc; c += 64) {                // rank by counting over (key, gallery index)
    const unsigned k = skey[c];
    const int gi = cand[c];
    int pos = 0;
    for (int o = 0; o < nc; ++o) {
      const unsigned ko = skey[o];
      pos += (ko < k || (ko == k && cand[o] < gi)) ? 1 : 0;
    }
    okey[pos] = k; oidx[pos] = gi;
  }
  if (lane == 0) npos[qi] = nc;
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
//    The work split, the clamped rows / columns, the narrow last tile (NJ < 4) and both epilogues are the fp32 kernel's; see
//    stream_eval.hip.
// ----------------------------------------------------------------------------------------
template <int DT, int EPI>
__global__ __launch_bounds__(256, 2) void sqdist_stream_h16_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ g, const float* __restrict__ qq,
    const float* __restrict__ gg, int m, int n, int D, const int64_t* __restrict__ q_pids, const int64_t* __restrict__ g_pids,
    int cap, int log2cap, const unsigned* __restrict__ pos_key, const int32_t* __restrict__ pos_idx,
    const int32_t* __restrict__ npos, unsigned* __restrict__ hist_out, int tiles_m, int U, int upw, int mode,
    const float* __restrict__ tau, unsigned long long* __restrict__ cand, int32_t* __restrict__ cand_count) {
  __shared__ __attribute__((aligned(16))) unsigned short As[SQ_TM * H_BK];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[SQ_TN * H_BK];
  __shared__ float s_qq[SQ_TM];
  __shared__ long long s_qpid[SQ_TM];
  __shared__ int s_np[SQ_TM];
  __shared__ unsigned s_kmax[SQ_TM];             // count: key of the row's last positive; top-k: key of the row's threshold
  extern __shared__ __attribute__((aligned(16))) unsigned dyn[];
  unsigned* s_keys = dyn;                        // [64][cap]
  unsigned* s_hist = dyn + SQ_TM * cap;          // [64][cap]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  // XCD-aware order: consecutive ids land on different XCDs; every XCD gets a contiguous run of ids
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int base = (xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    bid = base + (bid >> 3);
  }
  long long g0, g1;                              // this workgroup's run, in units of the rows laid end to end
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
    // the next tile's k-tile 0: under the (light) top-k epilogue; behind the count epilogue, whose searches need the registers
    if constexpr (EPI == EPI_TOPK) { if (next >= 0) { set_tile(next); gload(0, 8); } }
    // ---- epilogue: the tile is consumed here (row-major walk: the row's metadata is read once per NJ columns)
    int rbase = wm * 32 + 4 * kh;                  // opaque per tile: the 16 rows' LDS addresses derived from it are recomputed here
    asm volatile("" : "+v"(rbase));                // instead of living in registers (or scratch) across the k-loop
    float gv[NJ];
    [[maybe_unused]] long long gp[NJ];
    bool okc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = col0 + (wn + 2 * j) * 32 + l31;
      okc[j] = c < n;
      gv[j] = okc[j] ? gg[c] : 0.f;
      if constexpr (EPI == EPI_COUNT) gp[j] = okc[j] ? (long long)g_pids[c] : 0;
    }
    if constexpr (EPI == EPI_TOPK) {
      // One accumulator row at a time: its threshold is one LDS read, a hit one global atomic (rows beyond m multiply a
      // clamped copy of the last query row and are dropped here, like columns beyond n).
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = rbase + (r & 3) + 8 * (r >> 2);
        const float qv = s_qq[rl];
        const unsigned kt = s_kmax[rl];
        const bool okr = row0 + rl < m;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const unsigned key = mono_key(fmaf(-2.0f, acc[j][r], qv + gv[j]));
          if (okr && okc[j] && key <= kt) {
            const int64_t rr = row0 + rl;
            const int slot = atomicAdd(&cand_count[rr], 1);
            if (slot < cap)
              cand[rr * cap + slot] = ((unsigned long long)key << 32) | (unsigned)(col0 + (wn + 2 * j) * 32 + l31);
          }
        }
      }
      return;
    }
    // H accumulator rows x NJ column blocks = H NJ binary searches in flight per lane (the search is a chain of dependent LDS
    // reads).  The fp32 kernel runs two rows at a time; one row keeps this kernel inside the 256 registers of two workgroups
    // per CU, and the second workgroup fills the gaps of the chains.
    constexpr int H = 1;
#pragma unroll
    for (int r = 0; r < 16; r += H) {
      int rl[H], np[H], lo[H][NJ];
      unsigned key[H][NJ];
      bool live[H][NJ];
      const unsigned* K[H];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        rl[h] = rbase + ((r + h) & 3) + 8 * ((r + h) >> 2);
        np[h] = s_np[rl[h]];
        const long long qp = s_qpid[rl[h]];
        const float qv = s_qq[rl[h]];
        const unsigned kmax = s_kmax[rl[h]];
        K[h] = s_keys + (rl[h] << log2cap);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          key[h][j] = mono_key(fmaf(-2.0f, acc[j][r + h], qv + gv[j]));
          // positives / removed entries (same pid) are not counted; behind every positive: affects no rank
          live[h][j] = np[h] > 0 && okc[j] && gp[j] != qp && key[h][j] <= kmax;
          lo[h][j] = 0;
        }
      }
      if (np[0] == 0 && np[H - 1] == 0) continue;                      // uniform per wave half
      for (int step = cap >> 1; step > 0; step >>= 1) {
#pragma unroll
        for (int h = 0; h < H; ++h)
#pragma unroll
          for (int j = 0; j < NJ; ++j) lo[h][j] += (K[h][lo[h][j] + step - 1] < key[h][j]) ? step : 0;
      }
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          int l = lo[h][j];
          l += (K[h][l] < key[h][j]) ? 1 : 0;                      // l = #positives with key strictly below
          if (live[h][j]) {
            if (l < np[h] && K[h][l] == key[h][j]) {               // ties: by gallery index (rare)
              const int c = col0 + (wn + 2 * j) * 32 + l31;
              int rr_ = row0 + rl[h];
              asm volatile("" : "+v"(rr_));                        // keeps 16 rows' index pointers out of the k-loop's registers
              while (l < np[h] && K[h][l] == key[h][j] && pos_idx[(int64_t)rr_ * cap + l] < c) ++l;
            }
            if (l < np[h]) atomicAdd(&s_hist[(rl[h] << log2cap) + l], 1u);
          }
        }
    }
    if (next >= 0) { set_tile(next); gload(0, 8); }
  };

  while (g0 < g1) {                               // the run's segments: one per row it touches
    const int row = (int)(g0 / U), u0 = (int)(g0 - (long long)row * U);
    const int u1 = (int)min((long long)U, u0 + (g1 - g0));
    g0 += u1 - u0;
    row0 = row * SQ_TM;
    __syncthreads();                               // the previous segment's histogram has been flushed
    int ts = tid;                                  // opaque: the set-up's LDS addresses are recomputed per segment instead of
    asm volatile("" : "+v"(ts));                   // occupying registers across the k-loops
    if constexpr (EPI == EPI_TOPK) {
      if (ts < SQ_TM) {
        const int rr = row0 + ts;
        s_qq[ts] = rr < m ? qq[rr] : 0.f;
        s_kmax[ts] = rr < m ? mono_key(tau[rr]) : 0u;
      }
    } else {
      for (int i = ts; i < SQ_TM * cap; i += 256) {
        const int r = i >> log2cap, rr = row0 + r;
        s_keys[i] = rr < m ? pos_key[(int64_t)rr * cap + (i & (cap - 1))] : 0xffffffffu;
        s_hist[i] = 0u;
      }
      if (ts < SQ_TM) {
        const int rr = row0 + ts;
        const int np = rr < m ? npos[rr] : 0;
        s_np[ts] = np > 0 ? np : 0;
        s_qq[ts] = rr < m ? qq[rr] : 0.f;
        s_qpid[ts] = rr < m ? (long long)q_pids[rr] : 0;
        s_kmax[ts] = np > 0 ? pos_key[(int64_t)rr * cap + np - 1] : 0u;
      }
    }
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
      if (nj == 4) tile(std::integral_constant<int, 4>{}, col, next);
      else if (nj == 3) tile(std::integral_constant<int, 3>{}, col, next);
      else if (nj == 2) tile(std::integral_constant<int, 2>{}, col, next);
      else tile(std::integral_constant<int, 1>{}, col, next);
      col += 256;
    }
    if constexpr (EPI == EPI_COUNT) {
      __syncthreads();
      for (int i = ts; i < SQ_TM * cap; i += 256) {
        const unsigned v = s_hist[i];
        const int rr = row0 + (i >> log2cap);
        if (v && rr < m) atomicAdd(&hist_out[(int64_t)rr * cap + (i & (cap - 1))], v);      // integer: order-independent
      }
    }
  }
}

namespace {
constexpr int64_t H_MAX_D = 1 << 20;             // the staging offsets are 32-bit byte offsets over 256 rows of D elements
}

extern "C" {

int creid_stream_poslist_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n, int64_t D,
                             int dtype, const int32_t* q_slot, const int64_t* csr_off, const int32_t* g_order,
                             const int64_t* q_cams, const int64_t* g_cams, int32_t cap, uint32_t* pos_key, int32_t* pos_idx,
                             int32_t* npos, void* stream) {
  CREID_CHECK_ARG(m >= 0 && n > 0 && D > 0);
  if (m == 0) return 0;
  CREID_CHECK_ARG(q && g && qq && gg && q_slot && csr_off && g_order && q_cams && g_cams && pos_key && pos_idx && npos);
  if (cap < 2 || cap > PL_MAXC || (cap & (cap - 1)) != 0 || D % 8 != 0 || D > H_MAX_D) return CREID_E_SHAPE;
  if (n > 0x7ffffff0LL || m > 0x7ffffff0LL) return CREID_E_SHAPE;
  if (!creid_is16(dtype)) return CREID_E_DTYPE;
  const unsigned short* qh = static_cast<const unsigned short*>(q);
  const unsigned short* gh = static_cast<const unsigned short*>(g);
  if (dtype == CREID_BF16)
    hipLaunchKernelGGL(stream_poslist_h16_kernel<CREID_BF16>, dim3((unsigned)m), dim3(64), 0, as_stream(stream), qh, gh, qq, gg,
                       (int)D, q_slot, csr_off, g_order, q_cams, g_cams, (int)cap, pos_key, pos_idx, npos);
  else
    hipLaunchKernelGGL(stream_poslist_h16_kernel<CREID_F16>, dim3((unsigned)m), dim3(64), 0, as_stream(stream), qh, gh, qq, gg,
                       (int)D, q_slot, csr_off, g_order, q_cams, g_cams, (int)cap, pos_key, pos_idx, npos);
  CREID_LAUNCH_RET();
}

int creid_stream_count_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n, int64_t D,
                           int dtype, const int64_t* q_pids, const int64_t* g_pids, int32_t cap, const uint32_t* pos_key,
                           const int32_t* pos_idx, const int32_t* npos, uint32_t* hist, void* stream) {
  CREID_CHECK_ARG(m >= 0 && n > 0 && D > 0);
  if (m == 0) return 0;
  CREID_CHECK_ARG(q && g && qq && gg && q_pids && g_pids && pos_key && pos_idx && npos && hist);
  if (cap < 2 || cap > PL_MAXC || (cap & (cap - 1)) != 0 || D % 8 != 0 || D > H_MAX_D) return CREID_E_SHAPE;
  if (n > 0x7ffffff0LL || m > 0x7ffffff0LL) return CREID_E_SHAPE;
  if (!creid_is16(dtype)) return CREID_E_DTYPE;
  int log2cap = 0;
  while ((1 << log2cap) < cap) ++log2cap;
  const StreamSplit sp = stream_split(m, n, D, 2);
  const size_t dyn = (size_t)2 * SQ_TM * cap * sizeof(unsigned);
  const unsigned short* qh = static_cast<const unsigned short*>(q);
  const unsigned short* gh = static_cast<const unsigned short*>(g);
#define CREID_COUNT_H16_LAUNCH(DT)                                                                                          \
  do {                                                                                                                       \
    static const hipError_t attr_rc =                                                                                        \
        hipFuncSetAttribute(reinterpret_cast<const void*>(sqdist_stream_h16_kernel<DT, EPI_COUNT>),                          \
                            hipFuncAttributeMaxDynamicSharedMemorySize, 2 * SQ_TM * PL_MAXC * (int)sizeof(unsigned));         \
    if (attr_rc != hipSuccess) return (int)attr_rc;                                                                          \
    hipLaunchKernelGGL((sqdist_stream_h16_kernel<DT, EPI_COUNT>), dim3(sp.grid), dim3(256), dyn, as_stream(stream), qh, gh,  \
                       qq, gg, (int)m, (int)n, (int)D, q_pids, g_pids, (int)cap, log2cap, pos_key, pos_idx, npos, hist,        \
                       sp.tiles_m, sp.U, sp.upw, sp.mode, (const float*)nullptr, (unsigned long long*)nullptr,               \
                       (int32_t*)nullptr);                                                                                   \
  } while (0)
  if (dtype == CREID_BF16) CREID_COUNT_H16_LAUNCH(CREID_BF16); else CREID_COUNT_H16_LAUNCH(CREID_F16);
#undef CREID_COUNT_H16_LAUNCH
  CREID_LAUNCH_RET();
}

int creid_stream_topk_collect_h16(const void* q, const void* g, const float* qq, const float* gg, int64_t m, int64_t n,
                                  int64_t D, int dtype, const float* tau, int32_t cap, uint64_t* cand, int32_t* count,
                                  void* stream) {
  CREID_CHECK_ARG(m >= 0 && n > 0 && D > 0);
  if (cap < TS_MIN_CAP || cap > TS_MAX_CAP || (cap & (cap - 1)) != 0 || D % 8 != 0 || D > H_MAX_D) return CREID_E_SHAPE;
  if (n > 0x7ffffff0LL || m > 0x7ffffff0LL) return CREID_E_SHAPE;
  if (!creid_is16(dtype)) return CREID_E_DTYPE;
  if (m == 0) return 0;
  CREID_CHECK_ARG(q && g && qq && gg && tau && cand && count);
  const StreamSplit sp = stream_split(m, n, D, 2);
  const unsigned short* qh = static_cast<const unsigned short*>(q);
  const unsigned short* gh = static_cast<const unsigned short*>(g);
#define CREID_TOPK_H16_LAUNCH(DT)                                                                                           \
  hipLaunchKernelGGL((sqdist_stream_h16_kernel<DT, EPI_TOPK>), dim3(sp.grid), dim3(256), 0, as_stream(stream), qh, gh, qq,   \
                     gg, (int)m, (int)n, (int)D, (const int64_t*)nullptr, (const int64_t*)nullptr, (int)cap, 0,              \
                     (const unsigned*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, (unsigned*)nullptr,         \
                     sp.tiles_m, sp.U, sp.upw, sp.mode, tau, reinterpret_cast<unsigned long long*>(cand), count)
  if (dtype == CREID_BF16) CREID_TOPK_H16_LAUNCH(CREID_BF16); else CREID_TOPK_H16_LAUNCH(CREID_F16);
#undef CREID_TOPK_H16_LAUNCH
  CREID_LAUNCH_RET();
}

}  // extern "C"
