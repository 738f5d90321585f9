// What a streamed contraction does around and after its k-loop, whatever the operand type: stream_eval.hip (fp32 features, f32
// MFMA) and stream_h16.hip (bf16 / f16 features, 16-bit MFMA) stage their operands, run their k-loops and walk their run of tiles
// themselves, and call the pieces here for everything that touches a finished accumulator tile.  A tile is 64 x 256, four waves
// as 2 x 2 (wm, wn), each 32 rows x NJ blocks of 32 columns (block j of wave wn = columns (wn + 2 j) * 32 ..); accumulator
// register r of lane (l31 = lane & 31, kh = lane >> 5) is row wm * 32 + 4 kh + (r & 3) + 8 (r >> 2), column l31 of its block.
//
//   stream_segment_begin<EPI>   per (query tile, run of columns): the LDS state the consumer reads
//   stream_tile_consume<EPI, H, NJ>   one finished tile: the count, the top-k, the banded-count, the junk-free top-k or the
//                               radix-histogram epilogue
//   stream_segment_end          count / banded count / radix histogram: the LDS histogram leaves for global memory
//   STREAM_DISPATCH_NJ          the tile width as a compile-time constant
//   poslist_pad / poslist_rank_emit   the tail of the two positives kernels
//
// This file carries the bit contract of the streamed paths: the distance is fmaf(-2, acc, qq[row] + gg[col]), its key mono_key of
// it -- the bits of the materialised distance kernels -- and ties resolve by gallery index like the stable rank kernel.
#pragma once
#include "stream_common.hpp"
#include <type_traits>

// The LDS state of a segment: per query row of the tile its norm, pid, number of positives and `kmax` (count: key of the row's last
// positive; top-k: key of the row's threshold); count only: the rows' positive keys [64][cap] and the histogram [64][cap];
// banded count: the count's state and the rows' margins `mg`; junk-free top-k: the top-k's state and the rows' pid and camera;
// radix histogram: the rows' norm, pid and camera, and in `keys` the table [nsel][2][2^bits] of counts (class 0 genuine, 1 impostor).
struct StreamLds {
  float* qq;
  long long* qpid;
  int* np;
  unsigned* kmax;
  unsigned* keys;
  unsigned* hist;
  float* mg;
  long long* qcam;
};

// The problem the consumers see: sizes, list capacity, and the global arrays they read or write (count: q_pids .. hist_out;
// top-k: tau .. cand_count; the other group is unused and may be null.  Banded count: the count's group, and tau = the rows'
// margins, cand = the rows' lists of ambiguous columns -- [m][acap] 32-bit words --, cand_count = their lengths.  Junk-free
// top-k: the top-k's group, the pids, and the cameras: q_cams plain ids; g_cams plain ids, or -- camsets != 0 -- bitmasks.
// Radix histogram: the pids and the cameras; cap = the number of selectors nsel, log2cap = the digit's width `bits`, acap = the
// prefix bits, pos_key = the nsel prefixes, cand = the counts uint64 [nsel][2][2^bits] the segments add into.)
struct StreamProblem {
  int m, n, cap, log2cap;
  const float* qq;
  const float* gg;
  const int64_t* q_pids;
  const int64_t* g_pids;
  const unsigned* pos_key;
  const int32_t* pos_idx;
  const int32_t* npos;
  unsigned* hist_out;
  const float* tau;
  unsigned long long* cand;
  int32_t* cand_count;
  int acap;
  const int64_t* q_cams;
  const int64_t* g_cams;
  int camsets;
};

// One count per lane with `hit` into the LDS table `tab`, aggregated per wave: the first pending lane's bin is broadcast, the lanes
// that share it are counted with one ballot and leave with ONE ds_add of the popcount; the rounds go on while they pay -- until
// one collects fewer than HS_MIN_GROUP lanes, or after the first when `once` -- and whoever is still pending then adds for itself.
// The first radix pass is the contended one: the distance keys of unit rows crowd into 2-4 of its bins, so a wave is done after
// 2-4 rounds where 64 atomics would have queued on as many addresses.  Behind a prefix (`once`) the next digit is mantissa
// bits, close to uniform over its bins: a round per distinct bin would be up to 64 serial rounds per call (measured: the second
// pass 6.8 x the count kernel's time in fp32 and 27 x in bf16 with unbounded rounds, profiles/roc_stream.md), while 64 adds on
// distinct addresses are one cheap instruction; the one round still collapses a run of equal keys.  Every lane of the wave
// calls it (`lane` = its index in the wave); the loop is wave-uniform.
constexpr int HS_MIN_GROUP = 4;
__device__ __forceinline__ void wave_hist_add(unsigned* tab, bool hit, unsigned idx, int lane, bool once) {
  unsigned long long todo = __ballot(hit);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned lidx = __builtin_amdgcn_readlane(idx, leader);
    const unsigned long long same = todo & __ballot(idx == lidx);
    const int cnt = __popcll(same);
    if (lane == leader) atomicAdd(&tab[lidx], (unsigned)cnt);
    todo &= ~same;
    if (once || cnt < HS_MIN_GROUP) break;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&tab[idx], 1u);
}

// Every thread of the 256-thread workgroup calls it, behind a barrier after the previous segment's stream_segment_end; the
// barrier that opens the first tile publishes the state.
template <int EPI>
__device__ __forceinline__ void stream_segment_begin(const StreamLds& L, const StreamProblem& P, int row0) {
  int ts = threadIdx.x;                            // opaque: the set-up's LDS addresses are recomputed per segment instead of
  asm volatile("" : "+v"(ts));                     // occupying registers (or scratch) across the k-loops
  if constexpr (EPI == EPI_HIST) {
    for (int i = ts; i < (2 * P.cap) << P.log2cap; i += 256) L.keys[i] = 0u;
    if (ts < SQ_TM) {
      const int rr = row0 + ts;
      L.qq[ts] = rr < P.m ? P.qq[rr] : 0.f;
      L.qpid[ts] = rr < P.m ? (long long)P.q_pids[rr] : 0;
      L.qcam[ts] = rr < P.m ? (long long)P.q_cams[rr] : 0;
    }
  } else if constexpr (epi_is_topk(EPI)) {
    if (ts < SQ_TM) {
      const int rr = row0 + ts;
      L.qq[ts] = rr < P.m ? P.qq[rr] : 0.f;
      L.kmax[ts] = rr < P.m ? mono_key(P.tau[rr]) : 0u;
      if constexpr (EPI == EPI_TOPK_KEEP) {
        L.qpid[ts] = rr < P.m ? (long long)P.q_pids[rr] : 0;
        L.qcam[ts] = rr < P.m ? (long long)P.q_cams[rr] : 0;
      }
    }
  } else {
    for (int i = ts; i < SQ_TM * P.cap; i += 256) {
      const int r = i >> P.log2cap, rr = row0 + r;
      L.keys[i] = rr < P.m ? P.pos_key[(int64_t)rr * P.cap + (i & (P.cap - 1))] : 0xffffffffu;
      L.hist[i] = 0u;
    }
    if (ts < SQ_TM) {
      const int rr = row0 + ts;
      const int np = rr < P.m ? P.npos[rr] : 0;
      L.np[ts] = np > 0 ? np : 0;
      L.qq[ts] = rr < P.m ? P.qq[rr] : 0.f;
      L.qpid[ts] = rr < P.m ? (long long)P.q_pids[rr] : 0;
      L.kmax[ts] = np > 0 ? P.pos_key[(int64_t)rr * P.cap + np - 1] : 0u;
      if constexpr (EPI == EPI_BAND) L.mg[ts] = rr < P.m ? P.tau[rr] : 0.f;
    }
  }
}

// count / banded count: flushes the segment's histogram (every thread of the workgroup, after the segment's last tile);
// radix histogram: the segment's table is added to the call's, bin for bin (64-bit integers: order-independent)
template <int EPI = EPI_COUNT>
__device__ __forceinline__ void stream_segment_end(const StreamLds& L, const StreamProblem& P, int row0) {
  int ts = threadIdx.x;
  asm volatile("" : "+v"(ts));                     // opaque, as in stream_segment_begin
  __syncthreads();
  if constexpr (EPI == EPI_HIST) {
    for (int i = ts; i < (2 * P.cap) << P.log2cap; i += 256) {
      const unsigned v = L.keys[i];
      if (v) atomicAdd(&P.cand[i], (unsigned long long)v);
    }
    return;
  }
  for (int i = ts; i < SQ_TM * P.cap; i += 256) {
    const unsigned v = L.hist[i];
    const int rr = row0 + (i >> P.log2cap);
    if (v && rr < P.m) atomicAdd(&P.hist_out[(int64_t)rr * P.cap + (i & (P.cap - 1))], v);      // integer: order-independent
  }
}

// The finished tile at (row0, col0) is consumed here, in registers (row-major walk: a row's metadata is read once per NJ
// columns).  Rows beyond m multiply a clamped copy of the last query row and columns beyond n one of the last gallery row; both
// are dropped here.
//   EPI_COUNT: every NEGATIVE's distance becomes "how many positives of this query rank before it" (binary search in the
//              row's LDS positive list, ties walked by gallery index) and bumps the LDS histogram.  H accumulator rows x NJ
//              column blocks = H NJ searches in flight per lane: the search is a chain of dependent LDS reads (~100 cycles each),
//              so it is the number of INDEPENDENT chains that sets the epilogue time -- and the registers it needs.
//              skip_count & 1: timing ablation, no row has positives (results wrong).
//   EPI_TOPK : every element whose key is <= the row's threshold key takes a slot of its row's list with a global atomicAdd on
//              cand_count[row] and, while the slot is below `cap`, stores key << 32 | col there.
//   EPI_TOPK_KEEP: EPI_TOPK for the ranked lists of the evaluation protocol (utils/eval_reid.py:49-58): an element inside the
//              threshold takes its slot only if it is not junk -- the row's pid AND cam_removed for the row's camera.  The few
//              elements that pass the threshold fetch their pid, the fewer of the row's pid their camera word: the walk over
//              the other elements is EPI_TOPK's, instruction for instruction, and so are its registers.
//   EPI_BAND : the count for a distance dh known to lie within mg = L.mg[row] of the exact one d (16-bit operands, fp32 positive
//              keys: reid_metric.R1_mAP(prefilter=...)).  lo = sub_down(dh, mg) <= d <= hi = add_up(dh, mg).  key(lo) beyond the
//              row's last positive: behind every positive, skipped.  l = #positives with key < key(lo): each of them ranks before
//              the negative whatever d is.  K[l] <= key(hi): a positive lies inside the band, the pair is AMBIGUOUS and its
//              column is appended to the row's list (one global atomicAdd per half-wave and row on cand_count[row]; stored while
//              the slot is below `acap`) for creid_stream_count_rescore.  Otherwise every positive from l on ranks behind it and
//              the slot is l, as the fp32 kernel finds it.  A pair whose dh, lo or hi is not finite is ambiguous.  key(hi) is
//              formed again after the search instead of living through it: the search's registers are the count's.
//   EPI_HIST : one pass of a radix select over the keys of the pairs the evaluation protocol keeps (open-set operating points:
//              reid_metric.roc_stream).  An element of the row's pid fetches its camera word: junk counts nowhere, the others are
//              genuine (class 0); every other pid is an impostor (class 1).  For selector s the element counts when its leading
//              `acap` key bits equal pos_key[s] (always without prefix bits), in bin (key >> (32 - acap - bits)) & (2^bits - 1) of
//              the LDS table [s][class], with wave-aggregated LDS atomics (wave_hist_add).  Integers only: the
//              result does not depend on the work split or on the order of anything.
template <int EPI, int H, int NJ>
__device__ __forceinline__ void stream_tile_consume(const f32x16 (&acc)[NJ], int wm, int wn, int l31, int kh, int row0, int col0,
                                                    int skip_count, const StreamLds& L, const StreamProblem& P) {
  int rbase = wm * 32 + 4 * kh;                    // opaque per tile: the 16 rows' LDS addresses derived from it are recomputed here
  asm volatile("" : "+v"(rbase));                  // instead of living in registers (or scratch) across the k-loop
  float gv[NJ];
  [[maybe_unused]] long long gp[NJ];
  bool okc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = col0 + (wn + 2 * j) * 32 + l31;
    okc[j] = c < P.n;
    gv[j] = okc[j] ? P.gg[c] : 0.f;
    if constexpr (!epi_is_topk(EPI)) gp[j] = okc[j] ? (long long)P.g_pids[c] : 0;
  }
  if constexpr (EPI == EPI_HIST) {
    // One accumulator row at a time; a half-wave shares its row, so the 64 lanes of an aggregation hold two rows' elements.
    // (The selectors' prefixes are uniform scalar loads per element; keeping them in LDS instead changed no timing:
    // profiles/roc_stream.md.)
    const int nsel = P.cap, bits = P.log2cap, pb = P.acap;
    const int dshift = 32 - pb - bits;
    const unsigned dmask = (1u << bits) - 1u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const float qv = L.qq[rl];
      const long long qp = L.qpid[rl];
      const bool okr = row0 + rl < P.m;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const unsigned key = mono_key(fmaf(-2.0f, acc[j][r], qv + gv[j]));
        bool live = okr && okc[j];
        unsigned cls = 1u;                                           // impostor
        if (live && gp[j] == qp) {                                   // rare: the camera word is fetched for the row's pid only
          const int64_t gc = P.g_cams[col0 + (wn + 2 * j) * 32 + l31], qc = L.qcam[rl];
          cls = 0u;                                                  // genuine, unless the protocol removes it
          if (P.camsets ? cam_removed<true>(gc, qc) : cam_removed<false>(gc, qc)) live = false;
        }
        const unsigned pfx = (unsigned)((unsigned long long)key >> (32 - pb));       // 0 without prefix bits
        const unsigned bin = (key >> dshift) & dmask;
        for (int s = 0; s < nsel; ++s) {
          const unsigned want = pb ? P.pos_key[s] : 0u;              // uniform: a scalar load
          wave_hist_add(L.keys, live && pfx == want, ((2u * s + cls) << bits) | bin, l31 + 32 * kh, pb != 0);
        }
      }
    }
  } else if constexpr (epi_is_topk(EPI)) {
    // One accumulator row at a time: its threshold is one LDS read, a hit one global atomic.
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const float qv = L.qq[rl];
      const unsigned kt = L.kmax[rl];
      const bool okr = row0 + rl < P.m;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const unsigned key = mono_key(fmaf(-2.0f, acc[j][r], qv + gv[j]));
        if (okr && okc[j] && key <= kt) {
          if constexpr (EPI == EPI_TOPK_KEEP) {
            const int c = col0 + (wn + 2 * j) * 32 + l31;
            if ((long long)P.g_pids[c] == L.qpid[rl]) {              // rare: the camera word is fetched for the row's pid only
              const int64_t gc = P.g_cams[c], qc = L.qcam[rl];
              if (P.camsets ? cam_removed<true>(gc, qc) : cam_removed<false>(gc, qc)) continue;
            }
          }
          const int64_t rr = row0 + rl;
          const int slot = atomicAdd(&P.cand_count[rr], 1);
          if (slot < P.cap)
            P.cand[rr * P.cap + slot] = ((unsigned long long)key << 32) | (unsigned)(col0 + (wn + 2 * j) * 32 + l31);
        }
      }
    }
  } else if constexpr (EPI == EPI_BAND) {
    static_assert(H == 1, "one accumulator row at a time");
    unsigned* __restrict__ amb = reinterpret_cast<unsigned*>(P.cand);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = rbase + (r & 3) + 8 * (r >> 2);
      const int np = L.np[rl];
      // Uniform per wave half (a half shares its row), so the halves may diverge here.  The ballot below then sees only the active
      // lanes, every lane reads its own half of it, and the shuffle's source is the first ambiguous lane of that half: active.
      if (np == 0) continue;
      const long long qp = L.qpid[rl];
      const float qv = L.qq[rl], mg = L.mg[rl];
      const unsigned kmax = L.kmax[rl];
      const unsigned* K = L.keys + (rl << P.log2cap);
      int lo[NJ];
      unsigned key[NJ];
      bool live[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float dlo = sub_down(fmaf(-2.0f, acc[j][r], qv + gv[j]), mg);
        key[j] = mono_key(dlo);
        // not finite (then dh or hi may be so too: the test after the search): ambiguous, searched with whatever key it has
        live[j] = okc[j] && gp[j] != qp && (key[j] <= kmax || !(fabsf(dlo) <= 3.402823466e+38f));
        lo[j] = 0;
      }
      for (int step = P.cap >> 1; step > 0; step >>= 1) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) lo[j] += (K[lo[j] + step - 1] < key[j]) ? step : 0;
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        int l = lo[j];
        l += (K[l] < key[j]) ? 1 : 0;                                // l = #positives with key strictly below key(lo)
        const float dh = fmaf(-2.0f, acc[j][r], qv + gv[j]);
        const float dlo = sub_down(dh, mg), dhi = add_up(dh, mg);
        const bool fin = fabsf(dh) <= 3.402823466e+38f && fabsf(dlo) <= 3.402823466e+38f && fabsf(dhi) <= 3.402823466e+38f;
        const bool ambiguous = live[j] && (!fin || (l < np && K[l] <= mono_key(dhi)));
        if (live[j] && !ambiguous && l < np) atomicAdd(&L.hist[(rl << P.log2cap) + l], 1u);
        // the ambiguous lanes of this half-wave (one row) take their slots with one atomic
        const unsigned long long bal = __ballot(ambiguous);
        const unsigned half = kh ? (unsigned)(bal >> 32) : (unsigned)bal;
        if (ambiguous) {
          const int before = __popc(half & ((1u << l31) - 1u));
          int64_t rr = row0 + rl;
          int base = 0;
          if (before == 0) base = atomicAdd(&P.cand_count[rr], __popc(half));
          base = __shfl(base, 32 * kh + __ffs(half) - 1);
          const int slot = base + before;
          if (slot < P.acap) amb[rr * P.acap + slot] = (unsigned)(col0 + (wn + 2 * j) * 32 + l31);
        }
      }
    }
  } else {
    static_assert(16 % H == 0, "H rows at a time");
#pragma unroll
    for (int r = 0; r < 16; r += H) {
      int rl[H], np[H], lo[H][NJ];
      unsigned key[H][NJ];
      bool live[H][NJ];
      const unsigned* K[H];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        rl[h] = rbase + ((r + h) & 3) + 8 * ((r + h) >> 2);
        np[h] = (skip_count & 1) ? 0 : L.np[rl[h]];
        const long long qp = L.qpid[rl[h]];
        const float qv = L.qq[rl[h]];
        const unsigned kmax = L.kmax[rl[h]];
        K[h] = L.keys + (rl[h] << P.log2cap);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          key[h][j] = mono_key(fmaf(-2.0f, acc[j][r + h], qv + gv[j]));
          // positives / removed entries (same pid) are not counted; behind every positive: affects no rank
          live[h][j] = np[h] > 0 && okc[j] && gp[j] != qp && key[h][j] <= kmax;
          lo[h][j] = 0;
        }
      }
      if (np[0] == 0 && np[H - 1] == 0) continue;                    // uniform per wave half
      for (int step = P.cap >> 1; step > 0; step >>= 1) {
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
          l += (K[h][l] < key[h][j]) ? 1 : 0;                        // l = #positives with key strictly below
          if (live[h][j]) {
            if (l < np[h] && K[h][l] == key[h][j]) {                 // ties: by gallery index (rare)
              const int c = col0 + (wn + 2 * j) * 32 + l31;
              int rr_ = row0 + rl[h];
              asm volatile("" : "+v"(rr_));                          // keeps 16 rows' index pointers out of the k-loop's registers
              while (l < np[h] && K[h][l] == key[h][j] && P.pos_idx[(int64_t)rr_ * P.cap + l] < c) ++l;
            }
            if (l < np[h]) atomicAdd(&L.hist[(rl[h] << P.log2cap) + l], 1u);
          }
        }
    }
  }
}

// f(std::integral_constant<int, nj>{}, ...) for the tile width nj = 1 .. 4 units.  A macro on purpose: through a function that
// takes the callable, in every form tried, the register allocator spills 3-4 SGPRs in the fp32 count kernels and 1 in the 16-bit
// ones; expanded in place it spills none.
#define STREAM_DISPATCH_NJ(nj, f, ...)                                      \
  do {                                                                      \
    if ((nj) == 4) f(std::integral_constant<int, 4>{}, __VA_ARGS__);        \
    else if ((nj) == 3) f(std::integral_constant<int, 3>{}, __VA_ARGS__);   \
    else if ((nj) == 2) f(std::integral_constant<int, 2>{}, __VA_ARGS__);   \
    else f(std::integral_constant<int, 1>{}, __VA_ARGS__);                  \
  } while (0)

// ---- the positives kernels (one T-thread workgroup per query): what does not depend on how the distances are produced

// a query's lists start as padding: the count's binary search runs over all `cap` entries
template <int T>
__device__ __forceinline__ void poslist_pad(unsigned* __restrict__ okey, int32_t* __restrict__ oidx, int cap) {
  for (int i = threadIdx.x; i < cap; i += T) { okey[i] = 0xffffffffu; oidx[i] = 0x7fffffff; }
}

// The nc <= cap candidates (gallery index cand[c], distance key skey[c], both in LDS and published by a barrier) leave sorted by
// (key, gallery index): rank by counting.
template <int T>
__device__ __forceinline__ void poslist_rank_emit(const unsigned* skey, const int* cand, int nc, unsigned* __restrict__ okey,
                                                  int32_t* __restrict__ oidx, int32_t* __restrict__ npos_q) {
  for (int c = threadIdx.x; c < nc; c += T) {
    const unsigned k = skey[c];
    const int gi = cand[c];
    int pos = 0;
    for (int o = 0; o < nc; ++o) {
      const unsigned ko = skey[o];
      pos += (ko < k || (ko == k && cand[o] < gi)) ? 1 : 0;
    }
    okey[pos] = k; oidx[pos] = gi;
  }
  if (threadIdx.x == 0) *npos_q = nc;
}
