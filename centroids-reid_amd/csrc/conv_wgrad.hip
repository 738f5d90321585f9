// Stage A: convolution weight gradient  dW[n, (tap, c)] = sum_m dY[m, n] * Xg[m, (tap, c)]
// (replaces nn.Conv2d wgrad of modelling/backbones/resnet.py:56-61,94,109).
//
// Both operands are stored PIXEL-major (the reduction index m is the row index of dY and X), so
// this is a "TN" GEMM.  bf16: the tiles land in LDS exactly as they lie in memory ([pixel][channel])
// and the MFMA fragments (8 consecutive pixels of one channel per lane) come out of gfx950's
// transposing LDS read `ds_read_b64_tr_b16` -- no register or memory transpose.
//   wgrad_bf16_dma_kernel (1x1 / 3x3 layers): both tiles are fetched with the global->LDS DMA into linear
//     rows, bank conflicts avoided by an XOR swizzle of 64-byte units applied on the DMA source column; the
//     gathered operand's pixel coordinates advance incrementally (64 pixels per k-step); fragment reads run one
//     16-pixel slice ahead of the MFMAs.
//   wgrad_bf16_taps_kernel (stride-1 pad-1 3x3 layers, C_in 64..512, OW 8 / 16 / 32): one workgroup owns 64 co x 64 ci x ALL NINE
//     taps; per 128-pixel k-step the dY tile and the X halo patch enter LDS once, a tap is a per-lane slot address.  Same
//     workspace layout, its own split count (plan_wgrad_route); CREID_WGRAD_TAPS=0 puts these layers back on the kernel above.
//   wgrad_bf16_kernel (stem, span 32): register-staged 16-B stores, row pitch = tile width + 32 elements.
// f32 (parity mode): K-major LDS is the natural layout for v_mfma_f32_32x32x2_f32.
// The pixel range is split over gridDim.y workgroups; fp32 partial tiles go to the workspace and
// wgrad_reduce_kernel<SL> sums them in a fixed order (deterministic) and scatters into the OIHW fp32 gradient.
#include "conv_route.hpp"
#include <stdlib.h>
#include <atomic>

namespace {
constexpr int WKS = 64;   // pixels per k-step (bf16)
constexpr int WKF = 16;   // pixels per k-step (f32)
}

// Two MFMA fragments (channel offsets +0 / +32) x two 4-pixel halves from one base address.
// The loads are issued in one asm statement; the matching s_waitcnt statement below names every
// destination "+v" so no consumer can be scheduled before the data has landed (hipcc does not
// count inline-asm LDS reads itself).
template <int OFF_HI>
__device__ __forceinline__ void tr_load4(const unsigned short* p, s16x4& f0lo, s16x4& f0hi, s16x4& f1lo, s16x4& f1hi) {
  const unsigned addr = (unsigned)(uintptr_t)p;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %4 offset:%5\n\t"
      "ds_read_b64_tr_b16 %2, %4 offset:64\n\t"
      "ds_read_b64_tr_b16 %3, %4 offset:%6"
      : "=&v"(f0lo), "=&v"(f0hi), "=&v"(f1lo), "=&v"(f1hi)
      : "v"(addr), "i"(OFF_HI), "i"(OFF_HI + 64)
      : "memory");
}
__device__ __forceinline__ void tr_wait8(s16x4& a, s16x4& b, s16x4& c, s16x4& d, s16x4& e, s16x4& f, s16x4& g, s16x4& h) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h)::"memory");
}

template <int NW>
__device__ __forceinline__ void tr_wait8_n(s16x4& a, s16x4& b, s16x4& c, s16x4& d, s16x4& e, s16x4& f, s16x4& g, s16x4& h) {
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : "n"(NW) : "memory");
}

// s_waitcnt lgkmcnt(NW) naming the 2 * (IM + JN) destination registers of one fragment set (IM + JN transposing read pairs)
template <int NW, int IM, int JN>
__device__ __forceinline__ void tr_wait_set(s16x4 (&al)[IM], s16x4 (&ah)[IM], s16x4 (&bl)[JN], s16x4 (&bh)[JN]) {
  if constexpr (IM == 2 && JN == 2)
    asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(al[0]), "+v"(ah[0]), "+v"(al[1]), "+v"(ah[1]), "+v"(bl[0]), "+v"(bh[0]), "+v"(bl[1]), "+v"(bh[1]) : "n"(NW) : "memory");
  else if constexpr (IM == 2 && JN == 1)
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(al[0]), "+v"(ah[0]), "+v"(al[1]), "+v"(ah[1]), "+v"(bl[0]), "+v"(bh[0]) : "n"(NW) : "memory");
  else if constexpr (IM == 1 && JN == 2)
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(al[0]), "+v"(ah[0]), "+v"(bl[0]), "+v"(bh[0]), "+v"(bl[1]), "+v"(bh[1]) : "n"(NW) : "memory");
  else
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(al[0]), "+v"(ah[0]), "+v"(bl[0]), "+v"(bh[0]) : "n"(NW) : "memory");
}

template <int TM, int TN>
__global__ __launch_bounds__(256) void wgrad_bf16_kernel(IGemmGeom g, const unsigned short* __restrict__ dy,
                                                         const unsigned short* __restrict__ x, int NCO,
                                                         float* __restrict__ ws, int tiles_k, int m_per_split) {
  constexpr int PA = TM + 32, PB = TN + 32;                 // LDS row pitches (elements)
  constexpr int IM = TM / 64, JN = TN / 64;                 // MFMA tiles per wave
  constexpr int CA = TM / 8, CB = TN / 8;                   // 16-B chunks per row
  constexpr int RA = 256 / CA, RB = 256 / CB;               // rows per load pass
  constexpr int NA = WKS / RA, NBL = WKS / RB;              // load passes
  __shared__ __attribute__((aligned(16))) unsigned short Ad[WKS * PA];
  __shared__ __attribute__((aligned(16))) unsigned short Bx[WKS * PB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tile = blockIdx.x, split = blockIdx.y;
  const int tile_co = tile / tiles_k, tile_k = tile - tile_co * tiles_k;
  const int co0 = tile_co * TM, k0 = tile_k * TN;
  const int m_begin = split * m_per_split, m_end = min(g.M, m_begin + m_per_split);
  const int span_mask = (1 << g.log2span) - 1;

  // load maps
  const int a_ch = tid % CA, a_row = tid / CA;
  const int b_ch = tid % CB, b_row = tid / CB;
  const int kcol = k0 + 8 * b_ch;
  const int tap = kcol >> g.log2span, cc = kcol & span_mask;
  const int tr = tap / g.kw, ts = tap - tr * g.kw;
  // 3-deep register prefetch ring (first-class vector type so the ring stays in VGPRs)
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  struct Stage { u32x4 a[NA]; u32x4 b[NBL]; };
  Stage st0, st1, st2;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
#define WG_GLOAD(MB_, ST)                                                                                \
  do {                                                                                                   \
    const int mb_ = (MB_);                                                                               \
    _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                     \
      const int m = mb_ + a_row + RA * i;                                                                \
      ST.a[i] = (m < m_end) ? *reinterpret_cast<const u32x4*>(dy + (int64_t)m * NCO + co0 + 8 * a_ch) : zero4; \
    }                                                                                                    \
    _Pragma("unroll") for (int i = 0; i < NBL; ++i) {                                                    \
      const int m = mb_ + b_row + RB * i;                                                                \
      ST.b[i] = zero4;                                                                                   \
      if (m < m_end) {                                                                                   \
        int b, rem, oy, ox;                                                                              \
        fast_divmod(m, g.OH * g.OW, g.inv_ohow, b, rem);                                                 \
        fast_divmod(rem, g.OW, g.inv_ow, oy, ox);                                                        \
        int iy, ix;                                                                                      \
        if (igemm_src_pixel(g, oy, ox, tr, ts, iy, ix))                                                  \
          ST.b[i] = *reinterpret_cast<const u32x4*>(x + (int64_t)((b * g.SH + iy) * g.SW + ix) * g.pitch + cc); \
      }                                                                                                  \
    }                                                                                                    \
  } while (0)
#define WG_LSTORE(ST)                                                                                    \
  do {                                                                                                   \
    _Pragma("unroll") for (int i = 0; i < NA; ++i)                                                       \
      *reinterpret_cast<u32x4*>(&Ad[(a_row + RA * i) * PA + 8 * a_ch]) = ST.a[i];                        \
    _Pragma("unroll") for (int i = 0; i < NBL; ++i)                                                      \
      *reinterpret_cast<u32x4*>(&Bx[(b_row + RB * i) * PB + 8 * b_ch]) = ST.b[i];                        \
  } while (0)

  f32x16 acc[IM][JN];
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // transposing-read lane map: this lane supplies (row = 8*(lane>>5) + (li>>2) [+4q] [+16kk], col = 16*((lane>>4)&1) + 4*(li&3))
  const int li = lane & 15;
  const int t_row = 8 * (lane >> 5) + (li >> 2), t_col = 16 * ((lane >> 4) & 1) + 4 * (li & 3);

  // loads past m_end are predicated to zero, so the ring can always run 3 steps ahead
  WG_GLOAD(m_begin, st0);
  WG_GLOAD(m_begin + WKS, st1);
  WG_GLOAD(m_begin + 2 * WKS, st2);
  for (int mb = m_begin; mb < m_end; mb += WKS) {
    __syncthreads();            // previous step's fragment reads are done
    WG_LSTORE(st0);
    __syncthreads();
    st0 = st1; st1 = st2;
    WG_GLOAD(mb + 3 * WKS, st2);
#pragma unroll
    for (int kk = 0; kk < WKS / 16; ++kk) {
      s16x4 al[2], ah[2], bl[2], bh[2];
      tr_load4<4 * PA * 2>(&Ad[(kk * 16 + t_row) * PA + wm * (TM / 2) + t_col], al[0], ah[0], al[1], ah[1]);
      tr_load4<4 * PB * 2>(&Bx[(kk * 16 + t_row) * PB + wn * (TN / 2) + t_col], bl[0], bh[0], bl[1], bh[1]);
      tr_wait8(al[0], ah[0], al[1], ah[1], bl[0], bh[0], bl[1], bh[1]);
      __builtin_amdgcn_sched_barrier(0);
      s16x8 a[IM], b[JN];
#pragma unroll
      for (int i = 0; i < IM; ++i) a[i] = __builtin_shufflevector(al[i], ah[i], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
      for (int j = 0; j < JN; ++j) b[j] = __builtin_shufflevector(bl[j], bh[j], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
      for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[i]),
                                                              __builtin_bit_cast(bf16x8, b[j]), acc[i][j], 0, 0, 0);
    }
  }
#undef WG_GLOAD
#undef WG_LSTORE
  // partial tile -> workspace [split][NCO][K]
  const int l31 = lane & 31, kh = lane >> 5;
  float* wsp = ws + (int64_t)split * NCO * g.K;
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * (TM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int kc = k0 + wn * (TN / 2) + j * 32 + l31;
        wsp[(int64_t)co * g.K + kc] = acc[i][j][r];
      }
}

// ------------------------------------------------------------------------------------ bf16, LDS-DMA
// Same math as wgrad_bf16_kernel; both pixel-major tiles are fetched with the global->LDS DMA into LINEAR rows
// (pitch = tile width), double-buffered.  Bank conflicts of the transposing reads are avoided by an XOR
// swizzle of the 64-byte units of a row (key = row&3 for 256-B rows, (row>>1)&1 for 128-B rows: the four
// pixel rows a 16-lane group touches land on four different 16-bank ranges), applied on the DMA SOURCE column
// and again in the per-lane read address.  Rows past the split / out-of-image taps read a page of zeros.
__device__ __attribute__((aligned(128))) unsigned g_wgrad_zero_page[32];

template <int OFF_LO, int OFF_HI>
__device__ __forceinline__ void tr_load2(unsigned addr, s16x4& lo, s16x4& hi) {
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"
               : "=&v"(lo), "=&v"(hi) : "v"(addr), "i"(OFF_LO), "i"(OFF_HI) : "memory");
}

template <int N> __device__ __forceinline__ void wg_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// NS-stage LDS ring (see igemm_bf16_dma_kernel: with two stages the loop runs at global->LDS latency).
// WS = true: 512 threads, waves 4-7 issue the DMA (producers), waves 0-3 read fragments and multiply (consumers),
// one s_barrier per k-tile between them -- the split of igemm_bf16_ws_kernel.
// KG = 2 (non-WS): 512 threads = two k-groups of four waves.  Each group runs the whole pipeline (its own LDS ring, its own DMA
// and fragment reads) over HALF of the split's pixel range on the SAME output tile; at the end group 1 hands its accumulators to
// group 0 through LDS (fixed order: deterministic) and one partial tile leaves the CU.  Same waves per CU as two workgroups of
// a split twice as fine, half the fp32 partial-tile traffic (write here + re-read by the split reduction).
// ET = element type traits (common.hpp Bf16T / F16T): the operands move as raw 16-bit words (DMA, transposing LDS reads), so the
// element type only selects the MFMA instruction -- f16 is the reference's own mixed precision (utils/misc.py:111, precision=16)
template <int TM, int TN, int NS, bool WS = false, int KG = 1, typename ET = Bf16T>
__global__ __launch_bounds__(WS ? 512 : 256 * KG, (KG * NS * (TM + TN) * 128 <= 80 * 1024) ? ((WS || KG == 2) ? 4 : 2) : ((WS || KG == 2) ? 2 : 1)) void wgrad_bf16_dma_kernel(IGemmGeom g, const unsigned short* __restrict__ dy,
                                                                 const unsigned short* __restrict__ x, int NCO,
                                                                 float* __restrict__ ws, int tiles_k, int m_per_split,
                                                                 int xcd_tiles, int xcd_splits, BnBwdFinJob fin, int abl) {
  constexpr int IM = TM / 64, JN = TN / 64;
  constexpr int LPR_A = TM / 8, LPR_B = TN / 8;                // lanes (16-B chunks) per tile row
  constexpr int RPI_A = 64 / LPR_A, RPI_B = 64 / LPR_B;        // rows per wave-instruction
  constexpr int NIA = WKS / (4 * RPI_A), NIB = WKS / (4 * RPI_B);   // DMA instructions per wave per tile
  constexpr int TILE_A = WKS * TM, TILE_B = WKS * TN, STAGE = TILE_A + TILE_B;
  constexpr int LPT = NIA + NIB;
  static_assert((NS - 2) * LPT <= 63, "vmcnt is a 6-bit counter");
  static_assert(KG == 1 || (!WS && KG == 2 && KG * NS * STAGE * 2 <= 160 * 1024 && TM * TN * 2 <= KG * NS * STAGE), "k-groups");
  __shared__ __attribute__((aligned(1024))) unsigned short smem_all[KG * NS * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3;       // role-local wave index
  const int kg = KG > 1 ? (tid >> 8) : 0;                                    // k-group of this wave
  unsigned short* smem = smem_all + kg * NS * STAGE;                         // the group's own ring
  const bool producer = !WS || (tid >> 6) >= 4, consumer = !WS || (tid >> 6) < 4;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware split placement (xcd_tiles > 0, 1-D grid): workgroup b runs on XCD b % 8, and every XCD has its own
  // 4 MB L2.  A pixel range (split) is read by ALL tiles of the weight matrix, so all workgroups of a split go to
  // ONE XCD (split % 8 == XCD): the range's dY / X rows are fetched from HBM once and then re-read from that L2.
  // With the tile-major placement each XCD touched every pixel range and the operand re-reads (35x the unique bytes
  // for a 512 -> 512 3x3 layer) all missed to the fabric.
  // Fewer than 8 splits (xcd_splits in {1, 2, 4}): the 8 / splits XCDs that share a pixel range interleave its tiles.
  // carried job (bn_fin.hpp): the first workgroups (a multiple of 8, so the tiles keep their XCD) finalize the BatchNorm
  // backward that the NEXT launch in the stream needs; 1-D grid only
  int bid0 = (int)blockIdx.x;
  if (fin.partial) {
    const int nf8 = (fin.nblocks + 7) & ~7;
    if (bid0 < nf8) {
      if (bid0 < fin.nblocks) bn_bwd_finalize_block<WS ? 512 : 256 * KG>(fin, bid0, smem_all);
      return;
    }
    bid0 -= nf8;
  }
  int tile, split;
  if (xcd_tiles > 0 && xcd_splits >= 8) {
    const int bid = bid0, j = bid >> 3, ls = j / xcd_tiles;
    tile = j - ls * xcd_tiles;
    split = (bid & 7) + 8 * ls;
    if (split >= xcd_splits) return;
  } else if (xcd_tiles > 0) {
    const int bid = bid0, x8 = bid & 7, share = 8 / xcd_splits;
    split = x8 % xcd_splits;
    tile = x8 / xcd_splits + share * (bid >> 3);
    if (tile >= xcd_tiles) return;
  } else {
    tile = blockIdx.x; split = blockIdx.y;
  }
  const int tile_co = tile / tiles_k, tile_k = tile - tile_co * tiles_k;
  const int co0 = tile_co * TM, k0 = tile_k * TN;
  // the split's pixel range, cut into KG runs of nt k-steps (every group executes nt barriers; a run past the range reads zeros)
  const int m_begin0 = split * m_per_split, m_end0 = min(g.M, m_begin0 + m_per_split);
  const int nt = ((m_end0 - m_begin0 + WKS - 1) / WKS + KG - 1) / KG;
  const int m_begin = m_begin0 + kg * nt * WKS, m_end = min(m_end0, m_begin + nt * WKS);
  const int span_mask = (1 << g.log2span) - 1;
  const int tap = k0 >> g.log2span, cc = k0 & span_mask;
  const int tr = tap / g.kw, ts = tap - tr * g.kw;
  const unsigned short* zpage = reinterpret_cast<const unsigned short*>(g_wgrad_zero_page);

  // DMA lane maps (row within the instruction's row group, swizzled source column)
  const int ar = lane / LPR_A, aq = lane % LPR_A;
  const int br = lane / LPR_B, bq = lane % LPR_B;
  int arow[NIA], acol[NIA], brow[NIB], bcol[NIB];
#pragma unroll
  for (int i = 0; i < NIA; ++i) {
    arow[i] = (i * 4 + wave) * RPI_A + ar;
    const int key = (TM == 128) ? (arow[i] & 3) : ((arow[i] >> 1) & 1);
    acol[i] = ((((aq >> 2) ^ key) << 2) + (aq & 3)) << 3;
  }
#pragma unroll
  for (int i = 0; i < NIB; ++i) {
    brow[i] = (i * 4 + wave) * RPI_B + br;
    const int key = (TN == 128) ? (brow[i] & 3) : ((brow[i] >> 1) & 1);
    bcol[i] = ((((bq >> 2) ^ key) << 2) + (bq & 3)) << 3;
  }
  typedef const void __attribute__((address_space(1)))* gptr_t;
  typedef void __attribute__((address_space(3)))* lptr_t;
  // Pixel coordinates of this lane's B rows.  A k-step advances every row by WKS = 64 pixels: when 64 is a
  // multiple of OW (all ResNet shapes) that is "ox unchanged, oy += 64/OW, carry into the image index", a
  // handful of integer ops instead of two reciprocal divmods per DMA instruction per k-step.
  const bool inc_ok = (WKS % g.OW) == 0 && (WKS / g.OW) <= g.OH && g.check_bounds != 2;
  const int dy_rows = inc_ok ? WKS / g.OW : 0;
  int pb[NIB], poy[NIB], pox[NIB];
#pragma unroll
  for (int i = 0; i < NIB; ++i) {
    const int m = min(m_begin + brow[i], g.M - 1);
    int rem;
    fast_divmod(m, g.OH * g.OW, g.inv_ohow, pb[i], rem);
    fast_divmod(rem, g.OW, g.inv_ow, poy[i], pox[i]);
  }
  // LINEAR fast path (every 1x1 / 3x3 layer of the backbone): with 64 | OW-steps and SH == OH*stride the gathered
  // source pixel of a row advances by a CONSTANT number of elements per k-step -- image wrap included -- so both
  // operands keep running pointers (one 64-bit add per DMA instruction) and only the row's validity
  // (split end, vertical bound; the horizontal bound never changes) is re-evaluated.  PMC before this change:
  // 150 VALU + 164 SALU per k-step and wave against 16 MFMAs.
  const bool linear = inc_ok && g.log2span >= 6 && !g.transposed && g.SH == g.OH * g.stride && g.SW == g.OW * g.stride;
  const unsigned short* pa[NIA];
  const unsigned short* pbx[NIB];
  int ma[NIA], mbr[NIB], iy0[NIB];
  bool xok[NIB];
  const int a_inc = WKS * NCO, b_inc = dy_rows * g.stride * g.SW * g.pitch;
  if (linear) {
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      ma[i] = m_begin + arow[i];
      pa[i] = dy + (int64_t)ma[i] * NCO + co0 + acol[i];
    }
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      mbr[i] = m_begin + brow[i];
      int bb, rem, oy, ox;                                      // un-clamped coordinates of the (possibly virtual) row
      fast_divmod(mbr[i], g.OH * g.OW, g.inv_ohow, bb, rem);
      fast_divmod(rem, g.OW, g.inv_ow, oy, ox);
      poy[i] = oy;
      iy0[i] = tr - g.pad;                                      // iy = poy*stride + iy0
      const int ix = ox * g.stride + ts - g.pad;
      xok[i] = (unsigned)ix < (unsigned)g.SW;
      pbx[i] = x + ((int64_t)(bb * g.SH + oy * g.stride + iy0[i]) * g.SW + ix) * g.pitch + cc + bcol[i];
    }
  }
  auto issue = [&](int mb, int buf) {
    if (CREID_ABL_ON(abl, 2) && mb != m_begin) return;                      // timing ablation: only the first k-tile is fetched
    unsigned short* la = smem + buf * STAGE + wave * 512;
    unsigned short* lb = smem + buf * STAGE + TILE_A + wave * 512;
    if (linear) {
#pragma unroll
      for (int i = 0; i < NIA; ++i) {
        const unsigned short* p = (ma[i] < m_end) ? pa[i] : zpage;
        __builtin_amdgcn_global_load_lds((gptr_t)p, (lptr_t)(la + i * 2048), 16, 0, 0);
        pa[i] += a_inc; ma[i] += WKS;
      }
#pragma unroll
      for (int i = 0; i < NIB; ++i) {
        const bool ok = mbr[i] < m_end && xok[i] && (unsigned)(poy[i] * g.stride + iy0[i]) < (unsigned)g.SH;
        const unsigned short* p = ok ? pbx[i] : zpage;
        __builtin_amdgcn_global_load_lds((gptr_t)p, (lptr_t)(lb + i * 2048), 16, 0, 0);
        pbx[i] += b_inc; mbr[i] += WKS;
        poy[i] += dy_rows;
        if (poy[i] >= g.OH) poy[i] -= g.OH;
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      const int m = mb + arow[i];
      const unsigned short* p = (m < m_end) ? dy + (int64_t)m * NCO + co0 + acol[i] : zpage;
      __builtin_amdgcn_global_load_lds((gptr_t)p, (lptr_t)(la + i * 2048), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const int m = mb + brow[i];
      const unsigned short* p = zpage;
      int b, oy, ox;
      if (inc_ok) {
        b = pb[i]; oy = poy[i]; ox = pox[i];
        poy[i] += dy_rows;
        if (poy[i] >= g.OH) { poy[i] -= g.OH; ++pb[i]; }
      } else {
        int rem;
        fast_divmod(min(m, g.M - 1), g.OH * g.OW, g.inv_ohow, b, rem);
        fast_divmod(rem, g.OW, g.inv_ow, oy, ox);
      }
      if (m < m_end) {
        int iy, ix;
        if (g.log2span == 5) {
          // stem: a tap is one 32-element kernel row, so the TN-wide tile spans TN/32 taps: column col of the
          // tile row lies in kernel row tr + (col >> 5) at element (col & 31); pre-padded image, no bounds checks
          const int col = cc + bcol[i];
          p = x + (int64_t)((b * g.SH + oy * 2 + tr + (col >> 5)) * g.SW + ox * 2) * g.pitch + (col & 31);
        } else if (igemm_src_pixel(g, oy, ox, tr, ts, iy, ix))
          p = x + (int64_t)((b * g.SH + iy) * g.SW + ix) * g.pitch + cc + bcol[i];
      }
      __builtin_amdgcn_global_load_lds((gptr_t)p, (lptr_t)(lb + i * 2048), 16, 0, 0);
    }
  };

  f32x16 acc[IM][JN];
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // transposing-read lane map + swizzled per-fragment base byte addresses (relative to the stage base)
  const int li = lane & 15;
  const int t_row = 8 * (lane >> 5) + (li >> 2), t_col = 16 * ((lane >> 4) & 1) + 4 * (li & 3);
  const int keyA = (TM == 128) ? (t_row & 3) : ((t_row >> 1) & 1);
  const int keyB = (TN == 128) ? (t_row & 3) : ((t_row >> 1) & 1);
  unsigned fa[IM], fb[JN];
  const unsigned lds0 = (unsigned)(uintptr_t)smem;
#pragma unroll
  for (int i = 0; i < IM; ++i) {
    const int col = wm * (TM / 2) + i * 32 + t_col;
    fa[i] = lds0 + 2u * (unsigned)(t_row * TM + (((col >> 5) ^ keyA) << 5) + (col & 31));
  }
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const int col = wn * (TN / 2) + j * 32 + t_col;
    fb[j] = lds0 + 2u * (unsigned)(TILE_A + t_row * TN + (((col >> 5) ^ keyB) << 5) + (col & 31));
  }

  // fragment reads run one 16-pixel slice ahead of the MFMAs (two register sets): `s_waitcnt lgkmcnt(NRD)`
  // retires the older slice's NRD transposing reads while the younger slice's NRD stay in flight.  A slice reads exactly the
  // IM + JN fragments the wave multiplies (a 64-wide tile side used to be read twice: a third of the LDS read traffic of the
  // 128 x 64 tile nearly every plan picks)
  constexpr int NRD = 2 * (IM + JN);
  auto compute = [&](unsigned sb) {
    s16x4 al[2][IM], ah[2][IM], bl[2][JN], bh[2][JN];
#define WG_LOAD(KK, S)                                                                                   \
    _Pragma("unroll") for (int i = 0; i < IM; ++i)                                                       \
      tr_load2<(KK) * 16 * TM * 2, ((KK) * 16 + 4) * TM * 2>(fa[i] + sb, al[S][i], ah[S][i]);            \
    _Pragma("unroll") for (int j = 0; j < JN; ++j)                                                       \
      tr_load2<(KK) * 16 * TN * 2, ((KK) * 16 + 4) * TN * 2>(fb[j] + sb, bl[S][j], bh[S][j]);
#define WG_MMA(S, NWAIT)                                                                                 \
    {                                                                                                    \
      tr_wait_set<NWAIT, IM, JN>(al[S], ah[S], bl[S], bh[S]);                                            \
      __builtin_amdgcn_sched_barrier(0);                                                                 \
      s16x8 a[IM], b[JN];                                                                                \
      _Pragma("unroll") for (int i = 0; i < IM; ++i) a[i] = __builtin_shufflevector(al[S][i], ah[S][i], 0, 1, 2, 3, 4, 5, 6, 7); \
      _Pragma("unroll") for (int j = 0; j < JN; ++j) b[j] = __builtin_shufflevector(bl[S][j], bh[S][j], 0, 1, 2, 3, 4, 5, 6, 7); \
      if (!CREID_ABL_ON(abl, 1)) {                                                                                 \
      _Pragma("unroll") for (int i = 0; i < IM; ++i)                                                     \
        _Pragma("unroll") for (int j = 0; j < JN; ++j)                                                   \
          acc[i][j] = ET::mfma(a[i], b[j], acc[i][j]);                                                   \
      }                                                                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                                 \
    }
    if (CREID_ABL_ON(abl, 4)) return;                                                                                 
    WG_LOAD(0, 0)
    WG_LOAD(1, 1) WG_MMA(0, NRD)
    WG_LOAD(2, 0) WG_MMA(1, NRD)
    WG_LOAD(3, 1) WG_MMA(0, NRD)
    WG_MMA(1, 0)
#undef WG_LOAD
#undef WG_MMA
  };
  if constexpr (!WS) {
#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
      if (p < nt) issue(m_begin + p * WKS, p);
    int buf = 0;
    for (int t = 0; t < nt; ++t) {
      const int younger = min(nt - 1 - t, NS - 2);
      if constexpr (NS >= 5) { if (younger == 3) wg_wait_vm<3 * LPT>(); }
      if constexpr (NS >= 4) { if (younger == 2) wg_wait_vm<2 * LPT>(); }
      if constexpr (NS >= 3) { if (younger == 1) wg_wait_vm<1 * LPT>(); }
      if (younger == 0) wg_wait_vm<0>();
      asm volatile("s_barrier" ::: "memory");     // bare barrier: a fence would drain the whole ring (vmcnt 0)
      if (t + NS - 1 < nt) issue(m_begin + (t + NS - 1) * WKS, buf == 0 ? NS - 1 : buf - 1);
      compute((unsigned)(buf * STAGE * 2));
      buf = (buf + 1 == NS) ? 0 : buf + 1;
    }
  } else if (producer) {                            // separate loops: the two roles' registers never coexist
#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
      if (p < nt) issue(m_begin + p * WKS, p);
    int buf = 0;
    for (int t = 0; t < nt; ++t) {
      const int younger = min(nt - 1 - t, NS - 2);
      if constexpr (NS >= 3) { if (younger == 1) wg_wait_vm<1 * LPT>(); }
      if (younger == 0) wg_wait_vm<0>();
      asm volatile("s_barrier" ::: "memory");
      if (t + NS - 1 < nt) issue(m_begin + (t + NS - 1) * WKS, buf == 0 ? NS - 1 : buf - 1);
      buf = (buf + 1 == NS) ? 0 : buf + 1;
    }
    return;
  } else {
    int buf = 0;
    for (int t = 0; t < nt; ++t) {
      asm volatile("s_barrier" ::: "memory");
      compute((unsigned)(buf * STAGE * 2));
      buf = (buf + 1 == NS) ? 0 : buf + 1;
    }
  }
  if constexpr (KG > 1) {
    __syncthreads();                                             // both rings are dead
    float* ex = reinterpret_cast<float*>(smem_all);
    const int t256 = tid & 255;
    if (kg == 1) {
#pragma unroll
      for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) ex[((i * JN + j) * 16 + r) * 256 + t256] = acc[i][j][r];
    }
    __syncthreads();
    if (kg == 1) return;
#pragma unroll
    for (int i = 0; i < IM; ++i)
#pragma unroll
      for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] += ex[((i * JN + j) * 16 + r) * 256 + t256];
  }
  const int l31 = lane & 31, kh = lane >> 5;
  float* wsp = ws + (int64_t)split * NCO * g.K;
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * (TM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int kc = k0 + wn * (TN / 2) + j * 32 + l31;
        wsp[(int64_t)co * g.K + kc] = acc[i][j][r];
      }
}

// ------------------------------------------------------------------------------------ bf16 / f16, nine taps per workgroup
// Stride-1 pad-1 3x3 layers.  wgrad_bf16_dma_kernel gives every workgroup one (co-tile, tap x ci-tile) output tile, so the dY tile
// of a pixel range is DMA'd by nine times as many workgroups as a 1x1 layer of the same width needs and the X tile is fetched nine
// times under one-pixel shifts.  Here ONE workgroup owns (64 co x 64 ci x all nine taps) over its pixel range: per 128-pixel k-step
// (whole image rows of one image) the dY tile [128][64] enters LDS once and so does the X HALO patch of the same pixels -- output
// rows + 2, OW + 2 slots of 64 channels each, out-of-image slots fetched from the zero page.  Every 16-pixel slice's dY fragment
// is read from LDS once and multiplied against nine X fragments: a tap (r, s) is only another per-lane slot address,
//   slot(pixel p, r, s) = (p / OW + r) * (OW + 2) + p % OW + s.
// Rows are 128 bytes; the 64-byte-unit XOR key of a row / slot is (index >> 1) & 1, applied on the DMA source column and again in
// the read address: four CONSECUTIVE slots -- what a 16-lane group of a transposing read touches, whatever the tap's shift -- land
// on four different 16-bank ranges.  512 threads = two k-groups of four waves over ONE ring: a group multiplies four of a step's
// eight slices, each of its waves holding a 32 x 32 tile of all nine taps (144 accumulator registers, two waves per SIMD), and
// the groups' accumulators are merged through LDS before the store -- half the partial tiles of a split twice as fine.
// Fragment reads run one UNIT (three taps of one slice: 6 or 8 transposing reads) ahead of the MFMAs, so the 4-bit lgkmcnt
// suffices.  Partial tiles go to the workspace [split][NCO][K = 9 * C_in] (tap-major columns), i.e. the layout of the tile kernels:
// the split reductions are shared.  1-D grid, all tiles of a pixel range on one XCD; the first workgroups carry the BatchNorm job.
constexpr int TPK = 128;   // pixels per k-step (tap-fused kernel): split lengths are multiples of it

template <int OW>
struct TapsGeom {
  static constexpr int ROWS = TPK / OW, HP = OW + 2, NSLOT = (ROWS + 2) * HP;   // halo patch of a k-step: rows x slots per row
  static constexpr int NIH = (NSLOT + 63) / 64;                                 // halo DMA instructions per wave (8 slots each, 8 waves)
  static constexpr int TILE_A = TPK * 64, STAGE = TILE_A + NIH * 64 * 64;       // elements
  static constexpr int slice_slot(int kk) { return kk * 16 + 2 * ((kk * 16) / OW); }   // first halo slot of 16-pixel slice kk
};

template <int NW>
__device__ __forceinline__ void tr_wait_unit(s16x4& al, s16x4& ah, s16x4 (&bl)[3], s16x4 (&bh)[3]) {
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(al), "+v"(ah), "+v"(bl[0]), "+v"(bh[0]), "+v"(bl[1]), "+v"(bh[1]), "+v"(bl[2]), "+v"(bh[2]) : "n"(NW) : "memory");
}

// fragment reads of unit U = (slice U / 3, taps 3 * (U % 3) ..+2): the slice's dY fragment with its first tap group
template <int OW, int U>
__device__ __forceinline__ void taps_load_unit(unsigned fa, const unsigned (&fb)[9], unsigned sb, s16x4 (&al)[2], s16x4 (&ah)[2],
                                               s16x4 (&bl)[2][3], s16x4 (&bh)[2][3]) {
  constexpr int KK = U / 3, G = U % 3, S = TapsGeom<OW>::slice_slot(KK), FLIP = ((S >> 1) & 1) * 64;
  if constexpr (G == 0) tr_load2<KK * 16 * 128, (KK * 16 + 4) * 128>(fa + sb, al[KK & 1], ah[KK & 1]);
#pragma unroll
  for (int j = 0; j < 3; ++j) tr_load2<S * 128, (S + 4) * 128>((fb[3 * G + j] ^ (unsigned)FLIP) + sb, bl[U & 1][j], bh[U & 1][j]);
}

template <int OW, typename ET, int U>
__device__ __forceinline__ void taps_unit(unsigned fa, const unsigned (&fb)[9], unsigned sb, s16x4 (&al)[2], s16x4 (&ah)[2],
                                          s16x4 (&bl)[2][3], s16x4 (&bh)[2][3], f32x16 (&acc)[9]) {
  constexpr int NU = 3 * (TPK / 32), KK = U / 3, G = U % 3;           // a k-group multiplies four of a step's eight slices
  if constexpr (U + 1 < NU) {
    taps_load_unit<OW, U + 1>(fa, fb, sb, al, ah, bl, bh);
    tr_wait_unit<((U + 1) % 3 == 0) ? 8 : 6>(al[KK & 1], ah[KK & 1], bl[U & 1], bh[U & 1]);
  } else {
    tr_wait_unit<0>(al[KK & 1], ah[KK & 1], bl[U & 1], bh[U & 1]);
  }
  __builtin_amdgcn_sched_barrier(0);
  const s16x8 a = __builtin_shufflevector(al[KK & 1], ah[KK & 1], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const s16x8 b = __builtin_shufflevector(bl[U & 1][j], bh[U & 1][j], 0, 1, 2, 3, 4, 5, 6, 7);
    acc[3 * G + j] = ET::mfma(a, b, acc[3 * G + j]);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (U + 1 < NU) taps_unit<OW, ET, U + 1>(fa, fb, sb, al, ah, bl, bh, acc);
}

template <int OW, typename ET>
__global__ __launch_bounds__(512, 2) void wgrad_bf16_taps_kernel(const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
                                                                  int M, int OH, int CIN, int NCO, float* __restrict__ ws, int tiles,
                                                                  int tiles_ci, int splits, int m_per_split, BnBwdFinJob fin) {
  using G = TapsGeom<OW>;
  constexpr int NS = 3, NIA = TPK / 64, NIH = G::NIH, LPT = NIA + NIH, STAGE = G::STAGE;
  static_assert(NS * STAGE * 2 <= 160 * 1024 && (NS - 2) * LPT <= 63 && (G::slice_slot(7) + 4) * 128 < 65536, "LDS ring / vmcnt / ds offset");
  // k-group 1 reads slices 4..7 through k-group 0's immediate offsets: same swizzle flips, one constant slot distance
  static_assert(((G::slice_slot(4) >> 1) & 1) == 0 && G::slice_slot(5) - G::slice_slot(1) == G::slice_slot(4) &&
                G::slice_slot(6) - G::slice_slot(2) == G::slice_slot(4) && G::slice_slot(7) - G::slice_slot(3) == G::slice_slot(4), "k-groups");
  static_assert(5 * 16 * 256 * 4 <= NS * STAGE * 2, "accumulator exchange");
  __shared__ __attribute__((aligned(1024))) unsigned short smem[NS * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;          // 8 waves: all issue the DMA
  const int kg = wave >> 2, wm = (wave >> 1) & 1, wn = wave & 1;            // k-group; the wave's 32 x 32 corner of the 64 x 64 tile
  // carried job (bn_fin.hpp), as in wgrad_bf16_dma_kernel: the first workgroups (a multiple of 8, so the tiles keep their XCD);
  // 256 of the threads, so that the sums have the grouping -- the bits -- of the stand-alone launch
  int bid0 = (int)blockIdx.x;
  if (fin.partial) {
    const int nf8 = (fin.nblocks + 7) & ~7;
    if (bid0 < nf8) {
      if (bid0 < fin.nblocks) bn_bwd_finalize_block<256>(fin, bid0, smem, tid < 256);
      return;
    }
    bid0 -= nf8;
  }
  // XCD placement of wgrad_bf16_dma_kernel: workgroup b runs on XCD b % 8; all tiles of a pixel range (split) go to one XCD, or,
  // with 1 / 2 / 4 splits, to the 8 / splits XCDs that share the range
  int tile, split;
  if (splits >= 8 || (8 % splits) != 0) {
    const int j = bid0 >> 3, ls = j / tiles;
    tile = j - ls * tiles;
    split = (bid0 & 7) + 8 * ls;
    if (split >= splits) return;
  } else {
    const int x8 = bid0 & 7, share = 8 / splits;
    split = x8 % splits;
    tile = x8 / splits + share * (bid0 >> 3);
    if (tile >= tiles) return;
  }
  const int tile_co = tile / tiles_ci, tile_ci = tile - tile_co * tiles_ci;
  const int co0 = tile_co * 64, ci0 = tile_ci * 64;
  // M and the split length are multiples of TPK and a k-step never leaves its image (OH * OW % TPK == 0): every step is whole
  const int m_begin = split * m_per_split, m_end = min(M, m_begin + m_per_split);
  const int nt = (m_end - m_begin) / TPK;
  const unsigned short* zpage = reinterpret_cast<const unsigned short*>(g_wgrad_zero_page);

  // DMA lane maps: 8 lanes (16-B chunks) per 128-byte row, a wave instruction covers 8 rows / slots; swizzled source column
  const int dr = lane >> 3, dq = lane & 7;
  const unsigned short* pa[NIA];
#pragma unroll
  for (int i = 0; i < NIA; ++i) {
    const int row = (i * 8 + wave) * 8 + dr, key = (row >> 1) & 1;
    pa[i] = dy + (int64_t)(m_begin + row) * NCO + co0 + (((((dq >> 2) ^ key) << 2) + (dq & 3)) << 3);
  }
  // halo slot t = (hr, hx) holds the source pixel (oy0 - 1 + hr, hx - 1) of the step's image: relative to the step's first pixel
  // that is (hr - 1) * OW + hx - 1 pixels away, the same for every step; only the vertical bound moves with oy0
  int hoff[NIH], hrow[NIH];
#pragma unroll
  for (int i = 0; i < NIH; ++i) {
    const int t = (i * 8 + wave) * 8 + dr, hr = t / G::HP, hx = t - hr * G::HP, key = (t >> 1) & 1;
    const bool xok = t < G::NSLOT && hx >= 1 && hx <= OW;
    hrow[i] = xok ? hr - 1 : (1 << 20);                                  // (a slot never filled fails the row test below)
    hoff[i] = ((hr - 1) * OW + hx - 1) * CIN + ci0 + (((((dq >> 2) ^ key) << 2) + (dq & 3)) << 3);
  }
  const unsigned short* xs = x + (int64_t)m_begin * CIN;                   // the issued step's first pixel
  int oy0 = (m_begin % (OH * OW)) / OW;                                    // and its image row
  typedef const void __attribute__((address_space(1)))* gptr_t;
  typedef void __attribute__((address_space(3)))* lptr_t;
  auto issue = [&](int buf) {
    unsigned short* la = smem + buf * STAGE + wave * 512;
    unsigned short* lh = la + G::TILE_A;
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      __builtin_amdgcn_global_load_lds((gptr_t)pa[i], (lptr_t)(la + i * 4096), 16, 0, 0);
      pa[i] += (int64_t)TPK * NCO;
    }
#pragma unroll
    for (int i = 0; i < NIH; ++i) {
      const unsigned short* p = ((unsigned)(oy0 + hrow[i]) < (unsigned)OH) ? xs + hoff[i] : zpage;
      __builtin_amdgcn_global_load_lds((gptr_t)p, (lptr_t)(lh + i * 4096), 16, 0, 0);
    }
    xs += (int64_t)TPK * CIN;
    oy0 += G::ROWS;
    if (oy0 >= OH) oy0 = 0;
  };

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // transposing-read lane map (wgrad_bf16_dma_kernel) and the per-tap halo slot of this lane's pixel row
  const int li = lane & 15;
  const int t_row = 8 * (lane >> 5) + (li >> 2), t_col = 16 * ((lane >> 4) & 1) + 4 * (li & 3);
  const unsigned lds0 = (unsigned)(uintptr_t)smem;
  const int cola = wm * 32 + t_col, colb = wn * 32 + t_col;
  const unsigned fa = lds0 + 2u * (unsigned)((kg * 64 + t_row) * 64 + (((cola >> 5) ^ ((t_row >> 1) & 1)) << 5) + (cola & 31));
  const int slot0 = t_row + 2 * (t_row / OW) + kg * G::slice_slot(4);
  unsigned fb[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int slot = slot0 + (t / 3) * G::HP + (t % 3);
    fb[t] = lds0 + 2u * (unsigned)(G::TILE_A + slot * 64 + (((colb >> 5) ^ ((slot >> 1) & 1)) << 5) + (colb & 31));
  }
  auto compute = [&](unsigned sb) {
    s16x4 al[2], ah[2], bl[2][3], bh[2][3];
    taps_load_unit<OW, 0>(fa, fb, sb, al, ah, bl, bh);
    taps_unit<OW, ET, 0>(fa, fb, sb, al, ah, bl, bh, acc);
  };
#pragma unroll
  for (int p = 0; p < NS - 1; ++p)
    if (p < nt) issue(p);
  int buf = 0;
  for (int t = 0; t < nt; ++t) {
    const int younger = min(nt - 1 - t, NS - 2);
    if (younger == 1) wg_wait_vm<LPT>(); else wg_wait_vm<0>();
    asm volatile("s_barrier" ::: "memory");     // bare barrier: a fence would drain the whole ring (vmcnt 0)
    if (t + NS - 1 < nt) issue(buf == 0 ? NS - 1 : buf - 1);
    compute((unsigned)(buf * STAGE * 2));
    buf = (buf + 1 == NS) ? 0 : buf + 1;
  }
  // k-group 1 hands its accumulators to k-group 0 through LDS (five taps, then four: the ring is dead and holds 80 KB of them);
  // fixed order, so the result is deterministic, and ONE set of partial tiles leaves the CU
  {
    float* ex = reinterpret_cast<float*>(smem);
    const int t256 = tid & 255;
#pragma unroll
    for (int t0 = 0; t0 < 9; t0 += 5) {
      __syncthreads();
      if (kg == 1) {
#pragma unroll
        for (int t = t0; t < (t0 == 0 ? 5 : 9); ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) ex[((t - t0) * 16 + r) * 256 + t256] = acc[t][r];
      }
      __syncthreads();
      if (kg == 0) {
#pragma unroll
        for (int t = t0; t < (t0 == 0 ? 5 : 9); ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] += ex[((t - t0) * 16 + r) * 256 + t256];
      }
    }
    if (kg == 1) return;
  }
  // partial tiles -> workspace [split][NCO][K], column = tap * C_in + ci
  const int l31 = lane & 31, kh = lane >> 5, K = 9 * CIN;
  float* wsp = ws + ((int64_t)split * NCO + co0 + wm * 32 + 4 * kh) * K + ci0 + wn * 32 + l31;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) wsp[(int64_t)((r & 3) + 8 * (r >> 2)) * K + t * CIN] = acc[t][r];
}

template <int TM, int TN>
__global__ __launch_bounds__(256) void wgrad_f32_kernel(IGemmGeom g, const float* __restrict__ dy,
                                                        const float* __restrict__ x, int NCO, float* __restrict__ ws,
                                                        int tiles_k, int m_per_split) {
  constexpr int IM = TM / 64, JN = TN / 64;
  constexpr int CA = TM / 4, CB = TN / 4;
  constexpr int RA = 256 / CA, RB = 256 / CB;
  constexpr int NA = (WKF + RA - 1) / RA, NBL = (WKF + RB - 1) / RB;
  __shared__ __attribute__((aligned(16))) float Ad[WKF][TM];
  __shared__ __attribute__((aligned(16))) float Bx[WKF][TN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tile = blockIdx.x, split = blockIdx.y;
  const int tile_co = tile / tiles_k, tile_k = tile - tile_co * tiles_k;
  const int co0 = tile_co * TM, k0 = tile_k * TN;
  const int m_begin = split * m_per_split, m_end = min(g.M, m_begin + m_per_split);
  const int span_mask = (1 << g.log2span) - 1;
  const int a_ch = tid % CA, a_row = tid / CA;
  const int b_ch = tid % CB, b_row = tid / CB;
  const int kcol = k0 + 4 * b_ch;
  const int tap = kcol >> g.log2span, cc = kcol & span_mask;
  const int tr = tap / g.kw, ts = tap - tr * g.kw;
  float4 ra[NA], rb[NBL];
  auto gload = [&](int mb) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int pr = a_row + RA * i, m = mb + pr;
      ra[i] = (pr < WKF && m < m_end) ? *reinterpret_cast<const float4*>(dy + (int64_t)m * NCO + co0 + 4 * a_ch)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const int pr = b_row + RB * i, m = mb + pr;
      rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pr < WKF && m < m_end) {
        const int b = m / (g.OH * g.OW), rem = m - b * (g.OH * g.OW);
        const int oy = rem / g.OW, ox = rem - oy * g.OW;
        int iy, ix;
        if (igemm_src_pixel(g, oy, ox, tr, ts, iy, ix))
          rb[i] = *reinterpret_cast<const float4*>(x + (int64_t)((b * g.SH + iy) * g.SW + ix) * g.pitch + cc);
      }
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i)
      if (a_row + RA * i < WKF) *reinterpret_cast<float4*>(&Ad[a_row + RA * i][4 * a_ch]) = ra[i];
#pragma unroll
    for (int i = 0; i < NBL; ++i)
      if (b_row + RB * i < WKF) *reinterpret_cast<float4*>(&Bx[b_row + RB * i][4 * b_ch]) = rb[i];
  };
  f32x16 acc[IM][JN];
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int l31 = lane & 31, kh = lane >> 5;
  gload(m_begin);
  for (int mb = m_begin; mb < m_end; mb += WKF) {
    __syncthreads();
    lstore();
    __syncthreads();
    if (mb + WKF < m_end) gload(mb + WKF);
#pragma unroll
    for (int kk = 0; kk < WKF; kk += 2) {
      float a[IM], b[JN];
#pragma unroll
      for (int i = 0; i < IM; ++i) a[i] = Ad[kk + kh][wm * (TM / 2) + i * 32 + l31];
#pragma unroll
      for (int j = 0; j < JN; ++j) b[j] = Bx[kk + kh][wn * (TN / 2) + j * 32 + l31];
#pragma unroll
      for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  float* wsp = ws + (int64_t)split * NCO * g.K;
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * (TM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int kc = k0 + wn * (TN / 2) + j * 32 + l31;
        wsp[(int64_t)co * g.K + kc] = acc[i][j][r];
      }
}

// ------------------------------------------------------------------------------------ bf16x3
// fp32-grade weight gradient on the bf16 matrix pipe (CREID_BF16X3, see conv_x3.hip).  Both fp32 operands are split into
// (hi, lo) bf16 planes while a 32-pixel k-tile is written to LDS pixel-major -- the layout of wgrad_bf16_kernel, so the
// fragments (8 consecutive pixels of one channel per lane) come out of the same transposing reads -- and every product is
// lo*hi + hi*lo + hi*hi with fp32 accumulation.  Grid, pixel splits and the [split][NCO][K] fp32 partial tiles are exactly
// those of wgrad_f32_kernel under plan_wgrad(..., CREID_F32): the CREID_F32 reduce paths sum them.  The k order of every
// partial is fixed by the shape (pixel order inside one split, then the three terms), so results are deterministic.
constexpr int WKX = 32;   // pixels per k-step (bf16x3)

template <int TM, int TN>
__global__ __launch_bounds__(256) void wgrad_x3_kernel(IGemmGeom g, const float* __restrict__ dy, const float* __restrict__ x,
                                                       int NCO, float* __restrict__ ws, int tiles_k, int m_per_split) {
  constexpr int PA = TM + 32, PB = TN + 32;                 // LDS row pitches (elements), as wgrad_bf16_kernel
  constexpr int IM = TM / 64, JN = TN / 64;                 // MFMA tiles per wave
  constexpr int CA = TM / 4, CB = TN / 4;                   // float4 chunks per row
  constexpr int RA = 256 / CA, RB = 256 / CB;               // rows per load pass
  constexpr int NA = WKX / RA, NBL = WKX / RB;              // load passes
  // [pixel][channel] bf16, hi and lo planes of both operands
  __shared__ __attribute__((aligned(16))) unsigned short Ah[WKX * PA], Al[WKX * PA], Bh[WKX * PB], Bl[WKX * PB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tile = blockIdx.x, split = blockIdx.y;
  const int tile_co = tile / tiles_k, tile_k = tile - tile_co * tiles_k;
  const int co0 = tile_co * TM, k0 = tile_k * TN;
  const int m_begin = split * m_per_split, m_end = min(g.M, m_begin + m_per_split);
  const int span_mask = (1 << g.log2span) - 1;
  const int a_ch = tid % CA, a_row = tid / CA;
  const int b_ch = tid % CB, b_row = tid / CB;
  const int kcol = k0 + 4 * b_ch;                           // a 4-channel chunk never straddles two taps (span >= 64)
  const int tap = kcol >> g.log2span, cc = kcol & span_mask;
  const int tr = tap / g.kw, ts = tap - tr * g.kw;
  float4 ra[NA], rb[NBL];
  auto gload = [&](int mb) {                                // rows past the split or outside the image stage zeros
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int m = mb + a_row + RA * i;
      ra[i] = (m < m_end) ? *reinterpret_cast<const float4*>(dy + (int64_t)m * NCO + co0 + 4 * a_ch) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const int m = mb + b_row + RB * i;
      rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < m_end) {
        int b, rem, oy, ox, iy, ix;
        fast_divmod(m, g.OH * g.OW, g.inv_ohow, b, rem);
        fast_divmod(rem, g.OW, g.inv_ow, oy, ox);
        if (igemm_src_pixel(g, oy, ox, tr, ts, iy, ix))
          rb[i] = *reinterpret_cast<const float4*>(x + (int64_t)((b * g.SH + iy) * g.SW + ix) * g.pitch + cc);
      }
    }
  };
  auto split4 = [](const float4& v, unsigned short* hp, unsigned short* lp) {
    const unsigned h0 = f32x2_to_bf16x2_bits(v.x, v.y), h1 = f32x2_to_bf16x2_bits(v.z, v.w);
    const unsigned l0 = f32x2_to_bf16x2_bits(v.x - __uint_as_float(h0 << 16), v.y - __uint_as_float(h0 & 0xffff0000u));
    const unsigned l1 = f32x2_to_bf16x2_bits(v.z - __uint_as_float(h1 << 16), v.w - __uint_as_float(h1 & 0xffff0000u));
    *reinterpret_cast<uint2*>(hp) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(lp) = make_uint2(l0, l1);
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int o = (a_row + RA * i) * PA + 4 * a_ch;
      split4(ra[i], &Ah[o], &Al[o]);
    }
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const int o = (b_row + RB * i) * PB + 4 * b_ch;
      split4(rb[i], &Bh[o], &Bl[o]);
    }
  };
  f32x16 acc[IM][JN];
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // transposing-read lane map of wgrad_bf16_kernel
  const int li = lane & 15;
  const int t_row = 8 * (lane >> 5) + (li >> 2), t_col = 16 * ((lane >> 4) & 1) + 4 * (li & 3);
  gload(m_begin);
  for (int mb = m_begin; mb < m_end; mb += WKX) {
    __syncthreads();            // previous step's fragment reads are done
    lstore();
    __syncthreads();
    if (mb + WKX < m_end) gload(mb + WKX);
#pragma unroll
    for (int kk = 0; kk < WKX / 16; ++kk) {
      // [fragment 0 | 1] x [pixels 0..3 | 4..7] of each plane
      s16x4 ah0[2], ah1[2], bh0[2], bh1[2], al0[2], al1[2], bl0[2], bl1[2];
      const int ao = (kk * 16 + t_row) * PA + wm * (TM / 2) + t_col, bo = (kk * 16 + t_row) * PB + wn * (TN / 2) + t_col;
      tr_load4<4 * PA * 2>(&Ah[ao], ah0[0], ah1[0], ah0[1], ah1[1]);
      tr_load4<4 * PB * 2>(&Bh[bo], bh0[0], bh1[0], bh0[1], bh1[1]);
      tr_load4<4 * PA * 2>(&Al[ao], al0[0], al1[0], al0[1], al1[1]);
      tr_load4<4 * PB * 2>(&Bl[bo], bl0[0], bl1[0], bl0[1], bl1[1]);
      tr_wait8(ah0[0], ah1[0], ah0[1], ah1[1], bh0[0], bh1[0], bh0[1], bh1[1]);
      tr_wait8(al0[0], al1[0], al0[1], al1[1], bl0[0], bl1[0], bl0[1], bl1[1]);
      __builtin_amdgcn_sched_barrier(0);
      s16x8 ah[IM], al[IM], bh[JN], bl[JN];
#pragma unroll
      for (int i = 0; i < IM; ++i) {
        ah[i] = __builtin_shufflevector(ah0[i], ah1[i], 0, 1, 2, 3, 4, 5, 6, 7);
        al[i] = __builtin_shufflevector(al0[i], al1[i], 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < JN; ++j) {
        bh[j] = __builtin_shufflevector(bh0[j], bh1[j], 0, 1, 2, 3, 4, 5, 6, 7);
        bl[j] = __builtin_shufflevector(bl0[j], bl1[j], 0, 1, 2, 3, 4, 5, 6, 7);
      }
      // small terms first, interleaved over the wave's fragments (conv_x3.hip)
#pragma unroll
      for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) acc[i][j] = Bf16T::mfma(al[i], bh[j], acc[i][j]);
#pragma unroll
      for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) acc[i][j] = Bf16T::mfma(ah[i], bl[j], acc[i][j]);
#pragma unroll
      for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) acc[i][j] = Bf16T::mfma(ah[i], bh[j], acc[i][j]);
    }
  }
  const int l31 = lane & 31, kh = lane >> 5;
  float* wsp = ws + (int64_t)split * NCO * g.K;
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * (TM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int kc = k0 + wn * (TN / 2) + j * 32 + l31;
        wsp[(int64_t)co * g.K + kc] = acc[i][j][r];
      }
}

// sum over splits and scatter [NCO][K = (tap, within)] -> OIHW fp32 gradient (accumulating).
// r = tap / kw_taps; s = tap % kw_taps + within / cpitch; c = within % cpitch.
// Workgroup = (256/SL) float4 element groups x SL split lanes: every thread streams its 16-byte column slice
// through the splits it owns (4 loads in flight), the SL partial sums meet in LDS in a FIXED order
// (deterministic), and lane 0 of each group writes the four results.  The host picks SL from the split count
// so that the per-thread loop stays <= ~8 deep whether a layer has 4 splits of a 2.4M-element tensor or 512
// splits of a 4096-element one.
template <int SL>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int NCO, int K,
                                                           int log2span, int kw_taps, int cpitch, int cin, int kh,
                                                           int kw, float* __restrict__ dw_oihw, int accumulate) {
  constexpr int EG = 256 / SL;
  __shared__ float4 red[SL > 1 ? SL : 1][EG];
  const int64_t total = (int64_t)NCO * K, total4 = total >> 2;      // K % 64 == 0
  const int eg = threadIdx.x % EG, sl = threadIdx.x / EG;
  const int64_t i4 = (int64_t)blockIdx.x * EG + eg;
  const bool live = i4 < total4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float4* p = reinterpret_cast<const float4*>(ws) + i4;
    int sp = sl;
    for (; sp + 3 * SL < splits; sp += 4 * SL) {
      const float4 a = p[(int64_t)sp * total4], b = p[(int64_t)(sp + SL) * total4];
      const float4 c = p[(int64_t)(sp + 2 * SL) * total4], d = p[(int64_t)(sp + 3 * SL) * total4];
      acc.x += (a.x + b.x) + (c.x + d.x); acc.y += (a.y + b.y) + (c.y + d.y);
      acc.z += (a.z + b.z) + (c.z + d.z); acc.w += (a.w + b.w) + (c.w + d.w);
    }
    for (; sp < splits; sp += SL) {
      const float4 a = p[(int64_t)sp * total4];
      acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    }
  }
  if constexpr (SL > 1) {
    red[sl][eg] = acc;
    __syncthreads();
    if (sl != 0) return;
#pragma unroll
    for (int q = 1; q < SL; ++q) { const float4 v = red[q][eg]; acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
  }
  if (!live) return;
  const int64_t i = i4 << 2;
  if (kh == 1 && kw == 1 && cpitch == cin && (1 << log2span) == cin &&
      (reinterpret_cast<uintptr_t>(dw_oihw) & 15) == 0) {                  // 1x1: OIHW == [co][c], same index
    float4* dst = reinterpret_cast<float4*>(dw_oihw + i);
    if (accumulate) { const float4 o = *dst; acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w; }
    *dst = acc;
    return;
  }
  const int span_mask = (1 << log2span) - 1;
  const int co = (int)(i / K), kc0 = (int)(i - (int64_t)co * K);
  const float v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int kc = kc0 + e;
    const int tap = kc >> log2span, within = kc & span_mask;
    const int r = tap / kw_taps, s = tap % kw_taps + within / cpitch, c = within % cpitch;
    if (r < kh && s < kw && c < cin) {
      float* dst = dw_oihw + (((int64_t)co * cin + c) * kh + r) * kw + s;
      *dst = accumulate ? *dst + v[e] : v[e];
    }
  }
}

// 3x3 layers with few splits: one workgroup per output channel.  The partial row [tap][c] (K floats, contiguous) is
// summed over the splits with coalesced reads, transposed to OIHW's [c][tap] order in LDS, and leaves as ONE
// contiguous K-float run (the generic kernel writes those 4-byte values 36 bytes apart).
__global__ __launch_bounds__(256) void wgrad_reduce_taps_kernel(const float* __restrict__ ws, int splits, int NCO, int K,
                                                                int cin, int taps, float* __restrict__ dw_oihw,
                                                                int accumulate) {
  extern __shared__ float tr_lds[];                              // [K] in (c, tap) order
  const int co = blockIdx.x;
  const int64_t total = (int64_t)NCO * K;
  const float* src = ws + (int64_t)co * K;
  for (int e = threadIdx.x; e < K; e += 256) {
    float a0 = 0.f, a1 = 0.f;
    int sp = 0;
    for (; sp + 1 < splits; sp += 2) { a0 += src[(int64_t)sp * total + e]; a1 += src[(int64_t)(sp + 1) * total + e]; }
    if (sp < splits) a0 += src[(int64_t)sp * total + e];
    const int tap = e / cin, c = e - tap * cin;
    tr_lds[c * taps + tap] = a0 + a1;
  }
  __syncthreads();
  float* dst = dw_oihw + (int64_t)co * K;
  for (int e = threadIdx.x; e < K; e += 256) dst[e] = accumulate ? dst[e] + tr_lds[e] : tr_lds[e];
}

// ------------------------------------------------------------------------------------ host
int wgrad_dma_env() { static const int v = [] { const char* e = getenv("CREID_WGRAD_DMA"); return e ? atoi(e) : 1; }(); return v; }

// tile, split count and XCD form: from a measured plan, else the built-in rule (family, ring and grid: plan_wgrad_route)
static WgradPlan plan_wgrad(int M, int NCO, int K, int dtype, int stride = 1, bool peek = false) {
  // The fp32 partial tiles cost  workgroups x TM x TN x 8 bytes  of traffic per layer (write + re-read by the
  // reduce).  Measured (r01): shrinking the tile to cut that traffic LOSES (6147 vs 6370 img/s) -- the larger
  // tile's MFMA/LDS efficiency matters more and the partials mostly stay in the 256 MB Infinity Cache -- so the
  // largest tile wins by default; CREID_WGRAD_MAX_SPLITS re-enables the size/split trade-off for experiments.
  // Split target: ~512 workgroups per launch (r01 sweep with stand-alone reduce launches: 384-448 best; r02 with the
  // reduction riding on the next launch: 256 / 384 / 512 / 768 -> 7.20 / 7.10 / 7.08 / 7.18 ms per step).
  static const int target = [] { const char* e = getenv("CREID_WGRAD_TARGET_WGS"); int v = e ? atoi(e) : 0; return v > 0 ? v : 512; }();
  static const int max_splits_pref = [] { const char* e = getenv("CREID_WGRAD_MAX_SPLITS"); int v = e ? atoi(e) : 0; return v > 0 ? v : (1 << 30); }();
  const int ks = creid_is16(dtype) ? WKS : WKF;
  const int cand[3][2] = {{128, 128}, {128, 64}, {64, 64}};
  static const int xcd_mode = [] { const char* e = getenv("CREID_WGRAD_XCD"); return e ? atoi(e) : 1; }();
  WgradPlan p{};
  TunePlan tp;
  const bool have_plan = creid_is16(dtype) && (peek ? creid_tune_peek : creid_tune_lookup)(CREID_TUNE_WGRAD, M, NCO, K, stride << 1, tp);
  p.plan_state = have_plan ? 1 : 0;
  if (have_plan && !((tp.p0 == 64 || tp.p0 == 128) && (tp.p1 == 64 || tp.p1 == 128) && NCO % tp.p0 == 0 && K % tp.p1 == 0 && tp.p2 >= 1)) {
    p.plan_state = 2;                                                   // a word this shape cannot run: the built-in rule below
    if (!peek) creid_tune_declined(CREID_TUNE_WGRAD, M, NCO, K, stride << 1);
  } else if (have_plan) {
    // measured plan for this shape: tile tp.p0 x tp.p1, tp.p2 = pixel splits | ring depth << 16 | producer/consumer << 20 |
    // two k-groups << 21
    p.tm = tp.p0; p.tn = tp.p1;
    p.stages = (tp.p2 >> 16) & 15; p.ws = (tp.p2 >> 20) & 1; p.kg = (tp.p2 >> 21) & 1;
    tp.p2 &= 0xffff;
    p.tiles_k = K / p.tn;
    p.tiles = (NCO / p.tm) * p.tiles_k;
    int splits = tp.p2;
    const int max_splits = (M + ks - 1) / ks;
    if (splits > max_splits) splits = max_splits;
    p.m_per_split = ((M + splits - 1) / splits + ks - 1) / ks * ks;
    p.splits = (M + p.m_per_split - 1) / p.m_per_split;
    p.xcd = (xcd_mode && p.splits >= 8) ? 1 : 0;
    return p;
  }
  for (int ci = 0; ci < 3; ++ci) {
    int tm = cand[ci][0], tn = cand[ci][1];
    if (NCO % tm != 0) tm = 64;
    if (K % tn != 0) tn = 64;
    p.tm = tm; p.tn = tn;
    p.tiles_k = K / tn;
    p.tiles = (NCO / tm) * p.tiles_k;
    int splits = (target + p.tiles - 1) / p.tiles;
    // XCD placement (see wgrad_bf16_dma_kernel): a multiple of 8 splits, at least 8, so that every XCD owns whole
    // pixel ranges; CREID_WGRAD_XCD=0 keeps the round-1 rule
    p.xcd = 0;
    if (xcd_mode && creid_is16(dtype)) {
      if (splits >= 8) { splits = (splits + 4) / 8 * 8; p.xcd = 1; }                     // nearest multiple of 8
      else if (xcd_mode >= 2) { splits = splits >= 6 ? 8 : (splits >= 3 ? 4 : splits); p.xcd = 1; }   // 1, 2, 4, 8
    }
    const int max_splits = (M + 4 * ks - 1) / (4 * ks);
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    p.m_per_split = ((M + splits - 1) / splits + ks - 1) / ks * ks;
    p.splits = (M + p.m_per_split - 1) / p.m_per_split;
    if (p.xcd && p.splits < 8 && (8 % p.splits) != 0) p.xcd = 0;      // the shared-range map needs 1, 2, 4 (or >= 8) splits
    if (p.splits <= max_splits_pref) break;
  }
  return p;
}

// ---- the tap-fused route (wgrad_bf16_taps_kernel): coverage, split count and workspace are decided HERE for every caller
// (creid_conv2d_wgrad_workspace_bytes, wgrad_make_reduce_job, run_wgrad), so the three always agree
static std::atomic<int64_t> g_taps_launches{0};

static bool wgrad_taps_covers(int M, int NCO, int dtype, int stride, const WgradShape& sh) {
  if (!creid_is16(dtype) || sh.kh != 3 || sh.kw != 3 || stride != 1 || sh.pad != 1) return false;
  if (sh.cin != 64 && sh.cin != 128 && sh.cin != 256 && sh.cin != 512) return false;
  if (NCO <= 0 || NCO % 64 != 0 || sh.SH != sh.OH || sh.SW != sh.OW) return false;
  if (sh.OW != 8 && sh.OW != 16 && sh.OW != 32) return false;
  // a k-step is TPK pixels = whole rows of ONE image
  return (sh.OH * sh.OW) % TPK == 0 && M > 0 && M % (sh.OH * sh.OW) == 0;
}

// 1-D XCD grid: every XCD owns whole pixel ranges (>= 8 splits, or a split count that does not divide 8), else shares them
static unsigned wgrad_xcd_grid(const WgradPlan& p, bool ranged) {
  const int share = ranged ? 1 : 8 / p.splits;
  return ranged ? (unsigned)(p.tiles * ((p.splits + 7) / 8) * 8) : (unsigned)(8 * ((p.tiles + share - 1) / share));
}

// Everything about a weight-gradient launch: the tile plan, then kernel family, ring, k-groups, grid and whether the BatchNorm
// finalize job can ride.  creid_conv2d_wgrad_workspace_bytes, wgrad_make_reduce_job and run_wgrad all ask here, so they agree.
WgradPlan plan_wgrad_route(int M, int NCO, int K, int dtype, int stride, const WgradShape& sh, int fin_nblocks, bool peek) {
  WgradPlan p = plan_wgrad(M, NCO, K, dtype, stride, peek);      // (the registry lookup counts its hit / decline on either route)
  const unsigned nf8 = (unsigned)((fin_nblocks + 7) & ~7);
  const char* e = CREID_KNOB_ENV("CREID_WGRAD_TAPS");            // read per call: tests toggle it
  if (!(e && atoi(e) == 0) && wgrad_taps_covers(M, NCO, dtype, stride, sh)) {
    // One workgroup per CU (its LDS ring is > 80 KB), each writing 9 x 64 x 64 fp32 partials (147 KB) that the split reduction --
    // carried by the next data-gradient launch -- reads back.  Measured (profiles/wgrad_taps.md): with 1 or 4 tile-groups (64 and 128
    // channels) 256 workgroups of 4 k-steps make that launch 2-8 us slower than the tile kernel's partials did; ~170 workgroups of
    // 6 k-steps keep the kernel's gain and leave the carrier where it was.  16 and 64 tile-groups: one workgroup per CU.
    p.taps = 1; p.tm = 64; p.tn = 64; p.stages = 3; p.ws = 0; p.kg = 0; p.xcd = 1;
    p.tiles_k = sh.cin / 64;
    p.tiles = (NCO / 64) * p.tiles_k;
    const int steps = M / TPK;
    // CREID_WGRAD_TAPS_WGS: the workgroup target, for experiments and for tests that need many k-steps per workgroup at small shapes
    const char* we = CREID_KNOB_ENV("CREID_WGRAD_TAPS_WGS");
    const int target = (we && atoi(we) > 0) ? atoi(we) : (p.tiles <= 4 ? 192 : 256);
    int splits = (target + p.tiles / 2) / p.tiles;
    if (splits > steps) splits = steps;
    if (splits < 1) splits = 1;
    const int per = (steps + splits - 1) / splits;
    p.m_per_split = per * TPK;
    p.splits = (steps + per - 1) / per;
    p.family = WGRAD_TAPS; p.ns = 3; p.kgroups = 1;
    p.fin_rides = fin_nblocks > 0;                               // always: the grid is 1-D
    p.gx = wgrad_xcd_grid(p, p.splits >= 8 || (8 % p.splits) != 0) + nf8; p.gy = 1; p.block = 512;
  } else if (creid_is16(dtype) && wgrad_dma_env() && (sh.span >= p.tn || sh.stem)) {
    static const int use_ws_env = [] { const char* e = getenv("CREID_WGRAD_WS"); return e ? atoi(e) : 0; }();
    static const int stages_env = [] { const char* e = getenv("CREID_WGRAD_STAGES"); int v = e ? atoi(e) : 0; return (v >= 2 && v <= 4) ? v : 2; }();
    static const int kg_env = [] { const char* e = getenv("CREID_WGRAD_KG"); return e ? atoi(e) : 0; }();
    const int use_ws = p.ws ? 1 : use_ws_env;
    const int stages = (p.stages >= 2 && p.stages <= 4) ? p.stages : stages_env;
    const bool kg2 = (p.kg || kg_env == 2) && !use_ws && !sh.stem;
    const bool kg3_fits = 2 * 3 * (p.tm + p.tn) * 128 <= 160 * 1024;
    p.family = WGRAD_DMA;
    p.wsk = !kg2 && use_ws && !sh.stem;
    p.kgroups = kg2 ? 2 : 1;
    p.ns = kg2 ? ((stages >= 3 && kg3_fits) ? 3 : 2) : (p.wsk ? 2 : stages);
    p.block = (kg2 || p.wsk) ? 512 : 256;
    p.fin_rides = fin_nblocks > 0 && p.xcd;                      // the carried job needs the 1-D grid
    if (p.xcd) { p.gx = wgrad_xcd_grid(p, p.splits >= 8) + (p.fin_rides ? nf8 : 0u); p.gy = 1; }
    else { p.gx = (unsigned)p.tiles; p.gy = (unsigned)p.splits; }
  } else if (dtype == CREID_F16) {
    p.family = WGRAD_NONE; p.err = CREID_E_SHAPE;                // (no register-staged f16 fallback: refused, not mis-run)
  } else {
    p.family = dtype == CREID_BF16 ? WGRAD_REG_BF16 : WGRAD_F32;
    p.gx = (unsigned)p.tiles; p.gy = (unsigned)p.splits; p.block = 256;
  }
  if (dtype == CREID_F16 && !wgrad_dma_env()) { p.family = WGRAD_NONE; p.err = CREID_E_DTYPE; }   // f16: the LDS-DMA kernels only
  return p;
}

static void launch_wgrad_taps(const IGemmGeom& g, const void* dy, const void* x, int NCO, float* ws, const WgradPlan& p, int dtype,
                              hipStream_t s, const BnBwdFinJob& fin) {
  const int cin = 1 << g.log2span;
#define CREID_WT_LAUNCH(OW_, ET_)                                                                                          \
  hipLaunchKernelGGL((wgrad_bf16_taps_kernel<OW_, ET_>), dim3(p.gx), dim3(p.block), 0, s, (const unsigned short*)dy,       \
                     (const unsigned short*)x, g.M, g.OH, cin, NCO, ws, p.tiles, p.tiles_k, p.splits, p.m_per_split, fin)
#define CREID_WT_OW(OW_) do { if (dtype == CREID_F16) CREID_WT_LAUNCH(OW_, F16T); else CREID_WT_LAUNCH(OW_, Bf16T); } while (0)
  if (g.OW == 8) CREID_WT_OW(8); else if (g.OW == 16) CREID_WT_OW(16); else CREID_WT_OW(32);
#undef CREID_WT_OW
#undef CREID_WT_LAUNCH
  g_taps_launches.fetch_add(1, std::memory_order_relaxed);
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_job_kernel(BnBwdFinJob j) {
  __shared__ __attribute__((aligned(16))) double fin_lds[4 * 2 * 16];
  bn_bwd_finalize_block<256>(j, (int)blockIdx.x, fin_lds);
}

// fin: the BatchNorm-backward finalize job (bn_fin.hpp) where the plan says it rides in the first workgroups, else an empty job
template <int TM, int TN>
static void launch_wgrad_t(const IGemmGeom& g, const void* dy, const void* x, int NCO, float* ws, const WgradPlan& p,
                           int dtype, hipStream_t s, const BnBwdFinJob& fin) {
  const dim3 grid(p.gx, p.gy), block(p.block);
  const int xt = p.xcd ? p.tiles : 0;
#ifdef CREID_ABL_BUILD
  static const int wg_abl = creid_ablation_env("CREID_WGRAD_ABL");   // 1: no MFMA, 2: no DMA after the first k-tile, 4: no fragment reads either
#else
  const int wg_abl = 0;                                              // (the switches exist in the ablation build only: conv_common.hpp)
#endif
  if (p.family == WGRAD_DMA) {
    constexpr bool kg3_fits = 2 * 3 * (TM + TN) * 128 <= 160 * 1024;
#define CREID_WG_LAUNCH(NS_, WS_, KG_)                                                                                            \
    do {                                                                                                                          \
      if (dtype == CREID_F16)                                                                                                     \
        hipLaunchKernelGGL((wgrad_bf16_dma_kernel<TM, TN, NS_, WS_, KG_, F16T>), grid, block, 0, s, g, (const unsigned short*)dy, \
                           (const unsigned short*)x, NCO, ws, p.tiles_k, p.m_per_split, xt, p.splits, fin, wg_abl);               \
      else                                                                                                                        \
        hipLaunchKernelGGL((wgrad_bf16_dma_kernel<TM, TN, NS_, WS_, KG_, Bf16T>), grid, block, 0, s, g, (const unsigned short*)dy, \
                           (const unsigned short*)x, NCO, ws, p.tiles_k, p.m_per_split, xt, p.splits, fin, wg_abl);               \
    } while (0)
    if (p.kgroups == 2 && p.ns == 3) {
      if constexpr (kg3_fits) CREID_WG_LAUNCH(3, false, 2);
    } else if (p.kgroups == 2) CREID_WG_LAUNCH(2, false, 2);
    else if (p.wsk) CREID_WG_LAUNCH(2, true, 1);
    else if (p.ns == 2) CREID_WG_LAUNCH(2, false, 1);
    else if (p.ns == 3) CREID_WG_LAUNCH(3, false, 1);
    else CREID_WG_LAUNCH(4, false, 1);
#undef CREID_WG_LAUNCH
  }
  else if (p.family == WGRAD_REG_BF16)
    hipLaunchKernelGGL((wgrad_bf16_kernel<TM, TN>), grid, block, 0, s, g, (const unsigned short*)dy,
                       (const unsigned short*)x, NCO, ws, p.tiles_k, p.m_per_split);
  else
    hipLaunchKernelGGL((wgrad_f32_kernel<TM, TN>), grid, block, 0, s, g, (const float*)dy, (const float*)x, NCO, ws,
                       p.tiles_k, p.m_per_split);
}

static int run_wgrad(const IGemmGeom& g, const void* dy, const void* x, int NCO, float* dw, int kw_taps, int cpitch,
                     int cin, int kh, int kw, int accumulate, void* ws, size_t ws_bytes, int dtype, hipStream_t s,
                     int phases = 3, const BnBwdFinJob* fin = nullptr) {
  if (!creid_is16(dtype) && dtype != CREID_F32) return CREID_E_DTYPE;
  // f16 exists in the LDS-DMA kernels only (no register-staged fallback): shapes those do not cover are refused, not mis-run
  if (dtype == CREID_F16 && !wgrad_dma_env()) return CREID_E_DTYPE;
  // (the tap-fused route needs the plain NHWC gather: the stem's packed kernel rows and pre-padded image stay on the tile kernels)
  const WgradShape shp{(cpitch == cin && kw_taps == kw && g.check_bounds && (1 << g.log2span) == cin) ? kh : 0, kw, g.pad, cin, g.OH, g.OW,
                       g.SH, g.SW, 1 << g.log2span, conv_is_stem_geom(g)};
  const WgradPlan p = plan_wgrad_route(g.M, NCO, g.K, dtype, g.stride, shp, fin ? fin->nblocks : 0);
  // (a shape without a kernel -- an f16 stem with its DMA path switched off -- is refused here instead of summing an unwritten
  // workspace into dw)
  if ((phases & 1) && p.family == WGRAD_NONE) return p.err;
  const size_t need = (size_t)p.splits * NCO * g.K * sizeof(float);
  if (ws_bytes < need) return CREID_E_WS;
  if (phases & 1) {
    const BnBwdFinJob ride = (fin && p.fin_rides) ? *fin : BnBwdFinJob{};
    if (p.family == WGRAD_TAPS) launch_wgrad_taps(g, dy, x, NCO, (float*)ws, p, dtype, s, ride);
    else if (p.tm == 128 && p.tn == 128) launch_wgrad_t<128, 128>(g, dy, x, NCO, (float*)ws, p, dtype, s, ride);
    else if (p.tm == 128 && p.tn == 64) launch_wgrad_t<128, 64>(g, dy, x, NCO, (float*)ws, p, dtype, s, ride);
    else if (p.tm == 64 && p.tn == 128) launch_wgrad_t<64, 128>(g, dy, x, NCO, (float*)ws, p, dtype, s, ride);
    else launch_wgrad_t<64, 64>(g, dy, x, NCO, (float*)ws, p, dtype, s, ride);
    if (fin && !p.fin_rides)                                     // kernel variants without the carrier: stand-alone launch
      hipLaunchKernelGGL(bn_bwd_finalize_job_kernel, dim3((unsigned)fin->nblocks), dim3(256), 0, s, *fin);
  }
  if (!(phases & 2)) return (int)hipGetLastError();
  if (kh * kw == 9 && cpitch == cin && (1 << g.log2span) == cin && kw_taps == kw && p.splits <= 16 &&
      (size_t)g.K * sizeof(float) <= 48 * 1024) {
    hipLaunchKernelGGL(wgrad_reduce_taps_kernel, dim3((unsigned)NCO), dim3(256), (size_t)g.K * sizeof(float), s,
                       (const float*)ws, p.splits, NCO, g.K, cin, 9, dw, accumulate);
    return (int)hipGetLastError();
  }
  const int64_t total4 = (int64_t)NCO * g.K / 4;
#define CREID_WRED(SL_)                                                                                              \
  hipLaunchKernelGGL(wgrad_reduce_kernel<SL_>, dim3((unsigned)((total4 + 256 / SL_ - 1) / (256 / SL_))), dim3(256), 0, s, \
                     (const float*)ws, p.splits, NCO, g.K, g.log2span, kw_taps, cpitch, cin, kh, kw, dw, accumulate)
  if (p.splits <= 8) CREID_WRED(1);
  else if (p.splits <= 32) CREID_WRED(4);
  else if (p.splits <= 128) CREID_WRED(16);
  else CREID_WRED(64);
#undef CREID_WRED
  return (int)hipGetLastError();
}

// ---- the split reduction as a job (wgrad_reduce.hpp): stand-alone launch and the glue used by the data-gradient
// launch that carries it
__global__ __launch_bounds__(512) void wgrad_reduce_job_kernel(WRedJob j) {
  extern __shared__ __attribute__((aligned(16))) float wred_lds[];
  wgrad_reduce_block<512>(j, (int)blockIdx.x, wred_lds);
}

int wgrad_reduce_job_launch(const WRedJob& j, hipStream_t s) {
  hipLaunchKernelGGL(wgrad_reduce_job_kernel, dim3((unsigned)j.nblocks), dim3(512), (size_t)(4 * 512 + j.K) * sizeof(float), s, j);
  return (int)hipGetLastError();
}

bool wgrad_make_reduce_job(const creid_conv_desc* d, int dtype, const void* ws, size_t ws_bytes, float* dw, int accumulate,
                           WRedJob& j) {
  if (!d || !ws || !dw) return false;
  const int M = (int)(d->batch * d->out_h * d->out_w), K = (int)(d->kh * d->kw * d->in_c), NCO = (int)d->out_c;
  const WgradPlan p = plan_wgrad_route(M, NCO, K, dtype, d->stride, wgrad_shape_of(d));
  if (ws_bytes < (size_t)p.splits * NCO * K * sizeof(float)) return false;
  const bool ok = wred_make_job(j, (const float*)ws, dw, p.splits, NCO, K, (int)d->in_c, d->kh, d->kw, accumulate);
  // timing experiments only: the carrier workgroups are launched but do nothing (gradients are then WRONG)
  static const int dry = creid_ablation_env("CREID_WRED_DRY");
  if (ok && dry) { j.K = 0; j.splits = 0; }
  return ok;
}

extern "C" {

size_t creid_conv2d_wgrad_workspace_bytes(const creid_conv_desc* d, int dtype) {
  if (!d) return 0;
  const int M = (int)(d->batch * d->out_h * d->out_w), K = (int)(d->kh * d->kw * d->in_c);
  const WgradPlan p = plan_wgrad_route(M, (int)d->out_c, K, dtype, d->stride, wgrad_shape_of(d));
  return (size_t)p.splits * d->out_c * K * sizeof(float);
}

static int conv_wgrad_phases(const creid_conv_desc* d, const void* x, const void* dy, float* dw_oihw, int accumulate,
                             void* ws, size_t ws_bytes, int dtype, void* stream, int phases, const BnBwdFinJob* fin = nullptr);

int64_t creid_wgrad_taps_launches(void) { return (int64_t)g_taps_launches.load(std::memory_order_relaxed); }

int creid_conv2d_wgrad_nhwc(const creid_conv_desc* d, const void* x, const void* dy, float* dw_oihw, int accumulate,
                            void* ws, size_t ws_bytes, int dtype, void* stream) {
  CREID_CHECK_ARG(x && dy && dw_oihw);
  return conv_wgrad_phases(d, x, dy, dw_oihw, accumulate, ws, ws_bytes, dtype, stream, 3);
}

int creid_conv2d_wgrad_partials(const creid_conv_desc* d, const void* x, const void* dy, void* ws, size_t ws_bytes,
                                int dtype, void* stream) {
  CREID_CHECK_ARG(x && dy);
  return conv_wgrad_phases(d, x, dy, nullptr, 0, ws, ws_bytes, dtype, stream, 1);
}

int creid_conv2d_wgrad_partials_bnfin(const creid_conv_desc* d, const void* x, const void* dy, void* ws, size_t ws_bytes,
                                      int dtype, const float* bn_partial, int64_t bn_rows, int64_t bn_C, int64_t bn_count,
                                      const float* bn_mean, const float* bn_invstd, const float* bn_gamma, float* bn_sums,
                                      float* bn_dgamma, float* bn_dbeta, void* stream) {
  CREID_CHECK_ARG(x && dy && bn_partial && bn_mean && bn_invstd && bn_sums && bn_rows > 0 && bn_C > 0 && bn_count > 0);
  BnBwdFinJob fin{bn_partial, (int)bn_rows, (int)bn_C, (float)(1.0 / (double)bn_count), bn_mean, bn_invstd, bn_gamma, bn_sums,
                  bn_dgamma, bn_dbeta, 0, 16};
  bn_bwd_fin_shape(fin);
  return conv_wgrad_phases(d, x, dy, nullptr, 0, ws, ws_bytes, dtype, stream, 1, &fin);
}

int creid_conv2d_wgrad_reduce(const creid_conv_desc* d, float* dw_oihw, int accumulate, const void* ws, size_t ws_bytes,
                              int dtype, void* stream) {
  CREID_CHECK_ARG(dw_oihw);
  return conv_wgrad_phases(d, nullptr, nullptr, dw_oihw, accumulate, const_cast<void*>(ws), ws_bytes, dtype, stream, 2);
}

// BatchNorm-backward finalize + split reduction in ONE launch: the first workgroups (a multiple of 8) finalize, the rest sum
// the previous weight gradient's partial tiles.  Both are off each other's data; the reduction is bandwidth work that fills the
// ~4 us during which the 4-128 finalize workgroups wait on their dependent loads, and the data gradient before it keeps its
// full grid (no reduction tail).
__global__ __launch_bounds__(512) void wred_bnfin_kernel(WRedJob j, BnBwdFinJob fin) {
  extern __shared__ __attribute__((aligned(16))) float wredfin_lds[];
  const int nf8 = fin.partial ? ((fin.nblocks + 7) & ~7) : 0;
  if ((int)blockIdx.x < nf8) {
    if ((int)blockIdx.x < fin.nblocks) bn_bwd_finalize_block<512>(fin, (int)blockIdx.x, wredfin_lds);
    return;
  }
  wgrad_reduce_block<512>(j, (int)blockIdx.x - nf8, wredfin_lds);
}

int creid_bn2d_bwd_finalize_wred(const float* bn_partial, int64_t bn_rows, int64_t bn_C, int64_t bn_count, const float* bn_mean,
                                 const float* bn_invstd, const float* bn_gamma, float* bn_sums, float* bn_dgamma,
                                 float* bn_dbeta, const creid_conv_desc* wred_desc, float* wred_dw, int wred_accumulate,
                                 const void* wred_ws, size_t wred_ws_bytes, int dtype, void* stream) {
  CREID_CHECK_ARG(bn_partial && bn_mean && bn_invstd && bn_sums && bn_rows > 0 && bn_C > 0 && bn_count > 0 && wred_desc &&
                  wred_dw && wred_ws);
  if (!creid_is_storage(dtype)) return CREID_E_DTYPE;
  BnBwdFinJob fin{bn_partial, (int)bn_rows, (int)bn_C, (float)(1.0 / (double)bn_count), bn_mean, bn_invstd, bn_gamma, bn_sums,
                  bn_dgamma, bn_dbeta, 0, 16};
  bn_bwd_fin_shape(fin);
  WRedJob j{};
  if (!wgrad_make_reduce_job(wred_desc, dtype, wred_ws, wred_ws_bytes, wred_dw, wred_accumulate, j)) return CREID_E_SHAPE;
  const int nf8 = (fin.nblocks + 7) & ~7;
  size_t lds = (size_t)(4 * 512 + j.K) * sizeof(float);
  if (lds < 4096) lds = 4096;
  hipLaunchKernelGGL(wred_bnfin_kernel, dim3((unsigned)(nf8 + j.nblocks)), dim3(512), lds, as_stream(stream), j, fin);
  CREID_LAUNCH_RET();
}

/* The split reduction as the SAME job a data-gradient launch would have carried (wgrad_reduce_block, identical summation
 * order), as its own launch: for the reductions that find no carrier (end of a layer group / of the backward pass), so that
 * a schedule with and without carriers gives bit-identical gradients. */
int creid_conv2d_wgrad_reduce_job(const creid_conv_desc* d, float* dw_oihw, int accumulate, const void* ws, size_t ws_bytes,
                                  int dtype, void* stream) {
  CREID_CHECK_ARG(d && dw_oihw && ws);
  if (!creid_is_storage(dtype)) return CREID_E_DTYPE;
  WRedJob j{};
  if (!wgrad_make_reduce_job(d, dtype, ws, ws_bytes, dw_oihw, accumulate, j))
    return creid_conv2d_wgrad_reduce(d, dw_oihw, accumulate, ws, ws_bytes, dtype, stream);
  return wgrad_reduce_job_launch(j, as_stream(stream));
}

static int conv_wgrad_phases(const creid_conv_desc* d, const void* x, const void* dy, float* dw_oihw, int accumulate,
                             void* ws, size_t ws_bytes, int dtype, void* stream, int phases, const BnBwdFinJob* fin) {
  CREID_CHECK_ARG(d && ws);
  if (igemm_ilog2(d->in_c) < 0 || d->in_c < 64 || d->out_c % 64 != 0) return CREID_E_SHAPE;
  IGemmGeom g = fwd_geom(d);
  { static const int noinc = [] { const char* e = getenv("CREID_WGRAD_NOINC"); return e ? atoi(e) : 0; }(); if (noinc) g.check_bounds = 2; }
  return run_wgrad(g, dy, x, (int)d->out_c, dw_oihw, d->kw, (int)d->in_c, (int)d->in_c, d->kh, d->kw, accumulate, ws,
                   ws_bytes, dtype, as_stream(stream), phases, fin);
}

// ---- bf16x3: partial tiles by wgrad_x3_kernel in the CREID_F32 workspace layout, summed by the CREID_F32 split reduction
size_t creid_conv2d_wgrad_x3_workspace_bytes(const creid_conv_desc* d) {
  if (!d || conv_check_desc(d)) return 0;
  return creid_conv2d_wgrad_workspace_bytes(d, CREID_F32);
}

int creid_conv2d_wgrad_x3_partials(const creid_conv_desc* d, const void* x, const void* dy, void* ws, size_t ws_bytes,
                                   void* stream) {
  const int rc = conv_check_desc(d);
  if (rc) return rc;
  CREID_CHECK_ARG(x && dy && ws);
  IGemmGeom g = fwd_geom(d);
  const int NCO = (int)d->out_c;
  const WgradPlan p = plan_wgrad(g.M, NCO, g.K, CREID_F32, g.stride);
  if (ws_bytes < (size_t)p.splits * NCO * g.K * sizeof(float)) return CREID_E_WS;
  const dim3 grid((unsigned)p.tiles, (unsigned)p.splits), block(256);
  hipStream_t s = as_stream(stream);
#define CREID_WX3(TM_, TN_)                                                                                          \
  hipLaunchKernelGGL((wgrad_x3_kernel<TM_, TN_>), grid, block, 0, s, g, (const float*)dy, (const float*)x, NCO, (float*)ws, \
                     p.tiles_k, p.m_per_split)
  if (p.tm == 128 && p.tn == 128) CREID_WX3(128, 128);
  else if (p.tm == 128 && p.tn == 64) CREID_WX3(128, 64);
  else if (p.tm == 64 && p.tn == 128) CREID_WX3(64, 128);
  else CREID_WX3(64, 64);
#undef CREID_WX3
  CREID_LAUNCH_RET();
}

int creid_conv2d_wgrad_x3_nhwc(const creid_conv_desc* d, const void* x, const void* dy, float* dw_oihw, int accumulate,
                               void* ws, size_t ws_bytes, void* stream) {
  const int rc = conv_check_desc(d);
  if (rc) return rc;
  CREID_CHECK_ARG(x && dy && dw_oihw && ws);
  const int r1 = creid_conv2d_wgrad_x3_partials(d, x, dy, ws, ws_bytes, stream);
  if (r1) return r1;
  return creid_conv2d_wgrad_reduce_job(d, dw_oihw, accumulate, ws, ws_bytes, CREID_F32, stream);
}

size_t creid_stem_conv_wgrad_workspace_bytes(int64_t batch, int64_t H, int64_t W, int dtype) {
  // (stride 2: the launch looks its plan up with the stem geometry's stride -- with the default of 1 a measured plan of a 1 x 1
  // layer that happens to share (M, 64, 256) at another batch size answered here but not there: workspace too small)
  // 0: a shape creid_stem_conv_wgrad refuses (stem_check_shape) -- that call then returns the refusal whatever workspace it is handed
  if (stem_check_shape(batch, H, W)) return 0;
  const WgradPlan p = plan_wgrad((int)(batch * (H / 2) * (W / 2)), 64, 256, dtype, 2);
  return (size_t)p.splits * 64 * 256 * sizeof(float);
}

/* stem weight gradient into the OIHW [64,3,7,7] fp32 tensor (see creid_stem_conv_fwd for layouts). */
int creid_stem_conv_wgrad(int64_t batch, int64_t H, int64_t W, const void* xpad, const void* dy, float* dw_oihw,
                          int accumulate, void* ws, size_t ws_bytes, int dtype, void* stream) {
  CREID_CHECK_ARG(xpad && dy && dw_oihw && ws);
  if (const int rc = stem_check_shape(batch, H, W)) return rc;
  IGemmGeom g = stem_geom(batch, H, W);
  return run_wgrad(g, dy, xpad, 64, dw_oihw, 1, 4, 3, 7, 7, accumulate, ws, ws_bytes, dtype, as_stream(stream));
}

}  // extern "C"
