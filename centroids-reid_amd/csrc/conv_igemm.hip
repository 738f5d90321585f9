// Stage A: implicit-GEMM convolution forward / data-gradient for NHWC activations.
// (replaces nn.Conv2d fwd + dgrad of modelling/backbones/resnet.py:56-61,94,109 and
//  resnet_ibn_a.py:40-48,83,110 -- bias-free 7x7 s2, 3x3 (s1/s2), 1x1 (s1/s2) convolutions.)
//
// bf16: 128 x BN x 64 tile (2x2 waves, 64 x BN/2 per wave) on v_mfma_f32_32x32x16_bf16, fp32 accumulate; LDS
//       row-major [row][64] with the 16-B chunk index XOR-swizzled by (row>>1)&7 (conflict-free ds_read_b128).
//       Three kernels share that tiling:
//         igemm_bf16_ws_kernel   512 threads, producer waves issue the global->LDS DMA gather (the A rows come from
//                                different image rows / taps) into an NS-stage ring, consumer waves multiply -- the
//                                default for every 1x1 / 3x3 layer (igemm_bf16_halo_kernel: the same kernel with the A operand
//                                resident in LDS, for the stride-1 3x3 layers whose tile is whole image rows);
//         igemm_bf16_dma_kernel  256 threads, every wave issues its DMA pieces and multiplies -- the stem (32-element
//                                taps, two per k-tile), CREID_IGEMM_WS=0 and the plans that name it;
//         igemm_bf16_kernel      register-staged gather -- the fallback under CREID_IGEMM_DMA=0 / CREID_STEM_DMA=0.
//       The two DMA kernels share one epilogue (igemm_tile_epilogue below, built from conv_epilogue.hpp).
// f32 : 128 x BN x 16 tile on v_mfma_f32_32x32x2_f32 (exact f32; parity mode), K-major LDS.
// Epilogue (both): optional "+ add_src" (residual-gradient accumulation in dgrad), store in the
// activation dtype, and optional per-tile per-channel (sum, sum of squares) partials of the fp32
// accumulators for the training-mode BatchNorm that follows every convolution.
#include "conv_epilogue.hpp"
#include <type_traits>
#include <atomic>
#include "conv_route.hpp"
#include <stdlib.h>

// Out-of-image taps read this 128-byte page of zeros instead of selecting zeros per dword (saves 3 VALU
// per load in the gather path).
__device__ __attribute__((aligned(128))) unsigned g_zero_page[32];

// ------------------------------------------------------------------------------------ bf16
template <int BN>
__global__ __launch_bounds__(256, BN == 128 ? 1 : 2) void igemm_bf16_kernel(IGemmGeom g, const unsigned short* __restrict__ src,
                                                         const unsigned short* __restrict__ wgt,
                                                         unsigned short* __restrict__ out,
                                                         const unsigned short* __restrict__ add_src,
                                                         float* __restrict__ bn_part, int tiles_n) {
  constexpr int BK = 64, TNW = BN / 64, NB = BN / 32;
  constexpr int CP = BN + 8;                                   // C-tile staging pitch (elements)
  constexpr int LDS_ELEMS = (128 * BK + BN * BK) > (128 * CP) ? (128 * BK + BN * BK) : (128 * CP);
  __shared__ __attribute__((aligned(16))) unsigned short smem[LDS_ELEMS];
  unsigned short* As = smem;                 // single-buffered tiles + register prefetch: half the LDS of a
  unsigned short* Bs = smem + 128 * BK;      // double buffer -> twice the resident workgroups per CU
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
  const int row0 = tile_m * 128, col0 = tile_n * BN;
  const int span_mask = (1 << g.log2span) - 1;
  const bool tap_uniform = g.log2span >= 6;        // a 64-wide k-tile never straddles two taps (all but the stem)

  const int lrow = tid >> 3, lch = tid & 7;
  int oy[4], ox[4], bpix[4], soff[4];
  bool vm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = lrow + 32 * i, m = row0 + r;
    vm[i] = m < g.M;
    const int mm = vm[i] ? m : 0;
    int b, rem;
    fast_divmod(mm, g.OH * g.OW, g.inv_ohow, b, rem);
    fast_divmod(rem, g.OW, g.inv_ow, oy[i], ox[i]);
    bpix[i] = b * g.SH * g.SW;
    soff[i] = r * BK + ((lch ^ ((r >> 1) & 7)) << 3);
  }
  const unsigned short* wp[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) wp[i] = wgt + (int64_t)(col0 + lrow + 32 * i) * g.K + 8 * lch;

  // A-row source pointers are recomputed only when the k-loop enters a new tap (tap-major K order);
  // inside a tap consecutive k-tiles just advance by 64 channels.
  const unsigned short* aptr[4];
  int amul[4];                 // 1 for a real source row, 0 for the zero page (kills the channel offset)
  int cur_tap = -1;
  const unsigned short* zpage = reinterpret_cast<const unsigned short*>(g_zero_page) + 8 * lch;
  auto set_tap = [&](int tap) {
    const int r = tap / g.kw, s = tap - r * g.kw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int iy, ix;
      const bool ok = vm[i] && igemm_src_pixel(g, oy[i], ox[i], r, s, iy, ix);
      aptr[i] = ok ? src + (int64_t)(bpix[i] + iy * g.SW + ix) * g.pitch + 8 * lch : zpage;
      amul[i] = ok ? 1 : 0;
    }
  };
  // 3-deep register prefetch ring: the loads of k-tile t+3 are issued while tile t is multiplied, so a
  // load has ~3 compute phases to land (HBM/L2 latency >> one 16-MFMA phase at 2 workgroups per CU).
  // The ring lives in NAMED scalars (arrays / lambdas taking array references kept ending up in scratch).
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // first-class vector: always SROA-able
  struct Stage { u32x4 a0, a1, a2, a3, b0, b1, b2, b3; };
  Stage st0, st1, st2;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
#define IGEMM_LDA(I_, DST, C_) DST = *reinterpret_cast<const u32x4*>(aptr[I_] + (C_) * amul[I_])
#define IGEMM_LDA_G(I_, DST, R_, S_, C_)                                                                \
  do {                                                                                                  \
    int iy, ix;                                                                                         \
    if (vm[I_] && igemm_src_pixel(g, oy[I_], ox[I_], R_, S_, iy, ix))                                   \
      DST = *reinterpret_cast<const u32x4*>(src + (int64_t)(bpix[I_] + iy * g.SW + ix) * g.pitch + (C_)); \
    else                                                                                                \
      DST = zero4;                                                                                      \
  } while (0)
#define IGEMM_GLOAD(T_, ST)                                                                             \
  do {                                                                                                  \
    const int t_ = (T_);                                                                                \
    if (tap_uniform) {                                                                                  \
      const int tap_ = (t_ * BK) >> g.log2span;                                                         \
      if (tap_ != cur_tap) { set_tap(tap_); cur_tap = tap_; }                                           \
      const int c_ = (t_ * BK) & span_mask;                                                             \
      IGEMM_LDA(0, ST.a0, c_); IGEMM_LDA(1, ST.a1, c_); IGEMM_LDA(2, ST.a2, c_); IGEMM_LDA(3, ST.a3, c_); \
    } else {                                                                                            \
      const int kk_ = t_ * BK + 8 * lch;                                                                \
      const int tap_ = kk_ >> g.log2span, c_ = kk_ & span_mask;                                         \
      const int r_ = tap_ / g.kw, s_ = tap_ - r_ * g.kw;                                                \
      IGEMM_LDA_G(0, ST.a0, r_, s_, c_); IGEMM_LDA_G(1, ST.a1, r_, s_, c_);                             \
      IGEMM_LDA_G(2, ST.a2, r_, s_, c_); IGEMM_LDA_G(3, ST.a3, r_, s_, c_);                             \
    }                                                                                                   \
    ST.b0 = *reinterpret_cast<const u32x4*>(wp[0] + t_ * BK);                                           \
    ST.b1 = *reinterpret_cast<const u32x4*>(wp[1] + t_ * BK);                                           \
    if constexpr (NB == 4) {                                                                            \
      ST.b2 = *reinterpret_cast<const u32x4*>(wp[2] + t_ * BK);                                         \
      ST.b3 = *reinterpret_cast<const u32x4*>(wp[3] + t_ * BK);                                         \
    }                                                                                                   \
  } while (0)
#define IGEMM_LSTORE(ST)                                                                                \
  do {                                                                                                  \
    *reinterpret_cast<u32x4*>(&As[soff[0]]) = ST.a0; *reinterpret_cast<u32x4*>(&As[soff[1]]) = ST.a1;   \
    *reinterpret_cast<u32x4*>(&As[soff[2]]) = ST.a2; *reinterpret_cast<u32x4*>(&As[soff[3]]) = ST.a3;   \
    *reinterpret_cast<u32x4*>(&Bs[soff[0]]) = ST.b0; *reinterpret_cast<u32x4*>(&Bs[soff[1]]) = ST.b1;   \
    if constexpr (NB == 4) {                                                                            \
      *reinterpret_cast<u32x4*>(&Bs[soff[2]]) = ST.b2; *reinterpret_cast<u32x4*>(&Bs[soff[3]]) = ST.b3; \
    }                                                                                                   \
  } while (0)

  f32x16 acc[2][TNW];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TNW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = g.K / BK;
  const int l31 = lane & 31, kh = lane >> 5;
  auto compute = [&]() {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ch = 2 * kk + kh;
      s16x8 a[2], b[TNW];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = wm * 64 + i * 32 + l31;
        a[i] = *reinterpret_cast<const s16x8*>(&As[r * BK + ((ch ^ ((r >> 1) & 7)) << 3)]);
      }
#pragma unroll
      for (int j = 0; j < TNW; ++j) {
        const int c = wn * (BN / 2) + j * 32 + l31;
        b[j] = *reinterpret_cast<const s16x8*>(&Bs[c * BK + ((ch ^ ((c >> 1) & 7)) << 3)]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TNW; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[i]),
                                                              __builtin_bit_cast(bf16x8, b[j]), acc[i][j], 0, 0, 0);
    }
  };
  // Every prefetch is unconditional (the tile index is clamped; re-loading the last tile is harmless).
  // Main loop: whole triples of k-tiles with the ring stages named statically (no register rotation);
  // the 0-2 leftover tiles run through a rotating tail.
  const int last = nk - 1;
  IGEMM_GLOAD(0, st0);
  IGEMM_GLOAD(min(1, last), st1);
  IGEMM_GLOAD(min(2, last), st2);
  const int nk3 = nk - nk % 3;
  int t = 0;
  for (; t < nk3; t += 3) {
    __syncthreads();               // fragment reads of the previous tile are done
    IGEMM_LSTORE(st0);
    __syncthreads();
    IGEMM_GLOAD(min(t + 3, last), st0);
    compute();
    __syncthreads();
    IGEMM_LSTORE(st1);
    __syncthreads();
    IGEMM_GLOAD(min(t + 4, last), st1);
    compute();
    __syncthreads();
    IGEMM_LSTORE(st2);
    __syncthreads();
    IGEMM_GLOAD(min(t + 5, last), st2);
    compute();
  }
  for (; t < nk; ++t) {            // at most two iterations
    __syncthreads();
    IGEMM_LSTORE(st0);
    __syncthreads();
    st0 = st1;
    compute();
  }
#undef IGEMM_GLOAD
#undef IGEMM_LSTORE
#undef IGEMM_LDA
#undef IGEMM_LDA_G
  __syncthreads();

  // ---- epilogue: per-channel (sum, sumsq) partials from the fp32 accumulators, then the C tile is
  // staged through LDS (bf16) so that global stores (and the add_src reads) are 16-B coalesced rows.
  float s1v[TNW], s2v[TNW];
#pragma unroll
  for (int j = 0; j < TNW; ++j) {
    const int cl = wn * (BN / 2) + j * 32 + l31;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const float v = acc[i][j][r];               // rows >= M were zero-filled -> contribute 0
        s1 += v; s2 = fmaf(v, v, s2);
        smem[rl * CP + cl] = f32_to_bf16_bits(v);
      }
    }
    s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
    s1v[j] = s1; s2v[j] = s2;
  }
  __syncthreads();
  constexpr int CPR = BN / 8;                                  // 16-B chunks per tile row
#pragma unroll
  for (int i = 0; i < (128 * CPR) / 256; ++i) {
    const int id = tid + 256 * i, rl = id / CPR, ch = id - rl * CPR;
    const int rr = row0 + rl;
    if (rr < g.M) {
      uint4 v = *reinterpret_cast<const uint4*>(&smem[rl * CP + ch * 8]);
      const int64_t off = (int64_t)rr * g.N + col0 + ch * 8;
      if (add_src) {
        const uint4 a = *reinterpret_cast<const uint4*>(add_src + off);
        unsigned* vw = &v.x; const unsigned* aw = &a.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float lo = __uint_as_float(vw[q] << 16) + __uint_as_float(aw[q] << 16);
          const float hi = __uint_as_float(vw[q] & 0xffff0000u) + __uint_as_float(aw[q] & 0xffff0000u);
          vw[q] = (unsigned)f32_to_bf16_bits(lo) | ((unsigned)f32_to_bf16_bits(hi) << 16);
        }
      }
      *reinterpret_cast<uint4*>(out + off) = v;
    }
  }
  if (bn_part) {
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);      // [2 (wm)][2 (s1,s2)][BN]
#pragma unroll
    for (int j = 0; j < TNW; ++j) {
      const int cl = wn * (BN / 2) + j * 32 + l31;
      if (kh == 0) { red[(wm * 2 + 0) * BN + cl] = s1v[j]; red[(wm * 2 + 1) * BN + cl] = s2v[j]; }
    }
    __syncthreads();
    for (int i = tid; i < 2 * BN; i += 256) {
      const int which = i / BN, cl = i - which * BN;
      bn_part[((int64_t)tile_m * 2 + which) * g.N + col0 + cl] = red[(0 * 2 + which) * BN + cl] + red[(1 * 2 + which) * BN + cl];
    }
  }
}
// ------------------------------------------------------------------------------------ 16-bit C-tile epilogue
// The epilogue of the two LDS-DMA tile kernels (primitives: conv_epilogue.hpp), entered behind the __syncthreads() that ends
// the k-loop.  NT = 256 (igemm_bf16_dma_kernel): every wave holds a 64 x BN/2 accumulator sub-tile; NT = 512
// (igemm_bf16_ws_kernel): waves 0-3 hold BM/2 x BN/2 sub-tiles, all eight waves copy out.  `smem` is the kernel's whole LDS
// array: first the staged C tile ([BN columns][BM + 4 rows]), then the scratch of the two reductions.  pixel_of maps a GEMM
// row to the raster pixel of the output tensor.  Per chunk: "+ add_src" (full resolution, optionally bit-masked, or the
// stride-2 compact tensor), store, and the fused BatchNorm-backward column reduction (bnred.x; 128-row tiles only), whose
// operand chunks (x, act or its mask bits) are fetched BEFORE the staging so the loads fly while the accumulators go through
// LDS.  bn_part: per-channel (sum, sum of squares) of the fp32 accumulators, one row pair per 128 rows.
template <typename ET, int BM, int BN, int NT, typename PixelOf>
__device__ __forceinline__ void igemm_tile_epilogue(const IGemmGeom& g, unsigned short* smem, const f32x16 (&acc)[BM / 64][BN / 64],
                                                    unsigned short* __restrict__ out, const unsigned short* __restrict__ add_src,
                                                    float* __restrict__ bn_part, const BnRedArgs& bnred, int tile_m, int row0,
                                                    int col0, PixelOf pixel_of) {
  constexpr int MI = BM / 64, TNW = BN / 64, WS = NT / 64;
  constexpr int CPT = BM + 4;                                    // staging pitch (elements)
  constexpr int CPR = BN / 8, NIT = (BM * CPR) / NT;             // 16-byte chunks per tile row; chunks per thread
  constexpr int NRG = NT / CPR;                                  // row groups among the threads sharing a column octet
  constexpr int NPRE = BM == 128 ? NIT : 1;
  constexpr int UNR = NT == 512 ? 8 : NRG;                       // unroll of the octet sums (64 terms at NT = 512, BN = 64)
  static_assert(16 % CPR == 0, "copy-out map: 8 or 16 column octets per tile row");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool holds_acc = NT == 256 || wave < 4;
  const int wm = (wave & 3) >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const unsigned short* bx = BM == 128 ? reinterpret_cast<const unsigned short*>(bnred.x) : nullptr;
  const unsigned short* bact = reinterpret_cast<const unsigned short*>(bnred.act);

  uint4 pre_x[NPRE], pre_a[NPRE];
  unsigned pre_m[NPRE];                                          // ReLU mask bits of the chunk (bnred.mask) instead of pre_a
  if (bx) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      int rl, ch;
      copy_unit<WS, CPR>(lane, wave, i, rl, ch);
      const int rr = row0 + rl;
      pre_x[i] = make_uint4(0u, 0u, 0u, 0u);
      pre_a[i] = make_uint4(ET::ONE2, ET::ONE2, ET::ONE2, ET::ONE2);
      pre_m[i] = 0xffu;
      if (rr < g.M) {
        const int64_t off = (int64_t)pixel_of(rr) * g.N + col0 + ch * 8;
        pre_x[i] = *reinterpret_cast<const uint4*>(bx + off);
        if (bnred.mask) pre_m[i] = bnred.mask[off >> 3];
        else if (bact) pre_a[i] = *reinterpret_cast<const uint4*>(bact + off);
      }
    }
  }
  float s1v[TNW], s2v[TNW];
  if (holds_acc && g.epi_scale) {
    // eval-mode BatchNorm folded into the convolution: ReLU here unless the block's residual is still to be added in the copy-out
    const bool relu_now = g.epi_relu && !add_src;
#pragma unroll
    for (int j = 0; j < TNW; ++j) {
      const int cl = wn * (BN / 2) + j * 32 + l31;
      const float sc = g.epi_scale[col0 + cl], sh = g.epi_shift[col0 + cl];
      s1v[j] = 0.f; s2v[j] = 0.f;
#pragma unroll
      for (int i = 0; i < MI; ++i)
        stage_block<ET>(&smem[cl * CPT + wm * (BM / 2) + i * 32 + 4 * kh], acc[i][j], true, sc, sh, relu_now);
    }
  } else if (holds_acc) {
#pragma unroll
    for (int j = 0; j < TNW; ++j) {
      const int cl = wn * (BN / 2) + j * 32 + l31;
      float s1 = 0.f, s2 = 0.f;                                  // rows >= M were zero-filled -> contribute 0
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        colsum_block(acc[i][j], s1, s2);
        stage_block<ET>(&smem[cl * CPT + wm * (BM / 2) + i * 32 + 4 * kh], acc[i][j]);
      }
      colsum_lane_halves(s1, s2);
      s1v[j] = s1; s2v[j] = s2;
    }
  }
  __syncthreads();
  float rs1[8], rs2[8], rmu[8], ris[8];
  if (bx) {
    int rl0, ch0;
    copy_unit<WS, CPR>(lane, wave, 0, rl0, ch0);                 // this thread's column octet is the same in every pass
    const int c0 = col0 + ch0 * 8;
    const int64_t so = bnred.tiles_per_image ? (int64_t)(tile_m / bnred.tiles_per_image) * g.N : 0;   // per-image statistics (IBN)
#pragma unroll
    for (int k = 0; k < 8; k += 4) {
      const float4 a = *reinterpret_cast<const float4*>(bnred.mean + so + c0 + k);
      const float4 b = *reinterpret_cast<const float4*>(bnred.invstd + so + c0 + k);
      rmu[k] = a.x; rmu[k + 1] = a.y; rmu[k + 2] = a.z; rmu[k + 3] = a.w;
      ris[k] = b.x; ris[k + 1] = b.y; ris[k + 2] = b.z; ris[k + 3] = b.w;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { rs1[k] = 0.f; rs2[k] = 0.f; }
  }
  uint4 cv[NIT];
  read_back_chunks<NIT, WS, CPR, CPT>(smem, lane, wave, cv);
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    int rl, ch;
    copy_unit<WS, CPR>(lane, wave, i, rl, ch);
    const int rr = row0 + rl;
    if (rr < g.M) {
      uint4 v = cv[i];
      const int prow = pixel_of(rr);
      const int64_t off = (int64_t)prow * g.N + col0 + ch * 8;
      if (add_src) {
        int64_t aoff = off;
        bool has = true;
        if (g.add_compact) {                                     // the stride-2 downsample branch's gradient, compact
          int ab, arem, ay, ax;
          fast_divmod(prow, g.OH * g.OW, g.inv_ohow, ab, arem);
          fast_divmod(arem, g.OW, g.inv_ow, ay, ax);
          has = ((ay | ax) & 1) == 0;
          aoff = (int64_t)((ab * (g.OH >> 1) + (ay >> 1)) * (g.OW >> 1) + (ax >> 1)) * g.N + col0 + ch * 8;
        }
        if (has) {
          const uint4 a = *reinterpret_cast<const uint4*>(add_src + aoff);
          add_chunk<ET>(v, a, g.epi_relu, g.add_mask ? (unsigned)g.add_mask[aoff >> 3] : 0xffu);
        }
      }
      if (!CREID_ABL_ON(g.abl, 8)) *reinterpret_cast<uint4*>(out + off) = v;
      if (bx) bnred_chunk<ET>(v, pre_x[i % NPRE], pre_a[i % NPRE], pre_m[i % NPRE], rmu, ris, rs1, rs2);   // (NPRE == NIT whenever bx can be non-null)
    }
  }
  if (bx) {
    __syncthreads();                                             // staged C tile no longer needed
    float* red2 = reinterpret_cast<float*>(smem);                // [NRG][2][BN]
    const int cidx = lane >> 2;                                  // unit of the pass; lane & 3 = row of its quad
    const int rg = (wave * 4 + (lane & 3)) * (16 / CPR) + cidx / CPR, cb = (cidx % CPR) * 8;   // threads that share an octet
#pragma unroll
    for (int k = 0; k < 8; ++k) { red2[(rg * 2 + 0) * BN + cb + k] = rs1[k]; red2[(rg * 2 + 1) * BN + cb + k] = rs2[k]; }
    __syncthreads();
    for (int i = tid; i < 2 * BN; i += NT) {
      const int which = i / BN, cl = i - which * BN;
      float a = 0.f;
#pragma unroll UNR
      for (int q = 0; q < NRG; ++q) a += red2[(q * 2 + which) * BN + cl];
      bnred.partial[((int64_t)tile_m * 2 + which) * g.N + col0 + cl] = a;
    }
  }
  if (bn_part) {
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);                 // [2 (wm)][2 (s1, s2)][BN]
    if (holds_acc) {
#pragma unroll
      for (int j = 0; j < TNW; ++j) {
        const int cl = wn * (BN / 2) + j * 32 + l31;
        if (kh == 0) { red[(wm * 2 + 0) * BN + cl] = s1v[j]; red[(wm * 2 + 1) * BN + cl] = s2v[j]; }
      }
    }
    __syncthreads();
    for (int i = tid; i < 2 * BN; i += NT) {
      const int which = i / BN, cl = i - which * BN;
      if constexpr (BM == 128) {
        bn_part[((int64_t)tile_m * 2 + which) * g.N + col0 + cl] = red[(0 * 2 + which) * BN + cl] + red[(1 * 2 + which) * BN + cl];
      } else {                                                   // partial rows stay per 128 rows: one per consumer-wave row half
        bn_part[((int64_t)(tile_m * 2 + 0) * 2 + which) * g.N + col0 + cl] = red[(0 * 2 + which) * BN + cl];
        if (row0 + 128 < g.M) bn_part[((int64_t)(tile_m * 2 + 1) * 2 + which) * g.N + col0 + cl] = red[(1 * 2 + which) * BN + cl];
      }
    }
  }
}

// ------------------------------------------------------------------------------------ bf16, LDS-DMA
// Same tiling as igemm_bf16_kernel, but both operand tiles are fetched with gfx950's
// global->LDS DMA (`global_load_lds_dwordx4`: LDS[wave base + lane*16] <- that lane's 16 global bytes): no
// staging VGPRs, no ds_write pass, ~16 address VALU per k-tile.  The LDS image is linear (8 rows x 128 B per
// wave-instruction); the conflict-free XOR swizzle is applied on the SOURCE side (lane holding LDS chunk c'
// of row r fetches global chunk c' ^ ((r>>1)&7)) and again on the fragment reads.  Out-of-image taps and
// rows >= M fetch from a page of zeros.  NS-stage LDS ring: the DMAs of k-tiles t+1 .. t+NS-2 fly while tile t
// is multiplied; `s_waitcnt vmcnt(n)` with n = the DMA instructions of the younger tiles still in flight; one
// bare s_barrier per k-tile.  Measured (r01, profiles/r01_igemm_stage_sweep.md): NS = 2 wins on every ResNet50
// layer -- the loop is not DMA-latency bound, and 3+ stages cost a workgroup per CU.
template <int BN, int NS, typename ET = Bf16T>
__global__ __launch_bounds__(256, (NS * (128 + BN) * 128 <= 80 * 1024) ? 2 : 1) void igemm_bf16_dma_kernel(IGemmGeom g, const unsigned short* __restrict__ src,
                                                                 const unsigned short* __restrict__ wgt,
                                                                 unsigned short* __restrict__ out,
                                                                 const unsigned short* __restrict__ add_src,
                                                                 float* __restrict__ bn_part, int tiles_n,
                                                                 BnRedArgs bnred) {
  constexpr int BK = 64, TNW = BN / 64, NBI = BN / 32;          // NBI = B-tile DMA instructions per wave
  constexpr int CPT = 128 + 4;                                   // C staging pitch (igemm_tile_epilogue)
  constexpr int TILE_A = 128 * BK, TILE_B = BN * BK, STAGE = TILE_A + TILE_B;
  constexpr int LDS_ELEMS = (NS * STAGE) > (BN * CPT) ? (NS * STAGE) : (BN * CPT);
  constexpr int LPT = 4 + NBI;                                   // DMA instructions per wave per k-tile
  static_assert((NS - 2) * LPT <= 63, "vmcnt is a 6-bit counter");
  __shared__ __attribute__((aligned(1024))) unsigned short smem[LDS_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
  const int row0 = tile_m * 128, col0 = tile_n * BN;
  const int span_mask = (1 << g.log2span) - 1;

  // DMA lane map: instruction i of this wave covers tile rows ((i*4 + wave)*8 .. +7); lane -> (row, LDS chunk)
  const int lr8 = lane >> 3, lcp = lane & 7;
  int oy[4], ox[4], bpix[4], gch[4];
  bool vm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (i * 4 + wave) * 8 + lr8, m = row0 + r;
    vm[i] = m < g.M;
    const int mm = vm[i] ? m : 0;
    int b, rem;
    fast_divmod(mm, g.OH * g.OW, g.inv_ohow, b, rem);
    fast_divmod(rem, g.OW, g.inv_ow, oy[i], ox[i]);
    bpix[i] = b * g.SH * g.SW;
    gch[i] = (lcp ^ ((r >> 1) & 7)) << 3;                     // swizzled SOURCE chunk (elements)
  }
  const unsigned short* wp[NBI];
#pragma unroll
  for (int i = 0; i < NBI; ++i) {
    const int r = (i * 4 + wave) * 8 + lr8;
    wp[i] = wgt + (int64_t)(col0 + r) * g.K + ((lcp ^ ((r >> 1) & 7)) << 3);
  }
  const unsigned short* aptr[4];
  int amul[4];
  int cur_tap = -1, cur_r = 0, cur_s = -1;                     // taps are visited in order: (r, s) advance incrementally
  const unsigned short* zpage = reinterpret_cast<const unsigned short*>(g_zero_page);
  auto set_tap = [&]() {
    if (++cur_s == g.kw) { cur_s = 0; ++cur_r; }
    const int r = cur_r, s = cur_s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int iy, ix;
      const bool ok = vm[i] && igemm_src_pixel(g, oy[i], ox[i], r, s, iy, ix);
      aptr[i] = ok ? src + (int64_t)(bpix[i] + iy * g.SW + ix) * g.pitch + gch[i] : zpage;
      amul[i] = ok ? 1 : 0;
    }
  };
  typedef const void __attribute__((address_space(1)))* gptr_t;
  typedef void __attribute__((address_space(3)))* lptr_t;
  // The stem (7x7 s2 on the pre-padded NHWC4 image): a tap is one kernel row = 32 elements = 64 bytes, so a
  // 64-wide k-tile holds TWO taps; source chunk sc of the 128-byte tile row comes from kernel row 2t + (sc >> 2)
  // at byte offset (sc & 3) * 16.  No bounds checks (padding), the pointer just advances two image rows per k-tile.
  const bool stem = g.log2span == 5;
  const int stem_step = 2 * g.SW * g.pitch;
  if (stem) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int sc = gch[i] >> 3;
      aptr[i] = vm[i] ? src + (int64_t)(bpix[i] + (oy[i] * 2 + (sc >> 2)) * g.SW + ox[i] * 2) * g.pitch + (sc & 3) * 8 : zpage;
      amul[i] = vm[i] ? 1 : 0;
    }
  }
  auto issue = [&](int t, int buf) {
    // running pointers: inside a tap every k-tile advances the A rows by 64 channels (0 for the zero page), the
    // stem by two image rows, the weight rows by 64 columns -- no per-tile multiplies
    if (!stem) {
      const int tap = (t * BK) >> g.log2span;
      if (tap != cur_tap) { set_tap(); cur_tap = tap; }
    }
    unsigned short* la = smem + buf * STAGE + wave * 512;      // + i * 2048 elements (4 KiB) per instruction
    unsigned short* lb = smem + buf * STAGE + TILE_A + wave * 512;
    const int a_step = stem ? stem_step : BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_global_load_lds((gptr_t)aptr[i], (lptr_t)(la + i * 2048), 16, 0, 0);
      aptr[i] += amul[i] ? a_step : 0;
    }
#pragma unroll
    for (int i = 0; i < NBI; ++i) {
      __builtin_amdgcn_global_load_lds((gptr_t)wp[i], (lptr_t)(lb + i * 2048), 16, 0, 0);
      wp[i] += BK;
    }
  };

  f32x16 acc[2][TNW];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TNW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = g.K / BK;
  const int l31 = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int p = 0; p < NS - 1; ++p)
    if (p < nk) issue(p, p);
  int buf = 0;                                                 // t % NS
  for (int t = 0; t < nk; ++t) {
    // this wave's DMA pieces of tile t have landed once at most the younger tiles' instructions are pending
    const int younger = min(nk - 1 - t, NS - 2);
    if constexpr (NS >= 5) { if (younger == 3) wait_vm<3 * LPT>(); }
    if constexpr (NS >= 4) { if (younger == 2) wait_vm<2 * LPT>(); }
    if constexpr (NS >= 3) { if (younger == 1) wait_vm<1 * LPT>(); }
    if (younger == 0) wait_vm<0>();
    // bare s_barrier: __syncthreads() carries a release fence that drains vmcnt to 0, i.e. the whole ring.
    // LDS-DMA data is visible once vmcnt has counted it; this wave's ds_reads of tile t-1 were consumed by MFMAs.
    asm volatile("s_barrier" ::: "memory");                    // everyone's pieces landed; buffer (t-1)%NS is free
    if (t + NS - 1 < nk) issue(t + NS - 1, buf == 0 ? NS - 1 : buf - 1);
    const unsigned short* As = smem + buf * STAGE;
    buf = (buf + 1 == NS) ? 0 : buf + 1;
    const unsigned short* Bs = As + TILE_A;
    // All fragment reads of the k-tile are issued before the first MFMA (the compiler then waits with
    // decreasing lgkmcnt): with a read->wait->MFMA chain per 16-wide k slice the LDS latency was exposed four
    // times per k-tile and a wave kept its MFMA pipe ~16% busy.
    s16x8 a[4][2], b[4][TNW];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ch = 2 * kk + kh;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = wm * 64 + i * 32 + l31;
        a[kk][i] = *reinterpret_cast<const s16x8*>(&As[r * BK + ((ch ^ ((r >> 1) & 7)) << 3)]);
      }
#pragma unroll
      for (int j = 0; j < TNW; ++j) {
        const int c = wn * (BN / 2) + j * 32 + l31;
        b[kk][j] = *reinterpret_cast<const s16x8*>(&Bs[c * BK + ((ch ^ ((c >> 1) & 7)) << 3)]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TNW; ++j)
          acc[i][j] = ET::mfma(a[kk][i], b[kk][j], acc[i][j]);
  }
  __syncthreads();

  igemm_tile_epilogue<ET, 128, BN, 256>(g, smem, acc, out, add_src, bn_part, bnred, tile_m, row0, col0, [](int rr) { return rr; });
}

// ------------------------------------------------------------------------------------ bf16, warp-specialised
// Measured on MI355X (r01, tools/probes/lds_fill_bw_probe.hip + loop ablations): in igemm_bf16_dma_kernel a
// k-tile costs ~0.5 us of DMA *issue* time (each global_load_lds_dwordx4 holds the issuing wave for 60-180
// cycles) plus ~0.4 us of ds_read + MFMA time, and because the same four waves do both, the two mostly add up.
// Here a 512-thread workgroup splits the roles: waves 0-3 (consumers, 2x2 over the 128 x BN tile) only read
// fragments and issue MFMAs; waves 4-7 (producers) only compute gather addresses and issue the LDS-DMA pieces
// into an NS-deep LDS ring.  One s_barrier per k-tile couples them:
//   barrier B_t  <=  producers: their pieces of tile t have landed (vmcnt);  consumers: done reading tile t-1
//   after B_t    :   producers issue tile t+NS-1 into slot (t-1)%NS, consumers multiply tile t.
// Tiling, swizzle, zero page and the epilogue are those of igemm_bf16_dma_kernel (all 512 threads copy out).
// BM = 128: the consumer waves hold 64 x BN/2 sub-tiles (two workgroups per CU where the ring allows it; THREE for the
// 128 x 64 tile with a 2-deep ring: 48 KB of LDS, and the register allocator is held to 80 VGPRs (it needs 76) -- measured
// -0.06 ms per step on the rule-selected schedule, round 3).  BM = 256: 128 x BN/2
// sub-tiles -- 0.75 instead of 1 fragment read per MFMA and 1.125 instead of 1.5 KB of LDS traffic per MFMA; one workgroup
// per CU (the ring is 48 KB per stage), so only for grids that still fill the chip with 256-row tiles.
template <int BN, int NS, int BM = 128, typename ET = Bf16T>
__global__ __launch_bounds__(512, (BN == 64 && NS == 2 && BM == 128) ? 6 : ((NS * (BM + BN) * 128 <= 80 * 1024) ? 2 : 1)) void igemm_bf16_ws_kernel(IGemmGeom g, const unsigned short* __restrict__ src,
                                                                const unsigned short* __restrict__ wgt,
                                                                unsigned short* __restrict__ out,
                                                                const unsigned short* __restrict__ add_src,
                                                                float* __restrict__ bn_part, int tiles_n,
                                                                BnRedArgs bnred, WRedJob wred) {
  constexpr int NT = 512;
  constexpr int BK = 64, TNW = BN / 64, NBI = BN / 32;
  constexpr int MI = BM / 64, NAI = BM / 32;                     // 32-row blocks per consumer wave; A-tile DMA instructions per producer wave
  constexpr int CPT = BM + 4;                                    // transposed staging: [BN columns][BM rows + 4]
  constexpr int TILE_A = BM * BK, TILE_B = BN * BK, STAGE = TILE_A + TILE_B;
  constexpr int CPR = BN / 8, NRG = NT / CPR;
  constexpr int RED_ELEMS = NRG * 2 * BN * 2;                    // fp32 reduction scratch, in 2-byte units
  constexpr int LDS0 = (NS * STAGE) > (BN * CPT) ? (NS * STAGE) : (BN * CPT);
  constexpr int LDS_ELEMS = LDS0 > RED_ELEMS ? LDS0 : RED_ELEMS;
  constexpr int LPT = NAI + NBI;
  static_assert(NS >= 2 && (NS - 2) * LPT <= 63, "ring depth");
  static_assert(BM == 128 || BM == 256, "row tile");
  __shared__ __attribute__((aligned(1024))) unsigned short smem[LDS_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // piggybacked job: the LAST wred.nblocks workgroups sum the split partials of the PREVIOUS weight-gradient launch
  // instead of computing a tile.  Workgroups are dispatched in order, so these start when the final wave of tiles
  // is running and fill the CUs that wave leaves idle (placed first they held every workgroup slot for ~10 us and
  // delayed the tiles: measured, no gain over the stand-alone launch).
  const int nred = wred.ws ? wred.nblocks : 0;
  const int ntile_wgs = (int)gridDim.x - nred;
  if ((int)blockIdx.x >= ntile_wgs) {
    wgrad_reduce_block<NT>(wred, (int)blockIdx.x - ntile_wgs, reinterpret_cast<float*>(smem));
    return;
  }
  const bool producer = wave >= 4;
  const int cw = wave & 3;                                       // role-local wave index
  const int wm = cw >> 1, wn = cw & 1;
  const int bid = xcd_remap((int)blockIdx.x, ntile_wgs);
  const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
  const int row0 = tile_m * BM, col0 = tile_n * BN;
  const int l31 = lane & 31, kh = lane >> 5;
  // parity-class row order (g.parity): the tile's class fixes which taps exist; r, s step by 2 from (r0, s0)
  const int msub = g.M >> 2;
  const int cls = g.parity ? row0 / msub : 0, py = cls >> 1, px = cls & 1;
  const int tstep = g.parity ? 2 : 1;
  const int r0 = g.parity ? ((py + g.pad) & 1) : 0, s0 = g.parity ? ((px + g.pad) & 1) : 0;
  const int kh_taps = (g.K >> g.log2span) / g.kw;                 // kernel rows
  const int nk = g.parity ? ((kh_taps - r0 + 1) / 2) * ((g.kw - s0 + 1) / 2) * ((1 << g.log2span) / BK) : g.K / BK;
  // GEMM row -> raster pixel index of the output tensor (identity unless parity-class order)
  auto pixel_of = [&](int rr) -> int {
    if (!g.parity) return rr;
    const int rem2 = rr - cls * msub;
    int b, rem, a, c;
    fast_divmod(rem2, (g.OH >> 1) * (g.OW >> 1), g.inv_ohow * 4.f, b, rem);
    fast_divmod(rem, g.OW >> 1, g.inv_ow * 2.f, a, c);
    return (b * g.OH + 2 * a + py) * g.OW + 2 * c + px;
  };

  f32x16 acc[MI][TNW];
  if (producer) {
    const int span_mask = (1 << g.log2span) - 1;
    const int lr8 = lane >> 3, lcp = lane & 7;
    int oy[NAI], ox[NAI], bpix[NAI], gch[NAI];
    bool vm[NAI];
#pragma unroll
    for (int i = 0; i < NAI; ++i) {
      const int r = (i * 4 + cw) * 8 + lr8, m = row0 + r;
      vm[i] = m < g.M;
      const int mm = vm[i] ? m : row0;
      const int pix = pixel_of(mm);
      int b, rem;
      fast_divmod(pix, g.OH * g.OW, g.inv_ohow, b, rem);
      fast_divmod(rem, g.OW, g.inv_ow, oy[i], ox[i]);
      bpix[i] = b * g.SH * g.SW;
      gch[i] = (lcp ^ ((r >> 1) & 7)) << 3;
    }
    const unsigned short* wp[NBI];
    const unsigned short* wbase[NBI];
#pragma unroll
    for (int i = 0; i < NBI; ++i) {
      const int r = (i * 4 + cw) * 8 + lr8;
      wbase[i] = wgt + (int64_t)(col0 + r) * g.K + ((lcp ^ ((r >> 1) & 7)) << 3);
      wp[i] = wbase[i];
    }
    const unsigned short* aptr[NAI];
    int amul[NAI];
    int cur_tap = -1, cur_r = r0, cur_s = s0 - tstep;
    const unsigned short* zpage = reinterpret_cast<const unsigned short*>(g_zero_page);
    typedef const void __attribute__((address_space(1)))* gptr_t;
    typedef void __attribute__((address_space(3)))* lptr_t;
    auto issue = [&](int t, int buf) {
      if (CREID_ABL_ON(g.abl, 2) && t > 0) return;
      const int tap = (t * BK) >> g.log2span;
      if (tap != cur_tap) {
        cur_tap = tap;
        cur_s += tstep;
        if (cur_s >= g.kw) { cur_s = s0; cur_r += tstep; }
        if (g.parity) {
#pragma unroll
          for (int i = 0; i < NBI; ++i) wp[i] = wbase[i] + ((cur_r * g.kw + cur_s) << g.log2span);
        }
#pragma unroll
        for (int i = 0; i < NAI; ++i) {
          int iy, ix;
          const bool ok = vm[i] && igemm_src_pixel(g, oy[i], ox[i], cur_r, cur_s, iy, ix);
          aptr[i] = ok ? src + (int64_t)(bpix[i] + iy * g.SW + ix) * g.pitch + gch[i] : zpage;
          amul[i] = ok ? 1 : 0;
        }
      }
      unsigned short* la = smem + buf * STAGE + cw * 512;
      unsigned short* lb = smem + buf * STAGE + TILE_A + cw * 512;
#pragma unroll
      for (int i = 0; i < NAI; ++i) {
        __builtin_amdgcn_global_load_lds((gptr_t)aptr[i], (lptr_t)(la + i * 2048), 16, 0, 0);
        aptr[i] += amul[i] ? BK : 0;                             // running pointers
      }
#pragma unroll
      for (int i = 0; i < NBI; ++i) {
        __builtin_amdgcn_global_load_lds((gptr_t)wp[i], (lptr_t)(lb + i * 2048), 16, 0, 0);
        wp[i] += BK;
      }
    };
#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
      if (p < nk) issue(p, p);
    int buf = 0;
    for (int t = 0; t < nk; ++t) {
      const int younger = min(nk - 1 - t, NS - 2);
      if constexpr (NS >= 5) { if (younger == 3) wait_vm<3 * LPT>(); }
      if constexpr (NS >= 4) { if (younger == 2) wait_vm<2 * LPT>(); }
      if constexpr (NS >= 3) { if (younger == 1) wait_vm<1 * LPT>(); }
      if (younger == 0) wait_vm<0>();
      asm volatile("s_barrier" ::: "memory");                    // B_t
      if (t + NS - 1 < nk) issue(t + NS - 1, buf == 0 ? NS - 1 : buf - 1);
      buf = (buf + 1 == NS) ? 0 : buf + 1;
    }
  } else {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < TNW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    int buf = 0;
    for (int t = 0; t < nk; ++t) {
      asm volatile("s_barrier" ::: "memory");                    // B_t: tile t is in LDS
      const unsigned short* As = smem + buf * STAGE;
      const unsigned short* Bs = As + TILE_A;
      buf = (buf + 1 == NS) ? 0 : buf + 1;
      // fragment reads run one 16-wide k slice ahead of the MFMAs (register double buffer): the LDS latency of
      // slice kk+1 hides behind the MFMAs of slice kk instead of being exposed four times per k-tile
      s16x8 a[2][MI], b[2][TNW];
      auto load_frags = [&](int kk, int sl) {
        const int ch = 2 * kk + kh;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const int r = wm * (BM / 2) + i * 32 + l31;
          a[sl][i] = *reinterpret_cast<const s16x8*>(&As[r * BK + ((ch ^ ((r >> 1) & 7)) << 3)]);
        }
#pragma unroll
        for (int j = 0; j < TNW; ++j) {
          const int c = wn * (BN / 2) + j * 32 + l31;
          b[sl][j] = *reinterpret_cast<const s16x8*>(&Bs[c * BK + ((ch ^ ((c >> 1) & 7)) << 3)]);
        }
      };
      auto mma = [&](int sl) {
        if (CREID_ABL_ON(g.abl, 1)) return;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < TNW; ++j)
            acc[i][j] = ET::mfma(a[sl][i], b[sl][j], acc[i][j]);
      };
      if (CREID_ABL_ON(g.abl, 4)) continue;
      load_frags(0, 0);
      __builtin_amdgcn_sched_barrier(0);
      load_frags(1, 1); mma(0);
      __builtin_amdgcn_sched_barrier(0);
      load_frags(2, 0); mma(1);
      __builtin_amdgcn_sched_barrier(0);
      load_frags(3, 1); mma(0);
      __builtin_amdgcn_sched_barrier(0);
      mma(1);
    }
  }
  __syncthreads();

  igemm_tile_epilogue<ET, BM, BN, NT>(g, smem, acc, out, add_src, bn_part, bnred, tile_m, row0, col0, pixel_of);
}

// ------------------------------------------------------------------------------------ bf16, resident halo tile
// The stride-1 3 x 3 convolutions (forward and data gradient) whose 128-row tile is whole image rows of one image: the nine
// taps of such a tile read the same (128 / OW + 2) x (OW + 2) source pixels shifted by one, and the producer/consumer kernel
// above sends them through the global->LDS DMA nine times (the LDS fill, not the MFMA, sets its k-tile time).  Here the
// producer waves DMA that halo image ONCE, in the prologue, and only the weight tiles stream through the NS-deep ring.
//   halo image : C / 64 planes of [slot][64 channels] (the 128-byte row format of an A stage); slot = hr * (OW + 2) + hc holds
//                source pixel (y0 - 1 + hr, hc - 1) of the tile's image, y0 = the tile's first image row; slots outside the
//                image (and the padding up to whole DMA pieces) are filled from the zero page.  The 16-byte chunk index is
//                XOR-swizzled by key(hr, hc) = ((hc >> 1) + (OW == 8 ? 4 * hr : 0)) & 7: the 16 lanes of a ds_read_b128
//                group then hit 16 different (slot parity, chunk) bank groups under every tap shift (OW >= 32: one halo row
//                per 32 lanes; OW = 16: two rows, equal columns 16 apart; OW = 8: four rows, + 4 per row separates them).
//   fill       : a DMA instruction writes 8 consecutive slots of one plane; every producer wave issues HALO_PW pieces per
//                plane (so the vmcnt bookkeeping is the same in all four).  Order: plane 0, weight tiles 0 .. NS-2, planes
//                1 .. P-1 -- k-tile t < P needs plane t only, so the first multiplies start after about the bytes of
//                today's first k-tile and the other planes land behind them.
//   k-loop     : tap-major, 64-wide k-tiles inside a tap (plane kc), 16-wide slices, one accumulation chain per sub-tile --
//                the order of the tile kernels, so every output bit is theirs.  Row r of the tile under tap (tr, ts) reads
//                slot (r / OW + dr) * (OW + 2) + r % OW + dc, (dr, dc) = (tr, ts) forward, (2 - tr, 2 - ts) transposed.
// Consumer sub-tiles, C staging and the epilogue (igemm_tile_epilogue), and the piggy-backed split reduction are those of
// igemm_bf16_ws_kernel<BN, NS, 128>.
constexpr int halo_pw(int C) { return C == 64 ? 9 : 6; }                 // DMA pieces per producer wave per plane (36 / 24 KB planes)
constexpr int halo_lds_bytes(int C, int BN, int NS) { return ((C / 64) * 4 * halo_pw(C) * 512 + NS * BN * 64) * 2; }

template <int C, int BN, int NS, typename ET = Bf16T>
__global__ __launch_bounds__(512, halo_lds_bytes(C, BN, NS) <= 80 * 1024 ? 2 : 1) void igemm_bf16_halo_kernel(IGemmGeom g, const unsigned short* __restrict__ src,
                                                                const unsigned short* __restrict__ wgt,
                                                                unsigned short* __restrict__ out,
                                                                const unsigned short* __restrict__ add_src,
                                                                float* __restrict__ bn_part, int tiles_n,
                                                                BnRedArgs bnred, WRedJob wred) {
  constexpr int NT = 512, BM = 128;
  constexpr int BK = 64, TNW = BN / 64, NBI = BN / 32, MI = 2;
  constexpr int P = C / 64, PW = halo_pw(C);                    // planes; halo pieces per producer wave per plane
  constexpr int PLANE = 4 * PW * 512, HALO = P * PLANE;          // elements
  constexpr int CPT = BM + 4;
  constexpr int TILE_B = BN * BK;
  constexpr int CPR = BN / 8, NRG = NT / CPR;
  constexpr int RED_ELEMS = NRG * 2 * BN * 2;
  constexpr int LDS0 = (HALO + NS * TILE_B) > (BN * CPT) ? (HALO + NS * TILE_B) : (BN * CPT);
  constexpr int LDS_ELEMS = LDS0 > RED_ELEMS ? LDS0 : RED_ELEMS;
  static_assert(C == 64 || C == 128 || C == 256, "channels per tap");
  static_assert(NS >= 2 && NS <= 4, "ring depth");
  static_assert(LDS_ELEMS * 2 < 160 * 1024, "halo image + weight ring must fit the LDS");
  static_assert(sizeof(float) * (4 * 512 + 8192) <= LDS_ELEMS * 2, "reduce scratch of the piggy-backed job");
  static_assert((NS - 2) * NBI + (P - 1) * PW <= 63, "vmcnt is a 6-bit counter");
  __shared__ __attribute__((aligned(1024))) unsigned short smem[LDS_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nred = wred.ws ? wred.nblocks : 0;                   // (as in igemm_bf16_ws_kernel: the LAST workgroups reduce)
  const int ntile_wgs = (int)gridDim.x - nred;
  if ((int)blockIdx.x >= ntile_wgs) {
    wgrad_reduce_block<NT>(wred, (int)blockIdx.x - ntile_wgs, reinterpret_cast<float*>(smem));
    return;
  }
  const bool producer = wave >= 4;
  const int cw = wave & 3;
  const int wm = cw >> 1, wn = cw & 1;
  const int bid = xcd_remap((int)blockIdx.x, ntile_wgs);
  const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
  const int row0 = tile_m * BM, col0 = tile_n * BN;
  const int l31 = lane & 31, kh = lane >> 5;
  const int hp = g.OW + 2;                                       // halo row pitch (slots)
  const int kmul = g.OW == 8 ? 4 : 0;                            // swizzle key: + 4 per halo row where a lane group spans four rows
  constexpr int nk = 9 * P;

  f32x16 acc[MI][TNW];
  if (producer) {
    const int lr8 = lane >> 3, lcp = lane & 7;
    const int ohow = g.OH * g.OW;
    const int img = row0 / ohow, y0 = (row0 - img * ohow) / g.OW;   // the tile: rows y0 .. y0 + 128 / OW - 1 of image img
    const int nslot = (BM / g.OW + 2) * hp;
    const float inv_hp = 1.0f / (float)hp;
    const unsigned short* zpage = reinterpret_cast<const unsigned short*>(g_zero_page);
    typedef const void __attribute__((address_space(1)))* gptr_t;
    typedef void __attribute__((address_space(3)))* lptr_t;
    const unsigned short* hptr[PW];
    int hstep[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) {                               // plane 0; piece j of this wave = slots (j * 4 + cw) * 8 .. + 7
      const int slot = (j * 4 + cw) * 8 + lr8;
      int hr, hc;
      fast_divmod(slot, hp, inv_hp, hr, hc);
      const int iy = y0 - 1 + hr, ix = hc - 1;
      const bool ok = slot < nslot && (unsigned)iy < (unsigned)g.SH && (unsigned)ix < (unsigned)g.SW;
      const int key = ((hc >> 1) + kmul * hr) & 7;
      hptr[j] = ok ? src + (int64_t)((img * g.SH + iy) * g.SW + ix) * g.pitch + ((lcp ^ key) << 3) : zpage;
      hstep[j] = ok ? BK : 0;
      __builtin_amdgcn_global_load_lds((gptr_t)hptr[j], (lptr_t)(smem + (j * 4 + cw) * 512), 16, 0, 0);
    }
    const unsigned short* wp[NBI];
#pragma unroll
    for (int i = 0; i < NBI; ++i) {
      const int r = (i * 4 + cw) * 8 + lr8;
      wp[i] = wgt + (int64_t)(col0 + r) * g.K + ((lcp ^ ((r >> 1) & 7)) << 3);
    }
    auto issue = [&](int buf) {                                  // the next weight tile (running pointers)
      unsigned short* lb = smem + HALO + buf * TILE_B + cw * 512;
#pragma unroll
      for (int i = 0; i < NBI; ++i) {
        __builtin_amdgcn_global_load_lds((gptr_t)wp[i], (lptr_t)(lb + i * 2048), 16, 0, 0);
        wp[i] += BK;
      }
    };
#pragma unroll
    for (int p = 0; p < NS - 1; ++p) issue(p);
#pragma unroll
    for (int p = 1; p < P; ++p)
#pragma unroll
      for (int j = 0; j < PW; ++j) {
        hptr[j] += hstep[j];
        __builtin_amdgcn_global_load_lds((gptr_t)hptr[j], (lptr_t)(smem + p * PLANE + (j * 4 + cw) * 512), 16, 0, 0);
      }
    // instructions still allowed in flight at B_t while planes are landing (t < P): behind plane t (and weight tile t, issued
    // before plane 1 when t <= NS - 2) come the planes t + 1 .. P - 1 and the t weight tiles issued inside the loop so far
    constexpr int W0 = (NS - 2) * NBI + (P - 1) * PW;
    constexpr int W1 = (P > 2 ? (P - 2) * PW : 0) + NBI;
    constexpr int W2 = (P > 3 ? (P - 3) * PW : 0) + 2 * NBI;
    int buf = 0;
    for (int t = 0; t < nk; ++t) {
      if (P > 1 && t == 0) wait_vm<W0>();
      else if (P > 1 && t == 1 && NS >= 3) wait_vm<W1>();
      else if (P > 2 && t == 2 && NS >= 4) wait_vm<W2>();
      else {
        const int younger = min(nk - 1 - t, NS - 2);
        if constexpr (NS >= 4) { if (younger == 2) wait_vm<2 * NBI>(); }
        if constexpr (NS >= 3) { if (younger == 1) wait_vm<1 * NBI>(); }
        if (younger == 0) wait_vm<0>();
      }
      asm volatile("s_barrier" ::: "memory");                    // B_t
      if (t + NS - 1 < nk) issue(buf == 0 ? NS - 1 : buf - 1);
      buf = (buf + 1 == NS) ? 0 : buf + 1;
    }
  } else {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < TNW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int log2ow = 31 - __clz(g.OW);
    int hr0[MI], hc0[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int r = wm * (BM / 2) + i * 32 + l31;
      hr0[i] = r >> log2ow; hc0[i] = r & (g.OW - 1);
    }
    int buf = 0, tr = 0, ts = 0;
    for (int tap = 0; tap < 9; ++tap) {
      const int dr = g.transposed ? 2 - tr : tr, dc = g.transposed ? 2 - ts : ts;
      int aoff[MI], kx[MI];                                      // this tap's slot (elements) and swizzle key ^ k half, per row block
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int hr = hr0[i] + dr, hc = hc0[i] + dc;
        aoff[i] = (hr * hp + hc) * BK;
        kx[i] = (((hc >> 1) + kmul * hr) & 7) ^ kh;
      }
      if (++ts == 3) { ts = 0; ++tr; }
#pragma unroll
      for (int kc = 0; kc < P; ++kc) {
        asm volatile("s_barrier" ::: "memory");                  // B_t, t = tap * P + kc: weight tile t (and plane kc) is in LDS
        const unsigned short* As = smem + kc * PLANE;
        const unsigned short* Bs = smem + HALO + buf * TILE_B;
        buf = (buf + 1 == NS) ? 0 : buf + 1;
        s16x8 a[2][MI], b[2][TNW];
        auto load_frags = [&](int kk, int sl) {
          const int ch = 2 * kk + kh;
#pragma unroll
          for (int i = 0; i < MI; ++i)
            a[sl][i] = *reinterpret_cast<const s16x8*>(&As[aoff[i] + (((2 * kk) ^ kx[i]) << 3)]);
#pragma unroll
          for (int j = 0; j < TNW; ++j) {
            const int c = wn * (BN / 2) + j * 32 + l31;
            b[sl][j] = *reinterpret_cast<const s16x8*>(&Bs[c * BK + ((ch ^ ((c >> 1) & 7)) << 3)]);
          }
        };
        auto mma = [&](int sl) {
          if (CREID_ABL_ON(g.abl, 1)) return;
#pragma unroll
          for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < TNW; ++j)
              acc[i][j] = ET::mfma(a[sl][i], b[sl][j], acc[i][j]);
        };
        load_frags(0, 0);
        __builtin_amdgcn_sched_barrier(0);
        load_frags(1, 1); mma(0);
        __builtin_amdgcn_sched_barrier(0);
        load_frags(2, 0); mma(1);
        __builtin_amdgcn_sched_barrier(0);
        load_frags(3, 1); mma(0);
        __builtin_amdgcn_sched_barrier(0);
        mma(1);
      }
    }
  }
  __syncthreads();

  igemm_tile_epilogue<ET, BM, BN, NT>(g, smem, acc, out, add_src, bn_part, bnred, tile_m, row0, col0, [](int rr) { return rr; });
}

// ------------------------------------------------------------------------------------ f32
template <int BN>
__global__ __launch_bounds__(256) void igemm_f32_kernel(IGemmGeom g, const float* __restrict__ src,
                                                        const float* __restrict__ wgt, float* __restrict__ out,
                                                        const float* __restrict__ add_src,
                                                        float* __restrict__ bn_part, int tiles_n) {
  // LDS operand image of a 16-deep k-tile (the same as dist.hip's fp32 distance kernel): [kh = k & 1][half = k >> 3][row][4] -- the
  // per-lane MFMA operand is A[i = lane & 31][k = 2 step + (lane >> 5)], so four consecutive steps' values are one 16-byte unit
  // (ds_read_b128) and a staged float4 is two 8-byte writes ((x, z) -> kh 0, (y, w) -> kh 1).  The k order of the accumulation is
  // the sequential one of rounds 1-5: results unchanged.
  constexpr int BK = 16, PA = 128 * 4 + 16, PB = BN * 4 + 16, TNW = BN / 64, NB = BN / 64;
  __shared__ __attribute__((aligned(16))) float As[2][2][2][PA];
  __shared__ __attribute__((aligned(16))) float Bs[2][2][2][PB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
  const int row0 = tile_m * 128, col0 = tile_n * BN;
  const int span_mask = (1 << g.log2span) - 1;

  const int lrow = tid >> 2, lkc = tid & 3;
  int oy[2], ox[2], bpix[2];
  bool vm[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = row0 + lrow + 64 * i;
    vm[i] = m < g.M;
    const int mm = vm[i] ? m : 0;
    const int b = mm / (g.OH * g.OW), rem = mm - b * (g.OH * g.OW);
    oy[i] = rem / g.OW; ox[i] = rem - oy[i] * g.OW;
    bpix[i] = b * g.SH * g.SW;
  }
  const float* wp[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) wp[i] = wgt + (int64_t)(col0 + lrow + 64 * i) * g.K + 4 * lkc;
  float4 ra[2], rb[NB];
  unsigned amask[2] = {0u, 0u};                    // all ones where the staged tap is a real pixel (else the tile gets zeros)
  auto gload = [&](int t) {                        // branch-free: an absent tap reads the tensor's first element and is masked in lstore
    const int kk = t * BK + 4 * lkc;
    const int tap = kk >> g.log2span, c = kk & span_mask;
    const int r = tap / g.kw, s = tap - r * g.kw;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int iy, ix;
      const bool ok = vm[i] && igemm_src_pixel(g, oy[i], ox[i], r, s, iy, ix);
      amask[i] = ok ? 0xffffffffu : 0u;
      const int64_t off = ok ? (int64_t)(bpix[i] + iy * g.SW + ix) * g.pitch + c : 0;
      ra[i] = *reinterpret_cast<const float4*>(src + off);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) rb[i] = *reinterpret_cast<const float4*>(wp[i] + t * BK);
  };
  const int sh = lkc >> 1, so = lrow * 4 + 2 * (lkc & 1);          // global k = 4 lkc + {0..3}: steps 2 lkc, 2 lkc + 1
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      auto mk = [&](float v) { return __uint_as_float(__float_as_uint(v) & amask[i]); };
      *reinterpret_cast<float2*>(&As[buf][0][sh][so + 256 * i]) = make_float2(mk(ra[i].x), mk(ra[i].z));
      *reinterpret_cast<float2*>(&As[buf][1][sh][so + 256 * i]) = make_float2(mk(ra[i].y), mk(ra[i].w));
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      *reinterpret_cast<float2*>(&Bs[buf][0][sh][so + 256 * i]) = make_float2(rb[i].x, rb[i].z);
      *reinterpret_cast<float2*>(&Bs[buf][1][sh][so + 256 * i]) = make_float2(rb[i].y, rb[i].w);
    }
  };
  f32x16 acc[2][TNW];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TNW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int nk = g.K / BK;
  const int l31 = lane & 31, kh = lane >> 5;
  const int fa = (wm * 64 + l31) * 4, fb = (wn * (BN / 2) + l31) * 4;
  // Two-phase k-loop (round 6, from the evaluation's distance kernels): 8 TNW MFMAs (64 cycles each) per phase with everything
  // else issued in their shadow -- phase 1: the second half's fragment reads + the LDS writes of the next k-tile, barrier,
  // phase 2: the global loads of the k-tile after that + the next k-tile's first-half fragment reads.  (Before: reads, MFMAs,
  // writes, barrier in sequence per k-tile; the two waves a SIMD holds fell into step and the matrix pipe idled with them.)
  float4 a0[2], b0[TNW], a1[2], b1[TNW];
  auto frag = [&](int buf, int half, float4 (&a)[2], float4 (&b)[TNW]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const float4*>(&As[buf][kh][half][fa + 128 * i]);
#pragma unroll
    for (int j = 0; j < TNW; ++j) b[j] = *reinterpret_cast<const float4*>(&Bs[buf][kh][half][fb + 128 * j]);
  };
  auto mma = [&](const float4 (&a)[2], const float4 (&b)[TNW]) {   // steps in k order: 4 half + s4 multiplies k = 2 step + kh
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      float av[2], bv[TNW];
#pragma unroll
      for (int i = 0; i < 2; ++i) { const float c4[4] = {a[i].x, a[i].y, a[i].z, a[i].w}; av[i] = c4[s4]; }
#pragma unroll
      for (int j = 0; j < TNW; ++j) { const float c4[4] = {b[j].x, b[j].y, b[j].z, b[j].w}; bv[j] = c4[s4]; }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TNW; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  };
  gload(0);
  lstore(0);
  __syncthreads();
  gload(nk > 1 ? 1 : 0);
  frag(0, 0, a0, b0);
  for (int t = 0; t + 1 < nk; ++t) {
    const int buf = t & 1;
    __builtin_amdgcn_sched_barrier(0);
    frag(buf, 1, a1, b1);
    lstore(buf ^ 1);
    mma(a0, b0);
#pragma unroll
    for (int i = 0; i < 2 + TNW; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
#pragma unroll
    for (int i = 0; i < 2 + NB; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x200, 2, 0); }
    __builtin_amdgcn_sched_group_barrier(0x008, 8 * TNW - (2 + TNW) - (2 + NB), 0);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    gload(t + 2 < nk ? t + 2 : nk - 1);
    frag(buf ^ 1, 0, a0, b0);
    mma(a1, b1);
#pragma unroll
    for (int i = 0; i < 2 + NB; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 1); __builtin_amdgcn_sched_group_barrier(0x020, 1, 1); }
#pragma unroll
    for (int i = 0; i < 2 + TNW; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 1); __builtin_amdgcn_sched_group_barrier(0x100, 1, 1); }
    __builtin_amdgcn_sched_group_barrier(0x008, 8 * TNW - (2 + NB) - (2 + TNW), 1);
    __builtin_amdgcn_sched_barrier(0);
  }
  frag((nk - 1) & 1, 1, a1, b1);                   // last k-tile: nothing left to stage
  mma(a0, b0);
  mma(a1, b1);
  __syncthreads();                                 // the reduction scratch below aliases the operand image
  float* red = &As[0][0][0][0];
#pragma unroll
  for (int j = 0; j < TNW; ++j) {
    const int cl = wn * (BN / 2) + j * 32 + l31;
    const int c = col0 + cl;
    float s1 = 0.f, s2 = 0.f;
    const float esc = g.epi_scale ? g.epi_scale[c] : 1.f, esh = g.epi_scale ? g.epi_shift[c] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = row0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (rr < g.M) {
          float v = acc[i][j][r];
          if (g.epi_scale) v = fmaf(v, esc, esh);                   // folded eval-mode BatchNorm: bn2d_apply_kernel's arithmetic
          if (add_src && !g.add_compact) {
            v += add_src[(int64_t)rr * g.N + c];
          } else if (add_src) {                                    // the stride-2 compact tensor: even (y, x) only (igemm_tile_epilogue)
            int ab, arem, ay, ax;
            fast_divmod(rr, g.OH * g.OW, g.inv_ohow, ab, arem);
            fast_divmod(arem, g.OW, g.inv_ow, ay, ax);
            if (((ay | ax) & 1) == 0) v += add_src[(int64_t)((ab * (g.OH >> 1) + (ay >> 1)) * (g.OW >> 1) + (ax >> 1)) * g.N + c];
          }
          if (g.epi_relu) v = fmaxf(v, 0.f);
          s1 += v; s2 = fmaf(v, v, s2);
          out[(int64_t)rr * g.N + c] = v;
        }
      }
    }
    if (bn_part) {
      s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
      if (kh == 0) { red[(wm * 2 + 0) * BN + cl] = s1; red[(wm * 2 + 1) * BN + cl] = s2; }
    }
  }
  if (bn_part) {
    __syncthreads();
    for (int i = tid; i < 2 * BN; i += 256) {
      const int which = i / BN, cl = i - which * BN;
      bn_part[((int64_t)tile_m * 2 + which) * g.N + col0 + cl] = red[(0 * 2 + which) * BN + cl] + red[(1 * 2 + which) * BN + cl];
    }
  }
}

// ------------------------------------------------------------------------------------ host
// Every switch of the forward / data-gradient dispatch, gathered here and nowhere else.  CREID_KNOB_ENV ones: read once in
// production, per call under CREID_DEBUG_KNOBS=1 (tests, the tuner and the probes flip them inside one process); the rest once.
static int env_int(const char* e, int dflt) { return e ? atoi(e) : dflt; }
static int env_pos(const char* name, int dflt) { const int v = env_int(getenv(name), 0); return v > 0 ? v : dflt; }
int conv_stem_dma_env() { static const int v = env_int(getenv("CREID_STEM_DMA"), 1); return v; }

static IGemmKnobs read_igemm_knobs() {
  IGemmKnobs k{};
#ifdef CREID_ABL_BUILD
  k.abl = env_int(CREID_KNOB_ENV("CREID_IGEMM_ABL"), 0);                  // per call: the probes sweep it inside one process
  { static int warned = -1; if (k.abl && k.abl != warned) { warned = k.abl; creid_ablation_env("CREID_IGEMM_ABL"); } }
  k.c64_abl = env_int(CREID_KNOB_ENV("CREID_C64_ABL"), 0);
  static const int stream2_abl = creid_ablation_env("CREID_STREAM2_ABL");
  k.stream2_abl = stream2_abl;
#endif
  k.c64_on = env_int(CREID_KNOB_ENV("CREID_C64_3X3"), 1) != 0;
  const char* pe = CREID_KNOB_ENV("CREID_IGEMM_PP");
  k.force_pp = pe ? (int)strtol(pe, nullptr, 0) : 0;
  k.pp_off = pe && k.force_pp == 0;                                     // CREID_IGEMM_PP=0: never, not even where a plan selects it
  k.pp_wgs = env_int(CREID_KNOB_ENV("CREID_PP_WGS"), 0);
  k.force_stream1 = env_int(CREID_KNOB_ENV("CREID_STREAM1X1"), 0);
  k.force_stream2 = env_int(CREID_KNOB_ENV("CREID_STREAM2"), 0);
  k.stream2_bn = env_int(CREID_KNOB_ENV("CREID_STREAM2_BN"), 0);
  k.stream_wgs = env_int(CREID_KNOB_ENV("CREID_STREAM1X1_WGS"), 0);
  k.stream1_dbg = env_int(CREID_KNOB_ENV("CREID_STREAM1X1_DBG"), 0);
  k.force_bm = env_int(CREID_KNOB_ENV("CREID_IGEMM_BM"), 0);
  k.halo_on = env_int(CREID_KNOB_ENV("CREID_IGEMM_HALO"), 1) != 0;
  static const int min_wgs = env_pos("CREID_IGEMM_BN128_MIN_WGS", 384), use_dma = env_int(getenv("CREID_IGEMM_DMA"), 1),
                   use_ws = env_int(getenv("CREID_IGEMM_WS"), 1), ws_min_k = env_pos("CREID_IGEMM_WS_MIN_K", 1024),
                   parity_on = env_int(getenv("CREID_DGRAD_PARITY"), 1), bm256_min = env_pos("CREID_IGEMM_BM256_MIN_WGS", 256);
  static const int ws_stages = [] { const int x = env_int(getenv("CREID_IGEMM_WS_STAGES"), 0); return (x == 2 || x == 4) ? x : 3; }();
  static const int stages = [] { const int v = env_int(getenv("CREID_IGEMM_STAGES"), 0); return (v >= 2 && v <= 5) ? v : 2; }();
  k.min_wgs = min_wgs; k.use_dma = use_dma; k.use_ws = use_ws; k.ws_min_k = ws_min_k; k.parity_on = parity_on;
  k.bm256_min = bm256_min; k.ws_stages = ws_stages; k.stages = stages;
  return k;
}

const IGemmKnobs& conv_igemm_knobs() {
  static const IGemmKnobs once = read_igemm_knobs();
  if (!creid_knobs_live()) return once;
  static thread_local IGemmKnobs live;
  live = read_igemm_knobs();
  return live;
}

// What igemm_bf16_halo_kernel covers: 3x3, stride 1, pad 1 (forward or transposed) over C = 64 | 128 | 256 channels per tap,
// 128-row tiles that are whole rows of one image (OW = 8 .. 64 divides 128, OH * OW a multiple of 128), and a halo image
// ((128 / OW + 2) x (OW + 2) slots) plus weight ring that fit the planes and the LDS the instantiation has.
static bool igemm_halo_covers(const IGemmGeom& g, int bn, int stages) {
  const int c = 1 << g.log2span;
  if (g.kw != 3 || g.K != 9 * c || g.stride != 1 || g.pad != 1 || !g.check_bounds || g.parity || g.pitch != c) return false;
  if (c != 64 && c != 128 && c != 256) return false;
  if (g.SH != g.OH || g.SW != g.OW) return false;
  if (g.OW != 8 && g.OW != 16 && g.OW != 32 && g.OW != 64) return false;
  if ((g.OH * g.OW) % 128 != 0 || g.M % (g.OH * g.OW) != 0) return false;
  if ((128 / g.OW + 2) * (g.OW + 2) > 32 * halo_pw(c)) return false;
  if (stages < 2 || stages > 4 || (bn != 64 && bn != 128)) return false;
  return halo_lds_bytes(c, bn, stages) < 160 * 1024;
}
static std::atomic<long long> g_halo_launches{0};

static ConvRoute conv_refuse(ConvRoute r, int err) { r.family = CONV_NONE; r.err = err; return r; }

// Which kernel runs a forward convolution or a data gradient, in precedence order.
ConvRoute route_igemm(const IGemmGeom& g, const ConvFeat& f, const IGemmKnobs& k, bool peek) {
  ConvRoute r;
  const int dtype = r.dtype = f.dtype;
  if (!creid_is_storage(dtype)) return conv_refuse(r, CREID_E_DTYPE);     // (CREID_BF16X3 forward convolutions go to launch_igemm_x3)
  const bool is16 = creid_is16(dtype);
  const int tiles_m = (g.M + 127) / 128;
  // pick the N tile: 128 unless that leaves the chip (256 CUs) under-filled or N is only 64
  int bn = 128;
  if (g.N % 128 != 0 || (int64_t)tiles_m * (g.N / 128) < k.min_wgs) bn = 64;
  // measured plan for this GEMM shape (tune.hpp): N tile and ring depth of the producer/consumer kernel; the 4th key slot is
  // transposed | stride << 1 (a stride-2 and a stride-1 3x3 layer can share M, N, K but not their gather pattern).  Folded
  // eval-mode launches look for a plan measured with THAT epilogue first: key bit 3; plans recorded before the bit existed carry
  // no mode and serve both.
  TunePlan tp;
  int tuned_stages = 0, tuned_dma = 0, tuned_stream = 0, tuned_bm256 = 0, tuned_stream2 = 0, tuned_pp = -1;
  const auto lookup = peek ? creid_tune_peek : creid_tune_lookup;
  const int plan_d = g.transposed | (g.stride << 1);
  const bool plan_eval = is16 && f.affine && lookup(CREID_TUNE_IGEMM, g.M, g.N, g.K, plan_d | 8, tp);
  r.have_plan = plan_eval || (is16 && lookup(CREID_TUNE_IGEMM, g.M, g.N, g.K, plan_d, tp));
  r.plan_key = plan_eval ? (plan_d | 8) : plan_d;
  if (r.have_plan && dtype == CREID_F16 && tp.p2 == 2) {
    // (the first persistent 1x1 kernel of conv_stream.hip is bf16 only: f16 launches of those shapes take the built-in rule)
  } else if (r.have_plan && tp.p2 == 5) {
    tuned_pp = tp.p0;                                              // plan kind 5: all-waves-multiply persistent kernel, p0 = its variant word
    r.planned = 5;
  } else if (r.have_plan && (tp.p0 == 64 || tp.p0 == 128) && g.N % tp.p0 == 0 && (tp.p1 == 2 || tp.p1 == 3 || tp.p1 == 4)) {
    bn = tp.p0; tuned_stages = tp.p1; tuned_dma = tp.p2 == 1; tuned_stream = tp.p2 == 2; tuned_bm256 = tp.p2 == 3; tuned_stream2 = tp.p2 == 4;
    r.planned = (tp.p2 >= 1 && tp.p2 <= 4) ? tp.p2 : 0;          // (any other word: the producer/consumer kernel)
  }
  const bool no_jobs = !f.bnred && !f.wred;
  // layer1's 3 x 3, 64 -> 64 forward: halo tile in LDS, weights in registers (conv_stream.hip); CREID_C64_3X3=0: the tile kernels
  if (k.c64_on && is16 && !g.transposed && g.N == 64 && g.K == 576 && g.log2span == 6 && g.kw == 3 && g.stride == 1 && g.pad == 1 &&
      g.pitch == 64 && g.check_bounds && !f.add_src && no_jobs && g.SH == g.OH && g.SW == g.OW && !(f.stats && f.affine) &&
      conv3x3_c64_route(g, f, k, r)) {
    r.kernel_id = 6;
    return r;
  }
  // all-waves-multiply persistent kernel (conv_pipe.hip): plan kind 5, or CREID_IGEMM_PP = 0x1000 | variant for every launch it covers
  if (is16 && no_jobs && g.log2span >= 6 && !k.pp_off && (k.force_pp || tuned_pp >= 0) &&
      igemm_pp_route(g, f, k.force_pp ? (k.force_pp & 0xfff) : tuned_pp, k, r)) {
    r.kernel_id = k.force_pp ? -2 : 5;
    return r;
  }
  // persistent streaming kernels for the small-K 1x1 stride-1 forward convolutions (conv_stream.hip).  First form: plan kind 2, or
  // CREID_STREAM1X1=1 for every GEMM it covers (bf16, plain epilogue).  Second form (plan kind 4 / CREID_STREAM2=1): also the folded
  // eval-mode epilogue with the block's residual; the plan's p1 = 2 -> widest column slab the LDS allows, 3 -> at most 128, 4 -> 64
  const bool fwd_1x1 = !g.transposed && g.K == (1 << g.log2span) && g.stride == 1 && g.pad == 0 && g.kw == 1 && g.check_bounds &&
                       no_jobs && g.pitch == g.K;
  if (fwd_1x1 && dtype == CREID_BF16 && !f.add_src && !f.affine && (k.force_stream1 || tuned_stream) && stream1_route(g, k, r)) {
    r.kernel_id = tuned_stream ? 2 : -2;
    return r;
  }
  if (fwd_1x1 && is16 && !f.add_compact && !f.add_mask && !(f.stats && (f.affine || f.add_src)) && (k.force_stream2 || tuned_stream2) &&
      stream2_route(g, tuned_stream2 ? (tuned_stages == 3 ? 128 : (tuned_stages == 4 ? 64 : 0)) : 0, k, r)) {
    r.kernel_id = tuned_stream2 ? 4 : -2;
    return r;
  }
  if (g.N % bn != 0) return conv_refuse(r, CREID_E_SHAPE);
  r.bn = bn; r.tiles_m = tiles_m; r.tiles_n = g.N / bn;
  r.grid = (unsigned)(tiles_m * r.tiles_n); r.block = 256;
  if (is16 && k.use_dma && (g.log2span >= 6 || conv_is_stem_geom(g))) {
    if (g.K % 64 != 0) return conv_refuse(r, CREID_E_SHAPE);
    // Producer / consumer split everywhere (single-stream step, r01: +4 % from the long-k 64-wide tiles with a
    // 3-deep ring, +2.4 % more from 2-deep rings -- two workgroups per CU -- on all other tiles; standalone sweeps in
    // profiles/r01_igemm_ws_sweep.md).  CREID_IGEMM_WS=0: the 4-wave DMA kernel; =2: force CREID_IGEMM_WS_STAGES.
    if (g.log2span >= 6 && k.use_ws >= 1 && !(tuned_dma && no_jobs)) {
      // stride-2 3x3 data gradients: parity-class row order, 9 tap-tiles per 4 output pixels instead of 36
      if (k.parity_on && g.transposed && g.stride == 2 && g.kw == 3 && g.pad == 1 && (g.K >> g.log2span) == 9 &&
          g.OH % 2 == 0 && g.OW % 2 == 0 && (g.M / 4) % 128 == 0 && !f.add_compact && f.tiles_per_image == 0)
        r.parity = 1;
      int ws_stages = k.use_ws == 2 ? k.ws_stages : ((bn == 64 && g.K >= k.ws_min_k) ? 3 : 2);
      if (tuned_stages && k.use_ws != 2) ws_stages = tuned_stages;
      r.block = 512;
      r.wred_rides = f.wred;
      const unsigned ride = f.wred ? (unsigned)f.wred_nblocks : 0u;
      // 256-row tiles (128 x 64 consumer sub-tiles, one workgroup per CU): plan kind 3, or CREID_IGEMM_BM=256 wherever the grid
      // still has >= CREID_IGEMM_BM256_MIN_WGS (default 256) workgroups; not with the fused BN reduction / parity-class rows
      const int64_t wgs256 = (int64_t)((g.M + 255) / 256) * (g.N / 128);
      if (g.N % 128 == 0 && !f.bnred && !r.parity && k.force_bm != 128 && (tuned_bm256 || (k.force_bm == 256 && wgs256 >= k.bm256_min))) {
        r.family = CONV_WS256; r.bm = 256; r.bn = 128; r.ns = (ws_stages >= 3 || g.K >= 256) ? 3 : 2;
        r.tiles_m = (g.M + 255) / 256; r.tiles_n = g.N / 128;
        r.grid = (unsigned)wgs256 + ride;
        r.kernel_id = tuned_bm256 ? 3 : -2;
        return r;
      }
      // 4 x 32 KB at BN = 128 is one workgroup per CU (the C staging reuses the ring): only on request of a measured plan
      if (ws_stages == 4 && bn == 128 && !(tuned_stages == 4 && k.use_ws != 2)) ws_stages = 3;
      r.ns = ws_stages == 4 ? 4 : (ws_stages == 2 ? 2 : 3);
      r.grid += ride;
      r.kernel_id = 0;
      // stride-1 3x3 on whole-image-row tiles: the same tile, ring depth and epilogue with the A operand resident in LDS
      // (igemm_bf16_halo_kernel; identical bits).  CREID_IGEMM_HALO=0: the plain producer/consumer kernel
      IGemmGeom gp = g;
      gp.parity = r.parity;
      const bool halo = k.halo_on && igemm_halo_covers(gp, bn, ws_stages);
      r.family = halo ? CONV_HALO : CONV_WS;
      r.chan = halo ? (1 << g.log2span) : 0;
      return r;
    }
    // 4-wave DMA kernel; LDS ring depth CREID_IGEMM_STAGES = 2..5, default 2 -- measured r01: deeper rings LOSE, the k-loop is
    // bound by the LDS->MFMA chain and by workgroups/CU, not by DMA latency; 3+ stages cost occupancy (5 x 32 KB would not fit)
    const int stages = (tuned_dma && tuned_stages) ? tuned_stages : k.stages;
    r.family = CONV_DMA4; r.wred_first = f.wred;
    r.ns = (stages < 2 || stages > 5) ? 2 : ((bn == 128 && stages == 5) ? 4 : stages);
    r.kernel_id = 1;
    return r;
  }
  // the fused reduction / masked add / folded BatchNorm (and f16) exist only in the 16-bit LDS-DMA kernels
  if (f.bnred || f.add_mask || (f.affine && is16) || dtype == CREID_F16) return conv_refuse(r, CREID_E_DTYPE);
  if (g.K % (dtype == CREID_BF16 ? 64 : 16) != 0) return conv_refuse(r, CREID_E_SHAPE);
  r.family = dtype == CREID_BF16 ? CONV_REG_BF16 : CONV_F32;
  r.wred_first = f.wred;
  return r;
}

// The switch from a route to its template instantiation: decides nothing.
static void launch_igemm_tiles(const ConvRoute& r, const IGemmGeom& g, const ConvPtrs& p, const BnRedArgs& bnred, const WRedJob& wred,
                               hipStream_t s) {
  const dim3 grid(r.grid), block(r.block);
  const unsigned short *src = (const unsigned short*)p.src, *wgt = (const unsigned short*)p.wgt, *add_src = (const unsigned short*)p.add_src;
  unsigned short* out = (unsigned short*)p.out;
  const bool f16 = r.dtype == CREID_F16;
#define CREID_ET_LAUNCH(K_, ...) do { if (f16) hipLaunchKernelGGL((K_<__VA_ARGS__, F16T>), grid, block, 0, s, g, src, wgt, out, add_src, p.bn_part, r.tiles_n, bnred, wred); \
                                      else hipLaunchKernelGGL((K_<__VA_ARGS__, Bf16T>), grid, block, 0, s, g, src, wgt, out, add_src, p.bn_part, r.tiles_n, bnred, wred); } while (0)
#define CREID_DMA_LAUNCH(BN_, NS_) do { if (f16) hipLaunchKernelGGL((igemm_bf16_dma_kernel<BN_, NS_, F16T>), grid, block, 0, s, g, src, wgt, out, add_src, p.bn_part, r.tiles_n, bnred); \
                                        else hipLaunchKernelGGL((igemm_bf16_dma_kernel<BN_, NS_, Bf16T>), grid, block, 0, s, g, src, wgt, out, add_src, p.bn_part, r.tiles_n, bnred); } while (0)
  // (a 4-deep ring that does not fit beside the halo image is refused by igemm_halo_covers: that name is never launched)
#define CREID_HALO_STAGES(C_, BN_) do { constexpr int NS4 = halo_lds_bytes(C_, BN_, 4) < 160 * 1024 ? 4 : 3;                        \
                                        if (r.ns == 4) CREID_ET_LAUNCH(igemm_bf16_halo_kernel, C_, BN_, NS4);                       \
                                        else if (r.ns == 2) CREID_ET_LAUNCH(igemm_bf16_halo_kernel, C_, BN_, 2);                    \
                                        else CREID_ET_LAUNCH(igemm_bf16_halo_kernel, C_, BN_, 3); } while (0)
#define CREID_HALO_BN(C_) do { if (r.bn == 128) CREID_HALO_STAGES(C_, 128); else CREID_HALO_STAGES(C_, 64); } while (0)
#define CREID_NS_LAUNCH(L_, BN_) do { switch (r.ns) { case 2: L_(BN_, 2); break; case 3: L_(BN_, 3); break; case 4: L_(BN_, 4); break; default: L_(BN_, 5); break; } } while (0)
#define CREID_WS_LAUNCH(BN_, NS_) CREID_ET_LAUNCH(igemm_bf16_ws_kernel, BN_, NS_, 128)
  switch (r.family) {
    case CONV_WS256:
      if (r.ns == 3) CREID_ET_LAUNCH(igemm_bf16_ws_kernel, 128, 3, 256); else CREID_ET_LAUNCH(igemm_bf16_ws_kernel, 128, 2, 256);
      break;
    case CONV_HALO:
      if (r.chan == 64) CREID_HALO_BN(64); else if (r.chan == 128) CREID_HALO_BN(128); else CREID_HALO_BN(256);
      break;
    case CONV_WS:
      if (r.bn == 128) { if (r.ns == 4) CREID_WS_LAUNCH(128, 4); else if (r.ns == 2) CREID_WS_LAUNCH(128, 2); else CREID_WS_LAUNCH(128, 3); }
      else { if (r.ns == 4) CREID_WS_LAUNCH(64, 4); else if (r.ns == 2) CREID_WS_LAUNCH(64, 2); else CREID_WS_LAUNCH(64, 3); }
      break;
    case CONV_DMA4:
      if (r.bn == 128) { if (r.ns == 4) CREID_DMA_LAUNCH(128, 4); else if (r.ns == 3) CREID_DMA_LAUNCH(128, 3); else CREID_DMA_LAUNCH(128, 2); }
      else CREID_NS_LAUNCH(CREID_DMA_LAUNCH, 64);
      break;
    case CONV_REG_BF16:
      if (r.bn == 128) hipLaunchKernelGGL(igemm_bf16_kernel<128>, grid, block, 0, s, g, src, wgt, out, add_src, p.bn_part, r.tiles_n);
      else hipLaunchKernelGGL(igemm_bf16_kernel<64>, grid, block, 0, s, g, src, wgt, out, add_src, p.bn_part, r.tiles_n);
      break;
    default:
      if (r.bn == 128) hipLaunchKernelGGL(igemm_f32_kernel<128>, grid, block, 0, s, g, (const float*)p.src, (const float*)p.wgt, (float*)p.out,
                                          (const float*)p.add_src, p.bn_part, r.tiles_n);
      else hipLaunchKernelGGL(igemm_f32_kernel<64>, grid, block, 0, s, g, (const float*)p.src, (const float*)p.wgt, (float*)p.out,
                              (const float*)p.add_src, p.bn_part, r.tiles_n);
      break;
  }
#undef CREID_WS_LAUNCH
#undef CREID_NS_LAUNCH
#undef CREID_HALO_BN
#undef CREID_HALO_STAGES
#undef CREID_DMA_LAUNCH
#undef CREID_ET_LAUNCH
}

static void launch_route(const ConvRoute& r, const IGemmGeom& g, const ConvPtrs& p, const BnRedArgs& bnred, const WRedJob& wred,
                         hipStream_t s) {
  switch (r.family) {
    case CONV_C64: return launch_conv3x3_c64(r, g, p, s);
    case CONV_PP: return launch_igemm_pp(r, g, p, s);
    case CONV_STREAM1: return launch_stream1(r, g, p, s);
    case CONV_STREAM2: return launch_stream2(r, g, p, s);
    default: return launch_igemm_tiles(r, g, p, bnred, wred, s);
  }
}

static ConvFeat conv_feat_of(const IGemmGeom& g, const void* add_src, const float* bn_part, const BnRedArgs& bnred, const WRedJob* wred,
                             int dtype) {
  ConvFeat f;
  f.dtype = dtype; f.add_src = add_src != nullptr; f.add_compact = g.add_compact != 0; f.add_mask = g.add_mask != nullptr;
  f.stats = bn_part != nullptr; f.affine = g.epi_scale != nullptr; f.bnred = bnred.x != nullptr; f.tiles_per_image = bnred.tiles_per_image;
  f.wred = wred && wred->ws; f.wred_nblocks = f.wred ? wred->nblocks : 0;
  return f;
}

static int launch_igemm(const IGemmGeom& g_in, const void* src, const void* wgt, void* out, const void* add_src,
                        float* bn_part, int dtype, hipStream_t s, BnRedArgs bnred = BnRedArgs{},
                        const WRedJob* wred_in = nullptr) {
  static_assert(sizeof(float) * (4 * 512 + 8192) <= 2 * (128 + 64) * 64 * 2, "reduce scratch must fit the smallest LDS ring");
  const IGemmKnobs& k = conv_igemm_knobs();
  const ConvRoute r = route_igemm(g_in, conv_feat_of(g_in, add_src, bn_part, bnred, wred_in, dtype), k);
  if (r.err) return r.err;
  IGemmGeom g = g_in;
  g.abl = k.abl;
  g.parity = r.parity;
  WRedJob wred{};
  if (wred_in) wred = *wred_in;
  if (r.wred_first) {                                  // kernels without the carrier: the reduce job as its own launch first
    if (const int rc = wgrad_reduce_job_launch(wred, s)) return rc;
    wred.ws = nullptr;
  }
  // a launch that found a plan and takes another kernel (creid_tune_count, what = 1)
  if (r.have_plan && r.kernel_id != r.planned) creid_tune_declined(CREID_TUNE_IGEMM, g.M, g.N, g.K, r.plan_key);
  if (r.family == CONV_HALO) g_halo_launches.fetch_add(1, std::memory_order_relaxed);
  launch_route(r, g, ConvPtrs{src, wgt, out, add_src, bn_part}, bnred, wred, s);
  return (int)hipGetLastError();
}

static int check_desc(const creid_conv_desc* d) {
  if (!d || d->batch <= 0 || d->in_h <= 0 || d->in_w <= 0 || d->in_c <= 0 || d->out_c <= 0) return CREID_E_ARG;
  if (d->kh != d->kw || (d->kh != 1 && d->kh != 3) || d->stride < 1 || d->stride > 2) return CREID_E_SHAPE;
  if (igemm_ilog2(d->in_c) < 0 || igemm_ilog2(d->out_c) < 0 || d->in_c < 64 || d->out_c < 64) return CREID_E_SHAPE;
  if (d->out_h != (d->in_h + 2 * d->pad - d->kh) / d->stride + 1) return CREID_E_SHAPE;
  if (d->out_w != (d->in_w + 2 * d->pad - d->kw) / d->stride + 1) return CREID_E_SHAPE;
  if (d->batch * d->in_h * d->in_w >= (1LL << 24) || d->batch * d->out_h * d->out_w >= (1LL << 24) || d->batch * d->in_h * d->in_w * d->in_c > (1LL << 40)) return CREID_E_SHAPE;
  return 0;
}

int conv_check_desc(const creid_conv_desc* d) { return check_desc(d); }

// What a fused data-gradient call may combine (creid_conv2d_dgrad_fused_nhwc and creid_conv_route_describe): the compact add needs
// even extents, the fused BatchNorm reduction and the masked add exist only in the 16-bit LDS-DMA kernels.
int conv_dgrad_check(const creid_conv_desc* d, const ConvFeat& f, int64_t bn_stat_image_rows, int add_src_stride) {
  if (bn_stat_image_rows % 128 != 0) return CREID_E_SHAPE;
  if (add_src_stride != 1 && add_src_stride != 2) return CREID_E_ARG;
  if (add_src_stride == 2 && (!f.add_src || d->in_h % 2 || d->in_w % 2)) return CREID_E_SHAPE;
  const bool dma16 = creid_is16(f.dtype) && conv_igemm_knobs().use_dma;
  if (f.bnred && !dma16) return CREID_E_DTYPE;
  if (f.add_mask && (!f.add_src || add_src_stride != 1 || !dma16)) return CREID_E_ARG;
  return 0;
}

extern "C" {

int64_t creid_igemm_halo_launches(void) { return (int64_t)g_halo_launches.load(std::memory_order_relaxed); }

int64_t creid_conv2d_bn_partial_rows(const creid_conv_desc* d) {
  if (!d) return 0;
  return (d->batch * d->out_h * d->out_w + 127) / 128;   /* (sum, sumsq) row PAIRS */
}

int creid_conv2d_fwd_nhwc(const creid_conv_desc* d, const void* x, const void* w_krsc, void* y, float* bn_partial,
                          int dtype, void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  CREID_CHECK_ARG(x && w_krsc && y);
  IGemmGeom g = fwd_geom(d);
  if (dtype == CREID_BF16X3) return launch_igemm_x3(g, x, w_krsc, y, nullptr, bn_partial, as_stream(stream));
  return launch_igemm(g, x, w_krsc, y, nullptr, bn_partial, dtype, as_stream(stream));
}

/* Forward convolution with an eval-mode BatchNorm folded into the epilogue: y = act(conv(x) * scale + shift (+ residual)),
 * scale_shift = [2][out_c] fp32 (creid_bn2d_fold_multi), act = ReLU when relu != 0.  No statistics, no second pass. */
int creid_conv2d_fwd_affine_nhwc(const creid_conv_desc* d, const void* x, const void* w_krsc, void* y, const float* scale_shift,
                                 const void* residual, int relu, int dtype, void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  CREID_CHECK_ARG(x && w_krsc && y && scale_shift);
  IGemmGeom g = fwd_geom(d);
  g.epi_scale = scale_shift; g.epi_shift = scale_shift + d->out_c; g.epi_relu = relu ? 1 : 0;
  if (dtype == CREID_BF16X3) return launch_igemm_x3(g, x, w_krsc, y, residual, nullptr, as_stream(stream));
  return launch_igemm(g, x, w_krsc, y, residual, nullptr, dtype, as_stream(stream));
}

int creid_conv2d_dgrad_nhwc(const creid_conv_desc* d, const void* dy, const void* w_crsk, void* dx, const void* add_src,
                            int dtype, void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  CREID_CHECK_ARG(dy && w_crsk && dx);
  IGemmGeom g = dgrad_geom(d);
  return launch_igemm(g, dy, w_crsk, dx, add_src, nullptr, dtype, as_stream(stream));
}

/* bf16x3 data gradient (conv_x3.hip): fp32 dy / dx / add_src, w2_crsk = the two-plane transposed copy. */
int creid_conv2d_dgrad_x3_nhwc(const creid_conv_desc* d, const void* dy, const void* w2_crsk, void* dx, const void* add_src,
                               void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  CREID_CHECK_ARG(dy && w2_crsk && dx);
  IGemmGeom g = dgrad_geom(d);
  return launch_igemm_x3(g, dy, w2_crsk, dx, add_src, nullptr, as_stream(stream));
}

/* dgrad with the NEXT BatchNorm-backward's column reduction fused into the epilogue (bf16 only). */
int creid_conv2d_dgrad_bnred_nhwc(const creid_conv_desc* d, const void* dy, const void* w_crsk, void* dx,
                                  const void* add_src, const void* bn_x, const void* bn_act, const float* bn_mean,
                                  const float* bn_invstd, float* bn_partial, int64_t bn_stat_image_rows,
                                  int add_src_stride, int dtype, void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  CREID_CHECK_ARG(dy && w_crsk && dx && bn_x && bn_mean && bn_invstd && bn_partial && bn_stat_image_rows >= 0);   // (here bn_x is required)
  return creid_conv2d_dgrad_fused_nhwc(d, dy, w_crsk, dx, add_src, add_src_stride, nullptr, bn_x, bn_act, nullptr, bn_mean, bn_invstd,
                                       bn_partial, bn_stat_image_rows, nullptr, nullptr, 0, nullptr, 0, dtype, stream);
}

/* Data gradient with everything that can ride in the same launch: "+ add_src" (full or stride-2 compact), the NEXT
 * BatchNorm-backward's column reduction (bn_x != NULL; bf16), and the split reduction of the PREVIOUS weight-gradient
 * (bn_mask != NULL: the ReLU mask comes as bits from creid_bn2d_apply_mask, one byte per 8 channels, and bn_act is not read)
 * launch (wred_desc != NULL: creid_conv2d_wgrad_partials of that convolution wrote wred_ws; the first workgroups of
 * this launch sum the partials into wred_dw).  Where the fused kernel does not apply (fp32 parity mode, stem) the
 * reduction runs as its own launch first -- same result. */
int creid_conv2d_dgrad_fused_nhwc(const creid_conv_desc* d, const void* dy, const void* w_crsk, void* dx,
                                  const void* add_src, int add_src_stride, const uint8_t* add_mask, const void* bn_x,
                                  const void* bn_act, const uint8_t* bn_mask, const float* bn_mean, const float* bn_invstd, float* bn_partial,
                                  int64_t bn_stat_image_rows, const creid_conv_desc* wred_desc, float* wred_dw,
                                  int wred_accumulate, const void* wred_ws, size_t wred_ws_bytes, int dtype, void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!creid_is_storage(dtype)) return CREID_E_DTYPE;     // (before the piggy-backed weight-gradient reduction is planned)
  CREID_CHECK_ARG(dy && w_crsk && dx && bn_stat_image_rows >= 0);
  if (bn_x) CREID_CHECK_ARG(bn_mean && bn_invstd && bn_partial);
  ConvFeat f;
  f.dtype = dtype; f.add_src = add_src != nullptr; f.add_mask = add_mask != nullptr; f.bnred = bn_x != nullptr;
  if (const int rc = conv_dgrad_check(d, f, bn_stat_image_rows, add_src_stride)) return rc;
  WRedJob job{};
  bool have_job = false;
  if (wred_desc) {
    CREID_CHECK_ARG(wred_dw && wred_ws);
    if (!wgrad_make_reduce_job(wred_desc, dtype, wred_ws, wred_ws_bytes, wred_dw, wred_accumulate, job)) return CREID_E_SHAPE;
    have_job = true;
  }
  IGemmGeom g = dgrad_geom(d);
  g.add_compact = add_src_stride == 2;
  g.add_mask = add_mask;
  BnRedArgs br{};
  if (bn_x) br = BnRedArgs{bn_x, bn_mask ? nullptr : bn_act, bn_mean, bn_invstd, bn_partial, (int)(bn_stat_image_rows / 128), bn_mask};
  return launch_igemm(g, dy, w_crsk, dx, add_src, nullptr, dtype, as_stream(stream), br, have_job ? &job : nullptr);
}

/* stem: 7x7 stride-2 pad-3 conv, 3 -> 64 channels, on the pre-padded NHWC4 image
 * xpad [B, H+8, W+6, 4] (image at rows 3..H+2, cols 3..W+2, zeros elsewhere); w_stem [64][8][32]
 * (k = r*32 + s*4 + c, zero for s = 7, c = 3 and r = 7); y [B, H/2, W/2, 64]. */
int creid_stem_conv_fwd(int64_t batch, int64_t H, int64_t W, const void* xpad, const void* w_stem, void* y,
                        float* bn_partial, int dtype, void* stream) {
  CREID_CHECK_ARG(xpad && w_stem && y);
  if (const int rc = stem_check_shape(batch, H, W)) return rc;
  IGemmGeom g = stem_geom(batch, H, W);
  return launch_igemm(g, xpad, w_stem, y, nullptr, bn_partial, dtype, as_stream(stream));
}

/* the stem with its eval-mode BatchNorm (and, for the IBN-a variant, ReLU) folded into the epilogue */
int creid_stem_conv_fwd_affine(int64_t batch, int64_t H, int64_t W, const void* xpad, const void* w_stem, void* y,
                               const float* scale_shift, int relu, int dtype, void* stream) {
  CREID_CHECK_ARG(xpad && w_stem && y && scale_shift);
  if (const int rc = stem_check_shape(batch, H, W)) return rc;
  IGemmGeom g = stem_geom(batch, H, W);
  g.epi_scale = scale_shift; g.epi_shift = scale_shift + 64; g.epi_relu = relu ? 1 : 0;
  return launch_igemm(g, xpad, w_stem, y, nullptr, nullptr, dtype, as_stream(stream));
}

}  // extern "C"
