// bf16x3 forward convolution (CREID_BF16X3): fp32-grade results from the bf16 matrix pipe.
//
// Every operand x is carried as a pair hi = bf16(x), lo = bf16(x - hi) (|x - hi - lo| <= 2^-16 |x|), and each product is
// expanded into the three bf16 MFMAs  lo_a * hi_w + hi_a * lo_w + hi_a * hi_w  with fp32 accumulation (the lo * lo term,
// <= 2^-18 relative, is dropped).  A 32 x 32 x 16 fragment then costs 3 x 32 cycles of the matrix pipe against 16 x that for
// exact-f32 MFMA (v_mfma_f32_32x32x2f32 runs at 1/16 of the bf16 rate on gfx950, and the chip has no xf32).
//
//   activations  fp32 NHWC in and out (every other kernel of the eval-mode forward keeps its CREID_F32 path);
//   weights      split once at weight-prep time: [2][O][r][s][I] bf16, the hi plane then the lo plane (creid_weight_prep
//                with dtype CREID_BF16X3); the data gradient reads the transposed copy [2][I][r][s][O]
//                (creid_weight_prep_x3_train_multi);
//   dgrad        the same kernel with the transposed geometry (igemm_src_pixel): source dY, output dX, every tap visited in
//                the fixed order (absent taps of a stride-2 layer stage zeros), epilogue "+ add_src";
//   activation   split when the k-tile lands in LDS: one cooperative pass per tile, so a row that feeds both wave columns of
//                the tile is split once; the LDS image holds the hi and lo planes (the same bytes as the fp32 tile);
//   k order      the whole reduction of an output element runs in one workgroup, k-step by k-step, and inside a step always
//                lo*hi, hi*lo, hi*hi -- fixed by the convolution's shape alone, so a row's result does not depend on the batch
//                size, the grid or the N tile (run_inference's macro-batching relies on that);
//   epilogue     the fp32 kernel's: y = act(acc * scale + shift (+ residual)), optional per-128-row (sum, sumsq) partials.
//
// Tile: 128 rows x BN (64 | 128) columns x 32-deep k-tiles, 256 threads = 2 x 2 waves of 64 x BN/2, two LDS buffers
// (BN = 128: 64 KB, two workgroups per CU).  Launch rule (no tuner keys): BN = 128 where N % 128 == 0 and that still gives
// >= 512 workgroups (two per CU on 256 CUs), else BN = 64.
#include "conv_common.hpp"

namespace {

constexpr int X3_BK = 32, X3_KQ = X3_BK / 8;     // k-tile depth, 8-element (16-byte bf16) chunks per row of a k-tile

__device__ __forceinline__ f32x16 x3_mfma(const uint4& a, const uint4& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// (f0, f1) -> packed hi pair and packed lo pair
__device__ __forceinline__ void x3_split2(float f0, float f1, unsigned int& hi, unsigned int& lo) {
  const unsigned h = f32x2_to_bf16x2_bits(f0, f1);
  hi = h;
  lo = f32x2_to_bf16x2_bits(f0 - __uint_as_float(h << 16), f1 - __uint_as_float(h & 0xffff0000u));
}

template <int BN>
__global__ __launch_bounds__(256, 2) void igemm_x3_kernel(IGemmGeom g, const float* __restrict__ src,
                                                          const unsigned short* __restrict__ wgt, float* __restrict__ out,
                                                          const float* __restrict__ add_src, float* __restrict__ bn_part,
                                                          int tiles_n) {
  constexpr int TNW = BN / 64;                   // 32-column MFMA tiles per wave
  constexpr int NBU = BN * X3_KQ / 256;          // 16-byte weight chunks per thread and plane per k-tile
  // [buffer][plane: 0 hi, 1 lo][k chunk][row] -- a wave's fragment read is 32 consecutive rows of two chunks (no conflicts)
  constexpr int A_UNITS = 2 * 2 * X3_KQ * 128;
  __shared__ uint4 smem[A_UNITS + 2 * 2 * X3_KQ * BN];
  auto As = [&](int buf, int p, int kq, int row) -> uint4& { return smem[((buf * 2 + p) * X3_KQ + kq) * 128 + row]; };
  auto Bs = [&](int buf, int p, int kq, int row) -> uint4& { return smem[A_UNITS + ((buf * 2 + p) * X3_KQ + kq) * BN + row]; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
  const int row0 = tile_m * 128, col0 = tile_n * BN;
  const int span_mask = (1 << g.log2span) - 1;
  const int64_t plane = (int64_t)g.N * g.K;

  // A staging: thread -> one row (pixel) of the tile, chunks kq0 and kq0 + 2 of every k-tile
  const int arow = tid & 127, kq0 = tid >> 7;
  const int m = row0 + arow;
  const bool vm = m < g.M;
  int oy, ox, bpix;
  {
    const int mm = vm ? m : 0;
    const int b = mm / (g.OH * g.OW), rem = mm - b * (g.OH * g.OW);
    oy = rem / g.OW; ox = rem - oy * g.OW;
    bpix = b * g.SH * g.SW;
  }
  // B staging: chunk i of a thread (i < NBU) -> row tid % BN, k chunk tid / BN + (256 / BN) i, both planes
  static_assert(NBU == 1 || NBU == 2, "one or two weight chunks per thread");
  const int brow = tid % BN, bkq = tid / BN;
  const unsigned short* wp = wgt + (int64_t)(col0 + brow) * g.K + 8 * bkq;
  // the k-tile in flight in registers (separate members, not arrays: an indexed array of these is moved to LDS by the compiler)
  struct Stage {
    float4 a0, a1, a2, a3;                       // chunk kq0: k 0..3, 4..7; chunk kq0 + 2: k 0..3, 4..7
    uint4 bh0, bl0, bh1, bl1;                    // weight chunks (hi, lo) i = 0, 1
    unsigned amask;                              // all ones where the staged tap is a real pixel
  };
  auto gload = [&](Stage& st, int t) {           // a k-tile never straddles two taps (in_c is a power of two >= 64)
    const int kk = t * X3_BK;
    const int tap = kk >> g.log2span, c = kk & span_mask;
    const int r = tap / g.kw, s = tap - r * g.kw;
    int iy, ix;
    const bool ok = vm && igemm_src_pixel(g, oy, ox, r, s, iy, ix);
    st.amask = ok ? 0xffffffffu : 0u;            // an absent tap reads the tensor's first elements and stages zeros
    const float* ap = src + (ok ? (int64_t)(bpix + iy * g.SW + ix) * g.pitch + c : 0);
    st.a0 = *reinterpret_cast<const float4*>(ap + 8 * kq0);
    st.a1 = *reinterpret_cast<const float4*>(ap + 8 * kq0 + 4);
    st.a2 = *reinterpret_cast<const float4*>(ap + 8 * kq0 + 16);
    st.a3 = *reinterpret_cast<const float4*>(ap + 8 * kq0 + 20);
    st.bh0 = *reinterpret_cast<const uint4*>(wp + kk);
    st.bl0 = *reinterpret_cast<const uint4*>(wp + plane + kk);
    if constexpr (NBU == 2) {
      st.bh1 = *reinterpret_cast<const uint4*>(wp + kk + 8 * (256 / BN));
      st.bl1 = *reinterpret_cast<const uint4*>(wp + plane + kk + 8 * (256 / BN));
    }
  };
  auto lstore = [&](const Stage& st, int buf) {
    auto mk = [&](float v) { return __uint_as_float(__float_as_uint(v) & st.amask); };
    auto split8 = [&](const float4& v0, const float4& v1, int kq) {
      uint4 hw, lw;
      x3_split2(mk(v0.x), mk(v0.y), hw.x, lw.x);
      x3_split2(mk(v0.z), mk(v0.w), hw.y, lw.y);
      x3_split2(mk(v1.x), mk(v1.y), hw.z, lw.z);
      x3_split2(mk(v1.z), mk(v1.w), hw.w, lw.w);
      As(buf, 0, kq, arow) = hw;
      As(buf, 1, kq, arow) = lw;
    };
    split8(st.a0, st.a1, kq0);
    split8(st.a2, st.a3, kq0 + 2);
    Bs(buf, 0, bkq, brow) = st.bh0;
    Bs(buf, 1, bkq, brow) = st.bl0;
    if constexpr (NBU == 2) {
      Bs(buf, 0, bkq + 256 / BN, brow) = st.bh1;
      Bs(buf, 1, bkq + 256 / BN, brow) = st.bl1;
    }
  };

  f32x16 acc[2][TNW];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TNW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int l31 = lane & 31, kh = lane >> 5;
  const int fa = wm * 64 + l31, fb = wn * (BN / 2) + l31;
  auto mma = [&](int buf) {
#pragma unroll
    for (int ks = 0; ks < X3_BK / 16; ++ks) {
      const int kq = 2 * ks + kh;                // lanes 0..31: k 0..7 of the step, lanes 32..63: k 8..15
      uint4 ah[2], al[2], bh[TNW], bl[TNW];
#pragma unroll
      for (int i = 0; i < 2; ++i) { ah[i] = As(buf, 0, kq, fa + 32 * i); al[i] = As(buf, 1, kq, fa + 32 * i); }
#pragma unroll
      for (int j = 0; j < TNW; ++j) { bh[j] = Bs(buf, 0, kq, fb + 32 * j); bl[j] = Bs(buf, 1, kq, fb + 32 * j); }
      // small terms first; the three passes are interleaved over the wave's fragments so no MFMA waits on the previous one
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TNW; ++j) acc[i][j] = x3_mfma(al[i], bh[j], acc[i][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TNW; ++j) acc[i][j] = x3_mfma(ah[i], bl[j], acc[i][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TNW; ++j) acc[i][j] = x3_mfma(ah[i], bh[j], acc[i][j]);
    }
  };

  // k loop: LDS double buffer, the next k-tile's global loads in flight while this one multiplies.  (A second register stage --
  // loads issued two multiply phases ahead -- measured slower: 8.80 vs 8.63 ms for the ResNet50 forward at batch 128, at 242
  // instead of 147 VGPRs; the loop is not bound by load latency.)
  const int nk = g.K / X3_BK;
  Stage st;
  gload(st, 0);
  lstore(st, 0);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    if (t + 1 < nk) gload(st, t + 1);
    mma(buf);
    if (t + 1 < nk) lstore(st, buf ^ 1);         // buffer buf ^ 1 was last read in step t - 1, before the barrier below
    __syncthreads();
  }

  // epilogue: the arithmetic of igemm_f32_kernel's (conv_igemm.hip)
  float* red = reinterpret_cast<float*>(smem);
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
          if (g.epi_scale) v = fmaf(v, esc, esh);
          if (add_src) v += add_src[(int64_t)rr * g.N + c];
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

}  // namespace

int launch_igemm_x3(const IGemmGeom& g, const void* src, const void* wgt, void* out, const void* add_src, float* bn_part,
                    hipStream_t s) {
  // NHWC source whose channels (in_c forward, out_c data gradient) are a power of two >= 64 (check_desc): every k-tile lies
  // inside one tap
  if (!g.check_bounds || g.add_compact || g.add_mask || g.parity || g.log2span < 5 || g.K % X3_BK != 0 || g.N % 64 != 0) return CREID_E_SHAPE;
  const int tiles_m = (g.M + 127) / 128;
  const int bn = (g.N % 128 == 0 && (int64_t)tiles_m * (g.N / 128) >= 512) ? 128 : 64;
  const int tiles_n = g.N / bn;
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(256);
  if (bn == 128)
    hipLaunchKernelGGL(igemm_x3_kernel<128>, grid, block, 0, s, g, (const float*)src, (const unsigned short*)wgt, (float*)out,
                       (const float*)add_src, bn_part, tiles_n);
  else
    hipLaunchKernelGGL(igemm_x3_kernel<64>, grid, block, 0, s, g, (const float*)src, (const unsigned short*)wgt, (float*)out,
                       (const float*)add_src, bn_part, tiles_n);
  return (int)hipGetLastError();
}
