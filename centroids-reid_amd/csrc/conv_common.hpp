// Geometry shared by the implicit-GEMM convolution kernels (stage A).
//
// Every convolution of the backbone (modelling/backbones/resnet.py:56-61,94,109) is lowered to
// an im2col-FREE GEMM  C[M, N] = sum_k A[m, k] * W[n, k]  over NHWC activations:
//   m = (b, oy, ox) output pixel, n = output channel, k = (tap, c) with tap = (r, s);
// the A row for a tap is a CONTIGUOUS run of `span` channels of one source pixel, so the A tile
// is gathered straight from the activation tensor with 16-byte loads (zero-filled outside the
// image) -- no column buffer is ever materialised.  The same kernel computes the data gradient
// (`transposed` = 1: source = dY, weights pre-transposed to [Cin][r][s][Cout]) and the stem
// (7x7 s2 on a pre-padded NHWC4 image: span = 32 = 8 pixels x 4 channels per kernel row).
#pragma once
#include "common.hpp"

struct IGemmGeom {
  int M;              // rows of the GEMM = batch * OH * OW
  int OH, OW;         // spatial dims that index the rows
  int SH, SW;         // source spatial dims (tensor the A operand is gathered from)
  int pitch;          // elements per source pixel (channels; 4 for the padded stem image)
  int log2span;       // log2(elements of K per tap)
  int kw;             // taps per kernel row: tap -> (r = tap / kw, s = tap % kw)
  int stride, pad;
  int transposed;     // 0: iy = oy*stride + r - pad ; 1: ty = oy + pad - r, iy = ty/stride if divisible
  int K;              // reduction length = taps << log2span
  int N;              // output channels
  int check_bounds;   // 0: source is pre-padded (stem)
  float inv_ohow, inv_ow;   // 1/(OH*OW), 1/OW for fast_divmod (M < 2^24)
  int add_compact;          // epilogue add_src is a stride-2 COMPACT tensor [B, OH/2, OW/2, N]: added at even (y, x) only
  int parity;               // transposed stride-2 (data gradient): GEMM rows are enumerated parity-class major --
                            // row m = class*(M/4) + (b, y/2, x/2), class = (y&1)*2 + (x&1) -- so a 128-row tile holds
                            // one class and only that class's taps (1, 2, 2 or 4 of 9 for 3x3) are visited
  const unsigned char* add_mask;   // nullable (full-resolution add_src only): bit mask applied to add_src before the add,
                                   // one byte per 8 channels -- the residual-branch gradient is then the UNMASKED incoming
                                   // gradient plus the ReLU bits, and no masked copy has to be written and re-read
  const float* epi_scale;   // nullable: per-output-channel affine y = acc * scale + shift applied to the fp32 accumulators --
  const float* epi_shift;   // eval-mode BatchNorm (running statistics are constants) folded into the convolution
  int epi_relu;             // ReLU after the affine and after "+ add_src" (the block's residual) when that is given
  int abl;                  // timing-only ablation bits (CREID_IGEMM_ABL, producer/consumer kernel): 1 no MFMA, 2 no DMA after the
                            // first k-tile, 4 no fragment reads, 8 no copy-out stores -- results are WRONG when set.  Only the
                            // ablation build (build.py --ablation -> libcreid_hip_abl.so) looks at them
};

// The switches cost 0.07 ms per step when compiled into the k-loops (same-box A/B), so the shipped library folds them away.
#ifdef CREID_ABL_BUILD
#define CREID_ABL_ON(word, bits) ((word) & (bits))
#else
#define CREID_ABL_ON(word, bits) 0
#endif

// bf16x3 convolution (conv_x3.hip): fp32 source / output, two-plane bf16 weights [2][N][K]; forward or data gradient
// (g.transposed), epilogue "+ add_src" at full resolution; returns CREID_E_SHAPE for a geometry it does not cover (the
// pre-padded stem image, compact or masked add_src, parity-ordered rows)
int launch_igemm_x3(const IGemmGeom& g, const void* src, const void* wgt, void* out, const void* add_src, float* bn_part,
                    hipStream_t s);

// the descriptor checks of every convolution entry point (conv_igemm.hip): CREID_E_ARG for a null or non-positive descriptor,
// CREID_E_SHAPE for a geometry outside the kernels' cover, 0 otherwise
int conv_check_desc(const creid_conv_desc* d);

static inline int igemm_ilog2(int64_t v) {      // log2 of a power of two, -1 otherwise
  int l = 0;
  while ((1LL << l) < v) ++l;
  return ((1LL << l) == v) ? l : -1;
}

static inline void igemm_finish_geom(IGemmGeom& g) {
  g.inv_ohow = 1.0f / (float)(g.OH * g.OW);
  g.inv_ow = 1.0f / (float)g.OW;
  g.add_compact = 0;
  g.parity = 0;
  g.add_mask = nullptr;
  g.epi_scale = nullptr;
  g.epi_shift = nullptr;
  g.epi_relu = 0;
  g.abl = 0;
}

// Forward convolution of descriptor d: GEMM rows = output pixels, A gathered from the input, K = taps x in_c.
static inline IGemmGeom fwd_geom(const creid_conv_desc* d) {
  IGemmGeom g;
  g.M = (int)(d->batch * d->out_h * d->out_w); g.OH = (int)d->out_h; g.OW = (int)d->out_w;
  g.SH = (int)d->in_h; g.SW = (int)d->in_w; g.pitch = (int)d->in_c; g.log2span = igemm_ilog2(d->in_c);
  g.kw = d->kw; g.stride = d->stride; g.pad = d->pad; g.transposed = 0;
  g.K = (int)(d->kh * d->kw * d->in_c); g.N = (int)d->out_c; g.check_bounds = 1;
  igemm_finish_geom(g);
  return g;
}
// Its data gradient: GEMM rows = input pixels, A gathered from dY (transposed gather), K = taps x out_c.
static inline IGemmGeom dgrad_geom(const creid_conv_desc* d) {
  IGemmGeom g;
  g.M = (int)(d->batch * d->in_h * d->in_w); g.OH = (int)d->in_h; g.OW = (int)d->in_w;
  g.SH = (int)d->out_h; g.SW = (int)d->out_w; g.pitch = (int)d->out_c; g.log2span = igemm_ilog2(d->out_c);
  g.kw = d->kw; g.stride = d->stride; g.pad = d->pad; g.transposed = 1;
  g.K = (int)(d->kh * d->kw * d->out_c); g.N = (int)d->in_c; g.check_bounds = 1;
  igemm_finish_geom(g);
  return g;
}
// The shape check of every stem entry point (they take no creid_conv_desc, so check_desc never sees them): CREID_E_ARG for a
// non-positive extent, CREID_E_SHAPE for an odd H or W and for a size the kernels' index arithmetic does not hold --
//   * rows: fast_divmod decomposes a GEMM row with fp32 reciprocals, exact below 2^24 only (check_desc's limit for every other
//     convolution), and stem_geom narrows B * (H/2) * (W/2) to int;
//   * source: the kernels form the PIXEL index (b * SH + iy) * SW + ix of the padded image in int and widen it to 64 bits only
//     for the x 4 of the channel pitch, so B * (H + 8) * (W + 6) must fit an int.
// 0 otherwise.  Called before anything is launched.
static inline int stem_check_shape(int64_t B, int64_t H, int64_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return CREID_E_ARG;
  if (H % 2 || W % 2) return CREID_E_SHAPE;
  const int64_t lim = 1LL << 24;
  if (B >= lim || H / 2 >= lim || W / 2 >= lim || (H / 2) * (W / 2) >= lim) return CREID_E_SHAPE;   // (no 64-bit overflow below)
  if (B * ((H / 2) * (W / 2)) >= lim) return CREID_E_SHAPE;
  if (B * ((H + 8) * (W + 6)) > 0x7fffffffLL) return CREID_E_SHAPE;
  return 0;
}

// The stem (7x7 s2 on the pre-padded NHWC4 image [B, H + 8, W + 6, 4]): a "tap" is one kernel row of 8 pixels x 4 channels.
// Callers check stem_check_shape first: the narrowing casts below are then exact.
static inline IGemmGeom stem_geom(int64_t B, int64_t H, int64_t W) {
  IGemmGeom g;
  g.M = (int)(B * (H / 2) * (W / 2)); g.OH = (int)(H / 2); g.OW = (int)(W / 2);
  g.SH = (int)(H + 8); g.SW = (int)(W + 6); g.pitch = 4; g.log2span = 5;
  g.kw = 1; g.stride = 2; g.pad = 0; g.transposed = 0; g.K = 256; g.N = 64; g.check_bounds = 0;
  igemm_finish_geom(g);
  return g;
}

// Source pixel of output row (oy, ox) under tap (r, s); returns false when it falls outside.
// stride is 1 or 2 (check_desc / the stem), so the lattice test and the division are a mask and a shift --
// a runtime `%` and `/` here expand to ~60 VALU instructions per row on the k-loop path of every conv kernel.
__device__ __forceinline__ bool igemm_src_pixel(const IGemmGeom& g, int oy, int ox, int r, int s, int& iy, int& ix) {
  const int sh = g.stride - 1;                       // log2(stride); for stride 2 also the parity mask
  if (!g.transposed) {
    iy = (oy << sh) + r - g.pad;
    ix = (ox << sh) + s - g.pad;
  } else {
    const int ty = oy + g.pad - r, tx = ox + g.pad - s;
    if (((ty | tx) & sh) != 0) return false;         // not on the stride lattice
    iy = ty >> sh; ix = tx >> sh;                    // arithmetic shift: negatives stay negative, rejected below
  }
  if (!g.check_bounds) return true;
  return (unsigned)iy < (unsigned)g.SH && (unsigned)ix < (unsigned)g.SW;
}

// m / d and m % d for 0 <= m < 2^24 (exact in fp32) with a precomputed reciprocal: ~8 VALU ops instead
// of the ~25-op integer division sequence (the row -> (b, oy, ox) decomposition is on the k-loop path
// of the weight-gradient kernel).
__device__ __forceinline__ void fast_divmod(int m, int d, float inv_d, int& q, int& r) {
  q = (int)((float)m * inv_d);
  r = m - q * d;
  if (r >= d) { ++q; r -= d; }
  if (r < 0) { --q; r += d; }
}

// Optional fusion of the NEXT BatchNorm-backward's column reduction into a data-gradient epilogue: the tile
// just produced is g = dL/da for the layer whose raw conv output is `x` and post-ReLU activation is `act`;
// the epilogue accumulates (sum dy, sum dy*xhat), dy = g*[act>0], per channel into
// partial[tile_m][2][N] (the layout creid_bn2d_bwd expects, one row pair per 128 rows).
struct BnRedArgs {
  const void* x;
  const void* act;       // nullable: no ReLU mask
  const float* mean;
  const float* invstd;
  float* partial;
  int tiles_per_image;   // 0: mean/invstd are per channel [N]; > 0: per (image, channel) [B][N] (IBN), this many
                         // 128-row tiles per image
  const unsigned char* mask;   // nullable: ReLU mask as bits (creid_bn2d_apply_mask), one byte per 8 channels; replaces `act`
};

// XCD-aware bijective remap of the linear workgroup id (consecutive ids land on different XCDs;
// give every XCD a contiguous run of tiles so neighbouring tiles share operand panels in its L2).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int base = (xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  return base + (bid >> 3);
}

template <typename T> struct ElemIO;
template <> struct ElemIO<float> {
  static constexpr int DT = CREID_F32;
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct ElemIO<_Float16> {
  static constexpr int DT = CREID_F16;
  static __device__ __forceinline__ float ld(const _Float16* p) { return (float)*p; }
  static __device__ __forceinline__ void st(_Float16* p, float v) { *p = (_Float16)v; }
};
template <> struct ElemIO<unsigned short> {   // bf16 bits
  static constexpr int DT = CREID_BF16;
  static __device__ __forceinline__ float ld(const unsigned short* p) { return bf16_bits_to_f32(*p); }
  static __device__ __forceinline__ void st(unsigned short* p, float v) { *p = f32_to_bf16_bits(v); }
};
