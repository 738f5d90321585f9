// Input side of the path, first step: the Resize of datasets/transforms/build.py:17,28 (T.Resize(size) on a PIL RGB image =
// Image.resize((W, H), BILINEAR)) on a RAGGED uint8 batch -- images of any size packed back to back -- with Pillow's own
// fixed-point arithmetic, so the result EQUALS Pillow's byte for byte (tests/test_resize_gpu.py).  The arithmetic (include/creid.h
// spells it out): two separable passes, horizontal then vertical, 22-bit integer coefficients, the intermediate rounded to uint8.
// The coefficients are made on the host in float64 (transforms.resample_table); this kernel does integer work only.
//
// Shape: a workgroup owns RS_TY x RS_TX output pixels of one image; each of its four waves owns RS_RW output rows, a lane one
// output column.  The wave walks the source rows its output rows need ONCE: the lane forms the horizontally resampled, uint8-
// rounded value of its column for that source row (the tap count is a runtime value, nothing truncates a heavy downscale) and
// adds k_y * value into the int32 accumulators of those of its RS_RW output rows whose tap range holds the source row -- the
// intermediate image lives in three registers and never reaches memory.  Row bookkeeping is wave-uniform (scalar registers and
// branches); a source pixel is read with one unaligned dword load, correct at any alignment (3 h w is odd for odd sizes).
// Nothing read from the device-side metadata can send an access out of bounds: image extents are checked against `src_bytes`,
// table extents against `table_len`, and every tap range is clamped into its image; an image that fails a check comes out
// black.
#include "common.hpp"

namespace {
constexpr int RS_TX = 64;                  // output columns per workgroup (one per lane)
constexpr int RS_RW = 8;                   // output rows per wave
constexpr int RS_WAVES = 4;
constexpr int RS_TY = RS_RW * RS_WAVES;    // output rows per workgroup
constexpr int RS_BITS = 22;                // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)

struct ResizeArgs {
  const unsigned char* src;
  const int64_t* off;
  const int* size;
  const int* tab;
  const int* tab_off;
  unsigned char* out;
  int64_t src_bytes, tab_len, tiles;
  int B, H, W, tiles_x, tiles_y;
};

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }
// taps per output sample of an (n_in -> n_out) table: 2 ceil(max(n_in / n_out, 1)) + 1, in integers
__device__ __forceinline__ int rs_ksize(int n_in, int n_out) { return 2 * max((n_in + n_out - 1) / n_out, 1) + 1; }

// The three bytes of a pixel (r | g << 8 | b << 16) at ANY byte address: one unaligned dword load where the byte behind the pixel
// is still inside the buffer (gfx950 under HSA serves unaligned global loads; the fourth byte is dropped), three byte loads else.
__device__ __forceinline__ unsigned rs_pixel(const unsigned char* p, bool wide) {
  if (wide) {
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
  }
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

__global__ __launch_bounds__(256) void resize_u8_kernel(ResizeArgs a) {
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    const int tx = (int)(t % a.tiles_x);
    const int ty = (int)((t / a.tiles_x) % a.tiles_y);
    const int b = (int)(t / ((int64_t)a.tiles_x * a.tiles_y));
    const int y0 = ty * RS_TY + wv * RS_RW;
    if (y0 >= a.H) continue;                                            // wave-uniform
    const int x = tx * RS_TX + lane;
    const bool col_ok = x < a.W;
    const int h = a.size[2 * b], w = a.size[2 * b + 1];
    const int64_t o = a.off[b];
    const int64_t xt = a.tab_off[2 * b], yt = a.tab_off[2 * b + 1];
    bool ok = h >= 1 && h <= 16384 && w >= 1 && w <= 16384 && o >= 0 && o <= a.src_bytes && 3LL * h * w <= a.src_bytes - o;
    int kx = 3, ky = 3;
    if (ok) {
      kx = rs_ksize(w, a.W);
      ky = rs_ksize(h, a.H);
      ok = xt >= 0 && yt >= 0 && xt + (int64_t)a.W * (2 + kx) <= a.tab_len && yt + (int64_t)a.H * (2 + ky) <= a.tab_len;
    }
    unsigned char* dst = a.out + (((int64_t)b * a.H + y0) * a.W + x) * 3;
    if (!ok) {                                                          // never trust an extent that does not fit its buffer
      for (int r = 0; r < RS_RW; ++r)
        if (y0 + r < a.H && col_ok) { unsigned char* q = dst + (int64_t)r * a.W * 3; q[0] = 0; q[1] = 0; q[2] = 0; }
      continue;
    }
    const int* xb = a.tab + xt;                                         // {xmin, n} per output column, then kx coefficients each
    const int* yb = a.tab + yt;
    const int* xk = xb + 2 * (int64_t)a.W;
    const int* yk = yb + 2 * (int64_t)a.H;
    int ymin[RS_RW], yn[RS_RW], s_lo = h, s_hi = 0;
#pragma unroll
    for (int r = 0; r < RS_RW; ++r) {
      ymin[r] = 0; yn[r] = 0;
      if (y0 + r < a.H) {
        ymin[r] = min(max(yb[2 * (y0 + r)], 0), h);
        yn[r] = min(min(max(yb[2 * (y0 + r) + 1], 0), h - ymin[r]), ky);
        if (yn[r] > 0) { s_lo = min(s_lo, ymin[r]); s_hi = max(s_hi, ymin[r] + yn[r]); }
      }
    }
    int xmin = 0, xn = 0;
    if (col_ok) {
      xmin = min(max(xb[2 * x], 0), w);
      xn = min(min(max(xb[2 * x + 1], 0), w - xmin), kx);
      xk += (int64_t)x * kx;
    }
    int acc[RS_RW][3];
#pragma unroll
    for (int r = 0; r < RS_RW; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (RS_BITS - 1);
    const unsigned char* img = a.src + o;
    const int64_t avail = a.src_bytes - o;                              // bytes from the image's first to the buffer's last
    for (int sy = s_lo; sy < s_hi; ++sy) {
      const int64_t q = ((int64_t)sy * w + xmin) * 3;
      const unsigned char* p = img + q;
      const bool wide = q + 3 * (int64_t)xn + 1 <= avail;               // false only at the very end of the buffer
      int h0 = 1 << (RS_BITS - 1), h1 = h0, h2 = h0;
      for (int i = 0; i < xn; ++i) {
        const int k = xk[i];
        const unsigned v = rs_pixel(p + 3 * i, wide);
        h0 += k * (int)(v & 255u); h1 += k * (int)((v >> 8) & 255u); h2 += k * (int)((v >> 16) & 255u);
      }
      h0 = clip8(h0 >> RS_BITS); h1 = clip8(h1 >> RS_BITS); h2 = clip8(h2 >> RS_BITS);   // the uint8 intermediate image
#pragma unroll
      for (int r = 0; r < RS_RW; ++r) {
        const int d = sy - ymin[r];
        if ((unsigned)d < (unsigned)yn[r]) {                            // wave-uniform
          const int k = yk[(int64_t)(y0 + r) * ky + d];
          acc[r][0] += k * h0; acc[r][1] += k * h1; acc[r][2] += k * h2;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RS_RW; ++r) {
      if (y0 + r < a.H && col_ok) {
        unsigned char* q = dst + (int64_t)r * a.W * 3;
        q[0] = (unsigned char)clip8(acc[r][0] >> RS_BITS);
        q[1] = (unsigned char)clip8(acc[r][1] >> RS_BITS);
        q[2] = (unsigned char)clip8(acc[r][2] >> RS_BITS);
      }
    }
  }
}
}  // namespace

extern "C" int creid_resize_u8(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int32_t* sizes,
                               const int32_t* tables, int64_t table_len, const int32_t* table_offsets, int64_t B, int64_t H,
                               int64_t W, uint8_t* out, void* stream) {
  CREID_CHECK_ARG(src && offsets && sizes && tables && table_offsets && out);
  CREID_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && src_bytes > 0 && table_len > 0);
  CREID_CHECK_ARG(B <= 0x7fffffffLL && B * (H + 8) * (W + 6) < (1LL << 40));       // the bound of creid_augment_u8, which reads `out`
  ResizeArgs a;
  a.src = src; a.off = offsets; a.size = sizes; a.tab = tables; a.tab_off = table_offsets; a.out = out;
  a.src_bytes = src_bytes; a.tab_len = table_len;
  a.B = (int)B; a.H = (int)H; a.W = (int)W;
  a.tiles_x = (int)((W + RS_TX - 1) / RS_TX);
  a.tiles_y = (int)((H + RS_TY - 1) / RS_TY);
  a.tiles = B * a.tiles_x * a.tiles_y;
  const unsigned blocks = (unsigned)(a.tiles < (1LL << 20) ? a.tiles : (1LL << 20));
  hipLaunchKernelGGL(resize_u8_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), a);
  CREID_LAUNCH_RET();
}
