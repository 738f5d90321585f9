// C-tile epilogue primitives of the 16-bit implicit-GEMM convolution kernels (conv_igemm.hip's LDS-DMA tile kernels,
// conv_pipe.hip, conv_stream.hip, conv_pair.hip).  Every one of them leaves its accumulators the same way:
//   1. the C tile (or a piece of it) is staged COLUMN-major in LDS: a lane's four consecutive accumulator rows of one column
//      are one packed 8-byte store (2 conversions + 1 ds_write_b64 per 4 values; a row-major image took a 2-byte store per
//      value).  Column pitch CPT = rows + 4 elements, i.e. 8 bytes past a multiple of 256: 16 consecutive columns start 2 banks
//      apart (conflict-free b64 stores), and so do the 4 x 4 units of a transposing read;
//   2. the copy-out gets row-major 16-byte chunks back through the transposing LDS read, each thread owning one row of a row
//      quad and one column octet per pass;
//   3. per chunk: optional "+ residual" (optional bit mask on the residual, optional ReLU after the add), optional
//      BatchNorm-backward column accumulation, store.
// What differs between the callers (thread count, tile shape, where the chunks go) is a template parameter or stays in the
// caller; nothing here branches on the kernel it is inlined into.
#pragma once
#include "conv_common.hpp"

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Copy-out map.  A wave's pass covers 16 (row quad, column octet) units of the staged image, numbered row-quad major with CPR
// octets per row; pass i of wave w takes units (w + WS * i) * 16 .. + 15 (WS = waves that copy out).  Lane 4 * u + t stores
// row t of the row quad of unit u of the pass (a 16-lane group: 4 rows x 4 octets), so a thread's column octet is the same
// in every pass.  rl = row inside the staged image, ch = column octet.
template <int WS, int CPR>
__device__ __forceinline__ void copy_unit(int lane, int wave, int i, int& rl, int& ch) {
  const int Q = (wave + WS * i) * 16 + (lane >> 2);
  ch = Q % CPR;
  rl = 4 * (Q / CPR) + (lane & 3);
}

// Staging store of one lane's share of a 32 x 32 accumulator block: column l31, rows 8 * q + 4 * kh + 0..3 for q = 0..3.
// `col` points at (this column, row 4 * kh of the block) of the staged image.  affine: y = fmaf(acc, sc, sh) on the fp32
// accumulators (folded eval-mode BatchNorm; a lane's column is fixed per block), ReLU here when `relu`.
template <typename ET>
__device__ __forceinline__ void stage_block(unsigned short* col, const f32x16& acc, bool affine = false, float sc = 1.f,
                                            float sh = 0.f, bool relu = false) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v0 = acc[4 * q], v1 = acc[4 * q + 1], v2 = acc[4 * q + 2], v3 = acc[4 * q + 3];
    if (affine) {
      v0 = fmaf(v0, sc, sh); v1 = fmaf(v1, sc, sh); v2 = fmaf(v2, sc, sh); v3 = fmaf(v3, sc, sh);
      if (relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
    }
    *reinterpret_cast<uint2*>(col + 8 * q) = make_uint2(ET::pack2(v0, v1), ET::pack2(v2, v3));
  }
}
// Forward BatchNorm statistics: (s1, s2) += (sum, sum of squares) of the lane's 16 fp32 accumulators of a block, the four
// values of a quad in sequence, quad after quad; once all blocks of a column went in, the two lane halves (rows 4 * kh + ..
// of the same column) are added.  The order is part of the result: every kernel of the family sums this way.
__device__ __forceinline__ void colsum_block(const f32x16& acc, float& s1, float& s2) {
#pragma unroll
  for (int r = 0; r < 16; ++r) { const float v = acc[r]; s1 += v; s2 = fmaf(v, v, s2); }
}
__device__ __forceinline__ void colsum_lane_halves(float& s1, float& s2) {
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
}

// Transposing read-back of this thread's NIT chunks of the staged image (pitch CPT elements), in copy_unit's map.  In a
// 16-lane group lane s supplies the 8-byte unit (column 8 * octet(s & 3) + (s >> 2), the row quad) and lane l receives (row
// l & 3, columns 8 * octet(l >> 2) + 0..3); a second read 4 columns on completes the 16-byte chunk.  Every lane takes part
// (the data crosses lanes): only the caller's global store is predicated.  Returns once the data is there (lgkmcnt(0); the
// registers are pinned behind the wait, the compiler does not know the asm reads are asynchronous).
template <int NIT, int WS, int CPR, int CPT>
__device__ __forceinline__ void read_back_chunks(const unsigned short* stage, int lane, int wave, uint4 (&v)[NIT]) {
  u32x2 trlo[NIT], trhi[NIT];
  const int sq = lane & 3, sj = (lane >> 2) & 3;
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int Qs = (wave + WS * i) * 16 + (lane >> 4) * 4 + sq;
    const unsigned addr = (unsigned)(uintptr_t)&stage[((Qs % CPR) * 8 + sj) * CPT + 4 * (Qs / CPR)];
    asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%3"
                 : "=&v"(trlo[i]), "=&v"(trhi[i]) : "v"(addr), "i"(4 * CPT * 2) : "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < NIT; ++i) asm volatile("" : "+v"(trlo[i]), "+v"(trhi[i]));
#pragma unroll
  for (int i = 0; i < NIT; ++i) v[i] = make_uint4(trlo[i].x, trlo[i].y, trhi[i].x, trhi[i].y);
}

// v += a on a 16-byte chunk, in fp32, rounded once.  am: one bit per element, a cleared bit drops that element of `a` (the
// residual-branch gradient arrives unmasked plus its ReLU bits); relu: ReLU after the add (folded BatchNorm + residual).
template <typename ET>
__device__ __forceinline__ void add_chunk(uint4& v, const uint4& a, bool relu, unsigned am = 0xffu) {
  unsigned* vw = &v.x; const unsigned* aw = &a.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float alo = ((am >> (2 * q)) & 1u) ? ET::lo(aw[q]) : 0.f;
    const float ahi = ((am >> (2 * q + 1)) & 1u) ? ET::hi(aw[q]) : 0.f;
    float lo = ET::lo(vw[q]) + alo;
    float hi = ET::hi(vw[q]) + ahi;
    if (relu) { lo = fmaxf(lo, 0.f); hi = fmaxf(hi, 0.f); }
    vw[q] = ET::pack2(lo, hi);
  }
}

// BatchNorm-backward column accumulation of one chunk: g = the data gradient just produced (as stored), dy = g where the
// layer's activation `av` is positive and its mask bit in `mb` is set; rs1 += dy, rs2 += dy * (x - mean) * invstd per column.
template <typename ET>
__device__ __forceinline__ void bnred_chunk(const uint4& v, const uint4& xv, const uint4& av, unsigned mb, const float (&rmu)[8],
                                            const float (&ris)[8], float (&rs1)[8], float (&rs2)[8]) {
  const unsigned* vw = &v.x; const unsigned* xw = &xv.x; const unsigned* aw = &av.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float g0 = ET::lo(vw[q]), g1 = ET::hi(vw[q]);
    const float a0 = ET::lo(aw[q]), a1 = ET::hi(aw[q]);
    const float x0 = ET::lo(xw[q]), x1 = ET::hi(xw[q]);
    g0 = (a0 > 0.f && ((mb >> (2 * q)) & 1u)) ? g0 : 0.f; g1 = (a1 > 0.f && ((mb >> (2 * q + 1)) & 1u)) ? g1 : 0.f;
    rs1[2 * q] += g0; rs1[2 * q + 1] += g1;
    rs2[2 * q] = fmaf(g0, (x0 - rmu[2 * q]) * ris[2 * q], rs2[2 * q]);
    rs2[2 * q + 1] = fmaf(g1, (x1 - rmu[2 * q + 1]) * ris[2 * q + 1], rs2[2 * q + 1]);
  }
}
