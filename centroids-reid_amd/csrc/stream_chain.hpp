// The fp32 dot product of ONE (query row, gallery row) pair with the bits of the fp32 distance kernels, without an MFMA: a
// v_mfma_f32_32x32x2_f32 accumulation is the sequential fmaf chain over ascending k from zero, which this reproduces with plain
// fmaf in the same order; the caller finishes with the kernels' epilogue fmaf(-2, acc, qq + gg).  One copy, shared by
// stream_poslist_kernel (stream_eval.hip: a query's positives) and stream_topk_rescore_kernel (stream_prefilter.hip: the pairs a
// 16-bit pre-filter kept).
//
// STREAM_FMAF_CHAIN(acc, qrow, grow, D) declares `float acc` and leaves the dot product in it.  qrow, grow: names of
// `const float*` variables; grow 16-byte aligned with D % 4 == 0 (or D < 16); qrow is meant to be wave-uniform, so that its values
// arrive through the scalar cache.  Two 64-byte blocks of the gallery row are in flight while a third is chained: the loop is
// bound by the load round trip to the Infinity Cache, not by the 16 dependent FMAs of a block.
// A macro on purpose: stream_poslist_kernel was measured and pinned with this text in its body, and as a __forceinline__ function
// (pointers, or bases and offsets, with and without __restrict__) the compiler derives the query row's scalar addresses
// differently; expanded in place the kernel's instruction stream is the one it had.
#pragma once
#include "common.hpp"

#define STREAM_FMAF_CHAIN(acc, qrow, grow, D)                                                                                                                     \
  float acc = 0.f;                                                                                                                                                \
  {                                                                                                                                                               \
    int k_ = 0;                                                                                                                                                   \
    const int kend_ = (D) & ~15;                                                                                                                                  \
    float4 n0_, n1_, n2_, n3_, m0_, m1_, m2_, m3_;                                                                                                                \
    if (kend_ > 0) {                                                                                                                                              \
      n0_ = *reinterpret_cast<const float4*>(grow); n1_ = *reinterpret_cast<const float4*>(grow + 4);                                                             \
      n2_ = *reinterpret_cast<const float4*>(grow + 8); n3_ = *reinterpret_cast<const float4*>(grow + 12);                                                        \
      const int k1_ = min(16, kend_ - 16);                                                                                                                        \
      m0_ = *reinterpret_cast<const float4*>(grow + k1_); m1_ = *reinterpret_cast<const float4*>(grow + k1_ + 4);                                                 \
      m2_ = *reinterpret_cast<const float4*>(grow + k1_ + 8); m3_ = *reinterpret_cast<const float4*>(grow + k1_ + 12);                                            \
    }                                                                                                                                                             \
    for (; k_ < kend_; k_ += 16) {                                                                                                                                \
      const float4 v0_ = n0_, v1_ = n1_, v2_ = n2_, v3_ = n3_;                                                                                                    \
      n0_ = m0_; n1_ = m1_; n2_ = m2_; n3_ = m3_;                                                                                                                 \
      const int kn_ = min(k_ + 32, kend_ - 16);                                                                                                                   \
      m0_ = *reinterpret_cast<const float4*>(grow + kn_); m1_ = *reinterpret_cast<const float4*>(grow + kn_ + 4);                                                 \
      m2_ = *reinterpret_cast<const float4*>(grow + kn_ + 8); m3_ = *reinterpret_cast<const float4*>(grow + kn_ + 12);                                            \
      acc = fmaf(qrow[k_ + 0], v0_.x, acc); acc = fmaf(qrow[k_ + 1], v0_.y, acc); acc = fmaf(qrow[k_ + 2], v0_.z, acc); acc = fmaf(qrow[k_ + 3], v0_.w, acc);     \
      acc = fmaf(qrow[k_ + 4], v1_.x, acc); acc = fmaf(qrow[k_ + 5], v1_.y, acc); acc = fmaf(qrow[k_ + 6], v1_.z, acc); acc = fmaf(qrow[k_ + 7], v1_.w, acc);     \
      acc = fmaf(qrow[k_ + 8], v2_.x, acc); acc = fmaf(qrow[k_ + 9], v2_.y, acc); acc = fmaf(qrow[k_ + 10], v2_.z, acc); acc = fmaf(qrow[k_ + 11], v2_.w, acc);   \
      acc = fmaf(qrow[k_ + 12], v3_.x, acc); acc = fmaf(qrow[k_ + 13], v3_.y, acc); acc = fmaf(qrow[k_ + 14], v3_.z, acc); acc = fmaf(qrow[k_ + 15], v3_.w, acc); \
    }                                                                                                                                                             \
    for (; k_ < (D); ++k_) acc = fmaf(qrow[k_], grow[k_], acc);                                                                                                   \
  }
