// The per-output chain of the thin pooled first layer (3x3, C == 1,
// stride 1: FEMNIST conv1), shared by gemm_thin_conv_pool_kernel
// (gemm_bf16.hip) and the stage of the fused grad-free conv stack
// (halo_conv.hip). Both kernels call this one helper, so their bits
// cannot drift apart.
#pragma once

#include "common.h"

namespace bflc {
namespace thin {

typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef uint8_t u8x8 __attribute__((ext_vector_type(8)));

// Eight channels of one POOLED output from its 4x4 input patch.
//   pd     the patch, fp32-widened bf16 pixels (out-of-image ones +0),
//          each duplicated into a pair for the packed FMAs
//   wl     fp32-widened weights of these eight channels, tap-major:
//          wl[k * wstride + j], k = r*3 + s
//   bl     their fp32-widened biases
// Every conv output of window q = dy*2 + dx starts from the bias, takes
// the nine taps ascending - each one fused multiply-add - and then one
// `+ 0.f`: the kernel this chain comes from ran K padded to 16, and each
// of its seven padding taps was fma(+0, +0, acc) = acc + (+0), which
// leaves every value as it is except -0 -> +0; seven of them equal one.
// Then ReLU, the rounding to bf16, the pool kernel's running max over
// q = 0..3 (strict > from -inf; IDX keeps the argmax code) and the
// second rounding.
template <bool IDX>
__device__ __forceinline__ void conv_pool_chain(const f32x2 (&pd)[4][4],
                                                const float* wl, int wstride,
                                                const float* bl, int relu,
                                                bf16x8& out, u8x8& oidx) {
  f32x8 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = *reinterpret_cast<const f32x8*>(bl);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const f32x8 bv = *reinterpret_cast<const f32x8*>(&wl[k * wstride]);
    const f32x2* bv2 = reinterpret_cast<const f32x2*>(&bv);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x2 a = pd[(q >> 1) + k / 3][(q & 1) + k % 3];
      f32x2* acc2 = reinterpret_cast<f32x2*>(&acc[q]);
#pragma unroll
      for (int p = 0; p < 4; ++p) acc2[p] += bv2[p] * a;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = acc[q] + 0.f;
  if constexpr (!IDX) {
    // Without the argmax the tail folds, same bits. ReLU and the
    // rounding are monotone and no value is -0 after the `+ 0.f`, so the
    // running max of the rounded ReLUs is the rounded ReLU of the max,
    // and rounding it a second time changes nothing. A NaN output fails
    // `f > best` and is skipped; fmaxf skips it too (it returns its
    // non-NaN operand). Four NaNs leave `best` at -inf: the last fmaxf.
    // The tail is then 6 VALU instructions a channel where the literal
    // form below takes about 35.
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float m = fmaxf(fmaxf(acc[0][j], acc[1][j]),
                      fmaxf(acc[2][j], acc[3][j]));
      if (relu && m < 0.f) m = 0.f;
      out[j] = f2b(fmaxf(m, -INFINITY));
    }
    return;
  }
  float best[8];
  int bi[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; bi[j] = 0; }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = acc[q][j];
      if (relu && v < 0.f) v = 0.f;
      const float f = b2f(f2b(v));
      if (f > best[j]) {
        best[j] = f;
        if (IDX) bi[j] = q;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = f2b(best[j]);
  if (IDX) {
#pragma unroll
    for (int j = 0; j < 8; ++j) oidx[j] = (uint8_t)bi[j];
  }
}

}  // namespace thin
}  // namespace bflc
