// Fixed-order fp32 sum of squares (gfx950), shared by the gradient clip
// (optimizer.hip) and the update clip of the privacy path (privacy.hip).
//
// One definition of the lane walk, the block reduction and the geometry,
// so that every caller sums in the same order and a fused producer
// (delta_extract_sumsq_) gives bitwise the sum of the stand-alone pass
// over the values it stored. Geometry is a function of n alone.
#pragma once

#include "common.h"

#include <algorithm>
#include <cstdint>

namespace bflc {

constexpr int kOptBlock = 256;                 // 4 waves
constexpr int kOptWaves = kOptBlock / kWave;
constexpr int kGran = 8;                       // elements per lane granule
constexpr int kSumsqMaxBlocks = 1024;          // <= 4 partials per final lane

typedef __attribute__((ext_vector_type(8))) unsigned short us8_t;

// one 8-element granule -> fp32 (bf16: one 16-B load; fp32: two)
__device__ __forceinline__ void load8(const bf16* __restrict__ g, long k,
                                      float (&o)[kGran]) {
  const us8_t v = reinterpret_cast<const us8_t*>(g)[k];
#pragma unroll
  for (int j = 0; j < kGran; ++j)
    o[j] = __uint_as_float((unsigned)v[j] << 16);  // exact widening
}

__device__ __forceinline__ void load8(const float* __restrict__ g, long k,
                                      float (&o)[kGran]) {
  const float4 a = reinterpret_cast<const float4*>(g)[2 * k];
  const float4 b = reinterpret_cast<const float4*>(g)[2 * k + 1];
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

__device__ __forceinline__ void store8(float* __restrict__ p, long k,
                                       const float (&o)[kGran]) {
  reinterpret_cast<float4*>(p)[2 * k] = make_float4(o[0], o[1], o[2], o[3]);
  reinterpret_cast<float4*>(p)[2 * k + 1] =
      make_float4(o[4], o[5], o[6], o[7]);
}

__device__ __forceinline__ float ld1(const bf16* g, long k) {
  return b2f(g[k]);
}
__device__ __forceinline__ float ld1(const float* g, long k) { return g[k]; }

// Fixed block reduction: 6-level wave xor tree (offsets 32..1), then the
// 4 waves ascending through LDS. Valid in thread 0 only.
__device__ __forceinline__ float block_sum_fixed(float v) {
  __shared__ float ws[kOptWaves];
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) ws[threadIdx.x / kWave] = v;
  __syncthreads();
  float s = ws[0];
#pragma unroll
  for (int w = 1; w < kOptWaves; ++w) s += ws[w];
  return s;
}

// One lane's chain of sum(x^2) over an n-element vector. Lane i (global)
// walks granules i, i + T, i + 2T, ... (T = gridDim * 256) in ascending
// order, eight fmaf(x, x, acc) per granule in element order, then (lane
// i < n % 8) the tail element n8*8 + i — one fp32 chain per lane.
// granule(k, x) fills the 8 values of granule k, tail(t) returns element
// t; a producer stores them there as well.
template <class Granule, class Tail>
__device__ __forceinline__ float sumsq_lane(long n, Granule&& granule,
                                            Tail&& tail) {
  const long i = (long)blockIdx.x * kOptBlock + threadIdx.x;
  const long stride = (long)gridDim.x * kOptBlock;
  const long n8 = n / kGran;
  float acc = 0.f;
  for (long k = i; k < n8; k += stride) {
    float x[kGran];
    granule(k, x);
#pragma unroll
    for (int j = 0; j < kGran; ++j) acc = fmaf(x[j], x[j], acc);
  }
  const long t = n8 * kGran + i;
  if (t < n) {
    const float x = tail(t);
    acc = fmaf(x, x, acc);
  }
  return acc;
}

struct SumsqGeom { int blocks; long per_lane; int depth; };

// Sum-of-squares geometry from n alone: one granule per lane until the
// 1024-block cap, then a grid-stride walk. per_lane is the longest lane
// chain in elements; depth the adds after it (wave tree 6 + waves 4 in
// each of the two kernels, + <= 4 partials per final lane).
inline SumsqGeom sumsq_geom(long n) {
  SumsqGeom s;
  const long n8 = n / kGran;
  const long blocks = (n8 + kOptBlock - 1) / kOptBlock;
  s.blocks = (int)std::min<long>(std::max<long>(blocks, 1), kSumsqMaxBlocks);
  const long lanes = (long)s.blocks * kOptBlock;
  s.per_lane = kGran * ((n8 + lanes - 1) / lanes) + (n % kGran ? 1 : 0);
  s.depth = 2 * (6 + kOptWaves) + kSumsqMaxBlocks / kOptBlock;
  return s;
}

inline bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<std::uintptr_t>(t.data_ptr()) % 16 == 0;
}

#define CHECK_ALIGN16(t) \
  TORCH_CHECK(aligned16(t), #t " must be 16-byte aligned")

inline void check_scalar_dev(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.numel() >= 1,
              name, " must be a contiguous fp32 GPU tensor");
}

// grad_clip_final_kernel (optimizer.hip) on the current stream:
// out[0] = coef, out[1] = ss when nout > 1.
void launch_grad_clip_final(const float* part, int nparts, float clip,
                            float* out, int nout);

}  // namespace bflc
