// Differentially private updates (gfx950): clip a client's flat fp32
// update to an L2 bound and add Gaussian noise from a counter-based
// generator (DP-FedAvg, McMahan et al. 2018). Opt-in (FLConfig.dp_active).
//
// Three kernels, no atomics, no host sync, every launch geometry a
// function of n alone:
//
//   delta_extract_sumsq_kernel  out = (global - w) / lr AND the per-block
//                               partials of sum(out^2) in one pass, in
//                               the lane order of grad_sumsq_part_kernel
//                               (sumsq.h); grad_clip_final_kernel turns
//                               them into the device coefficient
//   dp_privatize_kernel         d = coef * d + sigma * z(i), in place
//   philox_words_kernel         test hook: the generator on given counters
//
// THE NOISE (DESIGN.md "Round-13"). z(i) is a pure function of (seed,
// stream, epoch, i): with b = i >> 2, e = i & 3, Philox4x32-10 on counter
// (b lo, b hi, stream, epoch) under key (seed lo, seed hi) gives x0..x3;
// u_j = ((x_j >> 8) + 0.5) * 2^-24; Box-Muller on (u0, u1) and (u2, u3)
// gives four normals, z(i) is the e-th. One generator call serves four
// consecutive coordinates, and nothing depends on the launch geometry,
// the access width, the stream or the rank. IEEE library functions only
// (logf, log1pf, sqrtf, sincospif) — no fast-math intrinsics.

#include "common.h"
#include "sumsq.h"

#include <cstdint>

namespace bflc {

namespace {

constexpr int kPrivMaxBlocks = 2048;  // 8 blocks per CU

struct Words { uint32_t x[4]; };

// Philox4x32-10 (Salmon et al., SC'11).
__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1,
                                               uint32_t c2, uint32_t c3,
                                               uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

// sqrt(-2 ln u), u = (k + 0.5) * 2^-24, k = x >> 8. k + 0.5 has 25
// significant bits once k >= 2^23, so u itself is exact in fp32 only in
// the lower half; in the upper half 1 - u = ((2^24 - 1 - k) + 0.5) * 2^-24
// is, and log1pf takes it. Rounding u instead would move the radius by
// 3e-8 / r, which is 1e-4 next to u = 1.
__device__ __forceinline__ float bm_radius(uint32_t x) {
  const uint32_t k = x >> 8;
  float l;
  if (k < (1u << 23)) {
    l = logf(((float)k + 0.5f) * 0x1p-24f);
  } else {
    l = log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 0x1p-24f));
  }
  return sqrtf(-2.f * l);
}

// (sin, cos) of 2 pi u = pi * t * 2^-24 with t = 2k + 1 in (0, 2^25).
// Half a turn is taken off in the integer, so the argument handed to
// sincospif (t odd, below 2^24) is exact.
__device__ __forceinline__ void bm_sincos(uint32_t x, float& s, float& c) {
  uint32_t t = 2u * (x >> 8) + 1u;
  const bool half = t >= (1u << 24);
  if (half) t -= 1u << 24;
  float sv, cv;
  sincospif((float)t * 0x1p-24f, &sv, &cv);
  s = half ? -sv : sv;
  c = half ? -cv : cv;
}

// The four normals of generator block b, scaled: o[e] = fp32(sigma * z).
__device__ __forceinline__ void noise4(long b, uint32_t stream,
                                       uint32_t epoch, uint32_t k0,
                                       uint32_t k1, float sigma,
                                       float (&o)[4]) {
  const Words w = philox4x32_10((uint32_t)b, (uint32_t)((uint64_t)b >> 32),
                                stream, epoch, k0, k1);
  const float r0 = bm_radius(w.x[0]), r1 = bm_radius(w.x[2]);
  float s0, c0, s1, c1;
  bm_sincos(w.x[1], s0, c0);
  bm_sincos(w.x[3], s1, c1);
  o[0] = sigma * (r0 * c0);
  o[1] = sigma * (r0 * s0);
  o[2] = sigma * (r1 * c1);
  o[3] = sigma * (r1 * s1);
}

// coef == 0 (non-finite update): the old value is not used at all.
template <bool NOISE>
__device__ __forceinline__ float privatize1(float coef, float d, float nz) {
  if (coef == 0.f) return nz;
  return NOISE ? fmaf(coef, d, nz) : coef * d;
}

// Grid-stride over generator blocks (4 coordinates each): one 16-B
// access per lane when the base is 16-byte aligned (VEC), four dword
// accesses at the same addresses otherwise; the P % 4 tail is scalar in
// both. NOISE = false (sigma == 0) is the clip alone: no generator work.
template <bool NOISE, bool VEC>
__global__ __launch_bounds__(kOptBlock) void dp_privatize_kernel(
    float* __restrict__ d, const float* __restrict__ coef_dev, float sigma,
    uint32_t k0, uint32_t k1, uint32_t stream, uint32_t epoch, long n) {
  const float coef = coef_dev[0];
  const long i = (long)blockIdx.x * kOptBlock + threadIdx.x;
  const long stride = (long)gridDim.x * kOptBlock;
  const long nb = n >> 2;
  for (long b = i; b < nb; b += stride) {
    float v[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (coef != 0.f) {
      if (VEC) {
        const float4 a = reinterpret_cast<const float4*>(d)[b];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = d[4 * b + e];
      }
    }
    if (NOISE) noise4(b, stream, epoch, k0, k1, sigma, nz);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = privatize1<NOISE>(coef, v[e], nz[e]);
    if (VEC) {
      reinterpret_cast<float4*>(d)[b] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) d[4 * b + e] = v[e];
    }
  }
  const int rem = (int)(n & 3);
  if (i == 0 && rem) {  // coordinates 4 nb .. n - 1 of generator block nb
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (NOISE) noise4(nb, stream, epoch, k0, k1, sigma, nz);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      if (e < rem) {
        const float old = coef != 0.f ? d[4 * nb + e] : 0.f;
        d[4 * nb + e] = privatize1<NOISE>(coef, old, nz[e]);
      }
    }
  }
}

__global__ __launch_bounds__(kOptBlock) void philox_words_kernel(
    const long* __restrict__ ctr, long* __restrict__ out, uint32_t k0,
    uint32_t k1, long rows) {
  const long r = (long)blockIdx.x * kOptBlock + threadIdx.x;
  if (r >= rows) return;
  const Words w = philox4x32_10((uint32_t)ctr[4 * r], (uint32_t)ctr[4 * r + 1],
                                (uint32_t)ctr[4 * r + 2],
                                (uint32_t)ctr[4 * r + 3], k0, k1);
#pragma unroll
  for (int e = 0; e < 4; ++e) out[4 * r + e] = (long)w.x[e];
}

// delta_extract_kernel's arithmetic (elementwise.hip: one fp32 subtract,
// one IEEE divide) feeding sumsq_lane: the lane that owns granule k of
// the sum computes and stores granule k of the update.
__global__ __launch_bounds__(kOptBlock) void delta_extract_sumsq_kernel(
    float* __restrict__ out, const float* __restrict__ gl,
    const float* __restrict__ w, float lr, float* __restrict__ part,
    long n) {
  const float acc = sumsq_lane(
      n,
      [&](long k, float (&x)[kGran]) {
        float a[kGran], b[kGran];
        load8(gl, k, a);
        load8(w, k, b);
#pragma unroll
        for (int j = 0; j < kGran; ++j) x[j] = (a[j] - b[j]) / lr;
        store8(out, k, x);
      },
      [&](long t) {
        const float x = (gl[t] - w[t]) / lr;
        out[t] = x;
        return x;
      });
  const float s = block_sum_fixed(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

inline void check_flat(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous(),
              name, " must be a contiguous fp32 GPU tensor");
}

}  // namespace

void delta_extract_sumsq_(torch::Tensor out, torch::Tensor global_flat,
                          torch::Tensor w, double lr, torch::Tensor part) {
  check_flat(out, "out"); CHECK_ALIGN16(out);
  check_flat(global_flat, "global_flat"); CHECK_ALIGN16(global_flat);
  check_flat(w, "w"); CHECK_ALIGN16(w);
  check_flat(part, "part");
  const long n = out.numel();
  TORCH_CHECK(global_flat.numel() == n && w.numel() == n,
              "out, global_flat and w differ in numel");
  const SumsqGeom s = sumsq_geom(n);
  TORCH_CHECK(part.numel() == s.blocks, "part must hold ", s.blocks,
              " partials (grad_sumsq_geom) for n = ", n);
  hipLaunchKernelGGL(delta_extract_sumsq_kernel, dim3(s.blocks),
                     dim3(kOptBlock), 0, cur_stream(), out.data_ptr<float>(),
                     global_flat.data_ptr<float>(), w.data_ptr<float>(),
                     (float)lr, part.data_ptr<float>(), n);
  HIP_CHECK(hipGetLastError());
}

void dp_privatize_(torch::Tensor d, torch::Tensor coef_dev, double sigma,
                   uint64_t seed, uint64_t stream, uint64_t epoch) {
  check_flat(d, "d");
  check_scalar_dev(coef_dev, "coef_dev");
  TORCH_CHECK(sigma >= 0.0, "sigma must be >= 0");
  TORCH_CHECK(stream <= 0xFFFFFFFFull && epoch <= 0xFFFFFFFFull,
              "stream and epoch are 32-bit");
  const long n = d.numel();
  if (n == 0) return;
  const long nb = (n + 3) / 4;
  const int blocks = (int)std::min<long>((nb + kOptBlock - 1) / kOptBlock,
                                         kPrivMaxBlocks);
  const bool noise = (float)sigma != 0.f;
  const bool vec = aligned16(d);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kOptBlock), 0,
                       cur_stream(), d.data_ptr<float>(),
                       coef_dev.data_ptr<float>(), (float)sigma,
                       (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)stream, (uint32_t)epoch, n);
  };
  if (noise) {
    if (vec) launch(dp_privatize_kernel<true, true>);
    else launch(dp_privatize_kernel<true, false>);
  } else {
    if (vec) launch(dp_privatize_kernel<false, true>);
    else launch(dp_privatize_kernel<false, false>);
  }
  HIP_CHECK(hipGetLastError());
}

torch::Tensor dp_philox_words(torch::Tensor ctr, uint64_t key0,
                              uint64_t key1) {
  TORCH_CHECK(ctr.is_cuda() && ctr.scalar_type() == at::kLong &&
                  ctr.is_contiguous() && ctr.dim() == 2 && ctr.size(1) == 4,
              "ctr must be a contiguous [N, 4] int64 GPU tensor");
  TORCH_CHECK(key0 <= 0xFFFFFFFFull && key1 <= 0xFFFFFFFFull,
              "key words are 32-bit");
  auto out = torch::empty_like(ctr);
  const long rows = ctr.size(0);
  if (rows == 0) return out;
  hipLaunchKernelGGL(philox_words_kernel, dim3(ceil_div(rows, kOptBlock)),
                     dim3(kOptBlock), 0, cur_stream(),
                     (const long*)ctr.data_ptr<int64_t>(),
                     (long*)out.data_ptr<int64_t>(), (uint32_t)key0,
                     (uint32_t)key1, rows);
  HIP_CHECK(hipGetLastError());
  return out;
}

}  // namespace bflc
