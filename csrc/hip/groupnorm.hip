// GroupNorm (NHWC, bf16, fp32 statistics) — gfx950.
//
// Statistics are per (sample, group) over H*W*cpg elements (cpg = C/G),
// so a sample's output never depends on what else shares its batch:
// the batch-independent alternative to batchnorm.hip for the ResNets
// (committee scores on label-skewed shards stop depending on the
// scorer's batch). Parameters are the same per-channel {gamma, beta},
// so the flat parameter layout is the BN model's.
//
// Every kernel reduces PER CHANNEL first (lane = one 16-B granule of 8
// channels, row-lanes combined by a fixed tree) and only then folds
// cpg consecutive channel sums into a group sum. That keeps the
// lane->group mapping trivial for every cpg: a 16-B vector spanning
// several groups (cpg < 8), a group spanning several vectors (cpg > 8)
// and cpg values that divide neither way all take the same path, and
// the backward's per-channel sums are the dgamma/dbeta partials anyway.
//
// Two routes, chosen from (H, W, C, G) only — never from N — so sample
// i of a batch runs exactly the instruction sequence it runs alone
// (bitwise per-sample invariance of y, mean, rstd and dx):
//   slab   H*W*C*2 B <= 64 KiB and C/8 a power of two <= 256: one
//          workgroup per sample holds the slab in registers, reads x
//          once, reduces mean then CENTRED variance from the on-chip
//          copy, writes y once. Backward likewise (x, dy, y read once).
//   split  anything else: grid (column blocks, row chunks, N) partial
//          pass -> per-(n, g) finalise over the chunks (fixed order) ->
//          vectorised normalise / dx pass.
// No atomics; all reductions are fixed trees (deterministic run to run
// and identical on every replica). No host sync, no allocation outside
// torch's allocator: safe inside hipGraph capture.

#include <cstdlib>
#include <cstring>
#include <string>

#include "common.h"

namespace bflc {

namespace {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

__device__ __forceinline__ float u2f(unsigned short u) {
  return __uint_as_float((unsigned)u << 16);
}
__device__ __forceinline__ unsigned short f2u(float f) {
  return __bfloat16_as_ushort(__float2bfloat16(f));
}

constexpr int kThreads = 256;
constexpr long kSlabBytes = 64 * 1024;  // 64 payload VGPRs per lane
constexpr int kSplitGranulesPerLane = 8;

// Sum v[0..8) over the row-lanes that share a channel granule. Lane
// layout: gi = t % GL (GL a power of two <= 256), rl = t / GL. The
// result is valid in threads t < GL. Fixed tree: xor-halving inside the
// wave (only when GL < 64), then the four waves / row-lanes ascending
// through LDS. `red` holds 256*8 floats and is reusable on return.
__device__ __forceinline__ void colsum8(float (&v)[8], int GL, float* red) {
  const int t = threadIdx.x;
  for (int off = 32; off >= GL; off >>= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += __shfl_xor(v[j], off, 64);
  }
  float4* r4 = reinterpret_cast<float4*>(red);
  r4[t * 2] = make_float4(v[0], v[1], v[2], v[3]);
  r4[t * 2 + 1] = make_float4(v[4], v[5], v[6], v[7]);
  __syncthreads();
  if (t < GL) {
    const int stride = GL < 64 ? 64 : GL;
    for (int k = t + stride; k < kThreads; k += stride) {
      const float4 a = r4[k * 2], b = r4[k * 2 + 1];
      v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
      v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------
// slab route: one workgroup per sample, slab cached in registers
// ---------------------------------------------------------------------

// 256 threads = RL row-lanes x cg channel granules (cg = C/8, a power of
// two); lane (rl, gi) owns rows rl, rl+RL, ... (at most NI of them).
template <int NI>
__global__ __launch_bounds__(kThreads) void gn_slab_fwd_kernel(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ res, int HW, int C, int G, float eps,
    int relu, unsigned short* __restrict__ y, float* __restrict__ mean,
    float* __restrict__ rstd) {
  extern __shared__ float4 gn_smem[];
  float* red = reinterpret_cast<float*>(gn_smem);  // 256*8
  float* chs = red + kThreads * 8;                 // C
  float* gm = chs + C;                             // G
  float* gr = gm + G;                              // G
  const int t = threadIdx.x;
  const int cg = C >> 3, RL = kThreads / cg;
  const int gi = t & (cg - 1), rl = t / cg;
  const int cpg = C / G, c8 = gi * 8;
  const long base = (long)blockIdx.x * HW * C;
  const float cnt = (float)HW * (float)cpg;

  u16x8 xr[NI];
  float s[8] = {};
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = rl + i * RL;
    if (row < HW) {
      xr[i] = *reinterpret_cast<const u16x8*>(&x[base + (long)row * C + c8]);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += u2f(xr[i][j]);
    } else {
      xr[i] = (u16x8)(0);
    }
  }
  colsum8(s, cg, red);
  if (t < cg) {
#pragma unroll
    for (int j = 0; j < 8; ++j) chs[c8 + j] = s[j];
  }
  __syncthreads();
  for (int g = t; g < G; g += kThreads) {
    float a = 0.f;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) a += chs[c];
    gm[g] = a / cnt;
  }
  __syncthreads();
  int grp[8];
  float mj[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    grp[j] = (c8 + j) / cpg;
    mj[j] = gm[grp[j]];
  }
  // centred second sweep over the on-chip copy: no E[x^2]-mean^2
  // cancellation
  float q[8] = {};
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (rl + i * RL < HW) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = u2f(xr[i][j]) - mj[j];
        q[j] += d * d;
      }
    }
  }
  colsum8(q, cg, red);
  if (t < cg) {
#pragma unroll
    for (int j = 0; j < 8; ++j) chs[c8 + j] = q[j];
  }
  __syncthreads();
  for (int g = t; g < G; g += kThreads) {
    float a = 0.f;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) a += chs[c];
    const float r = rsqrtf(a / cnt + eps);
    gr[g] = r;
    mean[(long)blockIdx.x * G + g] = gm[g];
    rstd[(long)blockIdx.x * G + g] = r;
  }
  __syncthreads();
  float sc[8], bt[8];
  {
    const u16x8 gv = *reinterpret_cast<const u16x8*>(&gamma[c8]);
    const u16x8 bv = *reinterpret_cast<const u16x8*>(&beta[c8]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sc[j] = gr[grp[j]] * u2f(gv[j]);
      bt[j] = u2f(bv[j]);
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = rl + i * RL;
    if (row < HW) {
      const long off = base + (long)row * C + c8;
      u16x8 rv;
      if (res) rv = *reinterpret_cast<const u16x8*>(&res[off]);
      u16x8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = (u2f(xr[i][j]) - mj[j]) * sc[j] + bt[j];
        if (res) f += u2f(rv[j]);
        if (relu) f = fmaxf(f, 0.f);
        out[j] = f2u(f);
      }
      *reinterpret_cast<u16x8*>(&y[off]) = out;
    }
  }
}

template <int NI>
__global__ __launch_bounds__(kThreads) void gn_slab_bwd_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ yr, const float* __restrict__ mean,
    const float* __restrict__ rstd, const unsigned short* __restrict__ gamma,
    int HW, int C, int G, unsigned short* __restrict__ dx,
    float* __restrict__ pdb, float* __restrict__ pdg) {
  extern __shared__ float4 gn_smem[];
  float* red = reinterpret_cast<float*>(gn_smem);  // 256*8
  float* ch1 = red + kThreads * 8;                 // C: sum dy
  float* ch2 = ch1 + C;                            // C: sum dy*xhat
  float* gm = ch2 + C;                             // G each below
  float* gr = gm + G;
  float* gA = gr + G;
  float* gB = gA + G;
  const int t = threadIdx.x;
  const int cg = C >> 3, RL = kThreads / cg;
  const int gi = t & (cg - 1), rl = t / cg;
  const int cpg = C / G, c8 = gi * 8;
  const long n = blockIdx.x;
  const long base = n * HW * C;
  const float cnt = (float)HW * (float)cpg;

  for (int g = t; g < G; g += kThreads) {
    gm[g] = mean[n * G + g];
    gr[g] = rstd[n * G + g];
  }
  u16x8 xr[NI], dr[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = rl + i * RL;
    if (row < HW) {
      const long off = base + (long)row * C + c8;
      xr[i] = *reinterpret_cast<const u16x8*>(&x[off]);
      dr[i] = *reinterpret_cast<const u16x8*>(&dy[off]);
      if (yr) {
        const u16x8 yv = *reinterpret_cast<const u16x8*>(&yr[off]);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!(u2f(yv[j]) > 0.f)) dr[i][j] = 0;
      }
    } else {
      xr[i] = (u16x8)(0);
      dr[i] = (u16x8)(0);
    }
  }
  __syncthreads();
  int grp[8];
  float mj[8], rj[8], gj[8];
  {
    const u16x8 gv = *reinterpret_cast<const u16x8*>(&gamma[c8]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      grp[j] = (c8 + j) / cpg;
      mj[j] = gm[grp[j]];
      rj[j] = gr[grp[j]];
      gj[j] = u2f(gv[j]);
    }
  }
  float s1[8] = {}, s2[8] = {};
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    // rows past HW hold dy = 0 and add nothing
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = u2f(dr[i][j]);
      s1[j] += g;
      s2[j] += g * ((u2f(xr[i][j]) - mj[j]) * rj[j]);
    }
  }
  colsum8(s1, cg, red);
  colsum8(s2, cg, red);
  if (t < cg) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ch1[c8 + j] = s1[j];
      ch2[c8 + j] = s2[j];
      pdb[n * C + c8 + j] = s1[j];
      pdg[n * C + c8 + j] = s2[j];
    }
  }
  __syncthreads();
  for (int g = t; g < G; g += kThreads) {
    float a = 0.f, b = 0.f;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
      const float gc = u2f(gamma[c]);
      a += gc * ch1[c];
      b += gc * ch2[c];
    }
    gA[g] = a / cnt;
    gB[g] = b / cnt;
  }
  __syncthreads();
  float aj[8], bj[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    aj[j] = gA[grp[j]];
    bj[j] = gB[grp[j]];
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = rl + i * RL;
    if (row < HW) {
      u16x8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (u2f(xr[i][j]) - mj[j]) * rj[j];
        out[j] = f2u(rj[j] * (gj[j] * u2f(dr[i][j]) - aj[j] - xh * bj[j]));
      }
      *reinterpret_cast<u16x8*>(&dx[base + (long)row * C + c8]) = out;
    }
  }
}

// ---------------------------------------------------------------------
// split route
// ---------------------------------------------------------------------

// Partial pass, grid (column blocks, row chunks, N): per-(n, chunk,
// channel) sum and sum of squares. 256 threads = RL row-lanes x GL
// granule lanes (GL = pow2 <= min(C/8, 256)).
__global__ __launch_bounds__(kThreads) void gn_part_kernel(
    const unsigned short* __restrict__ x, int HW, int C, int GL,
    int chunk_rows, float* __restrict__ psum, float* __restrict__ psq) {
  __shared__ float4 red4[kThreads * 2];
  float* red = reinterpret_cast<float*>(red4);
  const int t = threadIdx.x;
  const int gi = t & (GL - 1), rl = t / GL, RL = kThreads / GL;
  const int c8 = (blockIdx.x * GL + gi) * 8;
  const bool ok = c8 < C;
  const long n = blockIdx.z;
  const int r0 = blockIdx.y * chunk_rows;
  const int r1 = min(HW, r0 + chunk_rows);
  const unsigned short* xb = x + n * HW * C;
  float s[8] = {}, q[8] = {};
  if (ok)
#pragma unroll 4
    for (int m = r0 + rl; m < r1; m += RL) {
      const u16x8 v = *reinterpret_cast<const u16x8*>(&xb[(long)m * C + c8]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = u2f(v[j]);
        s[j] += f;
        q[j] += f * f;
      }
    }
  colsum8(s, GL, red);
  colsum8(q, GL, red);
  if (t < GL && ok) {
    const long o = (n * gridDim.y + blockIdx.y) * C + c8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      psum[o + j] = s[j];
      psq[o + j] = q[j];
    }
  }
}

// Finalise: one wave per (n, g). The chunks*cpg partials are numbered
// chunk-major; lane l adds entries l, l+64, l+128, ... in that order in
// fp64, then the 64 lane sums meet in an xor butterfly and lane 0
// writes. A fixed order (a function of chunks and cpg alone), though
// not one serial ascending walk. The statistics are E[x^2] - mean^2 on
// fp32 chunk sums combined in fp64, not the slab route's centred form.
__global__ __launch_bounds__(kThreads) void gn_stats_final_kernel(
    const float* __restrict__ psum, const float* __restrict__ psq, long NG,
    int chunks, int C, int G, double cnt, double eps,
    float* __restrict__ mean, float* __restrict__ rstd) {
  const long ng = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (ng >= NG) return;
  const int lane = threadIdx.x & 63;
  const int cpg = C / G;
  const long n = ng / G;
  const int g = (int)(ng % G);
  double S = 0.0, Q = 0.0;
  for (int e = lane; e < chunks * cpg; e += 64) {
    const long idx = (n * chunks + e / cpg) * C + g * cpg + e % cpg;
    S += (double)psum[idx];
    Q += (double)psq[idx];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    S += __shfl_xor(S, off, 64);
    Q += __shfl_xor(Q, off, 64);
  }
  if (lane == 0) {
    const double m = S / cnt;
    const double var = fmax(Q / cnt - m * m, 0.0);
    mean[ng] = (float)m;
    rstd[ng] = (float)(1.0 / sqrt(var + eps));
  }
}

// Normalise pass, grid (blocks per sample, N): the sample's folded
// per-channel scale/shift live in LDS, 16-B granules grid-stride the
// sample.
__global__ __launch_bounds__(kThreads) void gn_norm_kernel(
    const unsigned short* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ res, int HW, int C, int G, int relu,
    unsigned short* __restrict__ y) {
  extern __shared__ float4 gn_smem[];
  float* scale = reinterpret_cast<float*>(gn_smem);
  float* shift = scale + C;
  const long n = blockIdx.y;
  const int cpg = C / G;
  for (int c = threadIdx.x; c < C; c += kThreads) {
    const int g = c / cpg;
    const float sc = rstd[n * G + g] * u2f(gamma[c]);
    scale[c] = sc;
    shift[c] = u2f(beta[c]) - mean[n * G + g] * sc;
  }
  __syncthreads();
  // 32-bit granule index inside the sample (host checks H*W*C < 2^31):
  // the row/column split is one 32-bit division, not a 64-bit one
  const unsigned cg = C >> 3;
  const unsigned total = (unsigned)HW * cg;
  const long base = n * HW * C;
  for (unsigned q = blockIdx.x * kThreads + threadIdx.x; q < total;
       q += gridDim.x * kThreads) {
    const unsigned row = q / cg;
    const int c8 = (int)(q - row * cg) * 8;
    const long off = base + (long)row * C + c8;
    const u16x8 v = *reinterpret_cast<const u16x8*>(&x[off]);
    const float4 s0 = *reinterpret_cast<const float4*>(&scale[c8]);
    const float4 s1 = *reinterpret_cast<const float4*>(&scale[c8 + 4]);
    const float4 h0 = *reinterpret_cast<const float4*>(&shift[c8]);
    const float4 h1 = *reinterpret_cast<const float4*>(&shift[c8 + 4]);
    const float sj[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const float hj[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    u16x8 rv;
    if (res) rv = *reinterpret_cast<const u16x8*>(&res[off]);
    u16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = u2f(v[j]) * sj[j] + hj[j];
      if (res) f += u2f(rv[j]);
      if (relu) f = fmaxf(f, 0.f);
      out[j] = f2u(f);
    }
    *reinterpret_cast<u16x8*>(&y[off]) = out;
  }
}

// Backward partial pass: per-(n, chunk, channel) sum(dy), sum(dy*xhat)
// with the ReLU mask folded in. These rows are also the dgamma/dbeta
// partials.
__global__ __launch_bounds__(kThreads) void gn_bwd_part_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ yr, const float* __restrict__ mean,
    const float* __restrict__ rstd, int HW, int C, int G, int GL,
    int chunk_rows, float* __restrict__ pdb, float* __restrict__ pdg) {
  __shared__ float4 red4[kThreads * 2];
  float* red = reinterpret_cast<float*>(red4);
  const int t = threadIdx.x;
  const int gi = t & (GL - 1), rl = t / GL, RL = kThreads / GL;
  const int c8 = (blockIdx.x * GL + gi) * 8;
  const bool ok = c8 < C;
  const long n = blockIdx.z;
  const int cpg = C / G;
  const int r0 = blockIdx.y * chunk_rows;
  const int r1 = min(HW, r0 + chunk_rows);
  const long base = n * HW * C;
  float s1[8] = {}, s2[8] = {};
  if (ok) {
    float mj[8], rj[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int g = (c8 + j) / cpg;
      mj[j] = mean[n * G + g];
      rj[j] = rstd[n * G + g];
    }
#pragma unroll 4
    for (int m = r0 + rl; m < r1; m += RL) {
      const long off = base + (long)m * C + c8;
      const u16x8 xv = *reinterpret_cast<const u16x8*>(&x[off]);
      u16x8 gv = *reinterpret_cast<const u16x8*>(&dy[off]);
      if (yr) {
        const u16x8 yv = *reinterpret_cast<const u16x8*>(&yr[off]);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!(u2f(yv[j]) > 0.f)) gv[j] = 0;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = u2f(gv[j]);
        s1[j] += g;
        s2[j] += g * ((u2f(xv[j]) - mj[j]) * rj[j]);
      }
    }
  }
  colsum8(s1, GL, red);
  colsum8(s2, GL, red);
  if (t < GL && ok) {
    const long o = (n * gridDim.y + blockIdx.y) * C + c8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pdb[o + j] = s1[j];
      pdg[o + j] = s2[j];
    }
  }
}

// One wave per (n, g): A = sum(gamma*dy)/m, B = sum(gamma*dy*xhat)/m
// from the channel partials, in gn_stats_final_kernel's fixed order
// (lane-strided over the chunk-major entries, then an xor butterfly).
__global__ __launch_bounds__(kThreads) void gn_bwd_final_kernel(
    const float* __restrict__ pdb, const float* __restrict__ pdg,
    const unsigned short* __restrict__ gamma, long NG, int chunks, int C,
    int G, double cnt, float* __restrict__ gA, float* __restrict__ gB) {
  const long ng = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (ng >= NG) return;
  const int lane = threadIdx.x & 63;
  const int cpg = C / G;
  const long n = ng / G;
  const int g = (int)(ng % G);
  double A = 0.0, B = 0.0;
  for (int e = lane; e < chunks * cpg; e += 64) {
    const int c = g * cpg + e % cpg;
    const long idx = (n * chunks + e / cpg) * C + c;
    const double gc = (double)u2f(gamma[c]);
    A += gc * (double)pdb[idx];
    B += gc * (double)pdg[idx];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    A += __shfl_xor(A, off, 64);
    B += __shfl_xor(B, off, 64);
  }
  if (lane == 0) {
    gA[ng] = (float)(A / cnt);
    gB[ng] = (float)(B / cnt);
  }
}

// dx = rstd*(gamma*dy - A - xhat*B) folded to a*dy + b*x + d per
// channel of the sample (constants in LDS).
__global__ __launch_bounds__(kThreads) void gn_bwd_dx_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ yr, const float* __restrict__ mean,
    const float* __restrict__ rstd, const unsigned short* __restrict__ gamma,
    const float* __restrict__ gA, const float* __restrict__ gB, int HW, int C,
    int G, unsigned short* __restrict__ dx) {
  extern __shared__ float4 gn_smem[];
  float* pa = reinterpret_cast<float*>(gn_smem);
  float* pb = pa + C;
  float* pd = pb + C;
  const long n = blockIdx.y;
  const int cpg = C / G;
  for (int c = threadIdx.x; c < C; c += kThreads) {
    const int g = c / cpg;
    const float r = rstd[n * G + g], m = mean[n * G + g];
    const float b = -r * r * gB[n * G + g];
    pa[c] = r * u2f(gamma[c]);
    pb[c] = b;
    pd[c] = -r * gA[n * G + g] - m * b;
  }
  __syncthreads();
  // 32-bit granule index inside the sample (host checks H*W*C < 2^31):
  // the row/column split is one 32-bit division, not a 64-bit one
  const unsigned cg = C >> 3;
  const unsigned total = (unsigned)HW * cg;
  const long base = n * HW * C;
  for (unsigned q = blockIdx.x * kThreads + threadIdx.x; q < total;
       q += gridDim.x * kThreads) {
    const unsigned row = q / cg;
    const int c8 = (int)(q - row * cg) * 8;
    const long off = base + (long)row * C + c8;
    const u16x8 xv = *reinterpret_cast<const u16x8*>(&x[off]);
    u16x8 gv = *reinterpret_cast<const u16x8*>(&dy[off]);
    if (yr) {
      const u16x8 yv = *reinterpret_cast<const u16x8*>(&yr[off]);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (!(u2f(yv[j]) > 0.f)) gv[j] = 0;
    }
    u16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      out[j] = f2u(pa[c8 + j] * u2f(gv[j]) + pb[c8 + j] * u2f(xv[j]) +
                   pd[c8 + j]);
    *reinterpret_cast<u16x8*>(&dx[off]) = out;
  }
}

// dgamma/dbeta: reduce [rows][C] fp32 partials (rows = N or N*chunks)
// in a fixed order — KL row-lanes stride the rows ascending, pairwise
// halving tree over the row-lanes. G4 float4 granules per block.
// Grid (column blocks, row segments): block y reduces rows
// [y*seg_rows, (y+1)*seg_rows). With one segment the result is final
// (bf16 dgamma/dbeta); with several, each writes an fp32 row of
// [segments][C] (odb/odg) and a second launch reduces those.
__global__ __launch_bounds__(kThreads) void gn_param_final_kernel(
    const float* __restrict__ pdb, const float* __restrict__ pdg, long rows,
    long seg_rows, int C, int G4, float* __restrict__ odb,
    float* __restrict__ odg, unsigned short* __restrict__ dgamma,
    unsigned short* __restrict__ dbeta) {
  const int gi = threadIdx.x % G4, kl = threadIdx.x / G4;
  const int KL = kThreads / G4;
  const int c4 = (blockIdx.x * G4 + gi) * 4;
  const long k0 = (long)blockIdx.y * seg_rows;
  const long k1 = k0 + seg_rows < rows ? k0 + seg_rows : rows;
  float sj[4] = {}, qj[4] = {};
  if (c4 < C)
    for (long k = k0 + kl; k < k1; k += KL) {
      const float4 a = *reinterpret_cast<const float4*>(&pdb[k * C + c4]);
      const float4 b = *reinterpret_cast<const float4*>(&pdg[k * C + c4]);
      sj[0] += a.x; sj[1] += a.y; sj[2] += a.z; sj[3] += a.w;
      qj[0] += b.x; qj[1] += b.y; qj[2] += b.z; qj[3] += b.w;
    }
  __shared__ float rs[kThreads][4], rq[kThreads][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rs[threadIdx.x][j] = sj[j];
    rq[threadIdx.x][j] = qj[j];
  }
  __syncthreads();
  for (int h = KL >> 1; h > 0; h >>= 1) {
    if (kl < h) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rs[kl * G4 + gi][j] += rs[(kl + h) * G4 + gi][j];
        rq[kl * G4 + gi][j] += rq[(kl + h) * G4 + gi][j];
      }
    }
    __syncthreads();
  }
  if (kl == 0 && c4 < C) {
    if (odb) {
      const long o = (long)blockIdx.y * C + c4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        odb[o + j] = rs[gi][j];
        odg[o + j] = rq[gi][j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dbeta[c4 + j] = f2u(rs[gi][j]);
        dgamma[c4 + j] = f2u(rq[gi][j]);
      }
    }
  }
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------

inline bool is_pow2(long v) { return v > 0 && (v & (v - 1)) == 0; }

inline bool slab_legal(long HW, long C) {
  const long cg = C / 8;
  return is_pow2(cg) && cg <= 256 && HW * C * 2 <= kSlabBytes;
}

void check_shape(long C, long groups) {
  TORCH_CHECK(groups > 0, "groupnorm: groups must be positive, got ", groups);
  TORCH_CHECK(C % 8 == 0, "groupnorm: GPU path needs C % 8 == 0 (16-byte "
              "channel granules), got C=", C);
  TORCH_CHECK(C % groups == 0, "groupnorm: C=", C,
              " is not divisible by groups=", groups);
  TORCH_CHECK(C <= 4096, "groupnorm: C=", C, " exceeds the supported 4096");
}

// The route is a function of (H, W, C, G) and the BFLC_GN_ROUTE knob
// only. N must never enter: per-sample bitwise invariance rests on it.
bool use_slab(long HW, long C) {
  const bool legal = slab_legal(HW, C);
  if (const char* e = std::getenv("BFLC_GN_ROUTE")) {
    if (std::strcmp(e, "split") == 0) return false;
    if (std::strcmp(e, "slab") == 0) return legal;
    TORCH_CHECK(e[0] == '\0', "BFLC_GN_ROUTE must be slab or split, got '",
                e, "'");
  }
  return legal;
}

struct SplitGeom {
  int GL, cblocks, chunk_rows, chunks, norm_blocks;
};

// chunk geometry from (HW, C) only
SplitGeom split_geom(long HW, long C) {
  SplitGeom s;
  const int cg = (int)(C / 8);
  s.GL = 1;
  while (s.GL * 2 <= std::min(cg, kThreads)) s.GL *= 2;
  s.cblocks = ceil_div(cg, s.GL);
  s.chunk_rows = (kThreads / s.GL) * kSplitGranulesPerLane;
  s.chunks = ceil_div(HW, s.chunk_rows);
  // chunks is a grid y dimension
  TORCH_CHECK(s.chunks <= 65535, "groupnorm: H*W=", HW, " needs ", s.chunks,
              " row chunks at C=", C, ", above the supported 65535");
  s.norm_blocks = (int)std::max<long>(
      1, std::min<long>(HW * cg / (kThreads * 2), 256));
  return s;
}

inline int slab_ni(long HW, long C) {
  const long RL = kThreads / (C / 8);
  const long need = (HW + RL - 1) / RL;
  int ni = 1;
  while (ni < need) ni *= 2;
  return ni;
}

inline const unsigned short* u16(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}
inline unsigned short* u16w(torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

void check_bf16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, "groupnorm: ", name,
              " must be bf16");
}

void launch_param_final(const torch::Tensor& pdb, const torch::Tensor& pdg,
                        long rows, int C, torch::Tensor& dgamma,
                        torch::Tensor& dbeta) {
  int G4 = 1;  // <= 4: narrow blocks keep many row-lanes per channel
  while (G4 * 2 <= std::min(C / 4, 4)) G4 *= 2;
  const int cblocks = ceil_div(C / 4, G4);
  const float* p1 = pdb.data_ptr<float>();
  const float* p2 = pdg.data_ptr<float>();
  torch::Tensor sdb, sdg;  // keep the segment sums alive past the launch
  // many rows on few column blocks leave most of the chip idle (16
  // blocks walking 3136 rows at ResNet-50 stage 1): reduce 128-row
  // segments in parallel first. The segment size is a constant, so the
  // summation order stays a function of the shape alone.
  constexpr long kSegRows = 128;
  if (rows > 8 * kSegRows) {
    const int segs = ceil_div(rows, kSegRows);
    TORCH_CHECK(segs <= 65535, "groupnorm: too many partial rows");
    sdb = torch::empty({segs, C}, pdb.options());
    sdg = torch::empty({segs, C}, pdb.options());
    hipLaunchKernelGGL(gn_param_final_kernel, dim3(cblocks, segs),
                       dim3(kThreads), 0, cur_stream(), p1, p2, rows,
                       kSegRows, C, G4, sdb.data_ptr<float>(),
                       sdg.data_ptr<float>(), (unsigned short*)nullptr,
                       (unsigned short*)nullptr);
    p1 = sdb.data_ptr<float>();
    p2 = sdg.data_ptr<float>();
    rows = segs;
  }
  hipLaunchKernelGGL(gn_param_final_kernel, dim3(cblocks), dim3(kThreads), 0,
                     cur_stream(), p1, p2, rows, rows, C, G4,
                     (float*)nullptr, (float*)nullptr, u16w(dgamma),
                     u16w(dbeta));
}

}  // namespace

std::string groupnorm_route(long H, long W, long C, long groups) {
  check_shape(C, groups);
  return use_slab(H * W, C) ? "slab" : "split";
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> groupnorm_fwd(
    torch::Tensor x, torch::Tensor gamma, torch::Tensor beta, long groups,
    double eps, bool relu, c10::optional<torch::Tensor> residual) {
  CHECK_GPU(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 4, "groupnorm: x must be NHWC [N,H,W,C]");
  check_bf16(x, "x"); check_bf16(gamma, "gamma"); check_bf16(beta, "beta");
  const long N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  check_shape(C, groups);
  TORCH_CHECK(gamma.numel() == C && beta.numel() == C,
              "groupnorm: gamma/beta must have C elements");
  TORCH_CHECK(HW * C < (1L << 31), "groupnorm: H*W*C must be below 2^31");
  const unsigned short* resp = nullptr;
  if (residual.has_value()) {
    CHECK_GPU(*residual); CHECK_CONTIG(*residual);
    check_bf16(*residual, "residual");
    TORCH_CHECK(residual->sizes() == x.sizes(),
                "groupnorm: residual shape must match x");
    resp = u16(*residual);
  }
  const int G = (int)groups;
  auto gc = gamma.contiguous();
  auto bc = beta.contiguous();
  auto fopts = x.options().dtype(at::kFloat);
  auto y = torch::empty_like(x);
  auto mean = torch::empty({N, groups}, fopts);
  auto rstd = torch::empty({N, groups}, fopts);
  if (N == 0 || HW == 0) return {y, mean, rstd};

  if (use_slab(HW, C)) {
    const size_t lds = (kThreads * 8 + C + 2 * G) * sizeof(float);
#define GN_SLAB_FWD(NI)                                                     \
  hipLaunchKernelGGL(gn_slab_fwd_kernel<NI>, dim3((unsigned)N),             \
                     dim3(kThreads), lds, cur_stream(), u16(x), u16(gc),    \
                     u16(bc), resp, (int)HW, (int)C, G, (float)eps,         \
                     relu ? 1 : 0, u16w(y), mean.data_ptr<float>(),         \
                     rstd.data_ptr<float>())
    switch (slab_ni(HW, C)) {
      case 1: GN_SLAB_FWD(1); break;
      case 2: GN_SLAB_FWD(2); break;
      case 4: GN_SLAB_FWD(4); break;
      case 8: GN_SLAB_FWD(8); break;
      case 16: GN_SLAB_FWD(16); break;
      default: TORCH_CHECK(false, "groupnorm: slab does not fit");
    }
#undef GN_SLAB_FWD
  } else {
    TORCH_CHECK(N <= 65535, "groupnorm: split route needs N <= 65535");
    const SplitGeom s = split_geom(HW, C);
    auto psum = torch::empty({N * s.chunks, C}, fopts);
    auto psq = torch::empty({N * s.chunks, C}, fopts);
    hipLaunchKernelGGL(gn_part_kernel, dim3(s.cblocks, s.chunks, (unsigned)N),
                       dim3(kThreads), 0, cur_stream(), u16(x), (int)HW,
                       (int)C, s.GL, s.chunk_rows, psum.data_ptr<float>(),
                       psq.data_ptr<float>());
    const long NG = N * G;
    hipLaunchKernelGGL(gn_stats_final_kernel,
                       dim3(ceil_div(NG, kThreads / 64)), dim3(kThreads), 0,
                       cur_stream(), psum.data_ptr<float>(),
                       psq.data_ptr<float>(), NG, s.chunks, (int)C, G,
                       (double)HW * (double)(C / G), eps,
                       mean.data_ptr<float>(), rstd.data_ptr<float>());
    hipLaunchKernelGGL(gn_norm_kernel, dim3(s.norm_blocks, (unsigned)N),
                       dim3(kThreads), 2 * C * sizeof(float), cur_stream(),
                       u16(x), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       u16(gc), u16(bc), resp, (int)HW, (int)C, G,
                       relu ? 1 : 0, u16w(y));
  }
  HIP_CHECK(hipGetLastError());
  return {y, mean, rstd};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> groupnorm_bwd(
    torch::Tensor x, torch::Tensor dy, torch::Tensor mean, torch::Tensor rstd,
    torch::Tensor gamma, long groups, c10::optional<torch::Tensor> y_relu) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_GPU(dy); CHECK_CONTIG(dy);
  CHECK_GPU(mean); CHECK_GPU(rstd); CHECK_CONTIG(mean); CHECK_CONTIG(rstd);
  TORCH_CHECK(x.dim() == 4, "groupnorm: x must be NHWC [N,H,W,C]");
  check_bf16(x, "x"); check_bf16(dy, "dy"); check_bf16(gamma, "gamma");
  TORCH_CHECK(dy.sizes() == x.sizes(), "groupnorm: dy shape must match x");
  const long N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  check_shape(C, groups);
  TORCH_CHECK(gamma.numel() == C, "groupnorm: gamma must have C elements");
  TORCH_CHECK(mean.scalar_type() == at::kFloat &&
                  rstd.scalar_type() == at::kFloat &&
                  mean.numel() == N * groups && rstd.numel() == N * groups,
              "groupnorm: mean/rstd must be fp32 [N, groups]");
  TORCH_CHECK(HW * C < (1L << 31), "groupnorm: H*W*C must be below 2^31");
  const unsigned short* yr = nullptr;
  if (y_relu.has_value()) {
    CHECK_GPU(*y_relu); CHECK_CONTIG(*y_relu);
    check_bf16(*y_relu, "y");
    TORCH_CHECK(y_relu->sizes() == x.sizes(),
                "groupnorm: y shape must match x");
    yr = u16(*y_relu);
  }
  const int G = (int)groups;
  auto gc = gamma.contiguous();
  auto fopts = x.options().dtype(at::kFloat);
  auto dx = torch::empty_like(x);
  auto dgamma = torch::empty({C}, x.options());
  auto dbeta = torch::empty({C}, x.options());
  if (N == 0 || HW == 0) {
    dgamma.zero_(); dbeta.zero_();
    return {dx, dgamma, dbeta};
  }

  if (use_slab(HW, C)) {
    auto pdb = torch::empty({N, C}, fopts);
    auto pdg = torch::empty({N, C}, fopts);
    const size_t lds = (kThreads * 8 + 2 * C + 4 * G) * sizeof(float);
#define GN_SLAB_BWD(NI)                                                     \
  hipLaunchKernelGGL(gn_slab_bwd_kernel<NI>, dim3((unsigned)N),             \
                     dim3(kThreads), lds, cur_stream(), u16(x), u16(dy), yr, \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),        \
                     u16(gc), (int)HW, (int)C, G, u16w(dx),                 \
                     pdb.data_ptr<float>(), pdg.data_ptr<float>())
    switch (slab_ni(HW, C)) {
      case 1: GN_SLAB_BWD(1); break;
      case 2: GN_SLAB_BWD(2); break;
      case 4: GN_SLAB_BWD(4); break;
      case 8: GN_SLAB_BWD(8); break;
      case 16: GN_SLAB_BWD(16); break;
      default: TORCH_CHECK(false, "groupnorm: slab does not fit");
    }
#undef GN_SLAB_BWD
    launch_param_final(pdb, pdg, N, (int)C, dgamma, dbeta);
  } else {
    TORCH_CHECK(N <= 65535, "groupnorm: split route needs N <= 65535");
    const SplitGeom s = split_geom(HW, C);
    auto pdb = torch::empty({N * s.chunks, C}, fopts);
    auto pdg = torch::empty({N * s.chunks, C}, fopts);
    auto gA = torch::empty({N, groups}, fopts);
    auto gB = torch::empty({N, groups}, fopts);
    hipLaunchKernelGGL(gn_bwd_part_kernel,
                       dim3(s.cblocks, s.chunks, (unsigned)N), dim3(kThreads),
                       0, cur_stream(), u16(x), u16(dy), yr,
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       (int)HW, (int)C, G, s.GL, s.chunk_rows,
                       pdb.data_ptr<float>(), pdg.data_ptr<float>());
    const long NG = N * G;
    hipLaunchKernelGGL(gn_bwd_final_kernel,
                       dim3(ceil_div(NG, kThreads / 64)), dim3(kThreads), 0,
                       cur_stream(), pdb.data_ptr<float>(),
                       pdg.data_ptr<float>(), u16(gc), NG, s.chunks, (int)C,
                       G, (double)HW * (double)(C / G), gA.data_ptr<float>(),
                       gB.data_ptr<float>());
    hipLaunchKernelGGL(gn_bwd_dx_kernel, dim3(s.norm_blocks, (unsigned)N),
                       dim3(kThreads), 3 * C * sizeof(float), cur_stream(),
                       u16(x), u16(dy), yr, mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), u16(gc), gA.data_ptr<float>(),
                       gB.data_ptr<float>(), (int)HW, (int)C, G, u16w(dx));
    launch_param_final(pdb, pdg, N * s.chunks, (int)C, dgamma, dbeta);
  }
  HIP_CHECK(hipGetLastError());
  return {dx, dgamma, dbeta};
}

}  // namespace bflc
