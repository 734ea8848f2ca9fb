// Robust aggregation over the [K, P] fp32 delta stack (gfx950):
//
//   order_stat_mean  per-coordinate sort of the K values, trim t at each
//                    end, ascending fp32 sum / (K - 2t): trimmed mean
//                    (t = agg_trim) and median (t = (K-1)/2)
//   delta_gram       G = D * D^T on the f32-input MFMA, two stages with a
//                    fixed reduction order: multi-Krum's distances
//   masked_wmean     fedavg_kernel's fmaf chain with per-row addressing
//                    (correct for every P) that skips zero-weight rows
//
// Row k starts at float offset k * P, which is 16-byte aligned only when
// P % 4 == 0 (and the base is). order_stat_mean and masked_wmean take
// float4 accesses only then and a coalesced dword mapping otherwise;
// delta_gram stages coalesced dword row segments through LDS at every
// alignment. No atomics, no host sync, K <= 32.

#include "common.h"

namespace bflc {

namespace {

constexpr int kBlock = 256;
constexpr int kMaxK = 32;

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// ---------------------------------------------------------------------
// coordinate mapping shared by order_stat_mean and masked_wmean: a block
// covers 4 * kBlock consecutive coordinates, a thread four of them.
//   VEC   coordinates base + 4t + q   (one float4 per row)
//   !VEC  coordinates base + t + 256q (four coalesced dwords per row)
template <bool VEC>
__device__ __forceinline__ long coord_of(long base, int t, int q) {
  return VEC ? base + 4 * (long)t + q : base + t + (long)kBlock * q;
}

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ row,
                                      long base, int t, long P,
                                      float (&v)[4]) {
  if (VEC) {  // P % 4 == 0: a float4 is inside the row or wholly outside
    long c = base + 4 * (long)t;
    if (c < P) {
      float4 x = *reinterpret_cast<const float4*>(row + c);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      long c = base + t + (long)kBlock * q;
      v[q] = c < P ? row[c] : 0.f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ out, long base,
                                       int t, long P, const float (&v)[4]) {
  if (VEC) {
    long c = base + 4 * (long)t;
    if (c < P)
      *reinterpret_cast<float4*>(out + c) =
          make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      long c = base + t + (long)kBlock * q;
      if (c < P) out[c] = v[q];
    }
  }
}

// ---------------------------------------------------------------------
// order-preserving integer keys: k(a) < k(b) <=> a < b for non-NaN
// floats (-0 below +0), every NaN -> the top key. fminf/fmaxf would drop
// a NaN and duplicate its partner; unsigned min/max cannot.
constexpr unsigned kTopKey = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned key_of(float f) {
  unsigned u = __float_as_uint(f);
  unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (f != f) ? kTopKey : k;
}

__device__ __forceinline__ float value_of(unsigned k) {
  // the top key is not the image of any non-NaN float (+inf maps to
  // 0xFF800000), so it decodes to the canonical NaN
  unsigned u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return k == kTopKey ? __uint_as_float(0x7FC00000u) : __uint_as_float(u);
}

// Bitonic network on N = 4 | 8 | 16 | 32 keys, every compare-exchange
// ascending, all indices compile-time after unrolling (registers only).
template <int N>
__device__ __forceinline__ void sort_network(unsigned (&a)[N][4]) {
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      int l = i ^ (k - 1);
      if (l > i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          unsigned lo = min(a[i][q], a[l][q]), hi = max(a[i][q], a[l][q]);
          a[i][q] = lo; a[l][q] = hi;
        }
      }
    }
#pragma unroll
    for (int j = k >> 2; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        int l = i ^ j;
        if (l > i) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            unsigned lo = min(a[i][q], a[l][q]), hi = max(a[i][q], a[l][q]);
            a[i][q] = lo; a[l][q] = hi;
          }
        }
      }
    }
  }
}

template <int N, bool VEC>
__global__ __launch_bounds__(kBlock) void order_stat_mean_kernel(
    const float* __restrict__ d, int K, long P, int t,
    float* __restrict__ out) {
  long base = (long)blockIdx.x * (4 * kBlock);
  int tid = threadIdx.x;
  unsigned a[N][4];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i < K) {  // uniform; rows >= K are never read
      float v[4];
      load4<VEC>(d + (long)i * P, base, tid, P, v);
#pragma unroll
      for (int q = 0; q < 4; ++q) a[i][q] = key_of(v[q]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[i][q] = kTopKey;
    }
  }
  sort_network<N>(a);
  // ascending fp32 sum of sorted positions t .. K-1-t, then one
  // correctly rounded division
  int hi = K - t;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i >= t && i < hi) {  // uniform
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += value_of(a[i][q]);
    }
  }
  float cnt = (float)(K - 2 * t);
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = s[q] / cnt;
  store4<VEC>(out, base, tid, P, s);
}

// ---------------------------------------------------------------------
// sum_k w[k] * d[k][i] by fmaf in ascending k, times 1 / wsum: the
// chain of fedavg_kernel. wsum is read from device memory (no host
// sync); rows with w[k] == 0 are skipped and not read.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void masked_wmean_kernel(
    const float* __restrict__ d, const float* __restrict__ w,
    const float* __restrict__ wsum, int K, long P,
    float* __restrict__ out) {
  long base = (long)blockIdx.x * (4 * kBlock);
  int tid = threadIdx.x;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; ++k) {  // fixed order — do not reorder
    float wk = w[k];
    if (wk == 0.f) continue;  // uniform
    float v[4];
    load4<VEC>(d + (long)k * P, base, tid, P, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = fmaf(wk, v[q], acc[q]);
  }
  float inv = 1.f / wsum[0];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] *= inv;
  store4<VEC>(out, base, tid, P, acc);
}

// ---------------------------------------------------------------------
// delta_gram stage 1. R = 32: v_mfma_f32_32x32x2_f32 (lane l feeds row
// l & 31 at k = l >> 5); R = 16: v_mfma_f32_16x16x4_f32 (row l & 15 at
// k = l >> 4). B = A^T, so one register is both operands.
//
// A block owns coordinates [blk * chunk, (blk + 1) * chunk) and walks
// them in tiles of kTile. Each thread prefetches the next tile's column
// (coordinate tile + tid of every row < K: coalesced dwords at any row
// alignment) into registers while the MFMAs run on the tile in LDS.
// Rows >= K and coordinates >= P are zeros in LDS and never loaded. Wave
// w takes columns [64w, 64w + 64) of each tile; at the end the four
// waves' accumulators are added in wave order and the K x K corner is
// written as this block's partial.
constexpr int kTile = 256;

template <int R>
struct GramCfg {
  static constexpr int kPerMfma = 64 / R;       // coordinates per MFMA
  static constexpr int kStride = kTile + kPerMfma;  // bank-conflict-free:
  // lane (row, h) reads bank (row * kPerMfma + h) % 64, all 64 distinct
  static constexpr int kAcc = R * R / 64;
};

template <int R>
__global__ __launch_bounds__(kBlock) void gram_partial_kernel(
    const float* __restrict__ d, int K, long P, long chunk,
    float* __restrict__ partial) {
  using Cfg = GramCfg<R>;
  using acc_t = typename std::conditional<R == 32, f32x16, f32x4>::type;
  constexpr int kStride = Cfg::kStride;
  constexpr int kLdsFloats =
      R * kStride > 4 * R * R ? R * kStride : 4 * R * R;
  __shared__ float lds[kLdsFloats];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long c1 = c0 + chunk < P ? c0 + chunk : P;

  float pre[R];
  auto prefetch = [&](long tile) {
    long c = tile + tid;
    bool in = c < c1;
#pragma unroll
    for (int i = 0; i < R; ++i)
      pre[i] = (i < K && in) ? d[(long)i * P + c] : 0.f;
  };

  acc_t acc;
#pragma unroll
  for (int i = 0; i < Cfg::kAcc; ++i) acc[i] = 0.f;

  const int row = lane & (R - 1), h = lane / R;
  const float* my = lds + row * kStride + wave * 64 + h;

  prefetch(c0);
  for (long tile = c0; tile < c1; tile += kTile) {
    __syncthreads();  // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < R; ++i) lds[i * kStride + tid] = pre[i];
    __syncthreads();
    if (tile + kTile < c1) prefetch(tile + kTile);
#pragma unroll
    for (int s = 0; s < 64 / Cfg::kPerMfma; ++s) {
      float x = my[s * Cfg::kPerMfma];
      if constexpr (R == 32)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x, x, acc, 0, 0, 0);
      else
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x, x, acc, 0, 0, 0);
    }
  }

  // fixed-order reduction of the four waves' tiles through LDS
  __syncthreads();
  float* red = lds + wave * (R * R);
#pragma unroll
  for (int i = 0; i < Cfg::kAcc; ++i) {
    int col = lane & (R - 1);
    int r = R == 32 ? (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
                    : (lane >> 4) * 4 + i;
    red[r * R + col] = acc[i];
  }
  __syncthreads();
  float* dst = partial + (long)blockIdx.x * K * K;
  for (int e = tid; e < K * K; e += kBlock) {
    int a = e / K, b = e - a * K;
    float s = lds[a * R + b];
#pragma unroll
    for (int w = 1; w < 4; ++w) s += lds[w * (R * R) + a * R + b];
    dst[e] = s;
  }
}

// stage 2: one thread per G element adds the partials in ascending
// block order.
__global__ void gram_final_kernel(const float* __restrict__ partial, int nb,
                                  int KK, float* __restrict__ G) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= KK) return;
  float s = partial[e];
  for (int b = 1; b < nb; ++b) s += partial[(long)b * KK + e];
  G[e] = s;
}

// geometry from (K, P) alone: at most kGramBlocks blocks of whole tiles
constexpr int kGramBlocks = 512;

inline void gram_geom(long P, long* chunk, int* nb) {
  long tiles = (P + kTile - 1) / kTile;
  long per = (tiles + kGramBlocks - 1) / kGramBlocks;
  *chunk = per * kTile;
  *nb = (int)((P + *chunk - 1) / *chunk);
}

void check_stack(const torch::Tensor& d) {
  CHECK_GPU(d); CHECK_CONTIG(d);
  TORCH_CHECK(d.dim() == 2, "deltas must be [K, P]");
  TORCH_CHECK(d.scalar_type() == at::kFloat, "deltas must be fp32");
  TORCH_CHECK(d.size(0) >= 1 && d.size(0) <= kMaxK,
              "K must be in [1, 32], got ", d.size(0));
  TORCH_CHECK(d.size(1) >= 1, "P must be >= 1");
}

inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

template <int N>
void launch_osm(bool vec, int grid, const float* d, int K, long P, int t,
                float* out) {
  if (vec)
    hipLaunchKernelGGL((order_stat_mean_kernel<N, true>), dim3(grid),
                       dim3(kBlock), 0, cur_stream(), d, K, P, t, out);
  else
    hipLaunchKernelGGL((order_stat_mean_kernel<N, false>), dim3(grid),
                       dim3(kBlock), 0, cur_stream(), d, K, P, t, out);
}

}  // namespace

torch::Tensor order_stat_mean(torch::Tensor deltas, long t) {
  check_stack(deltas);
  int K = (int)deltas.size(0);
  long P = deltas.size(1);
  TORCH_CHECK(t >= 0 && 2 * t < K, "order_stat_mean: need 0 <= 2t < K, got "
              "t=", t, " K=", K);
  auto out = torch::empty({P}, deltas.options());
  const float* d = deltas.data_ptr<float>();
  float* o = out.data_ptr<float>();
  bool vec = P % 4 == 0 && aligned16(d) && aligned16(o);
  int grid = ceil_div(P, 4 * kBlock);
  if (K <= 4) launch_osm<4>(vec, grid, d, K, P, (int)t, o);
  else if (K <= 8) launch_osm<8>(vec, grid, d, K, P, (int)t, o);
  else if (K <= 16) launch_osm<16>(vec, grid, d, K, P, (int)t, o);
  else launch_osm<32>(vec, grid, d, K, P, (int)t, o);
  HIP_CHECK(hipGetLastError());
  return out;
}

torch::Tensor masked_wmean(torch::Tensor deltas, torch::Tensor w) {
  check_stack(deltas);
  CHECK_GPU(w); CHECK_CONTIG(w);
  TORCH_CHECK(w.dim() == 1 && w.size(0) == deltas.size(0),
              "w must be [K]");
  TORCH_CHECK(w.scalar_type() == at::kFloat, "w must be fp32");
  int K = (int)deltas.size(0);
  long P = deltas.size(1);
  auto wsum = w.sum();  // as weighted_fedavg, but left on the device
  auto out = torch::empty({P}, deltas.options());
  const float* d = deltas.data_ptr<float>();
  float* o = out.data_ptr<float>();
  bool vec = P % 4 == 0 && aligned16(d) && aligned16(o);
  int grid = ceil_div(P, 4 * kBlock);
  if (vec)
    hipLaunchKernelGGL(masked_wmean_kernel<true>, dim3(grid), dim3(kBlock),
                       0, cur_stream(), d, w.data_ptr<float>(),
                       wsum.data_ptr<float>(), K, P, o);
  else
    hipLaunchKernelGGL(masked_wmean_kernel<false>, dim3(grid), dim3(kBlock),
                       0, cur_stream(), d, w.data_ptr<float>(),
                       wsum.data_ptr<float>(), K, P, o);
  HIP_CHECK(hipGetLastError());
  return out;
}

torch::Tensor delta_gram(torch::Tensor deltas) {
  check_stack(deltas);
  int K = (int)deltas.size(0);
  long P = deltas.size(1);
  long chunk; int nb;
  gram_geom(P, &chunk, &nb);
  auto partial = torch::empty({(long)nb, (long)K * K}, deltas.options());
  auto G = torch::empty({(long)K, (long)K}, deltas.options());
  const float* d = deltas.data_ptr<float>();
  if (K <= 16)
    hipLaunchKernelGGL(gram_partial_kernel<16>, dim3(nb), dim3(kBlock), 0,
                       cur_stream(), d, K, P, chunk,
                       partial.data_ptr<float>());
  else
    hipLaunchKernelGGL(gram_partial_kernel<32>, dim3(nb), dim3(kBlock), 0,
                       cur_stream(), d, K, P, chunk,
                       partial.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(gram_final_kernel, dim3(ceil_div(K * K, kBlock)),
                     dim3(kBlock), 0, cur_stream(),
                     partial.data_ptr<float>(), nb, K * K,
                     G.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  return G;
}

std::tuple<long, long> delta_gram_geom_query(long P) {
  TORCH_CHECK(P >= 1, "P must be >= 1");
  long chunk; int nb;
  gram_geom(P, &chunk, &nb);
  return {(long)nb, chunk};
}

}  // namespace bflc
