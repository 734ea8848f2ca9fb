// MFMA bf16 GEMM family for gfx950 (CDNA4) + linear fwd/bwd entries.
//
// Owns the reference matmul ops (main.py:120 forward, 127-130 backward
// via compute_gradients) for every Dense/FC layer, and is the GEMM core
// behind the NHWC convolutions (conv2d.hip), including their
// implicit-GEMM forms.
//
// Three kernel tiers, all __builtin_amdgcn_mfma_f32_16x16x32_bf16 with
// fp32 accumulation, picked per shape by a cost model:
//   1. gemm8p_kernel — the 8-phase global_load_lds schedule
//      (cdna_hip_programming.md §5 "8-phase template"): counted vmcnt
//      keeps prefetched half-tiles in flight across raw barriers, one
//      barrier per phase, setprio around each 16-MFMA cluster, and a
//      conflict-free XOR source/read swizzle (bits 8,10 -> 5,6).
//      980 TF @4096^3 / 1114 @8192^3 on random data. Fully aligned
//      shapes (M,N % 256, K % 64) only — glds cannot zero-fill edges.
//   2. gemm256_kernel<BM, BN, CMODE> — double-buffered register-staged
//      BMxBN tile family (guide T14: write tile t+1 after the barrier,
//      re-issue t+2 loads immediately, one barrier per K-step), 8
//      waves, M/K edges zero-guarded. CMODE 1/2 fuse the NHWC conv
//      forward / data-grad gathers into the A staging.
//   3. gemm_kernel<..., CMODE> — synchronous small-tile kernel for
//      skinny shapes; CMODE 1 = implicit conv fwd (narrow Kout),
//      CMODE 3 = implicit wgrad (x gathered into the B staging).
// Shared machinery:
//   - operands not in the vector-staging layout (A [M][K] / B [N][K])
//     are pre-transposed by the LDS-tiled transpose (scatter staging
//     measured 3.4x slower than all-vector at 4096^3);
//   - split-K with a FIXED-ORDER fp32 reduce: K slices land in a
//     partial buffer [S, M, N], a deterministic 8-lane-tree kernel sums
//     ascending s — bitwise identical on every rank, no atomics; the
//     slice count comes from a GEMM-fill vs reduce-traffic cost model;
//   - fused bias/ReLU epilogues; 1-D tile grid with an XCD-bijective
//     swizzle (guide T1); hierarchical fixed-order colsum for bias
//     gradients.
//
// Fragment layout (gfx950 mfma_f32_16x16x32_bf16, cdna4_isa.md §10),
// verified on MI355X hardware by tests/test_ops_gpu.py (asymmetric
// operands, transpose-detecting):
//   A: lane l holds A[row = l&15][k = (l>>4)*8 + j], j = 0..7
//   B: lane l holds B[k = (l>>4)*8 + j][col = l&15]
//   D: lane l holds D[row = (l>>4)*4 + r][col = l&15], r = 0..3

#include "common.h"
#include "gemm_api.h"
#include "thin_pool_chain.h"

namespace bflc {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;
typedef __attribute__((ext_vector_type(2))) unsigned short u16x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int BK = 32;      // K per MFMA instruction / per LDS stage
constexpr int BKP = BK + 8; // padded row length (16 B) vs bank conflicts

// blockIdx.x = tile (XCD-swizzled), blockIdx.y = K slice (split-K).
// If Cpart != nullptr: write fp32 partials at Cpart[slice*M*N + ...] and
// skip bias/relu (applied by the reduce kernel). kslice = K per slice.
template <int BM, int BN, int WR, int WC, bool TA, bool TB,
          int CMODE = 0>
__launch_bounds__(WR * WC * 64)
__global__ void gemm_kernel(const bf16* __restrict__ A,
                            const bf16* __restrict__ B,
                            bf16* __restrict__ C, float* __restrict__ Cpart,
                            const bf16* __restrict__ bias, long M, long N,
                            long K, long kslice, int relu, int store_mode,
                            long ohw, int vecA, int vecB, ConvShape csh,
                            float* __restrict__ bn_psum = nullptr,
                            float* __restrict__ bn_psq = nullptr) {
  constexpr int THREADS = WR * WC * 64;
  constexpr int FM = BM / WR / 16;
  constexpr int FN = BN / WC / 16;

  __shared__ bf16 As[BM][BKP];
  __shared__ bf16 Bs[BN][BKP];
  // Row-dependent XOR swizzle (multiple of 8, so 16-B groups and the
  // b128 frag reads stay aligned): the b16 scatter stagings (TA / !TB /
  // implicit wgrad) write 8-row-strided columns whose dword stride is
  // 32 mod 64 banks — an 8-way conflict no 16-B-aligned padding can
  // fix; XORing k by (row & 24) spreads them to 4 banks (2x), measured
  // on the ResNet-20 implicit-wgrad kernel.
  auto swz = [](int row, int k) { return k ^ (row & 24); };

  const int ntn = (int)((N + BN - 1) / BN);
  const int ntm = (int)((M + BM - 1) / BM);
  const int nwg = ntm * ntn;
  int bid = blockIdx.x;
  {  // XCD-bijective remap (guide T1)
    const int nxcd = 8;
    const int q = nwg / nxcd, r = nwg % nxcd;
    const int xcd = bid % nxcd, idx = bid / nxcd;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const long tile_m = (long)(bid / ntn) * BM;
  const long tile_n = (long)(bid % ntn) * BN;

  const long k_begin = (long)blockIdx.y * kslice;
  const long k_end = min(K, k_begin + kslice);

  const int tid = threadIdx.x;
  const int wave = tid / 64, lane = tid % 64;
  const int wm0 = (wave / WC) * (BM / WR);
  const int wn0 = (wave % WC) * (BN / WC);
  const int l15 = lane & 15, l4 = lane >> 4;

  f32x4_t acc[FM][FN] = {};

  // Implicit-gather m-side decode hoisted out of the K loop: each
  // staging slot's output row gm is FIXED across k-steps, so its
  // (n, oh/ow or ih/iw) divides and the row base/offsets are computed
  // once here instead of every k-step (they were ~half the staging
  // instruction count on the ResNet-20 implicit kernels).
  constexpr int AGI =
      (CMODE == 1 || CMODE == 2)
          ? ((BM * BK / 8) + THREADS - 1) / THREADS : 1;
  long cv_nbase[AGI];
  int cv_i0[AGI], cv_j0[AGI];
  bool cv_mok[AGI];
  // k-side decode kept as incremental per-slot state: gk advances by
  // BK each step, so (c8, r, s) update with adds and wraps — no
  // divides left anywhere in the staging loop.
  int st_c8[AGI], st_rr[AGI], st_ss[AGI];
  if (CMODE == 1 || CMODE == 2) {
    constexpr int GROUPS = (BM * BK) / 8;
#pragma unroll
    for (int i = 0; i < AGI; ++i) {
      const int g = tid + i * THREADS;
      const int m = g / (BK / 8);
      const int k8 = (g % (BK / 8)) * 8;
      const long gm = tile_m + m;
      cv_mok[i] = g < GROUPS && gm < M;
      const long gmc = cv_mok[i] ? gm : 0;
      if (CMODE == 1) {
        const int ow = (int)(gmc % csh.OW);
        const int oh = (int)((gmc / csh.OW) % csh.OH);
        const int nn = (int)(gmc / ((long)csh.OW * csh.OH));
        cv_i0[i] = oh * csh.stride - csh.pad;  // ih0
        cv_j0[i] = ow * csh.stride - csh.pad;  // iw0
        cv_nbase[i] = (long)nn * csh.H;
      } else {
        const int iw = (int)(gmc % csh.W);
        const int ih = (int)((gmc / csh.W) % csh.H);
        const int nn = (int)(gmc / ((long)csh.W * csh.H));
        cv_i0[i] = ih + csh.pad;  // oh_num0
        cv_j0[i] = iw + csh.pad;  // ow_num0
        cv_nbase[i] = (long)nn * csh.OH;
      }
      const int inner = CMODE == 1 ? csh.C : csh.Kout;
      const long gk0 = k_begin + k8;
      const int rs = (int)(gk0 / inner);
      st_c8[i] = (int)(gk0 - (long)rs * inner);
      st_rr[i] = rs / csh.S;
      st_ss[i] = rs - st_rr[i] * csh.S;
    }
  }

  // CMODE 3/4: n'-side (r, s, c8) decode per staging slot, k-invariant;
  // the m-side (n, oh, ow) decode advances by BK each k-step, so it is
  // carried incrementally too — no divides in the staging loop.
  // CMODE 4 = the k-pair experiment (BFLC_WGRAD_KPAIR): each slot owns
  // TWO adjacent k's of one n-granule so the LDS writes are b32 —
  // half the write instructions at the same (4-way) conflict degree.
  constexpr int BGI =
      CMODE == 3 ? ((BN * BK / 8) + THREADS - 1) / THREADS
      : (CMODE == 4 ? ((BN * BK / 16) + THREADS - 1) / THREADS : 1);
  int cv3_rr[BGI], cv3_ss[BGI], cv3_c8[BGI];
  int st3_ow[BGI], st3_oh[BGI];
  long st3_nb[BGI];
  if (CMODE == 3 || CMODE == 4) {
#pragma unroll
    for (int i = 0; i < BGI; ++i) {
      const int g = tid + i * THREADS;
      const int n8 = (g % (BN / 8)) * 8;
      const long gn = tile_n + n8;
      const long gnc = gn + 8 <= N ? gn : 0;
      const int rs = (int)(gnc / csh.C);
      cv3_c8[i] = (int)(gnc - (long)rs * csh.C);
      cv3_rr[i] = rs / csh.S;
      cv3_ss[i] = rs - cv3_rr[i] * csh.S;
      const int k = (CMODE == 4 ? 2 : 1) * (g / (BN / 8));
      const long gm0 = k_begin + k;
      st3_ow[i] = (int)(gm0 % csh.OW);
      st3_oh[i] = (int)((gm0 / csh.OW) % csh.OH);
      st3_nb[i] = (long)(gm0 / ((long)csh.OW * csh.OH)) * csh.H;
    }
  }

  const bf16 zero = f2b(0.f);
  for (long k0 = k_begin; k0 < k_end; k0 += BK) {
    // ---- stage A tile (16-byte vector path when layout permits) ----
    if (CMODE == 1 || CMODE == 2) {  // implicit A gather (x / dy)
      constexpr int GROUPS = (BM * BK) / 8;
#pragma unroll
      for (int i = 0; i < AGI; ++i) {
        const int g = tid + i * THREADS;
        if (GROUPS % THREADS != 0 && g >= GROUPS) break;
        const int m = g / (BK / 8), k8 = (g % (BK / 8)) * 8;
        const long gk = k0 + k8;
        bool ok = cv_mok[i] && gk < k_end;
        long src = 0;
        if (ok && CMODE == 1) {  // fwd: x gather
          const int ih = cv_i0[i] + st_rr[i];
          const int iw = cv_j0[i] + st_ss[i];
          ok = ih >= 0 && ih < csh.H && iw >= 0 && iw < csh.W;
          src = ((cv_nbase[i] + ih) * csh.W + iw) * csh.C + st_c8[i];
        } else if (ok) {  // dgrad: dy gather, flipped correlation
          const int oh_num = cv_i0[i] - st_rr[i];
          const int ow_num = cv_j0[i] - st_ss[i];
          const int oh = oh_num / csh.stride;
          const int ow = ow_num / csh.stride;
          ok = oh_num >= 0 && ow_num >= 0 &&
               oh_num % csh.stride == 0 && ow_num % csh.stride == 0 &&
               oh < csh.OH && ow < csh.OW;
          src = ((cv_nbase[i] + oh) * csh.OW + ow) * csh.Kout + st_c8[i];
        }
        if (ok) {
          *reinterpret_cast<bf16x8_t*>(&As[m][swz(m, k8)]) =
              *reinterpret_cast<const bf16x8_t*>(&A[src]);
        } else {
          u16x8_t z = {};
          *reinterpret_cast<bf16x8_t*>(&As[m][swz(m, k8)]) =
              *reinterpret_cast<const bf16x8_t*>(&z);
        }
        {  // advance (c8, s, r) by BK along the gather row
          const int inner = CMODE == 1 ? csh.C : csh.Kout;
          int c8n = st_c8[i] + BK;
          while (c8n >= inner) {
            c8n -= inner;
            if (++st_ss[i] == csh.S) { st_ss[i] = 0; ++st_rr[i]; }
          }
          st_c8[i] = c8n;
        }
      }
    } else if (vecA) {
      constexpr int GROUPS = (BM * BK) / 8;
#pragma unroll
      for (int i = 0; i < (GROUPS + THREADS - 1) / THREADS; ++i) {
        const int g = tid + i * THREADS;
        if (GROUPS % THREADS != 0 && g >= GROUPS) break;
        if (!TA) {  // A[M][K]: 8 consecutive k per thread
          const int m = g / (BK / 8), k8 = (g % (BK / 8)) * 8;
          const long gm = tile_m + m, gk = k0 + k8;
          if (gm < M && gk + 8 <= k_end) {
            *reinterpret_cast<bf16x8_t*>(&As[m][swz(m, k8)]) =
                *reinterpret_cast<const bf16x8_t*>(&A[gm * K + gk]);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              As[m][swz(m, k8) + j] = (gm < M && gk + j < k_end)
                                  ? A[gm * K + gk + j] : zero;
          }
        } else {    // A[K][M]: 8 consecutive m (same k) per thread
          const int k = g / (BM / 8), m8 = (g % (BM / 8)) * 8;
          const long gm = tile_m + m8, gk = k0 + k;
          if (gk < k_end && gm + 8 <= M) {
            const u16x8_t v =
                *reinterpret_cast<const u16x8_t*>(&A[gk * M + gm]);
#pragma unroll
            for (int j = 0; j < 8; ++j)
              *reinterpret_cast<unsigned short*>(
                  &As[m8 + j][swz(m8 + j, k)]) = v[j];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              As[m8 + j][swz(m8 + j, k)] =
                  (gk < k_end && gm + j < M) ? A[gk * M + gm + j] : zero;
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < (BM * BK) / THREADS; ++i) {
        int idx = tid + i * THREADS;
        int m = idx / BK, k = idx % BK;
        long gm = tile_m + m, gk = k0 + k;
        As[m][swz(m, k)] = (gm < M && gk < k_end)
                       ? (TA ? A[gk * M + gm] : A[gm * K + gk]) : zero;
      }
    }
    // ---- stage B tile ----
    if (CMODE == 4) {  // k-pair wgrad staging (b32 LDS writes)
      constexpr int GROUPS = (BN * BK) / 16;
#pragma unroll
      for (int i = 0; i < BGI; ++i) {
        const int g = tid + i * THREADS;
        if (GROUPS % THREADS != 0 && g >= GROUPS) break;
        const int k2 = g / (BN / 8), n8 = (g % (BN / 8)) * 8;
        const int k = 2 * k2;
        const long gn = tile_n + n8;
        const long gm0 = k0 + k;
        const bool okn = gn + 8 <= N;
        u16x8_t v0 = {}, v1 = {};
        if (okn && gm0 < k_end) {
          const int ih = st3_oh[i] * csh.stride - csh.pad + cv3_rr[i];
          const int iw = st3_ow[i] * csh.stride - csh.pad + cv3_ss[i];
          if (ih >= 0 && ih < csh.H && iw >= 0 && iw < csh.W)
            v0 = *reinterpret_cast<const u16x8_t*>(
                &B[((st3_nb[i] + ih) * csh.W + iw) * csh.C + cv3_c8[i]]);
        }
        if (okn && gm0 + 1 < k_end) {
          int ow1 = st3_ow[i] + 1, oh1 = st3_oh[i];
          long nb1 = st3_nb[i];
          if (ow1 == csh.OW) {
            ow1 = 0;
            if (++oh1 == csh.OH) { oh1 = 0; nb1 += csh.H; }
          }
          const int ih = oh1 * csh.stride - csh.pad + cv3_rr[i];
          const int iw = ow1 * csh.stride - csh.pad + cv3_ss[i];
          if (ih >= 0 && ih < csh.H && iw >= 0 && iw < csh.W)
            v1 = *reinterpret_cast<const u16x8_t*>(
                &B[((nb1 + ih) * csh.W + iw) * csh.C + cv3_c8[i]]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          u16x2_t w2v;
          w2v[0] = v0[j];
          w2v[1] = v1[j];
          *reinterpret_cast<u16x2_t*>(
              &Bs[n8 + j][swz(n8 + j, k)]) = w2v;
        }
        {  // advance m pair by BK
          int ow = st3_ow[i] + BK;
          while (ow >= csh.OW) {
            ow -= csh.OW;
            if (++st3_oh[i] == csh.OH) { st3_oh[i] = 0; st3_nb[i] += csh.H; }
          }
          st3_ow[i] = ow;
        }
      }
    } else if (CMODE == 3) {
      // wgrad implicit col: B[k'=m][n'=(r,s,c)]; a granule is 8
      // consecutive c at fixed (m, r, s) -> one contiguous x load,
      // scatter-written like the vecB !TB path (col never exists).
      // The n'-side (r, s, c8) decode is fixed per slot across
      // k-steps; only the m decode varies.
      constexpr int GROUPS = (BN * BK) / 8;
#pragma unroll
      for (int i = 0; i < (GROUPS + THREADS - 1) / THREADS; ++i) {
        const int g = tid + i * THREADS;
        if (GROUPS % THREADS != 0 && g >= GROUPS) break;
        const int k = g / (BN / 8), n8 = (g % (BN / 8)) * 8;
        const long gn = tile_n + n8;   // (r, s, c8) flat index
        const long gm = k0 + k;        // m = (n, oh, ow)
        bool ok = gm < k_end && gn + 8 <= N;
        u16x8_t v = {};
        if (ok) {
          const int ih = st3_oh[i] * csh.stride - csh.pad + cv3_rr[i];
          const int iw = st3_ow[i] * csh.stride - csh.pad + cv3_ss[i];
          if (ih >= 0 && ih < csh.H && iw >= 0 && iw < csh.W)
            v = *reinterpret_cast<const u16x8_t*>(
                &B[((st3_nb[i] + ih) * csh.W + iw) * csh.C + cv3_c8[i]]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          *reinterpret_cast<unsigned short*>(
              &Bs[n8 + j][swz(n8 + j, k)]) = v[j];
        {  // advance m = (n, oh, ow) by BK
          int ow = st3_ow[i] + BK;
          while (ow >= csh.OW) {
            ow -= csh.OW;
            if (++st3_oh[i] == csh.OH) { st3_oh[i] = 0; st3_nb[i] += csh.H; }
          }
          st3_ow[i] = ow;
        }
      }
    } else if (vecB) {
      constexpr int GROUPS = (BN * BK) / 8;
#pragma unroll
      for (int i = 0; i < (GROUPS + THREADS - 1) / THREADS; ++i) {
        const int g = tid + i * THREADS;
        if (GROUPS % THREADS != 0 && g >= GROUPS) break;
        if (TB) {   // B[N][K]: 8 consecutive k per thread
          const int n = g / (BK / 8), k8 = (g % (BK / 8)) * 8;
          const long gn = tile_n + n, gk = k0 + k8;
          if (gn < N && gk + 8 <= k_end) {
            *reinterpret_cast<bf16x8_t*>(&Bs[n][swz(n, k8)]) =
                *reinterpret_cast<const bf16x8_t*>(&B[gn * K + gk]);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              Bs[n][swz(n, k8) + j] = (gn < N && gk + j < k_end)
                                  ? B[gn * K + gk + j] : zero;
          }
        } else {    // B[K][N]: 8 consecutive n (same k) per thread
          const int k = g / (BN / 8), n8 = (g % (BN / 8)) * 8;
          const long gn = tile_n + n8, gk = k0 + k;
          if (gk < k_end && gn + 8 <= N) {
            const u16x8_t v =
                *reinterpret_cast<const u16x8_t*>(&B[gk * N + gn]);
#pragma unroll
            for (int j = 0; j < 8; ++j)
              *reinterpret_cast<unsigned short*>(
                  &Bs[n8 + j][swz(n8 + j, k)]) = v[j];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              Bs[n8 + j][swz(n8 + j, k)] =
                  (gk < k_end && gn + j < N) ? B[gk * N + gn + j] : zero;
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < (BN * BK) / THREADS; ++i) {
        int idx = tid + i * THREADS;
        int n = idx / BK, k = idx % BK;
        long gn = tile_n + n, gk = k0 + k;
        Bs[n][swz(n, k)] = (gn < N && gk < k_end)
                       ? (TB ? B[gn * K + gk] : B[gk * N + gn]) : zero;
      }
    }
    __syncthreads();

    bf16x8_t a_frag[FM], b_frag[FN];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
      a_frag[fm] = *reinterpret_cast<const bf16x8_t*>(
          &As[wm0 + fm * 16 + l15][swz(wm0 + fm * 16 + l15, l4 * 8)]);
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
      b_frag[fn] = *reinterpret_cast<const bf16x8_t*>(
          &Bs[wn0 + fn * 16 + l15][swz(wn0 + fn * 16 + l15, l4 * 8)]);
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[fm], b_frag[fn], acc[fm][fn], 0, 0, 0);
    __syncthreads();
  }

  if (Cpart) {  // split-K partial store (fp32, plain [M,N] layout)
    float* out = Cpart + (long)blockIdx.y * M * N;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const long col = tile_n + wn0 + fn * 16 + l15;
        if (col >= N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long row = tile_m + wm0 + fm * 16 + l4 * 4 + r;
          if (row < M) out[row * N + col] = acc[fm][fn][r];
        }
      }
    return;
  }

  float ssum[FN] = {}, ssq[FN] = {};
#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const long col = tile_n + wn0 + fn * 16 + l15;
      if (col >= N) continue;
      const float bv = bias ? b2f(bias[col]) : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = tile_m + wm0 + fm * 16 + l4 * 4 + r;
        if (row >= M) continue;
        float v = acc[fm][fn][r] + bv;
        if (relu) v = fmaxf(v, 0.f);
        const bf16 stored = f2b(v);
        if (bn_psum) {  // per-channel stats of the ROUNDED output
          const float sv = b2f(stored);
          ssum[fn] += sv;
          ssq[fn] += sv * sv;
        }
        if (store_mode == (int)EpStore::kConvNCHW) {
          const long img = row / ohw, sp = row % ohw;
          C[(img * N + col) * ohw + sp] = stored;
        } else {
          C[row * N + col] = stored;
        }
      }
    }
  }
  if (bn_psum) {
    // fixed-structure block reduce: each (column, slot) has exactly
    // one writing thread; slot = (m-wave, l4) -> deterministic sums,
    // partial row = this block's tile_m index (bitwise-stable layout).
    constexpr int SLOTS = WR * 4;
    __shared__ float eps_sum[BN * SLOTS], eps_sq[BN * SLOTS];
    __syncthreads();
    const int slot = (wave / WC) * 4 + l4;
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int cl = wn0 + fn * 16 + l15;
      eps_sum[cl * SLOTS + slot] = ssum[fn];
      eps_sq[cl * SLOTS + slot] = ssq[fn];
    }
    __syncthreads();
    const long mrow = tile_m / BM;
    for (int cl = tid; cl < BN; cl += THREADS) {
      const long col = tile_n + cl;
      if (col >= N) continue;
      float a = 0.f, b2 = 0.f;
#pragma unroll
      for (int sl = 0; sl < SLOTS; ++sl) {
        a += eps_sum[cl * SLOTS + sl];
        b2 += eps_sq[cl * SLOTS + sl];
      }
      bn_psum[mrow * N + col] = a;
      bn_psq[mrow * N + col] = b2;
    }
  }
}

// ---------------------------------------------------------------------------
// Large-shape path: 256x256 tile, BK=64, 8 waves (2Mx4N), double-buffered
// register staging (guide T14: ds_write tile t+1 right after the barrier,
// re-issue tile t+2 loads immediately, one barrier per K-step). Gated to
// M%256==0 && N%256==0 && K%64==0 so the hot loop has no bounds checks;
// other shapes use gemm_kernel above. LDS rows padded +8 bf16 (16 B):
// row stride 144 B walks 9 mod 16 16-B slots, so every ds_read_b128 /
// 16-B ds_write lane group hits 16 distinct slots (conflict-free).
// ---------------------------------------------------------------------------

constexpr int BK2 = 64;
// +16-element pad: ds_read_b128 lane groups mix both 32-lane halves
// ((l15, l4) pairs), and a row walk of 10 mod 16 16-B slots puts all 16
// lanes of a group on distinct slots (72 was 2-way conflicted: 37.5%
// of LDS cycles were conflict stalls in rocprof). 2*(256+256)*80*2 B =
// exactly the 160 KiB LDS.
constexpr int BKP2 = BK2 + 16;

// Both operands in the vector-staging layout (A [M][K], B [N][K]; the
// host pre-transposes anything else). M and K edges are bounds-guarded,
// so only N % BN == 0 and K % 8 == 0 gate this path.
// CMODE 1 = implicit-GEMM NHWC conv forward: A is x [N,H,W,C] and the
// im2col gather (k = (r*S+s)*C + c, C % 8 == 0 so a 16-B granule stays
// inside one (r,s) window) happens in the A staging — no col matrix.
// CMODE 2 = implicit dgrad: A is dy [N,OH,OW,Kout], k = (r*S+s)*Kout +
// kout (Kout % 8 == 0), gathered with the flipped-correlation geometry
// oh = (ih + pad - r) / stride (zero when misaligned/out of range) —
// no dcol matrix and no col2im pass. B is the pre-permuted
// wrot[c][(r,s,kout)] = w[kout][r][s][c].
// POOL (CMODE 1 only) = fused 2x2/stride-2 maxpool epilogue for
// grad-free forwards: the tile's row index is WINDOW-MAJOR,
// m' = ((n*PH + ph)*PW + pw)*4 + dy*2 + dx, so the four conv outputs of
// one pool window are rows l4*4 + 0..3 of a 16x16 MFMA tile — one
// lane's f32x4 accumulator. The epilogue rounds each to bf16 exactly as
// the plain store does, keeps the max and stores ONE value at pooled
// row m'/4: no cross-lane traffic, no LDS, and the full-resolution
// activation never reaches HBM. Only the per-granule (n, oh, ow) decode
// differs from the plain mode; the K-loop gather is shared.
// POOL == 2 is the training forward: the same epilogue also stores the
// argmax code (dy*2 + dx, the lane's accumulator index) to pool_idx. It
// is a separate instantiation, not a runtime null check, so the scoring
// kernel (POOL == 1) compiles to exactly what it was.
// (The 128x128 conv-forward tile is LDS-sized for two blocks per CU and
// sits right at the 128-VGPR line for that; its launch bound asks for
// 4 waves per SIMD so the extra staging variants cannot push it over.)
template <int BM, int BN, int CMODE = 0, int POOL = 0>
__launch_bounds__(512, (CMODE == 1 && BM == 128 && BN == 128) ? 4 : 1)
__global__ void gemm256_kernel(const bf16* __restrict__ A,
                               const bf16* __restrict__ B,
                               bf16* __restrict__ C, float* __restrict__ Cpart,
                               const bf16* __restrict__ bias, long M, long N,
                               long K, long kslice, int relu, int store_mode,
                               long ohw, ConvShape csh,
                               float* __restrict__ bn_psum = nullptr,
                               float* __restrict__ bn_psq = nullptr,
                               uint8_t* __restrict__ pool_idx = nullptr) {
  // wave grid: 2(M) x 4(N) for BN >= 64; 4(M) x 2(N) for BN == 32
  constexpr int WR = BN >= 64 ? 2 : 4, WC = BN >= 64 ? 4 : 2;
  constexpr int FM = BM / WR / 16, FN = BN / WC / 16;
  constexpr int GA = BM / 64;                    // A granules per thread
  constexpr int GBT = BN * 8;                    // total B granules
  constexpr int GB = GBT >= 512 ? GBT / 512 : 1;
  __shared__ __align__(16) bf16 As[2][BM][BKP2];
  __shared__ __align__(16) bf16 Bs[2][BN][BKP2];

  const int ntn = (int)((N + BN - 1) / BN);
  const int ntm = (int)((M + BM - 1) / BM);
  const int nwg = ntm * ntn;
  int bid = blockIdx.x;
  {  // XCD-bijective remap (guide T1)
    const int nxcd = 8;
    const int q = nwg / nxcd, r = nwg % nxcd;
    const int xcd = bid % nxcd, idx = bid / nxcd;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const long tile_m = (long)(bid / ntn) * BM;
  const long tile_n = (long)(bid % ntn) * BN;
  const long k_begin = (long)blockIdx.y * kslice;
  const long k_end = min(K, k_begin + kslice);
  const int nt = (int)((k_end - k_begin + BK2 - 1) / BK2);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;             // 8 waves: WR(M) x WC(N)
  const int wm0 = (wave / WC) * (BM / WR);
  const int wn0 = (wave % WC) * (BN / WC);
  const int l15 = lane & 15, l4 = lane >> 4;

  // staging registers; granule g -> tile row g/8, k8 (g%8)*8.
  // M rows beyond the matrix and K columns beyond k_end stage zeros
  // (zeros are MFMA-neutral), so edge tiles need no special kernel.
  bf16x8_t ra[GA], rb[GB];
  // implicit-conv per-granule row geometry (fixed across K-steps)
  long cv_rowbase[CMODE ? GA : 1];
  int cv_ih0[CMODE ? GA : 1], cv_iw0[CMODE ? GA : 1];
  bool cv_mok[CMODE ? GA : 1];
  // incremental k-decode state (carry-based, no divides in the staging
  // loop — the per-load gk/C and rs/S divides were two ~24-instruction
  // VALU sequences per granule per K-step; these kernels are
  // issue-bound, not memory-bound: MfmaUtil 7.6%, MemUnitStalled 0.1%
  // on the FEMNIST conv2 fwd, profiles/r02_pmc_femnist.md). kd_in =
  // c8 (CMODE 1: channel offset) / k8 (CMODE 2: Kout offset); load
  // calls advance by BK2 per K-step, monotone, so carries suffice —
  // same design as the sync kernel's staging (commit b3bec0e).
  int kd_in[CMODE ? GA : 1], kd_rr[CMODE ? GA : 1], kd_ss[CMODE ? GA : 1];
  if (CMODE == 1) {
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      const int g = tid + i * 512;
      const long gm = tile_m + (g >> 3);
      cv_mok[i] = gm < M;
      const long m = cv_mok[i] ? gm : 0;
      int ow, oh, n;
      if (POOL) {  // window-major rows: m = pooled pixel * 4 + dy*2 + dx
        const long pp = m >> 2;
        const int q = (int)(m & 3);
        const int pw_n = csh.OW >> 1, ph_n = csh.OH >> 1;
        ow = (int)(pp % pw_n) * 2 + (q & 1);
        oh = (int)((pp / pw_n) % ph_n) * 2 + (q >> 1);
        n = (int)(pp / ((long)pw_n * ph_n));
      } else {
        ow = (int)(m % csh.OW);
        oh = (int)((m / csh.OW) % csh.OH);
        n = (int)(m / ((long)csh.OW * csh.OH));
      }
      cv_rowbase[i] = (long)n * csh.H * csh.W * csh.C;
      cv_ih0[i] = oh * csh.stride - csh.pad;
      cv_iw0[i] = ow * csh.stride - csh.pad;
      const long gk0 = k_begin + (g & 7) * 8;
      const int rs0 = (int)(gk0 / csh.C);  // one divide at init only
      kd_in[i] = (int)(gk0 - (long)rs0 * csh.C);
      kd_rr[i] = rs0 / csh.S;
      kd_ss[i] = rs0 - kd_rr[i] * csh.S;
    }
  } else if (CMODE == 2) {
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      const int g = tid + i * 512;
      const long gm = tile_m + (g >> 3);  // row of dx: (n, ih, iw)
      cv_mok[i] = gm < M;
      const long m = cv_mok[i] ? gm : 0;
      const int iw = (int)(m % csh.W);
      const int ih = (int)((m / csh.W) % csh.H);
      const int n = (int)(m / ((long)csh.W * csh.H));
      cv_rowbase[i] = (long)n * csh.OH * csh.OW * csh.Kout;
      cv_ih0[i] = ih + csh.pad;  // oh_num = ih + pad - r
      cv_iw0[i] = iw + csh.pad;
      const long gk0 = k_begin + (g & 7) * 8;
      const int rs0 = (int)(gk0 / csh.Kout);  // one divide at init only
      kd_in[i] = (int)(gk0 - (long)rs0 * csh.Kout);
      kd_rr[i] = rs0 / csh.S;
      kd_ss[i] = rs0 - kd_rr[i] * csh.S;
    }
  }
  // CMODE 1 stages FULL K-steps (k0 + BK2 <= k_end) without the
  // gk < k_end guard or the scalar tail loads, and blocks whose whole
  // tile lies inside the matrix additionally drop the row / column
  // tests: M is 1e5..1e6 rows and K a few K-steps, so those guards
  // almost never fire yet cost an exec-mask region each in an
  // issue-bound loop. The guarded form stays for the partial last
  // K-step and for edge tiles; every variant stages the same values.
  // The spatial padding test is real work and stays everywhere.
  const bool cv_interior =
      CMODE == 1 && tile_m + BM <= M && tile_n + BN <= N;
  // block-uniform split of one K-step for the CMODE 1 k-decode carries
  const int kq_c = CMODE == 1 ? BK2 / csh.C : 0;
  const int kr_c = CMODE == 1 ? BK2 - kq_c * csh.C : 0;
  const int kq_r = CMODE == 1 ? kq_c / csh.S : 0;
  const int kq_s = CMODE == 1 ? kq_c - kq_r * csh.S : 0;
  // (always_inline: left to its size heuristic the compiler emitted the
  // 256-wide tiles' staging as a real call, with the register arrays
  // passed through scratch)
  auto load_tiles_v = [&](long k0, auto fullk_c, auto inter_c)
      __attribute__((always_inline)) {
    constexpr bool FK = CMODE == 1 && decltype(fullk_c)::value;
    constexpr bool IN = FK && decltype(inter_c)::value;
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      const int g = tid + i * 512;
      const long gk = k0 + (g & 7) * 8;
      if (CMODE == 1) {
        const int ih = cv_ih0[i] + kd_rr[i];
        const int iw = cv_iw0[i] + kd_ss[i];
        // one predicate, no short-circuit: unsigned compares fold the
        // >= 0 halves, bitwise & keeps it a single exec-mask region
        const bool ok = (IN || cv_mok[i]) & (FK || gk < k_end) &
                        ((unsigned)ih < (unsigned)csh.H) &
                        ((unsigned)iw < (unsigned)csh.W);
        if (ok) {
          ra[i] = *reinterpret_cast<const bf16x8_t*>(
              &A[cv_rowbase[i] + ((long)ih * csh.W + iw) * csh.C
                 + kd_in[i]]);
        } else {
          u16x8_t z = {};
          ra[i] = *reinterpret_cast<const bf16x8_t*>(&z);
        }
        // advance the decode to this granule's next K-step. Load calls
        // are monotone in k by exactly BK2 = kq_c*C + kr_c with
        // kq_c = kq_r*S + kq_s, all block-uniform, so the carries are
        // two conditional subtracts (kd_in < C, kd_ss < S hold on
        // entry) — the per-lane while loops this replaces were two
        // divergent exec-mask loops per granule per K-step.
        int c8n = kd_in[i] + kr_c;
        const int cc = c8n >= csh.C ? 1 : 0;
        kd_in[i] = c8n - (cc ? csh.C : 0);
        int ssn = kd_ss[i] + kq_s + cc;
        const int cs = ssn >= csh.S ? 1 : 0;
        kd_ss[i] = ssn - (cs ? csh.S : 0);
        kd_rr[i] += kq_r + cs;
        continue;
      }
      if (CMODE == 2) {
        bool ok = cv_mok[i] && gk < k_end;
        const int oh_num = cv_ih0[i] - kd_rr[i];
        const int ow_num = cv_iw0[i] - kd_ss[i];
        const int oh = oh_num / csh.stride;
        const int ow = ow_num / csh.stride;
        ok = ok && oh_num >= 0 && ow_num >= 0 &&
             oh_num % csh.stride == 0 && ow_num % csh.stride == 0 &&
             oh < csh.OH && ow < csh.OW;
        if (ok) {
          ra[i] = *reinterpret_cast<const bf16x8_t*>(
              &A[cv_rowbase[i] + ((long)oh * csh.OW + ow) * csh.Kout
                 + kd_in[i]]);
        } else {
          u16x8_t z = {};
          ra[i] = *reinterpret_cast<const bf16x8_t*>(&z);
        }
        int k8n = kd_in[i] + BK2;
        int dss = 0;
        while (k8n >= csh.Kout) { k8n -= csh.Kout; ++dss; }
        kd_in[i] = k8n;
        kd_ss[i] += dss;
        while (kd_ss[i] >= csh.S) { kd_ss[i] -= csh.S; ++kd_rr[i]; }
        continue;
      }
      const long gm = tile_m + (g >> 3);
      if (gm < M && gk + 8 <= k_end) {
        ra[i] = *reinterpret_cast<const bf16x8_t*>(&A[gm * K + gk]);
      } else {
        u16x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (gm < M && gk + j < k_end)
                     ? *reinterpret_cast<const unsigned short*>(
                           &A[gm * K + gk + j])
                     : (unsigned short)0;
        ra[i] = *reinterpret_cast<const bf16x8_t*>(&v);
      }
    }
#pragma unroll
    for (int i = 0; i < GB; ++i) {
      const int g = tid + i * 512;
      if (GBT < 512 && g >= GBT) break;
      const long gn = tile_n + (g >> 3);
      const long gk = k0 + (g & 7) * 8;
      if (FK) {
        if (IN || gn < N) {
          rb[i] = *reinterpret_cast<const bf16x8_t*>(&B[gn * K + gk]);
        } else {
          u16x8_t z = {};
          rb[i] = *reinterpret_cast<const bf16x8_t*>(&z);
        }
        continue;
      }
      if (gn < N && gk + 8 <= k_end) {
        rb[i] = *reinterpret_cast<const bf16x8_t*>(&B[gn * K + gk]);
      } else {
        u16x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (gn < N && gk + j < k_end)
                     ? *reinterpret_cast<const unsigned short*>(
                           &B[gn * K + gk + j])
                     : (unsigned short)0;
        rb[i] = *reinterpret_cast<const bf16x8_t*>(&v);
      }
    }
  };
  auto load_tiles = [&](long k0) __attribute__((always_inline)) {
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;
    if (CMODE == 1 && k0 + BK2 <= k_end) {  // block-uniform
      if (cv_interior) load_tiles_v(k0, yes{}, yes{});
      else load_tiles_v(k0, yes{}, no{});
    } else {
      load_tiles_v(k0, no{}, no{});
    }
  };
  auto write_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      const int g = tid + i * 512;
      *reinterpret_cast<bf16x8_t*>(&As[buf][g >> 3][(g & 7) * 8]) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < GB; ++i) {
      const int g = tid + i * 512;
      if (GBT < 512 && g >= GBT) break;
      *reinterpret_cast<bf16x8_t*>(&Bs[buf][g >> 3][(g & 7) * 8]) = rb[i];
    }
  };

  f32x4_t acc[FM][FN] = {};

  load_tiles(k_begin);
  write_tiles(0);
  if (nt > 1) load_tiles(k_begin + BK2);
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      write_tiles(cur ^ 1);
      if (t + 2 < nt) load_tiles(k_begin + (long)(t + 2) * BK2);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8_t af[FM], bfr[FN];
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
        af[fm] = *reinterpret_cast<const bf16x8_t*>(
            &As[cur][wm0 + fm * 16 + l15][kk * 32 + l4 * 8]);
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        bfr[fn] = *reinterpret_cast<const bf16x8_t*>(
            &Bs[cur][wn0 + fn * 16 + l15][kk * 32 + l4 * 8]);
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[fm], bfr[fn], acc[fm][fn], 0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }

  if (POOL && !Cpart) {
    // M % 4 == 0 (OH, OW even), so a lane's four rows are all inside
    // the matrix or all outside. The running max walks the window in
    // the pool kernel's order (code dy*2 + dx, strict >, from -inf) on
    // the values the plain epilogue would have stored. Split-K
    // launches store window-major fp32 partials below and pool in
    // splitk_reduce_pool_kernel.
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const long col = tile_n + wn0 + fn * 16 + l15;
        const long row0 = tile_m + wm0 + fm * 16 + l4 * 4;
        if (col >= N || row0 >= M) continue;
        const float bv = bias ? b2f(bias[col]) : 0.f;
        float best = -INFINITY;
        int bi = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[fm][fn][r] + bv;
          if (relu) v = fmaxf(v, 0.f);
          const float f = b2f(f2b(v));
          if (f > best) {
            best = f;
            if (POOL == 2) bi = r;
          }
        }
        C[(row0 >> 2) * N + col] = f2b(best);
        if (POOL == 2) pool_idx[(row0 >> 2) * N + col] = (uint8_t)bi;
      }
    }
    return;
  }

  if (Cpart) {  // split-K partial store (fp32, plain [M,N] layout)
    float* out = Cpart + (long)blockIdx.y * M * N;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const long col = tile_n + wn0 + fn * 16 + l15;
        if (col >= N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long row = tile_m + wm0 + fm * 16 + l4 * 4 + r;
          if (row < M) out[row * N + col] = acc[fm][fn][r];
        }
      }
    return;
  }

  float ssum[FN] = {}, ssq[FN] = {};
#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const long col = tile_n + wn0 + fn * 16 + l15;
      if (col >= N) continue;
      const float bv = bias ? b2f(bias[col]) : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = tile_m + wm0 + fm * 16 + l4 * 4 + r;
        if (row >= M) continue;
        float v = acc[fm][fn][r] + bv;
        if (relu) v = fmaxf(v, 0.f);
        const bf16 stored = f2b(v);
        if (bn_psum) {  // per-channel stats of the ROUNDED output
          const float sv = b2f(stored);
          ssum[fn] += sv;
          ssq[fn] += sv * sv;
        }
        if (store_mode == (int)EpStore::kConvNCHW) {
          const long img = row / ohw, sp = row % ohw;
          C[(img * N + col) * ohw + sp] = stored;
        } else {
          C[row * N + col] = stored;
        }
      }
    }
  }
  if (bn_psum) {
    // fixed-structure block reduce: each (column, slot) has exactly
    // one writing thread; slot = (m-wave, l4) -> deterministic sums,
    // partial row = this block's tile_m index (bitwise-stable layout).
    // Scratch ALIASES the staging LDS (full at 160 KiB; dead after the
    // K loop, whose trailing barrier ordered all reads).
    constexpr int SLOTS = WR * 4;
    float* eps_sum = reinterpret_cast<float*>(&As[0][0][0]);
    float* eps_sq = eps_sum + BN * SLOTS;
    __syncthreads();
    const int slot = (wave / WC) * 4 + l4;
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int cl = wn0 + fn * 16 + l15;
      eps_sum[cl * SLOTS + slot] = ssum[fn];
      eps_sq[cl * SLOTS + slot] = ssq[fn];
    }
    __syncthreads();
    const long mrow = tile_m / BM;
    for (int cl = tid; cl < BN; cl += 512) {
      const long col = tile_n + cl;
      if (col >= N) continue;
      float a = 0.f, b2 = 0.f;
#pragma unroll
      for (int sl = 0; sl < SLOTS; ++sl) {
        a += eps_sum[cl * SLOTS + sl];
        b2 += eps_sq[cl * SLOTS + sl];
      }
      bn_psum[mrow * N + col] = a;
      bn_psq[mrow * N + col] = b2;
    }
  }
}

// ---------------------------------------------------------------------------
// 8-phase 256x256 GEMM (cdna_hip_programming.md §5 "8-phase template"):
// global_load_lds direct staging (no staging registers, no ds_writes),
// counted vmcnt so prefetches stay in flight ACROSS raw barriers, two
// barriers per phase, setprio(1) around each MFMA cluster. Per K-tile
// (BK=64): 4 phases, each issuing one half-tile prefetch (2 glds) for
// tile t+1 and computing one (kk, fn-pair) quadrant = 16 MFMAs; one
// s_waitcnt vmcnt(2) per K-tile (tile t fully landed, the just-issued
// half of t+1 still in flight). LDS image is lane-linear [256][64]
// per operand (glds requirement); the bank swizzle therefore moves to
// the per-lane SOURCE address plus the same XOR on every ds_read
// (guide rule 21): byte ^= bit8->bit5 ^ bit10->bit6, which puts all 16
// lanes of a ds_read_b128 group on 16 distinct 16-B slots (verified by
// enumeration; the 37.5% SQ_LDS_BANK_CONFLICT of the padded layout
// came from groups mixing both 32-lane halves). Gated to M%256, N%256,
// K%64 (glds cannot zero-fill, so no edge guards here).
// ---------------------------------------------------------------------------

__device__ __forceinline__ int swz8p(int byte) {
  return byte ^ (((byte >> 8) & 1) << 5) ^ (((byte >> 10) & 1) << 6);
}

__launch_bounds__(512, 1)
__global__ void gemm8p_kernel(const bf16* __restrict__ A,
                              const bf16* __restrict__ B,
                              bf16* __restrict__ C, float* __restrict__ Cpart,
                              const bf16* __restrict__ bias, long M, long N,
                              long K, long kslice, int relu,
                              float* __restrict__ bn_psum = nullptr,
                              float* __restrict__ bn_psq = nullptr) {
  constexpr int FM = 8, FN = 4;
  // ONE shared object (a second one makes hipcc drain vmcnt before
  // every ds_read of a glds pipeline — guide §5 trap 4a):
  // [dbuf][op][row][k] bf16, 128 KiB.
  __shared__ __align__(16) bf16 lds[2][2][256][64];

  const int ntn = (int)(N / 256);
  const int nwg = (int)((M / 256) * ntn);
  int bid = blockIdx.x;
  {
    const int nxcd = 8;
    const int q = nwg / nxcd, r = nwg % nxcd;
    const int xcd = bid % nxcd, idx = bid / nxcd;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const long tile_m = (long)(bid / ntn) * 256;
  const long tile_n = (long)(bid % ntn) * 256;
  const long k_begin = (long)blockIdx.y * kslice;
  const long k_end = min(K, k_begin + kslice);
  const int nt = (int)((k_end - k_begin) / 64);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm0 = (wave >> 2) * 128;
  const int wn0 = (wave & 3) * 64;
  const int l15 = lane & 15, l4 = lane >> 4;

  // per-thread glds source coordinates (2 passes of 16 B per half-tile;
  // the linear LDS offset o maps to the swizzled logical element)
  int srow[2], scol[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = (tid + i * 512) * 16;
    srow[i] = o >> 7;                       // 0..127 within the half
    scol[i] = (swz8p(o) & 127) >> 1;        // element column 0..63
  }
  const char* lds_base = (const char*)&lds[0][0][0][0];

  // h: 0 = A rows 0-127, 1 = B rows 0-127, 2 = A rows 128-255,
  //    3 = B rows 128-255
  auto issue_half = [&](int buf, long kt, int h) {
    const int op = h & 1, half = h >> 1;
    const bf16* src = op == 0 ? A : B;
    const long brow = (op == 0 ? tile_m : tile_n) + half * 128;
    const long k0 = k_begin + kt * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bf16* gp = &src[(brow + srow[i]) * K + k0 + scol[i]];
      char* lp = (char*)&lds[buf][op][half * 128][0] + wave * 1024 +
                 i * 8192;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)gp,
          (__attribute__((address_space(3))) unsigned int*)lp, 16, 0, 0);
    }
  };

  f32x4_t acc[FM][FN] = {};
  bf16x8_t a8[FM];

  // prologue: stage all 4 halves of tile 0
#pragma unroll
  for (int h = 0; h < 4; ++h) issue_half(0, 0, h);

  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    const char* abase = (const char*)&lds[buf][0][0][0];
    const char* bbase = (const char*)&lds[buf][1][0][0];
    auto do_phase = [&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr int kk = q >> 1, p = q & 1;
      if (t + 1 < nt) issue_half(buf ^ 1, t + 1, q);
      if (q == 0) {
        if (t + 1 < nt)
          asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      // issue this phase's ds_reads BEFORE the barrier (phases 1-3:
      // the tile landed at phase 0, and the read latency then hides
      // under the barrier wait); phase 0 must read after the
      // vmcnt+barrier pair that publishes the tile.
      bf16x8_t b2[2];
      auto load_frags = [&]() {
        if (p == 0) {  // (re)load the kk A-fragments
#pragma unroll
          for (int fm = 0; fm < FM; ++fm) {
            const int byte =
                (wm0 + fm * 16 + l15) * 128 + kk * 64 + l4 * 16;
            a8[fm] = *reinterpret_cast<const bf16x8_t*>(abase + swz8p(byte));
          }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int byte =
              (wn0 + (2 * p + j) * 16 + l15) * 128 + kk * 64 + l4 * 16;
          b2[j] = *reinterpret_cast<const bf16x8_t*>(bbase + swz8p(byte));
        }
      };
      if (q > 0) load_frags();
      // ONE barrier per phase: reads are issued pre-barrier, and the
      // MFMA cluster touches no LDS, so the next phase's pre-barrier
      // reads are ordered against this phase's by this barrier alone
      // (cross-tile glds writes stay >= one barrier behind the last
      // reads of the buffer they overwrite).
      __builtin_amdgcn_s_barrier();
      if (q == 0) load_frags();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[fm][2 * p + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a8[fm], b2[j], acc[fm][2 * p + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    };
    do_phase(std::integral_constant<int, 0>{});
    do_phase(std::integral_constant<int, 1>{});
    do_phase(std::integral_constant<int, 2>{});
    do_phase(std::integral_constant<int, 3>{});
  }
  (void)lds_base;

  if (Cpart) {
    float* out = Cpart + (long)blockIdx.y * M * N;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const long col = tile_n + wn0 + fn * 16 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long row = tile_m + wm0 + fm * 16 + l4 * 4 + r;
          out[row * N + col] = acc[fm][fn][r];
        }
      }
    return;
  }
  float ssum[FN] = {}, ssq[FN] = {};
#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const long col = tile_n + wn0 + fn * 16 + l15;
      const float bv = bias ? b2f(bias[col]) : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = tile_m + wm0 + fm * 16 + l4 * 4 + r;
        float v = acc[fm][fn][r] + bv;
        if (relu) v = fmaxf(v, 0.f);
        const bf16 stored = f2b(v);
        if (bn_psum) {
          const float sv = b2f(stored);
          ssum[fn] += sv;
          ssq[fn] += sv * sv;
        }
        C[row * N + col] = stored;
      }
    }
  }
  if (bn_psum) {
    // same fixed-structure per-tile stats as gemm256_kernel; the 128 KB
    // glds LDS image is dead after the K loop (loop barriers ordered
    // all reads) and is reused as scratch.
    constexpr int SLOTS = 8;  // 2 m-waves x l4
    float* eps_sum = reinterpret_cast<float*>(&lds[0][0][0][0]);
    float* eps_sq = eps_sum + 256 * SLOTS;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain any glds
    __builtin_amdgcn_s_barrier();
    const int slot = (wave >> 2) * 4 + l4;
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int cl = wn0 + fn * 16 + l15;
      eps_sum[cl * SLOTS + slot] = ssum[fn];
      eps_sq[cl * SLOTS + slot] = ssq[fn];
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const long mrow = tile_m / 256;
    for (int cl = tid; cl < 256; cl += 512) {
      float a = 0.f, b2 = 0.f;
#pragma unroll
      for (int sl = 0; sl < SLOTS; ++sl) {
        a += eps_sum[cl * SLOTS + sl];
        b2 += eps_sq[cl * SLOTS + sl];
      }
      bn_psum[mrow * N + tile_n + cl] = a;
      bn_psq[mrow * N + tile_n + cl] = b2;
    }
  }
}

// LDS-tiled bf16 transpose: out[C][R] = in[R][C]^T. 64x64 tiles, 16-B
// coalesced loads AND stores (the scatter happens inside LDS where the
// +8-element row pad keeps consecutive-row column reads conflict-free).
// Used to pre-transpose GEMM operands whose layout would otherwise need
// scalar scatter LDS staging in the 256-tile path (measured 3.4x slower
// than the all-vector layout at 4096^3).
__global__ void transpose_bf16_kernel(const bf16* __restrict__ in,
                                      bf16* __restrict__ out, long R,
                                      long C) {
  __shared__ __align__(16) bf16 t[64][72];
  const long tr = (long)blockIdx.y * 64;
  const long tc = (long)blockIdx.x * 64;
  const int tid = threadIdx.x;  // 256
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int g = tid + p * 256;
    const int r = g >> 3, c8 = (g & 7) * 8;
    const long gr = tr + r, gc = tc + c8;
    if (gr < R && gc + 8 <= C) {
      *reinterpret_cast<bf16x8_t*>(&t[r][c8]) =
          *reinterpret_cast<const bf16x8_t*>(&in[gr * C + gc]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        t[r][c8 + j] = (gr < R && gc + j < C) ? in[gr * C + gc + j]
                                              : f2b(0.f);
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int g = tid + p * 256;
    const int r = g >> 3, c8 = (g & 7) * 8;
    const long orow = tc + r, ocol = tr + c8;
    if (orow >= C) continue;
    u16x8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = *reinterpret_cast<const unsigned short*>(&t[c8 + j][r]);
    if (ocol + 8 <= R) {
      *reinterpret_cast<u16x8_t*>(&out[orow * R + ocol]) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (ocol + j < R)
          *reinterpret_cast<unsigned short*>(&out[orow * R + ocol + j]) =
              v[j];
    }
  }
}

// Deterministic split-K reduce: out = sum_s partial[s] (ascending s),
// then the fused epilogue (bias/relu/NCHW).
// Block = 8 slice-lanes x 32 output elements; each lane sums slices
// s === lane (mod 8) ascending, then a fixed-order 8-way combine — the
// reduction tree is independent of timing/data, so replicas stay
// bitwise identical (the old thread-per-element serial loop over up to
// 512 slices was latency-bound at ~50us/call).
// Plain-store fast path: one thread per 4 consecutive outputs, serial
// ascending-s walk (fixed order, deterministic) over the slice streams
// — all loads are 16-B and there is no LDS tree / barrier pair per 32
// outputs like the general kernel below. Requires N % 4 == 0 so a
// float4 never crosses a row (bias indexing stays affine).
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4_t;

__global__ void splitk_reduce_vec_kernel(const float* __restrict__ Cpart,
                                         int S, long M, long N,
                                         bf16* __restrict__ C,
                                         const bf16* __restrict__ bias,
                                         int relu) {
  const long total = M * N;
  const long total4 = total / 4;
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; t < total4; t += stride) {
    const long i = t * 4;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      const float4 v =
          *reinterpret_cast<const float4*>(&Cpart[(long)s * total + i]);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    float vj[4] = {acc.x, acc.y, acc.z, acc.w};
    const long col = i % N;
    u16x4_t out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (bias) vj[j] += b2f(bias[col + j]);
      if (relu) vj[j] = fmaxf(vj[j], 0.f);
      const bf16 b = f2b(vj[j]);
      out[j] = *reinterpret_cast<const unsigned short*>(&b);
    }
    *reinterpret_cast<u16x4_t*>(&C[i]) = out;
  }
}

__global__ void splitk_reduce_kernel(const float* __restrict__ Cpart, int S,
                                     long M, long N, bf16* __restrict__ C,
                                     const bf16* __restrict__ bias, int relu,
                                     int store_mode, long ohw) {
  const long total = M * N;
  const int slane = threadIdx.x >> 5;          // 0..7
  const int elane = threadIdx.x & 31;
  long i = (long)blockIdx.x * 32 + elane;
  const long stride = (long)gridDim.x * 32;
  __shared__ float red[8][33];
  for (; i - elane < total; i += stride) {
    // 4 independent accumulators per s-lane: the serial s-walk left
    // one outstanding load per iteration on the small-output reduces
    // (dw[16][144], S~128: 10.8 us/call, 6% of a ResNet-20 round);
    // fixed combine order keeps the reduction deterministic.
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (i < total) {
      int s = slane;
      for (; s + 24 < S; s += 32) {
        a0 += Cpart[(long)s * total + i];
        a1 += Cpart[(long)(s + 8) * total + i];
        a2 += Cpart[(long)(s + 16) * total + i];
        a3 += Cpart[(long)(s + 24) * total + i];
      }
      if (s < S) { a0 += Cpart[(long)s * total + i]; s += 8; }
      if (s < S) { a1 += Cpart[(long)s * total + i]; s += 8; }
      if (s < S) { a2 += Cpart[(long)s * total + i]; }
    }
    const float acc = (a0 + a1) + (a2 + a3);
    red[slane][elane] = acc;
    __syncthreads();
    if (slane == 0 && i < total) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) v += red[r][elane];
      const long row = i / N, col = i - row * N;
      if (bias) v += b2f(bias[col]);
      if (relu) v = fmaxf(v, 0.f);
      if (store_mode == (int)EpStore::kConvNCHW) {
        const long img = row / ohw, sp = row % ohw;
        C[(img * N + col) * ohw + sp] = f2b(v);
      } else {
        C[i] = f2b(v);
      }
    }
    __syncthreads();
  }
}

// Which of the two reduce kernels (= which fixed summation order) a
// plain-store reduce of this size takes.
bool splitk_reduce_is_vec(long M, long N) {
  return N % 4 == 0 && M * N >= 131072;
}

// Split-K reduce of the pooled conv forward (gemm256_kernel POOL):
// the partials are window-major, so rows 4p..4p+3 are one pool window.
// One thread per pooled output sums each of its four elements in
// EXACTLY the order the plain reduce of the same (M, N) would —
// vec_order: serial ascending s (splitk_reduce_vec_kernel); else the
// 8-lane tree of splitk_reduce_kernel walked serially — then applies
// bias/ReLU/bf16 rounding and the pool kernel's running max. Split-K
// only fires when the launch is a handful of tiles, so the serial
// walk is never on a hot shape.
__global__ void splitk_reduce_pool_kernel(const float* __restrict__ Cpart,
                                          int S, long M, long N,
                                          bf16* __restrict__ C,
                                          const bf16* __restrict__ bias,
                                          int relu, int vec_order,
                                          uint8_t* __restrict__ idx) {
  const long total = M * N;
  const long totalp = total / 4;
  long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; o < totalp; o += stride) {
    const long p = o / N, col = o - p * N;
    float best = -INFINITY;
    int bi = 0;
    for (int r = 0; r < 4; ++r) {
      const long i = (p * 4 + r) * N + col;
      float v = 0.f;
      if (vec_order) {
        for (int s = 0; s < S; ++s) v += Cpart[(long)s * total + i];
      } else {
        for (int sl = 0; sl < 8; ++sl) {
          float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
          int s = sl;
          for (; s + 24 < S; s += 32) {
            a0 += Cpart[(long)s * total + i];
            a1 += Cpart[(long)(s + 8) * total + i];
            a2 += Cpart[(long)(s + 16) * total + i];
            a3 += Cpart[(long)(s + 24) * total + i];
          }
          if (s < S) { a0 += Cpart[(long)s * total + i]; s += 8; }
          if (s < S) { a1 += Cpart[(long)s * total + i]; s += 8; }
          if (s < S) { a2 += Cpart[(long)s * total + i]; }
          v += (a0 + a1) + (a2 + a3);
        }
      }
      if (bias) v += b2f(bias[col]);
      if (relu) v = fmaxf(v, 0.f);
      const float f = b2f(f2b(v));
      if (f > best) { best = f; bi = r; }
    }
    C[o] = f2b(best);
    if (idx) idx[o] = (uint8_t)bi;  // training forward: argmax code
  }
}

void launch_splitk_reduce_pool(const float* part, long S, long M, long N,
                               bf16* c, const bf16* bias, int relu,
                               uint8_t* idx) {
  const long totalp = M * N / 4;
  const int blocks = (int)std::min<long>((totalp + 255) / 256, 16384);
  hipLaunchKernelGGL(splitk_reduce_pool_kernel, dim3(blocks), dim3(256), 0,
                     cur_stream(), part, (int)S, M, N, c, bias, relu,
                     splitk_reduce_is_vec(M, N) ? 1 : 0, idx);
  HIP_CHECK(hipGetLastError());
}

void launch_splitk_reduce(const float* part, long S, long M, long N,
                          bf16* c, const bf16* bias, int relu,
                          EpStore store, long ohw) {
  const long total = M * N;
  // vec path only when the output alone supplies enough threads: the
  // serial ascending-s walk underfills the chip on the small-output,
  // many-slice reduces (dw [16][144] with S~128 -> 3 blocks; routing
  // those here cost ResNet-20 21.0 -> 25.5 ms/round). The 8-lane-tree
  // kernel keeps 8-way S parallelism for them.
  if (store == EpStore::kPlain && splitk_reduce_is_vec(M, N)) {
    const long total4 = total / 4;
    const int blocks = (int)std::min<long>((total4 + 255) / 256, 16384);
    hipLaunchKernelGGL(splitk_reduce_vec_kernel, dim3(blocks), dim3(256),
                       0, cur_stream(), part, (int)S, M, N, c, bias, relu);
  } else {
    const int blocks = (int)std::min<long>((total + 31) / 32, 16384);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0,
                       cur_stream(), part, (int)S, M, N, c, bias, relu,
                       (int)store, ohw);
  }
  HIP_CHECK(hipGetLastError());
}

// Hierarchical colsum: pass 1 tiles rows into fp32 partials, pass 2
// reduces chunks in fixed ascending order. Block = 8 row-lanes x 32
// columns so each block has 8-way row parallelism (a single serial
// row-walk per thread was latency-bound at ~300us/call).
// Vectorized pass 1 (N % 8 == 0): RL row-lanes x G 16-B column
// granules per 256-thread block, fixed pairwise halving tree over the
// row-lanes (structure-deterministic).
__global__ void colsum_part_vec_kernel(const bf16* __restrict__ X, long M,
                                       long N, int G, long chunk_rows,
                                       float* __restrict__ part) {
  const int gi = threadIdx.x % G, rl = threadIdx.x / G;
  const int RL = (int)blockDim.x / G;
  const long c8 = ((long)blockIdx.x * G + gi) * 8;
  const long r0 = (long)blockIdx.y * chunk_rows;
  const long r1 = min(M, r0 + chunk_rows);
  float sj[8] = {};
  if (c8 < N)
    for (long m = r0 + rl; m < r1; m += RL) {
      const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(&X[m * N + c8]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sj[j] += b2f(v[j]);
    }
  __shared__ float rs[256][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) rs[threadIdx.x][j] = sj[j];
  __syncthreads();
  for (int h = RL >> 1; h > 0; h >>= 1) {
    if (rl < h) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        rs[rl * G + gi][j] += rs[(rl + h) * G + gi][j];
    }
    __syncthreads();
  }
  if (rl == 0 && c8 < N) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      part[(long)blockIdx.y * N + c8 + j] = rs[gi][j];
  }
}

// Fused relu-backward + column-sum partials: the biased-relu conv
// backward used to run relu_bwd (read y+dy, write dy') and then
// colsum_part (re-read all of dy') — together ~10% of a FEMNIST c1
// round. One pass masks, writes dx AND accumulates the db partials;
// same chunking/tree as colsum_part_vec, so db is bitwise what
// colsum(masked dy) produced.
__global__ void relu_bwd_colsum_part_vec_kernel(
    const bf16* __restrict__ y, const bf16* __restrict__ dy,
    bf16* __restrict__ dx, long M, long N, int G, long chunk_rows,
    float* __restrict__ part) {
  const int gi = threadIdx.x % G, rl = threadIdx.x / G;
  const int RL = (int)blockDim.x / G;
  const long c8 = ((long)blockIdx.x * G + gi) * 8;
  const long r0 = (long)blockIdx.y * chunk_rows;
  const long r1 = min(M, r0 + chunk_rows);
  float sj[8] = {};
  if (c8 < N)
    for (long m = r0 + rl; m < r1; m += RL) {
      const bf16x8_t yv =
          *reinterpret_cast<const bf16x8_t*>(&y[m * N + c8]);
      bf16x8_t gv = *reinterpret_cast<const bf16x8_t*>(&dy[m * N + c8]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!(b2f(yv[j]) > 0.f)) gv[j] = f2b(0.f);
        sj[j] += b2f(gv[j]);
      }
      *reinterpret_cast<bf16x8_t*>(&dx[m * N + c8]) = gv;
    }
  __shared__ float rs[256][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) rs[threadIdx.x][j] = sj[j];
  __syncthreads();
  for (int h = RL >> 1; h > 0; h >>= 1) {
    if (rl < h) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        rs[rl * G + gi][j] += rs[(rl + h) * G + gi][j];
    }
    __syncthreads();
  }
  if (rl == 0 && c8 < N) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      part[(long)blockIdx.y * N + c8 + j] = rs[gi][j];
  }
}

__global__ void colsum_part_kernel(const bf16* __restrict__ X, long M, long N,
                                   long chunk_rows,
                                   float* __restrict__ part) {
  const long col = (long)blockIdx.x * 32 + (threadIdx.x & 31);
  const int rlane = threadIdx.x >> 5;  // 0..7
  const int chunk = blockIdx.y;
  const long r0 = (long)chunk * chunk_rows;
  const long r1 = min(M, r0 + chunk_rows);
  float acc = 0.f;
  if (col < N)
    for (long m = r0 + rlane; m < r1; m += 8) acc += b2f(X[m * N + col]);
  __shared__ float red[8][33];
  red[rlane][threadIdx.x & 31] = acc;
  __syncthreads();
  if (rlane == 0 && col < N) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) t += red[r][threadIdx.x & 31];
    part[(long)chunk * N + col] = t;
  }
}

// Vectorized final (N % 4 == 0): float4 granules x KL chunk-lanes,
// fixed pairwise tree.
__global__ void colsum_final_vec_kernel(const float* __restrict__ part,
                                        int chunks, long N, int G,
                                        bf16* __restrict__ out) {
  const int gi = threadIdx.x % G, kl = threadIdx.x / G;
  const int KL = (int)blockDim.x / G;
  const long c4 = ((long)blockIdx.x * G + gi) * 4;
  float sj[4] = {};
  if (c4 < N)
    for (int k = kl; k < chunks; k += KL) {
      const float4 a =
          *reinterpret_cast<const float4*>(&part[(long)k * N + c4]);
      sj[0] += a.x; sj[1] += a.y; sj[2] += a.z; sj[3] += a.w;
    }
  __shared__ float rs[256][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) rs[threadIdx.x][j] = sj[j];
  __syncthreads();
  for (int h = KL >> 1; h > 0; h >>= 1) {
    if (kl < h) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        rs[kl * G + gi][j] += rs[(kl + h) * G + gi][j];
    }
    __syncthreads();
  }
  if (kl == 0 && c4 < N) {
#pragma unroll
    for (int j = 0; j < 4; ++j) out[c4 + j] = f2b(rs[gi][j]);
  }
}

// Scalar final fallback: fixed-order 8-lane tree (chunks can reach
// hundreds: a serial per-column loop was ~35us/call).
__global__ void colsum_final_kernel(const float* __restrict__ part,
                                    int chunks, long N,
                                    bf16* __restrict__ out) {
  const int clane = threadIdx.x >> 5;  // 0..7
  const int elane = threadIdx.x & 31;
  const long col = (long)blockIdx.x * 32 + elane;
  float acc = 0.f;
  if (col < N)
    for (int c = clane; c < chunks; c += 8) acc += part[(long)c * N + col];
  __shared__ float red[8][33];
  red[clane][elane] = acc;
  __syncthreads();
  if (clane == 0 && col < N) {
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) v += red[r][elane];
    out[col] = f2b(v);
  }
}

// ---- thin GEMM (K <= 32, N <= 64, both % 8; B in [N][K] layout) ----
// These shapes are memory-shaped (arithmetic intensity ~N/3 FLOP/B) and
// the MFMA tile machinery's LDS staging + barrier structure runs them
// ~4x off the traffic bound (the FEMNIST conv1 GEMM [802816x16]x[16->32]
// measured 47.6 us vs ~12 us of A+C traffic). A plain VALU dot kernel —
// one thread per output row, the whole B panel fp32 in LDS (broadcast
// reads, conflict-free), vectorized A reads and C writes — is bound by
// the A/C streams instead. KT is compile-time so the A row and the dot
// fully unroll in registers.
typedef __attribute__((ext_vector_type(8))) float f32x8v_t;
typedef __attribute__((ext_vector_type(2))) float f32x2v_t;
typedef uint8_t u8x8_t __attribute__((ext_vector_type(8)));

template <int KT>
__global__ __launch_bounds__(256) void gemm_thin_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    bf16* __restrict__ C, const bf16* __restrict__ bias, long M, int N,
    int relu) {
  // B panel TRANSPOSED in LDS ([k][n], n contiguous) so the dot runs as
  // 8-wide vector FMAs per k with a broadcast a[k]: the [n][k] row-dot
  // form compiled to 125 v_mov per 64 v_pk_fma (operand shuffles around
  // the packed FMAs — 2/3 of the VALU slots).
  __shared__ float Bl[32 * 64];
  __shared__ float bl[64];
  for (int i = threadIdx.x; i < N * KT; i += blockDim.x)
    Bl[(i % KT) * 64 + i / KT] = b2f(B[i]);
  for (int i = threadIdx.x; i < N; i += blockDim.x)
    bl[i] = bias ? b2f(bias[i]) : 0.f;
  __syncthreads();
  // One row per thread. (A 4-rows-per-thread ILP variant — 1 LDS read
  // amortized over 4 FMAs — measured 69 us vs 46 on the FEMNIST conv1
  // shape: the fatter register file cut occupancy more than the issue
  // mix helped.)
  long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; m < M; m += stride) {
    // A row pre-DUPLICATED into aligned fp32 pairs: v_pk_fma_f32 wants
    // a 64-bit (2xf32) src for the broadcast operand, and with a plain
    // float a[KT] the compiler re-materialized the (a[k], a[k]) pair
    // INSIDE the n8 loop — 120 v_mov_b32 per 64 v_pk_fma, 2/3 of the
    // VALU slots burned on operand shuffles (profiles/r01_kernel_
    // resources.md). Duplicating once per row hoists all of it: the
    // same body now compiles to 8 v_mov per 64 v_pk_fma.
    f32x2v_t a2[KT];
    const bf16* arow = &A[m * KT];
#pragma unroll
    for (int k8 = 0; k8 < KT; k8 += 8) {
      const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(&arow[k8]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = b2f(v[j]);
        a2[k8 + j] = f32x2v_t{f, f};
      }
    }
    for (int n8 = 0; n8 < N; n8 += 8) {
      f32x8v_t acc = *reinterpret_cast<const f32x8v_t*>(&bl[n8]);
      f32x2v_t* acc2 = reinterpret_cast<f32x2v_t*>(&acc);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const f32x8v_t bv =
            *reinterpret_cast<const f32x8v_t*>(&Bl[k * 64 + n8]);
        const f32x2v_t* bv2 = reinterpret_cast<const f32x2v_t*>(&bv);
#pragma unroll
        for (int p = 0; p < 4; ++p) acc2[p] += bv2[p] * a2[k];
      }
      bf16x8_t out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = acc[j];
        if (relu && v < 0.f) v = 0.f;
        out[j] = f2b(v);
      }
      *reinterpret_cast<bf16x8_t*>(&C[m * N + n8]) = out;
    }
  }
}

// Implicit-gather variant for grad-free conv forwards (committee
// scoring runs 16 of the ~28 forwards per FL round and never reads the
// col buffer back): the A row is gathered straight from the NHWC input
// window instead of a materialized im2col matrix — for FEMNIST conv1
// that removes a 77 MB col write + 77 MB re-read per forward and keeps
// only the (L2-resident) x reads. Same dot order as the col-backed
// kernel over the same KT-padded taps => bitwise-identical output.
template <int KT>
__global__ __launch_bounds__(256) void gemm_thin_conv_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ B,
    bf16* __restrict__ C, const bf16* __restrict__ bias, ConvShape sh,
    long M, int N, int relu) {
  __shared__ float Bl[32 * 64];
  __shared__ float bl[64];
  for (int i = threadIdx.x; i < N * KT; i += blockDim.x)
    Bl[(i % KT) * 64 + i / KT] = b2f(B[i]);
  for (int i = threadIdx.x; i < N; i += blockDim.x)
    bl[i] = bias ? b2f(bias[i]) : 0.f;
  __syncthreads();
  const int OW = sh.OW, OHW = sh.OH * sh.OW;
  long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; m < M; m += stride) {
    const int n = (int)(m / OHW);
    const int rem = (int)(m % OHW);
    const int oh = rem / OW, ow = rem % OW;
    const int ih0 = oh * sh.stride - sh.pad;
    const int iw0 = ow * sh.stride - sh.pad;
    f32x2v_t a2[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) a2[t] = f32x2v_t{0.f, 0.f};
    int t = 0;
    for (int r = 0; r < sh.R; ++r) {
      const int ih = ih0 + r;
      const bool okh = ih >= 0 && ih < sh.H;
      for (int s = 0; s < sh.S; ++s) {
        const int iw = iw0 + s;
        const bool ok = okh && iw >= 0 && iw < sh.W;
        const long base =
            (((long)n * sh.H + ih) * sh.W + iw) * sh.C;
        for (int c = 0; c < sh.C; ++c, ++t) {
          const float f = ok ? b2f(X[base + c]) : 0.f;
          a2[t] = f32x2v_t{f, f};
        }
      }
    }
    for (int n8 = 0; n8 < N; n8 += 8) {
      f32x8v_t acc = *reinterpret_cast<const f32x8v_t*>(&bl[n8]);
      f32x2v_t* acc2 = reinterpret_cast<f32x2v_t*>(&acc);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const f32x8v_t bv =
            *reinterpret_cast<const f32x8v_t*>(&Bl[k * 64 + n8]);
        const f32x2v_t* bv2 = reinterpret_cast<const f32x2v_t*>(&bv);
#pragma unroll
        for (int p = 0; p < 4; ++p) acc2[p] += bv2[p] * a2[k];
      }
      bf16x8_t out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = acc[j];
        if (relu && v < 0.f) v = 0.f;
        out[j] = f2b(v);
      }
      *reinterpret_cast<bf16x8_t*>(&C[m * N + n8]) = out;
    }
  }
}

// Fused conv + bias + ReLU + 2x2/stride-2 maxpool for the thin
// grad-free forward (3x3, C = 1, stride 1: FEMNIST conv1). One thread
// per POOLED pixel gathers the 4x4 input patch once (16 taps where the
// four windows separately read 36), forms the four conv outputs with
// gemm_thin_conv_kernel's dot - same tap order, same packed FMAs; that
// kernel's seven K-padding taps, each fma(+0, +0, acc), are the one
// `+ 0.f` of thin::conv_pool_chain, the same bits - rounds each to bf16
// and keeps the pool kernel's running max, so the result is bitwise
// conv-then-pool while the full-resolution activation never exists. B is
// the unpadded [N][9] weight view. The chain itself lives in
// thin_pool_chain.h, shared with the fused conv stack of halo_conv.hip.
template <bool IDX>
__global__ __launch_bounds__(256) void gemm_thin_conv_pool_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ B,
    bf16* __restrict__ C, uint8_t* __restrict__ idx,
    const bf16* __restrict__ bias, ConvShape sh, long MP, int N, int relu) {
  __shared__ __align__(32) float Bl[9 * 64];
  __shared__ __align__(32) float bl[64];
  for (int i = threadIdx.x; i < N * 9; i += blockDim.x)
    Bl[(i % 9) * 64 + i / 9] = b2f(B[i]);
  for (int i = threadIdx.x; i < N; i += blockDim.x)
    bl[i] = bias ? b2f(bias[i]) : 0.f;
  __syncthreads();
  const int PW = sh.OW >> 1, PHW = (sh.OH >> 1) * PW;
  long mp = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; mp < MP; mp += stride) {
    const int n = (int)(mp / PHW);
    const int rem = (int)(mp % PHW);
    const int ih0 = (rem / PW) * 2 - sh.pad;
    const int iw0 = (rem % PW) * 2 - sh.pad;
    thin::f32x2 pd[4][4];  // input patch, pre-duplicated for v_pk_fma
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ih = ih0 + r;
      const bool okh = ih >= 0 && ih < sh.H;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int iw = iw0 + s;
        const bool ok = okh && iw >= 0 && iw < sh.W;
        const float f =
            ok ? b2f(X[((long)n * sh.H + ih) * sh.W + iw]) : 0.f;
        pd[r][s] = thin::f32x2{f, f};
      }
    }
    for (int n8 = 0; n8 < N; n8 += 8) {
      thin::bf16x8 out;
      thin::u8x8 oidx;  // training forward: argmax code dy*2 + dx
      thin::conv_pool_chain<IDX>(pd, &Bl[n8], 64, &bl[n8], relu, out, oidx);
      *reinterpret_cast<thin::bf16x8*>(&C[mp * N + n8]) = out;
      if (IDX) *reinterpret_cast<thin::u8x8*>(&idx[mp * N + n8]) = oidx;
    }
  }
}

static_assert(BK == kSmallBK && BK2 == kDbufBK,
              "gemm_plan.h slices K in the kernels' steps");

// ---- runtime plan -> compile-time kernel parameters ----
// Each mapping is written once; a launcher passes a generic lambda that
// names its kernel and keeps only what is its own (CMODE, POOL, flags).
template <int V>
using ic = std::integral_constant<int, V>;

template <class F>
void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// thin kernels: (8-padded) K -> KT
template <class F>
void dispatch_thin(long K, F&& f) {
  switch (K) {
    case 8: f(ic<8>{}); break;
    case 16: f(ic<16>{}); break;
    case 24: f(ic<24>{}); break;
    default: f(ic<32>{}); break;
  }
}

// gemm_kernel: f(BM, BN, WR, WC) for the tiles pick_tile can return
template <class F>
void dispatch_small(const GemmPlan& p, F&& f) {
  switch (p.bm * 1000 + p.bn) {
    case 128128: f(ic<128>{}, ic<128>{}, ic<2>{}, ic<2>{}); break;
    case 128064: f(ic<128>{}, ic<64>{}, ic<2>{}, ic<2>{}); break;
    case 128032: f(ic<128>{}, ic<32>{}, ic<2>{}, ic<2>{}); break;
    case  64128: f(ic<64>{}, ic<128>{}, ic<2>{}, ic<2>{}); break;
    case  64064: f(ic<64>{}, ic<64>{}, ic<2>{}, ic<2>{}); break;
    case  64032: f(ic<64>{}, ic<32>{}, ic<2>{}, ic<2>{}); break;
    case  32128: f(ic<32>{}, ic<128>{}, ic<1>{}, ic<4>{}); break;
    case  32064: f(ic<32>{}, ic<64>{}, ic<1>{}, ic<4>{}); break;
    case  32032: f(ic<32>{}, ic<32>{}, ic<2>{}, ic<1>{}); break;
    default: TORCH_CHECK(false, "no tile config for ", p.bm, "x", p.bn);
  }
}

// gemm256_kernel: f(BM, BN) for the tiles plan_dbuf can return
template <class F>
void dispatch_dbuf(const GemmPlan& p, F&& f) {
  switch (p.bm * 1000 + p.bn) {
    case 256256: f(ic<256>{}, ic<256>{}); break;
    case 256128: f(ic<256>{}, ic<128>{}); break;
    case 256064: f(ic<256>{}, ic<64>{}); break;
    case 128256: f(ic<128>{}, ic<256>{}); break;
    case 128128: f(ic<128>{}, ic<128>{}); break;
    case 128064: f(ic<128>{}, ic<64>{}); break;
    case  64256: f(ic<64>{}, ic<256>{}); break;
    case  64128: f(ic<64>{}, ic<128>{}); break;
    case  64064: f(ic<64>{}, ic<64>{}); break;
    default: TORCH_CHECK(false, "no dbuf tile config for ", p.bm, "x", p.bn);
  }
}

// fp32 split-K partials [S, M, N]; ptr stays null for a single slice.
struct SplitKPart {
  torch::Tensor buf;
  float* ptr = nullptr;
};

SplitKPart alloc_splitk_part(const GemmPlan& p, long M, long N,
                             const torch::Tensor& like) {
  SplitKPart part;
  if (p.S > 1) {
    part.buf = torch::empty({p.S, M, N}, like.options().dtype(at::kFloat));
    part.ptr = part.buf.data_ptr<float>();
  }
  return part;
}

// Fused BN partials (psum, psq), one [N] row per tile row; both null
// (and *out left empty) unless the caller's condition holds.
struct BnStatsPtrs {
  float* sum = nullptr;
  float* sq = nullptr;
};

BnStatsPtrs alloc_bn_stats(std::pair<torch::Tensor, torch::Tensor>* out,
                           bool want, const GemmPlan& p, long M, long N,
                           const torch::Tensor& like) {
  BnStatsPtrs st;
  if (out && want) {
    const long chunks = (M + p.bm - 1) / p.bm;
    const auto opt = like.options().dtype(at::kFloat);
    out->first = torch::empty({chunks, N}, opt);
    out->second = torch::empty({chunks, N}, opt);
    st.sum = out->first.data_ptr<float>();
    st.sq = out->second.data_ptr<float>();
  }
  return st;
}

// BFLC_WGRAD_SMALL: -1 never, 1 always, unset/0 = plan_dense's gate.
int wgrad_small_gate() {
  static const int v = [] {
    const char* e = getenv("BFLC_WGRAD_SMALL");
    return e ? atoi(e) : 0;
  }();
  return v;
}

// Double-buffered narrow-BN conv route (default OFF — measured
// negative): gemm256_kernel's BN==32 wave grid register-stages
// K-step t+2 while the MFMAs of t run, the theory being that the
// sync kernel serializes gather-stage -> barrier -> MFMA at ~10x
// the traffic bound. A/B on hardware (gpurun_out/r20_kd*.json):
// ResNet-20 protocol round 67.5 ms dbuf vs 64.0 sync, FEMNIST 9.05
// vs 9.07 — the sync kernel's 256-thread blocks oversubscribe each
// CU with multiple blocks, which already hides the stage latency;
// the 512-thread dbuf blocks halve that block-level parallelism
// and its staging VALU count is no lower (the real bound —
// MemUnitStalled ~0, profiles/r02_pmc_femnist.md). Kept behind
// BFLC_NARROW_DBUF=1 as the documented experiment.
bool narrow_dbuf_gate() {
  static const bool v = [] {
    const char* e = getenv("BFLC_NARROW_DBUF");
    return e && e[0] == '1';
  }();
  return v;
}

// The GEMM view of the implicit conv entries:
//   fwd:   y[M=N*OH*OW][Kout], K = R*S*C,    A = x gather
//   dgrad: y[M=N*H*W][C],      K = R*S*Kout, A = dy gather
//   wgrad: dW[Kout][R*S*C],    K = N*OH*OW,  B = x gather
struct GemmDims { long M, N, K; };

GemmDims conv_gemm_dims(ConvEntry e, const ConvShape& sh) {
  if (e == ConvEntry::kWgrad) return {sh.Kout, sh.RSC(), sh.M()};
  if (e == ConvEntry::kDgrad)
    return {(long)sh.N * sh.H * sh.W, sh.C, (long)sh.R * sh.S * sh.Kout};
  return {sh.M(), sh.Kout, sh.RSC()};
}

void launch_colsum_final(const float* part, int chunks, long N, bf16* out) {
  if (N % 4 == 0) {
    const int G4 = colsum_final_g4(N);
    hipLaunchKernelGGL(colsum_final_vec_kernel,
                       dim3(ceil_div(N / 4, (long)G4)), dim3(256), 0,
                       cur_stream(), part, chunks, N, G4, out);
  } else {
    hipLaunchKernelGGL(colsum_final_kernel, dim3(ceil_div(N, 32)),
                       dim3(256), 0, cur_stream(), part, chunks, N, out);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace

// Fused thin conv + ReLU + 2x2 maxpool: true if handled. Same gate as
// gemm_thin_conv_raw (on the UNPOOLED M, so the two routes switch at
// the same shape), restricted to the geometry the kernel unrolls.
bool gemm_thin_conv_pool_eligible(const ConvShape& sh) {
  return sh.R == 3 && sh.S == 3 && sh.C == 1 && sh.RSC() == 9 &&
         sh.stride == 1 && sh.OH % 2 == 0 && sh.OW % 2 == 0 &&
         sh.Kout <= 64 && sh.Kout % 8 == 0 && sh.M() >= 65536;
}

bool gemm_thin_conv_pool_raw(const torch::Tensor& x,
                             const torch::Tensor& w2, torch::Tensor& y,
                             const ConvShape& sh, const torch::Tensor* bias,
                             bool relu, uint8_t* idx) {
  if (!gemm_thin_conv_pool_eligible(sh) || w2.size(1) != 9) return false;
  const long MP = sh.M() / 4;
  const bf16* bs = bias ? (const bf16*)bias->data_ptr() : nullptr;
  const int blocks = (int)std::min<long>((MP + 255) / 256, 16384);
  dispatch_bool(idx != nullptr, [&](auto want_idx) {
    hipLaunchKernelGGL(
        (gemm_thin_conv_pool_kernel<decltype(want_idx)::value>),
        dim3(blocks), dim3(256), 0, cur_stream(), (const bf16*)x.data_ptr(),
        (const bf16*)w2.data_ptr(), (bf16*)y.data_ptr(), idx, bs, sh, MP,
        (int)sh.Kout, relu ? 1 : 0);
  });
  HIP_CHECK(hipGetLastError());
  return true;
}

// Col-free thin conv fwd: true if this shape is handled (the caller
// falls back to im2col + GEMM otherwise). w2p must already be KT-padded
// ([Kout][KT], KT = RSC rounded up to 8).
bool gemm_thin_conv_raw(const torch::Tensor& x, const torch::Tensor& w2p,
                        torch::Tensor& y, const ConvShape& sh,
                        const torch::Tensor* bias, bool relu) {
  const long M = sh.M();
  const long KT = w2p.size(1);
  const long N = sh.Kout;
  if (KT > 32 || KT % 8 != 0 || N > 64 || N % 8 != 0 || M < 65536)
    return false;
  const bf16* bs = bias ? (const bf16*)bias->data_ptr() : nullptr;
  const int blocks = (int)std::min<long>((M + 255) / 256, 16384);
  dispatch_thin(KT, [&](auto kt) {
    hipLaunchKernelGGL((gemm_thin_conv_kernel<decltype(kt)::value>),
                       dim3(blocks), dim3(256), 0, cur_stream(),
                       (const bf16*)x.data_ptr(),
                       (const bf16*)w2p.data_ptr(), (bf16*)y.data_ptr(),
                       bs, sh, M, (int)N, relu ? 1 : 0);
  });
  HIP_CHECK(hipGetLastError());
  return true;
}

torch::Tensor transpose_bf16(const torch::Tensor& X) {
  const long R = X.size(0), C = X.size(1);
  auto out = torch::empty({C, R}, X.options());
  dim3 grid((unsigned)ceil_div(C, 64), (unsigned)ceil_div(R, 64));
  hipLaunchKernelGGL(transpose_bf16_kernel, grid, dim3(256), 0, cur_stream(),
                     (const bf16*)X.data_ptr(), (bf16*)out.data_ptr(), R, C);
  HIP_CHECK(hipGetLastError());
  return out;
}

void gemm_bf16_raw(const torch::Tensor& A, const torch::Tensor& B,
                   torch::Tensor& C, long M, long N, long K, bool ta, bool tb,
                   const torch::Tensor* bias, bool relu, EpStore store,
                   long ohw,
                   std::pair<torch::Tensor, torch::Tensor>* bn_stats) {
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 &&
              B.scalar_type() == at::kBFloat16, "gemm: bf16 only");
  CHECK_GPU(A); CHECK_GPU(B); CHECK_CONTIG(A); CHECK_CONTIG(B);
  const bf16* a = (const bf16*)A.data_ptr();
  const bf16* b = (const bf16*)B.data_ptr();
  bf16* c = (bf16*)C.data_ptr();
  const bf16* bs = bias ? (const bf16*)bias->data_ptr() : nullptr;
  const int relu_i = relu ? 1 : 0, sm = (int)store;

  const GemmPlan p =
      plan_dense(M, N, K, ta, tb, store == EpStore::kPlain,
                 bn_stats != nullptr, wgrad_small_gate());
  if (p.path == GemmPath::kThin) {
    dispatch_thin(K, [&](auto kt) {
      hipLaunchKernelGGL((gemm_thin_kernel<decltype(kt)::value>),
                         dim3((unsigned)p.tiles), dim3(256), 0, cur_stream(),
                         a, b, c, bs, M, (int)N, relu_i);
    });
    HIP_CHECK(hipGetLastError());
    return;
  }

  const SplitKPart part = alloc_splitk_part(p, M, N, A);
  const dim3 grid((unsigned)p.tiles, (unsigned)p.S);
  if (p.path == GemmPath::kSmall) {
    const int vecA = ta ? (M % 8 == 0) : (K % 8 == 0);
    const int vecB = tb ? (K % 8 == 0) : (N % 8 == 0);
    dispatch_small(p, [&](auto bm, auto bn, auto wr, auto wc) {
      constexpr int BMv = decltype(bm)::value, BNv = decltype(bn)::value;
      constexpr int WRv = decltype(wr)::value, WCv = decltype(wc)::value;
      dispatch_bool(ta, [&](auto tav) {
        dispatch_bool(tb, [&](auto tbv) {
          hipLaunchKernelGGL(
              (gemm_kernel<BMv, BNv, WRv, WCv, decltype(tav)::value,
                           decltype(tbv)::value>),
              grid, dim3(WRv * WCv * 64), 0, cur_stream(), a, b, c, part.ptr,
              bs, M, N, K, p.kslice, relu_i, sm, ohw, vecA, vecB,
              ConvShape{});
        });
      });
    });
  } else {
    // Pre-transpose any operand whose layout would need scalar scatter
    // LDS staging: the all-vector (A [M][K], B [N][K]) kernel measured
    // 819 TF vs 137-242 TF for the scatter layouts at 4096^3, and the
    // tiled transpose costs ~2 round trips of the operand (~5% here).
    torch::Tensor At, Bt;
    if (ta) { At = transpose_bf16(A); a = (const bf16*)At.data_ptr(); }
    if (!tb) { Bt = transpose_bf16(B); b = (const bf16*)Bt.data_ptr(); }
    const BnStatsPtrs st = alloc_bn_stats(
        bn_stats, p.S == 1 && store == EpStore::kPlain, p, M, N, A);
    if (p.path == GemmPath::kGemm8p)
      hipLaunchKernelGGL(gemm8p_kernel, grid, dim3(512), 0, cur_stream(), a,
                         b, c, part.ptr, bs, M, N, K, p.kslice, relu_i,
                         st.sum, st.sq);
    else
      dispatch_dbuf(p, [&](auto bm, auto bn) {
        hipLaunchKernelGGL(
            (gemm256_kernel<decltype(bm)::value, decltype(bn)::value>), grid,
            dim3(512), 0, cur_stream(), a, b, c, part.ptr, bs, M, N, K,
            p.kslice, relu_i, sm, ohw, ConvShape{}, st.sum, st.sq);
      });
  }
  HIP_CHECK(hipGetLastError());
  if (p.S > 1)
    launch_splitk_reduce(part.ptr, p.S, M, N, c, bs, relu_i, store, ohw);
}

// Route query: the plan gemm_raw's launch takes for this shape (path,
// bm, bn, S, kslice). Allocates and launches nothing.
PlanRow gemm_plan_route(long M, long N, long K, bool ta, bool tb) {
  return plan_row(plan_dense(M, N, K, ta, tb, true, false,
                             wgrad_small_gate()));
}

// The same plan, for a kernel outside this file that has to reproduce a
// dense launch's split-K slices (the fused thin-layer wgrad, conv2d.hip).
GemmPlan gemm_dense_plan(long M, long N, long K, bool ta, bool tb) {
  return plan_dense(M, N, K, ta, tb, true, false, wgrad_small_gate());
}

// The plain-store split-K reduce gemm_bf16_raw ends with, over partials
// produced outside this file: out[M, N] = bf16(sum over S of part[s]),
// same kernel choice and fixed order for a given (S, M * N, N % 4).
void splitk_reduce_plain(const torch::Tensor& part, torch::Tensor& out) {
  launch_splitk_reduce(part.data_ptr<float>(), part.size(0), part.size(1),
                       part.size(2), (bf16*)out.data_ptr(), nullptr, 0,
                       EpStore::kPlain, 0);
}

std::tuple<long, long, long, long> colsum_geom_query(long M, long N) {
  const ColsumGeom g = colsum_geom(M, N);
  return {g.G, g.cblocks, g.rows, g.chunks};
}

torch::Tensor colsum_bf16(const torch::Tensor& X) {
  CHECK_GPU(X); CHECK_CONTIG(X);
  long M = X.size(0), N = X.size(1);
  auto out = torch::empty({N}, X.options());
  const ColsumGeom g = colsum_geom(M, N);
  auto part = torch::empty({g.chunks, N}, X.options().dtype(at::kFloat));
  if (N % 8 == 0) {
    hipLaunchKernelGGL(colsum_part_vec_kernel, dim3(g.cblocks, g.chunks),
                       dim3(256), 0, cur_stream(),
                       (const bf16*)X.data_ptr(), M, N, g.G, g.rows,
                       part.data_ptr<float>());
  } else {
    hipLaunchKernelGGL(colsum_part_kernel, dim3(g.cblocks, g.chunks),
                       dim3(256), 0, cur_stream(),
                       (const bf16*)X.data_ptr(), M, N, g.rows,
                       part.data_ptr<float>());
  }
  HIP_CHECK(hipGetLastError());
  launch_colsum_final(part.data_ptr<float>(), g.chunks, N,
                      (bf16*)out.data_ptr());
  return out;
}

// Second colsum pass for partials produced outside this file (the
// pooled conv backward): out[n] = bf16(sum over chunks of part[k][n]),
// the same kernels and fixed trees colsum_bf16 ends with.
void colsum_finalize(const torch::Tensor& part, torch::Tensor& out) {
  launch_colsum_final(part.data_ptr<float>(), (int)part.size(0),
                      part.size(1), (bf16*)out.data_ptr());
}

// Fused relu backward + bias-grad column sum over dy viewed [M, N]
// (N = trailing dim, %8). Returns (dx, db). Bitwise equal to
// relu_bwd() followed by colsum_bf16() — same masking, same partial
// chunking, same final tree.
std::tuple<torch::Tensor, torch::Tensor> relu_bwd_colsum(
    const torch::Tensor& y, const torch::Tensor& dy) {
  CHECK_GPU(y); CHECK_GPU(dy); CHECK_CONTIG(y); CHECK_CONTIG(dy);
  const long N = dy.size(-1);
  const long M = dy.numel() / N;
  TORCH_CHECK(N % 8 == 0, "relu_bwd_colsum: N % 8 required");
  TORCH_CHECK(y.numel() == dy.numel());
  auto dx = torch::empty_like(dy);
  auto out = torch::empty({N}, dy.options());
  const ColsumGeom g = colsum_geom(M, N);
  auto part = torch::empty({g.chunks, N}, dy.options().dtype(at::kFloat));
  hipLaunchKernelGGL(relu_bwd_colsum_part_vec_kernel,
                     dim3(g.cblocks, g.chunks), dim3(256), 0, cur_stream(),
                     (const bf16*)y.data_ptr(), (const bf16*)dy.data_ptr(),
                     (bf16*)dx.data_ptr(), M, N, g.G, g.rows,
                     part.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  launch_colsum_final(part.data_ptr<float>(), g.chunks, N,
                      (bf16*)out.data_ptr());
  return {dx, out};
}

// Plan of an implicit-GEMM conv entry; path kNone = the entry declines
// the shape (its caller materializes col / dcol instead). The launchers
// and conv_plan_route both ask here. The pooled forward gets the plain
// forward's plan (M counts the same rows, window-major), so every
// output element sees the same accumulation order and the fused result
// is bitwise conv-then-pool.
GemmPlan gemm_conv_plan(ConvEntry e, const ConvShape& sh) {
  const GemmDims d = conv_gemm_dims(e, sh);
  if (e == ConvEntry::kWgrad)
    // always the small-tile split-K shape (M' = Kout is small, K' = M
    // is huge)
    return sh.C % 8 == 0 ? plan_small(d.M, d.N, d.K) : GemmPlan{};
  const int inner = e == ConvEntry::kDgrad ? sh.Kout : sh.C;  // granule dim
  if (inner % 8 != 0 || d.M < 48) return {};
  // fused pool: double-buffered wide-N forward only
  if (e == ConvEntry::kFwdPool &&
      (d.N % 64 != 0 || d.N < 64 || sh.OH % 2 != 0 || sh.OW % 2 != 0))
    return {};
  return plan_conv(d.M, d.N, d.K, narrow_dbuf_gate());
}

namespace {

// CMODE 1: forward (optionally pooled), CMODE 2: dgrad.
template <int CMODE>
bool conv_implicit_gemm(const torch::Tensor& x, const torch::Tensor& w2,
                        torch::Tensor& y, const ConvShape& sh,
                        const torch::Tensor* bias, bool relu,
                        std::pair<torch::Tensor, torch::Tensor>* bn_stats
                        = nullptr, bool pool = false,
                        uint8_t* pool_idx = nullptr,
                        HaloMode halo = HaloMode::kAuto,
                        int max_blocks = 0) {
  const ConvEntry e = CMODE == 2 ? ConvEntry::kDgrad
                                 : (pool ? ConvEntry::kFwdPool
                                         : ConvEntry::kFwd);
  const GemmPlan p = gemm_conv_plan(e, sh);
  if (p.path == GemmPath::kNone || (pool && bn_stats)) return false;
  if constexpr (CMODE == 1) {
    // conv2's pooled forward: whole images in LDS, same MFMA chain
    if (pool && halo != HaloMode::kOff && halo_conv_gate(sh)) {
      halo_conv_fwd_pool_launch(x, w2, y, sh, bias, relu, pool_idx,
                                max_blocks);
      return true;
    }
  }
  const GemmDims d = conv_gemm_dims(e, sh);
  const long M = d.M, N = d.N, K = d.K;
  const bf16* a = (const bf16*)x.data_ptr();
  const bf16* b = (const bf16*)w2.data_ptr();
  bf16* c = (bf16*)y.data_ptr();
  const bf16* bs = bias ? (const bf16*)bias->data_ptr() : nullptr;
  const int relu_i = relu ? 1 : 0, plain = (int)EpStore::kPlain;
  const SplitKPart part = alloc_splitk_part(p, M, N, x);
  const dim3 grid((unsigned)p.tiles, (unsigned)p.S);
  const BnStatsPtrs st =
      alloc_bn_stats(bn_stats, CMODE == 1 && p.S == 1, p, M, N, x);
  if (p.path == GemmPath::kSmall) {
    dispatch_small(p, [&](auto bm, auto bn, auto wr, auto wc) {
      constexpr int BMv = decltype(bm)::value, BNv = decltype(bn)::value;
      constexpr int WRv = decltype(wr)::value, WCv = decltype(wc)::value;
      hipLaunchKernelGGL(
          (gemm_kernel<BMv, BNv, WRv, WCv, false, true, CMODE>), grid,
          dim3(WRv * WCv * 64), 0, cur_stream(), a, b, c, part.ptr, bs, M,
          N, K, p.kslice, relu_i, plain, 0, 0, 1, sh, st.sum, st.sq);
    });
  } else if (p.bn == 32) {  // the BFLC_NARROW_DBUF experiment
    auto launchn = [&](auto bm) {
      hipLaunchKernelGGL((gemm256_kernel<decltype(bm)::value, 32, CMODE>),
                         grid, dim3(512), 0, cur_stream(), a, b, c, part.ptr,
                         bs, M, N, K, p.kslice, relu_i, plain, 0, sh,
                         st.sum, st.sq);
    };
    if (p.bm == 128) launchn(ic<128>{});
    else launchn(ic<64>{});
  } else {
    dispatch_dbuf(p, [&](auto bm, auto bn) {
      constexpr int BMv = decltype(bm)::value, BNv = decltype(bn)::value;
      if constexpr (CMODE == 1) {
        // split-K launches pool (and pick the argmax) in the reduce
        if (pool && pool_idx && p.S == 1) {
          hipLaunchKernelGGL((gemm256_kernel<BMv, BNv, 1, 2>), grid,
                             dim3(512), 0, cur_stream(), a, b, c, part.ptr,
                             bs, M, N, K, p.kslice, relu_i, plain, 0, sh,
                             st.sum, st.sq, pool_idx);
          return;
        }
        if (pool) {
          hipLaunchKernelGGL((gemm256_kernel<BMv, BNv, 1, 1>), grid,
                             dim3(512), 0, cur_stream(), a, b, c, part.ptr,
                             bs, M, N, K, p.kslice, relu_i, plain, 0, sh,
                             st.sum, st.sq);
          return;
        }
      }
      hipLaunchKernelGGL((gemm256_kernel<BMv, BNv, CMODE>), grid, dim3(512),
                         0, cur_stream(), a, b, c, part.ptr, bs, M, N, K,
                         p.kslice, relu_i, plain, 0, sh, st.sum, st.sq);
    });
  }
  HIP_CHECK(hipGetLastError());
  if (p.S > 1 && pool)
    launch_splitk_reduce_pool(part.ptr, p.S, M, N, c, bs, relu_i, pool_idx);
  else if (p.S > 1)
    launch_splitk_reduce(part.ptr, p.S, M, N, c, bs, relu_i,
                         EpStore::kPlain, 0);
  return true;
}

}  // namespace

bool gemm_conv_fwd_raw(const torch::Tensor& x, const torch::Tensor& w2,
                       torch::Tensor& y, const ConvShape& sh,
                       const torch::Tensor* bias, bool relu,
                       std::pair<torch::Tensor, torch::Tensor>* bn_stats) {
  return conv_implicit_gemm<1>(x, w2, y, sh, bias, relu, bn_stats);
}

bool gemm_conv_fwd_pool_eligible(const ConvShape& sh) {
  return gemm_conv_plan(ConvEntry::kFwdPool, sh).path != GemmPath::kNone;
}

bool gemm_conv_fwd_pool_raw(const torch::Tensor& x, const torch::Tensor& w2,
                            torch::Tensor& y, const ConvShape& sh,
                            const torch::Tensor* bias, bool relu,
                            uint8_t* idx, HaloMode halo, int max_blocks) {
  if (halo == HaloMode::kForce) {
    halo_conv_fwd_pool_launch(x, w2, y, sh, bias, relu, idx, max_blocks);
    return true;
  }
  return conv_implicit_gemm<1>(x, w2, y, sh, bias, relu, nullptr, true, idx,
                               halo, max_blocks);
}

bool gemm_conv_dgrad_raw(const torch::Tensor& dy, const torch::Tensor& wrot2,
                         torch::Tensor& dx, const ConvShape& sh) {
  return conv_implicit_gemm<2>(dy, wrot2, dx, sh, nullptr, false);
}

// wgrad: dW[Kout, RSC] = dy2^T @ implicit-col(x). A = dy2 [M, Kout]
// through the TA scatter staging, B = x through the CMODE-3 gather —
// the col matrix never exists.
bool gemm_conv_wgrad_raw(const torch::Tensor& dy2, const torch::Tensor& x,
                         torch::Tensor& dw, const ConvShape& sh) {
  const GemmPlan p = gemm_conv_plan(ConvEntry::kWgrad, sh);
  if (p.path == GemmPath::kNone) return false;
  const GemmDims d = conv_gemm_dims(ConvEntry::kWgrad, sh);
  const bf16* a = (const bf16*)dy2.data_ptr();
  const bf16* b = (const bf16*)x.data_ptr();
  bf16* c = (bf16*)dw.data_ptr();
  const SplitKPart part = alloc_splitk_part(p, d.M, d.N, x);
  const dim3 grid((unsigned)p.tiles, (unsigned)p.S);
  // k-pair scatter staging (CMODE 4): each LDS slot owns two adjacent
  // k's of one n-granule, halving ds_write instructions in the staging
  // loop. Default ON since the round-2 A/B on MI355X: every wgrad-heavy
  // conv bwd shape improved (-5..-11% in benchmarks/op_bench.py,
  // profiles/r02_kpair_ab.md; ResNet-20 round 92.8 -> 90.2 ms) with
  // bit-identical values (51 conv/resnet GPU tests pass under either
  // mode). BFLC_WGRAD_KPAIR=0 restores the old staging for A/B.
  static const bool kpair = [] {
    const char* e = getenv("BFLC_WGRAD_KPAIR");
    return !e || atoi(e) != 0;
  }();
  dispatch_small(p, [&](auto bm, auto bn, auto wr, auto wc) {
    constexpr int BMv = decltype(bm)::value, BNv = decltype(bn)::value;
    constexpr int WRv = decltype(wr)::value, WCv = decltype(wc)::value;
    dispatch_bool(kpair, [&](auto kp) {
      constexpr int CM = decltype(kp)::value ? 4 : 3;
      hipLaunchKernelGGL(
          (gemm_kernel<BMv, BNv, WRv, WCv, true, false, CM>), grid,
          dim3(WRv * WCv * 64), 0, cur_stream(), a, b, c, part.ptr, nullptr,
          d.M, d.N, d.K, p.kslice, 0, (int)EpStore::kPlain, 0, 1, 0, sh);
    });
  });
  HIP_CHECK(hipGetLastError());
  if (p.S > 1)
    launch_splitk_reduce(part.ptr, p.S, d.M, d.N, c, nullptr, 0,
                         EpStore::kPlain, 0);
  return true;
}

// Raw GEMM entry (benchmark/ablation): C[M,N] = op(A) @ op(B).
torch::Tensor gemm_raw(torch::Tensor A, torch::Tensor B, bool ta, bool tb) {
  CHECK_GPU(A); CHECK_CONTIG(A); CHECK_CONTIG(B);
  const long M = ta ? A.size(1) : A.size(0);
  const long K = ta ? A.size(0) : A.size(1);
  const long N = tb ? B.size(0) : B.size(1);
  TORCH_CHECK((tb ? B.size(1) : B.size(0)) == K, "shape mismatch");
  auto C = torch::empty({M, N}, A.options());
  gemm_bf16_raw(A, B, C, M, N, K, ta, tb, nullptr, false, EpStore::kPlain, 0);
  return C;
}

// ---------------------------------------------------------------------------
// linear layer entry points (reference main.py:120 fwd, 127-130 bwd)
// ---------------------------------------------------------------------------

torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                         bool relu) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_CONTIG(w);
  long M = x.size(0), K = x.size(1), N = w.size(1);
  TORCH_CHECK(w.size(0) == K, "shape mismatch");
  auto y = torch::empty({M, N}, x.options());
  auto bc = b.contiguous();
  gemm_bf16_raw(x, w, y, M, N, K, false, false, &bc, relu,
                EpStore::kPlain, 0);
  return y;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> linear_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor dy, bool want_dx) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_CONTIG(w); CHECK_CONTIG(dy);
  long M = x.size(0), K = x.size(1), N = w.size(1);
  // want_dx=false: first-layer linears (logreg/MLP on raw features)
  // need no input gradient — skip the dx GEMM
  torch::Tensor dx;
  if (want_dx) {
    dx = torch::empty({M, K}, x.options());
    gemm_bf16_raw(dy, w, dx, M, K, N, false, true, nullptr, false,
                  EpStore::kPlain, 0);
  } else {
    dx = torch::empty({0}, x.options());
  }
  auto dw = torch::empty({K, N}, x.options());
  gemm_bf16_raw(x, dy, dw, K, N, M, true, false, nullptr, false,
                EpStore::kPlain, 0);
  auto db = colsum_bf16(dy);
  return {dx, dw, db};
}

}  // namespace bflc
