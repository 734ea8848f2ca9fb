// Conv2D (NHWC, bf16) for gfx950: channels-last is the MI355X-native
// layout — the innermost C dimension makes every gather a contiguous
// 16-byte vector access, so
//   - 1x1 stride-1 convolutions are PURE GEMMs: x viewed [M, C] feeds
//     the MFMA kernel directly, no im2col materialization at all
//     (ResNet-50 is dominated by 1x1 convs; the NCHW design spent 25%
//     of a round re-laying them out),
//   - RxS convolutions stage through a vectorized NHWC im2col / col2im
//     (C-contiguous copies, not scalar scatter),
//   - dy.view(M, Kout) is free (no NCHW->MK permute kernel), and the
//     GEMM epilogue stores NHWC output plainly (no scatter epilogue).
// The reference has no conv at all (its model is a 5x2 logistic
// regression, main.py:113-120); BASELINE configs 2/3/5 (FEMNIST CNN,
// ResNet-20/50) demand Conv2D fwd/bwd as hand-written CDNA4 kernels.
//
// Layouts: x [N, H, W, C], w [Kout, R, S, C], y [N, OH, OW, Kout].
// GEMM views (M = N*OH*OW, RSC = R*S*C, k = (r*S + s)*C + c):
//   fwd   y2[M,Kout] = col[M,RSC] @ w2[Kout,RSC]^T — implicit GEMM
//         (the col gather runs inside the GEMM's A staging) whenever
//         C % 8 == 0; 1x1 stride-1 convs feed x [M, C] directly.
//   dgrad dx[M',C] = dy-gather @ w.permute(3,1,2,0) implicit when
//         stride == 1 and 8 <= C <= 64 (small C = col-traffic-bound);
//         else dcol = dy2 @ w2^T then vectorized col2im.
//   wgrad dw[Kout,RSC] = dy2^T @ implicit-col(x) when Kout <= 64;
//         else a materialized col (reused from fwd when available).
// The gates are measured crossovers: implicit wins where the col
// matrix round trip (R*S times the activation bytes) dominates, the
// materialized dbuf/8-phase GEMM wins where MFMA work dominates.

#include "common.h"
#include "gemm_api.h"

namespace bflc {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// col[m][(r*S+s)*C + c8..] = x[n][ih][iw][c8..]  — one 16-B granule per
// thread iteration; C % 8 == 0.
__global__ void im2col_nhwc_vec_kernel(const bf16* __restrict__ x,
                                       bf16* __restrict__ col, ConvShape sh,
                                       long total_g) {
  const int c8g = sh.C / 8;
  const int rs = sh.R * sh.S;
  long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; g < total_g; g += stride) {
    const int c8 = (int)(g % c8g) * 8;
    const int k = (int)((g / c8g) % rs);
    const long m = g / ((long)c8g * rs);
    const int s = k % sh.S, r = k / sh.S;
    const int ow = (int)(m % sh.OW), oh = (int)((m / sh.OW) % sh.OH);
    const int n = (int)(m / ((long)sh.OW * sh.OH));
    const int ih = oh * sh.stride - sh.pad + r;
    const int iw = ow * sh.stride - sh.pad + s;
    bf16x8_t v;
    if (ih >= 0 && ih < sh.H && iw >= 0 && iw < sh.W) {
      v = *reinterpret_cast<const bf16x8_t*>(
          &x[(((long)n * sh.H + ih) * sh.W + iw) * sh.C + c8]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = f2b(0.f);
    }
    *reinterpret_cast<bf16x8_t*>(&col[m * sh.RSC() + (long)k * sh.C + c8])
        = v;
  }
}

// Variants for C % 8 != 0 (FEMNIST C=1, ResNet stems C=3). Both write
// the K padding to %8 inline (the host allocates with torch::empty, no
// separate fill pass) and emit only 16-B stores; a thread-per-(m,r,s)
// scalar kernel paid 2-B scattered stores + a zero-fill pass (49 us on
// the FEMNIST conv1 shape vs ~6 us of traffic).
//
// Short padded rows (rscp <= 32: FEMNIST conv1, CIFAR stems): one
// thread per row stages the whole row through a bf16x8 register window
// — fewer index divmods than the granule kernel and the row fits in
// 2-4 stores (FEMNIST: 25 us rowvec vs 40 us granule vs 49 us scalar).
__global__ void im2col_nhwc_rowvec_kernel(const bf16* __restrict__ x,
                                          bf16* __restrict__ col,
                                          ConvShape sh, long ldc,
                                          long total_m) {
  long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const bf16 zero = f2b(0.f);
  for (; m < total_m; m += stride) {
    const int ow = (int)(m % sh.OW), oh = (int)((m / sh.OW) % sh.OH);
    const int n = (int)(m / ((long)sh.OW * sh.OH));
    const int ih0 = oh * sh.stride - sh.pad;
    const int iw0 = ow * sh.stride - sh.pad;
    bf16x8_t buf;
    int nb = 0;
    long w = m * ldc;
    for (int r = 0; r < sh.R; ++r) {
      const int ih = ih0 + r;
      const bool okh = ih >= 0 && ih < sh.H;
      const bf16* row = &x[((long)n * sh.H + ih) * sh.W * sh.C];
      for (int s = 0; s < sh.S; ++s) {
        const int iw = iw0 + s;
        const bool ok = okh && iw >= 0 && iw < sh.W;
        for (int c = 0; c < sh.C; ++c) {
          buf[nb++] = ok ? row[(long)iw * sh.C + c] : zero;
          if (nb == 8) {
            *reinterpret_cast<bf16x8_t*>(&col[w]) = buf;
            w += 8;
            nb = 0;
          }
        }
      }
    }
    if (nb) {  // K padding: zero the tail granule
      for (; nb < 8; ++nb) buf[nb] = zero;
      *reinterpret_cast<bf16x8_t*>(&col[w]) = buf;
    }
  }
}

// Long rows (7x7 stems, RSC 147): granule-per-thread keeps the
// parallelism proportional to the row length.
__global__ void im2col_nhwc_gran_kernel(const bf16* __restrict__ x,
                                        bf16* __restrict__ col,
                                        ConvShape sh, long ldc,
                                        long total_g) {
  const int gran = (int)(ldc / 8);
  const int rsc = (int)sh.RSC();
  long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const bf16 zero = f2b(0.f);
  for (; g < total_g; g += stride) {
    const int gi = (int)(g % gran);
    const long m = g / gran;
    const int ow = (int)(m % sh.OW), oh = (int)((m / sh.OW) % sh.OH);
    const int n = (int)(m / ((long)sh.OW * sh.OH));
    const int ih0 = oh * sh.stride - sh.pad;
    const int iw0 = ow * sh.stride - sh.pad;
    const int k0 = gi * 8;
    bf16x8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      bf16 val = zero;
      if (k < rsc) {
        const int c = k % sh.C;
        const int rs = k / sh.C;
        const int s = rs % sh.S, r = rs / sh.S;
        const int ih = ih0 + r, iw = iw0 + s;
        if (ih >= 0 && ih < sh.H && iw >= 0 && iw < sh.W)
          val = x[(((long)n * sh.H + ih) * sh.W + iw) * sh.C + c];
      }
      v[j] = val;
    }
    *reinterpret_cast<bf16x8_t*>(&col[m * ldc + k0]) = v;
  }
}

// Gather col2im (dgrad): dx[n][ih][iw][c8..] = sum over valid (r,s) of
// dcol[m(oh,ow)][(r*S+s)*C + c8..]. Fixed (r,s) order => deterministic.
__global__ void col2im_nhwc_vec_kernel(const bf16* __restrict__ dcol,
                                       bf16* __restrict__ dx, ConvShape sh,
                                       long total_g) {
  const int c8g = sh.C / 8;
  long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const long rsc = sh.RSC();
  for (; g < total_g; g += stride) {
    const int c8 = (int)(g % c8g) * 8;
    const long i = g / c8g;  // (n, ih, iw)
    const int iw = (int)(i % sh.W), ih = (int)((i / sh.W) % sh.H);
    const int n = (int)(i / ((long)sh.W * sh.H));
    float acc[8] = {};
    for (int r = 0; r < sh.R; ++r) {
      const int oh_num = ih + sh.pad - r;
      if (oh_num < 0 || oh_num % sh.stride) continue;
      const int oh = oh_num / sh.stride;
      if (oh >= sh.OH) continue;
      for (int s = 0; s < sh.S; ++s) {
        const int ow_num = iw + sh.pad - s;
        if (ow_num < 0 || ow_num % sh.stride) continue;
        const int ow = ow_num / sh.stride;
        if (ow >= sh.OW) continue;
        const long m = ((long)n * sh.OH + oh) * sh.OW + ow;
        const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(
            &dcol[m * rsc + ((long)(r * sh.S + s)) * sh.C + c8]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += b2f(v[j]);
      }
    }
    bf16x8_t out;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = f2b(acc[j]);
    *reinterpret_cast<bf16x8_t*>(&dx[i * sh.C + c8]) = out;
  }
}

__global__ void col2im_nhwc_kernel(const bf16* __restrict__ dcol,
                                   bf16* __restrict__ dx, ConvShape sh,
                                   long total) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const long rsc = sh.RSC();
  for (; i < total; i += stride) {
    const int c = (int)(i % sh.C);
    const long p = i / sh.C;
    const int iw = (int)(p % sh.W), ih = (int)((p / sh.W) % sh.H);
    const int n = (int)(p / ((long)sh.W * sh.H));
    float acc = 0.f;
    for (int r = 0; r < sh.R; ++r) {
      const int oh_num = ih + sh.pad - r;
      if (oh_num < 0 || oh_num % sh.stride) continue;
      const int oh = oh_num / sh.stride;
      if (oh >= sh.OH) continue;
      for (int s = 0; s < sh.S; ++s) {
        const int ow_num = iw + sh.pad - s;
        if (ow_num < 0 || ow_num % sh.stride) continue;
        const int ow = ow_num / sh.stride;
        if (ow >= sh.OW) continue;
        const long m = ((long)n * sh.OH + oh) * sh.OW + ow;
        acc += b2f(dcol[m * rsc + ((long)(r * sh.S + s)) * sh.C + c]);
      }
    }
    dx[i] = f2b(acc);
  }
}

// ---- maxpool (NHWC, C-vectorized) ----
// The argmax is stored as the WINDOW code r*S+s in a uint8 (windows are
// tiny; R*S <= 255), not a global int32 offset: the index plane is the
// same element count as y, so int32 indices cost 2x the y bytes
// themselves — uint8 makes the fwd+bwd index traffic 1/4.
typedef uint8_t u8x8_t __attribute__((ext_vector_type(8)));

__global__ void maxpool_nhwc_vec_fwd(const bf16* __restrict__ x,
                                     bf16* __restrict__ y,
                                     uint8_t* __restrict__ idx, ConvShape sh,
                                     long total_g) {
  const int c8g = sh.C / 8;
  long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; g < total_g; g += stride) {
    const int c8 = (int)(g % c8g) * 8;
    const long m = g / c8g;
    const int ow = (int)(m % sh.OW), oh = (int)((m / sh.OW) % sh.OH);
    const int n = (int)(m / ((long)sh.OW * sh.OH));
    float best[8];
    int bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; bi[j] = 0; }
    for (int r = 0; r < sh.R; ++r) {
      const int ih = oh * sh.stride + r;
      if (ih >= sh.H) break;
      for (int s = 0; s < sh.S; ++s) {
        const int iw = ow * sh.stride + s;
        if (iw >= sh.W) break;
        const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(
            &x[(((long)n * sh.H + ih) * sh.W + iw) * sh.C + c8]);
        const int code = r * sh.S + s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = b2f(v[j]);
          if (f > best[j]) { best[j] = f; bi[j] = code; }
        }
      }
    }
    bf16x8_t out;
    u8x8_t oidx;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      out[j] = f2b(best[j]);
      oidx[j] = (uint8_t)bi[j];
    }
    *reinterpret_cast<bf16x8_t*>(&y[m * sh.C + c8]) = out;
    if (idx)  // grad-free forwards skip the mask write entirely
      *reinterpret_cast<u8x8_t*>(&idx[m * sh.C + c8]) = oidx;
  }
}

__global__ void maxpool_nhwc_vec_bwd(const bf16* __restrict__ dy,
                                     const uint8_t* __restrict__ idx,
                                     bf16* __restrict__ dx, ConvShape sh,
                                     long total_g) {
  const int c8g = sh.C / 8;
  long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; g < total_g; g += stride) {
    const int c8 = (int)(g % c8g) * 8;
    const long i = g / c8g;  // (n, ih, iw)
    const int iw = (int)(i % sh.W), ih = (int)((i / sh.W) % sh.H);
    const int n = (int)(i / ((long)sh.W * sh.H));
    const int oh_lo = max(0, (ih - sh.R + sh.stride) / sh.stride);
    const int oh_hi = min(sh.OH - 1, ih / sh.stride);
    const int ow_lo = max(0, (iw - sh.S + sh.stride) / sh.stride);
    const int ow_hi = min(sh.OW - 1, iw / sh.stride);
    float acc[8] = {};
    for (int oh = oh_lo; oh <= oh_hi; ++oh)
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        // this input pixel sits at window position (r,s) of (oh,ow)
        const int code = (ih - oh * sh.stride) * sh.S
                         + (iw - ow * sh.stride);
        const long m = ((long)n * sh.OH + oh) * sh.OW + ow;
        const u8x8_t iv = *reinterpret_cast<const u8x8_t*>(
            &idx[m * sh.C + c8]);
        const bf16x8_t dv = *reinterpret_cast<const bf16x8_t*>(
            &dy[m * sh.C + c8]);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if ((int)iv[j] == code) acc[j] += b2f(dv[j]);
      }
    bf16x8_t out;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = f2b(acc[j]);
    *reinterpret_cast<bf16x8_t*>(&dx[i * sh.C + c8]) = out;
  }
}

// Scalar maxpool for C % 8 != 0.
__global__ void maxpool_nhwc_fwd(const bf16* __restrict__ x,
                                 bf16* __restrict__ y,
                                 uint8_t* __restrict__ idx,
                                 ConvShape sh, long total) {
  long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; g < total; g += stride) {
    const int c = (int)(g % sh.C);
    const long m = g / sh.C;
    const int ow = (int)(m % sh.OW), oh = (int)((m / sh.OW) % sh.OH);
    const int n = (int)(m / ((long)sh.OW * sh.OH));
    float best = -INFINITY;
    int bi = 0;
    for (int r = 0; r < sh.R; ++r) {
      const int ih = oh * sh.stride + r;
      if (ih >= sh.H) break;
      for (int s = 0; s < sh.S; ++s) {
        const int iw = ow * sh.stride + s;
        if (iw >= sh.W) break;
        const float f =
            b2f(x[(((long)n * sh.H + ih) * sh.W + iw) * sh.C + c]);
        if (f > best) { best = f; bi = r * sh.S + s; }
      }
    }
    y[g] = f2b(best);
    idx[g] = (uint8_t)bi;
  }
}

__global__ void maxpool_nhwc_bwd(const bf16* __restrict__ dy,
                                 const uint8_t* __restrict__ idx,
                                 bf16* __restrict__ dx, ConvShape sh,
                                 long total) {
  long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; g < total; g += stride) {
    const int c = (int)(g % sh.C);
    const long i = g / sh.C;
    const int iw = (int)(i % sh.W), ih = (int)((i / sh.W) % sh.H);
    const int n = (int)(i / ((long)sh.W * sh.H));
    const int oh_lo = max(0, (ih - sh.R + sh.stride) / sh.stride);
    const int oh_hi = min(sh.OH - 1, ih / sh.stride);
    const int ow_lo = max(0, (iw - sh.S + sh.stride) / sh.stride);
    const int ow_hi = min(sh.OW - 1, iw / sh.stride);
    float acc = 0.f;
    for (int oh = oh_lo; oh <= oh_hi; ++oh)
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const int code = (ih - oh * sh.stride) * sh.S
                         + (iw - ow * sh.stride);
        const long m = ((long)n * sh.OH + oh) * sh.OW + ow;
        if ((int)idx[m * sh.C + c] == code) acc += b2f(dy[m * sh.C + c]);
      }
    dx[g] = f2b(acc);
  }
}

// ---- backward of conv + ReLU + 2x2/stride-2 maxpool (training) ----
// A 2x2/stride-2 window sends each pooled gradient to exactly one
// full-resolution position, and at that position the activation IS the
// pooled value, so the ReLU mask of the unpooled gradient is just
// y_pooled > 0: mask-then-unpool == unpool-then-mask. Neither kernel
// below reads the full-resolution activation.

// Unpool + ReLU mask + bias-gradient partials in one pass, replacing
// maxpool_nhwc_vec_bwd -> relu_bwd_colsum_part_vec_kernel. Gather form:
// one thread per FULL-resolution pixel x 8-channel granule reads its
// window's pooled dy and y (16 B each) and argmax codes (8 B) — the four
// pixels of a window share them through L1/L2 — and writes its 16 B of
// the masked plane once: y > 0 && idx == own code ? dy : 0.
// The rows, the chunking and the row-lane tree are exactly
// relu_bwd_colsum_part_vec_kernel's over the same [M, N] plane, so every
// thread adds the same values in the same order (the zeros included) and
// db is BITWISE what that chain gives, as is the plane (0.f + dy is the
// pool backward's own accumulate, so even the zero signs agree).
// STORE = false is the bias-gradient-only pass of the fused thin-layer
// wgrad route: the same rows, per-lane walk and tree with the plane
// store left out, so db keeps its bits while nothing full-resolution is
// written.
template <bool STORE>
__global__ void pool_relu_bwd_colsum_part_kernel(
    const bf16* __restrict__ yp, const uint8_t* __restrict__ idx,
    const bf16* __restrict__ dyp, bf16* __restrict__ dx, long M, long N,
    int H, int W, int G, long chunk_rows, float* __restrict__ part) {
  const int gi = threadIdx.x % G, rl = threadIdx.x / G;
  const int RL = (int)blockDim.x / G;
  const long c8 = ((long)blockIdx.x * G + gi) * 8;
  const long r0 = (long)blockIdx.y * chunk_rows;
  const long r1 = min(M, r0 + chunk_rows);
  const int PH = H >> 1, PW = W >> 1;
  const bf16 zero = f2b(0.f);
  float sj[8] = {};
  if (!STORE && c8 < N) {
    // The same per-lane ascending walk, so the same sums; what differs
    // is only how the rows are fetched. The geometry gives this kernel
    // about one wave per SIMD and ~50 rows per lane, so a load -> add
    // loop is pure latency (the plane store is not what the storing
    // variant waits for either): fetch U rows at once, then add them in
    // order, with no branch between that could pull the loads back to
    // their uses. Indices are 32-bit (the caller checks M * N < 2^31).
    constexpr int U = 8;
    const unsigned Wu = (unsigned)W, Hu = (unsigned)H;
    for (long m0 = r0 + rl; m0 < r1; m0 += (long)U * RL) {
      bf16x8_t yv[U], dv[U];
      u8x8_t iv[U];
      int code[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long mu = m0 + (long)u * RL;
        const unsigned m = (unsigned)(mu < r1 ? mu : m0);
        const unsigned row = m / Wu, n = row / Hu;
        const unsigned iw = m - row * Wu, ih = row - n * Hu;
        // past the chunk: a code no window has, so the row adds +0,
        // which leaves a sum that is never -0 (no addend is) unchanged
        code[u] = mu < r1 ? (int)((ih & 1) * 2 + (iw & 1)) : 8;
        const unsigned pm =
            ((n * PH + (ih >> 1)) * PW + (iw >> 1)) * (unsigned)N +
            (unsigned)c8;
        yv[u] = *reinterpret_cast<const bf16x8_t*>(&yp[pm]);
        dv[u] = *reinterpret_cast<const bf16x8_t*>(&dyp[pm]);
        iv[u] = *reinterpret_cast<const u8x8_t*>(&idx[pm]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float a = 0.f;
          if ((int)iv[u][j] == code[u]) a += b2f(dv[u][j]);
          bf16 g = f2b(a);
          if (!(b2f(yv[u][j]) > 0.f)) g = zero;
          sj[j] += b2f(g);
        }
      }
    }
  }
  if (STORE && c8 < N)
    for (long m = r0 + rl; m < r1; m += RL) {  // m = (n, ih, iw)
      const int iw = (int)(m % W), ih = (int)((m / W) % H);
      const long n = m / ((long)W * H);
      const int code = (ih & 1) * 2 + (iw & 1);
      const long pm = ((n * PH + (ih >> 1)) * PW + (iw >> 1)) * N + c8;
      const bf16x8_t yv = *reinterpret_cast<const bf16x8_t*>(&yp[pm]);
      const bf16x8_t dv = *reinterpret_cast<const bf16x8_t*>(&dyp[pm]);
      const u8x8_t iv = *reinterpret_cast<const u8x8_t*>(&idx[pm]);
      bf16x8_t gv;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float a = 0.f;
        if ((int)iv[j] == code) a += b2f(dv[j]);
        gv[j] = f2b(a);
        if (!(b2f(yv[j]) > 0.f)) gv[j] = zero;
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

// Direct weight + bias gradient of the thin first layer (3x3, C = 1,
// stride 1) through the pool: no dx is wanted there and dW is Kout x 9
// numbers, so nothing full-resolution is materialised at all — the
// im2col matrix, the K = M GEMM, its split-K reduce and the narrow copy
// are replaced by one pass over (x, pooled y, idx, pooled dy).
// One thread per pooled pixel x 8-channel granule (G granules x PL
// pixel-lanes per block) reads the 4x4 input patch once and keeps
// 8 x (9 dW + 1 db) fp32 accumulators. For each window position q,
// g_q = (idx == q && y > 0) ? dy : 0 feeds nine FMAs against statically
// indexed patch taps (no dynamic register indexing). Pixels ascend per
// lane, then a fixed halving tree over the pixel-lanes in LDS; partials
// [chunks][Kout][10] go to thin_conv_pool_wgrad_final_kernel.
constexpr int kWgradAcc = 10;  // 9 taps + db

__global__ __launch_bounds__(256) void thin_conv_pool_wgrad_part_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ yp,
    const uint8_t* __restrict__ idx, const bf16* __restrict__ dyp,
    ConvShape sh, long MP, int G, long chunk_rows,
    float* __restrict__ part) {
  const int tid = threadIdx.x;
  const int gi = tid % G, pl = tid / G;
  const int PL = 256 / G;
  const int N = sh.Kout;
  const int PW = sh.OW >> 1, PHW = (sh.OH >> 1) * PW;
  const long r0 = (long)blockIdx.x * chunk_rows;
  const long r1 = min(MP, r0 + chunk_rows);
  float acc[8][kWgradAcc] = {};
  if (pl < PL)
    for (long mp = r0 + pl; mp < r1; mp += PL) {
      const long n = mp / PHW;
      const int rem = (int)(mp % PHW);
      const int ih0 = (rem / PW) * 2 - sh.pad;
      const int iw0 = (rem % PW) * 2 - sh.pad;
      float p[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ih = ih0 + r;
        const bool okh = ih >= 0 && ih < sh.H;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int iw = iw0 + s;
          const bool ok = okh && iw >= 0 && iw < sh.W;
          p[r][s] = ok ? b2f(X[(n * sh.H + ih) * sh.W + iw]) : 0.f;
        }
      }
      const long o = mp * N + gi * 8;
      const bf16x8_t yv = *reinterpret_cast<const bf16x8_t*>(&yp[o]);
      const bf16x8_t gv = *reinterpret_cast<const bf16x8_t*>(&dyp[o]);
      const u8x8_t iv = *reinterpret_cast<const u8x8_t*>(&idx[o]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = b2f(yv[j]) > 0.f ? b2f(gv[j]) : 0.f;
        const int code = (int)iv[j];
        acc[j][9] += g;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float gq = code == q ? g : 0.f;
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s)
              acc[j][r * 3 + s] =
                  fmaf(gq, p[(q >> 1) + r][(q & 1) + s], acc[j][r * 3 + s]);
        }
      }
    }
  // [accumulator][thread] so a tree step reads consecutive addresses
  __shared__ float rs[kWgradAcc][256];
  int plp2 = 1;
  while (plp2 < PL) plp2 *= 2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int a = 0; a < kWgradAcc; ++a) rs[a][tid] = acc[j][a];
    __syncthreads();
    for (int h = plp2 >> 1; h > 0; h >>= 1) {
      if (pl < h && pl + h < PL) {
#pragma unroll
        for (int a = 0; a < kWgradAcc; ++a) rs[a][tid] += rs[a][tid + h * G];
      }
      __syncthreads();
    }
    if (pl == 0) {
      float* out =
          &part[((long)blockIdx.x * N + gi * 8 + j) * kWgradAcc];
#pragma unroll
      for (int a = 0; a < kWgradAcc; ++a) out[a] = rs[a][tid];
    }
    __syncthreads();
  }
}

// Reduce the chunk partials: one wave per output (k, tap), each lane
// sums chunks lane, lane + 64, ... ascending, then a fixed halving tree
// over the 64 lanes; one rounding to bf16. Tap 9 is the bias gradient.
__global__ __launch_bounds__(256) void thin_conv_pool_wgrad_final_kernel(
    const float* __restrict__ part, int chunks, int N,
    bf16* __restrict__ dw, bf16* __restrict__ db) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int o = blockIdx.x * 4 + wv;  // k * 10 + tap
  const int total = N * kWgradAcc;
  float v = 0.f;
  if (o < total)
    for (int c = lane; c < chunks; c += 64) v += part[(long)c * total + o];
  __shared__ float rs[4][64];
  rs[wv][lane] = v;
  __syncthreads();
  for (int h = 32; h > 0; h >>= 1) {
    if (lane < h) rs[wv][lane] += rs[wv][lane + h];
    __syncthreads();
  }
  if (lane == 0 && o < total) {
    const int k = o / kWgradAcc, a = o % kWgradAcc;
    if (a < 9) dw[k * 9 + a] = f2b(rs[wv][0]);
    else db[k] = f2b(rs[wv][0]);
  }
}

// ---- order-preserving fused wgrad of the thin pooled first layer ----
// The materialised chain computes dWp[Kout, 16] = dyfull^T @ col with
// gemm_kernel<32,32,2,1,true,false>: per K slice and per 16-row
// fragment of Kout one chain of mfma_f32_16x16x32_bf16 over 32 pixels a
// step, then the fixed-order split-K reduce. dW's bits are fixed by the
// operand values of each MFMA, their order within a slice and the
// reduce — not by where the operands came from. This kernel issues the
// same chain per (slice, fragment) with operands built in registers:
//   A[kout][k]: the masked unpooled gradient at full-resolution pixel k,
//     by the expression pool_relu_bwd_colsum_part_kernel stores;
//   B[k][t]:    x at tap t of pixel k (im2col's row), +0 out of range
//     and for t >= 9; both +0 past the slice end.
// so neither the full-resolution plane nor the col matrix exists.
// One block per slice. A chain is serial, but building its operands is
// not, and that (VALU issue and 2-byte gathers) is the whole cost: Q
// waves per fragment each build the operands of CH consecutive k-steps
// into registers at once, then take turns, in step order, issuing their
// MFMAs on the one accumulator, which passes through LDS (an exact
// copy) with a barrier per turn — Q barriers per Q * CH steps, none per
// step. The build is branch-free:
//   - the slice's x rows are staged once into LDS as a ZERO-PADDED image
//     (rows oh + r of H + 2 pad, columns ow + s of OW + 2), so a tap is
//     an unconditional read at a lane-constant offset from its pixel;
//   - a table of the slice's pixel PAIRS (OW is even, so two adjacent
//     pixels share a pooled pixel) is decoded once into LDS: pooled
//     pixel index, LDS offset of the pair in the padded image, row
//     parity. Entries past the slice end point at a zero cell and carry
//     an argmax code no window has, so the tail needs no test;
//   - the pooled tensors are gathered straight into the A-fragment
//     layout (lane = channel, 8 consecutive pixels = 4 pairs), the loads
//     of the next PF steps already in flight.

// Rows [P0, P0 + rows) of the padded image stack (image n, padded row
// pr <-> n * (OH + 2) + pr) that pixels [k_begin, k_end) read. Host (LDS
// sizing) and device share it.
BFLC_HD inline void thin_wgrad_window(const ConvShape& sh, long k_begin,
                                      long k_end, int* P0, int* rows) {
  const long ohw = (long)sh.OH * sh.OW;
  const long n0 = k_begin / ohw, n1 = (k_end - 1) / ohw;
  const long oh0 = (k_begin - n0 * ohw) / sh.OW;
  const long oh1 = (k_end - 1 - n1 * ohw) / sh.OW;
  *P0 = (int)(n0 * (sh.OH + 2) + oh0);
  *rows = (int)(n1 * (sh.OH + 2) + oh1 + 2) - *P0 + 1;
}

constexpr int kThinFusedPF = 2;  // k-steps of pooled loads in flight
constexpr int kThinFusedCH = 6;  // k-steps a wave builds per round
constexpr long kThinFusedMaxLds = 60 * 1024;  // dynamic; + 4 KB static <= 64 KB

struct PooledRaw {
  unsigned short dy[4], y[4];
  uint8_t id[4];
  int code[4];       // argmax code of the pair's even pixel
  unsigned xpair[4];  // the pair's two x values at this lane's tap
};

constexpr int kNoCode = 8;  // matches no argmax code (0..3), +1 included

template <int Q>
__global__ __launch_bounds__(512) void thin_pool_wgrad_mfma_kernel(
    const unsigned short* __restrict__ X,
    const unsigned short* __restrict__ yp, const uint8_t* __restrict__ idx,
    const unsigned short* __restrict__ dyp, ConvShape sh, long Mpix,
    long kslice, int cshift, int tbl_pairs, float* __restrict__ part,
    bf16* __restrict__ dw) {
  // [tbl_pairs] int2 pair table, then the padded x rows
  extern __shared__ __align__(16) int lds[];
  int2* tbl = reinterpret_cast<int2*>(lds);
  unsigned short* xs = reinterpret_cast<unsigned short*>(lds + 2 * tbl_pairs);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave-uniform by construction; say so, so that the turns below are
  // scalar branches and no MFMA ever sits under an EXEC mask
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frag = wave / Q, wq = wave % Q;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int OH = sh.OH, PW = sh.OW >> 1, PH = sh.OH >> 1;
  const int WP = sh.OW + 2, OHP = sh.OH + 2;
  const int Kout = sh.Kout;
  const long k_begin = (long)blockIdx.x * kslice;
  const long k_end = min(Mpix, k_begin + kslice);
  const int npairs = (int)((k_end - k_begin) >> 1);  // both are even
  const int nsteps = (int)((k_end - k_begin + 31) >> 5);

  int P0, rows;
  thin_wgrad_window(sh, k_begin, k_end, &P0, &rows);
  // zero cells after the window: an invalid pair points here, and every
  // tap offset (< 2 * WP + 4) from it still reads +0
  const int zcell = rows * WP;

  // ---- pair table ----
  {
    const unsigned q0 = (unsigned)(k_begin >> 1);
    for (int i = tid; i < tbl_pairs; i += (int)blockDim.x) {
      int2 e = {0, zcell | (kNoCode << 16)};
      if (i < npairs) {
        const unsigned q = q0 + i;
        const unsigned row = q / (unsigned)PW;
        const unsigned n = row / (unsigned)OH;
        const int pw = (int)(q - row * PW), oh = (int)(row - n * OH);
        e.x = ((int)n * PH + (oh >> 1)) * PW + pw;
        e.y = (((int)n * OHP + oh - P0) * WP + 2 * pw) |
              (((oh & 1) * 2) << 16);
      }
      tbl[i] = e;
    }
  }
  // ---- stage the slice's padded x rows: CW columns x RPP rows a pass,
  // four passes of loads in flight ----
  {
    const int CW = 1 << cshift;  // <= 64 <= blockDim.x
    const int RPP = (int)blockDim.x >> cshift;
    const int col = tid & (CW - 1);
    int j = tid >> cshift;
    int n = (P0 + j) / OHP, pr = (P0 + j) - n * OHP;
    const int rwraps = (RPP + OHP - 1) / OHP;
    while (j < rows) {
      unsigned short v[4];
      int dst[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ih = pr - sh.pad;
        const bool rok = j < rows && ih >= 0 && ih < sh.H;
        dst[u] = j < rows ? j * WP : -1;
        const int iw = col - sh.pad;
        const bool ok = rok && col < WP && iw >= 0 && iw < sh.W;
        const unsigned short raw = X[ok ? (n * sh.H + ih) * sh.W + iw : 0];
        v[u] = ok ? raw : (unsigned short)0;
        // columns beyond CW (OW > 62) are walked here, one at a time
        for (int c = col + CW; c < WP; c += CW) {
          const int iwc = c - sh.pad;
          const bool okc = rok && iwc >= 0 && iwc < sh.W;
          const unsigned short rc =
              X[okc ? (n * sh.H + ih) * sh.W + iwc : 0];
          if (dst[u] >= 0) xs[dst[u] + c] = okc ? rc : (unsigned short)0;
        }
        j += RPP;
        pr += RPP;
        for (int t = 0; t < rwraps; ++t) {
          const bool w = pr >= OHP;
          pr -= w ? OHP : 0;
          n += w ? 1 : 0;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (dst[u] >= 0 && col < WP) xs[dst[u] + col] = v[u];
    }
    for (int z = tid; z < 2 * WP + 4; z += (int)blockDim.x) xs[zcell + z] = 0;
  }
  __syncthreads();

  const int ch = frag * 16 + l15;  // A row: output channel
  const int chc = ch < Kout ? ch : 0;
  const int cadd = ch < Kout ? 0 : kNoCode;   // rows >= Kout stay +0
  const int tr = l15 / 3, ts = l15 - tr * 3;  // B column: tap (r, s)
  const bool tap_ok = l15 < 9;                // columns >= 9 stay +0
  const int tbase = tr * WP + ts;

  // this lane's four pairs of k-step `st`; steps past the slice read
  // the all-invalid table row after it
  auto load_step = [&](PooledRaw& raw, int st) {
    st = min(st, nsteps);
    const int4* t = reinterpret_cast<const int4*>(&tbl[st * 16 + l4 * 4]);
    const int4 e01 = t[0], e23 = t[1];
    const int po[4] = {e01.x, e01.z, e23.x, e23.z};
    const int xc[4] = {e01.y, e01.w, e23.y, e23.w};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const unsigned o = (unsigned)(po[jj] * Kout + chc);
      raw.dy[jj] = dyp[o];
      raw.y[jj] = yp[o];
      raw.id[jj] = idx[o];
      raw.code[jj] = (xc[jj] >> 16) + cadd;
      const int xa = tap_ok ? (xc[jj] & 0xffff) + tbase : zcell;
      raw.xpair[jj] = (unsigned)xs[xa] | ((unsigned)xs[xa + 1] << 16);
    }
  };

  constexpr int PF = kThinFusedPF, CH = kThinFusedCH;
  __shared__ f32x4_t accs[4][64];  // the accumulator between turns
  const bf16 zero = f2b(0.f);
  f32x4_t acc = {};
  for (int base = 0; base < nsteps; base += Q * CH) {
    const int my0 = base + wq * CH;
    // ---- build this wave's CH steps ----
    u16x8_t av[CH], bv[CH];
    PooledRaw raw[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) load_step(raw[i], my0 + i);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const PooledRaw& rw = raw[i % PF];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float dyf = __uint_as_float((unsigned)rw.dy[jj] << 16);
        const float yf = __uint_as_float((unsigned)rw.y[jj] << 16);
        bv[i][jj * 2] = (unsigned short)(rw.xpair[jj] & 0xffff);
        bv[i][jj * 2 + 1] = (unsigned short)(rw.xpair[jj] >> 16);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int code = rw.code[jj] + p;
          float a = 0.f;
          if ((int)rw.id[jj] == code) a += dyf;
          bf16 gv = f2b(a);
          if (!(yf > 0.f)) gv = zero;
          av[i][jj * 2 + p] = __builtin_bit_cast(unsigned short, gv);
        }
      }
      if (i + PF < CH) load_step(raw[i % PF], my0 + i + PF);
    }
    // ---- the chain, in step order: one turn per wave ----
#pragma unroll
    for (int t = 0; t < Q; ++t) {
      if (wq == t && my0 < nsteps) {  // wave-uniform
        if (my0 > 0) acc = accs[frag][lane];
#pragma unroll
        for (int i = 0; i < CH; ++i)
          if (my0 + i < nsteps)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8_t, av[i]),
                __builtin_bit_cast(bf16x8_t, bv[i]), acc, 0, 0, 0);
        accs[frag][lane] = acc;
      }
      __syncthreads();
    }
  }
  if (wq != 0) return;
  acc = accs[frag][lane];  // the last turn's, whichever wave took it

  // D: lane holds rows l4 * 4 + r of the fragment, column l15 (= tap)
  if (l15 < 9) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = frag * 16 + l4 * 4 + r;
      if (row >= Kout) continue;
      if (part)
        part[((long)blockIdx.x * Kout + row) * 9 + l15] = acc[r];
      else  // single slice: the GEMM epilogue's store with a null bias
        dw[row * 9 + l15] = f2b(acc[r] + 0.f);
    }
  }
}

inline int ew_grid(long n) {
  return (int)std::min<long>((n + 255) / 256, 16384);
}

ConvShape make_shape(const torch::Tensor& x, const torch::Tensor& w,
                     long stride, long pad) {
  ConvShape sh;
  sh.N = (int)x.size(0); sh.H = (int)x.size(1);
  sh.W = (int)x.size(2); sh.C = (int)x.size(3);
  sh.Kout = (int)w.size(0); sh.R = (int)w.size(1); sh.S = (int)w.size(2);
  sh.stride = (int)stride; sh.pad = (int)pad;
  sh.OH = (sh.H + 2 * sh.pad - sh.R) / sh.stride + 1;
  sh.OW = (sh.W + 2 * sh.pad - sh.S) / sh.stride + 1;
  TORCH_CHECK(w.size(3) == sh.C, "conv channel mismatch (NHWC x, KRSC w)");
  return sh;
}

// When C % 8 != 0 (FEMNIST C=1, ResNet stems C=3) the col matrix's K
// is zero-padded to a multiple of 8 so the consuming GEMM takes the
// 16-B vector staging paths (the K=9 FEMNIST conv1 GEMM ran scalar
// staging at ~6 TF); the padded columns contribute zeros and the
// weight is padded to match by the callers.
torch::Tensor im2col(const torch::Tensor& x, const ConvShape& sh) {
  if (sh.C % 8 == 0) {
    auto col = torch::empty({sh.M(), sh.RSC()}, x.options());
    const long total_g = sh.M() * sh.R * sh.S * (sh.C / 8);
    hipLaunchKernelGGL(im2col_nhwc_vec_kernel, dim3(ew_grid(total_g)),
                       dim3(256), 0, cur_stream(),
                       (const bf16*)x.data_ptr(), (bf16*)col.data_ptr(), sh,
                       total_g);
    HIP_CHECK(hipGetLastError());
    return col;
  }
  const long rscp = (sh.RSC() + 7) / 8 * 8;
  auto col = torch::empty({sh.M(), rscp}, x.options());
  if (rscp <= 32) {
    const long total_m = sh.M();
    hipLaunchKernelGGL(im2col_nhwc_rowvec_kernel, dim3(ew_grid(total_m)),
                       dim3(256), 0, cur_stream(),
                       (const bf16*)x.data_ptr(), (bf16*)col.data_ptr(), sh,
                       rscp, total_m);
  } else {
    const long total_g = sh.M() * (rscp / 8);
    hipLaunchKernelGGL(im2col_nhwc_gran_kernel, dim3(ew_grid(total_g)),
                       dim3(256), 0, cur_stream(),
                       (const bf16*)x.data_ptr(), (bf16*)col.data_ptr(), sh,
                       rscp, total_g);
  }
  HIP_CHECK(hipGetLastError());
  return col;
}

// Zero-pad the [Kout, RSC] weight view to the (padded) col K.
torch::Tensor pad_w2(const torch::Tensor& w2, long kp) {
  if (kp == w2.size(1)) return w2;
  auto out = torch::zeros({w2.size(0), kp}, w2.options());
  out.slice(1, 0, w2.size(1)).copy_(w2);
  return out;
}

bool is_1x1_s1(const ConvShape& sh) {
  return sh.R == 1 && sh.S == 1 && sh.stride == 1 && sh.pad == 0;
}

// Measured implicit-vs-materialized crossovers, overridable for A/B
// profiling runs without a rebuild.
int env_gate(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
int wgrad_implicit_max_kout() {
  static int v = env_gate("BFLC_WGRAD_IMPLICIT_MAX_KOUT", 64);
  return v;
}
int dgrad_implicit_max_c() {
  static int v = env_gate("BFLC_DGRAD_IMPLICIT_MAX_C", 128);
  return v;
}

}  // namespace

// Returns (y, col) so the autograd wrapper hands col back to wgrad
// (recomputing im2col cost ~12% of an FL round; 288 GB HBM3E makes the
// cache free). For 1x1 stride-1 convs col is just a VIEW of x.
std::tuple<torch::Tensor, torch::Tensor> conv2d_fwd_col(
    torch::Tensor x, torch::Tensor w, torch::Tensor b, long stride,
    long pad, bool relu, bool want_col) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_CONTIG(w);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "conv: bf16 only");
  auto sh = make_shape(x, w, stride, pad);
  auto w2 = w.view({(long)sh.Kout, sh.RSC()});
  auto bc = b.contiguous();
  auto y = torch::empty({(long)sh.N, (long)sh.OH, (long)sh.OW,
                         (long)sh.Kout}, x.options());
  if (is_1x1_s1(sh)) {
    auto col = x.view({sh.M(), (long)sh.C});
    gemm_bf16_raw(col, w2, y, sh.M(), sh.Kout, sh.RSC(), false, true, &bc,
                  relu, EpStore::kPlain, 0);
    return {y, col};
  }
  // implicit-GEMM: the im2col gather runs inside the GEMM's A staging;
  // no col matrix exists (wgrad materializes its own in the backward).
  if (gemm_conv_fwd_raw(x, w2, y, sh, &bc, relu))
    return {y, torch::empty({0}, x.options())};
  const long kp = (sh.RSC() + 7) / 8 * 8;
  // grad-free forward (committee scoring): nobody reads col back, so
  // thin shapes gather the window inside the GEMM instead of paying
  // the im2col write + re-read (bitwise-identical output). RSC <= 16
  // only: at 27 scalar taps (CIFAR stem) the per-row gather costs more
  // than the col round trip it saves (A/B: stem eval 53 -> 66 us,
  // FEMNIST conv1 9 taps 50.7 -> 35.4 us).
  if (!want_col && sh.RSC() <= 16 && kp <= 32) {
    auto w2p = pad_w2(w2, kp);
    if (gemm_thin_conv_raw(x, w2p, y, sh, &bc, relu))
      return {y, torch::empty({0}, x.options())};
  }
  auto col = im2col(x, sh);
  TORCH_CHECK(col.size(1) == kp);
  gemm_bf16_raw(col, pad_w2(w2, kp), y, sh.M(), sh.Kout, kp, false, true,
                &bc, relu, EpStore::kPlain, 0);
  return {y, col};
}

torch::Tensor conv2d_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                         long stride, long pad, bool relu) {
  // inference entry: no col wanted
  return std::get<0>(conv2d_fwd_col(x, w, b, stride, pad, relu, false));
}

// Conv forward WITH fused per-tile BN stats from the GEMM epilogue:
// (y, col, psum, psq). col / psum / psq may be 0-size when that piece
// was not produced (materialized-col fallback keeps col; split-K or
// unsupported shapes leave the stats empty and the caller runs the
// standalone stats pass).
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
conv2d_fwd_bn(torch::Tensor x, torch::Tensor w, long stride, long pad) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_CONTIG(w);
  auto sh = make_shape(x, w, stride, pad);
  auto w2 = w.view({(long)sh.Kout, sh.RSC()});
  auto y = torch::empty({(long)sh.N, (long)sh.OH, (long)sh.OW,
                         (long)sh.Kout}, x.options());
  std::pair<torch::Tensor, torch::Tensor> stats;
  auto none = torch::empty({0}, x.options());
  // BN consumes the conv output unbiased: nullptr bias (a zeros tensor
  // here cost a tiny fill launch per conv per step)
  if (is_1x1_s1(sh)) {
    auto col = x.view({sh.M(), (long)sh.C});
    gemm_bf16_raw(col, w2, y, sh.M(), sh.Kout, sh.RSC(), false, true,
                  nullptr, false, EpStore::kPlain, 0, &stats);
    return {y, col, stats.first.defined() ? stats.first : none,
            stats.second.defined() ? stats.second : none};
  }
  if (gemm_conv_fwd_raw(x, w2, y, sh, nullptr, false, &stats))
    return {y, none, stats.first.defined() ? stats.first : none,
            stats.second.defined() ? stats.second : none};
  auto col = im2col(x, sh);
  const long kp = col.size(1);
  gemm_bf16_raw(col, pad_w2(w2, kp), y, sh.M(), sh.Kout, kp, false, true,
                nullptr, false, EpStore::kPlain, 0, &stats);
  return {y, col, stats.first.defined() ? stats.first : none,
          stats.second.defined() ? stats.second : none};
}

namespace {

// The two halves of conv2d_bwd, so that a caller with its own data
// gradient (the halo route of the pooled backward) runs the weight
// gradient alone through the same routing.
torch::Tensor conv_dgrad(const torch::Tensor& x, const torch::Tensor& w,
                         const torch::Tensor& dy2, const ConvShape& sh,
                         bool want_dx) {
  auto w2 = w.view({(long)sh.Kout, sh.RSC()});
  // dgrad. want_dx=false (first-layer convs: the input is data, not an
  // activation) skips the whole dgrad GEMM + col2im — on the ResNet-50
  // stem that is a dcol of M x 147 (~236 MB) plus its col2im pass,
  // computed for a gradient every model threw away.
  torch::Tensor dx;
  bool dgrad_done = !want_dx;
  if (!want_dx) {
    dx = torch::empty({0}, x.options());
  } else if (is_1x1_s1(sh)) {
    auto wT = transpose_bf16(w2);  // [C, Kout]
    dx = torch::empty_like(x);
    auto dxv = dx.view({sh.M(), (long)sh.C});
    gemm_bf16_raw(dy2, wT, dxv, sh.M(), sh.RSC(), sh.Kout, false, true,
                  nullptr, false, EpStore::kPlain, 0);
    dgrad_done = true;
  } else if (sh.Kout % 8 == 0 && sh.C <= dgrad_implicit_max_c() &&
             sh.C >= 8 && sh.stride == 1) {
    // (stride > 1 wastes stride^2 of the implicit MFMA work on
    // misaligned taps — the 7x7/2 stem forced implicit cost +17% of a
    // ResNet-50 round; tiny C additionally wastes the N tile)
    // implicit: dx[M, C] = dy-gather @ w.permute(3,1,2,0) — no dcol
    // matrix, no col2im pass. Only while C is small-to-mid: there the
    // dcol round trip dominates (R*S*C columns vs C outputs); at
    // large C the materialized dcol GEMM runs on the faster
    // 8-phase/dbuf path and wins (A/B on ResNet-50: C<=128 86.9
    // ms/round, C<=256 87.9, forced always +20%).
    auto wrot2 = w.permute({3, 1, 2, 0}).contiguous()
                     .view({(long)sh.C, (long)sh.R * sh.S * sh.Kout});
    dx = torch::empty_like(x);
    auto dxv = dx.view({(long)sh.N * sh.H * sh.W, (long)sh.C});
    dgrad_done = gemm_conv_dgrad_raw(dy2, wrot2, dxv, sh);
  }
  if (!dgrad_done) {
    auto wT = transpose_bf16(w2);  // [RSC, Kout]
    auto dcol = torch::empty({sh.M(), sh.RSC()}, x.options());
    gemm_bf16_raw(dy2, wT, dcol, sh.M(), sh.RSC(), sh.Kout, false, true,
                  nullptr, false, EpStore::kPlain, 0);
    dx = torch::empty_like(x);
    if (sh.C % 8 == 0) {
      const long total_g = (long)sh.N * sh.H * sh.W * (sh.C / 8);
      hipLaunchKernelGGL(col2im_nhwc_vec_kernel, dim3(ew_grid(total_g)),
                         dim3(256), 0, cur_stream(),
                         (const bf16*)dcol.data_ptr(),
                         (bf16*)dx.data_ptr(), sh, total_g);
    } else {
      const long total = dx.numel();
      hipLaunchKernelGGL(col2im_nhwc_kernel, dim3(ew_grid(total)), dim3(256),
                         0, cur_stream(), (const bf16*)dcol.data_ptr(),
                         (bf16*)dx.data_ptr(), sh, total);
    }
    HIP_CHECK(hipGetLastError());
  }
  return dx;
}

torch::Tensor conv_wgrad(const torch::Tensor& x, const torch::Tensor& w,
                         const torch::Tensor& dy2, const ConvShape& sh,
                         const c10::optional<torch::Tensor>& col_cache) {
  auto w2 = w.view({(long)sh.Kout, sh.RSC()});
  // wgrad: dW[Kout, RSC] = dy2^T @ col. Implicit (col gathered from x
  // inside the GEMM staging) when C % 8 == 0; else a materialized col
  // (reused from the fwd when it produced one).
  auto dw = torch::empty_like(w2);
  bool wgrad_done = false;
  // implicit only when the col round trip would dominate: the wgrad
  // GEMM does Kout flops per col element, so small Kout => col-bound
  // (measured: implicit at Kout>=128 ran 150us/call, slower than the
  // materialized dbuf path it replaced)
  if (!is_1x1_s1(sh) && sh.Kout <= wgrad_implicit_max_kout() &&
      !(col_cache.has_value() && col_cache->numel() > 0))
    wgrad_done = gemm_conv_wgrad_raw(dy2, x, dw, sh);
  if (!wgrad_done) {
    auto col = (col_cache.has_value() && col_cache->numel() > 0)
                   ? *col_cache
                   : (is_1x1_s1(sh) ? x.view({sh.M(), (long)sh.C})
                                    : im2col(x, sh));
    const long kp = col.size(1);
    if (kp == sh.RSC()) {
      gemm_bf16_raw(dy2, col, dw, sh.Kout, sh.RSC(), sh.M(), true, false,
                    nullptr, false, EpStore::kPlain, 0);
    } else {  // K-padded col: compute into [Kout, kp], narrow back
      auto dwp = torch::empty({(long)sh.Kout, kp}, dw.options());
      gemm_bf16_raw(dy2, col, dwp, sh.Kout, kp, sh.M(), true, false,
                    nullptr, false, EpStore::kPlain, 0);
      dw.copy_(dwp.slice(1, 0, sh.RSC()));
    }
  }
  return dw.view(w.sizes());
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> conv2d_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor dy, long stride,
    long pad, c10::optional<torch::Tensor> col_cache, bool want_db,
    bool want_dx) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_CONTIG(w); CHECK_CONTIG(dy);
  auto sh = make_shape(x, w, stride, pad);
  auto dy2 = dy.view({sh.M(), (long)sh.Kout});  // NHWC: free view
  auto dx = conv_dgrad(x, w, dy2, sh, want_dx);
  auto dw = conv_wgrad(x, w, dy2, sh, col_cache);

  // db only when the layer HAS a bias: the conv+BN blocks (every
  // ResNet conv) discard it, and colsum was ~3.3% of a ResNet-20 round
  // spent re-reading all of dy for a dead value
  auto db = want_db ? colsum_bf16(dy2)
                    : torch::empty({0}, dy.options());
  return {dx, dw, db};
}

std::tuple<torch::Tensor, torch::Tensor> maxpool2d_fwd(torch::Tensor x,
                                                       long kernel,
                                                       long stride,
                                                       bool want_idx) {
  CHECK_GPU(x); CHECK_CONTIG(x);
  ConvShape sh;
  sh.N = (int)x.size(0); sh.H = (int)x.size(1);
  sh.W = (int)x.size(2); sh.C = (int)x.size(3);
  sh.R = sh.S = (int)kernel; sh.stride = (int)stride; sh.pad = 0;
  sh.Kout = sh.C;
  sh.OH = (sh.H - sh.R) / sh.stride + 1;
  sh.OW = (sh.W - sh.S) / sh.stride + 1;
  auto y = torch::empty({(long)sh.N, (long)sh.OH, (long)sh.OW, (long)sh.C},
                        x.options());
  TORCH_CHECK(sh.R * sh.S <= 255, "maxpool window too large for u8 idx");
  // grad-free forwards (committee scoring) never read the argmax mask:
  // skip both its allocation and its write (vec path only; the C%8!=0
  // scalar path is not on any model's hot shape)
  const bool skip_idx = !want_idx && sh.C % 8 == 0;
  auto idx = skip_idx
                 ? torch::empty({0}, y.options().dtype(at::kByte))
                 : torch::empty_like(y, y.options().dtype(at::kByte));
  if (sh.C % 8 == 0) {
    const long total_g = sh.M() * (sh.C / 8);
    hipLaunchKernelGGL(maxpool_nhwc_vec_fwd, dim3(ew_grid(total_g)),
                       dim3(256), 0, cur_stream(),
                       (const bf16*)x.data_ptr(), (bf16*)y.data_ptr(),
                       skip_idx ? nullptr : idx.data_ptr<uint8_t>(), sh,
                       total_g);
  } else {
    const long total = y.numel();
    hipLaunchKernelGGL(maxpool_nhwc_fwd, dim3(ew_grid(total)), dim3(256), 0,
                       cur_stream(), (const bf16*)x.data_ptr(),
                       (bf16*)y.data_ptr(), idx.data_ptr<uint8_t>(), sh,
                       total);
  }
  HIP_CHECK(hipGetLastError());
  return {y, idx};
}

// ---- grad-free conv + bias + ReLU + 2x2/stride-2 maxpool ----
// Committee scoring pushes 4x the training sample volume through the
// conv stack and never needs the full-resolution activation, which the
// two-kernel form writes to HBM only for the pool to read back and keep
// one value in four. The fused routes pool in the conv epilogue; bias
// add, ReLU and the fp32->bf16 rounding are all monotone, so
// max(round(relu(v_i))) == round(relu(max(v_i))) and the result is
// bitwise the two-kernel one. Shapes no fused kernel takes run conv
// then pool right here, so the entry is always correct.
namespace {

enum class PoolRoute { kUnfused, kGemm256, kThin };

PoolRoute pool_route(const ConvShape& sh) {
  if (is_1x1_s1(sh)) return PoolRoute::kUnfused;
  if (gemm_conv_fwd_pool_eligible(sh)) return PoolRoute::kGemm256;
  if (gemm_thin_conv_pool_eligible(sh)) return PoolRoute::kThin;
  return PoolRoute::kUnfused;
}

ConvShape make_shape_dims(std::vector<long> xs, std::vector<long> ws,
                          long stride, long pad) {
  TORCH_CHECK(xs.size() == 4 && ws.size() == 4, "NHWC x, KRSC w");
  ConvShape sh;
  sh.N = (int)xs[0]; sh.H = (int)xs[1]; sh.W = (int)xs[2]; sh.C = (int)xs[3];
  sh.Kout = (int)ws[0]; sh.R = (int)ws[1]; sh.S = (int)ws[2];
  sh.stride = (int)stride; sh.pad = (int)pad;
  sh.OH = (sh.H + 2 * sh.pad - sh.R) / sh.stride + 1;
  sh.OW = (sh.W + 2 * sh.pad - sh.S) / sh.stride + 1;
  return sh;
}

}  // namespace

// Plan of an implicit-GEMM conv entry ("fwd", "fwd_pool", "dgrad",
// "wgrad") for these shapes: (path, bm, bn, S, kslice).
PlanRow conv_plan_route(const std::string& entry, std::vector<long> x_shape,
                        std::vector<long> w_shape, long stride, long pad) {
  const ConvEntry e = entry == "fwd"        ? ConvEntry::kFwd
                      : entry == "fwd_pool" ? ConvEntry::kFwdPool
                      : entry == "dgrad"    ? ConvEntry::kDgrad
                                            : ConvEntry::kWgrad;
  TORCH_CHECK(e != ConvEntry::kWgrad || entry == "wgrad",
              "conv_plan_route: entry is fwd | fwd_pool | dgrad | wgrad");
  return plan_row(
      gemm_conv_plan(e, make_shape_dims(x_shape, w_shape, stride, pad)));
}

// Name of the route conv2d_relu_pool_fwd takes for these shapes, so a
// test cannot pass silently through the fallback.
std::string conv2d_relu_pool_route(std::vector<long> x_shape,
                                   std::vector<long> w_shape, long stride,
                                   long pad) {
  switch (pool_route(make_shape_dims(x_shape, w_shape, stride, pad))) {
    case PoolRoute::kGemm256: return "gemm256_pool";
    case PoolRoute::kThin: return "thin_pool";
    default: return "unfused";
  }
}

namespace {

// (y_pooled, idx); idx is 0-size unless want_idx. Scoring passes
// want_idx = false and runs exactly the kernels it ran before.
std::tuple<torch::Tensor, torch::Tensor> relu_pool_fwd_impl(
    const torch::Tensor& x, const torch::Tensor& w, const torch::Tensor& b,
    long stride, long pad, bool want_idx, long max_blocks = 0,
    const std::string& impl = "") {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_CONTIG(w);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "conv: bf16 only");
  auto sh = make_shape(x, w, stride, pad);
  // impl: "" = what conv_fwd_pool_impl reports; "gemm256" / "halo_mfma"
  // pin one side of the conv2 pooled forward (tests, op benchmark)
  TORCH_CHECK(impl.empty() || impl == "gemm256" || impl == "halo_mfma",
              "conv2d_relu_pool: impl is '' | gemm256 | halo_mfma");
  const HaloMode halo = impl.empty()        ? HaloMode::kAuto
                        : impl == "gemm256" ? HaloMode::kOff
                                            : HaloMode::kForce;
  TORCH_CHECK(halo != HaloMode::kForce || halo_conv_geometry_ok(sh),
              "conv2d_relu_pool: shape outside the halo kernel's geometry");
  const PoolRoute route =
      halo == HaloMode::kForce ? PoolRoute::kGemm256 : pool_route(sh);
  if (route != PoolRoute::kUnfused) {
    auto w2 = w.view({(long)sh.Kout, sh.RSC()});
    auto bc = b.contiguous();
    auto y = torch::empty({(long)sh.N, (long)sh.OH / 2, (long)sh.OW / 2,
                           (long)sh.Kout}, x.options());
    auto idx = want_idx
                   ? torch::empty_like(y, y.options().dtype(at::kByte))
                   : torch::empty({0}, y.options().dtype(at::kByte));
    uint8_t* ip = want_idx ? idx.data_ptr<uint8_t>() : nullptr;
    const bool done =
        route == PoolRoute::kGemm256
            ? gemm_conv_fwd_pool_raw(x, w2, y, sh, &bc, true, ip, halo,
                                     (int)max_blocks)
            : gemm_thin_conv_pool_raw(x, w2, y, sh, &bc, true, ip);
    TORCH_CHECK(done, "conv2d_relu_pool: route query and launcher disagree");
    return {y, idx};
  }
  auto y = conv2d_fwd(x, w, b, stride, pad, true);
  return maxpool2d_fwd(y, 2, 2, want_idx);
}

// Geometry thin_conv_pool_wgrad unrolls: the thin pooled forward's,
// with no minimum-rows gate (the direct kernel has no GEMM to fall
// back to a better tile for).
bool thin_wgrad_eligible(const ConvShape& sh) {
  return sh.R == 3 && sh.S == 3 && sh.C == 1 && sh.stride == 1 &&
         sh.OH > 0 && sh.OW > 0 && sh.OH % 2 == 0 && sh.OW % 2 == 0 &&
         sh.Kout <= 64 && sh.Kout % 8 == 0;
}

void check_pooled(const torch::Tensor& y, const torch::Tensor& idx,
                  const torch::Tensor& dy) {
  CHECK_GPU(y); CHECK_GPU(idx); CHECK_GPU(dy);
  CHECK_CONTIG(y); CHECK_CONTIG(idx); CHECK_CONTIG(dy);
  TORCH_CHECK(y.scalar_type() == at::kBFloat16 &&
              dy.scalar_type() == at::kBFloat16 &&
              idx.scalar_type() == at::kByte,
              "pooled backward: bf16 y/dy and u8 idx");
  TORCH_CHECK(y.dim() == 4 && y.sizes() == dy.sizes() &&
              y.sizes() == idx.sizes(),
              "pooled backward: y, idx, dy must share one NHWC shape");
}

// BFLC_THIN_FUSED_WGRAD: 1 (default) routes the thin first layer's
// default backward through the order-preserving fused kernel, 0 keeps
// the materialised chain (A/B runs; the results are bitwise the same).
bool thin_fused_wgrad_gate() {
  static const bool v = env_gate("BFLC_THIN_FUSED_WGRAD", 1) != 0;
  return v;
}

// The slices of the materialised chain's GEMM, dWp[Kout, 16] over K =
// Mpix, and whether the fused kernel can stand in for it: the plan must
// be the small-tile kernel's (whose chain the fused kernel issues) and
// every slice's pair table and padded x rows must fit the LDS budget.
struct ThinFusedPlan {
  bool ok = false;
  long S = 1, kslice = 0;
  int tbl_pairs = 0;  // pair-table entries: a slice + one all-invalid step
  long lds = 0;       // LDS bytes: table + tallest window + zero cells
  int cshift = 0;     // staging columns per pass = 1 << cshift (<= 64)
};

ThinFusedPlan thin_fused_plan(const ConvShape& sh) {
  ThinFusedPlan t;
  if (!thin_wgrad_eligible(sh) || sh.N <= 0) return t;
  const long Mpix = sh.M();
  const long kp = (sh.RSC() + 7) / 8 * 8;
  const GemmPlan p = gemm_dense_plan(sh.Kout, kp, Mpix, true, false);
  // the kernel indexes x, the pooled tensors and its rows in 32 bits
  const long lim = 1L << 31;
  if (p.path != GemmPath::kSmall || kp != 16 || Mpix * sh.Kout >= lim ||
      (long)sh.N * sh.H * sh.W >= lim || (long)sh.N * (sh.OH + 2) >= lim)
    return t;
  t.S = p.S;
  t.kslice = p.kslice;
  int rows_max = 0;
  for (long s = 0; s < p.S; ++s) {
    int P0, rows;
    thin_wgrad_window(sh, s * p.kslice,
                      std::min(Mpix, (s + 1) * p.kslice), &P0, &rows);
    rows_max = std::max(rows_max, rows);
  }
  const long xelems = (long)(rows_max + 2) * (sh.OW + 2) + 4;
  const long pairs = (p.kslice / 32 + 1) * 16;  // + one all-invalid step
  t.tbl_pairs = (int)pairs;
  t.lds = pairs * 8 + (xelems + 1) / 2 * 4;
  while (t.cshift < 6 && (1 << t.cshift) < sh.OW + 2) ++t.cshift;
  // the x offset shares a table word with the row parity (16 bits)
  t.ok = t.lds <= kThinFusedMaxLds && xelems <= 32768;
  return t;
}

// db of the pooled backward alone: pool_relu_bwd_colsum's rows, chunks
// and trees with the plane store left out (the pass
// thin_conv_pool_wgrad_fused ends with), so db keeps its bits.
torch::Tensor pool_relu_bwd_db(const torch::Tensor& y_pooled,
                               const torch::Tensor& idx,
                               const torch::Tensor& dy_pooled,
                               const ConvShape& sh) {
  const long Mpix = sh.M();
  const long N = sh.Kout;
  TORCH_CHECK(Mpix * N < (1L << 31), "pool_relu_bwd_db: 32-bit indices");
  auto db = torch::empty({N}, dy_pooled.options());
  const ColsumGeom g = colsum_geom(Mpix, N);  // pool_relu_bwd_colsum's
  auto cpart = torch::empty({g.chunks, N},
                            dy_pooled.options().dtype(at::kFloat));
  hipLaunchKernelGGL(pool_relu_bwd_colsum_part_kernel<false>,
                     dim3(g.cblocks, g.chunks), dim3(256), 0, cur_stream(),
                     (const bf16*)y_pooled.data_ptr(),
                     idx.data_ptr<uint8_t>(),
                     (const bf16*)dy_pooled.data_ptr(), (bf16*)nullptr, Mpix,
                     N, sh.OH, sh.OW, g.G, g.rows, cpart.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  colsum_finalize(cpart, db);
  return db;
}

}  // namespace

torch::Tensor conv2d_relu_pool_fwd(torch::Tensor x, torch::Tensor w,
                                   torch::Tensor b, long stride, long pad,
                                   long max_blocks, std::string impl) {
  return std::get<0>(
      relu_pool_fwd_impl(x, w, b, stride, pad, false, max_blocks, impl));
}

// What the "gemm256_pool" route launches for these shapes: "halo_mfma"
// (halo_conv_pool_kernel) or "gemm256" (gemm256_kernel, also the answer
// for shapes that route does not take at all). Same bits either way.
std::string conv_fwd_pool_impl(std::vector<long> x_shape,
                               std::vector<long> w_shape, long stride,
                               long pad) {
  const auto sh = make_shape_dims(x_shape, w_shape, stride, pad);
  return pool_route(sh) == PoolRoute::kGemm256 && halo_conv_gate(sh)
             ? "halo_mfma"
             : "gemm256";
}

// Images per LDS group of the halo kernel for these shapes (0: the
// geometry is not the kernel's).
long halo_conv_group_images_query(std::vector<long> x_shape,
                                  std::vector<long> w_shape, long stride,
                                  long pad) {
  return halo_conv_group_images(
      make_shape_dims(x_shape, w_shape, stride, pad));
}

// ---- the grad-free conv stack: conv3x3 + ReLU + pool, twice ----
// conv2d_relu_pool_fwd(conv2d_relu_pool_fwd(x, w1, b1, 1, 1), w2, b2, 1,
// 1). Where the first call would take the thin route and the second the
// halo kernel, halo_conv_stack_kernel runs both: the first layer's
// pooled output is computed in LDS by the thin kernel's own chain and
// never reaches HBM. Same bits as the two calls, which every other shape
// keeps.
namespace {

struct StackShapes { ConvShape sh1, sh2; };

StackShapes stack_shapes(const std::vector<long>& xs,
                         const std::vector<long>& w1s,
                         const std::vector<long>& w2s) {
  StackShapes s;
  s.sh1 = make_shape_dims(xs, w1s, 1, 1);
  s.sh2 = make_shape_dims({xs[0], s.sh1.OH / 2, s.sh1.OW / 2, w1s[0]}, w2s,
                          1, 1);
  return s;
}

// the stack kernel's chains are those of exactly these two routes
bool stack_gate(const StackShapes& s) {
  return pool_route(s.sh1) == PoolRoute::kThin &&
         pool_route(s.sh2) == PoolRoute::kGemm256 &&
         halo_stack_gate(s.sh1, s.sh2);
}

}  // namespace

std::string conv_relu_pool_stack_route(std::vector<long> x_shape,
                                       std::vector<long> w1_shape,
                                       std::vector<long> w2_shape) {
  TORCH_CHECK(w2_shape.size() == 4 && w1_shape.size() == 4 &&
              w2_shape[3] == w1_shape[0],
              "conv stack: w2's channels are w1's outputs");
  return stack_gate(stack_shapes(x_shape, w1_shape, w2_shape))
             ? "halo_stack"
             : "two_call";
}

long halo_stack_group_images_query(std::vector<long> x_shape,
                                   std::vector<long> w1_shape,
                                   std::vector<long> w2_shape) {
  const StackShapes s = stack_shapes(x_shape, w1_shape, w2_shape);
  return halo_stack_group_images(s.sh1, s.sh2);
}

// impl: "" = what conv_relu_pool_stack_route reports; "two_call" pins
// the two calls, "halo_stack" the kernel on its geometry alone (tests,
// op benchmark). max_blocks > 0 caps the halo kernels' grids.
torch::Tensor conv_relu_pool_stack_fwd(torch::Tensor x, torch::Tensor w1,
                                       torch::Tensor b1, torch::Tensor w2,
                                       torch::Tensor b2, long max_blocks,
                                       std::string impl) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_CONTIG(w1); CHECK_CONTIG(w2);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              w1.scalar_type() == at::kBFloat16 &&
              w2.scalar_type() == at::kBFloat16 &&
              b1.scalar_type() == at::kBFloat16 &&
              b2.scalar_type() == at::kBFloat16, "conv: bf16 only");
  TORCH_CHECK(impl.empty() || impl == "two_call" || impl == "halo_stack",
              "conv_relu_pool_stack: impl is '' | two_call | halo_stack");
  TORCH_CHECK(x.dim() == 4 && w1.dim() == 4 && w2.dim() == 4 &&
              w2.size(3) == w1.size(0),
              "conv stack: NHWC x, KRSC weights, w2's channels w1's outputs");
  const StackShapes s = stack_shapes(x.sizes().vec(), w1.sizes().vec(),
                                     w2.sizes().vec());
  const bool pinned = impl == "halo_stack";
  TORCH_CHECK(!pinned || halo_stack_geometry_ok(s.sh1, s.sh2),
              "conv_relu_pool_stack: shape outside the stack kernel's "
              "geometry");
  if (pinned || (impl.empty() && stack_gate(s))) {
    auto b1c = b1.contiguous(), b2c = b2.contiguous();
    auto y = torch::empty({(long)s.sh2.N, (long)s.sh2.OH / 2,
                           (long)s.sh2.OW / 2, (long)s.sh2.Kout},
                          x.options());
    halo_stack_launch(x, w1, b1c, w2, b2c, y, s.sh1, s.sh2, (int)max_blocks);
    return y;
  }
  auto h = std::get<0>(relu_pool_fwd_impl(x, w1, b1, 1, 1, false));
  return std::get<0>(
      relu_pool_fwd_impl(h, w2, b2, 1, 1, false, max_blocks, ""));
}

// Training forward: the same routes, plus the u8 argmax plane the
// backward needs. Both outputs are bitwise conv2d_fwd(relu) then
// maxpool2d_fwd(2, 2, want_idx=true).
std::tuple<torch::Tensor, torch::Tensor> conv2d_relu_pool_fwd_idx(
    torch::Tensor x, torch::Tensor w, torch::Tensor b, long stride,
    long pad, long max_blocks, std::string impl) {
  return relu_pool_fwd_impl(x, w, b, stride, pad, true, max_blocks, impl);
}

// (masked full-resolution dy, db) from the pooled tensors; out_shape is
// the conv output [N, 2*PH, 2*PW, C]. Both are bitwise maxpool2d_bwd
// then relu_bwd_colsum: same plane, same chunks, same trees.
std::tuple<torch::Tensor, torch::Tensor> pool_relu_bwd_colsum(
    torch::Tensor y_pooled, torch::Tensor idx, torch::Tensor dy_pooled,
    std::vector<long> out_shape) {
  check_pooled(y_pooled, idx, dy_pooled);
  const long n = y_pooled.size(0), PH = y_pooled.size(1),
             PW = y_pooled.size(2), N = y_pooled.size(3);
  TORCH_CHECK(N % 8 == 0, "pool_relu_bwd_colsum: C % 8 required");
  TORCH_CHECK(out_shape.size() == 4 && out_shape[0] == n &&
              out_shape[1] == 2 * PH && out_shape[2] == 2 * PW &&
              out_shape[3] == N,
              "pool_relu_bwd_colsum: out_shape must be [N, 2*PH, 2*PW, C]");
  const long M = n * PH * PW * 4;  // full-resolution rows
  auto dx = torch::empty({n, 2 * PH, 2 * PW, N}, dy_pooled.options());
  auto db = torch::empty({N}, dy_pooled.options());
  const ColsumGeom g = colsum_geom(M, N);  // relu_bwd_colsum's
  auto part = torch::empty({g.chunks, N},
                           dy_pooled.options().dtype(at::kFloat));
  if (M > 0) {
    hipLaunchKernelGGL(pool_relu_bwd_colsum_part_kernel<true>,
                       dim3(g.cblocks, g.chunks), dim3(256), 0, cur_stream(),
                       (const bf16*)y_pooled.data_ptr(),
                       idx.data_ptr<uint8_t>(),
                       (const bf16*)dy_pooled.data_ptr(),
                       (bf16*)dx.data_ptr(), M, N, (int)(2 * PH),
                       (int)(2 * PW), g.G, g.rows, part.data_ptr<float>());
    HIP_CHECK(hipGetLastError());
  }
  colsum_finalize(part, db);
  return {dx, db};
}

// (dw, db) of the thin first layer straight from the pooled tensors.
std::tuple<torch::Tensor, torch::Tensor> thin_conv_pool_wgrad(
    torch::Tensor x, torch::Tensor y_pooled, torch::Tensor idx,
    torch::Tensor dy_pooled, long stride, long pad) {
  CHECK_GPU(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 4,
              "thin_conv_pool_wgrad: bf16 NHWC x");
  check_pooled(y_pooled, idx, dy_pooled);
  const auto sh = make_shape_dims(
      x.sizes().vec(), {y_pooled.size(3), 3, 3, x.size(3)}, stride, pad);
  TORCH_CHECK(thin_wgrad_eligible(sh),
              "thin_conv_pool_wgrad: 3x3, C == 1, stride 1, even OH/OW, "
              "Kout % 8 == 0 and Kout <= 64 only");
  TORCH_CHECK(y_pooled.size(0) == sh.N && y_pooled.size(1) == sh.OH / 2 &&
              y_pooled.size(2) == sh.OW / 2,
              "thin_conv_pool_wgrad: pooled shape does not match x");
  const long MP = sh.M() / 4;
  const int N = sh.Kout;
  const int G = N / 8, PL = 256 / G;
  // about two waves per SIMD over the 256 CUs (512 blocks), at least
  // one pixel per lane: from the row count, not a device query
  const long rows = std::max<long>(PL, (MP + 511) / 512);
  const int chunks = (int)std::max<long>(1, (MP + rows - 1) / rows);
  auto part = torch::empty({(long)chunks, (long)N, (long)kWgradAcc},
                           x.options().dtype(at::kFloat));
  auto dw = torch::empty({(long)N, 3, 3, 1}, x.options());
  auto db = torch::empty({(long)N}, x.options());
  hipLaunchKernelGGL(thin_conv_pool_wgrad_part_kernel, dim3(chunks),
                     dim3(256), 0, cur_stream(), (const bf16*)x.data_ptr(),
                     (const bf16*)y_pooled.data_ptr(),
                     idx.data_ptr<uint8_t>(),
                     (const bf16*)dy_pooled.data_ptr(), sh, MP, G, rows,
                     part.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(thin_conv_pool_wgrad_final_kernel,
                     dim3(ceil_div((long)N * kWgradAcc, 4)), dim3(256), 0,
                     cur_stream(), part.data_ptr<float>(), chunks, N,
                     (bf16*)dw.data_ptr(), (bf16*)db.data_ptr());
  HIP_CHECK(hipGetLastError());
  return {dw, db};
}

// (dw, db) of the thin first layer, BITWISE the materialised chain
// pool_relu_bwd_colsum -> conv2d_bwd (im2col, split-K GEMM, reduce,
// narrow copy): dW from the same MFMA chains and the same reduce, db
// from the unpool kernel's own walk with the plane store left out.
std::tuple<torch::Tensor, torch::Tensor> thin_conv_pool_wgrad_fused(
    torch::Tensor x, torch::Tensor y_pooled, torch::Tensor idx,
    torch::Tensor dy_pooled, long stride, long pad) {
  CHECK_GPU(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 4,
              "thin_conv_pool_wgrad_fused: bf16 NHWC x");
  check_pooled(y_pooled, idx, dy_pooled);
  const auto sh = make_shape_dims(
      x.sizes().vec(), {y_pooled.size(3), 3, 3, x.size(3)}, stride, pad);
  const ThinFusedPlan t = thin_fused_plan(sh);
  TORCH_CHECK(t.ok,
              "thin_conv_pool_wgrad_fused: 3x3, C == 1, stride 1, even "
              "OH/OW, Kout % 8 == 0 and Kout <= 64, on the small-tile "
              "split-K plan, only");
  TORCH_CHECK(y_pooled.size(0) == sh.N && y_pooled.size(1) == sh.OH / 2 &&
              y_pooled.size(2) == sh.OW / 2,
              "thin_conv_pool_wgrad_fused: pooled shape does not match x");
  const long Mpix = sh.M();
  const int N = sh.Kout;
  auto dw = torch::empty({(long)N, 3, 3, 1}, x.options());
  torch::Tensor db;

  torch::Tensor part;
  if (t.S > 1)
    part = torch::empty({t.S, (long)N, 9}, x.options().dtype(at::kFloat));
  const int frags = (N + 15) / 16;
  // waves per fragment: 4, or 2 where four fragments fill the block
  auto* kern = frags <= 2 ? thin_pool_wgrad_mfma_kernel<4>
                          : thin_pool_wgrad_mfma_kernel<2>;
  hipLaunchKernelGGL(kern, dim3((unsigned)t.S),
                     dim3(frags * (frags <= 2 ? 4 : 2) * 64), (size_t)t.lds,
                     cur_stream(), (const unsigned short*)x.data_ptr(),
                     (const unsigned short*)y_pooled.data_ptr(),
                     idx.data_ptr<uint8_t>(),
                     (const unsigned short*)dy_pooled.data_ptr(), sh, Mpix,
                     t.kslice, t.cshift, t.tbl_pairs,
                     t.S > 1 ? part.data_ptr<float>() : nullptr,
                     (bf16*)dw.data_ptr());
  HIP_CHECK(hipGetLastError());
  if (t.S > 1) {
    auto dw2 = dw.view({(long)N, 9});
    splitk_reduce_plain(part, dw2);
  }

  db = pool_relu_bwd_db(y_pooled, idx, dy_pooled, sh);
  return {dw, db};
}

// Which implementation conv2d_relu_pool_bwd's "unpool" route runs for
// the thin first layer: "fused_mfma" (thin_conv_pool_wgrad_fused) or
// "materialized" (unpool plane -> im2col -> GEMM). Both give the same
// bits; the query lets a test know which one it exercised.
std::string thin_pool_wgrad_impl(std::vector<long> x_shape,
                                 std::vector<long> w_shape, long stride,
                                 long pad, bool want_dx) {
  const auto sh = make_shape_dims(x_shape, w_shape, stride, pad);
  return !want_dx && thin_fused_wgrad_gate() && thin_fused_plan(sh).ok
             ? "fused_mfma"
             : "materialized";
}

// Route conv2d_relu_pool_bwd takes, so a test cannot pass through the
// wrong path: "thin_direct" (allowed, no dx wanted, thin geometry) or
// "unpool". The unpool route is bitwise the two-op backward; the direct
// one sums dW/db of the first layer in its own order (last-bit
// differences), which is why the caller has to allow it.
std::string conv2d_relu_pool_bwd_route(std::vector<long> x_shape,
                                       std::vector<long> w_shape,
                                       long stride, long pad, bool want_dx,
                                       bool allow_direct) {
  const auto sh = make_shape_dims(x_shape, w_shape, stride, pad);
  return allow_direct && !want_dx && thin_wgrad_eligible(sh) ? "thin_direct"
                                                             : "unpool";
}

namespace {

// (dx, masked full-resolution dy plane) of the halo dgrad kernel.
std::tuple<torch::Tensor, torch::Tensor> halo_pool_dgrad_impl(
    const torch::Tensor& x_like, const torch::Tensor& w,
    const torch::Tensor& y_pooled, const torch::Tensor& idx,
    const torch::Tensor& dy_pooled, const ConvShape& sh, long max_blocks,
    bool store_plane = true) {
  auto dyf = store_plane
                 ? torch::empty({(long)sh.N, (long)sh.OH, (long)sh.OW,
                                 (long)sh.Kout}, dy_pooled.options())
                 : torch::empty({0}, dy_pooled.options());
  auto dx = torch::empty({(long)sh.N, (long)sh.H, (long)sh.W, (long)sh.C},
                         x_like.options());
  halo_pool_dgrad_launch(w, y_pooled, idx, dy_pooled,
                         store_plane ? &dyf : nullptr, dx, sh,
                         (int)max_blocks);
  return {dx, dyf};
}

}  // namespace

// Which data gradient conv2d_relu_pool_bwd's "unpool" route runs:
// "halo_mfma" (halo_pool_dgrad_kernel on the pooled tensors, which also
// writes the plane; db from the store-free unpool pass) or
// "implicit_gemm" (unpool kernel, then conv2d_bwd; also the answer when
// no dx is wanted). Same bits either way.
std::string pool_dgrad_impl(std::vector<long> x_shape,
                            std::vector<long> w_shape, long stride, long pad,
                            bool want_dx) {
  const auto sh = make_shape_dims(x_shape, w_shape, stride, pad);
  return want_dx && halo_dgrad_gate(sh) ? "halo_mfma" : "implicit_gemm";
}

// Images per LDS group of the halo dgrad kernel (0: not its geometry).
long halo_dgrad_group_images_query(std::vector<long> x_shape,
                                   std::vector<long> w_shape, long stride,
                                   long pad) {
  return halo_dgrad_group_images(
      make_shape_dims(x_shape, w_shape, stride, pad));
}

// The halo dgrad kernel on its geometry alone (tests, op benchmark):
// (dx, plane). max_blocks > 0 caps the grid; store_plane = false leaves
// the plane store out (0-size plane), for the measurement of what it
// costs.
std::tuple<torch::Tensor, torch::Tensor> halo_pool_dgrad(
    torch::Tensor w, torch::Tensor y_pooled, torch::Tensor idx,
    torch::Tensor dy_pooled, long max_blocks, bool store_plane) {
  CHECK_GPU(w); CHECK_CONTIG(w);
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.dim() == 4,
              "halo_pool_dgrad: bf16 KRSC w");
  check_pooled(y_pooled, idx, dy_pooled);
  const auto sh = make_shape_dims(
      {y_pooled.size(0), 2 * y_pooled.size(1), 2 * y_pooled.size(2),
       w.size(3)},
      w.sizes().vec(), 1, 1);
  TORCH_CHECK(y_pooled.size(3) == sh.Kout && halo_dgrad_geometry_ok(sh),
              "halo_pool_dgrad: shape outside the halo kernel's geometry");
  return halo_pool_dgrad_impl(dy_pooled, w, y_pooled, idx, dy_pooled, sh,
                              max_blocks, store_plane);
}

// Backward of conv + bias + ReLU + 2x2/2 maxpool from what the fused
// forward saved: (dx, dw, db), dx / db 0-size unless wanted.
// dgrad_impl: "" = what pool_dgrad_impl reports; "halo_mfma" /
// "implicit_gemm" pin one side of the data gradient (tests, op
// benchmark; a pinned halo run checks the geometry only). max_blocks > 0
// caps the halo kernel's grid.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> conv2d_relu_pool_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor y_pooled,
    torch::Tensor idx, torch::Tensor dy_pooled, long stride, long pad,
    bool want_db, bool want_dx, bool allow_direct, std::string dgrad_impl,
    long max_blocks) {
  CHECK_GPU(x); CHECK_CONTIG(x); CHECK_CONTIG(w);
  const auto sh = make_shape(x, w, stride, pad);
  TORCH_CHECK(sh.OH % 2 == 0 && sh.OW % 2 == 0 &&
              y_pooled.dim() == 4 && y_pooled.size(0) == sh.N &&
              y_pooled.size(1) == sh.OH / 2 &&
              y_pooled.size(2) == sh.OW / 2 && y_pooled.size(3) == sh.Kout,
              "conv2d_relu_pool_bwd: pooled shape does not match the conv");
  TORCH_CHECK(dgrad_impl.empty() || dgrad_impl == "halo_mfma" ||
                  dgrad_impl == "implicit_gemm",
              "conv2d_relu_pool_bwd: dgrad_impl is '' | halo_mfma | "
              "implicit_gemm");
  const bool force_halo = dgrad_impl == "halo_mfma";
  TORCH_CHECK(!force_halo || (want_dx && halo_dgrad_geometry_ok(sh) &&
                              sh.M() * sh.Kout < (1L << 31)),
              "conv2d_relu_pool_bwd: shape outside the halo dgrad kernel's "
              "geometry");
  auto none = torch::empty({0}, x.options());
  if (allow_direct && !want_dx && thin_wgrad_eligible(sh)) {
    auto [dw, db] = thin_conv_pool_wgrad(x, y_pooled, idx, dy_pooled,
                                         stride, pad);
    return {none, dw.view(w.sizes()), want_db ? db : none};
  }
  // the unpool route of the thin first layer without its plane, col
  // matrix and narrow copy: same bits (thin_conv_pool_wgrad_fused)
  if (!want_dx && thin_fused_wgrad_gate() && thin_fused_plan(sh).ok) {
    auto [dw, db] = thin_conv_pool_wgrad_fused(x, y_pooled, idx, dy_pooled,
                                               stride, pad);
    return {none, dw.view(w.sizes()), want_db ? db : none};
  }
  // conv2's training shape: the data gradient straight from the pooled
  // tensors, whole images in LDS; the kernel leaves the plane behind for
  // the unchanged weight gradient. Same bits (halo_pool_dgrad_kernel).
  if (force_halo ||
      (dgrad_impl.empty() && want_dx && halo_dgrad_gate(sh))) {
    check_pooled(y_pooled, idx, dy_pooled);
    auto db = want_db ? pool_relu_bwd_db(y_pooled, idx, dy_pooled, sh) : none;
    auto [dx, dyf] = halo_pool_dgrad_impl(x, w, y_pooled, idx, dy_pooled, sh,
                                          max_blocks);
    auto dy2 = dyf.view({sh.M(), (long)sh.Kout});
    auto dw = conv_wgrad(x, w, dy2, sh, c10::nullopt);
    return {dx, dw, db};
  }
  auto [dyf, db] = pool_relu_bwd_colsum(
      y_pooled, idx, dy_pooled,
      {(long)sh.N, (long)sh.OH, (long)sh.OW, (long)sh.Kout});
  auto [dx, dw, db_unused] =
      conv2d_bwd(x, w, dyf, stride, pad, c10::nullopt, false, want_dx);
  (void)db_unused;
  return {dx, dw, want_db ? db : none};
}

torch::Tensor maxpool2d_bwd(torch::Tensor dy, torch::Tensor idx,
                            std::vector<long> in_shape, long kernel,
                            long stride) {
  CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_CONTIG(idx);
  TORCH_CHECK(idx.numel() == dy.numel(),
              "maxpool2d_bwd: argmax mask missing/size-mismatched (the "
              "forward ran with want_idx=false?)");
  ConvShape sh;
  sh.N = (int)in_shape[0]; sh.H = (int)in_shape[1];
  sh.W = (int)in_shape[2]; sh.C = (int)in_shape[3];
  sh.R = sh.S = (int)kernel; sh.stride = (int)stride; sh.pad = 0;
  sh.Kout = sh.C;
  sh.OH = (int)dy.size(1); sh.OW = (int)dy.size(2);
  auto dx = torch::empty({(long)sh.N, (long)sh.H, (long)sh.W, (long)sh.C},
                         dy.options());
  if (sh.C % 8 == 0) {
    const long total_g = (long)sh.N * sh.H * sh.W * (sh.C / 8);
    hipLaunchKernelGGL(maxpool_nhwc_vec_bwd, dim3(ew_grid(total_g)),
                       dim3(256), 0, cur_stream(),
                       (const bf16*)dy.data_ptr(), idx.data_ptr<uint8_t>(),
                       (bf16*)dx.data_ptr(), sh, total_g);
  } else {
    const long total = dx.numel();
    hipLaunchKernelGGL(maxpool_nhwc_bwd, dim3(ew_grid(total)), dim3(256), 0,
                       cur_stream(), (const bf16*)dy.data_ptr(),
                       idx.data_ptr<uint8_t>(), (bf16*)dx.data_ptr(), sh,
                       total);
  }
  HIP_CHECK(hipGetLastError());
  return dx;
}

}  // namespace bflc
