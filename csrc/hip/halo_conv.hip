// Halo-tile 3x3 conv + bias + ReLU + 2x2/2 maxpool forward for C == 32
// (FEMNIST conv2: [N,14,14,32] -> 64, pooled to 7x7).
//
// gemm256_kernel<.., 1, POOL> runs this shape as an implicit GEMM with
// K = 9 taps * 32 channels: every 64-wide K-step re-gathers the same x
// pixels from global memory one tap further on (predicate, (c,s,r)
// decode, register staging, LDS write) and re-stages the same 36 KB of
// weights, for a 64x16 wave tile that issues five ds_read_b128 per four
// MFMAs. At C == 32 one mfma_f32_16x16x32_bf16 k-chunk is exactly one
// tap with all its channels, and lane (l15, l4) needs channels
// l4*8..+7 of pixel (oh+r-1, ow+s-1): 16 contiguous bytes of x.
//
// So a block keeps G whole images in LDS inside a ring of zero pixels
// ((H+2) x (W+2) pixels of 64 B): every A fragment is ONE ds_read_b128
// at a per-lane base plus a tap offset, the padding predicate is the
// ring, and x is read from HBM once, in coalesced 16-B loads. The
// weights live in registers, fetched once per block (a wave owns all 64
// output columns: 9 taps x 4 fragments = 144 VGPRs, so one A fragment
// feeds four MFMAs). Blocks are persistent, two per CU: each walks its
// groups of G images and fetches group i+1 into registers while it
// computes group i, then writes it to the other LDS buffer.
//
// Bits: every accumulator runs gemm256_kernel's chain - from +0, taps
// (r,s) = (0,0)..(2,2) ascending (k = (r*3+s)*32 + c), then the tenth
// MFMA on all-zero operands that K = 288 padded to five 64-steps
// issues there - with the same instruction and operand layout, and the
// epilogue is its POOL epilogue operation for operation. The result is
// bitwise the unsplit gemm256 pooled forward; the gate therefore only
// takes shapes whose plan has one K slice.
//
// The second half of the file is the same structure for that layer's
// data gradient, fed from the pooled tensors (halo_pool_dgrad_kernel).
#include "common.h"
#include "gemm_api.h"

#include <cstdlib>

namespace bflc {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int kHaloThreads = 256;  // 4 row waves, each all 64 columns
constexpr int kHaloWC = 1;         // column waves
constexpr int kHaloPF = 8;         // prefetch granules (16 B) per thread
constexpr int kHaloMinBlocks = 2;  // blocks per CU the LDS budget allows
constexpr long kHaloLdsBudget = 80 * 1024;  // per block, both buffers

// n / d for n * d < 2^32 as one 64-bit multiply (d >= 1).
struct Magic { unsigned long long m; };
inline Magic make_magic(unsigned d) { return {0xFFFFFFFFull / d + 1}; }
__device__ __forceinline__ unsigned mdiv(unsigned n, Magic g) {
  return (unsigned)(((unsigned long long)n * g.m) >> 32);
}

struct HaloParams {
  int N, H, W, PH, PW;  // images, input size, pooled size
  int G;                // images per group
  int pitch;            // LDS bytes per halo row: (W+2)*64 + 32
  int img_lds;          // LDS bytes per image: (H+2) * pitch
  int hw4;              // 16-B granules per image: H*W*4
  int phw;              // pooled pixels per image
  Magic m_hw4, m_w, m_phw, m_pw;
};

// Row pitch (W+2)*64 + 32: the 16 lanes of one ds_read_b128 group hold
// both dy rows of four neighbouring windows - 8 pixels of a halo row at
// 64 B each cover the 16-B slots {0,16,64,80,128,144,192,208} mod 256,
// and a pitch that is 32 mod 64 puts the dy + 1 row on the other eight.
// (The launch bound's second argument counts waves per SIMD: a block
// puts kHaloThreads / 256 on each, so two blocks per CU leave a wave
// 256 VGPRs - the 144 of B, the prefetch and the accumulators fit
// without scratch.)
template <int POOLV>
__launch_bounds__(kHaloThreads, kHaloMinBlocks * (kHaloThreads / 256))
__global__ void halo_conv_pool_kernel(const unsigned char* __restrict__ x,
                                      const bf16* __restrict__ w2,
                                      const bf16* __restrict__ bias,
                                      bf16* __restrict__ y,
                                      uint8_t* __restrict__ pool_idx,
                                      int relu, HaloParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int WR = kHaloThreads / 64 / kHaloWC;  // row waves
  constexpr int FN = 4 / kHaloWC;  // 16-column fragments per wave
  constexpr int WN = FN * 16;      // columns per wave
  constexpr int KOUT = 64, KW = 9 * 32;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int l15 = lane & 15, l4 = lane >> 4;
  // wave roles and every tile-loop bound are scalar, so no MFMA sits
  // under a saved EXEC mask
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / kHaloWC, wc = wave % kHaloWC;

  const int buf_bytes = p.G * p.img_lds;
  const int ngroups = (p.N + p.G - 1) / p.G;

  // zero both buffers once: the ring stays zero for the block's life
  // (staging only ever writes interior pixels)
  {
    const u32x4_t z = {0u, 0u, 0u, 0u};
    for (int o = tid * 16; o < 2 * buf_bytes; o += kHaloThreads * 16)
      *reinterpret_cast<u32x4_t*>(smem + o) = z;
  }

  // weights: b[t][fn] = w2[col][t*32 + l4*8 ..+7], col = wc*WN + fn*16 + l15
  bf16x8_t bfr[9][FN];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
      bfr[t][fn] = *reinterpret_cast<const bf16x8_t*>(
          &w2[(long)(wc * WN + fn * 16 + l15) * KW + t * 32 + l4 * 8]);
  float bv[FN];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn)
    bv[fn] = bias ? b2f(bias[wc * WN + fn * 16 + l15]) : 0.f;

  // staging slots of this thread: granule gi of a group -> its interior
  // LDS offset (the same for every group)
  int st_off[kHaloPF];
#pragma unroll
  for (int i = 0; i < kHaloPF; ++i) {
    const unsigned gi = tid + i * kHaloThreads;
    const unsigned img = mdiv(gi, p.m_hw4);
    const unsigned rem = gi - img * p.hw4;
    const unsigned pix = rem >> 2, ch = rem & 3;
    const unsigned py = mdiv(pix, p.m_w), px = pix - py * p.W;
    st_off[i] = (int)(img * p.img_lds + (py + 1) * p.pitch + (px + 1) * 64 +
                      ch * 16);
  }
  u32x4_t pf[kHaloPF];
  auto fetch = [&](int g) __attribute__((always_inline)) {
    const int gc = min(p.G, p.N - g * p.G);
    const int ngr = gc * p.hw4;
    const unsigned char* src = x + (long)g * p.G * p.hw4 * 16;
#pragma unroll
    for (int i = 0; i < kHaloPF; ++i) {
      const int gi = tid + i * kHaloThreads;
      if (gi < ngr)
        pf[i] = *reinterpret_cast<const u32x4_t*>(src + (long)gi * 16);
    }
    return ngr;
  };
  auto stage = [&](int buf, int ngr) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < kHaloPF; ++i) {
      const int gi = tid + i * kHaloThreads;
      if (gi < ngr)
        *reinterpret_cast<u32x4_t*>(smem + buf * buf_bytes + st_off[i]) =
            pf[i];
    }
  };

  int g = blockIdx.x;
  if (g >= ngroups) return;  // block-uniform
  {
    const int ngr = fetch(g);
    __syncthreads();  // zero fill done before the interior lands
    stage(0, ngr);
  }
  __syncthreads();

  int cur = 0;
  for (; g < ngroups; g += gridDim.x) {
    const int gnext = g + gridDim.x;
    const bool has_next = gnext < ngroups;  // block-uniform
    int ngr_next = 0;
    if (has_next) ngr_next = fetch(gnext);

    const int gc = min(p.G, p.N - g * p.G);
    const int npp = gc * p.phw;            // pooled pixels of this group
    const int ntiles = (npp + 3) >> 2;     // 16-row MFMA tiles
    const long pp0 = (long)g * p.G * p.phw;
    const unsigned char* lbuf = smem + cur * buf_bytes;

    for (int mt = wr; mt < ntiles; mt += WR) {
      // rows are window-major: row = pooled pixel * 4 + dy*2 + dx
      const int pp = mt * 4 + (l15 >> 2);
      const int q = l15 & 3;
      const unsigned ppc = pp < npp ? pp : 0;
      const unsigned img = mdiv(ppc, p.m_phw);
      const unsigned rem = ppc - img * p.phw;
      const unsigned ph = mdiv(rem, p.m_pw), pw = rem - ph * p.PW;
      const unsigned char* a0 = lbuf + img * p.img_lds +
                                (2 * ph + (q >> 1)) * p.pitch +
                                (2 * pw + (q & 1)) * 64 + l4 * 16;
      const unsigned char* a1 = a0 + p.pitch;
      const unsigned char* a2 = a1 + p.pitch;

      f32x4_t acc[FN] = {};
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int r = t / 3, s = t - r * 3;
        const unsigned char* ar = r == 0 ? a0 : (r == 1 ? a1 : a2);
        const bf16x8_t af =
            *reinterpret_cast<const bf16x8_t*>(ar + s * 64);
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af, bfr[t][fn], acc[fn], 0, 0, 0);
      }
      {  // the K tail of the 64-wide steps: one all-zero chunk
        const u32x4_t zu = {0u, 0u, 0u, 0u};
        const bf16x8_t z = *reinterpret_cast<const bf16x8_t*>(&zu);
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              z, z, acc[fn], 0, 0, 0);
      }

      // POOL epilogue of gemm256_kernel: the lane's four accumulator
      // rows are one window, in the pool kernel's order
      const int opp = mt * 4 + l4;
      if (opp < npp) {
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
          const int col = wc * WN + fn * 16 + l15;
          float best = -INFINITY;
          int bi = 0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = acc[fn][r] + bv[fn];
            if (relu) v = fmaxf(v, 0.f);
            const float f = b2f(f2b(v));
            if (f > best) {
              best = f;
              if (POOLV == 2) bi = r;
            }
          }
          y[(pp0 + opp) * KOUT + col] = f2b(best);
          if (POOLV == 2) pool_idx[(pp0 + opp) * KOUT + col] = (uint8_t)bi;
        }
      }
    }

    if (has_next) stage(cur ^ 1, ngr_next);
    __syncthreads();
    cur ^= 1;
  }
}

// BFLC_HALO_CONV: 1 (default) routes the gated pooled conv forward to
// the halo kernel, 0 keeps gemm256_kernel (A/B runs; same bits).
bool halo_conv_env_gate() {
  static const bool v = [] {
    const char* e = getenv("BFLC_HALO_CONV");
    return (e ? atoi(e) : 1) != 0;
  }();
  return v;
}

struct HaloGeom {
  bool ok = false;
  int G = 0, pitch = 0, img_lds = 0;
};

HaloGeom halo_geom(const ConvShape& sh) {
  HaloGeom g;
  if (sh.C != 32 || sh.R != 3 || sh.S != 3 || sh.stride != 1 ||
      sh.pad != 1 || sh.Kout != 64 || sh.N <= 0 || sh.OH <= 0 ||
      sh.OW <= 0 || sh.OH % 2 != 0 || sh.OW % 2 != 0)
    return g;
  g.pitch = (sh.W + 2) * 64 + 32;
  const long img = (long)(sh.H + 2) * g.pitch;
  const long by_lds = kHaloLdsBudget / (2 * img);
  const long by_pf =
      (long)kHaloPF * kHaloThreads / ((long)sh.H * sh.W * 4);
  const long G = std::min(by_lds, by_pf);
  if (G < 1) return g;
  g.G = (int)G;
  g.img_lds = (int)img;
  g.ok = true;
  return g;
}

// ---- data gradient through the pool, fed from the pooled tensors ----
// conv2's backward at the training shape ran the implicit dgrad on
// gemm_kernel<.., CMODE 2>: 18 synchronous 32-wide K-steps that each
// re-gather the same dy pixels one tap (or half a tap) further on, and
// re-stage the weights, from a 64-channel full-resolution plane that the
// unpool kernel had just expanded from the pooled (dy, y, idx). dgrad is
// the forward's mirror image - a flipped 3x3 correlation of that plane
// with w, Kout = 64 in, C = 32 out - so the same halo structure serves:
// a tap is two mfma_f32_16x16x32_bf16 k-chunks (kout 0..31, 32..63) and
// lane (l15, l4) needs 16 contiguous bytes of one plane pixel per chunk.
//
// A block walks groups of G whole images. It prefetches a group's pooled
// dy / y (16 B) and idx (8 B) granules into registers while the previous
// group computes, then UNPOOLS them itself: all four positions of every
// 2x2 window go into a zero-ringed LDS image (128 B a pixel), each by
// pool_relu_bwd_colsum_part_kernel<true>'s own expression, and the same
// 16-B granules go to the global plane, which the weight gradient still
// reads. dgrad never reads the plane from HBM.
//
// LDS: pixel p (linear index in the ringed image stack) sits at p * 128;
// its eight 16-B slots are XORed with (p >> 1) & 7. Unswizzled, the 16
// lanes of a ds_read_b128 group - consecutive pixels - fall on two slots
// of the 256-B bank row (4-way); with the XOR eight consecutive pixels
// of one parity take eight different slots. A group mixes slots l4 and
// l4 + 1 and a 16-row tile at W = 14 crosses a row, so about half the
// reads stay 2-way (profiles/r09_halo_dgrad_ab.md).
//
// Weights: lane (l15, l4), chunk (tap, half), fragment fn holds
// w[half*32 + l4*8 + j][r][s][fn*16 + l15], j = 0..7 - wrot2 of
// conv2d_bwd, read from w itself. The block transposes w once through
// LDS (a wave's 64 lanes take the 64 kout of one 16-B channel granule,
// so the eight 2-B writes of a granule are contiguous across lanes) and
// every B fragment is then one ds_read_b128: no permute copy is issued.
//
// Bits: every output runs the parent's chain - from +0, 18 MFMAs
// ascending in k = (r*3+s)*64 + kout, the A fragment of tap (r, s) being
// plane pixel (ih + 1 - r, iw + 1 - s), with the operand layout of the
// gemm_bf16.hip header - and its plain epilogue bf16(acc + 0.f). K = 576
// has no padding chunk. The chain is the same in gemm_kernel and
// gemm256_kernel whatever the tile, so the gate asks only for S == 1.
constexpr int kDgPF = 2;      // pooled granules (8 channels) per thread
constexpr int kDgWPitch = 72;  // transposed-w row: 64 kout + 8 pad (bf16)
constexpr long kDgWBytes = 9L * 32 * kDgWPitch * 2;

struct DgradParams {
  int N, H, W, PW;
  int G;        // images per group
  int WP;       // ringed row: W + 2 pixels
  int img_pix;  // ringed image: (H + 2) * (W + 2) pixels
  int hw;       // pixels per image
  int pgr;      // pooled granules per image: PH * PW * 8
  Magic m_pgr8, m_pw, m_hw, m_w;  // pooled pixels / image, PW, hw, W
};

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

__device__ __forceinline__ int dg_lds_off(int pix, int slot) {
  return pix * 128 + ((slot ^ ((pix >> 1) & 7)) << 4);
}

// PLANE = false leaves the global plane store out (dyf is not touched):
// the other side of the "who writes the plane" measurement.
template <bool PLANE>
__launch_bounds__(kHaloThreads, kHaloMinBlocks * (kHaloThreads / 256))
__global__ void halo_pool_dgrad_kernel(const bf16* __restrict__ w,
                                       const unsigned char* __restrict__ yp,
                                       const unsigned char* __restrict__ idx,
                                       const unsigned char* __restrict__ dyp,
                                       unsigned char* __restrict__ dyf,
                                       bf16* __restrict__ dx, DgradParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int WR = kHaloThreads / 64;  // row waves, each all 32 columns
  constexpr int FN = 2, C = 32;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int l15 = lane & 15, l4 = lane >> 4;
  // the wave index and every tile-loop bound are scalar, so no MFMA
  // sits under a saved EXEC mask
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int buf_bytes = p.G * p.img_pix * 128;
  const int ngroups = (p.N + p.G - 1) / p.G;
  int g = blockIdx.x;
  if (g >= ngroups) return;  // block-uniform

  // staging slots of this thread: pooled granule gi of a group -> the
  // ringed LDS pixel and the plane granule of its window's (0, 0)
  // position (the same for every group)
  int st_pix[kDgPF], st_gl[kDgPF];
#pragma unroll
  for (int i = 0; i < kDgPF; ++i) {
    const unsigned gi = tid + i * kHaloThreads;
    const unsigned pp = gi >> 3;
    const unsigned img = mdiv(pp, p.m_pgr8);
    const unsigned rem = pp - img * (p.pgr >> 3);
    const unsigned ph = mdiv(rem, p.m_pw), pw = rem - ph * p.PW;
    st_pix[i] = (int)(img * p.img_pix + (2 * ph + 1) * p.WP + 2 * pw + 1);
    st_gl[i] = (int)((img * p.hw + 2 * ph * p.W + 2 * pw) * 8 + (gi & 7));
  }
  u32x4_t pf_dy[kDgPF], pf_y[kDgPF];
  u32x2_t pf_ix[kDgPF];
  auto fetch = [&](int gg) __attribute__((always_inline)) {
    const int gc = min(p.G, p.N - gg * p.G);
    const int ngr = gc * p.pgr;
    const long base = (long)gg * p.G * p.pgr;
#pragma unroll
    for (int i = 0; i < kDgPF; ++i) {
      const int gi = tid + i * kHaloThreads;
      if (gi < ngr) {
        pf_dy[i] =
            *reinterpret_cast<const u32x4_t*>(dyp + (base + gi) * 16);
        pf_y[i] = *reinterpret_cast<const u32x4_t*>(yp + (base + gi) * 16);
        pf_ix[i] = *reinterpret_cast<const u32x2_t*>(idx + (base + gi) * 8);
      }
    }
    return ngr;
  };
  // unpool group gg's prefetched granules into LDS buffer `buf` and the
  // global plane: position q of a window gets bf16(0.f + dy) where
  // idx == q and y > 0, +0 elsewhere
  auto stage = [&](int buf, int gg, int ngr) __attribute__((always_inline)) {
    unsigned char* lbuf = smem + buf * buf_bytes;
    unsigned char* gbase = dyf + (long)gg * p.G * p.hw * 128;
    const bf16 zero = f2b(0.f);
#pragma unroll
    for (int i = 0; i < kDgPF; ++i) {
      const int gi = tid + i * kHaloThreads;
      if (gi < ngr) {
        const bf16x8_t dv = __builtin_bit_cast(bf16x8_t, pf_dy[i]);
        const bf16x8_t yv = __builtin_bit_cast(bf16x8_t, pf_y[i]);
        const unsigned long long iv =
            __builtin_bit_cast(unsigned long long, pf_ix[i]);
        const int slot = gi & 7;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bf16x8_t gv;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float a = 0.f;
            if ((int)((iv >> (8 * j)) & 0xff) == q) a += b2f(dv[j]);
            gv[j] = f2b(a);
            if (!(b2f(yv[j]) > 0.f)) gv[j] = zero;
          }
          const int pix = st_pix[i] + (q >> 1) * p.WP + (q & 1);
          *reinterpret_cast<bf16x8_t*>(lbuf + dg_lds_off(pix, slot)) = gv;
          if (PLANE) {
            const long go = st_gl[i] + ((q >> 1) * p.W + (q & 1)) * 8;
            *reinterpret_cast<bf16x8_t*>(gbase + go * 16) = gv;
          }
        }
      }
    }
  };

  int ngr0 = fetch(g);  // in flight while the weights are transposed

  // ---- weights: wt[(tap*32 + c)][kout] through LDS, then B fragments
  {
    unsigned short* wt = reinterpret_cast<unsigned short*>(smem);
    const unsigned short* wg = reinterpret_cast<const unsigned short*>(w);
    const int kout = lane;
    u16x8_t wv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int q = wave + i * WR;  // (tap, c8): 36 granule columns
      wv[i] = *reinterpret_cast<const u16x8_t*>(&wg[kout * 288 + q * 8]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int q = wave + i * WR;
#pragma unroll
      for (int j = 0; j < 8; ++j) wt[(q * 8 + j) * kDgWPitch + kout] = wv[i][j];
    }
  }
  __syncthreads();
  bf16x8_t bfr[9][2][FN];
  {
    const unsigned short* wt = reinterpret_cast<const unsigned short*>(smem);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          bfr[t][h][fn] = *reinterpret_cast<const bf16x8_t*>(
              &wt[(t * 32 + fn * 16 + l15) * kDgWPitch + h * 32 + l4 * 8]);
  }
  __syncthreads();

  // zero both buffers once: the ring stays zero for the block's life
  // (staging only ever writes interior pixels, and writes all of them)
  {
    const u32x4_t z = {0u, 0u, 0u, 0u};
    for (int o = tid * 16; o < 2 * buf_bytes; o += kHaloThreads * 16)
      *reinterpret_cast<u32x4_t*>(smem + o) = z;
  }
  __syncthreads();
  stage(0, g, ngr0);
  __syncthreads();

  int cur = 0;
  for (; g < ngroups; g += gridDim.x) {
    const int gnext = g + gridDim.x;
    const bool has_next = gnext < ngroups;  // block-uniform
    int ngr_next = 0;
    if (has_next) ngr_next = fetch(gnext);

    const int gc = min(p.G, p.N - g * p.G);
    const int npix = gc * p.hw;          // output pixels of this group
    const int ntiles = (npix + 15) >> 4;  // 16-row MFMA tiles
    const long m0 = (long)g * p.G * p.hw;
    const unsigned char* lbuf = smem + cur * buf_bytes;

    for (int mt = wave; mt < ntiles; mt += WR) {
      const int m = mt * 16 + l15;
      const unsigned mc = m < npix ? m : 0;
      const unsigned img = mdiv(mc, p.m_hw);
      const unsigned rem = mc - img * p.hw;
      const unsigned ih = mdiv(rem, p.m_w), iw = rem - ih * p.W;
      // ringed pixel of tap (0, 0): plane pixel (ih + 1, iw + 1)
      const int pix0 =
          (int)(img * p.img_pix + (ih + 2) * p.WP + iw + 2);

      f32x4_t acc[FN] = {};
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int r = t / 3, s = t - r * 3;
        const int off = dg_lds_off(pix0 - r * p.WP - s, l4);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          // slot h*4 + l4: h is bit 2 of the slot, byte bit 6, on
          // either side of the XOR
          const bf16x8_t af =
              *reinterpret_cast<const bf16x8_t*>(lbuf + (off ^ (h << 6)));
#pragma unroll
          for (int fn = 0; fn < FN; ++fn)
            acc[fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af, bfr[t][h][fn], acc[fn], 0, 0, 0);
        }
      }

      // the parent's plain epilogue with a null bias
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mt * 16 + l4 * 4 + r;
        if (row < npix) {
#pragma unroll
          for (int fn = 0; fn < FN; ++fn)
            dx[(m0 + row) * C + fn * 16 + l15] = f2b(acc[fn][r] + 0.f);
        }
      }
    }

    if (has_next) stage(cur ^ 1, gnext, ngr_next);
    __syncthreads();
    cur ^= 1;
  }
}

// BFLC_HALO_DGRAD: 1 (default) routes the gated pooled conv backward's
// data gradient to halo_pool_dgrad_kernel, 0 keeps the unpool kernel and
// the implicit-GEMM dgrad (A/B runs; same bits).
bool halo_dgrad_env_gate() {
  static const bool v = [] {
    const char* e = getenv("BFLC_HALO_DGRAD");
    return (e ? atoi(e) : 1) != 0;
  }();
  return v;
}

struct DgradGeom {
  bool ok = false;
  int G = 0;
  long img_lds = 0;
};

DgradGeom dgrad_geom(const ConvShape& sh) {
  DgradGeom g;
  if (sh.C != 32 || sh.R != 3 || sh.S != 3 || sh.stride != 1 ||
      sh.pad != 1 || sh.Kout != 64 || sh.N <= 0 || sh.OH <= 0 ||
      sh.OW <= 0 || sh.OH % 2 != 0 || sh.OW % 2 != 0)
    return g;
  g.img_lds = (long)(sh.OH + 2) * (sh.OW + 2) * 128;
  const long by_lds = kHaloLdsBudget / (2 * g.img_lds);
  const long by_pf =
      (long)kDgPF * kHaloThreads / ((long)(sh.OH / 2) * (sh.OW / 2) * 8);
  const long G = std::min(by_lds, by_pf);
  if (G < 1) return g;
  g.G = (int)G;
  g.ok = true;
  return g;
}

}  // namespace

bool halo_dgrad_geometry_ok(const ConvShape& sh) { return dgrad_geom(sh).ok; }

int halo_dgrad_group_images(const ConvShape& sh) { return dgrad_geom(sh).G; }

// The one gate of the halo dgrad route: its geometry, an unsplit dgrad
// plan - whose chain the kernel issues - the 32-bit row x column index
// of the bias-gradient pass that goes with it, and the environment
// switch.
bool halo_dgrad_gate(const ConvShape& sh) {
  if (!halo_dgrad_env_gate() || !dgrad_geom(sh).ok) return false;
  if (sh.M() * sh.Kout >= (1L << 31)) return false;
  const GemmPlan p = gemm_conv_plan(ConvEntry::kDgrad, sh);
  return p.path != GemmPath::kNone && p.S == 1;
}

void halo_pool_dgrad_launch(const torch::Tensor& w,
                            const torch::Tensor& y_pooled,
                            const torch::Tensor& idx,
                            const torch::Tensor& dy_pooled,
                            torch::Tensor* dyf, torch::Tensor& dx,
                            const ConvShape& sh, int max_blocks) {
  const DgradGeom g = dgrad_geom(sh);
  TORCH_CHECK(g.ok, "halo dgrad: shape outside the kernel's geometry");
  // group bases are 64-bit; offsets inside a group are 32-bit
  TORCH_CHECK((long)sh.N * sh.OH * sh.OW < (1L << 31), "halo dgrad: N");
  DgradParams p;
  p.N = sh.N; p.H = sh.OH; p.W = sh.OW; p.PW = sh.OW / 2;
  p.G = g.G;
  p.WP = sh.OW + 2;
  p.img_pix = (sh.OH + 2) * (sh.OW + 2);
  p.hw = sh.OH * sh.OW;
  p.pgr = (sh.OH / 2) * (sh.OW / 2) * 8;
  p.m_pgr8 = make_magic((unsigned)(p.pgr / 8));
  p.m_pw = make_magic((unsigned)p.PW);
  p.m_hw = make_magic((unsigned)p.hw);
  p.m_w = make_magic((unsigned)p.W);
  const size_t lds =
      (size_t)std::max<long>(2L * g.G * g.img_lds, kDgWBytes);
  const int groups = (sh.N + g.G - 1) / g.G;
  int blocks = std::min(groups, kHaloMinBlocks * kNumCU);
  if (max_blocks > 0) blocks = std::min(blocks, max_blocks);
  static const bool attr_set = [] {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)halo_pool_dgrad_kernel<true>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHaloLdsBudget));
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)halo_pool_dgrad_kernel<false>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHaloLdsBudget));
    return true;
  }();
  (void)attr_set;
  auto* kern = dyf ? halo_pool_dgrad_kernel<true>
                   : halo_pool_dgrad_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks),
                     dim3(kHaloThreads), lds, cur_stream(),
                     (const bf16*)w.data_ptr(),
                     (const unsigned char*)y_pooled.data_ptr(),
                     (const unsigned char*)idx.data_ptr(),
                     (const unsigned char*)dy_pooled.data_ptr(),
                     dyf ? (unsigned char*)dyf->data_ptr() : nullptr,
                     (bf16*)dx.data_ptr(), p);
  HIP_CHECK(hipGetLastError());
}

bool halo_conv_geometry_ok(const ConvShape& sh) { return halo_geom(sh).ok; }

int halo_conv_group_images(const ConvShape& sh) { return halo_geom(sh).G; }

// The one gate of the halo route: its geometry, an unsplit (S == 1)
// gemm256 pooled-forward plan - whose chain the kernel issues - and the
// environment switch.
bool halo_conv_gate(const ConvShape& sh) {
  if (!halo_conv_env_gate() || !halo_geom(sh).ok) return false;
  const GemmPlan p = gemm_conv_plan(ConvEntry::kFwdPool, sh);
  return p.path == GemmPath::kGemm256 && p.S == 1;
}

void halo_conv_fwd_pool_launch(const torch::Tensor& x,
                               const torch::Tensor& w2, torch::Tensor& y,
                               const ConvShape& sh, const torch::Tensor* bias,
                               bool relu, uint8_t* idx, int max_blocks) {
  const HaloGeom g = halo_geom(sh);
  TORCH_CHECK(g.ok, "halo conv: shape outside the kernel's geometry");
  TORCH_CHECK((long)sh.N * sh.H * sh.W * 64 < (1L << 40), "halo conv: N");
  HaloParams p;
  p.N = sh.N; p.H = sh.H; p.W = sh.W;
  p.PH = sh.OH / 2; p.PW = sh.OW / 2;
  p.G = g.G; p.pitch = g.pitch; p.img_lds = g.img_lds;
  p.hw4 = sh.H * sh.W * 4;
  p.phw = p.PH * p.PW;
  p.m_hw4 = make_magic((unsigned)p.hw4);
  p.m_w = make_magic((unsigned)p.W);
  p.m_phw = make_magic((unsigned)p.phw);
  p.m_pw = make_magic((unsigned)p.PW);
  const size_t lds = (size_t)2 * g.G * g.img_lds;
  const int groups = (sh.N + g.G - 1) / g.G;
  int blocks = std::min(groups, kHaloMinBlocks * kNumCU);
  if (max_blocks > 0) blocks = std::min(blocks, max_blocks);
  auto* kern = idx ? halo_conv_pool_kernel<2> : halo_conv_pool_kernel<1>;
  static const bool attr_set = [] {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)halo_conv_pool_kernel<1>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHaloLdsBudget));
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)halo_conv_pool_kernel<2>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHaloLdsBudget));
    return true;
  }();
  (void)attr_set;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kHaloThreads), lds,
                     cur_stream(), (const unsigned char*)x.data_ptr(),
                     (const bf16*)w2.data_ptr(),
                     bias ? (const bf16*)bias->data_ptr() : nullptr,
                     (bf16*)y.data_ptr(), idx, relu ? 1 : 0, p);
  HIP_CHECK(hipGetLastError());
}

}  // namespace bflc
