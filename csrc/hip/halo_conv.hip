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
// The fused grad-free stack (halo_conv_stack_kernel). In committee
// scoring the layer before is FEMNIST conv1 (3x3, C = 1, Kout = 32, ReLU,
// 2x2 pool), and one conv2 input image, 12.5 KB, is a pure function of
// 1.5 KB of raw pixels and 320 parameters. Run as two kernels, conv1
// writes that tensor to HBM and conv2 reads it straight back: 77 MB of a
// 101 MB round trip per 3072 images that the result does not need. With
// STACK the block fetches RAW images (one 16-B granule a thread per
// group) into small zero-ringed LDS images and COMPUTES the interior of
// its halo buffers: thin::conv_pool_chain (thin_pool_chain.h), the very
// helper gemm_thin_conv_pool_kernel calls, eight channels of one pixel
// per call, stored as one 16-B LDS write. The pooled conv1 activation
// never reaches HBM, one launch disappears, and the bits are those of the
// two kernels. conv1 is VALU work (144 packed FMAs an item) next to
// conv2's MFMA work, so the next group's items run inside this group's
// tile loop, one 64-item pass per tile - a group has as many of either -
// rather than as a phase of their own between barriers: two blocks of a
// CU that run their phases in step would leave the MFMA pipe idle during
// both stages and the VALU idle during both tile loops. Everything after
// the stage - B fragments, tile loop, tenth MFMA, POOL epilogue,
// persistent walk, double buffering - is the same code (STACK is a
// template parameter of the one body).
//
// The second half of the file is the same structure for that layer's
// data gradient, fed from the pooled tensors (halo_pool_dgrad_kernel).
#include "common.h"
#include "gemm_api.h"
#include "thin_pool_chain.h"

#include <cstdlib>

namespace bflc {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
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

// The first layer of the fused stack. Its raw images sit in LDS behind
// the two halo buffers, each inside a zero ring: pixel (iy, ix) of an
// image is bf16 element (iy + 1) * rpitch + ix + 4. Four elements of
// left margin (the ring is the last of them) keep every run of four
// pixels 8-byte aligned; rpitch = W1 + 8 leaves the right ring and
// three unused elements.
struct StackParams {
  const bf16* w1;  // [32,3,3,1]
  const bf16* b1;  // [32]
  int W1;          // raw image width, 2 * W
  int rpitch;      // ringed raw row, in pixels
  int rimg;        // ringed raw image, in bytes: (H1 + 2) * rpitch * 2
  int rgr;         // 16-B granules per raw image: H1 * W1 / 8
  int raw_off;     // LDS offset of the raw images
  int w_off;       // LDS offset of the fp32 weights [9][32] + bias [32]
  Magic m_w1;
};
constexpr int kStackKout1 = 32;
constexpr int kStackWBytes = (9 + 1) * kStackKout1 * 4;

// Row pitch (W+2)*64 + 32: the 16 lanes of one ds_read_b128 group hold
// both dy rows of four neighbouring windows - 8 pixels of a halo row at
// 64 B each cover the 16-B slots {0,16,64,80,128,144,192,208} mod 256,
// and a pitch that is 32 mod 64 puts the dy + 1 row on the other eight.
// (The launch bound's second argument counts waves per SIMD: a block
// puts kHaloThreads / 256 on each, so two blocks per CU leave a wave
// 256 VGPRs - the 144 of B, the prefetch and the accumulators fit
// without scratch.)
//
// STACK: x is the RAW [N,2H,2W,1] input of the layer before (3x3, C = 1,
// Kout = 32, stride 1, pad 1, ReLU, 2x2 pool), and the stage computes
// this layer's input images instead of copying them (header: "The fused
// grad-free stack"). Everything after the stage is the same code.
template <int POOLV, bool STACK>
__device__ __forceinline__ void halo_conv_pool_body(
    const unsigned char* __restrict__ x, const bf16* __restrict__ w2,
    const bf16* __restrict__ bias, bf16* __restrict__ y,
    uint8_t* __restrict__ pool_idx, int relu, const HaloParams& p,
    const StackParams& sp) {
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
  // (STACK: and the raw images behind them, whose ring the first layer's
  // out-of-image taps read as +0)
  {
    const u32x4_t z = {0u, 0u, 0u, 0u};
    const int zbytes = STACK ? sp.w_off : 2 * buf_bytes;
    for (int o = tid * 16; o < zbytes; o += kHaloThreads * 16)
      *reinterpret_cast<u32x4_t*>(smem + o) = z;
  }
  // STACK: the first layer's weights, fp32 and tap-major, and its bias
  float* w1l = reinterpret_cast<float*>(smem + (STACK ? sp.w_off : 0));
  if constexpr (STACK) {
    for (int i = tid; i < kStackKout1 * 9; i += kHaloThreads)
      w1l[(i % 9) * kStackKout1 + i / 9] = b2f(sp.w1[i]);
    if (tid < kStackKout1) w1l[9 * kStackKout1 + tid] = b2f(sp.b1[tid]);
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
  // STACK: one raw granule (eight pixels) a thread covers a group -
  // G * H * W * 4 <= kHaloPF * kHaloThreads pixels - and lands in the
  // ringed raw image as two runs of four (W1 % 4 == 0: a run stays in
  // its row)
  int rst[2] = {0, 0};
  if constexpr (STACK) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const unsigned e = tid * 8 + h * 4;  // pixel of the group
      const unsigned img = mdiv(e, p.m_hw4);  // H1 * W1 == hw4
      const unsigned rem = e - img * p.hw4;
      const unsigned iy = mdiv(rem, sp.m_w1), ix = rem - iy * sp.W1;
      rst[h] = (int)(sp.raw_off + img * sp.rimg +
                     ((iy + 1) * sp.rpitch + ix + 4) * 2);
    }
  }
  u32x4_t rpf;
  auto fetch = [&](int g) __attribute__((always_inline)) {
    const int gc = min(p.G, p.N - g * p.G);
    if constexpr (STACK) {
      const int ngr = gc * sp.rgr;
      const unsigned char* src = x + (long)g * p.G * sp.rgr * 16;
      if (tid < ngr)
        rpf = *reinterpret_cast<const u32x4_t*>(src + (long)tid * 16);
      return ngr;
    } else {
      const int ngr = gc * p.hw4;
      const unsigned char* src = x + (long)g * p.G * p.hw4 * 16;
#pragma unroll
      for (int i = 0; i < kHaloPF; ++i) {
        const int gi = tid + i * kHaloThreads;
        if (gi < ngr)
          pf[i] = *reinterpret_cast<const u32x4_t*>(src + (long)gi * 16);
      }
      return ngr;
    }
  };
  // STACK: a group's raw granules, registers -> the ringed raw images
  auto raw_put = [&](int ngr) __attribute__((always_inline)) {
    if (tid < ngr) {
      *reinterpret_cast<u32x2_t*>(smem + rst[0]) = u32x2_t{rpf.x, rpf.y};
      *reinterpret_cast<u32x2_t*>(smem + rst[1]) = u32x2_t{rpf.z, rpf.w};
    }
  };
  // STACK: conv1 + bias + ReLU + pool of one item = (channel octet, pixel
  // of this layer's input) of a group of npix pixels, from the raw
  // images into halo buffer `buf`. Octet-major, so that a wave reads one
  // octet's weights (a broadcast) but for three boundaries.
  auto conv1_item = [&](int buf, int npix, int item)
      __attribute__((always_inline)) {
    if (item < 4 * npix) {
      const int hw = p.hw4 >> 2;
      const int oct =
          (item >= npix) + (item >= 2 * npix) + (item >= 3 * npix);
      const unsigned pix = item - oct * npix;
      const unsigned img = mdiv(pix * 4, p.m_hw4);
      const unsigned rem = pix - img * hw;
      const unsigned py = mdiv(rem, p.m_w), px = rem - py * p.W;
      // patch rows 2py-1..2py+2, columns 2px-1..2px+2 of the raw image:
      // ringed elements 2px+3..2px+6, read as three aligned words
      const unsigned char* rp = smem + sp.raw_off + img * sp.rimg +
                                ((2 * py) * sp.rpitch + 2 * px + 2) * 2;
      thin::f32x2 pd[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned* rw =
            reinterpret_cast<const unsigned*>(rp + r * sp.rpitch * 2);
        const unsigned a = rw[0], b = rw[1], c = rw[2];
        const float f0 = __uint_as_float(a & 0xffff0000u);
        const float f1 = __uint_as_float(b << 16);
        const float f2 = __uint_as_float(b & 0xffff0000u);
        const float f3 = __uint_as_float(c << 16);
        pd[r][0] = thin::f32x2{f0, f0};
        pd[r][1] = thin::f32x2{f1, f1};
        pd[r][2] = thin::f32x2{f2, f2};
        pd[r][3] = thin::f32x2{f3, f3};
      }
      thin::bf16x8 out;
      thin::u8x8 oidx;
      thin::conv_pool_chain<false>(pd, w1l + oct * 8, kStackKout1,
                                   w1l + 9 * kStackKout1 + oct * 8, 1, out,
                                   oidx);
      *reinterpret_cast<thin::bf16x8*>(
          smem + buf * buf_bytes + img * p.img_lds + (py + 1) * p.pitch +
          (px + 1) * 64 + oct * 16) = out;
    }
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
  // STACK: the raw granules of the group after this one, in flight from
  // one iteration's tile loop to the top of the next
  int ngr_ahead = 0;
  {
    const int ngr = fetch(g);
    __syncthreads();  // zero fill done before the interior lands
    if constexpr (STACK) {
      raw_put(ngr);
      __syncthreads();
      const int npix = ngr * 2;  // raw pixels / 4: images * H * W
      for (int item = tid; item < 4 * npix; item += kHaloThreads)
        conv1_item(0, npix, item);
      if (g + (int)gridDim.x < ngroups) ngr_ahead = fetch(g + gridDim.x);
    } else {
      stage(0, ngr);
    }
  }
  __syncthreads();

  int cur = 0;
  for (; g < ngroups; g += gridDim.x) {
    const int gnext = g + gridDim.x;
    const bool has_next = gnext < ngroups;  // block-uniform
    int ngr_next = 0;
    if constexpr (STACK) {
      // the next group's raw images replace this one's, which the
      // barrier that closed the last iteration left unread; the fetch
      // two groups ahead takes over the registers
      ngr_next = ngr_ahead;
      raw_put(ngr_next);
      __syncthreads();
      ngr_ahead = 0;
      if (gnext + (int)gridDim.x < ngroups)
        ngr_ahead = fetch(gnext + gridDim.x);
    } else {
      if (has_next) ngr_next = fetch(gnext);
    }

    const int gc = min(p.G, p.N - g * p.G);
    const int npp = gc * p.phw;            // pooled pixels of this group
    const int ntiles = (npp + 3) >> 2;     // 16-row MFMA tiles
    const long pp0 = (long)g * p.G * p.phw;
    const unsigned char* lbuf = smem + cur * buf_bytes;

    // STACK: the next group's conv1 runs inside this group's tile loop,
    // one 64-item pass of the wave ahead of each of its tiles, so that a
    // wave alternates VALU and MFMA work a tile at a time and the SIMD's
    // other wave - the CU's other block - fills the gaps of either kind.
    // A group has as many passes as tiles (H * W / 16 an image); `npass`
    // covers a next group that is the larger one all the same.
    const int npix_next = ngr_next * 2;
    const int npass = STACK ? (4 * npix_next + 63) >> 6 : 0;
    const int nloop = STACK ? max(ntiles, npass) : ntiles;

    for (int mt = wr; mt < nloop; mt += WR) {
      if constexpr (STACK) {
        if (mt < npass) conv1_item(cur ^ 1, npix_next, mt * 64 + lane);
        if (mt >= ntiles) continue;
      }
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

    if constexpr (!STACK) {
      if (has_next) stage(cur ^ 1, ngr_next);
    }
    __syncthreads();
    cur ^= 1;
  }
}

template <int POOLV>
__launch_bounds__(kHaloThreads, kHaloMinBlocks * (kHaloThreads / 256))
__global__ void halo_conv_pool_kernel(const unsigned char* __restrict__ x,
                                      const bf16* __restrict__ w2,
                                      const bf16* __restrict__ bias,
                                      bf16* __restrict__ y,
                                      uint8_t* __restrict__ pool_idx,
                                      int relu, HaloParams p) {
  halo_conv_pool_body<POOLV, false>(x, w2, bias, y, pool_idx, relu, p,
                                    StackParams{});
}

// The grad-free conv stack: raw pixels in, the second layer's pooled
// output out, ReLU on both layers, no idx plane.
__launch_bounds__(kHaloThreads, kHaloMinBlocks * (kHaloThreads / 256))
__global__ void halo_conv_stack_kernel(const unsigned char* __restrict__ x,
                                       const bf16* __restrict__ w2,
                                       const bf16* __restrict__ bias,
                                       bf16* __restrict__ y, HaloParams p,
                                       StackParams sp) {
  halo_conv_pool_body<1, true>(x, w2, bias, y, nullptr, 1, p, sp);
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

// BFLC_HALO_STACK: 1 (default) lets the gated grad-free conv stack run
// as halo_conv_stack_kernel, 0 keeps the two calls (A/B runs; same bits).
bool halo_stack_env_gate() {
  static const bool v = [] {
    const char* e = getenv("BFLC_HALO_STACK");
    return (e ? atoi(e) : 1) != 0;
  }();
  return v;
}

// sh1: the thin first layer on the raw images; sh2: the halo layer on
// its pooled output. G starts from the halo kernel's (whose staging
// bound, G * H * W * 4 <= kHaloPF * kHaloThreads, is one raw granule a
// thread here) and gives way to the raw images and weights in LDS.
struct StackGeom {
  bool ok = false;
  int G = 0, pitch = 0, img_lds = 0;
  int rpitch = 0, rimg = 0, raw_off = 0, w_off = 0;
  long lds = 0;
};

StackGeom stack_geom(const ConvShape& sh1, const ConvShape& sh2) {
  StackGeom s;
  if (sh1.C != 1 || sh1.R != 3 || sh1.S != 3 || sh1.stride != 1 ||
      sh1.pad != 1 || sh1.Kout != kStackKout1 || sh1.N <= 0 ||
      sh1.H <= 0 || sh1.W <= 0 || sh1.H % 4 != 0 || sh1.W % 4 != 0 ||
      sh2.N != sh1.N || sh2.H != sh1.H / 2 || sh2.W != sh1.W / 2)
    return s;
  const HaloGeom h = halo_geom(sh2);
  if (!h.ok) return s;
  s.pitch = h.pitch;
  s.img_lds = h.img_lds;
  s.rpitch = sh1.W + 8;
  s.rimg = (sh1.H + 2) * s.rpitch * 2;
  for (int G = h.G; G >= 1; --G) {
    const long raw_off = 2L * G * h.img_lds;
    const long w_off = (raw_off + (long)G * s.rimg + 63) / 64 * 64;
    if (w_off + kStackWBytes > kHaloLdsBudget) continue;
    s.G = G;
    s.raw_off = (int)raw_off;
    s.w_off = (int)w_off;
    s.lds = w_off + kStackWBytes;
    s.ok = (long)G * sh1.H * sh1.W / 8 <= kHaloThreads;
    break;
  }
  return s;
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

bool halo_stack_geometry_ok(const ConvShape& sh1, const ConvShape& sh2) {
  return stack_geom(sh1, sh2).ok;
}

int halo_stack_group_images(const ConvShape& sh1, const ConvShape& sh2) {
  return stack_geom(sh1, sh2).G;
}

// The stack kernel's own part of the gate: its geometry, the halo gate
// of the second layer (whose chain it issues) and the environment
// switch. That the first layer would take the thin route, whose chain
// the stage issues, is the caller's to ask (conv2d.hip).
bool halo_stack_gate(const ConvShape& sh1, const ConvShape& sh2) {
  return halo_stack_env_gate() && stack_geom(sh1, sh2).ok &&
         halo_conv_gate(sh2);
}

void halo_stack_launch(const torch::Tensor& x, const torch::Tensor& w1,
                       const torch::Tensor& b1, const torch::Tensor& w2,
                       const torch::Tensor& b2, torch::Tensor& y,
                       const ConvShape& sh1, const ConvShape& sh2,
                       int max_blocks) {
  const StackGeom g = stack_geom(sh1, sh2);
  TORCH_CHECK(g.ok, "halo stack: shape outside the kernel's geometry");
  TORCH_CHECK((long)sh2.N * sh2.H * sh2.W * 64 < (1L << 40), "halo stack: N");
  TORCH_CHECK(w1.numel() == kStackKout1 * 9 && b1.numel() == kStackKout1 &&
              w2.numel() == 64 * 9 * 32 && b2.numel() == 64,
              "halo stack: parameter sizes");
  HaloParams p;
  p.N = sh2.N; p.H = sh2.H; p.W = sh2.W;
  p.PH = sh2.OH / 2; p.PW = sh2.OW / 2;
  p.G = g.G; p.pitch = g.pitch; p.img_lds = g.img_lds;
  p.hw4 = sh2.H * sh2.W * 4;
  p.phw = p.PH * p.PW;
  p.m_hw4 = make_magic((unsigned)p.hw4);
  p.m_w = make_magic((unsigned)p.W);
  p.m_phw = make_magic((unsigned)p.phw);
  p.m_pw = make_magic((unsigned)p.PW);
  StackParams sp;
  sp.w1 = (const bf16*)w1.data_ptr();
  sp.b1 = (const bf16*)b1.data_ptr();
  sp.W1 = sh1.W;
  sp.rpitch = g.rpitch;
  sp.rimg = g.rimg;
  sp.rgr = sh1.H * sh1.W / 8;
  sp.raw_off = g.raw_off;
  sp.w_off = g.w_off;
  sp.m_w1 = make_magic((unsigned)sh1.W);
  const int groups = (sh2.N + g.G - 1) / g.G;
  int blocks = std::min(groups, kHaloMinBlocks * kNumCU);
  if (max_blocks > 0) blocks = std::min(blocks, max_blocks);
  static const bool attr_set = [] {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)halo_conv_stack_kernel,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHaloLdsBudget));
    return true;
  }();
  (void)attr_set;
  hipLaunchKernelGGL(halo_conv_stack_kernel, dim3((unsigned)blocks),
                     dim3(kHaloThreads), (size_t)g.lds, cur_stream(),
                     (const unsigned char*)x.data_ptr(),
                     (const bf16*)w2.data_ptr(), (const bf16*)b2.data_ptr(),
                     (bf16*)y.data_ptr(), p, sp);
  HIP_CHECK(hipGetLastError());
}

}  // namespace bflc
