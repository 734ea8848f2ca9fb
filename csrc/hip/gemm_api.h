// Internal API between the GEMM translation unit and its users (linear,
// conv). All tensors bf16 on GPU; accumulation fp32 in MFMA AGPRs.
#pragma once

#include <torch/extension.h>

#include <string>
#include <tuple>

#include "gemm_plan.h"

namespace bflc {

// NHWC convolution geometry (shared by conv2d.hip and the implicit-
// GEMM staging in gemm_bf16.hip).
#if defined(__HIPCC__) || defined(__HIP__)
#define BFLC_HD __host__ __device__
#else
#define BFLC_HD
#endif

struct ConvShape {
  int N, C, H, W, Kout, R, S, stride, pad, OH, OW;
  BFLC_HD long M() const { return (long)N * OH * OW; }
  BFLC_HD long RSC() const { return (long)R * S * C; }
};

// Epilogue store modes.
enum class EpStore : int {
  kPlain = 0,   // C[m * N + n]
  kConvNCHW = 1,  // m=(img,ohw) rows: C[((m/OHW)*N + n)*OHW + m%OHW]
};

// C[M,N] = A op B (+bias), fp32 accumulate, bf16 in/out.
//   ta: A accessed as A[k*M + m] (stored [K,M]), else A[m*K + k]
//   tb: B accessed as B[n*K + k] (stored [N,K]), else B[k*N + n]
//   bias: optional [N] bf16 added per column; relu: fused max(0,.)
//   ohw: only for EpStore::kConvNCHW
// bn_stats (optional out): when non-null and the launch runs as a
// single K slice, receives fused per-tile-row channel partials
// (psum, psq), each [chunks][N] fp32, finalized by bn_stats_finalize.
// Left empty when the shape took a split-K or unsupported path.
void gemm_bf16_raw(const torch::Tensor& A, const torch::Tensor& B,
                   torch::Tensor& C, long M, long N, long K, bool ta, bool tb,
                   const torch::Tensor* bias, bool relu, EpStore store,
                   long ohw,
                   std::pair<torch::Tensor, torch::Tensor>* bn_stats
                   = nullptr);

// What the route queries report of a plan: (path, bm, bn, S, kslice).
using PlanRow = std::tuple<std::string, long, long, long, long>;
inline PlanRow plan_row(const GemmPlan& p) {
  return {gemm_path_name(p.path), p.bm, p.bn, p.S, p.kslice};
}
// The plan gemm_bf16_raw takes for a plain-store call without bn_stats.
PlanRow gemm_plan_route(long M, long N, long K, bool ta, bool tb);
// That plan itself, and the plain-store split-K reduce that call ends
// with (part [S, M, N] fp32 -> out [M, N] bf16): for a kernel that feeds
// the same MFMA chains per slice without going through gemm_bf16_raw.
GemmPlan gemm_dense_plan(long M, long N, long K, bool ta, bool tb);
void splitk_reduce_plain(const torch::Tensor& part, torch::Tensor& out);

// The implicit-GEMM conv entries below and the plan each launches
// (path "none": the entry returns false for this shape). Pure host
// code: allocates and launches nothing.
enum class ConvEntry { kFwd, kFwdPool, kDgrad, kWgrad };
GemmPlan gemm_conv_plan(ConvEntry e, const ConvShape& sh);

// col-free thin conv forward (grad-free path): A gathered from the
// NHWC window, no im2col matrix. w2p is the KT-padded weight.
bool gemm_thin_conv_raw(const torch::Tensor& x, const torch::Tensor& w2p,
                        torch::Tensor& y, const ConvShape& sh,
                        const torch::Tensor* bias, bool relu);

// Implicit-GEMM NHWC conv forward: y[M, Kout] = im2col(x) @ w2^T with
// the im2col gather fused into the GEMM's A staging (no col matrix).
// Requires sh.C % 8 == 0 and M >= 48; returns false if the shape
// cannot take this path (caller materializes col instead).
bool gemm_conv_fwd_raw(const torch::Tensor& x, const torch::Tensor& w2,
                       torch::Tensor& y, const ConvShape& sh,
                       const torch::Tensor* bias, bool relu,
                       std::pair<torch::Tensor, torch::Tensor>* bn_stats
                       = nullptr);

// Grad-free conv forward with the 2x2/stride-2 maxpool fused into the
// epilogue: y is [N, OH/2, OW/2, Kout] and is bitwise what the plain
// forward followed by the index-free maxpool gives. The *_eligible
// predicates name the shapes each fused kernel takes (the route query
// and the launchers share them); *_raw return false otherwise.
bool gemm_conv_fwd_pool_eligible(const ConvShape& sh);
// idx (optional, [N, OH/2, OW/2, Kout] u8): the training forward also
// gets the argmax code dy*2 + dx of each window, chosen as
// maxpool2d_fwd chooses it (strict > from -inf on the rounded values).
// halo: which kernel a gated shape (halo_conv_gate) runs - kAuto the
// halo kernel, kOff gemm256_kernel as if the gate were closed, kForce
// the halo kernel on its geometry alone (halo_conv_geometry_ok; tests
// and the op benchmark, the bits are the unsplit chain's).
// max_blocks > 0 caps the halo kernel's grid.
enum class HaloMode { kAuto, kOff, kForce };
bool gemm_conv_fwd_pool_raw(const torch::Tensor& x, const torch::Tensor& w2,
                            torch::Tensor& y, const ConvShape& sh,
                            const torch::Tensor* bias, bool relu,
                            uint8_t* idx = nullptr,
                            HaloMode halo = HaloMode::kAuto,
                            int max_blocks = 0);

// Halo-tile pooled conv forward (halo_conv.hip): C == 32, 3x3, stride
// 1, pad 1, Kout == 64, even OH/OW, whole zero-ringed images in LDS.
// Bitwise gemm256_kernel's single-slice pooled forward.
bool halo_conv_geometry_ok(const ConvShape& sh);
// images a block stages per group for this geometry (0: not eligible)
int halo_conv_group_images(const ConvShape& sh);
// geometry && the fwd_pool plan is an unsplit gemm256 && BFLC_HALO_CONV
bool halo_conv_gate(const ConvShape& sh);
void halo_conv_fwd_pool_launch(const torch::Tensor& x,
                               const torch::Tensor& w2, torch::Tensor& y,
                               const ConvShape& sh, const torch::Tensor* bias,
                               bool relu, uint8_t* idx, int max_blocks);
// The grad-free conv stack as one kernel (halo_conv.hip): sh1 is a thin
// first layer (3x3, C == 1, Kout == 32, stride 1, pad 1, H and W
// multiples of 4) on raw [N,H1,W1,1] images, sh2 the halo layer above on
// its pooled output. Each block computes its sh2 input images in LDS with
// the thin pooled kernel's per-output chain (thin_pool_chain.h), so y is
// bitwise gemm_thin_conv_pool_raw then halo_conv_fwd_pool_launch, ReLU on
// both, while the pooled sh1 activation never reaches HBM.
bool halo_stack_geometry_ok(const ConvShape& sh1, const ConvShape& sh2);
// images a block computes per group (0: not eligible)
int halo_stack_group_images(const ConvShape& sh1, const ConvShape& sh2);
// geometry && halo_conv_gate(sh2) && BFLC_HALO_STACK; the caller adds
// that sh1 takes the thin route
bool halo_stack_gate(const ConvShape& sh1, const ConvShape& sh2);
void halo_stack_launch(const torch::Tensor& x, const torch::Tensor& w1,
                       const torch::Tensor& b1, const torch::Tensor& w2,
                       const torch::Tensor& b2, torch::Tensor& y,
                       const ConvShape& sh1, const ConvShape& sh2,
                       int max_blocks);
// Halo-tile data gradient of that layer's pooled backward
// (halo_conv.hip): Kout == 64 -> C == 32, 3x3, stride 1, pad 1, even
// OH/OW. Unpools the pooled (dy, y, idx) into zero-ringed LDS images,
// writes the masked full-resolution plane dyf [N, OH, OW, Kout] (bitwise
// pool_relu_bwd_colsum's) for the weight gradient and dx [N, H, W, C]
// (bitwise the unsplit implicit dgrad's on that plane); w is read as it
// is, no permuted copy. dyf == nullptr: the plane is not written.
bool halo_dgrad_geometry_ok(const ConvShape& sh);
// images a block unpools per group for this geometry (0: not eligible)
int halo_dgrad_group_images(const ConvShape& sh);
// geometry && the dgrad plan is unsplit && M * Kout < 2^31 &&
// BFLC_HALO_DGRAD
bool halo_dgrad_gate(const ConvShape& sh);
void halo_pool_dgrad_launch(const torch::Tensor& w,
                            const torch::Tensor& y_pooled,
                            const torch::Tensor& idx,
                            const torch::Tensor& dy_pooled,
                            torch::Tensor* dyf, torch::Tensor& dx,
                            const ConvShape& sh, int max_blocks);
// Thin pooled first layer (3x3, C == 1, stride 1, M >= 65536): w2 is
// the UNPADDED [Kout, 9] weight view.
bool gemm_thin_conv_pool_eligible(const ConvShape& sh);
bool gemm_thin_conv_pool_raw(const torch::Tensor& x,
                             const torch::Tensor& w2, torch::Tensor& y,
                             const ConvShape& sh, const torch::Tensor* bias,
                             bool relu, uint8_t* idx = nullptr);

// Implicit-GEMM NHWC conv data-gradient: dx[M, C] = dy-gather @ wrot2
// (wrot2[c][(r,s,kout)] = w[kout][r][s][c], i.e. w.permute(3,1,2,0)
// viewed [C, R*S*Kout]; r,s indices walk the SAME orientation as the
// forward because the gather uses oh = (ih + pad - r)/stride).
// Requires sh.Kout % 8 == 0; false => caller uses dcol + col2im.
bool gemm_conv_dgrad_raw(const torch::Tensor& dy, const torch::Tensor& wrot2,
                         torch::Tensor& dx, const ConvShape& sh);

// Implicit-GEMM NHWC conv weight-gradient: dW[Kout, RSC] = dy2^T @
// implicit-col(x) — no col matrix. Requires sh.C % 8 == 0.
bool gemm_conv_wgrad_raw(const torch::Tensor& dy2, const torch::Tensor& x,
                         torch::Tensor& dw, const ConvShape& sh);

// colsum: out[n] = sum_m X[m,n]  (bias gradient)
torch::Tensor colsum_bf16(const torch::Tensor& X);
// colsum's second pass over fp32 partials [chunks][N] -> bf16 out[N];
// colsum_geom (gemm_plan.h) gives the first pass's chunking.
void colsum_finalize(const torch::Tensor& part, torch::Tensor& out);
// fused relu-backward + bias-grad column sum: (dx, db)
std::tuple<torch::Tensor, torch::Tensor> relu_bwd_colsum(
    const torch::Tensor& y, const torch::Tensor& dy);

// LDS-tiled bf16 transpose: out[C][R] = X[R][C]^T (16-B coalesced both
// sides). Used to put GEMM operands into the vector-staging layout.
torch::Tensor transpose_bf16(const torch::Tensor& X);

}  // namespace bflc
