// Extended local optimizer (gfx950): SGD with momentum / Nesterov,
// L2 weight decay, the FedProx proximal term, global-norm gradient
// clipping and a DEVICE-resident learning rate, fused into the one
// master-weight pass that runs per minibatch inside the whole-phase
// hipGraphs. The legacy sgd_master_ path (elementwise.hip) is untouched;
// this path is opt-in (FLConfig.extended_sgd).
//
// Three kernels, no atomics, no host sync, torch-allocator temporaries
// only, every launch geometry a function of n alone (the colsum_geom
// rule: results never depend on a device query):
//
//   grad_sumsq_part_kernel   per-block partial of sum(g^2), fp32
//   grad_clip_final_kernel   one block: partials -> ss -> coef (device)
//   sgdm_master_dev_kernel   the fused update, lr and coef read from
//                            device memory so a captured graph replays
//                            under a refilled lr without recapture
//
// All three are HBM-bound: 16-B accesses on every stream + scalar tail.

#include "common.h"
#include "sumsq.h"

#include <cstdint>
#include <tuple>
#include <type_traits>

namespace bflc {

namespace {

constexpr int kStepMaxBlocks = 2048;           // 8 blocks per CU

// part[block] = sum of g^2 over the block's lanes. Lane i (global) walks
// granules i, i + T, i + 2T, ... (T = gridDim * 256) in ascending order,
// eight fmaf(x, x, acc) per granule in element order, then (lane i <
// n % 8) the tail element n8*8 + i — one fp32 chain per lane.
template <class G>
__global__ __launch_bounds__(kOptBlock) void grad_sumsq_part_kernel(
    const G* __restrict__ g, float* __restrict__ part, long n) {
  const float acc = sumsq_lane(
      n, [&](long k, float (&x)[kGran]) { load8(g, k, x); },
      [&](long t) { return ld1(g, t); });
  const float s = block_sum_fixed(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One block. Lane t sums partials t, t + 256, ... ascending (<= 4), then
// the same fixed block reduction. coef = min(1, clip / (sqrt(ss) + 1e-6))
// (torch.nn.utils.clip_grad_norm_); a non-finite ss gives coef = 0, which
// makes the update kernel skip the step. out[0] = coef, out[1] = ss when
// the caller passed a 2-float buffer.
__global__ __launch_bounds__(kOptBlock) void grad_clip_final_kernel(
    const float* __restrict__ part, int nparts, float clip,
    float* __restrict__ out, int nout) {
  float acc = 0.f;
  for (int j = threadIdx.x; j < nparts; j += kOptBlock) acc += part[j];
  const float ss = block_sum_fixed(acc);
  if (threadIdx.x == 0) {
    float coef = 0.f;
    if (isfinite(ss)) {
      const float c = clip / (sqrtf(ss) + 1e-6f);
      coef = c < 1.f ? c : 1.f;  // within the clip: exactly 1.0f
    }
    out[0] = coef;
    if (nout > 1) out[1] = ss;
  }
}

// One element of the fused update. OPERATION ORDER (mirrored by the CPU
// oracle, ops/functional.py sgdm_step_): every input is widened exactly
// to fp64, the chain below runs in fp64 with fma() where written, and p
// and buf are each rounded to fp32 ONCE on store (shadow = bf16 of that
// fp32 p). The kernel is HBM-bound, the ~6 fp64 ops per element are
// free, and one rounding per stored value keeps |p - exact| <=
// 2^-24 |p| whatever cancels inside d.
//
//   g = coef * grad
//   g = fma(wd, p, g)                    only if wd != 0
//   g = fma(mu, p - p0, g)               PROX instantiations only
//   b = fma(mom, buf, g); buf = fp32(b)  MOM instantiations only
//   d = NEST ? fma(mom, b, g) : b        (d = g without momentum)
//   p = fp32(fma(-lr, d, p))
template <bool MOM, bool NEST, bool PROX>
__device__ __forceinline__ float sgdm_elem(float p, float grad, float& buf,
                                           float p0, double coef,
                                           double nlr, double mom,
                                           double wd, double mu) {
  const double pd = (double)p;
  double g = coef * (double)grad;
  if (wd != 0.0) g = fma(wd, pd, g);
  if (PROX) g = fma(mu, pd - (double)p0, g);
  double d = g;
  if (MOM) {
    const double b = fma(mom, (double)buf, g);
    buf = (float)b;
    d = NEST ? fma(mom, b, g) : b;
  }
  return (float)fma(nlr, d, pd);
}

// Grid-stride over 8-element granules + scalar tail. coef == 0 (set by
// grad_clip_final_kernel on a non-finite gradient) skips the whole step:
// p, buf and shadow stay bit-identical. buf is touched only in the MOM
// instantiations and p0 only in the PROX ones.
template <class G, bool SHADOW, bool MOM, bool NEST, bool PROX>
__global__ __launch_bounds__(kOptBlock) void sgdm_master_dev_kernel(
    float* __restrict__ p, bf16* __restrict__ shadow,
    const G* __restrict__ g, float* __restrict__ buf,
    const float* __restrict__ p0, const float* __restrict__ lr_dev,
    const float* __restrict__ coef_dev, double mom, double wd, double mu,
    long n) {
  const float coef_f = coef_dev[0];
  if (coef_f == 0.f) return;
  const double coef = (double)coef_f;
  const double nlr = -(double)lr_dev[0];
  const long i = (long)blockIdx.x * kOptBlock + threadIdx.x;
  const long stride = (long)gridDim.x * kOptBlock;
  const long n8 = n / kGran;
  for (long k = i; k < n8; k += stride) {
    float pv[kGran], gv[kGran], bv[kGran], qv[kGran];
    load8(p, k, pv);
    load8(g, k, gv);
    if (MOM) load8(buf, k, bv);
    if (PROX) load8(p0, k, qv);
#pragma unroll
    for (int j = 0; j < kGran; ++j) {
      float b = MOM ? bv[j] : 0.f;
      pv[j] = sgdm_elem<MOM, NEST, PROX>(pv[j], gv[j], b,
                                         PROX ? qv[j] : 0.f, coef, nlr,
                                         mom, wd, mu);
      if (MOM) bv[j] = b;
    }
    store8(p, k, pv);
    if (MOM) store8(buf, k, bv);
    if (SHADOW) {
      us8_t sv;
#pragma unroll
      for (int j = 0; j < kGran; ++j)
        sv[j] = __bfloat16_as_ushort(f2b(pv[j]));
      reinterpret_cast<us8_t*>(shadow)[k] = sv;
    }
  }
  for (long k = n8 * kGran + i; k < n; k += stride) {
    float b = MOM ? buf[k] : 0.f;
    const float v = sgdm_elem<MOM, NEST, PROX>(
        p[k], ld1(g, k), b, PROX ? p0[k] : 0.f, coef, nlr, mom, wd, mu);
    p[k] = v;
    if (MOM) buf[k] = b;
    if (SHADOW) shadow[k] = f2b(v);
  }
}

template <class F>
void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

inline int step_blocks(long n) {
  const long per_block = (long)kOptBlock * kGran;
  return (int)std::min<long>(std::max<long>((n + per_block - 1) / per_block, 1),
                             kStepMaxBlocks);
}

}  // namespace

void launch_grad_clip_final(const float* part, int nparts, float clip,
                            float* out, int nout) {
  hipLaunchKernelGGL(grad_clip_final_kernel, dim3(1), dim3(kOptBlock), 0,
                     cur_stream(), part, nparts, clip, out, nout);
  HIP_CHECK(hipGetLastError());
}

std::tuple<long, long, long> grad_sumsq_geom_query(long n) {
  TORCH_CHECK(n >= 0);
  const SumsqGeom s = sumsq_geom(n);
  return {s.blocks, s.per_lane, s.depth};
}

std::tuple<long, long, long> sgdm_step_geom_query(long n) {
  TORCH_CHECK(n >= 0);
  return {step_blocks(n), kOptBlock, kGran};
}

void grad_clip_coef_(torch::Tensor g, double clip, torch::Tensor out) {
  CHECK_GPU(g); CHECK_CONTIG(g); CHECK_ALIGN16(g);
  TORCH_CHECK(g.scalar_type() == at::kBFloat16 ||
                  g.scalar_type() == at::kFloat,
              "g must be bf16 or fp32");
  check_scalar_dev(out, "out");
  TORCH_CHECK(out.numel() <= 2, "out holds (coef) or (coef, sumsq)");
  TORCH_CHECK(clip > 0.0, "clip must be > 0");
  const long n = g.numel();
  const SumsqGeom s = sumsq_geom(n);
  auto part = torch::empty({s.blocks}, out.options());
  if (g.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(grad_sumsq_part_kernel<bf16>, dim3(s.blocks),
                       dim3(kOptBlock), 0, cur_stream(),
                       (const bf16*)g.data_ptr(), part.data_ptr<float>(), n);
  } else {
    hipLaunchKernelGGL(grad_sumsq_part_kernel<float>, dim3(s.blocks),
                       dim3(kOptBlock), 0, cur_stream(),
                       g.data_ptr<float>(), part.data_ptr<float>(), n);
  }
  HIP_CHECK(hipGetLastError());
  launch_grad_clip_final(part.data_ptr<float>(), s.blocks, (float)clip,
                         out.data_ptr<float>(), (int)out.numel());
}

// The second half of grad_clip_coef_ on partials a producer kernel wrote
// (delta_extract_sumsq_): same kernel, same coefficient bits.
void grad_clip_final_(torch::Tensor part, double clip, torch::Tensor out) {
  check_scalar_dev(part, "part");
  check_scalar_dev(out, "out");
  TORCH_CHECK(part.numel() <= kSumsqMaxBlocks, "part holds at most ",
              kSumsqMaxBlocks, " partials");
  TORCH_CHECK(out.numel() <= 2, "out holds (coef) or (coef, sumsq)");
  TORCH_CHECK(clip > 0.0, "clip must be > 0");
  launch_grad_clip_final(part.data_ptr<float>(), (int)part.numel(),
                         (float)clip, out.data_ptr<float>(),
                         (int)out.numel());
}

void sgdm_master_dev_(torch::Tensor p, c10::optional<torch::Tensor> shadow,
                      torch::Tensor g, torch::Tensor buf, torch::Tensor p0,
                      torch::Tensor lr_dev, torch::Tensor coef_dev,
                      double momentum, bool nesterov, double wd, double mu) {
  CHECK_GPU(p); CHECK_CONTIG(p); CHECK_ALIGN16(p);
  CHECK_GPU(g); CHECK_CONTIG(g); CHECK_ALIGN16(g);
  TORCH_CHECK(p.scalar_type() == at::kFloat, "p must be fp32");
  TORCH_CHECK(g.scalar_type() == at::kBFloat16 ||
                  g.scalar_type() == at::kFloat,
              "g must be bf16 or fp32");
  const long n = p.numel();
  TORCH_CHECK(g.numel() == n, "g and p differ in numel");
  TORCH_CHECK(momentum >= 0.0 && wd >= 0.0 && mu >= 0.0);
  TORCH_CHECK(!nesterov || momentum > 0.0, "nesterov needs momentum > 0");
  bf16* sh = nullptr;
  if (shadow.has_value()) {
    const torch::Tensor& s = *shadow;
    CHECK_GPU(s); CHECK_CONTIG(s); CHECK_ALIGN16(s);
    TORCH_CHECK(s.scalar_type() == at::kBFloat16, "shadow must be bf16");
    TORCH_CHECK(s.numel() == n, "shadow and p differ in numel");
    sh = (bf16*)s.data_ptr();
  }
  const bool mom = momentum > 0.0, prox = mu > 0.0;
  // buf / p0 are validated only where an instantiation touches them;
  // callers pass any tensor (e.g. a 1-element dummy) otherwise
  float* bp = nullptr;
  const float* qp = nullptr;
  if (mom) {
    CHECK_GPU(buf); CHECK_CONTIG(buf); CHECK_ALIGN16(buf);
    TORCH_CHECK(buf.scalar_type() == at::kFloat, "buf must be fp32");
    TORCH_CHECK(buf.numel() == n, "buf and p differ in numel");
    bp = buf.data_ptr<float>();
  }
  if (prox) {
    CHECK_GPU(p0); CHECK_CONTIG(p0); CHECK_ALIGN16(p0);
    TORCH_CHECK(p0.scalar_type() == at::kFloat, "p0 must be fp32");
    TORCH_CHECK(p0.numel() == n, "p0 and p differ in numel");
    qp = p0.data_ptr<float>();
  }
  check_scalar_dev(lr_dev, "lr_dev");
  check_scalar_dev(coef_dev, "coef_dev");
  if (n == 0) return;
  const int blocks = step_blocks(n);
  const bool gbf = g.scalar_type() == at::kBFloat16;
  dispatch_bool(gbf, [&](auto gb) {
    using G = std::conditional_t<decltype(gb)::value, bf16, float>;
    dispatch_bool(sh != nullptr, [&](auto shv) {
      dispatch_bool(mom, [&](auto mv) {
        dispatch_bool(mom && nesterov, [&](auto nv) {
          dispatch_bool(prox, [&](auto pv) {
            constexpr bool M = decltype(mv)::value;
            constexpr bool N = decltype(nv)::value;
            if constexpr (M || !N) {  // nesterov only with momentum
              hipLaunchKernelGGL(
                  (sgdm_master_dev_kernel<G, decltype(shv)::value, M, N,
                                          decltype(pv)::value>),
                  dim3(blocks), dim3(kOptBlock), 0, cur_stream(),
                  p.data_ptr<float>(), sh, (const G*)g.data_ptr(), bp, qp,
                  lr_dev.data_ptr<float>(), coef_dev.data_ptr<float>(),
                  momentum, wd, mu, n);
            }
          });
        });
      });
    });
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace bflc
