// pybind11 bindings for the bflc_amd gfx950 HIP kernels.
#include <torch/extension.h>

#include <string>
#include <tuple>
#include <vector>

namespace bflc {

// elementwise.hip
void axpy_(torch::Tensor y, torch::Tensor x, double alpha);
void sgd_step_(torch::Tensor p, torch::Tensor g, double lr);
void adam_step_(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                torch::Tensor v, long step, double lr, double beta1,
                double beta2, double eps);
torch::Tensor weighted_fedavg(torch::Tensor deltas, torch::Tensor w);
void sgd_master_(torch::Tensor p, torch::Tensor shadow, torch::Tensor g,
                 double lr);
void adam_master_(torch::Tensor p, torch::Tensor shadow, torch::Tensor g,
                  torch::Tensor m, torch::Tensor v, long step, double lr,
                  double beta1, double beta2, double eps);
void adam_master_graph_(torch::Tensor p, torch::Tensor shadow,
                        torch::Tensor g, torch::Tensor m, torch::Tensor v,
                        torch::Tensor step, torch::Tensor bc, double lr,
                        double beta1, double beta2, double eps);
void refresh_shadow_(torch::Tensor p, torch::Tensor shadow);
void score_load_(torch::Tensor shadow, torch::Tensor global_flat,
                 torch::Tensor delta, double lr);
void delta_extract_(torch::Tensor out, torch::Tensor global_flat,
                    torch::Tensor w, double lr);
torch::Tensor relu_fwd(torch::Tensor x);
torch::Tensor relu_bwd(torch::Tensor y, torch::Tensor dy);
std::tuple<torch::Tensor, torch::Tensor> relu_bwd_colsum(
    const torch::Tensor& y, const torch::Tensor& dy);

// optimizer.hip
std::tuple<long, long, long> grad_sumsq_geom_query(long n);
std::tuple<long, long, long> sgdm_step_geom_query(long n);
void grad_clip_coef_(torch::Tensor g, double clip, torch::Tensor out);
void sgdm_master_dev_(torch::Tensor p, c10::optional<torch::Tensor> shadow,
                      torch::Tensor g, torch::Tensor buf, torch::Tensor p0,
                      torch::Tensor lr_dev, torch::Tensor coef_dev,
                      double momentum, bool nesterov, double wd, double mu);
void grad_clip_final_(torch::Tensor part, double clip, torch::Tensor out);

// privacy.hip
void delta_extract_sumsq_(torch::Tensor out, torch::Tensor global_flat,
                          torch::Tensor w, double lr, torch::Tensor part);
void dp_privatize_(torch::Tensor d, torch::Tensor coef_dev, double sigma,
                   uint64_t seed, uint64_t stream, uint64_t epoch);
torch::Tensor dp_philox_words(torch::Tensor ctr, uint64_t key0,
                              uint64_t key1);

// aggregate.hip
torch::Tensor order_stat_mean(torch::Tensor deltas, long t);
torch::Tensor delta_gram(torch::Tensor deltas);
std::tuple<long, long> delta_gram_geom_query(long P);
torch::Tensor masked_wmean(torch::Tensor deltas, torch::Tensor w);

// softmax_ce.hip
std::tuple<torch::Tensor, torch::Tensor> softmax_ce_fwd(torch::Tensor logits,
                                                        torch::Tensor target);
torch::Tensor softmax_ce_bwd(torch::Tensor probs, torch::Tensor target,
                             torch::Tensor gloss);

// reduce.hip
double accuracy(torch::Tensor logits, torch::Tensor target);
torch::Tensor accuracy_t(torch::Tensor logits, torch::Tensor target);

// gemm_bf16.hip
torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                         bool relu);
torch::Tensor gemm_raw(torch::Tensor A, torch::Tensor B, bool ta, bool tb);
using PlanRow = std::tuple<std::string, long, long, long, long>;
PlanRow gemm_plan_route(long M, long N, long K, bool ta, bool tb);
std::tuple<long, long, long, long> colsum_geom_query(long M, long N);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> linear_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor dy, bool want_dx);

// conv_im2col.hip
std::tuple<torch::Tensor, torch::Tensor> conv2d_fwd_col(
    torch::Tensor x, torch::Tensor w, torch::Tensor b, long stride, long pad,
    bool relu, bool want_col);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
conv2d_fwd_bn(torch::Tensor x, torch::Tensor w, long stride, long pad);
std::tuple<torch::Tensor, torch::Tensor> bn_stats(torch::Tensor x,
                                                  double eps);
std::tuple<torch::Tensor, torch::Tensor> bn_stats_finalize(
    torch::Tensor psum, torch::Tensor psq, double count, double eps);
torch::Tensor batchnorm_norm(torch::Tensor x, torch::Tensor gamma,
                             torch::Tensor beta, torch::Tensor mean,
                             torch::Tensor invstd, bool relu,
                             c10::optional<torch::Tensor> residual);
torch::Tensor conv2d_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                         long stride, long pad, bool relu);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> conv2d_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor dy, long stride,
    long pad, c10::optional<torch::Tensor> col_cache, bool want_db,
    bool want_dx);
std::tuple<torch::Tensor, torch::Tensor> maxpool2d_fwd(torch::Tensor x,
                                                       long kernel,
                                                       long stride,
                                                       bool want_idx);
torch::Tensor maxpool2d_bwd(torch::Tensor dy, torch::Tensor idx,
                            std::vector<long> in_shape, long kernel,
                            long stride);
torch::Tensor conv2d_relu_pool_fwd(torch::Tensor x, torch::Tensor w,
                                   torch::Tensor b, long stride, long pad,
                                   long max_blocks, std::string impl);
std::string conv_fwd_pool_impl(std::vector<long> x_shape,
                               std::vector<long> w_shape, long stride,
                               long pad);
torch::Tensor conv_relu_pool_stack_fwd(torch::Tensor x, torch::Tensor w1,
                                       torch::Tensor b1, torch::Tensor w2,
                                       torch::Tensor b2, long max_blocks,
                                       std::string impl);
std::string conv_relu_pool_stack_route(std::vector<long> x_shape,
                                       std::vector<long> w1_shape,
                                       std::vector<long> w2_shape);
long halo_stack_group_images_query(std::vector<long> x_shape,
                                   std::vector<long> w1_shape,
                                   std::vector<long> w2_shape);
long halo_conv_group_images_query(std::vector<long> x_shape,
                                  std::vector<long> w_shape, long stride,
                                  long pad);
std::string conv2d_relu_pool_route(std::vector<long> x_shape,
                                   std::vector<long> w_shape, long stride,
                                   long pad);
PlanRow conv_plan_route(const std::string& entry, std::vector<long> x_shape,
                        std::vector<long> w_shape, long stride, long pad);
std::tuple<torch::Tensor, torch::Tensor> conv2d_relu_pool_fwd_idx(
    torch::Tensor x, torch::Tensor w, torch::Tensor b, long stride,
    long pad, long max_blocks, std::string impl);
std::tuple<torch::Tensor, torch::Tensor> pool_relu_bwd_colsum(
    torch::Tensor y_pooled, torch::Tensor idx, torch::Tensor dy_pooled,
    std::vector<long> out_shape);
std::tuple<torch::Tensor, torch::Tensor> thin_conv_pool_wgrad(
    torch::Tensor x, torch::Tensor y_pooled, torch::Tensor idx,
    torch::Tensor dy_pooled, long stride, long pad);
std::tuple<torch::Tensor, torch::Tensor> thin_conv_pool_wgrad_fused(
    torch::Tensor x, torch::Tensor y_pooled, torch::Tensor idx,
    torch::Tensor dy_pooled, long stride, long pad);
std::string thin_pool_wgrad_impl(std::vector<long> x_shape,
                                 std::vector<long> w_shape, long stride,
                                 long pad, bool want_dx);
std::string conv2d_relu_pool_bwd_route(std::vector<long> x_shape,
                                       std::vector<long> w_shape,
                                       long stride, long pad, bool want_dx,
                                       bool allow_direct);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> conv2d_relu_pool_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor y_pooled,
    torch::Tensor idx, torch::Tensor dy_pooled, long stride, long pad,
    bool want_db, bool want_dx, bool allow_direct, std::string dgrad_impl,
    long max_blocks);
std::string pool_dgrad_impl(std::vector<long> x_shape,
                            std::vector<long> w_shape, long stride, long pad,
                            bool want_dx);
long halo_dgrad_group_images_query(std::vector<long> x_shape,
                                   std::vector<long> w_shape, long stride,
                                   long pad);
std::tuple<torch::Tensor, torch::Tensor> halo_pool_dgrad(
    torch::Tensor w, torch::Tensor y_pooled, torch::Tensor idx,
    torch::Tensor dy_pooled, long max_blocks, bool store_plane);

// batchnorm.hip
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> batchnorm_fwd(
    torch::Tensor x, torch::Tensor gamma, torch::Tensor beta, double eps,
    bool relu, c10::optional<torch::Tensor> residual);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> batchnorm_bwd(
    torch::Tensor x, torch::Tensor dy, torch::Tensor mean,
    torch::Tensor invstd, torch::Tensor gamma,
    c10::optional<torch::Tensor> y_relu);
torch::Tensor global_avgpool_fwd(torch::Tensor x);
torch::Tensor global_avgpool_bwd(torch::Tensor dy, long H, long W);
torch::Tensor add_relu_fwd(torch::Tensor a, torch::Tensor b);
torch::Tensor add_relu_bwd(torch::Tensor y, torch::Tensor dy);

// groupnorm.hip
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> groupnorm_fwd(
    torch::Tensor x, torch::Tensor gamma, torch::Tensor beta, long groups,
    double eps, bool relu, c10::optional<torch::Tensor> residual);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> groupnorm_bwd(
    torch::Tensor x, torch::Tensor dy, torch::Tensor mean, torch::Tensor rstd,
    torch::Tensor gamma, long groups, c10::optional<torch::Tensor> y_relu);
std::string groupnorm_route(long H, long W, long C, long groups);

}  // namespace bflc

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "bflc_amd hand-written gfx950 (CDNA4) HIP kernels";
  m.def("axpy_", &bflc::axpy_, "y += alpha*x (fp32, in place)");
  m.def("sgd_step_", &bflc::sgd_step_, "fused flat SGD");
  m.def("adam_step_", &bflc::adam_step_, "fused flat Adam");
  m.def("weighted_fedavg", &bflc::weighted_fedavg,
        "fixed-order weighted FedAvg reduce");
  m.def("sgd_master_", &bflc::sgd_master_,
        "fused fp32-master SGD + bf16 shadow refresh");
  m.def("adam_master_", &bflc::adam_master_);
  m.def("adam_master_graph_", &bflc::adam_master_graph_,
        "hipGraph-capturable Adam: device step counter + on-device bias "
        "corrections (tick kernel), fp32 master + bf16 shadow");
  m.def("refresh_shadow_", &bflc::refresh_shadow_, "shadow = bf16(master)");
  m.def("score_load_", &bflc::score_load_,
        "shadow = compute_dtype(global - lr*delta): one-pass scoring "
        "candidate load (replaces copy+axpy+set_flat)");
  m.def("delta_extract_", &bflc::delta_extract_,
        "out = (global - w)/lr: one-pass pseudo-gradient extraction");
  m.def("grad_sumsq_geom", &bflc::grad_sumsq_geom_query,
        "sum-of-squares geometry of an n-element gradient: (blocks, "
        "longest lane chain in elements, adds after the lane chain)",
        py::arg("n"));
  m.def("sgdm_step_geom", &bflc::sgdm_step_geom_query,
        "launch of sgdm_master_dev_ at n elements: (blocks, threads, "
        "elements per thread per grid-stride pass)",
        py::arg("n"));
  m.def("grad_clip_coef_", &bflc::grad_clip_coef_,
        "out[0] = min(1, clip / (||g||_2 + 1e-6)), 0 if the norm is not "
        "finite; out[1] = sum(g^2) when out has two elements",
        py::arg("g"), py::arg("clip"), py::arg("out"));
  m.def("sgdm_master_dev_", &bflc::sgdm_master_dev_,
        "fused SGD (momentum / nesterov / weight decay / FedProx / clip "
        "coefficient) on the fp32 master (+ bf16 shadow); lr and coef are "
        "device floats",
        py::arg("p"), py::arg("shadow"), py::arg("g"), py::arg("buf"),
        py::arg("p0"), py::arg("lr_dev"), py::arg("coef_dev"),
        py::arg("momentum"), py::arg("nesterov"), py::arg("wd"),
        py::arg("mu"));
  m.def("grad_clip_final_", &bflc::grad_clip_final_,
        "grad_clip_coef_'s second kernel on per-block partials of a sum "
        "of squares: out[0] = coef, out[1] = the sum",
        py::arg("part"), py::arg("clip"), py::arg("out"));
  m.def("delta_extract_sumsq_", &bflc::delta_extract_sumsq_,
        "out = (global - w)/lr (delta_extract_'s bits) and, in the same "
        "pass, part = per-block partials of sum(out^2) in "
        "grad_clip_coef_'s order; part has grad_sumsq_geom(n)[0] elements",
        py::arg("out"), py::arg("global_flat"), py::arg("w"), py::arg("lr"),
        py::arg("part"));
  m.def("dp_privatize_", &bflc::dp_privatize_,
        "in place d[i] = fmaf(coef, d[i], sigma * z(i)) with the "
        "Philox4x32-10 / Box-Muller normal z of (seed, stream, epoch, i); "
        "coef is a device float, coef == 0 publishes the noise alone, "
        "sigma == 0 is the clip alone",
        py::arg("d"), py::arg("coef_dev"), py::arg("sigma"), py::arg("seed"),
        py::arg("stream"), py::arg("epoch"));
  m.def("dp_philox_words", &bflc::dp_philox_words,
        "Philox4x32-10 of the [N, 4] int64 counters under (key0, key1): "
        "[N, 4] int64 words (test hook of dp_privatize_'s generator)",
        py::arg("ctr"), py::arg("key0"), py::arg("key1"));
  m.def("order_stat_mean", &bflc::order_stat_mean,
        "per coordinate: sort the K values (NaN above +inf), drop t at "
        "each end, ascending fp32 sum / (K - 2t); [K, P] fp32, K <= 32",
        py::arg("deltas"), py::arg("t"));
  m.def("delta_gram", &bflc::delta_gram,
        "G = D D^T of the [K, P] fp32 stack on the f32-input MFMA, "
        "fixed-order two-stage reduction; K <= 32",
        py::arg("deltas"));
  m.def("delta_gram_geom", &bflc::delta_gram_geom_query,
        "stage-1 geometry of delta_gram at P coordinates: (blocks, "
        "coordinates per block)",
        py::arg("P"));
  m.def("masked_wmean", &bflc::masked_wmean,
        "sum_k w[k] d[k] / sum(w) by fmaf in ascending k, any P; rows "
        "with w[k] == 0 are not read",
        py::arg("deltas"), py::arg("w"));
  m.def("relu_fwd", &bflc::relu_fwd);
  m.def("relu_bwd", &bflc::relu_bwd);
  m.def("relu_bwd_colsum", &bflc::relu_bwd_colsum,
        "fused relu backward + bias-grad column sum: (dx, db)");
  m.def("softmax_ce_fwd", &bflc::softmax_ce_fwd,
        "fused softmax cross-entropy fwd (loss, probs)");
  m.def("softmax_ce_bwd", &bflc::softmax_ce_bwd);
  m.def("accuracy", &bflc::accuracy, "fused argmax-compare-reduce");
  m.def("accuracy_t", &bflc::accuracy_t,
        "accuracy as a device tensor (no host sync)");
  m.def("linear_fwd", &bflc::linear_fwd, "MFMA bf16 GEMM + bias (+relu)",
        py::arg("x"), py::arg("w"), py::arg("b"), py::arg("relu") = false);
  m.def("gemm_raw", &bflc::gemm_raw, "raw GEMM (bench/ablation)");
  m.def("gemm_plan_route", &bflc::gemm_plan_route,
        "plan gemm_raw takes: (thin | gemm8p | gemm256 | small, bm, bn, S, "
        "kslice)",
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("ta"),
        py::arg("tb"));
  m.def("conv_plan_route", &bflc::conv_plan_route,
        "plan of the implicit-GEMM conv entry fwd | fwd_pool | dgrad | "
        "wgrad: (none | gemm256 | small, bm, bn, S, kslice)",
        py::arg("entry"), py::arg("x_shape"), py::arg("w_shape"),
        py::arg("stride"), py::arg("pad"));
  m.def("colsum_geom", &bflc::colsum_geom_query,
        "colsum pass-1 geometry of an [M, N] matrix: (G, cblocks, rows, "
        "chunks)",
        py::arg("M"), py::arg("N"));
  m.def("linear_bwd", &bflc::linear_bwd,
        "(dx, dw, db) - dx empty unless want_dx", py::arg("x"),
        py::arg("w"), py::arg("dy"), py::arg("want_dx") = true);
  m.def("conv2d_fwd", &bflc::conv2d_fwd,
        "NHWC implicit-GEMM convolution (MFMA); inference entry, no col",
        py::arg("x"), py::arg("w"), py::arg("b"), py::arg("stride"),
        py::arg("pad"), py::arg("relu") = false);
  m.def("conv2d_fwd_col", &bflc::conv2d_fwd_col, "(y, col) - col for bwd",
        py::arg("x"), py::arg("w"), py::arg("b"), py::arg("stride"),
        py::arg("pad"), py::arg("relu") = false,
        py::arg("want_col") = true);
  m.def("conv2d_fwd_bn", &bflc::conv2d_fwd_bn,
        "(y, col, psum, psq) - conv with fused epilogue BN stats");
  m.def("bn_stats", &bflc::bn_stats, "(mean, invstd) of x [.., C]");
  m.def("bn_stats_finalize", &bflc::bn_stats_finalize,
        "(mean, invstd) from [chunks][C] partials");
  m.def("batchnorm_norm", &bflc::batchnorm_norm,
        py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("mean"),
        py::arg("invstd"), py::arg("relu"),
        py::arg("residual") = py::none(),
        "normalization pass with known stats");
  m.def("conv2d_bwd", &bflc::conv2d_bwd,
        "(dx, dw, db) - db empty unless want_db, dx empty unless "
        "want_dx (first-layer convs need no input gradient)",
        py::arg("x"), py::arg("w"), py::arg("dy"), py::arg("stride"),
        py::arg("pad"), py::arg("col_cache") = py::none(),
        py::arg("want_db") = true, py::arg("want_dx") = true);
  m.def("maxpool2d_fwd", &bflc::maxpool2d_fwd, py::arg("x"),
        py::arg("kernel"), py::arg("stride"),
        py::arg("want_idx") = true);
  m.def("maxpool2d_bwd", &bflc::maxpool2d_bwd);
  m.def("conv2d_relu_pool_fwd", &bflc::conv2d_relu_pool_fwd,
        "grad-free conv + bias + ReLU + 2x2/2 maxpool, pooled in the conv "
        "epilogue where a fused route applies: [N, OH/2, OW/2, Kout]. "
        "max_blocks > 0 caps the halo kernel's grid; impl pins gemm256 | "
        "halo_mfma ('' = conv_fwd_pool_impl's answer)",
        py::arg("x"), py::arg("w"), py::arg("b"), py::arg("stride"),
        py::arg("pad"), py::arg("max_blocks") = 0, py::arg("impl") = "");
  m.def("conv_fwd_pool_impl", &bflc::conv_fwd_pool_impl,
        "what the gemm256_pool route launches: halo_mfma | gemm256",
        py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"),
        py::arg("pad"));
  m.def("halo_conv_group_images", &bflc::halo_conv_group_images_query,
        "images per LDS group of the halo kernel (0: not its geometry)",
        py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"),
        py::arg("pad"));
  m.def("conv_relu_pool_stack_fwd", &bflc::conv_relu_pool_stack_fwd,
        "grad-free conv3x3 + ReLU + pool twice (stride 1, pad 1): "
        "[N, H/4, W/4, Kout2]. impl pins two_call | halo_stack (geometry "
        "only; '' = conv_relu_pool_stack_route's answer); max_blocks > 0 "
        "caps the halo kernels' grids",
        py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
        py::arg("b2"), py::arg("max_blocks") = 0, py::arg("impl") = "");
  m.def("conv_relu_pool_stack_route", &bflc::conv_relu_pool_stack_route,
        "what conv_relu_pool_stack_fwd runs: halo_stack | two_call",
        py::arg("x_shape"), py::arg("w1_shape"), py::arg("w2_shape"));
  m.def("halo_stack_group_images", &bflc::halo_stack_group_images_query,
        "images per LDS group of the stack kernel (0: not its geometry)",
        py::arg("x_shape"), py::arg("w1_shape"), py::arg("w2_shape"));
  m.def("conv2d_relu_pool_route", &bflc::conv2d_relu_pool_route,
        "route conv2d_relu_pool_fwd takes: gemm256_pool | thin_pool | "
        "unfused",
        py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"),
        py::arg("pad"));
  m.def("conv2d_relu_pool_fwd_idx", &bflc::conv2d_relu_pool_fwd_idx,
        "training conv + bias + ReLU + 2x2/2 maxpool: (y_pooled, idx), "
        "same routes and options as conv2d_relu_pool_fwd",
        py::arg("x"), py::arg("w"), py::arg("b"), py::arg("stride"),
        py::arg("pad"), py::arg("max_blocks") = 0, py::arg("impl") = "");
  m.def("pool_relu_bwd_colsum", &bflc::pool_relu_bwd_colsum,
        "unpool + ReLU mask + bias grad in one pass: (dy_full_masked, db)",
        py::arg("y_pooled"), py::arg("idx"), py::arg("dy_pooled"),
        py::arg("out_shape"));
  m.def("thin_conv_pool_wgrad", &bflc::thin_conv_pool_wgrad,
        "direct first-layer (dw, db) from the pooled tensors",
        py::arg("x"), py::arg("y_pooled"), py::arg("idx"),
        py::arg("dy_pooled"), py::arg("stride"), py::arg("pad"));
  m.def("thin_conv_pool_wgrad_fused", &bflc::thin_conv_pool_wgrad_fused,
        "first-layer (dw, db) from the pooled tensors, bitwise the "
        "materialised unpool -> im2col -> split-K GEMM chain",
        py::arg("x"), py::arg("y_pooled"), py::arg("idx"),
        py::arg("dy_pooled"), py::arg("stride"), py::arg("pad"));
  m.def("thin_pool_wgrad_impl", &bflc::thin_pool_wgrad_impl,
        "what the unpool route runs for the thin first layer: "
        "fused_mfma | materialized",
        py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"),
        py::arg("pad"), py::arg("want_dx"));
  m.def("conv2d_relu_pool_bwd_route", &bflc::conv2d_relu_pool_bwd_route,
        "route conv2d_relu_pool_bwd takes: thin_direct | unpool",
        py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"),
        py::arg("pad"), py::arg("want_dx"), py::arg("allow_direct") = true);
  m.def("conv2d_relu_pool_bwd", &bflc::conv2d_relu_pool_bwd,
        "(dx, dw, db) of the fused conv + ReLU + pool from its saved "
        "(x, w, y_pooled, idx). dgrad_impl pins halo_mfma | implicit_gemm "
        "('' = pool_dgrad_impl's answer); max_blocks > 0 caps the halo "
        "kernel's grid",
        py::arg("x"), py::arg("w"), py::arg("y_pooled"), py::arg("idx"),
        py::arg("dy_pooled"), py::arg("stride"), py::arg("pad"),
        py::arg("want_db") = true, py::arg("want_dx") = true,
        py::arg("allow_direct") = true, py::arg("dgrad_impl") = "",
        py::arg("max_blocks") = 0);
  m.def("pool_dgrad_impl", &bflc::pool_dgrad_impl,
        "data gradient the unpool route runs: halo_mfma | implicit_gemm",
        py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"),
        py::arg("pad"), py::arg("want_dx"));
  m.def("halo_dgrad_group_images", &bflc::halo_dgrad_group_images_query,
        "images per LDS group of the halo dgrad kernel (0: not its "
        "geometry)",
        py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"),
        py::arg("pad"));
  m.def("halo_pool_dgrad", &bflc::halo_pool_dgrad,
        "the halo dgrad kernel on its geometry alone: (dx, masked "
        "full-resolution dy plane) from w and the pooled (y, idx, dy); "
        "store_plane = false skips the plane store (0-size plane)",
        py::arg("w"), py::arg("y_pooled"), py::arg("idx"),
        py::arg("dy_pooled"), py::arg("max_blocks") = 0,
        py::arg("store_plane") = true);
  m.def("batchnorm_fwd", &bflc::batchnorm_fwd,
        py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("eps"),
        py::arg("relu"), py::arg("residual") = py::none(),
        "(y, mean, invstd) — batch-stats BN, optional fused relu");
  m.def("batchnorm_bwd", &bflc::batchnorm_bwd, "(dx, dgamma, dbeta)",
        py::arg("x"), py::arg("dy"), py::arg("mean"), py::arg("invstd"),
        py::arg("gamma"), py::arg("y_relu") = py::none());
  m.def("global_avgpool_fwd", &bflc::global_avgpool_fwd);
  m.def("global_avgpool_bwd", &bflc::global_avgpool_bwd);
  m.def("add_relu_fwd", &bflc::add_relu_fwd, "fused residual add + relu");
  m.def("add_relu_bwd", &bflc::add_relu_bwd);
  m.def("groupnorm_fwd", &bflc::groupnorm_fwd,
        py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("groups"),
        py::arg("eps"), py::arg("relu"), py::arg("residual") = py::none(),
        "(y, mean [N,G], rstd [N,G]) — per-sample GroupNorm, optional "
        "fused residual add + relu");
  m.def("groupnorm_bwd", &bflc::groupnorm_bwd, "(dx, dgamma, dbeta)",
        py::arg("x"), py::arg("dy"), py::arg("mean"), py::arg("rstd"),
        py::arg("gamma"), py::arg("groups"), py::arg("y_relu") = py::none());
  m.def("groupnorm_route", &bflc::groupnorm_route,
        "route groupnorm_fwd/bwd take: slab | split (from H, W, C, groups "
        "only — never N)",
        py::arg("H"), py::arg("W"), py::arg("C"), py::arg("groups"));
}
