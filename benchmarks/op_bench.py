#!/usr/bin/env python3
"""Per-op timing sweep over the FL models' exact hot shapes.

Times each framework op (conv fwd/bwd, BN fwd/bwd, pool, the GEMM
shapes) with CUDA events and prints one JSON blob — a finer-grained
regression harness than rocprof kernel stats (which mix call sites):
run it before and after a kernel change and diff the per-shape numbers.

    python benchmarks/op_bench.py [--iters 50] \
        [--only conv,score,train,gemm,norm,optim]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bflc_amd.ops import functional as O


def timeit(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us


# (name, N, H, C, Kout, R, stride, pad) — the conv layers of the three
# image models at their bench batch sizes
CONVS = [
    ("fe.conv1", 1024, 28, 1, 32, 3, 1, 1),
    ("fe.conv2", 1024, 14, 32, 64, 3, 1, 1),
    ("r20.stem", 512, 32, 3, 16, 3, 1, 1),
    ("r20.b1", 512, 32, 16, 16, 3, 1, 1),
    ("r20.b2dn", 512, 32, 16, 32, 3, 2, 1),
    ("r20.b2", 512, 16, 32, 32, 3, 1, 1),
    ("r20.b3dn", 512, 16, 32, 64, 3, 2, 1),
    ("r20.b3", 512, 8, 64, 64, 3, 1, 1),
    ("r50.stem", 64, 224, 3, 64, 7, 2, 3),
    ("r50.c2.1x1", 64, 56, 64, 64, 1, 1, 0),
    ("r50.c2.3x3", 64, 56, 64, 64, 3, 1, 1),
    ("r50.c2.out", 64, 56, 64, 256, 1, 1, 0),
    ("r50.c3.3x3", 64, 28, 128, 128, 3, 1, 1),
    ("r50.c4.3x3", 64, 14, 256, 256, 3, 1, 1),
    ("r50.c5.3x3", 64, 7, 512, 512, 3, 1, 1),
]

# grad-free scoring forwards: one accuracy_t call pushes a scorer's
# whole 3072-sample shard through the conv stack
SCORE_CONVS = [
    ("fe.conv1", 3072, 28, 1, 32, 3, 1, 1),
    ("fe.conv2", 3072, 14, 32, 64, 3, 1, 1),
]

# training steps: the two FEMNIST conv stages at the trainer batch
# (4 trainers x 3 batches of 1024 per protocol round); the first stage
# takes no input gradient
TRAIN_CONVS = [
    ("fe.conv1", 1024, 28, 1, 32, 3, 1, 1, False),
    ("fe.conv2", 1024, 14, 32, 64, 3, 1, 1, True),
]

# (name, M, K, N) GEMMs (linear layers + eval shapes)
GEMMS = [
    ("fe.fc1", 1024, 3136, 128),
    ("fe.fc2", 1024, 128, 62),
    ("r50.fc", 64, 2048, 1000),
    ("sq.2048", 2048, 2048, 2048),
]

# (name, N, H, C, groups) normalisation inputs: the ResNet-20 stages at
# batch 512, ResNet-50 layers at batch 64, and two shapes around the
# GroupNorm slab/split threshold (64 KiB and 128 KiB per sample)
NORMS = [
    ("r20.s1", 512, 32, 16, 8),
    ("r20.s2", 512, 16, 32, 8),
    ("r20.s3", 512, 8, 64, 8),
    ("r50.stem", 64, 112, 64, 32),
    ("r50.c2", 64, 56, 64, 32),
    ("r50.c2.out", 64, 56, 256, 32),
    ("r50.c3.out", 64, 28, 512, 32),
    ("r50.c4.out", 64, 14, 1024, 32),
    ("r50.c5", 64, 7, 512, 32),
    ("r50.c5.out", 64, 7, 2048, 32),
    ("thr.64k", 256, 32, 32, 8),
    ("thr.128k", 256, 32, 64, 8),
]

# (name, P) flat master sizes of the fused optimizer steps: FEMNIST CNN,
# ResNet-20, ResNet-50
OPTIMS = [("fe", 421_000), ("r20", 272_000), ("r50", 25_600_000)]

COPY_BW = 6.29e12  # measured device copy bandwidth, bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default="conv,score,train,gemm,norm,optim",
                    help="comma-separated sections to run")
    args = ap.parse_args()
    only = set(args.only.split(","))
    assert torch.cuda.is_available(), "op_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    out = {}

    for name, n, h, c, k, r, stride, pad in (CONVS if "conv" in only else []):
        x = torch.randn(n, h, h, c, device=dev, dtype=torch.bfloat16)
        w = torch.randn(k, r, r, c, device=dev, dtype=torch.bfloat16) * 0.05
        b = torch.randn(k, device=dev, dtype=torch.bfloat16)
        h_ops = O.hip_ops()
        y, col, _, _ = h_ops.conv2d_fwd_bn(x, w, stride, pad)
        dy = torch.randn_like(y)
        col_arg = col if col.numel() else None
        out[f"conv.{name}.fwd"] = timeit(
            lambda: h_ops.conv2d_fwd_col(x, w, b, stride, pad, False,
                                         True), args.iters)
        out[f"conv.{name}.fwd_eval"] = timeit(
            lambda: h_ops.conv2d_fwd(x, w, b, stride, pad), args.iters)
        out[f"conv.{name}.bwd"] = timeit(
            lambda: h_ops.conv2d_bwd(x, w, dy, stride, pad, col_arg),
            args.iters)
        if k % 8 == 0:
            g = torch.rand(k, device=dev, dtype=torch.bfloat16) + 0.5
            be = torch.randn(k, device=dev, dtype=torch.bfloat16)
            yb, mean, invstd = h_ops.batchnorm_fwd(y, g, be, 1e-5, True,
                                                   None)
            out[f"bn.{name}.fwd"] = timeit(
                lambda: h_ops.batchnorm_fwd(y, g, be, 1e-5, True, None),
                args.iters)
            out[f"bn.{name}.bwd"] = timeit(
                lambda: h_ops.batchnorm_bwd(y, dy, mean, invstd, g, yb),
                args.iters)

    # committee-scoring forwards: conv + ReLU + 2x2 pool, fused in the
    # conv epilogue vs the two kernels it replaces (bitwise equal)
    for name, n, h, c, k, r, stride, pad in (SCORE_CONVS if "score" in only
                                             else []):
        x = torch.randn(n, h, h, c, device=dev, dtype=torch.bfloat16)
        w = torch.randn(k, r, r, c, device=dev, dtype=torch.bfloat16) * 0.05
        b = torch.randn(k, device=dev, dtype=torch.bfloat16)
        h_ops = O.hip_ops()
        out[f"score.{name}.route"] = h_ops.conv2d_relu_pool_route(
            list(x.shape), list(w.shape), stride, pad)
        out[f"score.{name}.conv_relu"] = timeit(
            lambda: h_ops.conv2d_fwd(x, w, b, stride, pad, True), args.iters)
        out[f"score.{name}.conv_relu+pool"] = timeit(
            lambda: h_ops.maxpool2d_fwd(
                h_ops.conv2d_fwd(x, w, b, stride, pad, True), 2, 2, False),
            args.iters)
        out[f"score.{name}.fused"] = timeit(
            lambda: h_ops.conv2d_relu_pool_fwd(x, w, b, stride, pad),
            args.iters)
        # what the gemm256_pool route launches (BFLC_HALO_CONV), next to
        # both of its implementations pinned
        impl = h_ops.conv_fwd_pool_impl(list(x.shape), list(w.shape), stride,
                                        pad)
        out[f"score.{name}.fused_impl"] = impl
        if impl == "halo_mfma":
            out[f"score.{name}.fused_gemm256"] = timeit(
                lambda: h_ops.conv2d_relu_pool_fwd(x, w, b, stride, pad, 0,
                                                   "gemm256"), args.iters)
            out[f"score.{name}.fused_halo_mfma"] = timeit(
                lambda: h_ops.conv2d_relu_pool_fwd(x, w, b, stride, pad, 0,
                                                   "halo_mfma"), args.iters)

    # the grad-free stack at the scoring shard: the two fused calls
    # (thin conv1 then halo conv2) vs the one kernel that computes
    # conv2's input in LDS (bitwise equal), both pinned, and the default
    # route. score.fe.conv1.fused above is conv1's pooled forward alone.
    if "score" in only:
        h_ops = O.hip_ops()
        n = SCORE_CONVS[0][1]
        x = torch.randn(n, 28, 28, 1, device=dev, dtype=torch.bfloat16)
        w1 = torch.randn(32, 3, 3, 1, device=dev, dtype=torch.bfloat16) * 0.3
        b1 = torch.randn(32, device=dev, dtype=torch.bfloat16)
        w2 = torch.randn(64, 3, 3, 32, device=dev, dtype=torch.bfloat16) * .05
        b2 = torch.randn(64, device=dev, dtype=torch.bfloat16)
        out["score.fe.stack.route"] = h_ops.conv_relu_pool_stack_route(
            list(x.shape), list(w1.shape), list(w2.shape))
        for impl in ("two_call", "halo_stack", ""):
            out[f"score.fe.stack.{impl or 'default'}"] = timeit(
                lambda: h_ops.conv_relu_pool_stack_fwd(x, w1, b1, w2, b2, 0,
                                                       impl), args.iters)
        # bytes the stack has to move: pixels in, pooled output out
        need = n * 28 * 28 * 2 + n * 7 * 7 * 64 * 2
        out["score.fe.stack.halo_stack_necessary_GBps"] = (
            need / out["score.fe.stack.halo_stack"] / 1e3)

    # training conv + ReLU + 2x2 pool stages: the two-op forward (conv
    # writes the full plane, pool reads it back) vs the fused one that
    # also emits the argmax plane, and the old backward chain (unpool,
    # relu mask + db, conv backward) vs the pooled backward entry
    for name, n, h, c, k, r, stride, pad, want_dx in (
            TRAIN_CONVS if "train" in only else []):
        x = torch.randn(n, h, h, c, device=dev, dtype=torch.bfloat16)
        w = torch.randn(k, r, r, c, device=dev, dtype=torch.bfloat16) * 0.05
        b = torch.randn(k, device=dev, dtype=torch.bfloat16) * 0.1
        h_ops = O.hip_ops()
        out[f"train.{name}.fwd_route"] = h_ops.conv2d_relu_pool_route(
            list(x.shape), list(w.shape), stride, pad)
        out[f"train.{name}.bwd_route"] = h_ops.conv2d_relu_pool_bwd_route(
            list(x.shape), list(w.shape), stride, pad, want_dx, False)
        out[f"train.{name}.bwd_route_direct_allowed"] = \
            h_ops.conv2d_relu_pool_bwd_route(
                list(x.shape), list(w.shape), stride, pad, want_dx, True)
        out[f"train.{name}.fwd_two_op"] = timeit(
            lambda: h_ops.maxpool2d_fwd(
                h_ops.conv2d_fwd_col(x, w, b, stride, pad, True, False)[0],
                2, 2, True), args.iters)
        out[f"train.{name}.fwd_fused_idx"] = timeit(
            lambda: h_ops.conv2d_relu_pool_fwd_idx(x, w, b, stride, pad),
            args.iters)
        impl = h_ops.conv_fwd_pool_impl(list(x.shape), list(w.shape), stride,
                                        pad)
        out[f"train.{name}.fwd_fused_impl"] = impl
        if impl == "halo_mfma":
            out[f"train.{name}.fwd_fused_idx_gemm256"] = timeit(
                lambda: h_ops.conv2d_relu_pool_fwd_idx(x, w, b, stride, pad,
                                                       0, "gemm256"),
                args.iters)
            out[f"train.{name}.fwd_fused_idx_halo_mfma"] = timeit(
                lambda: h_ops.conv2d_relu_pool_fwd_idx(x, w, b, stride, pad,
                                                       0, "halo_mfma"),
                args.iters)
        yfull = h_ops.conv2d_fwd(x, w, b, stride, pad, True)
        yp, idx = h_ops.maxpool2d_fwd(yfull, 2, 2, True)
        dy = torch.randn_like(yp)
        full = list(yfull.shape)

        def old_chain():
            dyf = h_ops.maxpool2d_bwd(dy, idx, full, 2, 2)
            dym, db = h_ops.relu_bwd_colsum(yfull, dyf)
            return h_ops.conv2d_bwd(x, w, dym, stride, pad, None, False,
                                    want_dx)

        out[f"train.{name}.bwd_old_chain"] = timeit(old_chain, args.iters)
        out[f"train.{name}.bwd_pooled"] = timeit(
            lambda: h_ops.conv2d_relu_pool_bwd(x, w, yp, idx, dy, stride,
                                               pad, True, want_dx, False),
            args.iters)
        out[f"train.{name}.bwd_pooled_direct_allowed"] = timeit(
            lambda: h_ops.conv2d_relu_pool_bwd(x, w, yp, idx, dy, stride,
                                               pad, True, want_dx, True),
            args.iters)
        out[f"train.{name}.unpool_relu_colsum"] = timeit(
            lambda: h_ops.pool_relu_bwd_colsum(yp, idx, dy, full),
            args.iters)
        # what bwd_pooled runs underneath for a thin first layer
        # (BFLC_THIN_FUSED_WGRAD), next to both of its implementations
        out[f"train.{name}.bwd_pooled_impl"] = h_ops.thin_pool_wgrad_impl(
            list(x.shape), list(w.shape), stride, pad, want_dx)

        def materialized_chain():
            dyf, db = h_ops.pool_relu_bwd_colsum(yp, idx, dy, full)
            return h_ops.conv2d_bwd(x, w, dyf, stride, pad, None, False,
                                    want_dx)

        out[f"train.{name}.bwd_materialized_chain"] = timeit(
            materialized_chain, args.iters)
        # the data gradient bwd_pooled runs (BFLC_HALO_DGRAD), next to
        # both of its implementations pinned and the halo kernel alone
        dimpl = h_ops.pool_dgrad_impl(list(x.shape), list(w.shape), stride,
                                      pad, want_dx)
        out[f"train.{name}.bwd_pooled_dgrad_impl"] = dimpl
        if dimpl == "halo_mfma":
            for pin in ("implicit_gemm", "halo_mfma"):
                out[f"train.{name}.bwd_pooled_dgrad_{pin}"] = timeit(
                    lambda: h_ops.conv2d_relu_pool_bwd(
                        x, w, yp, idx, dy, stride, pad, True, want_dx, False,
                        pin), args.iters)
            out[f"train.{name}.halo_pool_dgrad"] = timeit(
                lambda: h_ops.halo_pool_dgrad(w, yp, idx, dy), args.iters)
            # the plane store's cost, against unpool_relu_colsum above as
            # the other plane producer
            out[f"train.{name}.halo_pool_dgrad_no_plane"] = timeit(
                lambda: h_ops.halo_pool_dgrad(w, yp, idx, dy, 0, False),
                args.iters)
        if not want_dx:
            out[f"train.{name}.thin_fused_wgrad"] = timeit(
                lambda: h_ops.thin_conv_pool_wgrad_fused(x, yp, idx, dy,
                                                         stride, pad),
                args.iters)
            out[f"train.{name}.thin_direct_wgrad"] = timeit(
                lambda: h_ops.thin_conv_pool_wgrad(x, yp, idx, dy, stride,
                                                   pad), args.iters)

    for name, m, k, n in (GEMMS if "gemm" in only else []):
        x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
        w = torch.randn(k, n, device=dev, dtype=torch.bfloat16)
        b = torch.randn(n, device=dev, dtype=torch.bfloat16)
        dy = torch.randn(m, n, device=dev, dtype=torch.bfloat16)
        h_ops = O.hip_ops()
        out[f"gemm.{name}.fwd"] = timeit(
            lambda: h_ops.linear_fwd(x, w, b, False), args.iters)
        out[f"gemm.{name}.bwd"] = timeit(
            lambda: h_ops.linear_bwd(x, w, dy), args.iters)

    # normalisation layers at the ResNet hot shapes: GroupNorm forward /
    # backward on every legal route (BFLC_GN_ROUTE pins it), next to the
    # BN kernels at the same shape — the standalone stats + norm pair
    # and batchnorm_bwd. The thr.* rows sit on either side of the
    # slab/split threshold (64 KiB per sample).
    for name, n, h, c, groups in (NORMS if "norm" in only else []):
        h_ops = O.hip_ops()
        x = torch.randn(n, h, h, c, device=dev, dtype=torch.bfloat16)
        dy = torch.randn_like(x)
        g = torch.rand(c, device=dev, dtype=torch.bfloat16) + 0.5
        be = torch.randn(c, device=dev, dtype=torch.bfloat16)
        tensor_bytes = x.numel() * 2

        def bn_pair():
            mean, invstd = h_ops.bn_stats(x, 1e-5)
            return h_ops.batchnorm_norm(x, g, be, mean, invstd, True, None)

        yb, mean, invstd = h_ops.batchnorm_fwd(x, g, be, 1e-5, True, None)
        out[f"norm.{name}.bn.fwd_stats+norm"] = timeit(bn_pair, args.iters)
        out[f"norm.{name}.bn.bwd"] = timeit(
            lambda: h_ops.batchnorm_bwd(x, dy, mean, invstd, g, yb),
            args.iters)
        saved = os.environ.pop("BFLC_GN_ROUTE", None)
        out[f"norm.{name}.gn.route"] = h_ops.groupnorm_route(h, h, c, groups)
        for route in ("slab", "split"):
            os.environ["BFLC_GN_ROUTE"] = route
            if h_ops.groupnorm_route(h, h, c, groups) != route:
                continue  # slab is not legal at this shape
            yg, gm, gr = h_ops.groupnorm_fwd(x, g, be, groups, 1e-5, True)
            t_f = timeit(lambda: h_ops.groupnorm_fwd(x, g, be, groups, 1e-5,
                                                     True), args.iters)
            t_b = timeit(lambda: h_ops.groupnorm_bwd(x, dy, gm, gr, g,
                                                     groups, yg), args.iters)
            out[f"norm.{name}.gn.{route}.fwd"] = t_f
            out[f"norm.{name}.gn.{route}.bwd"] = t_b
            # whole-op traffic floor: fwd reads x, writes y (2 tensor
            # passes); bwd reads x, dy, y and writes dx (4)
            out[f"norm.{name}.gn.{route}.fwd_frac_copy_bw"] = \
                2 * tensor_bytes / (t_f * 1e-6) / COPY_BW
            out[f"norm.{name}.gn.{route}.bwd_frac_copy_bw"] = \
                4 * tensor_bytes / (t_b * 1e-6) / COPY_BW
        os.environ.pop("BFLC_GN_ROUTE", None)
        if saved is not None:
            os.environ["BFLC_GN_ROUTE"] = saved

    # fused master-weight steps: the legacy sgd_master_ (12 B/element:
    # p read + write, bf16 g read, bf16 shadow write), the extended
    # sgdm step (+8 B with momentum, +4 B with the proximal term) and
    # the clip pair (one 2 B/element pass + a one-block final)
    for name, n in (OPTIMS if "optim" in only else []):
        h_ops = O.hip_ops()
        p = torch.randn(n, device=dev)
        sh = p.to(torch.bfloat16)
        g = (torch.randn(n, device=dev) * 1e-3).to(torch.bfloat16)
        buf = torch.zeros(n, device=dev)
        p0 = p.clone()
        one = torch.zeros(1, device=dev)
        lr_dev = torch.full((1,), 1e-6, device=dev)
        coef = torch.ones(2, device=dev)
        rows = [
            ("sgd_master_", 12, lambda: h_ops.sgd_master_(p, sh, g, 1e-6)),
            ("sgdm.plain", 12, lambda: O.sgdm_step_(
                p, sh, g, one, one, lr_dev, coef, 0.0, False, 0.0, 0.0)),
            ("sgdm.mom", 20, lambda: O.sgdm_step_(
                p, sh, g, buf, one, lr_dev, coef, 0.9, False, 0.0, 0.0)),
            ("sgdm.mom_nest_wd", 20, lambda: O.sgdm_step_(
                p, sh, g, buf, one, lr_dev, coef, 0.9, True, 1e-4, 0.0)),
            ("sgdm.mom_nest_wd_prox", 24, lambda: O.sgdm_step_(
                p, sh, g, buf, p0, lr_dev, coef, 0.9, True, 1e-4, 0.01)),
            ("clip_coef_pair", 2, lambda: O.grad_clip_coef_(g, 1.0, coef)),
        ]
        for tag, bytes_per, fn in rows:
            t = timeit(fn, args.iters)
            out[f"optim.{name}.{tag}"] = t
            out[f"optim.{name}.{tag}.GBps"] = bytes_per * n / (t * 1e-6) / 1e9
        coef.fill_(1.0)

    print(json.dumps({"unit": "us_per_call", "ops": out}, indent=1))


if __name__ == "__main__":
    main()
